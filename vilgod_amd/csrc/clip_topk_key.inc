// The order of the top-k class selection (csrc/clip_topk.hip), `__host__ __device__`: the kernel and vg_clip_topk_host run the SAME
// text, so the device and the host pick the same classes in the same order.
//
//   clip_topk_before   does (pa, class ia) stand before (pb, class ib)?  The strict total order: probability descending, class index
//                      ascending; -0.0 and +0.0 are one probability; a NaN stands behind every number, NaNs among themselves by index.
//
// Integer comparisons on the float's bits only (sign-magnitude -> two's complement, NaN -> the lowest key): the answer does not
// depend on a floating-point mode (denormals are numbers like any other), and for two numbers it is the `>` / `==` of the top-1
// comparator of k_clip_scores / k_clip_scores_wide ("greater, or equal and the lower index").
#pragma once
#include <stdint.h>

#ifndef VG_HD
#define VG_HD __host__ __device__ __forceinline__
#endif

#define CLIP_TOPK_NONE 0x7fffffff          // the class index of "no candidate": with a NaN it stands behind every real entry

VG_HD bool clip_topk_before(float pa, int ia, float pb, int ib) {
    const uint32_t ua = __builtin_bit_cast(uint32_t, pa), ub = __builtin_bit_cast(uint32_t, pb);
    const uint32_t ma = ua & 0x7fffffffu, mb = ub & 0x7fffffffu;
    const int32_t ka = ma > 0x7f800000u ? INT32_MIN : ((ua >> 31) ? -(int32_t)ma : (int32_t)ma);
    const int32_t kb = mb > 0x7f800000u ? INT32_MIN : ((ub >> 31) ? -(int32_t)mb : (int32_t)mb);
    return ka > kb || (ka == kb && ia < ib);
}
