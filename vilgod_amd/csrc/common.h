// Shared helpers for the gfx950 kernels of libvilgod_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define VG_OK 0
#define VG_ERR_ARG 1
#define VG_ERR_HIP 2
#define VG_ERR_CAPACITY 3

#define VG_CHECK(expr)                                                                      \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            fprintf(stderr, "[vilgod_hip] %s:%d %s -> %s\n", __FILE__, __LINE__, #expr,     \
                    hipGetErrorString(_e));                                                 \
            return VG_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

#define VG_LAUNCH_CHECK() VG_CHECK(hipGetLastError())

static inline int vg_div_up(int a, int b) { return (a + b - 1) / b; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, DEVICE): the attribute belongs to the device's code object, so a
// process-wide `static bool` would leave a second device of the process without it (its launches with > 64 KB of dynamic LDS fail).
// One bit per device in an atomic word; setting it twice is harmless, so racing threads need no lock.
#include <atomic>
struct VgPerDeviceOnce { std::atomic<unsigned long long> done{0}; };
static inline int vg_max_dynamic_lds(const void* kernel, int bytes, VgPerDeviceOnce& once) {
    int dev = 0;
    VG_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (once.done.load(std::memory_order_acquire) & bit) return VG_OK;
    VG_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    once.done.fetch_or(bit, std::memory_order_release);
    return VG_OK;
}
#define VG_MAX_DYNAMIC_LDS(kernel, bytes)                                                   \
    do {                                                                                    \
        static VgPerDeviceOnce _once;                                                       \
        const int _rc = vg_max_dynamic_lds((const void*)(kernel), (int)(bytes), _once);    \
        if (_rc != VG_OK) return _rc;                                                       \
    } while (0)

#define WAVE 64

// order-preserving float <-> uint key (for radix select / atomic min-max on signed floats)
__device__ __forceinline__ uint32_t vg_fkey(float f) {
    uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float vg_fkey_inv(uint32_t k) {
    uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    return __uint_as_float(b);
}

// Wave reductions (xor butterfly: every lane ends with the result) for float, double and int.  min / max of finite values do not depend
// on the combine order; a sum does, and callers whose bits are pinned rely on this butterfly.
__device__ __forceinline__ float vg_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float vg_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double vg_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double vg_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ int vg_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int vg_max(int a, int b) { return a > b ? a : b; }
template <typename T>
__device__ __forceinline__ T vg_wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = vg_max(v, __shfl_xor(v, o));
    return v;
}
template <typename T>
__device__ __forceinline__ T vg_wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = vg_min(v, __shfl_xor(v, o));
    return v;
}
template <typename T>
__device__ __forceinline__ T vg_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A value every lane of the wave holds, moved to scalar registers: it then costs no vector register while it stays live
__device__ __forceinline__ int vg_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float vg_uniform(float v) { return __int_as_float(vg_uniform(__float_as_int(v))); }
__device__ __forceinline__ double vg_uniform(double v) {
    return __hiloint2double(vg_uniform(__double2hiint(v)), vg_uniform(__double2loint(v)));
}

// Four-wave (256-thread) block reductions through a caller-provided LDS array slot[4].  vg_block_put is called with a wave-reduced
// value; behind the CALLER's barrier every thread combines the four slots: one barrier serves any number of slots, and the next put
// into a slot needs a barrier behind its last read.  The sum is (w0 + w1) + (w2 + w3).
template <typename T>
__device__ __forceinline__ void vg_block_put(T* slot, T v) {
    if ((threadIdx.x & 63) == 0) slot[(threadIdx.x >> 6) & 3] = v;
}
template <typename T>
__device__ __forceinline__ T vg_block_min(const T* slot) { return vg_min(vg_min(slot[0], slot[1]), vg_min(slot[2], slot[3])); }
template <typename T>
__device__ __forceinline__ T vg_block_max(const T* slot) { return vg_max(vg_max(slot[0], slot[1]), vg_max(slot[2], slot[3])); }
template <typename T>
__device__ __forceinline__ T vg_block_sum(const T* slot) { return (slot[0] + slot[1]) + (slot[2] + slot[3]); }

// The extent pass over one cluster (points pts[idx[i] * stride], i < n) by a 256-thread workgroup: the float32 extent of the last
// NAX coordinates (1: z; 3: x, y, z) and, for PLANE, the extremes of the signed float64 distance to plane = {a, b, c, d}.  Every
// thread returns the result, in scalar registers (vg_uniform: a caller keeps it live across its later phases; left in vector
// registers it took k_cluster_filter_ex from 4 to 3 waves per SIMD).  fslot is [2 * NAX][4], dslot [2][4] (unused without PLANE);
// one barrier, behind the puts.  An empty cluster gives the reductions' identities (+inf / -inf).
struct VgExtent { float lo[3], hi[3]; double dmin, dmax; };
__device__ __forceinline__ double vg_plane_distance(const double* __restrict__ plane, double inv, const float* __restrict__ p) {
    return (((plane[0] * (double)p[0] + plane[1] * (double)p[1]) + plane[2] * (double)p[2]) + plane[3]) / inv;
}
__device__ __forceinline__ double vg_plane_norm(const double* __restrict__ plane) {
    return sqrt((plane[0] * plane[0] + plane[1] * plane[1]) + plane[2] * plane[2]);
}
template <int NAX, bool PLANE>
__device__ __forceinline__ VgExtent vg_cluster_extent(const float* __restrict__ pts, int stride, const int* __restrict__ idx, int n,
                                                      const double* __restrict__ plane, float (*fslot)[4], double (*dslot)[4]) {
    VgExtent e;
    const double inv = PLANE ? vg_plane_norm(plane) : 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { e.lo[a] = INFINITY; e.hi[a] = -INFINITY; }
    e.dmin = INFINITY; e.dmax = -INFINITY;
#pragma unroll 4                                       // (the gathers of four points in flight: the pass waits on memory, not on arithmetic)
    for (int i = threadIdx.x; i < n; i += 256) {
        const float* p = pts + (size_t)idx[i] * stride;
#pragma unroll
        for (int a = 3 - NAX; a < 3; ++a) { e.lo[a] = fminf(e.lo[a], p[a]); e.hi[a] = fmaxf(e.hi[a], p[a]); }
        if (PLANE) {
            const double dist = vg_plane_distance(plane, inv, p);
            e.dmin = fmin(e.dmin, dist);
            e.dmax = fmax(e.dmax, dist);
        }
    }
#pragma unroll
    for (int j = 0, a = 3 - NAX; j < NAX; ++j, ++a) {
        vg_block_put(fslot[2 * j], vg_wave_min(e.lo[a]));
        vg_block_put(fslot[2 * j + 1], vg_wave_max(e.hi[a]));
    }
    if (PLANE) { vg_block_put(dslot[0], vg_wave_min(e.dmin)); vg_block_put(dslot[1], vg_wave_max(e.dmax)); }
    __syncthreads();
#pragma unroll
    for (int j = 0, a = 3 - NAX; j < NAX; ++j, ++a) {
        e.lo[a] = vg_uniform(vg_block_min(fslot[2 * j]));
        e.hi[a] = vg_uniform(vg_block_max(fslot[2 * j + 1]));
    }
    if (PLANE) { e.dmin = vg_uniform(vg_block_min(dslot[0])); e.dmax = vg_uniform(vg_block_max(dslot[1])); }
    return e;
}

// Which of the 256 bins of `hist` holds rank k (0-based)?  Called by 256 threads (t = 0 .. 255: four whole waves) behind the barrier
// that completes the histogram.  Exclusive prefix of the counts by wave scans (a serial walk by one thread cost ~16 k cycles per pass);
// exactly one thread finds excl <= k < excl + count and writes sh[0] = the bin, sh[1] = the number of keys in the bins below it.
// sh[2..5] hold the wave totals.  One barrier inside; the callers put another in front of reading sh[0..1].
__device__ __forceinline__ void vg_rank_bin(const uint32_t* hist, uint32_t* sh, int t, int k) {
    const uint32_t cnt = hist[t];
    uint32_t inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if ((t & 63) >= o) inc += up;
    }
    if ((t & 63) == 63) sh[2 + (t >> 6)] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < (t >> 6); ++w) base += sh[2 + w];
    const uint32_t excl = base + inc - cnt;
    if (excl <= (uint32_t)k && (uint32_t)k < excl + cnt) { sh[0] = (uint32_t)t; sh[1] = excl; }
}

// One wave adds its keys to a 256-bin LDS histogram: one atomic per DISTINCT bin among the wave's active lanes, not one per key (the
// keys of one cluster share their leading bytes, so per-key atomics serialise 64 adds on one bin).  Called by whole waves.
__device__ __forceinline__ void vg_hist_add_wave(uint32_t* hist, uint32_t bin, bool active) {
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
        const unsigned long long same = __ballot(active && bin == lb) & todo;
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// k-th smallest (0-based) of the n float32 values whose order-preserving keys key_of(i) returns (a staged LDS key, a gathered column,
// a column of a packed array): 4-pass byte radix select.  Called by a 256-thread GROUP of whole waves (t = 0 .. 255 inside the group)
// with the group's own hist[256] / sh[6]; n and k are uniform over the workgroup, and every group of it makes the same calls, so the
// workgroup barriers inside line up.  WAVE_ADD: the histogram add is vg_hist_add_wave, otherwise one LDS atomic per key; the select
// is the same.  vg_hist_add_wave is a serial loop, one ballot + readlane round per DISTINCT bin of the wave: it wins where a wave's
// keys fall into a few bins (pass 3 and 2 of one cluster's coordinates: the per-key atomics then serialise on one LDS word), and
// loses where they spread, up to 64 rounds per 64 keys in the low-byte passes 1 and 0.  k_cluster_medians got it in round 4 (the
// comment there); k_cluster_median, where twelve waves of one workgroup run those rounds between the same barriers, measured
// 104 -> 540 us per frame with it and keeps the per-key add.  The cause is the likely one, not profiled; the choice is per caller.
template <bool WAVE_ADD, class KeyOf>
__device__ __forceinline__ float vg_radix_select(KeyOf key_of, int n, int k, uint32_t* hist, uint32_t* sh, int t) {
    uint32_t prefix = 0;
    const int end = WAVE_ADD ? (n + 63) & ~63 : n;     // whole waves run the aggregation (ballots need every lane of the wave)
    for (int pass = 3; pass >= 0; --pass) {
        hist[t] = 0;
        __syncthreads();
        const int shift = pass * 8;
        for (int i = t; i < end; i += 256) {
            const uint32_t key = i < n ? key_of(i) : 0u;
            const bool in = i < n && (pass == 3 || (key >> (shift + 8)) == prefix);
            if (WAVE_ADD) vg_hist_add_wave(hist, (key >> shift) & 255u, in);
            else if (in) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        vg_rank_bin(hist, sh, t, k);
        __syncthreads();
        prefix = (prefix << 8) | sh[0];
        k -= (int)sh[1];
        __syncthreads();
    }
    return vg_fkey_inv(prefix);
}

// np.median of n > 0 float32 values: the upper middle value, or the float32 mean of the two middle values
template <bool WAVE_ADD, class KeyOf>
__device__ __forceinline__ float vg_median_select(KeyOf key_of, int n, uint32_t* hist, uint32_t* sh, int t) {
    const float hi = vg_radix_select<WAVE_ADD>(key_of, n, n / 2, hist, sh, t);
    return (n & 1) ? hi : (vg_radix_select<WAVE_ADD>(key_of, n, n / 2 - 1, hist, sh, t) + hi) / 2.0f;
}
