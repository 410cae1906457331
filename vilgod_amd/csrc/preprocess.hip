// CLIP's PIL preprocessing for `classification.image_size` other than 224, on gfx950.
//
// Replaces, per crop, src/vilgod/zero_shot_detector.py:405-410 (F.interpolate to image_size^2 with align_corners=True, permute,
// np.uint8(img * 255), Image.fromarray) and the Resize(224, BICUBIC) that opens third_party/CLIP/clip/clip.py:79-86, which for a
// square PIL image is Image.resize((224, 224), Image.BICUBIC): Pillow's antialiased 8-bit resample (src/libImaging/Resample.c).
// At image_size 224 that resize is the identity and k_render (render.hip) writes the crops itself; this file serves every other size.
//
//   k_clip_preprocess<K>   one 1024-thread workgroup per crop; K = 5, 7, 9 taps reserved per output pixel (image_size <= 224, <= 336, above).
//     in_kind 0: the renderer's raw (R-2)^2 float image (vg_render_crops out_kind 3) is loaded into LDS; the bilinear step is
//                k_render's, float32 op for op: fma(p00, lw0, p01 * lw1), fma(t0, lh0, t1 * lh1), scale float(G-1)/float(S-1),
//                then (int)(o * 255) truncated and clamped.  This file is compiled with -ffp-contract=off like render.hip.
//     in_kind 1: uint8 [S][S] images that are at image_size already.
//     Then PIL's two passes in integers, horizontal first: clip8((2^21 + sum pixel * k) >> 22) with the int32 tables of
//     vilgod_amd/pil_resample.py (precompute_coeffs + normalize_coeffs_8bpc; the same table serves both passes of a square image).
//     sum |k| * 255 + 2^21 < 2^31 for every size 65 .. 448 (tests/test_image_size_host.py), so the accumulator is int32.
//
// LDS.  The S x 224 horizontally resampled bytes (100 KB at 448) and the G^2 float image (63.5 KB at G = 126) do not fit the CU's 160 KB
// together, so the OUTPUT rows are banded: 7 bands of 32 rows (whole 16-row patches, which the patch-row kinds write as whole 512-byte
// rows).  A band needs the input rows its taps reach, at most ceil(32 S / 224 + 2 * support) + 2 = 74 at 448:
//   T [G][G] float (in_kind 0) | U [rows][S] uint8, the image_size rows of the band | H [rows][224] uint8, their horizontal pass |
//   O [32][224] uint8, the band's output rows
// 120 400 bytes at the largest setting, plus 15 KB of static tables.  The rows two neighbouring bands share (<= 10) are computed twice.
#include "common.h"
#include "vilgod_hip.h"
#include <hip/hip_fp16.h>

#define OUT 224          // CLIP input side
#define PT 1024          // threads per workgroup
#define BAND 32          // output rows per band
#define MAXK 9           // taps reserved per output pixel at image_size 448: ceil(2 * 448 / 224) * 2 + 1
#define MAXS VG_PREPROCESS_MAX_IMAGE_SIZE

struct PreArgs {
    const void* in;        // in_kind 0: float [n][G][G]   1: uint8 [n][S][S]
    const int* bounds;     // [224][2] first input pixel, tap count
    const int* coef;       // [224][ksize]
    const float* lut;      // [3][256] CLIP-normalised value of each uint8 level
    void* out;
    int in_kind, G, S, ksize, need, out_kind;
    int urows;             // rows U and H hold
};

__device__ __forceinline__ int clip8(int v) {
    v >>= 22;                                           // PRECISION_BITS; arithmetic shift, like Resample.c's lookup index
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// K = the taps reserved per output pixel (5, 7 or 9): the tap loops are unrolled, taps beyond a pixel's own count are zeros in registers.
// Thread layout of the passes: a thread owns one COLUMN (its tables stay in registers over all rows and bands) and every RG-th row, so a
// wave's lanes read neighbouring bytes of one row and its row index is wave-uniform (the vertical taps are one broadcast read each).
template <int K>
__global__ __launch_bounds__(PT) void k_clip_preprocess(PreArgs a) {
    extern __shared__ float lds[];
    __shared__ int s_bounds[OUT * 2];
    __shared__ int s_coef[OUT * MAXK];
    __shared__ int t_i0[MAXS];
    __shared__ float t_l0[MAXS], t_l1[MAXS];

    const int tid = threadIdx.x;
    const int G = a.G, S = a.S, need = a.need, urows = a.urows;
    const size_t crop = blockIdx.x;
    const int t_floats = a.in_kind == 0 ? G * G : 0;
    float* T = lds;
    unsigned char* U = (unsigned char*)(lds + t_floats);
    unsigned char* H = U + ((urows * S + 3) & ~3);
    unsigned char* O = H + urows * OUT;

    // the tables, made safe for any caller: every tap a pass reads lies inside the image and inside the row's `need` coefficients
    for (int i = tid; i < OUT; i += PT) {
        int lo = a.bounds[i * 2], cnt = a.bounds[i * 2 + 1];
        lo = lo < 0 ? 0 : (lo > S - 1 ? S - 1 : lo);
        cnt = cnt < 0 ? 0 : cnt;
        cnt = min(cnt, min(need, S - lo));
        s_bounds[i * 2] = lo;
        s_bounds[i * 2 + 1] = cnt;
    }
    for (int i = tid; i < OUT * need; i += PT) {
        const int xx = i / need, k = i - xx * need;
        s_coef[xx * MAXK + k] = a.coef[xx * a.ksize + k];
    }
    if (a.in_kind == 0) {
        const float* src = (const float*)a.in + crop * G * G;
        for (int i = tid; i < G * G; i += PT) T[i] = src[i];
        // F.interpolate(..., align_corners=True): src = (float(G - 1) / float(S - 1)) * dst in float32, as k_render at S = 224
        const float scale = (float)(G - 1) / (float)(S - 1);
        for (int i = tid; i < S; i += PT) {
            const float sp = scale * (float)i;
            int i0 = (int)sp;
            if (i0 > G - 1) i0 = G - 1;
            const float l1 = sp - (float)i0;
            t_i0[i] = i0;
            t_l1[i] = l1;
            t_l0[i] = 1.0f - l1;
        }
    }
    __syncthreads();

    // this thread's column of the image_size rows: 128, 256 or 512 columns wide, whichever holds S
    const int cshift = S <= 128 ? 7 : (S <= 256 ? 8 : 9);
    const int uj = tid & ((1 << cshift) - 1), urg = tid >> cshift, URG = PT >> cshift;
    int uh0 = 0, uh1 = 0;
    float ulh0 = 0.0f, ulh1 = 0.0f;
    if (a.in_kind == 0 && uj < S) {
        const int h0 = t_i0[uj];
        uh0 = h0 * G;
        uh1 = (h0 + (h0 < G - 1 ? 1 : 0)) * G;
        ulh0 = t_l0[uj];
        ulh1 = t_l1[uj];
    }
    // ... and its column of the two passes' output, 256 wide (224 used): first tap and taps of the horizontal pass
    const int xx = tid & 255, rg = tid >> 8;
    constexpr int RG = PT / 256;
    int hlo = 0, hk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) hk[k] = 0;
    if (xx < OUT) {
        hlo = s_bounds[xx * 2];
        const int cnt = s_bounds[xx * 2 + 1];
#pragma unroll
        for (int k = 0; k < K; ++k) hk[k] = k < cnt ? s_coef[xx * MAXK + k] : 0;
    }

    for (int yy0 = 0; yy0 < OUT; yy0 += BAND) {
        // input rows of this band: from the first tap of its first output row to the last tap of its last one
        const int rlo = s_bounds[yy0 * 2];
        const int rhi = s_bounds[(yy0 + BAND - 1) * 2] + s_bounds[(yy0 + BAND - 1) * 2 + 1];
        const int rows = max(0, min(rhi - rlo, urows));             // rlo + rows <= S (the bounds above)

        // ---- U: the image_size rows rlo .. rlo + rows - 1
        if (uj < S) {
            if (a.in_kind == 0) {
                // image[row i][column j] = uint8( 255 * interp[h = j][w = i] ): the H <-> W swap of permute(0, 3, 2, 1)
#pragma unroll 1
                for (int r = urg; r < rows; r += URG) {
                    const int i = rlo + r;
                    const int w0 = t_i0[i], w1 = w0 + (w0 < G - 1 ? 1 : 0);
                    const float lw0 = t_l0[i], lw1 = t_l1[i];
                    const float p00 = T[uh0 + w0], p01 = T[uh0 + w1];
                    const float p10 = T[uh1 + w0], p11 = T[uh1 + w1];
                    const float t0 = fmaf(p00, lw0, p01 * lw1);
                    const float t1 = fmaf(p10, lw0, p11 * lw1);
                    const float o = fmaf(t0, ulh0, t1 * ulh1);
                    int iv = (int)(o * 255.0f);                     // np.uint8(): truncation
                    iv = iv < 0 ? 0 : (iv > 255 ? 255 : iv);
                    U[r * S + uj] = (unsigned char)iv;
                }
            } else {
                const unsigned char* src = (const unsigned char*)a.in + (crop * S + rlo) * S;
                for (int r = urg; r < rows; r += URG) U[r * S + uj] = src[r * S + uj];
            }
        }
        __syncthreads();

        // ---- H: ImagingResampleHorizontal_8bpc of those rows.  Taps beyond a pixel's count are zeros that multiply bytes further along
        // the row, of the next row or, behind the last row, of H: inside the allocation (K - 1 bytes at most)
        if (xx < OUT) {
#pragma unroll 1
            for (int r = rg; r < rows; r += RG) {
                const unsigned char* row = U + r * S + hlo;
                int ss = 1 << 21;
#pragma unroll
                for (int k = 0; k < K; ++k) ss += (int)row[k] * hk[k];
                H[r * OUT + xx] = (unsigned char)clip8(ss);
            }
        }
        __syncthreads();

        // ---- O: ImagingResampleVertical_8bpc for the band's 32 output rows; the row is wave-uniform, its taps are broadcast reads.
        // Zero taps beyond the count read up to K - 1 rows behind the band's, inside H's tail or O.
        if (xx < OUT) {
#pragma unroll 1
            for (int yl = rg; yl < BAND; yl += RG) {
                const int yy = yy0 + yl;
                const int lo = min(max(s_bounds[yy * 2] - rlo, 0), rows), cnt = s_bounds[yy * 2 + 1];     // (in range already with PIL's own tables)
                const unsigned char* col = H + lo * OUT + xx;
                int ss = 1 << 21;
#pragma unroll
                for (int k = 0; k < K; ++k) ss += (int)col[k * OUT] * (k < cnt ? s_coef[yy * MAXK + k] : 0);
                O[yl * OUT + xx] = (unsigned char)clip8(ss);
            }
        }
        __syncthreads();

        // ---- the band's rows in the requested kind: layouts and value mappings of k_render (render.hip)
        if (a.out_kind == 0) {
            unsigned char* o8 = (unsigned char*)a.out + (crop * OUT + yy0) * OUT * 3;
#pragma unroll 1
            for (int q = tid; q < BAND * OUT * 3; q += PT) o8[q] = O[q / 3];
        } else if (a.out_kind == 1 || a.out_kind == 2) {
#pragma unroll 1
            for (int q4 = tid; q4 < BAND * OUT / 4; q4 += PT) {
                const unsigned int u4 = *(const unsigned int*)(O + q4 * 4);
                const unsigned int u[4] = {u4 & 255u, (u4 >> 8) & 255u, (u4 >> 16) & 255u, u4 >> 24};
                const size_t at = crop * 3 * OUT * OUT + (size_t)yy0 * OUT + (size_t)q4 * 4;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float* lut = a.lut + ch * 256;
                    if (a.out_kind == 1) {
                        *(float4*)((float*)a.out + at + (size_t)ch * OUT * OUT) = make_float4(lut[u[0]], lut[u[1]], lut[u[2]], lut[u[3]]);
                    } else {
                        __half2 h01 = __floats2half2_rn(lut[u[0]], lut[u[1]]);
                        __half2 h23 = __floats2half2_rn(lut[u[2]], lut[u[3]]);
                        uint2 pk;
                        pk.x = *(unsigned int*)&h01;
                        pk.y = *(unsigned int*)&h23;
                        *(uint2*)((__half*)a.out + at + (size_t)ch * OUT * OUT) = pk;
                    }
                }
            }
        } else if (a.out_kind == 4) {
            // fp16 patch rows [crop*196 + py*14 + px][ch*256 + pi*16 + pj]: the band holds patch rows py = yy0 / 16 and the next; items of
            // 4 pixels in output order, so a wave writes 512 contiguous bytes
            __half* ob = (__half*)a.out + (crop * 196 + (size_t)(yy0 / 16) * 14) * 768;
#pragma unroll 1
            for (int q = tid; q < (BAND / 16) * 14 * 192; q += PT) {
                const int pp = q / 192, rem = q - pp * 192;
                const int ch = rem >> 6, pi = (rem >> 2) & 15, pj4 = rem & 3;
                const int py = pp / 14, px = pp - py * 14;
                const unsigned int u4 = *(const unsigned int*)(O + (py * 16 + pi) * OUT + px * 16 + pj4 * 4);
                const float* lut = a.lut + ch * 256;
                __half2 h01 = __floats2half2_rn(lut[u4 & 255u], lut[(u4 >> 8) & 255u]);
                __half2 h23 = __floats2half2_rn(lut[(u4 >> 16) & 255u], lut[u4 >> 24]);
                uint2 pk;
                pk.x = *(unsigned int*)&h01;
                pk.y = *(unsigned int*)&h23;
                *(uint2*)(ob + (size_t)pp * 768 + rem * 4) = pk;
            }
        } else {
            // single-channel patch rows, level / 256: 64 items of 4 pixels per patch row, one wave instruction writes one whole 512-byte row
            __half* ob = (__half*)a.out + (crop * 196 + (size_t)(yy0 / 16) * 14) * 256;
#pragma unroll 1
            for (int q = tid; q < (BAND / 16) * 14 * 64; q += PT) {
                const int pp = q >> 6, rem = q & 63;
                const int pi = rem >> 2, pj4 = rem & 3;
                const int py = pp / 14, px = pp - py * 14;
                const unsigned int u4 = *(const unsigned int*)(O + (py * 16 + pi) * OUT + px * 16 + pj4 * 4);
                const float sc = 0.00390625f;                               // 2^-8: level / 256 is exact in fp16
                __half2 h01 = __floats2half2_rn((float)(u4 & 255u) * sc, (float)((u4 >> 8) & 255u) * sc);
                __half2 h23 = __floats2half2_rn((float)((u4 >> 16) & 255u) * sc, (float)(u4 >> 24) * sc);
                uint2 pk;
                pk.x = *(unsigned int*)&h01;
                pk.y = *(unsigned int*)&h23;
                *(uint2*)(ob + (size_t)pp * 256 + rem * 4) = pk;
            }
        }
        // (the next band writes U, then H behind one barrier and O behind two: no barrier needed here)
    }
}

// taps precompute_coeffs reserves per output pixel: ceil(support * max(scale, 1)) * 2 + 1 with the bicubic support 2
static int pre_ksize(int S) {
    const double fs = S > OUT ? (double)S / OUT : 1.0;
    return (int)ceil(2.0 * fs) * 2 + 1;
}
// rows of image_size that the taps of BAND consecutive output rows reach, rounded up
static int pre_band_rows(int S) {
    const double scale = (double)S / OUT, fs = scale > 1.0 ? scale : 1.0;
    return (int)ceil(BAND * scale + 2.0 * 2.0 * fs) + 2;
}
static size_t pre_lds_bytes(int in_kind, int G, int S) {
    const int urows = pre_band_rows(S);
    return (in_kind == 0 ? (size_t)G * G * sizeof(float) : 0) + (size_t)((urows * S + 3) & ~3) + (size_t)urows * OUT + (size_t)BAND * OUT;
}

extern "C" int vg_clip_preprocess(const void* d_in, int in_kind, int n, int in_side, int image_size, const int32_t* d_bounds,
                                  const int32_t* d_coef, int ksize, const float* d_lut, void* d_out, int out_kind, void* stream) {
    if (n <= 0) return VG_OK;
    if (!d_in || !d_bounds || !d_coef || !d_lut || !d_out) return VG_ERR_ARG;
    if (in_kind != 0 && in_kind != 1) return VG_ERR_ARG;
    if (!(out_kind == 0 || out_kind == 1 || out_kind == 2 || out_kind == 4 || out_kind == 5)) return VG_ERR_ARG;
    if (image_size < VG_PREPROCESS_MIN_IMAGE_SIZE || image_size > VG_PREPROCESS_MAX_IMAGE_SIZE) return VG_ERR_ARG;
    if (in_kind == 0 && (in_side < VG_RENDER_MIN_RESOLUTION - 2 || in_side > VG_RENDER_MAX_RESOLUTION - 2)) return VG_ERR_ARG;
    const int need = pre_ksize(image_size);
    if (ksize < need) return VG_ERR_ARG;
    static_assert(MAXK == 2 * ((2 * VG_PREPROCESS_MAX_IMAGE_SIZE + OUT - 1) / OUT) + 1, "MAXK is the tap count at the largest image_size");
    PreArgs a;
    a.in = d_in;
    a.bounds = d_bounds;
    a.coef = d_coef;
    a.lut = d_lut;
    a.out = d_out;
    a.in_kind = in_kind;
    a.G = in_kind == 0 ? in_side : 0;
    a.S = image_size;
    a.ksize = ksize;
    a.need = need;
    a.out_kind = out_kind;
    a.urows = pre_band_rows(image_size);
    const size_t lds_bytes = pre_lds_bytes(in_kind, a.G, image_size);
    const size_t lds_max = pre_lds_bytes(0, VG_RENDER_MAX_RESOLUTION - 2, VG_PREPROCESS_MAX_IMAGE_SIZE);
    if (need == 5) {                                    // image_size <= 224
        VG_MAX_DYNAMIC_LDS(k_clip_preprocess<5>, lds_max);
        hipLaunchKernelGGL(k_clip_preprocess<5>, dim3(n), dim3(PT), lds_bytes, (hipStream_t)stream, a);
    } else if (need == 7) {                             // 225 .. 336
        VG_MAX_DYNAMIC_LDS(k_clip_preprocess<7>, lds_max);
        hipLaunchKernelGGL(k_clip_preprocess<7>, dim3(n), dim3(PT), lds_bytes, (hipStream_t)stream, a);
    } else {                                            // 337 .. 448
        VG_MAX_DYNAMIC_LDS(k_clip_preprocess<MAXK>, lds_max);
        hipLaunchKernelGGL(k_clip_preprocess<MAXK>, dim3(n), dim3(PT), lds_bytes, (hipStream_t)stream, a);
    }
    VG_LAUNCH_CHECK();
    return VG_OK;
}
