// Part of vit.hip (included in place): zero-shot scores -- k_clip_scores (one wave, up to 64 classes), k_clip_scores_wide (any
// number) and their entry points.

// clip_utils.py:42-61: f /= |f|; probs = softmax(100 f T^T); top-1.  one wave per crop, K <= 64 classes.
__global__ __launch_bounds__(64) void k_clip_scores(const float* __restrict__ feat, const float* __restrict__ text,
                                                    float* __restrict__ probs, int* __restrict__ top1,
                                                    float* __restrict__ top1_score, int n, int D, int Kc) {
    const int crop = blockIdx.x, lane = threadIdx.x;
    const float* f = feat + (size_t)crop * D;
    float ss = 0.f;
    for (int i = lane; i < D; i += 64) ss += f[i] * f[i];
    float nrm = sqrtf(vg_wave_sum(ss));
    float logit = -INFINITY;
    if (lane < Kc) {
        float a = 0.f;
        for (int i = 0; i < D; ++i) a = fmaf(100.0f * (f[i] / nrm), text[(size_t)lane * D + i], a);
        logit = a;
    }
    float mx = vg_wave_max(logit);
    float e = (lane < Kc) ? expf(logit - mx) : 0.f;
    float p = e / vg_wave_sum(e);
    if (lane < Kc) probs[(size_t)crop * Kc + lane] = p;
    // argmax, lowest index on ties
    float best = (lane < Kc) ? p : -1.f;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o);
        int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    if (lane == 0) {
        top1[crop] = bi;
        top1_score[crop] = best;
    }
}

// The same function for any number of classes: one 256-thread workgroup per crop, thread t owns classes t, t + 256, ...
// A class's numbers do not depend on how many other classes there are: the norm is the narrow kernel's (every wave forms it from the
// same 64 partial sums), a logit is one thread's chain a = fmaf(100 (f[i] / nrm), T[c][i], a) over i = 0 .. D-1, the maximum is exact,
// the exponentials are added per thread in ascending class order, then over the wave (vg_wave_sum), then over the waves in wave order,
// and the top-1 comparator is the narrow kernel's.  At Kc <= 64 only wave 0 owns classes and every step is the narrow kernel's step:
// the two return the same bits.
// The text rows go through LDS in tiles of 256 classes x VG_CSW_DT columns, read from memory as whole 16-byte pieces of a row (`vec`:
// D % 4 == 0 and a 16-byte aligned table; otherwise float by float) and from LDS as b128 at a row stride of 36 floats: lane l's slot
// is 9 l mod 16, distinct inside each of the 16-lane groups of such a read.  The scaled feature columns of the tile sit beside it (all
// lanes read the same address), so no LDS size depends on D.  Between the passes a thread's logits / exponentials live in the crop's
// own probs row: a thread reads back only what it wrote.  A thread's pieces of a tile are loaded into registers one tile ahead (while the
// chain of the tile before runs): with a single tile in flight per workgroup the kernel waited out a memory latency per tile.
#define VG_CSW_DT 32
#define VG_CSW_LD 36
// this thread's VG_CSW_DT floats of the text tile (classes cb .., columns d0 ..): piece k is element tid + 256 k of the tile counted in
// 16-byte pieces (vec) or in floats; zeros beyond the table
__device__ __forceinline__ void csw_fetch(float (&pre)[VG_CSW_DT], const float* __restrict__ text, int tid, int cb, int d0, int D, int Kc,
                                          int vec) {
    const int w = min(VG_CSW_DT, D - d0);
    if (vec) {
#pragma unroll
        for (int k = 0; k < VG_CSW_DT / 4; ++k) {
            const int q = tid + 256 * k, r = q / (VG_CSW_DT / 4), c4 = (q % (VG_CSW_DT / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cb + r < Kc && c4 < w) v = *reinterpret_cast<const float4*>(text + (size_t)(cb + r) * D + d0 + c4);
            pre[4 * k] = v.x, pre[4 * k + 1] = v.y, pre[4 * k + 2] = v.z, pre[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < VG_CSW_DT; ++k) {
            const int q = tid + 256 * k, r = q / VG_CSW_DT, c = q % VG_CSW_DT;
            pre[k] = (cb + r < Kc && c < w) ? text[(size_t)(cb + r) * D + d0 + c] : 0.f;
        }
    }
}
// ... into the LDS tile, rows below `live`
__device__ __forceinline__ void csw_store(const float (&pre)[VG_CSW_DT], float* Ts, int tid, int live, int vec) {
    if (vec) {
#pragma unroll
        for (int k = 0; k < VG_CSW_DT / 4; ++k) {
            const int q = tid + 256 * k, r = q / (VG_CSW_DT / 4), c4 = (q % (VG_CSW_DT / 4)) * 4;
            if (r < live) *reinterpret_cast<float4*>(Ts + r * VG_CSW_LD + c4) = make_float4(pre[4 * k], pre[4 * k + 1], pre[4 * k + 2], pre[4 * k + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < VG_CSW_DT; ++k) {
            const int q = tid + 256 * k, r = q / VG_CSW_DT, c = q % VG_CSW_DT;
            if (r < live) Ts[r * VG_CSW_LD + c] = pre[k];
        }
    }
}
__global__ __launch_bounds__(256) void k_clip_scores_wide(const float* __restrict__ feat, const float* __restrict__ text,
                                                         float* probs, int* __restrict__ top1, float* __restrict__ top1_score, int n,
                                                         int D, int Kc, int vec) {
    __shared__ __attribute__((aligned(16))) float Ts[256 * VG_CSW_LD];
    __shared__ __attribute__((aligned(16))) float fs[VG_CSW_DT];
    __shared__ float red_max[4], red_sum[4], red_best[4];
    __shared__ int red_bi[4];
    const int crop = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* f = feat + (size_t)crop * D;
    float* pr = probs + (size_t)crop * Kc;
    float ss = 0.f;
    for (int i = lane; i < D; i += 64) ss += f[i] * f[i];
    const float nrm = sqrtf(vg_wave_sum(ss));
    const float* trow = Ts + tid * VG_CSW_LD;
    float mx = -INFINITY;
    float pre[VG_CSW_DT];
    if (D > 0) csw_fetch(pre, text, tid, 0, 0, D, Kc, vec);
    for (int cb = 0; cb < Kc; cb += 256) {
        const int live = min(256, (Kc - cb + 63) & ~63);          // rows of the tile that a wave with classes reads
        float a = 0.f;
        for (int d0 = 0; d0 < D; d0 += VG_CSW_DT) {
            const int w = min(VG_CSW_DT, D - d0);
            __syncthreads();                                      // the readers of the tile before are done
            if (tid < w) fs[tid] = 100.0f * (f[d0 + tid] / nrm);
            csw_store(pre, Ts, tid, live, vec);
            __syncthreads();
            {                                                     // the next tile's pieces: in flight while this tile's chain runs
                int nd0 = d0 + VG_CSW_DT, ncb = cb;
                if (nd0 >= D) nd0 = 0, ncb = cb + 256;
                if (ncb < Kc) csw_fetch(pre, text, tid, ncb, nd0, D, Kc, vec);
            }
            if (cb + (tid & ~63) < Kc) {                          // whole waves without a class skip the chain
                if (w == VG_CSW_DT) {
#pragma unroll
                    for (int i = 0; i < VG_CSW_DT; ++i) a = fmaf(fs[i], trow[i], a);
                } else {
                    for (int i = 0; i < w; ++i) a = fmaf(fs[i], trow[i], a);
                }
            }
        }
        if (cb + tid < Kc) {
            pr[cb + tid] = a;
            mx = fmaxf(mx, a);
        }
    }
    mx = vg_wave_max(mx);
    float es = 0.f;
    if (lane == 0) red_max[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
    for (int c = tid; c < Kc; c += 256) {
        const float e = expf(pr[c] - mx);
        pr[c] = e;
        es += e;
    }
    es = vg_wave_sum(es);
    if (lane == 0) red_sum[wave] = es;
    __syncthreads();
    const float tot = ((red_sum[0] + red_sum[1]) + red_sum[2]) + red_sum[3];
    // argmax, lowest index on ties: a thread's classes ascend, so `>` keeps the lower one
    float best = -1.f;
    int bi = tid;
    for (int c = tid; c < Kc; c += 256) {
        const float p = pr[c] / tot;
        pr[c] = p;
        if (c == tid || p > best) {
            best = p;
            bi = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o);
        int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    if (lane == 0) {
        red_best[wave] = best;
        red_bi[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) {
            const float ob = red_best[k];
            const int oi = red_bi[k];
            if (ob > best || (ob == best && oi < bi)) {
                best = ob;
                bi = oi;
            }
        }
        top1[crop] = bi;
        top1_score[crop] = best;
    }
}

extern "C" {

int vg_clip_scores(const float* d_feat, int n, int dim, const float* d_text, int n_classes, float* d_probs,
                   int32_t* d_top1, float* d_top1_score, void* stream) {
    if (n <= 0) return VG_OK;
    if (!d_feat || !d_text || !d_probs || !d_top1 || !d_top1_score || n_classes <= 0 || n_classes > 64) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_clip_scores, dim3(n), dim3(64), 0, (hipStream_t)stream, d_feat, d_text, d_probs, d_top1,
                       d_top1_score, n, dim, n_classes);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_clip_scores_wide(const float* d_feat, int n, int dim, const float* d_text, int n_classes, float* d_probs,
                        int32_t* d_top1, float* d_top1_score, void* stream) {
    if (n <= 0) return VG_OK;
    if (!d_feat || !d_text || !d_probs || !d_top1 || !d_top1_score || n_classes <= 0) return VG_ERR_ARG;
    const int vec = dim % 4 == 0 && (uintptr_t)d_text % 16 == 0;         // whole 16-byte pieces of every text row
    hipLaunchKernelGGL(k_clip_scores_wide, dim3(n), dim3(256), 0, (hipStream_t)stream, d_feat, d_text, d_probs, d_top1,
                       d_top1_score, n, dim, n_classes, vec);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

}  // extern "C"
