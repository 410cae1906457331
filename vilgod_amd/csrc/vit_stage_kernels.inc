// Part of vit.hip (included in place): the kernels around the GEMMs and the attention -- patch rows, embedding + ln_pre, LayerNorm,
// head, the weight folds, and the class-row gather / scatter of the last block.


// ---------------------------------------------------------------------------------------------
// im2col of CHW crops into patch rows: P[(crop*G*G + py*G + px)][c*ps*ps + i*ps + j]; rows of Kpad >= 3*ps*ps columns (the GEMM's
// K, a multiple of 64: 588 -> 640 for patch 14), the padding columns zero
template <typename TI, typename TO>
__global__ void k_im2col(const TI* __restrict__ crops, TO* __restrict__ P, int n, int res, int ps, int Kpad) {
    const int G = res / ps, Kp = 3 * ps * ps;
    size_t total = (size_t)n * G * G * Kpad;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        int col = idx % Kpad;
        size_t row = idx / Kpad;
        if (col >= Kp) { P[idx] = (TO)0.f; continue; }
        int px = row % G, py = (row / G) % G;
        size_t crop = row / ((size_t)G * G);
        int j = col % ps, i = (col / ps) % ps, c = col / (ps * ps);
        P[idx] = (TO)(float)crops[((crop * 3 + c) * res + (py * ps + i)) * res + px * ps + j];
    }
}

// x[crop][t] = (t == 0 ? class_embedding : patch_out[crop][t-1]) + positional_embedding[t]; x = ln_pre(x)
// one wave per token row.  (model.py:227-229)
template <typename TO>
__global__ __launch_bounds__(256) void k_embed_lnpre(const float* __restrict__ patch_out, const float* __restrict__ cls,
                                                     const float* __restrict__ pos, const float* __restrict__ lw,
                                                     const float* __restrict__ lb, TO* __restrict__ x, int n_rows,
                                                     int T, int W, int n_rows_padded, const float* __restrict__ lw1 = nullptr,
                                                     const float* __restrict__ lb1 = nullptr, f16* __restrict__ h1 = nullptr,
                                                     f16* __restrict__ pair_hi = nullptr, f16* __restrict__ pair_lo = nullptr) {
    // pair_hi / pair_lo (TO = float, vectorised widths): the stream is written as the fp16 pair of EPI_BIAS_RESID_HL instead of to x
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows_padded) return;
    if (row >= n_rows) {
        // padding rows of the residual stream (GEMM row tile): re-zeroed on every call -- every residual epilogue adds its
        // bias into them, and the workspace carve-up moves when n_crops changes
        if (pair_hi) for (int c = lane; c < W; c += 64) { pair_hi[(size_t)row * W + c] = (f16)0.f; pair_lo[(size_t)row * W + c] = (f16)0.f; }
        else for (int c = lane; c < W; c += 64) x[(size_t)row * W + c] = (TO)0.f;
        return;
    }
    const int crop = row / T, t = row - crop * T;
    const float* src = (t == 0) ? cls : patch_out + ((size_t)crop * (T - 1) + (t - 1)) * W;
    if ((W & 255) == 0 && W <= 1024) {
        // vectorised path (every shipped width): float4 per lane like k_layernorm -- 1 KB per wave instruction instead of 256 B
        const int nv = W >> 8;
        float4 v4[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nv) {
                const int c = (i * 64 + lane) * 4;
                const float4 a = *(const float4*)(src + c), b = *(const float4*)(pos + (size_t)t * W + c);
                v4[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
                s += (v4[i].x + v4[i].y) + (v4[i].z + v4[i].w);
            }
        const float mean = vg_wave_sum(s) / (float)W;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nv) {
                const float a = v4[i].x - mean, b = v4[i].y - mean, c = v4[i].z - mean, d = v4[i].w - mean;
                q += (a * a + b * b) + (c * c + d * d);
            }
        const float rstd = rsqrtf(vg_wave_sum(q) / (float)W + 1e-5f);
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nv) {
                const int c = (i * 64 + lane) * 4;
                const float4 w4 = *(const float4*)(lw + c), b4 = *(const float4*)(lb + c);
                float o[4] = {(v4[i].x - mean) * rstd * w4.x + b4.x, (v4[i].y - mean) * rstd * w4.y + b4.y,
                              (v4[i].z - mean) * rstd * w4.z + b4.z, (v4[i].w - mean) * rstd * w4.w + b4.w};
                TO* dst = x + (size_t)row * W + c;
                if (sizeof(TO) == 2) {
                    const f16x4 h4 = {(f16)o[0], (f16)o[1], (f16)o[2], (f16)o[3]};
                    *(f16x4*)dst = h4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (float)h4[e];           // what a separate LayerNorm kernel would read back
                } else if (pair_hi) {
                    const f16x4 h4 = {(f16)o[0], (f16)o[1], (f16)o[2], (f16)o[3]};
                    const f16x4 l4 = {(f16)(o[0] - (float)h4[0]), (f16)(o[1] - (float)h4[1]), (f16)(o[2] - (float)h4[2]), (f16)(o[3] - (float)h4[3])};
                    *(f16x4*)(pair_hi + (size_t)row * W + c) = h4;
                    *(f16x4*)(pair_lo + (size_t)row * W + c) = l4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (float)h4[e] + (float)l4[e];          // what the stream holds from here on
                } else {
                    *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
                }
                v4[i] = make_float4(o[0], o[1], o[2], o[3]);
                s2 += (o[0] + o[1]) + (o[2] + o[3]);
            }
        if (h1) {
            // ln_1 of the first block on the row just produced, k_layernorm's arithmetic (bit-identical to the separate launch)
            const float mean2 = vg_wave_sum(s2) / (float)W;
            float q2 = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nv) {
                    const float a = v4[i].x - mean2, b = v4[i].y - mean2, c = v4[i].z - mean2, d = v4[i].w - mean2;
                    q2 += (a * a + b * b) + (c * c + d * d);
                }
            const float rstd2 = rsqrtf(vg_wave_sum(q2) / (float)W + 1e-5f);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nv) {
                    const int c = (i * 64 + lane) * 4;
                    const float4 w4 = *(const float4*)(lw1 + c), b4 = *(const float4*)(lb1 + c);
                    const f16x4 h4 = {(f16)((v4[i].x - mean2) * rstd2 * w4.x + b4.x), (f16)((v4[i].y - mean2) * rstd2 * w4.y + b4.y),
                                      (f16)((v4[i].z - mean2) * rstd2 * w4.z + b4.z), (f16)((v4[i].w - mean2) * rstd2 * w4.w + b4.w)};
                    *(f16x4*)(h1 + (size_t)row * W + c) = h4;
                }
        }
        return;
    }
    float v[16];
    const int per = W / 64;   // W multiple of 64, <= 1024
    float s = 0.f;
    for (int i = 0; i < per; ++i) {
        int c = lane + 64 * i;
        v[i] = src[c] + pos[(size_t)t * W + c];
        s += v[i];
    }
    float mean = vg_wave_sum(s) / (float)W;
    float q = 0.f;
    for (int i = 0; i < per; ++i) {
        float d = v[i] - mean;
        q += d * d;
    }
    float rstd = rsqrtf(vg_wave_sum(q) / (float)W + 1e-5f);
    float s2 = 0.f;
    for (int i = 0; i < per; ++i) {
        int c = lane + 64 * i;
        v[i] = (v[i] - mean) * rstd * lw[c] + lb[c];
        x[(size_t)row * W + c] = (TO)v[i];
        v[i] = (float)(TO)v[i];                     // what a separate LayerNorm kernel would read back
        s2 += v[i];
    }
    if (h1) {
        // ln_1 of the first block on the row just produced: one LayerNorm launch (and its read of the stream) less per encode
        const float mean2 = vg_wave_sum(s2) / (float)W;
        float q2 = 0.f;
        for (int i = 0; i < per; ++i) {
            float d = v[i] - mean2;
            q2 += d * d;
        }
        const float rstd2 = rsqrtf(vg_wave_sum(q2) / (float)W + 1e-5f);
        for (int i = 0; i < per; ++i) {
            int c = lane + 64 * i;
            h1[(size_t)row * W + c] = (f16)((v[i] - mean2) * rstd2 * lw1[c] + lb1[c]);
        }
    }
}

// LayerNorm (fp32 statistics, model.py:157-163): x f32 [rows,W] -> h (f16 or f32). one wave per row.
// W % 256 == 0 takes the vectorised path: float4 loads (1 KB per wave instruction), packed stores.
template <typename TO, typename TI = float>
__global__ __launch_bounds__(256) void k_layernorm(const TI* __restrict__ x, const float* __restrict__ lw,
                                                   const float* __restrict__ lb, TO* __restrict__ h, int n_rows, int W,
                                                   int row_stride_in /*in rows of W*/) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const TI* src = x + (size_t)row * row_stride_in * W;
    if ((W & 255) == 0 && W <= 1024) {
        const int nv = W >> 8;                       // float4 per lane
        float4 v[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nv) {
                if (sizeof(TI) == 2) {
                    const f16x4 t4 = *(const f16x4*)(src + (i * 64 + lane) * 4);
                    v[i] = make_float4((float)t4[0], (float)t4[1], (float)t4[2], (float)t4[3]);
                } else {
                    v[i] = *(const float4*)(src + (i * 64 + lane) * 4);
                }
                s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            }
        const float mean = vg_wave_sum(s) / (float)W;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nv) {
                const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
                q += (a * a + b * b) + (c * c + d * d);
            }
        const float rstd = rsqrtf(vg_wave_sum(q) / (float)W + 1e-5f);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nv) {
                const int c = (i * 64 + lane) * 4;
                const float4 w4 = *(const float4*)(lw + c), b4 = *(const float4*)(lb + c);
                const float o0 = (v[i].x - mean) * rstd * w4.x + b4.x, o1 = (v[i].y - mean) * rstd * w4.y + b4.y;
                const float o2 = (v[i].z - mean) * rstd * w4.z + b4.z, o3 = (v[i].w - mean) * rstd * w4.w + b4.w;
                TO* dst = h + (size_t)row * W + c;
                if (sizeof(TO) == 2) {
                    f16x4 h4 = {(f16)o0, (f16)o1, (f16)o2, (f16)o3};
                    *(f16x4*)dst = h4;
                } else {
                    *(float4*)dst = make_float4(o0, o1, o2, o3);
                }
            }
        return;
    }
    float v[16];
    const int per = W / 64;
    float s = 0.f;
    for (int i = 0; i < per; ++i) {
        v[i] = (float)src[lane + 64 * i];
        s += v[i];
    }
    float mean = vg_wave_sum(s) / (float)W;
    float q = 0.f;
    for (int i = 0; i < per; ++i) {
        float d = v[i] - mean;
        q += d * d;
    }
    float rstd = rsqrtf(vg_wave_sum(q) / (float)W + 1e-5f);
    for (int i = 0; i < per; ++i) {
        int c = lane + 64 * i;
        h[(size_t)row * W + c] = (TO)((v[i] - mean) * rstd * lw[c] + lb[c]);
    }
}

// ---------------------------------------------------------------------------------------------
// head: ln_post(x[crop, 0, :]) @ proj  (model.py:235-238).  one workgroup per crop.
// row_idx (text tower, model.py:352-354): row row_idx[crop] of the item's T rows instead of row 0, clamped into [0, T) -- a wrong index
// reads a wrong row, never outside the item.
template <typename TI>
__global__ __launch_bounds__(256) void k_head(const TI* __restrict__ x, const float* __restrict__ lw,
                                              const float* __restrict__ lb, const float* __restrict__ proj,
                                              float* __restrict__ feat, int T, int W, int D, const int32_t* __restrict__ row_idx = nullptr) {
    extern __shared__ float sm[];   // [W]
    __shared__ float red[8];
    const int crop = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = row_idx ? row_idx[crop] : 0;
    const TI* src = x + ((size_t)crop * T + (r < 0 ? 0 : r >= T ? T - 1 : r)) * W;
    float s = 0.f;
    for (int c = tid; c < W; c += 256) s += (float)src[c];
    s = vg_wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    float mean = (red[0] + red[1] + red[2] + red[3]) / (float)W;
    __syncthreads();
    float q = 0.f;
    for (int c = tid; c < W; c += 256) {
        float d = (float)src[c] - mean;
        q += d * d;
    }
    q = vg_wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)W + 1e-5f);
    for (int c = tid; c < W; c += 256) sm[c] = ((float)src[c] - mean) * rstd * lw[c] + lb[c];
    __syncthreads();
    for (int j = tid; j < D; j += 256) {
        float a = 0.f;
#pragma unroll 16                                  // 16 independent loads of the projection column in flight per trip (the chain
        for (int i = 0; i < W; ++i)               // a = fma(.., a) stays in order: same sum as before)
            a = fmaf(sm[i], proj[(size_t)i * D + j], a);
        feat[(size_t)crop * D + j] = a;
    }
}

// W'[n,k] = f16(g[k] * W[n,k]);  c1[n] = sum_k W'[n,k] (of the ROUNDED values, which is what the MFMAs will sum);
// c2[n] = b[n] + sum_k beta[k] * W[n,k].  One workgroup per output feature n, fixed summation order.
__global__ __launch_bounds__(256) void k_ln_fold(const float* __restrict__ W32, const float* __restrict__ g, const float* __restrict__ beta,
                                                 const float* __restrict__ b, f16* __restrict__ Wf, float* __restrict__ c1,
                                                 float* __restrict__ c2, int K) {
    __shared__ double sh1[256], sh2[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = tid; k < K; k += 256) {
        const float w = W32[(size_t)n * K + k];
        const f16 wf = (f16)(g[k] * w);
        Wf[(size_t)n * K + k] = wf;
        s1 += (double)(float)wf;
        s2 += (double)beta[k] * (double)w;
    }
    sh1[tid] = s1; sh2[tid] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { sh1[tid] += sh1[tid + o]; sh2[tid] += sh2[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { c1[n] = (float)sh1[0]; c2[n] = (float)((double)b[n] + sh2[0]); }
}

// Single-channel patch embedding (SURVEY 8d; mv_utils.py:36: the three channels of a rendered crop are one image).  With the crop's
// uint8 level u, channel c of the reference's input is (u / 255 - mean_c) / std_c (clip.py:79-86), so
//   conv1(x)[n] = sum_p (u_p / 256) * W1[n,p] + b1[n],   W1[n,p] = (256 / 255) * sum_c conv1[n,c,p] / std_c,
//                                                        b1[n]   = - sum_c (mean_c / std_c) * sum_p conv1[n,c,p]
// -- exact in real arithmetic; the renderer hands over u / 256 (exact in fp16), W1 is rounded to fp16 once from the fp32 sum.
// b1 is added to the positional embedding of the 196 patch tokens (k_embed_lnpre adds that table to the GEMM's rows anyway).
// One workgroup per output feature n, fixed summation order, double accumulation.
__global__ __launch_bounds__(256) void k_conv1_fold(const float* __restrict__ conv1, const float* __restrict__ pos, f16* __restrict__ W1,
                                                    float* __restrict__ pos1, int W, int T, int pp, float m0, float m1, float m2,
                                                    float s0, float s1, float s2) {
    __shared__ double sh[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* w = conv1 + (size_t)n * 3 * pp;
    double acc = 0.0;
    for (int p = tid; p < pp; p += 256) {
        const double a = (double)w[p], b = (double)w[pp + p], c = (double)w[2 * pp + p];
        W1[(size_t)n * pp + p] = (f16)(float)((256.0 / 255.0) * (a / (double)s0 + b / (double)s1 + c / (double)s2));
        acc += a * ((double)m0 / (double)s0) + b * ((double)m1 / (double)s1) + c * ((double)m2 / (double)s2);
    }
    sh[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    const float b1 = (float)(-sh[0]);
    for (int t = tid; t < T; t += 256) pos1[(size_t)t * W + n] = pos[(size_t)t * W + n] + (t > 0 ? b1 : 0.f);
}

extern "C" {      // (these three have always carried unmangled names)
// The last block's class-token rows, compacted: hc[c] = h[c * T] (attention output, fp16), xc[c] = x[c * T] (residual stream, fp32);
// rows n_crops .. Mc - 1 (padding of the GEMM row tile) are zeroed.  One workgroup per row.
__global__ __launch_bounds__(256) void k_gather_cls(const f16* __restrict__ h, const float* __restrict__ x, f16* __restrict__ hc,
                                                    float* __restrict__ xc, int n_crops, int T, int W,
                                                    const f16* __restrict__ pair_hi = nullptr, const f16* __restrict__ pair_lo = nullptr) {
    // pair_hi / pair_lo: the stream kept as an fp16 pair (EPI_BIAS_RESID_HL) -- the compact rows are fp32 either way
    const int c = blockIdx.x;
    for (int i = threadIdx.x; i < W; i += 256) {
        hc[(size_t)c * W + i] = c < n_crops ? h[(size_t)c * T * W + i] : (f16)0.f;
        if (pair_hi) xc[(size_t)c * W + i] = c < n_crops ? (float)pair_hi[(size_t)c * T * W + i] + (float)pair_lo[(size_t)c * T * W + i] : 0.f;
        else xc[(size_t)c * W + i] = c < n_crops ? x[(size_t)c * T * W + i] : 0.f;
    }
}

// The last block's QUERY projection needs the class-token rows only (round 5): their rows of the fp16 residual copy and of the folded
// LayerNorm's partial statistics, compacted (rows n_crops .. Mc - 1 zeroed: statistics (0, 0) give rstd = 1 / sqrt(eps), finite) ...
__global__ __launch_bounds__(256) void k_gather_cls_ln(const f16* __restrict__ x16, const LnPartial* __restrict__ st, f16* __restrict__ x16c,
                                                       LnPartial* __restrict__ stc, int n_crops, int T, int W, int nst) {
    const int c = blockIdx.x;
    for (int i = threadIdx.x; i < W; i += 256) x16c[(size_t)c * W + i] = c < n_crops ? x16[(size_t)c * T * W + i] : (f16)0.f;
    if ((int)threadIdx.x < nst) stc[(size_t)c * nst + threadIdx.x] = c < n_crops ? st[(size_t)c * T * nst + threadIdx.x] : LnPartial{0.f, 0.f};
}
// ... and the projected queries back into the class-token rows of the qkv buffer (columns [0, W)), where the attention reads them
__global__ __launch_bounds__(256) void k_scatter_cls_q(const f16* __restrict__ qc, f16* __restrict__ qkv, int T, int W, int ld) {
    const int c = blockIdx.x;
    for (int i = threadIdx.x; i < W; i += 256) qkv[(size_t)c * T * ld + i] = qc[(size_t)c * W + i];
}
}  // extern "C"
