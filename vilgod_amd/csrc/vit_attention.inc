// Part of vit.hip (included in place): the attention kernels (k_attention_f16, k_attention_f16_long, k_attention_f32; the first and the
// last also in a causal form for the text tower) and their launch paths (launch_attention, launch_attention_causal, launch_attention_f32).


// ---------------------------------------------------------------------------------------------
// fp16 attention, head dim 64, T <= 224.  One workgroup (7 waves) per (crop, head); wave w owns query rows
// [32w, 32w+32).  S^T[key][q] = K Q^T (A = K rows from LDS, B = Q rows from HBM), softmax along keys is a
// per-lane reduction (+ one cross-half shuffle), O^T[d][q] = V^T P^T with the S^T accumulators re-used
// as the B operand (guide §3 "An accumulator tile as the next MFMA's operand").
#define AT_MAXT 224
#define AT_KLD 72      // K rows: 64 + 8 halves
#define AT_LDS_BYTES ((AT_MAXT * AT_KLD + 64 * 228 + 7 * 32 * AT_KLD) * 2)   // 93,696 B
#define AT_LDS_BYTES_TR ((AT_MAXT * AT_KLD + AT_MAXT * AT_KLD + 7 * 32 * AT_KLD) * 2)   // 96,768 B (row-major V)
#define AT_VLD 228     // V^T rows: 224 + 4 halves (456 B: 32 rows of a fragment read hit 32 different banks; the 8 x 8 transposed
                       // writes of a wave land 2-way conflicted)
// NKB: number of 32-key blocks, ceil(T / 32), as a compile-time constant (7 for ViT-B/16's 197 tokens): with a run-time count every
// key block sits behind its own branch (14 scheduling regions per item); with the constant the item is straight-line code.
// TT: the token count as a constant too (197 for ViT-B/16: row clamps and key masks become per-thread constants), 0 = run-time T.
typedef short s16x4v __attribute__((__vector_size__(4 * sizeof(short))));
// TR: V stays ROW-major in LDS (one 16-byte write per chunk, like K) and the O^T MFMAs' A operand -- V^T[d][8 consecutive keys] -- comes
// from gfx950's transposing read: per group of 16 lanes ds_read_b64_tr_b16 takes a 4-key x 16-feature block (lane 4q + p of the group
// supplies the address of key q, features 4p .. 4p + 3) and hands lane i feature i of the four keys.
// STAG (round 5; MI355X_MICROARCH.md "two waves per SIMD", item 9): the two waves that share a SIMD (w and w + 4) run the same program and
// leave the staging barrier together, so they want the matrix pipe at the same time (S^T MFMAs), then the vector ALU at the same time
// (softmax), then the matrix pipe again.  With STAG waves 0-3 issue the NEXT item's twelve loads after their S^T MFMAs (which run on
// while the loads are issued) and waves 4-6 before theirs, as all waves did: the partners reach the softmax ~1-2 k cycles apart, one's
// vector work beside the other's matrix work.  Same instructions per wave on the same data: bit-identical output.  Alone, 337 crops, variants
// interleaved in one process: 96.0 us against 99.4 (331 crops: 94.7 / 98.2).  Measured and dropped: waves 4-6 ALSO deferring their output
// phase to the start of the next item (the guide's full recipe; accumulators kept across the barrier): 98.3 us, no better than no stagger.
// CAUSAL (the CLIP text tower, model.py:320-326 build_attention_mask): query row q sees keys 0 .. q.  Wave w's rows are [32w, 32w + 32), so
// key blocks kb > w are wholly masked: never multiplied, exponentiated or fed to the P V MFMAs.  Block kb == w holds the diagonal: registers
// with key > q are set to -inf before the max (a stored row has q < T, so the key >= T mask is implied), exp2(-inf) = 0 enters the sum and P
// as an exact zero, and key 0 is always visible: sum > 0.  Row i therefore equals, bit for bit, row i of the plain kernel run on the item's
// first i + 1 tokens.  With CAUSAL = false every added condition folds away at compile time.
template <bool TRACE = false, int NKB = 7, int TT = 0, bool TR = false, bool STAG = false, bool CAUSAL = false>
__global__ __launch_bounds__(448) void k_attention_f16(const f16* __restrict__ qkv, f16* __restrict__ out, int T_arg,
                                                       int W, int heads, int ld, int n_items, long long* __restrict__ trace = nullptr,
                                                       int q_tiles = 7) {
    const int T = TT ? TT : T_arg;
    long long tr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tc = 0;      // TRACE: cycles per phase, summed over this wave's items
#define AT_STAMP(i) if (TRACE) { const long long c_ = clock64(); tr[i] += c_ - tc; tc = c_; }
    extern __shared__ __attribute__((aligned(16))) char at_smem[];       // AT_LDS_BYTES: K rows | V^T rows | one 32-row tile per wave
    f16* const Ks = (f16*)at_smem;
    f16* const Vt = Ks + AT_MAXT * AT_KLD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // per-wave 32 x 64 tile (row stride AT_KLD): the wave's Q rows arrive coalesced (eight lanes per 128-byte row) and are re-read as
    // MFMA fragments (one row per lane); the output rows go the other way.  Only this wave touches it: LDS operations of one wave
    // execute in program order, no barrier needed.
    f16* const Vs = Vt;                       // TR: [AT_MAXT][AT_KLD] rows instead of the transposed [64][AT_VLD] image
    f16* const Qs = Vt + (TR ? AT_MAXT * AT_KLD : 64 * AT_VLD) + wave * 32 * AT_KLD;
    const int tr_i = lane & 15, tr_g = lane >> 4;
    const int tr_off = ((4 * (tr_g >> 1) + (tr_i >> 2)) * AT_KLD + 16 * (tr_g & 1) + 4 * (tr_i & 3)) * 2;      // bytes: + (kb*32 + 16s [+ 8]) rows, + dt*32 features
    const int crow = lane >> 3, cpart = lane & 7;                           // coalesced layout: row it * 8 + crow, 16-byte part
    const int r31 = lane & 31, hh = lane >> 5;
    const int q0 = wave * 32;
    const int q = q0 + r31;
    constexpr int nkb = NKB;                                          // == (T + 31) / 32, checked by the launcher
    const int wv = CAUSAL ? __builtin_amdgcn_readfirstlane(wave) : wave;      // (the causal block skip branches on it: wave-uniform by construction)
#define AT_LIVE(kb) ((kb) < nkb && (!CAUSAL || (kb) <= wv))          // key block kb holds keys that this wave's rows see
    static_assert(AT_MAXT * 8 == 4 * 448, "staging split");
    // PERSISTENT workgroups (182 VGPRs and 62 KB of LDS allow one 7-wave workgroup per CU, so nothing else would hide
    // an item's load latency): item = (crop, head); the NEXT item's Q / K / V rows are fetched into registers while
    // the current item is computed.  All eight 16-byte K/V loads of a thread go out back to back, branch-free
    // (clamped row, zeroed by select when written to LDS).
    f16x8 qf[4], qn[4];
    uint4 kreg[4];
    f16x8 vreg[4];
    // Per-lane element offsets inside an item, 32-bit and item-invariant (an item's rows span < T * ld elements): the item's base is a
    // wave-uniform 64-bit pointer, so a load is SGPR base + VGPR offset and nothing 64-bit per lane lives across the item loop (the
    // size_t row products did: 256 VGPRs + a spilled pair in the TR instantiation, round 3).
    unsigned qoff[4], kvoff[4], ooff[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int qr = q0 + it * 8 + crow;
        qoff[it] = (unsigned)((qr < T ? qr : T - 1) * ld + cpart * 8);
        ooff[it] = (unsigned)(qr * W + cpart * 8);
        const int c = tid + it * 448, key = c >> 3, part = c & 7;
        kvoff[it] = (unsigned)((key < T ? key : T - 1) * ld + part * 8);
    }
    auto fetch = [&](int item) {
        const int crop = item / heads, head = item - crop * heads;
        const f16* qbase = qkv + (size_t)crop * T * ld + head * 64;
        const f16* kbase = qbase + W;
        const f16* vbase = qbase + 2 * W;
#pragma unroll
        for (int it = 0; it < 4; ++it) qn[it] = *(const f16x8*)(qbase + qoff[it]);
        // K and V rows: eight lanes cover one 128-byte row (clamped row, zeroed by select when written to LDS).  For V the transpose
        // (TR = false) happens on the LDS-write side, 2-way bank-conflicted.  One key per lane (conflict-free writes, but 64 rows x 16 B
        // per load instruction) kept the waves that issue last waiting ~3.5 k cycles per item on the address path: 151 -> 146 us per
        // launch; a 16-key x 64-byte pattern (conflict-free writes, 16 rows per instruction) measured 149 us.
#pragma unroll
        for (int it = 0; it < 4; ++it) kreg[it] = *(const uint4*)(kbase + kvoff[it]);
#pragma unroll
        for (int it = 0; it < 4; ++it) vreg[it] = *(const f16x8*)(vbase + kvoff[it]);
    };
    int item = blockIdx.x;
    if (item < n_items) fetch(item);
    for (; item < n_items; item += gridDim.x) {
    if (TRACE) tc = clock64();
    const int crop = item / heads, head = item - crop * heads;
    f16* const obase = out + (size_t)crop * T * W + head * 64;
    // K -> LDS rows (zero beyond T)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = tid + it * 448, key = c >> 3, part = c & 7;
        *(uint4*)(Ks + key * AT_KLD + part * 8) = key < T ? kreg[it] : make_uint4(0, 0, 0, 0);
    }
    // V -> LDS transposed (zero beyond T)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = tid + it * 448, key = c >> 3, part = c & 7;
        const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        const f16x8 v = key < T ? vreg[it] : z;
        if (TR) *(f16x8*)(Vs + key * AT_KLD + part * 8) = v;
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(part * 8 + e) * AT_VLD + key] = v[e];
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) *(f16x8*)(Qs + (it * 8 + crow) * AT_KLD + cpart * 8) = qn[it];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const f16x8*)(Qs + r31 * AT_KLD + s * 16 + hh * 8);
    __syncthreads();
    AT_STAMP(0)                                                        // K / V^T into LDS + barrier
    const bool has_next = item + (int)gridDim.x < n_items;
    const bool computes = q0 < T && wave < q_tiles;   // (q_tiles: query tiles wanted -- 1 in the last block, whose class-token row alone is used)
    const bool late = STAG && wave < 4 && computes;   // this wave issues the next item's loads behind its S^T MFMAs
    if (has_next && !late) fetch(item + gridDim.x);                    // in flight during the compute below
    AT_STAMP(1)                                                        // issue of the next item's loads
    if (computes) {


    f32x16 sacc[7];
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
        if (AT_LIVE(kb)) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                f16x8 kf = *(const f16x8*)(Ks + (kb * 32 + r31) * AT_KLD + s * 16 + hh * 8);
                sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sacc[kb], 0, 0, 0);
            }
        }
    }
    if (STAG && has_next && late) fetch(item + gridDim.x);             // (the matrix pipe works on the 28 MFMAs meanwhile)
    AT_STAMP(2)                                                        // S^T MFMAs issued
    // softmax over keys (scores scaled by 1/8 = dh^-0.5, model.py via nn.MultiheadAttention).  Only the last key block
    // can hold keys >= T; blocks beyond it were never computed (zeros) and are skipped below.
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        if (!CAUSAL && kb == nkb - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (key >= T) sacc[kb][r] = -INFINITY;
            }
        }
        if (CAUSAL && kb < nkb && kb == wv) {                          // the diagonal block: keys behind the row's own position
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (key > q) sacc[kb][r] = -INFINITY;
            }
        }
        if (AT_LIVE(kb)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    AT_STAMP(3)                                                        // max pass (waits for the MFMA results)
    const float c2 = 0.125f * 1.4426950408889634f;
    const float mc = -mx * c2;
    float sum = 0.f;
    // keys of the LAST block that exist: register group g (4 registers) holds keys 8g .. 8g+7 of the block (both lane halves), so
    // a group with 8g >= tail is -inf throughout -> p = 0 without an exp (197 tokens: 12 of the block's 16 registers)
    const int tail = T - 32 * (nkb - 1);
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        if (AT_LIVE(kb)) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (CAUSAL || kb < nkb - 1 || 8 * g < tail) {
#pragma unroll
                    for (int r = 4 * g; r < 4 * g + 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kb][r], c2, mc));      // raw v_exp_f32: exp2(-inf) = 0
                        sacc[kb][r] = p;
                        sum += p;
                    }
                } else {
#pragma unroll
                    for (int r = 4 * g; r < 4 * g + 4; ++r) sacc[kb][r] = 0.f;
                }
            }
        }
    }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    AT_STAMP(4)                                                        // exp pass

    f32x16 oacc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        if (AT_LIVE(kb)) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!CAUSAL && kb == nkb - 1 && 16 * s >= tail) continue;        // k-step of keys that do not exist: P = 0 there, adds exact zeros
                f16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (f16)sacc[kb][8 * s + j];
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    // A[d][k]: element j <-> key kb*32 + 16s + 8(j>>2) + 4hh + (j&3)
                    f16x4 lo, hi;
                    if (TR) {
                        const char* vb = (const char*)Vs + tr_off + ((kb * 32 + 16 * s) * AT_KLD + dt * 32) * 2;
                        lo = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v*)vb));
                        hi = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v*)(vb + 8 * AT_KLD * 2)));
                    } else {
                        const f16* vp = Vt + (dt * 32 + r31) * AT_VLD + kb * 32 + 16 * s + 4 * hh;
                        lo = *(const f16x4*)vp; hi = *(const f16x4*)(vp + 8);
                    }
                    f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[dt], 0, 0, 0);
                }
            }
        }
    }
    AT_STAMP(5)                                                        // P -> fp16, V^T fragments, O^T MFMAs issued
    // output rows through the wave's tile: a lane's 4-feature pieces in, 16-byte parts of whole 128-byte rows out
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x4 h4;
#pragma unroll
            for (int e = 0; e < 4; ++e) h4[e] = (f16)(oacc[dt][4 * g + e] * inv);
            *(f16x4*)(Qs + r31 * AT_KLD + dt * 32 + 8 * g + 4 * hh) = h4;
        }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int qr = q0 + it * 8 + crow;
        const f16x8 v = *(const f16x8*)(Qs + (it * 8 + crow) * AT_KLD + cpart * 8);
        if (qr < T) *(f16x8*)(obase + ooff[it]) = v;
    }
    }
    AT_STAMP(6)                                                        // scaled output (waits for the O^T MFMAs) + stores issued
    __syncthreads();      // every wave is done with this item's K / V^T before the next item overwrites them
    AT_STAMP(7)                                                        // barrier at the end of the item
    }
    if (TRACE && trace && lane == 0) {
        long long* o = trace + ((size_t)blockIdx.x * 7 + wave) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = tr[i];
    }
#undef AT_STAMP
#undef AT_LIVE
}

// ---------------------------------------------------------------------------------------------
// fp16 attention, head dim 64, AT_MAXT < T <= AL_MAXT (ViT-L/14: 257 tokens) -- flash-style, the S x S scores never held at once.
// Same MFMA layout as k_attention_f16: S^T[key][q] = K Q^T (A = K rows from LDS, B = the wave's Q fragments, in registers), so a
// lane holds one query row's scores and the softmax is per lane (+ one cross-half shuffle); O^T[d][q] = V^T P^T with the scores
// re-used as the B operand and V^T fragments from the transposing LDS read of row-major V (the TR path).  Online softmax over
// 64-key blocks: running max m and running sum l per query row, O rescaled by exp2((m_old - m_new) c2) at each block.
// Workgroup: 4 waves, one item (crop, head) at a time, persistent over items.  The item's 32-row query tiles are processed in
// PASSES of 4 (wave w takes tile 4p + w); every pass streams the item's K / V through two LDS buffers of 64 keys (register-staged:
// the next block's loads are in flight under this block's MFMAs and softmax, written to the other buffer behind them, one barrier
// per block).  The step sequence (item, pass, key block) is flat, so the prefetch runs across pass and item seams too.
// Load balance: 257 tokens = 8 x 32 + 1 -> 9 tiles -> passes of 4, 4 and 1 tiles: in the third pass waves 1-3 only stage K / V and
// wait at the barriers (their SIMDs serve the CU's other workgroup meanwhile), and tile 8 computes 32 rows for its one live row.
// 9 of 12 wave-passes compute; K / V are read three times per item, from L2 after the first.  (Tiles per pass for other T:
// 225 -> 8 = 4 + 4; 577 -> 19 = 5 passes, last 3 of 4; 1024 -> 32 = 8 full passes.)
// Keys >= T: the last block's rows beyond T are staged as zeros (a clamped row's load, replaced by zero when written to LDS), their
// scores are set to -inf before the max, and 16-key steps wholly beyond T skip their P V MFMAs.
// q_tiles: query tiles wanted (1 in the class-row-only last block).  A tile's arithmetic does not depend on the other tiles, so the
// class row is bit-identical to an all-rows launch.  LDS: 2 x (K + V) 64-key images + a 32-row output tile per wave = 55,296 B,
// two workgroups per CU.
#define AL_MAXT 1024
#define AL_KB 64
#define AL_BUF (AL_KB * AT_KLD)                                       // halves of one 64-key K (or V) image
#define AL_LDS_BYTES ((4 * AL_BUF + 4 * 32 * AT_KLD) * 2)            // 55,296 B
__global__ __launch_bounds__(256, 2) void k_attention_f16_long(const f16* __restrict__ qkv, f16* __restrict__ out, int T, int W,
                                                               int heads, int ld, int n_items, int q_tiles) {
    extern __shared__ __attribute__((aligned(16))) char al_smem[];   // [buffer 0: K | V][buffer 1: K | V][wave 0..3 output tile]
    f16* const KV = (f16*)al_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    f16* const Os = KV + 4 * AL_BUF + wave * 32 * AT_KLD;
    const int r31 = lane & 31, hh = lane >> 5;
    const int crow = lane >> 3, cpart = lane & 7;
    const int tr_i = lane & 15, tr_g = lane >> 4;
    const int tr_off = ((4 * (tr_g >> 1) + (tr_i >> 2)) * AT_KLD + 16 * (tr_g & 1) + 4 * (tr_i & 3)) * 2;
    const int ntile = (T + 31) / 32;
    const int qt = q_tiles < ntile ? q_tiles : ntile;
    const int npass = (qt + 3) / 4;
    const int nkb = (T + AL_KB - 1) / AL_KB;
    const int per_item = npass * nkb;
    const int my_items = (int)blockIdx.x < n_items ? (n_items - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int nsteps = my_items * per_item;
    if (nsteps == 0) return;                                          // (workgroup-uniform, before any barrier)
    // step s -> (item, pass, key block); all wave-uniform
    auto decode = [&](int s, int& item, int& pass, int& kb) {
        const int u = s / per_item, r = s - u * per_item;
        item = (int)blockIdx.x + u * (int)gridDim.x;
        pass = r / nkb;
        kb = r - pass * nkb;
    };
    uint4 kreg[2];
    f16x8 vreg[2], qn[4];
    // 64 keys x 128 B of K and of V per block: 512 16-byte parts each, thread tid takes parts tid and tid + 256 of both
    auto fetch = [&](int s) {
        int item, pass, kb;
        decode(s, item, pass, kb);
        const int crop = item / heads, head = item - crop * heads;
        const f16* base = qkv + (size_t)crop * T * ld + head * 64;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int c = tid + it * 256, key = kb * AL_KB + (c >> 3), part = c & 7;
            const unsigned off = (unsigned)((key < T ? key : T - 1) * ld + part * 8);
            kreg[it] = *(const uint4*)(base + W + off);
            vreg[it] = *(const f16x8*)(base + 2 * W + off);
        }
        if (kb == 0) {                                                // the pass's Q fragments: row (4 pass + wave) * 32 + r31, clamped
            const int qr = (pass * 4 + wave) * 32 + r31;
            const unsigned off = (unsigned)((qr < T ? qr : T - 1) * ld + hh * 8);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) qn[s4] = *(const f16x8*)(base + off + s4 * 16);
        }
    };
    auto stage = [&](int s) {
        int item, pass, kb;
        decode(s, item, pass, kb);
        f16* const Kb = KV + (s & 1) * 2 * AL_BUF;
        f16* const Vb = Kb + AL_BUF;
        const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int c = tid + it * 256, row = c >> 3, part = c & 7;
            const bool live = kb * AL_KB + row < T;
            *(uint4*)(Kb + row * AT_KLD + part * 8) = live ? kreg[it] : make_uint4(0, 0, 0, 0);
            *(f16x8*)(Vb + row * AT_KLD + part * 8) = live ? vreg[it] : z;
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    const float c2 = 0.125f * 1.4426950408889634f;                   // dh^-0.5 in log2 units
    f16x8 qf[4];
    f32x16 oacc[2];
    float m = -INFINITY, l = 0.f;
    for (int s = 0; s < nsteps; ++s) {
        int item, pass, kb;
        decode(s, item, pass, kb);
        if (kb == 0) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) qf[s4] = qn[s4];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
            m = -INFINITY;
            l = 0.f;
        }
        if (s + 1 < nsteps) fetch(s + 1);                              // in flight during the compute below
        const int tile = pass * 4 + wave;
        if (tile < qt) {
            const f16* const Kb = KV + (s & 1) * 2 * AL_BUF;
            const f16* const Vb = Kb + AL_BUF;
            f32x16 sacc[2];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[h2][r] = 0.f;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const f16x8 kf = *(const f16x8*)(Kb + (h2 * 32 + r31) * AT_KLD + s4 * 16 + hh * 8);
                    sacc[h2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s4], sacc[h2], 0, 0, 0);
                }
            }
            const int k0 = kb * AL_KB;
            if (k0 + AL_KB > T) {                                      // the last block: keys >= T out of the max and the sum
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (k0 + h2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= T) sacc[h2][r] = -INFINITY;
            }
            float mx = m;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[h2][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));                        // finite: key k0 < T is in every block
            const float alpha = __builtin_amdgcn_exp2f((m - mx) * c2); // exp2(-inf) = 0 at the first block
            m = mx;
            const float mc = -mx * c2;
            float ps = 0.f;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[h2][r], c2, mc));
                    sacc[h2][r] = p;
                    ps += p;
                }
            l = fmaf(l, alpha, ps);                                    // this lane's keys; the halves are added at the end
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    if (k0 + h2 * 32 + 16 * s2 >= T) continue;         // 16 keys that do not exist (wave-uniform)
                    f16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (f16)sacc[h2][8 * s2 + j];
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        // A[d][k]: element j <-> key k0 + 32 h2 + 16 s2 + 8(j>>2) + 4hh + (j&3)
                        const char* vb = (const char*)Vb + tr_off + ((h2 * 32 + 16 * s2) * AT_KLD + dt * 32) * 2;
                        const f16x4 lo = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v*)vb));
                        const f16x4 hi = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v*)(vb + 8 * AT_KLD * 2)));
                        const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[dt], 0, 0, 0);
                    }
                }
            if (kb == nkb - 1) {                                       // the pass's last block: O / l -> rows through the wave's tile
                const float inv = 1.0f / (l + __shfl_xor(l, 32));
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f16x4 h4;
#pragma unroll
                        for (int e = 0; e < 4; ++e) h4[e] = (f16)(oacc[dt][4 * g + e] * inv);
                        *(f16x4*)(Os + r31 * AT_KLD + dt * 32 + 8 * g + 4 * hh) = h4;
                    }
                const int crop = item / heads, head = item - crop * heads;
                f16* const obase = out + (size_t)crop * T * W + head * 64;
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int qr = tile * 32 + it * 8 + crow;
                    const f16x8 v = *(const f16x8*)(Os + (it * 8 + crow) * AT_KLD + cpart * 8);
                    if (qr < T) *(f16x8*)(obase + (size_t)qr * W + cpart * 8) = v;
                }
            }
        }
        if (s + 1 < nsteps) stage(s + 1);                              // the other buffer: every wave left it at the last barrier
        __syncthreads();
    }
}

// Measured and dropped (round 4): k_attention_f16_dma -- K and V double-buffered in LDS and filled by LDS-DMA (8-row x 128-byte pieces,
// chunk swizzle by the reversed bits of row >> 1: conflict-free for the K fragment reads and the transposing V reads), the next item
// requested under this item's MFMAs and softmax, no staging phase, one barrier per item, 207 instead of 249 VGPRs.  Two things the
// compiler needed: the transposing reads as inline asm (through the builtin it waits vmcnt(0) in front of the first one: it cannot see
// that the DMA in flight fills the other buffers) and a raw s_barrier (__syncthreads adds vmcnt(0) for the output stores).
// Bit-identical to this kernel; 111.5 vs 114 us per launch alone (337 crops, two interleaved pairs), 65.2 vs 65.2 frames/s in the
// pipeline.  With the whole staging phase gone the item is as long as before: it is bound by the two waves that share a SIMD (seven
// waves on four SIMDs: 2 : 2 : 2 : 1) issuing their softmax and MFMA streams one after the other, not by getting K and V into LDS.
// fp32 parity-mode attention: one workgroup per (crop, head); K,V in LDS; one wave per query row at a time.
// CAUSAL (the text tower): row q sees keys 0 .. q.  A wave's four rows share their key loops, bounded by the last
// of the four (Tk); per row the keys behind its own position stay out of the max and the sum and enter P V as exact zeros, so the fmaf chain
// over the visible keys is the plain kernel's: row i equals, bit for bit, row i of k_attention_f32 on the item's first i + 1 tokens.
template <bool CAUSAL = false>
__global__ __launch_bounds__(256) void k_attention_f32(const float* __restrict__ qkv, float* __restrict__ out, int T,
                                                       int W, int heads) {
    extern __shared__ float sm[];
    float* Ks = sm;                 // [T][65]
    float* Vs = sm + (size_t)T * 65;  // [T][64]
    float* Ps = Vs + (size_t)T * 64;  // [4 waves][4 rows][T]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int crop = blockIdx.x / heads, head = blockIdx.x - crop * heads;
    const size_t row0 = (size_t)crop * T;
    const int ld = 3 * W;
    const float* qbase = qkv + row0 * ld + head * 64;
    for (int c = tid; c < T * 64; c += 256) {
        int key = c >> 6, d = c & 63;
        Ks[key * 65 + d] = qbase[(size_t)key * ld + W + d];
        Vs[key * 64 + d] = qbase[(size_t)key * ld + 2 * W + d];
    }
    __syncthreads();
    // Four query rows per wave at a time (round 4; one row at a time spent an LDS read on every multiply-add: 2.2 ms per layer for 64
    // crops, half of the fp32 tower): a K / V element read from LDS serves four rows, the query and probability values come out of
    // registers as wave-uniform scalars (v_readlane).  Per (row, key) the same fmaf chain over d, per (row, feature) the same chain over
    // the keys as before: the numbers do not change.
    constexpr int QB = 4;
    float* P = Ps + wave * QB * T;
    for (int q0 = wave * QB; q0 < T; q0 += 4 * QB) {
        float qd[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) qd[j] = q0 + j < T ? qbase[(size_t)(q0 + j) * ld + lane] * 0.125f : 0.f;   // q scaled before QK^T like nn.MultiheadAttention
        float mx[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) mx[j] = -INFINITY;
        const int Tk = CAUSAL ? (q0 + QB < T ? q0 + QB : T) : T;            // keys that any of the four rows sees
        for (int k0 = 0; k0 < Tk; k0 += 64) {
            const int key = k0 + lane;
            const float* kr = Ks + (key < T ? key : T - 1) * 65;
            float sacc[QB] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int d = 0; d < 64; ++d) {
                const float kv = kr[d];
#pragma unroll
                for (int j = 0; j < QB; ++j)
                    sacc[j] = fmaf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qd[j]), d)), kv, sacc[j]);
            }
            if (key < Tk) {
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    P[j * T + key] = sacc[j];
                    if (!CAUSAL || key <= q0 + j) mx[j] = fmaxf(mx[j], sacc[j]);
                }
            }
        }
        float sum[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            mx[j] = vg_wave_max(mx[j]);
            float sj = 0.f;
            const int Tj = CAUSAL ? (q0 + j + 1 < Tk ? q0 + j + 1 : Tk) : T;     // keys that row q0 + j sees
            for (int key = lane; key < Tj; key += 64) {
                const float p = expf(P[j * T + key] - mx[j]);
                P[j * T + key] = p;
                sj += p;
            }
            if (CAUSAL) for (int key = Tj + lane; key < Tk; key += 64) P[j * T + key] = 0.f;    // (at most three: the rows behind it in the group)
            sum[j] = vg_wave_sum(sj);
        }
        __builtin_amdgcn_s_waitcnt(0);
        float o[QB] = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Tk; k0 += 64) {
            float pv[QB];
#pragma unroll
            for (int j = 0; j < QB; ++j) pv[j] = k0 + lane < Tk ? P[j * T + k0 + lane] : 0.f;
            const int nk = Tk - k0 < 64 ? Tk - k0 : 64;
            if (nk == 64) {
#pragma unroll
                for (int kk = 0; kk < 64; ++kk) {
                    const float vv = Vs[(k0 + kk) * 64 + lane];
#pragma unroll
                    for (int j = 0; j < QB; ++j)
                        o[j] = fmaf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pv[j]), kk)), vv, o[j]);
                }
            } else {
                for (int kk = 0; kk < nk; ++kk) {
                    const float vv = Vs[(k0 + kk) * 64 + lane];
#pragma unroll
                    for (int j = 0; j < QB; ++j) o[j] = fmaf(__shfl(pv[j], kk), vv, o[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < QB; ++j)
            if (q0 + j < T) out[(row0 + q0 + j) * (size_t)W + head * 64 + lane] = o[j] / sum[j];
    }
}

// one short-sequence attention launch (T <= AT_MAXT): 7 waves per workgroup, at most 256 persistent workgroups
struct AttArgs { const f16* qkv; f16* out; int T, W, heads, ld, items; long long* trace; hipStream_t st; int q_tiles; };
template <bool TRACE, int NKB, int TT = 0, bool TR = false, bool STAG = false, bool CAUSAL = false>
static int launch_attention_short(const AttArgs& a) {
    auto kern = k_attention_f16<TRACE, NKB, TT, TR, STAG, CAUSAL>;
    const int lds = TR ? AT_LDS_BYTES_TR : AT_LDS_BYTES;
    VG_MAX_DYNAMIC_LDS(kern, lds);
    hipLaunchKernelGGL(kern, dim3(a.items < 256 ? a.items : 256), dim3(448), lds, a.st, a.qkv, a.out, a.T, a.W, a.heads, a.ld, a.items, a.trace,
                       a.q_tiles);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

template <bool TRACE>
static int launch_attention(const f16* qkv, f16* out, int T, int W, int heads, int ld, int items, long long* trace, hipStream_t st,
                            int q_tiles = 7, AttOptions opt = AttOptions()) {
    if (T > AT_MAXT && !TRACE) {                 // ViT-L/14 and other long token counts: the flash-style kernel
        if (T > AL_MAXT) return VG_ERR_ARG;
        const int cap = 2 * vg_cu_count();       // persistent: two workgroups per CU
        VG_MAX_DYNAMIC_LDS(k_attention_f16_long, AL_LDS_BYTES);
        hipLaunchKernelGGL(k_attention_f16_long, dim3(items < cap ? items : cap), dim3(256), AL_LDS_BYTES, st, qkv, out, T, W, heads, ld, items, q_tiles);
        VG_LAUNCH_CHECK();
        return VG_OK;
    }
    const int nkb = (T + 31) / 32;
    if (nkb < 1 || nkb > 7) return VG_ERR_ARG;
    const AttArgs a{qkv, out, T, W, heads, ld, items, trace, st, q_tiles};
    if (T == 197 && !TRACE) {
        // ViT-B/16: row-major V + transposing LDS reads (VG_ATT_TR=0: the transposed V image of rounds 1-2; same numbers, 1.6 % slower)
        // (opt: vg_vit::att of the calling handle; tests run the paths in one process and compare them bit for bit)
        if (opt.tr && opt.stagger) return launch_attention_short<false, 7, 197, true, true>(a);
        if (opt.tr) return launch_attention_short<false, 7, 197, true>(a);
        return launch_attention_short<false, 7, 197>(a);
    }
    switch (nkb) {
        case 1: return launch_attention_short<TRACE, 1>(a);
        case 2: return launch_attention_short<TRACE, 2>(a);
        case 3: return launch_attention_short<TRACE, 3>(a);
        case 4: return launch_attention_short<TRACE, 4>(a);
        case 5: return launch_attention_short<TRACE, 5>(a);
        case 6: return launch_attention_short<TRACE, 6>(a);
        default: return launch_attention_short<TRACE, 7>(a);
    }
}

// the causal form (text tower, T <= AT_MAXT): every query tile, the transposed V image, no token-count constant
static int launch_attention_causal(const f16* qkv, f16* out, int T, int W, int heads, int ld, int items, hipStream_t st) {
    const int nkb = (T + 31) / 32;
    if (T < 1 || T > AT_MAXT) return VG_ERR_ARG;
    const AttArgs a{qkv, out, T, W, heads, ld, items, nullptr, st, nkb};
    switch (nkb) {
        case 1: return launch_attention_short<false, 1, 0, false, false, true>(a);
        case 2: return launch_attention_short<false, 2, 0, false, false, true>(a);
        case 3: return launch_attention_short<false, 3, 0, false, false, true>(a);
        case 4: return launch_attention_short<false, 4, 0, false, false, true>(a);
        case 5: return launch_attention_short<false, 5, 0, false, false, true>(a);
        case 6: return launch_attention_short<false, 6, 0, false, false, true>(a);
        default: return launch_attention_short<false, 7, 0, false, false, true>(a);
    }
}

// k_attention_f32 (plain / causal): one workgroup per item; K, V and four probability rows per wave within the 160 KiB it requests
static int launch_attention_f32(bool causal, const float* qkv, float* out, int T, int W, int heads, int items, hipStream_t st) {
    const size_t lds = ((size_t)T * 65 + (size_t)T * 64 + 16 * (size_t)T) * sizeof(float);
    if (T < 1 || lds > 160 * 1024) return VG_ERR_ARG;
    if (causal) {
        VG_MAX_DYNAMIC_LDS(k_attention_f32<true>, 160 * 1024);
        hipLaunchKernelGGL(k_attention_f32<true>, dim3(items), dim3(256), lds, st, qkv, out, T, W, heads);
    } else {
        VG_MAX_DYNAMIC_LDS(k_attention_f32<false>, 160 * 1024);
        hipLaunchKernelGGL(k_attention_f32<false>, dim3(items), dim3(256), lds, st, qkv, out, T, W, heads);
    }
    VG_LAUNCH_CHECK();
    return VG_OK;
}
