// Cluster packing on the device: LidarFrame.generate_detections' grouping (src/vilgod/lidar_frame.py:163-167, 230-237) and the valid
// sub-lists that classification and the box fit read -- vg_pack_clusters / vg_pack_select of include/vilgod_hip.h.
//
// vg_pack_clusters is a stable least-significant-digit radix sort of (label, point index) over only the bits `label_bound` needs, 8 bits
// a pass, with the keep / drop decision folded into the first pass (dropped points are never counted, so the first pass is also the
// compaction).  A pass is three launches:
//   k_pack_hist     per tile of 2048 elements: how many kept elements carry each digit            -> hist[digit][tile]
//   k_pack_scan     exclusive scan of hist in (digit, tile) order = where each tile's run of a digit starts; the total = kept points
//   k_pack_scatter  every element to  start[digit][tile] + its rank among the tile's elements of that digit
// The rank comes from the element's POSITION: a wave walks its 512 consecutive elements 64 at a time, ballots find the lanes of the
// chunk with the same digit, rank = (elements of that digit in the wave's earlier chunks) + (lower lanes with the digit), and the four
// waves' counts are prefixed in wave order.  Nothing depends on the order in which atomics arrive (the histogram's LDS atomics only
// add), so the result is the same bits on every run: labels ascending, point indices ascending inside a label.
// The sorted labels then give the clusters: a head is an element whose label differs from its predecessor's; heads are counted per
// tile, scanned, and written as ids / segment offsets (three more launches).  No host work, no synchronisation, no allocation.
#include "common.h"
#include "vilgod_hip.h"

namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_WAVES = PK_THREADS / WAVE;
constexpr int PK_CHUNKS = 8;                              // 64-element chunks a wave walks
constexpr int PK_TILE = PK_THREADS * PK_CHUNKS;           // 2048
constexpr int PK_RADIX = 256;
constexpr int PK_HEAD_ITEMS = 4;                          // consecutive sorted elements per thread in the head kernels
constexpr int PK_HEAD_TILE = PK_THREADS * PK_HEAD_ITEMS;  // 1024
constexpr int PK_SCAN_THREADS = 1024;
constexpr int PK_MAX_N = 1 << 24;
constexpr int PK_MAX_BOUND = 1 << 24;

// device-side state of one call, at the start of the work buffer
struct PackState {
    int32_t kept;         // points that survive the keep / drop decision (= P)
    int32_t clusters;     // C
    int32_t overflow;     // some label >= label_bound
    int32_t pad;
};

__device__ __forceinline__ uint64_t pk_lanes_below() {
    const int lane = threadIdx.x & (WAVE - 1);
    return lane == 0 ? 0ull : (~0ull >> (WAVE - lane));
}

// pass 0 reads the caller's labels / probabilities, later passes the previous pass' (key, value) lists
template <bool FIRST>
__device__ __forceinline__ bool pk_load(const int32_t* __restrict__ keys, const int32_t* __restrict__ vals, const double* __restrict__ probs,
                                        double threshold, int label_bound, int count, int e, int32_t& key, int32_t& val, bool& over) {
    if (e >= count) return false;
    if (FIRST) {
        key = keys[e];
        val = e;
        if (key < 0) return false;
        if (key >= label_bound) {
            over = true;
            return false;
        }
        if (probs != nullptr && probs[e] < threshold) return false;      // strict <: a NaN probability keeps the point (numpy's mask)
        return true;
    }
    key = keys[e];
    val = vals != nullptr ? vals[e] : 0;              // (the histogram pass reads the keys only)
    return true;
}

template <bool FIRST>
__global__ __launch_bounds__(PK_THREADS) void k_pack_hist(const int32_t* __restrict__ keys, const double* __restrict__ probs, double threshold,
                                                          int label_bound, int n, int shift, int tiles, PackState* __restrict__ st,
                                                          int32_t* __restrict__ hist) {
    __shared__ int32_t cnt[PK_RADIX];
    const int tile = blockIdx.x;
    const int count = FIRST ? n : st->kept;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    bool over = false;
#pragma unroll
    for (int c = 0; c < PK_CHUNKS; ++c) {
        const int e = tile * PK_TILE + c * PK_THREADS + threadIdx.x;
        int32_t key = 0, val = 0;
        if (pk_load<FIRST>(keys, nullptr, probs, threshold, label_bound, count, e, key, val, over))
            atomicAdd(&cnt[(key >> shift) & (PK_RADIX - 1)], 1);
    }
    __syncthreads();
    hist[threadIdx.x * tiles + tile] = cnt[threadIdx.x];
    if (FIRST && over) st->overflow = 1;           // every writer stores the same value
}

// exclusive scan of data[0 .. count) in place by one workgroup; *total = the sum
__global__ __launch_bounds__(PK_SCAN_THREADS) void k_pack_scan(int32_t* __restrict__ data, int count, int32_t* __restrict__ total) {
    __shared__ int32_t wsum[PK_SCAN_THREADS / WAVE];
    __shared__ int32_t carry_s;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < count; base += PK_SCAN_THREADS * 4) {
        const int i0 = base + threadIdx.x * 4;
        int32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < count ? data[i0 + k] : 0;
        const int32_t mine = v[0] + v[1] + v[2] + v[3];
        int32_t inc = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int32_t up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == WAVE - 1) wsum[wave] = inc;
        __syncthreads();
        int32_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        int32_t run = before + inc - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < count) data[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (threadIdx.x == PK_SCAN_THREADS - 1) carry_s = run;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

template <bool FIRST>
__global__ __launch_bounds__(PK_THREADS) void k_pack_scatter(const int32_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                             const double* __restrict__ probs, double threshold, int label_bound, int n, int shift,
                                                             int tiles, const PackState* __restrict__ st, const int32_t* __restrict__ start,
                                                             int32_t* __restrict__ out_keys, int32_t* __restrict__ out_vals) {
    __shared__ int32_t wcnt[PK_WAVES][PK_RADIX];           // per wave: elements of each digit seen so far; then the wave's first position
    const int tile = blockIdx.x;
    const int count = FIRST ? n : st->kept;
    if (tile * PK_TILE >= count) return;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    volatile int32_t* mine = wcnt[wave];
#pragma unroll
    for (int w = 0; w < PK_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t below = pk_lanes_below();
    int32_t key[PK_CHUNKS], val[PK_CHUNKS], rank[PK_CHUNKS];
    bool over = false;
#pragma unroll
    for (int c = 0; c < PK_CHUNKS; ++c) {
        const int e = tile * PK_TILE + wave * (PK_CHUNKS * WAVE) + c * WAVE + lane;
        key[c] = val[c] = 0;
        const bool ok = pk_load<FIRST>(keys, vals, probs, threshold, label_bound, count, e, key[c], val[c], over);
        const int digit = (key[c] >> shift) & (PK_RADIX - 1);
        uint64_t same = __ballot(ok);                      // the chunk's kept lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1;
            const uint64_t has = __ballot(ok && bit);
            same &= bit ? has : ~has;
        }
        rank[c] = -1;
        if (ok) {
            const int32_t seen = mine[digit];
            rank[c] = seen + __popcll(same & below);
            if (((same >> lane) >> 1) == 0) mine[digit] = seen + __popcll(same);      // the digit's highest lane of the chunk
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // thread t owns digit t: the tile's run of the digit starts at start[t][tile]; the waves follow each other inside it
        int32_t at = start[threadIdx.x * tiles + tile];
#pragma unroll
        for (int w = 0; w < PK_WAVES; ++w) {
            const int32_t c_ = wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = at;
            at += c_;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < PK_CHUNKS; ++c) {
        if (rank[c] >= 0) {
            const int pos = wcnt[wave][(key[c] >> shift) & (PK_RADIX - 1)] + rank[c];
            out_keys[pos] = key[c];
            out_vals[pos] = val[c];
        }
    }
}

// heads of the sorted labels: element j starts a cluster when j == 0 or its label differs from the one before it
__device__ __forceinline__ int pk_heads(const int32_t* __restrict__ keys, int count, int j0, int32_t (&k)[PK_HEAD_ITEMS], bool (&head)[PK_HEAD_ITEMS]) {
    int32_t prev = (j0 > 0 && j0 < count) ? keys[j0 - 1] : -1;
    int h = 0;
#pragma unroll
    for (int i = 0; i < PK_HEAD_ITEMS; ++i) {
        const int j = j0 + i;
        k[i] = j < count ? keys[j] : -1;
        head[i] = j < count && (j == 0 || k[i] != prev);
        h += head[i];
        prev = k[i];
    }
    return h;
}

__global__ __launch_bounds__(PK_THREADS) void k_pack_head_count(const int32_t* __restrict__ keys, const PackState* __restrict__ st,
                                                                int32_t* __restrict__ tile_heads) {
    __shared__ int32_t wsum[PK_WAVES];
    const int count = st->kept;
    int32_t k[PK_HEAD_ITEMS];
    bool head[PK_HEAD_ITEMS];
    int h = 0;
    if (blockIdx.x * PK_HEAD_TILE < count) h = pk_heads(keys, count, blockIdx.x * PK_HEAD_TILE + threadIdx.x * PK_HEAD_ITEMS, k, head);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = h;
    __syncthreads();
    if (threadIdx.x == 0) tile_heads[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(PK_THREADS) void k_pack_head_write(const int32_t* __restrict__ keys, const PackState* __restrict__ st,
                                                                const int32_t* __restrict__ tile_start, int64_t* __restrict__ ids,
                                                                int32_t* __restrict__ seg, int32_t* __restrict__ counts) {
    __shared__ int32_t wsum[PK_WAVES];
    const int count = st->kept;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        seg[st->clusters] = count;                         // seg[C] = P (C == 0: seg[0] = 0)
        counts[0] = st->clusters;
        counts[1] = count;
        counts[2] = st->overflow;
    }
    if (blockIdx.x * PK_HEAD_TILE >= count) return;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int j0 = blockIdx.x * PK_HEAD_TILE + threadIdx.x * PK_HEAD_ITEMS;
    int32_t k[PK_HEAD_ITEMS];
    bool head[PK_HEAD_ITEMS];
    const int h = pk_heads(keys, count, j0, k, head);
    int inc = h;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    int c = tile_start[blockIdx.x] + inc - h;
    for (int w = 0; w < wave; ++w) c += wsum[w];
#pragma unroll
    for (int i = 0; i < PK_HEAD_ITEMS; ++i) {
        if (head[i]) {
            ids[c] = k[i];
            seg[c] = j0 + i;
            ++c;
        }
    }
}

// ---- vg_pack_select ----------------------------------------------------------------------------------------------------------------
// one workgroup: exclusive scan of the kept clusters' sizes -> out_seg, and every cluster's destination (or -1) for the copy
__global__ __launch_bounds__(PK_SCAN_THREADS) void k_pack_select_scan(const int32_t* __restrict__ seg, const uint8_t* __restrict__ valid, int n_clusters,
                                                                      int32_t* __restrict__ dst, int32_t* __restrict__ out_seg,
                                                                      int32_t* __restrict__ counts) {
    __shared__ int32_t wsum_p[PK_SCAN_THREADS / WAVE], wsum_c[PK_SCAN_THREADS / WAVE];
    __shared__ int32_t carry_p, carry_c;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) carry_p = carry_c = 0;
    __syncthreads();
    for (int base = 0; base < n_clusters; base += PK_SCAN_THREADS) {
        const int c = base + threadIdx.x;
        const bool keep = c < n_clusters && valid[c] != 0;
        const int32_t len = keep ? seg[c + 1] - seg[c] : 0;
        int32_t inc_p = len, inc_c = keep;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int32_t up_p = __shfl_up(inc_p, o), up_c = __shfl_up(inc_c, o);
            if (lane >= o) {
                inc_p += up_p;
                inc_c += up_c;
            }
        }
        if (lane == WAVE - 1) {
            wsum_p[wave] = inc_p;
            wsum_c[wave] = inc_c;
        }
        __syncthreads();
        int32_t bp = carry_p, bc = carry_c;
        for (int w = 0; w < wave; ++w) {
            bp += wsum_p[w];
            bc += wsum_c[w];
        }
        if (c < n_clusters) dst[c] = keep ? bp + inc_p - len : -1;
        if (keep) out_seg[bc + inc_c - 1] = bp + inc_p - len;
        __syncthreads();
        if (threadIdx.x == PK_SCAN_THREADS - 1) {
            carry_p = bp + inc_p;
            carry_c = bc + inc_c;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_seg[carry_c] = carry_p;
        counts[0] = carry_c;
        counts[1] = carry_p;
    }
}

// one thread per packed point: its cluster by bisection of seg, then the copy to the cluster's destination
__global__ __launch_bounds__(PK_THREADS) void k_pack_select_copy(const int32_t* __restrict__ index, const int32_t* __restrict__ seg, int n_clusters,
                                                                 int n_index, const int32_t* __restrict__ dst, int32_t* __restrict__ out_index) {
    const int j = blockIdx.x * PK_THREADS + threadIdx.x;
    int total = seg[n_clusters];
    if (total > n_index) total = n_index;
    if (j >= total) return;
    int lo = 0, hi = n_clusters - 1;                       // the last c with seg[c] <= j (empty segments are skipped by taking the last)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    const int32_t d = dst[lo];
    if (d >= 0) out_index[d + (j - seg[lo])] = index[j];
}

inline int64_t pk_align(int64_t b) { return (b + 255) & ~int64_t(255); }
inline int pk_tiles(int n) { return n > 0 ? vg_div_up(n, PK_TILE) : 1; }
inline int pk_head_tiles(int n) { return n > 0 ? vg_div_up(n, PK_HEAD_TILE) : 1; }

}  // namespace

extern "C" int64_t vg_pack_clusters_work_bytes(int n) {
    if (n < 0 || n > PK_MAX_N) return -1;
    // state | hist [256][tiles] | head counts [head tiles] | keys A, keys B, values A, values B [n each]
    return pk_align(sizeof(PackState)) + pk_align(int64_t(PK_RADIX) * pk_tiles(n) * 4) + pk_align(int64_t(pk_head_tiles(n)) * 4) +
           4 * pk_align(int64_t(n > 0 ? n : 1) * 4);
}

extern "C" int vg_pack_clusters(const int32_t* d_labels, const double* d_probs, int n, double threshold, int label_bound, void* d_work,
                                int64_t work_bytes, int64_t* d_ids, int32_t* d_index, int32_t* d_seg, int32_t* d_counts, void* stream) {
    if (n < 0 || n > PK_MAX_N || label_bound < 0 || label_bound > PK_MAX_BOUND) return VG_ERR_ARG;
    if (!d_work || !d_seg || !d_counts || (n > 0 && (!d_labels || !d_ids || !d_index))) return VG_ERR_ARG;
    if (work_bytes < vg_pack_clusters_work_bytes(n)) return VG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int tiles = pk_tiles(n), head_tiles = pk_head_tiles(n);
    char* w = (char*)d_work;
    PackState* st = (PackState*)w;
    w += pk_align(sizeof(PackState));
    int32_t* hist = (int32_t*)w;
    w += pk_align(int64_t(PK_RADIX) * tiles * 4);
    int32_t* tile_heads = (int32_t*)w;
    w += pk_align(int64_t(head_tiles) * 4);
    const int64_t list = pk_align(int64_t(n > 0 ? n : 1) * 4);
    int32_t* keys[2] = {(int32_t*)w, (int32_t*)(w + list)};
    int32_t* vals[2] = {(int32_t*)(w + 2 * list), (int32_t*)(w + 3 * list)};

    int bits = 0;
    while (bits < 31 && (1ll << bits) < label_bound) ++bits;            // labels < label_bound fit in `bits` bits
    const int passes = bits > 16 ? 3 : bits > 8 ? 2 : 1;
    VG_CHECK(hipMemsetAsync(st, 0, sizeof(PackState), s));
    for (int p = 0; p < passes; ++p) {
        const bool last = p == passes - 1;
        const int shift = 8 * p;
        int32_t* out_k = keys[p & 1];
        int32_t* out_v = last ? d_index : vals[p & 1];
        if (p == 0) {
            k_pack_hist<true><<<tiles, PK_THREADS, 0, s>>>(d_labels, d_probs, threshold, label_bound, n, shift, tiles, st, hist);
            k_pack_scan<<<1, PK_SCAN_THREADS, 0, s>>>(hist, PK_RADIX * tiles, &st->kept);
            k_pack_scatter<true><<<tiles, PK_THREADS, 0, s>>>(d_labels, nullptr, d_probs, threshold, label_bound, n, shift, tiles, st, hist, out_k, out_v);
        } else {
            const int32_t* in_k = keys[(p - 1) & 1];
            const int32_t* in_v = vals[(p - 1) & 1];
            k_pack_hist<false><<<tiles, PK_THREADS, 0, s>>>(in_k, nullptr, 0.0, 0, n, shift, tiles, st, hist);
            k_pack_scan<<<1, PK_SCAN_THREADS, 0, s>>>(hist, PK_RADIX * tiles, &st->pad);
            k_pack_scatter<false><<<tiles, PK_THREADS, 0, s>>>(in_k, in_v, nullptr, 0.0, 0, n, shift, tiles, st, hist, out_k, out_v);
        }
        VG_LAUNCH_CHECK();
    }
    const int32_t* sorted = keys[(passes - 1) & 1];
    k_pack_head_count<<<head_tiles, PK_THREADS, 0, s>>>(sorted, st, tile_heads);
    k_pack_scan<<<1, PK_SCAN_THREADS, 0, s>>>(tile_heads, head_tiles, &st->clusters);
    k_pack_head_write<<<head_tiles, PK_THREADS, 0, s>>>(sorted, st, tile_heads, d_ids, d_seg, d_counts);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

extern "C" int64_t vg_pack_select_work_bytes(int n_clusters) {
    if (n_clusters < 0) return -1;
    return pk_align(int64_t(n_clusters > 0 ? n_clusters : 1) * 4);
}

extern "C" int vg_pack_select(const int32_t* d_index, const int32_t* d_seg, int n_clusters, int n_index, const uint8_t* d_valid, void* d_work,
                              int64_t work_bytes, int32_t* d_out_index, int32_t* d_out_seg, int32_t* d_counts, void* stream) {
    if (n_clusters < 0 || n_index < 0) return VG_ERR_ARG;
    if (!d_seg || !d_work || !d_out_seg || !d_counts) return VG_ERR_ARG;
    if (n_clusters > 0 && !d_valid) return VG_ERR_ARG;
    if (n_index > 0 && (!d_index || !d_out_index)) return VG_ERR_ARG;
    if (work_bytes < vg_pack_select_work_bytes(n_clusters)) return VG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int32_t* dst = (int32_t*)d_work;
    k_pack_select_scan<<<1, PK_SCAN_THREADS, 0, s>>>(d_seg, d_valid, n_clusters, dst, d_out_seg, d_counts);
    if (n_clusters > 0 && n_index > 0)
        k_pack_select_copy<<<vg_div_up(n_index, PK_THREADS), PK_THREADS, 0, s>>>(d_index, d_seg, n_clusters, n_index, dst, d_out_index);
    VG_LAUNCH_CHECK();
    return VG_OK;
}
