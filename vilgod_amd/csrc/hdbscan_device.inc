// HDBSCAN hierarchy stage as data-parallel rules (round 6; SURVEY §8a row B2, kernel list K2d): the per-element bodies of the kernels of
// hdbscan_device.hip.  Same results, bit for bit, as the sequential host stage vg_hdbscan_tree_host (hdbscan_tree.cpp: single linkage ->
// condense -> stability -> excess of mass -> cluster_selection_epsilon -> labels / probabilities, the semantics of the library the
// reference calls, src/vilgod/zero_shot_detector.py:248), without its union-find over all n - 1 edges.
//
// This file is compiled twice: by hipcc into the kernels (HD_DEVICE defined), and by g++ into the CPU test-suite's emulation of the same
// bodies (tests/emul/hdbscan_device_emul.cpp: every "thread" of a phase in a loop) -- the rules are checked against the host stage on
// random trees without a GPU, the kernels on the GPU against both.
//
// rank = position of an edge in the (w2, lo, hi) order = its dendrogram node.  "side of u at edge e" = the vertices u reaches over
// tree edges of lower rank than e.  mcs = min_cluster_size.
//   R1  node e is a TRUE SPLIT iff both of its sides hold >= mcs vertices (two walks of at most mcs vertices);
//       it is a CHAIN node iff it is no split and the two sides together hold >= mcs.
//   R2  a point leaves its cluster at a(p) = the chain node on whose SMALL side (< mcs vertices) it lies: every point lies on exactly
//       one such side (the node at which its component first reaches mcs vertices); lambda_p = 1 / dist(a(p)).
//   R3  a non-split edge has a side without splits, so contracting ALL of them first (the tree falls into SEGMENTS) changes no ancestry
//       between splits: Kruskal over the split edges alone -- a few hundred -- on the segments gives the cluster tree.
//   R4  the cluster of a chain node j: from its segment's lowest-rank split upward, the first split of larger rank than j -- that
//       split's child on this side; none: the root cluster.
//   R5  the library numbers clusters in BFS order of the DENDROGRAM: depth of a split = depth of its cluster's top node + the cluster's
//       number of chain nodes; order inside a depth = preorder of the split tree, left (= the `lo` endpoint's side) first.
//   R6  stability is summed in the library's row order: per cluster its chain nodes by descending rank, k_j equal terms each, then the
//       two child rows; excess of mass, epsilon and the labels are walks over the (small) cluster tree.
// Provisional cluster ids: 0 = root, 1 + 2 k + side = child of split k (k = index among the splits in rank order).
#ifndef VG_HDBSCAN_DEVICE_INC
#define VG_HDBSCAN_DEVICE_INC
#include <math.h>
#include <stdint.h>

#ifdef HD_DEVICE
#define HD_FN __device__ __forceinline__
HD_FN unsigned hd_atomic_min_u32(unsigned* p, unsigned v) { return atomicMin(p, v); }
HD_FN int hd_atomic_add_i32(int* p, int v) { return atomicAdd(p, v); }
HD_FN int hd_atomic_cas_i32(int* p, int cmp, int v) { return atomicCAS(p, cmp, v); }
HD_FN unsigned long long hd_atomic_max_u64(unsigned long long* p, unsigned long long v) { return atomicMax(p, v); }
HD_FN int hd_load_i32(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
HD_FN void hd_store_i32(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
HD_FN unsigned long long hd_double_bits(double x) { return (unsigned long long)__double_as_longlong(x); }
HD_FN double hd_bits_double(unsigned long long b) { return __longlong_as_double((long long)b); }
#else
#include <string.h>
#define HD_FN static inline
HD_FN unsigned hd_atomic_min_u32(unsigned* p, unsigned v) { unsigned o = *p; if (v < o) *p = v; return o; }
HD_FN int hd_atomic_add_i32(int* p, int v) { int o = *p; *p = o + v; return o; }
HD_FN int hd_atomic_cas_i32(int* p, int cmp, int v) { int o = *p; if (o == cmp) *p = v; return o; }
HD_FN unsigned long long hd_atomic_max_u64(unsigned long long* p, unsigned long long v) { unsigned long long o = *p; if (v > o) *p = v; return o; }
HD_FN int hd_load_i32(const int* p) { return *p; }
HD_FN void hd_store_i32(int* p, int v) { *p = v; }
HD_FN unsigned long long hd_double_bits(double x) { unsigned long long b; memcpy(&b, &x, 8); return b; }
HD_FN double hd_bits_double(unsigned long long b) { double x; memcpy(&x, &b, 8); return x; }
#endif

#define HD_MAX_MCS 32            // walk stacks hold min_cluster_size frames per thread
#define HD_RANK_BITS 20          // n <= 2^20 points: sort keys pack a rank below a vertex / cluster number
#define HD_SPLIT 1u
#define HD_CHAIN 2u

struct HdChainRec {                  // per edge, written once its cluster is known: everything the later kernels read of a chain node
    int c;                           // provisional cluster; -1: the edge is no chain node
    int kc;                          // points that leave here
    double lam;                      // 1 / dist
};

struct HdView {
    int n, m, mcs, ncap;             // ncap: capacity of the per-split arrays (>= n / mcs + 2)
    double eps;
    const int* lo;                   // [m] edges in (w2, lo, hi) order
    const int* hi;
    const double* w2;
    const int* adj_off;              // [n + 1]
    const unsigned long long* adj;   // [2 m] per vertex, ascending rank: rank << 32 | other endpoint
    unsigned char* side;             // [2 m] vertices on the side of lo (2 r) / hi (2 r + 1) at edge r, capped at mcs
    unsigned char* eflag;            // [m] HD_SPLIT | HD_CHAIN
    int* kcnt;                       // [m] chain nodes: the points that leave here (the small sides' vertices)
    int* a;                          // [n] rank of the chain node at which the point leaves
    int* uf;                         // [n] union-find over the non-split edges; flattened: the segment's root vertex
    int* split_pos;                  // [m] exclusive scan of the split flags (filled by the caller between phases)
    int* S;                          // [ncap] rank of split k
    int* ns;                         // [1] number of splits
    unsigned* first;                 // [n] per segment root: min (k << 1 | side) over the splits at the segment
    int* node;                       // [2 ncap] union-find node of (split k, side) = first[segment of that endpoint]
    int* sp_parent;                  // [ncap] parent split (-1: the root split = the last one)
    int* sp_side;                    // [ncap] side of the parent this split hangs on
    int* kid;                        // [2 ncap] split below (k, side) or -1
    HdChainRec* crec;                // [m]
    double* lam_split;               // [ncap] lambda of split k = the birth of its two children
    int* chainlen;                   // [2 ncap + 1] chain nodes per cluster
    int* npts;                       // [2 ncap + 1] points that leave the cluster on its own chain
    double* death;                   // [2 ncap + 1] the largest lambda among the cluster's rows
    const unsigned* chain_key;       // [m] sorted hd_chain_sortkey
    const unsigned* chain_rank;      // [m] ... and the ranks in that order (ascending inside a cluster)
    // cluster tree work (hd_clusters_*)
    int* kw_parent;                  // [2 ncap] Kruskal union-find over nodes (global-memory form)
    int* kw_top;                     // [2 ncap]
    int* nsub;                       // [ncap] splits in the subtree of split k
    int* tot;                        // [ncap] points under split k
    int* csize;                      // [2 ncap + 1] points under the cluster
    int* depth;                      // [ncap] dendrogram depth of the split node
    int* pre;                        // [ncap] preorder index in the split tree
    int* q;                          // [ncap] BFS position
    int* done;                       // [2 ncap + 1] relaxation flags
    double* stab;                    // [2 ncap + 1] first the chain's rows (hd_chain_stats), then all rows (hd_up_all)
    double* stab2;                   // [2 ncap + 1] after excess of mass
    unsigned char* wins;             // [2 ncap + 1]
    unsigned char* selected;         // [2 ncap + 1]
    unsigned char* cand;             // [2 ncap + 1]
    int* sel_by_final;               // [2 ncap + 2]
    int* out_label;                  // [2 ncap + 1] provisional cluster -> flat label or -1
    double* out_death;               // [2 ncap + 1] ... and the owner's largest lambda
    int* n_clusters;                 // [1]
    int* labels;                     // [n]
    double* probs;                   // [n]
    // the library's cluster-selection options (zero: excess of mass, the root never selected, no size limit)
    int leaf;                        // cluster_selection_method = 'leaf'
    int allow_single;                // allow_single_cluster
    int max_size;                    // max_cluster_size; 0: unlimited
};

// The strict (w2, lo, hi) order from the weight order: edge i of the weight-sorted input moves, inside its run of equal weights, to the
// place its (lo, hi) pair has among the run's pairs.  Runs are short (the edges that share one point's core distance); a run of L edges
// costs L steps per edge.
HD_FN int hd_tie_position(const int* lo, const int* hi, const double* w2, int m, int i) {
    const double w = w2[i];
    int s = i, e = i + 1;
    while (s > 0 && w2[s - 1] == w) --s;
    while (e < m && w2[e] == w) ++e;
    if (e - s == 1) return i;
    const unsigned long long key = ((unsigned long long)(unsigned)lo[i] << 32) | (unsigned)hi[i];
    int pos = s;
    for (int j = s; j < e; ++j) pos += ((((unsigned long long)(unsigned)lo[j] << 32) | (unsigned)hi[j]) < key) ? 1 : 0;
    return pos;
}

HD_FN double hd_lambda(double w2) {                  // (hdbscan_tree.cpp: dist = sqrt(w2), lambda = dist > 0 ? 1 / dist : inf)
    const double d = sqrt(w2);
    return d > 0.0 ? 1.0 / d : INFINITY;
}

// ---- R1 / R2: the walk over one side -----------------------------------------------------------------------------------------------
// Vertices u reaches over edges of rank < r without stepping back to `from`, counted up to mcs.  mark >= 0: every vertex is given
// a[x] = mark (the caller knows the side is small).  st: this thread's stack, element d at st[d * stride]: vertex and cursor into adj.
HD_FN int hd_walk(const HdView& v, int u, int from, int r, int mark, int* st_x, int* st_i, int stride) {
    int cnt = 1, sp = 0;
    if (mark >= 0) v.a[u] = mark;
    if (cnt >= v.mcs) return v.mcs;
    st_x[0] = u; st_i[0] = v.adj_off[u];
    sp = 1;
    while (sp > 0) {
        const int x = st_x[(sp - 1) * stride];
        const int i = st_i[(sp - 1) * stride];
        if (i >= v.adj_off[x + 1]) { --sp; continue; }
        const unsigned long long e = v.adj[i];
        const int rr = (int)(e >> 32), y = (int)(e & 0xffffffffu);
        if (rr >= r) { --sp; continue; }              // ascending ranks: nothing further at x
        st_i[(sp - 1) * stride] = i + 1;
        const int f = sp >= 2 ? st_x[(sp - 2) * stride] : from;
        if (y == f) continue;
        ++cnt;
        if (mark >= 0) v.a[y] = mark;
        if (cnt >= v.mcs) return v.mcs;
        st_x[sp * stride] = y; st_i[sp * stride] = v.adj_off[y];     // (cnt < mcs: at most mcs - 1 frames)
        ++sp;
    }
    return cnt;
}

// phase: i in [0, 2 m)
HD_FN void hd_side_count(const HdView& v, int i, int* st_x, int* st_i, int stride) {
    const int r = i >> 1, sd = i & 1;
    const int u = sd ? v.hi[r] : v.lo[r], w = sd ? v.lo[r] : v.hi[r];
    v.side[i] = (unsigned char)hd_walk(v, u, w, r, -1, st_x, st_i, stride);
}

// phase: i in [0, 2 m)
HD_FN void hd_side_assign(const HdView& v, int i, int* st_x, int* st_i, int stride) {
    const int r = i >> 1, sd = i & 1;
    const int su = v.side[2 * r], sv = v.side[2 * r + 1];
    const bool split = su >= v.mcs && sv >= v.mcs, chain = !split && su + sv >= v.mcs;
    if (sd == 0) {
        v.eflag[r] = (unsigned char)((split ? HD_SPLIT : 0u) | (chain ? HD_CHAIN : 0u));
        v.kcnt[r] = chain ? (su < v.mcs ? su : 0) + (sv < v.mcs ? sv : 0) : 0;
    }
    if (chain && (sd ? sv : su) < v.mcs) {
        const int u = sd ? v.hi[r] : v.lo[r], w = sd ? v.lo[r] : v.hi[r];
        hd_walk(v, u, w, r, r, st_x, st_i, stride);
    }
}

// ---- R3: segments (lock-free union-find over the non-split edges) -------------------------------------------------------------------
HD_FN int hd_find(int* uf, int x) {
    int p = hd_load_i32(&uf[x]);
    while (p != x) {
        const int g = hd_load_i32(&uf[p]);
        if (g != p) hd_store_i32(&uf[x], g);          // path halving (a stale write still points at an ancestor)
        x = p; p = g;
    }
    return x;
}
// phase: r in [0, m)   (uf[x] = x before)
HD_FN void hd_segment_union(const HdView& v, int r) {
    if (v.eflag[r] & HD_SPLIT) return;
    int a = v.lo[r], b = v.hi[r];
    while (true) {
        a = hd_find(v.uf, a); b = hd_find(v.uf, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }  // the larger root goes under the smaller
        if (hd_atomic_cas_i32(&v.uf[a], a, b) == a) return;
    }
}
// phase: x in [0, n)   (after: uf[x] = the segment's root)
HD_FN void hd_segment_flatten(const HdView& v, int x) {
    int r = x;
    while (true) { const int p = hd_load_i32(&v.uf[r]); if (p == r) break; r = p; }
    hd_store_i32(&v.uf[x], r);                         // (a concurrent reader sees x's old parent or the root: both on the path)
    v.first[x] = 0xFFFFFFFFu;
}

// phase: r in [0, m), after the scan of the split flags
HD_FN void hd_split_scatter(const HdView& v, int r) {
    if (r == v.m - 1) *v.ns = v.split_pos[r] + ((v.eflag[r] & HD_SPLIT) ? 1 : 0);
    if (!(v.eflag[r] & HD_SPLIT)) return;
    const int k = v.split_pos[r];
    v.S[k] = r;
    v.lam_split[k] = hd_lambda(v.w2[r]);
    hd_atomic_min_u32(&v.first[v.uf[v.lo[r]]], (unsigned)(2 * k));
    hd_atomic_min_u32(&v.first[v.uf[v.hi[r]]], (unsigned)(2 * k + 1));
}
// phase: i in [0, 2 ns)
HD_FN void hd_split_nodes(const HdView& v, int i) {
    const int r = v.S[i >> 1];
    v.node[i] = (int)v.first[v.uf[(i & 1) ? v.hi[r] : v.lo[r]]];
    v.kid[i] = -1;
    if (!(i & 1)) { v.sp_parent[i >> 1] = -1; v.sp_side[i >> 1] = 0; }
}

// ---- R3: Kruskal over the splits (ONE thread; par / top: 2 ns ints each, LDS when they fit) ------------------------------------------
template <typename P>
HD_FN void hd_kruskal_splits(const HdView& v, int ns, P par, P top) {
    for (int i = 0; i < 2 * ns; ++i) { par[i] = i; top[i] = -1; }
    for (int k = 0; k < ns; ++k) {
        int ra = v.node[2 * k], rb = v.node[2 * k + 1];
        while (par[ra] != ra) { par[ra] = par[par[ra]]; ra = par[ra]; }
        while (par[rb] != rb) { par[rb] = par[par[rb]]; rb = par[rb]; }
        const int ta = top[ra], tb = top[rb];
        v.kid[2 * k] = ta; v.kid[2 * k + 1] = tb;
        if (ta >= 0) { v.sp_parent[ta] = k; v.sp_side[ta] = 0; }
        if (tb >= 0) { v.sp_parent[tb] = k; v.sp_side[tb] = 1; }
        par[ra] = rb;
        top[rb] = k;
    }
}

HD_FN int hd_cluster_above(const HdView& v, int k) {       // the cluster whose terminating split is k
    const int p = v.sp_parent[k];
    return p < 0 ? 0 : 1 + 2 * p + v.sp_side[k];
}

// ---- R4: phase r in [0, m) ----------------------------------------------------------------------------------------------------------
HD_FN int hd_chain_find(const HdView& v, int r) {                  // -> the chain node's provisional cluster; -1: no chain node
    if (!(v.eflag[r] & HD_CHAIN)) return -1;
    const unsigned f = v.first[v.uf[v.lo[r]]];
    int c = 0;
    if (f != 0xFFFFFFFFu) {
        int k = (int)(f >> 1), sd = (int)(f & 1u);
        while (k >= 0 && v.S[k] < r) { sd = v.sp_side[k]; k = v.sp_parent[k]; }
        c = k < 0 ? 0 : 1 + 2 * k + sd;
    }
    return c;
}
HD_FN HdChainRec hd_chain_rec(const HdView& v, int r, int c) {
    HdChainRec rec;
    rec.c = c; rec.kc = c >= 0 ? v.kcnt[r] : 0; rec.lam = c >= 0 ? hd_lambda(v.w2[r]) : 0.0;
    return rec;
}
// The chain nodes are grouped by cluster with ONE stable sort by this key (value: the rank), the root's nodes and the other edges behind
// all clusters: a cluster's chain is then a contiguous run of ascending ranks.  (Of the root only the chain LENGTH is read.)
#define HD_CHAIN_PAD 0x3FFFFFu
#define HD_CHAIN_KEY_BITS 22
HD_FN unsigned hd_chain_sortkey(const HdChainRec& rec) { return rec.c > 0 ? (unsigned)rec.c : HD_CHAIN_PAD; }
// ... with the root's chain as a run of its own between the clusters' and the other edges (allow_single_cluster reads all of it: the
// root's stability and largest lambda); every other run is where hd_chain_sortkey puts it
#define HD_CHAIN_ROOT 0x3FFFFEu
HD_FN unsigned hd_chain_sortkey_root(const HdChainRec& rec) { return rec.c > 0 ? (unsigned)rec.c : (rec.c == 0 ? HD_CHAIN_ROOT : HD_CHAIN_PAD); }
HD_FN unsigned hd_chain_key_of(int c) { return c > 0 ? (unsigned)c : HD_CHAIN_ROOT; }

HD_FN int hd_lower_bound_u32(const unsigned* a, int n, unsigned key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
HD_FN double hd_birth(const HdView& v, int c) { return c == 0 ? 0.0 : v.lam_split[(c - 1) >> 1]; }
// R6, first half: the cluster's rows of its OWN chain in the library's order -- chain nodes by DESCENDING rank, k_j equal terms each.
// hd_stab_terms is the exact inner step; the kernel runs a wave per cluster over the sorted run (loads in parallel, additions in order).
HD_FN double hd_stab_terms(double s, double t, int kc) {
    for (int j = 0; j < kc; ++j) s += t;
    return s;
}
// phase c in [1, 2 ns + 1) -- reference form (the emulation; the kernel's wave form is k_hd_chain_stats)
HD_FN void hd_chain_stats(const HdView& v, int c) {
    const int b = hd_lower_bound_u32(v.chain_key, v.m, hd_chain_key_of(c)), e = hd_lower_bound_u32(v.chain_key, v.m, hd_chain_key_of(c) + 1u);
    const double birth = hd_birth(v, c);
    double s = 0.0;
    int np = 0;
    for (int i = e - 1; i >= b; --i) {
        const HdChainRec rec = v.crec[v.chain_rank[i]];
        s = hd_stab_terms(s, (rec.lam - birth) * 1.0, rec.kc);
        np += rec.kc;
    }
    v.chainlen[c] = e - b; v.npts[c] = np; v.stab[c] = s;
    v.death[c] = e > b ? v.crec[v.chain_rank[b]].lam : 0.0;       // the lowest rank: the largest lambda
}
// allow_single_cluster: the same of the ROOT's chain (c = 0, birth 0; the chains sorted by hd_chain_sortkey_root) -- the longest chain of
// a LiDAR frame, walked only when the option asks for the root's stability
HD_FN void hd_chain_stats_root(const HdView& v) { hd_chain_stats(v, 0); }

// ---- R5 / R6: the cluster tree, relaxation phases over the splits k in [0, ns) -----------------------------------------------------
// A relaxation phase returns 1 when it computed its element; the caller repeats the phase, `sweep` = 0, 1, 2, ..., until no element
// does (as many sweeps as the split tree is high).  done[] is zero before a family of sweeps; an element computed in sweep s is
// stamped s + 1 and read by the others from sweep s + 1 on (behind the sweep's barrier): nobody sees the stamp before the values.
HD_FN bool hd_ready(const HdView& v, int k, int sweep) { const int d = hd_load_i32(&v.done[k]); return d != 0 && d <= sweep; }

// bottom-up: everything of the two clusters under split k -- sizes, the stability's last two rows (the children's), death, excess of mass
HD_FN void hd_up_node(const HdView& v, int k, int sweep) {         // (both kids are complete)
    // every load first, every store last: on the spine this body is one link of a chain of dependent steps, and a store between two
    // loads keeps the compiler from requesting the second early (the arrays may alias for all it knows)
    const int kl = v.kid[2 * k], kr = v.kid[2 * k + 1];
    const double birth = v.lam_split[k];
    const int cl = 1 + 2 * k, cr = 2 + 2 * k;
    const int np_l = v.npts[cl], np_r = v.npts[cr];
    const double st_l = v.stab[cl], st_r = v.stab[cr], de_l = v.death[cl], de_r = v.death[cr];
    int tot_l = 0, tot_r = 0, ns_l = 0, ns_r = 0, a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    double lam_l = 0.0, lam_r = 0.0, sa0 = 0.0, sa1 = 0.0, sb0 = 0.0, sb1 = 0.0;
    if (kl >= 0) { tot_l = v.tot[kl]; ns_l = v.nsub[kl]; lam_l = v.lam_split[kl]; a0 = v.csize[1 + 2 * kl]; a1 = v.csize[2 + 2 * kl]; sa0 = v.stab2[1 + 2 * kl]; sa1 = v.stab2[2 + 2 * kl]; }
    if (kr >= 0) { tot_r = v.tot[kr]; ns_r = v.nsub[kr]; lam_r = v.lam_split[kr]; b0 = v.csize[1 + 2 * kr]; b1 = v.csize[2 + 2 * kr]; sb0 = v.stab2[1 + 2 * kr]; sb1 = v.stab2[2 + 2 * kr]; }
    // the library's expressions, per child cluster: its stability's last two rows (its own children), death, excess of mass
    double s_l = st_l, sub_l = 0.0, d_l = de_l;
    if (kl >= 0) {
        s_l += (lam_l - birth) * (double)a0;
        s_l += (lam_l - birth) * (double)a1;
        if (lam_l > d_l) d_l = lam_l;
        sub_l += sa0;
        sub_l += sa1;
    }
    double s_r = st_r, sub_r = 0.0, d_r = de_r;
    if (kr >= 0) {
        s_r += (lam_r - birth) * (double)b0;
        s_r += (lam_r - birth) * (double)b1;
        if (lam_r > d_r) d_r = lam_r;
        sub_r += sb0;
        sub_r += sb1;
    }
    const int cs_l = np_l + tot_l, cs_r = np_r + tot_r;
    v.csize[cl] = cs_l; v.csize[cr] = cs_r;
    v.stab[cl] = s_l; v.stab[cr] = s_r;
    v.death[cl] = d_l; v.death[cr] = d_r;
    // (max_cluster_size: a larger cluster loses to its children whatever the stabilities, and takes their stability)
    const int mx = v.max_size;
    if (sub_l > s_l || (mx > 0 && cs_l > mx)) { v.wins[cl] = 0; v.stab2[cl] = sub_l; } else { v.wins[cl] = 1; v.stab2[cl] = s_l; }
    if (sub_r > s_r || (mx > 0 && cs_r > mx)) { v.wins[cr] = 0; v.stab2[cr] = sub_r; } else { v.wins[cr] = 1; v.stab2[cr] = s_r; }
    v.tot[k] = cs_l + cs_r;
    v.nsub[k] = 1 + ns_l + ns_r;
    hd_store_i32(&v.done[k], sweep + 1);
}
// The split tree of a LiDAR frame is a long spine (the background absorbing one cluster after the other: ~80 levels for ~700 splits)
// with shallow subtrees on it.  One level per sweep would spend most sweeps on ONE node each; so whoever completes a node goes on to
// its parent at once when the parent's other kid was complete BEFORE this sweep (then nobody else can complete the parent in this
// sweep: its owner sees this node's fresh stamp and waits) -- the spine is climbed by one thread inside one sweep.
HD_FN int hd_up_all(const HdView& v, int k, int sweep) {
    if (hd_load_i32(&v.done[k])) return 0;
    const int kl = v.kid[2 * k], kr = v.kid[2 * k + 1];
    if ((kl >= 0 && !hd_ready(v, kl, sweep)) || (kr >= 0 && !hd_ready(v, kr, sweep))) return 0;
    hd_up_node(v, k, sweep);
    for (int x = k;;) {
        const int p = v.sp_parent[x];
        if (p < 0) break;
        const int sib = v.kid[2 * p + (1 - v.sp_side[x])];
        if (sib >= 0 && !hd_ready(v, sib, sweep)) break;
        hd_up_node(v, p, sweep);
        x = p;
    }
    return 1;
}
// allow_single_cluster, ONE element behind the bottom-up sweeps (ns: the number of splits): the root as a cluster of the excess of mass --
// its stability's last two rows (the root split's children; birth 0), its largest lambda, its size = the two child clusters' (the
// library counts no point that leaves the root itself; a tree without a split: 0)
HD_FN void hd_root_node(const HdView& v, int ns) {
    double s = v.stab[0], sub = 0.0, d = v.death[0];
    int sz = 0;
    if (ns > 0) {
        const int k = ns - 1;                                      // the root split: the one of the highest rank
        const double lam = v.lam_split[k];
        const int a0 = v.csize[1 + 2 * k], a1 = v.csize[2 + 2 * k];
        s += (lam - 0.0) * (double)a0;
        s += (lam - 0.0) * (double)a1;
        if (lam > d) d = lam;
        sub += v.stab2[1 + 2 * k];
        sub += v.stab2[2 + 2 * k];
        sz = a0 + a1;
    }
    v.csize[0] = sz; v.stab[0] = s; v.death[0] = d;
    v.wins[0] = (sub > s || (v.max_size > 0 && sz > v.max_size)) ? 0 : 1;
}
// top-down: dendrogram depth of the split node and its preorder index in the split tree (R5)
HD_FN void hd_down_node(const HdView& v, int k, int sweep) {       // (the parent is complete)
    const int p = v.sp_parent[k];
    if (p < 0) { v.depth[k] = v.chainlen[0]; v.pre[k] = 0; }
    else {
        const int sd = v.sp_side[k];
        v.depth[k] = v.depth[p] + 1 + v.chainlen[1 + 2 * p + sd];
        const int kl = v.kid[2 * p];
        v.pre[k] = v.pre[p] + 1 + (sd && kl >= 0 ? v.nsub[kl] : 0);
    }
    hd_store_i32(&v.done[k], sweep + 1);
}
// ... and whoever completes a node goes on into its HEAVIER kid (more splits below) at once: a path from the root crosses at most
// log2(splits) lighter kids, so that many sweeps suffice
HD_FN int hd_down_order(const HdView& v, int k, int sweep) {
    if (hd_load_i32(&v.done[k])) return 0;
    const int p = v.sp_parent[k];
    if (p >= 0 && !hd_ready(v, p, sweep)) return 0;
    hd_down_node(v, k, sweep);
    for (int x = k;;) {
        const int kl = v.kid[2 * x], kr = v.kid[2 * x + 1];
        int h = kl;
        if (kr >= 0 && (kl < 0 || v.nsub[kr] > v.nsub[kl])) h = kr;
        if (h < 0) break;
        hd_down_node(v, h, sweep);
        x = h;
    }
    return 1;
}
// BFS position of split k: the splits in front of it in (depth, preorder) order
HD_FN bool hd_bfs_before(int da, int pa, int db, int pb) { return da < db || (da == db && pa < pb); }

HD_FN int hd_final_id(const HdView& v, int c) { return c == 0 ? 0 : 2 * v.q[(c - 1) >> 1] + 1 + ((c - 1) & 1); }
HD_FN int hd_cluster_parent(const HdView& v, int c) { return hd_cluster_above(v, (c - 1) >> 1); }       // c >= 1

// phase c in [1, 2 ns + 1): a cluster stays selected iff it wins and no cluster above it does (the root: only with allow_single_cluster)
HD_FN void hd_select_eom(const HdView& v, int c) {
    bool sel = v.wins[c];
    for (int a = hd_cluster_parent(v, c); sel && a > 0; a = hd_cluster_parent(v, a)) if (v.wins[a]) sel = false;
    if (sel && v.allow_single && v.wins[0]) sel = false;
    v.selected[c] = sel;
    v.cand[c] = 0;
}
// phase c in [0, 2 ns + 1): the selection by the options -- the root (selected only by the excess of mass with allow_single_cluster);
// 'leaf': cluster 1 + 2 k + side is a leaf of the cluster tree iff no split hangs below (k, side) -- a tree without a split has no leaf and
// selects nothing, allow_single_cluster or not, like the library; else the excess of mass
HD_FN void hd_select(const HdView& v, int c) {
    if (c == 0) { v.selected[0] = (v.allow_single && !v.leaf) ? v.wins[0] : 0; v.cand[0] = 0; return; }
    if (v.leaf) { v.selected[c] = v.kid[c - 1] < 0 ? 1 : 0; v.cand[c] = 0; return; }
    hd_select_eom(v, c);
}
// cluster_selection_epsilon, phase c in [1, 2 ns + 1) (hdbscan_tree.cpp: a selected cluster born below eps climbs to the first ancestor
// born above it, or stops under the root -- AT the root with allow_single_cluster).  With allow_single_cluster the phases run from c = 0:
// a selected root (birth 0: 1 / birth = inf) is its own candidate, which is the library's "only the root is selected" shortcut.
HD_FN void hd_eps_candidates(const HdView& v, int c) {
    if (!v.selected[c]) return;
    if (1.0 / hd_birth(v, c) < v.eps) {
        int node = c;
        while (true) {
            const int p = hd_cluster_parent(v, node);
            if (p == 0) { if (v.allow_single) node = 0; break; }
            if (1.0 / hd_birth(v, p) > v.eps) { node = p; break; }
            node = p;
        }
        v.cand[node] = 1;
    } else
        v.cand[c] = 1;
}
HD_FN void hd_eps_select(const HdView& v, int c) {                 // phase c in [1, 2 ns + 1), after a barrier behind hd_eps_candidates
    bool sel = v.cand[c];
    for (int a = c > 0 ? hd_cluster_parent(v, c) : 0; sel && a > 0; a = hd_cluster_parent(v, a)) if (v.cand[a]) sel = false;
    if (sel && c > 0 && v.allow_single && v.cand[0]) sel = false;
    v.wins[c] = sel;                                               // (wins is free now: the new selection, read by the next phase)
}
// phase c in [0, 2 ns + 1): sel_by_final[final id] = selected (then an exclusive scan over 2 ns + 1 entries gives the flat labels)
HD_FN void hd_selected_by_final(const HdView& v, int c, bool use_eps) {
    const bool sel = (c == 0 && !v.allow_single) ? false : (use_eps ? v.wins[c] : v.selected[c]);
    v.selected[c] = sel;
    v.sel_by_final[hd_final_id(v, c)] = sel ? 1 : 0;
}
// phase c in [0, 2 ns + 1), sel_by_final scanned (exclusive): the nearest selected cluster at or above c owns c's points.  A selected root
// (allow_single_cluster; then it is the one cluster, label 0) owns them under a threshold on the point's own lambda: out_label = HD_ROOT_OWNED.
#define HD_ROOT_OWNED (-2)
HD_FN void hd_owner(const HdView& v, int c) {
    int o = c;
    while (o > 0 && !v.selected[o]) o = hd_cluster_parent(v, o);
    if (o == 0 && v.allow_single && v.selected[0]) { v.out_label[c] = HD_ROOT_OWNED; v.out_death[c] = v.death[0]; return; }
    if (o <= 0) { v.out_label[c] = -1; v.out_death[c] = 0.0; return; }
    v.out_label[c] = v.sel_by_final[hd_final_id(v, o)];
    v.out_death[c] = v.death[o];
}
// phase p in [0, n)
HD_FN void hd_point(const HdView& v, int p) {
    const HdChainRec rec = v.crec[v.a[p]];
    int lab = v.out_label[rec.c];
    if (lab < 0) {
        // the root as the one cluster: the point's own lambda against 1 / eps, or without eps the largest lambda among the root's own rows
        if (lab != HD_ROOT_OWNED || !(rec.lam >= (v.eps != 0.0 ? 1.0 / v.eps : v.out_death[rec.c]))) { v.labels[p] = -1; v.probs[p] = 0.0; return; }
        lab = 0;
    }
    const double mx = v.out_death[rec.c], lam = rec.lam;
    v.labels[p] = lab;
    v.probs[p] = (mx == 0.0 || isinf(lam)) ? 1.0 : (lam < mx ? lam : mx) / mx;
}
#endif
