// Part of cluster.hip (included in place, first): the CL_* constants, ClGrid and the geometry of the cell grid and its implicit octree --
// Morton codes, THE faces, cell assignment, the origin, the level tables' layout, box and shell distances, the walk's stack entries, the
// float64 pair distance.  What is __host__ __device__ here is what vg_cluster_geom_probe exposes.  Expects common.h and nothing else.

#define CL_CELL 0.4
#define CL_NX 512
#define CL_NY 512
#define CL_NZ 64
#define CL_LB 6                       // interleaved bits per axis
#define CL_NCODES (1 << 24)           // 9 + 9 + 6 bits
#define CL_LMAX 6                     // coarsest Morton-contiguous level (25.6 m cubes): 8 x 8 x 1 roots
#define CL_PUR_LEVELS 4               // purity tables for levels 0..3 (0.4 .. 3.2 m); levels 4..6 were measured: no gain
#ifndef CL_LEAF
#define CL_LEAF 48                    // nodes with at most this many points are scanned instead of subdivided
#endif
#define CL_FIRST_BATCH 6      // Boruvka rounds queued before the first host read of the edge counter
#define CL_STACK 44      // DFS stack entries per thread (LDS): the walk never holds more than 1 + 7 * CL_LMAX = 43 nodes (a pop precedes every push of
                         // <= 8 children, level-0 nodes are never expanded); 44 KB per 256-thread block -> three blocks per CU instead of two
#define CL_K 16                       // neighbours kept (k-th other point = entry k, entry 0 is the point itself)

struct ClGrid {
    double ox, oy, oz;                // world coordinate of cell (0,0,0)'s min corner
    unsigned int kmin[3], kmax[3];    // ordered-int bbox keys (scratch for the reduction)
    double inf;                       // +infinity, set by the host.  Kernels that keep a wave-uniform float64 in SGPRs read it from
                                      // here: ROCm 7.2's gfx950 back end materialises a uniform `double x = INFINITY` as
                                      // `s_mov_b64 s[..], 0x7ff0000000000000`, which gfx9 cannot encode (32-bit literals only; the
                                      // assembler rejects the line, the direct object emission truncates it to 0.0)
};

// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned int cl_spread6(unsigned int v) {   // 6 bits -> every third bit
    v &= 63u;
    v = (v | (v << 8)) & 0x300Fu;
    v = (v | (v << 4)) & 0x30C3u;
    v = (v | (v << 2)) & 0x9249u;
    return v;
}
__host__ __device__ __forceinline__ unsigned int cl_code(int cx, int cy, int cz) {
    unsigned int lo = cl_spread6(cx) | (cl_spread6(cy) << 1) | (cl_spread6(cz) << 2);
    unsigned int hi = ((unsigned int)cx >> 6) | (((unsigned int)cy >> 6) << 3);
    return (hi << 18) | lo;
}
// THE faces of the grid: face i of an axis with origin o is the float64 value o + i * CL_CELL as computed (0.4 is not exact in binary,
// so this is not the real number).  A level-l node c spans [face(c << l), face((c + 1) << l)): o + c * (CL_CELL * 2^l) rounds the
// same real number, so every level computes the same faces.  Cells are assigned by these faces, not by the floor alone: the floor of
// (v - o) * 2.5 puts a coordinate that sits on or next to a face into the neighbouring cell for some origins (ox = -10.4, x = 62.0:
// floor gives cell 181, whose computed min face is 62.00000000000001), and a box that does not hold its own points is no lower bound.
__host__ __device__ __forceinline__ double cl_face(double o, int i, int l) {       // face i of level l: the ONLY place that computes one
    return o + (double)i * (CL_CELL * (double)(1 << l));
}
// distance along one axis from q to node c of level l (nb nodes on the axis): 0 inside [lo, hi]; a face the grid clips does not count
// (border nodes extend to infinity on the outside: points beyond the grid are clamped INTO border cells)
__host__ __device__ __forceinline__ double cl_axis_gap(double o, double q, int c, int l, int nb) {
    const double lo = cl_face(o, c, l), hi = cl_face(o, c + 1, l);                 // (lo + size is not a face)
    double d = 0.0;
    if (q < lo && c > 0) d = lo - q;
    else if (q > hi && c < nb - 1) d = q - hi;
    return d;
}
__host__ __device__ __forceinline__ int cl_cell_axis(double o, double v, int n) {
    int c = (int)floor((v - o) * (1.0 / CL_CELL));
    c = c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
    if (c > 0 && v < cl_face(o, c, 0)) --c;                                 // the floor is at most one cell off (errors ~1e-13 m)
    else if (c < n - 1 && v >= cl_face(o, c + 1, 0)) ++c;
    return c;
}
__host__ __device__ __forceinline__ void cl_cell_of(const ClGrid& g, double x, double y, double z, int& cx, int& cy, int& cz) {
    cx = cl_cell_axis(g.ox, x, CL_NX);
    cy = cl_cell_axis(g.oy, y, CL_NY);
    cz = cl_cell_axis(g.oz, z, CL_NZ);
}
// origin of one axis from the data's extremes: the data is centred in the grid when it fits, otherwise the grid is anchored at the
// minimum (outliers clamp to border cells); floored to a multiple of the cell size
__host__ __device__ __forceinline__ double cl_origin(double lo, double hi, double ext) {
    const double span = hi - lo;
    const double start = span < ext ? lo - 0.5 * (ext - span) : lo;
    return floor(start / CL_CELL) * CL_CELL;
}
// cell_start is stored reversed (index NCODES - code) so that the "first point with code >= c" table is a
// forward inclusive min-scan.
__device__ __forceinline__ int cl_start(const int* __restrict__ cs, unsigned int code) { return cs[CL_NCODES - code]; }
// The same table per coarser level l = 1 .. CL_LMAX, stored FORWARD and compact right behind the cell table: entry c of level l =
// first sorted point whose code >> 3l is >= c (c = 0 .. NCODES >> 3l, the last one = n).  The eight children of a node (nine
// consecutive entries: they include the node's own range) and the 64 grand-children of a block are then neighbours in memory,
// where the cell table has them 4 * 8^l bytes apart (k_cl_levels fills them, 16 us per frame).
__device__ __host__ __forceinline__ size_t cl_lvl_off(int l) {      // offset of level l (>= 1) behind the cell table
    return ((size_t)CL_NCODES - ((size_t)CL_NCODES >> (3 * (l - 1)))) / 7 + (size_t)(l - 1);
}
#define CL_LVL_TOTAL (cl_lvl_off(CL_LMAX + 1))
// first sorted point of node c (= code >> 3l) of level l; c + 1 gives the node's end
__device__ __forceinline__ int cl_start_l(const int* __restrict__ cs, int l, unsigned int c) {
    return l == 0 ? cs[CL_NCODES - c] : cs[(size_t)(CL_NCODES + 1) + cl_lvl_off(l) + c];
}

// ---------------------------------------------------------------------------------------------
// squared distance in float64, summed left to right over the DIM coordinates: ((((dx2 + dy2) + dz2) + de2) + dt2)
template <int DIM>
__device__ __forceinline__ double cl_d2(double ax, double ay, double az, double ae, double at, const float4& b,
                                        const float* __restrict__ st, int j) {
    double dx = ax - (double)b.x, dy = ay - (double)b.y, dz = az - (double)b.z;
    double d2 = (dx * dx + dy * dy) + dz * dz;
    if (DIM >= 4) { const double de = ae - (double)b.w; d2 = d2 + de * de; }
    if (DIM >= 5) { const double dt = at - (double)st[j]; d2 = d2 + dt * dt; }
    return d2;
}

// squared distance from q to the nearest face of the level-l block [b-1, b+2) (faces clipped by the grid do not count)
__host__ __device__ __forceinline__ double cl_block_radius2(const ClGrid& g, double qx, double qy, double qz, int bx, int by,
                                                   int bz, int l) {
    double r = INFINITY;
    const int nb[3] = {CL_NX >> l, CL_NY >> l, CL_NZ >> l};
    const int b[3] = {bx, by, bz};
    const double q[3] = {qx, qy, qz}, o[3] = {g.ox, g.oy, g.oz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // a face only bounds the search if cells exist beyond it (points outside the grid are clamped INTO border cells)
        if (b[a] - 2 >= 0) r = fmin(r, q[a] - cl_face(o[a], b[a] - 1, l));
        if (b[a] + 2 < nb[a]) r = fmin(r, cl_face(o[a], b[a] + 2, l) - q[a]);
    }
    if (r < 0) r = 0;
    return isinf(r) ? INFINITY : r * r;
}

// ---- pruned depth-first traversal of the implicit octree ---------------------------------------------------
// A node = (level l, cell coordinates at that level); its points are the contiguous range
// [start(code), start(code + 8^l)) of the Morton-sorted array.  Stack entries pack (l, x, y, z) in 32 bits and live
// in LDS, interleaved by thread (bank-conflict free).
__device__ __forceinline__ unsigned int cl_pack(int l, int x, int y, int z) {
    return ((unsigned int)l << 27) | ((unsigned int)x << 18) | ((unsigned int)y << 9) | (unsigned int)z;
}
__device__ __forceinline__ void cl_unpack(unsigned int e, int& l, int& x, int& y, int& z) {
    l = (int)(e >> 27); x = (int)((e >> 18) & 511u); y = (int)((e >> 9) & 511u); z = (int)(e & 511u);
}
// squared distance from q to the axis-aligned box of node (l,x,y,z); 0 inside.  Border nodes extend to infinity on
// the outside (points beyond the grid are clamped INTO border cells).
__host__ __device__ __forceinline__ double cl_box_d2(const ClGrid& g, double qx, double qy, double qz, int l, int x, int y, int z) {
    const int nb[3] = {CL_NX >> l, CL_NY >> l, CL_NZ >> l};
    const int c[3] = {x, y, z};
    const double q[3] = {qx, qy, qz}, o[3] = {g.ox, g.oy, g.oz};
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double d = cl_axis_gap(o[a], q[a], c[a], l, nb[a]);
        d2 += d * d;
    }
    return d2;
}

__host__ __device__ __forceinline__ size_t cl_pur_off_fwd(int l) {   // offset of level l inside the per-node tables (= cl_pur_off)
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += (size_t)CL_NCODES >> (3 * i);
    return o;
}
