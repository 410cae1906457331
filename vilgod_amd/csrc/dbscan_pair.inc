// THE pair test of DBSCAN (vg_cluster_dbscan / vg_dbscan_host): are two rows neighbours?  One text for the kernels and the host twin.
//
// sklearn.cluster.DBSCAN(metric='euclidean') converts X to float64 and asks its neighbour tree for `radius_neighbors(X, eps)`; the
// kd-tree and the brute-force path both compare the float64 sum of squared differences, accumulated coordinate by coordinate, with
// eps * eps, inclusive.  Here:
//   * both rows are widened EXACTLY to double (a float32 is a double)
//   * d2 = ((dx*dx + dy*dy) + dz*dz [+ d4*d4 [+ d5*d5]]), left to right, every product and every sum rounded on its own: the pragma
//     below forbids contraction into a fused multiply-add in this function, on the device and on the host, also where the translation
//     unit loses its -ffp-contract=off and falls back to hipcc's default (fast-honor-pragmas); checked in the assembly of both sides.
//     Only an explicit -ffp-contract=fast overrides pragmas: no build of this package passes it
//   * neighbours iff d2 <= eps2, eps2 = eps * eps formed in double by the caller.  A row is its own neighbour (d2 = 0).
// A NaN coordinate makes d2 NaN and the test false; the entry points promise nothing for non-finite rows.

struct DbRow {
    float x, y, z, e, t;              // e, t: the 4th and 5th clustering coordinate (read only when dim says so)
};

__host__ __device__ __forceinline__ double dbscan_pair_d2(int dim, const DbRow& a, const DbRow& b) {
#pragma clang fp contract(off)
    const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
    double d2 = (dx * dx + dy * dy) + dz * dz;
    if (dim >= 4) {
        const double d4 = (double)a.e - (double)b.e;
        d2 = d2 + d4 * d4;
    }
    if (dim >= 5) {
        const double d5 = (double)a.t - (double)b.t;
        d2 = d2 + d5 * d5;
    }
    return d2;
}

__host__ __device__ __forceinline__ bool dbscan_pair(int dim, const DbRow& a, const DbRow& b, double eps2) {
    return dbscan_pair_d2(dim, a, b) <= eps2;
}
