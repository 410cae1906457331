// The per-point body of the oriented extents (csrc/oriented_extent.hip): one point of a cluster, shifted by the cluster's float32
// median, turned by the track's direction, folded into the running extremes of its pair.  `__host__ __device__`:
// k_cluster_oriented_extents runs it one point per lane and vg_cluster_oriented_extents_host runs the SAME text over host arrays, so
// the CPU tests exercise the shipped arithmetic.  Compiled with -ffp-contract=off: the one fused operation per coordinate is the fma
// written below, nothing else is contracted, and host and device agree bit for bit.
//
// What it restates (the reference's src/vilgod/zero_shot_detector.py:576-603): `np.dot(pts[:, :3] - center, rot)` for float32 `pts` and
// `center` and a float64 `rot` whose third row and column are (0, 0, 1), then min / max per column, and min / max of the points' own z:
//     float  dx = x - cx,  dy = y - cy;                      float32 subtraction, rounded once
//     double px = fma((double)dy, r10, (double)dx * r00);    the product with row 0 is rounded, the one with row 1 is fused into the sum
//     double py = fma((double)dy, r11, (double)dx * r01);
// (the third term of the dot product is (z - cz) * 0 and changes nothing; column 2 of the product is not used by the caller).
//
// Zeros are folded in as +0 (`+ 0.0`; kept under IEEE rules, -0 + +0 = +0): with one sign of zero, minimum and maximum of finite
// values do not depend on the order in which they are combined, which is all the kernel's reduction relies on.
// A point whose x, y, z or projection is not finite marks the pair `bad`; the pair's six values are then NaN.
#pragma once

#ifndef VG_HD
#define VG_HD __host__ __device__ __forceinline__
#endif

struct OextRot { double r00, r01, r10, r11; };

// running result of one pair: {min px, max px, min py, max py, min z, max z} and whether anything non-finite was met
struct OextAcc {
    double v[6];
    int bad;
};

VG_HD bool oext_finite(float a) { return __builtin_isfinite(a); }
VG_HD bool oext_finite(double a) { return __builtin_isfinite(a); }
VG_HD double oext_min(double a, double b) { return b < a ? b : a; }
VG_HD double oext_max(double a, double b) { return b > a ? b : a; }

// the values one point contributes: p = {px, py, z}; returns false if the point (or its projection) is not finite
VG_HD bool oext_point(float x, float y, float z, float cx, float cy, const OextRot& r, double* p) {
    const float dx = x - cx, dy = y - cy;
    const double px = __builtin_fma((double)dy, r.r10, (double)dx * r.r00);
    const double py = __builtin_fma((double)dy, r.r11, (double)dx * r.r01);
    p[0] = px + 0.0;
    p[1] = py + 0.0;
    p[2] = (double)z + 0.0;
    return oext_finite(x) && oext_finite(y) && oext_finite(z) && oext_finite(px) && oext_finite(py);
}

VG_HD void oext_first(OextAcc& a, const double* p, bool ok) {
    a.v[0] = a.v[1] = p[0];
    a.v[2] = a.v[3] = p[1];
    a.v[4] = a.v[5] = p[2];
    a.bad = ok ? 0 : 1;
}

VG_HD void oext_fold(OextAcc& a, const double* p, bool ok) {
    a.v[0] = oext_min(a.v[0], p[0]); a.v[1] = oext_max(a.v[1], p[0]);
    a.v[2] = oext_min(a.v[2], p[1]); a.v[3] = oext_max(a.v[3], p[1]);
    a.v[4] = oext_min(a.v[4], p[2]); a.v[5] = oext_max(a.v[5], p[2]);
    a.bad |= ok ? 0 : 1;
}

// two partial results of the same pair (the kernel's wave and workgroup steps)
VG_HD void oext_merge(OextAcc& a, const OextAcc& b) {
    a.v[0] = oext_min(a.v[0], b.v[0]); a.v[1] = oext_max(a.v[1], b.v[1]);
    a.v[2] = oext_min(a.v[2], b.v[2]); a.v[3] = oext_max(a.v[3], b.v[3]);
    a.v[4] = oext_min(a.v[4], b.v[4]); a.v[5] = oext_max(a.v[5], b.v[5]);
    a.bad |= b.bad;
}
