// The per-pair body of points-in-boxes (csrc/points_in_boxes.hip): is the point (x, y, z) inside the box {cx, cy, cz, dx, dy, dz, rz}?
// `__host__ __device__`: k_points_in_boxes runs it one point per lane, and vg_points_in_boxes_host runs the SAME text over host
// arrays, so the CPU tests exercise the shipped arithmetic.  All float64 (float32 inputs widened exactly), only + - * and comparisons
// plus iou_sincos of csrc/iou_pair.inc, compiled with -ffp-contract=off: host and device agree bit for bit.
//
// The rule (the counterpart of pcdet's check_pt_in_box3d, restated; include/vilgod_hip.h carries it as the contract):
//     fabs(z - cz) <= dz / 2                                         (inclusive)
//     fabs(lx) < dx / 2 + 1e-5  and  fabs(ly) < dy / 2 + 1e-5       (strict, beyond a 1e-5 margin)
//     lx = sx cos(rz) + sy sin(rz),  ly = -sx sin(rz) + sy cos(rz),  (sx, sy) = (x - cx, y - cy)
// in its positive form: a NaN anywhere fails a comparison, |rz| >= 1.6e6 gives NaN from iou_sincos, and an extent that is not >= 0
// is refused outright (with the margin alone, dx = -1e-6 would still contain its centre).
//
// A box is prepared once (pib_prepare: the halves, the sine / cosine and a squared reject radius) and tested against many points
// (pib_inside).  The reject radius only skips pairs the full test rejects as well -- the comment at pib_prepare says why.
#pragma once

#include "iou_pair.inc"          // iou_sincos, VG_HD

#define PIB_MARGIN 1e-5

struct PibBox {
    double cx, cy, cz;           // centre
    double hx, hy, hz;           // dx / 2 + 1e-5, dy / 2 + 1e-5, dz / 2;  hz = -1 for a box that contains nothing
    double cs, sn;               // cos(rz), sin(rz)
    double r2;                   // squared reject radius; -1 for a box that contains nothing
};
// how pib_inside reads a prepared box: field by field, each where it is first needed (the kernel's view reads LDS words, so a pair
// that the radius rejects has read three of the nine)
struct PibBoxView {
    const PibBox& o;
    VG_HD double cx() const { return o.cx; }
    VG_HD double cy() const { return o.cy; }
    VG_HD double cz() const { return o.cz; }
    VG_HD double hx() const { return o.hx; }
    VG_HD double hy() const { return o.hy; }
    VG_HD double hz() const { return o.hz; }
    VG_HD double cs() const { return o.cs; }
    VG_HD double sn() const { return o.sn; }
    VG_HD double r2() const { return o.r2; }
};

// r2: a point passes the full test only if |lx| < hx and |ly| < hy for the COMPUTED lx, ly.  With rho^2 = sx^2 + sy^2 (exact) and
// u = 2^-53: each of lx, ly carries three roundings (two products, one sum) of terms <= rho, so it is within 3 u sqrt(2) rho (1 + u)^2
// of the value the computed cs, sn give exactly, and those satisfy cs^2 + sn^2 >= 1 - 5 u (each within an ulp of the true value).
// Hence rho^2 (1 - 5 u) <= (hx + 5 u rho)^2 + (hy + 5 u rho)^2, which bounds rho^2 by (hx^2 + hy^2) (1 + 40 u), and the computed
// d2 = fl(fl(sx sx) + fl(sy sy)) is within 2 u of rho^2: a passing point has d2 <= (hx^2 + hy^2) (1 + 50 u).  The pad here is 2^-40,
// ~8000 u, applied to the rounded sum (3 roundings: far inside the pad).  hx, hy >= 1e-5 for a valid box, so nothing underflows;
// a sum that overflows gives r2 = +inf and rejects nothing.  NaN in d2 or r2: `d2 > r2` is false, the full test decides.
VG_HD void pib_prepare(const double* b, PibBox& o) {
    o.cx = b[0]; o.cy = b[1]; o.cz = b[2];
    const bool ok = b[3] >= 0.0 && b[4] >= 0.0 && b[5] >= 0.0;
    o.hx = 0.5 * b[3] + PIB_MARGIN;
    o.hy = 0.5 * b[4] + PIB_MARGIN;
    o.hz = ok ? 0.5 * b[5] : -1.0;
    iou_sincos(b[6], o.sn, o.cs);
    const double r2 = (o.hx * o.hx + o.hy * o.hy) * (1.0 + 0x1p-40);
    o.r2 = ok ? r2 : -1.0;
}

// the three steps in the order the kernel walks them: radius reject, z, rotation
template <class View>
VG_HD bool pib_inside(const View& o, double x, double y, double z) {
    const double sx = x - o.cx(), sy = y - o.cy();
    if (sx * sx + sy * sy > o.r2()) return false;
    const double dz = z - o.cz();
    if (!((dz < 0.0 ? -dz : dz) <= o.hz())) return false;
    const double cs = o.cs(), sn = o.sn();
    const double lx = sx * cs + sy * sn;
    const double ly = sy * cs - sx * sn;
    return (lx < 0.0 ? -lx : lx) < o.hx() && (ly < 0.0 ? -ly : ly) < o.hy();
}
