// The per-pair body of the rotated-box IoU (csrc/iou.hip): one (a, b) pair of 7-value boxes [x, y, z, dx, dy, dz, heading] -> the 3-D
// IoU, the BEV IoU or the BEV intersection area, all in float64.  `__host__ __device__`: k_boxes_iou runs it one pair per lane, and
// vg_boxes_iou3d_host runs the SAME text over host arrays, so the CPU tests exercise the shipped arithmetic.
//
// Only + - * / sqrt, rint and comparisons are used, each correctly rounded on the host and on gfx950, and the file is compiled with
// -ffp-contract=off: host and device results are equal bit for bit.  That is why the sine and cosine are computed here and not by
// the two maths libraries (they agree to an ulp, not to the bit).
//
// Geometry.  Everything happens in B's frame, centred on B:
//   1. d = centre_a - centre_b first (world coordinates never meet the extents: the result does not depend on where the pair
//      stands), rotated by -heading_b;
//   2. the relative rotation is cos / sin of (heading_a - heading_b), the difference taken exactly (TwoSum; its rounding error
//      enters to first order), so identical headings give exactly (1, 0) and a heading + 2 pi gives what the float64 value means;
//   3. A's four corners are clipped by B's four axis-aligned half-planes x <= hx, x >= -hx, y <= hy, y >= -hy (Sutherland-Hodgman;
//      a convex polygon gains at most one vertex per half-plane: 8 at most).  A crossing point gets the clipped coordinate set to
//      the bound itself, so later closed tests see it ON the boundary;
//   4. the area is the triangle fan around vertex 0 (differences first: the error scales with the intersection, not with its
//      distance from B's centre).
// The vertex buffers are fixed-size arrays touched with compile-time indices only (every loop below is fully unrolled and a write
// at the running count is a chain of selects), so they live in registers: a runtime-indexed local array goes to scratch memory.
//
// Exact zeros: an extent <= 0 (dx, dy of either box; dz too in mode 0), no z overlap (mode 0), centres farther apart than the two
// half-diagonals, fewer than 3 vertices left.  Touching boxes with exactly representable corners give 0.0 through the clip: the
// closed tests keep a zero-width polygon whose fan products cancel exactly.
//
// Domain: |heading| < 2^20 * pi / 2 (beyond it the two-term pi / 2 reduction loses its exactness and the result is NaN).
#pragma once

#ifndef VG_HD
#define VG_HD __host__ __device__ __forceinline__
#endif

#include "vilgod_hip.h"          // VG_IOU_3D / VG_IOU_BEV / VG_IOU_BEV_AREA
#define IOU_NV 8                 // vertices a clipped rectangle can have

// sin and cos of x, |x| < 2^20 * pi / 2.  Reduction: n = rint(x * 2 / pi), x - n * pi / 2 with pi / 2 in 33-bit pieces (n * piece is
// exact) -- pio2_1 + pio2_2 + pio2_2t carry 118 bits, so the reduced head + tail is good to far below an ulp for every float64 x
// of the domain.  Kernels: the minimax polynomials on [-pi/4, pi/4] of the freely distributable fdlibm (Sun Microsystems, 1993:
// k_sin.c, k_cos.c; e_rem_pio2.c for the constants), error < 1 ulp.
VG_HD void iou_sincos(double x, double& sn, double& cs) {
    const double invpio2 = 6.36619772367581382433e-01;       // 0x3FE45F306DC9C883
    const double pio2_1 = 1.57079632673412561417e+00;        // 0x3FF921FB54400000  first 33 bits of pi / 2
    const double pio2_2 = 6.07710050630396597660e-11;        // 0x3DD0B4611A600000  next 33 bits
    const double pio2_2t = 2.02226624879595063154e-21;       // 0x3BA3198A2E037073  pi / 2 - (pio2_1 + pio2_2)
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    if (!(x > -1.6e6 && x < 1.6e6)) {                        // outside the domain, infinite or NaN
        sn = cs = x - x + (x - x) / (x - x);                 // NaN without a float -> int conversion of it
        return;
    }
    const double fn = rint(x * invpio2);
    const int n = (int)fn;
    const double t = x - fn * pio2_1;                        // exact product; the difference cancels to <= 1 rounding
    double w = fn * pio2_2;
    const double r = t - w;
    w = fn * pio2_2t - ((t - r) - w);
    const double y0 = r - w, y1 = (r - y0) - w;              // reduced argument = y0 + y1, |y0| <= pi / 4 (+ an ulp)
    const double z = y0 * y0;
    // sin(y0 + y1)
    const double v = z * y0;
    const double rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
    // cos(y0 + y1)
    const double rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double hz = 0.5 * z, wc = 1.0 - hz;
    const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1));
    const int q = n & 3;
    sn = (q == 0) ? ks : (q == 1) ? kc : (q == 2) ? -ks : -kc;
    cs = (q == 0) ? kc : (q == 1) ? -ks : (q == 2) ? -kc : ks;
}

struct IouPoly {
    double x[IOU_NV], y[IOU_NV];
    int n;
};

// out[cnt] = (px, py), cnt += 1 when `on`; compile-time slots only (a write past the last slot is dropped)
VG_HD void iou_emit(IouPoly& o, bool on, double px, double py) {
#pragma unroll
    for (int k = 0; k < IOU_NV; ++k) {
        const bool here = on && o.n == k;
        o.x[k] = here ? px : o.x[k];
        o.y[k] = here ? py : o.y[k];
    }
    o.n += on ? 1 : 0;
}

// One Sutherland-Hodgman step: keep sign * coord <= bound.  AXIS 0 clips x, 1 clips y.  NIN: the most vertices `in` can hold here.
template <int AXIS, int NIN>
VG_HD void iou_clip(const IouPoly& in, double sign, double bound, IouPoly& out) {
    out.n = 0;
#pragma unroll
    for (int k = 0; k < IOU_NV; ++k) out.x[k] = out.y[k] = 0.0;
    const double edge = sign * bound;                        // the coordinate of the clipping line
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const bool live = i < in.n;
        const bool wrap = i + 1 >= in.n;                     // the closing edge goes back to vertex 0
        const double px = in.x[i], py = in.y[i];
        const double qx = wrap ? in.x[0] : in.x[i + 1];       // NIN < IOU_NV: i + 1 is a slot
        const double qy = wrap ? in.y[0] : in.y[i + 1];
        const double dp = bound - sign * (AXIS == 0 ? px : py);          // >= 0: inside (closed)
        const double dq = bound - sign * (AXIS == 0 ? qx : qy);
        const bool pin = dp >= 0.0, qin = dq >= 0.0;
        iou_emit(out, live && pin, px, py);
        // the crossing (where it is used dp and dq have opposite signs: the denominator is not 0)
        const double den = dp - dq;
        const double tt = dp / (den != 0.0 ? den : 1.0);
        const double cx = AXIS == 0 ? edge : px + tt * (qx - px);
        const double cy = AXIS == 0 ? py + tt * (qy - py) : edge;
        iou_emit(out, live && (pin != qin), cx, cy);
    }
    out.n = out.n < IOU_NV ? out.n : IOU_NV;
}

// -> the value of `mode` for one pair; a, b: [x, y, z, dx, dy, dz, heading]
VG_HD double iou_pair(const double* a, const double* b, int mode) {
    if (!(a[3] > 0.0) || !(a[4] > 0.0) || !(b[3] > 0.0) || !(b[4] > 0.0)) return 0.0;
    double zov = 1.0;
    if (mode == VG_IOU_3D) {
        if (!(a[5] > 0.0) || !(b[5] > 0.0)) return 0.0;
        const double dz = a[2] - b[2], ha = 0.5 * a[5], hb = 0.5 * b[5];           // relative to B's centre: identical boxes give dz exactly
        const double top = dz + ha < hb ? dz + ha : hb, bot = dz - ha > -hb ? dz - ha : -hb;
        zov = top - bot;
        if (!(zov > 0.0)) return 0.0;
    }
    const double dx = a[0] - b[0], dy = a[1] - b[1];
    const double hax = 0.5 * a[3], hay = 0.5 * a[4], hbx = 0.5 * b[3], hby = 0.5 * b[4];
    const double reach = sqrt(hax * hax + hay * hay) + sqrt(hbx * hbx + hby * hby);
    if (dx * dx + dy * dy > reach * reach) return 0.0;
    // B's frame
    double sb, cb, s, c;
    iou_sincos(b[6], sb, cb);
    const double dh = a[6] - b[6];                            // TwoSum: dh + eh == a[6] - b[6] exactly
    const double bv = dh - a[6];
    const double eh = (a[6] - (dh - bv)) + (-b[6] - bv);
    iou_sincos(dh, s, c);
    const double s1 = s + eh * c, c1 = c - eh * s;
    s = s1; c = c1;
    const double ox = dx * cb + dy * sb, oy = dy * cb - dx * sb;
    IouPoly p, q;
    // A's corners (+,+), (-,+), (-,-), (+,-): counter-clockwise
    const double xc = hax * c, xs = hax * s, yc = hay * c, ys = hay * s;
    p.x[0] = ox + (xc - ys);  p.y[0] = oy + (xs + yc);
    p.x[1] = ox + (-xc - ys); p.y[1] = oy + (yc - xs);
    p.x[2] = ox + (ys - xc);  p.y[2] = oy + (-xs - yc);
    p.x[3] = ox + (xc + ys);  p.y[3] = oy + (xs - yc);
#pragma unroll
    for (int k = 4; k < IOU_NV; ++k) p.x[k] = p.y[k] = 0.0;
    p.n = 4;
    iou_clip<0, 4>(p, 1.0, hbx, q);
    iou_clip<0, 5>(q, -1.0, hbx, p);
    iou_clip<1, 6>(p, 1.0, hby, q);
    iou_clip<1, 7>(q, -1.0, hby, p);
    if (p.n < 3) return 0.0;
    double twice = 0.0;
#pragma unroll
    for (int i = 1; i + 1 < IOU_NV; ++i) {
        const double ux = p.x[i] - p.x[0], uy = p.y[i] - p.y[0], vx = p.x[i + 1] - p.x[0], vy = p.y[i + 1] - p.y[0];
        const double tri = ux * vy - vx * uy;
        twice += (i + 1 < p.n) ? tri : 0.0;
    }
    double area = 0.5 * (twice < 0.0 ? -twice : twice);
    if (!(area > 0.0)) return 0.0;
    if (mode == VG_IOU_BEV_AREA) return area;
    const double fa = a[3] * a[4], fb = b[3] * b[4];
    if (mode == VG_IOU_BEV) {
        const double uni = fa + fb - area;
        return uni > 0.0 ? area / uni : 0.0;
    }
    const double inter = area * zov;
    const double uni = fa * a[5] + fb * b[5] - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}
