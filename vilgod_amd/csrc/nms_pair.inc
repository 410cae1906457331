// The per-pair and per-row rules of the box NMS (csrc/nms.hip), `__host__ __device__`: the kernels and vg_boxes_nms_host run the SAME
// text, compiled with -ffp-contract=off, so the device and the host keep the same rows bit for bit.
//
//   nms_before        the strict total order of the ranking: score descending, row index ascending, a NaN score behind every number
//   nms_row_ok        may this row be kept / suppress?  (its score is a number and the five box values that are read are finite)
//   nms_normal_pair   pcdet's nms_normal_gpu value: the axis-aligned BEV IoU, headings ignored
//   nms_value         the value of a mode for (a = the later row, b = the kept row)
//
// Only + - * / and comparisons, all float64 (float32 inputs are widened exactly by the caller).
#pragma once

#include "iou_pair.inc"

// does key (sj, j) stand before key (si, i)?  j != i.  +-0.0 are one score; NaN scores come last, by row index among themselves.
VG_HD bool nms_before(double sj, int j, double si, int i) {
    const bool nj = sj != sj, ni = si != si;
    if (nj || ni) return nj ? (ni && j < i) : true;
    return sj > si || (sj == si && j < i);
}

VG_HD bool nms_finite(double v) { return v - v == 0.0; }          // inf - inf and NaN - NaN are NaN

// v: the row's 7 box values.  z and dz (v[2], v[5]) are not read by either mode and are not looked at here.
VG_HD bool nms_row_ok(double score, const double* v) {
    return score == score && nms_finite(v[0]) && nms_finite(v[1]) && nms_finite(v[3]) && nms_finite(v[4]) && nms_finite(v[6]);
}

// The axis-aligned BEV IoU of a and b, formed relative to b's centre like iou_pair (the value does not depend on where the pair
// stands).  Exactly 0.0 for an extent <= 0, a non-positive overlap on either axis or a non-positive union.
VG_HD double nms_normal_pair(const double* a, const double* b) {
    if (!(a[3] > 0.0) || !(a[4] > 0.0) || !(b[3] > 0.0) || !(b[4] > 0.0)) return 0.0;
    const double dx = a[0] - b[0], dy = a[1] - b[1];
    const double ahx = 0.5 * a[3], ahy = 0.5 * a[4], bhx = 0.5 * b[3], bhy = 0.5 * b[4];
    const double x1 = dx + ahx < bhx ? dx + ahx : bhx, x0 = dx - ahx > -bhx ? dx - ahx : -bhx;
    const double y1 = dy + ahy < bhy ? dy + ahy : bhy, y0 = dy - ahy > -bhy ? dy - ahy : -bhy;
    const double ix = x1 - x0, iy = y1 - y0;
    if (!(ix > 0.0) || !(iy > 0.0)) return 0.0;
    const double inter = ix * iy;
    const double uni = a[3] * a[4] + b[3] * b[4] - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

VG_HD double nms_value(const double* a, const double* b, int mode) {
    return mode == VG_NMS_ROTATED ? iou_pair(a, b, VG_IOU_BEV) : nms_normal_pair(a, b);
}
