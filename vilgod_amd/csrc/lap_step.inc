// The per-element steps of the linear-assignment solver (csrc/lap.hip), shared by the kernel and vg_lap_groups_host: what is done
// to ONE column (or one row's "stay unassigned" choice) in each phase of a shortest-augmenting-path search.  The kernel deals the
// columns to lanes, the host form walks them in order; every value is formed by the text below, the only reduction is a minimum over a
// strict total order of keys, so the two agree bit for bit.  All float64; no multiplication, so nothing can be contracted.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAP_HD __host__ __device__ __forceinline__
#else
#define LAP_HD inline
#endif

#define LAP_TAG_NONE 0x7fffffff

// NaN and -inf are refused (status 2); +inf forbids the pair
LAP_HD bool lap_invalid(double c) { return !(c == c) || c == -INFINITY; }

// the second half of a candidate's key: a free column ahead of an assigned one, then the lower column index.  Columns are below
// 2 * VG_LAP_MAX (the "stay unassigned" choice of row i is column m + i, always free).
LAP_HD int lap_tag(bool assigned, int col) { return (assigned ? 1 << 16 : 0) | col; }
LAP_HD int lap_tag_col(int tag) { return tag & 0xffff; }
LAP_HD bool lap_tag_assigned(int tag) { return (tag >> 16) != 0; }

// (cost, tag) < (cost', tag'): the strict total order the arg-min reduces over
LAP_HD bool lap_key_less(double ca, int ta, double cb, int tb) { return ca < cb || (ca == cb && ta < tb); }

// row i, reached at path cost minv, offers column j the path cost ((minv + c) - u[i]) - v[j]; a strictly smaller offer replaces the
// column's
LAP_HD void lap_relax(double minv, double c, double ui, double vj, int i, double& shortj, int& predj) {
    if (c < INFINITY) {
        const double r = ((minv + c) - ui) - vj;
        if (r < shortj) { shortj = r; predj = i; }
    }
}

// the path cost of leaving row i unassigned: its private column has the cost `unassigned` and a dual that stays 0
LAP_HD double lap_unassigned_offer(double minv, double unassigned, double ui) { return (minv + unassigned) - ui; }

// the running best "stay unassigned" choice of a search: lower offer, then lower row
LAP_HD void lap_unassigned_best(double offer, int i, double& dmin, int& drow) {
    if (offer < dmin || (offer == dmin && offer < INFINITY && i < drow)) { dmin = offer; drow = i; }
}

// the search ended at path cost minv: a visited column that is not the sink moves its dual and its row's by minv - short[j]
LAP_HD void lap_dual(double minv, double shortj, double& ur, double& vj) {
    const double d = minv - shortj;
    ur = ur + d;
    vj = vj - d;
}
