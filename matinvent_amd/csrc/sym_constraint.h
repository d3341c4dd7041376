// The arithmetic of the symmetry constraint (include/matinvent_hip_symc.h), host and device: the pull-back of an atom from its
// orbit representative, one slot of the metric's group sum, and the Cholesky cell of the mean.  sym_constraint.hip calls these functions
// with its thread index, scripts/sym_constraint_host_check.cpp runs the same text with the index as a loop variable under the host
// sanitizers.  Conventions of sym_ops.h / sym_refine.h, whose wrap, rigid metric, congruence and tree step are used as they stand: float64
// or exact integers, every operation rounded separately, sqrt and floor the only library functions, so that tests/symc_ref64.py
// reproduces the bits.
//
// Everything is in the basis of the state's own cell: an operation is g_k(f) = f W_k^-1 + t_k.  Per atom j the host prepared the affine map
// (Q_j, d_j) from the orbit representative's coordinates to the atom's: x_j = wrap(x_r Q_j + d_j).
#pragma once
#include "sym_refine.h"

namespace mi {

enum { SYMC_MAX_ATOMS = 256, SYMC_MAX_OPS = SYM_MAX_OPS, SYMC_THREADS = 256, SYMC_QUADS = 25 };

#pragma clang fp contract(off)

// det W = +-1: the rotation part of an operation is a lattice map
SM_HD bool symc_unimodular(const int* W) {
    const int d = sm_idet3(W);
    return d == 1 || d == -1;
}

// the coordinates of one atom from its representative's float32 coordinates: wrap(x_r Q + d) as float32 in [0, 1), sym_prim_frac's
// rounding rule (a float that rounds to 1 is 0)
SM_HD void symc_coord(const float* xr32, const double* Q, const double* d, float* out) {
    const double x0 = (double)xr32[0], x1 = (double)xr32[1], x2 = (double)xr32[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float w = (float)sm_wrap01(((x0 * Q[c] + x1 * Q[3 + c]) + x2 * Q[6 + c]) + d[c]);
        out[c] = w >= 1.0f ? 0.0f : w;
    }
}

// the metric of the float32 cell in float64
SM_HD void symc_metric(const float* lat32, double* G) {
    double L[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) L[e] = (double)lat32[e];
    sym_metric(L, G);
}

// slot k of the group sum: W_k G W_k^T for k < R, zeros above (the tree over SYMC_THREADS slots is a function of the slot count alone)
SM_HD void symc_slot(const int* rot, int R, int k, const double* G, double* out) {
    if (k < R) {
        refine_congruence(rot + 9 * k, G, out);
    } else {
#pragma unroll
        for (int e = 0; e < 9; ++e) out[e] = 0.0;
    }
}

// The projected cell from the tree's sums: Gbar = Gsum / R, out = its lower Cholesky factor as float32 (rows are the cell vectors: a along
// x, b in the xy plane).  false, and out is not to be used: a non-finite entry of Gbar, or a pivot that is not positive.
SM_HD bool symc_cell(const double* Gsum, int R, float* out) {
    double Gc[9];
    bool finite = true;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        Gc[e] = Gsum[e] / (double)R;
        finite = finite && sm_finite(Gc[e]);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = 0.0f;
    if (!finite) return false;
    if (!(Gc[0] > 0.0)) return false;
    const double l00 = sqrt(Gc[0]), l10 = Gc[3] / l00, l20 = Gc[6] / l00;
    const double p1 = Gc[4] - l10 * l10;
    if (!(p1 > 0.0)) return false;
    const double l11 = sqrt(p1), l21 = (Gc[7] - l20 * l10) / l11;
    const double p2 = (Gc[8] - l20 * l20) - l21 * l21;
    if (!(p2 > 0.0)) return false;
    out[0] = (float)l00, out[3] = (float)l10, out[4] = (float)l11, out[6] = (float)l20, out[7] = (float)l21, out[8] = (float)sqrt(p2);
    return true;
}

}  // namespace mi
