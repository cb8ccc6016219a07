// The 2 x 2 solve and the strain invariants shared by k_motion and k_local_strain (k_motion.hip; include/vbs.h states every
// expression).  Float64, every expression evaluated as written: no contraction, sums left to right.
#pragma once
#include <math.h>

#include "common.h"
#pragma clang fp contract(off)

// the centred normal equations of one component: g_x = (xe yy - ye xy) / det, g_y = (ye xx - xe xy) / det
__device__ __forceinline__ void strain_solve(double xx, double xy, double yy, double xe, double ye, double det, double& gx,
                                             double& gy) {
    gx = (xe * yy - ye * xy) / det;
    gy = (ye * xx - xe * xy) / det;
}

struct StrainInv {
    double dilation, omega, e1, e2, max_shear;               // the linearised part: what both kernels emit
    double shear_deg, rot_deg, lambda1, lambda2, tilt_deg;   // the finite part (polar decomposition of F) and the tilt of dZ
};

__device__ __forceinline__ void strain_small(double gxx, double gxy, double gyx, double gyy, StrainInv& v) {
    v.dilation = gxx + gyy;
    v.omega = 0.5 * (gyx - gxy);
    v.e1 = 0.5 * (gxx - gyy);
    v.e2 = 0.5 * (gxy + gyx);
    v.max_shear = sqrt(v.e1 * v.e1 + v.e2 * v.e2);
}

__device__ __forceinline__ void strain_finite(double gxx, double gxy, double gyx, double gyy, double gzx, double gzy, StrainInv& v) {
    const double f11 = 1.0 + gxx, f12 = gxy, f21 = gyx, f22 = 1.0 + gyy;
    const double p = f11 + f22, q = f21 - f12;
    const double a = f11 - f22, b = f12 + f21;
    const double h = sqrt(p * p + q * q), w = sqrt(a * a + b * b);
    v.shear_deg = 0.5 * atan2(v.e2, v.e1) * VBS_DEG;
    v.rot_deg = atan2(q, p) * VBS_DEG;
    v.lambda1 = 0.5 * (h + w);
    v.lambda2 = 0.5 * (h - w);
    v.tilt_deg = atan(sqrt(gzx * gzx + gzy * gzy)) * VBS_DEG;
}
