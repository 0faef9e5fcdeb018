// rigid.h -- the rigid-motion arithmetic that fuse.hip and calib.hip share: a source's extrinsics e = [R row-major, t] (12 float64) applied
// to a point, its inverse, and the distance of two points.  The orders of evaluation are part of the stated semantics
// (include/dpp_hip.h) and are restated by tests/fuse_ref.py, so both units are compiled with -ffp-contract=off (csrc/Makefile).
#pragma once
#include "dpp_common.h"

namespace {

// w = R p + t, row i as ((R_i0 x + R_i1 y) + R_i2 z) + t_i; e = [R row-major, t]
__device__ __forceinline__ void to_world(const double* __restrict__ e, const double p[3], double w[3]) {
    for (int i = 0; i < 3; ++i) w[i] = ((e[i * 3] * p[0] + e[i * 3 + 1] * p[1]) + e[i * 3 + 2] * p[2]) + e[9 + i];
}

// p = R^T (w - t), row i as (R_0i d0 + R_1i d1) + R_2i d2
__device__ __forceinline__ void to_camera(const double* __restrict__ e, const double w[3], double p[3]) {
    const double d[3] = {w[0] - e[9], w[1] - e[10], w[2] - e[11]};
    for (int i = 0; i < 3; ++i) p[i] = (e[i] * d[0] + e[3 + i] * d[1]) + e[6 + i] * d[2];
}

__device__ __forceinline__ double dist3(const double a[3], const double b[3]) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

}  // namespace
