// geom.h -- the camera, crop-bounds and warp-coordinate arithmetic that augment.hip, crop.hip, components.hip, prior.hip, fuse.hip, smooth.hip, visibility.hip and align.hip share,
// and the workgroup reductions of the whole-frame kernels (crop.hip, components.hip, ingest.hip, background.hip).
//
// Everything here restates NumPy / OpenCV 2.4 arithmetic that rounds after every operation and is pinned bit for bit to the reference,
// so every unit that uses that arithmetic is compiled with -ffp-contract=off (csrc/Makefile names them; ingest.hip takes
// only the min / max reductions and the source table, which do not round; background.hip is listed for its own cut-map arithmetic).  One body per rule: a fix
// made here reaches every kernel that applies the rule.
#pragma once
#include "dpp_common.h"

namespace {

constexpr int MAXJ3 = 192;     // up to 64 joints x 3

struct AugCam {
    double fx, fy, ux, uy;
    int flip_y;
};

// jointImgTo3D / joint3DToImg on float32 arrays evaluated in float64 and stored as float32 (importers.py:80-119)
__device__ __forceinline__ void to3d(const AugCam& c, double u, double v, double d, float out[3]) {
    out[0] = (float)((u - c.ux) * d / c.fx);
    out[1] = (float)((c.flip_y ? (c.uy - v) : (v - c.uy)) * d / c.fy);
    out[2] = (float)d;
}

// joint3DToImg; f32in: the sample is a float32 array, so sample[0]/sample[2] is a float32 division
__device__ __forceinline__ void toimg(const AugCam& c, double x, double y, double z, bool f32in, float out[3]) {
    if (z == 0.0) { out[0] = (float)c.ux; out[1] = (float)c.uy; out[2] = 0.0f; return; }
    double q0 = x / z, q1 = y / z;
    if (f32in) { q0 = (double)((float)x / (float)z); q1 = (double)((float)y / (float)z); }
    out[0] = (float)(q0 * c.fx + c.ux);
    out[1] = (float)(c.flip_y ? (c.uy - q1 * c.fy) : (q1 * c.fy + c.uy));
    out[2] = (float)z;
}

// comToBounds (handdetector.py:204-226); a float32 centre is widened by the caller first
__device__ __forceinline__ void com_to_bounds(const double com[3], const double size[3], double fx, double fy, int b[4]) {
    const double c0 = com[0], c1 = com[1], c2 = com[2];
    b[0] = (int)floor((c0 * c2 / fx - size[0] / 2.) / c2 * fx + 0.5);
    b[1] = (int)floor((c0 * c2 / fx + size[0] / 2.) / c2 * fx + 0.5);
    b[2] = (int)floor((c1 * c2 / fy - size[1] / 2.) / c2 * fy + 0.5);
    b[3] = (int)floor((c1 * c2 / fy + size[1] / 2.) / c2 * fy + 0.5);
}

__device__ __forceinline__ long long floordiv(long long a, long long b) {   // python-2 integer division
    long long q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

__device__ __forceinline__ void mat3_mul(const double A[9], const double B[9], double C[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += A[i * 3 + k] * B[k * 3 + j];
            C[i * 3 + j] = s;
        }
}

__device__ __forceinline__ void mat3_inv(const double S[9], double t[9]) {     // cv::invert, 3x3 cofactor branch
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (d == 0.0) { for (int i = 0; i < 9; ++i) t[i] = 0.0; return; }
    d = 1. / d;
    t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
    t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
    t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
    t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
    t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
    t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
    t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
}

__device__ __forceinline__ long long cv_round(double v) { return (long long)rint(v); }

// Source pixel (X, Y) of destination pixel (x, y) under cv::warpAffine, INTER_NEAREST: 10-bit fixed point, m[0..5] the inverse map.
// The y terms do not depend on x: a caller that walks a row gets them formed once (the calls are inlined).
__device__ __forceinline__ void affine_source(const double* m, int x, int y, long long& X, long long& Y) {
    const long long ad = cv_round(m[0] * (double)x * 1024.), bd = cv_round(m[3] * (double)x * 1024.);
    const long long X0 = cv_round((m[1] * (double)y + m[2]) * 1024.) + 512;
    const long long Y0 = cv_round((m[4] * (double)y + m[5]) * 1024.) + 512;
    X = (X0 + ad) >> 10; Y = (Y0 + bd) >> 10;
}

// The same under cv::warpPerspective: cvRound of the float64 coordinate, saturated to short; bx = (x >> 6) << 6 is the first column
// of x's 64-wide destination block, whose terms (nine float64 products) are likewise formed once per row and block.  divide = false
// skips the float64 division by W: only for a map whose bottom row is EXACTLY (0, 0, 1), where W = 0 * x + 0 * y + 1 = 1, 1. / W = 1
// and X * 1. = X bit for bit.
__device__ __forceinline__ void persp_source(const double* m, int bx, int x, int y, bool divide, long long& X, long long& Y) {
    const double x1 = (double)(x - bx), fbx = (double)bx, fy_ = (double)y;
    const double X0 = m[0] * fbx + m[1] * fy_ + m[2];
    const double Y0 = m[3] * fbx + m[4] * fy_ + m[5];
    const double W0 = m[6] * fbx + m[7] * fy_ + m[8];
    double Wv = 1.0;
    if (divide) {
        Wv = W0 + m[6] * x1;
        Wv = (Wv != 0.0) ? 1. / Wv : 0.;
    }
    const double fX = fmax(-2147483648.0, fmin(2147483647.0, (X0 + m[0] * x1) * Wv));
    const double fY = fmax(-2147483648.0, fmin(2147483647.0, (Y0 + m[3] * x1) * Wv));
    X = cv_round(fX); Y = cv_round(fY);
    X = X < -32768 ? -32768 : (X > 32767 ? 32767 : X);
    Y = Y < -32768 ? -32768 : (Y > 32767 ? 32767 : Y);
}

// The z-threshold of getCrop / recropHand / getInverseCrop: a non-zero value below zlo becomes zlo, above zhi becomes 0.
// (Written as two guarded assignments, not as a nest under v != 0: this form compiles to selects, the nest to branches.)
__device__ __forceinline__ float z_threshold(float v, float zlo, float zhi) {
    if (v < zlo && v != 0.0f) v = zlo;
    else if (v > zhi && v != 0.0f) v = 0.0f;
    return v;
}

// numpy.isclose(v, ref) of a float32 pixel against recropHand's nv_val (handdetector.py:782-803; NumPy 1: the comparison is float64)
__device__ __forceinline__ bool is_close(float v, double ref) { return fabs((double)v - ref) <= 1e-8 + 1e-5 * fabs(ref); }


// a centre that cannot be cropped around: its depth is numpy.isclose to 0 (comToBounds' "CoM ill-defined" test) or it is not finite
// (crop.hip's tracking launches, fuse.hip's peer centre)
__device__ __forceinline__ bool com_ill_defined(const float c[3]) {
    const bool finite = fabs((double)c[0]) <= 3.4e38 && fabs((double)c[1]) <= 3.4e38 && fabs((double)c[2]) <= 3.4e38;   // false for NaN
    return !finite || fabs((double)c[2]) <= 1e-8;
}


// ---- workgroup reductions that crop.hip and components.hip share ---------------------------------------------------------------
// The four sums over the workgroup: wave shuffle, then LDS, then thread 0 -- the only thread that gets `true` and the totals.
__device__ __forceinline__ bool com_block_sums(double& sx, double& sy, double& sd, double& cnt, double (*s_red)[DPP_THREADS / DPP_WAVE]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); sd += __shfl_xor(sd, o); cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { s_red[0][wave] = sx; s_red[1][wave] = sy; s_red[2][wave] = sd; s_red[3][wave] = cnt; }
    __syncthreads();
    if (tid != 0) return false;
    for (int w = 1; w < DPP_THREADS / DPP_WAVE; ++w) { sx += s_red[0][w]; sy += s_red[1][w]; sd += s_red[2][w]; cnt += s_red[3][w]; }
    return true;
}

// (mn, mx) over the workgroup: wave shuffle, then LDS, then thread 0 -- the only thread that gets `true` and the result.
__device__ __forceinline__ bool block_minmax(float& mn, float& mx, float* s_mn, float* s_mx) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    if ((tid & 63) == 0) { s_mn[tid >> 6] = mn; s_mx[tid >> 6] = mx; }
    __syncthreads();
    if (tid != 0) return false;
    for (int w = 1; w < DPP_THREADS / DPP_WAVE; ++w) { mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]); }
    return true;
}

constexpr int FR_BANDS = 64;            // workgroups per frame of the depth-range pass (= one wave of partials to reduce)

// (min, max) of frame b from its FR_BANDS partials: one wave, lane = band; every lane returns the result
__device__ __forceinline__ void frame_range_reduce(const float* __restrict__ partial, int b, int lane, float& mn, float& mx) {
    mn = partial[((size_t)b * FR_BANDS + lane) * 2];
    mx = partial[((size_t)b * FR_BANDS + lane) * 2 + 1];
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
}

// ---- frame sources of unlike cameras and sizes (ABI v19) --------------------------------------------------------------------------
// One record per frame source: its camera, what HandDetector is handed (crop_fx, crop_fy: already absolute), its frame size and where
// its frame starts in the ragged float32 frame buffer and in the ragged raw sensor buffer (ELEMENT offsets, padded by the host to 16
// bytes).  The kernels that read a frame or a camera take a pointer to the table: null in the plain and *_ix entry points, where the
// scalars of the launch hold for every row as before.  The host has validated the table; the kernels trust it.
struct SourceRec {
    double fx, fy, ux, uy;
    double crop_fx, crop_fy;
    long long frame_off, raw_off;
    int H, W, flip_y, pad_;
};

// Source c's float32 frame and its size: from the table, or frame c of equal [H][W] frames.  c is uniform over a workgroup.
__device__ __forceinline__ const float* source_frame(const float* __restrict__ frames, const SourceRec* __restrict__ tab, int c, int& H, int& W) {
    if (tab == nullptr) return frames + (size_t)c * H * W;
    H = tab[c].H; W = tab[c].W;
    return frames + tab[c].frame_off;
}

__device__ __forceinline__ void source_camera(const SourceRec* __restrict__ tab, int c, AugCam& cam) {
    if (tab == nullptr) return;
    cam.fx = tab[c].fx; cam.fy = tab[c].fy; cam.ux = tab[c].ux; cam.uy = tab[c].uy; cam.flip_y = tab[c].flip_y;
}

}  // namespace
