// calib.hip -- running sums for the extrinsics of a camera, taken from the hand the tracker follows anyway (ABI v21).
//
// THIS PROJECT'S OWN semantics, like fuse.hip's: the reference has one camera.  They are stated in include/dpp_hip.h and restated in
// NumPy float64 by tests/calib_ref.py, to which the accumulator is pinned bit for bit: all arithmetic is float64 in the stated order, no
// atomics, and the unit is compiled without FMA contraction (csrc/Makefile).  The rigid fit itself (a 3 x 3 SVD, once per calibration)
// is host work: hipdp/calib.py.
//
// One workgroup (one wave) per source to be calibrated.  Per group the first K lanes look at one member each (so the K loads overlap)
// and leave the anchor's and the source's member in LDS; all lanes then stride over the J joints into private partials, which one xor
// butterfly reduces after the last group.  The launch is bound by its launch, not by its work.
#include "rigid.h"

namespace {

constexpr int TRACK_OK = 0;                                         // dpp_track_refine's status word (crop.hip)
constexpr int NSUM = 18;                                            // n, sum p [3], sum q [3], S [3][3], sum |p|^2, sum |q|^2

struct CalList {                                                    // by value: the entry point has checked every entry
    int src[DPP_CALIB_MAX_SOURCES];
};

// v = v + shfl_xor(v, off) for off = 32 .. 1: both partners form the same sum (addition commutes), so every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(DPP_WAVE) void extrinsics_accumulate_kernel(const float* __restrict__ pose3d, const int* __restrict__ status,
                                                                         const int* __restrict__ src, int J, const double* __restrict__ extr,
                                                                         const int* __restrict__ members, const int* __restrict__ offsets,
                                                                         int G, int anchor, CalList cal, double max_shape_dev,
                                                                         double* __restrict__ acc) {
    __shared__ int s_pair[2][2];                 // [g & 1]: the group's member on the anchor source, and on this one (-1: none)
    const int k = blockIdx.x, lane = threadIdx.x;
    const int c = cal.src[k];
    const double* ea = extr + (size_t)anchor * 12;
    double v[NSUM];
    for (int i = 0; i < NSUM; ++i) v[i] = 0.0;
    double pairs = 0.0, refused = 0.0;           // the same in every lane: whether a pair takes part is decided from wave-wide values

    for (int g = 0; g < G; ++g) {
        const int m0 = offsets[g];
        const int k_all = offsets[g + 1] - m0;
        const int K = k_all < DPP_FUSE_MAX_MEMBERS ? k_all : DPP_FUSE_MAX_MEMBERS;      // (the host refuses larger groups)
        int* pair = s_pair[g & 1];
        if (lane == 0) { pair[0] = -1; pair[1] = -1; }
        __syncthreads();
        if (lane < K) {                          // members read pairwise distinct sources: at most one writer per slot
            const int t = members[m0 + lane];
            const int s = src[t];
            if (s == anchor) pair[0] = t;
            else if (s == c) pair[1] = t;
        }
        __syncthreads();
        const int a = pair[0], m = pair[1];
        if (a < 0 || m < 0 || status[a] != TRACK_OK || status[m] != TRACK_OK) continue;
        const float* pa = pose3d + (size_t)a * J * 3;
        const float* pm = pose3d + (size_t)m * J * 3;
        auto joint = [&](int j, double p[3], double q[3]) {
            const double qa[3] = {(double)pa[j * 3], (double)pa[j * 3 + 1], (double)pa[j * 3 + 2]};
            for (int d = 0; d < 3; ++d) p[d] = (double)pm[j * 3 + d];
            to_world(ea, qa, q);
        };
        if (max_shape_dev > 0.0) {               // rigid motions keep distances: the two views of one hand have one shape
            double sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
            for (int j = lane; j < J; j += DPP_WAVE) {
                double p[3], q[3];
                joint(j, p, q);
                for (int d = 0; d < 3; ++d) { sp[d] = sp[d] + p[d]; sq[d] = sq[d] + q[d]; }
            }
            double pc[3], qc[3];
            for (int d = 0; d < 3; ++d) { pc[d] = wave_sum(sp[d]) / (double)J; qc[d] = wave_sum(sq[d]) / (double)J; }
            double worst = 0.0;
            for (int j = lane; j < J; j += DPP_WAVE) {
                double p[3], q[3];
                joint(j, p, q);
                worst = fmax(worst, fabs(dist3(p, pc) - dist3(q, qc)));
            }
            worst = wave_max(worst);
            if (!(worst <= max_shape_dev)) { refused = refused + 1.0; continue; }
        }
        pairs = pairs + 1.0;
        for (int j = lane; j < J; j += DPP_WAVE) {
            double p[3], q[3];
            joint(j, p, q);
            v[0] = v[0] + 1.0;
            for (int d = 0; d < 3; ++d) v[1 + d] = v[1 + d] + p[d];
            for (int d = 0; d < 3; ++d) v[4 + d] = v[4 + d] + q[d];
            for (int d = 0; d < 3; ++d)
                for (int e = 0; e < 3; ++e) v[7 + d * 3 + e] = v[7 + d * 3 + e] + p[d] * q[e];
            v[16] = v[16] + ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
            v[17] = v[17] + ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        }
    }
    for (int i = 0; i < NSUM; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0) {
        double* row = acc + (size_t)k * DPP_CALIB_SLOTS;
        for (int i = 0; i < NSUM; ++i) row[i] = row[i] + v[i];
        row[NSUM] = row[NSUM] + pairs;
        row[NSUM + 1] = row[NSUM + 1] + refused;
    }
}

}  // namespace

extern "C" int dpp_extrinsics_accumulate(const float* pose3d, const int* status, const int* src, int T, int J, const double* extrinsics, int C,
                                         const int* members, const int* offsets, int G, int anchor, const int* cal_src, int n_cal,
                                         double max_shape_dev, double* acc, dpp_stream_t stream) {
    static_assert(NSUM + 2 == DPP_CALIB_SLOTS, "accumulator layout");
    if (!pose3d || !status || !src || !extrinsics || !members || !offsets || !cal_src || !acc) return DPP_E_BADARG;
    if (T < 1 || J < 1 || C < 1 || G < 1 || G > T || n_cal < 1 || n_cal > DPP_CALIB_MAX_SOURCES || anchor < 0 || anchor >= C) return DPP_E_BADARG;
    if (!(max_shape_dev >= 0.0) || !(max_shape_dev <= 1.7e308)) return DPP_E_BADARG;
    CalList cal;
    for (int i = 0; i < DPP_CALIB_MAX_SOURCES; ++i) cal.src[i] = 0;
    for (int i = 0; i < n_cal; ++i) {
        if (cal_src[i] < 0 || cal_src[i] >= C || cal_src[i] == anchor) return DPP_E_BADARG;
        cal.src[i] = cal_src[i];
    }
    DPP_LAUNCH(extrinsics_accumulate_kernel, dim3(n_cal), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), pose3d, status, src, J, extrinsics,
               members, offsets, G, anchor, cal, max_shape_dev, acc);
    return dpp_launch_status();
}
