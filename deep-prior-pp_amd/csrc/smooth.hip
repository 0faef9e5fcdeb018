// smooth.hip -- the One-Euro filter over the tracked and the fused poses, at the end of a tracker's tick (ABI v22; over real time: v24).
//
// THIS PROJECT'S OWN semantics, like fuse.hip's and calib.hip's: the reference draws what the net returns.  They are stated in
// include/dpp_hip.h and restated in NumPy float64 by tests/smooth_ref.py, to which every output and the state are pinned bit for bit:
// all arithmetic is float64 in the stated order (+ - * / sqrt only), every output is rounded to float32 once, and the unit is compiled
// without FMA contraction (csrc/Makefile) like the other units that include geom.h.
//
// One workgroup (one wave) per row: T track rows, then G group rows.  Every lane reads the row's `since` and its validity and forms the
// row's word from them; the lanes stride over the joints, a joint's three coordinates in one lane (the speed needs no cross-lane step);
// lane 0 settles `since` and the word behind a barrier, after all lanes have read the old `since`.  The launch is bound by its launch,
// not by its work.
//
// dpp_pose_smooth_t (ABI v24) is the same kernel body with the elapsed time taken from the sources' stamps instead of counted ticks: the
// TIMED instantiation reads the row's sample time and its last one (`tlast`, a state array of its own), refuses a sample that is not
// later than the last (DPP_SMOOTH_STALE on the not-valid path) and lets lane 0 settle `tlast` with `since`.
#include <cfloat>

#include "geom.h"

namespace {

constexpr int TRACK_OK = 0;                                         // dpp_track_refine's status word (crop.hip)

struct SmoothPar {
    double rate, mincutoff, beta, dcutoff;
    int max_hold;
};

// alpha(fc, Te) = r / (r + 1), r = (2 pi fc) Te
__device__ __forceinline__ double smooth_alpha(double fc, double Te) {
    const double r = (6.283185307179586 * fc) * Te;
    return r / (r + 1.0);
}

template <bool TIMED>
__global__ __launch_bounds__(DPP_WAVE) void pose_smooth_kernel(const float* __restrict__ pose3d, const int* __restrict__ status,
                                                               const int* __restrict__ src, int T, int J,
                                                               const float* __restrict__ fused_pose, const int* __restrict__ n_in,
                                                               const SourceRec* __restrict__ tab, AugCam cam, SmoothPar par,
                                                               int* since, double* __restrict__ xh, double* __restrict__ dxh,
                                                               float* __restrict__ pose_f, float* __restrict__ pose_img_f,
                                                               int* __restrict__ sstat, float* __restrict__ fused_pose_f,
                                                               int* __restrict__ gstat, const double* __restrict__ stamps, int C,
                                                               double* tlast) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool track = r < T;
    const int g = r - T;
    const int old = since[r];
    bool valid = track ? status[r] == TRACK_OK : n_in[g] >= 1;
    const float* x = track ? pose3d + (size_t)r * J * 3 : fused_pose + (size_t)g * J * 3;
    float* out = track ? pose_f + (size_t)r * J * 3 : fused_pose_f + (size_t)g * J * 3;
    float* img = track ? pose_img_f + (size_t)r * J * 3 : nullptr;
    double* sx = xh + (size_t)r * J * 3;
    double* sd = dxh + (size_t)r * J * 3;
    if (track) source_camera(tab, tab ? src[r] : 0, cam);              // the track's own camera

    // TIMED: the sample's time is its source's stamp (a group's: the tick's instant); Te is read only where old >= 0
    double Te = 0.0, s = 0.0;
    int stale = 0;
    if (TIMED) {
        s = track ? stamps[src ? src[r] : 0] : stamps[C];
        Te = s - tlast[r];
        if (valid && old >= 0 && !(Te > 0.0)) { valid = false; stale = DPP_SMOOTH_STALE; }      // not later than the last one: refused
    } else {
        Te = (double)(old + 1) / par.rate;                             // read only by the OK branch, where old >= 0
    }

    int word, now;
    if (valid) { word = old < 0 ? DPP_SMOOTH_INIT : DPP_SMOOTH_OK; now = 0; }
    else if (old < 0) { word = DPP_SMOOTH_EMPTY; now = -1; }
    else if (old >= par.max_hold) { word = DPP_SMOOTH_EMPTY | DPP_SMOOTH_DROPPED; now = -1; }      // since + 1 > max_hold
    else { word = DPP_SMOOTH_HELD; now = old + 1; }

    const double ad = smooth_alpha(par.dcutoff, Te);
    for (int j = lane; j < J; j += DPP_WAVE) {
        float o[3] = {0.0f, 0.0f, 0.0f};
        if (word == DPP_SMOOTH_INIT) {
            for (int d = 0; d < 3; ++d) {
                o[d] = x[j * 3 + d];
                sx[j * 3 + d] = (double)o[d];
                sd[j * 3 + d] = 0.0;
            }
        } else if (word == DPP_SMOOTH_OK) {
            double xs[3], h[3], v[3];
            for (int d = 0; d < 3; ++d) { xs[d] = (double)x[j * 3 + d]; h[d] = sx[j * 3 + d]; v[d] = sd[j * 3 + d]; }     // nine loads in flight
            for (int d = 0; d < 3; ++d) {
                const double dv = (xs[d] - h[d]) / Te;
                v[d] = ad * dv + (1.0 - ad) * v[d];
            }
            const double speed = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            const double a = smooth_alpha(par.mincutoff + par.beta * speed, Te);
            for (int d = 0; d < 3; ++d) {
                h[d] = a * xs[d] + (1.0 - a) * h[d];
                sx[j * 3 + d] = h[d];
                sd[j * 3 + d] = v[d];
                o[d] = (float)h[d];
            }
        } else if (word == DPP_SMOOTH_HELD) {
            for (int d = 0; d < 3; ++d) o[d] = (float)sx[j * 3 + d];
        }
        for (int d = 0; d < 3; ++d) out[j * 3 + d] = o[d];
        if (img) {
            float u[3] = {0.0f, 0.0f, 0.0f};                           // an EMPTY row is not projected
            if (!(word & DPP_SMOOTH_EMPTY)) toimg(cam, (double)o[0], (double)o[1], (double)o[2], true, u);
            for (int d = 0; d < 3; ++d) img[j * 3 + d] = u[d];
        }
    }
    __syncthreads();                                                   // every lane has read the old `since`
    if (lane == 0) {
        since[r] = now;
        if (TIMED && valid) tlast[r] = s;                              // INIT and OK
        if (track) sstat[r] = word | stale;
        else gstat[g] = word | stale;
    }
}

inline bool positive_finite(double v) { return v > 0.0 && v <= DBL_MAX; }      // false for NaN and +inf

}  // namespace

extern "C" int dpp_pose_smooth(const float* pose3d, const int* status, const int* src, int T, int J, const float* fused_pose, const int* n, int G,
                               const void* sources, double fx, double fy, double ux, double uy, int flip_y, double rate, double mincutoff,
                               double beta, double dcutoff, int max_hold, int* since, double* xh, double* dxh, float* pose_f, float* pose_img_f,
                               int* sstat, float* fused_pose_f, int* gstat, dpp_stream_t stream) {
    if (!pose3d || !status || !since || !xh || !dxh || !pose_f || !pose_img_f || !sstat) return DPP_E_BADARG;
    if (T < 1 || J < 1 || G < 0 || max_hold < 0) return DPP_E_BADARG;
    if (G > 0 && (!fused_pose || !n || !fused_pose_f || !gstat)) return DPP_E_BADARG;
    if (sources && !src) return DPP_E_BADARG;                            // a table needs src; without one src goes unread
    if (!positive_finite(rate) || !positive_finite(mincutoff) || !positive_finite(dcutoff) || !(beta >= 0.0) || !(beta <= DBL_MAX))
        return DPP_E_BADARG;
    if (!sources && (fx == 0.0 || fy == 0.0)) return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    SmoothPar par;
    par.rate = rate; par.mincutoff = mincutoff; par.beta = beta; par.dcutoff = dcutoff; par.max_hold = max_hold;
    DPP_LAUNCH(pose_smooth_kernel<false>, dim3(T + G), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), pose3d, status, src, T, J, fused_pose,
               n, static_cast<const SourceRec*>(sources), cam, par, since, xh, dxh, pose_f, pose_img_f, sstat, fused_pose_f, gstat,
               static_cast<const double*>(nullptr), 0, static_cast<double*>(nullptr));
    return dpp_launch_status();
}

extern "C" int dpp_pose_smooth_t(const float* pose3d, const int* status, const int* src, int T, int J, const float* fused_pose, const int* n, int G,
                                 const void* sources, double fx, double fy, double ux, double uy, int flip_y, const double* stamps, int C,
                                 double mincutoff, double beta, double dcutoff, int max_hold, int* since, double* tlast, double* xh, double* dxh,
                                 float* pose_f, float* pose_img_f, int* sstat, float* fused_pose_f, int* gstat, dpp_stream_t stream) {
    if (!pose3d || !status || !stamps || !since || !tlast || !xh || !dxh || !pose_f || !pose_img_f || !sstat) return DPP_E_BADARG;
    if (T < 1 || J < 1 || G < 0 || C < 1 || max_hold < 0) return DPP_E_BADARG;
    if (G > 0 && (!fused_pose || !n || !fused_pose_f || !gstat)) return DPP_E_BADARG;
    if (sources && !src) return DPP_E_BADARG;                            // a table needs src; without src every track is source 0
    if (!positive_finite(mincutoff) || !positive_finite(dcutoff) || !(beta >= 0.0) || !(beta <= DBL_MAX)) return DPP_E_BADARG;
    if (!sources && (fx == 0.0 || fy == 0.0)) return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    SmoothPar par;
    par.rate = 0.0; par.mincutoff = mincutoff; par.beta = beta; par.dcutoff = dcutoff; par.max_hold = max_hold;     // rate: unread
    DPP_LAUNCH(pose_smooth_kernel<true>, dim3(T + G), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), pose3d, status, src, T, J, fused_pose,
               n, static_cast<const SourceRec*>(sources), cam, par, since, xh, dxh, pose_f, pose_img_f, sstat, fused_pose_f, gstat, stamps, C,
               tlast);
    return dpp_launch_status();
}
