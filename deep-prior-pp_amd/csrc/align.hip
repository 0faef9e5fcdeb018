// align.hip -- every track of a tick brought to the tick's one instant, before anything combines tracks (ABI v24).
//
// THIS PROJECT'S OWN semantics, like fuse.hip's, calib.hip's and smooth.hip's: the reference has one camera and nothing to align.  They
// are stated in include/dpp_hip.h and restated in NumPy float64 by tests/align_ref.py, to which every output and the state are pinned bit
// for bit: all arithmetic is float64 in the stated order (+ - * / only), every output is rounded to float32 once, and the unit is compiled
// without FMA contraction (csrc/Makefile) like the other units that include geom.h.
//
// One workgroup (one wave) per track.  Every lane reads the row's `have`, its previous stamp and the two stamps of the tick and forms the
// row's word from them; the lanes stride over the joints, a joint's three coordinates in one lane; lane 0 moves the centre and settles
// `have`, the stamp and the word behind a barrier, after all lanes have read the old ones.  The launch is bound by its launch, not by
// its work.
#include <cfloat>

#include "geom.h"

namespace {

constexpr int TRACK_OK = 0;                                         // dpp_track_refine's status word (crop.hip)

// one coordinate: the constant-velocity step from the previous sample through this one to `now`
__device__ __forceinline__ float align_coord(float x, float xp, double dt, double lead) {
    const double v = ((double)x - (double)xp) / dt;
    return (float)((double)x + v * lead);
}

__global__ __launch_bounds__(DPP_WAVE) void pose_align_kernel(const float* __restrict__ pose3d, const float* __restrict__ com3d,
                                                              const int* __restrict__ status, const int* __restrict__ src, int T, int J,
                                                              const double* __restrict__ stamps, int C,
                                                              const SourceRec* __restrict__ tab, AugCam cam, double max_gap, double max_lead,
                                                              int* have, double* pt, float* __restrict__ pp, float* __restrict__ pc,
                                                              float* __restrict__ pose_t, float* __restrict__ pose_img_t,
                                                              float* __restrict__ com3d_t, float* __restrict__ lead_out,
                                                              int* __restrict__ astat) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const int c = src ? src[t] : 0;
    const bool ok = status[t] == TRACK_OK;
    const int had = have[t];
    const double ts = stamps[c], now = stamps[C];
    const double dt = ts - pt[t], lead = now - ts;                     // dt is read only where had != 0
    const float* x = pose3d + (size_t)t * J * 3;
    float* sp = pp + (size_t)t * J * 3;
    float* out = pose_t + (size_t)t * J * 3;
    float* img = pose_img_t + (size_t)t * J * 3;
    source_camera(tab, c, cam);                                        // the track's own camera

    int word;
    if (!ok) word = DPP_ALIGN_NONE;
    else if (!had) word = DPP_ALIGN_ASIS | DPP_ALIGN_NOPREV;
    else if (!(dt > 0.0 && dt <= max_gap)) word = DPP_ALIGN_ASIS | DPP_ALIGN_GAP;
    else if (!(fabs(lead) <= max_lead)) word = DPP_ALIGN_ASIS | DPP_ALIGN_FAR;
    else word = DPP_ALIGN_MOVED;

    for (int j = lane; j < J; j += DPP_WAVE) {
        float o[3] = {0.0f, 0.0f, 0.0f}, u[3] = {0.0f, 0.0f, 0.0f};    // a NONE row is zeros and is not projected
        if (ok) {
            float xs[3], xp[3];
            for (int d = 0; d < 3; ++d) xs[d] = x[j * 3 + d];
            if (word == DPP_ALIGN_MOVED) {
                for (int d = 0; d < 3; ++d) xp[d] = sp[j * 3 + d];
                for (int d = 0; d < 3; ++d) o[d] = align_coord(xs[d], xp[d], dt, lead);
            } else {
                for (int d = 0; d < 3; ++d) o[d] = xs[d];
            }
            for (int d = 0; d < 3; ++d) sp[j * 3 + d] = xs[d];         // the state is the UNALIGNED sample
            toimg(cam, (double)o[0], (double)o[1], (double)o[2], true, u);
        }
        for (int d = 0; d < 3; ++d) out[j * 3 + d] = o[d];
        for (int d = 0; d < 3; ++d) img[j * 3 + d] = u[d];
    }
    __syncthreads();                                                   // every lane has read the old `have` and stamp
    if (lane == 0) {
        float o[3] = {0.0f, 0.0f, 0.0f};
        if (ok) {
            for (int d = 0; d < 3; ++d) {
                const float cs = com3d[t * 3 + d];
                o[d] = word == DPP_ALIGN_MOVED ? align_coord(cs, pc[t * 3 + d], dt, lead) : cs;
                pc[t * 3 + d] = cs;
            }
            have[t] = 1;
            pt[t] = ts;
        }
        for (int d = 0; d < 3; ++d) com3d_t[t * 3 + d] = o[d];
        lead_out[t] = ok ? (float)lead : 0.0f;
        astat[t] = word;
    }
}

}  // namespace

extern "C" int dpp_pose_align(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* stamps,
                              int C, const void* sources, double fx, double fy, double ux, double uy, int flip_y, double max_gap,
                              double max_lead, int* have, double* pt, float* pp, float* pc, float* pose_t, float* pose_img_t,
                              float* com3d_t, float* lead, int* astat, dpp_stream_t stream) {
    if (!pose3d || !com3d || !status || !stamps || !have || !pt || !pp || !pc || !pose_t || !pose_img_t || !com3d_t || !lead || !astat)
        return DPP_E_BADARG;
    if (T < 1 || J < 1 || C < 1) return DPP_E_BADARG;
    if (sources && !src) return DPP_E_BADARG;                            // a table needs src; without src every track is source 0
    if (!(max_gap > 0.0) || !(max_gap <= DBL_MAX) || !(max_lead >= 0.0) || !(max_lead <= DBL_MAX)) return DPP_E_BADARG;
    if (!sources && (fx == 0.0 || fy == 0.0)) return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    DPP_LAUNCH(pose_align_kernel, dim3(T), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), pose3d, com3d, status, src, T, J, stamps, C,
               static_cast<const SourceRec*>(sources), cam, max_gap, max_lead, have, pt, pp, pc, pose_t, pose_img_t, com3d_t, lead, astat);
    return dpp_launch_status();
}
