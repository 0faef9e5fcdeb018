// visibility.hip -- which joints of a tracked pose the frame shows, behind pose_finish in a tracker's tick (ABI v23).
//
// THIS PROJECT'S OWN semantics, like fuse.hip's, calib.hip's and smooth.hip's: the reference has nothing comparable.  They are stated in
// include/dpp_hip.h and restated in NumPy float64 by tests/visibility_ref.py, to which every output is pinned bit for bit: the
// comparisons are float64 in the stated order, the counts are integers (so the order of their reduction is free), every float output
// is rounded to float32 once, and the unit is compiled without FMA contraction (csrc/Makefile) like the other units that include geom.h.
//
// One workgroup (one wave) per (joint, track).  Every lane forms the joint's pixel and its clipped window -- uniform over the wave --,
// the lanes stride over the window's pixels and count, the two counts travel packed in one int through six shuffles, and lane 0 stores
// the joint's three words.  The launch is bound by its launch, not by its work.
#include <cfloat>

#include "geom.h"

namespace {

constexpr int TRACK_OK = 0;                                         // dpp_track_refine's status word (crop.hip)
constexpr int VIS_RADIUS_MAX = DPP_VIS_MAX_RADIUS;                  // (2 * 8 + 1)^2 = 289 pixels: a count fits the 10 bits it travels in

struct VisPar {
    double margin;
    float hidden;                                                   // (float)hidden_weight, rounded once on the host
    int radius, min_support;
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= FLT_MAX; }      // false for NaN and +-inf

__global__ __launch_bounds__(DPP_WAVE) void joint_visibility_kernel(const float* __restrict__ pose_img, const int* __restrict__ status,
                                                                    const int* __restrict__ src, int J, const float* __restrict__ frames,
                                                                    const SourceRec* __restrict__ tab, int H, int W, VisPar par,
                                                                    float* __restrict__ vis, float* __restrict__ weight,
                                                                    int* __restrict__ vword) {
    const int j = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const size_t o = (size_t)t * J + j;
    float v_out = 0.0f, w_out = 0.0f;
    int word = 0;                                                      // a row that is not OK: written as zeros
    if (status[t] == TRACK_OK) {
        const float* frame = source_frame(frames, tab, src[t], H, W);  // H, W: the track's source's from here on
        const float u = pose_img[o * 3], v = pose_img[o * 3 + 1], zf = pose_img[o * 3 + 2];
        const double z = (double)zf;
        const double px = floor((double)u + 0.5), py = floor((double)v + 0.5);
        word = DPP_VIS_OFFFRAME;
        // compared in double: only a pixel inside the frame is ever converted to int
        if (finite32(u) && finite32(v) && finite32(zf) && z > 0.0 && px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H) {
            const int cx = (int)px, cy = (int)py, r = par.radius;
            const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < W - 1 ? cx + r : W - 1;
            const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < H - 1 ? cy + r : H - 1;
            const int ww = x1 - x0 + 1, n_in = ww * (y1 - y0 + 1);     // >= 1: (cx, cy) itself
            int cnt = 0;                                               // n_on | n_front << 10
            for (int i = lane; i < n_in; i += DPP_WAVE) {
                const int dy = i / ww, dx = i - dy * ww;
                const double d = (double)frame[(size_t)(y0 + dy) * W + (x0 + dx)];
                if (d == 0.0) continue;                                // empty
                const double e = d - z;
                if (e < -par.margin) cnt += 1 << 10;                   // front
                else if (!(e > par.margin)) cnt += 1;                  // on (what is left is behind)
            }
            for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
            const int n_on = cnt & 1023, n_front = cnt >> 10;
            v_out = (float)((double)n_on / (double)n_in);
            word = n_on >= par.min_support ? DPP_VIS_VISIBLE : (n_front >= par.min_support ? DPP_VIS_OCCLUDED : DPP_VIS_UNSUPPORTED);
            w_out = word == DPP_VIS_VISIBLE ? 1.0f : par.hidden;
        }
    }
    if (lane == 0) {
        vis[o] = v_out;
        weight[o] = w_out;
        vword[o] = word;
    }
}

}  // namespace

extern "C" int dpp_joint_visibility(const float* pose_img, const int* status, const int* src, int T, int J, const float* frames, int C,
                                    const void* sources, int H, int W, int radius, double margin, int min_support, double hidden_weight,
                                    float* vis, float* weight, int* vword, dpp_stream_t stream) {
    if (!pose_img || !status || !src || !frames || !vis || !weight || !vword) return DPP_E_BADARG;
    if (T < 1 || J < 1 || C < 1 || radius < 0 || radius > VIS_RADIUS_MAX) return DPP_E_BADARG;
    if (min_support < 1 || min_support > (2 * radius + 1) * (2 * radius + 1)) return DPP_E_BADARG;
    if (!(margin > 0.0) || !(margin <= DBL_MAX) || !(hidden_weight >= 0.0) || !(hidden_weight <= 1.0)) return DPP_E_BADARG;   // NaN fails all
    if (!sources && (H < 1 || W < 1)) return DPP_E_BADARG;
    VisPar par;
    par.margin = margin; par.hidden = (float)hidden_weight; par.radius = radius; par.min_support = min_support;
    DPP_LAUNCH(joint_visibility_kernel, dim3(J, T), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), pose_img, status, src, J, frames,
               static_cast<const SourceRec*>(sources), H, W, par, vis, weight, vword);
    return dpp_launch_status();
}
