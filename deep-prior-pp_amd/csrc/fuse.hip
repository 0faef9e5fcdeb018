// fuse.hip -- tracks of ONE hand seen by several calibrated cameras, fused at the end of MultiTracker's tick (ABI v20; per-joint weights:
// ABI v23, dpp_pose_fuse_w -- the same kernel, whose unweighted arithmetic is untouched: `weight` is null for dpp_pose_fuse).
//
// THIS PROJECT'S OWN semantics: the reference has one device and one camera and nothing to compare against.  They are
// stated in include/dpp_hip.h and restated in NumPy by tests/fuse_ref.py, to which every output is pinned bit for bit: all
// arithmetic is float64 in the stated order, every output is rounded to float32 once, and the unit is compiled without FMA
// contraction (csrc/Makefile) like the other units that include geom.h.
//
// One workgroup (one wave) per group.  The first K lanes put their member's status and world centre into LDS; lane 0 settles the
// group's membership from there -- the median test, the inliers, the fused centre; the K lanes then form their member's peer centre and
// the hand-over, and all lanes stride over the J joints.  The launch is bound by its launch, not by its work.
#include "geom.h"
#include "rigid.h"

namespace {

constexpr int TRACK_OK = 0, TRACK_LOST = 1;                         // dpp_track_refine's status word (crop.hip)
constexpr int FUSE_MAX = DPP_FUSE_MAX_MEMBERS;

__global__ __launch_bounds__(DPP_WAVE) void pose_fuse_kernel(const float* __restrict__ pose3d, const float* __restrict__ com3d,
                                                             const int* __restrict__ status, const int* __restrict__ src, int J,
                                                             const double* __restrict__ extr, const int* __restrict__ members,
                                                             const int* __restrict__ offsets, const SourceRec* __restrict__ tab, int H,
                                                             int W, AugCam cam0, double max_dev, int flags, float* com,
                                                             float* __restrict__ fused_pose, float* __restrict__ fused_com,
                                                             float* __restrict__ spread, int* __restrict__ n_out,
                                                             float* __restrict__ peer_com, int* __restrict__ fstat,
                                                             const float* __restrict__ weight, float* __restrict__ fused_weight) {
    __shared__ double s_w[FUSE_MAX][3];          // world centre of member k (contributors only)
    __shared__ double s_sort[FUSE_MAX];
    __shared__ int s_use[FUSE_MAX];              // member k is an inlier: it takes part in the fused outputs
    __shared__ int s_bits[FUSE_MAX];
    __shared__ int s_n;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int m0 = offsets[g];
    const int k_all = offsets[g + 1] - m0;
    const int K = k_all < FUSE_MAX ? k_all : FUSE_MAX;                 // (the host refuses larger groups)
    const int* mem = members + m0;
    // member k's own numbers, one lane each (the loads of the K members overlap instead of queueing behind one lane)
    int my_m = 0, my_c = 0, my_status = TRACK_OK;
    if (tid < K) {
        my_m = mem[tid];
        my_c = src[my_m];
        my_status = status[my_m];
        s_bits[tid] = 0;
        s_use[tid] = my_status == TRACK_OK;
        if (my_status == TRACK_OK) {
            const double p[3] = {(double)com3d[my_m * 3], (double)com3d[my_m * 3 + 1], (double)com3d[my_m * 3 + 2]};
            double w[3];
            to_world(extr + (size_t)my_c * 12, p, w);
            for (int d = 0; d < 3; ++d) s_w[tid][d] = w[d];
        }
    }
    __syncthreads();
    if (tid == 0) {                                                    // what needs all members at once: LDS only from here on
        int nc = 0;
        for (int k = 0; k < K; ++k) nc += s_use[k];
        if (max_dev > 0.0 && nc >= 3) {                                // the componentwise median; all outliers decided at once
            double med[3];
            for (int d = 0; d < 3; ++d) {
                int n = 0;
                for (int k = 0; k < K; ++k) {
                    if (!s_use[k]) continue;
                    const double v = s_w[k][d];
                    int i = n++;
                    for (; i > 0 && s_sort[i - 1] > v; --i) s_sort[i] = s_sort[i - 1];
                    s_sort[i] = v;
                }
                med[d] = (n & 1) ? s_sort[n >> 1] : (s_sort[(n >> 1) - 1] + s_sort[n >> 1]) / 2.0;
            }
            for (int k = 0; k < K; ++k) {
                if (!s_use[k]) continue;
                const double w[3] = {s_w[k][0], s_w[k][1], s_w[k][2]};
                if (dist3(w, med) > max_dev) s_bits[k] |= DPP_FUSE_OUTLIER;
            }
            for (int k = 0; k < K; ++k) {
                if (s_bits[k] & DPP_FUSE_OUTLIER) s_use[k] = 0;
            }
        } else if (max_dev > 0.0 && nc == 2) {                         // two that disagree: nobody can say who is wrong
            int a = -1, b = -1;
            for (int k = 0; k < K; ++k) {
                if (s_use[k]) { if (a < 0) a = k; else b = k; }
            }
            const double wa[3] = {s_w[a][0], s_w[a][1], s_w[a][2]}, wb[3] = {s_w[b][0], s_w[b][1], s_w[b][2]};
            if (dist3(wa, wb) > max_dev) { s_bits[a] |= DPP_FUSE_DISAGREE; s_bits[b] |= DPP_FUSE_DISAGREE; }
        }
        double sum[3] = {0.0, 0.0, 0.0};
        int n = 0;
        for (int k = 0; k < K; ++k) {
            if (!s_use[k]) continue;
            for (int d = 0; d < 3; ++d) sum[d] = sum[d] + s_w[k][d];
            ++n;
        }
        s_n = n;
        n_out[g] = n;
        for (int d = 0; d < 3; ++d) fused_com[g * 3 + d] = n ? (float)(sum[d] / (double)n) : 0.0f;
    }
    __syncthreads();
    // the peer centre of every member: the mean world centre of the inliers other than itself, through its own camera
    if (tid < K) {
        const int k = tid, m = my_m, c = my_c;
        double ps[3] = {0.0, 0.0, 0.0};
        int np = 0;
        for (int q = 0; q < K; ++q) {
            if (q == k || !s_use[q]) continue;
            for (int d = 0; d < 3; ++d) ps[d] = ps[d] + s_w[q][d];
            ++np;
        }
        float pc[3] = {0.0f, 0.0f, 0.0f};
        bool ok = false;
        if (np > 0) {
            const double w[3] = {ps[0] / (double)np, ps[1] / (double)np, ps[2] / (double)np};
            double p[3];
            to_camera(extr + (size_t)c * 12, w, p);
            const float pf[3] = {(float)p[0], (float)p[1], (float)p[2]};
            AugCam cam = cam0;
            source_camera(tab, c, cam);
            int Hc = H, Wc = W;
            if (tab) { Hc = tab[c].H; Wc = tab[c].W; }
            toimg(cam, (double)pf[0], (double)pf[1], (double)pf[2], true, pc);
            ok = pc[2] > 0.0f && !com_ill_defined(pc) && pc[0] >= 0.0f && (double)pc[0] < (double)Wc && pc[1] >= 0.0f &&
                 (double)pc[1] < (double)Hc;
        }
        for (int d = 0; d < 3; ++d) peer_com[m * 3 + d] = pc[d];
        int f = s_bits[k] | (s_use[k] ? DPP_FUSE_USED : 0) | (ok ? DPP_FUSE_PEER_OK : 0);
        // hand-over: a member that lost the hand in this tick, or that sits on something else, goes on from its peers' centre
        if ((flags & DPP_FUSE_HANDOVER) && ok && (my_status == TRACK_LOST || (f & DPP_FUSE_OUTLIER))) {
            for (int d = 0; d < 3; ++d) com[m * 3 + d] = pc[d];
            f |= DPP_FUSE_HANDED;
        }
        fstat[m] = f;
    }
    const int n = s_n;
    for (int j = tid; j < J; j += DPP_WAVE) {
        double sum[3] = {0.0, 0.0, 0.0}, wsum[3] = {0.0, 0.0, 0.0}, sw = 0.0;
        float wmax = 0.0f;
        for (int k = 0; k < K; ++k) {
            if (!s_use[k]) continue;
            const int m = mem[k];
            const float* q = pose3d + ((size_t)m * J + j) * 3;
            const double p[3] = {(double)q[0], (double)q[1], (double)q[2]};
            double w[3];
            to_world(extr + (size_t)src[m] * 12, p, w);
            for (int d = 0; d < 3; ++d) sum[d] = sum[d] + w[d];
            if (weight) {                                                      // a product, then an add: the unit has no FMA contraction
                const float wm = weight[(size_t)m * J + j];
                sw = sw + (double)wm;
                for (int d = 0; d < 3; ++d) wsum[d] = wsum[d] + (double)wm * w[d];
                if (wm > wmax) wmax = wm;
            }
        }
        const bool weighted = weight && sw > 0.0;                              // somebody sees the joint; else: the plain mean, as without weights
        double mean[3] = {0.0, 0.0, 0.0}, worst = 0.0;
        if (n) {
            for (int d = 0; d < 3; ++d) mean[d] = weighted ? wsum[d] / sw : sum[d] / (double)n;
            for (int k = 0; k < K; ++k) {                                      // (the world joints again: cheaper than keeping K x J of them)
                if (!s_use[k]) continue;
                const int m = mem[k];
                if (weighted && !(weight[(size_t)m * J + j] > 0.0f)) continue;  // the spread of those that took part
                const float* q = pose3d + ((size_t)m * J + j) * 3;
                const double p[3] = {(double)q[0], (double)q[1], (double)q[2]};
                double w[3];
                to_world(extr + (size_t)src[m] * 12, p, w);
                const double r = dist3(w, mean);
                if (r > worst) worst = r;
            }
        }
        float* fp = fused_pose + ((size_t)g * J + j) * 3;
        for (int d = 0; d < 3; ++d) fp[d] = (float)mean[d];
        spread[(size_t)g * J + j] = (float)worst;
        if (weight) fused_weight[(size_t)g * J + j] = (n && weighted) ? wmax : 0.0f;
    }
}

}  // namespace

// The argument checks and the one launch of both entry points.  weight == nullptr: dpp_pose_fuse, whose bytes the weighted form leaves alone.
static int launch_pose_fuse(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* extrinsics,
                            int C, const int* members, const int* offsets, int G, const void* sources, int H, int W, double fx, double fy,
                            double ux, double uy, int flip_y, double max_dev, int flags, float* com, float* fused_pose, float* fused_com,
                            float* spread, int* n_out, float* peer_com, int* fstat, const float* weight, float* fused_weight,
                            dpp_stream_t stream) {
    if (!pose3d || !com3d || !status || !src || !extrinsics || !members || !offsets || !com || !fused_pose || !fused_com || !spread || !n_out ||
        !peer_com || !fstat)
        return DPP_E_BADARG;
    if (T < 1 || J < 1 || C < 1 || G < 1 || G > T || (flags & ~DPP_FUSE_HANDOVER) || !(max_dev >= 0.0) || !(max_dev <= 1.7e308)) return DPP_E_BADARG;
    if (!sources && (H < 1 || W < 1 || fx == 0.0 || fy == 0.0)) return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    DPP_LAUNCH(pose_fuse_kernel, dim3(G), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), pose3d, com3d, status, src, J, extrinsics, members,
               offsets, static_cast<const SourceRec*>(sources), H, W, cam, max_dev, flags, com, fused_pose, fused_com, spread, n_out, peer_com,
               fstat, weight, fused_weight);
    return dpp_launch_status();
}

extern "C" int dpp_pose_fuse(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* extrinsics,
                             int C, const int* members, const int* offsets, int G, const void* sources, int H, int W, double fx, double fy,
                             double ux, double uy, int flip_y, double max_dev, int flags, float* com, float* fused_pose, float* fused_com,
                             float* spread, int* n_out, float* peer_com, int* fstat, dpp_stream_t stream) {
    return launch_pose_fuse(pose3d, com3d, status, src, T, J, extrinsics, C, members, offsets, G, sources, H, W, fx, fy, ux, uy, flip_y, max_dev,
                            flags, com, fused_pose, fused_com, spread, n_out, peer_com, fstat, nullptr, nullptr, stream);
}

// ABI v23: the same with a weight per track and joint (dpp_joint_visibility's), and the largest weight that went into each fused joint
extern "C" int dpp_pose_fuse_w(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* extrinsics,
                               int C, const int* members, const int* offsets, int G, const void* sources, int H, int W, double fx, double fy,
                               double ux, double uy, int flip_y, double max_dev, int flags, float* com, float* fused_pose, float* fused_com,
                               float* spread, int* n_out, float* peer_com, int* fstat, const float* weight, float* fused_weight,
                               dpp_stream_t stream) {
    if (!weight || !fused_weight) return DPP_E_BADARG;
    return launch_pose_fuse(pose3d, com3d, status, src, T, J, extrinsics, C, members, offsets, G, sources, H, W, fx, fy, ux, uy, flip_y, max_dev,
                            flags, com, fused_pose, fused_com, spread, n_out, peer_com, fstat, weight, fused_weight, stream);
}
