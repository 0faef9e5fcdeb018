// crop.hip -- everything that works on full depth frames and on finished crops, for gfx950:
//   the initial crop        crop_prepare / crop_com / crop_warp / crop_refine (HandDetector.cropArea3D + Dataset.imgStackDepthOnly)
//   the crop helpers        crop_warp_ex, resize_crops, recrop, inverse_crop (bilinearResize, resizeCrop, recropHand, getInverseCrop,
//                           applyCrop3D; ABI v12)
//   realtime tracking       frame_range, crop_prepare_ranged, track_refine, pose_finish, refine_com_iterative (HandDetector.track,
//                           RealtimeHandposePipeline; ABI v13)
//   several tracks          the *_ix entry points of the five tracking launches: T tracks over C frames (ABI v16)
//   several hands           refine_com_iterative_ix: several centres of one frame refined in one launch (ABI v17)
//   unlike sources          the *_src entry points: every frame source with its own camera and frame size (ABI v19)
// They share CropRec, crop_geometry and crop_window_value; each section below names the reference lines it restates.  The training-time
// augmentation of finished crops is augment.hip; finding the hand in a whole frame (connected components) is components.hip; the
// camera, bounds and warp-coordinate arithmetic and the workgroup reductions these units share are geom.h.
// Compiled with -ffp-contract=off like augment.hip: the reference's NumPy/OpenCV arithmetic rounds after every operation, so no fused
// multiply-add may be formed here (pixel coordinates at rounding boundaries would move).
#include "geom.h"
#include "crop_rec.h"

namespace {

// ---- initial crop: HandDetector.cropArea3D (docom = False) + Dataset.imgStackDepthOnly ------------------------------
// /root/reference/src/util/handdetector.py:53-68 (depth range of the detector), :204-226 (comToBounds), :260-296 (getCrop),
// :382-490 (cropArea3D), cv2.resize INTER_NEAREST (OpenCV 2.4 resizeNN), /root/reference/src/data/dataset.py:97-103.
// Two launches per batch of full depth frames, like the augmentation: crop_prepare (one workgroup per frame: min / max of
// the frame -> the detector's valid depth range, then lane 0 does the bounds / resize geometry in f64) and crop_warp (one
// thread per output pixel: gather through the nearest-neighbour resize map, range clamp, z-threshold, background,
// optional normalisation to [-1, 1]).
// (CropRec itself: crop_rec.h, shared with background.hip, which reads a track's window.)

// The crop geometry of one frame from its depth range (mn, mx) and centre c: the detector's valid range, the window of the metric
// cube, the resized size / paste offset and the crop transform M (9 floats, may be null).  Shared by crop_prepare_kernel (range from
// its own pass over the frame) and the realtime kernels below (range from frame_range_kernel's partials): one body, so their records
// are byte-identical.  The clamp of the range is idempotent: a record's own (min_depth, max_depth) may be passed back in.
__device__ __forceinline__ void crop_geometry(float mn, float mx, const float c[3], const float* __restrict__ cube_b, double fx, double fy,
                                              int dsz, int stretch, CropRec& r, float* __restrict__ M) {
    r.max_depth = fminf(1500.0f, mx);                          // handdetector.py:60-61
    r.min_depth = fmaxf(10.0f, mn);
    const double size[3] = {(double)cube_b[0], (double)cube_b[1], (double)cube_b[2]};
    int bd[4];
    const double cd[3] = {c[0], c[1], c[2]};
    com_to_bounds(cd, size, fx, fy, bd);
    r.xstart = bd[0]; r.ystart = bd[2];
    const int wb = bd[1] - bd[0], hb = bd[3] - bd[2];
    r.cw = wb; r.ch = hb;
    r.zstart = (float)((double)c[2] - size[2] / 2.);
    r.zend = (float)((double)c[2] + size[2] / 2.);
    long long sz0, sz1;                                         // (width, height) of the resized crop
    if (wb > hb) { sz0 = dsz; sz1 = floordiv((long long)hb * dsz, wb); }
    else { sz0 = floordiv((long long)wb * dsz, hb); sz1 = dsz; }
    if (stretch) { sz0 = dsz; sz1 = dsz; }                      // resizeCrop(cropped, dsize): the refinement net's input, handdetector.py:430
    r.szw = (int)sz0; r.szh = (int)sz1;
    const double sc = (hb > wb) ? (double)sz1 / (double)hb : (double)sz0 / (double)wb;     // cropped.shape = (hb, wb)
    r.ifx = 1. / ((double)sz0 / (double)wb);
    r.ify = 1. / ((double)sz1 / (double)hb);
    r.xs = (int)floor(dsz / 2. - (double)sz0 / 2.);
    r.ys = (int)floor(dsz / 2. - (double)sz1 / 2.);
    r.far_v = c[2] + (float)(size[2] / 2.);
    r.norm_off = c[2];
    r.norm_div = (float)(size[2] / 2.);
    if (M) {
        M[0] = (float)sc; M[1] = 0.f; M[2] = (float)(sc * (double)(-bd[0]) + (double)r.xs);
        M[3] = 0.f; M[4] = (float)sc; M[5] = (float)(sc * (double)(-bd[2]) + (double)r.ys);
        M[6] = 0.f; M[7] = 0.f; M[8] = 1.f;
    }
}

__global__ __launch_bounds__(DPP_THREADS) void crop_prepare_kernel(const float* __restrict__ frames, int H, int W,
                                                                   const float* __restrict__ com, const float* __restrict__ cube,
                                                                   double fx, double fy, int dsz, int stretch,
                                                                   CropRec* __restrict__ rec, float* __restrict__ M_out) {
    __shared__ float s_mn[DPP_THREADS / DPP_WAVE], s_mx[DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* f = frames + (size_t)b * H * W;
    float mn = 3.4e38f, mx = -3.4e38f;
    const int npx = H * W;
    int i0 = 0;
    if ((npx & 3) == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0) {          // 16-byte loads, 4 independent chains
        const float4* f4 = reinterpret_cast<const float4*>(f);
        const int n4 = npx >> 2;
        float4 lo = make_float4(mn, mn, mn, mn), hi = make_float4(mx, mx, mx, mx);
#pragma unroll 4
        for (int i = tid; i < n4; i += DPP_THREADS) {
            float4 v = f4[i];
            lo.x = fminf(lo.x, v.x); lo.y = fminf(lo.y, v.y); lo.z = fminf(lo.z, v.z); lo.w = fminf(lo.w, v.w);
            hi.x = fmaxf(hi.x, v.x); hi.y = fmaxf(hi.y, v.y); hi.z = fmaxf(hi.z, v.z); hi.w = fmaxf(hi.w, v.w);
        }
        mn = fminf(fminf(lo.x, lo.y), fminf(lo.z, lo.w));
        mx = fmaxf(fmaxf(hi.x, hi.y), fmaxf(hi.z, hi.w));
        i0 = npx;
    }
    for (int i = i0 + tid; i < npx; i += DPP_THREADS) { float v = f[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    if (!block_minmax(mn, mx, s_mn, s_mx)) return;
    CropRec r;
    const float c[3] = {com[b * 3], com[b * 3 + 1], com[b * 3 + 2]};
    crop_geometry(mn, mx, c, cube + b * 3, fx, fy, dsz, stretch, r, M_out ? M_out + (size_t)b * 9 : nullptr);
    rec[b] = r;
}

// ---- several tracks (ABI v16) -----------------------------------------------------------------------------------------------
// The tracking launches serve T tracks over C frames: row t of com / cube / records / net outputs is track t, which reads frame
// src[t] (and that frame's depth-range partials), sits a tick out where gate[t] == 0 and has its own POSE_* bits in tflags[t].
// The arrays are null in the plain entry points (row b reads frame b, nothing is gated, the flags are a launch argument), so both
// forms run the same bodies.  The host has checked 0 <= src[t] < C.
constexpr int POSE_HAND_RIGHT = 1, POSE_INV_X = 2, POSE_INV_Y = 4;     // dpp_pose_finish flags
constexpr int TRACK_OK = 0, TRACK_LOST = 1, TRACK_IDLE = 2;           // dpp_track_refine status

__device__ __forceinline__ int track_source(const int* __restrict__ src, int b) { return src ? src[b] : b; }
__device__ __forceinline__ bool track_gated(const int* __restrict__ gate, int b) { return gate && gate[b] == 0; }

constexpr int CW_NORMALIZE = 1, CW_BILINEAR = 2, CW_NO_RANGE = 4, CW_NO_THRESH = 8, CW_FLIP_X = 16;     // dpp_crop_warp_ex flags

// value of getCrop's window at window coordinates (sx, sy): zero padding outside the frame, the detector's valid depth
// range, then the z-threshold (handdetector.py:260-296).  applyCrop3D's options: `pad` outside the frame (getCrop's `background`),
// CW_NO_RANGE / CW_NO_THRESH switch the range test / the z-threshold off; the plain callers pass the literals (0, 0.0f), so their
// flag tests fold at compile time.
__device__ __forceinline__ float crop_window_value(const float* __restrict__ frame, int H, int W, const CropRec& r, long long sx, long long sy,
                                                   int flags, float pad) {
    const long long gx = r.xstart + sx, gy = r.ystart + sy;
    float v = pad;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
        v = frame[(size_t)gy * W + gx];
        if (!(flags & CW_NO_RANGE) && (v > r.max_depth || v < r.min_depth)) v = 0.0f;
    }
    if (!(flags & CW_NO_THRESH)) v = z_threshold(v, r.zstart, r.zend);
    return v;
}

// cv2 2.4 resizeNN: source index of destination index x of an n-wide source, min(floor(x * ifx), n - 1)
__device__ __forceinline__ long long resize_nn_index(int x, double ifx, int n) {
    const long long s = (long long)floor((double)x * ifx);
    return s > n - 1 ? n - 1 : s;
}

constexpr int COM_BANDS = 16;           // row bands of a crop window, one workgroup each

// calculateCoM's sums over window rows [y0, y1) x columns [x0, x1) of r: this thread's share of (sum x, sum y, sum depth, count) of the
// valid pixels in f64.  A wave walks whole rows (lane = column), so there is no division per pixel and a row's loads are contiguous.
__device__ __forceinline__ void com_window_sums(const float* __restrict__ f, int H, int W, const CropRec& r, int x0, int x1, int y0, int y1,
                                                double& sx, double& sy, double& sd, double& cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sx = 0.0; sy = 0.0; sd = 0.0; cnt = 0.0;
    for (int y = y0 + wave; y < y1; y += DPP_THREADS / DPP_WAVE) {
        double rs = 0.0, rc = 0.0, rx = 0.0;
        for (int x = x0 + lane; x < x1; x += DPP_WAVE) {
            float v = crop_window_value(f, H, W, r, x, y, 0, 0.0f);
            if (v < r.min_depth || v > r.max_depth) v = 0.0f;       // calculateCoM's own range test
            if (v > 0.0f) { rx += x; rs += (double)v; rc += 1.0; }
        }
        sx += rx; sd += rs; cnt += rc; sy += rc * (double)y;
    }
}

// One band of window rows: its sums -> partial[b][band][4].
__global__ __launch_bounds__(DPP_THREADS) void crop_com_partial_kernel(const float* __restrict__ frames, int H, int W,
                                                                       const CropRec* __restrict__ rec, double* __restrict__ partial) {
    __shared__ double s_red[4][DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.y, band = blockIdx.x;
    const CropRec r = rec[b];
    const int rows = (r.ch + COM_BANDS - 1) / COM_BANDS;
    const int y0 = band * rows, y1 = (y0 + rows < r.ch) ? y0 + rows : r.ch;
    double sx, sy, sd, cnt;
    com_window_sums(frames + (size_t)b * H * W, H, W, r, 0, r.cw, y0, y1, sx, sy, sd, cnt);
    if (!com_block_sums(sx, sy, sd, cnt, s_red)) return;
    double* out = partial + ((size_t)b * COM_BANDS + band) * 4;
    out[0] = sx; out[1] = sy; out[2] = sd; out[3] = cnt;
}

// calculateCoM of the crop window (handdetector.py:91-108, as called by cropArea3D with docom=True, :413-421): mean
// column, mean row and mean depth of the pixels inside the detector's range, moved back to frame coordinates; an empty
// window falls back to the depth of its centre pixel, then to 300 mm.  One thread per frame sums the bands in order.
__global__ __launch_bounds__(DPP_THREADS) void crop_com_finish_kernel(const float* __restrict__ frames, int B, int H, int W,
                                                                      const CropRec* __restrict__ rec, const double* __restrict__ partial,
                                                                      float* __restrict__ com_out) {
    const int b = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (b >= B) return;
    const CropRec r = rec[b];
    const float* f = frames + (size_t)b * H * W;
    double sx = 0.0, sy = 0.0, sd = 0.0, cnt = 0.0;
    for (int k = 0; k < COM_BANDS; ++k) {
        const double* p = partial + ((size_t)b * COM_BANDS + k) * 4;
        sx += p[0]; sy += p[1]; sd += p[2]; cnt += p[3];
    }
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (cnt > 0.0) { c0 = sx / cnt; c1 = sy / cnt; c2 = sd / cnt; }
    if (fabs(c0) <= 1e-8 && fabs(c1) <= 1e-8 && fabs(c2) <= 1e-8) {       // numpy.allclose(com, 0.)
        c2 = (double)crop_window_value(f, H, W, r, r.cw / 2, r.ch / 2, 0, 0.0f);
        if (fabs(c2) <= 1e-8) c2 = 300.0;
    }
    com_out[b * 3 + 0] = (float)(c0 + (double)r.xstart);
    com_out[b * 3 + 1] = (float)(c1 + (double)r.ystart);
    com_out[b * 3 + 2] = (float)c2;
}

// The centre update of cropArea3D's refinement step and of HandDetector.track, frame b's slices of com / net_out / cube passed in:
//   newCom3D = net_out * (cube_z / 2) + jointImgTo3D(com);  com' = joint3DToImg(newCom3D);
//   allclose(com', 0) -> com'_z = centre pixel of the crop window r
// -> c2 = com'.  Reads only (com may be the buffer the caller then writes c2 to).
__device__ __forceinline__ void refined_centre(const AugCam& cam, const float* com, const float* __restrict__ net_out, const float* __restrict__ cube,
                                               const float* __restrict__ frame, int H, int W, const CropRec& r, float c2[3]) {
    const float half = (float)((double)cube[2] / 2.);              // size[2] / 2. as a floatX constant
    float c3[3], n3[3];
    to3d(cam, com[0], com[1], com[2], c3);
    for (int d = 0; d < 3; ++d) n3[d] = net_out[d] * half + c3[d];   // float32 arrays: two roundings
    toimg(cam, n3[0], n3[1], n3[2], true, c2);
    if (fabs((double)c2[0]) <= 1e-8 && fabs((double)c2[1]) <= 1e-8 && fabs((double)c2[2]) <= 1e-8)
        c2[2] = crop_window_value(frame, H, W, r, r.cw / 2, r.ch / 2, 0, 0.0f);
}

// The CoM-refinement step of cropArea3D(docom=True) with a refineNet (handdetector.py:429-440, refineCoM :634-676), batched:
//   newCom3D = net_out * (cube_z / 2) + jointImgTo3D(com);  com' = joint3DToImg(newCom3D);
//   allclose(com', 0) -> com'_z = centre pixel of the (re-centred) crop window
// one workgroup per frame.  With gt3d_orig it also forms what the importers keep per frame for the NEXT crop (importers.py:388-392,
// dataset.py:103): gt3Dcrop = gt3Dorig - jointImgTo3D(com') and the training label gt3Dcrop / (cube_z / 2), optionally projected
// onto the PCA prior (poseregnettrainer.py:262) -- so that a refine -> re-crop -> regress cascade needs no host step.
__global__ __launch_bounds__(DPP_THREADS) void crop_refine_kernel(const float* __restrict__ frames, int H, int W,
                                                                  const CropRec* __restrict__ rec, const float* __restrict__ com_in,
                                                                  const float* __restrict__ cube, const float* __restrict__ net_out,
                                                                  AugCam cam, const float* __restrict__ gt3d_orig, int J,
                                                                  const float* __restrict__ pca_mean, const float* __restrict__ pca_comp,
                                                                  int E, float* __restrict__ com_out, float* __restrict__ com3d_out,
                                                                  float* __restrict__ gt3d_crop, float* __restrict__ out_y) {
    __shared__ float s_c3[3];
    __shared__ float s_label[MAXJ3];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        float c2[3];
        refined_centre(cam, com_in + b * 3, net_out + b * 3, cube + b * 3, frames + (size_t)b * H * W, H, W, rec[b], c2);
        for (int d = 0; d < 3; ++d) com_out[b * 3 + d] = c2[d];
        float q3[3];
        to3d(cam, c2[0], c2[1], c2[2], q3);
        for (int d = 0; d < 3; ++d) { s_c3[d] = q3[d]; if (com3d_out) com3d_out[b * 3 + d] = q3[d]; }
    }
    if (gt3d_orig == nullptr) return;
    __syncthreads();
    const float half = (float)((double)cube[b * 3 + 2] / 2.);
    for (int i = tid; i < J * 3; i += DPP_THREADS) {
        const float g = gt3d_orig[(size_t)b * J * 3 + i] - s_c3[i % 3];
        if (gt3d_crop) gt3d_crop[(size_t)b * J * 3 + i] = g;
        s_label[i] = g / half;
    }
    __syncthreads();
    if (out_y == nullptr) return;
    const int D = J * 3;
    if (pca_comp) {
        for (int e = tid; e < E; e += DPP_THREADS) {
            double s = 0.0;
            for (int d = 0; d < D; ++d) s += ((double)s_label[d] - (double)pca_mean[d]) * (double)pca_comp[(size_t)e * D + d];
            out_y[(size_t)b * E + e] = (float)s;
        }
    } else {
        for (int d = tid; d < D; d += DPP_THREADS) out_y[(size_t)b * D + d] = s_label[d];
    }
}

// ---- HandDetector crop helpers (ABI v12): bilinearResize, resizeCrop, recropHand, getInverseCrop, applyCrop3D ----------
// /root/reference/src/util/handdetector.py:132-202 (bilinearResize), :298-351 (getInverseCrop, resizeCrop), :353-380 (applyCrop3D),
// :782-803 (recropHand).  One launch per batch, one thread per output pixel.
struct PlaneSrc {              // a dense [sh][sw] crop as a bilinearResize source
    const float* s;
    int sw;
    __device__ __forceinline__ float operator()(int x, int y) const { return s[(size_t)y * sw + x]; }
};

struct WindowSrc {             // getCrop's window of one frame as a bilinearResize source
    const float* f;
    int H, W, flags;
    float pad;
    const CropRec* r;
    __device__ __forceinline__ float operator()(int x, int y) const { return crop_window_value(f, H, W, *r, x, y, flags, pad); }
};

// HandDetector.bilinearResize (handdetector.py:132-202) at destination pixel (col, row) of an sw x sh -> dw x dh resize: the
// reference's arithmetic step for step.  It ran on NumPy 1, where a float32 element times a Python float is a float64, so the
// weights and the weighted sum are f64 (no contraction: -ffp-contract=off), rounded once to f32.  More than two of the four taps
// equal to `nd` -> nd; a tap equal to nd loses its weight, the reference's re-balancing in its order; weights scaled by
// 1 / sum; all weights zero -> nd.  The host refuses sources narrower or shorter than 2 pixels (the reference's "Shape mismatch");
// the clamp of x + 1 / y + 1 only keeps every read inside the source.
template <class Src>
__device__ __forceinline__ float bilinear_nd(const Src& src, int sw, int sh, int dw, int dh, int col, int row, float nd) {
    const double x_ratio = (double)(sw - 1) / (double)dw, y_ratio = (double)(sh - 1) / (double)dh;
    const double fy = (double)row * y_ratio, fx = (double)col * x_ratio;
    const int y = (int)fy, x = (int)fx;
    const double y_diff = fy - (double)y, y_diff_2 = 1. - y_diff;
    const double x_diff = fx - (double)x, x_diff_2 = 1. - x_diff;
    double y2x2 = y_diff_2 * x_diff_2, y2x = y_diff_2 * x_diff, yx2 = y_diff * x_diff_2, yx = y_diff * x_diff;
    const int x1 = x + 1 < sw ? x + 1 : sw - 1, y1 = y + 1 < sh ? y + 1 : sh - 1;
    const float a = src(x, y), b = src(x1, y), c = src(x, y1), d = src(x1, y1);
    const bool na = a == nd, nb = b == nd, nc = c == nd, nd4 = d == nd;
    if ((int)na + (int)nb + (int)nc + (int)nd4 > 2) return nd;
    if (na) { y2x2 = 0.; y2x = 1. - yx - yx2; }
    if (nb) { y2x = 0.; if (y2x2 != 0.) y2x2 = 1. - yx - yx2; }
    if (nc) { yx2 = 0.; yx = 1. - y2x - y2x2; }
    if (nd4) { yx = 0.; if (yx2 != 0.) yx2 = 1. - y2x - y2x2; }
    if (!(y2x2 == 0. && y2x == 0. && yx2 == 0. && yx == 0.)) {
        const double sc = 1. / (yx + yx2 + y2x + y2x2);
        y2x2 *= sc; y2x *= sc; yx2 *= sc; yx *= sc;
    }
    if (y2x2 == 0. && y2x == 0. && yx2 == 0. && yx == 0.) return nd;
    return (float)(y2x2 * (double)a + y2x * (double)b + yx2 * (double)c + yx * (double)d);
}

// One output pixel of the crop warp: gather through the resize map, range clamp, z-threshold, fill outside the paste, optional
// normalisation to [-1, 1] (dataset.py:98-100) -- with the options of the reference's other callers of the window resize: bilinear mode
// (cropArea3D / applyCrop3D with resizeMethod = RESIZE_BILINEAR), no detector range test (applyCrop3D crops an arbitrary image),
// z-threshold off, getCrop's pad value and a fill value outside the paste of their own.  Inlined into both entry points below.
// src (null: row b reads frame b): the frame of row b, see "several tracks" below.
__device__ __forceinline__ void crop_warp_body(const float* __restrict__ frames, int H, int W, const CropRec* __restrict__ rec, int dsz, int flags,
                                               float nd_value, float fill_value, float pad_value, const int* __restrict__ src,
                                               const SourceRec* __restrict__ tab, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (p >= dsz * dsz) return;
    const CropRec r = rec[b];
    const float* f = source_frame(frames, tab, track_source(src, b), H, W);
    const int y = p / dsz, xo = p - y * dsz;
    const int x = (flags & CW_FLIP_X) ? dsz - 1 - xo : xo;      // crop[:, ::-1]: output column xo holds column dsz - 1 - xo
    float v = fill_value;
    const int rx = x - r.xs, ry = y - r.ys;
    if (rx >= 0 && rx < r.szw && ry >= 0 && ry < r.szh) {
        if (flags & CW_BILINEAR) {
            const WindowSrc src{f, H, W, flags, pad_value, &r};
            v = bilinear_nd(src, r.cw, r.ch, r.szw, r.szh, rx, ry, nd_value);
        } else {
            v = crop_window_value(f, H, W, r, resize_nn_index(rx, r.ifx, r.cw), resize_nn_index(ry, r.ify, r.ch), flags, pad_value);
        }
    }
    if (flags & CW_NORMALIZE) {
        if (v == 0.0f) v = r.far_v;                              // dataset.py:98-100
        v = (v - r.norm_off) / r.norm_div;
    }
    out[(size_t)b * dsz * dsz + p] = v;
}

// The training path's crop_frames: nearest neighbour, range test and z-threshold on, nd_value outside the paste.  Its flags are
// compile-time constants apart from the normalise bit, so the bilinear, flip and no-range branches of the body are compiled out.
__global__ __launch_bounds__(DPP_THREADS) void crop_warp_kernel(const float* __restrict__ frames, int H, int W, const CropRec* __restrict__ rec,
                                                                int dsz, int normalize, float nd_value, const int* __restrict__ src,
                                                                const SourceRec* __restrict__ tab, float* __restrict__ out) {
    crop_warp_body(frames, H, W, rec, dsz, normalize ? CW_NORMALIZE : 0, nd_value, nd_value, 0.0f, src, tab, out);
}

__global__ __launch_bounds__(DPP_THREADS) void crop_warp_ex_kernel(const float* __restrict__ frames, int H, int W, const CropRec* __restrict__ rec,
                                                                   int dsz, int flags, float nd_value, float fill_value, float pad_value,
                                                                   const int* __restrict__ src, const int* __restrict__ tflags,
                                                                   const SourceRec* __restrict__ tab, float* __restrict__ out) {
    if (tflags && (tflags[blockIdx.y] & POSE_HAND_RIGHT)) flags |= CW_FLIP_X;      // the row's own hand side
    crop_warp_body(frames, H, W, rec, dsz, flags, nd_value, fill_value, pad_value, src, tab, out);
}

// resizeCrop on B same-size crops: cv2 2.4 resizeNN (source index min(floor(x * ifx), sw - 1)) or bilinearResize
__global__ __launch_bounds__(DPP_THREADS) void resize_crops_kernel(const float* __restrict__ src, int sh, int sw, int dh, int dw, int bilinear,
                                                                   float nd_value, double ifx, double ify, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (p >= dh * dw) return;
    const float* s = src + (size_t)b * sh * sw;
    const int y = p / dw, x = p - y * dw;
    float v;
    if (bilinear) {
        v = bilinear_nd(PlaneSrc{s, sw}, sw, sh, dw, dh, x, y, nd_value);
    } else {
        v = s[(size_t)resize_nn_index(y, ify, sh) * sw + resize_nn_index(x, ifx, sw)];
    }
    out[(size_t)b * dh * dw + p] = v;
}

// recropHand (handdetector.py:782-803) on B crops in mm: cv2.warpPerspective(crop, dot(M, Mnew), (tw, th), INTER_NEAREST,
// BORDER_CONSTANT background) -- the product and cofactor inverse of the augmentation (mat3_mul, mat3_inv), formed once per
// workgroup, and the 64-wide-block coordinates of the augmentation's perspective warp (persp_source, always dividing) --, then
// isclose(warped, nv_val) -> background (is_close) and the z-threshold against the f32 zrange[b] = (zstart, zend).
__global__ __launch_bounds__(DPP_THREADS) void recrop_kernel(const float* __restrict__ crops, int h, int w, const double* __restrict__ M,
                                                             const double* __restrict__ Mnew, int th, int tw, float background, double nv_val,
                                                             int thresh, const float* __restrict__ zrange, float* __restrict__ out) {
    __shared__ double s_m[9];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        double A[9], Bm[9], P[9], T[9];
        for (int i = 0; i < 9; ++i) { A[i] = M[(size_t)b * 9 + i]; Bm[i] = Mnew[(size_t)b * 9 + i]; }
        mat3_mul(A, Bm, P);
        mat3_inv(P, T);
        for (int i = 0; i < 9; ++i) s_m[i] = T[i];
    }
    __syncthreads();
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (p >= th * tw) return;
    double m[9];
    for (int i = 0; i < 9; ++i) m[i] = s_m[i];
    const int y = p / tw, x = p - y * tw;
    long long X, Y;
    persp_source(m, (x >> 6) << 6, x, y, true, X, Y);
    float v = background;
    if (X >= 0 && X < w && Y >= 0 && Y < h) v = crops[(size_t)b * h * w + (size_t)Y * w + (size_t)X];
    if (is_close(v, nv_val)) v = background;
    if (thresh) v = z_threshold(v, zrange[b * 2], zrange[b * 2 + 1]);
    out[(size_t)b * th * tw + p] = v;
}

// getInverseCrop (handdetector.py:298-334): crop b resized to its window bounds[b] = (xstart, xend, ystart, yend) and pasted into an
// H x W canvas of `background`, then the z-threshold over the whole frame.  The reference's three early returns (window entirely
// left / above, entirely right / below, zero width or height) leave the bare canvas, z-threshold included.
__global__ __launch_bounds__(DPP_THREADS) void inverse_crop_kernel(const float* __restrict__ crops, int ch, int cw, const int* __restrict__ bounds,
                                                                   const float* __restrict__ zrange, int H, int W, int bilinear, float nd_value,
                                                                   float background, int thresh, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const int xs = bounds[b * 4], xe = bounds[b * 4 + 1], ys = bounds[b * 4 + 2], ye = bounds[b * 4 + 3];
    const int gy = p / W, gx = p - gy * W;
    float v = background;
    const bool early = (xe < 0 && xs < 0) || (ye < 0 && ys < 0) || (xe > W && xs > W) || (ye > H && ys > H) || xe == xs || ye == ys;
    if (!early) {
        if (gx >= (xs > 0 ? xs : 0) && gx < (xe < W ? xe : W) && gy >= (ys > 0 ? ys : 0) && gy < (ye < H ? ye : H)) {
            const float* s = crops + (size_t)b * ch * cw;
            const int dw = xe - xs, dh = ye - ys, col = gx - xs, row = gy - ys;
            if (bilinear) {
                v = bilinear_nd(PlaneSrc{s, cw}, cw, ch, dw, dh, col, row, nd_value);
            } else {
                const double ifx = 1. / ((double)dw / (double)cw), ify = 1. / ((double)dh / (double)ch);
                v = s[(size_t)resize_nn_index(row, ify, ch) * cw + resize_nn_index(col, ifx, cw)];
            }
        }
        if (thresh) v = z_threshold(v, zrange[b * 2], zrange[b * 2 + 1]);
    }
    out[(size_t)b * H * W + p] = v;
}

// ---- realtime tracking (ABI v13): HandDetector.track + RealtimeHandposePipeline.detect / estimatePose as device steps -----------
// /root/reference/src/util/handdetector.py:504-567, /root/reference/src/util/realtimehandposepipeline.py:296-370.  One frame is one
// chain of dependent launches, so what counts is their number and that none of them walks the frame with a single workgroup.
// min / max of frame b over FR_BANDS workgroups -> partial[b][band][2].  Interleaved 16-byte loads, four in flight per thread; a
// lane past the end re-reads its first element (harmless for min / max).  Every band writes its partial, also an empty one.
__global__ __launch_bounds__(DPP_THREADS) void frame_range_kernel(const float* __restrict__ frames, int H, int W,
                                                                  const SourceRec* __restrict__ tab, float* __restrict__ partial) {
    __shared__ float s_mn[DPP_THREADS / DPP_WAVE], s_mx[DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const float* f = source_frame(frames, tab, b, H, W);                // with a table: source b's own frame and size
    const int npx = H * W;
    const int t = band * DPP_THREADS + tid, nt = FR_BANDS * DPP_THREADS;
    float mn = 3.4e38f, mx = -3.4e38f;
    int i0 = 0;
    if ((npx & 3) == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0) {
        const float4* f4 = reinterpret_cast<const float4*>(f);
        const int n4 = npx >> 2;
        for (int i = t; i < n4; i += 4 * nt) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = i + u * nt;
                v[u] = f4[j < n4 ? j : i];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                mn = fminf(mn, fminf(fminf(v[u].x, v[u].y), fminf(v[u].z, v[u].w)));
                mx = fmaxf(mx, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
            }
        }
        i0 = npx;
    }
    for (int i = i0 + t; i < npx; i += nt) { const float v = f[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    if (!block_minmax(mn, mx, s_mn, s_mx)) return;
    partial[((size_t)b * FR_BANDS + band) * 2] = mn;
    partial[((size_t)b * FR_BANDS + band) * 2 + 1] = mx;
}

// the record of an EMPTY window: crop_warp writes its fill value everywhere (0 when normalised), nothing divides by zero; M = identity
__device__ __forceinline__ void crop_empty_record(float min_depth, float max_depth, CropRec& r, float* __restrict__ M) {
    r.xstart = 0; r.ystart = 0; r.cw = 0; r.ch = 0; r.szw = 0; r.szh = 0; r.xs = 0; r.ys = 0;
    r.ifx = 1.; r.ify = 1.;
    r.min_depth = min_depth; r.max_depth = max_depth; r.zstart = 0.f; r.zend = 0.f;
    r.far_v = 0.f; r.norm_off = 0.f; r.norm_div = 1.f;
    if (M) { for (int i = 0; i < 9; ++i) M[i] = (i % 4 == 0) ? 1.f : 0.f; }
}

// crop_prepare_kernel without its pass over the frame: one wave per frame reduces the partials, lane 0 writes the record.  An
// ill-defined centre (a lost track whose next frame is already queued) gets the empty window instead of a division by zero, and so
// does a gated track.
__global__ __launch_bounds__(DPP_WAVE) void crop_prepare_ranged_kernel(const float* __restrict__ partial, const float* __restrict__ com,
                                                                       const float* __restrict__ cube, double fx, double fy, int dsz, int stretch,
                                                                       const int* __restrict__ src, const int* __restrict__ gate,
                                                                       const SourceRec* __restrict__ tab, CropRec* __restrict__ rec,
                                                                       float* __restrict__ M_out) {
    const int b = blockIdx.x, sc = track_source(src, b);
    float mn, mx;
    frame_range_reduce(partial, sc, threadIdx.x, mn, mx);
    if (threadIdx.x != 0) return;
    if (tab) { fx = tab[sc].crop_fx; fy = tab[sc].crop_fy; }             // the source's own HandDetector focal lengths
    CropRec r;
    const float c[3] = {com[b * 3], com[b * 3 + 1], com[b * 3 + 2]};
    float* M = M_out ? M_out + (size_t)b * 9 : nullptr;
    if (com_ill_defined(c) || track_gated(gate, b)) crop_empty_record(fmaxf(10.0f, mn), fminf(1500.0f, mx), r, M);
    else crop_geometry(mn, mx, c, cube + b * 3, fx, fy, dsz, stretch, r, M);
    rec[b] = r;
}

// HandDetector.track's centre update (refined_centre, as in crop_refine_kernel) fused with the
// prepare of the final crop around the new centre (record, M, com3D) and a status word: 1 = lost, when the new centre's depth is
// numpy.isclose to 0 (comToBounds' "CoM ill-defined" branch, handdetector.py:204-213, which no device kernel implements; an all-zero
// centre is a case of it) or not finite, or when com_in already was.  A lost frame gets an EMPTY window (crop_warp then writes zeros, nothing divides by zero or
// leaves the frame), M = identity and com3D = 0.  One lane per frame does all of it, reads before writes: com_out may be com_in (the
// tracker's state buffer, updated in place -- the next reader is the next frame's first prepare, a later launch) and rec_out may be rec_in.
// A gated track is never lost: status 2 (idle), the empty window, M = identity, com3D = 0, and its centre's bits are left as they are.
__global__ __launch_bounds__(DPP_WAVE) void track_refine_kernel(const float* __restrict__ frames, int H, int W, const CropRec* rec_in,
                                                                const float* com_in, const float* __restrict__ cube,
                                                                const float* __restrict__ net_out, AugCam cam, double fx, double fy, int dsz,
                                                                const int* __restrict__ src, const int* __restrict__ gate,
                                                                const SourceRec* __restrict__ tab, float* com_out,
                                                                float* __restrict__ com3d_out, CropRec* rec_out,
                                                                float* __restrict__ M_out, int* __restrict__ status) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int c = track_source(src, b);
    const float* frame = source_frame(frames, tab, c, H, W);
    source_camera(tab, c, cam);
    if (tab) { fx = tab[c].crop_fx; fy = tab[c].crop_fy; }
    const CropRec r0 = rec_in[b];
    const bool idle = track_gated(gate, b);
    const float c1[3] = {com_in[b * 3], com_in[b * 3 + 1], com_in[b * 3 + 2]};
    float c2[3] = {c1[0], c1[1], c1[2]};                                     // a gated track keeps its centre
    if (!idle) refined_centre(cam, com_in + b * 3, net_out + b * 3, cube + b * 3, frame, H, W, r0, c2);
    const bool lost = !idle && (com_ill_defined(c2) || com_ill_defined(c1));  // (a frame queued behind a lost one stays lost)
    if (!idle || com_out != com_in) { for (int d = 0; d < 3; ++d) com_out[b * 3 + d] = c2[d]; }
    status[b] = idle ? TRACK_IDLE : lost ? TRACK_LOST : TRACK_OK;
    float* M = M_out ? M_out + (size_t)b * 9 : nullptr;
    CropRec r;
    float q3[3] = {0.f, 0.f, 0.f};
    if (lost || idle) {
        crop_empty_record(r0.min_depth, r0.max_depth, r, M);
    } else {
        crop_geometry(r0.min_depth, r0.max_depth, c2, cube + b * 3, fx, fy, dsz, 0, r, M);
        to3d(cam, c2[0], c2[1], c2[2], q3);
    }
    rec_out[b] = r;
    for (int d = 0; d < 3; ++d) com3d_out[b * 3 + d] = q3[d];
}

// RealtimeHandposePipeline.estimatePose's sign rules and its caller's pose * cube_z / 2. + com3D (realtimehandposepipeline.py:356-369,
// :198), float32 operation by operation, then importer.joints3DToImg of the result (:407).  flags: bit 0 HAND_RIGHT (column 0
// negated), bit 1 config['invX'] (column 1, as the reference has it), bit 2 config['invY'] (column 0).  One thread per joint.
__global__ __launch_bounds__(DPP_THREADS) void pose_finish_kernel(const float* __restrict__ net_out, int B, int J, const float* __restrict__ cube,
                                                                  const float* __restrict__ com3d, AugCam cam, int flags,
                                                                  const int* __restrict__ tflags, const int* __restrict__ src,
                                                                  const SourceRec* __restrict__ tab, float* __restrict__ pose3d,
                                                                  float* __restrict__ pose_img) {
    const int i = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (i >= B * J) return;
    const int b = i / J;
    source_camera(tab, track_source(src, b), cam);                     // the row's own camera (a workgroup may span rows)
    if (tflags) flags = tflags[b];                                     // the row's own sign rules
    float p[3] = {net_out[(size_t)i * 3], net_out[(size_t)i * 3 + 1], net_out[(size_t)i * 3 + 2]};
    if (flags & POSE_INV_X) p[1] = -p[1];
    if (flags & POSE_INV_Y) p[0] = -p[0];
    if (flags & POSE_HAND_RIGHT) p[0] = -p[0];
    const float cz = cube[b * 3 + 2];
    float q[3];
    for (int d = 0; d < 3; ++d) {
        float v = p[d] * cz;               // three float32 roundings: * cube_z, / 2., + com3D
        v = v / 2.0f;
        q[d] = v + com3d[b * 3 + d];
        pose3d[(size_t)i * 3 + d] = q[d];
    }
    float u[3];
    toimg(cam, q[0], q[1], q[2], true, u);
    for (int d = 0; d < 3; ++d) pose_img[(size_t)i * 3 + d] = u[d];
}

// HandDetector.refineCoMIterative (handdetector.py:546-567): num_iter times bounds -> getCrop -> calculateCoM -> fallback -> back to
// frame coordinates with the reference's max(xstart, 0) (sic).  One workgroup per frame runs ALL iterations; the centre stays
// float64 between them as on the host.  Window sums in float64 (column / row sums are integers, a sum of float32 depths of
// 10..1500 mm over at most a frame is exact: the order is free); the mean as NumPy forms it: sum / num, * num, / num.
// A centre whose depth is isclose to 0 ("CoM ill-defined") stops the frame with status 1 (com_out: the centre so far).
// src (ABI v17; NULL: row r works on frame r): row r refines com_in[r] in frame src[r], with that frame's partials and cube.
__global__ __launch_bounds__(DPP_THREADS) void refine_com_iterative_kernel(const float* __restrict__ frames, int H, int W,
                                                                           const float* __restrict__ partial, const int* __restrict__ src,
                                                                           const float* __restrict__ com_in, const float* __restrict__ cube,
                                                                           double fx, double fy, int num_iter, float* __restrict__ com_out,
                                                                           int* __restrict__ status) {
    __shared__ double s_red[4][DPP_THREADS / DPP_WAVE];
    __shared__ CropRec s_r;
    __shared__ double s_com[3];
    __shared__ int s_stop;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int fb = src ? src[b] : b;                                   // the row's frame
    const float* f = frames + (size_t)fb * H * W;
    float mn, mx;
    frame_range_reduce(partial, fb, tid & 63, mn, mx);
    const double size[3] = {(double)cube[fb * 3], (double)cube[fb * 3 + 1], (double)cube[fb * 3 + 2]};
    if (tid == 0) {
        for (int d = 0; d < 3; ++d) s_com[d] = (double)com_in[b * 3 + d];
        s_stop = 0;
        s_r.max_depth = fminf(1500.0f, mx);
        s_r.min_depth = fmaxf(10.0f, mn);
    }
    for (int it = 0; it < num_iter; ++it) {
        if (tid == 0) {
            if (fabs(s_com[2]) <= 1e-8 || !(fabs(s_com[0]) <= 1e300 && fabs(s_com[1]) <= 1e300 && fabs(s_com[2]) <= 1e300)) {
                s_stop = 1;
            } else {
                int bd[4];
                com_to_bounds(s_com, size, fx, fy, bd);
                s_r.xstart = bd[0]; s_r.ystart = bd[2]; s_r.cw = bd[1] - bd[0]; s_r.ch = bd[3] - bd[2];
                s_r.zstart = (float)(s_com[2] - size[2] / 2.);            // the window is a float32 array: its thresholds round to it
                s_r.zend = (float)(s_com[2] + size[2] / 2.);
            }
        }
        __syncthreads();
        if (s_stop) break;
        const CropRec r = s_r;
        // only the part of the window inside the frame can hold valid pixels
        const int y0 = r.ystart < 0 ? -r.ystart : 0, y1 = (r.ystart + r.ch > H) ? H - r.ystart : r.ch;
        const int x0 = r.xstart < 0 ? -r.xstart : 0, x1 = (r.xstart + r.cw > W) ? W - r.xstart : r.cw;
        double sx, sy, sd, cnt;
        com_window_sums(f, H, W, r, x0, x1, y0, y1, sx, sy, sd, cnt);
        if (com_block_sums(sx, sy, sd, cnt, s_red)) {
            double c0 = 0.0, c1 = 0.0, c2 = 0.0;
            if (cnt > 0.0) { c0 = sx / cnt * cnt / cnt; c1 = sy / cnt * cnt / cnt; c2 = sd / cnt; }
            if (fabs(c0) <= 1e-8 && fabs(c1) <= 1e-8 && fabs(c2) <= 1e-8 && r.cw > 0 && r.ch > 0)     // numpy.allclose(com, 0.)
                c2 = (double)crop_window_value(f, H, W, r, r.cw / 2, r.ch / 2, 0, 0.0f);
            s_com[0] = c0 + (double)(r.xstart > 0 ? r.xstart : 0);
            s_com[1] = c1 + (double)(r.ystart > 0 ? r.ystart : 0);
            s_com[2] = c2;
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int d = 0; d < 3; ++d) com_out[b * 3 + d] = (float)s_com[d];
        status[b] = s_stop;
    }
}

}  // namespace

extern "C" size_t dpp_crop_record_bytes(void) { return sizeof(CropRec); }

extern "C" int dpp_crop_prepare(const float* frames, int B, int H, int W, const float* com, const float* cube, double fx, double fy,
                                int dsz, int stretch, void* records, float* M_out, dpp_stream_t stream) {
    if (!frames || !com || !cube || !records || B < 1 || H < 1 || W < 1 || dsz < 1 || fx == 0.0 || fy == 0.0) return DPP_E_BADARG;
    DPP_LAUNCH(crop_prepare_kernel, dim3(B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W, com, cube,
                       fabs(fx), fabs(fy), dsz, stretch, static_cast<CropRec*>(records), M_out);
    return dpp_launch_status();
}

// tab (null: the launch's H, W hold for every row): the table of the *_src entry points, which pass no frame size of their own
static int launch_crop_warp(const float* frames, const void* records, int B, int H, int W, int dsz, int normalize, float nd_value,
                            const int* src, const SourceRec* tab, float* out, dpp_stream_t stream) {
    if (!frames || !records || !out || B < 1 || (!tab && (H < 1 || W < 1)) || dsz < 1) return DPP_E_BADARG;
    dim3 grid(dpp_cdiv(dsz * dsz, DPP_THREADS), B);
    DPP_LAUNCH(crop_warp_kernel, grid, dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W,
                       static_cast<const CropRec*>(records), dsz, normalize, nd_value, src, tab, out);
    return dpp_launch_status();
}

extern "C" int dpp_crop_warp(const float* frames, const void* records, int B, int H, int W, int dsz, int normalize, float nd_value,
                             float* out, dpp_stream_t stream) {
    return launch_crop_warp(frames, records, B, H, W, dsz, normalize, nd_value, nullptr, nullptr, out, stream);
}

extern "C" size_t dpp_crop_com_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * COM_BANDS * 4 * sizeof(double); }

extern "C" int dpp_crop_com(const float* frames, const void* records, int B, int H, int W, void* workspace, float* com_out,
                            dpp_stream_t stream) {
    if (!frames || !records || !workspace || !com_out || B < 1 || H < 1 || W < 1) return DPP_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DPP_LAUNCH(crop_com_partial_kernel, dim3(COM_BANDS, B), dim3(DPP_THREADS), 0, st, frames, H, W, static_cast<const CropRec*>(records),
               static_cast<double*>(workspace));
    DPP_LAUNCH(crop_com_finish_kernel, dim3(dpp_cdiv(B, DPP_THREADS)), dim3(DPP_THREADS), 0, st, frames, B, H, W,
               static_cast<const CropRec*>(records), static_cast<const double*>(workspace), com_out);
    return dpp_launch_status();
}

extern "C" int dpp_crop_refine(const float* frames, const void* records, int B, int H, int W, const float* com_in, const float* cube,
                               const float* net_out, double fx, double fy, double ux, double uy, int flip_y, const float* gt3d_orig, int J,
                               const float* pca_mean, const float* pca_comp, int E, float* com_out, float* com3d_out, float* gt3d_crop,
                               float* out_y, dpp_stream_t stream) {
    if (!frames || !records || !com_in || !cube || !net_out || !com_out || B < 1 || H < 1 || W < 1 || fx == 0.0 || fy == 0.0) return DPP_E_BADARG;
    if (gt3d_orig && (J < 1 || J * 3 > MAXJ3)) return DPP_E_BADARG;
    if ((gt3d_crop || out_y) && !gt3d_orig) return DPP_E_BADARG;
    if (pca_comp && (!pca_mean || E < 1)) return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    DPP_LAUNCH(crop_refine_kernel, dim3(B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W,
               static_cast<const CropRec*>(records), com_in, cube, net_out, cam, gt3d_orig, J, pca_mean, pca_comp, E, com_out, com3d_out,
               gt3d_crop, out_y);
    return dpp_launch_status();
}

static int launch_crop_warp_ex(const float* frames, const void* records, int B, int H, int W, int dsz, int flags, float nd_value,
                               float fill_value, float pad_value, const int* src, const int* tflags, const SourceRec* tab, float* out,
                               dpp_stream_t stream) {
    dim3 grid(dpp_cdiv(dsz * dsz, DPP_THREADS), B);
    DPP_LAUNCH(crop_warp_ex_kernel, grid, dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W,
               static_cast<const CropRec*>(records), dsz, flags, nd_value, fill_value, pad_value, src, tflags, tab, out);
    return dpp_launch_status();
}

extern "C" int dpp_crop_warp_ex(const float* frames, const void* records, int B, int H, int W, int dsz, int flags, float nd_value,
                                float fill_value, float pad_value, float* out, dpp_stream_t stream) {
    if (!frames || !records || !out || B < 1 || H < 1 || W < 1 || dsz < 1 || (flags & ~31)) return DPP_E_BADARG;
    return launch_crop_warp_ex(frames, records, B, H, W, dsz, flags, nd_value, fill_value, pad_value, nullptr, nullptr, nullptr, out, stream);
}

extern "C" int dpp_resize_crops(const float* src, int B, int sh, int sw, int dh, int dw, int bilinear, float nd_value, float* out,
                                dpp_stream_t stream) {
    if (!src || !out || src == out || B < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1) return DPP_E_BADARG;
    if (bilinear && (sw < 2 || sh < 2)) return DPP_E_BADARG;           // bilinearResize: "Shape mismatch"
    const double ifx = 1. / ((double)dw / (double)sw), ify = 1. / ((double)dh / (double)sh);
    dim3 grid(dpp_cdiv(dh * dw, DPP_THREADS), B);
    DPP_LAUNCH(resize_crops_kernel, grid, dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), src, sh, sw, dh, dw, bilinear ? 1 : 0,
               nd_value, ifx, ify, out);
    return dpp_launch_status();
}

extern "C" int dpp_recrop(const float* crops, int B, int h, int w, const double* M, const double* Mnew, int th, int tw, float background,
                          double nv_val, int thresh_z, const float* zrange, float* out, dpp_stream_t stream) {
    if (!crops || !M || !Mnew || !out || crops == out || B < 1 || h < 1 || w < 1 || th < 1 || tw < 1) return DPP_E_BADARG;
    if (thresh_z && !zrange) return DPP_E_BADARG;
    dim3 grid(dpp_cdiv(th * tw, DPP_THREADS), B);
    DPP_LAUNCH(recrop_kernel, grid, dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), crops, h, w, M, Mnew, th, tw, background, nv_val,
               thresh_z ? 1 : 0, zrange, out);
    return dpp_launch_status();
}

extern "C" int dpp_inverse_crop(const float* crops, int B, int ch, int cw, const int* bounds, const float* zrange, int H, int W, int bilinear,
                                float nd_value, float background, int thresh_z, float* out, dpp_stream_t stream) {
    if (!crops || !bounds || !out || crops == out || B < 1 || ch < 1 || cw < 1 || H < 1 || W < 1) return DPP_E_BADARG;
    if (bilinear && (cw < 2 || ch < 2)) return DPP_E_BADARG;
    if (thresh_z && !zrange) return DPP_E_BADARG;
    dim3 grid(dpp_cdiv(H * W, DPP_THREADS), B);
    DPP_LAUNCH(inverse_crop_kernel, grid, dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), crops, ch, cw, bounds, zrange, H, W,
               bilinear ? 1 : 0, nd_value, background, thresh_z ? 1 : 0, out);
    return dpp_launch_status();
}

extern "C" size_t dpp_frame_range_bytes(int B) { return (size_t)(B > 0 ? B : 0) * FR_BANDS * 2 * sizeof(float); }

extern "C" int dpp_frame_range(const float* frames, int B, int H, int W, float* partial, dpp_stream_t stream) {
    if (!frames || !partial || B < 1 || H < 1 || W < 1) return DPP_E_BADARG;
    DPP_LAUNCH(frame_range_kernel, dim3(FR_BANDS, B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W,
               static_cast<const SourceRec*>(nullptr), partial);
    return dpp_launch_status();
}

static int launch_crop_prepare_ranged(const float* partial, int B, const float* com, const float* cube, double fx, double fy, int dsz,
                                      int stretch, const int* src, const int* gate, const SourceRec* tab, void* records, float* M_out,
                                      dpp_stream_t stream) {
    if (!partial || !com || !cube || !records || B < 1 || dsz < 1 || (!tab && (fx == 0.0 || fy == 0.0))) return DPP_E_BADARG;
    DPP_LAUNCH(crop_prepare_ranged_kernel, dim3(B), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), partial, com, cube, fabs(fx), fabs(fy),
               dsz, stretch, src, gate, tab, static_cast<CropRec*>(records), M_out);
    return dpp_launch_status();
}

extern "C" int dpp_crop_prepare_ranged(const float* partial, int B, const float* com, const float* cube, double fx, double fy, int dsz,
                                       int stretch, void* records, float* M_out, dpp_stream_t stream) {
    return launch_crop_prepare_ranged(partial, B, com, cube, fx, fy, dsz, stretch, nullptr, nullptr, nullptr, records, M_out, stream);
}

static int launch_track_refine(const float* frames, const void* records_in, int B, int H, int W, const float* com_in, const float* cube,
                               const float* net_out, double fx, double fy, double ux, double uy, int flip_y, double crop_fx, double crop_fy,
                               int dsz, const int* src, const int* gate, const SourceRec* tab, float* com_out, float* com3d_out,
                               void* records_out, float* M_out, int* status, dpp_stream_t stream) {
    if (!frames || !records_in || !com_in || !cube || !net_out || !com_out || !com3d_out || !records_out || !status || B < 1 || dsz < 1)
        return DPP_E_BADARG;
    if (!tab && (H < 1 || W < 1 || fx == 0.0 || fy == 0.0 || crop_fx == 0.0 || crop_fy == 0.0)) return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    DPP_LAUNCH(track_refine_kernel, dim3(B), dim3(DPP_WAVE), 0, static_cast<hipStream_t>(stream), frames, H, W,
               static_cast<const CropRec*>(records_in), com_in, cube, net_out, cam, fabs(crop_fx), fabs(crop_fy), dsz, src, gate, tab, com_out,
               com3d_out, static_cast<CropRec*>(records_out), M_out, status);
    return dpp_launch_status();
}

extern "C" int dpp_track_refine(const float* frames, const void* records_in, int B, int H, int W, const float* com_in, const float* cube,
                                const float* net_out, double fx, double fy, double ux, double uy, int flip_y, double crop_fx, double crop_fy,
                                int dsz, float* com_out, float* com3d_out, void* records_out, float* M_out, int* status,
                                dpp_stream_t stream) {
    return launch_track_refine(frames, records_in, B, H, W, com_in, cube, net_out, fx, fy, ux, uy, flip_y, crop_fx, crop_fy, dsz, nullptr,
                               nullptr, nullptr, com_out, com3d_out, records_out, M_out, status, stream);
}

static int launch_pose_finish(const float* net_out, int B, int J, const float* cube, const float* com3d, double fx, double fy, double ux,
                              double uy, int flip_y, int flags, const int* tflags, const int* src, const SourceRec* tab, float* pose3d, float* pose_img,
                              dpp_stream_t stream) {
    if (!net_out || !cube || !com3d || !pose3d || !pose_img || B < 1 || J < 1 || (!tab && (fx == 0.0 || fy == 0.0)) || (flags & ~7))
        return DPP_E_BADARG;
    AugCam cam;
    cam.fx = fx; cam.fy = fy; cam.ux = ux; cam.uy = uy; cam.flip_y = flip_y;
    DPP_LAUNCH(pose_finish_kernel, dim3(dpp_cdiv(B * J, DPP_THREADS)), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), net_out, B, J,
               cube, com3d, cam, flags, tflags, src, tab, pose3d, pose_img);
    return dpp_launch_status();
}

extern "C" int dpp_pose_finish(const float* net_out, int B, int J, const float* cube, const float* com3d, double fx, double fy, double ux,
                               double uy, int flip_y, int flags, float* pose3d, float* pose_img, dpp_stream_t stream) {
    return launch_pose_finish(net_out, B, J, cube, com3d, fx, fy, ux, uy, flip_y, flags, nullptr, nullptr, nullptr, pose3d, pose_img, stream);
}

static int launch_refine_com_iterative(const float* frames, const float* partial, int B, const int* src, int H, int W, const float* com_in,
                                       const float* cube, double fx, double fy, int num_iter, float* com_out, int* status,
                                       dpp_stream_t stream) {
    if (!frames || !partial || !com_in || !cube || !com_out || !status || B < 1 || H < 1 || W < 1 || num_iter < 0 || fx == 0.0 || fy == 0.0)
        return DPP_E_BADARG;
    DPP_LAUNCH(refine_com_iterative_kernel, dim3(B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W, partial, src, com_in,
               cube, fabs(fx), fabs(fy), num_iter, com_out, status);
    return dpp_launch_status();
}

extern "C" int dpp_refine_com_iterative(const float* frames, const float* partial, int B, int H, int W, const float* com_in, const float* cube,
                                        double fx, double fy, int num_iter, float* com_out, int* status, dpp_stream_t stream) {
    return launch_refine_com_iterative(frames, partial, B, nullptr, H, W, com_in, cube, fx, fy, num_iter, com_out, status, stream);
}

// R rows over the frames src names (ABI v17): several centres of one frame, as the several-hands detector refines them; a NULL
// src is the plain entry point.  The caller guarantees that src[r] is a frame of `frames`; rows of a frame share its cube.
extern "C" int dpp_refine_com_iterative_ix(const float* frames, const float* partial, int R, const int* src, int H, int W, const float* com_in,
                                           const float* cube, double fx, double fy, int num_iter, float* com_out, int* status,
                                           dpp_stream_t stream) {
    return launch_refine_com_iterative(frames, partial, R, src, H, W, com_in, cube, fx, fy, num_iter, com_out, status, stream);
}

// ---- several tracks over several frames (ABI v16): the five tracking launches with one (src, gate, tflags) entry per track ----------
extern "C" int dpp_crop_prepare_ranged_ix(const float* partial, int T, const int* src, const int* gate, const float* com, const float* cube,
                                          double fx, double fy, int dsz, int stretch, void* records, float* M_out, dpp_stream_t stream) {
    if (!src || !gate) return DPP_E_BADARG;
    return launch_crop_prepare_ranged(partial, T, com, cube, fx, fy, dsz, stretch, src, gate, nullptr, records, M_out, stream);
}

extern "C" int dpp_crop_warp_ix(const float* frames, const void* records, int T, const int* src, int H, int W, int dsz, int normalize,
                                float nd_value, float* out, dpp_stream_t stream) {
    if (!src) return DPP_E_BADARG;
    return launch_crop_warp(frames, records, T, H, W, dsz, normalize, nd_value, src, nullptr, out, stream);
}

extern "C" int dpp_track_refine_ix(const float* frames, const void* records_in, int T, const int* src, const int* gate, int H, int W,
                                   const float* com_in, const float* cube, const float* net_out, double fx, double fy, double ux, double uy,
                                   int flip_y, double crop_fx, double crop_fy, int dsz, float* com_out, float* com3d_out, void* records_out,
                                   float* M_out, int* status, dpp_stream_t stream) {
    if (!src || !gate) return DPP_E_BADARG;
    return launch_track_refine(frames, records_in, T, H, W, com_in, cube, net_out, fx, fy, ux, uy, flip_y, crop_fx, crop_fy, dsz, src, gate,
                               nullptr, com_out, com3d_out, records_out, M_out, status, stream);
}

extern "C" int dpp_crop_warp_ex_ix(const float* frames, const void* records, int T, const int* src, const int* tflags, int H, int W, int dsz,
                                   int flags, float nd_value, float fill_value, float pad_value, float* out, dpp_stream_t stream) {
    if (!frames || !records || !src || !tflags || !out || T < 1 || H < 1 || W < 1 || dsz < 1 || (flags & ~15)) return DPP_E_BADARG;
    return launch_crop_warp_ex(frames, records, T, H, W, dsz, flags, nd_value, fill_value, pad_value, src, tflags, nullptr, out, stream);
}

extern "C" int dpp_pose_finish_ix(const float* net_out, int T, int J, const int* tflags, const float* cube, const float* com3d, double fx,
                                  double fy, double ux, double uy, int flip_y, float* pose3d, float* pose_img, dpp_stream_t stream) {
    if (!tflags) return DPP_E_BADARG;
    return launch_pose_finish(net_out, T, J, cube, com3d, fx, fy, ux, uy, flip_y, 0, tflags, nullptr, nullptr, pose3d, pose_img, stream);
}

// ---- frame sources of unlike cameras and sizes (ABI v19): the launches that read a frame or a camera, with the per-source table -----
// `sources`: C SourceRec on the device (geom.h), validated by the host; row t reads record src[t].  The same kernels as above: the
// table pointer replaces the launch's (H, W) and camera scalars, which are not passed here.
extern "C" size_t dpp_source_record_bytes(void) { return sizeof(SourceRec); }

extern "C" int dpp_frame_range_src(const float* frames, const void* sources, int C, float* partial, dpp_stream_t stream) {
    if (!frames || !sources || !partial || C < 1 || C > 65535) return DPP_E_BADARG;
    DPP_LAUNCH(frame_range_kernel, dim3(FR_BANDS, C), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, 0, 0,
               static_cast<const SourceRec*>(sources), partial);
    return dpp_launch_status();
}

extern "C" int dpp_crop_prepare_ranged_src(const float* partial, int T, const int* src, const int* gate, const void* sources, const float* com,
                                           const float* cube, int dsz, int stretch, void* records, float* M_out, dpp_stream_t stream) {
    if (!src || !gate || !sources) return DPP_E_BADARG;
    return launch_crop_prepare_ranged(partial, T, com, cube, 0.0, 0.0, dsz, stretch, src, gate, static_cast<const SourceRec*>(sources), records,
                                      M_out, stream);
}

extern "C" int dpp_crop_warp_src(const float* frames, const void* records, int T, const int* src, const void* sources, int dsz, int normalize,
                                 float nd_value, float* out, dpp_stream_t stream) {
    if (!src || !sources) return DPP_E_BADARG;
    return launch_crop_warp(frames, records, T, 0, 0, dsz, normalize, nd_value, src, static_cast<const SourceRec*>(sources), out, stream);
}

extern "C" int dpp_track_refine_src(const float* frames, const void* records_in, int T, const int* src, const int* gate, const void* sources,
                                    const float* com_in, const float* cube, const float* net_out, int dsz, float* com_out, float* com3d_out,
                                    void* records_out, float* M_out, int* status, dpp_stream_t stream) {
    if (!src || !gate || !sources) return DPP_E_BADARG;
    return launch_track_refine(frames, records_in, T, 0, 0, com_in, cube, net_out, 0.0, 0.0, 0.0, 0.0, 0, 0.0, 0.0, dsz, src, gate,
                               static_cast<const SourceRec*>(sources), com_out, com3d_out, records_out, M_out, status, stream);
}

extern "C" int dpp_crop_warp_ex_src(const float* frames, const void* records, int T, const int* src, const int* tflags, const void* sources,
                                    int dsz, int flags, float nd_value, float fill_value, float pad_value, float* out, dpp_stream_t stream) {
    if (!frames || !records || !src || !tflags || !sources || !out || T < 1 || dsz < 1 || (flags & ~15)) return DPP_E_BADARG;
    return launch_crop_warp_ex(frames, records, T, 0, 0, dsz, flags, nd_value, fill_value, pad_value, src, tflags,
                               static_cast<const SourceRec*>(sources), out, stream);
}

extern "C" int dpp_pose_finish_src(const float* net_out, int T, int J, const int* src, const int* tflags, const void* sources, const float* cube,
                                   const float* com3d, float* pose3d, float* pose_img, dpp_stream_t stream) {
    if (!src || !tflags || !sources) return DPP_E_BADARG;
    return launch_pose_finish(net_out, T, J, cube, com3d, 0.0, 0.0, 0.0, 0.0, 0, 0, tflags, src, static_cast<const SourceRec*>(sources), pose3d,
                              pose_img, stream);
}
