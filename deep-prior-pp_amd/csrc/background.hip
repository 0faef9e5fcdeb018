// background.hip -- a learned static background removed from the float32 frame before anything looks at it, for gfx950 (ABI v25).
//
// A fixed depth camera sees a desk edge, a monitor, the user's torso in every frame; the detector starts from the NEAREST object and
// crop_warp keeps whatever lies inside the cube.  The reference has no counterpart (its demo is one hand in front of an empty range):
// these are this project's own semantics, restated in NumPy by tests/background_ref.py and pinned bit for bit.
//
//   model, per source and pixel      near (float32; 0: nothing seen), the smallest non-zero depth of the learning frames
//                                    seen (int32), the number of learning frames in which the pixel had a depth
//   learning one frame f             where f != 0:  near = (near == 0 || f < near) ? f : near;  seen += 1
//   cut map (HOST, once per model)   near - (margin + rel * near), every operation rounded to float32, where seen >= min_seen, near != 0
//                                    and the result is > 0; elsewhere +inf: no background is known, every depth is foreground
//   applying it                      out = (f != 0 && f < cut) ? f : 0, written IN PLACE; a depth exactly at cut is background
//
// Applying is a selection and learning a selection and an integer increment: nothing here rounds, so this unit is not on the
// -ffp-contract=off lists of the Makefile although it includes geom.h (FR_BANDS, block_minmax and the source table only).  Comparisons
// and selects, no fminf on the frame's values, as in ingest.hip.  Applying twice gives the bits of applying once (an element that was
// kept is below its cut again, a zero stays zero): a source that delivers no frame in a tick has its stale, masked frame masked again.
//
// Shape: grid (FR_BANDS, B), DPP_THREADS, the element partition of frame_range_kernel -- thread t = band * DPP_THREADS + tid of
// nt = FR_BANDS * DPP_THREADS takes the 16-byte groups t, t + nt, ... of frame b where the frame, the cut map and the element count
// allow 16-byte accesses, else the single elements t, t + nt, ... (a second frame of odd H * W starts unaligned).  Unlike the range
// pass, a lane past the end reads and writes NOTHING: every element is read and written by the one thread that owns it.  The band's
// (min, max) over what it stored goes through block_minmax into frame_range's partials; every band writes its pair, a band without
// elements the identities.  With the per-source table (ABI v19) workgroup (band, c) takes H, W and the element offset of source c from
// record c -- the cut map and the model share the ragged layout of the frames, the padding words between frames are never touched.
#include "geom.h"

namespace {

__device__ __forceinline__ bool bg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ float bg_keep(float f, float cut) { return (f != 0.0f && f < cut) ? f : 0.0f; }

// element offset of frame b in the frames' layout (and so in the cut map's and the model's); with a table H, W become source b's
__device__ __forceinline__ size_t bg_frame_offset(const SourceRec* __restrict__ tab, int b, int& H, int& W) {
    if (tab == nullptr) return (size_t)b * H * W;
    H = tab[b].H; W = tab[b].W;
    return (size_t)tab[b].frame_off;
}

__global__ __launch_bounds__(DPP_THREADS) void frame_background_kernel(float* __restrict__ frames, const float* __restrict__ cutmap, int H, int W,
                                                                       const SourceRec* __restrict__ tab, float* __restrict__ partial) {
    __shared__ float s_mn[DPP_THREADS / DPP_WAVE], s_mx[DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const size_t off = bg_frame_offset(tab, b, H, W);
    float* f = frames + off;
    const float* c = cutmap + off;
    const int npx = H * W;
    const int t = band * DPP_THREADS + tid, nt = FR_BANDS * DPP_THREADS;
    float mn = 3.4e38f, mx = -3.4e38f;
    if ((npx & 3) == 0 && bg_aligned16(f) && bg_aligned16(c)) {
        float4* f4 = reinterpret_cast<float4*>(f);
        const float4* c4 = reinterpret_cast<const float4*>(c);
        const int n4 = npx >> 2;
        for (int i = t; i < n4; i += 4 * nt) {               // four groups in flight per thread; a group past the end is not touched
            float4 v[4], k[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = i + u * nt;
                if (j < n4) { v[u] = f4[j]; k[u] = c4[j]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = i + u * nt;
                if (j < n4) {
                    const float4 o = make_float4(bg_keep(v[u].x, k[u].x), bg_keep(v[u].y, k[u].y), bg_keep(v[u].z, k[u].z), bg_keep(v[u].w, k[u].w));
                    f4[j] = o;
                    mn = fminf(mn, fminf(fminf(o.x, o.y), fminf(o.z, o.w)));
                    mx = fmaxf(mx, fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w)));
                }
            }
        }
    } else {
        for (int i = t; i < npx; i += nt) {
            const float o = bg_keep(f[i], c[i]);
            f[i] = o;
            mn = fminf(mn, o); mx = fmaxf(mx, o);
        }
    }
    if (partial == nullptr) return;
    if (!block_minmax(mn, mx, s_mn, s_mx)) return;
    partial[((size_t)b * FR_BANDS + band) * 2] = mn;
    partial[((size_t)b * FR_BANDS + band) * 2 + 1] = mx;
}

// one learning frame into the model of every source that takes part (take[b] != 0); the same partition, no reduction
__global__ __launch_bounds__(DPP_THREADS) void background_learn_kernel(const float* __restrict__ frames, const int* __restrict__ take, int H, int W,
                                                                       const SourceRec* __restrict__ tab, float* __restrict__ near_,
                                                                       int* __restrict__ seen) {
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    if (take[b] == 0) return;
    const size_t off = bg_frame_offset(tab, b, H, W);
    const float* f = frames + off;
    float* nr = near_ + off;
    int* sn = seen + off;
    const int npx = H * W;
    const int t = band * DPP_THREADS + tid, nt = FR_BANDS * DPP_THREADS;
    if ((npx & 3) == 0 && bg_aligned16(f) && bg_aligned16(nr) && bg_aligned16(sn)) {
        const float4* f4 = reinterpret_cast<const float4*>(f);
        float4* n4p = reinterpret_cast<float4*>(nr);
        int4* s4p = reinterpret_cast<int4*>(sn);
        const int n4 = npx >> 2;
        for (int j = t; j < n4; j += nt) {
            const float4 v = f4[j];
            float4 n = n4p[j];
            int4 s = s4p[j];
            if (v.x != 0.0f) { n.x = (n.x == 0.0f || v.x < n.x) ? v.x : n.x; s.x += 1; }
            if (v.y != 0.0f) { n.y = (n.y == 0.0f || v.y < n.y) ? v.y : n.y; s.y += 1; }
            if (v.z != 0.0f) { n.z = (n.z == 0.0f || v.z < n.z) ? v.z : n.z; s.z += 1; }
            if (v.w != 0.0f) { n.w = (n.w == 0.0f || v.w < n.w) ? v.w : n.w; s.w += 1; }
            n4p[j] = n;
            s4p[j] = s;
        }
    } else {
        for (int i = t; i < npx; i += nt) {
            const float v = f[i];
            if (v != 0.0f) {
                const float n = nr[i];
                nr[i] = (n == 0.0f || v < n) ? v : n;
                sn[i] += 1;
            }
        }
    }
}

// [a, a + n elements of esz bytes) and [b, ...) share a byte
bool bg_overlap(const void* a, const void* b, size_t n, size_t esz_a, size_t esz_b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + n * esz_a;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + n * esz_b;
    return a0 < b1 && b0 < a1;
}

bool bg_bad_shape(int B, int H, int W) { return B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL; }

}  // namespace

extern "C" int dpp_frame_background(float* frames, const float* cut, int B, int H, int W, float* partial, dpp_stream_t stream) {
    if (!frames || !cut || bg_bad_shape(B, H, W)) return DPP_E_BADARG;
    if (bg_overlap(frames, cut, (size_t)B * H * W, 4, 4)) return DPP_E_BADARG;       // a frame is rewritten while other workgroups read cut
    DPP_LAUNCH(frame_background_kernel, dim3(FR_BANDS, B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, cut, H, W,
               static_cast<const SourceRec*>(nullptr), partial);
    return dpp_launch_status();
}

// C sources of unlike sizes (ABI v19): frames and cut share the ragged layout of sources[c].frame_off.  The host has validated the
// table and keeps the two buffers apart; only what needs no device memory is checked here.
extern "C" int dpp_frame_background_src(float* frames, const float* cut, const void* sources, int C, float* partial, dpp_stream_t stream) {
    if (!frames || !cut || !sources || static_cast<const float*>(frames) == cut || C < 1 || C > 65535) return DPP_E_BADARG;
    DPP_LAUNCH(frame_background_kernel, dim3(FR_BANDS, C), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, cut, 0, 0,
               static_cast<const SourceRec*>(sources), partial);
    return dpp_launch_status();
}

extern "C" int dpp_background_learn(const float* frames, const int* take, int B, int H, int W, float* near_, int* seen, dpp_stream_t stream) {
    if (!frames || !take || !near_ || !seen || bg_bad_shape(B, H, W)) return DPP_E_BADARG;
    const size_t n = (size_t)B * H * W;
    if (bg_overlap(frames, near_, n, 4, 4) || bg_overlap(frames, seen, n, 4, 4) || bg_overlap(near_, seen, n, 4, 4)) return DPP_E_BADARG;
    DPP_LAUNCH(background_learn_kernel, dim3(FR_BANDS, B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, take, H, W,
               static_cast<const SourceRec*>(nullptr), near_, seen);
    return dpp_launch_status();
}

extern "C" int dpp_background_learn_src(const float* frames, const int* take, const void* sources, int C, float* near_, int* seen,
                                        dpp_stream_t stream) {
    if (!frames || !take || !sources || !near_ || !seen || C < 1 || C > 65535) return DPP_E_BADARG;
    if (frames == near_ || static_cast<const void*>(frames) == static_cast<const void*>(seen) ||
        static_cast<const void*>(near_) == static_cast<const void*>(seen)) return DPP_E_BADARG;
    DPP_LAUNCH(background_learn_kernel, dim3(FR_BANDS, C), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, take, 0, 0,
               static_cast<const SourceRec*>(sources), near_, seen);
    return dpp_launch_status();
}
