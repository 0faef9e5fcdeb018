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
// Applying is a selection and learning a selection and an integer increment: nothing in them rounds (of geom.h they take FR_BANDS,
// block_minmax and the source table only).  Comparisons and selects, no fminf on the frame's values, as in ingest.hip.  Applying
// twice gives the bits of applying once (an element that was kept is below its cut again, a zero stays zero): a source that
// delivers no frame in a tick has its stale, masked frame masked again.
//
// Shape: grid (FR_BANDS, B), DPP_THREADS, the element partition of frame_range_kernel -- thread t = band * DPP_THREADS + tid of
// nt = FR_BANDS * DPP_THREADS takes the 16-byte groups t, t + nt, ... of frame b where the frame, the cut map and the element count
// allow 16-byte accesses, else the single elements t, t + nt, ... (a second frame of odd H * W starts unaligned).  Unlike the range
// pass, a lane past the end reads and writes NOTHING: every element is read and written by the one thread that owns it.  The band's
// (min, max) over what it stored goes through block_minmax into frame_range's partials; every band writes its pair, a band without
// elements the identities.  With the per-source table (ABI v19) workgroup (band, c) takes H, W and the element offset of source c from
// record c -- the cut map and the model share the ragged layout of the frames, the padding words between frames are never touched.
//
// Keeping the model current while tracking (dpp_frame_background_adapt; tests/background_adapt_ref.py is the definition): the cut
// launch itself adapts the model from the raw depth it is about to overwrite -- near / seen confirmed, a candidate depth `cand` counted
// over `run` ticks and taken over at `persist`, the windows of the tracked hands (crop_rec.h, as track_refine left them) kept out,
// and the cut map rewritten ON THE DEVICE where the model changed.  That arithmetic rounds -- band(x) = margin + rel * x and
// near - band, three float32 operations -- so this unit IS on the Makefile's -ffp-contract=off lists now, for the product and for
// the emulator: a contracted multiply-add would move the cut by an ulp against the host's NumPy cut map.
#include "geom.h"
#include "crop_rec.h"

namespace {

__device__ __forceinline__ bool bg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ float bg_keep(float f, float cut) { return (f != 0.0f && f < cut) ? f : 0.0f; }

// element offset of frame b in the frames' layout (and so in the cut map's and the model's); with a table H, W become source b's
__device__ __forceinline__ size_t bg_frame_offset(const SourceRec* __restrict__ tab, int b, int& H, int& W) {
    if (tab == nullptr) return (size_t)b * H * W;
    H = tab[b].H; W = tab[b].W;
    return (size_t)tab[b].frame_off;
}

// The cut over frame f (npx elements, cut map c) in the partition above, by thread t of nt; (mn, mx) gather what was stored.
__device__ __forceinline__ void bg_cut_sweep(float* __restrict__ f, const float* __restrict__ c, int npx, int t, int nt, float& mn, float& mx) {
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
}

__global__ __launch_bounds__(DPP_THREADS) void frame_background_kernel(float* __restrict__ frames, const float* __restrict__ cutmap, int H, int W,
                                                                       const SourceRec* __restrict__ tab, float* __restrict__ partial) {
    __shared__ float s_mn[DPP_THREADS / DPP_WAVE], s_mx[DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const size_t off = bg_frame_offset(tab, b, H, W);
    float mn = 3.4e38f, mx = -3.4e38f;
    bg_cut_sweep(frames + off, cutmap + off, H * W, band * DPP_THREADS + tid, FR_BANDS * DPP_THREADS, mn, mx);
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

// ---- the model kept current while tracking: adaptation inside the cut launch ----------------------------------------------------------
// frame_background_adapt_kernel is frame_background_kernel -- its grid, its element partition (decided by the frame and the cut map
// alone), its partials -- and, for a source with take[b] != 0, one step of tests/background_adapt_ref.py on every element it owns,
// from the RAW depth it holds in a register before the cut overwrites it.  A source with take[b] == 0 runs bg_cut_sweep and reads no
// model array.  Every element of all six arrays is read and written by the one thread that owns it; near / cand / run / cut are
// stored only for a 16-byte group (or element) in which they changed -- in the steady state that is `seen` alone.
struct BgWin { int x0, x1, y0, y1; };       // a track's dilated window clipped to the frame: [x0, x1) x [y0, y1), never empty
struct BgAdapt { float margin, rel; int min_seen, persist, guard; };
constexpr int BG_MAXWIN = 64;               // windows per source held in LDS; a source with more reads the rest from the records

__device__ __forceinline__ bool bg_window(const CropRec& r, int guard, int H, int W, BgWin& w) {
    if (r.cw <= 0 || r.ch <= 0) return false;                                   // a lost or gated track: the empty window
    const long long x0 = (long long)r.xstart - guard, x1 = (long long)r.xstart + r.cw + guard;
    const long long y0 = (long long)r.ystart - guard, y1 = (long long)r.ystart + r.ch + guard;
    w.x0 = (int)(x0 < 0 ? 0 : x0); w.x1 = (int)(x1 > W ? W : x1);
    w.y0 = (int)(y0 < 0 ? 0 : y0); w.y1 = (int)(y1 > H ? H : y1);
    return x0 < x1 && y0 < y1 && w.x0 < w.x1 && w.y0 < w.y1;
}

__device__ __forceinline__ bool bg_inside(const BgWin& w, int x, int y) { return x >= w.x0 && x < w.x1 && y >= w.y0 && y < w.y1; }

struct BgGuard {
    const BgWin* win; int n;                                                    // the windows in LDS
    const CropRec* rec; const int* src; int next, T, b, guard, H, W;             // tracks next .. T - 1 were not looked at yet
};

__device__ __forceinline__ bool bg_track_reads(const int* __restrict__ src, int t, int b) { return (src ? src[t] : t) == b; }

__device__ __forceinline__ bool bg_protected(const BgGuard& g, int x, int y) {
    for (int k = 0; k < g.n; ++k)
        if (bg_inside(g.win[k], x, y)) return true;
    for (int t = g.next; t < g.T; ++t) {
        BgWin w;
        if (bg_track_reads(g.src, t, g.b) && bg_window(g.rec[t], g.guard, g.H, g.W, w) && bg_inside(w, x, y)) return true;
    }
    return false;
}

// band(x) = float32(margin + float32(rel * x)) and the cut map's float32(near - band): three rounded operations, no contraction
__device__ __forceinline__ float bg_band(const BgAdapt& o, float x) { return o.margin + o.rel * x; }

__device__ __forceinline__ bool bg_in_band(const BgAdapt& o, float f, float ref) {
    const float bd = bg_band(o, ref);
    return f >= ref - bd && f <= ref + bd;
}

__device__ __forceinline__ float bg_cut_of(const BgAdapt& o, float near_, int seen) {
    const float c = near_ - bg_band(o, near_);
    return (seen >= o.min_seen && near_ != 0.0f && c > 0.0f) ? c : __int_as_float(0x7f800000);
}

// steps 3 - 7 of one tick for one pixel with raw depth f
__device__ __forceinline__ void bg_adapt_pixel(const BgAdapt& o, float f, bool prot, float& near_, int& seen, float& cand, int& run, float& cut) {
    if (prot) { cand = 0.0f; run = 0; return; }
    if (f == 0.0f) return;
    if (near_ != 0.0f && bg_in_band(o, f, near_)) {                              // confirm
        near_ = f < near_ ? f : near_;
        seen = seen < 0x7fffffff ? seen + 1 : seen;
        cand = 0.0f; run = 0;
    } else {                                                                    // candidate
        if (cand != 0.0f && bg_in_band(o, f, cand)) { cand = f < cand ? f : cand; run += 1; }
        else { cand = f; run = 1; }
        if (run < o.persist) return;
        near_ = cand; seen = run;                                               // the model is replaced
        cand = 0.0f; run = 0;
    }
    cut = bg_cut_of(o, near_, seen);
}

__device__ __forceinline__ void bg_ld4(const float* p, bool al, float v[4]) {
    if (al) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
}
__device__ __forceinline__ void bg_ld4(const int* p, bool al, int v[4]) {
    if (al) { const int4 q = *reinterpret_cast<const int4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
}
__device__ __forceinline__ void bg_st4(float* p, bool al, const float v[4]) {
    if (al) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
}
__device__ __forceinline__ void bg_st4(int* p, bool al, const int v[4]) {
    if (al) *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
    else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
}
__device__ __forceinline__ bool bg_differ(const float a[4], const float b[4]) {
    return ((__float_as_int(a[0]) ^ __float_as_int(b[0])) | (__float_as_int(a[1]) ^ __float_as_int(b[1])) |
            (__float_as_int(a[2]) ^ __float_as_int(b[2])) | (__float_as_int(a[3]) ^ __float_as_int(b[3]))) != 0;
}
__device__ __forceinline__ bool bg_differ(const int a[4], const int b[4]) { return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) != 0; }

__global__ __launch_bounds__(DPP_THREADS) void frame_background_adapt_kernel(float* __restrict__ frames, float* __restrict__ cutmap,
                                                                             float* __restrict__ near_, int* __restrict__ seen,
                                                                             float* __restrict__ cand, int* __restrict__ run,
                                                                             const int* __restrict__ take, int H, int W,
                                                                             const SourceRec* __restrict__ tab, const CropRec* __restrict__ rec, int T,
                                                                             const int* __restrict__ src, BgAdapt o, float* __restrict__ partial) {
    __shared__ float s_mn[DPP_THREADS / DPP_WAVE], s_mx[DPP_THREADS / DPP_WAVE];
    __shared__ BgWin s_win[BG_MAXWIN];
    __shared__ int s_n, s_next;
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const size_t off = bg_frame_offset(tab, b, H, W);
    float* f = frames + off;
    float* c = cutmap + off;
    const int npx = H * W;
    const int t = band * DPP_THREADS + tid, nt = FR_BANDS * DPP_THREADS;
    float mn = 3.4e38f, mx = -3.4e38f;
    if (take[b] == 0) {                                      // (uniform over the workgroup) the cut alone: no model array is read
        bg_cut_sweep(f, c, npx, t, nt, mn, mx);
    } else {
        if (rec == nullptr) T = 0;
        if (tid == 0) {                                      // the dilated windows of the tracks that read this source
            int n = 0, k = 0;
            for (; k < T && n < BG_MAXWIN; ++k)
                if (bg_track_reads(src, k, b) && bg_window(rec[k], o.guard, H, W, s_win[n])) ++n;
            s_n = n; s_next = k;
        }
        __syncthreads();
        BgGuard g = {s_win, s_n, rec, src, s_next, T, b, o.guard, H, W};
        bool any = g.n > 0;                                  // none: the row / column arithmetic is skipped
        for (int k = g.next; k < T && !any; ++k) any = bg_track_reads(src, k, b);
        float* nr = near_ + off;
        int* sn = seen + off;
        float* cd = cand + off;
        int* rn = run + off;
        if ((npx & 3) == 0 && bg_aligned16(f) && bg_aligned16(c)) {
            const bool al = bg_aligned16(nr) && bg_aligned16(sn) && bg_aligned16(cd) && bg_aligned16(rn);     // else: the model by elements
            const int n4 = npx >> 2;
            for (int j = t; j < n4; j += nt) {
                const size_t i = (size_t)j * 4;
                float fv[4], cv[4], nv[4], dv[4], c0[4], n0[4], d0[4];
                int sv[4], rv[4], s0[4], r0[4];
                bg_ld4(f + i, true, fv); bg_ld4(c + i, true, cv);
                bg_ld4(nr + i, al, nv); bg_ld4(sn + i, al, sv); bg_ld4(cd + i, al, dv); bg_ld4(rn + i, al, rv);
                int y = 0, x = 0;
                if (any) { y = (int)(i / W); x = (int)(i - (size_t)y * W); }       // a group may straddle rows: coordinates per element
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    c0[e] = cv[e]; n0[e] = nv[e]; d0[e] = dv[e]; s0[e] = sv[e]; r0[e] = rv[e];
                    const float out = bg_keep(fv[e], cv[e]);                      // with the cut as it stood before this tick
                    bg_adapt_pixel(o, fv[e], any && bg_protected(g, x, y), nv[e], sv[e], dv[e], rv[e], cv[e]);
                    fv[e] = out;
                    mn = fminf(mn, out); mx = fmaxf(mx, out);
                    if (++x == W) { x = 0; ++y; }
                }
                bg_st4(f + i, true, fv);
                if (bg_differ(sv, s0)) bg_st4(sn + i, al, sv);
                if (bg_differ(nv, n0)) bg_st4(nr + i, al, nv);
                if (bg_differ(dv, d0)) bg_st4(cd + i, al, dv);
                if (bg_differ(rv, r0)) bg_st4(rn + i, al, rv);
                if (bg_differ(cv, c0)) bg_st4(c + i, true, cv);
            }
        } else {
            for (int i = t; i < npx; i += nt) {
                const float v = f[i], c0 = c[i], n0 = nr[i], d0 = cd[i];
                const int s0 = sn[i], r0 = rn[i];
                float cv = c0, nv = n0, dv = d0;
                int sv = s0, rv = r0;
                const float out = bg_keep(v, c0);
                bool prot = false;
                if (any) { const int y = i / W; prot = bg_protected(g, i - y * W, y); }
                bg_adapt_pixel(o, v, prot, nv, sv, dv, rv, cv);
                f[i] = out;
                mn = fminf(mn, out); mx = fmaxf(mx, out);
                if (sv != s0) sn[i] = sv;
                if (__float_as_int(nv) != __float_as_int(n0)) nr[i] = nv;
                if (__float_as_int(dv) != __float_as_int(d0)) cd[i] = dv;
                if (rv != r0) rn[i] = rv;
                if (__float_as_int(cv) != __float_as_int(c0)) c[i] = cv;
            }
        }
    }
    if (partial == nullptr) return;
    if (!block_minmax(mn, mx, s_mn, s_mx)) return;
    partial[((size_t)b * FR_BANDS + band) * 2] = mn;
    partial[((size_t)b * FR_BANDS + band) * 2 + 1] = mx;
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

namespace {

// what both adapting entry points refuse before they look at a buffer: the options (the host's background_spec has checked them too)
bool bg_bad_adapt(const int* take, int T, float margin, float rel, int min_seen, int persist, int guard) {
    const bool finite = fabs((double)margin) <= 3.4e38 && fabs((double)rel) <= 3.4e38;      // false for NaN
    return !take || T < 0 || !finite || min_seen < 1 || persist < 2 || persist < min_seen || guard < 0;
}

}  // namespace

extern "C" int dpp_frame_background_adapt(float* frames, float* cut, float* near_, int* seen, float* cand, int* run, const int* take, int B, int H,
                                          int W, const void* records, int T, const int* src, float margin, float rel, int min_seen, int persist,
                                          int guard, float* partial, dpp_stream_t stream) {
    if (!frames || !cut || !near_ || !seen || !cand || !run || bg_bad_shape(B, H, W)) return DPP_E_BADARG;
    if (bg_bad_adapt(take, T, margin, rel, min_seen, persist, guard)) return DPP_E_BADARG;
    const void* buf[6] = {frames, cut, near_, seen, cand, run};                           // every one is rewritten while others are read
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (bg_overlap(buf[i], buf[j], (size_t)B * H * W, 4, 4)) return DPP_E_BADARG;
    const BgAdapt o = {margin, rel, min_seen, persist, guard};
    DPP_LAUNCH(frame_background_adapt_kernel, dim3(FR_BANDS, B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, cut, near_, seen,
               cand, run, take, H, W, static_cast<const SourceRec*>(nullptr), static_cast<const CropRec*>(records), T, src, o, partial);
    return dpp_launch_status();
}

extern "C" int dpp_frame_background_adapt_src(float* frames, float* cut, float* near_, int* seen, float* cand, int* run, const int* take,
                                              const void* sources, int C, const void* records, int T, const int* src, float margin, float rel,
                                              int min_seen, int persist, int guard, float* partial, dpp_stream_t stream) {
    if (!frames || !cut || !near_ || !seen || !cand || !run || !sources || C < 1 || C > 65535) return DPP_E_BADARG;
    if (bg_bad_adapt(take, T, margin, rel, min_seen, persist, guard)) return DPP_E_BADARG;
    const void* buf[6] = {frames, cut, near_, seen, cand, run};                           // (the host keeps the ragged buffers apart)
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (buf[i] == buf[j]) return DPP_E_BADARG;
    const BgAdapt o = {margin, rel, min_seen, persist, guard};
    DPP_LAUNCH(frame_background_adapt_kernel, dim3(FR_BANDS, C), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, cut, near_, seen,
               cand, run, take, 0, 0, static_cast<const SourceRec*>(sources), static_cast<const CropRec*>(records), T, src, o, partial);
    return dpp_launch_status();
}
