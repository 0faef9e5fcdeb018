// ingest.hip -- a depth frame as a sensor delivers it -> the float32 millimetre frame the tracker and the detector work on, for gfx950.
//
// What the reference's only live depth source does to every frame on the host (src/util/cameradevice.py:189-200 of the reference,
// CreativeCameraDevice.getDepth): an optional mirror ([:, ::-1]), cv2.medianBlur(depth, 3) on the 16-bit map (replicated border),
// the conversion to float32.  One launch does all three AND writes frame_range's per-band (min, max) partials of the frame it
// stores, so in a tracking plan it takes frame_range's place instead of adding a pass over the frame.
//
//   out[b][y][x] = float32( median of the nine src[b][clamp(y + dy, 0, H - 1)][clamp(xs + dx, 0, W - 1)] ),  xs = MIRROR_X ? W - 1 - x : x
//
// A 3x3 median is a selection: no arithmetic rounds here (uint16 -> float32 is exact), so this unit is not on the -ffp-contract=off
// lists of the Makefile although it includes geom.h (for FR_BANDS and block_minmax only).  The mirror commutes with the replicate-
// border median, so the kernel works in SOURCE coordinates and mirrors where it stores.
//
// Shape: grid (FR_BANDS, B) like frame_range_kernel; a workgroup owns the contiguous rows [band * rows, (band + 1) * rows) of one frame
// (rows = ceil(H / FR_BANDS)), so its reduction IS the band's partial.  With the median the band's rows plus one halo row above and
// one below are staged ONCE in LDS (16-byte global loads where the address allows it, scalar loads where not: odd W with uint16
// rows), replicated border included; every thread then takes groups of V = 16 bytes' worth of source pixels of one row: it sorts each of the
// V + 2 columns of three once and shares the sorted columns between the three outputs that use them,
//   median = med3(max of the lows, med3 of the mids, min of the highs),
// compare-and-select exchanges only (no fminf / fmaxf: nothing hangs on the denormal mode).  A band taller or a frame wider than the
// LDS tile is walked in row chunks / column tiles, whose halos are read again.  Without the median there is nothing to stage: one
// group per thread straight from memory.  Source type and flags are template parameters.
//
// Sources of unlike sizes (ABI v19, dpp_frame_ingest_src): the same kernel with the per-source table of geom.h -- workgroup (band, c)
// takes H, W and the element offsets of source c's frame in the ragged raw and float32 buffers from record c; the table pointer is
// null in dpp_frame_ingest, where the launch's H, W hold for all B frames.  The tile is static and sized from the run-time W either way.
#include "geom.h"

namespace {

constexpr int IG_TILE_BYTES = 32768;    // LDS tile of the median path
constexpr int IG_TCMAX = 1024;          // source columns per tile (a multiple of both group widths)
// The pitch P and the rows per staging are derived once from the WIDEST tile (min(W, IG_TCMAX) columns) and used for every column tile
// -- later tiles are only narrower.  At that width the tile must still hold one output row and its two halo rows, for either type:
static_assert(IG_TCMAX % 8 == 0, "a column tile is a whole number of 16-byte groups of either source type");
static_assert(IG_TILE_BYTES / ((IG_TCMAX + 2 * 4) * 4) - 2 >= 1 && IG_TILE_BYTES / ((IG_TCMAX + 2 * 8) * 2) - 2 >= 1,
              "the LDS tile holds fewer than three rows of the widest column tile");

template <class T> struct IgType;
template <> struct IgType<float> { typedef float reg; static constexpr int V = 4; };
template <> struct IgType<uint16_t> { typedef unsigned reg; static constexpr int V = 8; };      // compared as 32-bit unsigned

__device__ __forceinline__ bool ig_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// V consecutive elements at p (global memory or the LDS tile) widened to registers, as ONE 16-byte load: p must be 16-byte aligned
__device__ __forceinline__ void ig_load16(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ig_load16(const uint16_t* p, unsigned (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    v[0] = t.x & 0xffffu; v[1] = t.x >> 16; v[2] = t.y & 0xffffu; v[3] = t.y >> 16;
    v[4] = t.z & 0xffffu; v[5] = t.z >> 16; v[6] = t.w & 0xffffu; v[7] = t.w >> 16;
}

template <class R> __device__ __forceinline__ R ig_min(R a, R b) { return b < a ? b : a; }
template <class R> __device__ __forceinline__ R ig_max(R a, R b) { return b < a ? a : b; }
template <class R> __device__ __forceinline__ void ig_exchange(R& a, R& b) { const R lo = ig_min(a, b), hi = ig_max(a, b); a = lo; b = hi; }
template <class R> __device__ __forceinline__ R ig_med3(R a, R b, R c) { return ig_max(ig_min(a, b), ig_min(ig_max(a, b), c)); }

// n <= V outputs of SOURCE columns c0 .. c0 + n - 1 of one row -> the frame (mirrored: column W - 1 - c) and the running range.
// A full group is one or two 16-byte stores where its first address is aligned.
template <bool MIR, int V>
__device__ __forceinline__ void ig_emit(float* __restrict__ orow, int W, int c0, int n, const float (&o)[V], float& mn, float& mx) {
    if (n == V) {
        float w[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            w[j] = MIR ? o[V - 1 - j] : o[j];
            mn = fminf(mn, o[j]); mx = fmaxf(mx, o[j]);
        }
        float* q = orow + (MIR ? W - V - c0 : c0);
        if (ig_aligned16(q)) {
#pragma unroll
            for (int k = 0; k < V; k += 4) *reinterpret_cast<float4*>(q + k) = make_float4(w[k], w[k + 1], w[k + 2], w[k + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) q[j] = w[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (j < n) {
                orow[MIR ? W - 1 - c0 - j : c0 + j] = o[j];
                mn = fminf(mn, o[j]); mx = fmaxf(mx, o[j]);
            }
        }
    }
}

template <class T, bool MED, bool MIR>
__global__ __launch_bounds__(DPP_THREADS) void frame_ingest_kernel(const T* __restrict__ raw, int H, int W, const SourceRec* __restrict__ tab,
                                                                   float* __restrict__ frames, float* __restrict__ partial) {
    typedef typename IgType<T>::reg R;
    constexpr int V = IgType<T>::V;
    __shared__ float s_mn[DPP_THREADS / DPP_WAVE], s_mx[DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    // tab (null: B equal [H][W] frames): source b's own size and where its frame starts in the ragged raw and float32 buffers
    if (tab) { H = tab[b].H; W = tab[b].W; }
    const T* src = raw + (tab ? (size_t)tab[b].raw_off : (size_t)b * H * W);
    float* dst = frames + (tab ? (size_t)tab[b].frame_off : (size_t)b * H * W);
    const int rows = (H + FR_BANDS - 1) / FR_BANDS;
    const int y0 = band * rows < H ? band * rows : H, y1 = y0 + rows < H ? y0 + rows : H;     // an empty band: y0 == y1
    float mn = 3.4e38f, mx = -3.4e38f;
    if constexpr (!MED) {
        const int ng = (W + V - 1) / V, nit = (y1 - y0) * ng;
        for (int i = tid; i < nit; i += DPP_THREADS) {
            const int r = i / ng, c0 = (i - r * ng) * V, y = y0 + r;
            const int n = W - c0 < V ? W - c0 : V;
            const T* p = src + (size_t)y * W + c0;
            R v[V];
            if (n == V && ig_aligned16(p)) {
                ig_load16(p, v);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) v[j] = j < n ? (R)p[j] : (R)0;
            }
            float o[V];
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = (float)v[j];
            ig_emit<MIR, V>(dst + (size_t)y * W, W, c0, n, o, mn, mx);
        }
    } else {
        // the tile: row rr = source row clamp(ya - 1 + rr), element V - 1 + k = source column clamp(xa - 1 + k), k = 0 .. tc + 1.
        // The pitch is a multiple of V and the interior starts at element V: every full group is 16-byte aligned in LDS.
        __shared__ __attribute__((aligned(16))) unsigned char s_raw[IG_TILE_BYTES];
        T* s = reinterpret_cast<T*>(s_raw);
        const int tcmax = W < IG_TCMAX ? W : IG_TCMAX;
        const int P = (tcmax + V - 1) / V * V + 2 * V;
        const int rchunk = IG_TILE_BYTES / (P * (int)sizeof(T)) - 2;          // output rows per staging (>= 5 at the widest tile)
        for (int xa = 0; xa < W; xa += IG_TCMAX) {
            const int tc = W - xa < IG_TCMAX ? W - xa : IG_TCMAX, ng = (tc + V - 1) / V;
            for (int ya = y0; ya < y1; ya += rchunk) {
                const int nr = y1 - ya < rchunk ? y1 - ya : rchunk;
                const int nst = (nr + 2) * (ng + 1);                          // per tile row: ng groups and the two halo columns
                for (int i = tid; i < nst; i += DPP_THREADS) {
                    const int rr = i / (ng + 1), g = i - rr * (ng + 1);
                    int sy = ya - 1 + rr;
                    sy = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);
                    const T* rp = src + (size_t)sy * W;
                    T* sp = s + rr * P;
                    if (g == ng) {
                        sp[V - 1] = rp[xa > 0 ? xa - 1 : 0];
                        sp[V + tc] = rp[xa + tc < W ? xa + tc : W - 1];
                    } else {
                        const int c = xa + g * V, n = xa + tc - c < V ? xa + tc - c : V;
                        if (n == V && ig_aligned16(rp + c)) {
                            *reinterpret_cast<uint4*>(sp + V + g * V) = *reinterpret_cast<const uint4*>(rp + c);
                        } else {
#pragma unroll
                            for (int j = 0; j < V; ++j) { if (j < n) sp[V + g * V + j] = rp[c + j]; }
                        }
                    }
                }
                __syncthreads();
                const int nit = nr * ng;
                for (int i = tid; i < nit; i += DPP_THREADS) {
                    const int r = i / ng, g = i - r * ng;
                    R lo[V + 2], mi[V + 2], hi[V + 2];
                    {
                        R rowv[3][V];
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const T* sp = s + (r + k) * P + V + g * V;
                            ig_load16(sp, rowv[k]);
                            R a = (R)sp[-1], c = (R)sp[V];
                            if (k == 0) { lo[0] = a; lo[V + 1] = c; } else if (k == 1) { mi[0] = a; mi[V + 1] = c; } else { hi[0] = a; hi[V + 1] = c; }
                        }
#pragma unroll
                        for (int j = 0; j < V; ++j) { lo[j + 1] = rowv[0][j]; mi[j + 1] = rowv[1][j]; hi[j + 1] = rowv[2][j]; }
                    }
#pragma unroll
                    for (int j = 0; j < V + 2; ++j) {                        // each column of three sorted once
                        ig_exchange(lo[j], mi[j]); ig_exchange(mi[j], hi[j]); ig_exchange(lo[j], mi[j]);
                    }
                    float o[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const R a = ig_max(ig_max(lo[j], lo[j + 1]), lo[j + 2]);
                        const R m = ig_med3(mi[j], mi[j + 1], mi[j + 2]);
                        const R z = ig_min(ig_min(hi[j], hi[j + 1]), hi[j + 2]);
                        o[j] = (float)ig_med3(a, m, z);
                    }
                    const int n = tc - g * V < V ? tc - g * V : V;         // (columns past the tile hold stale LDS: computed, never stored)
                    ig_emit<MIR, V>(dst + (size_t)(ya + r) * W, W, xa + g * V, n, o, mn, mx);
                }
                __syncthreads();
            }
        }
    }
    if (partial == nullptr) return;
    if (!block_minmax(mn, mx, s_mn, s_mx)) return;
    partial[((size_t)b * FR_BANDS + band) * 2] = mn;
    partial[((size_t)b * FR_BANDS + band) * 2 + 1] = mx;
}

template <class T>
int ingest_launch(const void* raw, int B, int H, int W, const SourceRec* tab, int flags, float* frames, float* partial, hipStream_t st) {
    const T* r = static_cast<const T*>(raw);
    const dim3 grid(FR_BANDS, B), block(DPP_THREADS);
    switch (flags) {
    case 0: DPP_LAUNCH((frame_ingest_kernel<T, false, false>), grid, block, 0, st, r, H, W, tab, frames, partial); break;
    case DPP_INGEST_MEDIAN3: DPP_LAUNCH((frame_ingest_kernel<T, true, false>), grid, block, 0, st, r, H, W, tab, frames, partial); break;
    case DPP_INGEST_MIRROR_X: DPP_LAUNCH((frame_ingest_kernel<T, false, true>), grid, block, 0, st, r, H, W, tab, frames, partial); break;
    default: DPP_LAUNCH((frame_ingest_kernel<T, true, true>), grid, block, 0, st, r, H, W, tab, frames, partial); break;
    }
    return dpp_launch_status();
}

}  // namespace

extern "C" int dpp_frame_ingest(const void* raw, int src_type, int B, int H, int W, int flags, float* frames, float* partial,
                                dpp_stream_t stream) {
    if (!raw || !frames || B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return DPP_E_BADARG;
    if ((src_type != DPP_INGEST_U16 && src_type != DPP_INGEST_F32) || (flags & ~(DPP_INGEST_MEDIAN3 | DPP_INGEST_MIRROR_X))) return DPP_E_BADARG;
    const size_t npx = (size_t)B * H * W, esz = src_type == DPP_INGEST_U16 ? 2 : 4;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(raw), a1 = a0 + npx * esz;
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(frames), f1 = f0 + npx * 4;
    if (a0 < f1 && f0 < a1) return DPP_E_BADARG;                       // every output pixel reads neighbours other workgroups write
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (src_type == DPP_INGEST_U16) return ingest_launch<uint16_t>(raw, B, H, W, nullptr, flags, frames, partial, st);
    return ingest_launch<float>(raw, B, H, W, nullptr, flags, frames, partial, st);
}

// C sources of unlike sizes (ABI v19): source c is sources[c].H x sources[c].W, read at element sources[c].raw_off of `raw` and stored at
// element sources[c].frame_off of `frames`; band b of source c covers ceil(H_c / FR_BANDS) rows of that source.  The host has validated
// the table (sizes, offsets in range and 16-byte aligned, the two buffers apart); only what needs no device memory is checked here.
extern "C" int dpp_frame_ingest_src(const void* raw, int src_type, const void* sources, int C, int flags, float* frames, float* partial,
                                    dpp_stream_t stream) {
    if (!raw || !frames || !sources || raw == static_cast<const void*>(frames) || C < 1 || C > 65535) return DPP_E_BADARG;
    if ((src_type != DPP_INGEST_U16 && src_type != DPP_INGEST_F32) || (flags & ~(DPP_INGEST_MEDIAN3 | DPP_INGEST_MIRROR_X))) return DPP_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SourceRec* tab = static_cast<const SourceRec*>(sources);
    if (src_type == DPP_INGEST_U16) return ingest_launch<uint16_t>(raw, C, 0, 0, tab, flags, frames, partial, st);
    return ingest_launch<float>(raw, C, 0, 0, tab, flags, frames, partial, st);
}
