// components.hip -- finding the hand in a whole depth frame by 8-connected component labelling, for gfx950 (ABI v14, several hands: v17):
//   slab keys        slab_keys: the 20 depth slabs of HandDetector.detect (handdetector.py:576-582) as one uint8 key per pixel
//   labelling        cc_local / cc_border / cc_compress: labels[p] = smallest linear index of p's 8-connected component of equal key
//   statistics       cc_stats: per component pixel count, bounding box and coordinate sums (integer atomics only)
//   the seed         comp_select + detect_seed: the nearest slab's raster-first component of more than 200 px, the centre of mass of
//                    the +-100 px window around its centroid within that slab (handdetector.py:586-607) -> refine_com_iterative
//   several hands    comp_candidates + detect_select + detect_seeds: up to K seeds of one frame from the same labelling
//   hand size        mask_keys -> labelling -> comp_select -> hand_size: estimateHandsize (handdetector.py:911-937) from the bounding
//                    box of the largest component of the hand's depth range (:616-627)
// Where the reference walks cv2.findContours' contour list, this unit labels components: pixel count for contourArea, raster order
// for contour order, and a depth exactly on a slab boundary belongs to the nearer slab only.  Everything else restates the
// reference's NumPy arithmetic, which rounds after every operation: compiled with -ffp-contract=off like crop.hip.
//
// The labelling is a lock-free union-find over parent[] (Playne & Hawick style): a link only ever goes from a larger index to a smaller
// one of the SAME component and a parent is only ever lowered (an atomic minimum), so parent[i] <= i at all times, every walk ends,
// and a walk that reads an OLDER parent (another XCD's L2 has a newer one) still ends at a pixel of its component -- the atomic
// that follows returns the word's true value and the union loop carries on from it.  Stale loads cost iterations, never results.
// parent[] is held complemented (q = ~parent, background: parent = -1, q = 0), so that the minimum is an atomicMax.
#include "geom.h"

namespace {

constexpr int CC_TW = 32, CC_TH = 32;                  // labelling tile (one workgroup, four pixels per thread)
constexpr int CC_TILE = CC_TW * CC_TH;
constexpr unsigned char CC_BG = 255;                   // background key
constexpr int CC_SLABS = 20;                           // detect's `steps`
constexpr int CC_MIN_AREA = 200;                       // detect's contourArea threshold, here in pixels
constexpr int DET_FOUND = 1, DET_NO_SIZE = 2;          // status bits (DPP_DETECT_*)

struct CompStat {                                      // the statistics of the component whose root is this pixel; 40 bytes
    int cnt, ixmin, xmax, iymin, ymax, pad;            // ixmin = ~xmin, iymin = ~ymin (minimum as an atomicMax)
    unsigned long long sx, sy;
};

// ---- union-find on a complemented parent array (global memory or LDS) ------------------------------------------------------------
__device__ __forceinline__ int cc_find(const int* q, int i) {
    int p = ~q[i];
    while (p != i) { i = p; p = ~q[i]; }
    return i;
}

__device__ __forceinline__ void cc_union(int* q, int a, int b) {
    for (;;) {
        a = cc_find(q, a);
        b = cc_find(q, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = ~atomicMax(&q[a], ~b);         // parent[a] = min(parent[a], b)
        if (old == a) return;                          // a was a root: linked
        a = old;                                       // a had a parent already, which b may just have replaced: join that one with b
    }
}

// bound i of the 21 slab bounds: minDepth + i * (maxDepth - minDepth) / 20 in float64 from the float32 range (handdetector.py:577-581)
__device__ __forceinline__ double slab_bound(float min_depth, float max_depth, int i) {
    return (double)min_depth + (double)i * ((double)max_depth - (double)min_depth) / (double)CC_SLABS;
}

// ---- keys ------------------------------------------------------------------------------------------------------------------------
// key = the smallest i with b_i <= d <= b_{i+1}; background for d == 0 and outside the detector's range.  An all-zero frame has the
// inverted range (10, 0): every pixel fails the range test.  Also clears the frame's seed selection word.
__global__ __launch_bounds__(DPP_THREADS) void slab_keys_kernel(const float* __restrict__ frames, int H, int W, const float* __restrict__ partial,
                                                                unsigned char* __restrict__ keys, unsigned long long* __restrict__ best) {
    __shared__ double s_b[CC_SLABS + 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    float mn, mx;
    frame_range_reduce(partial, b, tid & 63, mn, mx);
    const float min_depth = fmaxf(10.0f, mn), max_depth = fminf(1500.0f, mx);
    if (tid <= CC_SLABS) s_b[tid] = slab_bound(min_depth, max_depth, tid);
    if (blockIdx.x == 0 && tid == 0) best[b * 2] = 0ull;
    __syncthreads();
    const int p = blockIdx.x * DPP_THREADS + tid;
    if (p >= H * W) return;
    const float d = frames[(size_t)b * H * W + p];
    unsigned char key = CC_BG;
    if (d != 0.0f && d >= min_depth && d <= max_depth) {
        const double dd = (double)d;
        for (int i = 0; i < CC_SLABS; ++i)
            if (s_b[i] <= dd && dd <= s_b[i + 1]) { key = (unsigned char)i; break; }
    }
    keys[(size_t)b * H * W + p] = key;
}

// The hand's depth range as a binary key (handdetector.py:616-619): d != 0 && zlo <= d <= zhi, zlo / zhi = com_z -+ cube_z / 2 in
// float64 from the float32 centre, over the raw frame.  Also clears the frame's hand-size selection word.
__global__ __launch_bounds__(DPP_THREADS) void mask_keys_kernel(const float* __restrict__ frames, int H, int W, const float* __restrict__ com,
                                                                const float* __restrict__ cube, unsigned char* __restrict__ keys,
                                                                unsigned long long* __restrict__ best) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) best[b * 2 + 1] = 0ull;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const double zlo = (double)com[b * 3 + 2] - (double)cube[b * 3 + 2] / 2., zhi = (double)com[b * 3 + 2] + (double)cube[b * 3 + 2] / 2.;
    const float d = frames[(size_t)b * H * W + p];
    keys[(size_t)b * H * W + p] = (d != 0.0f && zlo <= (double)d && (double)d <= zhi) ? (unsigned char)0 : CC_BG;
}

// ---- labelling -------------------------------------------------------------------------------------------------------------------
// One 32 x 32 tile per workgroup, labelled in LDS: every pixel is joined with its W / NW / N / NE neighbours of equal key inside
// the tile, then points at its tile-local root in global memory.  Local raster order is global raster order, so the local minimum
// is the tile's smallest linear index: parent[i] <= i holds from the start.
__global__ __launch_bounds__(DPP_THREADS) void cc_local_kernel(const unsigned char* __restrict__ keys, int H, int W, int* __restrict__ q) {
    __shared__ int s_q[CC_TILE];
    __shared__ unsigned char s_k[CC_TILE];
    const int b = blockIdx.z, x0 = blockIdx.x * CC_TW, y0 = blockIdx.y * CC_TH, tid = threadIdx.x;
    const unsigned char* k = keys + (size_t)b * H * W;
    int* qb = q + (size_t)b * H * W;
    for (int l = tid; l < CC_TILE; l += DPP_THREADS) {
        const int x = x0 + (l & (CC_TW - 1)), y = y0 + l / CC_TW;
        const unsigned char kv = (x < W && y < H) ? k[(size_t)y * W + x] : CC_BG;
        s_k[l] = kv;
        s_q[l] = kv == CC_BG ? 0 : ~l;
    }
    __syncthreads();
    for (int l = tid; l < CC_TILE; l += DPP_THREADS) {
        const int lx = l & (CC_TW - 1), ly = l / CC_TW;
        const unsigned char kv = s_k[l];
        if (kv == CC_BG) continue;
        if (lx > 0 && s_k[l - 1] == kv) cc_union(s_q, l, l - 1);
        if (ly > 0) {
            if (lx > 0 && s_k[l - CC_TW - 1] == kv) cc_union(s_q, l, l - CC_TW - 1);
            if (s_k[l - CC_TW] == kv) cc_union(s_q, l, l - CC_TW);
            if (lx < CC_TW - 1 && s_k[l - CC_TW + 1] == kv) cc_union(s_q, l, l - CC_TW + 1);
        }
    }
    __syncthreads();
    for (int l = tid; l < CC_TILE; l += DPP_THREADS) {
        const int x = x0 + (l & (CC_TW - 1)), y = y0 + l / CC_TW;
        if (x >= W || y >= H) continue;
        int v = 0;
        if (s_k[l] != CC_BG) {
            const int r = cc_find(s_q, l);
            v = ~((y0 + r / CC_TW) * W + x0 + (r & (CC_TW - 1)));
        }
        qb[(size_t)y * W + x] = v;
    }
}

// The joins that cross a tile border, in a launch of their own: the pixels of a tile's top row and of its left and right columns
// against those of their W / NW / N / NE neighbours that lie in another tile.  (A pair met twice is joined twice: harmless.)
__global__ __launch_bounds__(128) void cc_border_kernel(const unsigned char* __restrict__ keys, int H, int W, int* __restrict__ q) {
    const int b = blockIdx.z, t = threadIdx.x;
    if (t >= 3 * CC_TW) return;
    const int lx = t < CC_TW ? t : (t < 2 * CC_TW ? 0 : CC_TW - 1), ly = t < CC_TW ? 0 : (t & (CC_TW - 1));
    const int x = blockIdx.x * CC_TW + lx, y = blockIdx.y * CC_TH + ly;
    if (x >= W || y >= H) return;
    const unsigned char* k = keys + (size_t)b * H * W;
    int* qb = q + (size_t)b * H * W;
    const unsigned char kv = k[(size_t)y * W + x];
    if (kv == CC_BG) return;
    const int dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
    for (int n = 0; n < 4; ++n) {
        const int nx = x + dx[n], ny = y + dy[n];
        if (nx < 0 || nx >= W || ny < 0) continue;
        if (nx / CC_TW == x / CC_TW && ny / CC_TH == y / CC_TH) continue;
        if (k[(size_t)ny * W + nx] == kv) cc_union(qb, y * W + x, ny * W + nx);
    }
}

// labels = root of every pixel (-1: background); a root's statistics record is cleared here, for cc_stats_kernel to add to
__global__ __launch_bounds__(DPP_THREADS) void cc_compress_kernel(const int* __restrict__ q, int H, int W, int* __restrict__ labels,
                                                                  CompStat* __restrict__ stats) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const int* qb = q + (size_t)b * H * W;
    const int r = qb[p] == 0 ? -1 : cc_find(qb, p);
    labels[(size_t)b * H * W + p] = r;
    if (r == p && stats) {
        CompStat s;
        s.cnt = 0; s.ixmin = ~0x7fffffff; s.xmax = 0; s.iymin = ~0x7fffffff; s.ymax = 0; s.pad = 0; s.sx = 0ull; s.sy = 0ull;
        stats[(size_t)b * H * W + p] = s;
    }
}

// Statistics per root.  A wave holds 64 consecutive pixels; a run of equal labels inside one image row is aggregated in the wave
// (its head lane from a segmented scan, count and coordinate sum from the run's two ends) and its last lane issues the atomics.
__global__ __launch_bounds__(DPP_THREADS) void cc_stats_kernel(const int* __restrict__ labels, int H, int W, CompStat* __restrict__ stats) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    const int r = p < H * W ? labels[(size_t)b * H * W + p] : -1;
    const int y = p / W, x = p - y * W;
    const int prev = __shfl_up(r, 1), next = __shfl_down(r, 1);
    const bool head = r >= 0 && (lane == 0 || x == 0 || prev != r);
    const bool tail = r >= 0 && (lane == 63 || x == W - 1 || next != r);
    int h = head ? lane : -1;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(h, o);
        if (lane >= o && t > h) h = t;
    }
    if (!tail) return;
    const int n = lane - h + 1, x0 = x - n + 1;
    CompStat* s = stats + (size_t)b * H * W + r;
    atomicAdd(&s->cnt, n);
    atomicMax(&s->ixmin, ~x0);
    atomicMax(&s->xmax, x);
    atomicMax(&s->iymin, ~y);
    atomicMax(&s->ymax, y);
    atomicAdd(&s->sx, (unsigned long long)(x0 + x) * (unsigned long long)n / 2ull);
    atomicAdd(&s->sy, (unsigned long long)y * (unsigned long long)n);
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
// The winning root of frame b as one 64-bit maximum, best[b][mode] (0: none):
//   mode 0  components of more than 200 px: smallest key, then smallest root   (255 - key) << 32 | ~root
//   mode 1  largest pixel count, then smallest root                           count << 32 | ~root
// One atomic per wave that holds a candidate.
__global__ __launch_bounds__(DPP_THREADS) void comp_select_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ keys,
                                                                  const CompStat* __restrict__ stats, int H, int W, int mode,
                                                                  unsigned long long* __restrict__ best) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    unsigned long long v = 0ull;
    if (p < H * W && labels[(size_t)b * H * W + p] == p) {
        const int cnt = stats[(size_t)b * H * W + p].cnt;
        const unsigned long long lo = 0xffffffffull - (unsigned long long)p;
        if (mode == 0) { if (cnt > CC_MIN_AREA) v = ((unsigned long long)(255 - keys[(size_t)b * H * W + p]) << 32) | lo; }
        else if (cnt > 0) v = ((unsigned long long)cnt << 32) | lo;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    if ((threadIdx.x & 63) == 0 && v != 0ull) atomicMax(&best[b * 2 + mode], v);
}

__device__ __forceinline__ int select_root(unsigned long long v) { return (int)(0xffffffffull - (v & 0xffffffffull)); }

// detect's seed from one component (handdetector.py:589-607), one workgroup: the centroid of the component (rint of the float64
// quotient), the window [max(cx - 100, 0), min(cx + 100, W - 1)) x [max(cy - 100, 0), min(cy + 100, H - 1)), calculateCoM of the
// window's pixels inside the component's slab's inclusive bounds (float64 sums of integers and of float32 millimetres: exact, the
// order is free; the mean as NumPy forms it: sum / num * num / num), the centre-pixel fallback, the window origin added.  Thread 0
// stores com_out[0..2] and *status.  The ONE body of detect_seed_kernel (one winner per frame) and detect_seeds_kernel (K per frame).
__device__ __forceinline__ int seed_centroid(unsigned long long sum, int cnt) { return (int)rint((double)sum / (double)cnt); }
__device__ __forceinline__ int seed_window_lo(int c) { return c - 100 > 0 ? c - 100 : 0; }
__device__ __forceinline__ int seed_window_hi(int c, int n) { return c + 100 < n - 1 ? c + 100 : n - 1; }

__device__ __forceinline__ void detect_seed_body(const float* __restrict__ f, int H, int W, float min_depth, float max_depth, int key,
                                                 const CompStat& st, double (*s_red)[DPP_THREADS / DPP_WAVE], float* __restrict__ com_out,
                                                 int* __restrict__ status) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cx = seed_centroid(st.sx, st.cnt), cy = seed_centroid(st.sy, st.cnt);
    const int xs = seed_window_lo(cx), xe = seed_window_hi(cx, W);
    const int ys = seed_window_lo(cy), ye = seed_window_hi(cy, H);
    const double lo = slab_bound(min_depth, max_depth, key), hi = slab_bound(min_depth, max_depth, key + 1);
    // the window's value at frame pixel (x, y): the detector's range, then the slab
    auto value = [&](int x, int y) {
        const float d = f[(size_t)y * W + x];
        return (d >= min_depth && d <= max_depth && lo <= (double)d && (double)d <= hi) ? d : 0.0f;
    };
    double sx = 0.0, sy = 0.0, sd = 0.0, cnt = 0.0;
    for (int y = ys + wave; y < ye; y += DPP_THREADS / DPP_WAVE) {
        double rs = 0.0, rc = 0.0, rx = 0.0;
        for (int x = xs + lane; x < xe; x += DPP_WAVE) {
            const float d = value(x, y);
            if (d > 0.0f) { rx += (double)(x - xs); rs += (double)d; rc += 1.0; }
        }
        sx += rx; sd += rs; cnt += rc; sy += rc * (double)(y - ys);
    }
    if (!com_block_sums(sx, sy, sd, cnt, s_red)) return;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (cnt > 0.0) { c0 = sx / cnt * cnt / cnt; c1 = sy / cnt * cnt / cnt; c2 = sd / cnt; }
    if (fabs(c0) <= 1e-8 && fabs(c1) <= 1e-8 && fabs(c2) <= 1e-8 && xe > xs && ye > ys)       // numpy.allclose(com, 0.)
        c2 = (double)value(xs + (xe - xs) / 2, ys + (ye - ys) / 2);
    com_out[0] = (float)(c0 + (double)xs);
    com_out[1] = (float)(c1 + (double)ys);
    com_out[2] = (float)c2;
    *status = DET_FOUND;
}

// detect's seed for frame b from the component comp_select (mode 0) chose.  No component: com = (0, 0, 0) (:632) and status 0.
__global__ __launch_bounds__(DPP_THREADS) void detect_seed_kernel(const float* __restrict__ frames, int H, int W, const float* __restrict__ partial,
                                                                  const CompStat* __restrict__ stats, const unsigned long long* __restrict__ best,
                                                                  float* __restrict__ com_out, int* __restrict__ status) {
    __shared__ double s_red[4][DPP_THREADS / DPP_WAVE];
    const int b = blockIdx.x, tid = threadIdx.x;
    float mn, mx;
    frame_range_reduce(partial, b, tid & 63, mn, mx);
    const unsigned long long v = best[b * 2];
    if (v == 0ull) {
        if (tid == 0) { com_out[b * 3] = 0.f; com_out[b * 3 + 1] = 0.f; com_out[b * 3 + 2] = 0.f; status[b] = 0; }
        return;
    }
    const CompStat st = stats[(size_t)b * H * W + select_root(v)];
    detect_seed_body(frames + (size_t)b * H * W, H, W, fmaxf(10.0f, mn), fminf(1500.0f, mx), 255 - (int)(v >> 32), st, s_red, com_out + b * 3,
                     status + b);
}

// ---- several hands of one frame (ABI v17) ----------------------------------------------------------------------------------------
// comp_candidates -> detect_select -> detect_seeds: up to K seeds per frame from the labelling that detect_seed takes one from.
//   candidates   every root of more than 200 px (that passes the extent filter), in (key, root) order
//   selection    greedy: a candidate whose centroid lies in the seed window of an ACCEPTED one is suppressed; K acceptances
// The extent filter and the window suppression are this project's own rules.
constexpr int DET_MAX_HANDS = 16;
constexpr unsigned long long DET_NONE = ~0ull;

// candidates per frame: components of more than 200 px are disjoint, so there are at most H * W / 201 of them
__host__ __device__ __forceinline__ int cand_capacity(int H, int W) { return (int)((long long)H * W / (CC_MIN_AREA + 1)); }
// a frame's part of the candidate workspace, in 64-bit words: the list, the centroids of its entries, the selection
__host__ __device__ __forceinline__ size_t cand_stride(int H, int W) { return 2 * (size_t)cand_capacity(H, W) + DET_MAX_HANDS; }

// One word key << 32 | root per candidate root, and its centroid cy << 32 | cx beside it, appended through the frame's counter
// (best[b][0], which slab_keys cleared): the wave counts its candidates (an inclusive scan over the lanes) and its last lane
// draws the wave's range with ONE atomic.  The list's order is that of arrival; detect_select's result does not depend on it.
// Extent filter (max_extent > 0): a component whose box is wider or higher than max_extent mm at its slab's far bound is no
// candidate: (xmax - xmin + 1) * b_{key+1} / fx > max_extent, float64 in that order, likewise in y.
__global__ __launch_bounds__(DPP_THREADS) void comp_candidates_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ keys,
                                                                      const CompStat* __restrict__ stats, int H, int W,
                                                                      const float* __restrict__ partial, double max_extent, double fx, double fy,
                                                                      unsigned long long* __restrict__ best, unsigned long long* __restrict__ cand) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    const int cap = cand_capacity(H, W);
    float min_depth = 0.0f, max_depth = 0.0f;
    if (max_extent > 0.0) {                                                    // uniform: the whole wave reduces the range
        float mn, mx;
        frame_range_reduce(partial, b, lane, mn, mx);
        min_depth = fmaxf(10.0f, mn); max_depth = fminf(1500.0f, mx);
    }
    unsigned long long word = 0ull, cen = 0ull;
    int is_cand = 0;
    if (p < H * W && labels[(size_t)b * H * W + p] == p) {
        const CompStat st = stats[(size_t)b * H * W + p];
        if (st.cnt > CC_MIN_AREA) {
            const int key = keys[(size_t)b * H * W + p];
            is_cand = 1;
            if (max_extent > 0.0) {
                const double hi = slab_bound(min_depth, max_depth, key + 1);
                const double ex = (double)(st.xmax - ~st.ixmin + 1) * hi / fx, ey = (double)(st.ymax - ~st.iymin + 1) * hi / fy;
                if (ex > max_extent || ey > max_extent) is_cand = 0;
            }
            word = ((unsigned long long)key << 32) | (unsigned long long)p;
            cen = ((unsigned long long)seed_centroid(st.sy, st.cnt) << 32) | (unsigned long long)seed_centroid(st.sx, st.cnt);
        }
    }
    int scan = is_cand;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(scan, o);
        if (lane >= o) scan += t;
    }
    const int total = __shfl(scan, 63);
    if (total == 0) return;
    int base = 0;
    if (lane == 63) base = (int)atomicAdd(&best[b * 2], (unsigned long long)total);
    base = __shfl(base, 63);
    const int i = base + scan - 1;
    if (is_cand && i < cap) {                                                  // (i < cap always: see cand_capacity)
        unsigned long long* c = cand + (size_t)b * cand_stride(H, W);
        c[i] = word;
        c[cap + i] = cen;
    }
}

// Greedy selection for frame b, one workgroup, K rounds: the smallest word above the last accepted one whose centroid lies in no
// accepted window (a block minimum over the list, in whatever order it is; threads stride over it) is accepted and its window
// recorded.  Walking by a lower bound needs no marks: everything below the bound was accepted or suppressed, and suppressed
// candidates suppress nothing.  sel[k] = the k-th accepted word, DET_NONE from the first round that finds none.
__global__ __launch_bounds__(DPP_THREADS) void detect_select_kernel(const unsigned long long* __restrict__ best, int H, int W, int K,
                                                                    unsigned long long* __restrict__ cand) {
    __shared__ unsigned long long s_w[DPP_THREADS / DPP_WAVE], s_c[DPP_THREADS / DPP_WAVE];
    __shared__ int s_win[DET_MAX_HANDS][4];
    __shared__ unsigned long long s_bound;                                     // words below it are done; DET_NONE: no candidate left
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = cand_capacity(H, W);
    const unsigned long long count = best[b * 2];
    const int n = count < (unsigned long long)cap ? (int)count : cap;
    const unsigned long long* list = cand + (size_t)b * cand_stride(H, W);
    const unsigned long long* cens = list + cap;
    unsigned long long* sel = cand + (size_t)b * cand_stride(H, W) + 2 * (size_t)cap;
    unsigned long long bound = 0ull;
    for (int k = 0; k < K; ++k) {
        unsigned long long m = DET_NONE, mc = 0ull;
        if (bound != DET_NONE) {
            for (int i = tid; i < n; i += DPP_THREADS) {
                const unsigned long long w = list[i];
                if (w < bound || w >= m) continue;
                const unsigned long long c = cens[i];
                const int cx = (int)(c & 0xffffffffull), cy = (int)(c >> 32);
                bool free_ = true;
                for (int a = 0; a < k; ++a)
                    if (s_win[a][0] <= cx && cx < s_win[a][1] && s_win[a][2] <= cy && cy < s_win[a][3]) free_ = false;
                if (free_) { m = w; mc = c; }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long tw = __shfl_xor(m, o), tc = __shfl_xor(mc, o);
            if (tw < m) { m = tw; mc = tc; }
        }
        if (lane == 0) { s_w[wave] = m; s_c[wave] = mc; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < DPP_THREADS / DPP_WAVE; ++w)
                if (s_w[w] < m) { m = s_w[w]; mc = s_c[w]; }
            sel[k] = m;
            if (m != DET_NONE) {
                const int cx = (int)(mc & 0xffffffffull), cy = (int)(mc >> 32);
                s_win[k][0] = seed_window_lo(cx); s_win[k][1] = seed_window_hi(cx, W);
                s_win[k][2] = seed_window_lo(cy); s_win[k][3] = seed_window_hi(cy, H);
            }
            s_bound = m == DET_NONE ? DET_NONE : m + 1ull;
        }
        __syncthreads();
        bound = s_bound;
    }
}

// The seed of slot k of frame b (row b * K + k) from its accepted component, and the slot's report: key, pixel count, xmin, xmax,
// ymin, ymax.  An empty slot: seed (0, 0, 0), status 0, an all-zero report.
__global__ __launch_bounds__(DPP_THREADS) void detect_seeds_kernel(const float* __restrict__ frames, int H, int W, const float* __restrict__ partial,
                                                                   const CompStat* __restrict__ stats, const unsigned long long* __restrict__ cand,
                                                                   int K, float* __restrict__ com_out, int* __restrict__ status,
                                                                   int* __restrict__ report) {
    __shared__ double s_red[4][DPP_THREADS / DPP_WAVE];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, row = b * K + k;
    float mn, mx;
    frame_range_reduce(partial, b, tid & 63, mn, mx);
    const unsigned long long v = cand[(size_t)b * cand_stride(H, W) + 2 * (size_t)cand_capacity(H, W) + k];
    if (v == DET_NONE) {
        if (tid == 0) {
            com_out[row * 3] = 0.f; com_out[row * 3 + 1] = 0.f; com_out[row * 3 + 2] = 0.f; status[row] = 0;
            for (int j = 0; j < 6; ++j) report[row * 6 + j] = 0;
        }
        return;
    }
    const int key = (int)(v >> 32);
    const CompStat st = stats[(size_t)b * H * W + (int)(v & 0xffffffffull)];
    if (tid == 0) {
        int* r = report + row * 6;
        r[0] = key; r[1] = st.cnt; r[2] = ~st.ixmin; r[3] = st.xmax; r[4] = ~st.iymin; r[5] = st.ymax;
    }
    detect_seed_body(frames + (size_t)b * H * W, H, W, fmaxf(10.0f, mn), fminf(1500.0f, mx), key, st, s_red, com_out + row * 3, status + row);
}

// estimateHandsize (handdetector.py:920-935) from the bounding box of the selected (largest) component: w = xmax - xmin + 1 and
// h = ymax - ymin + 1 are cv2.boundingRect of its outer contour; float64 in the reference's operation order on the float32 centre,
// stored as float32.  A frame without a hand (status bit 0 clear) or with an empty mask keeps its cube; the latter sets status bit 1.
__global__ __launch_bounds__(DPP_WAVE) void hand_size_kernel(const CompStat* __restrict__ stats, const unsigned long long* __restrict__ best, int B,
                                                             int H, int W, const float* __restrict__ com, const float* __restrict__ cube_in,
                                                             double fx, double fy, double tol, float* __restrict__ cube_out,
                                                             int* __restrict__ status) {
    const int b = blockIdx.x * DPP_WAVE + threadIdx.x;
    if (b >= B) return;
    float cube[3] = {cube_in[b * 3], cube_in[b * 3 + 1], cube_in[b * 3 + 2]};
    const int st = status[b];
    const unsigned long long v = best[b * 2 + 1];
    if (st & DET_FOUND) {
        if (v == 0ull) {
            status[b] = st | DET_NO_SIZE;
        } else {
            const CompStat s = stats[(size_t)b * H * W + select_root(v)];
            const int w = s.xmax - ~s.ixmin + 1, h = s.ymax - ~s.iymin + 1;
            const double c0 = (double)com[b * 3], c1 = (double)com[b * 3 + 1], c2 = (double)com[b * 3 + 2];
            const double xstart = (c0 - (double)w / 2.) * c2 / fx, xend = (c0 + (double)w / 2.) * c2 / fx;
            const double ystart = (c1 - (double)h / 2.) * c2 / fy, yend = (c1 + (double)h / 2.) * c2 / fy;
            const double szx = xend - xstart, szy = yend - ystart;
            const double sz = (szx + szy) / 2.;
            cube[0] = cube[1] = cube[2] = (float)(sz + tol);
        }
    }
    for (int d = 0; d < 3; ++d) cube_out[b * 3 + d] = cube[d];
}

// sizes this unit can index: a frame's linear pixel index is an int, the batch and the rows of tiles are grid dimensions
bool cc_dims_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && H <= 65535 * CC_TH && W >= 1 && (long long)H * W <= 0x7fffffffLL - DPP_THREADS;
}

void cc_label_launches(const unsigned char* keys, int B, int H, int W, int* q, int* labels, CompStat* stats, hipStream_t st) {
    const dim3 tiles(dpp_cdiv(W, CC_TW), dpp_cdiv(H, CC_TH), B), px(dpp_cdiv(H * W, DPP_THREADS), B);
    DPP_LAUNCH(cc_local_kernel, tiles, dim3(DPP_THREADS), 0, st, keys, H, W, q);
    DPP_LAUNCH(cc_border_kernel, tiles, dim3(128), 0, st, keys, H, W, q);
    DPP_LAUNCH(cc_compress_kernel, px, dim3(DPP_THREADS), 0, st, static_cast<const int*>(q), H, W, labels, stats);
    if (stats) DPP_LAUNCH(cc_stats_kernel, px, dim3(DPP_THREADS), 0, st, static_cast<const int*>(labels), H, W, stats);
}

}  // namespace

extern "C" size_t dpp_label_workspace_bytes(int B, int H, int W) { return cc_dims_ok(B, H, W) ? (size_t)B * H * W * sizeof(int) : 0; }
extern "C" size_t dpp_component_stats_bytes(int B, int H, int W) { return cc_dims_ok(B, H, W) ? (size_t)B * H * W * sizeof(CompStat) : 0; }
extern "C" size_t dpp_detect_state_bytes(int B) { return (size_t)(B > 0 ? B : 0) * 2 * sizeof(unsigned long long); }

extern "C" int dpp_slab_keys(const float* frames, const float* partial, int B, int H, int W, unsigned char* keys, void* state,
                             dpp_stream_t stream) {
    if (!frames || !partial || !keys || !state || !cc_dims_ok(B, H, W)) return DPP_E_BADARG;
    DPP_LAUNCH(slab_keys_kernel, dim3(dpp_cdiv(H * W, DPP_THREADS), B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W,
               partial, keys, static_cast<unsigned long long*>(state));
    return dpp_launch_status();
}

extern "C" int dpp_mask_keys(const float* frames, int B, int H, int W, const float* com, const float* cube, unsigned char* keys, void* state,
                             dpp_stream_t stream) {
    if (!frames || !com || !cube || !keys || !state || !cc_dims_ok(B, H, W)) return DPP_E_BADARG;
    DPP_LAUNCH(mask_keys_kernel, dim3(dpp_cdiv(H * W, DPP_THREADS), B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), frames, H, W,
               com, cube, keys, static_cast<unsigned long long*>(state));
    return dpp_launch_status();
}

extern "C" int dpp_label_components(const unsigned char* keys, int B, int H, int W, void* workspace, int* labels, void* stats,
                                    dpp_stream_t stream) {
    if (!keys || !workspace || !labels || !cc_dims_ok(B, H, W)) return DPP_E_BADARG;
    cc_label_launches(keys, B, H, W, static_cast<int*>(workspace), labels, static_cast<CompStat*>(stats), static_cast<hipStream_t>(stream));
    return dpp_launch_status();
}

extern "C" int dpp_detect_seed(const float* frames, const float* partial, const unsigned char* keys, const int* labels, const void* stats, int B,
                               int H, int W, void* state, float* com_out, int* status, dpp_stream_t stream) {
    if (!frames || !partial || !keys || !labels || !stats || !state || !com_out || !status || !cc_dims_ok(B, H, W)) return DPP_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DPP_LAUNCH(comp_select_kernel, dim3(dpp_cdiv(H * W, DPP_THREADS), B), dim3(DPP_THREADS), 0, st, labels, keys, static_cast<const CompStat*>(stats),
               H, W, 0, static_cast<unsigned long long*>(state));
    DPP_LAUNCH(detect_seed_kernel, dim3(B), dim3(DPP_THREADS), 0, st, frames, H, W, partial, static_cast<const CompStat*>(stats),
               static_cast<const unsigned long long*>(state), com_out, status);
    return dpp_launch_status();
}

extern "C" size_t dpp_detect_candidates_bytes(int B, int H, int W) {
    return cc_dims_ok(B, H, W) ? (size_t)B * cand_stride(H, W) * sizeof(unsigned long long) : 0;
}

extern "C" int dpp_detect_seeds(const float* frames, const float* partial, const unsigned char* keys, const int* labels, const void* stats, int B,
                                int H, int W, void* state, void* candidates, int K, double max_extent, double fx, double fy, float* seed_out,
                                int* status, int* report, dpp_stream_t stream) {
    if (!frames || !partial || !keys || !labels || !stats || !state || !candidates || !seed_out || !status || !report || !cc_dims_ok(B, H, W))
        return DPP_E_BADARG;
    if (K < 1 || K > DET_MAX_HANDS || !(max_extent >= 0.0) || !(max_extent <= 1.7976931348623157e308)) return DPP_E_BADARG;
    if (max_extent > 0.0 && !(fabs(fx) > 0.0 && fabs(fy) > 0.0)) return DPP_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* cand = static_cast<unsigned long long*>(candidates);
    DPP_LAUNCH(comp_candidates_kernel, dim3(dpp_cdiv(H * W, DPP_THREADS), B), dim3(DPP_THREADS), 0, st, labels, keys,
               static_cast<const CompStat*>(stats), H, W, partial, max_extent, fabs(fx), fabs(fy), static_cast<unsigned long long*>(state), cand);
    DPP_LAUNCH(detect_select_kernel, dim3(B), dim3(DPP_THREADS), 0, st, static_cast<const unsigned long long*>(state), H, W, K, cand);
    DPP_LAUNCH(detect_seeds_kernel, dim3(K, B), dim3(DPP_THREADS), 0, st, frames, H, W, partial, static_cast<const CompStat*>(stats),
               static_cast<const unsigned long long*>(cand), K, seed_out, status, report);
    return dpp_launch_status();
}

extern "C" int dpp_hand_size(const unsigned char* keys, const int* labels, const void* stats, int B, int H, int W, void* state, const float* com,
                             const float* cube_in, double fx, double fy, double tol, float* cube_out, int* status, dpp_stream_t stream) {
    if (!keys || !labels || !stats || !state || !com || !cube_in || !cube_out || !status || !cc_dims_ok(B, H, W) || fx == 0.0 || fy == 0.0)
        return DPP_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DPP_LAUNCH(comp_select_kernel, dim3(dpp_cdiv(H * W, DPP_THREADS), B), dim3(DPP_THREADS), 0, st, labels, keys, static_cast<const CompStat*>(stats),
               H, W, 1, static_cast<unsigned long long*>(state));
    DPP_LAUNCH(hand_size_kernel, dim3(dpp_cdiv(B, DPP_WAVE)), dim3(DPP_WAVE), 0, st, static_cast<const CompStat*>(stats),
               static_cast<const unsigned long long*>(state), B, H, W, com, cube_in, fabs(fx), fabs(fy), tol, cube_out, status);
    return dpp_launch_status();
}
