/*
 * dpp_hip.h -- C ABI of libdpp_hip.so, the MI355X (gfx950) kernels behind the DeepPrior++ hot path.
 *
 * The reference (moberweger/deep-prior-pp) has NO FFI / plugin / operator interface for this path:
 * every device op is generated implicitly by Theano 0.9 from the Python layer classes (SURVEY.md
 * section 8(b)).  This ABI is therefore new; each entry point names the reference call site whose
 * arithmetic it replaces.  The Python packages net/ and trainer/ (the drop-in boundary proper) bind it
 * with ctypes (deep-prior-pp_amd/hipdp/lib.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm allocations in the product);
 *     nothing is allocated, freed or retained across calls;
 *   - all tensors are float32 (exception: the bf16 STORAGE mode below); activations are NHWC ("pixel-major": row m = (n*H + y)*W + x holds the C
 *     channels of one pixel); a single-channel NCHW depth crop is bit-identical to its NHWC form;
 *   - every call is asynchronous on `stream`; return value 0 = launched, otherwise a hipError_t or a
 *     DPP_E_* code; no exceptions cross the boundary; thread-compatible (one stream per process/GPU);
 *   - convolution weights are kept in "kernel layout" Wk[Cout][taps][Cin] with the Theano true-
 *     convolution flip already applied: Wk[o][(dy+ph)*kw + (dx+pw)][c] = W_ref[o][c][kh-1-(dy+ph)]
 *     [kw-1-(dx+pw)], so the kernels compute a plain correlation.
 */
#ifndef DPP_HIP_H
#define DPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dpp_stream_t; /* a hipStream_t */

#define DPP_OK 0
#define DPP_E_BADARG 10001
#define DPP_E_UNSUPPORTED 10002

#define DPP_ABI_VERSION 25
int dpp_abi_version(void);

/* bf16 STORAGE of activation tensors (ABI v9; BASELINE config 5 "bf16 MFMA, 256x256 input stress").  The [pixels][channels] tensors the
 * convolutions write -- and only those: weights, gradients, FC outputs and every vector stay float32 -- may be held as bfloat16: the
 * producer's epilogue rounds the f32 value it formed (accumulator + bias + residual) to nearest-even on the store, the fused BatchNorm
 * statistics are still those of the UNROUNDED values, and every reader widens on the load (exact).  A `store` bit mask on the entry
 * points that can see such a tensor says which of its pointers address bf16 elements (same element offsets / leading dimensions as
 * f32; 8-byte alignment instead of 16).  0 everywhere = the float32 layout of ABI v8.
 * The GRADIENTS of those tensors -- the masked gradient G a data-gradient epilogue writes, the dX dpp_bn_bwd_apply writes -- may be
 * bf16-stored in the same way (rounded on the store, partial sums from the unrounded values): they take the A / C roles of the calls
 * that read / write them. */
#define DPP_ST_A 1    /* operand A / the input map X */
#define DPP_ST_B 2    /* operand B (the forward activations in a filter-gradient call) */
#define DPP_ST_C 4    /* the output C / Y and, when given, the residual */
#define DPP_ST_BNX 8  /* dpp_epilogue.bn_x (the BatchNorm input a data-gradient epilogue reads) */

/* Pixel row map: row m of a compact (N,Ho,Wo) map -> row of a (N,Hi,Wi) map sampled with stride s.
 * s == 1 is the identity.  Used for Theano's `subsample` (convlayer.py:230-235) and its gradient. */
typedef struct {
    int s, Wo, HoWo, Wi, HiWi;
} dpp_rowmap;

/* Operand prologue applied while a tile is staged: the BatchNorm + ReLU that precede a conv / FC in the
 * pre-activation blocks (batchnormlayer.py:192, theano_helpers.py:61-69), evaluated as
 *   v = (x - mean[c]) * scale[c] + beta[c]   (mode & 2),   v = max(v, 0)   (mode & 1)
 * with c = (index along the operand's contiguous dimension) % cmod.
 * mode == 4 (operand A of dpp_gemm only): the operand is the gradient through a BatchNorm's batch statistics,
 *   v = scale[c] * g - aux[c] * (x2 - mean[c]) - beta[c]
 * evaluated from the masked gradient g (the operand itself) and the BatchNorm input x2 (same shape and leading dimension
 * as the operand) instead of being materialised by dpp_bn_bwd_apply: with scale = gamma*inv_std, aux = scale*inv_std*c2 and
 * beta = scale*c1 (written by dpp_bn_bwd_finalize) this is dX = scale * (G - c1 - xhat*c2), batchnormlayer.py:119-194 under
 * T.grad.  If `out` is set (K-contiguous operand only) the values formed are also written there, in the operand's layout,
 * by the workgroups of the first column block: the data-gradient GEMM materialises dX on the way for the kernels that
 * want it as a plain tensor (the filter gradient on the other stream). */
typedef struct {
    const float* mean;
    const float* scale;
    const float* beta;
    int mode;
    int cmod;
    const float* x2;     /* mode 4 only */
    const float* aux;    /* mode 4 only */
    float* out;          /* mode 4 only, may be NULL */
} dpp_act;

/* Optional fused epilogue work on the output tile (both NULL = plain epilogue).
 *   stats      [2][N][row_blocks] (block index fastest, see the BatchNorm section): per-workgroup-row-block (mean, M2) of
 *              every output column, i.e. the partial BatchNorm statistics of the tensor being written
 *              (batchnormlayer.py:154-155) -- saves the separate statistics pass; combine with
 *              dpp_bn_finalize(partial = stats, nb = row_blocks, rows_per_block = tile rows).
 *   bn_x ...   BatchNorm-backward fusion for a data-gradient call: the value written is G = acc * [ (x-mean)*scale+beta >= 0 ]
 *              (bn_relu != 0) with x = bn_x at the output's index, and bn_partial [2][N][row_blocks] receives the per-block
 *              (sum G, sum G*xhat), xhat = (x-mean)*inv_std: exactly what dpp_bn_bwd_reduce would produce. */
typedef struct {
    float* stats;
    const float* bn_x;
    const float* bn_mean;
    const float* bn_inv_std;
    const float* bn_scale;
    const float* bn_beta;
    int bn_relu;
    int pad_;
    float* bn_partial;
} dpp_epilogue;

/*
 * Generic f32 MFMA GEMM  C[M x N] = A_op[M x K] * B_op[K x N]  (v_mfma_f32_16x16x4_f32, LDS-staged).
 *   a_kc = 1: A_op(i,k) = A[mapA(i)*lda + k]      a_kc = 0: A_op(i,k) = A[mapA(k)*lda + i]
 *   b_kc = 1: B_op(k,j) = B[j*ldb + k]            b_kc = 0: B_op(k,j) = B[mapB(k)*ldb + j]
 * splitk == 1: C[mapC(i)*ldc + j] = acc + bias[j] + residual[mapC(i)*ldc + j]   (residual may alias C)
 * splitk  > 1: partial[z][i*N + j] = acc over K-slice z (reduce with dpp_reduce_partials).
 * Replaces, with the operand flags shown in deep-prior-pp_amd/hipdp/ops.py:
 *   1x1 ConvLayer forward                conv2d           /root/reference/src/net/convlayer.py:230-240
 *   its data / filter gradients          T.grad           /root/reference/src/trainer/poseregnettrainer.py:110-111
 *   HiddenLayer forward x.W + b          T.dot            /root/reference/src/net/hiddenlayer.py:136-139
 *   its gradients                        T.grad           poseregnettrainer.py:110-111
 *   residual add                         inputVar + conv  /root/reference/src/net/resnet.py:379,414
 */
typedef struct {
    const float* A; int lda; int a_kc; dpp_rowmap mapA; dpp_act actA;
    const float* B; int ldb; int b_kc; dpp_rowmap mapB; dpp_act actB;
    float* C; int ldc; dpp_rowmap mapC;
    const float* bias;
    const float* residual;
    int M, N, K;
    int splitk;
    float* partial;
    int bm, bn, wm; /* tile: rows, cols, waves along M (4 or 1); 0 = choose */
    int variant;    /* 0: LDS-tiled kernel (any layout, split-K); 1: row-streaming kernel for skinny conv GEMMs (a_kc = 1,
                       splitk = 1, bm in {64,128}, bn in {16,32,64}): A fragments straight from global memory, no barrier
                       in the K loop;
                       2: K-split kernel (a_kc = 1, splitk = 1, identity row maps, no actB; K = 256 with N % 64 == 0 or
                       K = 128 with N % 32 == 0, M % 32 == 0): a workgroup owns 32 rows x all columns x the whole K, every
                       load issued up front, the four waves split K; statistics blocks of 32 rows;
                       3: barrier-free row stream (a_kc = 1, splitk = 1, identity row maps, no actB; K = 64 -> N = 16
                       with M % 128 == 0, statistics blocks of 128 rows, or K = 16 -> N = 64 with M % 64 == 0, blocks of
                       64 rows): a wave owns whole 16-row tiles, epilogue in the MFMA D layout;
                       4: wave-autonomous strips for the channel-EXPANDING shapes (a_kc = 1, splitk = 1, identity row maps,
                       no actB; K in {16, 32, 64}, N % 64 == 0, M % bm == 0 with bm = rows per wave = rows per statistics
                       block, a multiple of 32, 0 = choose): a wave owns bm rows x 64 columns x the whole K, columns dealt
                       interleaved to the accumulator tiles so that the D layout gives 16-byte accesses; no LDS, no
                       barrier.  b_kc = 1 with the modes 0-3 prologue (forward), b_kc = 0 with a plain or mode-4
                       operand and the BatchNorm-backward epilogue (data gradient).
                       Variants 2-4 return DPP_E_UNSUPPORTED for anything else (bn / wm are ignored). */
    dpp_epilogue epi; /* fused statistics / BatchNorm-backward epilogue (requires splitk == 1) */
    int store;        /* DPP_ST_* mask: which of A, B, C (+ residual), epi.bn_x hold bf16 elements (0 = all float32).  Variant 4 and the
                         generic tiles with 16-byte-aligned whole-quad shapes take it; DPP_E_UNSUPPORTED otherwise. */
    int precision;    /* 0: f32 MFMA (exact); 1: both operands rounded to bf16 (RNE, A after its prologue), f32 accumulation on
                         v_mfma_f32_16x16x32_bf16 -- BASELINE config 5.  Variant 4 with K = 32 / 64 only (dpp_gemm_variant_rows says
                         0 otherwise); dpp_fc_gemm takes its precision as an argument and ignores this field. */
} dpp_gemm_desc;
/* Alignment.  A, B (and actA.x2 / actA.out of a mode-4 operand) off a 16-byte boundary: variant 0 loads that operand one float at a time,
 * variants 2-4 answer DPP_E_UNSUPPORTED.  C, residual, bias, epi.bn_x and the four epi.bn_* vectors off it: the one-float-per-store epilogue.
 * The prologue vectors (mean, scale, beta, aux) must be 16-byte aligned: DPP_E_BADARG.  partial, epi.stats and epi.bn_partial are accessed
 * one float at a time by every variant: 4-byte alignment is enough. */
int dpp_gemm(const dpp_gemm_desc* d, dpp_stream_t stream);
/* Would dpp_gemm run `d` on the kernel d->variant asks for (2, 3 or 4)?  Returns that kernel's rows per workgroup (the row-block count of
 * the fused-epilogue partials is M / rows), or 0: alignment, prologue mode or the epilogue rule it out and the caller should describe
 * the problem with variant 0 and a generic tile instead (dpp_gemm itself returns DPP_E_UNSUPPORTED rather than change the partial
 * layout behind the caller's back).  Launches nothing. */
int dpp_gemm_variant_rows(const dpp_gemm_desc* d);
/* ABI v18.  A variant-0 launch of more row tiles than the device holds at once runs on the WALKING form of the LDS-tiled kernel: as many
 * workgroups as are resident (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs, shared among the column tiles), each staging its K x bn
 * panel of B once and taking row tiles b, b + gx, ...; same tile, same arithmetic, bit-identical results, statistics partials indexed by
 * the tile.  Taken for splitk == 1, a K-contiguous A with a mode 0-3 prologue, a plain B, K <= 128 in whole chunks, whole column tiles and
 * the 16-byte epilogue; everything else keeps one workgroup per tile.  Environment DPP_GEMM_WALK (read per call): 0 = never walk, N = at most
 * N workgroups per column tile.  This query returns 1 and the grid (gx row-walking workgroups x gy column tiles) when dpp_gemm would run `d`
 * that way, 0 (and gx = gy = 0) when it would not.  Host only: launches nothing. */
int dpp_gemm_walk_grid(const dpp_gemm_desc* d, int* gx, int* gy);

/* Filter gradient of a 1x1 ConvLayer as a barrier-free row stream (csrc/wgrad.hip):
 *   partial[s][o][c] = sum over the pixel rows m of slice s of  dY[m][o] * act(X)[mapX(m)][c]
 * dY [M][Co] and X [rows][Ci] pixel-major (NHWC), mapX the stride row map of the layer (NULL = identity), actX the BatchNorm +
 * ReLU prologue of the layer's input (NULL = none; modes 0-3).  rows_per_wave (a multiple of 4) pixel rows go to one wave; the
 * number of slices written is dpp_wgrad_stream_slices(Co, Ci, M, rows_per_wave) -- 0 when (Co, Ci) is not one of the shapes of the
 * ResNet's 1x1 layers (16x64, 64x16, 16x32, 64x32, 32x64, 32x128, 128x32, 128x64, 64x128, 64x256, 256x64, 256x128), for which
 * (dY, X, partial and, with a mode 2 / 3 prologue, its mean / scale / beta must be 16-byte aligned -- here, in dpp_wgrad3_stream and in
 * dpp_fc_wgrad_stream (dW for partial): they are only accessed 8 or 16 bytes at a time; DPP_E_BADARG otherwise, nothing launched)
 * dpp_gemm's generic filter-gradient layout (a_kc = b_kc = 0, splitk) remains.  Sum the slices with dpp_reduce_multi /
 * dpp_reduce_partials (fixed order).  T.grad of convlayer.py:230-240 (poseregnettrainer.py:110-111). */
int dpp_wgrad_stream_slices(int Co, int Ci, int M, int rows_per_wave);
int dpp_wgrad_stream(const float* dY, int Co, const float* X, int Ci, const dpp_rowmap* mapX, const dpp_act* actX, int M,
                     int rows_per_wave, float* partial, int store /* DPP_ST_B: X, DPP_ST_A: dY hold bf16 */, dpp_stream_t stream);
/* (ABI v11) the same with both operands on bf16 MFMA (the activation rounded after its prologue); the stage-1 shapes only
 * (dpp_wgrad_stream_bf16_ok: Co in {16, 64} with Ci in {16, 32, 64}), DPP_E_UNSUPPORTED otherwise.  Same slices / partial layout. */
int dpp_wgrad_stream_bf16_ok(int Co, int Ci);
int dpp_wgrad_stream_bf16(const float* dY, int Co, const float* X, int Ci, const dpp_rowmap* mapX, const dpp_act* actX, int M,
                     int rows_per_wave, float* partial, int store /* DPP_ST_B: X, DPP_ST_A: dY hold bf16 */, dpp_stream_t stream);

/* Filter gradient of a 3x3 'half'-padded, stride-1 ConvLayer on the same kind of stream:
 *   partial[s][o][t][c] = sum over the pixels p of slice s of  dY[p][o] * act(X)[p + (dy, dx)][c],  t = 3 (dy + 1) + (dx + 1),
 * taps outside the image contribute zero.  X [N][H][W][Ci], dY [N][H][W][Co], W % 4 == 0 (a step is four neighbouring pixels of a
 * row).  Shapes: Co == Ci in {16, 32, 64} (the bottleneck convolutions of resnet.py:300-420); dpp_wgrad3_stream_slices returns 0
 * for anything else and dpp_conv3x3_wgrad (the LDS-tiled kernel, same partial layout per block) remains.  Same T.grad. */
/* Filter gradient of a HiddenLayer whose reduction is only the batch (FC1: dW[k][n] = sum_b act(X)[b][k] * dY[b][n]; X [Nb][K],
 * dY [Nb][N], dW [K][N], all row-major; actX = the BatchNorm + ReLU prologue of the flattened map, channel = column % cmod) on the
 * row stream: a wave owns a 64 x 64 block of dW over all rows, no LDS, no partials.  K and N multiples of 128
 * (dpp_fc_wgrad_stream_ok), otherwise dpp_fc_gemm's layout remains.  T.grad of hiddenlayer.py:136-139. */
int dpp_fc_wgrad_stream_ok(int Nb, int K, int N);
int dpp_fc_wgrad_stream(const float* X, const float* dY, float* dW, int Nb, int K, int N, const dpp_act* actX,
                        int store /* DPP_ST_B: X holds bf16 */, dpp_stream_t stream);
int dpp_wgrad3_stream_slices(int Co, int Ci, int N, int H, int W, int rows_per_wave);
int dpp_wgrad3_stream(const float* dY, int Co, const float* X, int Ci, int N, int H, int W, const dpp_act* actX, int rows_per_wave,
                      float* partial, int store /* DPP_ST_B: X, DPP_ST_A: dY hold bf16 */, dpp_stream_t stream);

/* The same contract on the weight-streaming kernel for the HiddenLayer behind the last convolution map (FC1: 16 384 x 1 024
 * weights at 128x128 input, 65 536 x 1 024 at 256x256; hiddenlayer.py:136-139 and its T.grad): tile 128 x 64, both operands
 * K-contiguous in LDS (memory-MN-contiguous operands are transposed while staged), double-buffered LDS.
 * precision 0: exact f32 (v_mfma_f32_16x16x4_f32; equals dpp_gemm up to summation order).
 * precision 1: operands rounded to bf16 (RNE, after the prologue), f32 accumulation (v_mfma_f32_16x16x32_bf16) -- BASELINE
 *              config 5; not for the 1e-3 mm parity path.
 * kchunk: 32 | 64 (0 = 64).  d->bm / bn / wm / variant are ignored; no fused statistics / BatchNorm-backward epilogue.
 * Alignment: A or B off a 16-byte boundary is loaded one float at a time (and keeps the call off the three-stage kernel); C / partial,
 * residual and bias off it: DPP_E_UNSUPPORTED; the mean / scale / beta of a mode 2 / 3 prologue off it: DPP_E_BADARG. */
int dpp_fc_gemm(const dpp_gemm_desc* d, int precision, int kchunk, dpp_stream_t stream);

/* out[i] = sum_z partial[z*n + i] (+ bias[i % nbias] if bias) -- fixed summation order (deterministic).  One float per access:
 * 4-byte alignment is enough (dpp_reduce_multi takes 16-byte accesses per job when n % 4 == 0 and the job's pointers allow them). */
int dpp_reduce_partials(const float* partial, int nz, int n, const float* bias, int nbias, float* out,
                        dpp_stream_t stream);


/* Batched form: jobs_dev = device array of { const float* partial; float* out; int nz, n, block0, pad; } sorted by block0,
 * job j owning workgroups [block0_j, block0_j + ceil(n_j / dpp_reduce_multi_block_cols())); total_blocks = sum.  One launch
 * reduces every filter / bias gradient partial of a backward pass. */
size_t dpp_reduce_job_bytes(void);
int dpp_reduce_multi_block_cols(void);
int dpp_reduce_multi(const void* jobs_dev, int njobs, int total_blocks, dpp_stream_t stream);

/* ---- 3x3 'half' stride-1 ConvLayer on NHWC maps (implicit GEMM, halo tile in LDS) --------------------------
 * Y[n,y,x,o] = sum_{tap,c} act(X)[n, y+dy, x+dx, c] * Wk[o][tap][c] + bias[o] + residual[n,y,x,o], zero padding applied
 * after `act`.  conv2d 3x3 of res_block, /root/reference/src/net/resnet.py:365-368,394-397 via
 * /root/reference/src/net/convlayer.py:230-240.  The data gradient is the same call on dY with the weights from
 * dpp_conv3x3_wtrans.  bm = 64 | 128 rows per workgroup (0 = choose).  Ci, Co multiples of 16.
 * Alignment: X (8 bytes when bf16-stored, else 16), Wk and the prologue's mean / scale / beta must lie on 16-byte boundaries --
 * DPP_E_BADARG otherwise, nothing is launched (they are only ever read 16 bytes at a time).  Y, residual, bias, epi->bn_x and the
 * four epi->bn_* vectors may be 4-byte aligned: the call then takes the one-float-per-store epilogue (float32 tensors only; with a
 * bf16-stored Y or bn_x DPP_E_UNSUPPORTED).  epi->stats and epi->bn_partial are accessed one float at a time. */
int dpp_conv3x3(const float* X, int N, int H, int W, int Ci, const dpp_act* act, const float* Wk, int Co,
                const float* bias, const float* residual, float* Y, int bm, const dpp_epilogue* epi,
                int store /* DPP_ST_A: X, DPP_ST_C: Y + residual, DPP_ST_BNX: epi->bn_x hold bf16 */, dpp_stream_t stream);
/* The same with the activated input and the weights rounded to bf16 (RNE) as they are staged in LDS, f32 accumulation
 * (v_mfma_f32_16x16x32_bf16): BASELINE config 5, not for the 1e-3 mm parity path.  Same tiling, epilogues and results layout. */
int dpp_conv3x3_bf16(const float* X, int N, int H, int W, int Ci, const dpp_act* act, const float* Wk, int Co,
                     const float* bias, const float* residual, float* Y, int bm, const dpp_epilogue* epi, int store, dpp_stream_t stream);
/* The same convolution for the narrow square layers (C = Ci = Co in {16, 32}, W % 16 == 0, float32 tensors, no residual) as a
 * wave-autonomous stream: a wave owns 16-pixel pieces of image rows, keeps the 9 x C x C filter in registers and loads every tap
 * straight from global memory -- no halo tile, no barrier before the column reductions.  dpp_conv3x3_stream_rows = pixels per
 * workgroup (= per block of epi->stats / epi->bn_partial), or 0 when the shape is not taken (then dpp_conv3x3_stream returns
 * DPP_E_UNSUPPORTED and dpp_conv3x3 remains).  Same arithmetic per output element as dpp_conv3x3 up to the summation order.
 * Alignment: X, Wk and the prologue vectors 16 bytes (DPP_E_UNSUPPORTED otherwise); Y, bias and everything in epi are accessed one
 * float at a time: 4-byte alignment is enough. */
int dpp_conv3x3_stream_rows(int N, int H, int W, int C);
int dpp_conv3x3_stream(const float* X, int N, int H, int W, int C, const dpp_act* act, const float* Wk, const float* bias, float* Y,
                       const dpp_epilogue* epi, dpp_stream_t stream);
/* tile geometry chosen for (N,H,W,bm): returns the number of workgroup row blocks, writes tile height / width / images */
int dpp_conv3x3_tiling(int N, int H, int W, int bm, int* th, int* tw, int* img);
/* Wd[c][8-tap][o] = Wk[o][tap][c] (mirrored taps, channels swapped): weights of the data-gradient correlation. */
int dpp_conv3x3_wtrans(const float* Wk, int Co, int Ci, float* Wd, dpp_stream_t stream);
/* Batched form: jobs_dev = device array of { const float* Wk; float* Wd; int Co, Ci, block0, pad; } sorted by block0, job j owning
 * workgroups [block0_j, block0_j + ceil(Co*9*Ci / 256)); one launch mirrors the weights of every 3x3 layer of a net. */
size_t dpp_wtrans_job_bytes(void);
int dpp_conv3x3_wtrans_multi(const void* jobs_dev, int njobs, int total_blocks, dpp_stream_t stream);
/* Filter gradient partials: partial[blk][o][tap][c] = sum over the workgroup's pixels of dY[.,o] * act(X)[.+tap, c];
 * blk < dpp_conv3x3_wgrad_blocks(N,H,W,Ci,Co,bm); sum over blk with dpp_reduce_partials.  (T.grad, poseregnettrainer.py:110-111)
 * Alignment: X, dY (8 bytes when bf16-stored, else 16) and the prologue vectors (16): DPP_E_BADARG otherwise, nothing launched; the
 * partials are stored one float at a time: 4-byte alignment is enough. */
int dpp_conv3x3_wgrad_blocks(int N, int H, int W, int Ci, int Co, int bm);
int dpp_conv3x3_wgrad(const float* X, int N, int H, int W, int Ci, const dpp_act* act, const float* dY, int Co,
                      float* partial, int bm, int store /* DPP_ST_A: X, DPP_ST_B: dY hold bf16 */, dpp_stream_t stream);
/* (ABI v11) the same with bf16 MFMA operands (BASELINE config 5; `T.grad` of /root/reference/src/net/convlayer.py:230-240 evaluated with
 * both operands rounded to bfloat16, f32 accumulation): act(X) is rounded to nearest-even AFTER the prologue, dY is rounded likewise (exact
 * when it is bf16-stored).  Layers dpp_conv3x3_wgrad_bf16_ok() accepts only (16 or 32 channels in and out, maps >= 12 wide);
 * DPP_E_UNSUPPORTED otherwise.  Same partial layout and slice count as dpp_conv3x3_wgrad. */
int dpp_conv3x3_wgrad_bf16_ok(int N, int H, int W, int Ci, int Co);
int dpp_conv3x3_wgrad_bf16(const float* X, int N, int H, int W, int Ci, const dpp_act* act, const float* dY, int Co,
                           float* partial, int bm, int store /* DPP_ST_A: X, DPP_ST_B: dY hold bf16 */, dpp_stream_t stream);

/* ---- ResNet stem: ConvPoolLayer 5x5 'half' 1 -> Co (<= 32), 2x2 max-pool, bias AFTER the pool ----------------
 * /root/reference/src/net/convpoollayer.py:251-282 as built at /root/reference/src/net/resnet.py:128-133.
 * X: [N][H][W] single-channel crops (NCHW == NHWC); Wk: [Co][25]; Y: [N][H/2][W/2][Co]; argmax: the TIE MASK of each
 * 2x2 window (bit j set = window element j, row-major, equals the maximum), kept for the filter gradient: Theano's
 * MaxPoolGrad gives the gradient to every element equal to the maximum, and the constant background of a depth crop
 * makes whole windows tie.
 * stats (may be NULL; needs H % 16 == W % 16 == 0): [2][Co][N * H/16 * W/16] per-tile (mean, M2) of the 64 pooled outputs a
 * workgroup writes -- the BatchNorm statistics partial of Y, combined by dpp_bn_finalize(rows_per_block = 64).
 * Alignment: dpp_stem_fwd stores the tie masks one byte at a time (any argmax pointer); dpp_stem_wgrad loads four channels of dY and
 * of the tie mask at once when Co % 4 == 0, dY is 16-byte and argmax 4-byte aligned, and element by element otherwise. */
int dpp_stem_fwd(const float* X, int N, int H, int W, const float* Wk, const float* bias, int Co, float* Y, uint8_t* argmax,
                 float* stats, int store /* DPP_ST_C: Y holds bf16 */, dpp_stream_t stream);
int dpp_stem_wgrad_blocks(int N, int H, int W, int tiles_per_block);
int dpp_stem_wgrad(const float* X, int N, int H, int W, const float* dY, const uint8_t* argmax, int Co, float* partial,
                   int tiles_per_block, dpp_stream_t stream);

/* ---- generic ConvPoolLayer: kh x kw conv ('valid': pad 0, 'half': pad k/2), pool x pool max-pool (ignore_border), bias
 * AFTER the pool; the activation is the consumer's operand prologue.  /root/reference/src/net/convpoollayer.py:251-282
 * as built by PoseRegNet, /root/reference/src/net/poseregnet.py:62-78 (5x5/pool 4, 5x5/pool 2, 3x3/no pool, 8 filters).
 * X: [N][H][W][Ci] with the optional ReLU / BN prologue `act`; Wk: [Co][kh*kw][Ci] (flipped, layout.py);
 * Y: [N][Hp][Wp][Co], Hp = (H + 2 pad - kh + 1) / pool; ties: [N][Hp][Wp][Co] uint16 tie masks of the pool windows
 * (bit j = window element j, row-major, equals the maximum; NULL allowed when pool == 1 or in inference).
 * wgrad: partial[blk][Co][kh*kw][Ci], blk < dpp_convpool_wgrad_blocks(N, Hp, Wp); sum with dpp_reduce_multi.
 * dgrad: dX[N][H][W][Ci] = gradient w.r.t. the (activated) input operand.  Limits: Co <= 32, Ci <= 32, pool <= 4, k <= 7.
 * These layers are 12.8 MFLOP / sample in total: VALU kernels, one thread per output pixel.  Every access to global memory is one
 * element wide: no pointer needs more than its element's alignment. */
int dpp_convpool_fwd(const float* X, int N, int H, int W, int Ci, const dpp_act* act, const float* Wk, int kh, int kw, int pad,
                     int Co, int pool, const float* bias, float* Y, uint16_t* ties, dpp_stream_t stream);
int dpp_convpool_wgrad_blocks(int N, int Hp, int Wp);
int dpp_convpool_wgrad(const float* X, int N, int H, int W, int Ci, const dpp_act* act, const float* dY, const uint16_t* ties,
                       int kh, int kw, int pad, int Co, int pool, float* partial, dpp_stream_t stream);
int dpp_convpool_dgrad(const float* dY, const uint16_t* ties, int N, int H, int W, int Ci, const float* Wk, int kh, int kw,
                       int pad, int Co, int pool, float* dX, dpp_stream_t stream);

/* ---- BatchNormLayer, /root/reference/src/net/batchnormlayer.py:119-194 (tensors pixel-major [M][C], C % 4 == 0) ----
 * stats_partial: per row-chunk (mean_b, M2_b) -> partial[2][C][nb], nb = ceil(M / rows_per_block); the block index is the
 *                fastest one so that the finalize (one wave per channel, lanes over blocks) reads contiguous memory
 * finalize:      batch mean, inv_std = 1/sqrt(var_biased + eps), scale = gamma*inv_std; running mean / inv_std EMA
 *                (alpha = 0 or run_mean == NULL: no update).  `partial` holds nseg consecutive [2][C][nb] segments (nseg = 1,
 *                or the ranks of a synchronised-BatchNorm all-gather) covering M rows in total, M / nseg per segment
 * eval_coeffs:   deterministic mode: mean = run_mean, inv_std = run_inv_std, scale = gamma*run_inv_std
 * bwd_reduce:    G = dA * [ (x-mean)*scale+beta >= 0 ] (relu != 0) or dA; partial[2][C][nb] = sum G, sum G*xhat
 * bwd_finalize:  dbeta, dgamma and c1 = dbeta/M, c2 = dgamma/M; if q != NULL also q = scale*c1 and p = scale*inv_std*c2, the
 *                per-channel constants of the mode-4 operand prologue (dpp_act)
 * bwd_apply:     dX = scale * (G - c1 - xhat*c2) + add      (gradient through the batch statistics)
 * Alignment: the [M][C] tensors (X, dA, G, add, dX: 16 bytes, 8 when bf16-stored) and the per-channel vectors that stats_partial,
 * bwd_reduce, bwd_apply and bwd_finalize_apply READ (mean, inv_std, scale, beta, c1, c2) are accessed four channels at a time:
 * DPP_E_BADARG otherwise, nothing launched; bwd_finalize_apply also reads `partial` 16 bytes at a time when nb % 4 == 0.  Partials,
 * column sums, and everything finalize / bwd_finalize / eval_coeffs touch go one float at a time: 4-byte alignment is enough. */
int dpp_bn_stats_partial(const float* X, int M, int C, int rows_per_block, float* partial, int store /* DPP_ST_A: X holds bf16 */,
                         dpp_stream_t stream);
int dpp_bn_finalize(const float* partial, int nb, int nseg, int M, int rows_per_block, int C, const float* gamma, float eps,
                    float* mean, float* inv_std, float* scale, float* run_mean, float* run_inv_std, float alpha,
                    dpp_stream_t stream);
int dpp_bn_eval_coeffs(const float* gamma, const float* run_mean, const float* run_inv_std, int C, float* mean,
                       float* inv_std, float* scale, dpp_stream_t stream);
/* eval_coeffs for EVERY BatchNorm of a net in ONE launch (ABI v10): the test-time forward pass issued one 4.7 us launch per
 * BatchNorm -- 61 of its 131 launches.  jobs (device): dpp_bn_eval_job_bytes() bytes each = { const float* gamma, * run_mean, * run_inv_std;
 * float* mean, * inv_std, * scale; int C; int block0 } with block0 = the first 256-thread block of the job, total_blocks their sum. */
size_t dpp_bn_eval_job_bytes(void);
int dpp_bn_eval_coeffs_multi(const void* jobs, int njobs, int total_blocks, dpp_stream_t stream);
int dpp_bn_bwd_reduce(const float* dA, const float* X, int M, int C, const float* mean, const float* inv_std,
                      const float* scale, const float* beta, int relu, float* G, int rows_per_block, float* partial,
                      int store /* DPP_ST_BNX: X, DPP_ST_A: the incoming gradient (dA / G), DPP_ST_C: the outgoing one (G / dX + add) hold bf16 */, dpp_stream_t stream);
int dpp_bn_bwd_finalize(const float* partial, int nb, int nseg, int M, int C, float* dbeta, float* dgamma, float* c1, float* c2,
                        const float* inv_std, const float* scale, float* q, float* p, dpp_stream_t stream);
int dpp_bn_bwd_apply(const float* G, const float* X, int M, int C, const float* mean, const float* inv_std,
                     const float* scale, const float* c1, const float* c2, const float* add, float* dX,
                     int rows_per_block, float* colsum_partial /* [nb][C] column sums of dX, or NULL */,
                     int store /* DPP_ST_BNX: X, DPP_ST_A: the incoming gradient (dA / G), DPP_ST_C: the outgoing one (G / dX + add) hold bf16 */, dpp_stream_t stream);
/* dpp_bn_bwd_finalize (nseg = 1, no q / p) + dpp_bn_bwd_apply in one launch, for BatchNorms whose per-block sums are few (the small
 * maps of the late stages): every workgroup -- grid (ceil(M / rows_per_block), C / 32) -- reduces the `nb` blocks of `partial`
 * ([2][C][nb], the layout dpp_bn_bwd_reduce and the fused data-gradient epilogues write) for its 32 channels itself, then applies.
 * Writes dbeta / dgamma like the finalize kernel; c1 / c2 never reach memory.  dpp_bn_bwd_finalize_apply_ok: C % 32 == 0 and
 * nb <= 256, else DPP_E_UNSUPPORTED (the two launches remain). */
int dpp_bn_bwd_finalize_apply_ok(int M, int C, int nb);
int dpp_bn_bwd_finalize_apply(const float* G, const float* X, int M, int C, const float* mean, const float* inv_std,
                              const float* scale, const float* partial, int nb, const float* add, float* dX, int rows_per_block,
                              float* colsum_partial, float* dbeta, float* dgamma, int store, dpp_stream_t stream);

/* ---- loss / optimiser / small elementwise ------------------------------------------------------------------ */
/* partial[b][c] = sum of rows of chunk b (bias gradients; reduce with dpp_reduce_partials) */
int dpp_colsum_partial(const float* X, int M, int C, int rows_per_block, float* partial, dpp_stream_t stream);
/* cost = (1/denom) sum (out-y)^2, dout = (2/denom)(out-y): /root/reference/src/trainer/poseregnettrainer.py:92-99
 * (denom = batch for the embedding loss, batch*numJoints for the joint loss); dout may be NULL */
int dpp_loss_sse(const float* out, const float* y, int rows, int d, int denom, float* cost, float* dout, dpp_stream_t stream);
/* (ABI v11) dpp_reduce_partials (out[rows][d] = sum of nz split-K slices + bias[d], the last HiddenLayer of the net,
 * /root/reference/src/net/hiddenlayer.py:136-139) and dpp_loss_sse on that output in ONE launch; rows * d <= 65536. */
int dpp_reduce_partials_loss(const float* partial, int nz, int rows, int d, const float* bias, float* out, const float* y, int denom,
                             float* cost, float* dout, dpp_stream_t stream);
/* The scalar-target case (numJoints == nDims == 1, poseregnettrainer.py:84-85, 92-93): Theano broadcasts the (B, 1) output against
 * the VECTOR y, so the cost is mean_i mean_j (out_i - y_j)^2 and dout_i = (2 / B)(out_i - mean(y)); n = B.  err (may be NULL):
 * the monitor of :115 under the same broadcast, err[0] = mean, err[1] = max over all pairs of |out_i - y_j|. */
int dpp_loss_sse_bcast(const float* out, const float* y, int n, float* cost, float* dout, float* err, dpp_stream_t stream);
/* err[0] = mean_rows sqrt(sum_d (out-y)^2), err[1] = max_rows: poseregnettrainer.py:114-129 (errors, errors_avg, errors_max) */
int dpp_error_l2(const float* out, const float* y, int rows, int d, float* err, dpp_stream_t stream);
/* The reference's ADAM (/root/reference/src/trainer/optimizer.py:58-90) over a flat parameter buffer.
 * state (device, 8 floats): lr, t, beta1, beta2, epsilon, gamma, 0, 0 -- the bias-correction terms are evaluated on the
 * device in float32; dpp_adam_tick performs `t <- t + 1` (optimizer.py:88) after the update. */
int dpp_adam(float* w, const float* g, float* m, float* v, size_t n, const float* state, dpp_stream_t stream);
/* (ABI v11) dpp_adam followed by dpp_adam_tick in ONE launch: the last workgroup to finish advances t (hyper[1]); hyper[7] is the
 * launch's ticket counter (an unsigned, zero between launches).  For an update that is a single launch over the whole flat buffer. */
int dpp_adam_ticked(float* w, const float* g, float* m, float* v, size_t n, float* hyper, dpp_stream_t stream);
int dpp_adam_tick(float* state, dpp_stream_t stream);
int dpp_axpy(float* y, const float* x, float alpha, size_t n, dpp_stream_t stream);              /* y += alpha x */
int dpp_sumsq(const float* x, size_t n, float alpha, float* out, int accumulate, dpp_stream_t stream);
/* The two above over nseg segments of ONE flat buffer in one launch: seg (DEVICE memory) holds (offset, length) pairs in elements
 * -- the weights of all layers inside the flat parameter / gradient buffers (cost += weightreg_factor * sum(W^2) and its gradient
 * 2 * weightreg_factor * W, poseregnettrainer.py:101-107).  Deterministic: fixed shares per block, f64 partials summed in order.
 * workspace: dpp_sumsq_multi_workspace_bytes() bytes of device memory. */
size_t dpp_sumsq_multi_workspace_bytes(void);
int dpp_sumsq_multi(const float* base, const long long* seg, int nseg, float alpha, void* workspace, float* out, int accumulate,
                    dpp_stream_t stream);
int dpp_axpy_multi(float* ybase, const float* xbase, const long long* seg, int nseg, float alpha, dpp_stream_t stream);
/* y = mask ? mask*relu?(x) : a*relu?(x): DropoutLayer, /root/reference/src/net/dropoutlayer.py:98-104 */
int dpp_scale(const float* x, const float* mask, float a, int relu, float* y, size_t n, dpp_stream_t stream);
/* g = (mask ? mask : a) * dy * [pre >= 0] */
int dpp_relu_bwd(const float* dy, const float* pre, const float* mask, float a, float* g, size_t n, dpp_stream_t stream);

int dpp_fill_zero(void* p, size_t nbytes, dpp_stream_t stream);
/* dst[r][c] = relu ? max(src[r][c], 0) : src[r][c] over rows x cols with row strides lds / ldd: the column-wise
 * concatenation of ScaleNet's flattened tower outputs (/root/reference/src/net/scalenet.py:167-171) and its gradient split */
int dpp_copy2d(const float* src, int lds, float* dst, int ldd, int rows, int cols, int relu, dpp_stream_t stream);
/* out[r][c] = x[r][c] * (s[r*sld + scol] * factor): normalised labels back to mm (label * cube_z / 2), the augmentation's input
 * when the labels are the joints themselves (/root/reference/src/trainer/poseregnettrainer.py:228-240) */
int dpp_rowscale(const float* x, const float* s, int sld, int scol, float factor, float* out, int rows, int cols, dpp_stream_t stream);
/* centre h x w window of each [H][W] image: ScaleNet's 1/2 and 1/4 inputs
 * (/root/reference/src/trainer/scalenettrainer.py:239-251, /root/reference/src/util/handdetector.py:654-666) */
int dpp_crop_center(const float* src, int B, int H, int W, float* dst, int h, int w, dpp_stream_t stream);
/* mask[i] = 1 with probability keep (counter-based generator keyed by seed, counter + *counter_dev, i): DropoutLayer
 * masks; counter_dev (may be NULL) is a device-resident step counter so that a recorded launch draws a new mask per step */
int dpp_bernoulli_mask(float* mask, size_t n, float keep, unsigned long long seed, unsigned long long counter,
                       const unsigned long long* counter_dev, dpp_stream_t stream);

/* ---- online crop augmentation, NetTrainer.augmentCrop (/root/reference/src/trainer/nettrainer.py:919-997) -------
 * prepare: per crop, the geometry of HandDetector.moveCoM / rotateHand / scaleHand
 *          (/root/reference/src/util/handdetector.py:678-780): new CoM, crop transform, inverse warp matrix,
 *          z-thresholds, augmented joint labels, PCA-prior projection (poseregnettrainer.py:262) -> records, out_y.
 *          norm_zero_one: bit 0: the crops are normalised to [0, 1] (normZeroOne, nettrainer.py:948, 982-988) instead of [-1, 1];
 *          bit 1: binarizeImage (poseregnettrainer.py:255-257): the augmented crop is thresholded, < 0.5 -> 0, >= 0.5 -> 1.
 *          mode codes: 0 none, 1 com, 2 rot, 3 sc.  mode == NULL: (mode, off, rot, sc) are drawn on the device from
 *          Philox(seed, counter, sample) with mode = mode_table[u % n_modes].
 * warp:    per pixel, cv2.warpAffine / warpPerspective (NEAREST, constant 0) + recropHand's z-clamp
 *          (handdetector.py:782-803) + the far-plane fill / clamp / re-normalisation of nettrainer.py:982-995. */
size_t dpp_augment_record_bytes(void);
int dpp_augment_prepare(const float* img, const float* com3d, const float* cube, const float* Mcrop, const float* gt3d,
                        int B, int J, int dsz, const int* mode, const double* off, const double* rot, const double* sc,
                        const int* mode_table, int n_modes, unsigned long long seed, unsigned long long counter,
                        double sigma_com, double sigma_sc, double rot_range, double fx, double fy, double ux, double uy,
                        int flip_y, int norm_zero_one, const float* pca_mean, const float* pca_comp, int E, void* records, float* out_y,
                        int* out_mode, const unsigned long long* counter_dev, dpp_stream_t stream);
/* *counter += inc (device-resident draw counter added to `counter` when counter_dev != NULL, so replayed graphs draw fresh
 * augmentation parameters every step) */
int dpp_counter_add(unsigned long long* counter, unsigned long long inc, dpp_stream_t stream);
int dpp_augment_warp(const float* img, const void* records, int B, int dsz, float* out, dpp_stream_t stream);
/* Both stages as ONE launch (what the trainer and bench.py use): prepare + warp of B crops into out_x [B][dsz][dsz] and
 * out_y, `records` optional (NULL: not written).  Device draws (mode == NULL) are keyed by
 *   (seed, (counter + *counter_dev) * global_batch + sample0 + b)
 * i.e. by (seed, step, GLOBAL sample index): a data-parallel rank passes sample0 = rank * B and the global minibatch size, so
 * what a sample draws does not depend on the number of GPUs (global_batch = 0 means B).  With ticket != NULL (a device
 * word, zero before the first call) the launch also advances *counter_dev by one after every workgroup has read it, so a
 * recorded plan / replayed graph draws fresh parameters each step without a dpp_counter_add launch.
 * splits: workgroups per crop (a power of two dividing dsz*dsz/4; 0 = choose so that the grid fills the chip). */
int dpp_augment(const float* img, const float* com3d, const float* cube, const float* Mcrop, const float* gt3d,
                int B, int J, int dsz, const int* mode, const double* off, const double* rot, const double* sc,
                const int* mode_table, int n_modes, unsigned long long seed, unsigned long long counter,
                double sigma_com, double sigma_sc, double rot_range, double fx, double fy, double ux, double uy,
                int flip_y, int norm_zero_one, const float* pca_mean, const float* pca_comp, int E, void* records,
                float* out_x, float* out_y, int* out_mode, unsigned long long* counter_dev, unsigned* ticket,
                unsigned long long sample0, unsigned long long global_batch, int splits, dpp_stream_t stream);

/* ---- initial crop: HandDetector.cropArea3D (docom = False) fused with Dataset.imgStackDepthOnly -------------------------
 * /root/reference/src/util/handdetector.py:53-68, 204-226, 260-296, 382-490; /root/reference/src/data/dataset.py:97-103.
 * frames: [B][H][W] raw depth in mm (0 = not defined); com: [B][3] crop centre in IMAGE coordinates (u, v, d mm);
 * cube: [B][3] metric crop size in mm.  prepare: per frame the detector's valid depth range [max(10, min), min(1500, max)],
 * the crop window (comToBounds), the aspect-preserving nearest-neighbour resize geometry (cv2.resize INTER_NEAREST) and the
 * crop transform M_out [B][9] (= comToTransform; may be NULL).  warp: out [B][dsz][dsz]: the crop in mm with background
 * nd_value (normalize == 0, what cropArea3D returns) or normalised like the training stacks: 0 -> com_z + cube_z/2, then
 * (d - com_z) / (cube_z / 2) (normalize != 0).  stretch != 0: the window is resized to dsz x dsz as it is (no aspect-preserving
 * size, no centred paste): `resizeCrop(cropped, dsize)`, the image cropArea3D shows its refinement net (handdetector.py:430). */
size_t dpp_crop_record_bytes(void);
int dpp_crop_prepare(const float* frames, int B, int H, int W, const float* com, const float* cube, double fx, double fy,
                     int dsz, int stretch, void* records, float* M_out, dpp_stream_t stream);
int dpp_crop_warp(const float* frames, const void* records, int B, int H, int W, int dsz, int normalize, float nd_value,
                  float* out, dpp_stream_t stream);
/* docom = True (handdetector.py:413-427): the centre of mass (calculateCoM, :91-108) of the crop window described by
 * `records`, in image coordinates -> com_out [B][3]; re-run dpp_crop_prepare with it, then dpp_crop_warp. */
size_t dpp_crop_com_workspace_bytes(int B);       /* device scratch of dpp_crop_com: per-band partial sums, summed in a fixed order */
int dpp_crop_com(const float* frames, const void* records, int B, int H, int W, void* workspace, float* com_out, dpp_stream_t stream);
/* docom = True WITH a refinement net (handdetector.py:429-440 and refineCoM, :634-676), batched: net_out [B][3] is the net's
 * output for the re-centred crops (normalised offset of the hand centre), com_in [B][3] the centre those crops were cut around
 * (dpp_crop_com's output), records the crop records of that second dpp_crop_prepare.
 *   com_out [B][3]  = joint3DToImg(net_out * cube_z / 2 + jointImgTo3D(com_in)); an all-zero result takes the depth of the crop
 *                     window's centre pixel.  Re-run dpp_crop_prepare / dpp_crop_warp with it (any dsz) for the final crop.
 * Optional, for a refine -> re-crop -> regress cascade that never leaves the device (importers.py:388-392, dataset.py:103,
 * poseregnettrainer.py:262): gt3d_orig [B][J][3] -> gt3d_crop = gt3d_orig - jointImgTo3D(com_out) (may be NULL), com3d_out
 * [B][3] (may be NULL) and out_y = gt3d_crop / (cube_z / 2), projected onto the PCA prior when pca_comp [E][J*3] / pca_mean are
 * given ([B][E]) and raw otherwise ([B][J*3]).  (fx, fy, ux, uy, flip_y): the importer's camera, signs included. */
int dpp_crop_refine(const float* frames, const void* records, int B, int H, int W, const float* com_in, const float* cube,
                    const float* net_out, double fx, double fy, double ux, double uy, int flip_y, const float* gt3d_orig, int J,
                    const float* pca_mean, const float* pca_comp, int E, float* com_out, float* com3d_out, float* gt3d_crop,
                    float* out_y, dpp_stream_t stream);

/* ---- HandDetector crop helpers (ABI v12) ----------------------------------------------------------------------------------------
 * bilinear: HandDetector.bilinearResize (/root/reference/src/util/handdetector.py:132-202) -- the reference's arithmetic on NumPy 1:
 * x_ratio = (sw - 1) / dw, int() truncation, the four tap weights in f64, more than two taps equal to nd_value -> nd_value, a tap
 * equal to nd_value drops out with the reference's re-balancing, weights renormalised by 1 / sum, all-zero weights -> nd_value, the
 * weighted sum in f64 rounded once to f32.  A source narrower or shorter than 2 pixels is DPP_E_BADARG (the reference raises
 * "Shape mismatch").  Nearest neighbour is cv2.resize INTER_NEAREST of OpenCV 2.4 (resizeNN), as in dpp_crop_warp.
 *
 * crop_warp_ex: dpp_crop_warp with the options of cropArea3D / applyCrop3D (handdetector.py:353-380, 382-490) under every
 * resizeMethod: flags bit 0 normalise (as dpp_crop_warp's `normalize`), bit 1 bilinear resize of the window (ND value nd_value),
 * bit 2 no detector range test (applyCrop3D crops an arbitrary image), bit 3 no z-threshold (thresh_z = False).  fill_value fills the
 * output outside the paste, pad_value the window outside the frame (getCrop's `background`).  flags = 0, fill_value = nd_value and
 * pad_value = 0 give dpp_crop_warp's output.  Records from dpp_crop_prepare (stretch included). */
int dpp_crop_warp_ex(const float* frames, const void* records, int B, int H, int W, int dsz, int flags, float nd_value, float fill_value,
                     float pad_value, float* out, dpp_stream_t stream);
/* resizeCrop (handdetector.py:336-351) of B same-size crops src [B][sh][sw] -> out [B][dh][dw]: nearest neighbour (bilinear == 0)
 * or bilinearResize with nd_value. */
int dpp_resize_crops(const float* src, int B, int sh, int sw, int dh, int dw, int bilinear, float nd_value, float* out, dpp_stream_t stream);
/* recropHand (handdetector.py:782-803), batched, on crops in mm [B][h][w] -> out [B][th][tw]: cv2.warpPerspective with the matrix
 * dot(M[b], Mnew[b]) (M, Mnew: [B][9] f64, row-major; product and cofactor inverse in the order of the augmentation's warp),
 * INTER_NEAREST, BORDER_CONSTANT background; then isclose(warped, nv_val) -> background and, when thresh_z, the z-threshold against
 * zrange [B][2] = (zstart, zend) in f32 (the host takes them from comToBounds; may be NULL when !thresh_z). */
int dpp_recrop(const float* crops, int B, int h, int w, const double* M, const double* Mnew, int th, int tw, float background,
               double nv_val, int thresh_z, const float* zrange, float* out, dpp_stream_t stream);
/* getInverseCrop (handdetector.py:298-334), batched: crop b [ch][cw] resized (nearest neighbour, or bilinearResize with nd_value)
 * to its window bounds [B][4] = (xstart, xend, ystart, yend) and pasted into out [B][H][W], a canvas of `background`; then, when
 * thresh_z, the z-threshold against zrange [B][2] over the whole frame.  The reference's early returns (window entirely left of /
 * above the frame, entirely right of / below it, zero width or height) give the bare canvas without the threshold.  A window of
 * negative width or height pastes nothing (the reference fails in cv2.resize; the host refuses it). */
int dpp_inverse_crop(const float* crops, int B, int ch, int cw, const int* bounds, const float* zrange, int H, int W, int bilinear,
                     float nd_value, float background, int thresh_z, float* out, dpp_stream_t stream);

/* ---- realtime tracking: a depth frame in, the followed hand's pose out (ABI v13) --------------------------------------------
 * HandDetector.track / refineCoMIterative (handdetector.py:504-567) and RealtimeHandposePipeline.detect / estimatePose
 * (realtimehandposepipeline.py:296-370) as device steps, so that one frame is one launch plan with its state (the last centre) on
 * the device (hipdp/tracker.py).
 * frame_range: min / max of every frame over many workgroups -> partial (dpp_frame_range_bytes(B) bytes); once per frame.
 * crop_prepare_ranged: dpp_crop_prepare from those partials instead of a pass of its own over the frame: the same records and M.
 *   A centre whose depth is isclose to 0 or that is not finite gets an EMPTY window (see track_refine) instead of a division by zero.
 * track_refine: dpp_crop_refine's centre update (com' = joint3DToImg(net_out * cube_z/2 + jointImgTo3D(com_in)), centre-pixel
 *   fallback from records_in) fused with the prepare of the final dsz x dsz crop around com' (records_out, M_out [B][9] or NULL,
 *   com3d_out = jointImgTo3D(com')) and status [B]: 0 ok, 1 lost -- the new centre's depth is isclose to 0 (comToBounds' "CoM
 *   ill-defined" branch) or not finite, or com_in already was; a lost frame gets an empty window (its crop is all fill value / zeros when normalised), M =
 *   identity and com3D = 0.  (fx, fy, ux, uy, flip_y) is the importer's camera, (crop_fx, crop_fy) what HandDetector was given.
 *   com_out may be com_in and records_out may be records_in.
 * dpp_crop_warp_ex flag DPP_CROP_FLIP_X: output column x takes the value of column dsz - 1 - x (crop[:, ::-1], HAND_RIGHT).
 * pose_finish: net_out [B][J][3] -> pose3d = signs(net_out) * cube_z / 2. + com3d (float32 step by step) and pose_img =
 *   joints3DToImg(pose3d); flags: 1 HAND_RIGHT (x negated), 2 invX (column 1 negated, as the reference has it), 4 invY (column 0).
 * refine_com_iterative: refineCoMIterative for B frames, all num_iter iterations in one launch (one workgroup per frame, float64
 *   state); status [B] = 1 where a centre's depth became isclose to 0 (the host handles that frame). */
#define DPP_CROP_FLIP_X 16
size_t dpp_frame_range_bytes(int B);
int dpp_frame_range(const float* frames, int B, int H, int W, float* partial, dpp_stream_t stream);
int dpp_crop_prepare_ranged(const float* partial, int B, const float* com, const float* cube, double fx, double fy, int dsz, int stretch,
                            void* records, float* M_out, dpp_stream_t stream);
int dpp_track_refine(const float* frames, const void* records_in, int B, int H, int W, const float* com_in, const float* cube,
                     const float* net_out, double fx, double fy, double ux, double uy, int flip_y, double crop_fx, double crop_fy, int dsz,
                     float* com_out, float* com3d_out, void* records_out, float* M_out, int* status, dpp_stream_t stream);
int dpp_pose_finish(const float* net_out, int B, int J, const float* cube, const float* com3d, double fx, double fy, double ux, double uy,
                    int flip_y, int flags, float* pose3d, float* pose_img, dpp_stream_t stream);
int dpp_refine_com_iterative(const float* frames, const float* partial, int B, int H, int W, const float* com_in, const float* cube,
                             double fx, double fy, int num_iter, float* com_out, int* status, dpp_stream_t stream);

/* ---- several tracks over several frames (ABI v16) -------------------------------------------------------------------------------
 * The five tracking launches for T tracks over C frames (hipdp/multitrack.py): every row t of com / cube / records / net_out /
 * the outputs is one track, and three int32 device arrays with one entry per track say
 *   src[t]     which frame of `frames` [C][H][W] (and which frame's partials of dpp_frame_range at B = C) track t reads; the
 *              caller guarantees 0 <= src[t] < C, the kernels do not check it;
 *   gate[t]    0: the track sits this launch out;
 *   tflags[t]  the track's own dpp_pose_finish flags (1 HAND_RIGHT, 2 invX, 4 invY).
 * With src[t] = t, gate[t] = 1 and tflags[t] = flags every entry point gives the bytes of its plain sibling (the same kernel bodies).
 * crop_prepare_ranged_ix: a gated track gets the empty window, like an ill-defined centre.
 * crop_warp_ix / crop_warp_ex_ix: row t is cropped from frame src[t]; crop_warp_ex_ix sets DPP_CROP_FLIP_X per row from
 *   tflags[t] & 1 (the bit is refused in `flags`), the remaining flags hold for all rows.
 * track_refine_ix: a gated track keeps com_out[t] = com_in[t] bit for bit and gets status DPP_TRACK_IDLE, the empty window,
 *   M = identity and com3D = 0; it is never reported lost.
 * pose_finish_ix: the sign rules of row t come from tflags[t]. */
#define DPP_TRACK_OK 0
#define DPP_TRACK_LOST 1
#define DPP_TRACK_IDLE 2
int dpp_crop_prepare_ranged_ix(const float* partial, int T, const int* src, const int* gate, const float* com, const float* cube, double fx,
                               double fy, int dsz, int stretch, void* records, float* M_out, dpp_stream_t stream);
int dpp_crop_warp_ix(const float* frames, const void* records, int T, const int* src, int H, int W, int dsz, int normalize, float nd_value,
                     float* out, dpp_stream_t stream);
int dpp_track_refine_ix(const float* frames, const void* records_in, int T, const int* src, const int* gate, int H, int W,
                        const float* com_in, const float* cube, const float* net_out, double fx, double fy, double ux, double uy, int flip_y,
                        double crop_fx, double crop_fy, int dsz, float* com_out, float* com3d_out, void* records_out, float* M_out,
                        int* status, dpp_stream_t stream);
int dpp_crop_warp_ex_ix(const float* frames, const void* records, int T, const int* src, const int* tflags, int H, int W, int dsz, int flags,
                        float nd_value, float fill_value, float pad_value, float* out, dpp_stream_t stream);
int dpp_pose_finish_ix(const float* net_out, int T, int J, const int* tflags, const float* cube, const float* com3d, double fx, double fy,
                       double ux, double uy, int flip_y, float* pose3d, float* pose_img, dpp_stream_t stream);

/* ---- sensor frames (ABI v15): uint16 / float32 ingest, mirror, 3x3 median (csrc/ingest.hip) ----------------------------------------
 * What the reference's live depth source does to every frame (src/util/cameradevice.py:189-200 of the reference): optional mirror,
 * cv2.medianBlur(depth, 3) with its replicated border, conversion to float32 -- in one launch that also writes frame_range's
 * partials, so that it REPLACES dpp_frame_range in a plan:
 *   frames[b][y][x] = float32( median of the nine raw[b][clamp(y + dy, 0, H - 1)][clamp(xs + dx, 0, W - 1)] ),
 *   xs = W - 1 - x under DPP_INGEST_MIRROR_X, else x; without DPP_INGEST_MEDIAN3 the conversion (and the mirror) alone.
 * raw [B][H][W] of src_type (DPP_INGEST_U16: uint16, DPP_INGEST_F32: float32); frames [B][H][W] float32, must not overlap raw.  The
 * median is selected in the source type by comparisons only (uint16 -> float32 is exact), so the result is bit for bit that of
 * cv2.medianBlur / scipy.ndimage.median_filter(size=3, mode='nearest'); the mirror commutes with it.  A float32 source must be free
 * of NaN (a NaN makes the comparisons, and so the selection, meaningless); which of -0.0 / +0.0 is selected among equal zeros and
 * the handling of subnormals are not part of the contract.
 * partial: NULL, or dpp_frame_range's workspace (dpp_frame_range_bytes(B) bytes): EVERY band's (min, max) over the float32 values
 * stored to frames is written, an empty band (H below the band count) gets dpp_frame_range's identities (3.4e38f, -3.4e38f).
 * DPP_E_BADARG (nothing launched): NULL raw / frames, overlapping raw and frames, B / H / W below 1, B above 65535, H * W above
 * 2^31 - 1, an unknown src_type, unknown flag bits. */
#define DPP_INGEST_U16 1
#define DPP_INGEST_F32 2
#define DPP_INGEST_MEDIAN3 1
#define DPP_INGEST_MIRROR_X 2
int dpp_frame_ingest(const void* raw, int src_type, int B, int H, int W, int flags, float* frames, float* partial, dpp_stream_t stream);

/* ---- frame sources of unlike cameras and frame sizes (ABI v19) ------------------------------------------------------------------------
 * The tracking launches that read a frame or a camera, for C frame sources that each have a camera and a frame size of their own
 * (hipdp/multitrack.py).  `sources` is a device array of C records of dpp_source_record_bytes() bytes:
 *   double fx, fy, ux, uy;         the importer's camera, signs included (to3d / toimg of track_refine and pose_finish)
 *   double crop_fx, crop_fy;       what the reference hands to HandDetector: abs(config fx / fy) (the crop geometry)
 *   int64  frame_off, raw_off;     ELEMENT offset of the source's frame in the float32 frame buffer / in the raw sensor buffer
 *   int32  H, W, flip_y, (pad);    the frame size; whether the camera flips the y axis
 * The frames are ragged: source c's H x W floats start at frames + frame_off (raw: raw + raw_off elements of the sensor type); the
 * host pads every offset to 16 bytes, the pad elements are never read or written.  The host validates the table once (offsets in range
 * and aligned, H, W > 0, focal lengths != 0, raw and frames apart); the kernels trust it as they trust src[].  Row t of the
 * track launches reads record src[t] (0 <= src[t] < C); the partials are dpp_frame_range's at B = C.
 * These are the kernels of the plain and *_ix entry points with the table in place of the launch's (H, W, fx, fy, ux, uy, flip_y,
 * crop_fx, crop_fy): with C equal records they give the bytes of the *_ix launches.  frame_ingest_src: band b of source c covers
 * ceil(H_c / 64) rows of that source; an empty band writes its identities as in dpp_frame_ingest.
 * DPP_E_BADARG (nothing launched): a NULL pointer (M_out and frame_ingest_src's partial may be NULL), T / C / J / dsz below 1, C above
 * 65535, raw == frames, an unknown src_type or flag bit (DPP_CROP_FLIP_X comes from tflags, as in crop_warp_ex_ix). */
size_t dpp_source_record_bytes(void);
int dpp_frame_range_src(const float* frames, const void* sources, int C, float* partial, dpp_stream_t stream);
int dpp_frame_ingest_src(const void* raw, int src_type, const void* sources, int C, int flags, float* frames, float* partial,
                         dpp_stream_t stream);
int dpp_crop_prepare_ranged_src(const float* partial, int T, const int* src, const int* gate, const void* sources, const float* com,
                                const float* cube, int dsz, int stretch, void* records, float* M_out, dpp_stream_t stream);
int dpp_crop_warp_src(const float* frames, const void* records, int T, const int* src, const void* sources, int dsz, int normalize,
                      float nd_value, float* out, dpp_stream_t stream);
int dpp_track_refine_src(const float* frames, const void* records_in, int T, const int* src, const int* gate, const void* sources,
                         const float* com_in, const float* cube, const float* net_out, int dsz, float* com_out, float* com3d_out,
                         void* records_out, float* M_out, int* status, dpp_stream_t stream);
int dpp_crop_warp_ex_src(const float* frames, const void* records, int T, const int* src, const int* tflags, const void* sources, int dsz,
                         int flags, float nd_value, float fill_value, float pad_value, float* out, dpp_stream_t stream);
int dpp_pose_finish_src(const float* net_out, int T, int J, const int* src, const int* tflags, const void* sources, const float* cube,
                        const float* com3d, float* pose3d, float* pose_img, dpp_stream_t stream);

/* ---- tracks of one hand across calibrated cameras (ABI v20; csrc/fuse.hip) --------------------------------------------------------------
 * ONE launch at the end of MultiTracker's tick (hipdp/multitrack.py) that fuses the tracks which observe the same physical hand from
 * different frame sources, and hands a track that lost the hand the centre its peers see.  The reference has no counterpart (one
 * device, one camera): these semantics are THIS PROJECT'S OWN, restated in NumPy by tests/fuse_ref.py and pinned to it bit for bit.
 * All arithmetic is float64 in the order given (no FMA contraction); every output is rounded to float32 once.
 *   extrinsics [C][12] float64: R (3 x 3, row-major) then t (mm) of every source; w = R p + t takes a point of the source's camera
 *              frame (the importer's jointImgTo3D frame, flip_y included: the frame of pose3d / com3d) to the common world frame.
 *              Row i is ((R_i0 x + R_i1 y) + R_i2 z) + t_i.  The inverse p = R^T (w - t): d = w - t, row i (R_0i d0 + R_1i d1) + R_2i d2.
 *   members / offsets [G + 1]: group g is the tracks members[offsets[g] .. offsets[g + 1]), in that (list) order; 1 to
 *              DPP_FUSE_MAX_MEMBERS of them, groups disjoint, a group's members on pairwise distinct sources.  The host has validated
 *              all of it (and R orthonormal, det > 0); the kernel trusts the arrays as it trusts src[].  Tracks in no group are not
 *              touched: none of their outputs is written.
 * Per group, one workgroup:
 *   1. contributors: the members with status[m] == DPP_TRACK_OK; world centre W_m = R com3d[m] + t of the member's source.
 *   2. consistency, only with max_dev > 0 (0: off).  n >= 3 contributors: the componentwise median of the W_m (even n: (a + b) / 2 of
 *      the two middle values); a contributor with sqrt((dx^2 + dy^2) + dz^2) > max_dev from it is an OUTLIER and stops contributing
 *      (all decided at once against the one median).  n == 2 farther apart than max_dev: both get DISAGREE and both still contribute.
 *   3. over the remaining contributors (the inliers, n_out[g] of them) in list order, sums starting from 0.0:
 *      fused_com [G][3] = sum of W_m / n; fused_pose [G][J][3] = sum of (R pose3d[m][j] + t) / n; spread [G][J] = the largest distance
 *      of an inlier's world joint from the (unrounded) fused joint.  n == 0: all zeros.
 *   4. peer_com [T][3], per member t: the mean world centre of the inliers OTHER than t (sum in list order / count), brought into t's
 *      camera frame, rounded to float32, projected by t's own camera with joint3DToImg on a float32 array (as pose_finish does) ->
 *      (u, v, z).  PEER_OK: such an inlier exists, z > 0 and the centre is not ill-defined (finite, |z| > 1e-8), 0 <= u < W and
 *      0 <= v < H of t's source.  No such inlier: (0, 0, 0).
 *   5. hand-over (flags & DPP_FUSE_HANDOVER): a member with PEER_OK whose status is DPP_TRACK_LOST, or which is an OUTLIER, gets
 *      com[t] = peer_com[t] and HANDED.  No other centre is written; a gated member (DPP_TRACK_IDLE) is never rewritten.
 *   6. fstat [T]: USED (an inlier) | OUTLIER | DISAGREE | PEER_OK | HANDED.
 * sources: NULL (every source has the camera and the H x W of the launch scalars) or the ABI v19 table.  src, status [T] int32;
 * pose3d [T][J][3], com3d [T][3], com [T][3] float32 (com is only written).
 * DPP_E_BADARG (nothing launched): a NULL pointer (sources may be NULL), T / J / C / G below 1, G above T, max_dev negative or not
 * finite, an unknown flag bit, and without a table H / W below 1 or a zero focal length. */
#define DPP_FUSE_MAX_MEMBERS 16
#define DPP_FUSE_USED 1
#define DPP_FUSE_OUTLIER 2
#define DPP_FUSE_DISAGREE 4
#define DPP_FUSE_PEER_OK 8
#define DPP_FUSE_HANDED 16
#define DPP_FUSE_HANDOVER 1 /* launch flag */
int dpp_pose_fuse(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* extrinsics, int C,
                  const int* members, const int* offsets, int G, const void* sources, int H, int W, double fx, double fy, double ux, double uy,
                  int flip_y, double max_dev, int flags, float* com, float* fused_pose, float* fused_com, float* spread, int* n_out,
                  float* peer_com, int* fstat, dpp_stream_t stream);
/* The same launch with a weight per track and joint (ABI v23; the weights that dpp_joint_visibility writes, or any finite weights >= 0):
 * weight [T][J] float32 (read only), fused_weight [G][J] float32.  Contributors, the median test, outliers, n, fused_com, peer_com,
 * the hand-over and fstat are those of dpp_pose_fuse and do not read the weights.  Per joint j, over the inliers m in list order, sums
 * starting from 0.0, W_mj = R pose3d[m][j] + t and w_m = weight[m][j]: sw = sw + (double) w_m; per coordinate
 * sum = sum + (double) w_m * W_mj (a product, then an add: no contraction).
 *   sw > 0:  fused_pose[g][j] = sum / sw; spread[g][j] = the largest distance from that (unrounded) joint of the W_mj of an inlier with
 *            w_m > 0; fused_weight[g][j] = the largest w_m.
 *   sw == 0 (nobody sees the joint): fused_pose and spread are dpp_pose_fuse's -- the unweighted mean, the spread over all inliers --
 *            and fused_weight[g][j] = 0.
 *   n == 0:  all zeros, fused_weight included.
 * So weights that are all 1.0f (1.0 * x is exact, sw == n) and weights that are all 0 both give dpp_pose_fuse's bytes in every output.
 * DPP_E_BADARG: dpp_pose_fuse's cases, and a NULL weight or fused_weight.  The weights themselves are not checked. */
int dpp_pose_fuse_w(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* extrinsics, int C,
                    const int* members, const int* offsets, int G, const void* sources, int H, int W, double fx, double fy, double ux,
                    double uy, int flip_y, double max_dev, int flags, float* com, float* fused_pose, float* fused_com, float* spread,
                    int* n_out, float* peer_com, int* fstat, const float* weight, float* fused_weight, dpp_stream_t stream);

/* ---- extrinsics of a camera from the tracked hand (ABI v21; csrc/calib.hip) ---------------------------------------------------------------
 * dpp_pose_fuse needs an (R, t) per source.  The tracker already has the correspondences for a rigid fit: every tick the same J joints
 * of the same hand in each camera's frame.  ONE launch at the end of a calibrating MultiTracker's tick (in place of dpp_pose_fuse) adds
 * the tick's joint pairs to running sums; the fit itself -- Kabsch on a 3 x 3 matrix, once per calibration -- is host work
 * (hipdp/calib.py: solve_rigid).  No counterpart in the reference: THIS PROJECT'S OWN semantics, restated in NumPy by tests/calib_ref.py
 * and pinned to it bit for bit.  All arithmetic is float64 in the order given (no FMA contraction, no atomics).
 *   pose3d, status, src, extrinsics, members, offsets: as for dpp_pose_fuse (read only).  Of `extrinsics` only the row of `anchor` is read.
 *   anchor:    the source whose (R, t) is known; cal_src: n_cal sources to calibrate, a HOST array of 1 .. DPP_CALIB_MAX_SOURCES
 *              entries that the entry point checks and copies into the launch's arguments.
 *   acc [n_cal][DPP_CALIB_SLOTS] float64, device, updated in place: row k belongs to source c = cal_src[k].  Slots: 0 n; 1..3 sum p;
 *              4..6 sum q; 7..15 S[d][e] = sum p_d q_e (d the row); 16 sum |p|^2; 17 sum |q|^2; 18 pairs; 19 refused.
 * One workgroup of one wave (64 lanes) per k.  Every lane starts with all-zero private partials v[0..17].  The groups in ascending order:
 *   a = the group's member with src == anchor, m = its member with src == c (at most one each).  The group takes part in this launch
 *   only if both exist and status[a] == status[m] == DPP_TRACK_OK.  For joint j: p = (double) pose3d[m][j], q = R_a (double) pose3d[a][j]
 *   + t_a by dpp_pose_fuse's row rule.  Lane l takes the joints j = l, l + 64, ... in ascending order.
 *   Shape gate, only with max_shape_dev > 0 (0: off): lane partial sums of p and of q over its joints (from 0.0), each of the six reduced
 *   by the butterfly below, divided by (double) J: the centroids pc, qc.  dev_j = |dist(p_j, pc) - dist(q_j, qc)| with dist =
 *   sqrt((dx^2 + dy^2) + dz^2); per lane worst = fmax(worst, dev_j) from 0.0, over the wave v = fmax(v, shfl_xor(v, off)), off = 32 .. 1.
 *   The pair is refused (refused += 1, nothing else changes) unless worst <= max_shape_dev.
 *   A pair that takes part: pairs += 1, and per joint of the lane, in this order: v0 += 1; v[1 + d] += p_d; v[4 + d] += q_d;
 *   v[7 + 3 d + e] += p_d * q_e; v16 += (p0 p0 + p1 p1) + p2 p2; v17 += (q0 q0 + q1 q1) + q2 q2.
 * After the last group each of the 18 partials is reduced over the wave: off = 32, 16, 8, 4, 2, 1: v = v + shfl_xor(v, off) (both
 * partners form the same sum, every lane ends with the same bits), then acc[k][i] = acc[k][i] + v_i once, acc[k][18] += pairs and
 * acc[k][19] += refused (both counted in float64).  A source that shares no group with the anchor leaves its row as it was.
 * DPP_E_BADARG (nothing launched): a NULL pointer, T / J / C / G below 1, G above T, n_cal outside 1 .. DPP_CALIB_MAX_SOURCES, anchor or
 * an entry of cal_src outside [0, C), anchor in cal_src, max_shape_dev negative or not finite. */
#define DPP_CALIB_MAX_SOURCES 32
#define DPP_CALIB_SLOTS 20
int dpp_extrinsics_accumulate(const float* pose3d, const int* status, const int* src, int T, int J, const double* extrinsics, int C,
                              const int* members, const int* offsets, int G, int anchor, const int* cal_src, int n_cal, double max_shape_dev,
                              double* acc, dpp_stream_t stream);

/* ---- tracked and fused poses smoothed over the ticks (ABI v22; csrc/smooth.hip) ----------------------------------------------------------
 * The trackers return every tick's joints as the pose net regressed them from that tick's crop; nothing connects one tick to the next.
 * ONE launch at the very end of a tracker's tick (behind dpp_pose_fuse / dpp_extrinsics_accumulate where the plan has one) runs the
 * One-Euro filter (Casiez, Roussel, Vogel, CHI 2012: a first-order low-pass whose cut-off rises with the filtered speed) over every
 * track's pose and every group's fused pose.  Its state lives on the device and is never downloaded.  The reference has no counterpart
 * (it draws what the net returns): these semantics are THIS PROJECT'S OWN, restated in NumPy float64 by tests/smooth_ref.py and pinned
 * to it bit for bit.  All arithmetic is float64 in the order given (+ - * / sqrt, no FMA contraction); every output is rounded to
 * float32 once.
 * Rows.  R = T + G rows of J x 3 values.  Row r < T is track r: its sample x is pose3d[r] (float32, camera frame, mm), VALID iff
 *   status[r] == DPP_TRACK_OK.  Row T + g is group g: its sample is fused_pose[g] (float32, world frame), VALID iff n[g] >= 1.  G may be
 *   0: fused_pose, n, fused_pose_f and gstat may then be NULL.
 * State, device memory, updated in place: since [R] int32 -- the ticks since the row's last valid sample, -1: the row is empty (what a
 *   fresh state holds, and what the host writes to clear a row); xh [R][J][3] float64, the filtered value; dxh [R][J][3] float64, the
 *   filtered derivative (mm / s).  xh / dxh are not read while since < 0, so only `since` needs initialising.
 * Parameters, launch scalars: rate (ticks per second), mincutoff (Hz), beta (Hz per mm / s), dcutoff (Hz), max_hold (ticks).
 * alpha(fc, Te) = r / (r + 1.0) with r = (6.283185307179586 * fc) * Te.  Per row:
 *   valid, since < 0:   xh = x, dxh = 0, since = 0; word DPP_SMOOTH_INIT.
 *   valid, since >= 0:  Te = (double)(since + 1) / rate, ad = alpha(dcutoff, Te).  Per joint and coordinate d = (x - xh) / Te, then
 *                       dxh = ad * d + (1.0 - ad) * dxh.  Per joint speed = sqrt((dxh0^2 + dxh1^2) + dxh2^2), fc = mincutoff + beta * speed,
 *                       a = alpha(fc, Te); per coordinate xh = a * x + (1.0 - a) * xh.  Then since = 0; word DPP_SMOOTH_OK.
 *   not valid, since < 0:                       word DPP_SMOOTH_EMPTY, all outputs of the row zero.
 *   not valid, since >= 0, since + 1 > max_hold: since = -1 (the state is dropped; xh / dxh keep their bits, unread); word
 *                       DPP_SMOOTH_EMPTY | DPP_SMOOTH_DROPPED, all outputs of the row zero.
 *   not valid, since >= 0, otherwise:           since += 1; word DPP_SMOOTH_HELD, the outputs are those of the unchanged xh.
 * Outputs: pose_f [T][J][3] = (float) xh; pose_img_f [T][J][3] = that float32 joint projected by the track's own camera with
 *   joint3DToImg on a float32 array, exactly as dpp_pose_finish projects pose3d (an EMPTY row is all zeros: it is not projected);
 *   sstat [T] the track's word; fused_pose_f [G][J][3] and gstat [G] the same for the group rows, which have no projection.
 * Camera: sources == NULL (src may then be NULL too: every track has the camera of the launch scalars) or the ABI v19 table with src [T].
 * One workgroup of one wave per row; lanes stride over the joints, a joint's three coordinates in one lane; vector loads and stores
 * only, no atomics.  Ticks on one state must be stream-ordered.
 * DPP_E_BADARG (nothing launched): a NULL required pointer (the four group pointers may be NULL only with G == 0; sources and src may
 * be NULL together, a table needs src); T / J below 1, G or max_hold below 0; rate, mincutoff or dcutoff not finite or <= 0; beta not
 * finite or < 0; without a table a zero focal length. */
#define DPP_SMOOTH_OK 1
#define DPP_SMOOTH_INIT 2
#define DPP_SMOOTH_HELD 4
#define DPP_SMOOTH_EMPTY 8
#define DPP_SMOOTH_DROPPED 16
int dpp_pose_smooth(const float* pose3d, const int* status, const int* src, int T, int J, const float* fused_pose, const int* n, int G,
                    const void* sources, double fx, double fy, double ux, double uy, int flip_y, double rate, double mincutoff, double beta,
                    double dcutoff, int max_hold, int* since, double* xh, double* dxh, float* pose_f, float* pose_img_f, int* sstat,
                    float* fused_pose_f, int* gstat, dpp_stream_t stream);

/* ---- which joints of a tracked pose the frame shows (ABI v23; csrc/visibility.hip) --------------------------------------------------------
 * The reason to point a second camera at a hand is that the first does not see all of it; the evidence is on the device at the end of
 * every tick: dpp_pose_finish writes each joint as (u, v, z) in its source's frame, and the float32 frame is still in the frame buffer.
 * ONE launch behind dpp_pose_finish (before dpp_pose_fuse_w / dpp_extrinsics_accumulate / dpp_pose_smooth where the plan has them)
 * classifies every joint of all T tracks by the depths around its pixel.  The reference has no counterpart: these semantics are THIS
 * PROJECT'S OWN, restated in NumPy float64 by tests/visibility_ref.py and pinned to it bit for bit.  Comparisons are float64 in the
 * order given (no FMA contraction); every float output is rounded to float32 once.
 * Inputs (read only): pose_img [T][J][3] float32; status [T], src [T] int32; frames, the float32 frame buffer: [C][H][W] with the
 *   launch's H, W (sources == NULL), or the ragged buffer of the ABI v19 table `sources`, whose record src[t] gives track t's H, W and
 *   offset.  The frames must be free of NaN, as for dpp_frame_ingest.  The kernel trusts src[] as every tracking launch does.
 * Parameters: radius (0 .. DPP_VIS_MAX_RADIUS), margin (mm, > 0 and finite), min_support (1 .. (2 radius + 1)^2), hidden_weight
 *   (in [0, 1]).
 * Per track t and joint j with (u, v, z) = pose_img[t][j]:
 *   status[t] != DPP_TRACK_OK: the whole row is WRITTEN as zeros (vis 0, weight 0, vword 0).
 *   px = floor((double) u + 0.5), py = floor((double) v + 0.5), compared as doubles before any conversion to int.
 *   DPP_VIS_OFFFRAME: any of u, v, z not finite, or z <= 0, or px outside [0, W), or py outside [0, H) of the track's source: vis = 0,
 *     weight = 0.
 *   Otherwise the window is the pixels (px + dx, py + dy), |dx|, |dy| <= radius, that lie inside the frame: n_in >= 1 of them.  With d
 *     the pixel's value as double: d == 0 is EMPTY; else d - z < -margin is FRONT; else d - z > margin is BEHIND; else ON.
 *   vis [T][J] = (float) ((double) n_on / (double) n_in).
 *   vword [T][J], exactly one class: DPP_VIS_VISIBLE if n_on >= min_support, else DPP_VIS_OCCLUDED if n_front >= min_support, else
 *     DPP_VIS_UNSUPPORTED (guessed onto background or into a hole).
 *   weight [T][J] = 1.0f when VISIBLE, else (float) hidden_weight.
 * One workgroup of one wave per (track, joint), lanes over the window's pixels; the counts are integers, so the order of their
 * reduction is free.  Vector loads and stores only, no atomics.
 * DPP_E_BADARG (nothing launched): a NULL pointer (sources may be NULL); T / J / C below 1; radius outside 0 .. DPP_VIS_MAX_RADIUS;
 * min_support outside 1 .. (2 radius + 1)^2; margin not finite or <= 0; hidden_weight outside [0, 1] (NaN included); without a table
 * H or W below 1. */
#define DPP_VIS_MAX_RADIUS 8
#define DPP_VIS_VISIBLE 1
#define DPP_VIS_OCCLUDED 2
#define DPP_VIS_UNSUPPORTED 4
#define DPP_VIS_OFFFRAME 8
int dpp_joint_visibility(const float* pose_img, const int* status, const int* src, int T, int J, const float* frames, int C,
                         const void* sources, int H, int W, int radius, double margin, int min_support, double hidden_weight, float* vis,
                         float* weight, int* vword, dpp_stream_t stream);

/* ---- every track of a tick brought to one instant (ABI v24; csrc/align.hip, dpp_pose_smooth_t in csrc/smooth.hip) -------------------------
 * Cameras without a hardware sync line are not simultaneous: two 30 Hz cameras are up to half a period apart, and a hand at 1 m / s is
 * then seen 17 mm apart by the two.  Every sensor stamps its frames.  ONE launch per tick behind dpp_pose_finish (and behind
 * dpp_joint_visibility, which compares a joint with its own frame and keeps reading the unaligned pose_img) and before dpp_pose_fuse /
 * dpp_pose_fuse_w / dpp_extrinsics_accumulate / dpp_pose_smooth_t moves every track's pose and centre from its source's stamp to the
 * tick's instant `now` along the velocity between the track's previous sample and this one.  The launches that combine tracks then read
 * pose_t / com3d_t in place of pose3d / com3d.  The reference has one camera and no counterpart: these semantics are THIS PROJECT'S
 * OWN, restated in NumPy float64 by tests/align_ref.py and pinned to it bit for bit.  All arithmetic is float64 in the order given
 * (+ - * /, no FMA contraction); every output is rounded to float32 once.
 * Inputs (read only): pose3d [T][J][3], com3d [T][3] float32 (camera frame, mm); status [T], src [T] int32; stamps [C + 1] float64 in
 *   device memory: stamps[c] is the time (s) of source c's frame of this tick, stamps[C] is `now`, the instant the tick's combined
 *   outputs refer to.  All stamps are on ONE clock and finite (the host checks).  The kernel trusts src[] as every tracking launch does.
 * Parameters, launch scalars: max_gap (s, > 0, finite), max_lead (s, >= 0, finite).
 * State, device memory, updated in place, never downloaded: have [T] int32, 0: the row is empty (what a fresh state holds, and what
 *   the host writes to clear a row); pt [T] float64, the previous stamp; pp [T][J][3], pc [T][3] float32, the previous pose and centre.
 *   pt / pp / pc are not used while have == 0, so only `have` needs initialising.
 * Per track t, with ts = stamps[src[t]], dt = ts - pt[t], lead = now - ts:
 *   status[t] != DPP_TRACK_OK:  word DPP_ALIGN_NONE; all outputs of the row are zero, the state is untouched (a stale state is refused
 *                       later by max_gap).
 *   OK, have[t] != 0, dt > 0, dt <= max_gap and fabs(lead) <= max_lead:  word DPP_ALIGN_MOVED.  Per coordinate x with its previous
 *                       value xp: v = ((double) x - (double) xp) / dt, y = (double) x + v * lead, out = (float) y; the same for the three
 *                       coordinates of com3d against pc.
 *   OK otherwise:       word DPP_ALIGN_ASIS with ONE reason bit, the first that applies: DPP_ALIGN_NOPREV (have[t] == 0), DPP_ALIGN_GAP
 *                       (not dt > 0, or dt > max_gap), DPP_ALIGN_FAR (not fabs(lead) <= max_lead).  The outputs are the inputs' bits.
 *   In both OK cases the state becomes the UNALIGNED sample afterwards: have = 1, pt = ts, pp = pose3d[t], pc = com3d[t].
 * Outputs: pose_t [T][J][3]; pose_img_t [T][J][3] = that float32 joint projected by the track's own camera with joint3DToImg on a
 *   float32 array, exactly as dpp_pose_finish projects pose3d (a NONE row is all zeros: it is not projected); com3d_t [T][3]; lead [T]
 *   float32 = (float) lead, 0 for NONE; astat [T] int32, the word.
 * Camera: sources == NULL (src may then be NULL too: every track is source 0 with the camera of the launch scalars) or the ABI v19
 *   table with src [T].
 * One workgroup of one wave per track; lanes stride over the joints, a joint's three coordinates in one lane; vector loads and stores
 * only, no atomics.  Ticks on one state must be stream-ordered.
 * DPP_E_BADARG (nothing launched): a NULL required pointer (sources and src may be NULL together, a table needs src); T / J / C below
 * 1; max_gap not finite or <= 0; max_lead not finite or < 0; without a table a zero focal length.
 * Out of scope: estimating an unknown clock offset between cameras, letting an IDLE track coast into the fusion, using the filtered
 * derivative as the velocity. */
#define DPP_ALIGN_NONE 0
#define DPP_ALIGN_MOVED 1
#define DPP_ALIGN_ASIS 2
#define DPP_ALIGN_NOPREV 4
#define DPP_ALIGN_GAP 8
#define DPP_ALIGN_FAR 16
int dpp_pose_align(const float* pose3d, const float* com3d, const int* status, const int* src, int T, int J, const double* stamps, int C,
                   const void* sources, double fx, double fy, double ux, double uy, int flip_y, double max_gap, double max_lead, int* have,
                   double* pt, float* pp, float* pc, float* pose_t, float* pose_img_t, float* com3d_t, float* lead, int* astat,
                   dpp_stream_t stream);

/* dpp_pose_smooth over real time: dpp_pose_smooth's kernel body and semantics with these differences and no others.  `rate` is not
 * an argument.  stamps [C + 1] float64 (device) as above; tlast [R] float64, one more state array (a buffer of its own, not read while
 * since < 0).  The sample time s of track row r is stamps[src[r]] (stamps[0] when src is NULL), of group row T + g stamps[C].
 *   valid, since < 0:   as dpp_pose_smooth, and tlast = s.
 *   valid, since >= 0, Te = s - tlast > 0:  as dpp_pose_smooth's OK branch with this Te, and tlast = s.
 *   valid, since >= 0, Te not > 0:  the sample is refused: the row takes the not-valid path (HELD / DROPPED / EMPTY by the max_hold
 *                       rule, which keeps counting ticks) with the additional bit DPP_SMOOTH_STALE; xh / dxh / tlast keep their bits.
 * Track rows filter the unaligned pose3d at the track's own stamps; group rows filter the fused pose at `now`.
 * DPP_E_BADARG: as dpp_pose_smooth without `rate`, and stamps or tlast NULL, C below 1. */
#define DPP_SMOOTH_STALE 32
int dpp_pose_smooth_t(const float* pose3d, const int* status, const int* src, int T, int J, const float* fused_pose, const int* n, int G,
                      const void* sources, double fx, double fy, double ux, double uy, int flip_y, const double* stamps, int C,
                      double mincutoff, double beta, double dcutoff, int max_hold, int* since, double* tlast, double* xh, double* dxh,
                      float* pose_f, float* pose_img_f, int* sstat, float* fused_pose_f, int* gstat, dpp_stream_t stream);

/* ---- a learned static background removed from the frame (ABI v25; csrc/background.hip) ------------------------------------------------------
 * A fixed depth camera sees the same desk edge, monitor or torso in every frame; the detector starts from the nearest object and the
 * crop keeps whatever lies inside the cube.  This project's own semantics (the reference has no counterpart), restated in NumPy by
 * tests/background_ref.py:
 *   model, per source and pixel, in the frames' layout:  near (float32; 0: nothing seen) the smallest non-zero depth of the learning
 *     frames, seen (int32) the number of learning frames in which the pixel had a depth.
 *   dpp_background_learn, one float32 frame f (with a sensor: dpp_frame_ingest's output), for every pixel with f != 0:
 *     near = (near == 0 || f < near) ? f : near;  seen += 1.      take [B] int32 (device): take[b] == 0 leaves frame b's model untouched.
 *   cut map (float32, the frames' layout), computed by the HOST once per model change, every operation rounded to float32:
 *     cut = near - (margin + rel * near)   where seen >= min_seen, near != 0 and the result is > 0;   +inf elsewhere.
 *   dpp_frame_background:  frames = (f != 0 && f < cut) ? f : 0, IN PLACE.  The comparison is strict: a depth exactly at cut is
 *     background.  A pure selection: nothing rounds, applying twice gives the bits of applying once, an all-+inf cut map keeps every
 *     frame (and its partials) as dpp_frame_range sees it.
 * partial: NULL, or dpp_frame_range's workspace: EVERY band's (min, max) over the values stored is written, in dpp_frame_range's
 * layout and element partition; a band without elements gets its identities (3.4e38f, -3.4e38f).  In a plan the launch stands in
 * dpp_frame_range's place (behind dpp_frame_ingest with partial NULL where there is a sensor).
 * *_src: the ragged layout of ABI v19 -- frames, cut, near and seen all start source c at element sources[c].frame_off; the padding
 * words between frames are neither read nor written.
 * DPP_E_BADARG (nothing launched, nothing written): a NULL pointer other than partial, B / C outside 1 .. 65535, H or W below 1, H * W
 * above 2^31 - 1, cut (near, seen) overlapping frames (*_src: equal to it; the host keeps the ragged buffers apart). */
int dpp_frame_background(float* frames, const float* cut, int B, int H, int W, float* partial, dpp_stream_t stream);
int dpp_frame_background_src(float* frames, const float* cut, const void* sources, int C, float* partial, dpp_stream_t stream);
int dpp_background_learn(const float* frames, const int* take, int B, int H, int W, float* near_, int* seen, dpp_stream_t stream);
int dpp_background_learn_src(const float* frames, const int* take, const void* sources, int C, float* near_, int* seen,
                             dpp_stream_t stream);

/* ---- ... kept current while tracking (additive to ABI v25: new symbols only -- DPP_ABI_VERSION stays 25, no existing prototype, record
 * or result block changes) ------------------------------------------------------------------------------------------------------
 * dpp_frame_background_adapt is dpp_frame_background -- the same grid, element partition and partials, frames cut IN PLACE by the cut
 * map AS IT STOOD BEFORE the launch -- and adapts the model from the raw depth in the same pass.  This project's own semantics,
 * restated by tests/background_adapt_ref.py.  Beside near / seen / cut, in their layout: cand (float32; 0: none), a depth that may
 * become the background, and run (int32), the consecutive adapting ticks that supported it.
 *   band(x) = float32(margin + float32(rel * x)), the cut map's roundings.
 *   One launch, for source b with take[b] != 0 (take[b] == 0: the cut alone, no model array is read) and every pixel with raw depth f:
 *     protected -- inside the window [xstart - guard, xstart + cw + guard) x [ystart - guard, ystart + ch + guard) of a track t with
 *       src[t] == b (src NULL: t == b) whose crop record records[t] has cw > 0 and ch > 0:   cand = 0, run = 0, nothing else.
 *     f == 0 (a hole):   nothing.
 *     confirm, near != 0 and float32(near - band(near)) <= f <= float32(near + band(near)):
 *       near = min(near, f); seen += 1 (saturating at 2^31 - 1); cand = 0, run = 0.
 *     candidate, everything else:   cand != 0 and float32(cand - band(cand)) <= f <= float32(cand + band(cand)):
 *       cand = min(cand, f), run += 1;   otherwise cand = f, run = 1.
 *       run >= persist:   near = cand, seen = run, cand = 0, run = 0 -- the model is replaced.
 *     where a pixel confirmed or was replaced, cut = float32(near - band(near)) where seen >= min_seen, near != 0 and the result is
 *     > 0, else +inf: the bits of the host's cut map.  The new cut applies from the next launch on.
 * records [T] crop records (dpp_crop_record_bytes() each) as dpp_track_refine left them in the previous tick: a lost or gated track
 * has the empty window and protects nothing.  records NULL or T == 0: no protection.  T is any number >= 0.
 * DPP_E_BADARG (nothing launched, nothing written): as dpp_frame_background, and any of the six buffers NULL or overlapping another
 * (*_src: equal to another), take NULL, T < 0, margin or rel not finite, min_seen < 1, persist < 2 or < min_seen, guard < 0. */
int dpp_frame_background_adapt(float* frames, float* cut, float* near_, int* seen, float* cand, int* run, const int* take, int B, int H,
                               int W, const void* records, int T, const int* src, float margin, float rel, int min_seen, int persist,
                               int guard, float* partial, dpp_stream_t stream);
int dpp_frame_background_adapt_src(float* frames, float* cut, float* near_, int* seen, float* cand, int* run, const int* take,
                                   const void* sources, int C, const void* records, int T, const int* src, float margin, float rel,
                                   int min_seen, int persist, int guard, float* partial, dpp_stream_t stream);

/* ---- whole-frame hand detection by connected components (ABI v14) -------------------------------------------------------------
 * What HandDetector.detect / estimateHandsize (handdetector.py:569-632, :911-937) take from cv2.findContours, restated with
 * 8-connected component labelling (csrc/components.hip): pixel count for contourArea, raster order for contour order, a depth
 * exactly on a slab boundary in the nearer slab only.  All launches of a frame are stream-ordered; nothing returns to the host.
 * slab_keys: keys [B][H][W] uint8 from frame_range's partials: the smallest i in [0, 20) with b_i <= d <= b_{i+1},
 *   b_i = minDepth + i * (maxDepth - minDepth) / 20 in float64; 255 (background) for d == 0 and outside [minDepth, maxDepth].
 * mask_keys: key 0 where d != 0 && com_z - cube_z / 2 <= d <= com_z + cube_z / 2 (float64, raw frame), else 255.
 * label_components: labels [B][H][W] int32 = the smallest linear index y * W + x of the pixel's 8-connected component of equal
 *   key, -1 for key 255.  workspace: dpp_label_workspace_bytes(B, H, W) bytes.  stats (may be NULL): dpp_component_stats_bytes(B, H,
 *   W) bytes, one 40-byte record per pixel, meaningful at roots (labels[p] == p): int32 count, ~xmin, xmax, ~ymin, ymax, pad;
 *   uint64 sum x, sum y.  Three launches, four with stats.
 * detect_seed: state (dpp_detect_state_bytes(B) bytes; slab_keys / mask_keys clear their word of it).  Among the components of
 *   more than 200 px the smallest key, then the smallest root; com_out [B][3] = calculateCoM of the +-100 px window around its
 *   centroid inside that slab (handdetector.py:589-607), status [B] = DPP_DETECT_FOUND; no such component: com (0, 0, 0), status 0.
 *   Two launches.  The caller feeds com_out to dpp_refine_com_iterative (num_iter 5, :610).
 * hand_size: after mask_keys + label_components with stats: the largest component (ties: smallest root), estimateHandsize from
 *   its bounding box and com [B][3] -> cube_out [B][3] = (sz + tol) x 3.  status [B] is read and updated: a frame without
 *   DPP_DETECT_FOUND keeps cube_in; an empty mask keeps cube_in and sets DPP_DETECT_NO_SIZE.  Two launches.
 * Limits: H * W < 2^31 - 256, H <= 65535 * 32, B <= 65535 (DPP_E_BADARG beyond; the *_bytes functions then return 0). */
#define DPP_DETECT_FOUND 1
#define DPP_DETECT_NO_SIZE 2
size_t dpp_label_workspace_bytes(int B, int H, int W);
size_t dpp_component_stats_bytes(int B, int H, int W);
size_t dpp_detect_state_bytes(int B);
int dpp_slab_keys(const float* frames, const float* partial, int B, int H, int W, unsigned char* keys, void* state, dpp_stream_t stream);
int dpp_mask_keys(const float* frames, int B, int H, int W, const float* com, const float* cube, unsigned char* keys, void* state,
                  dpp_stream_t stream);
int dpp_label_components(const unsigned char* keys, int B, int H, int W, void* workspace, int* labels, void* stats, dpp_stream_t stream);
int dpp_detect_seed(const float* frames, const float* partial, const unsigned char* keys, const int* labels, const void* stats, int B, int H,
                    int W, void* state, float* com_out, int* status, dpp_stream_t stream);
int dpp_hand_size(const unsigned char* keys, const int* labels, const void* stats, int B, int H, int W, void* state, const float* com,
                  const float* cube_in, double fx, double fy, double tol, float* cube_out, int* status, dpp_stream_t stream);

/* ---- several hands of one frame (ABI v17) ------------------------------------------------------------------------------------------
 * detect_seeds: up to K seeds per frame from the labelling of slab_keys + label_components (with stats), in detect_seed's place.
 *   Candidates: the components of more than 200 px, ordered by (key, root): nearest slab first, then raster-first.  With
 *   max_extent > 0 (mm; 0: off) a candidate is dropped when (xmax - xmin + 1) * b_{key+1} / |fx| > max_extent or the same in y with
 *   |fy| (float64, in that order): a far wall is no hand.  A dropped candidate suppresses nothing.
 *   Selection: the candidates are walked in order; one whose centroid (rint of sum / count, float64) lies inside the seed window
 *   [xs, xe) x [ys, ye) of an ACCEPTED candidate is suppressed (one hand across a slab boundary is two components), any other is
 *   accepted, until K are.  Suppressed candidates suppress nothing.
 *   Row b * K + k of seed_out [B * K][3] / status [B * K] is detect_seed's result for the k-th accepted component of frame b;
 *   report [B * K][6] int32 = its key, pixel count, xmin, xmax, ymin, ymax.  A slot without a component: seed (0, 0, 0), status
 *   0, report all zero.  K = 1 with max_extent 0 gives detect_seed's bytes.
 *   state: as for detect_seed; word 0 of a frame (which slab_keys cleared) counts the frame's candidates.  candidates:
 *   dpp_detect_candidates_bytes(B, H, W) bytes, (2 * (H * W / 201) + 16) 64-bit words per frame: the list cannot overflow, since
 *   components of more than 200 px are disjoint.  Three launches.  DPP_E_BADARG (nothing launched): a NULL pointer, the
 *   labelling's limits, K outside [1, 16], max_extent negative or not finite, max_extent > 0 with fx or fy 0.
 * refine_com_iterative_ix: R rows; row r refines com_in[r] in frame src[r] with that frame's partials and cube [C][3] (the rows of
 *   a frame share its cube); the caller guarantees 0 <= src[r] < C.  src NULL: row r reads frame r, the plain entry point. */
#define DPP_DETECT_MAX_HANDS 16
size_t dpp_detect_candidates_bytes(int B, int H, int W);
int dpp_detect_seeds(const float* frames, const float* partial, const unsigned char* keys, const int* labels, const void* stats, int B, int H,
                     int W, void* state, void* candidates, int K, double max_extent, double fx, double fy, float* seed_out, int* status,
                     int* report, dpp_stream_t stream);
int dpp_refine_com_iterative_ix(const float* frames, const float* partial, int R, const int* src, int H, int W, const float* com_in,
                                const float* cube, double fx, double fy, int num_iter, float* com_out, int* status, dpp_stream_t stream);

/* ---- PCA prior set-up and evaluation on the device --------------------------------------------
 * pose_sample: HandDetector.sampleRandomPoses (/root/reference/src/util/handdetector.py:805-909) for n samples: sample i augments
 *   base pose ridx[i] in label space with mode[i] (0 none, 1 com, 2 rot, 3 sc, 4 rot+com, 5 rot+com+sc) and the draws off[i][3],
 *   sc[i], rot[i] (degrees) -- the host draws them from the script's RandomState in the reference's order, the arithmetic (f64
 *   projections, f32 storage) runs here.  out_poses [n][J][3] normalised by the (new) cube_z / 2; out_com / out_cube may be NULL.
 * pca_fit: sklearn PCA.fit on X [N][D] f32 (main_nyu_posereg_embedding.py:86-92): mean[D], the eigenvalues of the covariance
 *   (1 / (N - 1)) in descending order and the eigenvectors as ROWS (components_, largest-magnitude entry of each row positive),
 *   all f64; D <= 80 (26 joints: the scatter tile and the Jacobi matrices are LDS-resident; DPP_E_BADARG beyond).  The Jacobi sweeps
 *   run until the off-diagonal mass is at f64 rounding level of the diagonal's (at most 30).  workspace: dpp_pca_workspace_bytes(N, D) bytes of device memory.
 * pose_eval: HandposeEvaluation's numeric methods (/root/reference/src/util/handpose_evaluation.py:92-228) on gt / pred [N][J][3]:
 *   err [N][J] Euclidean errors, frame [N][4] = per-frame (nanmean, nanmax, count, nanstd) over joints, and out (4 + 3J + 2T
 *   doubles): mean error, max error, mean of the frame stds, frames counted; per-joint nanmean / nanstd / nanmax; for each of the T
 *   thresholds the frames whose max (then: mean) error is <= it. */
int dpp_pose_sample(const float* base_poses, const float* base_com, const float* base_cube, int n_base, int J, const int* mode,
                    const int* ridx, const double* off, const double* sc, const double* rot, long n, double fx, double fy,
                    double ux, double uy, int flip_y, float* out_poses, float* out_com, float* out_cube, dpp_stream_t stream);
/* (ABI v11) the same with rot3D=True (handdetector.py:870, 891, 903): the rotation modes turn the pose in 3-D about the (new) centre --
 * rotatePoints3D, /root/reference/src/data/transformations.py:105-155 -- by the sample's matrix rot3[i] (3x3 row-major f64: getRotationMatrix of
 * the three drawn angles, formed on the host like the draws themselves) instead of in the image plane. */
int dpp_pose_sample_rot3d(const float* base_poses, const float* base_com, const float* base_cube, int n_base, int J, const int* mode,
                          const int* ridx, const double* off, const double* sc, const double* rot3, long n, double fx, double fy,
                          double ux, double uy, int flip_y, float* out_poses, float* out_com, float* out_cube, dpp_stream_t stream);
size_t dpp_pca_workspace_bytes(long N, int D);
int dpp_pca_fit(const float* X, long N, int D, void* workspace, double* mean, double* evals, double* components, dpp_stream_t stream);
int dpp_pose_eval(const float* gt, const float* pred, int N, int J, const double* thresholds, int T, double* err, double* frame,
                  double* out, dpp_stream_t stream);

/* ---- a whole bottleneck block of the deterministic forward pass as ONE launch (ABI v10) ----------------------------------------
 * res_block of /root/reference/src/net/resnet.py:349-414 with every BatchNormLayer in deterministic mode
 * (/root/reference/src/net/batchnormlayer.py:158-159: stored running mean / inv_std), as netbase.py:257-310 (computeOutput) runs it:
 *     h = relu(bn0(x));  c1 = conv1x1_s(h) + b1;  c2 = conv3x3(relu(bn1(c1))) + b2;  c3 = conv1x1(relu(bn2(c2))) + b3
 *     Y = x + c3  (identity block: Wsc == NULL, Cin == Cout, stride 1)     Y = c3 + conv1x1_s(h) + bsc  (projection block)
 * bn(v) = (v - mean) * (gamma * inv_std) + beta.  X [N][H][W][Cin], Y [N][Ho][Wo][Cout] (Ho = ceil(H / stride)), weights in kernel
 * layout: W1 [Nb][Cin], W2 [Nb][9][Nb], W3 [Cout][Nb], Wsc [Cout][Cin].  float32 tensors, f32 MFMA.  The 16- / 32- / 64-channel
 * intermediates stay in LDS (csrc/resblock.hip).  dpp_resblock_eval_ok: 1 when the kernel takes the shape, else the caller issues the
 * block layer by layer (dpp_gemm / dpp_conv3x3 with dpp_act prologues). */
typedef struct {
    const float* mean;
    const float* inv_std;
    const float* gamma;
    const float* beta;
} dpp_bn_eval;
typedef struct {
    const float* X; int N, H, W, Cin;
    int stride, Ho, Wo, Cout, Nb;
    dpp_bn_eval bn0, bn1, bn2;
    const float* W1; const float* b1;
    const float* W2; const float* b2;
    const float* W3; const float* b3;
    const float* Wsc; const float* bsc;
    float* Y;
    int store;      /* (ABI v11) DPP_ST_A: X holds bf16 elements, DPP_ST_C: Y does.  DPP_ST_C selects the bf16 MODE of the block (BASELINE config 5):
                     * what the layer-by-layer bf16 path stores is rounded to bfloat16 where it would have been stored, what it multiplies on bf16
                     * MFMA operands is rounded as its kernels round it.  DPP_ST_A alone is refused. */
} dpp_resblock_desc;
int dpp_resblock_eval_ok(int Cin, int Cout, int Nb, int stride, int projection);
int dpp_resblock_eval(const dpp_resblock_desc* d, dpp_stream_t stream);
/* (ABI v11) the status dpp_resblock_eval would return for this descriptor, without launching (alignment, LDS size, offsets, storage) */
int dpp_resblock_eval_check(const dpp_resblock_desc* d);

/* ---- launch plans: a whole train / inference step as ONE call --------------------------------------------------------
 * The reference runs `train_model(index, lr)` as one compiled device function (theano.function,
 * /root/reference/src/trainer/poseregnettrainer.py:146-170, called at /root/reference/src/trainer/nettrainer.py:840).
 * A plan is the equivalent here: the ordered kernel launches of a step, recorded once and re-issued from C++ without any
 * host-language work per launch.  While a plan is recording on the calling thread (dpp_plan_record_begin ..
 * dpp_plan_record_end) every dpp_* launch call of that thread appends its fully resolved launch (kernel, grid, arguments)
 * to the plan instead of launching, its `stream` argument being ignored.  A plan has two lanes: lane 0 (main) and lane 1 (side,
 * the parameter-gradient branch).  dpp_plan_fork makes the side lane wait for everything recorded so far on the main lane,
 * dpp_plan_join makes the main lane wait for everything recorded so far on the side lane.
 *   dpp_plan_run          issues the launches on two HIP streams (events for fork / join); side == NULL or == main: one stream
 *   dpp_plan_graph_build  builds an explicit hipGraph (hipGraphAddKernelNode + dependency edges: lanes stay parallel
 *                         branches); two_lanes == 0 chains everything in recorded order
 *   dpp_plan_graph_launch replays it on `stream`
 * Device pointers recorded in a plan must stay valid for its lifetime (the caller owns them, as everywhere in this ABI). */
/* Profiling build only (make -C csrc prof): kernels compiled with phase stamps write 16 x uint64 of 100 MHz ticks per workgroup
 * to `buf` (tools/phase_profile.py); in the product build the stamps are compiled out and this only stores the pointer. */
int dpp_prof_set(void* buf);
typedef struct dpp_plan dpp_plan;
int dpp_plan_create(dpp_plan** out);
int dpp_plan_destroy(dpp_plan* plan);
int dpp_plan_record_begin(dpp_plan* plan);
int dpp_plan_record_lane(dpp_plan* plan, int lane);
int dpp_plan_record_end(dpp_plan* plan);
int dpp_plan_fork(dpp_plan* plan);
int dpp_plan_join(dpp_plan* plan);
int dpp_plan_count(const dpp_plan* plan, int* launches, int* forks, int* joins);
int dpp_plan_run(dpp_plan* plan, dpp_stream_t main_stream, dpp_stream_t side_stream);
int dpp_plan_graph_build(dpp_plan* plan, int two_lanes);
int dpp_plan_graph_launch(dpp_plan* plan, dpp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DPP_HIP_H */
