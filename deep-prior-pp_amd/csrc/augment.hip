// augment.hip -- the online depth-crop augmentation (rotate / scale / translate CoM) fused for gfx950.
//
// Replaces the per-sample Python + cv2 loop that the reference runs in 8 worker processes:
//   NetTrainer.augmentCrop                 /root/reference/src/trainer/nettrainer.py:919-997
//   HandDetector.moveCoM / rotateHand / scaleHand / recropHand / comToBounds / comToTransform
//                                          /root/reference/src/util/handdetector.py:204-258, 678-803
//   importer (un)projection                /root/reference/src/data/importers.py:80-119, 1187-1224
//   rotatePoint2D                          /root/reference/src/data/transformations.py:71-88
//   proj.transform(label) (PCA prior)      /root/reference/src/trainer/poseregnettrainer.py:262
// cv2.warpAffine / warpPerspective (INTER_NEAREST, BORDER_CONSTANT 0) are restated from OpenCV 2.4's
// imgwarp.cpp exactly as oracle/augment.py documents (10-bit fixed point for the affine warp, cvRound of the
// double coordinate on 64-wide blocks for the perspective warp).
//
// One launch per batch (augment_fused_kernel, dpp_augment); the two stages also exist as separate launches
// (dpp_augment_prepare + dpp_augment_warp, used by the parity tests to look at the per-sample records):
//   augment_prepare_kernel  one workgroup per crop: wave-shuffle max of the crop (the reference's `premax`),
//                           then lane 0 does the per-sample geometry in f64 (new CoM, crop transform, inverse
//                           warp matrix, z-thresholds, joint labels) and the workgroup projects the label onto
//                           the PCA prior;
//   augment_warp_kernel     one thread per output pixel: de-normalise, gather through the inverse map, z-clamp,
//                           far-plane fill, re-normalise.  HBM traffic = read 64 KB + write 64 KB per crop; the
//                           gather hits L2 (a 64 KB crop is resident).
// The initial crop of full depth frames, the HandDetector crop helpers and the realtime tracking kernels live in crop.hip; the camera,
// bounds and warp-coordinate arithmetic both units (and prior.hip) use is geom.h.
// Compiled with -ffp-contract=off: the reference's NumPy/OpenCV arithmetic rounds after every operation, so no
// fused multiply-add may be formed here (pixel coordinates at rounding boundaries would move).
#include <stdlib.h>
#include "geom.h"

namespace {

constexpr int AUG_NONE = 0, AUG_COM = 1, AUG_ROT = 2, AUG_SC = 3;
constexpr int WARP_NONE = 0, WARP_AFFINE = 1, WARP_PERSP = 2;

struct AugRec {                // per-sample record written by prepare, read by warp
    double m[9];               // inverse map (affine uses m[0..5])
    int warp;
    int thresh;                // apply the 32000 / z-threshold rules of recropHand
    float zlo, zhi;            // zstart / zend
    float den_scale, den_off;  // img * (cz/2) + com_z  (old cube / old com)
    float premax;
    float far_v, near_v;       // com_z' +- cz'/2
    float norm_off, norm_div;  // (v - com_z') / (cz'/2)
    int binarize;              // then < 0.5 -> 0, >= 0.5 -> 1 (augment_poses' binarizeImage, poseregnettrainer.py:255-257)
};

// comToTransform: off . scale . trans  (3x3, row-major)
__device__ void com_to_transform(const float com[3], const double size[3], double fx, double fy, int dsz, double T[9]) {
    int b[4];
    const double comd[3] = {com[0], com[1], com[2]};
    com_to_bounds(comd, size, fx, fy, b);
    int wb = b[1] - b[0], hb = b[3] - b[2];
    double s;
    long long sz0, sz1;
    if (wb > hb) { s = (double)dsz / (double)wb; sz0 = dsz; sz1 = floordiv((long long)hb * dsz, wb); }
    else { s = (double)dsz / (double)hb; sz0 = floordiv((long long)wb * dsz, hb); sz1 = dsz; }
    double xs = floor(dsz / 2. - sz1 / 2.);
    double ys = floor(dsz / 2. - sz0 / 2.);
    // off * (scale * trans): scale*trans = [[s,0,-s*xstart],[0,s,-s*ystart],[0,0,1]]
    T[0] = s; T[1] = 0.; T[2] = s * (double)(-b[0]) + xs;
    T[3] = 0.; T[4] = s; T[5] = s * (double)(-b[2]) + ys;
    T[6] = 0.; T[7] = 0.; T[8] = 1.;
}

// ---- correctly rounded sin / cos --------------------------------------------------------------------------------------------
// cv2.getRotationMatrix2D and rotatePoint2D call libm, which on the reference's platform (glibc 2.19, IBM Accurate Mathematical
// Library) returns the CORRECTLY ROUNDED cosine / sine of the float64 angle; ocml's cos / sin (and today's NumPy) are only
// "< 1 ulp".  Rotation coefficients that differ in the last bit are a different affine map, and nearest-neighbour gathering is
// index work, so the coefficients are computed here in plain IEEE arithmetic that oracle/augment.py:sincos_cr repeats operation
// for operation: Cody-Waite reduction by pi/2 in three 33-bit parts (k * part is exact), Taylor series of sin and cos in
// double-double (two_prod through one fma: the exact error term, the pair Dekker's splitting gives the oracle), result = the
// high word.  ~106 bits, so a rounding can only be missed when the true value lies within 2^-100 of a midpoint of two doubles.
struct dd2 { double hi, lo; };
__device__ __forceinline__ dd2 dd_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return dd2{s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd2 dd_fast_two_sum(double a, double b) {
    const double s = a + b;
    return dd2{s, b - (s - a)};
}
__device__ __forceinline__ dd2 dd_mul(dd2 x, dd2 y) {
    const double p = x.hi * y.hi;
    double e = __builtin_fma(x.hi, y.hi, -p);
    e = e + (x.hi * y.lo + x.lo * y.hi);
    return dd_fast_two_sum(p, e);
}
__device__ __forceinline__ dd2 dd_add(dd2 x, dd2 y) {
    dd2 s = dd_two_sum(x.hi, y.hi);
    return dd_fast_two_sum(s.hi, s.lo + (x.lo + y.lo));
}
__device__ void dpp_sincos_cr(double a, double* sn, double* cs) {      // |a| < 8
    static const double SC[12][2] = {
        {-0x1.5555555555555p-3, -0x1.5555555555555p-57}, {0x1.1111111111111p-7, 0x1.1111111111111p-63},
        {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73}, {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},
        {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80}, {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},
        {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97}, {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103},
        {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112}, {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120},
        {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130}, {0x1.3f3ccdd165fa9p-84, -0x1.58ddadf344487p-139}};
    static const double CC[13][2] = {
        {-0x1.0000000000000p-1, 0x0.0p+0}, {0x1.5555555555555p-5, 0x1.5555555555555p-59},
        {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65}, {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},
        {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76}, {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},
        {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92}, {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101},
        {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107}, {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120},
        {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124}, {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135},
        {-0x1.88e85fc6a4e5ap-89, 0x1.71c37ebd16540p-143}};
    const double P1 = 0x1.921fb54400000p+0, P2 = 0x1.0b4611a600000p-34, P3 = 0x1.3198a2e000000p-69, P3T = 0x1.b839a252049c1p-104;
    const double k = rint(a * 0x1.45f306dc9c883p-1);
    dd2 r = dd_two_sum(a - k * P1, -(k * P2));
    r = dd_add(r, dd2{-(k * P3), -(k * P3T)});
    const dd2 z = dd_mul(r, r);
    dd2 ps = dd2{SC[11][0], SC[11][1]};
    for (int i = 10; i >= 0; --i) ps = dd_add(dd_mul(ps, z), dd2{SC[i][0], SC[i][1]});
    const dd2 s = dd_add(dd_mul(dd_mul(ps, z), r), r);
    dd2 pc = dd2{CC[12][0], CC[12][1]};
    for (int i = 11; i >= 0; --i) pc = dd_add(dd_mul(pc, z), dd2{CC[i][0], CC[i][1]});
    const dd2 c = dd_add(dd_mul(pc, z), dd2{1.0, 0.0});
    const int q = (int)k & 3;
    *sn = q == 0 ? s.hi : (q == 1 ? c.hi : (q == 2 ? -s.hi : -c.hi));
    *cs = q == 0 ? c.hi : (q == 1 ? -s.hi : (q == 2 ? -c.hi : s.hi));
}

// ---- counter-based RNG for on-device parameter draws (Philox-4x32-10) -----------------------------------
__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
__device__ void philox4(unsigned long long seed, unsigned long long ctr, unsigned sub, unsigned out[4]) {
    unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = sub, c3 = 0;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01f(unsigned a) {                   // (0,1), 24 bits
    return ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ double u01(unsigned a, unsigned b) {       // (0,1), 53 bits
    unsigned long long v = (((unsigned long long)a << 32) | b) >> 11;
    return ((double)v + 0.5) * (1.0 / 9007199254740992.0);
}

struct PrepArgs {
    const float* img;        // [B][H*W] normalised crops
    const float* com3d;      // [B][3]
    const float* cube;       // [B][3]
    const float* Mcrop;      // [B][9]
    const float* gt3d;       // [B][J][3] joints relative to the CoM (mm)
    const int* mode;         // [B] or null -> drawn on device
    const double* off;       // [B][3]
    const double* rot;       // [B]
    const double* sc;        // [B]
    const int* mode_table;   // [n_modes] aug_modes as AUG_* codes (device draws index into it)
    int n_modes;
    unsigned long long seed, counter;
    const unsigned long long* counter_dev;
    unsigned long long sample0, gbatch;   // draws are keyed by (seed, step, sample0 + b) with step * gbatch + ... as the counter
    double sigma_com, sigma_sc, rot_range;
    AugCam cam;
    int B, J, dsz;
    int norm01;              // crops normalised to [0, 1] (normZeroOne) instead of [-1, 1]
    int binarize;            // binarizeImage: the augmented crop is thresholded at 0.5 (bit 1 of the ABI's norm_zero_one argument)
    const float* pca_mean;   // [J*3] or null
    const float* pca_comp;   // [E][J*3]
    int E;
    AugRec* rec;             // [B]
    float* out_y;            // [B][E] or [B][J*3]
    int* out_mode;           // [B] (optional: the mode actually used)
    unsigned long long* prof; // phase stamps (profiling build only, see dpp_stamp)
};

// What the per-joint label transforms need from the per-sample geometry (written by thread 0, read by the joint threads).
struct AugLabelCtx {
    int mode, zero;            // augmentation mode actually applied; the reference's early-out (zero offset / angle)
    float c3[3], n3[3];        // old / new CoM in 3-D
    float com[3];              // old CoM in image coordinates
    double ca, sa;             // cos / sin of the label rotation
    float half_old, half_new;  // cube_z / 2 before / after scaling
};

// The per-sample geometry of augmentCrop, run by ONE thread: the four draws, the new CoM / cube, the inverse warp matrix and
// z-thresholds (-> r) and what the label transforms need (-> lc).  `mx` is the maximum of the stored crop.
__device__ void aug_prepare_geometry(const PrepArgs& a, int b, float mx, AugRec& r, AugLabelCtx& lc) {
    const AugCam cam = a.cam;
    const double fx = fabs(cam.fx), fy = fabs(cam.fy);      // HandDetector(..., abs(di.fx), abs(di.fy))
    // every global value this lane needs, requested BEFORE anything is computed: the draws, the mode table lookup and the geometry
    // used to reach them one after the other -- five dependent memory round trips on a lane that does nothing else (tools/
    // augment_phase.py: 9 us of geometry even in 'none' mode)
    const float g_cube[3] = {a.cube[b * 3], a.cube[b * 3 + 1], a.cube[b * 3 + 2]};
    const float g_com[3] = {a.com3d[b * 3], a.com3d[b * 3 + 1], a.com3d[b * 3 + 2]};
    float g_M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) g_M[i] = a.Mcrop[b * 9 + i];
    int g_tab[4] = {0, 0, 0, 0};
    if (!a.mode) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g_tab[i] = a.mode_table[i < a.n_modes ? i : 0];
    }
    const unsigned long long g_ctr = (!a.mode && a.counter_dev) ? *a.counter_dev : 0ull;
    DPP_SCHED_FENCE();
    // ---- the four draws of augmentCrop (nettrainer.py:954-957) ----
    int mode; double off[3], rot, sc;
    if (a.mode) {
        mode = a.mode[b]; off[0] = a.off[b * 3]; off[1] = a.off[b * 3 + 1]; off[2] = a.off[b * 3 + 2]; rot = a.rot[b]; sc = a.sc[b];
    } else {
        unsigned r0[4], r1[4], r2[4];
        unsigned long long ctr = (a.counter + g_ctr) * a.gbatch + a.sample0 + b;
        philox4(a.seed, ctr, 0, r0); philox4(a.seed, ctr, 1, r1); philox4(a.seed, ctr, 2, r2);
        const unsigned mi = r0[0] % (unsigned)a.n_modes;
        mode = mi < 4u ? (mi == 0 ? g_tab[0] : (mi == 1 ? g_tab[1] : (mi == 2 ? g_tab[2] : g_tab[3]))) : a.mode_table[mi];
        // Box-Muller in float32 (hardware log / sin / cos rates): the draws are this kernel's own random numbers -- nothing pins
        // their low bits (the reference draws from NumPy's Mersenne twister) -- and in float64 the six ocml transcendentals were
        // ~8 us of the ~25 us this lane spends before the first pixel moves.  Everything DOWNSTREAM of the draws stays float64.
        const float v1 = u01f(r0[1]), v2 = u01f(r0[3]), v3 = u01f(r1[1]), v4 = u01f(r1[3]);
        const float ra = sqrtf(-2.0f * logf(v1)), rb = sqrtf(-2.0f * logf(v3));
        float s2, c2, s4, c4;
        sincosf(6.2831853f * v2, &s2, &c2);
        sincosf(6.2831853f * v4, &s4, &c4);
        off[0] = (double)(ra * c2) * a.sigma_com;
        off[1] = (double)(ra * s2) * a.sigma_com;
        off[2] = (double)(rb * c4) * a.sigma_com;
        rot = (2.0 * u01(r2[1], r2[2]) - 1.0) * a.rot_range;
        sc = fabs(1.0 + (double)(rb * s4) * a.sigma_sc);
    }
    if (a.out_mode) a.out_mode[b] = mode;

    double cube[3] = {(double)g_cube[0], (double)g_cube[1], (double)g_cube[2]};
    float com[3];           // CoM in image coordinates (float32 array in the reference)
    toimg(cam, g_com[0], g_com[1], g_com[2], true, com);
    double Mold[9];
    for (int i = 0; i < 9; ++i) Mold[i] = (double)g_M[i];

    r.warp = WARP_NONE; r.thresh = 0; r.zlo = 0.f; r.zhi = 0.f;
    for (int i = 0; i < 9; ++i) r.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
    // de-normalisation of the stored crop (nettrainer.py:948-951): [-1, 1] about the CoM, or [0, 1] from the cube's front face
    r.den_scale = a.norm01 ? (float)cube[2] : (float)(cube[2] / 2.);
    r.den_off = a.norm01 ? (float)((double)com[2] - cube[2] / 2.) : com[2];
    r.premax = mx * r.den_scale + r.den_off;      // two roundings (contraction is off)
    float ncom[3] = {com[0], com[1], com[2]};
    double ncube[3] = {cube[0], cube[1], cube[2]};
    lc.mode = mode; lc.zero = 0; lc.ca = 1.0; lc.sa = 0.0;
    lc.com[0] = com[0]; lc.com[1] = com[1]; lc.com[2] = com[2];
    lc.half_old = (float)(cube[2] / 2.);
    to3d(cam, com[0], com[1], com[2], lc.c3);
    lc.n3[0] = lc.c3[0]; lc.n3[1] = lc.c3[1]; lc.n3[2] = lc.c3[2];

    if (mode == AUG_COM) {
        const bool zero = fabs(off[0]) <= 1e-8 && fabs(off[1]) <= 1e-8 && fabs(off[2]) <= 1e-8;
        lc.zero = zero;
        if (!zero) {
            toimg(cam, (double)lc.c3[0] + off[0], (double)lc.c3[1] + off[1], (double)lc.c3[2] + off[2], false, ncom);
            if (!(fabs((double)com[2]) <= 1e-8 || fabs((double)ncom[2]) <= 1e-8)) {
                double Mn[9], Mi[9], Mt[9];
                com_to_transform(ncom, cube, fx, fy, a.dsz, Mn);
                mat3_inv(Mold, Mi);                 // numpy.linalg.inv(M) restated as cofactor inverse (f64)
                mat3_mul(Mn, Mi, Mt);
                mat3_inv(Mt, r.m);                  // warpPerspective inverts the forward matrix
                r.warp = WARP_PERSP; r.thresh = 1;
                r.zlo = (float)((double)ncom[2] - cube[2] / 2.);
                r.zhi = (float)((double)ncom[2] + cube[2] / 2.);
            }
        }
        to3d(cam, ncom[0], ncom[1], ncom[2], lc.n3);
    } else if (mode == AUG_ROT) {
        const bool zero = fabs(rot) <= 1e-8;
        lc.zero = zero;
        if (!zero) {
            rot = rot - floor(rot / 360.0) * 360.0;                 // numpy.mod(rot, 360)
            // cv2.getRotationMatrix2D((W//2, H//2), -rot, 1) then the inversion at the top of cv::warpAffine
            // the warp angle -rot*pi/180 is exactly the negative of the label angle rot*pi/180 (negation is exact and commutes with
            // the two roundings), and the correctly rounded sine / cosine are odd / even: ONE evaluation serves both
            double sl, cl;
            dpp_sincos_cr(rot * 3.141592653589793 / 180., &sl, &cl);
            lc.sa = sl; lc.ca = cl;
            const double al = cl, be = -sl;
            double cx = (double)(a.dsz / 2), cy = (double)(a.dsz / 2);
            double F[6] = {al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy};
            double D = F[0] * F[4] - F[1] * F[3];
            D = D != 0 ? 1. / D : 0.;
            double A11 = F[4] * D, A22 = F[0] * D;
            r.m[0] = A11; r.m[1] = F[1] * (-D); r.m[3] = F[3] * (-D); r.m[4] = A22;
            r.m[2] = -r.m[0] * F[2] - r.m[1] * F[5];
            r.m[5] = -r.m[3] * F[2] - r.m[4] * F[5];
            r.warp = WARP_AFFINE;
        }
        if (zero) {
            const double alpha = rot * 3.141592653589793 / 180.;
            dpp_sincos_cr(alpha, &lc.sa, &lc.ca);
        }
    } else if (mode == AUG_SC) {
        const bool one = fabs(sc - 1.0) <= (1e-8 + 1e-5);                  // numpy.allclose(sc, 1.)
        if (!one) {
            for (int d = 0; d < 3; ++d) ncube[d] = cube[d] * sc;
            if (!(fabs((double)com[2]) <= 1e-8)) {
                double Mn[9], Mi[9], Mt[9];
                com_to_transform(com, ncube, fx, fy, a.dsz, Mn);
                mat3_inv(Mold, Mi);
                mat3_mul(Mn, Mi, Mt);
                mat3_inv(Mt, r.m);
                r.warp = WARP_PERSP; r.thresh = 1;
                r.zlo = (float)((double)com[2] - cube[2] / 2.);      // thresholds use the OLD cube
                r.zhi = (float)((double)com[2] + cube[2] / 2.);
            }
        }
    }
    lc.half_new = (float)(ncube[2] / 2.);
    double far_d = (double)ncom[2] + ncube[2] / 2., near_d = (double)ncom[2] - ncube[2] / 2.;
    r.far_v = (float)far_d; r.near_v = (float)near_d;
    r.norm_off = a.norm01 ? r.near_v : ncom[2];              // nettrainer.py:982-995
    r.norm_div = a.norm01 ? (float)ncube[2] : (float)(ncube[2] / 2.);
    r.binarize = a.binarize;
}

// The label of ONE joint j under the augmentation described by lc (the per-joint bodies of moveCoM / rotateHand / scaleHand's
// label handling, nettrainer.py:958-981): one thread per joint.
__device__ __forceinline__ void aug_label_joint(const PrepArgs& a, int b, const AugLabelCtx& lc, int j, float* s_label) {
    const AugCam cam = a.cam;
    float g[3];
    for (int d = 0; d < 3; ++d) g[d] = a.gt3d[((size_t)b * a.J + j) * 3 + d];
    if (lc.mode == AUG_COM) {
        for (int d = 0; d < 3; ++d) {
            const float nj = lc.zero ? g[d] : ((g[d] + lc.c3[d]) - lc.n3[d]);
            s_label[j * 3 + d] = nj / lc.half_old;
        }
    } else if (lc.mode == AUG_ROT) {
        if (lc.zero) { for (int d = 0; d < 3; ++d) s_label[j * 3 + d] = g[d] / lc.half_old; return; }
        float p3[3], p2[3], pr[3], q3[3];
        for (int d = 0; d < 3; ++d) p3[d] = g[d] + lc.c3[d];
        toimg(cam, p3[0], p3[1], p3[2], true, p2);
        const float px = p2[0] - lc.com[0], py = p2[1] - lc.com[1];          // rotatePoint2D on float32 arrays
        pr[0] = (float)((double)px * lc.ca - (double)py * lc.sa);
        pr[1] = (float)((double)px * lc.sa + (double)py * lc.ca);
        pr[0] = pr[0] + lc.com[0]; pr[1] = pr[1] + lc.com[1]; pr[2] = p2[2];
        to3d(cam, pr[0], pr[1], pr[2], q3);
        for (int d = 0; d < 3; ++d) s_label[j * 3 + d] = (q3[d] - lc.c3[d]) / lc.half_old;
    } else if (lc.mode == AUG_SC) {
        for (int d = 0; d < 3; ++d) s_label[j * 3 + d] = g[d] / lc.half_new;
    } else {
        for (int d = 0; d < 3; ++d) s_label[j * 3 + d] = g[d] / lc.half_old;
    }
}

// label -> PCA prior (poseregnettrainer.py:262) or the raw normalised joints, by threads t = 0 .. nt-1 (nt a multiple of 8: the whole
// workgroup, or one wave)
// (part / nparts: this caller's share of the outputs -- the rounds r = e0 / (nt / 8) with r % nparts == part; the fused launch deals
//  them to the `splits` workgroups of a crop)
__device__ __forceinline__ void aug_project_label(const PrepArgs& a, int b, const float* s_label, int t, int nt, int part = 0, int nparts = 1) {
    const int D = a.J * 3;
    if (a.pca_comp) {
        // 8 lanes per output: lane p sums d = p, p + 8, ..., the eight partial sums meet in an xor butterfly (a fixed order).  One
        // thread per output walked D dependent multiply-adds with two global loads each: 11 us for 30 x 48.
        const int p = t & 7;
        for (int e0 = part * (nt / 8); e0 < a.E; e0 += nparts * (nt / 8)) {
            const int e = e0 + (t >> 3);
            double sum = 0.0;
            if (e < a.E) {
                const float* comp = a.pca_comp + (size_t)e * D;
                for (int d0 = p; d0 < D; d0 += 48) {               // six terms per round, their loads issued together
                    float c[6], m[6];
#pragma unroll
                    for (int u = 0; u < 6; ++u) {
                        const int d = d0 + 8 * u;
                        c[u] = d < D ? comp[d] : 0.0f;
                        m[u] = d < D ? a.pca_mean[d] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 6; ++u) {
                        const int d = d0 + 8 * u;
                        if (d < D) sum += ((double)s_label[d] - (double)m[u]) * (double)c[u];
                    }
                }
            }
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 4);
            if (e < a.E && p == 0) a.out_y[(size_t)b * a.E + e] = (float)sum;
        }
    } else if (part == 0) {
        for (int d = t; d < D; d += nt) a.out_y[(size_t)b * D + d] = s_label[d];
    }
}

// maximum of a stored crop over the workgroup (the reference's `premax`): monotone under the f32 de-normalisation, so max
// first, de-normalise after.  Every thread returns the maximum.
__device__ __forceinline__ float aug_crop_max(const float* __restrict__ im, int npix, float* s_red) {
    const int tid = threadIdx.x;
    float mx = -3.4e38f;
    int i0 = 0;
    if ((npix & 3) == 0 && (reinterpret_cast<uintptr_t>(im) & 15) == 0) {
        const float4* im4 = reinterpret_cast<const float4*>(im);
        for (int i = tid; i < (npix >> 2); i += DPP_THREADS) {
            const float4 v = im4[i];
            mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
        i0 = npix;
    }
    for (int i = i0 + tid; i < npix; i += DPP_THREADS) mx = fmaxf(mx, im[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = s_red[0];
    for (int w = 1; w < DPP_THREADS / DPP_WAVE; ++w) mx = fmaxf(mx, s_red[w]);
    return mx;
}

__global__ __launch_bounds__(DPP_THREADS) void augment_prepare_kernel(PrepArgs a) {
    dpp_kernarg_warm<sizeof(PrepArgs)>();
    __shared__ float s_red[DPP_THREADS / DPP_WAVE];
    __shared__ float s_label[MAXJ3];
    const int b = blockIdx.x;
    const float mx = aug_crop_max(a.img + (size_t)b * a.dsz * a.dsz, a.dsz * a.dsz, s_red);
    __shared__ AugLabelCtx s_lc;
    if (threadIdx.x == 0) {
        AugRec r;
        aug_prepare_geometry(a, b, mx, r, s_lc);
        a.rec[b] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.J) aug_label_joint(a, b, s_lc, threadIdx.x, s_label);
    __syncthreads();
    aug_project_label(a, b, s_label, threadIdx.x, DPP_THREADS);
}

// The value rules of augmentCrop on one de-normalised pixel v (0: outside the source crop, BORDER_CONSTANT 0): recropHand's rules if
// the pixel went through a thresholded warp, then premax / zero -> far plane, the far / near clamp, re-normalisation, binarisation.
__device__ __forceinline__ float aug_pixel_value(const AugRec& r, float v, bool warped) {
    if (warped && r.thresh) {
        if (is_close(v, 32000.0)) v = 0.0f;                      // numpy.isclose(warped, nv_val)
        v = z_threshold(v, r.zlo, r.zhi);
    }
    if (v == r.premax) v = r.far_v;
    if (v == 0.0f) v = r.far_v;
    if (v >= r.far_v) v = r.far_v;
    if (v <= r.near_v) v = r.near_v;
    v = (v - r.norm_off) / r.norm_div;
    if (r.binarize) v = v < 0.5f ? 0.0f : 1.0f;
    return v;
}

// element index of source pixel (X, Y) in a dsz x dsz crop, -1 outside it
__device__ __forceinline__ int aug_index(long long X, long long Y, int dsz) {
    return (X >= 0 && X < dsz && Y >= 0 && Y < dsz) ? (int)Y * dsz + (int)X : -1;
}

// One output pixel (x, y) of the augmented crop: gather through the inverse map, z-rules, far-plane fill, re-normalise.
__device__ __forceinline__ float aug_warp_pixel(const AugRec& r, const float* __restrict__ im, int dsz, int x, int y) {
    if (r.warp == WARP_NONE) return aug_pixel_value(r, im[y * dsz + x] * r.den_scale + r.den_off, false);
    long long X, Y;
    if (r.warp == WARP_AFFINE) affine_source(r.m, x, y, X, Y);
    else persp_source(r.m, (x >> 6) << 6, x, y, true, X, Y);
    const int idx = aug_index(X, Y, dsz);
    return aug_pixel_value(r, idx >= 0 ? im[idx] * r.den_scale + r.den_off : 0.0f, true);
}

// Four consecutive output pixels (x .. x + 3, x % 4 == 0) of a crop that is NOT warped (r.warp == WARP_NONE, the fused kernel's only
// use of it): one 16-byte load, the same value rules as aug_warp_pixel.
__device__ __forceinline__ float4 aug_warp_quad(const AugRec& r, const float* __restrict__ im, int dsz, int x, int y) {
    const float4 t = *reinterpret_cast<const float4*>(im + y * dsz + x);
    return make_float4(aug_pixel_value(r, t.x * r.den_scale + r.den_off, false), aug_pixel_value(r, t.y * r.den_scale + r.den_off, false),
                       aug_pixel_value(r, t.z * r.den_scale + r.den_off, false), aug_pixel_value(r, t.w * r.den_scale + r.den_off, false));
}

// Four consecutive output pixels (x .. x + 3, x % 4 == 0: one row, one 64-wide block of cv::warpPerspective) of a WARPED crop in two
// halves, for a pixel pass that keeps MANY gathers in flight (round 6): the source element index of each of the four pixels (-1:
// outside the crop) with the terms that do not depend on x formed once -- the row part of the perspective map (nine float64 products)
// and of the affine map (two cvRound), a third of the float64 work per pixel --, and the value rules applied to the gathered elements.
// The same helpers on the same inputs as aug_warp_pixel: bit-identical results (tests: nbad == 0 in every mode).
__device__ __forceinline__ void aug_quad_index(const AugRec& r, int dsz, int x, int y, int (&idx)[4]) {
    long long X[4], Y[4];
    if (r.warp == WARP_AFFINE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) affine_source(r.m, x + j, y, X[j], Y[j]);
    } else {
        // The maps the augmentation builds are products of comToTransform matrices and their cofactor inverses: the bottom row is
        // EXACTLY (0, 0, 1) (0 / det and det / det of the same rounded products), so the float64 division per pixel (a third of the
        // pass) only runs for a truly projective map (see persp_source).
        const bool unit_w = r.m[6] == 0.0 && r.m[7] == 0.0 && r.m[8] == 1.0;
        const int bx = (x >> 6) << 6;
#pragma unroll
        for (int j = 0; j < 4; ++j) persp_source(r.m, bx, x + j, y, !unit_w, X[j], Y[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = aug_index(X[j], Y[j], dsz);
}

__device__ __forceinline__ float4 aug_quad_value(const AugRec& r, const float (&raw)[4], const int (&idx)[4]) {
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = aug_pixel_value(r, idx[j] >= 0 ? raw[j] * r.den_scale + r.den_off : 0.0f, true);
    return make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(DPP_THREADS) void augment_warp_kernel(const float* __restrict__ img, const AugRec* __restrict__ rec, int dsz,
                                                                   float* __restrict__ out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * DPP_THREADS + threadIdx.x;
    const int npix = dsz * dsz;
    if (p >= npix) return;
    const AugRec r = rec[b];
    const int y = p / dsz, x = p - y * dsz;
    out[(size_t)b * npix + p] = aug_warp_pixel(r, img + (size_t)b * npix, dsz, x, y);
}

// Advance the device draw counter: every workgroup takes a ticket once its own read of the counter is done (it is: the geometry
// consumed it before the barrier), the last one bumps the counter for the next launch and resets the ticket.  At the END of the
// kernel: an atomic with a returned value is a memory round trip, and in front of the barrier it delayed every pixel of the crop.
__device__ __forceinline__ void aug_take_ticket(unsigned long long* counter_rw, unsigned* ticket) {
    if (ticket == nullptr || threadIdx.x != 0) return;
    const unsigned long long c = *counter_rw;
    const unsigned one = 1u + (unsigned)(c >> 63);
    const unsigned t = atomicAdd(ticket, one);
    if (t == gridDim.x - 1) {
        *counter_rw = c + 1ull;
        *ticket = 0u;
    }
}

// The whole augmentation of a (macro-)batch as ONE launch.  Crop b is handled by S workgroups (S = a power of two chosen by the
// host so that the grid fills the chip at training batch sizes); each of them finds the crop maximum (the crop is 64 KB: after the
// first touch it is served by the XCD's L2, and the block -> (crop, split) map keeps the S workgroups of a crop on ONE XCD:
// workgroup w runs on XCD w % 8), lets its thread 0 do the per-sample geometry (identical, deterministic results in every
// split) and warps its share of the pixels, four consecutive x per thread and one 16-byte store.  Split 0 also writes the
// labels (and the optional records).  The draw counter lives on the device: after reading it every workgroup takes a ticket,
// and the one that draws the last ticket advances the counter for the next launch and resets the ticket -- so a recorded
// launch plan draws fresh parameters every step without a separate launch.
__global__ __launch_bounds__(DPP_THREADS) void augment_fused_kernel(PrepArgs a, float* __restrict__ out_x, int S,
                                                                    unsigned long long* counter_rw, unsigned* ticket) {
    dpp_kernarg_warm<sizeof(PrepArgs) + 32>();
    __shared__ float s_red[DPP_THREADS / DPP_WAVE];
    __shared__ float s_label[MAXJ3];
    __shared__ AugRec s_rec;
    const int w = blockIdx.x, tid = threadIdx.x;
    const int xcd = w & 7, q = w >> 3;                 // q-th workgroup of this XCD
    const int split = q % S, b = (q / S) * 8 + xcd;    // crops b with b % 8 == xcd live on this XCD
    const int npix = a.dsz * a.dsz;
    const bool live = b < a.B;
    const float* im = a.img + (size_t)(live ? b : 0) * npix;
    __shared__ AugLabelCtx s_lc;
    dpp_stamp(a.prof, 0);
    // Two jobs side by side: waves 1-3 find the maximum of the stored crop (`premax`, one pass over 64 KB), wave 0's first lane runs
    // the per-sample geometry, which needs the maximum only for ONE value (premax, patched in after the barrier).
    // (rotating the serial lane's wave with the workgroup index, so that co-resident workgroups do not queue their serial lanes on one
    //  SIMD, changed nothing: 26.0-26.5 us for every rotation, profiles/r03_augment_phases.txt)
    const int vt = tid;
    if (vt >= DPP_WAVE) {
        float mx = -3.4e38f;
        const int t = vt - DPP_WAVE, nt = DPP_THREADS - DPP_WAVE;
        int i0 = 0;
        if ((npix & 3) == 0 && (reinterpret_cast<uintptr_t>(im) & 15) == 0) {
            // batches of 8 loads in flight per thread: one load per iteration made this pass ~20 dependent L2 / HBM round trips,
            // the longest single item of the kernel at training batch sizes
            const float4* im4 = reinterpret_cast<const float4*>(im);
            const int n4 = npix >> 2;
            for (int i = t; i < n4; i += 8 * nt) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = i + u * nt;
                    v[u] = im4[j < n4 ? j : t];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) mx = fmaxf(mx, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
            }
            i0 = npix;
        }
        for (int i = i0 + t; i < npix; i += nt) mx = fmaxf(mx, im[i]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if ((vt & 63) == 0) s_red[vt >> 6] = mx;
    }
    if (vt < DPP_WAVE) {
        // the serial lane is what the workgroup waits for: its wave issues ahead of the streaming waves that share its SIMD
        DPP_SETPRIO(3);
        if (vt == 0 && live) aug_prepare_geometry(a, b, 0.0f, s_rec, s_lc);
        DPP_SETPRIO(0);
    }
    if (vt == 0) dpp_stamp(a.prof, 1);                 // geometry (+ ticket) done on lane 0
    __syncthreads();
    dpp_stamp(a.prof, 2);                              // ... and the crop maximum on waves 1-3
    if (!live) { aug_take_ticket(counter_rw, ticket); return; }
    if (vt == 0) {
        const float mx = fmaxf(fmaxf(s_red[1], s_red[2]), s_red[3]);
        s_rec.premax = mx * s_rec.den_scale + s_rec.den_off;      // two roundings (contraction is off), as in aug_prepare_geometry
    }
    __syncthreads();
    // The labels are shared out over the crop's S workgroups: in each, wave 0 transforms the joints (one lane per joint: every workgroup
    // needs the whole label) and projects ITS rounds of the PCA outputs (8 outputs per round, round r to workgroup r % S) while waves
    // 1-3 are already moving pixels; it then takes a small share of the pixels itself (an eighth of the workgroup's, against its normal
    // quarter).  With the whole projection on split 0 that workgroup's wave 0 spent 10-14 us there (tools/augment_phase.py) and was
    // what the launch waited for.
    const int chunk = npix / S;                          // host guarantees npix % (4 * S) == 0 and dsz % 4 == 0
    const int Q = chunk >> 2;                            // pixel quads of this workgroup
    int q0 = 0, q1 = Q, t = tid, nt = DPP_THREADS;
    {
        const int Qw = Q >= 8 * DPP_WAVE ? ((Q / 8) & ~(DPP_WAVE - 1)) : 0;
        if (vt < DPP_WAVE) {
            DPP_SETPRIO(3);                              // (the label wave starts its pixels late: it issues first until then)
            if (vt < a.J) aug_label_joint(a, b, s_lc, vt, s_label);
            DPP_WAVE_SYNC();
            aug_project_label(a, b, s_label, vt, DPP_WAVE, split, S);
            if (split == 0 && a.rec != nullptr && vt == 0) a.rec[b] = s_rec;
            DPP_SETPRIO(0);
            q1 = Qw; t = vt; nt = DPP_WAVE;
        } else {
            q0 = Qw; t = vt - DPP_WAVE; nt = DPP_THREADS - DPP_WAVE;
        }
    }
    dpp_stamp(a.prof, 3);                              // labels + projection (split 0, wave 0)
    const AugRec r = s_rec;
    float* o = out_x + (size_t)b * npix;
    if (r.warp == WARP_NONE) {
        for (int q = q0 + t; q < q1; q += nt) {
            const int p = split * chunk + q * 4;
            const int y = p / a.dsz, x = p - y * a.dsz;
            *reinterpret_cast<float4*>(o + p) = aug_warp_quad(r, im, a.dsz, x, y);        // p, dsz multiples of 4: x % 4 == 0
        }
    } else {
        // Round 6: the gathers of AUG_NB quads (24 pixels) of a thread are all issued before the first is used.  One quad per iteration
        // made the pass 5-6 dependent round trips to the L2 per thread (the indices of an iteration need the float64 map, its four
        // gathers were consumed on the spot): 12-15 us per workgroup (tools/augment_phase.py) for 64 KB of pixels.  Unconditional
        // loads (pixels outside the source crop and the lanes past the end read element 0 and are masked afterwards): a branch
        // between a load and its use would drain the queue again.
        constexpr int AUG_NB = 6;
        for (int q = q0 + t; q < q1; q += AUG_NB * nt) {
            int idx[AUG_NB][4];
            float raw[AUG_NB][4];
#pragma unroll
            for (int u = 0; u < AUG_NB; ++u) {
                const int qq = q + u * nt;
                const int p = split * chunk + (qq < q1 ? qq : q) * 4;
                const int y = p / a.dsz, x = p - y * a.dsz;
                aug_quad_index(r, a.dsz, x, y, idx[u]);
            }
#pragma unroll
            for (int u = 0; u < AUG_NB; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[u][j] = im[idx[u][j] >= 0 ? idx[u][j] : 0];
#pragma unroll
            for (int u = 0; u < AUG_NB; ++u) {
                const int qq = q + u * nt;
                if (qq < q1) *reinterpret_cast<float4*>(o + split * chunk + qq * 4) = aug_quad_value(r, raw[u], idx[u]);
            }
        }
    }
    dpp_stamp(a.prof, 4);
    aug_take_ticket(counter_rw, ticket);
}

}  // namespace

extern "C" size_t dpp_augment_record_bytes(void) { return sizeof(AugRec); }

// The kernel arguments both entry points build from their common parameters (the caller adds sample0 / gbatch / prof).
static PrepArgs aug_prep_args(const float* img, const float* com3d, const float* cube, const float* Mcrop, const float* gt3d, int B, int J,
                              int dsz, const int* mode, const double* off, const double* rot, const double* sc, const int* mode_table,
                              int n_modes, unsigned long long seed, unsigned long long counter, double sigma_com, double sigma_sc,
                              double rot_range, double fx, double fy, double ux, double uy, int flip_y, int norm_zero_one,
                              const float* pca_mean, const float* pca_comp, int E, void* records, float* out_y, int* out_mode,
                              const unsigned long long* counter_dev) {
    PrepArgs a;
    a.img = img; a.com3d = com3d; a.cube = cube; a.Mcrop = Mcrop; a.gt3d = gt3d;
    a.mode = mode; a.off = off; a.rot = rot; a.sc = sc; a.mode_table = mode_table; a.n_modes = n_modes;
    a.seed = seed; a.counter = counter; a.counter_dev = counter_dev; a.sigma_com = sigma_com; a.sigma_sc = sigma_sc; a.rot_range = rot_range;
    a.cam.fx = fx; a.cam.fy = fy; a.cam.ux = ux; a.cam.uy = uy; a.cam.flip_y = flip_y;
    a.B = B; a.J = J; a.dsz = dsz; a.norm01 = norm_zero_one & 1; a.binarize = (norm_zero_one >> 1) & 1; a.pca_mean = pca_mean; a.pca_comp = pca_comp; a.E = E;
    a.rec = static_cast<AugRec*>(records); a.out_y = out_y; a.out_mode = out_mode;
    return a;
}

extern "C" int dpp_augment_prepare(const float* img, const float* com3d, const float* cube, const float* Mcrop, const float* gt3d,
                                   int B, int J, int dsz, const int* mode, const double* off, const double* rot, const double* sc,
                                   const int* mode_table, int n_modes, unsigned long long seed, unsigned long long counter,
                                   double sigma_com, double sigma_sc, double rot_range, double fx, double fy, double ux, double uy,
                                   int flip_y, int norm_zero_one, const float* pca_mean, const float* pca_comp, int E, void* records,
                                   float* out_y, int* out_mode, const unsigned long long* counter_dev, dpp_stream_t stream) {
    if (!img || !com3d || !cube || !Mcrop || !gt3d || !records || !out_y || B < 1 || J < 1 || J * 3 > MAXJ3 || dsz < 1) return DPP_E_BADARG;
    if (!mode && (!mode_table || n_modes < 1)) return DPP_E_BADARG;
    if (mode && (!off || !rot || !sc)) return DPP_E_BADARG;
    if (pca_comp && (!pca_mean || E < 1)) return DPP_E_BADARG;
    PrepArgs a = aug_prep_args(img, com3d, cube, Mcrop, gt3d, B, J, dsz, mode, off, rot, sc, mode_table, n_modes, seed, counter, sigma_com,
                               sigma_sc, rot_range, fx, fy, ux, uy, flip_y, norm_zero_one, pca_mean, pca_comp, E, records, out_y, out_mode,
                               counter_dev);
    a.sample0 = 0; a.gbatch = (unsigned long long)B; a.prof = nullptr;
    DPP_LAUNCH(augment_prepare_kernel, dim3(B), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return dpp_launch_status();
}

extern "C" int dpp_augment(const float* img, const float* com3d, const float* cube, const float* Mcrop, const float* gt3d,
                           int B, int J, int dsz, const int* mode, const double* off, const double* rot, const double* sc,
                           const int* mode_table, int n_modes, unsigned long long seed, unsigned long long counter,
                           double sigma_com, double sigma_sc, double rot_range, double fx, double fy, double ux, double uy,
                           int flip_y, int norm_zero_one, const float* pca_mean, const float* pca_comp, int E, void* records,
                           float* out_x, float* out_y, int* out_mode, unsigned long long* counter_dev, unsigned* ticket,
                           unsigned long long sample0, unsigned long long global_batch, int splits, dpp_stream_t stream) {
    if (!img || !com3d || !cube || !Mcrop || !gt3d || !out_x || !out_y || B < 1 || J < 1 || J * 3 > MAXJ3 || dsz < 4 || (dsz & 3) || img == out_x)
        return DPP_E_BADARG;
    if (!mode && (!mode_table || n_modes < 1)) return DPP_E_BADARG;
    if (mode && (!off || !rot || !sc)) return DPP_E_BADARG;
    if (pca_comp && (!pca_mean || E < 1)) return DPP_E_BADARG;
    if (ticket && !counter_dev) return DPP_E_BADARG;
    if (global_batch < 1) global_batch = (unsigned long long)B;
    int S = splits;
    if (S <= 0) {                                   // enough workgroups for the chip: ~1024 at training batch sizes
        S = 1;
        while (S < 16 && B * S < 1024 && (dsz * dsz) % (8 * S) == 0 && dsz * dsz / (2 * S) >= DPP_THREADS * 4) S *= 2;
    }
    if (S < 1 || (S & (S - 1)) || (dsz * dsz) % (4 * S)) return DPP_E_BADARG;
    PrepArgs a = aug_prep_args(img, com3d, cube, Mcrop, gt3d, B, J, dsz, mode, off, rot, sc, mode_table, n_modes, seed, counter, sigma_com,
                               sigma_sc, rot_range, fx, fy, ux, uy, flip_y, norm_zero_one, pca_mean, pca_comp, E, records, out_y, out_mode,
                               counter_dev);
    a.sample0 = sample0; a.gbatch = global_batch; a.prof = dpp_prof_buffer;
    const int groups = dpp_cdiv(B, 8);             // crops are dealt to XCDs round-robin: 8 per group
    DPP_LAUNCH(augment_fused_kernel, dim3(groups * S * 8), dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), a, out_x, S,
               counter_dev, ticket);
    return dpp_launch_status();
}

namespace {
__global__ void counter_add_kernel(unsigned long long* c, unsigned long long inc) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *c += inc;
}
}  // namespace

extern "C" int dpp_counter_add(unsigned long long* counter, unsigned long long inc, dpp_stream_t stream) {
    if (!counter) return DPP_E_BADARG;
    DPP_LAUNCH(counter_add_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), counter, inc);
    return dpp_launch_status();
}

extern "C" int dpp_augment_warp(const float* img, const void* records, int B, int dsz, float* out, dpp_stream_t stream) {
    if (!img || !records || !out || B < 1 || dsz < 1 || img == out) return DPP_E_BADARG;
    dim3 grid(dpp_cdiv(dsz * dsz, DPP_THREADS), B);
    DPP_LAUNCH(augment_warp_kernel, grid, dim3(DPP_THREADS), 0, static_cast<hipStream_t>(stream), img,
                       static_cast<const AugRec*>(records), dsz, out);
    return dpp_launch_status();
}
