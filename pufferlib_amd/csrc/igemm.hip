// igemm.hip — fp32-MFMA implicit-GEMM kernels for the NatureCNN policy of BASELINE configs[3]
// (pufferlib/models.py:113-157 `Convolutional`: Conv2d(4,32,8,s4) - ReLU - Conv2d(32,64,4,s2) - ReLU - Conv2d(64,64,3,s1) - ReLU -
// Flatten - Linear(3136,512) - ReLU, heads Linear(512,A) / Linear(512,1); observations uint8 (4,84,84), `.float() / 255.0`).
//
// Every product of the forward pass and of loss.backward() is one of two contractions over v_mfma_f32_16x16x4_f32 (exact fp32
// FMA chains; the 1e-5 parity target rules out bf16):
//   rows form   C[m][n]  = sum_k A(m, k) * B[n][k]            forward conv / linear (m = output pixel or sample, k = patch index)
//                                                             and dX (m = INPUT pixel, k = (tap, oc), A = gathered dOut)
//   weight form G[k][n]  = sum_m A(m, k) * D[m][n]            dW (+ column sums of D = the bias gradient), split over row chunks
// A(m, k) is never materialised: the tile loader computes the address of the patch element (implicit im2col / col2im), so a conv
// layer reads its input once per k-slab from L2/HBM and nothing else.  Activations are NHWC f32 (patch index (ky, kx, ic), ic
// contiguous); the first layer reads the uint8 NCHW frames directly ((ic, ky, kx), kx contiguous: one aligned 32-bit word = four
// patch elements) as floats 0..255 — the `/ 255.0` is folded into its packed weights (forward) and into the reduction of its
// weight gradient, one VALU conversion per element instead of four.  dX of a stride-S layer runs as S*S phases (input pixels with equal
// (y mod S, x mod S) share the (KH/S)(KW/S) kernel taps that reach them), so no multiply is spent on the structural zeros of a
// transposed strided convolution; IH, IW need not be multiples of S (ragged phases of ceil(IH/S) x ceil(IW/S) pixel slots, the ones
// past the edge dropped by the epilogue), and input pixels no window covers receive exactly 0.
// Frames in any other layout — channel-last (H, W, C), a `[::d, ::d]` pixel stride, rows that are not multiples of four bytes — go through
// the strided uint8 mode (kAIm2colU8S): byte (ic, y, x) of a frame at ic*sc + y*sy + x*sx, patch order (ky, kx, ic), so that C = 4
// channel-last is one aligned word per pixel; C = 1 / 3 load bytes at four incrementally kept offsets.  Same `/ 255` folding.
//
// Address arithmetic is the cost that competes with the MFMAs (VALU and MFMA issue from the same SIMD port and do not overlap),
// so it is incremental: a thread keeps the (tap, channel) decomposition of its fixed k-quad (rows form) or its fixed row pair's
// (n, oy, ox) (weight form) and advances it by one slab with adds and compares; divisions happen once per tile.
//
// Tiling: 256 threads = 4 waves, k-slabs of 16, double-buffered in LDS, global loads of slab s+1 in flight under the MFMAs of
// slab s.  rows form: (64 MI) x (16 NI) output tile, both operands row-major in LDS with a 20-float row stride; lane (c, g) reads
// ONE float4 per 16 x 16 fragment and slab (row c, columns 4g..4g+3 — the MFMA's k-slot g then stands for k = 4g + kk in step kk,
// for A and B alike), 2 lanes per bank.  weight form: (64 KJ) x (16 NI) tile of G per workgroup (KJ = 1..4: the height that pads K
// least) and a chunk of rows; the partial sums
// of the row splits are reduced in f64 in a fixed order (deterministic) and scattered into torch's parameter layout.
#include <type_traits>

#include "common.hpp"
#include "mlp_tile.hpp"

namespace pfa {

constexpr int kIgThreads = 256;
constexpr int kIgBK = 16;
constexpr int kIgLS = kIgBK + 4;   // LDS row stride (floats) of a [row][16 k] slab

enum IgAMode : int { kADense = 0, kAIm2colF32 = 1, kAIm2colU8 = 2, kACol2im = 3, kAIm2colU8S = 4, kAIm2colPad = 5, kAIm2colU8P = 6 };
enum IgEpilogue : int { kEpiNone = 0, kEpiBias = 1, kEpiBiasRelu = 2, kEpiMask = 3, kEpiBiasAdd = 4, kEpiBiasAddRelu = 5, kEpiMaskAdd = 6 };
// Modes 5 / 6 — the stride-1 same-padded 3 x 3 convolutions of models.ProcgenResnet (models.py:159-231): a tap outside the image reads
// as 0.  Mode 5 (NHWC f32, IC a multiple of 4: a k-quad lies inside one pixel, one bounds test per quad, the shape of the col2im test)
// can apply ReLU as it loads (a residual block's conv0 reads relu(x) while the skip needs x itself); mode 6 reads strided uint8 frames
// with 1..4 channels (a quad may straddle pixels: one test per element; elements past KH*KW*IC read as 0 so the rows form can run K
// rounded up to 16).  Their epilogues 4..6 add a second [m][n] operand: the residual sum of the forward and of dX.

// One conv layer (valid padding): input [N][IH][IW][IC] (NHWC f32) or uint8 [N][IC][IH][IW]; output [N][OH][OW][OC] NHWC.
struct IgGeom {
    int IC, IH, IW, OC, OH, OW, KH, KW, S;
};

struct IgA {
    int mode;
    const void *ptr;   // dense: float [M][lda]; im2col f32: NHWC input; im2col u8: NCHW frames; col2im: dOut NHWC [N][OH][OW][OC]
    int lda;
    IgGeom g;
    int JH, JW, HP, WP;   // col2im: taps per phase (KH/S, KW/S) and pixel slots per phase and frame (ceil(IH/S), ceil(IW/S))
    // strided u8 (kAIm2colU8S): byte (ic, y, x) of frame n sits at n*fb + ic*sc + y*sy + x*sx (channel order and the `[::d, ::d]` of
    // models.py:148 are strides, not copies); word != 0: IC == 4 channel-last, every pixel one aligned 32-bit word; a slab of 16 patch
    // elements is adv_pix whole pixels + adv_ch channels
    // same-padded modes: adv_pix = the padding (K-1)/2; mode 5: word != 0 = ReLU on load; mode 6: adv_ch = KH*KW*IC (the true K)
    int sc, sy, sx, fb, word, adv_pix, adv_ch;
};

// -------------------------------------------------------------------------------------------------- the k part of an address
// Where patch elements k .. k+3 sit relative to a row's base element, kept incrementally (k advances by one slab at a time).
struct IgK {
    int off;          // element offset to add to the row base
    int p, q, ch;     // running decomposition: im2col f32 (ky, kx, ic) / u8 (ic, ky, kx) / col2im (jy, jx, oc) / strided u8 (ky, kx, ic)
    int o1, o2, o3;   // strided u8, byte path: the offsets of elements k+1 .. k+3 (they may sit in the next pixel or patch row)
};

// strided u8: byte offsets of patch elements k .. k+3 from (p, q, ch) = (ky, kx, ic) of element k; adds and compares only
__device__ __forceinline__ void ig_k_u8s_offsets(const IgA &a, IgK &s) {
    s.off = s.p * a.sy + s.q * a.sx + s.ch * a.sc;
    if (a.word) return;
    int o = s.off, q = s.q, ch = s.ch;
    auto step = [&]() {
        o += a.sc;
        if (++ch == a.g.IC) {
            ch = 0;
            o += a.sx - a.g.IC * a.sc;
            if (++q == a.g.KW) {
                q = 0;
                o += a.sy - a.g.KW * a.sx;
            }
        }
        return o;
    };
    s.o1 = step();
    s.o2 = step();
    s.o3 = step();
}

// same-padded uint8 (mode 6): elements k .. k+3 one by one — byte offsets (off, o1..o3) from the row's own pixel, tap rows / columns as
// bytes of p / q, validity (k + i < KH*KW*IC) in bits 0..3 of ch, k itself above them.  Divisions: once per slab, this layer has two.
__device__ __forceinline__ void ig_k_u8p(const IgA &a, IgK &s, int k) {
    int o[4];
    s.p = s.q = 0;
    s.ch = k << 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = k + i;
        const bool ok = kk < a.adv_ch;
        const int pix = ok ? kk / a.g.IC : 0, ic = ok ? kk - pix * a.g.IC : 0;
        const int ky = ok ? pix / a.g.KW : a.adv_pix, kx = ok ? pix - ky * a.g.KW : a.adv_pix;
        o[i] = ic * a.sc + (ky - a.adv_pix) * a.sy + (kx - a.adv_pix) * a.sx;
        s.p |= ky << (8 * i);
        s.q |= kx << (8 * i);
        s.ch |= (ok ? 1 : 0) << i;
    }
    s.off = o[0];
    s.o1 = o[1];
    s.o2 = o[2];
    s.o3 = o[3];
}

template <int MODE>
__device__ __forceinline__ IgK ig_k_init(const IgA &a, int k) {
    IgK s;
    if (MODE == kAIm2colPad) {          // k = (ky*KW + kx)*IC + ic; the row base is the output pixel's own input pixel
        const int pix = k / a.g.IC;
        s.ch = k - pix * a.g.IC;
        s.p = pix / a.g.KW;
        s.q = pix - s.p * a.g.KW;
        s.off = ((s.p - a.adv_pix) * a.g.IW + (s.q - a.adv_pix)) * a.g.IC + s.ch;
    } else if (MODE == kAIm2colU8P) {
        ig_k_u8p(a, s, k);
    } else if (MODE == kADense) {
        s.p = s.q = s.ch = 0;
        s.off = k;
    } else if (MODE == kAIm2colF32) {   // k = (ky*KW + kx)*IC + ic
        const int pix = k / a.g.IC;
        s.ch = k - pix * a.g.IC;
        s.p = pix / a.g.KW;
        s.q = pix - s.p * a.g.KW;
        s.off = (s.p * a.g.IW + s.q) * a.g.IC + s.ch;
    } else if (MODE == kAIm2colU8) {    // k = (ic*KH + ky)*KW + kx
        s.ch = k % a.g.KW;
        const int t = k / a.g.KW;
        s.q = t % a.g.KH;
        s.p = t / a.g.KH;
        s.off = (s.p * a.g.IH + s.q) * a.g.IW + s.ch;
    } else if (MODE == kAIm2colU8S) {   // k = (ky*KW + kx)*IC + ic
        const int pix = k / a.g.IC;
        s.ch = k - pix * a.g.IC;
        s.p = pix / a.g.KW;
        s.q = pix - s.p * a.g.KW;
        ig_k_u8s_offsets(a, s);
    } else {                              // k = (jy*JW + jx)*OC + oc; the row base is dOut pixel (yy, xx): tap (jy, jx) reads (yy-jy, xx-jx)
        const int pix = k / a.g.OC;
        s.ch = k - pix * a.g.OC;
        s.p = pix / a.JW;
        s.q = pix - s.p * a.JW;
        s.off = -(s.p * a.g.OW + s.q) * a.g.OC + s.ch;
    }
    return s;
}

template <int MODE>
__device__ __forceinline__ void ig_k_advance(const IgA &a, IgK &s) {   // k += 16
    if (MODE == kAIm2colPad) {
        s.ch += kIgBK;
        while (s.ch >= a.g.IC) {
            s.ch -= a.g.IC;
            if (++s.q == a.g.KW) {
                s.q = 0;
                ++s.p;
            }
        }
        s.off = ((s.p - a.adv_pix) * a.g.IW + (s.q - a.adv_pix)) * a.g.IC + s.ch;
    } else if (MODE == kAIm2colU8P) {
        ig_k_u8p(a, s, (s.ch >> 4) + kIgBK);
    } else if (MODE == kADense) {
        s.off += kIgBK;
    } else if (MODE == kAIm2colF32) {
        s.ch += kIgBK;
        while (s.ch >= a.g.IC) {
            s.ch -= a.g.IC;
            if (++s.q == a.g.KW) {
                s.q = 0;
                ++s.p;
            }
        }
        s.off = (s.p * a.g.IW + s.q) * a.g.IC + s.ch;
    } else if (MODE == kAIm2colU8) {
        s.ch += kIgBK;
        while (s.ch >= a.g.KW) {
            s.ch -= a.g.KW;
            if (++s.q == a.g.KH) {
                s.q = 0;
                ++s.p;
            }
        }
        s.off = (s.p * a.g.IH + s.q) * a.g.IW + s.ch;
    } else if (MODE == kAIm2colU8S) {
        s.ch += a.adv_ch;
        s.q += a.adv_pix;
        if (s.ch >= a.g.IC) {
            s.ch -= a.g.IC;
            ++s.q;
        }
        while (s.q >= a.g.KW) {
            s.q -= a.g.KW;
            ++s.p;
        }
        ig_k_u8s_offsets(a, s);
    } else {
        s.ch += kIgBK;
        while (s.ch >= a.g.OC) {
            s.ch -= a.g.OC;
            if (++s.q == a.JW) {
                s.q = 0;
                ++s.p;
            }
        }
        s.off = -(s.p * a.g.OW + s.q) * a.g.OC + s.ch;
    }
}

// ------------------------------------------------------------------------------------------------ the row part of an address
struct IgRow {
    int base;        // element offset of the row's first patch element (col2im: of dOut pixel (yy, xx), possibly outside the image)
    int y, x;        // col2im: (yy, xx); tap (jy, jx) reads dOut pixel (yy - jy, xx - jx) when that is inside the image
};

// rows form, col2im: m = (n, yy, xx) counts the input pixels of phase (py, px): y = yy*S + py, x = xx*S + px
template <int MODE>
__device__ __forceinline__ IgRow ig_row(const IgA &a, int m) {
    IgRow r;
    r.y = r.x = 0;
    if (MODE == kAIm2colPad || MODE == kAIm2colU8P) {   // OH == IH, OW == IW: the output pixel names the centre of its patch
        const int hw = a.g.IH * a.g.IW;
        const int n = m / hw, rem = m - n * hw;
        r.y = rem / a.g.IW;
        r.x = rem - r.y * a.g.IW;
        r.base = MODE == kAIm2colPad ? m * a.g.IC : n * a.fb + r.y * a.sy + r.x * a.sx;
    } else if (MODE == kADense) {
        r.base = m * a.lda;
    } else if (MODE == kAIm2colF32 || MODE == kAIm2colU8) {
        const int ohw = a.g.OH * a.g.OW;
        const int n = m / ohw, rem = m - n * ohw, oy = rem / a.g.OW, ox = rem - oy * a.g.OW;
        r.base = MODE == kAIm2colF32 ? ((n * a.g.IH + oy * a.g.S) * a.g.IW + ox * a.g.S) * a.g.IC
                                       : (n * a.g.IC * a.g.IH + oy * a.g.S) * a.g.IW + ox * a.g.S;
    } else if (MODE == kAIm2colU8S) {
        const int ohw = a.g.OH * a.g.OW;
        const int n = m / ohw, rem = m - n * ohw, oy = rem / a.g.OW, ox = rem - oy * a.g.OW;
        r.base = n * a.fb + oy * a.g.S * a.sy + ox * a.g.S * a.sx;
    } else {
        const int hw = a.HP * a.WP;
        const int n = m / hw, rem = m - n * hw, yy = rem / a.WP, xx = rem - yy * a.WP;
        r.base = ((n * a.g.OH + yy) * a.g.OW + xx) * a.g.OC;
        r.y = yy;
        r.x = xx;
    }
    return r;
}

#ifdef PFA_IG_BOUNDS   // debug builds (tools/experiments/igemm_index_check.hip): record the first out-of-range access instead of making it
__device__ long long ig_dbg_limits[3];   // elements of A, B, C
__device__ int ig_dbg[8];                // [0] hits, [1] operand (0 A, 1 B, 2 C), [2] index lo, [3] index hi, [4] blockIdx.x, [5] threadIdx.x, [6] aux
__device__ __forceinline__ bool ig_dbg_bad(int operand, long long idx, long long span, int aux) {
    if (idx >= 0 && idx + span <= ig_dbg_limits[operand]) return false;
    if (atomicAdd(&ig_dbg[0], 1) == 0) {
        ig_dbg[1] = operand;
        ig_dbg[2] = (int)(idx & 0xFFFFFFFF);
        ig_dbg[3] = (int)(idx >> 32);
        ig_dbg[4] = blockIdx.x;
        ig_dbg[5] = threadIdx.x;
        ig_dbg[6] = aux;
    }
    return true;
}
#define IG_DBG_BAD(op, idx, span, aux) ig_dbg_bad(op, idx, span, aux)
#else
#define IG_DBG_BAD(op, idx, span, aux) false
#endif

template <int MODE>
__device__ __forceinline__ float4 ig_load4(const IgA &a, const IgRow &r, const IgK &k) {
    if (MODE == kAIm2colPad) {   // the whole quad is one tap: zeros when it lies in the padding
        if ((unsigned)(r.y + k.p - a.adv_pix) >= (unsigned)a.g.IH || (unsigned)(r.x + k.q - a.adv_pix) >= (unsigned)a.g.IW)
            return make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v = *reinterpret_cast<const float4 *>((const float *)a.ptr + (r.base + k.off));
        if (a.word) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        return v;
    }
    if (MODE == kAIm2colU8P) {   // every element its own tap; `/ 255.0` rides in the other operand as in modes 2 and 4
        const uint8_t *p = (const uint8_t *)a.ptr + r.base;
        const int off[4] = {k.off, k.o1, k.o2, k.o3};
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int y = r.y + ((k.p >> (8 * i)) & 0xFF) - a.adv_pix, x = r.x + ((k.q >> (8 * i)) & 0xFF) - a.adv_pix;
            const bool ok = ((k.ch >> i) & 1) && (unsigned)y < (unsigned)a.g.IH && (unsigned)x < (unsigned)a.g.IW;
            v[i] = ok ? (float)p[off[i]] : 0.f;
        }
        return make_float4(v[0], v[1], v[2], v[3]);
    }
    if (MODE == kAIm2colU8) {   // four bytes = one aligned word, as floats 0..255; the `/ 255.0` of models.py:150 rides in the other operand
        const uint32_t w = *reinterpret_cast<const uint32_t *>((const uint8_t *)a.ptr + (r.base + k.off));   // (packed weights / dW scale)
        return make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24));
    }
    if (MODE == kAIm2colU8S) {   // bytes as floats 0..255 through three strides; the `/ 255.0` rides in the other operand as above
        const uint8_t *p = (const uint8_t *)a.ptr + r.base;
        if (a.word) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(p + k.off);
            return make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24));
        }
        return make_float4((float)p[k.off], (float)p[k.o1], (float)p[k.o2], (float)p[k.o3]);
    }
    if (MODE == kACol2im && ((unsigned)(r.y - k.p) >= (unsigned)a.g.OH || (unsigned)(r.x - k.q) >= (unsigned)a.g.OW))
        return make_float4(0.f, 0.f, 0.f, 0.f);
    if (IG_DBG_BAD(0, (long long)r.base + k.off, 4, k.off)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4 *>((const float *)a.ptr + (r.base + k.off));
}

// ------------------------------------------------------------------------------------------------------------------ rows form
// C[row(m)][n] = epilogue(sum_k A(m, k) B[n][k]); B row-major [N][ldb] (k contiguous); C row-major, row stride ldc.
// grid = (ceil(M / (64 MI)), N / (16 NI), phases); col2im: blockIdx.z = phase, M = pixels per phase, B = B0 + phase * N * ldb.
template <int MODE, int MI, int NI>
__global__ void __launch_bounds__(kIgThreads, 2) igemm_rows_kernel(IgA A, int M, int K, const float *__restrict__ B, int ldb, int N,
                                                                  float *__restrict__ Cout, int ldc, int epi, const float *__restrict__ bias,
                                                                  const float *__restrict__ mask, int ldmask, const float *__restrict__ addend,
                                                                  int ldadd) {
    constexpr int TM = 64 * MI, TN = 16 * NI;
    constexpr int kStage = (TM + TN) * kIgLS;
    __shared__ __attribute__((aligned(16))) float lds[2 * kStage];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), c = lane & 15, g = lane >> 4;
    // Workgroups are dealt round-robin to the 8 XCDs (each with its own L2); neighbouring row tiles read overlapping patches of the
    // same frames, so the tile index is permuted to give every XCD one contiguous run of tiles (grid.x is a multiple of 8).
    const int per_xcd = gridDim.x >> 3;
    const int tile_m = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const int m0 = tile_m * TM, n0 = blockIdx.y * TN;
    if (m0 >= M) return;
    const int py = MODE == kACol2im ? (int)blockIdx.z / A.g.S : 0, px = MODE == kACol2im ? (int)blockIdx.z % A.g.S : 0;
    B += (size_t)blockIdx.z * N * ldb;
    // loader role: slab row (tid >> 2) + 64 q, k-quad (tid & 3) * 4
    const int lr = tid >> 2, kq = (tid & 3) * 4;
    IgRow rows[MI];
#pragma unroll
    for (int q = 0; q < MI; ++q) {
        const int m = m0 + lr + 64 * q;
        rows[q] = ig_row<MODE>(A, m < M ? m : M - 1);      // rows past the end repeat the last one; the epilogue drops them
    }
    IgK kc = ig_k_init<MODE>(A, kq);
    const float *bp = B + (size_t)(n0 + (lr < TN ? lr : 0)) * ldb + kq;
    f32x4 acc[MI][NI];
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int stages = K / kIgBK;
    // global -> register prefetch one slab deep (two deep was measured: the extra registers cost occupancy, 60 vs 80 TFLOP/s),
    // register -> LDS double buffer
    float4 ra[MI], rb;
    auto fetch = [&](float4(&fa)[MI], float4 &fb) {   // the slab the cursor points at, then advance
#pragma unroll
        for (int q = 0; q < MI; ++q) fa[q] = ig_load4<MODE>(A, rows[q], kc);
        if (lr < TN && !IG_DBG_BAD(1, bp - B, 4, lr)) fb = *reinterpret_cast<const float4 *>(bp);
        ig_k_advance<MODE>(A, kc);
        bp += kIgBK;
    };
    auto stash = [&](int buf, const float4(&fa)[MI], const float4 &fb) {
        float *la = lds + buf * kStage, *lb = la + TM * kIgLS;
#pragma unroll
        for (int q = 0; q < MI; ++q) *reinterpret_cast<float4 *>(la + (lr + 64 * q) * kIgLS + kq) = fa[q];
        if (lr < TN) *reinterpret_cast<float4 *>(lb + lr * kIgLS + kq) = fb;
    };
    auto multiply = [&](int buf) {
        const float *la = lds + buf * kStage + (wv * 16 * MI + c) * kIgLS + 4 * g;
        const float *lb = lds + buf * kStage + TM * kIgLS + c * kIgLS + 4 * g;
        float4 fa[MI], fb[NI];
#pragma unroll
        for (int a = 0; a < MI; ++a) fa[a] = *reinterpret_cast<const float4 *>(la + a * 16 * kIgLS);
#pragma unroll
        for (int b = 0; b < NI; ++b) fb[b] = *reinterpret_cast<const float4 *>(lb + b * 16 * kIgLS);
        // step kk of the slab uses component kk of every fragment; consecutive MFMAs go to different accumulators
#pragma unroll
        for (int a = 0; a < MI; ++a)
#pragma unroll
            for (int b = 0; b < NI; ++b) acc[a][b] = mfma16(fa[a].x, fb[b].x, acc[a][b]);
#pragma unroll
        for (int a = 0; a < MI; ++a)
#pragma unroll
            for (int b = 0; b < NI; ++b) acc[a][b] = mfma16(fa[a].y, fb[b].y, acc[a][b]);
#pragma unroll
        for (int a = 0; a < MI; ++a)
#pragma unroll
            for (int b = 0; b < NI; ++b) acc[a][b] = mfma16(fa[a].z, fb[b].z, acc[a][b]);
#pragma unroll
        for (int a = 0; a < MI; ++a)
#pragma unroll
            for (int b = 0; b < NI; ++b) acc[a][b] = mfma16(fa[a].w, fb[b].w, acc[a][b]);
    };
    fetch(ra, rb);
    stash(0, ra, rb);
    __syncthreads();
    for (int s = 0; s < stages; ++s) {
        if (s + 1 < stages) fetch(ra, rb);
        multiply(s & 1);
        if (s + 1 < stages) stash((s & 1) ^ 1, ra, rb);
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < MI; ++a) {
        int en = 0, eyy = 0, exx = 0;
        if (MODE == kACol2im) {   // phase-local pixel of the first of this lane's four rows; the next ones by carry
            const int m = m0 + wv * 16 * MI + a * 16 + 4 * g, hw = A.HP * A.WP;
            en = m / hw;
            const int rem = m - en * hw;
            eyy = rem / A.WP;
            exx = rem - eyy * A.WP;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wv * 16 * MI + a * 16 + 4 * g + r;
            size_t orow = (size_t)m;
            bool inside = true;
            if (MODE == kACol2im) {   // -> input pixel; a slot of a ragged phase (IH or IW not a multiple of S) may lie past the edge
                inside = eyy * A.g.S + py < A.g.IH && exx * A.g.S + px < A.g.IW;
                orow = ((size_t)en * A.g.IH + (size_t)(eyy * A.g.S + py)) * A.g.IW + (size_t)(exx * A.g.S + px);
                if (++exx == A.WP) {
                    exx = 0;
                    if (++eyy == A.HP) {
                        eyy = 0;
                        ++en;
                    }
                }
            }
            if (m >= M || !inside) continue;
#pragma unroll
            for (int b = 0; b < NI; ++b) {
                const int n = n0 + b * 16 + c;
                float v = acc[a][b][r];
                if (epi == kEpiBias || epi == kEpiBiasRelu) v += bias[n];
                if (epi == kEpiBiasRelu) v = fmaxf(v, 0.0f);
                if (epi == kEpiMask) v = mask[orow * ldmask + n] > 0.0f ? v : 0.0f;   // relu' of the layer input, read where it was produced
                if constexpr (MODE == kAIm2colPad || MODE == kAIm2colU8P) {   // the residual sums (compiled into the same-padded modes only)
                    if (epi == kEpiBiasAdd || epi == kEpiBiasAddRelu) v = (v + bias[n]) + addend[orow * ldadd + n];   // conv1(..) + inputs
                    if (epi == kEpiBiasAddRelu) v = fmaxf(v, 0.0f);
                    if (epi == kEpiMaskAdd) v = (mask[orow * ldmask + n] > 0.0f ? v : 0.0f) + addend[orow * ldadd + n];   // dX + skip gradient
                }
                if (IG_DBG_BAD(2, (long long)(orow * ldc + n), 1, m)) continue;
                Cout[orow * ldc + n] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------- rows form on the bf16 matrix path (opt-in)
// The same contraction with every fp32 operand split into three bf16 pieces in the loader (a = hi + mid + lo, round to nearest each
// time; 24 mantissa bits in all) and every 16 x 16 x 32 tile product issued as the six partial products above 2^-24 relative — lo.hi,
// hi.lo, mid.mid, mid.hi, hi.mid, hi.hi, small terms first — on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: 6/16 of the fp32
// MFMA's matrix time per product.  The uint8 first layer needs three (its A values are integers 0..255: one exact bf16 piece).
// Measured against f64 the result is as close as the fp32 fma chain (tools/experiments/bf16_split_accuracy.py, gemm_bf16x6.hip);
// it is NOT the bit pattern of the fp32 kernel, so it is off unless pfa_igemm_set_products(1) asks for it (bench.py --products
// bf16x6, tests/test_gpu_cnn.py).  32-deep slabs, three bf16 planes [row][32 k] of 80-byte rows in LDS, single-buffered (46 KB for
// the 128 x 64 tile: three workgroups per CU), the next slab's global loads in flight under the products.
typedef __bf16 ig_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ig_bf16x2 __attribute__((ext_vector_type(2)));
typedef float ig_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t ig_pk_bf16(float a, float b) {   // two floats -> two bf16 (v_cvt_pk_bf16_f32, nearest even), a low
    ig_f32x2 v = {a, b};
    ig_bf16x2 r = __builtin_convertvector(v, ig_bf16x2);
    return *reinterpret_cast<uint32_t *>(&r);
}
__device__ __forceinline__ float ig_bf16_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float ig_bf16_hi(uint32_t p) { return __uint_as_float(p & 0xFFFF0000u); }
__device__ __forceinline__ void ig_split4(const float4 &x, uint2 &h, uint2 &m, uint2 &l) {
    h.x = ig_pk_bf16(x.x, x.y);
    h.y = ig_pk_bf16(x.z, x.w);
    const float r0 = x.x - ig_bf16_lo(h.x), r1 = x.y - ig_bf16_hi(h.x), r2 = x.z - ig_bf16_lo(h.y), r3 = x.w - ig_bf16_hi(h.y);
    m.x = ig_pk_bf16(r0, r1);
    m.y = ig_pk_bf16(r2, r3);
    l.x = ig_pk_bf16(r0 - ig_bf16_lo(m.x), r1 - ig_bf16_hi(m.x));
    l.y = ig_pk_bf16(r2 - ig_bf16_lo(m.y), r3 - ig_bf16_hi(m.y));
}

constexpr int kIgSplitBK = 32;
constexpr int kIgSplitRS = 80;   // bytes per LDS row of a plane: 32 bf16 + 16 bytes of padding (b128 fragment reads hit all banks once)

template <int MODE, int MI, int NI>
__global__ void __launch_bounds__(kIgThreads, 2) igemm_rows_split_kernel(IgA A, int M, int K, const float *__restrict__ B, int ldb, int N,
                                                                        float *__restrict__ Cout, int ldc, int epi, const float *__restrict__ bias,
                                                                        const float *__restrict__ mask, int ldmask) {
    constexpr int TM = 64 * MI, TN = 16 * NI, RS = kIgSplitRS, PLANE = (TM + TN) * RS;
    constexpr int RPP = 32, LA = TM / RPP, LB = TN / RPP;      // loader: 8 threads per slab row, 32 rows per pass
    constexpr bool kAInt = MODE == kAIm2colU8 || MODE == kAIm2colU8S;                // A = bytes as floats: exact in ONE bf16 piece
    static_assert(TN % RPP == 0 && LB >= 1 && LB <= 2, "the split form takes 32- and 64-column tiles");
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), c = lane & 15, g = lane >> 4;
    const int per_xcd = gridDim.x >> 3;
    const int tile_m = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const int m0 = tile_m * TM, n0 = blockIdx.y * TN;
    if (m0 >= M) return;
    const int py = MODE == kACol2im ? (int)blockIdx.z / A.g.S : 0, px = MODE == kACol2im ? (int)blockIdx.z % A.g.S : 0;
    B += (size_t)blockIdx.z * N * ldb;
    const int lr = tid >> 3, kq = (tid & 7) * 4;              // loader role: slab rows lr + 32 q, k-quad kq
    IgRow rows[LA];
#pragma unroll
    for (int q = 0; q < LA; ++q) {
        const int m = m0 + lr + RPP * q;
        rows[q] = ig_row<MODE>(A, m < M ? m : M - 1);
    }
    IgK kc = ig_k_init<MODE>(A, kq);
    const float *bp = B + (size_t)(n0 + lr) * ldb + kq;
    f32x4 acc[MI][NI];
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int stages = K / kIgSplitBK;
    float4 ra[LA], rb0, rb1 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&]() {   // the slab the cursor points at, then advance
#pragma unroll
        for (int q = 0; q < LA; ++q) ra[q] = ig_load4<MODE>(A, rows[q], kc);
        rb0 = *reinterpret_cast<const float4 *>(bp);
        if (LB > 1) rb1 = *reinterpret_cast<const float4 *>(bp + (size_t)RPP * ldb);
        ig_k_advance<MODE>(A, kc);
        ig_k_advance<MODE>(A, kc);
        bp += kIgSplitBK;
    };
    auto stash = [&]() {
        uint2 h, m, l;
#pragma unroll
        for (int q = 0; q < LA; ++q) {
            unsigned char *p = lds + (lr + RPP * q) * RS + kq * 2;
            if (kAInt) {
                *reinterpret_cast<uint2 *>(p) = make_uint2(ig_pk_bf16(ra[q].x, ra[q].y), ig_pk_bf16(ra[q].z, ra[q].w));
            } else {
                ig_split4(ra[q], h, m, l);
                *reinterpret_cast<uint2 *>(p) = h;
                *reinterpret_cast<uint2 *>(p + PLANE) = m;
                *reinterpret_cast<uint2 *>(p + 2 * PLANE) = l;
            }
        }
        unsigned char *pb = lds + (TM + lr) * RS + kq * 2;
        ig_split4(rb0, h, m, l);
        *reinterpret_cast<uint2 *>(pb) = h;
        *reinterpret_cast<uint2 *>(pb + PLANE) = m;
        *reinterpret_cast<uint2 *>(pb + 2 * PLANE) = l;
        if (LB > 1) {
            ig_split4(rb1, h, m, l);
            *reinterpret_cast<uint2 *>(pb + RPP * RS) = h;
            *reinterpret_cast<uint2 *>(pb + RPP * RS + PLANE) = m;
            *reinterpret_cast<uint2 *>(pb + RPP * RS + 2 * PLANE) = l;
        }
    };
    const unsigned char *la = lds + (wv * 16 * MI + c) * RS + g * 16, *lb = lds + (TM + c) * RS + g * 16;
    auto multiply = [&]() {
        ig_bf16x8 fa[kAInt ? 1 : 3][MI], fb[3][NI];
#pragma unroll
        for (int p = 0; p < (kAInt ? 1 : 3); ++p)
#pragma unroll
            for (int a = 0; a < MI; ++a) fa[p][a] = *reinterpret_cast<const ig_bf16x8 *>(la + p * PLANE + a * 16 * RS);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int b = 0; b < NI; ++b) fb[p][b] = *reinterpret_cast<const ig_bf16x8 *>(lb + p * PLANE + b * 16 * RS);
        // (piece of A, piece of B): 0 = hi, 1 = mid, 2 = lo; small terms first, consecutive MFMAs on different accumulators
        constexpr int kTerms = kAInt ? 3 : 6;
        constexpr int TA[6] = {kAInt ? 0 : 2, 0, kAInt ? 0 : 1, 1, 0, 0}, TB[6] = {kAInt ? 2 : 0, kAInt ? 1 : 2, kAInt ? 0 : 1, 0, 1, 0};
#pragma unroll
        for (int t = 0; t < kTerms; ++t)
#pragma unroll
            for (int a = 0; a < MI; ++a)
#pragma unroll
                for (int b = 0; b < NI; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[TA[t]][a], fb[TB[t]][b], acc[a][b], 0, 0, 0);
    };
    if (stages > 0) fetch();
    for (int s = 0; s < stages; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < stages) fetch();          // the next slab's global loads fly under this slab's products
        multiply();
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < MI; ++a) {
        int en = 0, eyy = 0, exx = 0;
        if (MODE == kACol2im) {
            const int m = m0 + wv * 16 * MI + a * 16 + 4 * g, hw = A.HP * A.WP;
            en = m / hw;
            const int rem = m - en * hw;
            eyy = rem / A.WP;
            exx = rem - eyy * A.WP;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wv * 16 * MI + a * 16 + 4 * g + r;
            size_t orow = (size_t)m;
            bool inside = true;
            if (MODE == kACol2im) {
                inside = eyy * A.g.S + py < A.g.IH && exx * A.g.S + px < A.g.IW;
                orow = ((size_t)en * A.g.IH + (size_t)(eyy * A.g.S + py)) * A.g.IW + (size_t)(exx * A.g.S + px);
                if (++exx == A.WP) {
                    exx = 0;
                    if (++eyy == A.HP) {
                        eyy = 0;
                        ++en;
                    }
                }
            }
            if (m >= M || !inside) continue;
#pragma unroll
            for (int b = 0; b < NI; ++b) {
                const int n = n0 + b * 16 + c;
                float v = acc[a][b][r];
                if (epi == kEpiBias || epi == kEpiBiasRelu) v += bias[n];
                if (epi == kEpiBiasRelu) v = fmaxf(v, 0.0f);
                if (epi == kEpiMask) v = mask[orow * ldmask + n] > 0.0f ? v : 0.0f;
                Cout[orow * ldc + n] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- weight form
// partial[split][k][n] = sum over the split's rows of A(m, k) D[m][n], and (k-tile 0 only) colpart[split][n] = sum of D[m][n];
// grid = ((K / 128 rounded up) * (N / (16 NI)), splits).  Wave w owns k rows 32w .. 32w+31 of the 128 x (16 NI) tile.
struct IgM {   // (n, oy, ox) of a row of an im2col operand, advanced by 16 rows per slab
    int n, oy, ox;
};
template <int MODE>
__device__ __forceinline__ int ig_m_base(const IgA &a, const IgM &r) {
    if (MODE == kAIm2colU8S || MODE == kAIm2colU8P) return r.n * a.fb + r.oy * a.g.S * a.sy + r.ox * a.g.S * a.sx;
    return MODE == kAIm2colF32 || MODE == kAIm2colPad ? ((r.n * a.g.IH + r.oy * a.g.S) * a.g.IW + r.ox * a.g.S) * a.g.IC
                                 : (r.n * a.g.IC * a.g.IH + r.oy * a.g.S) * a.g.IW + r.ox * a.g.S;
}

template <int MODE, int KJ, int NI>
__global__ void __launch_bounds__(kIgThreads, 2) igemm_weights_kernel(IgA A, int M, int K, const float *__restrict__ D, int ldd, int N,
                                                                     int rows_per_split, float *__restrict__ partial, double *__restrict__ colpart) {
    constexpr int TK = 64 * KJ, TN = 16 * NI, SA = TK + 16, SB = TN % 32 == 0 ? TN + 16 : TN + 32;
    constexpr int kStage = kIgBK * (SA + SB);
    constexpr int kDThreads = kIgBK * TN / 4;
    __shared__ __attribute__((aligned(16))) float lds[2 * kStage];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), c = lane & 15, g = lane >> 4;
    const int tiles_n = N / TN;
    const int ktile = blockIdx.x / tiles_n, k0 = ktile * TK, n0 = (blockIdx.x % tiles_n) * TN;
    const int m_lo = blockIdx.y * rows_per_split;
    const int m_hi = m_lo + rows_per_split < M ? m_lo + rows_per_split : M;
    const int stages = m_hi > m_lo ? (m_hi - m_lo + kIgBK - 1) / kIgBK : 0;
    // loader role: A row (tid >> 4) of the slab, k-quads (tid & 15) * 4 + 64 j, j < KJ — the k part is fixed for the whole kernel,
    // the row part is one cursor per thread.  Wave w owns k rows 16 KJ w .. 16 KJ (w + 1) - 1 of the tile (KJ fragments).
    const int ar = tid >> 4, aq = (tid & 15) * 4;
    bool k_ok[KJ];
    IgK kc[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
        const int ak = k0 + aq + 64 * j;
        k_ok[j] = ak < K;
        kc[j] = ig_k_init<MODE>(A, k_ok[j] ? ak : 0);
    }
    IgM rm;
    {
        const int m = m_lo + ar;
        if (MODE == kADense) {
            rm.n = m;
            rm.oy = rm.ox = 0;
        } else {
            const int ohw = A.g.OH * A.g.OW;
            rm.n = m / ohw;
            const int rem = m - rm.n * ohw;
            rm.oy = rem / A.g.OW;
            rm.ox = rem - rm.oy * A.g.OW;
        }
    }
    const int dr = tid / (TN / 4), dc = (tid % (TN / 4)) * 4;
    f32x4 acc[KJ][NI];
#pragma unroll
    for (int a = 0; a < KJ; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    double colsum = 0.0;
    float4 ra[KJ], rb;
    int mrow = m_lo;          // first row of the slab the cursors point at
    auto fetch = [&](float4(&fa)[KJ], float4 &fb) {
        IgRow r;
        r.y = r.x = 0;
        r.base = MODE == kADense ? rm.n * A.lda : ig_m_base<MODE>(A, rm);
        if (MODE == kAIm2colPad || MODE == kAIm2colU8P) {   // the padding test of ig_load4 needs the output pixel
            r.y = rm.oy;
            r.x = rm.ox;
        }
        const bool row_ok = mrow + ar < m_hi;
#pragma unroll
        for (int j = 0; j < KJ; ++j) fa[j] = (row_ok && k_ok[j]) ? ig_load4<MODE>(A, r, kc[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == kADense) {
            rm.n += kIgBK;
        } else {
            rm.ox += kIgBK;
            while (rm.ox >= A.g.OW) {
                rm.ox -= A.g.OW;
                if (++rm.oy == A.g.OH) {
                    rm.oy = 0;
                    ++rm.n;
                }
            }
        }
        fb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < kDThreads && mrow + dr < m_hi) fb = *reinterpret_cast<const float4 *>(D + (size_t)(mrow + dr) * ldd + n0 + dc);
        mrow += kIgBK;
    };
    auto stash = [&](int buf, const float4(&fa)[KJ], const float4 &fb) {
        float *la = lds + buf * kStage, *lb = la + kIgBK * SA;
#pragma unroll
        for (int j = 0; j < KJ; ++j) *reinterpret_cast<float4 *>(la + ar * SA + aq + 64 * j) = fa[j];
        if (tid < kDThreads) *reinterpret_cast<float4 *>(lb + dr * SB + dc) = fb;
    };
    auto multiply = [&](int buf) {
        const float *la = lds + buf * kStage + wv * 16 * KJ + c;
        const float *lb = lds + buf * kStage + kIgBK * SA + c;
#pragma unroll
        for (int kk = 0; kk < kIgBK / 4; ++kk) {
            float fa[KJ], fb[NI];
#pragma unroll
            for (int a = 0; a < KJ; ++a) fa[a] = la[(4 * kk + g) * SA + 16 * a];
#pragma unroll
            for (int b = 0; b < NI; ++b) fb[b] = lb[(4 * kk + g) * SB + 16 * b];
#pragma unroll
            for (int a = 0; a < KJ; ++a)
#pragma unroll
                for (int b = 0; b < NI; ++b) acc[a][b] = mfma16(fa[a], fb[b], acc[a][b]);
        }
        if (ktile == 0 && tid < TN) {   // bias gradient: column sums of this slab of D (rows past the split are zero in LDS)
            const float *lcol = lds + buf * kStage + kIgBK * SA + tid;
#pragma unroll
            for (int r = 0; r < kIgBK; ++r) colsum += (double)lcol[r * SB];
        }
    };
    if (stages > 0) {
        fetch(ra, rb);
        stash(0, ra, rb);
    }
    __syncthreads();
    for (int s = 0; s < stages; ++s) {
        if (s + 1 < stages) fetch(ra, rb);
        multiply(s & 1);
        if (s + 1 < stages) stash((s & 1) ^ 1, ra, rb);
        __syncthreads();
    }
    float *out = partial + (size_t)blockIdx.y * K * N;
#pragma unroll
    for (int a = 0; a < KJ; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + (wv * KJ + a) * 16 + 4 * g + r;
                if (k < K) out[(size_t)k * N + n0 + b * 16 + c] = acc[a][b][r];
            }
    if (ktile == 0 && tid < TN) colpart[(size_t)blockIdx.y * N + n0 + tid] = colsum;
}

// Sum of the split partials (f64, fixed order) scattered into the gradient in torch's layout.  perm: 0 = out[k*N + n] (a
// transposed Linear: [K][N] kept), 1 = Linear weight [n][k], 2 = conv weight [oc = n][ic][ky][kx] from k = (ky*KW + kx)*IC + ic,
// 3 = conv weight from k = (ic*KH + ky)*KW + kx, divided by 255 (the uint8 first layer: its loader hands out raw bytes).  Elements
// K*N .. K*N + N - 1: the bias gradient from the column-sum partials.  accumulate: += (micro-batches of one minibatch).
// 64 elements per workgroup, the splits dealt round-robin to its four waves and combined as (w0 + w1) + (w2 + w3).
__global__ void __launch_bounds__(256) igemm_weights_reduce_kernel(const float *__restrict__ partial, const double *__restrict__ colpart, int splits, int K,
                                                                  int N, float *__restrict__ out, float *__restrict__ bias_out, int perm, IgGeom g,
                                                                  int accumulate) {
    __shared__ double sh[4][64];
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + e;
    const long long kn = (long long)K * N;
    double s = 0.0;
    if (i < kn) {
        for (int q = sl; q < splits; q += 4) s += (double)partial[(size_t)q * kn + i];
    } else if (i < kn + N) {
        for (int q = sl; q < splits; q += 4) s += colpart[(size_t)q * N + (i - kn)];
    }
    sh[sl][e] = s;
    __syncthreads();
    if (sl != 0 || i >= kn + N) return;
    s = (sh[0][e] + sh[1][e]) + (sh[2][e] + sh[3][e]);
    if (i >= kn) {
        if (bias_out == nullptr) return;
        const int n = (int)(i - kn);
        bias_out[n] = (accumulate ? bias_out[n] : 0.0f) + (float)s;
        return;
    }
    const int k = (int)(i / N), n = (int)(i - (long long)k * N);
    long long p;
    if (perm == 0) p = i;
    else if (perm == 1) p = (long long)n * K + k;
    else if (perm == 2 || perm == 5) {   // 5: the strided uint8 first layer — mode-1 k order, bytes not yet divided by 255
        if (perm == 5) s /= 255.0;
        const int pix = k / g.IC, ic = k - pix * g.IC, ky = pix / g.KW, kx = pix - ky * g.KW;
        p = (((long long)n * g.IC + ic) * g.KH + ky) * g.KW + kx;
    } else if (perm == 3) {
        p = (long long)n * K + k;   // (ic, ky, kx) IS torch's order within an output channel
        s /= 255.0;
    } else {   // 4: Linear behind nn.Flatten of an NCHW tensor whose activations we keep NHWC: k = (y*IW + x)*IC + c -> c*IH*IW + y*IW + x
        const int pix = k / g.IC, cch = k - pix * g.IC;
        p = (long long)n * K + (long long)cch * g.IH * g.IW + pix;
    }
    out[p] = (accumulate ? out[p] : 0.0f) + (float)s;
}

// Weight re-packing after an optimizer step.  Conv [OC][IC][KH][KW] -> forward B [OC][k] with k in the loader's patch order
// (the uint8 first layer keeps torch's order and takes the / 255 of the observations), and dX B [phase][IC][(jy*JW + jx)*OC + oc] with
// phase = py*S + px and kernel tap (ky, kx) = (py + jy*S, px + jx*S).
__global__ void __launch_bounds__(256) ig_pack_conv_kernel(const float *__restrict__ w, IgGeom g, int u8_order, float *__restrict__ fwd,
                                                          float *__restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)g.OC * g.IC * g.KH * g.KW;
    if (i >= total) return;
    const int kx = (int)(i % g.KW);
    long long t = i / g.KW;
    const int ky = (int)(t % g.KH);
    t /= g.KH;
    const int ic = (int)(t % g.IC), oc = (int)(t / g.IC);
    const float v = w[i];
    const int K = g.IC * g.KH * g.KW;
    if (fwd) {   // the uint8 loader hands out raw bytes: its weights carry the `/ 255.0` of models.py:150
        if (u8_order == 1) fwd[(long long)oc * K + ((long long)ic * g.KH + ky) * g.KW + kx] = v / 255.0f;
        else if (u8_order == 2) fwd[(long long)oc * K + ((long long)ky * g.KW + kx) * g.IC + ic] = v / 255.0f;   // strided uint8 loader
        else fwd[(long long)oc * K + ((long long)ky * g.KW + kx) * g.IC + ic] = v;
    }
    if (dx) {
        const int JH = g.KH / g.S, JW = g.KW / g.S, py = ky % g.S, px = kx % g.S, jy = ky / g.S, jx = kx / g.S;
        const long long KP = (long long)JH * JW * g.OC;
        dx[((long long)(py * g.S + px) * g.IC + ic) * KP + ((long long)jy * JW + jx) * g.OC + oc] = v;
    }
}
// Linear(C*H*W, N) behind nn.Flatten (models.py:133): torch's column index is NCHW (c*H*W + y*W + x), our activation rows are NHWC
// ((y*W + x)*C + c).  perm_out [N][K'] (columns re-ordered: B of the forward) and t_out [K'][N] (B of dX).
__global__ void __launch_bounds__(256) ig_pack_fc_kernel(const float *__restrict__ w, int N, int Cc, int HW, float *__restrict__ perm_out,
                                                        float *__restrict__ t_out) {
    const int K = Cc * HW;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * K) return;
    const int kp = (int)(i % K), n = (int)(i / K);
    const int pix = kp / Cc, cch = kp - pix * Cc;
    const float v = w[(size_t)n * K + (size_t)cch * HW + pix];
    perm_out[i] = v;
    t_out[(size_t)kp * N + n] = v;
}
__global__ void __launch_bounds__(256) ig_transpose_kernel(const float *__restrict__ w, int N, int K, float *__restrict__ out) {   // [N][K] -> [K][N]
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * K) return;
    const int k = (int)(i % K), n = (int)(i / K);
    out[(size_t)k * N + n] = w[i];
}

// Stride-1 same-padded conv [OC][IC][KH][KW] -> forward B [OC][ldf] (k = (ky*KW + kx)*IC + ic; columns KH*KW*IC .. ldf-1 are the caller's
// zeros; u8: weights / 255) and dX B [IC][(ky'*KW + kx')*OC + oc] = w[oc][ic][KH-1-ky'][KW-1-kx']: dX of such a layer is the same mode-5
// product on dOut with the kernel flipped and the channel roles swapped.
__global__ void __launch_bounds__(256) ig_pack_conv_same_kernel(const float *__restrict__ w, IgGeom g, int u8, float *__restrict__ fwd, int ldf,
                                                               float *__restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)g.OC * g.IC * g.KH * g.KW;
    if (i >= total) return;
    const int kx = (int)(i % g.KW);
    long long t = i / g.KW;
    const int ky = (int)(t % g.KH);
    t /= g.KH;
    const int ic = (int)(t % g.IC), oc = (int)(t / g.IC);
    const float v = w[i];
    if (fwd) fwd[(long long)oc * ldf + ((long long)ky * g.KW + kx) * g.IC + ic] = u8 ? v / 255.0f : v;
    if (dx) dx[(long long)ic * g.KH * g.KW * g.OC + ((long long)(g.KH - 1 - ky) * g.KW + (g.KW - 1 - kx)) * g.OC + oc] = v;
}

// max_pool2d(kernel 3, stride 2, padding 1) on NHWC f32 [n][H][W][C] -> [n][PH][PW][C], PH = (H+1)/2, PW = (W+1)/2; one thread per
// output pixel and channel quad, the maximum over the in-image taps only (the padding never wins: a window always holds its centre).
__global__ void __launch_bounds__(256) ig_maxpool_fwd_kernel(const float *__restrict__ in, long long total, int H, int W, int C4, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int PH = (H + 1) / 2, PW = (W + 1) / 2;
    const int c = (int)(i % C4);
    long long t = i / C4;
    const int px = (int)(t % PW);
    t /= PW;
    const int py = (int)(t % PH);
    const long long n = t / PH;
    const float4 *src = reinterpret_cast<const float4 *>(in) + n * H * W * C4 + c;
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dy = -1; dy <= 1; ++dy) {
        const int y = 2 * py + dy;
        if ((unsigned)y >= (unsigned)H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int x = 2 * px + dx;
            if ((unsigned)x >= (unsigned)W) continue;
            const float4 v = src[((long long)y * W + x) * C4];
            m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
        }
    }
    reinterpret_cast<float4 *>(out)[i] = m;
}

// Its backward in gather form (no atomics, deterministic): an input pixel sums the dOut of the at most four windows (two per axis: a
// stride-2 window of 3 overlaps its neighbour in one row / column) whose maximum it is.  The pooled values are conv + bias with no
// ReLU in between, so exact ties have measure zero on real-valued maps; constant frame regions still produce them, and then the
// gradient goes where torch sends it: to the first tap in row-major order that holds the maximum.
__global__ void __launch_bounds__(256) ig_maxpool_bwd_kernel(const float *__restrict__ in, const float *__restrict__ out, const float *__restrict__ dout,
                                                            long long total, int H, int W, int C4, float *__restrict__ din) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int PH = (H + 1) / 2, PW = (W + 1) / 2;
    const int c = (int)(i % C4);
    long long t = i / C4;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    const long long n = t / H;
    const float4 *src = reinterpret_cast<const float4 *>(in) + n * H * W * C4 + c;
    const float4 mine4 = src[((long long)y * W + x) * C4];
    const float mine[4] = {mine4.x, mine4.y, mine4.z, mine4.w};
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int py = y / 2; py <= (y + 1) / 2 && py < PH; ++py)
        for (int px = x / 2; px <= (x + 1) / 2 && px < PW; ++px) {
            const long long o = ((n * PH + py) * PW + px) * C4 + c;
            const float4 m4 = reinterpret_cast<const float4 *>(out)[o], d4 = reinterpret_cast<const float4 *>(dout)[o];
            const float m[4] = {m4.x, m4.y, m4.z, m4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
            bool win[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) win[q] = mine[q] == m[q];
            if (!(win[0] || win[1] || win[2] || win[3])) continue;
            for (int ty = 2 * py - 1; ty <= y; ++ty) {          // an earlier tap with the same value takes the gradient (torch: first index)
                if (ty < 0) continue;
                for (int tx = 2 * px - 1; tx <= 2 * px + 1; ++tx) {
                    if (tx < 0 || tx >= W || (ty == y && tx >= x)) continue;
                    const float4 e4 = src[((long long)ty * W + tx) * C4];
                    const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) win[q] = win[q] && e[q] != m[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] += win[q] ? d[q] : 0.f;
        }
    reinterpret_cast<float4 *>(din)[i] = make_float4(g[0], g[1], g[2], g[3]);
}

static int ig_check_a(const pfa_igemm_operand *a, int64_t M, int K) {
    PFA_REQUIRE(a && a->ptr, "igemm: null A operand");
    PFA_REQUIRE(a->mode >= 0 && a->mode <= 6, "igemm: bad A mode %d", a->mode);
    PFA_REQUIRE(a->mode == kAIm2colU8P || (K >= 4 && K % 4 == 0), "igemm: K must be a multiple of 4 (got %d)", K);
    PFA_REQUIRE(((uintptr_t)a->ptr & 15) == 0, "igemm: the A operand must be 16-byte aligned");
    PFA_REQUIRE((a->reserved & ~1) == 0 && (a->reserved == 0 || a->mode == kAIm2colPad), "igemm: reserved bit 0 (ReLU on load) belongs to mode 5");
    if (a->mode == kAIm2colPad || a->mode == kAIm2colU8P) {   // stride 1, odd square kernel, padding (K-1)/2: the output is the input's size
        PFA_REQUIRE(a->S == 1 && a->KH == a->KW && a->KH >= 1 && a->KH % 2 == 1 && a->KH < 128 && a->OH == a->IH && a->OW == a->IW && a->IH >= 1 &&
                        a->IW >= 1 && a->IC >= 1 && a->OC >= 1,
                    "igemm: the same-padded modes take stride 1, an odd square kernel and OH == IH, OW == IW");
        const int64_t frames = M / ((int64_t)a->IH * a->IW) + 1;
        PFA_REQUIRE(frames * a->IC * a->IH * a->IW < (1ll << 31) && frames * a->OC * a->IH * a->IW < (1ll << 31),
                    "igemm: operand too large for 32-bit element offsets (split the rows)");
        const int kt = a->KH * a->KW * a->IC;
        if (a->mode == kAIm2colPad) {
            PFA_REQUIRE(a->IC % 4 == 0 && K == kt, "igemm: same-padded im2col f32 needs IC %% 4 == 0 and K == KH*KW*IC");
        } else {
            PFA_REQUIRE(a->IC <= 4 && (K == kt || (K % kIgBK == 0 && K >= kt && K < kt + kIgBK)),
                        "igemm: same-padded u8 needs IC <= 4 and K == KH*KW*IC (weight form) or that rounded up to 16 (rows form)");
            PFA_REQUIRE(a->sc >= 1 && a->sy >= 1 && a->sx >= 1 && a->frame_bytes >= 1 &&
                            (int64_t)(a->IC - 1) * a->sc + (int64_t)(a->IH - 1) * a->sy + (int64_t)(a->IW - 1) * a->sx < a->frame_bytes,
                        "igemm: same-padded u8: the last byte (IC-1)*sc + (IH-1)*sy + (IW-1)*sx must lie inside a frame of frame_bytes");
            PFA_REQUIRE(frames * a->frame_bytes < (1ll << 31), "igemm: operand too large for 32-bit element offsets (split the rows)");
        }
        return 0;
    }
    if (a->mode == kADense) {
        PFA_REQUIRE(a->lda % 4 == 0 && a->lda >= K, "igemm: dense lda must be a multiple of 4 and >= K");
        PFA_REQUIRE(M * a->lda < (1ll << 31), "igemm: operand too large for 32-bit element offsets (split the rows)");
        return 0;
    }
    PFA_REQUIRE(a->S >= 1 && a->KH >= 1 && a->KW >= 1 && a->OH == (a->IH - a->KH) / a->S + 1 && a->OW == (a->IW - a->KW) / a->S + 1,
                "igemm: inconsistent conv geometry");
    const int64_t frames = a->mode == kACol2im ? M / ((int64_t)a->IH * a->IW) + 1 : M / ((int64_t)a->OH * a->OW) + 1;
    PFA_REQUIRE(frames * a->IC * a->IH * a->IW < (1ll << 31) && frames * a->OC * a->OH * a->OW < (1ll << 31),
                "igemm: operand too large for 32-bit element offsets (split the rows)");
    if (a->mode == kAIm2colF32) PFA_REQUIRE(a->IC % 4 == 0 && K == a->KH * a->KW * a->IC, "igemm: im2col f32 needs IC %% 4 == 0 and K == KH*KW*IC");
    if (a->mode == kAIm2colU8)
        PFA_REQUIRE(a->KW % 4 == 0 && a->IW % 4 == 0 && a->S % 4 == 0 && (a->IC * a->IH * a->IW) % 4 == 0 && K == a->KH * a->KW * a->IC,
                    "igemm: im2col u8 needs KW, IW, S multiples of 4 (aligned 4-byte patch runs) and K == IC*KH*KW");
    if (a->mode == kAIm2colU8S) {
        PFA_REQUIRE(a->IC >= 1 && K == a->KH * a->KW * a->IC && K % kIgBK == 0, "igemm: strided u8 needs K == KH*KW*IC, a multiple of 16");
        PFA_REQUIRE(a->sc >= 1 && a->sy >= 1 && a->sx >= 1 && a->frame_bytes >= 1 &&
                        (int64_t)(a->IC - 1) * a->sc + (int64_t)(a->IH - 1) * a->sy + (int64_t)(a->IW - 1) * a->sx < a->frame_bytes,
                    "igemm: strided u8: the last byte (IC-1)*sc + (IH-1)*sy + (IW-1)*sx must lie inside a frame of frame_bytes");
        PFA_REQUIRE(frames * a->frame_bytes < (1ll << 31), "igemm: operand too large for 32-bit element offsets (split the rows)");
    }
    if (a->mode == kACol2im)
        PFA_REQUIRE(a->OC % 4 == 0 && K == a->KH * a->KW * a->OC && a->KH % a->S == 0 && a->KW % a->S == 0,
                    "igemm: col2im needs OC %% 4 == 0, K == KH*KW*OC, and KH, KW multiples of the stride");
    return 0;
}
static int g_ig_products = 0;   // 0: exact fp32 MFMA products (default); 1: six-term bf16 split products in the rows form

static IgA ig_make_a(const pfa_igemm_operand *a) {
    IgA r;
    r.mode = a->mode;
    r.ptr = a->ptr;
    r.lda = (int)a->lda;
    r.g = IgGeom{a->IC, a->IH, a->IW, a->OC, a->OH, a->OW, a->KH, a->KW, a->S};
    r.JH = r.JW = r.HP = r.WP = 0;
    r.sc = r.sy = r.sx = r.fb = r.word = r.adv_pix = r.adv_ch = 0;
    if (a->mode == kACol2im) {   // ragged phases: slots past the edge are computed and dropped by the epilogue
        r.JH = a->KH / a->S;
        r.JW = a->KW / a->S;
        r.HP = (a->IH + a->S - 1) / a->S;
        r.WP = (a->IW + a->S - 1) / a->S;
    }
    if (a->mode == kAIm2colU8S) {
        r.sc = a->sc;
        r.sy = a->sy;
        r.sx = a->sx;
        r.fb = a->frame_bytes;
        r.word = a->IC == 4 && a->sc == 1 && a->sx % 4 == 0 && a->sy % 4 == 0 && a->frame_bytes % 4 == 0;
        r.adv_pix = kIgBK / a->IC;
        r.adv_ch = kIgBK % a->IC;
    }
    if (a->mode == kAIm2colPad || a->mode == kAIm2colU8P) {
        r.adv_pix = a->KH / 2;
        r.word = a->reserved & 1;
        r.adv_ch = a->KH * a->KW * a->IC;
        if (a->mode == kAIm2colU8P) {
            r.sc = a->sc;
            r.sy = a->sy;
            r.sx = a->sx;
            r.fb = a->frame_bytes;
        }
    }
    return r;
}

// Launch plan of the weight form, shared by the workspace query and the launch: tile width over n, number of (k, n) tiles, row
// splits (>= 2048 rows each, about 2048 workgroups in all, at most 1024) and rows per split (a multiple of the k-slab).
struct IgWeightPlan {
    int tn, kj, tiles, splits;   // tile = (64 kj) x tn
    int rows_per_split;
};
static IgWeightPlan ig_weight_plan(int64_t M, int K, int N) {
    IgWeightPlan p;
    p.tn = N % 64 == 0 ? 64 : N % 32 == 0 ? 32 : 16;
    // tile height over k: the one of 256 / 192 / 128 that pads K least (ties: the taller — more MFMAs per loaded D row and barrier)
    p.kj = 2;
    int best = (K + 127) / 128 * 128;
    for (int kj = 3; kj <= 4; ++kj) {
        const int padded = (K + 64 * kj - 1) / (64 * kj) * (64 * kj);
        if (padded <= best) {
            best = padded;
            p.kj = kj;
        }
    }
    if (K <= 64) p.kj = 1;      // (one 64-row k-tile: the encoder gradient of a 64-float observation row)
    p.tiles = ((K + 64 * p.kj - 1) / (64 * p.kj)) * (N / p.tn);
    int64_t s = (M + 2047) / 2048;
    const int64_t cap = 2048 / p.tiles + 1;
    if (s > cap) s = cap;
    if (s > 1024) s = 1024;
    // A small G (few tiles) over many rows would leave most CUs idle at >= 2048 rows per split: go down to 256 rows per split until
    // ~1024 workgroups exist, as long as the partial sums stay small (<= 16 MB written and re-read).
    if (s * p.tiles < 1024) {
        int64_t want = (1024 + p.tiles - 1) / p.tiles;
        const int64_t by_rows = (M + 255) / 256, by_bytes = (16ll << 20) / ((int64_t)K * N * 4);
        if (want > by_rows) want = by_rows;
        if (want > by_bytes) want = by_bytes;
        if (want > s) s = want;
    }
    p.splits = (int)(s < 1 ? 1 : s);
    p.rows_per_split = (int)((((M + p.splits - 1) / p.splits) + 15) / 16 * 16);
    return p;
}
static size_t ig_partial_bytes(const IgWeightPlan &p, int K, int N) { return align_up((size_t)p.splits * (size_t)K * (size_t)N * sizeof(float), 256); }

// Launch plan of the rows form, shared by the launch and pfa_igemm_rows_plan: product form, tile (64 mi) x (16 ni) and the number of
// row tiles (grid.x is that rounded up to 8, one run of tiles per XCD).  Mp, Kp: rows and contraction length per phase.
struct IgRowsPlan {
    int split;   // 1: the six-term bf16 kernel, 0: the fp32 kernel
    int mi, ni;
    long long tiles;
};
static IgRowsPlan ig_rows_plan(int mode, long long Mp, int Kp, int N) {
    IgRowsPlan p;
    const int tn = N % 64 == 0 ? 64 : N % 32 == 0 ? 32 : 16;
    // A dense product over few rows (one rollout step of the width-general policies: 4096 rows) fills the chip only with 64-row tiles.
    const bool few = mode == kADense && ((Mp + (tn == 16 ? 255 : 127)) / (tn == 16 ? 256 : 128)) * (N / tn) < 256;
    // opt-in: the six-term bf16 form of the same products (modes 5, 6: always the fp32 kernel)
    p.split = g_ig_products == 1 && !few && tn >= 32 && Kp % kIgSplitBK == 0 && mode <= kAIm2colU8S;
    p.ni = tn / 16;
    if (p.split) p.mi = 2;
    else if (few) p.mi = 1;
    else p.mi = tn == 16 ? 4 : 2;   // (128 x 32 beats 256 x 32: the smaller stage keeps more workgroups per CU)
    p.tiles = (Mp + 64 * p.mi - 1) / (64 * p.mi);
    return p;
}

}  // namespace pfa

using namespace pfa;

template <int V>
using IgInt = std::integral_constant<int, V>;   // tile sizes as arguments of the generic launch lambdas
// Turns the run-time operand mode into a template argument: f(integral_constant<IgAMode, M>) for the M of the list that `mode`
// equals, the LAST one otherwise (ig_check_a has let only the enum's values through).  A generic callable is instantiated for every
// mode it is offered, so each site lists exactly the modes its kernel is built for.
template <IgAMode M, IgAMode... Rest, typename F>
static void ig_with_mode(int mode, F &&f) {
    if constexpr (sizeof...(Rest) == 0) {
        f(std::integral_constant<IgAMode, M>{});
    } else {
        if (mode == M) f(std::integral_constant<IgAMode, M>{});
        else ig_with_mode<Rest...>(mode, f);
    }
}

static int ig_rows(const pfa_igemm_operand *a, int64_t M, int32_t K, const float *B, int32_t ldb, int32_t N, float *C, int32_t ldc, int32_t epilogue,
                   const float *bias, const float *mask, int32_t ldmask, const float *addend, int32_t ldadd, pfa_stream_t stream);

extern "C" int pfa_igemm_rows(const pfa_igemm_operand *a, int64_t M, int32_t K, const float *B, int32_t ldb, int32_t N, float *C, int32_t ldc,
                              int32_t epilogue, const float *bias, const float *mask, int32_t ldmask, pfa_stream_t stream) {
    PFA_REQUIRE(epilogue >= 0 && epilogue <= 3, "igemm.rows: bad epilogue");
    return ig_rows(a, M, K, B, ldb, N, C, ldc, epilogue, bias, mask, ldmask, nullptr, 0, stream);
}

extern "C" int pfa_igemm_rows_add(const pfa_igemm_operand *a, int64_t M, int32_t K, const float *B, int32_t ldb, int32_t N, float *C, int32_t ldc,
                                  int32_t epilogue, const float *bias, const float *mask, int32_t ldmask, const float *addend, int32_t ldadd,
                                  pfa_stream_t stream) {
    PFA_REQUIRE(a && (a->mode == kAIm2colPad || a->mode == kAIm2colU8P), "igemm.rows_add: the residual epilogues belong to the same-padded modes 5 and 6");
    PFA_REQUIRE(epilogue >= 0 && epilogue <= 6, "igemm.rows_add: bad epilogue");
    PFA_REQUIRE(epilogue < kEpiBiasAdd || (addend && ldadd >= N && addend != C), "igemm.rows_add: epilogues 4..6 need an addend [M][ldadd >= N] that is not the output");
    PFA_REQUIRE((epilogue != kEpiBiasAdd && epilogue != kEpiBiasAddRelu) || bias, "igemm.rows_add: bias epilogue without a bias vector");
    PFA_REQUIRE(epilogue != kEpiMaskAdd || (mask && ldmask >= N), "igemm.rows_add: mask epilogue without a mask");
    return ig_rows(a, M, K, B, ldb, N, C, ldc, epilogue, bias, mask, ldmask, addend, ldadd, stream);
}

static int ig_rows(const pfa_igemm_operand *a, int64_t M, int32_t K, const float *B, int32_t ldb, int32_t N, float *C, int32_t ldc, int32_t epilogue,
                   const float *bias, const float *mask, int32_t ldmask, const float *addend, int32_t ldadd, pfa_stream_t stream) {
    if (int rc = ig_check_a(a, M, K)) return rc;
    PFA_REQUIRE(M >= 0 && M < (1ll << 31) && B && C && N >= 16 && N % 16 == 0 && ldc >= N, "igemm.rows: bad shapes (N must be a multiple of 16)");
    PFA_REQUIRE(((uintptr_t)B & 15) == 0 && ldb % 4 == 0, "igemm.rows: B must be 16-byte aligned with ldb a multiple of 4");
    PFA_REQUIRE((epilogue != kEpiBias && epilogue != kEpiBiasRelu) || bias, "igemm.rows: bias epilogue without a bias vector");
    PFA_REQUIRE(epilogue != kEpiMask || (mask && ldmask >= N), "igemm.rows: mask epilogue without a mask");
    if (M == 0) return 0;
    const IgA A = ig_make_a(a);
    int phases = 1, Kp = K;
    long long Mp = M;
    if (A.mode == kACol2im) {   // S*S phases of M / (S*S) pixels, each contracting over its own K / (S*S) taps x channels
        phases = A.g.S * A.g.S;
        PFA_REQUIRE(M % ((long long)A.g.IH * A.g.IW) == 0, "igemm.rows: col2im rows must be whole frames");
        Mp = M / ((long long)A.g.IH * A.g.IW) * A.HP * A.WP;   // pixel slots per phase (== M / phases when IH, IW are multiples of S)
        Kp = K / phases;
    }
    PFA_REQUIRE(Kp % kIgBK == 0 && ldb >= Kp, "igemm.rows: the contraction length (per phase) must be a multiple of 16 and ldb >= it");
    ScopedKernelTimer timer("igemm_rows", (hipStream_t)stream);
    const IgRowsPlan plan = ig_rows_plan(A.mode, Mp, Kp, N);
    const unsigned grid_x = (unsigned)((plan.tiles + 7) / 8 * 8);
    auto rows = [&](auto mode, auto mi, auto ni) {   // the fp32 kernel on (64 MI) x (16 NI) tiles
        constexpr int MI = decltype(mi)::value, NI = decltype(ni)::value;
        hipLaunchKernelGGL((igemm_rows_kernel<decltype(mode)::value, MI, NI>), dim3(grid_x, N / (16 * NI), phases),
                           dim3(kIgThreads), 0, (hipStream_t)stream, A, (int)Mp, (int)Kp, B, (int)ldb, (int)N, C, (int)ldc, (int)epilogue,
                           bias, mask, (int)ldmask, addend, (int)ldadd);
    };
    auto rows_any = [&](auto mi, auto ni) {   // ... for whatever operand mode A has
        ig_with_mode<kAIm2colPad, kAIm2colU8P, kADense, kAIm2colF32, kAIm2colU8, kAIm2colU8S, kACol2im>(A.mode, [&](auto mode) { rows(mode, mi, ni); });
    };
    auto split = [&](auto ni) {   // the six-term bf16 form on 128 x (16 NI) tiles
        ig_with_mode<kADense, kAIm2colF32, kAIm2colU8, kAIm2colU8S, kACol2im>(A.mode, [&](auto mode) {
            hipLaunchKernelGGL((igemm_rows_split_kernel<decltype(mode)::value, 2, decltype(ni)::value>),
                               dim3(grid_x, N / (16 * decltype(ni)::value), phases), dim3(kIgThreads), 0, (hipStream_t)stream,
                               A, (int)Mp, (int)Kp, B, (int)ldb, (int)N, C, (int)ldc, (int)epilogue, bias, mask, (int)ldmask);
        });
    };
    constexpr IgInt<1> i1{};
    constexpr IgInt<2> i2{};
    constexpr IgInt<4> i4{};
    if (plan.split) {
        if (plan.ni == 4) split(i4);
        else split(i2);
    } else if (plan.mi == 1) {   // the 64-row tiles of a small dense product
        constexpr std::integral_constant<IgAMode, kADense> dense{};
        if (plan.ni == 4) rows(dense, i1, i4);
        else if (plan.ni == 2) rows(dense, i1, i2);
        else rows(dense, i1, i1);
    } else if (plan.ni == 4) {
        rows_any(i2, i4);
    } else if (plan.ni == 2) {
        rows_any(i2, i2);
    } else {
        rows_any(i4, i1);
    }
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_igemm_rows_plan(int32_t mode, int64_t M, int32_t K, int32_t N, int32_t *out4_host) {
    PFA_REQUIRE(out4_host && mode >= 0 && mode <= 6 && M >= 1 && M < (1ll << 31) && K >= kIgBK && K % kIgBK == 0 && N >= 16 && N % 16 == 0,
                "igemm.rows_plan: mode 0..6, rows >= 1, K (per phase) and N multiples of 16");
    const IgRowsPlan p = ig_rows_plan(mode, M, K, N);
    out4_host[0] = p.split;
    out4_host[1] = 64 * p.mi;
    out4_host[2] = 16 * p.ni;
    out4_host[3] = (int32_t)p.tiles;
    return 0;
}

extern "C" int pfa_igemm_set_products(int32_t mode) {
    PFA_REQUIRE(mode == 0 || mode == 1, "igemm.set_products: 0 = fp32 MFMA (default), 1 = six bf16 partial products per fp32 product");
    g_ig_products = mode;
    return 0;
}
extern "C" int pfa_igemm_get_products(void) { return g_ig_products; }

extern "C" size_t pfa_igemm_weights_workspace_bytes(int64_t M, int32_t K, int32_t N) {
    if (M < 1 || K < 4 || N < 16 || N % 16 != 0) return 0;
    const IgWeightPlan p = ig_weight_plan(M, K, N);
    return ig_partial_bytes(p, K, N) + (size_t)p.splits * (size_t)N * sizeof(double) + 256;
}

extern "C" int pfa_igemm_weights_plan(int64_t M, int32_t K, int32_t N, int32_t *out5_host) {
    PFA_REQUIRE(out5_host && M >= 1 && M < (1ll << 31) && K >= 4 && K % 4 == 0 && N >= 16 && N % 16 == 0,
                "igemm.weights_plan: rows >= 1, K a multiple of 4, N a multiple of 16");
    const IgWeightPlan p = ig_weight_plan(M, K, N);
    out5_host[0] = p.tn;
    out5_host[1] = 64 * p.kj;
    out5_host[2] = p.tiles;
    out5_host[3] = p.splits;
    out5_host[4] = p.rows_per_split;
    return 0;
}

extern "C" int pfa_igemm_weights(const pfa_igemm_operand *a, int64_t M, int32_t K, const float *D, int32_t ldd, int32_t N, float *out,
                                 int32_t perm, int32_t accumulate, float *bias_out, void *workspace, pfa_stream_t stream) {
    if (int rc = ig_check_a(a, M, K)) return rc;
    PFA_REQUIRE(a->mode != kACol2im, "igemm.weights: the col2im operand belongs to the rows form");
    PFA_REQUIRE(M >= 1 && M < (1ll << 31) && D && out && workspace && N >= 16 && N % 16 == 0 && ldd >= N && ldd % 4 == 0 && ((uintptr_t)D & 15) == 0,
                "igemm.weights: bad shapes");
    PFA_REQUIRE(perm >= 0 && perm <= 5, "igemm.weights: bad permutation");
    const IgA A = ig_make_a(a);
    const IgWeightPlan p = ig_weight_plan(M, K, N);
    float *partial = (float *)workspace;
    double *colpart = (double *)((char *)workspace + ig_partial_bytes(p, K, N));
    const dim3 grid(p.tiles, p.splits);
    {
        ScopedKernelTimer timer("igemm_weights", (hipStream_t)stream);
        auto weights = [&](auto ni) {
            ig_with_mode<kADense, kAIm2colF32, kAIm2colU8S, kAIm2colPad, kAIm2colU8P, kAIm2colU8>(A.mode, [&](auto mode) {
                constexpr IgAMode MODE = decltype(mode)::value;
                constexpr int NI = decltype(ni)::value;
                auto go = [&](auto kj) {
                    hipLaunchKernelGGL((igemm_weights_kernel<MODE, decltype(kj)::value, NI>), grid, dim3(kIgThreads), 0, (hipStream_t)stream, A, (int)M, (int)K, D,
                                       (int)ldd, (int)N, p.rows_per_split, partial, colpart);
                };
                if (p.kj == 4) return go(IgInt<4>{});
                if (p.kj == 3) return go(IgInt<3>{});
                if constexpr (MODE == kADense || MODE == kAIm2colU8S) {   // the only operands whose K comes this small
                    if (p.kj == 1) return go(IgInt<1>{});
                }
                go(IgInt<2>{});
            });
        };
        if (p.tn == 64) weights(IgInt<4>{});
        else if (p.tn == 32) weights(IgInt<2>{});
        else weights(IgInt<1>{});
        PFA_LAUNCH_CHECK();
    }
    const long long total = (long long)K * N + N;
    hipLaunchKernelGGL(igemm_weights_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, (hipStream_t)stream, partial, colpart, p.splits,
                       (int)K, (int)N, out, bias_out, (int)perm, A.g, (int)accumulate);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_cnn_pack_conv(const float *w, const pfa_igemm_operand *geom, int32_t u8_order, float *fwd, float *dx, pfa_stream_t stream) {
    PFA_REQUIRE(w && geom && (fwd || dx), "cnn.pack_conv: null buffer");
    const IgA A = ig_make_a(geom);
    PFA_REQUIRE(!dx || (A.g.S >= 1 && A.g.KH % A.g.S == 0 && A.g.KW % A.g.S == 0), "cnn.pack_conv: the dX form needs KH, KW multiples of the stride");
    const long long total = (long long)A.g.OC * A.g.IC * A.g.KH * A.g.KW;
    hipLaunchKernelGGL(ig_pack_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, A.g, (int)u8_order, fwd, dx);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_cnn_transpose(const float *w, int32_t N, int32_t K, float *out, pfa_stream_t stream) {
    PFA_REQUIRE(w && out && N >= 1 && K >= 1, "cnn.transpose: bad arguments");
    const long long total = (long long)N * K;
    hipLaunchKernelGGL(ig_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (int)N, (int)K, out);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_cnn_pack_fc(const float *w, int32_t N, int32_t channels, int32_t hw, float *perm_out, float *t_out, pfa_stream_t stream) {
    PFA_REQUIRE(w && perm_out && t_out && N >= 1 && channels >= 1 && hw >= 1, "cnn.pack_fc: bad arguments");
    const long long total = (long long)N * channels * hw;
    hipLaunchKernelGGL(ig_pack_fc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (int)N, (int)channels, (int)hw,
                       perm_out, t_out);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_cnn_pack_conv_same(const float *w, const pfa_igemm_operand *geom, int32_t u8, float *fwd, int32_t ldf, float *dx, pfa_stream_t stream) {
    PFA_REQUIRE(w && geom && (fwd || dx), "cnn.pack_conv_same: null buffer");
    const IgGeom g{geom->IC, geom->IH, geom->IW, geom->OC, geom->OH, geom->OW, geom->KH, geom->KW, geom->S};
    PFA_REQUIRE(g.S == 1 && g.KH == g.KW && g.KH % 2 == 1 && g.IC >= 1 && g.OC >= 1, "cnn.pack_conv_same: stride 1 and an odd square kernel");
    PFA_REQUIRE(!fwd || ldf >= g.KH * g.KW * g.IC, "cnn.pack_conv_same: ldf must hold KH*KW*IC columns");
    const long long total = (long long)g.OC * g.IC * g.KH * g.KW;
    hipLaunchKernelGGL(ig_pack_conv_same_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, g, (int)u8, fwd, (int)ldf, dx);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_maxpool3s2_forward(const float *in, int64_t frames, int32_t H, int32_t W, int32_t channels, float *out, pfa_stream_t stream) {
    PFA_REQUIRE(in && out && frames >= 0 && H >= 1 && W >= 1 && channels >= 4 && channels % 4 == 0, "maxpool3s2.forward: bad arguments (channels a multiple of 4)");
    PFA_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 15) == 0, "maxpool3s2.forward: buffers must be 16-byte aligned");
    const long long total = (long long)frames * ((H + 1) / 2) * ((W + 1) / 2) * (channels / 4);
    if (total == 0) return 0;
    PFA_REQUIRE((total + 255) / 256 < (1ll << 31), "maxpool3s2.forward: too many elements for one launch");
    hipLaunchKernelGGL(ig_maxpool_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, total, (int)H, (int)W,
                       (int)(channels / 4), out);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_maxpool3s2_backward(const float *in, const float *out, const float *dout, int64_t frames, int32_t H, int32_t W, int32_t channels,
                                       float *din, pfa_stream_t stream) {
    PFA_REQUIRE(in && out && dout && din && frames >= 0 && H >= 1 && W >= 1 && channels >= 4 && channels % 4 == 0,
                "maxpool3s2.backward: bad arguments (channels a multiple of 4)");
    PFA_REQUIRE((((uintptr_t)in | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)din) & 15) == 0, "maxpool3s2.backward: buffers must be 16-byte aligned");
    const long long total = (long long)frames * H * W * (channels / 4);
    if (total == 0) return 0;
    PFA_REQUIRE((total + 255) / 256 < (1ll << 31), "maxpool3s2.backward: too many elements for one launch");
    hipLaunchKernelGGL(ig_maxpool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, dout, total, (int)H, (int)W,
                       (int)(channels / 4), din);
    PFA_LAUNCH_CHECK();
    return 0;
}
