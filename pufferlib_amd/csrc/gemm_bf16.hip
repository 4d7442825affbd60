// gemm_bf16.hip — the weight-gradient contractions of gemm.hip,
//   C[mo][no] = sum_k A[k][mo] * B[k][no]        (C = A^T B, k = minibatch rows; two-operand form: columns >= nb come from B2)
// in the OPT-IN bf16x6 product form (pfa_igemm_set_products(1)): every fp32 operand value is split into three bf16 pieces and every
// product is issued as its six partial products above 2^-24 on v_mfma_f32_16x16x32_bf16, small terms first (kBfTA / kBfTB), fp32
// accumulation.  Same output tiling (TM = 16 WR MI, TN = 16 WC NI, four waves), same split over k and the same workspace of fp32 partial
// tiles as gemm_tn_partial_kernel, so gemm_tn_reduce_kernel / pfa_reduce_multi finish it unchanged.  Reached from pfa_gemm_tn*_f32 for
// the tiles gemm_tn_bf16_takes names; pfa_gemm_tn_path says which.
//
// Both operands are contracted over their ROWS, so both fragments are transposed reads (bf_tr8, ds_read_b64_tr_b16) of row-major bf16
// planes.  Per slab of 32 k rows:
//   global  the coalesced float4 row loads of the fp32 kernel (rows at or past k_hi load zeros), held in registers across the MFMAs of
//           the slab before;
//   split   each float4 -> bf_split2 twice -> 8 bytes into each of the three planes [k row][column] of its operand: every value is split
//           once per workgroup, never per fragment;
//   MFMA    a wave keeps the three pieces of its A fragments resident (12 registers each; the 128 x 256 tile: of two of its four at a
//           time, GemmBfCfg::MA) and walks its NI B tiles, 3 x 2 transposed reads and 6 MFMAs per resident A fragment each; per
//           accumulator the six terms arrive in the order kBfTA / kBfTB.
// LDS.  A plane row is `columns x 2 + 32` bytes (stride R = 72 / 136 / 88 / 40 dwords for 128 / 256 / 160 / 64 columns: R = 8 or 24 mod 32)
// and rows 16..31 of every plane start 128 bytes later.  A transposed read is served 32 lanes at a time over 64 banks: lane groups
// g = 0, 1 (and 2, 3) together, each 16 lanes reading 8 dwords of four consecutive rows.  Group g reads plane rows 8 pb .. 8 pb + 7 with
// pb = 2 (g & 1) + (g >> 1) — which k row a plane row holds is free as long as A and B agree — so a 32-lane pass covers rows j and
// 16 + j, j = 0..3, at banks j R and 32 + j R mod 64: eight disjoint 8-bank runs, conflict-free in tools/lds_bank_model.py ('read_tr_b64');
// with a plain stride rows j and 8 + j always collide (8 R = 0 mod 64 for every even R / 4) and no stride is better than 2-way.  The
// 8-byte plane writes go 16 lanes at a time over 32 banks: 16 lanes are 32 consecutive dwords of one row (conflict-free) except where
// a 16-lane run straddles two rows of the 160-column plane (2-way on 8 banks, one pass in five).
// Buffering.  ONE slab buffer: the 128 x 256 tile's six planes are 80 640 bytes, two workgroups fit a CU's 160 KB and one of them
// splits and stores while the other issues MFMAs: 200 us per launch at the c3 shape.  NBUF = 2 (a second slab buffer, one barrier per
// slab, one workgroup per CU) measured 270 us and LOST; it is kept as a template parameter for
// tools/experiments/gemm_tn_bf16_variants.hip only, the library instantiates NBUF = 1.
// Measured at 131 072 rows against the fp32 kernels (profiles/r08_gemm_tn_bf16_ab.json): 128 x 256 two-operand 198 us against 305,
// 128 x 160 37 against 54, 128 x 64 20 against 26, 128 x 128 (512 x 128 output) 101 against 165.  No instantiation spills (tests/test_abi.py).
#include "bf16_frag.hpp"
#include "gemm_bf16.hpp"

namespace pfa {

constexpr int kGemmBfThreads = 256;

template <int WR, int WC, int MI, int NI, int NBUF>
struct GemmBfCfg {
    static constexpr int TM = WR * MI * 16, TN = WC * NI * 16;
    static constexpr int row_bytes(int cols) { return (cols * 2) % 64 == 0 ? cols * 2 + 32 : cols * 2 + 64; }   // == 32 or 96 mod 128
    static constexpr int RSA = row_bytes(TM), RSB = row_bytes(TN);
    static constexpr int kSkew = 128;                                           // rows 16..31 of a plane: 32 banks on
    static constexpr int kPlaneA = kGemmBfBK * RSA + kSkew, kPlaneB = kGemmBfBK * RSB + kSkew;
    static constexpr int kStageBytes = 3 * (kPlaneA + kPlaneB), kBytes = NBUF * kStageBytes;
    static constexpr int kA4 = kGemmBfBK * TM / 4, kB4 = kGemmBfBK * TN / 4;    // float4 per slab
    static constexpr int kLA = (kA4 + kGemmBfThreads - 1) / kGemmBfThreads, kLB = (kB4 + kGemmBfThreads - 1) / kGemmBfThreads;
    // A fragments resident per pass over the wave's B tiles: all of them, except beside the 128 accumulators of the 128 x 256 tile, where
    // 12 MI fragment registers + the 48 of the next slab's global loads do not fit the 256 of two waves per SIMD (B is read twice instead)
    static constexpr int MA = MI * NI >= 32 ? MI / 2 : MI;
    static_assert(WR * WC * 64 == kGemmBfThreads, "4 waves");
    static_assert((RSA % 128 == 32 || RSA % 128 == 96) && (RSB % 128 == 32 || RSB % 128 == 96), "row stride = 8 or 24 dwords mod 32");
    static_assert(kBytes <= 160 * 1024, "LDS of a CU");
};

// one float4 of a slab -> 8 bytes of each plane, at (k row `row` of the slab, columns col .. col + 3)
__device__ __forceinline__ void gemm_bf_put(unsigned char *planes, int plane_bytes, int row_stride, int row, int col, const float4 &x) {
    uint2 h, m, l;
    bf_split2(x.x, x.y, h.x, m.x, l.x);
    bf_split2(x.z, x.w, h.y, m.y, l.y);
    unsigned char *q = planes + row * row_stride + (row >> 4) * 128 + col * 2;
    *reinterpret_cast<uint2 *>(q) = h;
    *reinterpret_cast<uint2 *>(q + plane_bytes) = m;
    *reinterpret_cast<uint2 *>(q + 2 * plane_bytes) = l;
}

template <int WR, int WC, int MI, int NI, int NBUF>
__global__ void __launch_bounds__(kGemmBfThreads, 3 - NBUF)
    gemm_tn_partial_bf16_kernel(const float *__restrict__ A, long long lda, const float *__restrict__ B, long long ldb, int mo, int no, long long K,
                                long long k_per_split, float *__restrict__ partial, const float *__restrict__ B2, long long ldb2, int nb) {
    using Cfg = GemmBfCfg<WR, WC, MI, NI, NBUF>;
    constexpr int MA = Cfg::MA;
    extern __shared__ __attribute__((aligned(16))) unsigned char gemm_bf_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
    const int c = lane & 15, g = lane >> 4;
    const int wr = wv / WC, wc = wv % WC;
    const int tiles_n = no / Cfg::TN;
    const int tile = blockIdx.x, split = blockIdx.y;
    const int i0 = (tile / tiles_n) * Cfg::TM, j0 = (tile % tiles_n) * Cfg::TN;
    const long long k_lo = (long long)split * k_per_split;
    const long long k_hi = k_lo + k_per_split < K ? k_lo + k_per_split : K;
    const int slabs = (int)((k_hi - k_lo + kGemmBfBK - 1) / kGemmBfBK);

    f32x4 acc[MI][NI];
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 ra[Cfg::kLA], rb[Cfg::kLB];
    // Where 256 threads are whole rows of a tile (64, 128, 256 columns) thread tid loads the same columns of rows r0 + q x (rows per
    // pass): ONE pointer per operand that moves on by a slab, instead of one address pair per load (registers: see GemmBfCfg::MA).
    constexpr int PA = Cfg::TM / 4, PB = Cfg::TN / 4;                          // float4 per row
    constexpr bool kRowsA = kGemmBfThreads % PA == 0, kRowsB = kGemmBfThreads % PB == 0;
    const int ra0 = tid / PA, rb0 = tid / PB, ca = (tid % PA) * 4, cb = (tid % PB) * 4;
    const bool second = B2 && j0 + cb >= nb;                                   // (kRowsB: this thread's columns in every pass)
    const long long ldt = second ? ldb2 : ldb;
    const float *pa = A + (k_lo + ra0) * lda + i0 + ca;
    const float *pbt = (second ? B2 + (j0 + cb - nb) : B + j0 + cb) + (k_lo + rb0) * ldt;
    auto fetch = [&](int s) {
        const long long kb = k_lo + (long long)s * kGemmBfBK;
        const int rem = (int)(k_hi - kb < kGemmBfBK ? k_hi - kb : kGemmBfBK);   // rows of this slab below k_hi
#pragma unroll
        for (int q = 0; q < Cfg::kLA; ++q) {
            if constexpr (kRowsA) {
                constexpr int rq = kGemmBfThreads / PA;
                ra[q] = ra0 + q * rq < rem ? *(const float4 *)(pa + q * rq * lda) : float4{0.f, 0.f, 0.f, 0.f};
            } else {
                const int idx = tid + q * kGemmBfThreads;
                const int row = idx / PA, col = (idx % PA) * 4;
                const bool ok = idx < Cfg::kA4 && row < rem;
                ra[q] = ok ? *(const float4 *)(A + (kb + row) * lda + i0 + col) : float4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int q = 0; q < Cfg::kLB; ++q) {
            if constexpr (kRowsB) {
                constexpr int rq = kGemmBfThreads / PB;
                rb[q] = rb0 + q * rq < rem ? *(const float4 *)(pbt + q * rq * ldt) : float4{0.f, 0.f, 0.f, 0.f};
            } else {
                const int idx = tid + q * kGemmBfThreads;
                const int row = idx / PB, col = (idx % PB) * 4;
                const bool ok = idx < Cfg::kB4 && row < rem;
                const float *src = (B2 && j0 + col >= nb) ? B2 + (kb + row) * ldb2 + (j0 + col - nb) : B + (kb + row) * ldb + j0 + col;
                rb[q] = ok ? *(const float4 *)src : float4{0.f, 0.f, 0.f, 0.f};
            }
        }
        pa += kGemmBfBK * lda;
        pbt += kGemmBfBK * ldt;
    };
    auto stash = [&](int buf) {
        unsigned char *la = gemm_bf_lds + buf * Cfg::kStageBytes, *lb = la + 3 * Cfg::kPlaneA;
#pragma unroll
        for (int q = 0; q < Cfg::kLA; ++q) {
            const int idx = tid + q * kGemmBfThreads;
            if (idx < Cfg::kA4) gemm_bf_put(la, Cfg::kPlaneA, Cfg::RSA, idx / (Cfg::TM / 4), (idx % (Cfg::TM / 4)) * 4, ra[q]);
        }
#pragma unroll
        for (int q = 0; q < Cfg::kLB; ++q) {
            const int idx = tid + q * kGemmBfThreads;
            if (idx < Cfg::kB4) gemm_bf_put(lb, Cfg::kPlaneB, Cfg::RSB, idx / (Cfg::TN / 4), (idx % (Cfg::TN / 4)) * 4, rb[q]);
        }
    };
    // this lane group's eight plane rows: 8 pb .. 8 pb + 7, the upper half of a plane behind its skew
    const int pb = 2 * (g & 1) + (g >> 1), skew = (g & 1) * Cfg::kSkew;

    if (slabs > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    for (int s = 0; s < slabs; ++s) {
        const int buf = NBUF == 2 ? s & 1 : 0;
        if (s + 1 < slabs) fetch(s + 1);   // global loads in flight across this slab's MFMAs
        const unsigned char *la = gemm_bf_lds + buf * Cfg::kStageBytes + skew, *lb = la + 3 * Cfg::kPlaneA;
#pragma unroll
        for (int ah = 0; ah < MI; ah += MA) {   // MA of the wave's A fragments resident at a time
            BfFrag3 fa[MA];
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int p = 0; p < 3; ++p) bf_tr8(la + p * Cfg::kPlaneA, Cfg::RSA, 0, (wr * MI + ah + a) * 16, c, pb, fa[a].p[p]);
#pragma unroll
            for (int b = 0; b < NI; ++b) {
                BfFrag3 fb;
#pragma unroll
                for (int p = 0; p < 3; ++p) bf_tr8(lb + p * Cfg::kPlaneB, Cfg::RSB, 0, (wc * NI + b) * 16, c, pb, fb.p[p]);
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int a = 0; a < MA; ++a) acc[ah + a][b] = bf_mfma(fa[a].p[kBfTA[t]], fb.p[kBfTB[t]], acc[ah + a][b]);
                __builtin_amdgcn_sched_barrier(0);   // keep later B tiles' fragments out of the registers
            }
        }
        if (NBUF == 1) __syncthreads();    // every wave is done reading the one buffer
        if (s + 1 < slabs) stash(NBUF == 2 ? buf ^ 1 : 0);
        __syncthreads();
    }

    float *out = partial + (size_t)split * mo * no;
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(size_t)(i0 + (wr * MI + a) * 16 + 4 * g + r) * no + j0 + (wc * NI + b) * 16 + c] = acc[a][b][r];
}

#ifndef PFA_GEMM_BF16_KERNEL_ONLY   // (tools/experiments/gemm_tn_bf16_variants.hip includes the kernel alone)
// -------------------------------------------------------------------------------------------------------------------------- host
// Routed by measurement (profiles/r08_gemm_tn_bf16_ab.json, docs/lab-notebook.md): the two-operand 128 x 256 tile and the matrix-bound
// 128-row tiles of the single-operand form.  16 x 128, 128 x 32 and 128 x 16 are HBM- or latency-bound and keep fp32.
bool gemm_tn_bf16_takes(int cfg) { return pfa_igemm_get_products() == 1 && (cfg == 6 || cfg == 0 || cfg == 1 || cfg == 5); }

template <int WR, int WC, int MI, int NI>
static int gemm_bf16_launch_cfg(hipStream_t stream, dim3 grid, const float *a, long long lda, const float *b, long long ldb, int mo, int no, long long k,
                                long long per, float *partial, const float *b2, long long ldb2, int nb) {
    using Cfg = GemmBfCfg<WR, WC, MI, NI, 1>;
    static bool attr = false;
    if (!attr) {
        PFA_CHECK_HIP(hipFuncSetAttribute((const void *)gemm_tn_partial_bf16_kernel<WR, WC, MI, NI, 1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          Cfg::kBytes));
        attr = true;
    }
    hipLaunchKernelGGL((gemm_tn_partial_bf16_kernel<WR, WC, MI, NI, 1>), grid, dim3(kGemmBfThreads), Cfg::kBytes, stream, a, lda, b, ldb, mo, no, k, per,
                       partial, b2, ldb2, nb);
    return 0;
}

int gemm_tn_bf16_launch(int cfg, hipStream_t stream, unsigned tiles, unsigned splits, const float *a, long long lda, const float *b, long long ldb,
                        int mo, int no, long long k, long long k_per_split, float *partial, const float *b2, long long ldb2, int nb) {
    PFA_REQUIRE(k_per_split % kGemmBfBK == 0, "gemm_tn (bf16x6): the split size must be a multiple of the slab");
    const dim3 grid(tiles, splits);
    int rc = 0;
    if (cfg == 6)
        rc = gemm_bf16_launch_cfg<2, 2, 4, 8>(stream, grid, a, lda, b, ldb, mo, no, k, k_per_split, partial, b2, ldb2, nb);
    else if (cfg == 0)
        rc = gemm_bf16_launch_cfg<2, 2, 4, 4>(stream, grid, a, lda, b, ldb, mo, no, k, k_per_split, partial, b2, ldb2, nb);
    else if (cfg == 1)
        rc = gemm_bf16_launch_cfg<2, 2, 4, 2>(stream, grid, a, lda, b, ldb, mo, no, k, k_per_split, partial, b2, ldb2, nb);
    else if (cfg == 5)
        rc = gemm_bf16_launch_cfg<4, 1, 2, 10>(stream, grid, a, lda, b, ldb, mo, no, k, k_per_split, partial, b2, ldb2, nb);
    else
        PFA_REQUIRE(false, "gemm_tn (bf16x6): tile configuration %d is not routed", cfg);
    if (rc) return rc;
    PFA_LAUNCH_CHECK();
    return 0;
}
#endif

}  // namespace pfa
