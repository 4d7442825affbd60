// lstm_seq_bf16.hpp — the streaming six-term product of csrc/lstm_seq_bf16.hip (the recurrent training kernels in the opt-in bf16x6
// product form): the weight stream's register ring, the bf16 planes' reads and writes, and the product loop itself.  A header of its
// own so that the backward kernel of the same form, measured slower than the fp32 one and therefore kept out of the build
// (tools/experiments/lstm_seq_bwd_bf16.hip), compiles against the same text.
#pragma once
#include "bf16_frag.hpp"
#include "lstm_seq.hpp"
#include "lstm_tile.hpp"

namespace pfa {

constexpr int kSeqBfRing = 4;             // groups of the weight stream in registers
constexpr int kSeqBfTiles = 64;           // A tiles per wave in either pack: 8 slabs x 8 ct (forward), 16 slabs x 4 kt (backward)
constexpr int kSeqBfPackFrags = 4 * kSeqBfTiles * 3;    // 1 KB fragments per pack
constexpr int kXRowB = 2 * kLK + 16;      // bytes per row of an [xe | h] plane (+16: rows 4 banks apart)
constexpr int kXPlaneB = kSeqRows * kXRowB;
constexpr int kGRowB = 2 * kLG + 16;      // ... of a dG plane
constexpr int kGPlaneB = kSeqRows * kGRowB;

// four consecutive k of one row -> their 8 bytes in each of the three planes
__device__ __forceinline__ void bf_put4(unsigned char *p, int plane_bytes, float v0, float v1, float v2, float v3) {
    uint32_t h0, m0, l0, h1, m1, l1;
    bf_split2(v0, v1, h0, m0, l0);
    bf_split2(v2, v3, h1, m1, l1);
    *reinterpret_cast<uint2 *>(p) = make_uint2(h0, h1);
    *reinterpret_cast<uint2 *>(p + plane_bytes) = make_uint2(m0, m1);
    *reinterpret_cast<uint2 *>(p + 2 * plane_bytes) = make_uint2(l0, l1);
}

__device__ __forceinline__ BfFrag bf_frag_ld(const unsigned char *p) {
    BfFrag f;
    f.v = *reinterpret_cast<const bf16x8 *>(p);
    return f;
}
__device__ __forceinline__ BfFrag bf_stream_ld(const Stream &st, int frag) { return bf_frag_ld(reinterpret_cast<const unsigned char *>(st.base) + (size_t)frag * 1024 + st.loff); }

__device__ __forceinline__ void bf_ring_prefetch(const Stream &ws, BfFrag (&ring)[kSeqBfRing][6]) {
#pragma unroll
    for (int j = 0; j < kSeqBfRing - 1; ++j)
#pragma unroll
        for (int a = 0; a < 6; ++a) ring[j][a] = bf_stream_ld(ws, j * 6 + a);
}

// acc[rt][n] += sum over S slabs of A(s, n) . B(rt, s) in the six-term form, n = 0 .. NT-1 the wave's A tiles.
//   A: the wave's stream, group gq = s * NT/2 + pair holds tiles 2 pair, 2 pair + 1 as fragments gq*6 + 3*(n & 1) + piece;
//   B: plane `piece` of row tile rt at brow + piece * plane_bytes + rt * 16 rows, 64 bytes per slab (brow includes the lane's row and 16 g).
// Same shape as stream_product (lstm_tile.hpp): the ring runs kSeqBfRing - 1 groups ahead, `side(gq)` runs once per group right after
// that group's loads are issued, one scheduling barrier per group.
template <int S, int NT, int ROWB, int PLANEB, class Side>
__device__ __forceinline__ void bf_stream_product(const Stream &ws, const unsigned char *brow, BfFrag (&ring)[kSeqBfRing][6],
                                                  f32x4 (&acc)[kSeqRT][NT], Side &&side) {
    constexpr int D = kSeqBfRing, GPS = NT / 2, G = S * GPS;
    BfFrag bc[kSeqRT][3], bn[kSeqRT][3];
#pragma unroll
    for (int rt = 0; rt < kSeqRT; ++rt)
#pragma unroll
        for (int p = 0; p < 3; ++p) bc[rt][p] = bf_frag_ld(brow + p * PLANEB + rt * 16 * ROWB);
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
        const int s = gq / GPS, pair = gq % GPS;
        if (gq + D - 1 < G) {
#pragma unroll
            for (int a = 0; a < 6; ++a) ring[(gq + D - 1) & (D - 1)][a] = bf_stream_ld(ws, (gq + D - 1) * 6 + a);
        }
        side(gq);
        if (pair == 0 && s + 1 < S) {
#pragma unroll
            for (int rt = 0; rt < kSeqRT; ++rt)
#pragma unroll
                for (int p = 0; p < 3; ++p) bn[rt][p] = bf_frag_ld(brow + p * PLANEB + rt * 16 * ROWB + 64 * (s + 1));
        }
        // term outermost: the six products of one accumulator keep their order, three other MFMAs between two of them
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int rt = 0; rt < kSeqRT; ++rt)
                    acc[rt][2 * pair + n] = bf_mfma(ring[gq & (D - 1)][3 * n + kBfTA[t]], bc[rt][kBfTB[t]], acc[rt][2 * pair + n]);
        if (pair == GPS - 1) {
#pragma unroll
            for (int rt = 0; rt < kSeqRT; ++rt)
#pragma unroll
                for (int p = 0; p < 3; ++p) bc[rt][p] = bn[rt][p];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace pfa
