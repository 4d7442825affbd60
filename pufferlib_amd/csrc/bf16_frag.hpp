// bf16_frag.hpp — the operand pieces of the bf16x6 product form, shared by the fused gradient kernels that use it (ppo_bf16.hpp at hidden
// 128, ppo_wide_bf16.hip at hidden 256): the split of an fp32 value into three bf16 pieces (x = hi + mid + lo, round to nearest each
// time), one operand fragment of v_mfma_f32_16x16x32_bf16, the order of the six partial products, and the transposed LDS read.
#pragma once
#include "common.hpp"
#include "mlp_tile.hpp"

namespace pfa {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t bf_pk(float a, float b) {   // two floats -> two bf16 (round to nearest even), a in the low half
    f32x2_t v = {a, b};
    bf16x2_t r = __builtin_convertvector(v, bf16x2_t);
    return *reinterpret_cast<uint32_t *>(&r);
}
__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xFFFF0000u); }

// x = hi + mid + lo for a pair of values: one packed word per piece
__device__ __forceinline__ void bf_split2(float a, float b, uint32_t &h, uint32_t &m, uint32_t &l) {
    h = bf_pk(a, b);
    const float ra = a - bf_lo(h), rb = b - bf_hi(h);
    m = bf_pk(ra, rb);
    l = bf_pk(ra - bf_lo(m), rb - bf_hi(m));
}
union BfFrag {   // eight bf16 = one operand fragment of v_mfma_f32_16x16x32_bf16: element e sits in word e / 2, half e % 2
    uint32_t w[4];
    bf16x8 v;
    s16x4_t h[2];
};
struct BfFrag3 {
    BfFrag p[3];   // hi, mid, lo
};
__device__ __forceinline__ void bf_split8(const float *x, BfFrag3 &out) {
#pragma unroll
    for (int q = 0; q < 4; ++q) bf_split2(x[2 * q], x[2 * q + 1], out.p[0].w[q], out.p[1].w[q], out.p[2].w[q]);
}
// acc += A . B as the six partial products, small terms first
__device__ __forceinline__ f32x4 bf_mfma(const BfFrag &a, const BfFrag &b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0); }
constexpr int kBfTA[6] = {2, 0, 1, 1, 0, 0}, kBfTB[6] = {0, 2, 1, 0, 1, 0};

// One operand fragment whose contraction index is the ROW of a row-major bf16 plane: element e <-> (row row0 + 8 g + e, column
// col0 + c).  ds_read_b64_tr_b16: within a group of 16 lanes, lane 4 a + b receives element b of the 8 bytes lanes a, a + 4, a + 8,
// a + 12 point at — so lane j of the group points at (row (j >> 2), columns 4 (j & 3) .. + 3) of a 4 x 16 block; two reads = 8 rows.
typedef __attribute__((address_space(3))) s16x4_t *bf_lds_s16x4;
__device__ __forceinline__ void bf_tr8(const unsigned char *plane, int row_stride, int row0, int col0, int c, int g, BfFrag &f) {
    const unsigned char *p = plane + (row0 + 8 * g + (c >> 2)) * row_stride + (col0 + 4 * (c & 3)) * 2;
    f.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf_lds_s16x4)p);
    f.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf_lds_s16x4)(p + 4 * row_stride));
}

}  // namespace pfa
