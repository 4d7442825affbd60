// gemm_bf16.hpp — what csrc/gemm.hip needs of csrc/gemm_bf16.hip: the weight-gradient contractions C = A^T B in the opt-in bf16x6 product
// form.  gemm_tn_bf16_takes: does the tile configuration `cfg` of GemmTnPlan (6 = the two-operand 128 x 256 tile) run in the form under
// the products switch as it stands now — host state only, what pfa_gemm_tn_path reports.  gemm_tn_bf16_launch: the partial products of
// such a tile, same arguments, grid and workspace layout as gemm_tn_partial_kernel; k_per_split must be a multiple of kGemmBfBK.
#pragma once
#include "common.hpp"

namespace pfa {

constexpr int kGemmBfBK = 32;   // k rows per slab: one K step of v_mfma_f32_16x16x32_bf16

bool gemm_tn_bf16_takes(int cfg);
int gemm_tn_bf16_launch(int cfg, hipStream_t stream, unsigned tiles, unsigned splits, const float *a, long long lda, const float *b, long long ldb,
                        int mo, int no, long long k, long long k_per_split, float *partial, const float *b2, long long ldb2, int nb);

}  // namespace pfa
