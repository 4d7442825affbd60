// ppo_wide.hpp — what the two forms of the width-general fused PPO gradient step share: the layout of the partial a workgroup leaves
// (read by ppo_wide_reduce_kernel, ppo_wide.hip) and the host entry of the opt-in bf16x6 form (ppo_wide_bf16.hip), which
// pfa_ppo_wide_grad dispatches to.
#pragma once
#include "common.hpp"
#include "mlp_tile.hpp"
#include "ppo_tile.hpp"
#include "rollout_tile.hpp"

namespace pfa {

// One workgroup partial (floats), fragment order.  MT = H / 16 hidden tiles, KTM 16-column tiles of dW1 on MFMA (+ COL: the
// one trailing column 16 KTM, for rows of 16 KTM + 1 real columns like the 7x7 grid's 49).
struct WideLayout {
    int MT, KTM, col;
    int kCol, kDw2, kDb1, kDb2, kStats, kCount;
};
__host__ __device__ inline WideLayout wide_layout(int hidden, int ktm, bool col) {
    WideLayout l;
    l.MT = hidden / 16;
    l.KTM = ktm;
    l.col = col ? 1 : 0;
    l.kCol = ktm * l.MT * 256;                 // ((kt*MT + m)*4 + r)*64 + lane -> W1[16m + c][16kt + 4g + r]
    l.kDw2 = l.kCol + (col ? hidden : 0);      // u = 16m + c -> W1[u][16 KTM]
    l.kDb1 = l.kDw2 + l.MT * 256;              // (m*4 + r)*64 + lane -> W2v[o = c][16m + 4g + r]
    l.kDb2 = l.kDb1 + hidden;
    l.kStats = l.kDb2 + kOut;
    l.kCount = l.kStats + kNumStats;
    return l;
}

// The bf16x6 form (ppo_wide_bf16.hip): hidden 256 on rows of 32 / 64 floats, minibatches of whole 32-row tiles.
constexpr int kWideBfMaxGrid = 256;   // one workgroup per CU: never more partials than wide_slots sizes the workspace for
bool wide_bf16_takes(int hidden, int obs_stride, int64_t mb_rows);
int wide_bf16_grid(int64_t mb_rows);
// Launches ppo_wide_grad_bf16_kernel on `grid` workgroups; the partials have wide_layout(hidden, ktm, col) like the fp32 form's.
int wide_bf16_launch(int grid, hipStream_t stream, const pfa_experience &ex, RowMap map, long long mb_rows, const MlpView &pv, int obs_stride,
                     bool col, const pfa_ppo_hparams &hp, const double *adv_stats, double global_rows, float *partials);

}  // namespace pfa
