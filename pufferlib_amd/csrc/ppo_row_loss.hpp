// ppo_row_loss.hpp — THE per-row PPO loss of the multi-kernel update path (clean_pufferl.py:202-238), written once for the four heads
// kernels that run it: lstm_heads_loss (lstm.hip), cnn_heads_loss (cnn_heads.hip), heads_rows_loss and heads_wide_loss (general.hip).
// Each of them keeps only what is its own — where a row's logits come from, its softmax layout, its dh product, its block reduction —
// and hands the row's scalars to:
//   adv_norm         the advantage normalisation of a minibatch (clean_pufferl.py:211-213)
//   ppo_policy_loss  the clipped policy loss with torch.max's tie rule and clamp's pass-through: d loss / d new_logprob
//   ppo_value_loss   the (clipped) value loss with its own tie rule: d loss / d new_value
//   accumulate       the six loss statistics of the row into a kernel's running sums
//   logit_grad       d loss / d logit from d loss / d log-prob and the entropy coefficient
// Policy and value are two functions, called in this order, and not one: the compiler optimises an inlined function on its own before
// it inlines it, and as one function the products of d loss / d new_logprob end up behind the value branch, from where they sink into
// the callers' per-logit code and change which of its products contract into an fma (docs/lab-notebook.md).
// The fused kernels (ppo_update.hip, ppo_wide.hip, ppo_bf16.hpp) run ppo_tile.hpp's ppo_loss_tile: the same formula on the hardware
// exp and a reciprocal of the std, with its own text (docs/next-steps.md).  This header is the reference form of both.
#pragma once
#include <cmath>

#include "common.hpp"

namespace pfa {

struct AdvNorm {   // with hp.norm_adv: adv = (adv_raw - mean) / den
    float mean, den;
};

// adv_stats[2 mb], [2 mb + 1]: sum adv, sum adv^2 over the GLOBAL minibatch of global_rows rows (unbiased std, f64); {0, 1} without norm_adv
__device__ __forceinline__ AdvNorm adv_norm(const pfa_ppo_hparams &hp, const double *adv_stats, int mb, double global_rows) {
    AdvNorm n{0.0f, 1.0f};
    if (hp.norm_adv) {
        const double s1 = adv_stats[2 * mb], s2 = adv_stats[2 * mb + 1];
        const double mean = s1 / global_rows;
        double var = (s2 - s1 * mean) / (global_rows - 1.0);
        var = var > 0.0 ? var : 0.0;
        n.mean = (float)mean;
        n.den = (float)sqrt(var) + 1e-8f;
    }
    return n;
}

// `scale` in both: 1 / rows of the global minibatch (0 for a padding row)
struct PolicyLoss {
    float g_lp;    // d loss / d new_logprob (carries `scale`)
    float pg1, pg2, logratio, ratio;
};
struct ValueLoss {
    float dv;      // d loss / d new_value (carries the value coefficient and `scale`)
    float v_loss;
};

// `adv`: the normalised advantage
__device__ __forceinline__ PolicyLoss ppo_policy_loss(float new_logprob, float old_logprob, float adv, const pfa_ppo_hparams &hp, float scale) {
    PolicyLoss r;
    const float logratio = new_logprob - old_logprob;
    const float ratio = expf(logratio);
    const float lo_c = 1.0f - hp.clip_coef, hi_c = 1.0f + hp.clip_coef;
    const float pg1 = -adv * ratio, pg2 = -adv * fminf(fmaxf(ratio, lo_c), hi_c);
    const bool inside = ratio >= lo_c && ratio <= hi_c;
    float dpg;   // d max(pg1, pg2) / d ratio: torch.max sends half the gradient to each side of a tie, clamp passes it on inside only
    if (pg1 > pg2) dpg = -adv;
    else if (pg1 < pg2) dpg = inside ? -adv : 0.0f;
    else dpg = inside ? -adv : -0.5f * adv;
    r.g_lp = dpg * ratio * scale;
    r.pg1 = pg1, r.pg2 = pg2, r.logratio = logratio, r.ratio = ratio;
    return r;
}

__device__ __forceinline__ ValueLoss ppo_value_loss(float new_value, float old_value, float ret, const pfa_ppo_hparams &hp, float scale) {
    float v_loss, dv;
    if (hp.clip_vloss) {
        const float du = new_value - ret, vl_u = du * du;
        const float delta = new_value - old_value;
        const float vcl = old_value + fminf(fmaxf(delta, -hp.vf_clip_coef), hp.vf_clip_coef);
        const float dc = vcl - ret, vl_c = dc * dc;
        const bool vin = delta >= -hp.vf_clip_coef && delta <= hp.vf_clip_coef;
        v_loss = 0.5f * fmaxf(vl_u, vl_c);
        const float gu = 2.0f * du, gc = vin ? 2.0f * dc : 0.0f;
        dv = 0.5f * (vl_u > vl_c ? gu : (vl_u < vl_c ? gc : 0.5f * (gu + gc)));   // torch.max again: a tie halves both sides
    } else {
        const float du = new_value - ret;
        v_loss = 0.5f * du * du;
        dv = du;
    }
    return ValueLoss{dv * (hp.vf_coef * scale), v_loss};
}

// The row's six statistics: policy loss, value loss, entropy, old_approx_kl, approx_kl, clipfrac.  Formed where they are asked for
// (the 16-lane kernels ask on one lane of a row), not with the gradients.
__device__ __forceinline__ void row_stats(float (&s)[6], const PolicyLoss &pl, const ValueLoss &vl, float ent, const pfa_ppo_hparams &hp) {
    s[0] = fmaxf(pl.pg1, pl.pg2);
    s[1] = vl.v_loss;
    s[2] = ent;
    s[3] = -pl.logratio;
    s[4] = (pl.ratio - 1.0f) - pl.logratio;
    s[5] = fabsf(pl.ratio - 1.0f) > hp.clip_coef ? 1.0f : 0.0f;
}
// acc[i] += statistic i times w (1 for a row, 0 for a padding row): the product in float, the sum in the accumulator's type
template <class T>
__device__ __forceinline__ void accumulate(T (&acc)[6], const PolicyLoss &pl, const ValueLoss &vl, float ent, const pfa_ppo_hparams &hp, float w) {
    float s[6];
    row_stats(s, pl, vl, ent, hp);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] += (T)(s[i] * w);
}

// d / d logit of  g_lp * log-prob - c_ent * entropy  for a logit of softmax probability p and normalised value nl in a head of
// entropy head_entropy: d log-prob / d logit = [chosen] - p, d entropy / d logit = -p (nl + H).  The loss carries -ent_coef * entropy:
// its kernels pass c_ent = ent_coef * scale.  (The *_eval_backward kernels of policy(obs, action=...) are this with c_ent = -g_entropy;
// they keep the line as a subtraction, the instruction they always had.)
__device__ __forceinline__ float logit_grad(float g_lp, float c_ent, bool chosen, float p, float nl, float head_entropy) {
    return g_lp * ((chosen ? 1.0f : 0.0f) - p) + c_ent * p * (nl + head_entropy);
}

}  // namespace pfa
