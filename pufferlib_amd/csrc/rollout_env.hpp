// rollout_env.hpp — the fused persistent rollout of the MLP policy (clean_pufferl.py:76-154 evaluate) as one skeleton over an env
// adapter (env_adapters.hpp: load / step / refresh / store), and the host side its entry points share.  The tuned Squared kernel
// (rollout_mlp_squared_kernel, rollout.hip) is the deliberate exception: it stores after the env step and prefetches its tape.
#pragma once
#include "env_adapters.hpp"
#include "rollout_tile.hpp"

namespace pfa {

// 16 envs per 4-wave workgroup for all T steps, env state in registers of the owner lanes, the 16 observation rows in LDS as the MFMA
// B operand, weights in registers.  KS as the standalone forward chooses it for the policy's shape (dispatch_stride), so that the
// protocol path and this kernel run the same products.  Params = where the weights live: the flat 128-wide buffer (MW = kMW), or an
// MlpView of any of the four widths (hidden = 64 MW) — the fragments are loaded once, the rest of the kernel does not see the form.
template <class Env, int DP, int KS, int MW = kMW, class Params = const float *>
__global__ void __launch_bounds__(kRollThreads) rollout_mlp_env_kernel(typename Env::View v, Params params, int a, pfa_experience ex,
                                                                      const float *noise, uint64_t seed, uint64_t step0,
                                                                      long long env_offset, float *live_obs, float *live_rew,
                                                                      uint8_t *live_term, uint8_t *live_trunc, uint8_t *live_mask) {
    constexpr int XS = XTile<DP>::XS;
    __shared__ float xs[XTile<DP>::kFloats];
    __shared__ float part[kRollWaves][kPartFloats];
    __shared__ typename Env::Shared sh;
    const int le = threadIdx.x >> 4, lo = threadIdx.x & 15;
    const int e = blockIdx.x * 16 + le;
    const bool env_ok = e < v.n;
    const bool owner = lo == 0 && env_ok;
    const int T = ex.horizon_T;

    SliceFrags<DP, KS, MW> w;
    if constexpr (std::is_pointer_v<Params>) {
        w.load(params, a);
    } else {
        w.load(params);
    }
    stage_rows<DP>(live_obs, (long long)blockIdx.x * 16, v.n, xs, 16);
    Env env;
    float reward = 0.0f;
    bool terminal = false;
    if (owner) {
        env.load(v, e, le, sh);
        reward = live_rew[e];
        terminal = live_term[e] != 0;
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        unstage_rows<DP>(xs, ex.obs + (size_t)t * DP, (long long)blockIdx.x * 16, v.n, (size_t)T * DP, 16);
        forward_slice<DP, KS, MW>(w, xs, part);
        __syncthreads();
        const float q = env_ok ? noise_lane(noise ? noise + ((size_t)t * v.n + e) * a : nullptr, seed, step0 + t,
                                            (uint64_t)(env_offset + e), lo, a)
                               : 1.0f;
        const LaneSample sm = sample_lanes(part, le, lo, a, q);
        if (owner) {
            const size_t row = (size_t)e * T + t;
            ex.rewards[row] = reward;
            ex.dones[row] = terminal ? 1.0f : 0.0f;
            ex.actions[row] = sm.action;
            ex.logprobs[row] = sm.logprob;
            ex.values[row] = sm.value;
            env.step(v, e, le, sh, xs + le * XS, sm.action, reward, terminal);
        }
        __syncthreads();
        if constexpr (Env::kRefresh) {
            if (env_ok) env.refresh(v, e, le, lo, sh, xs + le * XS);
            __syncthreads();
        }
    }
    if (owner) {
        env.store(v, e, le, sh);
        store_live(e, reward, terminal ? 1 : 0, live_rew, live_term, live_trunc, live_mask);
    }
    unstage_rows<DP>(xs, live_obs, (long long)blockIdx.x * 16, v.n, (size_t)DP, 16);
}

// What the entry points of the skeleton share: `name` is the entry point's kernel-timer name and the prefix of its error texts; the
// entry point has checked its env, `dims` against it, and built the view.  kOnlyDP != 0: the one row width the env has.
template <class Env, int kOnlyDP = 0>
static int launch_rollout_mlp(const char *name, void *state, const typename Env::View &v, const float *params, const pfa_mlp_dims *dims,
                              const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs,
                              float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_rollout_args(name, state && params && exp && obs && rewards && terminals && truncations && masks, dims->heads, exp,
                                    noise, key))
        return rc;
    PFA_REQUIRE(dims->hidden == kHidden, "%s: hidden must be %d (got %d)", name, kHidden, dims->hidden);
    const uint64_t seed = key ? key->seed : 0, step = key ? key->step : 0;
    ScopedKernelTimer timer(name, (hipStream_t)stream);
    auto launch = [&](auto tile) {
        using T = decltype(tile);
        hipLaunchKernelGGL((rollout_mlp_env_kernel<Env, T::DP, T::KS>), dim3((unsigned)((v.n + 15) / 16)), dim3(kRollThreads), 0,
                           (hipStream_t)stream, v, params, dims->num_actions, *exp, noise, seed, step, (long long)env_offset, obs, rewards,
                           terminals, truncations, masks);
    };
    if constexpr (kOnlyDP != 0) {
        launch(Tile<kOnlyDP, kOnlyDP / 4, kMW>{});
    } else {
        dispatch_stride<kMW>(dims->obs_stride, dims->obs_dim, launch);
    }
    PFA_LAUNCH_CHECK();
    return 0;
}

// The view form of the same: a policy of any tile width (TilePolicy, rollout_tile.hpp: policy_of_view, or policy_of_flat for the flat
// 128-wide buffer), launched through dispatch_tile — the hidden -> MW map of the standalone forward, so that the protocol path and
// this kernel take the same Tile.  The entry point has checked its env and `p` against it.  kOnlyDP as above.
template <class Env, int kOnlyDP = 0>
static int launch_rollout_mlp_view(const char *name, void *state, const typename Env::View &v, const TilePolicy &p, const pfa_experience *exp,
                                   const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                   uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_rollout_args(name, state && exp && obs && rewards && terminals && truncations && masks, p.heads, exp, noise, key)) return rc;
    const uint64_t seed = key ? key->seed : 0, step = key ? key->step : 0;
    ScopedKernelTimer timer(name, (hipStream_t)stream);
    dispatch_tile<kOnlyDP>(p, [&](auto tile) {
        using T = decltype(tile);
        hipLaunchKernelGGL((rollout_mlp_env_kernel<Env, T::DP, T::KS, T::MW, MlpView>), dim3((unsigned)((v.n + 15) / 16)), dim3(kRollThreads), 0,
                           (hipStream_t)stream, v, p.pv, p.pv.a, *exp, noise, seed, step, (long long)env_offset, obs, rewards, terminals,
                           truncations, masks);
    });
    PFA_LAUNCH_CHECK();
    return 0;
}

}  // namespace pfa
