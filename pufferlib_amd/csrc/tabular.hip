// tabular.hip — protocol kernels of the Tabular vecenv (tabular_env.hpp: a user-given finite MDP / POMDP as device tables) and its
// fused persistent rollout with the MLP policy.  The fused recurrent rollout over it lives in lstm_fused.hip.
#include "common.hpp"
#include "env_adapters.hpp"
#include "rollout_tile.hpp"
#include "tabular_env.hpp"

namespace pfa {

__global__ void __launch_bounds__(256) tabular_reset_kernel(TabularView v, float *obs, float *rewards, uint8_t *terminals,
                                                           uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    TabularEnv s = {};
    s.episode = -1;
    float r;
    bool t;
    tabular_begin_episode(v, e, s, r, t);
    v.env[e] = s;
    v.fin[e] = EpisodeFin{};
    for (int chunk = 0; 16 * chunk < v.stride; ++chunk) tabular_copy_chunk(v, s.state, chunk, obs + (size_t)e * v.stride);
    rewards[e] = 0.0f;
    terminals[e] = 0;
    truncations[e] = 0;
    masks[e] = 1;
}

__global__ void __launch_bounds__(256) tabular_debug_states_kernel(TabularView v, int32_t *out5) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const TabularEnv s = v.env[e];
    int32_t *o = out5 + (size_t)e * 5;
    o[0] = s.state, o[1] = s.episode, o[2] = s.tick, o[3] = s.done, o[4] = s.ep_length;
}

// Fused persistent rollout, structure of rollout_mlp_stochastic_kernel (stochastic.hip) with the adapter's refresh step and its
// barrier: 16 envs per 4-wave workgroup, env state in registers of the owner lanes, the 16 observation rows in LDS as the MFMA B
// operand, weights in registers.  KS as the standalone forward chooses it for the policy's shape (rollout.hip: dispatch_stride), so
// that the protocol path and this kernel run the same products.
template <int DP, int KS>
__global__ void __launch_bounds__(kRollThreads) rollout_mlp_tabular_kernel(TabularView v, const float *params, int a, pfa_experience ex,
                                                                          const float *noise, uint64_t seed, uint64_t step0,
                                                                          long long env_offset, float *live_obs, float *live_rew,
                                                                          uint8_t *live_term, uint8_t *live_trunc, uint8_t *live_mask) {
    constexpr int XS = XTile<DP>::XS;
    __shared__ float xs[XTile<DP>::kFloats];
    __shared__ float part[kRollWaves][kPartFloats];
    __shared__ TabularRollEnv::Shared sh;
    const int le = threadIdx.x >> 4, lo = threadIdx.x & 15;
    const int e = blockIdx.x * 16 + le;
    const bool env_ok = e < v.n;
    const bool owner = lo == 0 && env_ok;
    const int T = ex.horizon_T;

    SliceFrags<DP, KS> w;
    w.load(params, a);
    stage_rows<DP>(live_obs, (long long)blockIdx.x * 16, v.n, xs, 16);
    TabularRollEnv env;
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
        forward_slice<DP, KS>(w, xs, part);
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
        if (env_ok) env.refresh(v, e, le, lo, sh, xs + le * XS);
        __syncthreads();
    }
    if (owner) {
        env.store(v, e, le, sh);
        live_rew[e] = reward;
        live_term[e] = terminal ? 1 : 0;
        live_trunc[e] = 0;
        live_mask[e] = 1;
    }
    unstage_rows<DP>(xs, live_obs, (long long)blockIdx.x * 16, v.n, (size_t)DP, 16);
}

int check_tabular_config(const pfa_tabular_config *c) {
    PFA_REQUIRE(c != nullptr, "tabular: null config");
    PFA_REQUIRE(c->num_envs >= 1, "tabular: num_envs must be >= 1");
    PFA_REQUIRE(c->num_states >= 1 && c->num_states <= kTabMaxStates, "tabular: num_states must be in 1..%d (got %d)", kTabMaxStates,
                c->num_states);
    PFA_REQUIRE(c->num_actions >= 1 && c->num_actions <= kTabMaxActions, "tabular: num_actions must be in 1..%d (got %d)", kTabMaxActions,
                c->num_actions);
    PFA_REQUIRE(c->num_outcomes >= 1 && c->num_outcomes <= kTabMaxOutcomes, "tabular: num_outcomes must be in 1..%d (got %d)",
                kTabMaxOutcomes, c->num_outcomes);
    PFA_REQUIRE(c->num_starts >= 1 && c->num_starts <= c->num_states, "tabular: num_starts must be in 1..num_states (got %d)", c->num_starts);
    PFA_REQUIRE(c->obs_dim >= 1 && c->obs_dim <= kTabMaxObs, "tabular: obs_dim must be in 1..%d (got %d)", kTabMaxObs, c->obs_dim);
    PFA_REQUIRE(c->obs_stride >= c->obs_dim && (c->obs_stride == 16 || c->obs_stride == 32 || c->obs_stride == 64 || c->obs_stride == 96 ||
                                                c->obs_stride == 128 || c->obs_stride == 160),
                "tabular: obs_stride must be one of 16/32/64/96/128/160 and >= obs_dim %d (got %d)", c->obs_dim, c->obs_stride);
    PFA_REQUIRE(c->horizon >= 1, "tabular: horizon must be >= 1 (got %d)", c->horizon);
    PFA_REQUIRE(c->next && c->cum && c->reward && c->terminal && c->obs && c->start_states && c->start_cum, "tabular: null table");
    PFA_REQUIRE((uintptr_t)c->obs % 16 == 0, "tabular: the observation table must be 16-byte aligned");
    return 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_tabular_state_bytes(const pfa_tabular_config *cfg) {
    return check_tabular_config(cfg) ? 0 : tabular_state_bytes(cfg->num_envs);
}

extern "C" int pfa_tabular_async_reset(void *state, const pfa_tabular_config *cfg, float *obs, float *rewards, uint8_t *terminals,
                                       uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_tabular_config(cfg)) return rc;
    PFA_REQUIRE(state && obs && rewards && terminals && truncations && masks, "tabular.async_reset: null buffer");
    hipLaunchKernelGGL(tabular_reset_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       tabular_view(state, *cfg), obs, rewards, terminals, truncations, masks);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_tabular_send(void *state, const pfa_tabular_config *cfg, const int64_t *actions, float *obs, float *rewards,
                                uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_tabular_config(cfg)) return rc;
    return launch_env_send<TabularRollEnv>("tabular.send", state, tabular_view(state, *cfg), cfg->obs_stride, actions, obs, rewards,
                                           terminals, truncations, masks, stream);
}

extern "C" int pfa_tabular_episode_stats(void *state, const pfa_tabular_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    if (int rc = check_tabular_config(cfg)) return rc;
    return launch_episode_stats("tabular", state, tabular_view(state, *cfg).fin, cfg->num_envs, out4, reset, nullptr, stream);
}

extern "C" int pfa_tabular_last_infos(void *state, const pfa_tabular_config *cfg, uint8_t *finished, double *episode_return,
                                      int32_t *episode_length, double *score, pfa_stream_t stream) {
    if (int rc = check_tabular_config(cfg)) return rc;
    return launch_episode_infos("tabular", state, tabular_view(state, *cfg).fin, cfg->num_envs, finished, episode_return, episode_length,
                                score, stream);
}

extern "C" int pfa_tabular_debug_states(void *state, const pfa_tabular_config *cfg, int32_t *out5, pfa_stream_t stream) {
    if (int rc = check_tabular_config(cfg)) return rc;
    PFA_REQUIRE(state && out5, "tabular.debug_states: null buffer");
    hipLaunchKernelGGL(tabular_debug_states_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       tabular_view(state, *cfg), out5);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_rollout_mlp_tabular(void *state, const pfa_tabular_config *cfg, const float *params, const pfa_mlp_dims *dims,
                                       const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset,
                                       float *obs, float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks,
                                       pfa_stream_t stream) {
    if (int rc = check_tabular_config(cfg)) return rc;
    PFA_REQUIRE(state && params && dims && exp && obs && rewards && terminals && truncations && masks, "rollout_mlp_tabular: null buffer");
    PFA_REQUIRE(dims->heads == 0, "rollout_mlp_tabular: the fused rollout samples one Discrete head");
    PFA_REQUIRE(dims->hidden == kHidden, "rollout_mlp_tabular: hidden must be %d (got %d)", kHidden, dims->hidden);
    PFA_REQUIRE(dims->obs_stride == cfg->obs_stride && dims->obs_dim == cfg->obs_dim && cfg->obs_stride <= 128,
                "rollout_mlp_tabular: the policy must take %d observation values in rows of %d floats (16/32/64/96/128), got %d in rows of %d",
                cfg->obs_dim, cfg->obs_stride, dims->obs_dim, dims->obs_stride);
    PFA_REQUIRE(dims->num_actions == cfg->num_actions && dims->num_actions >= 2 && dims->num_actions <= 15,
                "rollout_mlp_tabular: the policy must have one Discrete(%d) head of 2..15 actions (got %d)", cfg->num_actions, dims->num_actions);
    PFA_REQUIRE(exp->horizon_T >= 1 && exp->obs && exp->actions && exp->logprobs && exp->values && exp->rewards && exp->dones,
                "rollout_mlp_tabular: null experience buffer");
    PFA_REQUIRE(noise || key, "rollout_mlp_tabular: need an explicit noise tensor or a Philox key");
    const uint64_t seed = key ? key->seed : 0, step = key ? key->step : 0;
    const TabularView v = tabular_view(state, *cfg);
    ScopedKernelTimer timer("rollout_mlp_tabular", (hipStream_t)stream);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((cfg->num_envs + 15) / 16)), dim3(kRollThreads), 0, (hipStream_t)stream, v, params,
                           dims->num_actions, *exp, noise, seed, step, (long long)env_offset, obs, rewards, terminals, truncations, masks);
    };
    switch (cfg->obs_stride) {
        case 16: launch(rollout_mlp_tabular_kernel<16, 4>); break;
        case 32: launch(rollout_mlp_tabular_kernel<32, 8>); break;
        case 64:   // 49..52 columns: the 13 k-steps the standalone forward issues for them
            if (cfg->obs_dim > 48 && cfg->obs_dim <= 52) launch(rollout_mlp_tabular_kernel<64, 13>);
            else launch(rollout_mlp_tabular_kernel<64, 16>);
            break;
        case 96: launch(rollout_mlp_tabular_kernel<96, 24>); break;
        default: launch(rollout_mlp_tabular_kernel<128, 32>); break;
    }
    PFA_LAUNCH_CHECK();
    return 0;
}
