// tabular.hip — protocol kernels of the Tabular vecenv (tabular_env.hpp: a user-given finite MDP / POMDP as device tables) and its
// fused persistent rollout with the MLP policy (the env skeleton of rollout_env.hpp over TabularRollEnv, one instantiation per row
// stride 16 / 32 / 64 / 96 / 128 and the 13-k-step form of the 64-float row).  The fused recurrent rollout over it lives in
// lstm_fused.hip.
#include "common.hpp"
#include "rollout_env.hpp"
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
    PFA_REQUIRE(c->obs_stride >= c->obs_dim && valid_row_stride(c->obs_stride, 160),
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
    PFA_REQUIRE(dims, "rollout_mlp_tabular: null dims");
    PFA_REQUIRE(dims->obs_stride == cfg->obs_stride && dims->obs_dim == cfg->obs_dim && cfg->obs_stride <= 128,
                "rollout_mlp_tabular: the policy must take %d observation values in rows of %d floats (16/32/64/96/128), got %d in rows of %d",
                cfg->obs_dim, cfg->obs_stride, dims->obs_dim, dims->obs_stride);
    PFA_REQUIRE(dims->num_actions == cfg->num_actions && dims->num_actions >= 2 && dims->num_actions <= 15,
                "rollout_mlp_tabular: the policy must have one Discrete(%d) head of 2..15 actions (got %d)", cfg->num_actions, dims->num_actions);
    return launch_rollout_mlp<TabularRollEnv>("rollout_mlp_tabular", state, tabular_view(state, *cfg), params, dims, exp, noise, key, env_offset,
                                              obs, rewards, terminals, truncations, masks, stream);
}
