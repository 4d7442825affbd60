// acrobot.hip — protocol kernels of the Acrobot vecenv (acrobot_env.hpp: classic-control acrobot, f64 RK4 dynamics) and its fused
// persistent rollout with the MLP policy: the view form of the env skeleton (rollout_env.hpp) over AcrobotRollEnv, one instantiation
// per hidden width 64 / 128 / 256 / 512 of the 16-float row; the flat 128-wide buffer goes through the same kernel as a view of
// itself (mlp_view_of_flat).  The fused recurrent rollout over it lives in lstm_fused.hip.
#include "common.hpp"
#include "rollout_env.hpp"
#include "acrobot_env.hpp"

namespace pfa {

__global__ void __launch_bounds__(256) acrobot_reset_kernel(AcrobotView v, float *obs, float *rewards, uint8_t *terminals,
                                                           uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    AcrobotEnv s = {};
    s.episode = -1;
    acrobot_begin_episode(v, e, s);
    v.env[e] = s;
    v.fin[e] = EpisodeFin{};
    float *row = obs + (size_t)e * kAcroDP;
    for (int k = 6; k < kAcroDP; ++k) row[k] = 0.0f;
    acrobot_observe(v, s, row);
    rewards[e] = 0.0f;
    terminals[e] = 0;
    truncations[e] = 0;
    masks[e] = 1;
}

__global__ void __launch_bounds__(256) acrobot_debug_states_kernel(AcrobotView v, double *states4, int32_t *counters4) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const AcrobotEnv s = v.env[e];
    double *d = states4 + (size_t)e * 4;
    int32_t *o = counters4 + (size_t)e * 4;
    d[0] = s.th1, d[1] = s.th2, d[2] = s.w1, d[3] = s.w2;
    o[0] = s.episode, o[1] = s.tick, o[2] = s.done, o[3] = s.ep_length;
}

// the inverse: env e becomes an episode that is ep_length steps old (return -ep_length: no step of it has succeeded) in the given
// state, and its live observation row and terminal flag follow; the episode statistics are not touched
__global__ void __launch_bounds__(256) acrobot_debug_set_states_kernel(AcrobotView v, const double *states4, const int32_t *counters4,
                                                                      float *obs, uint8_t *terminals) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const double *d = states4 + (size_t)e * 4;
    const int32_t *o = counters4 + (size_t)e * 4;
    AcrobotEnv s;
    s.th1 = d[0], s.th2 = d[1], s.w1 = d[2], s.w2 = d[3];
    s.episode = o[0], s.tick = o[1], s.done = o[2] != 0, s.ep_length = o[3];
    s.ep_return = -(double)s.ep_length;
    v.env[e] = s;
    acrobot_observe(v, s, obs + (size_t)e * kAcroDP);
    terminals[e] = s.done ? 1 : 0;
}

int check_acrobot_config(const pfa_acrobot_config *c) {
    PFA_REQUIRE(c != nullptr, "acrobot: null config");
    PFA_REQUIRE(c->num_envs >= 1, "acrobot: num_envs must be >= 1 (got %d)", c->num_envs);
    PFA_REQUIRE(c->max_steps >= 0, "acrobot: max_steps must be >= 0, 0 = no time limit (got %d)", c->max_steps);
    return 0;
}

// what both MLP rollout entry points require of the policy they were given
static int check_acrobot_policy(const char *name, const TilePolicy &p) {
    PFA_REQUIRE(p.obs_stride == kAcroDP && p.obs_dim == 6, "%s: the policy must take 6 observation values in rows of %d floats (got %d in rows of %d)",
                name, kAcroDP, p.obs_dim, p.obs_stride);
    PFA_REQUIRE(p.pv.a == 3 && p.heads == 0, "%s: the policy must have one Discrete(3) head (got %d actions)", name, p.pv.a);
    return 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_acrobot_state_bytes(const pfa_acrobot_config *cfg) {
    return check_acrobot_config(cfg) ? 0 : acrobot_state_bytes(cfg->num_envs);
}

extern "C" int pfa_acrobot_async_reset(void *state, const pfa_acrobot_config *cfg, float *obs, float *rewards, uint8_t *terminals,
                                       uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    PFA_REQUIRE(state && obs && rewards && terminals && truncations && masks, "acrobot.async_reset: null buffer");
    hipLaunchKernelGGL(acrobot_reset_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       acrobot_view(state, *cfg), obs, rewards, terminals, truncations, masks);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_acrobot_send(void *state, const pfa_acrobot_config *cfg, const int64_t *actions, float *obs, float *rewards,
                                uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    return launch_env_send<AcrobotRollEnv>("acrobot.send", state, acrobot_view(state, *cfg), kAcroDP, actions, obs, rewards, terminals,
                                           truncations, masks, stream);
}

extern "C" int pfa_acrobot_episode_stats(void *state, const pfa_acrobot_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    return launch_episode_stats("acrobot", state, acrobot_view(state, *cfg).fin, cfg->num_envs, out4, reset, nullptr, stream);
}

extern "C" int pfa_acrobot_last_infos(void *state, const pfa_acrobot_config *cfg, uint8_t *finished, double *episode_return,
                                      int32_t *episode_length, double *score, pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    return launch_episode_infos("acrobot", state, acrobot_view(state, *cfg).fin, cfg->num_envs, finished, episode_return, episode_length,
                                score, stream);
}

extern "C" int pfa_acrobot_debug_states(void *state, const pfa_acrobot_config *cfg, double *states4, int32_t *counters4,
                                        pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    PFA_REQUIRE(state && states4 && counters4, "acrobot.debug_states: null buffer");
    hipLaunchKernelGGL(acrobot_debug_states_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       acrobot_view(state, *cfg), states4, counters4);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_acrobot_debug_set_states(void *state, const pfa_acrobot_config *cfg, const double *states4, const int32_t *counters4,
                                            float *obs, uint8_t *terminals, pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    PFA_REQUIRE(state && states4 && counters4 && obs && terminals, "acrobot.debug_set_states: null buffer");
    hipLaunchKernelGGL(acrobot_debug_set_states_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       acrobot_view(state, *cfg), states4, counters4, obs, terminals);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_rollout_mlp_acrobot(void *state, const pfa_acrobot_config *cfg, const float *params, const pfa_mlp_dims *dims,
                                       const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset,
                                       float *obs, float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks,
                                       pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    TilePolicy p;
    if (int rc = policy_of_flat(params, dims, &p)) return rc;
    if (int rc = check_acrobot_policy("rollout_mlp_acrobot", p)) return rc;
    return launch_rollout_mlp_view<AcrobotRollEnv, kAcroDP>("rollout_mlp_acrobot", state, acrobot_view(state, *cfg), p, exp, noise, key,
                                                            env_offset, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_rollout_mlp_view_acrobot(void *state, const pfa_acrobot_config *cfg, const pfa_mlp_view *view, const pfa_experience *exp,
                                            const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                            uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_acrobot_config(cfg)) return rc;
    TilePolicy p;
    if (int rc = policy_of_view(view, &p)) return rc;
    if (int rc = check_acrobot_policy("rollout_mlp_view_acrobot", p)) return rc;
    return launch_rollout_mlp_view<AcrobotRollEnv, kAcroDP>("rollout_mlp_view_acrobot", state, acrobot_view(state, *cfg), p, exp, noise, key,
                                                            env_offset, obs, rewards, terminals, truncations, masks, stream);
}
