// cartpole.hip — protocol kernels of the CartPole vecenv (cartpole_env.hpp: classic-control cart-pole, f64 dynamics) and its fused
// persistent rollout with the MLP policy: the view form of the env skeleton (rollout_env.hpp) over CartPoleRollEnv, one
// instantiation per hidden width 64 / 128 / 256 / 512 of the 16-float row; the flat 128-wide buffer goes through the same kernel as a
// view of itself (mlp_view_of_flat).  The fused recurrent rollout over it lives in lstm_fused.hip.
#include "common.hpp"
#include "rollout_env.hpp"
#include "cartpole_env.hpp"

namespace pfa {

__global__ void __launch_bounds__(256) cartpole_reset_kernel(CartPoleView v, float *obs, float *rewards, uint8_t *terminals,
                                                            uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    CartPoleEnv s = {};
    s.episode = -1;
    float r;
    bool t;
    cartpole_begin_episode(v, e, s, r, t);
    v.env[e] = s;
    v.fin[e] = EpisodeFin{};
    float *row = obs + (size_t)e * kCartDP;
    for (int k = 4; k < kCartDP; ++k) row[k] = 0.0f;
    cartpole_observe(v, s, row);
    rewards[e] = 0.0f;
    terminals[e] = 0;
    truncations[e] = 0;
    masks[e] = 1;
}

__global__ void __launch_bounds__(256) cartpole_debug_states_kernel(CartPoleView v, double *states4, int32_t *counters4) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const CartPoleEnv s = v.env[e];
    double *d = states4 + (size_t)e * 4;
    int32_t *o = counters4 + (size_t)e * 4;
    d[0] = s.x, d[1] = s.x_dot, d[2] = s.theta, d[3] = s.theta_dot;
    o[0] = s.episode, o[1] = s.tick, o[2] = s.done, o[3] = s.ep_length;
}

int check_cartpole_config(const pfa_cartpole_config *c) {
    PFA_REQUIRE(c != nullptr, "cartpole: null config");
    PFA_REQUIRE(c->num_envs >= 1, "cartpole: num_envs must be >= 1 (got %d)", c->num_envs);
    PFA_REQUIRE(c->max_steps >= 0, "cartpole: max_steps must be >= 0, 0 = no time limit (got %d)", c->max_steps);
    return 0;
}

// what both MLP rollout entry points require of the policy they were given
static int check_cartpole_policy(const char *name, const TilePolicy &p) {
    PFA_REQUIRE(p.obs_stride == kCartDP && p.obs_dim == 4, "%s: the policy must take 4 observation values in rows of %d floats (got %d in rows of %d)",
                name, kCartDP, p.obs_dim, p.obs_stride);
    PFA_REQUIRE(p.pv.a == 2 && p.heads == 0, "%s: the policy must have one Discrete(2) head (got %d actions)", name, p.pv.a);
    return 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_cartpole_state_bytes(const pfa_cartpole_config *cfg) {
    return check_cartpole_config(cfg) ? 0 : cartpole_state_bytes(cfg->num_envs);
}

extern "C" int pfa_cartpole_async_reset(void *state, const pfa_cartpole_config *cfg, float *obs, float *rewards, uint8_t *terminals,
                                        uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    PFA_REQUIRE(state && obs && rewards && terminals && truncations && masks, "cartpole.async_reset: null buffer");
    hipLaunchKernelGGL(cartpole_reset_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       cartpole_view(state, *cfg), obs, rewards, terminals, truncations, masks);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_cartpole_send(void *state, const pfa_cartpole_config *cfg, const int64_t *actions, float *obs, float *rewards,
                                 uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    return launch_env_send<CartPoleRollEnv>("cartpole.send", state, cartpole_view(state, *cfg), kCartDP, actions, obs, rewards, terminals,
                                            truncations, masks, stream);
}

extern "C" int pfa_cartpole_episode_stats(void *state, const pfa_cartpole_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    return launch_episode_stats("cartpole", state, cartpole_view(state, *cfg).fin, cfg->num_envs, out4, reset, nullptr, stream);
}

extern "C" int pfa_cartpole_last_infos(void *state, const pfa_cartpole_config *cfg, uint8_t *finished, double *episode_return,
                                       int32_t *episode_length, double *score, pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    return launch_episode_infos("cartpole", state, cartpole_view(state, *cfg).fin, cfg->num_envs, finished, episode_return, episode_length,
                                score, stream);
}

extern "C" int pfa_cartpole_debug_states(void *state, const pfa_cartpole_config *cfg, double *states4, int32_t *counters4,
                                         pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    PFA_REQUIRE(state && states4 && counters4, "cartpole.debug_states: null buffer");
    hipLaunchKernelGGL(cartpole_debug_states_kernel, dim3((unsigned)((cfg->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       cartpole_view(state, *cfg), states4, counters4);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_rollout_mlp_cartpole(void *state, const pfa_cartpole_config *cfg, const float *params, const pfa_mlp_dims *dims,
                                        const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset,
                                        float *obs, float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks,
                                        pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    TilePolicy p;
    if (int rc = policy_of_flat(params, dims, &p)) return rc;
    if (int rc = check_cartpole_policy("rollout_mlp_cartpole", p)) return rc;
    return launch_rollout_mlp_view<CartPoleRollEnv, kCartDP>("rollout_mlp_cartpole", state, cartpole_view(state, *cfg), p, exp, noise, key,
                                                             env_offset, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_rollout_mlp_view_cartpole(void *state, const pfa_cartpole_config *cfg, const pfa_mlp_view *view, const pfa_experience *exp,
                                             const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                             uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_cartpole_config(cfg)) return rc;
    TilePolicy p;
    if (int rc = policy_of_view(view, &p)) return rc;
    if (int rc = check_cartpole_policy("rollout_mlp_view_cartpole", p)) return rc;
    return launch_rollout_mlp_view<CartPoleRollEnv, kCartDP>("rollout_mlp_view_cartpole", state, cartpole_view(state, *cfg), p, exp, noise, key,
                                                             env_offset, obs, rewards, terminals, truncations, masks, stream);
}
