// acrobot.hip — the entry points of the Acrobot vecenv (acrobot_env.hpp: classic-control acrobot, f64 RK4 dynamics): each forwards to
// the protocol front (env_adapters.hpp) or to the classic-control family's bodies (control_entry.hpp) over AcrobotRollEnv; the
// state upload for tests is the family's own.  The fused recurrent rollout over it lives in lstm_fused.hip.
#include "common.hpp"
#include "control_entry.hpp"
#include "acrobot_env.hpp"

namespace pfa {

// the inverse of debug_states: env e becomes an episode that is ep_length steps old (return -ep_length: no step of it has succeeded)
// in the given state, and its live observation row and terminal flag follow; the episode statistics are not touched
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
    acrobot_observe(v, s, obs + (size_t)e * kControlDP);
    terminals[e] = s.done ? 1 : 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_acrobot_state_bytes(const pfa_acrobot_config *cfg) { return env_state_bytes<AcrobotRollEnv>(cfg); }

extern "C" int pfa_acrobot_async_reset(void *state, const pfa_acrobot_config *cfg, float *obs, float *rewards, uint8_t *terminals,
                                       uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return control_async_reset<AcrobotRollEnv>(state, cfg, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_acrobot_send(void *state, const pfa_acrobot_config *cfg, const int64_t *actions, float *obs, float *rewards,
                                uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return env_send<AcrobotRollEnv>(state, cfg, actions, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_acrobot_episode_stats(void *state, const pfa_acrobot_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    return env_episode_stats<AcrobotRollEnv>(state, cfg, out4, reset, stream);
}

extern "C" int pfa_acrobot_last_infos(void *state, const pfa_acrobot_config *cfg, uint8_t *finished, double *episode_return,
                                      int32_t *episode_length, double *score, pfa_stream_t stream) {
    return env_last_infos<AcrobotRollEnv>(state, cfg, finished, episode_return, episode_length, score, stream);
}

extern "C" int pfa_acrobot_debug_states(void *state, const pfa_acrobot_config *cfg, double *states4, int32_t *counters4,
                                        pfa_stream_t stream) {
    return control_debug_states<AcrobotRollEnv>(state, cfg, states4, counters4, stream);
}

extern "C" int pfa_acrobot_debug_set_states(void *state, const pfa_acrobot_config *cfg, const double *states4, const int32_t *counters4,
                                            float *obs, uint8_t *terminals, pfa_stream_t stream) {
    if (int rc = AcrobotRollEnv::check(cfg)) return rc;
    PFA_REQUIRE(state && states4 && counters4 && obs && terminals, "acrobot.debug_set_states: null buffer");
    return launch_per_env(acrobot_debug_set_states_kernel, cfg->num_envs, stream, AcrobotRollEnv::view(state, *cfg), states4, counters4, obs,
                          terminals);
}

extern "C" int pfa_rollout_mlp_acrobot(void *state, const pfa_acrobot_config *cfg, const float *params, const pfa_mlp_dims *dims,
                                       const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset,
                                       float *obs, float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks,
                                       pfa_stream_t stream) {
    return control_rollout_mlp<AcrobotRollEnv>(
        "rollout_mlp_acrobot", state, cfg, [&](TilePolicy *p) { return policy_of_flat(params, dims, p); }, exp, noise, key, env_offset, obs,
        rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_rollout_mlp_view_acrobot(void *state, const pfa_acrobot_config *cfg, const pfa_mlp_view *view, const pfa_experience *exp,
                                            const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                            uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return control_rollout_mlp<AcrobotRollEnv>(
        "rollout_mlp_view_acrobot", state, cfg, [&](TilePolicy *p) { return policy_of_view(view, p); }, exp, noise, key, env_offset, obs,
        rewards, terminals, truncations, masks, stream);
}
