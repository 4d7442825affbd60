// cartpole.hip — the entry points of the CartPole vecenv (cartpole_env.hpp: classic-control cart-pole, f64 dynamics): each forwards to
// the protocol front (env_adapters.hpp) or to the classic-control family's bodies (control_entry.hpp) over CartPoleRollEnv.  The fused
// recurrent rollout over it lives in lstm_fused.hip.
#include "common.hpp"
#include "control_entry.hpp"
#include "cartpole_env.hpp"

using namespace pfa;

extern "C" size_t pfa_cartpole_state_bytes(const pfa_cartpole_config *cfg) { return env_state_bytes<CartPoleRollEnv>(cfg); }

extern "C" int pfa_cartpole_async_reset(void *state, const pfa_cartpole_config *cfg, float *obs, float *rewards, uint8_t *terminals,
                                        uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return control_async_reset<CartPoleRollEnv>(state, cfg, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_cartpole_send(void *state, const pfa_cartpole_config *cfg, const int64_t *actions, float *obs, float *rewards,
                                 uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return env_send<CartPoleRollEnv>(state, cfg, actions, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_cartpole_episode_stats(void *state, const pfa_cartpole_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    return env_episode_stats<CartPoleRollEnv>(state, cfg, out4, reset, stream);
}

extern "C" int pfa_cartpole_last_infos(void *state, const pfa_cartpole_config *cfg, uint8_t *finished, double *episode_return,
                                       int32_t *episode_length, double *score, pfa_stream_t stream) {
    return env_last_infos<CartPoleRollEnv>(state, cfg, finished, episode_return, episode_length, score, stream);
}

extern "C" int pfa_cartpole_debug_states(void *state, const pfa_cartpole_config *cfg, double *states4, int32_t *counters4,
                                         pfa_stream_t stream) {
    return control_debug_states<CartPoleRollEnv>(state, cfg, states4, counters4, stream);
}

extern "C" int pfa_rollout_mlp_cartpole(void *state, const pfa_cartpole_config *cfg, const float *params, const pfa_mlp_dims *dims,
                                        const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset,
                                        float *obs, float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks,
                                        pfa_stream_t stream) {
    return control_rollout_mlp<CartPoleRollEnv>(
        "rollout_mlp_cartpole", state, cfg, [&](TilePolicy *p) { return policy_of_flat(params, dims, p); }, exp, noise, key, env_offset, obs,
        rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_rollout_mlp_view_cartpole(void *state, const pfa_cartpole_config *cfg, const pfa_mlp_view *view, const pfa_experience *exp,
                                             const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                             uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return control_rollout_mlp<CartPoleRollEnv>(
        "rollout_mlp_view_cartpole", state, cfg, [&](TilePolicy *p) { return policy_of_view(view, p); }, exp, noise, key, env_offset, obs,
        rewards, terminals, truncations, masks, stream);
}
