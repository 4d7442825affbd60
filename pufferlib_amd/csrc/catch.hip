// catch.hip — the Catch vecenv (catch_row_env.hpp: the Catch state machine of catch_env.hpp as flat float32 rows): the reset and
// debug-states kernels, the protocol entry points through the shared front (env_adapters.hpp) and the fused persistent MLP rollouts —
// the env skeleton of rollout_env.hpp over CatchRowEnv, in the flat 128-wide form at every row stride (16 / 32 / 64 / 96 / 128) and in
// the view form (hidden 64 / 128 / 256 / 512) at rows of up to 64 floats.  The fused recurrent rollout over it lives in lstm_fused.hip.
#include "common.hpp"
#include "rollout_env.hpp"
#include "catch_row_env.hpp"

namespace pfa {

__global__ void __launch_bounds__(256) catch_reset_kernel(CatchRowView v, float *obs, float *rewards, uint8_t *terminals,
                                                         uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    CatchRowSendEnv env;
    CatchRowSendEnv::Shared sh;
    env.reset(v, e);
    env.store(v, e, 0, sh);
    for (int lo = 0; lo < 16; ++lo) env.refresh(v, e, 0, lo, sh, obs + (size_t)e * v.stride);
    rewards[e] = 0.0f;
    terminals[e] = 0;
    truncations[e] = 0;
    masks[e] = 1;
}

__global__ void __launch_bounds__(256) catch_debug_states_kernel(CatchRowView v, int32_t *out6) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const CatchEnv s = v.env[e];
    int32_t *o = out6 + (size_t)e * 6;
    o[0] = s.r[0], o[1] = s.c[0], o[2] = s.p[0], o[3] = s.vx, o[4] = s.episode, o[5] = s.ep_length;
}

int check_catch_config(const pfa_catch_config *c) {
    PFA_REQUIRE(c != nullptr, "catch: null config");
    PFA_REQUIRE(c->num_envs >= 1, "catch: num_envs must be >= 1 (got %d)", c->num_envs);
    PFA_REQUIRE(c->rows >= 3 && c->cols >= 2, "catch: the grid must have at least 3 rows and 2 columns (got %d x %d)", c->rows, c->cols);
    PFA_REQUIRE(c->obs_form == PFA_CATCH_OBS_GRID || c->obs_form == PFA_CATCH_OBS_COORDS, "catch: obs_form must be 0 (grid) or 1 (coords), got %d",
                c->obs_form);
    PFA_REQUIRE(c->rows <= kCatchRowMaxSide && c->cols <= kCatchRowMaxSide, "catch: the grid's sides must be at most %d (got %d x %d)",
                kCatchRowMaxSide, c->rows, c->cols);
    PFA_REQUIRE(c->obs_form == PFA_CATCH_OBS_COORDS || c->rows * c->cols <= kCatchRowMaxCells,
                "catch: the grid form shows at most %d cells (got %d x %d)", kCatchRowMaxCells, c->rows, c->cols);
    const int values = c->obs_form == PFA_CATCH_OBS_COORDS ? 4 : c->rows * c->cols;
    PFA_REQUIRE(valid_row_stride(c->obs_stride, 160) && c->obs_stride >= values,
                "catch: obs_stride must be one of 16/32/64/96/128/160 and hold the %d observation values (got %d)", values, c->obs_stride);
    return 0;
}

// What a policy must look like to roll out on the env: the env's row and one Discrete(3) head.
static int check_catch_policy(const char *name, const pfa_catch_config *cfg, int obs_dim, int obs_stride, int max_stride, int a, uint32_t heads) {
    const int values = cfg->obs_form == PFA_CATCH_OBS_COORDS ? (cfg->velocities ? 4 : 3) : cfg->rows * cfg->cols;
    PFA_REQUIRE(obs_stride == cfg->obs_stride && obs_dim == values && obs_stride <= max_stride,
                "%s: the policy must take %d observation values in rows of %d floats (at most %d), got %d in rows of %d", name, values,
                cfg->obs_stride, max_stride, obs_dim, obs_stride);
    PFA_REQUIRE(a == 3 && heads == 0, "%s: the policy must have one Discrete(3) head (got %d actions)", name, a);
    return 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_catch_state_bytes(const pfa_catch_config *cfg) { return env_state_bytes<CatchRowSendEnv>(cfg); }

extern "C" int pfa_catch_async_reset(void *state, const pfa_catch_config *cfg, float *obs, float *rewards, uint8_t *terminals,
                                     uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return env_async_reset<CatchRowSendEnv>(catch_reset_kernel, state, cfg, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_catch_send(void *state, const pfa_catch_config *cfg, const int64_t *actions, float *obs, float *rewards, uint8_t *terminals,
                              uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return env_send<CatchRowSendEnv>(state, cfg, actions, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_catch_episode_stats(void *state, const pfa_catch_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    return env_episode_stats<CatchRowSendEnv>(state, cfg, out4, reset, stream);
}

extern "C" int pfa_catch_last_infos(void *state, const pfa_catch_config *cfg, uint8_t *finished, double *episode_return, int32_t *episode_length,
                                    double *score, pfa_stream_t stream) {
    return env_last_infos<CatchRowSendEnv>(state, cfg, finished, episode_return, episode_length, score, stream);
}

extern "C" int pfa_catch_debug_states(void *state, const pfa_catch_config *cfg, int32_t *out6, pfa_stream_t stream) {
    if (int rc = check_catch_config(cfg)) return rc;
    PFA_REQUIRE(state && out6, "catch.debug_states: null buffer");
    return launch_per_env(catch_debug_states_kernel, cfg->num_envs, stream, CatchRowEnv::view(state, *cfg), out6);
}

extern "C" int pfa_rollout_mlp_catch(void *state, const pfa_catch_config *cfg, const float *params, const pfa_mlp_dims *dims,
                                     const pfa_experience *exp, const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs,
                                     float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_catch_config(cfg)) return rc;
    if (int rc = check_dims(dims)) return rc;
    if (int rc = check_catch_policy("rollout_mlp_catch", cfg, dims->obs_dim, dims->obs_stride, 128, dims->num_actions, dims->heads)) return rc;
    return launch_rollout_mlp<CatchRowEnv>("rollout_mlp_catch", state, CatchRowEnv::view(state, *cfg), params, dims, exp, noise, key, env_offset,
                                           obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_rollout_mlp_view_catch(void *state, const pfa_catch_config *cfg, const pfa_mlp_view *view, const pfa_experience *exp,
                                          const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                          uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_catch_config(cfg)) return rc;
    TilePolicy p;
    if (int rc = policy_of_view(view, &p)) return rc;
    if (int rc = check_catch_policy("rollout_mlp_view_catch", cfg, p.obs_dim, p.obs_stride, 64, p.pv.a, p.heads)) return rc;
    return launch_rollout_mlp_view<CatchRowEnv>("rollout_mlp_view_catch", state, CatchRowEnv::view(state, *cfg), p, exp, noise, key, env_offset,
                                                obs, rewards, terminals, truncations, masks, stream);
}
