// control_entry.hpp — what the .hip files of the classic-control families (cartpole.hip, acrobot.hip) share beside the protocol front of
// env_adapters.hpp: the reset and debug-states kernels over the physics traits (control_env.hpp) and the bodies of the test
// introspection and fused MLP rollout entry points over the family's adapter.  The view form of the env skeleton (rollout_env.hpp) is
// instantiated per hidden width 64 / 128 / 256 / 512 of the 16-float row; the flat 128-wide buffer goes through the same kernel as a
// view of itself (mlp_view_of_flat).
#pragma once
#include "control_env.hpp"
#include "rollout_env.hpp"

namespace pfa {

template <class P>
__global__ void __launch_bounds__(256) control_reset_kernel(ControlView<typename P::State> v, float *obs, float *rewards, uint8_t *terminals,
                                                           uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    typename P::State s = {};
    s.episode = -1;
    control_begin_episode<P>(v, e, s);
    v.env[e] = s;
    v.fin[e] = EpisodeFin{};
    float *row = obs + (size_t)e * kControlDP;
    for (int k = P::kObs; k < kControlDP; ++k) row[k] = 0.0f;
    P::observe(v, s, row);
    rewards[e] = 0.0f;
    terminals[e] = 0;
    truncations[e] = 0;
    masks[e] = 1;
}

template <class P>
__global__ void __launch_bounds__(256) control_debug_states_kernel(ControlView<typename P::State> v, double *states4, int32_t *counters4) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const typename P::State s = v.env[e];
    int32_t *o = counters4 + (size_t)e * 4;
    P::values(s, states4 + (size_t)e * 4);
    o[0] = s.episode, o[1] = s.tick, o[2] = s.done, o[3] = s.ep_length;
}

template <class Env>
static int control_async_reset(void *state, const typename Env::Config *cfg, float *obs, float *rewards, uint8_t *terminals,
                               uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return env_async_reset<Env>(control_reset_kernel<typename Env::Physics>, state, cfg, obs, rewards, terminals, truncations, masks, stream);
}

template <class Env>
static int control_debug_states(void *state, const typename Env::Config *cfg, double *states4, int32_t *counters4, pfa_stream_t stream) {
    if (int rc = Env::check(cfg)) return rc;
    PFA_REQUIRE(state && states4 && counters4, "%s.debug_states: null buffer", Env::kName);
    return launch_per_env(control_debug_states_kernel<typename Env::Physics>, cfg->num_envs, stream, Env::view(state, *cfg), states4, counters4);
}

// The two MLP rollout entry points: `name` is the entry point's kernel-timer name and the prefix of its error texts, `policy` fills
// the TilePolicy from what the entry point was given (policy_of_flat / policy_of_view).
template <class Env, class Policy>
static int control_rollout_mlp(const char *name, void *state, const typename Env::Config *cfg, Policy policy, const pfa_experience *exp,
                               const float *noise, const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                               uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    using P = typename Env::Physics;
    if (int rc = Env::check(cfg)) return rc;
    TilePolicy p;
    if (int rc = policy(&p)) return rc;
    PFA_REQUIRE(p.obs_stride == kControlDP && p.obs_dim == P::kObs,
                "%s: the policy must take %d observation values in rows of %d floats (got %d in rows of %d)", name, P::kObs, kControlDP,
                p.obs_dim, p.obs_stride);
    PFA_REQUIRE(p.pv.a == P::kActions && p.heads == 0, "%s: the policy must have one Discrete(%d) head (got %d actions)", name, P::kActions,
                p.pv.a);
    return launch_rollout_mlp_view<Env, kControlDP>(name, state, Env::view(state, *cfg), p, exp, noise, key, env_offset, obs, rewards,
                                                    terminals, truncations, masks, stream);
}

}  // namespace pfa
