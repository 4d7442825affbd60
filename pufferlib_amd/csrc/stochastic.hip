// stochastic.hip — ocean `Stochastic` (pufferlib/environments/ocean/ocean.py:529-582) as a device-resident vecenv: the second
// env family behind the same kernel shape as Squared.  What the reference runs per env is
// pufferlib.vector.Serial (vector.py:78-162) over make_stochastic (ocean/environment.py:61-64: horizon fixed to 100) =
// GymnasiumPufferEnv (emulation.py:169-228) over EpisodeStats (postprocess.py:18-54) over the env itself.
//
// The env has no randomness and no cross-env coupling: state = (tick, count of action 0), observation always [0.0],
//   reward = 1 - (p - count/tick)^2 in f64 if the action moved the action-0 fraction towards p, else 0   (ocean.py:566-576)
// cast to f32 by the buffer write (emulation.py:219), terminal when tick == horizon, the next send() is the auto-reset row
// (reward 0, terminal False; vector.py:147-151).  EpisodeStats: f64 sum of the episode's rewards in order, length, score =
// the last proximity.  Kernels: async_reset, send (protocol path), episode statistics, and the fused persistent rollout
// with the MLP policy (the env skeleton of rollout_env.hpp over the adapter below; observation row stride 16).
#include "common.hpp"
#include "episode_fin.hpp"
#include "rollout_env.hpp"

namespace pfa {

constexpr int kStoDP = 16;  // observation row stride in floats (1 real column)

struct StochasticEnv {
    int tick, count, done, ep_length;
    double ep_return;
};
using StochasticFin = EpisodeFin;  // episode_fin.hpp
struct StochasticView {
    StochasticEnv *env;
    StochasticFin *fin;
    int n;
};
struct StochasticStepView : StochasticView {   // what the kernels that step the env take: the state and the env's parameters
    int horizon;
    double p;
};
__host__ __device__ inline size_t stochastic_state_bytes(int n) {
    return (size_t)n * (sizeof(StochasticEnv) + sizeof(StochasticFin));
}
__host__ __device__ inline StochasticView stochastic_view(void *state, int n) {
    StochasticView v;
    v.env = (StochasticEnv *)state;
    v.fin = (StochasticFin *)((char *)state + (size_t)n * sizeof(StochasticEnv));
    v.n = n;
    return v;
}
__host__ __device__ inline StochasticStepView stochastic_view(void *state, int n, double p, int horizon) {
    StochasticStepView v;
    static_cast<StochasticView &>(v) = stochastic_view(state, n);
    v.horizon = horizon;
    v.p = p;
    return v;
}

__device__ __forceinline__ void stochastic_reset(StochasticEnv &s, float &reward, bool &terminal) {
    s.tick = s.count = 0;
    s.done = 0;
    s.ep_length = 0;
    s.ep_return = 0.0;
    reward = 0.0f;
    terminal = false;
}

// One env step (ocean.py:562-582 + postprocess.py:22-54 + emulation.py:194-228).  Returns true when the episode finished.
__device__ __forceinline__ bool stochastic_step(StochasticEnv &s, int action, double p, int horizon, float &reward, bool &terminal,
                                                double &fin_return, int &fin_length, double &fin_score) {
#pragma clang fp contract(off)  // python evaluates 1 - (p - frac)**2 with one rounding per operation: no fma contraction here
    s.tick += 1;
    s.count += action == 0;
    const double frac = (double)s.count / (double)s.tick;
    const double diff = p - frac;
    const double proximity = 1.0 - diff * diff;
    const double r = ((action == 0 && frac < p) || (action == 1 && frac >= p)) ? proximity : 0.0;
    s.ep_return += r;
    s.ep_length += 1;
    reward = (float)r;
    terminal = s.tick == horizon;
    s.done = terminal;
    if (terminal) {
        fin_return = s.ep_return;
        fin_length = s.ep_length;
        fin_score = proximity;
    }
    return terminal;
}

__global__ void __launch_bounds__(256) stochastic_reset_kernel(StochasticView v, float *obs, float *rewards, uint8_t *terminals,
                                                              uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    StochasticEnv s;
    float r;
    bool t;
    stochastic_reset(s, r, t);
    v.env[e] = s;
    StochasticFin f = {};
    v.fin[e] = f;
#pragma unroll
    for (int k = 0; k < kStoDP; ++k) obs[(size_t)e * kStoDP + k] = 0.0f;
    rewards[e] = 0.0f;
    terminals[e] = 0;
    truncations[e] = 0;
    masks[e] = 1;
}

// The env adapter (env_adapters.hpp): the one definition of a send, for the protocol kernel and the fused rollout
// (rollout_mlp_env_kernel<StochasticRollEnv, 16, 4>, rollout_env.hpp).
struct StochasticRollEnv {
    using View = StochasticStepView;
    static constexpr bool kRefresh = false;
    struct Shared {};
    StochasticEnv s = {};
    int last_fin = 0;

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int, Shared &, float *row, int action, float &reward, bool &terminal) {
        last_fin = 0;
        if (s.done) {
            stochastic_reset(s, reward, terminal);
        } else {
            double fr, fs;
            int fl;
            if (stochastic_step(s, action, v.p, v.horizon, reward, terminal, fr, fl, fs)) {
                episode_account(v.fin[e], fr, fl, fs);
                last_fin = 1;
            }
        }
        row[0] = 0.0f;   // the observation never changes
    }
    __device__ __forceinline__ void refresh(const View &, int, int, int, Shared &, float *) {}
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_stochastic_state_bytes(int32_t num_envs) { return num_envs > 0 ? stochastic_state_bytes(num_envs) : 0; }

extern "C" int pfa_stochastic_async_reset(void *state, int32_t num_envs, float *obs, float *rewards, uint8_t *terminals,
                                          uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    PFA_REQUIRE(state && num_envs >= 1 && obs && rewards && terminals && truncations && masks, "stochastic.async_reset: bad arguments");
    hipLaunchKernelGGL(stochastic_reset_kernel, dim3((unsigned)((num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       stochastic_view(state, num_envs), obs, rewards, terminals, truncations, masks);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_stochastic_send(void *state, int32_t num_envs, double p, int32_t horizon, const int64_t *actions, float *obs,
                                   float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    PFA_REQUIRE(num_envs >= 1 && horizon >= 1, "stochastic.send: bad arguments");
    return launch_env_send<StochasticRollEnv>("stochastic.send", state, stochastic_view(state, num_envs, p, horizon), kStoDP, actions, obs,
                                              rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_stochastic_episode_stats(void *state, int32_t num_envs, double *out4, int32_t reset, pfa_stream_t stream) {
    return launch_episode_stats("stochastic", state, stochastic_view(state, num_envs).fin, num_envs, out4, reset, nullptr, stream);
}

extern "C" int pfa_stochastic_last_infos(void *state, int32_t num_envs, uint8_t *finished, double *episode_return,
                                         int32_t *episode_length, double *score, pfa_stream_t stream) {
    return launch_episode_infos("stochastic", state, stochastic_view(state, num_envs).fin, num_envs, finished, episode_return,
                                episode_length, score, stream);
}

extern "C" int pfa_rollout_mlp_stochastic(void *state, int32_t num_envs, double p, int32_t horizon, const float *params,
                                          const pfa_mlp_dims *dims, const pfa_experience *exp, const float *noise,
                                          const pfa_noise_key *key, int64_t env_offset, float *obs, float *rewards,
                                          uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    PFA_REQUIRE(num_envs >= 1 && horizon >= 1 && dims, "rollout_mlp_stochastic: bad arguments");
    PFA_REQUIRE(dims->obs_stride == kStoDP && dims->obs_dim == 1,
                "rollout_mlp_stochastic: the policy must take 1 observation value in rows of 16 floats");
    PFA_REQUIRE(dims->num_actions >= 2 && dims->num_actions <= 15, "rollout_mlp_stochastic: num_actions out of range");
    return launch_rollout_mlp<StochasticRollEnv, kStoDP>("rollout_mlp_stochastic", state, stochastic_view(state, num_envs, p, horizon), params,
                                                         dims, exp, noise, key, env_offset, obs, rewards, terminals, truncations, masks,
                                                         stream);
}
