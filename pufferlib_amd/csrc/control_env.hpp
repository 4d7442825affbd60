// control_env.hpp — what the classic-control device env families (cartpole_env.hpp, acrobot_env.hpp) share, over a physics traits
// struct P that the family's header supplies:
//   State                  the env's state struct: four named f64 state values, then {f64 ep_return, int episode, tick, done, ep_length}
//   Config                 the family's config typedef of the public header ({num_envs, max_steps, velocities, seed, env_offset})
//   kName                  the family name in error texts
//   kObs, kActions         observation values per row (columns kObs.. of the kControlDP-float row stay zero) and the Discrete head
//   kKeyTag                what is xor-ed into the high key word of the Philox draws
//   kDrawLo, kDrawWidth    the start-state values are uniform in [kDrawLo, kDrawLo + kDrawWidth)
//   values / set_values    the four state values as an array, in the State's field order
//   observe(v, s, row)     columns 0..kObs-1 of the env's observation row
//   send(v, e, s, action, row, reward, terminal)
//                          one send of env e, observation row included (control_begin_episode on a done env, else the physics);
//                          returns true when the episode finished and was accounted
//
// Randomness is counter-based, there is no tape: the start state of (env, episode) is
//   value i = kDrawLo + kDrawWidth * (word i * 2^-32),  words = Philox4x32-10(counter = (global env, episode, 0, 0),
//                                                                             key = (seed lo, kKeyTag ^ seed hi))
// in f64 `+ *`, uncontracted, like everything else in these families (a float64 walker on the host gives the same bits).
#pragma once
#include "common.hpp"
#include "episode_fin.hpp"
#include "philox.hpp"

namespace pfa {

constexpr int kControlDP = 16;   // floats per observation row

template <class State>
struct ControlView {
    State *env;
    EpisodeFin *fin;
    int n, max_steps;
    bool velocities;
    uint32_t key0, key1;
    long long env_offset;
};

template <class P>
__device__ __forceinline__ void control_draw(const ControlView<typename P::State> &v, int e, typename P::State &s) {
#pragma clang fp contract(off)
    const u32x4 w = philox4x32_10((uint32_t)(v.env_offset + e), (uint32_t)s.episode, 0u, 0u, v.key0, v.key1);
    constexpr double k = 1.0 / 4294967296.0;
    P::set_values(s, P::kDrawLo + P::kDrawWidth * ((double)w.x * k), P::kDrawLo + P::kDrawWidth * ((double)w.y * k),
                  P::kDrawLo + P::kDrawWidth * ((double)w.z * k), P::kDrawLo + P::kDrawWidth * ((double)w.w * k));
}

template <class P>
__device__ __forceinline__ void control_begin_episode(const ControlView<typename P::State> &v, int e, typename P::State &s) {
    s.episode += 1;
    s.tick = 0;
    s.done = 0;
    s.ep_length = 0;
    s.ep_return = 0.0;
    control_draw<P>(v, e, s);
}

// The env adapter (env_adapters.hpp) of a classic-control family, in the shape of MemoryRollEnv: the owner steps and writes the
// observation values itself.  Beside the adapter's members it carries what the shared protocol front asks of a family.
template <class P>
struct ControlRollEnv {
    using Physics = P;
    using Config = typename P::Config;
    using View = ControlView<typename P::State>;
    static constexpr const char *kName = P::kName;
    static constexpr bool kRefresh = false;
    struct Shared {};
    typename P::State s = {};
    int last_fin = 0;

    // What the entry points of the family refuse.
    static int check(const Config *c) {
        PFA_REQUIRE(c != nullptr, "%s: null config", kName);
        PFA_REQUIRE(c->num_envs >= 1, "%s: num_envs must be >= 1 (got %d)", kName, c->num_envs);
        PFA_REQUIRE(c->max_steps >= 0, "%s: max_steps must be >= 0, 0 = no time limit (got %d)", kName, c->max_steps);
        return 0;
    }
    static size_t state_bytes(int n) { return (size_t)n * (sizeof(typename P::State) + sizeof(EpisodeFin)); }
    static int stride(const Config &) { return kControlDP; }
    static View view(void *state, const Config &c) {
        View v;
        v.env = (typename P::State *)state;
        v.fin = (EpisodeFin *)((char *)state + (size_t)c.num_envs * sizeof(typename P::State));
        v.n = c.num_envs;
        v.max_steps = c.max_steps;
        v.velocities = c.velocities != 0;
        v.key0 = (uint32_t)c.seed;
        v.key1 = P::kKeyTag ^ (uint32_t)(c.seed >> 32);
        v.env_offset = c.env_offset;
        return v;
    }

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int, Shared &, float *row, int action, float &reward, bool &terminal) {
        last_fin = P::send(v, e, s, action, row, reward, terminal) ? 1 : 0;
    }
    __device__ __forceinline__ void refresh(const View &, int, int, int, Shared &, float *) {}
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

}  // namespace pfa
