// cartpole_env.hpp — classic-control cart-pole (the dynamics of gymnasium's CartPoleEnv, which the reference trains as
// `classic_control`): the one device env family with continuous dynamics and real-valued observations.  Per env the state is
// {f64 x, x_dot, theta, theta_dot, f64 ep_return, episode, tick, done, ep_length} next to an EpisodeFin.
//
// One send (the Serial protocol; the send after a terminal row is the auto-reset row):
//   done       action ignored, reward 0, terminal false, episode += 1, tick = 0, the four state values are drawn
//   otherwise  force = action == 1 ? +10 : -10, one explicit-Euler step of tau = 0.02 (x, x_dot, theta, theta_dot, each from the old
//              rates), tick += 1, reward 1 (on the terminating step too), terminal = |x| > 2.4 || |theta| > 12 degrees ||
//              (max_steps > 0 && tick == max_steps); on terminal the episode is accounted with score = the episode's return
// The observation row is 16 floats: the state cast to f32 in columns 0..3 (columns 1 and 3 are 0 without `velocities`: the partially
// observed task), zero behind them.
//
// Randomness is counter-based, there is no tape: the start state of (env, episode) is
//   value i = -0.05 + 0.1 * (word i * 2^-32),  words = Philox4x32-10(counter = (global env, episode, 0, 0), key = (seed lo, 'CP' ^ seed hi))
//
// Everything is f64 `+ - * /` in one fixed order and one f64 -> f32 conversion per observation value, so that a float64 walker on the
// host that spells the same operations gives the same bits (tests/cartpole_reference.py): sin and cos are fixed Taylor polynomials
// in theta^2 (|theta| stays inside the 12 degree threshold, because a terminal state is never stepped: the first dropped term is
// below 1e-20 there), and the arithmetic is compiled without contraction — a fused multiply-add rounds once where the walker
// rounds twice.
#pragma once
#include "common.hpp"
#include "episode_fin.hpp"
#include "philox.hpp"

namespace pfa {

constexpr int kCartDP = 16;   // floats per observation row
constexpr double kCartXLimit = 2.4, kCartThetaLimit = 0.20943951023931953;   // 12 * 2 * pi / 360 in f64

struct CartPoleEnv {
    double x, x_dot, theta, theta_dot, ep_return;
    int episode, tick, done, ep_length;
};
struct CartPoleView {
    CartPoleEnv *env;
    EpisodeFin *fin;
    int n, max_steps;
    bool velocities;
    uint32_t key0, key1;
    long long env_offset;
};
__host__ __device__ inline size_t cartpole_state_bytes(int n) { return (size_t)n * (sizeof(CartPoleEnv) + sizeof(EpisodeFin)); }
__host__ __device__ inline CartPoleView cartpole_view(void *state, const pfa_cartpole_config &c) {
    CartPoleView v;
    v.env = (CartPoleEnv *)state;
    v.fin = (EpisodeFin *)((char *)state + (size_t)c.num_envs * sizeof(CartPoleEnv));
    v.n = c.num_envs;
    v.max_steps = c.max_steps;
    v.velocities = c.velocities != 0;
    v.key0 = (uint32_t)c.seed;
    v.key1 = 0x4350u ^ (uint32_t)(c.seed >> 32);
    v.env_offset = c.env_offset;
    return v;
}

// What the entry points of the family refuse (cartpole.hip).
int check_cartpole_config(const pfa_cartpole_config *c);

__device__ __forceinline__ void cartpole_draw(const CartPoleView &v, int e, CartPoleEnv &s) {
#pragma clang fp contract(off)
    const u32x4 w = philox4x32_10((uint32_t)(v.env_offset + e), (uint32_t)s.episode, 0u, 0u, v.key0, v.key1);
    constexpr double k = 1.0 / 4294967296.0;
    s.x = -0.05 + 0.1 * ((double)w.x * k);
    s.x_dot = -0.05 + 0.1 * ((double)w.y * k);
    s.theta = -0.05 + 0.1 * ((double)w.z * k);
    s.theta_dot = -0.05 + 0.1 * ((double)w.w * k);
}

__device__ __forceinline__ void cartpole_begin_episode(const CartPoleView &v, int e, CartPoleEnv &s, float &reward, bool &terminal) {
    s.episode += 1;
    s.tick = 0;
    s.done = 0;
    s.ep_length = 0;
    s.ep_return = 0.0;
    cartpole_draw(v, e, s);
    reward = 0.0f;
    terminal = false;
}

// sin / cos of |theta| <= 0.21 as Horner polynomials in z = theta^2 (through theta^13 / theta^12)
__device__ __forceinline__ void cartpole_sincos(double theta, double &sn, double &cs) {
#pragma clang fp contract(off)
    const double z = theta * theta;
    double p = 1.0 / 6227020800.0;
    p = p * z + -1.0 / 39916800.0;
    p = p * z + 1.0 / 362880.0;
    p = p * z + -1.0 / 5040.0;
    p = p * z + 1.0 / 120.0;
    p = p * z + -1.0 / 6.0;
    p = p * z + 1.0;
    sn = theta * p;
    double q = 1.0 / 479001600.0;
    q = q * z + -1.0 / 3628800.0;
    q = q * z + 1.0 / 40320.0;
    q = q * z + -1.0 / 720.0;
    q = q * z + 1.0 / 24.0;
    q = q * z + -1.0 / 2.0;
    q = q * z + 1.0;
    cs = q;
}

// one env step; returns true when the episode finished
__device__ __forceinline__ bool cartpole_step(const CartPoleView &v, CartPoleEnv &s, int action, float &reward, bool &terminal,
                                              double &fin_return, int &fin_length, double &fin_score) {
#pragma clang fp contract(off)
    const double force = action == 1 ? 10.0 : -10.0;
    double sn, cs;
    cartpole_sincos(s.theta, sn, cs);
    const double temp = (force + 0.05 * (s.theta_dot * s.theta_dot) * sn) / 1.1;
    const double thetaacc = (9.8 * sn - cs * temp) / (0.5 * (4.0 / 3.0 - 0.1 * (cs * cs) / 1.1));
    const double xacc = temp - 0.05 * thetaacc * cs / 1.1;
    const double x = s.x + 0.02 * s.x_dot;
    const double x_dot = s.x_dot + 0.02 * xacc;
    const double theta = s.theta + 0.02 * s.theta_dot;
    const double theta_dot = s.theta_dot + 0.02 * thetaacc;
    s.x = x, s.x_dot = x_dot, s.theta = theta, s.theta_dot = theta_dot;
    s.tick += 1;
    s.ep_length += 1;
    s.ep_return += 1.0;
    reward = 1.0f;
    terminal = x < -kCartXLimit || x > kCartXLimit || theta < -kCartThetaLimit || theta > kCartThetaLimit ||
               (v.max_steps > 0 && s.tick == v.max_steps);
    s.done = terminal;
    if (terminal) {
        fin_return = s.ep_return;
        fin_length = s.ep_length;
        fin_score = s.ep_return;
    }
    return terminal;
}

// columns 0..3 of the env's observation row (the rest were zeroed by the reset and are never written again)
__device__ __forceinline__ void cartpole_observe(const CartPoleView &v, const CartPoleEnv &s, float *row) {
    row[0] = (float)s.x;
    row[1] = v.velocities ? (float)s.x_dot : 0.0f;
    row[2] = (float)s.theta;
    row[3] = v.velocities ? (float)s.theta_dot : 0.0f;
}

// The env adapter (env_adapters.hpp), in the shape of MemoryRollEnv: the owner steps and writes the four observation values itself.
struct CartPoleRollEnv {
    using View = CartPoleView;
    static View view(void *state, const pfa_cartpole_config &c) { return cartpole_view(state, c); }
    static constexpr bool kRefresh = false;
    struct Shared {};
    CartPoleEnv s = {};
    int last_fin = 0;

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int, Shared &, float *row, int action, float &reward, bool &terminal) {
        last_fin = 0;
        if (s.done) {
            cartpole_begin_episode(v, e, s, reward, terminal);
        } else {
            double fr, fs;
            int fl;
            if (cartpole_step(v, s, action, reward, terminal, fr, fl, fs)) {
                episode_account(v.fin[e], fr, fl, fs);
                last_fin = 1;
            }
        }
        cartpole_observe(v, s, row);
    }
    __device__ __forceinline__ void refresh(const View &, int, int, int, Shared &, float *) {}
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

}  // namespace pfa
