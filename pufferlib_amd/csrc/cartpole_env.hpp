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
#include "control_env.hpp"

namespace pfa {

constexpr double kCartXLimit = 2.4, kCartThetaLimit = 0.20943951023931953;   // 12 * 2 * pi / 360 in f64

struct CartPoleEnv {
    double x, x_dot, theta, theta_dot, ep_return;
    int episode, tick, done, ep_length;
};
using CartPoleView = ControlView<CartPoleEnv>;

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

// The physics traits of the family (control_env.hpp).
struct CartPolePhysics {
    using State = CartPoleEnv;
    using Config = pfa_cartpole_config;
    static constexpr const char *kName = "cartpole";
    static constexpr int kObs = 4, kActions = 2;
    static constexpr uint32_t kKeyTag = 0x4350u;   // 'CP'
    static constexpr double kDrawLo = -0.05, kDrawWidth = 0.1;
    __device__ __forceinline__ static void values(const State &s, double *d) { d[0] = s.x, d[1] = s.x_dot, d[2] = s.theta, d[3] = s.theta_dot; }
    __device__ __forceinline__ static void set_values(State &s, double x, double x_dot, double theta, double theta_dot) {
        s.x = x, s.x_dot = x_dot, s.theta = theta, s.theta_dot = theta_dot;
    }
    __device__ __forceinline__ static void observe(const CartPoleView &v, const State &s, float *row) { cartpole_observe(v, s, row); }
    __device__ __forceinline__ static bool send(const CartPoleView &v, int e, State &s, int action, float *row, float &reward, bool &terminal) {
        bool fin = false;
        if (s.done) {
            control_begin_episode<CartPolePhysics>(v, e, s);
            reward = 0.0f;
            terminal = false;
        } else {
            double fr, fs;
            int fl;
            fin = cartpole_step(v, s, action, reward, terminal, fr, fl, fs);
            if (fin) episode_account(v.fin[e], fr, fl, fs);
        }
        cartpole_observe(v, s, row);
        return fin;
    }
};
struct CartPoleRollEnv : ControlRollEnv<CartPolePhysics> {};

}  // namespace pfa
