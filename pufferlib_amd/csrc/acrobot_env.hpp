// acrobot_env.hpp — classic-control acrobot (the dynamics of gymnasium's AcrobotEnv, "book" equations, no torque noise): the two-link
// swing-up task.  Per env the state is {f64 th1, th2, w1, w2, f64 ep_return, episode, tick, done, ep_length} next to an EpisodeFin.
//
// One send (the Serial protocol; the send after a terminal row is the auto-reset row):
//   done       action ignored, reward 0, terminal false, episode += 1, tick = 0, the four state values are drawn
//   otherwise  torque = action - 1, one classical RK4 step of dt = 0.2 with the torque held, th1 and th2 wrapped into [-pi, pi] by
//              gymnasium's loops, w1 and w2 clamped to +-4 pi and +-9 pi, tick += 1; the swing-up has succeeded when -cos th1 -
//              cos(th1 + th2) > 1 on the new state; reward -1, or 0 on the succeeding step; terminal = succeeded || (max_steps > 0
//              && tick == max_steps); on terminal the episode is accounted with score = the episode's return
//              (the wrap loops take at most kAcroWraps turns each, so that no uploaded state can spin a lane: RK4 at dt = 0.2 is
//              far outside its stable range with both velocities at their clamps, where one step was seen to carry an angle to
//              29 rad, 5 turns)
// The observation row is 16 floats: (cos th1, sin th1, cos th2, sin th2, w1, w2) cast to f32 in columns 0..5 (columns 4 and 5 are 0
// without `velocities`: the partially observed task), zero behind them.
//
// Randomness is counter-based, there is no tape: the start state of (env, episode) is
//   value i = -0.1 + 0.2 * (word i * 2^-32),  words = Philox4x32-10(counter = (global env, episode, 0, 0), key = (seed lo, 'AC' ^ seed hi))
//
// Everything is f64 `+ - * /` in one fixed order, uncontracted, sin and cos are f64_sincos.hpp's, and there is one f64 -> f32
// conversion per observation value, so that a float64 walker on the host that spells the same operations gives the same bits
// (tests/acrobot_reference.py).  The four RK4 stages are one rolled loop: the right-hand side stands in a kernel once.
#pragma once
#include "common.hpp"
#include "episode_fin.hpp"
#include "philox.hpp"
#include "f64_sincos.hpp"

namespace pfa {

constexpr int kAcroDP = 16;     // floats per observation row
constexpr int kAcroWraps = 64;  // turns of each wrap loop at the most
constexpr double kAcroPi = 3.141592653589793, kAcroMaxVel1 = 4.0 * kAcroPi, kAcroMaxVel2 = 9.0 * kAcroPi;

struct AcrobotEnv {
    double th1, th2, w1, w2, ep_return;
    int episode, tick, done, ep_length;
};
struct AcrobotView {
    AcrobotEnv *env;
    EpisodeFin *fin;
    int n, max_steps;
    bool velocities;
    uint32_t key0, key1;
    long long env_offset;
};
__host__ __device__ inline size_t acrobot_state_bytes(int n) { return (size_t)n * (sizeof(AcrobotEnv) + sizeof(EpisodeFin)); }
__host__ __device__ inline AcrobotView acrobot_view(void *state, const pfa_acrobot_config &c) {
    AcrobotView v;
    v.env = (AcrobotEnv *)state;
    v.fin = (EpisodeFin *)((char *)state + (size_t)c.num_envs * sizeof(AcrobotEnv));
    v.n = c.num_envs;
    v.max_steps = c.max_steps;
    v.velocities = c.velocities != 0;
    v.key0 = (uint32_t)c.seed;
    v.key1 = 0x4143u ^ (uint32_t)(c.seed >> 32);
    v.env_offset = c.env_offset;
    return v;
}

// What the entry points of the family refuse (acrobot.hip).
int check_acrobot_config(const pfa_acrobot_config *c);

__device__ __forceinline__ void acrobot_draw(const AcrobotView &v, int e, AcrobotEnv &s) {
#pragma clang fp contract(off)
    const u32x4 w = philox4x32_10((uint32_t)(v.env_offset + e), (uint32_t)s.episode, 0u, 0u, v.key0, v.key1);
    constexpr double k = 1.0 / 4294967296.0;
    s.th1 = -0.1 + 0.2 * ((double)w.x * k);
    s.th2 = -0.1 + 0.2 * ((double)w.y * k);
    s.w1 = -0.1 + 0.2 * ((double)w.z * k);
    s.w2 = -0.1 + 0.2 * ((double)w.w * k);
}

__device__ __forceinline__ void acrobot_begin_episode(const AcrobotView &v, int e, AcrobotEnv &s) {
    s.episode += 1;
    s.tick = 0;
    s.done = 0;
    s.ep_length = 0;
    s.ep_return = 0.0;
    acrobot_draw(v, e, s);
}

// gymnasium's _dsdt with m1 = m2 = l1 = I1 = I2 = 1, lc1 = lc2 = 0.5, g = 9.8 (the products with 1 are dropped: they are exact)
__device__ __forceinline__ void acrobot_dsdt(double th1, double th2, double w1, double w2, double torque, double &a1, double &a2) {
#pragma clang fp contract(off)
    constexpr double kHalfPi = kAcroPi / 2.0;
    double s2, c2, sn, c12, c1;
    f64_sincos(th2, s2, c2);
    f64_sincos((th1 + th2) - kHalfPi, sn, c12);
    f64_sincos(th1 - kHalfPi, sn, c1);
    const double d1 = ((0.25 + (1.25 + c2)) + 1.0) + 1.0;
    const double d2 = (0.25 + 0.5 * c2) + 1.0;
    const double phi2 = (0.5 * 9.8) * c12;
    const double phi1 = (((-0.5 * (w2 * w2)) * s2 - (w2 * w1) * s2) + (1.5 * 9.8) * c1) + phi2;
    a2 = (((torque + (d2 / d1) * phi1) - (0.5 * (w1 * w1)) * s2) - phi2) / (1.25 - (d2 * d2) / d1);
    a1 = -((d2 * a2 + phi1) / d1);
}

__device__ __forceinline__ double acrobot_wrap(double x) {
#pragma clang fp contract(off)
    constexpr double kTwoPi = 2.0 * kAcroPi;
#pragma unroll 1
    for (int i = 0; i < kAcroWraps && x > kAcroPi; ++i) x = x - kTwoPi;
#pragma unroll 1
    for (int i = 0; i < kAcroWraps && x < -kAcroPi; ++i) x = x + kTwoPi;
    return x;
}

// RK4 over [0, dt], wrap, clamp: the physics of one step
__device__ __forceinline__ void acrobot_advance(AcrobotEnv &s, int action) {
#pragma clang fp contract(off)
    constexpr double kDt = 0.2, kHalfDt = kDt / 2.0, kSixthDt = kDt / 6.0;
    const double torque = (double)(action - 1);
    double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;           // the previous stage's derivative
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;           // k1 + 2 k2 + 2 k3 + k4 so far
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const double h = i == 0 ? 0.0 : (i == 3 ? kDt : kHalfDt);
        const double wgt = (i == 0 || i == 3) ? 1.0 : 2.0;
        const double y0 = s.th1 + h * k0, y1 = s.th2 + h * k1, y2 = s.w1 + h * k2, y3 = s.w2 + h * k3;
        k0 = y2, k1 = y3;
        acrobot_dsdt(y0, y1, y2, y3, torque, k2, k3);
        g0 = g0 + wgt * k0, g1 = g1 + wgt * k1, g2 = g2 + wgt * k2, g3 = g3 + wgt * k3;
    }
    s.th1 = acrobot_wrap(s.th1 + kSixthDt * g0);
    s.th2 = acrobot_wrap(s.th2 + kSixthDt * g1);
    double w1 = s.w1 + kSixthDt * g2, w2 = s.w2 + kSixthDt * g3;
    w1 = w1 < -kAcroMaxVel1 ? -kAcroMaxVel1 : w1;
    w1 = w1 > kAcroMaxVel1 ? kAcroMaxVel1 : w1;
    w2 = w2 < -kAcroMaxVel2 ? -kAcroMaxVel2 : w2;
    w2 = w2 > kAcroMaxVel2 ? kAcroMaxVel2 : w2;
    s.w1 = w1, s.w2 = w2;
}

// columns 0..5 of the env's observation row (the rest were zeroed by the reset and are never written again); returns cos th1
__device__ __forceinline__ double acrobot_observe(const AcrobotView &v, const AcrobotEnv &s, float *row) {
    double s1, c1, s2, c2;
    f64_sincos(s.th1, s1, c1);
    f64_sincos(s.th2, s2, c2);
    row[0] = (float)c1;
    row[1] = (float)s1;
    row[2] = (float)c2;
    row[3] = (float)s2;
    row[4] = v.velocities ? (float)s.w1 : 0.0f;
    row[5] = v.velocities ? (float)s.w2 : 0.0f;
    return c1;
}

// one send of env e, observation row included; returns true when the episode finished (and was accounted)
__device__ __forceinline__ bool acrobot_send(const AcrobotView &v, int e, AcrobotEnv &s, int action, float *row, float &reward, bool &terminal) {
#pragma clang fp contract(off)
    const bool stepped = !s.done;
    if (stepped) {
        acrobot_advance(s, action);
    } else {
        acrobot_begin_episode(v, e, s);
    }
    const double c1 = acrobot_observe(v, s, row);
    reward = 0.0f;
    terminal = false;
    if (stepped) {
        double sn, c12;
        f64_sincos(s.th1 + s.th2, sn, c12);
        const bool up = -c1 - c12 > 1.0;
        const double r = up ? 0.0 : -1.0;
        s.tick += 1;
        s.ep_length += 1;
        s.ep_return = s.ep_return + r;
        reward = (float)r;
        terminal = up || (v.max_steps > 0 && s.tick == v.max_steps);
        s.done = terminal;
        if (terminal) episode_account(v.fin[e], s.ep_return, s.ep_length, s.ep_return);
    }
    return terminal;
}

// The env adapter (env_adapters.hpp), in the shape of CartPoleRollEnv: the owner steps and writes the six observation values itself.
struct AcrobotRollEnv {
    using View = AcrobotView;
    static View view(void *state, const pfa_acrobot_config &c) { return acrobot_view(state, c); }
    static constexpr bool kRefresh = false;
    struct Shared {};
    AcrobotEnv s = {};
    int last_fin = 0;

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int, Shared &, float *row, int action, float &reward, bool &terminal) {
        last_fin = acrobot_send(v, e, s, action, row, reward, terminal) ? 1 : 0;
    }
    __device__ __forceinline__ void refresh(const View &, int, int, int, Shared &, float *) {}
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

}  // namespace pfa
