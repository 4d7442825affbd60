"""CPU restatement of vector.Acrobot (csrc/acrobot_env.hpp, csrc/f64_sincos.hpp) for the tests: a numpy float64 walker speaking the
Serial protocol (async_reset / recv / send, infos, auto-reset rows), with the interface of tests/cartpole_reference.CartPoleSerial.

Every operation is one numpy float64 scalar `+ - * /` (or np.rint, or a sign flip) in the order the device code spells it, and the
start states come from oracle.c_oracle.philox4x32_10 — counter (global env, episode, 0, 0), key (seed lo, 0x4143 ^ seed hi), value i =
-0.1 + 0.2 * (word i * 2^-32) — so the device must agree with it bit for bit.  `libm=True` swaps in gymnasium's own spelling of the
step (its `_dsdt` and `rk4` with every constant, math.sin / math.cos): the yardstick of the polynomials and of the device's order.
The walker counts what it met: wraps in each direction, clamps of each velocity, height terminals, time-limit terminals."""
import math

import numpy as np

F = np.float64
PI = F(math.pi)
TWO_PI = F(2.0) * PI
HALF_PI = PI / F(2.0)
MAX_VEL_1, MAX_VEL_2 = F(4.0) * PI, F(9.0) * PI
DT = F(0.2)
HALF_DT, SIXTH_DT = DT / F(2.0), DT / F(6.0)
WRAPS = 64                                 # turns of each wrap loop at the most (kAcroWraps)
TWO_OVER_PI, C1, C2 = F(0.63661977236758138), F(1.5707963267341256), F(6.0771005065061922e-11)
SIN_COEF = [F(1.0) / F(355687428096000.0), F(-1.0) / F(1307674368000.0), F(1.0) / F(6227020800.0), F(-1.0) / F(39916800.0),
            F(1.0) / F(362880.0), F(-1.0) / F(5040.0), F(1.0) / F(120.0), F(-1.0) / F(6.0), F(1.0)]
COS_COEF = [F(1.0) / F(20922789888000.0), F(-1.0) / F(87178291200.0), F(1.0) / F(479001600.0), F(-1.0) / F(3628800.0),
            F(1.0) / F(40320.0), F(-1.0) / F(720.0), F(1.0) / F(24.0), F(-1.0) / F(2.0), F(1.0)]
G49, G147 = F(0.5) * F(9.8), F(1.5) * F(9.8)


def poly_sincos(x):
    """csrc/f64_sincos.hpp: quadrant k = rint(x * 2 / pi), r = (x - k C1) - k C2, Horner in r^2 through r^17 / r^16, select by k & 3."""
    x = F(x)
    k = np.rint(x * TWO_OVER_PI)
    r = (x - k * C1) - k * C2
    z = r * r
    p = SIN_COEF[0]
    for c in SIN_COEF[1:]:
        p = p * z + c
    s = r * p
    q = COS_COEF[0]
    for c in COS_COEF[1:]:
        q = q * z + c
    n = int(k) & 3
    a, b = (q, s) if n & 1 else (s, q)
    return (-a if n & 2 else a), (-b if (n + 1) & 2 else b)


def libm_sincos(x):
    return F(math.sin(x)), F(math.cos(x))


def dsdt(th1, th2, w1, w2, torque, sincos=poly_sincos):
    """acrobot_dsdt of the device: gymnasium's _dsdt with the products by 1 dropped -> (ddth1, ddth2)."""
    s2, c2 = sincos(th2)
    c12 = sincos((th1 + th2) - HALF_PI)[1]
    c1 = sincos(th1 - HALF_PI)[1]
    d1 = ((F(0.25) + (F(1.25) + c2)) + F(1.0)) + F(1.0)
    d2 = (F(0.25) + F(0.5) * c2) + F(1.0)
    phi2 = G49 * c12
    phi1 = (((F(-0.5) * (w2 * w2)) * s2 - (w2 * w1) * s2) + G147 * c1) + phi2
    a2 = (((torque + (d2 / d1) * phi1) - (F(0.5) * (w1 * w1)) * s2) - phi2) / (F(1.25) - (d2 * d2) / d1)
    a1 = -((d2 * a2 + phi1) / d1)
    return a1, a2


def rk4(state, action, sincos=poly_sincos):
    """acrobot_advance's rolled RK4 loop -> the unwrapped, unclamped (th1, th2, w1, w2)."""
    torque = F(action - 1)
    y = [F(v) for v in state]
    k = [F(0.0)] * 4
    g = [F(0.0)] * 4
    for i in range(4):
        h = F(0.0) if i == 0 else (DT if i == 3 else HALF_DT)
        wgt = F(1.0) if i in (0, 3) else F(2.0)
        ys = [y[j] + h * k[j] for j in range(4)]
        a1, a2 = dsdt(ys[0], ys[1], ys[2], ys[3], torque, sincos)
        k = [ys[2], ys[3], a1, a2]
        g = [g[j] + wgt * k[j] for j in range(4)]
    return [y[j] + SIXTH_DT * g[j] for j in range(4)]


def gym_step(state, action):
    """gymnasium AcrobotEnv.step's integration in its own spelling (book equations, Python floats, math.sin / math.cos)."""
    from math import cos, pi, sin
    m1 = m2 = l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    a = float(action - 1)

    def f(s):
        theta1, theta2, dtheta1, dtheta2 = s
        d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * cos(theta2)) + I1 + I2
        d2 = m2 * (lc2 ** 2 + l1 * lc2 * cos(theta2)) + I2
        phi2 = m2 * lc2 * g * cos(theta1 + theta2 - pi / 2.0)
        phi1 = (-m2 * l1 * lc2 * dtheta2 ** 2 * sin(theta2) - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * sin(theta2)
                + (m1 * lc1 + m2 * l1) * g * cos(theta1 - pi / 2) + phi2)
        ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 ** 2 * sin(theta2) - phi2) / (m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
        ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
        return np.array([dtheta1, dtheta2, ddtheta1, ddtheta2])
    y0 = np.array([float(v) for v in state])
    dt = 0.2
    dt2 = dt / 2.0
    k1 = f(y0)
    k2 = f(y0 + dt2 * k1)
    k3 = f(y0 + dt2 * k2)
    k4 = f(y0 + dt * k3)
    return list(y0 + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4))


class AcrobotSerial:
    """pufferlib.vector.Serial over N acrobots behind GymnasiumPufferEnv + EpisodeStats, restated (reset stream: Philox)."""

    def __init__(self, num_envs, max_steps=500, velocities=True, env_offset=0, libm=False):
        self.n, self.max_steps, self.velocities, self.env_offset = int(num_envs), int(max_steps), bool(velocities), int(env_offset)
        self.num_envs = self.n
        self.libm = bool(libm)
        self.sincos = libm_sincos if libm else poly_sincos
        self.observations = np.zeros((self.n, 6), np.float32)       # (what oracle.ppo_torch.Trainer sizes its rows from)
        self.agent_ids = np.arange(self.n)
        self.counts = dict(wrap_up=0, wrap_down=0, clamp1=0, clamp2=0, height=0, limit=0)   # wrap_down: th > pi came down by 2 pi

    def _draw(self, e):
        from oracle import c_oracle
        ctr = [(self.env_offset + e) & 0xFFFFFFFF, int(self.episode[e]) & 0xFFFFFFFF, 0, 0]
        w = c_oracle.philox4x32_10(ctr, [self.seed & 0xFFFFFFFF, 0x4143 ^ ((self.seed >> 32) & 0xFFFFFFFF)])
        self.state[e] = [F(-0.1) + F(0.2) * (F(int(w[i])) * F(2.0 ** -32)) for i in range(4)]

    def async_reset(self, seed=0):
        n = self.n
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.episode = np.zeros(n, np.int64)
        self.tick = np.zeros(n, np.int64)
        self.done = np.zeros(n, bool)
        self.ep_length = np.zeros(n, np.int64)
        self.ep_return = [0.0] * n
        self.state = np.zeros((n, 4), np.float64)
        for e in range(n):
            self._draw(e)
        self.rewards = np.zeros(n, np.float32)
        self.terminals = np.zeros(n, bool)
        self.truncations = np.zeros(n, bool)
        self.masks = np.ones(n, bool)
        self.infos = []
        self.sums = np.zeros(4, np.float64)     # count, sum of returns, of lengths, of scores

    def _wrap(self, x):
        for _ in range(WRAPS):
            if not x > PI:
                break
            x = x - TWO_PI
            self.counts['wrap_down'] += 1
        for _ in range(WRAPS):
            if not x < -PI:
                break
            x = x + TWO_PI
            self.counts['wrap_up'] += 1
        return x

    def _clamp(self, w, limit, name):
        if w < -limit or w > limit:
            self.counts[name] += 1
        w = -limit if w < -limit else w
        return limit if w > limit else w

    def send(self, actions):
        actions = np.asarray(actions).reshape(self.n)
        self.infos = []
        for e in range(self.n):
            if self.done[e]:                      # the auto-reset row: the action is ignored
                self.episode[e] += 1
                self.tick[e] = 0
                self.done[e] = False
                self.ep_length[e] = 0
                self.ep_return[e] = 0.0
                self._draw(e)
                self.rewards[e] = 0.0
                self.terminals[e] = False
                continue
            y = gym_step(self.state[e], int(actions[e])) if self.libm else rk4(self.state[e], int(actions[e]))
            th1, th2 = self._wrap(F(y[0])), self._wrap(F(y[1]))
            w1, w2 = self._clamp(F(y[2]), MAX_VEL_1, 'clamp1'), self._clamp(F(y[3]), MAX_VEL_2, 'clamp2')
            self.state[e] = [th1, th2, w1, w2]
            c1 = self.sincos(th1)[1]
            c12 = self.sincos(th1 + th2)[1]
            up = bool(-c1 - c12 > F(1.0))
            r = 0.0 if up else -1.0
            self.tick[e] += 1
            self.ep_length[e] += 1
            self.ep_return[e] = self.ep_return[e] + r
            self.rewards[e] = r
            limit = self.max_steps > 0 and int(self.tick[e]) == self.max_steps
            t = up or limit
            self.counts['height'] += int(up)
            self.counts['limit'] += int(limit and not up)
            self.terminals[e] = self.done[e] = t
            if t:
                self.infos.append(dict(episode_return=self.ep_return[e], episode_length=int(self.ep_length[e]), score=self.ep_return[e]))
                self.sums += [1.0, self.ep_return[e], float(self.ep_length[e]), self.ep_return[e]]

    def obs(self):
        o = np.zeros((self.n, 6), np.float32)
        for e in range(self.n):
            s1, c1 = self.sincos(self.state[e, 0])
            s2, c2 = self.sincos(self.state[e, 1])
            o[e] = [np.float32(c1), np.float32(s1), np.float32(c2), np.float32(s2), np.float32(self.state[e, 2]), np.float32(self.state[e, 3])]
        if not self.velocities:
            o[:, 4:] = 0.0
        return o

    def recv(self):
        return (self.obs(), self.rewards.copy(), self.terminals.copy(), self.truncations.copy(), self.infos, self.agent_ids, self.masks.copy())

    def states(self):
        """([N][4] float64 state, [N][4] int32 (episode, tick, done, ep_length)) — what vector.Acrobot.debug_states() returns."""
        return self.state.copy(), np.stack([self.episode, self.tick, self.done.astype(np.int64), self.ep_length], 1).astype(np.int32)

    def set_states(self, states, counters):
        """What vector.Acrobot.debug_set_states() does: every env becomes an episode ep_length steps old (return -ep_length) in the
        given state; the live rewards and the statistics stay, the live terminal flag follows `done`."""
        states, counters = np.asarray(states, np.float64), np.asarray(counters, np.int64)
        assert states.shape == (self.n, 4) and counters.shape == (self.n, 4)
        self.state = states.copy()
        self.episode, self.tick, self.ep_length = counters[:, 0].copy(), counters[:, 1].copy(), counters[:, 3].copy()
        self.done = counters[:, 2] != 0
        self.terminals = self.done.copy()
        self.ep_return = [-float(x) for x in self.ep_length]


def pump_actions(state):
    """The scripted energy-pumping rule of the protocol tests: torque against the first link's velocity (action 0 where w1 > 0, else
    2).  From the start states it swings every one of 40 envs above the bar within 120 sends (tests/test_acrobot_cpu.py)."""
    return np.where(np.asarray(state)[:, 2] > 0, 0, 2).astype(np.int64)


def branch_states(states, counters, max_steps):
    """Copies of (states, counters) of at least 16 envs with envs 0..15 put on the rare branches of the step: an angle just inside +-pi
    with a velocity that carries it across (0..3), a velocity at its clamp and still accelerating (4..7), a state one step below
    the height threshold (8, 9), an episode two steps from the time limit (10, 11; max_steps = 0: left alone), and mixtures (12..15)."""
    s, c = np.array(states, np.float64), np.array(counters, np.int64)
    pi = math.pi
    s[:16] = [[pi - 0.05, 0.0, 3.0, 0.0], [-pi + 0.05, 0.0, -3.0, 0.0], [0.3, pi - 0.05, 0.0, 5.0], [-0.3, -pi + 0.05, 0.0, -5.0],
              [1.5, 0.0, 4 * pi, 0.0], [-1.5, 0.0, -4 * pi, 0.0], [0.0, 1.0, -6.0, 9 * pi], [0.0, -1.0, 6.0, -9 * pi],
              [2.0, 0.0, 2.0, 0.0], [-2.0, 0.1, -2.0, 0.0], [0.05, -0.05, 0.1, -0.1], [-0.05, 0.05, -0.1, 0.1],
              [pi, -pi, 4 * pi, -9 * pi], [-pi, pi, -4 * pi, 9 * pi], [3.0, 3.0, 12.0, 28.0], [-3.0, -3.0, -12.0, -28.0]]
    c[:16, 2] = 0
    c[:16, 1] = c[:16, 3] = 3
    if max_steps > 0:
        c[10:12, 1] = c[10:12, 3] = max_steps - 2
    return s, c
