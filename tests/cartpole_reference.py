"""CPU restatement of vector.CartPole (csrc/cartpole_env.hpp) for the tests: a numpy float64 walker speaking the Serial protocol
(async_reset / recv / send, infos, auto-reset rows), with the interface of tests/tabular_reference.TabularSerial.

Every operation is one numpy float64 scalar `+ - * /` in the order the device code spells it, sin and cos are the same Horner
polynomials in theta^2, and the start states come from oracle.c_oracle.philox4x32_10 — counter (global env, episode, 0, 0), key
(seed lo, 0x4350 ^ seed hi), value i = -0.05 + 0.1 * (word i * 2^-32) — so the device must agree with it bit for bit.
`libm=True` swaps the polynomials for math.sin / math.cos: gymnasium's formula, the yardstick of the polynomials."""
import math

import numpy as np

F = np.float64
GRAVITY, TOTAL_MASS, POLE_MASS, LENGTH, POLEMASS_LENGTH, FORCE_MAG, TAU = F(9.8), F(1.1), F(0.1), F(0.5), F(0.05), F(10.0), F(0.02)
X_LIMIT = F(2.4)
THETA_LIMIT = F(12 * 2 * math.pi / 360)
SIN_COEF = [F(1.0) / F(6227020800.0), F(-1.0) / F(39916800.0), F(1.0) / F(362880.0), F(-1.0) / F(5040.0), F(1.0) / F(120.0), F(-1.0) / F(6.0), F(1.0)]
COS_COEF = [F(1.0) / F(479001600.0), F(-1.0) / F(3628800.0), F(1.0) / F(40320.0), F(-1.0) / F(720.0), F(1.0) / F(24.0), F(-1.0) / F(2.0), F(1.0)]


def poly_sincos(theta):
    """sin / cos as Horner polynomials in z = theta^2, through theta^13 / theta^12 (|theta| <= 0.21: the first dropped term < 1e-20)."""
    theta = F(theta)
    z = theta * theta
    p = SIN_COEF[0]
    for c in SIN_COEF[1:]:
        p = p * z + c
    q = COS_COEF[0]
    for c in COS_COEF[1:]:
        q = q * z + c
    return theta * p, q


def libm_sincos(theta):
    return F(math.sin(theta)), F(math.cos(theta))


def physics(x, x_dot, theta, theta_dot, action, sincos=poly_sincos):
    """One explicit-Euler step (gymnasium CartPoleEnv.step, kinematics_integrator 'euler') -> the new (x, x_dot, theta, theta_dot)."""
    force = FORCE_MAG if action == 1 else -FORCE_MAG
    sn, cs = sincos(theta)
    temp = (force + POLEMASS_LENGTH * (theta_dot * theta_dot) * sn) / TOTAL_MASS
    thetaacc = (GRAVITY * sn - cs * temp) / (LENGTH * (F(4.0) / F(3.0) - POLE_MASS * (cs * cs) / TOTAL_MASS))
    xacc = temp - POLEMASS_LENGTH * thetaacc * cs / TOTAL_MASS
    return x + TAU * x_dot, x_dot + TAU * xacc, theta + TAU * theta_dot, theta_dot + TAU * thetaacc


class CartPoleSerial:
    """pufferlib.vector.Serial over N cart-poles behind GymnasiumPufferEnv + EpisodeStats, restated (reset stream: Philox)."""

    def __init__(self, num_envs, max_steps=500, velocities=True, env_offset=0, libm=False):
        self.n, self.max_steps, self.velocities, self.env_offset = int(num_envs), int(max_steps), bool(velocities), int(env_offset)
        self.num_envs = self.n
        self.sincos = libm_sincos if libm else poly_sincos
        self.observations = np.zeros((self.n, 4), np.float32)       # (what oracle.ppo_torch.Trainer sizes its rows from)
        self.agent_ids = np.arange(self.n)

    def _draw(self, e):
        from oracle import c_oracle
        ctr = [(self.env_offset + e) & 0xFFFFFFFF, int(self.episode[e]) & 0xFFFFFFFF, 0, 0]
        w = c_oracle.philox4x32_10(ctr, [self.seed & 0xFFFFFFFF, 0x4350 ^ ((self.seed >> 32) & 0xFFFFFFFF)])
        self.state[e] = [F(-0.05) + F(0.1) * (F(int(w[i])) * F(2.0 ** -32)) for i in range(4)]

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
            x, x_dot, theta, theta_dot = physics(*self.state[e], int(actions[e]), self.sincos)
            self.state[e] = [x, x_dot, theta, theta_dot]
            self.tick[e] += 1
            self.ep_length[e] += 1
            self.ep_return[e] += 1.0
            self.rewards[e] = 1.0                 # on the terminating step too
            t = bool(x < -X_LIMIT or x > X_LIMIT or theta < -THETA_LIMIT or theta > THETA_LIMIT
                     or (self.max_steps > 0 and int(self.tick[e]) == self.max_steps))
            self.terminals[e] = self.done[e] = t
            if t:
                self.infos.append(dict(episode_return=self.ep_return[e], episode_length=int(self.ep_length[e]), score=self.ep_return[e]))
                self.sums += [1.0, self.ep_return[e], float(self.ep_length[e]), self.ep_return[e]]

    def obs(self):
        o = self.state.astype(np.float32)
        if not self.velocities:
            o[:, [1, 3]] = 0.0
        return o

    def recv(self):
        return (self.obs(), self.rewards.copy(), self.terminals.copy(), self.truncations.copy(), self.infos, self.agent_ids, self.masks.copy())

    def states(self):
        """([N][4] float64 state, [N][4] int32 (episode, tick, done, ep_length)) — what vector.CartPole.debug_states() returns."""
        return self.state.copy(), np.stack([self.episode, self.tick, self.done.astype(np.int64), self.ep_length], 1).astype(np.int32)
