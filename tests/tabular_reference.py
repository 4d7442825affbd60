"""CPU restatement of vector.Tabular (csrc/tabular_env.hpp) for the tests: a numpy walker of a vector.TabularMDP speaking the Serial
protocol (async_reset / recv / send, infos, auto-reset rows), Stochastic-as-a-table, and value iteration for the builders.

The walker draws its words with oracle.c_oracle.philox4x32_10 — counter (global env, episode, tick, domain), key (seed lo,
0x5442 ^ seed hi), word 0; domain 0 = start draw, 1 = transition — and reads the MDP object's own uint32 thresholds through
TabularMDP.outcome, so it cannot disagree with the device about what a probability means."""
import numpy as np


def stochastic_as_table(p=0.7, horizon=100):
    """ocean.Stochastic (ocean.py:529-582) written as a table: state = tick * (H + 1) + count of action 0, two actions, one outcome
    each, observation always [0.0]; the reward of a move is the reference's Python expression evaluated at the state it leads to,
    the score of a state its proximity; the states of tick H are terminal."""
    from pufferlib_amd import vector
    H = int(horizon)
    W = H + 1
    S = W * W
    nxt = np.zeros((S, 2), np.int32)
    reward = np.zeros((S, 2), np.float64)
    score = np.zeros(S, np.float64)
    terminal = np.zeros(S, bool)
    for tick in range(W):
        for count in range(W):
            s = tick * W + count
            terminal[s] = tick == H
            if tick > 0 and count <= tick:
                score[s] = 1 - (p - count / tick) ** 2
            for a in (0, 1):
                if tick == H or count + (a == 0) > H:
                    nxt[s, a] = s
                    continue
                t2, c2 = tick + 1, count + (a == 0)
                nxt[s, a] = t2 * W + c2
                frac = c2 / t2
                proximity = 1 - (p - frac) ** 2
                reward[s, a] = proximity if ((a == 0 and frac < p) or (a == 1 and frac >= p)) else 0
    return vector.TabularMDP(nxt, reward=reward, terminal=terminal, obs=np.zeros((S, 1), np.float32), start=0, horizon=H, score=score)


class TabularSerial:
    """pufferlib.vector.Serial over N copies of one TabularMDP behind GymnasiumPufferEnv + EpisodeStats, restated."""

    def __init__(self, mdp, num_envs, env_offset=0):
        self.mdp, self.n, self.env_offset = mdp, int(num_envs), int(env_offset)
        self.num_envs = self.n
        self.observations = np.zeros((self.n, mdp.obs_dim), np.float32)       # (what oracle.ppo_torch.Trainer sizes its rows from)
        self.agent_ids = np.arange(self.n)

    def word(self, env, episode, tick, domain):
        from oracle import c_oracle
        ctr = [(self.env_offset + env) & 0xFFFFFFFF, episode & 0xFFFFFFFF, tick & 0xFFFFFFFF, domain]
        return int(c_oracle.philox4x32_10(ctr, [self.seed & 0xFFFFFFFF, 0x5442 ^ ((self.seed >> 32) & 0xFFFFFFFF)])[0])

    def _start(self, e):
        m = self.mdp
        if m.num_starts == 1:
            return int(m.start_states[0])
        return int(m.start_states[m.outcome(m.start_cum, self.word(e, int(self.episode[e]), 0, 0))])

    def async_reset(self, seed=0):
        m, n = self.mdp, self.n
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.episode = np.zeros(n, np.int64)
        self.tick = np.zeros(n, np.int64)
        self.done = np.zeros(n, bool)
        self.ep_length = np.zeros(n, np.int64)
        self.ep_return = [0.0] * n
        self.state = np.array([self._start(e) for e in range(n)], np.int64)
        self.rewards = np.zeros(n, np.float32)
        self.terminals = np.zeros(n, bool)
        self.truncations = np.zeros(n, bool)
        self.masks = np.ones(n, bool)
        self.infos = []
        self.sums = np.zeros(4, np.float64)     # count, sum of returns, of lengths, of scores

    def send(self, actions):
        m = self.mdp
        actions = np.asarray(actions).reshape(self.n)
        self.infos = []
        for e in range(self.n):
            if self.done[e]:                      # the auto-reset row (vector.py:144-151): the action is ignored
                self.episode[e] += 1
                self.tick[e] = 0
                self.done[e] = False
                self.ep_length[e] = 0
                self.ep_return[e] = 0.0
                self.state[e] = self._start(e)
                self.rewards[e] = 0.0
                self.terminals[e] = False
                continue
            s, a = int(self.state[e]), int(actions[e])
            k = 0
            if m.num_outcomes > 1:
                k = m.outcome(m.cum[s, a], self.word(e, int(self.episode[e]), int(self.tick[e]), 1))
            s2, r = int(m.next_state[s, a, k]), float(m.reward[s, a, k])
            self.state[e] = s2
            self.tick[e] += 1
            self.ep_length[e] += 1
            self.ep_return[e] += r                # Python floats: f64 sum in order (postprocess.py:39-41)
            self.rewards[e] = np.float32(r)       # the buffer write (emulation.py:219)
            t = bool(m.terminal[s2]) or int(self.tick[e]) == m.horizon
            self.terminals[e] = self.done[e] = t
            if t:
                score = float(m.score[s2]) if m.score is not None else self.ep_return[e]
                self.infos.append(dict(episode_return=self.ep_return[e], episode_length=int(self.ep_length[e]), score=score))
                self.sums += [1.0, self.ep_return[e], float(self.ep_length[e]), score]

    def recv(self):
        return (self.mdp.obs[self.state].copy(), self.rewards.copy(), self.terminals.copy(), self.truncations.copy(), self.infos,
                self.agent_ids, self.masks.copy())

    def states(self):
        """[N][5]: (state, episode, tick, done, ep_length) — what vector.Tabular.debug_states() returns."""
        return np.stack([self.state, self.episode, self.tick, self.done.astype(np.int64), self.ep_length], 1).astype(np.int32)


def reachable(mdp):
    """Boolean [S]: states some positive-probability path from a start state visits (outcomes with non-zero threshold mass only)."""
    cum = mdp.cum.astype(np.int64)
    mass = np.diff(np.concatenate([np.zeros(cum.shape[:2] + (1,), np.int64), cum], 2), axis=2) > 0
    smass = np.diff(np.concatenate([[0], mdp.start_cum.astype(np.int64)])) > 0
    seen = np.zeros(mdp.num_states, bool)
    todo = [int(s) for s in mdp.start_states[smass]]
    seen[todo] = True
    while todo:
        s = todo.pop()
        if mdp.terminal[s]:
            continue
        for s2 in np.unique(mdp.next_state[s][mass[s]]):
            if not seen[s2]:
                seen[s2] = True
                todo.append(int(s2))
    return seen


def optimal_score(mdp):
    """The largest expected infos['score'] a (state-aware, time-aware) policy reaches: finite-horizon value iteration in float64 on
    the MDP's own probabilities.  Without a score table the score is the episode's return."""
    S = mdp.num_states
    p, nxt = mdp.prob, mdp.next_state
    live = ~mdp.terminal[nxt]                                    # [S][A][K]: the episode goes on after this outcome
    value = np.zeros(S, np.float64)                              # 0 steps left
    for j in range(1, mdp.horizon + 1):
        if mdp.score is None:
            q = (p * (mdp.reward + np.where(live & (j > 1), value[nxt], 0.0))).sum(2)
        else:
            q = (p * np.where(live & (j > 1), value[nxt], mdp.score[nxt])).sum(2)
        value = q.max(1)
    return float((mdp.start_prob * value[mdp.start_states]).sum())
