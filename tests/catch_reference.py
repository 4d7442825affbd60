"""CPU restatement of vector.PixelCatch (csrc/catch_env.hpp, csrc/pixel_catch.hip) for the tests: a numpy integer walker over N envs —
the Philox start draw, one send, the frame painter — that the device must agree with bit for bit."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, k0, k1):
    """Philox4x32-10 of counters (c0, c1, 0, 0) (uint64 arrays holding 32-bit values) under key (k0, k1) -> the four output words."""
    c = [np.asarray(c0, np.uint64) & M32, np.asarray(c1, np.uint64) & M32, np.zeros_like(c0, np.uint64), np.zeros_like(c0, np.uint64)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


class CatchWalker:
    def __init__(self, num_envs, rows, cols, framestack, height, width, channels_last, env_offset=0):
        self.n, self.rows, self.cols, self.stack = num_envs, rows, cols, framestack
        self.height, self.width, self.channels_last, self.env_offset = height, width, channels_last, env_offset

    def _begin(self, mask):
        """Envs `mask` begin their next episode: every history slot holds the start state."""
        self.episode[mask] += 1
        self.ep_length[mask] = 0
        env = np.arange(self.n, dtype=np.uint64) + np.uint64(self.env_offset)
        w = [(x % np.uint64(m)).astype(np.int64) for x, m in zip(philox4x32_10(env, self.episode.astype(np.uint64), self.seed & 0xFFFFFFFF,
                                                                                 0x5043 ^ (self.seed >> 32)), (self.cols, 3, self.cols))]
        self.hist[mask] = np.stack([np.zeros(self.n, np.int64), w[0], w[2]], 1)[mask, None, :]
        self.vx[mask] = w[1][mask] - 1

    def async_reset(self, seed):
        n, self.seed = self.n, int(seed) & 0xFFFFFFFFFFFFFFFF
        self.episode, self.ep_length, self.vx = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.hist = np.zeros((n, 4, 3), np.int64)       # [env][sends ago] = (ball row, ball column, paddle column)
        self._begin(np.ones(n, bool))
        self.rewards, self.terminals = np.zeros(n, np.float32), np.zeros(n, bool)
        self.infos, self.sums = [], np.zeros(4, np.float64)     # count, sum of returns, of lengths, of scores

    def send(self, actions):
        r, c, p = self.hist[:, 0].T
        p = np.clip(p + np.asarray(actions) - 1, 0, self.cols - 1)
        self.vx = np.where((c + self.vx < 0) | (c + self.vx >= self.cols), -self.vx, self.vx)
        c, r = c + self.vx, r + 1
        self.hist = np.concatenate([np.stack([r, c, p], 1)[:, None], self.hist[:, :3]], 1)
        self.ep_length += 1
        self.terminals = r == self.rows - 1
        self.rewards = np.where(self.terminals, np.where(c == p, 1.0, -1.0), 0.0).astype(np.float32)
        self.infos = [dict(episode_return=float(self.rewards[e]), episode_length=int(self.ep_length[e]), score=float(c[e] == p[e]))
                      for e in np.nonzero(self.terminals)[0]]
        for i in self.infos:
            self.sums += [1.0, i['episode_return'], i['episode_length'], i['score']]
        self._begin(self.terminals)

    def frames(self):
        cy, cx = (np.arange(self.height) * self.rows // self.height)[:, None], (np.arange(self.width) * self.cols // self.width)[None, :]
        planes = []
        for k in range(self.stack):       # channel k: the state stack-1-k sends ago
            r, c, p = (self.hist[:, self.stack - 1 - k, i][:, None, None] for i in range(3))
            planes.append(np.where((cy == r) & (cx == c), 255, np.where((cy == self.rows - 1) & (cx == p), 128, 0)).astype(np.uint8))
        return np.stack(planes, -1 if self.channels_last else 1)

    def states(self):       # what vector.PixelCatch.debug_states() returns
        return self.hist[:, :self.stack].astype(np.int32), np.stack([self.vx, self.episode, self.ep_length], 1).astype(np.int32)
