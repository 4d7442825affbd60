"""vector.CartPole without a GPU: the numpy walker of tests/cartpole_reference.py (the device kernels' oracle) against libm and
against its own protocol semantics, the random-policy baseline of the learning tests, how the trainer rolls the class out, and the
host-side refusals of the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cartpole_reference as cr  # noqa: E402

# measured here (figures in the docstrings of the two tests); the assertions stand at 10 x the measured maximum
SIN_MAX, COS_MAX, WALK_MAX = 2.7755575615628914e-17, 1.1102230246251565e-16, 4.6629367034256575e-15
RANDOM_BASELINE = 22.397      # mean episode length of a uniformly random policy, measured below over 2000 episodes


def test_polynomial_sin_cos_against_libm():
    """The walker's (= the device's) Horner polynomials against math.sin / math.cos on 200001 points of |theta| <= 0.21 (the 12
    degree threshold is 0.2094).  Measured: max |sin difference| 2.78e-17, max |cos difference| 1.11e-16 — half an ulp of the result
    each, i.e. the polynomial is never further from libm than one rounding (it differs from it on 18 % / 0.6 % of the points)."""
    grid = np.linspace(-0.21, 0.21, 200001)
    ds = max(abs(float(cr.poly_sincos(t)[0]) - math.sin(t)) for t in grid)
    dc = max(abs(float(cr.poly_sincos(t)[1]) - math.cos(t)) for t in grid)
    print('polynomial vs libm: sin', ds, 'cos', dc)
    assert ds <= 10 * SIN_MAX and dc <= 10 * COS_MAX


def test_polynomial_walker_against_the_libm_walker():
    """gymnasium's formula (math.sin / math.cos) and the polynomial walker on the same 500 sends of random actions, 16 envs, seed 3
    (335 episodes each, with their reset rows): the same terminals on every send, and states at most 4.66e-15 apart (measured)."""
    n = 16
    a, b = cr.CartPoleSerial(n), cr.CartPoleSerial(n, libm=True)
    a.async_reset(3)
    b.async_reset(3)
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in range(500):
        act = rng.integers(0, 2, n)
        a.send(act)
        b.send(act)
        assert np.array_equal(a.terminals, b.terminals) and a.infos == b.infos, k
        worst = max(worst, float(np.abs(a.state - b.state).max()))
    print('walkers, polynomial vs libm: max |state difference|', worst, 'episodes', a.sums[0])
    assert a.sums[0] > 300 and worst <= 10 * WALK_MAX


def test_walker_semantics():
    n = 6
    w = cr.CartPoleSerial(n, max_steps=500)
    w.async_reset(7)
    o, r, te, tr, info, ids, m = w.recv()
    assert o.dtype == np.float32 and o.shape == (n, 4) and (np.abs(o) <= 0.05).all() and not r.any() and not te.any() and info == []
    assert len(np.unique(o)) == 4 * n                                   # four words per env, every env its own counter
    # one hand-written step of env 0 (action 1), in gymnasium's own spelling with libm: equal to within the polynomial's rounding
    x, xd, th, thd = (float(v) for v in w.state[0])
    temp = (10.0 + 0.05 * thd ** 2 * math.sin(th)) / 1.1
    thacc = (9.8 * math.sin(th) - math.cos(th) * temp) / (0.5 * (4.0 / 3.0 - 0.1 * math.cos(th) ** 2 / 1.1))
    xacc = temp - 0.05 * thacc * math.cos(th) / 1.1
    w.send(np.ones(n, np.int64))
    np.testing.assert_allclose(w.state[0], [x + 0.02 * xd, xd + 0.02 * xacc, th + 0.02 * thd, thd + 0.02 * thacc], rtol=0, atol=1e-15)
    # always pushing right: the pole falls over; reward 1 on the terminating step too, then the reset row
    lengths = np.zeros(n, int)                                           # of every env's first episode
    for k in range(2, 60):
        was_done, episode = w.done.copy(), w.episode.copy()
        w.send(np.ones(n, np.int64))
        o, r, te, tr, info, ids, m = w.recv()
        assert (r[~was_done] == 1.0).all() and not tr.any() and m.all(), k
        # the auto-reset row: reward 0, not terminal, the next episode's freshly drawn state
        assert not r[was_done].any() and not te[was_done].any() and (w.episode[was_done] == episode[was_done] + 1).all(), k
        assert (w.tick[was_done] == 0).all() and (np.abs(w.state[was_done]) <= 0.05).all(), k
        assert len(info) == te.sum() and all(i['episode_return'] == float(i['episode_length']) == i['score'] for i in info), k
        for e in np.nonzero(te)[0]:
            assert r[e] == 1.0 and w.tick[e] == w.ep_length[e] and (abs(w.state[e, 0]) > 2.4 or abs(w.state[e, 2]) > cr.THETA_LIMIT)
            if w.episode[e] == 0:
                lengths[e] = k
    assert lengths.all() and (lengths < 20).all() and w.sums[0] > 2 * n and w.sums[1] == w.sums[2] == w.sums[3]


def test_walker_time_limit_velocities_offset_and_seed():
    # max_steps: the step that makes the episode max_steps long is terminal (truncations stay 0), whatever the state
    w = cr.CartPoleSerial(4, max_steps=3)
    w.async_reset(0)
    alt = [np.array([k % 2] * 4) for k in range(8)]
    seen = []
    for k in range(8):
        w.send(alt[k])
        seen.append((w.terminals.copy(), w.rewards.copy(), [i['episode_length'] for i in w.infos]))
    assert [s[0].all() for s in seen] == [False, False, True, False, False, False, True, False] and not any(s[0].any() for s in seen[:2])
    assert seen[2][2] == [3] * 4 and (seen[2][1] == 1).all() and (seen[3][1] == 0).all() and not w.truncations.any()
    # max_steps = 0: no time limit
    free = cr.CartPoleSerial(1, max_steps=0)
    free.async_reset(0)
    for k in range(600):
        o = free.obs()[0]
        free.send([int(o[2] + 0.5 * o[3] + 0.02 * o[0] + 0.05 * o[1] > 0)])      # a hand-made balancing controller
        assert not free.terminals.any(), k
    assert free.tick[0] == 600
    # velocities=False: columns 1 and 3 read 0, the dynamics do not change
    full, masked = cr.CartPoleSerial(5), cr.CartPoleSerial(5, velocities=False)
    full.async_reset(2)
    masked.async_reset(2)
    rng = np.random.default_rng(2)
    for k in range(40):
        a = rng.integers(0, 2, 5)
        full.send(a)
        masked.send(a)
        of, om = full.recv()[0], masked.recv()[0]
        assert np.array_equal(of[:, [0, 2]], om[:, [0, 2]]) and not om[:, [1, 3]].any() and of[:, [1, 3]].all()
    assert np.array_equal(full.state, masked.state)
    # env_offset: envs 3.. of a larger vecenv; the same seed walks the same walk, another seed another
    big, part, again, other = cr.CartPoleSerial(7), cr.CartPoleSerial(4, env_offset=3), cr.CartPoleSerial(7), cr.CartPoleSerial(7)
    for v, s in ((big, 5), (part, 5), (again, 5), (other, 6)):
        v.async_reset(s)
    for k in range(60):
        a = rng.integers(0, 2, 7)
        for v in (big, again, other):
            v.send(a)
        part.send(a[3:])
        assert np.array_equal(big.state[3:], part.state) and np.array_equal(big.terminals[3:], part.terminals), k
    assert np.array_equal(big.state, again.state) and big.sums.tolist() == again.sums.tolist() and big.sums[0] > 7
    assert not np.array_equal(big.state, other.state)


def test_random_policy_baseline():
    """The walker under uniformly random actions, 64 envs, max_steps=500, seed 0, until 2000 episodes have ended: mean episode length
    22.397 (measured; gymnasium users know the figure as 'about 22').  The learning tests of tests/test_gpu_cartpole.py require their
    first rollout to lie within 2 x of it."""
    w = cr.CartPoleSerial(64)
    w.async_reset(0)
    rng = np.random.default_rng(0)
    while w.sums[0] < 2000:
        w.send(rng.integers(0, 2, 64))
    mean = w.sums[2] / w.sums[0]
    print('random-policy baseline: episodes', w.sums[0], 'mean length', mean)
    assert w.sums[0] >= 2000 and abs(mean - RANDOM_BASELINE) < 1e-9


def test_rollout_form_of_the_class_and_of_a_subclass():
    """(general, general + mlp_view, lstm, neither): CartPole declares the view rollout, the recurrent rollout and the flat one; a
    subclass inherits the latter two but not the view form, which reads the state layout of exactly the declaring class."""
    from pufferlib_amd import clean_pufferl as cp
    from pufferlib_amd import vector as v
    S, R, M = cp.STEPWISE, cp.FUSED_LSTM, cp.FUSED_MLP

    class CartPoleChild(v.CartPole):
        pass
    engines = [dict(gen_engine=True, lstm_engine=False, mlp_view=False), dict(gen_engine=True, lstm_engine=False, mlp_view=True),
               dict(gen_engine=False, lstm_engine=True, mlp_view=False), dict(gen_engine=False, lstm_engine=False, mlp_view=False)]
    for cls, want in ((v.CartPole, (S, M, R, M)), (CartPoleChild, (S, S, R, M)), (v.Tabular, (S, S, R, M)), (v.Squared, (S, M, R, M))):
        assert tuple(cp.rollout_form(cls, **kw) for kw in engines) == want, cls.__name__
    assert v.CartPole.SEEDED and v.env_creator('cartpole') is v.make_cartpole
    sp = v.make_cartpole()
    assert (sp.max_steps, sp.velocities) == (500, True) and sp.single_action_space.n == 2
    assert sp.single_observation_space.shape == (4,) and sp.single_observation_space.dtype == np.float32
    fmax = np.finfo(np.float32).max
    assert np.array_equal(sp.single_observation_space.high, np.array([4.8, fmax, 0.41887903, fmax], np.float32))
    assert np.array_equal(sp.single_observation_space.low, -sp.single_observation_space.high)
    from pufferlib_amd import demo
    assert demo.device_backend_for(v.make_cartpole) is v.CartPole


def test_state_bytes_refuses_bad_configurations_on_the_host():
    from pufferlib_amd import _lib
    _lib.build()
    L = _lib.lib()
    good = _lib.CartPoleConfig(40, 500, 1, 0, 0, 0)
    assert L.pfa_cartpole_state_bytes(C.byref(good)) >= 40 * (5 * 8 + 4 * 4)
    assert L.pfa_cartpole_state_bytes(C.byref(_lib.CartPoleConfig(40, 0, 0, 0, 0, 0))) == L.pfa_cartpole_state_bytes(C.byref(good))
    for n in (0, -3):
        assert L.pfa_cartpole_state_bytes(C.byref(_lib.CartPoleConfig(n, 500, 1, 0, 0, 0))) == 0
        assert b'cartpole: num_envs' in L.pfa_last_error()
    assert L.pfa_cartpole_state_bytes(C.byref(_lib.CartPoleConfig(40, -1, 1, 0, 0, 0))) == 0
    assert b'cartpole: max_steps' in L.pfa_last_error()
    assert L.pfa_cartpole_state_bytes(None) == 0 and b'null config' in L.pfa_last_error()
