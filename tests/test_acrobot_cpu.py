"""vector.Acrobot without a GPU: the numpy walker of tests/acrobot_reference.py (the device kernels' oracle) against libm and against
its own protocol semantics, the scripted inputs of the GPU protocol test, the random-policy baseline of the learning tests, how the
trainer rolls the class out, and the host-side refusals of the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import acrobot_reference as ar  # noqa: E402

# measured here (figures in the docstrings of the two tests): sin and cos 1.11e-16 from libm, asserted at the issue's 1e-15; one step of the
# polynomial walker 2.12e-12 from gymnasium's spelling with libm — a decade over that would be 2.1e-11, so the issue's cap of 1e-11 holds
STEP_BOUND = 1e-11
RANDOM_BASELINE = 498.109375              # mean episode length of a uniformly random policy, measured below over 64 episodes
BOX = np.array([math.pi, math.pi, 4 * math.pi, 9 * math.pi])


def test_polynomial_sin_cos_against_libm():
    """The walker's (= the device's) quadrant reduction + Horner polynomials against math.sin / math.cos on 400001 points of [-8, 8]
    and on k pi / 4 -+ 0 .. 4 ulps for k = -11 .. 11.  Measured: max |difference| 1.11e-16 for sin and for cos, on the grid and at the
    boundaries alike: half an ulp of a result near 1, i.e. never further from libm than one rounding.  The bound is the issue's 1e-15."""
    pts = list(np.linspace(-8.0, 8.0, 400001))
    for k in range(-11, 12):
        for u in range(-4, 5):
            y = np.float64(k * math.pi / 4)
            for _ in range(abs(u)):
                y = np.nextafter(y, np.inf if u > 0 else -np.inf)
            pts.append(y)
    ds = max(abs(float(ar.poly_sincos(t)[0]) - math.sin(t)) for t in pts)
    dc = max(abs(float(ar.poly_sincos(t)[1]) - math.cos(t)) for t in pts)
    print('polynomial vs libm on [-8, 8]: sin', ds, 'cos', dc)
    assert ds <= 1e-15 and dc <= 1e-15
    # every quadrant's selection and sign, and the reduction constants: C1 + C2 is pi / 2 beyond f64
    for k in range(-8, 9):
        s, c = ar.poly_sincos(k * math.pi / 2 + 0.3)
        assert abs(float(s) - math.sin(k * math.pi / 2 + 0.3)) < 1e-15 and abs(float(c) - math.cos(k * math.pi / 2 + 0.3)) < 1e-15, k
    assert float(ar.C1) + float(ar.C2) == math.pi / 2
    assert (float(ar.C1) * 2.0 ** 32) % 1.0 == 0.0                      # 33 significant bits: k * C1 is exact for |k| < 2^20


def _one_step(states, action, libm):
    n = len(states)
    w = ar.AcrobotSerial(n, libm=libm)
    w.async_reset(0)
    w.set_states(states, np.zeros((n, 4), np.int64))
    w.send(np.full(n, action))
    return w


def test_one_step_of_the_polynomial_walker_against_gymnasiums_spelling_with_libm():
    """1000 states uniform in the state box (numpy default_rng(0)) x 3 actions: one step of the walker in the device's spelling (rolled
    RK4 loop, products by 1 dropped, polynomial sin / cos) against one step in gymnasium's own spelling with math.sin / math.cos, wrap
    and clamp included.  Single steps, not trajectories: the system is chaotic.  Measured: the largest difference of a state value is
    2.12e-12 (action 0, w1 of the state (0.108, -2.112, -10.51, -26.34): velocities near their clamps, where the right-hand side is
    of the order 10^3 and a rounding of sin is amplified accordingly; 99.9 % of the states differ by less than 3e-13, half of them not
    at all), 1.4e-13 and 1.1e-13 for actions 1 and 2; the terminals agree everywhere.  A decade over the measured maximum would be
    2.1e-11, looser than the issue allows, so the assertion stands at its cap of 1e-11."""
    rng = np.random.default_rng(0)
    states = rng.uniform(-BOX, BOX, (1000, 4))
    worst = 0.0
    for action in range(3):
        p, g = _one_step(states, action, False), _one_step(states, action, True)
        assert np.array_equal(p.terminals, g.terminals) and np.array_equal(p.rewards, g.rewards), action
        d = float(np.abs(p.state - g.state).max())
        print('one step, polynomial vs libm, action', action, 'max |state difference|', d, p.counts)
        worst = max(worst, d)
        assert min(p.counts[k] for k in ('wrap_up', 'wrap_down', 'clamp1', 'clamp2', 'height')) > 50      # the box reaches every branch
    assert worst <= STEP_BOUND


def test_walker_semantics():
    n = 6
    w = ar.AcrobotSerial(n, max_steps=500)
    w.async_reset(7)
    o, r, te, tr, info, ids, m = w.recv()
    assert o.dtype == np.float32 and o.shape == (n, 6) and not r.any() and not te.any() and info == []
    assert (np.abs(w.state) <= 0.1).all() and len(np.unique(w.state)) == 4 * n            # four words per env, every env its own counter
    np.testing.assert_allclose(o, np.stack([np.cos(w.state[:, 0]), np.sin(w.state[:, 0]), np.cos(w.state[:, 1]), np.sin(w.state[:, 1]),
                                            w.state[:, 2], w.state[:, 3]], 1).astype(np.float32), rtol=0, atol=1e-7)
    # one hand-written step of env 0 (action 2), gymnasium's spelling: equal to within roundings
    want = ar.gym_step(w.state[0], 2)
    w.send(np.full(n, 2))
    np.testing.assert_allclose(w.state[0], want, rtol=0, atol=1e-14)
    assert (w.rewards == -1.0).all() and not w.terminals.any() and (w.tick == 1).all() and w.infos == []
    # a wrap in each direction, a clamp of each velocity, a height terminal from a hand-set state: one step each
    pi = math.pi
    s = np.array([[pi - 0.05, 0.0, 3.0, 0.0], [-pi + 0.05, 0.0, -3.0, 0.0], [0.0, 1.0, 4 * pi, 0.0], [0.0, 1.0, 0.0, -9 * pi],
                  [2.0, 0.0, 2.0, 0.0], [0.05, -0.05, 0.1, -0.1]])
    c = np.array([[0, 3, 0, 3]] * n)
    w.counts = dict.fromkeys(w.counts, 0)
    w.set_states(s, c)
    assert w.ep_return == [-3.0] * n and np.array_equal(w.states()[0], s) and np.array_equal(w.states()[1], c)
    w.send(np.ones(n, np.int64))
    assert w.state[0, 0] < -pi + 0.7 and w.state[1, 0] > pi - 0.7                         # came out on the other side
    assert w.state[2, 2] == 4 * pi and w.state[3, 3] == -9 * pi
    assert w.counts['wrap_down'] >= 1 and w.counts['wrap_up'] >= 1 and w.counts['clamp1'] >= 1 and w.counts['clamp2'] >= 1
    # env 4 was below the bar (-cos 2 - cos 2 = 0.83) and is above it now: reward 0 on the succeeding step, accounted with 3 + 1 steps
    assert -math.cos(2.0) - math.cos(2.0) < 1 < -math.cos(w.state[4, 0]) - math.cos(w.state[4, 0] + w.state[4, 1])
    assert w.terminals[4] and w.rewards[4] == 0.0 and not w.terminals[5] and w.rewards[5] == -1.0 and w.counts['height'] >= 1
    assert dict(episode_return=-3.0, episode_length=4, score=-3.0) in w.infos
    # the auto-reset row: reward 0, not terminal, the next episode's freshly drawn state, the action ignored
    done = w.done.copy()
    assert done[4] and not done[5]
    w.send(np.zeros(n, np.int64))
    assert (w.rewards[done] == 0.0).all() and not w.terminals[done].any() and (w.episode[done] == 1).all() and (w.tick[done] == 0).all()
    assert (np.abs(w.state[done]) <= 0.1).all() and w.tick[5] == 5 and not w.truncations.any() and w.masks.all()


def test_walker_time_limit_velocities_offset_and_seed():
    # max_steps: the step that makes the episode max_steps long is terminal with reward -1 (truncations stay 0), whatever the state
    w = ar.AcrobotSerial(4, max_steps=3)
    w.async_reset(0)
    seen = []
    for k in range(8):
        w.send(np.full(4, k % 3))
        seen.append((w.terminals.copy(), w.rewards.copy(), [i['episode_length'] for i in w.infos], [i['episode_return'] for i in w.infos]))
    assert [s[0].all() for s in seen] == [False, False, True, False, False, False, True, False] and not any(s[0].any() for s in seen[:2])
    assert seen[2][2] == [3] * 4 and seen[2][3] == [-3.0] * 4 and (seen[2][1] == -1).all() and (seen[3][1] == 0).all()
    assert not w.truncations.any() and w.counts['limit'] == 8 and w.counts['height'] == 0
    # max_steps = 0: no time limit
    free = ar.AcrobotSerial(1, max_steps=0)
    free.async_reset(0)
    for k in range(520):
        free.send([1])                                  # no torque: the links hang
        assert not free.terminals.any(), k
    assert free.tick[0] == 520
    # velocities=False: columns 4 and 5 read 0, the dynamics do not change
    full, masked = ar.AcrobotSerial(5), ar.AcrobotSerial(5, velocities=False)
    full.async_reset(2)
    masked.async_reset(2)
    rng = np.random.default_rng(2)
    for k in range(30):
        a = rng.integers(0, 3, 5)
        full.send(a)
        masked.send(a)
        of, om = full.recv()[0], masked.recv()[0]
        assert np.array_equal(of[:, :4], om[:, :4]) and not om[:, 4:].any() and of[:, 4:].all()
    assert np.array_equal(full.state, masked.state)
    # env_offset: envs 3.. of a larger vecenv; the same seed walks the same walk, another seed another
    big, part, again, other = ar.AcrobotSerial(7, max_steps=9), ar.AcrobotSerial(4, max_steps=9, env_offset=3), ar.AcrobotSerial(7, max_steps=9), ar.AcrobotSerial(7, max_steps=9)
    for v, s in ((big, 5), (part, 5), (again, 5), (other, 6)):
        v.async_reset(s)
    for k in range(25):
        a = rng.integers(0, 3, 7)
        for v in (big, again, other):
            v.send(a)
        part.send(a[3:])
        assert np.array_equal(big.state[3:], part.state) and np.array_equal(big.terminals[3:], part.terminals), k
    assert np.array_equal(big.state, again.state) and big.sums.tolist() == again.sums.tolist() and big.sums[0] == 14
    assert not np.array_equal(big.state, other.state)


@pytest.mark.parametrize('max_steps', [500, 12])
def test_the_scripted_inputs_of_the_protocol_test_reach_every_branch(max_steps):
    """What tests/test_gpu_acrobot.py's protocol test drives the device with, on the walker alone: 40 envs, seed 11, the energy-pumping
    rule, after send 14 envs 0..15 put on the branch states, 120 sends in all (30 at max_steps=12).  The walker must have met a wrap in
    each direction, a clamp of each velocity, a height terminal and a time-limit terminal; at max_steps=500 the rule alone swings the
    24 untouched envs up (first at send 70, all by send 116)."""
    w, natural = scripted_run(max_steps)
    print('scripted run, max_steps', max_steps, w.counts, 'natural swing-ups', natural)
    assert all(v >= 1 for v in w.counts.values()), w.counts
    if max_steps == 500:
        assert natural == 24


SET_AT = 14


def scripted_sends(max_steps):
    return 120 if max_steps == 500 else 30


def scripted_run(max_steps, velocities=True, each=None):
    """The scripted run on a walker; `each(k, walker, actions, branch)` is called before send k with the actions about to be sent and
    — at k == SET_AT, after the walker's own set_states — the (states, counters) just set, else None.
    -> (walker, how many of envs 16..39 finished an episode by height)."""
    n = 40
    w = ar.AcrobotSerial(n, max_steps=max_steps, velocities=velocities)
    w.async_reset(11)
    up = set()
    for k in range(scripted_sends(max_steps)):
        branch = None
        if k == SET_AT:
            branch = ar.branch_states(*w.states(), max_steps)
            w.set_states(*branch)
        acts = ar.pump_actions(w.state)
        if each is not None:
            each(k, w, acts, branch)
        w.send(acts)
        up |= {int(e) for e in np.nonzero(w.terminals & (w.rewards == 0.0))[0] if e >= 16}
    return w, len(up)


def test_random_policy_baseline():
    """The walker under uniformly random actions, 32 envs, max_steps=500, seed 0, until 64 episodes have ended: mean episode length
    498.109375 (measured): a random policy almost never swings up inside the limit.  The learning test of tests/test_gpu_acrobot.py
    reads the figure from here."""
    w = ar.AcrobotSerial(32)
    w.async_reset(0)
    rng = np.random.default_rng(0)
    while w.sums[0] < 64:
        w.send(rng.integers(0, 3, 32))
    mean = w.sums[2] / w.sums[0]
    print('random-policy baseline: episodes', w.sums[0], 'mean length', mean, w.counts)
    assert w.sums[0] >= 64 and abs(mean - RANDOM_BASELINE) < 1e-9 and mean > 450


def test_rollout_form_of_the_class_and_of_a_subclass():
    """(general, general + mlp_view, lstm, neither): Acrobot declares the view rollout, the recurrent rollout and the flat one; a
    subclass inherits the latter two but not the view form, which reads the state layout of exactly the declaring class."""
    from pufferlib_amd import clean_pufferl as cp
    from pufferlib_amd import vector as v
    S, R, M = cp.STEPWISE, cp.FUSED_LSTM, cp.FUSED_MLP

    class AcrobotChild(v.Acrobot):
        pass
    engines = [dict(gen_engine=True, lstm_engine=False, mlp_view=False), dict(gen_engine=True, lstm_engine=False, mlp_view=True),
               dict(gen_engine=False, lstm_engine=True, mlp_view=False), dict(gen_engine=False, lstm_engine=False, mlp_view=False)]
    for cls, want in ((v.Acrobot, (S, M, R, M)), (AcrobotChild, (S, S, R, M)), (v.CartPole, (S, M, R, M))):
        assert tuple(cp.rollout_form(cls, **kw) for kw in engines) == want, cls.__name__
    assert v.Acrobot.SEEDED and v.env_creator('acrobot') is v.make_acrobot
    sp = v.make_acrobot()
    assert (sp.max_steps, sp.velocities) == (500, True) and sp.single_action_space.n == 3
    assert sp.single_observation_space.shape == (6,) and sp.single_observation_space.dtype == np.float32
    assert np.array_equal(sp.single_observation_space.high, np.array([1, 1, 1, 1, 4 * math.pi, 9 * math.pi], np.float32))
    assert np.array_equal(sp.single_observation_space.low, -sp.single_observation_space.high)
    assert not v.make_acrobot(max_steps=0, velocities=False).velocities
    from pufferlib_amd import demo
    assert demo.device_backend_for(v.make_acrobot) is v.Acrobot and demo.device_backend_for(v.make_cartpole) is v.CartPole


def test_state_bytes_refuses_bad_configurations_on_the_host():
    from pufferlib_amd import _lib
    _lib.build()
    L = _lib.lib()
    good = _lib.AcrobotConfig(40, 500, 1, 0, 0, 0)
    assert L.pfa_acrobot_state_bytes(C.byref(good)) >= 40 * (5 * 8 + 4 * 4)
    assert L.pfa_acrobot_state_bytes(C.byref(_lib.AcrobotConfig(40, 0, 0, 0, 0, 0))) == L.pfa_acrobot_state_bytes(C.byref(good))
    for n in (0, -3):
        assert L.pfa_acrobot_state_bytes(C.byref(_lib.AcrobotConfig(n, 500, 1, 0, 0, 0))) == 0
        assert b'acrobot: num_envs' in L.pfa_last_error()
    assert L.pfa_acrobot_state_bytes(C.byref(_lib.AcrobotConfig(40, -1, 1, 0, 0, 0))) == 0
    assert b'acrobot: max_steps' in L.pfa_last_error()
    assert L.pfa_acrobot_state_bytes(None) == 0 and b'null config' in L.pfa_last_error()
    # the config struct is laid out like CartPole's, and every acrobot entry point of the header has its ctypes signature
    assert C.sizeof(_lib.AcrobotConfig) == C.sizeof(_lib.CartPoleConfig) == 32
    assert [f[0] for f in _lib.AcrobotConfig._fields_] == [f[0] for f in _lib.CartPoleConfig._fields_]
    import re
    with open(os.path.join(_lib.REPO, 'include', 'pufferlib_amd.h')) as fh:
        declared = set(re.findall(r'\b(pfa_(?:rollout_\w+_)?acrobot\w*)\(', fh.read()))
    bound = {k for k in _lib._SIGNATURES if 'acrobot' in k}
    assert declared == bound and len(bound) == 10 and 'pfa_acrobot_debug_set_states' in bound
    for name in bound:
        assert getattr(L, name) is not None
