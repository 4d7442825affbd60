"""vector.TabularMDP on the CPU: validation, the threshold rule, the two builders, and the numpy walker of tests/tabular_reference.py
(the restatement the GPU tests compare vector.Tabular with) against the golden trajectory of the unmodified reference."""
import os

import numpy as np
import pytest

import tabular_reference as tr
from pufferlib_amd import vector
from pufferlib_amd.vector import TabularMDP

M32 = 2 ** 32 - 1


def _chain(**over):
    """A valid 3-state, 2-action, 2-outcome table; `over` replaces fields."""
    kw = dict(next_state=[[[1, 0], [2, 0]], [[2, 1], [0, 1]], [[2, 2], [2, 2]]],
              prob=[[[0.5, 0.5], [0.25, 0.75]], [[1.0, 0.0], [0.0, 1.0]], [[0.5, 0.5], [0.5, 0.5]]],
              reward=[[0.0, 1.0], [0.5, 0.0], [0.0, 0.0]], terminal=[False, False, True], obs=[[0.0], [1.0], [2.0]], start=0, horizon=5)
    kw.update(over)
    return TabularMDP(**kw)


def test_a_valid_table_is_immutable_and_hashable_by_identity():
    m, m2 = _chain(), _chain()
    assert (m.num_states, m.num_actions, m.num_outcomes, m.num_starts, m.obs_dim) == (3, 2, 2, 1, 1)
    assert m.next_state.dtype == np.int32 and m.prob.dtype == np.float64 and m.reward.shape == (3, 2, 2) and m.obs.dtype == np.float32
    assert m.cum.dtype == np.uint32 and m.start_cum.tolist() == [M32]
    assert m != m2 and hash(m) != hash(m2) and len({m, m2, m}) == 2
    with pytest.raises(AttributeError):
        m.horizon = 3
    with pytest.raises(ValueError):
        m.prob[0, 0, 0] = 1.0
    # K = 1 with the axis omitted; [S][A] reward broadcast over outcomes
    d = TabularMDP([[1, 0], [1, 1]], reward=[[1.0, 0.0], [0.0, 0.0]], terminal=[0, 1], obs=[[0.0, 1.0], [1.0, 0.0]], start=0, horizon=2)
    assert d.num_outcomes == 1 and d.cum.shape == (2, 2, 1) and (d.cum == M32).all() and d.obs_dim == 2
    assert _chain(reward=[[[0.0, 1.0], [2.0, 3.0]]] * 3).reward[1, 1, 1] == 3.0


@pytest.mark.parametrize('field, over, number', [
    ('next_state', dict(next_state=[[[1, 0], [3, 0]], [[2, 1], [0, 1]], [[2, 2], [2, 2]]]), '3'),
    ('next_state', dict(next_state=[[[1, 0], [-1, 0]], [[2, 1], [0, 1]], [[2, 2], [2, 2]]]), '-1'),
    ('next_state', dict(next_state=np.zeros((3, 2, 9), int), prob=np.full((3, 2, 9), 1 / 9)), '9'),
    ('next_state', dict(next_state=np.zeros((3, 1025), int), prob=None), '1025'),
    ('prob', dict(prob=[[[0.5, 0.4], [0.25, 0.75]], [[1.0, 0.0], [0.0, 1.0]], [[0.5, 0.5], [0.5, 0.5]]]), '0.9'),
    ('prob', dict(prob=[[[1.5, -0.5], [0.25, 0.75]], [[1.0, 0.0], [0.0, 1.0]], [[0.5, 0.5], [0.5, 0.5]]]), '-0.5'),
    ('prob', dict(prob=[[[np.nan, 0.5], [0.25, 0.75]], [[1.0, 0.0], [0.0, 1.0]], [[0.5, 0.5], [0.5, 0.5]]]), 'non-finite'),
    ('prob', dict(prob=np.full((3, 2, 3), 1 / 3)), '(3, 2, 3)'),
    ('prob', dict(prob=None), '2'),
    ('reward', dict(reward=[[0.0, np.inf], [0.5, 0.0], [0.0, 0.0]]), 'non-finite'),
    ('reward', dict(reward=np.zeros((2, 2))), '(2, 2)'),
    ('terminal', dict(terminal=[False, True]), '(2,)'),
    ('obs', dict(obs=np.zeros((3, 161))), '161'),
    ('obs', dict(obs=np.zeros((2, 4))), '(2, 4)'),
    ('obs', dict(obs=[[0.0], [np.nan], [2.0]]), 'non-finite'),
    ('start', dict(start=2), '2'),                                       # a terminal start state
    ('start', dict(start=3), '3'),
    ('start', dict(start=([0, 1], [0.5, 0.4])), '0.9'),
    ('start', dict(start=([0, 1], [1.5, -0.5])), '-0.5'),
    ('start', dict(start=([0, 1, 0, 1], [0.25] * 4)), '4'),               # M > S
    ('horizon', dict(horizon=0), '0'),
    ('horizon', dict(horizon=2.5), '2.5'),
    ('score', dict(score=[0.0, 1.0]), '(2,)'),
    ('score', dict(score=[0.0, np.inf, 1.0]), 'non-finite'),
])
def test_every_violation_is_a_value_error_naming_the_field_and_the_number(field, over, number):
    with pytest.raises(ValueError) as err:
        _chain(**over)
    assert str(err.value).startswith(field + ':') and number in str(err.value), str(err.value)


def test_too_many_states_is_refused_before_any_table_is_looked_at():
    with pytest.raises(ValueError, match=r'next_state: 1048577 states'):
        TabularMDP(np.zeros((2 ** 20 + 1, 1), np.int32), obs=np.zeros((2 ** 20 + 1, 1), np.float32), horizon=1)


def test_threshold_rule_on_hand_computed_cases():
    m = _chain()
    # 0.5 / 0.5: floor(2^32 * 0.5) = 2^31, floor(2^32 * 1.0) clipped to 2^32 - 1
    assert m.cum[0, 0].tolist() == [2 ** 31, M32] and m.cum[0, 1].tolist() == [2 ** 30, M32]
    assert [m.outcome(m.cum[0, 0], w) for w in (0, 2 ** 31 - 1, 2 ** 31, M32 - 1, M32)] == [0, 0, 1, 1, 1]
    # probability 1.0 then 0.0: every word below 2^32 - 1 is under cum[0]; the word 2^32 - 1 is under no threshold and falls back to
    # the last outcome with non-zero probability, which is outcome 0 — the zero-probability outcome 1 is never chosen
    assert m.cum[1, 0].tolist() == [M32, M32]
    assert [m.outcome(m.cum[1, 0], w) for w in (0, 12345, M32 - 1, M32)] == [0, 0, 0, 0]
    # probability 0.0 then 1.0: cum[0] = 0 is above no word
    assert m.cum[1, 1].tolist() == [0, M32]
    assert [m.outcome(m.cum[1, 1], w) for w in (0, 1, M32 - 1, M32)] == [1, 1, 1, 1]
    # 1/3, 1/3, 1/3: the float64 partial sums are 1/3, 2/3 and 1.0 (or one ulp below: the clip and the fallback cover both)
    t = TabularMDP([[[0, 0, 0]]], prob=[[[1 / 3, 1 / 3, 1 / 3]]], obs=[[0.0]], horizon=1)
    third = 2 ** 32 // 3                       # 1431655765 = floor(2^32 / 3); 2/3 -> 2863311530
    assert t.cum[0, 0].tolist() == [third, 2 * third, M32]
    assert [t.outcome(t.cum[0, 0], w) for w in (0, third - 1, third, 2 * third - 1, 2 * third, M32 - 1, M32)] == [0, 0, 1, 1, 2, 2, 2]
    # a zero-probability outcome in the middle and at the end
    z = TabularMDP([[[0, 0, 0, 0]]], prob=[[[0.25, 0.0, 0.75, 0.0]]], obs=[[0.0]], horizon=1)
    assert z.cum[0, 0].tolist() == [2 ** 30, 2 ** 30, M32, M32]
    assert [z.outcome(z.cum[0, 0], w) for w in (0, 2 ** 30 - 1, 2 ** 30, M32 - 1, M32)] == [0, 0, 2, 2, 2]
    # the start distribution goes through the same rule
    s = _chain(start=([1, 0], [0.25, 0.75]))
    assert s.start_cum.tolist() == [2 ** 30, M32] and s.start_states.tolist() == [1, 0]


def test_walker_outcome_frequencies_match_the_probabilities():
    """2^16 transition words of the walker (seed 11: envs 0 .. 2^16 - 1 at episode 0, tick 0) select each outcome of a (0.5, 0.2, 0.0,
    0.3) row within 4 binomial standard deviations of its probability; so do 2^16 start draws of a (0.1, 0.9) start distribution."""
    from oracle import c_oracle
    prob = np.array([0.5, 0.2, 0.0, 0.3])
    m = TabularMDP([[[0, 0, 0, 0]]], prob=[[prob]], obs=[[0.0]], horizon=1)
    n = 2 ** 16
    ref = tr.TabularSerial(m, 1)
    ref.seed = 11
    e = np.arange(n, dtype=np.uint32)
    for domain, cum, p in ((1, m.cum[0, 0], prob), (0, TabularMDP.thresholds(np.cumsum([0.1, 0.9])), np.array([0.1, 0.9]))):
        words = c_oracle.philox4x32_10_bulk(e, 0, 0, domain, 11, 0x5442)[0]
        assert all(int(words[i]) == ref.word(i, 0, 0, domain) for i in (0, 1, 77, n - 1))      # the walker's own (scalar) words
        counts = np.bincount([TabularMDP.outcome(cum, w) for w in words], minlength=len(p))
        sigma = np.sqrt(n * p * (1 - p))
        assert (np.abs(counts - n * p) <= 4 * sigma).all(), (counts, n * p, sigma)
        assert counts[p == 0].sum() == 0


def test_gridworld_builder():
    g = TabularMDP.gridworld(5, 5, slip=0.1, horizon=20)
    assert (g.num_states, g.num_actions, g.num_outcomes, g.num_starts, g.obs_dim, g.horizon) == (25, 4, 3, 24, 25, 20)
    assert np.array_equal(g.obs, np.eye(25, dtype=np.float32)) and g.terminal.tolist() == [False] * 24 + [True]
    assert g.next_state[0, 0].tolist() == [0, 0, 1] and g.next_state[0, 3].tolist() == [1, 0, 5]      # corner: up stays, slips go left / right
    assert g.next_state[12, 1].tolist() == [17, 11, 13] and g.reward[19, 1].tolist() == [1.0, 0.0, 0.0]
    assert tr.reachable(g).all()
    d = TabularMDP.gridworld(3, 4, goal=(0, 2), horizon=3)
    assert d.num_outcomes == 1 and d.terminal.tolist().index(True) == 2 and tr.reachable(d).all()
    # deterministic: the goal is reached from exactly the cells at most 3 moves away; uniform start over the 11 other cells
    dist = np.array([abs(r - 0) + abs(c - 2) for r in range(3) for c in range(4)])
    assert abs(tr.optimal_score(d) - ((dist <= 3).sum() - 1) / 11) < 1e-12
    assert tr.optimal_score(TabularMDP.gridworld(5, 5, horizon=8)) == 1.0           # every cell is within 8 moves of the corner
    opt = tr.optimal_score(g)
    assert 0.99 < opt < 1.0                                                          # slip 0.1: 20 steps almost always suffice
    with pytest.raises(ValueError, match='goal'):
        TabularMDP.gridworld(3, 3, goal=(3, 0))
    with pytest.raises(ValueError, match='obs: rows of 169'):
        TabularMDP.gridworld(13, 13)


def test_tmaze_builder():
    t = TabularMDP.tmaze(3)
    assert (t.num_states, t.num_actions, t.num_outcomes, t.num_starts, t.obs_dim, t.horizon) == (10, 2, 1, 2, 3, 4)
    assert t.obs[0].tolist() == [1, 0, 0] and t.obs[4].tolist() == [0, 1, 0] and t.obs[3].tolist() == t.obs[7].tolist() == [0, 0, 1]
    assert np.array_equal(t.obs[1:3], t.obs[5:7]) and not t.obs[1:3].any()           # the corridor looks the same under either cue: a POMDP
    assert tr.reachable(t).all() and tr.optimal_score(t) == 1.0
    # a walk: the right turn scores 1, the wrong one 0; episodes take length + 1 steps
    ref = tr.TabularSerial(t, 8)
    ref.async_reset(3)
    cue = ref.recv()[0][:, 1].astype(np.int64)
    assert set(cue) == {0, 1}
    for step in range(4):
        ref.send(np.where(np.arange(8) < 4, cue, 1 - cue))
    infos = ref.recv()[4]
    assert [i['score'] for i in infos] == [1.0] * 4 + [0.0] * 4 and all(i['episode_length'] == 4 for i in infos)
    assert [i['episode_return'] for i in infos] == [1.0] * 4 + [0.0] * 4


def test_walker_replays_the_reference_golden_with_stochastic_as_a_table(golden_dir):
    """tests/golden/stochastic.npz (the unmodified reference: Serial over make_stochastic) replayed by the table walker: observations,
    f32 rewards, terminals of all 231 recvs and all 12 info rows, array_equal."""
    g = np.load(os.path.join(golden_dir, 'stochastic.npz'))
    n, seed, steps = (int(x) for x in g['config'])
    mdp = tr.stochastic_as_table(float(g['p'][0]))
    assert mdp.num_states == 101 * 101 and mdp.num_outcomes == 1
    ref = tr.TabularSerial(mdp, n)
    ref.async_reset(seed)
    infos = []
    for k in range(steps + 1):
        o, r, te, trunc, info, ids, m = ref.recv()
        assert np.array_equal(o, g['obs'][k]) and np.array_equal(r, g['rewards'][k]), k
        assert np.array_equal(te, g['terminals'][k]) and np.array_equal(trunc, g['truncations'][k]) and m.all(), k
        fin = np.flatnonzero(te)
        assert len(info) == len(fin)
        infos += [(k, j, i['episode_return'], i['episode_length'], i['score']) for j, i in enumerate(info)]
        if k < steps:
            ref.send(g['actions'][k].astype(np.int64))
    assert len(infos) == 12 and np.array_equal(np.array(infos, np.float64).reshape(-1, 5), g['infos'])


def test_spec_and_creator():
    t = TabularMDP.tmaze(2)
    spec = vector.make_tabular(mdp=t)
    assert isinstance(spec, vector.TabularSpec) and spec.single_observation_space.shape == (3,) and spec.single_action_space.n == 2
    assert spec.single_observation_space.dtype == np.float32 and float(spec.single_observation_space.high.max()) == 1.0
    assert spec.emulated.emulated_observation_dtype == np.dtype((np.float32, (3,)))
    assert vector.env_creator('tabular') is vector.make_tabular
    from pufferlib_amd import demo
    assert demo.device_backend_for(vector.make_tabular) is vector.Tabular
    from pufferlib_amd.exceptions import APIUsageError
    with pytest.raises(APIUsageError):
        vector.make_tabular(mdp='gridworld')


def test_make_without_a_gpu_raises_extension_error_and_two_mdps_are_refused():
    import torch
    from pufferlib_amd.exceptions import APIUsageError, ExtensionError
    t, g = TabularMDP.tmaze(2), TabularMDP.gridworld(2, 2)
    # "all envs must share one configuration" is decided before the GPU is asked for: two different tables, or two strides
    with pytest.raises(APIUsageError, match='share one Tabular configuration'):
        vector.make([vector.make_tabular] * 2, env_args=[[], []], env_kwargs=[dict(mdp=t), dict(mdp=g)], backend=vector.Tabular, num_envs=2)
    with pytest.raises(APIUsageError, match='share one Tabular configuration'):
        vector.make([vector.make_tabular] * 2, env_args=[[], []], env_kwargs=[dict(mdp=t), dict(mdp=t, obs_stride=32)],
                    backend=vector.Tabular, num_envs=2)
    with pytest.raises(APIUsageError, match='make_tabular needs mdp'):
        vector.make(vector.make_tabular, backend=vector.Tabular, num_envs=2)
    if not torch.cuda.is_available():
        with pytest.raises(ExtensionError):
            vector.make(vector.make_tabular, env_kwargs=dict(mdp=t), backend=vector.Tabular, num_envs=2)
