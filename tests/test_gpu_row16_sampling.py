"""The 16-lane sampler (csrc/sampler.hpp over csrc/lane_ops.hpp) through policy(obs) on crafted policies and crafted noise: exact
ties, the winner in a head's first and last column, probabilities that underflow to 0 next to masked lanes, and the value lane.
The policies have zero weights, so the decoder bias IS the logit vector and the value head's bias is the value, exactly; equal
logits give equal probabilities whatever the device's expf rounds to, so equal noise makes exact ties.  Every case that is not a
tie is decided by a factor of 100 or more, far beyond any float32 rounding, so the numpy restatement (row16_argmax_forms.py) names
the action without doubt.  Then the fused Squared rollout in both of its template forms (env count a multiple of 16 or not) against
the stepwise protocol path, bit for bit."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from row16_argmax_forms import sample_head

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

ROWS = 40            # two full 16-row tiles and a half-filled one
KINDS = 8
INF = float('inf')


def _head_noise(sz, r):
    """Noise of one head of `sz` columns in row r; the row's kind is r % 8 and r // 8 moves the lanes involved."""
    kind, k = r % KINDS, (r // KINDS) % sz
    q = np.ones(sz, np.float32)
    if kind == 1:                                   # two lanes tie (k and the last), the others a factor 128 behind
        q[:] = 64.0
        q[k] = q[sz - 1] = 0.5
    elif kind == 2:                                 # the winner in the last real lane
        q[sz - 1] = 2.0 ** -7
    elif kind == 3:                                 # the winner in lane k
        q[k] = 2.0 ** -7
    elif kind == 4:                                 # lanes k.. tie, the lanes below them a factor 128 behind
        q[:k] = 64.0
        q[k:] = 0.5
    elif kind == 5:                                 # every real ratio is 0: all tie, and no lane outside the head may win
        q[:] = INF
    elif kind == 6:                                 # all different, a factor 100 apart; the winner moves with the row
        q[:] = [100.0 ** ((c + r) % sz) for c in range(sz)]
    elif kind == 7:                                 # huge equal ratios
        q[:] = 1e-30
    return q                                        # kind 0: all equal


def _policy(space, obs_dim, head_logits, value):
    from pufferlib_amd import cleanrl, models, spaces
    env = SimpleNamespace(single_observation_space=spaces.Box(low=-10, high=10, shape=(obs_dim,), dtype=np.float32),
                          single_action_space=space)
    pol = cleanrl.Policy(models.Default(env))
    dec = pol.policy.decoder
    dec = list(dec) if isinstance(dec, torch.nn.ModuleList) else [dec]
    with torch.no_grad():
        for p in pol.parameters():
            p.zero_()
        for layer, lg in zip(dec, head_logits):
            layer.bias.copy_(torch.as_tensor(lg))
        pol.policy.value_head.bias.fill_(value)
    return pol


def _check(nvec, multi, head_logits, value):
    from pufferlib_amd import spaces
    space = spaces.MultiDiscrete(nvec) if multi else spaces.Discrete(nvec[0])
    pol = _policy(space, 11, head_logits, value)
    noise = np.stack([np.concatenate([_head_noise(sz, r) for sz in nvec]) for r in range(ROWS)])
    torch.manual_seed(0)
    a, lp, ent, val = pol(torch.randn(ROWS, 11).cuda(), noise=torch.as_tensor(noise))
    a = a.cpu().numpy().reshape(ROWS, len(nvec))
    want_a = np.zeros((ROWS, len(nvec)), np.int64)
    want_lp, want_ent = np.zeros(ROWS), np.zeros(ROWS)
    for r in range(ROWS):
        col = 0
        for h, sz in enumerate(nvec):
            want_a[r, h], l, e = sample_head(head_logits[h], noise[r, col:col + sz])
            want_lp[r] += l
            want_ent[r] += e
            col += sz
    bad = np.argwhere(a != want_a)
    assert bad.size == 0, f'nvec {nvec}: (row, head) {bad[:8].tolist()} got {a[bad[:8, 0], bad[:8, 1]]} want {want_a[bad[:8, 0], bad[:8, 1]]}'
    # the sampler's other outputs vs float32 numpy, at the tolerance the suite uses for them everywhere (expf / logf differ by ulps)
    np.testing.assert_allclose(lp.cpu().numpy(), want_lp, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ent.cpu().numpy(), want_ent, rtol=1e-5, atol=1e-5)
    assert torch.equal(val.cpu().flatten(), torch.full((ROWS,), value))       # the value lane's content, unchanged
    return want_a


def _far_apart(sz):
    """The last column at 0 and every other column at -200: exp(-200) is 0 in float32, so every other probability is exactly 0."""
    lg = np.full(sz, -200.0, np.float32)
    lg[sz - 1] = 0.0
    return lg


@pytest.mark.parametrize('a', [1, 2, 5, 8, 15])
def test_discrete_ties_take_the_lowest_index(a):
    want = _check([a], False, [np.full(a, 0.75, np.float32)], 3.25)
    assert (want[0::KINDS] == 0).all() and (want[5::KINDS] == 0).all() and (want[7::KINDS] == 0).all()     # all-lane ties
    assert (want[2::KINDS] == a - 1).all()                                                                # the last real lane
    assert sorted(set(want[3::KINDS, 0])) == list(range(min(a, ROWS // KINDS)))                           # the winner moves


@pytest.mark.parametrize('a', [1, 2, 5, 8, 15])
def test_discrete_underflowed_and_masked_lanes_never_win(a):
    # a huge value in lane `a`, right behind the winning last logit lane: it must stay out of the draw and come back unchanged
    want = _check([a], False, [_far_apart(a)], 1e30)
    rows = np.arange(ROWS)
    assert (want[rows % KINDS != 5] == a - 1).all()          # probability 1 in the last real lane whatever the noise
    assert (want[rows % KINDS == 5] == 0).all()              # infinite noise: every ratio +0, the first lane wins the tie


@pytest.mark.parametrize('nvec', [(3, 5, 2), (1, 14), (1, 15)])
def test_multidiscrete_ties_and_head_edges(nvec):
    # (1, 14) fills the row: 15 logit lanes and the value in lane 15.  (1, 15) is one logit too many for the 16 lanes and runs in the
    # row kernels of the GEMM path: the same rules hold there.
    want = _check(list(nvec), True, [np.full(sz, 0.25 - 0.5 * h, np.float32) for h, sz in enumerate(nvec)], -2.5)
    assert (want[0::KINDS] == 0).all()                                        # ties inside every head: its first column
    assert (want[2::KINDS] == np.array(nvec) - 1).all()                       # the winner at every head's last column
    _check(list(nvec), True, [_far_apart(sz) for sz in nvec], 1e30)


@pytest.mark.parametrize('n', [32, 24])      # whole 16-env tiles / a half-filled last tile: the two forms of the fused kernel
def test_fused_squared_rollout_equals_stepwise_in_both_tile_forms(n):
    from pufferlib_amd import clean_pufferl
    from test_gpu_ppo import _config, _make, _t
    horizon = 8
    hp = [2.5e-4, 0.99, 0.95, 0.1, 0.5, 0.1, 0.5, 0.01]
    vec, pol = _make(n)
    torch.manual_seed(n)
    with torch.no_grad():                    # spread the logits so that the actions differ between envs and steps
        for p in pol.parameters():
            p.add_(0.1 * torch.randn_like(p))
    data = clean_pufferl.create(_config(n, horizon, n * horizon // 2, 4, 1, n * horizon * 4, hp, seed=5), vec, pol)
    clean_pufferl.evaluate(data)
    exp = data.experience

    vec2, pol2 = _make(n)
    pol2.load_state_dict(pol.state_dict())
    pol2.noise_seed = 5
    vec2.async_reset(5)
    got = {k: [] for k in ('obs', 'actions', 'logprobs', 'values', 'rewards', 'dones')}
    for t in range(horizon):
        o, r, d, _, _, _, _ = vec2.recv()
        a, lp, _, val = pol2(o)
        for k, x in zip(got, (o.reshape(n, -1), a, lp, val.flatten(), r, d.float())):
            got[k].append(x.clone())
        vec2.send(a)
    assert len(set(torch.cat(got['actions']).tolist())) > 2 and torch.cat(got['dones']).any()     # the rollout is not trivial
    assert torch.equal(_t(exp.obs, n, horizon)[:, :49], torch.cat(got['obs']))
    assert torch.equal(_t(exp.actions, n, horizon).long(), torch.cat(got['actions']))
    for k in ('logprobs', 'values', 'rewards', 'dones'):
        assert torch.equal(_t(getattr(exp, k), n, horizon), torch.cat(got[k])), k
    # the final env state: the live buffers, the targets, and (position, tick, episode sums) through five more sends on both
    assert np.array_equal(np.asarray(vec.debug_targets()), np.asarray(vec2.debug_targets()))
    for t in range(5):
        for k in ('observations', 'rewards', 'terminals'):
            assert torch.equal(getattr(vec, k), getattr(vec2, k)), (t, k)
        act = (torch.arange(n, device=vec.rewards.device) + t) % 8
        for v in (vec, vec2):
            v.ensure_tape(1)
            v.device_send(act)
    vec._k_infos()
    vec2._k_infos()
    for k in ('_fin', '_fin_ret', '_fin_len', '_fin_score'):
        assert torch.equal(getattr(vec, k), getattr(vec2, k)), k
