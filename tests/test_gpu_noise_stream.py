"""The Philox stream position of policy(obs) on every kernel route of cleanrl.Policy / RecurrentPolicy (cleanrl.route): a sampling call
without explicit noise draws at (noise_seed, noise_step) and advances noise_step by exactly one; a call with explicit noise or with
given actions leaves it alone, and what an explicit-noise call returns does not depend on it.  A shifted stream is still a valid sample,
so nothing but a bit comparison of two policies at the same position sees one: policy B, same weights and seed, put at noise_step = 2,
must reproduce the third sampling call of policy A bit for bit.  16 rows per case, each route at its smallest shape."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import conv_geometry as cg  # noqa: E402
import resnet_reference as rr  # noqa: E402

gpu = pytest.mark.gpu
ROWS = 16
CONV_TAG = min(cg.GEOMETRIES, key=lambda t: int(np.prod(cg.GEOMETRIES[t]['obs'])))     # the smallest frame


def _flat_env(obs_dim=16, actions=4):
    from pufferlib_amd import namespace, spaces
    return namespace(single_observation_space=spaces.Box(low=-1, high=1, shape=(obs_dim,), dtype=np.float32),
                     single_action_space=spaces.Discrete(actions))


def _default(hidden):
    from pufferlib_amd import cleanrl, models
    return cleanrl.Policy(models.Default(_flat_env(), hidden_size=hidden), seed=5)


def _lstm():
    from pufferlib_amd import cleanrl, models
    env = _flat_env()
    return cleanrl.RecurrentPolicy(models.LSTMWrapper(env, models.Default(env)), seed=5)


def _cnn():
    """The conv engine with room for 8 frames a call: 16 rows span two chunks (the second one's noise rows start at row offset 8)."""
    from pufferlib_amd import cleanrl, models
    pol = cleanrl.Policy(models.Convolutional(cg.Env(CONV_TAG, 4), **cg.GEOMETRIES[CONV_TAG]['kwargs']), seed=5)
    pol.adopt(0, 'cuda')
    pol.cnn_engine.max_chunk = pol.cnn_engine.chunk = 8          # (the buffers stay sized for more)
    return pol


def _resnet():
    from pufferlib_amd import cleanrl, models
    return cleanrl.Policy(models.ProcgenResnet(rr.Env('tiny')), seed=5)


def _flat_obs():
    return torch.randn(ROWS, 16, generator=torch.Generator().manual_seed(1)).cuda()


# route -> (policy constructor, observations, logits, the route cleanrl.route names, tile view expected, policy(obs, action=...) built)
CASES = {
    'mlp': (lambda: _default(128), _flat_obs, 4, 'mlp', None, True),
    'general-tile': (lambda: _default(64), _flat_obs, 4, 'general', True, True),
    'general-rows': (lambda: _default(48), _flat_obs, 4, 'general', False, True),
    'lstm': (_lstm, _flat_obs, 4, 'lstm', None, True),
    'cnn': (_cnn, lambda: torch.from_numpy(cg.frames(CONV_TAG, ROWS)).cuda(), 4, 'cnn', None, True),
    'resnet': (_resnet, lambda: torch.from_numpy(rr.frames('tiny', ROWS)).cuda(), rr.ACTIONS, 'resnet', None, False),
}


def _same(x, y):
    """Bit equality of two call results (tensors, and the (h, c) state tuple of the recurrent route)."""
    assert len(x) == len(y)
    for p, q in zip(x, y):
        if isinstance(p, tuple):
            _same(p, q)
        else:
            assert p.shape == q.shape and torch.equal(p, q)


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_sampling_calls_advance_the_noise_stream_by_one_and_explicit_noise_leaves_it(case):
    from pufferlib_amd import cleanrl, general
    make, make_obs, A, route, tile, scores = CASES[case]
    recurrent = case == 'lstm'

    def build():
        torch.manual_seed(0)        # same weights for every policy of the case
        return make()

    def call(pol, state=None, **kw):
        return pol(obs, state, **kw) if recurrent else pol(obs, **kw)
    obs = make_obs()
    noise = torch.empty(ROWS, A).exponential_(1, generator=torch.Generator().manual_seed(2))
    a = build()
    assert cleanrl.route(a.policy, recurrent) == route
    one = call(a)
    assert a.noise_step == 1
    if tile is not None:
        assert (general.tile_view(a.flat_params) is not None) == tile
    two = call(a, one[4] if recurrent else None)
    state = two[4] if recurrent else None
    assert a.noise_step == 2
    given = call(a, state, noise=noise)
    assert a.noise_step == 2
    if scores:
        scored = call(a, state, action=two[0])
        assert scored[0] is two[0] and a.noise_step == 2
    three = call(a, state)
    assert a.noise_step == 3
    assert not torch.equal(two[1], three[1])          # (another stream position: another draw, another log-probability somewhere)
    if case == 'cnn':
        assert a.cnn_engine.chunk == 8
    # policy B at stream position 2: the third call of A, bit for bit
    b = build()
    b.noise_step = 2
    _same(call(b, state), three)
    assert b.noise_step == 3
    # explicit noise: the same outputs at stream position 3 (b), 2 (a, above) and 0 (a fresh policy)
    _same(call(b, state, noise=noise), given)
    assert b.noise_step == 3
    c = build()
    _same(call(c, state, noise=noise), given)
    assert c.noise_step == 0
