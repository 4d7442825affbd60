"""vector.Catch without a GPU: the creator's spec, how the trainer rolls the class out, and what the creator, the trainer and the C
ABI refuse — each naming the family."""
import ctypes as C

import numpy as np
import pytest

from pufferlib_amd import _lib, clean_pufferl as cp, vector
from pufferlib_amd.exceptions import APIUsageError


@pytest.mark.parametrize('kw,shape', [(dict(), (80,)), (dict(rows=16, cols=10), (160,)), (dict(obs='coords'), (4,)),
                                      (dict(rows=200, cols=256, obs='coords', velocities=False), (3,))])
def test_spec_and_rollout_form(kw, shape):
    sp = vector.make_catch(**kw)
    obs = sp.single_observation_space
    assert obs.shape == shape and obs.dtype == np.float32 and obs.low.min() == (-1.0 if kw.get('obs') == 'coords' else 0.0)
    assert sp.single_action_space.n == 3 and vector.env_creator('catch') is vector.make_catch
    assert vector.make_catch(rows=3, cols=4).text(1, 3, 0) == '....\n...o\n=...'
    # (general, general + mlp_view, lstm, neither): the view rollout, the recurrent rollout and the flat one
    engines = [(True, False, False), (True, False, True), (False, True, False), (False, False, False)]
    assert [cp.rollout_form(vector.Catch, *e) for e in engines] == [cp.STEPWISE, cp.FUSED_MLP, cp.FUSED_LSTM, cp.FUSED_MLP]


@pytest.mark.parametrize('refused,error,message', [
    (lambda: vector.make_catch(rows=9, cols=18), APIUsageError, 'vector.Catch: a 9 x 18 grid is a row of 162 values'),
    (lambda: vector.make_catch(obs='pixels'), APIUsageError, "vector.Catch: obs='pixels'"),
    (lambda: vector.make_catch(rows=2), APIUsageError, 'vector.Catch: a 2 x 8 grid'),
    (lambda: vector.make_catch(rows=300, obs='coords'), APIUsageError, 'vector.Catch: a 300 x 8 grid'),
    (lambda: vector.Catch.check_policy(conv=True), NotImplementedError, 'vector.Catch shows flat float32 rows'),
    (lambda: vector.Catch.check_policy(multidiscrete=True), NotImplementedError, 'vector.Catch takes one Discrete')])
def test_refusals_name_the_family(refused, error, message):
    with pytest.raises(error, match=message):
        refused()


@pytest.mark.parametrize('cfg,message', [
    ((48, 10, 8, 0, 1, 96, 0, 0), None), ((48, 16, 10, 0, 1, 160, 0, 0), None), ((48, 200, 256, 1, 0, 16, 0, 0), None),
    ((0, 10, 8, 0, 1, 96, 0, 0), b'catch: num_envs'), ((48, 2, 8, 0, 1, 16, 0, 0), b'catch: the grid must have at least'),
    ((48, 9, 18, 0, 1, 160, 0, 0), b'catch: the grid form shows at most 160'), ((48, 10, 8, 2, 1, 96, 0, 0), b'catch: obs_form'),
    ((48, 10, 8, 0, 1, 64, 0, 0), b'catch: obs_stride'), ((48, 10, 8, 0, 1, 80, 0, 0), b'catch: obs_stride'),
    ((48, 257, 8, 1, 1, 16, 0, 0), b'catch: the grid\'s sides')])
def test_state_bytes_refuses_bad_configurations_on_the_host(cfg, message):
    _lib.build()
    nbytes = _lib.lib().pfa_catch_state_bytes(C.byref(_lib.CatchConfig(*cfg)))
    assert (nbytes == 48 * (48 + 56)) if message is None else (nbytes == 0 and message in _lib.lib().pfa_last_error())     # CatchEnv + EpisodeFin
