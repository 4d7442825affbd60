"""vector.PixelCatch without a GPU: the creator's spec in both layouts, what the creator refuses, and the C ABI of the family."""
import os
import re

import numpy as np
import pytest

from pufferlib_amd import _lib, spaces, vector
from pufferlib_amd.exceptions import APIUsageError


@pytest.mark.parametrize('channels_last,shape', [(False, (4, 84, 84)), (True, (84, 84, 4))])
def test_spec(channels_last, shape):
    sp = vector.make_pixel_catch(channels_last=channels_last)
    assert isinstance(sp, vector.PixelCatchSpec) and (sp.rows, sp.cols, sp.framestack) == (10, 8, 4)
    obs = sp.single_observation_space
    assert isinstance(obs, spaces.Box) and obs.shape == shape and obs.dtype == np.uint8 and obs.low.min() == 0 and obs.high.max() == 255
    assert isinstance(sp.single_action_space, spaces.Discrete) and sp.single_action_space.n == 3
    assert sp.emulated.emulated_observation_dtype == np.dtype((np.uint8, shape))
    assert vector.env_creator('pixel_catch') is vector.make_pixel_catch
    cls = vector.PixelCatch
    assert issubclass(cls, vector._CounterSeededVecEnv) and cls.OBS_U8 is True and cls.fused_rollout_mlp is None and cls.ROLLOUT_LSTM is None


@pytest.mark.parametrize('kw,message', [
    (dict(rows=2), 'at least 3 rows'), (dict(cols=1), 'at least 3 rows'), (dict(height=9, width=16), 'cannot show'),
    (dict(height=16, width=7), 'cannot show'), (dict(framestack=0), 'framestack 0'), (dict(framestack=5), 'framestack 5'),
    (dict(rows=4, cols=3, height=9, width=8, framestack=1), 'multiple of 16 bytes'), (dict(height=10, width=10, framestack=2), 'multiple of 16 bytes')])
def test_the_creator_refuses(kw, message):
    with pytest.raises(APIUsageError, match=message):
        vector.make_pixel_catch(**kw)
    assert vector.make_pixel_catch(rows=3, cols=2, height=4, width=2, framestack=2).shape == (2, 4, 2)      # the smallest of everything: taken


def test_every_entry_point_is_declared_and_exported():
    hdr = open(os.path.join(_lib.REPO, 'include', 'pufferlib_amd.h')).read()
    declared = set(re.findall(r'\b(pfa_pixel_catch_[a-z_]+)\s*\(', hdr))
    assert declared == {'pfa_pixel_catch_' + s for s in ('state_bytes', 'async_reset', 'send', 'episode_stats', 'last_infos', 'debug_states')}
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, name) for name in declared) and 'pixel_catch.hip' in _lib.SOURCES
    assert L.pfa_pixel_catch_state_bytes(_lib.PixelCatchConfig(48, 10, 8, 4, 84, 84, 0, 0, 0, 0)) == 48 * (48 + 56)      # CatchEnv + EpisodeFin
