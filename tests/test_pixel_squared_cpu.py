"""vector.PixelSquared without a GPU: the creator and its spec, what the creator refuses, the paint rule (tests/pixel_squared_reference.py,
which the GPU test holds the kernel to) as properties of the frames it makes, and the trainer's routing of the class."""
import itertools

import numpy as np
import pytest

from pixel_squared_reference import render
from pufferlib_amd import spaces, vector
from pufferlib_amd.exceptions import APIUsageError

G = 7
# (height, width, channels, channels_last); (30, 44, 4): 30 and 44 are no multiples of 7, the cells are uneven
SHAPES = [(7, 7, 1, True), (40, 40, 3, True), (60, 80, 1, True), (84, 84, 4, False), (30, 44, 4, True)]
BYTES = {0: (0, 0), 1: (255, 128), -1: (128, 255)}      # cell value -> (even-channel byte, odd-channel byte)


def _random_grid(seed):
    """A grid with every cell value somewhere, as floats (what Squared.observations holds)."""
    rng = np.random.default_rng(seed)
    return rng.integers(-1, 2, size=(G, G)).astype(np.float32)


def test_creator_and_spec():
    sp = vector.make_pixel_squared()
    assert isinstance(sp, vector.PixelSquaredSpec) and isinstance(sp, vector.SquaredSpec)
    assert (sp.distance_to_target, sp.num_targets, sp.grid_size) == (3, 1, 7)
    obs = sp.single_observation_space
    assert isinstance(obs, spaces.Box) and obs.shape == (64, 64, 3) and obs.dtype == np.uint8
    assert obs.low.min() == 0 and obs.high.max() == 255
    assert isinstance(sp.single_action_space, spaces.Discrete) and sp.single_action_space.n == 8
    assert sp.observation_space is sp.single_observation_space and sp.action_space is sp.single_action_space
    assert sp.emulated.observation_dtype == np.dtype(np.uint8)
    assert sp.emulated.emulated_observation_dtype == np.dtype((np.uint8, (64, 64, 3)))
    assert sp.num_agents == 1
    first = vector.make_pixel_squared(2, 4, height=84, width=84, channels=4, channels_last=False)
    assert first.single_observation_space.shape == (4, 84, 84) and first.grid_size == 5 and first.num_targets == 4
    assert first.emulated.emulated_observation_dtype == np.dtype((np.uint8, (4, 84, 84)))
    last = vector.make_pixel_squared(height=30, width=44, channels=4)
    assert last.single_observation_space.shape == (30, 44, 4)
    assert vector.make_pixel_squared(distance_to_target=2, num_targets=-1, height=8, width=8, channels=1).num_targets == 8
    assert vector.env_creator('pixel_squared') is vector.make_pixel_squared and vector.env_creator('squared') is vector.make_squared


def test_class_attributes_of_the_backend():
    cls = vector.PixelSquared
    assert issubclass(cls, vector._ResetTape) and issubclass(cls, vector._DeviceVecEnv) and not issubclass(cls, vector.Squared)
    assert cls.OBS_U8 is True and cls.fused_rollout_mlp is None and cls.ROLLOUT_LSTM is None and cls.PREFETCH is False
    assert cls.ABI == 'pfa_squared' and hasattr(cls, 'ensure_tape') and hasattr(cls, 'debug_targets')


def test_the_creator_refuses_frames_smaller_than_the_grid():
    for kw in (dict(height=6, width=64), dict(height=64, width=6), dict(distance_to_target=5, height=10, width=16)):
        with pytest.raises(APIUsageError, match='at least'):
            vector.make_pixel_squared(channels=1, **kw)
    assert vector.make_pixel_squared(distance_to_target=1, height=4, width=4, channels=1).grid_size == 3      # 16 bytes, 3 x 3 grid: taken


def test_the_creator_refuses_channel_counts_outside_one_to_four():
    for c in (0, 5, 8, -1):
        with pytest.raises(APIUsageError, match=r'1\.\.4'):
            vector.make_pixel_squared(channels=c)
    for c in (1, 2, 3, 4):
        assert vector.make_pixel_squared(channels=c).single_observation_space.shape == (64, 64, c)


def test_the_creator_refuses_frames_that_are_no_multiple_of_sixteen_bytes():
    for kw in (dict(height=7, width=7, channels=1), dict(height=9, width=7, channels=3), dict(height=10, width=10, channels=2)):
        with pytest.raises(APIUsageError, match='multiple of 16 bytes'):
            vector.make_pixel_squared(**kw)


@pytest.mark.parametrize('height,width,channels,channels_last', SHAPES)
def test_renderer_properties(height, width, channels, channels_last):
    grid = _random_grid(height * 1000 + width)
    frame = render(grid, height, width, channels, channels_last)
    assert frame.dtype == np.uint8
    assert frame.shape == ((height, width, channels) if channels_last else (channels, height, width))
    hwc = frame if channels_last else frame.transpose(1, 2, 0)
    rows, cols = np.arange(height) * G // height, np.arange(width) * G // width
    # every cell is shown: the boundaries are monotone, start at cell 0, end at cell g - 1 and skip none
    for idx in (rows, cols):
        assert idx[0] == 0 and idx[-1] == G - 1 and set(np.diff(idx)) <= {0, 1}
        assert np.bincount(idx, minlength=G).min() >= 1
    # every pixel of a cell has its cell's byte, in every channel
    for i, j in itertools.product(range(G), range(G)):
        block = hwc[rows == i][:, cols == j]
        assert block.size > 0
        even, odd = BYTES[int(grid[i, j])]
        for c in range(channels):
            assert (block[:, :, c] == (even if c % 2 == 0 else odd)).all(), (i, j, c)
    # a frame determines its grid: one pixel per cell, channel 0, decoded
    decode = {even: v for v, (even, _) in BYTES.items()}
    first_row = [int(np.argmax(rows == i)) for i in range(G)]
    first_col = [int(np.argmax(cols == j)) for j in range(G)]
    back = np.array([[decode[int(hwc[y, x, 0])] for x in first_col] for y in first_row], np.float32)
    assert np.array_equal(back, grid)
    if channels > 1:       # ... and so does an odd channel alone
        decode_odd = {odd: v for v, (_, odd) in BYTES.items()}
        back = np.array([[decode_odd[int(hwc[y, x, 1])] for x in first_col] for y in first_row], np.float32)
        assert np.array_equal(back, grid)


def test_renderer_takes_a_batch_of_grids():
    grids = np.stack([_random_grid(s) for s in range(5)])
    for height, width, channels, channels_last in SHAPES:
        frames = render(grids, height, width, channels, channels_last)
        assert frames.shape[0] == 5
        for n in range(5):
            assert np.array_equal(frames[n], render(grids[n], height, width, channels, channels_last))


def test_the_three_cell_values_differ_in_every_channel():
    for parity in (0, 1):
        assert len({BYTES[v][parity] for v in (0, 1, -1)}) == 3


def test_the_trainer_steps_the_class_whatever_the_engines():
    from pufferlib_amd import clean_pufferl
    for gen, lstm, view in itertools.product((False, True), repeat=3):
        assert clean_pufferl.rollout_form(vector.PixelSquared, gen, lstm, view) == clean_pufferl.STEPWISE
    assert clean_pufferl.rollout_form(vector.Squared, False, False, False) == clean_pufferl.FUSED_MLP      # (what it must not inherit)


def test_the_demo_launcher_hosts_the_creator_on_device():
    from pufferlib_amd import demo
    assert demo.device_backend_for(vector.make_pixel_squared) is vector.PixelSquared
    assert demo.device_backend_for(vector.make_squared) is vector.Squared
