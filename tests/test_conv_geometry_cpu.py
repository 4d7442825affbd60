"""Host side of models.Convolutional at the frame geometries of tests/conv_geometry.py: the module has the reference's parameter
names and shapes at all seven, an inconsistent flat_size is a ValueError, and the geometry arithmetic the kernels are driven by
(layer sizes, byte strides of the first layer's loader, pixel counts of the dX phases, the chunk bound of 32-bit offsets) equals
brute-force enumeration on the seven shapes and on odd sizes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import conv_geometry as cg  # noqa: E402


@pytest.mark.parametrize('tag', list(cg.GEOMETRIES))
def test_convolutional_has_the_reference_state_dict_at_every_geometry(tag):
    from pufferlib_amd import models
    A = 18
    net = models.Convolutional(cg.Env(tag, A), **cg.GEOMETRIES[tag]['kwargs'])
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(cg.param_shapes(tag, A)) and got == cg.param_shapes(tag, A)
    ref = cg.reference_module(tag, A)
    ref.load_state_dict(net.state_dict(), strict=True)                      # interchangeable with a reference-shaped module
    assert (net.channels_last, net.downsample) == (ref.channels_last, ref.downsample)
    geo = models.conv_geometry_of(net)
    assert geo.obs_shape == cg.GEOMETRIES[tag]['obs'] and geo.flat_size == cg.GEOMETRIES[tag]['kwargs']['flat_size']
    assert tuple((l[4], l[5]) for l in geo.layers) == cg.GEOMETRIES[tag]['outs']
    # a reference-built module names no frame shape: it travels as an argument (or set_conv_obs_shape)
    assert models.conv_geometry_of(ref, cg.GEOMETRIES[tag]['obs']).layers == geo.layers
    # the float64 restatement runs at this geometry and returns (n, A) logits, (n,) values
    out = cg.reference_forward_backward(tag, cg.frames(tag, 2), cg.start_weights(tag, A))
    assert tuple(out['logits'].shape) == (2, A) and tuple(out['value'].shape) == (2,)
    assert tuple(out['a3'].shape[1:]) == geo.out_shape


@pytest.mark.parametrize('tag', list(cg.GEOMETRIES))
def test_inconsistent_flat_size_is_a_value_error_with_both_numbers(tag):
    from pufferlib_amd import models
    kw = dict(cg.GEOMETRIES[tag]['kwargs'])
    good = kw['flat_size']
    kw['flat_size'] = good + 64
    with pytest.raises(ValueError, match=f'{good + 64}.*{good}'):
        models.Convolutional(cg.Env(tag, 4), **kw)
    ref = cg.reference_module(tag, 4)
    wrong = (4, 100, 84) if tag == 'atari' else tuple(s + 32 if i < 2 else s for i, s in enumerate(cg.GEOMETRIES[tag]['obs']))
    with pytest.raises(ValueError):
        models.conv_geometry_of(ref, wrong)


def test_default_frame_shape_is_the_atari_one():
    from pufferlib_amd import models
    env = type('E', (), {'single_action_space': type('D', (), {'n': 4})()})()
    net = models.Convolutional(env, framestack=4, flat_size=3136)
    geo = models.conv_geometry_of(net)
    assert geo.obs_shape == (4, 84, 84) and geo.aligned_chw and geo.frame_bytes == 28224
    with pytest.raises(ValueError):
        models.Convolutional(cg.Env('crafter', 4), framestack=4, flat_size=1024, channels_last=True, hidden_size=128, output_size=128)


@pytest.mark.parametrize('tag', list(cg.GEOMETRIES))
def test_geometry_of_the_seven_shapes_against_enumeration(tag):
    from pufferlib_amd.conv_geometry import ConvGeometry
    g = cg.GEOMETRIES[tag]
    kw = g['kwargs']
    geo = ConvGeometry(g['obs'], kw.get('channels_last', False), kw.get('downsample', 1))
    b = cg.brute_geometry(g['obs'], kw.get('channels_last', False), kw.get('downsample', 1))
    assert (geo.channels, geo.ih, geo.iw) == (b['channels'], b['ih'], b['iw'])
    assert tuple((l[4], l[5]) for l in geo.layers) == tuple(b['sizes']) == g['outs']
    assert geo.frame_bytes == int(np.prod(g['obs']))
    for mine, want in ((geo.sc, b['sc']), (geo.sy, b['sy']), (geo.sx, b['sx'])):
        assert want is None or mine == want
    # the last byte the loader can touch lies inside the frame
    assert (geo.channels - 1) * geo.sc + (geo.ih - 1) * geo.sy + (geo.iw - 1) * geo.sx < geo.frame_bytes
    assert geo.aligned_chw == (tag == 'atari')
    # chunk bound: the largest n with (n + 1) * (largest per-frame operand) < 2^31
    per = max([geo.frame_bytes] + [max(l[0] * l[1] * l[2], l[3] * l[4] * l[5]) for l in geo.layers])
    n = geo.max_chunk()
    assert (n + 1) * per < 2 ** 31 <= (n + 2) * per
    if tag == 'butterfly':
        assert n == 5325 < 8192
    # with a memory budget: as many frames as keep activations + gradients + the frame itself inside it
    per_frame = geo.frame_bytes + 8 * sum(l[3] * l[4] * l[5] for l in geo.layers)
    assert geo.activation_bytes_per_frame() == per_frame
    assert geo.chunk_for(None) == n and geo.chunk_for(100 * per_frame + 7) == min(n, 100) and geo.chunk_for(1) == 1


@pytest.mark.parametrize('ih', range(13, 32))
def test_odd_sizes_layer_outputs_and_ragged_phase_pixel_counts(ih):
    from pufferlib_amd.conv_geometry import conv_out, phase_pixels, phase_slots
    for iw in range(13, 32):
        for k, s in ((8, 4), (4, 2), (3, 1)):
            assert conv_out(ih, k, s) == cg.brute_conv_out(ih, k, s) and conv_out(iw, k, s) == cg.brute_conv_out(iw, k, s)
        for s in (1, 2, 4):
            hp, wp = phase_slots(ih, iw, s)
            total = 0
            for py in range(s):
                for px in range(s):
                    got = phase_pixels(ih, iw, s, py, px)
                    assert got == cg.brute_phase_pixels(ih, iw, s, py, px) <= hp * wp
                    total += got
            assert total == ih * iw and hp * wp * s * s >= ih * iw
    # rows no 4 x 4 stride-2 window covers: exactly the (IH - KH) mod S leftover
    assert len(cg.uncovered(ih, 4, 2)) == (ih - 4) % 2


def test_frames_spec_shapes_and_default_byte_stream_layout():
    from pufferlib_amd import vector
    spec = vector.make_frames()
    assert spec.single_observation_space.shape == (4, 84, 84)
    spec = vector.make_frames(framestack=3, num_actions=17, height=64, width=64, channels_last=True)
    assert spec.single_observation_space.shape == (64, 64, 3) and spec.single_action_space.n == 17
    assert spec.emulated.emulated_observation_dtype.shape == (64, 64, 3)
    spec = vector.make_frames(framestack=3, height=280, width=480, channels_last=True)
    assert int(np.prod(spec.single_observation_space.shape)) == 403200


def test_float64_restatement_differentiates_the_ppo_loss():
    """The helper's gradient of the PPO loss against a central difference on one actor weight and one conv1 weight (crafter)."""
    tag, A, n = 'crafter', 5, 6
    w = cg.start_weights(tag, A)
    w['actor.weight'] = w['actor.weight'] * 100.0
    rs = np.random.RandomState(0)
    batch = dict(actions=rs.randint(0, A, n), logprobs=np.log(np.full(n, 1.0 / A)) + 0.05 * rs.randn(n), values=rs.randn(n),
                 advantages=rs.randn(n), returns=rs.randn(n))
    fr = cg.frames(tag, n)
    out = cg.reference_forward_backward(tag, fr, w, batch=batch)
    for name, idx in (('actor.weight', (1, 7)), ('network.0.weight', (3, 1, 2, 5))):
        eps = 1e-6
        vals = []
        for sgn in (1, -1):
            w2 = {k: np.asarray(v, np.float64).copy() for k, v in w.items()}
            w2[name][idx] += sgn * eps
            vals.append(float(cg.reference_forward_backward(tag, fr, w2, batch=batch)['loss']))
        fd = (vals[0] - vals[1]) / (2 * eps)
        assert abs(fd - float(out['grads'][name][idx])) <= 1e-6 * max(1.0, abs(fd)), (name, fd)


@pytest.mark.parametrize('tag', ['vizdoom', 'crafter', 'butterfly'])
def test_float64_restatement_equals_the_reference_fixtures(tag, golden_dir):
    """tests/golden/ppo_conv_<tag>.npz was written by the unmodified reference (make_golden_conv.py): the values and the logits it
    computed on its recorded rollout pin the restatement the GPU tests compare against."""
    g = np.load(os.path.join(golden_dir, f'ppo_conv_{tag}.npz'))
    n, horizon = int(g['config'][0]), int(g['config'][1])
    ids = g['it0.frame_ids']
    fr = np.stack([cg.frame(tag, ids[t, e]) for t in range(horizon) for e in range(n)])
    w = {k: torch.from_numpy(v).double() for k, v in cg.start_weights(tag, 18).items()}
    _, _, _, h = cg.encode(tag, torch.from_numpy(fr), w)
    logits, value, _, logprob, _, _ = cg.heads(h, w, actions=torch.from_numpy(g['it0.actions'].astype(np.int64)))
    from cnn_golden import digest
    print(f'[{tag}] values max |err| {np.abs(value.numpy() - g["it0.values"]).max():.3e}, logits digest max |err| '
          f'{np.abs(digest(logits.numpy()) - g["it0.logits"])[2:].max():.3e}')
    np.testing.assert_allclose(value.numpy(), g['it0.values'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(digest(logits.numpy())[2:], g['it0.logits'][2:], rtol=0, atol=1e-6)
    np.testing.assert_allclose(logprob.numpy(), g['it0.logprobs'], rtol=0, atol=1e-6)
