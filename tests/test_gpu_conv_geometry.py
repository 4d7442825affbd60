"""models.Convolutional at every frame geometry the reference's environment packages bind it to (tests/conv_geometry.py: vizdoom,
pokemon, links, crafter, dm_lab, butterfly — channel-last uint8 frames, 1 / 3 / 4 channels, odd conv sizes, a 4x pixel stride, hidden
128 or 512) against the reference's arithmetic restated in float64 on the CPU:

  1. every layer's forward, dX and dW (the strided uint8 loader, ragged dX phases), tolerances of tests/test_gpu_cnn.py;
  2. policy(frames) — heads + sampling — for 4 .. 63 actions at both hidden widths, and the width-carrying head entry point against
     the 512-wide one bit for bit;
  3. create / evaluate / train on the device frame vecenv at two geometries: rollout, losses and the gradient against float64, the
     same frames through the host-vecenv path bit for bit, the update in several chunks, a checkpoint into a reference-shaped module."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import conv_geometry as cg  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)
HP = [2.5e-4, 0.99, 0.95, 0.1, 0.5, 0.1, 0.5, 0.01]        # lr, gamma, lambda, clip, vf_coef, vf_clip, max_grad_norm, ent_coef


def _net(tag, actions=4):
    """models.Convolutional of geometry `tag` with the deterministic start weights; (module, float64 weights by name)."""
    from pufferlib_amd import models
    net = models.Convolutional(cg.Env(tag, actions), **cg.GEOMETRIES[tag]['kwargs'])
    w = cg.start_weights(tag, actions)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            assert tuple(v.shape) == w[k].shape, k
            v.copy_(torch.from_numpy(w[k]))
    return net, w


def _nchw(t, n, c, hw):
    return t[:n * hw[0] * hw[1]].view(n, hw[0], hw[1], c).permute(0, 3, 1, 2).cpu().numpy()


def _close_scaled(got, want, name, rtol=1e-4, atol=2e-5):
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got / scale, want / scale, rtol=rtol, atol=atol, err_msg=name)


@pytest.mark.parametrize('n', [3, 37])
@pytest.mark.parametrize('tag', cg.NEW)
def test_every_layer_forward_dx_and_dw_match_float64(tag, n, matrix_products):
    from pufferlib_amd import cnn, models
    net, w = _net(tag)
    cp = models.ConvParams(net, 'cuda')
    eng = cnn.Engine(cp, chunk=64)                       # 37 of 64 rows: a partial chunk, partial tiles in every layer
    geo = cg.GEOMETRIES[tag]
    assert cp.geometry.flat_size == geo['kwargs']['flat_size'] and eng.frame_bytes == int(np.prod(geo['obs']))
    o1, o2, o3 = geo['outs']
    H = cg.hidden_of(tag)
    frames = cg.frames(tag, n)
    G = torch.randn(n, H, generator=torch.Generator().manual_seed(1))
    ref = cg.reference_forward_backward(tag, frames, w, hidden_grad=G)
    dev_frames = torch.from_numpy(frames).cuda().reshape(n, -1).contiguous()
    hd = eng.forward(dev_frames, n)
    np.testing.assert_allclose(_nchw(eng.a1, n, 32, o1), ref['a1'].detach().numpy(), **TOL)
    np.testing.assert_allclose(_nchw(eng.a2, n, 64, o2), ref['a2'].detach().numpy(), **TOL)
    np.testing.assert_allclose(_nchw(eng.a3, n, 64, o3), ref['a3'].detach().numpy(), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(hd.cpu().numpy(), ref['h'].detach().numpy(), rtol=1e-5, atol=3e-5)
    # backward of sum(h * G): d(pre-ReLU hidden) = G * relu'
    eng.dh[:n] = (G * (ref['h'].detach() > 0)).float().cuda()
    eng.d1.fill_(float('nan'))
    eng.d2.fill_(float('nan'))
    grads = torch.zeros(cp.count, device='cuda')
    gv = cp.split(grads)
    eng.backward(dev_frames, n, eng.dh, gv, False)
    for name in ('network.7.weight', 'network.7.bias', 'network.4.weight', 'network.4.bias', 'network.2.weight', 'network.2.bias',
                 'network.0.weight', 'network.0.bias'):
        _close_scaled(gv[name].cpu().numpy(), ref['grads'][name].numpy(), name)
    # dX of conv3 / conv2 (what the engine keeps is d loss / d pre-ReLU input activation: masked by relu')
    want_d2 = (ref['d_a2'] * (ref['a2'].detach() > 0)).numpy()
    want_d1 = (ref['d_a1'] * (ref['a1'].detach() > 0)).numpy()
    _close_scaled(_nchw(eng.d2, n, 64, o2), want_d2, 'conv3 dX')
    d1 = _nchw(eng.d1, n, 32, o1)
    assert np.isfinite(d1).all(), 'conv2 dX left input pixels unwritten'
    _close_scaled(d1, want_d1, 'conv2 dX')
    # rows / columns of conv2's input that none of its 4 x 4 stride-2 windows covers receive exactly 0
    rows, cols = cg.uncovered(o1[0], 4, 2), cg.uncovered(o1[1], 4, 2)
    assert (len(rows) > 0) == ((o1[0] - 4) % 2 != 0) and (len(cols) > 0) == ((o1[1] - 4) % 2 != 0)
    for r in rows:
        assert np.all(d1[:, :, r, :] == 0.0), (tag, 'row', r)
    for c in cols:
        assert np.all(d1[:, :, :, c] == 0.0), (tag, 'column', c)
    # accumulate = True adds a second chunk
    eng.forward(dev_frames, n)
    eng.backward(dev_frames, n, eng.dh, gv, True)
    _close_scaled(gv['network.0.weight'].cpu().numpy(), 2 * ref['grads']['network.0.weight'].numpy(), 'accumulated conv1 dW')


def test_atari_frames_given_channel_last_take_the_strided_loader_to_the_same_numbers():
    """dm_lab's order on Atari-sized frames: (84, 84, 4) channel-last bytes through the word-per-pixel path of the strided loader
    against the same pixels channel-first through the aligned loader — the two first layers see identical patches."""
    from pufferlib_amd import cnn, models
    n = 5
    chw = cg.frames('atari', n)
    out = {}
    for last in (False, True):
        env = cg.Env('atari', 4)
        env.single_observation_space.shape = (84, 84, 4) if last else (4, 84, 84)
        net = models.Convolutional(env, framestack=4, flat_size=3136, channels_last=last)
        w = cg.start_weights('atari', 4)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(torch.from_numpy(w[k]))
        eng = cnn.Engine(models.ConvParams(net, 'cuda'), chunk=16)
        assert (eng.conv1.in_mode == cnn.MODE_IM2COL_U8S) == last
        x = np.ascontiguousarray(chw.transpose(0, 2, 3, 1)) if last else chw
        out[last] = eng.forward(torch.from_numpy(x).cuda().reshape(n, -1).contiguous(), n).clone()
    ref = cg.reference_forward_backward('atari', chw, cg.start_weights('atari', 4))
    for last in (False, True):
        np.testing.assert_allclose(out[last].cpu().numpy(), ref['h'].detach().numpy(), rtol=1e-5, atol=3e-5)


@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])                 # hidden width 128 / 512
@pytest.mark.parametrize('A', [4, 15, 16, 18, 63])
def test_policy_call_samples_and_scores_like_float64(tag, A):
    """policy(frames, noise=...) in rollout mode: <= 15 actions in the 16-lane head kernel at the policy's width, 16 .. 63 in the row
    kernels of the GEMM path; a partial last chunk of frames."""
    from pufferlib_amd import cleanrl, general, models
    n = 41
    net, w = _net(tag, A)
    w['actor.weight'] = w['actor.weight'] * 100.0            # (0.01-gain logits are all but uniform: spread them)
    with torch.no_grad():
        net.actor.weight.copy_(torch.from_numpy(w['actor.weight']))
    pol = cleanrl.Policy(net)
    frames = cg.frames(tag, n, first=100)
    noise = torch.empty(n, A).exponential_(1, generator=torch.Generator().manual_seed(A))
    w64 = {k: torch.from_numpy(v).double() for k, v in w.items()}
    _, _, _, h = cg.encode(tag, torch.from_numpy(frames), w64)
    _, value, action, logprob, entropy, gap = cg.heads(h, w64, noise=noise)
    assert float(gap.min()) > 1e-4, 'a sampling row of this test is a near tie: pick another noise seed'
    a, lp, ent, val = pol(torch.from_numpy(frames).cuda(), noise=noise)
    if A <= 15:                                              # once more in chunks of 16 + 16 + 9 rows (buffers stay sized for 41)
        pol.cnn_engine.chunk = 16
        again = pol(torch.from_numpy(frames).cuda(), noise=noise)
        for x, y in zip((a, lp, ent, val), again):
            assert torch.equal(x, y)
    assert isinstance(pol.flat_params, general.GeneralParams if A > 15 else models.ConvParams)
    assert np.array_equal(a.cpu().numpy(), action.numpy())
    np.testing.assert_allclose(lp.cpu().numpy(), logprob.numpy(), **TOL)
    np.testing.assert_allclose(ent.cpu().numpy(), entropy.numpy(), **TOL)
    np.testing.assert_allclose(val.cpu().numpy().reshape(-1), value.numpy(), **TOL)


@pytest.mark.parametrize('A', [4, 15])
def test_width_entry_point_at_512_returns_the_bits_of_the_old_one(A):
    from pufferlib_amd import _lib
    L = _lib.lib()
    n = 50
    g = torch.Generator().manual_seed(A)
    h = torch.relu(torch.randn(n, 512, generator=g)).cuda()
    aw, ab = (torch.randn(A, 512, generator=g) * 0.05).cuda(), torch.randn(A, generator=g).cuda()
    vw, vb = torch.randn(1, 512, generator=g).cuda(), torch.randn(1, generator=g).cuda()
    noise = torch.empty(n, A).exponential_(1, generator=g).cuda()
    key = _lib.NoiseKey(1, 0)
    got = []
    for wide in (False, True):
        acts = torch.empty(n, dtype=torch.int64, device='cuda')
        lp, ent, val = (torch.empty(n, device='cuda') for _ in range(3))
        tail = (_lib.ptr(aw), _lib.ptr(ab), _lib.ptr(vw), _lib.ptr(vb), A, _lib.ptr(noise), C.byref(key), 0, _lib.ptr(acts), _lib.ptr(lp),
                _lib.ptr(ent), _lib.ptr(val), None)
        if wide:
            _lib.check(L.pfa_cnn_heads_sample(_lib.ptr(h), 512, n, *tail), 'sample_w')
        else:
            _lib.check(L.pfa_cnn_heads_sample(_lib.ptr(h), 512, n, *tail), 'sample')
        got.append((acts, lp, ent, val))
    for x, y in zip(*got):
        assert torch.equal(x, y)
    # a width that has no instantiation of its own (the run-time loop): 144, against float64
    H = 144
    h2 = torch.relu(torch.randn(n, H, generator=g))
    w = {'actor.weight': torch.randn(A, H, generator=g) * 0.2, 'actor.bias': torch.randn(A, generator=g),
         'value_fn.weight': torch.randn(1, H, generator=g), 'value_fn.bias': torch.randn(1, generator=g)}
    _, value, action, logprob, entropy, gap = cg.heads(h2.double(), {k: v.double() for k, v in w.items()}, noise=noise.cpu())
    assert float(gap.min()) > 1e-4
    d = {k: v.cuda() for k, v in w.items()}
    acts = torch.empty(n, dtype=torch.int64, device='cuda')
    lp, ent, val = (torch.empty(n, device='cuda') for _ in range(3))
    _lib.check(L.pfa_cnn_heads_sample(_lib.ptr(h2.cuda()), H, n, _lib.ptr(d['actor.weight']), _lib.ptr(d['actor.bias']),
                                      _lib.ptr(d['value_fn.weight']), _lib.ptr(d['value_fn.bias']), A, _lib.ptr(noise), C.byref(key), 0,
                                      _lib.ptr(acts), _lib.ptr(lp), _lib.ptr(ent), _lib.ptr(val), None), 'sample_w')
    assert np.array_equal(acts.cpu().numpy(), action.numpy())
    np.testing.assert_allclose(lp.cpu().numpy(), logprob.numpy(), **TOL)
    np.testing.assert_allclose(ent.cpu().numpy(), entropy.numpy(), **TOL)
    np.testing.assert_allclose(val.cpu().numpy(), value.numpy(), **TOL)


# ------------------------------------------------------------------------------------------ create / evaluate / train
class _Replay:
    """Host vecenv (the reference's recv / send protocol) that hands out a recorded stream of frames, rewards and dones."""

    def __init__(self, obs, rewards, dones, shape, num_actions):
        from pufferlib_amd import spaces
        self.obs, self.rew, self.done = obs, rewards, dones              # [T][N]...
        n = obs.shape[1]
        self.single_observation_space = spaces.Box(low=0, high=255, shape=tuple(shape), dtype=np.uint8)
        self.single_action_space = spaces.Discrete(num_actions)
        self.driver_env = self
        self.num_envs = self.num_agents = self.agents_per_batch = n
        self.emulated = True
        self.t = 0

    def async_reset(self, seed=42):
        pass

    def recv(self):
        n, t = self.num_envs, self.t % self.obs.shape[0]
        return (self.obs[t].reshape(n, *self.single_observation_space.shape).copy(), self.rew[t].copy(), self.done[t].astype(bool),
                np.zeros(n, bool), [], np.arange(n), np.ones(n, bool))

    def send(self, actions):
        self.t += 1

    def close(self):
        pass


def _trainer(tag, A, n, horizon, nmb, bptt, epochs=1, vec=None, seed=3, rnn=False):
    from pufferlib_amd import clean_pufferl, cleanrl, models, vector
    from test_gpu_ppo import _config
    geo = cg.GEOMETRIES[tag]
    h, w_, c = geo['obs']
    if vec is None:
        vec = vector.make(vector.make_frames, num_envs=n, backend=vector.Frames,
                          env_kwargs=dict(framestack=c, num_actions=A, episode_length=5, height=h, width=w_, channels_last=True))
    net, w = _net(tag, A)
    if rnn:      # the `Recurrent` of the reference's vizdoom / pokemon_red packages: LSTMWrapper(input_size = hidden_size = the conv width)
        H = cg.hidden_of(tag)
        wrap = models.LSTMWrapper(cg.Env(tag, A), net, input_size=H, hidden_size=H)
        with torch.no_grad():
            for k, v in wrap.recurrent.state_dict().items():
                v.copy_(torch.from_numpy(cg.start_weight(k, tuple(v.shape))))
        pol = cleanrl.RecurrentPolicy(wrap)
    else:
        pol = cleanrl.Policy(net)
    B = n * horizon
    data = clean_pufferl.create(_config(n, horizon, B // nmb, bptt, epochs, B * 10, HP, seed=seed, env='frames'), vec, pol)
    return vec, pol, data, w


def _tm(x, n, horizon):
    """env-major experience rows -> [T][N]..."""
    return x.view(n, horizon, *x.shape[1:]).transpose(0, 1).contiguous().cpu().numpy()


# envs, horizon, bptt, env seed of the device-route test.  The gradient of a ReLU network is discontinuous where a ReLU input is 0, and
# fp32 rounding (~1e-6 on these dot products of up to 3520 terms) may flip a unit that close to it; the float64 restatement reports the
# smallest |ReLU input| of the batch and the seeds below are ones where it is well clear: 6.9e-6 (crafter), 1.6e-5 (butterfly; of seeds
# 1..8 at 4 x 8 frames of its 24 000 units each, four came within 1e-6 — hence the smaller batch).  The test asserts > 1e-6.
ROUTE = {'crafter': (4, 8, 4, 5), 'butterfly': (2, 4, 4, 4)}


@pytest.mark.parametrize('A', [6, 18])
@pytest.mark.parametrize('tag', ['crafter', 'butterfly'])
def test_device_frames_rollout_and_update_vs_float64_and_vs_the_host_path(tag, A):
    """vector.Frames at the geometry's frame shape through create / evaluate / train, two iterations.  Iteration 0 (one minibatch, one
    epoch, so losses and gradient belong to the start weights): rollout values / log-probabilities, the three losses and every
    parameter gradient against the float64 restatement.  Then the recorded frames through the host-vecenv path: bit for bit."""
    from pufferlib_amd import clean_pufferl
    n, horizon, bptt, seed = ROUTE[tag]
    B = n * horizon
    vec, pol, data, w = _trainer(tag, A, n, horizon, 1, bptt, seed=seed)
    assert tuple(vec.single_observation_space.shape) == cg.GEOMETRIES[tag]['obs']
    assert (data.gen_engine is not None) == (A > 15) and (data.cnn_engine is not None) == (A <= 15)
    rec = []
    for it in range(2):
        clean_pufferl.evaluate(data)
        e = data.experience
        snap = {k: getattr(e, k).clone() for k in ('obs', 'actions', 'logprobs', 'values', 'rewards', 'dones')}
        clean_pufferl.train(data)
        L = data.losses
        losses = np.array([L.policy_loss, L.value_loss, L.entropy, L.approx_kl, L.clipfrac])
        rec.append((snap, data.flat_params.flat.clone(), losses))
        if it > 0:
            continue
        frames = snap['obs'].cpu().numpy().reshape(B, *cg.GEOMETRIES[tag]['obs'])
        batch = dict(actions=snap['actions'].cpu().numpy(), logprobs=snap['logprobs'].cpu().numpy(), values=snap['values'].cpu().numpy(),
                     advantages=e.advantages.cpu().numpy(), returns=e.returns.cpu().numpy())
        ref = cg.reference_forward_backward(tag, frames, w, batch=batch, clip_coef=HP[3], vf_clip_coef=HP[5], vf_coef=HP[4], ent_coef=HP[7])
        np.testing.assert_allclose(snap['values'].cpu().numpy(), ref['value'].detach().numpy(), **TOL)
        np.testing.assert_allclose(snap['logprobs'].cpu().numpy(), ref['logprob'].detach().numpy(), **TOL)
        np.testing.assert_allclose(losses[:3], [float(ref['pg_loss']), float(ref['v_loss']), float(ref['entropy_loss'])], **TOL)
        gv = data.flat_params.split(data.grads[:data.flat_params.count])
        print(f'[{tag}-{A}] smallest |ReLU input| of the batch in float64: {ref["kink"]:.3e}')
        for name, want in ref['grads'].items():
            got = gv[name].cpu().numpy()
            bad = np.argwhere(np.abs(got - want.numpy()) > 2e-5 + 1e-4 * np.abs(want.numpy()))
            print(f'[{tag}-{A}] {name}: max |err| {np.abs(got - want.numpy()).max():.3e}, past the bound {len(bad)}'
                  f' in output channels {sorted(set(int(b[0]) for b in bad))[:8]}')
        # the gradient is discontinuous where a ReLU input is 0: a unit within fp32 rounding of it may flip (seed chosen so that none is)
        assert ref['kink'] > 1e-6, 'a ReLU input of this batch is a near tie: pick another env seed'
        for name, want in ref['grads'].items():
            _close_scaled(gv[name].cpu().numpy(), want.numpy(), name)
    assert not torch.equal(rec[0][1], rec[1][1]) and bool(torch.isfinite(rec[1][1]).all())
    # the same stream through the host path
    obs = np.concatenate([_tm(s['obs'], n, horizon) for s, _, _ in rec])
    rew = np.concatenate([_tm(s['rewards'], n, horizon) for s, _, _ in rec])
    done = np.concatenate([_tm(s['dones'], n, horizon) for s, _, _ in rec])
    host = _Replay(obs, rew, done, cg.GEOMETRIES[tag]['obs'], A)
    _, _, hdata, _ = _trainer(tag, A, n, horizon, 1, bptt, vec=host, seed=seed)
    assert hdata.host_bridge is not None
    for it in range(2):
        clean_pufferl.evaluate(hdata)
        for k in ('obs', 'actions', 'logprobs', 'values'):
            assert torch.equal(getattr(hdata.experience, k), rec[it][0][k]), (it, k)
        clean_pufferl.train(hdata)
        assert torch.equal(hdata.flat_params.flat, rec[it][1]), it


@pytest.mark.parametrize('tag', ['crafter', 'butterfly'])
def test_update_in_several_chunks_equals_one_chunk(tag):
    from pufferlib_amd import clean_pufferl
    out = []
    for chunk in (None, 16, 8):
        vec, pol, data, _ = _trainer(tag, 6, 8, 8, 2, 4, epochs=2)
        if chunk is not None:
            data.cnn_engine.chunk = chunk            # buffers stay sized for 32 rows; the loops step by `chunk`
        clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        L = data.losses
        out.append((data.experience.actions.clone(), data.experience.values.clone(), data.flat_params.flat.clone(),
                    np.array([L.policy_loss, L.value_loss, L.entropy, L.approx_kl, L.clipfrac])))
    for acts, vals, flat, losses in out[1:]:
        assert torch.equal(acts, out[0][0]) and torch.equal(vals, out[0][1])
        np.testing.assert_allclose(losses, out[0][3], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(flat.cpu().numpy(), out[0][2].cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_large_frames_clamp_the_chunk_to_32_bit_offsets():
    from pufferlib_amd import cnn, models
    net, _ = _net('butterfly')
    eng = cnn.Engine(models.ConvParams(net, 'cuda'), chunk=16)
    assert eng.max_chunk == (2 ** 31 - 1) // 403200 - 1 == 5325
    eng._alloc(8192)                                  # a too-large explicit chunk is clamped, not an error
    assert eng.chunk == 5325 and eng.frames.shape == (5325, 403200)


def test_crafter_checkpoint_loads_into_a_reference_shaped_module_and_resumes(tmp_path):
    from pufferlib_amd import clean_pufferl
    tag, A = 'crafter', 6
    vec, pol, data, _ = _trainer(tag, A, 4, 4, 2, 2)
    data.config.data_dir, data.config.exp_id = str(tmp_path), 'crafter'
    clean_pufferl.evaluate(data)
    clean_pufferl.train(data)
    path = clean_pufferl.save_checkpoint(data)
    want = {k: v.clone() for k, v in pol.state_dict().items()}
    loaded = torch.load(path, weights_only=False)
    ref = cg.reference_module(tag, A)
    ref.load_state_dict({k[len('policy.'):]: v.cpu() for k, v in loaded.state_dict().items()}, strict=True)
    clean_pufferl.evaluate(data)
    clean_pufferl.train(data)
    assert any(not torch.equal(want[k], v) for k, v in pol.state_dict().items())
    clean_pufferl.try_load_checkpoint(data)
    for k, v in pol.state_dict().items():
        assert torch.equal(want[k], v), k
    frames = vec.recv()[0]
    for x, y in zip(loaded(frames, noise=torch.ones(4, A)), pol(frames, noise=torch.ones(4, A))):
        assert torch.equal(x, y)
    # a reference-built module (it names no frame shape) adopts the vecenv's through create()
    from pufferlib_amd import cleanrl, models
    vec2, _, data2, _ = _trainer(tag, A, 4, 4, 2, 2)
    pol2 = cleanrl.Policy(ref)
    from test_gpu_ppo import _config
    d2 = clean_pufferl.create(_config(4, 4, 8, 2, 1, 160, HP, seed=3, env='frames'), vec2, pol2)
    assert d2.flat_params.geometry.obs_shape == cg.GEOMETRIES[tag]['obs']
    clean_pufferl.evaluate(d2)
    clean_pufferl.train(d2)
    assert bool(torch.isfinite(d2.flat_params.flat).all())
    with pytest.raises(ValueError, match='1024'):
        models.conv_geometry_of(ref, (84, 84, 3))


# ------------------------------------------------------------------------------------------ recurrent, device and host route
@pytest.mark.parametrize('A', [6, 18])
@pytest.mark.parametrize('tag', ['vizdoom', 'crafter'])
def test_recurrent_device_frames_rollout_and_update_equal_the_host_path(tag, A):
    """LSTMWrapper over the conv policy at a new frame shape through create / evaluate / train on vector.Frames, two iterations (LSTM
    state carried step to step and into the second rollout), then the recorded stream through the host-vecenv path: experience, final
    LSTM state and updated parameters bit for bit."""
    from pufferlib_amd import clean_pufferl, general
    n, horizon, bptt = 4, 8, 4
    vec, pol, data, _ = _trainer(tag, A, n, horizon, 2, bptt, epochs=2, rnn=True)
    assert tuple(vec.single_observation_space.shape) == cg.GEOMETRIES[tag]['obs']
    H = cg.hidden_of(tag)
    assert isinstance(data.flat_params, general.GeneralParams) and data.gen_engine.net.kind == 'cnn' and data.gen_engine.net.lstm == (H, H)
    rec = []
    for it in range(2):
        clean_pufferl.evaluate(data)
        e = data.experience
        snap = {k: getattr(e, k).clone() for k in ('obs', 'actions', 'logprobs', 'values', 'rewards', 'dones')}
        snap['lstm_h'], snap['lstm_c'] = data.gen_engine.lstm_h.clone(), data.gen_engine.lstm_c.clone()
        assert float(snap['lstm_h'].abs().max()) > 0
        clean_pufferl.train(data)
        rec.append((snap, data.flat_params.flat.clone()))
    assert not torch.equal(rec[0][1], rec[1][1]) and bool(torch.isfinite(rec[1][1]).all())
    assert not torch.equal(rec[0][0]['values'], rec[1][0]['values'])
    obs = np.concatenate([_tm(s['obs'], n, horizon) for s, _ in rec])
    rew = np.concatenate([_tm(s['rewards'], n, horizon) for s, _ in rec])
    done = np.concatenate([_tm(s['dones'], n, horizon) for s, _ in rec])
    host = _Replay(obs, rew, done, cg.GEOMETRIES[tag]['obs'], A)
    _, _, hdata, _ = _trainer(tag, A, n, horizon, 2, bptt, epochs=2, vec=host, rnn=True)
    assert hdata.host_bridge is not None
    for it in range(2):
        clean_pufferl.evaluate(hdata)
        for k in ('obs', 'actions', 'logprobs', 'values'):
            assert torch.equal(getattr(hdata.experience, k), rec[it][0][k]), (it, k)
        assert torch.equal(hdata.gen_engine.lstm_h, rec[it][0]['lstm_h']) and torch.equal(hdata.gen_engine.lstm_c, rec[it][0]['lstm_c']), it
        clean_pufferl.train(hdata)
        assert torch.equal(hdata.flat_params.flat, rec[it][1]), it


# ------------------------------------------------------------------------------------------ the reference's own runs
def _digest(a, samples=64):
    f = np.asarray(a, np.float64).reshape(-1)
    idx = np.linspace(0, f.size - 1, min(samples, f.size)).astype(np.int64)
    return np.concatenate([[f.sum(), np.abs(f).sum()], f[idx]])


@pytest.mark.parametrize('name', ['vizdoom', 'crafter', 'butterfly', 'vizdoom_lstm'])
def test_reference_run_replays_at_the_new_geometries(name, golden_dir, matrix_products):
    """tests/golden/ppo_conv_<name>.npz (make_golden_conv.py: the unmodified reference's create / evaluate / train with
    models.Convolutional at that geometry, 18 actions; `_lstm`: under LSTMWrapper(512, 512)) through create -> evaluate -> train on a
    host vecenv that hands out the recorded frames, rewards and dones, with the reference's multinomial draws as data.noise.
    evaluate(): its actions on every row, log-probabilities and values (and the LSTM state the rollout ends with) within 1e-5.
    train() on what evaluate() stored: losses and every updated tensor within 1e-5."""
    from pufferlib_amd import clean_pufferl, cleanrl, general, models
    from test_gpu_ppo import _config
    tag, rnn = name.replace('_lstm', ''), name.endswith('_lstm')
    g = np.load(os.path.join(golden_dir, f'ppo_conv_{name}.npz'))
    n, horizon, mbs, bptt, epochs, total, iters = (int(x) for x in g['config'])
    hp = [float(x) for x in g['hparams']]
    B, A = n * horizon, 18
    shape = cg.GEOMETRIES[tag]['obs']
    assert float(g['it0.min_gap']) > 1e-4
    frame_ids = g['it0.frame_ids']
    frames = np.stack([[cg.frame(tag, frame_ids[t, e]) for e in range(n)] for t in range(horizon)])      # (T, N, *shape)
    host = _Replay(frames.reshape(horizon, n, -1), g['it0.rewards'].reshape(horizon, n), g['it0.dones'].reshape(horizon, n), shape, A)
    net = models.Convolutional(cg.Env(tag, A), **cg.GEOMETRIES[tag]['kwargs'])
    H = cg.hidden_of(tag)
    pol = cleanrl.RecurrentPolicy(models.LSTMWrapper(cg.Env(tag, A), net, input_size=H, hidden_size=H)) if rnn else cleanrl.Policy(net)
    with torch.no_grad():
        for k, v in pol.state_dict().items():
            bare = k.split('.', 2)[2] if rnn else k[len('policy.'):]
            v.copy_(torch.from_numpy(cg.start_weight(bare, tuple(v.shape))))
            assert np.array_equal(_digest(v.numpy()), g['w0.' + k]), k
    data = clean_pufferl.create(_config(n, horizon, mbs, bptt, epochs, total, hp, seed=1, env='frames'), host, pol)
    assert isinstance(data.flat_params, general.GeneralParams) and data.gen_engine.net.kind == 'cnn' and data.host_bridge is not None
    data.noise = torch.as_tensor(g['it0.noise'])                                                       # (T, N, A)
    clean_pufferl.evaluate(data)
    e = data.experience
    assert data.global_step == int(g['it0.global_step']) and host.t == horizon
    assert np.array_equal(_tm(e.obs, n, horizon).reshape(B, -1), frames.reshape(B, -1))
    assert np.array_equal(_tm(e.actions, n, horizon).reshape(-1), g['it0.actions'].astype(np.int64))
    for key in ('logprobs', 'values', 'rewards', 'dones'):
        got = _tm(getattr(e, key), n, horizon).reshape(-1)
        print(f'[{name}] evaluate {key}: max |err| {np.abs(got - g["it0." + key]).max():.3e}')
        np.testing.assert_allclose(got, g['it0.' + key], err_msg=key, **TOL)
    if rnn:
        np.testing.assert_allclose(data.gen_engine.lstm_h.cpu().numpy(), g['it0.lstm_h'], **TOL)
        np.testing.assert_allclose(data.gen_engine.lstm_c.cpu().numpy(), g['it0.lstm_c'], **TOL)
    clean_pufferl.train(data)
    L = data.losses
    got = [L.policy_loss, L.value_loss, L.entropy, L.old_approx_kl, L.approx_kl, L.clipfrac, L.explained_variance]
    print(f'[{name}] losses max |err| {np.abs(np.array(got) - g["it0.losses"]).max():.3e}')
    np.testing.assert_allclose(got, g['it0.losses'], **TOL)
    worst = 0.0
    for k, v in pol.state_dict().items():
        worst = max(worst, float(np.abs(_digest(v.cpu().numpy())[2:] - g['it0.w.' + k][2:]).max()))
    print(f'[{name}] updated weights, sampled elements: max |err| {worst:.3e}')
    for k, v in pol.state_dict().items():
        got, want = _digest(v.cpu().numpy()), g['it0.w.' + k]
        np.testing.assert_allclose(got[2:], want[2:], err_msg=k, rtol=1e-5, atol=max(1e-5, 0.03 * hp[0]))   # the sampled elements
        np.testing.assert_allclose(got[:2], want[:2], rtol=0, atol=1e-5 * max(1.0, want[1]), err_msg=k + ' (sums)')


# ------------------------------------------------------------------------------------------ the loss kernel at every width form
@pytest.mark.parametrize('H', [512, 128, 144, 272])
@pytest.mark.parametrize('A', [4, 15])
def test_heads_loss_entry_point_at_each_width_vs_float64(H, A):
    """pfa_cnn_heads_loss on its own: the two instantiated widths and two that take the run-time loop (144: nine 16-column groups,
    one partial block of eight; 272: seventeen), a minibatch walked in two chunks (accumulate), rows that end inside a 16-row tile.
    d loss / d head outputs, d loss / d pre-ReLU hidden and the loss sums against float64 autograd; at 512 the bits of the old entry
    point."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    B, nmb, bptt = 88, 2, 4
    mbs = B // nmb
    g = torch.Generator().manual_seed(17 * H + A)
    h = torch.relu(torch.randn(B, H, generator=g))
    w = {'actor.weight': torch.randn(A, H, generator=g) * (1.0 / H ** 0.5), 'actor.bias': torch.randn(A, generator=g) * 0.1,
         'value_fn.weight': torch.randn(1, H, generator=g) * (1.0 / H ** 0.5), 'value_fn.bias': torch.randn(1, generator=g) * 0.1}
    actions = torch.randint(0, A, (B,), generator=g)
    old_lp = torch.log(torch.full((B,), 1.0 / A)) + 0.3 * torch.randn(B, generator=g)
    old_v, adv, ret = (torch.randn(B, generator=g) for _ in range(3))
    hp = _lib.PpoHparams(HP[3], HP[5], HP[4], HP[7], 1, 1, nmb, bptt)
    dev = {k: v.cuda().contiguous() for k, v in dict(h=h, actions=actions.to(torch.int32), lp=old_lp, v=old_v, adv=adv, ret=ret,
                                                      rew=torch.zeros(B), done=torch.zeros(B), obs=torch.zeros(B, 16)).items()}
    exp = _lib.Experience(dev['obs'].data_ptr(), dev['actions'].data_ptr(), dev['lp'].data_ptr(), dev['v'].data_ptr(), dev['rew'].data_ptr(),
                          dev['done'].data_ptr(), dev['adv'].data_ptr(), dev['ret'].data_ptr(), B // 4)
    dw = {k: v.cuda().contiguous() for k, v in w.items()}
    ws = torch.empty(L.pfa_cnn_heads_loss_workspace_bytes(), dtype=torch.uint8, device='cuda')
    mb = 1
    # segment k of minibatch mb is segment mb + k * nmb of the env-major batch (clean_pufferl.py:455-457)
    rows_of_mb = torch.arange(B).view(-1, bptt)[mb::nmb].reshape(-1)
    adv_mb = adv[rows_of_mb].double()
    stats = torch.tensor([[0.0, 0.0], [float(adv_mb.sum()), float((adv_mb ** 2).sum())]], dtype=torch.float64).cuda()

    def run(entry, chunks):
        dout = torch.full((mbs, 16), float('nan'), device='cuda')
        dh = torch.full((mbs, H), float('nan'), device='cuda')
        tail = torch.zeros(16, device='cuda')
        hm = dev['h'][rows_of_mb.cuda()].contiguous()
        q0 = 0
        for ci, m in enumerate(chunks):
            args = (C.byref(exp), B, mb, q0, m, _lib.ptr(dw['actor.weight']), _lib.ptr(dw['actor.bias']), _lib.ptr(dw['value_fn.weight']),
                    _lib.ptr(dw['value_fn.bias']), A, C.byref(hp), _lib.ptr(stats), mbs, _lib.ptr(dout[q0:]), _lib.ptr(dh[q0:]), _lib.ptr(tail),
                    1 if ci else 0, _lib.ptr(ws), None)
            if entry == 'w':
                _lib.check(L.pfa_cnn_heads_loss(_lib.ptr(hm[q0:]), H, *args), 'loss_w')
            else:                   # (what the fixed-width entry point of earlier versions passed)
                _lib.check(L.pfa_cnn_heads_loss(_lib.ptr(hm[q0:]), 512, *args), 'loss')
            q0 += m
        return dout, dh, tail

    dout, dh, tail = run('w', [27, mbs - 27])
    # float64: the loss as a function of the head outputs and of the pre-ReLU hidden vector z (h = relu(z), z := h where h > 0)
    w64 = {k: v.double() for k, v in w.items()}
    z = h[rows_of_mb].double().clone().requires_grad_(True)
    hz = torch.relu(z)
    logits = (hz @ w64['actor.weight'].t() + w64['actor.bias'])
    value = (hz @ w64['value_fn.weight'].t() + w64['value_fn.bias']).flatten()
    logits.retain_grad()
    value.retain_grad()
    logp = logits - logits.logsumexp(-1, keepdim=True)
    logprob = logp.gather(-1, actions[rows_of_mb].unsqueeze(-1)).squeeze(-1)
    entropy = -(logp.exp() * logp).sum(-1)
    loss, pg, vl, ent = cg.ppo_loss(logprob, entropy, value, old_lp[rows_of_mb].double(), old_v[rows_of_mb].double(), adv_mb,
                                    ret[rows_of_mb].double(), clip_coef=HP[3], vf_clip_coef=HP[5], vf_coef=HP[4], ent_coef=HP[7])
    loss.backward()
    want_dh = (z.grad * (h[rows_of_mb] > 0)).numpy()
    got_dout = dout.cpu().numpy()
    np.testing.assert_allclose(got_dout[:, :A], logits.grad.numpy(), **TOL)
    np.testing.assert_allclose(got_dout[:, A], value.grad.numpy(), **TOL)
    assert np.all(got_dout[:, A + 1:] == 0.0)
    assert np.isfinite(dh.cpu().numpy()).all(), 'columns of dh left unwritten'
    np.testing.assert_allclose(dh.cpu().numpy(), want_dh, **TOL)
    sums = tail.cpu().double().view(8, 2).sum(1).numpy() / mbs
    np.testing.assert_allclose(sums[:3], [float(pg), float(vl), float(ent)], **TOL)
    # one chunk = two chunks (fixed-order sums aside: the loss sums to 1e-6, the gradients bit for bit — rows are independent)
    dout1, dh1, tail1 = run('w', [mbs])
    assert torch.equal(dout1, dout) and torch.equal(dh1, dh)
    np.testing.assert_allclose(tail1.cpu().double().view(8, 2).sum(1).numpy(), tail.cpu().double().view(8, 2).sum(1).numpy(), rtol=1e-6, atol=1e-7)
    if H == 512:
        for x, y in zip(run('old', [27, mbs - 27]), (dout, dh, tail)):
            assert torch.equal(x, y)
