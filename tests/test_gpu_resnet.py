"""models.ProcgenResnet (the IMPALA ResNet of pufferlib/models.py:159-231) on the GPU against the reference's arithmetic restated in
float64 on the CPU (tests/resnet_reference.py):

  1. every new kernel on its own — the same-padded operand modes 5 (f32, with and without ReLU on load, every epilogue) and 6 (uint8
     frames) in the rows form, dX on the flipped kernel, dW + bias gradient through the weight form, max-pool forward and backward —
     each fed the float64 reference's layer input rounded to fp32, in slices from the middle of NaN-filled allocations;
  2. policy(frames, noise=...) of the whole stack: hidden, logits, values, actions, log-probabilities, entropy, bounded by 4x the error
     the same restatement makes in fp32 on the CPU (floored at 1e-5);
  3. the gradient of the PPO loss through Engine.update_from, in one chunk and in several, with elementwise activation gradients
     where the float64 reference is clear of ReLU kinks and pool ties;
  4. create / evaluate / train on vector.Frames, the same frames through a host vecenv bit for bit, a checkpoint into a
     reference-shaped module; the unmodified reference's own run (tests/golden/ppo_resnet.npz) replayed;
  5. a reference-built module behind cleanrl.Policy."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import resnet_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)
HP = [2.5e-4, 0.99, 0.95, 0.1, 0.5, 0.1, 0.5, 0.01]        # lr, gamma, lambda, clip, vf_coef, vf_clip, max_grad_norm, ent_coef
A = rr.ACTIONS
CASES = [('tiny', 3), ('tiny', 37), ('procgen', 3), ('rgba', 5)]


def _close_scaled(got, want, name, rtol=1e-4, atol=2e-5):
    """The gradient tolerance of tests/test_gpu_conv_geometry.py."""
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got / scale, want / scale, rtol=rtol, atol=atol, err_msg=name)


def _net(tag, module=None):
    from pufferlib_amd import models
    net = module or models.ProcgenResnet(rr.Env(tag), cnn_width=rr.SHAPES[tag]['cnn_width'], mlp_width=rr.SHAPES[tag]['mlp_width'])
    w = rr.start_weights(tag)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            assert tuple(v.shape) == w[k].shape, k
            v.copy_(torch.from_numpy(w[k]))
    return net, w


def _engine(tag, chunk=64):
    from pufferlib_amd import models, resnet
    net, w = _net(tag)
    rp = models.ResnetParams(net, 'cuda')
    eng = resnet.Engine(rp, chunk=chunk)
    eng.pack()
    return eng, rp, w


@functools.lru_cache(maxsize=None)
def _reference(tag, n):
    """Float64 forward and backward of sum(hidden * G) on the first n frames of `tag`, computed once per case."""
    G = torch.randn(n, rr.SHAPES[tag]['mlp_width'], generator=torch.Generator().manual_seed(1))
    return rr.reference_forward_backward(tag, rr.frames(tag, n), rr.start_weights(tag), hidden_grad=G), G


def _mid(values, fill=float('nan')):
    """`values` (numpy [rows][cols]) as a device slice from the middle of an allocation filled with NaN (uint8: 255) — a kernel that
    reads above the first frame or below the last poisons its result, one that writes there is caught by _untouched."""
    t = torch.as_tensor(values)
    rows, cols = t.shape
    pad = 64 * 16 // max(1, cols) + 16
    pad = (pad + 15) // 16 * 16                                # keeps the slice 16-byte aligned, whatever the row length
    big = torch.full((rows + 2 * pad, cols), 255 if t.dtype == torch.uint8 else fill, dtype=t.dtype, device='cuda')
    big[pad:pad + rows] = t.cuda()
    return big[pad:pad + rows], (big, pad, rows)


def _untouched(guard):
    big, pad, rows = guard
    return bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + rows:]).all())


def _nhwc(t64):
    """float64 NCHW map -> numpy fp32 rows [n*H*W][C]."""
    return t64.detach().permute(0, 2, 3, 1).reshape(-1, t64.shape[1]).float().numpy()


def _nchw(rows, n, h, w):
    return rows.view(n, h, w, -1).permute(0, 3, 1, 2).cpu().double().numpy()


def _w64(w, prefix):
    return torch.from_numpy(w[prefix + '.weight']).double(), torch.from_numpy(w[prefix + '.bias']).double()


# ------------------------------------------------------------------------------------------ 1. the kernels on their own
@pytest.mark.parametrize('tag,n', CASES)
def test_same_padded_forward_with_every_epilogue_matches_float64(tag, n):
    """Rows form: mode 6 on the uint8 frames (the first layer), mode 5 on f32 maps with and without ReLU on load, epilogues bias /
    bias + addend / relu(bias + addend) — each one product of depth <= 288 plus a bias, on the reference's own layer input."""
    from pufferlib_amd import resnet
    eng, rp, w = _engine(tag)
    ref, _ = _reference(tag, n)
    frames = rr.frames(tag, n)
    for i, (ic, h, wd, oc, ph, pw) in enumerate(rr.seq_sizes(tag)):
        s, m, pre = eng.seqs[i], ref['maps'][i], f'network.{i}'
        # the sequence's own conv: uint8 frames (mode 6) or the previous sequence's output (mode 5, IC != OC), no ReLU
        if i == 0:
            x_dev, _ = _mid(frames.reshape(n, -1))
            x64 = torch.from_numpy(frames).permute(0, 3, 1, 2).double() / 255.0
            assert s.conv.mode == resnet.MODE_IM2COL_U8P and s.conv.KR % 16 == 0 and s.conv.KR - s.conv.K < 16
        else:
            rows = _nhwc(ref['maps'][i - 1]['x2'])
            x_dev, _ = _mid(rows)
            x64 = torch.from_numpy(rows).double().view(n, h, wd, ic).permute(0, 3, 1, 2)
            assert s.conv.mode == resnet.MODE_IM2COL_PAD
        out, guard = _mid(np.full((n * h * wd, oc), np.nan, np.float32))
        s.conv.forward(x_dev, n, out)
        want = F.conv2d(x64, *_w64(w, pre + '.conv'), padding=1)
        np.testing.assert_allclose(_nchw(out, n, h, wd), want.numpy(), err_msg=f'{pre}.conv', **TOL)
        assert _untouched(guard)
        # a block's conv1 (IC == OC) on t0 with p as the addend: ReLU on load off / on x the three epilogues
        layer = s.b0c1
        t_rows, p_rows = _nhwc(m['t0']), _nhwc(m['p'])
        t_dev, _ = _mid(t_rows)
        p_dev, _ = _mid(p_rows)
        t64 = torch.from_numpy(t_rows).double().view(n, ph, pw, oc).permute(0, 3, 1, 2)
        p64 = torch.from_numpy(p_rows).double().view(n, ph, pw, oc).permute(0, 3, 1, 2)
        for relu_in in (0, 1):
            layer.relu_in = relu_in
            conv = F.conv2d(F.relu(t64) if relu_in else t64, *_w64(w, pre + '.res_block0.conv1'), padding=1)
            for epi, want in ((resnet.EPI_BIAS, conv), (resnet.EPI_BIAS_ADD, conv + p64), (resnet.EPI_BIAS_ADD_RELU, F.relu(conv + p64))):
                out, guard = _mid(np.full((n * ph * pw, oc), np.nan, np.float32))
                layer.forward(t_dev, n, out, epi, None if epi == resnet.EPI_BIAS else p_dev)
                np.testing.assert_allclose(_nchw(out, n, ph, pw), want.numpy(), err_msg=f'{pre} conv1 relu_in={relu_in} epilogue {epi}', **TOL)
                assert _untouched(guard)
        layer.relu_in = 1


@pytest.mark.parametrize('tag,n', CASES)
def test_same_padded_dx_and_dw_match_float64(tag, n):
    """dX = the mode-5 product on dOut against the flipped kernel (epilogues none / mask / mask + addend) into NaN-filled buffers, so a
    pixel left unwritten shows; dW and the bias gradient through the weight form, with ReLU on load, on the uint8 frames (K = 27: not
    a multiple of 4), and `accumulate`."""
    eng, rp, w = _engine(tag)
    ref, _ = _reference(tag, n)
    frames = rr.frames(tag, n)
    gen = torch.Generator().manual_seed(11)
    for i, (ic, h, wd, oc, ph, pw) in enumerate(rr.seq_sizes(tag)):
        s, m, pre = eng.seqs[i], ref['maps'][i], f'network.{i}'
        # ---- the sequence's conv: dX (not for the frames) with no epilogue, dW without ReLU
        d_rows = torch.randn(n * h * wd, oc, generator=gen).numpy()
        d_dev, _ = _mid(d_rows)
        d64 = torch.from_numpy(d_rows).double().view(n, h, wd, oc).permute(0, 3, 1, 2)
        if i == 0:
            x_dev, _ = _mid(frames.reshape(n, -1))
            x64 = torch.from_numpy(frames).permute(0, 3, 1, 2).double() / 255.0
        else:
            rows = _nhwc(ref['maps'][i - 1]['x2'])
            x_dev, _ = _mid(rows)
            x64 = torch.from_numpy(rows).double().view(n, h, wd, ic).permute(0, 3, 1, 2)
            dx, guard = _mid(np.full((n * h * wd, ic), np.nan, np.float32))
            s.conv.backward_dx(d_dev, n, dx)
            want = F.conv_transpose2d(d64, _w64(w, pre + '.conv')[0], padding=1)
            got = _nchw(dx, n, h, wd)
            assert np.isfinite(got).all(), f'{pre}.conv dX left pixels unwritten'
            _close_scaled(got, want.numpy(), f'{pre}.conv dX')
            assert _untouched(guard)
        xg = x64.clone().requires_grad_(False)
        wt = _w64(w, pre + '.conv')[0].clone().requires_grad_(True)
        (F.conv2d(xg, wt, None, padding=1) * d64).sum().backward()
        gw, gwg = _mid(np.full((oc, ic * 9), np.nan, np.float32))
        gb, gbg = _mid(np.full((1, oc), np.nan, np.float32))
        s.conv.backward_dw(x_dev, n, d_dev, gw, gb, False, eng.ws)
        _close_scaled(gw.view(oc, ic, 3, 3).cpu().double().numpy(), wt.grad.numpy(), f'{pre}.conv dW')
        _close_scaled(gb.view(-1).cpu().double().numpy(), d64.sum((0, 2, 3)).numpy(), f'{pre}.conv db')
        s.conv.backward_dw(x_dev, n, d_dev, gw, gb, True, eng.ws)
        _close_scaled(gw.view(oc, ic, 3, 3).cpu().double().numpy(), 2 * wt.grad.numpy(), f'{pre}.conv dW accumulated')
        _close_scaled(gb.view(-1).cpu().double().numpy(), 2 * d64.sum((0, 2, 3)).numpy(), f'{pre}.conv db accumulated')
        assert _untouched(gwg) and _untouched(gbg)
        # ---- a block's conv0 on p: dX masked by p > 0 (+ the skip gradient), dW of relu(p)
        layer, name = s.b0c0, pre + '.res_block0.conv0'
        p_rows = _nhwc(m['p'])
        p_dev, _ = _mid(p_rows)
        p64 = torch.from_numpy(p_rows).double().view(n, ph, pw, oc).permute(0, 3, 1, 2)
        d_rows = torch.randn(n * ph * pw, oc, generator=gen).numpy()
        a_rows = torch.randn(n * ph * pw, oc, generator=gen).numpy()
        d_dev, _ = _mid(d_rows)
        a_dev, _ = _mid(a_rows)
        d64 = torch.from_numpy(d_rows).double().view(n, ph, pw, oc).permute(0, 3, 1, 2)
        a64 = torch.from_numpy(a_rows).double().view(n, ph, pw, oc).permute(0, 3, 1, 2)
        full = F.conv_transpose2d(d64, _w64(w, name)[0], padding=1)
        for mask, addend, want in ((None, None, full), (p_dev, None, full * (p64 > 0)), (p_dev, a_dev, full * (p64 > 0) + a64)):
            dx, guard = _mid(np.full((n * ph * pw, oc), np.nan, np.float32))
            layer.backward_dx(d_dev, n, dx, mask=mask, addend=addend)
            got = _nchw(dx, n, ph, pw)
            assert np.isfinite(got).all(), f'{name} dX left pixels unwritten'
            _close_scaled(got, want.numpy(), f'{name} dX mask={mask is not None} addend={addend is not None}')
            assert _untouched(guard)
        wt = _w64(w, name)[0].clone().requires_grad_(True)
        (F.conv2d(F.relu(p64), wt, None, padding=1) * d64).sum().backward()
        gw, gwg = _mid(np.full((oc, oc * 9), np.nan, np.float32))
        gb, gbg = _mid(np.full((1, oc), np.nan, np.float32))
        layer.backward_dw(p_dev, n, d_dev, gw, gb, False, eng.ws)
        _close_scaled(gw.view(oc, oc, 3, 3).cpu().double().numpy(), wt.grad.numpy(), f'{name} dW (ReLU on load)')
        _close_scaled(gb.view(-1).cpu().double().numpy(), d64.sum((0, 2, 3)).numpy(), f'{name} db')
        assert _untouched(gwg) and _untouched(gbg)


@pytest.mark.parametrize('tag,n', CASES)
def test_max_pool_forward_and_backward_match_float64(tag, n):
    from pufferlib_amd import resnet
    ref, _ = _reference(tag, n)
    gen = torch.Generator().manual_seed(13)
    for i, (ic, h, wd, oc, ph, pw) in enumerate(rr.seq_sizes(tag)):
        c_rows = _nhwc(ref['maps'][i]['c'])
        c_dev, _ = _mid(c_rows)
        c64 = torch.from_numpy(c_rows).double().view(n, h, wd, oc).permute(0, 3, 1, 2).clone().requires_grad_(True)
        p64 = F.max_pool2d(c64, kernel_size=3, stride=2, padding=1)
        assert tuple(p64.shape[2:]) == (ph, pw)
        out, guard = _mid(np.full((n * ph * pw, oc), np.nan, np.float32))
        resnet.maxpool_forward(c_dev, n, h, wd, oc, out)
        assert np.array_equal(_nchw(out, n, ph, pw), p64.detach().numpy()), f'sequence {i}: a maximum is exact'
        assert _untouched(guard)
        d_rows = torch.randn(n * ph * pw, oc, generator=gen).numpy()
        d_dev, _ = _mid(d_rows)
        (p64 * torch.from_numpy(d_rows).double().view(n, ph, pw, oc).permute(0, 3, 1, 2)).sum().backward()
        dc, guard = _mid(np.full((n * h * wd, oc), np.nan, np.float32))
        resnet.maxpool_backward(c_dev, out, d_dev, n, h, wd, oc, dc)
        got = _nchw(dc, n, h, wd)
        assert np.isfinite(got).all()
        _close_scaled(got, c64.grad.numpy(), f'sequence {i} pool backward')
        assert _untouched(guard)


def test_max_pool_backward_sends_a_tie_to_the_first_tap():
    """Constant regions of a frame give exact ties; torch routes the gradient to the first maximum in row-major order."""
    from pufferlib_amd import resnet
    n, h, wd, oc = 2, 5, 6, 4
    c = torch.zeros(n, h, wd, oc)
    c[1, 2:, 3:, :] = torch.tensor([1.0, -1.0, 2.0, 0.0])
    c64 = c.permute(0, 3, 1, 2).double().clone().requires_grad_(True)
    p64 = F.max_pool2d(c64, kernel_size=3, stride=2, padding=1)
    d = torch.randn(n, 3, 3, oc, generator=torch.Generator().manual_seed(3))
    (p64 * d.permute(0, 3, 1, 2).double()).sum().backward()
    c_dev, _ = _mid(c.reshape(-1, oc).numpy())
    d_dev, _ = _mid(d.reshape(-1, oc).numpy())
    out, _ = _mid(np.full((n * 9, oc), np.nan, np.float32))
    dc, guard = _mid(np.full((n * h * wd, oc), np.nan, np.float32))
    resnet.maxpool_forward(c_dev, n, h, wd, oc, out)
    resnet.maxpool_backward(c_dev, out, d_dev, n, h, wd, oc, dc)
    np.testing.assert_allclose(_nchw(dc, n, h, wd), c64.grad.numpy(), rtol=1e-6, atol=1e-6)
    assert _untouched(guard)


# ------------------------------------------------------------------------------------------ 2. the whole stack
def _device_logits(eng, rp, n):
    """Head outputs [n][16] (logits, then the value) of eng.h[:n] through the dense rows kernel."""
    from pufferlib_amd import _lib, cnn
    B = torch.cat([rp.views['actor.weight'], rp.views['value.weight']]).contiguous()
    b = torch.cat([rp.views['actor.bias'], rp.views['value.bias']]).contiguous()
    out = torch.empty(n, 16, device='cuda')
    a = cnn._operand(cnn.MODE_DENSE, eng.h, eng.hidden)
    _lib.check(_lib.lib().pfa_igemm_rows(C.byref(a), n, eng.hidden, _lib.ptr(B), eng.hidden, 16, _lib.ptr(out), 16, cnn.EPI_BIAS, _lib.ptr(b),
                                         None, 0, _lib.stream_handle()), 'head outputs')
    return out.cpu().numpy()


@pytest.mark.parametrize('tag,n', [('tiny', 37), ('procgen', 3), ('rgba', 5)])
def test_policy_call_matches_float64_within_four_fp32_chain_errors(tag, n):
    """policy(frames, noise=...).  The bound is measured, not fixed: the same restatement in fp32 on the CPU against float64; the
    device, an fp32 chain of the same depth in another summation order, may be at most 4x that, floored at the 1e-5 contract.  Actions
    are compared exactly (fp32_chain_error asserts in float64 that every sampling row's margin exceeds 1e-4)."""
    from pufferlib_amd import cleanrl
    net, w = _net(tag)
    frames, noise = rr.frames(tag, n), rr.noise_for(tag, n)
    err, want = rr.fp32_chain_error(tag, frames, w, noise)
    pol = cleanrl.Policy(net)
    act, lp, ent, val = pol(torch.from_numpy(frames), noise=torch.from_numpy(noise))
    eng, rp = pol.cnn_engine, pol.flat_params
    assert val.shape == (n, 1) and act.dtype == torch.int64
    heads = _device_logits(eng, rp, n)
    got = dict(hidden=eng.h[:n].cpu().numpy(), logits=heads[:, :A], value=heads[:, A], logprob=lp.cpu().numpy(), entropy=ent.cpu().numpy())
    for k, g in got.items():
        bound = max(4 * err[k], 1e-5)
        worst = float(np.abs(g.astype(np.float64) - want[k]).max())
        print(f'[{tag}] {k}: fp32 on the CPU {err[k]:.3e}, device {worst:.3e}, bound {bound:.3e}')
    for k, g in got.items():
        assert float(np.abs(g.astype(np.float64) - want[k]).max()) <= max(4 * err[k], 1e-5), k
    assert float(np.abs(val.cpu().numpy().reshape(-1).astype(np.float64) - want['value']).max()) <= max(4 * err['value'], 1e-5)
    assert np.array_equal(act.cpu().numpy(), want['action'])
    with pytest.raises(NotImplementedError, match='action='):
        pol(torch.from_numpy(frames), action=act)


# ------------------------------------------------------------------------------------------ 3. gradients of the PPO loss
def _ppo_batch(tag, n, w):
    """A minibatch on the first n frames: the float64 policy's own draws as actions, old log-probabilities and values nudged off it
    (ratios != 1, some clipped), random advantages and returns."""
    g = torch.Generator().manual_seed(23)
    frames = rr.frames(tag, n)
    out = rr.policy_outputs(tag, frames, w, rr.noise_for(tag, n))
    batch = dict(actions=out['action'].astype(np.int64), logprobs=(out['logprob'] + 0.2 * torch.randn(n, generator=g).numpy()).astype(np.float32),
                 values=(out['value'] + 0.2 * torch.randn(n, generator=g).numpy()).astype(np.float32),
                 advantages=torch.randn(n, generator=g).numpy(), returns=(out['value'] + torch.randn(n, generator=g).numpy()).astype(np.float32))
    return frames, batch


def _update_from(eng, rp, frames, batch):
    """Engine.update_from on one minibatch holding the whole batch; returns (gradient views, loss sums / rows)."""
    from pufferlib_amd import _lib
    n = frames.shape[0]
    dev = {k: torch.as_tensor(v).cuda().contiguous() for k, v in batch.items()}
    dev['actions'] = dev['actions'].to(torch.int32)
    zeros = torch.zeros(n, device='cuda')
    obs = torch.from_numpy(frames).cuda().reshape(n, -1).contiguous()
    exp = _lib.Experience(obs.data_ptr(), dev['actions'].data_ptr(), dev['logprobs'].data_ptr(), dev['values'].data_ptr(), zeros.data_ptr(),
                          zeros.data_ptr(), dev['advantages'].data_ptr(), dev['returns'].data_ptr(), n)
    hp = _lib.PpoHparams(HP[3], HP[5], HP[4], HP[7], 1, 1, 1, 1)
    adv = torch.as_tensor(batch['advantages']).double()
    stats = torch.tensor([[float(adv.sum()), float((adv ** 2).sum())]], dtype=torch.float64).cuda()
    grads = torch.zeros(rp.count + 16, device='cuda')
    eng.update_from(exp, obs, n, 0, hp, stats, n, grads)
    torch.cuda.synchronize()
    return rp.split(grads[:rp.count]), grads[rp.count:].cpu().double().view(8, 2).sum(1).numpy() / n


@pytest.mark.parametrize('tag,n,chunk', [('tiny', 37, 64), ('tiny', 37, 16), ('procgen', 3, 64), ('rgba', 5, 64)])
def test_ppo_gradient_through_update_from_matches_float64(tag, n, chunk):
    """Every parameter gradient and the three loss terms; chunk 16: the minibatch walked as 16 + 16 + 5 rows (accumulate)."""
    eng, rp, w = _engine(tag, chunk=chunk)
    frames, batch = _ppo_batch(tag, n, w)
    ref = rr.reference_forward_backward(tag, frames, w, batch=batch, clip_coef=HP[3], vf_clip_coef=HP[5], vf_coef=HP[4], ent_coef=HP[7])
    gv, sums = _update_from(eng, rp, frames, batch)
    np.testing.assert_allclose(sums[:3], [float(ref['pg_loss']), float(ref['v_loss']), float(ref['entropy_loss'])], **TOL)
    for name, want in ref['grads'].items():
        got = gv[name].cpu().numpy()
        print(f'[{tag}-{n}-{chunk}] {name}: max |err| {np.abs(got - want.numpy()).max():.3e} of max |g| {np.abs(want.numpy()).max():.3e}')
    for name, want in ref['grads'].items():
        _close_scaled(gv[name].cpu().numpy(), want.numpy(), name)


def test_activation_gradients_elementwise_where_the_reference_is_clear_of_kinks_and_ties():
    """tiny, n = 5.  A gradient map is discontinuous where a ReLU input is 0 or a pool window's two best tie; the helper asserts that
    the float64 reference keeps 16 fp32 chain errors away from both (frame seed chosen on the CPU), so nothing is excluded."""
    tag, n = 'tiny', 5
    eng, rp, w = _engine(tag)
    frames, batch = _ppo_batch(tag, n, w)
    err, _ = rr.fp32_chain_error(tag, frames, w, rr.noise_for(tag, n))
    ref = rr.reference_forward_backward(tag, frames, w, batch=batch, clip_coef=HP[3], vf_clip_coef=HP[5], vf_coef=HP[4], ent_coef=HP[7])
    rr.check_margins(ref, max(err.values()))
    for s in eng.seqs:
        for t in (s.gc, s.g0, s.g1, s.gt):
            t.fill_(float('nan'))
    gv, _ = _update_from(eng, rp, frames, batch)
    for i, (ic, h, wd, oc, ph, pw) in enumerate(rr.seq_sizes(tag)):
        s, m = eng.seqs[i], ref['maps'][i]
        for buf, name, hh, ww in ((s.gc, 'c', h, wd), (s.g0, 'p', ph, pw), (s.g1, 'x1', ph, pw), (s.gt, 't0', ph, pw)):
            got = _nchw(buf[:n * hh * ww], n, hh, ww)
            assert np.isfinite(got).all(), f'sequence {i}: d/d{name} left elements unwritten'
            _close_scaled(got, m[name].grad.numpy(), f'sequence {i}: d loss / d {name}')
        # forward maps of the same run, elementwise
        for buf, name, hh, ww in ((s.c, 'c', h, wd), (s.p, 'p', ph, pw), (s.t0, 't0', ph, pw), (s.x1, 'x1', ph, pw), (s.t1, 't1', ph, pw)):
            np.testing.assert_allclose(_nchw(buf[:n * hh * ww], n, hh, ww), m[name].detach().numpy(), err_msg=f'sequence {i}: {name}', rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------ 4. create / evaluate / train
_Replay, _digest, _tm = rr.Replay, rr.digest, rr.time_major


def _trainer(obs, n, horizon, nmb, bptt, epochs=1, vec=None, seed=3, mlp_width=256, module=None, total=None):
    from pufferlib_amd import clean_pufferl, cleanrl, models, vector
    from test_gpu_ppo import _config
    h, w_, c = obs
    if vec is None:
        vec = vector.make(vector.make_frames, num_envs=n, backend=vector.Frames,
                          env_kwargs=dict(framestack=c, num_actions=A, episode_length=5, height=h, width=w_, channels_last=True))
    env = rr.Env('tiny', obs=obs)
    net = module or models.ProcgenResnet(env, mlp_width=mlp_width)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.from_numpy(rr.start_weight(k, tuple(v.shape))))
    w = {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}
    pol = cleanrl.Policy(net)
    B = n * horizon
    data = clean_pufferl.create(_config(n, horizon, B // nmb, bptt, epochs, total or B * 10, HP, seed=seed, env='frames'), vec, pol)
    return vec, pol, data, w


def _restated_update(tag_obs, frames, w, batch):
    """Float64: PPO loss, clip_grad_norm_(0.5), one torch.optim.Adam(lr, eps=1e-5) step -> (reference dict, updated weights)."""
    shape = dict(obs=tag_obs, cnn_width=16, mlp_width=w['network.5.weight'].shape[0])
    ref = rr.reference_forward_backward(shape, frames, w, batch=batch, clip_coef=HP[3], vf_clip_coef=HP[5], vf_coef=HP[4], ent_coef=HP[7])
    params = {k: torch.from_numpy(np.asarray(v)).double().clone().requires_grad_(True) for k, v in w.items()}
    for k, p in params.items():
        p.grad = ref['grads'][k].clone()
    torch.nn.utils.clip_grad_norm_(list(params.values()), HP[6])
    torch.optim.Adam(list(params.values()), lr=HP[0], eps=1e-5).step()
    return ref, {k: p.detach().numpy() for k, p in params.items()}


@pytest.mark.parametrize('obs', [(4, 4, 3), (64, 64, 3)])
def test_device_frames_rollout_and_update_vs_float64_and_vs_the_host_path(obs, tmp_path):
    """vector.Frames at the smallest frame shape it accepts with three channels (rows of a multiple of 16 bytes: 4 x 4 x 3, maps
    4x4 -> 2x2 -> 1x1 -> 1x1) and at Procgen's: 4 envs x 16 steps, one minibatch, one epoch — rollout, losses and the updated weights
    against the float64 restatement; the same frames through a host vecenv bit for bit; the checkpoint into a reference-shaped module."""
    from pufferlib_amd import clean_pufferl, models, resnet
    n, horizon, bptt = 4, 16, 8
    B = n * horizon
    vec, pol, data, w = _trainer(obs, n, horizon, 1, bptt)
    assert tuple(vec.single_observation_space.shape) == obs
    assert isinstance(data.cnn_engine, resnet.Engine) and data.gen_engine is None and isinstance(data.flat_params, models.ResnetParams)
    data.config.data_dir, data.config.exp_id = str(tmp_path), 'resnet'
    clean_pufferl.evaluate(data)
    e = data.experience
    snap = {k: getattr(e, k).clone() for k in ('obs', 'actions', 'logprobs', 'values', 'rewards', 'dones')}
    clean_pufferl.train(data)
    L = data.losses
    losses = np.array([L.policy_loss, L.value_loss, L.entropy])
    flat = data.flat_params.flat.clone()
    frames = snap['obs'].cpu().numpy().reshape(B, *obs)
    batch = dict(actions=snap['actions'].cpu().numpy(), logprobs=snap['logprobs'].cpu().numpy(), values=snap['values'].cpu().numpy(),
                 advantages=e.advantages.cpu().numpy(), returns=e.returns.cpu().numpy())
    ref, new_w = _restated_update(obs, frames, w, batch)
    np.testing.assert_allclose(snap['values'].cpu().numpy(), ref['value'].detach().numpy(), **TOL)
    np.testing.assert_allclose(snap['logprobs'].cpu().numpy(), ref['logprob'].detach().numpy(), **TOL)
    np.testing.assert_allclose(losses, [float(ref['pg_loss']), float(ref['v_loss']), float(ref['entropy_loss'])], **TOL)
    sd = {k[len('policy.'):]: v.cpu().numpy() for k, v in pol.state_dict().items()}
    worst = max(float(np.abs(sd[k] - new_w[k]).max()) for k in new_w)
    print(f'[{obs}] smallest |ReLU input| {ref["kink"]:.3e}, pool gap {ref["pool_gap"]:.3e}; updated weights max |err| {worst:.3e}')
    for k, want in new_w.items():
        assert not np.array_equal(sd[k], w[k]), k
        np.testing.assert_allclose(sd[k], want, err_msg=k, rtol=1e-5, atol=max(1e-5, 0.03 * HP[0]))
    # the checkpoint loads into a reference-shaped module
    path = clean_pufferl.save_checkpoint(data)
    loaded = torch.load(path, weights_only=False)
    twin = rr.reference_module(dict(obs=obs, cnn_width=16, mlp_width=256))
    twin.load_state_dict({k[len('policy.'):]: v.cpu() for k, v in loaded.state_dict().items()}, strict=True)
    for k, v in twin.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    # the same stream through the host path
    host = _Replay(_tm(snap['obs'], n, horizon), _tm(snap['rewards'], n, horizon), _tm(snap['dones'], n, horizon), obs, A)
    _, _, hdata, _ = _trainer(obs, n, horizon, 1, bptt, vec=host)
    assert hdata.host_bridge is not None and isinstance(hdata.cnn_engine, resnet.Engine)
    clean_pufferl.evaluate(hdata)
    for k in ('obs', 'actions', 'logprobs', 'values'):
        assert torch.equal(getattr(hdata.experience, k), snap[k]), k
    clean_pufferl.train(hdata)
    assert torch.equal(hdata.flat_params.flat, flat)


def test_host_route_at_frames_of_a_multiple_of_4_but_not_of_16_bytes():
    """rgba: (9, 7, 4) frames of 252 bytes through create / evaluate / train on a host vecenv.  The float4 row store and frame gather
    take whole 16-byte units, so these rows go through the byte kernels, like the 189-byte ones of `tiny` (which the replay of the
    reference's run covers): the stored frames bit for bit, the reference's actions on every row, log-probabilities and values from
    evaluate() and the three losses from train() (which reads the frames back through the gather) against float64."""
    from pufferlib_amd import clean_pufferl, resnet
    tag, n, horizon, bptt = 'rgba', 4, 4, 2
    B, obs, mlp = n * horizon, rr.SHAPES[tag]['obs'], rr.SHAPES[tag]['mlp_width']
    assert np.prod(obs) % 4 == 0 and np.prod(obs) % 16 != 0
    frames, noise = rr.frames(tag, B), rr.noise_for(tag, B)                                   # row t * n + e: step t, env e
    rewards = np.random.RandomState(3).rand(horizon, n).astype(np.float32)
    host = _Replay(frames.reshape(horizon, n, -1), rewards, np.zeros((horizon, n), np.float32), obs, A)
    _, _, data, w = _trainer(obs, n, horizon, 1, bptt, vec=host, mlp_width=mlp)
    assert data.host_bridge is not None and isinstance(data.cnn_engine, resnet.Engine)
    _, want = rr.fp32_chain_error(tag, frames, w, noise)                                      # (asserts that no sampling row is a near tie)
    data.noise = torch.as_tensor(noise.reshape(horizon, n, A))
    clean_pufferl.evaluate(data)
    e = data.experience
    assert host.t == horizon
    assert np.array_equal(_tm(e.obs, n, horizon).reshape(B, -1), frames.reshape(B, -1))
    assert np.array_equal(_tm(e.actions, n, horizon).reshape(-1), want['action'])
    np.testing.assert_allclose(_tm(e.logprobs, n, horizon).reshape(-1), want['logprob'], **TOL)
    np.testing.assert_allclose(_tm(e.values, n, horizon).reshape(-1), want['value'], **TOL)
    np.testing.assert_array_equal(_tm(e.rewards, n, horizon), rewards)
    snap = {k: getattr(e, k).clone() for k in ('obs', 'actions', 'logprobs', 'values')}
    clean_pufferl.train(data)
    L = data.losses
    batch = dict(actions=snap['actions'].cpu().numpy(), logprobs=snap['logprobs'].cpu().numpy(), values=snap['values'].cpu().numpy(),
                 advantages=e.advantages.cpu().numpy(), returns=e.returns.cpu().numpy())
    ref = rr.reference_forward_backward(tag, snap['obs'].cpu().numpy().reshape(B, *obs), w, batch=batch, clip_coef=HP[3], vf_clip_coef=HP[5],
                                        vf_coef=HP[4], ent_coef=HP[7])
    np.testing.assert_allclose([L.policy_loss, L.value_loss, L.entropy], [float(ref['pg_loss']), float(ref['v_loss']), float(ref['entropy_loss'])], **TOL)
    assert torch.isfinite(data.flat_params.flat).all()


@pytest.mark.parametrize('tag', ['tiny', 'procgen'])
def test_reference_run_replays(tag, golden_dir):
    """tests/golden/ppo_resnet.npz (make_golden_resnet.py: the unmodified reference's create / evaluate / train with
    pufferlib.models.ProcgenResnet) through create -> evaluate -> train on a host vecenv that hands out the recorded frames, rewards
    and dones, with the reference's multinomial draws as data.noise: its actions on every row; log-probabilities, values, losses and
    every updated tensor within 1e-5.  This pins the float64 restatement of tests/resnet_reference.py to the reference itself."""
    from pufferlib_amd import clean_pufferl, cleanrl, models, resnet
    from test_gpu_ppo import _config
    g = np.load(os.path.join(golden_dir, 'ppo_resnet.npz'))
    pre = tag + '.'
    n, horizon, mbs, bptt, epochs, total, iters = (int(x) for x in g[pre + 'config'])
    hp = [float(x) for x in g[pre + 'hparams']]
    B, shape = n * horizon, rr.SHAPES[tag]['obs']
    assert float(g[pre + 'it0.min_gap']) > 1e-4
    frame_ids = g[pre + 'it0.frame_ids']
    frames = np.stack([[rr.frame(tag, frame_ids[t, e]) for e in range(n)] for t in range(horizon)])      # (T, N, *shape)
    host = _Replay(frames.reshape(horizon, n, -1), g[pre + 'it0.rewards'].reshape(horizon, n), g[pre + 'it0.dones'].reshape(horizon, n), shape, A)
    net = models.ProcgenResnet(rr.Env(tag))
    pol = cleanrl.Policy(net)
    with torch.no_grad():
        for k, v in pol.state_dict().items():
            v.copy_(torch.from_numpy(rr.start_weight(k[len('policy.'):], tuple(v.shape))))
            assert np.array_equal(_digest(v.numpy()), g[pre + 'w0.' + k]), k
    # the restatement against the reference module's own forward on the recorded frames
    w64 = {k: torch.from_numpy(v).double() for k, v in rr.start_weights(tag).items()}
    _, h = rr.encode(tag, torch.from_numpy(frames.reshape(B, *shape)), w64)
    np.testing.assert_allclose(rr.heads(h, w64, actions=torch.zeros(B, dtype=torch.long))[0].numpy(), g[pre + 'it0.logits'], **TOL)
    data = clean_pufferl.create(_config(n, horizon, mbs, bptt, epochs, total, hp, seed=1, env='frames'), host, pol)
    assert isinstance(data.cnn_engine, resnet.Engine) and data.host_bridge is not None
    data.noise = torch.as_tensor(g[pre + 'it0.noise'])                                                   # (T, N, A)
    clean_pufferl.evaluate(data)
    e = data.experience
    assert data.global_step == int(g[pre + 'it0.global_step']) and host.t == horizon
    assert np.array_equal(_tm(e.obs, n, horizon).reshape(B, -1), frames.reshape(B, -1))
    assert np.array_equal(_tm(e.actions, n, horizon).reshape(-1), g[pre + 'it0.actions'].astype(np.int64))
    for key in ('logprobs', 'values', 'rewards', 'dones'):
        got = _tm(getattr(e, key), n, horizon).reshape(-1)
        print(f'[{tag}] evaluate {key}: max |err| {np.abs(got - g[pre + "it0." + key]).max():.3e}')
        np.testing.assert_allclose(got, g[pre + 'it0.' + key], err_msg=key, **TOL)
    clean_pufferl.train(data)
    L = data.losses
    got = [L.policy_loss, L.value_loss, L.entropy, L.old_approx_kl, L.approx_kl, L.clipfrac, L.explained_variance]
    print(f'[{tag}] losses max |err| {np.abs(np.array(got) - g[pre + "it0.losses"]).max():.3e}')
    np.testing.assert_allclose(got, g[pre + 'it0.losses'], **TOL)
    worst = 0.0
    for k, v in pol.state_dict().items():
        worst = max(worst, float(np.abs(_digest(v.cpu().numpy())[2:] - g[pre + 'it0.w.' + k][2:]).max()))
    print(f'[{tag}] updated weights, sampled elements: max |err| {worst:.3e}')
    for k, v in pol.state_dict().items():
        got, want = _digest(v.cpu().numpy()), g[pre + 'it0.w.' + k]
        np.testing.assert_allclose(got[2:], want[2:], err_msg=k, rtol=1e-5, atol=max(1e-5, 0.03 * hp[0]))   # the sampled elements
        np.testing.assert_allclose(got[:2], want[:2], rtol=0, atol=1e-5 * max(1.0, want[1]), err_msg=k + ' (sums)')


# ------------------------------------------------------------------------------------------ 5. a reference-built module
def test_reference_built_module_behind_policy_gives_the_same_outputs():
    """A module with the reference class's names (value head `value`, no recorded frame shape) wrapped in cleanrl.Policy: through
    create() it adopts the vecenv's frame shape and computes what models.ProcgenResnet computes with the same weights."""
    from pufferlib_amd import clean_pufferl, cleanrl, models
    from test_gpu_ppo import _config
    tag, n = 'tiny', 4
    obs = rr.SHAPES[tag]['obs']
    twin, w = _net(tag, module=rr.reference_module(tag))
    assert models.find_resnet(twin) is twin and models.find_cnn(twin) is None
    frames, noise = rr.frames(tag, n), rr.noise_for(tag, n)
    host = _Replay(frames.reshape(1, n, -1), np.zeros((1, n), np.float32), np.zeros((1, n), np.float32), obs, A)
    pol = cleanrl.Policy(twin)
    with pytest.raises(ValueError, match='frame shape'):
        pol(torch.from_numpy(frames), noise=torch.from_numpy(noise))        # on its own it cannot know (H, W)
    data = clean_pufferl.create(_config(n, 4, 16, 2, 1, 160, HP, seed=3, env='frames'), host, pol)
    assert data.flat_params.geometry.obs_shape == obs
    ours = cleanrl.Policy(_net(tag)[0])
    for x, y in zip(pol(torch.from_numpy(frames), noise=torch.from_numpy(noise)), ours(torch.from_numpy(frames), noise=torch.from_numpy(noise))):
        assert torch.equal(x, y)
