"""policy(frames, action=...) and autograd=True for the feed-forward models.Convolutional in the conv engine (up to 15 actions):
pfa_cnn_heads_eval / pfa_cnn_heads_eval_backward (csrc/cnn_heads.hip), cnn.Engine.policy_eval / eval_backward and cleanrl.Policy, against
the reference's arithmetic restated in float64 on the CPU (tests/conv_autograd_reference.py over tests/conv_geometry.py) and against the
rollout's own bits.

Bound of every gradient comparison, per tensor: max |device - f64| <= max(4 e32, 1e-5 max(1, max |f64|)) (autograd_reference.bound), e32
being what the same chain in fp32 on the CPU loses against float64 on that case — measured, printed next to the device error
("[conv autograd f64]" lines; the table is in docs/lab-notebook.md), never taken from the code under test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import conv_autograd_reference as CR  # noqa: E402
import conv_geometry as cg  # noqa: E402

gpu = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)
HP = [2.5e-4, 0.99, 0.95, CR.PPO['clip_coef'], CR.PPO['vf_coef'], CR.PPO['vf_clip_coef'], 0.5, CR.PPO['ent_coef']]
_refs, _cases = {}, {}


def _case(tag, rows, first=None):
    key = (tag, rows, first)
    if key not in _cases:
        torch.set_num_threads(4)
        _cases[key] = CR.case(tag, rows, first)
    return _cases[key]


def _reference(case, loss):
    """The float64 / fp32 reference of (case, loss), computed once on the CPU and left unchanged."""
    key = (case.name, case.first, loss.__name__)
    if key not in _refs:
        torch.set_num_threads(4)
        _refs[key] = CR.Reference(case, loss)
    return _refs[key]


def _policy(tag, A, params, autograd):
    """cleanrl.Policy over models.Convolutional of geometry `tag` with the given weights (name -> numpy)."""
    from pufferlib_amd import cleanrl, models
    net = models.Convolutional(cg.Env(tag, A), **cg.GEOMETRIES[tag]['kwargs'])
    with torch.no_grad():
        for k, v in net.state_dict().items():
            assert tuple(v.shape) == params[k].shape, k
            v.copy_(torch.from_numpy(np.asarray(params[k], np.float32)))
    return cleanrl.Policy(net, autograd=autograd)


def _call(pol, case):
    return pol(torch.from_numpy(case.frames).cuda(), action=torch.from_numpy(case.acts).cuda())


def _grads(pol):
    return {n[len('policy.'):]: p.grad.detach().cpu().numpy() for n, p in pol.named_parameters()}


def _guarded(rows, cols=None, pad=8):
    """A NaN-filled device allocation with `pad` guard rows above and below the [rows] (or [rows][cols]) slice a kernel writes."""
    big = torch.full((rows + 2 * pad,) + ((cols,) if cols else ()), float('nan'), device='cuda')
    return big[pad:pad + rows], big, pad


def _untouched(big, pad, rows):
    return bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + rows:]).all())


def _head_data(H, A, rows):
    g = torch.Generator().manual_seed(17 * H + A)
    h = torch.relu(torch.randn(rows, H, generator=g))
    w = {'actor.weight': torch.randn(A, H, generator=g) * (1.0 / H ** 0.5), 'actor.bias': torch.randn(A, generator=g) * 0.1,
         'value_fn.weight': torch.randn(1, H, generator=g) * (1.0 / H ** 0.5), 'value_fn.bias': torch.randn(1, generator=g) * 0.1}
    actions = torch.randint(0, A, (rows,), generator=g)
    ups = {k: torch.randn(rows, generator=g) for k in ('logprob', 'entropy', 'value')}
    return h, w, actions, ups


def _heads_at(h, w, actions, dtype, given=None):
    """The heads at dtype as functions of the pre-ReLU hidden z (h = relu(z), z := h): outputs, and for `given` upstream gradients
    d / d head outputs [rows][A + 1] and d / dz masked by relu'."""
    z = h.to(dtype).clone().requires_grad_(True)
    hz = torch.relu(z)
    wd = {k: v.to(dtype) for k, v in w.items()}
    logits = hz @ wd['actor.weight'].t() + wd['actor.bias']
    value = (hz @ wd['value_fn.weight'].t() + wd['value_fn.bias']).flatten()
    logp = logits - logits.logsumexp(-1, keepdim=True)
    terms = dict(logprob=logp.gather(-1, actions.unsqueeze(-1)).squeeze(-1), entropy=-(logp.exp() * logp).sum(-1), value=value)
    out = {k: v.detach().double().numpy() for k, v in terms.items()}
    if given is not None:
        logits.retain_grad()
        value.retain_grad()
        sum((g.to(dtype) * terms[k]).sum() for k, g in given.items() if g is not None).backward()
        lg, vg = (t.grad if t.grad is not None else torch.zeros_like(t) for t in (logits, value))
        out['dout'] = torch.cat([lg, vg.unsqueeze(1)], dim=1).double().numpy()
        out['dh'] = (z.grad * (h > 0)).double().numpy()
    return out


def _ptrs(dw, A):
    from pufferlib_amd import _lib
    return (_lib.ptr(dw['actor.weight']), _lib.ptr(dw['actor.bias']), _lib.ptr(dw['value_fn.weight']), _lib.ptr(dw['value_fn.bias']), A)


# ------------------------------------------------------------------------------------------------------------ 1. the entry points alone
@gpu
@pytest.mark.parametrize('rows', [1, 50])                   # 50: three full 16-row tiles plus two rows
@pytest.mark.parametrize('H', [512, 128, 144, 272])         # the two instantiated widths, two that take the run-time loop
@pytest.mark.parametrize('A', [4, 15])
def test_eval_entry_points_at_each_width_vs_float64(H, A, rows):
    """pfa_cnn_heads_eval against float64 at 1e-5, pfa_cnn_heads_eval_backward's dout and dh against float64 autograd under the bound
    rule — all three upstream gradients, and each one alone with the other two null pointers — every output inside a NaN-filled
    allocation whose guard rows stay NaN."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    h, w, actions, ups = _head_data(H, A, rows)
    hd, ad = h.cuda(), actions.cuda()
    dw = {k: v.cuda().contiguous() for k, v in w.items()}
    want = _heads_at(h, w, actions, torch.float64)
    outs = {k: _guarded(rows) for k in ('logprob', 'entropy', 'value')}
    _lib.check(L.pfa_cnn_heads_eval(_lib.ptr(hd), H, rows, *_ptrs(dw, A), _lib.ptr(ad), _lib.ptr(outs['logprob'][0]), _lib.ptr(outs['entropy'][0]),
                                    _lib.ptr(outs['value'][0]), None), 'cnn_heads_eval')
    for k, (t, big, pad) in outs.items():
        np.testing.assert_allclose(t.cpu().numpy(), want[k], err_msg=k, **TOL)
        assert _untouched(big, pad, rows), k
    lp2, v2 = torch.empty(rows, device='cuda'), torch.empty(rows, device='cuda')          # the entropy is optional
    _lib.check(L.pfa_cnn_heads_eval(_lib.ptr(hd), H, rows, *_ptrs(dw, A), _lib.ptr(ad), _lib.ptr(lp2), None, _lib.ptr(v2), None), 'cnn_heads_eval')
    assert torch.equal(lp2, outs['logprob'][0]) and torch.equal(v2, outs['value'][0])
    for upstream in ('all', 'logprob', 'entropy', 'value'):
        given = {k: (v if upstream in ('all', k) else None) for k, v in ups.items()}
        w64, w32 = (_heads_at(h, w, actions, dt, given) for dt in (torch.float64, torch.float32))
        dout, dbig, dpad = _guarded(rows, 16)
        dh, hbig, hpad = _guarded(rows, H)
        dev = {k: (None if v is None else v.cuda()) for k, v in given.items()}
        _lib.check(L.pfa_cnn_heads_eval_backward(_lib.ptr(hd), H, rows, *_ptrs(dw, A), _lib.ptr(ad), _lib.ptr(dev['logprob']), _lib.ptr(dev['entropy']),
                                                 _lib.ptr(dev['value']), _lib.ptr(dout), _lib.ptr(dh), None), 'cnn_heads_eval_backward')
        got = dict(dout=dout.cpu().numpy(), dh=dh.cpu().numpy())
        assert np.isfinite(got['dout']).all() and np.isfinite(got['dh']).all(), 'elements of dout / dh left unwritten'
        assert np.array_equal(got['dout'][:, A + 1:].view(np.uint32), np.zeros((rows, 15 - A), np.uint32)), 'padding columns must be exactly 0'
        assert _untouched(dbig, dpad, rows) and _untouched(hbig, hpad, rows), 'written outside dout / dh'
        for k, g in (('dout', got['dout'][:, :A + 1]), ('dh', got['dh'])):
            e32 = float(np.abs(w32[k] - w64[k]).max())
            b = CR.bound(e32, w64[k])
            err = float(np.abs(g.astype(np.float64) - w64[k]).max())
            print(f'[conv autograd f64] kernel H{H} A{A} rows{rows} upstream {upstream:<8} {k:<5} cpu-fp32 err {e32:.3e}  device err {err:.3e}  bound {b:.3e}')
            assert err <= b, (upstream, k)


# ------------------------------------------------------------------------------------------------------- 2. same bits as the rollout
@gpu
@pytest.mark.parametrize('H', [512, 128, 144])
@pytest.mark.parametrize('A', [4, 15])
def test_eval_returns_the_bits_of_the_sampling_kernel_for_the_action_it_drew(H, A):
    from pufferlib_amd import _lib
    L = _lib.lib()
    rows = 50
    h, w, _, _ = _head_data(H, A, rows)
    w['actor.weight'] = w['actor.weight'] * 5.0                                           # (spread the logits)
    hd = h.cuda()
    dw = {k: v.cuda().contiguous() for k, v in w.items()}
    noise = torch.empty(rows, A).exponential_(1, generator=torch.Generator().manual_seed(A)).cuda()
    key = _lib.NoiseKey(1, 0)
    acts = torch.empty(rows, dtype=torch.int64, device='cuda')
    s_lp, s_ent, s_val, e_lp, e_ent, e_val = (torch.empty(rows, device='cuda') for _ in range(6))
    _lib.check(L.pfa_cnn_heads_sample(_lib.ptr(hd), H, rows, *_ptrs(dw, A), _lib.ptr(noise), C.byref(key), 0, _lib.ptr(acts), _lib.ptr(s_lp),
                                      _lib.ptr(s_ent), _lib.ptr(s_val), None), 'cnn_heads_sample')
    _lib.check(L.pfa_cnn_heads_eval(_lib.ptr(hd), H, rows, *_ptrs(dw, A), _lib.ptr(acts), _lib.ptr(e_lp), _lib.ptr(e_ent), _lib.ptr(e_val), None),
               'cnn_heads_eval')
    assert len(set(acts.tolist())) > 1
    assert torch.equal(e_lp, s_lp) and torch.equal(e_val, s_val)
    np.testing.assert_allclose(e_ent.cpu().numpy(), s_ent.cpu().numpy(), **TOL)


# ------------------------------------------------------------------------------------------------------------------ 3. the policy call
@gpu
@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])                 # hidden 128, 3-channel byte loader / hidden 512, 1 channel
@pytest.mark.parametrize('A', [4, 15])
def test_policy_call_scores_given_actions(tag, A):
    from test_gpu_conv_geometry import _net
    from pufferlib_amd import cleanrl
    n = 41
    net, w = _net(tag, A)
    w['actor.weight'] = w['actor.weight'] * 100.0            # (0.01-gain logits are all but uniform: spread them)
    with torch.no_grad():
        net.actor.weight.copy_(torch.from_numpy(w['actor.weight']))
    pol = cleanrl.Policy(net)
    frames = cg.frames(tag, n, first=100)
    noise = torch.empty(n, A).exponential_(1, generator=torch.Generator().manual_seed(A))
    dev_frames = torch.from_numpy(frames).cuda()
    a, lp, ent, val = pol(dev_frames, noise=noise)
    for chunk in (None, 16):                                 # 16: 16 + 16 + 9 rows (buffers stay sized for 41)
        if chunk:
            pol.cnn_engine.chunk = chunk
        a2, lp2, ent2, val2 = pol(dev_frames, action=a)
        assert a2 is a and val2.shape == (n, 1) and lp2.grad_fn is None
        assert torch.equal(lp2, lp) and torch.equal(val2, val)
        np.testing.assert_allclose(ent2.cpu().numpy(), ent.cpu().numpy(), **TOL)
    # other actions, frames and actions on the host: against float64
    other = ((a + 1) % A).cpu()
    w64 = {k: torch.from_numpy(v).double() for k, v in w.items()}
    _, _, _, h = cg.encode(tag, torch.from_numpy(frames), w64)
    _, value, _, logprob, entropy, _ = cg.heads(h, w64, actions=other)
    a3, lp3, ent3, val3 = pol(torch.from_numpy(frames), action=other)
    assert a3 is other and lp3.is_cuda
    np.testing.assert_allclose(lp3.cpu().numpy(), logprob.numpy(), **TOL)
    np.testing.assert_allclose(ent3.cpu().numpy(), entropy.numpy(), **TOL)
    np.testing.assert_allclose(val3.cpu().numpy().reshape(-1), value.numpy(), **TOL)
    for bad_value in (A, -1):
        bad = a.clone()
        bad[3] = bad_value
        with pytest.raises(IndexError, match=f'action out of range for Discrete\\({A}\\)'):
            pol(dev_frames, action=bad)
    with pytest.raises(ValueError):
        pol(dev_frames, action=a[:-1])


# ------------------------------------------------------------------------------------------------------------------ 4. after a rollout
@gpu
def test_scoring_the_rollouts_own_actions_returns_its_stored_logprobs_and_values():
    """vector.Frames at the crafter shape, 16 envs x 8 steps, create -> evaluate; then the whole batch in one call (the rollout ran 16
    rows a step): the stored log-probabilities and values bit for bit, so a first minibatch's ratio is exactly 1."""
    from test_gpu_conv_geometry import _trainer
    from pufferlib_amd import clean_pufferl
    vec, pol, data, _ = _trainer('crafter', 6, 16, 8, 1, 8)
    clean_pufferl.evaluate(data)
    e = data.experience
    a, lp, ent, val = pol(e.obs, action=e.actions)
    assert lp.shape == (128,) and val.shape == (128, 1)
    assert torch.equal(lp, e.logprobs) and torch.equal(val.reshape(-1), e.values)
    assert bool(((lp - e.logprobs).exp() == 1.0).all())
    assert len(set(e.actions.tolist())) > 1


# ------------------------------------------------------------------------------------------------------------------------ 5. gradients
@gpu
@pytest.mark.parametrize('loss', [CR.linear_loss, CR.ppo_loss], ids=['linear', 'ppo'])
@pytest.mark.parametrize('n', [3, 37])
@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])
def test_gradients_match_float64_and_accumulate(tag, n, loss):
    """Outputs and every parameter's .grad against float64; the autograd call returns the plain call's bits; a second backward() on a
    fresh call doubles .grad exactly (the launches are deterministic and x + x = 2 x)."""
    case = _case(tag, n)
    ref = _reference(case, loss)
    pol = _policy(tag, case.A, case.params, True)
    assert all(p.grad is None for p in pol.parameters())
    with torch.no_grad():
        plain = _call(pol, case)
    a, lp, ent, val = _call(pol, case)
    for name, p, g in zip(('logprob', 'entropy', 'value'), plain[1:], (lp, ent, val)):
        assert torch.equal(p, g) and p.grad_fn is None and g.grad_fn is not None, name
    assert val.shape == (n, 1)
    assert ref.failures(dict(logprob=lp.detach().cpu().numpy(), entropy=ent.detach().cpu().numpy(), value=val.detach().cpu().numpy()), what='out') == []
    value = loss(case, lp, ent, val)
    value.backward()
    assert abs(value.item() - ref.r64['loss']) <= max(4 * abs(ref.r32['loss'] - ref.r64['loss']), 1e-5 * max(1.0, abs(ref.r64['loss'])))
    for name, p in pol.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.is_cuda, name
    first = {name: p.grad.clone() for name, p in pol.named_parameters()}
    assert ref.failures(_grads(pol)) == []
    if loss is CR.linear_loss:
        _, lp, ent, val = _call(pol, case)
        loss(case, lp, ent, val).backward()
        for name, p in pol.named_parameters():
            assert torch.equal(p.grad, 2 * first[name]), name


@gpu
@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])
def test_a_loss_on_the_value_alone_matches_float64(tag):
    """The upstream gradients of logprob and entropy arrive as None: null pointers to the kernel; the actor's gradient is exactly 0."""
    case = _case(tag, 3)
    ref = _reference(case, CR.value_loss)
    pol = _policy(tag, case.A, case.params, True)
    _, lp, ent, val = _call(pol, case)
    CR.value_loss(case, lp, ent, val).backward()
    got = _grads(pol)
    assert ref.failures(got) == []
    assert not got['actor.weight'].any() and not got['actor.bias'].any() and got['value_fn.weight'].any()


@gpu
@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])
def test_ppo_loss_gradient_equals_update_froms_on_the_same_minibatch(tag):
    """The tie to train(): the gradient of the torch-op PPO loss through the autograd path, the gradient cnn.Engine.update_from leaves
    in its flat buffer for the same minibatch (a fresh engine over the same weights) and the float64 gradient agree under the one rule."""
    from pufferlib_amd import _lib, cnn, models
    case = _case(tag, 37)
    n = case.rows
    ref = _reference(case, CR.ppo_loss)
    pol = _policy(tag, case.A, case.params, True)
    _, lp, ent, val = _call(pol, case)
    CR.ppo_loss(case, lp, ent, val).backward()
    mine = _grads(pol)
    cp = models.ConvParams(_policy(tag, case.A, case.params, False).policy, 'cuda')
    eng = cnn.Engine(cp, chunk=64)
    dev = {k: torch.as_tensor(v).cuda().contiguous() for k, v in dict(
        obs=case.frames.reshape(n, -1), actions=case.acts.astype(np.int32), lp=case.logprobs, v=case.values, adv=case.advantages, ret=case.returns,
        rew=np.zeros(n, np.float32), done=np.zeros(n, np.float32)).items()}
    exp = _lib.Experience(dev['obs'].data_ptr(), dev['actions'].data_ptr(), dev['lp'].data_ptr(), dev['v'].data_ptr(), dev['rew'].data_ptr(),
                          dev['done'].data_ptr(), dev['adv'].data_ptr(), dev['ret'].data_ptr(), 1)
    hp = _lib.PpoHparams(HP[3], HP[5], HP[4], HP[7], 1, 1, 1, 1)           # one minibatch of one-step segments: minibatch row q = batch row q
    adv = case.advantages.astype(np.float64)
    stats = torch.tensor([[adv.sum(), (adv ** 2).sum()]], dtype=torch.float64).cuda()
    grads = torch.full((cp.count + 16,), float('nan'), device='cuda')
    eng.update_from(exp, dev['obs'], n, 0, hp, stats, n, grads)
    engine = {k: v.cpu().numpy() for k, v in cp.split(grads[:cp.count]).items()}
    assert set(mine) == set(engine)
    assert ref.failures(mine) == []
    assert ref.failures(engine) == [], 'update_from\'s own gradient against float64'
    assert ref.failures(mine, against=engine) == [], 'autograd path against update_from\'s gradient'


# -------------------------------------------------------------------------------------------------------- 6. interleaving and staleness
@gpu
@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])
def test_two_interleaved_calls_back_propagate_their_own_frames(tag):
    """Two calls on different frames (37 and 3 rows), then both backward in reverse order: the first call's activations were
    overwritten by the second — its backward runs its forward again (the engine's generation counter)."""
    c1, c2 = _case(tag, 37, CR.OTHER[tag]), _case(tag, 3)
    r1, r2 = _reference(c1, CR.linear_loss), _reference(c2, CR.linear_loss)
    pol = _policy(tag, c1.A, c1.params, True)
    o1 = _call(pol, c1)
    gen = pol.cnn_engine.generation
    o2 = _call(pol, c2)
    assert pol.cnn_engine.generation == gen + 1
    CR.linear_loss(c2, *o2[1:]).backward()
    assert pol.cnn_engine.generation == gen + 1, 'the latest call\'s backward reads its own activations'
    assert r2.failures(_grads(pol)) == []
    pol.zero_grad(set_to_none=True)
    CR.linear_loss(c1, *o1[1:]).backward()
    assert pol.cnn_engine.generation == gen + 2, 'an overwritten call\'s backward runs its forward again'
    assert r1.failures(_grads(pol)) == []


@gpu
@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])
def test_a_torch_optimizer_step_reaches_the_packed_conv_operands(tag):
    """One torch.optim.SGD step on the nn.Parameters between two calls: the second call's outputs (scoring and sampling) are the
    float64 policy's at the stepped weights — the packed conv operands followed the parameters' version counters."""
    case = _case(tag, 3)
    pol = _policy(tag, case.A, case.params, True)
    _, lp, ent, val = _call(pol, case)
    CR.linear_loss(case, lp, ent, val).backward()
    torch.optim.SGD(pol.parameters(), lr=1e-3).step()                  # (moves the hidden vector by ~0.5 in float64)
    stepped = CR.Case(tag, case.rows, case.A, case.first, w={n[len('policy.'):]: p.detach().cpu().numpy() for n, p in pol.named_parameters()})
    moved = max(float(np.abs(stepped.params[k] - case.params[k]).max()) for k in ('network.0.weight', 'network.4.weight'))
    assert moved > 1e-4, moved
    with torch.no_grad():
        want = CR.forward(stepped, torch.float64)
    _, lp2, ent2, val2 = _call(pol, case)
    sampled = pol(torch.from_numpy(case.frames).cuda())
    assert not torch.equal(val2, val) and sampled[3].grad_fn is None
    for name, t, w in (('logprob', lp2, want['logprob']), ('entropy', ent2, want['entropy']), ('value', val2, want['value']),
                       ('policy(obs) value', sampled[3], want['value'])):
        np.testing.assert_allclose(t.detach().cpu().numpy(), w.numpy(), err_msg=name, **TOL)


# ------------------------------------------------------------------------------------------------------------------- 7. the whole step
@gpu
def test_hand_written_loop_moves_the_weights_like_train():
    """One rollout (vector.Frames at the crafter shape, 16 envs x 8 steps), then the same single optimizer step twice from the same
    weights: train() with one minibatch x one epoch, and the ten-line loop — policy(obs, action=...), the PPO loss in torch ops,
    backward, clip_grad_norm_(0.5), torch.optim.Adam(lr, eps=1e-5).step().  Bound per tensor: the rule on what the whole step loses in
    fp32 against float64 on the CPU."""
    from test_gpu_conv_geometry import _trainer
    from pufferlib_amd import clean_pufferl
    tag, A, N, T = 'crafter', 6, 16, 8
    vec, pol, data, w0 = _trainer(tag, A, N, T, 1, T, seed=2)
    clean_pufferl.evaluate(data)
    clean_pufferl.train(data)
    torch.cuda.synchronize()
    w_train = {n[len('policy.'):]: p.detach().cpu().numpy().copy() for n, p in pol.named_parameters()}
    e = data.experience
    cpu = lambda x: x.cpu().numpy()      # noqa: E731
    case = CR.Case(tag, N * T, A, w=w0, frames=cpu(e.obs).reshape(N * T, *cg.GEOMETRIES[tag]['obs']), actions=cpu(e.actions))
    case.name = 'crafter-rollout-128'
    case.set_experience(cpu(e.logprobs), cpu(e.values), cpu(e.advantages), cpu(e.returns))
    torch.set_num_threads(4)
    ref = CR.Reference(case, CR.ppo_loss, check=False)
    for name, (gap, err, need) in ref.margins().items():
        print(f'[conv autograd f64] {case.name} margin {name:<17} distance {gap:.3e}  fp32 chain error {err:.3e}  needs x{need:g}')
    ref.check_margins(relu=False)        # (the ReLU margins are printed only: no env seed clears them on 128 frames — conv_autograd_reference)
    w64, w32 = (CR.optimizer_step(case, dt, HP[0], HP[6]) for dt in (torch.float64, torch.float32))
    mine = _policy(tag, A, w0, True)
    opt = torch.optim.Adam(mine.parameters(), lr=HP[0], eps=1e-5)
    _, lp, ent, val = _call(mine, case)
    CR.ppo_loss(case, lp, ent, val).backward()
    torch.nn.utils.clip_grad_norm_(mine.parameters(), HP[6])
    opt.step()
    got = {n[len('policy.'):]: p.detach().cpu().numpy() for n, p in mine.named_parameters()}
    bad = []
    for k, want in w64.items():
        e32 = float(np.abs(w32[k] - want).max())
        b = CR.bound(e32, want)
        err, err_train, moved = (float(np.abs(np.asarray(x, np.float64) - y).max()) for x, y in ((got[k], want), (got[k], w_train[k]), (got[k], w0[k])))
        print(f'[conv autograd f64] {case.name} step  {k:<17} cpu-fp32 err {e32:.3e}  loop-vs-f64 {err:.3e}  loop-vs-train() {err_train:.3e}  '
              f'bound {b:.3e}  moved {moved:.3e}')
        if not (err <= b and err_train <= b and moved > 2 * b):
            bad.append(k)
    assert bad == []


# ------------------------------------------------------------------------------------------------------------------------- 8. guards
def _conv(A, tag='crafter'):
    from pufferlib_amd import models
    return models.Convolutional(cg.Env(tag, A), **cg.GEOMETRIES[tag]['kwargs'])


def test_the_feed_forward_conv_policy_admits_autograd_and_the_others_still_refuse_by_name():
    from pufferlib_amd import cleanrl, models
    assert cleanrl.Policy(_conv(4), autograd=True).autograd is True
    assert cleanrl.Policy(_conv(15), autograd=True).autograd is True
    assert cleanrl.Policy(_conv(4)).autograd is False
    env = cg.Env('crafter', 4)
    resnet_env = type('Env', (), dict(single_observation_space=type('Box', (), {'shape': (64, 64, 3), 'dtype': np.uint8})(),
                                      single_action_space=type('Discrete', (), {'n': 15})()))()
    for make in (lambda: cleanrl.Policy(_conv(18), autograd=True),
                 lambda: cleanrl.RecurrentPolicy(models.LSTMWrapper(env, _conv(4), input_size=128, hidden_size=128), autograd=True),
                 lambda: cleanrl.Policy(models.ProcgenResnet(resnet_env), autograd=True)):
        with pytest.raises(NotImplementedError, match='autograd=True with a convolutional encoder'):
            make()


@pytest.mark.parametrize('tag', ['crafter', 'vizdoom'])
def test_the_references_encode_is_conv_geometrys_in_float64(tag):
    """conv_autograd_reference.encode restates conv_geometry.encode with a dtype argument: in float64 the same bits; and the committed
    3-row cases keep their margins on this CPU."""
    case = _case(tag, 3)
    w64 = {k: torch.as_tensor(v).double() for k, v in case.params.items()}
    h, pre = CR.encode(tag, torch.as_tensor(case.frames), w64, torch.float64)
    info = {}
    assert torch.equal(h, cg.encode(tag, torch.as_tensor(case.frames), w64, info)[3])
    assert info['kink'] == min(float(z.abs().min()) for z in pre)
    for loss in (CR.linear_loss, CR.ppo_loss, CR.value_loss):
        assert _reference(case, loss).margins_ok()


def test_more_frames_than_one_chunk_in_autograd_mode_is_a_value_error_that_names_the_limit():
    """An autograd call is one chunk: cnn.Engine.check_one_chunk (what cleanrl.Policy asks before the forward) and Engine.eval_backward
    refuse more frames than the geometry's max_chunk, before anything is launched — the engine's buffers live on the CPU here."""
    from pufferlib_amd import cnn, models
    eng = cnn.Engine(models.ConvParams(_conv(4), 'cpu'), chunk=1)
    limit = eng.max_chunk
    assert limit > 1000
    eng.check_one_chunk(limit)
    for call in (lambda: eng.check_one_chunk(limit + 1), lambda: eng.eval_backward(None, limit + 1, None, None, None, None)):
        with pytest.raises(ValueError, match=str(limit)):
            call()
