"""Autograd through policy(obs, action=...): cleanrl.Policy / RecurrentPolicy built with autograd=True (general.Evaluator's autograd path,
csrc/general.hip's pfa_heads_rows_eval_backward) against torch autograd on the CPU in float64 over a restatement of the same policy
(tests/autograd_reference.py).

Bound of every comparison, per tensor: max |device - f64| <= max(4 e32, 1e-5 max(1, max |f64|)), e32 being what the restatement's own
fp32 run on the CPU loses against float64 on that case — measured, printed next to the device error ("[autograd f64]" lines), never
taken from the code under test.

Observed on an MI355X (largest over the tensors of a group: CPU fp32 err / device err / device err over bound; the table is in
docs/lab-notebook.md):
  kernel alone (all upstream | logprob | entropy | value only)  8.4e-7 / 1.3e-6 / 0.071   (value only: exact, 0 / 0)
  forward outputs logprob, entropy, value, h, c                 7.2e-7 / 1.1e-6 / 0.042
  random linear loss, every .grad                               2.6e-6 / 2.6e-6 / 0.044
  PPO loss in torch ops, every .grad                            1.1e-7 / 1.3e-7 / 0.013
  recorded Squared minibatch: autograd, trainer, one vs other   4.3e-8 / 4.3e-8 / 0.004
  whole hand-written step vs float64 and vs train()             1.4e-8 / 1.4e-8 / 0.0015  (weights moved 2.5e-4)
The device sits at the CPU's own fp32 error; 4 e32 never exceeded the floor, 1e-5 of the tensor's largest entry (at least 1e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

import autograd_reference as R

gpu = pytest.mark.gpu
HP = [2.5e-4, 0.99, 0.95, R.PPO['clip_coef'], R.PPO['vf_coef'], R.PPO['vf_clip_coef'], 0.5, R.PPO['ent_coef']]
CASES = {c.tag: c for c in R.cases()}
_refs = {}


def _reference(case, loss):
    """The float64 / fp32 reference of (case, loss), computed once on the CPU and left unchanged."""
    key = (case.tag, loss.__name__)
    if key not in _refs:
        torch.set_num_threads(4)
        _refs[key] = R.Reference(case, loss)
    return _refs[key]


def _short(name):
    """Module parameter name -> the reference's: policy.encoder.weight, policy.policy.encoder.weight, policy.recurrent.weight_ih_l0."""
    for prefix in ('policy.recurrent.', 'policy.policy.', 'policy.'):
        if name.startswith(prefix):
            return name[len(prefix):]
    raise KeyError(name)


def _heads_read(base, width):
    """As in the reference, the heads under LSTMWrapper(input_size, hidden_size) read hidden_size features: a Default whose encoder is
    wider than the LSTM gets heads of the LSTM's width."""
    if base.value_head.in_features != width:
        base.decoder = torch.nn.Linear(width, base.decoder.out_features)
        base.value_head = torch.nn.Linear(width, 1)


def _policy(case, autograd, **kw):
    """The cleanrl wrapper over the case's module with the case's weights."""
    from pufferlib_amd import cleanrl, models
    env = R.Env(case.obs_dim, case.nvec, case.multi)
    base = models.Default(env, hidden_size=case.hidden)
    if case.lstm:
        _heads_read(base, case.lstm[1])
        pol =cleanrl.RecurrentPolicy(models.LSTMWrapper(env, base, input_size=case.lstm[0], hidden_size=case.lstm[1]), autograd=autograd, **kw)
    else:
        pol = cleanrl.Policy(base, autograd=autograd, **kw)
    _load(pol, case.params)
    return pol


def _load(pol, params):
    with torch.no_grad():
        for name, p in pol.named_parameters():
            p.copy_(torch.as_tensor(params[_short(name)]).to(p.device))


def _call(pol, case):
    """policy(obs, action=...) on the case: (action, logprob, entropy, value, state or None)."""
    obs, acts = torch.as_tensor(case.obs).cuda(), torch.as_tensor(case.actions_for_policy()).cuda()
    if not case.lstm:
        return pol(obs, action=acts) + (None,)
    state = None if case.state is None else tuple(torch.as_tensor(s).cuda() for s in case.state)
    if case.TT > 1:                                     # (B, TT, obs...) with the observation shape the wrapper recorded from its env
        obs, acts = obs.view(case.B, case.TT, *pol.policy.obs_shape), acts.view(case.B, case.TT)
    return pol(obs, state, action=acts)


def _grads(pol):
    return {_short(n): p.grad.detach().cpu().numpy() for n, p in pol.named_parameters()}


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel alone
def _heads_word(nvec):
    return sum(n << (4 * h) for h, n in enumerate(nvec)) if len(nvec) > 1 else 0


@gpu
@pytest.mark.parametrize('nvec', [[3], [3, 2, 5], [63], [15, 15, 15, 15], [2] * 8])
@pytest.mark.parametrize('upstream', ['all', 'logprob', 'entropy', 'value'])
def test_eval_backward_kernel_matches_float64_autograd_of_sample_logits(nvec, upstream):
    """pfa_heads_rows_eval_backward on random head outputs and random upstream triples — and with only one of the three given, the
    others null pointers — against float64 autograd of the oracle's sample_logits; 300 rows (two blocks), row 0 with one logit 30 above
    the rest (p log p of the others underflows towards 0).  dout sits inside a NaN-filled buffer with a row stride wider than num_out:
    columns num_actions + 1 .. num_out - 1 are exactly 0, columns beyond num_out and everything around the rows stay NaN."""
    from pufferlib_amd import _lib
    from oracle import ppo_torch
    L = _lib.lib()
    A, rows = sum(nvec), 300
    NO, multi = (A + 1 + 15) // 16 * 16, len(nvec) > 1
    ldd = NO + 16
    g = torch.Generator().manual_seed(100 + A)
    out = torch.zeros(rows, NO)
    out[:, :A + 1] = torch.randn(rows, A + 1, generator=g) * 2
    out[0, :nvec[0]] = torch.randn(nvec[0], generator=g) * 0.1
    out[0, 1] += 30.0
    acts = torch.stack([torch.randint(0, n, (rows,), generator=g) for n in nvec], dim=1)
    acts[0, 0] = 0                                                          # (the chosen action of the dominant row is NOT the dominant one)
    ups = {k: torch.randn(rows, generator=g) for k in ('logprob', 'entropy', 'value')}
    given = {k: (v if upstream in ('all', k) else None) for k, v in ups.items()}
    cols = np.cumsum([0] + nvec)

    def want(dtype):
        o = out.to(dtype).requires_grad_(True)
        logits = [o[:, cols[h]:cols[h + 1]] for h in range(len(nvec))]
        _, lp, ent = ppo_torch.sample_logits(logits if multi else logits[0], action=acts if multi else acts[:, 0])
        terms = dict(logprob=lp, entropy=ent, value=o[:, A])
        sum((given[k].to(dtype) * terms[k]).sum() for k in terms if given[k] is not None).backward()
        return o.grad.double().numpy()
    w64, w32 = want(torch.float64), want(torch.float32)
    e32 = float(np.abs(w32 - w64).max())
    bound = R.bound(e32, w64)
    buf = torch.full((rows + 2, ldd), float('nan'), device='cuda')
    packed = sum(acts[:, h] << (4 * h) for h in range(len(nvec))) if multi else acts[:, 0]
    dev = lambda t: None if t is None else t.cuda()     # noqa: E731
    ga, ge, gv = dev(given['logprob']), dev(given['entropy']), dev(given['value'])
    out_d, packed_d = out.cuda(), packed.cuda().contiguous()               # (named: a temporary's memory is free for the next allocation)
    _lib.check(L.pfa_heads_rows_eval_backward(_lib.ptr(out_d), NO, rows, A, _heads_word(nvec), _lib.ptr(packed_d), _lib.ptr(ga),
                                              _lib.ptr(ge), _lib.ptr(gv), _lib.ptr(buf[1]), ldd, NO, None), 'heads_rows_eval_backward')
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    err = float(np.abs(got[1:rows + 1, :A + 1].astype(np.float64) - w64[:, :A + 1]).max())
    print(f'[autograd f64] kernel heads {nvec} upstream {upstream:<8} cpu-fp32 err {e32:.3e}  device err {err:.3e}  bound {bound:.3e}')
    assert err <= bound
    assert np.array_equal(got[1:rows + 1, A + 1:NO].view(np.uint32), np.zeros((rows, NO - A - 1), np.uint32)), 'padding columns must be exactly 0'
    assert np.isnan(got[1:rows + 1, NO:]).all() and np.isnan(got[0]).all() and np.isnan(got[rows + 1]).all(), 'written outside dout'


# ------------------------------------------------------------------------------------------------------------ 2. forward identity
@gpu
@pytest.mark.parametrize('tag', list(CASES))
def test_autograd_forward_is_bit_identical_to_the_plain_call(tag):
    case = CASES[tag]
    plain, auto = _call(_policy(case, False), case), _call(_policy(case, True), case)
    for name, p, a in zip(('action', 'logprob', 'entropy', 'value'), plain, auto):
        assert torch.equal(p, a), name
        assert p.grad_fn is None and not p.requires_grad, name
        assert (a.grad_fn is not None) == (name != 'action'), name
    if case.lstm:
        for p, a in zip(plain[4], auto[4]):
            assert torch.equal(p, a) and a.grad_fn is None and not a.requires_grad      # the returned state carries no graph
    ref = _reference(case, R.linear_loss)
    got = dict(logprob=auto[1], entropy=auto[2], value=auto[3])
    if case.lstm:
        got.update(h=auto[4][0], c=auto[4][1])
    assert ref.failures({k: v.detach().cpu().numpy() for k, v in got.items()}, what='out') == []


# --------------------------------------------------------------------------------------------------------- 3. a random linear loss
@gpu
@pytest.mark.parametrize('tag', list(CASES))
def test_random_linear_loss_gradients_match_float64_and_accumulate(tag):
    """(u logprob + v entropy + w value).sum() with random per-row u, v, w: every parameter's .grad within the margin of the float64
    gradient and of the parameter's shape; a second backward() on a fresh call doubles .grad exactly (the launches are deterministic
    and x + x = 2 x)."""
    case = CASES[tag]
    ref = _reference(case, R.linear_loss)
    pol = _policy(case, True)
    assert all(p.grad is None for p in pol.parameters())
    _, lp, ent, val, _ = _call(pol, case)
    R.linear_loss(case, lp, ent, val).backward()
    for n, p in pol.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.is_cuda, n
    first = {n: p.grad.clone() for n, p in pol.named_parameters()}
    assert ref.failures(_grads(pol)) == []
    _, lp, ent, val, _ = _call(pol, case)
    R.linear_loss(case, lp, ent, val).backward()
    for n, p in pol.named_parameters():
        assert torch.equal(p.grad, 2 * first[n]), n


# ------------------------------------------------------------------------------------------------------ 4. the PPO loss in torch ops
@gpu
@pytest.mark.parametrize('tag', list(CASES))
def test_ppo_loss_in_torch_ops_matches_float64(tag):
    """clean_pufferl.py:202-238 written in torch ops on the returned tensors (ratio, clipped surrogate, clipped value loss, entropy
    bonus), old log-probabilities and values the float64 policy's own plus noise so that rows sit on both sides of every clip."""
    case = CASES[tag]
    ref = _reference(case, R.ppo_loss)
    pol = _policy(case, True)
    _, lp, ent, val, _ = _call(pol, case)
    loss = R.ppo_loss(case, lp, ent, val)
    loss.backward()
    assert abs(loss.item() - ref.r64['loss']) <= max(4 * abs(ref.r32['loss'] - ref.r64['loss']), 1e-5)
    assert ref.failures(_grads(pol)) == []


N_ENVS, HORIZON = 16, 8


def _trained(kind, autograd, hidden=48):
    """create + evaluate on vector.Squared 3 x 3 (rows of 9 floats, 8 actions), 16 envs x 8 steps, one minibatch, one epoch; then
    train(): (data, policy, start weights by short name, weights after train())."""
    from pufferlib_amd import clean_pufferl, cleanrl, models, vector
    from test_gpu_ppo import _config
    vec = vector.make(vector.make_squared, env_kwargs=dict(distance_to_target=1, num_targets=1), num_envs=N_ENVS, backend=vector.Squared)
    torch.manual_seed(5)
    base = models.Default(vec.driver_env, hidden_size=hidden)
    if kind == 'lstm':
        _heads_read(base, 32)
        pol = cleanrl.RecurrentPolicy(models.LSTMWrapper(vec.driver_env, base, input_size=hidden, hidden_size=32), autograd=autograd)
    else:
        pol = cleanrl.Policy(base, autograd=autograd)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    B = N_ENVS * HORIZON
    data = clean_pufferl.create(_config(N_ENVS, HORIZON, B, HORIZON, 1, B * 10, HP), vec, pol)
    w0 = {_short(n): p.detach().cpu().numpy().copy() for n, p in pol.named_parameters()}
    clean_pufferl.evaluate(data)
    clean_pufferl.train(data)
    torch.cuda.synchronize()
    w1 = {_short(n): p.detach().cpu().numpy().copy() for n, p in pol.named_parameters()}
    return data, pol, w0, w1


def _recorded(tag, data, w0, hidden, lstm):
    """The one minibatch train() just used (all 128 rows, env-major = segment-major) as a reference case."""
    e = data.experience
    cpu = lambda x: x.cpu().numpy()      # noqa: E731
    B, TT = (N_ENVS, HORIZON) if lstm else (N_ENVS * HORIZON, 1)
    return R.recorded_case(tag, hidden, [8], B, TT, lstm, w0, cpu(e.obs)[:, :9], cpu(e.actions), cpu(e.logprobs), cpu(e.values), cpu(e.advantages),
                           cpu(e.returns))


@gpu
@pytest.mark.parametrize('kind,hidden', [('mlp', 48), ('lstm', 48), ('mlp', 128)])
def test_ppo_loss_gradient_equals_the_trainers_on_the_same_minibatch(kind, hidden):
    """The tie to train(): on the minibatch a rollout left in the experience buffers, the gradient of the torch-op PPO loss through the
    autograd path, the gradient general.Engine.update leaves in its flat buffer (Default(48), LSTMWrapper(48, 32): the GEMM path) or
    pfa_ppo_mlp_grad's (Default(128): the fused update), and the float64 gradient agree within the one measured margin."""
    from pufferlib_amd import _lib, clean_pufferl
    data, pol, w0, _ = _trained(kind, True, hidden)
    _load(pol, w0)                                       # back to the weights the rollout ran with; train() left GAE and adv_stats
    lstm = (48, 32) if kind == 'lstm' else None
    case = _recorded(f'squared3x3-{kind}{hidden}', data, w0, hidden, lstm)
    ref = R.Reference(case, R.ppo_loss)
    e, fp = data.experience, data.flat_params
    B = e.batch_size
    hp = clean_pufferl._make_hparams(data.config, e)
    grads = torch.full_like(data.grads, float('nan'))
    if data.gen_engine is not None:
        assert data.gen_engine.wide_ws is None
        data.gen_engine.state = None
        data.gen_engine.update(0, hp, data.adv_stats, B, grads, B)
    else:
        _lib.check(_lib.lib().pfa_ppo_mlp_grad(C.byref(e.c), B, 0, _lib.ptr(fp.flat), C.byref(fp.dims), C.byref(hp), _lib.ptr(data.adv_stats), B,
                                               _lib.ptr(grads), _lib.ptr(data.workspace), _lib.stream_handle()), 'ppo_grad')
    engine = {_short('policy.' + k): v.cpu().numpy() for k, v in fp.split(grads[:fp.count]).items()}     # (keys relative to the wrapped module)
    _, lp, ent, val, _ = _call(pol, case)
    R.ppo_loss(case, lp, ent, val).backward()
    mine = _grads(pol)
    assert set(mine) == set(engine)
    assert ref.failures(mine) == []
    assert ref.failures(engine) == [], 'the trainer\'s own gradient against float64'
    assert ref.failures(mine, against=engine) == [], 'autograd path against the trainer\'s gradient'
    # a step by somebody's torch optimizer on the module parameters reaches the packed operand copies the trainer's engine shares
    torch.optim.SGD(pol.parameters(), lr=0.5).step()
    assert not torch.equal(_call(pol, case)[1], lp)


# ------------------------------------------------------------------------------------------------------ 5. a custom loop end to end
@gpu
@pytest.mark.parametrize('hidden', [128, 48])
def test_hand_written_loop_moves_the_weights_like_train(hidden):
    """One rollout, then the same single optimizer step twice from the same weights: train(), and the ten-line loop — policy(obs,
    action=...), the PPO loss in torch ops, backward, clip_grad_norm_(0.5), torch.optim.Adam(lr, eps=1e-5).step().  Bound per tensor:
    4 x what the whole step loses in fp32 against float64 on the CPU.  Then policy(obs) and policy(obs, action=...) see the new weights
    (hidden 48: the GEMM path's packed operand copies are re-made although no engine made the step)."""
    data, pol, w0, w_train = _trained('mlp', False, hidden)
    case = _recorded(f'squared3x3-loop-{hidden}', data, w0, hidden, None)
    R.Reference(case, R.ppo_loss)                                        # (the margins check: the step is clear of every kink)
    torch.set_num_threads(4)
    w64, w32 = (R.optimizer_step(case, dt, HP[0], HP[6]) for dt in (torch.float64, torch.float32))
    mine = _policy(case, True)
    opt = torch.optim.Adam(mine.parameters(), lr=HP[0], eps=1e-5)
    before = _call(mine, case)
    R.ppo_loss(case, before[1], before[2], before[3]).backward()
    torch.nn.utils.clip_grad_norm_(mine.parameters(), HP[6])
    opt.step()
    got = {_short(n): p.detach().cpu().numpy() for n, p in mine.named_parameters()}
    bad = []
    for k, want in w64.items():
        e32 = float(np.abs(w32[k] - want).max())
        bound = R.bound(e32, want)
        err, err_train, moved = (float(np.abs(np.asarray(x, np.float64) - y).max()) for x, y in ((got[k], want), (got[k], w_train[k]), (got[k], w0[k])))
        print(f'[autograd f64] {case.tag:<22} step  {k:<20} cpu-fp32 err {e32:.3e}  loop-vs-f64 {err:.3e}  loop-vs-train() {err_train:.3e}  '
              f'bound {bound:.3e}  moved {moved:.3e}')
        if not (err <= bound and err_train <= bound and moved > 2 * bound):
            bad.append(k)
    assert bad == []
    # the next calls read the stepped weights: values of the float64 policy over w64 on the same rows
    case.params = {k: v.astype(np.float32) for k, v in w64.items()}
    with torch.no_grad():
        want = R.forward(case, torch.float64)
    obs = torch.as_tensor(case.obs).cuda()
    sampled = mine(obs)
    after = _call(mine, case)
    for name, t, w in (('policy(obs) value', sampled[3], want['value']), ('policy(obs, action) value', after[3], want['value']),
                       ('policy(obs, action) logprob', after[1], want['logprob'])):
        np.testing.assert_allclose(t.detach().cpu().numpy(), w.numpy(), rtol=1e-5, atol=1e-5, err_msg=name)
    assert sampled[3].grad_fn is None and after[3].grad_fn is not None
    assert not torch.equal(after[3], before[3])


# ---------------------------------------------------------------------------------------------------------------------- 6. guards
def test_autograd_is_off_by_default_and_is_an_explicit_constructor_switch():
    from pufferlib_amd import cleanrl, models
    env = R.Env(5, [3], False)
    assert cleanrl.Policy(models.Default(env)).autograd is False
    assert cleanrl.RecurrentPolicy(models.LSTMWrapper(env, models.Default(env))).autograd is False
    assert cleanrl.Policy(models.Default(env), seed=3, autograd=True).autograd is True
    assert cleanrl.RecurrentPolicy(models.LSTMWrapper(env, models.Default(env)), autograd=True).autograd is True


def test_conv_encoders_refuse_autograd_by_name():
    """The cnn kind of the GEMM path (recurrent NatureCNN; 16..63 actions) has no backward wired to the autograd path: said at construction."""
    import types
    from pufferlib_amd import cleanrl, models
    env = types.SimpleNamespace(single_observation_space=types.SimpleNamespace(shape=(4, 84, 84), dtype=np.uint8),
                                single_action_space=types.SimpleNamespace(n=18))
    conv = models.Convolutional(env, framestack=4)
    for make in (lambda: cleanrl.RecurrentPolicy(models.LSTMWrapper(env, conv, input_size=512, hidden_size=512), autograd=True),
                 lambda: cleanrl.Policy(conv, autograd=True)):
        with pytest.raises(NotImplementedError, match='autograd=True with a convolutional encoder'):
            make()
    cleanrl.Policy(conv)                                 # the default keeps constructing


@gpu
@pytest.mark.parametrize('tag', ['default-h48-d3', 'lstm48x32-B5-TT3', 'flat-default128'])
def test_no_grad_and_sampling_calls_take_the_plain_path(tag):
    case = CASES[tag]
    pol = _policy(case, True)
    with torch.no_grad():
        out = _call(pol, case)
    assert all(t.grad_fn is None and not t.requires_grad for t in out[:4])
    obs = torch.as_tensor(case.obs).cuda()
    if case.lstm:
        state = tuple(torch.as_tensor(s).cuda() for s in case.state)
        sampled = pol(obs.view(case.B, case.TT, -1)[:, 0], tuple(s.clone() for s in state))
    else:
        sampled = pol(obs)
    assert all(t.grad_fn is None and not t.requires_grad for t in sampled[:4])
    graph = _call(pol, case)
    assert graph[1].grad_fn is not None and torch.equal(graph[1], out[1])
