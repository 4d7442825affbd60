"""Action heads beyond 63 logits (csrc/general.hip's wave-per-row kernels: one Discrete head of 64 .. 1024 logits; MultiDiscrete up
to 8 x 15 = 120 logits through the per-thread kernels) against the torch-fp32 oracle (oracle/ppo_torch.py), float64 autograd
(tests/autograd_reference.py, tests/conv_geometry.py) and a run of the unmodified reference (tests/golden/ppo_bandit_wide.npz):

  1. the row kernels on their own: sampled actions EXACTLY the oracle's (every row's float64 gap between the best and the second-best
     log p - log q is checked on the CPU first), log-probability / entropy / value at 1e-5, and eval's log-probability of the sampled
     action bit for bit the one sample returned;
  2. the loss kernel against torch autograd on the reference's loss, more than one 256-row block;
  3. policy(obs, action=...) with autograd=True on 200 logits: forward bits of the plain path, gradients against float64;
  4. Default(128) and LSTMWrapper(128, 128) on the device Bandit with 100 actions through create / evaluate / train;
  5. the reference's own run on make_bandit(num_actions=100);
  6. the NatureCNN with 100 actions, under LSTMWrapper and alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from adam_moments import assert_moments_match  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)
HP = [2.5e-4, 0.99, 0.95, 0.1, 0.5, 0.1, 0.5, 0.01]
ROWS = 259                   # two loss-sized blocks of rows, the second with three


def _heads_word(nvec):
    return sum(n << (4 * h) for h, n in enumerate(nvec))


def _f64_gap(logits, noise):
    """Smallest (best - second best) of log p - log q over the rows, float64."""
    lp = logits.double() - logits.double().logsumexp(dim=-1, keepdim=True)
    top = (lp - noise.double().log()).topk(2, dim=-1).values
    return float((top[:, 0] - top[:, 1]).min())


# nvec, seed: exactly one logit per lane; one lane with two; an odd count; uneven lanes with NO = 1008; the cap with NO = 1040; and the
# MultiDiscrete limit of the action packing through the per-thread kernels (seed: the first from 120 on whose gap clears 1e-3)
@pytest.mark.parametrize('nvec,seed', [([64], 64), ([65], 65), ([127], 128), ([1000], 1000), ([1024], 1024), ([15] * 8, 128)])
def test_wide_row_kernels_sample_and_score_like_the_oracle(nvec, seed):
    from pufferlib_amd import _lib
    from oracle import ppo_torch
    L = _lib.lib()
    A, rows = sum(nvec), ROWS
    NO = (A + 1 + 15) // 16 * 16
    multi = len(nvec) > 1
    heads = _heads_word(nvec) if multi else 0
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(rows, NO)
    out[:, :A + 1] = torch.randn(rows, A + 1, generator=g) * 2
    noise = torch.empty(rows, A).exponential_(1, generator=g)
    cols = np.cumsum([0] + nvec)
    logits = [out[:, cols[h]:cols[h + 1]] for h in range(len(nvec))]
    gap = min(_f64_gap(logits[h], noise[:, cols[h]:cols[h + 1]]) for h in range(len(nvec)))
    assert gap > 1e-3, f'a sampling row of this case is a near tie ({gap:.3e}): pick another seed'
    oa, olp, oent = ppo_torch.sample_logits(logits if multi else logits[0], noise=noise)
    d, nz = out.cuda(), noise.cuda()
    actions = torch.empty(rows, dtype=torch.int64, device='cuda')
    lp, ent, val = (torch.empty(rows, device='cuda') for _ in range(3))
    _lib.check(L.pfa_heads_rows_sample(_lib.ptr(d), NO, rows, A, heads, _lib.ptr(nz), None, 0, _lib.ptr(actions), _lib.ptr(lp),
                                       _lib.ptr(ent), _lib.ptr(val), None), 'sample')
    got = actions.cpu()
    if multi:
        got = torch.stack([(got >> (4 * h)) & 15 for h in range(len(nvec))], dim=1)
    assert torch.equal(got, oa), f'{int((got != oa).sum())} rows differ'              # no row left out
    print(f'[wide heads] {nvec if multi else A}: logprob max |err| {float((lp.cpu() - olp).abs().max()):.3e}  '
          f'entropy max |err| {float((ent.cpu() - oent).abs().max()):.3e}  f64 gap {gap:.3e}')
    np.testing.assert_allclose(lp.cpu().numpy(), olp.numpy(), **TOL)
    np.testing.assert_allclose(ent.cpu().numpy(), oent.numpy(), **TOL)
    assert torch.equal(val.cpu(), out[:, A])
    # the same rows scored with the sampled actions as GIVEN ones
    lp2, ent2, val2 = (torch.empty(rows, device='cuda') for _ in range(3))
    _lib.check(L.pfa_heads_rows_eval(_lib.ptr(d), NO, rows, A, heads, _lib.ptr(actions), _lib.ptr(lp2), _lib.ptr(ent2), _lib.ptr(val2), None), 'eval')
    if not multi:            # one softmax routine behind both wide kernels: approx_kl is exactly 0 on the first minibatch
        assert torch.equal(lp2, lp), 'eval and sample disagree on the log-probability of the same action'
        assert torch.equal(ent2, ent)
    np.testing.assert_allclose(lp2.cpu().numpy(), olp.numpy(), **TOL)
    np.testing.assert_allclose(ent2.cpu().numpy(), oent.numpy(), **TOL)
    assert torch.equal(val2.cpu(), out[:, A])


def test_wide_sampling_with_the_philox_key_draws_the_stream_of_the_oracle():
    """noise = None: the kernel draws Exp(1) in place from (row offset + row, column quad, step), the stream oracle/c_oracle.py restates
    on the CPU — the actions are the oracle's under that table (float64 gap checked first), and handing the kernel the table gives the
    same actions and log-probabilities."""
    from pufferlib_amd import _lib
    from oracle import c_oracle, ppo_torch
    L = _lib.lib()
    A, rows, NO, off = 200, 37, 208, 11
    g = torch.Generator().manual_seed(5)
    out = torch.zeros(rows, NO)
    out[:, :A + 1] = torch.randn(rows, A + 1, generator=g) * 2
    table = torch.as_tensor(c_oracle.philox_exp_noise(9, 3, rows, A, off))
    assert _f64_gap(out[:, :A], table) > 1e-3
    oa, olp, _ = ppo_torch.sample_logits(out[:, :A], noise=table)
    d = out.cuda()
    key = _lib.NoiseKey(9, 3)
    res = []
    for nz in (None, table.cuda().contiguous()):
        actions = torch.empty(rows, dtype=torch.int64, device='cuda')
        lp, ent, val = (torch.empty(rows, device='cuda') for _ in range(3))
        _lib.check(L.pfa_heads_rows_sample(_lib.ptr(d), NO, rows, A, 0, _lib.ptr(nz), C.byref(key), off, _lib.ptr(actions), _lib.ptr(lp),
                                           _lib.ptr(ent), _lib.ptr(val), None), 'sample')
        res.append((actions, lp, ent, val))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert torch.equal(res[0][0].cpu(), oa)
    np.testing.assert_allclose(res[0][1].cpu().numpy(), olp.numpy(), **TOL)


@pytest.mark.parametrize('A,time_major,N,T', [(200, False, 24, 8), (1024, True, 40, 16)])
def test_wide_row_loss_kernel_matches_autograd(A, time_major, N, T):
    """PPO loss sums and d loss / d (head outputs) of one minibatch against torch autograd on the reference's loss
    (clean_pufferl.py:202-238): 96 rows in minibatch order, and 320 time-major rows (two blocks, the second of one wave)."""
    from pufferlib_amd import _lib
    from oracle import ppo_torch
    L = _lib.lib()
    NO = (A + 1 + 15) // 16 * 16
    Th, nmb = 4, 2
    B = N * T
    M = B // nmb
    R = M // Th
    g = torch.Generator().manual_seed(7 + A)
    hp = _lib.PpoHparams(HP[3], HP[5], HP[4], HP[7], 1, 1, nmb, Th)
    acts = torch.randint(0, A, (B,), generator=g)
    dev = 'cuda'
    bufs = dict(actions=acts.to(torch.int32).to(dev), logprobs=(-np.log(A) + 0.1 * torch.randn(B, generator=g)).to(dev),
                values=torch.randn(B, generator=g).to(dev), rewards=torch.zeros(B, device=dev), dones=torch.zeros(B, device=dev),
                advantages=torch.randn(B, generator=g).to(dev), returns=torch.randn(B, generator=g).to(dev))
    obs = torch.zeros(B, 16, device=dev)
    exp = _lib.Experience(obs.data_ptr(), bufs['actions'].data_ptr(), bufs['logprobs'].data_ptr(), bufs['values'].data_ptr(), bufs['rewards'].data_ptr(),
                          bufs['dones'].data_ptr(), bufs['advantages'].data_ptr(), bufs['returns'].data_ptr(), T)
    mb = 1
    k = torch.arange(R)
    idx = ((mb + k[:, None] * nmb) * Th + torch.arange(Th)[None, :]).reshape(-1)           # minibatch order (row k*Th + t)
    order = idx.view(R, Th).t().reshape(-1) if time_major else idx                          # row order of the chunk handed to the kernel
    out = torch.zeros(M, NO)
    out[:, :A + 1] = torch.randn(M, A + 1, generator=g)
    out_t = out.clone().requires_grad_(True)
    _, newlogprob, entropy = ppo_torch.sample_logits(out_t[:, :A], action=acts[order])
    adv_all = bufs['advantages'].cpu()[idx]
    adv = bufs['advantages'].cpu()[order]
    a_n = (adv - adv_all.mean()) / (adv_all.std() + 1e-8)
    logratio = newlogprob - bufs['logprobs'].cpu()[order]
    ratio = logratio.exp()
    pg = torch.max(-a_n * ratio, -a_n * torch.clamp(ratio, 1 - HP[3], 1 + HP[3])).mean()
    nv = out_t[:, A]
    ret, val = bufs['returns'].cpu()[order], bufs['values'].cpu()[order]
    vl = 0.5 * torch.max((nv - ret) ** 2, (val + torch.clamp(nv - val, -HP[5], HP[5]) - ret) ** 2).mean()
    loss = pg - HP[7] * entropy.mean() + HP[4] * vl
    loss.backward()
    stats = torch.zeros(nmb, 2, dtype=torch.float64, device=dev)
    stats[mb, 0], stats[mb, 1] = float(adv_all.double().sum()), float((adv_all.double() ** 2).sum())
    dout = torch.full((M, NO), 7.0, device=dev)
    pairs = torch.zeros(16, device=dev)
    ws = torch.zeros(L.pfa_heads_rows_loss_workspace_bytes(M), dtype=torch.uint8, device=dev)
    out_d = out.to(dev)
    _lib.check(L.pfa_heads_rows_loss(_lib.ptr(out_d), NO, C.byref(exp), B, mb, 0, M, R if time_major else 0, A, 0, C.byref(hp), _lib.ptr(stats),
                                     M, _lib.ptr(dout), NO, NO, _lib.ptr(pairs), 0, _lib.ptr(ws), None), 'loss')
    np.testing.assert_allclose(dout.cpu().numpy()[:, :A + 1], out_t.grad.numpy()[:, :A + 1], rtol=1e-4, atol=1e-8)
    assert float(dout[:, A + 1:].abs().sum()) == 0.0
    sums = (pairs[0::2].double() + pairs[1::2].double()).cpu().numpy() / M
    np.testing.assert_allclose(sums[:3], [pg.item(), vl.item(), entropy.mean().item()], **TOL)


# ------------------------------------------------------------------------------------------------------------------ 3. autograd
_ref = {}


def _wide_case():
    """Default(64) on 5 observation values and 200 logits, 17 rows; seed: the first of 1, 2, ... at which both losses of
    tests/autograd_reference.py keep their margins on the CPU."""
    import autograd_reference as R
    if 'case' not in _ref:
        torch.set_num_threads(4)
        _ref['case'] = R.Case('default-h64-d200', 64, 5, [200], B=17, seed=1)
        _ref['linear'] = R.Reference(_ref['case'], R.linear_loss)
    return _ref['case'], _ref['linear']


def test_wide_eval_backward_through_the_policy_matches_float64_for_arbitrary_upstream_gradients():
    import autograd_reference as R
    from test_gpu_autograd import _call, _grads, _policy
    case, ref = _wide_case()
    plain, auto = _call(_policy(case, False), case), _call(_policy(case, True), case)
    for name, p, a in zip(('action', 'logprob', 'entropy', 'value'), plain, auto):
        assert torch.equal(p, a), name                                    # the plain path's bits
        assert p.grad_fn is None and (a.grad_fn is not None) == (name != 'action'), name
    assert ref.failures({k: v.detach().cpu().numpy() for k, v in dict(logprob=auto[1], entropy=auto[2], value=auto[3]).items()}, what='out') == []
    pol = _policy(case, True)
    _, lp, ent, val, _ = _call(pol, case)
    R.linear_loss(case, lp, ent, val).backward()                           # random per-row upstream triples (u, v, w)
    assert ref.failures(_grads(pol)) == []
    # a given action outside Discrete(200) is an IndexError on the host, as for the narrow heads
    bad = torch.as_tensor(case.actions_for_policy()).cuda().clone()
    bad[3] = 200
    with pytest.raises(IndexError):
        pol(torch.as_tensor(case.obs).cuda(), action=bad)


# ------------------------------------------------------------------------------------------------------------- 4. whole update
class _Blank:
    """Only the shape: for an oracle Trainer whose experience buffers the test fills itself."""

    def __init__(self, n, obs_dim):
        self.num_envs = n
        self.observations = np.zeros((n, obs_dim), np.float32)

    def async_reset(self, seed):
        pass


def _bandit(n, num_actions=100):
    from pufferlib_amd import vector
    return vector.make(vector.make_bandit, env_kwargs=dict(num_actions=num_actions), num_envs=n, backend=vector.WideBandit)


def _step_major(x, n, horizon):
    return x.view(n, horizon, *x.shape[1:]).transpose(0, 1).reshape(n * horizon, *x.shape[1:]).cpu().numpy()


@pytest.mark.parametrize('recurrent', [False, True])
def test_wide_bandit_rollout_and_update_vs_oracle(recurrent, matrix_products):
    """Default(hidden_size=128) [under LSTMWrapper(128, 128)] on the device Bandit with 100 actions, 16 envs x 16 steps, 2 minibatches x 2
    epochs: the stepwise rollout draws its noise in place (Philox key, no [T][N][A] tensor); its log-probabilities and values, then
    losses, post-update weights and Adam moments against the oracle trainer on the stored experience."""
    from pufferlib_amd import clean_pufferl, cleanrl, general, models
    from test_gpu_ppo import _config
    from oracle import ppo_torch
    n, horizon, nmb, bptt, A = 16, 16, 2, 8, 100
    B = n * horizon
    vec = _bandit(n, A)
    assert vec.single_action_space.n == A
    torch.manual_seed(3)
    base = models.Default(vec.driver_env, hidden_size=128)
    pol = cleanrl.RecurrentPolicy(models.LSTMWrapper(vec.driver_env, base, input_size=128, hidden_size=128)) if recurrent else cleanrl.Policy(base)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    data = clean_pufferl.create(_config(n, horizon, B // nmb, bptt, 2, B * 10, HP, env='bandit'), vec, pol)
    assert isinstance(data.flat_params, general.GeneralParams) and data.gen_engine is not None and data.gen_engine.net.NO == 112
    assert data.gen_engine.mlp_view is None and (data.gen_engine.net.lstm == (128, 128)) == recurrent
    sd = pol.state_dict()
    if recurrent:
        w0 = {k[len('policy.policy.'):]: v.cpu().numpy().copy() for k, v in sd.items() if k.startswith('policy.policy.')}
        w0.update({k[len('policy.recurrent.'):]: v.cpu().numpy().copy() for k, v in sd.items() if k.startswith('policy.recurrent.')})
    else:
        w0 = {k[len('policy.'):]: v.cpu().numpy().copy() for k, v in sd.items()}
    assert data.noise is None
    clean_pufferl.evaluate(data)
    assert getattr(data, '_noise_bufs', None) is None                      # nothing of [T][N][A] was materialised
    exp = data.experience
    opol = ppo_torch.Policy(w0, recurrent=recurrent)
    tr = ppo_torch.Trainer(opol, _Blank(n, 1), batch_size=B, minibatch_size=B // nmb, bptt_horizon=bptt, update_epochs=2, learning_rate=HP[0],
                           gamma=HP[1], gae_lambda=HP[2], clip_coef=HP[3], vf_coef=HP[4], vf_clip_coef=HP[5], max_grad_norm=HP[6], ent_coef=HP[7],
                           total_timesteps=B * 10, seed=1)
    tr.obs = torch.as_tensor(_step_major(exp.obs, n, horizon)[:, :1].copy()).float()
    tr.actions = _step_major(exp.actions, n, horizon).astype(np.int64)
    tr.logprobs, tr.rewards, tr.dones, tr.values = (_step_major(x, n, horizon).copy() for x in (exp.logprobs, exp.rewards, exp.dones, exp.values))
    assert tr.actions.min() >= 0 and tr.actions.max() < A and len(np.unique(tr.actions)) > 40
    assert np.array_equal(tr.obs.numpy(), np.ones((B, 1), np.float32))
    solution = int(np.random.RandomState(42).randint(0, A))
    odd = tr.dones.reshape(horizon, n)                                     # one step per episode, then the reset row
    assert np.array_equal(odd[1::2], np.ones_like(odd[1::2])) and not odd[0::2].any()
    hit = tr.actions.reshape(horizon, n)[0::2] == solution
    noise_table = np.array([x for x in _bandit_noise(n)], np.float64)
    assert np.array_equal(tr.rewards.reshape(horizon, n)[1::2], ((hit + noise_table[None, :]) * 1.0).astype(np.float32))
    with torch.no_grad():                                                  # the rollout's own numbers on the stored observations
        state, lps, vals = None, [], []
        for t in range(horizon):
            logits, v, state = opol.forward(tr.obs[t * n:(t + 1) * n], state)
            _, lp, _ = ppo_torch.sample_logits(logits, action=torch.as_tensor(tr.actions[t * n:(t + 1) * n]))
            lps.append(lp)
            vals.append(v.flatten())
    np.testing.assert_allclose(tr.logprobs, torch.cat(lps).numpy(), **TOL)
    np.testing.assert_allclose(tr.values, torch.cat(vals).numpy(), **TOL)
    if recurrent:
        np.testing.assert_allclose(data.gen_engine.lstm_h.cpu().numpy(), state[0].numpy(), **TOL)
    tr.global_step = data.global_step
    torch.set_num_threads(8)
    Lo = tr.train()
    clean_pufferl.train(data)
    Ld = data.losses
    got = [Ld.policy_loss, Ld.value_loss, Ld.entropy, Ld.old_approx_kl, Ld.approx_kl, Ld.clipfrac]
    print(f'[wide bandit{" lstm" if recurrent else ""}] losses', got)
    np.testing.assert_allclose(got, [Lo[k] for k in ('policy_loss', 'value_loss', 'entropy', 'old_approx_kl', 'approx_kl', 'clipfrac')], **TOL)
    sd = pol.state_dict()
    for k, arr in opol.state_arrays().items():
        name = ('policy.recurrent.' + k if k in ppo_torch.Policy.LSTM_NAMES else 'policy.policy.' + k) if recurrent else 'policy.' + k
        np.testing.assert_allclose(sd[name].cpu().numpy(), arr, err_msg=k, **TOL)
    assert_moments_match(data, tr)


def _bandit_noise(n, seed=42, num_actions=100, scale=1.0):
    """ocean.py:36-57: seed(42), one randint for the solution, then env i's reward noise is the i-th legacy gaussian."""
    rs = np.random.RandomState(seed)
    rs.randint(0, num_actions)
    return [rs.randn() * scale for _ in range(n)]


def test_first_minibatch_of_a_wide_update_has_zero_approx_kl():
    """One minibatch, one epoch: the update scores the rollout's actions under the rollout's weights, and the wide eval / loss kernels
    share sample's softmax — every ratio is exactly 1."""
    from pufferlib_amd import clean_pufferl, cleanrl, models
    from test_gpu_ppo import _config
    n, horizon, A = 16, 16, 100
    B = n * horizon
    vec = _bandit(n, A)
    torch.manual_seed(4)
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=128))
    data = clean_pufferl.create(_config(n, horizon, B, 8, 1, B * 10, HP, env='bandit'), vec, pol)
    clean_pufferl.evaluate(data)
    clean_pufferl.train(data)
    assert data.losses.approx_kl == 0.0 and data.losses.old_approx_kl == 0.0 and data.losses.clipfrac == 0.0


# ---------------------------------------------------------------------------------------------------------- 5. the reference's run
def _digest(a, samples=64):
    f = np.asarray(a, np.float64).reshape(-1)
    idx = np.linspace(0, f.size - 1, min(samples, f.size)).astype(np.int64)
    return np.concatenate([[f.sum(), np.abs(f).sum()], f[idx]])


def test_wide_bandit_replays_the_reference_golden(golden_dir, matrix_products):
    """tests/golden/ppo_bandit_wide.npz (make_golden_wide.py): the unmodified reference's create / evaluate / train with
    models.Default(128) behind frameworks.cleanrl.Policy on Serial(make_bandit(num_actions=100)), 8 envs x 16 steps, its multinomial's
    exponential draws as data.noise.  The device Bandit's trajectory and the actions exactly; log-probabilities, values, advantages,
    losses and updated weights at 1e-5."""
    import cnn_golden
    from pufferlib_amd import clean_pufferl, cleanrl, general, models
    from test_gpu_ppo import _config
    g = np.load(os.path.join(golden_dir, 'ppo_bandit_wide.npz'))
    n, horizon, mbs, bptt, epochs, total, iters = (int(x) for x in g['config'])
    hp = [float(x) for x in g['hparams']]
    A = int(g['num_actions'])
    assert A == 100 and float(g['it0.min_gap']) > 1e-4
    vec = _bandit(n, A)
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=128))
    with torch.no_grad():
        for k, v in pol.state_dict().items():
            v.copy_(torch.from_numpy(cnn_golden.cnn_start_weight(k[len('policy.'):], tuple(v.shape))))
            assert np.array_equal(_digest(v.numpy()), g['w0.' + k]), k
    data = clean_pufferl.create(_config(n, horizon, mbs, bptt, epochs, total, hp, seed=1, env='bandit'), vec, pol)
    assert isinstance(data.flat_params, general.GeneralParams)
    data.noise = torch.as_tensor(g['it0.noise'])                                                       # (T, N, A)
    clean_pufferl.evaluate(data)
    e = data.experience
    assert data.global_step == int(g['it0.global_step'])
    assert np.array_equal(_step_major(e.actions, n, horizon).astype(np.int64), g['it0.actions'].astype(np.int64))
    assert np.array_equal(_step_major(e.obs, n, horizon)[:, :1], g['it0.obs'].astype(np.float32).reshape(-1, 1))
    assert np.array_equal(_step_major(e.rewards, n, horizon), g['it0.rewards'])
    assert np.array_equal(_step_major(e.dones, n, horizon), g['it0.dones'])
    np.testing.assert_allclose(_step_major(e.logprobs, n, horizon), g['it0.logprobs'], **TOL)
    np.testing.assert_allclose(_step_major(e.values, n, horizon), g['it0.values'], **TOL)
    clean_pufferl.train(data)
    for m in range(e.num_minibatches):
        idx = e.minibatch_rows_index(m)
        np.testing.assert_allclose(e.advantages[idx].cpu().numpy(), g['it0.advantages'][m], **TOL)
    L = data.losses
    got = [L.policy_loss, L.value_loss, L.entropy, L.old_approx_kl, L.approx_kl, L.clipfrac, L.explained_variance]
    np.testing.assert_allclose(got, g['it0.losses'], **TOL)
    for k, v in pol.state_dict().items():
        got, want = _digest(v.cpu().numpy()), g['it0.w.' + k]
        np.testing.assert_allclose(got[2:], want[2:], err_msg=k, **TOL)                               # the sampled elements
        np.testing.assert_allclose(got[:2], want[:2], rtol=0, atol=1e-5 * max(1.0, want[1]), err_msg=k + ' (sums)')


# ------------------------------------------------------------------------------------------------------------------ 6. one conv case
@pytest.mark.parametrize('recurrent', [True, False])
def test_nature_cnn_with_100_actions_samples_like_float64(recurrent):
    """models.Convolutional, under LSTMWrapper and alone, at the smallest frame geometry of tests/conv_geometry.py (vizdoom: 60 x 80 x 1)
    with 100 actions on a host vecenv: policy(frames, noise=...) (from the zero state) against the float64 restatement (encoder and
    heads of conv_geometry.py, nn.LSTM in float64 in between), bound and gap rule of test_gpu_conv_geometry.py."""
    import conv_geometry as cg
    from host_vecenv import HostFrames
    from pufferlib_amd import cleanrl, general, models, spaces
    tag, A, n = 'vizdoom', 100, 7
    shape = cg.GEOMETRIES[tag]['obs']
    H = cg.hidden_of(tag)

    class HostWideFrames(HostFrames):                # the same protocol at this geometry's frame shape, Discrete(100)
        def __init__(self, num_envs):
            super().__init__(num_envs)
            self.single_observation_space = spaces.Box(low=0, high=255, shape=shape, dtype=np.uint8)
            self.single_action_space = spaces.Discrete(A)
            self.obs = np.zeros((num_envs, *shape), np.uint8)

        def _draw(self, idx):
            self.obs[idx] = cg.frames(tag, len(idx), first=100)
    vec = HostWideFrames(n)
    vec.async_reset(1)
    net = models.Convolutional(vec.driver_env, **cg.GEOMETRIES[tag]['kwargs'])
    w = cg.start_weights(tag, A)
    w['actor.weight'] = w['actor.weight'] * 100.0            # (0.01-gain logits are all but uniform: spread them)
    wrap = models.LSTMWrapper(vec.driver_env, net, input_size=H, hidden_size=H)
    lw = {k: cg.start_weight(k, tuple(v.shape)) for k, v in wrap.recurrent.state_dict().items()}
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.from_numpy(w[k]))
        for k, v in wrap.recurrent.state_dict().items():
            v.copy_(torch.from_numpy(lw[k]))
    pol = cleanrl.RecurrentPolicy(wrap) if recurrent else cleanrl.Policy(net)
    frames = vec.recv()[0]
    noise = torch.empty(n, A).exponential_(1, generator=torch.Generator().manual_seed(A))
    w64 = {k: torch.from_numpy(v).double() for k, v in w.items()}
    _, _, _, h = cg.encode(tag, torch.from_numpy(frames), w64)
    lstm = torch.nn.LSTM(H, H).double()
    with torch.no_grad():
        for k, v in lstm.state_dict().items():
            v.copy_(torch.from_numpy(lw[k]).double())
        y, (h1, c1) = lstm(h.unsqueeze(0))
    _, value, action, logprob, entropy, gap = cg.heads(y[0] if recurrent else h, w64, noise=noise)
    assert float(gap.min()) > 1e-4, 'a sampling row of this test is a near tie: pick another noise seed'
    if recurrent:
        a, lp, ent, val, state = pol(torch.from_numpy(frames).cuda(), None, noise=noise)
    else:
        a, lp, ent, val = pol(torch.from_numpy(frames).cuda(), noise=noise)
    assert isinstance(pol.flat_params, general.GeneralParams) and pol.flat_params.num_actions == A
    assert np.array_equal(a.cpu().numpy().reshape(-1), action.numpy())
    np.testing.assert_allclose(lp.cpu().numpy(), logprob.numpy(), **TOL)
    np.testing.assert_allclose(ent.cpu().numpy(), entropy.numpy(), **TOL)
    np.testing.assert_allclose(val.cpu().numpy().reshape(-1), value.numpy(), **TOL)
    with pytest.raises(AssertionError):                      # the shape assert of noise=
        pol(torch.from_numpy(frames).cuda(), noise=noise[:, :63])
    if recurrent:
        np.testing.assert_allclose(state[0].cpu().numpy(), h1.numpy(), **TOL)
        np.testing.assert_allclose(state[1].cpu().numpy(), c1.numpy(), **TOL)
