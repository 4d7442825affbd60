"""vector.CartPole (csrc/cartpole_env.hpp, csrc/cartpole.hip): classic-control cart-pole on the device.  The protocol kernels
against the numpy float64 walker of tests/cartpole_reference.py bit for bit (f64 state included), fused rollouts == stepwise pieces
bit for bit for Default at every tile width and for the recurrent policy, one update against the torch-fp32 oracle trainer,
learning through create / evaluate / train, the refusals, and fused-faster-than-stepwise."""
import os
import sys

import numpy as np
import pytest
import torch

from adam_moments import assert_moments_match

sys.path.insert(0, os.path.dirname(__file__))
import cartpole_reference as cr  # noqa: E402
from test_cartpole_cpu import RANDOM_BASELINE  # noqa: E402

pytestmark = pytest.mark.gpu

HP = [1e-3, 0.97, 0.9, 0.2, 0.5, 0.2, 0.5, 0.02]
WIDTHS = [128, 64, 256, 512]          # 128: the flat buffer of the fused-kernel policy; the others: a pfa_mlp_view of the module's tensors


def _make(n, max_steps=500, velocities=True, **kw):
    from pufferlib_amd import vector
    return vector.make(vector.make_cartpole, env_kwargs=dict(max_steps=max_steps, velocities=velocities), num_envs=n, backend=vector.CartPole, **kw)


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize('setting', [dict(max_steps=500), dict(max_steps=12), dict(velocities=False)], ids=['limit500', 'limit12', 'no_velocities'])
def test_protocol_path_equals_the_walker_bit_for_bit(setting):
    """40 envs (two and a half 16-env tiles), 200 sends of numpy-drawn actions, info_mode 'sync': observations, rewards, terminals as
    bit patterns, the info dicts, the f64 state and the counters after every send, the episode_stats sums at the end — all equal to the
    float64 walker's.  There is no tolerance: the device's f64 `+ - * /` (uncontracted, division by the expansion LLVM documents as
    correctly rounded) and its one f64 -> f32 conversion must round as numpy does.  Then envs 16..39 of the run are reproduced by a
    24-env vecenv with env_offset=16."""
    n, sends, seed = 40, 200, 11
    rng = np.random.default_rng(1)
    acts = rng.integers(0, 2, (sends, n))
    vec, ref = _make(n, **setting), cr.CartPoleSerial(n, **setting)
    assert vec.obs_stride == 16 and vec.observations.shape == (n, 4) and vec.single_action_space.n == 2
    vec.async_reset(seed)
    ref.async_reset(seed)
    trace, ep_lengths = [], []
    for k in range(sends + 1):
        o, r, te, trunc, info, ids, m = vec.recv()
        o2, r2, te2, trunc2, info2, ids2, m2 = ref.recv()
        o, r, te = o.cpu().numpy(), r.cpu().numpy(), te.cpu().numpy()
        assert o.shape == (n, 4) and np.array_equal(_u32(o), _u32(o2)), k
        assert not vec.obs_buf[:, 4:].any(), k                                      # the row's padding stays zero
        assert np.array_equal(_u32(r), _u32(r2)) and np.array_equal(te, te2) and not trunc.any() and m.all() and np.array_equal(ids, ids2), k
        assert info == info2, (k, info, info2)
        st, cn = vec.debug_states()
        st2, cn2 = ref.states()
        assert np.array_equal(_u64(st), _u64(st2)) and np.array_equal(cn, cn2), k
        if 'velocities' in setting:
            assert not o[:, [1, 3]].any() and st[:, [1, 3]].all(), k
        trace.append((o, r, te, st, cn))
        ep_lengths += [i['episode_length'] for i in info]
        if k < sends:
            vec.send(acts[k])
            ref.send(acts[k])
    sums = vec.episode_stats(reset=False).cpu().numpy()
    assert np.array_equal(sums, ref.sums) and sums[0] == len(ep_lengths) > 2 * n and sums[2] == sum(ep_lengths)
    if setting.get('max_steps') == 12:                                   # both kinds of episode end: the time limit and a fallen pole
        assert max(ep_lengths) == 12 and ep_lengths.count(12) > n and min(ep_lengths) < 12
    # envs 16 .. 39 as a vecenv of their own
    part = _make(24, env_offset=16, **setting)
    part.async_reset(seed)
    for k in range(sends + 1):
        o, r, te, st, cn = trace[k]
        po, pr, pte = part.observations.cpu().numpy(), part.rewards.cpu().numpy(), part.terminals.cpu().numpy()
        pst, pcn = part.debug_states()
        assert np.array_equal(_u32(po), _u32(o[16:])) and np.array_equal(_u32(pr), _u32(r[16:])) and np.array_equal(pte, te[16:]), k
        assert np.array_equal(_u64(pst), _u64(st[16:])) and np.array_equal(pcn, cn[16:]), k
        if k < sends:
            part.recv()
            part.send(acts[k, 16:])


def _snapshot(data, vec, recurrent=False):
    e = data.experience
    out = [x.clone() for x in (e.obs, e.actions, e.logprobs, e.values, e.rewards, e.dones, vec.obs_buf, vec.rewards, vec.terminals_u8,
                                vec.state)]
    if recurrent:
        out += [data.lstm_engine.lstm_h.clone(), data.lstm_engine.lstm_c.clone()]
    return out + [torch.as_tensor(x) for x in vec.debug_states()]


def _policy(vec, hidden, recurrent):
    from pufferlib_amd import cleanrl, models
    env = getattr(vec, 'driver_env', vec)          # a vecenv, or the spaces a policy is to be built for
    base = models.Default(env, hidden_size=hidden)
    return cleanrl.RecurrentPolicy(models.LSTMWrapper(env, base)) if recurrent else cleanrl.Policy(base)


def _expected_form(data, recurrent):
    from pufferlib_amd import clean_pufferl
    gen = data.gen_engine
    form = clean_pufferl.rollout_form(type(data.vecenv), gen is not None, recurrent, gen is not None and gen.mlp_view is not None)
    assert form == (clean_pufferl.FUSED_LSTM if recurrent else clean_pufferl.FUSED_MLP)


def _both_rollouts(hidden, recurrent, n=40, T=64, rollouts=2, **setting):
    """evaluate() (one persistent kernel) and the stepwise pieces on twin vecenvs and policies -> (snapshots per path, vecs, datas)."""
    from pufferlib_amd import clean_pufferl
    from test_gpu_ppo import _config
    runs, vecs, datas = [], [], []
    for fused in (True, False):
        torch.manual_seed(4)
        vec = _make(n, **setting)
        pol = _policy(vec, hidden, recurrent)
        with torch.no_grad():
            for p_ in pol.parameters():
                p_.add_(0.05 * torch.randn_like(p_))
        data = clean_pufferl.create(_config(n, T, n * T // 2, 16, 2, n * T * 10, HP, seed=5), vec, pol)
        assert (data.gen_engine is not None) == (hidden != 128 and not recurrent)
        _expected_form(data, recurrent)
        out = []
        for it in range(rollouts):
            if fused:
                stats, _ = clean_pufferl.evaluate(data)
            else:
                if recurrent:
                    data.lstm_engine.rollout_stepwise(T, None, pol.noise_seed, pol.noise_step, vec.env_offset)
                    vec.sends += T
                else:
                    clean_pufferl._rollout_stepwise(data, None, T, n)
                stats, _ = clean_pufferl._finish_evaluate(data, n, T)
            out.append(_snapshot(data, vec, recurrent) + [dict(stats)])
        runs.append(out)
        vecs.append(vec)
        datas.append(data)
    for it in range(rollouts):
        for k, (a, b) in enumerate(zip(runs[0][it][:-1], runs[1][it][:-1])):
            assert torch.equal(a, b), (it, k)
        assert runs[0][it][-1] == runs[1][it][-1] and runs[0][it][-1]['episode_length'] > 0
    for vec in vecs:                       # the episode finished by the last send, as last_infos reports it: one meaning on both paths
        vec._k_infos()
    for k in ('_fin', '_fin_ret', '_fin_len', '_fin_score'):
        assert torch.equal(getattr(vecs[0], k), getattr(vecs[1], k)), k
    return runs, vecs, datas


def _episode_lengths(dones):
    """Lengths of the episodes that begin and end inside an env-major [n][T] block of Experience.dones rows (row t holds the terminal
    flag recv() showed before step t, and is the auto-reset row where it is set: two set rows are an episode and one reset row apart)."""
    out = []
    for row in dones.cpu().numpy():
        ends = np.nonzero(row)[0]
        out += [int(b - a - 1) for a, b in zip(ends[:-1], ends[1:])]
    return out


def _against_the_walker(data, n, T, **setting):
    """The rollout's experience rows against the walker stepped with the actions the policy drew: bit for bit."""
    e = data.experience
    ref = cr.CartPoleSerial(n, **setting)
    ref.async_reset(5)
    acts = e.actions.view(n, T).cpu().numpy()
    for t in range(T):
        o, r, d, _, _, _, _ = ref.recv()
        assert np.array_equal(_u32(o), _u32(e.obs.view(n, T, 16)[:, t, :4].cpu().numpy())), t
        assert np.array_equal(r, e.rewards.view(n, T)[:, t].cpu().numpy()) and np.array_equal(d.astype(np.float32), e.dones.view(n, T)[:, t].cpu().numpy()), t
        ref.send(acts[:, t].astype(np.int64))


@pytest.mark.parametrize('hidden', WIDTHS)
def test_fused_mlp_rollout_equals_the_stepwise_protocol_path(hidden):
    """40 envs (two and a half 16-env tiles) x 64 steps, two rollouts, max_steps=24, once per hidden width — rollout_mlp_env_kernel<CartPoleRollEnv,
    16, 4, MW, MlpView> with MW = 2 (the flat 128-wide buffer as a view of itself), 1, 4, 8: experience rows, live buffers, device state
    (f64) and the four last-infos buffers torch.equal with _rollout_stepwise, and both kinds of episode end occurred."""
    n, T = 40, 64
    runs, vecs, datas = _both_rollouts(hidden, False, n, T, rollouts=2, max_steps=24)
    e = datas[0].experience
    assert e.obs.shape == (n * T, 16) and not e.obs[:, 4:].any() and e.obs[:, :4].abs().max() > 0.05
    assert int(e.actions.min()) == 0 and int(e.actions.max()) == 1
    lengths = _episode_lengths(e.dones.view(n, T))
    assert len(lengths) > n and max(lengths) == 24 and lengths.count(24) >= 1 and min(lengths) < 24, sorted(set(lengths))


def test_fused_recurrent_rollout_equals_rollout_stepwise():
    """The same equalities plus the carried LSTM state, on the partially observed task (velocities=False), max_steps=24."""
    n, T = 40, 64
    runs, vecs, datas = _both_rollouts(128, True, n, T, rollouts=2, max_steps=24, velocities=False)
    e = datas[0].experience
    assert e.obs.shape == (n * T, 16) and not e.obs[:, [1, 3]].any() and not e.obs[:, 4:].any() and e.obs[:, [0, 2]].abs().max() > 0.05
    st, _ = vecs[0].debug_states()
    assert st[:, [1, 3]].all()                                           # the velocities are there, only hidden
    lengths = _episode_lengths(e.dones.view(n, T))
    assert len(lengths) > n and max(lengths) == 24 and min(lengths) < 24


@pytest.mark.parametrize('hidden', [128, 64])
def test_one_update_against_the_oracle_trainer(hidden):
    """evaluate() + train() at width 128 (ppo_mlp_grad at stride 16) and 64 (pfa_ppo_wide_grad): the rollout's rows against the walker
    bit for bit, then losses, updated weights (rtol = atol = 1e-5) and Adam's moments against oracle.ppo_torch.Trainer running on the
    walker and fed the same rollout."""
    from pufferlib_amd import clean_pufferl
    from oracle import ppo_torch
    from test_gpu_ppo import _config, _step_major
    n, T = 40, 64
    torch.manual_seed(4)
    vec = _make(n, max_steps=24)
    pol = _policy(vec, hidden, False)
    with torch.no_grad():
        for p_ in pol.parameters():
            p_.add_(0.05 * torch.randn_like(p_))
    data = clean_pufferl.create(_config(n, T, n * T // 2, 16, 2, n * T * 10, HP, seed=5), vec, pol)
    _expected_form(data, False)
    w0 = {k[len('policy.'):]: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items()}
    clean_pufferl.evaluate(data)
    e = data.experience
    _against_the_walker(data, n, T, max_steps=24)
    B = n * T
    opol = ppo_torch.Policy(w0)
    with torch.no_grad():                                               # the rollout's values and log-probabilities are the oracle's
        logits, oval, _ = opol.forward(e.obs[:, :4].cpu())
        _, olp, _ = ppo_torch.sample_logits(logits, action=e.actions.cpu().long())
    np.testing.assert_allclose(e.values.cpu().numpy(), oval.reshape(-1).numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(e.logprobs.cpu().numpy(), olp.numpy(), rtol=1e-5, atol=1e-5)
    trn = ppo_torch.Trainer(opol, cr.CartPoleSerial(n, max_steps=24), batch_size=B, minibatch_size=B // 2, bptt_horizon=16, update_epochs=2,
                            learning_rate=HP[0], gamma=HP[1], gae_lambda=HP[2], clip_coef=HP[3], vf_coef=HP[4], vf_clip_coef=HP[5],
                            max_grad_norm=HP[6], ent_coef=HP[7], total_timesteps=B * 10, seed=5)
    trn.obs = torch.as_tensor(_step_major(e.obs, n, T)[:, :4].copy())
    trn.actions = _step_major(e.actions, n, T).astype(np.int64)
    trn.logprobs, trn.rewards, trn.dones, trn.values = (_step_major(x, n, T).copy() for x in (e.logprobs, e.rewards, e.dones, e.values))
    trn.global_step = data.global_step
    Lo = trn.train()
    clean_pufferl.train(data)
    L = data.losses
    np.testing.assert_allclose([L.policy_loss, L.value_loss, L.entropy, L.approx_kl], [Lo[k] for k in ('policy_loss', 'value_loss', 'entropy', 'approx_kl')],
                               rtol=1e-5, atol=1e-5)
    sd = pol.state_dict()
    for k, arr in opol.state_arrays().items():
        np.testing.assert_allclose(sd['policy.' + k].cpu().numpy(), arr, rtol=1e-5, atol=1e-5, err_msg=k)
    assert_moments_match(data, trn)


def _train(hidden, recurrent, updates, n=256, T=128, bptt=8, nmb=8, **setting):
    from pufferlib_amd import clean_pufferl, namespace
    torch.manual_seed(0)
    vec = _make(n, **setting)
    pol = _policy(vec, hidden, recurrent)
    B = n * T
    cfg = namespace(env='cartpole', seed=1, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * updates,
                    learning_rate=5e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95, update_epochs=4, norm_adv=True,
                    clip_coef=0.2, clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.2, max_grad_norm=0.5, ent_coef=0.01,
                    target_kl=None, batch_size=B, minibatch_size=B // nmb, bptt_horizon=bptt, compile=False,
                    checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='cartpole')
    data = clean_pufferl.create(cfg, vec, pol)
    _expected_form(data, recurrent)
    lengths = []
    for _ in range(updates):
        stats, _ = clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        lengths.append(float(stats['episode_length']))
    return lengths


# Learning thresholds.  Every figure is the mean length of the episodes that ended in one rollout of 256 envs x 128 steps.
# The hyper-parameters were first tried on the CPU — oracle.ppo_torch.Trainer on the numpy walker, 30 updates, numpy action noise:
# with learning rate 1e-2 and 4 minibatches Default(64) went 21.7 -> 336.6 and Default(128) 21.7 -> 440.5; without velocities
# Default(128) stayed at 49 .. 53 from rollout 7 on and LSTMWrapper(Default) reached 282.4 with bptt_horizon 16 (54.8 with 8).  On the
# device, under its own noise stream, those settings did not hold: Default(64) rose to 337 at rollout 17, fell back and ended at 159,
# and the LSTM was still at 47 after 30 updates.  PPO on this task is that sensitive to the noise, so the settings were then chosen on
# the device for what holds over three (policy, env) seeds per width — of 15 candidates only learning rate 5e-3 with 8 minibatches
# kept the last ten rollouts of all six runs above 195 (lowest 258; the oracle trainer on the walker ends at 494.6 and 450.0 with it
# under two numpy noise seeds) — and for the recurrent run over two seeds and 60 updates
# (learning rate 5e-3, 4 minibatches, bptt_horizon 16: last rollout 327 and 325, lowest of the last ten 240 and 199).
# The bars of the fully observed runs are the issue's: the last rollout above 195 (the classic "solved" length), the first within
# 2 x of the random policy's 22.397 (tests/test_cartpole_cpu.py).  On top of them, from the measured curves in the docstrings and with
# the margin of tests/test_gpu_tabular.py's thresholds — a tenth of the scale, here 50 of the 500 steps an episode can last — the last
# rollout must exceed the measured one - 50.  The recurrent run is held to the MLP's last value on the same task + half the measured gap.
UPDATES, MASKED_UPDATES = 30, 60
SOLVED, MARGIN = 195.0, 50.0
MEASURED_LAST = {64: 446.5, 128: 286.6}
MASKED_GAP = 326.9 - 49.9     # measured: last(LSTM) - last(MLP) on the task without velocities


@pytest.mark.parametrize('hidden', [64, 128])
def test_default_solves_cartpole(hidden):
    """Default(64) — the reference's classic_control policy — and Default(128) on max_steps=500, 30 updates, seed 1, both through the
    fused rollout (view form at 64, flat at 128).  Measured on the MI355X, every third rollout: Default(64) 22, 68, 162, 267, 445, 447,
    438, 336, 404, 274 and 446.5 at the last (lowest of the last ten 274.4); Default(128) 22, 66, 184, 330, 430, 285, 287, 396, 281, 372
    and 286.6 at the last (lowest of the last ten 281.3); the same curve on both runs; 0.04 s per run."""
    a, b = _train(hidden, False, UPDATES), _train(hidden, False, UPDATES)
    print('cartpole lengths, hidden', hidden, [round(x, 1) for x in a])
    assert a == b                                        # fixed seed: the same curve on two runs
    assert RANDOM_BASELINE / 2 < a[0] < RANDOM_BASELINE * 2, a[0]
    assert a[-1] > SOLVED, a[-5:]
    assert a[-1] > MEASURED_LAST[hidden] - MARGIN, a[-5:]


def test_the_recurrent_policy_beats_the_memoryless_one_without_velocities():
    """velocities=False: x and theta alone do not say which way the pole is moving, so Default(128) cannot balance it and
    LSTMWrapper(Default) (bptt_horizon 16) learns to; 60 updates, 4 minibatches, seed 1.  Measured on the MI355X, every third rollout:
    the MLP 22, 36, 45, 49, 50, 51, 52, 51, 48, 49, 50, 52, 51, 52, 51, 52, 50, 52, 54, 53 and 49.9 at the last; the LSTM 22, 23, 36, 45, 67,
    164, 204, 299, 397, 415, 437, 390, 338, 316, 339, 317, 362, 389, 240, 303 and 326.9 at the last: a gap of 277; 0.76 s per recurrent run."""
    mlp = _train(128, False, MASKED_UPDATES, nmb=4, velocities=False)
    a, b = (_train(128, True, MASKED_UPDATES, bptt=16, nmb=4, velocities=False) for _ in range(2))
    print('cartpole without velocities: mlp', [round(x, 1) for x in mlp], 'lstm', [round(x, 1) for x in a])
    assert a == b
    assert a[-1] > mlp[-1] + MASKED_GAP / 2, (a[-5:], mlp[-5:])


def test_refusals():
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace, spaces, vector
    from pufferlib_amd.exceptions import APIUsageError, ExtensionError
    from test_gpu_ppo import _config
    cfg = _config(16, 16, 128, 16, 1, 16 * 16 * 4, HP)
    # a policy with other than two actions: every fused entry point names the head it needs
    for hidden, recurrent, text in ((128, False, 'rollout_mlp_cartpole: the policy must have one Discrete\\(2\\) head'),
                                    (64, False, 'rollout_mlp_view_cartpole: the policy must have one Discrete\\(2\\) head'),
                                    (128, True, 'rollout_lstm_cartpole: the policy must have one Discrete\\(2\\) head')):
        vec = _make(16)
        three = namespace(single_observation_space=vec.single_observation_space, single_action_space=spaces.Discrete(3))
        data = clean_pufferl.create(cfg, vec, _policy(three, hidden, recurrent))
        with pytest.raises(ExtensionError, match=text):
            clean_pufferl.evaluate(data)
    # a MultiDiscrete policy: the device envs take one Discrete head
    vec = _make(16)
    md_env = namespace(single_observation_space=vec.single_observation_space, single_action_space=spaces.MultiDiscrete([2, 2]))
    with pytest.raises(NotImplementedError, match='MultiDiscrete'):
        clean_pufferl.create(cfg, vec, cleanrl.Policy(models.Default(md_env)))
    # a conv policy reads uint8 frames
    frames = vector.make_frames()
    with pytest.raises(NotImplementedError, match='uint8 frames'):
        clean_pufferl.create(cfg, _make(16), cleanrl.Policy(models.Convolutional(frames, framestack=4)))
    # the start states are keyed by (seed, global env): seeds must be consecutive
    vec = _make(4)
    with pytest.raises(APIUsageError, match='CartPole needs consecutive seeds'):
        vec.async_reset([3, 4, 6, 7])
    vec.async_reset([3, 4, 5, 6])
    # a negative time limit, and an action outside the head on the first send
    with pytest.raises(APIUsageError, match='max_steps must be >= 0'):
        _make(4, max_steps=-1)
    vec.recv()
    with pytest.raises(APIUsageError, match='Actions do not match'):
        vec.send(np.array([0, 1, 2, 0]))


def test_fused_rollout_is_faster_than_its_own_stepwise_path():
    """4096 envs x 32 steps, Default(128) and Default(64), HIP-event times, median of 5 after a warm-up: one persistent kernel against
    three launches per step."""
    from pufferlib_amd import clean_pufferl
    from test_gpu_ppo import _config
    n, T = 4096, 32
    for hidden in (128, 64):
        vec = _make(n)
        pol = _policy(vec, hidden, False)
        data = clean_pufferl.create(_config(n, T, n * T // 4, 16, 1, n * T * 100, HP, seed=5), vec, pol)
        key = lambda: clean_pufferl._lib.NoiseKey(pol.noise_seed, pol.noise_step)  # noqa: E731
        view = None if data.gen_engine is None else data.gen_engine.mlp_view
        assert (view is None) == (hidden == 128)

        def timed(fn, reps=5):
            ms = []
            for i in range(reps + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return float(np.median(ms[1:]))
        fused = timed(lambda: vec.fused_rollout_mlp(data.flat_params, data.experience, None, key(), clean_pufferl._lib.stream_handle(), view=view))
        stepwise = timed(lambda: clean_pufferl._rollout_stepwise(data, None, T, n))
        print(f'cartpole rollout 4096 x 32, hidden {hidden}: fused {fused:.3f} ms, stepwise {stepwise:.3f} ms, factor {stepwise / fused:.1f}')
        assert fused < stepwise, (hidden, fused, stepwise)
