"""vector.Acrobot (csrc/acrobot_env.hpp, csrc/acrobot.hip, csrc/f64_sincos.hpp): classic-control acrobot on the device.  The protocol
kernels against the numpy float64 walker of tests/acrobot_reference.py bit for bit (f64 state included, every rare branch of the
step met), fused rollouts == stepwise pieces bit for bit for Default at every tile width and for the recurrent policy, one update
against the torch-fp32 oracle trainer, learning through create / evaluate / train, the refusals, and fused-faster-than-stepwise."""
import os
import sys

import numpy as np
import pytest
import torch

from adam_moments import assert_moments_match

sys.path.insert(0, os.path.dirname(__file__))
import acrobot_reference as ar  # noqa: E402
from test_acrobot_cpu import RANDOM_BASELINE, SET_AT, scripted_run  # noqa: E402

pytestmark = pytest.mark.gpu

HP = [1e-3, 0.97, 0.9, 0.2, 0.5, 0.2, 0.5, 0.02]
WIDTHS = [128, 64, 256, 512]          # 128: the flat buffer of the fused-kernel policy; the others: a pfa_mlp_view of the module's tensors
N, T = 40, 24                         # three 16-env workgroups, the last one half empty; under one 256-thread block of the send kernel


def _make(n, max_steps=500, velocities=True, **kw):
    from pufferlib_amd import vector
    return vector.make(vector.make_acrobot, env_kwargs=dict(max_steps=max_steps, velocities=velocities), num_envs=n, backend=vector.Acrobot, **kw)


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize('setting', [dict(max_steps=500), dict(max_steps=12), dict(velocities=False)], ids=['limit500', 'limit12', 'no_velocities'])
def test_protocol_path_equals_the_walker_bit_for_bit(setting):
    """40 envs, seed 11, info_mode 'sync', the scripted run of tests/test_acrobot_cpu.py (120 sends, 30 at max_steps=12): the actions are
    the energy-pumping rule computed on the host from the walker's state, and after send 14 envs 0..15 are put on the wrap, clamp,
    threshold and time-limit branches through debug_set_states.  Observations, rewards, terminals as bit patterns, the info dicts, the
    f64 state and the counters before every send, the episode_stats sums at the end — all equal to the float64 walker's.  There is no
    tolerance: the device's f64 `+ - * /` (uncontracted, division by the expansion LLVM documents as correctly rounded), its rint and
    its one f64 -> f32 conversion must round as numpy does.  The walker's counters say that the run met every branch.  At
    max_steps=12, envs 16..39 of the sends before the set are then reproduced by a 24-env vecenv with env_offset=16."""
    max_steps, velocities = setting.get('max_steps', 500), setting.get('velocities', True)
    vec = _make(N, **setting)
    assert vec.obs_stride == 16 and vec.observations.shape == (N, 6) and vec.single_action_space.n == 3
    vec.async_reset(11)
    trace, ep_lengths = [], []

    def each(k, ref, acts, branch):
        if branch is not None:
            vec.debug_set_states(*branch)
        o, r, te, trunc, info, ids, m = vec.recv()
        o2, r2, te2, trunc2, info2, ids2, m2 = ref.recv()
        o, r, te = o.cpu().numpy(), r.cpu().numpy(), te.cpu().numpy()
        assert o.shape == (N, 6) and np.array_equal(_u32(o), _u32(o2)), k
        assert not vec.obs_buf[:, 6:].any(), k                                      # the row's padding stays zero
        assert np.array_equal(_u32(r), _u32(r2)) and np.array_equal(te, te2) and not trunc.any() and m.all() and np.array_equal(ids, ids2), k
        assert info == info2, (k, info, info2)
        st, cn = vec.debug_states()
        st2, cn2 = ref.states()
        assert np.array_equal(_u64(st), _u64(st2)) and np.array_equal(cn, cn2), k
        if not velocities:
            assert not o[:, 4:].any() and st[:, 2:].any(1).all(), k           # the velocities are there, only hidden
        trace.append((o, r, te, st, cn))
        ep_lengths.extend(i['episode_length'] for i in info)
        vec.send(acts)

    ref, natural = scripted_run(max_steps, velocities, each)
    o, r, te = vec.observations.cpu().numpy(), vec.rewards.cpu().numpy(), vec.terminals.cpu().numpy()
    assert np.array_equal(_u32(o), _u32(ref.obs())) and np.array_equal(_u32(r), _u32(ref.rewards)) and np.array_equal(te, ref.terminals)
    assert vec.infos == ref.infos
    st, cn = vec.debug_states()
    assert np.array_equal(_u64(st), _u64(ref.states()[0])) and np.array_equal(cn, ref.states()[1])
    sums = vec.episode_stats(reset=False).cpu().numpy()
    assert np.array_equal(sums, ref.sums) and sums[0] >= 8 and sums[1] == sums[3] < 0
    # without these the comparison could pass having stepped only the easy branch
    assert all(v >= 1 for v in ref.counts.values()), ref.counts
    assert natural == (24 if max_steps == 500 else 0)
    if max_steps == 12:
        assert max(ep_lengths) == 12 and ep_lengths.count(12) > N
        part = _make(24, env_offset=16, **setting)         # envs 16 .. 39 as a vecenv of their own: the start states of two episodes
        part.async_reset(11)
        for k in range(SET_AT + 1):
            o, r, te, st, cn = trace[k]
            po, pr, pte = part.observations.cpu().numpy(), part.rewards.cpu().numpy(), part.terminals.cpu().numpy()
            pst, pcn = part.debug_states()
            assert np.array_equal(_u32(po), _u32(o[16:])) and np.array_equal(_u32(pr), _u32(r[16:])) and np.array_equal(pte, te[16:]), k
            assert np.array_equal(_u64(pst), _u64(st[16:])) and np.array_equal(pcn, cn[16:]), k
            part.recv()
            part.send(ar.pump_actions(st[16:]))
        assert (pcn[:, 0] == 1).all()


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


def _branch_start(vec):
    """Put envs 0..15 of a freshly reset vecenv on the branch states, so that a 24-step rollout meets wraps, clamps and swing-ups."""
    vec.debug_set_states(*ar.branch_states(*vec.debug_states(), vec.driver_env.max_steps))


def _both_rollouts(hidden, recurrent, n=N, T=T, rollouts=3, **setting):
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
        data = clean_pufferl.create(_config(n, T, n * T // 2, 8, 2, n * T * 10, HP, seed=5), vec, pol)
        assert (data.gen_engine is not None) == (hidden != 128 and not recurrent)
        _expected_form(data, recurrent)
        _branch_start(vec)
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


def _reset_rows(dones):
    """How many auto-reset rows an env-major [n][T] block of Experience.dones holds (row t is one where the flag recv() showed is set)."""
    return int(dones.sum().item())


def _against_the_walker(data, n, T, **setting):
    """The rollout's experience rows against the walker stepped with the actions the policy drew: bit for bit."""
    e = data.experience
    ref = ar.AcrobotSerial(n, **setting)
    ref.async_reset(5)
    ref.set_states(*ar.branch_states(*ref.states(), ref.max_steps))
    acts = e.actions.view(n, T).cpu().numpy()
    for t in range(T):
        o, r, d, _, _, _, _ = ref.recv()
        assert np.array_equal(_u32(o), _u32(e.obs.view(n, T, 16)[:, t, :6].cpu().numpy())), t
        assert np.array_equal(r, e.rewards.view(n, T)[:, t].cpu().numpy()) and np.array_equal(d.astype(np.float32), e.dones.view(n, T)[:, t].cpu().numpy()), t
        ref.send(acts[:, t].astype(np.int64))
    return ref


@pytest.mark.parametrize('hidden', WIDTHS)
def test_fused_mlp_rollout_equals_the_stepwise_protocol_path(hidden):
    """40 envs x 24 steps, three rollouts, max_steps=12, envs 0..15 started on the branch states, once per hidden width —
    rollout_mlp_env_kernel<AcrobotRollEnv, 16, 4, MW, MlpView> with MW = 2 (the flat 128-wide buffer as a view of itself), 1, 4, 8:
    experience rows, live buffers, device state (f64) and the four last-infos buffers torch.equal with _rollout_stepwise; auto-reset
    rows fall inside every rollout, and all three actions were drawn."""
    runs, vecs, datas = _both_rollouts(hidden, False, max_steps=12)
    e = datas[0].experience
    assert e.obs.shape == (N * T, 16) and not e.obs[:, 6:].any() and e.obs[:, 4:6].abs().max() > 1.0
    assert (e.obs[:, :4].abs() <= 1.0).all() and sorted(set(e.actions.cpu().numpy().tolist())) == [0, 1, 2]
    assert _reset_rows(e.dones) >= N
    assert (e.rewards.view(N, T)[:, 1:][e.dones.view(N, T)[:, :-1] != 0] == 0).all()        # the row after a done row shows the reset row's reward
    assert set(e.rewards.cpu().numpy().tolist()) == {0.0, -1.0}


def test_fused_recurrent_rollout_equals_rollout_stepwise():
    """The same equalities plus the carried LSTM state, on the partially observed task (velocities=False), max_steps=12."""
    runs, vecs, datas = _both_rollouts(128, True, max_steps=12, velocities=False)
    e = datas[0].experience
    assert e.obs.shape == (N * T, 16) and not e.obs[:, 4:].any() and e.obs[:, :4].abs().max() > 0.9
    st, _ = vecs[0].debug_states()
    assert st[:, 2:].all()                                               # the velocities are there, only hidden
    assert _reset_rows(e.dones) >= N and sorted(set(e.actions.cpu().numpy().tolist())) == [0, 1, 2]


@pytest.mark.parametrize('hidden', [128, 64])
def test_one_update_against_the_oracle_trainer(hidden):
    """evaluate() + train() at width 128 (ppo_mlp_grad at stride 16) and 64 (pfa_ppo_wide_grad) with 6 inputs and 3 actions: the
    rollout's rows against the walker bit for bit (envs 0..15 started on the branch states: the walker met wraps, clamps, swing-ups
    and time limits), then losses, updated weights (rtol = atol = 1e-5) and Adam's moments against oracle.ppo_torch.Trainer running
    on the walker and fed the same rollout."""
    from pufferlib_amd import clean_pufferl
    from oracle import ppo_torch
    from test_gpu_ppo import _config, _step_major
    n = N
    torch.manual_seed(4)
    vec = _make(n, max_steps=12)
    pol = _policy(vec, hidden, False)
    with torch.no_grad():
        for p_ in pol.parameters():
            p_.add_(0.05 * torch.randn_like(p_))
    data = clean_pufferl.create(_config(n, T, n * T // 2, 8, 2, n * T * 10, HP, seed=5), vec, pol)
    _expected_form(data, False)
    _branch_start(vec)
    w0 = {k[len('policy.'):]: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items()}
    clean_pufferl.evaluate(data)
    e = data.experience
    ref = _against_the_walker(data, n, T, max_steps=12)
    assert all(v >= 1 for v in ref.counts.values()), ref.counts
    B = n * T
    opol = ppo_torch.Policy(w0)
    with torch.no_grad():                                               # the rollout's values and log-probabilities are the oracle's
        logits, oval, _ = opol.forward(e.obs[:, :6].cpu())
        _, olp, _ = ppo_torch.sample_logits(logits, action=e.actions.cpu().long())
    np.testing.assert_allclose(e.values.cpu().numpy(), oval.reshape(-1).numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(e.logprobs.cpu().numpy(), olp.numpy(), rtol=1e-5, atol=1e-5)
    trn = ppo_torch.Trainer(opol, ar.AcrobotSerial(n, max_steps=12), batch_size=B, minibatch_size=B // 2, bptt_horizon=8, update_epochs=2,
                            learning_rate=HP[0], gamma=HP[1], gae_lambda=HP[2], clip_coef=HP[3], vf_coef=HP[4], vf_clip_coef=HP[5],
                            max_grad_norm=HP[6], ent_coef=HP[7], total_timesteps=B * 10, seed=5)
    trn.obs = torch.as_tensor(_step_major(e.obs, n, T)[:, :6].copy())
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


def _train(hidden, recurrent, updates, seed, n=4096, T=128, bptt=8, nmb=8, lr=5e-3, **setting):
    from pufferlib_amd import clean_pufferl, namespace
    torch.manual_seed(seed)
    vec = _make(n, **setting)
    pol = _policy(vec, hidden, recurrent)
    B = n * T
    cfg = namespace(env='acrobot', seed=seed + 1, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * updates,
                    learning_rate=lr, anneal_lr=True, gamma=0.99, gae_lambda=0.95, update_epochs=4, norm_adv=True,
                    clip_coef=0.2, clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.2, max_grad_norm=0.5, ent_coef=0.01,
                    target_kl=None, batch_size=B, minibatch_size=B // nmb, bptt_horizon=bptt, compile=False,
                    checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='acrobot')
    data = clean_pufferl.create(cfg, vec, pol)
    _expected_form(data, recurrent)
    lengths = []
    for _ in range(updates):
        stats, _ = clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        lengths.append(float(dict(stats).get('episode_length', float('nan'))))      # nan: no episode ended in this rollout
    return lengths


# Learning threshold.  Every figure is the mean length of the episodes that ended in one rollout of 4096 envs x 128 steps (the envs
# start together, so the early figures are those of the episodes that happened to end: nan where none did, 500 where only the time
# limit did).  The settings were chosen on the device over three (policy, env) seeds each — CartPole's were found not to carry over
# from the CPU oracle trainer, so that one was not tried.  40 updates were too few for every candidate (best: learning rate 1e-2, 8
# minibatches: 106, 241, 222; learning rate 1e-3 never left 500).  With 100 updates learning rate 5e-3 and 8 minibatches — CartPole's
# setting — fell smoothly on all three seeds: 93.3, 100.6, 89.0 at the last rollout (seeds 0, 1, 2; the last eight rollouts of each
# within 2 of that); learning rate 1e-2 ended at 87.8, 87.9, 88.8 but its seed 2 sat at 500 until rollout 65, and at 70 updates ended at
# 95.4, 163.3, 98.8 (8 minibatches) and 89.5, 89.1, 100.4 (16).  The pinned bound is the worst seed's last figure plus CartPole's margin,
# a tenth of the 500-step scale: 100.6 + 50 = 150.6, well inside the issue's weakest admissible bound of half the random policy's
# 498.1 (tests/test_acrobot_cpu.py).
UPDATES, LEARN_SEEDS = 100, (0, 1, 2)
WORST_LAST, MARGIN = 100.6, 50.0


def test_default_64_learns_to_swing_up():
    """Default(64) on max_steps=500, 4096 envs x 128 steps, 100 updates, learning rate 5e-3, 8 minibatches, seeds 0, 1, 2, all through
    the fused view rollout.  Measured on the MI355X, every fifth rollout: seed 0: nan, 500, 500, 500, 298, 318, 267, 254, 237, 202, 163,
    133, 116, 108, 102, 97, 97, 94, 92, 92 and 93.3 at the last; seed 1: nan, 500, 500, 500, 330, 342, 427, 331, 287, 274, 270, 257, 246,
    242, 225, 167, 131, 113, 106, 101 and 100.6; seed 2: nan, 500, 486, 448, 288, 277, 278, 248, 187, 143, 123, 109, 102, 98, 96, 94, 92,
    90, 89, 89 and 89.0; 0.17 s per run.  A run starts at the random policy's level and ends below the bound; seed 0 twice gives the
    same curve."""
    curves = {seed: _train(64, False, UPDATES, seed) for seed in LEARN_SEEDS}
    again = _train(64, False, UPDATES, LEARN_SEEDS[0])
    for seed, a in curves.items():
        print('acrobot lengths, seed', seed, [round(x, 1) for x in a[::5]], 'last', round(a[-1], 1))
    assert np.array_equal(np.array(again), np.array(curves[LEARN_SEEDS[0]]), equal_nan=True)        # fixed seed: the same curve on two runs
    bound = WORST_LAST + MARGIN
    assert bound < RANDOM_BASELINE / 2
    for seed, a in curves.items():
        assert np.nanmax(a[:10]) > 0.9 * RANDOM_BASELINE, (seed, a[:10])
        assert a[-1] < bound, (seed, a[-5:])


def test_refusals():
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace, spaces, vector, _lib
    from pufferlib_amd.exceptions import APIUsageError, ExtensionError
    from test_gpu_ppo import _config
    import ctypes as C
    cfg = _config(16, 16, 128, 16, 1, 16 * 16 * 4, HP)
    # a policy with other than three actions: every fused entry point names the head it needs
    for hidden, recurrent, text in ((128, False, 'rollout_mlp_acrobot: the policy must have one Discrete\\(3\\) head'),
                                    (64, False, 'rollout_mlp_view_acrobot: the policy must have one Discrete\\(3\\) head'),
                                    (128, True, 'rollout_lstm_acrobot: the policy must have one Discrete\\(3\\) head')):
        vec = _make(16)
        two = namespace(single_observation_space=vec.single_observation_space, single_action_space=spaces.Discrete(2))
        data = clean_pufferl.create(cfg, vec, _policy(two, hidden, recurrent))
        with pytest.raises(ExtensionError, match=text):
            clean_pufferl.evaluate(data)
    # a policy over another row shape: the same entry points, handed dims / a view that claim 4 observation values, or rows of 32 floats
    for hidden in (128, 64):
        vec = _make(16)
        data = clean_pufferl.create(cfg, vec, _policy(vec, hidden, False))
        args = (C.byref(data.experience.c), None, C.byref(_lib.NoiseKey(0, 0)), 0, *vec._live(), _lib.stream_handle())
        for field, value, got in (('obs_dim', 4, '4 in rows of 16'), ('obs_stride', 32, '6 in rows of 32')):
            if hidden == 128:
                d = _lib.MlpDims.from_buffer_copy(data.flat_params.dims)
                setattr(d, field, value)
                rc = vec.L.pfa_rollout_mlp_acrobot(_lib.ptr(vec.state), C.byref(vec.cfg), _lib.ptr(data.flat_params.flat), C.byref(d), *args)
                name = 'rollout_mlp_acrobot'
            else:
                d = _lib.MlpView.from_buffer_copy(data.gen_engine.mlp_view)
                setattr(d, field, value)
                rc = vec.L.pfa_rollout_mlp_view_acrobot(_lib.ptr(vec.state), C.byref(vec.cfg), C.byref(d), *args)
                name = 'rollout_mlp_view_acrobot'
            want = f'{name}: the policy must take 6 observation values in rows of 16 floats (got {got})'
            assert rc != 0 and want in vec.L.pfa_last_error().decode(), (vec.L.pfa_last_error(), want)
    # null buffers: every protocol entry point refuses before it launches
    vec = _make(4)
    L, st, cf, s = vec.L, _lib.ptr(vec.state), C.byref(vec.cfg), _lib.stream_handle()
    for call, text in ((lambda: L.pfa_acrobot_async_reset(st, cf, None, None, None, None, None, s), 'acrobot.async_reset: null buffer'),
                       (lambda: L.pfa_acrobot_send(st, cf, None, *vec._live(), s), 'acrobot.send: null buffer'),
                       (lambda: L.pfa_acrobot_debug_states(st, cf, None, None, s), 'acrobot.debug_states: null buffer'),
                       (lambda: L.pfa_acrobot_debug_set_states(st, cf, None, None, None, None, s), 'acrobot.debug_set_states: null buffer'),
                       (lambda: L.pfa_acrobot_debug_set_states(None, cf, None, None, None, None, s), 'acrobot.debug_set_states: null buffer'),
                       (lambda: L.pfa_acrobot_episode_stats(st, cf, None, 0, s), 'acrobot.episode_stats: bad arguments'),
                       (lambda: L.pfa_acrobot_last_infos(st, cf, None, None, None, None, s), 'acrobot.last_infos: bad arguments')):
        assert call() != 0 and text in L.pfa_last_error().decode(), text
    # a MultiDiscrete policy: the device envs take one Discrete head
    md_env = namespace(single_observation_space=vec.single_observation_space, single_action_space=spaces.MultiDiscrete([3, 3]))
    with pytest.raises(NotImplementedError, match='MultiDiscrete'):
        clean_pufferl.create(cfg, _make(16), cleanrl.Policy(models.Default(md_env)))
    # the start states are keyed by (seed, global env): seeds must be consecutive
    with pytest.raises(APIUsageError, match='Acrobot needs consecutive seeds'):
        vec.async_reset([3, 4, 6, 7])
    vec.async_reset([3, 4, 5, 6])
    # a negative time limit, and an action outside the head on the first send
    with pytest.raises(APIUsageError, match='max_steps must be >= 0'):
        _make(4, max_steps=-1)
    vec.recv()
    with pytest.raises(APIUsageError, match='Actions do not match'):
        vec.send(np.array([0, 1, 3, 0]))
    # debug_set_states: wrong shapes, a state outside the box, a negative counter — nothing is uploaded
    good_s, good_c = vec.debug_states()
    for s_, c_ in ((good_s[:3], good_c), (good_s, good_c[:, :3]), (good_s.reshape(-1), good_c), (np.zeros((4, 5)), good_c)):
        with pytest.raises(APIUsageError, match='must have shape \\(4, 4\\)'):
            vec.debug_set_states(s_, c_)
    bad = good_s.copy()
    bad[2, 0] = 3.5
    with pytest.raises(APIUsageError, match='outside the state box'):
        vec.debug_set_states(bad, good_c)
    bad = good_s.copy()
    bad[1, 3] = np.nan
    with pytest.raises(APIUsageError, match='outside the state box'):
        vec.debug_set_states(bad, good_c)
    with pytest.raises(APIUsageError, match='negative counter'):
        vec.debug_set_states(good_s, good_c - 1)
    assert np.array_equal(vec.debug_states()[0], good_s) and np.array_equal(vec.debug_states()[1], good_c)


def test_fused_rollout_is_faster_than_its_own_stepwise_path():
    """4096 envs x 128 steps, Default(128) and Default(64), HIP-event times, median of 5 after a warm-up: one persistent kernel against
    three launches per step."""
    from pufferlib_amd import clean_pufferl
    from test_gpu_ppo import _config
    n, T = 4096, 128
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
        print(f'acrobot rollout 4096 x 128, hidden {hidden}: fused {fused:.3f} ms, stepwise {stepwise:.3f} ms, factor {stepwise / fused:.1f}')
        assert fused < stepwise, (hidden, fused, stepwise)
