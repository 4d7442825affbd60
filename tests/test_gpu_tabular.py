"""vector.Tabular (csrc/tabular_env.hpp, csrc/tabular.hip): a user-given finite MDP / POMDP on the device.  Against the golden
trajectory of the unmodified reference (ocean Stochastic written as a table), against vector.Stochastic send for send, against the
numpy walker of tests/tabular_reference.py on every code path of the protocol kernels, fused rollouts == stepwise pieces bit for
bit for both policies and every row stride, one update against the torch-fp32 oracle trainer, learning through create / evaluate /
train, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from adam_moments import assert_moments_match

sys.path.insert(0, os.path.dirname(__file__))
import tabular_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

HP = [1e-3, 0.97, 0.9, 0.2, 0.5, 0.2, 0.5, 0.02]


def _make(mdp, n, **kw):
    from pufferlib_amd import vector
    return vector.make(vector.make_tabular, env_kwargs=dict(mdp=mdp), num_envs=n, backend=vector.Tabular, **kw)


def _random_mdp(S, A, K, D, M=1, horizon=6, seed=0, terminal_frac=0.2, score=True):
    from pufferlib_amd.vector import TabularMDP
    rng = np.random.default_rng(seed)
    terminal = rng.random(S) < terminal_frac
    terminal[:M] = False
    prob = rng.dirichlet(np.ones(K), size=(S, A)) if K > 1 else None
    starts = (np.arange(M), rng.dirichlet(np.ones(M))) if M > 1 else 0
    return TabularMDP(rng.integers(0, S, (S, A, K)), prob, reward=rng.normal(size=(S, A, K)), terminal=terminal,
                      obs=rng.normal(size=(S, D)).astype(np.float32), start=starts, horizon=horizon,
                      score=rng.normal(size=S) if score else None)


@pytest.fixture(scope='module')
def stochastic_table():
    return tr.stochastic_as_table(0.7)


def _bits(x):
    return x.cpu().numpy().view(np.uint32)


def test_reference_golden_through_the_device(golden_dir, stochastic_table):
    """tests/golden/stochastic.npz (unmodified reference) replayed by vector.Tabular over Stochastic-as-a-table, bit for bit."""
    g = np.load(os.path.join(golden_dir, 'stochastic.npz'))
    n, seed, steps = (int(x) for x in g['config'])
    assert float(g['p'][0]) == 0.7
    vec = _make(stochastic_table, n)
    assert vec.obs_stride == 16 and vec.observations.shape == (n, 1)
    vec.async_reset(seed)
    infos = []
    for k in range(steps + 1):
        o, r, te, trunc, info, ids, m = vec.recv()
        assert np.array_equal(o.cpu().numpy(), g['obs'][k]) and np.array_equal(_bits(r), g['rewards'][k].view(np.uint32)), k
        assert np.array_equal(te.cpu().numpy(), g['terminals'][k]) and not trunc.any() and m.all(), k
        infos += [(k, j, i['episode_return'], i['episode_length'], i['score']) for j, i in enumerate(info)]
        if k < steps:
            vec.send(g['actions'][k].astype(np.int64))
    assert np.array_equal(np.array(infos, np.float64).reshape(-1, 5), g['infos'])
    st = vec.episode_stats().cpu().numpy()
    assert st[0] == 12 and abs(st[1] - g['infos'][:, 2].sum()) < 1e-9 and st[2] == 1200 and abs(st[3] - g['infos'][:, 4].sum()) < 1e-9


@pytest.mark.parametrize('first', [0, 1])
def test_equals_vector_stochastic_send_for_send(stochastic_table, first):
    """The schedule of test_gpu_stochastic.test_every_reachable_reward_state_matches_the_oracle at p = 0.7, 101 envs: together the
    envs visit every (tick, count, last action) of a 100-step episode."""
    from pufferlib_amd import vector
    n = 101
    tab = _make(stochastic_table, n)
    sto = vector.make(vector.make_stochastic, env_kwargs=dict(p=0.7), num_envs=n, backend=vector.Stochastic)
    tab.async_reset(0)
    sto.async_reset(0)
    tab.recv(), sto.recv()
    finished = 0
    for t in range(101):
        a = np.where(np.arange(n) > t, first, 1 - first).astype(np.int64)
        tab.send(a)
        sto.send(a)
        o, r, te, _, info, _, _ = tab.recv()
        o2, r2, te2, _, info2, _, _ = sto.recv()
        assert torch.equal(o, o2) and np.array_equal(_bits(r), _bits(r2)) and torch.equal(te, te2), t
        assert info == info2 and len(info) == (n if t == 99 else 0), t         # send 100 ends every episode, send 101 is the reset row
        finished += len(info)
    assert finished == n and torch.equal(tab.episode_stats(), sto.episode_stats())


def _zero_one_table():
    """Outcomes of probability zero (first, middle, last) and one; two states that look alike."""
    from pufferlib_amd.vector import TabularMDP
    nxt = [[[1, 2, 0], [2, 1, 0]], [[0, 2, 1], [2, 2, 0]], [[0, 1, 2], [1, 0, 3]], [[3, 3, 3], [3, 3, 3]]]
    prob = [[[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], [[0.5, 0.0, 0.5], [0.0, 0.0, 1.0]], [[0.25, 0.75, 0.0], [0.0, 0.5, 0.5]],
            [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]]
    return TabularMDP(nxt, prob, reward=np.arange(24, dtype=np.float64).reshape(4, 2, 3) / 7, terminal=[0, 0, 0, 1],
                      obs=[[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]], start=([2, 0, 1], [0.0, 1.0, 0.0]), horizon=9)


def _protocol_cases():
    from pufferlib_amd.vector import TabularMDP
    return {
        'k1_d1': lambda: _random_mdp(7, 3, 1, 1, seed=1),
        'slippery_gridworld': lambda: TabularMDP.gridworld(3, 3, slip=0.3, horizon=7),
        'zero_and_one': _zero_one_table,
        'd17': lambda: _random_mdp(9, 2, 2, 17, seed=2),
        'd49': lambda: _random_mdp(9, 5, 3, 49, seed=3),
        'd100': lambda: _random_mdp(6, 2, 8, 100, seed=4),
        'd128': lambda: _random_mdp(5, 4, 2, 128, seed=5),
        'many_starts': lambda: _random_mdp(40, 3, 2, 5, M=33, seed=6),
        'horizon_cuts': lambda: _random_mdp(11, 2, 4, 3, M=2, horizon=3, seed=7, terminal_frac=0.0, score=False),
    }


def _walk_both(vec, ref, seed, sends, rng, actions_of=None):
    mdp = ref.mdp
    vec.async_reset(seed)
    ref.async_reset(seed)
    D = mdp.obs_dim
    for k in range(sends + 1):
        o, r, te, trunc, info, ids, m = vec.recv()
        o2, r2, te2, trunc2, info2, ids2, m2 = ref.recv()
        assert o.shape == (ref.n, D) and np.array_equal(o.cpu().numpy(), o2), k
        assert not vec.obs_buf[:, D:].any(), k                                     # the row's padding stays zero
        assert np.array_equal(_bits(r), r2.view(np.uint32)) and np.array_equal(te.cpu().numpy(), te2), k
        assert not trunc.any() and m.all() and np.array_equal(ids, ids2), k
        assert info == info2, (k, info, info2)
        assert np.array_equal(vec.debug_states(), ref.states()), k
        a = rng.integers(0, mdp.num_actions, ref.n) if actions_of is None else actions_of(k)
        vec.send(a)
        ref.send(a)
    st = vec.episode_stats(reset=False).cpu().numpy()
    assert st[0] == ref.sums[0] and st[2] == ref.sums[2] and np.allclose(st[[1, 3]], ref.sums[[1, 3]], rtol=0, atol=1e-9 * max(1.0, ref.sums[0]))
    return st


@pytest.mark.parametrize('case', ['k1_d1', 'slippery_gridworld', 'zero_and_one', 'd17', 'd49', 'd100', 'd128', 'many_starts', 'horizon_cuts'])
def test_protocol_path_equals_the_walker(case):
    """Observations, f32 reward bits, terminals, infos of every send and the device state, array_equal with the numpy walker; 1, 17 and
    257 envs (tail threads of the 256-thread send workgroup, a second workgroup), 40 sends each."""
    mdp = _protocol_cases()[case]()
    finished = 0
    for n in (1, 17, 257):
        vec = _make(mdp, n)
        assert vec.obs_stride == next(s for s in (16, 32, 64, 96, 128) if mdp.obs_dim <= s)
        finished += _walk_both(vec, tr.TabularSerial(mdp, n), 3 + n, 40, np.random.default_rng(n))[0]
    assert finished > 275            # episodes did end (and start again) in every case


def test_env_offset_reproduces_the_envs_of_a_larger_vecenv():
    """Data-parallel seeding: a vecenv built with env_offset = 5 is envs 5 .. of a larger one."""
    from pufferlib_amd.vector import TabularMDP
    mdp = TabularMDP.gridworld(3, 3, slip=0.3, horizon=7)
    big, part = _make(mdp, 17), _make(mdp, 12, env_offset=5)
    ref = tr.TabularSerial(mdp, 12, env_offset=5)
    rng = np.random.default_rng(0)
    acts = rng.integers(0, 4, (41, 17))
    big.async_reset(9)
    big.recv()

    def actions_of(k):     # called after recv k of the offset vecenv was compared with the walker: the larger one shows the same rows 5 ..
        assert torch.equal(part.observations, big.observations[5:]) and torch.equal(part.rewards, big.rewards[5:]), k
        assert torch.equal(part.terminals, big.terminals[5:]) and np.array_equal(part.debug_states(), big.debug_states()[5:]), k
        big.send(acts[k])
        big.recv()
        return acts[k, 5:]
    _walk_both(part, ref, 9, 40, rng, actions_of)


def _snapshot(data, vec, recurrent=False):
    e = data.experience
    out = [x.clone() for x in (e.obs, e.actions, e.logprobs, e.values, e.rewards, e.dones, vec.obs_buf, vec.rewards, vec.terminals_u8,
                                vec.state)]
    if recurrent:
        out += [data.lstm_engine.lstm_h.clone(), data.lstm_engine.lstm_c.clone()]
    return out + [torch.as_tensor(vec.debug_states())]


def _both_rollouts(mdp, n, T, recurrent, obs_stride, rollouts=1):
    """evaluate() (one persistent kernel) and the stepwise pieces on twin vecenvs and policies -> (snapshots per path, vecs, datas)."""
    from pufferlib_amd import clean_pufferl, cleanrl, models
    from test_gpu_ppo import _config
    runs, vecs, datas = [], [], []
    for fused in (True, False):
        torch.manual_seed(4)
        vec = _make(mdp, n, obs_stride=obs_stride)
        base = models.Default(vec.driver_env)
        pol = cleanrl.RecurrentPolicy(models.LSTMWrapper(vec.driver_env, base)) if recurrent else cleanrl.Policy(base)
        with torch.no_grad():
            for p_ in pol.parameters():
                p_.add_(0.05 * torch.randn_like(p_))
        data = clean_pufferl.create(_config(n, T, n * T // 2, 16, 2, n * T * 10, HP, seed=5), vec, pol)
        assert clean_pufferl.rollout_form(type(vec), False, recurrent, False) == (clean_pufferl.FUSED_LSTM if recurrent else clean_pufferl.FUSED_MLP)
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


@pytest.mark.parametrize('stride', [16, 32, 64, 96, 128])
def test_fused_mlp_rollout_equals_the_stepwise_protocol_path(stride):
    """40 envs (two and a half 16-env tiles) x 32 steps on the slippery 3 x 3 gridworld with horizon 7 — several episode ends and reset
    rows per env — once per row-stride instantiation of rollout_mlp_env_kernel<TabularRollEnv, DP, KS>: experience rows, live buffers, device state and
    the four last-infos buffers torch.equal; at stride 16 then one train() against the torch-fp32 oracle trainer fed the same rollout."""
    from pufferlib_amd import clean_pufferl
    from pufferlib_amd.vector import TabularMDP
    from oracle import ppo_torch
    from test_gpu_ppo import _step_major
    n, T = 40, 32
    mdp = TabularMDP.gridworld(3, 3, slip=0.3, horizon=7)
    runs, vecs, datas = _both_rollouts(mdp, n, T, False, stride, rollouts=2)
    data, vec = datas[0], vecs[0]
    e = data.experience
    assert e.obs.shape == (n * T, stride) and not e.obs[:, 9:].any() and (e.obs[:, :9].sum(1) == 1).all()
    assert int(e.actions.min()) >= 0 and int(e.actions.max()) <= 3 and e.dones.sum() > n
    if stride != 16:
        return
    # the rollout against the walker on the same actions, then the update against the oracle trainer
    torch.manual_seed(4)
    vec3 = _make(mdp, n, obs_stride=stride)
    from pufferlib_amd import cleanrl, models
    from test_gpu_ppo import _config
    pol = cleanrl.Policy(models.Default(vec3.driver_env))
    with torch.no_grad():
        for p_ in pol.parameters():
            p_.add_(0.05 * torch.randn_like(p_))
    data = clean_pufferl.create(_config(n, T, n * T // 2, 16, 2, n * T * 10, HP, seed=5), vec3, pol)
    w0 = {k[len('policy.'):]: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items()}
    clean_pufferl.evaluate(data)
    e = data.experience
    for a, b in zip(_snapshot(data, vec3)[:6], runs[0][0][:6]):
        assert torch.equal(a, b)
    ref = tr.TabularSerial(mdp, n)
    ref.async_reset(5)
    acts = e.actions.view(n, T).cpu().numpy()
    for t in range(T):
        o, r, d, _, _, _, _ = ref.recv()
        assert np.array_equal(o, e.obs.view(n, T, stride)[:, t, :9].cpu().numpy()), t
        assert np.array_equal(r, e.rewards.view(n, T)[:, t].cpu().numpy()) and np.array_equal(d.astype(np.float32), e.dones.view(n, T)[:, t].cpu().numpy()), t
        ref.send(acts[:, t].astype(np.int64))
    B = n * T
    opol = ppo_torch.Policy(w0)
    trn = ppo_torch.Trainer(opol, tr.TabularSerial(mdp, n), batch_size=B, minibatch_size=B // 2, bptt_horizon=16, update_epochs=2,
                            learning_rate=HP[0], gamma=HP[1], gae_lambda=HP[2], clip_coef=HP[3], vf_coef=HP[4], vf_clip_coef=HP[5],
                            max_grad_norm=HP[6], ent_coef=HP[7], total_timesteps=B * 10, seed=5)
    trn.obs = torch.as_tensor(_step_major(e.obs, n, T)[:, :9].copy())
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


def test_fused_mlp_rollout_at_the_trimmed_64_float_row():
    """49 .. 52 observation values in rows of 64 floats: the standalone forward issues 13 of the 16 k-steps, and so must the fused rollout."""
    _both_rollouts(_random_mdp(9, 5, 3, 49, M=3, horizon=5, seed=3), 40, 32, False, None)


@pytest.mark.parametrize('stride', [16, 160])
def test_fused_recurrent_rollout_equals_rollout_stepwise(stride):
    """The same equalities plus the carried LSTM state, T-maze of length 3 (episodes of 4 steps + the reset row), at the narrowest row and
    at the 160-float row of the recurrent kernels."""
    from pufferlib_amd.vector import TabularMDP
    runs, vecs, datas = _both_rollouts(TabularMDP.tmaze(3), 40, 32, True, stride, rollouts=2)
    e = datas[0].experience
    assert e.obs.shape == (40 * 32, stride) and not e.obs[:, 3:].any()
    assert runs[0][1][-1]['episode_length'] == 4 and 0 <= runs[0][1][-1]['score'] <= 1


def test_stepwise_on_the_gemm_path_with_twenty_actions():
    """Default(hidden_size=64) on a 20-action table: outside the fused kernels, so evaluate() steps the vecenv through general.Engine."""
    from pufferlib_amd import clean_pufferl, cleanrl, models
    from test_gpu_ppo import _config
    n, T = 48, 16
    mdp = _random_mdp(12, 20, 2, 6, M=2, horizon=5, seed=8)
    vec = _make(mdp, n)
    torch.manual_seed(1)
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=64))
    data = clean_pufferl.create(_config(n, T, n * T // 2, 16, 2, n * T * 10, HP, seed=5), vec, pol)
    assert data.gen_engine is not None
    assert clean_pufferl.rollout_form(type(vec), True, False, data.gen_engine.mlp_view is not None) == clean_pufferl.STEPWISE
    stats, _ = clean_pufferl.evaluate(data)
    e = data.experience
    assert int(e.actions.min()) >= 0 and int(e.actions.max()) < 20 and len(torch.unique(e.actions)) > 10
    assert stats['episode_length'] > 0 and torch.isfinite(e.values).all()
    # the env side against the walker on the actions the policy drew
    ref = tr.TabularSerial(mdp, n)
    ref.async_reset(5)
    acts = e.actions.view(n, T).cpu().numpy()
    for t in range(T):
        o, r, d, _, _, _, _ = ref.recv()
        assert np.array_equal(r, e.rewards.view(n, T)[:, t].cpu().numpy()) and np.array_equal(d.astype(np.float32), e.dones.view(n, T)[:, t].cpu().numpy()), t
        ref.send(acts[:, t].astype(np.int64))
    before = [p_.detach().clone() for p_ in pol.parameters()]
    clean_pufferl.train(data)
    assert all(torch.isfinite(p_).all() for p_ in pol.parameters()) and any(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    assert np.isfinite(data.losses.policy_loss) and np.isfinite(data.losses.value_loss)


def _train(mdp, recurrent, updates, obs_stride=None, n=256, T=32):
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace
    torch.manual_seed(0)
    vec = _make(mdp, n, obs_stride=obs_stride)
    base = models.Default(vec.driver_env)
    pol = cleanrl.RecurrentPolicy(models.LSTMWrapper(vec.driver_env, base)) if recurrent else cleanrl.Policy(base)
    B = n * T
    cfg = namespace(env='tabular', seed=1, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * updates,
                    learning_rate=5e-3, anneal_lr=True, gamma=0.95, gae_lambda=0.9, update_epochs=4, norm_adv=True,
                    clip_coef=0.1, clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.1, max_grad_norm=0.5, ent_coef=0.01,
                    target_kl=None, batch_size=B, minibatch_size=B // 4, bptt_horizon=8, compile=False,
                    checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='tab')
    data = clean_pufferl.create(cfg, vec, pol)
    scores = []
    for _ in range(updates):
        stats, _ = clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        scores.append(stats['score'])
    return scores


# Learning thresholds.  The hyper-parameters of _train were first confirmed on the CPU — oracle.ppo_torch.Trainer on the numpy walker, 30
# updates of 256 envs x 32 steps: gridworld score 0.278 -> 1.0 (0.997 at rollout 11), T-maze under the LSTM 0.497 -> 1.0 (0.988 at rollout
# 9), T-maze under the MLP 0.47 .. 0.54 throughout — and the thresholds then set from the first GPU run (figures in the tests'
# docstrings) with the 0.1 margin of tests/test_gpu_memory.py's solved / not-solved pair (solved: measured 1.0 -> above 0.9; chance:
# measured 0.5 -> below 0.6; untrained start: measured + 0.1).
GRID_UPDATES = TMAZE_UPDATES = 30
GRID_START_BELOW, GRID_MARGIN = 0.4, 0.1
TMAZE_SOLVED, TMAZE_CHANCE_BELOW = 0.9, 0.6


def test_default_learns_the_slippery_gridworld():
    """Default on gridworld(5, 5, slip=0.1, horizon=20), 256 envs x 32 steps, 30 updates, seed 1: the mean score (= the fraction of
    episodes that reach the goal) approaches the value-iteration optimum 0.9999989.  Measured on the MI355X: 0.302 after the first
    rollout, 0.975 at rollout 9, 0.999 at rollout 11, 1.0 from rollout 13 on; the same curve on both runs; 0.33 s per run."""
    from pufferlib_amd.vector import TabularMDP
    mdp = TabularMDP.gridworld(5, 5, slip=0.1, horizon=20)
    opt = tr.optimal_score(mdp)
    a, b = _train(mdp, False, GRID_UPDATES), _train(mdp, False, GRID_UPDATES)
    print('gridworld scores', [round(x, 3) for x in a[::3]], 'last', a[-1], 'optimum', opt)
    assert a == b                                        # fixed seed: the same curve on two runs
    assert a[0] < GRID_START_BELOW and a[-1] > opt - GRID_MARGIN, (a[0], a[-5:], opt)


@pytest.mark.parametrize('stride', [16, 160])
def test_the_recurrent_policy_solves_the_tmaze(stride):
    """LSTMWrapper(Default) on tmaze(3), 256 envs x 32 steps, 30 updates, seed 1, at the narrowest row and at obs_stride=160 (the row
    width of the recurrent kernels' c3 shape, on a task with dynamics).  Measured on the MI355X, the same at both strides (the padding
    columns are zero): 0.516 after the first rollout, 0.742 at rollout 7, 0.981 at rollout 9, 0.999 .. 1.0 from rollout 11 on; the
    same curve on both runs; 0.2 s per run."""
    from pufferlib_amd.vector import TabularMDP
    mdp = TabularMDP.tmaze(3)
    a, b = _train(mdp, True, TMAZE_UPDATES, obs_stride=stride), _train(mdp, True, TMAZE_UPDATES, obs_stride=stride)
    print('tmaze lstm scores, stride', stride, [round(x, 3) for x in a[::3]], 'last', a[-1])
    assert a == b
    assert a[0] < 0.6 and a[-1] > TMAZE_SOLVED, (a[0], a[-5:])


def test_the_memoryless_policy_stays_at_chance_on_the_tmaze():
    """Default without memory on tmaze(3): the corridor and the junction look the same under either cue, so the table really is a
    POMDP and the score stays at chance.  Measured on the MI355X over 30 updates: between 0.474 and 0.516 throughout."""
    from pufferlib_amd.vector import TabularMDP
    a = _train(TabularMDP.tmaze(3), False, TMAZE_UPDATES)
    print('tmaze mlp scores', [round(x, 3) for x in a[::3]], 'last', a[-1])
    assert all(x < TMAZE_CHANCE_BELOW for x in a[-5:]), a[-5:]


def test_refusals():
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace, spaces, vector
    from pufferlib_amd.exceptions import APIUsageError
    from pufferlib_amd.vector import TabularMDP
    from test_gpu_ppo import _config
    cfg = _config(16, 16, 128, 16, 1, 16 * 16 * 4, HP)
    t = TabularMDP.tmaze(3)
    # a conv policy reads uint8 frames
    frames = vector.make_frames()
    with pytest.raises(NotImplementedError, match='uint8 frames'):
        clean_pufferl.create(cfg, _make(t, 16), cleanrl.Policy(models.Convolutional(frames, framestack=4)))
    # a MultiDiscrete policy: the device envs take one Discrete head
    vec = _make(t, 16)
    md_env = namespace(single_observation_space=vec.single_observation_space, single_action_space=spaces.MultiDiscrete([2, 2]))
    with pytest.raises(NotImplementedError, match='MultiDiscrete'):
        clean_pufferl.create(cfg, vec, cleanrl.Policy(models.Default(md_env)))
    # rows wider than the feed-forward kernels' 128 floats need the explicit recurrent stride
    wide = _random_mdp(4, 2, 1, 130, seed=9)
    with pytest.raises(APIUsageError, match='obs_stride=160'):
        _make(wide, 4)
    assert _make(wide, 4, obs_stride=160).obs_stride == 160
    with pytest.raises(APIUsageError, match='obs_stride 48'):
        _make(t, 4, obs_stride=48)
    with pytest.raises(APIUsageError, match='obs_stride 16'):
        _make(_random_mdp(4, 2, 1, 17, seed=9), 4, obs_stride=16)
    # actions outside the head are refused by the first send, as on every device env
    vec = _make(t, 4)
    vec.async_reset(0)
    vec.recv()
    with pytest.raises(APIUsageError, match='Actions do not match'):
        vec.send(np.array([0, 1, 2, 0]))


def test_fused_rollout_is_faster_than_its_own_stepwise_path(stochastic_table):
    """4096 envs x 128 steps of Stochastic-as-a-table, HIP-event times, median of 5 after a warm-up: one persistent kernel against three
    launches per step.  (tools/tabular_bench.py reports the figures, with pfa_rollout_mlp_stochastic on the same policy beside them.)"""
    from pufferlib_amd import clean_pufferl, cleanrl, models
    from test_gpu_ppo import _config
    n, T = 4096, 128
    vec = _make(stochastic_table, n)
    pol = cleanrl.Policy(models.Default(vec.driver_env))
    data = clean_pufferl.create(_config(n, T, n * T // 4, 16, 1, n * T * 100, HP, seed=5), vec, pol)
    key = lambda: clean_pufferl._lib.NoiseKey(pol.noise_seed, pol.noise_step)  # noqa: E731

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
    fused = timed(lambda: vec.fused_rollout_mlp(data.flat_params, data.experience, None, key(), clean_pufferl._lib.stream_handle()))
    stepwise = timed(lambda: clean_pufferl._rollout_stepwise(data, None, T, n))
    print(f'tabular rollout 4096 x 128: fused {fused:.3f} ms, stepwise {stepwise:.3f} ms, factor {stepwise / fused:.1f}')
    assert fused < stepwise, (fused, stepwise)
