"""vector.PixelSquared on the GPU (csrc/pixel_squared.hip): it steps in lock step with vector.Squared bit for bit, its frames are the
numpy renderer's (tests/pixel_squared_reference.py) of Squared's grid at every send, the trainer's stepwise rollout stores what the env
showed, and — what the env is for — PPO through create / evaluate / train learns its one-move task with both conv engines."""
import time

import numpy as np
import pytest
import torch

from pixel_squared_reference import render

pytestmark = pytest.mark.gpu

# (height, width, channels, channels_last): channel-last with 3 and 1 channels, channel-first, and uneven cells with 4 channels
SHAPES = [(40, 40, 3, True), (60, 80, 1, True), (84, 84, 4, False), (30, 44, 4, True)]


def _pixel(n, d, nt, shape, **kw):
    from pufferlib_amd import vector
    h, w, c, last = shape
    return vector.make(vector.make_pixel_squared, num_envs=n, backend=vector.PixelSquared,
                       env_kwargs=dict(distance_to_target=d, num_targets=nt, height=h, width=w, channels=c, channels_last=last), **kw)


def _squared(n, d, nt, **kw):
    from pufferlib_amd import vector
    return vector.make(vector.make_squared, num_envs=n, backend=vector.Squared, env_kwargs=dict(distance_to_target=d, num_targets=nt), **kw)


def _same_live(px, sq, shape, where):
    for name in ('rewards', 'terminals', 'truncations', 'masks'):
        assert np.array_equal(getattr(px, name).cpu().numpy(), getattr(sq, name).cpu().numpy()), (name, where)
    grid = sq.observations.cpu().numpy()
    g = grid.shape[-1]
    assert np.array_equal(px.grid[:, :g * g].cpu().numpy().reshape(grid.shape), grid), ('grid', where)
    assert np.array_equal(px.observations.cpu().numpy(), render(grid, *shape)), ('frame', where)


@pytest.mark.parametrize('env_offset', [0, 1000])
@pytest.mark.parametrize('d,nt', [(3, 1), (2, 4)])
@pytest.mark.parametrize('n', [64, 257])
def test_lock_step_with_squared(n, d, nt, env_offset):
    """Same settings, seed and env offset, the same actions: live scalars, infos, statistics and targets equal vector.Squared's at
    every send, across three auto-resets, and the frame is the renderer's of Squared's grid — at every frame shape, 257 envs being
    a count no workgroup size divides."""
    sq = _squared(n, d, nt, env_offset=env_offset)
    pxs = [_pixel(n, d, nt, shape, env_offset=env_offset) for shape in SHAPES]
    for v in [sq] + pxs:
        v.async_reset(42 + env_offset)
    rng = np.random.default_rng(7)
    for px, shape in zip(pxs, SHAPES):
        assert px.episode_len == sq.episode_len
        _same_live(px, sq, shape, 'reset')
    for t in range(3 * sq.episode_len + 1):
        a = rng.integers(0, 8, n)
        sq.recv()
        sq.send(a)
        for px, shape in zip(pxs, SHAPES):
            px.recv()
            px.send(a)
            _same_live(px, sq, shape, t)
            assert px.infos == sq.infos, t
    want_stats, want_targets = sq.episode_stats().cpu().numpy(), sq.debug_targets()
    assert want_stats[0] == 3 * n
    for px in pxs:
        assert np.array_equal(px.episode_stats().cpu().numpy(), want_stats)
        assert np.array_equal(px.debug_targets(), want_targets)
        assert float(px.stats_with_flag(reset=False)[4]) == 0.0       # no tape underrun


@pytest.mark.parametrize('n', [2049, 4099, 8195])
def test_lock_step_where_a_workgroup_owns_several_envs(n):
    """From 2048 envs on a workgroup of the send kernel owns 2, then 4, then 8 envs (csrc/pixel_squared.hip, pixel_envs_per_wg); the
    counts leave the last workgroup 1, 3 and 3 of them.  Two small frame shapes, one with fewer 16-byte chunks than the workgroup has
    lanes, across one auto-reset."""
    shapes = [(40, 40, 3, True), (24, 24, 2, False)]
    sq = _squared(n, 2, 4)
    pxs = [_pixel(n, 2, 4, shape) for shape in shapes]
    for v in [sq] + pxs:
        v.async_reset(42)
    g = torch.Generator(device='cuda').manual_seed(9)
    for t in range(sq.episode_len + 2):
        a = torch.randint(0, 8, (n,), device='cuda', generator=g)
        sq.recv()
        sq.send(a)
        for px, shape in zip(pxs, shapes):
            px.recv()
            px.send(a)
            _same_live(px, sq, shape, t)
            assert px.infos == sq.infos, t
    want = sq.episode_stats().cpu().numpy()
    assert want[0] == n
    for px in pxs:
        assert np.array_equal(px.episode_stats().cpu().numpy(), want) and np.array_equal(px.debug_targets(), sq.debug_targets())


def test_protocol():
    from pufferlib_amd import vector
    from pufferlib_amd.exceptions import APIUsageError
    n, shape = 8, (30, 44, 4, True)
    px = _pixel(n, 3, 1, shape)
    assert px.single_observation_space.shape == (30, 44, 4) and px.single_observation_space.dtype == np.uint8
    assert px.single_action_space.n == 8 and px.obs_stride == 30 * 44 * 4 and px.num_envs == n
    with pytest.raises(APIUsageError, match='reset before stepping'):
        px.recv()
    with pytest.raises(APIUsageError):
        px.send(np.zeros(n, np.int64))
    px.async_reset(3)
    ptrs = set()
    for t in range(6):
        o, r, te, tr, infos, ids, mask = px.recv()
        assert o.dtype == torch.uint8 and tuple(o.shape) == (n, 30, 44, 4) and o.data_ptr() == px.obs_buf.data_ptr()
        ptrs.add(o.data_ptr())
        px.send(np.full(n, t % 8))
    assert len(ptrs) == 1
    # creators that do not agree, and creators of another family
    kw = dict(height=40, width=40, channels=3)
    with pytest.raises(APIUsageError, match='share one PixelSquared configuration'):
        vector.make([vector.make_pixel_squared] * 2, env_args=[[], []], env_kwargs=[dict(kw), dict(kw, channels=1)], num_envs=2, backend=vector.PixelSquared)
    with pytest.raises(APIUsageError, match='share one PixelSquared configuration'):
        vector.make([vector.make_pixel_squared] * 2, env_args=[[], []], env_kwargs=[dict(kw), dict(kw, distance_to_target=2)], num_envs=2,
                    backend=vector.PixelSquared)
    with pytest.raises(APIUsageError, match='pixel_squared'):
        vector.make(vector.make_squared, num_envs=2, backend=vector.PixelSquared)
    with pytest.raises(APIUsageError, match='multiple of 16 bytes'):
        vector.make(vector.make_pixel_squared, env_kwargs=dict(height=9, width=7, channels=3), num_envs=2, backend=vector.PixelSquared)
    with pytest.raises(APIUsageError, match='consecutive seeds'):
        px.async_reset([5, 9, 1, 2, 3, 4, 6, 7])


def test_a_horizon_longer_than_the_tape_is_drawn_in_chunks():
    """What clean_pufferl._rollout_stepwise does for a long horizon on few envs: one-move episodes reset on every other send, so 500
    sends need 250 reset rounds of a ring that holds 192 — one ensure_tape refuses them, chunks of max_sends_per_tape fit, and the run
    stays in lock step with Squared to the end with no underrun."""
    from pufferlib_amd.exceptions import APIUsageError
    n, T, shape = 8, 500, (40, 40, 3, True)
    px, sq = _pixel(n, 1, 1, shape), _squared(n, 1, 1)
    assert px.episode_len == 2 and px.tape_rounds == sq.tape_rounds == 192 and px.max_sends_per_tape == 192 < T
    for v in (px, sq):
        v.async_reset(11)
    with pytest.raises(APIUsageError, match='reset rounds'):
        px.ensure_tape(T)
    g = torch.Generator(device='cuda').manual_seed(5)
    actions = torch.randint(0, 8, (T, n), device='cuda', generator=g)
    chunk, fills = px.max_sends_per_tape, 0
    for t in range(T):
        if t % chunk == 0:
            before = px.rounds_filled
            for v in (px, sq):
                v.ensure_tape(min(chunk, T - t))
            fills += px.rounds_filled > before
        px.device_send(actions[t])
        sq.device_send(actions[t])
    assert fills >= 2 and px.sends == sq.sends == T
    _same_live(px, sq, shape, 'end')
    st = px.stats_with_flag(reset=False).cpu().numpy()
    assert st[4] == 0.0 and st[0] == n * (T // 2)
    assert np.array_equal(st[:4], sq.episode_stats(reset=False).cpu().numpy())
    assert np.array_equal(px.debug_targets(), sq.debug_targets())


def test_the_viewer_loop_hosts_the_creator_on_device(capsys):
    """clean_pufferl.rollout (the loop behind `demo.py --mode eval`) builds vector.PixelSquared for the creator, feeds the policy its
    frames and draws the grid the frames were painted from."""
    from pufferlib_amd import clean_pufferl, vector
    rewards = clean_pufferl.rollout(vector.make_pixel_squared, dict(distance_to_target=2, height=40, width=40, channels=3),
                                    lambda env: _policy('cnn', env.driver_env), {}, steps=5, frame_sleep=0.0)
    out = capsys.readouterr().out
    assert len(rewards) == 5 and out.count('Reward:') == 5 and all(np.isfinite(r) for r in rewards)
    assert out.count('\033[91m') == 5 and '\033[94m' in out       # the agent cell every frame, a target cell


def _config(n, horizon, updates, seed=1, **over):
    from pufferlib_amd import namespace
    B = n * horizon
    kw = dict(env='pixel_squared', seed=seed, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * updates,
              learning_rate=2.5e-3, anneal_lr=True, gamma=0.95, gae_lambda=0.9, update_epochs=4, norm_adv=True, clip_coef=0.1, clip_vloss=True,
              vf_coef=0.5, vf_clip_coef=0.1, max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=B, minibatch_size=B // 4,
              bptt_horizon=16, compile=False, checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='pixel')
    kw.update(over)
    return namespace(**kw)


def _policy(kind, env):
    from pufferlib_amd import cleanrl, models
    if kind == 'resnet':
        return cleanrl.Policy(models.ProcgenResnet(env, cnn_width=16, mlp_width=256))
    net = models.Convolutional(env, framestack=3, flat_size=64, channels_last=True, hidden_size=128, output_size=128)
    if kind == 'cnn_lstm':
        return cleanrl.RecurrentPolicy(models.LSTMWrapper(env, net, input_size=128, hidden_size=128))
    return cleanrl.Policy(net)


def test_the_stepwise_rollout_stores_the_frames_the_env_showed():
    from pufferlib_amd import clean_pufferl
    n, T, shape = 32, 8, (40, 40, 3, True)
    px = _pixel(n, 3, 1, shape)
    torch.manual_seed(0)
    data = clean_pufferl.create(_config(n, T, 4, bptt_horizon=T), px, _policy('cnn', px.driver_env))
    assert data.cnn_engine is not None and data.frame_rows
    clean_pufferl.evaluate(data)
    exp = data.experience
    obs = exp.obs.view(n, T, -1).cpu().numpy()                     # experience rows are env-major
    actions = exp.actions.view(n, T).cpu().numpy()
    rewards = exp.rewards.view(n, T).cpu().numpy()
    sq = _squared(n, 3, 1)
    sq.async_reset(1)                                              # create() resets with config.seed (+ env offset 0)
    for t in range(T):
        assert np.array_equal(obs[:, t], render(sq.observations.cpu().numpy(), *shape).reshape(n, -1)), t
        assert np.array_equal(rewards[:, t], sq.rewards.cpu().numpy()), t
        sq.recv()
        sq.send(actions[:, t])
    _same_live(px, sq, shape, 'after the rollout')


LEARN_UPDATES = {'cnn': 40, 'resnet': 40, 'cnn_lstm': 40}       # chosen from the measured curves (docs/lab-notebook.md): all three sit at their final score from update 27 on


def _learn(kind, updates=None, seed=1, **over):
    """PixelSquared(distance_to_target=1): the agent sits in the middle of a 3 x 3 grid, the target on one of the 8 perimeter cells,
    each of the 8 moves reaches another one of them and the episode is that one move — score 1 on the target, else 0, chance 1/8.
    Returns the score of every report (2048 episodes each) and the wall time."""
    from pufferlib_amd import clean_pufferl
    n, horizon = 256, 16
    updates = LEARN_UPDATES[kind] if updates is None else updates
    px = _pixel(n, 1, 1, (40, 40, 3, True))
    torch.manual_seed(0)
    data = clean_pufferl.create(_config(n, horizon, updates, seed=seed, **over), px, _policy(kind, px.driver_env))
    assert clean_pufferl.route(data.policy.policy, kind == 'cnn_lstm') == {'cnn': 'cnn', 'resnet': 'resnet', 'cnn_lstm': 'general'}[kind]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = []
    for _ in range(updates):
        stats, _ = clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        scores.append(float(stats['score']))
    torch.cuda.synchronize()
    assert np.isfinite(data.losses.value_loss) and bool(torch.isfinite(data.flat_params.flat).all())
    return scores, time.perf_counter() - t0


# kind: (score of the last report, wall seconds of the 40 updates) measured on an MI355X, seed 1 — docs/lab-notebook.md has the curves
MEASURED = {'cnn': (1.0, 0.42), 'resnet': (1.0, 2.39), 'cnn_lstm': (0.9995, 0.94)}
CHANCE = 0.125


@pytest.mark.parametrize('kind', ['cnn', 'resnet', 'cnn_lstm'])
def test_ppo_learns_the_one_move_task_from_pixels(kind):
    """models.Convolutional(hidden_size=128) (route cnn), models.ProcgenResnet(cnn_width=16, mlp_width=256) (route resnet) and the
    recurrent NatureCNN (route general) on 256 envs x horizon 16 of (40, 40, 3) frames, 40 updates with the hyper-parameters of
    tests/test_gpu_learning.py.  Measured on an MI355X (seed 1): the score starts at 0.1333 in all three (chance is exactly 1/8; 2048
    episodes per report put the binomial spread at 0.007) and ends at 1.0 (cnn, 0.42 s; at 0.999 from update 22 on), 1.0 (resnet,
    2.39 s; from update 25 on) and 0.9995 (cnn_lstm, 0.94 s; above 0.99 from update 18 on).  The bar for the last score is the midpoint
    between chance and that measured final score: a policy that learned half the mapping, or one whose frames and first-layer loader
    disagree about the layout, stays under it."""
    scores, wall = _learn(kind)
    print(f'{kind}: first {scores[0]:.4f} last {scores[-1]:.4f} wall {wall:.2f} s scores {[round(s, 3) for s in scores]}')
    assert scores[0] < 2 * CHANCE, scores
    assert scores[-1] > (CHANCE + MEASURED[kind][0]) / 2, scores


def test_the_same_seed_gives_the_same_score_curve_twice():
    """torch_deterministic and the Philox action noise make the engine reproducible; the env's tape, step and painter must keep it so."""
    first, _ = _learn('cnn')
    second, _ = _learn('cnn')
    assert np.array_equal(np.asarray(first), np.asarray(second)), (first, second)
