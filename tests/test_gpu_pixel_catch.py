"""vector.PixelCatch on the GPU (csrc/catch_env.hpp, csrc/pixel_catch.hip): bit for bit against the numpy walker of
tests/catch_reference.py, the meaning of the time stack, PPO learning the task from the stack, and the trainer's refusal."""
import numpy as np
import pytest
import torch

from catch_reference import CatchWalker

pytestmark = pytest.mark.gpu

# (rows, cols, framestack, height, width).  Grid 4 x 3 in 9 x 8 frames (9 x 16 for one channel: the 16-byte rule): uneven cells, and
# channel-first chunks that cross channels.  Grid 5 x 2: a bounce on every move; its stack of 3 is the channel-last form whose first
# channel differs from lane to lane.  Grid 4 x 8 in 10 x 8: width == cols.  The last three have more chunks than a workgroup has lanes.
CASES = [(4, 3, 1, 9, 16), (4, 3, 2, 9, 8), (4, 3, 4, 9, 8), (5, 2, 1, 12, 12), (5, 2, 2, 12, 12), (5, 2, 3, 12, 12), (5, 2, 4, 12, 12),
         (4, 8, 1, 10, 8), (4, 8, 2, 10, 8), (4, 8, 4, 10, 8), (10, 8, 4, 84, 84), (7, 5, 3, 64, 60), (6, 5, 4, 42, 42)]
# 48 envs and envs 32..47 of them as a vecenv of their own, three episodes; then the env counts from which a workgroup of the send
# kernel owns 2, 4 and 8 envs (catch_envs_per_wg), the last workgroup 1, 3 and 3
PARITY = [(48, c, 3, (32, 16)) for c in CASES] + [(n, (4, 3, 4, 9, 8), 1, None) for n in (2049, 4099, 8195)]


def _make(n, case, channels_last, **kw):
    from pufferlib_amd import vector
    kwargs = dict(zip(('rows', 'cols', 'framestack', 'height', 'width'), case), channels_last=channels_last)
    return vector.make(vector.make_pixel_catch, num_envs=n, backend=vector.PixelCatch, env_kwargs=kwargs, **kw)


def _same(vec, walker, rows, where):
    o, r, te, tr, infos, ids, mask = vec.recv()
    assert np.array_equal(o.cpu().numpy(), walker.frames()[rows]), ('frames', where)
    assert np.array_equal(r.cpu().numpy(), walker.rewards[rows]) and np.array_equal(te.cpu().numpy(), walker.terminals[rows]), where
    assert not tr.any() and bool(mask.all())
    for got, want in zip(vec.debug_states(), walker.states()):
        assert np.array_equal(got, want[rows]), ('states', where)


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('n,case,episodes,part', PARITY)
def test_trajectory_parity(n, case, episodes, part, channels_last):
    """Under seeded random actions, `episodes` episodes and one send: frames, rewards, terminals, the env states, infos and the
    statistics sums equal the walker's at every send, in the whole vecenv and in the one that starts at env_offset part[0]."""
    walker = CatchWalker(n, *case, channels_last)
    vecs = [(_make(n, case, channels_last), slice(0, n), np.zeros(4))]
    if part:
        vecs.append((_make(part[1], case, channels_last, env_offset=part[0]), slice(part[0], sum(part)), np.zeros(4)))
    walker.async_reset(42)
    for vec, rows, _ in vecs:
        vec.async_reset(42)
        _same(vec, walker, rows, 'reset')
    rng = np.random.default_rng(7)
    for t in range(episodes * (case[0] - 1) + 1):
        a = rng.integers(0, 3, n)
        walker.send(a)
        for vec, rows, sums in vecs:
            vec.send(a[rows])
            _same(vec, walker, rows, t)
            want = [i for e, i in zip(np.nonzero(walker.terminals)[0], walker.infos) if rows.start <= e < rows.stop]
            assert vec.infos == want, t
            sums += [len(want)] + [sum(i[k] for i in want) for k in ('episode_return', 'episode_length', 'score')]
    assert walker.sums[0] == episodes * n and 0 < walker.sums[3] < walker.sums[0]       # both endings happened
    assert np.array_equal(vecs[0][2], walker.sums)
    for vec, rows, sums in vecs:
        assert np.array_equal(vec.episode_stats().cpu().numpy(), sums)


@pytest.mark.parametrize('channels_last', [False, True])
def test_stack_semantics(channels_last):
    """After a reset all channels are equal; inside an episode channel k at send t is channel k + 1 at send t - 1."""
    case, n = (6, 5, 4, 12, 20), 48
    vec = _make(n, case, channels_last)
    vec.async_reset(3)
    chan = lambda: np.moveaxis(vec.observations.cpu().numpy(), -1 if channels_last else 1, 1)       # [N][channel][H][W]
    prev = chan()
    assert (prev == prev[:, :1]).all()
    for t in range(1, 2 * (case[0] - 1) + 1):
        vec.recv()
        vec.send(np.full(n, t % 3))
        cur = chan()
        if t % (case[0] - 1) == 0:
            assert bool(vec.terminals.all()) and (cur == cur[:, :1]).all()
        else:
            assert not bool(vec.terminals.any()) and np.array_equal(cur[:, :-1], prev[:, 1:])
            assert (cur[:, -1] != cur[:, -2]).reshape(n, -1).any(1).all()      # the ball fell one row: the newest channel is new
        prev = cur


# Grid 6 x 5 in 40 x 40 frames, 256 envs x horizon 20 (1024 episodes a report).  Uniformly random actions score exactly 1/5: the walker
# over all 75 start states x 3^5 action sequences counts 3645 catches of 18225.  MEASURED: the last of 40 reports on an MI355X at seed 1,
# the same in a process of its own and behind this file's other tests (docs/lab-notebook.md has the curves).
CHANCE, UPDATES, MEASURED = 0.2, 40, dict(cnn=1.0, resnet=0.9980)


def _learn(kind, seed=1):
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace
    n, horizon = 256, 20
    vec = _make(n, (6, 5, 4, 40, 40), kind == 'resnet')
    B = n * horizon         # (the hyper-parameters of tests/test_gpu_pixel_squared.py)
    config = namespace(env='pixel_catch', seed=seed, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * UPDATES,
                       learning_rate=2.5e-3, anneal_lr=True, gamma=0.95, gae_lambda=0.9, update_epochs=4, norm_adv=True, clip_coef=0.1,
                       clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.1, max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=B,
                       minibatch_size=B // 4, bptt_horizon=20, compile=False, checkpoint_interval=0, data_dir='/tmp/pfa_experiments',
                       exp_id='pixel_catch')
    torch.manual_seed(0)        # the initial weights are drawn from the global generator: seed it before the module is built
    net = (models.ProcgenResnet(vec.driver_env, cnn_width=16, mlp_width=256) if kind == 'resnet' else
           models.Convolutional(vec.driver_env, framestack=4, flat_size=64, channels_last=False, hidden_size=128, output_size=128))
    data = clean_pufferl.create(config, vec, cleanrl.Policy(net))
    scores = []
    for _ in range(UPDATES):
        stats, _ = clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        scores.append(float(stats['score']))
    assert bool(torch.isfinite(data.flat_params.flat).all())
    return scores


@pytest.mark.parametrize('kind', ['cnn', 'resnet'])
def test_ppo_learns_to_catch_from_the_stack(kind):
    """models.Convolutional on channel-first (4, 40, 40) frames, models.ProcgenResnet on channel-last (40, 40, 4) ones: the landing
    column needs the velocity, which only two channels together show.  The bar: midway between chance and the measured last score."""
    scores = _learn(kind)
    print(f'{kind}: scores {[round(s, 4) for s in scores]}')
    assert scores[0] < 2 * CHANCE, scores
    assert scores[-1] > (CHANCE + MEASURED[kind]) / 2, scores


def test_the_same_seed_gives_the_same_curve_twice_on_channel_first_frames():
    assert _learn('cnn') == _learn('cnn')


def test_a_policy_that_reads_no_frames_is_refused():
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace
    vec = _make(8, (4, 3, 2, 9, 8), False)
    config = namespace(seed=1, torch_deterministic=True, batch_size=64, bptt_horizon=8, minibatch_size=64, learning_rate=1e-3)
    with pytest.raises(NotImplementedError, match=r'vector\.PixelCatch'):
        clean_pufferl.create(config, vec, cleanrl.Policy(models.Default(vec.driver_env)))
