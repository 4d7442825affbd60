"""Generate tests/golden/ppo_conv_<tag>.npz by RUNNING THE UNMODIFIED REFERENCE at the frame geometries of tests/conv_geometry.py.

Run in the build container only (needs the reference checkout make_golden.py points at):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conv.py

Same recipe as make_golden.gen_ppo_cnn: clean_pufferl.create / evaluate / train (clean_pufferl.py:30-292) with
pufferlib.models.Convolutional built with the geometry's constructor arguments behind frameworks.cleanrl.Policy (or
RecurrentPolicy(LSTMWrapper(512, 512)) for the `_lstm` fixture), on a stub env whose frames tests/conv_geometry.frame regenerates
from recorded frame numbers; `Serial` backend, the multinomial's exponential draws recorded, big tensors as digests.  18 actions,
4 envs x 16 steps, one iteration, lr 2.5e-4.  Nothing of the reference is copied: its public functions are called and their inputs
and outputs recorded.

The script checks, in float64, that in every recorded sampling row the gap between the best and the second-best `log p - log noise`
is above 1e-4 (the GPU test compares actions exactly, without an exclusion list) and fails otherwise: choose another seed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the shims and the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import conv_geometry as cg  # noqa: E402

ACTIONS = 18


def gen(tag, use_rnn=False, num_envs=4, horizon=16, seed=1):
    import gymnasium
    import pufferlib
    import pufferlib.emulation
    import pufferlib.postprocess
    import pufferlib.vector
    import pufferlib.models
    import pufferlib.frameworks.cleanrl
    import clean_pufferl

    class _NoUtil:
        def __init__(self, *a, **k):
            self.cpu_util = self.cpu_mem = self.gpu_util = self.gpu_mem = [0]

        def stop(self):
            pass

    clean_pufferl.Utilization = _NoUtil
    clean_pufferl.print_dashboard = lambda *a, **k: None
    clean_pufferl.save_checkpoint = lambda data: None
    counters = {'next': 0}
    geo = cg.GEOMETRIES[tag]

    class FrameEnv(gymnasium.Env):
        def __init__(self):
            self.observation_space = gymnasium.spaces.Box(low=0, high=255, shape=geo['obs'], dtype=np.uint8)
            self.action_space = gymnasium.spaces.Discrete(ACTIONS)
            self.render_mode = 'ansi'
            self.tick = 0
            self.frame = None
            self.counter = -1

        def _draw(self):
            self.counter = counters['next']
            counters['next'] += 1
            self.frame = cg.frame(tag, self.counter)
            return self.frame

        def reset(self, seed=None):
            self.tick = 0
            return self._draw(), {}

        def step(self, action):
            reward = float(int(action) == int(self.frame.reshape(-1)[0]) % ACTIONS)
            self.tick += 1
            done = self.tick >= 5
            return self._draw(), reward, done, False, {'score': reward} if done else {}

    def make_env():
        return pufferlib.emulation.GymnasiumPufferEnv(env=pufferlib.postprocess.EpisodeStats(FrameEnv()))

    batch = num_envs * horizon
    config = pufferlib.namespace(
        env='frames', seed=seed, torch_deterministic=True, cpu_offload=False, device='cpu',
        total_timesteps=batch * 8, learning_rate=2.5e-4, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
        update_epochs=2, norm_adv=True, clip_coef=0.1, clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.1,
        max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=batch, minibatch_size=batch // 2,
        bptt_horizon=8, compile=False, compile_mode='reduce-overhead', checkpoint_interval=10 ** 9,
        data_dir='/tmp/golden_experiments', exp_id='golden')
    vec = pufferlib.vector.make(make_env, num_envs=num_envs, backend=pufferlib.vector.Serial)
    torch.manual_seed(seed)
    net = pufferlib.models.Convolutional(vec.driver_env, **geo['kwargs'])
    hid = cg.hidden_of(tag)
    if use_rnn:
        policy = pufferlib.frameworks.cleanrl.RecurrentPolicy(pufferlib.models.LSTMWrapper(vec.driver_env, net, input_size=hid, hidden_size=hid))
    else:
        policy = pufferlib.frameworks.cleanrl.Policy(net)
    bare = lambda k: k.split('.', 2)[2] if use_rnn else k[len('policy.'):]  # noqa: E731
    out = {}
    with torch.no_grad():
        for k, v in policy.state_dict().items():
            v.copy_(torch.from_numpy(cg.start_weight(bare(k), tuple(v.shape))))
    for k, v in policy.state_dict().items():
        out['w0.' + k] = mg.digest(v.detach().numpy())
    w64 = {bare(k): v.detach().double().clone() for k, v in policy.state_dict().items()}
    noise, probs = [], []
    orig_multinomial = torch.multinomial

    def recording_multinomial(p, n, *a, **kw):
        st = torch.get_rng_state()
        res = orig_multinomial(p, n, *a, **kw)
        st2 = torch.get_rng_state()
        torch.set_rng_state(st)
        q = torch.empty_like(p).exponential_(1)
        assert torch.equal((p / q).argmax(-1, keepdim=True), res), 'multinomial != argmax(p/q)'
        torch.set_rng_state(st2)
        noise.append(q.numpy().copy())
        probs.append(p.detach().numpy().copy())
        return res

    torch.multinomial = recording_multinomial
    try:
        data = clean_pufferl.create(config, vec, policy)
        exp = data.experience
        frame_ids = []
        orig_recv = vec.recv

        def recv():
            frame_ids.append([env.env.env.counter for env in vec.envs])
            return orig_recv()
        vec.recv = recv
        clean_pufferl.evaluate(data)
        vec.recv = orig_recv
        out['it0.frame_ids'] = np.array(frame_ids[:horizon], np.int64)            # (T, N)
        obs = exp.obs.numpy().reshape(batch, *geo['obs'])
        for t in range(horizon):
            for e in range(num_envs):
                assert np.array_equal(obs[t * num_envs + e], cg.frame(tag, frame_ids[t][e])), (t, e)
        out['it0.noise'] = np.stack(noise)                                        # (T, N, A)
        out['it0.actions'] = exp.actions_np.copy().astype(np.int8)
        out['it0.logprobs'] = exp.logprobs_np.copy()
        out['it0.rewards'] = exp.rewards_np.copy()
        out['it0.dones'] = exp.dones_np.copy()
        out['it0.values'] = exp.values_np.copy()
        out['it0.global_step'] = np.array(data.global_step, np.int64)
        # sampling margins in float64 on the probabilities the reference sampled from
        gaps = []
        for p, q in zip(probs, noise):
            score = np.log(p.astype(np.float64)) - np.log(q.astype(np.float64))
            top = np.sort(score, axis=-1)
            gaps.append(top[:, -1] - top[:, -2])
        out['it0.min_gap'] = np.array(float(np.min(gaps)))
        assert out['it0.min_gap'] > 1e-4, f'{tag}: a sampling row is a near tie ({out["it0.min_gap"]:.3e}): choose another seed'
        if not use_rnn:   # the float64 restatement of tests/conv_geometry.py on the recorded rollout, for the CPU test that pins it
            fr = np.stack([cg.frame(tag, frame_ids[t][e]) for t in range(horizon) for e in range(num_envs)])
            _, _, _, h = cg.encode(tag, torch.from_numpy(fr), w64)
            logits, value, _, _, _, _ = cg.heads(h, w64, actions=torch.zeros(batch, dtype=torch.long))
            with torch.no_grad():
                ref_logits, ref_value = net(torch.from_numpy(fr))
            out['it0.logits'] = mg.digest(ref_logits.numpy())                     # the reference module's own forward (fp32)
            assert np.abs(logits.numpy() - ref_logits.numpy()).max() < 1e-5 and np.abs(value.numpy() - ref_value.numpy().reshape(-1)).max() < 1e-5
        else:
            out['it0.lstm_h'] = exp.lstm_h.numpy().copy()
            out['it0.lstm_c'] = exp.lstm_c.numpy().copy()
        lr_used = data.optimizer.param_groups[0]['lr']
        clean_pufferl.train(data)
        out['it0.lr_used'] = np.array(lr_used, np.float64)
        out['it0.advantages'] = exp.b_advantages.numpy().copy()
        out['it0.returns'] = exp.b_returns.numpy().copy()
        L = data.losses
        out['it0.losses'] = np.array([L.policy_loss, L.value_loss, L.entropy, L.old_approx_kl, L.approx_kl, L.clipfrac,
                                      L.explained_variance], np.float64)
        for k, v in policy.state_dict().items():
            out['it0.w.' + k] = mg.digest(v.detach().numpy())
    finally:
        torch.multinomial = orig_multinomial
    out['config'] = np.array([num_envs, horizon, config.minibatch_size, config.bptt_horizon, config.update_epochs,
                              config.total_timesteps, 1], np.int64)
    out['hparams'] = np.array([config.learning_rate, config.gamma, config.gae_lambda, config.clip_coef, config.vf_coef,
                               config.vf_clip_coef, config.max_grad_norm, config.ent_coef], np.float64)
    fname = f'ppo_conv_{tag}_lstm.npz' if use_rnn else f'ppo_conv_{tag}.npz'
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, len(out), 'arrays; min sampling gap %.4f; losses' % out['it0.min_gap'], out['it0.losses'])


if __name__ == '__main__':
    which = sys.argv[1:] or ['vizdoom', 'crafter', 'butterfly', 'vizdoom_lstm']
    for name in which:
        gen(name.replace('_lstm', ''), use_rnn=name.endswith('_lstm'))
