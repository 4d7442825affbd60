"""Generate tests/golden/ppo_resnet.npz by RUNNING THE UNMODIFIED REFERENCE with pufferlib.models.ProcgenResnet at the frame shapes
`tiny` and `procgen` of tests/resnet_reference.py.

Run in the build container only (needs the reference checkout make_golden.py points at):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resnet.py

The recipe of make_golden_conv.py: clean_pufferl.create / evaluate / train (clean_pufferl.py:30-292) with the reference's class behind
frameworks.cleanrl.Policy on a stub env whose frames tests/resnet_reference.frame regenerates from recorded frame numbers; `Serial`
backend, the multinomial's exponential draws recorded, big tensors as digests, weights from the start_weight recipe (not stored).
15 actions, 4 envs x 16 steps, one iteration, lr 2.5e-4.  Also recorded: the state_dict's key and shape list, and the parameter count.
Nothing of the reference is copied: its public functions are called and their inputs and outputs recorded.

The script checks, in float64, that in every recorded sampling row the gap between the best and the second-best `log p - log noise`
is above 1e-4 (the GPU test compares actions exactly) and that the float64 restatement of tests/resnet_reference.py agrees with the
reference module's own forward, and fails otherwise."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the shims and the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import resnet_reference as rr  # noqa: E402

ACTIONS = rr.ACTIONS


def gen(tag, out, num_envs=4, horizon=16, seed=1):
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
    shape = rr.SHAPES[tag]

    class FrameEnv(gymnasium.Env):
        def __init__(self):
            self.observation_space = gymnasium.spaces.Box(low=0, high=255, shape=shape['obs'], dtype=np.uint8)
            self.action_space = gymnasium.spaces.Discrete(ACTIONS)
            self.render_mode = 'ansi'
            self.tick = 0
            self.frame = None
            self.counter = -1

        def _draw(self):
            self.counter = counters['next']
            counters['next'] += 1
            self.frame = rr.frame(tag, self.counter)
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
    net = pufferlib.models.ProcgenResnet(vec.driver_env, cnn_width=shape['cnn_width'], mlp_width=shape['mlp_width'])
    policy = pufferlib.frameworks.cleanrl.Policy(net)
    pre = tag + '.'
    sd = net.state_dict()
    out[pre + 'keys'] = np.array(list(sd.keys()))
    out[pre + 'shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)
    out[pre + 'param_count'] = np.array(sum(p.numel() for p in net.parameters()), np.int64)
    with torch.no_grad():
        for k, v in policy.state_dict().items():
            v.copy_(torch.from_numpy(rr.start_weight(k[len('policy.'):], tuple(v.shape))))
    for k, v in policy.state_dict().items():
        out[pre + 'w0.' + k] = mg.digest(v.detach().numpy())
    w64 = {k[len('policy.'):]: v.detach().double().clone() for k, v in policy.state_dict().items()}
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
        out[pre + 'it0.frame_ids'] = np.array(frame_ids[:horizon], np.int64)            # (T, N)
        obs = exp.obs.numpy().reshape(batch, *shape['obs'])
        for t in range(horizon):
            for e in range(num_envs):
                assert np.array_equal(obs[t * num_envs + e], rr.frame(tag, frame_ids[t][e])), (t, e)
        out[pre + 'it0.noise'] = np.stack(noise)                                        # (T, N, A)
        out[pre + 'it0.actions'] = exp.actions_np.copy().astype(np.int8)
        out[pre + 'it0.logprobs'] = exp.logprobs_np.copy()
        out[pre + 'it0.rewards'] = exp.rewards_np.copy()
        out[pre + 'it0.dones'] = exp.dones_np.copy()
        out[pre + 'it0.values'] = exp.values_np.copy()
        out[pre + 'it0.global_step'] = np.array(data.global_step, np.int64)
        gaps = []
        for p, q in zip(probs, noise):
            score = np.log(p.astype(np.float64)) - np.log(q.astype(np.float64))
            top = np.sort(score, axis=-1)
            gaps.append(top[:, -1] - top[:, -2])
        out[pre + 'it0.min_gap'] = np.array(float(np.min(gaps)))
        assert out[pre + 'it0.min_gap'] > 1e-4, f'{tag}: a sampling row is a near tie ({out[pre + "it0.min_gap"]:.3e}): choose another seed'
        # the float64 restatement of tests/resnet_reference.py on the recorded rollout against the reference module's own forward
        fr = np.stack([rr.frame(tag, frame_ids[t][e]) for t in range(horizon) for e in range(num_envs)])
        _, h = rr.encode(tag, torch.from_numpy(fr), w64)
        logits, value, _, _, _, _ = rr.heads(h, w64, actions=torch.zeros(batch, dtype=torch.long))
        with torch.no_grad():
            ref_logits, ref_value = net(torch.from_numpy(fr))
        out[pre + 'it0.logits'] = ref_logits.numpy().copy()                             # the reference module's own forward (fp32)
        assert np.abs(logits.numpy() - ref_logits.numpy()).max() < 1e-5 and np.abs(value.numpy() - ref_value.numpy().reshape(-1)).max() < 1e-5
        lr_used = data.optimizer.param_groups[0]['lr']
        clean_pufferl.train(data)
        out[pre + 'it0.lr_used'] = np.array(lr_used, np.float64)
        out[pre + 'it0.advantages'] = exp.b_advantages.numpy().copy()
        out[pre + 'it0.returns'] = exp.b_returns.numpy().copy()
        L = data.losses
        out[pre + 'it0.losses'] = np.array([L.policy_loss, L.value_loss, L.entropy, L.old_approx_kl, L.approx_kl, L.clipfrac,
                                            L.explained_variance], np.float64)
        for k, v in policy.state_dict().items():
            out[pre + 'it0.w.' + k] = mg.digest(v.detach().numpy())
    finally:
        torch.multinomial = orig_multinomial
    out[pre + 'config'] = np.array([num_envs, horizon, config.minibatch_size, config.bptt_horizon, config.update_epochs,
                                    config.total_timesteps, 1], np.int64)
    out[pre + 'hparams'] = np.array([config.learning_rate, config.gamma, config.gae_lambda, config.clip_coef, config.vf_coef,
                                     config.vf_clip_coef, config.max_grad_norm, config.ent_coef], np.float64)
    print(tag, 'min sampling gap %.4f; losses' % out[pre + 'it0.min_gap'], out[pre + 'it0.losses'])


if __name__ == '__main__':
    arrays = {}
    for name in ('tiny', 'procgen'):
        gen(name, arrays)
    np.savez_compressed(os.path.join(HERE, 'ppo_resnet.npz'), **arrays)
    print('ppo_resnet.npz', len(arrays), 'arrays')
