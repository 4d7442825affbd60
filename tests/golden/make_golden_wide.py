"""Generate tests/golden/ppo_bandit_wide.npz by RUNNING THE UNMODIFIED REFERENCE on an action space beyond 63 logits: ocean's
make_bandit(num_actions=100).

Run in the build container only (needs the reference checkout make_golden.py points at):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide.py

The recipe of make_golden.gen_ppo / make_golden_resnet.py: clean_pufferl.create / evaluate / train (clean_pufferl.py:30-292) with
pufferlib.models.Default(hidden_size=128) behind frameworks.cleanrl.Policy on pufferlib.vector.Serial over make_bandit, 8 envs x 16
steps, one iteration; the multinomial's exponential draws recorded (8 x 16 x 100 floats), big tensors as digests, weights from the
start-weight recipe of cnn_golden.py (not stored).  Nothing of the reference is copied: its public functions are called and their
inputs and outputs recorded.

The script checks, in float64, that in every recorded sampling row the gap between the best and the second-best `log p - log noise`
is above 1e-4 (the GPU test compares actions exactly), and fails otherwise: pick another SEED then."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (puts the shims and the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

NUM_ACTIONS, SEED = 100, 1


def gen(num_envs=8, horizon=16):
    import pufferlib
    import pufferlib.vector
    import pufferlib.models
    import pufferlib.frameworks.cleanrl
    import pufferlib.environments.ocean as ocean
    import clean_pufferl

    class _NoUtil:
        def __init__(self, *a, **k):
            self.cpu_util = self.cpu_mem = self.gpu_util = self.gpu_mem = [0]

        def stop(self):
            pass

    clean_pufferl.Utilization = _NoUtil
    clean_pufferl.print_dashboard = lambda *a, **k: None
    clean_pufferl.save_checkpoint = lambda data: None

    batch = num_envs * horizon
    config = pufferlib.namespace(
        env='bandit', seed=SEED, torch_deterministic=True, cpu_offload=False, device='cpu',
        total_timesteps=batch * 8, learning_rate=2.5e-4, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
        update_epochs=2, norm_adv=True, clip_coef=0.1, clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.1,
        max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=batch, minibatch_size=batch // 2,
        bptt_horizon=8, compile=False, compile_mode='reduce-overhead', checkpoint_interval=10 ** 9,
        data_dir='/tmp/golden_experiments', exp_id='golden')
    vec = pufferlib.vector.make(ocean.env_creator('bandit'), env_kwargs=dict(num_actions=NUM_ACTIONS), num_envs=num_envs,
                                backend=pufferlib.vector.Serial)
    assert vec.single_action_space.n == NUM_ACTIONS
    torch.manual_seed(SEED)
    policy = pufferlib.frameworks.cleanrl.Policy(pufferlib.models.Default(vec.driver_env, hidden_size=128))
    out = {'num_actions': np.array(NUM_ACTIONS, np.int64)}
    with torch.no_grad():
        for k, v in policy.state_dict().items():
            v.copy_(torch.from_numpy(mg.cnn_start_weight(k[len('policy.'):], tuple(v.shape))))
    for k, v in policy.state_dict().items():
        out['w0.' + k] = mg.digest(v.detach().numpy())
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
        clean_pufferl.evaluate(data)
        out['it0.noise'] = np.stack(noise)[:horizon]                              # (T, N, A)
        out['it0.obs'] = exp.obs.numpy().reshape(batch, -1).astype(np.int8)
        out['it0.actions'] = exp.actions_np.copy().astype(np.int16)
        out['it0.logprobs'] = exp.logprobs_np.copy()
        out['it0.rewards'] = exp.rewards_np.copy()
        out['it0.dones'] = exp.dones_np.copy()
        out['it0.values'] = exp.values_np.copy()
        out['it0.global_step'] = np.array(data.global_step, np.int64)
        gaps = []
        for p, q in zip(probs[:horizon], noise[:horizon]):
            score = np.log(p.astype(np.float64)) - np.log(q.astype(np.float64))
            top = np.sort(score, axis=-1)
            gaps.append(top[:, -1] - top[:, -2])
        out['it0.min_gap'] = np.array(float(np.min(gaps)))
        assert out['it0.min_gap'] > 1e-4, f'a sampling row is a near tie ({out["it0.min_gap"]:.3e}): choose another SEED'
        lr_used = data.optimizer.param_groups[0]['lr']
        clean_pufferl.train(data)
        out['it0.lr_used'] = np.array(lr_used, np.float64)
        out['it0.advantages'] = exp.b_advantages.numpy().copy()                   # (nmb, minibatch)
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
    np.savez_compressed(os.path.join(HERE, 'ppo_bandit_wide.npz'), **out)
    print('ppo_bandit_wide.npz', len(out), 'arrays; min sampling gap %.4f; distinct actions %d; losses' %
          (out['it0.min_gap'], len(np.unique(out['it0.actions']))), out['it0.losses'])


if __name__ == '__main__':
    gen()
