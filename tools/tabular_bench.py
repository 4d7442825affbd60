"""What the table walk costs on the fused MLP rollout's per-step chain (developer tool, not product code).

In ONE process, on the same policy weights: the fused rollout of ocean Stochastic written as a table (pfa_rollout_mlp_tabular), the
hand-written family's fused rollout (pfa_rollout_mlp_stochastic) and Tabular's own stepwise path (policy step + store + send per step),
4096 envs x 128 steps, HIP-event times after warm-up, median of --reps (default 25).
    python tools/tabular_bench.py [--envs 4096] [--steps 128] [--reps 25]
Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))       # tabular_reference.stochastic_as_table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import tabular_reference
    from pufferlib_amd import _lib, clean_pufferl, cleanrl, models, namespace, vector
    n, T = args.envs, args.steps

    def config():
        return namespace(env='tabular', seed=5, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=n * T * 1000,
                         learning_rate=1e-3, anneal_lr=True, gamma=0.97, gae_lambda=0.9, update_epochs=1, norm_adv=True, clip_coef=0.2,
                         clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.2, max_grad_norm=0.5, ent_coef=0.02, target_kl=None, batch_size=n * T,
                         minibatch_size=n * T // 4, bptt_horizon=16, compile=False, checkpoint_interval=0, data_dir='/tmp/pfa_experiments',
                         exp_id='tabular_bench')
    tab = vector.make(vector.make_tabular, env_kwargs=dict(mdp=tabular_reference.stochastic_as_table(0.7)), num_envs=n, backend=vector.Tabular)
    sto = vector.make(vector.make_stochastic, env_kwargs=dict(p=0.7), num_envs=n, backend=vector.Stochastic)
    torch.manual_seed(0)
    pol_t = cleanrl.Policy(models.Default(tab.driver_env))
    pol_s = cleanrl.Policy(models.Default(sto.driver_env))
    pol_s.load_state_dict(pol_t.state_dict())
    dt, ds = clean_pufferl.create(config(), tab, pol_t), clean_pufferl.create(config(), sto, pol_s)

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms[args.warmup:]))

    def fused(data):
        vec, pol = data.vecenv, data.policy
        return lambda: vec.fused_rollout_mlp(data.flat_params, data.experience, None, _lib.NoiseKey(pol.noise_seed, pol.noise_step),
                                             _lib.stream_handle())
    out = dict(envs=n, steps=T, reps=args.reps,
               fused_tabular_ms=timed(fused(dt)), fused_stochastic_ms=timed(fused(ds)),
               stepwise_tabular_ms=timed(lambda: clean_pufferl._rollout_stepwise(dt, None, T, n)))
    # the same start, policy and noise stream: the two families' rollouts agree row for row
    for data in (dt, ds):
        data.vecenv.async_reset(5)
        fused(data)()
    same = all(torch.equal(getattr(dt.experience, k), getattr(ds.experience, k)) for k in ('actions', 'logprobs', 'values', 'rewards', 'dones'))
    out.update(tabular_over_stochastic=out['fused_tabular_ms'] / out['fused_stochastic_ms'],
               stepwise_over_fused=out['stepwise_tabular_ms'] / out['fused_tabular_ms'],
               tabular_steps_per_s=n * T / out['fused_tabular_ms'] * 1e3, rollouts_identical=bool(same))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
