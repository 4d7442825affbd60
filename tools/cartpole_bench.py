"""Fused MLP rollout of vector.CartPole at 4096 envs x 128 steps, Default(128) and Default(64), next to pfa_rollout_mlp_stochastic on
the same policy shape in the same process: HIP-event times, median (min, max) of 9 launches after two warm-ups, the round run twice.
The lab notebook's "CartPole" section quotes this measurement.

    python tools/cartpole_bench.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pufferlib_amd import _lib, clean_pufferl, cleanrl, models, namespace, vector  # noqa: E402

N, T = 4096, 128


def timed(fn, reps=9, warmup=2):
    ms = []
    for _ in range(reps + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = ms[warmup:]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def one(name, vec, hidden):
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=hidden))
    B = N * T
    cfg = namespace(env=name, seed=5, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * 100, learning_rate=1e-3,
                    anneal_lr=True, gamma=0.97, gae_lambda=0.9, update_epochs=1, norm_adv=True, clip_coef=0.2, clip_vloss=True, vf_coef=0.5,
                    vf_clip_coef=0.2, max_grad_norm=0.5, ent_coef=0.02, target_kl=None, batch_size=B, minibatch_size=B // 4, bptt_horizon=16,
                    compile=False, checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='bench')
    data = clean_pufferl.create(cfg, vec, pol)
    kw = {} if data.gen_engine is None else dict(view=data.gen_engine.mlp_view)
    med, lo, hi = timed(lambda: vec.fused_rollout_mlp(data.flat_params, data.experience, None, _lib.NoiseKey(pol.noise_seed, pol.noise_step),
                                                      _lib.stream_handle(), **kw))
    print(f'{name} Default({hidden}) {N} x {T}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})', flush=True)


if __name__ == '__main__':
    for _ in range(2):
        one('stochastic', vector.make(vector.make_stochastic, num_envs=N, backend=vector.Stochastic), 128)
        one('cartpole', vector.make(vector.make_cartpole, num_envs=N, backend=vector.CartPole), 128)
        one('cartpole', vector.make(vector.make_cartpole, num_envs=N, backend=vector.CartPole), 64)
