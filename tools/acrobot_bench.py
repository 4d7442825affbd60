"""Fused MLP rollout of vector.Acrobot at 4096 envs x 128 steps, Default(128) and Default(64), next to pfa_rollout_mlp_stochastic and
vector.CartPole's rollout on the same policy shapes in the same process, so that the ratios come from one job: HIP-event times,
median (min, max) of 9 launches after two warm-ups, the round run twice.  Then the end-to-end steps/s of a Default(64) training
iteration (evaluate + train, 4096 x 128, the learning test's settings), median of 9 after two warm-ups.  The lab notebook's
"Acrobot" section quotes this measurement.

    python tools/acrobot_bench.py
"""
import os
import sys
import time

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


def config(name, B, nmb=4, lr=1e-3, epochs=1):
    return namespace(env=name, seed=5, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * 100, learning_rate=lr,
                     anneal_lr=True, gamma=0.99, gae_lambda=0.95, update_epochs=epochs, norm_adv=True, clip_coef=0.2, clip_vloss=True, vf_coef=0.5,
                     vf_clip_coef=0.2, max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=B, minibatch_size=B // nmb, bptt_horizon=16,
                     compile=False, checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='bench')


def one(name, vec, hidden):
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=hidden))
    data = clean_pufferl.create(config(name, N * T), vec, pol)
    kw = {} if data.gen_engine is None else dict(view=data.gen_engine.mlp_view)
    med, lo, hi = timed(lambda: vec.fused_rollout_mlp(data.flat_params, data.experience, None, _lib.NoiseKey(pol.noise_seed, pol.noise_step),
                                                      _lib.stream_handle(), **kw))
    print(f'{name} Default({hidden}) {N} x {T}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})', flush=True)


def iteration(hidden=64):
    vec = vector.make(vector.make_acrobot, num_envs=N, backend=vector.Acrobot)
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=hidden))
    data = clean_pufferl.create(config('acrobot', N * T, nmb=8, lr=5e-3, epochs=4), vec, pol)
    s = []
    for _ in range(11):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    med = float(np.median(s[2:]))
    print(f'acrobot Default({hidden}) evaluate + train, {N} x {T}, 4 epochs x 8 minibatches: median {med * 1e3:.2f} ms = {N * T / med / 1e6:.1f} M steps/s',
          flush=True)


if __name__ == '__main__':
    for _ in range(2):
        for hidden in (128, 64):
            if hidden == 128:       # Stochastic has the flat 128-wide rollout only
                one('stochastic', vector.make(vector.make_stochastic, num_envs=N, backend=vector.Stochastic), hidden)
            one('cartpole', vector.make(vector.make_cartpole, num_envs=N, backend=vector.CartPole), hidden)
            one('acrobot', vector.make(vector.make_acrobot, num_envs=N, backend=vector.Acrobot), hidden)
    iteration()
