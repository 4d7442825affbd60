"""Per-layer timing and end-to-end env steps/s of models.ProcgenResnet at Procgen's (64, 64, 3) frames (developer tool, not product
code; the settings of tools/conv_geometry_bench.py, so the two tables can sit side by side).

    python tools/resnet_bench.py layers [frames]     forward, dX and dW of every convolution, the two pool kernels and the Linear
                                                     (default 4096 frames): time, TFLOP/s and the fraction of the fp32-MFMA peak
    python tools/resnet_bench.py train [envs]        create / evaluate / train on vector.Frames(64, 64, framestack=3, channels_last=True),
                                                     [envs] x 16 steps, one minibatch, the c4 hyper-parameters: env steps/s

Launches go through the engine's own layer objects, timed with HIP events on their stream (median of 5 after 2 warm-ups).
TFLOP/s = algorithmic flop (2 m n k) / time against 157.3 TFLOP/s (256 CUs x 256 flop / clock x 2.4 GHz); the pool kernels move
bytes, not flop: GB/s."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
PEAK_TFLOPS = 157.3
OBS, ACTIONS = (64, 64, 3), 15


class _Env:
    single_observation_space = type('Box', (), {'shape': OBS, 'dtype': 'uint8'})()
    single_action_space = type('Discrete', (), {'n': ACTIONS})()


def _timed(fn, reps=5, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2]


def _row(name, flop, **times):
    row = dict(layer=name, mflop_per_frame=None)
    for k, (t, f) in times.items():
        row[k + '_us'] = round(t * 1e6, 1)
        row[k + '_tflops'] = round(f / t / 1e12, 2)
        row[k + '_peak_fraction'] = round(f / t / 1e12 / PEAK_TFLOPS, 3)
    return row


def layers(n):
    import torch
    from pufferlib_amd import models, resnet
    torch.manual_seed(0)
    rp = models.ResnetParams(models.ProcgenResnet(_Env()), 'cuda')
    eng = resnet.Engine(rp, chunk=n)
    m = min(n, eng.chunk)
    g = torch.Generator(device='cuda').manual_seed(1)
    frames = torch.randint(0, 256, (m, eng.frame_bytes), dtype=torch.uint8, device='cuda', generator=g)
    eng.forward(frames, m)                                   # every map holds real values
    total = dict(fwd=0.0, dx=0.0, dw=0.0)
    for i, s in enumerate(eng.seqs):
        for t in (s.gc, s.g0, s.g1, s.gt):
            t.normal_(generator=g)
        x_in = frames if i == 0 else eng.seqs[i - 1].x2
        jobs = [('conv', s.conv, x_in, s.c, s.gc, None if i == 0 else eng.seqs[i - 1].g0), ('res_block0.conv0', s.b0c0, s.p, s.t0, s.gt, s.g1),
                ('res_block0.conv1', s.b0c1, s.t0, s.x1, s.g0, s.gt), ('res_block1.conv0', s.b1c0, s.x1, s.t1, s.gt, s.g1),
                ('res_block1.conv1', s.b1c1, s.t1, s.x2, s.g0, s.gt)]
        for name, layer, x, out, dout, dx in jobs:
            flop = 2 * layer.rows(m) * layer.OC * layer.K
            gw, gb = torch.empty_like(layer.w), torch.empty_like(layer.b)
            times = dict(fwd=(_timed(lambda: layer.forward(x, m, out)), flop),
                         dw=(_timed(lambda: layer.backward_dw(x, m, dout, gw, gb, False, eng.ws)), flop))
            if dx is not None:
                times['dx'] = (_timed(lambda: layer.backward_dx(dout, m, dx, mask=x)), flop)
            row = _row(f'network.{i}.{name}', flop, **times)
            row.update(frames=m, mode=layer.mode, K=layer.K, OC=layer.OC, pixels=layer.H * layer.W, mflop_per_frame=round(flop / m / 1e6, 2))
            for k, (t, _) in times.items():
                total[k] += t
            print(json.dumps(row), flush=True)
        nbytes_f = 4 * m * s.OC * (s.H * s.W + s.PH * s.PW)
        nbytes_b = 4 * m * s.OC * (2 * s.H * s.W + 2 * s.PH * s.PW)
        t_f = _timed(lambda: resnet.maxpool_forward(s.c, m, s.H, s.W, s.OC, s.p))
        t_b = _timed(lambda: resnet.maxpool_backward(s.c, s.p, s.g0, m, s.H, s.W, s.OC, s.gc))
        total['fwd'] += t_f
        total['dx'] += t_b
        print(json.dumps(dict(layer=f'network.{i}.max_pool', frames=m, fwd_us=round(t_f * 1e6, 1), fwd_gb_per_s=round(nbytes_f / t_f / 1e9),
                              bwd_us=round(t_b * 1e6, 1), bwd_gb_per_s=round(nbytes_b / t_b / 1e9))), flush=True)
    fc, last = eng.fc, eng.seqs[-1]
    flop = 2 * m * fc.N * fc.K
    dh = torch.randn(m, fc.N, device='cuda', generator=g)
    gw, gb = torch.empty_like(fc.w), torch.empty_like(fc.b)
    times = dict(fwd=(_timed(lambda: fc.forward(last.x2, m, eng.h)), flop), dx=(_timed(lambda: fc.backward_dx(dh, m, last.x2, last.g0)), flop),
                 dw=(_timed(lambda: fc.backward_dw(last.x2, m, dh, gw, gb, False, eng.ws)), flop))
    for k, (t, _) in times.items():
        total[k] += t
    row = _row('network.5', flop, **times)
    row.update(frames=m, K=fc.K, OC=fc.N, mflop_per_frame=round(flop / m / 1e6, 2))
    print(json.dumps(row), flush=True)
    print(json.dumps(dict(layer='sum', frames=m, fwd_ms=round(total['fwd'] * 1e3, 2), dx_ms=round(total['dx'] * 1e3, 2), dw_ms=round(total['dw'] * 1e3, 2),
                          frames_per_s_forward=round(m / total['fwd']), frames_per_s_forward_backward=round(m / sum(total.values())))), flush=True)


def train(envs):
    import torch
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace, vector
    horizon = 16
    h, w, c = OBS
    vec = vector.make(vector.make_frames, num_envs=envs, backend=vector.Frames,
                      env_kwargs=dict(framestack=c, num_actions=ACTIONS, episode_length=100, height=h, width=w, channels_last=True))
    torch.manual_seed(0)
    pol = cleanrl.Policy(models.ProcgenResnet(vec.driver_env))
    B = envs * horizon
    cfg = namespace(env='frames', seed=1, torch_deterministic=True, device='cuda', total_timesteps=B * 1000, learning_rate=2.5e-4,
                    anneal_lr=True, gamma=0.99, gae_lambda=0.95, update_epochs=1, norm_adv=True, clip_coef=0.1, clip_vloss=True, vf_coef=0.5,
                    vf_clip_coef=0.1, max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=B, minibatch_size=B, bptt_horizon=16,
                    checkpoint_interval=0, data_dir='/tmp/pfa_bench', exp_id='resnet')
    data = clean_pufferl.create(cfg, vec, pol)
    for _ in range(2):
        clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
    torch.cuda.synchronize()
    t0, iters = time.perf_counter(), 4
    for _ in range(iters):
        clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(policy='ProcgenResnet', obs=OBS, envs=envs, horizon=horizon, chunk=data.cnn_engine.chunk, steps_per_s=round(iters * B / dt),
                          finite=bool(torch.isfinite(data.flat_params.flat).all()))), flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'layers'
    arg = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    layers(arg) if what == 'layers' else train(arg)
