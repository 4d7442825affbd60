"""First-layer loader timing and end-to-end env steps/s of models.Convolutional at every frame geometry (developer tool, not product
code; modelled on tools/igemm_bench.py).

    python tools/conv_geometry_bench.py layers [frames]      conv1 forward and conv1 dW per geometry (default 4096 frames): time and the
                                                             fraction of the fp32-MFMA peak, the aligned loader (mode 2, `atari`) next to
                                                             the strided one (mode 4, everything else)
    python tools/conv_geometry_bench.py train [envs] [tags]  create / evaluate / train on vector.Frames at the geometry's frame shape with
                                                             the c4 hyper-parameters: env steps/s (env parity unpinned, synthetic frames)
    python tools/conv_geometry_bench.py train_pixel [envs] [tags]  the same on vector.PixelSquared (Squared painted at the geometry's
                                                             frame shape; geometries of more than four channels are skipped)

Launches go through the C-ABI entry points the engine uses, timed with HIP events on their stream (median of 5 after 2 warm-ups).
TFLOP/s = algorithmic flop (2 m n k) / time; the peak it is held against is 157.3 TFLOP/s (256 CUs x 256 flop / clock x 2.4 GHz)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
PEAK_TFLOPS = 157.3


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


def layers(n):
    import torch
    import conv_geometry as cg
    from pufferlib_amd import cnn, models
    rows = []
    for tag, geo in cg.GEOMETRIES.items():
        net = models.Convolutional(cg.Env(tag, 4), **geo['kwargs'])
        cp = models.ConvParams(net, 'cuda')
        eng = cnn.Engine(cp, chunk=n)
        m = min(n, eng.chunk)
        eng.pack()
        g = torch.Generator(device='cuda').manual_seed(1)
        frames = torch.randint(0, 256, (m, eng.frame_bytes), dtype=torch.uint8, device='cuda', generator=g)
        c1 = eng.conv1
        d1 = torch.randn(c1.out_rows(m), 32, device='cuda', generator=g)
        gw, gb = torch.empty_like(c1.w), torch.empty_like(c1.b)
        flop = 2 * c1.out_rows(m) * 32 * c1.K
        t_f = _timed(lambda: c1.forward(frames, m, eng.a1))
        t_w = _timed(lambda: c1.backward_dw(frames, m, d1, gw, gb, False, eng.ws))
        row = dict(tag=tag, frames=m, mode=c1.in_mode, word_loads=bool(c1.in_mode == 2 or (c1.IC == 4 and eng.geometry.sc == 1)), K=c1.K,
                   out_pixels=c1.OH * c1.OW, fwd_us=round(t_f * 1e6, 1), fwd_tflops=round(flop / t_f / 1e12, 2),
                   fwd_peak_fraction=round(flop / t_f / 1e12 / PEAK_TFLOPS, 3), dw_us=round(t_w * 1e6, 1), dw_tflops=round(flop / t_w / 1e12, 2),
                   dw_peak_fraction=round(flop / t_w / 1e12 / PEAK_TFLOPS, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del eng, cp, net, frames, d1
        torch.cuda.empty_cache()
    return rows


def train(envs, tags, pixel=False):
    import torch
    import conv_geometry as cg
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace, vector
    horizon = 16
    for tag in tags:
        geo = cg.GEOMETRIES[tag]
        last = geo['kwargs'].get('channels_last', False)
        (h, w, c) = geo['obs'] if last else (geo['obs'][1], geo['obs'][2], geo['obs'][0])
        if pixel and c > vector.PixelSquaredSpec.MAX_CHANNELS:
            print(json.dumps(dict(tag=tag, skipped=f'{c} channels')), flush=True)
            continue
        if pixel:
            vec = vector.make(vector.make_pixel_squared, num_envs=envs, backend=vector.PixelSquared,
                              env_kwargs=dict(height=h, width=w, channels=c, channels_last=last))
        else:
            vec = vector.make(vector.make_frames, num_envs=envs, backend=vector.Frames,
                              env_kwargs=dict(framestack=c, num_actions=4, episode_length=100, height=h, width=w, channels_last=last))
        torch.manual_seed(0)
        pol = cleanrl.Policy(models.Convolutional(vec.driver_env, **geo['kwargs']))
        B = envs * horizon
        cfg = namespace(env='pixel_squared' if pixel else 'frames', seed=1, torch_deterministic=True, device='cuda', total_timesteps=B * 1000, learning_rate=2.5e-4,
                        anneal_lr=True, gamma=0.99, gae_lambda=0.95, update_epochs=1, norm_adv=True, clip_coef=0.1, clip_vloss=True, vf_coef=0.5,
                        vf_clip_coef=0.1, max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=B, minibatch_size=B, bptt_horizon=16,
                        checkpoint_interval=0, data_dir='/tmp/pfa_bench', exp_id='geom')
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
        print(json.dumps(dict(tag=tag, env=type(vec).__name__, envs=envs, horizon=horizon, chunk=data.cnn_engine.chunk, steps_per_s=round(iters * B / dt),
                              finite=bool(torch.isfinite(data.flat_params.flat).all()))), flush=True)
        del data, pol, vec
        torch.cuda.empty_cache()


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'layers'
    if what == 'layers':
        layers(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    else:
        import conv_geometry
        train(int(sys.argv[2]) if len(sys.argv) > 2 else 4096, sys.argv[3:] or list(conv_geometry.GEOMETRIES), pixel=what == 'train_pixel')
