"""A/B of the two forms of the heads_rows_* kernels (csrc/general.hip) on one Discrete head of 64 .. 1024 logits:

  wide        one wavefront per row, the row in registers after one coalesced read — what the library dispatches to from
              PFA_WIDE_HEADS_FROM logits on
  per-thread  one thread per row walking its logits from global memory, with only the cap lifted: a SECOND copy of the library whose
              general.hip is compiled with -DPFA_WIDE_HEADS_FROM above the cap (a build-time constant; the library has no run-time switch)

In ONE process, each of the four entry points (sample with the Philox key, eval, eval_backward, loss) at `--rows` rows and every `--actions`
count: `--warmup` launches of each form, then `--repeats` samples per form, the two forms alternating, each sample a pair of device events
around `--inner` back-to-back launches; the table holds the median per launch and the bytes the algorithm moves (one read of `out`
[rows][NO], plus one write of dout [rows][NO] for eval_backward and loss) over it.

    python tools/wide_heads_bench.py --build-per-thread          # where hipcc is (needs no GPU): compile + link the second library
    python tools/wide_heads_bench.py --forms wide per-thread --out wide_heads.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pufferlib_amd import _lib  # noqa: E402

PER_THREAD_LIB = os.path.join(_lib.LIB_DIR, 'libpufferlib_amd_heads_per_thread.so')
ENTRIES = ('sample', 'eval', 'eval_bwd', 'loss')
HBM_ACHIEVABLE = 6.3e12            # bytes/s a float4 copy reaches on an MI355X (8.0e12 on paper)


def build_per_thread():
    """The product library's objects, with general.o replaced by one compiled with the dispatch threshold above the cap."""
    _lib.build()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    obj = os.path.join(_lib.LIB_DIR, 'general_per_thread.o')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-DPFA_WIDE_HEADS_FROM=1025', '-x', 'hip', '-c',
                    os.path.join(_lib.CSRC, 'general.hip'), '-o', obj], check=True)
    objs = [obj if s == 'general.hip' else os.path.join(_lib.LIB_DIR, os.path.splitext(s)[0] + '.o') for s in _lib.SOURCES]
    subprocess.run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', PER_THREAD_LIB] + objs + ['-ldl'], check=True)
    return PER_THREAD_LIB


def load(form):
    if form == 'wide':
        return _lib.lib()
    if not os.path.exists(PER_THREAD_LIB):
        raise SystemExit(f'{PER_THREAD_LIB} is missing: run this tool with --build-per-thread where hipcc is')
    _lib.lib()                       # (torch and the HIP runtime first)
    L = C.CDLL(PER_THREAD_LIB)
    for name in ('pfa_heads_rows_sample', 'pfa_heads_rows_eval', 'pfa_heads_rows_eval_backward', 'pfa_heads_rows_loss',
                 'pfa_heads_rows_loss_workspace_bytes', 'pfa_last_error'):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib._SIGNATURES[name]
    return L


def bytes_moved(entry, rows, NO):
    return rows * NO * 4 * (2 if entry in ('eval_bwd', 'loss') else 1)


def bandit_sps(num_actions=100, n=4096, horizon=128, iters=6, warm=2):
    """Env steps per second of Default(128) on the device Bandit with `num_actions` actions through create / evaluate / train (stepwise
    rollout, noise drawn in place; 2 minibatches x 2 epochs, bptt 8), from the trainer's own profile after `warm` untimed iterations."""
    import time
    import torch
    from pufferlib_amd import clean_pufferl, cleanrl, models, namespace, vector
    vec = vector.make(vector.make_bandit, env_kwargs=dict(num_actions=num_actions), num_envs=n, backend=vector.WideBandit)
    torch.manual_seed(3)
    pol = cleanrl.Policy(models.Default(vec.driver_env, hidden_size=128))
    B = n * horizon
    cfg = namespace(env='bandit', seed=1, torch_deterministic=True, cpu_offload=False, device='cuda', total_timesteps=B * (iters + warm) * 2,
                    learning_rate=2.5e-4, anneal_lr=True, gamma=0.99, gae_lambda=0.95, update_epochs=2, norm_adv=True, clip_coef=0.1,
                    clip_vloss=True, vf_coef=0.5, vf_clip_coef=0.1, max_grad_norm=0.5, ent_coef=0.01, target_kl=None, batch_size=B,
                    minibatch_size=B // 2, bptt_horizon=8, compile=False, checkpoint_interval=0, data_dir='/tmp/pfa_experiments', exp_id='bench')
    data = clean_pufferl.create(cfg, vec, pol)
    for _ in range(warm):
        clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
    torch.cuda.synchronize()
    e0, t0 = data._timers['evaluate'].elapsed, data._timers['train'].elapsed
    steps0, w0 = data.global_step, time.time()
    for _ in range(iters):
        clean_pufferl.evaluate(data)
        clean_pufferl.train(data)
    torch.cuda.synchronize()
    wall = time.time() - w0
    ev, tr = data._timers['evaluate'].elapsed - e0, data._timers['train'].elapsed - t0
    steps = data.global_step - steps0
    res = dict(num_actions=num_actions, envs=n, horizon=horizon, iterations=iters, steps=steps, wall_s=wall, evaluate_s=ev, train_s=tr,
               steps_per_s=steps / wall, steps_per_s_profile=steps / (ev + tr))
    print(f'bandit A={num_actions} {n} envs x {horizon} steps: {steps / (ev + tr):,.0f} env steps/s over evaluate {ev / iters * 1e3:.1f} ms + train '
          f'{tr / iters * 1e3:.1f} ms per iteration ({steps / wall:,.0f} over the wall clock)', flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bandit-sps', action='store_true', help='also time Default(128) on vector.WideBandit(num_actions=100), 4096 envs x 128 steps')
    ap.add_argument('--build-per-thread', action='store_true', help='compile and link the per-thread copy of the library, then exit')
    ap.add_argument('--forms', nargs='+', default=['wide'], choices=['wide', 'per-thread'])
    ap.add_argument('--rows', type=int, default=131072)
    ap.add_argument('--actions', type=int, nargs='+', default=[64, 128, 256, 1024])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--inner', type=int, default=4)
    ap.add_argument('--out', default=None, help='also write the results as JSON here')
    args = ap.parse_args()
    if args.build_per_thread:
        print(build_per_thread())
        return
    import torch
    _lib.require_gpu()
    libs = {form: load(form) for form in args.forms}
    rows, dev = args.rows, 'cuda'
    g = torch.Generator().manual_seed(1)
    results = []
    for A in args.actions:
        NO = _lib.round_up(A + 1, 16)
        out = torch.zeros(rows, NO, device=dev)
        out[:, :A + 1] = (torch.randn(rows, A + 1, generator=g) * 2).to(dev)
        acts = torch.randint(0, A, (rows,), generator=g)
        actions64 = acts.to(dev)
        sampled = torch.empty(rows, dtype=torch.int64, device=dev)
        lp, ent, val, g_lp, g_ent, g_val = (torch.randn(rows, device=dev) for _ in range(6))
        dout = torch.empty(rows, NO, device=dev)
        bufs = dict(actions=acts.to(torch.int32).to(dev), logprobs=torch.full((rows,), -float(torch.log(torch.tensor(float(A)))), device=dev),
                    values=torch.randn(rows, device=dev), rewards=torch.zeros(rows, device=dev), dones=torch.zeros(rows, device=dev),
                    advantages=torch.randn(rows, device=dev), returns=torch.randn(rows, device=dev))
        obs = torch.zeros(16, device=dev)
        exp = _lib.Experience(obs.data_ptr(), bufs['actions'].data_ptr(), bufs['logprobs'].data_ptr(), bufs['values'].data_ptr(),
                              bufs['rewards'].data_ptr(), bufs['dones'].data_ptr(), bufs['advantages'].data_ptr(), bufs['returns'].data_ptr(), 16)
        hp = _lib.PpoHparams(0.1, 0.1, 0.5, 0.01, 1, 1, 1, 16)
        adv = bufs['advantages'].double()
        stats = torch.stack([adv.sum(), (adv * adv).sum()]).view(1, 2).contiguous()
        pairs = torch.zeros(16, device=dev)
        ws = torch.empty(_lib.lib().pfa_heads_rows_loss_workspace_bytes(rows), dtype=torch.uint8, device=dev)
        key = _lib.NoiseKey(1, 0)
        p = _lib.ptr

        def launch(L, entry):
            if entry == 'sample':
                rc = L.pfa_heads_rows_sample(p(out), NO, rows, A, 0, None, C.byref(key), 0, p(sampled), p(lp), p(ent), p(val), None)
            elif entry == 'eval':
                rc = L.pfa_heads_rows_eval(p(out), NO, rows, A, 0, p(actions64), p(lp), p(ent), p(val), None)
            elif entry == 'eval_bwd':
                rc = L.pfa_heads_rows_eval_backward(p(out), NO, rows, A, 0, p(actions64), p(g_lp), p(g_ent), p(g_val), p(dout), NO, NO, None)
            else:
                rc = L.pfa_heads_rows_loss(p(out), NO, C.byref(exp), rows, 0, 0, rows, 0, A, 0, C.byref(hp), p(stats), rows, p(dout), NO, NO,
                                           p(pairs), 0, p(ws), None)
            if rc != 0:
                raise SystemExit(f'{entry}: {L.pfa_last_error().decode()}')

        for entry in ENTRIES:
            for form, L in libs.items():
                for _ in range(args.warmup):
                    launch(L, entry)
            torch.cuda.synchronize()
            samples = {form: [] for form in libs}
            for _ in range(args.repeats):
                for form, L in libs.items():                     # the forms alternate: what shares the machine hits both alike
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.inner):
                        launch(L, entry)
                    t1.record()
                    t1.synchronize()
                    samples[form].append(t0.elapsed_time(t1) * 1e-3 / args.inner)
            for form, s in samples.items():
                med = statistics.median(s)
                rate = bytes_moved(entry, rows, NO) / med
                results.append(dict(entry=entry, form=form, actions=A, rows=rows, median_us=med * 1e6, min_us=min(s) * 1e6, max_us=max(s) * 1e6,
                                    bytes=bytes_moved(entry, rows, NO), bytes_per_s=rate, share_of_achievable_hbm=rate / HBM_ACHIEVABLE))
                print(f'{entry:<9} A={A:<5} {form:<10} median {med * 1e6:9.1f} us  (min {min(s) * 1e6:9.1f}, max {max(s) * 1e6:9.1f})  '
                      f'{rate / 1e12:6.3f} TB/s  {100 * rate / HBM_ACHIEVABLE:5.1f} % of 6.3 TB/s', flush=True)
        del out, dout
        torch.cuda.empty_cache()
    sps = bandit_sps() if args.bandit_sps else None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(dict(rows=rows, warmup=args.warmup, repeats=args.repeats, inner=args.inner, results=results, bandit=sps), f, indent=1)


if __name__ == '__main__':
    main()
