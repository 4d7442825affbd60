"""A/B of the weight-gradient contractions (csrc/gemm.hip) in their two product forms, in ONE process on one GPU: the fp32 kernels
(switch off — their text is the parent commit's) and the bf16x6 kernels of csrc/gemm_bf16.hip (switch on), alternating round by round
on the c3 shapes of the recurrent update (131 072 minibatch rows).  Timed: the split-partials launch alone (pfa_gemm_tn*_partial_f32,
what lstm.Engine.update calls; the reduction is the same launch for both forms), device events around `--reps` back-to-back launches.

    python tools/gemm_tn_bench.py --out profiles/gemm_tn_bf16_ab.json [--rounds 5 --reps 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pufferlib_amd                 # noqa: E402
from pufferlib_amd import _lib       # noqa: E402

# (tag, two_operand, mo, no): dW_ih | dW_hh, dW_enc at 160- and 64-float rows, and the 128 x 128 tile (dW_ih alone)
SHAPES = [('tn2_512x256', 1, 512, 256), ('tn_128x160', 0, 128, 160), ('tn_128x64', 0, 128, 64), ('tn_512x128', 0, 512, 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--k', type=int, default=131072)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    L, st, k = _lib.lib(), _lib.stream_handle(), args.k
    g = torch.Generator(device='cuda').manual_seed(7)
    result = {'note': f'one process on one GPU, forms alternating per round; k = {k} rows; us per split-partials launch = device events around '
                      f'{args.reps} back-to-back launches, {args.rounds} rounds; fp32 = the switch off (the parent commit\'s kernels)',
              'device': torch.cuda.get_device_name(0), 'launch_ab': {}}
    for tag, two, mo, no in SHAPES:
        a = torch.randn(k, mo, device='cuda', generator=g)
        b = torch.randn(k, no, device='cuda', generator=g)
        b0, b1 = (b[:, :128].contiguous(), b[:, 128:].contiguous()) if two else (b, None)
        ws = torch.empty(L.pfa_gemm_tn2_workspace_bytes(mo, k) if two else L.pfa_gemm_tn_workspace_bytes(mo, no, k), dtype=torch.uint8, device='cuda')
        job = _lib.ReduceJob()

        def launch():
            if two:
                rc = L.pfa_gemm_tn2_partial_f32(_lib.ptr(a), mo, _lib.ptr(b0), 128, _lib.ptr(b1), 128, mo, k, _lib.ptr(ws), C.byref(job), st)
            else:
                rc = L.pfa_gemm_tn_partial_f32(_lib.ptr(a), mo, _lib.ptr(b0), no, mo, no, k, _lib.ptr(ws), C.byref(job), st)
            _lib.check(rc, tag)
        times = {'fp32': [], 'bf16x6': []}
        info = {}
        for rnd in range(args.rounds + 1):                    # round 0 warms both forms up
            for form in ('fp32', 'bf16x6'):
                pufferlib_amd.set_matrix_products(form)
                info[form] = {'path': L.pfa_gemm_tn_path(mo, no, k, two)}
                launch()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                e1.synchronize()
                info[form]['splits'] = job.splits
                if rnd:
                    times[form].append(round(e0.elapsed_time(e1) * 1e3 / args.reps, 2))
        pufferlib_amd.set_matrix_products('fp32')
        for form in times:
            info[form].update(us=times[form], us_median=statistics.median(times[form]), us_spread=round(max(times[form]) - min(times[form]), 2))
            info[form]['tflops'] = round(2.0 * mo * no * k / info[form]['us_median'] / 1e6, 1)
        result['launch_ab'][tag] = info
        print(tag, {f: (info[f]['us_median'], info[f]['us_spread'], info[f]['path']) for f in info}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
