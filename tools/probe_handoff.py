"""Where the time of the partial-gradient hand-off goes (developer tool, not product code).

    python tools/probe_handoff.py build [name [path/to/ppo_update.hip]]    (no GPU needed: hipcc cross-compiles)
    python tools/probe_handoff.py run [name ...]                           (on the GPU box)

`build` compiles csrc/ppo_update.hip (or another copy of it, to stamp an older form of the kernels) with -DPFA_PROBES and links it
with the product's other objects into tools/_probe/libhandoff_<name>.so.  In that build thread 0 of every workgroup of
ppo_mlp_grad_kernel's epilogue and of ppo_reduce_adam_kernel stamps the device's 100 MHz wall clock (one clock for all
workgroups and both launches; 10 ns steps) at

    gradient launch   0 last tile done          1 reduction buffers written in LDS    2 partial stored (stores drained)
    reduce launch     0 entry                   1 partial loads landed and summed     2 past the barrier and the slice tree
                      3 norm word published     4 every workgroup's norm word seen    5 exit (Adam's stores drained)

`run` drives pfa_ppo_mlp_train on the bench shape (131 072-row minibatches of 64-float rows, 256 partials), keeps the stamps of the
last optimizer step of one call and prints, per phase, the median and the maximum over the workgroups, the spread of the reduce
launch's entry stamps (its ramp), and the launch-to-launch times.  The product executes no stamp.
"""
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, 'tools', '_probe')
REDUCE_ROW = 512      # kHandoffReduceRow
ROWS = 2048


def build(name='probe', src=None):
    from pufferlib_amd import _lib
    _lib.build()
    os.makedirs(OUT, exist_ok=True)
    src = src or os.path.join(_lib.CSRC, 'ppo_update.hip')
    obj = os.path.join(OUT, f'handoff_{name}.o')
    subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-DPFA_PROBES', '-I', _lib.CSRC, '-x', 'hip',
                           '-c', src, '-o', obj])
    objs = [os.path.join(_lib.LIB_DIR, os.path.splitext(s)[0] + '.o') for s in _lib.SOURCES if s != 'ppo_update.hip'] + [obj]
    so = os.path.join(OUT, f'libhandoff_{name}.so')
    subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-shared', '-fPIC', '-o', so] + objs + ['-ldl'])
    os.remove(obj)
    print(so)


def run(names):
    import numpy as np
    import torch
    from pufferlib_amd import _lib
    N, T, DP, A, NMB = 4096, 128, 64, 8, 4
    B = N * T
    dev = 'cuda'
    res = {}
    for name in names:
        L = C.CDLL(os.path.join(OUT, f'libhandoff_{name}.so'))
        for fn, (restype, argtypes) in _lib._SIGNATURES.items():
            if hasattr(L, fn):
                getattr(L, fn).restype, getattr(L, fn).argtypes = restype, argtypes
        L.pfa_probe_set_handoff.argtypes = [C.c_void_p]
        g = torch.Generator(device=dev).manual_seed(0)
        obs = torch.randn(B, DP, device=dev, generator=g)
        obs[:, 49:] = 0
        bufs = (torch.randint(0, A, (B,), device=dev, dtype=torch.int32, generator=g),
                torch.full((B,), -2.0794, device=dev), torch.randn(B, device=dev, generator=g),
                torch.randn(B, device=dev, generator=g), torch.zeros(B, device=dev),
                torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g))
        exp = _lib.Experience(obs.data_ptr(), *(t.data_ptr() for t in bufs), T)
        dims = _lib.MlpDims(49, DP, 128, A, 0)
        hp = _lib.PpoHparams(.1, .1, .5, .01, 1, 1, NMB, 16)
        P = 128 * DP + 128 + A * 128 + A + 128 + 1
        params = torch.randn(P, device=dev, generator=g) * 0.05
        params[:128 * DP].view(128, DP)[:, 49:] = 0
        m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
        grads = torch.zeros(P + 16, device=dev)
        losses = torch.zeros(8, dtype=torch.float64, device=dev)
        ws = torch.zeros(L.pfa_ppo_workspace_bytes(C.byref(dims), B, C.byref(hp)), dtype=torch.uint8, device=dev)
        stats = torch.tensor([[0.0, float(B // NMB)]] * NMB, dtype=torch.float64, device=dev)
        step = [0]

        def train():
            rc = L.pfa_ppo_mlp_train(C.byref(exp), B, params.data_ptr(), C.byref(dims), C.byref(hp), stats.data_ptr(), grads.data_ptr(),
                                     m.data_ptr(), v.data_ptr(), step[0], 2.5e-4, .9, .999, 1e-5, .5, 4, losses.data_ptr(), ws.data_ptr(), 0, None)
            assert rc == 0, (name, rc, L.pfa_last_error())
            step[0] += 16
        for _ in range(5):
            train()
        torch.cuda.synchronize()
        tr = torch.zeros(ROWS, 8, dtype=torch.int64, device=dev)
        phases = {}
        for rep in range(5):                       # five calls: the phase medians of each, then the median over the calls
            tr.zero_()
            torch.cuda.synchronize()
            assert L.pfa_probe_set_handoff(tr.data_ptr()) == 0
            train()
            torch.cuda.synchronize()
            assert L.pfa_probe_set_handoff(None) == 0
            t = tr.cpu().numpy().astype(np.int64)
            gr = t[:REDUCE_ROW][t[:REDUCE_ROW, 2] > 0]
            rd = t[REDUCE_ROW:][t[REDUCE_ROW:, 5] > 0]
            us = 0.01
            one = {
                'grad_workgroups': len(gr), 'reduce_workgroups': len(rd),
                'grad: last tile -> LDS buffers written': (gr[:, 1] - gr[:, 0]) * us,
                'grad: LDS buffers -> partial stored': (gr[:, 2] - gr[:, 1]) * us,
                'grad: first workgroup past its last tile -> last partial stored': np.array([(gr[:, 2].max() - gr[:, 0].min()) * us]),
                'last partial stored -> first reduce workgroup enters': np.array([(rd[:, 0].min() - gr[:, 2].max()) * us]),
                'reduce: spread of the entry stamps (ramp)': np.array([(rd[:, 0].max() - rd[:, 0].min()) * us]),
                'reduce: entry -> loads landed': (rd[:, 1] - rd[:, 0]) * us,
                'reduce: loads landed -> past barrier + tree': (rd[:, 2] - rd[:, 1]) * us,
                'reduce: tree -> norm word published': (rd[:, 3] - rd[:, 2]) * us,
                'reduce: published -> all norm words seen': (rd[:, 4] - rd[:, 3]) * us,
                'reduce: all seen -> exit (Adam + stores)': (rd[:, 5] - rd[:, 4]) * us,
                'reduce: first entry -> last exit': np.array([(rd[:, 5].max() - rd[:, 0].min()) * us]),
            }
            for k, val in one.items():
                phases.setdefault(k, []).append(val if isinstance(val, int) else (float(np.median(val)), float(np.max(val))))
        table = {}
        print(f'--- {name}: microseconds, median over 5 calls of (median over workgroups, max over workgroups), last optimizer step of a call')
        for k, vals in phases.items():
            if isinstance(vals[0], int):
                table[k] = vals[0]
                print(f'{k:70s} {vals[0]}')
            else:
                med, mx = float(np.median([a for a, _ in vals])), float(np.median([b for _, b in vals]))
                per_call = [round(a, 3) for a, _ in vals]      # the five calls' own medians: their max - min is the phase's run-to-run spread
                table[k] = dict(median_us=round(med, 2), max_us=round(mx, 2), calls_median_us=per_call)
                print(f'{k:70s} median {med:6.2f}   max {mx:6.2f}   calls {min(per_call):.2f} .. {max(per_call):.2f}')
        res[name] = table
    json.dump(res, open(os.path.join(OUT, 'probe_handoff.json'), 'w'), indent=1)


if __name__ == '__main__':
    if sys.argv[1] == 'build':
        build(*sys.argv[2:4])
    else:
        run(sys.argv[2:] or ['probe'])
