"""The chained global round trips of a PPO optimizer step (csrc/ppo_update.hip), issued together: wave 0 of every workgroup of the
reduce + Adam launch requests the norm words of all the workgroups it is responsible for before it looks at any, and the producers of
the gradient launch request their head biases and advantage sums in front of the table build.  Neither may change a bit:

  1. the one-launch step (ppo_reduce_adam_kernel: the grid-wide norm hand-off) against the two-launch form (PFA_FUSED_ADAM=0:
     the same kernel's sums-only form + adam_clip_kernel, no hand-off at all) after two full updates — parameters, both Adam moments and
     the six loss sums with array_equal, a fresh process per value, over every number of polls per lane the shape table can produce (2, 3, 4 and 5:
     step_roundtrips_cases.SHAPES; no shape has <= 64 reduce workgroups, i.e. one poll) and batch sizes with one and with several
     tiles per wavefront pair;
  2. the same with rewards scaled until the oracle's gradient norm is far above max_grad_norm (checked on the CPU before the GPU is
     used), so that the clip factor is not 1 and a wrong norm cannot hide;
  3. on the CPU: the bench instantiation of ppo_mlp_grad_kernel, cross-compiled for gfx950, keeps no scratch and at most 256 VGPRs."""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import step_roundtrips_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _worker(tmp, fused):
    out = os.path.join(str(tmp), f'fused{fused}.npz')
    env = {k: v for k, v in os.environ.items() if not k.startswith('PFA_')}
    env['PFA_FUSED_ADAM'] = fused
    r = subprocess.run([sys.executable, os.path.join(HERE, 'step_roundtrips_cases.py'), '--out', out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return np.load(out)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    # the CPU first: were a 'clipped' case's oracle norm not above max_grad_norm, no worker would be started
    norms = {cid: np.array(cases.oracle_grad_norms(cases.make(cid))) for cid in cases.case_ids() if cid.endswith('-clipped')}
    for cid, n in norms.items():
        assert n.min() > cases.MAX_GRAD_NORM, (cid, n)
    tmp = tmp_path_factory.mktemp('step_roundtrips')
    out = {fused: _worker(tmp, fused) for fused in ('1', '0')}
    out['oracle_norms'] = norms
    return out


def _compare(runs, cid):
    one, two = runs['1'], runs['0']
    for k in ('params', 'exp_avg', 'exp_avg_sq', 'losses'):
        x, y = one[f'{cid}.{k}'], two[f'{cid}.{k}']
        assert np.isfinite(x).all(), (cid, k)
        assert np.array_equal(x, y), (cid, k, int((x != y).sum()))
    assert np.abs(one[f'{cid}.exp_avg']).max() > 0 and np.abs(one[f'{cid}.losses'][:2]).max() > 0
    assert not np.array_equal(one[f'{cid}.params'], cases.make(cid)['flat'])


def test_reduce_grids_of_the_shapes_cover_two_to_five_polls():
    for name, grid in cases.REDUCE_GRID.items():
        assert (cases.native_count(name) + 63) // 64 == grid
    assert sorted((g + 63) // 64 for g in cases.REDUCE_GRID.values()) == [2, 3, 4, 5]


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c for c in cases.case_ids() if c.endswith('-plain')])
def test_one_launch_step_equals_the_two_launch_form_after_two_updates(runs, cid):
    _compare(runs, cid)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c for c in cases.case_ids() if c.endswith('-clipped')])
def test_one_launch_step_equals_the_two_launch_form_with_the_clip_active(runs, cid):
    norms = runs['oracle_norms'][cid]     # per minibatch, at the initial parameters (the fixture checked them before any worker ran)
    print(cid, 'oracle gradient norms', norms)
    assert norms.min() > cases.MAX_GRAD_NORM, norms
    _compare(runs, cid)


BENCH_KERNEL = '_ZN3pfa19ppo_mlp_grad_kernelILi64ELi0ELi13ELb0ELi3ELb1ELb1EEE'   # <64, 0, 13, false, 3, true, true>: the 7x7 grid, <= 11 actions


def test_bench_gradient_kernel_keeps_no_scratch_and_at_most_256_vgprs():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip(f'{hipcc} is not installed')
    src = os.path.join(REPO, 'pufferlib_amd', 'csrc', 'ppo_update.hip')
    budget = 180
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'ppo_update.s')
        t0 = time.time()
        try:
            r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-x', 'hip', '--cuda-device-only', '-S', src, '-o', asm],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=budget)
        except subprocess.TimeoutExpired:
            pytest.skip(f'cross-compiling ppo_update.hip took more than {budget} s on this machine')
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        print(f'compiled in {time.time() - t0:.0f} s')
        text = open(asm).read()
    meta = text[text.index('amdhsa.kernels:'):]
    found = []
    for entry in re.split(r'\n  - \.agpr_count:', meta)[1:]:
        name = re.search(r'\.name:\s+(\S+)', entry).group(1)
        if name.startswith(BENCH_KERNEL):
            found.append((int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', entry).group(1)),
                          int(re.search(r'\.vgpr_count:\s+(\d+)', entry).group(1)),
                          int(re.search(r'\.vgpr_spill_count:\s+(\d+)', entry).group(1))))
    assert len(found) == 1, found
    private, vgprs, spilled = found[0]
    print(f'private segment {private} B, {vgprs} VGPRs, {spilled} spilled')
    assert private == 0 and spilled == 0 and vgprs <= 256
