"""What tests/test_gpu_dense_gemm.py stands on, checked without a GPU: the bound of tests/dense_gemm_reference.py (4 scaled fp32 chain
errors, no floor) holds for correct products formed another way — the BLAS fp32 product, the emulated six-term bf16 form — and does NOT
hold for the six-term form with any one of its three 2^-16 terms lost, on the very cases the GPU test commits.  The usual max-norm bound
max(4 e32, 1e-5 max |f64|) lets such a kernel pass (docs/lab-notebook.md).  The launch plans are host code, so the kernel each case is
named for is asserted here as well.  The probe cases (one non-zero per row of A, K = 256 .. 3136) get the same three checks on 12
seeds, plus: their gather reference is the chain over all K bit for bit, and every k is some row's non-zero."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_gemm_reference as R

ROWS, WEIGHTS = R.rows_cases(), R.weight_cases()
SPLIT = [c for c in ROWS if c.kernel[0] == 1]
PROBES = R.probe_cases()


def _ids(cases):
    return [pytest.param(c, id=c.tag) for c in cases]


def test_the_case_tables_name_all_twenty_kernels():
    assert {c.kernel for c in ROWS} == {(0, 64, 64), (0, 64, 32), (0, 64, 16), (0, 128, 64), (0, 128, 32), (0, 256, 16), (1, 128, 64), (1, 128, 32)}
    assert {c.kernel for c in WEIGHTS} == {(tn, tk) for tn in (64, 32, 16) for tk in (64, 128, 192, 256)}
    assert {c.K for c in WEIGHTS} == {16, 52, 64, 68, 128, 132, 192, 320, 196, 256} and {c.N for c in WEIGHTS} == {64, 128, 96, 48, 80}
    assert len(SPLIT) == 3 and all(c.K <= 128 and c.K % 32 == 0 for c in SPLIT)


@pytest.mark.parametrize('case', _ids(SPLIT))
def test_the_bound_passes_the_six_term_form_and_fails_it_with_one_term_lost(case):
    ref = R.reference(case).out
    full = ref.scaled_err(case.epilogue(R.bf16x6_rows(case.A, case.B))) / ref.bound
    print(f'[dense gemm cpu] {case.tag:28s} e32s {ref.e32s:.3e}  six terms {full:.3f} of the bound')
    assert full <= 1.0
    for drop in R.DROPPABLE:
        lost = ref.scaled_err(case.epilogue(R.bf16x6_rows(case.A, case.B, drop=drop))) / ref.bound
        print(f'[dense gemm cpu] {case.tag:28s} without {drop[0]}.{drop[1]:3s} {lost:.3f} of the bound')
        assert lost > 1.0, drop


@pytest.mark.parametrize('case', _ids(ROWS))
def test_the_blas_fp32_product_is_inside_the_rows_bound(case):
    ref = R.reference(case).out
    err = ref.scaled_err(case.epilogue(R.blas_rows(case.A, case.B)))
    print(f'[dense gemm cpu] {case.tag:28s} e32s {ref.e32s:.3e}  blas {err / ref.bound:.3f} of the bound')
    assert err <= ref.bound
    if case.epi == R.EPI_MASK:
        off = case.mask <= 0
        assert off.any() and (case.mask[off] == 0).any() and (case.mask[off] < 0).any() and np.signbit(case.mask[case.mask == 0]).any()
        assert not ref.want[off].any()


@pytest.mark.parametrize('case', _ids(WEIGHTS))
def test_the_blas_fp32_product_is_inside_the_weight_bound(case):
    ref = R.reference(case)
    out, col = R.blas_weights(case.A, case.D)
    if case.accumulate:
        out, col = out + case.prefill_out, col + case.prefill_bias
    e_out, e_bias = ref.out.scaled_err(case.layout(out)), ref.bias.scaled_err(col)
    print(f'[dense gemm cpu] {case.tag:28s} out {e_out / ref.out.bound:.3f}  bias {e_bias / ref.bias.bound:.3f} of the bound')
    assert e_out <= ref.out.bound and e_bias <= ref.bias.bound


def test_every_case_lands_on_the_kernel_it_is_named_for():
    """pfa_igemm_rows_plan / pfa_igemm_weights_plan answer from the code the launches choose by (ig_rows_plan, ig_weight_plan), on the
    host: a change of the selection rules that takes a kernel out of the case table fails here."""
    from pufferlib_amd import _lib
    _lib.build()
    L = _lib.lib()
    out = (C.c_int32 * 5)()
    try:
        for c in ROWS:
            _lib.check(L.pfa_igemm_set_products(c.products), 'set_products')
            _lib.check(L.pfa_igemm_rows_plan(0, c.M, c.K, c.N, out), 'rows_plan')
            assert tuple(out[:4]) == c.kernel + (c.tiles,), (c.tag, tuple(out[:4]))
    finally:
        _lib.check(L.pfa_igemm_set_products(0), 'set_products')
    for c in WEIGHTS:
        _lib.check(L.pfa_igemm_weights_plan(c.M, c.K, c.N, out), 'weights_plan')
        tn, tk, tiles, splits, rps = out[:5]
        assert (tn, tk) == c.kernel and tiles == -(-c.K // tk) * (c.N // tn), (c.tag, tuple(out[:5]))
        assert splits == (3 if c.M == 600 else 1) and rps % 16 == 0 and (splits - 1) * rps < c.M <= splits * rps, (c.tag, tuple(out[:5]))
        assert L.pfa_igemm_weights_workspace_bytes(c.M, c.K, c.N) == R.workspace_bytes(splits, c.K, c.N)
    by_tag = {c.tag: c for c in ROWS}
    assert by_tag['128x64-M3970'].tiles == 32 and by_tag['128x64-M4100'].tiles == 33      # a grid of whole eights, and one rounded up to 40


# ------------------------------------------------------------------------------------------------------------------ the probe cases
def test_the_probe_table_covers_the_engines_contraction_lengths():
    assert {(c.kernel, c.K) for c in PROBES} == {(R.BF16_128x64, 256), (R.BF16_128x64, 576), (R.BF16_128x64, 3136), (R.BF16_128x32, 512)}
    assert all(c.products == 1 and c.epi == R.EPI_NONE and c.tiles >= 2 and c.M % c.kernel[1] != 0 for c in PROBES)
    assert not {c.tag for c in PROBES} & {c.tag for c in ROWS}
    for c in PROBES:
        assert sorted(set(c.k)) == list(range(c.K)), 'every k is the one non-zero of some row'
        assert (c.a != 0).all() and (c.B != 0).all()                            # ... and every output has S > 0 (Expected asserts it too)
        for x in (c.a, c.B):                                                    # all three bf16 pieces of both operands are populated
            assert all(bool((piece != 0).float().mean() > 0.9) for piece in R._split3(torch.from_numpy(x)).values())


def test_every_probe_lands_on_the_split_kernel_it_is_named_for():
    from pufferlib_amd import _lib
    _lib.build()
    L = _lib.lib()
    out = (C.c_int32 * 4)()
    try:
        _lib.check(L.pfa_igemm_set_products(1), 'set_products')
        for c in PROBES:
            _lib.check(L.pfa_igemm_rows_plan(0, c.M, c.K, c.N, out), 'rows_plan')
            assert tuple(out) == c.kernel + (c.tiles,) and c.kernel[0] == 1, (c.tag, tuple(out))
    finally:
        _lib.check(L.pfa_igemm_set_products(0), 'set_products')


@pytest.mark.parametrize('case', _ids([c for c in PROBES if c.K <= 576]))
def test_the_gather_reference_is_the_chain_on_the_materialised_operands(case):
    """Bit for bit: the fp32 chain over all K and the emulated six-term form (complete and with each term lost) on the materialised A;
    want and S against the float64 products, to float64 rounding (BLAS adds K - 1 exact zeros in an order of its own)."""
    ref = R.reference(case).out
    a, b = case.gathered()
    chain = R.chain_rows(case.A, case.B)
    assert np.array_equal(chain.view(np.uint32), (a * b).view(np.uint32)) and ref.e32s == ref.scaled_err(chain)
    A64, B64 = case.A.astype(np.float64), case.B.astype(np.float64)
    assert np.array_equal(A64 @ B64.T, ref.want) and np.array_equal(np.abs(A64) @ np.abs(B64).T, ref.S)
    for drop in (None,) + R.DROPPABLE:
        assert np.array_equal(R.bf16x6_rows(case.A, case.B, drop=drop), R.bf16x6_single(a, b, drop=drop)), drop


@pytest.mark.parametrize('case', _ids(PROBES))
def test_the_blas_fp32_product_is_inside_the_probe_bound(case):
    ref = R.reference(case).out
    err = ref.scaled_err(R.blas_rows(case.A, case.B))
    print(f'[dense probe cpu] {case.tag:24s} e32s {ref.e32s:.3e}  blas {err / ref.bound:.3f} of the bound')
    assert err <= ref.bound


@pytest.mark.parametrize('case', _ids(PROBES))
def test_the_probe_bound_passes_the_six_term_form_and_fails_it_with_one_term_lost_on_twelve_seeds(case):
    """From the reference and the emulator alone.  Worst complete form / smallest lost term over the 12 seeds, as multiples of the bound
    (docs/lab-notebook.md): K = 256: 0.45 / 30.3; 576: 0.44 / 31.4; 3136: 0.44 / 30.5; 128 x 32, K = 512: 0.43 / 30.5 (the smallest is
    lo.hi everywhere; hi.lo 32.1, mid.mid 58.6 - 60.0)."""
    worst, least = 0.0, {d: np.inf for d in R.DROPPABLE}
    for seed in range(12):
        c = case if seed == 0 else case.reseeded(case.seed + 100 * seed)
        ref = R.ProbeReference(c).out
        a, b = c.gathered()
        full = ref.scaled_err(R.bf16x6_single(a, b)) / ref.bound
        worst = max(worst, full)
        assert full <= 1.0, (c.tag, full)
        for drop in R.DROPPABLE:
            lost = ref.scaled_err(R.bf16x6_single(a, b, drop=drop)) / ref.bound
            least[drop] = min(least[drop], lost)
            assert lost > 1.0, (c.tag, drop, lost)
    print(f'[dense probe cpu] {case.tag:24s} six terms <= {worst:.3f}  ' + '  '.join(f'without {d[0]}.{d[1]} >= {v:.1f}' for d, v in least.items()))

