"""What tests/test_gpu_dense_gemm.py stands on, checked without a GPU: the bound of tests/dense_gemm_reference.py (4 scaled fp32 chain
errors, no floor) holds for correct products formed another way — the BLAS fp32 product, the emulated six-term bf16 form — and does NOT
hold for the six-term form with any one of its three 2^-16 terms lost, on the very cases the GPU test commits.  The usual max-norm bound
max(4 e32, 1e-5 max |f64|) lets such a kernel pass (docs/lab-notebook.md).  The launch plans are host code, so the kernel each case is
named for is asserted here as well."""
import ctypes as C

import numpy as np
import pytest

import dense_gemm_reference as R

ROWS, WEIGHTS = R.rows_cases(), R.weight_cases()
SPLIT = [c for c in ROWS if c.kernel[0] == 1]


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

