"""Every kernel the dense operand (mode 0) of pfa_igemm_rows / pfa_igemm_weights can select (csrc/igemm.hip: eight rows-form tiles, twelve
(tn, tile height) weight-form tiles) against float64, one launch per case.  Each case first asserts through pfa_igemm_rows_plan /
pfa_igemm_weights_plan that it runs the kernel it is named for, then compares under the scaled bound of tests/dense_gemm_reference.py:
max |got - f64| / (|A| |B|^T) <= 4 e32s, e32s the sequential fp32 chain's own figure, no absolute floor — a bound that
tests/test_dense_gemm_reference_cpu.py shows to fail a six-term bf16 kernel that loses one term.

Buffers: every leading dimension is wider than its matrix, the padding columns and two extra rows of A and D are NaN, and the outputs
sit inside NaN-filled buffers whose guard elements must still be the same NaN bits afterwards.  pfa_rows_perm (csrc/general.hip), whose
copies feed every product of the recurrent general path, is compared exactly with numpy indexing."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_gemm_reference as R

pytestmark = pytest.mark.gpu

NAN_BITS = np.array([np.nan], np.float32).view(np.uint32)[0]
GUARD = 64


def _ids(cases):
    return [pytest.param(c, id=c.tag) for c in cases]


def _padded(a, ld, extra_rows=0):
    """`a` in the top-left corner of a NaN-filled [rows + extra_rows][ld] device buffer."""
    host = np.full((a.shape[0] + extra_rows, ld), np.nan, np.float32)
    host[:a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(host).cuda()


def _nan(*shape):
    return torch.from_numpy(np.full(shape, np.nan, np.float32)).cuda()


def _untouched(x):
    return bool((np.ascontiguousarray(x).view(np.uint32) == NAN_BITS).all())


def _report(tag, err, exp):
    print(f'[dense gemm f64] {tag:32s} err {err:.3e}  e32s {exp.e32s:.3e}  err/bound {err / exp.bound:.3f}')


@pytest.mark.parametrize('case', _ids(R.rows_cases()))
def test_rows_form_matches_float64(case):
    from pufferlib_amd import _lib
    L = _lib.lib()
    ref = R.reference(case).out
    M, K, N = case.M, case.K, case.N
    lda, ldb, ldc, ldm = K + 4, K + 8, N + 4, N + 8
    A, B = _padded(case.A, lda, 2), _padded(case.B, ldb)
    bias = torch.from_numpy(case.bias).cuda() if case.epi in (R.EPI_BIAS, R.EPI_BIAS_RELU) else None
    mask = _padded(case.mask, ldm) if case.epi == R.EPI_MASK else None
    buf = _nan(M + 2, ldc)                       # one guard row before the output and one after
    plan = (C.c_int32 * 4)()
    try:
        _lib.check(L.pfa_igemm_set_products(case.products), 'set_products')
        _lib.check(L.pfa_igemm_rows_plan(_lib.MODE_DENSE, M, K, N, plan), 'rows_plan')
        assert tuple(plan) == case.kernel + (case.tiles,), f'{case.tag} no longer runs the kernel it is named for: plan {tuple(plan)}'
        _lib.check(L.pfa_igemm_rows(C.byref(_lib.operand(_lib.MODE_DENSE, A, lda)), M, K, _lib.ptr(B), ldb, N, C.c_void_p(buf.data_ptr() + 4 * ldc),
                                    ldc, case.epi, _lib.ptr(bias), _lib.ptr(mask), ldm, _lib.stream_handle()), 'igemm_rows')
        torch.cuda.synchronize()
    finally:
        _lib.check(L.pfa_igemm_set_products(0), 'set_products')
    host = buf.cpu().numpy()
    got = host[1:M + 1, :N]
    assert not np.isnan(got).any(), 'NaN in the output: a padding column or a row past M was read'
    err = ref.scaled_err(got)
    _report(case.tag, err, ref)
    assert _untouched(host[0]) and _untouched(host[M + 1]) and _untouched(host[1:M + 1, N:]), 'written outside the [M][N] output'
    if case.epi == R.EPI_MASK:
        off = case.mask <= 0
        assert not got[off].view(np.uint32).any(), 'mask <= 0 (0.0, -0.0, negative) must give exactly +0.0'
    assert err <= ref.bound, f'{case.tag}: {err:.3e} beyond 4 e32s = {ref.bound:.3e}'


@pytest.mark.parametrize('case', _ids(R.weight_cases()))
def test_weight_form_matches_float64(case):
    from pufferlib_amd import _lib
    L = _lib.lib()
    ref = R.reference(case)
    M, K, N = case.M, case.K, case.N
    lda, ldd = K + 4, N + 4
    A, D = _padded(case.A, lda, 2), _padded(case.D, ldd, 2)
    plan = (C.c_int32 * 5)()
    _lib.check(L.pfa_igemm_weights_plan(M, K, N, plan), 'weights_plan')
    tn, tk, tiles, splits, rps = plan
    assert (tn, tk) == case.kernel, f'{case.tag} no longer runs the kernel it is named for: plan {tuple(plan)}'
    assert tiles == -(-K // tk) * (N // tn) and splits == (3 if M == 600 else 1) and (splits - 1) * rps < M <= splits * rps
    ws_bytes = L.pfa_igemm_weights_workspace_bytes(M, K, N)
    assert ws_bytes == R.workspace_bytes(splits, K, N)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device='cuda')      # NaN patterns: nothing may rely on a cleared workspace
    obuf, bbuf = _nan(K * N + 2 * GUARD), _nan(N + 2 * GUARD)
    if case.accumulate:
        obuf[GUARD:GUARD + K * N] = torch.from_numpy(case.layout(case.prefill_out).reshape(-1)).cuda()
        bbuf[GUARD:GUARD + N] = torch.from_numpy(case.prefill_bias).cuda()
    bias_ptr = C.c_void_p(bbuf.data_ptr() + 4 * GUARD) if case.with_bias else None
    _lib.check(L.pfa_igemm_weights(C.byref(_lib.operand(_lib.MODE_DENSE, A, lda)), M, K, _lib.ptr(D), ldd, N, C.c_void_p(obuf.data_ptr() + 4 * GUARD),
                                   case.perm, case.accumulate, bias_ptr, _lib.ptr(ws), _lib.stream_handle()), 'igemm_weights')
    torch.cuda.synchronize()
    oh, bh = obuf.cpu().numpy(), bbuf.cpu().numpy()
    got = oh[GUARD:GUARD + K * N].reshape(ref.out.want.shape)
    assert not np.isnan(got).any(), 'NaN in out: a padding column or a row past M was read, or an element was not written'
    assert _untouched(oh[:GUARD]) and _untouched(oh[GUARD + K * N:]), 'out holds exactly K N written elements'
    err = ref.out.scaled_err(got)
    _report(case.tag, err, ref.out)
    if case.with_bias:
        gb = bh[GUARD:GUARD + N]
        assert not np.isnan(gb).any() and _untouched(bh[:GUARD]) and _untouched(bh[GUARD + N:])
        eb = ref.bias.scaled_err(gb)
        _report(case.tag + ' bias', eb, ref.bias)
        assert eb <= ref.bias.bound, f'{case.tag} bias_out: {eb:.3e} beyond 4 e32s = {ref.bias.bound:.3e}'
    else:
        assert _untouched(bh)
    assert err <= ref.out.bound, f'{case.tag}: {err:.3e} beyond 4 e32s = {ref.out.bound:.3e}'


def test_refusals_launch_nothing():
    """Arguments the kernels cannot take are refused by the entry points before anything is launched: the NaN-filled outputs stay as
    they are.  The same arguments with the one fault removed are accepted (first, into buffers of their own)."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    M, K, N = 64, 32, 32
    lda = ldb = K + 4
    ldc = ldd = N + 4
    A, B, D = torch.randn(M + 2, lda, device='cuda'), torch.randn(N, ldb, device='cuda'), torch.randn(M, ldd, device='cuda')
    ws = torch.zeros(L.pfa_igemm_weights_workspace_bytes(M, K, N), dtype=torch.uint8, device='cuda')
    stream = _lib.stream_handle()

    def rows(out, a=A, m=M, k=K, n=N, lda=lda, ldb=ldb, ldc=ldc, off=0):
        op = _lib.operand(_lib.MODE_DENSE, a, lda)
        op.ptr += off
        return L.pfa_igemm_rows(C.byref(op), m, k, _lib.ptr(B), ldb, n, _lib.ptr(out), ldc, R.EPI_NONE, None, None, 0, stream)

    def weights(out, op=None, m=M, k=K, n=N):
        op = op or _lib.operand(_lib.MODE_DENSE, A, lda)
        return L.pfa_igemm_weights(C.byref(op), m, k, _lib.ptr(D), ldd, n, _lib.ptr(out), 1, 0, None, _lib.ptr(ws), stream)

    ok_c, ok_g = _nan(M, ldc), _nan(K * N)
    assert rows(ok_c) == 0 and weights(ok_g) == 0
    torch.cuda.synchronize()
    assert not np.isnan(ok_c.cpu().numpy()[:, :N]).any() and not np.isnan(ok_g.cpu().numpy()).any()

    out_c, out_g = _nan(M, ldc), _nan(K * N)
    col2im = _lib.operand(_lib.MODE_COL2IM, A, 0, geom=(4, 4, 4, 4, 4, 4, 1, 1, 1))      # a consistent 1 x 1 layer: only the form is wrong
    refused = [('K % 4 != 0 (rows)', lambda: rows(out_c, k=18), b'multiple of 4'),
               ('K % 4 != 0 (weights)', lambda: weights(out_g, k=18), b'multiple of 4'),
               ('lda < K', lambda: rows(out_c, lda=K - 4), b'lda'),
               ('lda < K (weights)', lambda: weights(out_g, op=_lib.operand(_lib.MODE_DENSE, A, K - 4)), b'lda'),
               ('misaligned A', lambda: rows(out_c, off=4), b'16-byte aligned'),
               ('N % 16 != 0', lambda: rows(out_c, n=24), b'multiple of 16'),
               ('N % 16 != 0 (weights)', lambda: weights(out_g, n=24), b'bad shapes'),
               ('ldc < N', lambda: rows(out_c, ldc=N - 4), b'bad shapes'),
               ('ldb < K', lambda: rows(out_c, ldb=K - 4), b'ldb'),
               ('rows-form K % 16 != 0', lambda: rows(out_c, k=20), b'multiple of 16'),
               ('M lda >= 2^31', lambda: rows(out_c, m=1 << 26, lda=K), b'too large'),
               ('weight form, col2im', lambda: weights(out_g, op=col2im, m=16, k=4), b'rows form')]
    for what, call, message in refused:
        assert call() != 0, what
        assert message in L.pfa_last_error(), (what, L.pfa_last_error())
    torch.cuda.synchronize()
    assert _untouched(out_c.cpu().numpy()) and _untouched(out_g.cpu().numpy())


@pytest.mark.parametrize('cols', [4, 132])
@pytest.mark.parametrize('order', ['row_for_row', 'to_time_major', 'to_segment_major'])
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'act'])
def test_rows_perm_is_numpy_indexing(cols, order, masked):
    """pfa_rows_perm on 5 segments x 3 steps: dst[t * 5 + k] = src[k * 3 + t] and back, row for row with segments = 0; optionally
    dst = act > 0 ? src : 0 with act (0.0, -0.0 and negative entries included) in the SOURCE's row order under a stride of its own.
    Bit-exact; strides wider than cols, the rest of a NaN-filled destination stays NaN."""
    from pufferlib_amd import _lib
    segments, steps = 5, 3
    rows = segments * steps
    lds, ldd, lda = cols + 4, cols + 8, cols + 12
    rs = np.random.RandomState(cols + 7 * masked)
    src = np.full((rows, lds), np.nan, np.float32)
    src[:, :cols] = rs.standard_normal((rows, cols))
    src[1, 0] = -0.0
    act = np.full((rows, lda), np.nan, np.float32)
    flat = rs.standard_normal(rows * cols).astype(np.float32)
    flat[0::5], flat[2::5] = 0.0, -0.0
    act[:, :cols] = flat.reshape(rows, cols)
    act[1, 0] = 1.0                                          # the -0.0 of src is copied as it is
    r = np.arange(rows)
    if order == 'to_time_major':                             # source row k * steps + t -> t * segments + k
        rd = (r % steps) * segments + r // steps
    elif order == 'to_segment_major':                        # source row t * segments + k -> k * steps + t
        rd = (r % segments) * steps + r // segments
    else:
        rd = r
    want = np.full((rows + 2, ldd), np.nan, np.float32)
    want[1 + rd, :cols] = np.where(act[:, :cols] > 0, src[:, :cols], np.float32(0.0)) if masked else src[:, :cols]
    dst = _nan(rows + 2, ldd)
    s, a = torch.from_numpy(src).cuda(), torch.from_numpy(act).cuda()
    _lib.check(_lib.lib().pfa_rows_perm(_lib.ptr(s), lds, C.c_void_p(dst.data_ptr() + 4 * ldd), ldd, _lib.ptr(a) if masked else None,
                                        lda if masked else 0, rows, cols, 0 if order == 'row_for_row' else segments,
                                        0 if order == 'row_for_row' else steps, 1 if order == 'to_time_major' else 0, _lib.stream_handle()),
               'rows_perm')
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert sorted(rd) == list(r) and (order == 'row_for_row' or (rd != r).any())
