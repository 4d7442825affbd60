"""Every kernel the conv operand modes (1 - 6) of pfa_igemm_rows / pfa_igemm_rows_add / pfa_igemm_weights can select (csrc/igemm.hip: 18 fp32
and 8 six-term rows-form kernels, the weight form at every tile height a mode's K reaches, the reduce kernel's conv layouts) against
float64, one launch per case.  The operand of a case is materialised on the CPU by plain indexing (tests/conv_gemm_reference.py, which
tests/test_conv_gemm_reference_cpu.py shows to be torch's convolution and its gradients) and compared under the row-scaled bound of
tests/dense_gemm_reference.py: max |got - f64| / (|A| |B|^T) <= 4 e32s, no absolute floor.  Each case first asserts through the plan
queries that it runs the kernel it is named for.

Buffers: float inputs sit between NaN guard frames and byte inputs between guard frames of 255, and every input element the case does
not read (the rest of a frame M ends in, pixels no window reaches, stride gaps) is NaN / 255 as well; B, mask, addend and D have NaN
padding columns (B of mode 6: true zeros in columns KH KW IC .. K-1, NaN beyond K); outputs sit in NaN-filled buffers whose guards must
keep their NaN bits.  Elements whose scale S is 0 — col2im pixels no window covers, outputs under mask <= 0 — must be +0.0 by bits, and
EPI_MASK_ADD under mask <= 0 must return the addend's bits.  The four pack kernels are compared bit for bit with the numpy layouts."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_gemm_reference as R
from dense_gemm_reference import workspace_bytes

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


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _report(tag, err, exp):
    print(f'[conv gemm f64] {tag:32s} err {err:.3e}  e32s {exp.e32s:.3e}  err/bound {err / exp.bound:.3f}')


def _guarded_input(case):
    """The raw input with everything the case does not read poisoned, between one guard frame before and one after (NaN / 255); the
    view that starts at the first real frame (16-byte aligned: guard frames are rounded up to 16 bytes)."""
    raw = case.raw_guarded
    unit = 16 // raw.dtype.itemsize
    g = -(-case.per_frame // unit) * unit
    fill = np.uint8(255) if raw.dtype == np.uint8 else np.float32(np.nan)
    host = np.full(g + raw.size + g + unit, fill, raw.dtype)
    host[g:g + raw.size] = raw.reshape(-1)
    dev = torch.from_numpy(host).cuda()
    return dev, dev[g:]


@pytest.mark.parametrize('case', _ids(R.rows_cases()))
def test_rows_form_matches_float64(case):
    from pufferlib_amd import _lib
    L = _lib.lib()
    ref = R.reference(case).out
    M, K, N, P = case.M, case.K, case.N, case.phases
    ldb, ldc, ldm, lda = K + 4, N + 4, N + 8, N + 12
    keep, x = _guarded_input(case)
    B = _padded(case.B.reshape(P * N, K), ldb)
    bias = torch.from_numpy(case.bias).cuda() if case.epi in R.WITH_BIAS else None
    mask = _padded(case.mask, ldm) if case.epi in R.WITH_MASK else None
    addend = _padded(case.addend, lda) if case.epi in R.WITH_ADDEND else None
    buf = _nan(M + 2, ldc)                       # one guard row before the output and one after
    out = C.c_void_p(buf.data_ptr() + 4 * ldc)
    a = _lib.operand(case.mode, x, 0, geom=case.op.geom, strides=case.strides, relu_in=case.relu_in)
    plan = (C.c_int32 * 4)()
    try:
        _lib.check(L.pfa_igemm_set_products(case.products), 'set_products')
        _lib.check(L.pfa_igemm_rows_plan(case.mode, case.M_plan, K, N, plan), 'rows_plan')
        assert tuple(plan) == case.kernel + (case.tiles,), f'{case.tag} no longer runs the kernel it is named for: plan {tuple(plan)}'
        if case.mode in (R.IM2COL_PAD, R.IM2COL_U8P):
            _lib.check(L.pfa_igemm_rows_add(C.byref(a), M, case.K_call, _lib.ptr(B), ldb, N, out, ldc, case.epi, _lib.ptr(bias), _lib.ptr(mask),
                                            ldm if mask is not None else 0, _lib.ptr(addend), lda if addend is not None else 0, _lib.stream_handle()),
                       'igemm_rows_add')
        else:
            _lib.check(L.pfa_igemm_rows(C.byref(a), M, case.K_call, _lib.ptr(B), ldb, N, out, ldc, case.epi, _lib.ptr(bias), _lib.ptr(mask),
                                        ldm if mask is not None else 0, _lib.stream_handle()), 'igemm_rows')
        torch.cuda.synchronize()
    finally:
        _lib.check(L.pfa_igemm_set_products(0), 'set_products')
    host = buf.cpu().numpy()
    got = host[1:M + 1, :N]
    assert not np.isnan(got).any(), 'NaN in the output: an element outside the operand was read, or a row (col2im: a pixel) was not written'
    err = ref.scaled_err(got)
    _report(case.tag, err, ref)
    assert _untouched(host[0]) and _untouched(host[M + 1]) and _untouched(host[1:M + 1, N:]), 'written outside the [M][N] output'
    assert ref.dead_are_plus_zero(got), 'an output without any contribution (uncovered pixel, mask <= 0) must be exactly +0.0'
    if case.epi == R.EPI_MASK_ADD:
        off = case.mask <= 0
        assert np.array_equal(_bits(got[off]), _bits(case.addend[off])), 'mask <= 0: the addend bit for bit'
    assert err <= ref.bound, f'{case.tag}: {err:.3e} beyond 4 e32s = {ref.bound:.3e}'


@pytest.mark.parametrize('case', _ids(R.weight_cases()))
def test_weight_form_matches_float64(case):
    from pufferlib_amd import _lib
    L = _lib.lib()
    ref = R.reference(case)
    M, K, N = case.M, case.K, case.N
    ldd = N + 4
    D = _padded(case.D, ldd, 2)
    if case.mode == R.DENSE:
        lda = K + 4
        keep = x = _padded(case.A, lda, 2)
        a = _lib.operand(case.mode, x, lda, geom=case.layer.geom[:3] + (0,) * 6)
    else:
        keep, x = _guarded_input(case)
        a = _lib.operand(case.mode, x, 0, geom=case.layer.geom, strides=case.strides, relu_in=case.relu_in)
    plan = (C.c_int32 * 5)()
    if K % 4 == 0:
        _lib.check(L.pfa_igemm_weights_plan(M, K, N, plan), 'weights_plan')
        assert tuple(plan[:2]) == case.kernel and tuple(plan[3:]) == (case.splits, case.rows_per_split), f'{case.tag}: plan {tuple(plan)}'
    ws_bytes = L.pfa_igemm_weights_workspace_bytes(M, K, N)
    assert ws_bytes == workspace_bytes(case.splits, K, N)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device='cuda')      # NaN patterns: nothing may rely on a cleared workspace
    obuf, bbuf = _nan(K * N + 2 * GUARD), _nan(N + 2 * GUARD)
    if case.accumulate:
        obuf[GUARD:GUARD + K * N] = torch.from_numpy(case.layout(case.prefill_out)).cuda()
        bbuf[GUARD:GUARD + N] = torch.from_numpy(case.prefill_bias).cuda()
    bias_ptr = C.c_void_p(bbuf.data_ptr() + 4 * GUARD) if case.with_bias else None
    _lib.check(L.pfa_igemm_weights(C.byref(a), M, K, _lib.ptr(D), ldd, N, C.c_void_p(obuf.data_ptr() + 4 * GUARD), case.perm, case.accumulate,
                                   bias_ptr, _lib.ptr(ws), _lib.stream_handle()), 'igemm_weights')
    torch.cuda.synchronize()
    oh, bh = obuf.cpu().numpy(), bbuf.cpu().numpy()
    got = oh[GUARD:GUARD + K * N]
    assert not np.isnan(got).any(), 'NaN in out: an element outside the operand or a row past M was read, or an element was not written'
    assert _untouched(oh[:GUARD]) and _untouched(oh[GUARD + K * N:]), 'out holds exactly K N written elements'
    err = ref.out.scaled_err(got)
    _report(case.tag, err, ref.out)
    assert ref.out.dead_are_plus_zero(got), 'a weight whose taps are all padding has a gradient of exactly +0.0'
    if case.with_bias:
        gb = bh[GUARD:GUARD + N]
        assert not np.isnan(gb).any() and _untouched(bh[:GUARD]) and _untouched(bh[GUARD + N:])
        eb = ref.bias.scaled_err(gb)
        _report(case.tag + ' bias', eb, ref.bias)
        assert eb <= ref.bias.bound, f'{case.tag} bias_out: {eb:.3e} beyond 4 e32s = {ref.bias.bound:.3e}'
    else:
        assert _untouched(bh)
    assert err <= ref.out.bound, f'{case.tag}: {err:.3e} beyond 4 e32s = {ref.out.bound:.3e}'


def _weights(rs, oc, ic, kh, kw):
    w = rs.standard_normal((oc, ic, kh, kw)).astype(np.float32)
    w.reshape(-1)[1] = -0.0
    return w


def _run_pack(call, w, shapes):
    """Launch a pack kernel on NaN-filled outputs of the given sizes; -> the host copies."""
    from pufferlib_amd import _lib
    wd = torch.from_numpy(w).cuda()
    outs = [_nan(n + 2 * GUARD) for n in shapes]
    _lib.check(call(_lib.ptr(wd), *[C.c_void_p(o.data_ptr() + 4 * GUARD) for o in outs]), 'pack')
    torch.cuda.synchronize()
    hosts = [o.cpu().numpy() for o in outs]
    for h, n in zip(hosts, shapes):
        assert _untouched(h[:GUARD]) and _untouched(h[GUARD + n:]), 'written outside the packed matrix'
    return [h[GUARD:GUARD + n] for h, n in zip(hosts, shapes)]


@pytest.mark.parametrize('u8_order', [0, 1, 2])
@pytest.mark.parametrize('shape', [(5, 3, 4, 6, 2), (3, 4, 3, 6, 3), (4, 2, 3, 2, 1)], ids=['S2', 'S3', 'S1'])
def test_pack_conv_is_numpy_indexing(shape, u8_order):
    """pfa_cnn_pack_conv: forward [OC][k] in the loader's order (u8_order 1: torch's own order, 2: mode 4's; both / 255 as ONE fp32
    division) and the phase-major dX form with all S S phases, bit for bit."""
    from pufferlib_amd import _lib
    oc, ic, kh, kw, s = shape
    w = _weights(np.random.RandomState(31 + u8_order), oc, ic, kh, kw)
    Lr = R.Layer(ic, kh + 2 * s, kw + s, oc, kh, kw, S=s)
    geom = _lib.operand(0, torch.zeros(1), 0, geom=Lr.geom)
    fwd, dx = _run_pack(lambda wp, f, d: _lib.lib().pfa_cnn_pack_conv(wp, C.byref(geom), u8_order, f, d, _lib.stream_handle()), w, [w.size, w.size])
    want = R.fwd_layout(w, 'ckk' if u8_order == 1 else 'kkc', div=u8_order != 0)
    assert want.dtype == np.float32 and np.array_equal(_bits(fwd), _bits(want.reshape(-1)))
    want_dx = R.dx_phase_layout(w, s)
    assert want_dx.shape[0] == s * s and np.array_equal(_bits(dx), _bits(want_dx.reshape(-1)))


@pytest.mark.parametrize('u8', [0, 1])
@pytest.mark.parametrize('shape', [(5, 3, 3), (4, 8, 5), (3, 1, 1)], ids=['3x3', '5x5', '1x1'])
def test_pack_conv_same_is_numpy_indexing(shape, u8):
    """pfa_cnn_pack_conv_same with ldf > K: the padding columns keep what they held (NaN here); the dX form is the kernel flipped in both
    axes with the channel roles swapped."""
    from pufferlib_amd import _lib
    oc, ic, k = shape
    w = _weights(np.random.RandomState(41 + u8), oc, ic, k, k)
    K = ic * k * k
    ldf = -(-K // 16) * 16 + 16
    geom = _lib.operand(0, torch.zeros(1), 0, geom=R.Layer(ic, 4, 5, oc, k, k, same=True).geom)
    fwd, dx = _run_pack(lambda wp, f, d: _lib.lib().pfa_cnn_pack_conv_same(wp, C.byref(geom), u8, f, ldf, d, _lib.stream_handle()), w,
                        [oc * ldf, w.size])
    fwd = fwd.reshape(oc, ldf)
    assert np.array_equal(_bits(fwd[:, :K]), _bits(R.fwd_layout(w, 'kkc', div=bool(u8)))) and _untouched(fwd[:, K:])
    assert np.array_equal(_bits(dx), _bits(R.dx_flipped_layout(w).reshape(-1)))


def test_pack_fc_and_transpose_are_numpy_indexing():
    from pufferlib_amd import _lib
    n, c, hw = 7, 5, 6
    w = np.random.RandomState(51).standard_normal((n, c * hw)).astype(np.float32)
    perm, t = _run_pack(lambda wp, p, q: _lib.lib().pfa_cnn_pack_fc(wp, n, c, hw, p, q, _lib.stream_handle()), w, [w.size, w.size])
    want_p, want_t = R.fc_layouts(w, c, hw)
    assert np.array_equal(_bits(perm), _bits(want_p.reshape(-1))) and np.array_equal(_bits(t), _bits(want_t.reshape(-1)))
    assert not np.array_equal(want_p, w)
    (tr,) = _run_pack(lambda wp, o: _lib.lib().pfa_cnn_transpose(wp, n, c * hw, o, _lib.stream_handle()), w, [w.size])
    assert np.array_equal(_bits(tr), _bits(np.ascontiguousarray(w.T).reshape(-1)))
