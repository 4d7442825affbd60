"""What tests/test_gpu_conv_gemm.py stands on, checked without a GPU.
* The restated gather IS a convolution: for every forward case A64 B64^T equals torch's float64 conv2d on the torch-layout weights, every
  dX case float64 autograd's input gradient, every weight case its weight and bias gradient, to float64 rounding.
* The bound (4 scaled fp32 chain errors, no floor) holds for the BLAS fp32 product of the materialised operands and for the emulated
  six-term form, and does NOT hold for the six-term form with one droppable term lost (float operands: lo.hi, hi.lo, mid.mid; byte
  operands, three terms: hi.lo) — on the committed cases, whose per-phase contraction is 32 or 64.  Minimum over 12 seeds of the lost-term
  figure as a multiple of the bound: im2col f32 K = 32 / 64 / 96: 2.5 / 1.9 / 1.2; col2im per-phase K = 64: 2.1; bytes K = 32 / 64: 2.8 /
  1.6; at K = 192 / 288 it is 0.8 - 1.5 (e32s grows with K faster than the lost term), which is why longer contractions belong to the fp32
  cases only.
* The tables contain the kernels and edges they claim, and the launch plans (host code) put every case on the kernel it is named for."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_gemm_reference as R
import dense_gemm_reference as D

ROWS, WEIGHTS = R.rows_cases(), R.weight_cases()
SPLIT = [c for c in ROWS if c.kernel[0] == 1]
FORWARD, DX = [c for c in ROWS if c.kind == 'fwd'], [c for c in ROWS if c.kind == 'dx']
F64 = np.float64


def _ids(cases):
    return [pytest.param(c, id=c.tag) for c in cases]


def _close(got, want, S):
    assert got.shape == want.shape
    assert (np.abs(got - want) <= 1e-12 * S).all(), float((np.abs(got - want) / np.where(S > 0, S, 1)).max())


def _conv(case, W64):
    L = case.op
    return F.conv2d(torch.from_numpy(case.image64()), torch.from_numpy(W64), stride=L.S, padding=L.pad)


@pytest.mark.parametrize('case', _ids(FORWARD))
def test_the_forward_gather_is_conv2d(case):
    """bytes / 255 and the weights as torch holds them against the raw operand and B = the layout of the same weights / 255, in float64."""
    W64 = case.W.astype(F64)
    A64, B64 = case.A.astype(F64), case.make_B(W64)[0]
    want = _conv(case, W64).permute(0, 2, 3, 1).reshape(-1, case.N).numpy()[:case.M]
    _close(A64 @ B64.T, want, np.abs(A64) @ np.abs(B64).T)
    assert np.array_equal(case.B[0], case.make_B(case.W)[0]) and (case.B[0][:, case.K_true:] == 0).all()


@pytest.mark.parametrize('case', _ids(DX))
def test_the_dx_gather_is_autograd(case):
    L = case.layer
    W64 = case.W.astype(F64)
    x0 = torch.zeros(case.frames, L.IC, L.IH, L.IW, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(x0, torch.from_numpy(W64), stride=L.S, padding=L.pad)
    dout = torch.from_numpy(case.image64())
    assert dout.shape == out.shape
    want = torch.autograd.grad(out, x0, dout)[0].permute(0, 2, 3, 1).reshape(-1, case.N).numpy()[:case.M]
    A64, B64 = case.A.astype(F64), case.make_B(W64)
    _close(case.product(lambda a, b: a @ b.T, A64, B64, F64), want, case.product(lambda a, b: a @ b.T, np.abs(A64), np.abs(B64), F64))


@pytest.mark.parametrize('case', _ids(WEIGHTS))
def test_the_weight_gather_is_autograd(case):
    L, M, N = case.layer, case.M, case.N
    A64, D64 = case.A.astype(F64), case.D.astype(F64)
    got = case.layout(A64.T @ D64) / case.scale
    S = case.layout(np.abs(A64).T @ np.abs(D64)) / case.scale
    rows = np.zeros((case.frames * case.rows_per_frame, N))
    rows[:M] = D64
    if case.mode == R.DENSE:                 # Linear behind nn.Flatten of the NCHW form of the NHWC rows
        x = torch.from_numpy(A64.reshape(M, L.IH, L.IW, L.IC)).permute(0, 3, 1, 2).reshape(M, -1)
        W0 = torch.zeros(N, case.K, dtype=torch.float64, requires_grad=True)
        gw = torch.autograd.grad(x @ W0.T, W0, torch.from_numpy(D64))[0]
    else:
        W0 = torch.zeros(L.OC, L.IC, L.KH, L.KW, dtype=torch.float64, requires_grad=True)
        out = F.conv2d(torch.from_numpy(case.image64()), W0, stride=L.S, padding=L.pad)
        dout = torch.from_numpy(rows).reshape(case.frames, L.OH, L.OW, N).permute(0, 3, 1, 2)
        gw = torch.autograd.grad(out, W0, dout)[0]
    _close(got, gw.numpy().reshape(-1), S)
    ref = R.reference(case)
    _close(ref.bias.want if not case.accumulate else ref.bias.want - case.prefill_bias.astype(F64), D64.sum(0), np.abs(D64).sum(0))


@pytest.mark.parametrize('case', _ids(ROWS))
def test_the_blas_fp32_product_is_inside_the_rows_bound(case):
    ref = R.reference(case).out
    got = case.epilogue(case.product(D.blas_rows, case.A, case.B, np.float32))
    err = ref.scaled_err(got)
    print(f'[conv gemm cpu] {case.tag:28s} e32s {ref.e32s:.3e}  blas {err / ref.bound:.3f} of the bound')
    assert err <= ref.bound and ref.dead_are_plus_zero(got)
    if case.epi in R.WITH_MASK:
        off = case.mask <= 0
        assert (case.mask[off] == 0).any() and (case.mask[off] < 0).any() and np.signbit(case.mask[case.mask == 0]).any()
        if case.epi == R.EPI_MASK:
            assert not ref.live[off].any()
        else:
            assert np.array_equal(ref.want[off], case.addend[off].astype(F64))
            assert np.array_equal(got[off].view(np.uint32), case.addend[off].view(np.uint32))


@pytest.mark.parametrize('case', _ids(WEIGHTS))
def test_the_blas_fp32_product_is_inside_the_weight_bound(case):
    ref = R.reference(case)
    out, col = D.blas_weights(case.A, case.D)
    if case.accumulate:
        out, col = out + case.prefill_out, col + case.prefill_bias
    out = case.layout(out)
    if case.scale != 1.0:
        out = (out.astype(F64) / case.scale).astype(np.float32)       # the reduce kernel divides the float64 sum once
    e_out, e_bias = ref.out.scaled_err(out), ref.bias.scaled_err(col)
    print(f'[conv gemm cpu] {case.tag:28s} out {e_out / ref.out.bound:.3f}  bias {e_bias / ref.bias.bound:.3f} of the bound')
    assert e_out <= ref.out.bound and e_bias <= ref.bias.bound and ref.out.dead_are_plus_zero(out)      # (IW = 1: the side taps are all padding)


@pytest.mark.parametrize('case', _ids(SPLIT))
def test_the_bound_passes_the_six_term_form_and_fails_it_with_one_term_lost(case):
    ref = R.reference(case).out
    full = ref.scaled_err(case.epilogue(R.six_term(case))) / ref.bound
    print(f'[conv gemm cpu] {case.tag:28s} K {case.K}  e32s {ref.e32s:.3e}  all terms {full:.3f} of the bound')
    assert full <= 1.0 and case.K in (32, 64)
    for drop in (D.INT_DROPPABLE if case.mode in R.BYTE_MODES else D.DROPPABLE):
        lost = ref.scaled_err(case.epilogue(R.six_term(case, drop=drop))) / ref.bound
        print(f'[conv gemm cpu] {case.tag:28s} without {drop[0]}.{drop[1]:3s} {lost:.3f} of the bound')
        assert lost > 1.0, drop


def test_the_rows_table_names_all_twenty_six_kernels():
    fp32 = {(m, k) for m in range(1, 7) for k in (D.FP32_128x64, D.FP32_128x32, D.FP32_256x16)}
    split = {(m, k) for m in range(1, 5) for k in (D.BF16_128x64, D.BF16_128x32)}
    assert {(c.mode, c.kernel) for c in ROWS} == fp32 | split and len(fp32 | split) == 26
    for c in ROWS:
        assert c.kernel[2] == (64 if c.N % 64 == 0 else 32 if c.N % 32 == 0 else 16) and c.products == (1 if c.tag.startswith('bf16x6') else 0)
        assert c.tiles >= 2 and c.M_plan % c.kernel[1] != 0, c.tag                               # >= 2 row tiles, the last one ragged
        assert c.kernel[1] % c.rows_per_frame != 0, c.tag                                                # a tile holds rows of two frames
    asks = {c.tag: c for c in ROWS if 'asks' in c.tag}
    assert all(c.kernel[0] == 0 and c.products == 1 for c in asks.values())
    assert {c.K for c in asks.values() if c.kernel[2] >= 32 and c.mode <= 4} == {48} and {c.mode for c in asks.values() if c.K == 48} == {1, 3}
    assert any(c.kernel == D.FP32_256x16 and c.K % 32 == 0 for c in asks.values())
    assert any(c.mode == 5 and c.K % 32 == 0 for c in asks.values()) and any(c.mode == 6 and c.K % 32 == 0 for c in asks.values())
    grid = [c for c in ROWS if c.tiles >= 9]
    assert {c.mode for c in grid} == {1, 3, 5} and all(-(-c.tiles // 8) >= 2 for c in grid)
    assert {c.epi for c in ROWS if c.mode == 5} == set(range(7)) and {4, 5} <= {c.epi for c in ROWS if c.mode == 6}
    assert all(c.epi == R.EPI_BIAS_RELU for c in FORWARD if c.mode not in (5, 6)) and all(c.epi in R.WITH_MASK for c in DX)
    assert all(c.K in (32, 64) for c in SPLIT)


def test_the_rows_table_holds_the_edges_it_claims():
    def some(pred, cases=ROWS):
        hits = [c.tag for c in cases if pred(c)]
        assert hits
        return hits

    def straddles(c):       # a 16-slab whose first and last element sit in different pixels AND different patch rows
        L = c.op
        k = np.arange(c.K_true)
        pix, ky = k // L.IC, k // L.IC // L.KW
        return c.mode in (1, 4) and any(pix[s] != pix[s + 15] and ky[s] != ky[s + 15] for s in range(0, c.K_true - 15, 16))

    some(lambda c: straddles(c) and c.op.IC < 16 and c.op.IC & (c.op.IC - 1))                   # IC = 12
    some(lambda c: straddles(c) and c.mode == 4)
    some(lambda c: c.mode != 3 and c.op.OW < 16 and c.rows_per_frame >= 16)
    some(lambda c: c.mode != 3 and c.rows_per_frame < 16)
    some(lambda c: c.mode != 3 and c.M % c.rows_per_frame != 0)                                 # M ends inside a frame
    for mode in (1, 2, 4, 5, 6):
        some(lambda c: c.mode == mode and c.M % c.rows_per_frame != 0)
    some(lambda c: c.mode in (5, 6) and c.op.IW == 1)
    some(lambda c: c.mode in (1, 3, 4) and c.layer.KH != c.layer.KW and c.layer.IH != c.layer.IW)
    for mode in (1, 3, 4):
        some(lambda c: c.mode == mode and c.layer.KH != c.layer.KW)
    same = [c for c in ROWS if c.mode == 5]
    small = min(same, key=lambda c: c.op.IH * c.op.IW)
    assert (~small.valid).any(1).all(), 'every pixel of the smallest same-padded image touches the padding'
    assert not all((~c.valid).any(1).all() for c in same), 'and some image has an interior'
    relu = some(lambda c: c.relu_in)
    for c in ROWS:
        if c.tag in relu:
            assert (c.raw < 0).any() and (np.signbit(c.raw) & (c.raw == 0)).any() and (c.A >= 0).all()
    ragged = some(lambda c: c.mode == 3 and (c.layer.IH % c.layer.S or c.layer.IW % c.layer.S))
    for c in ROWS:
        if c.tag in ragged:      # an input pixel no window covers: its whole operand row is padding; the epilogue cursor crosses tiles
            assert (~c.valid).all(1).any() and c.kernel[1] % c.rows_per_frame != 0
            assert not R.reference(c).out.live.all()
    some(lambda c: c.mode == 3 and c.layer.IH % c.layer.S == 0 and c.layer.IW % c.layer.S == 0)
    some(lambda c: c.mode == 3 and c.layer.S == 3)
    some(lambda c: c.mode == 6 and c.K_true == 27 and c.K == 32)
    assert all(c.K > c.K_true and c.K - c.K_true < 16 for c in ROWS if c.mode == 6)
    some(lambda c: c.mode in (4, 6) and c.op.IC == 2 and c.bytes.order == 'chw')
    some(lambda c: c.mode in (4, 6) and c.op.IC == 4 and c.bytes.order == 'chw')
    some(lambda c: c.mode == 4 and c.op.IC == 4 and c.bytes.order == 'hwc' and c.strides[3] % 4 == 0)          # the word path
    some(lambda c: c.mode in (4, 6) and c.bytes.d > 1)
    some(lambda c: c.mode in (4, 6) and c.bytes.slack > 0)
    for c in ROWS:
        if c.mode in (4, 6):
            L, (sc, sy, sx, fb) = c.op, c.strides
            assert (L.IC - 1) * sc + (L.IH - 1) * sy + (L.IW - 1) * sx < fb
        assert c.used.any() and (c.mode == 3 or c.M % c.rows_per_frame == 0 or not c.used.reshape(c.frames, -1)[-1].all()), c.tag


def test_the_weight_table_names_every_reachable_height_and_width():
    heights = {(c.mode, c.kernel[1]) for c in WEIGHTS if c.mode != 0}
    assert heights == {(m, h) for m in (1, 2, 4, 5, 6) for h in (64, 128, 192, 256)}
    for mode in (1, 2, 4, 5, 6):
        mine = [c for c in WEIGHTS if c.mode == mode]
        assert {c.kernel[0] for c in mine} == {64, 32, 16}, mode
        long = [c for c in mine if c.M == 600]
        assert len(long) == 1 and long[0].splits == 3 and long[0].rows_per_split == 208
        assert all(b % long[0].rows_per_frame != 0 for b in (208, 416)), 'both split boundaries fall inside a frame'
        assert all(c.runs == (c.kernel[1] if mode == 4 else max(c.kernel[1], 128)) for c in mine)
    for c in WEIGHTS:
        K = c.K
        assert c.kernel[1] == (64 if K <= 64 else 128 if K <= 128 else 192 if K <= 192 else 256)
        assert c.kernel[0] == (64 if c.N % 64 == 0 else 32 if c.N % 32 == 0 else 16)
        assert c.rows_per_frame < 16 or c.layer.OW < 16                          # the 16-row advance carries at least once, mostly several times
    by = {c.tag: c for c in WEIGHTS}
    assert {c.K for c in WEIGHTS if c.mode == 6} >= {27, 9, 18} and by['m5-k64-K36'].layer.IC == 4 and by['m5-k64-K36'].runs == 128
    assert sum(c.accumulate for c in WEIGHTS) == 1 and sum(not c.with_bias for c in WEIGHTS) == 1
    assert by['dense-perm4-K24'].perm == 4 and {(c.mode, c.perm) for c in WEIGHTS if c.mode} == {(1, 2), (2, 3), (4, 5), (5, 2), (6, 5)}
    assert any(c.M % c.rows_per_frame for c in WEIGHTS) and any(c.relu_in for c in WEIGHTS)


def test_every_case_lands_on_the_kernel_it_is_named_for():
    """pfa_igemm_rows_plan answers per phase (col2im: pixel slots and taps of one phase); pfa_igemm_weights_plan refuses K % 4 != 0, which
    pfa_igemm_weights takes for mode 6: there the case's own splits stand and only the workspace formula is asserted."""
    from pufferlib_amd import _lib
    _lib.build()
    L = _lib.lib()
    out = (C.c_int32 * 5)()
    try:
        for c in ROWS:
            _lib.check(L.pfa_igemm_set_products(c.products), 'set_products')
            _lib.check(L.pfa_igemm_rows_plan(c.mode, c.M_plan, c.K, c.N, out), 'rows_plan')
            assert tuple(out[:4]) == c.kernel + (c.tiles,), (c.tag, tuple(out[:4]))
    finally:
        _lib.check(L.pfa_igemm_set_products(0), 'set_products')
    asked = 0
    for c in WEIGHTS:
        if c.K % 4 == 0:
            asked += 1
            _lib.check(L.pfa_igemm_weights_plan(c.M, c.K, c.N, out), 'weights_plan')
            tn, tk, tiles, splits, rps = out[:5]
            assert (tn, tk) == c.kernel and tiles == -(-c.K // tk) * (c.N // tn), (c.tag, tuple(out[:5]))
            assert splits == c.splits and rps == c.rows_per_split, (c.tag, tuple(out[:5]))
        else:
            assert c.mode == 6 and L.pfa_igemm_weights_plan(c.M, c.K, c.N, out) != 0
        assert L.pfa_igemm_weights_workspace_bytes(c.M, c.K, c.N) == D.workspace_bytes(c.splits, c.K, c.N), c.tag
    assert asked == len(WEIGHTS) - len([c for c in WEIGHTS if c.K % 4])
