"""The weight-gradient contractions C = A^T B (pfa_gemm_tn_f32, pfa_gemm_tn2_f32) in the opt-in bf16x6 product form (csrc/gemm_bf16.hip)
under set_matrix_products('bf16x6'): which tiles take it (host state), dense operands against float64 under the measure and bound of
tests/dense_gemm_reference.py, exact-product probes at the contraction lengths the recurrent update runs, and the engine's three
routed gradient tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_gemm_reference as DG

F32, F64 = np.float32, np.float64
# (mo, no, two_operand): 128 x 256 two-operand tile; 128 x 128, 128 x 64, 128 x 160 single-operand tiles
ROUTED = [(128, 256, 1), (512, 256, 1), (128, 128, 0), (256, 256, 0), (128, 64, 0), (128, 160, 0)]
UNROUTED = [(16, 128, 0), (128, 32, 0), (128, 16, 0), (24, 100, 0), (96, 256, 1)]      # three fp32 tiles, two unsupported shapes


def _switched(form, fn):
    import pufferlib_amd
    try:
        pufferlib_amd.set_matrix_products(form)
        return fn()
    finally:
        pufferlib_amd.set_matrix_products('fp32')


def test_gemm_tn_path_follows_the_switch_on_the_host():
    """pfa_gemm_tn_path launches nothing: 1 for every routed tile under the switch, 0 for the fp32 tiles and for unsupported shapes, 0
    for everything without it; the workspace queries do not depend on the switch."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    paths = lambda shapes: [L.pfa_gemm_tn_path(mo, no, 4099, two) for mo, no, two in shapes]      # noqa: E731
    sizes = lambda: ([L.pfa_gemm_tn_workspace_bytes(mo, no, k) for mo, no, _ in ROUTED + UNROUTED for k in (37, 4099, 131072)],      # noqa: E731
                     [L.pfa_gemm_tn2_workspace_bytes(mo, k) for mo in (128, 512) for k in (37, 4099, 131072)])
    off = sizes()
    assert _switched('bf16x6', lambda: (paths(ROUTED), paths(UNROUTED), sizes())) == ([1] * len(ROUTED), [0] * len(UNROUTED), off)
    assert paths(ROUTED + UNROUTED) == [0] * len(ROUTED + UNROUTED)


def _padded(x, pad):
    """[k][cols] on the device inside a NaN-filled [k][cols + pad] buffer."""
    full = torch.full((x.shape[0], x.shape[1] + pad), float('nan'), device='cuda')
    full[:, :x.shape[1]] = x if isinstance(x, torch.Tensor) else torch.from_numpy(x)
    return full[:, :x.shape[1]]


def _product(two, a, b, form):
    """One call of pfa_gemm_tn2_f32 (b = [b0 | b1], each in a buffer and with a row stride of its own) or pfa_gemm_tn_f32 under `form`,
    from NaN-filled outputs and workspace: C as int32 bits on the CPU, [mo][no].  Nothing outside the tiles is written."""
    from pufferlib_amd import _lib
    L, st = _lib.lib(), _lib.stream_handle()
    k, mo, no = a.shape[0], a.shape[1], b.shape[1]
    nbytes = L.pfa_gemm_tn2_workspace_bytes(mo, k) if two else L.pfa_gemm_tn_workspace_bytes(mo, no, k)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 64,), float('nan'), device='cuda')
    outs = [torch.full((mo, w + 8), float('nan'), device='cuda') for w in ((128, 128) if two else (no,))]
    p = _lib.ptr

    def call():
        if two:
            b0, b1 = b[:, :128], b[:, 128:]
            return L.pfa_gemm_tn2_f32(p(a), a.stride(0), p(b0), b0.stride(0), p(b1), b1.stride(0), p(outs[0]), 136, p(outs[1]), 136, mo, k, p(ws), st)
        return L.pfa_gemm_tn_f32(p(a), a.stride(0), p(b), b.stride(0), p(outs[0]), no + 8, mo, no, k, p(ws), st)
    _lib.check(_switched(form, call), 'gemm_tn')
    torch.cuda.synchronize()
    assert all(torch.isnan(o[:, -8:]).all() for o in outs) and torch.isnan(ws[nbytes // 4:]).all()
    return torch.cat([o[:, :-8] for o in outs], 1).cpu().numpy().view(np.int32)


def _check(two, a, b, exp, tag):
    """The switch-on product within the reference's bound, the same bits twice, and not the fp32 kernel's bits."""
    from pufferlib_amd import _lib
    k, mo, no = a.shape[0], a.shape[1], b.shape[1]
    assert _switched('bf16x6', lambda: _lib.lib().pfa_gemm_tn_path(mo, no, k, two)) == 1
    got = _product(two, a, b, 'bf16x6')
    err = exp.scaled_err(got.view(F32))
    print(f'[gemm_tn bf16x6] {tag}  e32s {exp.e32s:.3e}  err / (MARGIN e32s) {err / exp.bound:.3f}')
    assert err <= exp.bound, (tag, err, exp.bound)
    assert np.array_equal(got, _product(two, a, b, 'bf16x6'))
    assert not np.array_equal(got, _product(two, a, b, 'fp32'))


def _split_b(two, b, pad):
    """The device operand(s) of B: one padded [k][no] buffer, or for tn2 the two halves in buffers and with row strides of their own."""
    return _TwoB(_padded(b[:, :128], 0), _padded(b[:, 128:], 2 * pad)) if two else _padded(b, pad)


class _TwoB:
    """b0 and b1 in buffers of their own behind the [:, :128] / [:, 128:] slicing _product does."""

    def __init__(self, b0, b1):
        self.b0, self.b1, self.shape = b0, b1, (b0.shape[0], 256)

    def __getitem__(self, key):
        return self.b0 if key[1] == slice(None, 128) else self.b1


DENSE = [(1, 128, 256, 37, 16), (1, 256, 256, 1000, 0), (1, 512, 256, 4099, 0),
         (0, 128, 128, 37, 0), (0, 128, 64, 1000, 32), (0, 128, 160, 4099, 0), (0, 256, 256, 1000, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize('two,mo,no,k,pad', DENSE)
def test_dense_contraction_matches_float64_in_the_bf16x6_form(two, mo, no, k, pad):
    """Standard normal operands, every column of A and of B scaled by 2^j, j in -6 .. 6, against A64^T B64 under max |err| / (|A|^T |B|)
    <= MARGIN x the same measure of the fp32 chain over k (no floor).  37 rows: one full slab and a ragged one of 5; 1000 and 4099:
    several splits, the last ragged; 256 and 512 rows of C: two and four row tiles; padded row strides (NaN in the padding)."""
    rs = np.random.RandomState(mo + no + k + two)
    A = (rs.standard_normal((k, mo)).astype(F32) * DG._scales(rs, mo)[None, :]).astype(F32)
    B = (rs.standard_normal((k, no)).astype(F32) * DG._scales(rs, no)[None, :]).astype(F32)
    A64, B64 = A.astype(F64), B.astype(F64)
    exp = DG.Expected(A64.T @ B64, np.abs(A64).T @ np.abs(B64), DG.chain_weights(A, B)[0])
    _check(two, _padded(A, pad), _split_b(two, B, pad), exp, f'dense {mo}x{no} k{k}')


@pytest.mark.gpu
@pytest.mark.parametrize('mo,no,k', [(16, 128, 4099), (128, 32, 1000), (128, 16, 777)])
def test_fp32_tiles_keep_their_bits_under_the_switch(mo, no, k):
    g = torch.Generator(device='cuda').manual_seed(mo + no + k)
    a, b = torch.randn(k, mo, device='cuda', generator=g), torch.randn(k, no, device='cuda', generator=g)
    assert np.array_equal(_product(0, a, b, 'bf16x6'), _product(0, a, b, 'fp32'))


def probe_rows(n, K, seed):
    """k(i) = floor(i K / n) + (131 seed + 17 i) mod floor(K / n) for column i of n, and k(n - 1) = K - 1: one row in each of n equal
    stripes of K — every k split of a launch with at most n splits holds one — and the last in the final, ragged slab."""
    i = np.arange(n, dtype=np.int64)
    k = i * K // n + (131 * seed + 17 * i) % (K // n)
    k[-1] = K - 1
    return k


def probe_operands(mo, no, K, sparse_b, seed):
    """(sparse values [n], their rows k [n], the dense operand [K][cols] as a CPU tensor): the sparse operand (A, or with sparse_b B —
    for tn2 both halves) holds values[i] at (k[i], i) and zeros elsewhere.  Values: standard normal x 2^j per column, j in -6 .. 6."""
    n, cols = (no, mo) if sparse_b else (mo, no)
    rs = np.random.RandomState(seed)
    vals = (rs.standard_normal(n).astype(F32) * DG._scales(rs, n)).astype(F32)
    dense = torch.randn(K, cols, generator=torch.Generator().manual_seed(seed)) * torch.from_numpy(DG._scales(rs, cols))[None, :]
    return vals, probe_rows(n, K, seed), dense


def probe_factors(vals, k, dense, sparse_b):
    """The two factors of every output as [mo][no] broadcasts: out[i][j] = A[k][i] B[k][j] at the one k of its sparse operand's column."""
    d = dense[torch.from_numpy(k)].numpy()                       # [n][cols]
    return (d.T, vals[None, :]) if sparse_b else (vals[:, None], d)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [1, 2])
@pytest.mark.parametrize('sparse_b', [0, 1])
@pytest.mark.parametrize('two,mo,no,K', [(1, 512, 256, 4099), (1, 512, 256, 131072), (0, 128, 160, 131072)])
def test_single_products_keep_every_term_in_the_bf16x6_form(two, mo, no, K, sparse_b, seed):
    """One operand holds ONE non-zero per column (probe_rows), the other is dense, so every output is a single product whatever K is:
    want = the float64 product, S = |want|, the chain is the one rounded fp32 product, bound MARGIN x e32s with no floor — one
    rounding, at which a 2^-16 term stands out at the engine's K = 131 072 as it does at 32.  sparse_b = 0 probes A's loader and split
    against a dense B, 1 swaps the roles.  (128 x 160 runs 512 splits: its 128 / 160 probe rows reach every fourth / third.)
    On the CPU (DG.bf16x6_single on these seeds, all six (shape, role) pairs): the complete six-term form is at <= 0.43 of the bound,
    the form without lo.hi, hi.lo or mid.mid at >= 27.9 bounds."""
    vals, k, dense = probe_operands(mo, no, K, sparse_b, seed)
    fa, fb = probe_factors(vals, k, dense, sparse_b)
    want = fa.astype(F64) * fb.astype(F64)
    exp = DG.Expected(want, np.abs(want), fa * fb)
    sparse = torch.zeros(K, len(vals), device='cuda')
    sparse[torch.from_numpy(k).cuda(), torch.arange(len(vals), device='cuda')] = torch.from_numpy(vals).cuda()
    a, b = (dense.cuda(), sparse) if sparse_b else (sparse, dense.cuda())
    _check(two, a, _TwoB(b[:, :128].contiguous(), b[:, 128:].contiguous()) if two else b, exp, f'probe {mo}x{no} K{K} sparse_b{sparse_b} seed{seed}')


@pytest.mark.gpu
def test_engine_update_reaches_the_bf16x6_contractions():
    """lstm.Engine.update under the switch at 'lstm-s64-small': the two-operand product is routed for its minibatch, and dW_ih, dW_hh
    (128 x 256 tile) and dW_enc (128 x 64) pass test_gpu_lstm_grad_f64's bound against float64."""
    import lstm_grad_reference as LR
    from pufferlib_amd import _lib
    from test_gpu_lstm_grad_f64 import _Engine, _reference
    case = next(c for c in LR.cases() if c.tag == 'lstm-s64-small')
    ref, dev = _reference(case), _Engine(case)

    def run():
        assert _lib.lib().pfa_gemm_tn_path(512, 256, case.rows, 1) == 1
        return dev.sequence()[1]
    got = case.split_flat(_switched('bf16x6', run).cpu().numpy()[:dev.fp.count])
    assert ref.failures(got, names=('recurrent.weight_ih_l0', 'recurrent.weight_hh_l0', 'encoder.weight')) == []
