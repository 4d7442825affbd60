"""The two dense contractions of csrc/igemm.hip restated on the CPU: the rows form C = epilogue(A B^T) (pfa_igemm_rows, operand mode 0)
and the weight form G = A^T D with the column sums of D (pfa_igemm_weights).  Every case is generated from a seed; the module imports
neither the package under test nor the oracle.

Operands are standard normal, then every row of A and every row of B (for D: every column) is scaled by 2^j, j an integer drawn
uniformly from -6 .. 6.  The error measure follows the scales: with want = the float64 product (+ bias) and S = |A| |B|^T (+ |bias|)
in float64,
    scaled_err(got) = max_ij |got_ij - want_ij| / S_ij
so a wrong small row cannot hide behind a large one, as it can under a max-norm bound.  The bound of a case is MARGIN x e32s, e32s being
the scaled_err of the sequential fp32 chain in k order (weight form: in row order) — what include/pufferlib_amd.h promises of the default
kernel — with no absolute floor.  The bound therefore comes from the reference alone, never from the kernel.

ReLU is 1-Lipschitz, so the bias + ReLU epilogue is compared after the ReLU under the same S and no kink has to be excluded.  The
mask of epilogue 3 is an input: where mask <= 0 the expected output is exactly +0.0.

`bf16x6_rows` emulates the opt-in six-term product form of the rows kernels (three bf16 pieces per fp32 operand, the six partial
products above 2^-24 per 32-deep slab, fp32 accumulation), optionally with one term left out: tests/test_dense_gemm_reference_cpu.py
uses it to show that the bound sees a lost term."""
import numpy as np
import torch

MARGIN = 4.0          # fp32 chain errors: the project's own margin (tests/ppo_grad_reference.py, tests/resnet_reference.py)
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_MASK = range(4)
F32, F64 = np.float32, np.float64


def _scales(rs, n):
    return np.ldexp(1.0, rs.randint(-6, 7, n)).astype(F32)


class RowsCase:
    """C [M][N] = epilogue(A [M][K] B [N][K]^T).  kernel: (0 fp32 / 1 bf16x6, tile rows, tile columns) the case is named for; tiles: its
    number of row tiles; products: the pfa_igemm_set_products setting it runs under."""

    def __init__(self, tag, kernel, M, K, N, epi=EPI_BIAS_RELU, products=0, seed=0):
        self.tag, self.kernel, self.M, self.K, self.N, self.epi, self.products, self.seed = tag, kernel, M, K, N, epi, products, seed
        self.tiles = -(-M // kernel[1])

    def __getattr__(self, name):      # the operands are generated when first read: collecting the tests costs nothing
        if name not in ('A', 'B', 'bias', 'mask'):
            raise AttributeError(name)
        M, K, N = self.M, self.K, self.N
        rs = np.random.RandomState(self.seed)
        sb = _scales(rs, N)
        self.A = (rs.standard_normal((M, K)).astype(F32) * _scales(rs, M)[:, None]).astype(F32)
        self.B = (rs.standard_normal((N, K)).astype(F32) * sb[:, None]).astype(F32)
        self.bias = (rs.standard_normal(N).astype(F32) * sb).astype(F32)       # on the scale of its B row: neither lost nor dominant
        self.mask = None
        if self.epi == EPI_MASK:
            mask = rs.standard_normal((M, N)).astype(F32)
            flat = mask.reshape(-1)
            flat[0::7] = 0.0                                                   # relu' reads `mask > 0`: both zeros and the negative
            flat[3::7] = -0.0                                                  # entries give exactly +0.0
            self.mask = mask
        return self.__dict__[name]

    def epilogue(self, acc):
        """The epilogue in the dtype of `acc` (the fp32 chain, the emulator; float64 for the expected value)."""
        if self.epi in (EPI_BIAS, EPI_BIAS_RELU):
            acc = acc + self.bias.astype(acc.dtype)[None, :]
        if self.epi == EPI_BIAS_RELU:
            acc = np.maximum(acc, 0)
        if self.epi == EPI_MASK:
            acc = np.where(self.mask > 0, acc, 0).astype(acc.dtype)
        return acc


class WeightCase:
    """out = A [M][K]^T D [M][N] as [K][N] (perm 0) or [N][K] (perm 1, torch's Linear layout), bias_out = the column sums of D.
    kernel: (tile columns tn, tile height over k) the case is named for.  accumulate: onto `prefill_out` / `prefill_bias`."""

    def __init__(self, tag, kernel, M, K, N, perm=1, accumulate=0, with_bias=True, seed=0):
        self.tag, self.kernel, self.M, self.K, self.N, self.perm, self.accumulate, self.with_bias = tag, kernel, M, K, N, perm, accumulate, with_bias
        self.seed = seed

    def __getattr__(self, name):
        if name not in ('A', 'D', 'prefill_out', 'prefill_bias'):
            raise AttributeError(name)
        M, K, N = self.M, self.K, self.N
        rs = np.random.RandomState(self.seed)
        sd = _scales(rs, N)
        self.A = (rs.standard_normal((M, K)).astype(F32) * _scales(rs, M)[:, None]).astype(F32)
        self.D = (rs.standard_normal((M, N)).astype(F32) * sd[None, :]).astype(F32)
        # the earlier micro-batches' sum of an accumulating launch: on the scale of the product itself
        self.prefill_out = (rs.standard_normal((K, N)).astype(F32) * sd[None, :] * F32(np.sqrt(M))).astype(F32)
        self.prefill_bias = (rs.standard_normal(N).astype(F32) * sd * F32(np.sqrt(M))).astype(F32)
        return self.__dict__[name]

    def layout(self, kn):
        """[K][N] -> the order `out` is written in."""
        return kn if self.perm == 0 else np.ascontiguousarray(kn.T)


def chain_rows(A, B):
    """sum_k A[m][k] B[n][k] as one fp32 chain per output, k ascending: a rounded product, then a rounded add."""
    acc = np.zeros((A.shape[0], B.shape[0]), F32)
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * B[:, k][None, :]
    return acc


def chain_weights(A, D):
    """(sum_m A[m][k] D[m][n], sum_m D[m][n]) as fp32 chains, m ascending."""
    acc, col = np.zeros((A.shape[1], D.shape[1]), F32), np.zeros(D.shape[1], F32)
    for m in range(A.shape[0]):
        acc += A[m][:, None] * D[m][None, :]
        col += D[m]
    return acc, col


def blas_rows(A, B):
    return torch.matmul(torch.from_numpy(A), torch.from_numpy(B).T).numpy()


def blas_weights(A, D):
    return torch.matmul(torch.from_numpy(A).T, torch.from_numpy(D)).numpy(), torch.from_numpy(D).sum(0).numpy()


def _split3(x):
    """fp32 -> (hi, mid, lo) bf16 pieces held as fp32, round to nearest even each time: ig_split4 of csrc/igemm.hip."""
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return {'hi': hi, 'mid': mid, 'lo': lo}


TERMS = (('lo', 'hi'), ('hi', 'lo'), ('mid', 'mid'), ('mid', 'hi'), ('hi', 'mid'), ('hi', 'hi'))     # (piece of A, piece of B), small first
DROPPABLE = TERMS[:3]                                                                              # the three terms at 2^-16 relative
INT_TERMS = (('hi', 'lo'), ('hi', 'mid'), ('hi', 'hi'))      # A holds integers 0 .. 255 (one exact bf16 piece): the kernel issues three terms
INT_DROPPABLE = INT_TERMS[:1]


def bf16x6_rows(A, B, drop=None, a_int=False):
    """A B^T as igemm_rows_split_kernel forms it: per 32-deep slab the six partial products in the kernel's order, each added to the fp32
    accumulator (a bf16 x bf16 product is exact in fp32; the 32 of a slab are summed in fp32).  drop: one of TERMS to leave out.
    a_int: A is integer bytes as floats (the uint8 conv operands) — the three terms of INT_TERMS."""
    a, b = _split3(torch.from_numpy(A)), _split3(torch.from_numpy(B))
    assert not a_int or bool((a['hi'] == torch.from_numpy(A)).all())
    acc = torch.zeros(A.shape[0], B.shape[0])
    for s in range(0, A.shape[1], 32):
        for pa, pb in (INT_TERMS if a_int else TERMS):
            if (pa, pb) != drop:
                acc = acc + a[pa][:, s:s + 32] @ b[pb][:, s:s + 32].T
    return acc.numpy()


class Expected:
    """want, S (float64) and the fp32 chain's own scaled error of one output tensor.  prefill (accumulating launches): what the output
    held before; it joins `want` after e32s is taken, and one ulp of it is allowed per element on top of the bound."""

    def __init__(self, want, S, chain, prefill=None):
        self.want, self.S, self.slack = want, S, None
        assert want.dtype == F64 and S.dtype == F64 and chain.dtype == F32 and (S > 0).all()
        self.e32s = self.scaled_err(chain)
        self.bound = MARGIN * self.e32s
        assert self.e32s > 0
        if prefill is not None:
            self.want = want + prefill.astype(F64)
            self.slack = np.spacing(np.abs(prefill)).astype(F64)

    def scaled_err(self, got):
        """max |got - want| / S.  With a prefill the denominator is S + ulp(prefill) / bound, so that `<= bound` holds exactly when
        every element is within bound x S + one ulp of its prefill."""
        err = np.abs(got.astype(F64) - self.want)
        assert np.isfinite(err).all(), 'NaN or Inf in the result'
        return float((err / (self.S if self.slack is None else self.S + self.slack / self.bound)).max())


class RowsReference:
    def __init__(self, case):
        A64, B64 = case.A.astype(F64), case.B.astype(F64)
        S = np.abs(A64) @ np.abs(B64).T
        if case.epi in (EPI_BIAS, EPI_BIAS_RELU):
            S = S + np.abs(case.bias.astype(F64))[None, :]
        self.case = case
        self.out = Expected(case.epilogue(A64 @ B64.T), S, case.epilogue(chain_rows(case.A, case.B)))


class WeightReference:
    def __init__(self, case):
        A64, D64 = case.A.astype(F64), case.D.astype(F64)
        acc, col = chain_weights(case.A, case.D)
        self.case = case
        acc_on = bool(case.accumulate)
        self.out = Expected(case.layout(A64.T @ D64), case.layout(np.abs(A64).T @ np.abs(D64)), case.layout(acc),
                            case.layout(case.prefill_out) if acc_on else None)
        self.bias = Expected(D64.sum(0), np.abs(D64).sum(0), col, case.prefill_bias if acc_on else None)


def workspace_bytes(splits, K, N):
    """What pfa_igemm_weights_workspace_bytes must return for a plan of `splits` row splits: the fp32 partial tiles rounded up to 256
    bytes, the float64 column-sum partials, 256 bytes of slack."""
    return (splits * K * N * 4 + 255) // 256 * 256 + splits * N * 8 + 256


_refs = {}


def reference(case):
    """The reference of a case, computed once and left unchanged (the last few are kept: the tests of a case run next to each other,
    and the float64 tensors of the 4000-row cases are 16 MB each)."""
    if case.tag not in _refs:
        while len(_refs) >= 4:
            _refs.pop(next(iter(_refs)))
        _refs[case.tag] = (RowsReference if isinstance(case, RowsCase) else WeightReference)(case)
    return _refs[case.tag]


FP32_64x64, FP32_64x32, FP32_64x16 = (0, 64, 64), (0, 64, 32), (0, 64, 16)
FP32_128x64, FP32_128x32, FP32_256x16 = (0, 128, 64), (0, 128, 32), (0, 256, 16)
BF16_128x64, BF16_128x32 = (1, 128, 64), (1, 128, 32)


def rows_cases():
    """The smallest shapes that reach each of the eight rows-form kernels under the selection rules of ig_rows_plan (csrc/igemm.hip):
    64-row tiles while ceil(M / 128) (N / tn) < 256 (tn = 16: ceil(M / 256)), so the full tiles need ~4000 rows at N = 512.  3970 rows are
    32 tiles of 128 with 2 rows in the last; 4100 are 33, a grid of 40 whose XCD permutation leaves 7 workgroups without a tile.
    Epilogues 0..3 on one few-rows and one full-tile kernel, bias + ReLU everywhere else."""
    c = []
    for M in (1, 63, 70):
        for K in (16, 48):
            c.append(RowsCase(f'64x64-M{M}-K{K}', FP32_64x64, M, K, 64, seed=len(c)))
    c.append(RowsCase('64x32-M130-K32', FP32_64x32, 130, 32, 96, seed=len(c)))
    for N in (16, 48):
        for K in (16, 80):
            c.append(RowsCase(f'64x16-N{N}-K{K}', FP32_64x16, 65, K, N, seed=len(c)))
    c.append(RowsCase('128x64-M3970', FP32_128x64, 3970, 32, 512, seed=len(c)))
    c.append(RowsCase('128x64-M4100', FP32_128x64, 4100, 32, 512, seed=len(c)))
    c.append(RowsCase('128x32-M2180-K48', FP32_128x32, 2180, 48, 480, seed=len(c)))
    c.append(RowsCase('256x16-M3850-K16', FP32_256x16, 3850, 16, 272, seed=len(c)))
    for epi, name in ((EPI_NONE, 'none'), (EPI_BIAS, 'bias'), (EPI_MASK, 'mask')):
        c.append(RowsCase(f'64x64-M70-K48-{name}', FP32_64x64, 70, 48, 64, epi=epi, seed=len(c)))
        c.append(RowsCase(f'128x64-M3970-{name}', FP32_128x64, 3970, 32, 512, epi=epi, seed=len(c)))
    c.append(RowsCase('bf16x6-128x64-K32', BF16_128x64, 3970, 32, 512, products=1, seed=len(c)))
    c.append(RowsCase('bf16x6-128x64-K96', BF16_128x64, 3970, 96, 512, products=1, seed=len(c)))
    c.append(RowsCase('bf16x6-128x32-K64', BF16_128x32, 2180, 64, 480, products=1, seed=len(c)))
    # products = 1 where the split kernels do not apply: a contraction that is no multiple of 32, 16-column tiles
    c.append(RowsCase('bf16x6-asks-128x64-K48', FP32_128x64, 3970, 48, 512, products=1, seed=len(c)))
    c.append(RowsCase('bf16x6-asks-256x16-K16', FP32_256x16, 3850, 16, 272, products=1, seed=len(c)))
    assert len({x.tag for x in c}) == len(c)
    return c


def weight_cases():
    """One case per (tn, tile height) of igemm_weights_kernel: tn = 64 (N = 64, 128: one and two column tiles), 32 (N = 96), 16 (N = 48,
    80: three and five); heights 64 (K = 16, 52, 64), 128 (68, 128), 192 (132 — a multiple of 4, not of 16 —, 192, and 320: two k-tiles,
    the second ragged), 256 (196, 256).  600 rows: three row splits of 208 rows, the last slab of the last split ragged.  One case
    each writes [K][N], accumulates, and has no bias_out; 5 rows are fewer than one slab."""
    M = 600
    table = [('tn64-k64-K16-N64', (64, 64), M, 16, 64, {}),
             ('tn64-k128-K68-N128', (64, 128), M, 68, 128, {}),
             ('tn64-k192-K132-N64-perm0', (64, 192), M, 132, 64, {'perm': 0}),
             ('tn64-k256-K196-N128', (64, 256), M, 196, 128, {}),
             ('tn32-k64-K52-N96', (32, 64), M, 52, 96, {}),
             ('tn32-k128-K128-N96-accumulate', (32, 128), M, 128, 96, {'accumulate': 1}),
             ('tn32-k192-K192-N96', (32, 192), M, 192, 96, {}),
             ('tn32-k256-K256-N96', (32, 256), M, 256, 96, {}),
             ('tn16-k64-K64-N48', (16, 64), M, 64, 48, {}),
             ('tn16-k128-K68-N80-nobias', (16, 128), M, 68, 80, {'with_bias': False}),
             ('tn16-k192-K320-N48', (16, 192), M, 320, 48, {}),
             ('tn16-k256-K196-N80', (16, 256), M, 196, 80, {}),
             ('tn32-k64-K52-N96-M5', (32, 64), 5, 52, 96, {})]
    c = [WeightCase(tag, kernel, m, k, n, seed=100 + i, **kw) for i, (tag, kernel, m, k, n, kw) in enumerate(table)]
    assert len({x.tag for x in c}) == len(c)
    return c
