"""The conv operand modes (1 - 6) of csrc/igemm.hip restated on the CPU, under the measure of tests/dense_gemm_reference.py.  For each case
the operand A [M][K] is MATERIALISED in fp32 from the raw input (NHWC activations, uint8 frames) by plain numpy indexing, written from
the mode definitions of include/pufferlib_amd.h — patch order, strides, padding reads as 0, the col2im phases y = yy S + py with tap
(jy, jx) reading dOut (yy - jy, xx - jx) — and not from the kernels' incremental cursors.  B is built the same way from weights in
torch's layout [OC][IC][KH][KW]: forward [OC][k] in the loader's order (`/ 255` for byte operands, one fp32 division), phase-major dX,
flipped same-padded dX, NHWC-permuted fc.  From there on it is the dense machinery: want = A64 B64^T, S = |A64| |B64|^T (+ |bias| +
|addend|), e32s from the sequential fp32 chain in k order (weight form: in row order), bound = MARGIN x e32s, no floor.

Inputs: float inputs are standard normal with every input PIXEL scaled by 2^j, j uniform in -6 .. 6 (a per-frame scale would be useless:
the measure is invariant under it), every row of B and every column of D likewise; byte inputs are uniform 0 .. 255; ReLU-on-load inputs
carry -0.0 next to their negatives; masks hold 0.0, -0.0 and negatives; addends have the standard deviation of the product they join.

Where S == 0 — col2im pixels no window covers, outputs under mask <= 0 — the expected output is exactly +0.0 and is compared by bits,
outside the scaled error (`Masked`).  For EPI_MASK_ADD under mask <= 0, S = |addend| and want = addend: the fp32 sum 0 + addend is exact.
Weight-form results are compared in torch's parameter layout through `perm`; the `/ 255` of perm 3 and 5 is applied in float64 to want
and S.  The module imports neither the package under test nor the oracle."""
import numpy as np

from dense_gemm_reference import (BF16_128x32, BF16_128x64, F32, F64, FP32_128x32, FP32_128x64, FP32_256x16, Expected, _scales, bf16x6_rows,
                                  chain_rows, chain_weights)

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_MASK, EPI_BIAS_ADD, EPI_BIAS_ADD_RELU, EPI_MASK_ADD = range(7)
DENSE, IM2COL_F32, IM2COL_U8, COL2IM, IM2COL_U8S, IM2COL_PAD, IM2COL_U8P = range(7)
BYTE_MODES = (IM2COL_U8, IM2COL_U8S, IM2COL_U8P)
WITH_BIAS, WITH_MASK, WITH_ADDEND = (1, 2, 4, 5), (3, 6), (4, 5, 6)


class Layer:
    """Conv2d(IC, OC, (KH, KW), stride S), valid padding; same: stride 1, padding (KH - 1) / 2, OH = IH, OW = IW."""

    def __init__(self, IC, IH, IW, OC, KH, KW, S=1, same=False):
        self.IC, self.IH, self.IW, self.OC, self.KH, self.KW, self.S, self.same = IC, IH, IW, OC, KH, KW, S, same
        self.OH, self.OW = (IH, IW) if same else ((IH - KH) // S + 1, (IW - KW) // S + 1)
        self.pad = (KH - 1) // 2 if same else 0
        assert self.OH >= 1 and self.OW >= 1 and (not same or (S == 1 and KH == KW and KH % 2 == 1))

    @property
    def geom(self):
        return (self.IC, self.IH, self.IW, self.OC, self.OH, self.OW, self.KH, self.KW, self.S)

    def transposed(self):
        """dX of a same-padded layer: the same mode on dOut with the channel roles swapped."""
        return Layer(self.OC, self.IH, self.IW, self.IC, self.KH, self.KW, 1, True)


class Bytes:
    """Frames for modes 4 and 6: channel-first ('chw') or channel-last ('hwc') images of d times the layer's size read through a
    `[::d, ::d]` pixel stride, `slack` unused bytes behind every frame."""

    def __init__(self, order, d=1, slack=0):
        self.order, self.d, self.slack = order, d, slack

    def strides(self, L):
        """(sc, sy, sx, frame_bytes) as include/pufferlib_amd.h states them for CHW and HWC."""
        H, W, d = L.IH * self.d, L.IW * self.d, self.d
        if self.order == 'chw':
            return (H * W, d * W, d, L.IC * H * W + self.slack)
        return (1, d * W * L.IC, d * L.IC, H * W * L.IC + self.slack)


# ------------------------------------------------------------------------------------------------ the layouts of the other operand
def fwd_layout(W, order, div=False, ld=None):
    """torch [OC][IC][KH][KW] -> [OC][k]: 'kkc' k = (ky KW + kx) IC + ic (modes 1, 4, 5, 6), 'ckk' k = (ic KH + ky) KW + kx (mode 2, torch's
    own order); div: / 255 in W's precision; ld: that many columns, the added ones zero."""
    B = (W.transpose(0, 2, 3, 1) if order == 'kkc' else W).reshape(W.shape[0], -1)
    if div:
        B = B / W.dtype.type(255)
    if ld is not None:
        B = np.concatenate([B, np.zeros((B.shape[0], ld - B.shape[1]), W.dtype)], 1)
    return np.ascontiguousarray(B)


def dx_phase_layout(W, S):
    """-> [S S][IC][(jy JW + jx) OC + oc], phase py S + px, kernel tap (ky, kx) = (py + jy S, px + jx S)."""
    OC, IC, KH, KW = W.shape
    JH, JW = KH // S, KW // S
    B = np.zeros((S * S, IC, JH * JW * OC), W.dtype)
    for py in range(S):
        for px in range(S):
            for jy in range(JH):
                for jx in range(JW):
                    B[py * S + px, :, (jy * JW + jx) * OC:(jy * JW + jx + 1) * OC] = W[:, :, py + jy * S, px + jx * S].T
    return B


def dx_flipped_layout(W):
    """-> [IC][(ky KW + kx) OC + oc] = W[oc][ic][KH - 1 - ky][KW - 1 - kx]."""
    return np.ascontiguousarray(W[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(W.shape[1], -1))


def fc_layouts(W, C, HW):
    """Linear [N][c HW + pix] behind an NCHW Flatten -> ([N][pix C + c], its transpose [K][N])."""
    perm = np.ascontiguousarray(W.reshape(W.shape[0], C, HW).transpose(0, 2, 1).reshape(W.shape[0], -1))
    return perm, np.ascontiguousarray(perm.T)


def perm_positions(perm, K, N, geom):
    """Flat position in `out` of element (k, n) of G = A^T D, as a [K][N] array: the perm definitions of pfa_igemm_weights."""
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    IC, IH, IW, KH, KW = geom[0], geom[1], geom[2], geom[6], geom[7]
    if perm == 0:
        return k * N + n
    if perm in (1, 3):                                  # 3: (ic, ky, kx) is torch's order within an output channel
        return n * K + k
    pix, ic = k // IC, k % IC
    if perm == 4:                                       # k = (y IW + x) IC + c -> column c IH IW + y IW + x of a Linear
        return n * K + ic * IH * IW + pix
    return ((n * IC + ic) * KH + pix // KW) * KW + pix % KW      # 2, 5: [oc = n][ic][ky][kx] from k = (ky KW + kx) IC + ic


# ------------------------------------------------------------------------------------------------------------- the operand itself
def gather_index(mode, L, M, K, strides=None):
    """For rows m < M and patch elements k < K of operand `mode` on geometry L: (flat index into the raw input, valid, phase of each
    row).  An invalid element reads as 0.  mode 3: m counts INPUT pixels (n, y, x) of the forward layer L, the raw input is dOut."""
    m, k = np.arange(M)[:, None], np.arange(K)[None, :]
    phase = np.zeros(M, np.int64)
    if mode == COL2IM:
        S, JW = L.S, L.KW // L.S
        n, y, x = m // (L.IH * L.IW), m // L.IW % L.IH, m % L.IW
        phase = ((y % S) * S + x % S)[:, 0]
        jy, jx, oc = k // L.OC // JW, k // L.OC % JW, k % L.OC
        oy, ox = y // S - jy, x // S - jx
        ok = (oy >= 0) & (oy < L.OH) & (ox >= 0) & (ox < L.OW)
        return ((n * L.OH + oy) * L.OW + ox) * L.OC + oc, ok, phase
    n, oy, ox = m // (L.OH * L.OW), m // L.OW % L.OH, m % L.OW
    if mode == IM2COL_U8:
        ic, ky, kx = k // (L.KH * L.KW), k // L.KW % L.KH, k % L.KW
    else:
        ky, kx, ic = k // L.IC // L.KW, k // L.IC % L.KW, k % L.IC
    y, x = oy * L.S + ky - L.pad, ox * L.S + kx - L.pad
    ok = (y >= 0) & (y < L.IH) & (x >= 0) & (x < L.IW) & (k < L.KH * L.KW * L.IC)
    if mode in (IM2COL_F32, IM2COL_PAD):
        idx = ((n * L.IH + y) * L.IW + x) * L.IC + ic
    elif mode == IM2COL_U8:
        idx = ((n * L.IC + ic) * L.IH + y) * L.IW + x
    else:
        sc, sy, sx, fb = strides
        idx = n * fb + ic * sc + y * sy + x * sx
    return idx, ok, phase


def by_phase(f, A, B, phase, dtype):
    """out[m] = f(A[m], B[phase[m]]) with B [P][N][K]."""
    out = np.zeros((A.shape[0], B.shape[1]), dtype)
    for p in range(B.shape[0]):
        sel = phase == p
        if sel.any():
            out[sel] = f(A[sel], B[p])
    return out


class _Case:
    """What rows and weight cases share: the raw input, the gathered operand and the torch-layout weights."""
    FIELDS = ()

    def __getattr__(self, name):      # everything is generated when first read: collecting the tests costs nothing
        if name not in self.FIELDS:
            raise AttributeError(name)
        self._materialise(np.random.RandomState(self.seed))
        return self.__dict__[name]

    def _raw_and_operand(self, rs):
        """self.raw (flat, poisoned copy in self.raw_guarded: every element no (m, k) reads is NaN / 255), self.A, self.phase."""
        mode, L = self.mode, self.op
        self.strides = self.bytes.strides(L) if mode in (IM2COL_U8S, IM2COL_U8P) else (0,) * 4
        if mode in BYTE_MODES:
            per_frame = L.IC * L.IH * L.IW if mode == IM2COL_U8 else self.strides[3]
            raw = rs.randint(0, 256, self.frames * per_frame).astype(np.uint8)
        else:
            H, W, Cc = (L.OH, L.OW, L.OC) if mode == COL2IM else (L.IH, L.IW, L.IC)
            pix = rs.standard_normal((self.frames * H * W, Cc)).astype(F32) * _scales(rs, self.frames * H * W)[:, None]
            raw = pix.astype(F32).reshape(-1)
            if self.relu_in:
                raw[2::13] = -0.0
            per_frame = H * W * Cc
        self.per_frame = per_frame
        idx, ok, self.phase = gather_index(mode, L, self.M, self.K, self.strides)
        assert idx[ok].min() >= 0 and idx[ok].max() < raw.size
        A = np.where(ok, raw[np.where(ok, idx, 0)], 0).astype(F32)
        self.A = np.maximum(A, F32(0)) if self.relu_in else A
        used = np.zeros(raw.size, bool)
        used[idx[ok]] = True
        self.raw, self.used, self.index, self.valid = raw, used, idx, ok
        self.raw_guarded = np.where(used, raw, np.uint8(255) if raw.dtype == np.uint8 else F32(np.nan))

    def image64(self):
        """The raw input as torch sees it: float64 NCHW, bytes / 255, ReLU applied where the loader applies it."""
        L, n = self.op, self.frames
        if self.mode == IM2COL_U8:
            return self.raw.reshape(n, L.IC, L.IH, L.IW).astype(F64) / 255
        if self.mode in (IM2COL_U8S, IM2COL_U8P):
            sc, sy, sx, fb = self.strides
            ic, y, x = np.arange(L.IC)[:, None, None], np.arange(L.IH)[None, :, None], np.arange(L.IW)[None, None, :]
            return self.raw.reshape(n, fb)[:, ic * sc + y * sy + x * sx].astype(F64) / 255
        H, W, Cc = (L.OH, L.OW, L.OC) if self.mode == COL2IM else (L.IH, L.IW, L.IC)
        img = self.raw.reshape(n, H, W, Cc).transpose(0, 3, 1, 2).astype(F64)
        return np.maximum(img, 0) if self.relu_in else img


class ConvRows(_Case):
    """C = epilogue(A(m, k) B^T) for a conv operand.  layer: the FORWARD layer; kind 'fwd' (N = OC) or 'dx' (mode 3: col2im of dOut, m =
    input pixel; mode 5: the same-padded product on dOut against the flipped kernel; N = IC).  kernel: (0 fp32 / 1 six-term, tile rows,
    tile columns) the case is named for.  M: rows (default: whole frames); K: the contraction length the kernel runs per phase."""
    FIELDS = ('raw', 'raw_guarded', 'used', 'A', 'phase', 'W', 'B', 'bias', 'mask', 'addend', 'strides', 'per_frame', 'index', 'valid')

    def __init__(self, tag, mode, kernel, layer, frames, kind='fwd', M=None, epi=None, products=0, relu_in=0, bytes=None, seed=0):
        self.tag, self.mode, self.kernel, self.layer, self.frames, self.kind = tag, mode, kernel, layer, frames, kind
        self.products, self.relu_in, self.bytes, self.seed = products, relu_in, bytes, seed
        self.epi = epi if epi is not None else (EPI_BIAS_RELU if kind == 'fwd' else EPI_MASK)
        L = layer
        self.op = L.transposed() if (kind == 'dx' and mode == IM2COL_PAD) else L      # the geometry the operand is described by
        self.N = L.OC if kind == 'fwd' else L.IC
        if mode == COL2IM:
            assert kind == 'dx' and M is None
            self.phases = L.S * L.S
            self.K = self.K_true = (L.KH // L.S) * (L.KW // L.S) * L.OC
            self.K_call = L.KH * L.KW * L.OC
            self.M = frames * L.IH * L.IW
            self.M_plan = frames * -(-L.IH // L.S) * -(-L.IW // L.S)          # pixel slots per phase, ragged ones included
            self.rows_per_frame = -(-L.IH // L.S) * -(-L.IW // L.S)
        else:
            self.phases = 1
            self.K_true = self.op.KH * self.op.KW * self.op.IC
            self.K = -(-self.K_true // 16) * 16 if mode == IM2COL_U8P else self.K_true
            self.K_call = self.K
            self.rows_per_frame = self.op.OH * self.op.OW
            self.M = M if M is not None else frames * self.rows_per_frame
            self.M_plan = self.M
            assert (frames - 1) * self.rows_per_frame < self.M <= frames * self.rows_per_frame
        assert self.K % 16 == 0 and self.N % 16 == 0
        self.tiles = -(-self.M_plan // kernel[1])

    def make_B(self, W):
        """[P][N][K] from torch-layout weights, in W's precision."""
        L = self.layer
        if self.mode == COL2IM:
            return dx_phase_layout(W, L.S)
        if self.kind == 'dx':
            return dx_flipped_layout(W)[None]
        order = 'ckk' if self.mode == IM2COL_U8 else 'kkc'
        return fwd_layout(W, order, self.mode in BYTE_MODES, self.K)[None]

    def _materialise(self, rs):
        L, M, N = self.layer, self.M, self.N
        self._raw_and_operand(rs)
        W = rs.standard_normal((L.OC, L.IC, L.KH, L.KW)).astype(F32)
        sb = _scales(rs, N)                                                       # one scale per row of B
        self.W = (W * (sb[:, None, None, None] if self.kind == 'fwd' else sb[None, :, None, None])).astype(F32)
        self.B = self.make_B(self.W)
        assert self.B.dtype == F32 and self.B.shape == (self.phases, N, self.K)
        self.bias = (rs.standard_normal(N).astype(F32) * sb).astype(F32)
        mask = rs.standard_normal((M, N)).astype(F32)
        flat = mask.reshape(-1)
        flat[0::7], flat[3::7] = 0.0, -0.0
        self.mask = mask if self.epi in WITH_MASK else None
        std = np.sqrt(by_phase(lambda a, b: a @ b.T, self.A.astype(F64) ** 2, self.B.astype(F64) ** 2, self.phase, F64))
        self.addend = (rs.standard_normal((M, N)) * std).astype(F32) if self.epi in WITH_ADDEND else None

    def product(self, f, A, B, dtype):
        return by_phase(f, A, B, self.phase, dtype)

    def epilogue(self, acc):
        """The epilogue in the dtype of `acc`."""
        t = acc.dtype
        if self.epi in WITH_BIAS:
            acc = acc + self.bias.astype(t)[None, :]
        if self.epi in WITH_MASK:
            acc = np.where(self.mask > 0, acc, 0).astype(t)
        if self.epi in WITH_ADDEND:
            acc = acc + self.addend.astype(t)
        if self.epi in (EPI_BIAS_RELU, EPI_BIAS_ADD_RELU):
            acc = np.maximum(acc, 0)
        return acc.astype(t)

    def epilogue_S(self, S):
        if self.epi in WITH_BIAS:
            S = S + np.abs(self.bias.astype(F64))[None, :]
        if self.epi in WITH_MASK:
            S = np.where(self.mask > 0, S, 0.0)
        if self.epi in WITH_ADDEND:
            S = S + np.abs(self.addend.astype(F64))
        return S


class ConvWeights(_Case):
    """out = A(m, k)^T D [M][N] scattered through `perm` into torch's parameter layout, bias_out = the column sums of D.  kernel: (tile
    columns, tile height over k) of the PLAN; `runs`: the height the launch instantiates (a plan of 64 runs the 128-high kernel for every
    operand but modes 0 and 4).  splits: stated here, since pfa_igemm_weights_plan refuses the K % 4 != 0 that mode 6 brings."""
    FIELDS = ('raw', 'raw_guarded', 'used', 'A', 'phase', 'D', 'prefill_out', 'prefill_bias', 'strides', 'per_frame', 'index', 'valid')

    def __init__(self, tag, mode, kernel, layer, M, perm, accumulate=0, with_bias=True, relu_in=0, bytes=None, seed=0):
        self.tag, self.mode, self.kernel, self.layer, self.op, self.M, self.perm = tag, mode, kernel, layer, layer, M, perm
        self.accumulate, self.with_bias, self.relu_in, self.bytes, self.seed = accumulate, with_bias, relu_in, bytes, seed
        L = layer
        self.N = L.OC
        self.K = self.K_true = L.KH * L.KW * L.IC
        self.rows_per_frame = L.OH * L.OW
        self.frames = -(-M // self.rows_per_frame)
        self.splits = -(-M // 256)
        self.rows_per_split = -(-(-(-M // self.splits)) // 16) * 16
        self.runs = 128 if kernel[1] == 64 and mode != IM2COL_U8S else kernel[1]
        self.scale = 255.0 if mode in BYTE_MODES else 1.0

    def _materialise(self, rs):
        M, K, N = self.M, self.K, self.N
        self._raw_and_operand(rs)
        sd = _scales(rs, N)
        self.D = (rs.standard_normal((M, N)).astype(F32) * sd[None, :]).astype(F32)
        self.prefill_out = (rs.standard_normal((K, N)).astype(F32) * sd[None, :] * F32(np.sqrt(M))).astype(F32)
        self.prefill_bias = (rs.standard_normal(N).astype(F32) * sd * F32(np.sqrt(M))).astype(F32)

    def layout(self, kn):
        """[K][N] -> the flat order `out` is written in."""
        out = np.zeros(kn.size, kn.dtype)
        out[perm_positions(self.perm, self.K, self.N, self.layer.geom).reshape(-1)] = kn.reshape(-1)
        return out


class DenseFlatten(ConvWeights):
    """Mode 0 with the geometry of a flattened tensor: the dW of a Linear behind nn.Flatten of an NCHW tensor kept as NHWC rows (perm 4)."""

    def __init__(self, tag, kernel, C, H, W, N, M, seed=0):
        ConvWeights.__init__(self, tag, DENSE, kernel, Layer(C, H, W, N, H, W), M, 4, seed=seed)
        self.runs = kernel[1]

    def _raw_and_operand(self, rs):
        self.A = (rs.standard_normal((self.M, self.K)).astype(F32) * _scales(rs, self.M)[:, None]).astype(F32)
        self.raw = self.raw_guarded = self.A
        self.phase, self.strides, self.per_frame, self.used, self.index, self.valid = np.zeros(self.M, np.int64), (0,) * 4, self.K, None, None, None


# ---------------------------------------------------------------------------------------------------------------- the references
class Masked:
    """Expected (tests/dense_gemm_reference.py) on the elements with S > 0; the others are expected to be exactly +0.0, by bits.
    scale: want and S are divided by it in float64 after e32s is taken (the measure does not change under it)."""

    def __init__(self, want, S, chain, prefill=None, scale=1.0):
        self.live = S > 0
        assert self.live.any() and not want[~self.live].any()
        live = self.live
        self.exp = Expected(want[live], S[live], chain[live], None if prefill is None else prefill[live])
        assert scale == 1.0 or prefill is None
        self.exp.want, self.exp.S = self.exp.want / scale, self.exp.S / scale
        self.want = np.where(live, (want if prefill is None else want + prefill.astype(F64)) / scale, 0.0)
        self.S = S / scale
        self.e32s, self.bound = self.exp.e32s, self.exp.bound

    def scaled_err(self, got):
        return self.exp.scaled_err(got[self.live])

    def dead_are_plus_zero(self, got):
        return not np.ascontiguousarray(got[~self.live]).view(np.uint32).any()


class RowsReference:
    def __init__(self, c):
        A64, B64 = c.A.astype(F64), c.B.astype(F64)
        self.acc64 = c.product(lambda a, b: a @ b.T, A64, B64, F64)
        self.S_product = c.product(lambda a, b: a @ b.T, np.abs(A64), np.abs(B64), F64)
        self.out = Masked(c.epilogue(self.acc64), c.epilogue_S(self.S_product), c.epilogue(c.product(chain_rows, c.A, c.B, F32)))


class WeightReference:
    def __init__(self, c):
        A64, D64 = c.A.astype(F64), c.D.astype(F64)
        acc, col = chain_weights(c.A, c.D)
        on = bool(c.accumulate)
        self.out = Masked(c.layout(A64.T @ D64), c.layout(np.abs(A64).T @ np.abs(D64)), c.layout(acc), c.layout(c.prefill_out) if on else None,
                          c.scale)
        self.bias = Masked(D64.sum(0), np.abs(D64).sum(0), col, c.prefill_bias if on else None)


_refs = {}


def reference(case):
    """Computed once per case and left unchanged (the last few are kept: the tests of a case run next to each other)."""
    if case.tag not in _refs:
        while len(_refs) >= 4:
            _refs.pop(next(iter(_refs)))
        _refs[case.tag] = (RowsReference if isinstance(case, ConvRows) else WeightReference)(case)
    return _refs[case.tag]




def six_term(case, drop=None):
    """The product as igemm_rows_split_kernel forms it (float operands: six terms per 32-deep slab; byte operands: three)."""
    a_int = case.mode in BYTE_MODES
    return case.product(lambda a, b: bf16x6_rows(a, b, drop=drop, a_int=a_int), case.A, case.B, F32)


# --------------------------------------------------------------------------------------------------------------------- the tables
HWC, CHW = Bytes('hwc'), Bytes('chw')


def rows_cases():
    """The smallest shapes that reach every conv rows-form kernel and every edge tests/test_conv_gemm_reference_cpu.py lists.  The conv
    modes never take the 64-row tiles (ig_rows_plan: `few` is dense only), so N alone chooses the tile: 64 -> 128 x 64, 32 -> 128 x 32,
    16 -> 256 x 16, and ~180 - 300 rows are two row tiles with a ragged last one.  Images and kernels are non-square wherever the mode
    allows.  The three `grid` cases have 10 row tiles: a grid of 16, two tiles per XCD, six workgroups without one.
    Measured on an MI355X: the 85 tests of tests/test_gpu_conv_gemm.py (this table, the weight table, the pack kernels) and the 52 of the
    dense file take 3.4 s together."""
    c = []

    def add(tag, mode, kernel, layer, frames, **kw):
        c.append(ConvRows(tag, mode, kernel, layer, frames, seed=1000 + len(c), **kw))

    # mode 1: IC = 12 (a 16-slab straddles pixels and patch rows), OH OW = 12 with M inside a frame, IH != IW, KH != KW
    m1 = {64: (Layer(12, 6, 5, 64, 2, 2), 11, None), 32: (Layer(4, 10, 7, 32, 4, 3, S=2), 15, 175), 16: (Layer(8, 5, 6, 16, 3, 2), 20, None)}
    # mode 2: aligned NCHW bytes, KW, IW, S multiples of 4
    m2 = {64: (Layer(1, 12, 16, 64, 4, 4, S=4), 15, None), 32: (Layer(3, 6, 16, 32, 2, 8, S=4), 30, 177),
          16: (Layer(2, 10, 12, 16, 2, 4, S=4), 34, None)}
    # mode 4: one word per pixel (HWC, IC = 4); bytes at IC = 2 through a [::2, ::2] stride with 7 spare bytes per frame; channel-first IC = 4
    m4 = {64: (Layer(4, 7, 9, 64, 2, 2, S=2), 16, None, HWC), 32: (Layer(2, 5, 4, 32, 4, 2), 30, 178, Bytes('chw', 2, 7)),
          16: (Layer(4, 6, 5, 16, 4, 3), 30, None, CHW)}
    # mode 3: ragged phases with uncovered pixels (9 x 5 under a 4 x 2 kernel of stride 2; 7 x 8 under 3 x 6 of stride 3), one even
    m3 = {64: (Layer(64, 9, 5, 8, 4, 2, S=2), 12), 32: (Layer(32, 6, 8, 8, 2, 4, S=2), 14), 16: (Layer(16, 7, 8, 8, 3, 6, S=3), 30)}
    # mode 5: a 2 x 3 image (every pixel touches the padding), IW = 1 with ReLU on load, 4 x 5
    m5 = {64: (Layer(16, 2, 3, 64, 3, 3, same=True), 30, None, 0), 32: (Layer(16, 5, 1, 32, 3, 3, same=True), 36, 177, 1),
          16: (Layer(16, 4, 5, 16, 3, 3, same=True), 15, None, 0)}
    # mode 6: K = 27 -> 32 (HWC), 18 -> 32 (CHW bytes, IC = 2, stride 2, spare bytes), 36 -> 48 (channel-first IC = 4, a 2 x 3 image)
    m6 = {64: (Layer(3, 4, 3, 64, 3, 3, same=True), 15, None, HWC), 32: (Layer(2, 3, 5, 32, 3, 3, same=True), 12, 178, Bytes('chw', 2, 5)),
          16: (Layer(4, 2, 3, 16, 3, 3, same=True), 47, None, CHW)}
    for tn, kernel in ((64, FP32_128x64), (32, FP32_128x32), (16, FP32_256x16)):
        name = f'{kernel[1]}x{kernel[2]}'
        L, n, M = m1[tn]
        add(f'm1-{name}', IM2COL_F32, kernel, L, n, M=M)
        L, n, M = m2[tn]
        add(f'm2-{name}', IM2COL_U8, kernel, L, n, M=M)
        L, n = m3[tn]
        add(f'm3-{name}', COL2IM, kernel, L, n, kind='dx')
        L, n, M, b = m4[tn]
        add(f'm4-{name}', IM2COL_U8S, kernel, L, n, M=M, bytes=b)
        L, n, M, relu = m5[tn]
        add(f'm5-{name}', IM2COL_PAD, kernel, L, n, M=M, relu_in=relu)
        L, n, M, b = m6[tn]
        add(f'm6-{name}', IM2COL_U8P, kernel, L, n, M=M, bytes=b)
    # the six-term kernels: per-phase contractions of 32 and 64 only (tests/test_conv_gemm_reference_cpu.py: beyond 64 the bound does
    # not reliably see a lost term)
    add('bf16x6-m1-128x64-K32', IM2COL_F32, BF16_128x64, Layer(8, 6, 5, 64, 2, 2), 11, products=1)
    add('bf16x6-m1-128x32-K64', IM2COL_F32, BF16_128x32, Layer(8, 9, 6, 32, 4, 2, S=2), 20, M=175, products=1)
    add('bf16x6-m2-128x64-K32', IM2COL_U8, BF16_128x64, Layer(2, 12, 16, 64, 4, 4, S=4), 15, products=1)
    add('bf16x6-m2-128x32-K64', IM2COL_U8, BF16_128x32, Layer(2, 8, 16, 32, 4, 8, S=4), 30, M=178, products=1)
    add('bf16x6-m3-128x64-K32', COL2IM, BF16_128x64, Layer(64, 9, 7, 8, 4, 4, S=2), 9, kind='dx', products=1)
    add('bf16x6-m3-128x32-K64', COL2IM, BF16_128x32, Layer(32, 7, 6, 16, 4, 4, S=2), 15, kind='dx', products=1)
    add('bf16x6-m4-128x64-K32', IM2COL_U8S, BF16_128x64, Layer(4, 7, 9, 64, 2, 4, S=2), 20, products=1, bytes=HWC)
    add('bf16x6-m4-128x32-K64', IM2COL_U8S, BF16_128x32, Layer(1, 11, 10, 32, 8, 8), 15, M=178, products=1, bytes=Bytes('chw', 2, 3))
    # products = 1 where the six-term kernels do not apply: a per-phase contraction of 48, a 16-column tile, modes 5 and 6
    add('bf16x6-asks-m1-K48', IM2COL_F32, FP32_128x64, m1[64][0], 11, products=1)
    add('bf16x6-asks-m3-K48', COL2IM, FP32_128x32, Layer(32, 6, 7, 12, 4, 4, S=2), 15, kind='dx', products=1)
    add('bf16x6-asks-m2-256x16', IM2COL_U8, FP32_256x16, Layer(2, 10, 12, 16, 4, 4, S=4), 50, products=1)
    add('bf16x6-asks-m5', IM2COL_PAD, FP32_128x64, Layer(32, 3, 4, 64, 1, 1, same=True), 15, products=1)
    add('bf16x6-asks-m6', IM2COL_U8P, FP32_128x32, m6[32][0], 12, products=1, bytes=m6[32][3])
    # >= 9 row tiles: the XCD permutation deals two tiles to a workgroup column
    add('grid-m1', IM2COL_F32, FP32_128x64, m1[64][0], 60)
    add('grid-m5', IM2COL_PAD, FP32_128x64, Layer(16, 4, 5, 64, 3, 3, same=True), 60)
    add('grid-m3', COL2IM, FP32_128x64, m3[64][0], 80, kind='dx')
    # mode 5 under every epilogue (0, 1, 2, 4, 5 forward; 3 and 6 as dX against the flipped kernel), M inside a frame; a 5 x 5 kernel
    L = Layer(16, 3, 4, 32, 3, 3, same=True)
    for epi, name in ((EPI_NONE, 'none'), (EPI_BIAS, 'bias'), (EPI_BIAS_RELU, 'bias-relu'), (EPI_BIAS_ADD, 'bias-add'),
                      (EPI_BIAS_ADD_RELU, 'bias-add-relu')):
        add(f'm5-epi-{name}', IM2COL_PAD, FP32_128x32, L, 15, M=170, epi=epi, relu_in=epi == EPI_BIAS_ADD)
    Lx = Layer(32, 3, 4, 16, 3, 3, same=True)
    add('m5-dx-mask', IM2COL_PAD, FP32_128x32, Lx, 15, kind='dx', M=170, epi=EPI_MASK)
    add('m5-dx-mask-add', IM2COL_PAD, FP32_128x32, Lx, 15, kind='dx', M=170, epi=EPI_MASK_ADD)
    add('m5-k5', IM2COL_PAD, FP32_256x16, Layer(16, 3, 2, 16, 5, 5, same=True), 45)
    # mode 6 with the residual epilogues, IC = 1 (K = 9 -> 16)
    add('m6-epi-bias-add', IM2COL_U8P, FP32_128x32, Layer(1, 4, 3, 32, 3, 3, same=True), 15, epi=EPI_BIAS_ADD, bytes=HWC)
    add('m6-epi-bias-add-relu', IM2COL_U8P, FP32_128x64, Layer(1, 3, 5, 64, 3, 3, same=True), 12, M=178, epi=EPI_BIAS_ADD_RELU,
        bytes=Bytes('chw', 1, 3))
    assert len({x.tag for x in c}) == len(c)
    return c


def weight_cases():
    """Modes 1, 2, 4, 5, 6 at every tile height their K reaches (plan heights 64 / 128 / 192 / 256 by K <= 64 / 128 / 192 / 256), widths 64 /
    32 / 16 each at least once per mode, ~200 rows (one split) except one case of 600 rows per mode: three splits of 208 rows whose
    boundaries fall inside a frame.  Small OW and OH OW: the row cursor carries several times per 16-row advance."""
    c = []

    def add(tag, mode, kernel, layer, M, perm, **kw):
        c.append(ConvWeights(tag, mode, kernel, layer, M, perm, seed=2000 + len(c), **kw))

    add('m1-k64-K16', IM2COL_F32, (64, 64), Layer(4, 6, 5, 64, 2, 2), 200, 2)
    add('m1-k128-K96', IM2COL_F32, (32, 128), Layer(8, 10, 7, 32, 4, 3, S=2), 600, 2)
    add('m1-k192-K144-accumulate', IM2COL_F32, (16, 192), Layer(12, 5, 6, 16, 4, 3), 190, 2, accumulate=1)
    add('m1-k256-K240', IM2COL_F32, (64, 256), Layer(20, 5, 4, 64, 4, 3), 203, 2)
    add('m2-k64-K16', IM2COL_U8, (32, 64), Layer(1, 12, 16, 32, 4, 4, S=4), 200, 3)
    add('m2-k128-K120', IM2COL_U8, (64, 128), Layer(3, 13, 12, 64, 5, 8, S=4), 600, 3)
    add('m2-k192-K160-nobias', IM2COL_U8, (16, 192), Layer(4, 9, 16, 16, 5, 8, S=4), 201, 3, with_bias=False)
    add('m2-k256-K256', IM2COL_U8, (32, 256), Layer(4, 12, 12, 32, 8, 8, S=4), 199, 3)
    add('m4-k64-K16', IM2COL_U8S, (64, 64), Layer(4, 7, 9, 64, 2, 2, S=2), 200, 5, bytes=HWC)
    add('m4-k64-K48', IM2COL_U8S, (16, 64), Layer(3, 6, 7, 16, 4, 4), 600, 5, bytes=HWC)
    add('m4-k128-K96', IM2COL_U8S, (32, 128), Layer(2, 8, 9, 32, 6, 8), 203, 5, bytes=Bytes('chw', 2, 7))
    add('m4-k192-K144', IM2COL_U8S, (16, 192), Layer(3, 7, 10, 16, 6, 8), 197, 5, bytes=Bytes('hwc', 1, 2))
    add('m4-k256-K256', IM2COL_U8S, (64, 256), Layer(4, 9, 10, 64, 8, 8), 200, 5, bytes=HWC)
    add('m5-k64-K36', IM2COL_PAD, (32, 64), Layer(4, 3, 4, 32, 3, 3, same=True), 200, 2)
    add('m5-k128-K108-relu', IM2COL_PAD, (64, 128), Layer(12, 5, 1, 64, 3, 3, same=True), 600, 2, relu_in=1)
    add('m5-k192-K180', IM2COL_PAD, (16, 192), Layer(20, 2, 3, 16, 3, 3, same=True), 200, 2)
    add('m5-k256-K252', IM2COL_PAD, (32, 256), Layer(28, 4, 5, 32, 3, 3, same=True), 190, 2)
    add('m6-k64-K27', IM2COL_U8P, (64, 64), Layer(3, 4, 3, 64, 3, 3, same=True), 600, 5, bytes=HWC)
    add('m6-k64-K9', IM2COL_U8P, (16, 64), Layer(1, 3, 5, 16, 3, 3, same=True), 200, 5, bytes=Bytes('chw', 2, 5))
    add('m6-k64-K18', IM2COL_U8P, (32, 64), Layer(2, 2, 2, 32, 3, 3, same=True), 201, 5, bytes=CHW)
    add('m6-k64-K36', IM2COL_U8P, (32, 64), Layer(4, 5, 3, 32, 3, 3, same=True), 200, 5, bytes=CHW)
    add('m6-k128-K75', IM2COL_U8P, (16, 128), Layer(3, 4, 5, 16, 5, 5, same=True), 190, 5, bytes=HWC)
    add('m6-k192-K147', IM2COL_U8P, (32, 192), Layer(3, 5, 4, 32, 7, 7, same=True), 200, 5, bytes=HWC)
    add('m6-k256-K196', IM2COL_U8P, (64, 256), Layer(4, 3, 4, 64, 7, 7, same=True), 198, 5, bytes=HWC)
    c.append(DenseFlatten('dense-perm4-K24', (32, 64), 4, 3, 2, 32, 200, seed=2000 + len(c)))
    assert len({x.tag for x in c}) == len(c)
    return c
