"""The hand-off of the workgroup partials between the two launches of a PPO optimizer step (csrc/ppo_update.hip): the gradient
kernel's epilogue stores one partial per workgroup in 16-byte pieces, the reduce kernel loads them back in 16-byte pieces, four
native slots per lane.  Neither may change a bit of the result: the sum per native slot has a documented order (16 slices of the
partial index, sequential inside a slice, then a halving tree), restated here in numpy float32 from the partials themselves."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, OUT, NSTATS, MT, SLICES = 128, 16, 8, 8, 16

# (obs_dim, obs_stride, num_actions, heads, tiles per workgroup): the gradient shapes under test
SHAPE_7X7 = (49, 64, 8, 0, 4)         # GradShape<64, 13, false, 3, true, true>: trimmed dW1 + the column-48 slots, permuted head rows
SHAPE_MULTI = (12, 16, 5, 0x23, 4)    # obs_stride 16 behind a MultiDiscrete([3, 2]) head: untrimmed layout
SHAPE_WIDE = (100, 128, 6, 0, 2)      # 128-float rows: two wavefront pairs, the two-buffer epilogue
# the remaining reduce layouts (DP, KTM, COL, PERM) of with_grad_shape; every obs_dim leaves padding columns to be zeroed
SHAPE_32 = (30, 32, 4, 0, 4)          # <32, 2, false, false>
SHAPE_96 = (90, 96, 7, 0, 2)          # <96, 6, false, false>: two wavefront pairs
SHAPE_64 = (60, 64, 6, 0, 4)          # <64, 4, false, false>: 64-float rows, untrimmed
SHAPE_7X7_NATURAL = (49, 64, 13, 0, 4)   # <64, 3, true, false>: more than 11 actions keep the head rows in natural order
ALL_LAYOUTS = ((SHAPE_7X7, '7x7-perm'), (SHAPE_MULTI, 'stride16-multidiscrete'), (SHAPE_WIDE, 'stride128-two-buffers'), (SHAPE_32, 'stride32'),
               (SHAPE_96, 'stride96'), (SHAPE_64, 'stride64-untrimmed'), (SHAPE_7X7_NATURAL, '7x7-natural'))


def _layout(obs_dim, dp, a, heads):
    """NativeLayout of the shape with_grad_shape picks for these dimensions, and slot -> flat parameter index (-1: no parameter;
    `zero`: a slot that carries observation padding, whose gradient is written as 0)."""
    ktm, col, perm = dp // 16, False, False
    if dp == 64 and heads == 0 and obs_dim == 49:
        ktm, col, perm = 3, True, a <= 11
    k_col = ktm * MT * 4 * 64
    k_dw2 = k_col + (H if col else 0)
    k_db1 = k_dw2 + MT * 4 * 64
    k_db2 = k_db1 + H
    k_stats = k_db2 + OUT
    count = k_stats + NSTATS
    w1, b1 = 0, H * dp
    w2 = b1 + H
    b2 = w2 + a * H
    wv = b2 + a
    bv = wv + H
    nparams = bv + 1

    def output(slot):
        if not perm:
            return slot
        return 99 if (slot & 3) == 3 else 3 * (slot >> 2) + (slot & 3)
    p = np.full(count, -1, dtype=np.int64)
    zero = np.zeros(count, dtype=bool)
    for q in range(k_stats):
        if q < k_col:
            ln, r, m, kt = q & 63, (q >> 6) & 3, (q >> 8) & (MT - 1), q >> 11
            k = 16 * kt + 4 * (ln >> 4) + r
            p[q] = w1 + (16 * m + (ln & 15)) * dp + k
            zero[q] = k >= obs_dim
        elif q < k_dw2:
            p[q] = w1 + (q - k_col) * dp + 16 * ktm
            zero[q] = 16 * ktm >= obs_dim
        elif q < k_db1:
            t = q - k_dw2
            ln, r, m = t & 63, (t >> 6) & 3, t >> 8
            o, u = output(ln & 15), 16 * m + 4 * (ln >> 4) + r
            if o < a:
                p[q] = w2 + o * H + u
            elif o == a:
                p[q] = wv + u
        elif q < k_db2:
            p[q] = b1 + (q - k_db1)
        else:
            o = output(q - k_db2)
            if o < a:
                p[q] = b2 + o
            elif o == a:
                p[q] = bv
    first_pad = 16 * ktm + (1 if col else 0)
    return dict(count=count, stats=k_stats, nparams=nparams, slot_param=p, slot_zero=zero, first_pad=first_pad)


def _fixed_order_sum(partials):
    """[nparts][count] float32 -> the per-slot sum in the kernels' order, and the f64 sums of the same slices."""
    nparts, count = partials.shape
    assert nparts <= 16 * SLICES
    padded = np.zeros((16 * SLICES, count), dtype=np.float32)
    padded[:nparts] = partials
    by_slice = padded.reshape(16, SLICES, count)            # [u][slice]: partial index = slice + 16 u
    acc = np.zeros((SLICES, count), dtype=np.float32)
    dacc = np.zeros((SLICES, count), dtype=np.float64)
    for u in range(16):                                     # sequential inside a slice
        acc = (acc + by_slice[u]).astype(np.float32)
        dacc = dacc + by_slice[u].astype(np.float64)
    t = acc.copy()
    w = SLICES // 2
    while w > 0:                                            # the halving tree over the slices
        t[:w] = (t[:w] + t[w:2 * w]).astype(np.float32)
        w //= 2
    d = np.zeros(count, dtype=np.float64)
    for s in range(SLICES):
        d = d + dacc[s]
    return t[0], d


class _Case:
    def __init__(self, shape, rows, nmb=1, seed=0):
        from pufferlib_amd import _lib
        obs_dim, dp, a, heads, _ = shape
        self.L = _lib.lib()
        self.lay = _layout(obs_dim, dp, a, heads)
        self.rows, self.nmb, self.dp, self.obs_dim = rows, nmb, dp, obs_dim
        dev = 'cuda'
        g = torch.Generator(device=dev).manual_seed(seed)
        B = rows * nmb
        self.B = B
        obs = torch.randn(B, dp, device=dev, generator=g)
        obs[:, obs_dim:] = 0
        if heads:
            actions = (torch.randint(0, 3, (B,), device=dev, dtype=torch.int32, generator=g)
                       | (torch.randint(0, 2, (B,), device=dev, dtype=torch.int32, generator=g) << 4))
        else:
            actions = torch.randint(0, a, (B,), device=dev, dtype=torch.int32, generator=g)
        self.bufs = (obs, actions, torch.full((B,), -1.5, device=dev), torch.randn(B, device=dev, generator=g),
                     torch.randn(B, device=dev, generator=g), torch.zeros(B, device=dev),
                     torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g))
        self.exp = _lib.Experience(*(t.data_ptr() for t in self.bufs), 16)
        self.dims = _lib.MlpDims(obs_dim, dp, H, a, heads)
        self.hp = _lib.PpoHparams(.1, .1, .5, .01, 1, 1, nmb, 16)
        P = self.lay['nparams']
        self.params = torch.randn(P, device=dev, generator=g) * 0.05
        self.params[:H * dp].view(H, dp)[:, obs_dim:] = 0
        self.m, self.v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
        self.grads = torch.full((P + 2 * NSTATS,), float('nan'), device=dev)
        self.losses = torch.zeros(8, dtype=torch.float64, device=dev)
        self.ws = torch.zeros(self.L.pfa_ppo_workspace_bytes(C.byref(self.dims), B, C.byref(self.hp)), dtype=torch.uint8, device=dev)
        self.stats = torch.tensor([[0.0, float(rows)]] * nmb, dtype=torch.float64, device=dev)   # (sum, sum of squares) of the advantages

    def grad(self):
        from pufferlib_amd import _lib
        _lib.check(self.L.pfa_ppo_mlp_grad(C.byref(self.exp), self.B, 0, self.params.data_ptr(), C.byref(self.dims), C.byref(self.hp),
                                           self.stats.data_ptr(), self.rows, self.grads.data_ptr(), self.ws.data_ptr(), None), 'grad')
        torch.cuda.synchronize()

    def train(self, epochs):
        from pufferlib_amd import _lib
        _lib.check(self.L.pfa_ppo_mlp_train(C.byref(self.exp), self.B, self.params.data_ptr(), C.byref(self.dims), C.byref(self.hp),
                                            self.stats.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), 0, 2.5e-3, .9,
                                            .999, 1e-5, .5, epochs, self.losses.data_ptr(), self.ws.data_ptr(), 0, None), 'train')
        torch.cuda.synchronize()


def _cases():
    out = []
    for shape, name in ((SHAPE_7X7, '7x7-perm'), (SHAPE_MULTI, 'stride16-multidiscrete')):
        for grid in (1, 3, 17, 256):
            out.append(pytest.param(shape, grid, id=f'{name}-grid{grid}'))
    for shape, name in ALL_LAYOUTS[2:]:
        for grid in (3, 17):
            out.append(pytest.param(shape, grid, id=f'{name}-grid{grid}'))
    return out


@pytest.mark.parametrize('shape,grid', _cases())
def test_flat_gradient_is_the_fixed_order_sum_of_the_partials(shape, grid):
    """pfa_ppo_mlp_grad leaves `grid` partials in the caller's workspace and their sum in the flat gradient: every native slot,
    recomputed in numpy float32 in the documented order and pushed through the slot-to-parameter map, must give the same bits;
    W1's padding columns, which no slot covers, must be exactly 0 whatever the gradient buffer held (NaN here)."""
    rows = 16 * shape[4] * grid      # whole workgroups of 16-row tiles: 64 / 192 / 1088 / 16384 rows on rows of up to 64 floats
    case = _Case(shape, rows)
    case.grad()
    lay = case.lay
    count, P = lay['count'], lay['nparams']
    partials = case.ws[:grid * count * 4].view(torch.float32).view(grid, count).cpu().numpy()
    assert np.isfinite(partials).all() and np.abs(partials[:, :lay['stats']]).max() > 0
    s, d = _fixed_order_sum(partials)
    want = np.full(P, np.nan, dtype=np.float32)
    w1 = want[:H * case.dp].reshape(H, case.dp)
    w1[:, lay['first_pad']:] = 0.0
    has = lay['slot_param'] >= 0
    want[lay['slot_param'][has]] = np.where(lay['slot_zero'][has], np.float32(0), s[has])
    assert not np.isnan(want).any(), 'the restated map must cover every parameter'
    got = case.grads.cpu().numpy()
    assert np.array_equal(got[:P].view(np.uint32), want.view(np.uint32)), int((got[:P].view(np.uint32) != want.view(np.uint32)).sum())
    got_w1 = got[:H * case.dp].reshape(H, case.dp)
    assert np.array_equal(got_w1[:, case.obs_dim:].view(np.uint32), np.zeros((H, case.dp - case.obs_dim), dtype=np.uint32))
    # the loss sums behind the gradient: f64 over the same slices, left as (hi, lo) float pairs
    dst = d[lay['stats']:]
    hi = dst.astype(np.float32)
    lo = (dst - hi.astype(np.float64)).astype(np.float32)
    tail = got[P:P + 2 * NSTATS]
    assert np.array_equal(tail[0::2].view(np.uint32), hi.view(np.uint32)) and np.array_equal(tail[1::2].view(np.uint32), lo.view(np.uint32))


@pytest.mark.parametrize('grid', [3, 17])
@pytest.mark.parametrize('shape', [pytest.param(shape, id=name) for shape, name in ALL_LAYOUTS])
def test_one_launch_form_equals_the_two_kernel_form_at_small_grids(monkeypatch, shape, grid):
    """Three optimizer steps through pfa_ppo_mlp_train in the one-launch form (ppo_reduce_adam_kernel through Adam) and in the
    two-kernel form (PFA_FUSED_ADAM=0: the same kernel's sums-only instantiation + adam_clip_kernel; the switch is read at every
    call): parameters, both moments and the loss sums must be the same bits at every reduce layout, with 3 and with 17 partials
    (the slice tail cuts inside a round of 16)."""
    rows = 16 * shape[4] * grid
    runs = []
    for fused in ('1', '0'):
        monkeypatch.setenv('PFA_FUSED_ADAM', fused)
        case = _Case(shape, rows, seed=3)
        case.train(3)
        runs.append([t.cpu().numpy() for t in (case.params, case.m, case.v, case.losses)])
    for name, x, y in zip(('parameters', 'exp_avg', 'exp_avg_sq', 'loss sums'), *runs):
        assert np.isfinite(x).all() and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    assert np.abs(runs[0][1]).max() > 0 and np.abs(runs[0][3][:2]).max() > 0
