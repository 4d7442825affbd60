"""lstm.Engine.update — the recurrent path's whole gradient — against a float64 gradient of the same minibatch step
(tests/lstm_grad_reference.py), and its glue kernels each on its own.  The golden replays reach this gradient only through clipping and
Adam, which divide it by its own running magnitude: a minibatch that starts from zero or stale state, a d b_hh never written or a dW_hh
taken against the wrong slot moves the weights almost as a correct update does.  Here, per tensor of the flat gradient and for the state
left for the next minibatch, max |device - f64| <= max(4 e32, 1e-5 max |f64|), e32 being what the restatement's own fp32 run loses on
that case — a bound taken from the reference, not the kernels.  Every buffer a call is to write holds NaN before it."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lstm_grad_reference as LR
import ppo_grad_reference as R

pytestmark = pytest.mark.gpu

H = 128
NAN = float('nan')
_refs = {}


def _reference(case):
    """The float64 / fp32 reference of a case, computed once (on the CPU) and left unchanged."""
    if case.tag not in _refs:
        torch.set_num_threads(4)
        _refs[case.tag] = LR.Reference(case)
    return _refs[case.tag]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan(*shape):
    return torch.full(shape, NAN, device='cuda')


def _policy(obs_dim, stride, actions, heads=0):
    """A RecurrentPolicy over a stub env of that observation size and action space, adopted at `stride`: (policy, FlatParams)."""
    from pufferlib_amd import cleanrl, models, namespace, spaces
    act = spaces.MultiDiscrete(R.head_sizes(actions, heads)) if heads else spaces.Discrete(actions)
    env = namespace(single_observation_space=spaces.Box(low=-1, high=1, shape=(obs_dim,), dtype=np.float32), single_action_space=act)
    pol = cleanrl.RecurrentPolicy(models.LSTMWrapper(env, models.Default(env)))
    return pol, pol.adopt(stride, 'cuda')


class _Engine:
    """lstm.Engine over the experience of a case, without a trainer."""

    def __init__(self, case):
        from pufferlib_amd import _lib, clean_pufferl, lstm
        self.case = case
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()     # noqa: E731
        self.pol, self.fp = _policy(case.obs_dim, case.stride, case.actions, case.heads)
        fp = self.fp
        flat = case.flat_params()
        assert flat.size == fp.count and fp.dims.heads == case.heads
        fp.flat.copy_(dev(flat))
        B, Th, M, n = case.B, case.horizon, case.rows, case.R * case.nmb
        self.exp = exp = clean_pufferl.Experience(B, Th, M, case.stride, n, 'cuda')
        assert exp.horizon == Th and exp.num_minibatches == case.nmb and exp.obs.shape == (B, case.stride)
        for dst, src in ((exp.obs, case.obs), (exp.actions, case.packed_actions()), (exp.logprobs, case.logprobs), (exp.values, case.values),
                         (exp.advantages, case.advantages), (exp.returns, case.returns)):
            dst.copy_(dev(src))
        self.eng = lstm.Engine(fp, exp, SimpleNamespace(num_agents=n))
        self.hp = _lib.PpoHparams(case.clip_coef, case.vf_clip_coef, case.vf_coef, case.ent_coef, case.norm_adv, case.clip_vloss, case.nmb, Th)
        self.stats = dev(case.adv_stats())              # the true f64 (sum, sum of squares) of every minibatch's advantages
        assert self.stats.dtype == torch.float64 and self.stats.shape == (case.nmb, 2)
        self.grads = _nan(fp.count + 16)

    def poison(self):
        """NaN into the gradient and into every engine buffer an update is to write — all but slot Th of Hs / Cs, which carries the state."""
        e, Th = self.eng, self.case.horizon
        self.grads.fill_(NAN)
        for t in [e.xe, e.gates, e.Hs[:Th], e.Cs[:Th], e.dout, e.dh_heads, e.dG, e.dxe, e.g16, e.bsum16, e.wpack, e.wpack_bwd] + e.obs_tm_all:
            t.fill_(NAN)
        for ws in e.gemm_ws + [e.bwd_ws]:
            ws.view(torch.float32).fill_(NAN)

    def update(self, m):
        self.poison()
        self.eng.update(m, self.hp, self.stats, self.case.rows, self.grads, self.case.B)
        torch.cuda.synchronize()
        return self.grads.clone()

    def sequence(self):
        """One epoch up to the case's minibatch from eng.state = None, then the first minibatch of the next epoch: (gradient of
        update(0), gradient of update(mb), Hs[Th], Cs[Th] after update(mb), gradient of the next epoch's update(0))."""
        e, Th = self.eng, self.case.horizon
        e.state = None
        out = [self.update(m) for m in range(self.case.mb + 1)]
        hT, cT = e.Hs[Th].clone(), e.Cs[Th].clone()
        e.state = None          # clean_pufferl.train at the top of an epoch; slot Th still holds minibatch mb's final state
        return out[0], out[-1], hT, cT, self.update(0)


@pytest.mark.parametrize('case', [pytest.param(c, id=c.tag) for c in LR.cases()])
def test_engine_update_matches_the_float64_gradient(case):
    """update(0) .. update(mb) under unchanged parameters: the last call's ten gradient tensors, loss sums and final state against
    float64; nothing relies on what a buffer held before; an epoch boundary ignores the stale state in slot Th; the whole sequence twice
    gives the same bits (every reduction of this path has a fixed order)."""
    ref = _reference(case)
    dev = _Engine(case)
    count = dev.fp.count
    g0, g, hT, cT, g0_next = dev.sequence()
    flat = g.cpu().numpy()
    assert np.isfinite(flat).all(), f'{case.tag}: {np.flatnonzero(~np.isfinite(flat))[:8]} of the gradient and its tail were not written'
    got = case.split_flat(flat[:count])
    got.update(h_final=hT.cpu().numpy(), c_final=cT.cpu().numpy())
    bad = ref.failures(got, names=LR.NAMES + LR.STATE)
    assert bad == [], f'{case.tag}: {bad} beyond max(4 e32, 1e-5 max|f64|) of the float64 reference (figures printed above)'
    assert (got['encoder.weight'][:, case.obs_dim:] == 0).all(), 'W1\'s padding columns carry no gradient'
    ref.check_sums(flat[count:], rows=case.rows)
    assert _same_bits(g0, g0_next), 'update(0) after eng.state = None must not see the state left in slot Th'
    again = dev.sequence()
    for a, b in zip((g0, g, hT, cT, g0_next), again):
        assert _same_bits(a, b), 'the update is deterministic: the same sequence gives the same bits'


# ------------------------------------------------------------------------------------------------------------ the pieces, each alone
def _seq_forward(fp, obs, Th, Rr, slot0, init_slot, last=None):
    """pfa_lstm_seq_forward into NaN-filled buffers with 32 guard rows behind each: slot 0 = `slot0` (None: NaN), slot Th = `last`."""
    from pufferlib_amd import _lib, lstm
    L = _lib.lib()
    G = 32
    xe, gates = _nan(Th * Rr + G, H), _nan(Th * Rr + G, 4 * H)
    Hs, Cs = _nan((Th + 1) * Rr + G, H), _nan((Th + 1) * Rr + G, H)
    if slot0 is not None:
        Hs[:Rr], Cs[:Rr] = slot0
    if last is not None:
        Hs[Th * Rr:(Th + 1) * Rr], Cs[Th * Rr:(Th + 1) * Rr] = last
    before = [t.clone() for t in (xe, gates, Hs, Cs)]
    wpack = lstm.pack_gates(fp)
    rc = L.pfa_lstm_seq_forward(_lib.ptr(obs), Rr, Th, _lib.ptr(fp.flat), C.byref(fp.dims), _lib.ptr(wpack), _lib.ptr(xe), _lib.ptr(gates),
                                _lib.ptr(Hs), _lib.ptr(Cs), init_slot, _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, (xe, gates, Hs, Cs), before


@pytest.mark.parametrize('Rr', [40, 64])
def test_lstm_seq_forward_moves_the_initial_state_into_slot_0(Rr):
    """init_slot = -1 (zero state) and init_slot = Th (the previous minibatch's final state), the two values update() passes: slot 0
    comes out as zeros / as the bits of slot Th, and everything kept for the backward pass equals bit for bit the init_slot = 0 run
    that had that state in slot 0.  No row past the buffers' ends is touched; init_slot = Th + 1 is refused."""
    from pufferlib_amd import _lib
    Th = 3
    torch.manual_seed(100 + Rr)
    _, fp = _policy(49, 64, 8)
    fp.flat.copy_(torch.randn(fp.count, device='cuda') * 0.1)
    obs = torch.zeros(Th * Rr, 64, device='cuda')
    obs[:, :49] = torch.randn(Th * Rr, 49, device='cuda')
    zero = (torch.zeros(Rr, H, device='cuda'), torch.zeros(Rr, H, device='cuda'))
    state = (0.3 * torch.randn(Rr, H, device='cuda'), 0.3 * torch.randn(Rr, H, device='cuda'))

    def guards_intact(bufs, before):
        ends = (Th * Rr, Th * Rr, (Th + 1) * Rr, (Th + 1) * Rr)
        return all(_same_bits(b[e:], w[e:]) for b, w, e in zip(bufs, before, ends))

    for s0, init_slot, last in ((zero, -1, None), (state, Th, state)):
        rc, want, before = _seq_forward(fp, obs, Th, Rr, s0, 0)
        _lib.check(rc, 'lstm_seq_forward')
        assert guards_intact(want, before) and all(torch.isfinite(t[:e]).all() for t, e in zip(want, (Th * Rr, Th * Rr, (Th + 1) * Rr, (Th + 1) * Rr)))
        rc, got, before = _seq_forward(fp, obs, Th, Rr, None, init_slot, last=last)
        _lib.check(rc, 'lstm_seq_forward')
        assert guards_intact(got, before)
        assert _same_bits(got[2][:Rr], s0[0]) and _same_bits(got[3][:Rr], s0[1]), 'slot 0 must hold the initial state'
        for name, a, b in zip(('xe', 'gates', 'Hs', 'Cs'), got, want):
            assert _same_bits(a, b), f'{name} differs from the init_slot = 0 run (init_slot {init_slot})'
    assert (want[2][Th * Rr:(Th + 1) * Rr] - state[0]).abs().max().item() > 1e-3      # slot Th was overwritten with a new state

    rc, got, before = _seq_forward(fp, obs, Th, Rr, None, Th + 1, last=state)
    assert rc != 0 and b'init_slot' in _lib.lib().pfa_last_error()
    assert all(_same_bits(a, b) for a, b in zip(got, before)), 'a refused call writes nothing'


def _partial_products(k, seed):
    """Operands of the four products of one reduce launch: three one-operand shapes and the two-operand form."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)      # noqa: E731
    one = [(rnd(k, 128 + 16)[:, :128], rnd(k, 64)), (rnd(k, 128), rnd(k, 160 + 32)[:, :160]), (rnd(k, 16), rnd(k, 128))]
    two = (rnd(k, 512), rnd(k, 128), rnd(k, 128 + 8)[:, :128])
    return one, two, rnd(3, 640)


@pytest.mark.parametrize('k', [37, 4099])
def test_partial_products_and_column_sums_finish_in_one_reduce_launch(k):
    """update()'s four-jobs-in-one-launch pattern with one job more: three pfa_gemm_tn_partial_f32 products (128 x 64, 128 x 160, 16 x 128),
    one pfa_gemm_tn2_partial_f32 (columns >= 128 to a second output) and a kind-1 column sum ([3][640], columns >= 512 to a second output)
    finished by ONE pfa_reduce_multi call: bit-identical to pfa_gemm_tn_f32 / pfa_gemm_tn2_f32 on the same operands (they share
    gemm_tn_reduce_block), within test_gemm_tn_matches_f64_contraction's bound of the float64 products, and nothing outside the
    outputs' own columns is written (ldc wider than the matrix, NaN around).  k = 37 is one split, 4099 several."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    st = _lib.stream_handle()
    one, two, colpart = _partial_products(k, 1000 + k)
    ws = lambda n: torch.empty(n, dtype=torch.uint8, device='cuda')     # noqa: E731
    jobs = (_lib.ReduceJob * 5)()
    keep, outs = [], []
    for q, (a, b) in enumerate(one):
        mo, no = a.shape[1], b.shape[1]
        w = ws(L.pfa_gemm_tn_workspace_bytes(mo, no, k))
        _lib.check(L.pfa_gemm_tn_partial_f32(_lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0), mo, no, k, _lib.ptr(w), C.byref(jobs[q]), st), 'partial')
        out = _nan(mo + 1, no + 8)
        jobs[q].c, jobs[q].ldc = out.data_ptr(), out.stride(0)
        keep.append(w), outs.append(out)
    assert (jobs[0].splits == 1) == (k == 37) and all(jobs[q].kind == 0 for q in range(3))
    a, b0, b1 = two
    w = ws(L.pfa_gemm_tn2_workspace_bytes(512, k))
    _lib.check(L.pfa_gemm_tn2_partial_f32(_lib.ptr(a), a.stride(0), _lib.ptr(b0), b0.stride(0), _lib.ptr(b1), b1.stride(0), 512, k, _lib.ptr(w),
                                          C.byref(jobs[3]), st), 'partial2')
    o0, o1 = _nan(513, 136), _nan(513, 160)
    jobs[3].c, jobs[3].ldc, jobs[3].c2, jobs[3].ldc2 = o0.data_ptr(), o0.stride(0), o1.data_ptr(), o1.stride(0)
    assert jobs[3].nb == 128 and jobs[3].no == 256
    keep.append(w)
    s0, s1 = _nan(512 + 8), _nan(128 + 8)
    jobs[4] = _lib.ReduceJob(1, 3, 1, 640, colpart.data_ptr(), s0.data_ptr(), 0, s1.data_ptr(), 0, 512, 0)
    _lib.check(L.pfa_reduce_multi(jobs, 5, st), 'reduce_multi')
    torch.cuda.synchronize()

    tol = 2e-6 * (k ** 0.5) * 4 + 1e-5          # test_gemm_tn_matches_f64_contraction's
    for (a, b), out in zip(one, outs):
        mo, no = a.shape[1], b.shape[1]
        want = torch.empty(mo, no, device='cuda')
        w = ws(L.pfa_gemm_tn_workspace_bytes(mo, no, k))
        _lib.check(L.pfa_gemm_tn_f32(_lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0), _lib.ptr(want), no, mo, no, k, _lib.ptr(w), st), 'gemm_tn')
        assert _same_bits(out[:mo, :no], want), f'{mo} x {no}: the partial + reduce_multi product differs from pfa_gemm_tn_f32'
        assert (out[:mo, :no].double() - a.double().t() @ b.double()).abs().max().item() <= tol
        assert torch.isnan(out[mo:]).all() and torch.isnan(out[:, no:]).all()
    a, b0, b1 = two
    w0, w1 = torch.empty(512, 128, device='cuda'), torch.empty(512, 128, device='cuda')
    w = ws(L.pfa_gemm_tn2_workspace_bytes(512, k))
    _lib.check(L.pfa_gemm_tn2_f32(_lib.ptr(a), a.stride(0), _lib.ptr(b0), b0.stride(0), _lib.ptr(b1), b1.stride(0), _lib.ptr(w0), 128, _lib.ptr(w1), 128,
                                  512, k, _lib.ptr(w), st), 'gemm_tn2')
    for out, want, b in ((o0, w0, b0), (o1, w1, b1)):
        assert _same_bits(out[:512, :128], want), 'the two-operand partial + reduce_multi product differs from pfa_gemm_tn2_f32'
        assert (out[:512, :128].double() - a.double().t() @ b.double()).abs().max().item() <= tol
        assert torch.isnan(out[512:]).all() and torch.isnan(out[:, 128:]).all()
    # column sums of three fp32 values: two roundings of at most 2^-24 of the running magnitude each
    csum, cabs = colpart.double().sum(0), colpart.double().abs().sum(0)
    got = torch.cat([s0[:512], s1[:128]]).double()
    assert ((got - csum).abs() <= 2 * 2.0 ** -24 * cabs).all()
    assert torch.isnan(s0[512:]).all() and torch.isnan(s1[128:]).all()


def test_reduce_multi_refuses_bad_job_lists_and_writes_nothing():
    """More jobs than a launch carries (6), none at all, and a kind-1 job whose columns >= nb have no second output."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    part, out = torch.randn(3, 640, device='cuda'), _nan(640)
    good = _lib.ReduceJob(1, 3, 1, 640, part.data_ptr(), out.data_ptr(), 0, 0, 0, 640, 0)
    seven = (_lib.ReduceJob * 7)(*([good] * 7))
    assert L.pfa_reduce_multi(seven, 7, _lib.stream_handle()) != 0 and b'reduce_multi' in L.pfa_last_error()
    assert L.pfa_reduce_multi(seven, 0, _lib.stream_handle()) != 0
    bad = (_lib.ReduceJob * 1)(_lib.ReduceJob(1, 3, 1, 640, part.data_ptr(), out.data_ptr(), 0, None, 0, 512, 0))
    assert L.pfa_reduce_multi(bad, 1, _lib.stream_handle()) != 0 and b'c2' in L.pfa_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    _lib.check(L.pfa_reduce_multi(seven, 6, _lib.stream_handle()), 'reduce_multi')       # six is the most, and runs
    torch.cuda.synchronize()
    assert torch.equal(out, (part[0] + part[1]) + part[2])      # colsum_reduce_block's order for three groups: quarter 0 alone


@pytest.mark.parametrize('stride', [16, 160])
def test_gather_obs_time_major_is_the_minibatch_row_map(stride):
    """pfa_gather_obs_time_major against Case.rows_index (time-major: row t R + k = segment mb + k nmb at step t) for every minibatch
    of three, R = 5 segments of 3 steps, the narrowest and the widest row; the rest of the destination is left alone."""
    from pufferlib_amd import _lib, clean_pufferl
    L = _lib.lib()
    Rr, Th, nmb = 5, 3, 3
    M, B = Rr * Th, Rr * Th * nmb
    case = R.Case('gather', 9, 16, 4, rows=M, nmb=nmb, horizon=Th, time_major=True, seed=1)
    exp = clean_pufferl.Experience(B, Th, M, stride, Rr * nmb, 'cuda')
    exp.obs.copy_(torch.randn(B, stride, generator=torch.Generator().manual_seed(stride)).cuda())
    hp = _lib.PpoHparams(0.1, 0.1, 0.5, 0.01, 1, 1, nmb, Th)
    for mb in range(nmb):
        out = _nan(M + 3, stride)
        _lib.check(L.pfa_gather_obs_time_major(C.byref(exp.c), B, mb, C.byref(hp), stride, _lib.ptr(out), _lib.stream_handle()), 'gather_obs')
        torch.cuda.synchronize()
        idx = torch.as_tensor(case.rows_index(mb)).cuda()
        assert _same_bits(out[:M], exp.obs[idx]), f'minibatch {mb}'
        assert torch.isnan(out[M:]).all()


@pytest.mark.parametrize('A', [5, 15])
def test_lstm_finish_grads_scatters_the_head_product_and_copies_the_gate_bias(A):
    """pfa_lstm_finish_grads on a NaN-filled flat vector whose b_ih block is known: exactly decoder.weight (rows < A of g16),
    value_head.weight (row A), their biases (bsum16) and b_hh (= b_ih) are written; rows and entries past A + 1 are never read into it."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    dp = 32
    torch.manual_seed(A)
    n_mlp = H * dp + H + A * H + A + H + 1
    count = n_mlp + 8 * H * H + 8 * H
    o_w2 = H * dp + H
    o_b2, o_wv, o_bv = o_w2 + A * H, o_w2 + A * H + A, o_w2 + A * H + A + H
    o_bih = n_mlp + 8 * H * H
    flat = _nan(count + 16)
    flat[o_bih:o_bih + 4 * H] = torch.randn(4 * H, device='cuda')
    g16, bsum16 = torch.randn(16, H, device='cuda'), torch.randn(16, device='cuda')
    g16[A + 1:], bsum16[A + 1:] = NAN, NAN
    want = flat.clone()
    want[o_w2:o_b2] = g16[:A].reshape(-1)
    want[o_b2:o_wv] = bsum16[:A]
    want[o_wv:o_bv] = g16[A]
    want[o_bv] = bsum16[A]
    want[o_bih + 4 * H:o_bih + 8 * H] = flat[o_bih:o_bih + 4 * H]
    assert o_bih + 8 * H == count and int(torch.isfinite(want).sum()) == (A + 1) * (H + 1) + 8 * H
    dims = _lib.MlpDims(dp - 3, dp, H, A, 0)
    _lib.check(L.pfa_lstm_finish_grads(_lib.ptr(flat), C.byref(dims), _lib.ptr(g16), _lib.ptr(bsum16), _lib.stream_handle()), 'finish_grads')
    torch.cuda.synchronize()
    assert _same_bits(flat, want)
    before = flat.clone()
    assert L.pfa_lstm_finish_grads(_lib.ptr(flat), C.byref(_lib.MlpDims(dp - 3, dp, H, 16, 0)), _lib.ptr(g16), _lib.ptr(bsum16),
                                   _lib.stream_handle()) != 0 and b'num_actions' in L.pfa_last_error()
    torch.cuda.synchronize()
    assert _same_bits(flat, before)


def test_lstm_pack_both_is_the_two_pack_kernels():
    """pfa_lstm_pack_both (one launch, every optimizer step) against pfa_lstm_pack and pfa_lstm_pack_bwd: both outputs bit for bit."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    st = _lib.stream_handle()
    torch.manual_seed(2)
    _, fp = _policy(90, 96, 6)
    fp.flat.copy_(torch.randn(fp.count, device='cuda'))
    n = L.pfa_lstm_pack_bytes() // 4
    fwd, bwd, both_f, both_b = _nan(n), _nan(n), _nan(n), _nan(n)
    _lib.check(L.pfa_lstm_pack(_lib.ptr(fp.flat), C.byref(fp.dims), _lib.ptr(fwd), st), 'lstm_pack')
    _lib.check(L.pfa_lstm_pack_bwd(_lib.ptr(fp.flat), C.byref(fp.dims), _lib.ptr(bwd), st), 'lstm_pack_bwd')
    _lib.check(L.pfa_lstm_pack_both(_lib.ptr(fp.flat), C.byref(fp.dims), _lib.ptr(both_f), _lib.ptr(both_b), st), 'lstm_pack_both')
    torch.cuda.synchronize()
    assert torch.isfinite(fwd).all() and torch.isfinite(bwd).all() and not _same_bits(fwd, bwd)
    assert _same_bits(both_f, fwd) and _same_bits(both_b, bwd)
