"""The fused PPO gradient kernels against a float64 gradient of the same minibatch step (tests/ppo_grad_reference.py), one launch per
case: pfa_ppo_mlp_grad at every entry of its shape table (fp32 MFMA chains and the opt-in bf16x6 product form), pfa_ppo_wide_grad at the
widths and grids the trainer runs it on, pfa_lstm_heads_loss on random hidden states.  Everything else in the suite reaches these
gradients only through clipping and Adam, which divide a gradient by its own running magnitude: a gradient wrong by a constant
factor moves the weights almost exactly as a correct one does.  Here, per tensor, max |device - f64| <= max(4 e32, 1e-5 max |f64|),
e32 being what the restatement's own fp32 run loses against float64 on that case — a bound taken from the reference, not the kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_grad_reference as R

pytestmark = pytest.mark.gpu

_refs = {}


def _reference(case):
    """The float64 / fp32 reference of a case, computed once (on the CPU) and left unchanged."""
    if case.tag not in _refs:
        torch.set_num_threads(4)
        _refs[case.tag] = R.Reference(case)
    return _refs[case.tag]


def _ids(cases):
    return [pytest.param(c, id=c.tag) for c in cases]


class _Device:
    """The experience buffers of a case on the device and the structs the entry points read."""

    def __init__(self, case):
        from pufferlib_amd import _lib
        self.L, self.case = _lib.lib(), case
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()     # noqa: E731
        B = case.B
        self.bufs = (dev(case.obs), dev(case.packed_actions()), dev(case.logprobs), dev(case.values), torch.zeros(B, device='cuda'),
                     torch.zeros(B, device='cuda'), dev(case.advantages), dev(case.returns))
        assert self.bufs[0].shape == (B, case.stride) and all(t.shape[0] == B and t.element_size() == 4 for t in self.bufs)
        self.exp = _lib.Experience(*(t.data_ptr() for t in self.bufs), case.horizon)
        self.hp = _lib.PpoHparams(case.clip_coef, case.vf_clip_coef, case.vf_coef, case.ent_coef, case.norm_adv, case.clip_vloss, case.nmb,
                                  case.horizon)
        self.stats = dev(case.adv_stats())              # the true f64 (sum, sum of squares) of every minibatch's advantages
        assert self.stats.dtype == torch.float64 and self.stats.shape == (case.nmb, 2)
        self.dims = _lib.MlpDims(case.obs_dim, case.stride, case.hidden, case.actions, case.heads)

    def mlp_grad(self):
        """pfa_ppo_mlp_grad into a NaN-filled gradient buffer: (return code, flat gradient, 16-float tail)."""
        case, L = self.case, self.L
        self.params = torch.as_tensor(case.flat_params()).cuda()
        P = self.params.numel()
        self.grads = torch.full((P + 16,), float('nan'), device='cuda')
        self.ws = torch.zeros(L.pfa_ppo_workspace_bytes(C.byref(self.dims), case.B, C.byref(self.hp)), dtype=torch.uint8, device='cuda')
        rc = L.pfa_ppo_mlp_grad(C.byref(self.exp), case.B, case.mb, self.params.data_ptr(), C.byref(self.dims), C.byref(self.hp),
                                self.stats.data_ptr(), case.rows, self.grads.data_ptr(), self.ws.data_ptr(), None)
        torch.cuda.synchronize()
        g = self.grads.cpu().numpy()
        return rc, g[:P], g[P:]


def _check_mlp(case):
    from pufferlib_amd import _lib
    ref = _reference(case)
    rc, flat, tail = _Device(case).mlp_grad()
    _lib.check(rc, 'ppo_mlp_grad')
    got = case.split_flat(flat)
    bad = ref.failures(got)
    assert bad == [], f'{case.tag}: {bad} beyond max(4 e32, 1e-5 max|f64|) of the float64 gradient (figures printed above)'
    pad = got['encoder.weight'][:, case.obs_dim:]
    assert np.array_equal(pad.view(np.uint32), np.zeros(pad.shape, np.uint32)), 'W1\'s padding columns must be exactly 0'
    ref.check_sums(tail)


@pytest.mark.parametrize('case', _ids(R.mlp_cases()))
def test_mlp_grad_matches_the_float64_gradient(case):
    """Every GradShape of with_grad_shape (csrc/ppo_update.hip): row strides 16 / 32 / 96 / 128 behind one Discrete head and behind
    MultiDiscrete heads, stride 64 behind MultiDiscrete heads, the 7x7 grid with permuted (8, 11 actions) and natural (12, 15) head
    rows, 13 quads untrimmed (obs_dim 50), generic (60) — on one workgroup of tiles, and on three as minibatch 1 of 2 with segments of 4
    rows; tiles that leave wavefront pairs idle; norm_adv off; clip_vloss off."""
    from pufferlib_amd import _lib
    assert _lib.lib().pfa_ppo_mlp_grad_path(C.byref(_lib.MlpDims(case.obs_dim, case.stride, 128, case.actions, case.heads)), case.rows) == 0
    _check_mlp(case)


@pytest.mark.parametrize('case', _ids(R.bf16_cases()))
def test_mlp_grad_bf16x6_matches_the_float64_gradient(case):
    """The opt-in product form (six bf16 partial products per fp32 product, csrc/ppo_bf16.hpp) on the two 7x7 shapes, minibatches of
    whole 32-row tiles: the same bound."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    _reference(case)
    try:
        _lib.check(L.pfa_igemm_set_products(1), 'set_products')
        assert L.pfa_ppo_mlp_grad_path(C.byref(_lib.MlpDims(case.obs_dim, case.stride, 128, case.actions, case.heads)), case.rows) == 1
        _check_mlp(case)
    finally:
        _lib.check(L.pfa_igemm_set_products(0), 'set_products')


def test_mlp_grad_refuses_a_minibatch_that_is_no_multiple_of_16():
    """The entry point tiles minibatches in 16-row blocks and says so: 40 rows are refused before anything is launched, the gradient
    buffer stays as it was (the trainer sends such minibatches of a 128-wide policy through the GEMM path)."""
    from pufferlib_amd import _lib
    case = R.Case('40rows', 49, 64, 8, 0, rows=40, nmb=2, mb=1, horizon=8, seed=1)
    rc, flat, tail = _Device(case).mlp_grad()
    assert rc != 0 and b'multiple of 16' in _lib.lib().pfa_last_error()
    assert np.isnan(flat).all() and np.isnan(tail).all()


@pytest.mark.parametrize('case', _ids(R.wide_cases()))
def test_wide_grad_matches_the_float64_gradient(case):
    """pfa_ppo_wide_grad (csrc/ppo_wide.hip) at the (hidden, grid) pairs test_wide_default_policy_rollout_and_update_vs_oracle trains:
    torch-shaped tensors through a view, 16 and 48 rows per minibatch, minibatch 1 of 2."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    ref = _reference(case)
    d = _Device(case)
    flat = torch.as_tensor(case.flat_params(padded=False)).cuda()
    count = flat.numel()
    grads = torch.full((count + 16,), float('nan'), device='cuda')
    sizes = [v.size for v in case.split_flat(np.zeros(count, np.float32), padded=False).values()]

    def view(base):
        ptrs = [base.data_ptr() + 4 * int(o) for o in np.cumsum([0] + sizes[:-1])]
        return _lib.MlpView(ptrs[0], case.obs_dim, case.obs_dim, case.stride, case.hidden, case.actions, 0, *ptrs[1:])
    pv, gv = view(flat), view(grads)
    assert L.pfa_ppo_wide_supported(C.byref(pv)) == 1
    ws = torch.zeros(int(L.pfa_ppo_wide_workspace_bytes(C.byref(pv))), dtype=torch.uint8, device='cuda')
    _lib.check(L.pfa_ppo_wide_grad(C.byref(d.exp), case.B, case.mb, C.byref(pv), C.byref(gv), grads.data_ptr() + 4 * count, C.byref(d.hp),
                                   d.stats.data_ptr(), case.rows, ws.data_ptr(), None), 'ppo_wide_grad')
    torch.cuda.synchronize()
    g = grads.cpu().numpy()
    got = case.split_flat(g[:count], padded=False)
    got['encoder.weight'] = np.pad(got['encoder.weight'], ((0, 0), (0, case.stride - case.obs_dim)))
    bad = ref.failures(got)
    assert bad == [], f'{case.tag}: {bad} beyond max(4 e32, 1e-5 max|f64|) of the float64 gradient (figures printed above)'
    ref.check_sums(g[count:])


@pytest.mark.parametrize('case', _ids(R.heads_cases()))
def test_lstm_heads_loss_matches_the_float64_gradient(case):
    """pfa_lstm_heads_loss (csrc/lstm.hip: decode_actions + the PPO loss on the recurrent layer's time-major hidden states) on random h:
    d loss / d h, the head-bias gradients, the loss sums — and dout through the two products autograd would make of it (dout^T h =
    the gradients of decoder.weight and value_head.weight, formed here in float64).  70 rows: the last tile is ragged."""
    from pufferlib_amd import _lib
    L = _lib.lib()
    ref = _reference(case)
    d = _Device(case)
    A, H, rows = case.actions, case.hidden, case.rows
    params = torch.as_tensor(case.flat_params()).cuda()
    h = torch.as_tensor(case.h).cuda()
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')     # noqa: E731
    dout, dh, sums, bias16 = nan(rows, 16), nan(rows, H), nan(16), nan(16)
    ws = torch.zeros(int(L.pfa_lstm_heads_loss_workspace_bytes()), dtype=torch.uint8, device='cuda')
    _lib.check(L.pfa_lstm_heads_loss(h.data_ptr(), C.byref(d.exp), case.B, case.mb, params.data_ptr(), C.byref(d.dims), C.byref(d.hp),
                                     d.stats.data_ptr(), rows, dout.data_ptr(), dh.data_ptr(), sums.data_ptr(), bias16.data_ptr(),
                                     ws.data_ptr(), None), 'lstm_heads_loss')
    torch.cuda.synchronize()
    dout64, bias = dout.cpu().numpy().astype(np.float64), bias16.cpu().numpy()
    h64 = case.h.astype(np.float64)
    got = {'dh': dh.cpu().numpy(), 'decoder.bias': bias[:A], 'value_head.bias': bias[A:A + 1],
           'decoder.weight': dout64[:, :A].T @ h64, 'value_head.weight': dout64[:, A:A + 1].T @ h64}
    bad = ref.failures(got, names=tuple(got))
    assert bad == [], f'{case.tag}: {bad} beyond max(4 e32, 1e-5 max|f64|) of the float64 gradient (figures printed above)'
    assert not dout64[:, A + 1:].any(), 'the padding outputs carry no gradient'
    ref.check_sums(sums.cpu().numpy())
