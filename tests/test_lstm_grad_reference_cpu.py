"""tests/lstm_grad_reference.py on the CPU — what tests/test_gpu_lstm_grad_f64.py stands on: the committed recurrent cases are clear
of the loss's kinks at their committed seeds, the restated cell is torch.nn.LSTM, and the comparison's bound rejects four mistakes a
recurrent update can make (each a one-line switch of the restatement) while it accepts the restatement's own fp32 run."""
import numpy as np
import pytest
import torch

import lstm_grad_reference as LR


@pytest.fixture(scope='module')
def references():
    torch.set_num_threads(4)
    return [LR.Reference(c, check=False) for c in LR.cases()]


def test_case_table_names_every_stride_and_both_row_kinds():
    """All six instantiations of lstm_seq_fwd_kernel<DP>; R ragged and R a multiple of the 32-row workgroup (the two backward kernels);
    the state carried, carried twice and zero; one step and sixteen; the committed seed is the first of 1, 2, 3, ... (checked below)."""
    rows = {tag: (dp, r, th, nmb, mb) for tag, _, dp, _, _, r, th, nmb, mb, _ in LR.SHAPES}
    assert len(rows) == len(LR.SHAPES) == 11
    assert {dp for dp, *_ in rows.values()} == {16, 32, 64, 96, 128, 160}
    assert any(r % 32 for _, r, *_ in rows.values()) and any(r % 32 == 0 for _, r, *_ in rows.values())
    assert any(r < 32 for _, r, *_ in rows.values()) and any(r >= 96 for _, r, *_ in rows.values())
    assert {mb for *_, mb in rows.values()} == {0, 1, 2} and {th for _, _, th, _, _ in rows.values()} >= {1, 16}
    assert all(1 <= LR.SEEDS.get(tag, 1) for tag in rows) and set(LR.SEEDS) <= set(rows)


def test_committed_seeds_keep_their_margins_and_are_the_first_that_do(references):
    for ref in references:
        c = ref.case
        ref.check_margins()
        assert c.seed == LR.SEEDS.get(c.tag[len('lstm-'):], 1)
        for seed in range(1, c.seed):       # no earlier seed would have done
            kw = dict(norm_adv=c.norm_adv, clip_vloss=c.clip_vloss)
            earlier = LR.Case(c.tag, c.obs_dim, c.stride, c.actions, c.heads, c.R, c.horizon, c.nmb, c.mb, seed=seed, **kw)
            assert not LR.Reference(earlier, check=False).margins_ok(), (c.tag, seed)
        assert 0 < ref.sums[5] < c.rows, f'{c.tag}: some ratios must be clipped and some not'
        w1 = ref.grads['encoder.weight']
        assert np.abs(w1[:, :c.obs_dim]).max(axis=0).min() > 0 and not w1[:, c.obs_dim:].any()     # every live column, no pad column
        assert all(np.abs(ref.grads[k]).max() > 0 for k in LR.NAMES)
        p = c.params
        assert np.abs(p['recurrent.bias_ih_l0']).min() > 0 and np.abs(p['recurrent.bias_hh_l0']).min() > 0
        assert not np.array_equal(p['recurrent.bias_ih_l0'], p['recurrent.bias_hh_l0'])
        # d b_hh = d b_ih and dW_hh = sum_t dG_t^T h_{t-1}: what pfa_lstm_finish_grads and the two-operand product rely on
        assert np.array_equal(ref.grads['recurrent.bias_hh_l0'], ref.grads['recurrent.bias_ih_l0'])
        hh = ref.grads['recurrent.weight_hh_l0']
        assert np.abs(ref.r64['dwhh_by_hand'] - hh).max() <= 1e-12 * np.abs(hh).max()
        if c.mb:
            h0 = LR.carried_state(c, {k: torch.as_tensor(v).double() for k, v in p.items()}, c.mb, torch.float64)[0]
            assert h0.abs().max().item() > 0.01


def test_restated_cell_is_torch_nn_lstm_in_float64():
    """The cell of the restatement against torch.nn.LSTM on random input and non-zero state, three steps: 1e-12."""
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(LR.H, LR.H).double()
    with torch.no_grad():
        for prm in lstm.parameters():
            prm.copy_(torch.randn_like(prm) * 0.2)
    p = {'recurrent.' + k: v.detach() for k, v in lstm.named_parameters()}
    x = torch.randn(3, 7, LR.H, dtype=torch.float64)
    h, c = torch.randn(7, LR.H, dtype=torch.float64), torch.randn(7, LR.H, dtype=torch.float64)
    with torch.no_grad():
        want, (hn, cn) = lstm(x, (h[None], c[None]))
    for t in range(3):
        _, h, c = LR.cell(x[t], h, c, p)
        assert (h - want[t]).abs().max().item() <= 1e-12
    assert (h - hn[0]).abs().max().item() <= 1e-12 and (c - cn[0]).abs().max().item() <= 1e-12


def test_bound_accepts_the_fp32_run_and_rejects_four_wrong_restatements(references):
    """Zero (or stale) state in place of the right one, the last step's head gradient dropped, dW_hh against h_t in place of h_{t-1},
    d b_hh left at zero: each, run in float64, misses max(4 e32, 1e-5 max |f64|) on at least one of the ten tensors of every case."""
    names = LR.NAMES + LR.STATE
    for ref in references:
        tag = ref.case.tag
        g32 = dict(ref.r32['grads'], **{k: ref.r32[k] for k in LR.STATE})
        assert all(err <= bound for err, _, bound in ref.compare(g32, names).values()), tag
        for wrong in LR.WRONG:
            r = LR.run(ref.case, torch.float64, wrong=wrong)
            factors = {k: err / bound for k, (err, _, bound) in ref.compare(r['grads'], LR.NAMES).items()}
            worst = max(factors, key=factors.get)
            missed = [k for k, f in factors.items() if f > 1]
            print(f'[lstm grad f64] {tag:<24} wrong {wrong:<10} misses {len(missed):>2} of 10 tensors; worst {worst:<24} err/bound {factors[worst]:.3e}')
            assert missed, (tag, wrong, factors)
            if wrong == 'dwhh_h_t':
                assert missed == ['recurrent.weight_hh_l0']
            if wrong == 'dbhh_zero':
                assert missed == ['recurrent.bias_hh_l0']
