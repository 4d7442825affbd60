"""tests/ppo_grad_reference.py on the CPU: the committed cases are clear of the loss's kinks, the restatement agrees with the
oracle trainer's own loss.backward(), and the comparison the GPU tests apply is sharp enough to see a gradient that is 1 % off."""
import numpy as np
import pytest
import torch

import ppo_grad_reference as R


@pytest.fixture(scope='module')
def references():
    torch.set_num_threads(4)
    return [R.Reference(c, check=False) for c in R.all_cases()]


def test_committed_cases_cover_the_shape_table_and_keep_their_margins(references):
    """Every committed case keeps 16 fp32 chain errors between each row and each kink of the loss (ReLU at 0, ratio on 1 +- clip_coef,
    newvalue - val on +- vf_clip_coef, the tie of the two value-loss branches), so no row has to be excluded from any comparison."""
    tags = [r.case.tag for r in references]
    assert len(set(tags)) == len(tags)
    for name, *_ in R.MLP_SHAPES:
        assert f'{name}-1wg' in tags and f'{name}-3wg-mb1of2-bptt4' in tags
    assert len(R.MLP_SHAPES) == 15      # the 13 instantiations; (8, 11) and (12, 15) actions each name one of them twice
    for ref in references:
        ref.check_margins()
        c = ref.case
        assert 0 < ref.sums[5] < c.rows, f'{c.tag}: some ratios must be clipped and some not'
        if c.clip_vloss:
            inside = np.abs(ref.r64['newvalue'] - ref.r64['val']) <= c.vf_clip_coef
            assert 0 < inside.sum() < c.rows, f'{c.tag}: both value-loss branches must occur'
        if not c.heads_only:
            w1 = ref.grads['encoder.weight']
            assert np.abs(w1[:, :c.obs_dim]).min(axis=0).max() > 0 and not w1[:, c.obs_dim:].any()
        assert all(np.abs(ref.grads[k]).max() > 0 for k in R.NAMES[2:]) and np.abs(ref.dh).max() > 0


def _oracle_gradient(case):
    """ppo_torch.Trainer.train on the experience of `case` with one epoch, a learning rate of 0 and no clipping: what loss.backward()
    left in .grad for the last minibatch; the trainer's own GAE advantages go back into the case."""
    from oracle import ppo_torch
    hz, nmb, B = case.horizon, case.nmb, case.B
    n = B // hz                                    # one segment per env
    w = {k: v for k, v in case.params.items()}
    w['encoder.weight'] = w['encoder.weight'][:, :case.obs_dim]
    if case.heads:
        del w['decoder.weight'], w['decoder.bias']
        o = 0
        for h, size in enumerate(case.sizes):
            w[f'decoder.{h}.weight'], w[f'decoder.{h}.bias'] = case.params['decoder.weight'][o:o + size], case.params['decoder.bias'][o:o + size]
            o += size

    class _V:
        num_envs = n
        observations = np.zeros((n, case.obs_dim), np.float32)

        def async_reset(self, seed):
            pass
    pol = ppo_torch.Policy(w)
    tr = ppo_torch.Trainer(pol, _V(), batch_size=B, minibatch_size=B // nmb, bptt_horizon=hz, update_epochs=1, learning_rate=0.0, gamma=0.99,
                           gae_lambda=0.95, clip_coef=case.clip_coef, vf_coef=case.vf_coef, vf_clip_coef=case.vf_clip_coef, max_grad_norm=1e30,
                           ent_coef=case.ent_coef, total_timesteps=B * 10, norm_adv=bool(case.norm_adv), clip_vloss=bool(case.clip_vloss))
    sm = lambda x: np.ascontiguousarray(x.reshape(n, hz, *x.shape[1:]).swapaxes(0, 1).reshape(B, *x.shape[1:]))     # noqa: E731
    rs = np.random.RandomState(7)
    tr.obs = torch.as_tensor(sm(case.obs[:, :case.obs_dim]))
    tr.actions = sm(case.acts if case.heads else case.acts[:, 0])
    tr.logprobs, tr.values = sm(case.logprobs), sm(case.values)
    tr.rewards, tr.dones = rs.standard_normal(B).astype(np.float32), (rs.rand(B) < 0.1).astype(np.float32)
    tr.train()
    for m in range(nmb):
        case.advantages[case.rows_index(m)] = tr.b_advantages[m].numpy()
    case.returns = (case.advantages + case.values).astype(np.float32)
    g = {k: p.grad.numpy().copy() for k, p in zip(pol.names, pol.params)}
    if case.heads:
        g['decoder.weight'] = np.concatenate([g[f'decoder.{h}.weight'] for h in range(len(case.sizes))])
        g['decoder.bias'] = np.concatenate([g[f'decoder.{h}.bias'] for h in range(len(case.sizes))])
    return {k: g[k] for k in R.NAMES}


@pytest.mark.parametrize('shape', [('7x7-a8', 49, 64, 8, 0), ('s16-md', 12, 16, 5, 0x23)], ids=lambda s: s[0])
def test_fp32_restatement_matches_the_oracle_trainers_backward(shape):
    """The same minibatch (minibatch 1 of 2, segments of 4 rows) through oracle/ppo_torch.Trainer.train and through the restatement:
    the oracle's fp32 gradient is within the comparison's bound of the float64 reference, and within fp32 rounding of the restatement's
    own fp32 run — the new reference computes what the existing oracle computes."""
    tag, d, dp, a, heads = shape
    case = R.Case('oracle-tie-' + tag, d, dp, a, heads, rows=48, nmb=2, mb=1, horizon=4, seed=5)
    got = _oracle_gradient(case)
    ref = R.Reference(case)
    got['encoder.weight'] = np.pad(got['encoder.weight'], ((0, 0), (0, dp - d)))
    assert ref.failures(got) == []
    for k in R.NAMES:
        np.testing.assert_allclose(got[k], ref.r32['grads'][k].reshape(got[k].shape), rtol=1e-4, atol=4 * ref.e32[k] + 1e-9, err_msg=k)


def test_comparison_rejects_one_tensor_scaled_by_one_percent(references):
    """Adam hides a gradient that is wrong by a constant factor; the comparison with float64 must not: the restatement's own fp32
    gradient passes, and fails as soon as any single tensor is scaled by 1.01 (or the hidden gradient is)."""
    for ref in references:
        g32 = dict(ref.r32['grads'], dh=ref.r32['dh'])
        names = (R.NAMES[2:] if ref.case.heads_only else R.NAMES) + ('dh',)
        assert all(err <= bound for err, _, bound in ref.compare(g32, names).values()), ref.case.tag
        for k in names:
            scaled = dict(g32)
            scaled[k] = g32[k] * 1.01
            res = ref.compare(scaled, names)
            assert [n for n, (err, _, bound) in res.items() if not err <= bound] == [k], (ref.case.tag, k, res[k])
        nan = dict(g32)
        nan['encoder.bias'] = np.full_like(g32['encoder.bias'], np.nan)
        assert not ref.compare(nan, ('encoder.bias',))['encoder.bias'][0] <= ref.bound('encoder.bias')
