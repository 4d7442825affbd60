"""Adam's moments of the device trainer against the oracle trainer's, for every GPU test that trains both on the same experience.
The weights those tests compare barely see the gradient's magnitude (Adam divides the gradient by its own running magnitude: one
tensor's gradient scaled by 1.2 moves the weights by less than the 1e-5 they are compared at); exp_avg and exp_avg_sq see it in
full.  Tolerances: the ones tests/test_gpu_big_goldens.py holds the moments to against the reference's recorded ones."""
import numpy as np

EXP_AVG = dict(rtol=2e-4, atol=1e-6)
EXP_AVG_SQ = dict(rtol=2e-4, atol=1e-8)


def _device_key(keys, name):
    """The device-side name of the oracle's parameter `name`: the same, or with the module's prefixes in front."""
    hits = [k for k in keys if k == name or k.endswith('.' + name)]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def assert_moments_match(data, tr):
    """data: the device trainer after clean_pufferl.train; tr: the oracle/ppo_torch.Trainer after train() on the same experience."""
    fp, opt = data.flat_params, data.optimizer
    m_, v_ = fp.split(opt.exp_avg), fp.split(opt.exp_avg_sq)
    om, ov = tr.adam_moments()
    assert len(om) == len(m_), (sorted(om), sorted(m_))
    # (a tensor's moments may be all zero — the Stochastic env's only observation is 0.0, so its encoder.weight never moves — not all of them)
    assert sum(float(np.abs(x).max()) > 0 for x in om.values()) >= len(om) - 1 and all(float(x.min()) >= 0 for x in ov.values())
    for name in om:
        k = _device_key(list(m_), name)
        m, v = m_[k].cpu().numpy(), v_[k].cpu().numpy()
        np.testing.assert_allclose(m.reshape(om[name].shape), om[name], err_msg=f'exp_avg {name}', **EXP_AVG)
        np.testing.assert_allclose(v.reshape(ov[name].shape), ov[name], err_msg=f'exp_avg_sq {name}', **EXP_AVG_SQ)
