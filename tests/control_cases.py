"""What the GPU suites of the classic-control vecenvs (tests/test_gpu_cartpole.py, tests/test_gpu_acrobot.py) share: bit-pattern views
for the exact comparisons, the policies the rollouts are run with, the snapshot both rollout paths are compared by, and the check
that evaluate() took the fused form."""
import numpy as np
import torch


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def snapshot(data, vec, recurrent=False):
    e = data.experience
    out = [x.clone() for x in (e.obs, e.actions, e.logprobs, e.values, e.rewards, e.dones, vec.obs_buf, vec.rewards, vec.terminals_u8,
                                vec.state)]
    if recurrent:
        out += [data.lstm_engine.lstm_h.clone(), data.lstm_engine.lstm_c.clone()]
    return out + [torch.as_tensor(x) for x in vec.debug_states()]


def policy(vec, hidden, recurrent):
    from pufferlib_amd import cleanrl, models
    env = getattr(vec, 'driver_env', vec)          # a vecenv, or the spaces a policy is to be built for
    base = models.Default(env, hidden_size=hidden)
    return cleanrl.RecurrentPolicy(models.LSTMWrapper(env, base)) if recurrent else cleanrl.Policy(base)


def expected_form(data, recurrent):
    from pufferlib_amd import clean_pufferl
    gen = data.gen_engine
    form = clean_pufferl.rollout_form(type(data.vecenv), gen is not None, recurrent, gen is not None and gen.mlp_view is not None)
    assert form == (clean_pufferl.FUSED_LSTM if recurrent else clean_pufferl.FUSED_MLP)
