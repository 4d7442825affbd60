"""CPU reference of tests/test_gpu_autograd.py: pufferlib.models.Default (encoder Linear + ReLU, decoder head(s), value head), alone or
under LSTMWrapper (nn.LSTM between encoder and heads, models.py:84-111), scored with given actions by sample_logits (oracle/ppo_torch.py,
cleanrl.py:25-47), restated with torch autograd at a chosen dtype.  In float64 it is the expected value of what
cleanrl.Policy(..., autograd=True) returns and back-propagates; in float32 it measures what an fp32 chain of this depth loses against
float64 (`e32`) — the bound of every comparison is max(4 e32, 1e-5 max(1, max |f64|)) per tensor, taken from this file, never from the
code under test.

Every case is generated from a seed on the CPU.  Gradients are discontinuous where an encoder pre-activation is 0 and, for the PPO loss,
where the ratio sits on 1 +- clip_coef, where newvalue - val sits on +- vf_clip_coef and where the two value-loss branches tie: run()
reports the distance to each, and check_margins() asserts in float64 that every row keeps 16 fp32 chain errors away (the rule of
ppo_grad_reference).  Imports the oracle's sample_logits and nothing of the package under test."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ppo_torch import sample_logits

LSTM_NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
MARGIN = 16.0
PPO = dict(clip_coef=0.1, vf_clip_coef=0.1, vf_coef=0.5, ent_coef=0.01)


class Env:
    """What models.Default / LSTMWrapper read of an env: the two spaces."""

    def __init__(self, obs_dim, nvec, multi):
        self.single_observation_space = types.SimpleNamespace(shape=(obs_dim,), dtype=np.float32)
        self.single_action_space = types.SimpleNamespace(nvec=np.asarray(nvec)) if multi else types.SimpleNamespace(n=int(nvec[0]))


class Case:
    """One policy shape and one call: parameters by the module's short names (encoder.*, decoder.* or decoder.<h>.*, value_head.*, and
    the nn.LSTM's names when lstm = (input_size, hidden_size)), observations [B * TT][obs_dim] in (b, t) row order, actions
    [B * TT][heads], a non-zero state, and the per-row numbers the two losses read."""

    def __init__(self, tag, hidden, obs_dim, nvec, multi=False, B=37, TT=1, lstm=None, seed=1, state=True, integer_obs=False):
        self.tag, self.hidden, self.obs_dim, self.nvec, self.multi = tag, hidden, obs_dim, list(nvec), multi
        self.B, self.TT, self.lstm, self.seed = B, TT, lstm, seed
        self.rows = rows = B * TT
        rs = np.random.RandomState(seed)
        f32 = np.float32
        A, FH = sum(nvec), (lstm[1] if lstm else hidden)
        w = {'encoder.weight': rs.standard_normal((hidden, obs_dim)) / np.sqrt(obs_dim), 'encoder.bias': 0.1 * rs.standard_normal(hidden)}
        for h, n in enumerate(nvec):
            stem = f'decoder.{h}' if multi else 'decoder'
            w[stem + '.weight'] = rs.standard_normal((n, FH)) / np.sqrt(FH)
            w[stem + '.bias'] = 0.1 * rs.standard_normal(n)
        w['value_head.weight'] = rs.standard_normal((1, FH)) / np.sqrt(FH)
        w['value_head.bias'] = 0.1 * rs.standard_normal(1)
        if lstm:
            I, Hl = lstm
            assert I == hidden
            w['weight_ih_l0'] = rs.standard_normal((4 * Hl, I)) / np.sqrt(I)
            w['weight_hh_l0'] = rs.standard_normal((4 * Hl, Hl)) / np.sqrt(Hl)
            w['bias_ih_l0'], w['bias_hh_l0'] = 0.1 * rs.standard_normal(4 * Hl), 0.1 * rs.standard_normal(4 * Hl)
        self.params = {k: np.ascontiguousarray(v, dtype=f32) for k, v in w.items()}
        self.names = list(self.params)
        obs = rs.randint(0, 3, (rows, obs_dim)) if integer_obs else rs.standard_normal((rows, obs_dim))
        self.obs = obs.astype(f32)
        self.acts = np.stack([rs.randint(0, n, rows) for n in nvec], axis=1).astype(np.int64)
        self.state = None
        if lstm and state:
            self.state = tuple((0.3 * rs.standard_normal((1, B, lstm[1]))).astype(f32) for _ in range(2))
        # the random linear loss sum(u logprob + v entropy + w value) ...
        self.u, self.v, self.w = (rs.standard_normal(rows).astype(f32) for _ in range(3))
        # ... and a PPO minibatch: old log-probabilities and values = the float64 policy's own + noise, so ratios leave 1
        self.advantages = rs.standard_normal(rows).astype(f32)
        noise_lp, noise_v = 0.2 * rs.standard_normal(rows), 0.2 * rs.standard_normal(rows)
        with torch.no_grad():
            out = forward(self, torch.float64)
        self.logprobs = (out['logprob'].numpy() + noise_lp).astype(f32)
        self.values = (out['value'].numpy().reshape(-1) + noise_v).astype(f32)
        self.returns = (self.values + self.advantages).astype(f32)

    def set_experience(self, logprobs, values, advantages, returns):
        """A PPO minibatch recorded elsewhere (a rollout on the device) instead of the generated one."""
        f = lambda x: np.ascontiguousarray(np.asarray(x, np.float32).reshape(self.rows))      # noqa: E731
        self.logprobs, self.values, self.advantages, self.returns = f(logprobs), f(values), f(advantages), f(returns)

    def actions_for_policy(self):
        """[rows] for a Discrete head, [rows][heads] for MultiDiscrete: what policy(obs, action=...) takes."""
        return self.acts if self.multi else self.acts[:, 0]


def forward(case, dtype):
    """The policy call at `dtype`: dict(params (leaf tensors), pre, logprob, entropy, value [rows][1], state)."""
    p = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in case.params.items()}
    obs = torch.as_tensor(case.obs).to(dtype)
    pre = F.linear(obs, p['encoder.weight'], p['encoder.bias'])
    hidden = torch.relu(pre)
    state = None
    if case.lstm:
        I, Hl = case.lstm
        lstm = torch.nn.LSTM(I, Hl).to(dtype)      # nn.LSTM's own arithmetic; its parameters are the leaves of these four names
        with torch.no_grad():
            for n in LSTM_NAMES:
                getattr(lstm, n).copy_(p[n])
        p.update({n: getattr(lstm, n) for n in LSTM_NAMES})
        s = None if case.state is None else tuple(torch.as_tensor(x).to(dtype) for x in case.state)
        x = hidden.reshape(case.B, case.TT, I).transpose(0, 1)                      # models.py:99-101
        y, state = lstm(x, s)
        hidden = y.transpose(0, 1).reshape(case.rows, Hl)                           # models.py:107-108
    stems = [f'decoder.{h}' for h in range(len(case.nvec))] if case.multi else ['decoder']
    logits = [F.linear(hidden, p[s + '.weight'], p[s + '.bias']) for s in stems]
    value = F.linear(hidden, p['value_head.weight'], p['value_head.bias'])
    acts = torch.as_tensor(case.acts)
    _, logprob, entropy = sample_logits(logits if case.multi else logits[0], action=acts if case.multi else acts[:, 0])
    return dict(params=p, pre=pre, logprob=logprob, entropy=entropy, value=value, state=state)


def linear_loss(case, logprob, entropy, value):
    t = lambda x: torch.as_tensor(x).to(device=logprob.device, dtype=logprob.dtype)      # noqa: E731
    return (t(case.u) * logprob + t(case.v) * entropy + t(case.w) * value.reshape(-1)).sum()


def ppo_loss(case, logprob, entropy, value, parts=None):
    """clean_pufferl.py:202-238 in torch ops on the returned tensors: ratio, clipped surrogate on normalised advantages, clipped value
    loss, entropy bonus.  parts (a dict): also the per-row quantities the kinks sit on."""
    t = lambda x: torch.as_tensor(x).to(device=logprob.device, dtype=logprob.dtype)      # noqa: E731
    old_lp, val, adv, ret = t(case.logprobs), t(case.values), t(case.advantages), t(case.returns)
    logratio = logprob - old_lp
    ratio = logratio.exp()
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - PPO['clip_coef'], 1 + PPO['clip_coef'])).mean()
    newvalue = value.view(-1)
    v_clipped = val + torch.clamp(newvalue - val, -PPO['vf_clip_coef'], PPO['vf_clip_coef'])
    v_loss = 0.5 * torch.max((newvalue - ret) ** 2, (v_clipped - ret) ** 2).mean()
    if parts is not None:
        parts.update(ratio=ratio.detach(), newvalue=newvalue.detach(), val=val, ret=ret)
    return pg_loss - PPO['ent_coef'] * entropy.mean() + v_loss * PPO['vf_coef']


def run(case, loss, dtype):
    """Forward + loss + backward at dtype: outputs, state and gradients as float64 numpy, and the quantities of the kinks."""
    out = forward(case, dtype)
    parts = {}
    value = loss(case, out['logprob'], out['entropy'], out['value'], parts) if loss is ppo_loss else loss(case, out['logprob'], out['entropy'], out['value'])
    value.backward()
    d = lambda x: x.detach().double().numpy()           # noqa: E731
    res = dict(grads={k: d(v.grad) for k, v in out['params'].items()}, pre=d(out['pre']), loss=value.item(),
               outputs={k: d(out[k]) for k in ('logprob', 'entropy', 'value')}, parts={k: d(v) for k, v in parts.items()})
    if out['state'] is not None:
        res['outputs']['h'], res['outputs']['c'] = d(out['state'][0]), d(out['state'][1])
    return res


def recorded_case(tag, hidden, nvec, B, TT, lstm, params, obs, acts, logprobs, values, advantages, returns):
    """A case whose parameters and PPO minibatch were recorded elsewhere (a rollout on the device): zero state, rows in (b, t) order."""
    obs = np.ascontiguousarray(np.asarray(obs, np.float32))
    case = Case(tag, hidden, obs.shape[1], nvec, B=B, TT=TT, lstm=lstm, state=False)
    assert set(params) == set(case.params) and all(case.params[k].shape == np.asarray(v).shape for k, v in params.items())
    case.params = {k: np.ascontiguousarray(np.asarray(params[k], np.float32)) for k in case.names}
    case.obs, case.acts = obs, np.asarray(acts, np.int64).reshape(case.rows, -1)
    case.set_experience(logprobs, values, advantages, returns)
    return case


def optimizer_step(case, dtype, lr, max_grad_norm):
    """One whole custom-loop step at dtype: the policy call, the PPO loss, backward, clip_grad_norm_, Adam(lr, eps=1e-5).step()
    (clean_pufferl.py:54-55,240-244).  Returns the updated parameters as float64 numpy."""
    out = forward(case, dtype)
    params = [out['params'][k] for k in case.names]
    opt = torch.optim.Adam(params, lr=lr, eps=1e-5)
    ppo_loss(case, out['logprob'], out['entropy'], out['value']).backward()
    torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
    opt.step()
    return {k: p.detach().double().numpy() for k, p in zip(case.names, params)}


def bound(e32, want):
    """max(4 e32, 1e-5 max(1, max |f64|)): four fp32 chain errors, floored at the project's 1e-5 scaled by the tensor's largest entry
    (tests/test_gpu_resnet.py's _close_scaled)."""
    return max(4.0 * e32, 1e-5 * max(1.0, float(np.abs(want).max())))


class Reference:
    """float64 expected values of (case, loss), the fp32 chain error per tensor, and the margins check."""

    def __init__(self, case, loss, check=True):
        self.case, self.loss = case, loss
        self.r64, self.r32 = run(case, loss, torch.float64), run(case, loss, torch.float32)
        self.grads, self.outputs = self.r64['grads'], self.r64['outputs']
        self.e32 = {k: float(np.abs(self.r32['grads'][k] - v).max()) for k, v in self.grads.items()}
        self.e32_out = {k: float(np.abs(self.r32['outputs'][k] - v).max()) for k, v in self.outputs.items()}
        if check:
            self.check_margins()

    def margins(self):
        """name -> (smallest float64 distance to the kink, fp32 chain error of the quantity the kink is on)."""
        r64, r32 = self.r64, self.r32
        out = {'relu': (float(np.abs(r64['pre']).min()), float(np.abs(r32['pre'] - r64['pre']).max()))}
        if r64['parts']:
            p64, p32 = r64['parts'], r32['parts']
            out['ratio clip'] = (float(np.abs(np.abs(p64['ratio'] - 1.0) - PPO['clip_coef']).min()), float(np.abs(p32['ratio'] - p64['ratio']).max()))
            e_v = float(np.abs(p32['newvalue'] - p64['newvalue']).max())
            delta = p64['newvalue'] - p64['val']
            out['value clip'] = (float(np.abs(np.abs(delta) - PPO['vf_clip_coef']).min()), e_v)
            outside = np.abs(delta) > PPO['vf_clip_coef']         # (inside, the two branches are the same function: no kink)
            du = p64['newvalue'] - p64['ret']
            dc = p64['val'] + np.clip(delta, -PPO['vf_clip_coef'], PPO['vf_clip_coef']) - p64['ret']
            tie = np.abs(np.abs(du) - np.abs(dc))[outside]
            out['value branch tie'] = (float(tie.min()) if tie.size else float('inf'), e_v)
        return out

    def margins_ok(self):
        return all(gap > MARGIN * err for gap, err in self.margins().values())

    def check_margins(self):
        for name, (gap, err) in self.margins().items():
            assert gap > MARGIN * err, f'{self.case.tag}: {name}: smallest distance {gap:.3e} vs {MARGIN:g} x {err:.3e}: choose another seed'

    def failures(self, got, what='grad', against=None):
        """The tensors of `got` (name -> array) beyond their bound; one printed line per tensor: fp32 CPU error, device error, bound.
        against: compare with these arrays instead of the float64 ones (the bound stays this reference's)."""
        want_all, e_all = (self.grads, self.e32) if what == 'grad' else (self.outputs, self.e32_out)
        bad = []
        for k, g in got.items():
            want = want_all[k]
            b = bound(e_all[k], want)
            other = want if against is None else np.asarray(against[k], np.float64).reshape(want.shape)
            g = np.asarray(g, np.float64).reshape(want.shape)
            err = float(np.abs(g - other).max()) if np.isfinite(g).all() else float('inf')
            print(f'[autograd f64] {self.case.tag:<22} {self.loss.__name__:<11} {what:<5} {k:<20} cpu-fp32 err {e_all[k]:.3e}  device err {err:.3e}  '
                  f'bound {b:.3e}  err/bound {err / b:.3f}')
            if not err <= b:
                bad.append(k)
        return bad


# ------------------------------------------------------------------------------------------------------------------- committed cases
# the smallest shapes at which each piece can go wrong: hidden 48 = three 16-column tiles, 5 observation floats on a 16-float row,
# 37 rows (no multiple of 16, more than one 16-row tile); 63 logits (the head kernels' limit) on 17 rows; LSTMWrapper(48, 32) over
# B = 5 segments of TT = 3 steps from a non-zero state, and of one step; the kernel-layout family (Default(128) on 3 x 3 Squared rows =
# 9 floats, 8 actions) alone and under LSTMWrapper(128, 128), B = 4, TT = 4.  Seeds: the first of 1, 2, 3, ... at which both losses pass
# check_margins on the CPU.
def cases():
    return [Case('default-h48-d3', 48, 5, [3], seed=1),
            Case('default-h48-md325', 48, 5, [3, 2, 5], multi=True, seed=1),
            Case('default-h64-d63', 64, 5, [63], B=17, seed=1),
            Case('lstm48x32-B5-TT3', 48, 5, [3], B=5, TT=3, lstm=(48, 32), seed=1),
            Case('lstm48x32-B5-TT1', 48, 5, [3], B=5, TT=1, lstm=(48, 32), seed=1),
            Case('flat-default128', 128, 9, [8], B=37, seed=1, integer_obs=True),
            Case('flat-lstm128-B4-TT4', 128, 9, [8], B=4, TT=4, lstm=(128, 128), seed=1, integer_obs=True)]


def find_seeds():
    """Development aid: the first seed per case at which both losses are clear of every kink."""
    for c in cases():
        for seed in range(1, 50):
            cc = Case(c.tag, c.hidden, c.obs_dim, c.nvec, c.multi, c.B, c.TT, c.lstm, seed, integer_obs=bool((c.obs == c.obs.round()).all()))
            if all(Reference(cc, loss, check=False).margins_ok() for loss in (linear_loss, ppo_loss)):
                print(c.tag, seed)
                break


if __name__ == '__main__':
    find_seeds()
