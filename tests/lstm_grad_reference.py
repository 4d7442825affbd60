"""One minibatch step of clean_pufferl.train for an LSTMWrapper over a Default policy (oracle/ppo_torch.py Trainer.train, the recurrent
branch up to loss.backward()) restated with torch autograd at a chosen dtype, on top of tests/ppo_grad_reference.py: the rows of
minibatch m in time-major order (row t R + k = segment m + k nmb at step t) through encoder Linear + ReLU, Th steps of the LSTM cell in
torch's gate order i, f, g, o, the heads of `_policy_rows` on all Th R hidden states and the loss of `run()`.  The state is zero for
minibatch 0 and afterwards the final (h, c) of minibatch m - 1 under the same parameters, detached (clean_pufferl.py:176, :188-191).  In
float64 it is the expected value of lstm.Engine.update — the whole flat gradient, the loss sums and the state left for the next
minibatch; in float32 it measures what an fp32 chain of this depth loses (`e32`): the bound of the comparison comes from here alone.

`wrong=` switches one line of the restatement to a mistake a recurrent update can make while Adam still moves the weights almost as a
correct one would; tests/test_lstm_grad_reference_cpu.py shows that the bound rejects each of them.  Imports neither the package under
test nor the oracle."""
import numpy as np
import torch
import torch.nn.functional as F

import ppo_grad_reference as R

LSTM_NAMES = ('recurrent.weight_ih_l0', 'recurrent.weight_hh_l0', 'recurrent.bias_ih_l0', 'recurrent.bias_hh_l0')
NAMES = R.NAMES + LSTM_NAMES
STATE = ('h_final', 'c_final')
WRONG = ('state', 'last_dh', 'dwhh_h_t', 'dbhh_zero')
H = 128


def cell(x, h, c, p):
    """One nn.LSTM step: (gate pre-activations, h, c)."""
    pre = F.linear(x, p['recurrent.weight_ih_l0'], p['recurrent.bias_ih_l0']) + F.linear(h, p['recurrent.weight_hh_l0'], p['recurrent.bias_hh_l0'])
    i, f, g, o = pre.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return pre, torch.sigmoid(o) * torch.tanh(c), c


def forward(case, p, m, state, dtype, last_dh=True):
    """Minibatch m from `state`: (encoder pre-activation [M][H], h of every step as [M][H] time-major, per-step gate pre-activations,
    per-step h_{t-1}, final (h, c))."""
    Rr, Th = case.R, case.horizon
    obs = torch.as_tensor(case.obs)[torch.as_tensor(case.rows_index(m))].to(dtype)
    pre = F.linear(obs, p['encoder.weight'], p['encoder.bias'])
    x = torch.relu(pre)
    h, c = state
    hs, gates, prev = [], [], []
    for t in range(Th):
        prev.append(h)
        g, h, c = cell(x[t * Rr:(t + 1) * Rr], h, c, p)
        gates.append(g)
        hs.append(h)
    if not last_dh:
        hs[-1] = hs[-1].detach()        # WRONG 'last_dh': the heads' d loss / d h of the last step never reaches the cell
    return pre, torch.cat(hs), gates, prev, (h, c)


def carried_state(case, p, m, dtype):
    """The state minibatch m starts from: zeros, or minibatches 0 .. m-1 walked with the carry."""
    state = (torch.zeros(case.R, H, dtype=dtype), torch.zeros(case.R, H, dtype=dtype))
    with torch.no_grad():
        for q in range(m):
            state = forward(case, p, q, state, dtype)[4]
    return state


class Case(R.Case):
    """A recurrent case (obs_dim, stride, actions, heads, R, Th, nmb, mb): R segments of Th steps per minibatch, M = R Th rows."""

    def __init__(self, tag, obs_dim, stride, actions, heads, R_, Th, nmb, mb, seed, **kw):
        self.R = R_
        super().__init__(tag, obs_dim, stride, actions, heads, rows=R_ * Th, nmb=nmb, mb=mb, horizon=Th, seed=seed, time_major=True, **kw)

    def more_params(self, rs):
        f32 = np.float32
        self.params['recurrent.weight_ih_l0'] = (rs.standard_normal((4 * H, H)) / np.sqrt(H)).astype(f32)
        self.params['recurrent.weight_hh_l0'] = (rs.standard_normal((4 * H, H)) / np.sqrt(H)).astype(f32)
        self.params['recurrent.bias_ih_l0'] = (0.2 * rs.standard_normal(4 * H)).astype(f32)
        self.params['recurrent.bias_hh_l0'] = (0.2 * rs.standard_normal(4 * H)).astype(f32)

    def old_policy(self):
        """The float64 recurrent policy's own log-probabilities and values: minibatches 0 .. nmb-1 walked with the carry."""
        lp, val = np.zeros(self.B), np.zeros(self.B)
        p = {k: torch.as_tensor(v).double() for k, v in self.params.items()}
        acts = torch.as_tensor(self.acts)
        state = carried_state(self, p, 0, torch.float64)
        with torch.no_grad():
            for m in range(self.nmb):
                idx = self.rows_index(m)
                _, h_all, _, _, state = forward(self, p, m, state, torch.float64)
                _, _, l, _, v = R._policy_rows(p, None, acts[torch.as_tensor(idx)], self.sizes, hidden=h_all)
                lp[idx], val[idx] = l.numpy(), v.numpy()
        return lp, val

    def flat_params(self):
        """models.FlatParams' order: the padded MLP vector, then W_ih, W_hh, b_ih, b_hh."""
        return np.concatenate([super().flat_params()] + [self.params[k].reshape(-1) for k in LSTM_NAMES])

    def split_flat(self, flat):
        n = H * self.stride + H + self.actions * H + self.actions + H + 1
        out = super().split_flat(np.asarray(flat[:n]))
        for k in LSTM_NAMES:
            s = self.params[k].shape
            out[k] = np.asarray(flat[n:n + int(np.prod(s))]).reshape(s)
            n += int(np.prod(s))
        assert n == len(flat)
        return out


def run(case, dtype, wrong=None):
    """The minibatch step of `case` at `dtype`: the ten gradients, the loss sums, the final state and what the kinks sit on."""
    assert wrong is None or wrong in WRONG
    idx = torch.as_tensor(case.rows_index())
    t = lambda x: torch.as_tensor(x)[idx].to(dtype)     # noqa: E731
    p = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in case.params.items()}
    acts = torch.as_tensor(case.acts)[idx]
    m = case.mb
    if wrong == 'state':        # WRONG: zeros where a state is carried; where the state is zero (minibatch 0), the stale one of the
        m = 0 if case.mb else case.nmb      # epoch's last minibatch, which is what the engine's slot Th holds at an epoch boundary
    state = carried_state(case, {k: v.detach() for k, v in p.items()}, m, dtype)
    pre, h_all, gates, prev, final = forward(case, p, case.mb, state, dtype, last_dh=wrong != 'last_dh')
    for g in gates:
        g.retain_grad()
    _, _, newlogprob, entropy, newvalue = R._policy_rows(p, None, acts, case.sizes, hidden=h_all)
    old_lp, val, adv, ret = t(case.logprobs), t(case.values), t(case.advantages), t(case.returns)
    logratio = newlogprob - old_lp
    ratio = logratio.exp()
    a = adv
    if case.norm_adv:
        a = (a - a.mean()) / (a.std() + 1e-8)
    lo, hi = 1 - case.clip_coef, 1 + case.clip_coef
    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, lo, hi))
    if case.clip_vloss:
        v_clipped = val + torch.clamp(newvalue - val, -case.vf_clip_coef, case.vf_clip_coef)
        v_rows = 0.5 * torch.max((newvalue - ret) ** 2, (v_clipped - ret) ** 2)
    else:
        v_rows = 0.5 * (newvalue - ret) ** 2
    loss = pg.mean() - case.ent_coef * entropy.mean() + case.vf_coef * v_rows.mean()
    loss.backward()
    d = lambda x: x.detach().double().numpy()           # noqa: E731
    clipped = ((ratio - 1.0).abs() > case.clip_coef).double()
    gd = lambda x: d(x.grad if x.grad is not None else torch.zeros_like(x))      # noqa: E731  (no path to the loss: zero)
    grads = {k: gd(p[k]) for k in NAMES}
    # dW_hh once more, by hand from d loss / d gate pre-activations: against h_{t-1} it is autograd's (the CPU test holds them together)
    against = [h_all[i * case.R:(i + 1) * case.R] for i in range(case.horizon)] if wrong == 'dwhh_h_t' else prev     # WRONG: h_t
    by_hand = sum(gd(g).T @ d(h) for g, h in zip(gates, against))
    if wrong == 'dwhh_h_t':
        grads['recurrent.weight_hh_l0'] = by_hand
    if wrong == 'dbhh_zero':    # WRONG: d b_hh never written
        grads['recurrent.bias_hh_l0'] = np.zeros(4 * H)
    return dict(grads=grads, dwhh_by_hand=by_hand, h_final=d(final[0]), c_final=d(final[1]),
                sums=np.array([d(x).sum() for x in (pg, v_rows, entropy, -logratio, (ratio - 1) - logratio, clipped)]),
                pre=d(pre), ratio=d(ratio), newvalue=d(newvalue), val=d(val), ret=d(ret))


class Reference(R.Reference):
    """float64 expected values of a recurrent case, the fp32 chain error per output (the final state has its own), the margins check.
    The LSTM is smooth: the kinks are those of the encoder's ReLU and of the loss."""

    def __init__(self, case, check=True):
        self.case = case
        self.r64, self.r32 = run(case, torch.float64), run(case, torch.float32)
        self.grads, self.sums = self.r64['grads'], self.r64['sums']
        self.state = {k: self.r64[k] for k in STATE}
        self.e32 = {k: float(np.abs(self.r32['grads'][k] - v).max()) for k, v in self.grads.items()}
        self.e32.update({k: float(np.abs(self.r32[k] - v).max()) for k, v in self.state.items()})
        self.margins = R.kink_margins(self.r64, self.r32, case)
        if check:
            self.check_margins()

    def want(self, name):
        return self.state[name] if name in self.state else self.grads[name]

    def failures(self, got, names=NAMES, report=None):
        return super().failures(got, names, report)


# ------------------------------------------------------------------------------------------------------------------- committed cases
# (tag, obs_dim, stride, actions, heads, R, Th, nmb, mb, what else): the six row strides lstm_seq_fwd_kernel<DP> is built for; R ragged
# and a multiple of the 32-row workgroup (lstm_seq_bwd_kernel<false> / <true>); fewer rows than one workgroup and three full ones; the
# state carried once, twice, and not at all; Th = 1, where nothing but the carried state is recurrent; 16 steps
SHAPES = [
    ('s16-md', 12, 16, 5, 0x23, 33, 4, 2, 1, {}),
    ('s32', 25, 32, 8, 0, 64, 2, 2, 0, {}),
    ('s64-small', 49, 64, 8, 0, 7, 3, 2, 1, {}),
    ('s64-3mb', 49, 64, 8, 0, 40, 5, 3, 2, {}),
    ('s64-long', 49, 64, 15, 0, 96, 16, 2, 1, {}),
    ('s96', 81, 96, 6, 0, 32, 4, 2, 1, {}),
    ('s128', 121, 128, 15, 0, 17, 3, 2, 1, {}),
    ('s160', 147, 160, 7, 0, 64, 4, 2, 1, {}),
    ('s64-bptt1', 49, 64, 8, 0, 3, 1, 2, 1, {}),
    ('s64-no-norm-adv', 49, 64, 8, 0, 40, 5, 2, 1, dict(norm_adv=0)),
    ('s64-no-clip-vloss', 49, 64, 8, 0, 40, 5, 2, 1, dict(clip_vloss=0)),
]
# seeds chosen on the CPU (Reference.margins_ok): the first of 1, 2, 3, ... at which the float64 reference is clear of every kink
SEEDS = {'s16-md': 2, 's64-long': 3, 's96': 3, 's160': 3, 's64-no-norm-adv': 2, 's64-no-clip-vloss': 2}    # seed 1 unless listed here


def cases():
    return [Case('lstm-' + tag, d, dp, a, heads, r, th, nmb, mb, seed=SEEDS.get(tag, 1), **kw) for tag, d, dp, a, heads, r, th, nmb, mb, kw in SHAPES]
