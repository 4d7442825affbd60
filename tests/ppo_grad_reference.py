"""One minibatch step of clean_pufferl.train for a Default policy (oracle/ppo_torch.py Trainer.train, the non-recurrent branch up to
loss.backward()) restated with torch autograd at a chosen dtype: encoder Linear + ReLU, decoder head(s), value head, sample_logits with
the stored actions, loss = pg_loss - ent_coef * entropy + vf_coef * v_loss as means over the minibatch rows.  In float64 it is the
expected value of the fused gradient kernels (pfa_ppo_mlp_grad, pfa_ppo_wide_grad, pfa_lstm_heads_loss); in float32 it measures what an
fp32 chain of this depth loses (`e32`), which is where the bound of the comparisons comes from — never from the kernel.

Every case is generated from a seed on the CPU.  The gradient is discontinuous where a hidden pre-activation is 0, where the ratio sits
on 1 +- clip_coef, where newvalue - val sits on +- vf_clip_coef and where the two value-loss branches tie: `Reference` asserts, in
float64, that every row keeps 16x the matching fp32 chain error away from each (the rule of resnet_reference.check_margins), and the
seeds of the committed cases were chosen so that nothing has to be excluded.  Imports neither the package under test nor the oracle."""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ('encoder.weight', 'encoder.bias', 'decoder.weight', 'decoder.bias', 'value_head.weight', 'value_head.bias')
SUMS = ('pg_loss', 'v_loss', 'entropy', '-logratio', 'ratio-1-logratio', 'clipped')     # the six loss sums of pfa_ppo_mlp_grad
MARGIN = 16.0


def head_sizes(actions, heads):
    """pfa_mlp_dims.heads: 0 = one Discrete(actions) head, else head h has (heads >> 4h) & 15 logits."""
    if heads == 0:
        return [actions]
    out = []
    while heads:
        out.append(heads & 15)
        heads >>= 4
    assert sum(out) == actions
    return out


def _policy_rows(p, obs, acts, sizes, hidden=None):
    """(pre-activation, hidden, new log-probability, entropy, new value) per row; `hidden` given: the heads alone."""
    pre = None
    if hidden is None:
        pre = F.linear(obs, p['encoder.weight'], p['encoder.bias'])
        hidden = torch.relu(pre)
    logits = F.linear(hidden, p['decoder.weight'], p['decoder.bias'])
    value = F.linear(hidden, p['value_head.weight'], p['value_head.bias']).view(-1)
    logprob, entropy, o = 0.0, 0.0, 0
    for h, n in enumerate(sizes):              # cleanrl.py:25-47 with the stored actions: per head, summed over heads
        nl = torch.log_softmax(logits[:, o:o + n], dim=-1)
        logprob = logprob + nl.gather(-1, acts[:, h:h + 1]).squeeze(-1)
        entropy = entropy - (nl * nl.exp()).sum(-1)
        o += n
    return pre, hidden, logprob, entropy, value


class Case:
    """fp32 inputs of one launch: parameters, a batch of rows * nmb experience rows (env-major), and which minibatch is trained."""

    def __init__(self, tag, obs_dim, stride, actions, heads=0, rows=64, nmb=1, mb=0, horizon=16, seed=0, hidden=128, norm_adv=1,
                 clip_vloss=1, time_major=False, heads_only=False):
        self.tag, self.obs_dim, self.stride, self.actions, self.heads, self.hidden = tag, obs_dim, stride, actions, heads, hidden
        self.rows, self.nmb, self.mb, self.horizon, self.seed = rows, nmb, mb, horizon, seed
        self.norm_adv, self.clip_vloss = norm_adv, clip_vloss
        self.clip_coef, self.vf_clip_coef, self.vf_coef, self.ent_coef = 0.1, 0.1, 0.5, 0.01
        self.time_major, self.heads_only = time_major, heads_only
        assert rows % horizon == 0 and 0 <= mb < nmb and obs_dim <= stride
        self.sizes = head_sizes(actions, heads)
        B = self.B = rows * nmb
        rs = np.random.RandomState(seed)
        f32 = np.float32
        w1 = np.zeros((hidden, stride), f32)
        w1[:, :obs_dim] = rs.standard_normal((hidden, obs_dim)) / np.sqrt(obs_dim)
        self.params = {
            'encoder.weight': w1, 'encoder.bias': (0.1 * rs.standard_normal(hidden)).astype(f32),
            'decoder.weight': (rs.standard_normal((actions, hidden)) / np.sqrt(hidden)).astype(f32),
            'decoder.bias': (0.1 * rs.standard_normal(actions)).astype(f32),
            'value_head.weight': (rs.standard_normal((1, hidden)) / np.sqrt(hidden)).astype(f32),
            'value_head.bias': (0.1 * rs.standard_normal(1)).astype(f32)}
        self.obs = np.zeros((B, stride), f32)
        self.obs[:, :obs_dim] = rs.standard_normal((B, obs_dim))
        # (heads_only: the rows of h are what the recurrent layer would hand to the heads, time-major rows of the minibatch)
        self.h = np.tanh(rs.standard_normal((rows, hidden))).astype(f32) if heads_only else None
        self.acts = np.stack([rs.randint(0, n, B) for n in self.sizes], axis=1).astype(np.int64)
        self.advantages = rs.standard_normal(B).astype(f32)
        noise_lp, noise_v = 0.2 * rs.standard_normal(B), 0.2 * rs.standard_normal(B)
        self.more_params(rs)                    # (drawn last: the cases without any keep their numbers)
        lp, val = self.old_policy()             # old log-probabilities and values: the f64 policy's own + noise, so ratios leave 1
        self.logprobs = (lp + noise_lp).astype(f32)
        self.values = (val + noise_v).astype(f32)
        self.returns = (self.values + self.advantages).astype(f32)      # clean_pufferl.py:199

    def more_params(self, rs):
        """Parameters behind the six of NAMES (a subclass's: tests/lstm_grad_reference.py)."""

    def old_policy(self):
        """([B] log-probability of the stored actions, [B] value) of the float64 policy on every experience row."""
        B, idx = self.B, self.rows_index()
        with torch.no_grad():
            p = {k: torch.as_tensor(v).double() for k, v in self.params.items()}
            acts = torch.as_tensor(self.acts)
            if self.heads_only:
                lp, val = np.zeros(B), np.zeros(B)
                _, _, l, _, v = _policy_rows(p, None, acts[idx], self.sizes, hidden=torch.as_tensor(self.h).double())
                lp[idx], val[idx] = l.numpy(), v.numpy()
            else:
                _, _, l, _, v = _policy_rows(p, torch.as_tensor(self.obs).double(), acts, self.sizes)
                lp, val = l.numpy(), v.numpy()
        return lp, val

    def rows_index(self, mb=None):
        """Flat experience row of every minibatch row, in the order the kernel walks them: minibatch m = segments {m + k nmb} of
        `horizon` rows (clean_pufferl.py:455-457), segment after segment — or, time_major, step after step (row t R + k)."""
        mb = self.mb if mb is None else mb
        q = np.arange(self.rows)
        if self.time_major:
            R = self.rows // self.horizon
            t, k = q // R, q % R
        else:
            k, t = q // self.horizon, q % self.horizon
        return (mb + k * self.nmb) * self.horizon + t

    # ---- what the device reads --------------------------------------------------------------------------------------------------
    def flat_params(self, padded=True):
        """The flat parameter vector: W1 [H][stride] (padded) or [H][obs_dim], b1, W2, b2, wv, bv."""
        w1 = self.params['encoder.weight']
        parts = [w1 if padded else w1[:, :self.obs_dim]] + [self.params[k] for k in NAMES[1:]]
        return np.concatenate([np.ascontiguousarray(x).reshape(-1) for x in parts])

    def split_flat(self, flat, padded=True):
        """name -> array of a flat vector in that order (W1 keeps its padding columns when padded)."""
        cols = self.stride if padded else self.obs_dim
        H, A = self.hidden, self.actions
        shapes = [(H, cols), (H,), (A, H), (A,), (1, H), (1,)]
        out, o = {}, 0
        for k, s in zip(NAMES, shapes):
            n = int(np.prod(s))
            out[k] = np.asarray(flat[o:o + n]).reshape(s)
            o += n
        assert o == len(flat)
        return out

    def packed_actions(self):
        """int32 per row: the Discrete choice, or head h's choice in bits 4h..4h+3."""
        if self.heads == 0:
            return self.acts[:, 0].astype(np.int32)
        return sum(self.acts[:, h].astype(np.int32) << (4 * h) for h in range(len(self.sizes))).astype(np.int32)

    def adv_stats(self):
        """[nmb][2] f64: (sum, sum of squares) of every minibatch's advantages — what pfa_ppo_adv_stats leaves."""
        a = self.advantages.astype(np.float64)
        return np.array([[a[self.rows_index(m)].sum(), (a[self.rows_index(m)] ** 2).sum()] for m in range(self.nmb)])


def run(case, dtype):
    """The minibatch step of `case` at `dtype`: gradients, loss sums, d loss / d hidden and the per-row quantities the kinks sit on."""
    idx = torch.as_tensor(case.rows_index())
    t = lambda x: torch.as_tensor(x)[idx].to(dtype)     # noqa: E731
    p = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in case.params.items()}
    acts = torch.as_tensor(case.acts)[idx]
    hid_in = torch.as_tensor(case.h).to(dtype).clone().requires_grad_(True) if case.heads_only else None
    pre, hidden, newlogprob, entropy, newvalue = _policy_rows(p, None if case.heads_only else t(case.obs), acts, case.sizes, hidden=hid_in)
    if not case.heads_only:
        hidden.retain_grad()
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
    grads = {k: d(v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}     # (heads_only: no encoder)
    return dict(grads=grads, dh=d((hid_in if case.heads_only else hidden).grad),
                sums=np.array([d(x).sum() for x in (pg, v_rows, entropy, -logratio, (ratio - 1) - logratio, clipped)]),
                pre=None if pre is None else d(pre), ratio=d(ratio), newvalue=d(newvalue), val=d(val), ret=d(ret))


def kink_margins(r64, r32, case):
    """name -> (smallest float64 distance to the kink, fp32 chain error of the quantity the kink is on)."""
    out = {}
    if r64['pre'] is not None:
        out['relu'] = (float(np.abs(r64['pre']).min()), float(np.abs(r32['pre'] - r64['pre']).max()))
    out['ratio clip'] = (float(np.abs(np.abs(r64['ratio'] - 1.0) - case.clip_coef).min()), float(np.abs(r32['ratio'] - r64['ratio']).max()))
    if case.clip_vloss:
        e_v = float(np.abs(r32['newvalue'] - r64['newvalue']).max())
        delta = r64['newvalue'] - r64['val']
        out['value clip'] = (float(np.abs(np.abs(delta) - case.vf_clip_coef).min()), e_v)
        outside = np.abs(delta) > case.vf_clip_coef         # (inside, the two branches are the same function: no kink)
        du = r64['newvalue'] - r64['ret']
        dc = r64['val'] + np.clip(delta, -case.vf_clip_coef, case.vf_clip_coef) - r64['ret']
        tie = np.abs(np.abs(du) - np.abs(dc))[outside]
        out['value branch tie'] = (float(tie.min()) if tie.size else float('inf'), e_v)
    return out


class Reference:
    """float64 expected values of a case, the fp32 chain error per output, and the margins check."""

    def __init__(self, case, check=True):
        self.case = case
        self.r64, self.r32 = run(case, torch.float64), run(case, torch.float32)
        self.grads, self.sums, self.dh = self.r64['grads'], self.r64['sums'], self.r64['dh']
        self.e32 = {k: float(np.abs(self.r32['grads'][k] - v).max()) for k, v in self.grads.items()}
        self.e32['dh'] = float(np.abs(self.r32['dh'] - self.dh).max())
        self.margins = kink_margins(self.r64, self.r32, case)
        if check:
            self.check_margins()

    def margins_ok(self):
        return all(gap > MARGIN * err for gap, err in self.margins.values())

    def check_margins(self):
        for name, (gap, err) in self.margins.items():
            assert gap > MARGIN * err, f'{self.case.tag}: {name}: smallest distance {gap:.3e} vs {MARGIN:g} x {err:.3e}: choose another seed'

    def want(self, name):
        """The float64 expectation of a compared tensor."""
        return self.dh if name == 'dh' else self.grads[name]

    def bound(self, name):
        """max(4 e32, 1e-5 max|f64|): four fp32 chain errors, or the project's 1e-5 contract relative to the tensor's largest entry
        (the precedent of test_policy_call_matches_float64_within_four_fp32_chain_errors)."""
        return max(4.0 * self.e32[name], 1e-5 * float(np.abs(self.want(name)).max()))

    def compare(self, got, names=NAMES):
        """name -> (max |got - f64|, e32, bound) for every tensor of `got` (W1 without its padding columns, or 'dh')."""
        out = {}
        for k in names:
            want = self.want(k)
            g = np.asarray(got[k], np.float64).reshape(want.shape)
            err = float(np.abs(g - want).max()) if np.isfinite(g).all() else float('inf')
            out[k] = (err, self.e32[k], self.bound(k))
        return out

    def failures(self, got, names=NAMES, report=None):
        """The tensors of `got` that miss their bound; prints (or appends to `report`) one line per tensor."""
        bad = []
        for k, (err, e32, bound) in self.compare(got, names).items():
            line = f'[ppo grad f64] {self.case.tag:<44} {k:<18} err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}'
            print(line)
            if report is not None:
                report.append(line)
            if not err <= bound:
                bad.append(k)
        return bad

    def check_sums(self, tail16, rows=None):
        """The (hi, lo) pairs behind the gradient: six loss sums at rtol = atol = 1e-5 after division by the row count, the clipped
        count exactly."""
        tail = np.asarray(tail16, np.float64)
        got = tail[0:12:2] + tail[1:12:2]
        rows = rows or self.case.rows
        print(f'[ppo grad f64] {self.case.tag:<44} loss sums / rows: got {np.array2string(got / rows, precision=7)} want '
              f'{np.array2string(self.sums / rows, precision=7)}')
        np.testing.assert_allclose(got / rows, self.sums / rows, rtol=1e-5, atol=1e-5, err_msg=f'{self.case.tag}: loss sums')
        assert got[5] == self.sums[5], f'{self.case.tag}: clipped count {got[5]} != {self.sums[5]}'


# ------------------------------------------------------------------------------------------------------------------- committed cases
# pfa_ppo_mlp_grad: the 13 entries of with_grad_shape (csrc/ppo_update.hip) as (name, obs_dim, stride, actions, heads, rows per
# workgroup): rows of up to 64 floats run four 16-row tiles per workgroup, rows of 96 / 128 floats two.
MLP_SHAPES = [
    ('s16', 9, 16, 4, 0, 64), ('s16-md', 12, 16, 5, 0x23, 64),
    ('s32', 25, 32, 8, 0, 64), ('s32-md', 30, 32, 7, 0x34, 64),
    ('s96', 81, 96, 6, 0, 32), ('s96-md', 90, 96, 9, 0x432, 32),
    ('s128', 121, 128, 15, 0, 32), ('s128-md', 100, 128, 6, 0x24, 32),
    ('s64-md', 49, 64, 8, 0x53, 64),
    ('7x7-a8-perm', 49, 64, 8, 0, 64), ('7x7-a11-perm', 49, 64, 11, 0, 64),
    ('7x7-a12', 49, 64, 12, 0, 64), ('7x7-a15', 49, 64, 15, 0, 64),
    ('d50-13quads', 50, 64, 8, 0, 64), ('d60-generic', 60, 64, 8, 0, 64),
]
# seeds chosen on the CPU (Reference.margins_ok) so that the float64 reference alone is clear of every kink: the first of 1, 2, 3, ...
# that is; seed 1 unless listed here
SEEDS = {'s16-md-3wg-mb1of2-bptt4': 2, 's96-3wg-mb1of2-bptt4': 3, 's64-md-3wg-mb1of2-bptt4': 3, '7x7-a8-perm-3wg-mb1of2-bptt4': 3,
         '7x7-a11-perm-3wg-mb1of2-bptt4': 2, '7x7-a12-3wg-mb1of2-bptt4': 2}


def _seed(tag):
    return SEEDS.get(tag, 1)


def mlp_cases():
    """Per shape: one workgroup of whole tiles in one minibatch; three workgroups as minibatch 1 of 2 with segments of 4 rows (the
    strided segment map, tiles that straddle segments).  Then: tiles that do not fill the last workgroup's wavefront pairs, norm_adv
    off, clip_vloss off."""
    out = []
    for name, d, dp, a, heads, per_wg in MLP_SHAPES:
        for tag, kw in ((f'{name}-1wg', dict(rows=per_wg)), (f'{name}-3wg-mb1of2-bptt4', dict(rows=3 * per_wg, nmb=2, mb=1, horizon=4))):
            out.append(Case(tag, d, dp, a, heads, seed=_seed(tag), **kw))
    for tag, args, kw in (('7x7-a8-perm-5tiles', (49, 64, 8, 0), dict(rows=80)), ('s128-3tiles', (121, 128, 15, 0), dict(rows=48)),
                          ('7x7-a8-perm-no-norm-adv', (49, 64, 8, 0), dict(rows=64, norm_adv=0)),
                          ('s32-md-no-norm-adv', (30, 32, 7, 0x34), dict(rows=64, norm_adv=0)),
                          ('7x7-a12-no-clip-vloss', (49, 64, 12, 0), dict(rows=64, clip_vloss=0)),
                          ('s96-no-clip-vloss', (81, 96, 6, 0), dict(rows=32, clip_vloss=0))):
        out.append(Case(tag, *args, seed=_seed(tag), **kw))
    return out


def bf16_cases():
    """The opt-in bf16x6 product form: the two 7x7 shapes on minibatches of whole 32-row tiles."""
    out = []
    for name, a in (('7x7-a8-perm', 8), ('7x7-a12', 12)):
        for tag, kw in ((f'bf16x6-{name}-64rows', dict(rows=64)), (f'bf16x6-{name}-96rows-mb1of2-bptt4', dict(rows=96, nmb=2, mb=1, horizon=4))):
            out.append(Case(tag, 49, 64, a, 0, seed=_seed(tag), **kw))
    return out


def wide_cases():
    """pfa_ppo_wide_grad: the (hidden, grid) pairs test_wide_default_policy_rollout_and_update_vs_oracle trains through it (grid d: d*d*...
    = 9 / 25 / 49 columns on rows of 16 / 32 / 64 floats), 16 and 48 rows per minibatch, minibatch 1 of 2."""
    out = []
    for hidden, d in ((64, 3), (256, 3), (512, 3), (256, 1), (64, 2)):
        side = 2 * d + 1
        dim = side * side
        stride = 16 * ((dim + 15) // 16)
        for rows, hz in ((16, 8), (48, 4)):
            tag = f'wide-h{hidden}-grid{side}x{side}-{rows}rows'
            out.append(Case(tag, dim, stride, 8, 0, rows=rows, nmb=2, mb=1, horizon=hz, hidden=hidden, seed=_seed(tag)))
    return out


def heads_cases():
    """pfa_lstm_heads_loss: 70 time-major rows (no multiple of 16) of random h, 8 actions, minibatch 1 of 2; and MultiDiscrete heads."""
    return [Case('lstm-heads-70rows', 49, 64, 8, 0, rows=70, nmb=2, mb=1, horizon=5, time_major=True, heads_only=True, seed=_seed('lstm-heads-70rows')),
            Case('lstm-heads-md-72rows', 12, 16, 5, 0x23, rows=72, nmb=2, mb=0, horizon=4, time_major=True, heads_only=True,
                 seed=_seed('lstm-heads-md-72rows'))]


def all_cases():
    return mlp_cases() + bf16_cases() + wide_cases() + heads_cases()
