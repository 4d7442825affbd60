"""CPU reference of tests/test_gpu_conv_autograd.py: pufferlib.models.Convolutional scored with given actions — the arithmetic of
tests/conv_geometry.py (its frames, start weights and heads; its encode restated here with a dtype argument, and asserted equal to it in
float64) under torch autograd.  In float64 it is the expected value of what cleanrl.Policy(models.Convolutional(...), autograd=True)
returns and back-propagates; in float32 it measures what an fp32 chain of this depth loses against float64 (`e32`).  The bound of every
comparison is autograd_reference.bound(e32, f64) = max(4 e32, 1e-5 max(1, max |f64|)) per tensor: taken from this file, never from the
code under test.

Losses: a linear one with fixed random per-row coefficients on (logprob, entropy, value), one on the value alone (the other two upstream
gradients then arrive as None), and the PPO loss of conv_geometry.ppo_loss.

Gradients are discontinuous where a ReLU input is 0 and, for the PPO loss, where the ratio sits on 1 +- clip_coef, where
newvalue - val sits on +- vf_clip_coef and where the two value-loss branches tie.  A conv batch has ~10^4 ReLU units per frame, so the
nearest one lies within a few fp32 chain errors of its kink whatever the seed (37 crafter frames: 4 x 10^5 units, the nearest to 0
typically at 1e-6 .. 1e-5, the largest fp32 chain error of a pre-activation 2e-6 .. 3e-6 — on the units of magnitude ~5): the rule
of autograd_reference (16 times the largest chain error) is out of reach there.  margins() therefore measures, per layer, the fp32 chain
error where it matters — the largest over the NEAR = 1000 units nearest to 0 — and check_margins() asserts RELU_MARGIN = 4 of those (the
factor of the bound rule: a device whose pre-activations are as exact as the CPU's fp32 ones does not flip a unit), and the 16 of
autograd_reference for the per-row PPO kinks.  Cases are (tag, rows, first frame number): the first frame numbers below are among
0, 100, 200, ... ones at which every loss passes on the CPU (find_first()).  The one batch whose frames a test cannot choose — the 128
frames a device rollout leaves (1.4 x 10^6 units; of env seeds 1 .. 14 none kept even one chain error in every layer, the best, seed 2,
1.9 / 14.8 / 6.1 / 11.9) — is checked on the per-row kinks only (check_margins(relu=False)): there the CPU's own fp32 run flips units
too, and what that does to the result is part of e32.
Imports nothing of the package under test."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import autograd_reference as R  # noqa: E402
import conv_geometry as cg  # noqa: E402

bound = R.bound
RELU_MARGIN = 4.0
NEAR = 1000
ROW_MARGIN = R.MARGIN
PPO = dict(clip_coef=0.1, vf_clip_coef=0.1, vf_coef=0.5, ent_coef=0.01)
ACTOR_SCALE = 100.0          # the 0.01-gain start logits are all but uniform: spread them (as tests/test_gpu_conv_geometry.py does)


def weights(tag, num_actions):
    w = cg.start_weights(tag, num_actions)
    w['actor.weight'] = (w['actor.weight'] * ACTOR_SCALE).astype(np.float32)
    return w


def encode(tag, frames_u8, w, dtype):
    """conv_geometry.encode at `dtype`: (hidden, [the four ReLU inputs])."""
    kw = cg.GEOMETRIES[tag]['kwargs']
    x = frames_u8
    if kw.get('channels_last', False):
        x = x.permute(0, 3, 1, 2)
    d = kw.get('downsample', 1)
    if d > 1:
        x = x[:, :, ::d, ::d]
    x = x.to(dtype) / 255.0
    z1 = F.conv2d(x, w['network.0.weight'], w['network.0.bias'], stride=4)
    z2 = F.conv2d(F.relu(z1), w['network.2.weight'], w['network.2.bias'], stride=2)
    z3 = F.conv2d(F.relu(z2), w['network.4.weight'], w['network.4.bias'], stride=1)
    z4 = F.linear(F.relu(z3).flatten(1), w['network.7.weight'], w['network.7.bias'])
    return F.relu(z4), [z1, z2, z3, z4]


class Case:
    """One geometry, `rows` frames from frame number `first`, given actions, and the per-row numbers the losses read."""

    def __init__(self, tag, rows, num_actions=4, first=0, seed=1, w=None, frames=None, actions=None):
        self.tag, self.rows, self.A, self.first = tag, rows, num_actions, first
        self.name = f'{tag}-A{num_actions}-n{rows}'
        self.params = weights(tag, num_actions) if w is None else {k: np.ascontiguousarray(v, np.float32) for k, v in w.items()}
        self.names = list(self.params)
        self.frames = cg.frames(tag, rows, first=first) if frames is None else np.ascontiguousarray(frames, np.uint8)
        rs = np.random.RandomState(seed)
        f32 = np.float32
        self.acts = rs.randint(0, num_actions, rows).astype(np.int64) if actions is None else np.asarray(actions, np.int64).reshape(rows)
        self.u, self.v, self.w = (rs.standard_normal(rows).astype(f32) for _ in range(3))
        # a PPO minibatch: old log-probabilities and values = the float64 policy's own + noise, so ratios leave 1
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


def forward(case, dtype, actions=None):
    """The policy call at `dtype`: dict(params (leaf tensors), pre (the ReLU inputs), logprob, entropy, value [rows][1])."""
    p = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in case.params.items()}
    h, pre = encode(case.tag, torch.as_tensor(case.frames), p, dtype)
    acts = torch.as_tensor(case.acts if actions is None else np.asarray(actions, np.int64))
    _, value, _, logprob, entropy, _ = cg.heads(h, p, actions=acts)
    return dict(params=p, pre=pre, logprob=logprob, entropy=entropy, value=value.unsqueeze(1))


def _t(x, like):
    return torch.as_tensor(x).to(device=like.device, dtype=like.dtype)


def linear_loss(case, logprob, entropy, value):
    return (_t(case.u, logprob) * logprob + _t(case.v, logprob) * entropy + _t(case.w, logprob) * value.reshape(-1)).sum()


def value_loss(case, logprob, entropy, value):
    """Reads the value alone: the upstream gradients of logprob and entropy are None."""
    return (_t(case.w, value) * value.reshape(-1)).sum()


def ppo_loss(case, logprob, entropy, value):
    """conv_geometry.ppo_loss (clean_pufferl.py:202-238) on the case's minibatch, in torch ops on the returned tensors."""
    return cg.ppo_loss(logprob, entropy, value.reshape(-1), _t(case.logprobs, logprob), _t(case.values, logprob), _t(case.advantages, logprob),
                       _t(case.returns, logprob), **PPO)[0]


def run(case, loss, dtype):
    """Forward + loss + backward at dtype: outputs and gradients as float64 numpy, and the quantities the kinks sit on."""
    out = forward(case, dtype)
    value = loss(case, out['logprob'], out['entropy'], out['value'])
    value.backward()
    d = lambda x: x.detach().double().numpy()           # noqa: E731
    grads = {k: (d(v.grad) if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in out['params'].items()}
    res = dict(grads=grads, pre=[d(z) for z in out['pre']], loss=value.item(), outputs={k: d(out[k]) for k in ('logprob', 'entropy', 'value')},
               parts={})
    if loss is ppo_loss:
        res['parts'] = dict(ratio=np.exp(res['outputs']['logprob'] - case.logprobs.astype(np.float64)), newvalue=res['outputs']['value'].reshape(-1),
                            val=case.values.astype(np.float64), ret=case.returns.astype(np.float64))
    return res


def optimizer_step(case, dtype, lr, max_grad_norm):
    """One whole custom-loop step at dtype (autograd_reference.optimizer_step for this policy): the policy call, the PPO loss, backward,
    clip_grad_norm_, Adam(lr, eps=1e-5).step().  Returns the updated parameters as float64 numpy."""
    out = forward(case, dtype)
    params = [out['params'][k] for k in case.names]
    opt = torch.optim.Adam(params, lr=lr, eps=1e-5)
    ppo_loss(case, out['logprob'], out['entropy'], out['value']).backward()
    torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
    opt.step()
    return {k: p.detach().double().numpy() for k, p in zip(case.names, params)}


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
        """name -> (smallest float64 distance to the kink, fp32 chain error of the quantity the kink is on, required ratio)."""
        r64, r32 = self.r64, self.r32
        out = {}
        for i, (z64, z32) in enumerate(zip(r64['pre'], r32['pre'])):
            near = np.argsort(np.abs(z64), axis=None)[:NEAR]
            out[f'relu {i + 1}'] = (float(np.abs(z64).flat[near[0]]), float(np.abs(z32 - z64).flat[near].max()), RELU_MARGIN)
        if r64['parts']:
            p64, p32 = r64['parts'], r32['parts']
            out['ratio clip'] = (float(np.abs(np.abs(p64['ratio'] - 1.0) - PPO['clip_coef']).min()), float(np.abs(p32['ratio'] - p64['ratio']).max()), ROW_MARGIN)
            e_v = float(np.abs(p32['newvalue'] - p64['newvalue']).max())
            delta = p64['newvalue'] - p64['val']
            out['value clip'] = (float(np.abs(np.abs(delta) - PPO['vf_clip_coef']).min()), e_v, ROW_MARGIN)
            outside = np.abs(delta) > PPO['vf_clip_coef']         # (inside, the two branches are the same function: no kink)
            du = p64['newvalue'] - p64['ret']
            dc = p64['val'] + np.clip(delta, -PPO['vf_clip_coef'], PPO['vf_clip_coef']) - p64['ret']
            tie = np.abs(np.abs(du) - np.abs(dc))[outside]
            out['value branch tie'] = (float(tie.min()) if tie.size else float('inf'), e_v, ROW_MARGIN)
        return out

    def margins_ok(self):
        return all(gap > need * err for gap, err, need in self.margins().values())

    def check_margins(self, relu=True):
        """relu=False: the per-row PPO kinks only (a batch whose frames the test cannot choose: module docstring)."""
        for name, (gap, err, need) in self.margins().items():
            if not relu and name.startswith('relu'):
                continue
            assert gap > need * err, f'{self.case.name}: {name}: smallest distance {gap:.3e} vs {need:g} x {err:.3e}: choose another first frame'

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
            scaled = 2e-5 * max(1.0, float(np.abs(want).max()))      # the least _close_scaled (tests/test_gpu_conv_geometry.py) allows any entry
            print(f'[conv autograd f64] {self.case.name:<20} {self.loss.__name__:<11} {what:<5} {k:<17} cpu-fp32 err {e_all[k]:.3e}  device err {err:.3e}  '
                  f'bound {b:.3e}  err/bound {err / b:.3f}  (_close_scaled allows >= {scaled:.3e})')
            if not err <= b:
                bad.append(k)
        return bad


# ------------------------------------------------------------------------------------------------------------------- committed cases
# crafter: hidden 128, 3 channels through the byte loader; vizdoom: hidden 512, 1 channel.  3 rows: one partial 16-row tile; 37: two full
# tiles and a partial one.  (tag, rows) -> first frame number (find_first()).
FIRST = {('crafter', 3): 0, ('vizdoom', 3): 0, ('crafter', 37): 0, ('vizdoom', 37): 700}
OTHER = {'crafter': 700, 'vizdoom': 400}      # a second batch of 37 frames for the interleaving test (linear loss)


def case(tag, rows, first=None):
    return Case(tag, rows, 4, FIRST[(tag, rows)] if first is None else first)


def find_first():
    """Development aid: the first frame number per case at which every loss is clear of every kink."""
    torch.set_num_threads(8)
    for tag, rows, start in [k + (0,) for k in FIRST] + [(t, 37, FIRST[(t, 37)] + 100) for t in OTHER]:
        for first in range(start, start + 4000, 100):
            c = Case(tag, rows, 4, first)
            refs = [Reference(c, loss, check=False) for loss in (linear_loss, ppo_loss)]
            if all(r.margins_ok() for r in refs):
                print('->', tag, rows, first, flush=True)
                break


if __name__ == '__main__':
    find_first()
