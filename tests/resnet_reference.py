"""pufferlib.models.ProcgenResnet (models.py:159-231) as data and arithmetic for the tests: the frame shapes, deterministic frames and
start weights, a stub env, a reference-shaped twin module, and the reference's forward (`permute(0, 3, 1, 2) / 255.0`, three
ConvSequences of conv - max_pool2d(3, 2, 1) - two residual blocks, Flatten - ReLU - Linear - ReLU, the two heads) restated with
torch.nn.functional on the CPU — in float64 for the expected values, in float32 for the error an fp32 chain of this depth makes —
plus the PPO loss of clean_pufferl.py:202-238 and, through autograd, every parameter and activation gradient.  Imports neither the
package under test nor the reference: the GPU tests run where only this repository exists."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import conv_geometry as cg

ACTIONS = 15
# tag -> frame shape (H, W, C) uint8, widths.  tiny: odd sizes, every pool window ragged, maps 9x7 -> 5x4 -> 3x2 -> 2x1 (in the last
# sequence every tap but the centre column is padding); rgba: four channels (one k-quad = one pixel of the first layer), mlp_width 128
SHAPES = {
    'tiny': dict(obs=(9, 7, 3), cnn_width=16, mlp_width=256),
    'procgen': dict(obs=(64, 64, 3), cnn_width=16, mlp_width=256),
    'rgba': dict(obs=(9, 7, 4), cnn_width=16, mlp_width=128),
}
# frame seeds chosen on the CPU so that the float64 reference alone is clear of near ties (see check_margins / sampling rows)
FRAME_SEED = {'tiny': 782, 'procgen': 777, 'rgba': 780}
SEQ_NAMES = ('c', 'p', 't0', 'x1', 't1', 'x2')


def frame(tag, counter):
    rs = np.random.RandomState(FRAME_SEED[tag] + 7919 * (zlib.crc32(tag.encode()) % 1000) + int(counter))
    return rs.randint(0, 256, SHAPES[tag]['obs']).astype(np.uint8)


def frames(tag, n, first=0):
    return np.stack([frame(tag, first + i) for i in range(n)])


def start_weight(name, shape, seed=4242):
    """Deterministic start value of parameter `name`: the recipe of conv_geometry.start_weight with gain 1 for every layer — at the
    reference's actor gain of 0.01 the logits are ~1e-3 and every comparison of probabilities would pass whatever the encoder
    computed; sqrt(2) through ten residual additions would saturate them instead."""
    rs = np.random.RandomState(seed + zlib.crc32(name.encode()) % 100000)
    if name.endswith('bias'):
        return (0.01 * rs.standard_normal(shape)).astype(np.float32)
    return (1.0 / np.sqrt(np.prod(shape[1:])) * rs.standard_normal(shape)).astype(np.float32)


def spec(tag):
    """The entry of SHAPES that `tag` names; a dict of the same form (obs, cnn_width, mlp_width) stands for itself, so a test can ask
    for a shape that has no name."""
    return SHAPES[tag] if isinstance(tag, str) else tag


def seq_sizes(tag):
    """(IC, H, W, OC, PH, PW) per ConvSequence."""
    h, w, c = spec(tag)['obs']
    cw = spec(tag)['cnn_width']
    out, ic = [], c
    for oc in (cw, 2 * cw, 2 * cw):
        ph, pw = (h + 1) // 2, (w + 1) // 2
        out.append((ic, h, w, oc, ph, pw))
        ic, h, w = oc, ph, pw
    return out


def flat_size(tag):
    _, _, _, oc, ph, pw = seq_sizes(tag)[-1]
    return oc * ph * pw


def param_shapes(tag, num_actions=ACTIONS):
    """name -> shape in named_parameters() order."""
    out = {}
    for i, (ic, _, _, oc, _, _) in enumerate(seq_sizes(tag)):
        out[f'network.{i}.conv.weight'], out[f'network.{i}.conv.bias'] = (oc, ic, 3, 3), (oc,)
        for b in (0, 1):
            for c in (0, 1):
                out[f'network.{i}.res_block{b}.conv{c}.weight'], out[f'network.{i}.res_block{b}.conv{c}.bias'] = (oc, oc, 3, 3), (oc,)
    mlp = spec(tag)['mlp_width']
    out['network.5.weight'], out['network.5.bias'] = (mlp, flat_size(tag)), (mlp,)
    out['actor.weight'], out['actor.bias'] = (num_actions, mlp), (num_actions,)
    out['value.weight'], out['value.bias'] = (1, mlp), (1,)
    return out


def start_weights(tag, num_actions=ACTIONS):
    return {k: start_weight(k, sh) for k, sh in param_shapes(tag, num_actions).items()}


class Env:
    """Stub env: what models.ProcgenResnet reads from one."""

    def __init__(self, tag, num_actions=ACTIONS, obs=None, dtype=np.uint8):
        self.single_observation_space = type('Box', (), {'shape': obs or spec(tag)['obs'], 'dtype': dtype})()
        self.single_action_space = type('Discrete', (), {'n': num_actions})()


def reference_module(tag, num_actions=ACTIONS):
    """A torch module with the reference class's attribute names, parameter names and shapes (models.py:159-231), built here; it
    records no frame shape, like the reference's."""
    import torch.nn as nn
    mlp = spec(tag)['mlp_width']

    class ResidualBlock(nn.Module):
        def __init__(self, ch):
            super().__init__()
            self.conv0, self.conv1 = nn.Conv2d(ch, ch, 3, padding=1), nn.Conv2d(ch, ch, 3, padding=1)

    class ConvSequence(nn.Module):
        def __init__(self, ic, oc):
            super().__init__()
            self.conv = nn.Conv2d(ic, oc, 3, padding=1)
            self.res_block0, self.res_block1 = ResidualBlock(oc), ResidualBlock(oc)

    class ProcgenResnet(nn.Module):
        def __init__(self):
            super().__init__()
            seqs = [ConvSequence(ic, oc) for ic, _, _, oc, _, _ in seq_sizes(tag)]
            self.network = nn.Sequential(*seqs, nn.Flatten(), nn.ReLU(), nn.Linear(flat_size(tag), mlp), nn.ReLU())
            self.actor = nn.Linear(mlp, num_actions)
            self.value = nn.Linear(mlp, 1)
    return ProcgenResnet()


def _pool_gap(c):
    """Smallest (best - second best) over the 3 x 3 / stride 2 / padding 1 windows of c [n][C][H][W], in-image taps only."""
    n, ch, h, w = c.shape
    padded = F.pad(c.detach(), (1, 1, 1, 1), value=-float('inf'))
    win = F.unfold(padded, kernel_size=3, stride=2).view(n, ch, 9, -1)
    top = win.topk(2, dim=2).values
    gap = top[:, :, 0] - top[:, :, 1]
    return float(gap.min())


def encode(tag, frames_u8, w, dtype=torch.float64, info=None):
    """models.py:188-190 + the network.  frames_u8: (n, H, W, C) uint8 tensor; w: name -> tensor of `dtype`.  Returns (maps, hidden):
    maps[i][name] for name in SEQ_NAMES (NCHW; x2 of the last sequence BEFORE Flatten's ReLU).  info (a dict) receives 'kink', the
    smallest |ReLU input|, and 'pool_gap', the smallest top-two gap of a pool window."""
    x = frames_u8.permute(0, 3, 1, 2).to(dtype) / 255.0
    maps, kinks, gaps = [], [], []
    for i in range(3):
        pre = f'network.{i}.'
        m = {}
        m['c'] = F.conv2d(x, w[pre + 'conv.weight'], w[pre + 'conv.bias'], padding=1)
        m['p'] = F.max_pool2d(m['c'], kernel_size=3, stride=2, padding=1)
        m['t0'] = F.conv2d(F.relu(m['p']), w[pre + 'res_block0.conv0.weight'], w[pre + 'res_block0.conv0.bias'], padding=1)
        m['x1'] = F.conv2d(F.relu(m['t0']), w[pre + 'res_block0.conv1.weight'], w[pre + 'res_block0.conv1.bias'], padding=1) + m['p']
        m['t1'] = F.conv2d(F.relu(m['x1']), w[pre + 'res_block1.conv0.weight'], w[pre + 'res_block1.conv0.bias'], padding=1)
        m['x2'] = F.conv2d(F.relu(m['t1']), w[pre + 'res_block1.conv1.weight'], w[pre + 'res_block1.conv1.bias'], padding=1) + m['x1']
        maps.append(m)
        x = m['x2']
        kinks += [float(m[k].detach().abs().min()) for k in ('p', 't0', 'x1', 't1')]
        gaps.append(_pool_gap(m['c']))
    kinks.append(float(x.detach().abs().min()))
    z = F.linear(F.relu(x.flatten(1)), w['network.5.weight'], w['network.5.bias'])
    kinks.append(float(z.detach().abs().min()))
    if info is not None:
        info['kink'], info['pool_gap'] = min(kinks), min(gaps)
    return maps, F.relu(z)


def heads(h, w, actions=None, noise=None):
    """decode_actions + sample_logits: conv_geometry.heads with the ResNet's name for the value head."""
    return cg.heads(h, {'actor.weight': w['actor.weight'], 'actor.bias': w['actor.bias'], 'value_fn.weight': w['value.weight'],
                        'value_fn.bias': w['value.bias']}, actions=actions, noise=noise)


ppo_loss = cg.ppo_loss


def reference_forward_backward(tag, frames_u8, weights, hidden_grad=None, batch=None, dtype=torch.float64, **hparams):
    """Forward (maps NCHW, hidden, logits, values) and gradients of every parameter and every kept map, in `dtype`.  The scalar
    differentiated: sum(hidden * hidden_grad) when `hidden_grad` is given (layer tests), else the PPO loss on `batch` = dict(actions,
    logprobs, values, advantages, returns) (update tests); neither: forward only."""
    w = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in weights.items()}
    x = torch.as_tensor(np.asarray(frames_u8))
    info = {}
    maps, h = encode(tag, x, w, dtype, info)
    for m in maps:
        for t in m.values():
            t.retain_grad()
    out = dict(maps=maps, h=h, kink=info['kink'], pool_gap=info['pool_gap'])
    if hidden_grad is not None:
        (h * torch.as_tensor(np.asarray(hidden_grad)).to(dtype)).sum().backward()
    elif batch is not None:
        b = {k: torch.as_tensor(np.asarray(v)) for k, v in batch.items()}
        logits, value, _, logprob, entropy, _ = heads(h, w, actions=b['actions'])
        loss, pg, vl, ent = ppo_loss(logprob, entropy, value, b['logprobs'].to(dtype), b['values'].to(dtype), b['advantages'].to(dtype),
                                     b['returns'].to(dtype), **hparams)
        loss.backward()
        out.update(logits=logits, value=value, logprob=logprob, entropy=entropy, loss=loss, pg_loss=pg, v_loss=vl, entropy_loss=ent)
    else:
        logits, value, _, _, _, _ = heads(h, w, actions=torch.zeros(h.shape[0], dtype=torch.long))
        out.update(logits=logits, value=value)
    out['grads'] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()}
    return out


def policy_outputs(tag, frames_u8, weights, noise, dtype=torch.float64):
    """policy(frames, noise=...) restated: dict of hidden, logits, value, action, logprob, entropy, gap (numpy, `dtype`)."""
    w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in weights.items()}
    with torch.no_grad():
        _, h = encode(tag, torch.as_tensor(np.asarray(frames_u8)), w, dtype)
        logits, value, action, logprob, entropy, gap = heads(h, w, noise=torch.as_tensor(np.asarray(noise)))
    return dict(hidden=h.numpy(), logits=logits.numpy(), value=value.numpy(), action=action.numpy(), logprob=logprob.numpy(),
                entropy=entropy.numpy(), gap=gap.numpy())


def fp32_chain_error(tag, frames_u8, weights, noise):
    """What an fp32 chain of this depth loses: the restatement in float32 on the CPU against float64, max |difference| per output.
    Also returns the float64 outputs.  Asserts, in float64, that every sampling row is clear of a tie (gap > 1e-4: the rule of
    tests/golden/make_golden_conv.py), so that actions can be compared exactly."""
    want = policy_outputs(tag, frames_u8, weights, noise, torch.float64)
    assert float(want['gap'].min()) > 1e-4, f'{tag}: a sampling row is a near tie ({float(want["gap"].min()):.3e}): choose another seed'
    got = policy_outputs(tag, frames_u8, weights, noise, torch.float32)
    err = {k: float(np.abs(got[k].astype(np.float64) - want[k]).max()) for k in ('hidden', 'logits', 'value', 'logprob', 'entropy')}
    return err, want


def noise_for(tag, n, seed=5):
    """Exp(1) draws [n][ACTIONS] standing for torch.multinomial's."""
    return torch.empty(n, ACTIONS).exponential_(1, generator=torch.Generator().manual_seed(seed + zlib.crc32(tag.encode()) % 1000)).numpy()


def check_margins(ref, chain_error):
    """Elementwise activation-gradient checks are meaningful only where fp32 rounding cannot flip a ReLU or move a pool's argmax: the
    float64 reference's smallest |ReLU input| and smallest pool top-two gap must both exceed 16x the fp32 chain error."""
    assert ref['kink'] > 16 * chain_error, f'smallest |ReLU input| {ref["kink"]:.3e} vs 16 x {chain_error:.3e}: choose another seed'
    assert ref['pool_gap'] > 16 * chain_error, f'smallest pool gap {ref["pool_gap"]:.3e} vs 16 x {chain_error:.3e}: choose another seed'


# ------------------------------------------------------------------------------------------ the host route (GPU tests)
class Replay:
    """Host vecenv (the reference's recv / send protocol) that hands out a recorded stream of frames [T][N][bytes], rewards and dones
    [T][N], at any frame shape."""

    def __init__(self, obs, rewards, dones, shape, num_actions=ACTIONS):
        from pufferlib_amd import spaces
        self.obs, self.rew, self.done = obs, rewards, dones
        n = obs.shape[1]
        self.single_observation_space = spaces.Box(low=0, high=255, shape=tuple(shape), dtype=np.uint8)
        self.single_action_space = spaces.Discrete(num_actions)
        self.driver_env = self
        self.num_envs = self.num_agents = self.agents_per_batch = n
        self.emulated = True
        self.t = 0

    def async_reset(self, seed=42):
        pass

    def recv(self):
        n, t = self.num_envs, self.t % self.obs.shape[0]
        return (self.obs[t].reshape(n, *self.single_observation_space.shape).copy(), self.rew[t].copy(), self.done[t].astype(bool),
                np.zeros(n, bool), [], np.arange(n), np.ones(n, bool))

    def send(self, actions):
        self.t += 1

    def close(self):
        pass


def time_major(x, n, horizon):
    """env-major experience rows (a device tensor) -> numpy [T][N]..."""
    return x.view(n, horizon, *x.shape[1:]).transpose(0, 1).contiguous().cpu().numpy()


def digest(a, samples=64):
    """Sum, sum of magnitudes and `samples` evenly spaced elements: how tests/golden/make_golden_resnet.py records a big tensor."""
    f = np.asarray(a, np.float64).reshape(-1)
    idx = np.linspace(0, f.size - 1, min(samples, f.size)).astype(np.int64)
    return np.concatenate([[f.sum(), np.abs(f).sum()], f[idx]])


# ------------------------------------------------------------------------------------------ brute-force geometry (CPU tests)
def brute_pool_out(size):
    """Windows of max_pool2d(kernel 3, stride 2, padding 1) along one axis, by enumeration over the padded axis."""
    return len([o for o in range(size + 2) if 2 * o + 3 <= size + 2])


def brute_same_conv_out(size):
    return len([o for o in range(size + 2) if o + 3 <= size + 2])


def brute_geometry(obs_shape, cnn_width):
    """Per sequence (IC, H, W, OC, PH, PW), the flatten width and the byte strides of a channel-last frame, by enumeration."""
    h, w, c = obs_shape
    idx = np.arange(h * w * c).reshape(obs_shape).transpose(2, 0, 1)
    strides = tuple(int(idx[a] - idx[0, 0, 0]) if ok else None for a, ok in (((1, 0, 0), c > 1), ((0, 1, 0), h > 1), ((0, 0, 1), w > 1)))
    seqs, ic = [], c
    for oc in (cnn_width, 2 * cnn_width, 2 * cnn_width):
        assert brute_same_conv_out(h) == h and brute_same_conv_out(w) == w
        ph, pw = brute_pool_out(h), brute_pool_out(w)
        seqs.append((ic, h, w, oc, ph, pw))
        ic, h, w = oc, ph, pw
    return dict(seqs=seqs, flat=ic * h * w, strides=strides, frame_bytes=int(idx.max()) + 1)
