"""The frame geometries pufferlib.models.Convolutional is bound to by the reference's environment packages
(pufferlib/environments/{atari,vizdoom,pokemon_red,links_awaken,crafter,dm_lab,butterfly}/torch.py), as data, with deterministic
frames and start weights per geometry and the reference's arithmetic (models.py:147-157: permute for channel-last frames, strided
downsample, `.float() / 255.0`, the NatureCNN, the two heads) restated with torch.nn.functional on the CPU in float64, plus the PPO
loss of clean_pufferl.py:202-238 and — through autograd — every parameter gradient.  Imports neither the package under test nor the
reference: the GPU tests run where only this repository exists."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# tag -> observation shape (uint8), constructor arguments, conv1 / conv2 / conv3 output (H, W)
GEOMETRIES = {
    'atari': dict(obs=(4, 84, 84), kwargs=dict(framestack=4, flat_size=3136), outs=((20, 20), (9, 9), (7, 7))),
    'vizdoom': dict(obs=(60, 80, 1), kwargs=dict(framestack=1, flat_size=64 * 4 * 6, channels_last=True), outs=((14, 19), (6, 8), (4, 6))),
    'pokemon': dict(obs=(72, 80, 4), kwargs=dict(framestack=4, flat_size=64 * 5 * 6, channels_last=True), outs=((17, 19), (7, 8), (5, 6))),
    'links': dict(obs=(72, 80, 3), kwargs=dict(framestack=3, flat_size=64 * 5 * 6, channels_last=True), outs=((17, 19), (7, 8), (5, 6))),
    'crafter': dict(obs=(64, 64, 3), kwargs=dict(framestack=3, flat_size=1024, channels_last=True, hidden_size=128, output_size=128),
                    outs=((15, 15), (6, 6), (4, 4))),
    'dm_lab': dict(obs=(84, 84, 3), kwargs=dict(framestack=3, flat_size=3136, channels_last=True, hidden_size=128, output_size=128),
                   outs=((20, 20), (9, 9), (7, 7))),
    'butterfly': dict(obs=(280, 480, 3), kwargs=dict(framestack=3, flat_size=3520, channels_last=True, downsample=4, hidden_size=128,
                                                      output_size=128), outs=((16, 29), (7, 13), (5, 11))),
}
NEW = [t for t in GEOMETRIES if t != 'atari']


def hidden_of(tag):
    return GEOMETRIES[tag]['kwargs'].get('hidden_size', 512)


def frame(tag, counter, base_seed=777):
    """Frame number `counter` of geometry `tag`: uint8 of the observation shape, deterministic."""
    rs = np.random.RandomState(base_seed + 7919 * (zlib.crc32(tag.encode()) % 1000) + int(counter))
    return rs.randint(0, 256, GEOMETRIES[tag]['obs']).astype(np.uint8)


def frames(tag, n, first=0):
    return np.stack([frame(tag, first + i) for i in range(n)])


def start_weight(name, shape, seed=4242):
    """Deterministic start value of parameter `name` (the recipe of cnn_golden.cnn_start_weight)."""
    rs = np.random.RandomState(seed + zlib.crc32(name.encode()) % 100000)
    if name.endswith('bias') or name.startswith('bias_'):
        return (0.01 * rs.standard_normal(shape)).astype(np.float32)
    gain = 0.01 if 'actor' in name else 1.0 if ('value_fn' in name or name.startswith('weight_')) else np.sqrt(2)
    return (gain / np.sqrt(np.prod(shape[1:])) * rs.standard_normal(shape)).astype(np.float32)


def param_shapes(tag, num_actions):
    kw = GEOMETRIES[tag]['kwargs']
    c, flat, hid = kw['framestack'], kw['flat_size'], kw.get('hidden_size', 512)
    return {'network.0.weight': (32, c, 8, 8), 'network.0.bias': (32,), 'network.2.weight': (64, 32, 4, 4), 'network.2.bias': (64,),
            'network.4.weight': (64, 64, 3, 3), 'network.4.bias': (64,), 'network.7.weight': (hid, flat), 'network.7.bias': (hid,),
            'actor.weight': (num_actions, hid), 'actor.bias': (num_actions,), 'value_fn.weight': (1, hid), 'value_fn.bias': (1,)}


def start_weights(tag, num_actions):
    return {k: start_weight(k, sh) for k, sh in param_shapes(tag, num_actions).items()}


class Env:
    """Stub env: what models.Convolutional reads from one."""

    def __init__(self, tag, num_actions):
        self.single_observation_space = type('Box', (), {'shape': GEOMETRIES[tag]['obs'], 'dtype': np.uint8})()
        self.single_action_space = type('Discrete', (), {'n': num_actions})()


def reference_module(tag, num_actions):
    """A torch module with the reference class's attribute names, parameter names and shapes (models.py:113-140), built here."""
    import torch.nn as nn
    kw = GEOMETRIES[tag]['kwargs']
    hid = kw.get('hidden_size', 512)

    class Convolutional(nn.Module):
        def __init__(self):
            super().__init__()
            self.channels_last, self.downsample = kw.get('channels_last', False), kw.get('downsample', 1)
            self.network = nn.Sequential(nn.Conv2d(kw['framestack'], 32, 8, stride=4), nn.ReLU(), nn.Conv2d(32, 64, 4, stride=2), nn.ReLU(),
                                         nn.Conv2d(64, 64, 3, stride=1), nn.ReLU(), nn.Flatten(), nn.Linear(kw['flat_size'], hid), nn.ReLU())
            self.actor = nn.Linear(hid, num_actions)
            self.value_fn = nn.Linear(kw.get('output_size', 512), 1)
    return Convolutional()


def encode(tag, frames_u8, w, info=None):
    """models.py:147-152 + the network, float64.  frames_u8: (n, *obs shape) uint8 tensor; w: name -> float64 tensor.  info (a dict):
    receives 'kink', the smallest |ReLU input| of the batch."""
    kw = GEOMETRIES[tag]['kwargs']
    x = frames_u8
    if kw.get('channels_last', False):
        x = x.permute(0, 3, 1, 2)
    d = kw.get('downsample', 1)
    if d > 1:
        x = x[:, :, ::d, ::d]
    x = x.double() / 255.0
    z1 = F.conv2d(x, w['network.0.weight'], w['network.0.bias'], stride=4)
    a1 = F.relu(z1)
    z2 = F.conv2d(a1, w['network.2.weight'], w['network.2.bias'], stride=2)
    a2 = F.relu(z2)
    z3 = F.conv2d(a2, w['network.4.weight'], w['network.4.bias'], stride=1)
    a3 = F.relu(z3)
    z4 = F.linear(a3.flatten(1), w['network.7.weight'], w['network.7.bias'])
    h = F.relu(z4)
    if info is not None:      # distance of the nearest ReLU input to its kink (the gradient is discontinuous there)
        info['kink'] = min(float(z.detach().abs().min()) for z in (z1, z2, z3, z4))
    return a1, a2, a3, h


def heads(h, w, actions=None, noise=None):
    """decode_actions (models.py:154-157) + sample_logits (frameworks/cleanrl.py:25-47): with `noise` ~ Exp(1) the multinomial draw
    is argmax(log p - log noise).  Returns logits, value, action, logprob, entropy and the (best - second best) gap of the draw."""
    logits = F.linear(h, w['actor.weight'], w['actor.bias'])
    value = F.linear(h, w['value_fn.weight'], w['value_fn.bias']).flatten()
    logp = logits - logits.logsumexp(dim=-1, keepdim=True)
    gap = None
    if actions is None:
        score = logp - noise.double().log()
        top = score.topk(2, dim=-1).values
        gap = top[:, 0] - top[:, 1]
        actions = score.argmax(dim=-1)
    logprob = logp.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1)
    entropy = -(logp.exp() * logp).sum(-1)
    return logits, value, actions, logprob, entropy, gap


def ppo_loss(logprob, entropy, value, old_logprob, old_value, advantages, returns, clip_coef=0.1, vf_clip_coef=0.1, vf_coef=0.5,
             ent_coef=0.01, norm_adv=True, clip_vloss=True):
    """clean_pufferl.py:202-238 on one minibatch."""
    logratio = logprob - old_logprob
    ratio = logratio.exp()
    adv = advantages
    if norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)).mean()
    if clip_vloss:
        v_unclipped = (value - returns) ** 2
        v_clipped = old_value + torch.clamp(value - old_value, -vf_clip_coef, vf_clip_coef)
        v_loss = 0.5 * torch.max(v_unclipped, (v_clipped - returns) ** 2).mean()
    else:
        v_loss = 0.5 * ((value - returns) ** 2).mean()
    entropy_loss = entropy.mean()
    return pg_loss - ent_coef * entropy_loss + vf_coef * v_loss, pg_loss, v_loss, entropy_loss


def reference_forward_backward(tag, frames_u8, weights, hidden_grad=None, batch=None, **hparams):
    """Float64 forward (activations NCHW, hidden, logits, values) and gradients of every parameter.  The scalar that is
    'kink': the smallest |ReLU input| (a gradient comparison is meaningful only where fp32 rounding cannot flip a unit).  The scalar
    differentiated: sum(hidden * hidden_grad) when `hidden_grad` is given (layer tests), else the PPO loss on `batch` = dict(actions,
    logprobs, values, advantages, returns) (update tests).  weights: name -> numpy / tensor."""
    w = {k: torch.as_tensor(np.asarray(v)).double().clone().requires_grad_(True) for k, v in weights.items()}
    x = torch.as_tensor(np.asarray(frames_u8))
    info = {}
    a1, a2, a3, h = encode(tag, x, w, info)
    for t in (a1, a2, a3):
        t.retain_grad()
    out = dict(a1=a1, a2=a2, a3=a3, h=h, kink=info['kink'])
    if hidden_grad is not None:
        (h * torch.as_tensor(np.asarray(hidden_grad)).double()).sum().backward()
    elif batch is not None:
        b = {k: torch.as_tensor(np.asarray(v)) for k, v in batch.items()}
        logits, value, _, logprob, entropy, _ = heads(h, w, actions=b['actions'])
        loss, pg, vl, ent = ppo_loss(logprob, entropy, value, b['logprobs'].double(), b['values'].double(), b['advantages'].double(),
                                     b['returns'].double(), **hparams)
        loss.backward()
        out.update(logits=logits, value=value, logprob=logprob, entropy=entropy, loss=loss, pg_loss=pg, v_loss=vl, entropy_loss=ent)
    else:
        logits, value, _, _, _, _ = heads(h, w, actions=torch.zeros(h.shape[0], dtype=torch.long))
        out.update(logits=logits, value=value)
    out['grads'] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()}
    out['d_a1'], out['d_a2'] = a1.grad, a2.grad
    return out


# ------------------------------------------------------------------------------------------ brute-force geometry (CPU tests)
def brute_conv_out(size, kernel, stride):
    return len([o for o in range(size) if o * stride + kernel <= size])


def brute_geometry(obs_shape, channels_last, downsample):
    """Layer sizes, byte strides and frame size by enumeration of a frame's byte addresses."""
    idx = np.arange(int(np.prod(obs_shape))).reshape(obs_shape)
    if channels_last:
        idx = idx.transpose(2, 0, 1)
    idx = idx[:, ::downsample, ::downsample]
    c, ih, iw = idx.shape
    sc = int(idx[1, 0, 0] - idx[0, 0, 0]) if c > 1 else None
    sy = int(idx[0, 1, 0] - idx[0, 0, 0]) if ih > 1 else None
    sx = int(idx[0, 0, 1] - idx[0, 0, 0]) if iw > 1 else None
    sizes, h, w = [], ih, iw
    for k, s in ((8, 4), (4, 2), (3, 1)):
        h, w = brute_conv_out(h, k, s), brute_conv_out(w, k, s)
        sizes.append((h, w))
    return dict(channels=c, ih=ih, iw=iw, sc=sc, sy=sy, sx=sx, sizes=sizes, frame_bytes=int(idx.max()) + 1 if not downsample > 1 else int(np.prod(obs_shape)))


def brute_phase_pixels(ih, iw, stride, py, px):
    return sum(1 for y in range(ih) for x in range(iw) if y % stride == py and x % stride == px)


def uncovered(size, kernel, stride):
    """Input rows / columns no window of a valid-padding convolution covers."""
    n = brute_conv_out(size, kernel, stride)
    covered = {o * stride + k for o in range(n) for k in range(kernel)}
    return [i for i in range(size) if i not in covered]
