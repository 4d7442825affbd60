"""Cases and worker of tests/test_gpu_step_roundtrips.py.

A case is a policy shape x a batch size x a reward scale.  Everything is generated on the CPU from a fixed seed, so the test
process can put the oracle's gradient norm next to the results without touching the GPU, and each worker process (one per value of
PFA_FUSED_ADAM, which the library may read once per process) regenerates the same bytes.

    python tests/step_roundtrips_cases.py --out file.npz        (the environment is the caller's)

runs every case through pfa_ppo_adv_stats + two calls of pfa_ppo_mlp_train (two full updates: 2 epochs x 4 minibatches each) and
stores the parameters, both Adam moments and the six loss sums."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

H, NMB, HORIZON, EPOCHS, UPDATES = 128, 4, 16, 2, 2
MAX_GRAD_NORM = 0.5
HP = dict(clip_coef=.1, vf_clip_coef=.1, vf_coef=.5, ent_coef=.01, gamma=.99, gae_lambda=.95)

# (obs_dim, obs_stride, num_actions): one Discrete head each.  The reduce + Adam launch has ceil(NativeLayout::kCount / 64) workgroups,
# which depends on the row width (and the 7x7 trimming) only; wave 0 of each collects the others' norm words in ceil(workgroups / 64)
# polls per lane.  The shape table has NO shape with <= 64 workgroups (the narrowest rows, 16 floats, already give 67):
#   stride 16 -> 67 workgroups (65-128: 2 polls)      the 7x7 grid on stride 64 -> 133 (129-192: 3 polls)
#   stride 96 -> 227 (> 192: 4 polls)                 stride 128 -> 291 (> 192: 5 polls, the last one on 35 lanes)
SHAPES = {'stride16': (12, 16, 5), 'grid7x7': (49, 64, 8), 'stride96': (90, 96, 6), 'stride128': (100, 128, 6)}
REDUCE_GRID = {'stride16': 67, 'grid7x7': 133, 'stride96': 227, 'stride128': 291}
# envs x steps, 4 minibatches each: 256 rows = 16 tiles per minibatch (every wavefront pair gets at most one tile); 2048 rows = 128
# tiles; and 16 640 rows = 1040 tiles, more than the 1024 (512 on rows of 96 / 128 floats) pairs of a full gradient grid, so that
# pairs run a second, partly filled round of tiles (J > 1)
SIZES = {'64x16': (64, 16), '256x32': (256, 32), '1040x64': (1040, 64)}
SCALES = {'plain': 1.0, 'clipped': 50.0}    # reward scale; 'clipped': the oracle's gradient norm is far above max_grad_norm


def case_ids():
    return [f'{s}-{z}-{c}' for s in SHAPES for z in SIZES for c in SCALES]


def native_count(name):
    obs_dim, dp, _ = SHAPES[name]
    ktm, col = (3, True) if (dp == 64 and obs_dim == 49) else (dp // 16, False)
    return ktm * 8 * 4 * 64 + (H if col else 0) + 8 * 4 * 64 + H + 16 + 8


def make(case_id):
    """The case's experience (env-major rows, as the trainer sorts it) and initial parameters, numpy on the CPU."""
    from oracle import c_oracle
    shape, size, scale = case_id.split('-')
    obs_dim, dp, a = SHAPES[shape]
    n, t = SIZES[size]
    B = n * t
    rng = np.random.default_rng(10000 * dp + n)
    obs = rng.standard_normal((B, dp), dtype=np.float32)
    obs[:, obs_dim:] = 0
    actions = rng.integers(0, a, B).astype(np.int32)
    logprobs = (-np.log(a) + 0.05 * rng.standard_normal(B)).astype(np.float32)
    values = (0.5 * rng.standard_normal(B)).astype(np.float32)
    rewards = (SCALES[scale] * rng.standard_normal(B)).astype(np.float32)
    dones = (rng.random(B) < 0.02).astype(np.float32)
    adv = c_oracle.compute_gae(dones, values, rewards, HP['gamma'], HP['gae_lambda']).astype(np.float32)
    returns = (adv + values).astype(np.float32)
    w = dict(w1=0.05 * rng.standard_normal((H, dp), dtype=np.float32), b1=0.05 * rng.standard_normal(H, dtype=np.float32),
             w2=0.05 * rng.standard_normal((a, H), dtype=np.float32), b2=0.05 * rng.standard_normal(a, dtype=np.float32),
             wv=0.05 * rng.standard_normal((1, H), dtype=np.float32), bv=0.05 * rng.standard_normal(1, dtype=np.float32))
    w['w1'][:, obs_dim:] = 0
    flat = np.concatenate([w[k].reshape(-1) for k in ('w1', 'b1', 'w2', 'b2', 'wv', 'bv')])
    return dict(obs_dim=obs_dim, dp=dp, a=a, n=n, t=t, B=B, obs=obs, actions=actions, logprobs=logprobs, values=values, rewards=rewards,
                dones=dones, advantages=adv, returns=returns, weights=w, flat=flat)


def oracle_grad_norms(case):
    """Gradient norm of the PPO loss at the initial parameters, per minibatch, by the torch-fp32 oracle on the CPU (the loss of
    oracle/ppo_torch.Trainer.train; minibatch m = segments {m + k nmb} of HORIZON rows)."""
    import torch
    from oracle import ppo_torch
    w, d = case['weights'], case['obs_dim']
    pol = ppo_torch.Policy({'encoder.weight': w['w1'][:, :d], 'encoder.bias': w['b1'], 'decoder.weight': w['w2'], 'decoder.bias': w['b2'],
                            'value_head.weight': w['wv'], 'value_head.bias': w['bv']})
    seg = np.arange(case['B']).reshape(-1, NMB, HORIZON).transpose(1, 0, 2).reshape(NMB, -1)
    norms = []
    for mb in range(NMB):
        ix = seg[mb]
        logits, newvalue, _ = pol.forward(torch.from_numpy(case['obs'][ix][:, :d]))
        _, newlogprob, entropy = ppo_torch.sample_logits(logits, action=torch.from_numpy(case['actions'][ix]))
        ratio = (newlogprob - torch.from_numpy(case['logprobs'][ix])).exp()
        adv = torch.from_numpy(case['advantages'][ix])
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - HP['clip_coef'], 1 + HP['clip_coef'])).mean()
        ret, val, nv = torch.from_numpy(case['returns'][ix]), torch.from_numpy(case['values'][ix]), newvalue.view(-1)
        v_clipped = val + torch.clamp(nv - val, -HP['vf_clip_coef'], HP['vf_clip_coef'])
        v_loss = 0.5 * torch.max((nv - ret) ** 2, (v_clipped - ret) ** 2).mean()
        loss = pg - HP['ent_coef'] * entropy.mean() + HP['vf_coef'] * v_loss
        grads = torch.autograd.grad(loss, pol.params)
        norms.append(float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads))))
    return norms


def run_on_gpu(case):
    import torch
    from pufferlib_amd import _lib
    L = _lib.lib()
    dev = 'cuda'
    keep = [torch.from_numpy(case[k]).to(dev) for k in ('obs', 'actions', 'logprobs', 'values', 'rewards', 'dones', 'advantages', 'returns')]
    exp = _lib.Experience(*(x.data_ptr() for x in keep), case['t'])
    dims = _lib.MlpDims(case['obs_dim'], case['dp'], H, case['a'], 0)
    hp = _lib.PpoHparams(HP['clip_coef'], HP['vf_clip_coef'], HP['vf_coef'], HP['ent_coef'], 1, 1, NMB, HORIZON)
    B, P = case['B'], case['flat'].size
    params = torch.from_numpy(case['flat']).to(dev)
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    grads = torch.zeros(P + 16, device=dev)
    losses = torch.zeros(8, dtype=torch.float64, device=dev)
    ws = torch.zeros(L.pfa_ppo_workspace_bytes(C.byref(dims), B, C.byref(hp)), dtype=torch.uint8, device=dev)
    stats = torch.zeros(NMB, 2, dtype=torch.float64, device=dev)
    _lib.check(L.pfa_ppo_adv_stats(C.byref(exp), B, C.byref(hp), stats.data_ptr(), ws.data_ptr(), None), 'adv_stats')
    for u in range(UPDATES):
        _lib.check(L.pfa_ppo_mlp_train(C.byref(exp), B, params.data_ptr(), C.byref(dims), C.byref(hp), stats.data_ptr(), grads.data_ptr(),
                                       m.data_ptr(), v.data_ptr(), u * EPOCHS * NMB, 2.5e-3, .9, .999, 1e-5, MAX_GRAD_NORM, EPOCHS,
                                       losses.data_ptr(), ws.data_ptr(), 0, None), 'train')
    torch.cuda.synchronize()
    assert L.pfa_ppo_grid_status() == 0
    return dict(params=params.cpu().numpy(), exp_avg=m.cpu().numpy(), exp_avg_sq=v.cpu().numpy(), losses=losses.cpu().numpy()[:6])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    out = {}
    for cid in case_ids():
        for k, x in run_on_gpu(make(cid)).items():
            out[f'{cid}.{k}'] = x
    np.savez(a.out, **out)


if __name__ == '__main__':
    main()
