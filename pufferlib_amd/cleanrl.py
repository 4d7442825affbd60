"""frameworks.cleanrl.Policy (pufferlib/frameworks/cleanrl.py:50-66) over the HIP forward+sample kernel.

``policy(obs)`` (rollout mode, action=None) returns (actions, logprob, entropy, value) like the reference; the
multinomial draw is argmax(softmax(logits)/q) with q ~ Exp(1) from either an explicit ``noise`` tensor (parity with
torch.multinomial given its exponential draw) or the Philox stream keyed by ``seed`` (include/pufferlib_amd.h).
``policy(obs, action=...)`` (training mode, cleanrl.py:60-66,87-93) returns the log-probability of the GIVEN actions, the entropy and
the value through the GEMM path (pufferlib_amd.general.Evaluator) — on the `cnn` route through its own engine's head kernels
(cnn.Engine.policy_eval: the bits of the rollout for the action it drew).  By default these are plain tensors (the
gradients of clean_pufferl.train() are computed by its own kernels); ``Policy(policy, autograd=True)`` / ``RecurrentPolicy(policy,
autograd=True)`` attach an autograd graph to logprob, entropy and value of that call, so that a loss built from them in torch ops trains
the policy with ``loss.backward()``, ``clip_grad_norm_`` and any torch optimizer over ``policy.parameters()`` (general.Evaluator for
models.Default, alone or under LSTMWrapper; cnn.Engine.eval_backward on the `cnn` route, one chunk of frames per call).

Which kernels a module runs in is decided once, by route(policy_module, recurrent); everything else here and in the trainer reads it:

  route     module (wrapper)                                                                    parameters     autograd=True
  mlp       Default(128), rows of <= 128 floats, <= 15 logits (Policy)                          FlatParams     admitted
  lstm      LSTMWrapper(Default(128)) at (128, 128), rows of <= 160 floats (RecurrentPolicy)    FlatParams     admitted
  cnn       Convolutional, <= 15 actions (Policy)                                               ConvParams     admitted
  resnet    ProcgenResnet, <= 15 actions (Policy)                                               ResnetParams   refused
  general   every other Default / LSTMWrapper(Default) shape (hidden != 128, wider rows, more    GeneralParams  admitted
            logits, other LSTM sizes)
            Convolutional with 16 .. 1024 actions, LSTMWrapper(Convolutional)                   GeneralParams  refused
  (refused by route itself: LSTMWrapper(ProcgenResnet), ProcgenResnet with more than 15 actions)"""
import ctypes as C

import torch

from . import _lib
from .models import ConvParams, FlatParams, ResnetParams, find_cnn, find_lstm, find_resnet

KERNEL_STRIDES = (16, 32, 64, 96, 128)     # observation row strides (floats) every policy kernel is built for
RECURRENT_STRIDES = KERNEL_STRIDES + (160,)  # the recurrent path also takes MiniGrid-shaped 160-byte rows (SURVEY config C3)


def _narrowest(obs_dim, strides):
    return next((s for s in strides if obs_dim <= s), (obs_dim + 15) // 16 * 16)


def obs_stride_for(obs_dim, recurrent=False):
    """Row stride (floats) of a flat observation: the narrowest stride the fused kernels are built for, or — wider rows run in the
    GEMM path (general.py) — the next multiple of 16."""
    return _narrowest(obs_dim, RECURRENT_STRIDES if recurrent else KERNEL_STRIDES)


def _routed(policy_module, recurrent):
    """(route, whether the encoder reads uint8 frames).  A module's shape does not change: the answer is cached on it (forward() asks on
    every call)."""
    cache = policy_module.__dict__.setdefault('_pfa_route', {})
    if recurrent not in cache:
        cache[recurrent] = _route(policy_module, recurrent)
    return cache[recurrent]


def route(policy_module, recurrent):
    """Which kernels run the module behind Policy (recurrent=False) / RecurrentPolicy (True): 'mlp', 'lstm', 'cnn', 'resnet' — the
    fused kernels and the two conv engines — or 'general', the GEMM path, for every shape outside what those are instantiated for
    (the table in the module docstring)."""
    return _routed(policy_module, recurrent)[0]


def reads_frames(policy_module, recurrent):
    """True when the module's observations are uint8 frames (a conv encoder, on whichever route): rows are moved as bytes."""
    return _routed(policy_module, recurrent)[1]


def needs_general(policy_module, recurrent):
    """True when the policy's shape is outside what the fused kernels are instantiated for."""
    return route(policy_module, recurrent) == 'general'


def _route(policy_module, recurrent):
    from .models import HIDDEN, decoder_heads, find_mlp
    lstm = find_lstm(policy_module)
    cnn = find_cnn(policy_module)
    resnet = find_resnet(policy_module)
    if resnet is not None:    # models.ProcgenResnet has its own engine (resnet.py) and no GEMM-path form: what it cannot run is not built
        if lstm is not None:
            raise NotImplementedError('LSTMWrapper over models.ProcgenResnet (procgen\'s Recurrent) is not built: use the feed-forward Policy')
        if int(resnet.actor.weight.shape[0]) > 15:
            raise NotImplementedError(f'models.ProcgenResnet with {int(resnet.actor.weight.shape[0])} actions: the 16-lane head kernels take up to 15')
        return 'resnet', True
    if cnn is not None:       # the conv engine's 16-lane head kernels take 15 actions; wider sets sample in the row kernels of the GEMM path
        return ('general' if lstm is not None or int(cnn.actor.weight.shape[0]) > 15 else 'cnn'), True
    mlp = find_mlp(policy_module)
    H, D = mlp.encoder.weight.shape
    if (H != HIDDEN or sum(decoder_heads(mlp)) > 15 or D > (RECURRENT_STRIDES if recurrent else KERNEL_STRIDES)[-1]
            or (lstm is not None and (lstm.input_size, lstm.hidden_size) != (HIDDEN, HIDDEN))):
        return 'general', False
    return ('lstm' if recurrent else 'mlp'), False


def _weights_changed(module, _incompatible_keys=None):
    """The parameters of a Policy / RecurrentPolicy were overwritten in place (load_state_dict, whose post hook this is; the checkpoint
    loader; anybody's write between two policy(obs, action=...) calls), so every packed operand copy (GEMM-path Net, conv engine) is
    stale — the same version bump the engines' own optimizer steps make."""
    for obj in (getattr(getattr(module, 'gen_engine', None), 'net', None), getattr(getattr(module, '_evaluator', None), 'net', None),
                getattr(module, 'cnn_engine', None)):
        if obj is not None and hasattr(obj, 'version'):
            obj.version += 1


def _stage_rows(x2, D, allowed, required=None):
    """Observation rows [rows][D] as the kernels read them -> (src, stride): the caller's own rows where they already are float32 rows
    of a padded, 16-byte aligned kernel stride (e.g. the vecenv's live buffer) — of exactly `required` floats where that is given,
    else of any of `allowed` that holds D — otherwise a zero-padded copy (`required`, or the narrowest of `allowed`), made with
    .float() like models.Default (models.py:50)."""
    stride = x2.stride(0)
    if (x2.dtype == torch.float32 and x2.stride(1) == 1 and x2.data_ptr() % 16 == 0
            and (stride == required if required else stride >= D and stride in allowed)):
        return x2, stride
    stride = required or _narrowest(D, allowed)
    src = torch.zeros(x2.shape[0], stride, dtype=torch.float32, device=x2.device)
    src[:, :D] = x2.float()
    return src, stride


def _check_autograd(policy_module, autograd, recurrent):
    """autograd=True is built for MLP encoders and for the `cnn` route; said at construction, where no GPU is needed."""
    if autograd and reads_frames(policy_module, recurrent) and route(policy_module, recurrent) != 'cnn':
        raise NotImplementedError('autograd=True with a convolutional encoder (models.Convolutional, models.ProcgenResnet): autograd through '
                                  'policy(obs, action=...) is built for models.Default, alone or under LSTMWrapper, and for the feed-forward '
                                  'models.Convolutional with up to 15 actions; the other conv encoders\' backward is not wired to it — train '
                                  'them with clean_pufferl.train()')
    return bool(autograd)


class _ConvEvalGrad(torch.autograd.Function):
    """logprob, entropy, value of cnn.Engine.policy_eval as functions of the module parameters (the only tensor inputs, in
    named_parameters() order, so autograd itself accumulates into their .grad): the forward is the plain launch sequence on one chunk,
    the backward cnn.Engine.eval_backward — which runs the forward again where another call has overwritten the engine's activations
    since, and reads the parameters as they are when it runs.  Once differentiable."""

    @staticmethod
    def forward(ctx, eng, frames, rows, actions, *params):
        dev = frames.device
        logprob, entropy, value = (torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(3))
        eng._alloc(rows)
        eng.policy_eval(frames, rows, actions, logprob, entropy, value)
        ctx.eng, ctx.frames, ctx.rows, ctx.actions, ctx.generation = eng, frames, rows, actions, eng.generation
        ctx.set_materialize_grads(False)            # an output the loss does not use arrives as None: a null pointer to the kernel
        return logprob, entropy, value.unsqueeze(1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logprob, g_entropy, g_value):
        eng, rows = ctx.eng, ctx.rows
        g = [None if x is None else x.detach().to(device=ctx.frames.device, dtype=torch.float32).reshape(rows).contiguous()
             for x in (g_logprob, g_entropy, g_value)]
        gv = eng.cp.split(eng.eval_backward(ctx.frames, rows, ctx.actions, *g, generation=ctx.generation))
        return (None,) * 4 + tuple(gv[name] if need else None for name, need in zip(eng.cp.names, ctx.needs_input_grad[4:]))


class _Wrapper(torch.nn.Module):
    """What Policy and RecurrentPolicy share: the wrapped module, the Philox stream position, the flat parameter buffer of the module's
    route and the GEMM-path call."""
    recurrent = False
    autograd = False          # (the instances' own; this one answers for a module pickled before the option existed)

    def __init__(self, policy, seed=0, autograd=False):
        super().__init__()
        self.autograd = _check_autograd(policy, autograd, self.recurrent)
        self.policy = policy
        self.noise_seed = int(seed)
        self.noise_step = 0
        self._flat = None
        self.register_load_state_dict_post_hook(_weights_changed)

    @property
    def flat_params(self):
        return self._flat

    def __getstate__(self):
        """Pickles (torch.save of the whole module, clean_pufferl.py:517) carry the parameters only: the flat-buffer bookkeeping
        and the engines' buffers are rebuilt by adopt() on first use."""
        state = dict(self.__dict__)
        state['_flat'] = None
        for k in ('cnn_engine', 'gen_engine', '_evaluator'):
            state.pop(k, None)
        return state

    def adopt(self, obs_stride, device):
        """Move the parameters into one flat device buffer (idempotent for the same stride/device)."""
        kind, flat, device = route(self.policy, self.recurrent), self._flat, torch.device(device)
        if kind in ('cnn', 'resnet'):
            # a conv encoder with its own parameter layout and engine (cnn.py / resnet.py), both in the cnn_engine slot
            from . import cnn, resnet
            find, Params, Engine = (find_cnn, ConvParams, cnn.Engine) if kind == 'cnn' else (find_resnet, ResnetParams, resnet.Engine)
            recorded = find(self.policy).__dict__.get('_pfa_obs_shape')      # (a trainer may have recorded the env's frame shape since)
            if flat is None or flat.flat.device != device or (recorded is not None and flat.geometry.obs_shape != recorded):
                self._flat = Params(self.policy, device)
                self.cnn_engine = Engine(self._flat, chunk=256)           # grows on demand (Engine._alloc)
                if self.autograd:     # somebody's torch optimizer may step the nn.Parameters themselves: the packed conv operands
                    self.cnn_engine.watch = tuple(self._flat.net.parameters())    # follow their version counters
            return self._flat
        if kind == 'general':
            from . import general
            if (flat is None or flat.flat.device != device
                    or (flat.kind == 'mlp' and obs_stride and flat.obs_stride != obs_stride)):
                self._flat = general.GeneralParams(self.policy, device, obs_stride or None)
                self._evaluator = None
        elif flat is None or flat.obs_stride != obs_stride or flat.flat.device != device:
            self._flat = FlatParams(self.policy, obs_stride, device)
            self._evaluator = None
        return self._flat

    def _sampling_call(self, rows, device, num_actions, noise):
        """What a sampling kernel call of `rows` rows needs beside its input: the output tensors, the Philox key of this stream
        position and the explicit noise as the kernel reads it -> (actions, logprob, entropy, value, key, noise).  The stream moves on
        by one exactly when no noise is given."""
        key = _lib.NoiseKey(self.noise_seed, self.noise_step)
        if noise is not None:
            noise = noise.to(device=device, dtype=torch.float32).contiguous()
            assert noise.shape == (rows, num_actions)        # the kernel reads num_actions draws per row, whatever it is handed
        else:
            self.noise_step += 1
        actions = torch.empty(rows, dtype=torch.int64, device=device)
        logprob, entropy, value = (torch.empty(rows, dtype=torch.float32, device=device) for _ in range(3))
        return actions, logprob, entropy, value, key, noise

    def _scorer(self, device):
        """general.Evaluator over this policy's parameter buffer (built on first use)."""
        from . import general
        if self._flat is None:
            frames = reads_frames(self.policy, self.recurrent)
            D = 0 if frames else int(general.find_mlp(self.policy).encoder.weight.shape[1])
            self.adopt(obs_stride_for(D, self.recurrent) if D else 0, device)
        eng = getattr(self, 'gen_engine', None)
        if getattr(self, '_evaluator', None) is None:
            if route(self.policy, self.recurrent) == 'general':
                net = eng.net if eng is not None else general._net_for_general(self._flat)
            else:
                net = general.net_for_flat(self._flat)
            self._evaluator = general.Evaluator(net)
        if eng is None or self._evaluator.net is not eng.net:
            # the fused 128-wide update kernels change the kernel-layout buffer behind this evaluator's back: re-pack its operand copies on
            # every call (so does a policy used on its own, whose tensors anybody may write).  A trainer's GEMM-path Net is told when its
            # weights change: the optimizer step (Engine.clip_adam), the checkpoint loader and load_state_dict (post hook) bump its version.
            _weights_changed(self)
        if self.autograd:    # somebody's torch optimizer may step the nn.Parameters themselves: their version counters join the pack key
            self._evaluator.net.watch = tuple(general.module_parameters(self._flat).values())
        return self._evaluator

    def _evaluate(self, x, action, noise, **kw):
        """The GEMM path (general.Evaluator): the given actions scored (cleanrl.py:60-66,87-93) or, for a policy shape outside the
        fused kernels, actions sampled -> (actions, logprob, entropy, value, state).  With autograd opted in, actions given and grad
        mode on, logprob, entropy and value come with a graph over the module's nn.Parameters."""
        ev = self._scorer(x.device)
        key = None
        if action is None and noise is None:
            key = _lib.NoiseKey(self.noise_seed, self.noise_step)
            self.noise_step += 1
        params = None
        if self.autograd and action is not None and torch.is_grad_enabled():
            from . import general
            params = general.module_parameters(self._flat)
        a, logprob, entropy, value, state = ev.forward(x, action=action, noise=noise, key=key, params=params, **kw)
        return (action if action is not None else self._flat.unpack_actions(a)), logprob, entropy, value, state


class Policy(_Wrapper):
    """frameworks.cleanrl.Policy.  autograd=False (default): every call returns plain tensors.  autograd=True: ``policy(obs, action=a)``
    with grad mode on returns the same values, bit for bit, with logprob, entropy and value carrying a grad_fn whose backward
    accumulates into .grad of every module parameter (torch semantics: adds to an existing .grad, parameter-shaped, on the device);
    under torch.no_grad() or with action=None (sampling) the plain path runs.  Double backward is not built."""

    def get_value(self, x, state=None):
        return self.forward(x)[3]

    def get_action_and_value(self, x, action=None, noise=None):
        return self.forward(x, action=action, noise=noise)

    def forward(self, x, action=None, noise=None):
        _lib.require_gpu()
        if not x.is_cuda:
            x = x.cuda()
        rows = x.shape[0]
        x2 = x.reshape(rows, -1)
        kind = route(self.policy, False)
        if kind == 'resnet' and action is not None:
            raise NotImplementedError('policy(frames, action=...) for models.ProcgenResnet: use train()')
        if kind in ('cnn', 'resnet'):
            return self._forward_frames(x2, rows, noise, action)   # given actions: the conv engine's own heads (csrc/cnn_heads.hip)
        if action is None and kind == 'mlp':
            return self._forward_mlp(x2, rows, noise)
        if action is None and kind == 'general':
            out = self._forward_tile(x2, rows, noise)              # Default(64 / 256 / 512): the tile code the fused rollout runs
            if out is not None:
                return out
        # given actions (cleanrl.py:60-66 with action=...): log-prob / entropy / value of THOSE actions; or a policy shape that runs in
        # the GEMM path altogether
        return self._evaluate(x2, action, noise)[:4]

    def _forward_mlp(self, x2, rows, noise):
        """policy(obs) in rollout mode on the `mlp` route: one launch of the fused forward + sample kernel."""
        src, stride = _stage_rows(x2, x2.shape[1], KERNEL_STRIDES)
        fp = self.adopt(stride, x2.device)
        actions, logprob, entropy, value, key, noise = self._sampling_call(rows, x2.device, fp.num_actions, noise)
        _lib.check(_lib.lib().pfa_mlp_forward_sample(_lib.ptr(src), rows, _lib.ptr(fp.flat), C.byref(fp.dims), _lib.ptr(noise),
                                                     C.byref(key), 0, _lib.ptr(actions), _lib.ptr(logprob), _lib.ptr(entropy),
                                                     _lib.ptr(value), _lib.stream_handle()), 'mlp_forward_sample')
        return fp.unpack_actions(actions), logprob, entropy, value.unsqueeze(1)

    def _forward_tile(self, x2, rows, noise):
        """policy(obs) in rollout mode for a Default of one of the tile kernels' widths (general.tile_view): one launch of
        pfa_mlp_view_forward_sample — the same code, bit for bit, as the persistent fused rollout.  None when the shape is not one of them."""
        from . import general
        D = x2.shape[1]
        fp = self._flat if self._flat is not None else self.adopt(obs_stride_for(D), x2.device)
        view = general.tile_view(fp)
        if view is None:
            return None
        if D != fp.obs_dim:
            raise ValueError(f'observation rows of {D} values, the policy reads {fp.obs_dim}')
        src, _ = _stage_rows(x2, D, KERNEL_STRIDES, required=fp.obs_stride)
        actions, logprob, entropy, value, key, noise = self._sampling_call(rows, x2.device, fp.num_actions, noise)
        _lib.check(_lib.lib().pfa_mlp_view_forward_sample(_lib.ptr(src), rows, C.byref(view), _lib.ptr(noise), C.byref(key), 0, _lib.ptr(actions),
                                                          _lib.ptr(logprob), _lib.ptr(entropy), _lib.ptr(value), _lib.stream_handle()),
                   'mlp_view_forward_sample')
        return actions, logprob, entropy, value.unsqueeze(1)

    def _forward_frames(self, x2, rows, noise, action=None):
        """policy(frames) on the `cnn` / `resnet` routes: uint8 (rows, frame bytes in the env's order) -> (actions, logprob, entropy,
        value); with `action` (`cnn` only) the given actions are scored instead of sampled."""
        cp = self.adopt(0, x2.device)
        if x2.shape[1] != cp.obs_dim:
            raise ValueError(f'expected frames of {cp.obs_dim} bytes, got rows of {x2.shape[1]}')
        frames = x2.to(torch.uint8).contiguous()       # the reference divides whatever it is given by 255 (models.py:152); frames are bytes
        eng = self.cnn_engine
        if action is not None:
            return self._score_frames(cp, frames, rows, action, frames.data_ptr() == x2.data_ptr())
        eng._alloc(min(rows, eng.CHUNK_CAP))
        actions, logprob, entropy, value, key, noise = self._sampling_call(rows, x2.device, cp.num_actions, noise)
        eng.policy_step(frames, rows, noise, key, 0, actions, logprob, entropy, value)
        return actions, logprob, entropy, value.unsqueeze(1)

    def _score_frames(self, cp, frames, rows, action, aliased):
        """policy(frames, action=...) for models.Convolutional in the conv engine: (action, logprob, entropy, value) of the GIVEN actions."""
        eng, dev, A = self.cnn_engine, frames.device, cp.num_actions
        a = action.to(dev).reshape(-1).to(torch.int64).contiguous()
        if a.numel() != rows:
            raise ValueError(f'{a.numel()} actions for {rows} frames')
        # the kernel compares the action with its lane index: one outside the head would score as log-probability 0 (one host round
        # trip, as on the GEMM path: not the rollout)
        if rows and bool(((a < 0) | (a >= A)).any()):
            raise IndexError(f'action out of range for Discrete({A})')
        if self.autograd and torch.is_grad_enabled() and rows:
            eng.check_one_chunk(rows)
            if aliased:                                  # the backward reads the frames again: keep them from the caller's later writes
                frames = frames.clone()
            logprob, entropy, value = _ConvEvalGrad.apply(eng, frames, rows, a, *(p for _, p in cp.net.named_parameters()))
            return action, logprob, entropy, value
        eng._alloc(min(rows, eng.CHUNK_CAP))
        logprob, entropy, value = (torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(3))
        eng.policy_eval(frames, rows, a, logprob, entropy, value)
        return action, logprob, entropy, value.unsqueeze(1)


class RecurrentPolicy(_Wrapper):
    """frameworks.cleanrl.RecurrentPolicy (pufferlib/frameworks/cleanrl.py:69-93) over the HIP LSTM path.

    ``policy(obs, state)`` (rollout mode) returns (actions, logprob, entropy, value, (h, c)) with state tensors of shape
    (1, rows, 128) like nn.LSTM.  The training-mode forward of train() lives in pufferlib_amd.clean_pufferl.train.

    autograd=True: as for Policy — ``policy(obs, state, action=a)`` with grad mode on returns (action, logprob, entropy, value, state)
    with a grad_fn on logprob, entropy and value.  No gradient flows into the incoming ``state`` or out of the returned one (plain
    tensors): the reference's trainer detaches the state between minibatches the same way (clean_pufferl.py:188-191), so back-propagation
    through time covers the TT steps of one call."""
    recurrent = True

    @property
    def lstm(self):
        if hasattr(self.policy, 'recurrent'):
            return self.policy.recurrent
        elif hasattr(self.policy, 'lstm'):
            return self.policy.lstm
        raise ValueError('Policy must have a subnetwork named lstm or recurrent')

    def get_action_and_value(self, x, state=None, action=None, noise=None):
        return self.forward(x, state=state, action=action, noise=noise)

    def forward(self, x, state=None, action=None, noise=None):
        from . import lstm as plstm
        _lib.require_gpu()
        if not x.is_cuda:
            x = x.cuda()
        if action is not None or route(self.policy, True) == 'general':
            # cleanrl.py:87-93: (B, obs...) or (B, TT, obs...) through encoder -> LSTM over TT steps -> heads, with the given actions
            # scored (or, for a policy shape outside the fused kernels, sampled) — the GEMM path
            obs_shape = getattr(self.policy, 'obs_shape', None)
            return self._evaluate(x, action, noise, state=state, obs_rank=len(obs_shape) if obs_shape is not None else None)
        rows = x.shape[0]
        x2 = x.reshape(rows, -1)
        src, stride = _stage_rows(x2, x2.shape[1], RECURRENT_STRIDES)
        if src is x2:
            src = torch.as_strided(x2, (rows, stride), (stride, 1))
        fp = self.adopt(stride, x.device)
        if state is None:
            h = torch.zeros(rows, 128, device=x.device)
            c = torch.zeros(rows, 128, device=x.device)
        else:
            h, c = state[0][0].contiguous().clone(), state[1][0].contiguous().clone()
        *out, key, noise = self._sampling_call(rows, x.device, fp.num_actions, noise)
        return plstm.policy_step(fp, src, h, c, noise, key, 0, out=out) + ((h.unsqueeze(0), c.unsqueeze(0)),)
