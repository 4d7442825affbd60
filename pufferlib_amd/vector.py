"""Vectorised-env boundary: ``make`` and the device-resident Squared backend.

Mirrors pufferlib/vector.py of the reference:
  make(...)                      vector.py:577-637  (same validation, same APIUsageError messages)
  reset / step helpers           vector.py:44-53
  recv_precheck / send_precheck  vector.py:25-42    (RESET -> RECV -> SEND state machine)
  Squared (backend class)        replaces Serial (vector.py:70-166) for ocean ``make_squared`` envs: the N envs
                                 live in HBM and are stepped by HIP kernels (csrc/squared.hip); ``recv`` returns
                                 *device tensors* that alias the backend-owned live buffers, exactly like Serial
                                 returns aliases of its numpy buffers (vector.py:158-162).

Drop-in use with the reference's factory:  pufferlib.vector.make(make_squared, backend=pufferlib_amd.vector.Squared,
num_envs=N, env_kwargs=dict(distance_to_target=3, num_targets=1)).
"""
import ctypes as C

import numpy as np

from . import _lib, spaces
from .exceptions import APIUsageError
from .namespace import Namespace, namespace

# Deliberate interface mirror of pufferlib/vector.py:17-53 (flag constants, recv/send prechecks, reset/step helpers): callers of a
# drop-in backend compare against these constants and match on these messages.  Interface, not hot path.
RESET = 0
STEP = 1
SEND = 2
RECV = 3
CLOSE = 4
MAIN = 5
INFO = 6


def recv_precheck(vecenv):
    if vecenv.flag != RECV:
        raise APIUsageError('Call reset before stepping')
    vecenv.flag = SEND


def send_precheck(vecenv, actions):
    if vecenv.flag != SEND:
        raise APIUsageError('Call (async) reset + recv before sending')
    vecenv.flag = RECV


def reset(vecenv, seed=42):
    vecenv.async_reset(seed)
    obs, rewards, terminals, truncations, infos, env_ids, masks = vecenv.recv()
    return obs, infos


def step(vecenv, actions):
    vecenv.send(actions)
    obs, rewards, terminals, truncations, infos, env_ids, masks = vecenv.recv()
    return obs, rewards, terminals, truncations, infos


def make_seeds(seed, num_envs):
    if isinstance(seed, int):
        return [seed + i for i in range(num_envs)]
    err = f'seed {seed} must be an integer or a list of integers'
    if isinstance(seed, (list, tuple)):
        if len(seed) != num_envs:
            raise APIUsageError(err)
        return seed
    raise APIUsageError(err)


def make_squared(distance_to_target=3, num_targets=1, **kwargs):
    """Env creator token with the signature of ocean.environment.make_squared (ocean/environment.py:28-31).
    The Squared backend never calls it: it only reads its keyword defaults / env_kwargs."""
    return SquaredSpec(distance_to_target, num_targets)


def env_creator(name='squared'):
    """pufferlib.environments.ocean.env_creator (ocean/environment.py:6-26), squared only; plus pixel_squared, this package's frame
    rendering of it, tabular, the creator of a user-given TabularMDP (the reference has no such names), cartpole, the device
    restatement of environments.classic_control's env (make_cartpole's max_steps=0 is that creator's env: no time limit), and
    acrobot, gymnasium's Acrobot-v1 (the reference binds no such env)."""
    if name == 'squared':
        return make_squared
    if name == 'pixel_squared':
        return make_pixel_squared
    if name == 'tabular':
        return make_tabular
    if name == 'cartpole':
        return make_cartpole
    if name == 'acrobot':
        return make_acrobot
    raise ValueError('Invalid environment name')


def episode_means(st):
    """The means clean_pufferl.evaluate reports (clean_pufferl.py:127-137) from the (all-reduced) ``episode_stats`` sums
    (count, sum episode_return, sum episode_length, sum score)."""
    if st[0] <= 0:
        return {}
    return dict(episode_return=st[1] / st[0], episode_length=st[2] / st[0], score=st[3] / st[0])


class SquaredSpec:
    """What ``driver_env`` exposes to policies (models.py:26-37) and to clean_pufferl (:40-43)."""

    def __init__(self, distance_to_target=3, num_targets=1):
        self.distance_to_target = int(distance_to_target)
        self.num_targets = 4 * self.distance_to_target if num_targets == -1 else int(num_targets)
        g = 2 * self.distance_to_target + 1
        self.grid_size = g
        self.single_observation_space = spaces.Box(low=-1, high=1, shape=(g, g), dtype=np.float32)
        self.single_action_space = spaces.Discrete(8)
        self.observation_space = self.single_observation_space
        self.action_space = self.single_action_space
        self.num_agents = 1
        self.render_mode = 'ansi'
        self.emulated = namespace(observation_dtype=np.dtype(np.float32),
                                  emulated_observation_dtype=np.dtype((np.float32, (g, g))))
        self.done = True
        self._live_obs = None        # the vecenv's live observation buffer (set by the backend): render() draws env 0

    def render(self):
        """ocean.Squared.render (ocean.py:514-527) of env 0: targets blue, the agent red, empty cells grey."""
        if self._live_obs is None:
            return ''
        g = self.grid_size
        grid = self._live_obs[0, :g * g].detach().cpu().numpy().reshape(g, g)
        chars = []
        for row in grid:
            for val in row:
                color = 94 if val == 1 else (91 if val == -1 else 90)
                chars.append(f'\033[{color}m██\033[0m')
            chars.append('\n')
        return ''.join(chars)

    def close(self):
        pass


def _squared_kwargs(creator, args, kwargs):
    """Resolve (distance_to_target, num_targets) the way make_squared's signature would."""
    import inspect
    name = getattr(creator, '__name__', '')
    if 'squared' not in name.lower():
        raise APIUsageError(
            f'pufferlib_amd.vector.Squared only hosts ocean make_squared envs on device (got creator {name!r})')
    d, nt = 3, 1
    try:
        sig = inspect.signature(creator)
        if 'distance_to_target' in sig.parameters and sig.parameters['distance_to_target'].default is not inspect._empty:
            d = sig.parameters['distance_to_target'].default
        if 'num_targets' in sig.parameters and sig.parameters['num_targets'].default is not inspect._empty:
            nt = sig.parameters['num_targets'].default
    except (TypeError, ValueError):
        pass
    args = list(args)
    if len(args) > 0:
        d = args[0]
    if len(args) > 1:
        nt = args[1]
    d = kwargs.get('distance_to_target', d)
    nt = kwargs.get('num_targets', nt)
    return int(d), int(nt)


class _SimpleSpec:
    """What ``driver_env`` exposes to policies (models.py:26-37) and clean_pufferl for a one-value-observation ocean env."""

    def __init__(self, low, high, num_actions):
        self.single_observation_space = spaces.Box(low=low, high=high, shape=(1,), dtype=np.float32)
        self.single_action_space = spaces.Discrete(num_actions)
        self.observation_space = self.single_observation_space
        self.action_space = self.single_action_space
        self.num_agents = 1
        self.render_mode = 'ansi'
        self.emulated = namespace(observation_dtype=np.dtype(np.float32),
                                  emulated_observation_dtype=np.dtype((np.float32, (1,))))
        self.done = True

    def render(self):
        return ''

    def close(self):
        pass


def _creator_kwargs(creator, args, kwargs, names, defaults, family):
    """Resolve keyword values the way the reference creator's signature would (defaults < positional < keyword)."""
    import inspect
    name = getattr(creator, '__name__', '')
    if family not in name.lower():
        raise APIUsageError(f'this backend only hosts ocean make_{family} envs on device (got creator {name!r})')
    vals = dict(zip(names, defaults))
    try:
        sig = inspect.signature(creator)
        for n in names:
            if n in sig.parameters and sig.parameters[n].default is not inspect._empty:
                vals[n] = sig.parameters[n].default
    except (TypeError, ValueError):
        pass
    for i, n in enumerate(names):
        if len(args) > i:
            vals[n] = args[i]
        vals[n] = kwargs.get(n, vals[n])
    return tuple(vals[n] for n in names)


class _DeviceVecEnv:
    """Backend protocol (pufferlib/vector.py) over a device-resident env family with one observation value per env: live
    buffers as torch device tensors aliased by recv() (like Serial's numpy buffers, vector.py:158-162), RESET->RECV->SEND
    state machine, ``info_mode`` 'sync' (exact per-episode info dicts, one small D2H on the sends that finish episodes) or
    'lazy' (recv() returns [], statistics through ``episode_stats``).  Subclasses provide ``ABI``, the kernels
    ``_k_reset(seed)`` and ``_k_send(actions)``, and ``_finishing_send(sends)``."""
    reset = reset
    step = step
    obs_stride = 16
    ROLLOUT_LSTM = None     # name of the family's fused recurrent rollout entry point (lstm.Engine.rollout), None: it has none
    # fused_rollout_mlp(fp, experience, noise, key, stream): clean_pufferl.evaluate's T-step loop for the fused-kernel MLP policy as one
    # persistent kernel; None: the family has none (policy step + store + send per step)
    fused_rollout_mlp = None
    # whether fused_rollout_mlp also takes view=<pfa_mlp_view of a Default(64 / 128 / 256 / 512)>.  The view rollout reads the state layout
    # of the class that declares it: clean_pufferl.rollout_form looks in that class's own __dict__, never in a base class's
    ROLLOUT_MLP_VIEW = False
    PREFETCH = False        # whether the trainer draws the next rollout's reset tape (and action noise) on its side stream under a fused rollout
    FAMILY = ''
    ABI = ''                # prefix of the family's entry points: ABI + '_episode_stats', ABI + '_last_infos'
    NAMES = ()
    DEFAULTS = ()
    SEEDED = False          # whether the env family reads the seeds async_reset is given
    AGENTS_PER_ENV = 1      # agent rows per env, env-major (PettingZoo emulation order, emulation.py:325-345)
    OBS_U8 = False          # live observation buffer of bytes (frame envs) instead of floats
    CONFIG_NAME = ''        # how the "share one ... configuration" error names the family's settings

    @property
    def num_envs(self):
        return self.agents_per_batch

    def __init__(self, env_creators, env_args, env_kwargs, num_envs, info_mode='sync', env_offset=0, device=None, **kwargs):
        import torch
        for k in kwargs:
            if k not in ('num_workers', 'batch_size', 'zero_copy', 'backend'):
                raise APIUsageError(f'Invalid argument: {k}')
        if len(env_creators) != num_envs:
            raise APIUsageError('env_creators must be a list of length num_envs')
        specs = {self._creator_spec(c, a, k) for c, a, k in zip(env_creators, env_args, env_kwargs)}
        if len(specs) != 1:
            raise APIUsageError(f'obs/atn space mismatch: all envs must share one {self.CONFIG_NAME}configuration, got {specs}')
        _lib.require_gpu()
        self.L = _lib.lib()
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.driver_env = self._spec(*specs.pop())
        self.emulated = self.driver_env.emulated
        self.env_count = num_envs
        self.agents_per_env = [self.AGENTS_PER_ENV] * num_envs
        num_envs = num_envs * self.AGENTS_PER_ENV                      # agent rows from here on
        self.agents_per_batch = self.num_agents = num_envs
        self.single_observation_space = self.driver_env.single_observation_space
        self.single_action_space = self.driver_env.single_action_space
        if hasattr(self.single_action_space, 'n'):
            self.action_space = spaces.MultiDiscrete([self.single_action_space.n] * num_envs)
        else:                                                              # MultiDiscrete per agent: joint_space tiles it (vector.py:55-68)
            self.action_space = spaces.MultiDiscrete(np.tile(np.asarray(self.single_action_space.nvec)[None], (num_envs, 1)))
        self.observation_space = spaces.Box(low=self.single_observation_space.low.min(), high=self.single_observation_space.high.max(),
                                            shape=(num_envs,) + tuple(self.single_observation_space.shape), dtype=self.single_observation_space.dtype)
        self.agent_ids = np.arange(num_envs)
        self.initialized = False
        self.flag = RESET
        self.info_mode = info_mode
        self.env_offset = int(env_offset)
        self.obs_dim = 1
        dev = self.device
        self.obs_buf = torch.zeros(num_envs, self.obs_stride, dtype=torch.uint8 if self.OBS_U8 else torch.float32, device=dev)
        self.observations = self.obs_buf[:, :1]
        self.rewards = torch.zeros(num_envs, dtype=torch.float32, device=dev)
        self.terminals_u8 = torch.zeros(num_envs, dtype=torch.uint8, device=dev)
        self.truncations_u8 = torch.zeros(num_envs, dtype=torch.uint8, device=dev)
        self.masks_u8 = torch.ones(num_envs, dtype=torch.uint8, device=dev)
        self.terminals = self.terminals_u8.view(torch.bool)
        self.truncations = self.truncations_u8.view(torch.bool)
        self.masks = self.masks_u8.view(torch.bool)
        self._actions = torch.zeros(num_envs, dtype=torch.int64, device=dev)
        self._fin = torch.zeros(num_envs, dtype=torch.uint8, device=dev)
        self._fin_ret = torch.zeros(num_envs, dtype=torch.float64, device=dev)
        self._fin_len = torch.zeros(num_envs, dtype=torch.int32, device=dev)
        self._fin_score = torch.zeros(num_envs, dtype=torch.float64, device=dev)
        self._stats = torch.zeros(5, dtype=torch.float64, device=dev)   # 4 sums + tape underrun flag (0 for envs without a tape)
        self.infos = []
        self.sends = 0
        self._alloc_state()

    def _creator_spec(self, creator, args, kwargs):
        return _creator_kwargs(creator, args, kwargs, self.NAMES, self.DEFAULTS, self.FAMILY)

    def _live(self):
        return (_lib.ptr(self.obs_buf), _lib.ptr(self.rewards), _lib.ptr(self.terminals_u8), _lib.ptr(self.truncations_u8),
                _lib.ptr(self.masks_u8))

    def _fin_ptrs(self):
        return _lib.ptr(self._fin), _lib.ptr(self._fin_ret), _lib.ptr(self._fin_len), _lib.ptr(self._fin_score)

    def _state_args(self):
        """How the family's entry points address the device state: (state, config) or, without a config struct, (state, env count)."""
        cfg = getattr(self, 'cfg', None)
        return _lib.ptr(self.state), (self.env_count if cfg is None else C.byref(cfg))

    def _k_stats(self, reset, out):
        _lib.check(getattr(self.L, self.ABI + '_episode_stats')(*self._state_args(), _lib.ptr(out), reset, _lib.stream_handle()),
                   'episode_stats')

    def _k_infos(self):
        _lib.check(getattr(self.L, self.ABI + '_last_infos')(*self._state_args(), *self._fin_ptrs(), _lib.stream_handle()), 'last_infos')

    def async_reset(self, seed=42):
        self.flag = RECV
        seeds = make_seeds(seed, self.env_count)
        if self.SEEDED and any(s != seeds[0] + i for i, s in enumerate(seeds)):
            raise APIUsageError(f'pufferlib_amd.vector.{type(self).__name__} needs consecutive seeds (seed + env index)')
        self._k_reset(int(seeds[0]))
        self.sends = 0
        self.infos = []

    def device_send(self, actions):
        """send() for a device int64 tensor of actions, no protocol bookkeeping and no host sync (rollout loops)."""
        self._k_send(actions)
        self.sends += 1

    def send(self, actions):
        import torch
        send_precheck(self, actions)
        if not torch.is_tensor(actions):
            a = np.asarray(actions)
            if not self.initialized and not self.action_space.contains(a):
                raise APIUsageError('Actions do not match action space')
            actions = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64))
        elif not self.initialized:
            if actions.shape != (self.num_agents,) or actions.dtype not in (torch.int64, torch.int32):
                raise APIUsageError('Actions do not match action space')
        self.initialized = True
        self._actions.copy_(actions.reshape(-1), non_blocking=True)
        self._before_send()
        self.device_send(self._actions)
        self.infos = self._collect_infos() if self.info_mode == 'sync' else []

    def _before_send(self):
        """What send() does for the caller that device_send() leaves to it."""

    def recv(self):
        recv_precheck(self)
        return (self.observations, self.rewards, self.terminals, self.truncations, self.infos, self.agent_ids, self.masks)

    def close(self):
        self.flag = CLOSE

    def _collect_infos(self):
        if not self._finishing_send(self.sends):     # every env of these families finishes on the same sends
            return []
        self._k_infos()
        fin = self._fin.cpu().numpy().astype(bool)
        if not fin.any():
            return []
        ret, ln, sc = self._fin_ret.cpu().numpy(), self._fin_len.cpu().numpy(), self._fin_score.cpu().numpy()
        return [dict(episode_return=float(ret[i]), episode_length=int(ln[i]), score=float(sc[i])) for i in np.nonzero(fin)[0]]

    def episode_stats(self, reset=True):
        """(count, sum episode_return, sum episode_length, sum score) of the episodes finished since the last reset of the
        accumulators, as a device f64 tensor — what clean_pufferl.evaluate averages (clean_pufferl.py:127-137)."""
        self._k_stats(1 if reset else 0, self._stats)
        return self._stats[:4]      # [4] = tape underrun flag: read by the trainer from the same buffer (stats_with_flag)

    stats_from_sums = staticmethod(episode_means)

    def stats_with_flag(self, reset=True, out=None):
        """The four sums + the tape underrun flag; `out`: a 5-element f64 buffer the kernel writes instead of the vecenv's own
        (the trainer's pinned readback buffer: no device-to-host copy launch behind the kernel)."""
        out = self._stats if out is None else out
        self._k_stats(1 if reset else 0, out)
        return out


class _ResetTape:
    """Mixin of the device families whose resets consume random numbers that do not depend on actions: they are drawn ahead of
    the sends, one round per reset of all envs, into a ring of ``tape_rounds`` rounds in the device state.  This is the host
    mirror of the ring (the stream position itself lives on device).  The family provides ``_k_fill(rounds)``, ``episode_len``
    and ``tape_rounds``.  Only these families have ``ensure_tape``: callers test for it."""
    ROUNDS_AT_RESET = 0     # rounds async_reset itself draws and consumes
    RING_SPARE = 0          # rounds of the ring one ensure_tape() call must leave alone
    FILL_HALVES = False     # fill at most half the ring per launch

    def _tape_reset(self):
        """After the family's async_reset kernel: nothing sent, nothing drawn ahead."""
        self.sends = 0
        self.rounds_filled = self.ROUNDS_AT_RESET    # rounds drawn into the tape (mirrors the device counter)
        self.tape_event = None

    def _wait_tape(self):
        """Order the current stream behind a tape fill enqueued on a side stream (``tape_event``, recorded by whoever filled
        there: the trainer's prefetch): `rounds_filled` (host mirror) already counts those rounds, so every consumer of the
        tape — send(), a fused rollout, async_reset() — must wait for the fill itself."""
        if self.tape_event is not None:
            import torch
            torch.cuda.current_stream().wait_event(self.tape_event)

    def _rounds_needed(self, upto_send):
        """Rounds consumed by async_reset and sends 1..upto_send (every env resets on sends k*episode_len)."""
        return self.ROUNDS_AT_RESET + upto_send // self.episode_len

    @property
    def max_sends_per_tape(self):
        """Sends whose reset rounds one ensure_tape() call may draw ahead (half the ring: the other half may still be in use)."""
        return max(1, (self.tape_rounds // 2) * self.episode_len)

    def ensure_tape(self, extra_sends):
        self._wait_tape()
        need = self._rounds_needed(self.sends + extra_sends)
        asked = need - self._rounds_needed(self.sends)
        if asked > self.tape_rounds - self.RING_SPARE:
            raise APIUsageError(f'{extra_sends} sends need {asked} reset rounds; tape holds {self.tape_rounds}')
        while need > self.rounds_filled:
            n = need - self.rounds_filled
            if self.FILL_HALVES:
                n = min(n, self.tape_rounds // 2)
            self._k_fill(n)
            self.rounds_filled += n


class Squared(_ResetTape, _DeviceVecEnv):
    """Device-resident vecenv of N ocean Squared envs (csrc/squared.hip).  State, live buffers and the reset-target tape are
    torch device tensors (torch is the allocator); every method only enqueues HIP kernels on torch's current stream.  It has a
    fused rollout kernel for either policy; the trainer draws the next rollout's tape rounds on a side stream (``tape_event``)."""
    SEEDED = True
    CONFIG_NAME = 'Squared '
    ABI = 'pfa_squared'
    ROLLOUT_LSTM = 'pfa_rollout_lstm_squared'
    ROLLOUT_MLP_VIEW = True

    def __init__(self, env_creators, env_args, env_kwargs, num_envs, obs_stride=None, **kwargs):
        self._obs_stride_arg = obs_stride
        super().__init__(env_creators, env_args, env_kwargs, num_envs, **kwargs)

    PREFETCH = True

    def _creator_spec(self, creator, args, kwargs):
        return _squared_kwargs(creator, args, kwargs)

    def _spec(self, d, nt):
        spec = SquaredSpec(d, nt)
        self.obs_stride = int(self._obs_stride_arg) if self._obs_stride_arg is not None else max(16, _lib.round_up(spec.grid_size ** 2, 16))
        return spec

    def _alloc_state(self):
        import torch
        sp = self.driver_env
        g = sp.grid_size
        self.obs_dim = g * g
        self.observations = self.obs_buf[:, :self.obs_dim].unflatten(1, (g, g))   # view, shape (N, g, g)
        sp._live_obs = self.obs_buf
        self.episode_len = sp.num_targets * sp.distance_to_target + 1   # max_ticks steps + the auto-reset row
        self.tape_rounds = 192       # ring capacity: two rollouts of 4 x 96 sends.. (one being consumed + one prefetched)
        self.cfg = _lib.SquaredConfig(self.num_agents, sp.distance_to_target, sp.num_targets, self.obs_stride, self.tape_rounds)
        nbytes = self.L.pfa_squared_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._tape_reset()

    def _finishing_send(self, sends):
        return sends % self.episode_len == self.episode_len - 1

    def _k_fill(self, rounds):
        _lib.check(self.L.pfa_squared_fill_tape(_lib.ptr(self.state), C.byref(self.cfg), rounds, _lib.stream_handle()), 'fill_tape')

    def _k_reset(self, seed):
        self._wait_tape()
        _lib.check(self.L.pfa_squared_async_reset(_lib.ptr(self.state), C.byref(self.cfg), seed, *self._live(), _lib.stream_handle()),
                   'async_reset')
        self._tape_reset()

    def _before_send(self):
        self.ensure_tape(1)

    def _k_send(self, actions):
        """The caller has drawn the reset rounds (send() does; rollout loops call ensure_tape for many sends at once)."""
        self._wait_tape()
        _lib.check(self.L.pfa_squared_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(),
                                           _lib.stream_handle()), 'send')

    def fused_rollout_mlp(self, fp, experience, noise, key, stream, view=None):
        """clean_pufferl.evaluate's T-step loop as one persistent kernel (csrc/rollout.hip) over the flat 128-wide parameters `fp`,
        or over `view`: the pfa_mlp_view of a Default of another width (general.tile_view).  The caller has drawn the tape rounds."""
        if view is not None:
            _lib.check(self.L.pfa_rollout_mlp_view_squared(_lib.ptr(self.state), C.byref(self.cfg), C.byref(view), C.byref(experience.c),
                                                           _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(), stream), 'rollout')
        else:
            _lib.check(self.L.pfa_rollout_mlp_squared(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(fp.flat), C.byref(fp.dims),
                                                      C.byref(experience.c), _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(),
                                                      stream), 'rollout')
        self.sends += experience.horizon

    # -- test introspection -------------------------------------------------------------------------------
    def debug_targets(self):
        import torch
        out = torch.zeros(self.num_agents, self.cfg.num_targets, dtype=torch.int32, device=self.device)
        _lib.check(self.L.pfa_squared_debug_targets(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(out),
                                                    _lib.stream_handle()), 'debug_targets')
        return out.cpu().numpy()

    def debug_stream_pos(self):
        import torch
        out = torch.zeros(1, dtype=torch.int64, device=self.device)
        _lib.check(self.L.pfa_squared_debug_stream_pos(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(out),
                                                       _lib.stream_handle()), 'debug_stream_pos')
        return int(out.item())


def make_pixel_squared(distance_to_target=3, num_targets=1, height=64, width=64, channels=3, channels_last=True, **kwargs):
    """Env creator token of ocean Squared rendered as uint8 frames — the device env a conv policy can learn: make_squared's
    dynamics, shown as (height, width, channels) frames (channels_last) or (channels, height, width) ones."""
    return PixelSquaredSpec(distance_to_target, num_targets, height, width, channels, channels_last)


class PixelSquaredSpec(SquaredSpec):
    """SquaredSpec with the frame as observation.  Pixel (y, x) shows grid cell (y*g // height, x*g // width), g = 2d + 1; a cell
    shows 0 when empty, (255, 128) in (even, odd) channels for a target marker and (128, 255) for the agent: the three values differ in
    every channel.  Channels are colour planes, not a time stack."""
    MAX_CHANNELS = 4

    def __init__(self, distance_to_target=3, num_targets=1, height=64, width=64, channels=3, channels_last=True):
        super().__init__(distance_to_target, num_targets)
        self.height, self.width, self.channels, self.channels_last = int(height), int(width), int(channels), bool(channels_last)
        g = self.grid_size
        if self.height < g or self.width < g:
            raise APIUsageError(f'frames of {self.height} x {self.width} pixels cannot show a {g} x {g} grid: height and width must be at least {g}')
        if not 1 <= self.channels <= self.MAX_CHANNELS:
            raise APIUsageError(f'{self.channels} channels: the frame painter writes 1..{self.MAX_CHANNELS} colour planes')
        self.shape = (self.height, self.width, self.channels) if self.channels_last else (self.channels, self.height, self.width)
        if (self.height * self.width * self.channels) % 16 != 0:
            raise APIUsageError(f'frames of shape {self.shape}: the device env writes rows of a multiple of 16 bytes')
        self.single_observation_space = spaces.Box(low=0, high=255, shape=self.shape, dtype=np.uint8)
        self.observation_space = self.single_observation_space
        self.emulated = namespace(observation_dtype=np.dtype(np.uint8),
                                  emulated_observation_dtype=np.dtype((np.uint8, self.shape)))


class PixelSquared(_ResetTape, _DeviceVecEnv):
    """Device-resident vecenv of N ocean Squared envs shown as uint8 frames (csrc/pixel_squared.hip): `Squared`'s state machine, state
    layout, reset-target tape and statistics — rewards, terminals, infos and targets equal Squared's bit for bit at the same settings,
    seed and env count — with the float grid kept in the device state (``grid``) and the live observation a frame repainted from it on
    every send.  It has no fused rollout: a conv policy's step is many launches, so the trainer steps it (policy step + store + send)."""
    FAMILY = 'pixel_squared'
    NAMES = ('distance_to_target', 'num_targets', 'height', 'width', 'channels', 'channels_last')
    DEFAULTS = (3, 1, 64, 64, 3, True)
    SEEDED = True
    CONFIG_NAME = 'PixelSquared '
    ABI = 'pfa_squared'         # episode statistics and infos: Squared's entry points on the Squared block of the state
    OBS_U8 = True
    ROLLOUT_LSTM = None
    fused_rollout_mlp = None
    PREFETCH = False

    def _spec(self, d, nt, height, width, channels, channels_last):
        spec = PixelSquaredSpec(d, nt, height, width, channels, channels_last)
        self.obs_stride = spec.height * spec.width * spec.channels            # bytes per row
        return spec

    def _alloc_state(self):
        import torch
        sp = self.driver_env
        g = sp.grid_size
        self.obs_dim = self.obs_stride
        self.observations = self.obs_buf.view(self.num_agents, *sp.shape)
        self.episode_len = sp.num_targets * sp.distance_to_target + 1
        self.tape_rounds = 192
        grid_stride = _lib.round_up(g * g, 16)
        self.cfg = _lib.SquaredConfig(self.num_agents, sp.distance_to_target, sp.num_targets, grid_stride, self.tape_rounds)
        h, w, c = sp.height, sp.width, sp.channels
        self.pix = _lib.PixelConfig(h, w, c, *((1, w * c, c) if sp.channels_last else (h * w, w, 1)))
        nbytes = self.L.pfa_pixel_squared_state_bytes(C.byref(self.cfg), C.byref(self.pix))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        # the float grid Squared shows as its observation: rows of grid_stride floats behind the Squared block of the state
        self.grid = self.state[nbytes - self.num_agents * grid_stride * 4:].view(torch.float32).view(self.num_agents, grid_stride)
        sp._live_obs = self.grid
        self._tape_reset()

    _finishing_send = Squared._finishing_send
    _k_fill = Squared._k_fill
    _before_send = Squared._before_send
    debug_targets = Squared.debug_targets

    def _k_reset(self, seed):
        self._wait_tape()
        _lib.check(self.L.pfa_pixel_squared_async_reset(_lib.ptr(self.state), C.byref(self.cfg), C.byref(self.pix), seed, *self._live(),
                                                        _lib.stream_handle()), 'async_reset')
        self._tape_reset()

    def _k_send(self, actions):
        """The caller has drawn the reset rounds (send() does; the trainer's loop calls ensure_tape for many sends at once)."""
        self._wait_tape()
        _lib.check(self.L.pfa_pixel_squared_send(_lib.ptr(self.state), C.byref(self.cfg), C.byref(self.pix), _lib.ptr(actions), *self._live(),
                                                 _lib.stream_handle()), 'send')


def make_stochastic(p=0.7, horizon=100, **kwargs):
    """Env creator token with the signature of ocean.environment.make_stochastic (ocean/environment.py:61-64).  The
    reference's creator ignores its ``horizon`` argument and always builds Stochastic(horizon=100); so does this one."""
    return StochasticSpec(p)


class StochasticSpec(_SimpleSpec):
    """ocean.Stochastic (ocean.py:543-549)."""

    def __init__(self, p=0.7):
        super().__init__(0, 1, 2)
        self.p = float(p)
        self.horizon = 100


class Stochastic(_DeviceVecEnv):
    """Device-resident vecenv of N ocean Stochastic envs (csrc/stochastic.hip).  The env draws no random numbers, so there
    is no reset tape and seeds only matter to the policy's noise rows; it has a fused rollout kernel for the MLP policy."""
    FAMILY, NAMES, DEFAULTS = 'stochastic', ('p',), (0.7,)
    ABI = 'pfa_stochastic'

    def _spec(self, p):
        return StochasticSpec(p)

    def _alloc_state(self):
        import torch
        self.p, self.horizon = self.driver_env.p, self.driver_env.horizon
        self.episode_len = self.horizon + 1
        self.state = torch.zeros(self.L.pfa_stochastic_state_bytes(self.num_agents), dtype=torch.uint8, device=self.device)

    def _finishing_send(self, sends):
        return sends % self.episode_len == self.horizon

    def _k_reset(self, seed):
        _lib.check(self.L.pfa_stochastic_async_reset(_lib.ptr(self.state), self.num_agents, *self._live(), _lib.stream_handle()),
                   'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_stochastic_send(_lib.ptr(self.state), self.num_agents, self.p, self.horizon, _lib.ptr(actions),
                                              *self._live(), _lib.stream_handle()), 'send')

    def fused_rollout_mlp(self, fp, experience, noise, key, stream):
        """clean_pufferl.evaluate's T-step loop as one persistent kernel (csrc/stochastic.hip)."""
        _lib.check(self.L.pfa_rollout_mlp_stochastic(_lib.ptr(self.state), self.num_agents, self.p, self.horizon, _lib.ptr(fp.flat),
                                                     C.byref(fp.dims), C.byref(experience.c), _lib.ptr(noise), C.byref(key),
                                                     self.env_offset, *self._live(), stream), 'rollout_stochastic')
        self.sends += experience.horizon


def make_memory(mem_length=2, mem_delay=2, **kwargs):
    """Env creator token with the signature of ocean.environment.make_memory (ocean/environment.py:41-44)."""
    return MemorySpec(mem_length, mem_delay)


class MemorySpec(_SimpleSpec):
    """ocean.Memory (ocean.py:80-88)."""

    def __init__(self, mem_length=2, mem_delay=2):
        super().__init__(-1, 1, 2)
        self.mem_length, self.mem_delay = int(mem_length), int(mem_delay)
        self.horizon = 2 * self.mem_length + self.mem_delay


class Memory(_ResetTape, _DeviceVecEnv):
    """Device-resident vecenv of N ocean Memory envs (csrc/memory.hip) — the env family that needs the recurrent policy.
    The solutions of future episodes come from the tape the backend keeps ahead of the sends (numpy's process-global legacy
    stream, which does not depend on actions).  With the recurrent policy clean_pufferl.evaluate runs it in the fused rollout
    kernel (csrc/lstm_fused.hip); with the MLP policy it steps it through ``device_send`` (no host sync per step)."""
    FAMILY, NAMES, DEFAULTS = 'memory', ('mem_length', 'mem_delay'), (2, 2)
    SEEDED = True
    ABI = 'pfa_memory'
    ROLLOUT_LSTM = 'pfa_rollout_lstm_memory'

    def _spec(self, mem_length, mem_delay):
        return MemorySpec(mem_length, mem_delay)

    def _alloc_state(self):
        import torch
        self.horizon = self.driver_env.horizon
        self.episode_len = self.horizon          # H - 1 steps + the auto-reset row
        self.tape_rounds = 256
        self.cfg = _lib.MemoryConfig(self.num_agents, self.driver_env.mem_length, self.driver_env.mem_delay, self.tape_rounds)
        nbytes = self.L.pfa_memory_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._tape_reset()

    def _k_fill(self, rounds):
        _lib.check(self.L.pfa_memory_fill_tape(_lib.ptr(self.state), C.byref(self.cfg), rounds, _lib.stream_handle()), 'fill_tape')

    def _finishing_send(self, sends):
        return sends % self.episode_len == self.episode_len - 1

    def _k_reset(self, seed):
        _lib.check(self.L.pfa_memory_async_reset(_lib.ptr(self.state), C.byref(self.cfg), seed, *self._live(), _lib.stream_handle()),
                   'async_reset')
        self._tape_reset()

    def _k_send(self, actions):
        self.ensure_tape(1)
        _lib.check(self.L.pfa_memory_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(),
                                          _lib.stream_handle()), 'send')

    def debug_solutions(self):
        """(solution digits per env as a bit mask, tape underrun flag) — test introspection."""
        import torch
        bits = torch.zeros(self.num_agents, dtype=torch.int32, device=self.device)
        under = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.L.pfa_memory_debug_solutions(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(bits), _lib.ptr(under),
                                                     _lib.stream_handle()), 'debug_solutions')
        return bits.cpu().numpy(), int(under.item())


def make_spaces(**kwargs):
    """Env creator token with the signature of ocean.environment.make_spaces (ocean/environment.py:66-69)."""
    return SpacesSpec()


class SpacesSpec:
    """What ``driver_env`` exposes for ocean.Spaces behind GymnasiumPufferEnv: the EMULATED spaces (emulation.py:96-121) — the
    Dict observation {flat: int8[5], image: f32[5,5]} as 108 bytes (flat @0, image @8, numpy align=True), the Dict action
    {flat, image} as MultiDiscrete([2, 2]) in sorted-key order."""
    ROW_BYTES = 108

    def __init__(self):
        self.single_observation_space = spaces.Box(low=0, high=255, shape=(self.ROW_BYTES,), dtype=np.uint8)
        self.single_action_space = spaces.MultiDiscrete([2, 2])
        self.observation_space = self.single_observation_space
        self.action_space = self.single_action_space
        self.num_agents = 1
        self.render_mode = 'ansi'
        self.emulated = namespace(
            observation_dtype=np.dtype(np.uint8),
            emulated_observation_dtype=np.dtype([('flat', np.int8, (5,)), ('image', np.float32, (5, 5))], align=True))
        self.done = True

    def render(self):
        return ''

    def close(self):
        pass


class Spaces(_ResetTape, _DeviceVecEnv):
    """Device-resident vecenv of N ocean Spaces envs (csrc/spaces.hip): structured observation (108-byte emulated rows, kept
    on device as rows of 128 floats holding the byte values — what models.Default's ``observations.float()`` computes) and a
    MultiDiscrete([2, 2]) action.  Observations come from numpy's process-global legacy generator, whose data-dependent
    stream positions the tape kernel resolves ahead of the sends; ``async_reset(seed)`` = ``np.random.seed(seed)`` (what
    clean_pufferl.seed_everything does before it) followed by the initial resets.  clean_pufferl.evaluate steps it through
    ``device_send`` with packed action words (head h in bits 4h..4h+3), no host sync per step."""
    FAMILY, NAMES, DEFAULTS = 'spaces', (), ()
    ABI = 'pfa_spaces'
    SEEDED = False
    obs_stride = 128
    ROUNDS_AT_RESET = 1     # async_reset shows round 0
    RING_SPARE = 1
    FILL_HALVES = True

    def _spec(self):
        return SpacesSpec()

    def _alloc_state(self):
        import torch
        self.obs_dim = SpacesSpec.ROW_BYTES
        self.observations = self.obs_buf[:, :self.obs_dim]       # float byte values; recv() hands out the uint8 rows
        self.episode_len = 2                                      # one (terminal) step + the auto-reset row
        self.tape_rounds = 256
        self.cfg = _lib.SpacesConfig(self.num_agents, self.tape_rounds)
        nbytes = self.L.pfa_spaces_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._tape_reset()

    def _k_fill(self, rounds):
        _lib.check(self.L.pfa_spaces_fill_tape(_lib.ptr(self.state), C.byref(self.cfg), rounds, _lib.stream_handle()), 'fill_tape')

    def _finishing_send(self, sends):
        return sends % 2 == 1

    def _k_reset(self, seed):
        _lib.check(self.L.pfa_spaces_async_reset(_lib.ptr(self.state), C.byref(self.cfg), seed, *self._live(), _lib.stream_handle()),
                   'async_reset')
        self._tape_reset()

    def _k_send(self, actions):
        self.ensure_tape(1)
        _lib.check(self.L.pfa_spaces_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(),
                                          _lib.stream_handle()), 'send')

    def send(self, actions):
        """Actions [N, 2] = (flat, image) per env, as the reference's emulation hands them on (emulation.py:111-121)."""
        import torch
        send_precheck(self, actions)
        a = actions if torch.is_tensor(actions) else torch.as_tensor(np.ascontiguousarray(np.asarray(actions), dtype=np.int64))
        if tuple(a.shape) != (self.num_agents, 2) or (not self.initialized and (int(a.min()) < 0 or int(a.max()) > 1)):
            raise APIUsageError('Actions do not match action space')
        self.initialized = True
        a = a.to(device=self.device, dtype=torch.int64)
        self._actions.copy_(a[:, 0] | (a[:, 1] << 4))
        self.device_send(self._actions)
        self.infos = self._collect_infos() if self.info_mode == 'sync' else []

    def recv(self):
        import torch
        recv_precheck(self)
        return (self.observations.to(torch.uint8), self.rewards, self.terminals, self.truncations, self.infos, self.agent_ids,
                self.masks)


def make_synthetic(obs_values=160, num_actions=7, episode_length=100, obs_high=10, **kwargs):
    """Env creator token of the synthetic byte-row env (BASELINE configs[2]'s workload shape; defaults = MiniGrid's emulated row:
    160 bytes, 7 actions, episodes cut at 100 steps, minigrid/environment.py:14-48)."""
    return SyntheticSpec(obs_values, num_actions, episode_length, obs_high)


class SyntheticSpec(_SimpleSpec):
    def __init__(self, obs_values=160, num_actions=7, episode_length=100, obs_high=10):
        super().__init__(0, int(obs_high), int(num_actions))
        self.obs_values, self.num_actions = int(obs_values), int(num_actions)
        self.episode_length, self.obs_high = int(episode_length), int(obs_high)
        self.single_observation_space = spaces.Box(low=0, high=int(obs_high), shape=(self.obs_values,), dtype=np.uint8)
        self.observation_space = self.single_observation_space
        self.emulated = namespace(observation_dtype=np.dtype(np.uint8),
                                  emulated_observation_dtype=np.dtype((np.uint8, (self.obs_values,))))


class Synthetic(_DeviceVecEnv):
    """Device-resident synthetic byte-row vecenv (csrc/synth_env.hpp): observations from a counter-based generator keyed by
    (seed, global env, episode, tick), reward 1 when the action equals byte 0 of the shown row modulo the action count.  It is
    the workload of BASELINE configs[2] (MiniGrid-shaped rows + LSTM policy) — the third-party simulator itself is not part
    of the reference tree, so there is nothing to be bit-exact with on the env side."""
    FAMILY, NAMES, DEFAULTS = 'synthetic', ('obs_values', 'num_actions', 'episode_length', 'obs_high'), (160, 7, 100, 10)
    SEEDED = True
    ABI = 'pfa_synth'
    ROLLOUT_LSTM = 'pfa_rollout_lstm_synth'

    def _spec(self, obs_values, num_actions, episode_length, obs_high):
        from .cleanrl import obs_stride_for
        self.obs_stride = obs_stride_for(int(obs_values), recurrent=True)     # 16 .. 160 floats per row
        return SyntheticSpec(obs_values, num_actions, episode_length, obs_high)

    def _alloc_state(self):
        import torch
        sp = self.driver_env
        self.obs_dim = sp.obs_values
        self.observations = self.obs_buf[:, :self.obs_dim]
        self.episode_len = sp.episode_length + 1
        self.cfg = _lib.SynthConfig(self.num_agents, sp.obs_values, self.obs_stride, sp.num_actions, sp.episode_length, sp.obs_high, 0,
                                    self.env_offset)
        nbytes = self.L.pfa_synth_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _finishing_send(self, sends):
        return sends % self.episode_len == self.episode_len - 1

    def _k_reset(self, seed):
        self.cfg.seed = int(seed)
        self.cfg.env_offset = int(self.env_offset)
        _lib.check(self.L.pfa_synth_async_reset(_lib.ptr(self.state), C.byref(self.cfg), *self._live(), _lib.stream_handle()),
                   'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_synth_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(),
                                         _lib.stream_handle()), 'send')


def make_frames(framestack=4, num_actions=4, episode_length=100, height=84, width=84, channels_last=False, **kwargs):
    """Env creator token of the synthetic frame env (BASELINE configs[3]'s workload shape, SURVEY config C4: uint8
    (framestack, 84, 84) observations uniform in 0..255 as the Atari wrappers hand them to the NatureCNN, atari/environment.py:14-41,
    4 actions like Breakout).  height / width / channels_last give the other frame shapes models.Convolutional is bound to —
    (height, width, framestack) rows for the channel-last ones; the byte stream of a row does not depend on the shape's order."""
    return FramesSpec(framestack, num_actions, episode_length, height, width, channels_last)


class FramesSpec(_SimpleSpec):
    def __init__(self, framestack=4, num_actions=4, episode_length=100, height=84, width=84, channels_last=False):
        super().__init__(0, 255, int(num_actions))
        self.framestack, self.num_actions, self.episode_length = int(framestack), int(num_actions), int(episode_length)
        self.height, self.width, self.channels_last = int(height), int(width), bool(channels_last)
        self.shape = (self.height, self.width, self.framestack) if self.channels_last else (self.framestack, self.height, self.width)
        if (self.framestack * self.height * self.width) % 16 != 0:
            raise APIUsageError(f'frames of shape {self.shape}: the device env writes rows of a multiple of 16 bytes')
        self.single_observation_space = spaces.Box(low=0, high=255, shape=self.shape, dtype=np.uint8)
        self.observation_space = self.single_observation_space
        self.emulated = namespace(observation_dtype=np.dtype(np.uint8),
                                  emulated_observation_dtype=np.dtype((np.uint8, self.shape)))


class Frames(Synthetic):
    """Device-resident synthetic frame vecenv: the byte generator of ``Synthetic`` writing uint8 (framestack, 84, 84) rows (or any
    other frame shape, channel-first or channel-last: make_frames), reward 1
    when the action equals byte 0 of the shown frame modulo the action count.  Atari itself is a third-party emulator outside the
    reference tree (parity unpinned), so the workload keeps its observation / action shapes."""
    FAMILY, NAMES, DEFAULTS = 'frames', ('framestack', 'num_actions', 'episode_length', 'height', 'width', 'channels_last'), (4, 4, 100, 84, 84, False)
    OBS_U8 = True
    ROLLOUT_LSTM = None     # byte rows: a recurrent policy over frames is a conv LSTM, which runs on the GEMM-path engine

    def _spec(self, framestack, num_actions, episode_length, height=84, width=84, channels_last=False):
        self.obs_stride = int(framestack) * int(height) * int(width)            # bytes per row
        return FramesSpec(framestack, num_actions, episode_length, height, width, channels_last)

    def _alloc_state(self):
        import torch
        sp = self.driver_env
        self.obs_dim = self.obs_stride
        self.observations = self.obs_buf.view(self.num_agents, *sp.shape)
        self.episode_len = sp.episode_length + 1
        self.cfg = _lib.SynthConfig(self.num_agents, self.obs_stride, self.obs_stride, sp.num_actions, sp.episode_length, 255, 0, self.env_offset)
        nbytes = self.L.pfa_synth_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _k_reset(self, seed):
        self.cfg.seed = int(seed)
        self.cfg.env_offset = int(self.env_offset)
        _lib.check(self.L.pfa_frames_async_reset(_lib.ptr(self.state), C.byref(self.cfg), *self._live(), _lib.stream_handle()), 'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_frames_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(), _lib.stream_handle()),
                   'send')


class TabularMDP:
    """A finite MDP — or, with equal observation rows for different states, a POMDP — as tables: what `vector.Tabular` runs on the
    device.  Validated at construction, immutable afterwards (the arrays are read-only copies), hashable by identity.

      next_state [S][A][K] int     outcome k of action a in state s ([S][A]: one outcome each, a deterministic MDP)
      prob       [S][A][K] float64 outcome probabilities, every (s, a) row summing to 1 within 1e-9 (omitted with K = 1)
      reward     [S][A][K] float64 (or [S][A], the same for every outcome): the env's Python-float reward, cast to float32 on the
                                   buffer write and summed as float64 into the episode return (GymnasiumPufferEnv / EpisodeStats)
      terminal   [S] bool          entering such a state ends the episode
      obs        [S][D] float32    the row shown in state s, 1 <= D <= 160
      start      int, or (states[M], prob[M]): the initial-state distribution (no terminal state in it)
      horizon    int >= 1          the step that makes the episode this long ends it, reported as `terminal` (the reference drops
                                   truncations and only a terminal triggers the auto-reset)
      score      [S] float64, optional: infos['score'] = the entry of the state the episode ended in; default: the episode's return

    Limits: S <= 2^20, 1 <= A <= 1024, K <= 8, M <= S.  Every violation is a ValueError naming the field and the number.

    Probabilities become integer thresholds once, here, in float64 — the device kernels and any restatement read THESE integers:
      cum[s][a][k] = floor(2^32 * (prob[s][a][0] + ... + prob[s][a][k])) clipped to 2^32 - 1, as uint32   (`cum`, `start_cum`)
      outcome of a 32-bit word = the first k with word < cum[k]; if there is none (word >= cum[K-1], which only rounding makes
      possible) the last outcome with non-zero probability at this resolution, i.e. the last k whose cum[k] exceeds cum[k-1]
    — in one expression (`outcome`): the number of k with cum[k] <= min(word, cum[K-1] - 1).  A zero-probability outcome has
    cum[k] == cum[k-1] and is never drawn; probability 1.0 gives cum = 2^32 - 1 and relies on the fallback for the one word 2^32 - 1.
    The start distribution is treated the same way."""
    MAX_STATES, MAX_ACTIONS, MAX_OUTCOMES, MAX_OBS = 1 << 20, 1024, 8, 160

    def __init__(self, next_state, prob=None, reward=0.0, terminal=None, obs=None, start=0, horizon=None, score=None):
        nxt = np.asarray(next_state)
        if nxt.ndim == 2:
            nxt = nxt[:, :, None]
        if nxt.ndim != 3 or nxt.size == 0:
            raise ValueError(f'next_state: expected [S][A][K] (or [S][A]), got shape {nxt.shape}')
        S, A, K = nxt.shape
        if S > self.MAX_STATES:
            raise ValueError(f'next_state: {S} states, at most {self.MAX_STATES}')
        if A > self.MAX_ACTIONS:
            raise ValueError(f'next_state: {A} actions, at most {self.MAX_ACTIONS}')
        if K > self.MAX_OUTCOMES:
            raise ValueError(f'next_state: {K} outcomes per action, at most {self.MAX_OUTCOMES}')
        if not np.issubdtype(nxt.dtype, np.integer):
            if not np.all(np.isfinite(nxt)) or np.any(nxt != np.floor(nxt)):
                raise ValueError('next_state: entries must be finite integers')
        bad = (nxt < 0) | (nxt >= S)
        if bad.any():
            raise ValueError(f'next_state: index {int(nxt[bad][0])} at {tuple(int(i) for i in np.argwhere(bad)[0])} outside [0, {S})')
        nxt = nxt.astype(np.int32)

        if prob is None:
            if K != 1:
                raise ValueError(f'prob: required with {K} outcomes per action')
            pr = np.ones((S, A, 1), np.float64)
        else:
            pr = np.asarray(prob, np.float64)
            if pr.ndim == 2:
                pr = pr[:, :, None]
            if pr.shape != (S, A, K):
                raise ValueError(f'prob: shape {pr.shape}, expected {(S, A, K)}')
        if not np.all(np.isfinite(pr)):
            raise ValueError('prob: non-finite value')
        if (pr < 0).any():
            raise ValueError(f'prob: negative probability {float(pr[pr < 0][0])} at {tuple(int(i) for i in np.argwhere(pr < 0)[0])}')
        csum = np.cumsum(pr, axis=2)
        off = np.abs(csum[:, :, -1] - 1.0) > 1e-9
        if off.any():
            s_, a_ = (int(i) for i in np.argwhere(off)[0])
            raise ValueError(f'prob: row (state {s_}, action {a_}) sums to {float(csum[s_, a_, -1])!r}, not 1')

        rw = np.asarray(reward, np.float64)
        if rw.shape == (S, A):
            rw = rw[:, :, None]
        if rw.shape not in ((), (S, A, 1), (S, A, K)):
            raise ValueError(f'reward: shape {rw.shape}, expected {(S, A, K)} or {(S, A)}')
        rw = np.broadcast_to(rw, (S, A, K))
        if not np.all(np.isfinite(rw)):
            raise ValueError('reward: non-finite value')

        term = np.zeros(S, bool) if terminal is None else np.asarray(terminal)
        if term.shape != (S,):
            raise ValueError(f'terminal: shape {term.shape}, expected {(S,)}')
        term = term.astype(bool)

        if obs is None:
            raise ValueError('obs: required, [S][D] float32')
        ob = np.asarray(obs, np.float32)
        if ob.ndim == 1:
            ob = ob[:, None]
        if ob.ndim != 2 or ob.shape[0] != S:
            raise ValueError(f'obs: shape {ob.shape}, expected ({S}, D)')
        D = ob.shape[1]
        if not 1 <= D <= self.MAX_OBS:
            raise ValueError(f'obs: rows of {D} values, the device rows hold 1..{self.MAX_OBS}')
        if not np.all(np.isfinite(ob)):
            raise ValueError('obs: non-finite value')

        if np.ndim(start) == 0:
            st_states, st_prob = np.asarray([start]), np.ones(1, np.float64)
        else:
            try:
                st_states, st_prob = start
            except (TypeError, ValueError):
                raise ValueError('start: expected a state index or (states[M], prob[M])') from None
            st_states, st_prob = np.asarray(st_states), np.asarray(st_prob, np.float64)
        if st_states.ndim != 1 or st_states.shape != st_prob.shape or st_states.size == 0:
            raise ValueError(f'start: states of shape {st_states.shape} and prob of shape {st_prob.shape}, expected two [M] arrays')
        M = st_states.size
        if M > S:
            raise ValueError(f'start: {M} entries for {S} states')
        if not np.all(np.isfinite(st_prob)) or not np.all(np.isfinite(st_states.astype(np.float64))):
            raise ValueError('start: non-finite value')
        if np.any(st_states != np.floor(st_states)) or (st_states < 0).any() or (st_states >= S).any():
            badv = st_states[(st_states != np.floor(st_states)) | (st_states < 0) | (st_states >= S)][0]
            raise ValueError(f'start: state {badv} outside [0, {S})')
        st_states = st_states.astype(np.int32)
        if (st_prob < 0).any():
            raise ValueError(f'start: negative probability {float(st_prob[st_prob < 0][0])}')
        st_csum = np.cumsum(st_prob)
        if abs(st_csum[-1] - 1.0) > 1e-9:
            raise ValueError(f'start: probabilities sum to {float(st_csum[-1])!r}, not 1')
        if term[st_states].any():
            raise ValueError(f'start: state {int(st_states[term[st_states]][0])} is terminal')

        if horizon is None or int(horizon) != horizon or int(horizon) < 1 or int(horizon) >= 2 ** 31:
            raise ValueError(f'horizon: {horizon!r}, expected an integer >= 1')

        sc = None
        if score is not None:
            sc = np.asarray(score, np.float64)
            if sc.shape != (S,):
                raise ValueError(f'score: shape {sc.shape}, expected {(S,)}')
            if not np.all(np.isfinite(sc)):
                raise ValueError('score: non-finite value')

        def frozen(a):
            a = np.array(a, copy=True, order='C')
            a.setflags(write=False)
            return a
        d = self.__dict__
        d['num_states'], d['num_actions'], d['num_outcomes'], d['num_starts'], d['obs_dim'] = S, A, K, M, D
        d['next_state'], d['prob'], d['reward'], d['terminal'], d['obs'] = frozen(nxt), frozen(pr), frozen(rw), frozen(term), frozen(ob)
        d['start_states'], d['start_prob'], d['horizon'] = frozen(st_states), frozen(st_prob), int(horizon)
        d['score'] = None if sc is None else frozen(sc)
        d['cum'], d['start_cum'] = frozen(self.thresholds(csum)), frozen(self.thresholds(st_csum))

    def __setattr__(self, name, value):
        raise AttributeError('TabularMDP is immutable')

    __delattr__ = __setattr__

    @staticmethod
    def thresholds(cumulative):
        """floor(2^32 * cumulative probability) clipped to 2^32 - 1, as uint32 (float64 arithmetic; the product is exact)."""
        return np.minimum(np.floor(np.asarray(cumulative, np.float64) * 4294967296.0), 4294967295.0).astype(np.uint32)

    @staticmethod
    def outcome(cum, word):
        """The outcome a 32-bit word selects from one row of thresholds (the rule in the class docstring)."""
        cum = np.asarray(cum, np.uint32)
        return int(np.searchsorted(cum, min(int(word), int(cum[-1]) - 1), side='right'))

    @classmethod
    def gridworld(cls, rows, cols, goal=None, slip=0.0, horizon=None):
        """rows x cols cells, state = row * cols + col, one-hot observation (D = rows * cols <= 160), actions 0..3 = up / down / left /
        right; a move off the grid stays.  With slip > 0 a move has three outcomes: as intended with probability 1 - slip, to either
        side (the two perpendicular directions) with slip / 2 each.  Entering `goal` ((row, col) or a state index; default: the last
        cell) gives reward 1 and ends the episode; every other step gives 0.  Uniform start over the non-goal cells."""
        rows, cols = int(rows), int(cols)
        S = rows * cols
        if rows < 1 or cols < 1 or S < 2:
            raise ValueError(f'gridworld: {rows} x {cols} cells, need at least two')
        g = S - 1 if goal is None else (int(goal[0]) * cols + int(goal[1]) if np.ndim(goal) else int(goal))
        if not 0 <= g < S or (np.ndim(goal) and not (0 <= goal[0] < rows and 0 <= goal[1] < cols)):
            raise ValueError(f'gridworld: goal {goal!r} outside the {rows} x {cols} grid')
        if not 0.0 <= slip <= 1.0:
            raise ValueError(f'gridworld: slip {slip!r} outside [0, 1]')
        moves = ((-1, 0), (1, 0), (0, -1), (0, 1))
        sides = ((2, 3), (2, 3), (0, 1), (0, 1))

        def to(s, m):
            r, c = divmod(s, cols)
            r2, c2 = r + moves[m][0], c + moves[m][1]
            return r2 * cols + c2 if 0 <= r2 < rows and 0 <= c2 < cols else s
        K = 3 if slip > 0 else 1
        nxt = np.zeros((S, 4, K), np.int32)
        for s in range(S):
            for a in range(4):
                nxt[s, a, 0] = to(s, a)
                if K == 3:
                    nxt[s, a, 1], nxt[s, a, 2] = to(s, sides[a][0]), to(s, sides[a][1])
        prob = np.broadcast_to(np.array([1.0 - slip, slip / 2, slip / 2]), (S, 4, 3)) if K == 3 else None
        terminal = np.arange(S) == g
        starts = np.flatnonzero(~terminal)
        return cls(nxt, prob, reward=(nxt == g).astype(np.float64), terminal=terminal, obs=np.eye(S, dtype=np.float32),
                   start=(starts, np.full(starts.size, 1.0 / starts.size)), horizon=4 * (rows + cols) if horizon is None else horizon)

    @classmethod
    def tmaze(cls, length):
        """The cue-and-recall task: a cue (0 or 1, equally likely) is shown in the first observation only, then `length - 1` blank
        corridor cells follow, then a junction; in the corridor either action walks on, at the junction action == cue ends the episode
        with reward and score 1, the other action with 0.  D = 3: (cue is 0, cue is 1, at the junction); A = 2; an episode takes
        length + 1 steps.  States: cue c at position p (0 .. length) = c * (length + 1) + p, then the two end states."""
        length = int(length)
        if length < 1:
            raise ValueError(f'tmaze: length {length}, need at least 1')
        P = length + 1
        S = 2 * P + 2
        win, lose = 2 * P, 2 * P + 1
        nxt = np.zeros((S, 2), np.int32)
        obs = np.zeros((S, 3), np.float32)
        for c in (0, 1):
            for p in range(length):
                nxt[c * P + p] = c * P + p + 1
            nxt[c * P + length, c], nxt[c * P + length, 1 - c] = win, lose
            obs[c * P, c] = 1.0
            obs[c * P + length, 2] = 1.0
        nxt[win], nxt[lose] = win, lose
        terminal = np.zeros(S, bool)
        terminal[[win, lose]] = True
        score = np.zeros(S, np.float64)
        score[win] = 1.0
        return cls(nxt, reward=(nxt == win).astype(np.float64), terminal=terminal, obs=obs, start=([0, P], [0.5, 0.5]), horizon=P,
                   score=score)


def make_tabular(mdp=None, obs_stride=None, **kwargs):
    """Env creator token of a user-given `TabularMDP`: vector.make(make_tabular, env_kwargs=dict(mdp=mdp), backend=Tabular, ...).
    obs_stride: floats per device observation row (default: the narrowest of 16 / 32 / 64 / 96 / 128 that holds the row; 160 for
    wider rows under the recurrent policy)."""
    return TabularSpec(mdp)


class TabularSpec(_SimpleSpec):
    """What ``driver_env`` exposes for a TabularMDP: Box(obs.min(), obs.max(), (D,), float32) and Discrete(A)."""

    def __init__(self, mdp):
        if not isinstance(mdp, TabularMDP):
            raise APIUsageError(f'make_tabular needs mdp=<vector.TabularMDP> (got {type(mdp).__name__})')
        super().__init__(float(mdp.obs.min()), float(mdp.obs.max()), mdp.num_actions)
        self.mdp = mdp
        self.single_observation_space = spaces.Box(low=float(mdp.obs.min()), high=float(mdp.obs.max()), shape=(mdp.obs_dim,), dtype=np.float32)
        self.observation_space = self.single_observation_space
        self.emulated = namespace(observation_dtype=np.dtype(np.float32),
                                  emulated_observation_dtype=np.dtype((np.float32, (mdp.obs_dim,))))


class Tabular(_DeviceVecEnv):
    """Device-resident vecenv of N copies of one user-given `TabularMDP` (csrc/tabular_env.hpp, csrc/tabular.hip): the tables are
    uploaded once and walked by the kernels; randomness is counter-based — Philox keyed by (seed, global env, episode, tick) — so there
    is no tape and envs `env_offset ..` of a larger vecenv are reproduced exactly.  It has a fused rollout kernel for either policy (up
    to 15 actions); other policy shapes step it through ``device_send``.  Episodes end on different sends in different envs: in
    info_mode 'sync' every send reads the finished flags back (one small D2H), in 'lazy' none does."""
    FAMILY = 'tabular'
    ABI = 'pfa_tabular'
    SEEDED = True
    CONFIG_NAME = 'Tabular '
    ROLLOUT_LSTM = 'pfa_rollout_lstm_tabular'

    def __init__(self, env_creators, env_args, env_kwargs, num_envs, obs_stride=None, **kwargs):
        self._obs_stride_arg = obs_stride
        self._mdps = {}
        super().__init__(env_creators, env_args, env_kwargs, num_envs, **kwargs)

    def _creator_spec(self, creator, args, kwargs):
        mdp, stride = _creator_kwargs(creator, args, kwargs, ('mdp', 'obs_stride'), (None, None), self.FAMILY)
        if not isinstance(mdp, TabularMDP):
            raise APIUsageError(f'make_tabular needs mdp=<vector.TabularMDP> (got {type(mdp).__name__})')
        self._mdps[id(mdp)] = mdp
        stride = self._obs_stride_arg if stride is None else stride
        return id(mdp), (None if stride is None else int(stride))

    def _spec(self, mdp_id, stride):
        from .cleanrl import KERNEL_STRIDES, RECURRENT_STRIDES
        mdp = self._mdps[mdp_id]
        D = mdp.obs_dim
        if stride is None:
            if D > KERNEL_STRIDES[-1]:
                raise APIUsageError(f'observation rows of {D} values: the feed-forward kernels take rows of up to {KERNEL_STRIDES[-1]} floats; '
                                    f'pass obs_stride={RECURRENT_STRIDES[-1]} (the recurrent policy\'s widest row)')
            stride = next(s for s in KERNEL_STRIDES if D <= s)
        elif stride not in RECURRENT_STRIDES or stride < D:
            raise APIUsageError(f'obs_stride {stride}: must be one of {RECURRENT_STRIDES} and hold the {D} observation values')
        self.obs_stride = stride
        return TabularSpec(mdp)

    def _alloc_state(self):
        import torch
        mdp, dev = self.driver_env.mdp, self.device
        self.mdp = mdp
        self.obs_dim = mdp.obs_dim
        self.observations = self.obs_buf[:, :self.obs_dim]
        obs = np.zeros((mdp.num_states, self.obs_stride), np.float32)
        obs[:, :mdp.obs_dim] = mdp.obs

        def up(a, as_int32=False):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(np.array(a.view(np.int32) if as_int32 else a)).to(dev)
        # the device tables, kept alive by the vecenv (uint32 thresholds travel as their int32 bit patterns)
        self.tables = dict(next=up(mdp.next_state), cum=up(mdp.cum, True), reward=up(mdp.reward), terminal=up(mdp.terminal.astype(np.uint8)),
                           score=None if mdp.score is None else up(mdp.score), obs=up(obs), start_states=up(mdp.start_states),
                           start_cum=up(mdp.start_cum, True))
        t = self.tables
        self.cfg = _lib.TabularConfig(self.num_agents, mdp.num_states, mdp.num_actions, mdp.num_outcomes, mdp.num_starts, mdp.obs_dim,
                                      self.obs_stride, mdp.horizon, 0, self.env_offset,
                                      *(None if t[k] is None else t[k].data_ptr()
                                        for k in ('next', 'cum', 'reward', 'terminal', 'score', 'obs', 'start_states', 'start_cum')))
        nbytes = self.L.pfa_tabular_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def _finishing_send(self, sends):
        return True         # episodes end on different sends in different envs

    def _k_reset(self, seed):
        self.cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg.env_offset = int(self.env_offset)
        _lib.check(self.L.pfa_tabular_async_reset(_lib.ptr(self.state), C.byref(self.cfg), *self._live(), _lib.stream_handle()), 'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_tabular_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(), _lib.stream_handle()),
                   'send')

    def fused_rollout_mlp(self, fp, experience, noise, key, stream):
        """clean_pufferl.evaluate's T-step loop as one persistent kernel (csrc/tabular.hip)."""
        _lib.check(self.L.pfa_rollout_mlp_tabular(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(fp.flat), C.byref(fp.dims),
                                                  C.byref(experience.c), _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(),
                                                  stream), 'rollout_mlp_tabular')
        self.sends += experience.horizon

    def debug_states(self):
        """[N][5] int32: (state, episode, tick, done, ep_length) of every env — test introspection."""
        import torch
        out = torch.zeros(self.num_agents, 5, dtype=torch.int32, device=self.device)
        _lib.check(self.L.pfa_tabular_debug_states(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(out), _lib.stream_handle()),
                   'debug_states')
        return out.cpu().numpy()


def make_cartpole(max_steps=500, velocities=True, **kwargs):
    """Env creator token of classic-control cart-pole: vector.make(make_cartpole, backend=CartPole, ...).  max_steps: the time limit
    that ends an episode (500 is CartPole-v1's registered limit; 0 = none, which is what the reference's classic_control creator
    builds).  velocities=False hides x_dot and theta_dot from the observation: the partially observed task."""
    return CartPoleSpec(max_steps, velocities)


class CartPoleSpec(_SimpleSpec):
    """What ``driver_env`` exposes for cart-pole: gymnasium's Box(+-[4.8, f32 max, 24 degrees, f32 max], float32) and Discrete(2)."""

    def __init__(self, max_steps=500, velocities=True):
        import math
        super().__init__(0, 1, 2)
        self.max_steps, self.velocities = int(max_steps), bool(velocities)
        fmax = np.finfo(np.float32).max
        high = np.array([2.4 * 2, fmax, 12 * 2 * math.pi / 360 * 2, fmax], dtype=np.float32)
        self.single_observation_space = spaces.Box(low=-high, high=high, shape=(4,), dtype=np.float32)
        self.observation_space = self.single_observation_space
        self.emulated = namespace(observation_dtype=np.dtype(np.float32), emulated_observation_dtype=np.dtype((np.float32, (4,))))


class CartPole(_DeviceVecEnv):
    """Device-resident vecenv of N classic-control cart-poles (csrc/cartpole_env.hpp, csrc/cartpole.hip): f64 dynamics, real-valued
    observations.  The start states are counter-based — Philox keyed by (seed, global env, episode) — so there is no tape and envs
    `env_offset ..` of a larger vecenv are reproduced exactly.  It has a fused rollout kernel for the recurrent policy and for
    Default at every tile width (64 / 128 / 256 / 512).  Episodes end on different sends in different envs: in info_mode 'sync' every
    send reads the finished flags back (one small D2H), in 'lazy' none does."""
    FAMILY, NAMES, DEFAULTS = 'cartpole', ('max_steps', 'velocities'), (500, True)
    ABI = 'pfa_cartpole'
    SEEDED = True
    CONFIG_NAME = 'CartPole '
    ROLLOUT_LSTM = 'pfa_rollout_lstm_cartpole'
    ROLLOUT_MLP_VIEW = True

    def _spec(self, max_steps, velocities):
        return CartPoleSpec(max_steps, velocities)

    def _alloc_state(self):
        import torch
        sp = self.driver_env
        self.obs_dim = 4
        self.observations = self.obs_buf[:, :4]
        self.cfg = _lib.CartPoleConfig(self.num_agents, sp.max_steps, 1 if sp.velocities else 0, 0, 0, self.env_offset)
        nbytes = self.L.pfa_cartpole_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _finishing_send(self, sends):
        return True         # episodes end on different sends in different envs

    def _k_reset(self, seed):
        self.cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg.env_offset = int(self.env_offset)
        _lib.check(self.L.pfa_cartpole_async_reset(_lib.ptr(self.state), C.byref(self.cfg), *self._live(), _lib.stream_handle()), 'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_cartpole_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(), _lib.stream_handle()),
                   'send')

    def fused_rollout_mlp(self, fp, experience, noise, key, stream, view=None):
        """clean_pufferl.evaluate's T-step loop as one persistent kernel (csrc/cartpole.hip) over the flat 128-wide parameters `fp`, or
        over `view`: the pfa_mlp_view of a Default of another width (general.tile_view)."""
        if view is not None:
            _lib.check(self.L.pfa_rollout_mlp_view_cartpole(_lib.ptr(self.state), C.byref(self.cfg), C.byref(view), C.byref(experience.c),
                                                            _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(), stream),
                       'rollout_mlp_view_cartpole')
        else:
            _lib.check(self.L.pfa_rollout_mlp_cartpole(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(fp.flat), C.byref(fp.dims),
                                                       C.byref(experience.c), _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(),
                                                       stream), 'rollout_mlp_cartpole')
        self.sends += experience.horizon

    def debug_states(self):
        """([N][4] float64: x, x_dot, theta, theta_dot; [N][4] int32: episode, tick, done, ep_length) — test introspection."""
        import torch
        states = torch.zeros(self.num_agents, 4, dtype=torch.float64, device=self.device)
        counters = torch.zeros(self.num_agents, 4, dtype=torch.int32, device=self.device)
        _lib.check(self.L.pfa_cartpole_debug_states(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(states), _lib.ptr(counters),
                                                    _lib.stream_handle()), 'debug_states')
        return states.cpu().numpy(), counters.cpu().numpy()


def make_acrobot(max_steps=500, velocities=True, **kwargs):
    """Env creator token of classic-control acrobot: vector.make(make_acrobot, backend=Acrobot, ...).  max_steps: the time limit that
    ends an episode (500 is Acrobot-v1's registered limit; 0 = none).  velocities=False hides the two angular velocities from the
    observation: the partially observed task."""
    return AcrobotSpec(max_steps, velocities)


class AcrobotSpec(_SimpleSpec):
    """What ``driver_env`` exposes for acrobot: gymnasium's Box(+-[1, 1, 1, 1, 4 pi, 9 pi], float32) and Discrete(3)."""

    def __init__(self, max_steps=500, velocities=True):
        import math
        super().__init__(0, 1, 3)
        self.max_steps, self.velocities = int(max_steps), bool(velocities)
        high = np.array([1.0, 1.0, 1.0, 1.0, 4 * math.pi, 9 * math.pi], dtype=np.float32)
        self.single_observation_space = spaces.Box(low=-high, high=high, shape=(6,), dtype=np.float32)
        self.observation_space = self.single_observation_space
        self.emulated = namespace(observation_dtype=np.dtype(np.float32), emulated_observation_dtype=np.dtype((np.float32, (6,))))


class Acrobot(_DeviceVecEnv):
    """Device-resident vecenv of N classic-control acrobots (csrc/acrobot_env.hpp, csrc/acrobot.hip): f64 RK4 dynamics, observations
    (cos th1, sin th1, cos th2, sin th2, w1, w2), three torques, reward -1 per step until the tip swings above the bar.  The start
    states are counter-based — Philox keyed by (seed, global env, episode) — so there is no tape and envs `env_offset ..` of a larger
    vecenv are reproduced exactly.  It has a fused rollout kernel for the recurrent policy and for Default at every tile width (64 /
    128 / 256 / 512).  Episodes end on different sends in different envs: in info_mode 'sync' every send reads the finished flags back
    (one small D2H), in 'lazy' none does."""
    FAMILY, NAMES, DEFAULTS = 'acrobot', ('max_steps', 'velocities'), (500, True)
    ABI = 'pfa_acrobot'
    SEEDED = True
    CONFIG_NAME = 'Acrobot '
    ROLLOUT_LSTM = 'pfa_rollout_lstm_acrobot'
    ROLLOUT_MLP_VIEW = True

    def _spec(self, max_steps, velocities):
        return AcrobotSpec(max_steps, velocities)

    def _alloc_state(self):
        import torch
        sp = self.driver_env
        self.obs_dim = 6
        self.observations = self.obs_buf[:, :6]
        self.cfg = _lib.AcrobotConfig(self.num_agents, sp.max_steps, 1 if sp.velocities else 0, 0, 0, self.env_offset)
        nbytes = self.L.pfa_acrobot_state_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise APIUsageError(self.L.pfa_last_error().decode())
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _finishing_send(self, sends):
        return True         # episodes end on different sends in different envs

    def _k_reset(self, seed):
        self.cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg.env_offset = int(self.env_offset)
        _lib.check(self.L.pfa_acrobot_async_reset(_lib.ptr(self.state), C.byref(self.cfg), *self._live(), _lib.stream_handle()), 'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_acrobot_send(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(actions), *self._live(), _lib.stream_handle()),
                   'send')

    def fused_rollout_mlp(self, fp, experience, noise, key, stream, view=None):
        """clean_pufferl.evaluate's T-step loop as one persistent kernel (csrc/acrobot.hip) over the flat 128-wide parameters `fp`, or
        over `view`: the pfa_mlp_view of a Default of another width (general.tile_view)."""
        if view is not None:
            _lib.check(self.L.pfa_rollout_mlp_view_acrobot(_lib.ptr(self.state), C.byref(self.cfg), C.byref(view), C.byref(experience.c),
                                                           _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(), stream),
                       'rollout_mlp_view_acrobot')
        else:
            _lib.check(self.L.pfa_rollout_mlp_acrobot(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(fp.flat), C.byref(fp.dims),
                                                      C.byref(experience.c), _lib.ptr(noise), C.byref(key), self.env_offset, *self._live(),
                                                      stream), 'rollout_mlp_acrobot')
        self.sends += experience.horizon

    def debug_states(self):
        """([N][4] float64: th1, th2, w1, w2; [N][4] int32: episode, tick, done, ep_length) — test introspection."""
        import torch
        states = torch.zeros(self.num_agents, 4, dtype=torch.float64, device=self.device)
        counters = torch.zeros(self.num_agents, 4, dtype=torch.int32, device=self.device)
        _lib.check(self.L.pfa_acrobot_debug_states(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(states), _lib.ptr(counters),
                                                   _lib.stream_handle()), 'debug_states')
        return states.cpu().numpy(), counters.cpu().numpy()

    def debug_set_states(self, states, counters):
        """The inverse of debug_states(), for tests that put envs on the rare branches on purpose (an angle about to wrap, a velocity
        at its clamp, a state one step below the height threshold): env e becomes an episode ep_length steps old, with return
        -ep_length, in the given state; its live observation row and terminal flag follow.  The states must lie inside the state box
        (|th| <= pi, |w1| <= 4 pi, |w2| <= 9 pi) and the counters must be non-negative."""
        import math
        import torch
        states, counters = np.asarray(states), np.asarray(counters)
        n = self.num_agents
        if states.shape != (n, 4) or counters.shape != (n, 4):
            raise APIUsageError(f'Acrobot.debug_set_states: states and counters must have shape ({n}, 4), got {states.shape} and {counters.shape}')
        states, counters = np.ascontiguousarray(states, dtype=np.float64), np.ascontiguousarray(counters, dtype=np.int32)
        if not (np.abs(states) <= np.array([math.pi, math.pi, 4 * math.pi, 9 * math.pi])).all() or (counters < 0).any():
            raise APIUsageError('Acrobot.debug_set_states: a state outside the state box (|th| <= pi, |w1| <= 4 pi, |w2| <= 9 pi) or a negative counter')
        st, cn = torch.as_tensor(states).to(self.device), torch.as_tensor(counters).to(self.device)
        _lib.check(self.L.pfa_acrobot_debug_set_states(_lib.ptr(self.state), C.byref(self.cfg), _lib.ptr(st), _lib.ptr(cn),
                                                       _lib.ptr(self.obs_buf), _lib.ptr(self.terminals_u8), _lib.stream_handle()),
                   'debug_set_states')
        torch.cuda.current_stream().synchronize()       # st and cn are freed on return


def make_bandit(num_actions=10, reward_scale=1, reward_noise=1, **kwargs):
    """Env creator token with the signature of ocean.environment.make_bandit (ocean/environment.py:33-37)."""
    return BanditSpec(num_actions, reward_scale, reward_noise)


class BanditSpec(_SimpleSpec):
    """ocean.Bandit (ocean.py:22-31)."""

    def __init__(self, num_actions=10, reward_scale=1, reward_noise=1):
        super().__init__(-1, 1, int(num_actions))
        self.num_actions, self.reward_scale, self.reward_noise = int(num_actions), reward_scale, reward_noise
        self.hard_fixed_seed = 42


class Bandit(_DeviceVecEnv):
    """Device-resident vecenv of N ocean Bandit envs (csrc/bandit.hip).  Every reset reseeds numpy's global generator with the
    hard fixed seed, so the solution and the reward noise env i sees are the same in every episode: they are drawn here,
    once, with numpy's own legacy RandomState — the generator the reference calls — and the kernels keep the state machine."""
    FAMILY, NAMES, DEFAULTS = 'bandit', ('num_actions', 'reward_scale', 'reward_noise'), (10, 1, 1)
    ABI = 'pfa_bandit'
    MAX_ACTIONS = 15       # what every policy tier takes, the fused 128-wide kernels included (WideBandit: the GEMM path's limit)

    def _spec(self, num_actions, reward_scale, reward_noise):
        return BanditSpec(num_actions, reward_scale, reward_noise)

    def _alloc_state(self):
        import torch
        spec = self.driver_env
        if not 2 <= spec.num_actions <= self.MAX_ACTIONS:
            raise APIUsageError(f'the policy kernels take 1..{self.MAX_ACTIONS} actions')
        self.episode_len = 2                      # one step + the auto-reset row
        rs = np.random.RandomState(spec.hard_fixed_seed)              # ocean.py:36-42: seed(42) then randint for the solution
        self.solution = int(rs.randint(0, spec.num_actions))
        self.scale = float(spec.reward_scale)
        self.noise = None
        if spec.reward_noise != 0:                                     # ocean.py:55-57: randn() * reward_scale, env order
            table = np.array([rs.randn() * spec.reward_scale for _ in range(self.num_agents)], np.float64)
            self.noise = torch.as_tensor(table).to(self.device)
        self.state = torch.zeros(self.L.pfa_bandit_state_bytes(self.num_agents), dtype=torch.uint8, device=self.device)

    def _finishing_send(self, sends):
        return sends % 2 == 1

    def _k_reset(self, seed):
        _lib.check(self.L.pfa_bandit_async_reset(_lib.ptr(self.state), self.num_agents, *self._live(), _lib.stream_handle()),
                   'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_bandit_send(_lib.ptr(self.state), self.num_agents, self.solution, self.scale, _lib.ptr(self.noise),
                                          _lib.ptr(actions), *self._live(), _lib.stream_handle()), 'send')


class WideBandit(Bandit):
    """`Bandit` with any action count the reference's make_bandit(num_actions=...) is given, up to the 1024 logits one Discrete head
    of the GEMM-path policy engine takes (general.MAX_LOGITS): the same kernels and state.  A class of its own because `Bandit`
    refuses more than 15 actions at construction, and callers rely on that refusal; policies on more than 15 actions run through
    general.Engine with stepwise rollouts."""
    MAX_ACTIONS = 1024


def make_multiagent(**kwargs):
    """Env creator token with the signature of ocean.environment.make_multiagent (ocean/environment.py:76-79)."""
    return MultiagentSpec()


class MultiagentSpec(_SimpleSpec):
    """ocean.Multiagent behind PettingZooPufferEnv (ocean.py:148-174, emulation.py:236-306)."""

    def __init__(self):
        super().__init__(0, 1, 2)
        self.num_agents = 2
        self.possible_agents = [1, 2]


class Multiagent(_DeviceVecEnv):
    """Device-resident vecenv of N ocean Multiagent envs (csrc/multiagent.hip): two agent rows per env, env-major, so
    ``num_agents == 2 * len(env_creators)`` like the reference's Serial over PettingZooPufferEnv (vector.py:86-93).  Infos are
    the env's own ``{1: {'score': r}, 2: {'score': r}}`` per env; ``episode_stats`` holds the per-slot sums behind the
    ``1/score`` / ``2/score`` means clean_pufferl.evaluate reports."""
    FAMILY, NAMES, DEFAULTS = 'multiagent', (), ()
    ABI = 'pfa_multiagent'
    AGENTS_PER_ENV = 2

    def _spec(self):
        return MultiagentSpec()

    def _alloc_state(self):
        import torch
        self.episode_len = 2
        self.state = torch.zeros(self.L.pfa_multiagent_state_bytes(self.env_count), dtype=torch.uint8, device=self.device)

    def _finishing_send(self, sends):
        return sends % 2 == 1

    def _k_reset(self, seed):
        _lib.check(self.L.pfa_multiagent_async_reset(_lib.ptr(self.state), self.env_count, *self._live(), _lib.stream_handle()),
                   'async_reset')

    def _k_send(self, actions):
        _lib.check(self.L.pfa_multiagent_send(_lib.ptr(self.state), self.env_count, _lib.ptr(actions), *self._live(),
                                              _lib.stream_handle()), 'send')

    def _collect_infos(self):
        if not self._finishing_send(self.sends):
            return []
        r = self.rewards.cpu().numpy().astype(np.int64).reshape(-1, 2)      # ocean.py:207-210: score = the int reward
        return [{1: {'score': int(a)}, 2: {'score': int(b)}} for a, b in r]

    @staticmethod
    def stats_from_sums(st):
        out = {}
        if st[0] > 0:
            out['1/score'] = st[1] / st[0]
        if st[2] > 0:
            out['2/score'] = st[3] / st[2]
        return out


def make(env_creator_or_creators, env_args=None, env_kwargs=None, backend=Squared, num_envs=1, **kwargs):
    """pufferlib.vector.make (vector.py:577-637): same argument validation and error messages.

    Deliberate interface mirror of vector.py:579-624 — the reference's tests (tests/test_api.py:15-131) and user code match on these
    APIUsageError messages, so the checks keep the reference's order and wording.  Interface, not hot path."""
    if num_envs < 1:
        raise APIUsageError('num_envs must be at least 1')
    if num_envs != int(num_envs):
        raise APIUsageError('num_envs must be an integer')

    if 'num_workers' in kwargs:
        num_workers = kwargs['num_workers']
        envs_per_worker = num_envs / num_workers
        if envs_per_worker != int(envs_per_worker):
            raise APIUsageError('num_envs must be divisible by num_workers')
        if 'batch_size' in kwargs:
            batch_size = kwargs['batch_size']
            if batch_size is None:
                batch_size = num_envs
            if batch_size % envs_per_worker != 0:
                raise APIUsageError('batch_size must be divisible by (num_envs / num_workers)')

    if env_args is None:
        env_args = []
    if env_kwargs is None:
        env_kwargs = {}

    if not isinstance(env_creator_or_creators, (list, tuple)):
        env_creators = [env_creator_or_creators] * num_envs
        env_args = [env_args] * num_envs
        env_kwargs = [env_kwargs] * num_envs
    else:
        env_creators = env_creator_or_creators

    if len(env_creators) != num_envs:
        raise APIUsageError('env_creators must be a list of length num_envs')
    if len(env_args) != num_envs:
        raise APIUsageError('env_args must be a list of length num_envs')
    if len(env_kwargs) != num_envs:
        raise APIUsageError('env_kwargs must be a list of length num_envs')

    for i in range(num_envs):
        if not callable(env_creators[i]):
            raise APIUsageError('env_creators must be a list of callables')
        if not isinstance(env_args[i], (list, tuple)):
            raise APIUsageError('env_args must be a list of lists or tuples')
        if not isinstance(env_kwargs[i], (dict, Namespace)):
            raise APIUsageError('env_kwargs must be a list of dictionaries')

    for k in kwargs:
        if k not in ['num_workers', 'batch_size', 'zero_copy', 'backend', 'obs_stride', 'info_mode', 'env_offset', 'device']:
            raise APIUsageError(f'Invalid argument: {k}')

    return backend(env_creators, env_args, env_kwargs, num_envs, **kwargs)
