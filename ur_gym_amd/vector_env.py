"""Vectorised UR5e reach environments on one MI355X: the Gymnasium-VectorEnv-shaped surface of the HIP path.

Mirrors, batched over ``num_envs`` environments, the Env API of the reference's ``RobotTaskEnv``
(UR_gym/envs/core.py:222-320) as ``train.py:39-60`` / ``demo.py:6-17`` / ``model_test.py:27-49`` consume it:

    reset(seed=None, options=None) -> (obs_dict, info)                      core.py:263-273
    step(actions[N,6]) -> (obs_dict, reward[N], terminated[N], truncated[N], info)   core.py:303-317 + TimeLimit(100)

Host Python only holds the per-env state as PyTorch-ROCm tensors and launches the fused HIP kernels through the
C-ABI (include/urgym.h); every number is computed on the GPU.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, _native

try:  # gymnasium is optional (it is not installed in the build image)
    from gymnasium import spaces as _spaces

    Box, DictSpace = _spaces.Box, _spaces.Dict
except Exception:  # pragma: no cover - exercised when gymnasium is absent

    class Box:
        def __init__(self, low, high, shape, dtype=np.float32):
            self.low = np.full(shape, low, dtype=dtype)
            self.high = np.full(shape, high, dtype=dtype)
            self.shape, self.dtype = tuple(shape), np.dtype(dtype)

        def sample(self):
            return np.random.uniform(self.low, self.high).astype(self.dtype)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

        def __repr__(self):
            return f"Box({self.low.min()}, {self.high.max()}, {self.shape}, {self.dtype})"

    class DictSpace(dict):
        @property
        def spaces(self):
            return self

        def sample(self):
            return {k: v.sample() for k, v in self.items()}


_TORCH_DTYPE = {C.c_double: torch.float64, C.c_float: torch.float32, C.c_int32: torch.int32, C.c_uint8: torch.uint8}

# The training call's entry points (include/urgym.h), in the order ``sac_train`` tries them: (symbol, the option that selects it, the
# options it takes between ``learner, schedule`` and ``stream``, in the order of its signature).  The last row takes none.
_SAC_TRAIN_ENTRIES = (
    ("urgym_sac_train_tempered", "temper", ("planner", "temper", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_planned", "planner", ("planner", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_normalized", "normalizer", ("normalizer", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_clipped", "clipping", ("clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_hindsight", "hindsight", ("hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_prioritized", "prioritized", ("prioritized", "evaluation", "monitor")),
    ("urgym_sac_train_nstep", "nstep", ("nstep", "evaluation", "monitor")),
    ("urgym_sac_train_monitored", "monitor", ("evaluation", "monitor")),
    ("urgym_sac_train_evaluated", "evaluation", ("evaluation",)),
    ("urgym_sac_train", None, ()),
)

# The entry points ``sac_train`` tries ahead of that table, in the same form: a planner with coloured sampling noise
# goes to urgym_sac_train_colored whatever else is given; its temper struct, like every option after it, may be absent.  Ahead of that,
# behaviour cloning goes to urgym_sac_train_cloned, which takes every other option, each of which may be absent.
# Ahead of both, a demonstration ring goes to urgym_sac_train_demonstrated, which takes cloning and every other
# option but the three gathers' (each of those has a gather of its own).  Ahead of all three, the advantage weight on the cloning term
#  goes to urgym_sac_train_weighted, which needs cloning and takes every other option.
_SAC_TRAIN_ENTRIES_AHEAD = (
    ("urgym_sac_train_weighted", "weighting", ("weighting", "cloning", "demonstrating", "planner", "temper", "noise", "normalizer", "clipping", "nstep", "prioritized",
                                               "hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_demonstrated", "demonstrating", ("demonstrating", "cloning", "planner", "temper", "noise", "normalizer", "clipping", "evaluation", "monitor")),
    ("urgym_sac_train_cloned", "cloning", ("cloning", "planner", "temper", "noise", "normalizer", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
    ("urgym_sac_train_colored", "noise", ("planner", "noise", "temper", "clipping", "nstep", "prioritized", "hindsight", "evaluation", "monitor")),
)


def _sac_train_entry(present):
    """(symbol, option names) of the entry point that serves a call with the options in `present` (any container of names out of
    evaluation, monitor, nstep, prioritized, hindsight, clipping, normalizer, planner, temper -- the planner's temper struct, given where
    the planner has an ess_target -- noise, its noise struct, given where it has a noise_beta, cloning and demonstrating): the first row of
    ``_SAC_TRAIN_ENTRIES_AHEAD``, then of ``_SAC_TRAIN_ENTRIES``, whose option is given (weighting, too, is such a name)."""
    for symbol, selects, options in _SAC_TRAIN_ENTRIES_AHEAD + _SAC_TRAIN_ENTRIES:
        if selects is None or selects in present:
            return symbol, options


class UR5ReachVectorEnv:
    """N independent UR5{Ori,Obs,Dyn}Reach-v1 environments stepped by one fused kernel launch.

    Observations are returned as views of persistent device tensors (zero-copy); they are overwritten by the next
    ``step``/``reset``.  Pass ``copy_obs=True`` to get fresh tensors instead.
    """

    metadata = {"render_modes": []}

    def __init__(self, env_id="UR5DynReach-v1", num_envs=1, device="cuda:0", seed=0, auto_reset=True,
                 check_collision=True, copy_obs=False, **config_overrides):
        if env_id not in _abi.ENV_IDS:
            raise ValueError(f"unknown env id {env_id!r}; available: {sorted(_abi.ENV_IDS)}")
        self.lib = _native.lib()  # raises if the HIP extension is missing
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _native.NativeError("UR5ReachVectorEnv needs a ROCm GPU (torch device 'cuda:N'); there is no CPU path")
        self.env_id, self.env_kind = env_id, _abi.ENV_IDS[env_id]
        self.num_envs = int(num_envs)
        self.copy_obs = copy_obs
        self.obs_dim, self.goal_dim = _abi.OBS_DIMS[self.env_kind]
        self.cfg = _abi.Config()
        _native.check(self.lib.urgym_config_default(self.env_kind, self.num_envs, C.byref(self.cfg)))
        self.cfg.auto_reset = int(bool(auto_reset))
        self.cfg.check_collision = int(bool(check_collision))
        for k, v in config_overrides.items():
            if not hasattr(self.cfg, k):
                raise TypeError(f"unknown config field {k!r}")
            setattr(self.cfg, k, v)
        self._seed = int(seed)
        self._h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", dev_index)
        _native.check(self.lib.urgym_create(C.byref(self.cfg), dev_index, C.byref(self._h)))
        # all buffers are torch tensors owned here; the C side only borrows the pointers
        self.buf = {}
        cb = _abi.Buffers()
        for name, ct, shape in _abi.BUFFER_FIELDS:
            t = torch.zeros(shape(self.num_envs, self.obs_dim, self.goal_dim), dtype=_TORCH_DTYPE[ct], device=self.device)
            self.buf[name] = t
            setattr(cb, name, C.cast(t.data_ptr(), C.POINTER(ct)))
        self._cbuf = cb
        _native.check(self.lib.urgym_bind(self._h, C.byref(cb)), self._h)
        # spaces (core.py:241-248, UR5.py:251)
        self.single_observation_space = DictSpace(
            observation=Box(-10.0, 10.0, (self.obs_dim,), np.float32),
            achieved_goal=Box(-10.0, 10.0, (self.goal_dim,), np.float32),
            desired_goal=Box(-10.0, 10.0, (self.goal_dim,), np.float32),
        )
        self.single_action_space = Box(-1.0, 1.0, (6,), np.float32)
        self.observation_space = DictSpace(
            observation=Box(-10.0, 10.0, (self.num_envs, self.obs_dim), np.float32),
            achieved_goal=Box(-10.0, 10.0, (self.num_envs, self.goal_dim), np.float32),
            desired_goal=Box(-10.0, 10.0, (self.num_envs, self.goal_dim), np.float32),
        )
        self.action_space = Box(-1.0, 1.0, (self.num_envs, 6), np.float32)
        self._needs_reset = True

    # ------------------------------------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _obs(self):
        keys = ("observation", "achieved_goal", "desired_goal")
        if self.copy_obs:
            return {k: self.buf[k].clone() for k in keys}
        return {k: self.buf[k] for k in keys}

    def _mask_ptr(self, ids_or_mask):
        if ids_or_mask is None:
            return None, None
        m = torch.as_tensor(ids_or_mask, device=self.device)
        if m.dtype == torch.bool or (m.dtype == torch.uint8 and m.numel() == self.num_envs):
            mask = m.to(torch.uint8).contiguous()
        else:
            mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            mask[m.long()] = 1
        return mask, C.c_void_p(mask.data_ptr())

    # ------------------------------------------------------------------------------------------------ Env API
    def reset(self, seed=None, options=None, mask=None):
        """core.py:263-273 for every env (or the masked subset). ``seed`` re-keys the counter-based sampler."""
        if seed is not None:
            self._seed = int(seed)
            s = C.c_uint64(self._seed)
            if mask is None:
                # Gymnasium seeding contract: reset(seed=s) starts the SAME episodes every time.  The sampler is keyed by
                # (seed, env, episode id), so a seeded full reset rewinds the episode counters.
                self.buf["episode_id"].zero_()
        elif self._needs_reset:  # first reset, or the first one after SB3VecEnvAdapter.seed(): same rule
            s = C.c_uint64(self._seed)
            if mask is None:
                self.buf["episode_id"].zero_()
        else:
            s = C.c_uint64(_abi.KEEP_SEED)
        keep, mp = self._mask_ptr(mask)
        _native.check(self.lib.urgym_reset(self._h, mp, s, self._stream()), self._h)
        self._needs_reset = False
        info = {"is_success": self.buf["is_success"].bool()}
        return self._obs(), info

    def step(self, actions):
        """core.py:303-317 + TimeLimit; finished envs are auto-reset (their terminal observation is in
        info['final_observation'], valid where info['_final_observation'])."""
        if self._needs_reset:
            raise RuntimeError("call reset() before step()")
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = a.to(torch.float32).contiguous()
        if a.shape != (self.num_envs, 6):
            raise ValueError(f"actions must have shape ({self.num_envs}, 6), got {tuple(a.shape)}")
        _native.check(self.lib.urgym_step(self._h, C.c_void_p(a.data_ptr()), self._stream()), self._h)
        b = self.buf
        # the flag buffers hold 0 / 1 bytes: reinterpret them as bool instead of launching a conversion kernel per flag
        terminated, truncated = b["terminated"].view(torch.bool), b["truncated"].view(torch.bool)
        # status: the per-env URGYM_STATUS_* word (sticky): penetration depths consumed, joint limits passed, NaN, ... (include/urgym.h)
        info = {"is_success": b["is_success"].view(torch.bool), "collision": b["collision"].view(torch.bool), "status": b["status"]}
        if self.copy_obs:  # like the observations: private copies on request, zero-copy views of the live buffers otherwise
            terminated, truncated = terminated.clone(), truncated.clone()
            info = {k: v.clone() for k, v in info.items()}
        if self.cfg.auto_reset:
            if self.copy_obs:  # private copies: the mask is materialised now, it must not read the flags of a later step
                info["_final_observation"] = terminated | truncated
                info["final_observation"] = {"observation": b["final_observation"].clone(), "achieved_goal": b["final_achieved_goal"].clone(),
                                             "desired_goal": b["final_desired_goal"].clone()}
            else:
                # zero-copy mode: like the observations, these are views of live buffers, valid until the next step() / reset();
                # the mask is derived on first access (a kernel launch only if somebody looks) -- read it before stepping again
                info = _LazyInfo(info, {"_final_observation": lambda: terminated | truncated})
                info["final_observation"] = {"observation": b["final_observation"], "achieved_goal": b["final_achieved_goal"],
                                             "desired_goal": b["final_desired_goal"]}
        reward = b["reward"].clone() if self.copy_obs else b["reward"]
        return self._obs(), reward, terminated, truncated, info

    def rollout(self, actions):
        """K fused steps without returning to Python in between; ``actions`` is [K, N, 6] float32 on the device."""
        a = torch.as_tensor(actions, device=self.device, dtype=torch.float32).contiguous()
        if a.dim() != 3 or a.shape[1:] != (self.num_envs, 6):
            raise ValueError("actions must be [K, N, 6]")
        _native.check(self.lib.urgym_rollout(self._h, C.c_void_p(a.data_ptr()), int(a.shape[0]), self._stream()), self._h)

    # ------------------------------------------------------------------------------------------------ policy in the loop
    RECORD_KEYS = tuple(name for name, _, _ in _abi.TRAJECTORY_FIELDS)

    def _actor_ptr(self, actor):
        if getattr(actor, "env", None) is not self or not getattr(actor, "_a", None):
            raise ValueError("actor must be a live DeviceActor loaded for this environment (DeviceActor.load(npz, env))")
        return actor._a

    SAMPLE_RECORD_KEYS = tuple(name for name, _, _ in _abi.SAMPLE_RECORD_FIELDS)

    @staticmethod
    def _sampling(sample):
        """`sample`: a dict or object with ``mode`` ("mean" | "gaussian" | "uniform", or the URGYM_SAMPLE_* number), ``seed`` and
        ``first_draw`` (both default 0) -> _abi.Sampling."""
        get = sample.get if isinstance(sample, dict) else lambda k, d=None: getattr(sample, k, d)
        mode = get("mode", "gaussian")
        if isinstance(mode, str):
            if mode not in _abi.SAMPLE_MODES:
                raise ValueError(f"unknown sampling mode {mode!r}; available: {sorted(_abi.SAMPLE_MODES)}")
            mode = _abi.SAMPLE_MODES[mode]
        return _abi.Sampling(int(mode), 0, int(get("seed", 0) or 0), int(get("first_draw", 0) or 0))

    ROW_KEYS = ("observation", "achieved_goal", "desired_goal")

    def _rows(self, rows, action=None):
        """`rows` (see ``critic_values``) -> (_abi.CriticRows, leading shape, the tensors to keep alive).  None = the bound buffers."""
        dims = dict(observation=self.obs_dim, achieved_goal=self.goal_dim, desired_goal=self.goal_dim, action=6)
        given = {}
        if rows is not None:
            given = dict(zip(self.ROW_KEYS, rows)) if isinstance(rows, (tuple, list)) else {k: rows[k] for k in self.ROW_KEYS if k in rows}
            if set(given) != set(self.ROW_KEYS):
                raise ValueError(f"rows must give {self.ROW_KEYS} (the dict rollout_policy returns with these records, or a tuple in this order)")
        if action is not None:
            given["action"] = action
        lead, keep, cr = None, [], _abi.CriticRows()
        for name, t in given.items():
            t = torch.as_tensor(t, device=self.device)
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            if t.dim() not in (2, 3) or t.shape[-1] != dims[name]:
                raise ValueError(f"{name} must be [M, {dims[name]}] or [K, N, {dims[name]}], got {tuple(t.shape)}")
            if lead is None:
                lead = tuple(t.shape[:-1])
            elif tuple(t.shape[:-1]) != lead:
                raise ValueError(f"{name} has leading shape {tuple(t.shape[:-1])}, the others {lead}")
            keep.append(t)
            setattr(cr, name, C.cast(t.data_ptr(), C.POINTER(C.c_float)))
        if rows is None:
            if lead is None:
                lead = (self.num_envs,)
            elif lead != (self.num_envs,):
                raise ValueError(f"without rows the bound buffers are read: actions must be [{self.num_envs}, 6], got leading shape {lead}")
        return cr, lead, keep

    def critic_values(self, critic, actions, rows=None, reward=None, terminated=None, log_prob=None, gamma=None, ent_coef=0.0):
        """Both Q-networks of `critic` (a DeviceCritic of this environment) on (rows, actions), one launch of the HIP critic kernel:
        returns a dict of fresh device tensors ``q`` [2, ...], ``q_min`` [...] = min(q0, q1) and, when `reward` is given,
        ``target`` [...] = reward + gamma (1 - terminated) (q_min - ent_coef log_prob) -- SAC's y, with `actions` = a' drawn on the
        next observations (``policy_actions(..., rows=)``) and `log_prob` theirs; without `log_prob` the entropy term is absent.

        `rows`: None = the live observation buffers ([N] rows); or the dict ``rollout_policy`` returns (its ``observation``,
        ``achieved_goal``, ``desired_goal`` records), or a tuple of tensors in that order, with leading shape [K, N] or [M] -- all
        K N rows go into one launch.  `actions`, `reward`, `terminated`, `log_prob` have the same leading shape.  Nothing is
        synchronised: the tensors are valid in stream order."""
        if getattr(critic, "env", None) is not self or not getattr(critic, "_c", None):
            raise ValueError("critic must be a live DeviceCritic loaded for this environment (DeviceCritic.load(paths, env))")
        cr, lead, keep = self._rows(rows, action=actions)
        count = int(np.prod(lead))
        terms = _abi.CriticTerms()
        if reward is not None:
            if gamma is None:
                raise ValueError("the target needs gamma (tests/golden/critics/sac_hyperparameters.json has the checkpoints': 0.95)")
            terms.gamma, terms.ent_coef = float(gamma), float(ent_coef)
            for name, t, dt, ct in (("reward", reward, torch.float32, C.c_float), ("terminated", terminated, torch.uint8, C.c_uint8),
                                    ("log_prob", log_prob, torch.float32, C.c_float)):
                if t is None:
                    continue
                t = torch.as_tensor(t, device=self.device)
                t = t.view(torch.uint8) if t.dtype == torch.bool else t
                if t.dtype != dt or not t.is_contiguous():
                    t = t.to(dt).contiguous()
                if tuple(t.shape) != lead:
                    raise ValueError(f"{name} must have shape {lead}, got {tuple(t.shape)}")
                keep.append(t)
                setattr(terms, name, C.cast(t.data_ptr(), C.POINTER(ct)))
        elif terminated is not None or log_prob is not None:
            raise ValueError("terminated / log_prob are terms of the target, which needs reward")
        res = {"q": torch.empty((2,) + lead, dtype=torch.float32, device=self.device),
               "q_min": torch.empty(lead, dtype=torch.float32, device=self.device)}
        if reward is not None:
            res["target"] = torch.empty(lead, dtype=torch.float32, device=self.device)
        out = _abi.CriticOut(*[C.cast(res[k].data_ptr(), C.POINTER(C.c_float)) if k in res else None for k in ("q", "q_min", "target")])
        _native.check(self.lib.urgym_critic_evaluate(self._h, critic._c, C.byref(cr), count, C.byref(terms), C.byref(out), self._stream()), self._h)
        return res

    def critic_action_gradient(self, critic, actions, rows=None):
        """The gradient of both Q-networks of `critic` with respect to `actions`, one launch of the HIP gradient kernel
        (urgym_critic_action_gradient): a dict of fresh device tensors ``dq_da`` [2, ..., 6], ``dqmin_da`` [..., 6] = the gradient of
        min(q0, q1) (of qf0 on a tie), and ``q`` [2, ...], ``q_min`` [...] as ``critic_values`` gives them, bitwise.  `rows` and the
        leading shapes are ``critic_values``'; nothing is synchronised."""
        if getattr(critic, "env", None) is not self or not getattr(critic, "_c", None):
            raise ValueError("critic must be a live DeviceCritic loaded for this environment (DeviceCritic.load(paths, env))")
        cr, lead, keep = self._rows(rows, action=actions)
        count = int(np.prod(lead))
        res = {"dq_da": torch.empty((2,) + lead + (6,), dtype=torch.float32, device=self.device),
               "dqmin_da": torch.empty(lead + (6,), dtype=torch.float32, device=self.device),
               "q": torch.empty((2,) + lead, dtype=torch.float32, device=self.device),
               "q_min": torch.empty(lead, dtype=torch.float32, device=self.device)}
        out = _abi.CriticGradOut(*[C.cast(res[k].data_ptr(), C.POINTER(C.c_float)) for k in ("dq_da", "dqmin_da", "q", "q_min")])
        _native.check(self.lib.urgym_critic_action_gradient(self._h, critic._c, C.byref(cr), count, C.byref(out), self._stream()), self._h)
        return res

    def critic_gradient_workspace(self, critic, count):
        """A fresh workspace for ``critic_parameter_gradients`` on `count` rows: a float32 device tensor of the size the library reports."""
        size = C.c_uint64()
        _native.check(self.lib.urgym_critic_parameter_gradients_workspace(self._h, critic._c, int(count), C.byref(size)), self._h)
        return torch.empty(((size.value + 3) // 4,), dtype=torch.float32, device=self.device)

    def critic_parameter_gradients(self, critic, actions, *, dq=None, target=None, scale=None, rows=None, out=None, workspace=None):
        """The gradients of a loss on both Q-networks of `critic` with respect to their parameters, summed over the rows
        (urgym_critic_parameter_gradients: two launches up to 1024 rows, three above).  The upstream gradient d loss / d q is either
        `dq` [2, ...] or ``(q - target) * scale`` with `target` [...] and the call's own q (``scale = 1 / rows`` gives SB3's critic
        loss).  Returns a dict: ``grads``, a list of two dicts keyed by CRITIC_ARRAYS (tensors shaped like the parameters, so a
        parameter's ``.grad`` can be handed in through `out`, a list of two such dicts), and ``q`` [2, ...].  `workspace`: a float32 device tensor from
        ``critic_gradient_workspace`` (allocated where not given).  `rows` and the leading shapes are ``critic_values``'; nothing is
        synchronised, and the sums have a fixed order: two calls give the same bits."""
        from .evaluation import CRITIC_ARRAYS

        if getattr(critic, "env", None) is not self or not getattr(critic, "_c", None):
            raise ValueError("critic must be a live DeviceCritic loaded for this environment (DeviceCritic.load(paths, env))")
        if (dq is None) == (target is None):
            raise ValueError("exactly one of dq and target must be given")
        if target is not None and scale is None:
            raise ValueError("target needs scale (1 / rows for the mean squared error of SB3's critic loss)")
        cr, lead, keep = self._rows(rows, action=actions)
        count = int(np.prod(lead))
        up = torch.as_tensor(dq if dq is not None else target, device=self.device)
        if up.dtype != torch.float32 or not up.is_contiguous():
            up = up.to(torch.float32).contiguous()
        want = ((2,) + lead) if dq is not None else lead
        if tuple(up.shape) != want:
            raise ValueError(f"{'dq' if dq is not None else 'target'} must have shape {want}, got {tuple(up.shape)}")
        n, H = critic.in_features, critic.hidden_width
        shapes = dict(zip(CRITIC_ARRAYS, ((H, n), (H,), (H, H), (H,), (1, H), (1,))))
        if out is None:
            out = [{k: torch.empty(sh, dtype=torch.float32, device=self.device) for k, sh in shapes.items()} for _ in range(2)]
        grads = _abi.CriticParamGrads()
        for i, w in enumerate(out):
            for k in CRITIC_ARRAYS:
                t = w[k]
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != torch.device(self.device) or tuple(t.shape) != shapes[k]:
                    raise ValueError(f"out[{i}][{k!r}] must be a contiguous float32 tensor of shape {shapes[k]} on {self.device}")
            grads.qf[i] = _abi.QNetworkGrad(*[C.cast(w[k].data_ptr(), C.POINTER(C.c_float)) for k in CRITIC_ARRAYS])
        q = torch.empty((2,) + lead, dtype=torch.float32, device=self.device)
        grads.q = C.cast(q.data_ptr(), C.POINTER(C.c_float))
        if workspace is None:
            workspace = self.critic_gradient_workspace(critic, count)
        if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != torch.device(self.device):
            raise ValueError(f"workspace must be a contiguous float32 tensor on {self.device} (critic_gradient_workspace)")
        ptr = C.c_void_p(up.data_ptr())
        _native.check(self.lib.urgym_critic_parameter_gradients(self._h, critic._c, C.byref(cr), count, ptr if dq is not None else None,
                                                                None if dq is not None else ptr, float(scale or 0.0), C.byref(grads),
                                                                C.c_void_p(workspace.data_ptr()), workspace.numel() * 4, self._stream()), self._h)
        return {"grads": out, "q": q}

    def actor_gradient_workspace(self, actor, count):
        """A fresh workspace for ``actor_parameter_gradients`` on `count` rows: a float32 device tensor of the size the library reports."""
        size = C.c_uint64()
        _native.check(self.lib.urgym_actor_parameter_gradients_workspace(self._h, self._actor_ptr(actor), int(count), C.byref(size)), self._h)
        return torch.empty(((size.value + 3) // 4,), dtype=torch.float32, device=self.device)

    ACTOR_GRADIENT_RECORDS = _abi.ACTOR_GRAD_RECORDS[2:]  # besides action and log_prob, which are always returned

    def actor_parameter_gradients(self, actor, *, sample, rows=None, d_action=None, d_log_prob=None, d_mu=None, d_log_std=None, out=None,
                                  workspace=None, records=()):
        """The gradients of a loss on `actor` (a DeviceActor with its log_std head) with respect to its parameters, summed over the rows
        (urgym_actor_parameter_gradients: two launches up to 1024 rows, three above).  `sample` as in ``policy_actions`` (mode
        "gaussian" or "mean"); `rows` as in ``critic_values`` (None = the live buffers).  The upstream gradient is either `d_action`
        [..., 6] with `d_log_prob` [...] or None (= 0) -- the gradient with respect to the call's own action and log_prob, the noise a
        constant -- or `d_mu` and `d_log_std` [..., 6] each, the gradient at the heads, used as it is.  Returns a dict: ``grads``, keyed
        by ACTOR_ARRAYS + LOG_STD_ARRAYS and shaped like the parameters (a parameter's ``.grad`` can be handed in through `out`, such
        a dict); ``action`` [..., 6] and ``log_prob`` [...], bitwise ``policy_actions(..., sample=, rows=)``'s; and those of
        ACTOR_GRADIENT_RECORDS that `records` names (``noise``, ``log_std`` after the clamp, ``d_mu``, ``d_log_std`` before the clamp
        derivative, ``std`` = exp(log_std) as the forward pass formed it).  `workspace`: from ``actor_gradient_workspace`` (allocated where not given).  Nothing is synchronised, and the
        sums have a fixed order: two calls give the same bits."""
        from .evaluation import ACTOR_ARRAYS, LOG_STD_ARRAYS

        a = self._actor_ptr(actor)
        keys = ACTOR_ARRAYS + LOG_STD_ARRAYS
        sample_form, heads_form = d_action is not None or d_log_prob is not None, d_mu is not None or d_log_std is not None
        if sample_form == heads_form or (sample_form and d_action is None) or (heads_form and (d_mu is None or d_log_std is None)):
            raise ValueError("exactly one upstream form must be given: d_action (with d_log_prob or None), or both d_mu and d_log_std")
        unknown = [k for k in records if k not in self.ACTOR_GRADIENT_RECORDS]
        if unknown:
            raise ValueError(f"unknown records {unknown}; available: {self.ACTOR_GRADIENT_RECORDS}")
        cr, lead, keep = self._rows(rows)
        count = int(np.prod(lead))
        up = _abi.ActorUpstream()
        for name, t, shape in (("d_action", d_action, lead + (6,)), ("d_log_prob", d_log_prob, lead), ("d_mu", d_mu, lead + (6,)), ("d_log_std", d_log_std, lead + (6,))):
            if t is None:
                continue
            t = torch.as_tensor(t, device=self.device)
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
            keep.append(t)
            setattr(up, name, C.cast(t.data_ptr(), C.POINTER(C.c_float)))
        n, H = actor.in_features, actor.hidden_width
        shapes = dict(zip(keys, ((H, n), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))
        if out is None:
            out = {k: torch.empty(sh, dtype=torch.float32, device=self.device) for k, sh in shapes.items()}
        grads = _abi.ActorParamGrads()
        for field, k in zip(_abi.ACTOR_GRAD_ARRAYS, keys):
            t = out[k]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != torch.device(self.device) or tuple(t.shape) != shapes[k]:
                raise ValueError(f"out[{k!r}] must be a contiguous float32 tensor of shape {shapes[k]} on {self.device}")
            setattr(grads, field, C.cast(t.data_ptr(), C.POINTER(C.c_float)))
        res = {"grads": out, "action": torch.empty(lead + (6,), dtype=torch.float32, device=self.device),
               "log_prob": torch.empty(lead, dtype=torch.float32, device=self.device)}
        for k in records:
            res[k] = torch.empty(lead + (6,), dtype=torch.float32, device=self.device)
        for k in ("action", "log_prob") + tuple(records):
            setattr(grads, k, C.cast(res[k].data_ptr(), C.POINTER(C.c_float)))
        if workspace is None:
            workspace = self.actor_gradient_workspace(actor, count)
        if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != torch.device(self.device):
            raise ValueError(f"workspace must be a contiguous float32 tensor on {self.device} (actor_gradient_workspace)")
        how = self._sampling(sample)
        _native.check(self.lib.urgym_actor_parameter_gradients(self._h, a, C.byref(how), C.byref(cr), count, C.byref(up), C.byref(grads),
                                                               C.c_void_p(workspace.data_ptr()), workspace.numel() * 4, self._stream()), self._h)
        return res

    @staticmethod
    def _adam_hyper(lr, betas, eps, step):
        betas = tuple(betas)
        if len(betas) != 2:
            raise ValueError(f"betas must be a pair, got {betas}")
        return _abi.AdamHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), int(step), 0)

    def _grad_norm_args(self, who, max_norm, tensors, norm_out, scale_out, tensor_sums_out):
        """The ``_abi.GradNorm`` of a norm call and the dict it returns: outputs not handed in are allocated (not synchronised);
        ``tensor_sums_out=False`` asks for no per-tensor sums (a NULL pointer: the kernel then writes none)."""
        max_norm = float(max_norm)
        if not (self._finite32(max_norm) and max_norm > 0.0):
            raise ValueError(f"{who}: max_norm must be finite and positive, got {max_norm}")
        out = dict(norm=norm_out if norm_out is not None else torch.empty((1,), dtype=torch.float32, device=self.device),
                   scale=scale_out if scale_out is not None else torch.empty((1,), dtype=torch.float32, device=self.device),
                   tensor_sums=tensor_sums_out if tensor_sums_out is not None else torch.empty((tensors,), dtype=torch.float64, device=self.device))
        sums = None
        if tensor_sums_out is False:
            del out["tensor_sums"]
        else:
            sums = self._float_ptr(who, "tensor_sums_out", out["tensor_sums"], (tensors,), torch.float64, C.c_double)
        args = _abi.GradNorm(max_norm, 0, self._float_ptr(who, "norm_out", out["norm"], (1,)), self._float_ptr(who, "scale_out", out["scale"], (1,)), sums)
        return args, out

    def actor_gradient_norm(self, actor, grads, max_norm, *, norm_out=None, scale_out=None, tensor_sums_out=None):
        """The global norm of the actor's eight gradient tensors and the clip coefficient, on the device in ONE launch of one workgroup
        (urgym_actor_grad_norm): `grads` as ``actor_adam_step`` takes them, only read.  Returns ``dict(norm=, scale=, tensor_sums=)``:
        float32 [1], float32 [1] and float64 [8] tensors, the ones handed in (`norm_out`, `scale_out`, `tensor_sums_out`) or new ones;
        ``tensor_sums_out=False`` leaves the sums out (what the training call does).
        ``scale`` is what ``actor_adam_step(scale=)`` takes.  The arithmetic is ``evaluation.grad_norm``, bitwise.  On torch's current
        stream, nothing is synchronised."""
        from .evaluation import ACTOR_ARRAYS, LOG_STD_ARRAYS, DeviceActor

        who = "actor_gradient_norm"
        a = self._actor_ptr(actor)
        grads = dict(grads)
        if not DeviceActor.check_parameters(grads, actor.in_features, actor.hidden_width, self.device):
            raise ValueError(f"{who}: grads needs the log_std head too ({LOG_STD_ARRAYS})")
        g = _abi.ActorTensors(*[C.cast(grads[k].data_ptr(), C.POINTER(C.c_float)) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS])
        args, out = self._grad_norm_args(who, max_norm, _abi.GRAD_NORM_ACTOR_TENSORS, norm_out, scale_out, tensor_sums_out)
        _native.check(self.lib.urgym_actor_grad_norm(self._h, a, C.byref(g), C.byref(args), self._stream()), self._h)
        return out

    def critic_gradient_norm(self, critic, grads, max_norm, *, norm_out=None, scale_out=None, tensor_sums_out=None):
        """``actor_gradient_norm`` for the twelve gradient tensors of both Q-networks, ONE group (urgym_critic_grad_norm): `grads` as
        ``critic_adam_step`` takes them; ``tensor_sums`` is float64 [12], network 0 first."""
        from .evaluation import CRITIC_ARRAYS, DeviceCritic

        who = "critic_gradient_norm"
        if getattr(critic, "env", None) is not self or not getattr(critic, "_c", None):
            raise ValueError(f"{who}: critic must be a live DeviceCritic loaded for this environment (DeviceCritic.load(paths, env))")
        grads = [dict(w) for w in grads]
        DeviceCritic.check_parameters(grads, critic.in_features, critic.hidden_width, self.device)
        g = (_abi.QNetworkDev * 2)(*[_abi.QNetworkDev(*[C.cast(w[k].data_ptr(), C.POINTER(C.c_float)) for k in CRITIC_ARRAYS]) for w in grads])
        args, out = self._grad_norm_args(who, max_norm, _abi.GRAD_NORM_CRITIC_TENSORS, norm_out, scale_out, tensor_sums_out)
        _native.check(self.lib.urgym_critic_grad_norm(self._h, critic._c, g, C.byref(args), self._stream()), self._h)
        return out

    def actor_adam_step(self, actor, params, grads, exp_avg, exp_avg_sq, *, lr, betas=(0.9, 0.999), eps=1e-8, step, scale=None):
        """One Adam step of `actor`'s parameters on the device, and the reload, in ONE launch (urgym_actor_adam_step): `params`,
        `exp_avg` and `exp_avg_sq` are updated in place from `grads`, and the DeviceActor's packed buffer is rewritten from the stepped
        parameters, the log_std head included -- ``torch.optim.Adam.step()`` followed by ``actor.load_parameters(params)``.  The four
        are dicts under ACTOR_ARRAYS + LOG_STD_ARRAYS (all eight tensors) as ``DeviceActor.check_parameters`` takes them; no two of
        the 32 tensors may overlap (not checked).  `step` is the 1-based index of this step: the caller counts, the library keeps no
        optimiser state.  The arithmetic is ``evaluation.adam_step`` with ``evaluation.adam_coefficients``, bitwise.  On torch's
        current stream, nothing is synchronised; stream order as for ``DeviceActor.load_parameters``.  With `scale` (a float32 [1]
        tensor on this device: ``actor_gradient_norm(...)["scale"]``) the call is urgym_actor_adam_step_scaled: every gradient element is
        multiplied by it as it is read (``evaluation.adam_step(scale=)``); `grads` is not written.  ``None`` makes exactly the call above."""
        from .evaluation import ACTOR_ARRAYS, LOG_STD_ARRAYS, DeviceActor

        a = self._actor_ptr(actor)
        keys = ACTOR_ARRAYS + LOG_STD_ARRAYS
        t = _abi.ActorAdam(actor.in_features, actor.hidden_width, 0)
        for name, tensors in zip(_abi.ADAM_SETS, (params, grads, exp_avg, exp_avg_sq)):
            tensors = dict(tensors)
            if not DeviceActor.check_parameters(tensors, actor.in_features, actor.hidden_width, self.device):
                raise ValueError(f"actor_adam_step: {name} needs the log_std head too ({LOG_STD_ARRAYS})")
            setattr(t, name, _abi.ActorTensors(*[C.cast(tensors[k].data_ptr(), C.POINTER(C.c_float)) for k in keys]))
        hp = self._adam_hyper(lr, betas, eps, step)
        if scale is None:
            _native.check(self.lib.urgym_actor_adam_step(self._h, a, C.byref(t), C.byref(hp), self._stream()), self._h)
        else:
            sc = self._float_ptr("actor_adam_step", "scale", scale, (1,))
            _native.check(self.lib.urgym_actor_adam_step_scaled(self._h, a, C.byref(t), C.byref(hp), C.cast(sc, C.c_void_p), self._stream()), self._h)
        actor.has_log_std = True

    def critic_adam_step(self, online, params, grads, exp_avg, exp_avg_sq, *, lr, betas=(0.9, 0.999), eps=1e-8, step, target=None, tau=None,
                         scale=None):
        """One Adam step of both Q-networks on the device, the reload of `online` and, with `target`, its Polyak update, in ONE launch
        (urgym_critic_adam_step): ``torch.optim.Adam.step()`` followed by ``online.load_parameters(params, tau=1)`` and
        ``target.load_parameters(params, tau)``.  The four are lists of two dicts under CRITIC_ARRAYS as
        ``DeviceCritic.check_parameters`` takes them; no two of the 48 tensors may overlap (not checked).  `target`: another
        DeviceCritic of this environment with `online`'s shape, blended as ``evaluation.polyak`` states with `tau` in (0, 1].
        `step`, the arithmetic, the stream and the ordering as in ``actor_adam_step``; `scale` likewise
        (``critic_gradient_norm(...)["scale"]``: urgym_critic_adam_step_scaled), ``None`` makes exactly the call above."""
        from .evaluation import CRITIC_ARRAYS, DeviceCritic

        for who, c in (("online", online), ("target", target)):
            if c is None and who == "target":
                continue
            if getattr(c, "env", None) is not self or not getattr(c, "_c", None):
                raise ValueError(f"{who} must be a live DeviceCritic loaded for this environment (DeviceCritic.load(paths, env))")
        if target is not None:
            if tau is None:
                raise ValueError("a target needs tau (tests/golden/critics/sac_hyperparameters.json has the checkpoints': 0.005)")
            tau = float(tau)
            if not (np.isfinite(tau) and 0.0 < tau <= 1.0):
                raise ValueError(f"tau must be in (0, 1], got {tau}")
        t = _abi.CriticAdam(online.in_features, online.hidden_width, 0)
        for name, tensors in zip(_abi.ADAM_SETS, (params, grads, exp_avg, exp_avg_sq)):
            tensors = [dict(w) for w in tensors]
            DeviceCritic.check_parameters(tensors, online.in_features, online.hidden_width, self.device)
            nets = getattr(t, name)
            for i, w in enumerate(tensors):
                nets[i] = _abi.QNetworkDev(*[C.cast(w[k].data_ptr(), C.POINTER(C.c_float)) for k in CRITIC_ARRAYS])
        hp = self._adam_hyper(lr, betas, eps, step)
        if scale is None:
            _native.check(self.lib.urgym_critic_adam_step(self._h, online._c, target._c if target is not None else None, C.byref(t), C.byref(hp),
                                                          float(tau) if target is not None else 1.0, self._stream()), self._h)
        else:
            sc = self._float_ptr("critic_adam_step", "scale", scale, (1,))
            _native.check(self.lib.urgym_critic_adam_step_scaled(self._h, online._c, target._c if target is not None else None, C.byref(t), C.byref(hp),
                                                                 float(tau) if target is not None else 1.0, C.cast(sc, C.c_void_p), self._stream()), self._h)

    def _float_ptr(self, who, name, t, shape, dtype=torch.float32, ctype=C.c_float):
        """The DEVICE pointer of `t` for a call that reads or writes it in place: a contiguous `dtype` tensor of `shape` on this
        device (a bool tensor counts as uint8), or ValueError.  Nothing is converted or copied."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a torch tensor on {self.device}, got {type(t).__name__}")
        have = torch.uint8 if t.dtype == torch.bool and dtype == torch.uint8 else t.dtype
        if have != dtype or not t.is_contiguous() or t.device != torch.device(self.device) or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")
        return C.cast(t.data_ptr(), C.POINTER(ctype))

    @staticmethod
    def _finite32(x):
        with np.errstate(over="ignore"):
            return bool(np.isfinite(np.float32(x)))

    def entropy_step(self, state, log_prob, target_entropy, *, lr, betas=(0.9, 0.999), eps=1e-8, step, ent_coef_out, loss_out=None,
                     target=None, next_log_prob=None, terminated=None, gamma=None, y_out=None, d_log_prob_out=None, scale=None):
        """SB3's ``ent_coef_optimizer`` step on the device plus every per-row use of alpha that is ready then, in ONE launch
        (urgym_sac_entropy_step).  `state`: the three float32 [1] tensors (log_ent_coef, exp_avg, exp_avg_sq), as a tuple or a dict
        under those names, stepped in place on the mean of ``log_prob + target_entropy`` over `log_prob` [count]; `step` is the 1-based
        index of this step (the caller counts).  ``ent_coef_out`` [1] receives alpha = exp(log_ent_coef) of the value BEFORE the
        step, ``loss_out`` [1] the temperature loss.  The target group, whole or absent: `target`, `next_log_prob`, `y_out` [count],
        `gamma`, and `terminated` (bool or uint8 [count]) or None: ``y_out = target - ((gamma (1 - terminated)) alpha)
        next_log_prob``; `y_out` may be `target` itself.  The upstream group: ``d_log_prob_out`` [count] = alpha * `scale`.  Every
        tensor is checked (float32, contiguous, this device, its shape), none is converted.  The arithmetic is
        ``evaluation.entropy_step``, bitwise.  On torch's current stream, nothing is synchronised."""
        who = "entropy_step"
        names = ("log_ent_coef", "exp_avg", "exp_avg_sq")
        state = tuple(state[k] for k in names) if isinstance(state, dict) else tuple(state)
        if len(state) != 3:
            raise ValueError(f"{who}: state must be the three tensors {names}")
        if not isinstance(log_prob, torch.Tensor) or log_prob.dim() != 1:
            raise ValueError(f"{who}: log_prob must be a float32 [count] tensor")
        count = int(log_prob.shape[0])
        if not 1 <= count <= _abi.SAC_TERMS_MAX_COUNT:
            raise ValueError(f"{who}: count must be in [1, {_abi.SAC_TERMS_MAX_COUNT}], got {count}")
        group = (target is not None, next_log_prob is not None, y_out is not None, gamma is not None)
        if any(group) != all(group) or (terminated is not None and not all(group)):
            raise ValueError(f"{who}: the target group is half given: target, next_log_prob, y_out and gamma go together (terminated only with them)")
        if (d_log_prob_out is None) != (scale is None):
            raise ValueError(f"{who}: the upstream group is half given: d_log_prob_out and scale go together")
        for name, x in (("target_entropy", target_entropy), ("gamma", gamma), ("scale", scale)):
            if x is not None and not self._finite32(x):
                raise ValueError(f"{who}: {name} must be finite in float32, got {x}")
        a = _abi.SacEntropyArgs(count, 0, float(target_entropy), float(gamma or 0.0), float(scale or 0.0))
        a.log_prob = self._float_ptr(who, "log_prob", log_prob, (count,))
        for name, t in zip(names, state):
            setattr(a, name, self._float_ptr(who, name, t, (1,)))
        a.ent_coef_out = self._float_ptr(who, "ent_coef_out", ent_coef_out, (1,))
        if loss_out is not None:
            a.loss_out = self._float_ptr(who, "loss_out", loss_out, (1,))
        if all(group):
            a.target_in = self._float_ptr(who, "target", target, (count,))
            a.next_log_prob = self._float_ptr(who, "next_log_prob", next_log_prob, (count,))
            a.y_out = self._float_ptr(who, "y_out", y_out, (count,))
            if terminated is not None:
                a.terminated = self._float_ptr(who, "terminated", terminated, (count,), torch.uint8, C.c_uint8)
        if d_log_prob_out is not None:
            a.d_log_prob_out = self._float_ptr(who, "d_log_prob_out", d_log_prob_out, (count,))
        hp = self._adam_hyper(lr, betas, eps, step)
        _native.check(self.lib.urgym_sac_entropy_step(self._h, C.byref(a), C.byref(hp), self._stream()), self._h)

    def entropy_step_nstep(self, state, log_prob, target_entropy, *, lr, betas=(0.9, 0.999), eps=1e-8, step, ent_coef_out, loss_out=None,
                           reward=None, q_min_next=None, discount=None, next_log_prob=None, terminated=None, y_out=None,
                           d_log_prob_out=None, scale=None):
        """``entropy_step`` with the target group of a multi-step return, in ONE launch (urgym_sac_entropy_step_nstep): `reward`
        (the return R), `q_min_next` (min_i Q_i'(s', a')), `discount` (gamma^m), `next_log_prob` and `y_out`, [count] each and given
        together, and `terminated` or None: ``y_out = (reward + (discount (1 - terminated)) q_min_next) - ((discount (1 -
        terminated)) alpha) next_log_prob``; `y_out` may be `reward` itself.  Everything else as in ``entropy_step``.  The arithmetic
        is ``evaluation.entropy_step_nstep``, bitwise.  On torch's current stream, nothing is synchronised."""
        who = "entropy_step_nstep"
        names = ("log_ent_coef", "exp_avg", "exp_avg_sq")
        state = tuple(state[k] for k in names) if isinstance(state, dict) else tuple(state)
        if len(state) != 3:
            raise ValueError(f"{who}: state must be the three tensors {names}")
        if not isinstance(log_prob, torch.Tensor) or log_prob.dim() != 1:
            raise ValueError(f"{who}: log_prob must be a float32 [count] tensor")
        count = int(log_prob.shape[0])
        if not 1 <= count <= _abi.SAC_TERMS_MAX_COUNT:
            raise ValueError(f"{who}: count must be in [1, {_abi.SAC_TERMS_MAX_COUNT}], got {count}")
        group = {"reward": reward, "q_min_next": q_min_next, "discount": discount, "next_log_prob": next_log_prob, "y_out": y_out}
        given = [x is not None for x in group.values()]
        if any(given) != all(given) or (terminated is not None and not all(given)):
            raise ValueError(f"{who}: the target group is half given: {', '.join(group)} go together (terminated only with them)")
        if (d_log_prob_out is None) != (scale is None):
            raise ValueError(f"{who}: the upstream group is half given: d_log_prob_out and scale go together")
        for name, x in (("target_entropy", target_entropy), ("scale", scale)):
            if x is not None and not self._finite32(x):
                raise ValueError(f"{who}: {name} must be finite in float32, got {x}")
        a = _abi.SacEntropyNstepArgs(count, 0, float(target_entropy), float(scale or 0.0))
        a.log_prob = self._float_ptr(who, "log_prob", log_prob, (count,))
        for name, t in zip(names, state):
            setattr(a, name, self._float_ptr(who, name, t, (1,)))
        a.ent_coef_out = self._float_ptr(who, "ent_coef_out", ent_coef_out, (1,))
        if loss_out is not None:
            a.loss_out = self._float_ptr(who, "loss_out", loss_out, (1,))
        if all(given):
            for name, t in group.items():
                setattr(a, name, self._float_ptr(who, name, t, (count,)))
            if terminated is not None:
                a.terminated = self._float_ptr(who, "terminated", terminated, (count,), torch.uint8, C.c_uint8)
        if d_log_prob_out is not None:
            a.d_log_prob_out = self._float_ptr(who, "d_log_prob_out", d_log_prob_out, (count,))
        hp = self._adam_hyper(lr, betas, eps, step)
        _native.check(self.lib.urgym_sac_entropy_step_nstep(self._h, C.byref(a), C.byref(hp), self._stream()), self._h)

    def policy_terms(self, ent_coef, count, *, dqmin_da=None, scale=None, d_action_out=None, q=None, y=None, critic_loss_out=None,
                     log_prob=None, q_min=None, actor_loss_out=None):
        """What a SAC update forms after the critic's step and the action gradient, in ONE launch (urgym_sac_policy_terms).
        `ent_coef` [1]: what ``entropy_step`` wrote to ``ent_coef_out``.  Three groups, each whole or absent, at least one:
        (`dqmin_da`, `d_action_out` [count, 6], `scale`) writes ``d_action_out = dqmin_da * scale``; (`q` [2, count], `y` [count],
        `critic_loss_out` [1]) the critic loss ``0.5 (mean (q0 - y)^2 + mean (q1 - y)^2)``; (`log_prob`, `q_min` [count],
        `actor_loss_out` [1]) the actor loss ``mean(ent_coef log_prob - q_min)``.  Tensors are checked as in ``entropy_step``; the
        arithmetic is ``evaluation.policy_terms``, bitwise.  On torch's current stream, nothing is synchronised."""
        who = "policy_terms"
        count = int(count)
        if not 1 <= count <= _abi.SAC_TERMS_MAX_COUNT:
            raise ValueError(f"{who}: count must be in [1, {_abi.SAC_TERMS_MAX_COUNT}], got {count}")
        groups = {"upstream": (dqmin_da, d_action_out, scale), "critic loss": (q, y, critic_loss_out), "actor loss": (log_prob, q_min, actor_loss_out)}
        for name, g in groups.items():
            if any(x is not None for x in g) != all(x is not None for x in g):
                raise ValueError(f"{who}: the {name} group is half given")
        if all(g[0] is None for g in groups.values()):
            raise ValueError(f"{who}: no group is given (upstream, critic loss, actor loss)")
        if scale is not None and not self._finite32(scale):
            raise ValueError(f"{who}: scale must be finite in float32, got {scale}")
        a = _abi.SacPolicyArgs(count, 0, float(scale or 0.0))
        a.ent_coef = self._float_ptr(who, "ent_coef", ent_coef, (1,))
        if dqmin_da is not None:
            a.dqmin_da = self._float_ptr(who, "dqmin_da", dqmin_da, (count, 6))
            a.d_action_out = self._float_ptr(who, "d_action_out", d_action_out, (count, 6))
        if q is not None:
            a.q = self._float_ptr(who, "q", q, (2, count))
            a.y = self._float_ptr(who, "y", y, (count,))
            a.critic_loss_out = self._float_ptr(who, "critic_loss_out", critic_loss_out, (1,))
        if log_prob is not None:
            a.log_prob = self._float_ptr(who, "log_prob", log_prob, (count,))
            a.q_min = self._float_ptr(who, "q_min", q_min, (count,))
            a.actor_loss_out = self._float_ptr(who, "actor_loss_out", actor_loss_out, (1,))
        _native.check(self.lib.urgym_sac_policy_terms(self._h, C.byref(a), self._stream()), self._h)

    def policy_terms_cloned(self, ent_coef, count, *, dqmin_da, scale, d_action_out, q, y, critic_loss_out, log_prob, q_min, actor_loss_out,
                            action_pi, action_data, weight, bc_scale, scale_by_q=False, q_filter=False, bc_loss_out, bc_weight_out, bc_rows_out,
                            _row_mask=None, _advantage=None):
        """``policy_terms`` with behaviour cloning, in ONE launch in its place (urgym_sac_policy_terms_cloned): all
        three groups of ``policy_terms`` are required, `q` being the online critics at the REPLAYED action.  `action_pi`, `action_data`
        [count, 6]: the policy's action and the ring's on the batch rows.  A row is cloned where `q_filter` is off or ``min(q[0], q[1])
        > q_min``; a cloned row gets ``d_action_out = dqmin_da * scale + ((action_pi - action_data) * w) * bc_scale`` with ``w = weight``
        or, with `scale_by_q`, ``weight * mean |q_min|``; any other row what ``policy_terms`` writes.  ``bc_loss_out`` [1] receives the
        mean over all rows of half the squared distance of the cloned rows, ``bc_weight_out`` [1] w, ``bc_rows_out`` (int32 [1]) the
        number of cloned rows.  Tensors are checked as in ``policy_terms``; the arithmetic is ``evaluation.policy_terms_cloned``,
        bitwise.  On torch's current stream, nothing is synchronised."""
        who = "policy_terms_weighted" if _advantage is not None else "policy_terms_cloned" if _row_mask is None else "policy_terms_cloned_masked"
        count = int(count)
        if not 1 <= count <= _abi.SAC_TERMS_MAX_COUNT:
            raise ValueError(f"{who}: count must be in [1, {_abi.SAC_TERMS_MAX_COUNT}], got {count}")
        for name, x in (("scale", scale), ("bc_scale", bc_scale), ("weight", weight)):
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not self._finite32(x):
                raise ValueError(f"{who}: {name} must be a number that is finite in float32, got {x!r}")
        if float(np.float32(weight)) < 0.0:
            raise ValueError(f"{who}: weight must be >= 0, got {weight}")
        for name, x in (("scale_by_q", scale_by_q), ("q_filter", q_filter)):
            if not isinstance(x, (bool, np.bool_)):
                raise ValueError(f"{who}: {name} must be True or False, got {x!r}")
        a = _abi.SacPolicyArgs(count, 0, float(scale))
        a.ent_coef = self._float_ptr(who, "ent_coef", ent_coef, (1,))
        a.dqmin_da = self._float_ptr(who, "dqmin_da", dqmin_da, (count, 6))
        a.d_action_out = self._float_ptr(who, "d_action_out", d_action_out, (count, 6))
        a.q = self._float_ptr(who, "q", q, (2, count))
        a.y = self._float_ptr(who, "y", y, (count,))
        a.critic_loss_out = self._float_ptr(who, "critic_loss_out", critic_loss_out, (1,))
        a.log_prob = self._float_ptr(who, "log_prob", log_prob, (count,))
        a.q_min = self._float_ptr(who, "q_min", q_min, (count,))
        a.actor_loss_out = self._float_ptr(who, "actor_loss_out", actor_loss_out, (1,))
        b = _abi.SacCloneArgs(weight=float(weight), bc_scale=float(bc_scale), scale_by_q=int(bool(scale_by_q)), q_filter=int(bool(q_filter)), reserved0=0)
        b.action_pi = self._float_ptr(who, "action_pi", action_pi, (count, 6))
        b.action_data = self._float_ptr(who, "action_data", action_data, (count, 6))
        b.bc_loss_out = self._float_ptr(who, "bc_loss_out", bc_loss_out, (1,))
        b.bc_weight_out = self._float_ptr(who, "bc_weight_out", bc_weight_out, (1,))
        b.bc_rows_out = self._float_ptr(who, "bc_rows_out", bc_rows_out, (1,), torch.int32, C.c_int32)
        if d_action_out.data_ptr() in (action_pi.data_ptr(), action_data.data_ptr()):
            raise ValueError(f"{who}: d_action_out must not be action_pi or action_data (the actions are read again after it is written)")
        if _advantage is not None:  # policy_terms_weighted has checked its own arguments; the mask, if any, is in the struct
            _native.check(self.lib.urgym_sac_policy_terms_weighted(self._h, C.byref(a), C.byref(b), C.byref(_advantage), self._stream()), self._h)
            return
        if _row_mask is not None:  # policy_terms_cloned_masked has checked the tensor
            _native.check(self.lib.urgym_sac_policy_terms_cloned_masked(self._h, C.byref(a), C.byref(b), _row_mask.data_ptr(), self._stream()), self._h)
            return
        _native.check(self.lib.urgym_sac_policy_terms_cloned(self._h, C.byref(a), C.byref(b), self._stream()), self._h)

    def policy_terms_cloned_masked(self, ent_coef, count, *, row_mask, **terms):
        """``policy_terms_cloned`` on marked rows only, ONE launch in its place (urgym_sac_policy_terms_cloned_masked; DESIGN.md section
        34): `row_mask` is a contiguous uint8 (or bool) [count] tensor, and a row is cloned only where its mask is nonzero and
        ``policy_terms_cloned``'s verdict holds.  Every other argument and every output is that call's; the means stay over all rows.
        The arithmetic is ``evaluation.policy_terms_cloned(row_mask=)``, bitwise."""
        who = "policy_terms_cloned_masked"
        if not isinstance(row_mask, torch.Tensor):
            raise ValueError(f"{who}: row_mask must be a uint8 [count] tensor on {self.device}, got {type(row_mask).__name__}")
        mask = row_mask.view(torch.uint8) if row_mask.dtype == torch.bool else row_mask
        self._float_ptr(who, "row_mask", mask, (int(count),), torch.uint8, C.c_uint8)
        self.policy_terms_cloned(ent_coef, count, _row_mask=mask, **terms)

    def policy_terms_weighted(self, ent_coef, count, *, temperature, max_weight=None, row_mask=None, adv_ess_out, adv_max_out, adv_clipped_out, **terms):
        """``policy_terms_cloned`` with an advantage weight per row in the place of the verdict, ONE launch in its place
        (urgym_sac_policy_terms_weighted).  Every row with a finite advantage ``A = min(q[0], q[1]) - q_min`` -- and,
        with `row_mask` (a contiguous uint8 or bool [count] tensor), a nonzero mask -- is cloned with the weight ``a = min(e / mean(e),
        max_weight)``, ``e = exp((A - max A) / temperature)``: ``d_action_out = dqmin_da * scale + ((action_pi - action_data) * (w * a))
        * bc_scale``.  `temperature`: finite and > 0 in float32; `max_weight`: None (no cap) or > 0.  ``bc_loss_out`` receives the mean
        over all rows of ``a`` times half the squared distance, ``bc_rows_out`` the number of such rows, ``adv_ess_out`` [1] the effective
        number of rows the weights spread over, ``adv_max_out`` [1] the largest weight, ``adv_clipped_out`` (int32 [1]) the rows the cap
        held.  Every other argument is ``policy_terms_cloned``'s, without ``q_filter``.  The arithmetic is
        ``evaluation.policy_terms_weighted``, bitwise.  On torch's current stream, nothing is synchronised."""
        who = "policy_terms_weighted"
        if not 1 <= int(count) <= _abi.SAC_TERMS_MAX_COUNT:
            raise ValueError(f"{who}: count must be in [1, {_abi.SAC_TERMS_MAX_COUNT}], got {count}")
        if "q_filter" in terms:
            raise ValueError(f"{who}: q_filter is the other gate and is not taken here")
        temperature, max_weight = self._advantage_numbers(who, temperature, max_weight)
        adv = _abi.SacAdvantageArgs(temperature=temperature, max_weight=max_weight, reserved0=0)
        if row_mask is not None:
            if not isinstance(row_mask, torch.Tensor):
                raise ValueError(f"{who}: row_mask must be a uint8 [count] tensor on {self.device}, got {type(row_mask).__name__}")
            mask = row_mask.view(torch.uint8) if row_mask.dtype == torch.bool else row_mask
            adv.row_mask = self._float_ptr(who, "row_mask", mask, (int(count),), torch.uint8, C.c_uint8)
        adv.adv_ess_out = self._float_ptr(who, "adv_ess_out", adv_ess_out, (1,))
        adv.adv_max_out = self._float_ptr(who, "adv_max_out", adv_max_out, (1,))
        adv.adv_clipped_out = self._float_ptr(who, "adv_clipped_out", adv_clipped_out, (1,), torch.int32, C.c_int32)
        self.policy_terms_cloned(ent_coef, count, _advantage=adv, **terms)

    @staticmethod
    def _advantage_numbers(who, temperature, max_weight):
        """(temperature, max_weight) as the floats urgym_sac_policy_terms_weighted takes: a temperature that is finite and > 0 in float32,
        a cap that is None (+infinity) or a number > 0 (a cap above float32's range is +infinity)."""
        with np.errstate(over="ignore"):
            ok = not isinstance(temperature, bool) and isinstance(temperature, (int, float, np.integer, np.floating)) and bool(np.isfinite(np.float32(temperature))) \
                and float(np.float32(temperature)) > 0.0
            if not ok:
                raise ValueError(f"{who}: temperature must be a number that is finite and > 0 in float32, got {temperature!r}")
            if max_weight is None:
                return float(np.float32(temperature)), float("inf")
            ok = not isinstance(max_weight, bool) and isinstance(max_weight, (int, float, np.integer, np.floating)) and float(np.float32(max_weight)) > 0.0
            if not ok:
                raise ValueError(f"{who}: max_weight must be None or a number > 0 in float32, got {max_weight!r}")
            return float(np.float32(temperature)), float(np.float32(max_weight))

    def replay_sample_mixed(self, replay, demonstrations, demo_count, seed, draw, count, batch, source=None):
        """ONE gather launch whose first `demo_count` rows come from `demonstrations` and the rest from `replay` (urgym_replay_sample_mixed;
        DESIGN.md section 34).  `replay`: a ``DeviceReplay`` of this environment; `demonstrations`: a ``DeviceReplay`` of another
        environment of the same kind on this device, with any env count, read at its own ``oldest_slot`` and ``filled``; `batch`: an
        ``_abi.ReplayBatch`` of `count` rows (``DeviceReplay.sample_into(demonstrations=)`` builds it); `source`: None or a contiguous
        uint8 [count] tensor that receives 1 for a demonstration row and 0 otherwise.  The rows are ``evaluation.mixed_entries``'; rows from
        `demo_count` on are bitwise those of the plain gather at the same seed and draw."""
        from .evaluation import DeviceReplay

        who = "replay_sample_mixed"
        if not isinstance(replay, DeviceReplay) or replay.env is not self:
            raise ValueError(f"{who}: replay must be a DeviceReplay of this environment")
        demo = self._demonstrations(who, demonstrations, demo_count)
        count = int(count)
        if demo.count > count:
            raise ValueError(f"{who}: demo_count must be in [0, {count}], got {demo.count}")
        ptr = None if source is None else self._float_ptr(who, "source", source, (count,), torch.uint8, C.c_uint8)
        _native.check(self.lib.urgym_replay_sample_mixed(self._h, C.byref(replay._ring), replay.oldest_slot, replay.filled, int(seed), int(draw), count, C.byref(batch),
                                                         C.byref(demo), C.cast(ptr, C.c_void_p) if ptr is not None else None, self._stream()), self._h)

    def _demonstrations(self, who, demonstrations, demo_count):
        """The urgym_replay_demonstrations of `demonstrations`, a ``DeviceReplay`` of ANOTHER environment of this kind and device."""
        from .evaluation import DeviceReplay

        if not isinstance(demonstrations, DeviceReplay) or demonstrations.env is self:
            raise ValueError(f"{who}: demonstrations must be a DeviceReplay of another environment of the same kind")
        other = demonstrations.env
        if other.env_id != self.env_id or (other.obs_dim, other.goal_dim) != (self.obs_dim, self.goal_dim):
            raise ValueError(f"{who}: the demonstrations come from {other.env_id}, this environment is {self.env_id} (another env kind is out of scope)")
        if torch.device(other.device) != torch.device(self.device):
            raise ValueError(f"{who}: the demonstrations are on {other.device}, this environment on {self.device}")
        return demonstrations.demonstrations_struct(demo_count)

    def evaluation_stats(self, returns, last_step, success, best_mean, best_index, record, eval_index):
        """The statistics of N evaluation episodes, the improvement decision and the best state, in ONE launch of one workgroup
        (urgym_eval_stats): `returns` float64 [N], `last_step` int32 [N], `success` uint8 or bool [N] (the episode summary of
        ``rollout_policy``), N in [1, 65536]; `best_mean` float64 [1] and `best_index` int64 [1] are read and written; `record`, an
        int64 [9] tensor, receives the ``urgym_eval_record`` (``_abi.EvalRecord``).  Needs no environment of N envs.  Every tensor is
        checked, none is converted; the arithmetic is ``evaluation.evaluation_stats``, bitwise.  On torch's current stream, nothing is
        synchronised."""
        who = "evaluation_stats"
        if not isinstance(returns, torch.Tensor) or returns.dim() != 1:
            raise ValueError(f"{who}: returns must be a float64 [N] tensor")
        n = int(returns.shape[0])
        if not 1 <= n <= _abi.EVAL_MAX_COUNT:
            raise ValueError(f"{who}: N must be in [1, {_abi.EVAL_MAX_COUNT}], got {n}")
        if isinstance(eval_index, bool) or int(eval_index) != eval_index or not 0 <= int(eval_index) < 1 << 63:
            raise ValueError(f"{who}: eval_index must be an integer in [0, 2^63), got {eval_index!r}")
        a = _abi.EvalStatsArgs(n, 0, int(eval_index))
        a.episode_return = self._float_ptr(who, "returns", returns, (n,), torch.float64, C.c_double)
        a.episode_last_step = self._float_ptr(who, "last_step", last_step, (n,), torch.int32, C.c_int32)
        a.episode_success = self._float_ptr(who, "success", success, (n,), torch.uint8, C.c_uint8)
        a.best_mean = self._float_ptr(who, "best_mean", best_mean, (1,), torch.float64, C.c_double)
        a.best_index = self._float_ptr(who, "best_index", best_index, (1,), torch.int64, C.c_int64)
        a.record = C.cast(self._float_ptr(who, "record", record, (_abi.EVAL_RECORD_WORDS,), torch.int64, C.c_int64), C.POINTER(_abi.EvalRecord))
        _native.check(self.lib.urgym_eval_stats(self._h, C.byref(a), self._stream()), self._h)

    def actor_snapshot(self, source, destination, in_features, hidden_width, when=None):
        """``destination = source`` for an actor's eight tensors (dicts under ACTOR_ARRAYS + LOG_STD_ARRAYS of float32 device tensors
        shaped for ``in_features -> hidden_width -> hidden_width -> 6``), in ONE launch (urgym_actor_snapshot) -- or nothing at all
        where `when`, an int32 [1] device tensor, holds 0 when the launch runs.  ``when=None`` copies always.  Every tensor is
        checked, none is converted.  On torch's current stream, nothing is synchronised."""
        from .evaluation import ACTOR_ARRAYS, LOG_STD_ARRAYS, DeviceActor

        who = "actor_snapshot"
        keys = ACTOR_ARRAYS + LOG_STD_ARRAYS
        a = _abi.ActorSnapshotArgs(int(in_features), int(hidden_width))
        for name, tensors in (("source", source), ("destination", destination)):
            tensors = dict(tensors)
            if not DeviceActor.check_parameters(tensors, in_features, hidden_width, self.device):
                raise ValueError(f"{who}: {name} needs the log_std head too ({LOG_STD_ARRAYS})")
            setattr(a, name, _abi.ActorTensors(*[C.cast(tensors[k].data_ptr(), C.POINTER(C.c_float)) for k in keys]))
        if when is not None:
            a.when = self._float_ptr(who, "when", when, (1,), torch.int32, C.c_int32)
        _native.check(self.lib.urgym_actor_snapshot(self._h, C.byref(a), self._stream()), self._h)

    def _monitor_state(self, who, state):
        """The checked ``urgym_monitor_state`` of `state`: a dict under the names of ``_abi.MONITOR_STATE_FIELDS`` of [N] device tensors."""
        if not isinstance(state, dict) or sorted(state) != sorted(name for name, _ in _abi.MONITOR_STATE_FIELDS):
            raise ValueError(f"{who}: state must be a dict under {[name for name, _ in _abi.MONITOR_STATE_FIELDS]}")
        m = _abi.MonitorState()
        for name, ct in _abi.MONITOR_STATE_FIELDS:
            dtype = torch.int64 if ct is C.c_int64 else _TORCH_DTYPE[ct]
            setattr(m, name, self._float_ptr(who, f"state[{name!r}]", state[name], (self.num_envs,), dtype, ct))
        return m

    def monitor_fold(self, state, replay, first_slot, num_steps):
        """Follows the episodes of all N envs through `num_steps` steps of `replay` (an ``evaluation.DeviceReplay`` of this environment)
        from slot `first_slot` on -- the slots a ``collect`` with the same arguments has just filled -- in ONE launch, one lane per env
        (urgym_monitor_fold).  `state`: a dict under ``_abi.MONITOR_STATE_FIELDS`` of [N] device tensors (float64 ``running_return``
        and ``sum_return``, int64 ``sum_length``, int32 the others), read and written; all zero is the start.  Every tensor is
        checked, none is converted; the arithmetic is ``evaluation.monitor_fold``, bitwise.  At most the ring's capacity in steps, and
        only with auto_reset.  On torch's current stream, nothing is synchronised."""
        who = "monitor_fold"
        if getattr(replay, "env", None) is not self or not hasattr(replay, "_ring"):
            raise ValueError(f"{who}: replay must be a DeviceReplay allocated for this environment (DeviceReplay(env, capacity_steps))")
        if not self.cfg.auto_reset:
            raise ValueError(f"{who}: the environment has auto_reset off (its episodes do not restart)")
        replay.check_args(replay.capacity, num_steps=num_steps, first_slot=first_slot)
        if int(num_steps) > replay.capacity:
            raise ValueError(f"{who}: num_steps must be at most the ring's {replay.capacity} slots (it no longer holds the earlier steps), got {num_steps}")
        m = self._monitor_state(who, state)
        _native.check(self.lib.urgym_monitor_fold(self._h, C.byref(m), C.byref(replay._ring), int(first_slot), int(num_steps), self._stream()), self._h)

    def monitor_stats(self, state, record, iteration, clear=True):
        """The episodes finished since the last clear, over all N envs, reduced to one ``urgym_monitor_record`` (``_abi.MonitorRecord``)
        in `record`, an int64 [9] tensor, in ONE launch of one workgroup (urgym_monitor_stats); `iteration` is the caller's tag.  With
        `clear` the interval entries of `state` are zeroed, the episodes in progress stay.  The arithmetic is
        ``evaluation.monitor_stats``, bitwise.  On torch's current stream, nothing is synchronised."""
        who = "monitor_stats"
        if isinstance(iteration, bool) or int(iteration) != iteration or not -(1 << 63) <= int(iteration) < 1 << 63:
            raise ValueError(f"{who}: iteration must be an integer that fits int64, got {iteration!r}")
        m = self._monitor_state(who, state)
        rec = C.cast(self._float_ptr(who, "record", record, (_abi.MONITOR_RECORD_WORDS,), torch.int64, C.c_int64), C.POINTER(_abi.MonitorRecord))
        _native.check(self.lib.urgym_monitor_stats(self._h, C.byref(m), rec, int(iteration), int(bool(clear)), self._stream()), self._h)

    def sac_learner(self, *, actor, online, target, actor_params, actor_grads, actor_exp_avg, actor_exp_avg_sq, critic_params, critic_grads,
                    critic_exp_avg, critic_exp_avg_sq, actor_workspace, critic_workspace, log_ent_coef, exp_avg, exp_avg_sq, replay, batch, scratch,
                    count, seed, update_seed, gamma, tau, target_entropy, lr, betas=(0.9, 0.999), eps=1e-8):
        """The ``urgym_sac_learner`` of ``sac_train``, built and checked ONCE: a ``SacLearnerBinding`` that holds the struct and keeps
        every tensor it points to alive.  `actor`, `online`, `target`: the DeviceActor and the two DeviceCritics of this environment;
        the four actor sets as ``actor_adam_step`` takes them, the four critic sets as ``critic_adam_step`` does (the grads are the
        tensors the gradient launches write); the two workspaces from ``actor_gradient_workspace`` / ``critic_gradient_workspace``
        for `count` rows; `log_ent_coef`, `exp_avg`, `exp_avg_sq`: the temperature's [1] tensors; `replay`: a DeviceReplay of this
        environment; `batch`: a dict under the ring's field names (``truncated``, ``is_success`` and ``index`` optional) of [count, ...]
        tensors as ``DeviceReplay.sample_into`` takes them; `scratch`: a dict under the names of ``_abi.SAC_LEARNER_SCRATCH``.  Every
        tensor is checked (dtype, contiguity, device, shape) and none is converted; ValueError otherwise."""
        from .evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic

        who = "sac_learner"
        a = self._actor_ptr(actor)
        for name, c in (("online", online), ("target", target)):
            if getattr(c, "env", None) is not self or not getattr(c, "_c", None):
                raise ValueError(f"{who}: {name} must be a live DeviceCritic loaded for this environment (DeviceCritic.load(paths, env))")
        if online is target:
            raise ValueError(f"{who}: the target is the online critic itself")
        if getattr(replay, "env", None) is not self or not hasattr(replay, "_ring"):
            raise ValueError(f"{who}: replay must be a DeviceReplay allocated for this environment (DeviceReplay(env, capacity_steps))")
        M = int(count)
        if not 1 <= M <= _abi.SAC_TRAIN_MAX_COUNT:
            raise ValueError(f"{who}: count must be in [1, {_abi.SAC_TRAIN_MAX_COUNT}], got {count}")
        for name, x in (("gamma", gamma), ("tau", tau), ("target_entropy", target_entropy)):
            if not self._finite32(x):
                raise ValueError(f"{who}: {name} must be finite in float32, got {x}")
        if not 0.0 < float(tau) <= 1.0:
            raise ValueError(f"{who}: tau must be in (0, 1], got {tau}")
        hyper = self._adam_hyper(lr, betas, eps, 1)
        L = _abi.SacLearner()
        keep = []
        L.actor, L.online, L.target = a, online._c, target._c
        L.actor_adam = _abi.ActorAdam(actor.in_features, actor.hidden_width, 0)
        for name, tensors in zip(_abi.ADAM_SETS, (actor_params, actor_grads, actor_exp_avg, actor_exp_avg_sq)):
            tensors = dict(tensors)
            if not DeviceActor.check_parameters(tensors, actor.in_features, actor.hidden_width, self.device):
                raise ValueError(f"{who}: the actor's {name} needs the log_std head too ({LOG_STD_ARRAYS})")
            setattr(L.actor_adam, name, _abi.ActorTensors(*[C.cast(tensors[k].data_ptr(), C.POINTER(C.c_float)) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS]))
            keep.append(tensors)
        L.critic_adam = _abi.CriticAdam(online.in_features, online.hidden_width, 0)
        for name, tensors in zip(_abi.ADAM_SETS, (critic_params, critic_grads, critic_exp_avg, critic_exp_avg_sq)):
            tensors = [dict(w) for w in tensors]
            DeviceCritic.check_parameters(tensors, online.in_features, online.hidden_width, self.device)
            nets = getattr(L.critic_adam, name)
            for i, w in enumerate(tensors):
                nets[i] = _abi.QNetworkDev(*[C.cast(w[k].data_ptr(), C.POINTER(C.c_float)) for k in CRITIC_ARRAYS])
            keep.append(tensors)
        for name, w in (("actor_workspace", actor_workspace), ("critic_workspace", critic_workspace)):
            if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or not w.is_contiguous() or w.device != torch.device(self.device) or w.dim() != 1:
                raise ValueError(f"{who}: {name} must be a contiguous float32 [n] tensor on {self.device} (actor_gradient_workspace / critic_gradient_workspace)")
            setattr(L, name, w.data_ptr())
            setattr(L, name + "_bytes", w.numel() * 4)
            keep.append(w)
        for name, t in zip(_abi.SAC_LEARNER_STATE, (log_ent_coef, exp_avg, exp_avg_sq)):
            setattr(L, name, self._float_ptr(who, name, t, (1,)))
            keep.append(t)
        L.ring = replay._ring
        keep.append(replay)
        kinds = {name: (ct, shape(1, 1, self.obs_dim, self.goal_dim)[2:], required) for name, ct, shape, required in _abi.REPLAY_RING_FIELDS}
        kinds["index"] = (C.c_int64, (), False)
        batch = dict(batch)
        unknown = [k for k in batch if k not in kinds]
        if unknown:
            raise ValueError(f"{who}: unknown batch fields {unknown}; available: {sorted(kinds)}")
        for name, (ct, tail, required) in kinds.items():
            if name not in batch or batch[name] is None:
                if required:
                    raise ValueError(f"{who}: batch[{name!r}] is required (only truncated, is_success and index are optional)")
                continue
            dtype = torch.int64 if ct is C.c_int64 else _TORCH_DTYPE[ct]
            setattr(L.batch, name, self._float_ptr(who, f"batch[{name!r}]", batch[name], (M,) + tuple(tail), dtype, ct))
        keep.append(batch)
        scratch = dict(scratch)
        unknown = [k for k in scratch if k not in dict(_abi.SAC_LEARNER_SCRATCH)]
        if unknown:
            raise ValueError(f"{who}: unknown scratch tensors {unknown}; expected {[n for n, _ in _abi.SAC_LEARNER_SCRATCH]}")
        for name, shape in _abi.SAC_LEARNER_SCRATCH:
            if name not in scratch:
                raise ValueError(f"{who}: scratch[{name!r}] is missing")
            setattr(L, name, self._float_ptr(who, f"scratch[{name!r}]", scratch[name], shape(M)))
        keep.append(scratch)
        L.count, L.reserved0, L.seed, L.update_seed = M, 0, int(seed), int(update_seed)
        L.gamma, L.tau, L.target_entropy = float(gamma), float(tau), float(target_entropy)
        L.lr, L.beta1, L.beta2, L.eps = hyper.lr, hyper.beta1, hyper.beta2, hyper.eps
        return SacLearnerBinding(self, L, keep, actor, dict(actor_params))

    def sac_train(self, learner, critic_loss, actor_loss, ent_coef_loss, *, first_slot, filled_steps, num_iterations, steps_per_iteration=1,
                  updates_per_iteration=1, uniform_iterations=0, idle_iterations=0, collect_first_draw=0, update_first_draw=0, first_step=1,
                  evaluation=None, eval_every=None, monitor=None, log_every=None, nstep=None, prioritized=None, hindsight=None, clipping=None,
                  normalizer=None, planner=None, cloning=None, demonstrating=None, weighting=None):
        """``num_iterations`` x (a collection of ``steps_per_iteration`` steps, ``updates_per_iteration`` SAC updates) in ONE native
        call (urgym_sac_train): the launches of ``collect`` and of the thirteen calls of an update, bit for bit, without returning to
        Python in between.  `learner`: what ``sac_learner`` returned, or a dict of its keyword arguments (then built and checked here).
        `critic_loss`, `actor_loss`, `ent_coef_loss`: float32 tensors of one entry per update of the call, update u writes entry u.
        The schedule as ``evaluation.training_schedule`` takes it (``capacity_steps`` is the replay's); the caller owns the ring's
        cursor and fill level, the draw counters and the step count, and advances them.  On torch's current stream; nothing is
        synchronised, nothing is converted.  Returns the number of updates.

        The options combine freely but for the three gathers (`nstep`, `prioritized`, `hindsight`: at most one); an option left out
        changes nothing.  Which urgym_sac_train_* entry point serves the call is ``_sac_train_entry``'s table.

        With `evaluation` (an ``evaluation.DeviceEvaluation`` on a SECOND environment of this device) and `eval_every` (updates between
        evaluations): an evaluation of the learner's actor parameters after every iteration in which the update count passes a
        multiple of `eval_every` (``evaluation.evaluation_points``), into `evaluation`'s next records; its counters are advanced.

        With `monitor` (an ``evaluation.DeviceMonitor`` of this environment) and `log_every` (iterations between records): after every
        iteration that collects one ``monitor.fold`` of its slots, and after every iteration at which the monitor's iteration count
        reaches a multiple of `log_every` one ``monitor.record`` (``evaluation.monitor_points``); the monitor's count and record cursor
        are advanced.

        With `nstep` (a dict: ``n_steps`` in [2, 32] and the float32 [count] scratch tensors ``discount`` and ``q_min_next``): every
        update gathers multi-step returns (``DeviceReplay.sample_targets(n_steps=)``) and forms y by ``entropy_step_nstep``.

        With `prioritized` (a dict: ``replay``, the ``DevicePrioritizedReplay`` the learner's ring belongs to, ``beta0``,
        ``beta_steps``, and the scratch tensors of ``_abi.SAC_PRIORITIZED_SCRATCH`` and ``total``, float64 [1]): every collection is
        followed by the fill of its slots and every update draws through the priorities and writes the new ones back.

        With `hindsight` (a dict: ``n_sampled_goal``, ``strategy`` "future" or "final", ``horizon``): every update's gather is the one
        of ``DeviceReplay.sample_hindsight``.

        With `clipping` (a dict: ``max_grad_norm``, ``scale``, a float32 [2] scratch tensor, and ``critic_grad_norm`` and
        ``actor_grad_norm``, float32 tensors of one entry per update of the call like the losses): every update runs
        ``critic_gradient_norm`` and ``actor_gradient_norm`` before the two steps, which take the coefficients (``scale=``); update u
        writes the norms to entry u.

        With `normalizer` (an ``evaluation.DeviceNormalizer`` of this environment): every collection is ``collect(..., normalizer=)``
        followed by ``norm_fold`` of its slots, and every update's gather is followed by ``norm_batch``.  An `evaluation` given with it
        must have been made with this normalizer (``DeviceEvaluation(..., normalizer=)``): its evaluations are
        ``evaluation.evaluate``'s, on normalized rows, with the statistics snapshot beside the best actor.

        With `planner` (a dict: ``planner``, an ``evaluation.DeviceMPPI`` whose source is this environment, and optionally
        ``explore_sigma`` (0), ``sync`` (True) and ``records`` (False)): every collection is the planner's
        (``DeviceMPPI.collect(..., first_draw=collect_first_draw + i K, explore_sigma=)``, urgym_sac_train_planned); with ``sync`` the
        planner's actor and critic are reloaded from the learner's parameters after the updates of every iteration that has any; with
        ``records`` (it needs `monitor`) one ``DeviceMPPI.stats`` record is written beside every monitor record, into
        ``planner.records`` at the monitor's own index.  ``uniform_iterations`` must be 0; not together with `normalizer`.

        With `cloning` (a dict: ``weight``, optionally ``scale_by_q`` and ``q_filter`` (False), and ``bc_loss``, ``bc_weight`` (float32)
        and ``bc_rows`` (int32), tensors of one entry per update of the call like the losses): every update's ``policy_terms`` is
        ``policy_terms_cloned`` on the policy's action and the batch's (urgym_sac_train_cloned), ``bc_scale`` = 1 / count; update u
        writes entry u of the three.  With any of the options above.

        With `demonstrating` (a dict: ``replay``, a ``DeviceReplay`` of another environment of the same kind holding the demonstrations,
        ``count`` = D of the learner's rows, ``source``, a uint8 [count of the learner] scratch tensor, and optionally ``clone_only``
        (False; True needs `cloning`)): every update's gather is the mixed one (``DeviceReplay.sample_into(demonstrations=)``,
        urgym_sac_train_demonstrated) and, with ``clone_only``, its policy terms are ``policy_terms_cloned_masked`` with ``row_mask =
        source``.  Not together with `nstep`, `prioritized` or `hindsight`.

        With `weighting` (a dict: ``temperature``, optionally ``max_weight`` (None: no cap), and ``adv_ess``, ``adv_max`` (float32) and
        ``adv_clipped`` (int32) device tensors of one entry per update; it needs `cloning` without ``q_filter``): every update's policy
        terms are ``policy_terms_weighted`` (urgym_sac_train_weighted), with ``row_mask = source`` where `demonstrating` has
        ``clone_only``; update u writes entry u of the three.  With any of the options above."""
        from .evaluation import DeviceEvaluation, DeviceMonitor, DeviceMPPI, _her_arguments, evaluation_points, monitor_points, relabel_threshold, training_schedule

        who = "sac_train"
        if isinstance(learner, dict):
            learner = self.sac_learner(**learner)
        if not isinstance(learner, SacLearnerBinding) or learner.env is not self:
            raise ValueError(f"{who}: learner must come from this environment's sac_learner")
        sched = dict(first_slot=first_slot, filled_steps=filled_steps, capacity_steps=int(learner.struct.ring.capacity_steps), num_iterations=num_iterations,
                     steps_per_iteration=steps_per_iteration, updates_per_iteration=updates_per_iteration, uniform_iterations=uniform_iterations,
                     idle_iterations=idle_iterations, collect_first_draw=collect_first_draw, update_first_draw=update_first_draw, first_step=first_step)
        for name, v in sched.items():
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{who}: {name} must be an integer, got {v!r}")
        sched = {k: int(v) for k, v in sched.items()}
        ints = [k for k in sched if k not in ("collect_first_draw", "update_first_draw", "first_step")]
        if any(not -(1 << 31) <= sched[k] < 1 << 31 for k in ints) or not all(0 <= sched[k] < 1 << 64 for k in ("collect_first_draw", "update_first_draw")) \
                or not -(1 << 63) <= sched["first_step"] < 1 << 63:
            raise ValueError(f"{who}: a number of the schedule does not fit its field (int32 counts, uint64 draws, int64 first_step)")
        if (evaluation is None) != (eval_every is None):
            raise ValueError(f"{who}: evaluation and eval_every go together")
        points = []
        given = {}  # option name -> its _abi struct, for the options that are given
        if evaluation is not None:
            if not isinstance(evaluation, DeviceEvaluation):
                raise ValueError(f"{who}: evaluation must be a DeviceEvaluation")
            if evaluation.env is self:
                raise ValueError(f"{who}: the evaluation needs an environment of its own (an evaluation resets it); evaluation on the training env is not supported")
            if isinstance(eval_every, bool) or int(eval_every) != eval_every or not 1 <= int(eval_every) < 1 << 31:
                raise ValueError(f"{who}: eval_every must be an integer in [1, 2^31), got {eval_every!r}")
            given["evaluation"] = _abi.SacEvaluation(evaluation.env._h, evaluation.struct(learner.actor_params), int(eval_every), evaluation.count, evaluation.count)
            if sched["first_step"] >= 1 and sched["num_iterations"] >= 1 and min(sched["updates_per_iteration"], sched["idle_iterations"]) >= 0:
                points = evaluation_points(sched["first_step"], sched["num_iterations"], sched["updates_per_iteration"], sched["idle_iterations"], eval_every)
        if (monitor is None) != (log_every is None):
            raise ValueError(f"{who}: monitor and log_every go together")
        if monitor is not None:
            if not isinstance(monitor, DeviceMonitor) or monitor.env is not self:
                raise ValueError(f"{who}: monitor must be a DeviceMonitor of this environment")
            if isinstance(log_every, bool) or int(log_every) != log_every or not 1 <= int(log_every) < 1 << 31:
                raise ValueError(f"{who}: log_every must be an integer in [1, 2^31), got {log_every!r}")
            given["monitor"] = monitor.struct(int(log_every))
            logged = monitor_points(monitor.iterations, max(0, sched["num_iterations"]), int(log_every))
        active = max(0, sched["num_iterations"] - max(0, sched["idle_iterations"]))
        updates = active * max(0, sched["updates_per_iteration"])
        L = learner.struct
        if nstep is not None:
            n_steps = nstep["n_steps"]
            if isinstance(n_steps, bool) or int(n_steps) != n_steps or not 2 <= int(n_steps) <= _abi.REPLAY_NSTEP_MAX:
                raise ValueError(f"{who}: nstep['n_steps'] must be an integer in [2, {_abi.REPLAY_NSTEP_MAX}], got {n_steps!r}")
            count = int(L.count)
            given["nstep"] = _abi.SacNstep(int(n_steps), 0, self._float_ptr(who, "nstep['discount']", nstep["discount"], (count,)),
                                           self._float_ptr(who, "nstep['q_min_next']", nstep["q_min_next"], (count,)))
        if prioritized is not None:
            if nstep is not None:
                raise ValueError(f"{who}: priorities together with multi-step returns are out of scope (the multi-step gather draws its own indices)")
            rp, count = prioritized["replay"], int(L.count)
            total = prioritized["total"]
            if total.dtype != torch.float64 or tuple(total.shape) != (1,) or total.device != torch.device(self.device):
                raise ValueError(f"{who}: prioritized['total'] must be a float64 [1] tensor on {self.device}")
            P_ = given["prioritized"] = _abi.SacPrioritized(priorities=rp.priorities_struct(), beta0=float(prioritized["beta0"]), beta_steps=int(prioritized["beta_steps"]),
                                                            alpha=rp.alpha, eps=rp.eps, total=C.cast(total.data_ptr(), C.POINTER(C.c_double)))
            for name, shape in _abi.SAC_PRIORITIZED_SCRATCH:
                setattr(P_, name, self._float_ptr(who, f"prioritized[{name!r}]", prioritized[name], shape(count)))
        if hindsight is not None:
            if nstep is not None or prioritized is not None:
                raise ValueError(f"{who}: hindsight together with multi-step returns or priorities is out of scope")
            if hindsight["strategy"] not in ("future", "final"):
                raise ValueError(f"{who}: hindsight['strategy'] must be 'future' or 'final', got {hindsight['strategy']!r}")
            given["hindsight"] = _abi.SacHindsight(*_her_arguments(relabel_threshold(hindsight["n_sampled_goal"]), hindsight["strategy"], hindsight["horizon"]), 0)
        for name, t in zip(_abi.SAC_LEARNER_LOSSES, (critic_loss, actor_loss, ent_coef_loss)):
            setattr(L, name, self._float_ptr(who, name, t, (updates,)))
        S = _abi.SacSchedule(*[sched[name] for name, _ in _abi.SacSchedule._fields_])
        if clipping is not None:
            max_grad_norm = float(clipping["max_grad_norm"])
            if not (self._finite32(max_grad_norm) and max_grad_norm > 0.0):
                raise ValueError(f"{who}: clipping['max_grad_norm'] must be finite and positive, got {max_grad_norm}")
            given["clipping"] = _abi.SacClipping(max_grad_norm, 0, self._float_ptr(who, "clipping['scale']", clipping["scale"], (2,)),
                                                 self._float_ptr(who, "clipping['critic_grad_norm']", clipping["critic_grad_norm"], (updates,)),
                                                 self._float_ptr(who, "clipping['actor_grad_norm']", clipping["actor_grad_norm"], (updates,)))
        if evaluation is not None and getattr(evaluation, "normalizer", None) is not normalizer:
            raise ValueError(f"{who}: the evaluation and the call must share one normalizer (DeviceEvaluation(..., normalizer=)), or have none")
        if normalizer is not None:
            given["normalizer"] = self._normalization(who, normalizer)
            if evaluation is not None:
                given["normalizer"] = evaluation.norm_struct()
            if sched["steps_per_iteration"] > normalizer.fold_steps:
                raise ValueError(f"{who}: steps_per_iteration must be at most the normalizer's fold_steps = {normalizer.fold_steps} (its workspace)")
        if planner is not None:
            mppi = planner.get("planner") if isinstance(planner, dict) else None
            if not isinstance(mppi, DeviceMPPI) or mppi.env is not self:
                raise ValueError(f"{who}: planner must be a dict whose 'planner' is a DeviceMPPI of this environment (DeviceMPPI(env, ...))")
            unknown = [k for k in planner if k not in ("planner", "explore_sigma", "sync", "records")]
            if unknown:
                raise ValueError(f"{who}: unknown planner options {unknown}; available: planner, explore_sigma, sync, records")
            if normalizer is not None:
                raise ValueError(f"{who}: planner together with normalizer is out of scope (the planner's actor and critic read raw rows)")
            if planner.get("records", False) and monitor is None:
                raise ValueError(f"{who}: the planner's records need monitor (a plan-statistics record goes beside a monitor record)")
            if planner.get("records", False):
                mppi.reserve_records(monitor.count + len(logged))
            given["planner"] = mppi.planning(planner.get("explore_sigma", 0.0), planner.get("sync", True), planner.get("records", False))
            if mppi.temper() is not None:
                given["temper"] = mppi.temper()
            if mppi.noise() is not None:
                given["noise"] = mppi.noise()
        if cloning is not None:
            unknown = [k for k in cloning if k not in ("weight", "scale_by_q", "q_filter", "bc_loss", "bc_weight", "bc_rows")]
            if unknown:
                raise ValueError(f"{who}: unknown cloning options {unknown}; available: weight, scale_by_q, q_filter, bc_loss, bc_weight, bc_rows")
            weight = cloning["weight"]
            if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not self._finite32(weight) or float(np.float32(weight)) < 0.0:
                raise ValueError(f"{who}: cloning['weight'] must be a number that is finite in float32 and >= 0, got {weight!r}")
            flags = [cloning.get(k, False) for k in ("scale_by_q", "q_filter")]
            if not all(isinstance(x, (bool, np.bool_)) for x in flags):
                raise ValueError(f"{who}: cloning['scale_by_q'] and cloning['q_filter'] must be True or False")
            given["cloning"] = _abi.SacCloning(float(weight), int(flags[0]), int(flags[1]), 0, self._float_ptr(who, "cloning['bc_loss']", cloning["bc_loss"], (updates,)),
                                               self._float_ptr(who, "cloning['bc_weight']", cloning["bc_weight"], (updates,)),
                                               self._float_ptr(who, "cloning['bc_rows']", cloning["bc_rows"], (updates,), torch.int32, C.c_int32))
        if demonstrating is not None:
            from .evaluation import DEMO_OUT_OF_SCOPE

            unknown = [k for k in demonstrating if k not in ("replay", "count", "source", "clone_only")]
            if unknown:
                raise ValueError(f"{who}: unknown demonstrating options {unknown}; available: replay, count, source, clone_only")
            if nstep is not None or prioritized is not None or hindsight is not None:
                raise ValueError(f"{who}: {DEMO_OUT_OF_SCOPE}")
            clone_only = demonstrating.get("clone_only", False)
            if not isinstance(clone_only, (bool, np.bool_)):
                raise ValueError(f"{who}: demonstrating['clone_only'] must be True or False")
            if clone_only and cloning is None:
                raise ValueError(f"{who}: demonstrating['clone_only'] needs cloning")
            demo = self._demonstrations(who, demonstrating["replay"], demonstrating["count"])
            if demo.count > int(L.count):
                raise ValueError(f"{who}: demonstrating['count'] must be in [0, {int(L.count)}], got {demo.count}")
            given["demonstrating"] = _abi.SacDemonstrating(demo, self._float_ptr(who, "demonstrating['source']", demonstrating["source"], (int(L.count),), torch.uint8, C.c_uint8),
                                                           int(bool(clone_only)), 0)
        if weighting is not None:
            unknown = [k for k in weighting if k not in ("temperature", "max_weight", "adv_ess", "adv_max", "adv_clipped")]
            if unknown:
                raise ValueError(f"{who}: unknown weighting options {unknown}; available: temperature, max_weight, adv_ess, adv_max, adv_clipped")
            if cloning is None:
                raise ValueError(f"{who}: weighting needs cloning (it weights the cloning term)")
            if cloning.get("q_filter", False):
                raise ValueError(f"{who}: weighting together with cloning['q_filter'] is refused (the two gates are alternatives)")
            temperature, max_weight = self._advantage_numbers(who, weighting["temperature"], weighting.get("max_weight"))
            given["weighting"] = _abi.SacWeighting(temperature, max_weight, 0, self._float_ptr(who, "weighting['adv_ess']", weighting["adv_ess"], (updates,)),
                                                   self._float_ptr(who, "weighting['adv_max']", weighting["adv_max"], (updates,)),
                                                   self._float_ptr(who, "weighting['adv_clipped']", weighting["adv_clipped"], (updates,), torch.int32, C.c_int32))
        symbol, options = _sac_train_entry(given)
        try:
            _native.check(getattr(self.lib, symbol)(self._h, C.byref(L), C.byref(S), *[C.byref(given[o]) if o in given else None for o in options], self._stream()), self._h)
            if monitor is not None:
                monitor.advance(sched["num_iterations"], len(logged))
            if evaluation is not None:
                evaluation.advance(len(points))
        finally:
            for name in _abi.SAC_LEARNER_LOSSES:  # the loss slots belong to this call alone
                setattr(L, name, None)
        learner.actor.has_log_std = True
        return updates

    def policy_actions(self, actor, out=None, sample=None, rows=None):
        """model.predict(obs, deterministic=True) (model_test.py:41) for all envs, by the HIP actor kernel, from the live
        observation buffers: float32 [N, 6] on the device.

        With `sample` (see ``rollout_policy``) the actions are drawn -- model.predict(obs, deterministic=False) -- and the return
        value is ``(actions, log_prob)``, log_prob float32 [N] (None for mode "mean" on an actor without log_std head).

        With `rows` (as in ``critic_values``: leading shape [K, N] or [M]) the policy is evaluated on those rows instead of the live
        buffers (urgym_actor_sample_rows): SAC's a' ~ pi(.|s') on next-observation rows.  The noise of row i is that of env i, so on
        copies of the live buffers the result is bitwise the same.  Returns [..., 6] (and [...]); without `sample`, the mean action."""
        a = self._actor_ptr(actor)
        if rows is not None:
            cr, lead, keep = self._rows(rows)
            if out is None:
                out = torch.empty(lead + (6,), dtype=torch.float32, device=self.device)
            elif tuple(out.shape) != lead + (6,) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
                raise ValueError(f"out must be a contiguous float32 {lead + (6,)} tensor on {self.device}")
            how = self._sampling(sample if sample is not None else dict(mode="mean"))
            log_prob = None
            if sample is not None and (how.mode != _abi.SAMPLE_MEAN or actor.has_log_std):
                log_prob = torch.empty(lead, dtype=torch.float32, device=self.device)
            _native.check(self.lib.urgym_actor_sample_rows(self._h, a, C.byref(how), C.byref(cr), int(np.prod(lead)), C.c_void_p(out.data_ptr()),
                                                           C.c_void_p(log_prob.data_ptr()) if log_prob is not None else None, self._stream()), self._h)
            return out if sample is None else (out, log_prob)
        if out is None:
            out = torch.empty((self.num_envs, 6), dtype=torch.float32, device=self.device)
        elif out.shape != (self.num_envs, 6) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 [{self.num_envs}, 6] tensor on {self.device}")
        if sample is None:
            _native.check(self.lib.urgym_actor_forward(self._h, a, C.c_void_p(out.data_ptr()), self._stream()), self._h)
            return out
        how = self._sampling(sample)
        log_prob = None
        if how.mode != _abi.SAMPLE_MEAN or actor.has_log_std:
            log_prob = torch.empty((self.num_envs,), dtype=torch.float32, device=self.device)
        _native.check(self.lib.urgym_actor_sample(self._h, a, C.byref(how), C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(log_prob.data_ptr()) if log_prob is not None else None, self._stream()), self._h)
        return out, log_prob

    def rollout_policy(self, actor, num_steps, record=("reward", "terminated", "truncated", "is_success"), sample=None):
        """`num_steps` x (actor, step) without returning to Python: the loop of model_test.py:38-50, or an on-policy collection.

        `sample` = dict(mode=, seed=, first_draw=) makes the actor stochastic, as SAC collects (train.py): mode "gaussian" draws
        tanh(mu + exp(log_std) eps) (the actor needs its log_std arrays), "uniform" draws 2 u - 1 without a forward pass (SAC's
        warm-up before learning_starts), "mean" is the deterministic policy.  Pass k uses draw first_draw + k, so a rollout split
        in two calls (the second with first_draw advanced) draws the same noise; ``evaluation.policy_noise`` restates it.  With
        `sample`, `record` may also name SAMPLE_RECORD_KEYS: ``log_prob`` [K, N], ``noise`` (eps, or u), ``mean_action`` =
        tanh(mu) and ``log_std`` (clamped) as [K, N, 6]; "uniform" leaves the last two zero.  Without `sample` nothing changes.

        `record` names what to keep (RECORD_KEYS; "all" = every one): per step ``observation`` / ``achieved_goal`` / ``desired_goal``
        (what the actor saw) and ``action`` as [K, N, dim]; ``reward``, ``terminated``, ``truncated``, ``is_success``, ``collision``
        as [K, N]; ``final_observation`` [K, N, obs_dim] (auto-reset only; rows valid where terminated | truncated); and per env the
        summary of its first episode, ``episode_return`` (float64), ``episode_last_step``, ``episode_success``, ``episode_done``.
        Returns a dict of fresh device tensors (flags as bool views).  Nothing is synchronised: the tensors are valid in stream
        order.  Afterwards the environment is where `num_steps` calls of ``step`` would have left it."""
        a = self._actor_ptr(actor)
        K = int(num_steps)
        if K < 0:
            raise ValueError("num_steps must be >= 0")
        how = self._sampling(sample) if sample is not None else None
        density = how is not None and (how.mode == _abi.SAMPLE_UNIFORM or actor.has_log_std)  # the sample records exist
        names = self.RECORD_KEYS + (self.SAMPLE_RECORD_KEYS if density else ()) if record == "all" else tuple(record)
        if record == "all" and not self.cfg.auto_reset:
            names = tuple(n for n in names if n != "final_observation")
        known = self.RECORD_KEYS + (self.SAMPLE_RECORD_KEYS if how is not None else ())
        unknown = [n for n in names if n not in known]
        if unknown:
            raise ValueError(f"unknown record {unknown}; available: {known}")
        if "final_observation" in names and not self.cfg.auto_reset:
            raise ValueError("final_observation exists only with auto_reset")
        traj, out = _abi.Trajectory(), {}
        for name, ct, shape in _abi.TRAJECTORY_FIELDS:
            if name in names:
                t = torch.zeros(shape(K, self.num_envs, self.obs_dim, self.goal_dim), dtype=_TORCH_DTYPE[ct], device=self.device)
                setattr(traj, name, C.cast(t.data_ptr(), C.POINTER(ct)))
                out[name] = t.view(torch.bool) if ct is C.c_uint8 else t
        if how is None:
            _native.check(self.lib.urgym_rollout_actor(self._h, a, K, C.byref(traj) if names else None, self._stream()), self._h)
            return out
        extra = _abi.SampleRecords()
        for name, ct, shape in _abi.SAMPLE_RECORD_FIELDS:
            if name in names:
                out[name] = torch.zeros(shape(K, self.num_envs), dtype=_TORCH_DTYPE[ct], device=self.device)
                setattr(extra, name, C.cast(out[name].data_ptr(), C.POINTER(ct)))
        _native.check(self.lib.urgym_rollout_sampled(self._h, a, C.byref(how), K, C.byref(traj), C.byref(extra), self._stream()), self._h)
        return out

    def _normalization(self, who, normalizer, same_kind=False):
        """The ``urgym_normalization`` of `normalizer`, an ``evaluation.DeviceNormalizer`` of this environment, as it stands now.
        `same_kind`: one of another environment of this env kind on this device will do (only its statistics are read)."""
        other = getattr(normalizer, "env", None)
        if not hasattr(normalizer, "struct") or (other is not self and not (same_kind and other is not None and other.env_kind == self.env_kind
                                                                            and other.device == self.device)):
            raise ValueError(f"{who}: normalizer must be a DeviceNormalizer of this environment (DeviceNormalizer(env, ...))")
        return normalizer.struct()

    def norm_fold(self, normalizer, replay, first_slot, num_steps):
        """Folds what the actor saw and the rewards of `num_steps` steps of `replay` from slot `first_slot` on -- the slots a
        ``collect`` with the same arguments has just filled -- into the running statistics of `normalizer` (an
        ``evaluation.DeviceNormalizer`` of this environment), slot by slot, in TWO launches whatever `num_steps` is (urgym_norm_fold).
        With ``normalizer.training`` False nothing is launched.  The arithmetic is ``evaluation.norm_fold``, bitwise.  At most
        ``normalizer.fold_steps`` steps (the workspace's size) and the ring's capacity, and only with auto_reset.  On torch's current
        stream, nothing is synchronised."""
        who = "norm_fold"
        if getattr(replay, "env", None) is not self or not hasattr(replay, "_ring"):
            raise ValueError(f"{who}: replay must be a DeviceReplay allocated for this environment (DeviceReplay(env, capacity_steps))")
        if not self.cfg.auto_reset:
            raise ValueError(f"{who}: the environment has auto_reset off (its episodes do not restart)")
        replay.check_args(replay.capacity, num_steps=num_steps, first_slot=first_slot)
        if int(num_steps) > replay.capacity:
            raise ValueError(f"{who}: num_steps must be at most the ring's {replay.capacity} slots (it no longer holds the earlier steps), got {num_steps}")
        n = self._normalization(who, normalizer)
        if int(num_steps) > normalizer.fold_steps:
            raise ValueError(f"{who}: num_steps must be at most the normalizer's fold_steps = {normalizer.fold_steps} (its workspace), got {num_steps}")
        _native.check(self.lib.urgym_norm_fold(self._h, C.byref(n), C.byref(replay._ring), int(first_slot), int(num_steps), self._stream()), self._h)

    _NORM_ROWS = ("observation", "achieved_goal", "desired_goal")

    def norm_rows(self, normalizer, rows, out=None):
        """Normalizes rows with the statistics of `normalizer` as they stand when the launch RUNS, in ONE launch (urgym_norm_rows).
        `rows`: a dict under some or all of ``observation`` [count, obs_dim], ``achieved_goal`` and ``desired_goal`` [count, goal_dim]
        (float32 device tensors, any leading shape, the same for all); `out`: the destinations under the same names (default: fresh
        tensors; `rows` itself = in place).  Returns `out`.  The arithmetic is ``evaluation.normalize_rows``, bitwise.  The normalizer
        may belong to another environment of this env kind: an evaluation environment reads the TRAINING statistics this way (SB3's
        ``sync_envs_normalization``)."""
        who = "norm_rows"
        n = self._normalization(who, normalizer, same_kind=True)
        names = [k for k in self._NORM_ROWS if k in rows]
        if not names or len(names) != len(rows):
            raise ValueError(f"{who}: rows must be a dict under some of {self._NORM_ROWS}")
        if out is None:
            out = {k: torch.empty_like(rows[k]) for k in names}
        if sorted(out) != sorted(names):
            raise ValueError(f"{who}: out must hold exactly the groups of rows")
        dims = dict(observation=self.obs_dim, achieved_goal=self.goal_dim, desired_goal=self.goal_dim)
        lead = tuple(rows[names[0]].shape[:-1])
        count = int(np.prod(lead)) if lead else 1
        a = _abi.NormRowsArgs()
        for k in names:
            setattr(a, k, self._float_ptr(who, f"rows[{k!r}]", rows[k], lead + (dims[k],)))
            setattr(a, k + "_out", self._float_ptr(who, f"out[{k!r}]", out[k], lead + (dims[k],)))
        _native.check(self.lib.urgym_norm_rows(self._h, C.byref(n), C.byref(a), count, self._stream()), self._h)
        return out

    def norm_batch(self, normalizer, batch):
        """Normalizes a minibatch IN PLACE in ONE launch (urgym_norm_batch): `batch` as ``DeviceReplay.sample`` returns it --
        ``observations`` and ``next_observations`` with the three observation groups (``norm_obs``), ``rewards`` with the return
        group (``norm_reward``); actions and flags are not touched.  The arithmetic is ``evaluation.normalize_rows`` /
        ``normalize_reward``, bitwise.  Returns `batch`."""
        who = "norm_batch"
        n = self._normalization(who, normalizer)
        count = int(batch["rewards"].shape[0])
        dims = dict(observation=self.obs_dim, achieved_goal=self.goal_dim, desired_goal=self.goal_dim)
        b = _abi.ReplayBatch()
        for prefix, key in (("", "observations"), ("next_", "next_observations")):
            for k in self._NORM_ROWS:
                setattr(b, prefix + k, self._float_ptr(who, f"batch[{key!r}][{k!r}]", batch[key][k], (count, dims[k])))
        b.reward = self._float_ptr(who, "batch['rewards']", batch["rewards"], (count,))
        _native.check(self.lib.urgym_norm_batch(self._h, C.byref(n), C.byref(b), count, self._stream()), self._h)
        return batch

    def collect(self, actor, num_steps, replay, sample=None, first_slot=None, normalizer=None):
        """``rollout_policy`` that files every transition in `replay` (an ``evaluation.DeviceReplay`` of this environment) as it
        happens (urgym_rollout_collect): step k goes to slot (first_slot + k) % capacity, complete with the terminal observation
        and goals of envs that were auto-reset.  `sample` as in ``rollout_policy`` (None = the deterministic policy); `first_slot`
        defaults to the ring's cursor, which this method does NOT move -- ``replay.collect`` does.  Nothing is synchronised.

        With `normalizer` (an ``evaluation.DeviceNormalizer`` of this environment) the actor reads rows normalized with the
        statistics as they stand (urgym_rollout_collect_normalized: one more launch per step); the ring still holds the RAW rows, and
        the statistics are NOT folded here -- ``normalizer.fold`` afterwards does that."""
        a = self._actor_ptr(actor)
        if normalizer is not None:
            if getattr(replay, "env", None) is not self or not hasattr(replay, "_ring"):
                raise ValueError("replay must be a DeviceReplay allocated for this environment (DeviceReplay(env, capacity_steps))")
            n = self._normalization("collect", normalizer)
            first = replay.cursor if first_slot is None else first_slot
            replay.check_args(replay.capacity, num_steps=num_steps, first_slot=first)
            how = self._sampling(sample if sample is not None else dict(mode="mean"))
            _native.check(self.lib.urgym_rollout_collect_normalized(self._h, a, C.byref(how), int(num_steps), C.byref(replay._ring), int(first), C.byref(n),
                                                                    self._stream()), self._h)
            return
        if getattr(replay, "env", None) is not self or not hasattr(replay, "_ring"):
            raise ValueError("replay must be a DeviceReplay allocated for this environment (DeviceReplay(env, capacity_steps))")
        first = replay.cursor if first_slot is None else first_slot
        replay.check_args(replay.capacity, num_steps=num_steps, first_slot=first)
        how = self._sampling(sample if sample is not None else dict(mode="mean"))
        _native.check(self.lib.urgym_rollout_collect(self._h, a, C.byref(how), int(num_steps), C.byref(replay._ring), int(first), self._stream()), self._h)

    # --------------------------------------------------------------------------------- the scripted reach controller
    @staticmethod
    def check_controller(damping=0.2, gain=0.5, seed=0, explore_sigma=0.0):
        """Raises ValueError for what urgym_controller_* refuse about the controller's scalars (include/urgym.h): damping outside
        [1e-2, 10], gain outside (0, 10], explore_sigma negative or not finite in float32, a seed that is no uint64.  Returns the four as
        (float, float, int, float).  Needs no GPU."""
        lo, hi = _abi.IK_DAMPING_RANGE
        for name, v in (("damping", damping), ("gain", gain), ("explore_sigma", explore_sigma)):
            if isinstance(v, bool) or not np.isfinite(np.float64(v)):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if not lo <= float(damping) <= hi:
            raise ValueError(f"damping must be in [{lo}, {hi}], got {damping}")
        if not 0.0 < float(gain) <= _abi.IK_GAIN_MAX:
            raise ValueError(f"gain must be in (0, {_abi.IK_GAIN_MAX}], got {gain}")
        with np.errstate(over="ignore"):
            if not (np.isfinite(np.float32(explore_sigma)) and float(explore_sigma) >= 0.0):
                raise ValueError(f"explore_sigma must be finite (in float32) and >= 0, got {explore_sigma!r}")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        return float(damping), float(gain), int(seed), float(explore_sigma)

    def _controller(self, damping, gain, seed, explore_sigma, explore_eps):
        c = _abi.ReachController(*self.check_controller(damping, gain, seed, explore_sigma), 0, None)
        if explore_eps is not None:
            if (explore_eps.dtype != torch.float32 or tuple(explore_eps.shape) != (self.num_envs, 6) or not explore_eps.is_contiguous()
                    or explore_eps.device != self.device):
                raise ValueError(f"explore_eps must be a contiguous float32 [{self.num_envs}, 6] tensor on {self.device}")
            c.explore_eps = C.cast(explore_eps.data_ptr(), C.POINTER(C.c_float))
        return c

    @staticmethod
    def _check_draw(first_draw, count):
        if isinstance(first_draw, bool) or int(first_draw) != first_draw or not (0 <= int(first_draw) and int(first_draw) + int(count) <= 1 << 32):
            raise ValueError(f"draws must stay in [0, 2^32), got {first_draw} + {count}")
        return int(first_draw)

    def controller_actions(self, out=None, draw=0, damping=0.2, gain=0.5, seed=0, explore_sigma=0.0, explore_eps=None):
        """One damped least-squares IK step toward every env's goal pose as an action (urgym_controller_actions: ONE launch that reads
        the bound ``q`` and ``goal``; ``evaluation.ik_actions`` restates it): float32 [N, 6] in `out` (allocated if None), plus
        `explore_sigma` times the exploration noise of (`seed`, `draw`), clamped, where `explore_sigma` > 0; `explore_eps` ([N, 6],
        optional) receives the noise.  Returns `out`.  NOT synchronised."""
        if out is None:
            out = torch.empty((self.num_envs, 6), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (self.num_envs, 6) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 [{self.num_envs}, 6] tensor on {self.device}")
        c = self._controller(damping, gain, seed, explore_sigma, explore_eps)
        _native.check(self.lib.urgym_controller_actions(self._h, C.byref(c), self._check_draw(draw, 1), C.c_void_p(out.data_ptr()), self._stream()), self._h)
        return out

    def controller_control(self, num_steps, first_draw=0, record=("reward", "terminated", "truncated", "is_success"), damping=0.2, gain=0.5, seed=0,
                           explore_sigma=0.0, explore_eps=None):
        """`num_steps` x (controller action, step) in ONE native call (urgym_controller_control); step t draws with ``first_draw + t``.
        `record` names what to keep, as ``rollout_policy`` does ("all" = every key); the action rows are always kept (the call writes
        them into the trajectory).  Returns a dict of fresh device tensors (flags as bool views).  NOT synchronised."""
        T = int(num_steps)
        if T < 1:
            raise ValueError(f"num_steps must be positive, got {num_steps}")
        keys = tuple(name for name, _, _ in _abi.TRAJECTORY_FIELDS)
        names = tuple(k for k in keys if k != "final_observation" or self.cfg.auto_reset) if record == "all" else tuple(record)
        unknown = [n for n in names if n not in keys]
        if unknown:
            raise ValueError(f"unknown record {unknown}; available: {keys}")
        if "final_observation" in names and not self.cfg.auto_reset:
            raise ValueError("final_observation exists only with auto_reset")
        if any(n.startswith("episode_") for n in names) and "episode_done" not in names:
            names += ("episode_done",)
        if "action" not in names:
            names += ("action",)
        c = self._controller(damping, gain, seed, explore_sigma, explore_eps)
        traj, out = _abi.Trajectory(), {}
        for name, ct, shape in _abi.TRAJECTORY_FIELDS:
            if name in names:
                t = torch.zeros(shape(T, self.num_envs, self.obs_dim, self.goal_dim), dtype=_TORCH_DTYPE[ct], device=self.device)
                setattr(traj, name, C.cast(t.data_ptr(), C.POINTER(ct)))
                out[name] = t.view(torch.bool) if ct is C.c_uint8 else t
        _native.check(self.lib.urgym_controller_control(self._h, C.byref(c), self._check_draw(first_draw, T), T, C.byref(traj), self._stream()), self._h)
        return out

    def controller_collect(self, replay, num_steps, first_draw=0, first_slot=None, damping=0.2, gain=0.5, seed=0, explore_sigma=0.0, explore_eps=None):
        """`num_steps` x (store pass, controller action, step) in ONE native call (urgym_controller_collect) that files every transition
        in `replay` (an ``evaluation.DeviceReplay`` of this environment) as it happens: step t goes to slot (first_slot + t) % capacity
        and draws with ``first_draw + t``.  `first_slot` defaults to the ring's cursor, which this method does NOT move --
        ``replay.collect_scripted`` does.  NOT synchronised."""
        if getattr(replay, "env", None) is not self or not hasattr(replay, "_ring"):
            raise ValueError("replay must be a DeviceReplay allocated for this environment (DeviceReplay(env, capacity_steps))")
        first = replay.cursor if first_slot is None else first_slot
        replay.check_args(replay.capacity, num_steps=num_steps, first_slot=first)
        c = self._controller(damping, gain, seed, explore_sigma, explore_eps)
        _native.check(self.lib.urgym_controller_collect(self._h, C.byref(c), self._check_draw(first_draw, int(num_steps)), int(num_steps), C.byref(replay._ring),
                                                        int(first), self._stream()), self._h)

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self.lib.urgym_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --------------------------------------------------------------------------------- task-level setters (a13)
    def set_goal(self, ids, goal):
        """ReachOri.set_goal (reach.py:202-204) for env ids; goal is [len(ids), 6] (xyz + rpy)."""
        ids = torch.as_tensor(ids, device=self.device).long()
        g = torch.as_tensor(goal, device=self.device, dtype=torch.float64).reshape(len(ids), -1)
        self.buf["goal"][: g.shape[1], ids] = g.T
        self._refresh(ids)

    def set_goal_and_obstacle(self, ids, data):
        """Reach{Obs,Dyn}.set_goal_and_obstacle (reach.py:328-335, 702-713).
        Obs: data = [goal xyz, obstacle xyz+rpy] (9); Dyn: [goal 6, obstacle_start 6, obstacle_end 6] (18);
        Sta: [goal 6, obstacle 6] (12) or the 18-column moving form."""
        ids = torch.as_tensor(ids, device=self.device).long()
        d = torch.as_tensor(data, device=self.device, dtype=torch.float64).reshape(len(ids), -1)
        if self.env_kind == _abi.ENV_OBS:
            assert d.shape[1] == 9
            self.buf["goal"][:3, ids] = d[:, :3].T
            self.buf["obst_start"][:, ids] = d[:, 3:9].T
        elif self.env_kind == _abi.ENV_STA:  # reach.py:484-507: 12 columns = static obstacle, 18 = start/end (moving)
            assert d.shape[1] in (12, 18)
            self.buf["goal"][:, ids] = d[:, :6].T
            self.buf["obst_start"][:, ids] = d[:, 6:12].T
            self.buf["obst_end"][:, ids] = d[:, 12:18].T if d.shape[1] == 18 else 0.0
        elif self.env_kind == _abi.ENV_DYN:
            assert d.shape[1] == 18
            self.buf["goal"][:, ids] = d[:, :6].T
            self.buf["obst_start"][:, ids] = d[:, 6:12].T
            self.buf["obst_end"][:, ids] = d[:, 12:18].T
        else:
            raise TypeError("UR5OriReach-v1 has no obstacle; use set_goal")
        self._refresh(ids)

    def _refresh(self, ids=None):
        keep, mp = self._mask_ptr(ids)
        _native.check(self.lib.urgym_refresh(self._h, mp, self._stream()), self._h)

    STATE_KEYS = ("q", "goal", "obst_start", "obst_end", "obst_pos", "obst_quat", "obst_vel", "link_dist", "step_count",
                  "episode_id")

    def get_state(self):
        """Snapshot of the per-env state tensors (SoA layout of include/urgym.h), on the host."""
        return {k: self.buf[k].detach().cpu().numpy().copy() for k in self.STATE_KEYS}

    def set_state(self, state, refresh=False):
        """Overwrite state tensors (teacher-forced parity tests). With refresh=True the observation, collision flag and
        link distances are recomputed for all envs (obstacle placed at obst_start).  `obst_vel` may be given as the full [9, N]
        snapshot of get_state() or as a [6, N] twist, in which case the per-step displacement (rows 6..8) is re-derived from it."""
        derive = False
        for k, v in state.items():
            v = np.asarray(v)
            if k == "obst_vel" and v.shape[0] == 6:
                # a twist of the caller's own (rows 0..5): rows 6..8, the displacement of one env step under it, are derived state
                self.buf[k][:6].copy_(torch.as_tensor(v, device=self.device).reshape(6, self.num_envs).to(self.buf[k].dtype))
                derive = True
                continue
            t = torch.as_tensor(v, device=self.device).reshape(self.buf[k].shape)
            self.buf[k].copy_(t.to(self.buf[k].dtype))
        if derive:
            _native.check(self.lib.urgym_derive_obstacle_motion(self._h, self._stream()), self._h)
        if "episode_id" in state or "step_count" in state:
            # the library keeps the next episodes of every env prefetched, keyed by episode id: tell it they may no longer match
            _native.check(self.lib.urgym_invalidate_records(self._h), self._h)
        if refresh:
            self._refresh(None)
        self._needs_reset = False

    def _config_dict(self):
        """The configuration as JSON scalars and lists, in the struct's order: what a checkpoint compares."""
        out = {}
        for name, _ in _abi.Config._fields_:
            v = getattr(self.cfg, name)
            out[name] = v if isinstance(v, (int, float)) else [float(x) for x in v]
        return out

    def checkpoint_state(self):
        """Everything a run needs to continue bit for bit in another environment object: EVERY bound buffer of
        ``_abi.BUFFER_FIELDS`` on the host -- the outputs and the observation as well as ``STATE_KEYS``: a reset of UR5DynReach-v1 reads
        the observation it finds, and the status words are sticky -- with ``_seed``, ``_needs_reset``, the env id, the env count and the
        configuration.  Synchronises."""
        return dict(env_id=self.env_id, num_envs=self.num_envs, config=self._config_dict(), seed=self._seed, needs_reset=bool(self._needs_reset),
                    buffers={name: self.buf[name].detach().cpu().numpy() for name, _, _ in _abi.BUFFER_FIELDS})

    def check_checkpoint(self, state):
        """Raises ValueError unless `state` is a ``checkpoint_state`` of an environment of this id, env count and configuration, naming
        the first difference.  Writes nothing."""
        if state["env_id"] != self.env_id or int(state["num_envs"]) != self.num_envs:
            raise ValueError(f"restore_checkpoint: the state is of {state['env_id']} x {state['num_envs']}, this environment is {self.env_id} x {self.num_envs}")
        mine = self._config_dict()
        for name, v in mine.items():
            if name not in state["config"] or state["config"][name] != v:
                raise ValueError(f"restore_checkpoint: config.{name} is {state['config'].get(name)!r} in the state, {v!r} here")
        for name, ct, _ in _abi.BUFFER_FIELDS:
            a = np.asarray(state["buffers"][name])
            if a.dtype != np.dtype(ct) or a.shape != tuple(self.buf[name].shape):
                raise ValueError(f"restore_checkpoint: buffers[{name!r}] must be {np.dtype(ct)} {tuple(self.buf[name].shape)}, got {a.dtype} {a.shape}")

    def restore_checkpoint(self, state):
        """Puts a ``checkpoint_state`` back into this environment (same id, env count and configuration; ValueError otherwise, before
        anything is written).  The sampler is re-keyed with the saved seed by a full urgym_reset -- made with every env's episode id
        set ONE BELOW the saved one, so that the episode records the library prefetches behind a reset (keyed by seed, env and episode
        id) are those of the saved ids: the restored environment resets its finished envs inline from valid records, exactly as the
        one the state was taken from does, and never takes the kernel fallback, whose work list is itself a bound buffer.  Then every
        bound buffer is copied back over what that reset wrote.  The steps that follow are bit for bit those of the environment the
        state was taken from, in every bound buffer.  (A state that holds an episode id of 0 on an environment that has been reset
        -- ``set_state`` can make one -- has no id below it: its records are invalidated instead, urgym_invalidate_records, and it
        continues through the fallback with the same results but for the two work-list buffers.)  ``get_state`` / ``set_state`` are
        the teacher-forcing pair and stay as they are."""
        self.check_checkpoint(state)
        seed, fresh = int(state["seed"]), bool(state["needs_reset"])
        ids = np.asarray(state["buffers"]["episode_id"])
        if not fresh:
            self.buf["episode_id"].copy_(torch.from_numpy(np.maximum(ids - 1, 0).astype(ids.dtype)))
            _native.check(self.lib.urgym_reset(self._h, None, C.c_uint64(seed), self._stream()), self._h)
        for name, _, _ in _abi.BUFFER_FIELDS:
            self.buf[name].copy_(torch.from_numpy(np.ascontiguousarray(state["buffers"][name])))
        if not fresh and (ids < 1).any():
            _native.check(self.lib.urgym_invalidate_records(self._h), self._h)
        self._seed, self._needs_reset = seed, fresh

    def probe_closest(self, type_a, par_a, pose_a, type_b, par_b, pose_b, threshold=5.0):
        """Unit probe of the device closest-distance routine (urgym_probe_closest): arrays of queries -> (dist, info)."""
        dev = self.device
        ta = torch.as_tensor(np.asarray(type_a, np.int32), device=dev)
        tb = torch.as_tensor(np.asarray(type_b, np.int32), device=dev)
        n = ta.numel()
        pa = torch.as_tensor(np.asarray(par_a, np.float64).reshape(n, 3), device=dev).contiguous()
        pb = torch.as_tensor(np.asarray(par_b, np.float64).reshape(n, 3), device=dev).contiguous()
        xa = torch.as_tensor(np.asarray(pose_a, np.float64).reshape(n, 7), device=dev).contiguous()
        xb = torch.as_tensor(np.asarray(pose_b, np.float64).reshape(n, 7), device=dev).contiguous()
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        info = torch.zeros(n, dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        _native.check(self.lib.urgym_probe_closest(self._h, n, p(ta), p(pa), p(xa), p(tb), p(pb), p(xb), float(threshold), p(out), p(info),
                                                  self._stream()), self._h)
        return out.cpu().numpy(), info.cpu().numpy()

    def probe_pose_distance(self, a6, b6):
        """Unit probe of the device utils.distance / utils.angular_distance (urgym_probe_pose_distance): [n, 6] poses -> [n, 2]."""
        a = torch.as_tensor(np.asarray(a6, np.float64).reshape(-1, 6), device=self.device).contiguous()
        b = torch.as_tensor(np.asarray(b6, np.float64).reshape(-1, 6), device=self.device).contiguous()
        out = torch.zeros((a.shape[0], 2), dtype=torch.float64, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        _native.check(self.lib.urgym_probe_pose_distance(self._h, a.shape[0], p(a), p(b), p(out), self._stream()), self._h)
        return out.cpu().numpy()

    # ------------------------------------------------------------------------------------------------ timing
    def enable_timing(self, on=True, every=1):
        """HIP events around the step launch; every=k times each k-th step only (a pair of events costs the stream ~6 us)."""
        _native.check(self.lib.urgym_enable_timing(self._h, (max(1, int(every)) if on else 0)), self._h)

    def query_timing(self):
        """(avg step-kernel us, avg reset-kernel us, #step launches) since the last query — HIP events on the launch stream."""
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        _native.check(self.lib.urgym_query_timing(self._h, C.byref(a), C.byref(b), C.byref(n)), self._h)
        r = C.c_double()
        _native.check(self.lib.urgym_query_refill_timing(self._h, C.byref(r)), self._h)
        self.last_refill_us = r.value  # overlapped refill of prefetched episode records (0 when that path is off)
        return a.value, b.value, n.value


class SacLearnerBinding:
    """What ``UR5ReachVectorEnv.sac_learner`` returns: the checked ``urgym_sac_learner`` (``struct``) and references to every tensor
    and object it points to, so that none is freed while a call that reads it may still be queued."""

    def __init__(self, env, struct, keep, actor, actor_params=None):
        self.env, self.struct, self.keep, self.actor, self.actor_params = env, struct, keep, actor, actor_params


class _LazyInfo(dict):
    """info dict whose derived entries are computed on first access: a `step()` that nobody inspects launches no extra kernel."""

    def __init__(self, base, lazy):
        super().__init__(base)
        self._lazy = dict(lazy)

    def _materialise(self):
        for k in list(self._lazy):
            dict.__setitem__(self, k, self._lazy.pop(k)())

    def __missing__(self, key):
        if key in self._lazy:
            value = self._lazy.pop(key)()
            dict.__setitem__(self, key, value)
            return value
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._lazy

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        self._materialise()
        return dict.keys(self)

    def items(self):
        self._materialise()
        return dict.items(self)

    def values(self):
        self._materialise()
        return dict.values(self)

    def __iter__(self):
        self._materialise()
        return dict.__iter__(self)

    def __len__(self):
        return dict.__len__(self) + len(self._lazy)


def make_vec(env_id, num_envs=1, **kwargs):
    """Counterpart of ``gymnasium.make(id)`` for the ids the reference registers (UR_gym/__init__.py:19-42)."""
    return UR5ReachVectorEnv(env_id, num_envs=num_envs, **kwargs)
