"""Closed-loop evaluation harness: counterpart of the reference's ``model_test.py:26-61`` + ``utils/generate.py:23-102``.

The reference evaluates a trained SAC actor by (1) generating test points per env (a goal grid with sampled
orientations / obstacles, or plain resets), (2) ``env.reset(); env.task.set_goal[_and_obstacle](point)``, (3) rolling
the deterministic policy for at most 100 steps and recording episode reward, ``info['is_success']`` and the index of
the last step.  Here all trials run in parallel — one environment per trial — on either backend that offers the
VectorEnv verbs (the HIP environment of this package, or, in tests, the CPU oracle through a thin adapter).

The actor is re-implemented from the checkpoint's tensors (SB3 ``MultiInputPolicy``: features = concat of the Dict
observation in sorted key order achieved_goal | desired_goal | observation; ``latent_pi`` = Linear-ReLU-Linear-ReLU;
``mu`` = Linear; deterministic action = tanh(mu)); stable-baselines3 itself is not needed.

Two forms of the same loop: ``run_closed_loop`` with ``DeterministicActor`` (numpy, on the host: works on any backend, the CPU
oracle included) and ``run_closed_loop_device`` with ``DeviceActor`` (the HIP actor kernel: observations, actions and the
bookkeeping of model_test.py:38-50 stay on the GPU for the whole episode).
"""
import numpy as np


class DeterministicActor:
    """tanh(mu(latent_pi(x))) from the arrays exported by tests/golden/gen_actor_fixtures.py (or any SB3 SAC policy.pth)."""

    def __init__(self, weights):
        self.w = {k: np.asarray(v, dtype=np.float32) for k, v in dict(weights).items()}
        self.in_features = self.w["latent_pi_0_weight"].shape[1]

    @classmethod
    def load(cls, npz_path):
        return cls(np.load(npz_path))

    def __call__(self, achieved_goal, desired_goal, observation):
        x = np.concatenate([achieved_goal, desired_goal, observation], axis=1).astype(np.float32)
        assert x.shape[1] == self.in_features, (x.shape, self.in_features)
        h = np.maximum(x @ self.w["latent_pi_0_weight"].T + self.w["latent_pi_0_bias"], 0.0)
        h = np.maximum(h @ self.w["latent_pi_2_weight"].T + self.w["latent_pi_2_bias"], 0.0)
        return np.tanh(h @ self.w["mu_weight"].T + self.w["mu_bias"]).astype(np.float32)


def philox4x32_10(key, counter):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy: key = (k0, k1) ints, counter = four uint32 arrays (broadcast together).
    Returns the four output words as uint32 arrays.  The function of ur_gym_amd/csrc/urgym_philox.h."""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & mask for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]  # 32 x 32 bits: fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def policy_noise(seed, draw, env_ids, mode, dtype=np.float32):
    """The noise of the device's sampled policy, restated from include/urgym.h ("the stochastic half"): a pure function of
    (seed, draw, env, component).  `draw` and `env_ids` are integers or integer arrays that broadcast together; returns their
    shape + (6,): eps ~ N(0, 1) for mode "gaussian", u in [0, 1) for "uniform" (the action is 2 u - 1), zeros for "mean".
    `dtype` is the precision of ln / sqrt / cos / sin; the words and the uniforms are exact in either."""
    from . import _abi

    mode = _abi.SAMPLE_MODES.get(mode, mode)
    env, draw = np.broadcast_arrays(np.asarray(env_ids, dtype=np.uint64), np.asarray(draw, dtype=np.uint64))
    if mode == _abi.SAMPLE_MEAN:
        return np.zeros(env.shape + (6,), dtype)
    if mode not in (_abi.SAMPLE_GAUSSIAN, _abi.SAMPLE_UNIFORM):
        raise ValueError(f"unknown sampling mode {mode!r}")
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    lo, hi = draw & np.uint64(0xFFFFFFFF), draw >> np.uint64(32)
    a = philox4x32_10(key, (env, lo, hi, np.uint64(_abi.NOISE_TAG | 0)))
    b = philox4x32_10(key, (env, lo, hi, np.uint64(_abi.NOISE_TAG | 1)))
    m = _noise_integers(a, b, dtype)
    if mode == _abi.SAMPLE_UNIFORM:
        return m * dtype(2.0 ** -24)
    return _box_muller(m, dtype)


def _noise_integers(a, b, dtype):
    """The six 24-bit integers m(w) = w >> 8 of the words w0 .. w3 of block 0 (`a`) and w4, w5 of block 1 (`b`), exact in `dtype`."""
    return np.stack([w >> np.uint32(8) for w in (a[0], a[1], a[2], a[3], b[0], b[1])], axis=-1).astype(dtype)


def _box_muller(m, dtype):
    """Box-Muller on the pairs of `m` (shape + (6,) integers below 2^24) as include/urgym.h states it for the GAUSSIAN policy noise."""
    scale = dtype(2.0 ** -24)
    u1, u2 = (m[..., 0::2] + dtype(1)) * scale, m[..., 1::2] * scale  # (0, 1], [0, 1)
    r, angle = np.sqrt(dtype(-2) * np.log(u1)), dtype(2 * np.pi) * u2
    out = np.empty_like(m)
    out[..., 0::2], out[..., 1::2] = r * np.cos(angle), r * np.sin(angle)
    return out


def replay_indices(seed, draw, count, size):
    """The ring entries urgym_replay_sample draws, restated from include/urgym.h ("the replay buffer"): e_i for i < count, a pure
    function of (seed, draw, i, size) -- e = (w * size) >> 64 with w = (w0 << 32) | w1 of Philox4x32-10 at the counter
    (i, draw lo, draw hi, REPLAY_TAG).  The 128-bit product is taken in Python integers.  Returns int64 [count], each in [0, size);
    the caller maps e to slot (oldest_slot + e // N) % C and env e % N."""
    from . import _abi

    seed, draw, count, size = int(seed), int(draw), int(count), int(size)
    if count < 0 or not 0 < size < 1 << 63:
        raise ValueError(f"count must be >= 0 and size in [1, 2^63), got {count}, {size}")
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10(key, (np.arange(count, dtype=np.uint64), np.uint64(draw & 0xFFFFFFFF), np.uint64((draw >> 32) & 0xFFFFFFFF),
                            np.uint64(_abi.REPLAY_TAG)))
    return np.array([((int(hi) << 32 | int(lo)) * size) >> 64 for hi, lo in zip(w[0], w[1])], dtype=np.int64).reshape(count)


def mixed_indices(seed, draw, count, size, demo_count, demo_size):
    """The entries urgym_replay_sample_mixed draws, restated from include/urgym.h ("the demonstration ring"): int64 [count].  Row i <
    `demo_count` holds e = (w * demo_size) >> 64 with w of the Philox call at the counter (i, draw lo, draw hi, DEMO_TAG), an entry number
    of the DEMONSTRATION ring's `demo_size` = filled_d * N_d entries; row i >= `demo_count` holds ``replay_indices``' row i.  A function
    of (seed, draw, i, size, demo_size) alone.  The caller maps e to slot and env with the numbers of the row's own ring; ``source`` is
    ``arange(count) < demo_count``.  With ``demo_count == 0`` `demo_size` is not looked at beyond its range."""
    from . import _abi

    seed, draw, count, size, D, size_d = int(seed), int(draw), int(count), int(size), int(demo_count), int(demo_size)
    if not 0 <= D <= count:
        raise ValueError(f"demo_count must be in [0, count], got {D} of {count}")
    if not 0 < size_d < 1 << 63:
        raise ValueError(f"demo_size must be in [1, 2^63), got {size_d}")
    out = replay_indices(seed, draw, count, size)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10(key, (np.arange(D, dtype=np.uint64), np.uint64(draw & 0xFFFFFFFF), np.uint64((draw >> 32) & 0xFFFFFFFF), np.uint64(_abi.DEMO_TAG)))
    out[:D] = np.array([((int(hi) << 32 | int(lo)) * size_d) >> 64 for hi, lo in zip(w[0], w[1])], dtype=np.int64).reshape(D)
    return out


def mixed_entries(seed, draw, count, own, demo_count, demo):
    """``mixed_indices`` mapped to flat ring entries: `own` and `demo` are (oldest_slot, filled_steps, num_envs, capacity_steps) of the
    learner's ring and of the demonstration ring.  Returns (index int64 [count], source bool [count]): index = slot * N + env in the
    row's own ring, slot = (oldest_slot + e // N) % C, env = e % N."""
    e = mixed_indices(seed, draw, count, own[1] * own[2], demo_count, demo[1] * demo[2])
    source = np.arange(int(count)) < int(demo_count)
    index = np.empty(int(count), dtype=np.int64)
    for mask, (oldest, _, n, cap) in ((source, demo), (~source, own)):
        index[mask] = ((oldest + e[mask] // n) % cap) * n + e[mask] % n
    return index, source


def training_schedule(*, first_slot, filled_steps, capacity_steps, num_iterations, steps_per_iteration=1, updates_per_iteration=1,
                      uniform_iterations=0, idle_iterations=0, collect_first_draw=0, update_first_draw=0, first_step=1):
    """The index arithmetic of one urgym_sac_train call, restated from include/urgym.h (``urgym_sac_schedule``) and
    ur_gym_amd/csrc/urgym_sac_schedule.h in Python integers.  Returns a dict: ``iterations``, one dict per iteration
    (``collect_first_slot``, ``collect_first_draw``, ``collect_mode`` as the URGYM_SAMPLE_* number, ``idle``, and the ring view of its
    updates after its collection, ``oldest_slot`` and ``filled_steps``, and ``first_update``); ``updates``, one dict per update of the
    whole call (``gather_draw``, ``policy_draw`` = the same | 2^63, ``adam_step``, ``loss_slot``, and the ``iteration`` it runs in);
    ``num_updates``; and ``cursor`` and ``filled``, the ring afterwards.  Draws are taken modulo 2^64 like the uint64 they are.
    Raises ValueError for what the header's validation refuses.  Needs no GPU."""
    from . import _abi

    names = ("first_slot", "filled_steps", "capacity_steps", "num_iterations", "steps_per_iteration", "updates_per_iteration",
             "uniform_iterations", "idle_iterations", "collect_first_draw", "update_first_draw", "first_step")
    given = (first_slot, filled_steps, capacity_steps, num_iterations, steps_per_iteration, updates_per_iteration, uniform_iterations,
             idle_iterations, collect_first_draw, update_first_draw, first_step)
    for name, v in zip(names, given):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    slot, filled, C, n, K, G, U, I, cdraw, udraw, step = (int(v) for v in given)
    for name, v in zip(names[:8], (slot, filled, C, n, K, G, U, I)):
        if not -(1 << 31) <= v < 1 << 31:
            raise ValueError(f"{name} must fit int32, got {v}")
    if not (0 <= cdraw < 1 << 64 and 0 <= udraw < 1 << 64 and -(1 << 63) <= step < 1 << 63):
        raise ValueError("collect_first_draw and update_first_draw must fit uint64, first_step int64")
    active = max(0, n - I)
    num_updates = active * G
    if C <= 0:
        raise ValueError("capacity_steps must be positive")
    if n < 1:
        raise ValueError("num_iterations must be at least 1")
    if K < 0 or G < 0 or U < 0 or I < 0:
        raise ValueError("a count of the schedule is negative (steps_per_iteration, updates_per_iteration, uniform_iterations, idle_iterations)")
    if K == 0 and G == 0:
        raise ValueError("steps_per_iteration and updates_per_iteration are both 0")
    if not 0 <= slot < C:
        raise ValueError(f"first_slot must be in [0, {C}), got {slot}")
    if not 0 <= filled <= C:
        raise ValueError(f"filled_steps must be in [0, {C}], got {filled}")
    if num_updates > 0 and filled == 0 and K == 0:
        raise ValueError("an update would see an empty ring (filled_steps and steps_per_iteration are both 0)")
    if step < 1:
        raise ValueError(f"first_step is the 1-based index of the first Adam step, got {step}")
    if udraw + num_updates > 1 << 63:
        raise ValueError("update_first_draw + the number of updates is above 2^63 (the top bit marks the policy's own draw)")
    if step + num_updates > (1 << 63) - 1:
        raise ValueError("first_step + the number of updates does not fit int64")

    def ring(iterations):
        cursor, have = (slot + iterations * K) % C, min(C, filled + iterations * K)
        return cursor, have, (cursor - have) % C

    iterations, updates = [], []
    for i in range(n):
        _, have, oldest = ring(i + 1)
        iterations.append(dict(collect_first_slot=ring(i)[0], collect_first_draw=(cdraw + i * K) % (1 << 64),
                               collect_mode=_abi.SAMPLE_UNIFORM if i < U else _abi.SAMPLE_GAUSSIAN, idle=int(i < I), oldest_slot=oldest,
                               filled_steps=have, first_update=max(0, i - I) * G))
        if i >= I:
            for _ in range(G):
                u = len(updates)
                updates.append(dict(gather_draw=udraw + u, policy_draw=(udraw + u) | 1 << 63, adam_step=step + u, loss_slot=u, iteration=i))
    cursor, have, _ = ring(n)
    return dict(iterations=iterations, updates=updates, num_updates=num_updates, cursor=cursor, filled=have)


def warmup_iterations(env_steps, num_envs, learning_starts, iterations, steps_per_iteration):
    """(U, I) of ``training_schedule`` as SAC's warm-up decides them: iteration i starts at ``env_steps + i K`` steps per env;
    it collects with uniform actions while ``steps * num_envs < learning_starts`` at its start (``SACLearner.collect``'s rule) and
    runs no update while that still holds after its collection (the loop of tools/train_sac.py).  Both are prefixes of the call, so
    each is a count; I <= U where K > 0."""
    e, N, n, K = int(env_steps), int(num_envs), int(iterations), int(steps_per_iteration)

    def leading(offset):  # the iterations i < n, counted from 0, with (e + (i + offset) K) N < learning_starts
        if not (e + offset * K) * N < learning_starts:
            return 0
        if K == 0:
            return n
        i = min(n, max(0, int((learning_starts / N - e) // K) - offset - 1))  # a first guess from below, then the rule itself
        while i > 0 and not (e + (i - 1 + offset) * K) * N < learning_starts:
            i -= 1
        while i < n and (e + (i + offset) * K) * N < learning_starts:
            i += 1
        return i

    return leading(0), leading(1)


def polyak(old, src, tau):
    """The blend of urgym_critic_load, restated from include/urgym.h in numpy float32: ``src`` at tau == 1 (the old value is not
    read), otherwise ``(old * omt) + (tau * src)`` with ``omt = float32(1) - float32(tau)``, three operations each rounded to
    float32 on its own -- not the fused ``old + tau (src - old)``.  `old` and `src` are arrays of one shape (packed buffers:
    ``DeviceCritic.packed()``); padding that is +0 in both stays +0."""
    f = np.float32
    tau = f(tau)
    if not (np.isfinite(tau) and f(0) < tau <= f(1)):
        raise ValueError(f"tau must be in (0, 1], got {tau}")
    old, src = np.asarray(old, dtype=f), np.asarray(src, dtype=f)
    if old.shape != src.shape:
        raise ValueError(f"old and src must have one shape, got {old.shape} and {src.shape}")
    if tau == f(1):
        return src.copy()
    omt = f(1) - tau
    return ((old * omt).astype(f) + (tau * src).astype(f)).astype(f)


def adam_coefficients(env, lr, betas=(0.9, 0.999), eps=1e-8, step=1):
    """The seven float32 coefficients of one Adam step as the LIBRARY forms them (urgym_adam_coefficients: host only, no launch), a
    float32 array in the order of ``_abi.ADAM_COEFFICIENTS``: b1, omb1, b2, omb2, step_size = lr / (1 - beta1^step), bc2_sqrt =
    sqrt(1 - beta2^step), eps.  The step kernels use these very numbers, so ``adam_step`` with them is bitwise the device's step
    whatever ``pow`` the host has.  `env`: an environment (its library is used) or None (the library is loaded); `step` is 1-based.
    Raises ``NativeError`` for what the library refuses (lr, betas, eps, step out of range)."""
    import ctypes as C

    from . import _abi, _native

    lib = env.lib if env is not None else _native.lib()
    hp = _abi.AdamHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), int(step), 0)
    out = (C.c_float * 7)()
    _native.check(lib.urgym_adam_coefficients(C.byref(hp), out), None)
    return np.array(out[:], dtype=np.float32)


def adam_step(p, g, m, v, coef, scale=None):
    """The per-element arithmetic of urgym_actor_adam_step / urgym_critic_adam_step, restated from include/urgym.h in numpy float32:
    returns (p', m', v').  `coef`: the seven numbers of ``adam_coefficients``.  Every line is one operation rounded to float32 on its
    own (numpy's float32 sqrt and division are the correctly rounded ones, and subnormals are kept)::

        m' = (b1 * m) + (omb1 * g)
        gg = g * g          v' = (b2 * v) + (omb2 * gg)
        s  = sqrt(v')       d  = (s / bc2_sqrt) + eps
        u  = m' / d         p' = p - (step_size * u)

    With `scale` (a float32 scalar: ``grad_norm(...)["scale"]``) it is the element of urgym_*_adam_step_scaled: ``gs = g * scale``
    first, one float32 multiply rounded on its own, then the lines above on gs.  ``None`` is exactly the step without it.
    """
    f = np.float32
    coef = np.asarray(coef)
    if coef.dtype != f or coef.shape != (7,):
        raise ValueError(f"coef must be the float32 [7] of adam_coefficients, got {coef.dtype} {coef.shape}")
    b1, omb1, b2, omb2, step_size, bc2_sqrt, eps = coef
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    if not (p.shape == g.shape == m.shape == v.shape):
        raise ValueError(f"p, g, m, v must have one shape, got {p.shape}, {g.shape}, {m.shape}, {v.shape}")
    if scale is not None:
        scale = np.asarray(scale)
        if scale.dtype != f or scale.size != 1:
            raise ValueError(f"scale must be one float32 (grad_norm's), got {scale.dtype} {scale.shape}")
        with np.errstate(all="ignore"):
            g = g * scale.reshape(())
        assert g.dtype == f, g.dtype
    with np.errstate(all="ignore"):  # underflow of g * g, overflow and NaN are inputs the step is defined on
        m_old = b1 * m
        m_in = omb1 * g
        m_new = m_old + m_in
        gg = g * g
        v_old = b2 * v
        v_in = omb2 * gg
        v_new = v_old + v_in
        s = np.sqrt(v_new)
        r = s / bc2_sqrt
        d = r + eps
        u = m_new / d
        w = step_size * u
        p_new = p - w
    for x in (m_old, m_in, m_new, gg, v_old, v_in, v_new, s, r, d, u, w, p_new):
        assert x.dtype == f, x.dtype  # no intermediate was promoted
    return p_new, m_new, v_new


def ordered_sum(terms, dtype=np.float32):
    """THE ORDERED SUM of include/urgym.h ("SAC's entropy coefficient on the device") in numpy: `terms` is a float32 [count] array;
    lane t of 1024 starts at +0.0 and adds terms t, t + 1024, ... in ascending order in float64, then the partials are folded with
    ``partial[t] += partial[t + s]`` for s = 512, ..., 1.  Returns the float64 sum; the order depends on nothing but count.
    ``dtype=np.float64`` takes float64 terms instead (the evaluation statistics' returns): the same lanes, the same order."""
    from ._abi import SAC_TERMS_LANES as L

    terms = np.asarray(terms)
    if terms.dtype != np.dtype(dtype) or np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)) or terms.ndim != 1:
        raise ValueError(f"terms must be a {np.dtype(dtype)} [count] array, got {terms.dtype} {terms.shape}")
    partial = np.zeros(L, np.float64)
    with np.errstate(all="ignore"):
        for first in range(0, terms.size, L):  # every lane's next term, ascending
            row = terms[first:first + L]
            partial[:row.size] += row.astype(np.float64)
        s = L // 2
        while s >= 1:
            partial[:s] += partial[s:2 * s]
            s //= 2
    return np.float64(partial[0])


def grad_group(tensors):
    """The gradient tensors of one optimiser as the flat float32 arrays of urgym_*_grad_norm's group, in its FIXED order: a dict under
    ACTOR_ARRAYS + LOG_STD_ARRAYS (the actor's eight), a list of two dicts under CRITIC_ARRAYS (both Q-networks, network 0 first: one
    group), or a sequence of arrays taken in the order given.  torch tensors are copied to the host."""
    def host(x):
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        if x.dtype != np.float32:
            raise ValueError(f"gradient tensors must be float32, got {x.dtype}")
        return np.ascontiguousarray(x).reshape(-1)

    if isinstance(tensors, dict):
        return [host(tensors[k]) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS]
    tensors = list(tensors)
    if tensors and all(isinstance(w, dict) for w in tensors):
        if len(tensors) != 2:
            raise ValueError(f"the critics' group is two networks, got {len(tensors)}")
        return [host(w[k]) for w in tensors for k in CRITIC_ARRAYS]
    return [host(x) for x in tensors]


def grad_norm(tensors, max_norm):
    """urgym_actor_grad_norm / urgym_critic_grad_norm restated from include/urgym.h in numpy.  `tensors`: what ``grad_group`` takes.
    Returns a dict: ``tensor_sums`` (float64 [k]: per tensor THE ORDERED SUM, ``ordered_sum(..., dtype=np.float64)``, of the exact
    float64 squares of its flat elements), ``total`` (float64: ((s_0 + s_1) + s_2) + ..., tensor order), ``norm64`` =
    sqrt(total) (numpy's float64 sqrt is the correctly rounded one), ``scale`` (float32: c64 = max_norm / (norm64 + 1e-6) rounded to
    float32 where c64 < 1, else 1 -- so a NaN norm gives 1) and ``norm`` (float32 of norm64, for the record).  `max_norm` is taken as
    the float32 the library is handed."""
    from ._abi import GRAD_NORM_EPS

    group = grad_group(tensors)
    with np.errstate(over="ignore"):
        max32 = np.float32(max_norm)
    if not (np.isfinite(max32) and max32 > 0):
        raise ValueError(f"max_norm must be finite and positive in float32, got {max_norm!r}")
    with np.errstate(all="ignore"):
        sums = np.array([ordered_sum(g.astype(np.float64) * g.astype(np.float64), dtype=np.float64) for g in group], dtype=np.float64)
        total = np.float64(sums[0])
        for s_k in sums[1:]:
            total = np.float64(total + s_k)
        norm64 = np.sqrt(total)
        c64 = np.float64(max32) / np.float64(norm64 + np.float64(GRAD_NORM_EPS))
        scale = np.float32(c64) if c64 < 1.0 else np.float32(1.0)
        norm = np.float32(norm64)
    return dict(tensor_sums=sums, total=total, norm64=norm64, norm=norm, scale=scale)


def _ordered_mean(terms):
    assert terms.dtype == np.float32, terms.dtype
    with np.errstate(all="ignore"):
        return np.float32(ordered_sum(terms) / np.float64(terms.size))  # rounded once


def _rows32(name, x, shape):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.shape != shape:
        raise ValueError(f"{name} must be a float32 array of shape {shape}, got {x.dtype} {x.shape}")
    return x


def entropy_step(alpha, log_prob, target_entropy, l, m, v, coef, *, target=None, next_log_prob=None, terminated=None, gamma=None, scale=None):
    """urgym_sac_entropy_step restated from include/urgym.h in numpy: float32 with one operation per line, the mean by
    ``ordered_sum``, the step by ``adam_step`` with `coef` = ``adam_coefficients(...)``.  `alpha` is an INPUT -- the float32 the launch
    wrote to ``ent_coef_out`` -- because the device's expf and numpy's exp are different functions.  `l`, `m`, `v`: the state before
    the step (float32, one element each).  Returns a dict: ``l``, ``m``, ``v`` (float32 [1] each, after the step), ``loss``, ``mean``
    (float32), and ``y`` [count] where the target group (`target`, `next_log_prob`, `gamma`; `terminated` or None) is given,
    ``d_log_prob`` [count] where `scale` is."""
    f = np.float32
    alpha, te = f(alpha), f(target_entropy)
    log_prob = np.asarray(log_prob)
    if log_prob.dtype != f or log_prob.ndim != 1 or not 1 <= log_prob.size:
        raise ValueError(f"log_prob must be a float32 [count] array, got {log_prob.dtype} {log_prob.shape}")
    count = log_prob.size
    l, m, v = (np.asarray(x, dtype=f).reshape(1) for x in (l, m, v))
    group = [x is not None for x in (target, next_log_prob, gamma)]
    if any(group) != all(group) or (terminated is not None and not all(group)):
        raise ValueError("the target group is half given: target, next_log_prob and gamma go together (terminated only with them)")
    out, checked = {}, []
    with np.errstate(all="ignore"):  # NaN and overflow are inputs the step is defined on
        if all(group):
            target, next_log_prob = _rows32("target", target, (count,)), _rows32("next_log_prob", next_log_prob, (count,))
            nd = np.ones(count, f) if terminated is None else np.where(np.asarray(terminated).reshape(count).astype(bool), f(0), f(1))
            d = f(gamma) * nd
            t = d * alpha
            e = t * next_log_prob
            out["y"] = target - e
            checked += [nd, d, t, e, out["y"]]
        if scale is not None:
            up = alpha * f(scale)
            out["d_log_prob"] = np.full(count, up, f)
            checked += [up, out["d_log_prob"]]
        s = log_prob + te
        mean = _ordered_mean(s)
        g = -mean
        lm = l * mean
        loss = -lm
        checked += [s, mean, g, lm, loss]
    for x in checked:
        assert x.dtype == f, x.dtype  # no intermediate was promoted
    out["l"], out["m"], out["v"] = adam_step(l, np.full(1, g, f), m, v, coef)
    out["loss"], out["mean"] = loss[0], mean
    return out


def entropy_step_nstep(alpha, log_prob, target_entropy, l, m, v, coef, *, reward=None, q_min_next=None, discount=None, next_log_prob=None,
                       terminated=None, scale=None):
    """urgym_sac_entropy_step_nstep restated from include/urgym.h in numpy: ``entropy_step`` with the target group of a per-row
    discount -- `reward` (the multi-step return), `q_min_next`, `discount`, `next_log_prob`, float32 [count] each and given
    together; `terminated` or None.  ``y = (reward + (discount nd) q_min_next) - ((discount nd) alpha) next_log_prob``, float32 with
    one operation per line.  Everything else, and the returned dict, as ``entropy_step``."""
    f = np.float32
    out = entropy_step(alpha, log_prob, target_entropy, l, m, v, coef, scale=scale)
    group = [x is not None for x in (reward, q_min_next, discount, next_log_prob)]
    if any(group) != all(group) or (terminated is not None and not all(group)):
        raise ValueError("the target group is half given: reward, q_min_next, discount and next_log_prob go together (terminated only with them)")
    if all(group):
        count, alpha = np.asarray(log_prob).size, f(alpha)
        reward, q_min_next, discount, next_log_prob = (_rows32(name, x, (count,)) for name, x in (
            ("reward", reward), ("q_min_next", q_min_next), ("discount", discount), ("next_log_prob", next_log_prob)))
        with np.errstate(all="ignore"):  # NaN and overflow are inputs the step is defined on
            nd = np.ones(count, f) if terminated is None else np.where(np.asarray(terminated).reshape(count).astype(bool), f(0), f(1))
            d = discount * nd
            a = d * q_min_next
            tv = reward + a
            t = d * alpha
            e = t * next_log_prob
            out["y"] = tv - e
        for x in (nd, d, a, tv, t, e, out["y"]):
            assert x.dtype == f, x.dtype  # no intermediate was promoted
    return out


def nstep_batch(ring_arrays, oldest_slot, filled, seed, draw, count, n_steps, gamma):
    """urgym_replay_sample_nstep restated from include/urgym.h in numpy float32, on ``replay_indices``.  `ring_arrays`: the ring's
    fields as host arrays [C, N, ...] (``truncated`` and ``is_success`` may be absent; ``truncated`` is needed for `n_steps` > 1);
    `filled` valid slots from `oldest_slot` on.  For row i with e = replay_indices(...)[i]: p = e // N, env = e % N, L = min(n_steps,
    filled - p), entry_k = ((oldest_slot + p + k) % C) N + env, m = the first k + 1 at which terminated | truncated, else L; R =
    reward[entry_0], g = gamma, then for k = 1 .. m - 1: t = g reward[entry_k], R = R + t, g = g gamma, each rounded to float32.
    Returns a dict: every ring field present [count, ...] -- ``reward`` = R; the s rows and ``action`` from entry_0; the ``next_*``
    rows and the flags from entry_{m-1} -- and ``index`` (entry_0), ``last_index`` (entry_{m-1}), both int64, ``steps`` (m, int32) and
    ``discount`` (g = gamma^m, float32)."""
    f = np.float32
    n_steps, oldest_slot, filled, count = int(n_steps), int(oldest_slot), int(filled), int(count)
    from . import _abi

    if not 1 <= n_steps <= _abi.REPLAY_NSTEP_MAX:
        raise ValueError(f"n_steps must be in [1, {_abi.REPLAY_NSTEP_MAX}], got {n_steps}")
    if not np.isfinite(f(gamma)):
        raise ValueError(f"gamma must be finite in float32, got {gamma}")
    reward = np.asarray(ring_arrays["reward"])
    if reward.dtype != f or reward.ndim != 2:
        raise ValueError(f"ring_arrays['reward'] must be float32 [C, N], got {reward.dtype} {reward.shape}")
    cap, N = reward.shape
    if not (1 <= filled <= cap and 0 <= oldest_slot < cap):
        raise ValueError(f"filled must be in [1, {cap}] and oldest_slot in [0, {cap}), got {filled}, {oldest_slot}")
    truncated = ring_arrays.get("truncated")
    if truncated is None and n_steps > 1:
        raise ValueError("n_steps > 1 needs the ring's truncated (an episode's end at the time limit could not be seen)")
    flat = lambda a: np.asarray(a).reshape(cap * N, *np.asarray(a).shape[2:])  # noqa: E731
    ends = flat(ring_arrays["terminated"]) != 0
    if truncated is not None:
        ends = ends | (flat(truncated) != 0)
    e = replay_indices(seed, draw, count, filled * N)
    p, env = e // N, e % N
    L = np.minimum(n_steps, filled - p)
    gamma = f(gamma)
    R, g = np.zeros(count, f), np.full(count, gamma, f)
    m, first, last, running = np.zeros(count, np.int32), np.zeros(count, np.int64), np.zeros(count, np.int64), np.ones(count, bool)
    with np.errstate(all="ignore"):  # NaN and overflow are values a reward may hold
        for k in range(n_steps):
            take = running & (k < L)
            entry = np.where(take, ((oldest_slot + p + k) % cap) * N + env, 0)  # rows that take no step k read nothing of it
            r = flat(reward)[entry]
            if k == 0:
                R, first = r.copy(), entry.copy()
            else:
                t = g * r
                R_next = R + t
                g_next = g * gamma
                assert t.dtype == f and R_next.dtype == f and g_next.dtype == f  # no intermediate was promoted
                R, g = np.where(take, R_next, R), np.where(take, g_next, g)
            m, last = np.where(take, np.int32(k + 1), m), np.where(take, entry, last)
            running = running & ~(take & ends[entry])
    out = {"reward": R, "discount": g, "steps": m, "index": first, "last_index": last}
    for name in ("observation", "achieved_goal", "desired_goal", "action"):
        out[name] = flat(ring_arrays[name])[first]
    for name in ("next_observation", "next_achieved_goal", "next_desired_goal", "terminated", "truncated", "is_success"):
        if ring_arrays.get(name) is not None:
            out[name] = flat(ring_arrays[name])[last]
    return out


def relabel_threshold(n_sampled_goal):
    """The relabel threshold of urgym_replay_sample_hindsight for SB3's ``n_sampled_goal``, formed with integers:
    (n_sampled_goal << 32) // (n_sampled_goal + 1), i.e. a share n / (n + 1) of the rows (4 -> 0.8).  0 relabels nothing."""
    n = n_sampled_goal
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) < 1 << 31:
        raise ValueError(f"n_sampled_goal must be a non-negative integer, got {n_sampled_goal!r}")
    return (int(n) << 32) // (int(n) + 1)


def _her_arguments(threshold, strategy, horizon):
    from . import _abi

    strategy = _abi.HER_STRATEGIES.get(strategy, strategy)
    if isinstance(threshold, bool) or int(threshold) != threshold or not 0 <= int(threshold) <= 1 << 32:
        raise ValueError(f"the relabel threshold must be an integer in [0, 2^32], got {threshold!r}")
    if isinstance(strategy, bool) or strategy not in (_abi.HER_GOAL_FUTURE, _abi.HER_GOAL_FINAL, _abi.HER_GOAL_OWN):
        raise ValueError(f"strategy must be one of {sorted(_abi.HER_STRATEGIES)} (or URGYM_HER_GOAL_*), got {strategy!r}; SB3's 'episode' is out of scope")
    if isinstance(horizon, bool) or int(horizon) != horizon or not 1 <= int(horizon) <= _abi.HER_HORIZON_MAX:
        raise ValueError(f"horizon must be an integer in [1, {_abi.HER_HORIZON_MAX}], got {horizon!r}")
    return int(threshold), int(strategy), int(horizon)


def hindsight_pick(ring_flags, oldest_slot, filled, seed, draw, count, threshold, strategy, horizon, num_envs):
    """The integer half of urgym_replay_sample_hindsight restated from include/urgym.h: pure integers, no float.  `ring_flags`: the
    ring's ``terminated`` and ``truncated`` as host arrays [C, N]; `threshold` in [0, 2^32]; `strategy` "future", "final", "own" or
    the URGYM_HER_GOAL_* number.  For row i, with the Philox word w of ``replay_indices`` (same key, same counter): e as there, p = e //
    N, env = e % N, index = ((oldest_slot + p) % C) N + env; relabel = w[2] < threshold; H = min(horizon, filled - p), entry_k =
    ((oldest_slot + p + k) % C) N + env, F = the smallest k + 1 <= H with terminated | truncated at entry_k, else H; j = (w[3] F) >> 32
    for "future", F - 1 otherwise; g = entry_j.  Returns a dict of [count] arrays: ``e``, ``index``, ``g`` (int64), ``relabel``
    (bool), ``F``, ``j`` (int32) -- F, j and g for every row, relabelled or not -- and ``goal_index`` (int64): g where the row is
    relabelled and the strategy is not "own", else -1."""
    from . import _abi

    threshold, strategy, horizon = _her_arguments(threshold, strategy, horizon)
    oldest_slot, filled, count, N = int(oldest_slot), int(filled), int(count), int(num_envs)
    term, trunc = np.asarray(ring_flags["terminated"]), np.asarray(ring_flags["truncated"])
    if term.ndim != 2 or term.shape != trunc.shape or term.shape[1] != N:
        raise ValueError(f"terminated and truncated must be [C, {N}] arrays, got {term.shape} and {trunc.shape}")
    cap = term.shape[0]
    if not (1 <= filled <= cap and 0 <= oldest_slot < cap):
        raise ValueError(f"filled must be in [1, {cap}] and oldest_slot in [0, {cap}), got {filled}, {oldest_slot}")
    seed, draw = int(seed), int(draw)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10(key, (np.arange(count, dtype=np.uint64), np.uint64(draw & 0xFFFFFFFF), np.uint64((draw >> 32) & 0xFFFFFFFF),
                            np.uint64(_abi.REPLAY_TAG)))
    size = filled * N
    e = np.array([((int(hi) << 32 | int(lo)) * size) >> 64 for hi, lo in zip(w[0], w[1])], dtype=np.int64).reshape(count)
    p, env = e // N, e % N
    relabel = w[2].astype(np.uint64) < np.uint64(threshold) if threshold < 1 << 32 else np.ones(count, bool)
    ends = ((term != 0) | (trunc != 0)).reshape(cap * N)
    H = np.minimum(horizon, filled - p)
    F, running = np.zeros(count, np.int64), np.ones(count, bool)
    for k in range(int(H.max()) if count else 0):
        take = running & (k < H)
        entry = np.where(take, ((oldest_slot + p + k) % cap) * N + env, 0)  # rows that take no step k read nothing of it
        F = np.where(take, k + 1, F)
        running = running & ~(take & ends[entry])
    j = (w[3].astype(np.uint64) * F.astype(np.uint64)) >> np.uint64(32) if strategy == _abi.HER_GOAL_FUTURE else F - 1  # w3 F < 2^41
    j = j.astype(np.int64)
    g = ((oldest_slot + p + j) % cap) * N + env
    index = ((oldest_slot + p) % cap) * N + env
    goal_index = np.where(relabel & (strategy != _abi.HER_GOAL_OWN), g, -1).astype(np.int64)
    return dict(e=e, index=index.astype(np.int64), relabel=relabel, F=F.astype(np.int32), j=j.astype(np.int32), g=g.astype(np.int64), goal_index=goal_index)


HER_CONFIG_FIELDS = ("env_kind", "distance_threshold", "ori_threshold", "w_collision", "w_success", "w_distance", "w_orientation")


def _her_config(config):
    get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
    c = {k: get(k) for k in HER_CONFIG_FIELDS}
    return int(c.pop("env_kind")), {k: np.float64(v) for k, v in c.items()}


def hindsight_rescore(config, goal_dim, reward, terminated, is_success, pose_terms):
    """The re-scoring of urgym_her.h restated in numpy float64, one operation per line and in the header's order.  `reward` float32,
    `terminated`, `is_success` the stored flags, `pose_terms` [rows, 4] float64 = d, th, d0, th0.  Returns (reward' float32,
    terminated' uint8, is_success' uint8)."""
    from . import _abi

    kind, c = _her_config(config)
    t4 = np.asarray(pose_terms, dtype=np.float64)
    d, th, d0, th0 = t4[:, 0], t4[:, 1], t4[:, 2], t4[:, 3]
    r = np.asarray(reward, dtype=np.float32).astype(np.float64)
    term, succ0 = np.asarray(terminated) != 0, np.asarray(is_success) != 0
    coll = term & ~succ0
    with np.errstate(all="ignore"):  # a NaN goal is a value
        succ = d < c["distance_threshold"]
        if goal_dim == 6:
            succ = succ & (th < c["ori_threshold"])

        def goal_terms(s, dist, ang):
            g = np.where(s, c["w_success"], np.float64(0))
            k = np.where(coll, c["w_collision"], np.float64(0))
            g = g + k
            t = c["w_distance"] * dist
            g = g + t
            u = c["w_orientation"] * ang
            g = g + u
            return g

        if kind in (_abi.ENV_ORI, _abi.ENV_OBS):
            g0 = goal_terms(succ0, d0, th0)
            g1 = goal_terms(succ, d, th)
            out = r - g0
            out = out + g1
        else:
            t0 = c["w_distance"] * d0
            S = r - t0
            u0 = c["w_orientation"] * th0
            S = S - u0
            S = np.where(succ0, np.float64(0), S)
            t = c["w_distance"] * d
            u = c["w_orientation"] * th
            shaped = t + u
            shaped = shaped + S
            out = np.where(coll, c["w_collision"], np.where(succ, c["w_success"], shaped))
        assert out.dtype == np.float64
        new_term = succ | coll
        return out.astype(np.float32), new_term.astype(np.uint8), (new_term & ~coll).astype(np.uint8)


def hindsight_batch(ring_arrays, oldest_slot, filled, seed, draw, count, threshold, strategy, horizon, config, pose_terms):
    """urgym_replay_sample_hindsight restated from include/urgym.h, every output, given the pose terms.  `ring_arrays`: the ring's
    eleven fields as host arrays [C, N, ...]; `config`: the env's urgym_config (``_abi.Config``, or a dict of ``HER_CONFIG_FIELDS``);
    `pose_terms`: [count, 4] float64 = d, th, d0, th0 per row (the library's own output, or a harness's: sincos and acos are restated
    bitwise by no host; rows that are not relabelled ignore theirs).  Returns a dict: ``index``, ``goal_index`` (int64), ``relabel``
    (bool), the seven row outputs, ``reward`` (float32) and the three flags (uint8).  A row that is not relabelled is plain indexing."""
    from . import _abi

    obs = np.asarray(ring_arrays["observation"])
    cap, N, obs_dim = obs.shape
    goal_dim = int(np.asarray(ring_arrays["desired_goal"]).shape[2])
    if goal_dim not in (3, 6) or obs_dim < _abi.HER_GOAL_OFFSET + goal_dim:
        raise ValueError(f"the observation row ({obs_dim} floats) holds no goal of {goal_dim} floats at [{_abi.HER_GOAL_OFFSET}, {_abi.HER_GOAL_OFFSET + goal_dim})")
    for k in ("truncated", "is_success"):
        if ring_arrays.get(k) is None:
            raise ValueError(f"hindsight needs the ring's {k}")
    pick = hindsight_pick(ring_arrays, oldest_slot, filled, seed, draw, count, threshold, strategy, horizon, N)
    _, strategy, _ = _her_arguments(threshold, strategy, horizon)
    t4 = np.asarray(pose_terms)
    if t4.dtype != np.float64 or t4.shape != (int(count), 4):
        raise ValueError(f"pose_terms must be float64 [{int(count)}, 4], got {t4.dtype} {t4.shape}")
    flat = lambda a: np.asarray(a).reshape(cap * N, *np.asarray(a).shape[2:])  # noqa: E731
    e, rel = pick["index"], pick["relabel"]
    out = {name: flat(ring_arrays[name])[e].copy() for name, _, _, _ in _abi.REPLAY_RING_FIELDS}
    goal = flat(ring_arrays["next_desired_goal"])[e] if strategy == _abi.HER_GOAL_OWN else flat(ring_arrays["next_achieved_goal"])[pick["g"]]
    lo = _abi.HER_GOAL_OFFSET
    for name, at in (("desired_goal", 0), ("next_desired_goal", 0), ("observation", lo), ("next_observation", lo)):
        out[name][rel, at:at + goal_dim] = goal[rel]  # float32 words, copied bitwise
    reward, term, succ = hindsight_rescore(config, goal_dim, out["reward"], out["terminated"], out["is_success"], t4)
    out["reward"] = np.where(rel, reward, out["reward"])
    out["terminated"] = np.where(rel, term, out["terminated"]).astype(np.uint8)
    out["is_success"] = np.where(rel, succ, out["is_success"]).astype(np.uint8)
    out.update(index=e, goal_index=pick["goal_index"], relabel=rel)
    return out


def per_sums(leaf, fanout=None):
    """The sum levels of the prioritized replay restated from ur_gym_amd/csrc/urgym_per.h in numpy float64.  `leaf`: float32, any
    shape (taken flat: the ring's entry order).  Level 0 is the leaves; entry b of level k + 1 is the ascending float64 sum, from +0.0,
    of entries fanout b .. fanout b + fanout - 1 of level k (``np.cumsum`` in float64 is that sum); levels are added until one has at
    most `fanout` entries; the total is the ascending sum of that level.  Returns ``levels`` (a list of float64 arrays, level 1
    first), ``total`` (np.float64) and ``flat`` (the levels and the total as the device lays them out)."""
    from . import _abi

    F = int(_abi.PER_FANOUT if fanout is None else fanout)
    leaf = np.asarray(leaf)
    if leaf.dtype != np.float32 or F < 2:
        raise ValueError(f"leaf must be float32 and fanout at least 2, got {leaf.dtype}, {F}")
    v, levels = leaf.reshape(-1).astype(np.float64), []
    while True:
        blocks = -(-v.size // F)
        padded = np.zeros(blocks * F, np.float64)  # an absent entry adds +0.0: no change
        padded[:v.size] = v
        v = np.cumsum(padded.reshape(blocks, F), axis=1)[:, -1] + 0.0  # + 0.0: the sum starts from +0.0 (a block of one -0.0)
        levels.append(v)
        if blocks <= F:
            break
    padded = np.zeros(F, np.float64)
    padded[:v.size] = v
    total = np.float64(np.cumsum(padded)[-1] + 0.0)
    return dict(levels=levels, total=total, flat=np.concatenate(levels + [np.array([total])]))


def per_words(seed, draw, count):
    """The 64-bit words of urgym_replay_sample_prioritized's draw: (w0 << 32) | w1 of Philox4x32-10 at the counter
    (i, draw lo, draw hi, PER_TAG), uint64 [count]."""
    from . import _abi

    seed, draw = int(seed), int(draw)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10(key, (np.arange(int(count), dtype=np.uint64), np.uint64(draw & 0xFFFFFFFF), np.uint64((draw >> 32) & 0xFFFFFFFF),
                            np.uint64(_abi.PER_TAG)))
    return (w[0].astype(np.uint64) << np.uint64(32)) | w[1].astype(np.uint64)


def per_descent(leaf, words, fanout=None, sums=None):
    """The descent of urgym_per.h restated in numpy float64: for each 64-bit word (``per_words``) the leaf it draws.  u = (w >> 11)
    2^-53, t = u total, then from the top level down over the children of the chosen node in ascending order with s = +0.0:
    s2 = s + v[k]; t < s2 takes k and t = t - s; else s = s2.  If no child is taken: the last child with v > 0, else the first, and t
    stays.  `sums`: a ``per_sums`` result of the same leaves (formed here if None).  Returns int64 [len(words)]."""
    from . import _abi

    F = int(_abi.PER_FANOUT if fanout is None else fanout)
    leaf = np.asarray(leaf).reshape(-1)
    sums = per_sums(leaf, F) if sums is None else sums
    below = [leaf.astype(np.float64)] + list(sums["levels"])  # below[k]: level k
    prefix = []
    for v in below:  # the running s2 of every block, once: np.cumsum is the chain s2 = s + v[k] from s = +0.0
        blocks = -(-v.size // F)
        padded = np.zeros(blocks * F, np.float64)
        padded[:v.size] = v
        prefix.append(np.cumsum(padded.reshape(blocks, F), axis=1) + 0.0)
    total, out = sums["total"], np.zeros(len(words), np.int64)
    for i, w in enumerate(np.asarray(words, dtype=np.uint64)):
        t = np.float64(int(w) >> 11) * np.float64(2.0 ** -53) * total
        node = 0
        for k in range(len(below) - 1, -1, -1):  # the top level has one block
            v, span = below[k], min(F, below[k].size - node * F)
            s2 = prefix[k][node]
            j = int(np.searchsorted(s2[:span], t, side="right"))  # the first k with t < s2[k]: s2 never decreases
            if j < span:
                t = t - (s2[j - 1] if j else np.float64(0.0))
            else:
                positive = np.nonzero(v[node * F:node * F + span] > 0)[0]
                j = int(positive[-1]) if positive.size else 0
            node = node * F + j
        out[i] = node
    return out


def per_beta(beta0, step, beta_steps):
    """beta of the update at Adam step `step` (1, 2, ...): beta0 + (1 - beta0) min(1, step / beta_steps) in float64, rounded to
    float32 once (per_beta of urgym_per.h)."""
    f = float(int(step)) / float(int(beta_steps))
    return np.float32(float(beta0) + (1.0 - float(beta0)) * (f if f < 1.0 else 1.0))


def per_terms(leaf_in, total, size, beta, q, y, scale, eps, alpha, w_raw, new_leaf=None, index=None, leaf=None, max_leaf=None):
    """urgym_per_terms restated from include/urgym.h in numpy, one float32 operation per line.  `w_raw` [count] and `new_leaf` [count]
    are INPUTS, as alpha is to ``entropy_step``: the device's powf and numpy's are different functions.  Returns a dict with ``x``
    (powf's argument of w_raw) and ``p`` (that of new_leaf), ``wmax``, ``w``, ``dq`` [2, count], ``replaced`` (the rows whose powf
    cannot be finite: their new_leaf must be the old max_leaf) and, with the write-back group (`new_leaf`, `index`, `leaf` flat or
    [C, N], `max_leaf`), ``leaf`` (a copy: every drawn entry at the largest new_leaf of its rows) and ``max_leaf``."""
    f = np.float32
    q, y, w_raw = np.asarray(q), np.asarray(y), np.asarray(w_raw)
    leaf_in = np.asarray(leaf_in)
    if any(a.dtype != f for a in (q, y, w_raw, leaf_in)) or q.shape != (2, y.size):
        raise ValueError("leaf_in, q [2, count], y and w_raw must be float32")
    size, beta, scale, eps, alpha = f(size), f(beta), f(scale), f(eps), f(alpha)
    with np.errstate(all="ignore"):
        prob = (leaf_in.astype(np.float64) / np.float64(total)).astype(f)
        x = size * prob
        wmax = np.fmax.reduce(w_raw, initial=f(0))
        w = w_raw / wmax
        e = q - y[None, :]
        g = e * scale
        dq = g * w[None, :]
        td = np.fmax(np.abs(e[0]), np.abs(e[1]))
        p = td + eps
    assert all(a.dtype == f for a in (x, w, dq, p))  # no intermediate was promoted
    out = dict(x=x, p=p, wmax=wmax, w=w, dq=dq, replaced=~np.isfinite(p) & (alpha > 0))
    if new_leaf is not None:
        new_leaf, after = np.asarray(new_leaf), np.array(leaf, dtype=f).reshape(-1)
        index = np.asarray(index, dtype=np.int64)
        after[index] = 0
        np.maximum.at(after, index, new_leaf)
        out["leaf"] = after.reshape(np.shape(leaf))
        out["max_leaf"] = np.fmax(f(max_leaf), np.fmax.reduce(new_leaf, initial=f(0)))
    return out


def policy_terms(alpha, *, dqmin_da=None, scale=None, q=None, y=None, log_prob=None, q_min=None):
    """urgym_sac_policy_terms restated from include/urgym.h in numpy float32, the means by ``ordered_sum``; `alpha` as in
    ``entropy_step``.  Groups, each whole or absent: (`dqmin_da` [count, 6], `scale`) gives ``d_action``; (`q` [2, count], `y`
    [count]) gives ``critic_loss`` and ``critic_terms`` [2, count]; (`log_prob`, `q_min` [count] each) gives ``actor_loss`` and
    ``actor_terms`` [count].  Returns a dict."""
    f = np.float32
    alpha = f(alpha)
    if (dqmin_da is None) != (scale is None) or (q is None) != (y is None) or (log_prob is None) != (q_min is None):
        raise ValueError("a group is half given: (dqmin_da, scale), (q, y), (log_prob, q_min)")
    if dqmin_da is None and q is None and log_prob is None:
        raise ValueError("no group is given")
    out, checked = {}, []
    with np.errstate(all="ignore"):
        if dqmin_da is not None:
            dqmin_da = np.asarray(dqmin_da)
            dqmin_da = _rows32("dqmin_da", dqmin_da, (dqmin_da.shape[0], 6))
            out["d_action"] = dqmin_da * f(scale)
            checked.append(out["d_action"])
        if q is not None:
            y = np.asarray(y)
            y = _rows32("y", y, (y.size,))
            q = _rows32("q", q, (2, y.size))
            e = q - y[None, :]
            sq = e * e
            mean0, mean1 = _ordered_mean(sq[0]), _ordered_mean(sq[1])
            both = mean0 + mean1
            out["critic_loss"], out["critic_terms"] = f(0.5) * both, sq
            checked += [e, sq, mean0, mean1, both, out["critic_loss"]]
        if log_prob is not None:
            log_prob = np.asarray(log_prob)
            log_prob = _rows32("log_prob", log_prob, (log_prob.size,))
            q_min = _rows32("q_min", q_min, log_prob.shape)
            a = alpha * log_prob
            b = a - q_min
            out["actor_loss"], out["actor_terms"] = _ordered_mean(b), b
            checked += [a, b, out["actor_loss"]]
    for x in checked:
        assert x.dtype == f, x.dtype  # no intermediate was promoted
    return out


def policy_terms_cloned(alpha, *, dqmin_da, scale, q, y, log_prob, q_min, action_pi, action_data, weight, bc_scale, scale_by_q=False, q_filter=False,
                        w_mean_abs=None, row_mask=None):
    """urgym_sac_policy_terms_cloned restated from include/urgym.h in numpy float32, line by line, the means by ``ordered_sum``.  The
    arguments of ``policy_terms`` (all three groups, `q` the online critics at the replayed action) and `action_pi`, `action_data`
    [count, 6], `weight`, `bc_scale`, the two flags.  `w_mean_abs`: None, or the float32 to take for the mean of ``|q_min|`` in the
    weight instead of this function's own (a test that feeds another reduction's value).  Returns a dict: ``d_action`` [count, 6],
    ``critic_loss``, ``actor_loss``, ``bc_loss``, ``bc_weight`` (float32 scalars), ``bc_rows`` (int32), ``cloned`` (bool [count]),
    ``mean_abs`` (float32) and ``bc_terms`` (h, float32 [count]).

    With `row_mask` ([count], uint8 or bool) the call restated is urgym_sac_policy_terms_cloned_masked: a row is cloned only where its
    mask is nonzero AND the verdict above holds; everything else is unchanged (the means stay over all rows)."""
    f = np.float32
    out = policy_terms(alpha, dqmin_da=dqmin_da, scale=scale, q=q, y=y, log_prob=log_prob, q_min=q_min)
    g = out.pop("d_action")
    count = g.shape[0]
    q, q_min = np.asarray(q), np.asarray(q_min)
    action_pi, action_data = _rows32("action_pi", action_pi, (count, 6)), _rows32("action_data", action_data, (count, 6))
    with np.errstate(all="ignore"):
        weight, bc_scale = f(weight), f(bc_scale)
        if not (np.isfinite(weight) and weight >= 0 and np.isfinite(bc_scale)):
            raise ValueError(f"weight must be finite and >= 0 and bc_scale finite in float32, got {weight!r}, {bc_scale!r}")
        qd = np.where(q[1] < q[0], q[1], q[0])
        cloned = (qd > q_min) if q_filter else np.ones(count, dtype=bool)
        if row_mask is not None:
            mask = np.asarray(row_mask)
            if mask.shape != (count,) or mask.dtype not in (np.dtype(np.uint8), np.dtype(bool)):
                raise ValueError(f"row_mask must be uint8 or bool [{count}], got {mask.dtype} {mask.shape}")
            cloned = (mask != 0) & cloned
        d = action_pi - action_data
        s = np.zeros(count, dtype=f)
        for k in range(6):
            p = d[:, k] * d[:, k]
            s = s + p
        h = np.where(cloned, f(0.5) * s, f(0.0))
        absq = np.abs(q_min)
        mean_abs = _ordered_mean(absq)
        bc_loss = _ordered_mean(h)
        used = mean_abs if w_mean_abs is None else f(w_mean_abs)
        w = weight * used if scale_by_q else weight
        t = d * w
        u = t * bc_scale
        d_action = np.where(cloned[:, None], g + u, g)
    for x in (qd, d, s, h, absq, mean_abs, bc_loss, w, t, u, d_action):
        assert x.dtype == f, x.dtype  # no intermediate was promoted
    out.update(d_action=d_action, bc_loss=bc_loss, bc_weight=w, bc_rows=np.int32(np.count_nonzero(cloned)), cloned=cloned, mean_abs=mean_abs, bc_terms=h)
    return out


def policy_terms_weighted(alpha, *, dqmin_da, scale, q, y, log_prob, q_min, action_pi, action_data, weight, bc_scale, temperature, max_weight=np.inf,
                          scale_by_q=False, row_mask=None):
    """urgym_sac_policy_terms_weighted restated from include/urgym.h ("advantage-weighted cloning in the policy loss") in numpy, line by
    line: float32 where the header says float32, float64 where it says float64, the sums by ``ordered_sum``, the exponential by
    ``mppi_temper_exp``.  The arguments of ``policy_terms_cloned`` without the Q-filter, and `temperature` (finite, > 0 in float32),
    `max_weight` (> 0, finite or inf), `row_mask` (None, or uint8 / bool [count]).  Returns a dict: ``d_action`` [count, 6],
    ``critic_loss``, ``actor_loss``, ``bc_loss``, ``bc_weight``, ``adv_ess``, ``adv_max`` (float32 scalars), ``bc_rows``, ``adv_clipped``
    (int32), ``eligible`` (bool [count]), ``advantage`` (A, float32 [count]), ``a`` (the weights, float32 [count]), ``e`` (float64
    [count]), ``Z``, ``Q`` (float64), ``mean_abs`` (float32), ``bc_terms`` (h, float32 [count]) and ``weighted_terms`` (a * h)."""
    f, d8 = np.float32, np.float64
    out = policy_terms(alpha, dqmin_da=dqmin_da, scale=scale, q=q, y=y, log_prob=log_prob, q_min=q_min)
    g = out.pop("d_action")
    count = g.shape[0]
    q, q_min = np.asarray(q), np.asarray(q_min)
    action_pi, action_data = _rows32("action_pi", action_pi, (count, 6)), _rows32("action_data", action_data, (count, 6))
    with np.errstate(all="ignore"):
        weight, bc_scale, temperature, max_weight = f(weight), f(bc_scale), f(temperature), f(max_weight)
        if not (np.isfinite(weight) and weight >= 0 and np.isfinite(bc_scale)):
            raise ValueError(f"weight must be finite and >= 0 and bc_scale finite in float32, got {weight!r}, {bc_scale!r}")
        if not (np.isfinite(temperature) and temperature > 0):
            raise ValueError(f"temperature must be finite and > 0 in float32, got {temperature!r}")
        if not max_weight > 0:
            raise ValueError(f"max_weight must be > 0 (finite or inf), got {max_weight!r}")
        qd = np.where(q[1] < q[0], q[1], q[0])
        A = qd - q_min
        eligible = np.isfinite(A)
        if row_mask is not None:
            mask = np.asarray(row_mask)
            if mask.shape != (count,) or mask.dtype not in (np.dtype(np.uint8), np.dtype(bool)):
                raise ValueError(f"row_mask must be uint8 or bool [{count}], got {mask.dtype} {mask.shape}")
            eligible = (mask != 0) & eligible
        n = int(np.count_nonzero(eligible))
        absq = np.abs(q_min)
        mean_abs = _ordered_mean(absq)
        w = weight * mean_abs if scale_by_q else weight
        d = action_pi - action_data
        s = np.zeros(count, dtype=f)
        for k in range(6):
            p = d[:, k] * d[:, k]
            s = s + p
        h = np.where(eligible, f(0.5) * s, f(0.0))
        e = np.zeros(count, dtype=d8)
        a = np.zeros(count, dtype=f)
        Z = Q = d8(0.0)
        adv_ess = adv_max = f(0.0)
        clipped = 0
        if n > 0:
            A_max = A[eligible].max()
            dd = np.where(eligible, A.astype(d8) - d8(A_max), d8(0.0))
            x = dd / d8(temperature)
            e = np.where(eligible, mppi_temper_exp(x), d8(0.0))
            Z, Q = ordered_sum(e, d8), ordered_sum(e * e, d8)
            mean_e = Z / d8(n)
            u = e / mean_e
            over = eligible & (u > d8(max_weight))
            v = np.where(over, d8(max_weight), u)
            a = np.where(eligible, v, d8(0.0)).astype(f)
            clipped = int(np.count_nonzero(over))
            zz = Z * Z
            adv_ess = f(zz / Q)
            top = d8(1.0) / mean_e
            adv_max = f(d8(max_weight) if top > d8(max_weight) else top)
            for x64 in (dd, x, e, mean_e, u, v, zz):
                assert x64.dtype == d8, x64.dtype
        ah = a * h
        bc_loss = _ordered_mean(ah)
        wr = w * a
        t = d * wr[:, None]
        uu = t * bc_scale
        d_action = np.where(eligible[:, None], g + uu, g)
    for x32 in (qd, A, d, s, h, absq, mean_abs, a, ah, bc_loss, w, wr, t, uu, d_action, adv_ess, adv_max):
        assert x32.dtype == f, x32.dtype  # no intermediate was promoted
    out.update(d_action=d_action, bc_loss=bc_loss, bc_weight=w, bc_rows=np.int32(n), adv_ess=adv_ess, adv_max=adv_max, adv_clipped=np.int32(clipped),
               eligible=eligible, advantage=A, a=a, e=e, Z=d8(Z), Q=d8(Q), mean_abs=mean_abs, bc_terms=h, weighted_terms=ah)
    return out


def _check_device_tensors(tensors, wanted, device, who):
    """`wanted`: name -> shape.  Raises ValueError unless every one is a contiguous float32 torch tensor of that shape on `device`."""
    import torch

    device = torch.device(device)
    for name, shape in wanted.items():
        t = tensors[name]
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a torch tensor on {device}, got {type(t).__name__}")
        if t.device != device:
            raise ValueError(f"{who}: {name} is on {t.device}, the object lives on {device}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous (row-major [out][in])")


def _read_packed(env, call, obj):
    import ctypes as C

    from . import _native

    count = C.c_uint64()
    _native.check(call(env._h, obj, None, 0, C.byref(count)), env._h)
    out = np.empty(count.value, dtype=np.float32)
    _native.check(call(env._h, obj, C.c_void_p(out.ctypes.data), count.value, C.byref(count)), env._h)
    return out


LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0  # SB3 sac/policies.py
LOG_STD_ARRAYS = ("log_std_weight", "log_std_bias")


class StochasticActor(DeterministicActor):
    """The sampled half of the same policy (SB3 SquashedDiagGaussianDistribution) on the host, float32: needs the two log_std
    arrays (tests/golden/gen_log_std_fixtures.py) next to DeterministicActor's six."""

    def heads(self, achieved_goal, desired_goal, observation):
        """(mu, log_std after the clamp), float32 [N, 6] each."""
        x = np.concatenate([achieved_goal, desired_goal, observation], axis=1).astype(np.float32)
        assert x.shape[1] == self.in_features, (x.shape, self.in_features)
        h = np.maximum(x @ self.w["latent_pi_0_weight"].T + self.w["latent_pi_0_bias"], 0.0)
        h = np.maximum(h @ self.w["latent_pi_2_weight"].T + self.w["latent_pi_2_bias"], 0.0)
        mu = (h @ self.w["mu_weight"].T + self.w["mu_bias"]).astype(np.float32)
        log_std = h @ self.w["log_std_weight"].T + self.w["log_std_bias"]
        return mu, np.clip(log_std, LOG_STD_MIN, LOG_STD_MAX).astype(np.float32)

    @staticmethod
    def gaussian_log_prob(eps, log_std):
        """sum_j [-eps_j^2 / 2 - log_std_j - log(2 pi) / 2] in the arrays' precision."""
        t = eps.dtype.type
        return (t(-0.5) * eps * eps - log_std - t(0.5 * np.log(2 * np.pi))).sum(axis=1)

    def __call__(self, achieved_goal, desired_goal, observation, eps):
        """eps: float32 [N, 6] (policy_noise(..., "gaussian"), or zeros for the mean).  Returns (action, log_prob)."""
        mu, log_std = self.heads(achieved_goal, desired_goal, observation)
        eps = np.asarray(eps, dtype=np.float32)
        action = np.tanh(mu + np.exp(log_std) * eps).astype(np.float32)
        squash = np.log(np.float32(1.0) - action * action + np.float32(1e-6)).sum(axis=1)
        return action, (self.gaussian_log_prob(eps, log_std) - squash).astype(np.float32)

    def parameter_gradients(self, achieved_goal, desired_goal, observation, eps=None, d_action=None, d_log_prob=None, d_mu=None, d_log_std=None):
        """(grads, records) in float32 as include/urgym.h states urgym_actor_parameter_gradients: `grads` keyed by ACTOR_ARRAYS +
        LOG_STD_ARRAYS, the gradients of a loss summed over the rows; `records` a dict with ``action``, ``log_prob``, ``noise``,
        ``log_std`` (clamped), ``std`` = exp(log_std), ``d_mu`` and ``d_log_std`` (before the clamp derivative).  `eps`: the noise [N, 6] (None = zeros, the
        mean).  The upstream gradient is either the SAMPLE form (`d_action` [N, 6], `d_log_prob` [N] or None = 0: the gradient with
        respect to this call's action and log_prob, the noise a constant; ``sample_head_gradients`` states its arithmetic) or the
        HEADS form (`d_mu` and `d_log_std` [N, 6], used as they are).  A pre-activation of exactly 0 has derivative 0; the clamp
        passes the gradient where -20 <= r <= 2.  (The order of the sums is numpy's, not the kernel's.)"""
        sample_form, heads_form = d_action is not None or d_log_prob is not None, d_mu is not None or d_log_std is not None
        if sample_form == heads_form or (sample_form and d_action is None) or (heads_form and (d_mu is None or d_log_std is None)):
            raise ValueError("exactly one upstream form must be given: d_action (with d_log_prob or None), or both d_mu and d_log_std")
        f, zero = np.float32, np.float32(0.0)
        w = self.w
        x = np.concatenate([achieved_goal, desired_goal, observation], axis=1).astype(f)
        assert x.shape[1] == self.in_features, (x.shape, self.in_features)
        eps = np.zeros((len(x), 6), f) if eps is None else np.asarray(eps, dtype=f)
        z1 = x @ w["latent_pi_0_weight"].T + w["latent_pi_0_bias"]
        h1 = np.maximum(z1, zero)
        z2 = h1 @ w["latent_pi_2_weight"].T + w["latent_pi_2_bias"]
        h2 = np.maximum(z2, zero)
        mu = (h2 @ w["mu_weight"].T + w["mu_bias"]).astype(f)
        r = (h2 @ w["log_std_weight"].T + w["log_std_bias"]).astype(f)
        log_std = np.clip(r, f(LOG_STD_MIN), f(LOG_STD_MAX)).astype(f)
        std = np.exp(log_std).astype(f)
        action = np.tanh(mu + std * eps).astype(f)
        squash = np.log(f(1.0) - action * action + f(1e-6)).sum(axis=1)
        log_prob = (self.gaussian_log_prob(eps, log_std) - squash).astype(f)
        if sample_form:
            d_mu, d_log_std = sample_head_gradients(action, log_std, eps, d_action, d_log_prob, std=std)
        d_mu, d_log_std = np.asarray(d_mu, dtype=f), np.asarray(d_log_std, dtype=f)
        dr = np.where((r >= f(LOG_STD_MIN)) & (r <= f(LOG_STD_MAX)), d_log_std, zero).astype(f)
        d2 = np.where(z2 > 0.0, d_mu @ w["mu_weight"] + dr @ w["log_std_weight"], zero).astype(f)
        d1 = np.where(z1 > 0.0, d2 @ w["latent_pi_2_weight"], zero).astype(f)
        g = (d1.T @ x, d1.sum(axis=0), d2.T @ h1, d2.sum(axis=0), d_mu.T @ h2, d_mu.sum(axis=0), dr.T @ h2, dr.sum(axis=0))
        grads = {k: np.asarray(v, dtype=f) for k, v in zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, g)}
        return grads, dict(action=action, log_prob=log_prob, noise=eps, log_std=log_std, std=std, d_mu=d_mu, d_log_std=d_log_std)


def sample_head_gradients(action, log_std, noise, d_action, d_log_prob=None, std=None):
    """(d_mu, d_log_std), float32 [N, 6] each: the head arithmetic of urgym_actor_parameter_gradients' SAMPLE form as include/urgym.h
    states it, from the call's own records, every line one float32 operation rounded on its own:
        p = a * a;  t = 1 - p;  c = (2 a) / (t + 1e-6);  A = d_action + (d_log_prob * c);  d_pre = A * t;  d_mu = d_pre;
        e = exp(log_std) * noise;  d_log_std = (d_pre * e) - d_log_prob.
    `d_log_prob` None means 0.  `std`: exp(log_std) as the forward pass formed it, where the caller has it bit for bit (the call's ``std`` record: the
    kernel's expf and numpy's float32 exp are both good to an ulp and differ in the last bit on more than a third of the values); None = numpy's."""
    f = np.float32
    a, ls, eps, da = (np.asarray(v, dtype=f) for v in (action, log_std, noise, d_action))
    dlp = np.zeros(len(a), f) if d_log_prob is None else np.asarray(d_log_prob, dtype=f)
    dlp = dlp[:, None]
    p = (a * a).astype(f)
    t = (f(1.0) - p).astype(f)
    c = ((f(2.0) * a).astype(f) / (t + f(1e-6)).astype(f)).astype(f)
    big_a = (da + (dlp * c).astype(f)).astype(f)
    d_pre = (big_a * t).astype(f)
    e = ((np.exp(ls).astype(f) if std is None else np.asarray(std, dtype=f)) * eps).astype(f)
    return d_pre, ((d_pre * e).astype(f) - dlp).astype(f)


def goal_grid(low, high, step=0.05, repeats=5):
    """utils/generate.py:29-43, 63-80: every grid node of the goal range, `repeats` times (float arithmetic as there)."""
    n = [int((high[i] - low[i]) / step) + 1 for i in range(3)]
    pts = [(low[0] + i * step, low[1] + j * step, low[2] + k * step)
           for i in range(n[0]) for j in range(n[1]) for k in range(n[2]) for _ in range(repeats)]
    return np.array(pts, dtype=np.float64)


def constrained_euler(rng, n):
    """utils.sample_euler_constrained (utils.py:81-86) for n goals."""
    return np.stack([np.deg2rad(-rng.uniform(90, 180, n)), np.zeros(n), np.deg2rad(-rng.uniform(0, 180, n))], axis=1)


def run_closed_loop(backend, actor, max_steps=100):
    """model_test.run_test (model_test.py:26-61) for all envs of `backend` at once.

    backend: object with ``num_envs``, ``observe() -> (achieved, desired, observation)`` numpy arrays and
    ``step(actions) -> (reward, terminated, is_success)`` numpy arrays; auto-reset must be OFF.
    Returns dict(success_rate_percent, mean_episode_reward, mean_last_step_index, per-trial arrays).
    """
    n = backend.num_envs
    done = np.zeros(n, bool)
    success = np.zeros(n, bool)
    reward = np.zeros(n)
    last = np.zeros(n)
    for t in range(max_steps):
        a = actor(*backend.observe())
        r, term, succ = backend.step(a)
        live = ~done
        reward[live] += r[live]
        fin = live & (term.astype(bool) | (t == max_steps - 1))  # model_test.py:46: `if steps == 99 or terminated`
        success[fin] = succ[fin].astype(bool)
        last[fin] = t
        done |= fin
        if done.all():
            break
    return {"success_rate_percent": 100.0 * success.mean(), "mean_episode_reward": float(reward.mean()),
            "mean_last_step_index": float(last.mean()), "success": success, "reward": reward, "last_step": last}


class HipBackend:
    """Adapter of UR5ReachVectorEnv (created with auto_reset=False) for run_closed_loop."""

    def __init__(self, env):
        import torch

        self.env, self.torch = env, torch
        self.num_envs = env.num_envs

    def observe(self):
        b = self.env.buf
        return b["achieved_goal"].cpu().numpy(), b["desired_goal"].cpu().numpy(), b["observation"].cpu().numpy()

    def step(self, actions):
        obs, rew, term, trunc, info = self.env.step(self.torch.from_numpy(actions).to(self.env.device))
        return rew.cpu().numpy().astype(np.float64), term.cpu().numpy(), info["is_success"].cpu().numpy()


ACTOR_ARRAYS = ("latent_pi_0_weight", "latent_pi_0_bias", "latent_pi_2_weight", "latent_pi_2_bias", "mu_weight", "mu_bias")


class DeviceActor:
    """The same actor as ``DeterministicActor``, evaluated by the HIP kernel of the extension (urgym_actor_create).

    It belongs to the environment it was loaded for (the native actor lives in that environment's handle) and is consumed by
    ``env.policy_actions(actor)``, ``env.rollout_policy(actor, K)`` and ``run_closed_loop_device(env, actor)``.
    """

    def __init__(self, weights, env):
        import ctypes as C

        from . import _abi, _native

        w = {k: v for k, v in dict(weights).items()}
        self.in_features, self.hidden_width = self.check_shapes(w, env.env_kind)
        self.env = env
        arrays = [np.ascontiguousarray(w[k], dtype=np.float32) for k in ACTOR_ARRAYS]  # copied by the library during the call
        desc = _abi.ActorDesc(self.in_features, self.hidden_width, 6, 0, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrays])
        self._a = C.c_void_p()
        _native.check(env.lib.urgym_actor_create(env._h, C.byref(desc), C.byref(self._a)), env._h)
        self.has_log_std = all(k in w for k in LOG_STD_ARRAYS)  # the stochastic half: sample= of policy_actions / rollout_policy
        if self.has_log_std:
            head = [np.ascontiguousarray(w[k], dtype=np.float32) for k in LOG_STD_ARRAYS]
            _native.check(env.lib.urgym_actor_set_log_std(env._h, self._a, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in head]), env._h)

    @classmethod
    def load(cls, npz_path, env):
        return cls(np.load(npz_path), env)

    @staticmethod
    def check_shapes(weights, env_kind):
        """Raises ValueError unless `weights` is an ``in -> H -> H -> 6`` actor the kernel supports for `env_kind`
        (in = obs_dim + 2 goal_dim of that env, H a multiple of 32 and at most 512).  Returns (in_features, H).  Needs no GPU."""
        from . import _abi

        missing = [k for k in ACTOR_ARRAYS if k not in weights]
        if missing:
            raise ValueError(f"actor arrays missing: {missing}")
        shape = {k: tuple(np.shape(weights[k])) for k in ACTOR_ARRAYS}
        if any(len(shape[k]) != 2 for k in ACTOR_ARRAYS[0::2]) or any(len(shape[k]) != 1 for k in ACTOR_ARRAYS[1::2]):
            raise ValueError(f"actor weights must be 2-d and biases 1-d, got {shape}")
        (h0, in_features), (h1, h0_in), (out, h1_in) = shape["latent_pi_0_weight"], shape["latent_pi_2_weight"], shape["mu_weight"]
        obs_dim, goal_dim = _abi.OBS_DIMS[env_kind]
        if in_features != obs_dim + 2 * goal_dim:
            raise ValueError(f"actor takes {in_features} features, this env offers {obs_dim + 2 * goal_dim} (achieved_goal | desired_goal | observation)")
        if not (h0 == h1 == h0_in == h1_in):
            raise ValueError(f"the two hidden layers must have one width, got {shape}")
        if h0 % 32 != 0 or not 0 < h0 <= 512:
            raise ValueError(f"hidden width must be a multiple of 32 and at most 512, got {h0}")
        if out != 6:
            raise ValueError(f"the actor must have 6 outputs, got {out}")
        if shape["latent_pi_0_bias"] != (h0,) or shape["latent_pi_2_bias"] != (h0,) or shape["mu_bias"] != (6,):
            raise ValueError(f"bias shapes do not match the weights: {shape}")
        present = [k for k in LOG_STD_ARRAYS if k in weights]
        if present:  # optional; both or neither, shaped like mu's
            if len(present) != 2:
                raise ValueError(f"log_std head needs both {LOG_STD_ARRAYS}, got only {present}")
            got = tuple(tuple(np.shape(weights[k])) for k in LOG_STD_ARRAYS)
            if got != ((6, h0), (6,)):
                raise ValueError(f"log_std head must be [6, {h0}] and [6], got {got}")
        return in_features, h0

    @staticmethod
    def check_parameters(tensors, in_features, hidden_width, device):
        """Raises ValueError unless `tensors` (a dict under ACTOR_ARRAYS, optionally with both LOG_STD_ARRAYS) holds contiguous
        float32 torch tensors on `device` shaped for an ``in_features -> hidden_width -> hidden_width -> 6`` actor.  Returns whether
        the log_std head is present.  Needs no GPU."""
        missing = [k for k in ACTOR_ARRAYS if k not in tensors]
        if missing:
            raise ValueError(f"load_parameters: actor tensors missing: {missing}")
        unknown = [k for k in tensors if k not in ACTOR_ARRAYS + LOG_STD_ARRAYS]
        if unknown:
            raise ValueError(f"load_parameters: unknown actor tensors {unknown}; expected {ACTOR_ARRAYS + LOG_STD_ARRAYS}")
        present = [k for k in LOG_STD_ARRAYS if k in tensors]
        if len(present) == 1:
            raise ValueError(f"load_parameters: the log_std head needs both {LOG_STD_ARRAYS}, got only {present}")
        n, H = int(in_features), int(hidden_width)
        wanted = dict(zip(ACTOR_ARRAYS, ((H, n), (H,), (H, H), (H,), (6, H), (6,))))
        if present:
            wanted.update(zip(LOG_STD_ARRAYS, ((6, H), (6,))))
        _check_device_tensors(tensors, wanted, device, "load_parameters")
        return bool(present)

    def load_parameters(self, tensors):
        """Reloads the actor from device tensors (urgym_actor_load): `tensors` as ``check_parameters`` takes them, e.g. the
        parameters of a torch module as they lie.  ONE launch on torch's current stream, nothing is synchronised: passes enqueued
        before it see the old weights, later ones the new; the tensors are read when the launch runs, so whatever writes them must
        come before it on that stream, and they must stay alive until it has run (a tensor freed earlier is safe only if torch
        reuses its memory on the same stream).  Without the log_std tensors the head keeps what it held."""
        import ctypes as C

        from . import _abi, _native

        env = self.env
        head = self.check_parameters(tensors, self.in_features, self.hidden_width, env.device)
        p = _abi.ActorParamsDev(self.in_features, self.hidden_width, 0)
        for field, key in zip(_abi.ACTOR_DEV_ARRAYS, ACTOR_ARRAYS + (LOG_STD_ARRAYS if head else ())):
            setattr(p, field, C.cast(tensors[key].data_ptr(), C.POINTER(C.c_float)))
        _native.check(env.lib.urgym_actor_load(env._h, self._a, C.byref(p), env._stream()), env._h)
        self.has_log_std = self.has_log_std or head

    def parameters(self, out=None):
        """The actor's tensors as the packed buffer holds them (urgym_actor_unpack): a dict of device tensors under ACTOR_ARRAYS, and
        LOG_STD_ARRAYS too when the actor has the head.  `out`: the tensors to write, checked as ``check_parameters`` checks sources
        (without the head tensors the head is skipped); None = fresh ones.  ONE launch on torch's current stream, nothing is
        synchronised: it sees the loads and Adam steps enqueued before it, and the tensors hold the result once it has run."""
        import ctypes as C

        import torch

        from . import _abi, _native

        env, n, H = self.env, self.in_features, self.hidden_width
        if out is None:
            shapes = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, ((H, n), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))
            keys = ACTOR_ARRAYS + (LOG_STD_ARRAYS if self.has_log_std else ())
            out = {k: torch.empty(shapes[k], dtype=torch.float32, device=env.device) for k in keys}
        head = self.check_parameters(out, n, H, env.device)
        if head and not self.has_log_std:
            raise ValueError(f"parameters: the actor has no log_std head, out must not hold {LOG_STD_ARRAYS}")
        p = _abi.ActorParamsOut(n, H, 0)
        for field, key in zip(_abi.ACTOR_DEV_ARRAYS, ACTOR_ARRAYS + (LOG_STD_ARRAYS if head else ())):
            setattr(p, field, C.cast(out[key].data_ptr(), C.POINTER(C.c_float)))
        _native.check(env.lib.urgym_actor_unpack(env._h, self._a, C.byref(p), env._stream()), env._h)
        return out

    def packed(self):
        """The packed weight buffer as the kernel reads it (float32 numpy array; urgym_actor_read_packed).  A verification aid:
        synchronises the device."""
        return _read_packed(self.env, self.env.lib.urgym_actor_read_packed, self._a)

    def close(self):
        if getattr(self, "_a", None) and getattr(self.env, "_h", None):
            self.env.lib.urgym_actor_destroy(self.env._h, self._a)
        self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CRITIC_ARRAYS = ("q_0_weight", "q_0_bias", "q_2_weight", "q_2_bias", "q_4_weight", "q_4_bias")


class TwinCritic:
    """The two Q-networks of the SAC agent (SB3 ContinuousCritic of MultiInputPolicy: q_i = Linear-ReLU-Linear-ReLU-Linear on
    achieved_goal | desired_goal | observation | action) on the host, float32, and the SAC target as include/urgym.h states it.
    `weights`: the two networks, each a mapping with CRITIC_ARRAYS (tests/golden/gen_critic_fixtures.py writes one file each)."""

    def __init__(self, weights):
        self.qf = [{k: np.asarray(dict(w)[k], dtype=np.float32) for k in CRITIC_ARRAYS} for w in weights]
        self.in_features = self.qf[0]["q_0_weight"].shape[1]

    @classmethod
    def load(cls, npz_paths):
        return cls([np.load(p) for p in npz_paths])

    def __call__(self, achieved_goal, desired_goal, observation, action):
        """(q0, q1), float32 [M] each."""
        x = np.concatenate([achieved_goal, desired_goal, observation, action], axis=1).astype(np.float32)
        assert x.shape[1] == self.in_features, (x.shape, self.in_features)
        out = []
        for w in self.qf:
            h = np.maximum(x @ w["q_0_weight"].T + w["q_0_bias"], 0.0)
            h = np.maximum(h @ w["q_2_weight"].T + w["q_2_bias"], 0.0)
            out.append((h @ w["q_4_weight"].T + w["q_4_bias"])[:, 0].astype(np.float32))
        return tuple(out)

    def action_gradient(self, achieved_goal, desired_goal, observation, action):
        """(dq_da [2, M, 6], dqmin_da [M, 6], q [2, M]) in float32 as include/urgym.h states urgym_critic_action_gradient:
        dq_da[i] = W0[:, action columns]^T D1 W1^T D2 w_q with D = diag(pre-activation > 0) -- a pre-activation of exactly 0 has
        derivative 0 -- and dqmin_da = dq_da[sel], sel = 1 where q_1 < q_0, else 0 (a tie takes qf0)."""
        x = np.concatenate([achieved_goal, desired_goal, observation, action], axis=1).astype(np.float32)
        assert x.shape[1] == self.in_features, (x.shape, self.in_features)
        f, zero = np.float32, np.float32(0.0)
        grads, qs = [], []
        for w in self.qf:
            z1 = x @ w["q_0_weight"].T + w["q_0_bias"]
            z2 = np.maximum(z1, zero) @ w["q_2_weight"].T + w["q_2_bias"]
            qs.append((np.maximum(z2, zero) @ w["q_4_weight"].T + w["q_4_bias"])[:, 0].astype(f))
            d2 = np.where(z2 > 0.0, w["q_4_weight"][0][None, :], zero).astype(f)
            d1 = np.where(z1 > 0.0, d2 @ w["q_2_weight"], zero).astype(f)
            grads.append((d1 @ w["q_0_weight"][:, self.in_features - 6:] + zero).astype(f))
        dq_da, q = np.stack(grads), np.stack(qs)
        dqmin_da = np.where((q[1] < q[0])[:, None], dq_da[1], dq_da[0])
        return dq_da, dqmin_da, q

    def parameter_gradients(self, achieved_goal, desired_goal, observation, action, dq=None, target=None, scale=None):
        """(grads, q) in float32 as include/urgym.h states urgym_critic_parameter_gradients: `grads` a list of two dicts keyed by
        CRITIC_ARRAYS, the gradients of a loss with d loss / d q_i[m] = dq[i][m] summed over the rows; q [2, M].  Exactly one of `dq`
        [2, M] and `target` [M] with `scale` is given; with `target`, dq = (q - target) * scale in two rounded float32 operations.
        A pre-activation of exactly 0 has derivative 0.  (The order of the sums is numpy's, not the kernel's.)"""
        if (dq is None) == (target is None):
            raise ValueError("exactly one of dq and target must be given")
        x = np.concatenate([achieved_goal, desired_goal, observation, action], axis=1).astype(np.float32)
        assert x.shape[1] == self.in_features, (x.shape, self.in_features)
        f, zero = np.float32, np.float32(0.0)
        grads, qs = [], []
        for i, w in enumerate(self.qf):
            z1 = x @ w["q_0_weight"].T + w["q_0_bias"]
            h1 = np.maximum(z1, zero)
            z2 = h1 @ w["q_2_weight"].T + w["q_2_bias"]
            h2 = np.maximum(z2, zero)
            q = (h2 @ w["q_4_weight"].T + w["q_4_bias"])[:, 0].astype(f)
            up = np.asarray(dq[i], f) if dq is not None else ((q - np.asarray(target, f)).astype(f) * f(scale)).astype(f)
            d2 = np.where(z2 > 0.0, up[:, None] * w["q_4_weight"][0][None, :], zero).astype(f)
            d1 = np.where(z1 > 0.0, d2 @ w["q_2_weight"], zero).astype(f)
            g = (d1.T @ x, d1.sum(axis=0), d2.T @ h1, d2.sum(axis=0), (up @ h2)[None, :], up.sum(keepdims=True))
            grads.append({k: np.asarray(v, dtype=f) for k, v in zip(CRITIC_ARRAYS, g)})
            qs.append(q)
        return grads, np.stack(qs)

    @staticmethod
    def target(q0, q1, reward, gamma, terminated=None, log_prob=None, ent_coef=0.0):
        """(q_min, target) in float32, operation by operation as urgym_critic_evaluate does:
        target = reward + ((gamma * not_done) * (q_min - (ent_coef * log_prob)))."""
        f = np.float32
        q_min = np.minimum(np.asarray(q0, f), np.asarray(q1, f))
        v = q_min
        if log_prob is not None:
            v = q_min - f(ent_coef) * np.asarray(log_prob, f)
        not_done = np.ones_like(q_min) if terminated is None else np.where(np.asarray(terminated).astype(bool), f(0), f(1))
        return q_min, (np.asarray(reward, f) + (f(gamma) * not_done) * v).astype(f)


class DeviceCritic:
    """The same two networks as ``TwinCritic``, evaluated by the HIP kernel of the extension (urgym_critic_create).  Belongs to the
    environment it was loaded for, like ``DeviceActor``; consumed by ``env.critic_values(critic, actions, ...)``."""

    def __init__(self, weights, env):
        import ctypes as C

        from . import _abi, _native

        weights = [dict(w) for w in weights]
        self.in_features, self.hidden_width = self.check_shapes(weights, env.env_kind)
        self.env = env
        desc = _abi.CriticDesc(self.in_features, self.hidden_width, 2, 0)
        keep = []  # copied by the library during the call
        for i, w in enumerate(weights):
            arrays = [np.ascontiguousarray(w[k], dtype=np.float32) for k in CRITIC_ARRAYS]
            keep.append(arrays)
            desc.qf[i] = _abi.QNetwork(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrays])
        self._c = C.c_void_p()
        _native.check(env.lib.urgym_critic_create(env._h, C.byref(desc), C.byref(self._c)), env._h)

    @classmethod
    def load(cls, npz_paths, env):
        return cls([np.load(p) for p in npz_paths], env)

    @staticmethod
    def check_shapes(weights, env_kind):
        """Raises ValueError unless `weights` is a pair of ``in -> H -> H -> 1`` networks the kernel supports for `env_kind`
        (in = obs_dim + 2 goal_dim + 6 of that env, one H for all four hidden layers, a multiple of 32 and at most 512).
        Returns (in_features, H).  Needs no GPU."""
        from . import _abi

        weights = list(weights)
        if len(weights) != 2:
            raise ValueError(f"a twin critic has two Q-networks, got {len(weights)}")
        obs_dim, goal_dim = _abi.OBS_DIMS[env_kind]
        want_in = obs_dim + 2 * goal_dim + 6
        widths = []
        for i, w in enumerate(weights):
            missing = [k for k in CRITIC_ARRAYS if k not in w]
            if missing:
                raise ValueError(f"qf{i}: critic arrays missing: {missing}")
            shape = {k: tuple(np.shape(w[k])) for k in CRITIC_ARRAYS}
            if any(len(shape[k]) != 2 for k in CRITIC_ARRAYS[0::2]) or any(len(shape[k]) != 1 for k in CRITIC_ARRAYS[1::2]):
                raise ValueError(f"qf{i}: critic weights must be 2-d and biases 1-d, got {shape}")
            (h0, in_features), (h1, h0_in), (out, h1_in) = shape["q_0_weight"], shape["q_2_weight"], shape["q_4_weight"]
            if in_features != want_in:
                raise ValueError(f"qf{i} takes {in_features} features, this env offers {want_in} (achieved_goal | desired_goal | observation | action)")
            if not (h0 == h1 == h0_in == h1_in):
                raise ValueError(f"qf{i}: the two hidden layers must have one width, got {shape}")
            if h0 % 32 != 0 or not 0 < h0 <= 512:
                raise ValueError(f"qf{i}: hidden width must be a multiple of 32 and at most 512, got {h0}")
            if out != 1:
                raise ValueError(f"qf{i} must have 1 output, got {out}")
            if shape["q_0_bias"] != (h0,) or shape["q_2_bias"] != (h0,) or shape["q_4_bias"] != (1,):
                raise ValueError(f"qf{i}: bias shapes do not match the weights: {shape}")
            widths.append(h0)
        if widths[0] != widths[1]:
            raise ValueError(f"both Q-networks must have one hidden width, got {widths}")
        return want_in, widths[0]

    @staticmethod
    def check_parameters(tensors, in_features, hidden_width, device):
        """Raises ValueError unless `tensors` is a pair of dicts under CRITIC_ARRAYS holding contiguous float32 torch tensors on
        `device` shaped for ``in_features -> hidden_width -> hidden_width -> 1`` networks.  Needs no GPU."""
        tensors = list(tensors)
        if len(tensors) != 2:
            raise ValueError(f"load_parameters: a twin critic has two Q-networks, got {len(tensors)}")
        n, H = int(in_features), int(hidden_width)
        wanted = dict(zip(CRITIC_ARRAYS, ((H, n), (H,), (H, H), (H,), (1, H), (1,))))
        for i, w in enumerate(tensors):
            missing = [k for k in CRITIC_ARRAYS if k not in w]
            if missing:
                raise ValueError(f"load_parameters: qf{i}: critic tensors missing: {missing}")
            unknown = [k for k in w if k not in CRITIC_ARRAYS]
            if unknown:
                raise ValueError(f"load_parameters: qf{i}: unknown critic tensors {unknown}; expected {CRITIC_ARRAYS}")
            _check_device_tensors(w, wanted, device, f"load_parameters: qf{i}")

    def load_parameters(self, tensors, tau=1.0):
        """Reloads both Q-networks from device tensors (urgym_critic_load), blending with what the critic holds: tau == 1 replaces,
        otherwise ``packed = (packed * (1 - tau)) + (tau * src)`` -- SAC's Polyak update of a target critic (``polyak`` restates
        it).  ONE launch on torch's current stream, nothing is synchronised; stream order as for ``DeviceActor.load_parameters``."""
        import ctypes as C

        from . import _abi, _native

        env = self.env
        tensors = [dict(w) for w in tensors]
        self.check_parameters(tensors, self.in_features, self.hidden_width, env.device)
        tau = float(tau)
        if not (np.isfinite(tau) and 0.0 < tau <= 1.0):
            raise ValueError(f"tau must be in (0, 1], got {tau}")
        p = _abi.CriticParamsDev(self.in_features, self.hidden_width, 0)
        for i, w in enumerate(tensors):
            p.qf[i] = _abi.QNetworkDev(*[C.cast(w[k].data_ptr(), C.POINTER(C.c_float)) for k in CRITIC_ARRAYS])
        _native.check(env.lib.urgym_critic_load(env._h, self._c, C.byref(p), tau, env._stream()), env._h)

    def parameters(self, out=None):
        """Both Q-networks' tensors as the packed buffer holds them (urgym_critic_unpack): a list of two dicts of device tensors
        under CRITIC_ARRAYS -- for a target critic, the Polyak average itself, which no torch tensor holds otherwise.  `out`: the
        tensors to write, checked as ``check_parameters`` checks sources; None = fresh ones.  ONE launch on torch's current
        stream, nothing is synchronised; stream order as for ``DeviceActor.parameters``."""
        import ctypes as C

        import torch

        from . import _abi, _native

        env, n, H = self.env, self.in_features, self.hidden_width
        if out is None:
            shapes = dict(zip(CRITIC_ARRAYS, ((H, n), (H,), (H, H), (H,), (1, H), (1,))))
            out = [{k: torch.empty(sh, dtype=torch.float32, device=env.device) for k, sh in shapes.items()} for _ in range(2)]
        out = [dict(w) for w in out]
        self.check_parameters(out, n, H, env.device)
        p = _abi.CriticParamsOut(n, H, 0)
        for i, w in enumerate(out):
            p.qf[i] = _abi.QNetworkOut(*[C.cast(w[k].data_ptr(), C.POINTER(C.c_float)) for k in CRITIC_ARRAYS])
        _native.check(env.lib.urgym_critic_unpack(env._h, self._c, C.byref(p), env._stream()), env._h)
        return out

    def packed(self):
        """The packed weight buffer of both networks as the kernel reads it (float32 numpy array; urgym_critic_read_packed).  A
        verification aid: synchronises the device."""
        return _read_packed(self.env, self.env.lib.urgym_critic_read_packed, self._c)

    def close(self):
        if getattr(self, "_c", None) and getattr(self.env, "_h", None):
            self.env.lib.urgym_critic_destroy(self.env._h, self._c)
        self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DEMO_OUT_OF_SCOPE = "demonstrations together with multi-step returns, prioritized replay or hindsight is out of scope"


class DeviceReplay:
    """SAC's replay buffer (train.py:40-48, SB3 DictReplayBuffer) as a ring of `capacity_steps` slots x N transitions in device
    memory, filled by ``collect`` (urgym_rollout_collect: the transitions are written as the rollout runs, terminal observations
    and goals included) and read by ``sample`` (urgym_replay_sample: one gather launch).  The ring tensors are ``self.ring[name]``
    ([C, N, ...]; _abi.REPLAY_RING_FIELDS).  ``cursor`` (the slot the next step goes to) and ``filled`` (valid slots) live on the
    host: pushes are host-driven, so both are known without a synchronisation.  ``terminated`` is the environment's own flag, not
    terminated | truncated: a time-limit end is bootstrapped through, as SB3 does (handle_timeout_termination)."""

    def __init__(self, env, capacity_steps):
        import ctypes as C

        import torch

        from . import _abi
        from .vector_env import _TORCH_DTYPE

        self.capacity = self.check_args(capacity_steps)
        self.env, self.cursor, self.filled = env, 0, 0
        self.ring = {}
        self._ring = _abi.ReplayRing(self.capacity, 0)
        for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS:
            t = torch.zeros(shape(self.capacity, env.num_envs, env.obs_dim, env.goal_dim), dtype=_TORCH_DTYPE[ct], device=env.device)
            self.ring[name] = t
            setattr(self._ring, name, C.cast(t.data_ptr(), C.POINTER(ct)))

    @staticmethod
    def check_args(capacity_steps, num_steps=None, first_slot=None, filled_steps=None, oldest_slot=None, batch_size=None):
        """Raises ValueError for what urgym_rollout_collect / urgym_replay_sample refuse about the ring's sizes (include/urgym.h):
        capacity_steps <= 0, num_steps <= 0, first_slot or oldest_slot outside [0, C), filled_steps outside [1, C], batch_size <= 0.
        Arguments left None are not checked.  Returns the capacity.  Needs no GPU."""
        def integer(name, v):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
            return int(v)

        cap = integer("capacity_steps", capacity_steps)
        if not 0 < cap < 1 << 31:
            raise ValueError(f"capacity_steps must be positive (and fit int32), got {cap}")
        if num_steps is not None and not 0 < integer("num_steps", num_steps) < 1 << 31:
            raise ValueError(f"num_steps must be positive, got {num_steps}")
        for name, v in (("first_slot", first_slot), ("oldest_slot", oldest_slot)):
            if v is not None and not 0 <= integer(name, v) < cap:
                raise ValueError(f"{name} must be in [0, {cap}), got {v}")
        if filled_steps is not None and not 1 <= integer("filled_steps", filled_steps) <= cap:
            raise ValueError(f"filled_steps must be in [1, {cap}] (nothing has been collected yet?), got {filled_steps}")
        if batch_size is not None and not 0 < integer("batch_size", batch_size) < 1 << 31:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        return cap

    @property
    def oldest_slot(self):
        return (self.cursor - self.filled) % self.capacity

    def __len__(self):
        return self.filled * self.env.num_envs

    def _geometry(self):
        env = self.env
        return dict(capacity=self.capacity, num_envs=env.num_envs, obs_dim=env.obs_dim, goal_dim=env.goal_dim)

    def state_dict(self, include_data=True):
        """The ring for a checkpoint: ``cursor``, ``filled``, the geometry, and under ``ring`` every tensor of
        ``_abi.REPLAY_RING_FIELDS`` as a host array of the ``filled`` valid slots, oldest first.  ``include_data=False`` leaves the
        tensors out: such a state loads as an empty ring.  Synchronises (device-to-host copies)."""
        import torch

        from . import _abi

        out = dict(self._geometry(), cursor=self.cursor, filled=self.filled, include_data=bool(include_data))
        if include_data:
            slots = torch.as_tensor([(self.oldest_slot + i) % self.capacity for i in range(self.filled)], dtype=torch.int64, device=self.env.device)
            whole = self.filled == self.capacity and self.oldest_slot == 0
            out["ring"] = {name: (self.ring[name] if whole else self.ring[name].index_select(0, slots)).cpu().numpy()
                           for name, _, _, _ in _abi.REPLAY_RING_FIELDS}
        return out

    def check_state_dict(self, state):
        """Raises ValueError unless `state` is a ``state_dict`` of a ring of this capacity and env shape.  Writes nothing."""
        from . import _abi

        for k, v in self._geometry().items():
            if int(state[k]) != v:
                raise ValueError(f"DeviceReplay.load_state_dict: {k} is {state[k]} in the state, {v} here")
        cursor, filled = int(state["cursor"]), int(state["filled"])
        if not (0 <= cursor < self.capacity and 0 <= filled <= self.capacity):
            raise ValueError(f"DeviceReplay.load_state_dict: cursor {cursor} or filled {filled} outside a ring of {self.capacity}")
        if state["include_data"]:
            env = self.env
            for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS:
                a, want = np.asarray(state["ring"][name]), (filled,) + tuple(shape(1, env.num_envs, env.obs_dim, env.goal_dim)[1:])
                if a.dtype != np.dtype(ct) or a.shape != want:
                    raise ValueError(f"DeviceReplay.load_state_dict: ring[{name!r}] must be {np.dtype(ct)} {want}, got {a.dtype} {a.shape}")

    def load_state_dict(self, state):
        """Restores what ``state_dict`` saved, every tensor to the slots it came from, so that ``oldest_slot`` and the index draw see
        the same ring.  A state without data leaves an empty ring (``filled == 0``) at the saved cursor.  A capacity or env-shape
        mismatch raises ValueError before anything is written."""
        import torch

        self.check_state_dict(state)
        cursor, filled = int(state["cursor"]), int(state["filled"])
        if not state["include_data"]:
            self.cursor, self.filled = cursor, 0
            return
        oldest = (cursor - filled) % self.capacity
        slots = torch.as_tensor([(oldest + i) % self.capacity for i in range(filled)], dtype=torch.int64, device=self.env.device)
        for name, t in self.ring.items():
            if filled:
                t.index_copy_(0, slots, torch.from_numpy(np.ascontiguousarray(state["ring"][name])).to(self.env.device))
        self.cursor, self.filled = cursor, filled

    def collect(self, actor, num_steps, sample=None, normalizer=None):
        """`num_steps` x (store pass, actor, step) from slot ``cursor`` on, without returning to Python; `sample` as in
        ``env.rollout_policy`` (None = the deterministic policy); `normalizer` as in ``env.collect`` (the actor reads normalized rows;
        nothing is folded here).  Advances ``cursor`` and ``filled``."""
        K = int(num_steps)
        self.env.collect(actor, K, self, sample=sample, first_slot=self.cursor, **({} if normalizer is None else dict(normalizer=normalizer)))
        self.cursor = (self.cursor + K) % self.capacity
        self.filled = min(self.capacity, self.filled + K)

    def collect_planned(self, planner, num_steps, first_draw=0, explore_sigma=0.0):
        """``collect`` with a planner as the policy: `num_steps` x (store pass, plan, execute, step) from slot ``cursor`` on in one native
        call (urgym_mppi_collect), `planner` a ``DeviceMPPI`` of this ring's environment; step t plans and explores with draw
        ``first_draw + t``, and the executed action is the plan's first action plus `explore_sigma` times the exploration noise, clamped.
        The slots are what a policy collection writes, so every gather, the monitor's fold and the normalizer's fold serve them as they
        are.  Advances ``cursor`` and ``filled``."""
        K = int(num_steps)
        planner.collect(self, K, first_draw=first_draw, explore_sigma=explore_sigma, first_slot=self.cursor)
        self.cursor = (self.cursor + K) % self.capacity
        self.filled = min(self.capacity, self.filled + K)

    def collect_scripted(self, controller, num_steps, first_draw=0, explore_sigma=0.0):
        """``collect`` with the scripted reach controller as the policy: `num_steps` x (store pass, controller action, step) from slot
        ``cursor`` on in one native call (urgym_controller_collect), `controller` a ``DeviceReachController`` of this ring's environment;
        step t draws its exploration noise with ``first_draw + t``.  The slots are what a policy collection writes.  Advances ``cursor``
        and ``filled`` as ``collect_planned`` does."""
        K = int(num_steps)
        controller.collect(self, K, first_draw=first_draw, explore_sigma=explore_sigma, first_slot=self.cursor)
        self.cursor = (self.cursor + K) % self.capacity
        self.filled = min(self.capacity, self.filled + K)

    def sample_into(self, out, seed, draw, n_steps=None, gamma=None, hindsight=None, demonstrations=None):
        """The gather itself: `out` maps ring field names (and ``index``, int64) to contiguous device tensors with one leading
        length, the batch size; only those are written.  The rows are ``replay_indices(seed, draw, count, len(self))``.

        With `n_steps` and `gamma` (both or neither) the launch is urgym_replay_sample_nstep: a row spans up to `n_steps` steps of
        its env (``nstep_batch``), `out` must hold ``discount`` (float32) and may hold ``steps`` (int32) and ``last_index`` (int64).

        With `hindsight` (a dict: ``threshold`` in [0, 2^32], ``strategy``, ``horizon``; not together with `n_steps`) the launch is
        urgym_replay_sample_hindsight (``hindsight_batch``): `out` may hold ``goal_index`` (int64) and ``pose_terms`` (float64 [count, 4]).

        With `demonstrations` = (other_replay, D) (not together with `n_steps` or `hindsight`) the launch is urgym_replay_sample_mixed
        (``env.replay_sample_mixed``): rows 0 .. D - 1 come from `other_replay`, a ``DeviceReplay`` of another env of the same kind with any
        env count, read at its own ``oldest_slot`` and ``filled``; `out` may hold ``source`` (uint8: 1 = a demonstration row).  The rows
        are ``mixed_entries``'."""
        import ctypes as C

        import torch

        from . import _abi, _native
        from .vector_env import _TORCH_DTYPE

        env = self.env
        kinds = {name: (ct, shape(1, 1, env.obs_dim, env.goal_dim)[2:]) for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
        kinds["index"] = (C.c_int64, ())
        if (n_steps is None) != (gamma is None):
            raise ValueError("n_steps and gamma go together")
        extra = {"discount": (C.c_float, ()), "steps": (C.c_int32, ()), "last_index": (C.c_int64, ())} if n_steps is not None else {}
        her = _abi.ReplayHindsight()
        if hindsight is not None:
            if n_steps is not None:
                raise ValueError("hindsight together with multi-step returns is out of scope")
            extra = {"goal_index": (C.c_int64, ()), "pose_terms": (C.c_double, (4,))}
            her.relabel_threshold, her.strategy, her.horizon = _her_arguments(hindsight["threshold"], hindsight["strategy"], hindsight["horizon"])
        if demonstrations is not None:
            if n_steps is not None or hindsight is not None:
                raise ValueError(DEMO_OUT_OF_SCOPE)
            extra = {"source": (C.c_uint8, ())}
        kinds.update(extra)
        dtypes = {C.c_int64: torch.int64, C.c_int32: torch.int32, C.c_double: torch.float64}
        batch, nstep, count = _abi.ReplayBatch(), _abi.ReplayNstep(), None
        for name, t in out.items():
            if name not in kinds:
                raise ValueError(f"unknown batch field {name!r}; available: {sorted(kinds)}")
            ct, tail = kinds[name]
            want = dtypes[ct] if ct in dtypes else _TORCH_DTYPE[ct]
            t = t.view(torch.uint8) if t.dtype == torch.bool else t
            if t.dtype != want or not t.is_contiguous() or t.device != env.device or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
                raise ValueError(f"{name} must be a contiguous {want} [count{''.join(f', {d}' for d in tail)}] tensor on {env.device}")
            if count is None:
                count = int(t.shape[0])
            elif int(t.shape[0]) != count:
                raise ValueError(f"{name} has {int(t.shape[0])} rows, the others {count}")
            if name == "source":
                continue
            setattr((nstep if hindsight is None else her) if name in extra else batch, name, C.cast(t.data_ptr(), C.POINTER(ct)))
        if count is None:
            raise ValueError("no output requested")
        self.check_args(self.capacity, filled_steps=self.filled, oldest_slot=self.oldest_slot, batch_size=count)
        if n_steps is not None:
            if isinstance(n_steps, bool) or int(n_steps) != n_steps or not 1 <= int(n_steps) <= _abi.REPLAY_NSTEP_MAX:
                raise ValueError(f"n_steps must be an integer in [1, {_abi.REPLAY_NSTEP_MAX}], got {n_steps!r}")
            if not abs(float(gamma)) < 3.4028235677973366e38:  # the first double that rounds to an infinite float32; refuses NaN too
                raise ValueError(f"gamma must be finite in float32, got {gamma}")
            if "discount" not in out:
                raise ValueError("with n_steps the batch needs discount")
            nstep.n_steps, nstep.gamma = int(n_steps), float(gamma)
            _native.check(env.lib.urgym_replay_sample_nstep(env._h, C.byref(self._ring), self.oldest_slot, self.filled, int(seed), int(draw), count,
                                                            C.byref(batch), C.byref(nstep), env._stream()), env._h)
            return
        if hindsight is not None:
            _native.check(env.lib.urgym_replay_sample_hindsight(env._h, C.byref(self._ring), self.oldest_slot, self.filled, int(seed), int(draw), count,
                                                                C.byref(batch), C.byref(her), env._stream()), env._h)
            return
        if demonstrations is not None:
            other, D = demonstrations
            env.replay_sample_mixed(self, other, D, seed, draw, count, batch, source=out.get("source"))
            return
        _native.check(env.lib.urgym_replay_sample(env._h, C.byref(self._ring), self.oldest_slot, self.filled, int(seed), int(draw), count,
                                                  C.byref(batch), env._stream()), env._h)

    def demonstrations_struct(self, count):
        """This ring as the urgym_replay_demonstrations of a mixed gather with `count` demonstration rows: read at its own ``oldest_slot``
        and ``filled``.  Raises ValueError for an empty ring or a negative count."""
        from . import _abi

        if isinstance(count, bool) or int(count) != count or not 0 <= int(count) < 1 << 31:
            raise ValueError(f"the number of demonstration rows must be an integer >= 0, got {count!r}")
        self.check_args(self.capacity, filled_steps=self.filled, oldest_slot=self.oldest_slot)
        return _abi.ReplayDemonstrations(self._ring, self.env.num_envs, self.oldest_slot, self.filled, int(count))

    def save(self, path):
        """The ring alone as one ``.npz`` (``checkpoint.write`` of ``state_dict()``): a demonstration set that outlives the process."""
        from . import checkpoint

        checkpoint.write(path, {"replay": self.state_dict()})

    def load_file(self, path):
        """Restores what ``save`` wrote into this ring (the same capacity and env shape, ``load_state_dict``)."""
        from . import checkpoint

        state = checkpoint.read(path)
        if not isinstance(state, dict) or "replay" not in state:
            raise ValueError(f"{path}: not a file of DeviceReplay.save (no 'replay' entry)")
        self.load_state_dict(state["replay"])

    def sample(self, batch_size, seed, draw, n_steps=None, gamma=None, demonstrations=None):
        """A minibatch of `batch_size` transitions drawn uniformly with replacement, one launch: a dict of fresh device tensors --
        ``observations`` and ``next_observations`` (each {observation, achieved_goal, desired_goal}: the `rows` of
        ``env.policy_actions`` / ``env.critic_values``), ``actions``, ``rewards``, ``terminated``, ``truncated``, ``is_success``
        (bool views) and ``index`` (int64: the flat ring entry slot * N + env of each row).  Nothing is synchronised.

        With `n_steps` and `gamma` the rows are multi-step transitions (``sample_into``): ``rewards`` is the discounted return over
        the m steps taken, ``next_observations`` and the flags are those of the last of them, and the dict also holds ``discount``
        (gamma^m, float32), ``steps`` (m, int32) and ``last_index`` (int64).

        With `demonstrations` = (other_replay, D) the first D rows come from `other_replay` (``sample_into``) and the dict also holds
        ``source`` (uint8 [batch_size]: 1 = a demonstration row); ``index`` of such a row is an entry of `other_replay`."""
        import ctypes as C

        import torch

        from . import _abi
        from .vector_env import _TORCH_DTYPE

        self.check_args(self.capacity, batch_size=batch_size)
        env, B = self.env, int(batch_size)
        flat = {name: torch.empty((B,) + tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:]), dtype=_TORCH_DTYPE[ct], device=env.device)
                for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
        flat["index"] = torch.empty((B,), dtype=torch.int64, device=env.device)
        if n_steps is not None:
            flat.update(discount=torch.empty((B,), dtype=torch.float32, device=env.device), steps=torch.empty((B,), dtype=torch.int32, device=env.device),
                        last_index=torch.empty((B,), dtype=torch.int64, device=env.device))
        if demonstrations is not None:
            flat["source"] = torch.empty((B,), dtype=torch.uint8, device=env.device)
        self.sample_into(flat, seed, draw, n_steps=n_steps, gamma=gamma, demonstrations=demonstrations)
        rows = ("observation", "achieved_goal", "desired_goal")
        more = {k: flat[k] for k in ("discount", "steps", "last_index")} if n_steps is not None else {}
        if demonstrations is not None:
            more["source"] = flat["source"]
        return {**more, "observations": {k: flat[k] for k in rows}, "next_observations": {k: flat["next_" + k] for k in rows},
                "actions": flat["action"], "rewards": flat["reward"], "terminated": flat["terminated"].view(torch.bool),
                "truncated": flat["truncated"].view(torch.bool), "is_success": flat["is_success"].view(torch.bool), "index": flat["index"]}

    def sample_hindsight(self, batch_size, seed, draw, n_sampled_goal=4, strategy="future", pose_terms=False):
        """``sample`` with hindsight experience replay (SB3's HerReplayBuffer; urgym_replay_sample_hindsight, ``hindsight_batch``), one
        launch: a share n_sampled_goal / (n_sampled_goal + 1) of the rows gets, as its goal, a pose its own episode reached at the
        same or a later step (`strategy` "future": uniform over them; "final": the episode's last; "own": the row's own goal, a
        diagnostic), and is re-scored against it with the task's reward.  The horizon is the env's ``max_episode_steps``.  The dict
        of ``sample`` plus ``goal_index`` (int64: the ring entry the goal came from, -1 = not relabelled) and, with `pose_terms`,
        ``pose_terms`` (float64 [batch_size, 4]: d, th, d0, th0).  Nothing is synchronised."""
        import torch

        from . import _abi
        from .vector_env import _TORCH_DTYPE

        self.check_args(self.capacity, batch_size=batch_size)
        env, B = self.env, int(batch_size)
        how = dict(threshold=relabel_threshold(n_sampled_goal), strategy=strategy, horizon=int(env.cfg.max_episode_steps))
        flat = {name: torch.empty((B,) + tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:]), dtype=_TORCH_DTYPE[ct], device=env.device)
                for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
        flat["index"] = torch.empty((B,), dtype=torch.int64, device=env.device)
        flat["goal_index"] = torch.empty((B,), dtype=torch.int64, device=env.device)
        if pose_terms:
            flat["pose_terms"] = torch.empty((B, 4), dtype=torch.float64, device=env.device)
        self.sample_into(flat, seed, draw, hindsight=how)
        rows = ("observation", "achieved_goal", "desired_goal")
        more = {k: flat[k] for k in ("goal_index", "pose_terms") if k in flat}
        return {**more, "observations": {k: flat[k] for k in rows}, "next_observations": {k: flat["next_" + k] for k in rows},
                "actions": flat["action"], "rewards": flat["reward"], "terminated": flat["terminated"].view(torch.bool),
                "truncated": flat["truncated"].view(torch.bool), "is_success": flat["is_success"].view(torch.bool), "index": flat["index"]}

    def sample_targets(self, actor, critic, batch_size, seed, draw, gamma, ent_coef, sample=None, n_steps=None, hindsight=None, normalizer=None,
                       demonstrations=None):
        """``sample``, then a' ~ pi(.|s') on the gathered next observations (``env.policy_actions(rows=)``), then SAC's target
        y = r + gamma (1 - terminated) (min_i Q_i(s', a') - ent_coef log pi(a'|s')) (``env.critic_values``): three launches.
        `sample` = how a' is drawn (default: gaussian with this call's seed and draw).  Returns the batch with ``next_actions``,
        ``next_log_prob`` and ``target`` added.

        With `n_steps` the batch is ``sample(..., n_steps=, gamma=)`` and the third launch writes the bootstrap value alone: the
        batch gets ``q_min_next`` = min_i Q_i(s', a') beside its ``discount`` instead of ``target`` (``env.entropy_step_nstep`` forms
        y from them); `ent_coef` is not used.

        With `normalizer` (a ``DeviceNormalizer``) the gathered batch is normalized in place right after the gather
        (``env.norm_batch``: one more launch); with `n_steps` the normalized reward is the row's accumulated return.

        With `demonstrations` = (other_replay, D) the batch is ``sample(..., demonstrations=)`` (not with `n_steps` or `hindsight`);
        demonstration rows are raw rows like any other and are normalized with the batch."""
        if demonstrations is not None and (hindsight is not None or n_steps is not None):
            raise ValueError(DEMO_OUT_OF_SCOPE)
        if hindsight is not None:  # dict(n_sampled_goal=, strategy=): the batch is ``sample_hindsight``'s, the rest as below
            if n_steps is not None:
                raise ValueError("hindsight together with multi-step returns is out of scope")
            batch = self.sample_hindsight(batch_size, seed, draw, **hindsight)
        else:
            batch = self.sample(batch_size, seed, draw, n_steps=n_steps, gamma=None if n_steps is None else gamma, demonstrations=demonstrations)
        if normalizer is not None:
            self.env.norm_batch(normalizer, batch)
        how = dict(mode="gaussian", seed=seed, first_draw=draw) if sample is None else sample
        nxt = batch["next_observations"]
        batch["next_actions"], batch["next_log_prob"] = self.env.policy_actions(actor, sample=how, rows=nxt)
        if n_steps is not None:
            batch["q_min_next"] = self.env.critic_values(critic, batch["next_actions"], rows=nxt)["q_min"]
            return batch
        batch["target"] = self.env.critic_values(critic, batch["next_actions"], rows=nxt, reward=batch["rewards"], terminated=batch["terminated"],
                                                 log_prob=batch["next_log_prob"], gamma=gamma, ent_coef=ent_coef)["target"]
        return batch


class DevicePrioritizedReplay(DeviceReplay):
    """``DeviceReplay`` with proportional priorities on the device (include/urgym.h, "prioritized replay"; urgym_per.h).  ``leaf``
    [C, N] float32 holds priority ** alpha per ring entry (0 = never drawn: unfilled slots are never sampled), ``sums`` the float64
    sum levels and the total (``per_sums(...)["flat"]``), ``max_leaf`` [1] what a new transition gets (1 at the start).  ``collect``
    also fills the slots it wrote; ``sample_prioritized`` draws through the sums (``per_descent``); ``terms`` forms the importance
    weights and the critics' weighted upstream gradient and writes the new priorities back (``per_terms``).  The sums are never
    saved: ``load_state_dict`` rebuilds them, bitwise what they were."""

    def __init__(self, env, capacity_steps, alpha=0.6, eps=1e-6):
        import ctypes as C

        import torch

        from . import _native

        super().__init__(env, capacity_steps)
        self.alpha, self.eps = self.check_per_args(alpha, eps)
        doubles = C.c_uint64(0)
        _native.check(env.lib.urgym_per_sums_count(env._h, self.capacity, C.byref(doubles)), env._h)
        self.leaf = torch.zeros((self.capacity, env.num_envs), dtype=torch.float32, device=env.device)
        self.sums = torch.zeros((int(doubles.value),), dtype=torch.float64, device=env.device)
        self.max_leaf = torch.ones((1,), dtype=torch.float32, device=env.device)
        self._pri = self.priorities_struct()

    def priorities_struct(self):
        import ctypes as C

        from . import _abi

        return _abi.PerPriorities(self.capacity, 0, C.cast(self.leaf.data_ptr(), C.POINTER(C.c_float)),
                                  C.cast(self.sums.data_ptr(), C.POINTER(C.c_double)), C.cast(self.max_leaf.data_ptr(), C.POINTER(C.c_float)))

    @staticmethod
    def check_per_args(alpha, eps):
        """Raises ValueError for what urgym_per_terms refuses about alpha (outside [0, 1]) and eps (not positive and finite in float32).
        Returns both as floats.  Needs no GPU."""
        a, e = np.float32(alpha), np.float32(eps)
        if not 0.0 <= a <= 1.0:
            raise ValueError(f"alpha must be in [0, 1], got {alpha}")
        if not (e > 0 and np.isfinite(e)):
            raise ValueError(f"eps must be positive and finite in float32, got {eps}")
        return float(alpha), float(eps)

    def state_dict(self, include_data=True):
        """``DeviceReplay.state_dict`` plus, under ``priorities``: alpha, eps, max_leaf and (with data) the leaves [C, N] as they lie.
        The sums are not saved."""
        out = super().state_dict(include_data)
        out["priorities"] = dict(alpha=self.alpha, eps=self.eps, max_leaf=self.max_leaf.cpu().numpy())
        if include_data:
            out["priorities"]["leaf"] = self.leaf.cpu().numpy()
        return out

    def check_state_dict(self, state):
        super().check_state_dict(state)
        pri = state.get("priorities")
        if pri is None:
            raise ValueError("DevicePrioritizedReplay.load_state_dict: the state holds no priorities (a uniform ring's?)")
        for k in ("alpha", "eps"):
            if float(pri[k]) != getattr(self, k):
                raise ValueError(f"DevicePrioritizedReplay.load_state_dict: {k} is {pri[k]} in the state, {getattr(self, k)} here")
        m = np.asarray(pri["max_leaf"])
        if m.dtype != np.float32 or m.shape != (1,):
            raise ValueError(f"DevicePrioritizedReplay.load_state_dict: max_leaf must be float32 [1], got {m.dtype} {m.shape}")
        if state["include_data"]:
            a = np.asarray(pri["leaf"])
            if a.dtype != np.float32 or a.shape != tuple(self.leaf.shape):
                raise ValueError(f"DevicePrioritizedReplay.load_state_dict: leaf must be float32 {tuple(self.leaf.shape)}, got {a.dtype} {a.shape}")

    def load_state_dict(self, state):
        """``DeviceReplay.load_state_dict``, then the leaves and max_leaf, then ``rebuild``: the sums are bitwise what they were.  A
        state without data leaves an empty structure (every leaf 0)."""
        import torch

        super().load_state_dict(state)
        pri = state["priorities"]
        self.max_leaf.copy_(torch.from_numpy(np.ascontiguousarray(pri["max_leaf"])))
        if state["include_data"]:
            self.leaf.copy_(torch.from_numpy(np.ascontiguousarray(pri["leaf"])))
        else:
            self.leaf.zero_()
        self.rebuild()

    def rebuild(self):
        """Every sum level and the total from the leaves as they lie (urgym_per_rebuild: two launches)."""
        import ctypes as C

        from . import _native

        env = self.env
        _native.check(env.lib.urgym_per_rebuild(env._h, C.byref(self._pri), env._stream()), env._h)

    def fill(self, first_slot, num_steps):
        """The leaves of `num_steps` slots from `first_slot` on become ``max_leaf`` and the sums are repaired (urgym_per_fill: two
        launches)."""
        import ctypes as C

        from . import _native

        env = self.env
        self.check_args(self.capacity, num_steps=num_steps, first_slot=first_slot)
        _native.check(env.lib.urgym_per_fill(env._h, C.byref(self._pri), int(first_slot), int(num_steps), env._stream()), env._h)

    def collect(self, actor, num_steps, sample=None, normalizer=None):
        """``DeviceReplay.collect``, then ``fill`` on the slots just written: a new transition is drawn at the largest priority seen."""
        first = self.cursor
        super().collect(actor, num_steps, sample=sample, normalizer=normalizer)
        self.fill(first, num_steps)

    def collect_planned(self, planner, num_steps, first_draw=0, explore_sigma=0.0):
        """``DeviceReplay.collect_planned``, then ``fill`` on the slots just written, as ``collect`` does."""
        first = self.cursor
        super().collect_planned(planner, num_steps, first_draw=first_draw, explore_sigma=explore_sigma)
        self.fill(first, num_steps)

    def collect_scripted(self, controller, num_steps, first_draw=0, explore_sigma=0.0):
        """``DeviceReplay.collect_scripted``, then ``fill`` on the slots just written, as ``collect`` does."""
        first = self.cursor
        super().collect_scripted(controller, num_steps, first_draw=first_draw, explore_sigma=explore_sigma)
        self.fill(first, num_steps)

    def sample_prioritized(self, batch_size, seed, draw):
        """``sample`` with each row drawn in proportion to its leaf, one launch (urgym_replay_sample_prioritized): the dict of
        ``sample`` plus ``leaf`` (float32 [B]: the leaf each row was drawn at) and ``total`` (float64 [1]).  The rows are
        ``per_descent(leaf, per_words(seed, draw, B))``.  Nothing is synchronised."""
        import ctypes as C

        import torch

        from . import _abi, _native
        from .vector_env import _TORCH_DTYPE

        self.check_args(self.capacity, batch_size=batch_size)
        env, B = self.env, int(batch_size)
        flat = {name: torch.empty((B,) + tuple(shape(1, 1, env.obs_dim, env.goal_dim)[2:]), dtype=_TORCH_DTYPE[ct], device=env.device)
                for name, ct, shape, _ in _abi.REPLAY_RING_FIELDS}
        batch = _abi.ReplayBatch()
        for name, ct, _, _ in _abi.REPLAY_RING_FIELDS:
            setattr(batch, name, C.cast(flat[name].data_ptr(), C.POINTER(ct)))
        index = torch.empty((B,), dtype=torch.int64, device=env.device)
        batch.index = C.cast(index.data_ptr(), C.POINTER(C.c_int64))
        leaf, total = torch.empty((B,), dtype=torch.float32, device=env.device), torch.empty((1,), dtype=torch.float64, device=env.device)
        _native.check(env.lib.urgym_replay_sample_prioritized(env._h, C.byref(self._ring), C.byref(self._pri), int(seed), int(draw), B, C.byref(batch),
                                                              leaf.data_ptr(), total.data_ptr(), env._stream()), env._h)
        rows = ("observation", "achieved_goal", "desired_goal")
        return {"observations": {k: flat[k] for k in rows}, "next_observations": {k: flat["next_" + k] for k in rows}, "actions": flat["action"],
                "rewards": flat["reward"], "terminated": flat["terminated"].view(torch.bool), "truncated": flat["truncated"].view(torch.bool),
                "is_success": flat["is_success"].view(torch.bool), "index": index, "leaf": leaf, "total": total}

    def terms(self, batch, q, y, beta, scale, write_back=True, out=None):
        """urgym_per_terms on a ``sample_prioritized`` batch: `q` float32 [2, B] (``env.critic_values`` of the batch rows), `y`
        float32 [B] (the target), `beta` and `scale` floats.  Returns (or fills `out`) ``w_raw``, ``w`` [B], ``dq`` [2, B] and, with
        `write_back`, ``new_leaf`` [B]; then the leaves of ``batch["index"]``, ``max_leaf`` and the sums are updated (three launches;
        one without `write_back`).  ``per_terms`` restates it."""
        import ctypes as C

        import torch

        from . import _abi, _native

        env, B = self.env, int(batch["index"].shape[0])
        fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
        want = {"q": (q, (2, B)), "y": (y, (B,)), "leaf": (batch["leaf"], (B,))}
        for name, (t, shape) in want.items():
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != env.device:
                raise ValueError(f"{name} must be a contiguous float32 {shape} tensor on {env.device}")
        out = {} if out is None else out
        for name, shape in (("w_raw", (B,)), ("w", (B,)), ("dq", (2, B))) + ((("new_leaf", (B,)),) if write_back else ()):
            if name not in out:
                out[name] = torch.empty(shape, dtype=torch.float32, device=env.device)
        a = _abi.PerTermsArgs(count=B, size=float(np.float32(self.filled * env.num_envs)), beta=float(beta), alpha=self.alpha, eps=self.eps,
                              scale=float(scale), leaf_in=fp(batch["leaf"]), total=C.cast(batch["total"].data_ptr(), C.POINTER(C.c_double)),
                              q=fp(q), y=fp(y), w_raw=fp(out["w_raw"]), w=fp(out["w"]), dq=fp(out["dq"]))
        if write_back:
            a.index, a.new_leaf = C.cast(batch["index"].data_ptr(), C.POINTER(C.c_int64)), fp(out["new_leaf"])
            a.priorities = self._pri
        _native.check(env.lib.urgym_per_terms(env._h, C.byref(a), env._stream()), env._h)
        return out


def run_closed_loop_device(env, actor, max_steps=100, normalizer=None):
    """``run_closed_loop`` with everything on the device: `env` is a UR5ReachVectorEnv (auto-reset off, like there), `actor` a
    DeviceActor of it.  One native call enqueues the max_steps x (actor, step) launches; the per-trial reward, success flag and
    last step come from the episode summary the launches keep (model_test.py:38-50).  Returns the same dictionary.  With `normalizer`
    (a ``DeviceNormalizer`` of an environment of this kind) the actor reads normalized rows, step by step from Python."""
    import torch

    if normalizer is not None:
        return _run_closed_loop_normalized(env, actor, normalizer, max_steps)
    rec = env.rollout_policy(actor, max_steps, record=("episode_return", "episode_last_step", "episode_success"))
    torch.cuda.synchronize(env.device)
    reward = rec["episode_return"].cpu().numpy()
    success = rec["episode_success"].cpu().numpy().astype(bool)
    last = rec["episode_last_step"].cpu().numpy().astype(np.float64)
    return {"success_rate_percent": 100.0 * success.mean(), "mean_episode_reward": float(reward.mean()),
            "mean_last_step_index": float(last.mean()), "success": success, "reward": reward, "last_step": last}


def _run_closed_loop_normalized(env, actor, normalizer, max_steps):
    """``run_closed_loop_device`` whose actor reads rows normalized with `normalizer`'s statistics as they stand (a ``DeviceNormalizer``,
    usually the TRAINING environment's: SB3's ``sync_envs_normalization``): a Python loop of ``env.norm_rows``, ``policy_actions(rows=)``
    and ``step``, three launches a step, with the episode of every env summed in float64 on the device as the rollout's summary sums
    it (model_test.py:42-49): rewards while the episode runs, closed at ``terminated`` or at the last step, success as that step reports."""
    import torch

    n, dev = env.num_envs, env.device
    ret = torch.zeros(n, dtype=torch.float64, device=dev)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    success = torch.zeros(n, dtype=torch.bool, device=dev)
    last = torch.full((n,), max_steps - 1, dtype=torch.int32, device=dev)
    for k in range(max_steps):
        rows = env.norm_rows(normalizer, {g: env.buf[g] for g in NORM_ROW_GROUPS})
        _, rew, term, trunc, info = env.step(env.policy_actions(actor, rows=rows))
        ret += torch.where(alive, rew.to(torch.float64), torch.zeros_like(ret))
        done = alive & (term | (k == max_steps - 1))
        success |= done & info["is_success"]
        last = torch.where(done, torch.full_like(last, k), last)
        alive &= ~done
    torch.cuda.synchronize(dev)
    reward, ok, last = ret.cpu().numpy(), success.cpu().numpy().astype(bool), last.cpu().numpy().astype(np.float64)
    return {"success_rate_percent": 100.0 * ok.mean(), "mean_episode_reward": float(reward.mean()), "mean_last_step_index": float(last.mean()),
            "success": ok, "reward": reward, "last_step": last}


# ------------------------------------------------------------------------------------------------ evaluation inside the training call
def evaluation_stats(returns, last_step, success, best_mean, best_index, eval_index):
    """THE STATISTICS of include/urgym.h ("evaluation inside the training call") in numpy, bitwise what urgym_eval_stats writes:
    `returns` float64 [N], `last_step` int32 [N], `success` uint8 or bool [N]; every line one float64 operation.  Returns a dict with
    the fields of ``urgym_eval_record`` (and ``std_return = sqrt(var_return)``, which the device does not compute) and the best state
    afterwards under ``best_mean`` and ``best_index``."""
    r, last, succ = np.asarray(returns), np.asarray(last_step), np.asarray(success)
    if r.dtype != np.float64 or r.ndim != 1 or r.size < 1:
        raise ValueError(f"returns must be a float64 [N] array with N >= 1, got {r.dtype} {r.shape}")
    if last.dtype != np.int32 or last.shape != r.shape:
        raise ValueError(f"last_step must be an int32 {r.shape} array, got {last.dtype} {last.shape}")
    if succ.dtype not in (np.dtype(np.uint8), np.dtype(bool)) or succ.shape != r.shape:
        raise ValueError(f"success must be a uint8 or bool {r.shape} array, got {succ.dtype} {succ.shape}")
    n = np.float64(r.size)
    with np.errstate(all="ignore"):
        mean = ordered_sum(r, np.float64) / n
        d = r - mean
        var = ordered_sum(d * d, np.float64) / n
        length_sum = int(last.astype(np.int64).sum()) + r.size
        successes = int(np.count_nonzero(succ))
        mean_length = np.float64(length_sum) / n
        success_rate = np.float64(successes) / n
        improved = bool(mean > np.float64(best_mean))  # strict; False for a NaN mean
        std = np.sqrt(var)
    best_mean, best_index = (mean, int(eval_index)) if improved else (np.float64(best_mean), int(best_index))
    return dict(mean_return=mean, var_return=var, mean_length=mean_length, success_rate=success_rate, best_mean_after=best_mean,
                eval_index=int(eval_index), length_sum=length_sum, successes=successes, count=int(r.size), improved=int(improved), reserved0=0,
                std_return=std, best_mean=best_mean, best_index=best_index)


def evaluation_points(first_step, iterations, updates_per_iteration, idle_iterations, every):
    """The iterations of a ``SACLearner.train(..., evaluation=, eval_every=every)`` call that are followed by an evaluation
    (ur_gym_amd/csrc/urgym_eval_schedule.h): with s_i = first_step - 1 + G (the iterations among 0..i that are not idle), iteration i
    where ``s_i // every > s_{i-1} // every`` -- the update count passes a multiple of `every` in it.  `first_step`: the 1-based Adam
    step of the call's first update."""
    first, n, G, idle, E = int(first_step), int(iterations), int(updates_per_iteration), int(idle_iterations), int(every)
    if first < 1 or n < 1 or G < 0 or idle < 0 or E < 1:
        raise ValueError(f"evaluation_points: first_step >= 1, iterations >= 1, updates_per_iteration >= 0, idle_iterations >= 0 and every >= 1, got "
                         f"{(first_step, iterations, updates_per_iteration, idle_iterations, every)}")
    after = lambda i: first - 1 + G * max(0, i + 1 - idle)  # noqa: E731
    return [i for i in range(n) if after(i) // E > after(i - 1) // E]


class DeviceEvaluation:
    """The EvalCallback of the reference's train.py:55-60 on the device: an evaluation environment (`test_env`, auto_reset off, at most
    65536 envs), a DeviceActor on it, the episode scratch, `capacity` evaluation records, the best actor's tensors and the best state
    (mean ``-inf``, index ``-1`` until an evaluation improves).  `actor_tensors_like`: a dict under ACTOR_ARRAYS + LOG_STD_ARRAYS (torch
    tensors or arrays) that gives the shape and the eval actor's first weights.  Every evaluation zeroes `test_env`'s observation
    buffer and resets it with `seed` -- ``reset(seed=)`` as a fresh environment answers it: on UR5DynReach-v1 a reset keeps the
    velocity slot of the observation it finds -- so that all of them play the same episodes, and runs `num_steps` steps (default: the
    env's max_episode_steps).  With `normalizer` (the TRAINING environment's ``DeviceNormalizer``, of the same env kind and device) every
    evaluation runs its actor on rows normalized with those statistics as they stand when it runs (urgym_policy_evaluate_normalized:
    SB3's ``sync_envs_normalization``), and an evaluation that improves also snapshots the statistics into ``best_norm``, which
    ``save_best`` writes beside the actor under ``norm/...`` keys (``load_best_normalization`` reads them back)."""

    def __init__(self, test_env, actor_tensors_like, num_steps=None, seed=0, capacity=64, normalizer=None):
        import torch

        from . import _abi

        if test_env.cfg.auto_reset:
            raise ValueError("DeviceEvaluation: test_env must be made with auto_reset=False (whole first episodes are summarised)")
        if test_env.num_envs > _abi.EVAL_MAX_COUNT:
            raise ValueError(f"DeviceEvaluation: at most {_abi.EVAL_MAX_COUNT} evaluation envs, got {test_env.num_envs}")
        like = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in dict(actor_tensors_like).items()}
        missing = [k for k in ACTOR_ARRAYS + LOG_STD_ARRAYS if k not in like]
        if missing:
            raise ValueError(f"DeviceEvaluation: actor_tensors_like needs all of {ACTOR_ARRAYS + LOG_STD_ARRAYS}; missing {missing}")
        self.env, self.seed = test_env, int(seed)
        self.num_steps = int(test_env.cfg.max_episode_steps if num_steps is None else num_steps)
        self.capacity = int(capacity)
        if self.num_steps < 1 or self.capacity < 1:
            raise ValueError("DeviceEvaluation: num_steps and capacity must be at least 1")
        self.actor = DeviceActor({k: like[k].astype(np.float32) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS}, test_env)
        dev, N = test_env.device, test_env.num_envs
        self.scratch = dict(episode_return=torch.zeros(N, dtype=torch.float64, device=dev), episode_last_step=torch.zeros(N, dtype=torch.int32, device=dev),
                            episode_success=torch.zeros(N, dtype=torch.uint8, device=dev), episode_done=torch.zeros(N, dtype=torch.uint8, device=dev))
        self.records = torch.zeros((self.capacity, _abi.EVAL_RECORD_WORDS), dtype=torch.int64, device=dev)  # [capacity] urgym_eval_record
        self.best = {k: torch.zeros(like[k].shape, dtype=torch.float32, device=dev) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS}
        self.best_mean = torch.full((1,), -np.inf, dtype=torch.float64, device=dev)
        self.best_index = torch.full((1,), -1, dtype=torch.int64, device=dev)
        self.count = 0   # evaluations made: the next one's eval_index and record slot
        self._struct = self._source = None
        self.normalizer = self.best_norm = self._norm_struct = None
        if normalizer is not None:
            import ctypes as C

            other = getattr(normalizer, "env", None)
            if not isinstance(normalizer, DeviceNormalizer) or other.env_kind != test_env.env_kind or other.device != test_env.device:
                raise ValueError("DeviceEvaluation: normalizer must be a DeviceNormalizer of an environment of test_env's kind and device")
            self.normalizer = normalizer
            self.eval_scratch = torch.zeros((N * (test_env.obs_dim + 2 * test_env.goal_dim),), dtype=torch.float32, device=dev)
            self.best_norm = {k: torch.from_numpy(a).to(dev) for k, a in norm_initial_state(1, test_env.obs_dim, test_env.goal_dim).items() if k != "running_ret"}
            self._best_norm_struct = _abi.NormState()
            for k, t in self.best_norm.items():
                setattr(self._best_norm_struct, k, C.cast(t.data_ptr(), C.POINTER(C.c_double)))

    def struct(self, tensors):
        """The checked ``urgym_policy_evaluation`` for the source `tensors` (a dict of device tensors as ``DeviceActor.check_parameters``
        takes them, with the log_std head); rebuilt only when another set of tensors is handed in."""
        import ctypes as C

        from . import _abi

        keys = ACTOR_ARRAYS + LOG_STD_ARRAYS
        ptrs = tuple(tensors[k].data_ptr() for k in keys) if all(k in tensors for k in keys) else None
        if self._struct is not None and ptrs is not None and ptrs == self._source:
            return self._struct
        a, env = self.actor, self.env
        if not DeviceActor.check_parameters(dict(tensors), a.in_features, a.hidden_width, env.device):
            raise ValueError(f"DeviceEvaluation: the source needs the log_std head too ({LOG_STD_ARRAYS})")
        fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
        E = _abi.PolicyEvaluation()
        E.eval_actor, E.in_features, E.hidden_width = a._a, a.in_features, a.hidden_width
        E.source = _abi.ActorTensors(*[fp(tensors[k]) for k in keys])
        E.best = _abi.ActorTensors(*[fp(self.best[k]) for k in keys])
        sc = self.scratch
        E.episode_return = C.cast(sc["episode_return"].data_ptr(), C.POINTER(C.c_double))
        E.episode_last_step = C.cast(sc["episode_last_step"].data_ptr(), C.POINTER(C.c_int32))
        E.episode_success = C.cast(sc["episode_success"].data_ptr(), C.POINTER(C.c_uint8))
        E.episode_done = C.cast(sc["episode_done"].data_ptr(), C.POINTER(C.c_uint8))
        E.records = C.cast(self.records.data_ptr(), C.POINTER(_abi.EvalRecord))
        E.best_mean = C.cast(self.best_mean.data_ptr(), C.POINTER(C.c_double))
        E.best_index = C.cast(self.best_index.data_ptr(), C.POINTER(C.c_int64))
        E.reset_seed, E.record_capacity, E.num_steps, E.reserved0 = self.seed, self.capacity, self.num_steps, 0
        self._struct, self._source, self._keep = E, ptrs, dict(tensors)
        return E

    def norm_struct(self):
        """The ``urgym_normalization`` of an evaluation with this object: the normalizer's as it stands, with ``eval_scratch`` and
        ``best_state`` set.  None without a normalizer."""
        import ctypes as C

        from . import _abi

        if self.normalizer is None:
            return None
        Z = _abi.Normalization.from_buffer_copy(bytes(self.normalizer.struct()))
        Z.eval_scratch = C.cast(self.eval_scratch.data_ptr(), C.POINTER(C.c_float))
        Z.best_state = C.pointer(self._best_norm_struct)
        self._norm_struct = Z
        return Z

    def advance(self, evaluations):
        """What a native call that made `evaluations` evaluations leaves behind on the host side: the counters, and the environment's
        own bookkeeping of ``reset(seed=)``."""
        if evaluations:
            self.count += int(evaluations)
            self.actor.has_log_std = True
            self.env._seed, self.env._needs_reset = self.seed, False

    def evaluate(self, tensors):
        """One evaluation of the actor whose parameters are `tensors` (urgym_policy_evaluate): reload, ``reset(seed=)``, `num_steps`
        steps of the deterministic policy, the statistics into the next record, and the copy into the best tensors where the mean
        return is strictly above the best so far.  On torch's current stream; NOT synchronised.  Returns the record's index."""
        import ctypes as C

        from . import _native

        if self.count >= self.capacity:
            raise ValueError(f"DeviceEvaluation: all {self.capacity} records are used")
        env, slot = self.env, self.count
        if self.normalizer is not None:
            _native.check(env.lib.urgym_policy_evaluate_normalized(env._h, C.byref(self.struct(tensors)), C.byref(self.norm_struct()), slot, slot, env._stream()), env._h)
        else:
            _native.check(env.lib.urgym_policy_evaluate(env._h, C.byref(self.struct(tensors)), slot, slot, env._stream()), env._h)
        self.advance(1)
        return slot

    def results(self):
        """Synchronises; one dict per evaluation made, with the record's fields and ``std_return = sqrt(var_return)``."""
        import ctypes as C

        import torch

        from . import _abi

        torch.cuda.synchronize(self.env.device)
        raw = self.records[:self.count].cpu().numpy().tobytes()
        out = []
        for i in range(self.count):
            rec = _abi.EvalRecord.from_buffer_copy(raw, i * C.sizeof(_abi.EvalRecord))
            d = {name: getattr(rec, name) for name, _ in _abi.EvalRecord._fields_}
            with np.errstate(all="ignore"):
                d["std_return"] = float(np.sqrt(np.float64(d["var_return"])))
            out.append(d)
        return out

    def best_state(self):
        """(best mean return, index of the evaluation that reached it); synchronises."""
        return float(self.best_mean.cpu()[0]), int(self.best_index.cpu()[0])

    def best_parameters(self):
        """The best actor's tensors (device tensors under ACTOR_ARRAYS + LOG_STD_ARRAYS): zeros until an evaluation has improved."""
        return self.best

    def save_best(self, path):
        """Writes the best actor as an ``.npz`` under ACTOR_ARRAYS + LOG_STD_ARRAYS: what ``DeviceActor.load`` and
        ``DeterministicActor.load`` read.  With a normalizer the file also holds the statistics the best actor was selected under, as
        float64 arrays under ``norm/<field>`` (the twelve of ``best_norm``) and the options under ``norm/options`` (gamma, epsilon,
        clip_obs, clip_reward, norm_obs, norm_reward as float64): ``load_best_normalization`` reads them.  Without one the file is what it
        always was.  Synchronises."""
        extra, normalizer = None, getattr(self, "normalizer", None)
        if normalizer is not None:
            o = normalizer.options
            extra = {"norm/" + k: v.cpu().numpy() for k, v in self.best_norm.items()}
            extra["norm/options"] = np.array([o["gamma"], o["epsilon"], o["clip_obs"], o["clip_reward"], float(o["norm_obs"]), float(o["norm_reward"])], np.float64)
        save_actor(path, self.best, extra)

    def state_dict(self):
        """The evaluation for a checkpoint: the records written so far, the best actor's tensors, ``best_mean``, ``best_index`` and
        ``count``; ``seed`` and ``num_steps``, which a load checks; and the evaluation environment's ``checkpoint_state`` (its sticky
        status words are the only thing of it that an evaluation does not rewrite).  Synchronises."""
        out = dict(seed=self.seed, num_steps=self.num_steps, count=self.count, records=self.records[:self.count].cpu().numpy(),
                   best={k: v.cpu().numpy() for k, v in self.best.items()}, best_mean=self.best_mean.cpu().numpy(),
                   best_index=self.best_index.cpu().numpy(), env=self.env.checkpoint_state())
        if getattr(self, "normalizer", None) is not None:  # an evaluation without a normalizer gains no key
            out["best_norm"] = {k: v.cpu().numpy() for k, v in self.best_norm.items()}
        return out

    def load_state_dict(self, state):
        """Restores what ``state_dict`` saved, in place (a ``struct`` made earlier stays valid).  Raises ValueError, before anything
        is written, for another seed, episode length, actor shape or environment, or more records than this evaluation's capacity."""
        import torch

        from . import _abi

        count, records = int(state["count"]), np.asarray(state["records"])
        if int(state["seed"]) != self.seed or int(state["num_steps"]) != self.num_steps:
            raise ValueError(f"DeviceEvaluation.load_state_dict: the state evaluates with seed {state['seed']} for {state['num_steps']} steps, "
                             f"this evaluation with seed {self.seed} for {self.num_steps}")
        if not 0 <= count <= self.capacity or records.shape != (count, _abi.EVAL_RECORD_WORDS) or records.dtype != np.int64:
            raise ValueError(f"DeviceEvaluation.load_state_dict: {count} records ({records.dtype} {records.shape}) do not fit a capacity of {self.capacity}")
        best = {k: np.asarray(state["best"][k]) for k in ACTOR_ARRAYS + LOG_STD_ARRAYS}
        for k, v in best.items():
            if v.dtype != np.float32 or v.shape != tuple(self.best[k].shape):
                raise ValueError(f"DeviceEvaluation.load_state_dict: best[{k!r}] must be float32 {tuple(self.best[k].shape)}, got {v.dtype} {v.shape}")
        normalizer = getattr(self, "normalizer", None)
        if (state.get("best_norm") is None) != (normalizer is None):
            raise ValueError("DeviceEvaluation.load_state_dict: the best statistics are in the state and this evaluation has no normalizer, or the reverse")
        best_norm = None
        if normalizer is not None:
            best_norm = {k: np.asarray(state["best_norm"][k]) for k in self.best_norm}
            for k, v in best_norm.items():
                if v.dtype != np.float64 or v.shape != tuple(self.best_norm[k].shape):
                    raise ValueError(f"DeviceEvaluation.load_state_dict: best_norm[{k!r}] must be float64 {tuple(self.best_norm[k].shape)}, got {v.dtype} {v.shape}")
        self.env.check_checkpoint(state["env"])
        for k, v in (best_norm or {}).items():
            self.best_norm[k].copy_(torch.from_numpy(v))
        for k, v in best.items():
            self.best[k].copy_(torch.from_numpy(v))
        self.best_mean.copy_(torch.from_numpy(np.asarray(state["best_mean"], dtype=np.float64).reshape(1)))
        self.best_index.copy_(torch.from_numpy(np.asarray(state["best_index"], dtype=np.int64).reshape(1)))
        self.records.zero_()
        self.records[:count].copy_(torch.from_numpy(np.ascontiguousarray(records)))
        self.env.restore_checkpoint(state["env"])
        self.count = count
        if count:
            self.actor.has_log_std = True

    def close(self):
        self._struct = self._source = None
        self.actor.close()


def load_best_normalization(path):
    """The statistics ``DeviceEvaluation.save_best`` wrote beside the best actor: ``(state, options)`` -- the twelve float64 arrays under
    the names of ``_abi.NORM_STATE_FIELDS`` (no ``running_ret``) and a dict of the options -- or None for a file that holds none."""
    with np.load(path, allow_pickle=False) as f:
        keys = [k for k in f.files if k.startswith("norm/")]
        if not keys:
            return None
        state = {k[len("norm/"):]: np.array(f[k]) for k in keys if k != "norm/options"}
        o = np.array(f["norm/options"])
    return state, dict(gamma=float(o[0]), epsilon=float(o[1]), clip_obs=float(o[2]), clip_reward=float(o[3]), norm_obs=bool(o[4]), norm_reward=bool(o[5]))


def save_actor(path, tensors, extra=None):
    """An actor's ten arrays (device tensors or arrays under ACTOR_ARRAYS + LOG_STD_ARRAYS) as an ``.npz`` ``DeviceActor.load`` and
    ``DeterministicActor.load`` read back bitwise; `extra`: further arrays under names of their own."""
    arrays = dict(extra or {})
    for k in ACTOR_ARRAYS + LOG_STD_ARRAYS:
        v = tensors[k]
        arrays[k] = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
    with open(path, "wb") as f:  # a file object: np.savez appends no suffix of its own
        np.savez(f, **arrays)


# ------------------------------------------------------------------------------------------------ training-episode statistics (the Monitor)
def _monitor_arrays(state):
    """A copy of `state` (a dict under ``_abi.MONITOR_STATE_FIELDS`` of [N] arrays) with every dtype and shape checked."""
    from . import _abi

    names = [name for name, _ in _abi.MONITOR_STATE_FIELDS]
    if not isinstance(state, dict) or sorted(state) != sorted(names):
        raise ValueError(f"state must be a dict under {names}")
    out, n = {}, None
    for name, ct in _abi.MONITOR_STATE_FIELDS:
        a, want = np.asarray(state[name]), np.dtype(ct)
        n = a.shape if n is None else n
        if a.dtype != want or a.ndim != 1 or a.shape != n:
            raise ValueError(f"state[{name!r}] must be a {want} [N] array, got {a.dtype} {a.shape}")
        out[name] = a.copy()
    return out


def monitor_fold(state, reward, terminated, truncated, is_success, first_slot, num_steps):
    """THE FOLD of include/urgym.h ("training-episode statistics on the device") in numpy, bitwise what urgym_monitor_fold leaves:
    `state` a dict under ``_abi.MONITOR_STATE_FIELDS`` of [N] arrays; `reward` float32 [C, N] and the three flags uint8 or bool [C, N],
    the ring's tensors; the steps k = 0 .. num_steps - 1 are read in order from slot (first_slot + k) % C.  Every line is one operation,
    in float64 where a float is involved.  Returns the new state (the argument is not written)."""
    from . import _abi

    st = _monitor_arrays(state)
    r = np.asarray(reward)
    flags = [np.asarray(x) for x in (terminated, truncated, is_success)]
    n = st["running_return"].shape[0]
    if r.dtype != np.float32 or r.ndim != 2 or r.shape[1] != n:
        raise ValueError(f"reward must be a float32 [C, {n}] array, got {r.dtype} {r.shape}")
    for name, x in zip(("terminated", "truncated", "is_success"), flags):
        if x.dtype not in (np.dtype(np.uint8), np.dtype(bool)) or x.shape != r.shape:
            raise ValueError(f"{name} must be a uint8 or bool {r.shape} array, got {x.dtype} {x.shape}")
    cap, first, K = r.shape[0], int(first_slot), int(num_steps)
    if not 0 <= first < cap or not 1 <= K <= cap:
        raise ValueError(f"first_slot must be in [0, {cap}) and num_steps in [1, {cap}], got {first_slot} and {num_steps}")
    term, trunc, succ = (x.view(np.uint8) if x.dtype == bool else x for x in flags)
    with np.errstate(all="ignore"):
        for k in range(K):
            s = (first + k) % cap
            running = st["running_return"] + r[s].astype(np.float64)
            length = st["running_length"] + np.int32(1)
            done = (term[s] | trunc[s]) != 0
            st["sum_return"] = np.where(done, st["sum_return"] + running, st["sum_return"])
            st["sum_length"] = np.where(done, st["sum_length"] + length.astype(np.int64), st["sum_length"])
            st["episodes"] = np.where(done, st["episodes"] + np.int32(1), st["episodes"])
            st["successes"] = np.where(done, st["successes"] + (succ[s] != 0).astype(np.int32), st["successes"])
            st["running_return"] = np.where(done, np.float64(0.0), running)
            st["running_length"] = np.where(done, np.int32(0), length)
    for name, ct in _abi.MONITOR_STATE_FIELDS:
        assert st[name].dtype == np.dtype(ct), (name, st[name].dtype)  # no intermediate was promoted
    return st


def monitor_stats(state, iteration, clear=True):
    """THE RECORD of include/urgym.h ("training-episode statistics on the device") in numpy, bitwise what urgym_monitor_stats writes:
    the exact integer sums, the ordered sum of ``sum_return`` in float64, the three quotients (one division each; ``+0.0`` where no
    episode finished).  Returns ``(record, state)``: a dict with the fields of ``urgym_monitor_record``, and the state afterwards -- with
    `clear` its four interval arrays zeroed, the episode in progress untouched (the argument is not written)."""
    st = _monitor_arrays(state)
    episodes = int(st["episodes"].astype(np.int64).sum())
    length_sum = int(st["sum_length"].sum())
    successes = int(st["successes"].astype(np.int64).sum())
    with np.errstate(all="ignore"):
        sum_r = ordered_sum(st["sum_return"], np.float64)
        zero = np.float64(0.0)
        e = np.float64(episodes)
        mean_return = sum_r / e if episodes else zero
        mean_length = np.float64(length_sum) / e if episodes else zero
        success_rate = np.float64(successes) / e if episodes else zero
    if clear:
        for name in ("sum_return", "sum_length", "episodes", "successes"):
            st[name] = np.zeros_like(st[name])
    rec = dict(mean_return=mean_return, mean_length=mean_length, success_rate=success_rate, sum_return=sum_r, episodes=episodes, length_sum=length_sum,
               successes=successes, iteration=int(iteration), reserved0=0)
    return rec, st


def monitor_points(first_iteration, iterations, log_every):
    """The iterations i of a ``SACLearner.train(..., monitor=, log_every=)`` call of `iterations` iterations that are followed by a record
    (ur_gym_amd/csrc/urgym_monitor.h): those where ``(first_iteration + i + 1) % log_every == 0`` -- the monitor's count of iterations,
    that one included, reaches a multiple of `log_every`.  `first_iteration`: the count before the call."""
    first, n, E = int(first_iteration), int(iterations), int(log_every)
    if first < 0 or n < 0 or E < 1:
        raise ValueError(f"monitor_points: first_iteration >= 0, iterations >= 0 and log_every >= 1, got {(first_iteration, iterations, log_every)}")
    return [i for i in range(n) if (first + i + 1) % E == 0]


class DeviceMonitor:
    """The ``Monitor(env, log_dir)`` of the reference's train.py:52 on the device: per env the return and the length of the episode the
    COLLECTING policy is playing and the episodes it finished since the last record, read from the replay ring the collection has just
    written; and `capacity` records of them (SB3's rollout/ep_rew_mean, rollout/ep_len_mean, rollout/success_rate), each over the
    episodes finished since the record before it (``clear=False``: since the start).  `env`: a UR5ReachVectorEnv with auto_reset.
    ``iterations`` (training iterations seen) and ``count`` (records written) live on the host: ``SACLearner.train`` advances them, so
    that split calls place records where one call would."""

    def __init__(self, env, capacity=64, clear=True):
        import ctypes as C

        import torch

        from . import _abi
        from .vector_env import _TORCH_DTYPE

        if not env.cfg.auto_reset:
            raise ValueError("DeviceMonitor: env must be made with auto_reset=True (the episodes of an env that is not reset do not restart)")
        self.env, self.capacity, self.clear = env, int(capacity), bool(clear)
        if self.capacity < 1:
            raise ValueError("DeviceMonitor: capacity must be at least 1")
        self.state = {name: torch.zeros(env.num_envs, dtype=torch.int64 if ct is C.c_int64 else _TORCH_DTYPE[ct], device=env.device)
                      for name, ct in _abi.MONITOR_STATE_FIELDS}
        self.records = torch.zeros((self.capacity, _abi.MONITOR_RECORD_WORDS), dtype=torch.int64, device=env.device)  # [capacity] urgym_monitor_record
        self.count = 0       # records written: the next one's slot
        self.iterations = 0  # training iterations train() has run with this monitor
        self._struct = None

    def struct(self, log_every):
        """The ``urgym_sac_monitoring`` of the next ``env.sac_train`` call: the state, the records from the cursor on, the count so far."""
        import ctypes as C

        from . import _abi

        if self._struct is None:
            M = _abi.SacMonitoring()
            M.state = self.env._monitor_state("DeviceMonitor", self.state)
            M.records = C.cast(self.records.data_ptr(), C.POINTER(_abi.MonitorRecord))
            M.record_capacity, M.reserved0 = self.capacity, 0
            self._struct = M
        M = self._struct
        M.first_record, M.log_every, M.clear, M.first_iteration = self.count, int(log_every), int(self.clear), self.iterations
        return M

    def advance(self, iterations, records):
        """What a native call of `iterations` iterations that wrote `records` records leaves behind on the host side."""
        self.iterations += int(iterations)
        self.count += int(records)

    def state_dict(self):
        """The monitor for a checkpoint: the per-env running state, the records written so far, ``iterations`` and ``count`` (and
        ``num_envs`` and ``clear``, which a load checks).  Synchronises."""
        return dict(num_envs=self.env.num_envs, clear=self.clear, iterations=self.iterations, count=self.count,
                    state={k: v.cpu().numpy() for k, v in self.state.items()}, records=self.records[:self.count].cpu().numpy())

    def load_state_dict(self, state):
        """Restores what ``state_dict`` saved, in place (a ``struct`` made earlier stays valid).  Raises ValueError, before anything
        is written, for another env count or ``clear``, or more records than this monitor's capacity."""
        import torch

        from . import _abi

        count, records = int(state["count"]), np.asarray(state["records"])
        if int(state["num_envs"]) != self.env.num_envs or bool(state["clear"]) != self.clear:
            raise ValueError(f"DeviceMonitor.load_state_dict: the state is of {state['num_envs']} envs with clear={state['clear']}, "
                             f"this monitor of {self.env.num_envs} with clear={self.clear}")
        if not 0 <= count <= self.capacity or records.shape != (count, _abi.MONITOR_RECORD_WORDS) or records.dtype != np.int64:
            raise ValueError(f"DeviceMonitor.load_state_dict: {count} records ({records.dtype} {records.shape}) do not fit a capacity of {self.capacity}")
        arrays = _monitor_arrays({k: np.asarray(v) for k, v in dict(state["state"]).items()})
        if arrays["running_return"].shape != (self.env.num_envs,):
            raise ValueError(f"DeviceMonitor.load_state_dict: the state arrays must be [{self.env.num_envs}]")
        for k, v in arrays.items():
            self.state[k].copy_(torch.from_numpy(v))
        self.records.zero_()
        self.records[:count].copy_(torch.from_numpy(np.ascontiguousarray(records)))
        self.iterations, self.count = int(state["iterations"]), count

    def fold(self, replay, first_slot, num_steps):
        """The `num_steps` steps `replay` holds from `first_slot` on, folded into the state (``env.monitor_fold``): call it behind the
        ``collect`` that wrote them, with its arguments.  One launch; NOT synchronised."""
        self.env.monitor_fold(self.state, replay, first_slot, num_steps)

    def record(self, iteration, clear=None):
        """The episodes finished since the last clear into the next record, tagged `iteration` (``env.monitor_stats``); `clear`
        defaults to the monitor's.  One launch; NOT synchronised.  Returns the record's index."""
        if self.count >= self.capacity:
            raise ValueError(f"DeviceMonitor: all {self.capacity} records are used")
        slot = self.count
        self.env.monitor_stats(self.state, self.records[slot], iteration, self.clear if clear is None else clear)
        self.count += 1
        return slot

    def results(self):
        """Synchronises; one dict per record written, with the record's fields."""
        import ctypes as C

        import torch

        from . import _abi

        torch.cuda.synchronize(self.env.device)
        raw = self.records[:self.count].cpu().numpy().tobytes()
        recs = [_abi.MonitorRecord.from_buffer_copy(raw, i * C.sizeof(_abi.MonitorRecord)) for i in range(self.count)]
        return [{name: getattr(r, name) for name, _ in _abi.MonitorRecord._fields_} for r in recs]


# ------------------------------------------------------------------------------------------------ running normalization (VecNormalize)
def norm_sums(terms):
    """THE ORDER OF THE SUMS of include/urgym.h ("running observation and reward normalization on the device") in numpy: `terms`
    float64 [N] or [N, d], summed over the rows per column, bitwise what the two fold kernels leave.  Slabs of 128 rows, four chains
    per slab over rows q, q + 4, ..., ``(c0 + c1) + (c2 + c3)``, sixteen parts over slabs c, c + 16, ..., then ``part[c] += part[c + s]``
    for s = 8, 4, 2, 1.  An absent term is +0.0: no partial sum is ever -0.0, so that leaves the bits a skipped term would."""
    from . import _abi

    x = np.asarray(terms)
    if x.dtype != np.float64 or x.ndim not in (1, 2) or x.shape[0] < 1:
        raise ValueError(f"terms must be a float64 [N] or [N, d] array, got {x.dtype} {x.shape}")
    flat = x.ndim == 1
    x = x.reshape(x.shape[0], -1)
    n, d = x.shape
    R, Q, P = _abi.NORM_SLAB_ROWS, _abi.NORM_CHAINS, _abi.NORM_PARTS
    slabs = -(-n // R)
    padded = np.zeros((slabs * R, d), np.float64)
    padded[:n] = x
    rows = padded.reshape(slabs, R // Q, Q, d)
    with np.errstate(all="ignore"):
        chain = np.zeros((slabs, Q, d), np.float64)
        for i in range(R // Q):
            chain = chain + rows[:, i]
        slab = (chain[:, 0] + chain[:, 1]) + (chain[:, 2] + chain[:, 3])
        rounds = -(-slabs // P)
        held = np.zeros((rounds * P, d), np.float64)
        held[:slabs] = slab
        held = held.reshape(rounds, P, d)
        part = np.zeros((P, d), np.float64)
        for i in range(rounds):
            part = part + held[i]
        s = P // 2
        while s >= 1:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
    return part[0, 0] if flat else part[0].copy()


def norm_merge(mean, var, count, s1, s2, n):
    """One slot's merge into one group (SB3's ``RunningMeanStd.update_from_moments``), every line ONE float64 operation in the
    association include/urgym.h writes: `mean`, `var` float64 [d], `count` a float64, `s1` and `s2` the sums of the slot, `n` the row
    count.  Returns ``(mean', var', count')``."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    count, nn = np.float64(count), np.float64(n)
    with np.errstate(all="ignore"):
        bm = s1 / nn
        m2 = s2 / nn
        sq = bm * bm
        d = m2 - sq
        bv = np.where(d > 0.0, d, np.float64(0.0))
        delta = bm - mean
        tot = count + nn
        dn = delta * nn
        step = dn / tot
        ma = var * count
        mb = bv * nn
        mab = ma + mb
        d2 = delta * delta
        d2c = d2 * count
        d2cn = d2c * nn
        cross = d2cn / tot
        new_m2 = mab + cross
        return mean + step, new_m2 / tot, tot


NORM_ROW_GROUPS = ("observation", "achieved_goal", "desired_goal")


def norm_initial_state(num_envs, obs_dim, goal_dim):
    """SB3's ``RunningMeanStd`` at its start for the four groups, and ``running_ret`` = 0: a dict under ``_abi.NORM_STATE_FIELDS``."""
    from . import _abi

    out = {}
    for name, shape in _abi.NORM_STATE_FIELDS:
        fill = 1.0 if name.endswith("_var") else (_abi.NORM_INITIAL_COUNT if name.endswith("_count") else 0.0)
        out[name] = np.full(shape(num_envs, obs_dim, goal_dim), fill, np.float64)
    return out


def _norm_arrays(state):
    from . import _abi

    names = [name for name, _ in _abi.NORM_STATE_FIELDS]
    if not isinstance(state, dict) or sorted(state) != sorted(names):
        raise ValueError(f"state must be a dict under {names}")
    out = {}
    for name in names:
        a = np.asarray(state[name])
        if a.dtype != np.float64 or a.ndim != 1:
            raise ValueError(f"state[{name!r}] must be a float64 1-d array, got {a.dtype} {a.shape}")
        out[name] = a.copy()
    return out


def norm_fold(state, ring, first_slot, num_steps, gamma, norm_obs=True, norm_reward=True):
    """THE FOLD of include/urgym.h in numpy, bitwise what urgym_norm_fold leaves: `state` a dict under ``_abi.NORM_STATE_FIELDS``;
    `ring` a dict of the ring's arrays ``observation`` [C, N, obs_dim], ``achieved_goal``, ``desired_goal`` [C, N, goal_dim], ``reward``
    float32 [C, N], ``terminated`` and ``truncated`` uint8 or bool [C, N]; the slots (first_slot + k) % C are folded in order, one merge
    per slot and group.  Returns the new state (the argument is not written)."""
    st = _norm_arrays(state)
    reward = np.asarray(ring["reward"])
    cap, n = reward.shape
    first, K = int(first_slot), int(num_steps)
    if reward.dtype != np.float32 or not 0 <= first < cap or not 1 <= K <= cap or st["running_ret"].shape != (n,):
        raise ValueError(f"norm_fold: reward must be float32 [C, N], first_slot in [0, C), num_steps in [1, C], running_ret [N]; got {reward.dtype} {reward.shape}, {first_slot}, {num_steps}")
    flags = []
    for name in ("terminated", "truncated"):
        x = np.asarray(ring[name])
        if x.dtype not in (np.dtype(np.uint8), np.dtype(bool)) or x.shape != reward.shape:
            raise ValueError(f"norm_fold: {name} must be a uint8 or bool {reward.shape} array, got {x.dtype} {x.shape}")
        flags.append(x.view(np.uint8) if x.dtype == bool else x)
    rows = {}
    for g in NORM_ROW_GROUPS:
        x = np.asarray(ring[g])
        if x.dtype != np.float32 or x.ndim != 3 or x.shape[:2] != reward.shape or x.shape[2] != st[g + "_mean"].shape[0]:
            raise ValueError(f"norm_fold: {g} must be a float32 [C, N, {st[g + '_mean'].shape[0]}] array, got {x.dtype} {x.shape}")
        rows[g] = x
    g64 = np.float64(gamma)
    with np.errstate(all="ignore"):
        for k in range(K):
            s = (first + k) % cap
            if norm_obs:
                for g in NORM_ROW_GROUPS:
                    x = rows[g][s].astype(np.float64)
                    m, v, c = norm_merge(st[g + "_mean"], st[g + "_var"], st[g + "_count"][0], norm_sums(x), norm_sums(x * x), n)
                    st[g + "_mean"], st[g + "_var"], st[g + "_count"] = m, v, np.array([c], np.float64)
            if norm_reward:
                scaled = st["running_ret"] * g64
                running = scaled + reward[s].astype(np.float64)
                m, v, c = norm_merge(st["ret_mean"], st["ret_var"], st["ret_count"][0], norm_sums(running), norm_sums(running * running), n)
                st["ret_mean"], st["ret_var"], st["ret_count"] = np.atleast_1d(m), np.atleast_1d(v), np.array([c], np.float64)
                st["running_ret"] = np.where((flags[0][s] | flags[1][s]) != 0, np.float64(0.0), running)
    return st


def _norm_clip(v, clip):
    c = np.float64(clip)
    lo = np.where(v < -c, -c, v)
    return np.where(lo > c, c, lo)


def normalize_rows(x, mean, var, eps, clip):
    """NORMALIZE of include/urgym.h in numpy, bitwise what urgym_norm_rows / urgym_norm_batch write: `x` float32 [..., d], `mean` and
    `var` float64 [d]; ``inv = 1 / sqrt(var + eps)`` once per feature, then ``(float)min(max(((double)x - mean) * inv, -clip), clip)``."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, got {x.dtype}")
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.sqrt(np.asarray(var, np.float64) + np.float64(eps))
        centred = x.astype(np.float64) - np.asarray(mean, np.float64)
        return _norm_clip(centred * inv, clip).astype(np.float32)


def normalize_reward(r, var, eps, clip):
    """A reward as urgym_norm_batch writes it: ``(float)min(max((double)r * inv_ret, -clip), clip)``, no mean subtracted (SB3)."""
    r = np.asarray(r)
    if r.dtype != np.float32:
        raise ValueError(f"r must be float32, got {r.dtype}")
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.sqrt(np.float64(np.asarray(var).reshape(-1)[0]) + np.float64(eps))
        return _norm_clip(r.astype(np.float64) * inv, clip).astype(np.float32)


class DeviceNormalizer:
    """stable-baselines3's ``VecNormalize`` on the device: the running mean and variance of the three observation groups the collecting
    actor saw and of the discounted return, in float64 device tensors (``self.state``, under ``_abi.NORM_STATE_FIELDS``), the scratch
    rows the collecting actor reads and the fold's workspace.  `env`: a UR5ReachVectorEnv with auto_reset.  ``fold`` follows a
    ``collect`` with its arguments; ``training = False`` freezes the statistics (``fold`` then launches nothing).  `fold_steps`: the most
    steps one fold (or one iteration of ``SACLearner.train``) may hold; the workspace is sized for it."""

    def __init__(self, env, gamma=0.95, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, epsilon=1e-8, fold_steps=32):
        import ctypes as C

        import torch

        from . import _abi, _native

        if not env.cfg.auto_reset:
            raise ValueError("DeviceNormalizer: env must be made with auto_reset=True (the return of an env that is not reset does not restart)")
        self.options = self.check_options(gamma=gamma, norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=clip_obs, clip_reward=clip_reward, epsilon=epsilon)
        if isinstance(fold_steps, bool) or int(fold_steps) != fold_steps or not 1 <= int(fold_steps) < 65535:
            raise ValueError(f"DeviceNormalizer: fold_steps must be an integer in [1, 65535), got {fold_steps!r}")
        self.env, self.training, self.fold_steps = env, True, int(fold_steps)
        dev = env.device
        self.state = {name: torch.from_numpy(a).to(dev) for name, a in norm_initial_state(env.num_envs, env.obs_dim, env.goal_dim).items()}
        self.scratch = torch.zeros((env.num_envs * (env.obs_dim + 2 * env.goal_dim),), dtype=torch.float32, device=dev)
        need = C.c_uint64(0)
        _native.check(env.lib.urgym_norm_workspace(env._h, self.fold_steps, C.byref(need)), env._h)
        self.workspace = torch.zeros((need.value // 8,), dtype=torch.float64, device=dev)
        Z = _abi.Normalization()
        for name, _ in _abi.NORM_STATE_FIELDS:
            setattr(Z.state, name, C.cast(self.state[name].data_ptr(), C.POINTER(C.c_double)))
        o = self.options
        Z.gamma, Z.eps, Z.clip_obs, Z.clip_reward = o["gamma"], o["epsilon"], o["clip_obs"], o["clip_reward"]
        Z.norm_obs, Z.norm_reward, Z.reserved0 = int(o["norm_obs"]), int(o["norm_reward"]), 0
        Z.scratch = C.cast(self.scratch.data_ptr(), C.POINTER(C.c_float))
        Z.workspace, Z.workspace_bytes = self.workspace.data_ptr(), need.value
        self._struct = Z

    @staticmethod
    def check_options(*, gamma, norm_obs, norm_reward, clip_obs, clip_reward, epsilon):
        """Raises ValueError for what the entry points refuse about the options (include/urgym.h); returns them as plain values.
        Needs no GPU."""
        for name, v in (("norm_obs", norm_obs), ("norm_reward", norm_reward)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"{name} must be True or False, got {v!r}")
        for name, v in (("gamma", gamma), ("clip_obs", clip_obs), ("clip_reward", clip_reward), ("epsilon", epsilon)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"{name} must be a number, got {v!r}")
        if not 0.0 <= float(gamma) <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
        if not (float(epsilon) >= 0.0 and np.isfinite(float(epsilon))):
            raise ValueError(f"epsilon must be finite and at least 0, got {epsilon!r}")
        for name, v in (("clip_obs", clip_obs), ("clip_reward", clip_reward)):
            if not float(v) > 0.0:
                raise ValueError(f"{name} must be positive (+inf is allowed), got {v!r}")
        return dict(gamma=float(gamma), norm_obs=bool(norm_obs), norm_reward=bool(norm_reward), clip_obs=float(clip_obs), clip_reward=float(clip_reward),
                    epsilon=float(epsilon))

    def struct(self):
        """The ``urgym_normalization`` as it stands: ``training`` is read now."""
        self._struct.training = int(bool(self.training))
        return self._struct

    def fold(self, replay, first_slot, num_steps):
        """The `num_steps` steps `replay` holds from `first_slot` on, folded into the statistics (``env.norm_fold``): call it behind the
        ``collect`` that wrote them, with its arguments.  Two launches, none with ``training`` False; NOT synchronised."""
        self.env.norm_fold(self, replay, first_slot, num_steps)

    def normalize(self, rows, out=None):
        """``env.norm_rows`` with these statistics: one launch, NOT synchronised."""
        return self.env.norm_rows(self, rows, out)

    def normalize_batch(self, batch):
        """``env.norm_batch`` with these statistics, in place: one launch, NOT synchronised."""
        return self.env.norm_batch(self, batch)

    def state_dict(self):
        """The statistics for a checkpoint: the thirteen arrays, the options, ``training``, and the env shape a load checks.
        Synchronises."""
        env = self.env
        return dict(num_envs=env.num_envs, obs_dim=env.obs_dim, goal_dim=env.goal_dim, options=dict(self.options), training=bool(self.training),
                    state={k: v.cpu().numpy() for k, v in self.state.items()})

    def check_state_dict(self, state):
        """Raises ValueError unless `state` is a ``state_dict`` of a normalizer of this env shape and these options.  Writes nothing."""
        from . import _abi

        env = self.env
        for k, v in dict(num_envs=env.num_envs, obs_dim=env.obs_dim, goal_dim=env.goal_dim).items():
            if int(state[k]) != v:
                raise ValueError(f"DeviceNormalizer.load_state_dict: {k} is {state[k]} in the state, {v} here")
        if dict(state["options"]) != self.options:
            raise ValueError(f"DeviceNormalizer.load_state_dict: the options are {dict(state['options'])} in the state, {self.options} here")
        arrays = _norm_arrays({k: np.asarray(v) for k, v in dict(state["state"]).items()})
        for name, shape in _abi.NORM_STATE_FIELDS:
            if arrays[name].shape != tuple(shape(env.num_envs, env.obs_dim, env.goal_dim)):
                raise ValueError(f"DeviceNormalizer.load_state_dict: state[{name!r}] must be {tuple(shape(env.num_envs, env.obs_dim, env.goal_dim))}, got {arrays[name].shape}")
        return arrays

    def load_state_dict(self, state):
        """Restores what ``state_dict`` saved, in place (the struct stays valid).  Everything is checked before anything is written."""
        import torch

        arrays = self.check_state_dict(state)
        for k, v in arrays.items():
            self.state[k].copy_(torch.from_numpy(v))
        self.training = bool(state["training"])


# ------------------------------------------------------------------------------------------------ sampling-based MPC on the device (MPPI)
def mppi_noise(seed, draw, iteration, parents, samples, steps, dtype=np.float32):
    """The noise of the device's MPPI planner, restated from include/urgym.h ("sampling-based MPC on the device"): a pure function of
    (seed, draw, iteration, parent p, sample j, horizon step h, component).  `parents`, `samples`, `steps` are integers or integer
    arrays that broadcast together; returns their shape + (6,): zeros where j == 0 (the nominal sequence), else Box-Muller as
    ``policy_noise`` states it on the words of the counter (p, (i << 24) | (h << 16) | j, draw, MPPI_TAG | block).  `dtype` is the
    precision of ln / sqrt / cos / sin."""
    from . import _abi

    draw, i = int(draw), int(iteration)
    if not 0 <= draw < 1 << 32 or not 0 <= i < _abi.MPPI_ITERATIONS_MAX:
        raise ValueError(f"draw must be in [0, 2^32) and iteration in [0, {_abi.MPPI_ITERATIONS_MAX}), got {draw}, {i}")
    p, j, h = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (parents, samples, steps)))
    if j.size and (int(j.max()) >= _abi.MPPI_SAMPLES_MAX or int(h.max()) >= _abi.MPPI_HORIZON_MAX):
        raise ValueError("samples must be below 1024 and steps below 64")
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    mid = np.uint64(i << 24) | (h << np.uint64(16)) | j
    a = philox4x32_10(key, (p, mid, np.uint64(draw), np.uint64(_abi.MPPI_TAG | 0)))
    b = philox4x32_10(key, (p, mid, np.uint64(draw), np.uint64(_abi.MPPI_TAG | 1)))
    eps = _box_muller(_noise_integers(a, b, dtype), dtype)
    eps[j == 0] = 0
    return eps


def mppi_colored_noise(xi, beta):
    """THE COLOURED SAMPLE's recurrence in numpy, bitwise (include/urgym.h, "temporally correlated sampling noise"): `xi` float32
    [H, ...], THE SAMPLE's eps (``mppi_noise``), `beta` in [0, 1].  scale = float32(sqrt(1 - beta * beta)) with beta taken as float32
    and everything up to the square root in float64; eps[0] = xi[0]; for h >= 1: a = beta * eps[h - 1]; b = scale * xi[h];
    eps[h] = a + b, each one float32 operation.  Every step has unit variance and lag-1 correlation beta; the nominal sample's zeros
    stay +0.0."""
    xi = np.asarray(xi)
    if xi.dtype != np.float32 or xi.ndim < 1:
        raise ValueError(f"xi must be float32 [H, ...], got {xi.dtype} {xi.shape}")
    with np.errstate(over="ignore"):
        beta = np.float32(beta)
    if not (np.isfinite(beta) and 0.0 <= beta <= 1.0):
        raise ValueError(f"beta must be finite and in [0, 1], got {beta!r}")
    b = np.float64(beta)
    bb = b * b
    d = np.float64(1.0) - bb
    scale = np.float32(np.sqrt(d))
    eps = np.empty_like(xi)
    if xi.shape[0]:
        eps[0] = xi[0]
    for h in range(1, xi.shape[0]):
        a = beta * eps[h - 1]
        b = scale * xi[h]
        eps[h] = a + b
    return eps


def mppi_actions(mean, eps, sigma):
    """THE SAMPLE's action line in numpy, bitwise: `mean` float32 [H, E, 6], `eps` float32 [H, E * K, 6]; planner env n = p * K + j reads
    parent p's mean.  s = sigma * eps; a = mean + s; action = fmin(fmax(a, -1), 1), each one float32 operation.  `sigma` is a number, or
    -- THE ADAPTIVE SAMPLE -- a float32 [H, E, 6] array of one width per element, read as the mean is."""
    mean, eps = np.asarray(mean), np.asarray(eps)
    if mean.dtype != np.float32 or eps.dtype != np.float32 or mean.ndim != 3 or eps.ndim != 3 or eps.shape[1] % mean.shape[1]:
        raise ValueError(f"mean must be float32 [H, E, 6] and eps float32 [H, E * K, 6], got {mean.dtype} {mean.shape}, {eps.dtype} {eps.shape}")
    K = eps.shape[1] // mean.shape[1]
    if np.ndim(sigma) == 0:
        width = np.float32(sigma)
    else:
        width = np.asarray(sigma)
        if width.dtype != np.float32 or width.shape != mean.shape:
            raise ValueError(f"an array sigma must be float32 {mean.shape} like mean, got {width.dtype} {width.shape}")
        width = np.repeat(width, K, axis=1)
    s = width * eps
    a = np.repeat(mean, K, axis=1) + s
    return np.fmin(np.fmax(a, np.float32(-1)), np.float32(1))


def mppi_score(reward, terminated, truncated, is_success, collision, gamma):
    """THE SCORE in numpy, bitwise what H urgym_mppi_score launches leave: the five arrays are [H, N], what planner step h returned.
    Returns a dict of ret, g (float64), alive, success, collided (uint8) and end_step (int32), each [N]."""
    reward = np.asarray(reward)
    if reward.dtype != np.float32 or reward.ndim != 2:
        raise ValueError(f"reward must be a float32 [H, N] array, got {reward.dtype} {reward.shape}")
    H, n = reward.shape
    done = (np.asarray(terminated).astype(np.uint8) | np.asarray(truncated).astype(np.uint8)) != 0
    ret, g, alive = np.zeros(n, np.float64), np.ones(n, np.float64), np.ones(n, bool)
    end_step, success, collided = np.full(n, H - 1, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for h in range(H):
            t = g * reward[h].astype(np.float64)
            ret = np.where(alive, ret + t, ret)
            g = np.where(alive, g * np.float64(gamma), g)
            ends = alive & done[h]
            end_step[ends] = h
            success[ends] = np.asarray(is_success[h]).astype(np.uint8)[ends]
            collided[ends] = np.asarray(collision[h]).astype(np.uint8)[ends]
            alive = alive & ~ends
    return dict(ret=ret, g=g, alive=alive.astype(np.uint8), end_step=end_step, success=success, collided=collided)


def mppi_weights(ret, lam, samples):
    """THE UPDATE's weights with numpy's float64 exp in place of the device's: `ret` float64 [E * K].  Returns (w [E, K], rmax [E]).
    A return that is not finite weighs nothing; a parent without a finite return puts everything on its sample 0."""
    r = np.asarray(ret, dtype=np.float64).reshape(-1, int(samples))
    finite = np.isfinite(r)
    rmax = np.where(finite, r, -np.inf).max(axis=1)
    with np.errstate(all="ignore"):
        w = np.where(finite, np.exp((r - rmax[:, None]) / np.float64(lam)), 0.0)
    none = ~finite.any(axis=1)
    w[none] = 0.0
    w[none, 0] = 1.0
    return w, rmax


def mppi_update(ret, w, actions, shift):
    """THE UPDATE in numpy given the weights, bitwise: `ret` float64 [E * K], `w` float64 [E, K] (the device's own, or ``mppi_weights``),
    `actions` float32 [H, E * K, 6].  Every sum is THE ORDERED SUM over the K float64 terms of a parent.  Returns a dict of new_mean and
    mean ([H, E, 6] float32; mean is new_mean advanced by one step where `shift`), action_out [E, 6], best_return, nominal_return, ess [E]."""
    w, actions = np.asarray(w), np.asarray(actions)
    if w.dtype != np.float64 or w.ndim != 2 or actions.dtype != np.float32 or actions.ndim != 3 or actions.shape[1:] != (w.size, 6):
        raise ValueError(f"w must be float64 [E, K] and actions float32 [H, E * K, 6], got {w.dtype} {w.shape}, {actions.dtype} {actions.shape}")
    E, K = w.shape
    H = actions.shape[0]
    r = np.asarray(ret, dtype=np.float64).reshape(E, K)
    new_mean, ess = np.zeros((H, E, 6), np.float32), np.zeros(E, np.float64)
    with np.errstate(all="ignore"):
        for p in range(E):
            Z = ordered_sum(w[p], np.float64)
            Q = ordered_sum(w[p] * w[p], np.float64)
            ess[p] = (Z * Z) / Q
            a = actions[:, p * K:(p + 1) * K].astype(np.float64)
            for h in range(H):
                for c in range(6):
                    new_mean[h, p, c] = np.float32(ordered_sum(w[p] * a[h, :, c], np.float64) / Z)
    mean = new_mean.copy()
    if shift:
        mean[:-1] = new_mean[1:]
    rmax = np.where(np.isfinite(r), r, -np.inf).max(axis=1)
    return dict(new_mean=new_mean, mean=mean, action_out=new_mean[0].copy(), best_return=rmax, nominal_return=r[:, 0].copy(), ess=ess)


def mppi_elite_rank(ret, samples, elites):
    """THE RANK in numpy (include/urgym.h, "elite samples and an adaptive std"): `ret` float64 [E * K].  key = the return, or -inf where it
    is not finite; rank_j counts the samples of the same parent with a larger key, or an equal key (-0.0 == 0.0) and a lower index.
    Returns a dict of rank (int32 [E, K], a permutation per parent), elite (uint8 [E, K]: rank < `elites` and finite), elite_count (int32
    [E]) and threshold (float64 [E]: the smallest elite return, its bits kept; -inf with no elite)."""
    K, M = int(samples), int(elites)
    if not 1 <= M <= K:
        raise ValueError(f"elites must be in [1, samples], got {M}, {K}")
    r = np.asarray(ret, dtype=np.float64).reshape(-1, K)
    finite = np.isfinite(r)
    key = np.where(finite, r, -np.inf)
    index = np.arange(K)
    before = (key[:, :, None] > key[:, None, :]) | ((key[:, :, None] == key[:, None, :]) & (index[:, None] < index[None, :]))  # [p, i, j]
    rank = before.sum(axis=1).astype(np.int32)
    elite = (rank < M) & finite
    count = elite.sum(axis=1).astype(np.int32)
    threshold = np.full(r.shape[0], -np.inf, np.float64)
    for p in np.nonzero(count)[0]:
        threshold[p] = r[p, rank[p] == count[p] - 1][0]
    return dict(rank=rank, elite=elite.astype(np.uint8), elite_count=count, threshold=threshold)


def mppi_elite_weights(ret, lam, samples, elites):
    """THE ELITE WEIGHT with numpy's float64 exp in place of the device's: ``mppi_weights`` with every sample that is no elite weighing
    nothing.  Returns (w [E, K], rmax [E]); with ``elites == samples`` they are ``mppi_weights``'."""
    w, rmax = mppi_weights(ret, lam, samples)
    elite = mppi_elite_rank(ret, samples, elites)["elite"] != 0
    none = ~np.isfinite(np.asarray(ret, dtype=np.float64).reshape(-1, int(samples))).any(axis=1)
    w = np.where(elite | none[:, None], w, 0.0)
    return w, rmax


def mppi_elite_update(ret, w, actions, shift, std_min, std_max):
    """THE ELITE UPDATE in numpy given the weights, bitwise: ``mppi_update``'s dict (the same lines on the same `w`, zero for a sample that
    is no elite) and new_std, float32 [H, E, 6] -- THE STD: m = S / Z unrounded; per sample d = a - m, dd = d * d, t = w * dd; V their
    ordered sum; v = V / Z; sd = sqrt(v); fmin(fmax(sd, std_min), std_max), rounded to float32 once.  A NaN v ends at std_min."""
    out = mppi_update(ret, w, actions, shift)
    w, actions = np.asarray(w), np.asarray(actions)
    E, K = w.shape
    H = actions.shape[0]
    lo, hi = np.float64(np.float32(std_min)), np.float64(np.float32(std_max))
    new_std = np.zeros((H, E, 6), np.float32)
    with np.errstate(all="ignore"):
        for p in range(E):
            Z = ordered_sum(w[p], np.float64)
            a = actions[:, p * K:(p + 1) * K].astype(np.float64)
            for h in range(H):
                for c in range(6):
                    m = ordered_sum(w[p] * a[h, :, c], np.float64) / Z
                    d = a[h, :, c] - m
                    dd = d * d
                    v = ordered_sum(w[p] * dd, np.float64) / Z
                    new_std[h, p, c] = np.float32(np.fmin(np.fmax(np.sqrt(v), lo), hi))
    out["new_std"] = new_std
    return out


_TEMPER_LOG2E, _TEMPER_LN2_HI, _TEMPER_LN2_LO = np.float64(1.4426950408889634), np.float64(6.93147180369123816490e-01), np.float64(1.90821492927058770002e-10)
# 1 / n! for n = 0 .. 13, each the correctly rounded float64 (urgym_mppi_temper.h writes the same literals)
_TEMPER_COEF = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984,
                2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10)


def mppi_temper_exp(x):
    """THE EXPONENTIAL of include/urgym.h ("the temperature from a target effective sample size") in numpy, bitwise, elementwise: `x`
    float64, not positive and no NaN.  x < -708 gives +0.0; otherwise y = x * LOG2E; kf = rint(y); hi = kf * LN2_HI; r1 = x - hi;
    lo = kf * LN2_LO; r = r1 - lo; Horner over 1 / n!, n = 13 .. 0, as t = p * r; p = t + c; the result is p times the power of two whose
    exponent field is 1023 + kf.  Every operation is one float64 rounding.  Within 2 ulp of exp; exactly 1 at 0 and -0.0."""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any() or (x > 0).any():
        raise ValueError("mppi_temper_exp takes arguments that are not positive and no NaN")
    below = x < -708.0
    xs = np.where(below, 0.0, x)  # the lanes that return early take no part in what follows
    kf = np.rint(xs * _TEMPER_LOG2E)
    r = xs - kf * _TEMPER_LN2_HI
    r = r - kf * _TEMPER_LN2_LO
    p = np.full_like(r, _TEMPER_COEF[13])
    for c in _TEMPER_COEF[12::-1]:
        t = p * r
        p = t + np.float64(c)
    scale = ((np.int64(1023) + kf.astype(np.int64)) << np.int64(52)).view(np.float64)
    return np.where(below, 0.0, p * scale)


def mppi_temper_solve(ret, samples, ess_target, lam_min, lam_max, steps, lam=5.0, elites=None):
    """THE SEARCH of include/urgym.h ("the temperature from a target effective sample size") and the weights it ends with, in numpy,
    bitwise: `ret` float64 [E * K].  A sample is counted where its return is finite and, with `elites`, where it is an elite of
    ``mppi_elite_rank``.  ess(lam) = (Z * Z) / Q with Z and Q THE ORDERED SUMs of w_j = ``mppi_temper_exp((r_j - rmax) / lam)`` (0 where
    j is not counted) and of w_j * w_j.  Per parent: no finite return keeps `lam` (urgym_mppi.lam) and puts everything on sample 0
    (saturated 3); ess(lam_max) < T ends at lam_max (1); ess(lam_min) >= T at lam_min (2); otherwise `steps` bisections of
    mid = sqrt(lo * hi) -- ess(mid) >= T moves hi, else lo -- end at hi (0).  Returns a dict of lam [E], saturated (uint8 [E]), w
    ([E, K], what ``mppi_update`` / ``mppi_elite_update`` take), ess [E] (the value the search last accepted: that of w), rmax [E], and
    lam_below [E]: the lo the bisection ended with (ess there is below T; lam itself where there was no bisection)."""
    from . import _abi

    K, S, T = int(samples), int(steps), np.float64(ess_target)
    r = np.asarray(ret, dtype=np.float64).reshape(-1, K)
    E = r.shape[0]
    finite = np.isfinite(r)
    counted = finite if elites is None else mppi_elite_rank(ret, K, elites)["elite"] != 0
    rmax = np.where(finite, r, -np.inf).max(axis=1)
    out = dict(lam=np.zeros(E, np.float64), saturated=np.zeros(E, np.uint8), w=np.zeros((E, K), np.float64), ess=np.zeros(E, np.float64), rmax=rmax,
               lam_below=np.zeros(E, np.float64))

    def weights(p, at):
        with np.errstate(all="ignore"):
            d = np.where(counted[p], r[p] - rmax[p], 0.0)
            return np.where(counted[p], mppi_temper_exp(d / np.float64(at)), 0.0)

    def ess(p, at):
        w = weights(p, at)
        Z, Q = ordered_sum(w, np.float64), ordered_sum(w * w, np.float64)
        return (Z * Z) / Q

    for p in range(E):
        if not finite[p].any():
            at, below, how = np.float64(lam), np.float64(lam), _abi.MPPI_TEMPER_NO_RETURN
            w = np.zeros(K, np.float64)
            w[0] = 1.0
        else:
            lo, hi = np.float64(lam_min), np.float64(lam_max)
            if ess(p, hi) < T:
                at, below, how = hi, hi, _abi.MPPI_TEMPER_AT_MAX
            elif ess(p, lo) >= T:
                at, below, how = lo, lo, _abi.MPPI_TEMPER_AT_MIN
            else:
                for _ in range(S):
                    q = lo * hi
                    mid = np.sqrt(q)
                    if ess(p, mid) >= T:
                        hi = mid
                    else:
                        lo = mid
                at, below, how = hi, lo, _abi.MPPI_TEMPER_SOLVED
            w = weights(p, at)
        Z, Q = ordered_sum(w, np.float64), ordered_sum(w * w, np.float64)
        out["lam"][p], out["lam_below"][p], out["saturated"][p], out["w"][p], out["ess"][p] = at, below, how, w, (Z * Z) / Q
    return out


def mppi_guided_actions(actions, policy_action, eps, policy_sigma, samples, policy_samples):
    """THE GUIDE in numpy, bitwise (include/urgym.h, "MPPI with the learner in the loop"): `actions` and `eps` float32 [H, E * K, 6] as the
    sample launch left them, `policy_action` float32 [H, E * K, 6] -- row h what the actor gave before planner step h -- or [E * K, 6] for
    every step alike.  Returns a copy of `actions` in which the rows of samples 1 .. `policy_samples` of every parent are
    s = policy_sigma * eps; a = policy_action + s; fmin(fmax(a, -1), 1), each one float32 operation; every other row is `actions`'."""
    actions, eps, pa = np.asarray(actions), np.asarray(eps), np.asarray(policy_action)
    K, P = int(samples), int(policy_samples)
    if actions.dtype != np.float32 or eps.dtype != np.float32 or pa.dtype != np.float32 or actions.ndim != 3 or actions.shape != eps.shape:
        raise ValueError(f"actions and eps must be float32 [H, E * K, 6] and policy_action float32, got {actions.dtype} {actions.shape}, {eps.dtype} {eps.shape}, {pa.dtype}")
    if pa.shape not in (actions.shape, actions.shape[1:]) or actions.shape[1] % K or not 0 <= P <= K - 1:
        raise ValueError(f"policy_action must be [H, E * K, 6] or [E * K, 6] and policy_samples in [0, samples - 1], got {pa.shape}, {P}, {K}")
    j = np.arange(actions.shape[1]) % K
    guided = (j >= 1) & (j <= P)
    with np.errstate(all="ignore"):
        s = np.float32(policy_sigma) * eps
        a = np.broadcast_to(pa, actions.shape) + s
        line = np.fmin(np.fmax(a, np.float32(-1)), np.float32(1))
    out = actions.copy()
    out[:, guided] = line[:, guided]
    return out


def mppi_terminal(score, value, terminal_value, fail_cost):
    """THE TERMINAL STEP in numpy, bitwise: `score` is ``mppi_score``'s dict (ret, g, alive, success are read), `value` float32 [N] or None
    where `terminal_value` is off.  v = value for a live future (0 with `terminal_value` off), 0 for one that ended in success, -fail_cost
    for one that ended otherwise -- a selection, so a NaN value of an ended future reaches nothing; where v != 0, t = g * v and
    ret = ret + t in float64.  Returns dict(terminal [N], ret [N])."""
    ret, g = np.asarray(score["ret"], dtype=np.float64), np.asarray(score["g"], dtype=np.float64)
    alive, success = np.asarray(score["alive"]) != 0, np.asarray(score["success"]) != 0
    live = np.asarray(value, dtype=np.float32).astype(np.float64) if terminal_value else np.zeros(ret.shape, np.float64)
    if live.shape != ret.shape:
        raise ValueError(f"value must be [N] like ret, got {live.shape}, {ret.shape}")
    v = np.where(alive, live, np.where(success, np.float64(0.0), -np.float64(fail_cost)))
    with np.errstate(all="ignore"):
        t = g * v
        new = np.where(v != 0, ret + t, ret)
    return dict(terminal=v, ret=new)


def mppi_explore_counters(draw, parents):
    """The two Philox counters of the exploration noise of (parent p, draw) (include/urgym.h, "planner-collected experience"): a pair of
    4-tuples (p, 0, draw, MPPI_TAG | block) for block 2 and block 3, `parents` an integer or an integer array."""
    from . import _abi

    draw = int(draw)
    if not 0 <= draw < 1 << 32:
        raise ValueError(f"draw must be in [0, 2^32), got {draw}")
    p = np.asarray(parents, dtype=np.uint64)
    if p.size and int(p.max()) >= 1 << 31:
        raise ValueError("parents must be env indices")
    return tuple((p, np.uint64(0), np.uint64(draw), np.uint64(_abi.MPPI_TAG | (_abi.MPPI_EXPLORE_BLOCK + b))) for b in (0, 1))


def mppi_explore_noise(seed, draw, parents, dtype=np.float32):
    """The exploration noise of a planner-driven collection, restated from include/urgym.h: a pure function of (seed, draw, parent p,
    component) -- six normals per parent, Box-Muller as ``mppi_noise`` forms the planner's on the words of the counters
    ``mppi_explore_counters`` states (blocks 2 and 3 under the planner's tag; the planner's own noise draws blocks 0 and 1), with the
    planner's key.  `parents` is an integer or an integer array; returns its shape + (6,).  `dtype` is the precision of ln / sqrt / cos /
    sin."""
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    c2, c3 = mppi_explore_counters(draw, parents)
    return _box_muller(_noise_integers(philox4x32_10(key, c2), philox4x32_10(key, c3), dtype), dtype)


def mppi_execute(action_out, eps, explore_sigma):
    """THE EXECUTE LINE in numpy, bitwise given `eps`: `action_out` and `eps` float32 [E, 6].  s = explore_sigma * eps; a = action_out + s;
    executed = fmin(fmax(a, -1), 1), each one float32 operation.  With ``explore_sigma == 0`` the result is a copy of `action_out`'s
    bytes (no clamp, a -0.0 stays -0.0) and `eps` is not read (it may be None)."""
    action_out = np.asarray(action_out)
    if action_out.dtype != np.float32 or action_out.ndim != 2 or action_out.shape[1] != 6:
        raise ValueError(f"action_out must be float32 [E, 6], got {action_out.dtype} {action_out.shape}")
    sigma = np.float32(explore_sigma)
    if not (np.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"explore_sigma must be finite and >= 0, got {explore_sigma}")
    if sigma == 0:
        return action_out.copy()
    eps = np.asarray(eps)
    if eps.dtype != np.float32 or eps.shape != action_out.shape:
        raise ValueError(f"eps must be float32 {action_out.shape}, got {eps.dtype} {eps.shape}")
    with np.errstate(all="ignore"):
        s = sigma * eps
        a = action_out + s
        return np.fmin(np.fmax(a, np.float32(-1)), np.float32(1))


def _stats_fmin(a, b):
    """urgym_mppi_stats.h's mppi_stats_fmin, elementwise: a NaN operand gives the other one, equal operands give `a`."""
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b < a, b, a)))


def mppi_plan_stats(best_return, nominal_return, ess, elite_count=None, threshold=None, iteration=0):
    """THE PLAN STATISTICS of include/urgym.h ("the planner inside the training call") in numpy, bitwise what urgym_mppi_stats writes:
    `best_return`, `nominal_return`, `ess` float64 [E] as a plan leaves them; `elite_count` (int32 [E]) and `threshold` (float64 [E]) both
    given (a planner with elites or the adaptive std) or neither.  Every sum is ``ordered_sum(..., np.float64)`` over all E parents with
    +0.0 for a parent that does not count; every mean is one float64 division, +0.0 where nothing counted; the minimum runs the ordered
    sum's lanes and levels with ``mppi_stats_fmin``.  Returns a dict with the fields of ``urgym_mppi_stats_record``."""
    from ._abi import MPPI_STATS_MAX_PARENTS
    from ._abi import SAC_TERMS_LANES as L

    best, nominal, ess = (np.asarray(x) for x in (best_return, nominal_return, ess))
    for name, x in (("best_return", best), ("nominal_return", nominal), ("ess", ess)):
        if x.dtype != np.float64 or x.ndim != 1 or x.shape != best.shape:
            raise ValueError(f"{name} must be a float64 [E] array, got {x.dtype} {x.shape}")
    E = best.shape[0]
    if not 1 <= E <= MPPI_STATS_MAX_PARENTS:
        raise ValueError(f"E must be in [1, {MPPI_STATS_MAX_PARENTS}], got {E}")
    if (elite_count is None) != (threshold is None):
        raise ValueError("elite_count and threshold go together")
    adaptive = elite_count is not None
    if adaptive:
        elite_count, threshold = np.asarray(elite_count), np.asarray(threshold)
        if elite_count.dtype != np.int32 or elite_count.shape != (E,) or threshold.dtype != np.float64 or threshold.shape != (E,):
            raise ValueError(f"elite_count must be int32 [{E}] and threshold float64 [{E}]")
    zero = np.float64(0.0)

    def mean(total, count):
        return total / np.float64(count) if count else zero

    def counted(mask, x):
        return ordered_sum(np.where(mask, x, zero), np.float64), int(mask.sum())

    with np.errstate(all="ignore"):
        fin_b, fin_n = (best - best) == 0.0, (nominal - nominal) == 0.0  # false for a NaN and for either infinity
        both = fin_b & fin_n
        sum_b, planned = counted(fin_b, best)
        sum_n, nominal_finite = counted(fin_n, nominal)
        sum_g, gain_count = counted(both, best - nominal)
        sum_e = ordered_sum(ess, np.float64)
        low = np.full(L, np.nan)
        for first in range(0, E, L):  # every lane's next parent, ascending
            row = ess[first:first + L]
            low[:row.size] = _stats_fmin(low[:row.size], row)
        s = L // 2
        while s >= 1:
            low[:s] = _stats_fmin(low[:s], low[s:2 * s])
            s //= 2
        rec = dict(mean_best_return=mean(sum_b, planned), mean_nominal_return=mean(sum_n, nominal_finite), mean_gain=mean(sum_g, gain_count),
                   mean_ess=mean(sum_e, E), min_ess=np.float64(low[0]), mean_elite_count=zero, mean_threshold=zero, iteration=int(iteration), num_parents=E,
                   planned=planned, nominal_finite=nominal_finite, gain_count=gain_count, threshold_count=0, reserved0=0)
        if adaptive:
            fin_t = (threshold - threshold) == 0.0
            sum_t, threshold_count = counted(fin_t, threshold)
            rec.update(mean_elite_count=mean(ordered_sum(elite_count.astype(np.float64), np.float64), E), mean_threshold=mean(sum_t, threshold_count),
                       threshold_count=threshold_count)
    return rec


def mppi_stats_record_bytes(rec):
    """A dict of ``mppi_plan_stats`` as the 88 bytes of ``urgym_mppi_stats_record``."""
    from . import _abi

    return bytes(_abi.MppiStatsRecord(*[rec[name] for name, _ in _abi.MppiStatsRecord._fields_]))


class DeviceMPPI:
    """An MPPI planner (Williams et al., 2017) for `env`, a UR5ReachVectorEnv of E envs, that plans with the step kernel itself: it owns a
    planner environment of E * `samples` envs (same env id, configuration and device, ``auto_reset=False``) and every buffer of
    ``urgym_mppi``.  A plan clones each env into `samples` futures, rolls them `horizon` steps under perturbed action sequences, weighs
    the sequences by exp((return - best) / `lam`) and keeps the weighted mean as the next nominal sequence; `iterations` repeats that
    from the refined mean.  `sigma` is the standard deviation of the perturbation in action units ([-1, 1] per joint), `gamma` the
    discount inside the horizon.  With `shift` the nominal sequence advances by one step after each plan (receding horizon).  The
    defaults of `horizon`, `sigma` and `lam` are a row of the grid tools/bench_mppi.py ran on UR5DynReach-v1 and UR5OriReach-v1 (DESIGN.md
    section 26); a horizon whose summed step rewards outweigh the collision penalty makes ending the episode the best-scoring future.

    The learner in the loop, all opt-in.  `actor` and `critic` are what ``DeviceActor`` and ``DeviceCritic`` take
    (the weights, or a path / a pair of paths to load them from); they are created on the planner environment and closed with it, and
    see its raw rows.  `policy_samples` = P in [0, samples - 1]: samples 1 .. P of every parent execute actor(state) + `policy_sigma` *
    noise at every horizon step.  `terminal_value`: a future still alive after the horizon is credited gamma^H min Q(s_H, actor(s_H));
    the shipped critics were trained with gamma = 0.95, so use ``gamma=0.95`` with them.  `fail_cost`: a future that ends without success
    is charged that much, discounted.  With all four at their defaults the plain entry points are called as before.

    Elite samples and the adaptive std, opt-in.  `elites` = M in [1, samples]: only the M best-scoring samples of
    a parent weigh in (``None``: every finite one, as before).  `adapt_std`: the update also forms a standard deviation per (horizon step,
    joint) from the elites, clamped to [`std_min`, `std_max`] (`std_max` defaults to `sigma`), and iterations >= 1 of the same plan sample
    with it; every plan starts at `sigma` again.  With either given the ``urgym_mppi_*_adaptive`` entry points are called, ``adapt()`` is
    the struct, and ``DIAGNOSTICS`` gains ``elite_count`` and ``threshold``; with ``elites=None`` and ``adapt_std=False`` the planner
    makes exactly the calls it made before.

    The temperature from a target effective sample size, opt-in.  `ess_target` = T in [1, M] (M = `elites`, or
    `samples` without them): every update solves its own temperature per env, within [`lam_min`, `lam_max`] by `temper_steps` bisections,
    so that the weights have an effective sample size of T (``mppi_temper_solve`` restates it); `lam` is then used only for an env
    without a finite return.  The ``urgym_mppi_*_tempered`` entry points are called, ``temper()`` is the struct, and ``DIAGNOSTICS``
    gains ``lam`` (the temperature of the last update) and ``saturated`` (``_abi.MPPI_TEMPER_*``: 0 solved, 1 at `lam_max`, the target
    cannot be met, 2 at `lam_min`, 3 no finite return) [E]; with ``ess_target=None`` the planner makes exactly the calls it made before.

    Temporally correlated sampling noise, opt-in.  `noise_beta` = beta in [0, 1]: the noise of every sample is a
    first-order autoregressive sequence along the horizon on top of the same draws -- unit variance at every step, lag-1 correlation
    beta (``mppi_colored_noise`` restates it) -- with whichever of the options above is set; ``eps`` holds the coloured values, so the
    policy samples of a guide are correlated too.  The ``urgym_mppi_*_colored`` entry points are called and ``noise()`` is the struct;
    ``noise_beta=0.0`` is a set option and goes through them; with ``noise_beta=None`` the planner makes exactly the calls it made before.

    Plan statistics.  ``stats()`` reduces the diagnostics of the last plan to one ``urgym_mppi_stats_record`` on
    the device; ``records`` is this planner's array of them (int64 [capacity, 11], grown by ``reserve_records``), which
    ``SACLearner.train(planner=, plan_stats=True)`` fills beside the monitor's records; ``planning()`` is the ``urgym_sac_planning`` of such
    a call."""

    DIAGNOSTICS = ("best_return", "nominal_return", "ess")

    def __init__(self, env, samples=256, horizon=6, sigma=0.6, lam=5.0, gamma=1.0, iterations=1, shift=True, seed=0, keep_weights=False,
                 actor=None, critic=None, policy_samples=0, policy_sigma=0.0, terminal_value=False, fail_cost=0.0, elites=None, adapt_std=False,
                 std_min=0.05, std_max=None, ess_target=None, lam_min=1e-3, lam_max=1e6, temper_steps=32, noise_beta=None):
        import ctypes as C

        import torch

        from . import _abi
        from .vector_env import _TORCH_DTYPE, UR5ReachVectorEnv

        E, K, H = env.num_envs, int(samples), int(horizon)
        if not 2 <= K <= _abi.MPPI_SAMPLES_MAX or not 1 <= H <= _abi.MPPI_HORIZON_MAX or not 1 <= int(iterations) <= _abi.MPPI_ITERATIONS_MAX:
            raise ValueError(f"DeviceMPPI: samples must be in [2, 1024], horizon in [1, 64], iterations in [1, 8]; got {samples}, {horizon}, {iterations}")
        if not (np.isfinite(sigma) and sigma >= 0 and np.isfinite(lam) and lam > 0 and np.isfinite(gamma)):
            raise ValueError(f"DeviceMPPI: sigma must be finite and >= 0, lam finite and > 0, gamma finite; got {sigma}, {lam}, {gamma}")
        adapt = self.check_adapt(K, sigma, elites, adapt_std, std_min, std_max)
        temper = self.check_temper(K if adapt is None else adapt[0], ess_target, lam_min, lam_max, temper_steps)
        beta = self.check_noise(noise_beta)
        same = {name: getattr(env.cfg, name) for name, _ in _abi.Config._fields_ if name not in ("env_kind", "num_envs", "auto_reset", "check_collision")}
        self.env = env
        self.planner = UR5ReachVectorEnv(env.env_id, num_envs=E * K, device=env.device, auto_reset=False, check_collision=bool(env.cfg.check_collision), **same)
        self.planner._needs_reset = False  # its state is the fan-out's
        self.samples, self.horizon = K, H
        self.buf = {}
        self.explore = {}  # executed and explore_eps of ``execute``, allocated at its first call
        M = _abi.Mppi()
        M.num_parents, M.samples, M.horizon, M.iterations, M.shift = E, K, H, int(iterations), int(bool(shift))
        M.sigma, M.lam, M.gamma, M.seed = float(sigma), float(lam), float(gamma), int(seed)
        for name, ct, shape in _abi.MPPI_FIELDS:
            if name == "w" and not keep_weights:
                continue
            self.buf[name] = torch.zeros(shape(E, K, H), dtype=_TORCH_DTYPE[ct], device=env.device)
            setattr(M, name, C.cast(self.buf[name].data_ptr(), C.POINTER(ct)))
        self._struct = M
        self._adapt = None
        if adapt is not None:
            A = _abi.MppiAdapt()
            A.elites, A.adapt_std, A.std_min, A.std_max = adapt
            for name, ct, shape in _abi.MPPI_ADAPT_FIELDS:
                self.buf[name] = torch.zeros(shape(E, K, H), dtype=_TORCH_DTYPE[ct], device=env.device)
                setattr(A, name, C.cast(self.buf[name].data_ptr(), C.POINTER(ct)))
            self._adapt = A
            self.DIAGNOSTICS = DeviceMPPI.DIAGNOSTICS + ("elite_count", "threshold")
        self._temper = None
        if temper is not None:
            T = _abi.MppiTemper()
            T.ess_target, T.lam_min, T.lam_max, T.steps = temper
            for name, ct, shape in _abi.MPPI_TEMPER_FIELDS:
                self.buf[name] = torch.zeros(shape(E, K, H), dtype=_TORCH_DTYPE[ct], device=env.device)
                setattr(T, name, C.cast(self.buf[name].data_ptr(), C.POINTER(ct)))
            self._temper = T
            self.DIAGNOSTICS = self.DIAGNOSTICS + ("lam", "saturated")
        self._noise = None if beta is None else _abi.MppiNoise(beta, 0)
        self.records = torch.zeros((64, _abi.MPPI_STATS_RECORD_WORDS), dtype=torch.int64, device=env.device)  # [capacity] urgym_mppi_stats_record
        self.actor = self.critic = self._guide = None
        P = int(policy_samples)
        if P or terminal_value or fail_cost or policy_sigma:
            try:
                self._guide = self._make_guide(actor, critic, P, float(policy_sigma), bool(terminal_value), float(fail_cost))
            except Exception:
                self.close()
                raise

    def _make_guide(self, actor, critic, P, policy_sigma, terminal_value, fail_cost):
        import ctypes as C
        import os

        import torch

        from . import _abi
        from .vector_env import _TORCH_DTYPE

        E, K = self.env.num_envs, self.samples
        if not 0 <= P <= K - 1:
            raise ValueError(f"DeviceMPPI: policy_samples must be in [0, samples - 1], got {P}")
        if not (np.isfinite(policy_sigma) and policy_sigma >= 0 and np.isfinite(fail_cost) and fail_cost >= 0):
            raise ValueError(f"DeviceMPPI: policy_sigma and fail_cost must be finite and >= 0, got {policy_sigma}, {fail_cost}")
        if (P or terminal_value) and actor is None:
            raise ValueError("DeviceMPPI: policy_samples > 0 and terminal_value need actor=")
        if terminal_value and critic is None:
            raise ValueError("DeviceMPPI: terminal_value needs critic=")
        G = _abi.MppiGuide()
        G.policy_samples, G.terminal_value, G.policy_sigma, G.fail_cost = P, int(terminal_value), policy_sigma, fail_cost
        if actor is not None and (P or terminal_value):
            self.actor = DeviceActor.load(actor, self.planner) if isinstance(actor, (str, os.PathLike)) else DeviceActor(actor, self.planner)
            G.actor = self.actor._a
        if critic is not None and terminal_value:
            paths = isinstance(critic, (tuple, list)) and all(isinstance(c, (str, os.PathLike)) for c in critic)
            self.critic = DeviceCritic.load(critic, self.planner) if paths else DeviceCritic(critic, self.planner)
            G.critic = self.critic._c
        needed = {"policy_action": bool(P or terminal_value), "value": terminal_value, "terminal": terminal_value or fail_cost > 0}
        for name, ct, shape in _abi.MPPI_GUIDE_FIELDS:
            if needed[name]:
                self.buf[name] = torch.zeros(shape(E, K), dtype=_TORCH_DTYPE[ct], device=self.env.device)
                setattr(G, name, C.cast(self.buf[name].data_ptr(), C.POINTER(ct)))
        return G

    @staticmethod
    def check_adapt(samples, sigma, elites=None, adapt_std=False, std_min=0.05, std_max=None):
        """Raises ValueError for what the adaptive entry points refuse about urgym_mppi_adapt's scalars.  Returns None where neither option
        is asked for, else (elites, adapt_std, std_min, std_max) as the struct takes them.  Needs no GPU."""
        if elites is None and not adapt_std:
            return None
        M = int(samples) if elites is None else int(elites)
        if isinstance(elites, bool) or not 1 <= M <= int(samples):
            raise ValueError(f"DeviceMPPI: elites must be in [1, samples], got {elites!r}")
        lo, hi = float(std_min), float(sigma) if std_max is None else float(std_max)
        with np.errstate(over="ignore"):
            ok = bool(np.isfinite(np.float32(lo))) and bool(np.isfinite(np.float32(hi))) and 0.0 <= lo and np.float32(lo) <= np.float32(hi)
        if not ok:
            raise ValueError(f"DeviceMPPI: std_min and std_max must be finite (in float32) with 0 <= std_min <= std_max, got {std_min!r}, {std_max!r}")
        return M, int(bool(adapt_std)), lo, hi

    @staticmethod
    def check_temper(most, ess_target=None, lam_min=1e-3, lam_max=1e6, temper_steps=32):
        """Raises ValueError for what the tempered entry points refuse about urgym_mppi_temper's scalars; `most` is M, the elites, or the
        samples without them.  Returns None where `ess_target` is None (nothing else is looked at), else (ess_target, lam_min, lam_max,
        steps) as the struct takes them.  Needs no GPU."""
        from . import _abi

        if ess_target is None:
            return None
        low, high = _abi.MPPI_TEMPER_LAM_RANGE
        if isinstance(ess_target, bool) or not (np.isfinite(ess_target) and 1.0 <= float(ess_target) <= float(most)):
            raise ValueError(f"DeviceMPPI: ess_target must be finite and in [1, M] (M = {int(most)}: elites, or samples without them), got {ess_target!r}")
        if not (np.isfinite(lam_min) and np.isfinite(lam_max) and low <= float(lam_min) <= float(lam_max) <= high):
            raise ValueError(f"DeviceMPPI: lam_min and lam_max must be finite with 1e-100 <= lam_min <= lam_max <= 1e100, got {lam_min!r}, {lam_max!r}")
        if isinstance(temper_steps, bool) or int(temper_steps) != temper_steps or not 1 <= int(temper_steps) <= _abi.MPPI_TEMPER_STEPS_MAX:
            raise ValueError(f"DeviceMPPI: temper_steps must be an integer in [1, {_abi.MPPI_TEMPER_STEPS_MAX}], got {temper_steps!r}")
        return float(ess_target), float(lam_min), float(lam_max), int(temper_steps)

    @staticmethod
    def check_noise(noise_beta=None):
        """Raises ValueError for what the coloured entry points refuse about urgym_mppi_noise.beta.  Returns None where `noise_beta` is
        None, else beta as the struct takes it (0.0 is a set option).  Needs no GPU."""
        if noise_beta is None:
            return None
        with np.errstate(over="ignore"):
            ok = not isinstance(noise_beta, bool) and bool(np.isfinite(np.float32(noise_beta))) and 0.0 <= float(np.float32(noise_beta)) <= 1.0
        if not ok:
            raise ValueError(f"DeviceMPPI: noise_beta must be finite and in [0, 1] (in float32), got {noise_beta!r}")
        return float(noise_beta)

    def struct(self):
        """The ``urgym_mppi`` of this planner (its pointers stay valid until ``close``)."""
        return self._struct

    def noise(self):
        """The ``urgym_mppi_noise`` of this planner, or None where `noise_beta` was not given."""
        return self._noise

    def sample(self, draw=0, iteration=0, adaptive=False):
        """The single sample launch into ``eps`` and ``actions`` from the mean as it stands: ``urgym_mppi_sample_colored`` with
        `noise_beta` (with `adaptive`, the width is ``std``), else ``urgym_mppi_sample_adaptive`` with `adaptive`, else
        ``urgym_mppi_sample``.  NOT synchronised."""
        import ctypes as C

        from . import _native

        env = self.env
        if adaptive and self._adapt is None:
            raise ValueError("sample(adaptive=True) needs a planner made with elites or adapt_std")
        adapt = C.byref(self._adapt) if adaptive else None
        if self._noise is not None:
            _native.check(env.lib.urgym_mppi_sample_colored(env._h, C.byref(self._struct), C.byref(self._noise), adapt, int(draw), int(iteration), env._stream()), env._h)
        elif adaptive:
            _native.check(env.lib.urgym_mppi_sample_adaptive(env._h, C.byref(self._struct), adapt, int(draw), int(iteration), env._stream()), env._h)
        else:
            _native.check(env.lib.urgym_mppi_sample(env._h, C.byref(self._struct), int(draw), int(iteration), env._stream()), env._h)

    def temper(self):
        """The ``urgym_mppi_temper`` of this planner, or None where `ess_target` was not given."""
        return self._temper

    def update(self):
        """The single update launch on the returns as they stand: ``urgym_mppi_update_tempered`` with `ess_target`, else
        ``urgym_mppi_update_elite`` with elites or the adaptive std, else ``urgym_mppi_update``.  NOT synchronised."""
        import ctypes as C

        from . import _native

        env = self.env
        adapt = None if self._adapt is None else C.byref(self._adapt)
        if self._temper is not None:
            _native.check(env.lib.urgym_mppi_update_tempered(env._h, C.byref(self._struct), C.byref(self._temper), adapt, env._stream()), env._h)
        elif self._adapt is not None:
            _native.check(env.lib.urgym_mppi_update_elite(env._h, C.byref(self._struct), adapt, env._stream()), env._h)
        else:
            _native.check(env.lib.urgym_mppi_update(env._h, C.byref(self._struct), env._stream()), env._h)

    def adapt(self):
        """The ``urgym_mppi_adapt`` of this planner, or None where neither `elites` nor `adapt_std` was given."""
        return self._adapt

    def guide(self):
        """The ``urgym_mppi_guide`` of this planner, or None where the learner is not in the loop."""
        return self._guide

    def plan(self, draw=0):
        """One ``urgym_mppi_plan`` (or its guided, adaptive, tempered or coloured kin, as the options ask) from the environment's state as it stands.  Returns (action_out [E, 6], diagnostics): views of this
        planner's buffers, overwritten by the next plan; diagnostics holds ``best_return``, ``nominal_return`` and ``ess`` [E], with
        elites or the adaptive std ``elite_count`` and ``threshold`` [E], and with `ess_target` ``lam`` and ``saturated`` [E].  NOT
        synchronised."""
        import ctypes as C

        from . import _native

        env = self.env
        guide = None if self._guide is None else C.byref(self._guide)
        if self._noise is not None:
            _native.check(env.lib.urgym_mppi_plan_colored(env._h, self.planner._h, C.byref(self._struct), C.byref(self._noise),
                                                          None if self._temper is None else C.byref(self._temper),
                                                          None if self._adapt is None else C.byref(self._adapt), guide, int(draw), env._stream()), env._h)
        elif self._temper is not None:
            _native.check(env.lib.urgym_mppi_plan_tempered(env._h, self.planner._h, C.byref(self._struct), C.byref(self._temper),
                                                           None if self._adapt is None else C.byref(self._adapt), guide, int(draw), env._stream()), env._h)
        elif self._adapt is not None:
            _native.check(env.lib.urgym_mppi_plan_adaptive(env._h, self.planner._h, C.byref(self._struct), C.byref(self._adapt), guide, int(draw), env._stream()), env._h)
        elif self._guide is None:
            _native.check(env.lib.urgym_mppi_plan(env._h, self.planner._h, C.byref(self._struct), int(draw), env._stream()), env._h)
        else:
            _native.check(env.lib.urgym_mppi_plan_guided(env._h, self.planner._h, C.byref(self._struct), C.byref(self._guide), int(draw), env._stream()), env._h)
        return self.buf["action_out"], {k: self.buf["lam_out" if k == "lam" else k] for k in self.DIAGNOSTICS + (("terminal",) if "terminal" in self.buf else ())}

    def run(self, num_steps, first_draw=0, record=("reward", "terminated", "truncated", "is_success")):
        """`num_steps` x (plan, step the environment with the plan's first action) in ONE native call (``urgym_mppi_control``); step t
        draws with ``first_draw + t``.  `record` names what to keep, as ``UR5ReachVectorEnv.rollout_policy`` does ("all" = every key).
        Returns a dict of fresh device tensors (flags as bool views).  NOT synchronised."""
        import ctypes as C

        import torch

        from . import _abi, _native
        from .vector_env import _TORCH_DTYPE

        env, T = self.env, int(num_steps)
        keys = tuple(name for name, _, _ in _abi.TRAJECTORY_FIELDS)
        names = tuple(k for k in keys if k != "final_observation" or env.cfg.auto_reset) if record == "all" else tuple(record)
        unknown = [n for n in names if n not in keys]
        if unknown:
            raise ValueError(f"unknown record {unknown}; available: {keys}")
        if "final_observation" in names and not env.cfg.auto_reset:
            raise ValueError("final_observation exists only with auto_reset")
        if any(n.startswith("episode_") for n in names) and "episode_done" not in names:
            names += ("episode_done",)
        traj, out = _abi.Trajectory(), {}
        for name, ct, shape in _abi.TRAJECTORY_FIELDS:
            if name in names:
                t = torch.zeros(shape(T, env.num_envs, env.obs_dim, env.goal_dim), dtype=_TORCH_DTYPE[ct], device=env.device)
                setattr(traj, name, C.cast(t.data_ptr(), C.POINTER(ct)))
                out[name] = t.view(torch.bool) if ct is C.c_uint8 else t
        if self._noise is not None:
            _native.check(env.lib.urgym_mppi_control_colored(env._h, self.planner._h, C.byref(self._struct), C.byref(self._noise),
                                                             None if self._temper is None else C.byref(self._temper),
                                                             None if self._adapt is None else C.byref(self._adapt),
                                                             None if self._guide is None else C.byref(self._guide), int(first_draw), T,
                                                             C.byref(traj) if names else None, env._stream()), env._h)
        elif self._temper is not None:
            _native.check(env.lib.urgym_mppi_control_tempered(env._h, self.planner._h, C.byref(self._struct), C.byref(self._temper),
                                                              None if self._adapt is None else C.byref(self._adapt),
                                                              None if self._guide is None else C.byref(self._guide), int(first_draw), T,
                                                              C.byref(traj) if names else None, env._stream()), env._h)
        elif self._adapt is not None:
            _native.check(env.lib.urgym_mppi_control_adaptive(env._h, self.planner._h, C.byref(self._struct), C.byref(self._adapt),
                                                              None if self._guide is None else C.byref(self._guide), int(first_draw), T,
                                                              C.byref(traj) if names else None, env._stream()), env._h)
        elif self._guide is None:
            _native.check(env.lib.urgym_mppi_control(env._h, self.planner._h, C.byref(self._struct), int(first_draw), T, C.byref(traj) if names else None,
                                                     env._stream()), env._h)
        else:
            _native.check(env.lib.urgym_mppi_control_guided(env._h, self.planner._h, C.byref(self._struct), C.byref(self._guide), int(first_draw), T,
                                                            C.byref(traj) if names else None, env._stream()), env._h)
        return out

    @staticmethod
    def check_explore(explore_sigma):
        """Raises ValueError for what urgym_mppi_execute / urgym_mppi_collect refuse about explore_sigma.  Returns it as a float.  Needs no GPU."""
        with np.errstate(over="ignore"):
            ok = not isinstance(explore_sigma, bool) and bool(np.isfinite(np.float32(explore_sigma))) and float(explore_sigma) >= 0.0
        if not ok:
            raise ValueError(f"explore_sigma must be finite (in float32) and >= 0, got {explore_sigma!r}")
        return float(explore_sigma)

    def execute(self, draw=0, explore_sigma=0.0):
        """The action the environment should execute after a ``plan``: ``action_out`` plus `explore_sigma` times the exploration noise of
        `draw`, clamped to [-1, 1] (urgym_mppi_execute: one launch; ``mppi_execute`` on ``mppi_explore_noise`` restates it).  With
        ``explore_sigma == 0`` it is a copy of ``action_out``.  Returns (executed [E, 6], explore_eps [E, 6]): tensors of this planner's,
        allocated at the first call and overwritten by the next.  NOT synchronised."""
        import ctypes as C

        import torch

        from . import _abi, _native

        env = self.env
        x = _abi.MppiExplore(self.check_explore(explore_sigma), 0, None)
        if not self.explore:
            for name in ("executed", "explore_eps"):
                self.explore[name] = torch.zeros((env.num_envs, 6), dtype=torch.float32, device=env.device)
        x.explore_eps = C.cast(self.explore["explore_eps"].data_ptr(), C.POINTER(C.c_float))
        _native.check(env.lib.urgym_mppi_execute(env._h, C.byref(self._struct), C.byref(x), int(draw), C.c_void_p(self.explore["executed"].data_ptr()),
                                                 env._stream()), env._h)
        return self.explore["executed"], self.explore["explore_eps"]

    def collect(self, replay, num_steps, first_draw=0, explore_sigma=0.0, first_slot=None):
        """`num_steps` x (store pass, plan, execute, step the environment) in ONE native call (urgym_mppi_collect) that files every
        transition in `replay` (an ``evaluation.DeviceReplay`` of this planner's environment) as it happens: step t goes to slot
        (first_slot + t) % capacity and draws with ``first_draw + t``.  `first_slot` defaults to the ring's cursor, which this method does
        NOT move -- ``replay.collect_planned`` does.  NOT synchronised."""
        import ctypes as C

        from . import _abi, _native

        env = self.env
        if getattr(replay, "env", None) is not env or not hasattr(replay, "_ring"):
            raise ValueError("replay must be a DeviceReplay allocated for this planner's environment (DeviceReplay(env, capacity_steps))")
        first = replay.cursor if first_slot is None else first_slot
        replay.check_args(replay.capacity, num_steps=num_steps, first_slot=first)
        x = _abi.MppiExplore(self.check_explore(explore_sigma), 0, None)
        guide = None if self._guide is None else C.byref(self._guide)
        if self._noise is not None:
            _native.check(env.lib.urgym_mppi_collect_colored(env._h, self.planner._h, C.byref(self._struct), C.byref(self._noise),
                                                             None if self._temper is None else C.byref(self._temper),
                                                             None if self._adapt is None else C.byref(self._adapt), guide, C.byref(x),
                                                             int(first_draw), int(num_steps), C.byref(replay._ring), int(first), env._stream()), env._h)
            return
        if self._temper is not None:
            _native.check(env.lib.urgym_mppi_collect_tempered(env._h, self.planner._h, C.byref(self._struct), C.byref(self._temper),
                                                              None if self._adapt is None else C.byref(self._adapt), guide, C.byref(x),
                                                              int(first_draw), int(num_steps), C.byref(replay._ring), int(first), env._stream()), env._h)
            return
        if self._adapt is not None:
            _native.check(env.lib.urgym_mppi_collect_adaptive(env._h, self.planner._h, C.byref(self._struct), C.byref(self._adapt), guide, C.byref(x),
                                                              int(first_draw), int(num_steps), C.byref(replay._ring), int(first), env._stream()), env._h)
            return
        _native.check(env.lib.urgym_mppi_collect(env._h, self.planner._h, C.byref(self._struct), guide,
                                                 C.byref(x), int(first_draw), int(num_steps), C.byref(replay._ring), int(first), env._stream()), env._h)

    def stats(self, iteration=0, out=None):
        """The diagnostics the last plan left, reduced over the E parents to one ``urgym_mppi_stats_record`` (urgym_mppi_stats: ONE launch
        of one workgroup; ``mppi_plan_stats`` restates it bitwise).  `out`: an int64 [11] device tensor to write, a row of ``records`` for
        instance; a fresh one by default.  Returns a dict of 0-dim device views of that record under the struct's field names, and the
        row itself under ``"record"``.  NOT synchronised."""
        import ctypes as C

        import torch

        from . import _abi, _native

        env = self.env
        if isinstance(iteration, bool) or int(iteration) != iteration or not -(1 << 63) <= int(iteration) < 1 << 63:
            raise ValueError(f"stats: iteration must be an integer that fits int64, got {iteration!r}")
        if out is None:
            out = torch.zeros((_abi.MPPI_STATS_RECORD_WORDS,), dtype=torch.int64, device=env.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (_abi.MPPI_STATS_RECORD_WORDS,) or not out.is_contiguous() \
                or out.device != torch.device(env.device):
            raise ValueError(f"stats: out must be a contiguous int64 [{_abi.MPPI_STATS_RECORD_WORDS}] tensor on {env.device}")
        _native.check(env.lib.urgym_mppi_stats(env._h, C.byref(self._struct), None if self._adapt is None else C.byref(self._adapt),
                                               C.cast(out.data_ptr(), C.POINTER(_abi.MppiStatsRecord)), int(iteration), env._stream()), env._h)
        return self._record_views(out)

    @staticmethod
    def _record_views(row):
        """The fields of one record row (int64 [11]) as 0-dim views: the doubles and the int64 by word, the int32 by half word."""
        import torch

        from . import _abi

        f64, i32 = row.view(torch.float64), row.view(torch.int32)
        rec, offset = {"record": row}, 0
        for name, ct in _abi.MppiStatsRecord._fields_:
            size = 8 if ct in (_abi.C.c_double, _abi.C.c_int64) else 4
            rec[name] = f64[offset // 8] if ct is _abi.C.c_double else row[offset // 8] if ct is _abi.C.c_int64 else i32[offset // 4]
            offset += size
        return rec

    def reserve_records(self, count):
        """Grows ``records`` to hold at least `count` records; what is there is kept.  Nothing happens where they already fit."""
        import torch

        if int(count) <= self.records.shape[0]:
            return
        grown = torch.zeros((max(int(count), 2 * self.records.shape[0]), self.records.shape[1]), dtype=torch.int64, device=self.records.device)
        grown[:self.records.shape[0]].copy_(self.records)
        self.records = grown

    def plan_stats(self, first, count):
        """Synchronises; records `first` .. `first` + `count` - 1 of ``records`` as dicts under the struct's field names."""
        import ctypes as C

        import torch

        from . import _abi

        torch.cuda.synchronize(self.env.device)
        raw = self.records[int(first):int(first) + int(count)].cpu().numpy().tobytes()
        recs = [_abi.MppiStatsRecord.from_buffer_copy(raw, i * C.sizeof(_abi.MppiStatsRecord)) for i in range(int(count))]
        return [{name: getattr(r, name) for name, _ in _abi.MppiStatsRecord._fields_} for r in recs]

    def planning(self, explore_sigma=0.0, sync=True, records=False):
        """The ``urgym_sac_planning`` of an ``env.sac_train(planner=)`` call: this planner's handle and structs, the exploration noise,
        whether the actor and the critic follow the learner, and, with `records`, ``records`` as it stands (``reserve_records`` first)."""
        import ctypes as C

        from . import _abi

        P = _abi.SacPlanning()
        P.planner_handle = self.planner._h
        P.mppi = C.pointer(self._struct)
        if self._adapt is not None:
            P.adapt_or_NULL = C.pointer(self._adapt)
        if self._guide is not None:
            P.guide_or_NULL = C.pointer(self._guide)
        P.explore = _abi.MppiExplore(self.check_explore(explore_sigma), 0, None)
        P.sync = int(bool(sync))
        if records:
            P.record_capacity = int(self.records.shape[0])
            P.records = C.cast(self.records.data_ptr(), C.POINTER(_abi.MppiStatsRecord))
        return P

    def reset_plan(self, mask=None):
        """Zeroes the nominal sequence of every env, or of those `mask` (a bool [E] tensor or array, or env ids) selects."""
        import torch

        if mask is None:
            self.buf["mean"].zero_()
        else:
            self.buf["mean"][:, torch.as_tensor(mask, device=self.env.device)] = 0.0

    def close(self):
        for name in ("actor", "critic"):  # they live in the planner's handle
            if getattr(self, name, None) is not None:
                getattr(self, name).close()
                setattr(self, name, None)
        if getattr(self, "planner", None) is not None:
            self.planner.close()
            self.planner = None


def run_closed_loop_mppi(env, points=None, max_steps=100, first_draw=0, **planner):
    """``run_closed_loop_device`` with an MPPI planner in place of ``model.predict``: model_test.py's protocol (model_test.py:26-61) for all
    envs of `env` at once, a UR5ReachVectorEnv with auto-reset off that has been reset.  `points`, if given, are one test point per env,
    set with ``set_goal`` (UR5OriReach-v1) or ``set_goal_and_obstacle`` first.  `planner` are ``DeviceMPPI``'s keywords.  One native call;
    returns the same dictionary."""
    import torch

    from . import _abi

    if env.cfg.auto_reset:
        raise ValueError("run_closed_loop_mppi: env must be made with auto_reset=False")
    if points is not None:
        (env.set_goal if env.env_kind == _abi.ENV_ORI else env.set_goal_and_obstacle)(np.arange(env.num_envs), points)
    mppi = DeviceMPPI(env, **planner)
    try:
        rec = mppi.run(max_steps, first_draw, record=("episode_return", "episode_last_step", "episode_success"))
        torch.cuda.synchronize(env.device)
    finally:
        mppi.close()
    reward = rec["episode_return"].cpu().numpy()
    success = rec["episode_success"].cpu().numpy().astype(bool)
    last = rec["episode_last_step"].cpu().numpy().astype(np.float64)
    return {"success_rate_percent": 100.0 * success.mean(), "mean_episode_reward": float(reward.mean()),
            "mean_last_step_index": float(last.mean()), "success": success, "reward": reward, "last_step": last}



# ------------------------------------------------------------------------------------------------ the scripted reach controller
def _ik_model():
    """joint_xyz [6, 3] and the fixed rotations [6, 3, 3] of the URDF's joint origins, R = Rz(yaw) Ry(pitch) Rx(roll) of joint_rpy
    (data/ur5e_model.npz) -- formed here from the angles, not read from the table the kernels use."""
    import os

    if not hasattr(_ik_model, "cache"):
        with np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "ur5e_model.npz")) as m:
            xyz, rpy = np.array(m["joint_xyz"], np.float64), np.array(m["joint_rpy"], np.float64)
        _ik_model.cache = (xyz, np.stack([_ik_rpy_matrix(a[None])[0] for a in rpy]))
    return _ik_model.cache


def _ik_rpy_matrix(rpy):
    """[M, 3] fixed-axis roll-pitch-yaw -> [M, 3, 3], R = Rz(yaw) Ry(pitch) Rx(roll): the URDF's convention, and the rotation of
    pybullet's getQuaternionFromEuler."""
    (cr, cp, cy), (sr, sp, sy) = np.cos(rpy).T, np.sin(rpy).T
    R = np.empty(rpy.shape[:1] + (3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sp, cp * sr, cp * cr
    return R


def _ik_rotation_quat(D):
    """[M, 3, 3] rotations -> [M, 4] unit quaternions xyzw with w >= 0 (Shepperd: the largest of the four squares leads)."""
    tr = D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2]
    four = np.stack([1 + 2 * D[:, 0, 0] - tr, 1 + 2 * D[:, 1, 1] - tr, 1 + 2 * D[:, 2, 2] - tr, 1 + tr], 1)  # 4 x^2, 4 y^2, 4 z^2, 4 w^2
    lead = four.argmax(1)
    sym = lambda i, j: D[:, i, j] + D[:, j, i]
    skew = np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1)  # 4 w (x, y, z)
    rows = np.stack([np.stack([four[:, 0], sym(0, 1), sym(0, 2), skew[:, 0]], 1), np.stack([sym(0, 1), four[:, 1], sym(1, 2), skew[:, 1]], 1),
                     np.stack([sym(0, 2), sym(1, 2), four[:, 2], skew[:, 2]], 1), np.stack([skew[:, 0], skew[:, 1], skew[:, 2], four[:, 3]], 1)], 1)
    q = rows[np.arange(len(D)), lead]  # 4 q_lead q
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(q[:, 3:] < 0, -q, q)


def ik_chain(q):
    """The chain walk in float64 numpy from the URDF's joint origins: `q` [M, 6] -> (z [M, 6, 3] joint axes, o [M, 6, 3] joint origins,
    R [M, 3, 3] and p [M, 3] of the end-effector, link 6), all in the world frame."""
    xyz, fixed = _ik_model()
    q = np.asarray(q, np.float64)
    M = len(q)
    R, t = np.broadcast_to(np.eye(3), (M, 3, 3)).copy(), np.zeros((M, 3))
    z, o = np.empty((M, 6, 3)), np.empty((M, 6, 3))
    for k in range(6):
        c, s = np.cos(q[:, k]), np.sin(q[:, k])
        t = t + R @ xyz[k]
        G = R @ fixed[k]
        o[:, k], z[:, k] = t, G[:, :, 2]
        Rz = np.zeros((M, 3, 3))
        Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
        R = G @ Rz
    return z, o, R, t


def ik_terms(q, goal, env_kind, damping):
    """The Jacobian, the error, A = J J^T + damping^2 I and the solution y of A y = e of the reach controller (include/urgym.h, "a
    scripted reach controller on the device"), float64 numpy: `q` [M, 6], `goal` [M, 6] or [M, 3] (rows 3.. are not read for
    UR5ObsReach-v1).  Returns a dict J [M, 6, 6], e [M, 6], A [M, 6, 6], y [M, 6], dw [M] (the scalar part of the error quaternion
    before the shortest-arc flip; 1 where the kind has no orientation)."""
    from . import _abi

    q, goal = np.atleast_2d(np.asarray(q, np.float64)), np.atleast_2d(np.asarray(goal, np.float64))
    rotational = _abi.OBS_DIMS[env_kind][1] == 6
    z, o, R, p = ik_chain(q)
    M = len(q)
    J, e, dw = np.zeros((M, 6, 6)), np.zeros((M, 6)), np.ones(M)
    J[:, :3, :] = np.cross(z, p[:, None, :] - o).transpose(0, 2, 1)
    e[:, :3] = goal[:, :3] - p
    if rotational:
        J[:, 3:, :] = z.transpose(0, 2, 1)
        D = _ik_rpy_matrix(goal[:, 3:6]) @ R.transpose(0, 2, 1)  # the rotation of q_goal (x) conj(q_ee)
        d = _ik_rotation_quat(D)
        # the sign the product of the two quaternions carries before the flip is not a property of D: |d.w| is, and that is what the
        # shortest-arc discontinuity depends on
        dw = d[:, 3]
        n = np.linalg.norm(d[:, :3], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(n < 1e-12, 2.0, 2.0 * np.arctan2(n, d[:, 3]) / n)
        e[:, 3:] = d[:, :3] * scale[:, None]
    A = J @ J.transpose(0, 2, 1) + float(damping) ** 2 * np.eye(6)
    y = np.linalg.solve(A, e[:, :, None])[:, :, 0]
    return dict(J=J, e=e, A=A, y=y, dw=dw)


def ik_actions(q, goal, env_kind, damping, gain, action_scale):
    """THE STEP of the reach controller in float64 numpy, rounded once to float32: `q` [M, 6] (or [6]), `goal` [M, 6] or [M, 3] ->
    float32 [M, 6].  dq = gain J^T y with y of ``ik_terms``; a = dq / action_scale; the whole row is divided by max |a_c| where that
    exceeds 1.  A row whose q or goal (the columns its kind reads) is not finite gets zeros.  Written from the URDF's joint origins, not
    from ur_gym_amd/csrc/urgym_ik.h: the kernel is held to 2^-22 of this."""
    from . import _abi

    q, goal = np.atleast_2d(np.asarray(q, np.float64)), np.atleast_2d(np.asarray(goal, np.float64))
    gd = _abi.OBS_DIMS[env_kind][1]
    if q.shape[1] != 6 or goal.shape[0] != q.shape[0] or goal.shape[1] < gd:
        raise ValueError(f"q must be [M, 6] and goal [M, >= {gd}], got {q.shape} and {goal.shape}")
    ok = np.isfinite(q).all(1) & np.isfinite(goal[:, :gd]).all(1)
    out = np.zeros((len(q), 6), np.float32)
    if ok.any():
        t = ik_terms(q[ok], goal[ok], env_kind, damping)
        a = float(gain) * np.einsum("mrk,mr->mk", t["J"], t["y"]) / float(action_scale)
        m = np.abs(a).max(1, keepdims=True)
        a = np.where(m > 1.0, a / np.where(m > 1.0, m, 1.0), a)
        fin = np.isfinite(a).all(1)
        rows = np.flatnonzero(ok)
        out[rows[fin]] = a[fin].astype(np.float32)
    return out


def ik_explore_counters(draw, envs):
    """The two Philox counters of the reach controller's exploration noise of (env n, draw): 4-tuples (n, 0, draw, IK_TAG | block) for
    block 0 and block 1, `envs` an integer or an integer array."""
    from . import _abi

    draw = int(draw)
    if not 0 <= draw < 1 << 32:
        raise ValueError(f"draw must be in [0, 2^32), got {draw}")
    n = np.asarray(envs, dtype=np.uint64)
    if n.size and int(n.max()) >= 1 << 31:
        raise ValueError("envs must be env indices")
    return tuple((n, np.uint64(0), np.uint64(draw), np.uint64(_abi.IK_TAG | b)) for b in (0, 1))


def ik_box_muller(m):
    """Box-Muller of the reach controller's noise, bit for bit (ur_gym_amd/csrc/urgym_ik.h: ik_ln_unit, ik_sincospi, ik_box_muller): `m`
    integers below 2^24 of shape + (6,), the pairs (m[2p], m[2p + 1]); returns float32 of the same shape.  The pairing is the planner's
    (u1 = (m1 + 1) 2^-24, angle = 2 pi m2 2^-24, r = sqrt(-2 ln u1), (r cos, r sin)), but ln, cos and sin are the float64 lines the
    header states -- every operation below is one IEEE operation, in the header's order -- so the device's noise can be restated
    exactly, which a library's logf and cospif cannot."""
    m = np.asarray(m)
    M = m[..., 0::2].astype(np.float64) + 1.0
    f, e = np.frexp(M)
    low = f < 0.7071067811865476
    f, e = np.where(low, f * 2.0, f), np.where(low, e - 1, e)
    s = (f - 1.0) / (f + 1.0)
    z = s * s
    p = np.full(z.shape, 1.0 / 13.0)
    for c in (1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0):
        p = p * z
        p = p + c
    ln = (e - 24).astype(np.float64) * 0.6931471805599453 + 2.0 * (s * p)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(-2.0 * ln)
    t = m[..., 1::2].astype(np.float64) * (1.0 / 8388608.0)
    k = np.rint(t * 2.0)
    x = 3.141592653589793 * (t - k * 0.5)
    z = x * x
    ps = np.full(z.shape, 1.0 / 6227020800.0)
    for c in (-1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
        ps = ps * z
        ps = ps + c
    sn = x * ps
    pc = np.full(z.shape, -1.0 / 87178291200.0)
    for c in (1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -1.0 / 2.0):
        pc = pc * z
        pc = pc + c
    cs = pc * z + 1.0
    q = k.astype(np.int64) & 3
    sin = np.select([q == 0, q == 1, q == 2], [sn, cs, -sn], -cs)
    cos = np.select([q == 0, q == 1, q == 2], [cs, -sn, -cs], sn)
    out = np.empty(m.shape, np.float32)
    out[..., 0::2], out[..., 1::2] = (r * cos).astype(np.float32), (r * sin).astype(np.float32)
    return out


def ik_explore_noise(seed, draw, N, dtype=np.float32):
    """The exploration noise of the reach controller, restated from include/urgym.h: six normals for each of the envs 0 .. N - 1, a
    pure function of (seed, draw, env, component), on the words of the counters ``ik_explore_counters`` states with key (seed lo,
    seed hi).  With the default `dtype` it is ``ik_box_muller``, BIT FOR BIT what the device reports in ``explore_eps``; with
    ``np.float64`` it is the planner's ``_box_muller`` in float64 on the same words (numpy's log, cos and sin), the yardstick that says
    the stated lines compute Box-Muller.  Returns [N, 6]; the executed action is ``mppi_execute(action, eps, explore_sigma)``."""
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    c0, c1 = ik_explore_counters(draw, np.arange(int(N)))
    a, b = philox4x32_10(key, c0), philox4x32_10(key, c1)
    if dtype is np.float32:
        return ik_box_muller(_noise_integers(a, b, np.float64).astype(np.int64))
    return _box_muller(_noise_integers(a, b, dtype), dtype)


class DeviceReachController:
    """A scripted expert for the reach tasks: resolved-rate control by damped least-squares inverse kinematics, one small launch per
    control step on the environment's own state (urgym_controller_*).  It needs no second environment and no
    training; it does not see obstacles, so its failures are collisions on the way.  `env` is a UR5ReachVectorEnv; `seed` keys the
    exploration noise.  Holds no native object: there is nothing to close."""

    def __init__(self, env, damping=0.2, gain=0.5, seed=0):
        self.env = env
        self.damping, self.gain, self.seed, _ = env.check_controller(damping, gain, seed, 0.0)
        self.explore_eps = None

    def _eps(self):
        import torch

        if self.explore_eps is None:
            self.explore_eps = torch.zeros((self.env.num_envs, 6), dtype=torch.float32, device=self.env.device)
        return self.explore_eps

    def _keywords(self, explore_sigma):
        return dict(damping=self.damping, gain=self.gain, seed=self.seed, explore_sigma=explore_sigma, explore_eps=self._eps())

    def actions(self, draw=0, explore_sigma=0.0, out=None):
        """The action of every env for the state it is in (``env.controller_actions``: one launch); ``self.explore_eps`` then holds the
        noise of `draw` (zeros with ``explore_sigma == 0``).  Returns `out` (allocated if None).  NOT synchronised."""
        return self.env.controller_actions(out=out, draw=draw, **self._keywords(explore_sigma))

    def run(self, num_steps, first_draw=0, record=("reward", "terminated", "truncated", "is_success"), explore_sigma=0.0):
        """`num_steps` x (action, step) in ONE native call (``env.controller_control``); returns its dict of device tensors."""
        return self.env.controller_control(num_steps, first_draw=first_draw, record=record, **self._keywords(explore_sigma))

    def collect(self, replay, num_steps, first_draw=0, explore_sigma=0.0, first_slot=None):
        """`num_steps` x (store pass, action, step) in ONE native call that files every transition in `replay`
        (``env.controller_collect``); does NOT move the ring's cursor -- ``replay.collect_scripted`` does."""
        self.env.controller_collect(replay, num_steps, first_draw=first_draw, first_slot=first_slot, **self._keywords(explore_sigma))

    def close(self):
        self.explore_eps = None


def run_closed_loop_controller(env, points=None, max_steps=100, first_draw=0, explore_sigma=0.0, **controller):
    """``run_closed_loop_mppi`` with the scripted reach controller in place of the planner: model_test.py's protocol
    (model_test.py:26-61) for all envs of `env` at once, a UR5ReachVectorEnv with auto-reset off that has been reset.  `points`, if
    given, are one test point per env, set with ``set_goal`` (UR5OriReach-v1) or ``set_goal_and_obstacle`` first.  `controller` are
    ``DeviceReachController``'s keywords.  One native call; returns the same dictionary."""
    import torch

    from . import _abi

    if env.cfg.auto_reset:
        raise ValueError("run_closed_loop_controller: env must be made with auto_reset=False")
    if points is not None:
        (env.set_goal if env.env_kind == _abi.ENV_ORI else env.set_goal_and_obstacle)(np.arange(env.num_envs), points)
    rec = DeviceReachController(env, **controller).run(max_steps, first_draw, record=("episode_return", "episode_last_step", "episode_success"),
                                                       explore_sigma=explore_sigma)
    torch.cuda.synchronize(env.device)
    reward = rec["episode_return"].cpu().numpy()
    success = rec["episode_success"].cpu().numpy().astype(bool)
    last = rec["episode_last_step"].cpu().numpy().astype(np.float64)
    return {"success_rate_percent": 100.0 * success.mean(), "mean_episode_reward": float(reward.mean()),
            "mean_last_step_index": float(last.mean()), "success": success, "reward": reward, "last_step": last}
