"""A policy in the loop on the device: the HIP actor kernel (urgym_actor_forward) and the recorded closed-loop rollout
(urgym_rollout_actor), through ``DeviceActor``, ``UR5ReachVectorEnv.policy_actions`` / ``rollout_policy`` and
``run_closed_loop_device``.

What is pinned and against what:
  * the actor against a float64 numpy evaluation of the same weights on the same float32 inputs.  The bound is not a chosen number:
    on the same inputs the float32 numpy ``DeterministicActor`` (what the host loop uses) is measured against float64, and the
    kernel -- another float32 summation order of the same function, plus the device tanh -- gets 4 x that deviation;
  * the records and the interleaved launches by teacher-forced replay: a second environment stepped from Python with the recorded
    actions must reproduce every recorded row and the final state BITWISE;
  * the episode summary against ``run_closed_loop``'s bookkeeping applied to the recorded per-step rows;
  * the whole thing against the reference's per-trial statistics (tests/test_closed_loop.py::check_against_reference).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import ACTOR_ARRAYS, DeterministicActor, DeviceActor, run_closed_loop, run_closed_loop_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTORS = os.path.join(ROOT, "tests", "golden", "actors")
ENVS = {"ori": "UR5OriReach-v1", "obs": "UR5ObsReach-v1", "sta": "UR5StaReach-v1", "dyn": "UR5DynReach-v1"}
NEW_SYMBOLS = ("urgym_actor_create", "urgym_actor_destroy", "urgym_actor_forward", "urgym_rollout_actor")


# ------------------------------------------------------------------------------------------------ CPU
def _struct_fields(hdr, name):
    body = hdr[hdr.index(f"typedef struct {name}"):hdr.index(f"}} {name};")]
    return re.findall(r"^\s*(?:const\s+)?(?:double|float|int32_t|uint8_t)\s*\*?\s*(\w+);", body, flags=re.M)


def test_actor_and_trajectory_structs_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    desc = _struct_fields(hdr, "urgym_actor_desc")
    assert desc == [f[0] for f in _abi.ActorDesc._fields_] and len(desc) == 10
    traj = _struct_fields(hdr, "urgym_trajectory")
    assert traj == [f[0] for f in _abi.Trajectory._fields_] == [name for name, _, _ in _abi.TRAJECTORY_FIELDS] and len(traj) == 14
    # element types of the trajectory pointers, as the header spells them
    body = hdr[hdr.index("typedef struct urgym_trajectory"):hdr.index("} urgym_trajectory;")]
    ctype = {"float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "uint8_t": C.c_uint8}
    for t, name in re.findall(r"^\s*(double|float|int32_t|uint8_t)\*\s*(\w+);", body, flags=re.M):
        assert dict((n, c) for n, c, _ in _abi.TRAJECTORY_FIELDS)[name] is ctype[t], name
    assert _abi.ABI_VERSION == 4 and int(re.search(r"#define URGYM_ABI_VERSION (\d+)", hdr).group(1)) == 4
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


def test_device_actor_shape_checks_need_no_gpu():
    good = dict(np.load(os.path.join(ACTORS, "actor_dyn.npz")))
    assert DeviceActor.check_shapes(good, _abi.ENV_DYN) == (47, 256)
    for name, kind, n_in in (("ori", _abi.ENV_ORI, 30), ("obs", _abi.ENV_OBS, 32), ("sta", _abi.ENV_STA, 41)):
        assert DeviceActor.check_shapes(dict(np.load(os.path.join(ACTORS, f"actor_{name}.npz"))), kind) == (n_in, 256)
    with pytest.raises(ValueError, match="features"):
        DeviceActor.check_shapes(good, _abi.ENV_ORI)  # wrong in_features for the env kind
    rng = np.random.default_rng(0)

    def make(n_in, h0, h1, out=6):
        return {"latent_pi_0_weight": rng.normal(size=(h0, n_in)), "latent_pi_0_bias": np.zeros(h0), "latent_pi_2_weight": rng.normal(size=(h1, h0)),
                "latent_pi_2_bias": np.zeros(h1), "mu_weight": rng.normal(size=(out, h1)), "mu_bias": np.zeros(out)}

    assert DeviceActor.check_shapes(make(47, 64, 64), _abi.ENV_DYN) == (47, 64)
    assert DeviceActor.check_shapes(make(47, 512, 512), _abi.ENV_DYN) == (47, 512)
    with pytest.raises(ValueError, match="one width"):
        DeviceActor.check_shapes(make(47, 256, 128), _abi.ENV_DYN)
    with pytest.raises(ValueError, match="multiple of 32"):
        DeviceActor.check_shapes(make(47, 100, 100), _abi.ENV_DYN)
    with pytest.raises(ValueError, match="multiple of 32"):
        DeviceActor.check_shapes(make(47, 544, 544), _abi.ENV_DYN)
    with pytest.raises(ValueError, match="6 outputs"):
        DeviceActor.check_shapes(make(47, 64, 64, out=7), _abi.ENV_DYN)
    for k in ACTOR_ARRAYS:
        with pytest.raises(ValueError, match="missing"):
            DeviceActor.check_shapes({n: v for n, v in good.items() if n != k}, _abi.ENV_DYN)


# ------------------------------------------------------------------------------------------------ GPU
def _actor_f64(w, x):
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    h = np.maximum(x.astype(np.float64) @ w["latent_pi_0_weight"].T + w["latent_pi_0_bias"], 0.0)
    h = np.maximum(h @ w["latent_pi_2_weight"].T + w["latent_pi_2_bias"], 0.0)
    return np.tanh(h @ w["mu_weight"].T + w["mu_bias"])


def _bits(t):
    import torch

    return t.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ori", "obs", "sta", "dyn"])
def test_actor_kernel_against_float64(name):
    """Bound = 4 x the deviation of the float32 numpy actor from float64, measured here on the N = 4096 inputs of this actor.  The
    N = 1 and N = 4097 runs (partial tiles) take the same bound: a maximum over six numbers is no stable measurement of a summation
    order's error, and they draw from the same observations.  Measured on MI355X at N = 4096, Ori / Obs /
    Sta / Dyn: numpy float32 3.2e-6 / 3.4e-6 / 1.2e-5 / 4.9e-6 from float64, the kernel 4.3e-6 / 3.7e-6 / 9.0e-6 / 9.9e-6."""
    import torch

    from ur_gym_amd import make_vec

    path = os.path.join(ACTORS, f"actor_{name}.npz")
    w = dict(np.load(path))
    host = DeterministicActor(w)
    bound = None
    for n in (4096, 1, 4097):
        env = make_vec(ENVS[name], num_envs=n, device="cuda:0", seed=21)
        env.reset(seed=21)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(5)
        for _ in range(20):  # leave the neutral pose
            env.step(torch.rand((n, 6), device="cuda:0", generator=g) * 2.0 - 1.0)
        actor = DeviceActor.load(path, env)
        got = env.policy_actions(actor).cpu().numpy()
        ach, des, obs = (env.buf[k].cpu().numpy() for k in ("achieved_goal", "desired_goal", "observation"))
        ref = _actor_f64(w, np.concatenate([ach, des, obs], axis=1))
        dev_numpy = float(np.abs(host(ach, des, obs).astype(np.float64) - ref).max())
        dev_kernel = float(np.abs(got.astype(np.float64) - ref).max())
        if bound is None:
            bound = 4.0 * dev_numpy
        print(f"actor {name} N={n}: numpy float32 vs float64 {dev_numpy:.3e}, kernel vs float64 {dev_kernel:.3e}, bound {bound:.3e}, "
              f"saturated {float((np.abs(ref) > 0.999).mean()):.3f}")
        assert got.shape == (n, 6) and got.dtype == np.float32
        assert dev_kernel <= bound, (name, n, dev_kernel, bound)
        actor.close()
        env.close()


def replay_teacher_forced(name, n, steps, w, sample=None, seed=17, min_finished=None):
    """The body of the teacher-forced replay tests (tests/test_policy_sampling.py and tests/test_actor_widths.py run it too): a
    recorded rollout of `steps` steps with the actor of the arrays `w` -- sampled if `sample` is given --, then a second environment
    stepped from Python with the recorded actions, which must reproduce every recorded row and the final state BITWISE.  More than
    `min_finished` (default n // 2) episodes must have ended on the way, so that final_observation had rows to be compared on.
    Returns the records."""
    import torch

    from ur_gym_amd import make_vec

    env_a = make_vec(ENVS[name], num_envs=n, device="cuda:0", seed=seed, auto_reset=True)
    env_b = make_vec(ENVS[name], num_envs=n, device="cuda:0", seed=seed, auto_reset=True)
    env_a.reset(seed=seed)
    env_b.reset(seed=seed)
    actor = DeviceActor(w, env_a)
    rec = env_a.rollout_policy(actor, steps, record="all", sample=sample)
    torch.cuda.synchronize()
    assert set(rec) == set(env_a.RECORD_KEYS + (env_a.SAMPLE_RECORD_KEYS if sample is not None else ()))
    finished = 0
    for k in range(steps):
        for key in ("observation", "achieved_goal", "desired_goal"):
            assert _same_bits(rec[key][k], env_b.buf[key]), (key, k)
        obs, rew, term, trunc, info = env_b.step(rec["action"][k])
        assert _same_bits(rec["reward"][k], rew), ("reward", k)
        assert torch.equal(rec["terminated"][k], term) and torch.equal(rec["truncated"][k], trunc), ("flags", k)
        assert torch.equal(rec["is_success"][k], info["is_success"]) and torch.equal(rec["collision"][k], info["collision"]), ("info", k)
        fin = term | trunc
        assert _same_bits(rec["final_observation"][k][fin], info["final_observation"]["observation"][fin]), ("final_observation", k)
        finished += int(fin.sum())
    assert finished > (n // 2 if min_finished is None else min_finished)  # the check above had rows to look at
    if steps > 100:
        assert bool(rec["truncated"].any())  # K passes the common truncation at step 100
    torch.cuda.synchronize()
    for key in env_a.buf:
        if key in ("done_list", "done_count"):  # scratch of the reset path, not state
            continue
        assert _same_bits(env_a.buf[key], env_b.buf[key]), key
    actor.close()
    env_a.close()
    env_b.close()
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps", [("dyn", 4096, 130), ("obs", 1000, 20)])
def test_teacher_forced_replay_is_bitwise(name, n, steps):
    replay_teacher_forced(name, n, steps, dict(np.load(os.path.join(ACTORS, f"actor_{name}.npz"))))


@pytest.mark.gpu
def test_episode_summary_is_run_closed_loop_bookkeeping():
    import torch

    from ur_gym_amd import make_vec

    n, steps = 2000, 100
    env = make_vec("UR5DynReach-v1", num_envs=n, device="cuda:0", seed=9, auto_reset=False)
    env.reset(seed=9)
    actor = DeviceActor.load(os.path.join(ACTORS, "actor_dyn.npz"), env)
    rec = env.rollout_policy(actor, steps, record=("reward", "terminated", "is_success", "episode_return", "episode_last_step",
                                                   "episode_success", "episode_done"))
    torch.cuda.synchronize()
    r, term, succ = (rec[k].cpu().numpy() for k in ("reward", "terminated", "is_success"))
    done, success, reward, last = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n), np.zeros(n, np.int32)
    for t in range(steps):  # run_closed_loop, on the recorded rows
        live = ~done
        reward[live] += r[t][live].astype(np.float64)
        fin = live & (term[t] | (t == steps - 1))
        success[fin] = succ[t][fin]
        last[fin] = t
        done |= fin
    assert np.array_equal(rec["episode_last_step"].cpu().numpy(), last)
    assert np.array_equal(rec["episode_success"].cpu().numpy(), success)
    assert np.array_equal(rec["episode_done"].cpu().numpy(), done) and done.all()
    got = rec["episode_return"].cpu().numpy()
    assert got.dtype == np.float64 and np.all(np.abs(got - reward) <= 1e-9 * np.abs(reward))
    assert 0.5 < success.mean() < 1.0 and last.min() < steps - 1  # episodes of both kinds took part
    actor.close()
    env.close()


@pytest.mark.gpu
def test_device_closed_loop_reproduces_the_reference_protocol():
    """The four trial sets of test_closed_loop_hip_full_protocol (same points, same seeds), actor and bookkeeping on the device."""
    import torch

    from test_closed_loop import DYN_HIGH, DYN_LOW, ORI_HIGH, ORI_LOW, REF, check_against_reference, constrained_euler, dyn_points, goal_grid
    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import HipBackend

    rng = np.random.default_rng(0)
    grid = goal_grid(ORI_LOW, ORI_HIGH)
    ori_pts = np.concatenate([grid, constrained_euler(rng, len(grid))], axis=1)

    def draw(n):
        gen = make_vec("UR5DynReach-v1", num_envs=n, device="cuda:0", seed=3, auto_reset=False, min_travel=0.3)
        gen.reset(seed=3)
        torch.cuda.synchronize()
        st = gen.get_state()
        gen.close()
        return st["goal"][3:].T.copy(), st["obst_start"].T.copy(), st["obst_end"].T.copy()

    probe_env = make_vec("UR5DynReach-v1", num_envs=64, device="cuda:0", seed=0)

    def clearance(goal6, end6):
        from scipy.spatial.transform import Rotation as Rot

        n = len(goal6)
        qa = Rot.from_euler("xyz", goal6[:, 3:]).as_quat()
        qb = Rot.from_euler("xyz", end6[:, 3:]).as_quat()
        d, _ = probe_env.probe_closest(np.full(n, 2), np.tile([0.025] * 3, (n, 1)), np.c_[goal6[:, :3], qa], np.full(n, 1),
                                       np.tile([0.05, 0.4, 0.0], (n, 1)), np.c_[end6[:, :3], qb])
        return d

    dyn_pts = dyn_points(draw, clearance, 10 ** 9, rng)
    probe_env.close()

    def ori_env():
        env = make_vec("UR5OriReach-v1", num_envs=len(ori_pts), device="cuda:0", seed=1, auto_reset=False)
        env.reset(seed=1)
        env.set_goal(np.arange(len(ori_pts)), ori_pts)
        return env

    def dyn_env():
        env = make_vec("UR5DynReach-v1", num_envs=len(dyn_pts), device="cuda:0", seed=4, auto_reset=False)
        env.reset(seed=4)
        env.set_goal_and_obstacle(np.arange(len(dyn_pts)), dyn_pts)
        return env

    def reset_env(env_id, seed):
        def make():
            env = make_vec(env_id, num_envs=5000, device="cuda:0", seed=seed, auto_reset=False, link_dist_scope=_abi.LINK_DIST_WORKBENCH)
            env.reset(seed=seed)
            return env
        return make

    out = {}
    for name, make in (("ori", ori_env), ("dyn", dyn_env), ("sta", reset_env("UR5StaReach-v1", 5)), ("obs", reset_env("UR5ObsReach-v1", 2))):
        path = os.path.join(ACTORS, f"actor_{name}.npz")
        env = make()
        actor = DeviceActor.load(path, env)
        out[name] = run_closed_loop_device(env, actor)
        actor.close()
        env.close()
        env = make()
        host = run_closed_loop(HipBackend(env), DeterministicActor.load(path))
        env.close()
        r = out[name]
        print(f"{name} closed loop (device actor): success {r['success_rate_percent']:.2f}%  reward {r['mean_episode_reward']:.2f}  "
              f"last step {r['mean_last_step_index']:.2f}; host loop: success {host['success_rate_percent']:.2f}%; "
              f"trials whose success flag differs from the host loop's: {100.0 * float((r['success'] != host['success']).mean()):.3f} %")
    assert len(out["ori"]["success"]) == REF["ori"]["trials"] and len(out["dyn"]["success"]) == REF["dyn"]["trials"]
    check_against_reference("ori", out["ori"], REF["ori"]["trials"], reward=True)
    check_against_reference("dyn", out["dyn"], REF["dyn"]["trials"], reward=True)
    check_against_reference("sta", out["sta"], 5000)
    check_against_reference("obs", out["obs"], 5000)


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable():
    import torch

    from ur_gym_amd import make_vec

    lib = _native.lib()
    n = 300
    env = make_vec("UR5DynReach-v1", num_envs=n, device="cuda:0", seed=2)
    other = make_vec("UR5OriReach-v1", num_envs=n, device="cuda:0", seed=2)
    actor = DeviceActor.load(os.path.join(ACTORS, "actor_dyn.npz"), env)
    ori_actor = DeviceActor.load(os.path.join(ACTORS, "actor_ori.npz"), other)
    stream = env._stream()
    # before reset: no observations to act on
    assert lib.urgym_rollout_actor(env._h, actor._a, 3, None, stream) == _abi.ERR_STATE
    assert b"urgym_reset" in lib.urgym_last_error(env._h)
    with pytest.raises(_native.NativeError):
        env.rollout_policy(actor, 3)
    env.reset(seed=2)
    other.reset(seed=2)
    # an actor made for another env kind (it lives in that env's handle)
    assert lib.urgym_rollout_actor(env._h, ori_actor._a, 3, None, stream) == _abi.ERR_ARG
    assert lib.urgym_actor_forward(env._h, ori_actor._a, C.c_void_p(env.buf["reward"].data_ptr()), stream) == _abi.ERR_ARG
    with pytest.raises(ValueError):
        env.rollout_policy(ori_actor, 3)
    assert lib.urgym_rollout_actor(env._h, actor._a, -1, None, stream) == _abi.ERR_ARG
    assert lib.urgym_actor_forward(env._h, actor._a, None, stream) == _abi.ERR_ARG
    # urgym_actor_create: shapes the kernel does not take
    w = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in np.load(os.path.join(ACTORS, "actor_dyn.npz")).items()}
    ptr = [w[k].ctypes.data_as(C.POINTER(C.c_float)) for k in ACTOR_ARRAYS]
    for n_in, width, n_out, arrays in ((41, 256, 6, ptr), (47, 100, 6, ptr), (47, 544, 6, ptr), (47, 0, 6, ptr), (47, 256, 7, ptr),
                                       (47, 256, 6, ptr[:5] + [None])):
        made = C.c_void_p()
        desc = _abi.ActorDesc(n_in, width, n_out, 0, *arrays)
        assert lib.urgym_actor_create(env._h, C.byref(desc), C.byref(made)) == _abi.ERR_ARG, (n_in, width, n_out)
        assert b"urgym_actor_create" in lib.urgym_last_error(env._h) and not made.value
    with pytest.raises(ValueError):
        DeviceActor.load(os.path.join(ACTORS, "actor_ori.npz"), env)
    # the handle still works, with and without records; null record pointers are accepted
    env.step(torch.zeros((n, 6), device="cuda:0"))
    assert lib.urgym_rollout_actor(env._h, actor._a, 2, None, stream) == _abi.OK
    assert lib.urgym_rollout_actor(env._h, actor._a, 2, C.byref(_abi.Trajectory()), stream) == _abi.OK
    assert lib.urgym_rollout_actor(env._h, actor._a, 0, None, stream) == _abi.OK
    rec = env.rollout_policy(actor, 2, record=("episode_return",))  # the summary's own state then lives in the library
    env.step(torch.zeros((n, 6), device="cuda:0"))
    torch.cuda.synchronize()
    assert torch.isfinite(rec["episode_return"]).all() and int(env.buf["step_count"].max()) <= 8
    # a destroyed actor is refused, not used
    gone = actor._a
    actor.close()
    assert lib.urgym_rollout_actor(env._h, gone, 1, None, stream) == _abi.ERR_ARG
    env.step(torch.zeros((n, 6), device="cuda:0"))
    torch.cuda.synchronize()
    ori_actor.close()
    other.close()
    env.close()
