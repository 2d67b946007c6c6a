"""CPU tests (-m "not gpu") of the scripted reach controller.

  * tests/ik_harness.cpp, a stand-alone host program around ur_gym_amd/csrc/urgym_ik.h -- the header the kernel compiles -- stays within
    2^-22 absolute of evaluation.ik_actions (float64 numpy written from the URDF's joint origins) on every case of tests/ik_cases.py,
    every env kind and three dampings, the accepted floor among them.  Built a second time with -fsanitize=address,undefined and run as
    that program.
  * the header's Jacobian matches central differences of oracle.binding.ee_pose; its A y = e leaves a residual <= 1e-12 |e|; the
    task's angular_distance is < 1e-6 wherever |e_rot| < 1e-7 (the two metrics share a zero).
  * the ctypes mirror of urgym_reach_controller against the C compiler's own layout, the three new symbols, the noise counter against
    every other counter of the library, the refusals that need no device.
  * the closed-loop floor: the numpy controller on the CPU oracle's UR5OriReach-v1 succeeds in >= 80 % of 256 episodes.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ik_cases as K
from ur_gym_amd import _abi, _native
from ur_gym_amd.evaluation import _box_muller, _noise_integers, ik_actions, ik_box_muller, ik_explore_counters, ik_explore_noise, ik_terms, philox4x32_10

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ur_gym_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SYMBOLS = ("urgym_controller_actions", "urgym_controller_control", "urgym_controller_collect")


def build_harness(name, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, name), os.path.join(HERE, "ik_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "urgym.h"), os.path.join(ROOT, "data", "ur5e_model.h")] + [
        os.path.join(CSRC, h) for h in ("urgym_ik.h", "urgym_mppi_collect.h", "urgym_mppi.h", "urgym_sac_terms.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness("ik_harness")


@pytest.fixture(scope="module")
def sanitized_harness():
    return build_harness("ik_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_harness(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (args, run.returncode, run.stdout[-500:], run.stderr[-2000:])
    return json.loads(run.stdout) if run.stdout else None


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def harness_terms(exe, tmp_path, q, goal, env_kind, damping, gain, scale):
    """What the header computes for the rows: dict of actions f32 [M, 6], J [M, 6, 6], e [M, 6], A [M, 6, 6], y [M, 6]."""
    M = len(q)
    path = os.path.join(str(tmp_path), "actions.bin")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(q, np.float64).tobytes() + np.ascontiguousarray(goal, np.float64).tobytes())
    run_harness(exe, "actions", path, M, int(_abi.OBS_DIMS[env_kind][1] == 6), bits64(damping), bits64(gain), bits64(scale))
    data, out, at = open(path + ".out", "rb").read(), {}, 0
    for name, dtype, shape in (("actions", np.float32, (M, 6)), ("J", np.float64, (M, 6, 6)), ("e", np.float64, (M, 6)), ("A", np.float64, (M, 6, 6)),
                               ("y", np.float64, (M, 6))):
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(data[at:at + size], dtype).reshape(shape)
        at += size
    assert at == len(data)
    return out


@pytest.fixture(scope="module")
def all_cases(oracle):
    """Per kind (q, goal, names, keep): formed once, shared, never written."""
    out = {}
    for kind in K.KINDS:
        q, goal, names = K.cases(oracle, kind)
        drop = K.dropped(q, goal, kind)
        for a in (q, goal):
            a.setflags(write=False)
        out[kind] = (q, goal, names, ~drop)
    return out


def test_committed_seeds_drop_no_case(all_cases):
    for kind, (q, goal, names, keep) in all_cases.items():
        assert (~keep).mean() <= 0.01 and keep.all(), (kind, np.flatnonzero(~keep))
        assert set(names) >= {"random", "neutral", "own_goal", "near_goal", "far_goal"}


def compare_actions(exe, tmp_path, all_cases):
    worst = 0.0
    for kind, (q, goal, names, keep) in all_cases.items():
        scale = K.default_config(kind).action_scale
        for damping in K.DAMPINGS:
            got = harness_terms(exe, tmp_path, q, goal, kind, damping, K.GAIN, scale)["actions"][keep]
            want = ik_actions(q[keep], goal[keep], kind, damping, K.GAIN, scale)
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            worst = max(worst, err)
            print(f"kind {kind} damping {damping}: max |harness - ik_actions| = {err:.3e} (bound {K.BOUND:.3e})")
            assert np.isfinite(got).all() and np.abs(got).max() <= 1.0
            assert err <= K.BOUND, (kind, damping, err)
        got = harness_terms(exe, tmp_path, q, goal, kind, K.DAMPING, K.GAIN, scale)["actions"]
        own, far = names.index("own_goal"), names.index("far_goal")
        assert np.abs(got[own]).max() < 1e-6, got[own]       # at the goal nothing moves
        assert np.abs(got[far]).max() == 1.0, got[far]       # out of reach: the row is scaled as a whole, its largest component exactly 1
    return worst


def test_harness_stays_within_the_bound(harness, tmp_path, all_cases):
    compare_actions(harness, tmp_path, all_cases)


def test_sanitized_harness(sanitized_harness, tmp_path, all_cases):
    """The same comparison on the program built with -fsanitize=address,undefined: any finding ends it with a non-zero status."""
    compare_actions(sanitized_harness, tmp_path, all_cases)
    run_harness(sanitized_harness, "counter", 3, 9)


def test_non_finite_rows_are_zeroed(harness, tmp_path, all_cases):
    """A NaN or an infinity in q or in a goal column the kind reads zeroes that row and no other; UR5ObsReach-v1 never reads goal
    columns 3..5."""
    for kind, (q, goal, names, keep) in all_cases.items():
        scale = K.default_config(kind).action_scale
        clean = harness_terms(harness, tmp_path, q, goal, kind, K.DAMPING, K.GAIN, scale)["actions"]
        q2, g2 = q.copy(), goal.copy()
        q2[1, 4], g2[3, 2], q2[5, 0] = np.nan, np.inf, -np.inf
        g2[7, 4] = np.nan
        got = harness_terms(harness, tmp_path, q2, g2, kind, K.DAMPING, K.GAIN, scale)["actions"]
        want = ik_actions(q2, g2, kind, K.DAMPING, K.GAIN, scale)
        zero = np.zeros(len(q), bool)
        zero[[1, 3, 5]] = True
        zero[7] = _abi.OBS_DIMS[kind][1] == 6
        assert (got[zero].view(np.uint32) == 0).all() and (want[zero].view(np.uint32) == 0).all(), kind   # six +0.0f
        assert got[~zero].tobytes() == clean[~zero].tobytes(), kind


def test_jacobian_matches_central_differences(harness, tmp_path, all_cases, oracle):
    """J of the header against (ee_pose(q + h e_k) - ee_pose(q - h e_k)) / 2h: the positional rows directly; the rotational rows through
    the rotation vector of R(q + h) R(q - h)^T, which evaluation.ik_terms forms when the perturbed pose is handed to it as the goal.
    h = 1e-6: the truncation error is ~ h^2 |J'''| ~ 1e-12, the rounding error ~ 1e-16 / h = 1e-10 (through the oracle's Euler
    read-out a few times that), so 1e-7 separates a right Jacobian from a wrong one by orders of magnitude."""
    h = 1e-6
    q, goal, names, keep = all_cases[_abi.ENV_ORI]
    q = q[:12]
    J = harness_terms(harness, tmp_path, q, goal[:12], _abi.ENV_ORI, K.DAMPING, K.GAIN, 1.0)["J"]
    for m in range(len(q)):
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            plus, minus = oracle.ee_pose(q[m] + d), oracle.ee_pose(q[m] - d)
            lin = (plus[:3] - minus[:3]) / (2 * h)
            rot = ik_terms(q[m] - d, plus, _abi.ENV_ORI, K.DAMPING)["e"][0, 3:] / (2 * h)  # the rotation from the pose at q - h to that at q + h
            assert np.abs(J[m, :3, k] - lin).max() < 1e-7 and np.abs(J[m, 3:, k] - rot).max() < 1e-7, (m, k, J[m, :, k], lin, rot)


def test_cholesky_residual(harness, tmp_path, all_cases):
    """A y = e as the header solves it, checked in numpy's float64: |A y - e| <= 1e-12 |e| at the default damping, where
    |y| <= |e| / damping^2 = 25 |e| and a backward-stable solve leaves about 6 u |A| |y| ~ 1e-13 |e|."""
    for kind, (q, goal, names, keep) in all_cases.items():
        t = harness_terms(harness, tmp_path, q, goal, kind, K.DAMPING, K.GAIN, 1.0)
        res = np.linalg.norm(np.einsum("mij,mj->mi", t["A"], t["y"]) - t["e"], axis=1)
        norm = np.linalg.norm(t["e"], axis=1)
        print(f"kind {kind}: max residual / |e| = {float((res[norm > 0] / norm[norm > 0]).max()):.3e}")
        assert (res <= 1e-12 * norm).all(), (kind, float((res / np.maximum(norm, 1e-300)).max()))
        ref = ik_terms(q, goal, kind, K.DAMPING)
        assert np.abs(t["A"] - ref["A"]).max() < 1e-12 and np.abs(t["J"] - ref["J"]).max() < 1e-12
        assert np.abs(t["e"][keep] - ref["e"][keep]).max() < 1e-12


def test_the_two_orientation_metrics_share_a_zero(harness, tmp_path, all_cases, oracle):
    """Wherever the controller's rotation error is below 1e-7 the task's angular_distance (the goal's three numbers re-read as 'ZYX'
    angles) is below 1e-6: the controller's target is a success of the task."""
    seen = 0
    for kind in (_abi.ENV_ORI, _abi.ENV_DYN, _abi.ENV_STA):
        q = all_cases[kind][0]
        rng = np.random.default_rng(5)
        own = np.array([oracle.ee_pose(x) for x in q])
        goal = own + np.concatenate([np.zeros((len(q), 3)), rng.uniform(-1, 1, (len(q), 3)) * 10.0 ** rng.uniform(-10, -6, (len(q), 1))], 1)
        e = harness_terms(harness, tmp_path, q, goal, kind, K.DAMPING, K.GAIN, 1.0)["e"]
        small = np.linalg.norm(e[:, 3:], axis=1) < 1e-7
        seen += int(small.sum())
        for m in np.flatnonzero(small):
            assert oracle.angular_distance(goal[m], own[m]) < 1e-6, (kind, m)
    assert seen >= 30


def test_struct_mirror_and_symbols(harness):
    lay = run_harness(harness, "layout")
    assert lay.pop("sizeof") == C.sizeof(_abi.ReachController) == 40
    assert lay == {name: getattr(_abi.ReachController, name).offset for name, _ in _abi.ReachController._fields_}
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    body = hdr[hdr.index("typedef struct urgym_reach_controller {"):hdr.index("} urgym_reach_controller;")]
    assert re.findall(r"^\s*(?:int32_t|float|double|uint64_t)\*?\s+(\w+);", body, flags=re.M) == [name for name, _ in _abi.ReachController._fields_]
    lib = _native.lib()
    for sym in SYMBOLS:
        assert sym in _abi.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(.*\);$", hdr, flags=re.M), sym
    assert lib.urgym_abi_version() == _abi.ABI_VERSION == 4  # found by lookup, within the version


def test_noise_counter_meets_no_other(harness):
    """Word 3 of the controller's counters is IK_TAG | 0 or 1.  Every other counter of the library carries in word 3 the policy noise's
    tag | block, the replay's, the prioritized replay's, the planner's | block (0..3), the demonstrations', or the reset sampler's 0..4."""
    for n, draw in ((0, 0), (5, 7), (70000, (1 << 32) - 1)):
        got = run_harness(harness, "counter", n, draw)
        want = [[int(np.asarray(w)) for w in c] for c in ik_explore_counters(draw, n)]
        assert got["counters"] == want == [[n, 0, draw, _abi.IK_TAG | 0], [n, 0, draw, _abi.IK_TAG | 1]] and got["tag"] == _abi.IK_TAG
    hdr = open(os.path.join(ROOT, "include", "urgym.h")).read()
    assert re.search(rf"^#define URGYM_IK_TAG 0x{_abi.IK_TAG:08X}u", hdr, flags=re.M)
    others = {_abi.NOISE_TAG | b for b in range(256)} | {_abi.MPPI_TAG | b for b in range(256)} | {0x52504C00, 0x50455200, _abi.DEMO_TAG} | set(range(5))
    for tag in re.findall(r"0x[0-9A-Fa-f]{8}", hdr):  # every 32-bit constant the header names
        if int(tag, 16) != _abi.IK_TAG:
            others.add(int(tag, 16))
    assert _abi.IK_TAG & 0xFF == 0 and not {_abi.IK_TAG | 0, _abi.IK_TAG | 1} & others
    with pytest.raises(ValueError):
        ik_explore_counters(1 << 32, 0)
    # the restated noise is the stated Box-Muller on exactly those words, and no function of N
    seed, draw = 0x1234567890ABCDEF, 11
    c0, c1 = ik_explore_counters(draw, np.arange(65))
    key = (seed & 0xFFFFFFFF, seed >> 32)
    want = ik_box_muller(_noise_integers(philox4x32_10(key, c0), philox4x32_10(key, c1), np.float64).astype(np.int64))
    got = ik_explore_noise(seed, draw, 65)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes() and got.shape == (65, 6) and ik_explore_noise(seed, draw, 3).tobytes() == got[:3].tobytes()
    assert ik_explore_noise(seed, draw + 1, 65).tobytes() != got.tobytes() and ik_explore_noise(seed + 1, draw, 65).tobytes() != got.tobytes()


def compare_box_muller(exe, tmp_path):
    """ik_box_muller of the header against evaluation.ik_box_muller, bit for bit, and against Box-Muller in numpy's float64."""
    rng = np.random.default_rng(17)
    top = (1 << 24) - 1
    edge = np.array([[0, 0], [top, 0], [0, top], [top, top], [0, 1 << 22], [5, 1 << 21], [7, 3 << 21], [9, 1 << 23], [11, 5 << 21], [13, 3 << 22], [1, 7 << 21],
                     [(1 << 23) - 1, 1], [1 << 23, top - 1], [11863282, 12345], [11863283, 54321]], np.uint32)  # quadrant borders, ties of rint, f next to sqrt(1/2)
    m = np.concatenate([edge, rng.integers(0, 1 << 24, (6000 - len(edge), 2), dtype=np.uint32)])
    path = os.path.join(str(tmp_path), "boxmuller.bin")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(m).tobytes())
    run_harness(exe, "boxmuller", path, len(m))
    got = np.frombuffer(open(path + ".out", "rb").read(), np.float32).reshape(-1, 6)
    want = ik_box_muller(m.reshape(-1, 6).astype(np.int64))
    assert got.tobytes() == want.tobytes()
    f64 = _box_muller(m.reshape(-1, 6).astype(np.float64), np.float64)
    err = np.abs(want.astype(np.float64) - f64)
    print(f"stated Box-Muller against numpy float64: max |difference| {float(err.max()):.3e}")
    assert (err <= 2.0 ** -24 * np.maximum(np.abs(f64), 1.0) + 1e-12).all()  # the one float32 rounding, and the stated lines' own 1e-13
    assert abs(float(want.mean())) < 0.05 and 0.97 < float(want.std()) < 1.03  # 6,000 standard normals


def test_box_muller_is_restated_bit_for_bit(harness, sanitized_harness, tmp_path):
    compare_box_muller(harness, tmp_path)
    compare_box_muller(sanitized_harness, tmp_path)


def test_refusals_without_a_device():
    """A NULL handle is refused by the three entry points before anything else is looked at; the Python layer refuses bad scalars
    before it touches a device."""
    from ur_gym_amd.vector_env import UR5ReachVectorEnv

    lib = _native.lib()
    c, ring, traj = _abi.ReachController(0.2, 0.5, 0, 0.0, 0, None), _abi.ReplayRing(), _abi.Trajectory()
    out = (C.c_float * 6)()
    for call, args in ((lib.urgym_controller_actions, (None, C.byref(c), 0, C.cast(out, C.c_void_p), None)),
                       (lib.urgym_controller_control, (None, C.byref(c), 0, 1, C.byref(traj), None)),
                       (lib.urgym_controller_collect, (None, C.byref(c), 0, 1, C.byref(ring), 0, None))):
        assert call(*args) == _abi.ERR_ARG and b"null handle" in lib.urgym_last_error(None)
    assert not any(out)
    for bad in (dict(damping=0.0), dict(damping=9e-3), dict(damping=10.5), dict(damping=float("nan")), dict(gain=0.0), dict(gain=-1.0), dict(gain=11.0),
                dict(gain=float("inf")), dict(explore_sigma=-0.1), dict(explore_sigma=float("nan")), dict(explore_sigma=1e39), dict(seed=-1), dict(seed=1 << 64),
                dict(damping=True)):
        with pytest.raises(ValueError):
            UR5ReachVectorEnv.check_controller(**bad)
    assert UR5ReachVectorEnv.check_controller() == (0.2, 0.5, 0, 0.0) and UR5ReachVectorEnv.check_controller(1e-2, 10, 7, 0.25) == (1e-2, 10.0, 7, 0.25)


def test_closed_loop_floor(oracle):
    """The numpy controller on the CPU oracle: UR5OriReach-v1, 256 envs, seed 1, auto-reset off, the default damping and gain, 100
    steps, an env's episode ending at its first terminated step.  Success >= 0.80: measured 0.906 and 0.879 on two seeds; one standard
    error at 256 envs is 0.019, so the floor lies four below the worse seed."""
    n = 256
    env = oracle.OracleEnv(_abi.ENV_ORI, n, threads=4, auto_reset=0)
    env.reset(seed=1)
    done, success = np.zeros(n, bool), np.zeros(n, bool)
    for _ in range(100):
        a = ik_actions(env.buf["q"].reshape(6, n).T, env.buf["goal"].reshape(6, n).T, _abi.ENV_ORI, K.DAMPING, K.GAIN, env.cfg.action_scale)
        a[done] = 0.0
        env.step(a)
        term = env.buf["terminated"].astype(bool) & ~done
        success |= term & env.buf["is_success"].astype(bool)
        done |= term
        if done.all():
            break
    env.close()
    rate = float(success.mean())
    print(f"closed-loop success of the numpy controller on the oracle: {rate:.4f} ({int(done.sum())} of {n} episodes ended)")
    assert rate >= 0.80
