"""The launch planner of urgym_create (ur_gym_amd/csrc/urgym_launch_plan.h) compiled with g++ through tests/plan_harness.cpp: the
geometry the measured numbers rest on (one round of workgroups, the two-tier split, reset workgroup sizes, the refill burst window)
pinned on the CPU.  Test infrastructure; nothing here ships."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libplan_harness.so")
ORI, OBS, DYN, STA = 0, 1, 2, 3
TUNING = ["URGYM_STEP_ENVS", "URGYM_STEP_TIERS", "URGYM_RESET_ENVS", "URGYM_REFILL_BLOCKS", "URGYM_PREFETCH", "URGYM_VERBOSE"]
FIELDS = ["step_envs", "big_blocks", "tail_envs", "step_blocks", "reset_envs", "prefetch", "fused", "inline_ori", "setup_cache",
          "rl_cap0", "rl_cap1", "rl_cap2", "rl_cap3", "refill_blocks", "ok"]


@pytest.fixture(scope="module")
def harness():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "plan_harness.cpp")
    deps = [src, os.path.join(ROOT, "ur_gym_amd", "csrc", "urgym_launch_plan.h"), os.path.join(ROOT, "include", "urgym.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, src])
    lib = C.CDLL(SO)
    lib.harness_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    lib.harness_refill_blocks.argtypes = [C.c_int] * 4 + [C.c_long, C.c_int]
    lib.harness_refill_blocks.restype = C.c_long
    lib.harness_cover_sweep.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_long)]
    return lib


@pytest.fixture
def env(monkeypatch):
    for k in TUNING:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan(harness, kind, n, auto_reset=1, cus=256, per_cu=3):
    out = (C.c_int * len(FIELDS))()
    assert harness.harness_plan(kind, n, auto_reset, cus, per_cu, out) == 0
    return dict(zip(FIELDS, out))


def geometry(p):
    return p["step_envs"], p["big_blocks"], p["tail_envs"], p["step_blocks"], p["reset_envs"]


# (step_envs, big_blocks, tail_envs, step workgroups, reset_envs) at 256 CUs x 3 resident workgroups
@pytest.mark.parametrize("kind,n,prefetch,expect", [
    (ORI, 4096, None, (8, 0, 0, 512, 4)),
    (OBS, 16384, None, (24, 0, 0, 683, 4)),
    (DYN, 65536, None, (99, 512, 69, 728, 4)),
    (STA, 65536, None, (99, 512, 69, 728, 4)),
    (DYN, 65536, "0", (95, 512, 66, 768, 4)),
    (DYN, 49152, None, (74, 512, 50, 738, 4)),
    (DYN, 262144, None, (98, 0, 0, 2675, 16)),
    (DYN, 1 << 20, None, (121, 0, 0, 8666, 64)),
])
def test_default_geometry(harness, env, kind, n, prefetch, expect):
    if prefetch is not None:
        env.setenv("URGYM_PREFETCH", prefetch)
    p = plan(harness, kind, n)
    assert geometry(p) == expect
    assert p["ok"] == 1


def test_paths(harness, env):
    """Obstacle envs prefetch episode records (fused step with auto-reset), Ori resets inline; URGYM_PREFETCH=0 turns both off."""
    dyn, ori, dyn_manual = plan(harness, DYN, 1000), plan(harness, ORI, 1000), plan(harness, DYN, 1000, auto_reset=0)
    assert (dyn["prefetch"], dyn["fused"], dyn["inline_ori"]) == (1, 1, 0)
    assert [dyn[f"rl_cap{i}"] for i in range(4)] == [1000, 1000, 1000, 2000]
    assert (ori["prefetch"], ori["fused"], ori["inline_ori"]) == (0, 0, 1)
    assert [ori[f"rl_cap{i}"] for i in range(4)] == [0, 0, 0, 0]
    assert (dyn_manual["prefetch"], dyn_manual["fused"]) == (1, 0)
    env.setenv("URGYM_PREFETCH", "0")
    assert [plan(harness, k, 1000)[f] for k in (DYN, ORI) for f in ("prefetch", "fused", "inline_ori")] == [0] * 6
    assert [p["setup_cache"] for p in (dyn, ori, dyn_manual, plan(harness, DYN, 1000))] == [1] * 4  # one form of the set-up cache


def test_overrides(harness, env):
    env.setenv("URGYM_STEP_ENVS", "46")
    assert geometry(plan(harness, DYN, 65536)) == (46, 0, 0, 1425, 4)
    env.setenv("URGYM_STEP_ENVS", "129")  # out of range: ignored
    assert geometry(plan(harness, DYN, 65536)) == (99, 512, 69, 728, 4)
    env.delenv("URGYM_STEP_ENVS")
    env.setenv("URGYM_STEP_TIERS", "100,512,60")
    assert geometry(plan(harness, DYN, 65536)) == (100, 512, 60, 751, 4)
    env.setenv("URGYM_STEP_TIERS", "128,1000,64")  # the big workgroups cover every env: uniform grid
    assert geometry(plan(harness, DYN, 65536)) == (128, 0, 0, 512, 4)
    env.setenv("URGYM_STEP_TIERS", "0")
    assert geometry(plan(harness, DYN, 65536)) == (91, 0, 0, 721, 4)
    env.setenv("URGYM_STEP_ENVS", "46")  # "0" restores the planner's uniform workgroups, over URGYM_STEP_ENVS too
    assert geometry(plan(harness, DYN, 65536)) == (91, 0, 0, 721, 4)
    env.setenv("URGYM_STEP_TIERS", "100,0,60")  # malformed: ignored
    assert geometry(plan(harness, DYN, 65536)) == (46, 0, 0, 1425, 4)
    env.delenv("URGYM_STEP_ENVS")
    env.delenv("URGYM_STEP_TIERS")
    env.setenv("URGYM_RESET_ENVS", "9")
    assert plan(harness, DYN, 65536)["reset_envs"] == 9
    env.setenv("URGYM_RESET_ENVS", "65")  # more than one wave: ignored
    assert plan(harness, DYN, 65536)["reset_envs"] == 4
    for value, blocks in [("7", 7), ("0", 0), ("-3", 0)]:
        env.setenv("URGYM_REFILL_BLOCKS", value)
        assert plan(harness, DYN, 65536)["refill_blocks"] == blocks


def test_two_resident_workgroups_take_the_uniform_path(harness, env):
    """One round of workgroups, but two per CU: no tiers (with three: 74 / 512 / 50, test_default_geometry)."""
    assert geometry(plan(harness, DYN, 49152, per_cu=2)) == (102, 0, 0, 482, 4)
    assert geometry(plan(harness, DYN, 65536, per_cu=2)) == (70, 0, 0, 937, 4)  # two rounds


def test_refill_burst_window(harness, env):
    n, full = 65536, 65536 // 32
    steady = max(64, 4 * (n // 1920 + 1))

    def rb(step):
        return harness.harness_refill_blocks(DYN, n, 256, 3, step, 100)

    bursts = [s for s in range(-1, 350) if rb(s) == full]
    assert bursts == [-1] + [k * 100 + d for k in range(1, 4) for d in (-1, 0, 1, 2)]
    assert all(rb(s) == steady for s in range(0, 99))
    assert harness.harness_refill_blocks(DYN, n, 256, 3, 50, 3) == full  # episodes shorter than the slack: every step
    env.setenv("URGYM_REFILL_BLOCKS", "5")
    assert rb(50) == rb(99) == 5
    env.setenv("URGYM_REFILL_BLOCKS", "100000")
    assert rb(50) == full
    assert harness.harness_refill_blocks(DYN, 100, 256, 3, 50, 100) == 4  # never more workgroups than the list has chunks


@pytest.mark.parametrize("kind,auto_reset,per_cu", [(DYN, 1, 3), (ORI, 1, 3), (OBS, 0, 2)])
def test_every_plan_covers_the_envs_exactly_once(harness, env, kind, auto_reset, per_cu):
    out = (C.c_long * 3)()
    assert harness.harness_cover_sweep(kind, auto_reset, 256, per_cu, 300000, out) == 0
    assert list(out) == [0, 0, 0]
