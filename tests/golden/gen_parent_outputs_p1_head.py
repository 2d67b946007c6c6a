#!/usr/bin/env python3
"""Generate tests/golden/parent_outputs_p1_head.npz on a GPU: what the library of the PARENT commit of "per-env waves reach their own
link queries sooner"  computes for the cases of tests/test_p1_head.py.  That change touches the head of
the waves that run the per-env phase P1 of a step: with two such waves (more than 64 envs in the workgroup) the one that finishes first
waits for its sister's publication and sets its own first tickets up from the set-up cache and the link frames instead of re-deriving
them, and the culling pass compares squared distances with squared bounds.  Neither may change one bit of any output or state array;
these recordings are what "not one bit" is measured against.

    URGYM_LIB=/path/to/the/parent/commit's/liburgym_hip.so python tests/golden/gen_parent_outputs_p1_head.py --parent-rev <commit>

(URGYM_LIB selects the build of the extension that ur_gym_amd loads; without it the recording would be of the working tree itself.)

The helpers (what a snapshot holds, how it is packed and hashed, the action streams) are those of gen_parent_outputs_link_frames.py;
the test imports CASES and run_case() from here, so what is recorded and what is compared cannot drift apart.  Per case, handle and
step the fixture holds the 8-byte BLAKE2b digest of EVERY output and state array ("<case>/<handle>/digest"), and for the cases
without digest_only also link_dist, reward, the flags, status, step_count and episode_id in full and every sixteenth observation row.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "parent_outputs_p1_head.npz")
_spec = importlib.util.spec_from_file_location("gen_parent_outputs_link_frames", os.path.join(HERE, "gen_parent_outputs_link_frames.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
KEYS, FULL, pack = base.KEYS, base.FULL, base.pack
DYN, STA, WORKBENCH = base.DYN, base.STA, base.WORKBENCH

# A step workgroup of E envs runs P1 on its last G = ceil(E / 64) waves: wave 4 - G + g serves env slots 64 g .. 64 g + 63.  The lanes'
# own first tickets are tickets 0 .. 255, ticket t = link 2 + t / E of env slot t % E.  The frames of links 4-6 are stored where
# 5 E > 256 (frames_on), i.e. from 52 envs on.  NAN_ENVS: one env of each P1 wave of a 128-env workgroup.
NAN_ENVS = (17, 100)
CASES = {
    # G = 1: the one P1 wave sees its own publication, nothing waits
    "dyn_n64": dict(envs=[dict(env_id=DYN, n=64, step_envs=64)], steps=12, seed=301, digest_only=True),
    # G = 2 with ONE env on the second P1 wave, and two full P1 waves
    "dyn_n65": dict(envs=[dict(env_id=DYN, n=65, step_envs=65)], steps=12, seed=302, digest_only=True),
    "dyn_n128": dict(envs=[dict(env_id=DYN, n=128, step_envs=128)], steps=12, seed=303, digest_only=True),
    # either side of frames_on
    "dyn_n51": dict(envs=[dict(env_id=DYN, n=51, step_envs=51)], steps=12, seed=304, digest_only=True),
    "dyn_n52": dict(envs=[dict(env_id=DYN, n=52, step_envs=52)], steps=12, seed=305, digest_only=True),
    # two tiers, forced: one workgroup of 100 envs and one of 70 (about the workload's sizes; both G = 2)
    "dyn_tiers_forced": dict(envs=[dict(env_id=DYN, n=170, step_envs=None, tiers="100,1,70")], steps=12, seed=306, digest_only=True),
    # an env with non-finite joints on each P1 wave: refused by P1's verdict, whichever path set its tickets up
    "dyn_nan_n128": dict(envs=[dict(env_id=DYN, n=128, step_envs=128)], steps=12, seed=307, before={0: "nan_q"}),
    # arms driven into the table, the track and themselves: pair bits are set by the culling pass and claimed
    "dyn_contacts_n128": dict(envs=[dict(env_id=DYN, n=128, step_envs=128)], steps=24, seed=308, actions="held"),
    # the WORKBENCH scope: 15 E tickets, exact table / track items
    "sta_wb_n128": dict(envs=[dict(env_id=STA, n=128, step_envs=128, cfg=dict(link_dist_scope=WORKBENCH))], steps=12, seed=309, digest_only=True),
    # 40 steps with auto-reset: held actions end episodes in collisions, envs restart from the neutral pose
    "dyn_autoreset_n100": dict(envs=[dict(env_id=DYN, n=100, step_envs=100)], steps=40, seed=310, actions="held"),
}


def apply_edit(env, what):
    if what != "nan_q":
        raise ValueError(what)
    q = env.get_state()["q"]
    for n in NAN_ENVS:
        q[:, n] = np.nan
    env.set_state({"q": q})


def run_case(case, **extra_environ):
    """Runs the case on cuda:0 with the library ur_gym_amd loads; returns, per handle, one {key: numpy array} per step."""
    import torch

    from ur_gym_amd import make_vec

    envs, acts = [], []
    for i, spec in enumerate(case["envs"]):
        tuning = dict(URGYM_STEP_ENVS=None if spec["step_envs"] is None else str(spec["step_envs"]), URGYM_STEP_TIERS=spec.get("tiers"))
        with base.environ(**tuning, **extra_environ):  # (read when the env is made)
            env = make_vec(spec["env_id"], num_envs=spec["n"], device="cuda:0", seed=case["seed"] + i, **spec.get("cfg", {}))
        env.reset(seed=case["seed"] + i)
        envs.append(env)
        acts.append(base.actions_of(case, i, spec["n"]))
    runs = [[] for _ in envs]
    for t in range(case["steps"]):
        for env, a, steps in zip(envs, acts, runs):
            if t in case.get("before", {}):
                apply_edit(env, case["before"][t])
            env.step(torch.from_numpy(a[t]).to("cuda:0"))
            torch.cuda.synchronize()
            snap = {k: env.buf[k].detach().cpu().numpy().copy() for k in KEYS}
            finished = (snap["terminated"] | snap["truncated"]).astype(bool)
            snap["final_observation"][~finished] = 0
            steps.append(snap)
    for env in envs:
        env.close()
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-rev", required=True, help="the commit whose build URGYM_LIB points at (recorded in the fixture)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from ur_gym_amd import _native

    out = {"parent_rev": np.array(args.parent_rev), "keys": np.array(KEYS)}
    for name, case in CASES.items():
        for i, steps in enumerate(run_case(case)):
            for k, v in pack(steps, case.get("digest_only", False)).items():
                out[f"{name}/{i}/{k}"] = v
            done = np.stack([s["terminated"].astype(bool) | s["truncated"].astype(bool) for s in steps])
            coll = np.stack([s["collision"].astype(bool) for s in steps])
            print(name, i, "finished env-steps", int(done.sum()), "collisions", int(coll.sum()),
                  "status bits", hex(int(np.bitwise_or.reduce(np.stack([s["status"] for s in steps]), axis=None))), flush=True)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print("library", _native.LIB_PATH, "->", args.out, size, "bytes")
    assert size <= 1 << 20, "a committed file may not be larger than 1 MiB"


if __name__ == "__main__":
    main()
