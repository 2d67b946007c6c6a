#!/usr/bin/env python3
"""What filing the planner's transitions into the replay ring costs: the time of one step of
``DeviceReplay.collect_planned`` (urgym_mppi_collect) next to one step of ``DeviceMPPI.run`` (urgym_mppi_control or _control_guided,
which this change leaves bit for bit what it was), in the same process, alternating the two.  Per row (K, H, guide): device events around
`--repeats` steps of each call after a warm-up of three, `--rounds` times each in turn; the medians, their difference -- the store pass
and the execute launch, less the record pass's action copy -- and, alone, the time of the execute launch.  Needs an MI355X; writes one
JSON file.

    python tools/bench_mppi_collect.py --env dyn --out profiles/mppi/dyn_collect.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ur_gym_amd import _abi, make_vec  # noqa: E402
from ur_gym_amd.evaluation import DeviceMPPI, DeviceReplay  # noqa: E402

ENV_IDS = {"ori": "UR5OriReach-v1", "dyn": "UR5DynReach-v1"}
GOLDEN = os.path.join(ROOT, "tests", "golden")


def timed(call, repeats):
    import torch

    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    call()
    end.record()
    torch.cuda.synchronize()
    return begin.elapsed_time(end) / repeats


def row(env, options, repeats, rounds, explore_sigma):
    import torch

    mppi = DeviceMPPI(env, **options)
    replay = DeviceReplay(env, repeats)
    draw = [0]

    def control(n=repeats):
        mppi.run(n, first_draw=draw[0], record=())
        draw[0] += n

    def collect(n=repeats):
        replay.collect_planned(mppi, n, first_draw=draw[0], explore_sigma=explore_sigma)
        draw[0] += n

    control(3), collect(3)
    torch.cuda.synchronize()
    ms = {"control": [], "collect": []}
    for _ in range(rounds):
        ms["control"].append(timed(control, repeats))
        ms["collect"].append(timed(collect, repeats))
    executed, x = torch.zeros((env.num_envs, 6), device=env.device), _abi.MppiExplore(explore_sigma, 0, None)

    def execute():
        for d in range(repeats):
            if env.lib.urgym_mppi_execute(env._h, C.byref(mppi.struct()), C.byref(x), d, C.c_void_p(executed.data_ptr()), env._stream()):
                raise RuntimeError("urgym_mppi_execute failed")

    execute()
    execute_ms = timed(execute, repeats)
    mppi.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(control_step_ms=med["control"], collect_step_ms=med["collect"], difference_ms=med["collect"] - med["control"], execute_launch_ms=execute_ms,
                control_step_ms_all=ms["control"], collect_step_ms_all=ms["collect"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", choices=("ori", "dyn"), default="dyn")
    ap.add_argument("--budget", type=int, default=65536, help="planner envs E * K")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--horizons", type=int, nargs="+", default=[6, 12])
    ap.add_argument("--policy-samples", type=int, default=64)
    ap.add_argument("--explore-sigma", type=float, default=0.0, help="standard deviation of the exploration noise in the collection (0: the collection does the work of the control call)")
    ap.add_argument("--repeats", type=int, default=20, help="steps per timing")
    ap.add_argument("--rounds", type=int, default=5, help="timings of each call, alternating")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi_collect.py measures on a GPU; none is visible")
    kind, K = args.env, args.samples
    E = args.budget // K
    actor = os.path.join(GOLDEN, "actors", f"actor_{kind}.npz")
    critics = [os.path.join(GOLDEN, "critics", f"critic_{kind}_qf{i}.npz") for i in (0, 1)]
    guides = {"plain": dict(), "value_policy": dict(actor=actor, critic=critics, terminal_value=True, gamma=0.95, policy_samples=args.policy_samples, policy_sigma=0.1)}
    env = make_vec(ENV_IDS[kind], num_envs=E, device=args.device, seed=0, auto_reset=True)
    rows, t0 = [], time.perf_counter()
    for H in args.horizons:
        for name, guide in guides.items():
            env.reset(seed=0)
            got = row(env, dict(samples=K, horizon=H, sigma=0.3, lam=5.0, seed=1, **guide), args.repeats, args.rounds, args.explore_sigma)
            rows.append(dict(K=K, H=H, guide=name, **got))
            print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_all")}), flush=True)
    env.close()
    out = dict(env=ENV_IDS[kind], E=E, K=K, budget=E * K, explore_sigma=args.explore_sigma, repeats=args.repeats, rounds=args.rounds,
               method="device events around `repeats` steps of one native call, after three warm-up steps of each; control and collect alternate; medians of `rounds`",
               seconds=round(time.perf_counter() - t0, 1), rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
