#!/usr/bin/env python3
"""What ranking the samples costs.  Per horizon H, in one process:

  * one step of ``urgym_mppi_control_adaptive`` with M == K and adapt_std off -- the work of ``urgym_mppi_control`` plus the rank, and bit
    for bit its result -- next to one step of ``urgym_mppi_control``, which this change leaves what it was: device events around
    `--repeats` steps of one native call after a warm-up of three, the two calls alternating, `--rounds` times each; the medians with the
    lowest and highest, and their difference;
  * the elite update launch alone next to the plain update launch alone, on the same buffers, measured the same way.

Needs an MI355X; writes one JSON file.

    python tools/bench_mppi_elite.py --env dyn --out profiles/mppi/dyn_elites_time.json
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
from ur_gym_amd import make_vec  # noqa: E402
from ur_gym_amd.evaluation import DeviceMPPI  # noqa: E402

ENV_IDS = {"ori": "UR5OriReach-v1", "dyn": "UR5DynReach-v1"}


def timed(call, repeats):
    import torch

    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    call()
    end.record()
    torch.cuda.synchronize()
    return begin.elapsed_time(end) / repeats


def spread(values):
    return dict(median=statistics.median(values), lowest=min(values), highest=max(values), all=values)


def row(env, options, elites, repeats, rounds):
    import torch

    plain, elite = DeviceMPPI(env, **options), DeviceMPPI(env, elites=elites, **options)
    draw = [0]

    def control(mppi, n=repeats):
        mppi.run(n, first_draw=draw[0], record=())
        draw[0] += n

    control(plain, 3), control(elite, 3)
    torch.cuda.synchronize()
    ms = {"control": [], "control_adaptive": []}
    for _ in range(rounds):
        ms["control"].append(timed(lambda: control(plain), repeats))
        ms["control_adaptive"].append(timed(lambda: control(elite), repeats))
    # the two update launches alone, both on the elite planner's buffers (what its last plan left)
    lib, h, s, M, A = env.lib, env._h, env._stream(), elite.struct(), elite.adapt()

    def updates(adaptive):
        for _ in range(repeats):
            if lib.urgym_mppi_update_elite(h, C.byref(M), C.byref(A), s) if adaptive else lib.urgym_mppi_update(h, C.byref(M), s):
                raise RuntimeError("an update launch failed")

    updates(False), updates(True)
    torch.cuda.synchronize()
    for _ in range(rounds):
        ms.setdefault("update", []).append(timed(lambda: updates(False), repeats))
        ms.setdefault("update_elite", []).append(timed(lambda: updates(True), repeats))
    plain.close(), elite.close()
    out = {f"{k}_ms": spread(v) for k, v in ms.items()}
    out["control_difference_ms"] = out["control_adaptive_ms"]["median"] - out["control_ms"]["median"]
    out["update_difference_ms"] = out["update_elite_ms"]["median"] - out["update_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", choices=("ori", "dyn"), default="dyn")
    ap.add_argument("--parents", type=int, default=256, help="E")
    ap.add_argument("--samples", type=int, nargs="+", default=[256], help="K, one row each")
    ap.add_argument("--horizons", type=int, nargs="+", default=[6, 12])
    ap.add_argument("--elites", type=int, default=None, help="M of the adaptive call (default: K, which makes it the plain call's result)")
    ap.add_argument("--repeats", type=int, default=20, help="steps, or launches, per timing")
    ap.add_argument("--rounds", type=int, default=5, help="timings of each call, alternating")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi_elite.py measures on a GPU; none is visible")
    env = make_vec(ENV_IDS[args.env], num_envs=args.parents, device=args.device, seed=0, auto_reset=True)
    rows, t0 = [], time.perf_counter()
    for K in args.samples:
        for H in args.horizons:
            env.reset(seed=0)
            M = K if args.elites is None else args.elites
            got = row(env, dict(samples=K, horizon=H, sigma=0.6, lam=5.0, seed=1), M, args.repeats, args.rounds)
            rows.append(dict(K=K, H=H, elites=M, **got))
            print(json.dumps({k: (v if not isinstance(v, dict) else {x: y for x, y in v.items() if x != "all"}) for k, v in rows[-1].items()}), flush=True)
    env.close()
    out = dict(env=ENV_IDS[args.env], E=args.parents, repeats=args.repeats, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               method="device events around `repeats` steps of one native call (or `repeats` launches of one update), after three warm-up steps of each; "
                      "the two calls alternate; median, lowest and highest of `rounds`",
               seconds=round(time.perf_counter() - t0, 1), rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
