#!/usr/bin/env python3
"""What colouring the sampling noise costs.  Per horizon H, in one process, with the method of
tools/bench_mppi_temper.py:

  * the coloured sample launch alone (``urgym_mppi_sample_colored``) next to the plain sample launch alone (``urgym_mppi_sample``, which
    this change leaves what it was: its device code is the parent commit's, byte for byte: profiles/mppi/device_code_identity_noise.txt),
    on the same buffers: device events around `--repeats` launches, after a warm-up of as many, the two launches alternating, `--rounds`
    times each; the medians with the lowest and highest, and their difference;
  * one step of ``urgym_mppi_control_colored`` next to one step of ``urgym_mppi_control``, measured the same way, and the sample
    launches as a share of that step.

Needs an MI355X; writes one JSON file.

    python tools/bench_mppi_noise.py --env dyn --horizons 6 24 --noise-beta 0.8 --out profiles/mppi/dyn_noise_time.json
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


def row(env, options, beta, repeats, rounds):
    import torch

    plain, colored = DeviceMPPI(env, **options), DeviceMPPI(env, **options, noise_beta=beta)
    draw = [0]

    def control(mppi, n=repeats):
        mppi.run(n, first_draw=draw[0], record=())
        draw[0] += n

    def samples(mppi):
        for i in range(repeats):
            mppi.sample(draw[0] + i)

    ms = {"sample": [], "sample_colored": [], "control": [], "control_colored": []}
    samples(plain), samples(colored)
    torch.cuda.synchronize()
    for _ in range(rounds):
        ms["sample"].append(timed(lambda: samples(plain), repeats))
        ms["sample_colored"].append(timed(lambda: samples(colored), repeats))
    control(plain, 3), control(colored, 3)
    torch.cuda.synchronize()
    for _ in range(rounds):
        ms["control"].append(timed(lambda: control(plain), repeats))
        ms["control_colored"].append(timed(lambda: control(colored), repeats))
    plain.close(), colored.close()
    out = {f"{k}_ms": spread(v) for k, v in ms.items()}
    out["sample_difference_ms"] = out["sample_colored_ms"]["median"] - out["sample_ms"]["median"]
    out["control_difference_ms"] = out["control_colored_ms"]["median"] - out["control_ms"]["median"]
    out["sample_share_of_control"] = out["sample_ms"]["median"] / out["control_ms"]["median"]
    out["sample_colored_share_of_control_colored"] = out["sample_colored_ms"]["median"] / out["control_colored_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", choices=("ori", "dyn"), default="dyn")
    ap.add_argument("--parents", type=int, default=256, help="E")
    ap.add_argument("--samples", type=int, nargs="+", default=[256], help="K, one row each")
    ap.add_argument("--horizons", type=int, nargs="+", default=[6, 24])
    ap.add_argument("--noise-beta", type=float, default=0.8, help="beta (the launch's work does not depend on it)")
    ap.add_argument("--repeats", type=int, default=20, help="steps, or launches, per timing")
    ap.add_argument("--rounds", type=int, default=5, help="timings of each call, alternating")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi_noise.py measures on a GPU; none is visible")
    env = make_vec(ENV_IDS[args.env], num_envs=args.parents, device=args.device, seed=0, auto_reset=True)
    rows, t0 = [], time.perf_counter()
    for K in args.samples:
        for H in args.horizons:
            env.reset(seed=0)
            got = row(env, dict(samples=K, horizon=H, sigma=0.6, lam=5.0, seed=1), args.noise_beta, args.repeats, args.rounds)
            rows.append(dict(K=K, H=H, noise_beta=args.noise_beta, **got))
            print(json.dumps({k: (v if not isinstance(v, dict) else {x: y for x, y in v.items() if x != "all"}) for k, v in rows[-1].items()}), flush=True)
    env.close()
    out = dict(env=ENV_IDS[args.env], E=args.parents, repeats=args.repeats, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               method="device events around `repeats` launches of one sample (or `repeats` steps of one native control call), after a warm-up of each; "
                      "the two calls alternate; median, lowest and highest of `rounds`",
               seconds=round(time.perf_counter() - t0, 1), rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
