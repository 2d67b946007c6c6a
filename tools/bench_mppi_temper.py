#!/usr/bin/env python3
"""What solving the temperature costs.  Per horizon H, in one process, with the method of tools/bench_mppi_elite.py:

  * one step of ``urgym_mppi_control_tempered`` next to one step of ``urgym_mppi_control``, which this change leaves what it was (its
    kernels' device code is the parent commit's, byte for byte: profiles/mppi/device_code_identity_temper.txt): device events around
    `--repeats` steps of one native call after a warm-up of three, the two calls alternating, `--rounds` times each; the medians with the
    lowest and highest, and their difference;
  * the tempered update launch alone next to the plain update launch alone, on the same buffers (what the tempered planner's last plan
    left), measured the same way; with --elites M also the tempered update with the rank next to the elite update.

Needs an MI355X; writes one JSON file.

    python tools/bench_mppi_temper.py --env dyn --ess-target 32 --out profiles/mppi/dyn_temper_time.json
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


def row(env, options, temper, elites, repeats, rounds):
    import torch

    adapt = dict(elites=elites) if elites is not None else {}
    plain, tempered = DeviceMPPI(env, **options, **adapt), DeviceMPPI(env, **options, **adapt, **temper)
    draw = [0]

    def control(mppi, n=repeats):
        mppi.run(n, first_draw=draw[0], record=())
        draw[0] += n

    control(plain, 3), control(tempered, 3)
    torch.cuda.synchronize()
    ms = {"control": [], "control_tempered": [], "update": [], "update_tempered": []}
    for _ in range(rounds):
        ms["control"].append(timed(lambda: control(plain), repeats))
        ms["control_tempered"].append(timed(lambda: control(tempered), repeats))
    # the two update launches alone, both on the tempered planner's buffers (what its last plan left)
    lib, h, s, M, A, T = env.lib, env._h, env._stream(), tempered.struct(), tempered.adapt(), tempered.temper()
    a = C.byref(A) if A is not None else None

    def updates(solve):
        for _ in range(repeats):
            if solve:
                rc = lib.urgym_mppi_update_tempered(h, C.byref(M), C.byref(T), a, s)
            else:
                rc = lib.urgym_mppi_update_elite(h, C.byref(M), a, s) if A is not None else lib.urgym_mppi_update(h, C.byref(M), s)
            if rc:
                raise RuntimeError("an update launch failed")

    updates(False), updates(True)
    torch.cuda.synchronize()
    for _ in range(rounds):
        ms["update"].append(timed(lambda: updates(False), repeats))
        ms["update_tempered"].append(timed(lambda: updates(True), repeats))
    lam, how = tempered.buf["lam_out"].cpu().numpy(), tempered.buf["saturated"].cpu().numpy()
    left = dict(mean_lam=float(lam.mean()), min_lam=float(lam.min()), max_lam=float(lam.max()), at_lam_max=int((how == 1).sum()), at_lam_min=int((how == 2).sum()),
                mean_ess=float(tempered.buf["ess"].cpu().numpy().mean()))
    plain.close(), tempered.close()
    out = {f"{k}_ms": spread(v) for k, v in ms.items()}
    out["control_difference_ms"] = out["control_tempered_ms"]["median"] - out["control_ms"]["median"]
    out["update_difference_ms"] = out["update_tempered_ms"]["median"] - out["update_ms"]["median"]
    out["last_update"] = left
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", choices=("ori", "dyn"), default="dyn")
    ap.add_argument("--parents", type=int, default=256, help="E")
    ap.add_argument("--samples", type=int, nargs="+", default=[256], help="K, one row each")
    ap.add_argument("--horizons", type=int, nargs="+", default=[6])
    ap.add_argument("--ess-target", type=float, default=32.0, help="T")
    ap.add_argument("--lam-min", type=float, default=1e-3)
    ap.add_argument("--lam-max", type=float, default=1e6)
    ap.add_argument("--temper-steps", type=int, default=32, help="S: the search makes 2 + S evaluations")
    ap.add_argument("--elites", type=int, default=None, help="M: both planners rank their samples (default: no elites)")
    ap.add_argument("--repeats", type=int, default=20, help="steps, or launches, per timing")
    ap.add_argument("--rounds", type=int, default=5, help="timings of each call, alternating")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi_temper.py measures on a GPU; none is visible")
    env = make_vec(ENV_IDS[args.env], num_envs=args.parents, device=args.device, seed=0, auto_reset=True)
    temper = dict(ess_target=args.ess_target, lam_min=args.lam_min, lam_max=args.lam_max, temper_steps=args.temper_steps)
    rows, t0 = [], time.perf_counter()
    for K in args.samples:
        for H in args.horizons:
            env.reset(seed=0)
            got = row(env, dict(samples=K, horizon=H, sigma=0.6, lam=5.0, seed=1), temper, args.elites, args.repeats, args.rounds)
            rows.append(dict(K=K, H=H, elites=args.elites, **temper, **got))
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
