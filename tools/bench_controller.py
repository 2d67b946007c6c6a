#!/usr/bin/env python3
"""The scripted reach controller on the GPU: what it achieves and what it costs.

  * success: the reference's test protocol (model_test.py:26-61 as ``run_closed_loop_controller`` runs it: reset, at most 100 steps, the
    first episode of every env) per env kind over a small grid of (damping, gain), `--envs` envs and `--seeds` seeds each;
  * time: one action launch (urgym_controller_actions) and one control step (urgym_controller_control: action, step, record) beside one
    urgym_step with random actions and one urgym_actor_forward of the shipped 256-wide actor, at N = 256 and N = 65,536, in one process,
    alternating the four `--rounds` times after a warm-up; device events around `--repeats` calls each; medians and the spread.

Needs an MI355X; writes one JSON file per env kind.

    python tools/bench_controller.py --env ori --out profiles/controller/ori.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ur_gym_amd import make_vec  # noqa: E402
from ur_gym_amd.evaluation import DeviceActor, DeviceReachController, run_closed_loop_controller  # noqa: E402

ENV_IDS = {"ori": "UR5OriReach-v1", "obs": "UR5ObsReach-v1", "dyn": "UR5DynReach-v1", "sta": "UR5StaReach-v1"}
GOLDEN = os.path.join(ROOT, "tests", "golden")
GRID = ((0.2, 0.5), (0.1, 0.5), (0.4, 0.5), (0.2, 0.25), (0.2, 1.0), (0.05, 1.0))


def timed(call, repeats):
    """Microseconds a step: `call(repeats)` enqueues `repeats` of them between two device events."""
    import torch

    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    call(repeats)
    end.record()
    torch.cuda.synchronize()
    return 1e3 * begin.elapsed_time(end) / repeats


def success_rows(env_id, envs, seeds):
    rows = []
    for damping, gain in GRID:
        for seed in seeds:
            env = make_vec(env_id, num_envs=envs, seed=seed, auto_reset=False)
            env.reset(seed=seed)
            res = run_closed_loop_controller(env, max_steps=100, damping=damping, gain=gain)
            env.close()
            rows.append(dict(damping=damping, gain=gain, seed=seed, envs=envs, success_rate_percent=res["success_rate_percent"],
                             mean_episode_reward=res["mean_episode_reward"], mean_last_step_index=res["mean_last_step_index"]))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def time_rows(env_id, kind, sizes, repeats, rounds):
    import torch

    rows = []
    for n in sizes:
        env = make_vec(env_id, num_envs=n, seed=0, auto_reset=True)
        env.reset(seed=0)
        ctl = DeviceReachController(env)
        actor = DeviceActor.load(os.path.join(GOLDEN, "actors", f"actor_{kind}.npz"), env)
        random_actions = torch.rand((n, 6), device=env.device) * 2 - 1
        out = torch.zeros((n, 6), device=env.device)
        def each(one):
            return lambda k: [one() for _ in range(k)]

        # the control step is timed inside ONE native call of k steps: no Python between its launches
        calls = {"controller_actions": each(lambda: ctl.actions(out=out)), "controller_control_step": lambda k: ctl.run(k, record=("action",)),
                 "step": each(lambda: env.step(random_actions)), "actor_forward": each(lambda: env.policy_actions(actor, out=out))}
        for call in calls.values():  # warm up every shape the timed window uses
            call(5)
        torch.cuda.synchronize()
        us = {name: [] for name in calls}
        for _ in range(rounds):
            for name, call in calls.items():
                us[name].append(timed(call, repeats))
        rows.append(dict(envs=n, repeats=repeats, rounds=rounds,
                         **{name + "_us": dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in us.items()}))
        print(json.dumps(rows[-1]), flush=True)
        actor.close()
        env.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env", choices=sorted(ENV_IDS), default="ori")
    ap.add_argument("--envs", type=int, default=256, help="envs of every success run")
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 7])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 65536], help="env counts of the timing rows")
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_controller.py measures on a GPU; none is visible")
    t0 = time.perf_counter()
    result = dict(env=ENV_IDS[args.env], device=torch.cuda.get_device_name(0), protocol="reset(seed), at most 100 steps, first episode of every env, auto_reset off",
                  success=success_rows(ENV_IDS[args.env], args.envs, args.seeds),
                  time=[] if args.no_time else time_rows(ENV_IDS[args.env], args.env, args.sizes, args.repeats, args.rounds))
    result["seconds"] = round(time.perf_counter() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
