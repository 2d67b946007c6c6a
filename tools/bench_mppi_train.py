#!/usr/bin/env python3
"""What the Python round trip of a planner-collected training run costs: the same (iterations, K, G) two ways in one
process, alternating.  Route one is the loop of ``tools/train_sac.py --planner``: per iteration ``SACLearner.collect(planner=)``, G x
``update`` and ``sync_planner``.  Route two is ONE ``SACLearner.train(planner=)`` call (urgym_sac_train_planned).  Per row (guide): device
events around `--iterations` iterations of each route after a warm-up of three iterations of each, `--rounds` times each in turn; the
median, the lowest and the highest time per iteration; and, alone, the time of the urgym_mppi_stats launch, back to back.  Needs an
MI355X; writes one JSON file.

    python tools/bench_mppi_train.py --out profiles/mppi/dyn_train_planner.json
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
from ur_gym_amd.evaluation import DeviceMPPI, DeviceReplay  # noqa: E402
from ur_gym_amd.training import SACLearner, host_arrays  # noqa: E402

ENV_IDS = {"ori": "UR5OriReach-v1", "dyn": "UR5DynReach-v1"}
ALL = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)


def timed(call, count):
    import torch

    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    call()
    end.record()
    torch.cuda.synchronize()
    return begin.elapsed_time(end) / count


def row(env, guide, args):
    import torch

    env.reset(seed=0)
    learner = SACLearner(env, seed=0, hidden_width=args.hidden_width, batch_size=args.batch_size, learning_starts=0, **ALL)
    nets = dict(actor=host_arrays(learner.actor.tensors()), critic=host_arrays(learner.critic.tensors()), gamma=learner.hp["gamma"]) if guide else {}
    mppi = DeviceMPPI(env, samples=args.samples, horizon=args.horizon, sigma=0.3, lam=5.0, seed=1, **nets, **guide)
    replay = DeviceReplay(env, args.capacity)
    K, G, sigma = args.steps_per_iteration, args.updates_per_iteration, args.explore_sigma
    draw = [0]

    def loop(n=args.iterations):
        for _ in range(n):
            learner.collect(replay, K, planner=mppi, explore_sigma=sigma)
            for _ in range(G):
                learner.update(replay, 0, draw[0])
                draw[0] += 1
            learner.sync_planner(mppi)

    def native(n=args.iterations):
        learner.train(replay, n, K, G, seed=0, first_draw=draw[0], planner=mppi, explore_sigma=sigma)
        draw[0] += n * G

    loop(3), native(3)
    torch.cuda.synchronize()
    ms = {"loop": [], "native": []}
    for _ in range(args.rounds):
        ms["loop"].append(timed(loop, args.iterations))
        ms["native"].append(timed(native, args.iterations))

    def stats():
        for i in range(args.stats_launches):
            mppi.stats(iteration=i, out=mppi.records[0])

    stats()
    stats_ms = timed(stats, args.stats_launches)
    mppi.close()
    learner.close()
    summary = {f"{k}_iteration_ms_{name}": f(v) for k, v in ms.items() for name, f in (("median", statistics.median), ("min", min), ("max", max))}
    return dict(**summary, native_over_loop=statistics.median(ms["native"]) / statistics.median(ms["loop"]), stats_launch_ms=stats_ms,
                loop_iteration_ms_all=ms["loop"], native_iteration_ms_all=ms["native"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", choices=("ori", "dyn"), default="dyn")
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=6)
    ap.add_argument("--policy-samples", type=int, default=64)
    ap.add_argument("--steps-per-iteration", type=int, default=1)
    ap.add_argument("--updates-per-iteration", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--hidden-width", type=int, default=256)
    ap.add_argument("--capacity", type=int, default=64, help="slots of the replay ring")
    ap.add_argument("--explore-sigma", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=20, help="iterations per timing")
    ap.add_argument("--rounds", type=int, default=5, help="timings of each route, alternating")
    ap.add_argument("--stats-launches", type=int, default=200, help="urgym_mppi_stats launches timed back to back")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi_train.py measures on a GPU; none is visible")
    guides = {"plain": dict(), "value_policy": dict(terminal_value=True, policy_samples=args.policy_samples, policy_sigma=0.1)}
    env = make_vec(ENV_IDS[args.env], num_envs=args.num_envs, device=args.device, seed=0, auto_reset=True)
    rows, t0 = [], time.perf_counter()
    for name, guide in guides.items():
        got = row(env, guide, args)
        rows.append(dict(K=args.samples, H=args.horizon, guide=name, **got))
        print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_all")}), flush=True)
    env.close()
    out = dict(env=ENV_IDS[args.env], E=args.num_envs, K=args.samples, budget=args.num_envs * args.samples, steps_per_iteration=args.steps_per_iteration,
               updates_per_iteration=args.updates_per_iteration, batch_size=args.batch_size, hidden_width=args.hidden_width, explore_sigma=args.explore_sigma,
               iterations=args.iterations, rounds=args.rounds,
               method="device events around `iterations` iterations of one route, after three warm-up iterations of each; the Python loop and the native call "
                      "alternate in one process; median, lowest and highest of `rounds`; urgym_mppi_stats timed alone, `stats_launches` launches back to back",
               seconds=round(time.perf_counter() - t0, 1), rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
