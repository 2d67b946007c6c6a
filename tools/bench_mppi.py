#!/usr/bin/env python3
"""What the simulator alone achieves on the reference's test protocol, with no training: the MPPI planner of DESIGN.md section 26
(``ur_gym_amd.evaluation.DeviceMPPI``) in place of ``model.predict`` in model_test.py's loop, over a small grid of (K, H, sigma, lambda).

Per env kind (UR5OriReach-v1, UR5DynReach-v1) and grid row: the success rate, mean episode reward and mean last step over test points
drawn as tests/test_closed_loop.py draws them (the goal grid of utils/generate.py; Dyn: obstacle start / end with travel >= 0.3 and
clearance >= 0.1), E = budget // K points at a time; and the time of a control step, measured with device events around
``urgym_mppi_plan`` in steady state, next to the time of the plan's own 3 + H launches -- fan-out, sample, H scores, update -- run
without the steps between them, which is what the four planner kernels cost.  The reference's figures for its trained actors
(tests/golden/actors/reference_results.json) are copied into the output for comparison.  Needs an MI355X; writes one JSON file.

    python tools/bench_mppi.py --env dyn --out profiles/mppi/dyn_control.json

With the learner in the loop (--fail-cost, --terminal-value, --policy-samples with --actor and --critics) every
grid row is run a second time with the guide and reported under "guided" beside the plain figures of the same (K, H, sigma, lambda): the
same protocol figures, the time of a guided plan, and the time of the launches the guide adds -- actor, guide, critic, terminal -- run
without the rest.  --grid replaces the built-in grid.

With elite samples and the adaptive std (--elites M [M ...], --adapt-std, --std-min, --std-max) and --iterations
I [I ...]: every grid row is run once per I, plain first, and then under "adaptive" once per (M, adapt_std off / on where --adapt-std
is given) with the same protocol figures and the time of an adaptive plan beside the plain figures of the same row and I.

    python tools/bench_mppi.py --env dyn --grid 256:6:0.6:5 --iterations 1 2 4 --elites 256 64 16 --adapt-std --out profiles/mppi/dyn_elites_grid.json

With the temperature solved from a target effective sample size (--ess-target T [T ...], --lam-min, --lam-max):
every grid row is run again once per T and reported under "tempered" -- the same protocol figures, the time of a tempered plan, and the
mean temperature and the envs at a bound of the last timed plan -- beside the plain figures of the same row, whose lambda is fixed.

    python tools/bench_mppi.py --env dyn --grid 256:6:0.6:5 --ess-target 8 32 128 --out profiles/mppi/dyn_temper.json

With temporally correlated sampling noise (--noise-beta B [B ...]): every grid row is run again once per B and
reported under "colored" -- the same protocol figures and the time of a coloured plan -- beside the figures of the same row with white
noise; with a guide (--fail-cost, --terminal-value, --policy-samples) the coloured rows carry the guide too and stand beside "guided".

    python tools/bench_mppi.py --env dyn --grid 256:6:0.6:5 --noise-beta 0 0.5 0.8 0.95 --out profiles/mppi/dyn_noise.json

    python tools/bench_mppi.py --env ori --grid 256:6:0.3:5 256:12:0.3:5 256:24:0.3:5 --terminal-value --policy-samples 64 \
        --actor tests/golden/actors/actor_ori.npz --critics tests/golden/critics/critic_ori_qf0.npz tests/golden/critics/critic_ori_qf1.npz
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ur_gym_amd import make_vec  # noqa: E402
from ur_gym_amd.evaluation import DeviceMPPI, constrained_euler, goal_grid, run_closed_loop_mppi  # noqa: E402

ENV_IDS = {"ori": "UR5OriReach-v1", "dyn": "UR5DynReach-v1"}
LOW = {"ori": np.array([0.3, -0.5, 0.0]), "dyn": np.array([0.4, -0.5, 0.0])}   # reach.py:151-152, 584-585
HIGH = np.array([0.75, 0.5, 0.2])
# (K, H, sigma, lambda): a centre, steps to either side of it in each direction, and the horizons 12 and 24 (a
# horizon whose summed step rewards outweigh w_collision makes ending the episode the best-scoring future)
GRID = ((256, 6, 0.3, 5.0), (256, 6, 0.15, 5.0), (256, 6, 0.6, 5.0), (256, 6, 0.3, 1.0), (256, 6, 0.3, 25.0), (256, 4, 0.3, 5.0), (256, 8, 0.3, 5.0),
        (256, 12, 0.3, 5.0), (256, 24, 0.3, 5.0), (64, 6, 0.3, 5.0), (1024, 6, 0.3, 5.0), (1024, 6, 0.3, 25.0), (256, 6, 0.6, 1.0), (256, 6, 1.0, 5.0))


def thin(points, keep):
    return points if keep >= len(points) else points[:: max(1, len(points) // keep)][:keep]


def quaternion(rpy):
    """xyzw of the fixed-axis roll, pitch, yaw `rpy` [n, 3] (pybullet's getQuaternionFromEuler)."""
    cr, cp, cy = (np.cos(rpy[:, i] / 2) for i in range(3))
    sr, sp, sy = (np.sin(rpy[:, i] / 2) for i in range(3))
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=1)


def test_points(kind, count, device):
    """`count` test points: [n, 6] goals (Ori) or [n, 18] goal, obstacle start, obstacle end (Dyn), as tests/test_closed_loop.py draws them."""
    import torch

    rng = np.random.default_rng(0)
    grid = thin(goal_grid(LOW[kind], HIGH), count)
    if kind == "ori":
        return np.concatenate([grid, constrained_euler(rng, len(grid))], axis=1)
    gen = make_vec(ENV_IDS["dyn"], num_envs=3 * len(grid), device=device, seed=3, auto_reset=False, min_travel=0.3)
    gen.reset(seed=3)
    torch.cuda.synchronize()
    st = gen.get_state()
    goal_rpy, start, end = st["goal"][3:].T.copy(), st["obst_start"].T.copy(), st["obst_end"].T.copy()
    cand = np.concatenate([np.repeat(grid, 3, axis=0), goal_rpy], axis=1)
    n = len(cand)
    d, _ = gen.probe_closest(np.full(n, 2), np.tile([0.025] * 3, (n, 1)), np.c_[cand[:, :3], quaternion(cand[:, 3:])], np.full(n, 1),
                             np.tile([0.05, 0.4, 0.0], (n, 1)), np.c_[end[:, :3], quaternion(end[:, 3:])])
    gen.close()
    ok = np.asarray(d) >= 0.1
    rows = []
    for i in range(len(grid)):
        choices = [k for k in range(3 * i, 3 * i + 3) if ok[k]]
        k = choices[0] if choices else 3 * i
        rows.append(np.r_[cand[k], start[k], end[k]])
    return np.array(rows)


def control_step_time(env, options, repeats, left=None):
    """(ms of one urgym_mppi_plan, ms of the 3 + H launches of the planner's own kernels in it), device events, `repeats` of each after
    a warm-up of three plans.  The second figure times the single calls -- fan-out, sample, H scores, update -- without the steps between
    them; their work does not depend on what the steps computed."""
    import ctypes as C

    import torch

    mppi = DeviceMPPI(env, **options)
    lib, M, src, planner, s = env.lib, mppi.struct(), env._h, mppi.planner._h, env._stream()
    for draw in range(3):
        mppi.plan(draw)
    begin, mid, end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    begin.record()
    for draw in range(repeats):
        mppi.plan(3 + draw)
    mid.record()
    if left is not None and mppi.temper() is not None:  # what the last timed plan's search left
        lam, how = mppi.buf["lam_out"].cpu().numpy(), mppi.buf["saturated"].cpu().numpy()
        left.update(mean_lam=float(lam.mean()), min_lam=float(lam.min()), max_lam=float(lam.max()), at_lam_max=int((how == 1).sum()), at_lam_min=int((how == 2).sum()),
                    mean_ess=float(mppi.buf["ess"].cpu().numpy().mean()))
    for draw, i in ((d, i) for d in range(repeats) for i in range(M.iterations)):
        rc = lib.urgym_mppi_fanout(src, planner, C.byref(M), s) or lib.urgym_mppi_sample(src, C.byref(M), 3 + draw, i, s)
        for h in range(M.horizon):
            rc = rc or lib.urgym_mppi_score(planner, C.byref(M), h, s)
        rc = rc or lib.urgym_mppi_update(src, C.byref(M), s)
        if rc:
            raise RuntimeError(f"a planner launch failed ({rc})")
    end.record()
    torch.cuda.synchronize()
    mppi.close()
    return begin.elapsed_time(mid) / repeats, mid.elapsed_time(end) / repeats


def plan_time(env, options, repeats):
    """ms of one plan of a DeviceMPPI with `options`, whichever entry point they select: device events around `repeats` plans after a
    warm-up of three."""
    import torch

    mppi = DeviceMPPI(env, **options)
    for draw in range(3):
        mppi.plan(draw)
    begin, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    begin.record()
    for draw in range(repeats):
        mppi.plan(3 + draw)
    end.record()
    torch.cuda.synchronize()
    mppi.close()
    return begin.elapsed_time(end) / repeats


def guided_step_time(env, options, repeats):
    """(ms of one urgym_mppi_plan_guided, ms of the launches the guide adds to it), measured like ``control_step_time``.  The second
    figure times the single calls -- per horizon step the actor and the guide launch where samples follow the policy, then actor, critic
    and the terminal launch as the options ask -- without the steps between them; the planner is reset once before them, because the
    single call urgym_actor_forward wants a handle that has observed something."""
    import ctypes as C

    import torch

    from ur_gym_amd import _abi

    mppi = DeviceMPPI(env, **options)
    lib, M, G, planner, s = env.lib, mppi.struct(), mppi.guide(), mppi.planner._h, env._stream()
    for draw in range(3):
        mppi.plan(draw)
    begin, mid, end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    begin.record()
    for draw in range(repeats):
        mppi.plan(3 + draw)
    mid.record()
    torch.cuda.synchronize()
    plan_ms = begin.elapsed_time(mid) / repeats
    mppi.planner.reset(seed=0)
    pa = C.c_void_p(mppi.buf["policy_action"].data_ptr()) if "policy_action" in mppi.buf else None
    rows, out = _abi.CriticRows(None, None, None, G.policy_action), _abi.CriticOut(None, G.value, None)

    def added():
        rc = 0
        for h in range(M.horizon if G.policy_samples else 0):
            rc = rc or lib.urgym_actor_forward(planner, mppi.actor._a, pa, s) or lib.urgym_mppi_guide_actions(planner, C.byref(M), C.byref(G), h, s)
        if G.terminal_value:
            rc = rc or lib.urgym_actor_forward(planner, mppi.actor._a, pa, s)
            rc = rc or lib.urgym_critic_evaluate(planner, mppi.critic._c, C.byref(rows), M.num_parents * M.samples, None, C.byref(out), s)
        if G.terminal_value or G.fail_cost > 0:
            rc = rc or lib.urgym_mppi_terminal(planner, C.byref(M), C.byref(G), s)
        if rc:
            raise RuntimeError(f"a guide launch failed ({rc})")

    for _ in range(3):
        added()
    mid.record()
    for _ in range(repeats):
        added()
    end.record()
    torch.cuda.synchronize()
    mppi.close()
    return plan_ms, mid.elapsed_time(end) / repeats


def protocol(env_id, points, E, steps, device, options):
    """model_test.py's protocol over `points`, E at a time: (success, reward, last step, wall seconds)."""
    import torch

    success, reward, last, wall = [], [], [], 0.0
    for first in range(0, len(points) - E + 1, E) if len(points) >= E else [0]:
        batch = points[first:first + E]
        env = make_vec(env_id, num_envs=len(batch), device=device, seed=4, auto_reset=False)
        env.reset(seed=4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run_closed_loop_mppi(env, batch, max_steps=steps, first_draw=0, **options)  # ends in a device synchronise
        wall += time.perf_counter() - t0
        success.append(res["success"]), reward.append(res["reward"]), last.append(res["last_step"])
        env.close()
    success, reward, last = (np.concatenate(x) for x in (success, reward, last))
    return success, reward, last, wall


def figures(success, reward, last, steps):
    return dict(trials=int(success.size), success_rate_percent=100.0 * float(success.mean()), mean_episode_reward=float(reward.mean()),
                mean_last_step_index=float(last.mean()), early_fail_percent=100.0 * float((~success & (last < steps - 1)).mean()),
                timeout_percent=100.0 * float((last >= steps - 1).mean()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", choices=("ori", "dyn"), default="dyn")
    ap.add_argument("--budget", type=int, default=65536, help="planner envs E * K")
    ap.add_argument("--points", type=int, default=1024, help="test points per grid row (E = budget // K at a time)")
    ap.add_argument("--steps", type=int, default=100, help="control steps per trial (model_test.py: 100)")
    ap.add_argument("--repeats", type=int, default=20, help="plans per timing")
    ap.add_argument("--rows", type=int, default=len(GRID), help="the first so many rows of the grid")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", nargs="+", default=None, metavar="K:H:SIGMA:LAMBDA", help="rows to run in place of the built-in grid")
    ap.add_argument("--actor", default=None, help="actor weights (.npz) for --policy-samples and --terminal-value")
    ap.add_argument("--critics", nargs=2, default=None, metavar="NPZ", help="the two Q-networks' weights for --terminal-value")
    ap.add_argument("--policy-samples", type=int, default=0, help="P: samples 1 .. P of every parent follow the actor")
    ap.add_argument("--policy-sigma", type=float, default=0.1, help="the noise scale around the actor's action (with --policy-samples)")
    ap.add_argument("--terminal-value", action="store_true", help="credit a future alive after H steps with min Q(s_H, actor(s_H))")
    ap.add_argument("--fail-cost", type=float, default=0.0, help="the cost of a future that ends without success")
    ap.add_argument("--guided-gamma", type=float, default=None, help="gamma of the guided rows (default 0.95 with --terminal-value, the critics' own, else 1)")
    ap.add_argument("--iterations", type=int, nargs="+", default=[1], metavar="I", help="refinement iterations of a plan; every row is run once per value")
    ap.add_argument("--elites", type=int, nargs="+", default=None, metavar="M", help="run every row again with only the M best samples weighing in, once per value")
    ap.add_argument("--adapt-std", action="store_true", help="... and once more per M with the std adapted across the iterations of a plan")
    ap.add_argument("--std-min", type=float, default=0.05, help="--adapt-std: the floor of the adaptive std")
    ap.add_argument("--std-max", type=float, default=None, help="--adapt-std: its ceiling (default: the row's sigma)")
    ap.add_argument("--ess-target", type=float, nargs="+", default=None, metavar="T",
                    help="run every row again with the temperature solved per env and update for an effective sample size of T, once per value")
    ap.add_argument("--lam-min", type=float, default=1e-3, help="--ess-target: the lowest temperature of the search")
    ap.add_argument("--lam-max", type=float, default=1e6, help="--ess-target: the highest temperature of the search")
    ap.add_argument("--noise-beta", type=float, nargs="+", default=None, metavar="B",
                    help="run every row again with sampling noise of lag-1 correlation B along the horizon, once per value (0: white noise through the coloured calls)")
    args = ap.parse_args()
    import torch

    kind, env_id = args.env, ENV_IDS[args.env]
    points = test_points(kind, args.points, args.device)
    grid = GRID[:args.rows] if args.grid is None else [(int(k), int(h), float(sg), float(lm)) for k, h, sg, lm in (r.split(":") for r in args.grid)]
    guide = None
    if args.policy_samples or args.terminal_value or args.fail_cost:
        guide = dict(policy_samples=args.policy_samples, policy_sigma=args.policy_sigma if args.policy_samples else 0.0, terminal_value=args.terminal_value,
                     fail_cost=args.fail_cost, actor=args.actor, critic=args.critics,
                     gamma=args.guided_gamma if args.guided_gamma is not None else (0.95 if args.terminal_value else 1.0))
    if args.adapt_std and args.elites is None:
        raise SystemExit("--adapt-std runs beside --elites M (M = K keeps every finite sample)")
    rows = []
    for K, H, sigma, lam, iterations in [(*row, i) for row in grid for i in args.iterations]:
        E = max(1, args.budget // K)
        options = dict(samples=K, horizon=H, sigma=sigma, lam=lam, gamma=1.0, iterations=iterations, shift=True, seed=0)
        success, reward, last, wall = protocol(env_id, points, E, args.steps, args.device, options)
        env = make_vec(env_id, num_envs=E, device=args.device, seed=4, auto_reset=False)
        env.reset(seed=4)
        plan_ms, own_ms = control_step_time(env, options, args.repeats)
        env.close()
        row = dict(K=K, H=H, sigma=sigma, lam=lam, iterations=iterations, E=E, planner_envs=E * K, **figures(success, reward, last, args.steps),
                   plan_ms=plan_ms, planner_kernels_ms=own_ms, planner_kernels_share=own_ms / plan_ms,
                   control_steps_per_second=1e3 / plan_ms, env_control_steps_per_second=E * 1e3 / plan_ms,
                   closed_loop_wall_seconds_including_setup=wall)
        if guide:
            guided = dict(options, **guide)
            success, reward, last, wall = protocol(env_id, points, E, args.steps, args.device, guided)
            env = make_vec(env_id, num_envs=E, device=args.device, seed=4, auto_reset=False)
            env.reset(seed=4)
            guided_ms, added_ms = guided_step_time(env, guided, args.repeats)
            env.close()
            row["guided"] = dict({k: v for k, v in guide.items() if k not in ("actor", "critic")}, **figures(success, reward, last, args.steps),
                                 plan_ms=guided_ms, plan_ms_over_plain=guided_ms / plan_ms, guide_launches_ms=added_ms, guide_launches_share=added_ms / guided_ms,
                                 closed_loop_wall_seconds_including_setup=wall)
        for M, adapt_std in [(m, a) for m in args.elites or () for a in ((False, True) if args.adapt_std else (False,))]:
            adaptive = dict(options, elites=M, adapt_std=adapt_std, std_min=args.std_min, std_max=args.std_max)
            success, reward, last, wall = protocol(env_id, points, E, args.steps, args.device, adaptive)
            env = make_vec(env_id, num_envs=E, device=args.device, seed=4, auto_reset=False)
            env.reset(seed=4)
            adaptive_ms, _ = control_step_time(env, adaptive, args.repeats)  # the second figure times the plain launches: not reported here
            env.close()
            row.setdefault("adaptive", []).append(dict(elites=M, adapt_std=adapt_std, std_min=args.std_min, std_max=sigma if args.std_max is None else args.std_max,
                                                       **figures(success, reward, last, args.steps), plan_ms=adaptive_ms, plan_ms_over_plain=adaptive_ms / plan_ms,
                                                       closed_loop_wall_seconds_including_setup=wall))
        for target in args.ess_target or ():
            tempered = dict(options, ess_target=target, lam_min=args.lam_min, lam_max=args.lam_max)
            success, reward, last, wall = protocol(env_id, points, E, args.steps, args.device, tempered)
            env = make_vec(env_id, num_envs=E, device=args.device, seed=4, auto_reset=False)
            env.reset(seed=4)
            left = {}
            tempered_ms, _ = control_step_time(env, tempered, args.repeats, left)  # the second figure times the plain launches: not reported here
            env.close()
            row.setdefault("tempered", []).append(dict(ess_target=target, lam_min=args.lam_min, lam_max=args.lam_max, **figures(success, reward, last, args.steps),
                                                       plan_ms=tempered_ms, plan_ms_over_plain=tempered_ms / plan_ms, last_plan=left,
                                                       closed_loop_wall_seconds_including_setup=wall))
        for beta in args.noise_beta or ():
            colored = dict(options, **(guide or {}), noise_beta=beta)
            success, reward, last, wall = protocol(env_id, points, E, args.steps, args.device, colored)
            env = make_vec(env_id, num_envs=E, device=args.device, seed=4, auto_reset=False)
            env.reset(seed=4)
            colored_ms = plan_time(env, colored, args.repeats)
            env.close()
            row.setdefault("colored", []).append(dict(noise_beta=beta, guided=bool(guide), **figures(success, reward, last, args.steps), plan_ms=colored_ms,
                                                      plan_ms_over_plain=colored_ms / plan_ms, closed_loop_wall_seconds_including_setup=wall))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "actors", "reference_results.json")))[kind]
    out = dict(env_id=env_id, protocol=f"model_test.py: {args.steps} steps per trial, closed at the first terminated step", budget=args.budget,
               timing=f"device events around {args.repeats} urgym_mppi_plan calls after 3 warm-up plans; planner_kernels_ms is the fan-out, sample, H score and update launches alone",
               reference_trained_actor={k: ref[k] for k in ("success_rate_percent", "mean_episode_reward", "mean_last_step_index", "trials")},
               device=torch.cuda.get_device_name(0), grid=rows)
    if guide:
        out["guide"] = dict({k: v for k, v in guide.items() if k not in ("actor", "critic")}, actor=args.actor and os.path.basename(args.actor),
                            critics=args.critics and [os.path.basename(c) for c in args.critics])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "grid"}))


if __name__ == "__main__":
    main()
