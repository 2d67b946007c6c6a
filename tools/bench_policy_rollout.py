#!/usr/bin/env python
"""Closed-loop rollout with a policy in the loop: what it costs per step, three ways, in ONE process on one MI355X.

  (a) host        the loop as shipped before the device actor: HipBackend.observe() copies three tensors to the host,
                  DeterministicActor (numpy) runs there, the actions are copied back, env.step.
  (b) torch       what a user could build without the device actor: the actor as three torch.nn.functional.linear calls in
                  float32 on the device (cat, relu, tanh around them), then env.step -- no host copies.
  (c) device      env.rollout_policy (urgym_rollout_actor): K x (HIP actor kernel + records, step) enqueued by one native call;
                  once without records and once with all of them.

Every figure is wall time around work that ends in a device synchronise, per step, median of `--repeats` windows that alternate
between the variants.  The actor launch alone is timed with device events around back-to-back urgym_actor_forward calls and set
against the step launch (urgym_query_timing) and the float32 matrix peak.  One JSON line on stdout; --out also writes it to a file.

    python tools/bench_policy_rollout.py --out profiles/policy_rollout/dyn65536.json

--critic measures the twin Q critic launch instead (urgym_critic_evaluate with q, q_min and the SAC target on the N bound rows):
ten alternating windows of 200 back-to-back launches of (1) the deterministic actor, (2) the critic kernel, (3) the same evaluation
in torch float32 on the device (cat, 2 x (3 F.linear, relu), minimum, target arithmetic).  Bar 1: critic median <= 2496 / 1216 x
actor median + the spread of the actor's windows (the matrix instructions per wave of the two kernels at width 256).

    python tools/bench_policy_rollout.py --critic --out profiles/policy_rollout/dyn65536_critic.json

--replay measures the device replay ring (DeviceReplay, capacity --capacity slots), GAUSSIAN policy, auto-reset.  Bar 1: per-step
wall time of ``collect`` (urgym_rollout_collect) against the Python loop that produces the same ring without it -- per step
policy_actions(sample=) into the slot, env.step, and the torch assembly of the transition (three copies of s, three
where(done, final, live) for s', reward and flags) into the preallocated ring tensors -- and against ``rollout_policy`` with all
records; alternating windows, median of --repeats.  The copy bandwidth of the same run (a device-to-device copy_ of one ring
array) prices the bytes collect writes beyond the recorded rollout.  Bar 2: the gather launch (all eleven fields and the index,
preallocated outputs) at batch 256 and 65536 against torch.randint + one index_select per field on the same ring, device events
around --launches back-to-back repetitions.

    python tools/bench_policy_rollout.py --replay --out profiles/policy_rollout/dyn65536_replay.json

--action-gradient measures urgym_critic_action_gradient on the checkpoint's critic (H = 256) at M = 256 (the
learner's batch) and M = --num-envs explicit rows: alternating windows of (1) the gradient launch, (2) critic_kernel on the same rows,
(3) the torch route (cat, two MLPs, minimum, sum().backward() onto a.grad).  Bar 1, at the larger M: gradient median <= (28 HT + 32 HT^2)
/ (28 HT + 16 HT^2) x forward median + the spread of the forward windows (the kernels' own MFMA counts; 1.82 at HT = 8).  Bar 2:
not slower than torch at both M.  Also one SACLearner.update at batch 256 with and without device_action_gradient.  Hidden widths above
256 are not measured: the call refuses them.
    python tools/bench_policy_rollout.py --action-gradient --out profiles/policy_rollout/dyn65536_action_gradient.json

--critic-gradient measures urgym_critic_parameter_gradients on the checkpoint's critic (H = 256) at M = 256 and
M = --num-envs rows: alternating windows of (1) the call (its two or three launches, `target` form, preallocated outputs and workspace)
and (2) torch float32 for the same quantities: critic forward, loss, backward().  Bar: the call is not slower than torch at either M
beyond the spread of the windows.  Also one SACLearner.update at batch 256: default, device_action_gradient, both options.
    python tools/bench_policy_rollout.py --critic-gradient --windows 6 --launches 100 --out profiles/policy_rollout/dyn65536_critic_gradient.json
--actor-gradient measures urgym_actor_parameter_gradients in the SAMPLE form on the checkpoint's actor (H = 256) at
M = 256 and M = num_envs rows, preallocated outputs and workspace, against the torch float32 route for the same quantities
(TorchActor.sample on the call's own noise, then backward() of (action * d_action).sum() + (log_prob * d_log_prob).sum()), and one
SACLearner.update at batch 256 four ways: the default route, device_action_gradient, that with device_critic_gradient, and all three.
    python tools/bench_policy_rollout.py --actor-gradient --windows 6 --launches 100 --out profiles/policy_rollout/dyn65536_actor_gradient.json
--optimizer measures the Adam step kernels at hidden width 256 and 512 on freshly initialised networks with
seeded gradients: one critic_adam_step with a target (tau = 0.005) against torch.optim.Adam.step on the twelve .grad tensors followed by
online.load_parameters(tau=1) and target.load_parameters(tau); one actor_adam_step against Adam.step followed by
device_actor.load_parameters; torch's fused=True Adam in both comparisons as a second line (not the bar).  Each route steps parameters of
its own.  Alternating windows in one process, medians.  Bar: each call is not slower than the torch route beyond the spread of torch's
windows.  Then one SACLearner.update at batch 256 with the three gradient options and with device_optimizer as well, alternating.
    python tools/bench_policy_rollout.py --optimizer --windows 6 --launches 100 --out profiles/policy_rollout/dyn65536_optimizer.json
--entropy measures one SACLearner.update at batch 256, H = 256 (and 512, which the gradient kernels the
options need refuse: recorded as refused), two ways: device_optimizer with the
three gradient options (the route before device_entropy) and the same plus device_entropy.  Alternating windows of --launches updates in one
process, each ending in a device synchronise; wall time per update, medians.  Bar: the new route is not slower than the old beyond the
spread of the old route's windows.  The ratio is reported whatever it is.
    python tools/bench_policy_rollout.py --entropy --windows 8 --launches 200 --out profiles/policy_rollout/dyn65536_entropy.json

--clip measures gradient-norm clipping on the same update (4096 envs, batch 256, H = 256, device_entropy):
`device_entropy`, the learner without max_grad_norm (the thirteen calls it always made), against `clipped`, the learner with
max_grad_norm (fifteen: two norm launches, two scaled steps); and the same pair as ONE SACLearner.train call per window
(urgym_sac_train against urgym_sac_train_clipped).  Alternating windows of --launches updates in one process, each ending in a device
synchronise; median, min and max of the wall time per update, and the extra time per update of the clipped route.  No bar on the
clipped route; the unclipped one is compared with the parent commit's --entropy figure by whoever runs both.  --clip-only runs the
clipped native updates alone: the program of a kernel-trace run.
    python tools/bench_policy_rollout.py --clip --windows 8 --launches 200 --out profiles/policy_rollout/dyn65536_clip.json

--demos measures the demonstration ring.  The launches alone, each pair alternating in one process: urgym_replay_sample
against urgym_replay_sample_mixed with D = M / 2 rows from a second ring of an eighth of the envs, and urgym_sac_policy_terms_cloned against
urgym_sac_policy_terms_cloned_masked with the first M / 2 rows marked, at M = 256 and M = 65536, --launches per window, --windows windows per
kind, timed with device events.  Then one SAC update (4096 envs, batch 256, H = 256) as one native call per window: without the option, with
128 demonstration rows, with cloning, and with cloning on the demonstration rows only.

    python tools/bench_policy_rollout.py --demos --windows 10 --launches 200 --out profiles/policy_rollout/demo_time.json

--clone-weighted measures advantage-weighted cloning.  The launch alone: urgym_sac_policy_terms_cloned (weight 1,
scale_by_q on, no filter) against urgym_sac_policy_terms_weighted (temperature 1, cap 20) on the same seeded device tensors at M = 256 and
M = 65536, alternating in one process, --launches per window, --windows windows per kind, timed with device events.  Then one SAC update
(4096 envs, batch 256, H = 256) as one native call per window: without cloning, with plain cloning, with the advantage weight.

    python tools/bench_policy_rollout.py --clone-weighted --windows 10 --launches 200 --out profiles/policy_rollout/bc_weighted_time.json

--clone measures behaviour cloning in the policy terms.  First the launch alone: urgym_sac_policy_terms against
urgym_sac_policy_terms_cloned (weight 1, scale_by_q and q_filter on) on the same seeded device tensors at M = 256 and M = 65536, --launches
back-to-back launches per window between two device events and a synchronise, the two alternating, median of --windows; both and the
difference are reported, no bound is fixed.  Then the update as in --clip: the learner without the option against the one with
bc_weight=1, bc_scale_by_q, bc_q_filter, as update() calls and as one native call per window, alternating; both and the differences.
    python tools/bench_policy_rollout.py --clone --windows 10 --launches 200 --out profiles/policy_rollout/bc_time.json

--normalize measures running normalization.  The update as in --clip: `device_entropy`, the learner without the
option (the thirteen calls it always made), against `normalized` (fourteen: one urgym_norm_batch after the gather), and the same pair as
ONE SACLearner.train call per window.  Then, at --num-envs envs, a collection step without and with the normalize launch
(env.collect of --collect-steps steps, alternating windows; the two collections follow different trajectories, so their difference is
NOT the launch's cost: the kernel trace of --normalize-only is) and one fold of those steps (two launches).  Medians, mins and maxes of
wall times between device synchronises.  No bar on the normalized routes.  --normalize-only runs the normalized collection, the fold and
the normalized native updates alone: the program of a kernel-trace run.
    python tools/bench_policy_rollout.py --normalize --windows 8 --launches 200 --out profiles/policy_rollout/dyn65536_norm.json

--native measures the same update (batch 256, H = 256, device_entropy) two ways: the thirteen-call
SACLearner.update, and SACLearner.train(steps_per_iteration=0, updates_per_iteration=--launches), one native call per window.
Alternating windows in one process, each ending in a device synchronise; median, min and max of the wall time per update.  Bar: the
native route's median is not above the thirteen-call route's by more than the spread (max - min) of that route's own windows.  A second
pair, `loop`, runs one collection step per 4 updates on both routes (--launches / 4 iterations per window).  With --native-only the
tool runs --launches native updates --windows times and nothing else: the program of a kernel-trace run.
    python tools/bench_policy_rollout.py --native --windows 8 --launches 200 --out profiles/policy_rollout/dyn65536_native.json

--evaluate measures the evaluation inside the training call, 1024 evaluation envs x 100 steps, H = 256.
`one_evaluation`: DeviceEvaluation.evaluate + results() against the route before it, load_parameters + reset(seed) +
run_closed_loop_device; one evaluation per window, ending in a synchronise and reading its result.  `training_run`: --launches
updates as --launches / 4 x (1 step, 4 updates) with an evaluation every 40 updates, as ONE SACLearner.train(..., evaluation=,
eval_every=40) call against one train call per interval plus the Python evaluation.  Alternating windows in one process; median,
min and max of the wall time in ms; the bar of --native on `one_evaluation`, the ratio reported whatever it is.
    python tools/bench_policy_rollout.py --evaluate --windows 8 --launches 200 --out profiles/policy_rollout/dyn_evaluation.json

--monitor measures the training-episode statistics inside the training call, 4096 envs, batch 256, H = 256:
--launches updates as --launches / 4 x (1 step, 4 updates) in ONE SACLearner.train call as it was, against the same call with
monitor=, log_every=10 (a fold launch per iteration, a stats launch per ten).  Alternating windows in one process, each ending in a
synchronise; median, min and max of the wall time in ms.  Bar: the monitored median is not above the plain one by more than the spread
(max - min) of the plain route's own windows; the excess per iteration is reported whatever it is.  --monitored-only runs the monitored
call alone: the program of a kernel-trace run.
    python tools/bench_policy_rollout.py --monitor --windows 8 --launches 200 --out profiles/policy_rollout/dyn_monitor.json

With --refresh: what it costs to hand new weights to a device actor / critic, at hidden width 256 and 512.
`actor_load`, `critic_load_tau1` and `critic_load_polyak` (tau = 0.005) are load_parameters from device tensors, one launch each;
`*_host_route` is the only route there was before: every tensor .cpu().numpy(), destroy and create the object (the actor's head by
set_log_std); `*_copy` is the floor, one torch device-to-device copy_ of as many bytes as the packed buffer.  Wall time around
--launches calls that end in a device synchronise (the host route: --host-steps calls), alternating windows, median of --windows.
Bar 1: each load is not slower than its host route.  Bar 2 (no threshold): the ratio to the copy and the bytes written per second.
Then one SACLearner.update at batch 256 and the share of it that the two loads take.

    python tools/bench_policy_rollout.py --refresh --out profiles/policy_rollout/dyn65536_refresh.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 (AMD's specification)
ACTOR_NPZ = {"UR5OriReach-v1": "ori", "UR5ObsReach-v1": "obs", "UR5StaReach-v1": "sta", "UR5DynReach-v1": "dyn"}


def critic_mode(args):
    import ctypes as C

    import torch
    import torch.nn.functional as F

    from ur_gym_amd import _abi, make_vec
    from ur_gym_amd.evaluation import CRITIC_ARRAYS, DeviceActor, DeviceCritic

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, kind = "cuda:0", args.num_envs, ACTOR_NPZ[args.env]
    golden = os.path.join(ROOT, "tests", "golden")
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    actor = DeviceActor.load(os.path.join(golden, "actors", f"actor_{kind}.npz"), env)
    paths = [os.path.join(golden, "critics", f"critic_{kind}_qf{i}.npz") for i in (0, 1)]
    critic = DeviceCritic.load(paths, env)
    with open(os.path.join(golden, "critics", "sac_hyperparameters.json")) as f:
        hyp = json.load(f)[kind]
    gamma, alpha = hyp["gamma"], float(np.exp(hyp["log_ent_coef"]))
    tw = [{k: torch.from_numpy(np.ascontiguousarray(np.load(p)[k], dtype=np.float32)).to(dev) for k in CRITIC_ARRAYS} for p in paths]
    for _ in range(20):
        env.step(torch.rand((n, 6), device=dev) * 2.0 - 1.0)
    b = env.buf
    actions = torch.rand((n, 6), device=dev) * 2.0 - 1.0
    log_prob = torch.randn((n,), device=dev) * 2.0 - 3.0
    reward, term = b["reward"].clone(), b["terminated"].clone()
    out = {k: torch.empty(shape, dtype=torch.float32, device=dev) for k, shape in (("a", (n, 6)), ("q", (2, n)), ("q_min", (n,)), ("target", (n,)))}
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float))  # noqa: E731
    rows = _abi.CriticRows(None, None, None, fp(actions))
    terms = _abi.CriticTerms(fp(reward), C.cast(term.data_ptr(), C.POINTER(C.c_uint8)), fp(log_prob), gamma, alpha)
    outs = _abi.CriticOut(fp(out["q"]), fp(out["q_min"]), fp(out["target"]))
    h, stream, a_p = env._h, env._stream(), C.c_void_p(out["a"].data_ptr())

    def torch_critic():
        x = torch.cat([b["achieved_goal"], b["desired_goal"], b["observation"], actions], dim=1)
        q = []
        for w in tw:
            y = F.relu(F.linear(x, w["q_0_weight"], w["q_0_bias"]))
            y = F.relu(F.linear(y, w["q_2_weight"], w["q_2_bias"]))
            q.append(F.linear(y, w["q_4_weight"], w["q_4_bias"])[:, 0])
        q_min = torch.minimum(q[0], q[1])
        return q, q_min, reward + gamma * (1.0 - term.float()) * (q_min - alpha * log_prob)

    def check(rc):
        if rc != 0:
            raise SystemExit(env.lib.urgym_last_error(h).decode())

    kinds = {"actor": lambda: check(env.lib.urgym_actor_forward(h, actor._a, a_p, stream)),
             "critic": lambda: check(env.lib.urgym_critic_evaluate(h, critic._c, C.byref(rows), n, C.byref(terms), C.byref(outs), stream)),
             "torch_critic": torch_critic}
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in kinds.values():
        for _ in range(10):
            fn()
    # faster and different is not faster: the two evaluations agree to float32 rounding on these rows
    sync()
    tq, tq_min, tt = torch_critic()
    agree = {"q": float((torch.stack(tq) - out["q"]).abs().max()), "q_min": float((tq_min - out["q_min"]).abs().max()),
             "target": float((tt - out["target"]).abs().max()), "q_abs_max": float(out["q"].abs().max())}
    windows = {k: [] for k in kinds}
    for _ in range(args.windows):
        for name, fn in kinds.items():
            sync()
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            sync()
            windows[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    med = {k: float(np.median(v)) for k, v in windows.items()}
    spread = float(max(windows["actor"]) - min(windows["actor"]))
    H = critic.hidden_width
    flop = 2.0 * n * 2 * (critic.in_features * H + H * H + H)
    result = {"tool": "bench_policy_rollout --critic", "env": args.env, "num_envs": n, "hidden_width": H, "windows": args.windows,
              "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0),
              "us_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()}, "us_median": med, "actor_us_spread": spread,
              "mfma_per_wave": {"actor": 1216, "critic": 2496}, "bar1_us": 2496.0 / 1216.0 * med["actor"] + spread,
              "within_bar1": med["critic"] <= 2496.0 / 1216.0 * med["actor"] + spread, "critic_over_actor": med["critic"] / med["actor"],
              "not_slower_than_torch": med["critic"] <= med["torch_critic"], "speedup_over_torch": med["torch_critic"] / med["critic"],
              "critic_gflop_per_launch": flop / 1e9, "critic_tflops": flop / med["critic"] / 1e6,
              "critic_fraction_of_f32_matrix_peak": flop / med["critic"] / 1e6 / F32_MATRIX_PEAK_TFLOPS, "max_abs_difference_from_torch": agree}
    critic.close()
    actor.close()
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def replay_mode(args):
    import torch

    from ur_gym_amd import _abi, make_vec
    from ur_gym_amd.evaluation import DeviceActor, DeviceReplay

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, K, cap, kind = "cuda:0", args.num_envs, args.steps, args.capacity, ACTOR_NPZ[args.env]
    w = dict(np.load(os.path.join(ROOT, "tests", "golden", "actors", f"actor_{kind}.npz")))
    w.update(np.load(os.path.join(ROOT, "tests", "golden", "actors", f"log_std_{kind}.npz")))
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    actor = DeviceActor(w, env)
    replay, loop_ring = DeviceReplay(env, cap), DeviceReplay(env, cap)  # the second one is filled by the Python loop
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    draws = [0]  # every window continues the draw sequence
    rows = ("observation", "achieved_goal", "desired_goal")

    def how(steps):
        d = dict(mode="gaussian", seed=1, first_draw=draws[0])
        draws[0] += steps
        return d

    def collect(steps):
        replay.collect(actor, steps, sample=how(steps))

    def python_loop(steps):
        r, b = loop_ring.ring, env.buf
        first = how(steps)["first_draw"]
        for k in range(steps):
            slot = (loop_ring.cursor + k) % cap
            for key in rows:
                r[key][slot].copy_(b[key])
            env.policy_actions(actor, out=r["action"][slot], sample=dict(mode="gaussian", seed=1, first_draw=first + k))
            obs, rew, term, trunc, info = env.step(r["action"][slot])
            done = (term | trunc)[:, None]
            for key in rows:
                torch.where(done, info["final_observation"][key], obs[key], out=r["next_" + key][slot])
            r["reward"][slot].copy_(rew)
            r["terminated"][slot].copy_(term)
            r["truncated"][slot].copy_(trunc)
            r["is_success"][slot].copy_(info["is_success"])
        loop_ring.cursor = (loop_ring.cursor + steps) % cap
        loop_ring.filled = min(cap, loop_ring.filled + steps)

    def recorded(steps):
        return env.rollout_policy(actor, steps, record="all", sample=how(steps))

    def plain(steps):
        env.rollout_policy(actor, steps, record=(), sample=how(steps))

    variants = [("collect", collect), ("python_loop_into_ring", python_loop), ("rollout_all_records", recorded), ("rollout_no_records", plain)]
    for _, fn in variants:
        fn(10)
    plain(args.warmup)
    sync()
    times = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            fn(K)
            sync()
            times[name].append((time.perf_counter() - t0) / K * 1e6)
    per_step = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float(max(v) - min(v)) for k, v in times.items()}

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        sync()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / reps

    # the copy bandwidth of this run: one ring array onto another, read + write counted
    src, dst = replay.ring["observation"], loop_ring.ring["observation"]
    copy_bytes = 2 * src.numel() * 4
    window(lambda: dst.copy_(src), 3)
    copy_us = float(np.median([window(lambda: dst.copy_(src), 5) for _ in range(args.repeats)]))
    copy_bw = copy_bytes / copy_us * 1e6
    row_bytes = (2 * (env.obs_dim + 2 * env.goal_dim) + 6 + 1) * 4 + 3  # a transition in the ring
    # rollout_policy(record="all", sample=): s, action, reward, four flags, the four sample records (final_observation only where done)
    record_bytes = (env.obs_dim + 2 * env.goal_dim + 6 + 1 + 19) * 4 + 4
    extra = per_step["collect"] - per_step["rollout_all_records"]
    byte_cost = (row_bytes - record_bytes) * n / copy_bw * 1e6

    # bar 2: the gather against torch on the same (full) ring
    while replay.filled < cap:
        collect(min(K, cap - replay.filled))
    sync()
    size, gather = replay.filled * n, {}
    flat = {name: t.reshape((cap * n,) + tuple(t.shape[2:])) for name, t in replay.ring.items()}
    for B in (256, 65536):
        out = {name: torch.empty((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for name, t in flat.items()}
        ours = dict(out, index=torch.empty((B,), dtype=torch.int64, device=dev))
        tick = [0]

        def device_gather():
            tick[0] += 1
            replay.sample_into(ours, 3, tick[0])

        def torch_gather():
            idx = torch.randint(0, size, (B,), device=dev)
            for name, t in flat.items():
                torch.index_select(t, 0, idx, out=out[name])

        kinds = {"device": device_gather, "torch": torch_gather}
        for fn in kinds.values():
            for _ in range(10):
                fn()
        wins = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for name, fn in kinds.items():
                wins[name].append(window(fn, args.launches))
        med = {k: float(np.median(v)) for k, v in wins.items()}
        moved = B * (2 * row_bytes + 8)
        gather[str(B)] = {"us_windows": {k: [round(x, 3) for x in v] for k, v in wins.items()}, "us_median": med,
                          "not_slower_than_torch": med["device"] <= med["torch"], "speedup_over_torch": med["torch"] / med["device"],
                          "bytes_read_and_written": moved, "device_bytes_per_s": moved / med["device"] * 1e6}
    result = {"tool": "bench_policy_rollout --replay", "env": args.env, "num_envs": n, "steps": K, "capacity_steps": cap, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "us_per_step_median": per_step, "us_per_step_spread": spread,
              "us_per_step_all": {k: [round(x, 2) for x in v] for k, v in times.items()},
              "collect_not_slower_than_python_loop": per_step["collect"] <= per_step["python_loop_into_ring"],
              "speedup_over_python_loop": per_step["python_loop_into_ring"] / per_step["collect"],
              "ring_bytes_per_env_step": row_bytes, "record_bytes_per_env_step": record_bytes,
              "collect_minus_rollout_all_records_us": extra, "copy_bytes_per_s": copy_bw, "extra_bytes_at_copy_bandwidth_us": byte_cost,
              "extra_within_spread_plus_byte_cost": extra <= spread["collect"] + spread["rollout_all_records"] + byte_cost,
              "collect_minus_rollout_no_records_us": per_step["collect"] - per_step["rollout_no_records"],
              "store_bytes_per_s": (row_bytes - 24) * n / max(per_step["collect"] - per_step["rollout_no_records"], 1e-9) * 1e6,
              "gather": gather, "parent_rollout_all_records_us": 466.0}
    actor.close()
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def refresh_mode(args):
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import ACTOR_ARRAYS, CRITIC_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceCritic, DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n = "cuda:0", args.num_envs
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    n_in = env.obs_dim + 2 * env.goal_dim
    rng = np.random.default_rng(0)

    def window(fn, calls):
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        return (time.perf_counter() - t0) * 1e6 / calls

    rows = {}
    for H in (256, 512):
        shapes_a = dict(zip(ACTOR_ARRAYS + LOG_STD_ARRAYS, ((H, n_in), (H,), (H, H), (H,), (6, H), (6,), (6, H), (6,))))
        shapes_c = dict(zip(CRITIC_ARRAYS, ((H, n_in + 6), (H,), (H, H), (H,), (1, H), (1,))))
        wa = {k: (rng.standard_normal(sh) * 0.1).astype(np.float32) for k, sh in shapes_a.items()}
        wc = [{k: (rng.standard_normal(sh) * 0.1).astype(np.float32) for k, sh in shapes_c.items()} for _ in range(2)]
        ta = {k: torch.from_numpy(v).to(dev) for k, v in wa.items()}
        tc = [{k: torch.from_numpy(v).to(dev) for k, v in w.items()} for w in wc]
        obj = {"actor": DeviceActor(wa, env), "critic": DeviceCritic(wc, env)}
        bytes_a, bytes_c = obj["actor"].packed().nbytes, obj["critic"].packed().nbytes
        flat = {"a": (torch.empty(bytes_a // 4, device=dev), torch.empty(bytes_a // 4, device=dev)),
                "c": (torch.empty(bytes_c // 4, device=dev), torch.empty(bytes_c // 4, device=dev))}

        def actor_host_route():
            w = {k: v.cpu().numpy() for k, v in ta.items()}
            obj["actor"].close()
            obj["actor"] = DeviceActor(w, env)

        def critic_host_route():
            w = [{k: v.cpu().numpy() for k, v in net.items()} for net in tc]
            obj["critic"].close()
            obj["critic"] = DeviceCritic(w, env)

        kinds = {"actor_load": (lambda: obj["actor"].load_parameters(ta), args.launches),
                 "critic_load_tau1": (lambda: obj["critic"].load_parameters(tc, tau=1.0), args.launches),
                 "critic_load_polyak": (lambda: obj["critic"].load_parameters(tc, tau=0.005), args.launches),
                 "actor_copy": (lambda: flat["a"][0].copy_(flat["a"][1]), args.launches),
                 "critic_copy": (lambda: flat["c"][0].copy_(flat["c"][1]), args.launches),
                 "actor_host_route": (actor_host_route, args.host_steps),
                 "critic_host_route": (critic_host_route, args.host_steps)}
        for fn, _ in kinds.values():
            for _ in range(3):
                fn()
        wins = {k: [] for k in kinds}
        for _ in range(args.windows):
            for name, (fn, calls) in kinds.items():
                wins[name].append(window(fn, calls))
        med = {k: float(np.median(v)) for k, v in wins.items()}
        row = {"packed_bytes": {"actor": bytes_a, "critic": bytes_c}, "us_median": med,
               "us_windows": {k: [round(x, 3) for x in v] for k, v in wins.items()}}
        for load, base, copy, nbytes in (("actor_load", "actor_host_route", "actor_copy", bytes_a),
                                         ("critic_load_tau1", "critic_host_route", "critic_copy", bytes_c),
                                         ("critic_load_polyak", "critic_host_route", "critic_copy", bytes_c)):
            row[load] = {"not_slower_than_host_route": med[load] <= med[base], "host_route_over_load": med[base] / med[load],
                         "load_over_copy": med[load] / med[copy], "packed_gbytes_per_s": nbytes / med[load] / 1e3}
        rows[str(H)] = row
        obj["actor"].close()
        obj["critic"].close()

    # one SACLearner.update at batch 256 and the share of the two loads
    learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256)
    replay = DeviceReplay(env, 4)
    learner.collect(replay, 4)
    for i in range(5):
        learner.update(replay, 1, i)
    loads = lambda: (learner.device_actor.load_parameters(learner.actor.tensors()),  # noqa: E731
                     learner.target.load_parameters(learner.critic.tensors(), tau=learner.hp["tau"]))
    draw = [100]

    def one_update():
        draw[0] += 1
        learner.update(replay, 1, draw[0])

    up, ld = [], []
    for _ in range(args.windows):
        up.append(window(one_update, 20))
        ld.append(window(loads, 20))
    up_med, ld_med = float(np.median(up)), float(np.median(ld))
    learner.close()
    result = {"tool": "bench_policy_rollout --refresh", "env": args.env, "num_envs": n, "windows": args.windows, "launches_per_window": args.launches,
              "host_route_calls_per_window": args.host_steps, "device": torch.cuda.get_device_name(0), "hidden_width": rows,
              "learner_update": {"batch_size": 256, "hidden_width": 256, "us_median": up_med, "us_windows": [round(x, 2) for x in up],
                                 "two_loads_us_median": ld_med, "two_loads_share": ld_med / up_med}}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def action_gradient_mode(args):
    import torch
    import torch.nn.functional as F

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import CRITIC_ARRAYS, DeviceCritic, DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, kind = "cuda:0", args.num_envs, ACTOR_NPZ[args.env]
    golden = os.path.join(ROOT, "tests", "golden")
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    paths = [os.path.join(golden, "critics", f"critic_{kind}_qf{i}.npz") for i in (0, 1)]
    critic = DeviceCritic.load(paths, env)
    tw = [{k: torch.from_numpy(np.ascontiguousarray(np.load(p)[k], dtype=np.float32)).to(dev) for k in CRITIC_ARRAYS} for p in paths]
    for _ in range(20):
        env.step(torch.rand((n, 6), device=dev) * 2.0 - 1.0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, count):
        sync()
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / count

    HT = (critic.hidden_width + 127) // 128 * 4
    ratio = (28.0 * HT + 32.0 * HT * HT) / (28.0 * HT + 16.0 * HT * HT)
    sizes = {}
    for m in sorted({256, n}):
        rows = {k: env.buf[k][:m].clone() for k in env.ROW_KEYS}
        actions = torch.rand((m, 6), device=dev) * 2.0 - 1.0
        feat = torch.cat([rows["achieved_goal"], rows["desired_goal"], rows["observation"]], dim=1)

        def torch_route():
            a = actions.clone().requires_grad_(True)
            x = torch.cat([feat, a], dim=1)
            q = []
            for w in tw:
                y = F.relu(F.linear(x, w["q_0_weight"], w["q_0_bias"]))
                y = F.relu(F.linear(y, w["q_2_weight"], w["q_2_bias"]))
                q.append(F.linear(y, w["q_4_weight"], w["q_4_bias"])[:, 0])
            torch.minimum(q[0], q[1]).sum().backward()
            return a.grad

        kinds = {"gradient": lambda: env.critic_action_gradient(critic, actions, rows=rows),
                 "forward": lambda: env.critic_values(critic, actions, rows=rows), "torch": torch_route}
        for fn in kinds.values():
            for _ in range(5):
                fn()
        sync()
        got, ref = env.critic_action_gradient(critic, actions, rows=rows)["dqmin_da"], torch_route()
        agree = {"max_abs_difference_from_torch": float((got - ref).abs().max()), "g_abs_max": float(ref.abs().max())}
        windows = {k: [] for k in kinds}
        for _ in range(args.windows):
            for name, fn in kinds.items():
                windows[name].append(window(fn, args.launches))
        med = {k: float(np.median(v)) for k, v in windows.items()}
        spread = float(max(windows["forward"]) - min(windows["forward"]))
        sizes[str(m)] = {"us_median": med, "us_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()}, "forward_us_spread": spread,
                         "gradient_over_forward": med["gradient"] / med["forward"], "bar1_us": ratio * med["forward"] + spread,
                         "within_bar1": med["gradient"] <= ratio * med["forward"] + spread,
                         "not_slower_than_torch": med["gradient"] <= med["torch"], "speedup_over_torch": med["torch"] / med["gradient"], **agree}
    critic.close()
    updates = {}
    for label, option in (("parent_route", False), ("device_action_gradient", True)):
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, device_action_gradient=option)
        replay = DeviceReplay(env, 4)
        learner.collect(replay, 4)
        draw = [0]

        def one_update():
            draw[0] += 1
            learner.update(replay, 1, draw[0])

        for _ in range(5):
            one_update()
        w = [window(one_update, 20) for _ in range(args.windows)]
        updates[label] = {"us_median": float(np.median(w)), "us_windows": [round(x, 2) for x in w]}
        learner.close()
    result = {"tool": "bench_policy_rollout --action-gradient", "env": args.env, "hidden_width": critic.hidden_width, "windows": args.windows,
              "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0), "mfma_ratio": ratio, "rows": sizes,
              "bar1_at_rows": n, "within_bar1": sizes[str(n)]["within_bar1"],
              "not_slower_than_torch": all(v["not_slower_than_torch"] for v in sizes.values()),
              "learner_update_batch256": updates, "hidden_512": "not measured: urgym_critic_action_gradient refuses hidden widths above 256"}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def critic_gradient_mode(args):
    import torch
    import torch.nn.functional as F

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import CRITIC_ARRAYS, DeviceCritic, DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, kind = "cuda:0", args.num_envs, ACTOR_NPZ[args.env]
    golden = os.path.join(ROOT, "tests", "golden")
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    paths = [os.path.join(golden, "critics", f"critic_{kind}_qf{i}.npz") for i in (0, 1)]
    critic = DeviceCritic.load(paths, env)
    tw = [{k: torch.from_numpy(np.ascontiguousarray(np.load(p)[k], dtype=np.float32)).to(dev).requires_grad_(True) for k in CRITIC_ARRAYS} for p in paths]
    for _ in range(20):
        env.step(torch.rand((n, 6), device=dev) * 2.0 - 1.0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, count):
        sync()
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / count

    sizes = {}
    for m in sorted({256, n}):
        rows = {k: env.buf[k][:m].clone() for k in env.ROW_KEYS}
        actions = torch.rand((m, 6), device=dev) * 2.0 - 1.0
        y = torch.randn((m,), device=dev)
        x = torch.cat([rows["achieved_goal"], rows["desired_goal"], rows["observation"], actions], dim=1)
        out = [{k: torch.empty_like(v) for k, v in w.items()} for w in tw]
        ws = env.critic_gradient_workspace(critic, m)

        def torch_route():  # critic forward, loss, backward(): the same quantities in torch float32
            q = []
            for w in tw:
                w_grad = [w[k] for k in CRITIC_ARRAYS]
                for p in w_grad:
                    p.grad = None
                h = F.relu(F.linear(x, w["q_0_weight"], w["q_0_bias"]))
                h = F.relu(F.linear(h, w["q_2_weight"], w["q_2_bias"]))
                q.append(F.linear(h, w["q_4_weight"], w["q_4_bias"])[:, 0])
            (0.5 * (((q[0] - y) ** 2).mean() + ((q[1] - y) ** 2).mean())).backward()

        kinds = {"gradients": lambda: env.critic_parameter_gradients(critic, actions, target=y, scale=1.0 / m, rows=rows, out=out, workspace=ws),
                 "torch": torch_route}
        for fn in kinds.values():
            for _ in range(5):
                fn()
        sync()
        agree = {k: {"max_abs_difference_from_torch": float((out[0][k] - tw[0][k].grad).abs().max()), "g_abs_max": float(tw[0][k].grad.abs().max())}
                 for k in CRITIC_ARRAYS}
        windows = {k: [] for k in kinds}
        for _ in range(args.windows):
            for name, fn in kinds.items():
                windows[name].append(window(fn, args.launches))
        med = {k: float(np.median(v)) for k, v in windows.items()}
        spread = float(max(windows["torch"]) - min(windows["torch"]))
        sizes[str(m)] = {"us_median": med, "us_windows": {k: [round(v, 3) for v in vs] for k, vs in windows.items()}, "torch_us_spread": spread,
                         "launches_per_call": 2 if m <= 1024 else 3, "workspace_bytes": int(ws.numel()) * 4,
                         "not_slower_than_torch": med["gradients"] <= med["torch"] + spread, "speedup_over_torch": med["torch"] / med["gradients"],
                         "qf0": agree}
    critic.close()
    updates = {}
    for label, options in (("parent_route", {}), ("device_action_gradient", dict(device_action_gradient=True)),
                           ("both_options", dict(device_action_gradient=True, device_critic_gradient=True))):
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, **options)
        replay = DeviceReplay(env, 4)
        learner.collect(replay, 4)
        draw = [0]

        def one_update():
            draw[0] += 1
            learner.update(replay, 1, draw[0])

        for _ in range(5):
            one_update()
        w = [window(one_update, 20) for _ in range(args.windows)]
        updates[label] = {"us_median": float(np.median(w)), "us_windows": [round(v, 2) for v in w]}
        learner.close()
    result = {"tool": "bench_policy_rollout --critic-gradient", "env": args.env, "hidden_width": critic.hidden_width, "windows": args.windows,
              "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0), "rows": sizes,
              "not_slower_than_torch": all(v["not_slower_than_torch"] for v in sizes.values()), "learner_update_batch256": updates}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def actor_gradient_mode(args):
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import ACTOR_ARRAYS, LOG_STD_ARRAYS, DeviceActor, DeviceReplay
    from ur_gym_amd.training import SACLearner, TorchActor

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, kind = "cuda:0", args.num_envs, ACTOR_NPZ[args.env]
    golden = os.path.join(ROOT, "tests", "golden", "actors")
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    w = dict(np.load(os.path.join(golden, f"actor_{kind}.npz")))
    w.update(np.load(os.path.join(golden, f"log_std_{kind}.npz")))
    actor = DeviceActor(w, env)
    keys = ACTOR_ARRAYS + LOG_STD_ARRAYS
    ta = TorchActor(actor.in_features, actor.hidden_width).to(dev)
    for k, p in ta.tensors().items():
        p.data.copy_(torch.from_numpy(np.ascontiguousarray(w[k], dtype=np.float32)))
    for _ in range(20):
        env.step(torch.rand((n, 6), device=dev) * 2.0 - 1.0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, count):
        sync()
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / count

    sizes = {}
    how = dict(mode="gaussian", seed=1, first_draw=1 << 63)
    for m in sorted({256, n}):
        rows = {k: env.buf[k][:m].clone() for k in env.ROW_KEYS}
        d_action = torch.randn((m, 6), device=dev) / m
        d_log_prob = torch.full((m,), 1.0 / m, device=dev)
        x = torch.cat([rows["achieved_goal"], rows["desired_goal"], rows["observation"]], dim=1)
        out = {k: torch.empty_like(p) for k, p in ta.tensors().items()}
        ws = env.actor_gradient_workspace(actor, m)
        eps = env.actor_parameter_gradients(actor, sample=how, rows=rows, d_action=d_action, d_log_prob=d_log_prob, records=("noise",))["noise"]

        def torch_route():  # TorchActor.sample forward on given eps, loss, backward(): the same quantities in torch float32
            for p in ta.parameters():
                p.grad = None
            action, log_prob = ta.sample(x, eps)
            ((action * d_action).sum() + (log_prob * d_log_prob).sum()).backward()

        kinds = {"gradients": lambda: env.actor_parameter_gradients(actor, sample=how, rows=rows, d_action=d_action, d_log_prob=d_log_prob, out=out, workspace=ws),
                 "torch": torch_route}
        for fn in kinds.values():
            for _ in range(5):
                fn()
        sync()
        agree = {k: {"max_abs_difference_from_torch": float((out[k] - p.grad).abs().max()), "g_abs_max": float(p.grad.abs().max())} for k, p in ta.tensors().items()}
        windows = {k: [] for k in kinds}
        for _ in range(args.windows):
            for name, fn in kinds.items():
                windows[name].append(window(fn, args.launches))
        med = {k: float(np.median(v)) for k, v in windows.items()}
        spread = float(max(windows["torch"]) - min(windows["torch"]))
        sizes[str(m)] = {"us_median": med, "us_windows": {k: [round(v, 3) for v in vs] for k, vs in windows.items()}, "torch_us_spread": spread,
                         "launches_per_call": 2 if m <= 1024 else 3, "workspace_bytes": int(ws.numel()) * 4,
                         "not_slower_than_torch": med["gradients"] <= med["torch"] + spread, "speedup_over_torch": med["torch"] / med["gradients"],
                         "tensors": agree}
    actor.close()
    updates = {}
    for label, options in (("parent_route", {}), ("device_action_gradient", dict(device_action_gradient=True)),
                           ("action_and_critic", dict(device_action_gradient=True, device_critic_gradient=True)),
                           ("all_three_options", dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True))):
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, **options)
        replay = DeviceReplay(env, 4)
        learner.collect(replay, 4)
        draw = [0]

        def one_update():
            draw[0] += 1
            learner.update(replay, 1, draw[0])

        for _ in range(5):
            one_update()
        wdw = [window(one_update, 20) for _ in range(args.windows)]
        updates[label] = {"us_median": float(np.median(wdw)), "us_windows": [round(v, 2) for v in wdw]}
        learner.close()
    result = {"tool": "bench_policy_rollout --actor-gradient", "env": args.env, "hidden_width": int(w["mu_weight"].shape[1]), "windows": args.windows,
              "launches_per_window": args.launches, "device": torch.cuda.get_device_name(0), "rows": sizes,
              "not_slower_than_torch": all(v["not_slower_than_torch"] for v in sizes.values()), "learner_update_batch256": updates}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def optimizer_mode(args):
    """--optimizer: one critic_adam_step (with a target) and one actor_adam_step against the torch route the learner uses today
    (Adam.step on the .grad tensors, then the reloads), at H = 256 and 512, alternating windows in one process, medians; torch's
    fused=True Adam as a second line; and SACLearner.update at batch 256 with three options and with four."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceActor, DeviceCritic, DeviceReplay
    from ur_gym_amd.training import SACLearner, TorchActor, TorchTwinCritic, host_arrays

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n = "cuda:0", min(args.num_envs, 4096)  # the step calls do not depend on the number of envs
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    n_in = env.obs_dim + 2 * env.goal_dim
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, count):
        sync()
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / count

    def measure(kinds):
        for fn in kinds.values():
            for _ in range(5):
                fn()
        windows = {k: [] for k in kinds}
        for _ in range(args.windows):
            for name, fn in kinds.items():
                windows[name].append(window(fn, args.launches))
        med = {k: float(np.median(v)) for k, v in windows.items()}
        spread = float(max(windows["torch"]) - min(windows["torch"]))
        return {"us_median": med, "us_windows": {k: [round(v, 3) for v in vs] for k, vs in windows.items()}, "torch_us_spread": spread,
                "not_slower_than_torch": med["device"] <= med["torch"] + spread, "speedup_over_torch": med["torch"] / med["device"],
                "speedup_over_torch_fused": med["torch_fused"] / med["device"]}

    widths = {}
    for H in (256, 512):
        torch.manual_seed(H)
        res = {}
        # each route steps parameters of its own, so that none sees another's moments; the gradients are shared and only read
        critics = [TorchTwinCritic(n_in + 6, H).to(dev) for _ in range(3)]
        grads = [{k: torch.randn_like(p) * 1e-3 for k, p in w.items()} for w in critics[0].tensors()]
        for c in critics[1:]:
            for w, g in zip(c.tensors(), grads):
                for k, p in w.items():
                    p.grad = g[k]
        online, target = DeviceCritic(host_arrays(critics[0].tensors()), env), DeviceCritic(host_arrays(critics[0].tensors()), env)
        online_t, target_t = DeviceCritic(host_arrays(critics[0].tensors()), env), DeviceCritic(host_arrays(critics[0].tensors()), env)
        m = [{k: torch.zeros_like(p) for k, p in w.items()} for w in critics[0].tensors()]
        v = [{k: torch.zeros_like(p) for k, p in w.items()} for w in critics[0].tensors()]
        opt = torch.optim.Adam(critics[1].parameters(), lr=1e-4)
        opt_fused = torch.optim.Adam(critics[2].parameters(), lr=1e-4, fused=True)
        step = [0]

        def device_critic():
            step[0] += 1
            env.critic_adam_step(online, critics[0].tensors(), grads, m, v, lr=1e-4, step=step[0], target=target, tau=0.005)

        def torch_critic(o=opt, c=critics[1]):
            o.step()
            online_t.load_parameters(c.tensors(), tau=1.0)
            target_t.load_parameters(c.tensors(), tau=0.005)

        res["critic"] = measure({"device": device_critic, "torch": torch_critic, "torch_fused": lambda: torch_critic(opt_fused, critics[2])})
        for c in (online, target, online_t, target_t):
            c.close()

        actors = [TorchActor(n_in, H).to(dev) for _ in range(3)]
        agrads = {k: torch.randn_like(p) * 1e-3 for k, p in actors[0].tensors().items()}
        for a in actors[1:]:
            for k, p in a.tensors().items():
                p.grad = agrads[k]
        da, da_t = DeviceActor(host_arrays(actors[0].tensors()), env), DeviceActor(host_arrays(actors[0].tensors()), env)
        am, av = ({k: torch.zeros_like(p) for k, p in actors[0].tensors().items()} for _ in range(2))
        aopt = torch.optim.Adam(actors[1].parameters(), lr=1e-4)
        aopt_fused = torch.optim.Adam(actors[2].parameters(), lr=1e-4, fused=True)
        astep = [0]

        def device_actor():
            astep[0] += 1
            env.actor_adam_step(da, actors[0].tensors(), agrads, am, av, lr=1e-4, step=astep[0])

        def torch_actor(o=aopt, a=actors[1]):
            o.step()
            da_t.load_parameters(a.tensors())

        res["actor"] = measure({"device": device_actor, "torch": torch_actor, "torch_fused": lambda: torch_actor(aopt_fused, actors[2])})
        da.close()
        da_t.close()
        widths[str(H)] = res

    three = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True)
    learners = {}
    for label, options in (("three_options", three), ("four_options", dict(three, device_optimizer=True))):
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, **options)
        replay = DeviceReplay(env, 4)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0])

    def one_update(label):
        learner, replay, draw = learners[label]
        draw[0] += 1
        learner.update(replay, 1, draw[0])

    for label in learners:
        for _ in range(5):
            one_update(label)
    wdw = {label: [] for label in learners}
    for _ in range(args.windows):
        for label in learners:
            wdw[label].append(window(lambda: one_update(label), 20))
    updates = {label: {"us_median": float(np.median(v)), "us_windows": [round(x, 2) for x in v]} for label, v in wdw.items()}
    for learner, _, _ in learners.values():
        learner.close()
    result = {"tool": "bench_policy_rollout --optimizer", "env": args.env, "windows": args.windows, "launches_per_window": args.launches,
              "device": torch.cuda.get_device_name(0), "hidden_width": widths,
              "not_slower_than_torch": all(r["not_slower_than_torch"] for w in widths.values() for r in w.values()),
              "learner_update_batch256": updates}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def entropy_mode(args):
    """--entropy: SACLearner.update at batch 256 with device_optimizer only against the same plus device_entropy, at H = 256 and 512,
    alternating windows in one process, medians of wall time per update (each window ends in a synchronise)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd._native import NativeError
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches  # an update does not depend on the number of envs
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    four = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True)
    widths = {}
    for H in (256, 512):
        learners = {}
        try:
            for label, options in (("device_optimizer", four), ("device_entropy", dict(four, device_entropy=True))):
                learner = SACLearner(env, seed=0, batch_size=256, hidden_width=H, **options)
                replay = DeviceReplay(env, 4)
                learners[label] = (learner, replay, [0])
                learner.collect(replay, 4)
        except NativeError as e:  # the gradient kernels the options need are built for hidden widths up to 256
            for learner, _, _ in learners.values():
                learner.close()
            widths[str(H)] = {"refused": str(e)}
            continue

        def one_update(label):
            learner, replay, draw = learners[label]
            draw[0] += 1
            learner.update(replay, 1, draw[0])

        def window(label):
            sync()
            t0 = time.perf_counter()
            for _ in range(per_window):
                one_update(label)
            sync()
            return (time.perf_counter() - t0) * 1e6 / per_window

        for label in learners:
            for _ in range(10):
                one_update(label)
        wdw = {label: [] for label in learners}
        for _ in range(args.windows):
            for label in learners:
                wdw[label].append(window(label))
        med = {k: float(np.median(v)) for k, v in wdw.items()}
        spread = float(max(wdw["device_optimizer"]) - min(wdw["device_optimizer"]))
        widths[str(H)] = {"us_median": med, "us_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()},
                          "device_optimizer_us_spread": spread, "ratio_entropy_over_optimizer": med["device_entropy"] / med["device_optimizer"],
                          "not_slower": med["device_entropy"] <= med["device_optimizer"] + spread}
        for learner, _, _ in learners.values():
            learner.close()
    result = {"tool": "bench_policy_rollout --entropy", "env": args.env, "windows": args.windows, "updates_per_window": per_window,
              "batch": 256, "device": torch.cuda.get_device_name(0), "hidden_width": widths,
              "not_slower": all(w.get("not_slower", True) for w in widths.values())}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def clip_mode(args):
    """--clip: the update without and with max_grad_norm, as update() calls and as one native call per window (see above)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches  # an update does not depend on the number of envs
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    routes = {"device_entropy": (False, {}), "clipped": (False, dict(max_grad_norm=args.max_grad_norm)),
              "native": (True, {}), "native_clipped": (True, dict(max_grad_norm=args.max_grad_norm))}
    if args.clip_only:
        routes = {"native_clipped": routes["native_clipped"]}
    learners = {}
    for label, (native, extra) in routes.items():
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options, **extra)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0], native)

    def updates(label, count):
        learner, replay, draw, native = learners[label]
        if native:
            learner.train(replay, 1, 0, count, seed=1, first_draw=draw[0] + 1)
            draw[0] += count
        else:
            for _ in range(count):
                draw[0] += 1
                learner.update(replay, 1, draw[0])

    def window(label):
        sync()
        t0 = time.perf_counter()
        updates(label, per_window)
        sync()
        return (time.perf_counter() - t0) * 1e6 / per_window

    for label in learners:
        updates(label, 10)
    if args.clip_only:
        for _ in range(args.windows):
            updates("native_clipped", per_window)
        sync()
        print(json.dumps({"tool": "bench_policy_rollout --clip --clip-only", "updates": args.windows * per_window}))
    else:
        wdw = {label: [] for label in learners}
        for _ in range(args.windows):
            for label in learners:
                wdw[label].append(window(label))
        med = {k: float(np.median(v)) for k, v in wdw.items()}
        last = learners["clipped"][0].last_update
        result = {"tool": "bench_policy_rollout --clip", "env": args.env, "num_envs": n, "windows": args.windows, "updates_per_window": per_window,
                  "batch": 256, "hidden_width": 256, "max_grad_norm": args.max_grad_norm, "device": torch.cuda.get_device_name(0),
                  "us_per_update_median": med, "us_per_update_min": {k: float(min(v)) for k, v in wdw.items()},
                  "us_per_update_max": {k: float(max(v)) for k, v in wdw.items()},
                  "us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()},
                  "device_entropy_us_spread": float(max(wdw["device_entropy"]) - min(wdw["device_entropy"])),
                  "clipped_minus_device_entropy_us": med["clipped"] - med["device_entropy"],
                  "native_clipped_minus_native_us": med["native_clipped"] - med["native"],
                  "last_update": {k: float(last[k][0]) for k in ("critic_grad_norm", "actor_grad_norm", "critic_scale", "actor_scale")}}
        line = json.dumps(result)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    for learner, _, _, _ in learners.values():
        learner.close()
    env.close()


def clone_mode(args):
    """--clone: urgym_sac_policy_terms against urgym_sac_policy_terms_cloned at two batch sizes, and the update without and with the option
    (see above)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    launch = {}
    for M in (256, 65536):
        rng = np.random.default_rng(M)
        t = {k: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
             for k, shape in dict(dqmin_da=(M, 6), q=(2, M), y=(M,), log_prob=(M,), q_min=(M,), action_pi=(M, 6), action_data=(M, 6)).items()}
        t["action_pi"], t["action_data"] = torch.tanh(t["action_pi"]), torch.tanh(t["action_data"])
        out = {k: torch.zeros(shape, dtype=torch.float32, device=dev) for k, shape in dict(d_action=(M, 6), critic_loss=(1,), actor_loss=(1,), bc_loss=(1,), bc_weight=(1,)).items()}
        out["bc_rows"], ent_coef = torch.zeros((1,), dtype=torch.int32, device=dev), torch.full((1,), 0.2, dtype=torch.float32, device=dev)
        common = dict(dqmin_da=t["dqmin_da"], scale=-1.0 / M, d_action_out=out["d_action"], q=t["q"], y=t["y"], critic_loss_out=out["critic_loss"],
                      log_prob=t["log_prob"], q_min=t["q_min"], actor_loss_out=out["actor_loss"])
        calls = {"policy_terms": lambda: env.policy_terms(ent_coef, M, **common),
                 "policy_terms_cloned": lambda: env.policy_terms_cloned(ent_coef, M, **common, action_pi=t["action_pi"], action_data=t["action_data"], weight=1.0,
                                                                       bc_scale=1.0 / M, scale_by_q=True, q_filter=True, bc_loss_out=out["bc_loss"],
                                                                       bc_weight_out=out["bc_weight"], bc_rows_out=out["bc_rows"])}

        def window(call):
            first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            t0 = time.perf_counter()
            first.record()
            for _ in range(per_window):
                call()
            last.record()
            sync()
            return first.elapsed_time(last) * 1e3 / per_window, (time.perf_counter() - t0) * 1e6 / per_window

        for call in calls.values():
            for _ in range(20):
                call()
        wdw = {k: [] for k in calls}
        for _ in range(args.windows):
            for k, call in calls.items():
                wdw[k].append(window(call))
        sync()
        med = {k: float(np.median([w[0] for w in v])) for k, v in wdw.items()}
        launch[str(M)] = {"us_per_launch_device_events_median": med, "us_per_launch_wall_median": {k: float(np.median([w[1] for w in v])) for k, v in wdw.items()},
                          "us_per_launch_device_events_min": {k: float(min(w[0] for w in v)) for k, v in wdw.items()},
                          "us_per_launch_device_events_max": {k: float(max(w[0] for w in v)) for k, v in wdw.items()},
                          "cloned_minus_plain_us": med["policy_terms_cloned"] - med["policy_terms"], "cloned_rows": int(out["bc_rows"].item())}

    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    bc = dict(bc_weight=1.0, bc_scale_by_q=True, bc_q_filter=True)
    routes = {"device_entropy": (False, {}), "cloned": (False, bc), "native": (True, {}), "native_cloned": (True, bc)}
    learners = {}
    for label, (native, extra) in routes.items():
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options, **extra)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0], native)

    def updates(label, count):
        learner, replay, draw, native = learners[label]
        if native:
            learner.train(replay, 1, 0, count, seed=1, first_draw=draw[0] + 1)
            draw[0] += count
        else:
            for _ in range(count):
                draw[0] += 1
                learner.update(replay, 1, draw[0])

    def update_window(label):
        sync()
        t0 = time.perf_counter()
        updates(label, per_window)
        sync()
        return (time.perf_counter() - t0) * 1e6 / per_window

    for label in learners:
        updates(label, 10)
    wdw = {label: [] for label in learners}
    for _ in range(args.windows):
        for label in learners:
            wdw[label].append(update_window(label))
    med = {k: float(np.median(v)) for k, v in wdw.items()}
    last = learners["cloned"][0].last_update
    result = {"tool": "bench_policy_rollout --clone", "env": args.env, "num_envs": n, "windows": args.windows, "launches_per_window": per_window,
              "device": torch.cuda.get_device_name(0), "launch": launch, "update": {
                  "batch": 256, "hidden_width": 256, "options": bc, "us_per_update_median": med, "us_per_update_min": {k: float(min(v)) for k, v in wdw.items()},
                  "us_per_update_max": {k: float(max(v)) for k, v in wdw.items()}, "us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()},
                  "cloned_minus_device_entropy_us": med["cloned"] - med["device_entropy"], "native_cloned_minus_native_us": med["native_cloned"] - med["native"],
                  "last_update": {"bc_loss": float(last["bc_loss"][0]), "bc_weight": float(last["bc_weight"][0]), "bc_rows": int(last["bc_rows"][0])}}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for learner, _, _, _ in learners.values():
        learner.close()
    env.close()


def clone_weighted_mode(args):
    """--clone-weighted: urgym_sac_policy_terms_cloned against urgym_sac_policy_terms_weighted at two batch sizes, and the native update
    without cloning, with plain cloning and with the advantage weight (see above).  Every set alternates in one process."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731

    def window(call):
        first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        first.record()
        for _ in range(per_window):
            call()
        last.record()
        sync()
        return first.elapsed_time(last) * 1e3 / per_window

    launch = {}
    for M in (256, 65536):
        rng = np.random.default_rng(M)
        t = {k: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
             for k, shape in dict(dqmin_da=(M, 6), q=(2, M), y=(M,), log_prob=(M,), q_min=(M,), action_pi=(M, 6), action_data=(M, 6)).items()}
        t["action_pi"], t["action_data"] = torch.tanh(t["action_pi"]), torch.tanh(t["action_data"])
        out = {k: torch.zeros(shape, dtype=torch.float32, device=dev)
               for k, shape in dict(d_action=(M, 6), critic_loss=(1,), actor_loss=(1,), bc_loss=(1,), bc_weight=(1,), adv_ess=(1,), adv_max=(1,)).items()}
        out["bc_rows"], out["adv_clipped"] = torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
        ent_coef = torch.full((1,), 0.2, dtype=torch.float32, device=dev)
        kw = dict(dqmin_da=t["dqmin_da"], scale=-1.0 / M, d_action_out=out["d_action"], q=t["q"], y=t["y"], critic_loss_out=out["critic_loss"], log_prob=t["log_prob"],
                  q_min=t["q_min"], actor_loss_out=out["actor_loss"], action_pi=t["action_pi"], action_data=t["action_data"], weight=1.0, bc_scale=1.0 / M, scale_by_q=True,
                  bc_loss_out=out["bc_loss"], bc_weight_out=out["bc_weight"], bc_rows_out=out["bc_rows"])
        calls = {"policy_terms_cloned": lambda: env.policy_terms_cloned(ent_coef, M, q_filter=False, **kw),
                 "policy_terms_weighted": lambda: env.policy_terms_weighted(ent_coef, M, temperature=1.0, max_weight=20.0, adv_ess_out=out["adv_ess"], adv_max_out=out["adv_max"],
                                                                           adv_clipped_out=out["adv_clipped"], **kw)}
        for call in calls.values():
            for _ in range(20):
                call()
        wdw = {k: [] for k in calls}
        for _ in range(args.windows):
            for k, call in calls.items():
                wdw[k].append(window(call))
        sync()
        med = {k: float(np.median(v)) for k, v in wdw.items()}
        launch[str(M)] = {"us_per_launch_device_events_median": med, "us_per_launch_device_events_min": {k: float(min(v)) for k, v in wdw.items()},
                          "us_per_launch_device_events_max": {k: float(max(v)) for k, v in wdw.items()},
                          "weighted_minus_cloned_us": med["policy_terms_weighted"] - med["policy_terms_cloned"],
                          "weighted_over_cloned": med["policy_terms_weighted"] / med["policy_terms_cloned"], "adv_ess": float(out["adv_ess"].item()),
                          "adv_max": float(out["adv_max"].item()), "adv_clipped": int(out["adv_clipped"].item()), "rows": int(out["bc_rows"].item())}

    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    bc = dict(bc_weight=1.0, bc_scale_by_q=True)
    routes = {"native": {}, "native_cloned": bc, "native_weighted": dict(bc, bc_advantage_temperature=1.0, bc_advantage_max_weight=20.0)}
    learners = {}
    for label, extra in routes.items():
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options, **extra)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0])

    def updates(label, count):
        learner, replay, draw = learners[label]
        learner.train(replay, 1, 0, count, seed=1, first_draw=draw[0] + 1)
        draw[0] += count

    def update_window(label):
        sync()
        t0 = time.perf_counter()
        updates(label, per_window)
        sync()
        return (time.perf_counter() - t0) * 1e6 / per_window

    for label in learners:
        updates(label, 10)
    wdw = {label: [] for label in learners}
    for _ in range(args.windows):
        for label in learners:
            wdw[label].append(update_window(label))
    med = {k: float(np.median(v)) for k, v in wdw.items()}
    last = learners["native_weighted"][0].last_update
    result = {"tool": "bench_policy_rollout --clone-weighted", "env": args.env, "num_envs": n, "windows": args.windows, "launches_per_window": per_window,
              "device": torch.cuda.get_device_name(0), "launch": launch, "update": {
                  "batch": 256, "hidden_width": 256, "options": routes["native_weighted"], "us_per_update_median": med,
                  "us_per_update_min": {k: float(min(v)) for k, v in wdw.items()}, "us_per_update_max": {k: float(max(v)) for k, v in wdw.items()},
                  "us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()},
                  "native_weighted_minus_native_cloned_us": med["native_weighted"] - med["native_cloned"],
                  "native_cloned_minus_native_us": med["native_cloned"] - med["native"],
                  "last_update": {"bc_loss": float(last["bc_loss"][0]), "bc_weight": float(last["bc_weight"][0]), "bc_rows": int(last["bc_rows"][0]),
                                  "adv_ess": float(last["adv_ess"][0]), "adv_max": float(last["adv_max"][0]), "adv_clipped": int(last["adv_clipped"][0])}}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for learner, _, _ in learners.values():
        learner.close()
    env.close()


def demos_mode(args):
    """--demos: the mixed gather beside urgym_replay_sample and the masked terms beside urgym_sac_policy_terms_cloned at two batch sizes, and
    the update without and with a demonstration ring (see above).  Every pair alternates in one process."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    env_d = make_vec(args.env, num_envs=max(1, n // 8), device=dev, seed=1, auto_reset=True)
    env_d.reset(seed=1)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    filler = SACLearner(env_d, seed=2, batch_size=256, hidden_width=256, learning_starts=0, **options)
    demos = DeviceReplay(env_d, 64)
    filler.collect(demos, 64)  # the ring's content does not matter to a time: a policy fills it
    own = DeviceReplay(env, 64)
    plain_learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options)
    plain_learner.collect(own, 64)

    def windows(calls):
        def window(call):
            first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            t0 = time.perf_counter()
            first.record()
            for _ in range(per_window):
                call()
            last.record()
            sync()
            return first.elapsed_time(last) * 1e3 / per_window, (time.perf_counter() - t0) * 1e6 / per_window

        for call in calls.values():
            for _ in range(20):
                call()
        wdw = {k: [] for k in calls}
        for _ in range(args.windows):
            for k, call in calls.items():
                wdw[k].append(window(call))
        sync()
        return {"us_per_launch_device_events_median": {k: float(np.median([w[0] for w in v])) for k, v in wdw.items()},
                "us_per_launch_wall_median": {k: float(np.median([w[1] for w in v])) for k, v in wdw.items()},
                "us_per_launch_device_events_min": {k: float(min(w[0] for w in v)) for k, v in wdw.items()},
                "us_per_launch_device_events_max": {k: float(max(w[0] for w in v)) for k, v in wdw.items()}}

    gather, terms = {}, {}
    for M in (256, 65536):
        D, draw = M // 2, [0]
        batch = own.sample(M, 0, 0, demonstrations=(demos, D))  # the tensors both gathers write
        flat = {**batch["observations"], **{"next_" + k: v for k, v in batch["next_observations"].items()}, "action": batch["actions"], "reward": batch["rewards"],
                "terminated": batch["terminated"], "truncated": batch["truncated"], "is_success": batch["is_success"], "index": batch["index"]}

        def sample(**more):
            draw[0] += 1
            own.sample_into(dict(flat, **({"source": batch["source"]} if more else {})), 1, draw[0], **more)

        got = windows({"replay_sample": sample, "replay_sample_mixed": lambda: sample(demonstrations=(demos, D))})
        med = got["us_per_launch_device_events_median"]
        gather[str(M)] = dict(got, demo_rows=D, mixed_minus_plain_us=med["replay_sample_mixed"] - med["replay_sample"])

        rng = np.random.default_rng(M)
        t = {k: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
             for k, shape in dict(dqmin_da=(M, 6), q=(2, M), y=(M,), log_prob=(M,), q_min=(M,), action_pi=(M, 6), action_data=(M, 6)).items()}
        t["action_pi"], t["action_data"] = torch.tanh(t["action_pi"]), torch.tanh(t["action_data"])
        out = {k: torch.zeros(shape, dtype=torch.float32, device=dev) for k, shape in dict(d_action=(M, 6), critic_loss=(1,), actor_loss=(1,), bc_loss=(1,), bc_weight=(1,)).items()}
        out["bc_rows"], ent_coef = torch.zeros((1,), dtype=torch.int32, device=dev), torch.full((1,), 0.2, dtype=torch.float32, device=dev)
        mask = (torch.arange(M, device=dev) < D).to(torch.uint8)
        kw = dict(dqmin_da=t["dqmin_da"], scale=-1.0 / M, d_action_out=out["d_action"], q=t["q"], y=t["y"], critic_loss_out=out["critic_loss"], log_prob=t["log_prob"],
                  q_min=t["q_min"], actor_loss_out=out["actor_loss"], action_pi=t["action_pi"], action_data=t["action_data"], weight=1.0, bc_scale=1.0 / M, scale_by_q=True,
                  q_filter=True, bc_loss_out=out["bc_loss"], bc_weight_out=out["bc_weight"], bc_rows_out=out["bc_rows"])
        got = windows({"policy_terms_cloned": lambda: env.policy_terms_cloned(ent_coef, M, **kw),
                       "policy_terms_cloned_masked": lambda: env.policy_terms_cloned_masked(ent_coef, M, row_mask=mask, **kw)})
        med = got["us_per_launch_device_events_median"]
        terms[str(M)] = dict(got, masked_rows=D, cloned_rows=int(out["bc_rows"].item()), masked_minus_cloned_us=med["policy_terms_cloned_masked"] - med["policy_terms_cloned"])

    bc = dict(bc_weight=1.0, bc_scale_by_q=True, bc_q_filter=True)
    demo = dict(demonstrations=demos, demo_batch_size=128)
    routes = {"native": {}, "native_demo": demo, "native_cloned": bc, "native_demo_cloned_demo_only": dict(bc, bc_demo_only=True, **demo)}
    learners = {}
    for label, extra in routes.items():
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options, **extra)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0])

    def updates(label, count):
        learner, replay, draw = learners[label]
        learner.train(replay, 1, 0, count, seed=1, first_draw=draw[0] + 1)
        draw[0] += count

    def update_window(label):
        sync()
        t0 = time.perf_counter()
        updates(label, per_window)
        sync()
        return (time.perf_counter() - t0) * 1e6 / per_window

    for label in learners:
        updates(label, 10)
    wdw = {label: [] for label in learners}
    for _ in range(args.windows):
        for label in learners:
            wdw[label].append(update_window(label))
    med = {k: float(np.median(v)) for k, v in wdw.items()}
    result = {"tool": "bench_policy_rollout --demos", "env": args.env, "num_envs": n, "demo_envs": env_d.num_envs, "windows": args.windows, "launches_per_window": per_window,
              "device": torch.cuda.get_device_name(0), "gather": gather, "terms": terms, "update": {
                  "batch": 256, "demo_batch_size": 128, "hidden_width": 256, "us_per_update_median": med, "us_per_update_min": {k: float(min(v)) for k, v in wdw.items()},
                  "us_per_update_max": {k: float(max(v)) for k, v in wdw.items()}, "us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()},
                  "native_demo_minus_native_us": med["native_demo"] - med["native"],
                  "native_demo_cloned_demo_only_minus_native_cloned_us": med["native_demo_cloned_demo_only"] - med["native_cloned"]}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for learner, _, _ in learners.values():
        learner.close()
    filler.close(), plain_learner.close()
    env_d.close(), env.close()


def normalize_mode(args):
    """--normalize: the update without and with normalize, the collection step without and with the normalize launch, the fold (see above)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceNormalizer, DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches  # an update does not depend on the number of envs
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    routes = {"device_entropy": (False, {}), "normalized": (False, dict(normalize=True)), "native": (True, {}), "native_normalized": (True, dict(normalize=True))}
    if args.normalize_only:
        routes = {"native_normalized": routes["native_normalized"]}
    learners = {}
    for label, (native, extra) in routes.items():
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options, **extra)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0], native)

    def updates(label, count):
        learner, replay, draw, native = learners[label]
        if native:
            learner.train(replay, 1, 0, count, seed=1, first_draw=draw[0] + 1)
            draw[0] += count
        else:
            for _ in range(count):
                draw[0] += 1
                learner.update(replay, 1, draw[0])

    def window(label):
        sync()
        t0 = time.perf_counter()
        updates(label, per_window)
        sync()
        return (time.perf_counter() - t0) * 1e6 / per_window

    for label in learners:
        updates(label, 10)
    wdw = {label: [] for label in learners}
    for _ in range(args.windows):
        for label in learners:
            if args.normalize_only:
                updates(label, per_window)
            else:
                wdw[label].append(window(label))
    sync()
    # the collection and the fold at the full env count, on an environment of their own
    K = args.collect_steps
    big = make_vec(args.env, num_envs=args.num_envs, device=dev, seed=0, auto_reset=True)
    big.reset(seed=0)
    from ur_gym_amd.evaluation import DeviceActor
    from ur_gym_amd.training import host_arrays

    big_actor = DeviceActor(host_arrays(learners[next(iter(learners))][0].actor.tensors()), big)
    ring, nz = DeviceReplay(big, K), DeviceNormalizer(big, fold_steps=K)
    how = dict(mode="gaussian", seed=3, first_draw=0)

    def timed(fn):
        torch.cuda.synchronize(big.device)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(big.device)
        return (time.perf_counter() - t0) * 1e6

    plain = lambda: big.collect(big_actor, K, ring, sample=how, first_slot=0)  # noqa: E731
    normed = lambda: big.collect(big_actor, K, ring, sample=how, first_slot=0, normalizer=nz)  # noqa: E731
    fold = lambda: nz.fold(ring, 0, K)  # noqa: E731
    for fn in (plain, normed, fold):
        fn()
    cw = {"collect": [], "collect_normalized": [], "fold": []}
    for _ in range(args.windows):
        if not args.normalize_only:
            cw["collect"].append(timed(plain) / K)
        cw["collect_normalized"].append(timed(normed) / K)
        cw["fold"].append(timed(fold))
    if args.normalize_only:
        print(json.dumps({"tool": "bench_policy_rollout --normalize --normalize-only", "updates": args.windows * per_window, "collect_steps": args.windows * K}))
    else:
        med = {k: float(np.median(v)) for k, v in wdw.items()}
        cmed = {k: float(np.median(v)) for k, v in cw.items()}
        result = {"tool": "bench_policy_rollout --normalize", "env": args.env, "num_envs_update": n, "num_envs_collect": args.num_envs, "windows": args.windows,
                  "updates_per_window": per_window, "batch": 256, "hidden_width": 256, "collect_steps": K, "device": torch.cuda.get_device_name(0),
                  "us_per_update_median": med, "us_per_update_min": {k: float(min(v)) for k, v in wdw.items()},
                  "us_per_update_max": {k: float(max(v)) for k, v in wdw.items()},
                  "us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()},
                  "device_entropy_us_spread": float(max(wdw["device_entropy"]) - min(wdw["device_entropy"])),
                  "normalized_minus_device_entropy_us": med["normalized"] - med["device_entropy"],
                  "native_normalized_minus_native_us": med["native_normalized"] - med["native"],
                  "us_per_collect_step_median": {k: cmed[k] for k in ("collect", "collect_normalized")},
                  "us_per_collect_step_windows": {k: [round(x, 2) for x in cw[k]] for k in ("collect", "collect_normalized")},
                  "us_per_fold_median": cmed["fold"], "us_per_fold_windows": [round(x, 2) for x in cw["fold"]], "us_per_fold_per_step": cmed["fold"] / K}
        line = json.dumps(result)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    big_actor.close()
    big.close()
    for learner, _, _, _ in learners.values():
        learner.close()
    env.close()


def native_mode(args):
    """--native: the thirteen-call SACLearner.update against SACLearner.train, one native call per window (see above)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, per_window = "cuda:0", min(args.num_envs, 4096), args.launches  # an update does not depend on the number of envs
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    learners = {}
    for label in ("thirteen_calls", "native"):
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        learners[label] = (learner, replay, [0])

    def updates(label, count):
        learner, replay, draw = learners[label]
        if label == "native":
            learner.train(replay, 1, 0, count, seed=1, first_draw=draw[0] + 1)
            draw[0] += count
        else:
            for _ in range(count):
                draw[0] += 1
                learner.update(replay, 1, draw[0])

    def loop(label, iterations, per_step=4):
        learner, replay, draw = learners[label]
        if label == "native":
            learner.train(replay, iterations, 1, per_step, seed=1, first_draw=draw[0] + 1)
            draw[0] += iterations * per_step
        else:
            for _ in range(iterations):
                learner.collect(replay, 1)
                for _ in range(per_step):
                    draw[0] += 1
                    learner.update(replay, 1, draw[0])

    def window(fn, label, count, per_update):
        sync()
        t0 = time.perf_counter()
        fn(label, count)
        sync()
        return (time.perf_counter() - t0) * 1e6 / per_update

    if args.native_only:
        for _ in range(args.windows):
            updates("native", per_window)
        sync()
        print(json.dumps({"tool": "bench_policy_rollout --native --native-only", "updates": args.windows * per_window}))
        for learner, _, _ in learners.values():
            learner.close()
        env.close()
        return
    pairs = {}
    for pair, fn, count in (("updates", updates, per_window), ("loop", loop, max(1, per_window // 4))):
        per_update = count if pair == "updates" else count * 4
        for label in learners:
            fn(label, 10 if pair == "updates" else 3)
        wdw = {label: [] for label in learners}
        for _ in range(args.windows):
            for label in learners:
                wdw[label].append(window(fn, label, count, per_update))
        med = {k: float(np.median(v)) for k, v in wdw.items()}
        spread = float(max(wdw["thirteen_calls"]) - min(wdw["thirteen_calls"]))
        pairs[pair] = {"us_per_update_median": med, "us_per_update_min": {k: float(min(v)) for k, v in wdw.items()},
                       "us_per_update_max": {k: float(max(v)) for k, v in wdw.items()},
                       "us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wdw.items()}, "thirteen_calls_us_spread": spread,
                       "ratio_native_over_thirteen_calls": med["native"] / med["thirteen_calls"],
                       "not_slower": med["native"] <= med["thirteen_calls"] + spread}
    pairs["loop"]["collection_steps_per_window"] = max(1, per_window // 4)
    pairs["loop"]["updates_per_collection_step"] = 4
    result = {"tool": "bench_policy_rollout --native", "env": args.env, "num_envs": n, "windows": args.windows, "updates_per_window": per_window,
              "batch": 256, "hidden_width": 256, "device": torch.cuda.get_device_name(0), **pairs, "not_slower_overall": pairs["updates"]["not_slower"]}
    for learner, _, _ in learners.values():
        learner.close()
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def nstep_mode(args):
    """--nstep: the gather of multi-step returns (urgym_replay_sample_nstep) on a filled ring, in alternating windows in one process:
    at n_steps = 1 against the one-step gather (urgym_replay_sample: the same work but one store per row), at n_steps = 3 and 5 against
    a torch composition of the same batch (index arithmetic, flag gathers, index_select per field); then SACLearner.update and
    SACLearner.train at batch 256, H = 256, with n_steps = 1 and 3."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceActor, DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, cap, kind, gamma = "cuda:0", args.num_envs, args.capacity, ACTOR_NPZ[args.env], 0.95
    w = dict(np.load(os.path.join(ROOT, "tests", "golden", "actors", f"actor_{kind}.npz")))
    w.update(np.load(os.path.join(ROOT, "tests", "golden", "actors", f"log_std_{kind}.npz")))
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    actor = DeviceActor(w, env)
    replay = DeviceReplay(env, cap)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    done = 0
    while replay.filled < cap:  # a filled ring, from the sampled policy
        steps = min(64, cap - replay.filled)
        replay.collect(actor, steps, sample=dict(mode="gaussian", seed=1, first_draw=done))
        done += steps
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        sync()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / reps

    def alternate(kinds):
        for fn in kinds.values():
            for _ in range(10):
                fn()
        wins = {k: [] for k in kinds}
        for _ in range(args.windows):
            for name, fn in kinds.items():
                wins[name].append(window(fn, args.launches))
        return wins, {k: float(np.median(v)) for k, v in wins.items()}

    size, oldest, filled = replay.filled * n, replay.oldest_slot, replay.filled
    flat = {name: t.reshape((cap * n,) + tuple(t.shape[2:])) for name, t in replay.ring.items()}
    first_fields = ("observation", "achieved_goal", "desired_goal", "action")
    last_fields = ("next_observation", "next_achieved_goal", "next_desired_goal", "terminated", "truncated", "is_success")
    gather = {}
    for B in (256, 65536):
        out = {name: torch.empty((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for name, t in flat.items()}
        one = dict(out, index=torch.empty((B,), dtype=torch.int64, device=dev))
        multi = dict(one, discount=torch.empty((B,), dtype=torch.float32, device=dev), steps=torch.empty((B,), dtype=torch.int32, device=dev),
                     last_index=torch.empty((B,), dtype=torch.int64, device=dev))
        tick = [0]

        def one_step():
            tick[0] += 1
            replay.sample_into(one, 3, tick[0])

        def nstep(steps, into=multi):
            def fn():
                tick[0] += 1
                replay.sample_into(into, 3, tick[0], n_steps=steps, gamma=gamma)
            return fn

        def torch_nstep(steps):
            k = torch.arange(steps, device=dev)
            powers = torch.tensor([gamma ** i for i in range(steps + 1)], dtype=torch.float32, device=dev)

            def fn():
                e = torch.randint(0, size, (B,), device=dev)
                p, envi = e // n, e % n
                L = torch.clamp(filled - p, max=steps)
                entries = ((oldest + p[:, None] + k[None, :]) % cap) * n + envi[:, None]
                valid = k[None, :] < L[:, None]
                entries = torch.where(valid, entries, entries[:, :1])
                ends = ((flat["terminated"][entries] | flat["truncated"][entries]) != 0) & valid
                m = torch.minimum(torch.where(ends.any(1), ends.int().argmax(1) + 1, L), L)
                taken = k[None, :] < m[:, None]
                torch.sum(torch.where(taken, flat["reward"][entries], 0.0) * powers[None, :steps], 1, out=out["reward"])
                multi["discount"].copy_(powers[m])
                multi["steps"].copy_(m)
                last = entries.gather(1, (m - 1)[:, None])[:, 0]
                multi["index"].copy_(entries[:, 0])
                multi["last_index"].copy_(last)
                for name in first_fields:
                    torch.index_select(flat[name], 0, entries[:, 0], out=out[name])
                for name in last_fields:
                    torch.index_select(flat[name], 0, last, out=out[name])
            return fn

        # the same outputs plus the one required array, discount: the same work plus one store per row
        wins, med = alternate({"one_step_gather": one_step, "nstep_gather_1": nstep(1, dict(one, discount=multi["discount"]))})
        spread = float(max(wins["one_step_gather"]) - min(wins["one_step_gather"]))
        entry = {"n_steps_1": {"us_windows": {k: [round(x, 3) for x in v] for k, v in wins.items()}, "us_median": med, "one_step_us_spread": spread,
                               "difference_us": med["nstep_gather_1"] - med["one_step_gather"],
                               "within_the_one_step_spread": med["nstep_gather_1"] <= med["one_step_gather"] + spread}}
        for steps in (3, 5):
            wins, med = alternate({"device": nstep(steps), "torch": torch_nstep(steps)})
            entry[f"n_steps_{steps}"] = {"us_windows": {k: [round(x, 3) for x in v] for k, v in wins.items()}, "us_median": med,
                                         "not_slower_than_torch": med["device"] <= med["torch"], "speedup_over_torch": med["torch"] / med["device"]}
        gather[str(B)] = entry
        del out, one, multi
    actor.close()

    # the learner: one update and one train window at batch 256, H = 256
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    learners = {}
    for label, steps in (("n_steps_1", 1), ("n_steps_3", 3)):
        learners[label] = (SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, n_steps=steps, **options), [0])

    def updates(label, native):
        learner, draw = learners[label]

        def fn():
            if native:
                learner.train(replay, 1, 0, args.launches, seed=1, first_draw=draw[0] + 1)
                draw[0] += args.launches
            else:
                for _ in range(args.launches):
                    draw[0] += 1
                    learner.update(replay, 1, draw[0])
        return fn

    def host_window(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e6 / args.launches

    learner_result = {}
    for route, native in (("update", False), ("train", True)):
        fns = {label: updates(label, native) for label in learners}
        for fn in fns.values():
            fn()
        wins = {label: [] for label in fns}
        for _ in range(args.windows):
            for label, fn in fns.items():
                wins[label].append(host_window(fn))
        med = {k: float(np.median(v)) for k, v in wins.items()}
        learner_result[route] = {"us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wins.items()}, "us_per_update_median": med,
                                 "n_steps_1_us_spread": float(max(wins["n_steps_1"]) - min(wins["n_steps_1"])),
                                 "n_steps_3_minus_n_steps_1_us": med["n_steps_3"] - med["n_steps_1"]}
    for learner, _ in learners.values():
        learner.close()
    result = {"tool": "bench_policy_rollout --nstep", "env": args.env, "num_envs": n, "capacity_steps": cap, "windows": args.windows,
              "launches_per_window": args.launches, "gamma": gamma, "device": torch.cuda.get_device_name(0), "gather": gather,
              "learner": dict(learner_result, batch=256, hidden_width=256)}
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def prioritized_mode(args):
    """--prioritized: the prioritized update against the uniform one, both as SACLearner.train on the same filled
    ring (a DevicePrioritizedReplay serves both: the uniform learner goes through exactly the calls it always made), H = 256, batch
    65,536 and 4,096, in alternating windows of --launches updates in one native call each, timed on the host around a
    synchronisation.  Then the pieces on their own, timed with events: the uniform gather against the prioritized one (the descent's
    cost per row), and urgym_per_terms with its write-back (one workgroup, then the two repair launches)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DevicePrioritizedReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, cap = "cuda:0", args.num_envs, args.capacity
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    replay = DevicePrioritizedReplay(env, cap)
    filler = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options)
    while replay.filled < cap:  # a filled ring, from the sampled policy; every leaf at max_leaf
        filler.collect(replay, min(64, cap - replay.filled))
    filler.close()
    sync()
    batches = (65536,) if args.prioritized_only else (65536, 4096)
    result = {}
    for M in batches:
        learners = {} if args.prioritized_only else {"uniform": (SACLearner(env, seed=0, batch_size=M, hidden_width=256, learning_starts=0, **options), [0])}
        learners["prioritized"] = (SACLearner(env, seed=0, batch_size=M, hidden_width=256, learning_starts=0, prioritized=True, per_beta_steps=1000, **options), [0])

        def updates(label):
            learner, draw = learners[label]

            def fn():
                learner.train(replay, 1, 0, args.launches, seed=1, first_draw=draw[0] + 1)
                draw[0] += args.launches
            return fn

        def host_window(fn):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            return (time.perf_counter() - t0) * 1e6 / args.launches

        fns = {label: updates(label) for label in learners}
        for fn in fns.values():
            fn()
        wins = {label: [] for label in fns}
        for _ in range(args.windows):
            for label, fn in fns.items():
                wins[label].append(host_window(fn))
        med = {k: float(np.median(v)) for k, v in wins.items()}
        entry = {"us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wins.items()}, "us_per_update_median": med}
        if not args.prioritized_only:
            entry["prioritized_minus_uniform_us"] = med["prioritized"] - med["uniform"]
            entry["uniform_us_spread"] = float(max(wins["uniform"]) - min(wins["uniform"]))
            # the pieces, with events
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def window(fn, reps=args.launches):
                for _ in range(5):
                    fn()
                sync()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                sync()
                return e0.elapsed_time(e1) * 1e3 / reps

            tick = [0]

            def uniform_gather():
                tick[0] += 1
                replay.sample(M, 3, tick[0])

            def prioritized_gather():
                tick[0] += 1
                replay.sample_prioritized(M, 3, tick[0])

            batch = replay.sample_prioritized(M, 3, 1)
            q, y = torch.randn((2, M), device=dev), torch.randn((M,), device=dev)
            out = {}
            pieces = {"uniform_gather_us": [window(uniform_gather) for _ in range(args.windows)],
                      "prioritized_gather_us": [window(prioritized_gather) for _ in range(args.windows)],
                      "per_terms_three_launches_us": [window(lambda: replay.terms(batch, q, y, 0.7, 1.0 / M, out=out)) for _ in range(args.windows)],
                      "per_terms_one_launch_us": [window(lambda: replay.terms(batch, q, y, 0.7, 1.0 / M, write_back=False, out=out)) for _ in range(args.windows)],
                      "fill_one_slot_us": [window(lambda: replay.fill(3, 1)) for _ in range(args.windows)]}
            entry["pieces_us_median"] = {k: float(np.median(v)) for k, v in pieces.items()}
            entry["descent_ns_per_row"] = (entry["pieces_us_median"]["prioritized_gather_us"] - entry["pieces_us_median"]["uniform_gather_us"]) * 1e3 / M
        result[str(M)] = entry
        for learner, _ in learners.values():
            learner.close()
    out = {"tool": "bench_policy_rollout --prioritized", "env": args.env, "num_envs": n, "capacity_steps": cap, "windows": args.windows,
           "launches_per_window": args.launches, "hidden_width": 256, "device": torch.cuda.get_device_name(0), "batch": result}
    env.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def hindsight_mode(args):
    """--hindsight: the update with hindsight relabelling against the uniform one, both as SACLearner.train on the
    same filled ring (the uniform learner goes through exactly the calls it always made), H = 256, batch 65,536 and 4,096, in
    alternating windows of --launches updates in one native call each, timed on the host around a synchronisation.  Then the two
    gathers on their own, timed with events, and what the relabelled batch looks like (the share, the mean window length F).
    --hindsight-only runs only the hindsight updates and gathers (for a kernel trace)."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, cap = "cuda:0", args.num_envs, args.capacity
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    replay = DeviceReplay(env, cap)
    filler = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options)
    while replay.filled < cap:  # a filled ring, from the sampled policy: deep enough that the walks run to the episodes' ends
        filler.collect(replay, min(64, cap - replay.filled))
    filler.close()
    sync()
    result = {}
    for M in (65536, 4096):
        learners = {} if args.hindsight_only else {"uniform": (SACLearner(env, seed=0, batch_size=M, hidden_width=256, learning_starts=0, **options), [0])}
        learners["hindsight"] = (SACLearner(env, seed=0, batch_size=M, hidden_width=256, learning_starts=0, hindsight=True, **options), [0])

        def updates(label):
            learner, draw = learners[label]

            def fn():
                learner.train(replay, 1, 0, args.launches, seed=1, first_draw=draw[0] + 1)
                draw[0] += args.launches
            return fn

        def host_window(fn):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            return (time.perf_counter() - t0) * 1e6 / args.launches

        fns = {label: updates(label) for label in learners}
        for fn in fns.values():
            fn()
        wins = {label: [] for label in fns}
        for _ in range(args.windows):
            for label, fn in fns.items():
                wins[label].append(host_window(fn))
        med = {k: float(np.median(v)) for k, v in wins.items()}
        entry = {"us_per_update_windows": {k: [round(x, 2) for x in v] for k, v in wins.items()}, "us_per_update_median": med}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def window(fn, reps=args.launches):
            for _ in range(5):
                fn()
            sync()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            sync()
            return e0.elapsed_time(e1) * 1e3 / reps

        tick = [0]

        def uniform_gather():
            tick[0] += 1
            replay.sample(M, 3, tick[0])

        def hindsight_gather():
            tick[0] += 1
            replay.sample_hindsight(M, 3, tick[0])

        pieces = {"hindsight_gather_us": [window(hindsight_gather) for _ in range(args.windows)]}
        if not args.hindsight_only:
            entry["hindsight_minus_uniform_us"] = med["hindsight"] - med["uniform"]
            entry["uniform_us_spread"] = float(max(wins["uniform"]) - min(wins["uniform"]))
            pieces["uniform_gather_us"] = [window(uniform_gather) for _ in range(args.windows)]
        entry["pieces_us_median"] = {k: float(np.median(v)) for k, v in pieces.items()}
        batch = replay.sample_hindsight(M, 3, 1)
        sync()
        g, e = batch["goal_index"], batch["index"]
        rel = g >= 0
        ahead = ((g // n - e // n) % cap)[rel].double()
        entry["relabelled_share"] = float(rel.double().mean())
        entry["mean_steps_to_the_goal"] = float(ahead.mean())  # FUTURE: about half the mean window length F
        entry["new_successes"] = int((batch["is_success"] & rel).sum())
        result[str(M)] = entry
        for learner, _ in learners.values():
            learner.close()
    out = {"tool": "bench_policy_rollout --hindsight", "env": args.env, "num_envs": n, "capacity_steps": cap, "windows": args.windows,
           "launches_per_window": args.launches, "hidden_width": 256, "horizon": int(env.cfg.max_episode_steps), "device": torch.cuda.get_device_name(0), "batch": result}
    env.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def evaluate_mode(args):
    """--evaluate: the evaluation inside the training call.  (1) ONE evaluation of 1024 envs x 100 steps ending in
    a synchronise: DeviceEvaluation.evaluate + results against the route before it, load_parameters + reset(seed) +
    run_closed_loop_device, in alternating windows.  (2) a training run with an evaluation every E updates: ONE
    SACLearner.train(..., evaluation=, eval_every=E) call against one train call per interval plus the Python evaluation."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceActor, DeviceEvaluation, DeviceReplay, run_closed_loop_device
    from ur_gym_amd.training import SACLearner, host_arrays

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, eval_n, K, E, per_step = "cuda:0", min(args.num_envs, 4096), 1024, 100, 40, 4
    iterations = max(1, args.launches // per_step)  # --launches updates per window, as --native counts them
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    sides = {}
    for label in ("python_evaluate", "native"):
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        test_env = make_vec(args.env, num_envs=eval_n, device=dev, seed=1, auto_reset=False)
        side = dict(learner=learner, replay=replay, test_env=test_env, draw=0)
        if label == "native":
            side["ev"] = DeviceEvaluation(test_env, learner.actor.tensors(), num_steps=K, seed=1, capacity=max(8, iterations * per_step // E + 2))
        else:
            side["actor"] = DeviceActor(host_arrays(learner.actor.tensors()), test_env)
        sides[label] = side

    def evaluate(label):
        sd = sides[label]
        if label == "native":
            sd["ev"].count = 0
            sd["ev"].evaluate(sd["learner"].actor.tensors())
            return sd["ev"].results()[0]["mean_return"]  # synchronises, reads the record
        sd["actor"].load_parameters(sd["learner"].actor.tensors())  # tools/train_sac.py's evaluate() before this call existed
        sd["test_env"].reset(seed=1)
        return run_closed_loop_device(sd["test_env"], sd["actor"], K)["mean_episode_reward"]

    def run(label):
        sd = sides[label]
        learner, replay = sd["learner"], sd["replay"]
        if label == "native":
            sd["ev"].count = 0
            learner.train(replay, iterations, 1, per_step, seed=1, first_draw=sd["draw"] + 1, evaluation=sd["ev"], eval_every=E)
            sd["draw"] += iterations * per_step
            return [r["mean_return"] for r in sd["ev"].results()]
        out, left = [], iterations
        while left > 0:  # one native call per interval, then the Python evaluation: tools/train_sac.py --native before this call existed
            step = learner.adam_state["step"]
            trips = min(left, -(-(E - step % E) // per_step))
            learner.train(replay, trips, 1, per_step, seed=1, first_draw=sd["draw"] + 1)
            sd["draw"] += trips * per_step
            left -= trips
            if learner.adam_state["step"] // E > step // E:
                out.append(evaluate(label))
        sync()
        return out

    def window(fn, label):
        sync()
        t0 = time.perf_counter()
        got = fn(label)
        sync()
        return (time.perf_counter() - t0) * 1e3, got

    result = {"tool": "bench_policy_rollout --evaluate", "env": args.env, "num_envs": n, "eval_envs": eval_n, "eval_steps": K, "windows": args.windows,
              "batch": 256, "hidden_width": 256, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("one_evaluation", evaluate), ("training_run", run)):
        for label in sides:
            fn(label), fn(label)
        wdw, evaluations = {label: [] for label in sides}, {}
        for _ in range(args.windows):
            for label in sides:
                ms, got = window(fn, label)
                wdw[label].append(ms)
                evaluations[label] = len(got) if isinstance(got, list) else 1
        med = {k: float(np.median(v)) for k, v in wdw.items()}
        spread = float(max(wdw["python_evaluate"]) - min(wdw["python_evaluate"]))
        result[name] = {"ms_median": med, "ms_min": {k: float(min(v)) for k, v in wdw.items()}, "ms_max": {k: float(max(v)) for k, v in wdw.items()},
                        "ms_windows": {k: [round(x, 3) for x in v] for k, v in wdw.items()}, "python_evaluate_ms_spread": spread,
                        "ratio_native_over_python_evaluate": med["native"] / med["python_evaluate"], "evaluations_per_window": evaluations,
                        "not_slower": med["native"] <= med["python_evaluate"] + spread}
    result["training_run"].update(iterations_per_window=iterations, updates_per_iteration=per_step, eval_every=E)
    for sd in sides.values():
        (sd.get("ev") or sd.get("actor")).close()
        sd["learner"].close()
        sd["test_env"].close()
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def monitor_mode(args):
    """--monitor: what the training-episode statistics cost inside the training call.  --launches updates as
    --launches / 4 x (1 step, 4 updates) in ONE SACLearner.train call, without a monitor and with ``monitor=, log_every=10`` (one fold
    launch per iteration, one stats launch per ten), in alternating windows of one process, each ending in a synchronise."""
    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceMonitor, DeviceReplay
    from ur_gym_amd.training import SACLearner

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev, n, E, per_step = "cuda:0", min(args.num_envs, 4096), 10, 4
    iterations = max(1, args.launches // per_step)  # --launches updates per window, as --native counts them
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    sync = lambda: torch.cuda.synchronize(env.device)  # noqa: E731
    options = dict(device_action_gradient=True, device_critic_gradient=True, device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    sides = {}
    for label in ("plain", "monitored")[1 if args.monitored_only else 0:]:
        learner = SACLearner(env, seed=0, batch_size=256, hidden_width=256, learning_starts=0, **options)
        replay = DeviceReplay(env, 64)
        learner.collect(replay, 4)
        sides[label] = dict(learner=learner, replay=replay, draw=0, mon=DeviceMonitor(env, capacity=iterations // E + 1) if label == "monitored" else None)

    def run(label):
        sd = sides[label]
        extra = {}
        if sd["mon"] is not None:
            sd["mon"].count = 0
            extra = dict(monitor=sd["mon"], log_every=E)
        sd["learner"].train(sd["replay"], iterations, 1, per_step, seed=1, first_draw=sd["draw"] + 1, **extra)
        sd["draw"] += iterations * per_step

    def window(label):
        sync()
        t0 = time.perf_counter()
        run(label)
        sync()
        return (time.perf_counter() - t0) * 1e3

    for label in sides:
        run(label), run(label)
    wdw = {label: [] for label in sides}
    for _ in range(args.windows):
        for label in sides:
            wdw[label].append(window(label))
    result = {"tool": "bench_policy_rollout --monitor", "env": args.env, "num_envs": n, "windows": args.windows, "batch": 256, "hidden_width": 256,
              "iterations_per_window": iterations, "updates_per_iteration": per_step, "log_every": E, "device": torch.cuda.get_device_name(0),
              "ms_median": {k: float(np.median(v)) for k, v in wdw.items()}, "ms_min": {k: float(min(v)) for k, v in wdw.items()},
              "ms_max": {k: float(max(v)) for k, v in wdw.items()}, "ms_windows": {k: [round(x, 3) for x in v] for k, v in wdw.items()}}
    if not args.monitored_only:
        med, spread = result["ms_median"], float(max(wdw["plain"]) - min(wdw["plain"]))
        excess = med["monitored"] - med["plain"]
        result.update(plain_ms_spread=spread, excess_ms=excess, excess_us_per_iteration=excess * 1e3 / iterations,
                      ratio_monitored_over_plain=med["monitored"] / med["plain"], not_slower=med["monitored"] <= med["plain"] + spread)
        last = sides["monitored"]["mon"].results()
        result["last_window_records"] = [{k: r[k] for k in ("iteration", "episodes", "mean_return", "mean_length", "success_rate")} for r in last]
    for sd in sides.values():
        sd["learner"].close()
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="UR5DynReach-v1", choices=sorted(ACTOR_NPZ))
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=20, help="steps of a window of the host loop (it is ~100x slower)")
    ap.add_argument("--warmup", type=int, default=110, help="steps before the first window (past the common truncation at step 100)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", action="store_true",
                    help="also time the stochastic half: the GAUSSIAN launch interleaved with the deterministic one, and a sampled "
                         "rollout without records and with all of them (sample records included)")
    ap.add_argument("--added-valu-per-wave", type=int, default=1858,
                    help="--sample: vector instructions the sampling instance executes beyond the deterministic one (from the ISA)")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--critic", action="store_true", help="measure the twin Q critic launch against the actor launch and torch (see above)")
    ap.add_argument("--windows", type=int, default=10, help="--critic: alternating windows per kind")
    ap.add_argument("--launches", type=int, default=200, help="--critic: back-to-back launches per window")
    ap.add_argument("--replay", action="store_true", help="measure the device replay ring: collect against a Python loop, the gather against torch (see above)")
    ap.add_argument("--capacity", type=int, default=256, help="--replay: slots of the ring")
    ap.add_argument("--refresh", action="store_true", help="measure reloading actor / critic weights from device tensors against the host route and a copy (see above)")
    ap.add_argument("--action-gradient", action="store_true", help="measure the critics' action gradient launch against critic_kernel and torch autograd (see above)")
    ap.add_argument("--critic-gradient", action="store_true", help="measure the critics' parameter gradients (two or three launches) against torch autograd (see above)")
    ap.add_argument("--actor-gradient", action="store_true", help="measure the actor's parameter gradients (two or three launches) against torch autograd (see above)")
    ap.add_argument("--optimizer", action="store_true", help="measure the Adam step kernels (one launch each) against torch's Adam.step followed by the reloads, and the learner's update with and without them")
    ap.add_argument("--entropy", action="store_true", help="measure the learner's update with device_optimizer only against the same plus device_entropy (see above)")
    ap.add_argument("--clip", action="store_true", help="measure the update with max_grad_norm against the update without it, as update() calls and as one native call per window (see above)")
    ap.add_argument("--clone", action="store_true", help="measure urgym_sac_policy_terms_cloned against urgym_sac_policy_terms at M = 256 and 65536, and the update with and without bc_weight (see above)")
    ap.add_argument("--clone-weighted", action="store_true", help="measure urgym_sac_policy_terms_weighted against urgym_sac_policy_terms_cloned at M = 256 and 65536, and the native update without cloning, with plain cloning and with the advantage weight (see above)")
    ap.add_argument("--demos", action="store_true", help="measure urgym_replay_sample_mixed against urgym_replay_sample and the masked cloned terms against the cloned ones at M = 256 and 65536 (D = M / 2), and the update with and without a demonstration ring (see above)")
    ap.add_argument("--normalize", action="store_true", help="measure the update with normalize against the update without it, the collection step without and with the normalize launch, and the fold (see above)")
    ap.add_argument("--normalize-only", action="store_true", help="--normalize: run only the normalized collection, the fold and the normalized native updates (for a kernel trace)")
    ap.add_argument("--collect-steps", type=int, default=8, help="--normalize: steps per collection and per fold")
    ap.add_argument("--clip-only", action="store_true", help="--clip: run only the clipped native updates, --windows x --launches of them (for a kernel trace)")
    ap.add_argument("--max-grad-norm", type=float, default=1.0, help="--clip: the bound of the clipped learners")
    ap.add_argument("--native", action="store_true", help="measure the thirteen-call update against SACLearner.train, one native call per window (see above)")
    ap.add_argument("--native-only", action="store_true", help="--native: run only the native updates, --windows x --launches of them (for a kernel trace)")
    ap.add_argument("--evaluate", action="store_true", help="measure one evaluation (DeviceEvaluation.evaluate) against load_parameters + reset + run_closed_loop_device, and a training run with evaluations as one call against one call per interval plus the Python evaluation")
    ap.add_argument("--monitor", action="store_true", help="measure SACLearner.train with monitor=, log_every=10 against the same call without a monitor (see above)")
    ap.add_argument("--monitored-only", action="store_true", help="--monitor: run only the monitored call, --windows times (for a kernel trace)")
    ap.add_argument("--nstep", action="store_true", help="measure the gather of multi-step returns against the one-step gather and a torch composition, and the learner at n_steps 1 and 3")
    ap.add_argument("--prioritized", action="store_true", help="measure the prioritized update against the uniform one (SACLearner.train, batch 65,536 and 4,096, H = 256), and the prioritized gather and urgym_per_terms on their own")
    ap.add_argument("--prioritized-only", action="store_true", help="--prioritized: run only the prioritized native updates at batch 65,536, --windows x --launches of them (for a kernel trace)")
    ap.add_argument("--hindsight", action="store_true", help="measure the update with hindsight relabelling against the uniform one (SACLearner.train, batch 65,536 and 4,096, H = 256), and the two gathers on their own")
    ap.add_argument("--hindsight-only", action="store_true", help="--hindsight: run only the hindsight updates and gathers (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.prioritized or args.prioritized_only:
        return prioritized_mode(args)
    if args.hindsight or args.hindsight_only:
        return hindsight_mode(args)
    if args.nstep:
        return nstep_mode(args)
    if args.monitor:
        return monitor_mode(args)
    if args.evaluate:
        return evaluate_mode(args)
    if args.clone_weighted:
        return clone_weighted_mode(args)
    if args.clone:
        return clone_mode(args)
    if args.demos:
        return demos_mode(args)
    if args.clip or args.clip_only:
        return clip_mode(args)
    if args.normalize or args.normalize_only:
        return normalize_mode(args)
    if args.native:
        return native_mode(args)
    if args.entropy:
        return entropy_mode(args)
    if args.optimizer:
        return optimizer_mode(args)
    if args.actor_gradient:
        return actor_gradient_mode(args)
    if args.action_gradient:
        return action_gradient_mode(args)
    if args.critic_gradient:
        return critic_gradient_mode(args)
    if args.critic:
        return critic_mode(args)
    if args.replay:
        return replay_mode(args)
    if args.refresh:
        return refresh_mode(args)

    import torch
    import torch.nn.functional as F

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeterministicActor, DeviceActor, HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout.py measures on a GPU; none is visible")
    dev = "cuda:0"
    n, K = args.num_envs, args.steps
    path = os.path.join(ROOT, "tests", "golden", "actors", f"actor_{ACTOR_NPZ[args.env]}.npz")
    w = dict(np.load(path))
    if args.sample:
        w.update(np.load(os.path.join(ROOT, "tests", "golden", "actors", f"log_std_{ACTOR_NPZ[args.env]}.npz")))
    env = make_vec(args.env, num_envs=n, device=dev, seed=0, auto_reset=True)
    env.reset(seed=0)
    actor = DeviceActor(w, env)
    host_actor, backend = DeterministicActor(w), HipBackend(env)
    tw = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in w.items()}
    sync = lambda: torch.cuda.synchronize(env.device)

    def host_loop(steps):
        for _ in range(steps):
            backend.step(host_actor(*backend.observe()))

    def torch_loop(steps):
        b = env.buf
        for _ in range(steps):
            x = torch.cat([b["achieved_goal"], b["desired_goal"], b["observation"]], dim=1)
            h = F.relu(F.linear(x, tw["latent_pi_0_weight"], tw["latent_pi_0_bias"]))
            h = F.relu(F.linear(h, tw["latent_pi_2_weight"], tw["latent_pi_2_bias"]))
            env.step(torch.tanh(F.linear(h, tw["mu_weight"], tw["mu_bias"])))

    def device_loop(steps):
        env.rollout_policy(actor, steps, record=())

    def device_loop_recorded(steps):
        return env.rollout_policy(actor, steps, record="all")

    variants = [("host_numpy_actor", host_loop, args.host_steps), ("torch_linear_actor", torch_loop, K),
                ("device_actor", device_loop, K), ("device_actor_all_records", device_loop_recorded, K)]
    if args.sample:
        draws = [0]  # every window continues the draw sequence

        def sampled(record):
            def run(steps):
                out = env.rollout_policy(actor, steps, record=record, sample=dict(mode="gaussian", seed=1, first_draw=draws[0]))
                draws[0] += steps
                return out
            return run

        variants += [("device_actor_gaussian", sampled(()), K), ("device_actor_gaussian_all_records", sampled("all"), K)]
    # warm-up: every variant once (code objects, BLAS algorithm choice, the allocator's blocks for the records), then past step 100
    for _, fn, steps in variants:
        fn(min(steps, 10))
    device_loop(args.warmup)
    sync()
    times = {name: [] for name, _, _ in variants}
    for _ in range(args.repeats):
        for name, fn, steps in variants:
            sync()
            t0 = time.perf_counter()
            fn(steps)
            sync()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    per_step = {name: float(np.median(v)) for name, v in times.items()}

    # the actor launch alone (device events around back-to-back launches), and the step launch as the library times it
    out = torch.empty((n, 6), dtype=torch.float32, device=dev)
    for _ in range(10):
        env.policy_actions(actor, out=out)
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    e0.record()
    for _ in range(reps):
        env.policy_actions(actor, out=out)
    e1.record()
    sync()
    actor_us = e0.elapsed_time(e1) * 1e3 / reps
    launch_pairs = None
    if args.sample:
        # Deterministic and GAUSSIAN launches of the same build, alternating windows of `reps` back-to-back launches in this process.
        # Both go straight to the C ABI with fixed buffers, so the two windows differ in the kernel alone.
        import ctypes as C

        from ur_gym_amd import _abi

        how = _abi.Sampling(_abi.SAMPLE_GAUSSIAN, 0, 1, 0)
        log_prob = torch.empty((n,), dtype=torch.float32, device=dev)
        h, a, stream = env._h, actor._a, env._stream()
        act_p, lp_p = C.c_void_p(out.data_ptr()), C.c_void_p(log_prob.data_ptr())

        def window(fn):
            sync()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            sync()
            return e0.elapsed_time(e1) * 1e3 / reps

        kinds = (lambda: env.lib.urgym_actor_forward(h, a, act_p, stream),
                 lambda: env.lib.urgym_actor_sample(h, a, C.byref(how), act_p, lp_p, stream))
        for fn in kinds:
            for _ in range(10):
                fn()
        launch_pairs = [tuple(window(fn) for fn in kinds) for _ in range(10)]
    env.enable_timing(True, every=8)
    device_loop(K)
    sync()
    step_us, _, launches = env.query_timing()
    env.enable_timing(False)
    flop = 2.0 * n * (actor.in_features * actor.hidden_width + actor.hidden_width ** 2 + actor.hidden_width * 6)
    result = {
        "tool": "bench_policy_rollout", "env": args.env, "num_envs": n, "steps": K, "host_steps": args.host_steps, "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0),
        "us_per_step_median": per_step, "us_per_step_all": {k: [round(x, 2) for x in v] for k, v in times.items()},
        "env_steps_per_s": {k: n / v * 1e6 for k, v in per_step.items()},
        "device_not_slower_than_torch": per_step["device_actor"] <= per_step["torch_linear_actor"],
        "speedup_device_over_torch": per_step["torch_linear_actor"] / per_step["device_actor"],
        "speedup_device_over_host": per_step["host_numpy_actor"] / per_step["device_actor"],
        "actor_launch_us": actor_us, "step_launch_us": step_us, "step_launches_timed": launches,
        "actor_over_step_launch": actor_us / step_us if step_us > 0 else None,
        "actor_gflop_per_step": flop / 1e9, "actor_tflops": flop / actor_us / 1e6,
        "actor_fraction_of_f32_matrix_peak": flop / actor_us / 1e6 / F32_MATRIX_PEAK_TFLOPS,
    }
    if launch_pairs:
        det, gau = [p[0] for p in launch_pairs], [p[1] for p in launch_pairs]
        det_med, gau_med, spread = float(np.median(det)), float(np.median(gau)), float(max(det) - min(det))
        # what the added vector instructions would cost if none of them hid behind the matrix pipe: 4 cycles of issue each for
        # one wave, two waves per SIMD (DESIGN.md section 8 counts them in the final ISA of the width-256 instance)
        unhidden = args.added_valu_per_wave * 4 * 2 / (args.clock_ghz * 1e3)
        result["sampling_launch"] = {
            "deterministic_us_windows": [round(x, 3) for x in det], "gaussian_us_windows": [round(x, 3) for x in gau],
            "deterministic_us_median": det_med, "gaussian_us_median": gau_med, "deterministic_us_spread": spread,
            "gaussian_minus_deterministic_us": gau_med - det_med, "added_valu_per_wave": args.added_valu_per_wave,
            "unhidden_valu_us": unhidden, "bar_us": det_med + unhidden + spread, "within_bar": gau_med <= det_med + unhidden + spread,
            "parent_deterministic_us": 90.7,
        }
    actor.close()
    env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
