"""Times SACLearner.save / load at the defaults of tools/train_sac.py (UR5DynReach-v1, N = 1024, a full ring of 1024 slots, H = 256),
each split into its device <-> host copies and its file I/O, and prints one JSON line (nothing here is a hot
path, the numbers are reported, not barred).

    python tools/bench_checkpoint.py --out profiles/policy_rollout/dyn_checkpoint.json
    rocprofv3 --kernel-trace --stats -- python tools/bench_checkpoint.py --unpack-only 50     # the two unpack launches, in a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="UR5DynReach-v1")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--hidden-width", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--unpack-only", type=int, default=0, metavar="K", help="K x (actor unpack, critic unpack) and nothing else: the run a profiler traces")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from ur_gym_amd import checkpoint, make_vec
    from ur_gym_amd.evaluation import DeviceReplay
    from ur_gym_amd.training import SACLearner

    env = make_vec(args.env, num_envs=args.num_envs, seed=0, auto_reset=True)
    env.reset(seed=0)
    learner = SACLearner(env, seed=0, hidden_width=args.hidden_width, device_action_gradient=True, device_critic_gradient=True,
                         device_actor_gradient=True, device_optimizer=True, device_entropy=True)
    if args.unpack_only:
        for _ in range(args.unpack_only):
            learner.device_actor.parameters()
            learner.target.parameters()
        torch.cuda.synchronize(env.device)
        learner.close(), env.close()
        return
    replay = DeviceReplay(env, args.capacity)
    learner.train(replay, args.capacity, 1, 0, seed=0, first_draw=0)  # a full ring
    learner.train(replay, 4, 1, 2, seed=0, first_draw=0)              # moments that are not zero
    torch.cuda.synchronize(env.device)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "run.npz")
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            state = dict(learner=learner.state_dict(), extra=None, replay=replay.state_dict(), monitor=None, evaluation=None, env=env.checkpoint_state())
            t1 = time.perf_counter()
            checkpoint.write(path, state)
            t2 = time.perf_counter()
            loaded = checkpoint.read(path)
            t3 = time.perf_counter()
            learner.load_state_dict(loaded["learner"])
            env.restore_checkpoint(loaded["env"])
            replay.load_state_dict(loaded["replay"])
            torch.cuda.synchronize(env.device)
            t4 = time.perf_counter()
            rows.append(dict(save_device_to_host_s=t1 - t0, save_file_s=t2 - t1, load_file_s=t3 - t2, load_host_to_device_s=t4 - t3))
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        learner.save(path, replay=replay)
        t1 = time.perf_counter()
        learner.load(path, replay=replay)
        torch.cuda.synchronize(env.device)
        t2 = time.perf_counter()
    out = dict(env=args.env, num_envs=args.num_envs, capacity=args.capacity, hidden_width=args.hidden_width, repeats=args.repeats, file_bytes=size,
               save_s=t1 - t0, load_s=t2 - t1, **{k: statistics.median(r[k] for r in rows) for k in rows[0]}, runs=rows)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    learner.close(), env.close()


if __name__ == "__main__":
    main()
