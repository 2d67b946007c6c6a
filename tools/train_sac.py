"""Runs ur_gym_amd.training.SACLearner: the loop of the reference's train.py:40-60 (SAC.learn) on the device pieces, printing the
mean episode return and the success rate of the deterministic policy (evaluation.run_closed_loop_device on a second, auto-reset-off
environment, as model_test.py evaluates) every so many updates.

    python tools/train_sac.py --env UR5OriReach-v1 --num-envs 1024 --steps 2000 --updates-per-step 4 --eval-every 200

One loop trip = one env step of all N envs into the ring, then `--updates-per-step` gradient steps.  Prints one JSON line per
evaluation.  No checkpoint is written.  With --native (and --device-entropy and the options it needs) the trips between two
evaluations are ONE native call, SACLearner.train: the same launches, bit for bit, with no Python between them.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="UR5OriReach-v1")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2000, help="env steps (of all N envs) to collect")
    ap.add_argument("--updates-per-step", type=int, default=4)
    ap.add_argument("--capacity", type=int, default=1024, help="slots of the replay ring (N transitions each)")
    ap.add_argument("--eval-every", type=int, default=200, help="updates between evaluations")
    ap.add_argument("--eval-envs", type=int, default=1024)
    ap.add_argument("--hidden-width", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-action-gradient", action="store_true",
                    help="take the actor loss's d min Q / da from the HIP gradient kernel instead of a second torch critic pass (hidden width <= 256)")
    ap.add_argument("--device-critic-gradient", action="store_true",
                    help="take the critic loss's parameter gradients from the HIP kernels instead of torch autograd (hidden width <= 256)")
    ap.add_argument("--device-actor-gradient", action="store_true",
                    help="take the actor loss's parameter gradients from the HIP kernels instead of torch autograd: with the two options "
                         "above, which it needs, no forward or backward pass of an update runs in torch (hidden width <= 256)")
    ap.add_argument("--device-optimizer", action="store_true",
                    help="step the actor's and the critics' parameters with the HIP Adam kernels, which also reload the device networks and "
                         "blend the target: one launch each instead of torch's optimisers and three reloads (needs --device-critic-gradient "
                         "and --device-actor-gradient)")
    ap.add_argument("--device-entropy", action="store_true",
                    help="step the entropy coefficient and form its uses and the three loss values with two HIP launches: no torch operation "
                         "is left in an update but allocations and views (needs --device-optimizer)")
    ap.add_argument("--native", action="store_true",
                    help="run the loop between two evaluations as ONE native call (SACLearner.train): no Python between the launches "
                         "(needs --device-entropy)")
    args = ap.parse_args()

    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceActor, DeviceReplay, run_closed_loop_device
    from ur_gym_amd.training import SACLearner, host_arrays

    if not torch.cuda.is_available():
        raise SystemExit("train_sac.py trains on a GPU; none is visible")
    env = make_vec(args.env, num_envs=args.num_envs, seed=args.seed, auto_reset=True)
    env.reset(seed=args.seed)
    test_env = make_vec(args.env, num_envs=args.eval_envs, seed=args.seed + 1, auto_reset=False)
    learner = SACLearner(env, seed=args.seed, hidden_width=args.hidden_width, batch_size=args.batch_size,
                         device_action_gradient=args.device_action_gradient, device_critic_gradient=args.device_critic_gradient,
                         device_actor_gradient=args.device_actor_gradient, device_optimizer=args.device_optimizer,
                         device_entropy=args.device_entropy)
    eval_actor = DeviceActor(host_arrays(learner.actor.tensors()), test_env)  # actors belong to the environment they were made for
    replay = DeviceReplay(env, args.capacity)
    updates, t0 = 0, time.perf_counter()

    def evaluate():
        eval_actor.load_parameters(learner.actor.tensors())
        test_env.reset(seed=args.seed + 1)
        res = run_closed_loop_device(test_env, eval_actor)
        print(json.dumps({"updates": updates, "env_steps": learner.env_steps * env.num_envs, "seconds": round(time.perf_counter() - t0, 1),
                          "mean_episode_return": res["mean_episode_reward"], "success_rate_percent": res["success_rate_percent"]}), flush=True)

    step = 0
    while args.native and step < args.steps:
        # as many loop trips as reach the next evaluation, in one call (warm-up trips run no update, so a call may fall short of it and
        # the next one goes on); an evaluation falls at the end of the trip that passes a multiple of --eval-every
        per_trip = max(1, args.updates_per_step)
        trips = min(args.steps - step, -(-(args.eval_every - updates % args.eval_every) // per_trip))
        before = learner.adam_state["step"]
        learner.train(replay, trips, 1, args.updates_per_step, seed=args.seed, first_draw=updates)
        step += trips
        done = learner.adam_state["step"] - before
        passed = (updates + done) // args.eval_every > updates // args.eval_every
        updates += done
        if passed:
            evaluate()
    for step in range(step, args.steps):  # the Python loop (every trip of it where --native is off)
        learner.collect(replay, 1)
        if learner.env_steps * env.num_envs < learner.hp["learning_starts"]:
            continue
        for _ in range(args.updates_per_step):
            learner.update(replay, args.seed, updates)
            updates += 1
            if updates % args.eval_every == 0:
                evaluate()
    eval_actor.close()
    learner.close()
    test_env.close()
    env.close()


if __name__ == "__main__":
    main()
