"""Runs ur_gym_amd.training.SACLearner: the loop of the reference's train.py:40-60 (SAC.learn) on the device pieces, printing the
mean episode return and the success rate of the deterministic policy (evaluation.run_closed_loop_device on a second, auto-reset-off
environment, as model_test.py evaluates) every so many updates.

    python tools/train_sac.py --env UR5OriReach-v1 --num-envs 1024 --steps 2000 --updates-per-step 4 --eval-every 200

One loop trip = one env step of all N envs into the ring, then `--updates-per-step` gradient steps.  Prints one JSON line per
evaluation.  With --native (and --device-entropy and the options it needs) the WHOLE run is ONE native call,
SACLearner.train(..., evaluation=, eval_every=): the same launches, bit for bit, with no Python between them; the evaluations run
inside the call (evaluation.DeviceEvaluation: statistics, the improvement decision and the copy of the best actor on the device), and
their records are printed after one synchronise at the end (each evaluation there starts from a zeroed observation buffer, which
matters on UR5DynReach-v1 alone: its reset keeps the velocity slot it finds).  --save-best PATH writes the best actor as an .npz DeviceActor.load reads.
With --monitor the training curve is printed as well, on both routes: every --log-every trips one line with the number, the mean return,
the mean length and the success rate of the episodes the COLLECTING policy finished since the line before (evaluation.DeviceMonitor: the
reference's Monitor and SB3's rollout/ep_rew_mean, ep_len_mean and success_rate, reduced on the device).  With --native those records,
too, are written inside the one call and read after its one synchronise.
--save PATH writes the WHOLE run as a checkpoint when it ends and every --save-every updates (SACLearner.save: the parameters, the target
critic, every Adam moment, the entropy coefficient, the ring, the environment, the monitor, with --native the evaluation, and this loop's
own counters); --resume PATH continues it with the same arguments up to --steps trips in all -- the reference's train.py:31-36 -- and
prints the evaluation and monitor lines from the resume point on as the uninterrupted run prints them (on the device routes every number
in them is the same; without --native the evaluations are this script's own and its best actor so far is kept only as its mean).
--init-from ACTOR.npz CRITIC0.npz CRITIC1.npz starts a run from plain parameter files instead (SACLearner.load_parameters).
--max-grad-norm X clips the critics' and the actor's gradients by their global norm on the device (SACLearner(max_grad_norm=X), needs
--device-entropy; SB3's SAC does not clip) and adds to every evaluation line the three losses and the two gradient norms, before
clipping, of the latest update.
--normalize keeps stable-baselines3's VecNormalize on the device (SACLearner(normalize=True), needs --device-entropy): the collecting actor
and the update read observations and rewards normalized with running statistics, the ring keeps the raw rows, and every evaluation runs
its actor on rows normalized with the TRAINING statistics as they then stand (sync_envs_normalization) -- with --native inside the one
call (urgym_policy_evaluate_normalized), otherwise step by step from this script -- and --save-best writes the statistics the best actor
was selected under beside it (evaluation.load_best_normalization reads them).
--planner collects with an MPPI planner in place of the sampled policy (SACLearner.collect(planner=), urgym_mppi_collect; DESIGN.md section
28): every trip plans with --planner-samples futures per env over --planner-horizon steps, optionally guided by the learner's own actor
(--planner-policy-samples) and critic (--planner-terminal-value), executes the plan's first action plus --planner-explore-sigma times
exploration noise (--planner-iterations, --planner-elites, --planner-adapt-std, --planner-std-min, --planner-std-max: refinement with
elite samples and an adaptive std), and after the trip's updates puts the planner's actor and critic on the learner's parameters (SACLearner.sync_planner).
With --native the planned collection, the updates and the reload are inside the one call as well (SACLearner.train(planner=),
urgym_sac_train_planned), and with --monitor every line of the training curve is followed by a line of plan
statistics over the envs' last plans (evaluation.mppi_plan_stats: the mean best and nominal return, their mean difference, the mean and
the lowest effective sample size, how many envs had a finite plan, and with elites their mean count and threshold).  Not with
--normalize (the planner's actor and critic read raw rows).  Otherwise it prints what it prints without.
--planner-ess-target T solves the planner's temperature per env at every update so that the weights have an effective sample size of T
(DeviceMPPI(ess_target=), urgym_mppi_*_tempered and with --native urgym_sac_train_tempered); --planner-lam is then
used only by an env without a finite return.  With --monitor the last line of plan statistics of a native call also carries the mean of
the temperatures its last plan left and how many envs ended at a bound, read on the host after the call's synchronise.
--planner-noise-beta B gives the planner's sampling noise a lag-1 correlation of B along the horizon (DeviceMPPI(noise_beta=),
urgym_mppi_*_colored and with --native urgym_sac_train_colored); 0 is white noise through the same calls.
--bc-weight X adds behaviour cloning to the policy loss (SACLearner(bc_weight=X), needs --device-entropy): the
policy's action is pulled towards the action the ring holds -- the planner's, with --planner -- with weight X, or with --bc-scale-by-q X
times the batch's mean |min Q| (TD3+BC's normalisation), on every row or with --bc-q-filter on the rows where the critics rate the ring's
action above the policy's own; with --native urgym_sac_train_cloned.  Every evaluation line then also carries the three losses, bc_loss,
bc_weight and the cloned share of the batch of the latest update.
--bc-advantage-temperature T (with --bc-weight, not with --bc-q-filter) weights every cloned row by exp(advantage / T),
normalised over the batch and capped at --bc-advantage-max-weight (SACLearner(bc_advantage_temperature=T, bc_advantage_max_weight=);
with --native urgym_sac_train_weighted): the evaluation lines then also carry adv_ess (the effective number of rows the weights spread over),
adv_max (the largest weight) and adv_clipped (the rows the cap held), and with --native one more line gives adv_ess over the whole run.
--demo-steps T --demo-envs N_d fills a demonstration ring first: T steps of the planner the --planner* flags describe
on a second env of N_d envs, filed into a ring of T slots that the run never writes again (--demo-save PATH keeps it as an .npz,
--demo-load PATH reads one instead of filling).  --demo-batch-size D then draws the first D rows of every minibatch from it
(SACLearner(demonstrations=, demo_batch_size=D), urgym_replay_sample_mixed; with --native urgym_sac_train_demonstrated), and --bc-demo-only
restricts --bc-weight's cloning to those rows: the evaluation lines then also carry the cloned share of the demonstration rows.
--demo-controller fills the ring with the scripted reach controller instead (damped least-squares IK, --demo-damping,
--demo-gain; DeviceReplay.collect_scripted, urgym_controller_collect): one small launch per step and no planner env.
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
    ap.add_argument("--n-steps", type=int, default=1,
                    help="multi-step returns: a target spans up to this many consecutive steps of an env and stops at an episode's end "
                         "(SB3's n_steps; above 1 needs --device-entropy)")
    ap.add_argument("--prioritized", action="store_true",
                    help="proportional prioritized replay on the device: draw each minibatch row in proportion to |TD error| ** alpha and "
                         "weight the critics' gradient by the importance weights (needs --device-entropy; not with --n-steps above 1)")
    ap.add_argument("--per-alpha", type=float, default=0.6, help="--prioritized: the priority exponent, in [0, 1]")
    ap.add_argument("--per-beta", type=float, default=0.4, help="--prioritized: the importance exponent at the first update, in [0, 1]")
    ap.add_argument("--per-beta-steps", type=int, default=100000, help="--prioritized: updates over which beta rises linearly to 1")
    ap.add_argument("--hindsight", action="store_true",
                    help="hindsight experience replay on the device (SB3's HerReplayBuffer): the gather gives a share of each minibatch's rows "
                         "a goal their own episode reached later and re-scores them (needs --device-entropy; not with --n-steps above 1 or --prioritized)")
    ap.add_argument("--her-n-sampled-goal", type=int, default=4, help="--hindsight: relabelled rows per kept row (4: a share of 0.8)")
    ap.add_argument("--her-strategy", default="future", choices=("future", "final"), help="--hindsight: which later pose of the episode becomes the goal")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="clip the critics' and the actor's gradients by their global norm on the device (torch's clip_grad_norm_ idiom; SB3's SAC "
                         "does not clip) and print the losses and the norms with every evaluation (needs --device-entropy)")
    ap.add_argument("--bc-weight", type=float, default=None, metavar="X",
                    help="behaviour cloning in the policy loss: pull the policy's action towards the ring's with weight X >= 0 and print bc_loss and the "
                         "cloned share with the losses (needs --device-entropy; DESIGN.md section 33)")
    ap.add_argument("--bc-scale-by-q", action="store_true", help="--bc-weight: multiply the weight by the batch's mean |min Q| (TD3+BC's normalisation)")
    ap.add_argument("--bc-q-filter", action="store_true", help="--bc-weight: clone only the rows where the critics rate the ring's action above the policy's own")
    ap.add_argument("--bc-advantage-temperature", type=float, default=None, metavar="T",
                    help="--bc-weight: weight every cloned row by exp(advantage / T), normalised over the batch (AWAC's weight; not with --bc-q-filter; "
                         "DESIGN.md section 35)")
    ap.add_argument("--bc-advantage-max-weight", type=float, default=None, metavar="C", help="--bc-advantage-temperature: cap a row's weight at C (default: no cap)")
    ap.add_argument("--demo-steps", type=int, default=0, metavar="T",
                    help="fill a demonstration ring of T slots first, on a second env of the same kind, with the planner the --planner* flags describe "
                         "(guided by the learner's initial networks where they ask for a guide; --planner itself is not needed; DESIGN.md section 34)")
    ap.add_argument("--demo-guide", nargs=3, metavar=("ACTOR.npz", "CRITIC0.npz", "CRITIC1.npz"), default=None,
                    help="--demo-steps: guide the demonstrating planner with these plain parameter files (as --init-from reads them) instead of the "
                         "learner's initial networks: a demonstrator that already knows the task")
    ap.add_argument("--demo-controller", action="store_true",
                    help="--demo-steps: fill the demonstration ring with the scripted reach controller (damped least-squares IK) instead of the planner; "
                         "--planner-explore-sigma scales its exploration noise")
    ap.add_argument("--demo-damping", type=float, default=0.2, metavar="L", help="--demo-controller: the damping of the least-squares step, in [1e-2, 10]")
    ap.add_argument("--demo-gain", type=float, default=0.5, metavar="G", help="--demo-controller: the share of the solved step taken, in (0, 10]")
    ap.add_argument("--demo-envs", type=int, default=64, metavar="N_d", help="--demo-steps, --demo-load: envs of the demonstration ring's env")
    ap.add_argument("--demo-save", metavar="PATH", default=None, help="write the demonstration ring as an .npz (DeviceReplay.save) once it is filled")
    ap.add_argument("--demo-load", metavar="PATH", default=None,
                    help="read the demonstration ring from a file --demo-save wrote, with the same --demo-steps (its capacity) and --demo-envs, instead of filling it")
    ap.add_argument("--demo-batch-size", type=int, default=None, metavar="D",
                    help="draw the first D rows of every minibatch from the demonstration ring (needs --device-entropy and --demo-steps; not with "
                         "--n-steps above 1, --prioritized or --hindsight)")
    ap.add_argument("--bc-demo-only", action="store_true", help="--bc-weight with --demo-batch-size: clone only the demonstration rows")
    ap.add_argument("--normalize", action="store_true",
                    help="running observation and reward normalization on the device (SB3's VecNormalize; needs --device-entropy)")
    ap.add_argument("--no-norm-obs", action="store_true", help="--normalize: leave the observations as they are")
    ap.add_argument("--no-norm-reward", action="store_true", help="--normalize: leave the rewards as they are")
    ap.add_argument("--clip-obs", type=float, default=10.0, help="--normalize: the bound of a normalized observation element")
    ap.add_argument("--clip-reward", type=float, default=10.0, help="--normalize: the bound of a normalized reward")
    ap.add_argument("--norm-epsilon", type=float, default=1e-8, help="--normalize: added to a variance before its square root")
    ap.add_argument("--native", action="store_true",
                    help="run the whole loop, evaluations included, as ONE native call (SACLearner.train): no Python between the launches "
                         "(needs --device-entropy)")
    ap.add_argument("--monitor", action="store_true",
                    help="print the training curve: the episodes the collecting policy finishes, reduced on the device (DeviceMonitor)")
    ap.add_argument("--log-every", type=int, default=100, help="loop trips between two lines of the training curve (--monitor)")
    ap.add_argument("--save-best", metavar="PATH", default=None,
                    help="write the actor of the best evaluation (mean episode return strictly above every earlier one) as an .npz")
    ap.add_argument("--save", metavar="PATH", default=None,
                    help="write the whole run as a checkpoint (SACLearner.save: learner, target critic, moments, ring, environment, monitor, "
                         "evaluation, counters) when it ends, and every --save-every updates; written to a temporary name and renamed")
    ap.add_argument("--save-every", type=int, default=0, metavar="UPDATES", help="updates between two checkpoints (0: only at the end); needs --save")
    ap.add_argument("--resume", metavar="PATH", default=None,
                    help="continue the run a checkpoint holds, with the same arguments, up to --steps trips in all: bit for bit the "
                         "uninterrupted run on the device routes, and the same evaluation and monitor lines from the resume point on")
    ap.add_argument("--init-from", nargs=3, metavar=("ACTOR.npz", "CRITIC0.npz", "CRITIC1.npz"), default=None,
                    help="warm start from plain parameter files (the reference's SAC.load then learn, train.py:31-36): the actor's eight "
                         "arrays as --save-best writes them, one file per Q-network; moments and step count start at zero")
    ap.add_argument("--planner", action="store_true",
                    help="collect with an MPPI planner on the step kernel instead of the sampled policy, from the first trip on "
                         "(SACLearner.collect(planner=), with --native SACLearner.train(planner=); not with --normalize)")
    ap.add_argument("--planner-samples", type=int, default=64, help="--planner: futures per env, in [2, 1024]; the planner steps num-envs times as many envs")
    ap.add_argument("--planner-horizon", type=int, default=6, help="--planner: steps of a future, in [1, 64]")
    ap.add_argument("--planner-sigma", type=float, default=0.6, help="--planner: standard deviation of the sampled action sequences")
    ap.add_argument("--planner-lam", type=float, default=5.0, help="--planner: the temperature of the weights")
    ap.add_argument("--planner-policy-samples", type=int, default=0, help="--planner: futures per env that follow the learner's actor, in [0, samples - 1]")
    ap.add_argument("--planner-policy-sigma", type=float, default=0.1, help="--planner: noise on the actions of the futures that follow the actor")
    ap.add_argument("--planner-terminal-value", action="store_true",
                    help="--planner: credit a future alive after the horizon with the learner's min Q of the state it stops in (the planner then discounts with the learner's gamma)")
    ap.add_argument("--planner-fail-cost", type=float, default=0.0, help="--planner: what a future that ends without success is charged")
    ap.add_argument("--planner-explore-sigma", type=float, default=0.0, help="--planner: standard deviation of the exploration noise on the executed action")
    ap.add_argument("--planner-iterations", "--iterations", type=int, default=1, help="--planner: refinement iterations of a plan, in [1, 8]")
    ap.add_argument("--planner-elites", "--elites", type=int, default=None, metavar="M",
                    help="--planner: only the M best-scoring futures of an env weigh in, M in [1, samples] (DESIGN.md section 29; default: every finite one)")
    ap.add_argument("--planner-adapt-std", "--adapt-std", action="store_true",
                    help="--planner: iterations after the first sample with a std per (step, joint) formed from the elites of the one before (needs --planner-iterations > 1 to act)")
    ap.add_argument("--planner-std-min", "--std-min", type=float, default=0.05, help="--planner-adapt-std: the floor of the adaptive std")
    ap.add_argument("--planner-std-max", "--std-max", type=float, default=None, help="--planner-adapt-std: its ceiling (default: --planner-sigma)")
    ap.add_argument("--planner-ess-target", type=float, default=None, metavar="T",
                    help="--planner: solve the temperature per env and update for an effective sample size of T, in [1, M] (M = --planner-elites, else "
                         "--planner-samples; DESIGN.md section 31; default: the fixed --planner-lam)")
    ap.add_argument("--planner-noise-beta", type=float, default=None, metavar="B",
                    help="--planner: sampling noise with lag-1 correlation B in [0, 1] along the horizon (DESIGN.md section 32; default: white noise, the calls of before)")
    args = ap.parse_args()
    if args.planner and args.normalize:
        raise SystemExit("--planner plans on raw rows: not with --normalize (the planner's actor and critic read raw rows)")
    if (args.bc_scale_by_q or args.bc_q_filter) and args.bc_weight is None:
        raise SystemExit("--bc-scale-by-q and --bc-q-filter qualify --bc-weight and need it")
    if args.bc_advantage_temperature is not None and (args.bc_weight is None or args.bc_q_filter):
        raise SystemExit("--bc-advantage-temperature needs --bc-weight and is the alternative to --bc-q-filter")
    if args.bc_advantage_max_weight is not None and args.bc_advantage_temperature is None:
        raise SystemExit("--bc-advantage-max-weight qualifies --bc-advantage-temperature and needs it")
    if args.demo_batch_size is not None and args.demo_steps < 1:
        raise SystemExit("--demo-batch-size needs a demonstration ring: give --demo-steps T (with --demo-load, the capacity of the file's ring)")
    if (args.demo_save or args.demo_load) and args.demo_steps < 1:
        raise SystemExit("--demo-save and --demo-load need --demo-steps T, the capacity of the ring")
    if args.bc_demo_only and (args.bc_weight is None or args.demo_batch_size is None):
        raise SystemExit("--bc-demo-only needs --bc-weight and --demo-batch-size")
    if args.demo_controller and (args.demo_steps < 1 or args.demo_load or args.demo_guide):
        raise SystemExit("--demo-controller fills the ring of --demo-steps T itself: not with --demo-load or --demo-guide")
    if args.save_every and not args.save:
        raise SystemExit("--save-every needs --save")
    if args.save_every < 0:
        raise SystemExit("--save-every must not be negative")
    if args.resume and args.init_from:
        raise SystemExit("--resume continues a run, --init-from starts one: give one of them")

    import torch

    from ur_gym_amd import make_vec
    from ur_gym_amd.evaluation import DeviceActor, DeviceEvaluation, DeviceMonitor, DeviceMPPI, DevicePrioritizedReplay, DeviceReachController, DeviceReplay, evaluation_points, run_closed_loop_device, save_actor, warmup_iterations
    from ur_gym_amd.training import SACLearner, host_arrays

    if not torch.cuda.is_available():
        raise SystemExit("train_sac.py trains on a GPU; none is visible")
    env = make_vec(args.env, num_envs=args.num_envs, seed=args.seed, auto_reset=True)
    env.reset(seed=args.seed)
    test_env = make_vec(args.env, num_envs=args.eval_envs, seed=args.seed + 1, auto_reset=False)
    demo_env = demos = None
    if args.demo_steps > 0:  # the ring exists before the learner, which checks it; it is filled below, once the planner can be made
        demo_env = make_vec(args.env, num_envs=args.demo_envs, seed=args.seed + 2, auto_reset=True)
        demo_env.reset(seed=args.seed + 2)
        demos = DeviceReplay(demo_env, args.demo_steps)
        if args.demo_load:
            demos.load_file(args.demo_load)
        else:
            demos.cursor, demos.filled = 0, args.demo_steps  # what the fill below leaves: the learner refuses an empty ring
    learner = SACLearner(env, seed=args.seed, hidden_width=args.hidden_width, batch_size=args.batch_size,
                         device_action_gradient=args.device_action_gradient, device_critic_gradient=args.device_critic_gradient,
                         device_actor_gradient=args.device_actor_gradient, device_optimizer=args.device_optimizer,
                         device_entropy=args.device_entropy, n_steps=args.n_steps,
                         **(dict(prioritized=True, per_beta=args.per_beta, per_beta_steps=args.per_beta_steps) if args.prioritized else {}),
                         **(dict(hindsight=True, her_n_sampled_goal=args.her_n_sampled_goal, her_strategy=args.her_strategy) if args.hindsight else {}),
                         **(dict(max_grad_norm=args.max_grad_norm) if args.max_grad_norm is not None else {}),
                         **(dict(bc_weight=args.bc_weight, bc_scale_by_q=args.bc_scale_by_q, bc_q_filter=args.bc_q_filter) if args.bc_weight is not None else {}),
                         **(dict(bc_advantage_temperature=args.bc_advantage_temperature, bc_advantage_max_weight=args.bc_advantage_max_weight)
                            if args.bc_advantage_temperature is not None else {}),
                         **(dict(demonstrations=demos, demo_batch_size=args.demo_batch_size, bc_demo_only=args.bc_demo_only) if args.demo_batch_size is not None else {}),
                         **(dict(normalize=True, norm_obs=not args.no_norm_obs, norm_reward=not args.no_norm_reward, clip_obs=args.clip_obs,
                                 clip_reward=args.clip_reward, norm_epsilon=args.norm_epsilon) if args.normalize else {}))
    normalizer = learner.normalizer  # None without --normalize
    eval_actor = DeviceActor(host_arrays(learner.actor.tensors()), test_env)  # actors belong to the environment they were made for
    replay = DevicePrioritizedReplay(env, args.capacity, alpha=args.per_alpha) if args.prioritized else DeviceReplay(env, args.capacity)
    planner, t_demo = None, time.perf_counter()

    def make_planner(of_env, guide=None):
        guided = args.planner_policy_samples > 0 or args.planner_terminal_value
        if guide is not None:
            import numpy as np

            return DeviceMPPI(of_env, samples=args.planner_samples, horizon=args.planner_horizon, sigma=args.planner_sigma, lam=args.planner_lam,
                              gamma=learner.hp["gamma"] if args.planner_terminal_value else 1.0, seed=args.seed, actor=dict(np.load(guide[0])) if guided else None,
                              critic=[dict(np.load(p)) for p in guide[1:]] if args.planner_terminal_value else None, policy_samples=args.planner_policy_samples,
                              policy_sigma=args.planner_policy_sigma if args.planner_policy_samples else 0.0, terminal_value=args.planner_terminal_value,
                              fail_cost=args.planner_fail_cost, iterations=args.planner_iterations, elites=args.planner_elites, adapt_std=args.planner_adapt_std,
                              std_min=args.planner_std_min, std_max=args.planner_std_max, ess_target=args.planner_ess_target, noise_beta=args.planner_noise_beta)
        return DeviceMPPI(of_env, samples=args.planner_samples, horizon=args.planner_horizon, sigma=args.planner_sigma, lam=args.planner_lam,
                             gamma=learner.hp["gamma"] if args.planner_terminal_value else 1.0, seed=args.seed,
                             actor=host_arrays(learner.actor.tensors()) if guided else None,
                             critic=host_arrays(learner.critic.tensors()) if args.planner_terminal_value else None,
                             policy_samples=args.planner_policy_samples, policy_sigma=args.planner_policy_sigma if args.planner_policy_samples else 0.0,
                             terminal_value=args.planner_terminal_value, fail_cost=args.planner_fail_cost, iterations=args.planner_iterations,
                             elites=args.planner_elites, adapt_std=args.planner_adapt_std, std_min=args.planner_std_min, std_max=args.planner_std_max,
                             ess_target=args.planner_ess_target, noise_beta=args.planner_noise_beta)

    if args.planner:  # guided by copies of the learner's own networks, kept current by sync_planner
        planner = make_planner(env)
    if demos is not None and not args.demo_load:  # the demonstrations: the planner's own transitions on the second env, T steps into T slots
        demos.cursor = demos.filled = 0
        if args.demo_controller:
            demonstrator = DeviceReachController(demo_env, damping=args.demo_damping, gain=args.demo_gain, seed=args.seed)
            demos.collect_scripted(demonstrator, args.demo_steps, first_draw=0, explore_sigma=args.planner_explore_sigma)
        else:
            demonstrator = make_planner(demo_env, args.demo_guide)
            demos.collect_planned(demonstrator, args.demo_steps, first_draw=0, explore_sigma=args.planner_explore_sigma)
        torch.cuda.synchronize()
        ok = demos.ring["is_success"].float().mean().item()
        print(json.dumps({"demonstrator": "controller" if args.demo_controller else "planner", "demo_steps": args.demo_steps, "demo_envs": args.demo_envs, "demo_transitions": len(demos), "demo_success_flag_share": ok,
                          "demo_mean_reward": demos.ring["reward"].mean().item(), "seconds": round(time.perf_counter() - t_demo, 1)}), flush=True)
        demonstrator.close()
    if demos is not None and args.demo_save:
        demos.save(args.demo_save)
    updates, t0 = 0, time.perf_counter()
    best = dict(mean=-float("inf"), tensors=None)  # the Python route's own best_model
    if args.monitor and args.log_every < 1:
        raise SystemExit("--log-every must be at least 1")
    mon = DeviceMonitor(env, capacity=max(1, args.steps // args.log_every)) if args.monitor else None

    latest = {}  # --max-grad-norm, --bc-weight on the Python route: the losses the latest update returned (device tensors)
    with_losses = args.max_grad_norm is not None or args.bc_weight is not None  # the evaluation lines carry the latest update's values

    def cloned_share(values):
        """bc_rows of a line becomes the share of the batch that was cloned."""
        if "bc_rows" in values:
            if args.bc_demo_only and args.demo_batch_size:  # only demonstration rows can be cloned: their cloned share as well
                values["bc_cloned_share_of_demos"] = values["bc_rows"] / args.demo_batch_size
            values["bc_cloned_share"] = values.pop("bc_rows") / args.batch_size
        return values

    def evaluate():
        eval_actor.load_parameters(learner.actor.tensors())
        test_env.reset(seed=args.seed + 1)
        res = run_closed_loop_device(test_env, eval_actor, **(dict(normalizer=normalizer) if normalizer is not None and not args.no_norm_obs else {}))
        norms = {}
        if with_losses:  # the run is synchronised here anyway
            norms = {k: float(v) for k, v in latest.items()}
            keys = (("critic_grad_norm", "actor_grad_norm") if args.max_grad_norm is not None else ()) + (("bc_loss", "bc_weight", "bc_rows") if args.bc_weight is not None else ()) + \
                (("adv_ess", "adv_max", "adv_clipped") if args.bc_advantage_temperature is not None else ())
            norms.update({k: float(learner.last_update[k][0]) for k in keys})
            cloned_share(norms)
        if args.save_best and res["mean_episode_reward"] > best["mean"]:  # strictly above, as the reference's EvalCallback decides
            best.update(mean=res["mean_episode_reward"], tensors=host_arrays(learner.actor.tensors()))
            if normalizer is not None:  # the statistics it was selected under, as DeviceEvaluation.save_best writes them
                import numpy as np

                o = normalizer.options
                best["norm"] = {"norm/" + k: v.cpu().numpy() for k, v in normalizer.state.items() if k != "running_ret"}
                best["norm"]["norm/options"] = np.array([o["gamma"], o["epsilon"], o["clip_obs"], o["clip_reward"], float(o["norm_obs"]), float(o["norm_reward"])])
        print(json.dumps({"updates": updates, "env_steps": learner.env_steps * env.num_envs, "seconds": round(time.perf_counter() - t0, 1),
                          "mean_episode_return": res["mean_episode_reward"], "success_rate_percent": res["success_rate_percent"], **norms}), flush=True)

    if args.init_from:
        import numpy as np

        actor = dict(np.load(args.init_from[0]))
        learner.load_parameters(actor=actor, critics=[dict(np.load(p)) for p in args.init_from[1:]])

    # the whole run's schedule, counted from its first trip whether this process starts there or resumes: an evaluation falls at the
    # end of every trip in which the update count passes a multiple of --eval-every (evaluation.evaluation_points); warm-up trips run
    # no update
    _, idle = warmup_iterations(0, env.num_envs, learner.hp["learning_starts"], args.steps, 1)
    points = evaluation_points(1, args.steps, args.updates_per_step, idle, args.eval_every) if args.steps > 0 else []
    ev = DeviceEvaluation(test_env, learner.actor.tensors(), seed=args.seed + 1, capacity=max(1, len(points)),
                          **(dict(normalizer=normalizer) if normalizer is not None else {})) if args.native else None
    parts = dict(replay=replay, monitor=mon, evaluation=ev, **(dict(demonstrations=demos) if args.demo_batch_size is not None else {}))
    step = shown_evals = shown_curve = 0
    if args.resume:
        extra = learner.load(args.resume, **parts)  # refuses another env, width, option set or hyperparameter, naming it
        step, updates, best["mean"] = int(extra["trips"]), int(extra["updates"]), float(extra["best_mean"])
        shown_evals, shown_curve = (ev.count if ev is not None else 0), (mon.count if mon is not None else 0)
        if step > args.steps:
            raise SystemExit(f"--resume: the checkpoint is {step} trips into the run, --steps asks for {args.steps} in all")

    def save(trips):
        learner.save(args.save, **parts, extra=dict(trips=trips, updates=updates, best_mean=best["mean"]))

    def print_curve(seconds):
        for rec in mon.results()[shown_curve:]:  # synchronises
            print(json.dumps({"trips": rec["iteration"], "env_steps": rec["iteration"] * env.num_envs, "seconds": seconds, "train_episodes": rec["episodes"],
                              "train_mean_return": rec["mean_return"], "train_mean_length": rec["mean_length"],
                              "train_success_rate_percent": 100.0 * rec["success_rate"]}), flush=True)

    def print_plan_stats(seconds):
        recs = planner.plan_stats(shown_curve, mon.count - shown_curve)  # beside the monitor's records, at their indices; synchronises
        for i, rec in enumerate(recs):
            last = {}
            if planner.temper() is not None and i == len(recs) - 1 and rec["iteration"] == step:  # the buffers hold the last plan of the call
                lam, how = planner.buf["lam_out"].cpu().numpy(), planner.buf["saturated"].cpu().numpy()
                last = dict(plan_mean_lam=float(lam.mean()), plan_at_lam_max=int((how == 1).sum()), plan_at_lam_min=int((how == 2).sum()))
            print(json.dumps({"trips": rec["iteration"], "seconds": seconds, "plan_envs": rec["num_parents"], "plan_planned": rec["planned"],
                              "plan_mean_best_return": rec["mean_best_return"], "plan_mean_nominal_return": rec["mean_nominal_return"],
                              "plan_mean_gain": rec["mean_gain"], "plan_mean_ess": rec["mean_ess"], "plan_min_ess": rec["min_ess"],
                              **(dict(plan_mean_elite_count=rec["mean_elite_count"], plan_mean_threshold=rec["mean_threshold"])
                                 if planner.adapt() is not None else {}), **last}), flush=True)

    if args.native:
        # one call for the whole run -- or, with --save-every, one per stretch between two checkpoints: split calls are bit for bit the
        # single one (the schedule's counters are handed on), so the checkpoints cost the launches nothing but their own copies
        stretch = max(1, -(-args.save_every // max(1, args.updates_per_step))) if args.save_every else max(1, args.steps)
        first_update, curves = updates, []  # --max-grad-norm, --bc-weight: the losses, norms and cloning values of every update of this process, one entry per call
        while step < args.steps:
            n = min(stretch, args.steps - step)
            got = learner.train(replay, n, 1, args.updates_per_step, seed=args.seed, first_draw=updates, evaluation=ev, eval_every=args.eval_every,
                                **(dict(monitor=mon, log_every=args.log_every) if mon is not None else {}),
                                **(dict(planner=planner, explore_sigma=args.planner_explore_sigma, plan_stats=mon is not None) if planner is not None else {}))
            if with_losses:
                curves.append({k: v for k, v in got.items() if k != "plan_stats"})
            step, updates = step + n, learner.adam_state["step"]
            if args.save and (args.save_every or step == args.steps):
                save(step)
        seconds = None
        curve = {k: torch.cat([c[k] for c in curves]).cpu().numpy() for k in curves[0]} if curves else {}  # after the run: synchronises
        for trip, rec in list(zip(points, ev.results()))[shown_evals:]:  # results() synchronises, once
            seconds = round(time.perf_counter() - t0, 1) if seconds is None else seconds
            done = max(0, trip + 1 - idle) * args.updates_per_step
            norms = cloned_share({k: float(v[done - 1 - first_update]) for k, v in curve.items()}) if curve and done - 1 >= first_update else {}
            print(json.dumps({"updates": done, "env_steps": (trip + 1) * env.num_envs, "seconds": seconds, "mean_episode_return": rec["mean_return"],
                              "success_rate_percent": 100.0 * rec["success_rate"], "std_episode_return": rec["std_return"],
                              "mean_episode_length": rec["mean_length"], "improved": bool(rec["improved"]), **norms}), flush=True)
        if "adv_ess" in curve and curve["adv_ess"].size:  # the weights' effective sample size over every update of this process
            ess, rows = curve["adv_ess"], curve["bc_rows"]
            print(json.dumps({"adv_updates": int(ess.size), "adv_ess_mean": float(ess.mean()), "adv_ess_min": float(ess.min()), "adv_ess_max": float(ess.max()),
                              "adv_ess_share_of_rows_mean": float((ess / rows.clip(1)).mean()), "adv_max_mean": float(curve["adv_max"].mean()),
                              "adv_clipped_mean": float(curve["adv_clipped"].mean())}), flush=True)
        if mon is not None:
            print_curve(round(time.perf_counter() - t0, 1) if seconds is None else seconds)
            if planner is not None:
                print_plan_stats(round(time.perf_counter() - t0, 1) if seconds is None else seconds)
        if args.save_best and ev.best_state()[1] >= 0:
            ev.save_best(args.save_best)
    for step in range(step, args.steps):  # the Python loop (every trip of it where --native is off)
        learner.collect(replay, 1, monitor=mon, **(dict(planner=planner, explore_sigma=args.planner_explore_sigma) if planner is not None else {}))
        if mon is not None and (step + 1) % args.log_every == 0:
            mon.record(step + 1)
        if learner.env_steps * env.num_envs < learner.hp["learning_starts"]:
            continue
        for _ in range(args.updates_per_step):
            latest = learner.update(replay, args.seed, updates)
            updates += 1
            if updates % args.eval_every == 0:
                evaluate()
        if planner is not None:  # the next plan uses the parameters these updates left
            learner.sync_planner(planner)
        if args.save_every and updates // args.save_every > (updates - args.updates_per_step) // args.save_every:
            save(step + 1)  # this trip is done
    if not args.native:
        if mon is not None:
            print_curve(round(time.perf_counter() - t0, 1))
        if args.save:
            save(args.steps)
    if ev is not None:
        ev.close()
    if args.save_best and best["tensors"] is not None:
        save_actor(args.save_best, best["tensors"], best.get("norm"))
    eval_actor.close()
    if planner is not None:
        planner.close()
    learner.close()
    test_env.close()
    env.close()
    if demo_env is not None:
        demo_env.close()


if __name__ == "__main__":
    main()
