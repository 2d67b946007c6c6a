"""ctypes mirror of include/urgym.h (struct layouts and constants only; no library is loaded here)."""
import ctypes as C

ABI_VERSION = 4

ENV_ORI, ENV_OBS, ENV_DYN, ENV_STA = 0, 1, 2, 3
ENV_IDS = {"UR5OriReach-v1": ENV_ORI, "UR5ObsReach-v1": ENV_OBS, "UR5DynReach-v1": ENV_DYN, "UR5StaReach-v1": ENV_STA}

OK, ERR_ARG, ERR_HIP, ERR_STATE = 0, -1, -2, -3

STATUS_NAN = 1
STATUS_RESET_EXHAUSTED = 2
STATUS_RESET_COLLISION = 4
STATUS_PENETRATION = 8
STATUS_GJK_ITER = 16
STATUS_JOINT_LIMIT = 32
STATUS_STALE_RECORD = 64

OBS_DIMS = {ENV_ORI: (18, 6), ENV_OBS: (26, 3), ENV_DYN: (35, 6), ENV_STA: (29, 6)}  # (observation, goal) — core.py:241-247

GJK_START_BULLET, GJK_START_GUIDED = 0, 1  # urgym_config.gjk_start (include/urgym.h)
LINK_DIST_OBSTACLE, LINK_DIST_WORKBENCH = 0, 1  # urgym_config.link_dist_scope (include/urgym.h)
KEEP_SEED = 0xFFFFFFFFFFFFFFFF


class Config(C.Structure):
    _fields_ = [
        ("env_kind", C.c_int32),
        ("num_envs", C.c_int32),
        ("max_episode_steps", C.c_int32),
        ("auto_reset", C.c_int32),
        ("check_collision", C.c_int32),
        ("max_reset_tries", C.c_int32),
        ("dyn_motion_steps", C.c_int32),
        ("gjk_start", C.c_int32),
        ("link_dist_scope", C.c_int32),
        ("reserved0", C.c_int32),
        ("action_scale", C.c_double),
        ("dt", C.c_double),
        ("distance_threshold", C.c_double),
        ("ori_threshold", C.c_double),
        ("w_collision", C.c_double),
        ("w_success", C.c_double),
        ("w_distance", C.c_double),
        ("w_orientation", C.c_double),
        ("w_link", C.c_double * 5),
        ("near_threshold", C.c_double),
        ("collision_margin", C.c_double),
        ("target_clearance", C.c_double),
        ("min_travel", C.c_double),
        ("dyn_time_duration", C.c_double),
        ("goal_low", C.c_double * 3),
        ("goal_high", C.c_double * 3),
        ("obst_low", C.c_double * 3),
        ("obst_high", C.c_double * 3),
        ("neutral_q", C.c_double * 6),
    ]


# name -> (ctype of element, leading shape given (N, obs_dim, goal_dim), is_state)
BUFFER_FIELDS = [
    ("q", C.c_double, lambda N, od, gd: (6, N)),
    ("goal", C.c_double, lambda N, od, gd: (6, N)),
    ("obst_start", C.c_double, lambda N, od, gd: (6, N)),
    ("obst_end", C.c_double, lambda N, od, gd: (6, N)),
    ("obst_pos", C.c_double, lambda N, od, gd: (3, N)),
    ("obst_quat", C.c_double, lambda N, od, gd: (4, N)),
    ("obst_vel", C.c_double, lambda N, od, gd: (9, N)),
    ("link_dist", C.c_double, lambda N, od, gd: (5, N)),
    ("step_count", C.c_int32, lambda N, od, gd: (N,)),
    ("episode_id", C.c_int32, lambda N, od, gd: (N,)),
    ("observation", C.c_float, lambda N, od, gd: (N, od)),
    ("achieved_goal", C.c_float, lambda N, od, gd: (N, gd)),
    ("desired_goal", C.c_float, lambda N, od, gd: (N, gd)),
    ("reward", C.c_float, lambda N, od, gd: (N,)),
    ("terminated", C.c_uint8, lambda N, od, gd: (N,)),
    ("truncated", C.c_uint8, lambda N, od, gd: (N,)),
    ("is_success", C.c_uint8, lambda N, od, gd: (N,)),
    ("collision", C.c_uint8, lambda N, od, gd: (N,)),
    ("final_observation", C.c_float, lambda N, od, gd: (N, od)),
    ("final_achieved_goal", C.c_float, lambda N, od, gd: (N, gd)),
    ("final_desired_goal", C.c_float, lambda N, od, gd: (N, gd)),
    ("status", C.c_int32, lambda N, od, gd: (N,)),
    ("done_list", C.c_int32, lambda N, od, gd: (N,)),
    ("done_count", C.c_int32, lambda N, od, gd: (2,)),
]


class Buffers(C.Structure):
    _fields_ = [(name, C.POINTER(ct)) for name, ct, _ in BUFFER_FIELDS]


class ActorDesc(C.Structure):
    """urgym_actor_desc: dimensions + six HOST pointers to float32 arrays in torch's [out][in] layout."""
    _fields_ = [
        ("in_features", C.c_int32),
        ("hidden_width", C.c_int32),
        ("action_dim", C.c_int32),
        ("reserved0", C.c_int32),
        ("w0", C.POINTER(C.c_float)),
        ("b0", C.POINTER(C.c_float)),
        ("w1", C.POINTER(C.c_float)),
        ("b1", C.POINTER(C.c_float)),
        ("w_mu", C.POINTER(C.c_float)),
        ("b_mu", C.POINTER(C.c_float)),
    ]


# urgym_trajectory: name -> (ctype of element, shape given (K, N, obs_dim, goal_dim)); every pointer may be NULL
TRAJECTORY_FIELDS = [
    ("observation", C.c_float, lambda K, N, od, gd: (K, N, od)),
    ("achieved_goal", C.c_float, lambda K, N, od, gd: (K, N, gd)),
    ("desired_goal", C.c_float, lambda K, N, od, gd: (K, N, gd)),
    ("action", C.c_float, lambda K, N, od, gd: (K, N, 6)),
    ("reward", C.c_float, lambda K, N, od, gd: (K, N)),
    ("terminated", C.c_uint8, lambda K, N, od, gd: (K, N)),
    ("truncated", C.c_uint8, lambda K, N, od, gd: (K, N)),
    ("is_success", C.c_uint8, lambda K, N, od, gd: (K, N)),
    ("collision", C.c_uint8, lambda K, N, od, gd: (K, N)),
    ("final_observation", C.c_float, lambda K, N, od, gd: (K, N, od)),
    ("episode_return", C.c_double, lambda K, N, od, gd: (N,)),
    ("episode_last_step", C.c_int32, lambda K, N, od, gd: (N,)),
    ("episode_success", C.c_uint8, lambda K, N, od, gd: (N,)),
    ("episode_done", C.c_uint8, lambda K, N, od, gd: (N,)),
]


class Trajectory(C.Structure):
    _fields_ = [(name, C.POINTER(ct)) for name, ct, _ in TRAJECTORY_FIELDS]


SAMPLE_MEAN, SAMPLE_GAUSSIAN, SAMPLE_UNIFORM = 0, 1, 2  # urgym_sampling.mode
SAMPLE_MODES = {"mean": SAMPLE_MEAN, "gaussian": SAMPLE_GAUSSIAN, "uniform": SAMPLE_UNIFORM}
NOISE_TAG = 0x504F4C00  # word 3 of the policy noise's Philox counter is NOISE_TAG | block


class Sampling(C.Structure):
    """urgym_sampling: how urgym_actor_sample / urgym_rollout_sampled draw."""
    _fields_ = [("mode", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64), ("first_draw", C.c_uint64)]


# urgym_sample_records: name -> (ctype of element, shape given (K, N)); every pointer may be NULL
SAMPLE_RECORD_FIELDS = [
    ("log_prob", C.c_float, lambda K, N: (K, N)),
    ("noise", C.c_float, lambda K, N: (K, N, 6)),
    ("mean_action", C.c_float, lambda K, N: (K, N, 6)),
    ("log_std", C.c_float, lambda K, N: (K, N, 6)),
]


class SampleRecords(C.Structure):
    _fields_ = [(name, C.POINTER(ct)) for name, ct, _ in SAMPLE_RECORD_FIELDS]


class QNetwork(C.Structure):
    """urgym_q_network: six HOST pointers to float32 arrays in torch's [out][in] layout."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("w0", "b0", "w1", "b1", "w_q", "b_q")]


class CriticDesc(C.Structure):
    """urgym_critic_desc: dimensions + the two Q-networks."""
    _fields_ = [
        ("in_features", C.c_int32),
        ("hidden_width", C.c_int32),
        ("n_critics", C.c_int32),
        ("reserved0", C.c_int32),
        ("qf", QNetwork * 2),
    ]


class CriticRows(C.Structure):
    """urgym_critic_rows: DEVICE pointers to `count` rows; observation NULL = the bound buffers."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("observation", "achieved_goal", "desired_goal", "action")]


class CriticTerms(C.Structure):
    """urgym_critic_terms: the terms of the SAC target; every pointer may be NULL."""
    _fields_ = [
        ("reward", C.POINTER(C.c_float)),
        ("terminated", C.POINTER(C.c_uint8)),
        ("log_prob", C.POINTER(C.c_float)),
        ("gamma", C.c_float),
        ("ent_coef", C.c_float),
    ]


class CriticOut(C.Structure):
    """urgym_critic_out: what urgym_critic_evaluate writes; every pointer may be NULL, not all."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("q", "q_min", "target")]


class CriticGradOut(C.Structure):
    """urgym_critic_grad_out: what urgym_critic_action_gradient writes; every pointer may be NULL, not both of the first two."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("dq_da", "dqmin_da", "q", "q_min")]


class QNetworkGrad(C.Structure):
    """urgym_q_network_grad: six DEVICE pointers the gradients of one Q-network are written to, torch's [out][in] layout."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("w0", "b0", "w1", "b1", "w_q", "b_q")]


class CriticParamGrads(C.Structure):
    """urgym_critic_param_grads: where urgym_critic_parameter_gradients writes; q may be NULL."""
    _fields_ = [("qf", QNetworkGrad * 2), ("q", C.POINTER(C.c_float))]


CRITIC_GRADIENTS_MAX_COUNT = 65536  # URGYM_CRITIC_GRADIENTS_MAX_COUNT

ACTOR_GRAD_ARRAYS = ("w0", "b0", "w1", "b1", "w_mu", "b_mu", "w_log_std", "b_log_std")  # urgym_actor_params_dev's eight, all required
ACTOR_GRAD_RECORDS = ("action", "log_prob", "noise", "log_std", "d_mu", "d_log_std", "std")  # optional per-row outputs, each may be NULL


class ActorUpstream(C.Structure):
    """urgym_actor_upstream: the SAMPLE form (d_action, d_log_prob or NULL) or the HEADS form (d_mu and d_log_std); DEVICE pointers."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("d_action", "d_log_prob", "d_mu", "d_log_std")]


class ActorParamGrads(C.Structure):
    """urgym_actor_param_grads: where urgym_actor_parameter_gradients writes: eight tensors, then the optional per-row outputs."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ACTOR_GRAD_ARRAYS + ACTOR_GRAD_RECORDS]


ACTOR_GRADIENTS_MAX_COUNT = 65536  # URGYM_ACTOR_GRADIENTS_MAX_COUNT

REPLAY_TAG = 0x52504C00  # word 3 of the Philox counter of urgym_replay_sample's index draw
DEMO_TAG = 0x44454D00  # URGYM_DEMO_TAG: word 3 of the counter of a draw from the demonstrations (urgym_replay_sample_mixed)

# urgym_replay_ring after capacity_steps / reserved0: name -> (ctype of element, shape given (C, N, obs_dim, goal_dim), required)
REPLAY_RING_FIELDS = [
    ("observation", C.c_float, lambda Cs, N, od, gd: (Cs, N, od), True),
    ("achieved_goal", C.c_float, lambda Cs, N, od, gd: (Cs, N, gd), True),
    ("desired_goal", C.c_float, lambda Cs, N, od, gd: (Cs, N, gd), True),
    ("action", C.c_float, lambda Cs, N, od, gd: (Cs, N, 6), True),
    ("reward", C.c_float, lambda Cs, N, od, gd: (Cs, N), True),
    ("next_observation", C.c_float, lambda Cs, N, od, gd: (Cs, N, od), True),
    ("next_achieved_goal", C.c_float, lambda Cs, N, od, gd: (Cs, N, gd), True),
    ("next_desired_goal", C.c_float, lambda Cs, N, od, gd: (Cs, N, gd), True),
    ("terminated", C.c_uint8, lambda Cs, N, od, gd: (Cs, N), True),
    ("truncated", C.c_uint8, lambda Cs, N, od, gd: (Cs, N), False),
    ("is_success", C.c_uint8, lambda Cs, N, od, gd: (Cs, N), False),
]


class ReplayRing(C.Structure):
    """urgym_replay_ring: the caller's ring of C slots x N transitions (DEVICE pointers)."""
    _fields_ = [("capacity_steps", C.c_int32), ("reserved0", C.c_int32)] + [(name, C.POINTER(ct)) for name, ct, _, _ in REPLAY_RING_FIELDS]


class ReplayBatch(C.Structure):
    """urgym_replay_batch: what urgym_replay_sample writes, `count` rows each; every pointer may be NULL, not all."""
    _fields_ = [(name, C.POINTER(ct)) for name, ct, _, _ in REPLAY_RING_FIELDS] + [("index", C.POINTER(C.c_int64))]


ACTOR_DEV_ARRAYS = ("w0", "b0", "w1", "b1", "w_mu", "b_mu", "w_log_std", "b_log_std")  # the last two may be NULL, together


class ActorParamsDev(C.Structure):
    """urgym_actor_params_dev: the shape for checking + eight DEVICE pointers to float32 tensors in torch's [out][in] layout."""
    _fields_ = [("in_features", C.c_int32), ("hidden_width", C.c_int32), ("reserved0", C.c_int32)] + [(name, C.POINTER(C.c_float)) for name in ACTOR_DEV_ARRAYS]


class QNetworkDev(C.Structure):
    """urgym_q_network_dev: six DEVICE pointers to float32 tensors in torch's [out][in] layout."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("w0", "b0", "w1", "b1", "w_q", "b_q")]


class CriticParamsDev(C.Structure):
    """urgym_critic_params_dev: the shape for checking + the two Q-networks."""
    _fields_ = [("in_features", C.c_int32), ("hidden_width", C.c_int32), ("reserved0", C.c_int32), ("qf", QNetworkDev * 2)]


class ActorParamsOut(C.Structure):
    """urgym_actor_params_out: ActorParamsDev with pointers that are written (urgym_actor_unpack)."""
    _fields_ = list(ActorParamsDev._fields_)


class QNetworkOut(C.Structure):
    """urgym_q_network_out: QNetworkDev with pointers that are written."""
    _fields_ = list(QNetworkDev._fields_)


class CriticParamsOut(C.Structure):
    """urgym_critic_params_out: the shape for checking + the two Q-networks that are written (urgym_critic_unpack)."""
    _fields_ = [("in_features", C.c_int32), ("hidden_width", C.c_int32), ("reserved0", C.c_int32), ("qf", QNetworkOut * 2)]


class AdamHyper(C.Structure):
    """urgym_adam_hyper: Adam's hyperparameters and the 1-based index of this step (the caller counts; the library keeps no state)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("step", C.c_int64), ("reserved0", C.c_int32)]


ADAM_COEFFICIENTS = ("b1", "omb1", "b2", "omb2", "step_size", "bc2_sqrt", "eps")  # the float[7] of urgym_adam_coefficients, in order
ADAM_SETS = ("param", "grad", "exp_avg", "exp_avg_sq")  # the four tensor sets of urgym_actor_adam / urgym_critic_adam, in order


class ActorTensors(C.Structure):
    """urgym_actor_tensors / urgym_actor_tensors_const: eight DEVICE pointers named like urgym_actor_params_dev's."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ACTOR_DEV_ARRAYS]


class ActorAdam(C.Structure):
    """urgym_actor_adam: the shape for checking + 4 x 8 DEVICE pointers, all required."""
    _fields_ = [("in_features", C.c_int32), ("hidden_width", C.c_int32), ("reserved0", C.c_int32)] + [(name, ActorTensors) for name in ADAM_SETS]


class CriticAdam(C.Structure):
    """urgym_critic_adam: the shape for checking + 4 x 2 x 6 DEVICE pointers, all required."""
    _fields_ = [("in_features", C.c_int32), ("hidden_width", C.c_int32), ("reserved0", C.c_int32)] + [(name, QNetworkDev * 2) for name in ADAM_SETS]


SAC_TERMS_MAX_COUNT = 65536  # URGYM_SAC_TERMS_MAX_COUNT: the row cap of urgym_sac_entropy_step / urgym_sac_policy_terms
SAC_TERMS_LANES = 1024       # the lanes of their one workgroup: the stride of the ordered sum


class SacEntropyArgs(C.Structure):
    """urgym_sac_entropy_args: the rows, the state (stepped in place), alpha and the loss, the optional target and upstream groups."""
    _fields_ = [("count", C.c_int32), ("reserved0", C.c_int32), ("target_entropy", C.c_float), ("gamma", C.c_float), ("scale", C.c_float),
                ("log_prob", C.POINTER(C.c_float)), ("log_ent_coef", C.POINTER(C.c_float)), ("exp_avg", C.POINTER(C.c_float)),
                ("exp_avg_sq", C.POINTER(C.c_float)), ("ent_coef_out", C.POINTER(C.c_float)), ("loss_out", C.POINTER(C.c_float)),
                ("target_in", C.POINTER(C.c_float)), ("next_log_prob", C.POINTER(C.c_float)), ("terminated", C.POINTER(C.c_uint8)),
                ("y_out", C.POINTER(C.c_float)), ("d_log_prob_out", C.POINTER(C.c_float))]


class SacPolicyArgs(C.Structure):
    """urgym_sac_policy_args: alpha and the three optional groups (upstream, critic loss, actor loss)."""
    _fields_ = [("count", C.c_int32), ("reserved0", C.c_int32), ("scale", C.c_float), ("ent_coef", C.POINTER(C.c_float)),
                ("dqmin_da", C.POINTER(C.c_float)), ("d_action_out", C.POINTER(C.c_float)),
                ("q", C.POINTER(C.c_float)), ("y", C.POINTER(C.c_float)), ("critic_loss_out", C.POINTER(C.c_float)),
                ("log_prob", C.POINTER(C.c_float)), ("q_min", C.POINTER(C.c_float)), ("actor_loss_out", C.POINTER(C.c_float))]


class SacSchedule(C.Structure):
    """urgym_sac_schedule: where a urgym_sac_train call starts and how long it runs (ur_gym_amd/csrc/urgym_sac_schedule.h)."""
    _fields_ = [(name, C.c_int32) for name in ("first_slot", "filled_steps", "capacity_steps", "num_iterations", "steps_per_iteration",
                                                "updates_per_iteration", "uniform_iterations", "idle_iterations")] + \
               [("collect_first_draw", C.c_uint64), ("update_first_draw", C.c_uint64), ("first_step", C.c_int64)]


# urgym_sac_learner's scratch after the batch: name -> shape given the batch size M; float32, all required, reused by every update
SAC_LEARNER_SCRATCH = [
    ("next_actions", lambda M: (M, 6)), ("next_log_prob", lambda M: (M,)), ("target_value", lambda M: (M,)), ("y", lambda M: (M,)),
    ("action_pi", lambda M: (M, 6)), ("log_prob", lambda M: (M,)), ("q", lambda M: (2, M)), ("q_min", lambda M: (M,)),
    ("dqmin_da", lambda M: (M, 6)), ("d_action", lambda M: (M, 6)), ("d_log_prob", lambda M: (M,)), ("ent_coef", lambda M: (1,)),
]
SAC_LEARNER_STATE = ("log_ent_coef", "exp_avg", "exp_avg_sq")         # the temperature's three [1] tensors
SAC_LEARNER_LOSSES = ("critic_loss", "actor_loss", "ent_coef_loss")  # one float per update of the call each
SAC_LEARNER_OPTIONAL = ("batch.truncated", "batch.is_success", "batch.index")  # the only pointers of the struct that may be NULL
SAC_TRAIN_MAX_COUNT = 65536  # the row cap of the gradient kernels and of the SAC terms


class SacLearner(C.Structure):
    """urgym_sac_learner: everything the launches of a collection and an update take (objects, Adam tensors, workspaces, the
    temperature's state, the ring, the batch and its scratch, the loss slots, the numbers)."""
    _fields_ = [("actor", C.c_void_p), ("online", C.c_void_p), ("target", C.c_void_p), ("actor_adam", ActorAdam), ("critic_adam", CriticAdam),
                ("actor_workspace", C.c_void_p), ("actor_workspace_bytes", C.c_uint64), ("critic_workspace", C.c_void_p),
                ("critic_workspace_bytes", C.c_uint64)] + \
               [(name, C.POINTER(C.c_float)) for name in SAC_LEARNER_STATE] + [("ring", ReplayRing), ("batch", ReplayBatch)] + \
               [(name, C.POINTER(C.c_float)) for name, _ in SAC_LEARNER_SCRATCH] + [(name, C.POINTER(C.c_float)) for name in SAC_LEARNER_LOSSES] + \
               [("count", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64), ("update_seed", C.c_uint64), ("gamma", C.c_float),
                ("tau", C.c_float), ("target_entropy", C.c_float), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double)]


class EvalRecord(C.Structure):
    """urgym_eval_record: one evaluation as the device reduced it (include/urgym.h states every float); 72 bytes, 8-byte aligned."""
    _fields_ = [(name, C.c_double) for name in ("mean_return", "var_return", "mean_length", "success_rate", "best_mean_after")] + \
               [("eval_index", C.c_int64), ("length_sum", C.c_int64)] + \
               [(name, C.c_int32) for name in ("successes", "count", "improved", "reserved0")]


EVAL_RECORD_WORDS = 9  # an EvalRecord as int64 words: how a torch tensor holds an array of them
EVAL_MAX_COUNT = SAC_TERMS_MAX_COUNT  # the cap on the evaluation envs: one workgroup reduces them


class EvalStatsArgs(C.Structure):
    """urgym_eval_stats_args: the three episode arrays, the best state (read and written) and the record to write; DEVICE pointers."""
    _fields_ = [("count", C.c_int32), ("reserved0", C.c_int32), ("eval_index", C.c_int64), ("episode_return", C.POINTER(C.c_double)),
                ("episode_last_step", C.POINTER(C.c_int32)), ("episode_success", C.POINTER(C.c_uint8)), ("best_mean", C.POINTER(C.c_double)),
                ("best_index", C.POINTER(C.c_int64)), ("record", C.POINTER(EvalRecord))]


class ActorSnapshotArgs(C.Structure):
    """urgym_actor_snapshot_args: source -> destination, all sixteen tensors, under the DEVICE flag `when` (NULL = always)."""
    _fields_ = [("in_features", C.c_int32), ("hidden_width", C.c_int32), ("source", ActorTensors), ("destination", ActorTensors),
                ("when", C.POINTER(C.c_int32)), ("reserved0", C.c_int32)]


class PolicyEvaluation(C.Structure):
    """urgym_policy_evaluation: the eval actor, the source and the best tensors, the [N] scratch, the records and the best state."""
    _fields_ = [("eval_actor", C.c_void_p), ("in_features", C.c_int32), ("hidden_width", C.c_int32), ("source", ActorTensors), ("best", ActorTensors),
                ("episode_return", C.POINTER(C.c_double)), ("episode_last_step", C.POINTER(C.c_int32)), ("episode_success", C.POINTER(C.c_uint8)),
                ("episode_done", C.POINTER(C.c_uint8)), ("records", C.POINTER(EvalRecord)), ("best_mean", C.POINTER(C.c_double)),
                ("best_index", C.POINTER(C.c_int64)), ("reset_seed", C.c_uint64), ("record_capacity", C.c_int32), ("num_steps", C.c_int32),
                ("reserved0", C.c_int32)]


class SacEvaluation(C.Structure):
    """urgym_sac_evaluation: the evaluation handle, the evaluation, the interval in updates and where the call's records start."""
    _fields_ = [("eval_handle", C.c_void_p), ("evaluation", PolicyEvaluation), ("every", C.c_int32), ("first_record_slot", C.c_int32),
                ("first_eval_index", C.c_int64)]


# urgym_monitor_state: name -> ctype of the six [N] DEVICE arrays, in the struct's order
MONITOR_STATE_FIELDS = [("running_return", C.c_double), ("running_length", C.c_int32), ("sum_return", C.c_double), ("sum_length", C.c_int64),
                        ("episodes", C.c_int32), ("successes", C.c_int32)]


class MonitorState(C.Structure):
    """urgym_monitor_state: per env the episode in progress and the episodes finished since the last clear; all zero is the start."""
    _fields_ = [(name, C.POINTER(ct)) for name, ct in MONITOR_STATE_FIELDS]


class MonitorRecord(C.Structure):
    """urgym_monitor_record: the training episodes finished since the last clear as the device reduced them; 72 bytes, 8-byte aligned."""
    _fields_ = [(name, C.c_double) for name in ("mean_return", "mean_length", "success_rate", "sum_return")] + \
               [(name, C.c_int64) for name in ("episodes", "length_sum", "successes", "iteration", "reserved0")]


MONITOR_RECORD_WORDS = 9  # a MonitorRecord as int64 words: how a torch tensor holds an array of them


class SacMonitoring(C.Structure):
    """urgym_sac_monitoring: the state, the records, where the call's records start, the interval in iterations and the caller's count."""
    _fields_ = [("state", MonitorState), ("records", C.POINTER(MonitorRecord)), ("record_capacity", C.c_int32), ("first_record", C.c_int32),
                ("log_every", C.c_int32), ("clear", C.c_int32), ("first_iteration", C.c_int64), ("reserved0", C.c_int64)]


REPLAY_NSTEP_MAX = 32  # URGYM_REPLAY_NSTEP_MAX: the longest window of urgym_replay_sample_nstep


class ReplayNstep(C.Structure):
    """urgym_replay_nstep: the window and gamma of urgym_replay_sample_nstep and its three extra outputs (discount required)."""
    _fields_ = [("n_steps", C.c_int32), ("reserved0", C.c_int32), ("gamma", C.c_float), ("reserved1", C.c_float),
                ("discount", C.POINTER(C.c_float)), ("steps", C.POINTER(C.c_int32)), ("last_index", C.POINTER(C.c_int64))]


class SacEntropyNstepArgs(C.Structure):
    """urgym_sac_entropy_nstep_args: SacEntropyArgs with the target group of a per-row discount (reward, q_min_next, discount)."""
    _fields_ = [("count", C.c_int32), ("reserved0", C.c_int32), ("target_entropy", C.c_float), ("scale", C.c_float),
                ("log_prob", C.POINTER(C.c_float)), ("log_ent_coef", C.POINTER(C.c_float)), ("exp_avg", C.POINTER(C.c_float)),
                ("exp_avg_sq", C.POINTER(C.c_float)), ("ent_coef_out", C.POINTER(C.c_float)), ("loss_out", C.POINTER(C.c_float)),
                ("reward", C.POINTER(C.c_float)), ("q_min_next", C.POINTER(C.c_float)), ("discount", C.POINTER(C.c_float)),
                ("next_log_prob", C.POINTER(C.c_float)), ("terminated", C.POINTER(C.c_uint8)), ("y_out", C.POINTER(C.c_float)),
                ("d_log_prob_out", C.POINTER(C.c_float))]


class SacNstep(C.Structure):
    """urgym_sac_nstep: the window of urgym_sac_train_nstep and its two [count] scratch arrays."""
    _fields_ = [("n_steps", C.c_int32), ("reserved0", C.c_int32), ("discount", C.POINTER(C.c_float)), ("q_min_next", C.POINTER(C.c_float))]


HER_HORIZON_MAX = 256  # URGYM_HER_HORIZON_MAX: the longest episode window of urgym_replay_sample_hindsight
HER_GOAL_FUTURE, HER_GOAL_FINAL, HER_GOAL_OWN = 0, 1, 2  # URGYM_HER_GOAL_*
HER_STRATEGIES = {"future": HER_GOAL_FUTURE, "final": HER_GOAL_FINAL, "own": HER_GOAL_OWN}
HER_GOAL_OFFSET = 12  # the goal lies at floats [12, 12 + goal_dim) of an observation row in all four env kinds


class ReplayHindsight(C.Structure):
    """urgym_replay_hindsight: the relabel threshold, the strategy and the horizon of urgym_replay_sample_hindsight and its two
    optional outputs."""
    _fields_ = [("relabel_threshold", C.c_uint64), ("strategy", C.c_int32), ("horizon", C.c_int32), ("goal_index", C.POINTER(C.c_int64)),
                ("pose_terms", C.POINTER(C.c_double)), ("reserved0", C.c_int64)]


class SacHindsight(C.Structure):
    """urgym_sac_hindsight: the rule of urgym_sac_train_hindsight's gathers."""
    _fields_ = [("relabel_threshold", C.c_uint64), ("strategy", C.c_int32), ("horizon", C.c_int32), ("reserved0", C.c_int64)]


GRAD_NORM_ACTOR_TENSORS, GRAD_NORM_CRITIC_TENSORS = 8, 12  # the tensors of the two groups of urgym_*_grad_norm, in their fixed order
GRAD_NORM_EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s: c64 = max_norm / (norm64 + GRAD_NORM_EPS)


class GradNorm(C.Structure):
    """urgym_grad_norm: the bound and the three outputs of urgym_actor_grad_norm / urgym_critic_grad_norm (tensor_sums_out may be NULL)."""
    _fields_ = [("max_norm", C.c_float), ("reserved0", C.c_int32), ("norm_out", C.POINTER(C.c_float)), ("scale_out", C.POINTER(C.c_float)),
                ("tensor_sums_out", C.POINTER(C.c_double))]


class SacClipping(C.Structure):
    """urgym_sac_clipping: the bound, the [2] scratch of the two coefficients and the two norm slots per update of urgym_sac_train_clipped."""
    _fields_ = [("max_grad_norm", C.c_float), ("reserved0", C.c_int32), ("scale", C.POINTER(C.c_float)), ("critic_grad_norm", C.POINTER(C.c_float)),
                ("actor_grad_norm", C.POINTER(C.c_float))]


# urgym_norm_state: the thirteen float64 DEVICE arrays in the struct's order, name -> shape(num_envs, obs_dim, goal_dim)
NORM_GROUPS = ("observation", "achieved_goal", "desired_goal", "ret")
NORM_STATE_FIELDS = [(f"{g}_{part}", (lambda N, od, gd, g=g, part=part: (1,) if part == "count" or g == "ret" else ((od,) if g == "observation" else (gd,))))
                     for g in NORM_GROUPS for part in ("mean", "var", "count")] + [("running_ret", lambda N, od, gd: (N,))]
NORM_SLAB_ROWS, NORM_CHAINS, NORM_PARTS = 128, 4, 16  # the order of the sums (ur_gym_amd/csrc/urgym_norm.h)
NORM_INITIAL_COUNT = 1e-4  # SB3's RunningMeanStd(epsilon=1e-4)


class NormState(C.Structure):
    """urgym_norm_state: mean, var and count of the four groups and the running discounted return of every env, all float64."""
    _fields_ = [(name, C.POINTER(C.c_double)) for name, _ in NORM_STATE_FIELDS]


class Normalization(C.Structure):
    """urgym_normalization: the state, the options, the actor's scratch rows and the fold's workspace."""
    _fields_ = [("state", NormState), ("gamma", C.c_double), ("eps", C.c_double), ("clip_obs", C.c_double), ("clip_reward", C.c_double),
                ("norm_obs", C.c_int32), ("norm_reward", C.c_int32), ("training", C.c_int32), ("scratch", C.POINTER(C.c_float)),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64), ("eval_scratch", C.POINTER(C.c_float)), ("best_state", C.POINTER(NormState)),
                ("reserved0", C.c_int64)]


class NormRowsArgs(C.Structure):
    """urgym_norm_rows_args: the three optional sources and their destinations."""
    _fields_ = [(name, C.POINTER(C.c_float)) for name in ("observation", "achieved_goal", "desired_goal", "observation_out", "achieved_goal_out",
                                                          "desired_goal_out")]


PER_FANOUT = 256  # URGYM_PER_FANOUT: the fan-out of the priority sums
PER_TERMS_MAX_COUNT = 65536  # URGYM_PER_TERMS_MAX_COUNT
PER_TAG = 0x50455200  # word 3 of the Philox counter of urgym_replay_sample_prioritized's draw


class PerPriorities(C.Structure):
    """urgym_per_priorities: the leaves [C][N] (priority ** alpha, 0 = never drawn), the float64 sum levels and the total, max_leaf[1]."""
    _fields_ = [("capacity_steps", C.c_int32), ("reserved0", C.c_int32), ("leaf", C.POINTER(C.c_float)), ("sums", C.POINTER(C.c_double)),
                ("max_leaf", C.POINTER(C.c_float))]


class PerTermsArgs(C.Structure):
    """urgym_per_terms_args: the drawn leaves and the total, q and y, the outputs w_raw, w, dq, and the write-back group (index,
    new_leaf, priorities) given whole or not at all."""
    _fields_ = [("count", C.c_int32), ("reserved0", C.c_int32), ("size", C.c_float), ("beta", C.c_float), ("alpha", C.c_float),
                ("eps", C.c_float), ("scale", C.c_float), ("reserved1", C.c_float), ("leaf_in", C.POINTER(C.c_float)),
                ("total", C.POINTER(C.c_double)), ("q", C.POINTER(C.c_float)), ("y", C.POINTER(C.c_float)), ("w_raw", C.POINTER(C.c_float)),
                ("w", C.POINTER(C.c_float)), ("dq", C.POINTER(C.c_float)), ("index", C.POINTER(C.c_int64)), ("new_leaf", C.POINTER(C.c_float)),
                ("priorities", PerPriorities)]


class SacPrioritized(C.Structure):
    """urgym_sac_prioritized: the structure, the beta schedule, the exponents and the [count] scratch of urgym_sac_train_prioritized."""
    _fields_ = [("priorities", PerPriorities), ("beta0", C.c_double), ("beta_steps", C.c_int64), ("alpha", C.c_float), ("eps", C.c_float),
                ("leaf", C.POINTER(C.c_float)), ("total", C.POINTER(C.c_double)), ("q", C.POINTER(C.c_float)), ("w_raw", C.POINTER(C.c_float)),
                ("w", C.POINTER(C.c_float)), ("dq", C.POINTER(C.c_float)), ("new_leaf", C.POINTER(C.c_float)), ("reserved0", C.c_int64)]


# urgym_sac_prioritized: name -> shape(count) of the float32 scratch (total is float64 [1])
SAC_PRIORITIZED_SCRATCH = [("leaf", lambda M: (M,)), ("q", lambda M: (2, M)), ("w_raw", lambda M: (M,)), ("w", lambda M: (M,)), ("dq", lambda M: (2, M)),
                           ("new_leaf", lambda M: (M,))]


MPPI_TAG = 0x4D505000  # URGYM_MPPI_TAG: word 3 of the Philox counter of the planner's noise is MPPI_TAG | block
MPPI_SAMPLES_MAX, MPPI_HORIZON_MAX, MPPI_ITERATIONS_MAX = 1024, 64, 8  # URGYM_MPPI_*_MAX

# urgym_mppi's device pointers: name -> (ctype of element, shape given (E, K, H)); w may be NULL
MPPI_FIELDS = [
    ("mean", C.c_float, lambda E, K, H: (H, E, 6)),
    ("new_mean", C.c_float, lambda E, K, H: (H, E, 6)),
    ("actions", C.c_float, lambda E, K, H: (H, E * K, 6)),
    ("eps", C.c_float, lambda E, K, H: (H, E * K, 6)),
    ("ret", C.c_double, lambda E, K, H: (E * K,)),
    ("g", C.c_double, lambda E, K, H: (E * K,)),
    ("alive", C.c_uint8, lambda E, K, H: (E * K,)),
    ("end_step", C.c_int32, lambda E, K, H: (E * K,)),
    ("success", C.c_uint8, lambda E, K, H: (E * K,)),
    ("collided", C.c_uint8, lambda E, K, H: (E * K,)),
    ("action_out", C.c_float, lambda E, K, H: (E, 6)),
    ("best_return", C.c_double, lambda E, K, H: (E,)),
    ("nominal_return", C.c_double, lambda E, K, H: (E,)),
    ("ess", C.c_double, lambda E, K, H: (E,)),
    ("w", C.c_double, lambda E, K, H: (E, K)),
]


class Mppi(C.Structure):
    """urgym_mppi: the scalars of a planner and its caller-owned device arrays."""
    _fields_ = [("num_parents", C.c_int32), ("samples", C.c_int32), ("horizon", C.c_int32), ("iterations", C.c_int32), ("shift", C.c_int32),
                ("reserved0", C.c_int32), ("sigma", C.c_float), ("reserved1", C.c_int32), ("lam", C.c_double), ("gamma", C.c_double),
                ("seed", C.c_uint64)] + [(name, C.POINTER(ct)) for name, ct, _ in MPPI_FIELDS]


# urgym_mppi_guide's device pointers: name -> (ctype of element, shape given (E, K)); each may be NULL where the options do not need it
MPPI_GUIDE_FIELDS = [
    ("policy_action", C.c_float, lambda E, K: (E * K, 6)),
    ("value", C.c_float, lambda E, K: (E * K,)),
    ("terminal", C.c_double, lambda E, K: (E * K,)),
]


class MppiGuide(C.Structure):
    """urgym_mppi_guide: the learner in the planner's loop -- an actor and a critic of the PLANNER handle, how they are used, and the
    caller-owned device arrays they write."""
    _fields_ = [("actor", C.c_void_p), ("critic", C.c_void_p), ("policy_samples", C.c_int32), ("terminal_value", C.c_int32),
                ("policy_sigma", C.c_float), ("reserved0", C.c_int32), ("fail_cost", C.c_double)] + [(name, C.POINTER(ct)) for name, ct, _ in MPPI_GUIDE_FIELDS]


MPPI_EXPLORE_BLOCK = 2  # URGYM_MPPI_EXPLORE_BLOCK: the exploration noise draws blocks 2 and 3 under MPPI_TAG (0 and 1 are the sample noise)


class MppiExplore(C.Structure):
    """urgym_mppi_explore: the exploration noise on the action a planner-driven collection executes; explore_eps ([E][6]) may be NULL."""
    _fields_ = [("explore_sigma", C.c_float), ("reserved0", C.c_int32), ("explore_eps", C.POINTER(C.c_float))]


# urgym_mppi_adapt's device pointers: name -> (ctype of element, shape given (E, K, H)); rank and elite may be NULL
MPPI_ADAPT_FIELDS = [
    ("std", C.c_float, lambda E, K, H: (H, E, 6)),
    ("new_std", C.c_float, lambda E, K, H: (H, E, 6)),
    ("rank", C.c_int32, lambda E, K, H: (E, K)),
    ("elite", C.c_uint8, lambda E, K, H: (E, K)),
    ("elite_count", C.c_int32, lambda E, K, H: (E,)),
    ("threshold", C.c_double, lambda E, K, H: (E,)),
]


class MppiAdapt(C.Structure):
    """urgym_mppi_adapt: elite selection and the per-(step, joint) std of a planner, and the caller-owned device arrays they write."""
    _fields_ = [("elites", C.c_int32), ("adapt_std", C.c_int32), ("std_min", C.c_float), ("std_max", C.c_float)] + [
        (name, C.POINTER(ct)) for name, ct, _ in MPPI_ADAPT_FIELDS]


class MppiStatsRecord(C.Structure):
    """urgym_mppi_stats_record: one record of plan statistics over the E parents of a planner (urgym_mppi_stats)."""
    _fields_ = [("mean_best_return", C.c_double), ("mean_nominal_return", C.c_double), ("mean_gain", C.c_double), ("mean_ess", C.c_double),
                ("min_ess", C.c_double), ("mean_elite_count", C.c_double), ("mean_threshold", C.c_double), ("iteration", C.c_int64),
                ("num_parents", C.c_int32), ("planned", C.c_int32), ("nominal_finite", C.c_int32), ("gain_count", C.c_int32),
                ("threshold_count", C.c_int32), ("reserved0", C.c_int32)]


MPPI_STATS_RECORD_WORDS = 11  # sizeof(urgym_mppi_stats_record) / 8: a record as a row of an int64 tensor
MPPI_STATS_MAX_PARENTS = 65536  # SAC_TERMS_MAX_COUNT: one workgroup reduces them


class SacPlanning(C.Structure):
    """urgym_sac_planning: the planner that collects inside urgym_sac_train_planned, whether its actor and critic follow the learner, and
    the plan-statistics records."""
    _fields_ = [("planner_handle", C.c_void_p), ("mppi", C.POINTER(Mppi)), ("adapt_or_NULL", C.POINTER(MppiAdapt)), ("guide_or_NULL", C.POINTER(MppiGuide)),
                ("explore", MppiExplore), ("sync", C.c_int32), ("record_capacity", C.c_int32), ("records", C.POINTER(MppiStatsRecord)),
                ("reserved0", C.c_int64)]


MPPI_TEMPER_SOLVED, MPPI_TEMPER_AT_MAX, MPPI_TEMPER_AT_MIN, MPPI_TEMPER_NO_RETURN = 0, 1, 2, 3  # URGYM_MPPI_TEMPER_*: what `saturated` holds
MPPI_TEMPER_STEPS_MAX = 64  # URGYM_MPPI_TEMPER_STEPS_MAX
MPPI_TEMPER_LAM_RANGE = (1e-100, 1e100)  # the bounds lam_min and lam_max must lie in

# urgym_mppi_temper's device pointers: name -> (ctype of element, shape given (E, K, H)); saturated may be NULL
MPPI_TEMPER_FIELDS = [
    ("lam_out", C.c_double, lambda E, K, H: (E,)),
    ("saturated", C.c_uint8, lambda E, K, H: (E,)),
]


class MppiTemper(C.Structure):
    """urgym_mppi_temper: the target effective sample size of the tempered update, the bracket and the steps of its search, and the
    caller-owned device arrays it writes."""
    _fields_ = [("ess_target", C.c_double), ("lam_min", C.c_double), ("lam_max", C.c_double), ("steps", C.c_int32), ("reserved0", C.c_int32)] + [
        (name, C.POINTER(ct)) for name, ct, _ in MPPI_TEMPER_FIELDS]


class MppiNoise(C.Structure):
    """urgym_mppi_noise: the lag-1 correlation of the planner's sampling noise along the horizon.  It owns no array."""
    _fields_ = [("beta", C.c_float), ("reserved0", C.c_int32)]


class SacCloneArgs(C.Structure):
    """urgym_sac_clone_args: what urgym_sac_policy_terms_cloned takes beside urgym_sac_policy_args -- the two actions, the weight and its
    two flags, the three [1] outputs.  All pointers required."""
    _fields_ = [("action_pi", C.POINTER(C.c_float)), ("action_data", C.POINTER(C.c_float)), ("weight", C.c_float), ("bc_scale", C.c_float),
                ("scale_by_q", C.c_int32), ("q_filter", C.c_int32), ("bc_loss_out", C.POINTER(C.c_float)), ("bc_weight_out", C.POINTER(C.c_float)),
                ("bc_rows_out", C.POINTER(C.c_int32)), ("reserved0", C.c_int32)]


class SacCloning(C.Structure):
    """urgym_sac_cloning: the option of urgym_sac_train_cloned -- the weight, its two flags and one slot per update of the call each for
    the cloning loss, the weight used and the number of cloned rows."""
    _fields_ = [("weight", C.c_float), ("scale_by_q", C.c_int32), ("q_filter", C.c_int32), ("reserved0", C.c_int32),
                ("bc_loss", C.POINTER(C.c_float)), ("bc_weight", C.POINTER(C.c_float)), ("bc_rows", C.POINTER(C.c_int32))]


class ReplayDemonstrations(C.Structure):
    """urgym_replay_demonstrations: the demonstration ring of urgym_replay_sample_mixed -- a ring of the same env kind with its own env
    count, cursor and fill level, and D, the number of leading rows of a minibatch that come from it."""
    _fields_ = [("ring", ReplayRing), ("num_envs", C.c_int32), ("oldest_slot", C.c_int32), ("filled_steps", C.c_int32), ("count", C.c_int32)]


class SacDemonstrating(C.Structure):
    """urgym_sac_demonstrating: the option of urgym_sac_train_demonstrated -- the demonstrations, the [M] scratch the gather's source goes
    to, and whether cloning applies to demonstration rows only."""
    _fields_ = [("demonstrations", ReplayDemonstrations), ("source", C.POINTER(C.c_uint8)), ("clone_demonstrations_only", C.c_int32),
                ("reserved0", C.c_int32)]


class SacAdvantageArgs(C.Structure):
    """urgym_sac_advantage_args: what urgym_sac_policy_terms_weighted takes beside the clone args -- the temperature and the cap of the
    advantage weight, the optional row mask and the three outputs."""
    _fields_ = [("temperature", C.c_float), ("max_weight", C.c_float), ("row_mask", C.POINTER(C.c_uint8)), ("adv_ess_out", C.POINTER(C.c_float)),
                ("adv_max_out", C.POINTER(C.c_float)), ("adv_clipped_out", C.POINTER(C.c_int32)), ("reserved0", C.c_int32)]


class SacWeighting(C.Structure):
    """urgym_sac_weighting: the option of urgym_sac_train_weighted -- the temperature, the cap and the per-update records."""
    _fields_ = [("temperature", C.c_float), ("max_weight", C.c_float), ("reserved0", C.c_int32), ("adv_ess", C.POINTER(C.c_float)),
                ("adv_max", C.POINTER(C.c_float)), ("adv_clipped", C.POINTER(C.c_int32))]


IK_TAG = 0x494B5200  # URGYM_IK_TAG: word 3 of the Philox counter of the reach controller's exploration noise is IK_TAG | block (0, 1)
IK_DAMPING_RANGE, IK_GAIN_MAX = (1e-2, 10.0), 10.0  # what urgym_controller_* accept: damping in [1e-2, 10], gain in (0, 10]


class ReachController(C.Structure):
    """urgym_reach_controller: the scalars of the scripted reach controller (damped least-squares IK) and where its exploration noise
    goes; explore_eps ([N][6]) may be NULL."""
    _fields_ = [("damping", C.c_double), ("gain", C.c_double), ("seed", C.c_uint64), ("explore_sigma", C.c_float), ("reserved0", C.c_int32),
                ("explore_eps", C.POINTER(C.c_float))]


# Every symbol include/urgym.h declares (tests check that the built library exports each of them).
EXPORTED_SYMBOLS = [
    "urgym_abi_version",
    "urgym_config_default",
    "urgym_obs_dims",
    "urgym_create",
    "urgym_destroy",
    "urgym_bind",
    "urgym_reset",
    "urgym_step",
    "urgym_rollout",
    "urgym_actor_create",
    "urgym_actor_destroy",
    "urgym_actor_forward",
    "urgym_rollout_actor",
    "urgym_actor_set_log_std",
    "urgym_actor_sample",
    "urgym_rollout_sampled",
    "urgym_critic_create",
    "urgym_critic_destroy",
    "urgym_critic_evaluate",
    "urgym_critic_action_gradient",
    "urgym_critic_parameter_gradients_workspace",
    "urgym_critic_parameter_gradients",
    "urgym_actor_parameter_gradients_workspace",
    "urgym_actor_parameter_gradients",
    "urgym_actor_sample_rows",
    "urgym_rollout_collect",
    "urgym_replay_sample",
    "urgym_actor_load",
    "urgym_critic_load",
    "urgym_actor_unpack",
    "urgym_critic_unpack",
    "urgym_adam_coefficients",
    "urgym_actor_adam_step",
    "urgym_critic_adam_step",
    "urgym_sac_entropy_step",
    "urgym_sac_policy_terms",
    "urgym_sac_train",
    "urgym_eval_stats",
    "urgym_actor_snapshot",
    "urgym_policy_evaluate",
    "urgym_sac_train_evaluated",
    "urgym_monitor_fold",
    "urgym_monitor_stats",
    "urgym_sac_train_monitored",
    "urgym_replay_sample_nstep",
    "urgym_sac_entropy_step_nstep",
    "urgym_sac_train_nstep",
    "urgym_per_sums_count",
    "urgym_per_rebuild",
    "urgym_per_fill",
    "urgym_replay_sample_prioritized",
    "urgym_per_terms",
    "urgym_sac_train_prioritized",
    "urgym_replay_sample_hindsight",
    "urgym_sac_train_hindsight",
    "urgym_actor_grad_norm",
    "urgym_critic_grad_norm",
    "urgym_actor_adam_step_scaled",
    "urgym_critic_adam_step_scaled",
    "urgym_sac_train_clipped",
    "urgym_actor_read_packed",
    "urgym_critic_read_packed",
    "urgym_norm_workspace",
    "urgym_norm_fold",
    "urgym_norm_rows",
    "urgym_norm_batch",
    "urgym_norm_snapshot",
    "urgym_rollout_collect_normalized",
    "urgym_policy_evaluate_normalized",
    "urgym_sac_train_normalized",
    "urgym_mppi_fanout",
    "urgym_mppi_sample",
    "urgym_mppi_score",
    "urgym_mppi_update",
    "urgym_mppi_record",
    "urgym_mppi_plan",
    "urgym_mppi_control",
    "urgym_mppi_guide_actions",
    "urgym_mppi_terminal",
    "urgym_mppi_plan_guided",
    "urgym_mppi_control_guided",
    "urgym_mppi_execute",
    "urgym_mppi_collect",
    "urgym_mppi_sample_adaptive",
    "urgym_mppi_update_elite",
    "urgym_mppi_plan_adaptive",
    "urgym_mppi_control_adaptive",
    "urgym_mppi_collect_adaptive",
    "urgym_mppi_stats",
    "urgym_sac_train_planned",
    "urgym_mppi_update_tempered",
    "urgym_mppi_plan_tempered",
    "urgym_mppi_control_tempered",
    "urgym_mppi_collect_tempered",
    "urgym_sac_train_tempered",
    "urgym_mppi_sample_colored",
    "urgym_mppi_plan_colored",
    "urgym_mppi_control_colored",
    "urgym_mppi_collect_colored",
    "urgym_sac_train_colored",
    "urgym_sac_policy_terms_cloned",
    "urgym_sac_train_cloned",
    "urgym_replay_sample_mixed",
    "urgym_sac_policy_terms_cloned_masked",
    "urgym_sac_train_demonstrated",
    "urgym_sac_policy_terms_weighted",
    "urgym_sac_train_weighted",
    "urgym_controller_actions",
    "urgym_controller_control",
    "urgym_controller_collect",
    "urgym_refresh",
    "urgym_invalidate_records",
    "urgym_derive_obstacle_motion",
    "urgym_probe_closest",
    "urgym_probe_pose_distance",
    "urgym_enable_timing",
    "urgym_query_timing", "urgym_query_refill_timing",
    "urgym_last_error",
]
