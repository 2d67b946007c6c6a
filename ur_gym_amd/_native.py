"""Loader of the HIP extension (liburgym_hip.so) through ctypes.

There is deliberately NO fallback: if the shared library is missing, cannot be loaded, or does not export the
ABI of include/urgym.h, importing the native layer raises.  The CPU oracle under oracle/ is test infrastructure
and is never reachable from here.
"""
import ctypes as C
import os
import subprocess

from . import _abi

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# URGYM_LIB: another build of the same extension (tuning experiments: tools/exp_*.sh); there is still no fallback of any kind
LIB_PATH = os.environ.get("URGYM_LIB") or os.path.join(_CSRC, "liburgym_hip.so")
_lib = None


class NativeError(RuntimeError):
    pass


def build(force=False):
    """Compile the extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-s"] + (["-B"] if force else [])
    subprocess.check_call(args)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).  Import torch
    # FIRST so that this extension binds to the very runtime instance whose streams and device pointers it is handed;
    # loading the extension first would pull in a second, system-wide runtime.
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ur_gym_amd/csrc`). There is no CPU fallback.")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime, wrong arch, ...
        raise NativeError(f"cannot load {LIB_PATH}: {e}. There is no CPU fallback.") from e
    missing = [s for s in _abi.EXPORTED_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise NativeError(f"{LIB_PATH} does not export {missing}")
    L.urgym_abi_version.restype = C.c_int
    if L.urgym_abi_version() != _abi.ABI_VERSION:
        raise NativeError(f"ABI mismatch: library {L.urgym_abi_version()} vs binding {_abi.ABI_VERSION}")
    L.urgym_config_default.argtypes = [C.c_int, C.c_int, C.POINTER(_abi.Config)]
    L.urgym_obs_dims.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.urgym_create.argtypes = [C.POINTER(_abi.Config), C.c_int, C.POINTER(C.c_void_p)]
    L.urgym_destroy.argtypes = [C.c_void_p]
    L.urgym_bind.argtypes = [C.c_void_p, C.POINTER(_abi.Buffers)]
    L.urgym_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.urgym_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.urgym_actor_create.argtypes = [C.c_void_p, C.POINTER(_abi.ActorDesc), C.POINTER(C.c_void_p)]
    L.urgym_actor_destroy.argtypes = [C.c_void_p, C.c_void_p]
    L.urgym_actor_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_rollout_actor.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_actor_set_log_std.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.urgym_actor_sample.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Sampling), C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_rollout_sampled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Sampling), C.c_int, C.POINTER(_abi.Trajectory),
                                        C.POINTER(_abi.SampleRecords), C.c_void_p]
    L.urgym_critic_create.argtypes = [C.c_void_p, C.POINTER(_abi.CriticDesc), C.POINTER(C.c_void_p)]
    L.urgym_critic_destroy.argtypes = [C.c_void_p, C.c_void_p]
    L.urgym_critic_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticRows), C.c_int, C.POINTER(_abi.CriticTerms),
                                        C.POINTER(_abi.CriticOut), C.c_void_p]
    L.urgym_critic_action_gradient.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticRows), C.c_int, C.POINTER(_abi.CriticGradOut), C.c_void_p]
    L.urgym_critic_parameter_gradients_workspace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.urgym_critic_parameter_gradients.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticRows), C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                                   C.POINTER(_abi.CriticParamGrads), C.c_void_p, C.c_uint64, C.c_void_p]
    L.urgym_actor_parameter_gradients_workspace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.urgym_actor_parameter_gradients.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Sampling), C.POINTER(_abi.CriticRows), C.c_int,
                                                  C.POINTER(_abi.ActorUpstream), C.POINTER(_abi.ActorParamGrads), C.c_void_p, C.c_uint64, C.c_void_p]
    L.urgym_actor_sample_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Sampling), C.POINTER(_abi.CriticRows), C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    L.urgym_rollout_collect.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Sampling), C.c_int, C.POINTER(_abi.ReplayRing), C.c_int, C.c_void_p]
    L.urgym_replay_sample.argtypes = [C.c_void_p, C.POINTER(_abi.ReplayRing), C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                      C.POINTER(_abi.ReplayBatch), C.c_void_p]
    L.urgym_actor_load.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.ActorParamsDev), C.c_void_p]
    L.urgym_critic_load.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticParamsDev), C.c_float, C.c_void_p]
    L.urgym_actor_unpack.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.ActorParamsOut), C.c_void_p]
    L.urgym_critic_unpack.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticParamsOut), C.c_void_p]
    L.urgym_adam_coefficients.argtypes =[C.POINTER(_abi.AdamHyper), C.POINTER(C.c_float)]
    L.urgym_actor_adam_step.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.ActorAdam), C.POINTER(_abi.AdamHyper), C.c_void_p]
    L.urgym_critic_adam_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticAdam), C.POINTER(_abi.AdamHyper), C.c_float, C.c_void_p]
    L.urgym_sac_entropy_step.argtypes = [C.c_void_p, C.POINTER(_abi.SacEntropyArgs), C.POINTER(_abi.AdamHyper), C.c_void_p]
    L.urgym_sac_policy_terms.argtypes = [C.c_void_p, C.POINTER(_abi.SacPolicyArgs), C.c_void_p]
    L.urgym_sac_train.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.c_void_p]
    L.urgym_eval_stats.argtypes = [C.c_void_p, C.POINTER(_abi.EvalStatsArgs), C.c_void_p]
    L.urgym_actor_snapshot.argtypes = [C.c_void_p, C.POINTER(_abi.ActorSnapshotArgs), C.c_void_p]
    L.urgym_policy_evaluate.argtypes = [C.c_void_p, C.POINTER(_abi.PolicyEvaluation), C.c_int64, C.c_int32, C.c_void_p]
    L.urgym_sac_train_evaluated.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacEvaluation), C.c_void_p]
    L.urgym_monitor_fold.argtypes = [C.c_void_p, C.POINTER(_abi.MonitorState), C.POINTER(_abi.ReplayRing), C.c_int, C.c_int, C.c_void_p]
    L.urgym_monitor_stats.argtypes = [C.c_void_p, C.POINTER(_abi.MonitorState), C.POINTER(_abi.MonitorRecord), C.c_int64, C.c_int, C.c_void_p]
    L.urgym_sac_train_monitored.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacEvaluation),
                                            C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_replay_sample_nstep.argtypes = [C.c_void_p, C.POINTER(_abi.ReplayRing), C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                            C.POINTER(_abi.ReplayBatch), C.POINTER(_abi.ReplayNstep), C.c_void_p]
    L.urgym_sac_entropy_step_nstep.argtypes = [C.c_void_p, C.POINTER(_abi.SacEntropyNstepArgs), C.POINTER(_abi.AdamHyper), C.c_void_p]
    L.urgym_sac_train_nstep.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacNstep),
                                        C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_per_sums_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.urgym_per_rebuild.argtypes = [C.c_void_p, C.POINTER(_abi.PerPriorities), C.c_void_p]
    L.urgym_per_fill.argtypes = [C.c_void_p, C.POINTER(_abi.PerPriorities), C.c_int, C.c_int, C.c_void_p]
    L.urgym_replay_sample_prioritized.argtypes = [C.c_void_p, C.POINTER(_abi.ReplayRing), C.POINTER(_abi.PerPriorities), C.c_uint64, C.c_uint64,
                                                  C.c_int, C.POINTER(_abi.ReplayBatch), C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_per_terms.argtypes = [C.c_void_p, C.POINTER(_abi.PerTermsArgs), C.c_void_p]
    L.urgym_sac_train_prioritized.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacPrioritized),
                                              C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_replay_sample_hindsight.argtypes = [C.c_void_p, C.POINTER(_abi.ReplayRing), C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                                C.POINTER(_abi.ReplayBatch), C.POINTER(_abi.ReplayHindsight), C.c_void_p]
    L.urgym_sac_train_hindsight.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacHindsight),
                                            C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_actor_grad_norm.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.ActorTensors), C.POINTER(_abi.GradNorm), C.c_void_p]
    L.urgym_critic_grad_norm.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.QNetworkDev), C.POINTER(_abi.GradNorm), C.c_void_p]
    L.urgym_actor_adam_step_scaled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.ActorAdam), C.POINTER(_abi.AdamHyper), C.c_void_p, C.c_void_p]
    L.urgym_critic_adam_step_scaled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_abi.CriticAdam), C.POINTER(_abi.AdamHyper), C.c_float,
                                                C.c_void_p, C.c_void_p]
    L.urgym_sac_train_clipped.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacClipping),
                                          C.POINTER(_abi.SacNstep), C.POINTER(_abi.SacPrioritized), C.POINTER(_abi.SacHindsight),
                                          C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_norm_workspace.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.urgym_norm_fold.argtypes = [C.c_void_p, C.POINTER(_abi.Normalization), C.POINTER(_abi.ReplayRing), C.c_int, C.c_int, C.c_void_p]
    L.urgym_norm_rows.argtypes = [C.c_void_p, C.POINTER(_abi.Normalization), C.POINTER(_abi.NormRowsArgs), C.c_int, C.c_void_p]
    L.urgym_norm_batch.argtypes = [C.c_void_p, C.POINTER(_abi.Normalization), C.POINTER(_abi.ReplayBatch), C.c_int, C.c_void_p]
    L.urgym_norm_snapshot.argtypes = [C.c_void_p, C.POINTER(_abi.NormState), C.POINTER(_abi.NormState), C.c_void_p, C.c_void_p]
    L.urgym_policy_evaluate_normalized.argtypes = [C.c_void_p, C.POINTER(_abi.PolicyEvaluation), C.POINTER(_abi.Normalization), C.c_int64, C.c_int32, C.c_void_p]
    L.urgym_rollout_collect_normalized.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Sampling), C.c_int, C.POINTER(_abi.ReplayRing), C.c_int,
                                                   C.POINTER(_abi.Normalization), C.c_void_p]
    L.urgym_sac_train_normalized.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.Normalization),
                                             C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacNstep), C.POINTER(_abi.SacPrioritized),
                                             C.POINTER(_abi.SacHindsight), C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_mppi_fanout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.c_void_p]
    L.urgym_mppi_sample.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.c_uint64, C.c_int, C.c_void_p]
    L.urgym_mppi_score.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.c_int, C.c_void_p]
    L.urgym_mppi_update.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.c_void_p]
    L.urgym_mppi_record.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.c_int, C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_mppi_plan.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.c_uint64, C.c_void_p]
    L.urgym_mppi_control.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.c_uint64, C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_mppi_guide_actions.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiGuide), C.c_int, C.c_void_p]
    L.urgym_mppi_terminal.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiGuide), C.c_void_p]
    L.urgym_mppi_plan_guided.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiGuide), C.c_uint64, C.c_void_p]
    L.urgym_mppi_control_guided.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiGuide), C.c_uint64, C.c_int,
                                            C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_mppi_execute.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiExplore), C.c_uint64, C.c_void_p, C.c_void_p]
    L.urgym_mppi_collect.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiGuide), C.POINTER(_abi.MppiExplore), C.c_uint64,
                                     C.c_int, C.POINTER(_abi.ReplayRing), C.c_int, C.c_void_p]
    L.urgym_mppi_sample_adaptive.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiAdapt), C.c_uint64, C.c_int, C.c_void_p]
    L.urgym_mppi_update_elite.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiAdapt), C.c_void_p]
    L.urgym_mppi_plan_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiGuide), C.c_uint64,
                                           C.c_void_p]
    L.urgym_mppi_control_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiGuide), C.c_uint64,
                                              C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_mppi_collect_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiGuide),
                                              C.POINTER(_abi.MppiExplore), C.c_uint64, C.c_int, C.POINTER(_abi.ReplayRing), C.c_int, C.c_void_p]
    L.urgym_mppi_stats.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiStatsRecord), C.c_int64, C.c_void_p]
    L.urgym_sac_train_planned.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacPlanning),
                                          C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacNstep), C.POINTER(_abi.SacPrioritized),
                                          C.POINTER(_abi.SacHindsight), C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_mppi_update_tempered.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.MppiAdapt), C.c_void_p]
    L.urgym_mppi_plan_tempered.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.MppiAdapt),
                                           C.POINTER(_abi.MppiGuide), C.c_uint64, C.c_void_p]
    L.urgym_mppi_control_tempered.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.MppiAdapt),
                                              C.POINTER(_abi.MppiGuide), C.c_uint64, C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_mppi_collect_tempered.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.MppiAdapt),
                                              C.POINTER(_abi.MppiGuide), C.POINTER(_abi.MppiExplore), C.c_uint64, C.c_int, C.POINTER(_abi.ReplayRing), C.c_int,
                                              C.c_void_p]
    L.urgym_sac_train_tempered.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacPlanning),
                                           C.POINTER(_abi.MppiTemper), C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacNstep), C.POINTER(_abi.SacPrioritized),
                                           C.POINTER(_abi.SacHindsight), C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_mppi_sample_colored.argtypes = [C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiNoise), C.POINTER(_abi.MppiAdapt), C.c_uint64, C.c_int, C.c_void_p]
    L.urgym_mppi_plan_colored.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiNoise), C.POINTER(_abi.MppiTemper),
                                          C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiGuide), C.c_uint64, C.c_void_p]
    L.urgym_mppi_control_colored.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiNoise), C.POINTER(_abi.MppiTemper),
                                             C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiGuide), C.c_uint64, C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_mppi_collect_colored.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Mppi), C.POINTER(_abi.MppiNoise), C.POINTER(_abi.MppiTemper),
                                             C.POINTER(_abi.MppiAdapt), C.POINTER(_abi.MppiGuide), C.POINTER(_abi.MppiExplore), C.c_uint64, C.c_int,
                                             C.POINTER(_abi.ReplayRing), C.c_int, C.c_void_p]
    L.urgym_sac_train_colored.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacPlanning),
                                          C.POINTER(_abi.MppiNoise), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacNstep),
                                          C.POINTER(_abi.SacPrioritized), C.POINTER(_abi.SacHindsight), C.POINTER(_abi.SacEvaluation),
                                          C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_sac_policy_terms_cloned.argtypes = [C.c_void_p, C.POINTER(_abi.SacPolicyArgs), C.POINTER(_abi.SacCloneArgs), C.c_void_p]
    L.urgym_sac_train_cloned.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacCloning),
                                         C.POINTER(_abi.SacPlanning), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.MppiNoise), C.POINTER(_abi.Normalization),
                                         C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacNstep), C.POINTER(_abi.SacPrioritized), C.POINTER(_abi.SacHindsight),
                                         C.POINTER(_abi.SacEvaluation), C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_replay_sample_mixed.argtypes = [C.c_void_p, C.POINTER(_abi.ReplayRing), C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                            C.POINTER(_abi.ReplayBatch), C.POINTER(_abi.ReplayDemonstrations), C.c_void_p, C.c_void_p]
    L.urgym_sac_policy_terms_cloned_masked.argtypes = [C.c_void_p, C.POINTER(_abi.SacPolicyArgs), C.POINTER(_abi.SacCloneArgs), C.c_void_p, C.c_void_p]
    L.urgym_sac_train_demonstrated.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacDemonstrating),
                                               C.POINTER(_abi.SacCloning), C.POINTER(_abi.SacPlanning), C.POINTER(_abi.MppiTemper), C.POINTER(_abi.MppiNoise),
                                               C.POINTER(_abi.Normalization), C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacEvaluation),
                                               C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_sac_policy_terms_weighted.argtypes = [C.c_void_p, C.POINTER(_abi.SacPolicyArgs), C.POINTER(_abi.SacCloneArgs), C.POINTER(_abi.SacAdvantageArgs), C.c_void_p]
    L.urgym_sac_train_weighted.argtypes = [C.c_void_p, C.POINTER(_abi.SacLearner), C.POINTER(_abi.SacSchedule), C.POINTER(_abi.SacWeighting),
                                           C.POINTER(_abi.SacCloning), C.POINTER(_abi.SacDemonstrating), C.POINTER(_abi.SacPlanning), C.POINTER(_abi.MppiTemper),
                                           C.POINTER(_abi.MppiNoise), C.POINTER(_abi.Normalization), C.POINTER(_abi.SacClipping), C.POINTER(_abi.SacNstep),
                                           C.POINTER(_abi.SacPrioritized), C.POINTER(_abi.SacHindsight), C.POINTER(_abi.SacEvaluation),
                                           C.POINTER(_abi.SacMonitoring), C.c_void_p]
    L.urgym_controller_actions.argtypes = [C.c_void_p, C.POINTER(_abi.ReachController), C.c_uint64, C.c_void_p, C.c_void_p]
    L.urgym_controller_control.argtypes = [C.c_void_p, C.POINTER(_abi.ReachController), C.c_uint64, C.c_int, C.POINTER(_abi.Trajectory), C.c_void_p]
    L.urgym_controller_collect.argtypes = [C.c_void_p, C.POINTER(_abi.ReachController), C.c_uint64, C.c_int, C.POINTER(_abi.ReplayRing), C.c_int, C.c_void_p]
    L.urgym_actor_read_packed.argtypes =[C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.urgym_critic_read_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.urgym_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_invalidate_records.argtypes = [C.c_void_p]
    L.urgym_derive_obstacle_motion.argtypes = [C.c_void_p, C.c_void_p]
    L.urgym_probe_closest.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_probe_pose_distance.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.urgym_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.urgym_query_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.urgym_query_refill_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.urgym_last_error.argtypes = [C.c_void_p]
    L.urgym_last_error.restype = C.c_char_p
    _lib = L
    return L


def check(rc, handle=None):
    if rc != 0:
        msg = lib().urgym_last_error(handle)
        raise NativeError(f"urgym call failed ({rc}): {msg.decode() if msg else '?'}")
