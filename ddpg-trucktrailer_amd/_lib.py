"""ctypes binding of libttenv.so (include/ttenv.h).  The product has no CPU fallback: if the
library is missing or a call fails, this raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TT_LIB_PATH") or os.path.join(HERE, "libttenv.so")  # override: kernel-variant A/B runs

OBS_DIM = 23
MAX_EPISODE_STEPS = 4095      # TT_MAX_EPISODE_STEPS
TT_OK, TT_EINVAL, TT_ENOMEM, TT_EHIP, TT_ENODEV = 0, -1, -2, -3, -4
F_JACKKNIFE, F_OUT_OF_MAP, F_MAX_STEPS, F_GOAL_REACHED, F_GOAL_PASSED, F_EXCESSIVE_BACK, F_SUCCESS = (1 << i for i in range(7))
VIOLATIONS = ("none", "jackknife", "jackknife_warning", "major_boundary", "minor_boundary", "past_the_goal",
              "max_step", "excessive_backward")
INFO_ROWS = ("total_reward", "progress_reward", "heading_reward", "orientation_reward", "staged_success",
             "safety_penalty", "exploration_bonus", "final_success_bonus", "backward_penalty", "smoothness_penalty",
             "cumulative_backward", "movement_budget")
NINFO = len(INFO_ROWS)
# counters of the episode log (TT_LOG_NCOUNTS, include/ttenv.h: tt_env_set_episode_log), in their order
LOG_COUNTS = ("episodes", "successes", "jackknife", "out_of_map", "max_steps", "goal_reached", "goal_passed",
              "excessive_back", "success_flag")
# the detailed episode log (TT_LOG_DETAIL, include/ttenv.h: tt_env_set_episode_log2): one sum per reward term, INFO_ROWS[1:10]
LOG_DETAIL = 1
LOG_COMPONENTS = INFO_ROWS[1:10]


class TTParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("L1", "L2", "hitch_offset", "v1x", "dt", "map_min_x", "map_max_x", "map_min_y",
                                          "map_max_y", "max_steer", "position_threshold", "orientation_threshold",
                                          "step_length")] + \
               [("extra_steps", C.c_int32), ("fixed_max_steps", C.c_int32), ("term_mask", C.c_uint32),
                ("variant", C.c_int32), ("stateless_reward", C.c_int32), ("reserved_", C.c_int32),
                ("goal", C.c_double * 3), ("reset_lo", C.c_double * 3),
                ("reset_hi", C.c_double * 3)]


class TTInfo(C.Structure):
    _fields_ = [("comp", C.c_void_p), ("violation", C.c_void_p), ("flags", C.c_void_p)]


class TTMlpWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3", "wa", "ba")] + \
               [("in_dim", C.c_int32), ("fc1_dims", C.c_int32), ("fc2_dims", C.c_int32), ("capped_grids", C.c_int32),
                ("split_ws", C.c_void_p), ("ws_packed", C.c_int32), ("max_workgroups", C.c_int32), ("split_ws_alt", C.c_void_p), ("fc2_img", C.c_void_p)]


class TTFc2Images(C.Structure):
    _fields_ = [("net", C.c_void_p), ("target", C.c_void_p)]


class TTMlpSaved(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("xh1", "h1", "xh2", "h2", "rstd1", "rstd2")]


class TTFwdJob(C.Structure):
    _fields_ = [("critic", C.c_int32), ("reserved_", C.c_int32), ("obs", C.c_void_p), ("action", C.c_void_p),
                ("w", C.POINTER(TTMlpWeights)), ("out", C.c_void_p), ("saved", C.POINTER(TTMlpSaved)),
                ("dq_da", C.c_void_p), ("z_state", C.c_void_p)]


class TTTdInput(C.Structure):
    _fields_ = [("z_state", C.c_void_p), ("mu_target", C.c_void_p), ("target_critic", C.POINTER(TTMlpWeights)),
                ("reward", C.c_void_p), ("done", C.c_void_p), ("gamma", C.c_float), ("reserved_", C.c_float),
                ("y_out", C.c_void_p), ("q_out", C.c_void_p), ("step_dev", C.c_void_p), ("window_dev", C.c_void_p),
                ("bias_corr_out", C.c_void_p), ("adam_beta1", C.c_float), ("adam_beta2", C.c_float)]


class TTSideBuffer(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("act", C.c_void_p), ("rew", C.c_void_p), ("obs2", C.c_void_p), ("done", C.c_void_p),
                ("count", C.c_int32), ("reserved_", C.c_int32)]


class TTRingView(C.Structure):
    _fields_ = [("cursor", C.c_void_p), ("obs", C.c_void_p), ("act", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p),
                ("n_envs", C.c_int32), ("slots", C.c_int32)]


class TTRingCursor(C.Structure):
    _fields_ = [("k_dev", C.c_void_p), ("slots", C.c_int32), ("reserved_", C.c_int32), ("cursor", C.c_void_p)]


class TTSampleArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("n_envs", C.c_int32), ("slots", C.c_int32), ("reserve", C.c_int32), ("k_dev", C.c_void_p),
                ("obs", C.c_void_p), ("act", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p), ("seed", C.c_uint64),
                ("side", C.POINTER(TTSideBuffer)), ("s_out", C.c_void_p), ("a_out", C.c_void_p), ("r_out", C.c_void_p),
                ("s2_out", C.c_void_p), ("d_out", C.c_void_p), ("idx_out", C.c_void_p), ("lag", C.c_int32),
                ("draws", C.c_int32), ("seed_stride", C.c_uint64), ("step_progress", C.c_void_p)]


class TTImageJob(C.Structure):
    _fields_ = [("actor", C.POINTER(TTMlpWeights)), ("cursor", C.POINTER(TTRingCursor))]


class TTMlpBwdWs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dpre", "dz", "dx2", "dy1", "dx1")]


class TTPopNet(C.Structure):
    _fields_ = [("ws", C.POINTER(TTMlpBwdWs)), ("grads", C.POINTER(TTMlpWeights)), ("count", C.c_int32), ("reserved_", C.c_int32),
                ("params", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("targets", C.c_void_p)] + \
               [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "tau")] + [("images", C.POINTER(TTFc2Images))]


class TTPopAgent(C.Structure):
    _fields_ = [("sample", C.POINTER(TTSampleArgs)), ("jobs", C.POINTER(TTFwdJob)), ("td", C.POINTER(TTTdInput)),
                ("critic", TTPopNet), ("actor", TTPopNet), ("q_pi", C.c_void_p), ("dq_da", C.c_void_p), ("tail_words", C.c_void_p),
                ("gave_up_host", C.c_void_p)]


class TTPopExploitPair(C.Structure):
    _fields_ = [("dst", C.c_int32), ("src", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float), ("tau", C.c_float),
                ("gamma", C.c_float)]


class TTPopNstep(C.Structure):
    _fields_ = [("n_step", C.c_int32), ("gamma", C.c_float), ("discount", C.c_float)]


class TTPopClip(C.Structure):
    """struct tt_pop_clip (include/ttenv.h): max_norm of an agent's critic and actor, each a finite number > 0 or 0 = not clipped."""
    _fields_ = [("max_norm_critic", C.c_float), ("max_norm_actor", C.c_float)]


class TTTd3Agent(C.Structure):
    _fields_ = [("sample", C.POINTER(TTSampleArgs)), ("jobs", C.POINTER(TTFwdJob)), ("td", C.POINTER(TTTdInput)),
                ("critic", TTPopNet), ("critic_2", TTPopNet), ("actor", TTPopNet), ("z_state_2", C.c_void_p),
                ("target_critic_2", C.POINTER(TTMlpWeights)), ("target_noise", C.c_float), ("noise_clip", C.c_float),
                ("noise_seed", C.c_uint64), ("eps_out", C.c_void_p), ("y2_out", C.c_void_p), ("q2t_out", C.c_void_p),
                ("step_snapshot", C.c_void_p), ("actor_step_dev", C.c_void_p), ("actor_bias_corr_out", C.c_void_p),
                ("q_pi", C.c_void_p), ("dq_da", C.c_void_p), ("tail_words", C.c_void_p), ("gave_up_host", C.c_void_p)]


class TTPopTd3Pair(C.Structure):
    _fields_ = [("dst", C.c_int32), ("src", C.c_int32)] + \
               [(n, C.c_float) for n in ("alpha", "beta", "tau", "gamma", "target_noise", "noise_clip")]


class TTLossShape(C.Structure):
    """tt_loss_shape (include/ttenv.h): huber_delta (0 = MSE with the caller's scale), pre_scale = 2c/B, pre [n]."""
    _fields_ = [("huber_delta", C.c_float), ("pre_scale", C.c_float), ("pre", C.c_void_p)]


class TTDemoLoss(C.Structure):
    """tt_demo_loss (include/ttenv.h): a [n], idx [n][2], q [n] (with q_filter), k = 2 lambda, q_filter; out: dq_eff [n], code [n]."""
    _fields_ = [("a", C.c_void_p), ("idx", C.c_void_p), ("q", C.c_void_p), ("k", C.c_float), ("q_filter", C.c_int32),
                ("dq_eff", C.c_void_p), ("code", C.c_void_p)]


class TTDemoLabels(C.Structure):
    """tt_demo_labels (include/ttenv.h): the ring's label array [slots, n_envs] f32 and the labelled lanes [first, first + count)."""
    _fields_ = [("label", C.c_void_p), ("n_envs", C.c_int32), ("slots", C.c_int32), ("first", C.c_int32), ("count", C.c_int32)]


class TTGradClip(C.Structure):
    """tt_grad_clip (include/ttenv.h): max_norm, partials [GRAD_CLIP_PARTIALS] f64, out [2] f32, counts [2] int64 or NULL."""
    _fields_ = [("max_norm", C.c_float), ("partials", C.c_void_p), ("out", C.c_void_p), ("counts", C.c_void_p)]


class TTMpcArgs(C.Structure):
    """tt_mpc_args (include/ttenv.h: tt_env_mpc_plan)."""
    _fields_ = [("horizon", C.c_int32), ("samples", C.c_int32)] + \
               [(n, C.c_float) for n in ("sigma", "rho", "lambda_", "gamma", "k_lat", "k_yaw", "action_scale")] + [("seed", C.c_uint64)]


class TTCurriculum(C.Structure):
    """tt_curriculum (include/ttenv.h: tt_env_set_curriculum)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nyaw", C.c_int32), ("mode", C.c_int32), ("alpha", C.c_double),
                ("uniform", C.c_double)]


class TTCurriculumArrays(C.Structure):
    """tt_curriculum_arrays (include/ttenv.h): p f64, seen u64, attempts / successes / q / cum u32, each [C]; cell u32 [npad]."""
    _fields_ = [(n, C.c_void_p) for n in ("p", "seen", "attempts", "successes", "q", "cum", "cell")]


class TTRandomization(C.Structure):
    """tt_randomization (include/ttenv.h: tt_env_set_randomization): goal_lo, goal_hi (x, y, yaw), L2_lo, L2_hi."""
    _fields_ = [("goal_lo", C.c_double * 3), ("goal_hi", C.c_double * 3), ("L2_lo", C.c_double), ("L2_hi", C.c_double)]


class TTTaskCurriculum(C.Structure):
    """tt_task_curriculum (include/ttenv.h: tt_env_set_task_curriculum): bins (ngx, ngy, ngyaw, nl2), mode, alpha, uniform."""
    _fields_ = [("bins", C.c_int32 * 4), ("mode", C.c_int32), ("alpha", C.c_double), ("uniform", C.c_double)]


class TTHarvest(C.Structure):
    """tt_harvest (include/ttenv.h: tt_ring_harvest): state int64 [8]; the region's obs, act, rew, obs2, done; capacity, tail;
    step_base; work int32 [record_capacity]."""
    _fields_ = [(n, C.c_void_p) for n in ("state", "obs", "act", "rew", "obs2", "done")] + \
               [("capacity", C.c_int32), ("tail", C.c_int32), ("step_base", C.c_int64), ("work", C.c_void_p)]


HARVEST_STATE = ("mark", "written_rows", "episodes", "rows_cut", "expired")     # words 0..4 of tt_harvest.state; 5..7 are zero
CURRICULUM_MAX_CELLS = 4096             # TT_CURRICULUM_MAX_CELLS
CURRICULUM_NO_CELL = 0xFFFFFFFF         # TT_CURRICULUM_NO_CELL
CURRICULUM_MODES = ("frontier", "hard")  # TT_CURRICULUM_FRONTIER, TT_CURRICULUM_HARD
CURRICULUM_ARRAYS = ("p", "seen", "attempts", "successes", "q", "cum", "cell")


class TTLearnLogJob(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("y", "q", "q_pi", "dq_da", "mu", "grad_critic", "grad_actor")] + \
               [("numel_critic", C.c_int32), ("numel_actor", C.c_int32), ("step_dev", C.c_void_p)]


# the values of a learn-log record (TT_LEARN_LOG_NVALUES, include/ttenv.h: tt_learn_log_drain), in their order
LEARN_LOG_VALUES = ("critic_loss", "actor_loss", "q_mean", "q_min", "q_max", "y_mean", "y_min", "y_max", "td_abs_mean", "td_abs_max",
                    "dq_da_abs_mean", "dq_da_abs_max", "mu_abs_mean", "gate_mean", "grad_norm_critic", "grad_norm_actor")
LEARN_LOG_CHUNKS = 16                   # TT_LEARN_LOG_CHUNKS
LEARN_LOG_MAX_CAPACITY = 1 << 22        # TT_LEARN_LOG_MAX_CAPACITY
POP_MAX_AGENTS = 16     # TT_POP_MAX_AGENTS
NSTEP_MAX = 16          # TT_NSTEP_MAX
TD3_NOISE_TAG = 0x7D3E  # the Philox domain of TD3's target-smoothing noise (csrc/tttd3.h)
MPC_NOISE_TAG = 0x4D50  # the Philox domain of the MPC expert's exploration noise (csrc/ttenv_mpc.h)
MPC_MAX_HORIZON, MPC_MAX_SAMPLES = 64, 1024     # TT_MPC_MAX_HORIZON, TT_MPC_MAX_SAMPLES
GRAD_CLIP_PARTIALS = 64     # TT_GRAD_CLIP_PARTIALS


class TTError(RuntimeError):
    pass


_P, _I, _U64 = C.c_void_p, C.c_int, C.c_uint64
_SIGNATURES = {
    "tt_version": (C.c_int, []),
    "tt_last_error": (C.c_char_p, [_P]),
    "tt_params_default": (C.c_int, [_I, C.POINTER(TTParams)]),
    "tt_env_create": (C.c_int, [_I, _I, C.POINTER(TTParams), C.POINTER(_P)]),
    "tt_env_destroy": (C.c_int, [_P]),
    "tt_env_num_envs": (C.c_int, [_P]),
    "tt_env_reset": (C.c_int, [_P, _P, _U64, _P, _P]),
    "tt_env_set_reset_pool": (C.c_int, [_P, _P, _I]),
    "tt_env_set_pose": (C.c_int, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "tt_env_set_attrs": (C.c_int, [_P, _P, _I, _P, _P, _P, _P]),
    "tt_env_set_state": (C.c_int, [_P, _P, _I, _P, _P]),
    "tt_env_get_state": (C.c_int, [_P, _P, _P]),
    "tt_env_set_max_steps": (C.c_int, [_P, _P, _I, _P, _P]),
    "tt_env_set_steps": (C.c_int, [_P, _P, _I, _P, _P]),
    "tt_env_get_episode": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "tt_env_observe": (C.c_int, [_P, _P, _P, _P]),
    "tt_env_set_step_counter": (C.c_int, [_P, _P]),
    "tt_env_step": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(TTInfo), _I, _P]),
    "tt_env_step_random": (C.c_int, [_P, _U64, _P, _P, _P, _P, C.POINTER(TTInfo), _I, _P]),
    "tt_env_state_bytes": (C.c_size_t, [_P]),
    "tt_env_export": (C.c_int, [_P, _P, C.POINTER(C.c_uint64 * 4), _P]),
    "tt_env_import": (C.c_int, [_P, _P, C.POINTER(C.c_uint64 * 4), _P]),
    "tt_env_set_episode_log": (C.c_int, [_P, C.c_int64, _P]),
    "tt_env_drain_episode_log": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tt_env_episode_log_bytes": (C.c_size_t, [_P]),
    "tt_env_export_episode_log": (C.c_int, [_P, _P, C.POINTER(C.c_uint64 * 2), _P]),
    "tt_env_import_episode_log": (C.c_int, [_P, _P, C.POINTER(C.c_uint64 * 2), _P]),
    "tt_env_set_episode_log2": (C.c_int, [_P, C.c_int64, C.c_uint32, _P]),
    "tt_env_drain_episode_log2": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tt_env_set_hold": (C.c_int, [_P, _I, _P]),
    "tt_env_hold_begin": (C.c_int, [_P, _P]),
    "tt_env_step_hold": (C.c_int, [_P, _P, C.c_float, _P, _P]),
    "tt_env_hold_read": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "tt_env_rollout_random": (C.c_int, [_P, _I, _U64, _P, _P, _P, _P]),
    "tt_env_mpc_plan": (C.c_int, [_P, C.POINTER(TTMpcArgs), _P, _P, _P, _P, _P]),
    "tt_env_profile": (C.c_int, [_P, _I]),
    "tt_env_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "tt_mlp_split_ws_bytes": (C.c_uint64, []),
    "tt_mlp_split_pack": (C.c_int, [C.POINTER(TTMlpWeights), _I, _P, _P, C.POINTER(TTRingCursor), _P]),
    "tt_mlp_split_pack_and_sample": (C.c_int, [C.POINTER(TTMlpWeights), _I, _P, C.POINTER(TTSampleArgs), C.POINTER(TTRingCursor), _P]),
    "tt_actor_act_ring": (C.c_int, [_I, C.POINTER(TTRingView), C.POINTER(TTMlpWeights), _P, _U64, _U64, _P, C.c_float, C.c_float,
                                    C.c_float, _P, _P]),
    "tt_env_step_ring": (C.c_int, [_P, _P, C.POINTER(TTRingView), _I, _P]),
    "tt_actor_forward": (C.c_int, [_I, _P, C.POINTER(TTMlpWeights), _P, _P]),
    "tt_actor_act": (C.c_int, [_I, _P, C.POINTER(TTMlpWeights), _P, _P, _U64, _U64, _P, C.c_float, C.c_float, C.c_float,
                               _P, _P, _P, _P]),
    "tt_ring_sample": (C.c_int, [_I, _I, _I, _P, _P, _P, _P, _P, _U64, _I, _I, C.POINTER(TTSideBuffer), _P, _P, _P, _P, _P, _P, _P]),
    "tt_critic_forward": (C.c_int, [_I, _P, _P, C.POINTER(TTMlpWeights), _P, _P]),
    "tt_mlp_forward_save": (C.c_int, [_I, _I, _P, _P, C.POINTER(TTMlpWeights), _P, C.POINTER(TTMlpSaved), _P, _P]),
    "tt_mlp_forward_multi": (C.c_int, [_I, _I, C.POINTER(TTFwdJob), _P]),
    "tt_mlp_forward_multi_sampled": (C.c_int, [_I, _I, C.POINTER(TTFwdJob), C.POINTER(TTSampleArgs), _P, _P]),
    "tt_ring_sample_nstep": (C.c_int, [C.POINTER(TTSampleArgs), _I, C.c_float, _P]),
    "tt_mlp_forward_multi_sampled_nstep": (C.c_int, [_I, _I, C.POINTER(TTFwdJob), C.POINTER(TTSampleArgs), _I, C.c_float, _P, _P]),
    "tt_mlp_backward_rows_pair": (C.c_int, [_I, C.c_float, _P, C.POINTER(TTMlpWeights), C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs),
                                            C.POINTER(TTTdInput), _P, C.POINTER(TTMlpWeights), C.POINTER(TTMlpSaved),
                                            C.POINTER(TTMlpBwdWs), C.POINTER(TTImageJob), _P]),
    "tt_mlp_backward_weights": (C.c_int, [_I, _I, _P, _P, C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs), C.POINTER(TTMlpWeights),
                                          _P, _P, C.c_float, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, _P]),
    "tt_mlp_actor_tail": (C.c_int, [_I, _P, _P, C.POINTER(TTMlpWeights), _P, _P, C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs),
                                    C.POINTER(TTMlpWeights), C.c_float, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, _P, _P, _P]),
    "tt_adam_soft_update": (C.c_int, [_I, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, _P]),
    "tt_p2p_create": (C.c_int, [_I, _I, _I, _I, _P, C.POINTER(_P)]),
    "tt_p2p_destroy": (C.c_int, [_P]),
    "tt_p2p_export": (C.c_int, [_P, _P]),
    "tt_p2p_attach": (C.c_int, [_P, _I, _P]),
    "tt_p2p_grad": (_P, [_P, _I]),
    "tt_p2p_reset": (C.c_int, [_P, _P]),
    "tt_p2p_reset_at": (C.c_int, [_P, C.c_int64, _P]),
    "tt_p2p_set_timeout": (C.c_int, [_P, C.c_double]),
    "tt_p2p_gave_up": (C.c_int, [_P]),
    "tt_p2p_last_error": (C.c_char_p, [_P]),
    "tt_adam_soft_update_p2p": (C.c_int, [_P, _I, _I, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, _P]),
    "tt_mlp_fc2_image_bytes": (C.c_uint64, []),
    "tt_mlp_fc2_image_pack": (C.c_int, [C.POINTER(TTMlpWeights), _P]),
    "tt_random_actions": (C.c_int, [_I, _U64, _U64, _P, _P]),
    "tt_pop_learn_create": (C.c_int, [_I, _I, C.POINTER(TTPopAgent), C.POINTER(_P)]),
    "tt_pop_learn": (C.c_int, [_P, _I, _P]),
    "tt_pop_learn_destroy": (C.c_int, [_P]),
    "tt_pop_exploit": (C.c_int, [_P, _I, C.POINTER(TTPopExploitPair), _P]),
    "tt_pop_hyper": (C.c_int, [_P, _I, C.POINTER(C.c_float * 4)]),
    "tt_pop_learn_set_nstep": (C.c_int, [_P, C.POINTER(TTPopNstep)]),
    "tt_pop_exploit_nstep": (C.c_int, [_P, _I, C.POINTER(TTPopExploitPair), C.POINTER(TTPopNstep), _P]),
    "tt_pop_nstep": (C.c_int, [_P, _I, C.POINTER(TTPopNstep)]),
    "tt_learn_log_create": (C.c_int, [_I, _I, C.POINTER(TTLearnLogJob), C.c_int64, C.c_int32, C.POINTER(_P)]),
    "tt_learn_log_append": (C.c_int, [_P, _P]),
    "tt_learn_log_drain": (C.c_int, [_P, _I, C.c_int64, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "tt_learn_log_clear": (C.c_int, [_P, _P]),
    "tt_learn_log_destroy": (C.c_int, [_P]),
    "tt_td3_create": (C.c_int, [_I, C.POINTER(TTTd3Agent), C.POINTER(_P)]),
    "tt_td3_update": (C.c_int, [_P, C.POINTER(TTTd3Agent)]),
    "tt_td3_learn": (C.c_int, [_P, _I, _I, _P]),
    "tt_td3_destroy": (C.c_int, [_P]),
    "tt_pop_td3_create": (C.c_int, [_I, _I, C.POINTER(TTTd3Agent), C.POINTER(_P)]),
    "tt_pop_td3_learn": (C.c_int, [_P, _I, _I, _P]),
    "tt_pop_td3_exploit": (C.c_int, [_P, _I, C.POINTER(TTPopTd3Pair), _P]),
    "tt_pop_td3_hyper": (C.c_int, [_P, _I, C.POINTER(C.c_float * 6)]),
    "tt_pop_td3_destroy": (C.c_int, [_P]),
    "tt_mlp_backward_rows_pair_shaped": (C.c_int, [_I, C.c_float, _P, C.POINTER(TTMlpWeights), C.POINTER(TTMlpSaved),
                                                   C.POINTER(TTMlpBwdWs), C.POINTER(TTTdInput), _P, C.POINTER(TTMlpWeights),
                                                   C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs), C.POINTER(TTImageJob),
                                                   C.POINTER(TTLossShape), _P]),
    "tt_mlp_backward_weights_shaped": (C.c_int, [_I, _I, _P, _P, C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs), C.POINTER(TTMlpWeights),
                                                 _P, _P, C.c_float, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                                 C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, C.POINTER(TTLossShape), _P]),
    "tt_mlp_actor_tail_shaped": (C.c_int, [_I, _P, _P, C.POINTER(TTMlpWeights), _P, _P, C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs),
                                           C.POINTER(TTMlpWeights), C.c_float, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float,
                                           C.c_float, C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, _P, _P,
                                           C.POINTER(TTLossShape), _P]),
    "tt_mlp_forward_save_demo": (C.c_int, [_I, _I, _P, _P, C.POINTER(TTMlpWeights), _P, C.POINTER(TTMlpSaved), _P,
                                           C.POINTER(TTDemoLoss), _P]),
    "tt_mlp_actor_tail_demo": (C.c_int, [_I, _P, _P, C.POINTER(TTMlpWeights), _P, _P, C.POINTER(TTMlpSaved), C.POINTER(TTMlpBwdWs),
                                         C.POINTER(TTMlpWeights), C.c_float, _I, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, _P, _P,
                                         C.POINTER(TTLossShape), C.POINTER(TTDemoLoss), _P]),
    "tt_env_mpc_act_ring": (C.c_int, [_P, C.POINTER(TTMpcArgs), _P, C.c_int32, C.POINTER(TTRingView), C.c_float, _P, _P]),
    "tt_mlp_forward_save_demo_lanes": (C.c_int, [_I, _I, _P, _P, C.POINTER(TTMlpWeights), _P, C.POINTER(TTMlpSaved), _P,
                                                 C.POINTER(TTDemoLoss), C.c_int32, _P]),
    "tt_mlp_actor_tail_demo_lanes": (C.c_int, [_I, _P, _P, C.POINTER(TTMlpWeights), _P, _P, C.POINTER(TTMlpSaved),
                                               C.POINTER(TTMlpBwdWs), C.POINTER(TTMlpWeights), C.c_float, _I, _P, _P, _P, _P, _P,
                                               C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                               C.POINTER(TTFc2Images), _P, _P, _P, C.POINTER(TTLossShape), C.POINTER(TTDemoLoss),
                                               C.c_int32, _P]),
    "tt_env_mpc_label_ring": (C.c_int, [_P, C.POINTER(TTMpcArgs), _P, C.c_int32, C.c_int32, C.POINTER(TTRingView), _P, C.c_float, _P,
                                        _P]),
    "tt_mlp_forward_save_demo_labels": (C.c_int, [_I, _I, _P, _P, C.POINTER(TTMlpWeights), _P, C.POINTER(TTMlpSaved), _P,
                                                  C.POINTER(TTDemoLoss), C.c_int32, C.POINTER(TTDemoLabels), _P]),
    "tt_mlp_actor_tail_demo_labels": (C.c_int, [_I, _P, _P, C.POINTER(TTMlpWeights), _P, _P, C.POINTER(TTMlpSaved),
                                                C.POINTER(TTMlpBwdWs), C.POINTER(TTMlpWeights), C.c_float, _I, _P, _P, _P, _P, _P,
                                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                                C.POINTER(TTFc2Images), _P, _P, _P, C.POINTER(TTLossShape), C.POINTER(TTDemoLoss),
                                                C.c_int32, C.POINTER(TTDemoLabels), _P]),
    "tt_adam_soft_update_clipped": (C.c_int, [_I, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                              C.c_float, C.c_float, C.POINTER(TTFc2Images), _P, C.POINTER(TTGradClip), _P]),
    "tt_pop_learn_set_clip": (C.c_int, [_P, C.POINTER(TTPopClip)]),
    "tt_pop_clip_write": (C.c_int, [_P, _I, C.POINTER(C.c_int32), C.POINTER(TTPopClip), _P]),
    "tt_pop_clip": (C.c_int, [_P, _I, C.POINTER(TTPopClip), C.POINTER(C.c_float * 4), C.POINTER(C.c_int64 * 4)]),
    "tt_env_set_curriculum": (C.c_int, [_P, C.POINTER(TTCurriculum), C.POINTER(TTCurriculumArrays), _P]),
    "tt_env_curriculum_update": (C.c_int, [_P, _P]),
    "tt_env_curriculum_read": (C.c_int, [_P, C.POINTER(TTCurriculumArrays), _P]),
    "tt_env_curriculum_write": (C.c_int, [_P, C.POINTER(TTCurriculumArrays), _P]),
    "tt_env_set_randomization": (C.c_int, [_P, C.POINTER(TTRandomization), _P]),
    "tt_env_randomization": (C.c_int, [_P, C.POINTER(TTRandomization)]),
    "tt_env_set_task_curriculum": (C.c_int, [_P, C.POINTER(TTTaskCurriculum), C.POINTER(TTCurriculumArrays), _P]),
    "tt_env_task_curriculum_update": (C.c_int, [_P, _P]),
    "tt_env_task_curriculum_read": (C.c_int, [_P, C.POINTER(TTCurriculumArrays), _P]),
    "tt_env_task_curriculum_write": (C.c_int, [_P, C.POINTER(TTCurriculumArrays), _P]),
    "tt_env_task_curriculum": (C.c_int, [_P, C.POINTER(TTTaskCurriculum)]),
    "tt_ring_harvest": (C.c_int, [C.POINTER(TTHarvest), C.POINTER(TTRingView), _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "tt_env_harvest": (C.c_int, [_P, C.POINTER(TTHarvest), C.POINTER(TTRingView), _P, _P]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


def load():
    """dlopen libttenv.so and declare every entry point of include/ttenv.h."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # torch first: it brings its own copy of the HIP runtime (torch/lib/libamdhip64.so, loaded by path), and libttenv.so then
        # binds to that copy by its soname.  The other way round the process holds TWO runtimes -- /opt/rocm's for this library,
        # torch's for the tensors it is handed -- and tt_env_create finds no device in its own (seen on the GPU box with
        # `g.build(); g.smoke()`, where build() loaded the library before anything had imported torch)
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def ptr(t):
    """A tensor's device address as the `void *` of a call or of a struct field (None: NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device=None):
    """torch's current stream on `device` (None: the current device) as a tt_stream_t."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc, handle=None):
    if rc != TT_OK:
        msg = load().tt_last_error(handle)
        raise TTError(f"libttenv error {rc}: {msg.decode() if msg else '?'}")


def check_p2p(rc, handle=None):
    if rc != TT_OK:
        msg = load().tt_p2p_last_error(handle)
        raise TTError(f"libttenv p2p error {rc}: {msg.decode() if msg else '?'}")


P2P_HANDLE_BYTES, P2P_MAX_RANKS = 128, 8


def default_params(variant=0):
    p = TTParams()
    check(load().tt_params_default(variant, C.byref(p)))
    return p
