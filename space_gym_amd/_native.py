"""ctypes binding of libspacegym_hip.so (include/spacegym.h).  There is no CPU path: if the HIP library is
missing or no GPU is visible, creating an engine raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPACEGYM_LIB points at another build of the SAME library (e.g. the stamped diagnostic build); never at a CPU path
LIB_PATH = os.environ.get("SPACEGYM_LIB") or os.path.join(_HERE, "lib", "libspacegym_hip.so")
_lib = None


class SgConfig(C.Structure):
    _fields_ = [("env_id", C.c_char * 64), ("num_envs", C.c_int64), ("seed", C.c_uint64),
                ("env_index_base", C.c_uint32), ("max_episode_steps", C.c_int32), ("auto_reset", C.c_int32),
                ("steering", C.c_int32)]


class SgParams(C.Structure):
    """sg_params (include/spacegym.h): the reference's constructor kwargs; NaN / -1 keeps the id's registered value"""
    _fields_ = [("struct_size", C.c_uint32), ("n_planets", C.c_int32), ("randomize", C.c_int32), ("reserved", C.c_int32),
                ("goal_vel_reward_scale", C.c_double), ("safety_reward_scale", C.c_double), ("goal_sparse_reward", C.c_double),
                ("survival_reward_scale", C.c_double), ("danger_zone", C.c_double),
                ("ref_orbit_a", C.c_double), ("ref_orbit_eccentricity", C.c_double), ("ref_orbit_angle", C.c_double),
                ("numerator_C", C.c_double), ("rad_penalty_C", C.c_double), ("act_penalty_C", C.c_double), ("step_size", C.c_double),
                ("ship_moi", C.c_double), ("max_engine_force", C.c_double)]


class SgTerminalList(C.Structure):
    _fields_ = [("count", C.c_void_p), ("step_env", C.c_void_p), ("obs", C.c_void_p), ("capacity", C.c_uint32)]


class SgEpisodeList(C.Structure):
    _fields_ = [("count", C.c_void_p), ("step_env", C.c_void_p), ("ret", C.c_void_p), ("length", C.c_void_p),
                ("truncated", C.c_void_p), ("capacity", C.c_uint32)]


class SgNormalize(C.Structure):
    """sg_normalize (include/spacegym.h): running observation / reward normalization (gym NormalizeObservation /
    NormalizeReward); sg_normalize_init fills in gym's defaults"""
    _fields_ = [("struct_size", C.c_uint32), ("obs", C.c_int32), ("reward", C.c_int32), ("update", C.c_int32),
                ("gamma", C.c_double), ("epsilon", C.c_double), ("clip_obs", C.c_double), ("clip_reward", C.c_double)]


class SgRenderConfig(C.Structure):
    """sg_render_config (include/spacegym.h): render(mode="rgb_array") on the device; sg_render_config_init fills in capacity 1
    and the family's trace length, decay and lidar switch (-1 / NaN)"""
    _fields_ = [("struct_size", C.c_uint32), ("capacity", C.c_int32), ("trace_len", C.c_int32), ("debug_lidar", C.c_int32),
                ("trace_decay", C.c_double)]


class SgRewardProfile(C.Structure):
    """sg_reward_profile (include/spacegym.h): values of the reward-only constructor kwargs of one reward profile; NaN keeps the
    handle's own value"""
    _fields_ = [("struct_size", C.c_uint32), ("survival_reward_scale", C.c_double), ("goal_vel_reward_scale", C.c_double),
                ("safety_reward_scale", C.c_double), ("goal_sparse_reward", C.c_double), ("danger_zone", C.c_double),
                ("numerator_C", C.c_double), ("rad_penalty_C", C.c_double), ("act_penalty_C", C.c_double)]


class SgGaeConfig(C.Structure):
    """sg_gae_config (include/spacegym.h): sg_gae_config_init fills in gamma 0.99, lambda 0.95, bootstrap_truncated 1"""
    _fields_ = [("struct_size", C.c_uint32), ("gamma", C.c_double), ("lambda_", C.c_double), ("bootstrap_truncated", C.c_int32)]


class SgValueList(C.Structure):
    """sg_value_list (include/spacegym.h): a rollout's terminal list with the caller's values of its observations"""
    _fields_ = [("count", C.c_void_p), ("step_env", C.c_void_p), ("value", C.c_void_p), ("capacity", C.c_uint32)]


class SgReturnsConfig(C.Structure):
    """sg_returns_config (include/spacegym.h): sg_returns_config_init fills in gamma 0.99, lambda 0.95, bootstrap_truncated 1, the three
    bars 1.0, groups 0"""
    _fields_ = [("struct_size", C.c_uint32), ("groups", C.c_int32), ("discounts", C.c_void_p), ("gamma", C.c_double), ("lambda_", C.c_double),
                ("bootstrap_truncated", C.c_int32), ("rho_bar", C.c_double), ("c_bar", C.c_double), ("pg_rho_bar", C.c_double),
                ("reserved", C.c_int32)]


class SgRetraceConfig(C.Structure):
    """sg_retrace_config (include/spacegym.h): sg_retrace_config_init fills in gamma 0.99, lambda 1.0, c_bar 1.0, bootstrap_truncated 1,
    huber_delta +inf and a null discounts"""
    _fields_ = [("struct_size", C.c_uint32), ("gamma", C.c_double), ("lambda_", C.c_double), ("c_bar", C.c_double),
                ("bootstrap_truncated", C.c_int32), ("huber_delta", C.c_float), ("discounts", C.c_void_p), ("reserved", C.c_int32)]


class SgReplay(C.Structure):
    """sg_replay (include/spacegym.h): the members of a replay ring in device memory"""
    _fields_ = [("struct_size", C.c_uint32), ("steps", C.c_int32), ("term_capacity", C.c_uint32), ("reserved", C.c_uint32),
                ("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("trunc", C.c_void_p),
                ("term_idx", C.c_void_p), ("term_obs", C.c_void_p), ("slot_seq", C.c_void_p), ("hdr", C.c_void_p)]


class SgReplaySampleConfig(C.Structure):
    """sg_replay_sample_config (include/spacegym.h): sg_replay_sample_config_init fills in seed 0, n_step 1, gamma 0.99"""
    _fields_ = [("struct_size", C.c_uint32), ("seed", C.c_uint64), ("n_step", C.c_int32), ("gamma", C.c_double)]


class SgReplayBatch(C.Structure):
    """sg_replay_batch (include/spacegym.h): the outputs of sg_replay_sample_device"""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("next_obs", C.c_void_p),
                ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("discount", C.c_void_p), ("steps", C.c_void_p),
                ("index", C.c_void_p)]


class SgReplaySequenceConfig(C.Structure):
    """sg_replay_sequence_config (include/spacegym.h): sg_replay_sequence_config_init fills in seed 0, length 1, n_extra 0"""
    _fields_ = [("struct_size", C.c_uint32), ("seed", C.c_uint64), ("length", C.c_int32), ("n_extra", C.c_int32)]


class SgReplaySequences(C.Structure):
    """sg_replay_sequences (include/spacegym.h): the outputs of sg_replay_sequence_device and the extra columns it gathers"""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("trunc", C.c_void_p),
                ("terminal_obs", C.c_void_p), ("index", C.c_void_p), ("extra_in", C.c_void_p * 4), ("extra_out", C.c_void_p * 4)]


class SgReplayRelabelConfig(C.Structure):
    """sg_replay_relabel_config (include/spacegym.h): sg_replay_relabel_config_init fills in seed 0, her_ratio 0.8, horizon 1, strategy 0"""
    _fields_ = [("struct_size", C.c_uint32), ("seed", C.c_uint64), ("her_ratio", C.c_double), ("horizon", C.c_int32),
                ("strategy", C.c_int32)]


class SgReplayRelabelOut(C.Structure):
    """sg_replay_relabel_out (include/spacegym.h): the optional outputs of sg_replay_relabel_device"""
    _fields_ = [("relabelled", C.c_void_p), ("offset", C.c_void_p), ("goal", C.c_void_p)]


class SgPriority(C.Structure):
    """sg_priority (include/spacegym.h): the members of the priorities of a replay ring in device memory"""
    _fields_ = [("struct_size", C.c_uint32), ("steps", C.c_int32), ("frac_bits", C.c_int32), ("reserved", C.c_uint32),
                ("leaf", C.c_void_p), ("node", C.c_void_p), ("hdr", C.c_void_p)]


class SgPrioritySampleConfig(C.Structure):
    """sg_priority_sample_config (include/spacegym.h): sg_priority_sample_config_init fills in seed 0, beta 0.4, stratified 1"""
    _fields_ = [("struct_size", C.c_uint32), ("seed", C.c_uint64), ("beta", C.c_double), ("stratified", C.c_int32)]


class SgPriorityDraw(C.Structure):
    """sg_priority_draw (include/spacegym.h): the outputs of sg_priority_sample_device"""
    _fields_ = [("index", C.c_void_p), ("cell", C.c_void_p), ("weight", C.c_void_p), ("leaf", C.c_void_p)]


class SgPolicyMlp(C.Structure):
    """sg_policy_mlp (include/spacegym.h): device pointers of one net's layers, torch.nn.Linear layout"""
    _fields_ = [("weight", C.c_void_p * 4), ("bias", C.c_void_p * 4)]


class SgPolicy(C.Structure):
    """sg_policy (include/spacegym.h): a small MLP actor-critic whose parameters stay where the learner keeps them"""
    _fields_ = [("struct_size", C.c_uint32), ("n_hidden", C.c_int32), ("hidden", C.c_int32), ("activation", C.c_int32),
                ("head", C.c_int32), ("reserved", C.c_int32), ("actor", SgPolicyMlp), ("critic", SgPolicyMlp), ("log_std", C.c_void_p)]


class SgPolicyGrads(C.Structure):
    """sg_policy_grads (include/spacegym.h): where sg_policy_grad_device writes the gradient of every parameter of an sg_policy"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("actor", SgPolicyMlp), ("critic", SgPolicyMlp), ("log_std", C.c_void_p)]


class SgPpoConfig(C.Structure):
    """sg_ppo_config (include/spacegym.h): sg_ppo_config_init fills in clip_range 0.2, clip_range_vf 0 (off), ent_coef 0, vf_coef 0.5,
    normalize_advantage 1, adv_epsilon 1e-8"""
    _fields_ = [("struct_size", C.c_uint32), ("clip_range", C.c_float), ("clip_range_vf", C.c_float), ("ent_coef", C.c_float),
                ("vf_coef", C.c_float), ("normalize_advantage", C.c_int32), ("adv_epsilon", C.c_float), ("reserved", C.c_int32)]


class SgPpoBatch(C.Structure):
    """sg_ppo_batch (include/spacegym.h): the columns of the flattened rollout and the minibatch's int64 row index"""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("old_logp", C.c_void_p), ("advantage", C.c_void_p), ("ret", C.c_void_p),
                ("old_value", C.c_void_p), ("index", C.c_void_p)]


class SgPpoRows(C.Structure):
    """sg_ppo_rows (include/spacegym.h): optional per-row outputs of sg_ppo_grad_device"""
    _fields_ = [("logp", C.c_void_p), ("value", C.c_void_p), ("g_logp", C.c_void_p), ("g_value", C.c_void_p)]


class SgAdamTensor(C.Structure):
    """sg_adam_tensor (include/spacegym.h): one parameter tensor stacked [members, numel] with its gradient and its two moments"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64)]


class SgPbtColumn(C.Structure):
    """sg_pbt_column (include/spacegym.h): one hyperparameter column of a float32 [members, C] tensor and how explore perturbs it"""
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int64), ("mode", C.c_int32), ("down", C.c_float), ("up", C.c_float), ("lo", C.c_float),
                ("hi", C.c_float)]


class SgQnet(C.Structure):
    """sg_qnet (include/spacegym.h): one or two Q critics on [obs | action] rows, parameters read where the learner keeps them"""
    _fields_ = [("struct_size", C.c_uint32), ("n_critics", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32),
                ("activation", C.c_int32), ("critic", SgPolicyMlp * 2)]


class SgQnetGrads(C.Structure):
    """sg_qnet_grads (include/spacegym.h): where sg_q_grad_device writes the gradient of every parameter of an sg_qnet"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("critic", SgPolicyMlp * 2)]


class SgSquashedPolicy(C.Structure):
    """sg_squashed_policy (include/spacegym.h): the SAC actor -- a tanh-squashed Gaussian whose head gives mean and raw log_std"""
    _fields_ = [("struct_size", C.c_uint32), ("n_hidden", C.c_int32), ("hidden", C.c_int32), ("activation", C.c_int32),
                ("log_std_min", C.c_float), ("log_std_max", C.c_float), ("actor", SgPolicyMlp), ("reserved", C.c_int32)]


class SgSquashedGrads(C.Structure):
    """sg_squashed_grads (include/spacegym.h): where sg_squashed_grad_device writes the gradient of every parameter of the actor"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("actor", SgPolicyMlp)]


class SgDqn(C.Structure):
    """sg_dqn (include/spacegym.h): the DQN head of the discrete ids -- one MLP Q(obs) -> 6, parameters read where the learner keeps them"""
    _fields_ = [("struct_size", C.c_uint32), ("n_hidden", C.c_int32), ("hidden", C.c_int32), ("activation", C.c_int32),
                ("reserved", C.c_int32), ("net", SgPolicyMlp)]


class SgDqnGrads(C.Structure):
    """sg_dqn_grads (include/spacegym.h): where sg_dqn_grad_device writes the gradient of every parameter of an sg_dqn"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("net", SgPolicyMlp)]


class SgDqnTdConfig(C.Structure):
    """sg_dqn_td_config (include/spacegym.h): sg_dqn_td_config_init fills in double_q 1 and huber_delta 1"""
    _fields_ = [("struct_size", C.c_uint32), ("double_q", C.c_int32), ("huber_delta", C.c_float), ("reserved", C.c_int32)]


class SgDqnTdBatch(C.Structure):
    """sg_dqn_td_batch (include/spacegym.h): the columns of a replay batch and the optional importance weights"""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("next_obs", C.c_void_p), ("terminated", C.c_void_p),
                ("discount", C.c_void_p), ("weight", C.c_void_p)]


class SgDqnTdRows(C.Structure):
    """sg_dqn_td_rows (include/spacegym.h): optional per-row outputs of sg_dqn_td_grad_device"""
    _fields_ = [("td_error", C.c_void_p), ("q_taken", C.c_void_p), ("target", C.c_void_p), ("q_next", C.c_void_p), ("g", C.c_void_p)]


class SgQTdConfig(C.Structure):
    """sg_q_td_config (include/spacegym.h): sg_q_td_config_init fills in huber_delta +inf, alpha 0.2, noise_std 0.2, noise_clip 0.5 and
    action_clip 1"""
    _fields_ = [("struct_size", C.c_uint32), ("huber_delta", C.c_float), ("alpha", C.c_float), ("noise_std", C.c_float),
                ("noise_clip", C.c_float), ("action_clip", C.c_float), ("reserved", C.c_int32 * 2)]


class SgQTdBatch(C.Structure):
    """sg_q_td_batch (include/spacegym.h): the columns of a replay batch, the target action and the optional weights, log-probs, device
    alpha and smoothing noise"""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("next_obs", C.c_void_p), ("terminated", C.c_void_p),
                ("discount", C.c_void_p), ("next_action", C.c_void_p), ("weight", C.c_void_p), ("next_logp", C.c_void_p),
                ("alpha_dev", C.c_void_p), ("noise", C.c_void_p)]


class SgQTdRows(C.Structure):
    """sg_q_td_rows (include/spacegym.h): optional per-row outputs of sg_q_td_grad_device"""
    _fields_ = [("td1", C.c_void_p), ("td2", C.c_void_p), ("q1", C.c_void_p), ("q2", C.c_void_p), ("target", C.c_void_p),
                ("q_next", C.c_void_p), ("g1", C.c_void_p), ("g2", C.c_void_p), ("td_abs", C.c_void_p)]


class SgQActorConfig(C.Structure):
    """sg_q_actor_config (include/spacegym.h): sg_q_actor_config_init fills in alpha 0.2, target_entropy -2 and q_select -1 (the default:
    the minimum for the squashed actor on two critics, else critic 1)"""
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("target_entropy", C.c_float), ("q_select", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class SgQActorRows(C.Structure):
    """sg_q_actor_rows (include/spacegym.h): optional per-row outputs of sg_q_actor_squashed_grad_device / sg_q_actor_gaussian_grad_device"""
    _fields_ = [("action", C.c_void_p), ("logp", C.c_void_p), ("q1", C.c_void_p), ("q2", C.c_void_p), ("q_sel", C.c_void_p),
                ("dq1_da", C.c_void_p), ("dq2_da", C.c_void_p), ("g_action", C.c_void_p)]


class SgCounters(C.Structure):
    _fields_ = [("env_steps", C.c_uint64), ("episodes_finished", C.c_uint64), ("truncations", C.c_uint64), ("goal_hits", C.c_uint64)]


class NativeError(RuntimeError):
    pass


# every symbol include/spacegym.h declares: (restype, argtypes)
_fp, _u8p, _i32p, _vp = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_void_p
SYMBOLS = {
    "sg_create": (C.c_int, [C.POINTER(SgConfig), C.c_int, C.POINTER(_vp)]),
    "sg_create_ex": (C.c_int, [C.POINTER(SgConfig), C.POINTER(SgParams), C.c_int, C.POINTER(_vp)]),
    "sg_params_init": (None, [C.POINTER(SgParams)]),
    "sg_get_params": (C.c_int, [_vp, C.POINTER(SgParams)]),
    "sg_create_sharded": (C.c_int, [C.POINTER(SgConfig), C.c_int, C.POINTER(C.c_int), C.POINTER(_vp)]),
    "sg_create_sharded_ex": (C.c_int, [C.POINTER(SgConfig), C.POINTER(SgParams), C.c_int, C.POINTER(C.c_int), C.POINTER(_vp)]),
    "sg_destroy": (C.c_int, [_vp]),
    "sg_last_error": (C.c_char_p, [_vp]),
    "sg_num_envs": (C.c_int64, [_vp]),
    "sg_obs_dim": (C.c_int32, [_vp]),
    "sg_num_planets": (C.c_int32, [_vp]),
    "sg_discrete_actions": (C.c_int32, [_vp]),
    "sg_seed": (C.c_int, [_vp, C.c_uint64]),
    "sg_set_auto_reset": (C.c_int, [_vp, C.c_int32]),
    "sg_reset": (C.c_int, [_vp, _vp]),
    "sg_reset_device": (C.c_int, [_vp, _vp, _vp]),
    "sg_reset_masked": (C.c_int, [_vp, _vp, _vp]),
    "sg_reset_masked_device": (C.c_int, [_vp, _vp, _vp, _vp]),
    "sg_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_step_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_step_begin": (C.c_int, [_vp, _vp, C.c_int32]),
    "sg_step_end": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "sg_rollout_device": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_set_unfused_rollout": (C.c_int, [_vp, C.c_int32]),
    "sg_rollout_device_terminal": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgTerminalList), _vp]),
    "sg_set_episode_stats": (C.c_int, [_vp, C.c_int32]),
    "sg_step_device_episodes": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_step_episodes": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_step_end_episodes": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "sg_rollout_device_episodes": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgTerminalList),
                                             C.POINTER(SgEpisodeList), _vp]),
    "sg_normalize_init": (None, [C.POINTER(SgNormalize)]),
    "sg_set_normalize": (C.c_int, [_vp, C.POINTER(SgNormalize)]),
    "sg_get_normalize": (C.c_int, [_vp, C.POINTER(SgNormalize)]),
    "sg_normalize_reserve": (C.c_int, [_vp, C.c_int32]),
    "sg_get_normalize_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_set_normalize_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_render_config_init": (None, [C.POINTER(SgRenderConfig)]),
    "sg_set_render": (C.c_int, [_vp, C.POINTER(SgRenderConfig)]),
    "sg_render_device": (C.c_int, [_vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp]),
    "sg_render": (C.c_int, [_vp, C.c_int32, _vp, _vp, C.c_int32, _vp]),
    "sg_reward_profile_init": (None, [C.POINTER(SgRewardProfile)]),
    "sg_set_reward_profiles": (C.c_int, [_vp, C.c_int32, C.POINTER(SgRewardProfile)]),
    "sg_get_reward_profiles": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(SgRewardProfile), C.c_int32]),
    "sg_set_env_profiles": (C.c_int, [_vp, _vp]),
    "sg_set_env_profiles_device": (C.c_int, [_vp, _vp, _vp]),
    "sg_get_env_profiles": (C.c_int, [_vp, _vp]),
    "sg_check_status": (C.c_int, [_vp]),
    "sg_set_counters": (C.c_int, [_vp, C.c_int32]),
    "sg_get_counters": (C.c_int, [_vp, C.POINTER(SgCounters), C.c_int32]),
    "sg_state_bytes": (C.c_size_t, [_vp]),
    "sg_save_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "sg_load_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "sg_snapshot_bytes": (C.c_size_t, [_vp]),
    "sg_snapshot_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "sg_restore_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "sg_gae_config_init": (None, [C.POINTER(SgGaeConfig)]),
    "sg_gae_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgGaeConfig), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgValueList), _vp, _vp, _vp]),
    "sg_gae": (C.c_int, [_vp, C.c_int32, C.POINTER(SgGaeConfig), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgValueList), _vp, _vp]),
    "sg_returns_config_init": (None, [C.POINTER(SgReturnsConfig)]),
    "sg_gae_groups_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgReturnsConfig), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgValueList), _vp, _vp,
                                       _vp]),
    "sg_vtrace_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgReturnsConfig), _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgValueList), _vp, _vp,
                                   _vp]),
    "sg_retrace_config_init": (None, [C.POINTER(SgRetraceConfig)]),
    "sg_retrace_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(SgRetraceConfig), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp]),
    "sg_replay_bytes": (C.c_size_t, [_vp, C.c_int32, C.c_uint32, C.POINTER(C.c_size_t)]),
    "sg_replay_begin_device": (C.c_int, [_vp, C.POINTER(SgReplay), _vp, _vp]),
    "sg_replay_commit_device": (C.c_int, [_vp, C.POINTER(SgReplay), C.c_int32, C.c_int32, C.c_int32, C.POINTER(SgTerminalList), _vp, _vp]),
    "sg_replay_sample_config_init": (None, [C.POINTER(SgReplaySampleConfig)]),
    "sg_replay_sample_device": (C.c_int, [_vp, C.POINTER(SgReplay), C.POINTER(SgReplaySampleConfig), C.c_int64, _vp,
                                          C.POINTER(SgReplayBatch), _vp]),
    "sg_replay_sequence_config_init": (None, [C.POINTER(SgReplaySequenceConfig)]),
    "sg_replay_sequence_device": (C.c_int, [_vp, C.POINTER(SgReplay), C.POINTER(SgReplaySequenceConfig), C.c_int64, _vp,
                                            C.POINTER(SgReplaySequences), _vp]),
    "sg_replay_relabel_config_init": (None, [C.POINTER(SgReplayRelabelConfig)]),
    "sg_replay_relabel_device": (C.c_int, [_vp, C.POINTER(SgReplay), C.POINTER(SgReplayRelabelConfig), C.c_int64, C.POINTER(SgReplayBatch),
                                           C.POINTER(SgReplayRelabelOut), _vp]),
    "sg_priority_bytes": (C.c_size_t, [_vp, C.c_int32, C.POINTER(C.c_size_t)]),
    "sg_priority_begin_device": (C.c_int, [_vp, C.POINTER(SgPriority), _vp]),
    "sg_priority_commit_device": (C.c_int, [_vp, C.POINTER(SgPriority), C.c_int32, C.c_int32, C.c_int32, _vp]),
    "sg_priority_update_device": (C.c_int, [_vp, C.POINTER(SgPriority), C.c_int64, _vp, _vp, _vp]),
    "sg_priority_sample_config_init": (None, [C.POINTER(SgPrioritySampleConfig)]),
    "sg_priority_sample_device": (C.c_int, [_vp, C.POINTER(SgReplay), C.POINTER(SgPriority), C.POINTER(SgPrioritySampleConfig), C.c_int64,
                                            C.POINTER(SgPriorityDraw), _vp]),
    "sg_policy_act_device": (C.c_int, [_vp, C.POINTER(SgPolicy), _vp, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp]),
    "sg_rollout_policy_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgPolicy), C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, C.POINTER(SgTerminalList), _vp, _vp]),
    "sg_policy_evaluate_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_policy_grad_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int64, _vp, _vp, _vp, _vp, _vp, C.POINTER(SgPolicyGrads), _vp, C.c_size_t, _vp]),
    "sg_policy_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgPolicy), C.c_int64]),
    "sg_ppo_config_init": (None, [C.POINTER(SgPpoConfig)]),
    "sg_ppo_grad_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.POINTER(SgPpoConfig), C.POINTER(SgPpoBatch), C.c_int64, C.c_int64,
                                     C.POINTER(SgPolicyGrads), _vp, C.POINTER(SgPpoRows), _vp, C.c_size_t, _vp]),
    "sg_ppo_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgPolicy), C.c_int64]),
    "sg_q_evaluate_device": (C.c_int, [_vp, C.POINTER(SgQnet), C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "sg_q_grad_device": (C.c_int, [_vp, C.POINTER(SgQnet), C.c_int64, _vp, _vp, _vp, _vp, C.POINTER(SgQnetGrads), _vp, _vp, C.c_size_t, _vp]),
    "sg_q_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgQnet), C.c_int64]),
    "sg_policy_action_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int64, _vp, _vp, _vp, _vp]),
    "sg_policy_action_grad_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int64, _vp, _vp, _vp, C.POINTER(SgPolicyGrads), _vp, C.c_size_t, _vp]),
    "sg_squashed_act_device": (C.c_int, [_vp, C.POINTER(SgSquashedPolicy), _vp, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp]),
    "sg_squashed_sample_device": (C.c_int, [_vp, C.POINTER(SgSquashedPolicy), C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "sg_squashed_grad_device": (C.c_int, [_vp, C.POINTER(SgSquashedPolicy), C.c_int64, _vp, _vp, _vp, _vp, C.POINTER(SgSquashedGrads), _vp,
                                          C.c_size_t, _vp]),
    "sg_squashed_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgSquashedPolicy), C.c_int64]),
    "sg_rollout_squashed_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgSquashedPolicy), C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp,
                                             _vp, _vp, C.POINTER(SgTerminalList), _vp]),
    "sg_dqn_act_device": (C.c_int, [_vp, C.POINTER(SgDqn), _vp, C.c_uint64, C.c_uint64, C.c_float, _vp, _vp, _vp, _vp]),
    "sg_rollout_dqn_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgDqn), C.c_uint64, C.c_uint64, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        C.POINTER(SgTerminalList), _vp]),
    "sg_dqn_evaluate_device": (C.c_int, [_vp, C.POINTER(SgDqn), C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_dqn_grad_device": (C.c_int, [_vp, C.POINTER(SgDqn), C.c_int64, _vp, _vp, _vp, _vp, C.POINTER(SgDqnGrads), _vp, C.c_size_t, _vp]),
    "sg_dqn_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgDqn), C.c_int64]),
    "sg_dqn_td_config_init": (None, [C.POINTER(SgDqnTdConfig)]),
    "sg_dqn_td_grad_device": (C.c_int, [_vp, C.POINTER(SgDqn), C.POINTER(SgDqn), C.POINTER(SgDqnTdConfig), C.POINTER(SgDqnTdBatch), C.c_int64,
                                        C.POINTER(SgDqnGrads), _vp, C.POINTER(SgDqnTdRows), _vp, C.c_size_t, _vp]),
    "sg_dqn_td_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgDqn), C.c_int64]),
    "sg_q_td_config_init": (None, [C.POINTER(SgQTdConfig)]),
    "sg_q_td_grad_device": (C.c_int, [_vp, C.POINTER(SgQnet), C.POINTER(SgQnet), C.POINTER(SgQTdConfig), C.POINTER(SgQTdBatch), C.c_int64,
                                      C.POINTER(SgQnetGrads), _vp, C.POINTER(SgQTdRows), _vp, C.c_size_t, _vp]),
    "sg_q_td_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgQnet), C.c_int64]),
    "sg_q_actor_config_init": (None, [C.POINTER(SgQActorConfig)]),
    "sg_q_actor_squashed_grad_device": (C.c_int, [_vp, C.POINTER(SgSquashedPolicy), C.POINTER(SgQnet), C.POINTER(SgQActorConfig), C.c_int64, _vp, _vp,
                                                  _vp, C.POINTER(SgSquashedGrads), _vp, C.POINTER(SgQActorRows), _vp, C.c_size_t, _vp]),
    "sg_q_actor_gaussian_grad_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.POINTER(SgQnet), C.POINTER(SgQActorConfig), C.c_int64, _vp, _vp, _vp,
                                                  C.POINTER(SgPolicyGrads), _vp, C.POINTER(SgQActorRows), _vp, C.c_size_t, _vp]),
    "sg_q_actor_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgSquashedPolicy), C.POINTER(SgPolicy), C.POINTER(SgQnet), C.c_int64]),
    "sg_policy_population_act_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int32, _vp, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp]),
    "sg_rollout_policy_population_device": (C.c_int, [_vp, C.c_int32, C.POINTER(SgPolicy), C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp,
                                                      _vp, _vp, _vp, _vp, _vp, C.POINTER(SgTerminalList), _vp, _vp]),
    "sg_policy_population_evaluate_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sg_policy_population_grad_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp,
                                                   C.POINTER(SgPolicyGrads), _vp, C.c_size_t, _vp]),
    "sg_policy_population_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgPolicy), C.c_int32, C.c_int64]),
    "sg_ppo_population_grad_device": (C.c_int, [_vp, C.POINTER(SgPolicy), C.c_int32, C.POINTER(SgPpoConfig), C.POINTER(SgPpoBatch), _vp, C.c_int64,
                                                C.c_int64, C.POINTER(SgPolicyGrads), _vp, C.POINTER(SgPpoRows), _vp, C.c_size_t, _vp]),
    "sg_ppo_population_grad_workspace_bytes": (C.c_size_t, [_vp, C.POINTER(SgPolicy), C.c_int32, C.c_int64]),
    "sg_adam_step_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(SgAdamTensor), _vp, _vp, _vp]),
    "sg_adam_exploit_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(SgAdamTensor), _vp, _vp, _vp, _vp]),
    "sg_pbt_fitness_device": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "sg_pbt_fitness_workspace_bytes": (C.c_size_t, [_vp, C.c_int32]),
    "sg_pbt_fitness_clear_device": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "sg_pbt_select_device": (C.c_int, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int32, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "sg_pbt_explore_device": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, C.POINTER(SgPbtColumn), C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    "sg_minibatch_size": (C.c_int64, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sg_minibatch_index_device": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    "sg_get_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "sg_set_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "sg_vector_field": (C.c_int, [_vp, _vp, _vp, _vp]),
    "sg_host_alloc": (_vp, [C.c_size_t]),
    "sg_host_free": (None, [_vp]),
    "sg_set_profiling": (C.c_int, [_vp, C.c_int32]),
    "sg_get_profile": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sg_stream": (_vp, [_vp]),
    "sg_rollout_kernel": (C.c_char_p, [_vp, C.c_int32]),
    "sg_random_actions_device": (C.c_int, [_vp, C.c_int32, C.c_uint64, C.c_uint64, _vp, _vp]),
    "sg_version": (C.c_char_p, []),
}


def load():
    """Load the HIP library once.  torch (if installed) is imported first so that both use the same HIP runtime
    (torch bundles libamdhip64 under the same SONAME) and device pointers can be shared."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} not found: build it with `python -m space_gym_amd.build` "
                          "(hipcc, gfx950). The engine is HIP-only; there is no CPU fallback.")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        except AttributeError:
            if not os.environ.get("SPACEGYM_LIB"):
                raise
            continue  # an older diagnostic build of the same library (A/B measurements): newer entry points are absent
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    if rc != 0:
        msg = lib.sg_last_error(handle)
        raise NativeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
