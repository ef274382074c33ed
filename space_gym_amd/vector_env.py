"""gym.vector.VectorEnv-shaped front end of the HIP engine.

Mirrors the reference's env surface for the step path -- `reset() -> obs`, `step(a) -> (obs, reward, done, info)`
(old-gym 4-tuple, gym_space/envs/spaceship_env.py:59-78), `seed(s)` (:92-94), observation/action spaces
(:102-111,206-208; kepler.py:158-170) -- batched over `num_envs` instances, with what gym.wrappers.TimeLimit
(max_episode_steps=500, gym_space/__init__.py:29) and a VectorEnv add: per-env step counters, truncation and
auto-reset, all inside the step kernel.

Two I/O modes:
  * NumPy (`reset`, `step` = `step_async` + `step_wait`): host arrays in/out (H2D + kernel + D2H per step).  step_async
    enqueues all of it (sg_step_begin) and returns; step_wait waits (sg_step_end) and hands out the step's results, which
    sit in one of two page-locked blocks that alternate -- with copy=False the arrays of step t stay valid while step t + 1
    is in flight;
  * torch (`reset_torch`, `step_torch`, `rollout_torch`): device tensors in/out through sg_step_device on torch's
    current stream, zero-copy -- the high-throughput path.

Episode statistics (`episode_statistics=True` / `set_episode_statistics`): the return and length of every finished episode,
with gym.wrappers.RecordEpisodeStatistics' semantics, summed on the device by a pass behind every stepping call --
`info["episode"]` / `info["_episode"]` of step(), `episodes=` of step_torch and rollout_torch.

Normalization (`normalize_obs=True` / `normalize_reward=True`, `set_normalization`): gym's NormalizeObservation and
NormalizeReward with running float64 statistics on the device; every call that returns observations or rewards returns them
normalized (reset, step, step_torch, rollout_torch, prepare_rollout), terminal observations included.

Masked reset (`reset(mask=...)`, `reset_torch(mask=...)`): only the chosen envs restart, with the episode auto-reset would
start for them -- the loop of a training run with `auto_reset=False` (gymnasium's `reset(options={"reset_mask": ...})`).

Rendering (`render=True` / `render=dict(...)`, `set_render`): `render(mode="rgb_array")` of the reference's Renderer
(gym_space/rendering.py) for chosen envs, drawn on the device -- `render()` (NumPy) and `render_torch()` (device tensor).
"""
import ctypes as C
import math

import numpy as np

from . import _native
from .registration import (ENV_CLASSES, ENV_SPECS, constructor_kwargs, is_discrete, obs_dim, single_action_space,
                           single_observation_space)
from .spaces import MultiDiscrete, batch_box


_KEEP = object()  # set_normalization: leave the value as it is


class StepInfo(dict):
    """Batched info: {"TimeLimit.truncated": bool[B], "terminal_observation": float32[B, D] (rows of finished envs)}; with
    episode statistics on also "episode": {"r": float64[B], "l": int32[B]} and the mask "_episode": bool[B] of the envs whose
    episode ended (gymnasium's vector convention; other rows of "r" / "l" read NaN / -1).
    A per-env list of dicts (old gym VectorEnv) would cost more than the step itself at B = 65536."""


# rendering: the largest frame side, and the Python default for the number of trace slots (frames per call)
RENDER_SIZES = (16, 2048)
RENDER_CAPACITY = 16


# reward profiles: the most a handle holds, and the reward-only constructor keywords a profile sets (goal.py:147-158,204-227;
# kepler.py:111-150).  Physics keywords are not profile keywords.
REWARD_PROFILES_MAX = 256
REWARD_KWARGS = {"goal": ("survival_reward_scale", "goal_vel_reward_scale", "safety_reward_scale", "goal_sparse_reward", "danger_zone"),
                 "kepler": ("numerator_C", "rad_penalty_C", "act_penalty_C")}
_PHYSICS_KWARGS = ("max_engine_force", "ship_moi", "step_size", "n_planets", "ref_orbit_a", "ref_orbit_eccentricity", "ref_orbit_angle",
                   "randomize", "ship_steering")


def render_config(family, capacity=RENDER_CAPACITY, trace_len=None, trace_decay=None, debug_lidar=None):
    """Checks set_render's keywords and returns them as the native config takes them (-1 / NaN: the family's value).
    family: "goal" or "kepler"."""
    capacity = int(capacity)
    if not 1 <= capacity <= 1 << 20:
        raise ValueError(f"capacity must be in 1 .. {1 << 20}, got {capacity}")
    trace_len = -1 if trace_len is None else int(trace_len)
    if not -1 <= trace_len <= 256:
        raise ValueError(f"trace_len must be in 0 .. 256 (None: the family's), got {trace_len}")
    trace_decay = float("nan") if trace_decay is None else float(trace_decay)
    if not (np.isnan(trace_decay) or 0.0 <= trace_decay <= 1.0):
        raise ValueError(f"trace_decay must be in [0, 1] (None: the family's), got {trace_decay}")
    debug_lidar = -1 if debug_lidar is None else int(bool(debug_lidar))
    if debug_lidar == 1 and family != "goal":
        raise ValueError("debug_lidar: the Kepler ids have no lidar")
    return dict(capacity=capacity, trace_len=trace_len, trace_decay=trace_decay, debug_lidar=debug_lidar)


def check_render_size(size):
    size = int(size)
    if not RENDER_SIZES[0] <= size <= RENDER_SIZES[1]:
        raise ValueError(f"size must be in {RENDER_SIZES[0]} .. {RENDER_SIZES[1]}, got {size}")
    return size


class ReplayRing:
    """The tensors of a replay ring (replay_torch; include/spacegym.h, sg_replay) and the host mirror of its head and fill.
    obs [T, B, D], action [T, B, 2] (int32 [T, B]), reward, done, trunc [T, B] are the rollout's own layout: hand
    ring.rows(K) to rollout_torch / step_torch(out=...), then replay_commit_torch(ring, K, ...).  term_idx, term_obs, slot_seq and
    hdr are written by the commit kernels."""
    MEMBERS = ("obs", "action", "reward", "done", "trunc", "term_idx", "term_obs", "slot_seq", "hdr")

    def __init__(self, steps, num_envs, obs_dim, term_capacity, discrete, **tensors):
        self.steps, self.num_envs, self.obs_dim, self.term_capacity, self.discrete = steps, num_envs, obs_dim, term_capacity, discrete
        for k in self.MEMBERS:
            setattr(self, k, tensors[k])
        self.head = self.filled = 0

    def __len__(self):
        """valid transitions: min(filled, T - 1) slots of the whole batch"""
        return min(self.filled, self.steps - 1) * self.num_envs

    def rows(self, n_steps):
        """views of the next n_steps slots (obs, action, reward, done, trunc), to be written by the stepping call"""
        K = int(n_steps)
        if K < 1 or self.head + K > self.steps:
            raise ValueError(f"rows: slots {self.head} .. {self.head + K - 1} cross the end of a ring of {self.steps}")
        p = self.head
        return {k: getattr(self, k)[p:p + K] for k in ("obs", "action", "reward", "done", "trunc")}


class ReplayPriority:
    """The priorities of a replay ring (replay_priority_torch; include/spacegym.h, sg_priority): leaf int32 [T, B] holds the bits of
    the uint32 fixed-point priority q of every cell (0: not samplable), node int64 the library's partial sums (opaque), hdr int32
    [16] the 64-byte header (magic, T, B, frac_bits, head, filled, max_q, sample_calls, then the uint64 total)."""
    MEMBERS = ("leaf", "node", "hdr")

    def __init__(self, steps, num_envs, frac_bits, leaf, node, hdr):
        self.steps, self.num_envs, self.frac_bits = steps, num_envs, frac_bits
        self.leaf, self.node, self.hdr = leaf, node, hdr


class Policy:
    """What policy_torch returns: the sg_policy struct (include/spacegym.h) over the caller's parameter tensors, which it keeps
    alive; n_hidden, hidden, activation and has_critic describe the nets."""

    def __init__(self, struct, tensors, has_critic):
        self.struct, self.tensors, self.has_critic = struct, tuple(tensors), bool(has_critic)
        self.n_hidden, self.hidden = int(struct.n_hidden), int(struct.hidden)
        self.activation = "relu" if struct.activation else "tanh"
        self.workspace = None  # policy_grad_torch's partial sums: a uint8 tensor, grown on demand


class QNet:
    """What q_torch returns: the sg_qnet struct (include/spacegym.h) over the caller's parameter tensors, which it keeps alive --
    critic 0's (weight, bias) pairs, then critic 1's; n_critics, n_hidden, hidden and activation describe the nets."""

    def __init__(self, struct, tensors):
        self.struct, self.tensors = struct, tuple(tensors)
        self.n_critics, self.n_hidden, self.hidden = int(struct.n_critics), int(struct.n_hidden), int(struct.hidden)
        self.activation = "relu" if struct.activation else "tanh"
        self.workspace = None  # q_grad_torch's partial sums: a uint8 tensor, grown on demand


def _ptr(t):
    """a tensor's device pointer as a ctypes argument; None stays NULL"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


class SquashedPolicy:
    """What squashed_policy_torch returns: the sg_squashed_policy struct (include/spacegym.h) over the caller's actor tensors, which
    it keeps alive; n_hidden, hidden, activation and log_std_bounds describe the net."""

    def __init__(self, struct, tensors):
        self.struct, self.tensors = struct, tuple(tensors)
        self.n_hidden, self.hidden = int(struct.n_hidden), int(struct.hidden)
        self.activation = "relu" if struct.activation else "tanh"
        self.log_std_bounds = (float(struct.log_std_min), float(struct.log_std_max))
        self.workspace = None  # squashed_grad_torch's partial sums: a uint8 tensor, grown on demand


class Dqn:
    """What dqn_torch returns: the sg_dqn struct (include/spacegym.h) over the caller's parameter tensors, which it keeps alive;
    n_hidden, hidden and activation describe the net.  A target network is a second handle."""

    def __init__(self, struct, tensors):
        self.struct, self.tensors = struct, tuple(tensors)
        self.n_hidden, self.hidden = int(struct.n_hidden), int(struct.hidden)
        self.activation = "relu" if struct.activation else "tanh"
        self.workspace = None  # dqn_grad_torch's partial sums: a uint8 tensor, grown on demand


class PolicyPopulation:
    """What policy_population_torch returns: the sg_policy struct (include/spacegym.h) over the caller's STACKED parameter tensors
    (weight [P, out, in], bias [P, out], log_std [P, 2]; its pointers address member 0), which it keeps alive; members, n_hidden,
    hidden, activation and has_critic describe the nets."""

    def __init__(self, struct, tensors, has_critic, members):
        self.struct, self.tensors, self.has_critic, self.members = struct, tuple(tensors), bool(has_critic), int(members)
        self.n_hidden, self.hidden = int(struct.n_hidden), int(struct.hidden)
        self.activation = "relu" if struct.activation else "tanh"
        self.workspace = None  # population_grad_torch's partial sums: a uint8 tensor, grown on demand


class AdamState:
    """What adam_torch returns: the optimizer state of adam_step_torch over handle.tensors, which it keeps alive through the handle.
    hyper float32 [P, 8] (env.adam_hyper_names) is read on the device at every call: write it to change a member's learning rate;
    state float64 [P, 8] (env.adam_state_names); exp_avg / exp_avg_sq: float32 tensors shaped like handle.tensors; members = P."""

    def __init__(self, handle, members, hyper, state, exp_avg, exp_avg_sq):
        self.handle, self.members, self.hyper, self.state = handle, int(members), hyper, state
        self.exp_avg, self.exp_avg_sq = tuple(exp_avg), tuple(exp_avg_sq)
        self._table = None  # (the pointers it was made from, the sg_adam_tensor array)


class PbtFitness:
    """What pbt_fitness_torch returns: the running return and length of every env's unfinished episode (env_return float64 [B],
    env_length int32 [B]), the per-member table float64 [P, 8] (env.pbt_fitness_names) over the episodes finished since a row was
    cleared, and the workspace of pbt_fitness_update_torch; members = P.  fitness is the table's column 6, a view."""

    def __init__(self, members, env_return, env_length, table, workspace):
        self.members, self.env_return, self.env_length, self.table, self.workspace = int(members), env_return, env_length, table, workspace

    @property
    def fitness(self):
        return self.table[:, 6]


# per handle class: the argument's name, the method that makes the handle, and what cannot serve a discrete id (Dqn: a continuous one)
_NET_HANDLES = {Policy: ("policy", "policy_torch", "a = mean + exp(log_std) eps"), QNet: ("q", "q_torch", "the Q critics"),
                SquashedPolicy: ("sp", "squashed_policy_torch", "the squashed Gaussian actor"), Dqn: ("dqn", "dqn_torch", "the DQN head Q(obs) -> 6"),
                PolicyPopulation: ("pop", "policy_population_torch", "a = mean + exp(log_std) eps")}


def _activation_code(activation):
    if activation not in ("tanh", "relu"):
        raise ValueError(f"activation: expected 'tanh' or 'relu', got {activation!r}")
    return 1 if activation == "relu" else 0


def _empty_pairs(like):
    """(weight, bias) gradient tensors for the parameters like = (w0, b0, w1, b1, ...)"""
    import torch
    return [(torch.empty_like(like[l]), torch.empty_like(like[l + 1])) for l in range(0, len(like), 2)]


def _flat_grads(handle, out):
    """the tensors of a *_grad_torch dict in the order of handle.tensors: None for every tensor of a net whose gradients are None or
    absent (a frozen critic, the critic behind policy_action_grad_torch); log_std last, when the dict has one"""
    if "critics" in out:
        nets = out["critics"] or [None] * handle.n_critics
    elif "net" in out:
        nets = [out["net"]]
    else:
        nets = [out["actor"]] + ([out.get("critic")] if getattr(handle, "has_critic", False) else [])
    flat = [t for pairs in nets for pair in (pairs if pairs is not None else [(None, None)] * (handle.n_hidden + 1)) for t in pair]
    return flat + ([out["log_std"]] if out.get("log_std") is not None else [])


_NET_FUNCTIONS = {}  # key -> torch.autograd.Function


def _net_function(key, forward, backward, materialize=False):
    """The torch.autograd.Function `key` behind a *_torch method, made on first use (torch is imported lazily); its inputs are
    (env, handle, obs, col, *handle.tensors), col the column beside obs (action or eps; may be None).  forward(env, handle, obs, col)
    gives the outputs.  backward(env, handle, obs, col, needs, *gs) -- needs: whether col and each tensor need a gradient; gs: the
    outputs' gradients, float32 and contiguous -- returns the gradients of (col, *handle.tensors), or None where there is nothing to
    compute.  materialize False: the g of an output the loss does not use arrives as None (a NULL g), not as zeros."""
    if key in _NET_FUNCTIONS:
        return _NET_FUNCTIONS[key]
    import torch

    def fwd(ctx, env, handle, obs, col, *params):
        ctx.env, ctx.handle, ctx.has_col = env, handle, col is not None
        ctx.save_for_backward(*((obs, col) if col is not None else (obs,)))
        if not materialize:
            ctx.set_materialize_grads(False)
        return forward(env, handle, obs, col)

    def bwd(ctx, *gs):
        col = ctx.saved_tensors[1] if ctx.has_col else None
        gs = [None if g is None else g.to(torch.float32).contiguous() for g in gs]
        grads = backward(ctx.env, ctx.handle, ctx.saved_tensors[0], col, ctx.needs_input_grad[3:], *gs)
        return (None, None, None, *(grads if grads is not None else (None,) * (1 + len(ctx.handle.tensors))))

    _NET_FUNCTIONS[key] = type(key, (torch.autograd.Function,), dict(forward=staticmethod(fwd), backward=staticmethod(bwd)))
    return _NET_FUNCTIONS[key]


def _actor_critic_backward(grad_torch, skip):
    """the backward of policy_evaluate_torch / population_evaluate_torch over env.<grad_torch>; skip: no call when no output was used
    or no parameter needs a gradient"""
    def backward(env, handle, obs, action, needs, g_logp, g_entropy, g_value=None):
        if skip and ((g_logp is None and g_entropy is None and g_value is None) or not any(needs[1:])):
            return None
        out = getattr(env, grad_torch)(handle, obs, action, g_logp, g_entropy, g_value if handle.has_critic else None)
        return (None, *_flat_grads(handle, out))
    return backward


def _q_backward(env, q, obs, action, needs, g_q1, g_q2=None):
    want_params, want_action = any(needs[1:]), needs[0]
    out = env.q_grad_torch(q, obs, action, g_q1, g_q2 if q.n_critics == 2 else None, params=want_params, action_grad=want_action)
    return (out["action"], *_flat_grads(q, out))


def _policy_action_backward(env, policy, obs, eps, needs, g_action):
    if g_action is None or not any(needs[1:]):
        return None
    return (None, *_flat_grads(policy, env.policy_action_grad_torch(policy, obs, g_action, eps)))


def _squashed_backward(env, sp, obs, eps, needs, g_action, g_logp):
    if (g_action is None and g_logp is None) or not any(needs[1:]):
        return None
    return (None, *_flat_grads(sp, env.squashed_grad_torch(sp, obs, eps, g_action, g_logp)))


def _dqn_forward(env, dqn, obs, action):
    import torch
    n = int(obs.shape[0])
    out = dict(q_all=torch.empty((n, 6), dtype=torch.float32, device=obs.device))
    if action is not None:
        out["q_taken"] = torch.empty(n, dtype=torch.float32, device=obs.device)
    q_all, q_taken = env.dqn_evaluate_raw_torch(dqn, obs, action, out=out)[:2]
    return q_all if action is None else (q_all, q_taken)


def _dqn_backward(env, dqn, obs, action, needs, g_all, g_taken=None):
    if (g_all is None and g_taken is None) or not any(needs[1:]):
        return None
    return (None, *_flat_grads(dqn, env.dqn_grad_torch(dqn, obs, action if g_taken is not None else None, g_taken, g_all)))


# The methods that take or make a net handle: served by SpaceGymVectorEnv only, refused by the multi-device front ends
NET_METHODS = ("policy_torch", "policy_act_torch", "rollout_policy_torch", "policy_evaluate_torch", "policy_evaluate_raw_torch", "policy_grad_torch",
               "ppo_grad_torch", "ppo_assign_grads", "q_torch", "q_evaluate_torch", "q_evaluate_raw_torch", "q_grad_torch", "policy_action_torch",
               "policy_action_raw_torch", "policy_action_grad_torch", "squashed_policy_torch", "squashed_act_torch", "rollout_squashed_torch",
               "squashed_sample_torch", "squashed_sample_raw_torch", "squashed_grad_torch", "dqn_torch", "dqn_act_torch", "rollout_dqn_torch",
               "dqn_evaluate_torch", "dqn_evaluate_raw_torch", "dqn_grad_torch", "policy_population_torch", "population_member_torch",
               "population_act_torch", "rollout_population_torch", "population_evaluate_torch", "population_evaluate_raw_torch",
               "population_grad_torch", "population_ppo_grad_torch", "adam_torch", "adam_step_torch", "adam_exploit_torch", "pbt_fitness_torch",
               "pbt_fitness_update_torch", "pbt_fitness_clear_torch", "pbt_select_torch", "pbt_explore_torch", "minibatch_index_torch",
               "ppo_update_torch", "dqn_td_grad_torch", "dqn_update_torch", "q_td_grad_torch",
               "q_update_torch", "q_actor_grad_torch", "q_actor_update_torch", "retrace_torch", "dqn_retrace_grad_torch")


class SpaceGymVectorEnv:
    metadata = {"render.modes": ["rgb_array"]}

    def __init__(self, env_id, num_envs, device=0, seed=0, env_index_base=0, max_episode_steps=None, auto_reset=True,
                 validate_actions=True, terminal_observation=True, copy=True, steering=None, env_kwargs=None, from_class=False,
                 episode_statistics=False, normalize_obs=False, normalize_reward=False, norm_gamma=0.99, norm_epsilon=1e-8,
                 clip_obs=None, clip_reward=None, render=False, reward_profiles=None, _handle=None):
        """steering: "velocity" (ship_steering=1, what every registered id uses) or "acceleration" (ship_steering=0, the
        constructor default of the reference classes: omega is a state, the thruster a torque); None: what env_kwargs say.
        env_kwargs: keyword arguments of the reference's constructor (GoalEnv.__init__ goal.py:18-31, KeplerEnv.__init__
        kepler.py:189-203) on top of the ones the id is registered with -- what gym.make(env_id, **env_kwargs) does; make_vec
        passes its unknown keywords here.  from_class: the id only names the family and action space, every keyword comes from
        the class defaults and env_kwargs (make_vec_from_class).
        validate_actions: step() checks on the host that the actions are in range, as the reference's step asserts
        (spaceship_env.py:71; discrete ids: ValueError, :201-202); off, out-of-range actions are clamped on the device (the
        device-tensor calls never validate: that would need a device-to-host synchronisation).
        copy=False: reset()/step() return views of the engine's pinned output buffers, overwritten by the next call
        (no per-step allocation or copy); copy=True returns fresh arrays like gym's vector envs.
        episode_statistics: switch the episode statistics on from the start (set_episode_statistics).
        normalize_obs / normalize_reward, norm_gamma, norm_epsilon, clip_obs, clip_reward: switch normalization on from the start
        (set_normalization).
        render: True or a dict of set_render's keywords (capacity, trace_len, trace_decay, debug_lidar): switch rendering on.
        reward_profiles: a list of dicts of reward keywords: switch reward profiles on from the start (set_reward_profiles)."""
        if env_id not in ENV_SPECS:
            raise ValueError(f"unknown env id {env_id!r}; served ids: {sorted(ENV_SPECS)}")
        self._lib = _native.load()
        self.env_id, self.num_envs, self.device = env_id, int(num_envs), int(device)
        self.spec = dict(ENV_SPECS[env_id])
        # the constructor's keyword arguments as the reference would see them, and the native parameter block they fill
        self.env_kwargs = constructor_kwargs(env_id, env_kwargs, from_class=from_class)
        if steering is None:
            if self.env_kwargs["ship_steering"] not in (0, 1):  # Steering.angle: no thruster does anything (dynamic_model.py:138-141,160-163)
                raise ValueError("ship_steering must be 0 (Steering.acceleration) or 1 (Steering.velocity)")
            steering = "velocity" if self.env_kwargs["ship_steering"] == 1 else "acceleration"
        self.env_kwargs["ship_steering"] = {"velocity": 1, "acceleration": 0}[steering]
        params = self._native_params(self.env_kwargs)
        if self.spec["family"] == "goal":
            self.spec["n_planets"] = int(self.env_kwargs["n_planets"])
        self.obs_dim = obs_dim(env_id, self.spec["n_planets"])
        self.n_planets = self.spec["n_planets"]
        self.single_observation_space = single_observation_space(env_id, self.n_planets)
        self.single_action_space = single_action_space(env_id)
        self.observation_space = batch_box(self.single_observation_space, self.num_envs)
        self.discrete = is_discrete(env_id)
        self.action_space = (MultiDiscrete([self.single_action_space.n] * self.num_envs) if self.discrete
                             else batch_box(self.single_action_space, self.num_envs))
        self.validate_actions = validate_actions
        self.want_terminal_obs = terminal_observation
        cfg = _native.SgConfig(env_id=env_id.encode(), num_envs=self.num_envs, seed=int(seed),
                               env_index_base=int(env_index_base), max_episode_steps=int(max_episode_steps or 0),
                               auto_reset=int(bool(auto_reset)), steering={"velocity": 0, "acceleration": 1}[steering])
        self._cfg, self._params = cfg, params
        if _handle is None:
            h = C.c_void_p()
            rc = self._lib.sg_create_ex(C.byref(cfg), C.byref(params), self.device, C.byref(h))
            _native.check(self._lib, None, rc, "sg_create_ex")
        else:  # a handle made by sg_create_sharded_ex (MultiDeviceVectorEnv): `num_envs`, `device`, `env_index_base` describe it
            h = _handle
        self._h = h
        assert self._lib.sg_obs_dim(h) == self.obs_dim
        B, D = self.num_envs, self.obs_dim
        self.copy = bool(copy)
        self._pinned = []
        self._obs = self._host_array((B, D), np.float32)  # reset()'s observations (a step's outputs sit in the handle's blocks)
        self._act = self._host_array((B,) if self.discrete else (B, 2), np.int32 if self.discrete else np.float32)
        self._pending = False
        self._blocks = {}
        self._torch_bufs = None
        self._episode_stats = False
        self._render_on = False
        self._have_act = False  # a step() has filled the pinned action buffer: render() shows that action
        self._last_obs = None  # the observations the last reset() / step() returned (reset(mask=...) keeps their other rows)
        if render:
            self.set_render(True, **(render if isinstance(render, dict) else {}))
        if episode_statistics:
            self.set_episode_statistics(True)
        if normalize_obs or normalize_reward:
            self.set_normalization(obs=normalize_obs, reward=normalize_reward, gamma=norm_gamma, epsilon=norm_epsilon,
                                   clip_obs=clip_obs, clip_reward=clip_reward)
        if reward_profiles is not None:
            self.set_reward_profiles(reward_profiles)

    def _native_params(self, kw):
        """sg_params (include/spacegym.h) from the constructor's keyword arguments"""
        p = _native.SgParams()
        self._lib.sg_params_init(C.byref(p))
        names = (("goal_vel_reward_scale", "safety_reward_scale", "goal_sparse_reward", "survival_reward_scale", "danger_zone")
                 if self.spec["family"] == "goal" else
                 ("ref_orbit_a", "ref_orbit_eccentricity", "ref_orbit_angle", "numerator_C", "rad_penalty_C", "act_penalty_C", "step_size"))
        for k in names + ("ship_moi", "max_engine_force"):
            setattr(p, k, float(kw[k]))
        if self.spec["family"] == "goal":
            p.n_planets = int(kw["n_planets"])
        else:
            p.randomize = int(bool(kw["randomize"]))
        return p

    def native_params(self):
        """the parameters the handle was built with (sg_get_params), as a dict of the reference's keyword names"""
        p = _native.SgParams()
        self._ck(self._lib.sg_get_params(self._h, C.byref(p)), "sg_get_params")
        out = {k: getattr(p, k) for k, _ in p._fields_ if k not in ("struct_size", "reserved")}
        return {k: v for k, v in out.items() if not (isinstance(v, float) and np.isnan(v)) and v != -1}

    def _host_array(self, shape, dtype):
        """NumPy array over page-locked memory (sg_host_alloc); ordinary memory if pinning fails."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self._lib.sg_host_alloc(n)
        if not ptr:
            return np.empty(shape, dtype)
        self._pinned.append(ptr)
        return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self._lib.sg_destroy(self._h)
            self._h = None
            self._obs = self._act = None
            self._blocks = {}
            for ptr in self._pinned:
                self._lib.sg_host_free(ptr)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        _native.check(self._lib, self._h, rc, what)

    def seed(self, seed=None):
        """SpaceshipEnv.seed (spaceship_env.py:92-94): returns [seed]; applies from the next reset()."""
        seed = int(np.random.SeedSequence().entropy % (1 << 63)) if seed is None else int(seed)
        self._ck(self._lib.sg_seed(self._h, seed), "sg_seed")
        return [seed]

    def set_counters(self, on=True):
        """per-batch event counters (sg_set_counters): env-steps, finished episodes, truncations, goals reached; off by default"""
        self._ck(self._lib.sg_set_counters(self._h, int(bool(on))), "sg_set_counters")

    def counters(self, reset=False):
        k = _native.SgCounters()
        self._ck(self._lib.sg_get_counters(self._h, C.byref(k), int(bool(reset))), "sg_get_counters")
        return {f: int(getattr(k, f)) for f, _ in k._fields_}

    def set_episode_statistics(self, on=True):
        """gym.wrappers.RecordEpisodeStatistics on the device (sg_set_episode_stats): per env the float64 sum of the rewards and
        the number of steps since the episode began, both reset by done.  Switching (on or off) zeroes them; off by default."""
        if self._pending:
            raise RuntimeError("set_episode_statistics() while a step is in flight (step_wait() first)")
        self._ck(self._lib.sg_set_episode_stats(self._h, int(bool(on))), "sg_set_episode_stats")
        self._episode_stats = bool(on)
        self._blocks = {}  # the result blocks are made again with (or without) the two rows

    @property
    def episode_statistics(self):
        return self._episode_stats

    def _need_episode_stats(self, what):
        if not self._episode_stats:
            raise ValueError(f"{what}: episode statistics are off (make_vec(..., episode_statistics=True) or set_episode_statistics())")

    def normalization(self):
        """the normalization configuration (sg_get_normalize) as a dict: obs, reward, update (bool), gamma, epsilon, clip_obs,
        clip_reward (None: no clipping)"""
        n = _native.SgNormalize()
        self._ck(self._lib.sg_get_normalize(self._h, C.byref(n)), "sg_get_normalize")
        clip = lambda v: None if v == float("inf") else v  # noqa: E731
        return dict(obs=bool(n.obs), reward=bool(n.reward), update=bool(n.update), gamma=n.gamma, epsilon=n.epsilon,
                    clip_obs=clip(n.clip_obs), clip_reward=clip(n.clip_reward))

    def set_normalization(self, obs=None, reward=None, update=None, gamma=None, epsilon=None, clip_obs=_KEEP, clip_reward=_KEEP):
        """gym.wrappers.NormalizeObservation (obs) and NormalizeReward (reward) on the device (sg_set_normalize): running float64
        mean and variance of the observations and of the discounted return, updated by every step and (observations) reset.
        Arguments left out keep their value; clip_obs / clip_reward None: no clipping.  update=False freezes the statistics
        (evaluation).  Switching on from off starts the statistics afresh, switching both off frees them."""
        if self._pending:
            raise RuntimeError("set_normalization() while a step is in flight (step_wait() first)")
        cur = self.normalization()
        new = dict(obs=cur["obs"] if obs is None else bool(obs), reward=cur["reward"] if reward is None else bool(reward),
                   update=cur["update"] if update is None else bool(update), gamma=cur["gamma"] if gamma is None else float(gamma),
                   epsilon=cur["epsilon"] if epsilon is None else float(epsilon),
                   clip_obs=cur["clip_obs"] if clip_obs is _KEEP else clip_obs,
                   clip_reward=cur["clip_reward"] if clip_reward is _KEEP else clip_reward)
        if not 0.0 <= new["gamma"] <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {new['gamma']}")
        if not 0.0 <= new["epsilon"] < float("inf"):
            raise ValueError(f"epsilon must be finite and >= 0, got {new['epsilon']}")
        for k in ("clip_obs", "clip_reward"):
            if new[k] is not None and not float(new[k]) > 0.0:
                raise ValueError(f"{k} must be > 0 or None, got {new[k]}")
        n = _native.SgNormalize()
        self._lib.sg_normalize_init(C.byref(n))
        n.obs, n.reward, n.update = int(new["obs"]), int(new["reward"]), int(new["update"])
        n.gamma, n.epsilon = new["gamma"], new["epsilon"]
        n.clip_obs = float("inf") if new["clip_obs"] is None else float(new["clip_obs"])
        n.clip_reward = float("inf") if new["clip_reward"] is None else float(new["clip_reward"])
        self._ck(self._lib.sg_set_normalize(self._h, C.byref(n)), "sg_set_normalize")

    _NORM_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns")

    def _norm_shapes(self):
        return dict(obs_mean=(self.obs_dim,), obs_var=(self.obs_dim,), obs_count=(), ret_mean=(), ret_var=(), ret_count=(),
                    returns=(self.num_envs,))

    def normalizer_state(self):
        """the running statistics (sg_get_normalize_state) as float64 NumPy arrays: obs_mean, obs_var [D], obs_count, ret_mean,
        ret_var, ret_count (0-d) and returns [B]; waits for the enqueued work"""
        out = {k: np.zeros(s, np.float64) for k, s in self._norm_shapes().items()}
        self._ck(self._lib.sg_get_normalize_state(self._h, *[self._ptr(out[k]) for k in self._NORM_KEYS]), "sg_get_normalize_state")
        return out

    def set_normalizer_state(self, state):
        """puts statistics (a normalizer_state() dict; missing keys keep their value) into this env, e.g. a trained policy's
        into an evaluation env"""
        args = []
        for k, shape in self._norm_shapes().items():
            if k in state and state[k] is not None:
                a = np.array(state[k], np.float64, order="C")  # (ascontiguousarray would make a 0-d value 1-d)
                if a.shape != shape:
                    raise ValueError(f"{k}: expected shape {shape}, got {a.shape}")
                args.append(a)
            else:
                args.append(None)
        self._ck(self._lib.sg_set_normalize_state(self._h, *[self._ptr(a) for a in args]), "sg_set_normalize_state")

    # ------------------------------------------------------------------ reward profiles
    def set_reward_profiles(self, profiles):
        """Different reward coefficients for different envs of the batch (sg_set_reward_profiles).  profiles: a list of at most
        256 dicts of the reference's reward-only constructor keywords -- Goal ids survival_reward_scale, goal_vel_reward_scale,
        safety_reward_scale, goal_sparse_reward, danger_zone; Kepler ids numerator_C, rad_penalty_C, act_penalty_C; a keyword
        left out keeps the env's own value.  Env i under profile p gives bit for bit what env i of make_vec(..., **p) gives.
        Every env starts at profile 0 (set_env_profiles chooses); the indices are kept while profiles stay on.  None or []:
        off."""
        if self._pending:
            raise RuntimeError("set_reward_profiles() while a step is in flight (step_wait() first)")
        profiles = [] if profiles is None else list(profiles)
        if len(profiles) > REWARD_PROFILES_MAX:
            raise ValueError(f"reward profiles: at most {REWARD_PROFILES_MAX}, got {len(profiles)}")
        arr = (_native.SgRewardProfile * max(1, len(profiles)))()
        for k, prof in enumerate(profiles):
            if not isinstance(prof, dict):
                raise TypeError(f"reward profile {k}: a dict of reward keywords, got {type(prof).__name__}")
            self._lib.sg_reward_profile_init(C.byref(arr[k]))
            for name, v in prof.items():
                if name not in REWARD_KWARGS["goal"] + REWARD_KWARGS["kepler"]:
                    what = "a physics keyword: reward profiles set reward keywords only" if name in _PHYSICS_KWARGS else "unknown keyword"
                    raise ValueError(f"reward profile {k}: {name!r}: {what} ({', '.join(REWARD_KWARGS[self.spec['family']])})")
                if v is None:
                    continue
                setattr(arr[k], name, float(v))  # (the other family's keywords are refused by the library, as sg_create_ex does)
        self._ck(self._lib.sg_set_reward_profiles(self._h, len(profiles), arr if profiles else None), "sg_set_reward_profiles")

    def reward_profiles(self):
        """the effective profiles (sg_get_reward_profiles): a list of dicts of the family's reward keywords; [] while off"""
        n = C.c_int32()
        self._ck(self._lib.sg_get_reward_profiles(self._h, C.byref(n), None, 0), "sg_get_reward_profiles")
        if not n.value:
            return []
        arr = (_native.SgRewardProfile * n.value)()
        self._ck(self._lib.sg_get_reward_profiles(self._h, C.byref(n), arr, n.value), "sg_get_reward_profiles")
        return [{k: getattr(p, k) for k in REWARD_KWARGS[self.spec["family"]]} for p in arr]

    def set_env_profiles(self, idx):
        """Each env's reward profile, from the next env-step's reward on (also in mid-episode; a curriculum that changes profiles
        at episode boundaries only selects on the device: torch.where(done, new, idx)).  idx: integers of shape [num_envs] (NumPy
        or any array-like; refused if one is past the table), or a uint8 CUDA tensor on the env's device -- then one kernel on
        torch's current stream copies it, with no host synchronisation (graph-capturable); an index past the table makes that
        env use profile 0 and is reported by check_status()."""
        try:
            import torch
        except ImportError:
            torch = None
        if torch is not None and isinstance(idx, torch.Tensor) and idx.is_cuda:
            self._check_tensor("idx", idx, torch.uint8, (self.num_envs,))
            self._ck(self._lib.sg_set_env_profiles_device(self._h, C.c_void_p(idx.data_ptr()), self._stream()),
                     "sg_set_env_profiles_device")
            return
        a = np.asarray(idx.cpu() if torch is not None and isinstance(idx, torch.Tensor) else idx)
        if a.shape != (self.num_envs,):
            raise ValueError(f"idx: expected shape ({self.num_envs},), got {a.shape}")
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"idx: expected integers, got {a.dtype}")
        n = len(self.reward_profiles())
        if not n:
            raise ValueError("set_env_profiles: reward profiles are off (set_reward_profiles first)")
        if a.size and (a.min() < 0 or a.max() >= n):
            raise ValueError(f"idx: profile indices must be in [0, {n}), got [{a.min()}, {a.max()}]")
        a = np.ascontiguousarray(a, np.uint8)
        self._ck(self._lib.sg_set_env_profiles(self._h, self._ptr(a)), "sg_set_env_profiles")

    def env_profiles(self):
        """each env's reward profile index, uint8 [num_envs] (waits for the enqueued work)"""
        out = np.empty(self.num_envs, np.uint8)
        self._ck(self._lib.sg_get_env_profiles(self._h, self._ptr(out)), "sg_get_env_profiles")
        return out

    # ------------------------------------------------------------------ rendering
    def set_render(self, on=True, capacity=RENDER_CAPACITY, trace_len=None, trace_decay=None, debug_lidar=None):
        """render(mode="rgb_array") on the device (sg_set_render).  capacity: trace slots, the most frames per call; trace_len
        (num_prev_pos_vis), trace_decay (prev_pos_color_decay), debug_lidar: None keeps the family's (Goal 30, 0.85, lidar
        lines; Kepler 75, 0.95, none: rendering.py:21-22, goal.py:71, kepler.py:222).  Switching on (again) empties every trace
        slot; off frees them."""
        if self._pending:
            raise RuntimeError("set_render() while a step is in flight (step_wait() first)")
        if not on:
            self._ck(self._lib.sg_set_render(self._h, None), "sg_set_render")
            self._render_on = False
            return
        v = render_config(self.spec["family"], capacity, trace_len, trace_decay, debug_lidar)
        cfg = _native.SgRenderConfig()
        self._lib.sg_render_config_init(C.byref(cfg))
        for k, x in v.items():
            setattr(cfg, k, x)
        self._ck(self._lib.sg_set_render(self._h, C.byref(cfg)), "sg_set_render")
        self._render_on = True
        self._render_capacity = v["capacity"]

    def _need_render(self, env_ids, what):
        if not self._render_on:
            raise ValueError(f"{what}: rendering is off (make_vec(..., render=True) or set_render())")
        if len(env_ids) > self._render_capacity:
            raise ValueError(f"{what}: {len(env_ids)} frames, capacity {self._render_capacity} (set_render(capacity=...))")

    def render(self, mode="rgb_array", env_ids=(0,), size=600):
        """SpaceshipEnv.render(mode="rgb_array") (spaceship_env.py:80-90) of the envs `env_ids`: uint8 [n, size, size, 3], row 0
        the top.  The exhaust and the torque indicator show the actions of the last step() (none before the first).  Every
        call appends the envs' positions to their traces.  mode="human" (a window) is not served."""
        if mode == "human":
            raise NotImplementedError('render(mode="human") opens a window: not served, use mode="rgb_array"')
        if mode != "rgb_array":
            raise ValueError(f"unknown render mode {mode!r}; served: {self.metadata['render.modes']}")
        size = check_render_size(size)
        ids = np.ascontiguousarray(np.atleast_1d(np.asarray(env_ids)), dtype=np.int32)
        if ids.ndim != 1:
            raise ValueError("env_ids must be a sequence of env indices")
        if np.any(ids < 0) or np.any(ids >= self.num_envs):
            raise ValueError(f"env_ids must be in 0 .. {self.num_envs - 1}")
        if self._pending:
            raise RuntimeError("render() while a step is in flight (step_wait() first)")
        self._need_render(ids, "render")
        out = np.empty((len(ids), size, size, 3), np.uint8)
        act = self._act if self._have_act else None
        self._ck(self._lib.sg_render(self._h, len(ids), self._ptr(ids), self._ptr(act), size, self._ptr(out)), "sg_render")
        return out

    def render_torch(self, env_ids, actions=None, size=600, out=None):
        """render() on torch's current stream, without synchronisation (sg_render_device): env_ids an int32 device tensor (or a
        sequence, copied to the device), actions the step's layout for the whole batch ([B, 2] float32 / [B] int32) or None,
        out a uint8 device tensor [n, size, size, 3] (allocated if None).  With tensors passed in, the call allocates nothing and
        can be captured into a graph.  An id outside the batch gives a white frame and an error from check_status()."""
        import torch
        size = check_render_size(size)
        dev = torch.device("cuda", self.device)
        if not isinstance(env_ids, torch.Tensor):
            env_ids = torch.as_tensor(np.atleast_1d(np.asarray(env_ids, np.int32)), device=dev)
        self._check_tensor("env_ids", env_ids, torch.int32, (env_ids.shape[0],) if env_ids.dim() == 1 else (-1,))
        n = env_ids.shape[0]
        self._need_render(range(n), "render_torch")
        if actions is not None:
            self._check_tensor("actions", actions, torch.int32 if self.discrete else torch.float32,
                               (self.num_envs,) if self.discrete else (self.num_envs, 2))
        if out is None:
            out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev)
        self._check_tensor("out", out, torch.uint8, (n, size, size, 3))
        self._ck(self._lib.sg_render_device(self._h, n, C.c_void_p(env_ids.data_ptr()),
                                            C.c_void_p(actions.data_ptr()) if actions is not None else None, size,
                                            C.c_void_p(out.data_ptr()), self._stream()), "sg_render_device")
        return out

    def set_auto_reset(self, on):
        self._ck(self._lib.sg_set_auto_reset(self._h, int(bool(on))), "sg_set_auto_reset")
        self._cfg.auto_reset = int(bool(on))

    # ------------------------------------------------------------------ NumPy path
    @staticmethod
    def _ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def reset(self, mask=None):
        """First observations of every env; with `mask` (bool or uint8 [num_envs]) only the envs whose entry is set are reset
        (sg_reset_masked: what auto-reset would start next for each of them, the rest is left alone -- for a loop with
        auto_reset off, gymnasium's reset(options={"reset_mask": mask})).  Returns the handle's host observation buffer (a copy
        unless copy=False) with the masked rows replaced; its other rows are what the last reset() / step() returned."""
        if mask is None:
            self._ck(self._lib.sg_reset(self._h, self._ptr(self._obs)), "sg_reset")
        else:
            m = self._mask_host(mask)
            if self._last_obs is not None and self._last_obs is not self._obs:
                np.copyto(self._obs, self._last_obs)
            self._ck(self._lib.sg_reset_masked(self._h, self._ptr(m), self._ptr(self._obs)), "sg_reset_masked")
        self._last_obs = self._obs
        return self._obs.copy() if self.copy else self._obs

    def _mask_host(self, mask):
        """reset(mask=...): a bool or uint8 array of shape [num_envs], as contiguous uint8"""
        mask = np.asarray(mask)
        if mask.dtype not in (np.bool_, np.uint8) or mask.shape != (self.num_envs,):
            raise ValueError(f"mask: expected bool or uint8 of shape ({self.num_envs},), got {mask.dtype} {mask.shape}")
        return np.ascontiguousarray(mask).view(np.uint8)

    def _check_actions(self, actions):
        if self.discrete:  # int index per env, spaceship_env.py:189-202
            actions = np.ascontiguousarray(actions, dtype=np.int32)
            if actions.shape != (self.num_envs,):
                raise ValueError(f"actions must have shape ({self.num_envs},), got {actions.shape}")
            if self.validate_actions and not (np.all(actions >= 0) and np.all(actions <= 5)):
                raise ValueError("discrete action out of range")  # the reference raises ValueError, spaceship_env.py:201-202
            return actions
        actions = np.ascontiguousarray(actions, dtype=np.float32)  # raw_action.astype(np.float32), spaceship_env.py:69-70
        if actions.shape != (self.num_envs, 2):
            raise ValueError(f"actions must have shape ({self.num_envs}, 2), got {actions.shape}")
        if self.validate_actions:  # assert self.action_space.contains(raw_action), spaceship_env.py:71
            assert np.all(actions >= -1.0) and np.all(actions <= 1.0), actions
        return actions

    def step_async(self, actions):
        """gym.vector's step_async: the step kernel is enqueued on the engine's stream -- it reads the actions from the pinned
        action buffer and stores its outputs into one of the handle's two page-locked result blocks itself -- and the call
        returns; step_wait() collects."""
        if self._pending:
            raise RuntimeError("step_async() while a step is in flight (step_wait() first)")
        np.copyto(self._act, self._check_actions(actions))  # into the pinned action buffer (unchanged until step_wait)
        self._have_act = True
        self._ck(self._lib.sg_step_begin(self._h, self._ptr(self._act), int(self.want_terminal_obs)), "sg_step_begin")
        self._pending = True

    def _block_views(self, ptrs):
        """NumPy views of one of the handle's two result blocks (made once per block)"""
        key = ptrs[0]
        if key not in self._blocks:
            B, D = self.num_envs, self.obs_dim

            def view(ptr, shape, dtype):
                n = int(np.prod(shape)) * np.dtype(dtype).itemsize
                return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)
            self._blocks[key] = (view(ptrs[0], (B, D), np.float32), view(ptrs[1], (B,), np.float32), view(ptrs[2], (B,), np.uint8),
                                 view(ptrs[3], (B,), np.uint8), view(ptrs[4], (B, D), np.float32) if ptrs[4] else None)
        return self._blocks[key]

    def _episode_views(self):
        """NumPy views of the episode rows of the block sg_step_end returned last (sg_step_end_episodes)"""
        r, l = C.c_void_p(), C.c_void_p()
        self._ck(self._lib.sg_step_end_episodes(self._h, C.byref(r), C.byref(l)), "sg_step_end_episodes")
        key = ("episode", r.value)
        if key not in self._blocks:
            B = self.num_envs
            self._blocks[key] = (np.frombuffer((C.c_char * (8 * B)).from_address(r.value), dtype=np.float64),
                                 np.frombuffer((C.c_char * (4 * B)).from_address(l.value), dtype=np.int32))
        return self._blocks[key]

    def step_wait(self):
        if not self._pending:
            raise RuntimeError("step_wait() without step_async()")
        p = [C.c_void_p() for _ in range(5)]
        rc = self._lib.sg_step_end(self._h, *[C.byref(x) for x in p])
        self._pending = False  # (the native side has given the step up as well if the wait failed)
        self._ck(rc, "sg_step_end")
        obs, rew, done, trunc, tobs = self._block_views([x.value for x in p])
        self._last_obs = obs
        info = StepInfo({"TimeLimit.truncated": trunc.view(np.bool_) if not self.copy else trunc.astype(bool)})
        if tobs is not None:
            info["terminal_observation"] = tobs.copy() if self.copy else tobs
        if self._episode_stats:
            r, l = self._episode_views()
            info["episode"] = {"r": r.copy(), "l": l.copy()} if self.copy else {"r": r, "l": l}
            info["_episode"] = done.astype(bool) if self.copy else done.view(np.bool_)
        if self.copy:
            return obs.copy(), rew.copy(), done.astype(bool), info
        return obs, rew, done.view(np.bool_), info

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # ------------------------------------------------------------------ state access (golden-vector injection, checkpoints)
    def get_state(self):
        B, N = self.num_envs, self.n_planets
        ship = np.empty((B, 6), np.float32)
        planets = np.empty((B, N, 2), np.float32) if N else None
        goal = np.empty((B, 2), np.float32)
        elapsed = np.empty(B, np.int32)
        self._ck(self._lib.sg_get_state(self._h, self._ptr(ship), self._ptr(planets), self._ptr(goal), self._ptr(elapsed)),
                 "sg_get_state")
        return dict(ship=ship, planets=planets, goal=goal, elapsed=elapsed)

    def set_state(self, ship=None, planets=None, goal=None, elapsed=None):
        B, N = self.num_envs, self.n_planets

        def prep(a, shape, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != shape:
                raise ValueError(f"expected shape {shape}, got {a.shape}")
            return a
        ship, goal = prep(ship, (B, 6), np.float32), prep(goal, (B, 2), np.float32)
        planets, elapsed = prep(planets, (B, N, 2), np.float32), prep(elapsed, (B,), np.int32)
        self._ck(self._lib.sg_set_state(self._h, self._ptr(ship), self._ptr(planets), self._ptr(goal), self._ptr(elapsed)),
                 "sg_set_state")

    def vector_field(self, actions, ship=None):
        """SpaceshipEnv.vector_field (spaceship_env.py:96-100) for every env: float32 [B, 6] = (vx, vy, omega, ax, ay, alpha),
        at the current state or at the given `ship` states [B, 6] (planets as they are now)."""
        a = self._check_actions(actions)
        ship = None if ship is None else np.ascontiguousarray(ship, np.float32)
        out = np.empty((self.num_envs, 6), np.float32)
        self._ck(self._lib.sg_vector_field(self._h, self._ptr(a), self._ptr(ship), self._ptr(out)), "sg_vector_field")
        return out

    # ------------------------------------------------------------------ torch path (device tensors, current stream)
    def _torch(self):
        import torch
        if self._torch_bufs is None:
            dev = torch.device("cuda", self.device)
            B, D = self.num_envs, self.obs_dim
            self._torch_bufs = dict(
                obs=torch.empty((B, D), dtype=torch.float32, device=dev), reward=torch.empty(B, dtype=torch.float32, device=dev),
                done=torch.empty(B, dtype=torch.uint8, device=dev), trunc=torch.empty(B, dtype=torch.uint8, device=dev))
        return torch, self._torch_bufs

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset_torch(self, out=None, mask=None):
        """First observations of every env into `out` (default: the env's own obs tensor, the one step_torch writes by default).
        mask: bool or uint8 CUDA tensor [num_envs] on the env's device -- only the envs whose entry is set are reset
        (sg_reset_masked_device, no host synchronisation, graph-capturable) and only their rows of `out` are written: pass the
        tensor step_torch filled and it holds the whole batch's observations afterwards."""
        torch, bufs = self._torch()
        obs = bufs["obs"] if out is None else out
        if out is not None:
            self._check_tensor("out", out, torch.float32, (self.num_envs, self.obs_dim))
        if mask is None:
            self._ck(self._lib.sg_reset_device(self._h, C.c_void_p(obs.data_ptr()), self._stream()), "sg_reset_device")
            return obs
        if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)  # (same bytes: no copy)
        self._check_tensor("mask", mask, torch.uint8, (self.num_envs,))
        self._ck(self._lib.sg_reset_masked_device(self._h, C.c_void_p(mask.data_ptr()), C.c_void_p(obs.data_ptr()), self._stream()),
                 "sg_reset_masked_device")
        return obs

    def step_torch(self, actions, out=None, terminal_obs=None, episodes=None):
        """actions: float32 CUDA tensor [B, 2] (discrete ids: int32 [B]), or any device array exporting DLPack
        (`__dlpack__`: CuPy, JAX, ...; taken zero-copy).  Returns (obs, reward, done, truncated) device tensors, which are
        reused by the next call unless `out` (a dict with the same keys) is given; `torch.utils.dlpack.to_dlpack` /
        `__dlpack__` hands them on to other frameworks without a copy.
        episodes: dict(r=float64 [B], l=int32 [B]) of device tensors (episode statistics on): rows of envs that finished in
        this step receive the return and length of the episode that ended, other rows are left untouched."""
        torch, bufs = self._torch()
        o = bufs if out is None else out
        if not isinstance(actions, torch.Tensor) and hasattr(actions, "__dlpack__"):
            actions = torch.from_dlpack(actions)
        B, D = self.num_envs, self.obs_dim
        self._check_tensor("actions", actions, torch.int32 if self.discrete else torch.float32, (B,) if self.discrete else (B, 2))
        if out is not None:
            self._check_tensor("out['obs']", o["obs"], torch.float32, (B, D))
            self._check_tensor("out['reward']", o["reward"], torch.float32, (B,))
            self._check_tensor("out['done']", o["done"], torch.uint8, (B,))
            self._check_tensor("out['trunc']", o["trunc"], torch.uint8, (B,))
        if terminal_obs is not None:
            self._check_tensor("terminal_obs", terminal_obs, torch.float32, (B, D))
        args = (self._h, C.c_void_p(actions.data_ptr()), C.c_void_p(o["obs"].data_ptr()), C.c_void_p(o["reward"].data_ptr()),
                C.c_void_p(o["done"].data_ptr()), C.c_void_p(o["trunc"].data_ptr()),
                C.c_void_p(terminal_obs.data_ptr()) if terminal_obs is not None else None)
        if episodes is None:
            self._ck(self._lib.sg_step_device(*args, self._stream()), "sg_step_device")
        else:
            self._need_episode_stats("step_torch(episodes=...)")
            self._check_tensor("episodes['r']", episodes["r"], torch.float64, (B,))
            self._check_tensor("episodes['l']", episodes["l"], torch.int32, (B,))
            self._ck(self._lib.sg_step_device_episodes(*args, C.c_void_p(episodes["r"].data_ptr()), C.c_void_p(episodes["l"].data_ptr()),
                                                       self._stream()), "sg_step_device_episodes")
        return o["obs"], o["reward"], o["done"], o["trunc"]

    def _check_tensor(self, name, t, dtype, shape):
        """a raw pointer goes to the kernel: refuse anything whose memory is not what the kernel will write / read"""
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device):
            raise ValueError(f"{name}: expected a CUDA tensor on device {self.device}")
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}"
                             f"{'' if t.is_contiguous() else ' (not contiguous)'}")

    def rollout_torch(self, actions, obs, reward, done, trunc, terminal=None, episodes=None):
        """actions [K, B, 2] (discrete ids: int32 [K, B]) -> obs [K, B, D], reward/done/trunc [K, B]: K steps, one launch.
        terminal: optional dict(count=uint32/int32 [1], step_env=int32 [cap, 2], obs=float32 [cap, D]) of device tensors
        that receives one record per finished env-step: its (step, env) and the LAST observation of the episode that ended
        there (sg_rollout_device_terminal); `terminal_records` turns it into sorted host arrays.
        episodes: optional list from episode_list_torch (episode statistics on) that receives one record per finished episode:
        (step, env), return, length, truncated (sg_rollout_device_episodes); `episode_records` sorts it."""
        import torch
        K, B, D = int(actions.shape[0]), self.num_envs, self.obs_dim
        self._check_tensor("actions", actions, torch.int32 if self.discrete else torch.float32, (K, B) if self.discrete else (K, B, 2))
        self._check_tensor("obs", obs, torch.float32, (K, B, D))
        self._check_tensor("reward", reward, torch.float32, (K, B))
        self._check_tensor("done", done, torch.uint8, (K, B))
        self._check_tensor("trunc", trunc, torch.uint8, (K, B))
        args = (self._h, K, C.c_void_p(actions.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(reward.data_ptr()),
                C.c_void_p(done.data_ptr()), C.c_void_p(trunc.data_ptr()))
        el = self._episode_list_arg(episodes) if episodes is not None else None
        tl = None
        if terminal is not None:
            cap = int(terminal["step_env"].shape[0])
            if terminal["count"].dtype not in (torch.int32, torch.uint32) or terminal["count"].numel() != 1:
                raise ValueError("terminal['count']: expected one 32-bit integer")
            self._check_tensor("terminal['step_env']", terminal["step_env"], torch.int32, (cap, 2))
            self._check_tensor("terminal['obs']", terminal["obs"], torch.float32, (cap, D))
            tl = _native.SgTerminalList(terminal["count"].data_ptr(), terminal["step_env"].data_ptr(), terminal["obs"].data_ptr(), cap)
        if el is not None:
            self._ck(self._lib.sg_rollout_device_episodes(*args, C.byref(tl) if tl is not None else None, C.byref(el), self._stream()),
                     "sg_rollout_device_episodes")
        elif tl is None:
            self._ck(self._lib.sg_rollout_device(*args, self._stream()), "sg_rollout_device")
        else:
            self._ck(self._lib.sg_rollout_device_terminal(*args, C.byref(tl), self._stream()), "sg_rollout_device_terminal")
        return obs, reward, done, trunc

    def _episode_list_arg(self, episodes):
        """SgEpisodeList over the tensors of an episode_list_torch() dict, checked"""
        import torch
        self._need_episode_stats("episodes=")
        cap = int(episodes["step_env"].shape[0])
        if episodes["count"].dtype not in (torch.int32, torch.uint32) or episodes["count"].numel() != 1:
            raise ValueError("episodes['count']: expected one 32-bit integer")
        self._check_tensor("episodes['count']", episodes["count"], episodes["count"].dtype, (1,))
        self._check_tensor("episodes['step_env']", episodes["step_env"], torch.int32, (cap, 2))
        self._check_tensor("episodes['r']", episodes["r"], torch.float64, (cap,))
        self._check_tensor("episodes['l']", episodes["l"], torch.int32, (cap,))
        self._check_tensor("episodes['truncated']", episodes["truncated"], torch.uint8, (cap,))
        return _native.SgEpisodeList(episodes["count"].data_ptr(), episodes["step_env"].data_ptr(), episodes["r"].data_ptr(),
                                     episodes["l"].data_ptr(), episodes["truncated"].data_ptr(), cap)

    def prepare_rollout(self, actions, obs, reward, done, trunc, episodes=None):
        """Validates the buffers once and returns a zero-argument callable that enqueues the rollout on torch's current
        stream: for loops that re-use the same buffers (the per-call checks of rollout_torch cost more host time than a
        short rollout takes on the GPU).  episodes: as rollout_torch's."""
        import torch
        K, B, D = int(actions.shape[0]), self.num_envs, self.obs_dim
        self._check_tensor("actions", actions, torch.int32 if self.discrete else torch.float32, (K, B) if self.discrete else (K, B, 2))
        self._check_tensor("obs", obs, torch.float32, (K, B, D))
        self._check_tensor("reward", reward, torch.float32, (K, B))
        self._check_tensor("done", done, torch.uint8, (K, B))
        self._check_tensor("trunc", trunc, torch.uint8, (K, B))
        el = self._episode_list_arg(episodes) if episodes is not None else None
        # (normalization on: its scratch for K steps is made now, so that the callable can be captured into a graph)
        self._ck(self._lib.sg_normalize_reserve(self._h, K), "sg_normalize_reserve")
        keep = (actions, obs, reward, done, trunc)  # the callable keeps the tensors alive
        args = (self._h, K) + tuple(C.c_void_p(t.data_ptr()) for t in keep)
        fn, what, ck, dev = self._lib.sg_rollout_device, "sg_rollout_device", self._ck, self.device
        if el is not None:
            fn, what = self._lib.sg_rollout_device_episodes, "sg_rollout_device_episodes"
            args += (None, C.byref(el))
            keep += (episodes, el)
        cur = torch.cuda.current_stream

        def call():
            ck(fn(*args, C.c_void_p(cur(dev).cuda_stream)), what)
        call.keep = keep
        return call

    def terminal_list_torch(self, capacity):
        """device buffers for rollout_torch(..., terminal=...)"""
        import torch
        dev = torch.device("cuda", self.device)
        return dict(count=torch.zeros(1, dtype=torch.int32, device=dev), step_env=torch.empty((capacity, 2), dtype=torch.int32, device=dev),
                    obs=torch.empty((capacity, self.obs_dim), dtype=torch.float32, device=dev))

    def episode_list_torch(self, capacity):
        """device buffers for rollout_torch(..., episodes=...): count, step_env [cap, 2], r float64 [cap], l int32 [cap],
        truncated uint8 [cap]"""
        import torch
        dev = torch.device("cuda", self.device)
        return dict(count=torch.zeros(1, dtype=torch.int32, device=dev), step_env=torch.empty((capacity, 2), dtype=torch.int32, device=dev),
                    r=torch.empty(capacity, dtype=torch.float64, device=dev), l=torch.empty(capacity, dtype=torch.int32, device=dev),
                    truncated=torch.empty(capacity, dtype=torch.uint8, device=dev))

    @staticmethod
    def episode_records(episodes):
        """dict(step, env int32 [n], r float64 [n], l int32 [n], truncated bool [n]) sorted by (step, env); raises if the
        list overflowed"""
        n = int(episodes["count"].item())
        cap = int(episodes["step_env"].shape[0])
        if n > cap:
            raise OverflowError(f"episode list overflow: {n} records, capacity {cap}")
        se = episodes["step_env"][:n].cpu().numpy()
        order = np.lexsort((se[:, 1], se[:, 0]))
        return dict(step=se[order, 0], env=se[order, 1], r=episodes["r"][:n].cpu().numpy()[order],
                    l=episodes["l"][:n].cpu().numpy()[order], truncated=episodes["truncated"][:n].cpu().numpy()[order].astype(bool))

    @staticmethod
    def terminal_records(terminal):
        """(step int32 [n], env int32 [n], obs float32 [n, D]) sorted by (step, env); raises if the list overflowed"""
        n = int(terminal["count"].item())
        cap = int(terminal["step_env"].shape[0])
        if n > cap:
            raise OverflowError(f"terminal list overflow: {n} records, capacity {cap}")
        se = terminal["step_env"][:n].cpu().numpy()
        ob = terminal["obs"][:n].cpu().numpy()
        order = np.lexsort((se[:, 1], se[:, 0]))
        return se[order, 0], se[order, 1], ob[order]

    def check_status(self):
        """waits for the enqueued work; raises if a rollout kernel's bounded wave hand-off wait ran out, or a device-side call
        refused its input (render id, profile index, a restore's snapshot or source index) since the last call (sg_check_status)"""
        self._ck(self._lib.sg_check_status(self._h), "sg_check_status")

    # ------------------------------------------------------------------ complete snapshot
    def save_state(self):
        """opaque uint8 blob with every per-env column (incl. the tiling state and episode counters) and the RNG key"""
        n = int(self._lib.sg_state_bytes(self._h))
        blob = np.empty(n, np.uint8)
        self._ck(self._lib.sg_save_state(self._h, self._ptr(blob), n), "sg_save_state")
        return blob

    def load_state(self, blob):
        """a save_state() blob taken with episode statistics on switches them on and resumes them"""
        blob = np.ascontiguousarray(blob, np.uint8)
        self._ck(self._lib.sg_load_state(self._h, self._ptr(blob), blob.size), "sg_load_state")
        if self._snapshot_has_episodes(blob) and not self._episode_stats:
            self._episode_stats = True
            self._blocks = {}

    SNAPSHOT_HEADER_BYTES = 48  # sizeof(SnapshotHeader), which csrc/sg_engine.hip pins with a static_assert

    def _snapshot_blocks(self, version, flags=0, n_profiles=0):
        """(name, dtype, shape) of the blocks of a blob of this env, in order: the mirror of snapshot_layout() in
        csrc/sg_engine.hip, where the format is described (norm_mean, norm_var, norm_count are its norm_stats block).  Like
        there, a reader that does not know flags or n_profiles yet passes 0: the blocks before the word that holds them stay"""
        B, S, goal = self.num_envs, self.obs_dim + 1, self.spec["family"] == "goal"
        eps, nrm, prf = flags & 1, flags & 2, flags & 4
        table = [("header", np.uint8, (self.SNAPSHOT_HEADER_BYTES,), True),
                 ("q0", np.float32, (B, 4), True), ("q1", np.float32, (B, 4), True),
                 ("ctr", np.uint32, (B, 2), True), ("aux", np.uint32, (B, 4), True),
                 ("pl0", np.float32, (B, 4), goal), ("pl1", np.float32, (B, 4), goal and self.n_planets > 2),
                 ("cshift", np.float32, (B, 4), goal), ("orbd", np.float64, (B, 2), self.env_id == "KeplerRandomOrbits-v0"),
                 ("flags", np.uint32, (1, 2), version == 3),
                 ("ep_ret", np.float64, (B, 1), eps), ("ep_len", np.int32, (B, 1), eps),
                 ("norm_config", np.uint8, (C.sizeof(_native.SgNormalize),), nrm),
                 ("norm_mean", np.float64, (S,), nrm), ("norm_var", np.float64, (S,), nrm), ("norm_count", np.float64, (S,), nrm),
                 ("norm_returns", np.float64, (B,), nrm),
                 ("profile_count", np.uint32, (2,), prf),
                 ("profiles", np.uint8, (n_profiles * C.sizeof(_native.SgRewardProfile),), prf),
                 ("profile_index", np.uint8, (B,), prf)]
        return [row[:3] for row in table if row[3]]

    def _snapshot_views(self, blob, blocks):
        """{name: view of the blob} of `blocks`, and where the last one ends"""
        off, out = 0, {}
        for name, dt, shape in blocks:
            n = int(np.prod(shape))
            out[name] = np.frombuffer(blob, dtype=dt, count=n, offset=off).reshape(shape)
            off += out[name].nbytes
        return out, off

    @staticmethod
    def _snapshot_version(blob):
        return int(np.frombuffer(blob, dtype=np.uint32, count=2)[1])

    def _snapshot_flags(self, blob):
        """which blocks follow the columns (1: episode statistics, 2: normalization, 4: reward profiles): the flags word of a
        version-3 blob; versions 1 and 2 are flags 0 and 1 without the word"""
        version = self._snapshot_version(blob)
        if version < 3:
            return int(version == 2)
        return int(self._snapshot_views(blob, self._snapshot_blocks(3))[0]["flags"][0, 0])

    def _snapshot_has_episodes(self, blob):
        return bool(self._snapshot_flags(blob) & 1)

    def snapshot_columns(self, blob):
        """introspection of a save_state() blob: its blocks (all but the header) as NumPy views under the names of
        _snapshot_blocks -- q0 (x, y, theta, vx), q1 (vy, omega, goal_x, goal_y | orbit angle, eccentricity), ctr (elapsed,
        episode), aux (goal draws, ship_tile | goal_tile << 8 | case_b << 16 | flip << 17, free-tile multiset lo, hi),
        Goal: pl0 / pl1 (two planets each), cshift (tiling column shifts); KeplerRandomOrbits: orbd (cos, sin of the angle);
        then what the blob was taken with: flags, ep_ret / ep_len, norm_config (sg_normalize bytes) and norm_*,
        profile_count (n, 0), profiles (sg_reward_profile bytes) and profile_index.  Raises if they do not add up to the blob"""
        version, flags = self._snapshot_version(blob), self._snapshot_flags(blob)
        n_profiles = 0
        if flags & 4:
            n_profiles = int(self._snapshot_views(blob, self._snapshot_blocks(version, flags))[0]["profile_count"][0])
        out, off = self._snapshot_views(blob, self._snapshot_blocks(version, flags, n_profiles))
        assert off == blob.size, (off, blob.size)
        del out["header"]
        return out

    # ------------------------------------------------------------------ device-resident snapshots
    def snapshot_torch(self, out=None):
        """The per-env data of the handle (state columns, running episode statistics and normalizer returns when on) copied into
        a buffer in device memory on torch's current stream (sg_snapshot_device: one launch, no host synchronisation,
        graph-capturable).  Returns a DeviceSnapshot; out= (an earlier one of this env) reuses its buffer.  Not in a snapshot: the
        seed, the normalizer's running statistics, the reward profiles and every env's profile index."""
        import torch
        n = int(self._lib.sg_snapshot_bytes(self._h))
        if out is None:
            out = DeviceSnapshot(torch.empty(n, dtype=torch.uint8, device=f"cuda:{self.device}"), self.num_envs, self.env_id)
        self._check_snapshot("out", out, n)
        self._ck(self._lib.sg_snapshot_device(self._h, C.c_void_p(out.buffer.data_ptr()), C.c_size_t(n), self._stream()),
                 "sg_snapshot_device")
        return out

    def _check_snapshot(self, name, snap, n):
        if not isinstance(snap, DeviceSnapshot):
            raise ValueError(f"{name}: expected a DeviceSnapshot (snapshot_torch), got {type(snap).__name__}")
        if snap.num_envs != self.num_envs or snap.env_id != self.env_id:
            raise ValueError(f"{name}: a snapshot of {snap.num_envs} envs of {snap.env_id}, this env has {self.num_envs} of {self.env_id}")
        import torch
        buf = snap.buffer
        if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.device.index == self.device):
            raise ValueError(f"{name}.buffer: expected a CUDA tensor on device {self.device}")
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() < n or not buf.is_contiguous():
            raise ValueError(f"{name}.buffer: expected contiguous uint8 of at least {n} bytes (has the env's configuration -- episode "
                             f"statistics, normalization -- changed since the snapshot?), got {buf.dtype} {tuple(buf.shape)}")

    def restore_torch(self, snap, mask=None, src=None, out=None):
        """Env i with mask[i] set (mask None: every env) takes the state of the snapshot's env src[i] (src None: i) on torch's
        current stream (sg_restore_device: no host synchronisation, graph-capturable).  mask: bool or uint8 CUDA tensor
        [num_envs]; src: int32 CUDA tensor [num_envs] (duplicates allowed; an index outside the batch leaves its env as it is
        and check_status() raises).  Only the restored envs' rows of `out` (default: the env's own obs tensor, as reset_torch)
        are written: the observation of the restored state, normalized with the statistics as they are -- which a restore does
        not update.  With rendering on every trace starts afresh.  Returns the obs tensor."""
        torch, bufs = self._torch()
        self._check_snapshot("snap", snap, int(self._lib.sg_snapshot_bytes(self._h)))
        obs = bufs["obs"] if out is None else out
        if out is not None:
            self._check_tensor("out", out, torch.float32, (self.num_envs, self.obs_dim))
        if mask is not None:
            if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)  # (same bytes: no copy)
            self._check_tensor("mask", mask, torch.uint8, (self.num_envs,))
        if src is not None:
            self._check_tensor("src", src, torch.int32, (self.num_envs,))
        self._ck(self._lib.sg_restore_device(self._h, C.c_void_p(snap.buffer.data_ptr()), C.c_size_t(snap.buffer.numel()),
                                             C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                             C.c_void_p(src.data_ptr()) if src is not None else None,
                                             C.c_void_p(obs.data_ptr()), self._stream()), "sg_restore_device")
        return obs

    def snapshot(self):
        """NumPy-path convenience: snapshot_torch() after the work enqueued so far (the snapshot itself stays on the device)"""
        import torch
        snap = self.snapshot_torch()
        torch.cuda.current_stream(self.device).synchronize()
        return snap

    def restore(self, snap, mask=None, src=None):
        """NumPy-path convenience over restore_torch: mask (bool or uint8 [num_envs]) and src (integers [num_envs]) are host
        arrays; returns the host observation block the way reset(mask=...) does -- the restored envs' rows replaced, the other
        rows what the last reset() / step() returned."""
        import torch
        dev = f"cuda:{self.device}"
        m = torch.from_numpy(self._mask_host(mask).copy()).to(dev) if mask is not None else None
        if src is not None:
            src = np.asarray(src)
            if src.dtype.kind not in "iu" or src.shape != (self.num_envs,):
                raise ValueError(f"src: expected integers of shape ({self.num_envs},), got {src.dtype} {src.shape}")
            src = torch.from_numpy(np.clip(src, -1, self.num_envs).astype(np.int32)).to(dev)  # (outside the batch stays outside)
        last = self._last_obs if self._last_obs is not None else self._obs
        obs = torch.from_numpy(np.ascontiguousarray(last, np.float32)).to(dev)
        self.restore_torch(snap, mask=m, src=src, out=obs)
        np.copyto(self._obs, obs.cpu().numpy())
        self._last_obs = self._obs
        return self._obs.copy() if self.copy else self._obs

    # ------------------------------------------------------------------ GAE advantages and returns of a rollout
    @staticmethod
    def _gae_config(gamma, lam, bootstrap_truncated):
        gamma, lam = float(gamma), float(lam)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lam must be in [0, 1], got {lam}")
        return _native.SgGaeConfig(C.sizeof(_native.SgGaeConfig), gamma, lam, int(bool(bootstrap_truncated)))

    @staticmethod
    def value_list_torch(terminal, values):
        """the `terminal=` argument of gae_torch from a rollout's terminal list (terminal_list_torch, filled by rollout_torch)
        and the caller's values of its observations, V(terminal["obs"]) as float32 [capacity]"""
        return dict(count=terminal["count"], step_env=terminal["step_env"], value=values)

    def gae_torch(self, reward, done, trunc, value=None, last_value=None, terminal_value=None, terminal=None, gamma=0.99, lam=0.95,
                  bootstrap_truncated=True, out=None):
        """Advantages and returns of a rollout by generalized advantage estimation (sg_gae_device: one launch, two with a
        list; torch's current stream, no host synchronisation, nothing allocated by the engine, graph-capturable).
        reward float32 / done, trunc uint8 [K, B] as rollout_torch wrote them; value float32 [K, B]: V of the observation action t
        was taken from (None: zeros -- the advantage is the discounted reward-to-go); last_value float32 [B]: V of obs[K - 1]
        (None: zeros).  The value of the last observation of an episode that was truncated at (t, i), to bootstrap from, comes
        either from terminal_value (dense float32 [K, B], read only where done and trunc are both set) or from terminal, a dict
        count / step_env / value (value_list_torch: a rollout's terminal list with V(terminal["obs"]) beside it); with neither,
        or bootstrap_truncated=False, a truncation ends the episode like a terminal event.  out: dict advantage / returns of
        float32 [K, B] (allocated when absent).  Returns (advantage, returns); tests/gae_model.py states the arithmetic."""
        import torch
        if terminal_value is not None and terminal is not None:
            raise ValueError("terminal_value and terminal: give the terminal values in one form")
        cfg = self._gae_config(gamma, lam, bootstrap_truncated)
        if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
            raise ValueError("reward: expected a CUDA tensor of shape (K, num_envs)")
        K, B = int(reward.shape[0]), self.num_envs
        if K < 1:
            raise ValueError("reward: expected at least one step")
        self._check_tensor("reward", reward, torch.float32, (K, B))
        self._check_tensor("done", done, torch.uint8, (K, B))
        self._check_tensor("trunc", trunc, torch.uint8, (K, B))
        if value is not None:
            self._check_tensor("value", value, torch.float32, (K, B))
        if last_value is not None:
            self._check_tensor("last_value", last_value, torch.float32, (B,))
        if terminal_value is not None:
            self._check_tensor("terminal_value", terminal_value, torch.float32, (K, B))
        vl = None
        if terminal is not None:
            cap = int(terminal["step_env"].shape[0])
            if (not isinstance(terminal["count"], torch.Tensor) or terminal["count"].dtype not in (torch.int32, torch.uint32)
                    or terminal["count"].numel() != 1):
                raise ValueError("terminal['count']: expected one 32-bit integer")
            self._check_tensor("terminal['count']", terminal["count"], terminal["count"].dtype, tuple(terminal["count"].shape))
            self._check_tensor("terminal['step_env']", terminal["step_env"], torch.int32, (cap, 2))
            self._check_tensor("terminal['value']", terminal["value"], torch.float32, (cap,))
            vl = _native.SgValueList(terminal["count"].data_ptr(), terminal["step_env"].data_ptr(), terminal["value"].data_ptr(), cap)
        if out is None:
            out = dict(advantage=torch.empty((K, B), dtype=torch.float32, device=reward.device),
                       returns=torch.empty((K, B), dtype=torch.float32, device=reward.device))
        else:
            self._check_tensor("out['advantage']", out["advantage"], torch.float32, (K, B))
            self._check_tensor("out['returns']", out["returns"], torch.float32, (K, B))

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self._lib.sg_gae_device(self._h, K, C.byref(cfg), ptr(reward), ptr(done), ptr(trunc), ptr(value), ptr(last_value),
                                         ptr(terminal_value), C.byref(vl) if vl is not None else None, ptr(out["advantage"]),
                                         ptr(out["returns"]), self._stream()), "sg_gae_device")
        return out["advantage"], out["returns"]

    # ------------------------------------------------------------------ GAE and V-trace targets with per-group discounts
    def _returns_call(self, reward, done, trunc, value, last_value, ratio, terminal_value, terminal, discounts, out, names):
        """what gae_groups_torch and vtrace_torch check as gae_torch does; returns (K, the groups of `discounts` or 0, the value list or
        None, the two outputs named `names` -- allocated when out is None)"""
        import torch
        if terminal_value is not None and terminal is not None:
            raise ValueError("terminal_value and terminal: give the terminal values in one form")
        if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
            raise ValueError("reward: expected a CUDA tensor of shape (K, num_envs)")
        K, B = int(reward.shape[0]), self.num_envs
        if K < 1:
            raise ValueError("reward: expected at least one step")
        self._check_tensor("reward", reward, torch.float32, (K, B))
        self._check_tensor("done", done, torch.uint8, (K, B))
        self._check_tensor("trunc", trunc, torch.uint8, (K, B))
        for name, t, shape in (("value", value, (K, B)), ("last_value", last_value, (B,)), ("ratio", ratio, (K, B)),
                               ("terminal_value", terminal_value, (K, B))):
            if t is not None:
                self._check_tensor(name, t, torch.float32, shape)
        groups = 0
        if discounts is not None:
            if not isinstance(discounts, torch.Tensor) or discounts.dim() != 2:
                raise ValueError("discounts: expected a CUDA tensor of shape (groups, 2)")
            groups = int(discounts.shape[0])
            self._check_tensor("discounts", discounts, torch.float32, (groups, 2))
            if groups < 1 or B % groups:
                raise ValueError(f"discounts: its {groups} rows must divide num_envs = {B}")
        vl = None
        if terminal is not None:
            cap = int(terminal["step_env"].shape[0])
            if (not isinstance(terminal["count"], torch.Tensor) or terminal["count"].dtype not in (torch.int32, torch.uint32)
                    or terminal["count"].numel() != 1):
                raise ValueError("terminal['count']: expected one 32-bit integer")
            self._check_tensor("terminal['count']", terminal["count"], terminal["count"].dtype, tuple(terminal["count"].shape))
            self._check_tensor("terminal['step_env']", terminal["step_env"], torch.int32, (cap, 2))
            self._check_tensor("terminal['value']", terminal["value"], torch.float32, (cap,))
            vl = _native.SgValueList(terminal["count"].data_ptr(), terminal["step_env"].data_ptr(), terminal["value"].data_ptr(), cap)
        if out is None:
            out = {n: torch.empty((K, B), dtype=torch.float32, device=reward.device) for n in names}
        else:
            for n in names:
                self._check_tensor(f"out['{n}']", out[n], torch.float32, (K, B))
        return K, groups, vl, out

    def gae_groups_torch(self, reward, done, trunc, discounts, value=None, last_value=None, terminal_value=None, terminal=None,
                         bootstrap_truncated=True, out=None):
        """gae_torch with per-group discounts read on the device (sg_gae_groups_device).  discounts: float32 device tensor [G, 2] of
        (gamma, lambda) rows; G divides num_envs and env i uses row i // (num_envs // G) -- G = members gives a population per-member
        discounts, G = num_envs per-env ones.  The kernel reads the tensor at every call or graph replay, so PBT's explore step or a
        schedule inside a captured graph is a write to it; its values are NOT checked (a NaN or a value outside [0, 1] affects that
        group's envs only).  Everything else is gae_torch's; equal rows give gae_torch's bits at gamma = float(float32(g)), lam
        likewise.  Returns (advantage, returns); tests/returns_model.py states the arithmetic."""
        if discounts is None:
            raise ValueError("discounts: expected a CUDA tensor of shape (groups, 2)")
        K, groups, vl, out = self._returns_call(reward, done, trunc, value, last_value, None, terminal_value, terminal, discounts, out,
                                                ("advantage", "returns"))
        cfg = _native.SgReturnsConfig(C.sizeof(_native.SgReturnsConfig), groups, discounts.data_ptr(), 0.99, 0.95, int(bool(bootstrap_truncated)),
                                      1.0, 1.0, 1.0, 0)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self._lib.sg_gae_groups_device(self._h, K, C.byref(cfg), ptr(reward), ptr(done), ptr(trunc), ptr(value), ptr(last_value),
                                                ptr(terminal_value), C.byref(vl) if vl is not None else None, ptr(out["advantage"]),
                                                ptr(out["returns"]), self._stream()), "sg_gae_groups_device")
        return out["advantage"], out["returns"]

    def vtrace_torch(self, reward, done, trunc, value, last_value=None, ratio=None, terminal_value=None, terminal=None, gamma=0.99, lam=1.0,
                     discounts=None, rho_bar=1.0, c_bar=1.0, pg_rho_bar=None, bootstrap_truncated=True, out=None):
        """V-trace value targets and policy-gradient advantages of a rollout (sg_vtrace_device; Espeholt et al. 2018): the
        importance-corrected counterpart of gae_torch for rows the policy being updated did not generate -- another member's env block,
        a later epoch over the same rollout.  ratio float32 [K, B]: exp(logp_target - logp_behaviour) of the action taken, formed by the
        caller (None: on-policy, all ones; with the bars >= 1 vs is then gae_torch's returns bit for bit).  value is required.  The
        discounts are the scalars gamma / lam, or -- discounts float32 [G, 2] given -- the rows of a device table as in gae_groups_torch
        (gamma and lam are then not read).  rho_bar, c_bar, pg_rho_bar (None: rho_bar) clip the ratio of the temporal difference, of the
        trace and of pg_advantage; each > 0, float("inf") for none.  reward / done / trunc / last_value / terminal_value / terminal /
        bootstrap_truncated as gae_torch's.  out: dict vs / pg_advantage of float32 [K, B] (allocated when absent).  Returns
        (vs, pg_advantage); tests/returns_model.py states the arithmetic."""
        if pg_rho_bar is None:
            pg_rho_bar = rho_bar
        bars = dict(rho_bar=float(rho_bar), c_bar=float(c_bar), pg_rho_bar=float(pg_rho_bar))
        for name, bar in bars.items():
            if not bar > 0.0:
                raise ValueError(f"{name} must be > 0, got {bar}")
        if discounts is None:
            checked = self._gae_config(gamma, lam, bootstrap_truncated)  # (gamma and lam in [0, 1])
            gamma, lam = checked.gamma, checked.lambda_
        else:
            gamma, lam = 0.99, 0.95  # (not read)
        if value is None:
            raise ValueError("value: V-trace needs the values of the rollout's observations")
        K, groups, vl, out = self._returns_call(reward, done, trunc, value, last_value, ratio, terminal_value, terminal, discounts, out,
                                                ("vs", "pg_advantage"))
        cfg = _native.SgReturnsConfig(C.sizeof(_native.SgReturnsConfig), groups, discounts.data_ptr() if groups else None, gamma, lam,
                                      int(bool(bootstrap_truncated)), bars["rho_bar"], bars["c_bar"], bars["pg_rho_bar"], 0)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self._lib.sg_vtrace_device(self._h, K, C.byref(cfg), ptr(reward), ptr(done), ptr(trunc), ptr(value), ptr(last_value), ptr(ratio),
                                            ptr(terminal_value), C.byref(vl) if vl is not None else None, ptr(out["vs"]),
                                            ptr(out["pg_advantage"]), self._stream()), "sg_vtrace_device")
        return out["vs"], out["pg_advantage"]

    # ------------------------------------------------------------------ Retrace(lambda) / Q(lambda) targets over replayed sequences
    _RETRACE_LOSS_KEYS = ("q_online", "weight", "huber_delta", "td_error", "g")

    def retrace_torch(self, reward, done, trunc, q, value, last_value=None, ratio=None, terminal_value=None, gamma=0.99, lam=1.0, c_bar=1.0,
                      discounts=None, bootstrap_truncated=True, out=None, loss=None):
        """Multi-step off-policy-corrected targets for Q(s_t, a_t) over a time-major sequence batch [L, n] -- what
        replay_sample_sequences_torch returns, any n (sg_retrace_device; Munos et al. 2016): one launch on torch's current stream, no
        host synchronisation, graph-capturable.  q float32 [L, n]: Q(s_t, a_t) of the net the targets are built from (normally the
        target net); value float32 [L, n]: V_pi(s_t) = E_{a ~ pi} Q(s_t, a) under the target policy; last_value float32 [n]: V_pi(s_L)
        (None: zeros).  Per column, backwards in float64:
            G_t = r_t + gamma * (done_t ? (trunc_t ? terminal_value_t : 0) : value_{t+1} + c_{t+1} (G_{t+1} - q_{t+1})),
            c_t = lam * min(c_bar, ratio_t)
        and target = float32(G).  ratio float32 [L, n] is the caller's (no exp runs on the device) and picks the estimator: pi / mu with
        c_bar = 1 is Retrace(lambda); pi(a_t | s_t) tree backup; None (all ones) Peng's Q(lambda); [a_t greedy] Watkins' Q(lambda);
        pi / mu with c_bar = float("inf") plain importance sampling; lam = 0 one-step TD.  terminal_value float32 [L, n] is read only
        where done and trunc are both set (None, or bootstrap_truncated=False: a truncation bootstraps from 0).  The discounts are the
        scalars gamma / lam in [0, 1], or -- discounts given -- a float32 device tensor [2] of (gamma, lam) that the kernel reads at
        every launch or graph replay (its values are not checked; gamma and lam are then not read).  c_bar > 0.  out: the float32
        [L, n] target to fill (allocated when None).
        loss: None, or dict(q_online=float32 [L, n], weight=None or float32 [n], huber_delta=inf, td_error=None, g=None): the same launch
        also writes td_error = q_online - target and g = (weight * clip(td_error, -huber_delta, huber_delta)) / (L * n), the Huber
        loss' gradient by q_online -- flattened, the g_taken of dqn_grad_torch / q_grad_torch (td_error, g: float32 [L, n] tensors to
        fill, allocated when None).  Returns target, or with loss (target, td_error, g).  tests/retrace_model.py states the arithmetic."""
        import torch
        c_bar = float(c_bar)
        if not c_bar > 0.0:
            raise ValueError(f"c_bar must be > 0, got {c_bar}")
        if discounts is None:
            checked = self._gae_config(gamma, lam, bootstrap_truncated)  # (gamma and lam in [0, 1])
            gamma, lam = checked.gamma, checked.lambda_
        else:
            gamma, lam = 0.99, 1.0  # (not read)
        if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
            raise ValueError("reward: expected a CUDA tensor of shape (L, n)")
        L, n = int(reward.shape[0]), int(reward.shape[1])
        if L < 1 or n < 1:
            raise ValueError("reward: expected at least one step and one column")
        if L * n > 2 ** 31 - 1:
            raise ValueError(f"reward: L * n = {L * n}: at most 2^31 - 1 (elements are addressed by 32 bits)")
        self._check_tensor("reward", reward, torch.float32, (L, n))
        self._check_tensor("done", done, torch.uint8, (L, n))
        self._check_tensor("trunc", trunc, torch.uint8, (L, n))
        if q is None:
            raise ValueError("q: Retrace needs Q(s_t, a_t) of the actions taken")
        if value is None:
            raise ValueError("value: Retrace needs V_pi(s_t) of the sequence's observations")
        for name, t, shape in (("q", q, (L, n)), ("value", value, (L, n)), ("last_value", last_value, (n,)), ("ratio", ratio, (L, n)),
                               ("terminal_value", terminal_value, (L, n)), ("discounts", discounts, (2,))):
            if t is not None:
                self._check_tensor(name, t, torch.float32, shape)
        q_online = weight = td_error = g = None
        huber_delta = float("inf")
        if loss is not None:
            if not isinstance(loss, dict) or set(loss) - set(self._RETRACE_LOSS_KEYS):
                raise ValueError(f"loss: expected a dict with keys among {self._RETRACE_LOSS_KEYS}")
            q_online, weight = loss.get("q_online"), loss.get("weight")
            if q_online is None:
                raise ValueError("loss['q_online']: missing")
            self._check_tensor("loss['q_online']", q_online, torch.float32, (L, n))
            if weight is not None:
                self._check_tensor("loss['weight']", weight, torch.float32, (n,))
            huber_delta = float(loss.get("huber_delta", float("inf")))
            if not huber_delta > 0.0:
                raise ValueError(f"loss['huber_delta'] must be > 0, got {huber_delta}")
            for k in ("td_error", "g"):
                if loss.get(k) is not None:
                    self._check_tensor(f"loss['{k}']", loss[k], torch.float32, (L, n))
        if out is None:
            out = torch.empty((L, n), dtype=torch.float32, device=reward.device)
        else:
            self._check_tensor("out", out, torch.float32, (L, n))
        if loss is not None:
            td_error, g = (loss.get(k) if loss.get(k) is not None else torch.empty((L, n), dtype=torch.float32, device=reward.device)
                           for k in ("td_error", "g"))
        cfg = _native.SgRetraceConfig(C.sizeof(_native.SgRetraceConfig), gamma, lam, c_bar, int(bool(bootstrap_truncated)), huber_delta,
                                      discounts.data_ptr() if discounts is not None else None, 0)
        self._ck(self._lib.sg_retrace_device(self._h, L, n, C.byref(cfg), _ptr(reward), _ptr(done), _ptr(trunc), _ptr(q), _ptr(value),
                                             _ptr(last_value), _ptr(ratio), _ptr(terminal_value), _ptr(out), _ptr(q_online), _ptr(weight),
                                             _ptr(td_error), _ptr(g), self._stream()), "sg_retrace_device")
        return out if loss is None else (out, td_error, g)

    # ------------------------------------------------------------------ what the net handles and their methods share
    def _mlp_layers(self, name, layers, fan_in, out, mlp, keep, members=None):
        """checks one net [(weight, bias), ...] of fan_in -> hidden -> ... -> out, writes its pointers into the sg_policy_mlp `mlp`,
        appends its tensors to `keep` and returns (n_hidden, hidden); members: a stacked net (weight [P, width, fan_in], bias
        [P, width]), whose pointers address member 0"""
        import torch
        layers = [tuple(l) for l in layers]
        lead = () if members is None else (members,)
        n_hidden = len(layers) - 1
        if not 1 <= n_hidden <= 3:
            raise ValueError(f"{name}: n_hidden must be 1 .. 3 (2 .. 4 (weight, bias) pairs with the head), got {n_hidden}")
        w0 = layers[0][0]
        if not isinstance(w0, torch.Tensor) or w0.dim() != 2 + len(lead):
            raise ValueError(f"{name}[0]: expected a " + (f"stacked weight of shape ({members}, hidden, {fan_in})" if lead else
                                                          f"weight of shape (hidden, {fan_in})"))
        hidden = int(w0.shape[-2])
        if not 1 <= hidden <= 128:
            raise ValueError(f"{name}: hidden must be 1 .. 128, got {hidden}")
        for l, (w, b) in enumerate(layers):
            width = out if l == n_hidden else hidden
            self._check_tensor(f"{name}[{l}] weight", w, torch.float32, (*lead, width, fan_in))
            self._check_tensor(f"{name}[{l}] bias", b, torch.float32, (*lead, width))
            mlp.weight[l], mlp.bias[l] = w.data_ptr(), b.data_ptr()
            keep.extend((w, b))
            fan_in = hidden
        return n_hidden, hidden

    def _net_handle(self, handle, cls, who=None):
        """checks a handle's class and, for `who` (a method of the continuous ids only), the id's action space"""
        name, maker, subject = _NET_HANDLES[cls]
        if not isinstance(handle, cls):
            raise ValueError(f"{name}: expected the handle {maker} returns")
        if who is not None and self.discrete:
            raise ValueError(f"{who}: {subject} needs a continuous id; the discrete ids are not served")

    def _net_rows(self, handle, cls, obs, who=None, **cols):
        """checks (handle, obs [n, D]) as _net_handle and a column beside obs -- action=: [n, 2], int32 [n] under a discrete id's
        Policy or Dqn; eps=: [n, 2], or None -- and returns n"""
        import torch
        self._net_handle(handle, cls, who)
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or int(obs.shape[0]) < 1:
            raise ValueError(f"obs: expected a CUDA tensor of shape (n, {self.obs_dim}) with n >= 1")
        n = int(obs.shape[0])
        self._check_tensor("obs", obs, torch.float32, (n, self.obs_dim))
        if "action" in cols:
            index = self.discrete and cls in (Policy, Dqn)
            self._check_tensor("action", cols["action"], torch.int32 if index else torch.float32, (n,) if index else (n, 2))
        if cols.get("eps") is not None:
            self._check_tensor("eps", cols["eps"], torch.float32, (n, 2))
        return n

    def _grad_pairs(self, name, pairs, like, mlp):
        """checks the (weight, bias) gradient tensors of one net against its parameters `like` (w0, b0, w1, ...) and writes their
        pointers into the sg_policy_grads_mlp `mlp`"""
        import torch
        pairs = [tuple(x) for x in pairs]
        if 2 * len(pairs) != len(like):
            raise ValueError(f"{name}: expected {len(like) // 2} (weight, bias) pairs, got {len(pairs)}")
        for l, (w, b) in enumerate(pairs):
            self._check_tensor(f"{name}[{l}] weight", w, torch.float32, tuple(like[2 * l].shape))
            self._check_tensor(f"{name}[{l}] bias", b, torch.float32, tuple(like[2 * l + 1].shape))
            mlp.weight[l], mlp.bias[l] = w.data_ptr(), b.data_ptr()

    def _grad_workspace(self, handle, bytes_fn, n, device, who, refused=None, members=None, query=None):
        """the workspace tensor cached on a Policy / QNet / SquashedPolicy / Dqn / PolicyPopulation handle, grown when n needs more -- never
        inside a capture; refused: what the error names when the engine refuses the net or n (default: who); members: a population's,
        which its query takes before n; query: the arguments of bytes_fn after the env, where they are not (the handle's struct, n)"""
        import torch
        if query is None:
            query = (C.byref(handle.struct), *((n,) if members is None else (members, n)))
        need = int(getattr(self._lib, bytes_fn)(self._h, *query))
        if need == 0:
            self._ck(-1, refused or who)
        ws = handle.workspace
        if ws is None or ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError(f"{who}: the workspace ({0 if ws is None else ws.numel()} bytes) is too small for n = {n} ({need} bytes) "
                                 "and cannot be allocated during a graph capture: make one warm-up call with this n before capturing")
            ws = handle.workspace = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def _actor_critic_struct(self, members, actor, critic, log_std, activation):
        """(the sg_policy over the nets of a policy, or over the stacked nets of `members` of them; the tensors it points into)"""
        import torch
        lead = () if members is None else (members,)
        head = 6 if self.discrete else 2
        p = _native.SgPolicy(struct_size=C.sizeof(_native.SgPolicy), activation=_activation_code(activation), head=head)
        keep = []
        p.n_hidden, p.hidden = self._mlp_layers("actor", actor, self.obs_dim, head, p.actor, keep, members)
        if critic is not None:
            if self._mlp_layers("critic", critic, self.obs_dim, 1, p.critic, keep, members) != (p.n_hidden, p.hidden):
                raise ValueError(f"critic: expected {p.n_hidden} hidden layers of width {p.hidden}, like the actor")
        if self.discrete:
            if log_std is not None:
                raise ValueError("log_std: the discrete ids take none")
        else:
            if log_std is None:
                raise ValueError(f"log_std: a continuous id needs the float32 {list(lead + (2,))} log standard deviations")
            self._check_tensor("log_std", log_std, torch.float32, (*lead, 2))
            p.log_std = log_std.data_ptr()
            keep.append(log_std)
        return p, keep

    def _act_out(self, out, noun, has_critic, device, values_alone):
        """(action, logp, value) of an act call over the handle's envs: allocated, or out's, checked; values_alone: out may ask for
        the values only"""
        import torch
        B = self.num_envs
        a_dtype, a_shape = (torch.int32, (B,)) if self.discrete else (torch.float32, (B, 2))
        if out is None:
            return (torch.empty(a_shape, dtype=a_dtype, device=device), torch.empty(B, dtype=torch.float32, device=device),
                    torch.empty(B, dtype=torch.float32, device=device) if has_critic else None)
        action = logp = None
        if not values_alone or out.get("action") is not None:
            action, logp = out["action"], out["logp"]
            self._check_tensor("out['action']", action, a_dtype, a_shape)
            self._check_tensor("out['logp']", logp, torch.float32, (B,))
        elif out.get("value") is None:
            raise ValueError("out: expected action (with logp), value, or both")
        value = out.get("value")
        if value is not None:
            if not has_critic:
                raise ValueError(f"out['value']: the {noun} has no critic")
            self._check_tensor("out['value']", value, torch.float32, (B,))
        return action, logp, value

    def _rollout_buffers(self, obs, action, action_like, cols, reward, done, trunc):
        """checks the buffers of K closed-loop steps and returns K: obs [K + 1, B, D], action (action_like: the test of its dim() and
        the shape the message names), then cols -- (name, float32 tensor, rows beyond K) -- and reward / done / trunc [K, B]"""
        import torch
        dim_ok, shape = action_like
        if not isinstance(action, torch.Tensor) or not dim_ok(action.dim()) or int(action.shape[0]) < 1:
            raise ValueError(f"action: expected a CUDA tensor {shape}of at least one step")
        K, B = int(action.shape[0]), self.num_envs
        self._check_tensor("obs", obs, torch.float32, (K + 1, B, self.obs_dim))
        self._check_tensor("action", action, torch.int32 if self.discrete else torch.float32, (K, B) if self.discrete else (K, B, 2))
        for name, t, extra in cols:
            self._check_tensor(name, t, torch.float32, (K + extra, B))
        self._check_tensor("reward", reward, torch.float32, (K, B))
        self._check_tensor("done", done, torch.uint8, (K, B))
        self._check_tensor("trunc", trunc, torch.uint8, (K, B))
        return K

    def _out_columns(self, out, cols):
        """an out dict of optional columns, each (name, dtype, shape): at least one given, those given checked; returns them in
        order, None for a column that is absent"""
        if all(out.get(k) is None for k, _, _ in cols):
            raise ValueError(f"out: expected at least one of {', '.join(k for k, _, _ in cols)}")
        for k, dtype, shape in cols:
            if out.get(k) is not None:
                self._check_tensor(f"out['{k}']", out[k], dtype, shape)
        return tuple(out.get(k) for k, _, _ in cols)

    def _policy_grads(self, handle, out, noun, critic_needed, why):
        """(out, its sg_policy_grads) for the gradients of a Policy or PolicyPopulation: out a dict actor / critic / log_std of tensors
        like the parameters, made when None -- the critic's when critic_needed, else they may be absent (why: what the error says when
        they are needed and are not there)"""
        import torch
        L = handle.n_hidden + 1
        params = handle.tensors
        a_par, c_par = params[:2 * L], params[2 * L:4 * L] if handle.has_critic else ()
        if out is None:
            out = dict(actor=_empty_pairs(a_par), critic=_empty_pairs(c_par) if critic_needed else None,
                       log_std=None if self.discrete else torch.empty_like(params[-1]))
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        self._grad_pairs("out['actor']", out["actor"], a_par, g.actor)
        if out.get("critic") is not None:
            if not handle.has_critic:
                raise ValueError(f"out['critic']: the {noun} has no critic")
            self._grad_pairs("out['critic']", out["critic"], c_par, g.critic)
        elif critic_needed:
            raise ValueError(f"out['critic']: {why}")
        if self.discrete:
            if out.get("log_std") is not None:
                raise ValueError("out['log_std']: the discrete ids have none")
        else:
            shape = tuple(params[-1].shape)
            if out.get("log_std") is None:
                raise ValueError(f"out['log_std']: expected a float32 {list(shape)} tensor")
            self._check_tensor("out['log_std']", out["log_std"], torch.float32, shape)
            g.log_std = out["log_std"].data_ptr()
        return out, g

    # ------------------------------------------------------------------ actor-critic policy on the device, closed-loop rollouts
    def policy_torch(self, actor, critic=None, log_std=None, activation="tanh"):
        """A handle on a small MLP actor-critic whose parameters stay where they are (sg_policy: no copy, no transpose; what an
        optimizer step writes is what the next call reads).  actor / critic: lists [(weight, bias), ...] of float32 CUDA tensors
        in torch.nn.Linear layout -- 1 .. 3 hidden layers of one width (1 .. 128) and the head: obs_dim -> hidden -> ... -> 2
        (continuous ids: the mean; log_std float32 [2] is needed) or 6 (discrete ids: the logits), the critic -> 1 (None: no
        values).  Parameters of nn.Linear modules pass as they are: [(m.weight, m.bias) for m in linears].  activation: "tanh" or
        "relu", after every hidden layer."""
        p, keep = self._actor_critic_struct(None, actor, critic, log_std, activation)
        return Policy(p, keep, critic is not None)

    def policy_act_torch(self, policy, obs, seed=0, step=0, deterministic=False, out=None):
        """(action, logp, value) of the observations obs float32 [B, D] under a policy_torch handle, in one launch on torch's
        current stream (sg_policy_act_device: no host synchronisation, nothing allocated by the engine, graph-capturable).
        action float32 [B, 2], unclamped (discrete ids: int32 [B]); logp float32 [B]; value float32 [B], None without a critic.
        Env i's noise is a function of (seed, step, env_index_base + i); deterministic: the mean / the first argmax.
        out: dict action / logp / value of tensors to fill (allocated when absent)."""
        import torch
        self._net_handle(policy, Policy)
        self._check_tensor("obs", obs, torch.float32, (self.num_envs, self.obs_dim))
        action, logp, value = self._act_out(out, "policy", policy.has_critic, obs.device, values_alone=False)
        self._ck(self._lib.sg_policy_act_device(self._h, C.byref(policy.struct), _ptr(obs), int(seed), int(step), int(bool(deterministic)),
                                                _ptr(action), _ptr(logp), _ptr(value), self._stream()), "sg_policy_act_device")
        return action, logp, value

    def _terminal_list_struct(self, terminal):
        """checks a terminal_list_torch dict and returns (its sg_terminal_list by reference, its capacity), (None, None) for None: shared
        by the closed-loop rollouts"""
        import torch
        if terminal is None:
            return None, None
        for k in ("count", "step_env", "obs"):
            if not isinstance(terminal.get(k), torch.Tensor):
                raise ValueError(f"terminal['{k}']: expected a CUDA tensor (terminal_list_torch makes the dict)")
        if terminal["count"].dtype not in (torch.int32, torch.uint32) or terminal["count"].numel() != 1:
            raise ValueError("terminal['count']: expected one 32-bit integer")
        if terminal["step_env"].dim() != 2:
            raise ValueError("terminal['step_env']: expected an int32 tensor of shape (capacity, 2)")
        cap = int(terminal["step_env"].shape[0])
        self._check_tensor("terminal['count']", terminal["count"], terminal["count"].dtype, tuple(terminal["count"].shape))
        self._check_tensor("terminal['step_env']", terminal["step_env"], torch.int32, (cap, 2))
        self._check_tensor("terminal['obs']", terminal["obs"], torch.float32, (cap, self.obs_dim))
        return C.byref(_native.SgTerminalList(terminal["count"].data_ptr(), terminal["step_env"].data_ptr(), terminal["obs"].data_ptr(), cap)), cap

    def rollout_policy_torch(self, policy, obs, action, logp, value, reward, done, trunc, seed=0, first_step=0, deterministic=False,
                             terminal=None):
        """K closed-loop steps on torch's current stream without a host synchronisation (sg_rollout_policy_device): for every t the
        policy acts on obs[t] (noise step first_step + t) and the env steps into obs[t + 1], exactly as policy_act_torch followed by
        step_torch would.  obs float32 [K + 1, B, D] with the current observations in row 0; action float32 [K, B, 2] (discrete
        ids: int32 [K, B]); logp, reward float32 / done, trunc uint8 [K, B]; value float32 [K + 1, B] (None without a critic): row K
        is GAE's last_value.  terminal: a terminal_list_torch dict; it is filled like rollout_torch's and, with a critic,
        terminal["value"] (float32 [capacity], made on first use) receives V of every record's observation, so that
            env.gae_torch(reward, done, trunc, value[:-1], value[-1], terminal=env.value_list_torch(terminal, terminal["value"]))
        needs nothing in between."""
        import torch
        self._net_handle(policy, Policy)
        if policy.has_critic and value is None:
            raise ValueError("value: the policy has a critic; pass the float32 [K + 1, B] tensor its values go to")
        if not policy.has_critic and value is not None:
            raise ValueError("value: the policy has no critic")
        K = self._rollout_buffers(obs, action, (lambda d: d >= 2, ""), [("logp", logp, 0)] + [("value", value, 1)] * (value is not None), reward,
                                  done, trunc)
        tl, cap = self._terminal_list_struct(terminal)
        tv = None
        if terminal is not None and policy.has_critic:
            if terminal.get("value") is None:
                terminal["value"] = torch.empty(cap, dtype=torch.float32, device=terminal["obs"].device)
            self._check_tensor("terminal['value']", terminal["value"], torch.float32, (cap,))
            tv = terminal["value"]
        self._ck(self._lib.sg_rollout_policy_device(self._h, K, C.byref(policy.struct), int(seed), int(first_step), int(bool(deterministic)),
                                                    _ptr(obs), _ptr(action), _ptr(logp), _ptr(value), _ptr(reward), _ptr(done), _ptr(trunc),
                                                    tl, _ptr(tv), self._stream()), "sg_rollout_policy_device")
        return obs, action, logp, value, reward, done, trunc

    # ------------------------------------------------------------------ the learner's half: evaluate given actions, parameter gradients
    def policy_evaluate_raw_torch(self, policy, obs, action, out=None):
        """(logp, entropy, value) float32 [n] of the given rows -- obs float32 [n, D], action float32 [n, 2] as policy_act_torch stored
        it (discrete ids: int32 [n]) -- under a policy_torch handle: one launch on torch's current stream, no autograd
        (sg_policy_evaluate_device; graph-capturable).  n is the caller's: a minibatch of the flattened rollout.  value and the discrete
        logp are policy_act_torch's bit for bit.  out: dict logp / entropy / value of tensors to fill (allocated when None; an entry
        that is absent or None is not computed).  value is None without a critic."""
        import torch
        n = self._net_rows(policy, Policy, obs, action=action)
        if out is None:
            out = {k: torch.empty(n, dtype=torch.float32, device=obs.device) for k in (("logp", "entropy", "value") if policy.has_critic else ("logp", "entropy"))}
        elif out.get("value") is not None and not policy.has_critic:
            raise ValueError("out['value']: the policy has no critic")
        cols = self._out_columns(out, [(k, torch.float32, (n,)) for k in ("logp", "entropy", "value")])
        self._ck(self._lib.sg_policy_evaluate_device(self._h, C.byref(policy.struct), n, _ptr(obs), _ptr(action), *map(_ptr, cols), self._stream()),
                 "sg_policy_evaluate_device")
        return cols

    def policy_grad_torch(self, policy, obs, action, g_logp=None, g_entropy=None, g_value=None, out=None):
        """Gradients of a loss with respect to the policy's parameters, given the loss's gradients g_logp / g_entropy / g_value
        (float32 [n], None: zeros) by policy_evaluate_raw_torch's outputs at the same (obs, action): sg_policy_grad_device, two
        launches on torch's current stream, the forward pass recomputed inside, graph-capturable after one warm-up call with the same
        n (which sizes the workspace kept on the handle).  Returns a dict actor / critic (lists of (weight, bias) gradients, critic
        None without g_value) / log_std (None for the discrete ids), WRITTEN, not accumulated; out: such a dict of tensors to fill.
        Same inputs and same n: the same bits."""
        import torch
        n = self._net_rows(policy, Policy, obs, action=action)
        for name, g in (("g_logp", g_logp), ("g_entropy", g_entropy), ("g_value", g_value)):
            if g is not None:
                self._check_tensor(name, g, torch.float32, (n,))
        if g_value is not None and not policy.has_critic:
            raise ValueError("g_value: the policy has no critic")
        out, g = self._policy_grads(policy, out, "policy", g_value is not None, "g_value is given; the critic's gradients need tensors")
        ws = self._grad_workspace(policy, "sg_policy_grad_workspace_bytes", n, obs.device, "policy_grad_torch", "sg_policy_grad_workspace_bytes")
        self._ck(self._lib.sg_policy_grad_device(self._h, C.byref(policy.struct), n, _ptr(obs), _ptr(action), _ptr(g_logp), _ptr(g_entropy),
                                                 _ptr(g_value), C.byref(g), _ptr(ws), ws.numel(), self._stream()), "sg_policy_grad_device")
        return out

    def policy_evaluate_torch(self, policy, obs, action):
        """logp, entropy, value = the scores of the stored (obs, action) rows under the CURRENT parameters, differentiable with respect
        to the parameter tensors the handle holds: a torch.autograd.Function whose forward is policy_evaluate_raw_torch and whose
        backward is policy_grad_torch (no [n, hidden] activation is kept between the two; obs and action get no gradient).  Write
        the loss in torch on the three [n] vectors and call backward(): the parameters' .grad accumulate as usual.  Under
        torch.no_grad(), or when no parameter requires grad, it is the plain forward.  value is None without a critic."""
        self._net_rows(policy, Policy, obs, action=action)
        fn = _net_function("PolicyEvaluate", lambda env, h, o, a: env.policy_evaluate_raw_torch(h, o, a), _actor_critic_backward("policy_grad_torch", False), True)
        return fn.apply(self, policy, obs, action, *policy.tensors)

    # ------------------------------------------------------------------ the PPO minibatch update: loss, statistics and gradients in one call
    ppo_stats_names = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "old_approx_kl", "clip_fraction", "adv_mean", "adv_std",
                       "bad_rows", "reserved0", "reserved1")

    def ppo_grad_torch(self, policy, batch, index=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5,
                       normalize_advantage=True, out=None, stats=None, rows=None):
        """One PPO minibatch update without autograd (sg_ppo_grad_device: the gathers, the forward, the clipped loss and the backward in
        two or three launches on torch's current stream; no host synchronisation; graph-capturable after one warm-up call with the same
        n, which sizes the workspace kept on the handle).  batch: dict obs [rows, D] / action [rows, 2] (discrete ids: int32 [rows]) /
        logp / advantage / ret / value (float32 [rows]) of the flattened rollout; ret may be absent without a critic, value unless
        clip_range_vf is given.  index: int64 [n] rows of the minibatch (repeats allowed; None: all rows, in order).  The objective is the
        CleanRL / SB3 form stated in include/spacegym.h: clip_range may be float("inf") (A2C), clip_range_vf None turns value clipping off.
        Returns (grads, stats): grads a dict actor / critic (None without a critic) / log_std (None for the discrete ids) as
        policy_grad_torch's, WRITTEN, not accumulated (out: such a dict of tensors to fill); stats float32 [12], named by
        ppo_stats_names (stats: the tensor to fill).  rows: optional dict logp / value / g_logp / g_value of float32 [n] tensors that
        receive the per-row numbers the kernel used.  ppo_assign_grads hands the gradients to an optimizer.  Same inputs and same n:
        the same bits."""
        import torch
        self._net_handle(policy, Policy)
        obs, R, need = self._ppo_batch(policy, batch, clip_range, clip_range_vf, ent_coef, vf_coef)
        if index is None:
            n = R
        else:
            if not isinstance(index, torch.Tensor) or index.dim() != 1 or int(index.shape[0]) < 1:
                raise ValueError("index: expected an int64 CUDA tensor of shape (n,) with n >= 1")
            n = int(index.shape[0])
            self._check_tensor("index", index, torch.int64, (n,))
        if normalize_advantage and n < 2:
            raise ValueError("normalize_advantage: needs n >= 2")
        out, g = self._policy_grads(policy, out, "policy", policy.has_critic, "the policy has a critic; its gradients need tensors")
        if stats is None:
            stats = obs.new_empty(len(self.ppo_stats_names))
        else:
            self._check_tensor("stats", stats, torch.float32, (len(self.ppo_stats_names),))
        r = self._ppo_rows(policy, rows, (n,), "policy")
        cfg, b = self._ppo_structs(policy, batch, need, index, clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage)
        ws = self._grad_workspace(policy, "sg_ppo_grad_workspace_bytes", n, obs.device, "ppo_grad_torch", "sg_ppo_grad_workspace_bytes")
        self._ck(self._lib.sg_ppo_grad_device(self._h, C.byref(policy.struct), C.byref(cfg), C.byref(b), R, n, C.byref(g), _ptr(stats),
                                              C.byref(r) if rows is not None else None, _ptr(ws), ws.numel(), self._stream()), "sg_ppo_grad_device")
        return out, stats

    def _ppo_batch(self, handle, batch, clip_range, clip_range_vf, ent_coef, vf_coef, coef=False):
        """checks the batch dict and the four host coefficients of ppo_grad_torch / population_ppo_grad_torch; coef: a coefficient
        tensor is given, which makes batch['value'] necessary beside a critic.  Returns (obs, rows, the columns needed beside obs and action)"""
        import math
        import torch
        if not isinstance(batch, dict):
            raise ValueError("batch: expected a dict obs / action / logp / advantage / ret / value of flattened CUDA tensors")
        obs = batch.get("obs")
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or int(obs.shape[0]) < 1:
            raise ValueError(f"batch['obs']: expected a CUDA tensor of shape (rows, {self.obs_dim}) with rows >= 1")
        R = int(obs.shape[0])
        self._check_tensor("batch['obs']", obs, torch.float32, (R, self.obs_dim))
        self._check_tensor("batch['action']", batch.get("action"), torch.int32 if self.discrete else torch.float32, (R,) if self.discrete else (R, 2))
        if not clip_range > 0:
            raise ValueError(f"clip_range: expected a value > 0 (float('inf'): no clipping), got {clip_range}")
        if clip_range_vf is not None and not clip_range_vf > 0:
            raise ValueError(f"clip_range_vf: expected None or a value > 0, got {clip_range_vf}")
        for name, v in (("ent_coef", ent_coef), ("vf_coef", vf_coef)):
            if not v >= 0 or math.isinf(v):
                raise ValueError(f"{name}: expected a finite value >= 0, got {v}")
        value = handle.has_critic and (clip_range_vf is not None or coef)
        need = ["logp", "advantage"] + (["ret"] if handle.has_critic else []) + (["value"] if value else [])
        for k in need:
            if batch.get(k) is None:
                why = " (clip_range_vf is given)" if clip_range_vf is not None else " (coef is given: any member may turn value clipping on)"
                raise ValueError(f"batch['{k}']: missing" + (why if k == "value" else ""))
            self._check_tensor(f"batch['{k}']", batch[k], torch.float32, (R,))
        return obs, R, need

    def _ppo_rows(self, handle, rows, shape, noun):
        """the sg_ppo_rows of the optional per-row outputs, each float32 of `shape`"""
        import torch
        r = _native.SgPpoRows()
        if rows is not None:
            for k, t in rows.items():
                if k not in ("logp", "value", "g_logp", "g_value"):
                    raise ValueError(f"rows['{k}']: expected the keys logp, value, g_logp, g_value")
                if t is None:
                    continue
                if k in ("value", "g_value") and not handle.has_critic:
                    raise ValueError(f"rows['{k}']: the {noun} has no critic")
                self._check_tensor(f"rows['{k}']", t, torch.float32, shape)
                setattr(r, k, t.data_ptr())
        return r

    def _ppo_structs(self, handle, batch, need, index, clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage):
        """(sg_ppo_config, sg_ppo_batch) of a checked call"""
        cfg = _native.SgPpoConfig()
        self._lib.sg_ppo_config_init(C.byref(cfg))
        cfg.clip_range, cfg.clip_range_vf = clip_range, clip_range_vf if clip_range_vf is not None else 0.0
        cfg.ent_coef, cfg.vf_coef, cfg.normalize_advantage = ent_coef, vf_coef, int(bool(normalize_advantage))
        b = _native.SgPpoBatch(obs=batch["obs"].data_ptr(), action=batch["action"].data_ptr(), old_logp=batch["logp"].data_ptr(),
                               advantage=batch["advantage"].data_ptr(), ret=batch["ret"].data_ptr() if handle.has_critic else None,
                               old_value=batch["value"].data_ptr() if "value" in need else None,
                               index=index.data_ptr() if index is not None else None)
        return cfg, b

    @staticmethod
    def ppo_assign_grads(policy, grads):
        """makes ppo_grad_torch's (or policy_grad_torch's) tensors the .grad of the parameters the handle holds, so that optimizer.step()
        follows directly; a net whose gradients are None keeps its .grad"""
        for p, t in zip(policy.tensors, _flat_grads(policy, grads)):
            if t is not None:
                p.grad = t

    # ------------------------------------------------------------------ policy populations: P stacked actor-critics on P env blocks per launch
    def _population(self, pop, per_env=False):
        """checks a policy_population_torch handle; per_env: its members must divide this handle's envs"""
        self._net_handle(pop, PolicyPopulation)
        if per_env and self.num_envs % pop.members:
            raise ValueError(f"pop: {pop.members} members do not divide num_envs = {self.num_envs} (member m owns the envs [m B / P, (m + 1) B / P))")
        return pop.members

    def policy_population_torch(self, members, actor, critic=None, log_std=None, activation="tanh"):
        """A handle on a population of `members` actor-critics of one architecture whose parameters are STACKED along a leading
        dimension, the layout of torch.func.stack_module_state, and stay where they are: actor / critic lists [(weight, bias), ...]
        of contiguous float32 CUDA tensors, weight [P, out, in] and bias [P, out], shapes per member as policy_torch's; log_std
        float32 [P, 2] (continuous ids).  Member m owns the contiguous env block [m B / P, (m + 1) B / P) of the handle's B envs in
        population_act_torch / rollout_population_torch (P must divide B) and rows [m] of the [P, n, ...] tensors of the evaluate
        and grad calls.  A PBT exploit step is W[loser].copy_(W[winner]) on the caller's tensors: the next call reads it
        (adam_exploit_torch does it for all members in one launch and carries the Adam state along)."""
        members = int(members)
        if not 1 <= members <= 65535:
            raise ValueError(f"members must be 1 .. 65535, got {members}")
        if self.num_envs % members:
            raise ValueError(f"members: {members} does not divide num_envs = {self.num_envs}")
        p, keep = self._actor_critic_struct(members, actor, critic, log_std, activation)
        return PolicyPopulation(p, keep, critic is not None, members)

    def population_member_torch(self, pop, m):
        """Member m of a population as a plain policy_torch handle over the views W[m], b[m], log_std[m] of the stacked tensors (no
        copy): to evaluate or export one member with the single-policy calls."""
        members = self._population(pop)
        m = int(m)
        if not 0 <= m < members:
            raise ValueError(f"m: expected a member index 0 .. {members - 1}, got {m}")
        L = pop.n_hidden + 1
        t = pop.tensors
        pairs = lambda ts: [(ts[2 * l][m], ts[2 * l + 1][m]) for l in range(L)]
        return self.policy_torch(actor=pairs(t[:2 * L]), critic=pairs(t[2 * L:4 * L]) if pop.has_critic else None,
                                 log_std=None if self.discrete else t[-1][m], activation=pop.activation)

    def population_act_torch(self, pop, obs, seed=0, step=0, deterministic=False, out=None):
        """policy_act_torch with member i // (B / P) acting for env i, in ONE launch (sg_policy_population_act_device;
        graph-capturable): the same tensors, and per row bit for bit what policy_act_torch gives with that member's handle."""
        import torch
        self._population(pop, per_env=True)
        self._check_tensor("obs", obs, torch.float32, (self.num_envs, self.obs_dim))
        action, logp, value = self._act_out(out, "population", pop.has_critic, obs.device, values_alone=True)
        self._ck(self._lib.sg_policy_population_act_device(self._h, C.byref(pop.struct), pop.members, _ptr(obs), int(seed), int(step),
                                                           int(bool(deterministic)), _ptr(action), _ptr(logp), _ptr(value), self._stream()),
                 "sg_policy_population_act_device")
        return action, logp, value

    def rollout_population_torch(self, pop, obs, action, logp, value, reward, done, trunc, seed=0, first_step=0, deterministic=False,
                                 terminal=None, terminal_value=None):
        """rollout_policy_torch with a population acting (sg_rollout_policy_population_device): the same tensors, bit for bit the loop
        of population_act_torch and step_torch.  terminal: a terminal_list_torch dict, filled like rollout_torch's (observation
        records; no terminal["value"]: a record's member varies).  terminal_value: float32 [K, B], DENSE -- entry (t, i) is V, under
        env i's member, of the last observation of the episode env i finished at step t, and unspecified elsewhere; it is
        gae_torch's terminal_value as it stands:
            env.gae_torch(reward, done, trunc, value[:-1], value[-1], terminal_value=terminal_value)"""
        import torch
        self._population(pop, per_env=True)
        if pop.has_critic and value is None:
            raise ValueError("value: the population has a critic; pass the float32 [K + 1, B] tensor its values go to")
        if not pop.has_critic and (value is not None or terminal_value is not None):
            raise ValueError("value / terminal_value: the population has no critic")
        K = self._rollout_buffers(obs, action, (lambda d: d >= 2, ""), [("logp", logp, 0)] + [("value", value, 1)] * (value is not None), reward,
                                  done, trunc)
        if terminal_value is not None:
            self._check_tensor("terminal_value", terminal_value, torch.float32, (K, self.num_envs))
        self._ck(self._lib.sg_rollout_policy_population_device(
            self._h, K, C.byref(pop.struct), pop.members, int(seed), int(first_step), int(bool(deterministic)), _ptr(obs), _ptr(action),
            _ptr(logp), _ptr(value), _ptr(reward), _ptr(done), _ptr(trunc), self._terminal_list_struct(terminal)[0], _ptr(terminal_value),
            self._stream()), "sg_rollout_policy_population_device")
        return obs, action, logp, value, reward, done, trunc

    def _population_rows(self, pop, obs, action):
        """checks (pop, obs [P, n, D], action [P, n, 2] or int32 [P, n]) and returns (P, n)"""
        import torch
        P = self._population(pop)
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or int(obs.shape[1]) < 1:
            raise ValueError(f"obs: expected a CUDA tensor of shape ({P}, n, {self.obs_dim}) with n >= 1")
        n = int(obs.shape[1])
        self._check_tensor("obs", obs, torch.float32, (P, n, self.obs_dim))
        self._check_tensor("action", action, torch.int32 if self.discrete else torch.float32, (P, n) if self.discrete else (P, n, 2))
        return P, n

    def population_evaluate_raw_torch(self, pop, obs, action, out=None):
        """policy_evaluate_raw_torch for every member on its own n rows in ONE launch (sg_policy_population_evaluate_device): obs
        float32 [P, n, D], action float32 [P, n, 2] (discrete ids: int32 [P, n]) -> (logp, entropy, value) float32 [P, n]; row [m] is
        bit for bit policy_evaluate_raw_torch(population_member_torch(pop, m), obs[m], action[m]).  out as there."""
        import torch
        P, n = self._population_rows(pop, obs, action)
        if out is None:
            out = {k: torch.empty((P, n), dtype=torch.float32, device=obs.device) for k in (("logp", "entropy", "value") if pop.has_critic else ("logp", "entropy"))}
        elif out.get("value") is not None and not pop.has_critic:
            raise ValueError("out['value']: the population has no critic")
        cols = self._out_columns(out, [(k, torch.float32, (P, n)) for k in ("logp", "entropy", "value")])
        self._ck(self._lib.sg_policy_population_evaluate_device(self._h, C.byref(pop.struct), P, n, _ptr(obs), _ptr(action), *map(_ptr, cols),
                                                                self._stream()), "sg_policy_population_evaluate_device")
        return cols

    def population_grad_torch(self, pop, obs, action, g_logp=None, g_entropy=None, g_value=None, out=None):
        """policy_grad_torch for every member on its own n rows (sg_policy_population_grad_device: two launches, graph-capturable
        after one warm-up call with the same n): g_* float32 [P, n] (None: zeros) -> a dict actor / critic / log_std as
        policy_grad_torch's, of STACKED gradient tensors of the parameters' shapes, WRITTEN, not accumulated.  Member m's slices are bit
        for bit policy_grad_torch's for the same rows with member m's handle while ceil(n / R) <= 256 // P (R = 256, 128 or 64 rows
        by the hidden width); beyond that they are the same sums in another grouping.  Same inputs and same n: the same bits."""
        import torch
        P, n = self._population_rows(pop, obs, action)
        for name, g in (("g_logp", g_logp), ("g_entropy", g_entropy), ("g_value", g_value)):
            if g is not None:
                self._check_tensor(name, g, torch.float32, (P, n))
        if g_value is not None and not pop.has_critic:
            raise ValueError("g_value: the population has no critic")
        out, g = self._policy_grads(pop, out, "population", g_value is not None, "g_value is given; the critic's gradients need tensors")
        ws = self._grad_workspace(pop, "sg_policy_population_grad_workspace_bytes", n, obs.device, "population_grad_torch",
                                  "sg_policy_population_grad_workspace_bytes", members=P)
        self._ck(self._lib.sg_policy_population_grad_device(self._h, C.byref(pop.struct), P, n, _ptr(obs), _ptr(action), _ptr(g_logp), _ptr(g_entropy),
                                                            _ptr(g_value), C.byref(g), _ptr(ws), ws.numel(), self._stream()),
                 "sg_policy_population_grad_device")
        return out

    ppo_coef_names = ("clip_range", "clip_range_vf", "ent_coef", "vf_coef")  # the columns of population_ppo_grad_torch's coef [P, 4]

    def population_ppo_grad_torch(self, pop, batch, index=None, coef=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5,
                                  normalize_advantage=True, out=None, stats=None, rows=None):
        """ppo_grad_torch for every member of a population in one call (sg_ppo_population_grad_device: two or three launches, no host
        synchronisation, graph-capturable after one warm-up call with the same n).  batch: ppo_grad_torch's dict, ONE flattened
        rollout of `rows` rows shared by all members (the [K, B] buffers of rollout_population_torch and gae_torch, reshaped).  index:
        int64 [P, n], entry (m, i) the row member m's minibatch entry i reads -- the gather puts a member's env block into its
        minibatch; repeats allowed, an entry outside [0, rows) handled as ppo_grad_torch's; None: member m takes rows [m n, (m + 1) n),
        n = rows // P.  coef: optional float32 CUDA tensor [P, 4] of per-member (clip_range, clip_range_vf, ent_coef, vf_coef), the
        columns named by ppo_coef_names; given, it replaces the four scalars for every member and is READ ON THE DEVICE at every
        call or graph replay; its values are not checked (clip_range_vf <= 0 or NaN: no value clipping for that member; a value the
        scalars would be refused for affects that member's outputs only), and with a critic batch['value'] is needed.  The scalars
        are checked as ppo_grad_torch checks them.  Returns (grads, stats): grads the dict of STACKED tensors population_grad_torch
        returns, written; stats float32 [P, 12] named by ppo_stats_names.  rows: optional dict logp / value / g_logp / g_value of
        float32 [P, n].  Member m's slices, statistics and rows are bit for bit ppo_grad_torch's on population_member_torch(pop, m)
        with index[m] and member m's coefficients while ceil(n / R) <= 256 // P (R = 256, 128 or 64 by the hidden width) and
        ceil(n / 1024) <= 256 // P; beyond that the same sums in another grouping.  Same inputs and same n: the same bits."""
        import torch
        P = self._population(pop)
        if coef is not None:
            self._check_tensor("coef", coef, torch.float32, (P, len(self.ppo_coef_names)))
        obs, R, need = self._ppo_batch(pop, batch, clip_range, clip_range_vf, ent_coef, vf_coef, coef=coef is not None)
        if index is None:
            n = R // P
            if n < 1:
                raise ValueError(f"index: None gives member m the rows [m n, (m + 1) n), but the batch holds {R} rows for {P} members")
        else:
            if not isinstance(index, torch.Tensor) or index.dim() != 2 or int(index.shape[0]) != P or int(index.shape[1]) < 1:
                raise ValueError(f"index: expected an int64 CUDA tensor of shape ({P}, n) with n >= 1")
            n = int(index.shape[1])
            self._check_tensor("index", index, torch.int64, (P, n))
        if normalize_advantage and n < 2:
            raise ValueError("normalize_advantage: needs n >= 2")
        out, g = self._policy_grads(pop, out, "population", pop.has_critic, "the population has a critic; its gradients need tensors")
        if stats is None:
            stats = obs.new_empty((P, len(self.ppo_stats_names)))
        else:
            self._check_tensor("stats", stats, torch.float32, (P, len(self.ppo_stats_names)))
        r = self._ppo_rows(pop, rows, (P, n), "population")
        cfg, b = self._ppo_structs(pop, batch, need, index, clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage)
        ws = self._grad_workspace(pop, "sg_ppo_population_grad_workspace_bytes", n, obs.device, "population_ppo_grad_torch",
                                  "sg_ppo_population_grad_workspace_bytes", members=P)
        self._ck(self._lib.sg_ppo_population_grad_device(self._h, C.byref(pop.struct), P, C.byref(cfg), C.byref(b), _ptr(coef), R, n, C.byref(g),
                                                         _ptr(stats), C.byref(r) if rows is not None else None, _ptr(ws), ws.numel(),
                                                         self._stream()), "sg_ppo_population_grad_device")
        return out, stats

    # ------------------------------------------------------------------ the parameter update: per-member Adam with clipping, PBT exploit
    adam_hyper_names = ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm", "reserved", "reserved")  # AdamState.hyper [P, 8]
    adam_state_names = ("steps", "beta1_pow", "beta2_pow", "skipped", "grad_norm", "clip_scale", "step_size", "applied")  # AdamState.state [P, 8]

    def adam_torch(self, handle, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        """The optimizer state of adam_step_torch over handle.tensors: any handle of policy_torch, q_torch, squashed_policy_torch or
        dqn_torch (P = 1) or of policy_population_torch (P = members).  Every hyperparameter is a scalar or a length-P sequence:
        member m steps with its own learning rate, betas, eps, decoupled weight_decay (AdamW; 0 is Adam) and max_grad_norm (the
        member's global-norm clip over all its gradients; None, inf or 0: off).  They are checked here; AdamState.hyper is READ ON THE
        DEVICE at every call or graph replay, its later contents are not checked, and a bad value affects that member only -- PBT's
        explore step, or a learning-rate schedule, is a write to that tensor.  The moments start at zero."""
        import torch
        if type(handle) not in _NET_HANDLES:
            raise ValueError("handle: expected a handle of policy_torch, q_torch, squashed_policy_torch, dqn_torch or policy_population_torch")
        P = handle.members if isinstance(handle, PolicyPopulation) else 1
        for i, t in enumerate(handle.tensors):
            self._check_tensor(f"handle.tensors[{i}]", t, torch.float32, t.shape)
        hyper = np.zeros((P, len(self.adam_hyper_names)), np.float32)
        betas = tuple(betas)
        if len(betas) != 2:
            raise ValueError("betas: expected (beta1, beta2)")
        ok = {"lr": lambda v: np.isfinite(v) & (v >= 0), "beta1": lambda v: (v >= 0) & (v < 1), "beta2": lambda v: (v >= 0) & (v < 1),
              "eps": lambda v: np.isfinite(v) & (v >= 0), "weight_decay": lambda v: np.isfinite(v) & (v >= 0), "max_grad_norm": lambda v: v >= 0}
        scalar = max_grad_norm is None or np.ndim(max_grad_norm) == 0
        clip = [float("inf") if x is None else x for x in ([max_grad_norm] if scalar else max_grad_norm)]  # (None: off, also inside a sequence)
        given = (lr, betas[0], betas[1], eps, weight_decay, clip[0] if scalar else clip)
        for c, (name, v) in enumerate(zip(self.adam_hyper_names, given)):
            v = np.asarray(v, np.float64)
            if v.shape not in ((), (P,)):
                raise ValueError(f"{name}: expected a scalar or a sequence of {P} (one per member), got shape {v.shape}")
            if not np.all(ok[name](v)):
                raise ValueError(f"{name}: " + {"lr": "expected finite values >= 0", "beta1": "expected values in [0, 1)", "beta2": "expected values in [0, 1)",
                                                "eps": "expected finite values >= 0", "weight_decay": "expected finite values >= 0",
                                                "max_grad_norm": "expected values >= 0 (None, inf or 0: no clipping)"}[name] + f", got {v.tolist()}")
            hyper[:, c] = v
        dev = handle.tensors[0].device
        state = np.zeros((P, len(self.adam_state_names)), np.float64)
        state[:, 1:3] = 1.0
        return AdamState(handle, P, torch.from_numpy(hyper).to(dev), torch.from_numpy(state).to(dev),
                         tuple(torch.zeros_like(t) for t in handle.tensors), tuple(torch.zeros_like(t) for t in handle.tensors))

    def _adam_state(self, opt):
        if not isinstance(opt, AdamState):
            raise ValueError("opt: expected the AdamState adam_torch returns")
        import torch
        self._check_tensor("opt.hyper", opt.hyper, torch.float32, (opt.members, len(self.adam_hyper_names)))
        self._check_tensor("opt.state", opt.state, torch.float64, (opt.members, len(self.adam_state_names)))
        return opt.members

    def _adam_table(self, opt, flat):
        """the sg_adam_tensor table over the handle's tensors whose entry of `flat` is not None (flat None: all of them, without
        gradients), kept on the AdamState while the pointers stay the same"""
        params = opt.handle.tensors
        key = tuple(t.data_ptr() for t in (*params, *opt.exp_avg, *opt.exp_avg_sq)) + (
            None if flat is None else tuple(None if g is None else g.data_ptr() for g in flat),)
        if opt._table is None or opt._table[0] != key:
            use = [k for k in range(len(params)) if flat is None or flat[k] is not None]
            tab = (_native.SgAdamTensor * len(use))()
            for row, k in zip(tab, use):
                row.param, row.grad = params[k].data_ptr(), None if flat is None else flat[k].data_ptr()
                row.exp_avg, row.exp_avg_sq = opt.exp_avg[k].data_ptr(), opt.exp_avg_sq[k].data_ptr()
                row.numel = params[k].numel() // opt.members
            opt._table = (key, tab)
        return opt._table[1]

    def adam_step_torch(self, opt, grads):
        """One Adam / AdamW step of every member with its own row of opt.hyper (sg_adam_step_device: two launches, no host
        synchronisation, nothing allocated, graph-capturable).  grads: the dict policy_grad_torch, ppo_grad_torch,
        population_ppo_grad_torch, q_grad_torch, squashed_grad_torch or dqn_grad_torch returns; its tensors are read, never written.
        A net whose gradients are None (a frozen critic) stays out of the norm and of the update.  Per member: the float32 l2 norm
        over ALL its gradient elements, torch's clip_grad_norm_ coefficient for its max_grad_norm, and the update in float32 with
        bias corrections from running beta products; a member whose norm is not finite is skipped and counted, the others step.
        opt.state's columns (adam_state_names) report per member what the call used.  tests/adam_model.py is the arithmetic, bit for
        bit.  Returns opt.state."""
        import torch
        P = self._adam_state(opt)
        params = opt.handle.tensors
        flat = list(_flat_grads(opt.handle, grads))
        flat += [None] * (len(params) - len(flat))
        if len(flat) != len(params):
            raise ValueError(f"grads: {len(flat)} gradient tensors for the handle's {len(params)} parameter tensors")
        if all(g is None for g in flat):
            raise ValueError("grads: no tensor has a gradient")
        for k, g in enumerate(flat):
            if g is not None:
                self._check_tensor(f"grads (tensor {k})", g, torch.float32, params[k].shape)
        tab = self._adam_table(opt, flat)
        self._ck(self._lib.sg_adam_step_device(self._h, P, len(tab), tab, _ptr(opt.hyper), _ptr(opt.state), self._stream()), "sg_adam_step_device")
        return opt.state

    def adam_exploit_torch(self, opt, src, refused=None):
        """PBT's exploit step with the optimizer state carried along (sg_adam_exploit_device: one launch, graph-capturable).  src: int32
        CUDA tensor [P]; for every m with src[m] != m, member m's parameters, both moments and its steps, beta powers and skipped count
        become member src[m]'s.  opt.hyper is not touched: explore is the caller's write.  A copy is performed only if its source is not
        itself a destination (src[src[m]] == src[m]) -- truncation selection always satisfies that -- and is in [0, P); the others are
        not performed and are counted in refused (int32 CUDA tensor [1], written; optional)."""
        import torch
        P = self._adam_state(opt)
        self._check_tensor("src", src, torch.int32, (P,))
        if refused is not None:
            self._check_tensor("refused", refused, torch.int32, (1,))
        tab = self._adam_table(opt, None)
        self._ck(self._lib.sg_adam_exploit_device(self._h, P, len(tab), tab, _ptr(opt.state), _ptr(src), _ptr(refused), self._stream()),
                 "sg_adam_exploit_device")
        return refused

    # ------------------------------------------------------------------ the rest of a PBT generation: member fitness, selection, explore
    pbt_fitness_names = ("episodes", "return_sum", "length_sum", "return_sq_sum", "return_max", "return_min", "fitness", "reserved")  # PbtFitness.table [P, 8]
    pbt_max_members, pbt_max_columns = 256, 16
    pbt_modes = {"copy": 0, "scale": 1, "scale_complement": 2}  # SG_PBT_COPY / SG_PBT_SCALE / SG_PBT_SCALE_COMPLEMENT

    def _pbt_members(self, members, divide=False):
        members = int(members)
        if not 1 <= members <= self.pbt_max_members:
            raise ValueError(f"members must be 1 .. {self.pbt_max_members}, got {members}")
        if divide and self.num_envs % members:
            raise ValueError(f"members: {members} does not divide num_envs = {self.num_envs} (member m owns the envs [m B / P, (m + 1) B / P))")
        return members

    def _pbt_fitness(self, fit):
        import torch
        if not isinstance(fit, PbtFitness):
            raise ValueError("fit: expected the PbtFitness pbt_fitness_torch returns")
        P = self._pbt_members(fit.members, divide=True)
        self._check_tensor("fit.env_return", fit.env_return, torch.float64, (self.num_envs,))
        self._check_tensor("fit.env_length", fit.env_length, torch.int32, (self.num_envs,))
        self._check_tensor("fit.table", fit.table, torch.float64, (P, len(self.pbt_fitness_names)))
        return P

    def _pbt_step_dev(self, step_dev):
        import torch
        if step_dev is not None:
            self._check_tensor("step_dev", step_dev, torch.int64, (1,))
        return _ptr(step_dev)

    def pbt_fitness_torch(self, members):
        """The fitness state of a population of `members` = P (1 .. 256, dividing num_envs; member m owns the envs
        [m B / P, (m + 1) B / P), as in rollout_population_torch): zero running returns and lengths, a cleared table, the workspace."""
        import torch
        P = self._pbt_members(members, divide=True)
        need = int(self._lib.sg_pbt_fitness_workspace_bytes(self._h, P))
        if need == 0:
            self._ck(-1, "sg_pbt_fitness_workspace_bytes")
        dev = torch.device("cuda", self.device)
        table = torch.zeros((P, len(self.pbt_fitness_names)), dtype=torch.float64, device=dev)
        table[:, 4], table[:, 5], table[:, 6] = float("-inf"), float("inf"), float("nan")
        return PbtFitness(P, torch.zeros(self.num_envs, dtype=torch.float64, device=dev), torch.zeros(self.num_envs, dtype=torch.int32, device=dev),
                          table, torch.empty(need // 8, dtype=torch.float64, device=dev))

    def pbt_fitness_update_torch(self, fit, reward, done):
        """Adds the episodes that finished inside the rows reward float32 [K, B], done uint8 / bool [K, B] (any K >= 1; as a rollout
        wrote them, truncations included) to every member's row of fit.table, and carries every env's unfinished episode on in
        fit.env_return / fit.env_length, so that episodes span calls (sg_pbt_fitness_device: two launches, no host synchronisation,
        nothing allocated, graph-capturable).  Returns in float64, summed in a fixed order that depends on (B, P) only;
        fitness = return_sum / episodes, NaN while a member has finished no episode.  tests/pbt_model.py is the arithmetic, bit for
        bit.  The values of reward are not checked: a NaN stays within its env's member.  Returns fit.table."""
        import torch
        P = self._pbt_fitness(fit)
        if not (isinstance(reward, torch.Tensor) and reward.dim() == 2 and reward.shape[0] >= 1):
            raise ValueError("reward: expected a float32 CUDA tensor [K, num_envs] with K >= 1")
        K = int(reward.shape[0])
        self._check_tensor("reward", reward, torch.float32, (K, self.num_envs))
        if isinstance(done, torch.Tensor) and done.dtype == torch.bool:
            done = done.view(torch.uint8)  # (same bytes: no copy)
        self._check_tensor("done", done, torch.uint8, (K, self.num_envs))
        ws = fit.workspace
        if not (isinstance(ws, torch.Tensor) and ws.dtype == torch.float64 and ws.dim() == 1):
            raise ValueError("fit.workspace: expected the float64 tensor pbt_fitness_torch made")
        self._check_tensor("fit.workspace", ws, torch.float64, ws.shape)
        self._ck(self._lib.sg_pbt_fitness_device(self._h, P, K, _ptr(reward), _ptr(done), _ptr(fit.env_return), _ptr(fit.env_length),
                                                 _ptr(fit.table), _ptr(ws), ws.numel() * 8, self._stream()), "sg_pbt_fitness_device")
        return fit.table

    def pbt_fitness_clear_torch(self, fit, src=None):
        """Starts a new fitness window: table rows back to the identities and fitness to NaN (sg_pbt_fitness_clear_device: one launch,
        graph-capturable).  src None: every row; src (int32 [P], as pbt_select_torch wrote it): the rows of the members that were
        replaced, src[m] != m.  The running returns of unfinished episodes are left alone.  Returns fit.table."""
        import torch
        P = self._pbt_fitness(fit)
        if src is not None:
            self._check_tensor("src", src, torch.int32, (P,))
        self._ck(self._lib.sg_pbt_fitness_clear_device(self._h, P, _ptr(fit.table), _ptr(src), self._stream()), "sg_pbt_fitness_clear_device")
        return fit.table

    def pbt_select_torch(self, fitness, ready=None, fraction=0.2, seed=0, step=0, step_dev=None, out=None, rank=None, count=None):
        """Truncation selection on the device (sg_pbt_select_device: one launch, graph-capturable): src int32 [P] for
        adam_exploit_torch, pbt_explore_torch and pbt_fitness_clear_torch.  fitness: float64 CUDA tensor [P], possibly a strided view
        such as fit.table[:, 6]; ready: uint8 / bool [P], optional.  Member m takes part iff it is ready and its fitness is not NaN;
        with r taking part and k_eff = min(floor(fraction P), r // 2), each of the k_eff worst draws one of the k_eff best (ties go to
        the lower index; Philox keyed by seed, counter (m, step)) and every other member keeps itself, so src[src[m]] == src[m].
        step_dev: int64 CUDA tensor [1] added to step on the device -- bump it inside a captured graph and every replay draws afresh.
        rank: int32 [P], receives every member's rank (-1: not taking part); count: int32 [2], receives (copies, k_eff).  Returns src
        (`out` if given)."""
        import torch
        if not (isinstance(fitness, torch.Tensor) and fitness.dim() == 1 and fitness.dtype == torch.float64):
            raise ValueError("fitness: expected a float64 CUDA tensor [members] (a strided view such as fit.table[:, 6] will do)")
        P = self._pbt_members(fitness.shape[0])
        if not (fitness.is_cuda and fitness.device.index == self.device):
            raise ValueError(f"fitness: expected a CUDA tensor on device {self.device}")
        stride = int(fitness.stride(0)) if P > 1 else 1
        if stride < 1:
            raise ValueError(f"fitness: expected a positive stride, got {stride}")
        if ready is not None:
            if isinstance(ready, torch.Tensor) and ready.dtype == torch.bool:
                ready = ready.view(torch.uint8)
            self._check_tensor("ready", ready, torch.uint8, (P,))
        fraction = float(fraction)
        if not 0.0 < fraction <= 0.5:
            raise ValueError(f"fraction: expected a value in (0, 0.5], got {fraction}")
        ptr_step = self._pbt_step_dev(step_dev)
        for name, t, n in (("out", out, P), ("rank", rank, P), ("count", count, 2)):
            if t is not None:
                self._check_tensor(name, t, torch.int32, (n,))
        src = torch.empty(P, dtype=torch.int32, device=fitness.device) if out is None else out
        self._ck(self._lib.sg_pbt_select_device(self._h, P, _ptr(fitness), stride, _ptr(ready), int(math.floor(fraction * P)), int(seed), int(step),
                                                ptr_step, _ptr(src), _ptr(rank), _ptr(count), self._stream()), "sg_pbt_select_device")
        return src

    def pbt_explore_torch(self, src, columns, seed=0, step=0, step_dev=None, refused=None):
        """PBT's explore step on the device (sg_pbt_explore_device: one launch, graph-capturable).  columns: up to 16 entries
        (tensor, column, spec): tensor a float32 CUDA tensor [P, C] -- opt.hyper, a population_ppo_grad_torch coef, gae_groups_torch's
        discounts with one group per member, or any tensor of the caller's; spec = dict(mode=, down=0.8, up=1.25, lo=-inf, hi=inf).
        For every member m that src lets copy (src[m] != m, in range, and its source not a destination) and every column, the
        source's value v becomes, by mode: "copy" v; "scale" v f; "scale_complement" 1 - (1 - v) f (gamma, lambda, beta); f is `up`
        or `down` by one Philox bit of (seed, step, column's position, m); then it is clamped to [lo, hi] and stored in m's row.  Other
        members keep their bits.  Copies the rule refuses are counted in refused (int32 [1], optional).  Returns refused."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.dim() == 1):
            raise ValueError("src: expected an int32 CUDA tensor [members]")
        P = self._pbt_members(src.shape[0])
        self._check_tensor("src", src, torch.int32, (P,))
        columns = list(columns)
        if not 1 <= len(columns) <= self.pbt_max_columns:
            raise ValueError(f"columns: expected 1 .. {self.pbt_max_columns} entries, got {len(columns)}")
        tab = (_native.SgPbtColumn * len(columns))()
        for i, (row, entry) in enumerate(zip(tab, columns)):
            try:
                t, col, spec = entry
                spec = dict(spec)
            except (TypeError, ValueError):
                raise ValueError(f"columns[{i}]: expected (tensor, column, spec) with spec a dict") from None
            if not (isinstance(t, torch.Tensor) and t.dim() == 2):
                raise ValueError(f"columns[{i}]: expected a float32 CUDA tensor [{P}, C]")
            self._check_tensor(f"columns[{i}] tensor", t, torch.float32, (P, t.shape[1]))
            if not (isinstance(col, (int, np.integer)) and 0 <= col < t.shape[1]):
                raise ValueError(f"columns[{i}]: column {col!r} outside the tensor's 0 .. {t.shape[1] - 1}")
            unknown = set(spec) - {"mode", "down", "up", "lo", "hi"}
            if unknown or "mode" not in spec:
                raise ValueError(f"columns[{i}]: spec takes mode (required), down, up, lo, hi" + (f"; got {sorted(unknown)}" if unknown else ""))
            mode = self.pbt_modes.get(spec["mode"], spec["mode"]) if isinstance(spec["mode"], str) else spec["mode"]
            if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or int(mode) not in self.pbt_modes.values():
                raise ValueError(f"columns[{i}]: unknown mode {spec['mode']!r}; expected one of {sorted(self.pbt_modes)}")
            down, up = float(spec.get("down", 0.8)), float(spec.get("up", 1.25))
            lo, hi = float(spec.get("lo", float("-inf"))), float(spec.get("hi", float("inf")))
            if any(math.isnan(x) for x in (down, up, lo, hi)):
                raise ValueError(f"columns[{i}]: down, up, lo and hi must not be NaN")
            if lo > hi:
                raise ValueError(f"columns[{i}]: lo = {lo} above hi = {hi}")
            row.data, row.stride, row.mode = t.data_ptr() + 4 * int(col), int(t.shape[1]), int(mode)
            row.down, row.up, row.lo, row.hi = down, up, lo, hi
        ptr_step = self._pbt_step_dev(step_dev)
        if refused is not None:
            self._check_tensor("refused", refused, torch.int32, (1,))
        self._ck(self._lib.sg_pbt_explore_device(self._h, P, _ptr(src), len(tab), tab, int(seed), int(step), ptr_step, _ptr(refused), self._stream()),
                 "sg_pbt_explore_device")
        return refused

    # ------------------------------------------------------------------ shuffled minibatch indices drawn on the device; the whole PPO update in one call
    minibatch_units = {"row": 0, "env": 1}  # SG_MINIBATCH_ROW / SG_MINIBATCH_ENV
    minibatch_max_members, minibatch_max_epochs = 256, 64

    def _minibatch_shape(self, steps, members, epochs, minibatches, unit):
        """checks the arguments of minibatch_index_torch and returns (K, P, epochs, M, unit's number, n)"""
        ints = {}
        for name, v in (("steps", steps), ("members", 1 if members is None else members), ("epochs", epochs), ("minibatches", minibatches)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name}: expected an integer, got {v!r}")
            ints[name] = int(v)
        K, P, epochs, M = ints["steps"], ints["members"], ints["epochs"], ints["minibatches"]
        if K < 1:
            raise ValueError(f"steps must be at least 1, got {K}")
        if not 1 <= P <= self.minibatch_max_members:
            raise ValueError(f"members must be 1 .. {self.minibatch_max_members}, got {P}")
        if self.num_envs % P:
            raise ValueError(f"members: {P} does not divide num_envs = {self.num_envs} (member m owns the envs [m B / P, (m + 1) B / P))")
        if not 1 <= epochs <= self.minibatch_max_epochs:
            raise ValueError(f"epochs must be 1 .. {self.minibatch_max_epochs}, got {epochs}")
        if M < 1:
            raise ValueError(f"minibatches must be at least 1, got {M}")
        u = self.minibatch_units.get(unit) if isinstance(unit, str) else unit
        if isinstance(u, bool) or not isinstance(u, (int, np.integer)) or int(u) not in self.minibatch_units.values():
            raise ValueError(f"unit: unknown unit {unit!r}; expected one of {sorted(self.minibatch_units)}")
        if K * self.num_envs >= 2 ** 31:
            raise ValueError(f"steps: {K} steps of {self.num_envs} envs are 2^31 rows or more")
        E = self.num_envs // P
        n = (K * E) // M if int(u) == 0 else K * (E // M)
        if n < 1:
            raise ValueError(f"minibatches: {M} minibatches of a member's {K * E if int(u) == 0 else E} {'rows' if int(u) == 0 else 'envs'} "
                             "leave none for a minibatch")
        return K, P, epochs, M, int(u), n

    def minibatch_index_torch(self, steps, members=None, epochs=1, minibatches=1, unit="row", seed=0, step=0, step_dev=None, out=None):
        """Shuffled minibatch indices of an on-policy update, drawn on the device (sg_minibatch_index_device: one launch, no sort, no
        workspace, no host synchronisation, graph-capturable): int64 [epochs, M, P, n] over the rows t B + i of a flattened rollout of
        `steps` = K rows; every index[e, b] is the [P, n] index of population_ppo_grad_torch, inside member m's env block
        [m B / P, (m + 1) B / P) for row m.  members None: one policy, the result is [epochs, M, n] and index[e, b] is ppo_grad_torch's
        [n].  unit "row": a member's K B / P rows are shuffled afresh per epoch and cut into M minibatches of n = (K B / P) // M (the
        fewer than M rows left over are another set in every epoch); unit "env": its B / P env columns are shuffled and a minibatch holds
        c = (B / P) // M whole columns, n = K c, index[e, b, m] a time-major [K, c] view.  Within one (epoch, member) no row repeats.
        An index is a pure function of (seed, step + step_dev, epoch, member, position) -- a keyed bijection, tests/minibatch_model.py;
        uniform in single positions and pairs, not over all orders.  step_dev: int64 CUDA tensor [1] added to step on the device -- bump
        it inside a captured graph and every replay shuffles afresh.  out: the tensor to fill.  Returns the index."""
        import torch
        K, P, epochs, M, u, n = self._minibatch_shape(steps, members, epochs, minibatches, unit)
        shape = (epochs, M, n) if members is None else (epochs, M, P, n)
        ptr_step = self._pbt_step_dev(step_dev)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=torch.device("cuda", self.device))
        else:
            self._check_tensor("out", out, torch.int64, shape)
        self._ck(self._lib.sg_minibatch_index_device(self._h, K, P, epochs, M, u, int(seed), int(step), ptr_step, _ptr(out), self._stream()),
                 "sg_minibatch_index_device")
        return out

    def ppo_update_torch(self, handle, opt, batch, steps, epochs, minibatches, unit="row", seed=0, step=0, step_dev=None, coef=None,
                         clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, index=None, stats=None,
                         grads=None):
        """The whole PPO update of one rollout in one call: epochs x minibatches times (shuffled index, gradient, Adam step).  A
        COMPOSITION OF EXISTING ENTRY POINTS THAT ADDS NO NATIVE CODE: one minibatch_index_torch call, then for every (e, b)
        ppo_grad_torch (handle a policy_torch handle) or population_ppo_grad_torch (a policy_population_torch handle, with coef) with
        index[e, b], out=grads and stats=stats[e, b], followed by adam_step_torch(opt, grads).  No host synchronisation; graph-capturable
        after one warm-up call, as the calls it makes are.  batch: ppo_grad_torch's dict over the steps * num_envs rows of the flattened
        rollout; opt: adam_torch's state of `handle`; steps, epochs, minibatches, unit, seed, step, step_dev: minibatch_index_torch's;
        the loss keywords: ppo_grad_torch's.  index / stats / grads: the tensors to fill (int64 [epochs, M, (P,) n]; float32
        [epochs, M, (P,) 12]; a gradient dict), made when None.  Returns (stats, index)."""
        import torch
        pop = isinstance(handle, PolicyPopulation)
        if not pop:
            self._net_handle(handle, Policy)
            if coef is not None:
                raise ValueError("coef: per-member coefficients belong to a population; pass the four scalars")
        P = self._population(handle, per_env=True) if pop else None
        if coef is not None:
            self._check_tensor("coef", coef, torch.float32, (P, len(self.ppo_coef_names)))
        if not isinstance(opt, AdamState) or opt.handle is not handle:
            raise ValueError("opt: expected the AdamState adam_torch returned for this handle")
        K, _, epochs, M, _, n = self._minibatch_shape(steps, P, epochs, minibatches, unit)
        obs, R, _ = self._ppo_batch(handle, batch, clip_range, clip_range_vf, ent_coef, vf_coef, coef=coef is not None)
        if R != K * self.num_envs:
            raise ValueError(f"batch: {R} rows, but steps * num_envs = {K * self.num_envs}")
        lead = (epochs, M, P) if pop else (epochs, M)
        if stats is None:
            stats = obs.new_empty((*lead, len(self.ppo_stats_names)))
        else:
            self._check_tensor("stats", stats, torch.float32, (*lead, len(self.ppo_stats_names)))
        index = self.minibatch_index_torch(K, P, epochs, M, unit, seed, step, step_dev, out=index)
        loss = dict(clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage)
        for e in range(epochs):
            for b in range(M):
                if pop:
                    grads, _ = self.population_ppo_grad_torch(handle, batch, index[e, b], coef=coef, out=grads, stats=stats[e, b], **loss)
                else:
                    grads, _ = self.ppo_grad_torch(handle, batch, index[e, b], out=grads, stats=stats[e, b], **loss)
                self.adam_step_torch(opt, grads)
        return stats, index

    def population_evaluate_torch(self, pop, obs, action):
        """logp, entropy, value, each [P, n], of the stored rows under the CURRENT parameters, differentiable with respect to the
        stacked tensors the handle holds: ONE torch.autograd.Function over population_evaluate_raw_torch whose backward is one
        population_grad_torch call (a None g for an output the loss did not use).  A loss summed over the members' losses gives every
        member its own gradient in its slices; .grad accumulates as usual.  value is None without a critic."""
        self._population_rows(pop, obs, action)
        fn = _net_function("PopulationEvaluate", lambda env, h, o, a: env.population_evaluate_raw_torch(h, o, a), _actor_critic_backward("population_grad_torch", True))
        return fn.apply(self, pop, obs, action, *pop.tensors)

    # ------------------------------------------------------------------ the off-policy learner's nets: twin Q critics, action gradients
    def q_torch(self, critics, activation="relu"):
        """A handle on one or two Q critics whose parameters stay where they are (sg_qnet: no copy, no transpose; a target network
        is a second handle).  critics: a list of one or two nets, each a list [(weight, bias), ...] of float32 CUDA tensors in
        torch.nn.Linear layout -- obs_dim + 2 -> hidden (1 .. 3 layers of one width 1 .. 128) -> 1, on the row [obs | action].
        Continuous ids only.  The action is used as given: nothing clamps it."""
        if self.discrete:
            raise ValueError("q_torch: the Q critics take the continuous ids' 2-vector action; the discrete ids are not served "
                             "(their Q head is dqn_torch's Q(obs) -> 6)")
        code = _activation_code(activation)
        critics = [list(c) for c in critics]
        if not 1 <= len(critics) <= 2:
            raise ValueError(f"critics: expected one or two nets, got {len(critics)}")
        q = _native.SgQnet(struct_size=C.sizeof(_native.SgQnet), n_critics=len(critics), activation=code)
        keep = []
        shapes = [self._mlp_layers(f"critics[{c}]", layers, self.obs_dim + 2, 1, q.critic[c], keep) for c, layers in enumerate(critics)]
        if len(set(shapes)) != 1:
            raise ValueError(f"critics[1]: expected {shapes[0][0]} hidden layers of width {shapes[0][1]}, like critics[0]")
        q.n_hidden, q.hidden = shapes[0]
        return QNet(q, keep)

    def q_evaluate_raw_torch(self, q, obs, action, out=None):
        """(q1, q2) float32 [n] of the rows obs float32 [n, D], action float32 [n, 2] under a q_torch handle; q2 is None with one
        critic.  One launch on torch's current stream, no host synchronisation, no autograd (sg_q_evaluate_device; graph-capturable).
        out: dict q1 / q2 of tensors to fill (allocated when None; an entry that is absent or None is not computed)."""
        import torch
        n = self._net_rows(q, QNet, obs, action=action)
        if out is None:
            out = {k: torch.empty(n, dtype=torch.float32, device=obs.device) for k in ("q1", "q2")[:q.n_critics]}
        elif out.get("q2") is not None and q.n_critics != 2:
            raise ValueError("out['q2']: the handle has one critic")
        q1, q2 = self._out_columns(out, [(k, torch.float32, (n,)) for k in ("q1", "q2")])
        self._ck(self._lib.sg_q_evaluate_device(self._h, C.byref(q.struct), n, _ptr(obs), _ptr(action), _ptr(q1), _ptr(q2), self._stream()),
                 "sg_q_evaluate_device")
        return q1, q2

    def q_grad_torch(self, q, obs, action, g_q1=None, g_q2=None, params=True, action_grad=False, out=None):
        """The critics' half of a backward pass, given the loss's gradients g_q1 / g_q2 (float32 [n], None: zeros) by
        q_evaluate_raw_torch's outputs at the same (obs, action): sg_q_grad_device on torch's current stream, the forward pass
        recomputed inside.  Returns dict critics / action:
          critics  (params) per critic the list of (weight, bias) gradients, WRITTEN, not accumulated (zeros for a critic whose g is
                   None); None with params=False: the critics are frozen, no weight-gradient work is done
          action   (action_grad) float32 [n, 2] = sum_c g_qc[i] dQ_c[i] / d action[i]: per row, the same bits for any n and for
                   params on or off; None otherwise
        out: such a dict of tensors to fill.  With params the call is graph-capturable after one warm-up call with the same n (which
        sizes the workspace kept on the handle).  Same inputs and same n: the same bits."""
        import torch
        n = self._net_rows(q, QNet, obs, action=action)
        for name, g in (("g_q1", g_q1), ("g_q2", g_q2)):
            if g is not None:
                self._check_tensor(name, g, torch.float32, (n,))
        if g_q2 is not None and q.n_critics != 2:
            raise ValueError("g_q2: the handle has one critic")
        if not params and not action_grad:
            raise ValueError("q_grad_torch: nothing to compute (params and action_grad are both off)")
        L = q.n_hidden + 1
        like = [q.tensors[2 * L * c:2 * L * (c + 1)] for c in range(q.n_critics)]
        if out is None:
            out = dict(critics=[_empty_pairs(ts) for ts in like] if params else None,
                       action=torch.empty((n, 2), dtype=torch.float32, device=obs.device) if action_grad else None)
        else:
            if params and out.get("critics") is None:
                raise ValueError("out['critics']: params is on; the critics' gradients need tensors")
            if action_grad and out.get("action") is None:
                raise ValueError("out['action']: action_grad is on; expected a float32 [n, 2] tensor")
            out = dict(critics=out.get("critics") if params else None, action=out.get("action") if action_grad else None)
        g, ws = None, None
        if params:
            g = _native.SgQnetGrads(struct_size=C.sizeof(_native.SgQnetGrads))
            nets = [list(c) for c in out["critics"]]
            if len(nets) != q.n_critics:
                raise ValueError(f"out['critics']: expected {q.n_critics} nets, got {len(nets)}")
            for c, pairs in enumerate(nets):
                self._grad_pairs(f"out['critics'][{c}]", pairs, like[c], g.critic[c])
        if action_grad:
            self._check_tensor("out['action']", out["action"], torch.float32, (n, 2))
        if params:
            ws = self._grad_workspace(q, "sg_q_grad_workspace_bytes", n, obs.device, "q_grad_torch")
        self._ck(self._lib.sg_q_grad_device(self._h, C.byref(q.struct), n, _ptr(obs), _ptr(action), _ptr(g_q1), _ptr(g_q2),
                                            C.byref(g) if g is not None else None, _ptr(out["action"]), _ptr(ws),
                                            ws.numel() if ws is not None else 0, self._stream()), "sg_q_grad_device")
        return out

    def q_evaluate_torch(self, q, obs, action):
        """q1, q2 = the critics' values of the (obs, action) rows under the CURRENT parameters, differentiable with respect to the
        parameter tensors the handle holds and, when action.requires_grad, with respect to action (obs gets None): a
        torch.autograd.Function whose forward is q_evaluate_raw_torch and whose backward is ONE q_grad_torch call -- params off when
        no parameter needs a gradient, action_grad only when the action needs one.  q2 is None with one critic.  With
        policy_action_torch it makes a TD3 / DDPG update plain torch on [n] vectors."""
        self._net_rows(q, QNet, obs, action=action)
        fn = _net_function("QEvaluate", lambda env, h, o, a: env.q_evaluate_raw_torch(h, o, a), _q_backward)
        return fn.apply(self, q, obs, action, *q.tensors)

    def policy_action_raw_torch(self, policy, obs, eps=None, out=None):
        """action float32 [n, 2] = mean(obs) + exp(log_std) * eps under a policy_torch handle of a continuous id, unclamped; eps
        float32 [n, 2] is the caller's noise, None: the mean (policy_act_torch(deterministic=True)'s action bit for bit).  One launch
        on torch's current stream, no autograd (sg_policy_action_device; graph-capturable).  out: the tensor to fill."""
        import torch
        n = self._net_rows(policy, Policy, obs, "policy_action_raw_torch", eps=eps)
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=obs.device)
        else:
            self._check_tensor("out", out, torch.float32, (n, 2))
        self._ck(self._lib.sg_policy_action_device(self._h, C.byref(policy.struct), n, _ptr(obs), _ptr(eps), _ptr(out), self._stream()),
                 "sg_policy_action_device")
        return out

    def policy_action_grad_torch(self, policy, obs, g_action, eps=None, out=None):
        """Gradients of a loss with respect to the actor's parameters and log_std through policy_action_raw_torch's action, given the
        loss's gradient g_action float32 [n, 2] by it (e.g. q_grad_torch's `action`): sg_policy_action_grad_device, policy_grad_torch's
        two launches with another score and its workspace.  Returns dict actor (list of (weight, bias) gradients) / log_std, WRITTEN,
        not accumulated; the policy's critic is not involved.  out: such a dict of tensors to fill."""
        import torch
        n = self._net_rows(policy, Policy, obs, "policy_action_grad_torch", eps=eps)
        self._check_tensor("g_action", g_action, torch.float32, (n, 2))
        L = policy.n_hidden + 1
        a_par = policy.tensors[:2 * L]
        if out is None:
            out = dict(actor=_empty_pairs(a_par), log_std=torch.empty_like(policy.tensors[-1]))
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        self._grad_pairs("out['actor']", out["actor"], a_par, g.actor)
        if out.get("log_std") is None:
            raise ValueError("out['log_std']: expected a float32 [2] tensor")
        self._check_tensor("out['log_std']", out["log_std"], torch.float32, (2,))
        g.log_std = out["log_std"].data_ptr()
        ws = self._grad_workspace(policy, "sg_policy_grad_workspace_bytes", n, obs.device, "policy_action_grad_torch")
        self._ck(self._lib.sg_policy_action_grad_device(self._h, C.byref(policy.struct), n, _ptr(obs), _ptr(eps), _ptr(g_action), C.byref(g), _ptr(ws),
                                                        ws.numel(), self._stream()), "sg_policy_action_grad_device")
        return out

    def policy_action_torch(self, policy, obs, eps=None):
        """action = mean(obs) + exp(log_std) * eps (eps None: the mean), differentiable with respect to the actor's tensors and log_std
        of the handle: a torch.autograd.Function over policy_action_raw_torch / policy_action_grad_torch.  obs and eps get None.  The
        action is unclamped; clamp it in torch where the algorithm wants that."""
        self._net_rows(policy, Policy, obs, "policy_action_torch", eps=eps)
        fn = _net_function("PolicyAction", lambda env, h, o, e: env.policy_action_raw_torch(h, o, e), _policy_action_backward, True)
        return fn.apply(self, policy, obs, eps, *policy.tensors)

    # ------------------------------------------------------------------ the SAC actor: tanh-squashed Gaussian, state-dependent log_std
    def squashed_policy_torch(self, actor, log_std_bounds=(-20.0, 2.0), activation="relu"):
        """A handle on a SAC actor whose parameters stay where they are (sg_squashed_policy: no copy, no transpose).  actor: a list
        [(weight, bias), ...] of float32 CUDA tensors in torch.nn.Linear layout -- obs_dim -> hidden (1 .. 3 layers of one width
        1 .. 128) -> 4: head outputs 0, 1 are the mean, 2, 3 the raw log_std, clamped to log_std_bounds (SB3's -20, 2).  The action
        is tanh(mean + exp(log_std) eps) in [-1, 1]^2, logp the squashed Gaussian's.  Continuous ids only."""
        import math
        if self.discrete:
            raise ValueError(f"squashed_policy_torch: {_NET_HANDLES[SquashedPolicy][2]} needs a continuous id; the discrete ids are not served")
        code = _activation_code(activation)
        try:
            lo, hi = (float(x) for x in log_std_bounds)
        except (TypeError, ValueError):
            raise ValueError(f"log_std_bounds: expected (min, max), got {log_std_bounds!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"log_std_bounds: expected finite min <= max, got {log_std_bounds!r}")
        p = _native.SgSquashedPolicy(struct_size=C.sizeof(_native.SgSquashedPolicy), activation=code, log_std_min=lo, log_std_max=hi)
        keep = []
        p.n_hidden, p.hidden = self._mlp_layers("actor", actor, self.obs_dim, 4, p.actor, keep)
        return SquashedPolicy(p, keep)

    def _squashed_out(self, out, n, device):
        import torch
        if out is None:
            return dict(action=torch.empty((n, 2), dtype=torch.float32, device=device), logp=torch.empty(n, dtype=torch.float32, device=device))
        if out.get("action") is None:
            raise ValueError("out['action']: expected a float32 [n, 2] tensor")
        self._check_tensor("out['action']", out["action"], torch.float32, (n, 2))
        if out.get("logp") is not None:
            self._check_tensor("out['logp']", out["logp"], torch.float32, (n,))
        return out

    def squashed_act_torch(self, sp, obs, seed=0, step=0, deterministic=False, out=None):
        """(action, logp) of the observations obs float32 [B, D] under a squashed_policy_torch handle, in one launch on torch's current
        stream (sg_squashed_act_device; graph-capturable).  action float32 [B, 2] in [-1, 1]; logp float32 [B].  Env i's noise is a
        function of (seed, step, env_index_base + i); deterministic: tanh(mean).  out: dict action / logp of tensors to fill (logp
        absent or None: not computed)."""
        import torch
        self._net_handle(sp, SquashedPolicy, "squashed_act_torch")
        B, D = self.num_envs, self.obs_dim
        self._check_tensor("obs", obs, torch.float32, (B, D))
        out = self._squashed_out(out, B, obs.device)
        self._ck(self._lib.sg_squashed_act_device(self._h, C.byref(sp.struct), _ptr(obs), int(seed), int(step), int(bool(deterministic)),
                                                  _ptr(out["action"]), _ptr(out.get("logp")), self._stream()), "sg_squashed_act_device")
        return out["action"], out.get("logp")

    def rollout_squashed_torch(self, sp, obs, action, reward, done, trunc, logp=None, seed=0, first_step=0, deterministic=False, terminal=None):
        """K closed-loop steps on torch's current stream without a host synchronisation (sg_rollout_squashed_device): for every t the
        actor acts on obs[t] (noise step first_step + t) and the env steps into obs[t + 1], exactly as squashed_act_torch followed by
        step_torch would.  obs float32 [K + 1, B, D] with the current observations in row 0; action float32 [K, B, 2]; reward float32 /
        done, trunc uint8 [K, B]; logp float32 [K, B] or None.  terminal: a terminal_list_torch dict, filled like rollout_torch's.  The
        buffers may be a replay ring's rows(K)."""
        self._net_handle(sp, SquashedPolicy, "rollout_squashed_torch")
        K = self._rollout_buffers(obs, action, (lambda d: d == 3, "[K, B, 2] "), [("logp", logp, 0)] * (logp is not None), reward, done, trunc)
        self._ck(self._lib.sg_rollout_squashed_device(self._h, K, C.byref(sp.struct), int(seed), int(first_step), int(bool(deterministic)),
                                                      _ptr(obs), _ptr(action), _ptr(logp), _ptr(reward), _ptr(done), _ptr(trunc),
                                                      self._terminal_list_struct(terminal)[0], self._stream()), "sg_rollout_squashed_device")
        return obs, action, logp, reward, done, trunc

    def squashed_sample_raw_torch(self, sp, obs, eps=None, out=None):
        """(action, logp) of the rows obs float32 [n, D] with the caller's noise eps float32 [n, 2] (None: zeros -- for the same rows
        squashed_act_torch(deterministic=True) bit for bit), any n >= 1: one launch on torch's current stream, no autograd
        (sg_squashed_sample_device; graph-capturable).  out: dict action / logp of tensors to fill (logp absent or None: not computed)."""
        n = self._net_rows(sp, SquashedPolicy, obs, "squashed_sample_raw_torch", eps=eps)
        out = self._squashed_out(out, n, obs.device)
        self._ck(self._lib.sg_squashed_sample_device(self._h, C.byref(sp.struct), n, _ptr(obs), _ptr(eps), _ptr(out["action"]), _ptr(out.get("logp")),
                                                     self._stream()), "sg_squashed_sample_device")
        return out["action"], out.get("logp")

    def squashed_grad_torch(self, sp, obs, eps=None, g_action=None, g_logp=None, out=None):
        """Gradients of a loss with respect to the actor's parameters through squashed_sample_raw_torch's (action, logp) at the same
        (obs, eps), given the loss's gradients g_action float32 [n, 2] and g_logp float32 [n] by them (each may be None: zeros, not
        both): sg_squashed_grad_device, two launches on torch's current stream, the forward pass recomputed inside, graph-capturable
        after one warm-up call with the same n (which sizes the workspace kept on the handle).  Returns dict actor: the list of
        (weight, bias) gradients, WRITTEN, not accumulated; out: such a dict of tensors to fill.  Same inputs and same n: the same bits."""
        import torch
        n = self._net_rows(sp, SquashedPolicy, obs, "squashed_grad_torch", eps=eps)
        if g_action is None and g_logp is None:
            raise ValueError("squashed_grad_torch: nothing to compute (g_action and g_logp are both None)")
        if g_action is not None:
            self._check_tensor("g_action", g_action, torch.float32, (n, 2))
        if g_logp is not None:
            self._check_tensor("g_logp", g_logp, torch.float32, (n,))
        if out is None:
            out = dict(actor=_empty_pairs(sp.tensors))
        g = _native.SgSquashedGrads(struct_size=C.sizeof(_native.SgSquashedGrads))
        self._grad_pairs("out['actor']", out["actor"], sp.tensors, g.actor)
        ws = self._grad_workspace(sp, "sg_squashed_grad_workspace_bytes", n, obs.device, "squashed_grad_torch")
        self._ck(self._lib.sg_squashed_grad_device(self._h, C.byref(sp.struct), n, _ptr(obs), _ptr(eps), _ptr(g_action), _ptr(g_logp), C.byref(g),
                                                   _ptr(ws), ws.numel(), self._stream()), "sg_squashed_grad_device")
        return out

    def squashed_sample_torch(self, sp, obs, eps=None):
        """action, logp = tanh(mean + exp(log_std) eps) and its log-prob (eps None: zeros), differentiable with respect to the actor's
        tensors of the handle: ONE torch.autograd.Function over squashed_sample_raw_torch whose backward is one squashed_grad_torch
        call (a None g for an output the loss did not use).  obs and eps get None.  The SAC actor loss stays on the device:
            a, lp = env.squashed_sample_torch(sp, obs, torch.randn_like(...))
            (alpha * lp - torch.min(*env.q_evaluate_torch(q, obs, a))).mean().backward()"""
        self._net_rows(sp, SquashedPolicy, obs, "squashed_sample_torch", eps=eps)
        fn = _net_function("SquashedSample", lambda env, h, o, e: env.squashed_sample_raw_torch(h, o, e), _squashed_backward)
        return fn.apply(self, sp, obs, eps, *sp.tensors)

    # ------------------------------------------------------------------ the DQN head of the discrete ids: Q(obs) -> 6, epsilon-greedy
    def _dqn_handle(self, dqn, who):
        """checks a dqn_torch handle and that the id is a discrete one"""
        self._net_handle(dqn, Dqn)
        if not self.discrete:
            raise ValueError(f"{who}: {_NET_HANDLES[Dqn][2]} needs a discrete id; the continuous ids are not served")

    def _dqn_rows(self, dqn, who, obs, action=None):
        """_dqn_handle, obs [n, D] and (given) action int32 [n]; returns n"""
        self._dqn_handle(dqn, who)
        return self._net_rows(dqn, Dqn, obs, **({} if action is None else dict(action=action)))

    def _dqn_epsilon(self, epsilon):
        """(the host scalar, the per-env tensor or None) of an epsilon that is a float in [0, 1] or a float32 CUDA tensor [num_envs]"""
        import math
        import torch
        if isinstance(epsilon, torch.Tensor):
            self._check_tensor("epsilon", epsilon, torch.float32, (self.num_envs,))
            return 0.0, epsilon
        try:
            eps = float(epsilon)
        except (TypeError, ValueError):
            raise ValueError(f"epsilon: expected a float in [0, 1] or a float32 CUDA tensor [num_envs], got {epsilon!r}") from None
        if math.isnan(eps) or not 0.0 <= eps <= 1.0:
            raise ValueError(f"epsilon: expected a float in [0, 1] or a float32 CUDA tensor [num_envs], got {epsilon!r}")
        return eps, None

    def dqn_torch(self, net, activation="relu"):
        """A handle on a DQN head whose parameters stay where they are (sg_dqn: no copy, no transpose; a target network is a second
        handle).  net: a list [(weight, bias), ...] of float32 CUDA tensors in torch.nn.Linear layout -- obs_dim -> hidden (1 .. 3
        layers of one width 1 .. 128) -> 6: output j is Q(obs, action j).  Discrete ids only."""
        if not self.discrete:
            raise ValueError(f"dqn_torch: {_NET_HANDLES[Dqn][2]} needs a discrete id; the continuous ids are not served")
        d = _native.SgDqn(struct_size=C.sizeof(_native.SgDqn), activation=_activation_code(activation))
        keep = []
        d.n_hidden, d.hidden = self._mlp_layers("net", net, self.obs_dim, 6, d.net, keep)
        return Dqn(d, keep)

    def dqn_act_torch(self, dqn, obs, seed=0, step=0, epsilon=0.0, out=None):
        """(action, q) of the observations obs float32 [B, D] under a dqn_torch handle, epsilon-greedy, in one launch on torch's
        current stream (sg_dqn_act_device; graph-capturable).  action int32 [B]; q float32 [B], the Q value of the action taken.
        epsilon: a float in [0, 1], or a float32 CUDA tensor [B] of per-env values that is read on the device at every launch (a
        captured graph anneals it by writing the tensor; its values are not checked: <= 0 never explores, >= 1 always does).  Env
        i's draw is a function of (seed, step, env_index_base + i); epsilon 0.0: the first argmax, nothing drawn.  out: dict action /
        q of tensors to fill (q absent or None: not computed)."""
        import torch
        self._dqn_handle(dqn, "dqn_act_torch")
        B, D = self.num_envs, self.obs_dim
        self._check_tensor("obs", obs, torch.float32, (B, D))
        eps, eps_dev = self._dqn_epsilon(epsilon)
        if out is None:
            out = dict(action=torch.empty(B, dtype=torch.int32, device=obs.device), q=torch.empty(B, dtype=torch.float32, device=obs.device))
        else:
            if out.get("action") is None:
                raise ValueError("out['action']: expected an int32 [num_envs] tensor")
            self._check_tensor("out['action']", out["action"], torch.int32, (B,))
            if out.get("q") is not None:
                self._check_tensor("out['q']", out["q"], torch.float32, (B,))
        self._ck(self._lib.sg_dqn_act_device(self._h, C.byref(dqn.struct), _ptr(obs), int(seed), int(step), eps, _ptr(eps_dev),
                                             _ptr(out["action"]), _ptr(out.get("q")), self._stream()), "sg_dqn_act_device")
        return out["action"], out.get("q")

    def rollout_dqn_torch(self, dqn, obs, action, reward, done, trunc, q=None, seed=0, first_step=0, epsilon=0.0, terminal=None):
        """K closed-loop steps on torch's current stream without a host synchronisation (sg_rollout_dqn_device): for every t the net
        acts on obs[t] (draw step first_step + t, epsilon as dqn_act_torch's) and the env steps into obs[t + 1], exactly as
        dqn_act_torch followed by step_torch would.  obs float32 [K + 1, B, D] with the current observations in row 0; action int32
        [K, B]; reward float32 / done, trunc uint8 [K, B]; q float32 [K, B] or None.  terminal: a terminal_list_torch dict, filled
        like rollout_torch's.  The buffers may be a replay ring's rows(K)."""
        self._dqn_handle(dqn, "rollout_dqn_torch")
        K = self._rollout_buffers(obs, action, (lambda d: d == 2, "[K, B] "), [("q", q, 0)] * (q is not None), reward, done, trunc)
        eps, eps_dev = self._dqn_epsilon(epsilon)
        self._ck(self._lib.sg_rollout_dqn_device(self._h, K, C.byref(dqn.struct), int(seed), int(first_step), eps, _ptr(eps_dev), _ptr(obs),
                                                 _ptr(action), _ptr(q), _ptr(reward), _ptr(done), _ptr(trunc),
                                                 self._terminal_list_struct(terminal)[0], self._stream()), "sg_rollout_dqn_device")
        return obs, action, q, reward, done, trunc

    def dqn_evaluate_raw_torch(self, dqn, obs, action=None, out=None):
        """(q_all, q_taken, q_max, argmax) of the rows obs float32 [n, D], any n >= 1, under a dqn_torch handle: one launch on torch's
        current stream, no autograd (sg_dqn_evaluate_device; graph-capturable).  q_all float32 [n, 6]; q_taken float32 [n] =
        q_all[i, action[i]] for action int32 [n] (None without an action); q_max float32 [n]; argmax int32 [n], the first argmax --
        all three elements of q_all bit for bit, and for the rows dqn_act_torch saw its bits.  out: dict q_all / q_taken / q_max /
        argmax of tensors to fill (allocated when None; an entry that is absent or None is not computed).  Double DQN's target:
        argmax of the online handle on next_obs, then q_taken of the target handle with it."""
        import torch
        n = self._dqn_rows(dqn, "dqn_evaluate_raw_torch", obs, action)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=obs.device)
        if out is None:
            out = dict(q_all=f32(n, 6), q_taken=f32(n) if action is not None else None, q_max=f32(n),
                       argmax=torch.empty(n, dtype=torch.int32, device=obs.device))
        elif out.get("q_taken") is not None and action is None:
            raise ValueError("action: out['q_taken'] is given; expected the int32 [n] actions")
        cols = self._out_columns(out, [("q_all", torch.float32, (n, 6)), ("q_taken", torch.float32, (n,)), ("q_max", torch.float32, (n,)),
                                       ("argmax", torch.int32, (n,))])
        self._ck(self._lib.sg_dqn_evaluate_device(self._h, C.byref(dqn.struct), n, _ptr(obs), _ptr(action), *map(_ptr, cols), self._stream()),
                 "sg_dqn_evaluate_device")
        return cols

    def dqn_grad_torch(self, dqn, obs, action=None, g_taken=None, g_all=None, out=None):
        """Gradients of a loss with respect to the net's parameters, given the loss's gradients g_taken float32 [n] and g_all float32
        [n, 6] by dqn_evaluate_raw_torch's q_taken and q_all at the same (obs, action) (each may be None: zeros, not both; action
        int32 [n] is needed with g_taken): sg_dqn_grad_device, two launches on torch's current stream, the forward pass recomputed
        inside, graph-capturable after one warm-up call with the same n (which sizes the workspace kept on the handle).  Returns dict
        net: the list of (weight, bias) gradients, WRITTEN, not accumulated; out: such a dict of tensors to fill.  Same inputs and
        same n: the same bits."""
        import torch
        n = self._dqn_rows(dqn, "dqn_grad_torch", obs, action)
        if g_taken is None and g_all is None:
            raise ValueError("dqn_grad_torch: nothing to compute (g_taken and g_all are both None)")
        if g_taken is not None:
            if action is None:
                raise ValueError("action: g_taken is given; expected the int32 [n] actions")
            self._check_tensor("g_taken", g_taken, torch.float32, (n,))
        if g_all is not None:
            self._check_tensor("g_all", g_all, torch.float32, (n, 6))
        if out is None:
            out = dict(net=_empty_pairs(dqn.tensors))
        g = _native.SgDqnGrads(struct_size=C.sizeof(_native.SgDqnGrads))
        self._grad_pairs("out['net']", out["net"], dqn.tensors, g.net)
        ws = self._grad_workspace(dqn, "sg_dqn_grad_workspace_bytes", n, obs.device, "dqn_grad_torch")
        self._ck(self._lib.sg_dqn_grad_device(self._h, C.byref(dqn.struct), n, _ptr(obs), _ptr(action), _ptr(g_taken), _ptr(g_all), C.byref(g),
                                              _ptr(ws), ws.numel(), self._stream()), "sg_dqn_grad_device")
        return out

    def dqn_evaluate_torch(self, dqn, obs, action=None):
        """q_all, or (q_all, q_taken) with an action int32 [n]: the Q values of the rows under the CURRENT parameters, differentiable
        with respect to the parameter tensors the handle holds: ONE torch.autograd.Function over dqn_evaluate_raw_torch whose backward
        is one dqn_grad_torch call (a None g for an output the loss did not use).  obs and action get None.  q_max and argmax come
        from the raw form; targets are computed under torch.no_grad().  A Double DQN update stays on the device:
            with torch.no_grad():
                a2 = env.dqn_evaluate_raw_torch(online, next_obs)[3]
                target = reward + discount * env.dqn_evaluate_raw_torch(target_net, next_obs, a2)[1]
            huber(env.dqn_evaluate_torch(online, obs, action)[1], target).mean().backward()"""
        self._dqn_rows(dqn, "dqn_evaluate_torch", obs, action)
        return _net_function("DqnEvaluate", _dqn_forward, _dqn_backward).apply(self, dqn, obs, action, *dqn.tensors)

    # ------------------------------------------------------------------ a DQN update on Retrace(lambda) / Q(lambda) targets of sequences
    retrace_traces = ("retrace", "tree_backup", "peng", "watkins", "is")

    def dqn_retrace_grad_torch(self, online, target_net, seq, mu=None, trace="retrace", epsilon=0.0, gamma=0.99, lam=1.0, huber_delta=1.0,
                               weight=None):
        """The online net's gradients of the Huber loss against Retrace(lambda) / Q(lambda) targets of a sequence batch, without
        autograd: a composition of dqn_evaluate_raw_torch, retrace_torch and dqn_grad_torch with no native code of its own, no host
        synchronisation, graph-capturable after one warm-up call.  online, target_net: dqn_torch handles of one architecture.  seq:
        the dict replay_sample_sequences_torch returns (obs [L + 1, n, D], action int32 [L, n], reward, done, trunc, terminal_obs
        [L, n, D]).  terminal_obs MUST BE A PREFILLED FINITE BUFFER: the sampler writes it only where done, and the target net is
        evaluated on all of it (the sampler's own allocation is zeros; retrace_torch then reads the values only where done and trunc).
        The target policy pi is greedy (epsilon 0.0) or epsilon-greedy in the target net, epsilon a float in [0, 1]:
            pi(a | s) = (1 - epsilon) [a == argmax] + epsilon / 6,    value = (1 - epsilon) q_max + (epsilon / 6) sum_j q_all[j]
        trace picks the ratio of retrace_torch: "retrace" pi / mu with c_bar 1; "tree_backup" pi; "peng" none; "watkins"
        [a == argmax]; "is" pi / mu with c_bar inf.  mu float32 [L, n]: the behaviour policy's probability of the action taken,
        gathered by the sampler's columns= as a rollout's logp is; needed by "retrace" and "is".  weight: float32 [n] per-sequence
        importance weights.  Returns (grads, rows): grads is dqn_grad_torch's dict, accepted by adam_step_torch as is; rows is
        dict(target, td_error, g) of float32 [L, n]."""
        import torch
        self._dqn_handle(online, "dqn_retrace_grad_torch")
        self._dqn_handle(target_net, "dqn_retrace_grad_torch")
        if trace not in self.retrace_traces:
            raise ValueError(f"trace: expected one of {self.retrace_traces}, got {trace!r}")
        eps, eps_dev = self._dqn_epsilon(epsilon)
        if eps_dev is not None:
            raise ValueError("epsilon: expected a float in [0, 1] (the target policy has one epsilon)")
        if not isinstance(seq, dict) or not isinstance(seq.get("obs"), torch.Tensor) or seq["obs"].dim() != 3 or int(seq["obs"].shape[0]) < 2:
            raise ValueError("seq: expected the dict replay_sample_sequences_torch returns (obs [L + 1, n, D], action, reward, done, trunc, "
                             "terminal_obs)")
        L, n, D = int(seq["obs"].shape[0]) - 1, int(seq["obs"].shape[1]), self.obs_dim
        for k, dtype, shape in (("obs", torch.float32, (L + 1, n, D)), ("action", torch.int32, (L, n)), ("terminal_obs", torch.float32, (L, n, D))):
            if seq.get(k) is None:
                raise ValueError(f"seq['{k}']: missing")
            self._check_tensor(f"seq['{k}']", seq[k], dtype, shape)
        needs_mu = trace in ("retrace", "is")
        if needs_mu and mu is None:
            raise ValueError(f"mu: trace {trace!r} needs the behaviour policy's probability of the action taken, float32 [L, n]")
        if mu is not None:
            self._check_tensor("mu", mu, torch.float32, (L, n))
        obs, last_obs = seq["obs"][:L].reshape(L * n, D), seq["obs"][L]
        action = seq["action"].reshape(L * n)

        def value_of(q_all, q_max):
            return q_max if eps == 0.0 else (1.0 - eps) * q_max + (eps / 6.0) * q_all.sum(dim=1)
        q_all, q, q_max, argmax = self.dqn_evaluate_raw_torch(target_net, obs, action)
        value = value_of(q_all, q_max).reshape(L, n)
        last_all, _, last_max, _ = self.dqn_evaluate_raw_torch(target_net, last_obs)
        term_all, _, term_max, _ = self.dqn_evaluate_raw_torch(target_net, seq["terminal_obs"].reshape(L * n, D))
        q_online = self.dqn_evaluate_raw_torch(online, obs, action)[1]
        greedy = (action == argmax).to(torch.float32).reshape(L, n)
        pi = greedy if eps == 0.0 else (1.0 - eps) * greedy + eps / 6.0
        ratio = {"retrace": lambda: pi / mu, "is": lambda: pi / mu, "tree_backup": lambda: pi, "watkins": lambda: greedy,
                 "peng": lambda: None}[trace]()
        rows = self.retrace_torch(seq["reward"], seq["done"], seq["trunc"], q.reshape(L, n), value, last_value=value_of(last_all, last_max),
                                  ratio=ratio, terminal_value=value_of(term_all, term_max).reshape(L, n), gamma=gamma, lam=lam,
                                  c_bar=float("inf") if trace == "is" else 1.0,
                                  loss=dict(q_online=q_online.reshape(L, n), weight=weight, huber_delta=huber_delta))
        grads = self.dqn_grad_torch(online, obs, action, g_taken=rows[2].reshape(L * n))
        return grads, dict(target=rows[0], td_error=rows[1], g=rows[2])

    # ------------------------------------------------------------------ the Double-DQN TD update: target, Huber loss, statistics and gradients
    dqn_td_stats_names = ("loss", "td_abs_mean", "td_abs_max", "q_mean", "target_mean", "clip_fraction", "weight_mean", "bad_rows")
    _DQN_TD_ROWS = ("td_error", "q_taken", "target", "q_next", "g")

    def _dqn_td_batch(self, batch, weight):
        """checks the replay batch dict of dqn_td_grad_torch and the optional weights; returns (obs, n)"""
        import torch
        if not isinstance(batch, dict):
            raise ValueError("batch: expected the dict replay_sample_torch returns (obs, action, reward, next_obs, terminated, discount)")
        obs = batch.get("obs")
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or int(obs.shape[0]) < 1:
            raise ValueError(f"batch['obs']: expected a CUDA tensor of shape (n, {self.obs_dim}) with n >= 1")
        n = int(obs.shape[0])
        spec = (("obs", torch.float32, (n, self.obs_dim)), ("action", torch.int32, (n,)), ("reward", torch.float32, (n,)),
                ("next_obs", torch.float32, (n, self.obs_dim)), ("terminated", torch.uint8, (n,)), ("discount", torch.float32, (n,)))
        for k, dtype, shape in spec:
            if batch.get(k) is None:
                raise ValueError(f"batch['{k}']: missing")
            self._check_tensor(f"batch['{k}']", batch[k], dtype, shape)
        if weight is not None:
            self._check_tensor("weight", weight, torch.float32, (n,))
        return obs, n

    def dqn_td_grad_torch(self, online, target, batch, double_q=True, huber_delta=1.0, weight=None, rows=None, out=None, stats=None):
        """One DQN / Double DQN TD update without autograd (sg_dqn_td_grad_device: the target, the Huber loss, its statistics and the
        online net's gradients in three launches on torch's current stream; no host synchronisation; graph-capturable after one
        warm-up call with the same n, which sizes the workspace kept on the online handle).  online, target: dqn_torch handles of one
        architecture.  batch: the dict replay_sample_torch / replay_sample_prioritized_torch return -- obs [n, D], action int32 [n],
        reward, next_obs [n, D], terminated uint8, discount (the per-row n-step discount: there is no separate gamma).  double_q: the
        online net's argmax on next_obs evaluated by the target net (False: the target net's maximum).  huber_delta: > 0;
        float("inf") gives 0.5 td^2.  weight: float32 [n] importance weights on the loss (a prioritized batch's weight).  Returns
        (grads, stats): grads is dqn_grad_torch's dict (net: the list of (weight, bias) gradients), WRITTEN, not accumulated (out:
        such a dict to fill), accepted by adam_step_torch as is; stats float32 [8], named by dqn_td_stats_names (stats: the tensor
        to fill).  rows: optional dict td_error (q_taken - target, signed) / q_taken / target / q_next / g of float32 [n] tensors
        that receive the per-row numbers the kernels used.  A row whose action is outside 0 .. 5 adds nothing and is counted in
        bad_rows.  Same inputs and same n: the same bits.  include/spacegym.h states the arithmetic."""
        import math
        import torch
        self._dqn_handle(online, "dqn_td_grad_torch")
        self._net_handle(target, Dqn)
        if (online.n_hidden, online.hidden, online.activation) != (target.n_hidden, target.hidden, target.activation):
            raise ValueError("target: expected a net of the online net's architecture (n_hidden, hidden, activation): "
                             f"{(target.n_hidden, target.hidden, target.activation)} against {(online.n_hidden, online.hidden, online.activation)}")
        obs, n = self._dqn_td_batch(batch, weight)
        try:
            delta = float(huber_delta)
        except (TypeError, ValueError):
            raise ValueError(f"huber_delta: expected a value > 0 (float('inf'): the squared loss), got {huber_delta!r}") from None
        if math.isnan(delta) or not delta > 0.0:
            raise ValueError(f"huber_delta: expected a value > 0 (float('inf'): the squared loss), got {huber_delta!r}")
        r = _native.SgDqnTdRows()
        if rows is not None:
            for k, t in rows.items():
                if k not in self._DQN_TD_ROWS:
                    raise ValueError(f"rows['{k}']: expected the keys {', '.join(self._DQN_TD_ROWS)}")
                if t is None:
                    continue
                self._check_tensor(f"rows['{k}']", t, torch.float32, (n,))
                setattr(r, k, t.data_ptr())
        if out is None:
            out = dict(net=_empty_pairs(online.tensors))
        g = _native.SgDqnGrads(struct_size=C.sizeof(_native.SgDqnGrads))
        self._grad_pairs("out['net']", out["net"], online.tensors, g.net)
        if stats is None:
            stats = obs.new_empty(len(self.dqn_td_stats_names))
        else:
            self._check_tensor("stats", stats, torch.float32, (len(self.dqn_td_stats_names),))
        cfg = _native.SgDqnTdConfig()
        self._lib.sg_dqn_td_config_init(C.byref(cfg))
        cfg.double_q, cfg.huber_delta = int(bool(double_q)), delta
        b = _native.SgDqnTdBatch(obs=obs.data_ptr(), action=batch["action"].data_ptr(), reward=batch["reward"].data_ptr(),
                                 next_obs=batch["next_obs"].data_ptr(), terminated=batch["terminated"].data_ptr(),
                                 discount=batch["discount"].data_ptr(), weight=weight.data_ptr() if weight is not None else None)
        ws = self._grad_workspace(online, "sg_dqn_td_grad_workspace_bytes", n, obs.device, "dqn_td_grad_torch", "sg_dqn_td_grad_workspace_bytes")
        self._ck(self._lib.sg_dqn_td_grad_device(self._h, C.byref(online.struct), C.byref(target.struct), C.byref(cfg), C.byref(b), n, C.byref(g),
                                                 _ptr(stats), C.byref(r) if rows is not None else None, _ptr(ws), ws.numel(), self._stream()),
                 "sg_dqn_td_grad_device")
        return out, stats

    def dqn_update_torch(self, online, target, opt, batch, double_q=True, huber_delta=1.0, weight=None, rows=None, grads=None, stats=None,
                         prio=None, alpha=0.6, priority_epsilon=1e-6, tau=None):
        """One whole DQN learner step in one call.  A COMPOSITION OF EXISTING ENTRY POINTS THAT ADDS NO NATIVE CODE:
        dqn_td_grad_torch(online, target, batch, ...) with out=grads, then adam_step_torch(opt, grads); with prio (a
        replay_priority_torch handle; batch needs the prioritized sampler's cell) replay_update_priorities_torch(prio, batch['cell'],
        rows['td_error'], alpha, priority_epsilon); with tau the target's tensors move towards the online ones by
        torch._foreach_lerp_(target, online, tau) (Polyak averaging).  tau: a float in [0, 1], or a float32 CUDA scalar tensor read
        on the device, so that a captured graph does a hard sync every N replays by writing 0 or 1 into it.  opt: adam_torch's state
        of `online`.  No host synchronisation; graph-capturable after one warm-up call, as the calls it makes are (rows and grads
        are then the caller's tensors, or those of the warm-up call's return).  Returns (stats, rows, grads)."""
        return self._td_update(online, target, opt, batch, rows, "td_error", lambda: self._dqn_td_batch(batch, weight),
                               lambda rows: self.dqn_td_grad_torch(online, target, batch, double_q=double_q, huber_delta=huber_delta, weight=weight,
                                                                   rows=rows, out=grads, stats=stats),
                               prio, alpha, priority_epsilon, tau)

    def _td_update(self, online, target, opt, batch, rows, priority_row, check_batch, grad_call, prio, priority_alpha, priority_epsilon, tau):
        """what dqn_update_torch and q_update_torch share: the checks of opt, tau and a prioritized batch, grad_call(rows) -> (grads,
        stats) with rows[priority_row] made when prio needs it (after check_batch()), the Adam step, the priority update and the lerp"""
        import torch
        if not isinstance(opt, AdamState) or opt.handle is not online:
            raise ValueError("opt: expected the AdamState adam_torch returned for the online handle")
        if tau is not None:
            if isinstance(tau, torch.Tensor):
                self._check_tensor("tau", tau, torch.float32, ())
            else:
                try:
                    tau = float(tau)
                except (TypeError, ValueError):
                    raise ValueError(f"tau: expected None, a float in [0, 1] or a float32 CUDA scalar tensor, got {tau!r}") from None
                if not 0.0 <= tau <= 1.0:
                    raise ValueError(f"tau: expected None, a float in [0, 1] or a float32 CUDA scalar tensor, got {tau!r}")
        rows = dict(rows) if rows is not None else {}
        if prio is not None:
            if not isinstance(batch, dict) or batch.get("cell") is None:
                raise ValueError("batch['cell']: missing (prio is given: the batch must be replay_sample_prioritized_torch's)")
            self._priority_arg(prio)
            if rows.get(priority_row) is None:
                check_batch()
                rows[priority_row] = torch.empty_like(batch["reward"])
        grads, stats = grad_call(rows or None)
        self.adam_step_torch(opt, grads)
        if prio is not None:
            self.replay_update_priorities_torch(prio, batch["cell"], rows[priority_row], alpha=priority_alpha, epsilon=priority_epsilon)
        if tau is not None:
            with torch.no_grad():  # (the target's tensors may be nn.Parameters)
                torch._foreach_lerp_(list(target.tensors), list(online.tensors), [tau] * len(target.tensors) if isinstance(tau, torch.Tensor) else tau)
        return stats, rows, grads

    # ------------------------------------------------------------------ the TD critic update of SAC / TD3 / DDPG: target, Huber loss, statistics and gradients
    q_td_stats_names = ("loss", "td1_abs_mean", "td2_abs_mean", "td_abs_max", "q1_mean", "q2_mean", "target_mean", "clip_fraction", "weight_mean")
    _Q_TD_ROWS = ("td1", "td2", "q1", "q2", "target", "q_next", "g1", "g2", "td_abs")

    def _q_td_batch(self, batch, next_action, next_logp, noise, weight):
        """checks the replay batch dict of q_td_grad_torch and the columns beside it; returns (obs, n)"""
        import torch
        if not isinstance(batch, dict):
            raise ValueError("batch: expected the dict replay_sample_torch returns (obs, action, reward, next_obs, terminated, discount)")
        obs = batch.get("obs")
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or int(obs.shape[0]) < 1:
            raise ValueError(f"batch['obs']: expected a CUDA tensor of shape (n, {self.obs_dim}) with n >= 1")
        n = int(obs.shape[0])
        spec = (("obs", torch.float32, (n, self.obs_dim)), ("action", torch.float32, (n, 2)), ("reward", torch.float32, (n,)),
                ("next_obs", torch.float32, (n, self.obs_dim)), ("terminated", torch.uint8, (n,)), ("discount", torch.float32, (n,)))
        for k, dtype, shape in spec:
            if batch.get(k) is None:
                raise ValueError(f"batch['{k}']: missing")
            self._check_tensor(f"batch['{k}']", batch[k], dtype, shape)
        if next_action is None:
            raise ValueError("next_action: expected the actor's float32 [n, 2] action at batch['next_obs']")
        self._check_tensor("next_action", next_action, torch.float32, (n, 2))
        for name, t, shape in (("next_logp", next_logp, (n,)), ("noise", noise, (n, 2)), ("weight", weight, (n,))):
            if t is not None:
                self._check_tensor(name, t, torch.float32, shape)
        return obs, n

    def q_td_grad_torch(self, online, target, batch, next_action, next_logp=None, alpha=0.2, noise=None, noise_std=0.2, noise_clip=0.5,
                        action_clip=1.0, huber_delta=float("inf"), weight=None, rows=None, out=None, stats=None):
        """One TD critic update of SAC, TD3 or DDPG without autograd (sg_q_td_grad_device: the target, the Huber loss, its statistics
        and the online critics' gradients in three launches on torch's current stream; no host synchronisation; graph-capturable
        after one warm-up call with the same n, which sizes the workspace kept on the online handle).  online, target: q_torch
        handles of one shape.  batch: the dict replay_sample_torch / replay_sample_prioritized_torch return -- obs [n, D], action
        [n, 2], reward, next_obs [n, D], terminated uint8, discount (the per-row n-step discount: there is no separate gamma).
        next_action float32 [n, 2]: the actor's action at next_obs, from one launch of the caller's --
          SAC   next_action, next_logp = squashed_act_torch(sp, batch['next_obs'], seed, step); alpha: a float, or a one-element
                float32 CUDA tensor read on the device (a learned alpha changes inside a captured graph): q_next -= alpha * next_logp
          TD3   next_action = policy_action_raw_torch(target_actor, batch['next_obs']); noise float32 [n, 2] standard normal draws:
                a' = clamp(next_action + clamp(noise_std * noise, -noise_clip, noise_clip), -action_clip, action_clip)
          DDPG  next_action alone, one critic: used as given, never clamped.
        huber_delta: > 0; the default float("inf") gives 0.5 td^2 PER CRITIC, half of the sum of the two mean squared errors that
        CleanRL's and SB3's TD3 / SAC minimise: their gradients are twice these (fold the factor into the learning rate).  weight:
        float32 [n] importance weights on the loss (a prioritized batch's weight).  Returns (grads, stats): grads is q_grad_torch's
        dict (critics: per critic the list of (weight, bias) gradients; action None), WRITTEN, not accumulated (out: such a dict to
        fill), accepted by adam_step_torch as is; stats float32 [9], named by q_td_stats_names (stats: the tensor to fill; with one
        critic the critic-2 entries are 0).  rows: optional dict td1 / td2 / q1 / q2 / target / q_next / g1 / g2 / td_abs of float32
        [n] tensors that receive the per-row numbers the kernels used; td_abs = 0.5 (|td1| + |td2|) (one critic: |td1|) is what
        replay_update_priorities_torch takes.  Same inputs and same n: the same bits.  include/spacegym.h states the arithmetic."""
        import math
        import torch
        self._net_handle(online, QNet, "q_td_grad_torch")
        self._net_handle(target, QNet)
        shape = lambda q: (q.n_critics, q.n_hidden, q.hidden, q.activation)
        if shape(online) != shape(target):
            raise ValueError("target: expected critics of the online handle's shape (n_critics, n_hidden, hidden, activation): "
                             f"{shape(target)} against {shape(online)}")
        obs, n = self._q_td_batch(batch, next_action, next_logp, noise, weight)

        def number(name, v, ok, what):
            try:
                x = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{name}: expected {what}, got {v!r}") from None
            if math.isnan(x) or not ok(x):
                raise ValueError(f"{name}: expected {what}, got {v!r}")
            return x
        delta = number("huber_delta", huber_delta, lambda x: x > 0.0, "a value > 0 (float('inf'): the squared loss)")
        noise_std = number("noise_std", noise_std, lambda x: x >= 0.0, "a value >= 0")
        noise_clip = number("noise_clip", noise_clip, lambda x: x >= 0.0, "a value >= 0 (float('inf'): no clamp)")
        action_clip = number("action_clip", action_clip, lambda x: x >= 0.0, "a value >= 0 (float('inf'): no clamp)")
        alpha_dev = None
        if isinstance(alpha, torch.Tensor):
            if next_logp is None:
                raise ValueError("alpha: a tensor is read only with next_logp (it scales the entropy term)")
            self._check_tensor("alpha", alpha, torch.float32, tuple(alpha.shape))
            if alpha.numel() != 1:
                raise ValueError(f"alpha: expected a float or a one-element float32 CUDA tensor, got shape {tuple(alpha.shape)}")
            alpha_dev, alpha = alpha, 0.0
        else:
            alpha = number("alpha", alpha, lambda x: True, "a float or a one-element float32 CUDA tensor")
        r = _native.SgQTdRows()
        if rows is not None:
            for k, t in rows.items():
                if k not in self._Q_TD_ROWS:
                    raise ValueError(f"rows['{k}']: expected the keys {', '.join(self._Q_TD_ROWS)}")
                if t is None:
                    continue
                if k in ("td2", "q2", "g2") and online.n_critics != 2:
                    raise ValueError(f"rows['{k}']: the handle has one critic")
                self._check_tensor(f"rows['{k}']", t, torch.float32, (n,))
                setattr(r, k, t.data_ptr())
        L = online.n_hidden + 1
        like = [online.tensors[2 * L * c:2 * L * (c + 1)] for c in range(online.n_critics)]
        if out is None:
            out = dict(critics=[_empty_pairs(ts) for ts in like], action=None)
        elif out.get("critics") is None:
            raise ValueError("out['critics']: the critics' gradients need tensors")
        g = _native.SgQnetGrads(struct_size=C.sizeof(_native.SgQnetGrads))
        nets = [list(c) for c in out["critics"]]
        if len(nets) != online.n_critics:
            raise ValueError(f"out['critics']: expected {online.n_critics} nets, got {len(nets)}")
        for c, pairs in enumerate(nets):
            self._grad_pairs(f"out['critics'][{c}]", pairs, like[c], g.critic[c])
        if stats is None:
            stats = obs.new_empty(len(self.q_td_stats_names))
        else:
            self._check_tensor("stats", stats, torch.float32, (len(self.q_td_stats_names),))
        cfg = _native.SgQTdConfig()
        self._lib.sg_q_td_config_init(C.byref(cfg))
        cfg.huber_delta, cfg.alpha, cfg.noise_std, cfg.noise_clip, cfg.action_clip = delta, alpha, noise_std, noise_clip, action_clip
        ptr = lambda t: t.data_ptr() if t is not None else None
        b = _native.SgQTdBatch(obs=obs.data_ptr(), action=batch["action"].data_ptr(), reward=batch["reward"].data_ptr(),
                               next_obs=batch["next_obs"].data_ptr(), terminated=batch["terminated"].data_ptr(),
                               discount=batch["discount"].data_ptr(), next_action=next_action.data_ptr(), weight=ptr(weight),
                               next_logp=ptr(next_logp), alpha_dev=ptr(alpha_dev), noise=ptr(noise))
        ws = self._grad_workspace(online, "sg_q_td_grad_workspace_bytes", n, obs.device, "q_td_grad_torch", "sg_q_td_grad_workspace_bytes")
        self._ck(self._lib.sg_q_td_grad_device(self._h, C.byref(online.struct), C.byref(target.struct), C.byref(cfg), C.byref(b), n, C.byref(g),
                                               _ptr(stats), C.byref(r) if rows is not None else None, _ptr(ws), ws.numel(), self._stream()),
                 "sg_q_td_grad_device")
        return out, stats

    def q_update_torch(self, online, target, opt, batch, next_action, next_logp=None, alpha=0.2, noise=None, noise_std=0.2, noise_clip=0.5,
                       action_clip=1.0, huber_delta=float("inf"), weight=None, rows=None, grads=None, stats=None, prio=None,
                       priority_alpha=0.6, priority_epsilon=1e-6, tau=None):
        """One whole critic step of SAC / TD3 / DDPG in one call.  A COMPOSITION OF EXISTING ENTRY POINTS THAT ADDS NO NATIVE CODE:
        q_td_grad_torch(online, target, batch, next_action, ...) with out=grads, then adam_step_torch(opt, grads); with prio (a
        replay_priority_torch handle; batch needs the prioritized sampler's cell) replay_update_priorities_torch(prio, batch['cell'],
        rows['td_abs'], priority_alpha, priority_epsilon); with tau the target's tensors move towards the online ones by
        torch._foreach_lerp_(target, online, tau) (Polyak averaging).  tau: a float in [0, 1], or a float32 CUDA scalar tensor read
        on the device.  opt: adam_torch's state of `online`.  The actor's step is q_actor_update_torch; alpha's stays
        the caller's.  No host synchronisation; graph-capturable after one warm-up call, as the calls
        it makes are (rows and grads are then the caller's tensors, or those of the warm-up call's return).  Returns (stats, rows,
        grads)."""
        return self._td_update(online, target, opt, batch, rows, "td_abs", lambda: self._q_td_batch(batch, next_action, next_logp, noise, weight),
                               lambda rows: self.q_td_grad_torch(online, target, batch, next_action, next_logp=next_logp, alpha=alpha, noise=noise,
                                                                 noise_std=noise_std, noise_clip=noise_clip, action_clip=action_clip,
                                                                 huber_delta=huber_delta, weight=weight, rows=rows, out=grads, stats=stats),
                               prio, priority_alpha, priority_epsilon, tau)

    # ------------------------------------------------------------------ the actor update of SAC / TD3 / DDPG through the twin Q critics
    q_actor_stats_names = ("loss", "logp_mean", "q1_mean", "q2_mean", "q_sel_mean", "critic2_fraction", "action_abs_mean", "dq_da_abs_max",
                           "log_alpha_grad")
    _Q_ACTOR_ROWS = dict(action=2, logp=1, q1=1, q2=1, q_sel=1, dq1_da=2, dq2_da=2, g_action=2)  # the columns of each row output

    def q_actor_grad_torch(self, actor, q, obs, eps=None, alpha=0.2, q_select=None, target_entropy=-2.0, rows=None, out=None, stats=None):
        """One actor update of SAC, TD3 or DDPG without autograd (sg_q_actor_squashed_grad_device / sg_q_actor_gaussian_grad_device: the
        action, the critics' values and action gradients, the loss mean(alpha logp - Q), its statistics and the actor's gradients in two
        launches on torch's current stream, the critics run once; no host synchronisation; graph-capturable after one warm-up call
        with the same n, which sizes the workspace kept on the actor handle).  actor: a squashed_policy_torch handle (SAC; with
        eps=None, alpha=0 a deterministic tanh actor), or a continuous policy_torch handle, whose action is policy_action_raw_torch's
        mean + exp(log_std) eps (TD3 / DDPG: eps=None, or the exploration noise; alpha must stay 0).  q: a q_torch handle.  obs
        float32 [n, D]; eps float32 [n, 2] standard normal draws or None (zeros).  alpha: a float >= 0, or a one-element float32 CUDA
        tensor read on the device (a learned temperature changes inside a captured graph).  q_select: 1 takes the smaller of two
        critics per row (ties and a NaN as torch.minimum), 0 critic 1 alone; None: 1 for a squashed actor on two critics, else 0.
        Returns (grads, stats): grads is squashed_grad_torch's dict (actor) or policy_action_grad_torch's (actor, log_std), WRITTEN,
        not accumulated (out: such a dict to fill), accepted by adam_step_torch as is; the critics get no gradient.  stats float32
        [9], named by q_actor_stats_names (stats: the tensor to fill): q2_mean and critic2_fraction are 0 when critic 2 did not run;
        log_alpha_grad = -(logp_mean + target_entropy) is the gradient of SB3's temperature loss by log_alpha (0 for a policy_torch
        actor), so the temperature step is the caller's three lines:
            log_alpha -= lr * stats[8]; alpha.copy_(log_alpha.exp())      (alpha: the tensor the calls read)
        rows: optional dict action [n, 2] / logp / q1 / q2 / q_sel / dq1_da [n, 2] / dq2_da [n, 2] / g_action [n, 2] of float32
        tensors that receive the per-row numbers the kernel used.  Same inputs and same n: the same bits.  include/spacegym.h states
        the arithmetic."""
        import math
        import torch
        who = "q_actor_grad_torch"
        squashed = isinstance(actor, SquashedPolicy)
        if not squashed and not isinstance(actor, Policy):
            raise ValueError("actor: expected the handle squashed_policy_torch returns, or the one policy_torch returns for a continuous id")
        n = self._net_rows(actor, SquashedPolicy if squashed else Policy, obs, who, eps=eps)
        self._net_handle(q, QNet, who)
        if q_select is None:
            q_select = 1 if squashed and q.n_critics == 2 else 0
        if isinstance(q_select, bool) or q_select not in (0, 1):
            raise ValueError(f"q_select: expected None, 0 (critic 1) or 1 (the minimum of two critics), got {q_select!r}")
        if q_select == 1 and q.n_critics != 2:
            raise ValueError("q_select: 1 takes the minimum of two critics, but the handle has one critic")
        alpha_dev = None
        if isinstance(alpha, torch.Tensor):
            if not squashed:
                raise ValueError("alpha: the policy_torch actor has no log-prob term: alpha must be 0")
            self._check_tensor("alpha", alpha, torch.float32, tuple(alpha.shape))
            if alpha.numel() != 1:
                raise ValueError(f"alpha: expected a float >= 0 or a one-element float32 CUDA tensor, got shape {tuple(alpha.shape)}")
            alpha_dev, alpha = alpha, 0.0
        else:
            try:
                alpha = float(alpha)
            except (TypeError, ValueError):
                raise ValueError(f"alpha: expected a float >= 0 or a one-element float32 CUDA tensor, got {alpha!r}") from None
            if math.isnan(alpha) or alpha < 0.0:
                raise ValueError(f"alpha: expected a float >= 0 or a one-element float32 CUDA tensor, got {alpha!r}")
            if not squashed and alpha != 0.0:
                raise ValueError("alpha: the policy_torch actor has no log-prob term: alpha must be 0")
        try:
            target_entropy = float(target_entropy)
        except (TypeError, ValueError):
            raise ValueError(f"target_entropy: expected a float, got {target_entropy!r}") from None
        if math.isnan(target_entropy):
            raise ValueError(f"target_entropy: expected a float, got {target_entropy!r}")
        r = _native.SgQActorRows()
        if rows is not None:
            for k, t in rows.items():
                if k not in self._Q_ACTOR_ROWS:
                    raise ValueError(f"rows['{k}']: expected the keys {', '.join(self._Q_ACTOR_ROWS)}")
                if t is None:
                    continue
                if k in ("q2", "dq2_da") and not q_select:
                    raise ValueError(f"rows['{k}']: critic 2 does not run (q_select is 0)")
                self._check_tensor(f"rows['{k}']", t, torch.float32, (n, 2) if self._Q_ACTOR_ROWS[k] == 2 else (n,))
                setattr(r, k, t.data_ptr())
        if squashed:
            if out is None:
                out = dict(actor=_empty_pairs(actor.tensors))
            g = _native.SgSquashedGrads(struct_size=C.sizeof(_native.SgSquashedGrads))
            self._grad_pairs("out['actor']", out["actor"], actor.tensors, g.actor)
        else:
            a_par = actor.tensors[:2 * (actor.n_hidden + 1)]
            if out is None:
                out = dict(actor=_empty_pairs(a_par), log_std=torch.empty_like(actor.tensors[-1]))
            g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
            self._grad_pairs("out['actor']", out["actor"], a_par, g.actor)
            if out.get("log_std") is None:
                raise ValueError("out['log_std']: expected a float32 [2] tensor")
            self._check_tensor("out['log_std']", out["log_std"], torch.float32, (2,))
            g.log_std = out["log_std"].data_ptr()
        if stats is None:
            stats = obs.new_empty(len(self.q_actor_stats_names))
        else:
            self._check_tensor("stats", stats, torch.float32, (len(self.q_actor_stats_names),))
        cfg = _native.SgQActorConfig()
        self._lib.sg_q_actor_config_init(C.byref(cfg))
        cfg.alpha, cfg.target_entropy, cfg.q_select = alpha, target_entropy, q_select
        a_ref = C.byref(actor.struct)
        ws = self._grad_workspace(actor, "sg_q_actor_grad_workspace_bytes", n, obs.device, who, "sg_q_actor_grad_workspace_bytes",
                                  query=(a_ref if squashed else None, None if squashed else a_ref, C.byref(q.struct), n))
        fn = "sg_q_actor_squashed_grad_device" if squashed else "sg_q_actor_gaussian_grad_device"
        self._ck(getattr(self._lib, fn)(self._h, a_ref, C.byref(q.struct), C.byref(cfg), n, _ptr(obs), _ptr(eps), _ptr(alpha_dev), C.byref(g),
                                        _ptr(stats), C.byref(r) if rows is not None else None, _ptr(ws), ws.numel(), self._stream()), fn)
        return out, stats

    def q_actor_update_torch(self, actor, q, opt, obs, eps=None, alpha=0.2, q_select=None, target_entropy=-2.0, rows=None, grads=None,
                             stats=None):
        """One whole actor step of SAC / TD3 / DDPG in one call.  A COMPOSITION OF EXISTING ENTRY POINTS THAT ADDS NO NATIVE CODE:
        q_actor_grad_torch(actor, q, obs, eps, ...) with out=grads, then adam_step_torch(opt, grads).  opt: adam_torch's state of
        `actor`.  The temperature's step stays the caller's (q_actor_grad_torch gives its three lines).  With q_update_torch before it
        this is the whole update of the continuous off-policy learners on the device.  No host synchronisation; graph-capturable
        after one warm-up call, as the calls it makes are (rows and grads are then the caller's tensors, or those of the warm-up
        call's return).  Returns (stats, rows, grads)."""
        if not isinstance(opt, AdamState) or opt.handle is not actor:
            raise ValueError("opt: expected the AdamState adam_torch returned for the actor handle")
        rows = dict(rows) if rows is not None else {}
        grads, stats = self.q_actor_grad_torch(actor, q, obs, eps=eps, alpha=alpha, q_select=q_select, target_entropy=target_entropy,
                                               rows=rows or None, out=grads, stats=stats)
        self.adam_step_torch(opt, grads)
        return stats, rows, grads

    def gae(self, reward, done, trunc, value=None, last_value=None, terminal_value=None, terminal=None, gamma=0.99, lam=0.95,
            bootstrap_truncated=True):
        """NumPy form of gae_torch (sg_gae): host arrays up and back.  terminal: dict count (an integer or a one-element array) /
        step_env [n, 2] / value [n] of host arrays, e.g. from terminal_records.  Returns (advantage, returns) float32 [K, B]."""
        if terminal_value is not None and terminal is not None:
            raise ValueError("terminal_value and terminal: give the terminal values in one form")
        cfg = self._gae_config(gamma, lam, bootstrap_truncated)
        B = self.num_envs
        if np.ndim(reward) != 2 or np.shape(reward)[0] < 1 or np.shape(reward)[1] != B:
            raise ValueError(f"reward: expected shape (K, {B}) with K >= 1, got {np.shape(reward)}")
        K = int(np.shape(reward)[0])

        def arr(name, a, dtype, shape):
            if a is None:
                return None
            a = np.asarray(a)
            if a.dtype == np.bool_ and dtype == np.uint8:
                a = a.view(np.uint8)
            if a.dtype != dtype or a.shape != shape:
                raise ValueError(f"{name}: expected {np.dtype(dtype).name} of shape {shape}, got {a.dtype} {a.shape}")
            return np.ascontiguousarray(a)
        reward = arr("reward", reward, np.float32, (K, B))
        done, trunc = arr("done", done, np.uint8, (K, B)), arr("trunc", trunc, np.uint8, (K, B))
        if done is None or trunc is None:
            raise ValueError("done and trunc are required")
        value, last_value = arr("value", value, np.float32, (K, B)), arr("last_value", last_value, np.float32, (B,))
        terminal_value = arr("terminal_value", terminal_value, np.float32, (K, B))
        vl, keep = None, None
        if terminal is not None:
            count = np.asarray(terminal["count"]).reshape(-1)
            if count.size != 1 or count.dtype.kind not in "iu" or int(count[0]) < 0:
                raise ValueError("terminal['count']: expected one non-negative integer")
            cap = int(np.shape(terminal["step_env"])[0])
            keep = (count.astype(np.uint32), arr("terminal['step_env']", terminal["step_env"], np.int32, (cap, 2)),
                    arr("terminal['value']", terminal["value"], np.float32, (cap,)))
            vl = _native.SgValueList(keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, cap)
        adv, ret = np.empty((K, B), np.float32), np.empty((K, B), np.float32)

        def ptr(a):
            return self._ptr(a) if a is not None else None
        self._ck(self._lib.sg_gae(self._h, K, C.byref(cfg), ptr(reward), ptr(done), ptr(trunc), ptr(value), ptr(last_value),
                                  ptr(terminal_value), C.byref(vl) if vl is not None else None, ptr(adv), ptr(ret)), "sg_gae")
        return adv, ret

    # ------------------------------------------------------------------ replay ring with uniform n-step sampling
    def replay_torch(self, steps, term_capacity=None):
        """A replay ring of `steps` time slots of the whole batch in device memory (ReplayRing): its rows are the tensors
        rollout_torch / step_torch(out=...) write into, so inserting copies nothing.  term_capacity: terminal observations kept
        (default max(2 B, T B // 16): a whole batch may truncate in one step, and the random policy finishes about 2 % of the
        env-steps).  Call replay_begin_torch before the first step."""
        import torch
        T, B, D = int(steps), self.num_envs, self.obs_dim
        if T < 2:
            raise ValueError(f"steps: at least 2 expected, got {T}")
        if T * B > 2 ** 31 - 1:
            raise ValueError(f"steps * num_envs = {T * B}: at most 2^31 - 1 (transitions are addressed by 32 bits)")
        cap = max(2 * B, T * B // 16) if term_capacity is None else int(term_capacity)
        if not 1 <= cap <= 2 ** 31 - 1:
            raise ValueError(f"term_capacity: 1 .. 2^31 - 1 expected, got {cap}")
        self._replay_need_auto_reset("replay_torch")
        dev = torch.device("cuda", self.device)
        e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        return ReplayRing(
            steps=T, num_envs=B, obs_dim=D, term_capacity=cap, discrete=self.discrete, obs=e((T, B, D), torch.float32),
            action=e((T, B), torch.int32) if self.discrete else e((T, B, 2), torch.float32), reward=e((T, B), torch.float32),
            done=e((T, B), torch.uint8), trunc=e((T, B), torch.uint8), term_idx=e((T, B), torch.int32),
            term_obs=e((cap, D), torch.float32), slot_seq=e((T,), torch.int32), hdr=torch.zeros(8, dtype=torch.int32, device=dev))

    def _replay_need_auto_reset(self, what):
        if not self._cfg.auto_reset:
            raise ValueError(f"{what}: the replay ring needs auto_reset on (with it off obs[t] of a finished step is the terminal "
                             "observation itself)")

    def _replay_arg(self, ring):
        """SgReplay over the tensors of a ReplayRing, checked"""
        import torch
        if not isinstance(ring, ReplayRing):
            raise ValueError("ring: expected the object replay_torch returned")
        T, B, D, cap = ring.steps, self.num_envs, self.obs_dim, ring.term_capacity
        if ring.num_envs != B or ring.obs_dim != D or ring.discrete != self.discrete:
            raise ValueError("ring: made for another batch size, observation width or action type")
        self._check_tensor("ring.obs", ring.obs, torch.float32, (T, B, D))
        self._check_tensor("ring.action", ring.action, torch.int32 if self.discrete else torch.float32, (T, B) if self.discrete else (T, B, 2))
        self._check_tensor("ring.reward", ring.reward, torch.float32, (T, B))
        self._check_tensor("ring.done", ring.done, torch.uint8, (T, B))
        self._check_tensor("ring.trunc", ring.trunc, torch.uint8, (T, B))
        self._check_tensor("ring.term_idx", ring.term_idx, torch.int32, (T, B))
        self._check_tensor("ring.term_obs", ring.term_obs, torch.float32, (cap, D))
        self._check_tensor("ring.slot_seq", ring.slot_seq, torch.int32, (T,))
        self._check_tensor("ring.hdr", ring.hdr, torch.int32, (8,))
        self._replay_need_auto_reset("ring")
        return _native.SgReplay(C.sizeof(_native.SgReplay), T, cap, 0, *(getattr(ring, k).data_ptr() for k in ReplayRing.MEMBERS))

    def replay_begin_torch(self, ring, obs0=None):
        """Empties the ring (sg_replay_begin_device).  obs0: float32 [B, D], the observation the first action will be taken from,
        copied into ring.obs[T - 1]; None: the caller wrote that row itself, e.g. reset_torch(out=ring.obs[ring.steps - 1])."""
        import torch
        r = self._replay_arg(ring)
        if obs0 is not None:
            self._check_tensor("obs0", obs0, torch.float32, (self.num_envs, self.obs_dim))
        self._ck(self._lib.sg_replay_begin_device(self._h, C.byref(r), C.c_void_p(obs0.data_ptr()) if obs0 is not None else None,
                                                  self._stream()), "sg_replay_begin_device")
        ring.head = ring.filled = 0
        return ring

    def replay_commit_torch(self, ring, n_steps, terminal=None, terminal_obs=None, priority=None):
        """Makes the n_steps slots at the ring's head, which the caller has just had written (ring.rows(n_steps): rollout_torch
        rows with their actions, or one step_torch(out=..., terminal_obs=...)), part of the ring (sg_replay_commit_device).
        Exactly one of terminal (the rollout's terminal list, terminal_list_torch) and terminal_obs (float32 [B, D] of one step).
        A commit may not cross the end of the ring: choose `steps` a multiple of the rollout length.
        priority: the ring's ReplayPriority: its commit (sg_priority_commit_device) follows with the same integers."""
        import torch
        r = self._replay_arg(ring)
        pr = self._priority_arg(priority, ring) if priority is not None else None
        K, T, D = int(n_steps), ring.steps, self.obs_dim
        if K < 1:
            raise ValueError(f"n_steps: at least 1 expected, got {K}")
        if ring.head + K > T:
            raise ValueError(f"n_steps: slots {ring.head} .. {ring.head + K - 1} cross the end of a ring of {T} (choose steps a "
                             "multiple of the rollout length)")
        if (terminal is None) == (terminal_obs is None):
            raise ValueError("terminal and terminal_obs: exactly one terminal form expected")
        tl = None
        if terminal is not None:
            cap = int(terminal["step_env"].shape[0])
            if (not isinstance(terminal["count"], torch.Tensor) or terminal["count"].dtype not in (torch.int32, torch.uint32)
                    or terminal["count"].numel() != 1):
                raise ValueError("terminal['count']: expected one 32-bit integer")
            self._check_tensor("terminal['count']", terminal["count"], terminal["count"].dtype, tuple(terminal["count"].shape))
            self._check_tensor("terminal['step_env']", terminal["step_env"], torch.int32, (cap, 2))
            self._check_tensor("terminal['obs']", terminal["obs"], torch.float32, (cap, D))
            tl = _native.SgTerminalList(terminal["count"].data_ptr(), terminal["step_env"].data_ptr(), terminal["obs"].data_ptr(), cap)
        else:
            if K != 1:
                raise ValueError(f"terminal_obs: dense terminal observations describe one step, n_steps = {K}")
            self._check_tensor("terminal_obs", terminal_obs, torch.float32, (self.num_envs, D))
        self._ck(self._lib.sg_replay_commit_device(self._h, C.byref(r), ring.head, ring.filled, K, C.byref(tl) if tl is not None else None,
                                                   C.c_void_p(terminal_obs.data_ptr()) if terminal_obs is not None else None,
                                                   self._stream()), "sg_replay_commit_device")
        first, filled = ring.head, ring.filled
        ring.head, ring.filled = (first + K) % T, min(filled + K, T)  # (the device ring has moved, whatever follows)
        if pr is not None:
            self._ck(self._lib.sg_priority_commit_device(self._h, C.byref(pr), first, filled, K, self._stream()),
                     "sg_priority_commit_device")
        return ring

    def replay_sample_torch(self, ring, n, seed=0, n_step=1, gamma=0.99, index=None, out=None):
        """A minibatch of n transitions drawn uniformly with replacement, with n_step-step returns (sg_replay_sample_device: one
        launch; torch's current stream, no host synchronisation, graph-capturable: a replayed call draws fresh indices).  Returns
        a dict obs [n, D], action [n, 2] (int32 [n]), reward, next_obs [n, D], terminated, truncated (uint8), discount, steps
        (uint8), index (int64): the target is reward + discount * (1 - terminated) * Q(next_obs).  index: int64 [n] of transition
        numbers in [0, len(ring)) to gather instead of drawing.  out: such a dict to write into (discount, steps, index optional).
        tests/replay_model.py states the arithmetic."""
        import torch
        r = self._replay_arg(ring)
        n, n_step, gamma, seed = int(n), int(n_step), float(gamma), int(seed)
        B, D = self.num_envs, self.obs_dim
        if not 0 <= n <= 2 ** 31 - 1:
            raise ValueError(f"n: 0 .. 2^31 - 1 expected, got {n}")
        if not 1 <= n_step <= 16:
            raise ValueError(f"n_step: 1 .. 16 expected, got {n_step}")
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed: an unsigned 64-bit integer expected, got {seed}")
        if n > 0 and len(ring) == 0:
            raise ValueError("ring: no valid transition yet (commit at least one step)")
        if index is not None:
            self._check_tensor("index", index, torch.int64, (n,))
        spec = dict(obs=(torch.float32, (n, D)), action=(torch.int32, (n,)) if self.discrete else (torch.float32, (n, 2)),
                    reward=(torch.float32, (n,)), next_obs=(torch.float32, (n, D)), terminated=(torch.uint8, (n,)),
                    truncated=(torch.uint8, (n,)), discount=(torch.float32, (n,)), steps=(torch.uint8, (n,)), index=(torch.int64, (n,)))
        if out is None:
            dev = torch.device("cuda", self.device)
            out = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (dtype, shape) in spec.items()}
        else:
            for k, (dtype, shape) in spec.items():
                if k in out or k not in ("discount", "steps", "index"):
                    self._check_tensor(f"out['{k}']", out[k], dtype, shape)
        cfg = _native.SgReplaySampleConfig(C.sizeof(_native.SgReplaySampleConfig), seed, n_step, gamma)
        batch = _native.SgReplayBatch(*(out[k].data_ptr() if k in out else None for k in spec))
        self._ck(self._lib.sg_replay_sample_device(self._h, C.byref(r), C.byref(cfg), n,
                                                   C.c_void_p(index.data_ptr()) if index is not None else None, C.byref(batch),
                                                   self._stream()), "sg_replay_sample_device")
        return out

    # ------------------------------------------------------------------ fixed-length sequences from the replay ring
    def replay_sample_sequences_torch(self, ring, n, length, seed=0, index=None, columns=None, out=None):
        """n sequences of `length` consecutive steps of one env each, drawn uniformly with replacement among the starts whose last
        step is still a valid transition (sg_replay_sequence_device: one launch; torch's current stream, no host synchronisation,
        graph-capturable: a replayed call draws afresh).  Returns a dict of time-major tensors, column j one pseudo-env of an L-step
        rollout: obs [L + 1, n, D], action [L, n, 2] (int32 [L, n]), reward, done, trunc [L, n], terminal_obs [L, n, D] (written
        only where done; allocated as zeros), index (int64 [n], the transition number of each column's first step) and, with
        columns=, `columns`: a list of [L, n] tensors.  With n == num_envs they go straight into gae_torch / gae_groups_torch /
        vtrace_torch, with terminal_value = V(terminal_obs).  index: int64 [n] of first transitions in [0, len(ring) - (L - 1)
        num_envs) to gather instead of drawing.  columns: up to four caller-owned float32 [T, B] tensors in the ring's slot layout
        (e.g. the logp and value a closed-loop rollout wrote next to ring.rows(K)), gathered like the reward.  out: such a dict to
        write into (terminal_obs, index and columns optional).  tests/sequence_model.py states the arithmetic."""
        import torch
        r = self._replay_arg(ring)
        n, L, seed = int(n), int(length), int(seed)
        T, B, D = ring.steps, self.num_envs, self.obs_dim
        held = len(ring) // B
        if not 0 <= n <= 2 ** 31 - 1:
            raise ValueError(f"n: 0 .. 2^31 - 1 expected, got {n}")
        if not 1 <= L <= T - 1:
            raise ValueError(f"length: 1 .. {T - 1} expected for a ring of {T} slots, got {L}")
        if L > held:
            raise ValueError(f"length: {L} steps asked for, the ring holds {held} steps per env")
        if (L + 1) * n > 2 ** 31 - 1:
            raise ValueError(f"(length + 1) * n = {(L + 1) * n}: at most 2^31 - 1 (rows are addressed by 32 bits)")
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed: an unsigned 64-bit integer expected, got {seed}")
        if index is not None:
            self._check_tensor("index", index, torch.int64, (n,))
        columns = list(columns) if columns is not None else []
        if len(columns) > 4:
            raise ValueError(f"columns: at most 4 expected, got {len(columns)}")
        for e, col in enumerate(columns):
            self._check_tensor(f"columns[{e}]", col, torch.float32, (T, B))
        spec = dict(obs=(torch.float32, (L + 1, n, D)), action=(torch.int32, (L, n)) if self.discrete else (torch.float32, (L, n, 2)),
                    reward=(torch.float32, (L, n)), done=(torch.uint8, (L, n)), trunc=(torch.uint8, (L, n)),
                    terminal_obs=(torch.float32, (L, n, D)), index=(torch.int64, (n,)))
        if out is None:
            dev = torch.device("cuda", self.device)
            out = {k: (torch.zeros if k == "terminal_obs" else torch.empty)(shape, dtype=dtype, device=dev)
                   for k, (dtype, shape) in spec.items()}
            if columns:
                out["columns"] = [torch.empty((L, n), dtype=torch.float32, device=dev) for _ in columns]
        else:
            for k, (dtype, shape) in spec.items():
                if k in out or k not in ("terminal_obs", "index"):
                    self._check_tensor(f"out['{k}']", out[k], dtype, shape)
            if columns:
                if "columns" not in out:
                    out["columns"] = [torch.empty((L, n), dtype=torch.float32, device=torch.device("cuda", self.device)) for _ in columns]
                elif len(out["columns"]) != len(columns):
                    raise ValueError(f"out['columns']: {len(columns)} tensors expected, got {len(out['columns'])}")
                for e, col in enumerate(out["columns"]):
                    self._check_tensor(f"out['columns'][{e}]", col, torch.float32, (L, n))
        cfg = _native.SgReplaySequenceConfig(C.sizeof(_native.SgReplaySequenceConfig), seed, L, len(columns))
        seqs = _native.SgReplaySequences(*(out[k].data_ptr() if k in out else None for k in spec))
        for e, col in enumerate(columns):
            seqs.extra_in[e], seqs.extra_out[e] = col.data_ptr(), out["columns"][e].data_ptr()
        self._ck(self._lib.sg_replay_sequence_device(self._h, C.byref(r), C.byref(cfg), n,
                                                     C.c_void_p(index.data_ptr()) if index is not None else None, C.byref(seqs),
                                                     self._stream()), "sg_replay_sequence_device")
        return out

    # ------------------------------------------------------------------ prioritized sampling with an exact integer sum tree
    def replay_priority_torch(self, ring, frac_bits=16):
        """The priorities of `ring` in device memory (ReplayPriority): one unsigned fixed-point integer with frac_bits fractional
        bits per cell, and the partial sums over them (64-bit integers: exact, order-independent, never drifting).  Call
        replay_priority_begin_torch before the first commit."""
        import torch
        self._replay_arg(ring)
        frac_bits = int(frac_bits)
        if not 0 <= frac_bits <= 31:
            raise ValueError(f"frac_bits: 0 .. 31 expected, got {frac_bits}")
        T, B = ring.steps, self.num_envs
        m = (C.c_size_t * 3)()
        if not self._lib.sg_priority_bytes(self._h, T, m):
            raise ValueError(f"replay_priority_torch: sg_priority_bytes refused steps = {T}")
        dev = torch.device("cuda", self.device)
        return ReplayPriority(T, B, frac_bits, leaf=torch.empty((T, B), dtype=torch.int32, device=dev),
                              node=torch.empty(m[1] // 8, dtype=torch.int64, device=dev), hdr=torch.zeros(16, dtype=torch.int32, device=dev))

    def _priority_arg(self, prio, ring=None):
        """SgPriority over the tensors of a ReplayPriority, checked"""
        import torch
        if not isinstance(prio, ReplayPriority):
            raise ValueError("priority: expected the object replay_priority_torch returned")
        T, B = prio.steps, self.num_envs
        if prio.num_envs != B:
            raise ValueError("priority: made for another batch size")
        if ring is not None and ring.steps != T:
            raise ValueError(f"priority: made for a ring of {T} slots, this ring has {ring.steps}")
        if not 0 <= prio.frac_bits <= 31:
            raise ValueError(f"priority: frac_bits 0 .. 31 expected, got {prio.frac_bits}")
        self._check_tensor("priority.leaf", prio.leaf, torch.int32, (T, B))
        self._check_tensor("priority.node", prio.node, torch.int64, tuple(prio.node.shape))
        if prio.node.dim() != 1:
            raise ValueError("priority.node: a one-dimensional tensor expected")
        self._check_tensor("priority.hdr", prio.hdr, torch.int32, (16,))
        self._replay_need_auto_reset("priority")
        return _native.SgPriority(C.sizeof(_native.SgPriority), T, prio.frac_bits, 0, prio.leaf.data_ptr(), prio.node.data_ptr(),
                                  prio.hdr.data_ptr())

    def replay_priority_begin_torch(self, prio):
        """Empties the priorities (sg_priority_begin_device): every cell 0, max priority 1.0."""
        p = self._priority_arg(prio)
        self._ck(self._lib.sg_priority_begin_device(self._h, C.byref(p), self._stream()), "sg_priority_begin_device")
        return prio

    def replay_priority_commit_torch(self, prio, first_slot, filled_before, n_steps):
        """sg_priority_commit_device on its own, with the three integers of the ring's commit (replay_commit_torch(priority=...)
        does both): the committed slots get the largest priority seen so far, the hole slot 0."""
        p = self._priority_arg(prio)
        first, filled, K, T = int(first_slot), int(filled_before), int(n_steps), prio.steps
        if K < 1 or first < 0 or first + K > T:
            raise ValueError(f"n_steps: slots {first} .. {first + K - 1} cross the end of a ring of {T}")
        if not 0 <= filled <= T:
            raise ValueError(f"filled_before: 0 .. {T} expected, got {filled}")
        self._ck(self._lib.sg_priority_commit_device(self._h, C.byref(p), first, filled, K, self._stream()), "sg_priority_commit_device")
        return prio

    def replay_update_priorities_torch(self, prio, cell, td_error=None, alpha=0.6, epsilon=1e-6, priority=None):
        """New priorities for the cells a prioritized batch named (sg_priority_update_device): (|td_error| + epsilon) ** alpha,
        computed in torch, or `priority` (float32 [n], already raised to alpha) passed straight through.  Duplicates: the largest
        wins; cells the collector has overwritten meanwhile are skipped."""
        import torch
        p = self._priority_arg(prio)
        if (td_error is None) == (priority is None):
            raise ValueError("td_error and priority: exactly one expected")
        if not isinstance(cell, torch.Tensor) or cell.dim() != 1:
            raise ValueError("cell: a one-dimensional int64 tensor expected")
        n = int(cell.shape[0])
        self._check_tensor("cell", cell, torch.int64, (n,))
        if priority is None:
            alpha, epsilon = float(alpha), float(epsilon)
            if not alpha >= 0.0 or not epsilon >= 0.0:
                raise ValueError(f"alpha and epsilon must be >= 0, got {alpha}, {epsilon}")
            self._check_tensor("td_error", td_error, torch.float32, (n,))
            priority = (td_error.abs() + epsilon) ** alpha
        else:
            self._check_tensor("priority", priority, torch.float32, (n,))
        self._ck(self._lib.sg_priority_update_device(self._h, C.byref(p), n, C.c_void_p(cell.data_ptr()), C.c_void_p(priority.data_ptr()),
                                                     self._stream()), "sg_priority_update_device")
        return prio

    def replay_priority_draw_torch(self, ring, prio, n, seed=0, beta=0.4, stratified=True, out=None):
        """n draws in proportion to the priorities (sg_priority_sample_device: one launch plus the call counter; no host
        synchronisation, graph-capturable: a replayed call draws afresh).  Returns a dict index (int64 [n], transition numbers for
        replay_sample_torch(index=...)), cell (int64 [n], the handle for replay_update_priorities_torch), weight (float32 [n],
        (N P)^-beta, unnormalised) and leaf (int32 [n], the bits of the drawn uint32 priorities).  out: such a dict to write into
        (cell and leaf optional).  tests/priority_model.py states the arithmetic."""
        import torch
        r = self._replay_arg(ring)
        p = self._priority_arg(prio, ring)
        n, seed, beta = int(n), int(seed), float(beta)
        if not 0 <= n <= 2 ** 31 - 1:
            raise ValueError(f"n: 0 .. 2^31 - 1 expected, got {n}")
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed: an unsigned 64-bit integer expected, got {seed}")
        if not 0.0 <= beta < float("inf"):
            raise ValueError(f"beta must be finite and >= 0, got {beta}")
        if n > 0 and len(ring) == 0:
            raise ValueError("ring: no valid transition yet (commit at least one step)")
        spec = dict(index=torch.int64, cell=torch.int64, weight=torch.float32, leaf=torch.int32)
        if out is None:
            dev = torch.device("cuda", self.device)
            out = {k: torch.empty((n,), dtype=dtype, device=dev) for k, dtype in spec.items()}
        else:
            for k, dtype in spec.items():
                if k in out or k not in ("cell", "leaf"):
                    self._check_tensor(f"out['{k}']", out[k], dtype, (n,))
        cfg = _native.SgPrioritySampleConfig(C.sizeof(_native.SgPrioritySampleConfig), seed, beta, int(bool(stratified)))
        draw = _native.SgPriorityDraw(*(out[k].data_ptr() if k in out else None for k in spec))
        self._ck(self._lib.sg_priority_sample_device(self._h, C.byref(r), C.byref(p), C.byref(cfg), n, C.byref(draw), self._stream()),
                 "sg_priority_sample_device")
        return out

    def replay_sample_prioritized_torch(self, ring, prio, n, seed=0, beta=0.4, stratified=True, n_step=1, gamma=0.99, normalize=True,
                                        out=None):
        """A minibatch of n transitions drawn in proportion to their priorities, with n_step-step returns: the draw
        (replay_priority_draw_torch), then the gather through replay_sample_torch(index=...).  Returns the uniform sampler's dict
        plus cell (int64) and weight (float32).  normalize: weight is divided by the batch maximum, in place, without a
        synchronisation (Dopamine's convention); False leaves (N P)^-beta.  out: such a dict to write into (discount, steps
        optional)."""
        draw_out = gather_out = None
        if out is not None:
            missing = [k for k in ("index", "cell", "weight") if k not in out]
            if missing:
                raise ValueError(f"out: {', '.join(missing)} missing (index, cell and weight are required; leaf, discount, steps optional)")
            draw_out = {k: out[k] for k in ("index", "cell", "weight", "leaf") if k in out}
            gather_out = {k: v for k, v in out.items() if k not in ("cell", "weight", "leaf")}
        d = self.replay_priority_draw_torch(ring, prio, n, seed=seed, beta=beta, stratified=stratified, out=draw_out)
        batch = self.replay_sample_torch(ring, n, seed=seed, n_step=n_step, gamma=gamma, index=d["index"], out=gather_out)
        if int(n) > 0 and normalize:
            d["weight"].div_(d["weight"].max())
        if out is not None:
            return out
        batch["index"], batch["cell"], batch["weight"] = d["index"], d["cell"], d["weight"]
        return batch

    # ------------------------------------------------------------------ hindsight goal relabelling of a replay batch
    HER_STRATEGIES = {"future": 0, "final": 1}

    def _her_args(self, ring, her_ratio, horizon, strategy, seed):
        """what both hindsight calls refuse before anything runs: (her_ratio, horizon, strategy code, seed)"""
        if self.spec["family"] != "goal":
            raise ValueError(f"replay_relabel_torch: {self.env_id} has no goal to relabel (a Goal id expected)")
        T = ring.steps
        her_ratio, seed = float(her_ratio), int(seed)
        H = T - 1 if horizon is None else int(horizon)
        if not 0.0 <= her_ratio <= 1.0:
            raise ValueError(f"her_ratio must be in [0, 1], got {her_ratio}")
        if not 1 <= H <= T - 1:
            raise ValueError(f"horizon: 1 .. {T - 1} expected for a ring of {T} slots, got {H}")
        if not isinstance(strategy, str) or strategy not in self.HER_STRATEGIES:
            raise ValueError(f"strategy: 'future' or 'final' expected, got {strategy!r}")
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed: an unsigned 64-bit integer expected, got {seed}")
        return her_ratio, H, self.HER_STRATEGIES[strategy], seed

    def replay_relabel_torch(self, ring, batch, her_ratio=0.8, horizon=None, strategy="future", seed=0, out=None):
        """Hindsight Experience Replay on a batch of a Goal id, in place (sg_replay_relabel_device: one launch; torch's current
        stream, no host synchronisation, graph-capturable).  batch: the dict replay_sample_torch or
        replay_sample_prioritized_torch has just returned from this ring with n_step = 1 (index and steps included), no commit in
        between.  With probability her_ratio a row's goal becomes the position the ship reached k steps later in the same episode:
        k uniform on 0 .. m ("future"; 0 is the step's own end position, as SB3's) or k = m ("final"), m the last of the next
        `horizon` steps (default: all the ring holds, steps - 1) before an episode end or the ring's newest edge.  The goal columns
        of obs and next_obs and the goal term of reward are rewritten (each env's current reward profile); action, terminated,
        truncated, discount, weight and cell stay as drawn.  Returns `batch` with relabelled (uint8 [n]: 0 as drawn, 1 relabelled,
        2 refused: steps != 1), offset (int32 [n]: k) and goal (float32 [n, 2]: the new goal position) added; the last two are
        written where relabelled.  out: a dict of such tensors to write into.  Refused: a Kepler id and auto_reset off
        (ValueError), observation or reward normalization on (by the native call: NativeError).  tests/her_model.py states the arithmetic."""
        import torch
        r = self._replay_arg(ring)
        her_ratio, H, code, seed = self._her_args(ring, her_ratio, horizon, strategy, seed)
        if not isinstance(batch, dict) or any(k not in batch for k in ("obs", "next_obs", "reward", "steps", "index")):
            raise ValueError("batch: a dict with obs, next_obs, reward, steps and index expected (what replay_sample_torch returns)")
        D = self.obs_dim
        n = int(batch["index"].shape[0]) if isinstance(batch["index"], torch.Tensor) and batch["index"].dim() == 1 else -1
        if not 0 <= n <= 2 ** 31 - 1:
            raise ValueError("batch['index']: a one-dimensional int64 tensor expected")
        for k, (dtype, shape) in dict(obs=(torch.float32, (n, D)), next_obs=(torch.float32, (n, D)), reward=(torch.float32, (n,)),
                                      steps=(torch.uint8, (n,)), index=(torch.int64, (n,))).items():
            self._check_tensor(f"batch['{k}']", batch[k], dtype, shape)
        spec = dict(relabelled=(torch.uint8, (n,)), offset=(torch.int32, (n,)), goal=(torch.float32, (n, 2)))
        if out is None:
            dev = torch.device("cuda", self.device)
            out = {k: torch.zeros(shape, dtype=dtype, device=dev) for k, (dtype, shape) in spec.items()}
        else:
            for k, (dtype, shape) in spec.items():
                if k in out:
                    self._check_tensor(f"out['{k}']", out[k], dtype, shape)
        cfg = _native.SgReplayRelabelConfig(C.sizeof(_native.SgReplayRelabelConfig), seed, her_ratio, H, code)
        b = _native.SgReplayBatch(obs=batch["obs"].data_ptr(), reward=batch["reward"].data_ptr(), next_obs=batch["next_obs"].data_ptr(),
                                  steps=batch["steps"].data_ptr(), index=batch["index"].data_ptr())
        o = _native.SgReplayRelabelOut(*(out[k].data_ptr() if k in out else None for k in spec))
        self._ck(self._lib.sg_replay_relabel_device(self._h, C.byref(r), C.byref(cfg), n, C.byref(b), C.byref(o), self._stream()),
                 "sg_replay_relabel_device")
        for k in spec:
            if k in out:
                batch[k] = out[k]
        return batch

    def replay_sample_her_torch(self, ring, n, her_ratio=0.8, horizon=None, strategy="future", seed=0, gamma=0.99, prio=None, beta=0.4,
                                stratified=True, normalize=True, out=None):
        """A minibatch of n single-step transitions with hindsight goals: replay_sample_torch (prio=None) or
        replay_sample_prioritized_torch (prio: the ring's ReplayPriority; weight and cell are left as drawn) with n_step = 1, then
        replay_relabel_torch with the same seed.  A composition of those calls: it ADDS NO NATIVE CODE of its own.  out: a dict to
        write into, the sampler's members and optionally relabelled, offset, goal."""
        extra = ("relabelled", "offset", "goal")
        self._replay_arg(ring)
        self._her_args(ring, her_ratio, horizon, strategy, seed)  # (refused before the sampler advances the ring's call counter)
        sample_out = None if out is None else {k: v for k, v in out.items() if k not in extra}
        if prio is None:
            batch = self.replay_sample_torch(ring, n, seed=seed, n_step=1, gamma=gamma, out=sample_out)
        else:
            batch = self.replay_sample_prioritized_torch(ring, prio, n, seed=seed, beta=beta, stratified=stratified, n_step=1, gamma=gamma,
                                                         normalize=normalize, out=sample_out)
        batch = self.replay_relabel_torch(ring, batch, her_ratio=her_ratio, horizon=horizon, strategy=strategy, seed=seed,
                                          out=None if out is None else {k: out[k] for k in extra if k in out})
        if out is not None:
            out.update({k: batch[k] for k in extra if k in batch})
            return out
        return batch

    def random_actions_torch(self, n_steps, seed=0, first_step=0, out=None):
        """the uniformly random policy generated on the device: [n_steps, B, 2] float32 in (-1, 1) (discrete ids: int32
        [n_steps, B] in 0..5); entry (t, i) depends only on (seed, global env index, first_step + t)."""
        import torch
        shape = (int(n_steps), self.num_envs) if self.discrete else (int(n_steps), self.num_envs, 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32 if self.discrete else torch.float32, device=f"cuda:{self.device}")
        assert tuple(out.shape) == shape and out.is_contiguous()
        rc = self._lib.sg_random_actions_device(self._h, int(n_steps), C.c_uint64(seed), C.c_uint64(first_step),
                                                C.c_void_p(out.data_ptr()), self._stream())
        self._ck(rc, "sg_random_actions_device")
        return out

    def set_unfused_rollout(self, on):
        """rollout_torch as K launches of the step kernel instead of the fused K-step kernel (A/B, equivalence test)."""
        self._ck(self._lib.sg_set_unfused_rollout(self._h, int(on)), "sg_set_unfused_rollout")

    # ------------------------------------------------------------------ measurement aid
    def rollout_kernel(self, n_steps):
        """name of the kernel rollout_torch launches for n_steps steps (as rocprofv3 prints it)"""
        return self._lib.sg_rollout_kernel(self._h, int(n_steps)).decode()

    def set_profiling(self, on):
        self._ck(self._lib.sg_set_profiling(self._h, int(bool(on))), "sg_set_profiling")

    def get_profile(self):
        """(launches, total_ms, min_ms, max_ms) of the step-kernel launches since the last call; synchronise first."""
        n, tot, mn, mx = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        self._ck(self._lib.sg_get_profile(self._h, C.byref(n), C.byref(tot), C.byref(mn), C.byref(mx)), "sg_get_profile")
        return n.value, tot.value, mn.value, mx.value


_ENGINE_KWARGS = ("device", "seed", "env_index_base", "max_episode_steps", "auto_reset", "validate_actions", "terminal_observation",
                  "copy", "steering", "env_kwargs", "from_class", "episode_statistics", "normalize_obs", "normalize_reward",
                  "norm_gamma", "norm_epsilon", "clip_obs", "clip_reward", "render", "reward_profiles")
# the normalization keywords, which the multi-device front ends do not serve yet (a cross-device reduction is needed)
_NORM_KWARGS = ("normalize_obs", "normalize_reward", "norm_gamma", "norm_epsilon", "clip_obs", "clip_reward")


class DeviceSnapshot:
    """What snapshot_torch returns: `buffer` (uint8 CUDA tensor of sg_snapshot_bytes bytes, the caller's to keep, clone or
    overwrite through snapshot_torch(out=...)), and the batch size and env id it was taken from (checked by restore_torch)."""
    __slots__ = ("buffer", "num_envs", "env_id")

    def __init__(self, buffer, num_envs, env_id):
        self.buffer, self.num_envs, self.env_id = buffer, int(num_envs), env_id


def make_vec(env_id, num_envs=1, **kwargs):
    """Batched counterpart of gym.make(env_id, **kwargs) for the ids in gym_space/__init__.py: keywords of the reference's
    constructors (GoalEnv.__init__ goal.py:18-31: goal_vel_reward_scale, safety_reward_scale, goal_sparse_reward, danger_zone,
    survival_reward_scale, n_planets, ship_steering, ship_moi, max_engine_force; KeplerEnv.__init__ kepler.py:189-203: randomize,
    ref_orbit_a, ref_orbit_eccentricity, ref_orbit_angle, numerator_C, rad_penalty_C, act_penalty_C, step_size, ship_steering,
    ship_moi, max_engine_force) override what the id is registered with; the engine's own keywords (device, seed, ...) are
    SpaceGymVectorEnv's.  devices=[...] cuts the batch into one block per listed GPU, driven by this one process
    (MultiDeviceVectorEnv)."""
    devices = kwargs.pop("devices", None)
    if devices is not None:  # one VectorEnv over several GPUs, driven by this process (space_gym_amd/multi_device.py)
        from .multi_device import MultiDeviceVectorEnv
        return MultiDeviceVectorEnv(env_id, num_envs, devices, **kwargs)
    engine = {k: kwargs.pop(k) for k in list(kwargs) if k in _ENGINE_KWARGS}
    if kwargs:
        engine["env_kwargs"] = {**(engine.get("env_kwargs") or {}), **kwargs}
    return SpaceGymVectorEnv(env_id, num_envs, **engine)


def make_vec_from_class(class_name, num_envs=1, **kwargs):
    """Batched counterpart of constructing one of the reference's classes directly -- GoalContinuousEnv(**kwargs),
    GoalDiscreteEnv, KeplerContinuousEnv, KeplerDiscreteEnv (goal.py:286-291, kepler.py:270-275): the constructor's own
    defaults apply (ship_steering=0, i.e. Steering.acceleration; KeplerEnv: step_size=0.1) and GoalEnv's three reward scales
    are required.  No TimeLimit unless max_episode_steps is given (the classes have none; it is gym.make that adds it)."""
    if class_name not in ENV_CLASSES:
        raise ValueError(f"unknown class {class_name!r}; served: {sorted(ENV_CLASSES)}")
    kwargs.setdefault("max_episode_steps", 2 ** 31 - 1)
    return make_vec(ENV_CLASSES[class_name], num_envs, from_class=True, **kwargs)
