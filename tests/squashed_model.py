"""The contract of sg_squashed_act_device / sg_squashed_sample_device / sg_squashed_grad_device (include/spacegym.h)
in NumPy: the SAC actor -- an MLP whose head of 4 gives (mean_0, mean_1, raw_0, raw_1) -- and per row, d = 0, 1:
    ls_d  = min(max(raw_d, log_std_min), log_std_max)
    u_d   = mean_d + exp(ls_d) eps_d;  e_d = exp(-2 |u_d|);  a_d = sign(u_d) (1 - e_d) / (1 + e_d)
    ldj_d = 2 (ln 2 - |u_d| - log1p(e_d));  logp = sum_d(-eps_d^2 / 2 - ls_d - ln(2 pi) / 2 - ldj_d)
and a hand-written backprop of sum_i (g_action[i] . a[i] + g_logp[i] logp[i]) to every parameter, eps a constant:
    gu_d = g_action_d 4 e_d / (1 + e_d)^2 + g_logp 2 a_d;  dz_mean_d = gu_d
    dz_raw_d = (gu_d exp(ls_d) eps_d - g_logp) [log_std_min <= raw_d <= log_std_max]
float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every per-row contribution
is formed in float32 and the batch is summed by plain sequential float32 accumulation (G32seq), as tests/policy_grad_model.py, whose
_forward / _backward / flat / grad_tolerances are used as they are."""
import numpy as np

from policy_grad_model import _backward, _forward, flat, grad_tolerances  # noqa: F401  (flat, grad_tolerances: re-exported)
from policy_model import LOG_SQRT_2PI, u23
from replay_model import philox4x32_10

STREAM_SQUASHED = 6
LN2 = 0.6931471805599453
BOUNDS = (-0.5, 0.5)  # the cases' clamp: dense random heads land below, inside and above it
NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS
MARGIN = 1e-3  # no case keeps a row whose float64 raw_d is this close to a bound


def words(seed, step, env_global):
    """the four Philox words of env-steps (seed, step, env_global[...]): key = seed, counter = (env, step lo, step hi, 6)"""
    seed, step = int(seed), int(step)
    env = np.asarray(env_global, np.uint64)
    return philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (env, step & 0xFFFFFFFF, step >> 32, STREAM_SQUASHED))


def noise(seed, step, env_global, dtype=np.float64):
    """eps [B, 2]: the Box-Muller pair of words 0, 1"""
    dtype = np.dtype(dtype).type
    o = words(seed, step, env_global)
    r = np.sqrt(dtype(-2) * np.log(u23(o[0]).astype(dtype)))
    ang = dtype(2 * np.pi) * u23(o[1]).astype(dtype)
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).astype(dtype)


def random_squashed(rng, obs_dim, hidden, n_hidden):
    """dense random float32 actor with a head of 4 (uniform in +-1 / sqrt(fan_in), as policy_model.random_policy's nets); the raw
    log_std rows of the head are scaled up so that they spread over about +-1.5"""
    dims = [obs_dim] + [hidden] * n_hidden + [4]
    layers = [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.float32(np.sqrt(i)), rng.uniform(-1, 1, o).astype(np.float32) / np.float32(np.sqrt(i)))
              for i, o in zip(dims[:-1], dims[1:])]
    W, b = layers[-1]
    W[2:] *= np.float32(3.0)
    b[2:] = rng.uniform(-1, 1, 2).astype(np.float32)
    return layers


def sample(actor, obs, eps=None, g_action=None, g_logp=None, bounds=(-20.0, 2.0), activation="relu", dtype=np.float64):
    """actor: [(W, b), ...] with a head of 4.  obs [n, D]; eps [n, 2] or None (zeros); g_action [n, 2], g_logp [n]: None means zeros.
    Returns dict action [n, 2], logp [n], the intermediates mean, raw, ls, u, and, when a g is given, actor: [(dW, db), ...]."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(obs)
    n = obs.shape[0]
    lo, hi = dtype(np.float32(bounds[0])), dtype(np.float32(bounds[1]))  # the struct holds float32 bounds
    hs, pre, head = _forward(actor, obs, activation, dtype)
    mean, raw = head[:, :2], head[:, 2:]
    ls = np.minimum(np.maximum(raw, lo), hi)
    e_ = np.zeros((n, 2), dtype) if eps is None else np.asarray(eps, dtype)
    sigma = np.exp(ls)
    u = mean + sigma * e_
    au = np.abs(u)
    e = np.exp(dtype(-2) * au)
    a = np.copysign((dtype(1) - e) / (dtype(1) + e), u)
    ldj = dtype(2) * ((dtype(LN2) - au) - np.log1p(e))
    logp = (((dtype(-0.5) * e_ * e_ - ls) - dtype(LOG_SQRT_2PI)) - ldj).sum(axis=1)
    out = dict(action=a.astype(dtype), logp=logp.astype(dtype), mean=mean, raw=raw, ls=ls, u=u)
    if g_action is None and g_logp is None:
        return out
    ga = np.zeros((n, 2), dtype) if g_action is None else np.asarray(g_action, dtype)
    gl = (np.zeros(n, dtype) if g_logp is None else np.asarray(g_logp, dtype))[:, None]
    gu = ga * (dtype(4) * e / ((dtype(1) + e) * (dtype(1) + e))) + gl * (dtype(2) * a)
    inside = ((raw >= lo) & (raw <= hi)).astype(dtype)  # bounds inclusive, as torch.clamp's backward
    dz = np.concatenate([gu, (gu * (sigma * e_) - gl) * inside], axis=1).astype(dtype)
    out["actor"] = _backward(actor, hs, pre, dz, activation, dtype)
    return out


def act(actor, obs, seed=0, step=0, env_index_base=0, deterministic=False, **kw):
    """sample() with the engine's own noise of (seed, step, env_index_base + i); deterministic: eps = 0"""
    B = np.asarray(obs).shape[0]
    dtype = kw.get("dtype", np.float64)
    eps = None if deterministic else noise(seed, step, int(env_index_base) + np.arange(B), dtype)
    out = sample(actor, obs, eps, **kw)
    out["eps"] = np.zeros((B, 2), np.dtype(dtype).type) if eps is None else eps
    return out


def case(obs_dim, n, hidden, n_hidden, seed):
    """The shared inputs of a (net, n) case, CPU and GPU tests alike: actor, obs [n, D], eps [n, 2], g_action [n, 2], g_logp [n], all
    float32, with the tight BOUNDS.  Any observation row whose float64 raw_d lies within MARGIN of a bound is redrawn (deterministically,
    from the case's own generator) until none does: a float32 / float64 disagreement about the clamp mask would move a summed gradient
    by O(1).  No row is left out."""
    return case_of(obs_dim, n, hidden, n_hidden, seed)


def case_of(obs_dim, n, hidden, n_hidden, seed, bounds=BOUNDS, prepare=None):
    """case() under other clamp bounds and with the freshly drawn actor passed through `prepare` (tests/net_regimes.py scales it) before
    the redraw rule is applied to it: the same draws in the same order"""
    rng = np.random.default_rng([seed, obs_dim, n, hidden, n_hidden])
    actor = random_squashed(rng, obs_dim, hidden, n_hidden)
    if prepare is not None:
        actor = prepare(actor)
    obs = rng.standard_normal((n, obs_dim)).astype(np.float32)
    eps = rng.standard_normal((n, 2)).astype(np.float32)
    ga = rng.standard_normal((n, 2)).astype(np.float32)
    gl = rng.standard_normal(n).astype(np.float32)
    lo, hi = float(np.float32(bounds[0])), float(np.float32(bounds[1]))
    for activation in ("tanh", "relu"):  # the same rows serve both activations
        for _ in range(100):
            raw = _forward(actor, obs, activation, np.float64)[2][:, 2:]
            near = (np.minimum(np.abs(raw - lo), np.abs(raw - hi)) < MARGIN).any(axis=1)
            if not near.any():
                break
            obs[near] = rng.standard_normal((int(near.sum()), obs_dim)).astype(np.float32)
        else:
            raise AssertionError("case: rows near a clamp bound remain")
    for activation in ("tanh", "relu"):
        raw = _forward(actor, obs, activation, np.float64)[2][:, 2:]
        assert not (np.minimum(np.abs(raw - lo), np.abs(raw - hi)) < MARGIN).any()
    return dict(actor=actor, obs=obs, eps=eps, g_action=ga, g_logp=gl)


# (obs_dim, n, hidden, n_hidden, activation): the gradient cases tests/test_gpu_squashed.py runs; tests/test_squashed.py checks on the
# CPU that each one's tolerance is at most 1 % of its tensor's largest gradient.  obs_dim 15: the Goal 3-planet id, 10: the Kepler ids.
GRAD_NS = [1, 200, 2049]
BIG_N = 256 * 64 + 300  # hidden 128 has workgroups of 64 rows: past the grid cap of 256 they take a second row tile


def grad_cases():
    """both activations on every net at n = 200; at the other row counts the activations alternate over the nets"""
    cases = []
    for n in GRAD_NS:
        for i, (hidden, n_hidden) in enumerate(NETS):
            for activation in ("tanh", "relu") if n == 200 else (("tanh", "relu")[i % 2],):
                cases.append((15 if i % 2 == 0 else 10, n, hidden, n_hidden, activation))
    cases.append((15, BIG_N, 128, 1, "relu"))
    return cases


SELECTIONS = ("both", "action", "logp")


def grad_reference(c, activation, selection, dtype, bounds=BOUNDS):
    """flat gradients of a case under a selection of the loss gradients"""
    ga = c["g_action"] if selection in ("both", "action") else None
    gl = c["g_logp"] if selection in ("both", "logp") else None
    return flat(sample(c["actor"], c["obs"], c["eps"], ga, gl, bounds=bounds, activation=activation, dtype=dtype))
