"""The contract of sg_dqn_act_device / sg_dqn_evaluate_device / sg_dqn_grad_device (include/spacegym.h) in NumPy:
the DQN head of the discrete ids -- an MLP whose head of 6 gives Q(obs, action j) -- and per row
    argmax = the first j with Q_j = max_j Q_j;  q_max = Q[argmax];  q_taken = Q[action]
    act:   explore = u23(o0) < eps_i;  action = explore ? floor(o1 * 6 / 2^32) : argmax
with o the Philox block of key = seed, counter = (env_index_base + i, step lo, step hi, 7), and a hand-written backprop of
    sum_i (g_taken[i] Q[i][action[i]] + sum_j g_all[i][j] Q[i][j])         (dz_ij = g_all[i][j] + [j == action[i]] g_taken[i])
to every parameter.  float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every
per-row contribution is formed in float32 and the batch is summed by plain sequential float32 accumulation (G32seq), as
tests/policy_grad_model.py, whose _forward / _backward / _sum_rows / flat / grad_tolerances are used as they are (flat names a result's
first net "actor": the gradients are kept under that key)."""
import numpy as np

from policy_grad_model import _backward, _forward, _sum_rows, flat, grad_tolerances  # noqa: F401  (_sum_rows, flat, grad_tolerances: re-exported)
from policy_model import u23
from replay_model import philox4x32_10

STREAM_DQN = 7
ACTIONS = 6
NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS


def words(seed, step, env_global):
    """the four Philox words of env-steps (seed, step, env_global[...]): key = seed, counter = (env, step lo, step hi, 7)"""
    seed, step = int(seed), int(step)
    env = np.asarray(env_global, np.uint64)
    return philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (env, step & 0xFFFFFFFF, step >> 32, STREAM_DQN))


def random_dqn(rng, obs_dim, hidden, n_hidden):
    """dense random float32 net with a head of 6 (uniform in +-1 / sqrt(fan_in), as policy_model.random_policy's nets)"""
    dims = [obs_dim] + [hidden] * n_hidden + [ACTIONS]
    return [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.float32(np.sqrt(i)), rng.uniform(-1, 1, o).astype(np.float32) / np.float32(np.sqrt(i)))
            for i, o in zip(dims[:-1], dims[1:])]


def first_argmax(q):
    """the first j with q[i][j] = max_j q[i][j] (np.argmax's convention)"""
    return np.argmax(q, axis=1).astype(np.int32)


def evaluate(net, obs, action=None, g_taken=None, g_all=None, activation="relu", dtype=np.float64):
    """net: [(W, b), ...] with a head of 6.  obs [n, D]; action int [n] or None; g_taken [n], g_all [n, 6]: None means zeros.  Returns
    dict q_all [n, 6], q_taken [n] (None without an action), q_max [n], argmax int32 [n] and, when a g is given, actor: [(dW, db), ...]."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(obs)
    n = obs.shape[0]
    hs, pre, q = _forward(net, obs, activation, dtype)
    arg = first_argmax(q)
    out = dict(q_all=q.astype(dtype), q_max=q[np.arange(n), arg], argmax=arg, q_taken=None)
    onehot = None
    if action is not None:
        a = np.asarray(action, np.int64)
        out["q_taken"] = q[np.arange(n), a]
        onehot = (np.arange(ACTIONS)[None, :] == a[:, None]).astype(dtype)
    if g_taken is None and g_all is None:
        return out
    dz = np.zeros((n, ACTIONS), dtype) if g_all is None else np.asarray(g_all, dtype).copy()
    if g_taken is not None:
        dz = dz + onehot * np.asarray(g_taken, dtype)[:, None]
    out["actor"] = _backward(net, hs, pre, dz.astype(dtype), activation, dtype)
    return out


def act(net, obs, seed=0, step=0, epsilon=0.0, env_index_base=0, activation="relu", dtype=np.float64):
    """epsilon: a scalar or [B] per-env values, compared as the float32 the engine holds.  Returns dict explore bool [B], random_action
    int32 [B] (what an exploring env takes: drawn for every env), q [B, 6], argmax int32 [B] and action int32 [B] (the model's own
    argmax where the env does not explore: a near-tie of two Q values may round the other way in float32)."""
    B = np.asarray(obs).shape[0]
    o = words(seed, step, int(env_index_base) + np.arange(B))
    eps = np.broadcast_to(np.asarray(epsilon, np.float32), (B,)).astype(np.float64)
    explore = u23(o[0]) < eps  # (a NaN never explores)
    rnd = ((o[1].astype(np.uint64) * np.uint64(ACTIONS)) >> np.uint64(32)).astype(np.int32)
    ev = evaluate(net, obs, activation=activation, dtype=dtype)
    return dict(explore=explore, random_action=rnd, q=ev["q_all"], argmax=ev["argmax"], action=np.where(explore, rnd, ev["argmax"]).astype(np.int32))


def case(obs_dim, n, hidden, n_hidden, seed):
    """The shared inputs of a (net, n) case, CPU and GPU tests alike: net, obs [n, D], action int32 [n], g_taken [n], g_all [n, 6],
    float32 but for the actions"""
    rng = np.random.default_rng([seed, obs_dim, n, hidden, n_hidden])
    net = random_dqn(rng, obs_dim, hidden, n_hidden)
    obs = rng.standard_normal((n, obs_dim)).astype(np.float32)
    action = rng.integers(0, ACTIONS, n).astype(np.int32)
    gt = rng.standard_normal(n).astype(np.float32)
    ga = rng.standard_normal((n, ACTIONS)).astype(np.float32)
    return dict(net=net, obs=obs, action=action, g_taken=gt, g_all=ga)


# (obs_dim, n, hidden, n_hidden, activation): the gradient cases tests/test_gpu_dqn.py runs; tests/test_dqn.py checks on the CPU that
# each one's tolerance is at most 1 % of its tensor's largest gradient.  obs_dim 15: GoalDiscrete3-v0, 10: KeplerDiscrete-v0.
GRAD_NS = [1, 200, 2049]
BIG_N = 256 * 64 + 300  # hidden 128 has workgroups of 64 rows: past the grid cap of 256 they take a second row tile
CASE_SEED = 0  # case(..., seed=CASE_SEED + n + hidden): chosen on the CPU so that every case keeps the 1 % cap


def grad_cases():
    """both activations on every net at n = 200; at the other row counts the activations alternate over the nets"""
    cases = []
    for n in GRAD_NS:
        for i, (hidden, n_hidden) in enumerate(NETS):
            for activation in ("tanh", "relu") if n == 200 else (("tanh", "relu")[i % 2],):
                cases.append((15 if i % 2 == 0 else 10, n, hidden, n_hidden, activation))
    cases.append((15, BIG_N, 128, 1, "relu"))
    return cases


def grad_case(obs_dim, n, hidden, n_hidden):
    return case(obs_dim, n, hidden, n_hidden, seed=CASE_SEED + n + hidden)


SELECTIONS = ("both", "taken", "all")


def grad_reference(c, activation, selection, dtype):
    """flat gradients of a case under a selection of the loss gradients"""
    gt = c["g_taken"] if selection in ("both", "taken") else None
    ga = c["g_all"] if selection in ("both", "all") else None
    return flat(evaluate(c["net"], c["obs"], c["action"], gt, ga, activation=activation, dtype=dtype))
