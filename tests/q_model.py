"""The contract of sg_q_evaluate_device / sg_q_grad_device / sg_policy_action_device / sg_policy_action_grad_device (include/spacegym.h;
DESIGN section 19) in NumPy: one or two Q critics on the row x = [obs | action], a hand-written backprop of
    sum_i (g_q1[i] Q_1[i] + g_q2[i] Q_2[i])
to every parameter and to the action, and the actor's action a = mean(obs) + exp(log_std) eps with the backprop of
sum_i g_action[i] . a[i] to the actor's parameters and log_std.  float64 by default.  With dtype=np.float32 it is the yardstick the GPU
tests derive their tolerances from: every per-row contribution is formed in float32 and the batch is summed by plain sequential
float32 accumulation, as tests/policy_grad_model.py (whose _forward / _backward / flat / grad_tolerances are used as they are)."""
import numpy as np

from policy_grad_model import _backward, _forward, _sum_rows, flat, grad_tolerances  # noqa: F401  (flat, grad_tolerances: re-exported)


def random_qnet(rng, obs_dim, hidden, n_hidden, n_critics=2):
    """dense random float32 critics on obs_dim + 2 inputs (uniform in +-1 / sqrt(fan_in), as policy_model.random_policy's nets)"""
    def net():
        dims = [obs_dim + 2] + [hidden] * n_hidden + [1]
        return [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.float32(np.sqrt(i)), rng.uniform(-1, 1, o).astype(np.float32) / np.float32(np.sqrt(i)))
                for i, o in zip(dims[:-1], dims[1:])]
    return [net() for _ in range(n_critics)]


def q_evaluate(critics, obs, action, g_q1=None, g_q2=None, activation="relu", dtype=np.float64, grads=True):
    """critics: a list of one or two nets [(W, b), ...].  obs [n, D], action [n, 2]; g_q*: [n] or None (zeros).
    Returns dict q: [Q_1, Q_2 or None] and, with grads, critics: per critic [(dW, db), ...] (zeros without its g) and
    action: [n, 2] = sum_c g_qc[i] dQ_c[i] / d action[i], critic 0's term first."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(obs)
    n = obs.shape[0]
    x = np.concatenate([np.asarray(obs, dtype), np.asarray(action, dtype)], axis=1)
    gs = [np.zeros(n, dtype) if g is None else np.asarray(g, dtype) for g in (g_q1, g_q2)]
    out = dict(q=[None, None])
    if grads:
        out.update(critics=[], action=np.zeros((n, 2), dtype))
    for c, layers in enumerate(critics):
        hs, pre, head = _forward(layers, x, activation, dtype)
        out["q"][c] = head[:, 0]
        if not grads:
            continue
        out["critics"].append(_backward(layers, hs, pre, gs[c][:, None], activation, dtype))
        # the walk once more, down to the input row: dx = W0^T dz0, its last two columns
        dz = gs[c][:, None]
        for l in range(len(layers) - 1, 0, -1):
            dh = dz @ np.asarray(layers[l][0], dtype)
            dz = dh * ((dtype(1) - hs[l] * hs[l]) if activation == "tanh" else (pre[l - 1] > 0).astype(dtype))  # relu'(0) = 0
        out["action"] = out["action"] + (dz @ np.asarray(layers[0][0], dtype)[:, -2:]).astype(dtype)
    return out


def q_flat(result):
    """{name: gradient array} of a q_evaluate() result or of q_grad_torch's dict turned to NumPy"""
    named = {}
    for c, pairs in enumerate(result["critics"]):
        for l, (W, b) in enumerate(pairs):
            named[f"critic{c}.{l}.weight"], named[f"critic{c}.{l}.bias"] = np.asarray(W), np.asarray(b)
    return named


def action(policy, obs, eps=None, g_action=None, activation="tanh", dtype=np.float64):
    """policy: policy_model's dict (continuous: log_std given; its critic is not used).  Returns dict action = mean + exp(log_std) eps
    (eps None: the mean) and, with g_action [n, 2], actor: [(dW, db), ...] and log_std: [2], the gradients of sum_i g_action[i] . a[i]."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(obs)
    hs, pre, mean = _forward(policy["actor"], obs, activation, dtype)
    std = np.exp(np.asarray(policy["log_std"], dtype))
    e = np.zeros(mean.shape, dtype) if eps is None else np.asarray(eps, dtype)
    out = dict(action=mean + std * e)
    if g_action is not None:
        ga = np.asarray(g_action, dtype)
        out["actor"] = _backward(policy["actor"], hs, pre, ga, activation, dtype)
        out["critic"] = None
        out["log_std"] = _sum_rows(ga * (std * e), dtype)
    return out
