"""The contract of sg_policy_evaluate_device / sg_policy_grad_device (include/spacegym.h) in NumPy: log-prob,
entropy and value of GIVEN actions under the two MLPs of tests/policy_model.py, and a hand-written backprop of
    sum_i (g_logp[i] logp_i + g_entropy[i] entropy_i + g_value[i] value_i)
to every parameter.  float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every
per-row contribution to a gradient is formed in float32 and the batch is summed by plain sequential float32 accumulation
(np.add.accumulate), the least favourable fixed order a correct implementation could use."""
import numpy as np

from policy_model import LOG_SQRT_2PI


def _sum_rows(contrib, dtype):
    """sum over axis 0: float64 exactly as NumPy sums; float32 one row after the other"""
    if dtype == np.float64:
        return contrib.sum(axis=0)
    return np.add.accumulate(contrib, axis=0, dtype=np.float32)[-1]


def _forward(layers, x, activation, dtype):
    """activations [x, h_0, ..., h_{L-1}], pre-activations of the hidden layers, and the head's outputs"""
    hs, pre = [np.asarray(x, dtype)], []
    for l, (W, b) in enumerate(layers):
        z = hs[-1] @ np.asarray(W, dtype).T + np.asarray(b, dtype)
        if l == len(layers) - 1:
            return hs, pre, z
        pre.append(z)
        hs.append(np.tanh(z) if activation == "tanh" else np.maximum(z, dtype(0)))


def _backward(layers, hs, pre, dz, activation, dtype):
    """[(dW, db), ...] from dz [n, out] at the head"""
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        W = np.asarray(layers[l][0], dtype)
        dW = np.empty(W.shape, dtype)
        step = max(1, (1 << 22) // max(1, hs[l].size))  # output rows per pass: bounds the [n, rows, in] contributions
        for j in range(0, W.shape[0], step):
            dW[j:j + step] = _sum_rows(dz[:, j:j + step, None] * hs[l][:, None, :], dtype)
        grads[l] = (dW, _sum_rows(dz, dtype))
        if l:
            dh = dz @ W
            dz = dh * ((dtype(1) - hs[l] * hs[l]) if activation == "tanh" else (pre[l - 1] > 0).astype(dtype))  # relu'(0) = 0
    return grads


def evaluate(policy, obs, action, g_logp=None, g_entropy=None, g_value=None, activation="tanh", dtype=np.float64, grads=True):
    """policy: policy_model's dict.  obs [n, D]; action float [n, 2] (continuous) or int [n] (discrete).  g_*: [n] or None (zeros).
    Returns dict logp, entropy, value (None without a critic) and, with grads, actor / critic: [(dW, db), ...] (critic None without
    one; zeros without g_value), log_std: [2] or None."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(obs)
    n = obs.shape[0]
    g = lambda v: np.zeros(n, dtype) if v is None else np.asarray(v, dtype)
    gl, ge, gv = g(g_logp), g(g_entropy), g(g_value)
    hs, pre, head = _forward(policy["actor"], obs, activation, dtype)
    out = {}
    if policy["log_std"] is not None:
        ls = np.asarray(policy["log_std"], dtype)
        inv = np.exp(-ls)
        z = (np.asarray(action, dtype) - head) * inv
        out["logp"] = (dtype(-0.5) * z * z - ls - dtype(LOG_SQRT_2PI)).sum(axis=1)
        out["entropy"] = np.full(n, ls.sum() + dtype(1 + 2 * LOG_SQRT_2PI), dtype)
        dz = gl[:, None] * z * inv
        d_ls = _sum_rows(gl[:, None] * (z * z - dtype(1)) + ge[:, None], dtype)
    else:
        a = np.asarray(action, np.int64)
        mx = head.max(axis=1, keepdims=True)
        e = np.exp(head - mx)
        total = e.sum(axis=1, keepdims=True)
        logp_all = (head - mx) - np.log(total)
        p = e / total
        H = -(p * logp_all).sum(axis=1)
        out["logp"] = logp_all[np.arange(n), a]
        out["entropy"] = H
        onehot = (np.arange(head.shape[1])[None, :] == a[:, None]).astype(dtype)
        dz = gl[:, None] * (onehot - p) - ge[:, None] * p * (logp_all + H[:, None])
        d_ls = None
    out["value"] = None
    if grads:
        out["actor"] = _backward(policy["actor"], hs, pre, dz.astype(dtype), activation, dtype)
        out["log_std"] = d_ls
        out["critic"] = None
    if policy["critic"] is not None:
        hs, pre, v = _forward(policy["critic"], obs, activation, dtype)
        out["value"] = v[:, 0]
        if grads:
            out["critic"] = _backward(policy["critic"], hs, pre, gv[:, None], activation, dtype)
    return out


def flat(result):
    """{name: gradient array} of an evaluate() result or of policy_grad_torch's dict turned to NumPy"""
    named = {}
    for net in ("actor", "critic"):
        if result.get(net) is not None:
            for l, (W, b) in enumerate(result[net]):
                named[f"{net}.{l}.weight"], named[f"{net}.{l}.bias"] = np.asarray(W), np.asarray(b)
    if result.get("log_std") is not None:
        named["log_std"] = np.asarray(result["log_std"])
    return named


def grad_tolerances(g32, g64):
    """per tensor: 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) -- 8 x for another fixed order and FMA contraction (DESIGN section
    17's margin), the floor for tensors whose gradient is near zero"""
    return {k: 8.0 * float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) + 1e-6 * (1.0 + float(np.abs(g64[k]).max())) for k in g64}
