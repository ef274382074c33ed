"""The contract of sg_policy_act_device / sg_rollout_policy_device (include/spacegym.h, sg_policy) in NumPy: the two
MLPs in torch.nn.Linear layout, the Philox block of an env-step, the Gaussian and the categorical draw and their log-probs.  The
statement is float64 (`dtype=np.float64`, the default): the same float32 parameters and observations, promoted.  With
`dtype=np.float32` the same formulas run in float32 on the CPU -- the yardstick for "a correct float32 implementation" that the GPU
tests derive their tolerances from."""
import numpy as np

from replay_model import philox4x32_10

STREAM_POLICY = 5
LOG_SQRT_2PI = 0.9189385332046727


def u23(w):
    """((w >> 9) + 0.5) / 2^23 in (0, 1): exact in float32 and float64"""
    return ((np.asarray(w, np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0


def words(seed, step, env_global):
    """the four Philox words of env-steps (seed, step, env_global[...]): key = seed, counter = (env, step lo, step hi, 5)"""
    seed, step = int(seed), int(step)
    env = np.asarray(env_global, np.uint64)
    return philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (env, step & 0xFFFFFFFF, step >> 32, STREAM_POLICY))


def mlp(layers, x, activation, dtype=np.float64):
    """layers [(W [out, in], b [out]), ...]: activation after every layer but the last"""
    h = np.asarray(x, dtype)
    for l, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, dtype).T + np.asarray(b, dtype)
        if l < len(layers) - 1:
            h = np.tanh(h) if activation == "tanh" else np.maximum(h, dtype(0))
    return h


def random_policy(rng, obs_dim, hidden, n_hidden, head, critic=True, continuous=True):
    """dense random float32 parameters (uniform in +-1 / sqrt(fan_in), as nn.Linear's default): an indexing error moves an output
    by O(0.1)"""
    def net(out):
        dims = [obs_dim] + [hidden] * n_hidden + [out]
        return [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.float32(np.sqrt(i)), rng.uniform(-1, 1, o).astype(np.float32) / np.float32(np.sqrt(i)))
                for i, o in zip(dims[:-1], dims[1:])]
    return dict(actor=net(head), critic=net(1) if critic else None,
                log_std=rng.uniform(-1.0, 0.0, 2).astype(np.float32) if continuous else None)


def act(policy, obs, seed=0, step=0, env_index_base=0, deterministic=False, activation="tanh", dtype=np.float64, action=None):
    """policy: dict actor / critic (lists of (W, b); critic may be None) / log_std (None: a discrete id).  obs [B, D].
    Returns a dict: action, logp, value (None without a critic), and the intermediates the tests look at -- continuous: mean,
    eps [B, 2]; discrete: logits, cum [B, 6] (running sums of p), total, want = u * total.  `action` (discrete) scores the given
    actions instead of the drawn ones."""
    obs = np.asarray(obs)
    B = obs.shape[0]
    head = mlp(policy["actor"], obs, activation, dtype)
    value = mlp(policy["critic"], obs, activation, dtype)[:, 0] if policy["critic"] is not None else None
    o = words(seed, step, int(env_index_base) + np.arange(B))
    out = dict(value=value)
    if policy["log_std"] is not None:
        ls = np.asarray(policy["log_std"], dtype)
        if deterministic:
            eps = np.zeros((B, 2), dtype)
        else:
            r = np.sqrt(dtype(-2) * np.log(u23(o[0]).astype(dtype)))
            ang = dtype(2 * np.pi) * u23(o[1]).astype(dtype)
            eps = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).astype(dtype)
        out.update(mean=head, eps=eps, action=head + np.exp(ls) * eps,
                   logp=(dtype(-0.5) * eps * eps - ls - dtype(LOG_SQRT_2PI)).sum(axis=1))
    else:
        mx = head.max(axis=1, keepdims=True)
        p = np.exp(head - mx)
        cum = np.cumsum(p, axis=1)
        total = cum[:, -1]
        want = u23(o[0]).astype(dtype) * total
        if action is not None:
            a = np.asarray(action, np.int64)
        elif deterministic:
            a = head.argmax(axis=1)  # the first maximum
        else:
            a = (cum >= want[:, None]).argmax(axis=1)  # the first index whose running sum reaches u * total
        logp = (head[np.arange(B), a] - mx[:, 0]) - np.log(total)
        out.update(logits=head, cum=cum, total=total, want=want, action=a.astype(np.int32), logp=logp)
    return out
