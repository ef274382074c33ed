"""The contract of the policy-population calls (include/spacegym.h, sg_policy_population_*) in NumPy.  A population is
P members of one architecture with their parameters stacked along a leading dimension (weight [P, out, in], bias [P, out], log_std
[P, 2]); member m owns the contiguous block of rows [m n, (m + 1) n).  The statement has no arithmetic of its own: it loops over the
members and calls tests/policy_model.py (act) and tests/policy_grad_model.py (evaluate, gradients) on each member's slice -- which is
exactly what the device promises, bit for bit against its own single-policy kernels."""
import numpy as np

import policy_grad_model
import policy_model
from policy_model import random_policy

OBS_DIM = 15  # GoalContinuous3P-v0 and GoalDiscrete3-v0
GROUP_CAP = 256  # kPolicyGradMaxGroups


def stack(policies):
    """policy_model policies of one shape -> the stacked population dict (actor / critic: [(W [P, out, in], b [P, out]), ...], log_std [P, 2])"""
    def net(key):
        if policies[0][key] is None:
            return None
        return [(np.stack([p[key][l][0] for p in policies]), np.stack([p[key][l][1] for p in policies])) for l in range(len(policies[0][key]))]
    return dict(actor=net("actor"), critic=net("critic"),
                log_std=np.stack([p["log_std"] for p in policies]) if policies[0]["log_std"] is not None else None)


def member(pop, m):
    """member m as a policy_model policy: views of the stacked arrays"""
    net = lambda layers: None if layers is None else [(W[m], b[m]) for W, b in layers]
    return dict(actor=net(pop["actor"]), critic=net(pop["critic"]), log_std=pop["log_std"][m] if pop["log_std"] is not None else None)


def members(pop):
    return int(pop["actor"][0][0].shape[0])


def random_population(rng, P, obs_dim, hidden, n_hidden, head, critic=True, continuous=True):
    """P independently drawn dense members: a wrong member offset moves an output by O(0.1)"""
    return stack([random_policy(rng, obs_dim, hidden, n_hidden, head, critic=critic, continuous=continuous) for _ in range(P)])


def act(pop, obs, seed=0, step=0, env_index_base=0, deterministic=False, activation="tanh", dtype=np.float64):
    """obs [B, D], B a multiple of P: env i acts under member i // (B / P); its noise is keyed by the global index env_index_base + i.
    Returns dict action, logp, value (None without critics) over all B rows."""
    P, B = members(pop), obs.shape[0]
    assert B % P == 0
    n = B // P
    parts = [policy_model.act(member(pop, m), obs[m * n:(m + 1) * n], seed=seed, step=step, env_index_base=env_index_base + m * n,
                              deterministic=deterministic, activation=activation, dtype=dtype) for m in range(P)]
    cat = lambda k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts])
    return dict(action=cat("action"), logp=cat("logp"), value=cat("value"))


def evaluate(pop, obs, action, g_logp=None, g_entropy=None, g_value=None, activation="tanh", dtype=np.float64, grads=True):
    """obs [P, n, D], action [P, n, 2] or int [P, n], g_* [P, n] or None.  Returns dict logp / entropy / value [P, n] and, with grads,
    actor / critic / log_std as policy_grad_model.evaluate's but stacked [P, ...]."""
    P = members(pop)
    sl = lambda g, m: None if g is None else g[m]
    parts = [policy_grad_model.evaluate(member(pop, m), obs[m], action[m], sl(g_logp, m), sl(g_entropy, m), sl(g_value, m),
                                        activation=activation, dtype=dtype, grads=grads) for m in range(P)]
    st = lambda k: None if parts[0][k] is None else np.stack([p[k] for p in parts])
    out = dict(logp=st("logp"), entropy=st("entropy"), value=st("value"))
    if grads:
        for key in ("actor", "critic"):
            out[key] = None if parts[0][key] is None else [
                (np.stack([p[key][l][0] for p in parts]), np.stack([p[key][l][1] for p in parts])) for l in range(len(parts[0][key]))]
        out["log_std"] = st("log_std")
    return out


def flat_member(result, m):
    """policy_grad_model.flat of member m's slices of a stacked gradient dict"""
    pick = lambda pairs: None if pairs is None else [(np.asarray(W)[m], np.asarray(b)[m]) for W, b in pairs]
    return policy_grad_model.flat(dict(actor=pick(result.get("actor")), critic=pick(result.get("critic")),
                                       log_std=np.asarray(result["log_std"])[m] if result.get("log_std") is not None else None))


# ---- how a member's rows group into workgroups (sg_policy_population_grad_device)
def grad_rows(hidden):
    """R, the rows of a workgroup's tile: policy_grad_block of the net's 32-output tiles"""
    nt = (hidden + 31) // 32
    return 256 if nt <= 1 else 128 if nt == 2 else 64


def groups_single(n, R):
    """sg_policy_grad_device's workgroups for n rows"""
    return min(-(-n // R), GROUP_CAP)


def groups(n, R, P):
    """G = min(ceil(n / R), max(1, 256 / P)), integer division"""
    return min(-(-n // R), max(1, GROUP_CAP // P))


def bit_equal_to_single(n, R, P):
    """member m's gradient is sg_policy_grad_device's bits at the same n: the rows group alike"""
    return -(-n // R) <= GROUP_CAP // P


def workspace_floats(n, R, P, total):
    return P * groups(n, R, P) * total


# ---- the gradient cases beyond the cap that tests/test_gpu_population.py runs; tests/test_population.py checks each one's tolerance
BEYOND_P = 3
BEYOND_CASES = [(5, 256), (40, 128), (97, 64)]  # (hidden, R): n = 85 R + 300 rows per member, one hidden layer, tanh
BEYOND_SEED = 0  # chosen on the CPU so that every case keeps the 1 % cap, per tensor and per member


def beyond_n(R):
    return (GROUP_CAP // BEYOND_P) * R + 300


def beyond_case(hidden, R):
    """the shared inputs of a beyond-the-cap case, CPU and GPU tests alike (continuous id)"""
    assert grad_rows(hidden) == R
    n = beyond_n(R)
    rng = np.random.default_rng([BEYOND_SEED, hidden, R])
    pop = random_population(rng, BEYOND_P, OBS_DIM, hidden, 1, 2)
    obs = rng.standard_normal((BEYOND_P, n, OBS_DIM)).astype(np.float32)
    action = rng.standard_normal((BEYOND_P, n, 2)).astype(np.float32)
    g = {k: rng.standard_normal((BEYOND_P, n)).astype(np.float32) for k in ("logp", "entropy", "value")}
    return dict(pop=pop, obs=obs, action=action, g=g, n=n)


def beyond_reference(c, dtype):
    return evaluate(c["pop"], c["obs"], c["action"], c["g"]["logp"], c["g"]["entropy"], c["g"]["value"], dtype=dtype)
