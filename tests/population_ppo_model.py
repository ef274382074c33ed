"""The contract of sg_ppo_population_grad_device (include/spacegym.h) in NumPy.  The statement has no arithmetic of
its own: for every member m it calls tests/ppo_model.py on member m's slices of the stacked parameters, with row m of the index and
member m's four coefficients, on the ONE flattened rollout all members share.  That is what the device promises: bit for bit against
sg_ppo_grad_device while a member's rows group as the single call groups them, the same sums in another grouping beyond."""
import numpy as np

from population_model import GROUP_CAP, groups, member, members, random_population, grad_rows
from ppo_model import STATS, ppo

COEF = ("clip_range", "clip_range_vf", "ent_coef", "vf_coef")  # the columns of coef [P, 4]
ADV_BLOCK, ADV_CAP = 1024, 256  # kPpoAdvBlock, kPpoAdvMaxGroups
SUMS = 8  # kPpoSums


def member_kwargs(coef, m, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5):
    """member m's coefficients as ppo_model.ppo's keywords: row m of coef [P, 4] when given (clip_range_vf <= 0 or NaN: off, by the
    comparison), else the call's scalars"""
    if coef is None:
        return dict(clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef)
    c = np.asarray(coef, np.float32)[m]
    return dict(clip_range=float(c[0]), clip_range_vf=float(c[1]) if c[1] > 0 else None, ent_coef=float(c[2]), vf_coef=float(c[3]))


def population_ppo(pop, batch, index=None, coef=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5,
                   normalize_advantage=True, adv_epsilon=1e-8, activation="tanh", dtype=np.float64):
    """pop: population_model's stacked dict.  batch: ppo_model's dict, `rows` rows shared by all members.  index: int64 [P, n], or None:
    member m takes rows [m n, (m + 1) n), n = rows // P.  coef: [P, 4] (COEF) or None.  Returns the list of ppo_model.ppo's results, one
    per member."""
    P, rows = members(pop), batch["obs"].shape[0]
    if index is None:
        n = rows // P
        assert n >= 1
        index = np.arange(P * n, dtype=np.int64).reshape(P, n)
    index = np.asarray(index, np.int64)
    assert index.shape[0] == P and index.ndim == 2
    return [ppo(member(pop, m), batch, index[m], normalize_advantage=normalize_advantage, adv_epsilon=adv_epsilon, activation=activation,
                dtype=dtype, **member_kwargs(coef, m, clip_range, clip_range_vf, ent_coef, vf_coef)) for m in range(P)]


def stats(results):
    """[P, 12]"""
    return np.stack([r["stats"] for r in results])


# ---- how a member's entries group into workgroups
def adv_groups_single(n):
    return min(-(-n // ADV_BLOCK), ADV_CAP)


def adv_groups(n, P):
    """Gadv = min(ceil(n / 1024), max(1, 256 / P)), integer division"""
    return min(-(-n // ADV_BLOCK), max(1, ADV_CAP // P))


def bit_equal_to_single(n, R, P):
    """member m's outputs are sg_ppo_grad_device's bits at the same n: both the parameter partials and the advantage partials group alike"""
    return -(-n // R) <= GROUP_CAP // P and -(-n // ADV_BLOCK) <= ADV_CAP // P


def workspace_bytes(n, R, P, total):
    """the parameter partials rounded up to 8 bytes, double [P][Gadv][2], float [P][G][8]"""
    G = groups(n, R, P)
    return (4 * P * G * total + 7) // 8 * 8 + 8 * 2 * P * adv_groups(n, P) + 4 * P * G * SUMS


# ---- the cases beyond the cap that tests/test_gpu_population_ppo.py runs; tests/test_population_ppo.py checks each one's 1 % cap
BEYOND_P, BEYOND_ROWS = 64, 2048  # 256 / P = 4 workgroups per member; the rollout of B = 256 envs, K = 8 steps
BEYOND_CASES = [(5, 256, 4 * 256 + 300), (40, 128, 4 * 128 + 300), (97, 64, 4 * 64 + 300), (5, 256, 4396)]  # (hidden, R, n per member)
BEYOND_KW = dict(normalize_advantage=True)


def beyond_coef(rng, P):
    """per-member coefficients that differ: clip_range 0.1 .. 0.3, clip_range_vf 0.1 .. 0.3 (every fourth member: off), ent_coef, vf_coef"""
    c = np.stack([rng.uniform(0.1, 0.3, P), rng.uniform(0.1, 0.3, P), rng.uniform(0.0, 0.02, P), rng.uniform(0.25, 1.0, P)], axis=1).astype(np.float32)
    c[::4, 1] = 0.0
    return c


def synthetic_batch(rng, pop, rows, continuous, activation="tanh"):
    """a flattened rollout whose stored logp / value lie around those of member 0 .. P - 1 in turn (row r by member r % P), so that both
    branches of both max occur in every member; tests/test_ppo.py's generator, per member"""
    from policy_grad_model import evaluate
    P, D = members(pop), pop["actor"][0][0].shape[2]
    obs = rng.standard_normal((rows, D)).astype(np.float32)
    action = rng.standard_normal((rows, 2)).astype(np.float32) if continuous else rng.integers(0, 6, rows).astype(np.int32)
    logp, value = np.zeros(rows), np.zeros(rows)
    for m in range(P):
        sel = np.arange(m, rows, P)
        now = evaluate(member(pop, m), obs[sel], action[sel], activation=activation, grads=False)
        logp[sel] = now["logp"]
        if now["value"] is not None:
            value[sel] = now["value"]
    batch = dict(obs=obs, action=action, logp=(logp + 0.3 * rng.standard_normal(rows)).astype(np.float32),
                 advantage=(0.5 + 2.0 * rng.standard_normal(rows)).astype(np.float32))
    if pop["critic"] is not None:
        batch["value"] = (value + 0.3 * rng.standard_normal(rows)).astype(np.float32)
        batch["ret"] = (value + 0.5 + rng.standard_normal(rows)).astype(np.float32)  # (off centre, as returns are: the head bias's gradient is dense)
    return batch


def beyond_case(hidden, R, n, continuous=True):
    """the shared inputs of a beyond-the-cap case, for the CPU and the GPU tests alike: P = 64 one-hidden-layer tanh members, a synthetic
    rollout of 2 048 rows, random indices with repeats, per-member coefficients"""
    assert grad_rows(hidden) == R and not bit_equal_to_single(n, R, BEYOND_P)
    rng = np.random.default_rng([7, hidden, n, int(continuous)])
    pop = random_population(rng, BEYOND_P, 15, hidden, 1, 2 if continuous else 6, continuous=continuous)
    batch = synthetic_batch(rng, pop, BEYOND_ROWS, continuous)
    index = rng.integers(0, BEYOND_ROWS, (BEYOND_P, n)).astype(np.int64)
    return dict(pop=pop, batch=batch, index=index, coef=beyond_coef(rng, BEYOND_P), n=n)


def beyond_reference(c, dtype, members_subset=None):
    """ppo_model's results of the case's members (all, or the listed ones: the rest are None)"""
    out = [None] * BEYOND_P
    for m in (range(BEYOND_P) if members_subset is None else members_subset):
        out[m] = ppo(member(c["pop"], m), c["batch"], c["index"][m], dtype=dtype, **BEYOND_KW, **member_kwargs(c["coef"], m))
    return out


def magnitudes(m64, kw, critic):
    """the float64 magnitude of each statistic 0 .. 8: for a mean the mean of the absolute per-row terms (for loss: of its three parts,
    weighted by the coefficients); adv_mean is measured against adv_std (tests/test_gpu_ppo.py's rule)"""
    t = [float(np.abs(v).mean()) for v in m64["terms"]]
    loss = t[0] + kw.get("ent_coef", 0.0) * t[2] + (kw.get("vf_coef", 0.5) * t[1] if critic else 0.0)
    std = float(m64["stats"][8])
    return [loss] + t + [max(abs(float(m64["stats"][7])), std), std]
