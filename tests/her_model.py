"""The contract of sg_replay_relabel_device (include/spacegym.h) in NumPy, bit for bit: the draw, the window that
stops at an episode end and at the newest edge, the offset, the achieved position through the terminal join, the new goal columns in
float32 and the reward in delta form in float64 with every operation rounded on its own.  The ring is tests/replay_model.Ring."""
import numpy as np

from replay_model import M32, philox4x32_10, umul64hi

STREAM_HER = 12
FUTURE, FINAL = 0, 1


def threshold(her_ratio):
    """thr = floor(her_ratio 2^32 + 0.5), as the host computes it in float64"""
    return int(np.floor(np.float64(her_ratio) * np.float64(4294967296.0) + np.float64(0.5)))


def words(seed, call, n):
    """the four Philox words of rows 0 .. n - 1 of call number `call`"""
    j = np.arange(n, dtype=np.uint64)
    seed = int(seed)
    return philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (j & M32, j >> np.uint64(32), int(call) & 0xFFFFFFFF, STREAM_HER))


def window(ring, u, H):
    """m of every transition number u (all in range): min(H - 1, v - 1 - q, the first k with done[p_k, i])"""
    T, B, v = ring.T, ring.B, ring.valid
    u = np.asarray(u, np.int64)
    q, i = u // B, u % B
    first = (ring.head - v) % T
    m = np.minimum(H - 1, v - 1 - q)
    for k in range(H - 1):  # ascending: a later done never replaces an earlier one
        hit = (k < m) & (ring.done[(first + q + k) % T, i] != 0)
        m = np.where(hit, k, m)
    return m


def offsets(w, m, strategy):
    """k*: umul64hi(w0 | w1 << 32, m + 1) for future, m for final"""
    if strategy == FINAL:
        return np.asarray(m, np.int64).copy()
    lo, hi, n1 = np.asarray(w[0], np.uint64), np.asarray(w[1], np.uint64), np.asarray(m, np.uint64) + np.uint64(1)
    return ((hi * n1 + ((lo * n1) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)  # m + 1 < 2^31: exact in uint64


def achieved(ring, u, ks):
    """columns 0, 1 of s' of (p_k*, i): the terminal record where done, else the stored row"""
    T, B, v = ring.T, ring.B, ring.valid
    q, i = u // B, u % B
    p = ((ring.head - v) % T + q + ks) % T
    fin = ring.done[p, i] != 0
    slot = np.where(fin, ring.term_idx[p, i].astype(np.int64) % ring.C, 0)
    return np.where(fin[:, None], ring.term_obs[slot, :2], ring.obs[p, i, :2]).astype(np.float32)


def _norm(v0, v1):
    n2 = v0 * v0 + v1 * v1  # two products and a sum, each rounded (NumPy does not contract)
    return np.sqrt(n2), n2


def goal_term(a, b, goal_scale, sparse, goal_r2):
    """goal_scale (|a| - |b|) + (|b|^2 < goal_r2 ? sparse : 0) for float64 vectors a, b [n, 2]: the goal vector before and after"""
    la, _ = _norm(a[:, 0], a[:, 1])
    lb, b2 = _norm(b[:, 0], b[:, 1])
    return goal_scale * (la - lb) + np.where(b2 < goal_r2, sparse, 0.0)


def relabel_rows(obs, next_obs, reward, a, goal_scale, sparse, goal_r2, two_over_world, half_world):
    """Rows relabelled with the goal positions a [n, 2]: (obs, next_obs, reward) as the device writes them.  goal_scale and sparse
    are float64 scalars or arrays [n]; the arithmetic is the header's, operation by operation."""
    obs, next_obs = np.array(obs, np.float32), np.array(next_obs, np.float32)
    a = np.asarray(a, np.float32)
    tow, hw = np.float32(two_over_world), np.float64(np.float32(half_world))
    x0, x1 = obs[:, :2].copy(), next_obs[:, :2].copy()
    old = next_obs[:, -2:].astype(np.float64)  # the goal the reward was formed under: next_obs carries it
    vo1 = old * hw
    vo0 = vo1 + (x1.astype(np.float64) - x0.astype(np.float64))
    vn0 = a.astype(np.float64) - x0.astype(np.float64)
    vn1 = a.astype(np.float64) - x1.astype(np.float64)
    gs, sp = np.asarray(goal_scale, np.float64), np.asarray(sparse, np.float64)
    t_old = goal_term(vo0, vo1, gs, sp, np.float64(goal_r2))
    t_new = goal_term(vn0, vn1, gs, sp, np.float64(goal_r2))
    new_reward = ((np.asarray(reward, np.float32).astype(np.float64) - t_old) + t_new).astype(np.float32)
    obs[:, -2:] = (a - x0) * tow  # float32 subtract, float32 multiply
    next_obs[:, -2:] = (a - x1) * tow
    return obs, next_obs, new_reward


def relabel(ring, batch, consts, her_ratio=0.8, horizon=1, strategy=FUTURE, seed=0, profile=None):
    """What sg_replay_relabel_device leaves in `batch` (a dict with obs, next_obs, reward, steps, index and whatever else: copied,
    not modified) and the optional outputs: (batch, relabelled, offset, goal, ok).  consts: dict goal_scale, sparse, goal_r2,
    two_over_world, half_world; profile: (goal_scale [B], sparse [B]) of every env, replacing the first two.  Rows with ok False
    (index outside the ring) set the status word and are untouched, relabelled included; offset and goal are written where
    relabelled == 1 and are zero elsewhere here.  The call number is ring.sample_calls as it stands: it is not advanced."""
    out = {k: np.array(x) for k, x in batch.items()}
    n = out["index"].shape[0]
    B, v = ring.B, ring.valid
    cells = v * B
    relabelled, offset, goal = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
    if cells == 0:
        if n:
            ring.status = True
        return out, relabelled, offset, goal, np.zeros(n, bool)
    u = out["index"].astype(np.int64)
    ok = (u >= 0) & (u < cells)
    if not ok.all():
        ring.status = True
    single = out["steps"] == 1
    relabelled[ok & ~single] = 2
    w = words(seed, ring.sample_calls, n)
    act = ok & single & (w[2].astype(np.uint64) < np.uint64(threshold(her_ratio)))
    relabelled[act] = 1
    uu = np.where(act, u, 0)
    m = window(ring, uu, int(horizon))
    ks = offsets(w, m, strategy)
    a = achieved(ring, uu, ks)
    i = uu % B
    gs = consts["goal_scale"] if profile is None else np.asarray(profile[0], np.float64)[i]
    sp = consts["sparse"] if profile is None else np.asarray(profile[1], np.float64)[i]
    o, no, r = relabel_rows(out["obs"], out["next_obs"], out["reward"], a, gs, sp, consts["goal_r2"], consts["two_over_world"],
                            consts["half_world"])
    out["obs"][act], out["next_obs"][act], out["reward"][act] = o[act], no[act], r[act]
    offset[act] = ks[act]
    goal[act] = a[act]
    return out, relabelled, offset, goal, ok
