"""The contract of the PBT calls (include/spacegym.h, sg_pbt_*) in NumPy: member fitness from rollout rows with
its summation order, truncation selection with its ranking and draws, explore with its three modes, each operation rounded on its
own in the format the kernel uses."""
import math

import numpy as np

from replay_model import philox4x32_10

NAMES = ("episodes", "return_sum", "length_sum", "return_sq_sum", "return_max", "return_min", "fitness", "reserved")
EPISODES, RETURN_SUM, LENGTH_SUM, RETURN_SQ_SUM, RETURN_MAX, RETURN_MIN, FITNESS, RESERVED = range(8)
CHUNK = 256        # envs per chunk of the reduction
MAX_MEMBERS = 256
MAX_COLUMNS = 16
STREAM_SELECT, STREAM_EXPLORE = 9, 10
COPY, SCALE, SCALE_COMPLEMENT = 0, 1, 2
IDENTITY = (0.0, 0.0, 0.0, 0.0, -np.inf, np.inf)  # of (episodes, return_sum, length_sum, return_sq_sum, return_max, return_min)


def _combine(a, b):
    """(+, +, +, +, max, min) of two [..., 6] blocks; fmax / fmin return the other operand of a NaN"""
    out = np.empty_like(a)
    out[..., :4] = a[..., :4] + b[..., :4]
    out[..., 4] = np.fmax(a[..., 4], b[..., 4])
    out[..., 5] = np.fmin(a[..., 5], b[..., 5])
    return out


def fresh_table(P):
    t = np.zeros((P, 8))
    t[:, RETURN_MAX], t[:, RETURN_MIN], t[:, FITNESS] = -np.inf, np.inf, np.nan
    return t


def workspace_bytes(B, P):
    return P * (-(-(B // P) // CHUNK)) * 6 * 8


def env_windows(reward, done, env_return, env_length):
    """pass 1: per env, the six values over the episodes finished inside the rows, and the running (return, length) afterwards"""
    K, B = reward.shape
    run, ln = np.array(env_return, np.float64), np.array(env_length, np.int32)
    w = np.tile(np.array(IDENTITY), (B, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(K):
            run = run + reward[t].astype(np.float64)
            ln = ln + np.int32(1)
            d = np.asarray(done[t]) != 0
            fin = np.stack([np.ones(B), run, ln.astype(np.float64), run * run, run, run], axis=1)
            w = np.where(d[:, None], _combine(w, fin), w)
            run = np.where(d, 0.0, run)
            ln = np.where(d, np.int32(0), ln).astype(np.int32)
    return w, run, ln


def member_windows(w, P):
    """pass 2: chunks of 256 consecutive envs of a member's block, lanes past E holding the identities, reduced by the tree
    x[l] = x[l] (+) x[l + s], s = 128 .. 1; then the chunks in ascending order, starting from chunk 0's"""
    B = w.shape[0]
    E = B // P
    out = np.empty((P, 6))
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(P):
            acc = None
            for c0 in range(0, E, CHUNK):
                x = np.tile(np.array(IDENTITY), (CHUNK, 1))
                n = min(CHUNK, E - c0)
                x[:n] = w[m * E + c0:m * E + c0 + n]
                s = CHUNK // 2
                while s:
                    x[:s] = _combine(x[:s], x[s:2 * s])
                    s //= 2
                acc = x[0].copy() if acc is None else _combine(acc, x[0])
            out[m] = acc
    return out


def fitness_update(table, env_return, env_length, reward, done):
    """-> (table, env_return, env_length) after sg_pbt_fitness_device on reward float32 [K, B], done [K, B]"""
    reward = np.asarray(reward, np.float32)
    P = table.shape[0]
    assert reward.shape[1] % P == 0
    w, run, ln = env_windows(reward, done, env_return, env_length)
    mw = member_windows(w, P)
    new = np.array(table, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        new[:, :6] = _combine(new[:, :6], mw)
        ep = new[:, EPISODES]
        new[:, FITNESS] = np.where(ep >= 1.0, new[:, RETURN_SUM] / np.where(ep >= 1.0, ep, 1.0), np.nan)
    return new, run, ln


def fitness_clear(table, src=None):
    new = np.array(table, np.float64)
    rows = np.ones(len(new), bool) if src is None else np.asarray(src) != np.arange(len(new))
    new[rows] = fresh_table(1)[0]
    return new


def truncation_count(fraction, P):
    """the k the host passes"""
    assert 0.0 < fraction <= 0.5
    return int(math.floor(fraction * P))


def _step_words(step, step_dev=0):
    step = (int(step) + int(step_dev)) & 0xFFFFFFFFFFFFFFFF  # a 64-bit sum
    return step & 0xFFFFFFFF, step >> 32


def select(fitness, ready=None, k=0, seed=0, step=0, step_dev=0):
    """-> (src int32 [P], rank int32 [P] (-1: not taking part), (copies, k_eff))"""
    f = np.asarray(fitness, np.float64)
    P = len(f)
    assert 1 <= P <= MAX_MEMBERS and 0 <= k <= P // 2
    part = ~np.isnan(f) & (np.ones(P, bool) if ready is None else np.asarray(ready) != 0)
    r = int(part.sum())
    idx = np.arange(P)
    with np.errstate(invalid="ignore"):  # ahead[m, j]: j takes part and is ranked before m (all pairs: exact)
        ahead = part[None, :] & ((f[None, :] > f[:, None]) | ((f[None, :] == f[:, None]) & (idx[None, :] < idx[:, None])))
    rank = np.where(part, ahead.sum(axis=1), -1).astype(np.int32)
    k_eff = min(int(k), r // 2)
    by_rank = {int(rank[m]): m for m in range(P) if part[m]}
    lo, hi = _step_words(step, step_dev)
    seed = int(seed)
    o0 = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (np.arange(P), lo, hi, STREAM_SELECT))[0]
    src = np.arange(P, dtype=np.int32)
    for m in range(P):
        if part[m] and rank[m] >= r - k_eff:
            src[m] = by_rank[(int(o0[m]) * k_eff) >> 32]
    return src, rank, (k_eff, k_eff)


def exploit_sources(src):
    """adam_model.exploit_sources' rule: (the source of every copy that is performed, else -1; the refused copies)"""
    src = np.asarray(src, np.int64)
    P = len(src)
    out, refused = np.full(P, -1, np.int64), 0
    for m in range(P):
        s = int(src[m])
        if s == m:
            continue
        if 0 <= s < P and src[s] == s:
            out[m] = s
        else:
            refused += 1
    return out, refused


def column(tensor, col, mode, down=0.8, up=1.25, lo=-np.inf, hi=np.inf):
    return dict(tensor=tensor, col=col, mode=mode, down=down, up=up, lo=lo, hi=hi)


def explore_bits(P, n_columns, seed=0, step=0, step_dev=0):
    """[n_columns, P] bool: True where the draw of (column, member) takes `up`"""
    lo, hi = _step_words(step, step_dev)
    seed = int(seed)
    c, m = np.meshgrid(np.arange(n_columns), np.arange(P), indexing="ij")
    o0 = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (((c << 16) | m).ravel(), lo, hi, STREAM_EXPLORE))[0]
    return ((o0 >> np.uint64(31)) != 0).reshape(n_columns, P)


def explore(src, columns, seed=0, step=0, step_dev=0):
    """columns: column(...) dicts whose tensors are float32 [P, C] arrays, changed IN PLACE; -> the refused copies"""
    performed, refused = exploit_sources(src)
    P = len(performed)
    assert 1 <= len(columns) <= MAX_COLUMNS
    up = explore_bits(P, len(columns), seed, step, step_dev)
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, spec in enumerate(columns):
            t = spec["tensor"]
            assert t.dtype == np.float32 and t.shape[0] == P
            for m in range(P):
                if performed[m] < 0:
                    continue
                v = t[performed[m], spec["col"]]
                f = np.float32(spec["up"] if up[c, m] else spec["down"])
                if spec["mode"] == COPY:
                    x = v
                elif spec["mode"] == SCALE:
                    x = np.float32(v * f)
                else:
                    assert spec["mode"] == SCALE_COMPLEMENT
                    x = np.float32(one - np.float32(np.float32(one - v) * f))
                t[m, spec["col"]] = np.fmin(np.fmax(x, np.float32(spec["lo"])), np.float32(spec["hi"]))
    return refused
