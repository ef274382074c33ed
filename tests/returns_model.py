"""NumPy statement of sg_gae_groups_device / sg_vtrace_device (include/spacegym.h): GAE and V-trace targets with the
discounts of env i taken from row i // (B // G) of a float32 table [G, 2] of (gamma, lambda) rows.  Per env in float64 with every
operation rounded on its own, outputs rounded to float32 once; the HIP kernels reproduce both bit for bit (tests/test_gpu_returns.py).

GAE has one statement, gae_model.gae_model_f64: the grouped form calls it per block of B // G envs with gamma = float64(float32 g),
lambda = float64(float32 l) -- the kernel's gl = (double) g * (double) l is that product, exact before its one rounding.

V-trace (Espeholt et al. 2018, equation 1, with c_t = lambda min(c_bar, ratio)):
    acc = 0; v_next = last_value
    for t = K-1 .. 0:
        rc = rho_bar < rho ? rho_bar : rho          (cc with c_bar, rp with pg_rho_bar; a NaN ratio stays NaN)
        done:      nv = term;    vs_next = term      term = terminal value if truncated, bootstrapped and given, else 0
        otherwise: nv = v_next;  vs_next = v_next + acc
        delta = rc * ((r + gamma * nv) - v)
        acc   = done ? delta : delta + (gl * cc) * acc
        vs[t] = float32(acc + v);  pg_advantage[t] = float32(rp * ((r + gamma * vs_next) - v));  v_next = v
"""
import numpy as np

from gae_model import gae_model_f64


def _f32(x):
    with np.errstate(all="ignore"):
        return x.astype(np.float32)


def group_columns(B, G):
    """the env blocks of the G groups, as slices: env i belongs to group i // (B // G)"""
    if G < 1 or B % G:
        raise ValueError("G must divide B")
    n = B // G
    return [slice(g * n, (g + 1) * n) for g in range(G)]


def per_env(discounts, B):
    """the table as per-env float64 (gamma, gl) rows [B]: gl = gamma * lambda, exact in float64 before its one rounding"""
    d = np.asarray(discounts, np.float32).astype(np.float64)
    rows = np.repeat(np.arange(d.shape[0]), B // d.shape[0])
    if rows.size != B:
        raise ValueError("G must divide B")
    with np.errstate(all="ignore"):
        return d[rows, 0], d[rows, 0] * d[rows, 1]


def gae_groups_model(reward, done, trunc, discounts, value=None, last_value=None, terminal_value=None, bootstrap_truncated=True):
    """discounts float32 [G, 2]; the rest as gae_model -> (advantage, ret) float32 [K, B]: gae_model_f64 on each group's columns"""
    reward = np.asarray(reward, np.float32)
    K, B = reward.shape
    discounts = np.asarray(discounts, np.float32)
    A, R = np.empty((K, B)), np.empty((K, B))
    cut = lambda a, c: None if a is None else np.asarray(a)[..., c]  # noqa: E731
    for g, cols in enumerate(group_columns(B, discounts.shape[0])):
        A[:, cols], R[:, cols] = gae_model_f64(reward[:, cols], cut(done, cols), cut(trunc, cols), cut(value, cols), cut(last_value, cols),
                                               cut(terminal_value, cols), np.float64(discounts[g, 0]), np.float64(discounts[g, 1]),
                                               bootstrap_truncated)
    return _f32(A), _f32(R)


def vtrace_model(reward, done, trunc, value, last_value=None, ratio=None, terminal_value=None, gamma=0.99, lam=1.0, discounts=None,
                 rho_bar=1.0, c_bar=1.0, pg_rho_bar=None, bootstrap_truncated=True):
    """-> (vs, pg_advantage) float32 [K, B]"""
    return tuple(_f32(x) for x in vtrace_model_f64(reward, done, trunc, value, last_value, ratio, terminal_value, gamma, lam, discounts,
                                                  rho_bar, c_bar, pg_rho_bar, bootstrap_truncated))


def vtrace_model_f64(reward, done, trunc, value, last_value=None, ratio=None, terminal_value=None, gamma=0.99, lam=1.0, discounts=None,
                     rho_bar=1.0, c_bar=1.0, pg_rho_bar=None, bootstrap_truncated=True):
    """the same before the one rounding to float32.  discounts None: the scalars gamma and lam, gl = gamma * lam rounded once"""
    reward = np.asarray(reward, np.float32)
    K, B = reward.shape
    done, trunc = np.asarray(done).astype(bool), np.asarray(trunc).astype(bool)
    r, v = reward.astype(np.float64), np.asarray(value, np.float32).astype(np.float64)
    rho = np.ones((K, B)) if ratio is None else np.asarray(ratio, np.float32).astype(np.float64)
    v_next = np.zeros(B) if last_value is None else np.asarray(last_value, np.float32).astype(np.float64)
    use_tv = bool(bootstrap_truncated) and terminal_value is not None
    tv = np.asarray(terminal_value, np.float32).astype(np.float64) if use_tv else None
    if discounts is None:
        gamma = np.float64(gamma)
        gl = gamma * np.float64(lam)
    else:
        gamma, gl = per_env(discounts, B)
    rho_bar, c_bar = np.float64(rho_bar), np.float64(c_bar)
    pg_rho_bar = rho_bar if pg_rho_bar is None else np.float64(pg_rho_bar)
    vs, pg = np.empty((K, B)), np.empty((K, B))
    acc = np.zeros(B)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            d = done[t]
            rc, cc, rp = (np.where(bar < rho[t], bar, rho[t]) for bar in (rho_bar, c_bar, pg_rho_bar))
            term = np.where(trunc[t], tv[t], 0.0) if use_tv else np.zeros(B)
            nv = np.where(d, term, v_next)
            vs_next = np.where(d, term, v_next + acc)
            delta = rc * ((r[t] + gamma * nv) - v[t])
            acc = np.where(d, delta, delta + (gl * cc) * acc)
            vs[t] = acc + v[t]
            pg[t] = rp * ((r[t] + gamma * vs_next) - v[t])
            v_next = v[t]
    return vs, pg


# The shapes of tests/test_gpu_returns.py.  K: 1, 1, 2, 3, 3, 4 and 7 stages of the GAE kernel's 8 rows, 1, 2, 2, 3, 4, 5 and 9 of the
# V-trace kernel's 6 -- every exit of the three-way stage rotation, and a wrap, in both.  (B, G): blocks of 80 put a group boundary
# inside a wave; 65 is an odd row length and a partial wave.
STAGE_ROWS = (8, 6)  # kGaeRows, kVtraceRows
KS = (1, 8, 9, 17, 24, 25, 49)
BLOCKS = ((240, 1), (240, 3), (240, 240), (65, 1), (65, 5), (65, 65), (1, 1))
CASES = [(K, B, G) for B, G in BLOCKS for K in KS]


def returns_case(K, B, G, seed=None):
    """the inputs of one test case (shared by the CPU and the GPU tests): gae_model.synthetic at p_done = 0.1, G distinct rows with gamma
    in [0.9, 0.999] and lambda in [0.8, 1], ratios exp(0.5 N(0, 1)) -- about half exceed a bar of 1"""
    from gae_model import synthetic
    seed = 1000 * K + B + G + 4 if seed is None else seed  # (+ 4: at K = 9, B = 1 most seeds force a done step onto the stage boundary)
    s = synthetic(K, B, seed=seed, p_done=0.1)
    rng = np.random.default_rng(seed + 7919)
    discounts = np.stack([rng.uniform(0.9, 0.999, G), rng.uniform(0.8, 1.0, G)], 1).astype(np.float32)
    ratio = np.exp(0.5 * rng.standard_normal((K, B))).astype(np.float32)
    return s, discounts, ratio
