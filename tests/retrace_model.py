"""NumPy statement of sg_retrace_device (include/spacegym.h): Retrace(lambda) / Q(lambda) targets over a time-major
sequence batch [L, n], and the optional loss outputs.  Per column in float64 with every operation rounded on its own, the target rounded
to float32 once; the loss outputs in float32.  The HIP kernel reproduces all of it bit for bit (tests/test_gpu_retrace.py).

    carry = 0; v_next = last_value
    for t = L-1 .. 0:
        boot = done ? (trunc and bootstrapped and given ? terminal_value : 0) : v_next + carry
        G = r + gamma * boot;  target[t] = float32(G)
        cc = c_bar < ratio ? c_bar : ratio            (ratio 1 if None; a NaN ratio stays NaN)
        carry = (lam * cc) * (G - q);  v_next = value

    td = q_online - target;  c = fmin(fmax(td, -delta), delta);  g = (w * c) / float32(L n)                       (float32)

discounts: None, or float32 [2] of (gamma, lam), widened -- the recurrence has no gamma * lam product, so the tensor form is the scalar
form at gamma = float64(float32 g), lam likewise.
"""
import numpy as np

ROWS = 4  # kRetraceRows: the rows of one stage of the kernel's rotation (tests/test_retrace.py checks it against the source)


def _f32(x):
    with np.errstate(all="ignore"):
        return x.astype(np.float32)


def retrace_model_f64(reward, done, trunc, q, value, last_value=None, ratio=None, terminal_value=None, gamma=0.99, lam=1.0, c_bar=1.0,
                      discounts=None, bootstrap_truncated=True):
    """-> G float64 [L, n], before the one rounding to float32"""
    reward = np.asarray(reward, np.float32)
    L, n = reward.shape
    done, trunc = np.asarray(done).astype(bool), np.asarray(trunc).astype(bool)
    r, qq, v = (np.asarray(x, np.float32).astype(np.float64) for x in (reward, q, value))
    rho = np.ones((L, n)) if ratio is None else np.asarray(ratio, np.float32).astype(np.float64)
    v_next = np.zeros(n) if last_value is None else np.asarray(last_value, np.float32).astype(np.float64)
    use_tv = bool(bootstrap_truncated) and terminal_value is not None
    tv = np.asarray(terminal_value, np.float32).astype(np.float64) if use_tv else None
    if discounts is not None:
        d = np.asarray(discounts, np.float32).astype(np.float64)
        gamma, lam = d[0], d[1]
    gamma, lam, c_bar = np.float64(gamma), np.float64(lam), np.float64(c_bar)
    G = np.empty((L, n))
    carry = np.zeros(n)
    with np.errstate(all="ignore"):
        for t in range(L - 1, -1, -1):
            term = np.where(trunc[t], tv[t], 0.0) if use_tv else np.zeros(n)
            boot = np.where(done[t], term, v_next + carry)
            G[t] = r[t] + gamma * boot
            cc = np.where(c_bar < rho[t], c_bar, rho[t])
            carry = (lam * cc) * (G[t] - qq[t])
            v_next = v[t]
    return G


def retrace_model(reward, done, trunc, q, value, last_value=None, ratio=None, terminal_value=None, gamma=0.99, lam=1.0, c_bar=1.0,
                  discounts=None, bootstrap_truncated=True, loss=None):
    """-> target float32 [L, n]; with loss = dict(q_online, weight=None, huber_delta=inf): (target, td_error, g)"""
    target = _f32(retrace_model_f64(reward, done, trunc, q, value, last_value, ratio, terminal_value, gamma, lam, c_bar, discounts,
                                    bootstrap_truncated))
    if loss is None:
        return target
    L, n = target.shape
    delta = np.float32(loss.get("huber_delta", np.inf))
    w = np.ones(n, np.float32) if loss.get("weight") is None else np.asarray(loss["weight"], np.float32)
    with np.errstate(all="ignore"):
        td = (np.asarray(loss["q_online"], np.float32) - target).astype(np.float32)
        c = np.fmin(np.fmax(td, -delta), delta).astype(np.float32)
        g = ((w[None, :] * c).astype(np.float32) / np.float32(L * n)).astype(np.float32)
    return target, td, g


# The shapes of tests/test_gpu_retrace.py.  L: 1, 1, 1, 2, 2, 3 and 13 stages of the kernel's 4 rows -- every exit of the three-way stage
# rotation and a wrap; n: one lane, a partial wave plus one, several waves of odd width.
LS = (1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS, 2 * ROWS + 1, 49)
NS = (1, 65, 240)
CASES = [(L, n) for n in NS for L in LS]


def stage_boundaries(L):
    """the first row (the latest step) of every stage after the first: the carry and v_next cross into it"""
    return [L - 1 - ROWS * c for c in range(1, (L + ROWS - 1) // ROWS)]


def case_fits(s):
    """what every GPU case must hold where its shape admits it: a done-and-truncated step and a done-only step (two steps needed), and a
    column that is not done at the first row of a later stage (L > ROWS needed)"""
    done, trunc = s["done"].astype(bool), s["trunc"].astype(bool)
    L = done.shape[0]
    kinds = done.size < 2 or ((done & trunc).any() and (done & ~trunc).any())
    return bool(kinds and (L <= ROWS or (~done[stage_boundaries(L)]).any()))


def retrace_case(L, n, seed=None):
    """the inputs of one test case (shared by the CPU and the GPU tests): gae_model.synthetic at p_done = 0.1 (reward, done, trunc,
    value, last_value, terminal_value; a done-and-truncated and a done-only step forced in), q and q_online around value, ratios
    exp(0.5 N(0, 1)) -- about half exceed a c_bar of 1 -- and per-column weights in [0.2, 1].  -> (s, extra): s the model's keyword
    arguments, extra = dict(ratio, q_online, weight)"""
    from gae_model import synthetic
    seed = 1000 * L + n + 2 if seed is None else seed
    while True:  # (the first seed from there whose flags fit: at L = 5, n = 1 the forced done steps sit on the only stage boundary)
        s = dict(synthetic(L, n, seed=seed, p_done=0.1))
        if case_fits(s):
            break
        seed += 1
    rng = np.random.default_rng(seed + 7919)
    s["q"] = (s["value"] + 0.5 * rng.standard_normal((L, n))).astype(np.float32)
    extra = dict(ratio=np.exp(0.5 * rng.standard_normal((L, n))).astype(np.float32),
                 q_online=(s["value"] + 1.5 * rng.standard_normal((L, n))).astype(np.float32),
                 weight=rng.uniform(0.2, 1.0, n).astype(np.float32))
    return s, extra
