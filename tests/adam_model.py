"""The per-member Adam / AdamW step with global-norm gradient clipping and the PBT exploit copy (sg_adam_step_device /
sg_adam_exploit_device; include/spacegym.h) in NumPy: the contract the kernels follow operation by operation.

dtype=np.float32 is the engine's arithmetic and gives its bits: the norm's squares and their sum in float64 in the kernel's order,
the per-member scalars in float64 and rounded once to float32, every per-element operation a float32 operation rounded on its own.
dtype=np.float64 is the same sequence with nothing rounded to float32 (hyper then holds Python floats as they are): the form
that is compared with torch.optim.Adam / AdamW and clip_grad_norm_ on float64 tensors.

tensors: a list of arrays [P, ...], one per parameter tensor; grads: the same, or None for a tensor without a gradient (it stays
out of the norm and of the update); hyper: [P, 8] in HYPER's order; state: float64 [P, 8] in STATE's order."""
import numpy as np

HYPER = ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm", "reserved", "reserved")
STATE = ("steps", "beta1_pow", "beta2_pow", "skipped", "grad_norm", "clip_scale", "step_size", "applied")
LR, BETA1, BETA2, EPS, WEIGHT_DECAY, MAX_GRAD_NORM = range(6)
STEPS, BETA1_POW, BETA2_POW, SKIPPED, GRAD_NORM, CLIP_SCALE, STEP_SIZE, APPLIED = range(8)
LANES = 1024  # adam_prepare_kernel's workgroup


def make_hyper(P, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, dtype=np.float32):
    """[P, 8]: every hyperparameter a scalar or a length-P sequence; max_grad_norm None is inf (no clipping)"""
    h = np.zeros((P, 8), dtype)
    clip = [np.inf if x is None else x for x in np.atleast_1d(np.asarray(max_grad_norm, object))]  # (None: off, also in a sequence)
    cols = (lr, betas[0], betas[1], eps, weight_decay, clip[0] if len(clip) == 1 else clip)
    for c, v in enumerate(cols):
        h[:, c] = np.broadcast_to(np.asarray(v, np.float64), (P,))
    return h


def fresh_state(P):
    s = np.zeros((P, 8), np.float64)
    s[:, BETA1_POW] = s[:, BETA2_POW] = 1.0
    return s


def sum_of_squares(member_grads):
    """the float64 sum of the squares of one member's gradient elements in the kernel's order: lane l of LANES takes elements
    l, l + LANES, ... of the first tensor, then of the next; then lane[i] += lane[i + s] for s = LANES / 2 .. 1"""
    acc = np.zeros(LANES, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in member_grads:
            sq = np.asarray(g, np.float64).reshape(-1) ** 2
            rows = np.zeros(-(-sq.size // LANES) * LANES, np.float64)
            rows[:sq.size] = sq
            for row in rows.reshape(-1, LANES):  # (the padding adds +0 to a sum that is never -0)
                acc = acc + row
        s = LANES // 2
        while s:
            acc = acc[:s] + acc[s:2 * s]
            s //= 2
    return acc[0]


def clip_scale(norm, max_grad_norm, dtype=np.float32):
    """torch's clip_grad_norm_ coefficient in float64, rounded once to dtype; 1 unless 0 < max_grad_norm < inf"""
    if max_grad_norm > 0 and max_grad_norm < np.inf:
        return dtype(min(1.0, np.float64(max_grad_norm) / (np.float64(norm) + 1e-6)))
    return dtype(1.0)


def adam_step(tensors, grads, exp_avg, exp_avg_sq, hyper, state, dtype=np.float32):
    """One call: returns new (tensors, exp_avg, exp_avg_sq, state); the inputs are left as they are."""
    f = dtype
    P = state.shape[0]
    hyper = np.asarray(hyper, f)
    tensors, exp_avg, exp_avg_sq = ([np.array(t, f) for t in ts] for ts in (tensors, exp_avg, exp_avg_sq))
    state = np.array(state, np.float64)
    live = [k for k, g in enumerate(grads) if g is not None]
    assert live, "no tensor has a gradient"
    for mem in range(P):
        h, st = hyper[mem], state[mem]
        with np.errstate(over="ignore", invalid="ignore"):
            norm = f(np.sqrt(sum_of_squares([np.asarray(grads[k], f)[mem] for k in live])))
        st[GRAD_NORM] = norm
        if not np.isfinite(norm):
            st[SKIPPED] += 1.0
            st[CLIP_SCALE] = st[STEP_SIZE] = st[APPLIED] = 0.0
            continue
        scale = clip_scale(norm, h[MAX_GRAD_NORM], f)
        b1p = st[BETA1_POW] * np.float64(h[BETA1])
        b2p = st[BETA2_POW] * np.float64(h[BETA2])
        with np.errstate(divide="ignore", invalid="ignore"):
            step_size = f(np.float64(h[LR]) / (1.0 - b1p))
            bc2s = f(np.sqrt(1.0 - b2p))
        st[STEPS] += 1.0
        st[BETA1_POW], st[BETA2_POW] = b1p, b2p
        st[CLIP_SCALE], st[STEP_SIZE], st[APPLIED] = scale, step_size, 1.0
        b1, b2, eps = h[BETA1], h[BETA2], h[EPS]
        omb1, omb2 = f(1.0) - b1, f(1.0) - b2
        lrwd = h[LR] * h[WEIGHT_DECAY]
        with np.errstate(all="ignore"):
            for k in live:
                g1 = np.asarray(grads[k], f)[mem] * scale
                m = b1 * exp_avg[k][mem] + omb1 * g1
                v = b2 * exp_avg_sq[k][mem] + (omb2 * g1) * g1
                den = np.sqrt(v) / bc2s + eps
                p = tensors[k][mem]
                p = (p - lrwd * p) - (step_size * m) / den
                assert m.dtype == f and v.dtype == f and p.dtype == f
                exp_avg[k][mem], exp_avg_sq[k][mem], tensors[k][mem] = m, v, p
    return tensors, exp_avg, exp_avg_sq, state


def exploit_sources(src):
    """(performed, refused): performed[m] is the member whose slices member m receives, or -1; refused counts the copies asked for
    (src[m] != m) that are not performed: a source outside [0, P), or one that is itself a destination"""
    src = np.asarray(src, np.int64)
    P = src.size
    performed = np.full(P, -1, np.int64)
    refused = 0
    for m in range(P):
        s = int(src[m])
        if s == m:
            continue
        if 0 <= s < P and src[s] == s:
            performed[m] = s
        else:
            refused += 1
    return performed, refused


def adam_exploit(tensors, exp_avg, exp_avg_sq, state, src):
    """returns new (tensors, exp_avg, exp_avg_sq, state, refused): the parameter and moment slices and state columns 0 .. 3 of every
    performed destination are its source's; everything else, hyper included, is untouched"""
    performed, refused = exploit_sources(src)
    tensors, exp_avg, exp_avg_sq = ([np.array(t) for t in ts] for ts in (tensors, exp_avg, exp_avg_sq))
    state = np.array(state, np.float64)
    for m, s in enumerate(performed):
        if s >= 0:
            for ts in (tensors, exp_avg, exp_avg_sq):
                for t in ts:
                    t[m] = t[s]
            state[m, :SKIPPED + 1] = state[s, :SKIPPED + 1]
    return tensors, exp_avg, exp_avg_sq, state, refused
