"""The contract of sg_ppo_grad_device (include/spacegym.h) in NumPy: the clipped PPO objective of the CleanRL / SB3
form on rows gathered from a flattened rollout, its statistics, the derivatives it feeds to the backward pass and, through
tests/policy_grad_model.py, the gradient of every parameter.  For entry i of the minibatch, r = index[i] (r = i without an index):
    lr = logp - old_logp[r];  ratio = exp(lr);  A = (adv[r] - mean) * rstd when normalising, else adv[r]
    pg = max(-A ratio, -A clamp(ratio, 1 - c, 1 + c))
    vl = 0.5 max((value - ret)^2, (vclip - ret)^2),  vclip = old_value + clamp(value - old_value, -cv, cv)   (cv given; else 0.5 (value - ret)^2)
    loss = mean(pg) - ent_coef mean(entropy) + vf_coef mean(vl)
    g_logp = -A ratio / n where the unclipped term is >= the clipped one, else 0;  g_entropy = -ent_coef / n
    g_value = vf_coef (value - ret) / n where the unclipped square is >= the clipped one, else vf_coef (vclip - ret) / n inside the clamp
              (bounds included) and 0 outside it
An index outside [0, rows) is clamped for every load; such an entry contributes zero to every gradient and statistic (to the advantage
statistics it counts as advantage 0), is counted in bad_rows, and the means still divide by n.  A policy without a critic ignores
vf_coef, has value_loss 0 and needs no ret.

float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every per-row term is formed
in float32 and every sum over the rows is plain sequential float32 accumulation, as policy_grad_model's; the advantage mean and
standard deviation are float64 sums rounded to float32 in both forms' float32 use, as the kernel's."""
import numpy as np

from policy_grad_model import _sum_rows, evaluate

STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "old_approx_kl", "clip_fraction", "adv_mean", "adv_std", "bad_rows",
         "reserved0", "reserved1")


def ppo(policy, batch, index=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True,
        adv_epsilon=1e-8, activation="tanh", dtype=np.float64):
    """policy: policy_model's dict.  batch: dict obs [rows, D] / action / logp / advantage / ret / value of NumPy arrays.
    Returns dict actor / critic / log_std (policy_grad_model.flat takes it), stats [12] named by STATS, rows (dict logp, value, g_logp,
    g_value: [n]), terms (the per-row terms of statistics 1 .. 6, zero for a bad entry), and the branch masks pg_unclipped / v_unclipped /
    v_inside ([n] bool) of the rows' max and clamp."""
    dtype = np.dtype(dtype).type
    rows = batch["obs"].shape[0]
    idx = np.arange(rows, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    n = idx.shape[0]
    good = (idx >= 0) & (idx < rows)
    r = np.clip(idx, 0, rows - 1)
    col = lambda k: np.asarray(batch[k])[r].astype(dtype)
    obs, action = np.asarray(batch["obs"])[r], np.asarray(batch["action"])[r]
    fwd = evaluate(policy, obs, action, activation=activation, dtype=dtype, grads=False)
    critic = policy["critic"] is not None
    nf, zero, one = dtype(n), dtype(0), dtype(1)
    # the advantage statistics: float64 whatever the dtype; a bad entry counts as advantage 0
    adv = col("advantage")
    mean = std = 0.0
    if normalize_advantage:
        a64 = np.where(good, np.asarray(batch["advantage"], np.float64)[r], 0.0)
        mean = a64.sum() / n
        std = np.sqrt(max(0.0, ((a64 - mean) ** 2).sum() / (n - 1)))
        adv = (adv - dtype(mean)) * dtype(1.0 / (std + adv_epsilon))
    lr = fwd["logp"] - col("logp")
    ratio = np.exp(lr)
    c = dtype(clip_range)
    t1, t2 = -adv * ratio, -adv * np.clip(ratio, one - c, one + c)
    pg_unclipped = t1 >= t2
    pg = np.where(pg_unclipped, t1, t2)
    g_logp = np.where(good & pg_unclipped, t1 / nf, zero).astype(dtype)
    g_entropy = np.where(good, -dtype(ent_coef) / nf, zero).astype(dtype)
    g_value = None
    vl = np.zeros(n, dtype)
    v_unclipped, v_inside = np.ones(n, bool), np.ones(n, bool)
    if critic:
        vf = dtype(vf_coef)
        d = fwd["value"] - col("ret")
        vl, g_value = dtype(0.5) * (d * d), vf * d / nf
        if clip_range_vf is not None:
            cv, ov = dtype(clip_range_vf), col("value")
            dv = fwd["value"] - ov
            e2 = (ov + np.clip(dv, -cv, cv)) - col("ret")
            v_unclipped, v_inside = d * d >= e2 * e2, (dv >= -cv) & (dv <= cv)
            vl = np.where(v_unclipped, vl, dtype(0.5) * (e2 * e2))
            g_value = np.where(v_unclipped, g_value, np.where(v_inside, vf * e2 / nf, zero))
        g_value = np.where(good, g_value, zero).astype(dtype)
    out = evaluate(policy, obs, action, g_logp, g_entropy, g_value, activation=activation, dtype=dtype)
    mean_of = lambda v: _sum_rows(np.where(good, v, zero).astype(dtype), dtype) / nf
    s = np.zeros(len(STATS), dtype)
    s[1], s[2], s[3] = mean_of(pg), mean_of(vl) if critic else zero, mean_of(fwd["entropy"])
    s[0] = s[1] - dtype(ent_coef) * s[3] + (dtype(vf_coef) * s[2] if critic else zero)
    s[4], s[5] = mean_of((ratio - one) - lr), mean_of(-lr)
    s[6] = mean_of((np.abs(ratio - one) > c).astype(dtype))
    s[7], s[8], s[9] = dtype(mean), dtype(std), dtype((~good).sum())
    terms = [pg, vl, fwd["entropy"], (ratio - one) - lr, -lr, (np.abs(ratio - one) > c).astype(dtype)]
    return dict(actor=out["actor"], critic=out["critic"], log_std=out["log_std"], stats=s, terms=[np.where(good, v, zero) for v in terms],
                rows=dict(logp=fwd["logp"], value=fwd["value"], g_logp=g_logp, g_value=g_value),
                pg_unclipped=pg_unclipped, v_unclipped=v_unclipped, v_inside=v_inside)
