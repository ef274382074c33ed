"""NumPy statement of sg_gae_device / sg_gae (include/spacegym.h): generalized advantage estimation over a
rollout of K steps of B envs, per env in float64 with every operation rounded on its own, outputs rounded to float32 once.  The
HIP kernel reproduces it bit for bit (tests/test_gpu_gae.py); tests/test_gae.py checks it against the textbook sum.

    A = 0
    for t = K-1 .. 0:
        done:      nv = terminal value of (t, i) if truncated, bootstrapped and terminal values are given, else 0
                   A  = (r + gamma * nv) - v
        otherwise: nv = value[t + 1] (t = K-1: last_value)
                   A  = ((r + gamma * nv) - v) + gl * A              gl = gamma * lam, rounded once
        advantage[t] = float32(A);  ret[t] = float32(A + v)
"""
import numpy as np


def dense_from_list(K, B, count, step_env, value):
    """the list form as dense rows: value[k] at (step_env[k, 0], step_env[k, 1]) for k < min(count, capacity); records outside
    the rollout are ignored (the device reports them and a count past the capacity through the status word)"""
    dense = np.zeros((K, B), np.float32)
    step_env, value = np.asarray(step_env), np.asarray(value, np.float32)
    n = min(int(count), step_env.shape[0])
    t, i = step_env[:n, 0], step_env[:n, 1]
    ok = (t >= 0) & (t < K) & (i >= 0) & (i < B)
    dense[t[ok], i[ok]] = value[:n][ok]
    return dense


def gae_model(reward, done, trunc, value=None, last_value=None, terminal_value=None, gamma=0.99, lam=0.95, bootstrap_truncated=True):
    """reward float32 [K, B], done / trunc uint8 or bool [K, B], value float32 [K, B] or None, last_value float32 [B] or None,
    terminal_value dense float32 [K, B] or None -> (advantage, ret) float32 [K, B]"""
    A, R = gae_model_f64(reward, done, trunc, value, last_value, terminal_value, gamma, lam, bootstrap_truncated)
    with np.errstate(all="ignore"):
        return A.astype(np.float32), R.astype(np.float32)


def gae_model_f64(reward, done, trunc, value=None, last_value=None, terminal_value=None, gamma=0.99, lam=0.95, bootstrap_truncated=True):
    """the same before the one rounding to float32: (A, A + v) float64 [K, B]"""
    reward = np.asarray(reward, np.float32)
    K, B = reward.shape
    done, trunc = np.asarray(done).astype(bool), np.asarray(trunc).astype(bool)
    r = reward.astype(np.float64)
    v = np.zeros((K, B)) if value is None else np.asarray(value, np.float32).astype(np.float64)
    v_next = np.zeros(B) if last_value is None else np.asarray(last_value, np.float32).astype(np.float64)
    use_tv = bool(bootstrap_truncated) and terminal_value is not None
    tv = np.asarray(terminal_value, np.float32).astype(np.float64) if use_tv else None
    gamma, lam = np.float64(gamma), np.float64(lam)
    gl = gamma * lam
    adv, ret = np.empty((K, B)), np.empty((K, B))
    A = np.zeros(B)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            d = done[t]
            term = np.where(trunc[t], tv[t], 0.0) if use_tv else np.zeros(B)
            nv = np.where(d, term, v_next)
            delta = (r[t] + gamma * nv) - v[t]
            A = np.where(d, delta, delta + gl * A)
            adv[t] = A
            ret[t] = A + v[t]
            v_next = v[t]
    return adv, ret


def synthetic(K, B, seed, p_done=0.02, with_nan=False):
    """random inputs with constructed flags: about p_done of the steps done, every other one of them (in raster order)
    truncated, so both kinds are present whenever two steps are done; at least one done step is forced when K * B >= 2"""
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((K, B)).astype(np.float32)
    value = rng.standard_normal((K, B)).astype(np.float32)
    last_value = rng.standard_normal(B).astype(np.float32)
    terminal_value = rng.standard_normal((K, B)).astype(np.float32)
    done = rng.random((K, B)) < p_done
    if K * B >= 2 and done.sum() < 2:
        done.reshape(-1)[[0, K * B - 1]] = True
    trunc = np.zeros((K, B), bool)
    flat = np.flatnonzero(done.reshape(-1))
    trunc.reshape(-1)[flat[::2]] = True
    return dict(reward=reward, done=done.astype(np.uint8), trunc=trunc.astype(np.uint8), value=value, last_value=last_value,
                terminal_value=terminal_value)
