"""The contract of sg_replay_sequence_device (include/spacegym.h) in NumPy: the draw over the starts whose last
step is still a valid transition, the L + 1 observation rows and L steps of each column, the terminal join where a step is done, the
extra columns and the device-side refusals.  The ring, Philox and umul64hi are tests/replay_model.py's."""
import numpy as np

from replay_model import M32, Ring, philox4x32_10, synthetic, umul64hi  # noqa: F401  (Ring, synthetic: what the tests build rings with)

STREAM_SEQUENCE = 8


def starts(ring, L):
    """S: the number of (slot offset, env) cells a sequence of L steps may start at; 0 or less: the device refuses the call"""
    return (ring.valid - int(L) + 1) * ring.B


def draws(seed, call, n, cells):
    """u of columns 0 .. n - 1 of call number `call`: uniform on [0, cells)"""
    j = np.arange(n, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (j & M32, j >> np.uint64(32), int(call) & 0xFFFFFFFF, STREAM_SEQUENCE))
    return umul64hi(w[0], w[1], cells)


def sample_sequences(ring, n, length, seed=0, index=None, columns=(), advance=True):
    """What sg_replay_sequence_device writes: (out, ok, written).  out: obs [L + 1, n, D], action [L, n(, 2)], reward, done, trunc
    [L, n], terminal_obs [L, n, D], index [n], columns (a list of [L, n]).  ok bool [n]: columns with ok False are left untouched by
    the device (their entries here are zero) and set the status word.  written bool [L, n]: where terminal_obs is written (done, in
    a column that is ok); its other rows are zero here and untouched on the device.  A ring that holds fewer than L steps: the
    device writes nothing and sets the status word; here ring.status is set and (None, None, None) returned."""
    T, B, D, C, v, h = ring.T, ring.B, ring.D, ring.C, ring.valid, ring.head
    L = int(length)
    assert 1 <= L <= T - 1 and len(columns) <= 4
    if advance:
        call, ring.sample_calls = ring.sample_calls, (ring.sample_calls + 1) % 2 ** 32
    else:
        call = ring.sample_calls
    if v < L:
        ring.status = ring.status or n > 0
        return None, None, None
    S = (v - L + 1) * B
    u = draws(seed, call, n, S) if index is None else np.asarray(index, np.int64)
    ok = (u >= 0) & (u < S)
    uu = np.where(ok, u, 0)
    q, i = uu // B, uu % B
    first = (h - v) % T
    p = (first + q[None, :] + np.arange(L)[:, None]) % T  # [L, n]
    ii = np.broadcast_to(i, (L, n))
    obs = np.concatenate([ring.obs[(p[0] - 1) % T, i][None], ring.obs[p, ii]], 0)
    done = ring.done[p, ii]
    written = (done != 0) & ok[None, :]
    rec = np.where(written, ring.term_idx[p, ii].astype(np.int64) % C, 0)
    terminal_obs = np.where(written[..., None], ring.term_obs[rec], np.float32(0))
    out = dict(obs=obs, action=ring.action[p, ii], reward=ring.reward[p, ii], done=done, trunc=ring.trunc[p, ii],
               terminal_obs=terminal_obs.astype(np.float32), columns=[np.asarray(c, np.float32)[p, ii] for c in columns])
    for k, a in out.items():
        if k == "columns":
            for c in a:
                c[:, ~ok] = 0
        else:
            a = np.array(a)
            a[:, ~ok] = 0
            out[k] = a
    out["index"] = np.where(ok, u, 0).astype(np.int64)
    ring.status = ring.status or bool((~ok).any())
    return out, ok, written
