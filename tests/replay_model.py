"""The contract of the replay ring (include/spacegym.h, sg_replay_*) in NumPy with Python integers: Philox4x32-10,
umul64hi, the valid window, the n-step walk in float64 one operation at a time, the terminal join, the commits and their device-side
refusals.  `synthetic` fills a ring by simulating commits of random rows, wrapping more than once, and keeps an independent dense
[T, B, D] copy of every terminal row."""
import numpy as np

STREAM_REPLAY = 3
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr):
    """key (k0, k1), ctr (c0, c1, c2, c3): integers or equal-length arrays of 32-bit values -> four uint32 arrays"""
    k0, k1 = (np.atleast_1d(np.asarray(k, np.uint64)) & M32 for k in key)
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, np.uint64)) & M32 for c in ctr)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # < 2^64: exact
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(np.broadcast_arrays(c0, c1, c2, c3))


def umul64hi(lo, hi, n):
    """floor((lo | hi << 32) * n / 2^64) for 0 <= n < 2^31, exact in uint64"""
    n = int(n)
    assert 0 <= n < 2 ** 31
    lo, hi, n64 = np.asarray(lo, np.uint64), np.asarray(hi, np.uint64), np.uint64(n)
    return ((hi * n64 + ((lo * n64) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def draws(seed, call, n, cells):
    """u of draws 0 .. n - 1 of call number `call`: uniform on [0, cells)"""
    j = np.arange(n, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (j & M32, j >> np.uint64(32), int(call) & 0xFFFFFFFF, STREAM_REPLAY))
    return umul64hi(w[0], w[1], cells)


class Ring:
    """the ring's members as host arrays, the header as Python integers, `status` = the device-side refusal (code 8) seen"""

    def __init__(self, T, B, D, C, discrete=False):
        self.T, self.B, self.D, self.C, self.discrete = T, B, D, C, discrete
        self.obs = np.zeros((T, B, D), np.float32)
        self.action = np.zeros((T, B), np.int32) if discrete else np.zeros((T, B, 2), np.float32)
        self.reward = np.zeros((T, B), np.float32)
        self.done, self.trunc = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8)
        self.term_idx = np.zeros((T, B), np.uint32)
        self.term_obs = np.zeros((C, D), np.float32)
        self.slot_seq = np.zeros(T, np.uint32)
        self.head = self.filled = self.term_head = self.sample_calls = 0
        self.status = False

    def begin(self, obs0=None):
        self.head = self.filled = self.term_head = self.sample_calls = 0
        if obs0 is not None:
            self.obs[self.T - 1] = obs0

    @property
    def valid(self):
        return min(self.filled, self.T - 1)

    def __len__(self):
        return self.valid * self.B

    def write_rows(self, first, rows):
        K = rows["reward"].shape[0]
        for k in ("obs", "action", "reward", "done", "trunc"):
            getattr(self, k)[first:first + K] = rows[k]

    def _finish(self, first, K, before, after, bad):
        T = self.T
        self.slot_seq[first:first + K] = before
        self.term_head = after
        self.head, self.filled = (first + K) % T, min(self.filled + K, T)
        v = self.valid
        if v:
            oldest = (self.head - v) % T
            bad = bad or ((after - int(self.slot_seq[oldest])) % 2 ** 32) > self.C
        self.status = self.status or bad

    def commit_list(self, first, K, count, step_env, obs, capacity):
        assert first + K <= self.T
        before = self.term_head
        n = min(count, capacity)
        bad = count > capacity
        for k in range(n):
            t, i = int(step_env[k, 0]), int(step_env[k, 1])
            if not (0 <= t < K and 0 <= i < self.B):
                bad = True
                continue
            seq = (before + k) % 2 ** 32
            self.term_obs[seq % self.C] = obs[k]
            self.term_idx[first + t, i] = seq
        self._finish(first, K, before, (before + n) % 2 ** 32, bad)

    def commit_dense(self, first, tobs):
        """the order of the sequence numbers is free on the device; here: ascending env"""
        before = self.term_head
        seq = before
        for i in np.nonzero(self.done[first])[0]:
            self.term_obs[seq % self.C] = tobs[i]
            self.term_idx[first, i] = seq
            seq = (seq + 1) % 2 ** 32
        self._finish(first, 1, before, seq, False)


def sample(ring, n, seed=0, n_step=1, gamma=0.99, index=None, advance=True):
    """The batch sg_replay_sample_device writes, and `ok` bool [n]: rows with ok False are left untouched by the device (their
    entries here are zero) and set the status word."""
    T, B, D, C, v, h = ring.T, ring.B, ring.D, ring.C, ring.valid, ring.head
    cells = v * B
    assert cells > 0
    u = draws(seed, ring.sample_calls, n, cells) if index is None else np.asarray(index, np.int64)
    if advance:
        ring.sample_calls = (ring.sample_calls + 1) % 2 ** 32
    ok = (u >= 0) & (u < cells)
    uu = np.where(ok, u, 0)
    q, i = uu // B, uu % B
    first = (h - v) % T
    p0 = (first + q) % T
    R = ring.reward[p0, i].astype(np.float64)
    g = np.full(n, float(gamma), np.float64)
    gamma = np.float64(gamma)
    last = np.zeros(n, np.int64)
    open_ = np.ones(n, bool)
    for k in range(1, n_step):
        pk, pprev = (first + q + k) % T, (first + q + k - 1) % T
        open_ = open_ & (ring.done[pprev, i] == 0) & (q + k < v)
        term = g * ring.reward[pk, i].astype(np.float64)  # one rounding
        R = np.where(open_, R + term, R)                    # one rounding
        g = np.where(open_, g * gamma, g)
        last = np.where(open_, k, last)
    pl = (first + q + last) % T
    fin = ring.done[pl, i] != 0
    tr = ring.trunc[pl, i] != 0
    slot = np.where(fin, ring.term_idx[pl, i].astype(np.int64) % C, 0)
    next_obs = np.where(fin[:, None], ring.term_obs[slot], ring.obs[pl, i])
    out = dict(obs=ring.obs[(p0 - 1) % T, i], action=ring.action[p0, i], reward=R.astype(np.float32), next_obs=next_obs,
               terminated=(fin & ~tr).astype(np.uint8), truncated=tr.astype(np.uint8), discount=g.astype(np.float32),
               steps=(last + 1).astype(np.uint8), index=u.astype(np.int64))
    for k, a in out.items():
        a = np.array(a)
        a[~ok] = 0
        out[k] = a
    return out, ok


def synthetic(T, B, D, laps=2.5, K=None, p_done=0.02, p_trunc=0.5, seed=0, discrete=False, C=None, dense=False):
    """A ring filled by simulated commits of random rows (K slots per commit; K divides T; dense form: K = 1), about `laps` times
    round, with the given finish rate and truncation share.  Returns (ring, commits, term_dense): `commits` is the list of what a
    caller hands over, dicts of rows (obs, action, reward, done, trunc [K, ...]), first, and either count / step_env / tobs /
    capacity (list form, records shuffled, buffers larger than the count) or terminal_obs [B, D] (dense form); obs0 [B, D] is the
    row before the first step; term_dense [T, B, D] holds the terminal observation of every finished (slot, env) of the final
    ring, kept independently of term_idx / term_obs."""
    rng = np.random.default_rng(seed)
    K = 1 if dense else (K or max(1, T // 4))
    assert T % K == 0
    C = C or max(2 * B, T * B // 16)
    ring = Ring(T, B, D, C, discrete)
    obs0 = rng.standard_normal((B, D)).astype(np.float32)
    ring.begin(obs0)
    term_dense = np.full((T, B, D), np.nan, np.float32)
    commits = []
    for c in range(int(round(laps * T / K))):
        first = ring.head
        done = rng.random((K, B)) < p_done
        trunc = done & (rng.random((K, B)) < p_trunc)
        reward = rng.standard_normal((K, B)).astype(np.float32)
        reward[rng.random((K, B)) < 0.01] = np.float32(-0.0)
        rows = dict(obs=rng.standard_normal((K, B, D)).astype(np.float32),
                    action=rng.integers(0, 6, (K, B)).astype(np.int32) if discrete else rng.uniform(-1, 1, (K, B, 2)).astype(np.float32),
                    reward=reward, done=done.astype(np.uint8), trunc=trunc.astype(np.uint8))
        ring.write_rows(first, rows)
        t, i = np.nonzero(done)
        rec = rng.standard_normal((t.size, D)).astype(np.float32)
        term_dense[first + t, i] = rec
        com = dict(first=first, K=K, rows=rows)
        if dense:
            tobs = np.full((B, D), np.nan, np.float32)  # rows of envs that did not finish are never read
            tobs[i] = rec
            com["terminal_obs"] = tobs
            ring.commit_dense(first, tobs)
        else:
            order = rng.permutation(t.size)
            cap = t.size + 7
            step_env = np.full((cap, 2), -7, np.int32)
            step_env[:t.size, 0], step_env[:t.size, 1] = t[order], i[order]
            lobs = np.full((cap, D), np.nan, np.float32)
            lobs[:t.size] = rec[order]
            com.update(count=int(t.size), step_env=step_env, tobs=lobs, capacity=cap)
            ring.commit_list(first, K, int(t.size), step_env, lobs, cap)
        commits.append(com)
    return ring, commits, dict(obs0=obs0, term_dense=term_dense)
