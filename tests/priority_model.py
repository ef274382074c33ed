"""The contract of prioritized replay sampling (include/spacegym.h, sg_priority_*) in NumPy.  The state is integers
only: q uint32 [T B] (0 = not samplable), total and every prefix sum uint64, head / filled / max_q / sample_calls Python integers.
The draw knows no tree: the cell chosen for r in [0, total) is np.searchsorted(np.cumsum(q, dtype=uint64), r, side="right"), i.e.
the smallest cell c with q[0] + ... + q[c] > r."""
import numpy as np

from replay_model import M32, philox4x32_10

STREAM_PRIORITY = 4


def quantise(p, frac_bits):
    """q = clamp(rint((double) p 2^frac_bits), 1, 2^32 - 1) of float32 priorities, and which of them are accepted at all (not NaN,
    negative or infinite)"""
    p = np.asarray(p, np.float32)
    ok = np.isfinite(p) & (p >= 0)
    x = np.rint(np.where(ok, p, 0).astype(np.float64) * float(2 ** frac_bits))  # (a power of two: exact)
    return np.clip(x, 1.0, float(2 ** 32 - 1)).astype(np.uint64).astype(np.uint32), ok


def umul64hi_64(x, n):
    """floor(x n / 2^64) for uint64 arrays x and a non-negative integer n < 2^64, through 32-bit limbs (exact in uint64)"""
    x = np.asarray(x, np.uint64)
    n = int(n)
    assert 0 <= n < 2 ** 64
    s32 = np.uint64(32)
    x0, x1 = x & M32, x >> s32
    n0, n1 = np.uint64(n & 0xFFFFFFFF), np.uint64(n >> 32)
    p00, p01, p10, p11 = x0 * n0, x0 * n1, x1 * n0, x1 * n1
    mid = (p00 >> s32) + (p01 & M32) + (p10 & M32)
    return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)


def numbers(total, call, n, seed, stratified):
    """r of draws 0 .. n - 1 of call number `call` over `total` units, exact in uint64"""
    j = np.arange(n, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (j & M32, j >> np.uint64(32), int(call) & 0xFFFFFFFF, STREAM_PRIORITY))
    x = w[0] | (w[1] << np.uint64(32))
    if not stratified or n == 0:
        return umul64hi_64(x, total)
    each, rest = divmod(int(total), n)
    r = j * np.uint64(each) + np.minimum(j, np.uint64(rest))
    short = j >= np.uint64(rest)
    r[short] += umul64hi_64(x[short], each)
    r[~short] += umul64hi_64(x[~short], each + 1)
    return r


class Priorities:
    """q as a host array, the header as Python integers, `status` = a device-side refusal (code 9) seen"""

    def __init__(self, T, B, frac_bits=16):
        self.T, self.B, self.frac_bits = T, B, frac_bits
        self.q = np.zeros(T * B, np.uint32)
        self.begin()

    def begin(self):
        self.q[:] = 0
        self.head = self.filled = self.sample_calls = 0
        self.max_q = 1 << self.frac_bits
        self.status = False

    @property
    def total(self):
        return int(self.q.sum(dtype=np.uint64))

    @property
    def valid(self):
        return min(self.filled, self.T - 1)

    def slot_valid(self, p):
        return ((self.head - 1 - np.asarray(p)) % self.T) < self.valid

    def commit(self, first, filled_before, K):
        T, B = self.T, self.B
        assert K >= 1 and 0 <= first and first + K <= T and 0 <= filled_before <= T
        self.q[first * B:(first + K) * B] = self.max_q
        hole = (first + K) % T
        self.q[hole * B:(hole + 1) * B] = 0
        self.head, self.filled = hole, min(filled_before + K, T)

    def update(self, cell, priority):
        """returns the mask of the rows applied"""
        cell = np.asarray(cell, np.int64)
        q, ok = quantise(priority, self.frac_bits)
        ok &= (cell >= 0) & (cell < self.T * self.B)
        if not ok.all():
            self.status = True
        c = np.where(ok, cell, 0)
        on = ok & self.slot_valid(c // self.B)
        if on.any():
            new = np.zeros_like(self.q)
            np.maximum.at(new, c[on], q[on])  # duplicates: the largest wins
            named = np.zeros(self.q.size, bool)
            named[c[on]] = True
            self.q[named] = new[named]
            self.max_q = max(self.max_q, int(q[on].max()))
        return on

    def numbers(self, n, seed, stratified):
        return numbers(self.total, self.sample_calls, n, seed, stratified)

    def sample(self, n, seed=0, beta=0.4, stratified=True, ring_head=None, ring_filled=None, advance=True):
        """dict(index, cell, weight, leaf), or None where the device refuses the whole call (status 9, nothing written)"""
        total = self.total
        lag = (ring_head is not None and ring_head != self.head) or (ring_filled is not None and ring_filled != self.filled)
        if n > 0 and (total == 0 or (stratified and total < n) or lag):
            self.status = True
            if advance:
                self.sample_calls = (self.sample_calls + 1) % 2 ** 32
            return None
        r = self.numbers(n, seed, stratified)
        if advance:
            self.sample_calls = (self.sample_calls + 1) % 2 ** 32
        assert n == 0 or int(r.max()) < total
        cell = np.searchsorted(np.cumsum(self.q, dtype=np.uint64), r, side="right").astype(np.int64)
        q = self.q[cell]
        p, i = cell // self.B, cell % self.B
        v = self.valid
        assert self.slot_valid(p).all() and (q > 0).all()
        index = ((p - (self.head - v)) % self.T) * self.B + i
        share = (np.float64(v * self.B) * q.astype(np.float64)) / np.float64(total)  # each operation rounded on its own
        weight64 = np.power(share, -np.float64(beta))
        return dict(index=index.astype(np.int64), cell=cell, weight=weight64.astype(np.float32), leaf=q, weight64=weight64)
