"""The contract of the minibatch index call (include/spacegym.h, sg_minibatch_index_device) in NumPy with Python
integers: a keyed bijection pi of [0, N) per (seed, step + step_dev, epoch, member) -- an 8-round unbalanced Feistel network over
max(2, bit_length(N - 1)) bits with cycle walking -- and the two maps from pi to rows of a flattened [K, B] rollout.  The kernel
follows it bit for bit.

What is NOT claimed: uniformity over all N! orders.  The network is a small family of bijections (8 round keys), and at tiny N it
is visibly non-uniform over the orders: a 3-bit Feistel over the 120 orders of N = 5 cannot reach most of them equally.  The claim is
uniformity of single positions and of pairs at the sizes anyone trains with; tests/test_minibatch.py states the conditions."""
import numpy as np

from replay_model import philox4x32_10

STREAM_MINIBATCH = 11
ROUNDS = 8
ROW, ENV = 0, 1
MAX_MEMBERS, MAX_EPOCHS = 256, 64
WALK_CAP = 64  # no element of the tested sizes needs more than 20 encryptions; a broken round function must not look like a slow one
M32 = 0xFFFFFFFF


def fmix32(x):
    """murmur3's finaliser on Python integers or uint64 arrays of 32-bit values"""
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def _step_words(step, step_dev=0):
    step = (int(step) + int(step_dev)) & 0xFFFFFFFFFFFFFFFF  # a 64-bit wrapping sum
    return step & M32, step >> 32


def round_keys(seed=0, step=0, member=0, epoch=0, step_dev=0):
    """the eight round keys of (member, epoch): two Philox blocks, k[4 blk + i] = o_i.  step an integer: a list of eight integers;
    step, member or epoch sequences of S integers (or some of them, the others integers): uint64 [8, S], one column per entry"""
    seed, member, epoch = int(seed), np.asarray(member, np.int64), np.asarray(epoch, np.int64)
    assert ((0 <= member) & (member < MAX_MEMBERS)).all() and ((0 <= epoch) & (epoch < MAX_EPOCHS)).all()
    many = np.ndim(step) == 1 or member.ndim == 1 or epoch.ndim == 1
    words = [_step_words(s, step_dev) for s in (step if np.ndim(step) == 1 else [step])]
    lo, hi = [w[0] for w in words], [w[1] for w in words]
    k = []
    for blk in range(2):
        k += philox4x32_10((seed & M32, (seed >> 32) & M32), ((epoch << 16) | (blk << 8) | member, lo, hi, STREAM_MINIBATCH))
    return np.stack(k) if many else [int(w[0]) for w in k]


def widths(N):
    """(bits, wa, wb): the domain 2^bits >= max(N, 4), split into a left part of wa bits and a right part of wb bits"""
    bits = max(2, (int(N) - 1).bit_length())
    return bits, bits // 2, bits - bits // 2


def encrypt(x, k, N):
    """one encryption of x in [0, 2^bits): x an integer or an integer array; k[r] integers, or arrays that broadcast against x"""
    _, a, b = widths(N)
    x = np.asarray(x, np.uint64)
    L, R = x >> np.uint64(b), x & np.uint64((1 << b) - 1)
    for r in range(ROUNDS):
        t = fmix32((R + np.asarray(k[r], np.uint64)) & np.uint64(M32)) >> np.uint64(32 - a)
        L, R = R, L ^ t
        a, b = b, a
    return (L << np.uint64(b)) | R


def permutation(N, k, positions=None, count=False):
    """pi at `positions` (None: all of 0 .. N - 1) as int64; k a list of eight integers -> [len(positions)], k uint64 [8, S] ->
    [S, len(positions)].  count: also the encryptions every element needed"""
    N = int(N)
    assert N >= 1
    x = np.arange(N) if positions is None else np.asarray(positions)
    assert x.ndim == 1 and ((0 <= x) & (x < N)).all()
    k = np.asarray(k, np.uint64)
    if k.ndim == 2:
        k, x = k[:, :, None], np.broadcast_to(x, (k.shape[1], len(x)))
    y = encrypt(x, k, N)
    n = np.ones(y.shape, np.int64)
    while True:
        out = y >= np.uint64(N)
        if not out.any():
            break
        assert n.max() < WALK_CAP, "cycle walking passed the cap: the round function is broken"
        y = np.where(out, encrypt(y, k, N), y)
        n += out
    y = y.astype(np.int64)
    return (y, n) if count else y


def pi(N, seed=0, step=0, member=0, epoch=0, step_dev=0):
    return permutation(N, round_keys(seed, step, member, epoch, step_dev))


def size(K, B, P, M, unit):
    """n of the [epochs, M, P, n] index, or -1 for a refused shape"""
    K, B, P, M = int(K), int(B), int(P), int(M)
    if not (1 <= P <= MAX_MEMBERS and B % P == 0 and M >= 1 and K >= 1 and K * B < 2 ** 31 and unit in (ROW, ENV)):
        return -1
    E = B // P
    n = (K * E) // M if unit == ROW else K * (E // M)
    return n if n >= 1 else -1


def index(K, B, P, epochs, M, unit, seed=0, step=0, step_dev=0):
    """int64 [epochs, M, P, n]"""
    n = size(K, B, P, M, unit)
    assert n >= 1 and 1 <= epochs <= MAX_EPOCHS
    E = B // P
    e, m = (g.ravel() for g in np.meshgrid(np.arange(epochs), np.arange(P), indexing="ij"))
    keys = round_keys(seed, step, m, e, step_dev)  # [8, epochs P]
    first = (np.arange(P) * E).reshape(1, 1, P, 1)
    if unit == ROW:
        j = permutation(K * E, keys, positions=np.arange(M * n)).reshape(epochs, P, M, n).transpose(0, 2, 1, 3)
        return (j // E) * B + first + j % E
    c = E // M
    col = permutation(E, keys, positions=np.arange(M * c)).reshape(epochs, P, M, 1, c).transpose(0, 2, 1, 3, 4)
    return ((np.arange(K) * B).reshape(1, 1, 1, K, 1) + first[..., None] + col).reshape(epochs, M, P, n)
