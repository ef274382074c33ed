"""CPU tests of the minibatch index call and the one-call PPO update (sg_minibatch_size / sg_minibatch_index_device,
minibatch_index_torch / ppo_update_torch): the NumPy statement (tests/minibatch_model.py) against its known answers,
the bijection, the keys, the two units, the statistics the shuffle must stay within, the declarations and sources, the Python argument
checks with the native calls stubbed, and the resources of the new kernel."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import engine_asm
import minibatch_model as mm
from test_adam import _grads, _handles, _opt
from test_episode_stats import _fake_cuda, _stub_env
from test_snapshot_device import _header_args

METHODS = ("minibatch_index_torch", "ppo_update_torch")


# ---------------------------------------------------------------------------------------------------------------- the model: known answers
def test_known_answers():
    k = mm.round_keys(seed=0x123456789, step=5)
    assert ["%08x" % x for x in k] == ["0d56ca9e", "6b54284f", "ec78c2e9", "b5ea8ec3", "be64c71a", "209bbb51", "4b8eb8e0", "8c5afe0a"]
    assert mm.permutation(10, k).tolist() == [4, 5, 9, 2, 1, 6, 0, 7, 3, 8]
    assert mm.pi(10, seed=0x123456789, step=2 ** 32 + 5, member=3, epoch=2).tolist() == [5, 2, 3, 7, 1, 8, 4, 0, 9, 6]
    assert mm.pi(1).tolist() == [0] and mm.pi(1, seed=9, step=4, member=2, epoch=1).tolist() == [0]
    assert mm.pi(2, seed=1, step=0).tolist() == [0, 1]
    assert mm.STREAM_MINIBATCH == 11 and mm.ROUNDS == 8
    assert mm.fmix32(0) == 0 and mm.fmix32(1) == 0x514E28B7  # murmur3's finaliser


def test_the_widths_and_one_encryption_by_hand():
    assert [mm.widths(N) for N in (1, 2, 3, 4, 5, 9, 10, 4097, 2 ** 31 - 1)] == [
        (2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1), (3, 1, 2), (4, 2, 2), (4, 2, 2), (13, 6, 7), (31, 15, 16)]
    k = mm.round_keys(seed=3, step=1)
    for N in (5, 10, 4097):  # the rounds written out with Python integers
        bits, wa, wb = mm.widths(N)
        for x in (0, 1, 2 ** bits - 1, 2 ** bits // 3):
            L, R, a, b = x >> wb, x & (2 ** wb - 1), wa, wb
            for r in range(8):
                t = mm.fmix32((R + k[r]) % 2 ** 32) >> (32 - a)
                L, R = R, L ^ t
                a, b = b, a
            assert int(mm.encrypt(x, k, N)) == (L << b) | R
        every = mm.encrypt(np.arange(2 ** bits), k, N)
        assert sorted(every.tolist()) == list(range(2 ** bits))  # a bijection of [0, 2^bits)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 257, 1000, 4097, 65537])
def test_pi_is_a_bijection(N):
    for seed, step, m, e in ((0, 0, 0, 0), (7, 3, 255, 63), (2 ** 63 + 5, 2 ** 64 - 1, 17, 9)):
        p = mm.pi(N, seed, step, m, e)
        assert p.dtype == np.int64 and p.shape == (N,) and np.array_equal(np.sort(p), np.arange(N)), (N, seed, step, m, e)


def test_every_part_of_the_key_changes_the_permutation():
    N, base = 1000, dict(seed=3, step=5, member=1, epoch=2)
    a = mm.pi(N, **base)
    for change in (dict(member=2), dict(epoch=3), dict(seed=4), dict(seed=3 + 2 ** 32), dict(step=6), dict(step=5 + 2 ** 32), dict(member=0, epoch=0)):
        assert not np.array_equal(a, mm.pi(N, **dict(base, **change))), change
    assert np.array_equal(a, mm.pi(N, **dict(base, step=2, step_dev=3)))
    assert np.array_equal(a, mm.pi(N, **dict(base, step=2 ** 64 - 1, step_dev=6)))  # a 64-bit wrapping sum
    carry = mm.pi(N, **dict(base, step=2 ** 32 - 1, step_dev=1))                     # a carry into the high word
    assert np.array_equal(carry, mm.pi(N, **dict(base, step=2 ** 32))) and not np.array_equal(carry, mm.pi(N, **dict(base, step=0)))
    assert not np.array_equal(carry, mm.pi(N, **dict(base, step=2 ** 32 - 1)))
    # the batched keys are the single ones
    ks = mm.round_keys(3, [5, 6, 2 ** 32 + 5], 1, 2)
    assert ks.shape == (8, 3) and [int(x) for x in ks[:, 2]] == mm.round_keys(3, 2 ** 32 + 5, 1, 2)
    assert np.array_equal(mm.permutation(N, ks)[0], a) and np.array_equal(mm.permutation(N, ks, positions=[7, 0])[1], mm.pi(N, 3, 6, 1, 2)[[7, 0]])


# ---------------------------------------------------------------------------------------------------------------- from pi to rows
SHAPES = [(1, 1, 1, 1, 1), (3, 5, 1, 2, 2), (4, 192, 3, 4, 2), (7, 1040, 2, 3, 3), (17, 241, 1, 5, 1), (1, 256, 256, 1, 64)]  # (K, B, P, M, epochs)


@pytest.mark.parametrize("K,B,P,M,epochs", SHAPES)
@pytest.mark.parametrize("unit", [mm.ROW, mm.ENV])
def test_both_units_shapes_blocks_distinct_entries_and_left_overs(K, B, P, M, epochs, unit):
    E = B // P
    n = mm.size(K, B, P, M, unit)
    assert n == ((K * E) // M if unit == mm.ROW else K * (E // M))
    if n < 1:
        assert n == -1
        return
    idx = mm.index(K, B, P, epochs, M, unit, seed=11, step=2 ** 33 + 1)
    assert idx.shape == (epochs, M, P, n) and idx.dtype == np.int64
    t, i = idx // B, idx % B
    assert ((0 <= idx) & (idx < K * B)).all()
    assert (i // E == np.arange(P).reshape(1, 1, P, 1)).all()  # every entry lies in its member's env block
    left = []
    for e in range(epochs):
        for m in range(P):
            rows = idx[e, :, m].ravel()
            assert len(set(rows.tolist())) == M * n  # distinct within one (epoch, member)
            block = {tt * B + m * E + c for tt in range(K) for c in range(E)}
            left.append(frozenset(block - set(rows.tolist())))
    assert all(len(l) == (K * E - M * n) for l in left)
    if unit == mm.ROW:
        assert K * E - M * n < M
    else:  # [K, c] column views: row t of a block is row 0 plus t B, and its c columns are distinct envs
        c = E // M
        v = idx.reshape(epochs, M, P, K, c)
        assert (v == v[..., :1, :] + (np.arange(K) * B).reshape(K, 1)).all()
        assert K * E - M * n == K * (E - M * c) and E - M * c < M
        for e in {0, epochs - 1}:
            for m in {0, P // 2, P - 1}:
                assert np.array_equal(v[e, :, m, 0].ravel() - m * E, mm.pi(E, 11, 2 ** 33 + 1, m, e)[:M * c])
    if unit == mm.ROW and epochs > 1 and K * E - M * n > 0 and K * E > 4:
        assert len(set(left[m::P][k] for k in range(epochs) for m in [0])) > 1  # the left-over rows are another set per epoch


def test_the_row_map_written_out():
    K, B, P, M, E = 3, 12, 2, 2, 6
    idx = mm.index(K, B, P, 2, M, mm.ROW, seed=1, step=2)
    n = (K * E) // M
    for e in range(2):
        for m in range(P):
            p = mm.pi(K * E, 1, 2, m, e)
            for b in range(M):
                for i in range(n):
                    j = int(p[b * n + i])
                    assert idx[e, b, m, i] == (j // E) * B + m * E + j % E


def test_size_refuses_what_the_header_lists():
    assert mm.size(4, 12, 5, 1, mm.ROW) == -1 and mm.size(4, 12, 0, 1, mm.ROW) == -1 and mm.size(4, 512, 512, 1, mm.ROW) == -1
    assert mm.size(4, 12, 3, 0, mm.ROW) == -1 and mm.size(4, 12, 3, 17, mm.ROW) == -1 and mm.size(4, 12, 3, 16, mm.ROW) == 1
    assert mm.size(4, 12, 3, 5, mm.ENV) == -1 and mm.size(4, 12, 3, 4, mm.ENV) == 4 and mm.size(4, 12, 3, 1, 2) == -1
    assert mm.size(2 ** 15, 2 ** 16, 1, 1, mm.ROW) == -1 and mm.size(2 ** 15 - 1, 2 ** 16, 1, 1, mm.ROW) == (2 ** 15 - 1) * 2 ** 16
    assert mm.size(0, 12, 3, 1, mm.ROW) == -1


# ---------------------------------------------------------------------------------------------------------------- statistics
def test_every_position_is_uniform_over_the_100_rows():
    """N = 100, seed 7, steps 0 .. 9 999: for every position j the chi-square of pi(j) over 100 bins (99 degrees of freedom, standard
    deviation sqrt(198)) is at most 99 + 5 sqrt(198) = 169.4"""
    S, N = 10000, 100
    p = mm.permutation(N, mm.round_keys(7, range(S)))
    chi = [float(((np.bincount(p[:, j], minlength=N) - S / N) ** 2 / (S / N)).sum()) for j in range(N)]
    print("worst position: chi-square %.1f" % max(chi))
    assert max(chi) <= 99 + 5 * math.sqrt(198), max(chi)


def test_the_pair_of_the_first_two_positions_is_uniform_over_the_ordered_pairs():
    """N = 33, seed 5, 52 800 steps: the chi-square of (pi(0), pi(1)) over the 1 056 ordered pairs of distinct rows (50 expected in
    each) is within 4 standard deviations sqrt(2 x 1 055) of its 1 055 degrees of freedom"""
    S, N = 52800, 33
    p = mm.permutation(N, mm.round_keys(5, range(S)), positions=[0, 1])
    assert (p[:, 0] != p[:, 1]).all()
    counts = np.bincount(p[:, 0] * N + p[:, 1], minlength=N * N).reshape(N, N)
    off = counts[~np.eye(N, dtype=bool)]
    assert off.size == 1056 and off.sum() == S
    chi = float(((off - S / 1056) ** 2 / (S / 1056)).sum())
    z = (chi - 1055) / math.sqrt(2 * 1055)
    print("pairs: chi-square %.1f, %+.2f standard deviations" % (chi, z))
    assert abs(z) <= 4.0, z


def test_two_rows_share_a_minibatch_as_often_as_a_uniform_shuffle_makes_them():
    """N = 1 024, M = 4, seed 3, 4 000 steps: rows 0 and 1 are in the same minibatch with probability 255 / 1 023; the share over the
    steps is within 4 standard deviations sqrt(p (1 - p) / 4 000) = 0.0068 each, 0.0274 in all"""
    S, N, M = 4000, 1024, 4
    p = mm.permutation(N, mm.round_keys(3, range(S)))
    where = np.empty_like(p)
    np.put_along_axis(where, p, np.broadcast_to(np.arange(N), p.shape), axis=1)  # where[s, row] = its position
    share = float((where[:, 0] // (N // M) == where[:, 1] // (N // M)).mean())
    prob = 255 / 1023
    print("share %.4f of %.4f" % (share, prob))
    assert abs(share - prob) <= 4.0 * math.sqrt(prob * (1 - prob) / S), share


def test_cycle_walking_stays_far_below_the_cap():
    """over 300 keys at N = 65 and 4 097 (just past a power of two: the longest walks) no element needs 64 encryptions; the model
    asserts the cap, which keeps a broken round function from looking like a slow one"""
    assert mm.WALK_CAP == 64
    for N in (65, 4097):
        worst, total = 0, 0
        for s in range(300):
            p, n = mm.permutation(N, mm.round_keys(s, 7 * s), count=True)
            worst, total = max(worst, int(n.max())), total + int(n.sum())
        print("N = %d: at most %d encryptions, %.3f on average" % (N, worst, total / (300 * N)))
        assert worst < mm.WALK_CAP and total / (300 * N) < 2.0
    broken = [0] * 8  # not broken as a bijection, but a walk of a fixed point outside [0, N) would trip the cap: the assert is live
    with pytest.raises(AssertionError, match="cap"):
        real = mm.encrypt
        try:
            mm.encrypt = lambda x, k, N: np.full_like(np.asarray(x, np.uint64), np.uint64(N))  # never returns below N
            mm.permutation(5, broken)
        finally:
            mm.encrypt = real


# ---------------------------------------------------------------------------------------------------------------- declarations and sources
def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    assert _header_args("sg_minibatch_size", "int64_t") == ["sg_env *env", "int32_t steps", "int32_t members", "int32_t minibatches", "int32_t unit"]
    assert _header_args("sg_minibatch_index_device") == [
        "sg_env *env", "int32_t steps", "int32_t members", "int32_t epochs", "int32_t minibatches", "int32_t unit", "uint64_t seed",
        "uint64_t step", "const int64_t *step_dev", "int64_t *index_out", "void *hip_stream"]
    vp, i32, u64 = C.c_void_p, C.c_int32, C.c_uint64
    assert _native.SYMBOLS["sg_minibatch_size"] == (C.c_int64, [vp, i32, i32, i32, i32])
    assert _native.SYMBOLS["sg_minibatch_index_device"] == (C.c_int, [vp, i32, i32, i32, i32, i32, u64, u64, vp, vp, vp])
    header = open(os.path.join(build.ROOT, "include", "spacegym.h")).read()
    for name, value in (("SG_MINIBATCH_ROW", mm.ROW), ("SG_MINIBATCH_ENV", mm.ENV)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert SpaceGymVectorEnv.minibatch_units == dict(row=mm.ROW, env=mm.ENV)
    assert (SpaceGymVectorEnv.minibatch_max_members, SpaceGymVectorEnv.minibatch_max_epochs) == (mm.MAX_MEMBERS, mm.MAX_EPOCHS) == (256, 64)


def test_the_kernel_lives_in_sg_minibatch_inc_after_sg_pbt_inc_and_is_plain():
    from space_gym_amd import build
    assert build.HEADERS.index("sg_minibatch.inc") == build.HEADERS.index("sg_pbt.inc") + 1
    engine = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert engine.count('#include "sg_minibatch.inc"') == 1
    assert engine.index('#include "sg_pbt.inc"') < engine.index('#include "sg_minibatch.inc"') < engine.index("struct sg_env {")
    inc = open(os.path.join(build.CSRC, "sg_minibatch.inc")).read()
    assert re.findall(r"void (\w+_kernel)\(", inc) == ["minibatch_index_kernel"]
    code = re.sub(r"//.*", "", inc)
    assert "atomic" not in code.lower() and "template" not in code
    assert code.count("__shared__") == 1 and "__shared__ uint32_t keys[kMinibatchRounds];" in code  # the round keys, nothing else
    assert re.search(r"kStreamMinibatch = kStreamSequence \+ 3u;", code)
    assert re.search(r"static_assert\(kStreamMinibatch == %du," % mm.STREAM_MINIBATCH, code)
    assert len(re.findall(r"kStreamMinibatch, o\)", code)) == 1
    assert re.search(r"kMinibatchRounds = %d\b" % mm.ROUNDS, code) and re.search(r"kMinibatchWalkCap = %d\b" % mm.WALK_CAP, code)
    assert re.search(r"kMinibatchMaxMembers = %d\b" % mm.MAX_MEMBERS, code) and re.search(r"kMinibatchMaxEpochs = %d\b" % mm.MAX_EPOCHS, code)
    assert "0x85EBCA6Bu" in code and "0xC2B2AE35u" in code
    assert not re.search(r"[^/]/ |%", re.sub(r"/\*.*?\*/", "", code.split("minibatch_index_kernel(")[1]).replace("bits / 2", ""))  # no divide per lane


def test_the_methods_are_net_methods_and_the_multi_device_front_ends_refuse_them():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    assert set(METHODS) <= set(NET_METHODS) and all(callable(getattr(SpaceGymVectorEnv, n)) for n in METHODS)
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in METHODS:
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
    assert "ADDS NO NATIVE CODE" in SpaceGymVectorEnv.ppo_update_torch.__doc__


# ---------------------------------------------------------------------------------------------------------------- Python checks, native calls stubbed
B = 12


def _out(*shape):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=torch.int64))


@pytest.mark.parametrize("kw,match", [
    (dict(steps=0), "steps"), (dict(steps=-3), "steps"), (dict(steps=2.0), "steps"), (dict(steps=True), "steps"),
    (dict(members=0), "members"), (dict(members=257), "members"), (dict(members=5), "members"), (dict(members=8), "members"),
    (dict(epochs=0), "epochs"), (dict(epochs=65), "epochs"), (dict(minibatches=0), "minibatches"), (dict(minibatches=-1), "minibatches"),
    (dict(members=3, minibatches=17), "minibatches"), (dict(members=3, minibatches=5, unit="env"), "minibatches"),
    (dict(unit="column"), "unit"), (dict(unit=2), "unit"), (dict(unit=None), "unit"), (dict(unit=1.0), "unit"),
    (dict(steps=2 ** 31 // B + 1), "steps"),
    (dict(step_dev="int32"), "step_dev"), (dict(step_dev="two"), "step_dev"),
    (dict(out="dtype"), "out"), (dict(out="shape"), "out"), (dict(out="host"), "out"), (dict(members=3, out="flat"), "out"),
])
def test_minibatch_index_torch_refuses_before_any_native_call(kw, match):
    import torch
    env = _stub_env(B=B)
    kw = dict(dict(steps=4, out=_out(1, 1, 48)), **kw)
    special = {"int32": _fake_cuda(torch.zeros(1, dtype=torch.int32)), "two": _fake_cuda(torch.zeros(2, dtype=torch.int64)),
               "dtype": _fake_cuda(torch.zeros((1, 1, 48), dtype=torch.int32)), "shape": _out(1, 1, 47), "host": torch.zeros((1, 1, 48), dtype=torch.int64),
               "flat": _out(1, 1, 48)}
    for k in ("step_dev", "out"):
        if isinstance(kw.get(k), str):
            kw[k] = special[kw[k]]
    with pytest.raises(ValueError, match=match):
        env.minibatch_index_torch(**kw)
    assert not env._lib.calls


def test_minibatch_index_torch_reaches_the_native_call():
    import torch
    env = _stub_env(B=B)
    step_dev = _fake_cuda(torch.zeros(1, dtype=torch.int64))
    out = _out(3, 2, 3, 8)  # K = 4, P = 3: E = 4, N = 16, n = 8
    assert env.minibatch_index_torch(4, members=3, epochs=3, minibatches=2, unit="row", seed=2 ** 40 + 1, step=2 ** 63, step_dev=step_dev, out=out) is out
    name, a = env._lib.calls[-1]
    assert name == "sg_minibatch_index_device" and a[1:8] == (4, 3, 3, 2, mm.ROW, 2 ** 40 + 1, 2 ** 63)
    assert a[8].value == step_dev.data_ptr() and a[9].value == out.data_ptr()
    one = _out(1, 2, 4 * 6)  # members None: [epochs, M, n], P = 1 passed on; unit "env": c = 6, n = K c
    assert env.minibatch_index_torch(4, minibatches=2, unit="env", out=one) is one
    a = env._lib.calls[-1][1]
    assert a[1:8] == (4, 1, 1, 2, mm.ENV, 0, 0) and a[8] is None
    assert env.minibatch_index_torch(4, minibatches=2, unit=mm.ENV, out=one) is one and env._lib.calls[-1][1][5] == mm.ENV
    with pytest.raises(ValueError, match="out"):
        env.minibatch_index_torch(4, members=1, minibatches=2, unit="env", out=one)  # members = 1 is a population of one: [1, 2, 1, 24]
    assert len(env._lib.calls) == 3
    for K, P, M, unit in ((4, 3, 2, mm.ROW), (4, 3, 4, mm.ENV), (5, 1, 7, mm.ROW), (5, 12, 1, mm.ENV), (3, 2, 4, mm.ENV)):
        n = mm.size(K, B, P, M, unit)
        env.minibatch_index_torch(K, members=P, minibatches=M, unit=unit, out=_out(1, M, P, n))
        with pytest.raises(ValueError, match="out"):
            env.minibatch_index_torch(K, members=P, minibatches=M, unit=unit, out=_out(1, M, P, n + 1))


class _Recorder:
    def __init__(self, env):
        self.calls = []
        env.ppo_grad_torch = lambda *a, **kw: self._grad("ppo_grad_torch", a, kw)
        env.population_ppo_grad_torch = lambda *a, **kw: self._grad("population_ppo_grad_torch", a, kw)
        env.adam_step_torch = lambda opt, grads: self.calls.append(("adam_step_torch", (opt, grads), {}))

    def _grad(self, name, a, kw):
        self.calls.append((name, a, kw))
        return (kw["out"] if kw["out"] is not None else self.made), kw["stats"]


def _batch(rows, D=13):
    import torch
    z = lambda *s: _fake_cuda(torch.zeros(s))
    return dict(obs=z(rows, D), action=z(rows, 2), logp=z(rows), advantage=z(rows), ret=z(rows), value=z(rows))


@pytest.mark.parametrize("population", [False, True])
def test_ppo_update_torch_is_the_loop_of_the_existing_calls(population):
    import torch
    env = _stub_env(B=B)
    rec = _Recorder(env)
    one, pop = _handles(3)
    handle = pop if population else one
    opt, K, epochs, M = _opt(handle), 4, 2, 2
    P = 3 if population else 1
    n = mm.size(K, B, P, M, mm.ROW)
    lead = (epochs, M, P) if population else (epochs, M)
    index, stats = _out(*lead, n), _fake_cuda(torch.zeros((*lead, 12)))
    batch, grads = _batch(K * B), _grads(handle)
    coef = _fake_cuda(torch.zeros((3, 4))) if population else None
    step_dev = _fake_cuda(torch.zeros(1, dtype=torch.int64))
    got = env.ppo_update_torch(handle, opt, batch, K, epochs, M, seed=5, step=9, step_dev=step_dev, coef=coef, clip_range=0.1, clip_range_vf=0.3,
                               ent_coef=0.01, vf_coef=0.25, normalize_advantage=False, index=index, stats=stats, grads=grads)
    assert got[0] is stats and got[1] is index
    assert env._lib.names() == ["sg_minibatch_index_device"]  # one index call; everything else went through the recorded methods
    a = env._lib.calls[0][1]
    assert a[1:8] == (K, P, epochs, M, mm.ROW, 5, 9) and a[8].value == step_dev.data_ptr() and a[9].value == index.data_ptr()
    assert [c[0] for c in rec.calls] == ["population_ppo_grad_torch" if population else "ppo_grad_torch", "adam_step_torch"] * (epochs * M)
    for k, (e, b) in enumerate((e, b) for e in range(epochs) for b in range(M)):
        name, args, kw = rec.calls[2 * k]
        assert args[0] is handle and args[1] is batch and args[2].data_ptr() == index[e, b].data_ptr() and args[2].shape == index[e, b].shape
        assert kw["out"] is grads and kw["stats"].data_ptr() == stats[e, b].data_ptr() and kw["stats"].shape == stats[e, b].shape
        assert (kw["clip_range"], kw["clip_range_vf"], kw["ent_coef"], kw["vf_coef"], kw["normalize_advantage"]) == (0.1, 0.3, 0.01, 0.25, False)
        assert (kw.get("coef") is coef) if population else ("coef" not in kw)
        assert rec.calls[2 * k + 1][1] == (opt, grads)
    # grads None: what the first gradient call made is handed to every later one
    rec.calls.clear()
    rec.made = _grads(handle)
    env.ppo_update_torch(handle, opt, batch, K, epochs, M, coef=coef, index=index, stats=stats)
    assert rec.calls[0][2]["out"] is None and all(c[2]["out"] is rec.made for c in rec.calls[2::2]) and all(c[1][1] is rec.made for c in rec.calls[1::2])


def test_ppo_update_torch_refusals():
    import torch
    env = _stub_env(B=B)
    rec = _Recorder(env)
    one, pop = _handles(3)
    opt1, optp, K = _opt(one), _opt(pop), 4
    batch = _batch(K * B)
    ok = dict(index=_out(1, 2, 24), stats=_fake_cuda(torch.zeros((1, 2, 12))), grads=_grads(one))
    bad = [
        (dict(handle=object()), "policy"), (dict(opt=optp), "opt"), (dict(opt=None), "opt"), (dict(coef=_fake_cuda(torch.zeros((1, 4)))), "coef"),
        (dict(batch=_batch(K * B - 1)), "batch"), (dict(batch=[1]), "batch"), (dict(steps=0), "steps"), (dict(epochs=65), "epochs"),
        (dict(minibatches=0), "minibatches"), (dict(minibatches=49), "minibatches"), (dict(unit="rows"), "unit"),
        (dict(clip_range=0.0), "clip_range"), (dict(ent_coef=-1.0), "ent_coef"), (dict(stats=_fake_cuda(torch.zeros((1, 2, 11)))), "stats"),
        (dict(index=_out(1, 2, 23)), "out"), (dict(step_dev=_fake_cuda(torch.zeros(1))), "step_dev"),
    ]
    for change, match in bad:
        kw = dict(dict(handle=one, opt=opt1, batch=batch, steps=K, epochs=1, minibatches=2, **ok), **change)
        with pytest.raises(ValueError, match=match):
            env.ppo_update_torch(**kw)
    # a population: its members must divide the envs, be at most 256, and coef is [P, 4]
    for members, match in ((5, "members"), (8, "members")):
        _, p5 = _handles(members)
        with pytest.raises(ValueError, match=match):
            env.ppo_update_torch(p5, _opt(p5), batch, K, 1, 2)
    with pytest.raises(ValueError, match="coef"):
        env.ppo_update_torch(pop, optp, batch, K, 1, 2, coef=_fake_cuda(torch.zeros((3, 3))))
    with pytest.raises(ValueError, match="opt"):
        env.ppo_update_torch(pop, opt1, batch, K, 1, 2)
    assert not env._lib.calls and not rec.calls


# ---------------------------------------------------------------------------------------------------------------- the build
NEW = r"\S*minibatch_\w+_kernel\S*"


def test_the_new_kernel_builds_for_gfx950_without_scratch_or_spills():
    """In the code object minibatch_index_kernel uses no scratch, 32 bytes of LDS (the eight round keys) and spills neither vector nor
    scalar registers; it fits 8 waves per SIMD (<= 64 VGPRs); the keys are formed on the scalar unit (Philox's multiply-high appears as s_mul_hi_u32, and no v_mul_hi_u32
    beyond the two of the per-lane divisions); no 64-bit division is called or expanded (no v_rcp / v_cvt of a float division); the
    stores are 8-byte global stores; no atomics"""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    assert b"sg_minibatch_size" in lib and b"sg_minibatch_index_device" in lib
    kernels = engine_asm.descriptors(NEW)
    assert len(kernels) == 1
    name, field = kernels[0]
    assert re.match(r"_Z\d+minibatch_index_kernel", name) and not re.search(r"_kernelI", name)
    assert field["private_segment_fixed_size"] == 0 and field["group_segment_fixed_size"] == 8 * 4
    assert field["next_free_vgpr"] <= 64, field["next_free_vgpr"]
    fn = engine_asm.function(name)
    ins = engine_asm.instructions(fn)
    assert not re.search(r"\bscratch_", fn) and "atomic" not in fn
    assert sum(i.startswith("s_mul_hi_u32") for i in ins) >= 40, "Philox is not on the scalar unit"
    assert sum(i.startswith("v_mul_hi_u32") for i in ins) <= 2
    assert not any(i.startswith(("v_rcp", "v_cvt_f32_u32", "v_cvt_f64", "v_div_")) for i in ins), "a division was expanded per lane"
    assert any(i.startswith("global_store_dwordx2") for i in ins) and not any(i.startswith(("global_store_dword ", "global_store_byte")) for i in ins)
    for kind in ("vgpr", "sgpr"):
        spills = engine_asm.spill_counts(NEW, kind)
        assert len(spills) == 1 and spills[0][1] == 0, (kind, spills)
    rows = [r for r in engine_asm.resource_rows() if "minibatch_index_kernel" in r["name"]]
    assert len(rows) == 1 and rows[0]["ScratchSize [bytes/lane]"] == "0" and rows[0]["VGPRs Spill"] == "0" and rows[0]["SGPRs Spill"] == "0", rows
