"""CPU tests of the PBT calls (sg_pbt_fitness_device / sg_pbt_fitness_clear_device / sg_pbt_select_device / sg_pbt_explore_device,
pbt_fitness_torch / pbt_fitness_update_torch / pbt_fitness_clear_torch / pbt_select_torch / pbt_explore_torch): the
declarations, the NumPy statement (tests/pbt_model.py) against independent arithmetic, the properties of the selection, the shares of
its draws, explore's modes, the Python argument checks with the native calls stubbed, and the resources of the new kernels."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import engine_asm
import pbt_model as pm
from test_episode_stats import _fake_cuda, _stub_env
from test_snapshot_device import _header_args

METHODS = ("pbt_fitness_torch", "pbt_fitness_update_torch", "pbt_fitness_clear_torch", "pbt_select_torch", "pbt_explore_torch")


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_pbt_fitness_device") == [
        "sg_env *env", "int32_t members", "int32_t n_steps", "const float *reward", "const uint8_t *done", "double *env_return",
        "int32_t *env_length", "double *table", "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_pbt_fitness_workspace_bytes", "size_t") == ["sg_env *env", "int32_t members"]
    assert _header_args("sg_pbt_fitness_clear_device") == ["sg_env *env", "int32_t members", "double *table", "const int32_t *src",
                                                           "void *hip_stream"]
    assert _header_args("sg_pbt_select_device") == [
        "sg_env *env", "int32_t members", "const double *fitness", "int64_t fitness_stride", "const uint8_t *ready", "int32_t k",
        "uint64_t seed", "uint64_t step", "const int64_t *step_dev", "int32_t *src_out", "int32_t *rank_out", "int32_t *count_out",
        "void *hip_stream"]
    assert _header_args("sg_pbt_explore_device") == [
        "sg_env *env", "int32_t members", "const int32_t *src", "int32_t n_columns", "const sg_pbt_column *columns", "uint64_t seed",
        "uint64_t step", "const int64_t *step_dev", "int32_t *refused_out", "void *hip_stream"]
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    S = _native.SYMBOLS
    assert S["sg_pbt_fitness_device"] == (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.c_size_t, vp])
    assert S["sg_pbt_fitness_workspace_bytes"] == (C.c_size_t, [vp, i32])
    assert S["sg_pbt_fitness_clear_device"] == (C.c_int, [vp, i32, vp, vp, vp])
    assert S["sg_pbt_select_device"] == (C.c_int, [vp, i32, vp, i64, vp, i32, u64, u64, vp, vp, vp, vp, vp])
    assert S["sg_pbt_explore_device"] == (C.c_int, [vp, i32, vp, i32, C.POINTER(_native.SgPbtColumn), u64, u64, vp, vp, vp])


def test_the_column_struct_and_the_constants_mirror_the_header():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    header = open(os.path.join(build.ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct sg_pbt_column {"):header.index("} sg_pbt_column;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct sg_pbt_column {", "")
    decls = [d.strip() for d in body.split(";") if d.strip()]
    ctype = {"float *": C.c_void_p, "int64_t ": C.c_int64, "int32_t ": C.c_int32, "float ": C.c_float}
    want = [(d.split()[-1].lstrip("*"), ctype[d[:len(d) - len(d.split()[-1].lstrip("*"))]]) for d in decls]
    assert want == list(_native.SgPbtColumn._fields_)
    assert [f for f, _ in want] == ["data", "stride", "mode", "down", "up", "lo", "hi"]
    offsets = {f: getattr(_native.SgPbtColumn, f).offset for f, _ in want}
    assert offsets == dict(data=0, stride=8, mode=16, down=20, up=24, lo=28, hi=32) and C.sizeof(_native.SgPbtColumn) == 40
    for name, value in (("SG_PBT_COPY", pm.COPY), ("SG_PBT_SCALE", pm.SCALE), ("SG_PBT_SCALE_COMPLEMENT", pm.SCALE_COMPLEMENT)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert SpaceGymVectorEnv.pbt_modes == dict(copy=pm.COPY, scale=pm.SCALE, scale_complement=pm.SCALE_COMPLEMENT)
    assert SpaceGymVectorEnv.pbt_fitness_names == pm.NAMES and len(pm.NAMES) == 8
    assert (SpaceGymVectorEnv.pbt_max_members, SpaceGymVectorEnv.pbt_max_columns) == (pm.MAX_MEMBERS, pm.MAX_COLUMNS) == (256, 16)
    flat = " ".join(header.split()).replace(" * ", " ")
    assert "(episodes, return_sum, length_sum, return_sq_sum, return_max, return_min, fitness, reserved)" in flat


def test_the_kernels_live_in_sg_pbt_inc_after_sg_adam_inc_and_use_no_atomics():
    from space_gym_amd import build
    assert "sg_pbt.inc" in build.HEADERS and build.HEADERS.index("sg_pbt.inc") == build.HEADERS.index("sg_adam.inc") + 1
    engine = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert engine.count('#include "sg_pbt.inc"') == 1
    assert engine.index('#include "sg_adam.inc"') < engine.index('#include "sg_pbt.inc"') < engine.index("struct sg_env {")
    inc = open(os.path.join(build.CSRC, "sg_pbt.inc")).read()
    kernels = re.findall(r"void (\w+_kernel)\(", inc)
    assert kernels == ["pbt_fitness_scan_kernel", "pbt_fitness_combine_kernel", "pbt_fitness_clear_kernel", "pbt_select_kernel",
                       "pbt_explore_kernel"]
    code = re.sub(r"//.*", "", inc)
    assert "atomic" not in code.lower() and "template" not in code
    # both stream tags, 9 and 10: written from kStreamSequence = 8 and pinned by a static_assert; no other tag has either value
    assert re.search(r"kStreamSequence = 8u\b", open(os.path.join(build.CSRC, "sg_sequence.inc")).read())
    assert re.search(r"kStreamPbtSelect = kStreamSequence \+ 1u;", code) and re.search(r"kStreamPbtExplore = kStreamSequence \+ 2u;", code)
    assert re.search(r"static_assert\(kStreamPbtSelect == %du && kStreamPbtExplore == %du," % (pm.STREAM_SELECT, pm.STREAM_EXPLORE), code)
    assert (pm.STREAM_SELECT, pm.STREAM_EXPLORE) == (9, 10)
    literal = [int(v) for f in sorted(os.listdir(build.CSRC)) for v in re.findall(r"\bkStream\w+ = (\d+)u", open(os.path.join(build.CSRC, f)).read())]
    assert sorted(literal) == list(range(9)), literal
    assert len(re.findall(r"kStreamPbtSelect, o\)", code)) == 1 and len(re.findall(r"kStreamPbtExplore, o\)", code)) == 1
    assert re.search(r"kPbtChunk = %d\b" % pm.CHUNK, code) and re.search(r"kPbtMaxMembers = %d\b" % pm.MAX_MEMBERS, code)
    assert re.search(r"kPbtMaxColumns = %d\b" % pm.MAX_COLUMNS, code)
    assert "fmaf" not in code and "__fdividef" not in code  # every operation rounds on its own


def test_the_methods_are_net_methods_and_the_multi_device_front_ends_refuse_them():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    assert set(METHODS) <= set(NET_METHODS) and all(callable(getattr(SpaceGymVectorEnv, n)) for n in METHODS)
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in METHODS:
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))


# ---------------------------------------------------------------------------------------------------------------- the model against plain arithmetic
def _rows(rng, K, B, nan_at=None):
    """done at 10 %, rewards over a wide exponent range"""
    reward = (rng.standard_normal((K, B)) * 10.0 ** rng.integers(-6, 7, (K, B))).astype(np.float32)
    done = (rng.random((K, B)) < 0.1).astype(np.uint8)
    if nan_at is not None:
        reward[nan_at] = np.nan
    return reward, done


def _plain(reward_calls, done_calls, B, P):
    """per env, a Python loop over all the calls' rows: the finished episodes (return as the float64 running sum, length)"""
    E = B // P
    episodes = [[] for _ in range(P)]
    run, ln = [0.0] * B, [0] * B
    for reward, done in zip(reward_calls, done_calls):
        for t in range(reward.shape[0]):
            for i in range(B):
                run[i] += float(reward[t, i])
                ln[i] += 1
                if done[t, i]:
                    episodes[i // E].append((run[i], ln[i]))
                    run[i], ln[i] = 0.0, 0
    return episodes, run, ln


@pytest.mark.parametrize("B,P", [(192, 3), (1040, 2), (64, 64), (512, 1)])
def test_the_model_equals_a_plain_loop_over_two_calls(B, P):
    rng = np.random.default_rng(B + P)
    calls = [_rows(rng, 7, B), _rows(rng, 20, B)]
    table, run, ln = pm.fresh_table(P), np.zeros(B), np.zeros(B, np.int32)
    for reward, done in calls:
        table, run, ln = pm.fitness_update(table, run, ln, reward, done)
    episodes, prun, pln = _plain([c[0] for c in calls], [c[1] for c in calls], B, P)
    assert run.tolist() == prun and ln.tolist() == pln and ln.dtype == np.int32
    assert sum(1 for ep in episodes if ep) >= max(1, P // 2)
    for m in range(P):
        ep = episodes[m]
        if not ep:  # (E = 1: some members finish nothing in 27 rows)
            assert table[m, :6].tolist() == list(pm.IDENTITY) and np.isnan(table[m, pm.FITNESS])
            continue
        assert table[m, pm.EPISODES] == len(ep) and table[m, pm.LENGTH_SUM] == sum(l for _, l in ep)
        assert table[m, pm.RETURN_MAX] == max(r for r, _ in ep) and table[m, pm.RETURN_MIN] == min(r for r, _ in ep)
        s, q = math.fsum(r for r, _ in ep), math.fsum(r * r for r, _ in ep)
        scale = math.fsum(abs(r) for r, _ in ep)
        assert abs(table[m, pm.RETURN_SUM] - s) <= 1e-12 * scale
        assert abs(table[m, pm.RETURN_SQ_SUM] - q) <= 1e-12 * q
        assert table[m, pm.FITNESS] == table[m, pm.RETURN_SUM] / len(ep)
        assert table[m, pm.RESERVED] == 0


def test_a_member_without_a_finished_episode_has_the_identities_and_a_nan_fitness():
    reward, done = np.ones((3, 8), np.float32), np.zeros((3, 8), np.uint8)
    done[2, 5] = 1
    table, run, ln = pm.fitness_update(pm.fresh_table(2), np.zeros(8), np.zeros(8, np.int32), reward, done)
    assert table[0, :6].tolist() == list(pm.IDENTITY) and np.isnan(table[0, pm.FITNESS])
    assert table[1].tolist()[:7] == [1, 3, 3, 9, 3, 3, 3]
    assert run.tolist() == [3, 3, 3, 3, 3, 0, 3, 3] and ln.tolist() == [3, 3, 3, 3, 3, 0, 3, 3]


def test_a_nan_reward_stays_within_its_member_and_the_order_is_the_chunk_tree():
    rng = np.random.default_rng(3)
    B, P = 1040, 2
    reward, done = _rows(rng, 20, B)
    bad = reward.copy()
    bad[4, 700] = np.nan
    done[10, 700] = 1  # (the episode with the NaN finishes inside the rows)
    clean = pm.fitness_update(pm.fresh_table(P), np.zeros(B), np.zeros(B, np.int32), reward, done)[0]
    got = pm.fitness_update(pm.fresh_table(P), np.zeros(B), np.zeros(B, np.int32), bad, done)[0]
    assert got[0].tobytes() == clean[0].tobytes()
    assert np.isnan(got[1, pm.RETURN_SUM]) and np.isnan(got[1, pm.FITNESS]) and got[1, pm.EPISODES] == clean[1, pm.EPISODES]
    assert np.isfinite(got[1, pm.RETURN_MAX]) and np.isfinite(got[1, pm.RETURN_MIN])  # fmax / fmin pass a NaN by
    # the stated order differs from a left-to-right sum in the last bits on these rows: the order is observable
    w = pm.env_windows(reward, done, np.zeros(B), np.zeros(B, np.int32))[0]
    left = [functools.reduce(lambda x, y: x + y, w[m * 520:(m + 1) * 520, 1].tolist()) for m in range(P)]
    assert any(left[m] != clean[m, pm.RETURN_SUM] for m in range(P))
    assert pm.workspace_bytes(1040, 2) == 2 * 3 * 48 and pm.workspace_bytes(256, 256) == 256 * 48 and pm.workspace_bytes(192, 3) == 3 * 48


def test_clear_with_and_without_src():
    rng = np.random.default_rng(4)
    table = rng.random((4, 8))
    fresh = pm.fresh_table(1)[0]
    every = pm.fitness_clear(table)
    assert all(every[m].tobytes() == fresh.tobytes() for m in range(4))
    some = pm.fitness_clear(table, [0, 0, 2, 0])
    assert some[0].tobytes() == table[0].tobytes() and some[2].tobytes() == table[2].tobytes()
    assert some[1].tobytes() == fresh.tobytes() and some[3].tobytes() == fresh.tobytes()


# ---------------------------------------------------------------------------------------------------------------- selection
def _fitness_cases(P, rng):
    base = rng.standard_normal(P)
    ties = np.round(base * 2) / 2
    wild = base.copy()
    wild[rng.random(P) < 0.2] = np.inf
    wild[rng.random(P) < 0.2] = -np.inf
    wild[rng.random(P) < 0.2] = np.nan
    ready = rng.random(P) < 0.7
    yield base, None
    yield ties, None
    yield wild, None
    yield wild, ready
    yield ties, ready
    yield np.full(P, np.nan), None                      # r = 0
    one = np.full(P, np.nan)
    one[P // 2] = 1.0
    yield one, None                                     # r = 1
    yield np.zeros(P), np.zeros(P, bool)                # nobody is ready
    yield np.zeros(P), None                             # all tied


@pytest.mark.parametrize("P", [1, 2, 5, 64, 256])
@pytest.mark.parametrize("fraction", [0.2, 0.5])
def test_selection_properties(P, fraction):
    rng = np.random.default_rng(100 + P)
    k = pm.truncation_count(fraction, P)
    assert k == int(fraction * P) and k <= P // 2
    for n, (f, ready) in enumerate(_fitness_cases(P, rng)):
        src, rank, (copies, k_eff) = pm.select(f, ready, k, seed=7, step=n)
        part = ~np.isnan(f) & (np.ones(P, bool) if ready is None else ready)
        r = int(part.sum())
        assert k_eff == min(k, r // 2) == copies
        assert src.dtype == np.int32 and rank.dtype == np.int32
        assert (rank[~part] == -1).all() and sorted(rank[part].tolist()) == list(range(r))
        order = sorted(np.flatnonzero(part).tolist(), key=lambda m: (-f[m], m))  # descending fitness, ties to the lower index
        assert [int(rank[m]) for m in order] == list(range(r))
        assert (src[src] == src).all() and ((0 <= src) & (src < P)).all()
        dest = np.flatnonzero(src != np.arange(P))
        assert sorted(dest.tolist()) == sorted(order[r - k_eff:] if k_eff else [])  # exactly the bottom k_eff
        assert all(rank[src[m]] < k_eff for m in dest)                          # every source has top rank
        assert (src[~part] == np.flatnonzero(~part)).all()
        assert pm.exploit_sources(src)[1] == 0                                    # adam_exploit_torch refuses nothing


def test_selection_reads_both_words_of_step_and_step_dev_adds_to_it():
    f = np.random.default_rng(1).standard_normal(64)
    a = pm.select(f, None, 12, seed=3, step=5)[0]
    assert not np.array_equal(a, pm.select(f, None, 12, seed=3, step=6)[0])
    assert not np.array_equal(a, pm.select(f, None, 12, seed=3, step=5 + 2 ** 32)[0])
    assert not np.array_equal(a, pm.select(f, None, 12, seed=4, step=5)[0])
    assert not np.array_equal(a, pm.select(f, None, 12, seed=3 + 2 ** 32, step=5)[0])
    assert np.array_equal(a, pm.select(f, None, 12, seed=3, step=2, step_dev=3)[0])
    assert np.array_equal(a, pm.select(f, None, 12, seed=3, step=2 ** 64 - 1, step_dev=6)[0])  # a 64-bit sum
    assert np.array_equal(pm.select(f, None, 12, seed=3, step=2 ** 32 - 1, step_dev=1)[0], pm.select(f, None, 12, seed=3, step=2 ** 32)[0])


def test_the_share_of_every_top_member_is_within_four_standard_deviations():
    """P = 256, k = 51, 400 steps: 20 400 draws over 51 winners, each with n p = 400 and sd = sqrt(n p (1 - p)) = 19.8"""
    P, k, steps = 256, 51, 400
    f = np.random.default_rng(2).standard_normal(P)
    counts = np.zeros(P, np.int64)
    for step in range(steps):
        src, rank, _ = pm.select(f, None, k, seed=11, step=step)
        dest = src != np.arange(P)
        assert dest.sum() == k
        np.add.at(counts, src[dest], 1)
    top = np.flatnonzero(pm.select(f, None, k)[1] < k)
    assert counts.sum() == counts[top].sum() == steps * k
    n, p = steps * k, 1.0 / k
    assert np.abs(counts[top] - n * p).max() <= 4.0 * math.sqrt(n * p * (1 - p)), counts[top]


def test_the_up_share_of_the_explore_draw_is_within_four_standard_deviations():
    ups = sum(int(pm.explore_bits(256, 16, seed=11, step=step).sum()) for step in range(25))
    n = 25 * 256 * 16
    assert abs(ups - n / 2) <= 4.0 * math.sqrt(n / 4), (ups, n)
    per_column = sum(pm.explore_bits(256, 16, seed=11, step=step).sum(axis=1) for step in range(25))
    assert np.abs(per_column - 25 * 128).max() <= 4.0 * math.sqrt(25 * 256 / 4), per_column


# ---------------------------------------------------------------------------------------------------------------- explore
def _explore_case(P=6, seed=0):
    rng = np.random.default_rng(seed)
    hyper = rng.random((P, 8)).astype(np.float32) * np.float32(1e-3)
    coef = rng.random((P, 4)).astype(np.float32)
    disc = (0.9 + 0.1 * rng.random((P, 2))).astype(np.float32)
    cols = [pm.column(hyper, 0, pm.SCALE, lo=1e-5, hi=1e-3), pm.column(hyper, 1, pm.SCALE_COMPLEMENT), pm.column(hyper, 3, pm.COPY),
            pm.column(coef, 2, pm.SCALE, down=0.5, up=2.0), pm.column(disc, 0, pm.SCALE_COMPLEMENT, lo=0.9, hi=0.9999),
            pm.column(disc, 1, pm.COPY)]
    return hyper, coef, disc, cols


def test_explore_model_modes_clamp_and_untouched_rows():
    hyper, coef, disc, cols = _explore_case()
    before = [t.copy() for t in (hyper, coef, disc)]
    src = np.array([0, 1, 0, 1, 4, 0], np.int32)
    assert pm.explore(src, cols, seed=5, step=9) == 0
    up = pm.explore_bits(6, len(cols), seed=5, step=9)
    assert up.any() and not up.all()
    for t, b in zip((hyper, coef, disc), before):
        assert t[[0, 1, 4]].tobytes() == b[[0, 1, 4]].tobytes()     # members with src[m] == m keep their bits
    f32 = np.float32
    for m, s in ((2, 0), (3, 1), (5, 0)):
        f = lambda c: f32(cols[c]["up"] if up[c, m] else cols[c]["down"])
        assert hyper[m, 0] == min(max(f32(before[0][s, 0] * f(0)), f32(1e-5)), f32(1e-3))
        assert hyper[m, 1] == f32(f32(1) - f32(f32(f32(1) - before[0][s, 1]) * f(1)))
        assert hyper[m, 3] == before[0][s, 3] and coef[m, 2] == f32(before[1][s, 2] * f(3))
        assert disc[m, 0] == min(max(f32(f32(1) - f32(f32(f32(1) - before[2][s, 0]) * f(4))), f32(0.9)), f32(0.9999))
        assert disc[m, 1] == before[2][s, 1]
        assert hyper[m, 2] == before[0][m, 2] and coef[m, 0] == before[1][m, 0]  # columns that were not named
    assert (hyper[:, 0] <= f32(1e-3)).all() and (disc[:, 0] <= f32(0.9999)).all()
    # the clamp binds somewhere in this case
    big = np.full((6, 1), 1e-3, np.float32)
    pm.explore(src, [pm.column(big, 0, pm.SCALE, down=2.0, up=2.0, hi=1.5e-3)], seed=1)
    assert big[[2, 3, 5], 0].tolist() == [f32(1.5e-3)] * 3 and big[[0, 1, 4], 0].tolist() == [f32(1e-3)] * 3


def test_explore_model_refuses_chains_and_sources_out_of_range():
    hyper, coef, disc, cols = _explore_case()
    before = [t.copy() for t in (hyper, coef, disc)]
    src = np.array([2, 0, 2, 7, -1, 2], np.int32)  # 1 <- 0 is a chain (0 is a destination); 3 and 4 are out of range
    assert pm.explore(src, cols, seed=5) == 3
    for t, b in zip((hyper, coef, disc), before):
        assert t[[1, 2, 3, 4]].tobytes() == b[[1, 2, 3, 4]].tobytes()
    assert (hyper[[0, 5], 3] == before[0][2, 3]).all() and (disc[[0, 5], 1] == before[2][2, 1]).all()


# ---------------------------------------------------------------------------------------------------------------- Python checks, native calls stubbed
B, P = 12, 3


def _fit(env, members=P):
    import torch
    from space_gym_amd.vector_env import PbtFitness
    return PbtFitness(members, _fake_cuda(torch.zeros(env.num_envs, dtype=torch.float64)), _fake_cuda(torch.zeros(env.num_envs, dtype=torch.int32)),
                      _fake_cuda(torch.zeros((members, 8), dtype=torch.float64)), _fake_cuda(torch.zeros(members * 6, dtype=torch.float64)))


def test_pbt_fitness_torch_refuses_bad_members_before_any_native_call():
    env = _stub_env(B=B)
    for members in (0, -1, 257, 5, 8):
        with pytest.raises(ValueError, match="members"):
            env.pbt_fitness_torch(members)
    assert not env._lib.calls


def test_fitness_update_and_clear_check_and_reach_the_native_calls():
    import torch
    env = _stub_env(B=B)
    fit = _fit(env)
    reward, done = _fake_cuda(torch.zeros((5, B))), _fake_cuda(torch.zeros((5, B), dtype=torch.bool))
    bad = [(None, reward, done, "fit"), (fit, torch.zeros((5, B)), done, "reward"), (fit, _fake_cuda(torch.zeros((0, B))), done, "reward"),
           (fit, _fake_cuda(torch.zeros((5, B + 1))), done, "reward"), (fit, _fake_cuda(torch.zeros((5, B), dtype=torch.float64)), done, "reward"),
           (fit, _fake_cuda(torch.zeros(B)), done, "reward"), (fit, reward, _fake_cuda(torch.zeros((4, B), dtype=torch.uint8)), "done"),
           (fit, reward, _fake_cuda(torch.zeros((5, B), dtype=torch.int32)), "done")]
    for f, r, d, match in bad:
        with pytest.raises(ValueError, match=match):
            env.pbt_fitness_update_torch(f, r, d)
    for attr, value in (("table", _fake_cuda(torch.zeros((P, 8)))), ("env_return", _fake_cuda(torch.zeros(B))),
                        ("env_length", _fake_cuda(torch.zeros(B, dtype=torch.int64))), ("workspace", _fake_cuda(torch.zeros(64, dtype=torch.uint8))),
                        ("members", 5)):
        broken = _fit(env)
        setattr(broken, attr, value)
        with pytest.raises(ValueError, match="members" if attr == "members" else "fit." + attr):
            env.pbt_fitness_update_torch(broken, reward, done)
    with pytest.raises(ValueError, match="src"):
        env.pbt_fitness_clear_torch(fit, _fake_cuda(torch.zeros(P, dtype=torch.int64)))
    with pytest.raises(ValueError, match="src"):
        env.pbt_fitness_clear_torch(fit, _fake_cuda(torch.zeros(P + 1, dtype=torch.int32)))
    assert not env._lib.calls
    assert env.pbt_fitness_update_torch(fit, reward, done) is fit.table
    name, a = env._lib.calls[-1]
    assert name == "sg_pbt_fitness_device" and a[1:3] == (P, 5) and a[9] == P * 48
    assert [x.value for x in a[3:9]] == [t.data_ptr() for t in (reward, done, fit.env_return, fit.env_length, fit.table, fit.workspace)]
    src = _fake_cuda(torch.zeros(P, dtype=torch.int32))
    assert env.pbt_fitness_clear_torch(fit, src) is fit.table and env.pbt_fitness_clear_torch(fit) is fit.table
    (n1, a1), (n2, a2) = env._lib.calls[-2:]
    assert n1 == n2 == "sg_pbt_fitness_clear_device" and a1[1] == P and a1[2].value == fit.table.data_ptr()
    assert a1[3].value == src.data_ptr() and a2[3] is None
    assert fit.fitness.data_ptr() == fit.table.data_ptr() + 48 and fit.fitness.stride(0) == 8


def test_select_checks_and_reaches_the_native_call():
    import torch
    env = _stub_env(B=B)
    table = _fake_cuda(torch.zeros((5, 8), dtype=torch.float64))
    f = table[:, 6]
    for fraction in (0.0, -0.1, 0.51, float("nan")):
        with pytest.raises(ValueError, match="fraction"):
            env.pbt_select_torch(f, fraction=fraction)
    for bad in (torch.zeros(5, dtype=torch.float64), _fake_cuda(torch.zeros(5)), _fake_cuda(torch.zeros((5, 1), dtype=torch.float64)), [0.0] * 5):
        with pytest.raises(ValueError, match="fitness"):
            env.pbt_select_torch(bad)
    with pytest.raises(ValueError, match="members"):
        env.pbt_select_torch(_fake_cuda(torch.zeros(257, dtype=torch.float64)))
    for kw, match in ((dict(ready=_fake_cuda(torch.zeros(4, dtype=torch.uint8))), "ready"), (dict(ready=_fake_cuda(torch.zeros(5))), "ready"),
                      (dict(out=_fake_cuda(torch.zeros(5, dtype=torch.int64))), "out"), (dict(rank=_fake_cuda(torch.zeros(6, dtype=torch.int32))), "rank"),
                      (dict(count=_fake_cuda(torch.zeros(1, dtype=torch.int32))), "count"),
                      (dict(step_dev=_fake_cuda(torch.zeros(1, dtype=torch.int32))), "step_dev"),
                      (dict(step_dev=_fake_cuda(torch.zeros(2, dtype=torch.int64))), "step_dev")):
        with pytest.raises(ValueError, match=match):
            env.pbt_select_torch(f, **kw)
    assert not env._lib.calls
    out, rank, count = (_fake_cuda(torch.zeros(n, dtype=torch.int32)) for n in (5, 5, 2))
    ready, step_dev = _fake_cuda(torch.ones(5, dtype=torch.bool)), _fake_cuda(torch.zeros(1, dtype=torch.int64))
    assert env.pbt_select_torch(f, ready=ready, fraction=0.4, seed=3, step=2 ** 40, step_dev=step_dev, out=out, rank=rank, count=count) is out
    name, a = env._lib.calls[-1]
    assert name == "sg_pbt_select_device" and a[1] == 5 and a[2].value == table.data_ptr() + 48 and a[3] == 8
    assert a[4].value == ready.data_ptr() and a[5:8] == (2, 3, 2 ** 40)
    assert [x.value for x in a[8:12]] == [t.data_ptr() for t in (step_dev, out, rank, count)]
    env.pbt_select_torch(_fake_cuda(torch.zeros(5, dtype=torch.float64)), out=out)
    a = env._lib.calls[-1][1]
    assert a[3] == 1 and a[4] is None and a[5] == 1 and a[8] is None and a[10] is None and a[11] is None


def test_explore_checks_and_reaches_the_native_call():
    import torch
    env = _stub_env(B=B)
    src = _fake_cuda(torch.zeros(P, dtype=torch.int32))
    hyper, coef, disc = (_fake_cuda(torch.zeros((P, c))) for c in (8, 4, 2))
    ok = dict(mode="scale")
    bad = [([], "columns"), ([(hyper, 0, ok)] * 17, "columns"), ([(hyper, 8, ok)], "column"), ([(hyper, -1, ok)], "column"),
           ([(hyper, 0.5, ok)], "column"), ([(hyper, 0, dict(mode="resample"))], "mode"), ([(hyper, 0, dict(mode=3))], "mode"),
           ([(hyper, 0, dict())], "mode"), ([(hyper, 0, dict(mode="scale", factor=2))], "spec"),
           ([(hyper, 0, dict(mode="scale", down=float("nan")))], "NaN"), ([(hyper, 0, dict(mode="scale", up=float("nan")))], "NaN"),
           ([(hyper, 0, dict(mode="scale", lo=float("nan")))], "NaN"), ([(hyper, 0, dict(mode="scale", hi=float("nan")))], "NaN"),
           ([(hyper, 0, dict(mode="scale", lo=2.0, hi=1.0))], "lo"), ([(torch.zeros((P, 8)), 0, ok)], "CUDA tensor"),
           ([(_fake_cuda(torch.zeros((P + 1, 8))), 0, ok)], "tensor"), ([(_fake_cuda(torch.zeros((P, 8), dtype=torch.float64)), 0, ok)], "tensor"),
           ([(_fake_cuda(torch.zeros(P)), 0, ok)], "tensor"), ([(hyper, 0)], "spec")]
    for columns, match in bad:
        with pytest.raises(ValueError, match=match):
            env.pbt_explore_torch(src, columns)
    with pytest.raises(ValueError, match="src"):
        env.pbt_explore_torch(_fake_cuda(torch.zeros(P, dtype=torch.int64)), [(hyper, 0, ok)])
    with pytest.raises(ValueError, match="refused"):
        env.pbt_explore_torch(src, [(hyper, 0, ok)], refused=_fake_cuda(torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="step_dev"):
        env.pbt_explore_torch(src, [(hyper, 0, ok)], step_dev=_fake_cuda(torch.zeros(1)))
    assert not env._lib.calls
    refused, step_dev = _fake_cuda(torch.zeros(1, dtype=torch.int32)), _fake_cuda(torch.zeros(1, dtype=torch.int64))
    columns = [(hyper, 0, dict(mode="scale", lo=1e-5, hi=1e-2)), (hyper, 1, dict(mode="scale_complement", down=0.5, up=2.0)),
               (coef, 2, dict(mode="copy")), (disc, 1, dict(mode=pm.SCALE_COMPLEMENT, hi=0.9999))]
    assert env.pbt_explore_torch(src, columns, seed=9, step=4, step_dev=step_dev, refused=refused) is refused
    name, a = env._lib.calls[-1]
    assert name == "sg_pbt_explore_device" and a[1] == P and a[2].value == src.data_ptr() and a[3] == 4 == len(a[4]) and a[5:7] == (9, 4)
    assert a[7].value == step_dev.data_ptr() and a[8].value == refused.data_ptr()
    rows = [(r.data, r.stride, r.mode, r.down, r.up, r.lo, r.hi) for r in a[4]]
    f32 = lambda x: float(np.float32(x))
    assert rows == [(hyper.data_ptr(), 8, pm.SCALE, f32(0.8), 1.25, f32(1e-5), f32(1e-2)),
                    (hyper.data_ptr() + 4, 8, pm.SCALE_COMPLEMENT, 0.5, 2.0, -np.inf, np.inf),
                    (coef.data_ptr() + 8, 4, pm.COPY, f32(0.8), 1.25, -np.inf, np.inf),
                    (disc.data_ptr() + 4, 2, pm.SCALE_COMPLEMENT, f32(0.8), 1.25, -np.inf, f32(0.9999))]
    assert env.pbt_explore_torch(src, columns[:1]) is None and env._lib.calls[-1][1][7] is None and env._lib.calls[-1][1][8] is None


# ---------------------------------------------------------------------------------------------------------------- the build
NEW = r"\S*pbt_\w+_kernel\S*"


def test_the_new_kernels_build_for_gfx950_without_scratch_or_spills():
    """In the code object the five kernels use no scratch and spill neither vector nor scalar registers; the scan fits 4 waves per
    SIMD (<= 128 VGPRs); LDS is what the sources declare (the scan's six trees of 256 doubles, the select's fitness, flags and inverse
    ranks, the explore's counts; none for the one-lane-per-member kernels); no float64 or float32 operation of the scan, select or explore is fused"""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    for name in (b"sg_pbt_fitness_device", b"sg_pbt_fitness_workspace_bytes", b"sg_pbt_fitness_clear_device", b"sg_pbt_select_device",
                 b"sg_pbt_explore_device"):
        assert name in lib
    kernels = dict(engine_asm.descriptors(NEW))
    lds = {"pbt_fitness_scan_kernel": 6 * 256 * 8, "pbt_fitness_combine_kernel": 0, "pbt_fitness_clear_kernel": 0,
           "pbt_select_kernel": 256 * 8 + 2 * 256 * 4, "pbt_explore_kernel": 256 * 4}
    assert len(kernels) == 5 and sorted(re.match(r"_Z\d+(\w+_kernel)", k).group(1) for k in kernels) == sorted(lds)
    for name, field in kernels.items():
        short = re.match(r"_Z\d+(\w+_kernel)", name).group(1)
        assert not re.search(r"_kernelI", name), name  # plain kernels: no template arguments
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == lds[short], (name, field["group_segment_fixed_size"])
        assert field["next_free_vgpr"] <= 128, (name, field["next_free_vgpr"])
        fn = engine_asm.function(name)
        if short != "pbt_fitness_combine_kernel":  # (its one float64 division is the correctly rounded sequence, which uses v_fma_f64)
            assert not re.search(r"\bv_fma_f64\b|\bv_fma_f32\b|\bv_fmac_f32\b|\bv_mad_f32\b", fn), name
        assert not re.search(r"\bscratch_", fn) and "atomic" not in fn, name
    for kind in ("vgpr", "sgpr"):
        spills = engine_asm.spill_counts(NEW, kind)
        assert len(spills) == 5 and all(n == 0 for _, n in spills), (kind, spills)
