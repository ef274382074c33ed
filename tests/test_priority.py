"""CPU tests of prioritized replay sampling (sg_priority_*_device): the declarations and struct layouts, the Python front end with the
native calls stubbed (nothing reaches a kernel), the NumPy model (tests/priority_model.py) against a per-draw linear scan with Python
integers, the draw frequencies, and the resources of the new kernels in the gfx950 build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import engine_asm
from priority_model import STREAM_PRIORITY, Priorities, quantise, umul64hi_64
from replay_model import philox4x32_10
from test_episode_stats import _fake_cuda
from test_gae import _struct_fields
from test_replay import B, D, T, _env, _ring, _ring_arg_matches, _tlist
from test_snapshot_device import _header_args


# ---------------------------------------------------------------------------------------------- declarations
def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_priority_bytes", "size_t") == ["const sg_env *env", "int32_t steps", "size_t *member_bytes"]
    assert _header_args("sg_priority_begin_device") == ["sg_env *env", "const sg_priority *prio", "void *hip_stream"]
    assert _header_args("sg_priority_commit_device") == ["sg_env *env", "const sg_priority *prio", "int32_t first_slot",
                                                         "int32_t filled_before", "int32_t n_steps", "void *hip_stream"]
    assert _header_args("sg_priority_update_device") == ["sg_env *env", "const sg_priority *prio", "int64_t n", "const int64_t *cell_dev",
                                                         "const float *priority_dev", "void *hip_stream"]
    assert _header_args("sg_priority_sample_device") == [
        "sg_env *env", "const sg_replay *ring", "const sg_priority *prio", "const sg_priority_sample_config *cfg", "int64_t n",
        "const sg_priority_draw *out", "void *hip_stream"]
    assert _header_args("sg_priority_sample_config_init", "void") == ["sg_priority_sample_config *cfg"]
    vp = C.c_void_p
    S = _native.SYMBOLS
    P = C.POINTER(_native.SgPriority)
    assert S["sg_priority_bytes"] == (C.c_size_t, [vp, C.c_int32, C.POINTER(C.c_size_t)])
    assert S["sg_priority_begin_device"] == (C.c_int, [vp, P, vp])
    assert S["sg_priority_commit_device"] == (C.c_int, [vp, P, C.c_int32, C.c_int32, C.c_int32, vp])
    assert S["sg_priority_update_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp])
    assert S["sg_priority_sample_config_init"] == (None, [C.POINTER(_native.SgPrioritySampleConfig)])
    assert S["sg_priority_sample_device"] == (C.c_int, [vp, C.POINTER(_native.SgReplay), P, C.POINTER(_native.SgPrioritySampleConfig),
                                                        C.c_int64, C.POINTER(_native.SgPriorityDraw), vp])
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    for name, mirror, size in (("sg_priority", _native.SgPriority, 40), ("sg_priority_sample_config", _native.SgPrioritySampleConfig, 32),
                               ("sg_priority_draw", _native.SgPriorityDraw, 32)):
        decls = _struct_fields(name)
        assert [d.split()[-1].lstrip("*") for d in decls] == [f for f, _ in mirror._fields_], name
        for d, (_, ct) in zip(decls, mirror._fields_):
            assert ct is (C.c_void_p if "*" in d else ctype[d.split()[0]]), (name, d)
        assert C.sizeof(mirror) == size, name
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    assert "status code 9" in header and "the smallest cell c with q[0] + ... + q[c] > r" in header


# ---------------------------------------------------------------------------------------------- the front end, stubbed
def _prio(env, steps=T, frac_bits=16, nodes=64):
    import torch
    from space_gym_amd.vector_env import ReplayPriority
    z = lambda shape, dtype: _fake_cuda(torch.zeros(shape, dtype=dtype))  # noqa: E731
    return ReplayPriority(steps, B, frac_bits, leaf=z((steps, B), torch.int32), node=z((nodes,), torch.int64), hdr=z((16,), torch.int32))


def _prio_arg_matches(arg, prio):
    p = arg._obj
    assert (p.struct_size, p.steps, p.frac_bits, p.reserved) == (40, prio.steps, prio.frac_bits, 0)
    for k in prio.MEMBERS:
        assert getattr(p, k) == getattr(prio, k).data_ptr(), k


def test_the_calls_reach_the_native_entry_points_in_order():
    import torch
    env = _env()
    ring, prio = _ring(env), _prio(env, frac_bits=12)
    assert env.replay_priority_begin_torch(prio) is prio
    assert env._lib.names() == ["sg_priority_begin_device"]
    a = env._lib.calls[0][1]
    assert len(a) == 3
    _prio_arg_matches(a[1], prio)
    # the ring's commit, then the priorities' commit, with the same integers
    env.replay_commit_torch(ring, 4, terminal=_tlist(), priority=prio)
    env.replay_commit_torch(ring, 4, terminal=_tlist(), priority=prio)
    assert env._lib.names()[1:] == ["sg_replay_commit_device", "sg_priority_commit_device"] * 2
    r, p = env._lib.calls[-2][1], env._lib.calls[-1][1]
    assert tuple(r[2:5]) == tuple(p[2:5]) == (4, 4, 4) and len(p) == 6
    _prio_arg_matches(p[1], prio)
    assert (ring.head, ring.filled) == (8, 8)
    env.replay_priority_commit_torch(prio, 8, 8, 2)
    assert env._lib.calls[-1][0] == "sg_priority_commit_device" and tuple(env._lib.calls[-1][1][2:5]) == (8, 8, 2)
    # update: td errors are raised to alpha in torch, priorities pass straight through
    cell = _fake_cuda(torch.tensor([3, 5, 5], dtype=torch.int64))
    pri = _fake_cuda(torch.tensor([0.5, 2.0, 1.0]))
    env.replay_update_priorities_torch(prio, cell, priority=pri)
    a = env._lib.calls[-1][1]
    assert env._lib.calls[-1][0] == "sg_priority_update_device" and len(a) == 6
    assert a[2] == 3 and a[3].value == cell.data_ptr() and a[4].value == pri.data_ptr()
    # the draw
    out = dict(index=_fake_cuda(torch.zeros(7, dtype=torch.int64)), weight=_fake_cuda(torch.zeros(7)))
    assert env.replay_priority_draw_torch(ring, prio, 7, seed=2 ** 63 + 5, beta=0.7, stratified=False, out=out) is out
    a = env._lib.calls[-1][1]
    assert env._lib.calls[-1][0] == "sg_priority_sample_device" and len(a) == 7
    _ring_arg_matches(a[1], ring)
    _prio_arg_matches(a[2], prio)
    cfg, draw = a[3]._obj, a[5]._obj
    assert (cfg.struct_size, cfg.seed, cfg.beta, cfg.stratified) == (32, 2 ** 63 + 5, 0.7, 0) and a[4] == 7
    assert (draw.index, draw.weight, draw.cell, draw.leaf) == (out["index"].data_ptr(), out["weight"].data_ptr(), None, None)
    # the defaults are the header's
    out = dict(index=_fake_cuda(torch.zeros(3, dtype=torch.int64)), weight=_fake_cuda(torch.zeros(3)))
    env.replay_priority_draw_torch(ring, prio, 3, out=out)
    cfg = env._lib.calls[-1][1][3]._obj
    assert (cfg.seed, cfg.beta, cfg.stratified) == (0, 0.4, 1)


def test_the_prioritized_sample_draws_then_gathers_through_the_index_path():
    import torch
    env = _env()
    ring, prio = _ring(env), _prio(env)
    ring.head, ring.filled = 4, 4
    n = 5
    z = lambda shape, dtype=torch.float32: _fake_cuda(torch.ones(shape, dtype=dtype))  # noqa: E731
    out = dict(obs=z((n, D)), action=z((n, 2)), reward=z(n), next_obs=z((n, D)), terminated=z(n, torch.uint8), truncated=z(n, torch.uint8),
               index=z(n, torch.int64), cell=z(n, torch.int64), weight=z(n))
    assert env.replay_sample_prioritized_torch(ring, prio, n, seed=9, beta=0.5, n_step=3, gamma=0.9, normalize=False, out=out) is out
    assert env._lib.names() == ["sg_priority_sample_device", "sg_replay_sample_device"]
    d, g = env._lib.calls[0][1], env._lib.calls[1][1]
    assert d[5]._obj.index == out["index"].data_ptr() == g[4].value  # the gather reads what the draw wrote
    assert d[5]._obj.cell == out["cell"].data_ptr() and d[5]._obj.weight == out["weight"].data_ptr()
    assert (g[2]._obj.n_step, g[2]._obj.gamma) == (3, 0.9) and g[3] == n
    assert g[5]._obj.index == out["index"].data_ptr()


def test_without_priorities_the_commit_makes_exactly_the_native_call_it_made_before():
    env = _env()
    ring = _ring(env)
    tl = _tlist()
    env.replay_commit_torch(ring, 4, terminal=tl)
    env.replay_commit_torch(ring, 4, terminal=tl, priority=None)
    assert env._lib.names() == ["sg_replay_commit_device"] * 2
    assert [len(c[1]) for c in env._lib.calls] == [8, 8] and tuple(env._lib.calls[1][1][2:5]) == (4, 4, 4)


def _refusals():
    import torch
    z = torch.zeros
    i64 = lambda n: _fake_cuda(z(n, dtype=torch.int64))  # noqa: E731
    f32 = lambda n: _fake_cuda(z(n))  # noqa: E731

    def draw(**kw):
        return lambda env, ring, prio: env.replay_priority_draw_torch(ring, prio, **{"n": 4, **kw})

    def upd(*a, **kw):
        return lambda env, ring, prio: env.replay_update_priorities_torch(prio, *a, **kw)

    def broken(member, t):
        def go(env, ring, prio):
            setattr(prio, member, t)
            env.replay_priority_begin_torch(prio)
        return go

    def frac(env, ring, prio):
        prio.frac_bits = 32
        env.replay_priority_begin_torch(prio)
    return {
        "n negative": draw(n=-1), "seed negative": draw(seed=-1), "beta negative": draw(beta=-0.1), "beta nan": draw(beta=float("nan")),
        "out\\['index'\\] dtype": draw(out=dict(index=_fake_cuda(z(4, dtype=torch.int32)), weight=f32(4))),
        "out\\['weight'\\] shape": draw(out=dict(index=i64(4), weight=f32(5))),
        "out\\['cell'\\] host": draw(out=dict(index=i64(4), weight=f32(4), cell=z(4, dtype=torch.int64))),
        "priority: made for a ring": lambda env, ring, prio: env.replay_priority_draw_torch(ring, _prio(env, steps=T + 1), 4),
        "priority: expected the object": lambda env, ring, prio: env.replay_priority_begin_torch(dict(leaf=prio.leaf)),
        "priority.leaf dtype": broken("leaf", _fake_cuda(z((T, B), dtype=torch.int64))),
        "priority.hdr shape": broken("hdr", _fake_cuda(z(8, dtype=torch.int32))),
        "priority.node host": broken("node", z(64, dtype=torch.int64)),
        "frac_bits": frac,
        "exactly one both": upd(i64(3), td_error=f32(3), priority=f32(3)), "exactly one neither": upd(i64(3)),
        "cell dtype": upd(_fake_cuda(z(3, dtype=torch.int32)), priority=f32(3)), "td_error shape": upd(i64(3), td_error=f32(4)),
        "priority shape": upd(i64(3), priority=f32(2)), "alpha": upd(i64(3), td_error=f32(3), alpha=-1.0),
        "cross the end": lambda env, ring, prio: env.replay_priority_commit_torch(prio, 10, 4, 4),
        "n_steps zero": lambda env, ring, prio: env.replay_priority_commit_torch(prio, 0, 0, 0),
        "filled_before": lambda env, ring, prio: env.replay_priority_commit_torch(prio, 0, T + 1, 1),
        "priority: made for a ring of 13": lambda env, ring, prio: env.replay_commit_torch(ring, 1, terminal=_tlist(),
                                                                                        priority=_prio(env, steps=T + 1)),
    }


@pytest.mark.parametrize("bad", sorted(_refusals()))
def test_host_refusals_raise_before_any_native_call(bad):
    env = _env()
    ring, prio = _ring(env), _prio(env)
    ring.head, ring.filled = 4, 4
    match = {"n negative": "n:", "seed negative": "seed", "beta negative": "beta", "beta nan": "beta", "exactly one both": "exactly one",
             "exactly one neither": "exactly one", "n_steps zero": "n_steps", "cell dtype": "cell", "td_error shape": "td_error",
             "priority shape": "priority"}.get(bad, bad.rsplit(" ", 1)[0] if bad.split()[-1] in ("dtype", "shape", "host") else bad)
    with pytest.raises(ValueError, match=match):
        _refusals()[bad](env, ring, prio)
    assert env._lib.calls == [] and (ring.head, ring.filled) == (4, 4)


def test_an_empty_ring_and_auto_reset_off_are_refused():
    env = _env()
    ring, prio = _ring(env), _prio(env)
    with pytest.raises(ValueError, match="no valid transition"):
        env.replay_priority_draw_torch(ring, prio, 4)
    off = _env(auto_reset=0)
    for call in (lambda: off.replay_priority_begin_torch(prio), lambda: off.replay_priority_commit_torch(prio, 0, 0, 1),
                 lambda: off.replay_priority_draw_torch(ring, prio, 4), lambda: off.replay_priority_torch(ring)):
        with pytest.raises(ValueError, match="auto_reset"):
            call()
    assert env._lib.calls == [] and off._lib.calls == []


# ---------------------------------------------------------------------------------------------- the model itself
def _scan(q, r):
    """the definition, one draw, Python integers: the smallest cell c with q[0] + ... + q[c] > r"""
    acc = 0
    for c, x in enumerate(q):
        acc += int(x)
        if acc > r:
            return c
    raise AssertionError("r >= total")


def _numbers_by_hand(m, n, seed, stratified):
    total = m.total
    out = []
    for j in range(n):
        w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (j & 0xFFFFFFFF, j >> 32, m.sample_calls, STREAM_PRIORITY))
        x = int(w[0][0]) | int(w[1][0]) << 32
        if stratified:
            each, rest = divmod(total, n)
            out.append(j * each + min(j, rest) + ((x * (each + (j < rest))) >> 64))
        else:
            out.append((x * total) >> 64)
    return out


def test_umul64hi_and_quantisation():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 64, 300, dtype=np.uint64)
    for n in (0, 1, 2 ** 31 - 1, 2 ** 40 + 12345, 2 ** 63 - 1, 2 ** 64 - 1):
        assert [int(v) for v in umul64hi_64(x, n)] == [(int(v) * n) >> 64 for v in x]
    q, ok = quantise(np.array([0.0, 1e-9, 1.0, 0.5 + 2.0 ** -17, 1.5 * 2.0 ** -16, 2.5 * 2.0 ** -16, 70000.0, np.nan, -1.0, np.inf, -0.0], np.float32), 16)
    assert ok.tolist() == [True] * 7 + [False, False, False, True]
    # p = 0 gives 1; ties round to even; 2^32 - 1 is the ceiling
    assert q[:7].tolist() == [1, 1, 65536, 32768, 2, 2, 2 ** 32 - 1] and q[10] == 1
    assert quantise(np.float32(3.0), 0)[0] == 3 and quantise(np.float32(1.0), 31)[0] == 2 ** 31


@pytest.mark.parametrize("stratified", [True, False])
def test_model_equals_the_per_draw_linear_scan(stratified):
    """three laps of a small ring with updates in between: after every commit the draw of the model (cumsum + searchsorted, uint64)
    equals a linear scan with Python integers over numbers r computed by hand; the strata tile [0, total) exactly, also when
    total mod n != 0; the hole slot and never-filled slots are never drawn"""
    Tn, Bn, K = 6, 7, 2
    m = Priorities(Tn, Bn, frac_bits=8)
    rng = np.random.default_rng(4)
    first = 0
    tiled_uneven = False
    for c in range(3 * Tn // K):
        m.commit(first, m.filled, K)
        first = (first + K) % Tn
        hole = np.arange(m.head * Bn, (m.head + 1) * Bn)
        assert (m.q[hole] == 0).all() and m.head == first
        valid = m.slot_valid(np.arange(Tn))
        assert valid.sum() == m.valid and ((m.q.reshape(Tn, Bn) > 0) == valid[:, None]).all()
        cells = rng.integers(0, Tn * Bn, 9)
        m.update(cells, rng.uniform(0, 3, 9).astype(np.float32))
        assert ((m.q.reshape(Tn, Bn) > 0) == valid[:, None]).all()  # an update never makes an invalid cell samplable
        for n in (1, 5, 13):
            total = m.total
            if stratified:
                each, rest = divmod(total, n)
                tiled_uneven |= rest != 0
                lo = [j * each + min(j, rest) for j in range(n + 1)]
                assert lo[0] == 0 and lo[n] == total and all(lo[j + 1] - lo[j] == each + (j < rest) for j in range(n))
            want_r = _numbers_by_hand(m, n, 77, stratified)
            assert [int(x) for x in m.numbers(n, 77, stratified)] == want_r  # the model's numbers are the definition's
            got = m.sample(n, seed=77, beta=0.5, stratified=stratified, ring_head=m.head, ring_filled=m.filled)
            assert [int(x) for x in m.numbers(n, 77, stratified)] != want_r  # (the call number moved on)
            if stratified:
                assert all(lo[j] <= want_r[j] < lo[j + 1] for j in range(n))
            want_cell = [_scan(m.q, r) for r in want_r]
            assert got["cell"].tolist() == want_cell
            assert not np.isin(got["cell"], hole).any()
            p, i = got["cell"] // Bn, got["cell"] % Bn
            assert got["index"].tolist() == [((int(a) - (m.head - m.valid)) % Tn) * Bn + int(b) for a, b in zip(p, i)]
            assert (got["index"] >= 0).all() and (got["index"] < m.valid * Bn).all()
            assert got["leaf"].tolist() == m.q[got["cell"]].tolist()
    assert not m.status and (not stratified or tiled_uneven)


def test_updates_largest_wins_stale_cells_are_skipped_and_max_q_is_monotone():
    m = Priorities(4, 5, frac_bits=16)
    m.commit(0, 0, 2)  # slots 0, 1 valid; hole = slot 2; slot 3 never filled
    assert m.max_q == 65536 and m.total == 10 * 65536
    on = m.update([3, 3, 3, 7, 12, 17], np.array([0.5, 2.0, 1.0, 0.25, 9.0, 9.0], np.float32))
    assert on.tolist() == [True] * 4 + [False, False] and not m.status  # the hole and the never-filled slot: silently
    assert m.q[3] == 2 * 65536 and m.q[7] == 16384 and m.q[12] == 0 and m.q[17] == 0
    assert m.max_q == 2 * 65536  # 9.0 was not applied, so it does not count
    again = Priorities(4, 5, frac_bits=16)
    again.commit(0, 0, 2)
    again.update([7, 3, 3, 3], np.array([0.25, 1.0, 0.5, 2.0], np.float32))  # any order
    assert np.array_equal(again.q, m.q)
    m.update([3], np.array([0.125], np.float32))
    assert m.q[3] == 8192 and m.max_q == 2 * 65536  # monotone
    m.commit(2, 2, 1)
    assert (m.q[10:15] == 2 * 65536).all() and (m.q[15:20] == 0).all() and m.head == 3
    # refused rows set the status word and leave the rest applied
    on = m.update([0, -1, 20, 1, 2, 4], np.array([1.0, 1.0, 1.0, np.nan, -2.0, np.inf], np.float32))
    assert on.tolist() == [True, False, False, False, False, False] and m.status and m.q[0] == 65536


def test_device_refusals_of_the_model_and_beta_zero():
    m = Priorities(4, 5, frac_bits=0)
    assert m.sample(3) is None and m.status  # total = 0
    m.begin()
    m.commit(0, 0, 1)  # 5 cells of q = 1
    assert m.total == 5 and m.sample(6, stratified=True) is None and m.status  # more strata than units
    m.status = False
    assert m.sample(6, stratified=False) is not None and m.sample(5, stratified=True)["cell"].tolist() == [0, 1, 2, 3, 4]
    assert m.sample(2, ring_head=2, ring_filled=2) is None and m.status  # the priorities lag the ring
    m.status = False
    m.update([0, 1], np.array([7.0, 3.0], np.float32))
    w = m.sample(64, beta=0.0, stratified=False)
    assert (w["weight"] == np.float32(1.0)).all() and len(set(w["cell"].tolist())) > 1
    w = m.sample(64, beta=1.0, stratified=False)
    assert np.array_equal(w["weight64"], m.total / (5.0 * w["leaf"])) or np.allclose(w["weight64"], m.total / (5.0 * w["leaf"]), rtol=1e-15)


def test_draw_frequencies_are_proportional_to_q():
    """n = 400 000 independent draws over 300 valid cells with priorities spread over a factor of 50: every cell's count within
    5 standard deviations of its binomial expectation n p_c (sigma_c^2 = n p_c (1 - p_c)), and the chi-square statistic within
    5 sigma of its mean (299 degrees of freedom: mean 299, variance 598).  Stratified draws: a stratum is total // n or total // n + 1 units
    long and holds one draw, so a cell of q units meets at most q / (total // n) + 2 strata and contains at least
    q / (total // n + 1) - 2 whole ones: its count lies between the two."""
    Tn, Bn, n = 4, 100, 400_000
    m = Priorities(Tn, Bn, frac_bits=16)
    m.commit(0, 0, 3)
    rng = np.random.default_rng(11)
    m.update(np.arange(300), rng.uniform(0.1, 5.0, 300).astype(np.float32))
    p = m.q[:300].astype(np.float64) / m.total
    got = m.sample(n, seed=2024, stratified=False)
    hist = np.bincount(got["cell"], minlength=Tn * Bn)
    assert hist[300:].sum() == 0
    assert (np.abs(hist[:300] - n * p) <= 5.0 * np.sqrt(n * p * (1 - p))).all()
    chi2 = ((hist[:300] - n * p) ** 2 / (n * p)).sum()
    assert abs(chi2 - 299) <= 5.0 * np.sqrt(2.0 * 299)
    strat = np.bincount(m.sample(n, seed=2024, stratified=True)["cell"], minlength=Tn * Bn)
    each, q = m.total // n, m.q[:300].astype(np.float64)
    assert each > 100 and (strat[:300] <= q / each + 2).all() and (strat[:300] >= q / (each + 1) - 2).all() and strat[300:].sum() == 0


# ---------------------------------------------------------------------------------------------- the build
def test_the_status_message_of_a_refused_priority_call_is_reachable():
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    inc = open(os.path.join(build.CSRC, "sg_priority.inc")).read()
    assert "sg_priority.inc" in build.HEADERS and '#include "sg_priority.inc"' in src
    assert int(re.search(r"constexpr int kStatusPriority = (\d+);", inc).group(1)) == 9
    others = "".join(open(os.path.join(build.CSRC, f)).read() for f in ("sg_engine.hip", "sg_gae.inc", "sg_replay.inc", "sg_device.hpp"))
    assert 9 not in [int(v) for v in re.findall(r"constexpr int kStatus\w+ = (\d+);", others)]
    assert re.search(r"constexpr uint32_t kStreamPriority = 4u;", inc)
    assert "kStreamPriority, w)" in engine_asm.function_body(inc, "void priority_draw_kernel(")
    for sig in ("static int status_error(sg_env *e, const char *who)", 'extern "C" int sg_check_status(sg_env *e)'):
        assert re.search(r"if \(st == kStatusPriority\)\s*return fail\(", engine_asm.function_body(src, sig)), sig
    lib = open(build.build(), "rb").read()
    assert b"sg_priority_*_device: priorities without a matching header" in lib
    assert b"an earlier sg_priority_*_device call refused its input on the device" in lib


def test_the_new_kernels_build_for_gfx950_without_scratch():
    """In the code object the priority kernels use no scratch and spill no register; only the one-workgroup top kernel needs LDS
    (one level of at most 64 sums: 512 B); the draw kernel stays within 128 VGPRs; no instruction writes memory through the scalar
    unit, scratch, flat or buffer addressing; the integer atomics are the update's and they are global_atomic_* instructions"""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    for name in (b"sg_priority_bytes", b"sg_priority_begin_device", b"sg_priority_commit_device", b"sg_priority_update_device",
                 b"sg_priority_sample_device", b"sg_priority_sample_config_init", b"priority_draw_kernel", b"priority_commit_kernel",
                 b"priority_update_kernel", b"priority_level_kernel", b"priority_top_kernel", b"priority_begin_kernel"):
        assert name in lib
    kernels = engine_asm.descriptors(r"\S*priority_\w+_kernel\S*")
    # begin, commit, update<0 | 1>, level, top, tick, draw
    assert len(kernels) == 8, [k for k, _ in kernels]
    for name, field in kernels:
        assert not re.search(r"replay_\w+_kernel|profile|snapshot_kernel|_restore_kernel|gae_\w+_kernel", name), name
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == (512 if "top" in name else 0), name
        assert field["next_free_vgpr"] <= 128, name
    spills = engine_asm.spill_counts(r"\S*priority_\w+_kernel\S*")
    assert len(spills) == 8 and all(n == 0 for _, n in spills), spills
    sspills = engine_asm.spill_counts(r"\S*priority_\w+_kernel\S*", kind="sgpr")
    assert len(sspills) == 8 and all(n == 0 for _, n in sspills), sspills
    for name, _ in kernels:
        fn = engine_asm.function(name)
        writes = set(re.findall(r"^\s+(\w*(?:store|atomic)\w*)\s", fn, flags=re.M))
        allowed = {"global_store_dword", "global_store_dwordx2", "global_store_dwordx3", "global_store_dwordx4"}
        if "update" in name:
            allowed |= {"global_atomic_swap", "global_atomic_umax", "global_atomic_add_x2"}
        if "top" in name:
            allowed |= {"ds_write_b64", "ds_store_b64"}
        assert writes and writes <= allowed, (name, sorted(writes))
        assert not re.search(r"\b(scratch_|buffer_store|flat_store|flat_atomic)", fn), name
        if "update" in name:
            assert any(w.startswith("global_atomic") for w in writes), name
