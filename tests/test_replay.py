"""CPU tests of the replay ring (sg_replay_bytes / sg_replay_begin_device / sg_replay_commit_device / sg_replay_sample_device): the
declarations and struct layouts, the Python front end with the native calls stubbed (nothing reaches a kernel), the NumPy model
(tests/replay_model.py) against an independent per-draw formulation, and the resources of the new kernels in the gfx950 build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import engine_asm
from replay_model import Ring, draws, philox4x32_10, sample, synthetic, umul64hi
from test_episode_stats import _fake_cuda, _stub_env
from test_gae import _struct_fields
from test_snapshot_device import _header_args

B, D, T = 8, 13, 12


# ---------------------------------------------------------------------------------------------- declarations
def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_replay_bytes", "size_t") == ["const sg_env *env", "int32_t steps", "uint32_t term_capacity", "size_t *member_bytes"]
    assert _header_args("sg_replay_begin_device") == ["sg_env *env", "const sg_replay *ring", "const float *obs0_dev", "void *hip_stream"]
    assert _header_args("sg_replay_commit_device") == [
        "sg_env *env", "const sg_replay *ring", "int32_t first_slot", "int32_t filled_before", "int32_t n_steps",
        "const sg_terminal_list *terminal_list", "const float *terminal_obs_dense_dev", "void *hip_stream"]
    assert _header_args("sg_replay_sample_device") == [
        "sg_env *env", "const sg_replay *ring", "const sg_replay_sample_config *cfg", "int64_t n", "const int64_t *index_in_dev",
        "const sg_replay_batch *out", "void *hip_stream"]
    assert _header_args("sg_replay_sample_config_init", "void") == ["sg_replay_sample_config *cfg"]
    vp = C.c_void_p
    S = _native.SYMBOLS
    assert S["sg_replay_bytes"] == (C.c_size_t, [vp, C.c_int32, C.c_uint32, C.POINTER(C.c_size_t)])
    assert S["sg_replay_begin_device"] == (C.c_int, [vp, C.POINTER(_native.SgReplay), vp, vp])
    assert S["sg_replay_commit_device"] == (C.c_int, [vp, C.POINTER(_native.SgReplay), C.c_int32, C.c_int32, C.c_int32,
                                                      C.POINTER(_native.SgTerminalList), vp, vp])
    assert S["sg_replay_sample_device"] == (C.c_int, [vp, C.POINTER(_native.SgReplay), C.POINTER(_native.SgReplaySampleConfig), C.c_int64, vp,
                                                      C.POINTER(_native.SgReplayBatch), vp])
    assert S["sg_replay_sample_config_init"] == (None, [C.POINTER(_native.SgReplaySampleConfig)])
    assert "sg_replay_commit" not in S and "sg_replay_sample" not in S  # no host-array forms: the ring is device memory
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    for name, mirror, size in (("sg_replay", _native.SgReplay, 88), ("sg_replay_sample_config", _native.SgReplaySampleConfig, 32),
                               ("sg_replay_batch", _native.SgReplayBatch, 72)):
        decls = _struct_fields(name)
        assert [d.split()[-1].lstrip("*") for d in decls] == [f for f, _ in mirror._fields_], name
        for d, (_, ct) in zip(decls, mirror._fields_):
            assert ct is (C.c_void_p if "*" in d else ctype[d.split()[0]]), (name, d)
        assert C.sizeof(mirror) == size, name
    assert [f for f, _ in _native.SgReplay._fields_][4:] == ["obs", "action", "reward", "done", "trunc", "term_idx", "term_obs", "slot_seq", "hdr"]
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    assert "needs auto_reset on" in header and "status code 8" in header


# ---------------------------------------------------------------------------------------------- the front end, stubbed
def _env(discrete=False, auto_reset=1):
    from space_gym_amd import _native
    env = _stub_env(B=B, D=D)
    env.discrete = discrete
    env._cfg = _native.SgConfig(auto_reset=auto_reset)
    return env


def _ring(env, steps=T, cap=5):
    import torch
    from space_gym_amd.vector_env import ReplayRing
    z = lambda shape, dtype: _fake_cuda(torch.zeros(shape, dtype=dtype))  # noqa: E731
    return ReplayRing(steps=steps, num_envs=B, obs_dim=D, term_capacity=cap, discrete=env.discrete, obs=z((steps, B, D), torch.float32),
                      action=z((steps, B), torch.int32) if env.discrete else z((steps, B, 2), torch.float32),
                      reward=z((steps, B), torch.float32), done=z((steps, B), torch.uint8), trunc=z((steps, B), torch.uint8),
                      term_idx=z((steps, B), torch.int32), term_obs=z((cap, D), torch.float32), slot_seq=z((steps,), torch.int32),
                      hdr=z((8,), torch.int32))


def _tlist(cap=6):
    import torch
    return dict(count=_fake_cuda(torch.zeros(1, dtype=torch.int32)), step_env=_fake_cuda(torch.zeros((cap, 2), dtype=torch.int32)),
                obs=_fake_cuda(torch.zeros((cap, D))))


def _ring_arg_matches(arg, ring):
    r = arg._obj
    assert (r.struct_size, r.steps, r.term_capacity, r.reserved) == (88, ring.steps, ring.term_capacity, 0)
    for k in ring.MEMBERS:
        assert getattr(r, k) == getattr(ring, k).data_ptr(), k


def test_begin_commit_and_sample_reach_the_native_calls_in_order():
    import torch
    env = _env()
    ring = _ring(env)
    obs0 = _fake_cuda(torch.zeros((B, D)))
    assert env.replay_begin_torch(ring, obs0) is ring and env.replay_begin_torch(ring) is ring
    assert env._lib.names() == ["sg_replay_begin_device"] * 2
    a = env._lib.calls[0][1]
    _ring_arg_matches(a[1], ring)
    assert len(a) == 4 and a[2].value == obs0.data_ptr() and env._lib.calls[1][1][2] is None
    # list form: 4 slots at the head
    tl = _tlist()
    env.replay_commit_torch(ring, 4, terminal=tl)
    a = env._lib.calls[-1][1]
    assert env._lib.names()[-1] == "sg_replay_commit_device" and len(a) == 8
    _ring_arg_matches(a[1], ring)
    assert tuple(a[2:5]) == (0, 0, 4) and a[6] is None
    t = a[5]._obj
    assert (t.count, t.step_env, t.obs, t.capacity) == (tl["count"].data_ptr(), tl["step_env"].data_ptr(), tl["obs"].data_ptr(), 6)
    assert (ring.head, ring.filled, len(ring)) == (4, 4, 4 * B)
    # dense form: one slot
    tobs = _fake_cuda(torch.zeros((B, D)))
    env.replay_commit_torch(ring, 1, terminal_obs=tobs)
    a = env._lib.calls[-1][1]
    assert tuple(a[2:5]) == (4, 4, 1) and a[5] is None and a[6].value == tobs.data_ptr()
    assert (ring.head, ring.filled) == (5, 5)
    # sample
    idx = _fake_cuda(torch.zeros(7, dtype=torch.int64))
    out = env.replay_sample_torch(ring, 7, seed=2 ** 63 + 5, n_step=3, gamma=0.5, index=idx,
                                  out={k: _fake_cuda(v) for k, v in dict(
                                      obs=torch.zeros((7, D)), action=torch.zeros((7, 2)), reward=torch.zeros(7), next_obs=torch.zeros((7, D)),
                                      terminated=torch.zeros(7, dtype=torch.uint8), truncated=torch.zeros(7, dtype=torch.uint8),
                                      steps=torch.zeros(7, dtype=torch.uint8)).items()})
    a = env._lib.calls[-1][1]
    assert env._lib.names()[-1] == "sg_replay_sample_device" and len(a) == 7
    _ring_arg_matches(a[1], ring)
    cfg, batch = a[2]._obj, a[5]._obj
    assert (cfg.struct_size, cfg.seed, cfg.n_step, cfg.gamma) == (32, 2 ** 63 + 5, 3, 0.5)
    assert a[3] == 7 and a[4].value == idx.data_ptr()
    for k in ("obs", "action", "reward", "next_obs", "terminated", "truncated", "steps"):
        assert getattr(batch, k) == out[k].data_ptr(), k
    assert batch.discount is None and batch.index is None
    # the defaults are the header's
    env._torch_bufs = None
    assert (lambda c: (c.seed, c.n_step, c.gamma))(_default_cfg(env, ring)) == (0, 1, 0.99)


def _default_cfg(env, ring):
    import torch
    n = 3
    out = {k: _fake_cuda(v) for k, v in dict(
        obs=torch.zeros((n, D)), action=torch.zeros((n, 2)), reward=torch.zeros(n), next_obs=torch.zeros((n, D)),
        terminated=torch.zeros(n, dtype=torch.uint8), truncated=torch.zeros(n, dtype=torch.uint8)).items()}
    env.replay_sample_torch(ring, n, out=out)
    assert env._lib.calls[-1][1][4] is None
    return env._lib.calls[-1][1][2]._obj


def test_rows_are_views_at_the_mirrored_head_and_len_follows_the_valid_window():
    env = _env()
    ring = _ring(env)
    env.replay_begin_torch(ring)
    assert len(ring) == 0
    seen = []
    for c in range(7):  # 4 slots per commit, T = 12: two and a third laps
        rows = ring.rows(4)
        p = ring.head
        assert p == (4 * c) % T and set(rows) == {"obs", "action", "reward", "done", "trunc"}
        for k, v in rows.items():
            full = getattr(ring, k)
            assert v.shape[0] == 4 and v.data_ptr() == full[p].data_ptr() and v.is_contiguous(), k
        env.replay_commit_torch(ring, 4, terminal=_tlist())
        seen.append(len(ring))
        assert env._lib.calls[-1][1][2:5] == (p, min(4 * c, T), 4)
    assert seen == [4 * B, 8 * B] + [(T - 1) * B] * 5
    with pytest.raises(ValueError, match="cross the end"):
        ring.rows(9)


def test_discrete_rings_carry_int32_actions():
    import torch
    env = _env(discrete=True)
    ring = _ring(env)
    assert ring.action.dtype == torch.int32 and tuple(ring.action.shape) == (T, B)
    env.replay_begin_torch(ring)
    env.replay_commit_torch(ring, 2, terminal=_tlist())
    with pytest.raises(ValueError, match="action"):
        env.replay_sample_torch(ring, 4, out=dict(
            obs=_fake_cuda(torch.zeros((4, D))), action=_fake_cuda(torch.zeros((4, 2))), reward=_fake_cuda(torch.zeros(4)),
            next_obs=_fake_cuda(torch.zeros((4, D))), terminated=_fake_cuda(torch.zeros(4, dtype=torch.uint8)),
            truncated=_fake_cuda(torch.zeros(4, dtype=torch.uint8))))


def _refusals():
    import torch
    z = torch.zeros

    def commit(**kw):
        return lambda env, ring: env.replay_commit_torch(ring, **kw)

    def smp(**kw):
        return lambda env, ring: env.replay_sample_torch(ring, **{"n": 4, **kw})

    def broken(member, t):
        def go(env, ring):
            setattr(ring, member, t)
            env.replay_begin_torch(ring)
        return go
    return {
        "cross the end": commit(n_steps=9, terminal=_tlist()),
        "n_steps zero": commit(n_steps=0, terminal=_tlist()),
        "exactly one both": commit(n_steps=1, terminal=_tlist(), terminal_obs=_fake_cuda(z((B, D)))),
        "exactly one neither": commit(n_steps=1),
        "describe one step": commit(n_steps=2, terminal_obs=_fake_cuda(z((B, D)))),
        "terminal_obs shape": commit(n_steps=1, terminal_obs=_fake_cuda(z((B, D + 1)))),
        "terminal_obs host": commit(n_steps=1, terminal_obs=z((B, D))),
        "count dtype": commit(n_steps=1, terminal={**_tlist(), "count": _fake_cuda(z(1, dtype=torch.int64))}),
        "step_env shape": commit(n_steps=1, terminal={**_tlist(), "step_env": _fake_cuda(z((6, 3), dtype=torch.int32))}),
        "obs width": commit(n_steps=1, terminal={**_tlist(), "obs": _fake_cuda(z((6, D - 1)))}),
        "n_step high": smp(n_step=17), "n_step low": smp(n_step=0),
        "gamma high": smp(gamma=1.5), "gamma nan": smp(gamma=float("nan")),
        "n negative": smp(n=-1), "seed negative": smp(seed=-1),
        "index dtype": smp(index=_fake_cuda(z(4, dtype=torch.int32))), "index shape": smp(index=_fake_cuda(z(5, dtype=torch.int64))),
        "index host": smp(index=z(4, dtype=torch.int64)),
        "out reward": smp(out=dict(obs=_fake_cuda(z((4, D))), action=_fake_cuda(z((4, 2))), reward=_fake_cuda(z(5)),
                                   next_obs=_fake_cuda(z((4, D))), terminated=_fake_cuda(z(4, dtype=torch.uint8)),
                                   truncated=_fake_cuda(z(4, dtype=torch.uint8)))),
        "ring.obs host": broken("obs", z((T, B, D))),
        "ring.term_idx dtype": broken("term_idx", _fake_cuda(z((T, B), dtype=torch.int64))),
        "ring.hdr shape": broken("hdr", _fake_cuda(z(4, dtype=torch.int32))),
        "ring.slot_seq stride": broken("slot_seq", _fake_cuda(z(2 * T, dtype=torch.int32)[::2])),
        "expected the object": lambda env, ring: env.replay_begin_torch(dict(obs=ring.obs)),
    }


@pytest.mark.parametrize("bad", sorted(_refusals()))
def test_host_refusals_raise_before_any_native_call(bad):
    env = _env()
    ring = _ring(env)
    ring.head, ring.filled = 4, 4  # (as after one commit of 4 slots)
    with pytest.raises(ValueError, match=bad.rsplit(" ", 1)[0] if bad.split()[0] in ("cross", "exactly", "describe", "expected") else bad.split()[0]):
        _refusals()[bad](env, ring)
    assert env._lib.calls == [] and (ring.head, ring.filled) == (4, 4)


def test_an_empty_ring_and_auto_reset_off_are_refused():
    env = _env()
    ring = _ring(env)
    with pytest.raises(ValueError, match="no valid transition"):
        env.replay_sample_torch(ring, 4)
    off = _env(auto_reset=0)
    for call in (lambda: off.replay_torch(8), lambda: off.replay_begin_torch(ring), lambda: off.replay_commit_torch(ring, 1, terminal=_tlist()),
                 lambda: off.replay_sample_torch(ring, 4)):
        with pytest.raises(ValueError, match="auto_reset"):
            call()
    assert env._lib.calls == [] and off._lib.calls == []
    for steps, cap, what in ((1, None, "steps"), (2 ** 29, None, "steps \\* num_envs"), (8, 0, "term_capacity")):
        with pytest.raises(ValueError, match=what):
            env.replay_torch(steps, cap)


# ---------------------------------------------------------------------------------------------- the model itself
def test_philox_known_answers_and_umul64hi():
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        assert tuple(int(w[0]) for w in philox4x32_10(key, ctr)) == want
    # vectorised over the counter: the same words as one call each
    j = np.array([0, 1, 2 ** 32 - 1, 12345], np.uint64)
    w = philox4x32_10((7, 9), (j, 0, 3, 3))
    for n, c0 in enumerate(j):
        assert tuple(int(x[n]) for x in w) == tuple(int(x[0]) for x in philox4x32_10((7, 9), (int(c0), 0, 3, 3)))
    rng = np.random.default_rng(0)
    for _ in range(200):
        x, n = int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 31))
        assert int(umul64hi(x & 0xFFFFFFFF, x >> 32, n)) == (x * n) >> 64
    assert int(umul64hi(0xFFFFFFFF, 0xFFFFFFFF, 2 ** 31 - 1)) == 2 ** 31 - 2


def _brute(ring, term_dense, u, n_step, gamma):
    """one draw, from the definition, with Python integers, NumPy float64 scalars and the dense terminal copy"""
    T, Bn, v, h = ring.T, ring.B, ring.valid, ring.head
    q, i = divmod(int(u), Bn)
    p = [(h - v + q + k) % T for k in range(n_step)]
    R, g, last = np.float64(ring.reward[p[0], i]), np.float64(gamma), 0
    for k in range(1, n_step):
        if ring.done[p[k - 1], i] or q + k >= v:
            break
        R = R + g * np.float64(ring.reward[p[k], i])
        g = g * np.float64(gamma)
        last = k
    pl = p[last]
    fin = bool(ring.done[pl, i])
    return dict(obs=ring.obs[(p[0] - 1) % T, i], action=ring.action[p[0], i], reward=np.float32(R),
                next_obs=term_dense[pl, i] if fin else ring.obs[pl, i], terminated=np.uint8(fin and not ring.trunc[pl, i]),
                truncated=np.uint8(ring.trunc[pl, i]), discount=np.float32(g), steps=np.uint8(last + 1), index=np.int64(u)), p[:last + 1]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("dense", [False, True])
def test_model_equals_the_per_draw_definition(dense):
    ring, _, extra = synthetic(12, 9, 5, laps=2.5, K=4, p_done=0.15, seed=3, dense=dense, C=64)
    assert not ring.status and ring.filled == 12 and len(ring) == 11 * 9
    assert ring.done.any() and (ring.done & ring.trunc).any() and (ring.done & ~ring.trunc).any()
    every = np.arange(len(ring))
    for n_step in (1, 3, 16):
        got, ok = sample(ring, every.size, n_step=n_step, gamma=0.97, index=every, advance=False)
        assert ok.all()
        for u in every:
            want, path = _brute(ring, extra["term_dense"], u, n_step, 0.97)
            for k, w in want.items():
                assert np.array_equal(_bits(got[k][u]), _bits(np.asarray(w))), (n_step, u, k)
            # a walk never crosses a done nor the newest edge
            assert not ring.done[path[:-1], u % 9].any() and u // 9 + len(path) - 1 < ring.valid
            assert all((ring.head - 1 - p) % 12 < ring.valid for p in path)


def test_one_step_samples_are_the_stored_transitions_and_negative_zero_survives():
    ring, _, extra = synthetic(8, 50, 4, laps=2.5, K=2, p_done=0.1, seed=5)
    every = np.arange(len(ring))
    got, _ = sample(ring, every.size, n_step=1, gamma=0.9, index=every, advance=False)
    q, i = every // 50, every % 50
    p = (ring.head - ring.valid + q) % 8
    assert np.array_equal(_bits(got["reward"]), _bits(ring.reward[p, i]))
    neg = np.signbit(ring.reward[p, i]) & (ring.reward[p, i] == 0)
    assert neg.sum() > 0 and np.signbit(got["reward"][neg]).all()
    assert np.array_equal(_bits(got["obs"]), _bits(ring.obs[(p - 1) % 8, i])) and np.array_equal(_bits(got["action"]), _bits(ring.action[p, i]))
    fin = ring.done[p, i] != 0
    assert np.array_equal(_bits(got["next_obs"][~fin]), _bits(ring.obs[p, i][~fin]))
    assert np.array_equal(_bits(got["next_obs"][fin]), _bits(extra["term_dense"][p, i][fin]))
    assert (got["discount"] == np.float32(0.9)).all() and (got["steps"] == 1).all()
    # -0.0 also survives as the first reward of a longer walk that stops at once
    got3, _ = sample(ring, every.size, n_step=3, gamma=0.9, index=every, advance=False)
    stop = got3["steps"] == 1
    assert np.array_equal(_bits(got3["reward"][stop]), _bits(ring.reward[p, i][stop]))


def test_model_refusals():
    ring, commits, _ = synthetic(8, 20, 3, laps=1.0, K=2, p_done=0.2, seed=7, C=200)
    assert not ring.status
    out, ok = sample(ring, 4, index=[0, -1, len(ring), len(ring) - 1], advance=False)
    assert ok.tolist() == [True, False, False, True]
    r = Ring(8, 20, 3, 64)
    r.begin()
    se = np.array([[0, 1], [2, 0], [0, 20], [-1, 3], [1, 19]], np.int32)
    r.commit_list(0, 2, 5, se, np.ones((5, 3), np.float32), 5)
    assert r.status and r.term_head == 5 and r.term_idx[0, 1] == 0 and r.term_idx[1, 19] == 4
    r = Ring(8, 20, 3, 64)
    r.begin()
    r.commit_list(0, 2, 6, se, np.ones((5, 3), np.float32), 5)  # count > capacity
    assert r.status and r.term_head == 5
    # a terminal ring too small for the live window
    small, _, _ = synthetic(8, 20, 3, laps=2.0, K=2, p_done=0.5, seed=8, C=5)
    assert small.status


def test_draws_are_uniform_over_the_cells():
    """10^6 draws over v B = 1 000 cells: every cell within 5 sigma of n / cells (sigma^2 = n p (1 - p)), and the chi-square
    statistic within 5 sigma of its mean (999 degrees of freedom: mean 999, variance 1 998)"""
    n, cells = 10 ** 6, 1000
    u = draws(seed=12345, call=7, n=n, cells=cells)
    assert u.min() >= 0 and u.max() < cells
    hist = np.bincount(u, minlength=cells)
    p = 1.0 / cells
    assert np.abs(hist - n * p).max() <= 5.0 * np.sqrt(n * p * (1 - p))
    chi2 = ((hist - n * p) ** 2 / (n * p)).sum()
    assert abs(chi2 - (cells - 1)) <= 5.0 * np.sqrt(2.0 * (cells - 1))
    assert not np.array_equal(u, draws(seed=12345, call=8, n=n, cells=cells))  # the call number is part of the counter


# ---------------------------------------------------------------------------------------------- the build
def test_the_status_message_of_a_refused_replay_call_is_reachable():
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    inc = open(os.path.join(build.CSRC, "sg_replay.inc")).read()
    assert "sg_replay.inc" in build.HEADERS and '#include "sg_replay.inc"' in src
    assert int(re.search(r"constexpr int kStatusReplay = (\d+);", inc).group(1)) == 8
    others = [int(v) for v in re.findall(r"constexpr int kStatus\w+ = (\d+);", src + open(os.path.join(build.CSRC, "sg_gae.inc")).read())]
    assert 8 not in others
    assert re.search(r"constexpr uint32_t kStreamReplay = 3u;", inc)
    assert "kStreamReset = 0u, kStreamGoal = 1u, kStreamAction = 2u;" in open(os.path.join(build.CSRC, "sg_device.hpp")).read()
    for fn, n in (("void replay_commit_list_kernel(", 1), ("void replay_finish_kernel(", 2), ("void replay_sample_kernel(", 2)):
        assert len(re.findall(r"\*status = kStatusReplay;", engine_asm.function_body(inc, fn))) == n, fn
    for sig in ("static int status_error(sg_env *e, const char *who)", 'extern "C" int sg_check_status(sg_env *e)'):
        assert re.search(r"if \(st == kStatusReplay\)\s*return fail\(", engine_asm.function_body(src, sig)), sig
    lib = open(build.build(), "rb").read()
    assert b"sg_replay_*_device: a ring without a matching header" in lib
    assert b"an earlier sg_replay_*_device call refused its input on the device" in lib


def test_the_new_kernels_build_for_gfx950_without_scratch():
    """In the code object the replay kernels use no scratch and spill no vector register; only the dense commit kernel needs LDS
    (its per-workgroup reservation: 20 B); the samplers stay within 128 VGPRs (4 waves per SIMD) and contain no v_fma_f64 (every
    float64 operation of the return rounds on its own); every instruction that writes memory is a global_store_* of a byte, a
    dword or (the int64 index) two dwords -- nothing assumes more than the element's alignment -- except the one global atomic of
    the dense commit's reservation"""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    for name in (b"sg_replay_bytes", b"sg_replay_begin_device", b"sg_replay_commit_device", b"sg_replay_sample_device",
                 b"replay_sample_kernel", b"replay_commit_list_kernel", b"replay_commit_dense_kernel", b"replay_finish_kernel"):
        assert name in lib
    kernels = engine_asm.descriptors(r"\S*replay_\w+_kernel\S*")
    # begin, commit_list, dense_mark, commit_dense, finish, tick, sample<1 | 4 | 8 | 16>
    assert len(kernels) == 10, [k for k, _ in kernels]
    for name, field in kernels:
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == (20 if "commit_dense" in name else 0), name
        assert field["next_free_vgpr"] <= 128, name
    spills = engine_asm.spill_counts(r"\S*replay_\w+_kernel\S*")
    assert len(spills) == 10 and all(n == 0 for _, n in spills), spills
    for name, _ in kernels:
        fn = engine_asm.function(name)
        writes = set(re.findall(r"^\s+(\w*(?:store|atomic)\w*)\s", fn, flags=re.M))
        allowed = {"global_store_dword", "global_store_byte", "global_store_dwordx2"}
        if "commit_dense" in name:
            allowed |= {"global_atomic_add", "ds_write_b32", "ds_store_b32"}
        if "begin" in name or "finish" in name:  # the header's words, merged by the compiler (legal at 4-byte alignment)
            allowed |= {"global_store_dwordx3", "global_store_dwordx4"}
        assert writes and writes <= allowed, (name, sorted(writes))
        assert not re.search(r"\b(scratch_|buffer_store|flat_store)", fn), name
        if "sample" in name:
            assert not re.search(r"\bv_fma_f64\b", fn), name
