"""CPU tests of hindsight goal relabelling (sg_replay_relabel_device / replay_relabel_torch / replay_sample_her_torch): the
declarations and struct layouts, the NumPy model (tests/her_model.py) exhaustively on a tiny hand-made ring, the identity on a
rollout of the CPU oracle, the Python front end with the native call stubbed (nothing reaches a kernel), and the resources of the new
kernel in the gfx950 build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import engine_asm
import her_model as hm
import replay_model
from test_episode_stats import _fake_cuda, _stub_env
from test_gae import _struct_fields
from test_snapshot_device import _header_args

CONSTS = dict(goal_scale=500.0, sparse=5.0, goal_r2=0.1607142857142857 ** 2, two_over_world=np.float32(2.0 / 3.0), half_world=1.5)


# ---------------------------------------------------------------------------------------------- declarations
def test_entry_point_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_replay_relabel_device") == [
        "sg_env *env", "const sg_replay *ring", "const sg_replay_relabel_config *cfg", "int64_t n", "const sg_replay_batch *batch",
        "const sg_replay_relabel_out *out", "void *hip_stream"]
    assert _header_args("sg_replay_relabel_config_init", "void") == ["sg_replay_relabel_config *cfg"]
    vp = C.c_void_p
    S = _native.SYMBOLS
    assert S["sg_replay_relabel_device"] == (C.c_int, [vp, C.POINTER(_native.SgReplay), C.POINTER(_native.SgReplayRelabelConfig), C.c_int64,
                                                       C.POINTER(_native.SgReplayBatch), C.POINTER(_native.SgReplayRelabelOut), vp])
    assert S["sg_replay_relabel_config_init"] == (None, [C.POINTER(_native.SgReplayRelabelConfig)])
    assert "sg_replay_relabel" not in S  # no host-array form: the ring is device memory
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    for name, mirror, size in (("sg_replay_relabel_config", _native.SgReplayRelabelConfig, 32),
                               ("sg_replay_relabel_out", _native.SgReplayRelabelOut, 24)):
        decls = _struct_fields(name)
        assert len(decls) == len(mirror._fields_), name
        for d, (field, ct) in zip(decls, mirror._fields_):
            m = re.fullmatch(r"(.*?)(\w+)", d)
            kind, ident = m.group(1), m.group(2)
            assert ident == field, (name, d)
            assert ct is (C.c_void_p if "*" in kind else ctype[kind.split()[0]]), (name, d)
        assert C.sizeof(mirror) == size, name
    assert [(f, getattr(_native.SgReplayRelabelConfig, f).offset) for f, _ in _native.SgReplayRelabelConfig._fields_] == [
        ("struct_size", 0), ("seed", 8), ("her_ratio", 16), ("horizon", 24), ("strategy", 28)]
    assert [f for f, _ in _native.SgReplayRelabelOut._fields_] == ["relabelled", "offset", "goal"]


def test_the_kernel_file_is_listed_and_included_and_its_stream_tag_is_its_own():
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_her.inc" in build.HEADERS
    assert src.index('#include "sg_sequence.inc"') < src.index('#include "sg_her.inc"') < src.index('#include "sg_priority.inc"')
    inc = open(os.path.join(build.CSRC, "sg_her.inc")).read()
    # tag 12: written from kStreamSequence (8), as 9 .. 11 are, and pinned by a static_assert; no other tag has the value
    assert re.search(r"constexpr uint32_t kStreamHer = kStreamSequence \+ 4u;", inc) and hm.STREAM_HER == 12
    assert re.search(r"static_assert\(kStreamHer == 12u,", inc)
    taken = []
    for f in sorted(os.listdir(build.CSRC)):
        code = open(os.path.join(build.CSRC, f)).read()
        taken += [int(v) for _, v in re.findall(r"\bkStream(\w+) = (\d+)u", code)]
        taken += [8 + int(v) for _, v in re.findall(r"\bkStream(\w+) = kStreamSequence \+ (\d+)u", code)]
    assert sorted(taken) == list(range(13)), taken
    header = open(os.path.join(build.ROOT, "include", "spacegym.h")).read()
    assert "counter = (j lo, j hi, c, 12)" in header
    # one kernel, no replay_*_kernel (tests/test_replay.py counts those); it refuses through the ring's status code
    assert re.findall(r"void (\w+_kernel)\(", inc) == ["her_relabel_kernel"] and "template" not in inc
    assert len(re.findall(r"\*status = kStatusReplay;", engine_asm.function_body(inc, "void her_relabel_kernel("))) == 2
    body = engine_asm.function_body(src, 'extern "C" int sg_replay_relabel_device(')
    assert body.count("<<<") == 1 and "replay_tick_kernel" not in body  # one launch; the call counter is the sampler's to advance
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", body)


# ---------------------------------------------------------------------------------------------- the model on a hand-made ring
T, B, D, CAP = 8, 5, 15, 16
HEAD = 3  # a full ring whose oldest valid slot is 4: the valid slots, oldest first, are 4 5 6 7 0 1 2
DONE = {(7, 1): 0, (0, 1): 0, (2, 2): 0, (4, 3): 0, (6, 4): 1, (1, 4): 1, (5, 0): 0}  # (slot, env): truncated


def _tiny_ring():
    rng = np.random.default_rng(5)
    ring = replay_model.Ring(T, B, D, CAP)
    ring.obs[:] = rng.uniform(-1.5, 1.5, (T, B, D)).astype(np.float32)
    ring.action[:] = rng.uniform(-1, 1, (T, B, 2)).astype(np.float32)
    ring.reward[:] = rng.standard_normal((T, B)).astype(np.float32)
    ring.term_obs[:] = rng.uniform(-1.5, 1.5, (CAP, D)).astype(np.float32)
    ring.term_idx[:] = 0xdeadbeef  # never read where done is clear
    for seq, ((p, i), tr) in enumerate(DONE.items()):
        ring.done[p, i], ring.trunc[p, i], ring.term_idx[p, i] = 1, tr, seq + CAP  # (seq mod C is the record's place)
    ring.head, ring.filled, ring.sample_calls = HEAD, T, 3
    return ring


def _brute_window(ring, u, H):
    """m by walking: step k + 1 is reached while k + 1 <= H - 1, q + k + 1 < v and step k is not done"""
    v = ring.valid
    q, i = divmod(int(u), B)
    first = (ring.head - v) % T
    k = 0
    while k + 1 <= H - 1 and q + k + 1 < v and not ring.done[(first + q + k) % T, i]:
        k += 1
    return k


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("strategy", [hm.FUTURE, hm.FINAL])
def test_windows_and_offsets_of_every_transition_and_every_horizon(strategy):
    """T = 8, B = 5, wrapped, hand-placed done / trunc: for every u, every H in 1 .. 7 and both strategies no window crosses a done
    or the newest edge, `final` is the window's last step, her_ratio 0 leaves the batch as it was bit for bit and her_ratio 1
    relabels every row, with the position of s' of (p_k*, i) -- the terminal record where that step is done"""
    ring = _tiny_ring()
    v = ring.valid
    assert v == T - 1 and (ring.head - v) % T == 4
    every = np.arange(v * B, dtype=np.int64)
    batch, ok = replay_model.sample(ring, every.size, index=every, advance=False)
    assert ok.all() and (batch["steps"] == 1).all()
    first = (ring.head - v) % T
    seen_m = set()
    for H in range(1, T):
        same, rel0, off0, goal0, ok0 = hm.relabel(ring, batch, CONSTS, her_ratio=0.0, horizon=H, strategy=strategy, seed=11)
        assert ok0.all() and not rel0.any() and not off0.any() and not goal0.any()
        assert all(_same(same[k], batch[k]) for k in batch)
        out, rel, off, goal, ok1 = hm.relabel(ring, batch, CONSTS, her_ratio=1.0, horizon=H, strategy=strategy, seed=11)
        assert ok1.all() and (rel == 1).all() and ring.sample_calls == 3 and not ring.status
        for u in every:
            q, i = divmod(int(u), B)
            m, ks = _brute_window(ring, u, H), int(off[u])
            seen_m.add(m)
            assert 0 <= ks <= m <= H - 1 and q + m < v, (u, H)
            assert not ring.done[(first + q + np.arange(ks)) % T, i].any(), (u, H)  # no step before k* ends an episode
            assert int(hm.window(ring, [u], H)[0]) == m
            if strategy == hm.FINAL:
                assert ks == m
            p = (first + q + ks) % T
            want = ring.term_obs[int(ring.term_idx[p, i]) % CAP, :2] if ring.done[p, i] else ring.obs[p, i, :2]
            assert _same(goal[u], want), (u, H)
        for k in ("action", "terminated", "truncated", "discount", "steps", "index"):
            assert _same(out[k], batch[k]), k
        assert _same(out["obs"][:, :-2], batch["obs"][:, :-2]) and _same(out["next_obs"][:, :-2], batch["next_obs"][:, :-2])
        assert _same(out["obs"][:, -2:], (goal - batch["obs"][:, :2]) * CONSTS["two_over_world"])
        assert _same(out["next_obs"][:, -2:], (goal - batch["next_obs"][:, :2]) * CONSTS["two_over_world"])
    assert seen_m == set(range(T - 1))  # every window length 0 .. 6 occurred: done at the first step, mid-window, the edge, none


def test_rows_that_are_not_single_steps_or_name_no_transition_are_left_alone():
    ring = _tiny_ring()
    cells = ring.valid * B
    index = np.array([0, -1, cells, cells - 1, 7, 2 ** 40], np.int64)
    batch, ok = replay_model.sample(ring, 6, index=np.where((index >= 0) & (index < cells), index, 0), advance=False)
    batch["index"] = index
    batch["steps"] = np.array([1, 1, 1, 1, 3, 1], np.uint8)
    out, rel, off, goal, ok = hm.relabel(ring, batch, CONSTS, her_ratio=1.0, horizon=4)
    assert ok.tolist() == [True, False, False, True, True, False] and ring.status
    assert rel.tolist() == [1, 0, 0, 1, 2, 0]
    for j in (1, 2, 4, 5):
        assert all(_same(out[k][j], batch[k][j]) for k in batch) and off[j] == 0 and not goal[j].any()
    assert not _same(out["obs"][0], batch["obs"][0]) and off[3] == 0  # the newest transition has no future but its own end


def test_future_offsets_are_uniform_on_the_window():
    """2^16 rows of one transition whose window is 0 .. m: every value's count within 4 standard deviations of n / (m + 1)"""
    ring = _tiny_ring()
    n = 2 ** 16
    for u, H, m in ((2, 7, 6), (2, 4, 3), (4, 7, 2)):  # env 2 from the oldest slot: done only at the newest; env 4: done at its third step
        assert _brute_window(ring, u, H) == m
        index = np.full(n, u, np.int64)
        batch, _ = replay_model.sample(ring, n, index=index, advance=False)
        _, rel, off, _, _ = hm.relabel(ring, batch, CONSTS, her_ratio=1.0, horizon=H, seed=2024)
        hist = np.bincount(off, minlength=m + 1)
        p = 1.0 / (m + 1)
        assert hist.size == m + 1 and np.abs(hist - n * p).max() <= 4.0 * np.sqrt(n * p * (1 - p)), hist
        # the share relabelled follows her_ratio (the third word decides, so it does not depend on the offset)
        _, rel, _, _, _ = hm.relabel(ring, batch, CONSTS, her_ratio=0.3, horizon=H, seed=2024)
        assert abs((rel == 1).mean() - 0.3) <= 4.0 * np.sqrt(0.3 * 0.7 / n)
    assert hm.threshold(0.0) == 0 and hm.threshold(1.0) == 2 ** 32 and hm.threshold(0.8) == 3435973837
    a, b = hm.words(7, 2, 50), hm.words(7, 3, 50)
    assert not np.array_equal(a[0], b[0])  # the call number is part of the counter


def test_rows_relabelled_with_their_own_end_position_sit_on_the_goal():
    """k* = 0 (horizon 1): the goal columns of next_obs are exactly +0 and the new goal term is goal_scale |x1 - x0| + sparse"""
    ring = _tiny_ring()
    every = np.arange(ring.valid * B, dtype=np.int64)
    batch, _ = replay_model.sample(ring, every.size, index=every, advance=False)
    out, rel, off, goal, _ = hm.relabel(ring, batch, CONSTS, her_ratio=1.0, horizon=1)
    assert (rel == 1).all() and not off.any() and _same(goal, batch["next_obs"][:, :2])
    assert not _bits(out["next_obs"][:, -2:]).any()  # +0.0, bit for bit
    x0, x1 = batch["obs"][:, :2].astype(np.float64), batch["next_obs"][:, :2].astype(np.float64)
    vo1 = batch["next_obs"][:, -2:].astype(np.float64) * 1.5
    vo0 = vo1 + (x1 - x0)
    t_old = 500.0 * (np.linalg.norm(vo0, axis=1) - np.linalg.norm(vo1, axis=1)) + np.where((vo1 ** 2).sum(1) < CONSTS["goal_r2"], 5.0, 0.0)
    want = batch["reward"].astype(np.float64) - t_old + 500.0 * np.linalg.norm(x1 - x0, axis=1) + 5.0
    assert np.abs(out["reward"] - want).max() <= 2.0 ** -23 * np.abs(want).max() + 1e-9  # (float32 rounding of the result)


# ---------------------------------------------------------------------------------------------- the identity on an oracle rollout
IDENTITY_MEASURED = 1.049041748046875e-05  # max |reward' - reward| on the rollout below (also in DESIGN section 34, profiles/her_cost.txt)


def test_relabelling_with_the_transitions_own_goal_reproduces_the_stored_reward():
    """400 consecutive steps of 64 Goal 3P envs of the CPU oracle under random actions, as float32 (obs, reward, next_obs) rows, s' of
    a finished step being its terminal observation: relabelled with the goal the step was taken under, the reward comes back to
    within 4x the measured 1.05e-5 (goal_scale x a few ulp of a position: the old term is re-formed from rounded positions).  The
    rows include goal hits and the steps right after one, whose obs still names the goal that was hit."""
    from oracle.pyoracle import Oracle
    o = Oracle("GoalContinuous3P-v0")
    Bn, K = 64, 400
    envs, obs = o.vec_reset(Bn, seed=7)
    rng = np.random.default_rng(1)
    rows = dict(obs=[], next_obs=[], reward=[], goal=[], done=[])
    for _ in range(K):
        a = rng.uniform(-1, 1, (Bn, 2)).astype(np.float32)
        rows["goal"].append(envs["goal_xy"].copy())
        nxt, r, d, _, tobs = o.vec_step(envs, a, seed=7, want_terminal_obs=True)
        rows["obs"].append(obs); rows["next_obs"].append(np.where(d[:, None] != 0, tobs, nxt)); rows["reward"].append(r); rows["done"].append(d)
        obs = nxt
    p = o.params
    goal64, next64, done = np.array(rows["goal"]), np.array(rows["next_obs"]), np.array(rows["done"])
    dist = np.linalg.norm(goal64 - next64[..., :2], axis=-1)
    hit = dist < p.goal_radius
    after_hit = np.zeros_like(hit)
    after_hit[1:] = hit[:-1] & (done[:-1] == 0)
    near = (np.abs(dist - p.goal_radius) < 1e-6).reshape(-1)
    assert near.mean() <= 0.01 and (hit.reshape(-1) & ~near).sum() >= 1 and (after_hit.reshape(-1) & ~near).sum() >= 1
    f32 = lambda x: np.array(x).reshape(Bn * K, -1).astype(np.float32)  # noqa: E731
    reward = np.array(rows["reward"]).reshape(-1).astype(np.float32)
    consts = dict(goal_scale=p.goal_vel_reward_scale * p.distance_fctr, sparse=p.goal_sparse_reward, goal_r2=p.goal_radius ** 2,
                  two_over_world=np.float32(2.0 / p.world_size), half_world=np.float32(p.world_size / 2))
    assert consts["goal_scale"] == CONSTS["goal_scale"] and consts["goal_r2"] == CONSTS["goal_r2"] and consts["half_world"] == 1.5
    o2, n2, r2 = hm.relabel_rows(f32(rows["obs"]), f32(rows["next_obs"]), reward, f32(rows["goal"]), consts["goal_scale"], consts["sparse"],
                                 consts["goal_r2"], consts["two_over_world"], consts["half_world"])
    err = np.abs(r2.astype(np.float64) - reward.astype(np.float64))[~near]
    print("identity: max |reward' - reward| = %.6g over %d rows (%d goal hits, %d rows after a hit)"
          % (err.max(), err.size, hit.sum(), after_hit.sum()))
    assert err.max() <= 4.0 * IDENTITY_MEASURED
    # the goal columns come back too: (goal - x) * two_over_world from the float32 goal, within an ulp of the stored columns
    assert np.abs(n2[:, -2:] - f32(rows["next_obs"])[:, -2:]).max() <= 2.0 ** -22


# ---------------------------------------------------------------------------------------------- the front end, stubbed
def _env(discrete=False, auto_reset=1, family="goal"):
    from space_gym_amd import _native
    env = _stub_env(B=B, D=D)
    env.discrete = discrete
    env.env_id = "GoalContinuous3P-v0" if family == "goal" else "KeplerCircleOrbit-v0"
    env.spec = dict(family=family)
    env._cfg = _native.SgConfig(auto_reset=auto_reset)
    return env


def _ring(env, steps=T, cap=5, filled=8):
    import torch
    from space_gym_amd.vector_env import ReplayRing
    z = lambda shape, dtype: _fake_cuda(torch.zeros(shape, dtype=dtype))  # noqa: E731
    ring = ReplayRing(steps=steps, num_envs=B, obs_dim=D, term_capacity=cap, discrete=env.discrete, obs=z((steps, B, D), torch.float32),
                      action=z((steps, B), torch.int32) if env.discrete else z((steps, B, 2), torch.float32),
                      reward=z((steps, B), torch.float32), done=z((steps, B), torch.uint8), trunc=z((steps, B), torch.uint8),
                      term_idx=z((steps, B), torch.int32), term_obs=z((cap, D), torch.float32), slot_seq=z((steps,), torch.int32),
                      hdr=z((8,), torch.int32))
    ring.head, ring.filled = filled % steps, filled
    return ring


def _batch(n, **over):
    import torch
    b = dict(obs=torch.zeros((n, D)), action=torch.zeros((n, 2)), reward=torch.zeros(n), next_obs=torch.zeros((n, D)),
             terminated=torch.zeros(n, dtype=torch.uint8), truncated=torch.zeros(n, dtype=torch.uint8), discount=torch.zeros(n),
             steps=torch.zeros(n, dtype=torch.uint8), index=torch.zeros(n, dtype=torch.int64))
    b.update(over)
    return {k: _fake_cuda(v) for k, v in b.items() if v is not None}


def test_the_call_reaches_the_native_entry_point_with_the_header_structs():
    import torch
    env = _env()
    ring = _ring(env)
    batch = _batch(6)
    out = {k: _fake_cuda(v) for k, v in dict(relabelled=torch.zeros(6, dtype=torch.uint8), goal=torch.zeros((6, 2))).items()}
    got = env.replay_relabel_torch(ring, batch, her_ratio=0.25, horizon=5, strategy="final", seed=2 ** 63 + 5, out=out)
    assert got is batch and got["relabelled"] is out["relabelled"] and got["goal"] is out["goal"] and "offset" not in got
    assert env._lib.names() == ["sg_replay_relabel_device"]
    a = env._lib.calls[0][1]
    assert len(a) == 7 and a[3] == 6
    r, cfg, b, o = a[1]._obj, a[2]._obj, a[4]._obj, a[5]._obj
    assert (r.struct_size, r.steps, r.term_capacity) == (88, T, 5) and r.hdr == ring.hdr.data_ptr()
    assert (cfg.struct_size, cfg.seed, cfg.her_ratio, cfg.horizon, cfg.strategy) == (32, 2 ** 63 + 5, 0.25, 5, 1)
    for k in ("obs", "next_obs", "reward", "steps", "index"):
        assert getattr(b, k) == batch[k].data_ptr(), k
    assert (o.relabelled, o.offset, o.goal) == (out["relabelled"].data_ptr(), None, out["goal"].data_ptr())
    # the defaults: ratio 0.8, the whole ring as horizon, future, seed 0
    env = _env(discrete=True)
    ring = _ring(env)
    assert env.HER_STRATEGIES == {"future": 0, "final": 1}
    full = dict(relabelled=torch.zeros(4, dtype=torch.uint8), offset=torch.zeros(4, dtype=torch.int32), goal=torch.zeros((4, 2)))
    got = env.replay_relabel_torch(ring, _batch(4, action=None), out={k: _fake_cuda(v) for k, v in full.items()})
    cfg = env._lib.calls[-1][1][2]._obj
    assert (cfg.seed, cfg.her_ratio, cfg.horizon, cfg.strategy) == (0, 0.8, T - 1, 0)
    assert got["offset"].dtype == torch.int32 and env._lib.names() == ["sg_replay_relabel_device"]


def test_the_her_sampler_is_the_sampler_followed_by_the_relabel():
    import torch
    from space_gym_amd.vector_env import ReplayPriority, SpaceGymVectorEnv
    assert "ADDS NO NATIVE CODE" in SpaceGymVectorEnv.replay_sample_her_torch.__doc__
    env = _env()
    ring = _ring(env)
    extra = dict(relabelled=torch.zeros(4, dtype=torch.uint8), offset=torch.zeros(4, dtype=torch.int32), goal=torch.zeros((4, 2)))
    out = {**_batch(4), **{k: _fake_cuda(v) for k, v in extra.items()}}
    assert env.replay_sample_her_torch(ring, 4, her_ratio=0.5, horizon=3, strategy="final", seed=9, gamma=0.9, out=out) is out
    assert env._lib.names() == ["sg_replay_sample_device", "sg_replay_relabel_device"]
    scfg, rcfg = env._lib.calls[0][1][2]._obj, env._lib.calls[1][1][2]._obj
    assert (scfg.seed, scfg.n_step, scfg.gamma) == (9, 1, 0.9) and (rcfg.seed, rcfg.her_ratio, rcfg.horizon, rcfg.strategy) == (9, 0.5, 3, 1)
    assert env._lib.calls[0][1][5]._obj.obs == env._lib.calls[1][1][4]._obj.obs == out["obs"].data_ptr()
    # prioritized: the draw, the gather, the relabel; weight and cell are the draw's
    env = _env()
    prio = ReplayPriority(T, B, 16, leaf=_fake_cuda(torch.zeros((T, B), dtype=torch.int32)), node=_fake_cuda(torch.zeros(64, dtype=torch.int64)),
                          hdr=_fake_cuda(torch.zeros(16, dtype=torch.int32)))
    out = {**_batch(4), **{k: _fake_cuda(v) for k, v in extra.items()}, "cell": _fake_cuda(torch.zeros(4, dtype=torch.int64)),
           "weight": _fake_cuda(torch.ones(4))}
    assert env.replay_sample_her_torch(ring, 4, prio=prio, beta=0.5, out=out) is out
    assert env._lib.names() == ["sg_priority_sample_device", "sg_replay_sample_device", "sg_replay_relabel_device"]
    assert env._lib.calls[0][1][5]._obj.weight == out["weight"].data_ptr()


def _refusals():
    import torch
    z = torch.zeros

    def rel(batch=None, **kw):
        return lambda env, ring: env.replay_relabel_torch(ring, _batch(4) if batch is None else batch, **kw)
    return {
        "ratio negative": ("^her_ratio", rel(her_ratio=-0.1)), "ratio large": ("^her_ratio", rel(her_ratio=1.5)),
        "ratio nan": ("^her_ratio", rel(her_ratio=float("nan"))),
        "horizon zero": ("^horizon: 1 .. 7 expected", rel(horizon=0)), "horizon the slots": ("^horizon: 1 .. 7 expected", rel(horizon=T)),
        "strategy": ("^strategy", rel(strategy="episode")), "strategy code": ("^strategy", rel(strategy=0)),
        "seed negative": ("^seed:", rel(seed=-1)), "seed large": ("^seed:", rel(seed=2 ** 64)),
        "no steps": ("^batch: a dict", rel(_batch(4, steps=None))), "no index": ("^batch: a dict", rel(_batch(4, index=None))),
        "not a dict": ("^batch: a dict", rel([1, 2])),
        "index dtype": (r"^batch\['index'\]", rel(_batch(4, index=z(4, dtype=torch.int32)))),
        "index shape": (r"^batch\['index'\]", rel(_batch(4, index=z((4, 1), dtype=torch.int64)))),
        "steps dtype": (r"^batch\['steps'\]", rel(_batch(4, steps=z(4, dtype=torch.int32)))),
        "obs shape": (r"^batch\['obs'\]", rel(_batch(4, obs=z((4, D + 1))))),
        "next_obs rows": (r"^batch\['next_obs'\]", rel(_batch(4, next_obs=z((5, D))))),
        "reward host": (r"^batch\['reward'\]", lambda env, ring: env.replay_relabel_torch(ring, {**_batch(4), "reward": z(4)})),
        "out relabelled": (r"^out\['relabelled'\]", rel(out=dict(relabelled=_fake_cuda(z(4, dtype=torch.int32))))),
        "out offset": (r"^out\['offset'\]", rel(out=dict(offset=_fake_cuda(z(4, dtype=torch.uint8))))),
        "out goal": (r"^out\['goal'\]", rel(out=dict(goal=_fake_cuda(z((4, 3)))))),
        "ring": ("expected the object", lambda env, ring: env.replay_relabel_torch(dict(obs=ring.obs), _batch(4))),
    }


@pytest.mark.parametrize("bad", sorted(_refusals()))
def test_host_refusals_raise_before_the_native_call(bad):
    env = _env()
    ring = _ring(env)
    match, call = _refusals()[bad]
    with pytest.raises(ValueError, match=match):
        call(env, ring)
    assert env._lib.calls == [] and (ring.head, ring.filled) == (0, 8)


def test_a_kepler_id_auto_reset_off_and_the_multi_device_front_ends_are_refused():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    kepler = _env(family="kepler")
    with pytest.raises(ValueError, match="has no goal to relabel"):
        kepler.replay_relabel_torch(_ring(kepler), _batch(4))
    with pytest.raises(ValueError, match="has no goal to relabel"):
        kepler.replay_sample_her_torch(_ring(kepler), 4)
    off = _env(auto_reset=0)
    with pytest.raises(ValueError, match="auto_reset"):
        off.replay_relabel_torch(_ring(off), _batch(4))
    with pytest.raises(ValueError, match="^horizon"):
        _env().replay_sample_her_torch(_ring(_env()), 4, horizon=T)
    assert off._lib.calls == [] and kepler._lib.calls == []  # (the composition refuses before its sampler runs)
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("replay_relabel_torch", "replay_sample_her_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))


# ---------------------------------------------------------------------------------------------- the build
def test_the_kernel_builds_for_gfx950_without_scratch_lds_or_spills():
    """from the compiler's report: no scratch, no LDS, no spilled register, at most 64 VGPRs (8 waves per SIMD)"""
    kernels = engine_asm.descriptors(r"\S*her_\w+_kernel\S*")
    assert len(kernels) == 1, [k for k, _ in kernels]
    for name, field in kernels:
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == 0, name
        assert field["next_free_vgpr"] <= 64, (name, field["next_free_vgpr"])
    for kind in ("vgpr", "sgpr"):
        spills = engine_asm.spill_counts(r"\S*her_\w+_kernel\S*", kind)
        assert len(spills) == 1 and all(n == 0 for _, n in spills), (kind, spills)
    fn = engine_asm.function(kernels[0][0])
    assert not re.search(r"\bds_(read|write|bpermute)|\bglobal_atomic|\bscratch_", fn)
