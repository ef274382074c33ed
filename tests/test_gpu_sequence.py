"""GPU tests of the sequence sampler of the replay ring (replay_sample_sequences_torch / sg_replay_sequence_device) against the NumPy
model tests/sequence_model.py.  "Equal" is bitwise: the same bit patterns in every output.  Outputs are prefilled (NaN in the float
tensors, 77 elsewhere) so that what the call must leave alone is seen to be left alone."""
import ctypes as C

import numpy as np
import pytest

import replay_model
from returns_model import vtrace_model
from sequence_model import sample_sequences, starts, synthetic
from test_gpu_replay import _apply, _bits, _dev, _expect_refusal, _header, _same, make

pytestmark = pytest.mark.gpu

KEYS = ("obs", "action", "reward", "done", "trunc", "terminal_obs", "index")
P_DONE = 0.15


def _filled(env_id, T, B, laps, dense, seed=3, upto=None):
    """an env of B envs, the model ring of tests/replay_model.synthetic and the device ring after the same commits (the first `upto`)"""
    import torch
    env = make(B, env_id)
    # (C = T B: at this finish rate the default terminal capacity would be too small for the live window)
    model, commits, extra = synthetic(T, B, env.obs_dim, laps=laps, K=None if dense else 4, p_done=P_DONE, seed=seed, discrete=env.discrete,
                                      dense=dense, C=T * B)
    assert not model.status
    ring = env.replay_torch(T, term_capacity=T * B)
    env.replay_begin_torch(ring, _dev(extra["obs0"]))
    for com in commits[:upto]:
        _apply(env, ring, com)
    torch.cuda.synchronize()
    env.check_status()
    return env, ring, model, commits, extra


def _prefilled(env, n, L, n_cols=0):
    import torch
    D = env.obs_dim
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")  # noqa: E731
    b77 = lambda *shape: torch.full(shape, 77, dtype=torch.uint8, device="cuda")  # noqa: E731
    out = dict(obs=nan(L + 1, n, D), action=torch.full((L, n), 77, dtype=torch.int32, device="cuda") if env.discrete else nan(L, n, 2),
               reward=nan(L, n), done=b77(L, n), trunc=b77(L, n), terminal_obs=nan(L, n, D),
               index=torch.full((n,), 77, dtype=torch.int64, device="cuda"))
    if n_cols:
        out["columns"] = [nan(L, n) for _ in range(n_cols)]
    return out


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: [c.cpu().numpy() for c in v] if k == "columns" else v.cpu().numpy() for k, v in out.items()}


def _assert_sequences(got, before, want, ok, written, what):
    """columns with ok: the model's bits (terminal_obs where written only); everything else: the prefill's bits"""
    for k in KEYS + ("columns",):
        if k not in got:
            continue
        pairs = zip(got[k], before[k], want[k]) if k == "columns" else [(got[k], before[k], want[k])]
        for g, b, w in pairs:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
            if k == "index":
                keep = ~ok
            elif k == "terminal_obs":
                keep = ~written
            else:
                keep = np.broadcast_to(~ok, g.shape[:2])
            bad = int((_bits(g[~keep]) != _bits(w[~keep])).sum())
            assert bad == 0, (what, k, bad)
            assert np.array_equal(_bits(g[keep]), _bits(b[keep])), (what, k, "touched")


RINGS = {"wrapped": (16, 8, 2.5, False), "not full": (16, 8, 0.5, False), "dense": (12, 5, 2.5, True)}


@pytest.mark.parametrize("kind", sorted(RINGS))
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "GoalContinuous4P-v0", "KeplerCircleOrbit-v0", "GoalDiscrete3-v0"])
def test_sequences_equal_the_model_bit_for_bit(env_id, kind):
    """1: L = 1, 5 and v; n = 1, 67 (a partial wave and a partial group of four rows) and 1 000; two extra columns of random floats;
    terminal_obs rows without a done keep their NaN bits"""
    T, B, laps, dense = RINGS[kind]
    env, ring, model, _, _ = _filled(env_id, T, B, laps, dense)
    assert env.obs_dim == {"GoalContinuous3P-v0": 15, "GoalContinuous4P-v0": 17, "KeplerCircleOrbit-v0": 10, "GoalDiscrete3-v0": 15}[env_id]
    v = model.valid
    assert v == (8 if kind == "not full" else T - 1) and len(ring) == v * B
    rng = np.random.default_rng(17)
    cols = [rng.standard_normal((T, B)).astype(np.float32) for _ in range(2)]
    cols_dev = [_dev(c) for c in cols]
    calls = 0
    for L in (1, 5, v):
        for n in (1, 67, 1000):
            out = _prefilled(env, n, L, 2)
            before = _host(out)
            assert env.replay_sample_sequences_torch(ring, n, L, seed=2 ** 40 + 9, columns=cols_dev, out=out) is out
            want, ok, written = sample_sequences(model, n, L, seed=2 ** 40 + 9, columns=cols)
            calls += 1
            assert ok.all()
            if L > 1 and n > 1:
                assert written.any() and not written.all()
            _assert_sequences(_host(out), before, want, ok, written, (L, n))
    assert _header(ring)["sample_calls"] == calls == model.sample_calls
    # the allocating form: terminal_obs starts as zeros, no columns asked for
    got = _host(env.replay_sample_sequences_torch(ring, 67, min(5, v), seed=1))
    want, ok, written = sample_sequences(model, 67, min(5, v), seed=1)
    assert set(got) == set(KEYS) and all(_same(got[k], want[k]) for k in KEYS)
    env.check_status()
    env.close()


@pytest.mark.parametrize("env_id", ["GoalContinuous4P-v0", "GoalDiscrete3-v0"])
def test_every_row_is_the_single_transition_sampler_s_and_the_window_comes_back_in_age_order(env_id):
    """2: device against device"""
    import torch
    T, B = 16, 8
    env, ring, model, _, extra = _filled(env_id, T, B, 2.5, False)
    v, L, n = T - 1, 5, 67
    seq = env.replay_sample_sequences_torch(ring, n, L, seed=4)
    for k in range(L):
        one = env.replay_sample_torch(ring, n, n_step=1, index=seq["index"] + k * B)
        fin = seq["done"][k] != 0
        nxt = torch.where(fin[:, None], seq["terminal_obs"][k], seq["obs"][k + 1])
        for a, b in ((one["obs"], seq["obs"][k]), (one["action"], seq["action"][k]), (one["reward"], seq["reward"][k]), (one["next_obs"], nxt),
                     (one["terminated"], (fin & (seq["trunc"][k] == 0)).to(torch.uint8)), (one["truncated"], seq["trunc"][k])):
            assert _same(a.cpu().numpy(), b.cpu().numpy()), k
    # index = arange(B), L = v: the valid window, oldest slot first
    got = _host(env.replay_sample_sequences_torch(ring, B, v, index=torch.arange(B, dtype=torch.int64, device="cuda")))
    order = (ring.head - v + np.arange(v)) % T
    full = {k: getattr(ring, k).cpu().numpy() for k in ("obs", "action", "reward", "done", "trunc")}
    assert _same(got["obs"][1:], full["obs"][order]) and _same(got["obs"][0], full["obs"][(order[0] - 1) % T])
    for k in ("action", "reward", "done", "trunc"):
        assert _same(got[k], full[k][order]), k
    fin = got["done"] != 0
    assert fin.any() and _same(got["terminal_obs"][fin], extra["term_dense"][order][fin]) and not got["terminal_obs"][~fin].any()
    assert got["index"].tolist() == list(range(B))
    env.check_status()
    env.close()


def test_an_index_outside_the_starts_leaves_its_column_untouched():
    """3"""
    env, ring, model, _, _ = _filled("GoalContinuous3P-v0", 16, 8, 2.5, False)
    L = 5
    S = starts(model, L)
    assert S == (15 - L + 1) * 8
    index = np.array([0, -1, S, S - 1, 2 ** 40, 17, -2 ** 63, S - 8], np.int64)
    rng = np.random.default_rng(5)
    cols = [rng.standard_normal((16, 8)).astype(np.float32)]
    out = _prefilled(env, index.size, L, 1)
    before = _host(out)
    env.replay_sample_sequences_torch(ring, index.size, L, index=_dev(index), columns=[_dev(cols[0])], out=out)
    want, ok, written = sample_sequences(model, index.size, L, index=index, columns=cols)
    assert ok.tolist() == [True, False, False, True, False, True, False, True] and model.status
    _expect_refusal(env, ring)  # reported once, then cleared
    _assert_sequences(_host(out), before, want, ok, written, "index")
    assert _header(ring)["sample_calls"] == 1
    env.close()


def _native_call(env, ring, n, L, out, index=None, n_extra=0, extras=(), struct_size=None, cfg=True, seqs=True, drop=()):
    """sg_replay_sequence_device as a C caller reaches it: no Python check in front"""
    from space_gym_amd import _native
    r = env._replay_arg(ring)
    c = _native.SgReplaySequenceConfig(C.sizeof(_native.SgReplaySequenceConfig) if struct_size is None else struct_size, 0, L, n_extra)
    s = _native.SgReplaySequences(*(out[k].data_ptr() if k not in drop else None for k in KEYS))
    for e, (src, dst) in enumerate(extras):
        s.extra_in[e], s.extra_out[e] = src, dst
    return r, lambda: env._lib.sg_replay_sequence_device(env._h, C.byref(r), C.byref(c) if cfg else None, n,
                                                         C.c_void_p(index.data_ptr()) if index is not None else None,
                                                         C.byref(s) if seqs else None, env._stream())


def test_a_ring_that_holds_fewer_steps_than_asked_for_writes_nothing():
    """4: v = 8 < L = 9, through the native call (the Python form refuses first)"""
    env, ring, model, _, _ = _filled("KeplerCircleOrbit-v0", 16, 8, 0.5, False)
    with pytest.raises(ValueError, match="the ring holds 8 steps"):
        env.replay_sample_sequences_torch(ring, 67, 9)
    out = _prefilled(env, 67, 9)
    before = _host(out)
    _, call = _native_call(env, ring, 67, 9, out)
    assert call() == 0
    assert sample_sequences(model, 67, 9) == (None, None, None) and model.status
    _expect_refusal(env, ring)
    got = _host(out)
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(before[k])), k
    assert _header(ring)["sample_calls"] == 1 == model.sample_calls  # (the tick is a launch of its own)
    env.close()


def test_a_captured_call_draws_afresh_and_sees_the_ring_grow():
    """5: a captured graph replayed twice equals the model's calls c and c + 1; a commit between two replays on a ring that is not
    full lets the next draw range over the larger S"""
    import torch
    T, B, L, n = 16, 8, 3, 1000
    env, ring, model, commits, _ = _filled("GoalContinuous3P-v0", T, B, 0.75, False, upto=2)
    full_model = model  # (synthetic ran all three commits: rebuild the model ring as it is after two)
    model = replay_model.Ring(T, B, env.obs_dim, T * B)
    model.begin(full_model.obs[T - 1])
    for com in commits[:2]:
        model.write_rows(com["first"], com["rows"])
        model.commit_list(com["first"], com["K"], com["count"], com["step_env"], com["tobs"], com["capacity"])
    assert model.valid == 8 and ring.filled == 8
    kw = dict(seed=7)
    out = _prefilled(env, n, L)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.replay_sample_sequences_torch(ring, n, L, out=out, **kw)  # (call 0, warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    sample_sequences(model, n, L, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.replay_sample_sequences_torch(ring, n, L, out=out, **kw)
    assert _header(ring)["sample_calls"] == 1 == model.sample_calls  # (capturing ran nothing)
    seen = []
    for rep in range(2):
        graph.replay()
        want, ok, _ = sample_sequences(model, n, L, **kw)
        got = _host(out)
        assert ok.all() and all(_same(got[k], want[k]) for k in KEYS if k != "terminal_obs"), rep
        seen.append(got["index"].copy())
    assert not np.array_equal(seen[0], seen[1]) and max(s.max() for s in seen) < starts(model, L) == 6 * B
    _apply(env, ring, commits[2])
    com = commits[2]
    model.write_rows(com["first"], com["rows"])
    model.commit_list(com["first"], com["K"], com["count"], com["step_env"], com["tobs"], com["capacity"])
    graph.replay()
    want, ok, written = sample_sequences(model, n, L, **kw)
    got = _host(out)
    assert all(_same(got[k], want[k]) for k in KEYS if k != "terminal_obs") and _same(got["terminal_obs"][written], want["terminal_obs"][written])
    assert starts(model, L) == 10 * B and got["index"].max() >= 6 * B  # the draw ranges over the larger S
    assert _header(ring)["sample_calls"] == 4 == model.sample_calls
    env.check_status()
    env.close()


def test_sampled_sequences_feed_vtrace_end_to_end():
    """6: three closed-loop rollouts of K = 4 into ring.rows(4) with logp / value as slices of two [T, B] column tensors, each
    committed; 64 sequences of L = 6 with both columns; the current policy's logp and values of the sampled rows; V-trace.  The targets
    equal tests/returns_model.py on the model's sequences bit for bit, and the sampled reward / done rows are the rollouts' own"""
    import torch
    from policy_model import random_policy
    from test_gpu_policy import _handle
    B, T, K, L, n = 64, 16, 4, 6, 64
    env = make(B, "GoalContinuous3P-v0", seed=5, max_episode_steps=5)
    D = env.obs_dim
    behaviour = _handle(env, random_policy(np.random.default_rng(1), D, 32, 2, 2))
    current = _handle(env, random_policy(np.random.default_rng(2), D, 32, 2, 2))
    ring = env.replay_torch(T, term_capacity=T * B)
    logp_col, value_col = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    env.replay_begin_torch(ring, env.reset_torch())
    term = env.terminal_list_torch(K * B)
    hist = dict(reward=[], done=[])
    for c in range(3):
        p = ring.head
        rows = ring.rows(K)
        if p == 0:  # the first action's observation is the ring's last slot, not adjacent to slot 0
            obs = torch.empty((K + 1, B, D), device="cuda")
            obs[0].copy_(ring.obs[T - 1])
        else:
            obs = ring.obs[p - 1:p + K]
        env.rollout_policy_torch(behaviour, obs, rows["action"], logp_col[p:p + K], value_col[p:p + K + 1], rows["reward"], rows["done"],
                                 rows["trunc"], seed=3, first_step=c * K, terminal=term)
        if p == 0:
            rows["obs"].copy_(obs[1:])
        env.replay_commit_torch(ring, K, terminal=term)
        hist["reward"].append(rows["reward"].cpu().numpy().copy())
        hist["done"].append(rows["done"].cpu().numpy().copy())
    env.check_status()
    seq = env.replay_sample_sequences_torch(ring, n, L, seed=11, columns=[logp_col, value_col])
    ev = lambda o, a: env.policy_evaluate_raw_torch(current, o.reshape(-1, D).contiguous(), a.reshape(-1, 2).contiguous())  # noqa: E731
    logp_new, _, value = ev(seq["obs"][:-1], seq["action"])
    _, _, terminal_value = ev(seq["terminal_obs"], seq["action"])
    _, _, last_value = ev(seq["obs"][-1], seq["action"][0])
    ratio = torch.exp(logp_new.reshape(L, n) - seq["columns"][0])
    vs, pg = env.vtrace_torch(seq["reward"], seq["done"], seq["trunc"], value.reshape(L, n), last_value=last_value, ratio=ratio,
                              terminal_value=terminal_value.reshape(L, n), gamma=0.97, lam=0.9)
    env.check_status()
    # the model ring is the device ring's members; the model's sequences are then the device's, bit for bit
    hdr = _header(ring)
    model = replay_model.Ring(T, B, D, T * B)
    for k in ("obs", "action", "reward", "done", "trunc", "term_obs"):
        setattr(model, k, getattr(ring, k).cpu().numpy())
    model.term_idx = ring.term_idx.cpu().numpy().view(np.uint32)
    model.head, model.filled, model.sample_calls = hdr["head"], hdr["filled"], 0
    assert (model.head, model.filled, hdr["sample_calls"]) == (12, 12, 1)
    cols = [logp_col.cpu().numpy(), value_col.cpu().numpy()]
    want, ok, written = sample_sequences(model, n, L, seed=11, columns=cols)
    got = _host(seq)
    assert ok.all() and all(_same(got[k], want[k]) for k in KEYS) and all(_same(g, w) for g, w in zip(got["columns"], want["columns"]))
    assert written.any() and (want["trunc"] != 0).any()
    h = lambda t, *shape: t.cpu().numpy().reshape(*shape)  # noqa: E731
    wvs, wpg = vtrace_model(want["reward"], want["done"], want["trunc"], h(value, L, n), h(last_value, n), h(ratio, L, n),
                            h(terminal_value, L, n), gamma=0.97, lam=0.9)
    assert _same(h(vs, L, n), wvs) and _same(h(pg, L, n), wpg)
    assert np.abs(h(ratio, L, n) - 1.0).max() > 0.1  # (off-policy: the correction does something)
    # the sampled rows are the rollouts' own bits: the ring is not full, so slot = q + k
    reward, done = np.concatenate(hist["reward"]), np.concatenate(hist["done"])
    q, i = got["index"] // B, got["index"] % B
    slots = q[None, :] + np.arange(L)[:, None]
    assert _same(got["reward"], reward[slots, i[None, :]]) and _same(got["done"], done[slots, i[None, :]])
    assert _same(got["columns"][1], cols[1][slots, i[None, :]])
    env.close()


def test_native_refusals_enqueue_and_write_nothing():
    """7: SG_ERR_INVALID with a message; the outputs keep their prefill and the ring's call counter stands"""
    from space_gym_amd._native import NativeError, check
    import torch
    env, ring, _, _, _ = _filled("GoalContinuous3P-v0", 16, 8, 2.5, False)
    T, n, L = 16, 67, 5
    out = _prefilled(env, n, L)
    before = _host(out)
    col, col_out = torch.zeros((T, 8), device="cuda"), torch.zeros((L, n), device="cuda")
    ex = (col.data_ptr(), col_out.data_ptr())
    cases = {
        "struct_size": dict(struct_size=20), "null cfg": dict(cfg=False), "null out": dict(seqs=False),
        "length = 0": dict(L=0), "length = 16": dict(L=T), "length = -1": dict(L=-1),
        "n = -1": dict(n=-1), "n = 2147483648": dict(n=2 ** 31), r"\(length \+ 1\) \* n": dict(n=2 ** 30, L=1),
        "null obs": dict(drop=("obs",)), "null.*action": dict(drop=("action",)), "null.*reward": dict(drop=("reward",)),
        "null.*done": dict(drop=("done",)), "null.*trunc": dict(drop=("trunc",)),
        "n_extra = 5": dict(n_extra=5, extras=[ex] * 4), "n_extra = -1": dict(n_extra=-1),
        r"null extra_in\[1\]": dict(n_extra=2, extras=[ex]), r"null extra_in\[0\] or extra_out\[0\]": dict(n_extra=1, extras=[(ex[0], None)]),
    }
    for match, kw in cases.items():
        _, call = _native_call(env, ring, kw.pop("n", n), kw.pop("L", L), out, **kw)
        rc = call()
        assert rc == -1, match
        with pytest.raises(NativeError, match=match):
            check(env._lib, env._h, rc, "sg_replay_sequence_device")
    # auto_reset off, as for the ring
    _, call = _native_call(env, ring, n, L, out)
    env.set_auto_reset(False)
    rc = call()
    env.set_auto_reset(True)
    assert rc == -1
    # n = 0 is accepted and enqueues nothing; the optional outputs may be absent
    _, call = _native_call(env, ring, 0, L, out)
    assert call() == 0
    torch.cuda.synchronize()
    got = _host(out)
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(before[k])), k
    assert _header(ring)["sample_calls"] == 0
    _, call = _native_call(env, ring, n, L, out, drop=("terminal_obs", "index"))
    assert call() == 0
    got = _host(out)
    assert np.array_equal(_bits(got["terminal_obs"]), _bits(before["terminal_obs"])) and (got["index"] == 77).all()
    assert not np.isnan(got["obs"]).any() and _header(ring)["sample_calls"] == 1
    env.check_status()
    env.close()
