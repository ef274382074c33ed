"""GPU tests of the device-resident snapshots (snapshot_torch / restore_torch, sg_snapshot_device / sg_restore_device).  The
oracles: the handle itself (what followed the snapshot is what follows an identity restore, bit for bit), save_state() blobs
column by column (a masked restore touches the masked envs only), and sg_load_state of a blob whose per-env columns were gathered
on the host with NumPy (a gathered restore is that, by construction).  Batches of 1000 and 70 001 envs: both step plans (the
wave-pair kernels; above 65 536 envs the many-subtile kernels), the last workgroup and wave partial."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = ["GoalContinuous3P-v0", "GoalContinuous4P-v0", "GoalContinuous2P-v0", "KeplerCircleOrbit-v0", "KeplerRandomOrbits-v0",
       "GoalDiscrete3-v0"]
BATCHES = [1000, 70001]
PER_ENV = ("q0", "q1", "ctr", "aux", "pl0", "pl1", "cshift", "orbd", "ep_ret", "ep_len", "norm_returns")
PRE, W, EPISODE = 50, 200, 50  # steps before the snapshot, steps of a window, TimeLimit


def make(env_id, n, **kw):
    import space_gym_amd as sg
    kw.setdefault("max_episode_steps", EPISODE)
    env = sg.make_vec(env_id, n, device=0, **kw)
    env.set_counters(True)
    return env


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    """bit for bit (NaN rows included)"""
    import torch
    return torch.equal(_bits(a), _bits(b))


def _random_mask(n, p, seed):
    import torch
    return torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) < p


def _randint(n, hi, seed):
    import torch
    return torch.randint(0, hi, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed), dtype=torch.int32)


def _is_goal(env):
    return env.spec["family"] == "goal"


def _window(env, acts, mode, stats=False):
    """W = len(acts) steps as a step_torch loop (mode "step") or as rollouts of K steps (mode K); returns every output: obs,
    reward, done, truncated, the terminal observations (dense NaN-filled rows / sorted records per rollout), with `stats` the
    episode records, and the counters of the window"""
    import torch
    n, D, steps = env.num_envs, env.obs_dim, int(acts.shape[0])
    env.counters(reset=True)
    out = {}
    if mode == "step":
        obs, tobs = torch.empty((steps, n, D), device="cuda"), torch.full((steps, n, D), float("nan"), device="cuda")
        rew = torch.empty((steps, n), device="cuda")
        done, trunc = torch.empty((steps, n), dtype=torch.uint8, device="cuda"), torch.empty((steps, n), dtype=torch.uint8, device="cuda")
        if stats:
            out["ep_r"] = torch.full((steps, n), float("nan"), dtype=torch.float64, device="cuda")
            out["ep_l"] = torch.full((steps, n), -1, dtype=torch.int32, device="cuda")
        for t in range(steps):
            o = dict(obs=obs[t], reward=rew[t], done=done[t], trunc=trunc[t])
            env.step_torch(acts[t], out=o, terminal_obs=tobs[t], episodes=dict(r=out["ep_r"][t], l=out["ep_l"][t]) if stats else None)
        out.update(obs=obs, reward=rew, done=done, trunc=trunc, tobs=tobs)
    else:
        K = int(mode)
        assert steps % K == 0
        obs, rew = torch.empty((steps, n, D), device="cuda"), torch.empty((steps, n), device="cuda")
        done, trunc = torch.empty((steps, n), dtype=torch.uint8, device="cuda"), torch.empty((steps, n), dtype=torch.uint8, device="cuda")
        cap = 2 * n * (K // EPISODE + 2)
        for c in range(steps // K):
            s = slice(c * K, (c + 1) * K)
            term = env.terminal_list_torch(cap)
            eps = env.episode_list_torch(cap) if stats else None
            env.rollout_torch(acts[s].contiguous(), obs[s], rew[s], done[s], trunc[s], terminal=term, episodes=eps)
            for k, v in zip(("t_step", "t_env", "t_obs"), env.terminal_records(term)):
                out[f"{k}{c}"] = torch.as_tensor(v)
            if stats:
                for k, v in env.episode_records(eps).items():
                    out[f"e_{k}{c}"] = torch.as_tensor(v)
        out.update(obs=obs, reward=rew, done=done, trunc=trunc)
    env.check_status()
    return out, env.counters(reset=True)


def _assert_windows_equal(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert _same(a[k], b[k]), (what, k)


def _assert_not_vacuous(env, counters, what):
    assert counters["episodes_finished"] > 0, (what, counters)  # auto-resets inside the window
    if _is_goal(env):
        assert counters["goal_hits"] > 0, (what, counters)  # goal resamples (random draws of the env's own stream)


def _columns(env, blob):
    return {k: v for k, v in env.snapshot_columns(blob).items() if k in PER_ENV}


def _warm(env, seed, steps=PRE):
    env.reset_torch()
    acts = env.random_actions_torch(steps, seed=seed)
    for t in range(steps):
        env.step_torch(acts[t])


# ---------------------------------------------------------------------------------------------------- 1. identity restore
@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["step", 20, 200])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id", IDS)
def test_identity_restore_resumes_bit_for_bit(env_id, n, mode):
    env = make(env_id, n, seed=3)
    _warm(env, seed=1)
    snap = env.snapshot_torch()
    acts = env.random_actions_torch(W, seed=2)
    first, c1 = _window(env, acts, mode)
    _assert_not_vacuous(env, c1, (env_id, n, mode))
    env.restore_torch(snap)
    second, c2 = _window(env, acts, mode)
    _assert_windows_equal(first, second, (env_id, n, mode))
    assert c1 == c2
    env.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["step", 20, 200])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_identity_restore_resumes_the_episode_statistics(env_id, n, mode):
    """the episode records (return float64, length) of the two windows are equal: the running sums are part of the snapshot"""
    env = make(env_id, n, seed=4, episode_statistics=True)
    _warm(env, seed=5)
    snap = env.snapshot_torch()
    assert snap.buffer.numel() == int(env._lib.sg_snapshot_bytes(env._h))
    acts = env.random_actions_torch(W, seed=6)
    first, c1 = _window(env, acts, mode, stats=True)
    _assert_not_vacuous(env, c1, (env_id, n, mode))
    mid = _columns(env, env.save_state())
    env.restore_torch(snap)
    second, _ = _window(env, acts, mode, stats=True)
    _assert_windows_equal(first, second, (env_id, n, mode))
    end = _columns(env, env.save_state())
    for k in mid:
        assert np.array_equal(mid[k], end[k]), k  # (ep_ret / ep_len among them)
    env.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["step", 200])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerCircleOrbit-v0"])
def test_identity_restore_with_frozen_normalization(env_id, n, mode):
    """normalized observations and rewards of the two windows are equal (the per-env discounted returns are part of the
    snapshot); the running statistics are not touched by the restore, and the restored rows are the normalized observation of
    the state: what the last step before the snapshot returned for the envs that did not resample their goal there"""
    import torch
    env = make(env_id, n, seed=5, normalize_reward=True, normalize_obs=True)
    env.reset_torch()
    acts0 = env.random_actions_torch(PRE, seed=7)
    for t in range(PRE - 1):
        env.step_torch(acts0[t])
    env.set_normalization(update=False)
    goal0 = env.get_state()["goal"].copy() if _is_goal(env) else None
    last_obs, _, last_done, _ = (x.clone() for x in env.step_torch(acts0[PRE - 1]))
    snap = env.snapshot_torch()
    at_snapshot = env.normalizer_state()
    acts = env.random_actions_torch(W, seed=8)
    first, c1 = _window(env, acts, mode)
    _assert_not_vacuous(env, c1, (env_id, n, mode))
    before = env.normalizer_state()
    out = torch.full((n, env.obs_dim), float("nan"), device="cuda")
    env.restore_torch(snap, out=out)
    after = env.normalizer_state()
    for k in before:
        want = at_snapshot[k] if k == "returns" else before[k]
        assert np.array_equal(np.asarray(after[k]), np.asarray(want)), k
    keep = np.ones(n, bool)
    if goal0 is not None:
        keep = ~((env.get_state()["goal"] != goal0).any(axis=1) & (_np(last_done) == 0))
    assert keep.sum() > n // 2
    assert _same(out[torch.as_tensor(keep, device="cuda")], last_obs[torch.as_tensor(keep, device="cuda")])
    second, _ = _window(env, acts, mode)
    _assert_windows_equal(first, second, (env_id, n, mode))
    env.close()


# ---------------------------------------------------------------------------------------------------- 2. masked restore
@pytest.mark.timeout(900)
@pytest.mark.parametrize("which", ["random", "zeros", "ones"])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id,extras", [("GoalContinuous3P-v0", True), ("GoalContinuous4P-v0", False), ("GoalContinuous2P-v0", False),
                                           ("KeplerCircleOrbit-v0", False), ("KeplerRandomOrbits-v0", True), ("GoalDiscrete3-v0", False)])
def test_masked_restore_touches_only_the_masked_envs(env_id, extras, n, which):
    """every per-env column of save_state() after the restore is where(mask, at the snapshot, just before the restore); with
    `extras` that includes the running episode statistics and the normalizer's returns; `out` is written in the masked rows"""
    import torch
    kw = dict(episode_statistics=True, normalize_obs=True, normalize_reward=True) if extras else {}
    env = make(env_id, n, seed=9, **kw)
    _warm(env, seed=3)
    snap = env.snapshot_torch()
    at_snapshot = _columns(env, env.save_state())
    acts = env.random_actions_torch(30, seed=4)
    for t in range(30):
        env.step_torch(acts[t])
    blob = env.save_state()
    before = _columns(env, blob)
    assert any(not np.array_equal(at_snapshot[k], before[k]) for k in before)
    if extras:
        assert {"ep_ret", "ep_len", "norm_returns"} <= set(before)
    mask = {"random": _random_mask(n, 0.3, seed=5), "zeros": torch.zeros(n, dtype=torch.bool, device="cuda"),
            "ones": torch.ones(n, dtype=torch.bool, device="cuda")}[which]
    m = _np(mask)
    out = torch.full((n, env.obs_dim), float("nan"), device="cuda")
    stats = env.normalizer_state() if extras else None
    got = env.restore_torch(snap, mask=mask, out=out)
    env.check_status()
    assert got is out
    rows_written = ~torch.isnan(out).any(dim=1)
    assert torch.equal(rows_written, mask) and torch.equal(torch.isnan(out).all(dim=1), ~mask)
    after_blob = env.save_state()
    after = _columns(env, after_blob)
    assert after.keys() == before.keys()
    for k in before:
        sel = m.reshape((n,) + (1,) * (before[k].ndim - 1))
        assert np.array_equal(after[k], np.where(sel, at_snapshot[k], before[k])), (which, k)
    if which == "zeros":
        assert np.array_equal(after_blob, blob)
    if extras:
        now = env.normalizer_state()
        for k in stats:
            if k != "returns":
                assert np.array_equal(np.asarray(now[k]), np.asarray(stats[k])), k
    env.close()


# ---------------------------------------------------------------------------------------------------- 3. gathered restore
def _gather_case(n, which):
    import torch
    if which == "permutation":
        src = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11)).to(torch.int32)
        return None, src
    if which == "broadcast":
        return None, torch.full((n,), 7, dtype=torch.int32, device="cuda")
    return _random_mask(n, 0.4, seed=12), _randint(n, n, seed=13)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("which", ["permutation", "broadcast", "masked"])
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id", IDS)
def test_gathered_restore_equals_the_host_path(env_id, n, which):
    """restore_torch(snap, mask, src) against load_state of a blob whose per-env columns were gathered with NumPy from the
    snapshot-time blob, in a second handle of the same id, batch and seed: the same columns, then the same 200 steps and the
    same K = 200 rollout, through goal resamples and auto-resets (which draw from the stream of the env's own index)"""
    import torch
    kw = dict(seed=21, episode_statistics=True)
    A, B = make(env_id, n, **kw), make(env_id, n, **kw)
    _warm(A, seed=2)
    snap = A.snapshot_torch()
    at_snapshot = A.save_state()
    acts = A.random_actions_torch(30, seed=3)
    for t in range(30):
        A.step_torch(acts[t])
    mask, src = _gather_case(n, which)
    want = A.save_state().copy()
    cols_w, cols_s = _columns(A, want), _columns(A, at_snapshot)
    m = _np(mask) if mask is not None else np.ones(n, bool)
    j = _np(src).astype(np.int64)
    for k in cols_w:
        cols_w[k][m] = cols_s[k][j[m]]  # (views into `want`)
    B.load_state(want)
    A.restore_torch(snap, mask=mask, src=src)
    A.check_status()
    ca, cb = _columns(A, A.save_state()), _columns(B, B.save_state())
    assert ca.keys() == cb.keys() and "ep_ret" in ca
    for k in ca:
        assert np.array_equal(ca[k], cb[k]), (which, k)
    steps = A.random_actions_torch(W, seed=4)
    wa, counters = _window(A, steps, "step", stats=True)
    wb, _ = _window(B, steps, "step", stats=True)
    _assert_not_vacuous(A, counters, (env_id, n, which, "steps"))
    _assert_windows_equal(wa, wb, (env_id, n, which, "steps"))
    more = A.random_actions_torch(W, seed=5)
    wa, counters = _window(A, more, 200, stats=True)
    wb, _ = _window(B, more, 200, stats=True)
    _assert_not_vacuous(A, counters, (env_id, n, which, "rollout"))
    _assert_windows_equal(wa, wb, (env_id, n, which, "rollout"))
    assert np.array_equal(A.save_state(), B.save_state())
    A.close(); B.close()


# ---------------------------------------------------------------------------------------------------- 4. observation rows
@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id", IDS)
def test_restored_rows_are_the_observation_of_the_state(env_id, n):
    """a snapshot right after a step, restored: the rows equal that step's rows, except the goal lidar of the envs whose goal
    the step resampled (the step observes before it resamples; the restore observes the state)"""
    import torch
    env = make(env_id, n, seed=31)
    _warm(env, seed=6, steps=PRE - 1)
    acts = env.random_actions_torch(12, seed=7)
    resampled_total = 0
    for t in range(12):
        s0 = env.get_state()
        obs, _, done, _ = (x.clone() for x in env.step_torch(acts[t]))
        snap = env.snapshot_torch()
        s1 = env.get_state()
        env.step_torch(acts[t])  # (the handle moves on: the rows below come from the snapshot)
        rows = _np(env.restore_torch(snap, out=torch.full((n, env.obs_dim), float("nan"), device="cuda")))
        o = _np(obs)
        if not _is_goal(env):
            assert np.array_equal(rows.view(np.uint32), o.view(np.uint32)), t
            continue
        resampled = (s0["goal"] != s1["goal"]).any(axis=1) & (_np(done) == 0)
        resampled_total += int(resampled.sum())
        assert np.array_equal(rows[~resampled].view(np.uint32), o[~resampled].view(np.uint32)), t
        head = 7 + 2 * env.n_planets
        assert np.array_equal(rows[resampled, :head].view(np.uint32), o[resampled, :head].view(np.uint32)), t
        lidar = (s1["goal"].astype(np.float32) - s1["ship"][:, :2].astype(np.float32)) * np.float32(2.0 / 3.0)
        assert np.array_equal(rows[resampled, head:].view(np.uint32), lidar[resampled].astype(np.float32).view(np.uint32)), t
    if _is_goal(env):
        assert resampled_total > 0
    env.close()


# ---------------------------------------------------------------------------------------------------- 5. graph capture
def _capture(fn):
    import torch
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warm = torch.cuda.CUDAGraph()  # (torch's own per-capture state is made by a first capture)
    with torch.cuda.stream(s):
        with torch.cuda.graph(warm, stream=s):
            pass
    g = torch.cuda.CUDAGraph()
    before = torch.cuda.memory_allocated()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before  # the capture allocates nothing
    return g


@pytest.mark.timeout(600)
@pytest.mark.parametrize("render", [False, True])
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_graph_of_restore_and_rollout_equals_eager(env_id, render):
    """restore_torch(snap, mask, src) + a K = 20 rollout in one graph: three replays give the eager result.  With rendering
    on, the frame rendered after each replay is the eager run's: the traces start afresh on a replayed restore as well"""
    import torch
    n, K = 8192, 20
    kw = dict(seed=41, **(dict(render=dict(capacity=4)) if render else {}))
    G, E = make(env_id, n, **kw), make(env_id, n, **kw)
    ids = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    for e in (G, E):
        _warm(e, seed=8)
    snap_g, snap_e = G.snapshot_torch(), E.snapshot_torch()
    assert torch.equal(snap_g.buffer, snap_e.buffer)
    mask, src = _random_mask(n, 0.5, seed=9), _randint(n, n, seed=10)
    mask[:4] = True  # (the rendered envs are restored)
    acts = G.random_actions_torch(K, seed=11)
    D = G.obs_dim

    def bufs():
        return (torch.empty((K, n, D), device="cuda"), torch.empty((K, n), device="cuda"),
                torch.empty((K, n), dtype=torch.uint8, device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda"))
    out_g, out_e, row_g = bufs(), bufs(), torch.zeros((n, D), device="cuda")
    G.rollout_torch(acts, *bufs())  # (outside capture once; the handles stay in step)
    E.rollout_torch(acts, *bufs())

    def graphed():
        G.restore_torch(snap_g, mask=mask, src=src, out=row_g)
        G.rollout_torch(acts, *out_g)
    g = _capture(graphed)
    F = make(env_id, n, **kw)  # (rendering: a handle whose traces are empty by construction, load_state starts them afresh)
    grow = G.random_actions_torch(20, seed=12)
    masked_rows = []
    for rep in range(3):
        # both handles move on (the unmasked envs keep going); with rendering on the traces of the rendered envs grow
        for t in range(20):
            G.step_torch(grow[t]); E.step_torch(grow[t])
            if render:
                assert torch.equal(G.render_torch(ids, size=256), E.render_torch(ids, size=256))
        if render:
            F.load_state(G.save_state())
            assert not torch.equal(G.render_torch(ids, size=256), F.render_torch(ids, size=256))  # the grown trace shows
        row_e = E.restore_torch(snap_e, mask=mask, src=src, out=torch.zeros((n, D), device="cuda"))
        E.rollout_torch(acts, *out_e)
        for t in out_g:
            t.zero_()
        row_g.zero_()
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(out_g, out_e):
            assert _same(x, y), rep
        assert _same(row_g, row_e), rep
        masked_rows.append([x[:, mask].clone() for x in out_g])
        if render:  # restore, 20 steps, one frame: the trace holds that one position, on a replayed restore as well
            F.load_state(G.save_state())
            fg = G.render_torch(ids, size=256)
            assert torch.equal(fg, E.render_torch(ids, size=256)) and torch.equal(fg, F.render_torch(ids, size=256)), rep
    # three replays, identical outputs: of the restored envs only -- the others are not rolled back and move on between replays
    for other in masked_rows[1:]:
        for x, y in zip(masked_rows[0], other):
            assert _same(x, y)
    F.close()
    G.check_status(); E.check_status()
    assert np.array_equal(G.save_state(), E.save_state())
    G.close(); E.close()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def _restore_raw(env, buf, nbytes=None, mask=None, src=None, out=None):
    return env._lib.sg_restore_device(env._h, C.c_void_p(buf.data_ptr()), C.c_size_t(buf.numel() if nbytes is None else nbytes),
                                      C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                      C.c_void_p(src.data_ptr()) if src is not None else None,
                                      C.c_void_p(out.data_ptr()) if out is not None else None, env._stream())


@pytest.mark.timeout(600)
@pytest.mark.parametrize("other", ["batch", "id", "blocks", "garbage"])
def test_a_snapshot_of_another_handle_restores_nothing(other):
    """through the C ABI (restore_torch refuses these on the host): the kernel reads the header first, writes nothing and sets
    the status word"""
    import torch
    from space_gym_amd._native import NativeError
    n = 5000
    env = make("GoalContinuous3P-v0", n, seed=1)
    _warm(env, seed=2)
    need = int(env._lib.sg_snapshot_bytes(env._h))
    buf = torch.zeros(2 * need, dtype=torch.uint8, device="cuda")
    if other != "garbage":
        donor = {"batch": lambda: make("GoalContinuous3P-v0", n - 1, seed=1), "id": lambda: make("GoalContinuous4P-v0", n // 2, seed=1),
                 "blocks": lambda: make("GoalContinuous3P-v0", n, seed=1, episode_statistics=True)}[other]()
        _warm(donor, seed=2)
        s = donor.snapshot_torch()
        assert s.buffer.numel() <= buf.numel()
        buf[:s.buffer.numel()].copy_(s.buffer)
        donor.close()
    blob = env.save_state()
    out = torch.full((n, env.obs_dim), float("nan"), device="cuda")
    assert _restore_raw(env, buf, out=out) == 0  # enqueued: the refusal is the kernel's
    with pytest.raises(NativeError, match="sg_restore_device: a snapshot of another env id, batch size or configuration"):
        env.check_status()
    env.check_status()  # reported once, cleared
    assert np.array_equal(env.save_state(), blob) and torch.isnan(out).all()
    env.step_torch(env.random_actions_torch(1, seed=3)[0])  # the handle works on
    env.check_status()
    env.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_source_indices_outside_the_batch_leave_their_envs_alone(env_id, n):
    import torch
    from space_gym_amd._native import NativeError
    env = make(env_id, n, seed=2, normalize_obs=True)
    _warm(env, seed=4)
    snap = env.snapshot_torch()
    at_snapshot = _columns(env, env.save_state())
    acts = env.random_actions_torch(20, seed=5)
    for t in range(20):
        env.step_torch(acts[t])
    before = _columns(env, env.save_state())
    src = _randint(n, n, seed=6)
    bad = _np(_random_mask(n, 0.05, seed=7))
    bad[[0, n - 1]] = True
    j = _np(src).astype(np.int64)
    j[bad] = np.where(np.arange(n)[bad] % 2 == 0, -1, n)
    j[n - 1] = np.iinfo(np.int32).max
    out = torch.full((n, env.obs_dim), float("nan"), device="cuda")
    env.restore_torch(snap, src=torch.as_tensor(j.astype(np.int32), device="cuda"), out=out)
    with pytest.raises(NativeError, match="source index outside the batch"):
        env.check_status()
    env.check_status()  # raised once
    after = _columns(env, env.save_state())
    for k in before:
        want = np.array(before[k])
        want[~bad] = at_snapshot[k][j[~bad]]
        assert np.array_equal(after[k], want), k
    assert torch.equal(torch.isnan(out).all(dim=1), torch.as_tensor(bad, device="cuda"))
    assert not torch.isnan(out[torch.as_tensor(~bad, device="cuda")]).any()
    env.close()


@pytest.mark.timeout(300)
def test_host_side_refusals_and_the_numpy_route():
    import torch
    from space_gym_amd._native import NativeError
    n = 3000
    env = make("GoalContinuous3P-v0", n, seed=1)
    buf = torch.zeros(int(env._lib.sg_snapshot_bytes(env._h)) + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(NativeError, match="sg_reset first"):
        env.snapshot_torch()  # fresh after create
    env.reset()
    snap = env.snapshot()
    assert snap.num_envs == n and snap.env_id == "GoalContinuous3P-v0" and snap.buffer.dtype == torch.uint8
    assert _restore_raw(env, snap.buffer, nbytes=snap.buffer.numel() - 1) < 0 and "needed" in env._lib.sg_last_error(env._h).decode()
    assert _restore_raw(env, buf[1:]) < 0 and "aligned" in env._lib.sg_last_error(env._h).decode()
    assert env._lib.sg_restore_device(env._h, None, C.c_size_t(1 << 30), None, None, None, env._stream()) < 0
    other = make("GoalContinuous3P-v0", n + 1, seed=1)
    other.reset()
    with pytest.raises(ValueError, match="snap"):
        other.restore_torch(snap)
    other.close()
    env.seed(5)
    with pytest.raises(NativeError, match="sg_reset first"):
        env.restore_torch(snap)  # fresh after seed
    env.reset()
    rng = np.random.default_rng(0)
    first = env.step(rng.uniform(-1, 1, (n, 2)).astype(np.float32))[0]
    snap = env.snapshot()
    for _ in range(5):
        last = env.step(rng.uniform(-1, 1, (n, 2)).astype(np.float32))[0]
    env.step_async(rng.uniform(-1, 1, (n, 2)).astype(np.float32))  # a step in flight: refused on the host, nothing enqueued
    with pytest.raises(NativeError, match="a step is in flight"):
        env.snapshot_torch(out=snap)
    with pytest.raises(NativeError, match="a step is in flight"):
        env.restore_torch(snap)
    last = env.step_wait()[0]
    m = rng.random(n) < 0.3
    got = env.restore(snap, mask=m)
    assert np.array_equal(got[~m], last[~m])
    st = env.get_state()
    assert np.array_equal(got[m][:, :2], st["ship"][m][:, :2]) and not np.array_equal(got[m], last[m])
    src = rng.integers(0, n, n)
    got = env.restore(snap, src=src)
    st = env.get_state()
    assert np.array_equal(got[:, :2], st["ship"][:, :2])
    env.check_status()
    env.close()
    assert first.shape == (n, env.obs_dim)
