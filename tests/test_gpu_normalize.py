"""GPU tests of the running normalization (sg_set_normalize): a handle with normalization on next to a twin with the same seed
and actions and normalization off, whose raw outputs feed the NumPy float64 model of gym's NormalizeObservation /
NormalizeReward (tests/normalize_model.py) -- on every rollout plan, through every route, with terminal observations, episode
statistics, update=False, reset, snapshots and graph capture."""
import numpy as np
import pytest

from normalize_model import NormalizeModel

pytestmark = pytest.mark.gpu

MAX_STEPS = 45


def make(env_id, n, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _actions(env, K, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if env.discrete:
        return torch.randint(0, 6, (K, env.num_envs), device="cuda", generator=gen, dtype=torch.int32)
    return torch.rand((K, env.num_envs, 2), device="cuda", generator=gen) * 2 - 1


def _rollout_buffers(env, K):
    import torch
    n, D = env.num_envs, env.obs_dim
    return (torch.empty((K, n, D), device="cuda"), torch.empty((K, n), device="cuda"),
            torch.empty((K, n), dtype=torch.uint8, device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda"))


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_f32_close(got, want, what):
    """within one float32 ulp of the float64 model's value, rounded (or 1e-10 absolute: values near 0, where the last bits of
    the running mean -- which the model sums in another order -- decide)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = (d <= np.spacing(np.abs(want)).astype(np.float64)) | (d <= 1e-10) | nan
    assert ok.all(), (what, int((~ok).sum()), float(d[~ok].max()))


def assert_state_matches(env, model, what):
    st = env.normalizer_state()
    for k, rms in (("obs", model.obs_rms), ("ret", model.ret_rms)):
        assert float(st[k + "_count"]) == rms.count, (what, k)  # bit for bit
        np.testing.assert_allclose(st[k + "_mean"], rms.mean, rtol=1e-10, atol=1e-300, err_msg=f"{what} {k} mean")
        np.testing.assert_allclose(st[k + "_var"], rms.var, rtol=1e-10, atol=1e-300, err_msg=f"{what} {k} var")
    assert np.array_equal(st["returns"].view(np.uint64), model.returns.view(np.uint64)), what  # bit for bit


CASES = [("GoalContinuous3P-v0", None), ("KeplerRandomOrbits-v0", None), ("GoalDiscrete3-v0", None),
         ("GoalContinuous3P-v0", "acceleration")]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("plan", ["pair", "single", "unfused", "step_torch"])
@pytest.mark.parametrize("env_id,steering", CASES)
def test_outputs_and_statistics_match_the_model(env_id, steering, plan, monkeypatch):
    """160 steps (rollouts: two calls of 60 + 100, the first with a terminal list; step_torch: with dense terminal rows):
    normalized obs / reward within one float32 ulp of the model fed the twin's raw outputs, running means and variances within
    1e-10, counts and returns bit for bit after every call; terminal observations normalized with their step's statistics"""
    import torch
    n = 8192
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", "single" if plan == "single" else "pair")
    kw = dict(steering=steering) if steering else {}
    env = make(env_id, n, seed=21, max_episode_steps=MAX_STEPS, normalize_obs=True, normalize_reward=True, **kw)
    twin = make(env_id, n, seed=21, max_episode_steps=MAX_STEPS, **kw)
    if plan == "unfused":
        env.set_unfused_rollout(True)
    model = NormalizeModel(n, env.obs_dim)
    assert_f32_close(_np(env.reset_torch()), model.reset(_np(twin.reset_torch())), "reset")
    assert_state_matches(env, model, "reset")
    a = _actions(env, 160, seed=3)
    n_term = 0
    if plan == "step_torch":
        for t in range(160):
            tobs = torch.full((n, env.obs_dim), float("nan"), device="cuda")
            ttwin = torch.full((n, env.obs_dim), float("nan"), device="cuda")
            ob, rw, _, _ = env.step_torch(a[t], terminal_obs=tobs)
            rob, rrw, rdn, _ = twin.step_torch(a[t], terminal_obs=ttwin)
            d = _np(rdn).astype(bool)
            wo, wr, wt = model.step(_np(rob), _np(rrw), d, terminal_obs=_np(ttwin)[d])
            assert_f32_close(_np(ob), wo, f"obs {t}")
            assert_f32_close(_np(rw), wr, f"reward {t}")
            assert_f32_close(_np(tobs)[d], wt, f"terminal rows {t}")
            assert np.isnan(_np(tobs)[~d]).all()  # rows of envs that did not finish are left untouched
            n_term += int(d.sum())
            if t % 40 == 39:
                assert_state_matches(env, model, f"step {t}")
    else:
        for lo, hi in ((0, 60), (60, 160)):
            K = hi - lo
            bufs, raw = _rollout_buffers(env, K), _rollout_buffers(twin, K)
            term = env.terminal_list_torch(n * K // 4) if lo == 0 else None
            rterm = twin.terminal_list_torch(n * K // 4) if lo == 0 else None
            env.rollout_torch(a[lo:hi].contiguous(), *bufs, terminal=term)
            twin.rollout_torch(a[lo:hi].contiguous(), *raw, terminal=rterm)
            torch.cuda.synchronize()
            ro, rr, rd = _np(raw[0]), _np(raw[1]), _np(raw[2]).astype(bool)
            if lo == 0:
                ts, te, tob = env.terminal_records(term)
                rts, rte, rtob = twin.terminal_records(rterm)
                assert np.array_equal(ts, rts) and np.array_equal(te, rte)
            go, gr = _np(bufs[0]), _np(bufs[1])
            for t in range(K):
                wo, wr, wt = model.step(ro[t], rr[t], rd[t], terminal_obs=rtob[rts == t] if lo == 0 else None)
                assert_f32_close(go[t], wo, f"obs {lo + t}")
                assert_f32_close(gr[t], wr, f"reward {lo + t}")
                if lo == 0:
                    assert_f32_close(tob[ts == t], wt, f"terminal records {t}")
                    n_term += int((ts == t).sum())
            assert_state_matches(env, model, f"call {lo}")
    assert n_term > 0
    env.check_status()
    env.close(); twin.close()


def _hash(t):
    """exact fingerprint of a float32 / uint8 device tensor's bits"""
    import torch
    v = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8).reshape(-1).to(torch.int64)
    w = torch.arange(v.numel(), device=v.device, dtype=torch.int64) % 1000003 + 1
    return int((v * w).sum().item())


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [1, 63, 1000, 8192, 131072])
def test_every_route_gives_the_same_bits(n):
    """step(), step_async / step_wait, step_torch and rollouts of K = 1 / 20 / 100 over the same actions: bit-identical
    normalized outputs (terminal observations of step() and step_torch included) and statistics.  131 072 envs: the
    one-wave, multi-subtile step kernels"""
    import torch
    K = 100 if n < 131072 else 40
    routes = ["step", "async", "step_torch", "k1", "k20", "k100"]
    envs = {r: make("GoalContinuous3P-v0", n, seed=17, max_episode_steps=20, normalize_obs=True, normalize_reward=True,
                    terminal_observation=True) for r in routes}
    a = _actions(envs["step"], K, seed=9)
    fp = {r: [] for r in routes}
    tfp = {r: [] for r in ("step", "step_torch")}
    for r, e in envs.items():
        if r in ("step", "async"):
            fp[r].append(_hash(torch.from_numpy(e.reset()).cuda()))
            for t in range(K):
                if r == "step":
                    ob, rw, dn, info = e.step(_np(a[t]))
                else:
                    e.step_async(_np(a[t]))
                    ob, rw, dn, info = e.step_wait()
                fp[r] += [_hash(torch.from_numpy(ob).cuda()), _hash(torch.from_numpy(rw).cuda())]
                if r == "step":
                    tfp[r].append(_hash(torch.from_numpy(np.nan_to_num(info["terminal_observation"], nan=7.0)).cuda()))
        elif r == "step_torch":
            fp[r].append(_hash(e.reset_torch()))
            for t in range(K):
                tobs = torch.full((n, e.obs_dim), float("nan"), device="cuda")
                ob, rw, dn, _ = e.step_torch(a[t], terminal_obs=tobs)
                fp[r] += [_hash(ob), _hash(rw)]
                tfp[r].append(_hash(tobs.nan_to_num(7.0)))
        else:
            k = int(r[1:])
            fp[r].append(_hash(e.reset_torch()))
            for lo in range(0, K, k):
                hi = min(K, lo + k)
                bufs = _rollout_buffers(e, hi - lo)
                e.rollout_torch(a[lo:hi].contiguous(), *bufs)
                for t in range(hi - lo):
                    fp[r] += [_hash(bufs[0][t]), _hash(bufs[1][t])]
        torch.cuda.synchronize()
    for r in routes[1:]:
        assert fp[r] == fp["step"], r
    assert tfp["step_torch"] == tfp["step"]
    ref = envs["step"].normalizer_state()
    for r in routes[1:]:
        st = envs[r].normalizer_state()
        for k in ref:
            assert np.array_equal(np.asarray(st[k]).view(np.uint64), np.asarray(ref[k]).view(np.uint64)), (r, k)
    for e in envs.values():
        e.close()


@pytest.mark.timeout(300)
def test_episode_statistics_stay_raw():
    """with normalization on, the episode returns are the twin's bit for bit: they are summed from the raw rewards"""
    import torch
    n, K = 8192, 90
    on = make("GoalContinuous3P-v0", n, seed=4, max_episode_steps=30, episode_statistics=True, normalize_obs=True,
              normalize_reward=True)
    off = make("GoalContinuous3P-v0", n, seed=4, max_episode_steps=30, episode_statistics=True)
    a = _actions(on, K, seed=1)
    recs, rews = [], []
    for e in (on, off):
        e.reset_torch()
        bufs = _rollout_buffers(e, K)
        el = e.episode_list_torch(n * 8)
        e.rollout_torch(a, *bufs, episodes=el)
        torch.cuda.synchronize()
        recs.append(e.episode_records(el))
        rews.append(_np(bufs[1]))
    for k in ("step", "env", "l", "truncated"):
        assert np.array_equal(recs[0][k], recs[1][k]), k
    assert np.array_equal(recs[0]["r"].view(np.uint64), recs[1]["r"].view(np.uint64)) and len(recs[0]["r"]) > 0
    assert not np.array_equal(rews[0], rews[1])  # (the returned rewards are normalized)
    on.close(); off.close()


@pytest.mark.timeout(300)
def test_switching_off_changes_nothing():
    """on for a while, then off: the outputs that follow and the snapshot bytes equal those of a handle that never had it"""
    import torch
    n, K = 8192, 40
    sw = make("GoalContinuous3P-v0", n, seed=5, max_episode_steps=25, normalize_obs=True, normalize_reward=True)
    never = make("GoalContinuous3P-v0", n, seed=5, max_episode_steps=25)
    a = _actions(sw, 2 * K, seed=2)
    outs = []
    for e in (sw, never):
        e.reset_torch()
        e.rollout_torch(a[:K].contiguous(), *_rollout_buffers(e, K))
        if e is sw:
            e.set_normalization(obs=False, reward=False)
            assert e.normalization()["obs"] is False
        bufs = _rollout_buffers(e, K)
        e.rollout_torch(a[K:].contiguous(), *bufs)
        torch.cuda.synchronize()
        outs.append((bufs, e.save_state(), e.step(_np(a[0]))))
    (b1, s1, h1), (b2, s2, h2) = outs
    for u, v in zip(b1, b2):
        assert torch.equal(u, v)
    assert s1.size == s2.size and np.array_equal(s1, s2) and int(s1[4:8].view(np.uint32)[0]) == 1
    for u, v in zip(h1[:3], h2[:3]):
        assert np.array_equal(u, v)
    sw.close(); never.close()


@pytest.mark.timeout(300)
def test_update_false_freezes_and_the_state_transfers():
    """update=False: statistics and returns stay as they are and the outputs use them (the model, frozen); an evaluation handle
    given the trained handle's statistics (set_normalizer_state) returns the same bits"""
    import torch
    n, K = 8192, 30
    env = make("GoalContinuous3P-v0", n, seed=8, max_episode_steps=20, normalize_obs=True, normalize_reward=True)
    ev = make("GoalContinuous3P-v0", n, seed=8, max_episode_steps=20)
    twin = make("GoalContinuous3P-v0", n, seed=8, max_episode_steps=20)
    a = _actions(env, 2 * K, seed=4)
    model = NormalizeModel(n, env.obs_dim)
    model.reset(_np(twin.reset_torch())); env.reset_torch(); ev.reset_torch()
    raw = _rollout_buffers(twin, K)
    twin.rollout_torch(a[:K].contiguous(), *raw)
    env.rollout_torch(a[:K].contiguous(), *_rollout_buffers(env, K))
    ev.rollout_torch(a[:K].contiguous(), *_rollout_buffers(ev, K))
    torch.cuda.synchronize()
    for t in range(K):
        model.step(_np(raw[0][t]), _np(raw[1][t]), _np(raw[2][t]).astype(bool))
    env.set_normalization(update=False)
    before = env.normalizer_state()
    ev.set_normalization(obs=True, reward=True, update=False)
    ev.set_normalizer_state(before)
    model.update = False
    bufs, ebufs, raw = _rollout_buffers(env, K), _rollout_buffers(ev, K), _rollout_buffers(twin, K)
    env.rollout_torch(a[K:].contiguous(), *bufs)
    ev.rollout_torch(a[K:].contiguous(), *ebufs)
    twin.rollout_torch(a[K:].contiguous(), *raw)
    torch.cuda.synchronize()
    after = env.normalizer_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for t in range(K):
        wo, wr, _ = model.step(_np(raw[0][t]), _np(raw[1][t]), _np(raw[2][t]).astype(bool))
        assert_f32_close(_np(bufs[0][t]), wo, f"obs {t}")
        assert_f32_close(_np(bufs[1][t]), wr, f"reward {t}")
    for u, v in zip(bufs, ebufs):
        assert torch.equal(u, v)
    env.close(); ev.close(); twin.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_reset_updates_the_observation_statistics_only(env_id):
    import torch
    n = 4096
    env = make(env_id, n, seed=3, max_episode_steps=20, normalize_obs=True, normalize_reward=True)
    twin = make(env_id, n, seed=3, max_episode_steps=20)
    model = NormalizeModel(n, env.obs_dim)
    assert_f32_close(env.reset(), model.reset(twin.reset()), "reset")
    a = _actions(env, 10, seed=1)
    raw, bufs = _rollout_buffers(twin, 10), _rollout_buffers(env, 10)
    twin.rollout_torch(a, *raw); env.rollout_torch(a, *bufs)
    torch.cuda.synchronize()
    for t in range(10):
        model.step(_np(raw[0][t]), _np(raw[1][t]), _np(raw[2][t]).astype(bool))
    before = env.normalizer_state()
    assert_f32_close(_np(env.reset_torch()), model.reset(_np(twin.reset_torch())), "second reset")
    after = env.normalizer_state()
    assert float(after["obs_count"]) == float(before["obs_count"]) + n  # the reset batch, and nothing else
    for k in ("ret_mean", "ret_var", "ret_count", "returns"):
        assert np.array_equal(before[k], after[k]), k
    assert_state_matches(env, model, "reset")
    env.close(); twin.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("episodes", [False, True])
def test_snapshot_resumes_bit_identically(episodes):
    """a snapshot taken with normalization on is version 3; loading it resumes outputs and statistics bit for bit, in the same
    handle and in a fresh one (where it switches normalization on); a version-1 blob restarts the statistics"""
    import torch
    n, K = 8192, 30
    env = make("GoalContinuous3P-v0", n, seed=12, max_episode_steps=MAX_STEPS, normalize_obs=True, normalize_reward=True,
               clip_obs=5.0, episode_statistics=episodes)
    env.reset_torch()
    a = _actions(env, 2 * K, seed=5)
    env.rollout_torch(a[:K].contiguous(), *_rollout_buffers(env, K))
    blob = env.save_state()
    assert int(blob[4:8].view(np.uint32)[0]) == 3 and blob.size == int(env._lib.sg_state_bytes(env._h))
    cols = env.snapshot_columns(blob)
    assert int(cols["flags"][0, 0]) == (3 if episodes else 2) and cols["norm_count"][0] > 1.0

    def run(e):
        bufs = _rollout_buffers(e, K)
        e.rollout_torch(a[K:].contiguous(), *bufs)
        torch.cuda.synchronize()
        return bufs, e.normalizer_state()
    first = run(env)
    env.load_state(blob)
    fresh = make("GoalContinuous3P-v0", n, seed=99, max_episode_steps=MAX_STEPS)
    fresh.load_state(blob)
    assert fresh.normalization()["obs"] and fresh.normalization()["clip_obs"] == 5.0
    assert fresh.episode_statistics == episodes
    for got in (run(env), run(fresh)):
        for u, v in zip(got[0], first[0]):
            assert torch.equal(u, v)
        for k in first[1]:
            assert np.array_equal(got[1][k], first[1][k]), k
    plain = make("GoalContinuous3P-v0", n, seed=12, max_episode_steps=MAX_STEPS)
    plain.reset_torch()
    env.load_state(plain.save_state())  # version 1 into a handle with normalization on: fresh statistics, same configuration
    st = env.normalizer_state()
    assert float(st["obs_count"]) == 1e-4 and np.all(st["obs_var"] == 1.0) and np.all(st["returns"] == 0.0)
    assert env.normalization()["clip_obs"] == 5.0
    env.close(); fresh.close(); plain.close()


@pytest.mark.timeout(300)
def test_graph_replay_advances_the_statistics():
    """step_torch and a prepare_rollout callable, each captured into a graph and replayed, equal eager calls on a twin, and
    every replay advances the statistics"""
    import torch
    n, T, K = 8192, 12, 20
    kw = dict(seed=7, max_episode_steps=12, normalize_obs=True, normalize_reward=True)
    graphed, eager = make("GoalContinuous3P-v0", n, **kw), make("GoalContinuous3P-v0", n, **kw)
    graphed.reset_torch(); eager.reset_torch()
    torch.cuda.synchronize()
    a = _actions(eager, T + 3 * K, seed=2)
    static_a = torch.empty((n, 2), device="cuda")
    out = dict(obs=torch.empty((n, graphed.obs_dim), device="cuda"), reward=torch.empty(n, device="cuda"),
               done=torch.empty(n, dtype=torch.uint8, device="cuda"), trunc=torch.empty(n, dtype=torch.uint8, device="cuda"))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        static_a.copy_(a[0])
        with torch.cuda.graph(g, stream=s):
            graphed.step_torch(static_a, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    counts = []
    for t in range(T):
        static_a.copy_(a[t])
        g.replay()
        torch.cuda.synchronize()
        ob, rw, dn, _ = eager.step_torch(a[t].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(out["obs"], ob) and torch.equal(out["reward"], rw) and torch.equal(out["done"], dn)
        counts.append(float(graphed.normalizer_state()["obs_count"]))
    want, c = [], 1e-4 + n  # (the reset, then one batch per replay)
    for _ in range(T):
        c += n
        want.append(c)
    assert counts == want
    static_k = a[T:T + K].clone()
    bufs = _rollout_buffers(graphed, K)
    call = graphed.prepare_rollout(static_k, *bufs)
    g2 = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g2, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for r in range(2):
        static_k.copy_(a[T + r * K:T + (r + 1) * K])
        g2.replay()
        ebufs = _rollout_buffers(eager, K)
        eager.rollout_torch(a[T + r * K:T + (r + 1) * K].contiguous(), *ebufs)
        torch.cuda.synchronize()
        for u, v in zip(bufs, ebufs):
            assert torch.equal(u, v)
    sg, se = graphed.normalizer_state(), eager.normalizer_state()
    for k in sg:
        assert np.array_equal(sg[k], se[k]), k
    graphed.check_status()
    graphed.close(); eager.close()
