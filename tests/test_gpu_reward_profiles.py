"""GPU tests of reward profiles (set_reward_profiles / set_env_profiles).  The oracle is by construction: every coefficient of a
profile enters the reward only, so env i under profile p must equal, bit for bit, env i of an ordinary handle made with p's
keywords (same seed, same actions) -- observations, rewards, flags and terminal observations, through resets and time limits.
Around it: rollouts against steps, the identity profile, indices changed on the device inside a captured graph, an index past
the table, episode statistics, normalization, masked reset, snapshots and the errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORACLE_IDS = [("GoalContinuous2P-v0", None), ("GoalContinuous3P-v0", None), ("GoalContinuous4P-v0", None),
              ("GoalDiscrete3-v0", None), ("GoalContinuous3P-v0", "acceleration"), ("KeplerCircleOrbit-v0", None),
              ("KeplerRandomOrbits-v0", None), ("KeplerDiscrete-v0", None)]


def make(env_id, n, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def random_profiles(family, P, seed):
    """P profiles with random values; about a third of the keywords left out (the handle's own value)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(P):
        if family == "goal":
            p = dict(survival_reward_scale=rng.uniform(-0.5, 0.5), goal_vel_reward_scale=rng.uniform(0.0, 2.0),
                     safety_reward_scale=rng.uniform(0.0, 5.0), goal_sparse_reward=rng.uniform(0.0, 20.0),
                     danger_zone=rng.uniform(0.0, 0.6))
        else:
            p = dict(numerator_C=rng.uniform(0.005, 0.1), rad_penalty_C=rng.uniform(0.5, 4.0), act_penalty_C=rng.uniform(0.0, 1.0))
        out.append({k: float(v) for k, v in p.items() if rng.uniform() > 0.33})
    return out


def _actions(env, K, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if env.discrete:
        return torch.randint(0, 6, (K, env.num_envs), device="cuda", generator=gen, dtype=torch.int32)
    return torch.rand((K, env.num_envs, 2), device="cuda", generator=gen) * 2 - 1


def _outs(env):
    import torch
    n, D = env.num_envs, env.obs_dim
    return (dict(obs=torch.empty((n, D), device="cuda"), reward=torch.empty(n, device="cuda"),
                 done=torch.empty(n, dtype=torch.uint8, device="cuda"), trunc=torch.empty(n, dtype=torch.uint8, device="cuda")),
            torch.full((n, D), float("nan"), device="cuda"))


def _same_rows(x, y, rows):
    """bit-equal rows (float compared as integers: NaN-free and -0.0 exact)"""
    import torch
    x, y = x[rows], y[rows]
    if x.dtype == torch.float32:
        x, y = x.view(torch.int32), y.view(torch.int32)
    return torch.equal(x, y)


def _run_oracle(env_id, steering, n, steps, seed, monkeypatch, plan):
    import torch
    monkeypatch.setenv("SPACEGYM_STEP_KERNEL", plan)
    kw = dict(seed=seed, max_episode_steps=60)
    if steering:
        kw["steering"] = steering
    probe = make(env_id, 1, **kw)
    family = probe.spec["family"]
    probe.close()
    P = 4 + seed % 5
    profs = random_profiles(family, P, seed)
    env = make(env_id, n, reward_profiles=profs, **kw)
    refs = [make(env_id, n, **kw, **p) for p in profs]
    idx = np.random.default_rng(seed + 1).integers(0, P, n).astype(np.uint8)
    env.set_env_profiles(idx)
    assert np.array_equal(env.env_profiles(), idx)
    it = torch.as_tensor(idx, device="cuda").long()
    rows = [it == p for p in range(P)]
    o0 = env.reset_torch().clone()
    for p, r in enumerate(refs):
        assert _same_rows(o0, r.reset_torch(), rows[p]), ("reset", p)
    acts = _actions(env, steps, seed + 2)
    out, tobs = _outs(env)
    routs = [_outs(r) for r in refs]
    finished = 0
    for t in range(steps):
        env.step_torch(acts[t], out=out, terminal_obs=tobs)
        done = out["done"].bool()
        finished += int(done.sum())
        for p, r in enumerate(refs):
            ro, rt = routs[p]
            r.step_torch(acts[t], out=ro, terminal_obs=rt)
            for k in ("obs", "reward", "done", "trunc"):
                assert _same_rows(out[k], ro[k], rows[p]), (env_id, plan, n, t, p, k)
            assert _same_rows(tobs, rt, rows[p] & done), (env_id, plan, n, t, p, "terminal_obs")
    assert finished > 0
    env.check_status()
    for x in [env] + refs:
        x.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("plan", ["pair", "single"])
@pytest.mark.parametrize("env_id, steering", ORACLE_IDS)
def test_profiled_env_equals_a_handle_made_with_its_profile(env_id, steering, plan, monkeypatch):
    """a ragged batch of 1000 envs, 300 steps: every row equals the ordinary handle of that env's profile"""
    _run_oracle(env_id, steering, 1000, 300, 11 + ORACLE_IDS.index((env_id, steering)), monkeypatch, plan)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("plan", ["pair", "single"])
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_profiled_env_above_the_pair_threshold(env_id, plan, monkeypatch):
    """70 001 envs (above one wave-pair workgroup per CU): the same oracle"""
    _run_oracle(env_id, None, 70001, 120, 5, monkeypatch, plan)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("plan", ["pair", "single", "unfused"])
@pytest.mark.parametrize("env_id", ["GoalContinuous2P-v0", "GoalContinuous3P-v0", "GoalContinuous4P-v0", "KeplerCircleOrbit-v0",
                                    "KeplerRandomOrbits-v0"])
def test_rollout_equals_steps(env_id, plan, monkeypatch):
    """rollout_torch of K = 50 with terminal and episode lists equals K step_torch calls of a twin with the same profiles.  The
    pair plan runs the profiled K-step kernel (*_pair_rollout_profiled_kernel); single (the one-wave K-step kernels have no
    profiled variant) and unfused run K launches of the profiled step kernel"""
    import torch
    n, K = 5000, 50
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", "single" if plan == "single" else "pair")
    profs = random_profiles("goal" if env_id.startswith("Goal") else "kepler", 5, 3)
    kw = dict(seed=9, max_episode_steps=20, reward_profiles=profs, episode_statistics=True)
    A, B = make(env_id, n, **kw), make(env_id, n, **kw)
    if plan == "unfused":
        A.set_unfused_rollout(True)
    kernel = A.rollout_kernel(K)
    if plan == "pair":
        assert kernel.split("<")[0] == ("goal" if env_id.startswith("Goal") else "kepler") + "_pair_rollout_profiled_kernel", kernel
    else:
        assert "_step_profiled_kernel<" in kernel, kernel
    idx = np.random.default_rng(4).integers(0, 5, n)
    A.set_env_profiles(idx); B.set_env_profiles(idx)
    A.reset_torch(); B.reset_torch()
    acts = _actions(A, K, 8)
    D = A.obs_dim
    obs, rew = torch.empty((K, n, D), device="cuda"), torch.empty((K, n), device="cuda")
    done, trunc = torch.empty((K, n), dtype=torch.uint8, device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda")
    term, eps = A.terminal_list_torch(n * K), A.episode_list_torch(n * K)
    A.rollout_torch(acts, obs, rew, done, trunc, terminal=term, episodes=eps)
    steps, envs, tobs = A.terminal_records(term)
    ep = A.episode_records(eps)
    to = torch.full((n, D), float("nan"), device="cuda")
    er = dict(r=torch.zeros(n, dtype=torch.float64, device="cuda"), l=torch.zeros(n, dtype=torch.int32, device="cuda"))
    want_t, want_e = [], []
    for t in range(K):
        ob, rw, dn, tr = B.step_torch(acts[t], terminal_obs=to, episodes=er)
        for x, y in ((ob, obs[t]), (rw, rew[t]), (dn, done[t]), (tr, trunc[t])):
            assert torch.equal(x, y), (plan, t)
        d = dn.bool().cpu().numpy()
        for i in np.flatnonzero(d):
            want_t.append((t, i, to[i].cpu().numpy()))
            want_e.append((t, i, float(er["r"][i]), int(er["l"][i])))
    assert len(want_t) == len(steps) > 0
    assert np.array_equal(steps, [w[0] for w in want_t]) and np.array_equal(envs, [w[1] for w in want_t])
    assert np.array_equal(tobs, np.stack([w[2] for w in want_t]))
    assert np.array_equal(ep["r"], [w[2] for w in want_e]) and np.array_equal(ep["l"], [w[3] for w in want_e])
    A.check_status()
    A.close(); B.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("plan", ["pair", "single"])
@pytest.mark.parametrize("env_id", ["GoalContinuous4P-v0", "KeplerRandomOrbits-v0", "GoalDiscrete2-v0"])
def test_identity_profile_changes_nothing(env_id, plan, monkeypatch):
    """one profile that sets nothing, every index 0: bit for bit a handle without profiles"""
    import torch
    monkeypatch.setenv("SPACEGYM_STEP_KERNEL", plan)
    n = 3000
    A, B = make(env_id, n, seed=21, max_episode_steps=40, reward_profiles=[{}]), make(env_id, n, seed=21, max_episode_steps=40)
    assert torch.equal(A.reset_torch(), B.reset_torch())
    acts = _actions(A, 100, 1)
    for t in range(100):
        for x, y in zip(A.step_torch(acts[t]), B.step_torch(acts[t])):
            assert torch.equal(x, y), t
    A.close(); B.close()


@pytest.mark.timeout(300)
def test_indices_set_inside_a_graph_apply_at_the_next_step():
    """set_env_profiles(tensor) + step_torch captured in one graph: each replay uses the indices it copied; an eager twin that
    sets the same indices from the host gives the same bits"""
    import torch
    n, T, P = 8192, 30, 6
    profs = random_profiles("goal", P, 17)
    kw = dict(seed=3, max_episode_steps=25, reward_profiles=profs)
    graphed, eager = make("GoalContinuous3P-v0", n, **kw), make("GoalContinuous3P-v0", n, **kw)
    graphed.reset_torch(); eager.reset_torch()
    acts = _actions(eager, T, 2)
    static_a = torch.empty((n, 2), device="cuda")
    static_i = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = dict(obs=torch.empty((n, graphed.obs_dim), device="cuda"), reward=torch.empty(n, device="cuda"),
               done=torch.empty(n, dtype=torch.uint8, device="cuda"), trunc=torch.empty(n, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warm = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(warm, stream=s):
            pass
    g = torch.cuda.CUDAGraph()
    before = torch.cuda.memory_allocated()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed.set_env_profiles(static_i)
            graphed.step_torch(static_a, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    gen = torch.Generator(device="cuda").manual_seed(5)
    for t in range(T):
        idx = torch.randint(0, P, (n,), device="cuda", generator=gen, dtype=torch.int32).to(torch.uint8)
        static_a.copy_(acts[t]); static_i.copy_(idx)
        g.replay()
        eager.set_env_profiles(idx.cpu().numpy())
        ob, rw, dn, tr = eager.step_torch(acts[t])
        torch.cuda.synchronize()
        for k, v in (("obs", ob), ("reward", rw), ("done", dn), ("trunc", tr)):
            assert torch.equal(out[k], v), (t, k)
        assert np.array_equal(graphed.env_profiles(), idx.cpu().numpy())
    graphed.check_status()
    graphed.close(); eager.close()


@pytest.mark.timeout(300)
def test_device_index_past_the_table_is_reported_and_uses_profile_0():
    import torch
    from space_gym_amd._native import NativeError
    n = 2000
    profs = [{"survival_reward_scale": 0.25}, {"survival_reward_scale": -1.0}, {"goal_sparse_reward": 3.0}]
    env = make("GoalContinuous2P-v0", n, seed=8, reward_profiles=profs)
    ref0 = make("GoalContinuous2P-v0", n, seed=8, **profs[0])
    idx = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    idx[::3] = 200
    idx[1::3] = 3
    env.set_env_profiles(idx)
    with pytest.raises(NativeError, match="profile"):
        env.check_status()
    env.check_status()  # (cleared)
    got = env.env_profiles()
    want = np.where(np.arange(n) % 3 == 2, 2, 0)
    assert np.array_equal(got, want)
    env.reset_torch(); ref0.reset_torch()
    a = _actions(env, 1, 0)[0]
    ob, rw, dn, tr = env.step_torch(a)
    rob, rrw, rdn, rtr = ref0.step_torch(a)
    rows = torch.as_tensor(want == 0, device="cuda")
    assert _same_rows(rw, rrw, rows) and _same_rows(ob, rob, rows)
    env.close(); ref0.close()


@pytest.mark.timeout(300)
def test_episode_returns_are_float64_sums_of_profiled_rewards():
    import torch
    n, T = 4000, 150
    profs = random_profiles("goal", 5, 31)
    env = make("GoalContinuous3P-v0", n, seed=2, max_episode_steps=40, reward_profiles=profs, episode_statistics=True)
    env.set_env_profiles(np.arange(n) % 5)
    env.reset_torch()
    acts = _actions(env, T, 6)
    er = dict(r=torch.zeros(n, dtype=torch.float64, device="cuda"), l=torch.zeros(n, dtype=torch.int32, device="cuda"))
    acc, length, checked = np.zeros(n), np.zeros(n, np.int64), 0
    for t in range(T):
        _, rw, dn, _ = env.step_torch(acts[t], episodes=er)
        r = rw.cpu().numpy().astype(np.float64)
        d = dn.bool().cpu().numpy()
        acc += r
        length += 1
        assert np.array_equal(er["r"].cpu().numpy()[d], acc[d]), t
        assert np.array_equal(er["l"].cpu().numpy()[d], length[d]), t
        checked += int(d.sum())
        acc[d] = 0.0
        length[d] = 0
    assert checked > n
    env.close()


@pytest.mark.timeout(300)
def test_normalization_of_profiled_rewards():
    import torch
    from normalize_model import NormalizeModel
    from test_gpu_normalize import assert_f32_close, assert_state_matches
    n, T = 5000, 60
    profs = random_profiles("kepler", 4, 12)
    idx = np.random.default_rng(0).integers(0, 4, n)
    env = make("KeplerCircleOrbit-v0", n, seed=4, max_episode_steps=25, reward_profiles=profs, normalize_obs=True, normalize_reward=True)
    twin = make("KeplerCircleOrbit-v0", n, seed=4, max_episode_steps=25, reward_profiles=profs)
    env.set_env_profiles(idx); twin.set_env_profiles(idx)
    model = NormalizeModel(n, env.obs_dim)
    assert_f32_close(env.reset_torch().cpu().numpy(), model.reset(twin.reset_torch().cpu().numpy()), "reset")
    acts = _actions(env, T, 3)
    for t in range(T):
        ob, rw, _, _ = env.step_torch(acts[t])
        rob, rrw, rdn, _ = twin.step_torch(acts[t])
        wo, wr, _ = model.step(rob.cpu().numpy(), rrw.cpu().numpy(), rdn.bool().cpu().numpy())
        assert_f32_close(ob.cpu().numpy(), wo, f"obs {t}")
        assert_f32_close(rw.cpu().numpy(), wr, f"reward {t}")
    assert_state_matches(env, model, "end")
    env.close(); twin.close()


@pytest.mark.timeout(300)
def test_resets_seed_and_masked_reset_keep_table_and_indices():
    import torch
    n = 1000
    profs = random_profiles("goal", 7, 2)
    env = make("GoalContinuous2P-v0", n, seed=1, reward_profiles=profs)
    idx = np.random.default_rng(3).integers(0, 7, n).astype(np.uint8)
    env.set_env_profiles(idx)
    eff = env.reward_profiles()
    env.reset_torch()
    env.reset_torch(mask=torch.rand(n, device="cuda") < 0.5)
    env.reset(mask=np.arange(n) % 2 == 0)
    env.seed(5)
    env.reset()
    assert np.array_equal(env.env_profiles(), idx)
    assert env.reward_profiles() == eff
    env.close()


@pytest.mark.timeout(300)
def test_snapshot_carries_profiles_and_off_is_unchanged():
    import torch
    from space_gym_amd._native import NativeError
    n = 3000
    profs = random_profiles("kepler", 6, 8)
    A = make("KeplerRandomOrbits-v0", n, seed=12, max_episode_steps=30, reward_profiles=profs)
    A.set_env_profiles(np.random.default_rng(1).integers(0, 6, n))
    A.reset_torch()
    acts = _actions(A, 80, 2)
    for t in range(40):
        A.step_torch(acts[t])
    blob = A.save_state()
    B = make("KeplerRandomOrbits-v0", n, seed=99, max_episode_steps=30)
    B.load_state(blob)
    assert B.reward_profiles() == A.reward_profiles()
    assert np.array_equal(B.env_profiles(), A.env_profiles())
    for t in range(40, 80):
        for x, y in zip(A.step_torch(acts[t]), B.step_torch(acts[t])):
            assert torch.equal(x, y), t
    assert np.array_equal(A.save_state(), B.save_state())
    # a blob whose index block names a profile past its table is refused before anything is switched on
    bad = blob.copy()
    bad[-1] = 200
    C0 = make("KeplerRandomOrbits-v0", n, seed=12, max_episode_steps=30)
    with pytest.raises(NativeError, match="past the snapshot"):
        C0.load_state(bad)
    assert C0.reward_profiles() == []
    C0.close()
    # profiles off: the blob is what a handle that never had them writes (header version 1)
    C, D = make("KeplerRandomOrbits-v0", n, seed=12), make("KeplerRandomOrbits-v0", n, seed=12)
    C.reset(); D.reset()
    C.set_reward_profiles(profs)
    C.set_reward_profiles(None)
    c, d = C.save_state(), D.save_state()
    assert np.array_equal(c, d) and C._snapshot_version(c) == 1
    for x in (A, B, C, D):
        x.close()


@pytest.mark.timeout(300)
def test_profiles_round_trip_and_errors():
    from space_gym_amd._native import NativeError
    n = 256
    env = make("GoalContinuous3P-v0", n, seed=0)
    own = env.native_params()
    assert env.reward_profiles() == []
    full = [dict(survival_reward_scale=0.1, goal_vel_reward_scale=0.7, safety_reward_scale=2.0, goal_sparse_reward=5.0, danger_zone=0.2),
            {"survival_reward_scale": -0.3}]
    env.set_reward_profiles(full)
    got = env.reward_profiles()
    assert got[0] == full[0]
    assert got[1]["survival_reward_scale"] == -0.3
    for k in ("goal_vel_reward_scale", "safety_reward_scale", "goal_sparse_reward", "danger_zone"):
        assert got[1][k] == own[k], k  # the handle's own values
    env.set_reward_profiles(got)
    assert env.reward_profiles() == got
    assert np.array_equal(env.env_profiles(), np.zeros(n, np.uint8))
    with pytest.raises(NativeError, match="KeplerEnv keyword"):
        env.set_reward_profiles([{"numerator_C": 0.1}])
    with pytest.raises(NativeError, match="danger_zone must not be negative"):
        env.set_reward_profiles([{}, {"danger_zone": -0.1}])
    assert env.reward_profiles() == got  # (a refused call changes nothing)
    env.set_env_profiles(np.ones(n, np.uint8))
    with pytest.raises(NativeError, match="past a table"):
        env.set_reward_profiles([{}])  # an index in use would point past the table
    env.set_reward_profiles([{}, {}, {}])  # indices kept
    assert np.array_equal(env.env_profiles(), np.ones(n, np.uint8))
    env.set_reward_profiles(None)
    assert env.reward_profiles() == []
    with pytest.raises(ValueError, match="off"):
        env.set_env_profiles(np.zeros(n, np.uint8))
    env.close()
    k = make("KeplerCircleOrbit-v0", n, seed=0)
    with pytest.raises(NativeError, match="GoalEnv keyword"):
        k.set_reward_profiles([{"survival_reward_scale": 1.0}])
    k.close()
