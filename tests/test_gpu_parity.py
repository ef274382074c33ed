"""GPU parity tests proper: the HIP engine, called through the C ABI (include/spacegym.h via ctypes), against
(1) the golden vectors captured from the reference and (2) the CPU oracle on the same seeded inputs.

Stated tolerances (fp32 engine vs fp64 reference):
    state, observation   1e-5 absolute          (theta compared modulo 2 pi)
    reward               1e-5 * max(1, |r|)     (the Goal reward multiplies position differences by 500..1000)
    done, goal-hit, event decisions: equal, except inputs within fp32 rounding of a boundary (none in the fixtures)
"""
import numpy as np
import pytest

from conftest import FAMILIES, has_gpu
from oracle import Oracle

pytestmark = pytest.mark.gpu

TOL_STATE = 1e-5
TOL_OBS = 1e-5
TOL_REWARD_REL = 1e-5


def circ_diff(a, b):
    d = np.abs(a - b) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def make(env_id, n, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def check_against(out_obs, out_rew, out_done, s1, ref_state1, ref_obs, ref_rew, ref_done, allow_mismatch=0):
    same = out_done == ref_done.astype(bool)
    assert (~same).sum() <= allow_mismatch, f"{(~same).sum()} done mismatches"
    s1 = s1.astype(np.float64)
    lin = [0, 1, 3, 4, 5]
    assert np.abs(s1[same][:, lin] - ref_state1[same][:, lin]).max() <= TOL_STATE
    assert circ_diff(s1[same][:, 2], ref_state1[same][:, 2]).max() <= TOL_STATE
    assert np.abs(out_obs[same] - ref_obs[same]).max() <= TOL_OBS
    rel = np.abs(out_rew[same] - ref_rew[same]) / np.maximum(1.0, np.abs(ref_rew[same]))
    assert rel.max() <= TOL_REWARD_REL, rel.max()


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_step_matches_reference_golden(fam, golden_steps):
    """Inject the fixture inputs, run ONE step without auto-reset, compare with what the reference produced."""
    d = golden_steps[fam]
    m = len(d["state0"])
    env = make(FAMILIES[fam], m, seed=1, auto_reset=False)
    env.reset()
    is_goal = "planets" in d
    env.set_state(ship=d["state0"], planets=d["planets"] if is_goal else None, goal=d["goal"] if is_goal else None,
                  elapsed=np.zeros(m, np.int32))
    obs, rew, done, info = env.step(d["action"])
    st = env.get_state()
    check_against(obs, rew, done, st["ship"], d["state1"], d["obs"], d["reward"], d["done"])
    assert not info["TimeLimit.truncated"].any()
    if is_goal:  # goal resampled exactly on the steps where the reference resampled it (goal.py:154-157)
        changed = np.any(st["goal"] != d["goal"].astype(np.float32), axis=1)
        assert np.array_equal(changed, d["goal_changed"].astype(bool))
    assert np.array_equal(st["elapsed"], np.ones(m, np.int32))
    assert env.discrete == ("discrete" in fam)
    env.close()


@pytest.mark.parametrize("env_id,n", [("GoalContinuous2P-v0", 4096), ("GoalContinuous3P-v0", 65536),
                                      ("KeplerCircleOrbit-v0", 65536), ("GoalContinuous4P-v0", 65536),
                                      ("KeplerEllipseHard-v0", 8192), ("KeplerRandomOrbits-v0", 16384)])
def test_rollout_steps_match_oracle(env_id, n):
    """BASELINE.json configs at full batch: engine-generated states (own reset + auto-reset rollout), every step
    re-checked against the oracle applied to the engine's own pre-step state."""
    env = make(env_id, n, seed=7, auto_reset=True)
    o = Oracle(env_id, threads=16)
    env.reset()
    rng = np.random.default_rng(11)
    is_goal = env.spec["family"] == "goal"
    for step in range(6):
        # let episodes age (auto-reset keeps every env valid), then verify one step in detail
        for _ in range(8 if step else 0):
            env.step(rng.uniform(-1, 1, size=(n, 2)).astype(np.float32))
        st = env.get_state()
        a = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        obs, rew, done, info = env.step(a)
        s1 = env.get_state()
        orbit = None
        if "Random" in env_id:  # per-env (angle, eccentricity); a = 1.2 for every id
            orbit = np.concatenate([st["goal"].astype(np.float64), np.full((n, 1), 1.2)], axis=1)
        ref = o.step(st["ship"].astype(np.float64), a, st["planets"].astype(np.float64) if is_goal else None,
                     st["goal"].astype(np.float64) if is_goal else None, orbit=orbit)
        trunc = info["TimeLimit.truncated"]
        ref_done = ref["done"].astype(bool) | trunc
        # finished envs were restarted inside the kernel: their last observation is in info["terminal_observation"],
        # and the 7 leading observation slots ARE the terminal state (x, y, cos, sin, vx, vy, omega)
        last_obs = np.where(done[:, None], info["terminal_observation"], obs)
        ship1 = s1["ship"].astype(np.float64)
        ship1[done] = ref["state1"][done]  # state of a restarted env is the new episode's; checked through last_obs
        # a handful of envs sit within fp32 rounding of an event boundary at this batch size
        check_against(last_obs, rew, done, ship1, ref["state1"], ref["obs"], ref["reward"], ref_done,
                      allow_mismatch=max(2, n // 20000))
        assert np.isfinite(obs).all() and np.isfinite(rew).all()
        assert (s1["elapsed"][done] == 0).all() and (s1["elapsed"][~done] == st["elapsed"][~done] + 1).all()
    env.close()


def test_invariants_full_batch():
    """Size-independent properties at B = 65536: theta in [0, 2pi], omega == 5 a1, a terminal state sits on
    a boundary, observation layout, finite rewards, restarted envs are inside the world and clear of every planet."""
    n = 65536
    env = make("GoalContinuous3P-v0", n, seed=3)
    env.reset()
    rng = np.random.default_rng(5)
    half = 1.5
    R = 0.75 * (2 * np.sqrt(3) * 3.0 / (3 * 7)) * np.sqrt(3) / 2  # hexagonal_tiling.py:37,45-47,173 for the 3x3 tiling
    n_done = 0
    for _ in range(120):
        a = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        planets0 = env.get_state()["planets"]
        obs, rew, done, info = env.step(a)
        st = env.get_state()
        ship = st["ship"]
        live = ~done
        assert (ship[:, 2] >= 0).all() and (ship[:, 2] <= np.float32(2 * np.pi)).all()
        assert np.array_equal(ship[live, 5], a[live, 1] * np.float32(5.0))  # dynamic_model.py:138-141
        assert np.array_equal(obs[:, :2], ship[:, :2]) and np.array_equal(obs[:, 4:7], ship[:, 3:6])
        assert np.allclose(obs[:, 2] ** 2 + obs[:, 3] ** 2, 1.0, atol=1e-5)
        assert np.isfinite(rew).all() and np.isfinite(obs).all()
        term = done & ~info["TimeLimit.truncated"]
        if term.any():  # terminal observation = state at the event (scipy ivp.py:689-692): on a planet or a wall
            tob = info["terminal_observation"][term]
            dist = np.linalg.norm(planets0[term] - tob[:, None, :2], axis=2)
            g = np.minimum(np.abs(dist - R).min(axis=1), np.abs(half - np.abs(tob[:, :2]).max(axis=1)))
            assert g.max() < 2e-6, g.max()
            assert np.array_equal(tob[:, 6], a[term, 1] * np.float32(5.0))
        if done.any():  # first state of the next episode
            s = ship[done]
            assert (np.abs(s[:, :2]) < half - R / 2 + 1e-5).all()
            clear = np.linalg.norm(st["planets"][done] - s[:, None, :2], axis=2).min(axis=1) - R
            assert (clear > 0).all()
            assert (np.abs(s[:, 5]) <= 4.2 + 1e-6).all() and (st["elapsed"][done] == 0).all()
        n_done += int(done.sum())
    assert n_done > n  # on average every env finished at least once
    env.close()


def test_time_limit_and_auto_reset():
    """gym TimeLimit semantics (max_episode_steps, gym_space/__init__.py:29) + VectorEnv auto-reset."""
    n, T = 4096, 5
    env = make("KeplerCircleOrbit-v0", n, seed=2, max_episode_steps=T, auto_reset=True)
    obs0 = env.reset()
    zero = np.zeros((n, 2), np.float32)
    zero[:, 0] = -1.0  # engine off
    for t in range(1, T + 1):
        obs, rew, done, info = env.step(zero)
        trunc = info["TimeLimit.truncated"]
        if t < T:
            assert not trunc.any()
            assert np.array_equal(env.get_state()["elapsed"][~done], np.full((~done).sum(), t, np.int32))
        else:
            assert np.array_equal(trunc | done, np.ones(n, bool)) and trunc.sum() > 0.9 * n
            st = env.get_state()
            assert (st["elapsed"] == 0).all()  # every env restarted
            assert np.allclose(obs[:, :2], st["ship"][:, :2])  # obs is the first observation of the new episode
            tob = info["terminal_observation"]
            assert np.isfinite(tob[trunc]).all()
            r = np.linalg.norm(st["ship"][:, :2], axis=1)
            assert (r >= 0.7 - 1e-5).all() and (r <= 2.5 + 1e-5).all()  # kepler.py:235-237
    # a different episode index gives a different start
    assert not np.allclose(obs0[:, :2], obs[:, :2])
    env.close()


@pytest.mark.parametrize("env_id", ["GoalContinuous2P-v0", "GoalContinuous3P-v0", "GoalContinuous4P-v0", "KeplerCircleOrbit-v0",
                                    "KeplerRandomOrbits-v0"])
def test_reset_matches_oracle_sampler(env_id):
    """Same counter-based RNG words on both sides: tile decisions are integer-exact, positions agree to fp32."""
    n = 8192
    env = make(env_id, n, seed=99, env_index_base=1000)
    obs = env.reset()
    st = env.get_state()
    o = Oracle(env_id)
    envs, oobs = o.vec_reset(n, seed=99, env_id0=1000)
    assert np.abs(st["ship"] - envs["state"]).max() < 2e-6
    assert np.abs(obs - oobs).max() < 5e-6
    if st["planets"] is not None:
        N = st["planets"].shape[1]
        assert np.abs(st["planets"] - envs["planets_xy"][:, :N]).max() < 2e-6
        assert np.abs(st["goal"] - envs["goal_xy"]).max() < 2e-6
    elif "Random" in env_id:
        assert np.abs(st["goal"] - envs["orbit"][:, :2]).max() < 2e-6  # (orbit angle, eccentricity) per env
    env.close()


def test_vector_env_trajectory_matches_oracle_vec_step():
    """Whole VectorEnv semantics (step + goal resample + TimeLimit + auto-reset) against the oracle's vec_step for
    100 steps from the same seed: states track within tolerance; envs whose discrete history diverged (an event
    decided differently within fp32 rounding) are excluded and must be very few."""
    env_id, n = "GoalContinuous3P-v0", 4096
    env = make(env_id, n, seed=5, max_episode_steps=40)
    o = Oracle(env_id, threads=8)
    o.params.max_episode_steps = 40
    obs = env.reset()
    envs, oobs = o.vec_reset(n, seed=5)
    rng = np.random.default_rng(1)
    ok = np.ones(n, bool)
    n_done = 0
    for t in range(100):
        a = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        obs, rew, done, info = env.step(a)
        oobs, orew, odone, otrunc = o.vec_step(envs, a, seed=5)
        ok &= (done == odone.astype(bool))
        ok &= np.abs(obs - oobs).max(axis=1) < 1e-4  # errors compound over steps; single-step parity is tested above
        assert np.array_equal(info["TimeLimit.truncated"][ok], otrunc.astype(bool)[ok])
        n_done += int(done.sum())
    assert n_done > n  # several generations of episodes went by
    assert ok.mean() > 0.99, ok.mean()
    env.close()


def test_device_tensor_path_matches_host_path():
    """sg_step_device on torch tensors (current stream) == sg_step on host arrays."""
    import torch
    n = 2048
    a = np.random.default_rng(0).uniform(-1, 1, size=(4, n, 2)).astype(np.float32)
    e1 = make("GoalContinuous3P-v0", n, seed=4)
    e2 = make("GoalContinuous3P-v0", n, seed=4)
    o1 = e1.reset()
    o2 = e2.reset_torch().cpu().numpy()
    assert np.array_equal(o1, o2)
    at = torch.from_numpy(a).cuda()
    K, D = 4, e2.obs_dim
    obs = torch.empty((K, n, D), device="cuda"); rew = torch.empty((K, n), device="cuda")
    done = torch.empty((K, n), dtype=torch.uint8, device="cuda"); trunc = torch.empty_like(done)
    e2.rollout_torch(at, obs, rew, done, trunc)
    torch.cuda.synchronize()
    for t in range(K):
        ob, rw, dn, info = e1.step(a[t])
        assert np.array_equal(ob, obs[t].cpu().numpy()) and np.array_equal(rw, rew[t].cpu().numpy())
        assert np.array_equal(dn, done[t].cpu().numpy().astype(bool))
    e1.close(); e2.close()


@pytest.mark.parametrize("env_id,host_out", [("GoalContinuous3P-v0", "fine"), ("KeplerDiscrete-v0", "fine"),
                                             ("GoalContinuous3P-v0", "coarse"), ("GoalContinuous3P-v0", "copy")])
def test_step_async_wait_pair_and_raw_begin_end(env_id, host_out, monkeypatch):
    """step_async() + step_wait() (sg_step_begin / sg_step_end: the step in two halves, its outputs in one of two page-locked
    blocks that alternate) against the one-call sg_step through raw ctypes: same outputs step for step incl. terminal
    observations; with copy=False the arrays of step t stay intact while step t + 1 is in flight; misuse raises.  All three
    ways the outputs can reach the host: stored by the step kernel into coherent (default) or non-coherent page-locked memory,
    or into a device block that is copied; with event counters on (which uses the device block) for the second half."""
    import ctypes as C
    n, K = 4096, 60
    rng = np.random.default_rng(3)
    monkeypatch.setenv("SPACEGYM_HOST_OUT", host_out)  # (read when the handle is created)
    env = make(env_id, n, seed=9, max_episode_steps=25, copy=False)
    ref = make(env_id, n, seed=9, max_episode_steps=25)
    D = env.obs_dim
    assert np.array_equal(env.reset(), ref.reset())
    with pytest.raises(RuntimeError):
        env.step_wait()
    prev = None
    n_done = 0
    for t in range(K):
        if t == K // 2:
            env.set_counters(True)
        a = rng.integers(0, 6, n).astype(np.int32) if env.discrete else rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        env.step_async(a)
        with pytest.raises(RuntimeError):
            env.step_async(a)
        # reference: the one-call entry point, host arrays, through raw ctypes
        o2, r2 = np.empty((n, D), np.float32), np.empty(n, np.float32)
        d2, t2, to2 = np.empty(n, np.uint8), np.empty(n, np.uint8), np.full((n, D), np.nan, np.float32)
        a2 = np.ascontiguousarray(a)
        rc = ref._lib.sg_step(ref._h, *[x.ctypes.data_as(C.c_void_p) for x in (a2, o2, r2, d2, t2, to2)])
        assert rc == 0
        if prev is not None:  # the previous step's arrays (views of the other block) are untouched by the step in flight
            assert all(np.array_equal(x, y) for x, y in zip(prev[0], prev[1]))
        obs, rew, done, info = env.step_wait()
        assert np.array_equal(obs, o2) and np.array_equal(rew, r2) and np.array_equal(done, d2.astype(bool))
        assert np.array_equal(info["TimeLimit.truncated"], t2.astype(bool))
        tobs = info["terminal_observation"]
        assert np.array_equal(tobs[done], to2[done]) and np.isnan(tobs[~done]).all()
        prev = ((obs, rew, done), (obs.copy(), rew.copy(), done.copy()))
        n_done += int(done.sum())
    assert n_done > n
    env.close(); ref.close()


@pytest.mark.parametrize("env_id", ["GoalContinuous2P-v0", "GoalContinuous3P-v0", "GoalContinuous4P-v0", "KeplerCircleOrbit-v0",
                                    "KeplerRandomOrbits-v0", "GoalDiscrete3-v0", "KeplerDiscrete-v0"])
def test_fused_rollout_equals_step_by_step(env_id):
    """sg_rollout_device (ONE launch for K steps, state in registers; Goal: next episodes pre-generated into a per-lane
    LDS queue by the one-lane reset, Kepler: restarts handed back through shuffles) is bit-identical to K launches of the
    step kernel (8-lane cooperative restart): outputs of every step and the final state, through several generations of
    episodes and goal resamples."""
    _fused_vs_step_by_step(env_id)


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_fused_rollout_kernels_kepler(kernel, monkeypatch):
    """Kepler: both rollout kernels against the step kernel, per-env random orbits, episodes of at most 40 steps"""
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", kernel)
    _fused_vs_step_by_step("KeplerRandomOrbits-v0", max_episode_steps=40)


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_fused_rollout_kernels_and_queue_depths(kernel, monkeypatch):
    """both rollout kernels (one wave per 64 envs | pilot + finisher wave pairs; the engine picks by grid size), with their
    episode queues, give the same bits as the step kernel, with episodes of at most 40 steps (3 % of the envs restart per
    step)"""
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", kernel)
    _fused_vs_step_by_step("GoalContinuous4P-v0", max_episode_steps=40)


def test_fused_rollout_restarts_every_step(monkeypatch):
    """max_episode_steps = 1: every env restarts in every step, so the pilot wave outruns the episode queue and generates
    its episodes itself"""
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", "pair")
    _fused_vs_step_by_step("GoalContinuous2P-v0", max_episode_steps=1, K=64, split=40)
    _fused_vs_step_by_step("KeplerEllipseHard-v0", max_episode_steps=1, K=64, split=40)


@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerEllipseEasy-v0"])
def test_fused_rollout_without_auto_reset(env_id):
    """auto_reset off: finished envs keep their terminal state (and keep being stepped from it); the wave-pair kernels then
    solve terminal events in the pilot wave and never touch the episode queue"""
    _fused_vs_step_by_step(env_id, K=120, split=50, auto_reset=False)


@pytest.mark.parametrize("n", [1, 1000])
def test_fused_rollout_ragged_batches(n):
    """batches that do not fill a workgroup (BASELINE's single-env plumbing case, and a last workgroup with idle lanes):
    both rollout kernels and the pair step kernel against the one-wave step kernel"""
    for env_id in ("GoalContinuous2P-v0", "KeplerCircleOrbit-v0"):
        _fused_vs_step_by_step(env_id, max_episode_steps=40, n=n)


def test_fused_rollout_more_workgroups_than_cus():
    """a grid with more wave-pair workgroups than CUs (they are resident one per CU at a time and take turns)"""
    _fused_vs_step_by_step("GoalContinuous3P-v0", max_episode_steps=30, K=96, split=40, n=70000)


def _fused_vs_step_by_step(env_id, max_episode_steps=120, K=300, split=100, auto_reset=True, n=8192):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(3)
    if "Discrete" in env_id:
        a = torch.randint(0, 6, (K, n), device="cuda", generator=gen, dtype=torch.int32)
    else:
        a = torch.rand((K, n, 2), device="cuda", generator=gen) * 2 - 1
    outs = []
    for mode in (0, 1):  # one K-step launch (default) | one launch per step
        env = make(env_id, n, seed=21, max_episode_steps=max_episode_steps, auto_reset=auto_reset)
        env.set_unfused_rollout(mode)
        env.reset_torch()
        D = env.obs_dim
        obs = torch.empty((K, n, D), device="cuda"); rew = torch.empty((K, n), device="cuda")
        done = torch.empty((K, n), dtype=torch.uint8, device="cuda"); trunc = torch.empty_like(done)
        env.rollout_torch(a[:split], obs[:split], rew[:split], done[:split], trunc[:split])   # two calls: state survives between them
        env.rollout_torch(a[split:], obs[split:], rew[split:], done[split:], trunc[split:])
        torch.cuda.synchronize()
        st = env.get_state()
        outs.append((obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), trunc.cpu().numpy(), st))
        env.close()
    (o1, r1, d1, t1, s1), (o2, r2, d2, t2, s2) = outs
    _assert_same_rollout(n, o1, r1, d1, t1, s1, o2, r2, d2, t2, s2, restarts=auto_reset)


@pytest.mark.parametrize("env_id", ["GoalContinuous2P-v0", "GoalContinuous3P-v0", "GoalContinuous4P-v0", "GoalDiscrete3-v0",
                                    "KeplerCircleOrbit-v0", "KeplerRandomOrbits-v0", "KeplerDiscrete-v0"])
def test_pair_step_kernel_equals_step_kernel(env_id, monkeypatch):
    """the one-launch-per-step kernel with pilot + finisher wave pairs (next episodes generated by the one-lane reset while
    the pilot integrates) gives the same bits as the one-wave kernel (8-lane cooperative restart): every output of every
    step incl. terminal observations, and the final state"""
    import torch
    n, K = 8192, 200
    rng = np.random.default_rng(9)
    acts = rng.integers(0, 6, (K, n)).astype(np.int32) if "Discrete" in env_id else rng.uniform(-1, 1, (K, n, 2)).astype(np.float32)
    outs = []
    for kernel in ("single", "pair"):
        monkeypatch.setenv("SPACEGYM_STEP_KERNEL", kernel)
        env = make(env_id, n, seed=33, max_episode_steps=60)
        o0 = env.reset()
        rec = [o0.copy()]
        for t in range(K):
            obs, rew, done, info = env.step(acts[t])
            rec += [obs.copy(), rew.copy(), done.copy(), info["TimeLimit.truncated"].copy(),
                    np.where(done[:, None], info["terminal_observation"], 0.0)]
        st = env.get_state()
        outs.append((rec, st))
        env.close()
    (r1, s1), (r2, s2) = outs
    assert sum(int(x.sum()) for x in r1[3::5]) > 2 * n  # restarts happened
    for k, (x, y) in enumerate(zip(r1, r2)):
        assert np.array_equal(x, y), f"record {k} (step {(k - 1) // 5}, field {(k - 1) % 5}) differs"
    for k in ("ship", "goal", "elapsed", "planets"):
        assert np.array_equal(s1[k], s2[k]), k


def _assert_same_rollout(n, o1, r1, d1, t1, s1, o2, r2, d2, t2, s2, restarts=True):
    assert (d1.sum() > 2 * n and t1.sum() > 0) if restarts else d1.sum() > 0  # restarts by events and by truncation happened
    for name, x, y in (("done", d1, d2), ("truncated", t1, t2), ("reward", r1, r2), ("obs", o1, o2)):
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            t0 = bad[:, 0].min()
            raise AssertionError(f"{name} differs first at step {t0}: {(bad[:, 0] == t0).sum()} entries; "
                                 f"envs {bad[bad[:, 0] == t0][:5, 1]}, done there fused/unfused "
                                 f"{d1[t0 - 1 if t0 else 0, bad[bad[:, 0] == t0][:5, 1]]}")
    for k in ("ship", "goal", "elapsed"):
        assert np.array_equal(s1[k], s2[k]), k
    if s1["planets"] is not None:
        assert np.array_equal(s1["planets"], s2["planets"])


def test_step_accepts_dlpack_actions():
    """step_torch takes any DLPack exporter zero-copy; outputs export DLPack themselves"""
    import torch

    class Foreign:  # stands in for a CuPy / JAX device array: only the DLPack protocol
        def __init__(self, t): self.t = t
        def __dlpack__(self, stream=None): return self.t.__dlpack__()
        def __dlpack_device__(self): return self.t.__dlpack_device__()

    n = 2048
    a = torch.rand((n, 2), device="cuda") * 2 - 1
    outs = []
    for wrap in (lambda x: x, Foreign):
        env = make("GoalContinuous3P-v0", n, seed=4)
        env.reset_torch()
        obs, rew, done, trunc = env.step_torch(wrap(a))
        torch.cuda.synchronize()
        outs.append((obs.clone(), rew.clone()))
        assert torch.equal(torch.from_dlpack(obs.__dlpack__()), obs)
        env.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_device_random_policy():
    """sg_random_actions_device: entry (t, i) is the documented function of (seed, global env index, step) -- checked against
    the oracle's Philox --, independent of sharding and of how the steps are cut into calls; uniform on (-1, 1) / on 0..5"""
    import torch
    o = Oracle("GoalContinuous3P-v0")
    n, K, seed = 4096, 64, 0x1234567890ABCDEF
    env = make("GoalContinuous3P-v0", n, seed=1)
    a = env.random_actions_torch(K, seed=seed).cpu().numpy()
    assert a.shape == (K, n, 2) and a.dtype == np.float32
    for t, i in [(0, 0), (1, 0), (2, 5), (63, 4095), (17, 1000)]:
        w = o.philox((seed & 0xFFFFFFFF, seed >> 32), (i, t >> 1, 0, 2))
        w0, w1 = (w[2], w[3]) if t & 1 else (w[0], w[1])
        exp = [np.float32(2.0 * (((x >> 9) + 0.5) / 8388608.0) - 1.0) for x in (w0, w1)]
        assert a[t, i, 0] == exp[0] and a[t, i, 1] == exp[1]
    assert np.abs(a).max() < 1.0 and abs(a.mean()) < 5e-3 and abs(a.var() - 1 / 3) < 5e-3
    assert abs(np.corrcoef(a[:-1].ravel(), a[1:].ravel())[0, 1]) < 5e-3
    b = torch.cat([env.random_actions_torch(40, seed=seed), env.random_actions_torch(24, seed=seed, first_step=40)]).cpu().numpy()
    assert np.array_equal(a, b)
    env.close()
    hi = make("GoalContinuous3P-v0", n // 2, seed=1, env_index_base=n // 2)
    assert np.array_equal(hi.random_actions_torch(K, seed=seed).cpu().numpy(), a[:, n // 2:])
    hi.close()
    d = make("GoalDiscrete3-v0", n, seed=1)
    k = d.random_actions_torch(K, seed=seed).cpu().numpy()
    assert k.shape == (K, n) and k.dtype == np.int32 and k.min() == 0 and k.max() == 5
    assert np.abs(np.bincount(k.ravel(), minlength=6) / k.size - 1 / 6).max() < 5e-3
    obs = torch.empty((K, n, d.obs_dim), device="cuda"); rew = torch.empty((K, n), device="cuda")
    done = torch.empty((K, n), dtype=torch.uint8, device="cuda"); trunc = torch.empty_like(done)
    d.reset_torch()
    d.rollout_torch(d.random_actions_torch(K, seed=seed), obs, rew, done, trunc)
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    d.close()


def test_sharding_is_invariant_to_the_split():
    """Two handles with env_index_base 0 and B/2 reproduce one handle of B envs bit for bit (RNG keyed by global index)."""
    n = 4096
    full = make("GoalContinuous4P-v0", n, seed=8)
    lo = make("GoalContinuous4P-v0", n // 2, seed=8, env_index_base=0)
    hi = make("GoalContinuous4P-v0", n // 2, seed=8, env_index_base=n // 2)
    assert np.array_equal(full.reset(), np.concatenate([lo.reset(), hi.reset()]))
    rng = np.random.default_rng(2)
    for _ in range(60):
        a = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        of, rf, df, _ = full.step(a)
        ol, rl, dl, _ = lo.step(a[: n // 2])
        oh, rh, dh, _ = hi.step(a[n // 2:])
        assert np.array_equal(of, np.concatenate([ol, oh])) and np.array_equal(rf, np.concatenate([rl, rh]))
        assert np.array_equal(df, np.concatenate([dl, dh]))
    for e in (full, lo, hi):
        e.close()


def test_step_device_is_graph_capturable():
    """sg_step_device only enqueues a kernel on the given stream (no allocation, copy or sync), so it can be captured
    into a HIP graph and replayed; replays equal eager launches."""
    import torch
    n = 4096
    a = (torch.rand((6, n, 2), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 2 - 1)
    eager, graphed = make("GoalContinuous3P-v0", n, seed=9), make("GoalContinuous3P-v0", n, seed=9)
    eager.reset_torch(); graphed.reset_torch()
    torch.cuda.synchronize()
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
    # the capture itself does not execute the kernel: replay steps 0..5
    for t in range(6):
        static_a.copy_(a[t])
        g.replay()
        torch.cuda.synchronize()
        ob, rw, dn, tr = eager.step_torch(a[t].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(out["obs"], ob) and torch.equal(out["reward"], rw) and torch.equal(out["done"], dn)
    eager.close(); graphed.close()


def test_random_orbits_match_reference_golden():
    """Per-env orbits injected through set_state(goal=(angle, eccentricity)); outputs against the reference fixture."""
    from conftest import load_golden
    d = load_golden("step_kepler_random")
    m = len(d["state0"])
    env = make("KeplerRandomOrbits-v0", m, seed=1, auto_reset=False)
    env.reset()
    env.set_state(ship=d["state0"], goal=d["orbit"][:, :2], elapsed=np.zeros(m, np.int32))
    obs, rew, done, info = env.step(d["action"])
    check_against(obs, rew, done, env.get_state()["ship"], d["state1"], d["obs"], d["reward"], d["done"])
    env.close()


@pytest.mark.parametrize("fam,env_id", [("goal3p_accel", "GoalContinuous3P-v0"), ("kepler_circle_accel", "KeplerCircleOrbit-v0")])
def test_acceleration_steering_matches_reference_golden(fam, env_id):
    """Steering.acceleration through sg_config.steering = 1: fixtures from the reference with ship_steering=0."""
    from conftest import load_golden
    d = load_golden("step_" + fam)
    m = len(d["state0"])
    env = make(env_id, m, seed=1, auto_reset=False, steering="acceleration")
    env.reset()
    is_goal = "planets" in d
    env.set_state(ship=d["state0"], planets=d["planets"] if is_goal else None, goal=d["goal"] if is_goal else None,
                  elapsed=np.zeros(m, np.int32))
    obs, rew, done, info = env.step(d["action"])
    check_against(obs, rew, done, env.get_state()["ship"], d["state1"], d["obs"], d["reward"], d["done"])
    env.close()
    # and the rollout kernel == step kernel in this mode too, with omega carried between steps
    import torch
    n, K = 4096, 150
    a = torch.rand((K, n, 2), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 2 - 1
    outs = []
    for mode in (0, 1):
        env = make(env_id, n, seed=2, steering="acceleration")
        env.set_unfused_rollout(mode)
        env.reset_torch()
        obs = torch.empty((K, n, env.obs_dim), device="cuda"); rew = torch.empty((K, n), device="cuda")
        dn = torch.empty((K, n), dtype=torch.uint8, device="cuda"); tr = torch.empty_like(dn)
        env.rollout_torch(a, obs, rew, dn, tr)
        torch.cuda.synchronize()
        outs.append((obs.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy(), env.get_state()["ship"]))
        env.close()
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x, y)
    assert outs[0][2].sum() > n // 2


def test_integration_md_stub_runs_as_written():
    """INTEGRATION.md shows the ctypes stub a maintainer of the reference would add; execute that very code block against
    the built library and compare with the package's own front end."""
    import os, re
    from conftest import ROOT
    from space_gym_amd import _native
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = re.search(r"```python\n(# gym_space/vector_hip.py.*?)```", md, re.S).group(1)
    ns = {}
    exec(compile(block, "INTEGRATION.md", "exec"), ns)
    n = 1024
    stub = ns["HipVectorEnv"]("GoalContinuous3P-v0", n, lib=_native.LIB_PATH, seed=5)
    ours = make("GoalContinuous3P-v0", n, seed=5)
    assert np.array_equal(stub.reset(), ours.reset())
    a = np.random.default_rng(0).uniform(-1, 1, size=(n, 2)).astype(np.float32)
    o1, r1, d1, i1 = stub.step(a)
    o2, r2, d2, i2 = ours.step(a)
    assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2)
    assert np.array_equal(i1["TimeLimit.truncated"], i2["TimeLimit.truncated"])
    stub.close(); ours.close()
    # the constructor-kwargs block of the same section, as written: sg_params_init + sg_create_ex
    import ctypes as C
    block2 = re.search(r"```python\n(class _Params\(C.Structure\).*?)```", md, re.S).group(1)
    exec(compile(block2, "INTEGRATION.md", "exec"), ns)
    lib = C.CDLL(_native.LIB_PATH)
    cfg = ns["_Cfg"](b"KeplerCircleOrbit-v0", 256, 3, 0, 0, 1, 0)
    kw = dict(ref_orbit_a=1.5, ref_orbit_eccentricity=0.3, ref_orbit_angle=2.0, step_size=0.1, max_engine_force=0.6)
    h = ns["create"](lib, cfg, 0, **kw)
    got = ns["_Params"]()
    lib.sg_get_params.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.sg_get_params(h, C.byref(got)) == 0
    for k, v in kw.items():
        assert abs(getattr(got, k) - v) < 1e-6, (k, getattr(got, k))
    lib.sg_destroy.argtypes = [C.c_void_p]
    lib.sg_destroy(h)
    with pytest.raises(RuntimeError, match="GoalEnv keyword"):
        ns["create"](lib, cfg, 0, danger_zone=0.3)  # a GoalEnv keyword for a Kepler id is refused


def test_vector_field_matches_reference():
    """sg_vector_field against SpaceshipEnv.vector_field outputs captured from the reference."""
    from conftest import load_golden
    d = load_golden("vector_field")
    m = len(d["goal3p_state"])
    env = make("GoalContinuous3P-v0", m, seed=1)
    env.reset()
    env.set_state(ship=d["goal3p_state"], planets=d["goal3p_planets"])
    assert np.abs(env.vector_field(d["goal3p_action"]) - d["goal3p_field"]).max() < 1e-6
    assert np.abs(env.vector_field(d["goal3p_action"], ship=d["goal3p_state"]) - d["goal3p_field"]).max() < 1e-6
    env.close()
    env = make("KeplerEllipseEasy-v0", m, seed=1)
    env.reset()
    assert np.abs(env.vector_field(d["kepler_easy_action"], ship=d["kepler_easy_state"]) - d["kepler_easy_field"]).max() < 1e-6
    env.close()


def test_bench_line_contract():
    """bench.py prints ONE JSON line with the driver's keys plus `roofline` and `cpu_baseline` (tiny sizes here); the metric
    names the workload that ran"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "64", "--warmup", "8", "--preroll", "16",
                          "--batch", "4096", "--cpu-seconds", "0.5"], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    b = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "roofline_one_launch_per_step", "host_numpy_path"):
        assert k in b, k
    assert b["metric"] == "env-steps/sec at batch=4096, GoalContinuous3P-v0, 1/2/4/8 MI355X"
    assert b["steps"] == 64 and b["warmup"] == 8 and b["n_gpus"] == 1 and b["unit"] == "env-steps/s" and b["higher_is_better"]
    assert abs(b["value"] - 4096 * 64 / (b["ms_per_step"] * 64e-3)) / b["value"] < 1e-6
    r = b["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["kernel"].startswith("goal_pair_rollout_kernel<3") and r["steps_per_launch"] == 64
    assert r["traffic"] is None  # no PMC profile of this workload is committed: nothing is borrowed from another one
    u = b["roofline_one_launch_per_step"]
    assert u["kernel"].startswith("goal_pair_step_kernel<3") and u["launches"] == 64
    c = b["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "env-steps/s"
    assert c["single_core"]["cores"] == 1 and 0 < c["single_core"]["value"] <= c["value"] * 1.5


def test_bench_dump_outputs_are_reproducible(tmp_path):
    """bench.py --dump-outputs DIR: the last timed step's (obs, reward, done, truncated) of every env; two runs with the same
    arguments write the same arrays (the timed steps span several rollout calls here: --chunk below --steps)"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, dumps = 4096, []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "40", "--warmup", "4", "--preroll", "16",
                              "--chunk", "16", "--repeats", "2", "--batch", str(B), "--no-cpu-baseline", "--no-host-path",
                              "--no-graph", "--dump-outputs", d], capture_output=True, text=True, timeout=300, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == 40
        dumps.append({k: np.load(os.path.join(d, k + ".npy")) for k in ("obs", "reward", "done", "truncated", "env_index")})
    a, b = dumps
    assert np.array_equal(a["env_index"], np.arange(B)) and a["obs"].shape == (B, 15)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["reward"]).all()
    assert (np.abs(a["obs"][:, 2] ** 2 + a["obs"][:, 3] ** 2 - 1) < 1e-5).all()  # (cos, sin) of the ship's angle
    assert set(np.unique(a["done"])) <= {0.0, 1.0} and set(np.unique(a["truncated"])) <= {0.0, 1.0}


@pytest.mark.parametrize("name", ["goal_a", "goal_b", "goal_c", "kepler_a", "kepler_b", "kepler_c", "kepler_d"])
def test_constructor_kwargs_match_reference_golden(name):
    """sg_create_ex / make_vec(env_id, **kwargs): the reference's constructor kwargs (goal.py:18-31, kepler.py:189-203) beyond
    what the ids register -- fixtures from the unmodified reference (tools/gen_golden.py --stage kwargs); the env-steps of 0.1
    (KeplerEnv's own default) go through the Dormand-Prince kernels, those up to 0.072 through the fast step."""
    import json
    from conftest import load_golden
    import space_gym_amd as sg
    d = load_golden("step_kw_" + name)
    kw = json.loads(str(d["kwargs_json"]))
    m = len(d["state0"])
    env = sg.make_vec(str(d["env_id"]), m, device=0, seed=1, auto_reset=False, from_class=True, **kw)
    p = env.native_params()
    for k, v in kw.items():  # the handle holds what was asked for
        if k in p:
            assert abs(p[k] - float(v)) < 1e-6 * max(1.0, abs(float(v))), (k, p[k], v)
    assert abs(p["step_size"] - float(d["const_step_size"])) < 1e-7
    env.reset()
    is_goal = "planets" in d
    assert env.obs_dim == d["obs"].shape[1] and env.n_planets == (int(d["const_n_planets"]) if is_goal else 0)
    env.set_state(ship=d["state0"], planets=d["planets"] if is_goal else None, goal=d["goal"] if is_goal else None,
                  elapsed=np.zeros(m, np.int32))
    obs, rew, done, info = env.step(d["action"])
    st = env.get_state()
    check_against(obs, rew, done, st["ship"], d["state1"], d["obs"], d["reward"], d["done"])
    if is_goal:
        changed = np.any(st["goal"] != d["goal"].astype(np.float32), axis=1)
        assert np.array_equal(changed, d["goal_changed"].astype(bool))
    env.close()
    # the same parameters through K-step rollouts (wave-pair kernels) against one-launch-per-step: bit-identical
    import torch
    n, K = 4096, 48
    envs = [sg.make_vec(str(d["env_id"]), n, device=0, seed=3, from_class=True, max_episode_steps=40, **kw) for _ in range(2)]
    a = torch.rand((K, n, 2), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 2 - 1
    outs = []
    for k, e in enumerate(envs):
        e.reset_torch()
        e.set_unfused_rollout(k == 1)
        o = torch.empty((K, n, e.obs_dim), device="cuda"); r = torch.empty((K, n), device="cuda")
        dn = torch.empty((K, n), dtype=torch.uint8, device="cuda"); tr = torch.empty_like(dn)
        e.rollout_torch(a, o, r, dn, tr)
        e.check_status()
        outs.append((o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy(), tr.cpu().numpy()))
        e.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    assert outs[0][2].sum() > 0
