"""GPU tests of the masked reset (sg_reset_masked*, reset(mask=...) / reset_torch(mask=...)).  The core oracle: with auto_reset
off, step_torch followed by reset_torch(mask=done) is bit for bit what a twin with auto_reset on returns -- the masked reset runs
the step kernels' own restart code for the episode auto-reset would start.  Around it: an all-ones mask against a full reset,
untouched unmasked envs, the rollout kernels' episode queue, episode statistics, normalization, rendering, snapshots, graph
capture, errors and the NumPy route."""
import numpy as np
import pytest

from normalize_model import NormalizeModel

pytestmark = pytest.mark.gpu

IDENTITY_CASES = [("GoalContinuous2P-v0", None), ("GoalContinuous3P-v0", None), ("GoalContinuous4P-v0", None),
                  ("GoalContinuous3P-v0", "acceleration"), ("GoalDiscrete3-v0", None), ("KeplerRandomOrbits-v0", None),
                  ("KeplerCircleOrbit-v0", None)]
SERVED = ["GoalContinuous2P-v0", "GoalContinuous3P-v0", "GoalContinuous4P-v0", "GoalDiscrete2-v0", "GoalDiscrete3-v0",
          "GoalDiscrete4-v0", "KeplerCircleOrbit-v0", "KeplerEllipseEasy-v0", "KeplerEllipseHard-v0", "KeplerRandomOrbits-v0",
          "KeplerDiscrete-v0"]


def make(env_id, n, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _actions(env, K, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if env.discrete:
        return torch.randint(0, 6, (K, env.num_envs), device="cuda", generator=gen, dtype=torch.int32)
    return torch.rand((K, env.num_envs, 2), device="cuda", generator=gen) * 2 - 1


def _random_mask(n, p, seed):
    import torch
    return torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) < p


def _np(t):
    return t.cpu().numpy()


def _assert_states_equal(a, b, what, rows=None):
    sa, sb = a.get_state(), b.get_state()
    for k in ("ship", "planets", "goal", "elapsed"):
        if sa.get(k) is None:
            assert sb.get(k) is None, (what, k)
            continue
        x, y = (sa[k], sb[k]) if rows is None else (sa[k][rows], sb[k][rows])
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y), (what, k)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [1000, 131072])
@pytest.mark.parametrize("env_id,steering", IDENTITY_CASES)
def test_masked_reset_of_done_envs_is_auto_reset(env_id, steering, n):
    """twin A (auto_reset on) against twin B (auto_reset off, step_torch then reset_torch(mask=done)), 120 steps of 40-step
    episodes: obs, reward, done, truncated and every state column bit for bit after every step; A's terminal observations are
    B's step rows of the finished envs"""
    import torch
    kw = dict(seed=17, max_episode_steps=40, **(dict(steering=steering) if steering else {}))
    A, B = make(env_id, n, auto_reset=True, **kw), make(env_id, n, auto_reset=False, **kw)
    assert torch.equal(A.reset_torch(), B.reset_torch())
    acts = _actions(A, 120, seed=5)
    tobs = torch.empty((n, A.obs_dim), device="cuda")
    finished = 0
    for t in range(120):
        tobs.fill_(float("nan"))
        oa, ra, da, ta = A.step_torch(acts[t], terminal_obs=tobs)
        ob, rb, db, tb = B.step_torch(acts[t])
        d = db.bool()
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ta, tb), t
        assert torch.equal(tobs[d], ob[d]), t  # the episode's last observation
        B.reset_torch(mask=db)  # into B's own obs tensor: the rows of the finished envs
        assert torch.equal(oa, ob), t
        finished += int(d.sum())
        if t % 10 == 9 or n <= 1000:
            _assert_states_equal(A, B, f"{env_id} step {t}")
    _assert_states_equal(A, B, "end")
    assert finished > n  # every env went through several episodes
    A.check_status(); B.check_status()
    A.close(); B.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("env_id", SERVED)
def test_all_ones_mask_is_a_full_reset(env_id):
    import torch
    n = 3000
    A, B = make(env_id, n, seed=8), make(env_id, n, seed=8)
    A.reset_torch(); B.reset_torch()
    for a in _actions(A, 7, seed=1):  # mid-episode
        A.step_torch(a); B.step_torch(a)
    oa = A.reset_torch(mask=torch.ones(n, dtype=torch.bool, device="cuda"))
    ob = B.reset_torch()
    assert torch.equal(oa, ob)
    _assert_states_equal(A, B, env_id)
    assert np.array_equal(A.save_state(), B.save_state())  # every column, episode counters and tiling state included
    A.close(); B.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_unmasked_envs_are_untouched(env_id):
    """NaN rows of unmasked envs stay NaN, their state does not change, and their next 50 steps equal those of a twin that got
    an empty mask"""
    import torch
    n = 5000  # (ragged: the last workgroup and wave are partial)
    A, B = make(env_id, n, seed=4, max_episode_steps=60), make(env_id, n, seed=4, max_episode_steps=60)
    A.reset_torch(); B.reset_torch()
    acts = _actions(A, 65, seed=2)
    for t in range(15):
        A.step_torch(acts[t]); B.step_torch(acts[t])
    before = A.get_state()
    mask = _random_mask(n, 0.1, seed=3)
    keep = ~_np(mask)
    oa = torch.full((n, A.obs_dim), float("nan"), device="cuda")
    ob = torch.full((n, B.obs_dim), float("nan"), device="cuda")
    A.reset_torch(out=oa, mask=mask)
    B.reset_torch(out=ob, mask=torch.zeros(n, dtype=torch.uint8, device="cuda"))
    assert torch.isnan(oa[~mask]).all() and not torch.isnan(oa[mask]).any()
    assert torch.isnan(ob).all()
    after = A.get_state()
    for k in ("ship", "planets", "goal", "elapsed"):
        if before.get(k) is not None:
            assert np.array_equal(before[k][keep], after[k][keep]), k
    assert (after["elapsed"][~keep] == 0).all()
    _assert_states_equal(A, B, "empty mask", rows=keep)
    assert np.array_equal(before["ship"], B.get_state()["ship"])  # an empty mask changes nothing
    for t in range(15, 65):
        ra, rb = A.step_torch(acts[t]), B.step_torch(acts[t])
        for x, y in zip(ra, rb):
            assert torch.equal(x[~mask], y[~mask]), t
    A.close(); B.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("plan", ["pair", "single", "unfused"])
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_rollout_after_a_masked_reset_equals_steps(env_id, plan, monkeypatch):
    """the rollout kernels' episode queue is emptied for the masked envs: a K=50 rollout after a masked reset equals a twin's
    step_torch loop after the same masked reset"""
    import torch
    n, K = 8192, 50
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", "single" if plan == "single" else "pair")
    A, B = make(env_id, n, seed=6, max_episode_steps=30), make(env_id, n, seed=6, max_episode_steps=30)
    if plan == "unfused":
        A.set_unfused_rollout(True)
    A.reset_torch(); B.reset_torch()
    acts = _actions(A, 2 * K, seed=9)
    D = A.obs_dim

    def bufs():
        return (torch.empty((K, n, D), device="cuda"), torch.empty((K, n), device="cuda"),
                torch.empty((K, n), dtype=torch.uint8, device="cuda"), torch.empty((K, n), dtype=torch.uint8, device="cuda"))
    A.rollout_torch(acts[:K].contiguous(), *bufs())  # (fills the episode queue)
    for t in range(K):
        B.step_torch(acts[t])
    mask = _random_mask(n, 0.1, seed=4)
    A.reset_torch(mask=mask); B.reset_torch(mask=mask)
    out = bufs()
    A.rollout_torch(acts[K:].contiguous(), *out)
    for t in range(K):
        ob, rb, db, tb = B.step_torch(acts[K + t])
        for x, y in zip((ob, rb, db, tb), out):
            assert torch.equal(x, y[t]), (plan, t)
    _assert_states_equal(A, B, plan)
    A.check_status()
    A.close(); B.close()


@pytest.mark.timeout(300)
def test_episode_statistics_restart_for_masked_envs():
    """masked sums go back to zero and the abandoned episode leaves no record; the returns of later episodes are bit for bit
    a float64 loop over the float32 rewards"""
    import torch
    n = 4096
    env = make("GoalContinuous3P-v0", n, seed=11, auto_reset=False, max_episode_steps=40, episode_statistics=True)
    env.reset_torch()
    acts = _actions(env, 90, seed=3)
    ret, length = np.zeros(n), np.zeros(n, np.int64)
    rows = dict(r=torch.empty(n, dtype=torch.float64, device="cuda"), l=torch.empty(n, dtype=torch.int32, device="cuda"))
    finished = forced = 0
    for t in range(90):
        rows["r"].fill_(float("nan")); rows["l"].fill_(-1)
        _, rw, dn, _ = env.step_torch(acts[t], episodes=rows)
        r, d = _np(rw), _np(dn).astype(bool)
        ret += r.astype(np.float64)  # (one float64 add per step, in step order)
        length += 1
        assert np.array_equal(_np(rows["r"])[d].view(np.uint64), ret[d].view(np.uint64)), t
        assert np.array_equal(_np(rows["l"])[d], length[d]), t
        assert np.isnan(_np(rows["r"])[~d]).all() and (_np(rows["l"])[~d] == -1).all()
        finished += int(d.sum())
        extra = _np(_random_mask(n, 0.03, seed=100 + t)) if t % 3 == 0 else np.zeros(n, bool)
        m = d | extra
        forced += int((extra & ~d).sum())
        ret[m] = 0.0
        length[m] = 0
        env.reset_torch(mask=torch.as_tensor(m, device="cuda"))
    assert finished > 0 and forced > 0
    env.close()


def _norm_tools():
    from test_gpu_normalize import assert_f32_close, assert_state_matches
    return assert_f32_close, assert_state_matches


@pytest.mark.timeout(600)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_normalization_sees_the_masked_rows_only(env_id):
    """the observation statistics are updated with RunningMeanStd.update(obs_raw[mask]) and the masked rows are normalized with
    the result; unmasked rows, returns and the return statistics stay; an empty mask changes no bit; update=False freezes"""
    import torch
    assert_f32_close, assert_state_matches = _norm_tools()
    n = 5000
    env = make(env_id, n, seed=13, auto_reset=False, max_episode_steps=30, normalize_obs=True, normalize_reward=True)
    twin = make(env_id, n, seed=13, auto_reset=False, max_episode_steps=30)
    model = NormalizeModel(n, env.obs_dim)
    assert_f32_close(_np(env.reset_torch()), model.reset(_np(twin.reset_torch())), "reset")
    acts = _actions(env, 60, seed=7)
    for t in range(60):
        ob, rw, dn, _ = env.step_torch(acts[t])
        rob, rrw, rdn, _ = twin.step_torch(acts[t])
        d = _np(rdn).astype(bool)
        wo, wr, _ = model.step(_np(rob), _np(rrw), d)
        assert_f32_close(_np(ob), wo, f"obs {t}")
        assert_f32_close(_np(rw), wr, f"reward {t}")
        if t == 20:
            m = np.zeros(n, bool)
        elif t == 40:
            m = _np(_random_mask(n, 0.2, seed=t)) | d
        else:
            m = d
        before = env.normalizer_state()
        prev = _np(ob).copy()
        mt = torch.as_tensor(m, device="cuda")
        got = _np(env.reset_torch(mask=mt))
        raw = _np(twin.reset_torch(mask=mt))
        after = env.normalizer_state()
        if m.any():
            model.obs_rms.update(raw[m])
        assert float(after["obs_count"]) == float(before["obs_count"]) + int(m.sum()), t  # exactly the masked rows
        for k in ("ret_mean", "ret_var", "ret_count", "returns"):
            assert np.array_equal(before[k], after[k]), (t, k)
        if not m.any():
            for k in before:
                assert np.array_equal(before[k], after[k]), (t, k)  # no update at all, no NaN
        assert np.array_equal(got[~m], prev[~m]), t
        assert_f32_close(got[m], model.norm_obs(raw[m]), f"masked rows {t}")
        assert_state_matches(env, model, f"reset {t}")
    # frozen: only normalize
    env.set_normalization(update=False)
    before = env.normalizer_state()
    m = np.zeros(n, bool); m[::7] = True
    mt = torch.as_tensor(m, device="cuda")
    got, raw = _np(env.reset_torch(mask=mt)), _np(twin.reset_torch(mask=mt))
    after = env.normalizer_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert_f32_close(got[m], model.norm_obs(raw[m]), "frozen")
    env.close(); twin.close()


@pytest.mark.timeout(300)
def test_render_traces_restart_for_masked_envs_only():
    """after a masked reset of env 1: its frames equal those of a twin that reset every env (its trace starts afresh there as
    well); the frames of the other envs equal those of a twin without any reset"""
    import torch
    env_id, n = "GoalContinuous3P-v0", 64
    kw = dict(seed=21, render=dict(capacity=4))
    A, B, C = make(env_id, n, **kw), make(env_id, n, **kw), make(env_id, n, **kw)
    for e in (A, B, C):
        e.reset_torch()
    ids = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    acts = _actions(A, 12, seed=5)
    for t in range(6):
        fa, fb, fc = (e.render_torch(ids, actions=acts[t], size=64) for e in (A, B, C))
        assert torch.equal(fa, fb) and torch.equal(fa, fc)
        for e in (A, B, C):
            e.step_torch(acts[t])
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mask[1] = 1
    A.reset_torch(mask=mask)
    C.reset_torch()
    for t in range(6, 12):
        fa, fb, fc = (e.render_torch(ids, actions=acts[t], size=64) for e in (A, B, C))
        assert torch.equal(fa[1], fc[1]), t
        for k in (0, 2, 3):
            assert torch.equal(fa[k], fb[k]), (t, k)
        for e in (A, B, C):
            e.step_torch(acts[t])
    A.check_status()
    A.close(); B.close(); C.close()


@pytest.mark.timeout(300)
def test_snapshot_right_after_a_masked_reset_resumes():
    import torch
    n = 4096
    kw = dict(seed=2, max_episode_steps=25, episode_statistics=True)
    A = make("GoalContinuous4P-v0", n, **kw)
    A.reset_torch()
    acts = _actions(A, 40, seed=1)
    for t in range(10):
        A.step_torch(acts[t])
    A.reset_torch(mask=_random_mask(n, 0.3, seed=8))
    blob = A.save_state()
    F = make("GoalContinuous4P-v0", n, seed=77, max_episode_steps=25)
    F.load_state(blob)
    ra_rows = dict(r=torch.empty(n, dtype=torch.float64, device="cuda"), l=torch.empty(n, dtype=torch.int32, device="cuda"))
    rf_rows = dict(r=torch.empty(n, dtype=torch.float64, device="cuda"), l=torch.empty(n, dtype=torch.int32, device="cuda"))
    for t in range(10, 40):
        for r in (ra_rows, rf_rows):
            r["r"].fill_(0.0); r["l"].fill_(0)
        oa = [x.clone() for x in A.step_torch(acts[t], episodes=ra_rows)]
        of = F.step_torch(acts[t], episodes=rf_rows)
        for x, y in zip(oa, of):
            assert torch.equal(x, y), t
        assert torch.equal(ra_rows["r"], rf_rows["r"]) and torch.equal(ra_rows["l"], rf_rows["l"]), t
    assert np.array_equal(A.save_state(), F.save_state())
    A.close(); F.close()


@pytest.mark.timeout(300)
def test_graph_of_step_and_masked_reset_equals_eager():
    """one graph holds step_torch + reset_torch(mask=done) with auto_reset off, captured on one stream; its replays equal the
    eager loop, and the capture allocates nothing"""
    import torch
    n, T = 8192, 30
    kw = dict(seed=7, auto_reset=False, max_episode_steps=12)
    graphed, eager = make("GoalContinuous3P-v0", n, **kw), make("GoalContinuous3P-v0", n, **kw)
    graphed.reset_torch(); eager.reset_torch()
    acts = _actions(eager, T, seed=2)
    static_a = torch.empty((n, 2), device="cuda")
    out = dict(obs=torch.empty((n, graphed.obs_dim), device="cuda"), reward=torch.empty(n, device="cuda"),
               done=torch.empty(n, dtype=torch.uint8, device="cuda"), trunc=torch.empty(n, dtype=torch.uint8, device="cuda"))
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
            graphed.step_torch(static_a, out=out)
            graphed.reset_torch(out=out["obs"], mask=out["done"])
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    finished = 0
    for t in range(T):
        static_a.copy_(acts[t])
        g.replay()
        ob, rw, dn, tr = eager.step_torch(acts[t])
        eager.reset_torch(mask=dn)
        torch.cuda.synchronize()
        for k, v in (("obs", ob), ("reward", rw), ("done", dn), ("trunc", tr)):
            assert torch.equal(out[k], v), (t, k)
        finished += int(dn.sum())
    assert finished > n
    _assert_states_equal(graphed, eager, "graph")
    graphed.check_status()
    graphed.close(); eager.close()


@pytest.mark.timeout(300)
def test_errors_and_the_numpy_route():
    import torch
    from space_gym_amd._native import NativeError
    n = 2048
    env = make("GoalContinuous3P-v0", n, seed=1, auto_reset=False, max_episode_steps=20)
    ones = torch.ones(n, dtype=torch.bool, device="cuda")
    with pytest.raises(NativeError, match="sg_reset first"):
        env.reset_torch(mask=ones)  # fresh after create
    with pytest.raises(NativeError, match="sg_reset first"):
        env.reset(mask=np.ones(n, bool))
    env.reset_torch()
    env.seed(5)
    with pytest.raises(NativeError, match="sg_reset first"):
        env.reset_torch(mask=ones)  # fresh after seed
    for bad in (torch.ones(n + 1, dtype=torch.bool, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda"),
                torch.ones(n, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask"):
            env.reset_torch(mask=bad)
    with pytest.raises(ValueError, match="mask"):
        env.reset(mask=np.ones(n - 1, bool))
    # the NumPy route equals the torch route
    tw = make("GoalContinuous3P-v0", n, seed=5, auto_reset=False, max_episode_steps=20)
    assert np.array_equal(env.reset(), _np(tw.reset_torch()))
    acts = _actions(env, 50, seed=4)
    for t in range(50):
        o, r, d, _ = env.step(_np(acts[t]))
        ot, rt, dt, _ = tw.step_torch(acts[t])
        assert np.array_equal(o, _np(ot)) and np.array_equal(d, _np(dt).astype(bool)), t
        m = d.copy()
        if t % 5 == 0:
            m[t::97] = True
        got = env.reset(mask=m)
        want = tw.reset_torch(mask=torch.as_tensor(m, device="cuda"))
        assert np.array_equal(got, _np(want)), t
    _assert_states_equal(env, tw, "numpy route")
    env.close(); tw.close()
