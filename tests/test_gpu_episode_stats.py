"""GPU tests of the episode statistics (sg_set_episode_stats): the device pass against a float64 NumPy loop over the rewards
the engine returned -- gym.wrappers.RecordEpisodeStatistics' return and length -- on every rollout plan, the same numbers
through every stepping route, no effect on the step outputs, snapshots, graph replay and list overflow."""
import numpy as np
import pytest

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


class NumpyEpisodes:
    """RecordEpisodeStatistics as a float64 loop over the float32 rewards: one add per step, in step order"""

    def __init__(self, n):
        self.ret, self.len = np.zeros(n, np.float64), np.zeros(n, np.int32)

    def step(self, rew, done, trunc):
        self.ret += rew.astype(np.float64)
        self.len += 1
        idx = np.nonzero(done)[0]
        out = (idx, self.ret[idx].copy(), self.len[idx].copy(), trunc[idx] != 0)
        self.ret[idx] = 0.0
        self.len[idx] = 0
        return out

    def rollout(self, rew, done, trunc):
        """records of a [K, B] rollout, sorted by (step, env) like episode_records"""
        parts = [self.step(rew[t], done[t], trunc[t]) for t in range(rew.shape[0])]
        return dict(step=np.concatenate([np.full(len(p[0]), t, np.int32) for t, p in enumerate(parts)]),
                    env=np.concatenate([p[0] for p in parts]).astype(np.int32), r=np.concatenate([p[1] for p in parts]),
                    l=np.concatenate([p[2] for p in parts]), truncated=np.concatenate([p[3] for p in parts]))


def _assert_records_equal(got, want):
    for k in ("step", "env", "l", "truncated"):
        assert np.array_equal(got[k], want[k]), k
    assert got["r"].dtype == np.float64
    assert np.array_equal(got["r"].view(np.uint64), want["r"].view(np.uint64))  # bit for bit


def _rollout_with_records(env, a, cap, terminal=False):
    import torch
    K = a.shape[0]
    obs, rew, done, trunc = _rollout_buffers(env, K)
    el = env.episode_list_torch(cap)
    term = env.terminal_list_torch(cap) if terminal else None
    env.rollout_torch(a, obs, rew, done, trunc, terminal=term, episodes=el)
    torch.cuda.synchronize()
    out = dict(obs=obs, rew=rew.cpu().numpy(), done=done.cpu().numpy(), trunc=trunc.cpu().numpy(), rec=env.episode_records(el))
    if terminal:
        out["term"] = env.terminal_records(term)
    return out


CASES = [("GoalContinuous3P-v0", None), ("KeplerRandomOrbits-v0", None), ("GoalDiscrete3-v0", None),
         ("GoalContinuous3P-v0", "acceleration")]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("plan", ["pair", "single", "unfused"])
@pytest.mark.parametrize("env_id,steering", CASES)
def test_rollout_records_equal_a_float64_loop(env_id, steering, plan, monkeypatch):
    """K = 160 steps in two calls (60 + 100): the records are exactly those of a NumPy float64 accumulation of the returned
    rewards -- same (step, env) set, return bit for bit, length, truncated flag -- and length == max_episode_steps exactly where
    truncated; the terminal list of the same call names the same env-steps"""
    n = 8192
    monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", "single" if plan == "single" else "pair")
    kw = dict(steering=steering) if steering else {}
    env = make(env_id, n, seed=21, max_episode_steps=MAX_STEPS, episode_statistics=True, **kw)
    if plan == "unfused":
        env.set_unfused_rollout(True)
    env.reset_torch()
    a = _actions(env, 160, seed=3)
    ref = NumpyEpisodes(n)
    n_trunc = n_term = 0
    for lo, hi in ((0, 60), (60, 160)):
        got = _rollout_with_records(env, a[lo:hi].contiguous(), cap=n * 8, terminal=(lo == 0))
        want = ref.rollout(got["rew"], got["done"], got["trunc"])
        _assert_records_equal(got["rec"], want)
        assert np.all(got["rec"]["l"][got["rec"]["truncated"]] == MAX_STEPS)
        assert np.all(got["rec"]["l"] >= 1)
        if lo == 0:
            ts, te, _ = got["term"]
            assert np.array_equal(ts, got["rec"]["step"]) and np.array_equal(te, got["rec"]["env"])
        n_trunc += int(got["rec"]["truncated"].sum())
        n_term += int((~got["rec"]["truncated"]).sum())
    assert n_trunc > 0, (n_trunc, n_term)
    if env_id.startswith("Goal"):
        assert n_term > 0, (n_trunc, n_term)  # both ways of ending an episode occurred
    env.check_status()
    env.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n,K,max_steps", [(8192, 100, MAX_STEPS), (131072, 50, 20)])
def test_every_route_gives_the_same_episodes(n, K, max_steps):
    """the same actions through K calls of step_torch(episodes=...), K calls of NumPy step() (info["episode"]) and one
    rollout_torch(episodes=...): identical returns and lengths on every finished env; step_torch leaves the rows of envs
    that did not finish untouched, step() reports NaN / -1 there.  131 072 envs: the one-wave step kernel."""
    import torch
    env_id = "GoalContinuous3P-v0"
    envs = [make(env_id, n, seed=17, max_episode_steps=max_steps, episode_statistics=True) for _ in range(3)]
    dev, host, roll = envs
    dev.reset_torch(); host.reset(); roll.reset_torch()
    a = _actions(dev, K, seed=9)
    got = _rollout_with_records(roll, a, cap=n * K // 4)["rec"]
    rows = dict(r=torch.empty(n, dtype=torch.float64, device="cuda"), l=torch.empty(n, dtype=torch.int32, device="cuda"))
    seen = 0
    for t in range(K):
        rows["r"].fill_(12345.0); rows["l"].fill_(-7)
        _, rw, dn, _ = dev.step_torch(a[t], episodes=rows)
        torch.cuda.synchronize()
        r, l, d = rows["r"].cpu().numpy(), rows["l"].cpu().numpy(), dn.cpu().numpy().astype(bool)
        _, rw_h, d_h, info = host.step(a[t].cpu().numpy())
        assert np.array_equal(d_h, d) and np.array_equal(rw_h, rw.cpu().numpy())
        assert np.array_equal(info["_episode"], d)
        hr, hl = info["episode"]["r"], info["episode"]["l"]
        assert np.all(np.isnan(hr[~d])) and np.all(hl[~d] == -1)
        assert np.all(r[~d] == 12345.0) and np.all(l[~d] == -7)  # untouched
        sel = got["step"] == t
        envs_t = got["env"][sel]
        assert np.array_equal(envs_t, np.nonzero(d)[0])
        for x, y in ((r[d], got["r"][sel]), (hr[d], got["r"][sel])):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        assert np.array_equal(l[d], got["l"][sel]) and np.array_equal(hl[d], got["l"][sel])
        seen += int(d.sum())
    assert seen == len(got["step"]) > 0
    for e in envs:
        e.close()


@pytest.mark.timeout(300)
def test_statistics_do_not_change_the_step_outputs():
    """with statistics on, obs / reward / done / trunc / terminal observations are bit-identical to a handle with them off:
    a rollout with a terminal list, step_torch with terminal_obs, NumPy steps with terminal observations"""
    import torch
    n, K = 8192, 80
    on = make("GoalContinuous3P-v0", n, seed=4, max_episode_steps=30, episode_statistics=True)
    off = make("GoalContinuous3P-v0", n, seed=4, max_episode_steps=30)
    a = _actions(on, K + 30, seed=1)
    outs = []
    for e in (on, off):
        o = {}
        o["reset"] = e.reset_torch().clone()
        obs, rew, done, trunc = _rollout_buffers(e, K)
        term = e.terminal_list_torch(n * K)
        e.rollout_torch(a[:K], obs, rew, done, trunc, terminal=term)
        torch.cuda.synchronize()
        o["roll"] = (obs, rew, done, trunc)
        o["term"] = e.terminal_records(term)
        steps = []
        for t in range(K, K + 20):
            tobs = torch.full((n, e.obs_dim), float("nan"), device="cuda")
            steps.append(tuple(x.clone() for x in e.step_torch(a[t], terminal_obs=tobs)) + (tobs,))
        o["steps"] = steps
        o["host"] = [e.step(a[t].cpu().numpy()) for t in range(K + 20, K + 30)]
        outs.append(o)
    x, y = outs
    assert torch.equal(x["reset"], y["reset"])
    for u, v in zip(x["roll"], y["roll"]):
        assert torch.equal(u, v)
    for u, v in zip(x["term"], y["term"]):
        assert np.array_equal(u, v)
    for s, t in zip(x["steps"], y["steps"]):
        for u, v in zip(s, t):
            assert torch.equal(u.nan_to_num(7.0), v.nan_to_num(7.0))
    for (o1, r1, d1, i1), (o2, r2, d2, i2) in zip(x["host"], y["host"]):
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2)
        assert np.array_equal(i1["TimeLimit.truncated"], i2["TimeLimit.truncated"])
        assert np.array_equal(i1["terminal_observation"], i2["terminal_observation"], equal_nan=True)
        assert "episode" in i1 and "episode" not in i2
    on.close(); off.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerRandomOrbits-v0"])
def test_snapshot_resumes_the_statistics(env_id):
    """save mid-episode, 50 steps, load, the same 50 steps: identical records; a blob taken with statistics on switches them
    on in a fresh handle and continues the same way; with them off the blob keeps the layout it had before they existed"""
    n = 8192
    env = make(env_id, n, seed=12, max_episode_steps=MAX_STEPS)
    env.reset_torch()
    a = _actions(env, 80, seed=5)
    blob_off = env.save_state()
    cols = env.snapshot_columns(blob_off)  # asserts header + version-1 columns == the whole blob
    assert int(blob_off[4:8].view(np.uint32)[0]) == 1 and "ep_ret" not in cols
    assert blob_off.size == int(env._lib.sg_state_bytes(env._h))
    env.set_episode_statistics(True)
    _rollout_with_records(env, a[:30].contiguous(), cap=n * 4)  # mid-episode
    blob = env.save_state()
    assert blob.size == blob_off.size + 12 * n and int(blob[4:8].view(np.uint32)[0]) == 2
    cols = env.snapshot_columns(blob)
    assert cols["ep_len"].max() > 0 and np.any(cols["ep_ret"] != 0)
    first = _rollout_with_records(env, a[30:].contiguous(), cap=n * 4)["rec"]
    env.load_state(blob)
    again = _rollout_with_records(env, a[30:].contiguous(), cap=n * 4)["rec"]
    _assert_records_equal(again, first)
    fresh = make(env_id, n, seed=99, max_episode_steps=MAX_STEPS)
    assert not fresh.episode_statistics
    fresh.load_state(blob)
    assert fresh.episode_statistics
    _assert_records_equal(_rollout_with_records(fresh, a[30:].contiguous(), cap=n * 4)["rec"], first)
    # a version-1 blob still loads (into a handle with statistics on: they start from zero)
    env.load_state(blob_off)
    assert env.episode_statistics and np.all(env.snapshot_columns(env.save_state())["ep_len"] == 0)
    assert len(first["step"]) > 0
    env.close(); fresh.close()


@pytest.mark.timeout(300)
def test_graph_replay_accumulates_on_the_device():
    """step_torch(episodes=...) captured in a graph on one stream and replayed 30 times equals 30 eager steps: the running
    sums live on the device, so each replay continues them"""
    import torch
    n, T = 8192, 30
    graphed = make("GoalContinuous3P-v0", n, seed=7, max_episode_steps=12, episode_statistics=True)
    eager = make("GoalContinuous3P-v0", n, seed=7, max_episode_steps=12, episode_statistics=True)
    graphed.reset_torch(); eager.reset_torch()
    torch.cuda.synchronize()
    a = _actions(eager, T, seed=2)
    static_a = torch.empty((n, 2), device="cuda")
    out = dict(obs=torch.empty((n, graphed.obs_dim), device="cuda"), reward=torch.empty(n, device="cuda"),
               done=torch.empty(n, dtype=torch.uint8, device="cuda"), trunc=torch.empty(n, dtype=torch.uint8, device="cuda"))
    rows = dict(r=torch.zeros(n, dtype=torch.float64, device="cuda"), l=torch.zeros(n, dtype=torch.int32, device="cuda"))
    erows = dict(r=torch.zeros(n, dtype=torch.float64, device="cuda"), l=torch.zeros(n, dtype=torch.int32, device="cuda"))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        static_a.copy_(a[0])
        with torch.cuda.graph(g, stream=s):
            graphed.step_torch(static_a, out=out, episodes=rows)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    finished = 0
    for t in range(T):
        static_a.copy_(a[t])
        g.replay()
        torch.cuda.synchronize()
        ob, rw, dn, tr = eager.step_torch(a[t].contiguous(), episodes=erows)
        torch.cuda.synchronize()
        assert torch.equal(out["obs"], ob) and torch.equal(out["reward"], rw) and torch.equal(out["done"], dn)
        assert torch.equal(rows["r"], erows["r"]) and torch.equal(rows["l"], erows["l"])
        finished += int(dn.sum().item())
    assert finished > 0
    assert int(rows["l"].max().item()) == 12  # episodes that ran their whole length, summed over replays
    graphed.close(); eager.close()


@pytest.mark.timeout(300)
def test_episode_list_overflow_is_reported():
    import torch
    n, K = 4096, 64
    env = make("GoalContinuous3P-v0", n, seed=6, max_episode_steps=10, episode_statistics=True)
    env.reset_torch()
    a = _actions(env, K, seed=4)
    obs, rew, done, trunc = _rollout_buffers(env, K)
    el = env.episode_list_torch(capacity=100)
    env.rollout_torch(a, obs, rew, done, trunc, episodes=el)
    torch.cuda.synchronize()
    assert int(el["count"].item()) == int(done.sum().item()) > 100
    with pytest.raises(OverflowError):
        env.episode_records(el)
    env.close()


@pytest.mark.timeout(120)
def test_episode_calls_fail_while_statistics_are_off():
    """the native *_episodes entry points refuse a handle without statistics (SG_ERR_INVALID), whatever the Python side does"""
    import ctypes as C
    import torch
    from space_gym_amd import _native
    n = 8192
    env = make("GoalContinuous3P-v0", n, seed=1)
    env.reset_torch()
    a = _actions(env, 1, seed=1)
    obs, rew, done, trunc = _rollout_buffers(env, 1)
    r = torch.zeros(n, dtype=torch.float64, device="cuda"); l = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = env._stream()
    rc = env._lib.sg_step_device_episodes(env._h, p(a), p(obs), p(rew), p(done), p(trunc), None, p(r), p(l), s)
    assert rc == -1
    el = env.episode_list_torch(16)
    lst = _native.SgEpisodeList(*(el[k].data_ptr() for k in ("count", "step_env", "r", "l", "truncated")), 16)
    assert env._lib.sg_rollout_device_episodes(env._h, 1, p(a), p(obs), p(rew), p(done), p(trunc), None, C.byref(lst), s) == -1
    ret, ln = C.c_void_p(), C.c_void_p()
    assert env._lib.sg_step_end_episodes(env._h, C.byref(ret), C.byref(ln)) == -1
    env.close()
