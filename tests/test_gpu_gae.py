"""GPU tests of gae_torch / gae (sg_gae_device / sg_gae) against the NumPy model tests/gae_model.py.  "Equal" is bitwise: the
same float32 bit patterns, and NaN exactly where the model has NaN."""
import numpy as np
import pytest

from gae_model import dense_from_list, gae_model, synthetic

pytestmark = pytest.mark.gpu

ENV_ID = "KeplerCircleOrbit-v0"  # (the result does not depend on the id: the handle only gives the batch size)
SHAPES = [(1, 1), (7, 63), (128, 4101), (20, 65536)]


def make(n, env_id=ENV_ID, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _equal(got, want):
    """bitwise, NaN positions included"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w])


def _dev(a, offset=0):
    """the array on the device; offset=1: as a view that starts one element into a larger buffer (4-byte aligned only for
    float32, 1-byte for uint8)"""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset * a.itemsize
    return view


def _run(env, s, offset=0, **kw):
    import torch
    K, B = s["reward"].shape
    t = {k: _dev(v, offset) for k, v in s.items() if v is not None}
    out = dict(advantage=_dev(np.zeros((K, B), np.float32), offset), returns=_dev(np.zeros((K, B), np.float32), offset))
    adv, ret = env.gae_torch(t["reward"], t["done"], t["trunc"], value=t.get("value"), last_value=t.get("last_value"),
                             terminal_value=t.get("terminal_value"), out=out, **kw)
    torch.cuda.synchronize()
    env.check_status()
    return adv.cpu().numpy(), ret.cpu().numpy()


def _assert_model(got, s, what, **kw):
    want = gae_model(**s, **kw)
    for g, w, name in zip(got, want, ("advantage", "returns")):
        assert _equal(g, w), (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K,B", SHAPES)
def test_dense_terminal_values_equal_the_model(K, B, offset):
    """5: synthetic inputs, dense terminal values; and the same through views offset by one element"""
    env = make(B)
    s = synthetic(K, B, seed=100 + K)
    if K * B >= 2:
        d = s["done"].astype(bool)
        assert (d & s["trunc"].astype(bool)).any() and (d & ~s["trunc"].astype(bool)).any()
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        got = _run(env, s, offset, gamma=gamma, lam=lam)
        _assert_model(got, s, (K, B, offset, gamma, lam), gamma=gamma, lam=lam)
    env.close()


def _list_of(s, rng, extra_capacity):
    """the records of every done step in shuffled order, with the dense terminal value of each, in buffers larger than the count"""
    t, i = np.nonzero(s["done"])
    order = rng.permutation(t.size)
    n, cap = t.size, t.size + extra_capacity
    step_env = np.full((cap, 2), -7, np.int32)  # (rows past the count are never read)
    step_env[:n, 0], step_env[:n, 1] = t[order], i[order]
    value = np.full(cap, np.nan, np.float32)
    value[:n] = s["terminal_value"][t[order], i[order]]
    return n, step_env, value


@pytest.mark.parametrize("K,B", SHAPES)
def test_list_form_equals_dense_form(K, B):
    """6: the list holds every done step (as sg_terminal_list does), shuffled; capacity > count"""
    import torch
    env = make(B)
    s = synthetic(K, B, seed=200 + K)
    n, step_env, value = _list_of(s, np.random.default_rng(K), extra_capacity=37)
    dense = _run(env, s)
    t = {k: _dev(v) for k, v in s.items()}
    term = dict(count=torch.tensor([n], dtype=torch.int32, device="cuda"), step_env=_dev(step_env), value=_dev(value))
    adv, ret = env.gae_torch(t["reward"], t["done"], t["trunc"], value=t["value"], last_value=t["last_value"], terminal=term)
    torch.cuda.synchronize()
    env.check_status()
    assert _equal(adv.cpu().numpy(), dense[0]) and _equal(ret.cpu().numpy(), dense[1])
    _assert_model(dense, s, (K, B))
    # and the NumPy front end (sg_gae), both forms
    h_list = env.gae(s["reward"], s["done"], s["trunc"], value=s["value"], last_value=s["last_value"],
                     terminal=dict(count=n, step_env=step_env, value=value))
    h_dense = env.gae(s["reward"], s["done"], s["trunc"], value=s["value"], last_value=s["last_value"], terminal_value=s["terminal_value"])
    for h in (h_list, h_dense):
        assert _equal(h[0], dense[0]) and _equal(h[1], dense[1])
    env.close()


@pytest.mark.parametrize("env_id", ["GoalContinuous3P-v0", "KeplerCircleOrbit-v0"])
def test_a_real_rollout_equals_the_model(env_id):
    """7: rollout_torch with random actions and a terminal list, a fixed value function of the observation evaluated on obs and
    on terminal["obs"]; the model is fed from terminal_records.  The time limit (40) is below the ~50-step mean episode of
    random actions, so most episodes are truncated and some end by a terminal event first."""
    import torch
    K, B, LIMIT = 96, 2048, 40
    env = make(B, env_id, seed=5, max_episode_steps=LIMIT)
    D = env.obs_dim
    w = torch.from_numpy(np.random.default_rng(3).standard_normal(D).astype(np.float32)).cuda()
    V = lambda o: torch.tanh((o * w).sum(-1))  # noqa: E731
    obs0 = env.reset_torch().clone()
    acts = env.random_actions_torch(K, seed=6)
    obs = torch.empty((K, B, D), device="cuda")
    rew = torch.empty((K, B), device="cuda")
    done, trunc = torch.empty((K, B), dtype=torch.uint8, device="cuda"), torch.empty((K, B), dtype=torch.uint8, device="cuda")
    term = env.terminal_list_torch(K * B // 8)
    term["obs"].zero_()
    env.rollout_torch(acts, obs, rew, done, trunc, terminal=term)
    value = torch.cat([V(obs0)[None], V(obs[:-1])]).contiguous()
    last_value = V(obs[-1]).contiguous()
    tvals = V(term["obs"]).contiguous()
    adv, ret = env.gae_torch(rew, done, trunc, value=value, last_value=last_value, terminal=env.value_list_torch(term, tvals))
    torch.cuda.synchronize()
    env.check_status()
    d, tr = done.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool)
    assert (d & tr).sum() >= 1 and (d & ~tr).sum() >= 1, ((d & tr).sum(), (d & ~tr).sum())
    step, envs, tobs = env.terminal_records(term)
    n = int(term["count"].item())
    assert n == d.sum() == step.size and d[step, envs].all()
    se = term["step_env"][:n].cpu().numpy()
    order = np.lexsort((se[:, 1], se[:, 0]))
    assert np.array_equal(se[order, 0], step) and np.array_equal(se[order, 1], envs)
    assert np.array_equal(term["obs"][:n].cpu().numpy()[order], tobs)
    dense = dense_from_list(K, B, n, np.stack([step, envs], 1), tvals[:n].cpu().numpy()[order])
    s = dict(reward=rew.cpu().numpy(), done=d, trunc=tr, value=value.cpu().numpy(), last_value=last_value.cpu().numpy(), terminal_value=dense)
    _assert_model((adv.cpu().numpy(), ret.cpu().numpy()), s, env_id)
    # bootstrapping matters in this rollout: without it the truncated steps differ
    off = gae_model(bootstrap_truncated=False, **s)[0]
    assert not np.array_equal(off, adv.cpu().numpy())
    env.close()


def test_a_nan_reward_stays_inside_its_episode():
    """8"""
    K, B = 64, 300
    env = make(B)
    s = synthetic(K, B, seed=8, p_done=0.05)
    base = _run(env, s)
    t0 = 40

    def episode_start(i):
        return max([t + 1 for t in range(t0) if s["done"][t, i]], default=0)
    # an env whose episode around t0 has steps before t0 and an episode on either side
    i0 = next(i for i in range(B) if 0 < episode_start(i) < t0 and not s["done"][t0, i] and s["done"][t0 + 1:, i].any())
    first = episode_start(i0)
    bad = {k: v.copy() for k, v in s.items()}
    bad["reward"][t0, i0] = np.nan
    got = _run(env, bad)
    _assert_model(got, bad, "nan")
    inside = np.zeros((K, B), bool)
    inside[first:t0 + 1, i0] = True
    for g, b in zip(got, base):
        assert np.isnan(g[inside]).all() and not np.isnan(g[~inside]).any()
        assert np.array_equal(g.view(np.uint32)[~inside], b.view(np.uint32)[~inside])
    env.close()


def test_bootstrap_off_and_missing_values():
    """9: bootstrap_truncated=False equals the model with it off (and reads no terminal values); value=None equals zeros"""
    K, B = 33, 1000
    env = make(B)
    s = synthetic(K, B, seed=9)
    got = _run(env, s, bootstrap_truncated=False)
    _assert_model(got, s, "off", bootstrap_truncated=False)
    assert not _equal(got[0], _run(env, s)[0])
    no_tv = _run(env, {**s, "terminal_value": None})
    assert _equal(no_tv[0], got[0]) and _equal(no_tv[1], got[1])
    for keep_tv in (True, False):
        base = {**s, "terminal_value": s["terminal_value"] if keep_tv else None}
        none = _run(env, {**base, "value": None, "last_value": None})
        zeros = _run(env, {**base, "value": np.zeros((K, B), np.float32), "last_value": np.zeros(B, np.float32)})
        assert _equal(none[0], zeros[0]) and _equal(none[1], zeros[1])
        _assert_model(none, {**base, "value": None, "last_value": None}, ("value none", keep_tv))
    env.close()


@pytest.mark.parametrize("form", ["dense", "list"])
def test_captured_into_a_graph_and_replayed_on_changed_inputs(form):
    """10"""
    import torch
    K, B = 24, 5000
    env = make(B)
    a, b = synthetic(K, B, seed=10), synthetic(K, B, seed=11)
    static = {k: _dev(v) for k, v in a.items()}
    out = dict(advantage=torch.zeros((K, B), device="cuda"), returns=torch.zeros((K, B), device="cuda"))
    cap = K * B // 10
    term = dict(count=torch.zeros(1, dtype=torch.int32, device="cuda"), step_env=torch.zeros((cap, 2), dtype=torch.int32, device="cuda"),
                value=torch.zeros(cap, device="cuda"))

    def fill_list(s, seed):
        n, se, val = _list_of(s, np.random.default_rng(seed), extra_capacity=0)
        assert n <= cap
        term["count"].fill_(n)
        term["step_env"][:n].copy_(torch.from_numpy(se))
        term["value"][:n].copy_(torch.from_numpy(val))
    fill_list(a, 1)
    kw = dict(terminal=term) if form == "list" else dict(terminal_value=static["terminal_value"])

    def call():
        env.gae_torch(static["reward"], static["done"], static["trunc"], value=static["value"], last_value=static["last_value"], out=out, **kw)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for s, seed in ((a, 1), (b, 2)):
        for k, v in s.items():
            static[k].copy_(torch.from_numpy(v))
        fill_list(s, seed)
        out["advantage"].fill_(float("nan")); out["returns"].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _assert_model((out["advantage"].cpu().numpy(), out["returns"].cpu().numpy()), s, (form, seed))
    env.check_status()
    env.close()


@pytest.mark.parametrize("bad", ["count", "record"])
def test_a_bad_list_is_reported_once_and_the_handle_works_afterwards(bad):
    """11: count > capacity, a (step, env) outside the rollout: the status word, nothing else"""
    import torch
    from space_gym_amd._native import NativeError
    K, B = 16, 500
    env = make(B)
    s = synthetic(K, B, seed=12)
    n, se, val = _list_of(s, np.random.default_rng(0), extra_capacity=0)
    if bad == "count":
        se, val, count = se[:n - 3], val[:n - 3], n  # three values are missing
    else:
        se = se.copy()
        k = int(np.flatnonzero(~s["trunc"].astype(bool)[se[:, 0], se[:, 1]])[0])  # a record the scan would not have read anyway
        se[k] = (K, 0) if K % 2 else (3, B)
        count = n
    t = {k2: _dev(v) for k2, v in s.items()}
    term = dict(count=torch.tensor([count], dtype=torch.int32, device="cuda"), step_env=_dev(se), value=_dev(val))
    adv, ret = env.gae_torch(t["reward"], t["done"], t["trunc"], value=t["value"], last_value=t["last_value"], terminal=term)
    torch.cuda.synchronize()
    with pytest.raises(NativeError, match="sg_gae_device: a value list"):
        env.check_status()
    env.check_status()  # reported once
    if bad == "record":  # the bad record is ignored: everything else is as the model has it
        _assert_model((adv.cpu().numpy(), ret.cpu().numpy()), s, bad)
    got = _run(env, s)
    _assert_model(got, s, "afterwards")
    env.reset_torch()
    env.step_torch(env.random_actions_torch(1, seed=1)[0])
    env.check_status()
    # the host form refuses both up front
    with pytest.raises(NativeError, match="value list"):
        env.gae(s["reward"], s["done"], s["trunc"], terminal=dict(count=count, step_env=se, value=val))
    env.check_status()
    env.close()


def test_the_envs_are_untouched():
    """12: a step after gae_torch equals the step of a twin env that never called it"""
    import torch
    B, K = 3000, 12
    a, b = make(B, "GoalContinuous3P-v0", seed=21), make(B, "GoalContinuous3P-v0", seed=21)
    a.reset_torch(); b.reset_torch()
    acts = a.random_actions_torch(3, seed=2)
    for env in (a, b):
        env.step_torch(acts[0])
    s = synthetic(K, B, seed=13)
    _assert_model(_run(a, s), s, "twin")
    a.gae(s["reward"], s["done"], s["trunc"])
    for t in (1, 2):
        ra, rb = a.step_torch(acts[t]), b.step_torch(acts[t])
        torch.cuda.synchronize()
        for x, y in zip(ra, rb):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert np.array_equal(a.save_state(), b.save_state())
    a.close(); b.close()
