"""GPU tests of retrace_torch / dqn_retrace_grad_torch (sg_retrace_device) against the NumPy model of tests/retrace_model.py.  "Equal" is
bitwise: the same float32 bit patterns, and NaN exactly where the model has NaN.  The shapes are retrace_model.CASES;
tests/test_retrace.py checks on the CPU that their inputs exercise what each case is for."""
import ctypes as C

import numpy as np
import pytest

from retrace_model import CASES, retrace_case, retrace_model
from test_gpu_gae import _dev, _equal

pytestmark = pytest.mark.gpu

ENV_ID = "GoalDiscrete3-v0"  # (retrace_torch does not depend on the id or on num_envs; the helper needs a discrete id)
B = 64
INF = float("inf")


@pytest.fixture(scope="module")
def env():
    import space_gym_amd as sg
    e = sg.make_vec(ENV_ID, B, device=0, seed=5, max_episode_steps=5)
    yield e
    e.check_status()
    e.close()


def _host(*ts):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device="cuda")


def _call(env, s, ratio=None, loss=None, offset=0, discounts=None, **kw):
    """retrace_torch on inputs given as NumPy arrays (None: left out), into NaN-prefilled outputs -> NumPy target, or (target, td, g)"""
    Ls, n = s["reward"].shape
    t = {k: _dev(v, offset) for k, v in s.items() if v is not None}
    if loss is not None:
        loss = dict(q_online=_dev(loss["q_online"], offset), weight=None if loss.get("weight") is None else _dev(loss["weight"], offset),
                    huber_delta=loss.get("huber_delta", INF), td_error=_nan(Ls, n), g=_nan(Ls, n))
    got = env.retrace_torch(t["reward"], t["done"], t["trunc"], t["q"], t["value"], last_value=t.get("last_value"),
                            ratio=None if ratio is None else _dev(ratio, offset), terminal_value=t.get("terminal_value"),
                            discounts=None if discounts is None else _dev(discounts), out=_nan(Ls, n), loss=loss, **kw)
    return _host(got)[0] if loss is None else _host(*got)


def _same(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    for k, (g, w) in enumerate(zip(got, want)):
        assert _equal(g, w), (what, k, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


@pytest.mark.parametrize("Ls,n", CASES)
def test_the_targets_and_the_loss_outputs_equal_the_model(env, Ls, n):
    """with and without ratio, last_value and terminal_value; bootstrap_truncated off; c_bar below, at and above the ratios and +inf;
    lam 0 and 1; scalar discounts and the device tensor, bit-equal at float(gamma), float(lam); the loss outputs with and without
    weight at huber_delta 1 and inf"""
    s, x = retrace_case(Ls, n)
    ratio = x["ratio"]
    no_tv, no_last = {**s, "terminal_value": None}, {**s, "last_value": None}
    for what, a, kw in (("retrace", s, dict(ratio=ratio)), ("peng", s, dict()), ("no terminal", no_tv, dict(ratio=ratio, gamma=0.97, lam=0.9)),
                        ("no last, no ratio", no_last, dict(lam=0.5)), ("bare", {**no_tv, "last_value": None}, dict(gamma=1.0)),
                        ("bootstrap off", s, dict(ratio=ratio, bootstrap_truncated=False)),
                        ("c_bar low", s, dict(ratio=ratio, c_bar=float(ratio.min()) / 2, lam=0.95)),
                        ("c_bar high", s, dict(ratio=ratio, c_bar=float(ratio.max()) * 2, gamma=0.9)),
                        ("c_bar inf", s, dict(ratio=ratio, c_bar=INF, gamma=0.9, lam=0.8)), ("c_bar inf, no ratio", s, dict(c_bar=INF)),
                        ("lam 0", s, dict(ratio=ratio, lam=0.0)), ("lam 1", s, dict(ratio=ratio, gamma=0.95, lam=1.0))):
        _same(_call(env, a, **kw), retrace_model(**a, **kw), what)
    g, l = np.float32(0.987), np.float32(0.913)
    table = _call(env, s, ratio=ratio, discounts=np.array([g, l], np.float32), gamma=0.5, lam=0.5)  # (the scalars are not read)
    _same(table, retrace_model(**s, ratio=ratio, discounts=np.array([g, l], np.float32)), "discounts")
    _same(table, _call(env, s, ratio=ratio, gamma=float(g), lam=float(l)), "discounts against scalars")
    for weight in (None, x["weight"]):
        for delta in (1.0, INF):
            for a, kw in ((s, dict(ratio=ratio, lam=0.9)), (no_tv, dict())):
                loss = dict(q_online=x["q_online"], weight=weight, huber_delta=delta)
                _same(_call(env, a, loss=loss, **kw), retrace_model(**a, loss=loss, **kw), ("loss", weight is not None, delta))
    env.check_status()


def test_two_calls_write_every_cell_and_views_at_odd_offsets_work(env):
    Ls, n = 49, 240
    s, x = retrace_case(Ls, n)
    loss = dict(q_online=x["q_online"], weight=x["weight"], huber_delta=1.0)
    want = retrace_model(**s, ratio=x["ratio"], loss=loss)
    a, b = _call(env, s, ratio=x["ratio"], loss=loss), _call(env, s, ratio=x["ratio"], loss=loss)
    _same(a, want, "first")
    _same(b, a, "second")
    assert not any(np.isnan(o).any() for o in a)
    # every input a view that starts one element into a larger buffer: 4-byte aligned floats, 1-byte aligned flags
    _same(_call(env, s, ratio=x["ratio"], loss=loss, offset=1), want, "odd offsets")
    s65, x65 = retrace_case(9, 65)
    _same(_call(env, s65, ratio=x65["ratio"], offset=1), retrace_model(**s65, ratio=x65["ratio"]), "odd offsets, odd n")


def test_a_nan_reward_stays_inside_its_episode_and_column(env):
    Ls, n = 49, 240
    s, x = retrace_case(Ls, n)
    done = s["done"].astype(bool)
    t0 = 30
    i0 = next(i for i in range(n) if done[:t0, i].any() and not done[t0, i] and done[t0 + 1:, i].any())
    first = max(t + 1 for t in range(t0) if done[t, i0])
    inside = np.zeros((Ls, n), bool)
    inside[first:t0 + 1, i0] = True
    bad = {k: v.copy() for k, v in s.items()}
    bad["reward"][t0, i0] = np.nan
    loss = dict(q_online=x["q_online"], weight=x["weight"], huber_delta=1.0)
    base, got = _call(env, s, ratio=x["ratio"], loss=loss), _call(env, bad, ratio=x["ratio"], loss=loss)
    _same(got, retrace_model(**bad, ratio=x["ratio"], loss=loss), "nan")
    for g, b in zip(got[:2], base[:2]):  # target and td_error are NaN there; g's clip turns a NaN td into -delta, as the model's does
        assert np.isnan(g[inside]).all() and not np.isnan(g[~inside]).any()
    for g, b in zip(got, base):
        assert np.array_equal(g.view(np.uint32)[~inside], b.view(np.uint32)[~inside])


def test_a_captured_graph_reads_the_discounts_at_every_replay(env):
    import torch
    Ls, n = 9, 240
    s, x = retrace_case(Ls, n)
    t = {k: _dev(v) for k, v in s.items()}
    ratio, q_online, weight = _dev(x["ratio"]), _dev(x["q_online"]), _dev(x["weight"])
    first = np.array([0.99, 0.95], np.float32)
    disc = _dev(first)
    out, td, g = _nan(Ls, n), _nan(Ls, n), _nan(Ls, n)

    def call():
        env.retrace_torch(t["reward"], t["done"], t["trunc"], t["q"], t["value"], last_value=t["last_value"], ratio=ratio,
                          terminal_value=t["terminal_value"], discounts=disc, out=out,
                          loss=dict(q_online=q_online, weight=weight, huber_delta=1.0, td_error=td, g=g))
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    seen = []
    for values in (first, np.array([0.9, 0.5], np.float32), np.array([1.0, 0.0], np.float32)):
        disc.copy_(torch.from_numpy(values))
        for o in (out, td, g):
            o.fill_(float("nan"))
        graph.replay()
        got = _host(out, td, g)
        _same(got, retrace_model(**s, ratio=x["ratio"], discounts=values, loss=dict(q_online=x["q_online"], weight=x["weight"], huber_delta=1.0)),
              tuple(values))
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
    env.check_status()


def _dqn_pair(env, seed):
    from dqn_model import random_dqn
    from test_gpu_dqn import _handle
    rng = np.random.default_rng(seed)
    return _handle(env, random_dqn(rng, env.obs_dim, 32, 2)), _handle(env, random_dqn(rng, env.obs_dim, 32, 2))


def test_g_passed_to_dqn_grad_torch_gives_the_gradients_of_the_model_s_g(env):
    import torch
    Ls, n = 9, 65
    s, x = retrace_case(Ls, n)
    online, _ = _dqn_pair(env, 3)
    loss = dict(q_online=x["q_online"], weight=x["weight"], huber_delta=1.0)
    t = {k: _dev(v) for k, v in s.items()}
    _, _, g = env.retrace_torch(t["reward"], t["done"], t["trunc"], t["q"], t["value"], last_value=t["last_value"], ratio=_dev(x["ratio"]),
                                terminal_value=t["terminal_value"],
                                loss=dict(q_online=_dev(x["q_online"]), weight=_dev(x["weight"]), huber_delta=1.0))
    want_g = retrace_model(**s, ratio=x["ratio"], loss=loss)[2]
    rng = np.random.default_rng(1)
    obs, action = _dev(rng.standard_normal((Ls * n, env.obs_dim)).astype(np.float32)), _dev(rng.integers(0, 6, Ls * n).astype(np.int32))
    got = env.dqn_grad_torch(online, obs, action, g_taken=g.reshape(Ls * n))
    want = env.dqn_grad_torch(online, obs, action, g_taken=_dev(want_g.reshape(Ls * n)))
    torch.cuda.synchronize()
    for (gw, gb), (ww, wb) in zip(got["net"], want["net"]):
        assert torch.equal(gw, ww) and torch.equal(gb, wb) and float(gw.abs().max()) > 0.0


def test_sampled_sequences_feed_the_dqn_retrace_update_end_to_end(env):
    """a closed-loop epsilon-greedy rollout_dqn_torch into a ring of T = 32 slots in two chunks; 48 sequences of L = 8 with a behaviour
    probability column gathered by columns=; dqn_retrace_grad_torch for each trace equals the same composition with retrace_model in
    place of the kernel, bit for bit: the targets, the td errors, the loss gradients and the net's gradients"""
    import torch
    T, K, Ls, n, D = 32, 16, 8, 48, env.obs_dim
    online, target = _dqn_pair(env, 7)
    ring = env.replay_torch(T, term_capacity=T * B)
    env.replay_begin_torch(ring, env.reset_torch())
    term = env.terminal_list_torch(K * B)
    rows = ring.rows(K)
    first = torch.empty((K + 1, B, D), device="cuda")  # the first action's observation is the ring's last slot, not adjacent to slot 0
    first[0].copy_(ring.obs[T - 1])
    env.rollout_dqn_torch(online, first, rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=2, first_step=0, epsilon=0.5, terminal=term)
    rows["obs"].copy_(first[1:])
    env.replay_commit_torch(ring, K, terminal=term)
    rows = ring.rows(K)
    env.rollout_dqn_torch(online, ring.obs[K - 1:T], rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=2, first_step=K, epsilon=0.5,
                          terminal=term)
    env.replay_commit_torch(ring, K, terminal=term)
    mu_col = _dev(np.random.default_rng(4).uniform(0.2, 1.0, (T, B)).astype(np.float32))  # (stands for the behaviour probabilities)
    seq = env.replay_sample_sequences_torch(ring, n, Ls, seed=11, columns=[mu_col])
    mu = seq["columns"][0]
    env.check_status()
    done, trunc = _host(seq["done"], seq["trunc"])
    assert (done != 0).any() and (trunc != 0).any() and not done.all()
    weight = _dev(np.random.default_rng(5).uniform(0.2, 1.0, n).astype(np.float32))
    real = env.retrace_torch

    def modelled(reward, done, trunc, q, value, **kw):
        h = lambda v: None if v is None else v.cpu().numpy()  # noqa: E731
        loss = kw.pop("loss")
        out = retrace_model(h(reward), h(done), h(trunc), h(q), h(value), last_value=h(kw.pop("last_value")), ratio=h(kw.pop("ratio")),
                            terminal_value=h(kw.pop("terminal_value")),
                            loss=dict(q_online=h(loss["q_online"]), weight=h(loss["weight"]), huber_delta=loss["huber_delta"]), **kw)
        return tuple(_dev(o) for o in out)
    targets = {}
    for trace in env.retrace_traces:
        for epsilon in (0.0, 0.1):
            kw = dict(mu=mu if trace in ("retrace", "is") else None, trace=trace, epsilon=epsilon, gamma=0.97, lam=0.9, huber_delta=1.0, weight=weight)
            env.retrace_torch = real
            grads, got = env.dqn_retrace_grad_torch(online, target, seq, **kw)
            grads = [tuple(x.clone() for x in pair) for pair in grads["net"]]
            env.retrace_torch = modelled
            try:
                want_grads, want = env.dqn_retrace_grad_torch(online, target, seq, **kw)
            finally:
                env.retrace_torch = real
            torch.cuda.synchronize()
            for k in ("target", "td_error", "g"):
                assert _equal(*_host(got[k], want[k])), (trace, epsilon, k)
            for (gw, gb), (ww, wb) in zip(grads, want_grads["net"]):
                assert torch.equal(gw, ww) and torch.equal(gb, wb) and float(gw.abs().max()) > 0.0, (trace, epsilon)
            targets[trace, epsilon] = _host(got["target"])[0]
    # the estimators differ: under the greedy policy retrace, tree backup and Watkins coincide (min(1, [greedy] / mu) = [greedy]); the rest do not
    assert len({v.tobytes() for v in targets.values()}) >= 6
    env.check_status()


def test_native_refusals_write_nothing(env):
    """every refusal of the C call, into NaN-prefilled outputs; then the same arguments, accepted"""
    import torch
    from space_gym_amd import _native
    Ls, n = 9, 65
    s, x = retrace_case(Ls, n)
    t = {k: _dev(v) for k, v in s.items()}
    ratio, q_online, weight = _dev(x["ratio"]), _dev(x["q_online"]), _dev(x["weight"])
    out = dict(target=_nan(Ls, n), td=_nan(Ls, n), g=_nan(Ls, n))
    p = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None  # noqa: E731
    disc = _dev(np.array([0.9, 0.8], np.float32))

    def cfg(**over):
        c = _native.SgRetraceConfig()
        env._lib.sg_retrace_config_init(C.byref(c))
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)

    def call(c, length=Ls, cols=n, q_on=q_online, w=weight, td=out["td"], g=out["g"], **over):
        a = dict(reward=t["reward"], done=t["done"], trunc=t["trunc"], q=t["q"], value=t["value"], target=out["target"])
        a.update(over)
        return env._lib.sg_retrace_device(env._h, length, cols, c, p(a["reward"]), p(a["done"]), p(a["trunc"]), p(a["q"]), p(a["value"]),
                                          p(t["last_value"]), p(ratio), p(t["terminal_value"]), p(a["target"]), p(q_on), p(w), p(td), p(g), None)
    c0 = _native.SgRetraceConfig()
    env._lib.sg_retrace_config_init(C.byref(c0))
    assert (c0.struct_size, c0.gamma, c0.lambda_, c0.c_bar, c0.bootstrap_truncated, c0.huber_delta, c0.discounts, c0.reserved) == (
        56, 0.99, 1.0, 1.0, 1, INF, None, 0)
    nan = float("nan")
    cases = [("null cfg", lambda: call(None)), ("struct_size", lambda: call(cfg(struct_size=48))), ("reserved", lambda: call(cfg(reserved=1))),
             ("length", lambda: call(cfg(), length=0)), ("n = ", lambda: call(cfg(), cols=0)), ("n = ", lambda: call(cfg(), cols=-5)),
             ("2^31 - 1", lambda: call(cfg(), length=1 << 16, cols=1 << 15)),
             *[("null reward", lambda k=k: call(cfg(), **{k: None})) for k in ("reward", "done", "trunc", "q", "value", "target")],
             ("gamma", lambda: call(cfg(gamma=1.5))), ("gamma", lambda: call(cfg(gamma=nan))), ("lambda", lambda: call(cfg(lambda_=-0.5))),
             ("lambda", lambda: call(cfg(lambda_=nan))), ("c_bar", lambda: call(cfg(c_bar=0.0))), ("c_bar", lambda: call(cfg(c_bar=nan))),
             ("huber_delta", lambda: call(cfg(huber_delta=0.0))), ("huber_delta", lambda: call(cfg(huber_delta=nan))),
             ("without q_online", lambda: call(cfg(), q_on=None)), ("without q_online", lambda: call(cfg(), q_on=None, w=None, g=None)),
             ("weight given without g", lambda: call(cfg(), g=None))]
    for match, run in cases:
        assert run() == -1, match
        assert match in env._lib.sg_last_error(env._h).decode(), (match, env._lib.sg_last_error(env._h))
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in out.values())
    env.check_status()
    # accepted: out-of-range scalars beside a discounts tensor (not read), c_bar and huber_delta of +inf
    assert call(cfg(gamma=7.0, lambda_=nan, discounts=disc.data_ptr(), c_bar=INF, huber_delta=INF)) == 0
    _same(_host(out["target"], out["td"], out["g"]),
          retrace_model(**s, ratio=x["ratio"], discounts=np.array([0.9, 0.8], np.float32), c_bar=np.inf,
                        loss=dict(q_online=x["q_online"], weight=x["weight"], huber_delta=np.inf)), "accepted")
    env.check_status()
