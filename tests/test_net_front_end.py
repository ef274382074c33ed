"""Characterisation of the Python front end of the seven net families (policy, population, PPO, Q, policy_action, squashed, DQN) with
the native library stubbed: for every public method, called once with out=None and once with the caller's tensors, on a continuous
and on a discrete stub where the method serves both -- the native function, its full argument tuple (pointers against data_ptr()),
the shapes and dtypes of what the method allocates, and the value returned.  For the six autograd forms: which *_grad_torch arguments
are None and which parameters get no gradient, for every subset of outputs a loss uses."""
import ctypes as C
import itertools

import pytest

from test_episode_stats import _StubLib, _fake_cuda, _stub_env

B, D, H, K, N, P, CAP, WS = 8, 13, 16, 3, 24, 4, 10, 64  # envs, obs width, hidden, steps, rows, members, list capacity, workspace bytes


class _Lib(_StubLib):
    """_StubLib whose *_grad_workspace_bytes queries answer WS"""

    def __getattr__(self, name):
        fn = _StubLib.__getattr__(self, name)
        if not name.endswith("_workspace_bytes"):
            return fn

        def sized(*args):
            fn(*args)
            return WS
        return sized


@pytest.fixture
def torch(monkeypatch):
    """torch with empty(..., device=cuda) served by the CPU, as the tensors of _fake_cuda are"""
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: _fake_cuda(real(*a, **k)))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return torch


def _env(discrete=False):
    env = _stub_env(B=B, D=D)
    env._lib, env.discrete = _Lib(), discrete
    return env


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _net(fan_in, out, lead=()):
    dims = [fan_in, H, H, out]
    return [(_z(*lead, o, i), _z(*lead, o)) for i, o in zip(dims[:-1], dims[1:])]


def _like(pairs):
    return [(_z(*w.shape), _z(*b.shape)) for w, b in pairs]


def _actor_critic(discrete, critic=True, lead=()):
    return dict(actor=_net(D, 6 if discrete else 2, lead), critic=_net(D, 1, lead) if critic else None, log_std=None if discrete else _z(*lead, 2))


def _action(discrete, *lead):
    import torch
    return _z(*lead, dtype=torch.int32) if discrete else _z(*lead, 2)


def _norm(a):
    """a ctypes argument as a comparable value: a pointer's address, a byref's object, anything else as it is"""
    if isinstance(a, C.c_void_p):
        return a.value
    return a._obj if hasattr(a, "_obj") else a


def _values(s):
    """a ctypes structure as nested tuples"""
    if isinstance(s, C.Structure):
        return tuple(_values(getattr(s, f[0])) for f in s._fields_)
    return tuple(_values(x) for x in s) if isinstance(s, C.Array) else s


def _mlp(pairs):
    pad = (None,) * (4 - len(pairs or ()))
    return tuple(w.data_ptr() for w, _ in pairs or ()) + pad, tuple(b.data_ptr() for _, b in pairs or ()) + pad


def _p(t):
    return None if t is None else t.data_ptr()


def _calls(env, fn, *args, **kw):
    """(what fn returns, the native calls it made as (name, normalised arguments))"""
    env._lib.calls.clear()
    ret = fn(*args, **kw)
    return ret, [(name, tuple(_norm(a) for a in a_)) for name, a_ in env._lib.calls]


def _is(t, torch, dtype, *shape):
    return isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape


def _terminal(torch):
    return dict(count=_z(1, dtype=torch.int32), step_env=_z(CAP, 2, dtype=torch.int32), obs=_z(CAP, D))


def _roll(torch, discrete, value=True):
    u8 = torch.uint8
    return dict(obs=_z(K + 1, B, D), action=_action(discrete, K, B), logp=_z(K, B), value=_z(K + 1, B) if value else None, reward=_z(K, B),
                done=_z(K, B, dtype=u8), trunc=_z(K, B, dtype=u8))


def _tl_values(terminal):
    return (_p(terminal["count"]), _p(terminal["step_env"]), _p(terminal["obs"]), CAP)


# ---------------------------------------------------------------------------------------------- act
@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("critic", [True, False])
def test_policy_and_population_act(torch, discrete, critic):
    env = _env(discrete)
    par, spar = _actor_critic(discrete, critic), _actor_critic(discrete, critic, (P,))
    pol, pop = env.policy_torch(**par), env.policy_population_torch(P, **spar)
    obs = _z(B, D)
    a_dtype, a_shape = (torch.int32, (B,)) if discrete else (torch.float32, (B, 2))
    for method, handle, name, members in ((env.policy_act_torch, pol, "sg_policy_act_device", ()),
                                          (env.population_act_torch, pop, "sg_policy_population_act_device", (P,))):
        (a, lp, v), calls = _calls(env, method, handle, obs)
        assert _is(a, torch, a_dtype, *a_shape) and _is(lp, torch, torch.float32, B) and (_is(v, torch, torch.float32, B) if critic else v is None)
        assert calls == [(name, (1, handle.struct, *members, _p(obs), 0, 0, 0, _p(a), _p(lp), _p(v), None))]
        out = dict(action=_action(discrete, B), logp=_z(B), value=_z(B) if critic else None)
        ret, calls = _calls(env, method, handle, obs, seed=3, step=2 ** 33, deterministic=True, out=out)
        assert ret[0] is out["action"] and ret[1] is out["logp"] and ret[2] is out["value"]
        assert calls == [(name, (1, handle.struct, *members, _p(obs), 3, 2 ** 33, 1, _p(out["action"]), _p(out["logp"]), _p(out["value"]), None))]
    # the two differ: the single policy needs out['action'], the population serves the values alone
    if critic:
        value = _z(B)
        with pytest.raises(KeyError, match="action"):
            env.policy_act_torch(pol, obs, out=dict(value=value))
        ret, calls = _calls(env, env.population_act_torch, pop, obs, out=dict(value=value, logp=_z(B)))
        assert ret == (None, None, value)
        assert calls == [("sg_policy_population_act_device", (1, pop.struct, P, _p(obs), 0, 0, 0, None, None, _p(value), None))]
    else:
        with pytest.raises(ValueError, match=r"out\['value'\]: the policy has no critic"):
            env.policy_act_torch(pol, obs, out=dict(action=_action(discrete, B), logp=_z(B), value=_z(B)))
        with pytest.raises(ValueError, match=r"out\['value'\]: the population has no critic"):
            env.population_act_torch(pop, obs, out=dict(action=_action(discrete, B), logp=_z(B), value=_z(B)))
    with pytest.raises(ValueError, match="out: expected action \\(with logp\\), value, or both"):
        env.population_act_torch(pop, obs, out={})


def test_squashed_and_dqn_act(torch):
    env = _env()
    sp = env.squashed_policy_torch(_net(D, 4))
    obs = _z(B, D)
    (a, lp), calls = _calls(env, env.squashed_act_torch, sp, obs)
    assert _is(a, torch, torch.float32, B, 2) and _is(lp, torch, torch.float32, B)
    assert calls == [("sg_squashed_act_device", (1, sp.struct, _p(obs), 0, 0, 0, _p(a), _p(lp), None))]
    out = dict(action=_z(B, 2))
    ret, calls = _calls(env, env.squashed_act_torch, sp, obs, seed=5, step=6, deterministic=1, out=out)
    assert ret[0] is out["action"] and ret[1] is None
    assert calls == [("sg_squashed_act_device", (1, sp.struct, _p(obs), 5, 6, 1, _p(out["action"]), None, None))]
    with pytest.raises(ValueError, match=r"out\['action'\]: expected a float32 \[n, 2\] tensor"):
        env.squashed_act_torch(sp, obs, out=dict(logp=_z(B)))
    env = _env(discrete=True)
    dqn = env.dqn_torch(_net(D, 6))
    (a, q), calls = _calls(env, env.dqn_act_torch, dqn, obs)
    assert _is(a, torch, torch.int32, B) and _is(q, torch, torch.float32, B)
    assert calls == [("sg_dqn_act_device", (1, dqn.struct, _p(obs), 0, 0, 0.0, None, _p(a), _p(q), None))]
    out, eps = dict(action=_z(B, dtype=torch.int32)), _z(B)
    ret, calls = _calls(env, env.dqn_act_torch, dqn, obs, seed=5, step=6, epsilon=eps, out=out)
    assert ret[0] is out["action"] and ret[1] is None
    assert calls == [("sg_dqn_act_device", (1, dqn.struct, _p(obs), 5, 6, 0.0, _p(eps), _p(out["action"]), None, None))]
    assert _calls(env, env.dqn_act_torch, dqn, obs, epsilon=0.25, out=dict(out, q=_z(B)))[1][0][1][5] == 0.25
    with pytest.raises(ValueError, match=r"out\['action'\]: expected an int32 \[num_envs\] tensor"):
        env.dqn_act_torch(dqn, obs, out=dict(q=_z(B)))


# ---------------------------------------------------------------------------------------------- closed-loop rollouts
@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("critic", [True, False])
def test_policy_and_population_rollout(torch, discrete, critic):
    env = _env(discrete)
    pol = env.policy_torch(**_actor_critic(discrete, critic))
    pop = env.policy_population_torch(P, **_actor_critic(discrete, critic, (P,)))
    r = _roll(torch, discrete, critic)
    cols = tuple(_p(r[k]) for k in ("obs", "action", "logp", "value", "reward", "done", "trunc"))
    for method, handle, name, members in ((env.rollout_policy_torch, pol, "sg_rollout_policy_device", ()),
                                          (env.rollout_population_torch, pop, "sg_rollout_policy_population_device", (P,))):
        ret, calls = _calls(env, method, handle, **r)
        assert len(ret) == 7 and all(x is r[k] for x, k in zip(ret, ("obs", "action", "logp", "value", "reward", "done", "trunc")))
        assert calls == [(name, (1, K, handle.struct, *members, 0, 0, 0, *cols, None, None, None))]
    # the single policy's terminal values go to the list, made on first use; a population's are a dense [K, B] argument
    term = _terminal(torch)
    _, calls = _calls(env, env.rollout_policy_torch, pol, **r, seed=5, first_step=7, deterministic=True, terminal=term)
    (name, args), = calls
    assert name == "sg_rollout_policy_device" and args[:13] == (1, K, pol.struct, 5, 7, 1, *cols) and args[15] is None
    assert _values(args[13]) == _tl_values(term)
    if critic:
        assert _is(term["value"], torch, torch.float32, CAP) and args[14] == _p(term["value"])
        given = dict(_terminal(torch), value=_z(CAP))
        assert _calls(env, env.rollout_policy_torch, pol, **r, terminal=given)[1][0][1][14] == _p(given["value"])
    else:
        assert "value" not in term and args[14] is None
    term, tv = _terminal(torch), _z(K, B) if critic else None
    _, calls = _calls(env, env.rollout_population_torch, pop, **r, seed=5, first_step=7, terminal=term, terminal_value=tv)
    (name, args), = calls
    assert name == "sg_rollout_policy_population_device" and args[:14] == (1, K, pop.struct, P, 5, 7, 0, *cols) and args[15:] == (_p(tv), None)
    assert _values(args[14]) == _tl_values(term) and "value" not in term
    for method, handle, noun in ((env.rollout_policy_torch, pol, "policy"), (env.rollout_population_torch, pop, "population")):
        with pytest.raises(ValueError, match="action: expected a CUDA tensor of at least one step"):
            method(handle, **dict(r, action=_z(K)))
        with pytest.raises(ValueError, match=f"the {noun} has " + ("a critic; pass the float32" if critic else "no critic")):
            method(handle, **dict(r, value=None if critic else _z(K + 1, B)))
        with pytest.raises(ValueError, match=r"terminal\['count'\]: expected one 32-bit integer"):
            method(handle, **r, terminal=dict(_terminal(torch), count=_z(2, dtype=torch.int32)))


def test_squashed_and_dqn_rollout(torch):
    env = _env()
    sp = env.squashed_policy_torch(_net(D, 4))
    r = {k: v for k, v in _roll(torch, False).items() if k != "value"}
    cols = tuple(_p(r[k]) for k in ("obs", "action", "logp", "reward", "done", "trunc"))
    ret, calls = _calls(env, env.rollout_squashed_torch, sp, **r)
    assert all(x is r[k] for x, k in zip(ret, ("obs", "action", "logp", "reward", "done", "trunc"))) and len(ret) == 6
    assert calls == [("sg_rollout_squashed_device", (1, K, sp.struct, 0, 0, 0, *cols, None, None))]
    term = _terminal(torch)
    ret, calls = _calls(env, env.rollout_squashed_torch, sp, **dict(r, logp=None), seed=2, first_step=9, deterministic=True, terminal=term)
    (name, args), = calls
    assert ret[2] is None and args[:12] == (1, K, sp.struct, 2, 9, 1, cols[0], cols[1], None, *cols[3:]) and args[13] is None
    assert _values(args[12]) == _tl_values(term)
    with pytest.raises(ValueError, match=r"action: expected a CUDA tensor \[K, B, 2\] of at least one step"):
        env.rollout_squashed_torch(sp, **dict(r, action=_z(K, B)))
    env = _env(discrete=True)
    dqn = env.dqn_torch(_net(D, 6))
    r = {k: v for k, v in _roll(torch, True).items() if k not in ("value", "logp")}
    q = _z(K, B)
    ret, calls = _calls(env, env.rollout_dqn_torch, dqn, **r)
    assert len(ret) == 6 and ret[2] is None and all(x is r[k] for x, k in zip(ret, ("obs", "action", None, "reward", "done", "trunc")) if k)
    assert calls == [("sg_rollout_dqn_device", (1, K, dqn.struct, 0, 0, 0.0, None, _p(r["obs"]), _p(r["action"]), None, _p(r["reward"]),
                                                _p(r["done"]), _p(r["trunc"]), None, None))]
    term, eps = _terminal(torch), _z(B)
    ret, calls = _calls(env, env.rollout_dqn_torch, dqn, **r, q=q, seed=2, first_step=9, epsilon=eps, terminal=term)
    (name, args), = calls
    assert ret[2] is q and args[:13] == (1, K, dqn.struct, 2, 9, 0.0, _p(eps), _p(r["obs"]), _p(r["action"]), _p(q), _p(r["reward"]), _p(r["done"]),
                                         _p(r["trunc"])) and args[14] is None
    assert _values(args[13]) == _tl_values(term)
    with pytest.raises(ValueError, match=r"action: expected a CUDA tensor \[K, B\] of at least one step"):
        env.rollout_dqn_torch(dqn, **dict(r, action=_z(K, B, 1, dtype=torch.int32)))


# ---------------------------------------------------------------------------------------------- evaluate_raw and grad
def _grads_values(actor, critic, log_std):
    return (C.sizeof(_policy_grads()), 0, _mlp(actor), _mlp(critic), _p(log_std))


def _policy_grads():
    from space_gym_amd import _native
    return _native.SgPolicyGrads


@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("critic", [True, False])
def test_policy_and_population_evaluate_and_grad(torch, discrete, critic):
    env = _env(discrete)
    f32 = torch.float32
    for lead, make, prefix, native, noun in (((), env.policy_torch, "policy", "sg_policy", "policy"),
                                             ((P,), lambda **par: env.policy_population_torch(P, **par), "population", "sg_policy_population", "population")):
        par = _actor_critic(discrete, critic, lead)
        handle = make(**par)
        evaluate, grad = getattr(env, prefix + "_evaluate_raw_torch"), getattr(env, prefix + "_grad_torch")
        obs, action = _z(*lead, N, D), _action(discrete, *lead, N)
        ret, calls = _calls(env, evaluate, handle, obs, action)
        assert all(_is(t, torch, f32, *lead, N) for t in ret[:2]) and (_is(ret[2], torch, f32, *lead, N) if critic else ret[2] is None)
        assert calls == [(native + "_evaluate_device", (1, handle.struct, *lead, N, _p(obs), _p(action), *(_p(t) for t in ret), None))]
        out = dict(entropy=_z(*lead, N), value=_z(*lead, N) if critic else None)
        ret, calls = _calls(env, evaluate, handle, obs, action, out=out)
        assert ret[0] is None and ret[1] is out["entropy"] and ret[2] is out["value"]
        assert calls == [(native + "_evaluate_device", (1, handle.struct, *lead, N, _p(obs), _p(action), None, _p(out["entropy"]), _p(out["value"]), None))]
        with pytest.raises(ValueError, match="out: expected at least one of logp, entropy, value"):
            evaluate(handle, obs, action, out={})
        if not critic:
            with pytest.raises(ValueError, match=rf"out\['value'\]: the {noun} has no critic"):
                evaluate(handle, obs, action, out=dict(value=_z(*lead, N)))
        # grad: the workspace query, then the call; critic gradients only with g_value
        for g_value in ((None, _z(*lead, N)) if critic else (None,)):
            g_logp = _z(*lead, N)
            handle.workspace = None
            ret, calls = _calls(env, grad, handle, obs, action, g_logp=g_logp, g_value=g_value)
            assert set(ret) == {"actor", "critic", "log_std"} and (ret["critic"] is None) == (g_value is None) and (ret["log_std"] is None) == discrete
            for got, like in ((ret["actor"], par["actor"]), (ret["critic"], par["critic"] if g_value is not None else None)):
                assert got is None and like is None or [(tuple(w.shape), tuple(b.shape), w.dtype) for w, b in got] == [
                    (tuple(w.shape), tuple(b.shape), f32) for w, b in like]
            assert discrete or _is(ret["log_std"], torch, f32, *lead, 2)
            ws = handle.workspace
            assert _is(ws, torch, torch.uint8, WS)
            (qname, qargs), (name, args) = calls
            assert (qname, qargs) == (native + "_grad_workspace_bytes", (1, handle.struct, *lead, N))
            k = 2 + len(lead)
            assert name == native + "_grad_device" and args[:k] == (1, handle.struct, *lead)
            assert args[k:k + 6] == (N, _p(obs), _p(action), _p(g_logp), None, _p(g_value)) and args[k + 7:] == (_p(ws), WS, None)
            assert _values(args[k + 6]) == _grads_values(ret["actor"], ret["critic"], ret["log_std"])
            out = dict(actor=_like(par["actor"]), critic=_like(par["critic"]) if critic else None, log_std=None if discrete else _z(*lead, 2))
            ret, calls = _calls(env, grad, handle, obs, action, g_entropy=g_logp, g_value=g_value, out=out)
            assert ret is out and handle.workspace is ws and calls[1][1][k + 3:k + 6] == (None, _p(g_logp), _p(g_value))
            assert _values(calls[1][1][k + 6]) == _grads_values(out["actor"], out["critic"], out["log_std"])  # a given critic is passed on, with or without g_value
        if critic:
            with pytest.raises(ValueError, match=r"out\['critic'\]: g_value is given; the critic's gradients need tensors"):
                grad(handle, obs, action, g_value=_z(*lead, N), out=dict(out, critic=None))
        else:
            with pytest.raises(ValueError, match=rf"g_value: the {noun} has no critic"):
                grad(handle, obs, action, g_value=_z(*lead, N))
            with pytest.raises(ValueError, match=rf"out\['critic'\]: the {noun} has no critic"):
                grad(handle, obs, action, out=dict(out, critic=_like(_net(D, 1, lead))))
        if not discrete:
            with pytest.raises(ValueError, match=r"out\['log_std'\]: expected a float32 \[" + ("4, 2" if lead else "2") + r"\] tensor"):
                grad(handle, obs, action, out=dict(out, log_std=None))


@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("critic", [True, False])
def test_ppo_grad(torch, discrete, critic):
    from space_gym_amd import _native
    env = _env(discrete)
    par = _actor_critic(discrete, critic)
    pol = env.policy_torch(**par)
    R = 40
    batch = dict(obs=_z(R, D), action=_action(discrete, R), logp=_z(R), advantage=_z(R), ret=_z(R), value=_z(R))
    (grads, stats), calls = _calls(env, env.ppo_grad_torch, pol, batch)
    assert (grads["critic"] is None) == (not critic) and (grads["log_std"] is None) == discrete and _is(stats, torch, torch.float32, 12)
    (n0, a0), (n1, a1), (n2, a2) = calls
    assert n0 == "sg_ppo_config_init" and isinstance(a0[0], _native.SgPpoConfig)
    assert (n1, a1) == ("sg_ppo_grad_workspace_bytes", (1, pol.struct, R))
    assert n2 == "sg_ppo_grad_device" and a2[:2] == (1, pol.struct) and a2[2] is a0[0] and a2[4:6] == (R, R)
    assert a2[7:] == (_p(stats), None, _p(pol.workspace), WS, None)
    assert _values(a2[3]) == (_p(batch["obs"]), _p(batch["action"]), _p(batch["logp"]), _p(batch["advantage"]), _p(batch["ret"]) if critic else None, None, None)
    assert _values(a2[6]) == _grads_values(grads["actor"], grads["critic"], grads["log_std"])
    index, given, rows = _z(N, dtype=torch.int64), _z(12), dict(logp=_z(N), g_logp=_z(N))
    out = dict(actor=_like(par["actor"]), critic=_like(par["critic"]) if critic else None, log_std=None if discrete else _z(2))
    (grads, stats), calls = _calls(env, env.ppo_grad_torch, pol, batch, index, clip_range_vf=0.2, out=out, stats=given, rows=rows)
    a2 = calls[2][1]
    assert grads is out and stats is given and a2[4:6] == (R, N) and a2[7] == _p(given)
    assert _values(a2[3])[5:] == (_p(batch["value"]) if critic else None, _p(index)) and _values(a2[8]) == (_p(rows["logp"]), None, _p(rows["g_logp"]), None)
    assert _values(a2[6]) == _grads_values(out["actor"], out["critic"], out["log_std"])
    # unlike policy_grad_torch, a critic's gradients are needed whenever there is a critic
    if critic:
        with pytest.raises(ValueError, match=r"out\['critic'\]: the policy has a critic; its gradients need tensors"):
            env.ppo_grad_torch(pol, batch, out=dict(out, critic=None))
    else:
        with pytest.raises(ValueError, match=r"out\['critic'\]: the policy has no critic"):
            env.ppo_grad_torch(pol, batch, out=dict(out, critic=_like(_net(D, 1))))
    # ppo_assign_grads: the tensors become the parameters' .grad in parameter order; a net without gradients keeps its own
    env.ppo_assign_grads(pol, out)
    flat = [t for pair in out["actor"] + (out["critic"] or []) for t in pair] + ([] if discrete else [out["log_std"]])
    assert len(flat) == len(pol.tensors) and all(p.grad is g for p, g in zip(pol.tensors, flat))
    if critic:
        for p in pol.tensors:
            p.grad = None
        env.ppo_assign_grads(pol, dict(out, critic=None))
        assert [p.grad is None for p in pol.tensors] == [False] * 6 + [True] * 6 + [False] * (not discrete)


def test_q_and_policy_action(torch):
    from space_gym_amd import _native
    env = _env()
    f32 = torch.float32
    obs, action = _z(N, D), _z(N, 2)
    for n_critics in (2, 1):
        nets = [_net(D + 2, 1) for _ in range(n_critics)]
        q = env.q_torch(nets)
        ret, calls = _calls(env, env.q_evaluate_raw_torch, q, obs, action)
        assert _is(ret[0], torch, f32, N) and (_is(ret[1], torch, f32, N) if n_critics == 2 else ret[1] is None)
        assert calls == [("sg_q_evaluate_device", (1, q.struct, N, _p(obs), _p(action), _p(ret[0]), _p(ret[1]), None))]
        out = dict(q2=_z(N)) if n_critics == 2 else dict(q1=_z(N))
        ret, calls = _calls(env, env.q_evaluate_raw_torch, q, obs, action, out=out)
        assert ret == (out.get("q1"), out.get("q2")) and calls[0][1][5:7] == (_p(out.get("q1")), _p(out.get("q2")))
        with pytest.raises(ValueError, match="out: expected at least one of q1, q2"):
            env.q_evaluate_raw_torch(q, obs, action, out={})
        g1 = _z(N)
        ret, calls = _calls(env, env.q_grad_torch, q, obs, action, g_q1=g1)
        assert ret["action"] is None and [[tuple(w.shape) for w, _ in net] for net in ret["critics"]] == [[tuple(w.shape) for w, _ in net] for net in nets]
        (qname, qargs), (name, args) = calls
        assert (qname, qargs) == ("sg_q_grad_workspace_bytes", (1, q.struct, N))
        assert name == "sg_q_grad_device" and args[:7] == (1, q.struct, N, _p(obs), _p(action), _p(g1), None) and args[8:] == (None, _p(q.workspace), WS, None)
        pad = ((None,) * 4, (None,) * 4)
        assert _values(args[7]) == (C.sizeof(_native.SgQnetGrads), 0, tuple(_mlp(net) for net in ret["critics"]) + (pad,) * (2 - n_critics))
        ret, calls = _calls(env, env.q_grad_torch, q, obs, action, g_q1=g1, params=False, action_grad=True)
        assert ret["critics"] is None and _is(ret["action"], torch, f32, N, 2)
        assert calls == [("sg_q_grad_device", (1, q.struct, N, _p(obs), _p(action), _p(g1), None, None, _p(ret["action"]), None, 0, None))]
        out = dict(critics=[_like(net) for net in nets], action=_z(N, 2))
        ret, calls = _calls(env, env.q_grad_torch, q, obs, action, g_q1=g1, action_grad=True, out=out)
        assert ret["critics"] is out["critics"] and ret["action"] is out["action"] and calls[1][1][8] == _p(out["action"])
        assert _values(calls[1][1][7])[2][:n_critics] == tuple(_mlp(net) for net in out["critics"])
    for critic in (True, False):
        par = _actor_critic(False, critic)
        pol = env.policy_torch(**par)
        eps = _z(N, 2)
        a, calls = _calls(env, env.policy_action_raw_torch, pol, obs)
        assert _is(a, torch, f32, N, 2) and calls == [("sg_policy_action_device", (1, pol.struct, N, _p(obs), None, _p(a), None))]
        given = _z(N, 2)
        a, calls = _calls(env, env.policy_action_raw_torch, pol, obs, eps, out=given)
        assert a is given and calls == [("sg_policy_action_device", (1, pol.struct, N, _p(obs), _p(eps), _p(given), None))]
        g = _z(N, 2)
        ret, calls = _calls(env, env.policy_action_grad_torch, pol, obs, g, eps)
        assert set(ret) == {"actor", "log_std"} and _is(ret["log_std"], torch, f32, 2)
        assert calls[0] == ("sg_policy_grad_workspace_bytes", (1, pol.struct, N))
        name, args = calls[1]
        assert name == "sg_policy_action_grad_device" and args[:6] == (1, pol.struct, N, _p(obs), _p(eps), _p(g)) and args[7:] == (_p(pol.workspace), WS, None)
        assert _values(args[6]) == _grads_values(ret["actor"], None, ret["log_std"])
        out = dict(actor=_like(par["actor"]), log_std=_z(2))
        ret, calls = _calls(env, env.policy_action_grad_torch, pol, obs, g, out=out)
        assert ret is out and calls[1][1][4] is None and _values(calls[1][1][6]) == _grads_values(out["actor"], None, out["log_std"])
    denv = _env(discrete=True)
    with pytest.raises(ValueError, match="needs a continuous id"):
        denv.policy_action_raw_torch(denv.policy_torch(**_actor_critic(True)), obs)


def test_squashed_sample_and_grad(torch):
    from space_gym_amd import _native
    env = _env()
    f32 = torch.float32
    net = _net(D, 4)
    sp = env.squashed_policy_torch(net)
    obs, eps = _z(N, D), _z(N, 2)
    (a, lp), calls = _calls(env, env.squashed_sample_raw_torch, sp, obs)
    assert _is(a, torch, f32, N, 2) and _is(lp, torch, f32, N)
    assert calls == [("sg_squashed_sample_device", (1, sp.struct, N, _p(obs), None, _p(a), _p(lp), None))]
    out = dict(action=_z(N, 2))
    ret, calls = _calls(env, env.squashed_sample_raw_torch, sp, obs, eps, out=out)
    assert ret == (out["action"], None) and calls == [("sg_squashed_sample_device", (1, sp.struct, N, _p(obs), _p(eps), _p(out["action"]), None, None))]
    g_a, g_lp = _z(N, 2), _z(N)
    ret, calls = _calls(env, env.squashed_grad_torch, sp, obs, eps, g_action=g_a)
    assert list(ret) == ["actor"] and [(tuple(w.shape), tuple(b.shape)) for w, b in ret["actor"]] == [(tuple(w.shape), tuple(b.shape)) for w, b in net]
    assert calls[0] == ("sg_squashed_grad_workspace_bytes", (1, sp.struct, N))
    name, args = calls[1]
    assert name == "sg_squashed_grad_device" and args[:7] == (1, sp.struct, N, _p(obs), _p(eps), _p(g_a), None) and args[8:] == (_p(sp.workspace), WS, None)
    assert _values(args[7]) == (C.sizeof(_native.SgSquashedGrads), 0, _mlp(ret["actor"]))
    out = dict(actor=_like(net))
    ret, calls = _calls(env, env.squashed_grad_torch, sp, obs, g_logp=g_lp, out=out)
    assert ret is out and calls[1][1][4:7] == (None, None, _p(g_lp)) and _values(calls[1][1][7])[2] == _mlp(out["actor"])


def test_dqn_evaluate_and_grad(torch):
    from space_gym_amd import _native
    env = _env(discrete=True)
    f32, i32 = torch.float32, torch.int32
    net = _net(D, 6)
    dqn = env.dqn_torch(net)
    obs, action = _z(N, D), _z(N, dtype=i32)
    ret, calls = _calls(env, env.dqn_evaluate_raw_torch, dqn, obs)
    assert _is(ret[0], torch, f32, N, 6) and ret[1] is None and _is(ret[2], torch, f32, N) and _is(ret[3], torch, i32, N)
    assert calls == [("sg_dqn_evaluate_device", (1, dqn.struct, N, _p(obs), None, _p(ret[0]), None, _p(ret[2]), _p(ret[3]), None))]
    ret, calls = _calls(env, env.dqn_evaluate_raw_torch, dqn, obs, action)
    assert _is(ret[1], torch, f32, N) and calls[0][1][4:9] == (_p(action), *(_p(t) for t in ret))
    out = dict(q_taken=_z(N), argmax=_z(N, dtype=i32))
    ret, calls = _calls(env, env.dqn_evaluate_raw_torch, dqn, obs, action, out=out)
    assert ret == (None, out["q_taken"], None, out["argmax"]) and calls[0][1][5:9] == (None, _p(out["q_taken"]), None, _p(out["argmax"]))
    with pytest.raises(ValueError, match="out: expected at least one of q_all, q_taken, q_max, argmax"):
        env.dqn_evaluate_raw_torch(dqn, obs, out={})
    with pytest.raises(ValueError, match=r"action: out\['q_taken'\] is given"):
        env.dqn_evaluate_raw_torch(dqn, obs, out=out)
    g_t, g_a = _z(N), _z(N, 6)
    ret, calls = _calls(env, env.dqn_grad_torch, dqn, obs, action, g_taken=g_t)
    assert list(ret) == ["net"] and [(tuple(w.shape), tuple(b.shape)) for w, b in ret["net"]] == [(tuple(w.shape), tuple(b.shape)) for w, b in net]
    assert calls[0] == ("sg_dqn_grad_workspace_bytes", (1, dqn.struct, N))
    name, args = calls[1]
    assert name == "sg_dqn_grad_device" and args[:7] == (1, dqn.struct, N, _p(obs), _p(action), _p(g_t), None) and args[8:] == (_p(dqn.workspace), WS, None)
    assert _values(args[7]) == (C.sizeof(_native.SgDqnGrads), 0, _mlp(ret["net"]))
    out = dict(net=_like(net))
    ret, calls = _calls(env, env.dqn_grad_torch, dqn, obs, g_all=g_a, out=out)
    assert ret is out and calls[1][1][4:7] == (None, None, _p(g_a)) and _values(calls[1][1][7])[2] == _mlp(out["net"])


# ---------------------------------------------------------------------------------------------- the autograd forms
def _leaf(t):
    return t.requires_grad_()


def _subsets(k):
    return [s for r in range(k + 1) for s in itertools.combinations(range(k), r)]


def _loss(outputs, used):
    """the sum of the chosen outputs (as plain tensors: the stand-ins of CUDA tensors do not add); None when there is nothing to differentiate"""
    import torch
    terms = [outputs[i].as_subclass(torch.Tensor).sum() for i in used if outputs[i] is not None and outputs[i].requires_grad]
    return sum(terms[1:], terms[0]) if terms else None


def _none_mask(seq):
    return [x is None for x in seq]


@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("critic", [True, False])
@pytest.mark.parametrize("family", ["policy", "population"])
def test_policy_and_population_evaluate_autograd(torch, monkeypatch, family, discrete, critic):
    env = _env(discrete)
    lead = (P,) if family == "population" else ()
    par = _actor_critic(discrete, critic, lead)
    handle = env.policy_torch(**par) if not lead else env.policy_population_torch(P, **par)
    for t in handle.tensors:
        _leaf(t)
    obs, action = _z(*lead, N, D), _action(discrete, *lead, N)
    seen = []
    monkeypatch.setattr(env, family + "_evaluate_raw_torch", lambda h, o, a: tuple(_z(*lead, N) for _ in range(2)) + ((_z(*lead, N),) if critic else (None,)))

    def grad(h, o, a, g_logp=None, g_entropy=None, g_value=None):
        assert h is handle and o is obs and a is action
        for g in (g_logp, g_entropy, g_value):
            assert g is None or (g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (*lead, N))
        seen.append(_none_mask((g_logp, g_entropy, g_value)))
        return dict(actor=_like(par["actor"]), critic=_like(par["critic"]) if g_value is not None else None, log_std=None if discrete else _z(*lead, 2))
    monkeypatch.setattr(env, family + "_grad_torch", grad)
    L2 = 6
    for used in _subsets(3):
        for t in handle.tensors:
            t.grad = None
        seen.clear()
        outputs = getattr(env, family + "_evaluate_torch")(handle, obs, action)
        assert len(outputs) == 3 and (outputs[2] is None) == (not critic)
        loss = _loss(outputs, used)
        if loss is None:
            continue
        loss.backward()
        live = [i in used and outputs[i] is not None for i in range(3)]
        # the single policy's function materialises the gradients of unused outputs (zeros, not None); the population's passes None
        want = [False, False, not critic] if family == "policy" else [not x for x in live]
        assert seen == [want], (used, seen)
        got = _none_mask(t.grad for t in handle.tensors)
        critic_none = [want[2]] * L2 if critic else []
        assert got == [False] * L2 + critic_none + [False] * (not discrete), (used, got)
    # nothing needs a gradient: the plain forward, no backward call
    for t in handle.tensors:
        t.requires_grad_(False)
    seen.clear()
    assert not any(o is not None and o.requires_grad for o in getattr(env, family + "_evaluate_torch")(handle, obs, action)) and seen == []


@pytest.mark.parametrize("n_critics", [2, 1])
def test_q_evaluate_autograd(torch, monkeypatch, n_critics):
    env = _env()
    nets = [_net(D + 2, 1) for _ in range(n_critics)]
    q = env.q_torch(nets)
    obs = _z(N, D)
    seen = []
    monkeypatch.setattr(env, "q_evaluate_raw_torch", lambda h, o, a: (_z(N), _z(N) if n_critics == 2 else None))

    def grad(h, o, a, g_q1=None, g_q2=None, params=True, action_grad=False):
        assert h is q and o is obs
        seen.append((_none_mask((g_q1, g_q2)), params, action_grad))
        return dict(critics=[_like(net) for net in nets] if params else None, action=_z(N, 2) if action_grad else None)
    monkeypatch.setattr(env, "q_grad_torch", grad)
    for want_params, want_action in ((True, False), (False, True), (True, True)):
        for used in _subsets(2):
            for t in q.tensors:
                t.grad = None
                t.requires_grad_(want_params)
            action = _z(N, 2).requires_grad_(want_action)
            seen.clear()
            outputs = env.q_evaluate_torch(q, obs, action)
            assert len(outputs) == 2 and (outputs[1] is None) == (n_critics == 1)
            loss = _loss(outputs, used)
            if loss is None:
                continue
            loss.backward()
            live = [i in used and outputs[i] is not None for i in range(2)]
            assert seen == [([not x for x in live], want_params, want_action)], (used, seen)
            assert all((t.grad is not None) == want_params for t in q.tensors) and (action.grad is not None) == want_action


@pytest.mark.parametrize("critic", [True, False])
def test_policy_action_autograd(torch, monkeypatch, critic):
    env = _env()
    par = _actor_critic(False, critic)
    pol = env.policy_torch(**par)
    for t in pol.tensors:
        _leaf(t)
    obs = _z(N, D)
    seen = []
    monkeypatch.setattr(env, "policy_action_raw_torch", lambda h, o, e: _z(N, 2))

    def grad(h, o, g_action, eps=None):
        assert h is pol and o is obs and g_action.dtype == torch.float32 and g_action.is_contiguous()
        seen.append(eps)
        return dict(actor=_like(par["actor"]), log_std=_z(2))
    monkeypatch.setattr(env, "policy_action_grad_torch", grad)
    for eps in (None, _z(N, 2)):
        for t in pol.tensors:
            t.grad = None
        seen.clear()
        a = env.policy_action_torch(pol, obs, eps)
        a.sum().backward()
        assert len(seen) == 1 and seen[0] is eps
        assert _none_mask(t.grad for t in pol.tensors) == [False] * 6 + [True] * (6 if critic else 0) + [False]  # the critic is not involved
    for t in pol.tensors:
        t.requires_grad_(False)
    seen.clear()
    assert not env.policy_action_torch(pol, obs).requires_grad and seen == []


def test_squashed_sample_autograd(torch, monkeypatch):
    env = _env()
    net = _net(D, 4)
    sp = env.squashed_policy_torch(net)
    for t in sp.tensors:
        _leaf(t)
    obs = _z(N, D)
    seen = []
    monkeypatch.setattr(env, "squashed_sample_raw_torch", lambda h, o, e: (_z(N, 2), _z(N)))

    def grad(h, o, eps=None, g_action=None, g_logp=None):
        assert h is sp and o is obs
        seen.append((eps, _none_mask((g_action, g_logp))))
        return dict(actor=_like(net))
    monkeypatch.setattr(env, "squashed_grad_torch", grad)
    for eps in (None, _z(N, 2)):
        for used in _subsets(2):
            for t in sp.tensors:
                t.grad = None
            seen.clear()
            outputs = env.squashed_sample_torch(sp, obs, eps)
            loss = _loss(outputs, used)
            if loss is None:
                continue
            loss.backward()
            assert len(seen) == 1 and seen[0][0] is eps and seen[0][1] == [i not in used for i in range(2)], (used, seen)
            assert not any(_none_mask(t.grad for t in sp.tensors))


def test_dqn_evaluate_autograd(torch, monkeypatch):
    env = _env(discrete=True)
    net = _net(D, 6)
    dqn = env.dqn_torch(net)
    for t in dqn.tensors:
        _leaf(t)
    obs, action = _z(N, D), _z(N, dtype=torch.int32)
    seen, raw = [], []

    def evaluate(h, o, a=None, out=None):
        raw.append((a, sorted(out)))
        return out["q_all"], out.get("q_taken"), None, None
    monkeypatch.setattr(env, "dqn_evaluate_raw_torch", evaluate)

    def grad(h, o, a=None, g_taken=None, g_all=None):
        assert h is dqn and o is obs
        seen.append((a, _none_mask((g_taken, g_all))))
        return dict(net=_like(net))
    monkeypatch.setattr(env, "dqn_grad_torch", grad)
    # without an action: one output, q_all [n, 6]
    q_all = env.dqn_evaluate_torch(dqn, obs)
    assert _is(q_all, torch, torch.float32, N, 6) and raw == [(None, ["q_all"])]
    q_all.sum().backward()
    assert seen == [(None, [True, False])] and not any(_none_mask(t.grad for t in dqn.tensors))
    # with one: (q_all, q_taken); the action reaches the backward only with g_taken
    for used in _subsets(2)[1:]:
        for t in dqn.tensors:
            t.grad = None
        seen.clear()
        raw.clear()
        outputs = env.dqn_evaluate_torch(dqn, obs, action)
        assert len(outputs) == 2 and _is(outputs[1], torch, torch.float32, N) and raw == [(action, ["q_all", "q_taken"])]
        _loss(outputs, used).backward()
        assert len(seen) == 1 and seen[0][0] is (action if 1 in used else None) and seen[0][1] == [1 not in used, 0 not in used], (used, seen)
        assert not any(_none_mask(t.grad for t in dqn.tensors))


# ---------------------------------------------------------------------------------------------- the multi-device front ends
def test_the_multi_device_front_ends_refuse_every_net_method():
    """the names the tests of the seven families list, together"""
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    names = ("policy_torch", "policy_act_torch", "rollout_policy_torch", "policy_evaluate_torch", "policy_evaluate_raw_torch", "policy_grad_torch",
             "ppo_grad_torch", "ppo_assign_grads", "q_torch", "q_evaluate_torch", "q_evaluate_raw_torch", "q_grad_torch", "policy_action_torch",
             "policy_action_raw_torch", "policy_action_grad_torch", "squashed_policy_torch", "squashed_act_torch", "rollout_squashed_torch",
             "squashed_sample_torch", "squashed_sample_raw_torch", "squashed_grad_torch", "dqn_torch", "dqn_act_torch", "rollout_dqn_torch",
             "dqn_evaluate_torch", "dqn_evaluate_raw_torch", "dqn_grad_torch", "policy_population_torch", "population_member_torch",
             "population_act_torch", "rollout_population_torch", "population_evaluate_torch", "population_evaluate_raw_torch", "population_grad_torch")
    for cls, served in ((MultiDeviceVectorEnv, "one SpaceGymVectorEnv per device runs a policy on its envs"),
                        (ShardedVectorEnv, "a rank's SpaceGymVectorEnv runs a policy on its envs")):
        for name in names:
            with pytest.raises(NotImplementedError) as err:
                getattr(cls, name)(object.__new__(cls))
            assert str(err.value) == ("policy_torch / policy_act_torch / rollout_policy_torch: single-device front end only, not served by "
                                      f"{cls.__name__} ({served})")
