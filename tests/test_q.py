"""CPU tests of the Q critics and the actor's action chain (sg_q_evaluate_device / sg_q_grad_device / sg_policy_action_device /
sg_policy_action_grad_device): the declarations, the NumPy model (tests/q_model.py) against torch.autograd on float64 nn.Linear stacks,
the relu-at-zero convention, and the Python argument checks of q_torch / q_evaluate_raw_torch / q_grad_torch / policy_action_*_torch
with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from policy_model import random_policy
from q_model import action as action_model
from q_model import flat, grad_tolerances, q_evaluate, q_flat, random_qnet
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_snapshot_device import _header_args

NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS
REL = 1e-10  # float64 model against float64 autograd: section 18's figure for the same kind of comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    assert _header_args("sg_q_evaluate_device") == [
        "sg_env *env", "const sg_qnet *qnet", "int64_t n", "const float *obs", "const float *action", "float *q1_out", "float *q2_out",
        "void *hip_stream"]
    assert _header_args("sg_q_grad_device") == [
        "sg_env *env", "const sg_qnet *qnet", "int64_t n", "const float *obs", "const float *action", "const float *g_q1", "const float *g_q2",
        "const sg_qnet_grads *grads", "float *g_action_out", "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_q_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_qnet *qnet", "int64_t n"]
    assert _header_args("sg_policy_action_device") == [
        "sg_env *env", "const sg_policy *policy", "int64_t n", "const float *obs", "const float *eps", "float *action_out", "void *hip_stream"]
    assert _header_args("sg_policy_action_grad_device") == [
        "sg_env *env", "const sg_policy *policy", "int64_t n", "const float *obs", "const float *eps", "const float *g_action",
        "const sg_policy_grads *grads", "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    vp, Q, G = C.c_void_p, C.POINTER(_native.SgQnet), C.POINTER(_native.SgQnetGrads)
    P, PG = C.POINTER(_native.SgPolicy), C.POINTER(_native.SgPolicyGrads)
    assert _native.SYMBOLS["sg_q_evaluate_device"] == (C.c_int, [vp, Q, C.c_int64, vp, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_q_grad_device"] == (C.c_int, [vp, Q, C.c_int64, vp, vp, vp, vp, G, vp, vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_q_grad_workspace_bytes"] == (C.c_size_t, [vp, Q, C.c_int64])
    assert _native.SYMBOLS["sg_policy_action_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_policy_action_grad_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, PG, vp, C.c_size_t, vp])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls in (("sg_qnet", _native.SgQnet), ("sg_qnet_grads", _native.SgQnetGrads)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_], name
    assert C.sizeof(_native.SgQnet) == 24 + 2 * 64 and _native.SgQnet.critic.offset == 24
    assert C.sizeof(_native.SgQnetGrads) == 8 + 2 * 64 and _native.SgQnetGrads.critic.offset == 8
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_qnet.inc" in build.HEADERS and '#include "sg_qnet.inc"' in src


def _torch_q(critics, obs, act, g, activation):
    """Q_c, every parameter gradient and d / d action of sum_c sum_i g_c[i] Q_c[i] from torch.autograd on float64 nn.Linear stacks"""
    import torch
    nets = [_torch_net(layers, activation) for layers in critics]
    a = torch.from_numpy(act.astype(np.float64)).requires_grad_()
    x = torch.cat([torch.from_numpy(obs.astype(np.float64)), a], 1)
    qs = [net(x)[:, 0] for net in nets]
    sum((torch.from_numpy(np.asarray(gc, np.float64)) * q).sum() for gc, q in zip(g, qs)).backward()
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    grads = q_flat(dict(critics=[[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(net)] for net in nets]))
    return [q.detach().numpy() for q in qs], grads, a.grad.numpy()


@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", NETS)
def test_q_model_equals_torch_autograd_in_float64(hidden, n_hidden, activation, n_critics):
    rng = np.random.default_rng(hidden + 7 * n_hidden + n_critics)
    D, n = 13, 37
    obs = rng.standard_normal((n, D)).astype(np.float32)
    act = rng.standard_normal((n, 2)).astype(np.float32)
    critics = random_qnet(rng, D, hidden, n_hidden, n_critics)
    g = [rng.standard_normal(n) for _ in range(n_critics)]
    got = q_evaluate(critics, obs, act, *g, activation=activation)
    qs, grads, da = _torch_q(critics, obs, act, g, activation)
    for c in range(n_critics):
        assert rel(got["q"][c], qs[c]) <= REL
    assert n_critics == 2 or got["q"][1] is None
    mine = q_flat(got)
    assert set(mine) == set(grads)
    for k in grads:
        assert mine[k].shape == grads[k].shape and rel(mine[k], grads[k]) <= REL, (k, rel(mine[k], grads[k]))
    assert got["action"].shape == (n, 2) and rel(got["action"], da) <= REL


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", NETS)
def test_action_model_equals_torch_autograd_in_float64(hidden, n_hidden, activation):
    import torch
    rng = np.random.default_rng(hidden + 11 * n_hidden)
    D, n = 13, 37
    obs = rng.standard_normal((n, D)).astype(np.float32)
    pol = random_policy(rng, D, hidden, n_hidden, 2)
    eps, ga = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 2))
    actor = _torch_net(pol["actor"], activation)
    ls = torch.from_numpy(pol["log_std"].astype(np.float64)).requires_grad_()
    mean = actor(torch.from_numpy(obs.astype(np.float64)))
    a = mean + ls.exp() * torch.from_numpy(eps.astype(np.float64))
    (torch.from_numpy(ga) * a).sum().backward()
    lin = [m for m in actor if isinstance(m, torch.nn.Linear)]
    ref = flat(dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin], log_std=ls.grad.numpy()))
    got = action_model(pol, obs, eps, ga, activation=activation)
    assert rel(got["action"], a.detach().numpy()) <= REL
    mine = flat(got)
    assert set(mine) == set(ref)
    for k in ref:
        assert mine[k].shape == ref[k].shape and rel(mine[k], ref[k]) <= REL, (k, rel(mine[k], ref[k]))
    plain = action_model(pol, obs, None, ga, activation=activation)  # no noise: the mean, and no gradient reaches log_std
    assert rel(plain["action"], mean.detach().numpy()) <= REL and not plain["log_std"].any()


def test_float32_mode_is_float32_and_close():
    rng = np.random.default_rng(3)
    n, D = 300, 13
    obs, act = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    critics = random_qnet(rng, D, 33, 2)
    g = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    r64, r32 = q_evaluate(critics, obs, act, *g), q_evaluate(critics, obs, act, *g, dtype=np.float32)
    g64, g32 = q_flat(r64), q_flat(r32)
    g64["action"], g32["action"] = r64["action"], r32["action"]
    tol = grad_tolerances(g32, g64)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
    assert r32["q"][0].dtype == np.float32 and 0 < np.abs(r32["q"][0] - r64["q"][0]).max() < 1e-5


def test_relu_has_zero_slope_at_zero_as_torch():
    """a unit whose pre-activation is exactly 0 passes no gradient, to the parameters or to the action: relu'(0) = 0"""
    rng = np.random.default_rng(4)
    n, D = 9, 13
    obs, act = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    critics = random_qnet(rng, D, 5, 2)
    for layers in critics:
        W, b = layers[0]
        W[2] = 0.0
        b[2] = 0.0  # unit 2 of layer 0: pre-activation 0 for every row
    g = [rng.standard_normal(n) for _ in range(2)]
    got = q_evaluate(critics, obs, act, *g, activation="relu")
    named = q_flat(got)
    qs, ref, da = _torch_q(critics, obs, act, g, "relu")
    for c in range(2):
        assert not named[f"critic{c}.0.weight"][2].any() and named[f"critic{c}.0.bias"][2] == 0 and not named[f"critic{c}.1.weight"][:, 2].any()
        assert named[f"critic{c}.0.weight"][[0, 1, 3, 4]].any()
    for k in ref:
        assert np.allclose(named[k], ref[k], rtol=1e-10, atol=1e-14), k
    assert np.allclose(got["action"], da, rtol=1e-10, atol=1e-14)
    # one unit alone, its weights on the action set: at pre-activation 0 the action gets exactly nothing, just above it the unit's slope
    one = [[(np.array([[0.0] * D + [1.0, -2.0]], np.float32), np.zeros(1, np.float32)), (np.array([[3.0]], np.float32), np.zeros(1, np.float32))]]
    at_zero = q_evaluate(one, np.zeros((1, D), np.float32), np.array([[2.0, 1.0]], np.float32), np.ones(1), activation="relu")
    above = q_evaluate(one, np.zeros((1, D), np.float32), np.array([[2.5, 1.0]], np.float32), np.ones(1), activation="relu")
    assert not at_zero["action"].any() and np.array_equal(above["action"], [[3.0, -6.0]])


def _q_params(D=13, hidden=16, n_hidden=2, n_critics=2):
    import torch
    dims = [D + 2] + [hidden] * n_hidden + [1]
    return [[(_fake_cuda(torch.zeros((o, i))), _fake_cuda(torch.zeros(o))) for i, o in zip(dims[:-1], dims[1:])] for _ in range(n_critics)]


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def test_q_torch_builds_the_struct_over_the_callers_tensors():
    env = _stub_env()
    par = _q_params()
    q = env.q_torch(critics=par)
    s = q.struct
    assert (s.struct_size, s.n_critics, s.n_hidden, s.hidden, s.activation) == (152, 2, 2, 16, 1) and q.activation == "relu"
    for c in range(2):
        for l in range(3):
            assert s.critic[c].weight[l] == par[c][l][0].data_ptr() and s.critic[c].bias[l] == par[c][l][1].data_ptr()
        assert s.critic[c].weight[3] is None
    assert len(q.tensors) == 12 and q.tensors[6] is par[1][0][0] and q.workspace is None
    one = env.q_torch(critics=par[:1], activation="tanh")
    assert one.n_critics == 1 and one.struct.activation == 0 and one.struct.critic[1].weight[0] is None
    assert env._lib.names() == []  # a handle is made without a native call


def test_q_torch_refuses_what_the_kernel_cannot_take():
    import torch
    env = _stub_env()
    par = _q_params()
    with pytest.raises(ValueError, match="activation"):
        env.q_torch(critics=par, activation="gelu")
    with pytest.raises(ValueError, match="one or two nets"):
        env.q_torch(critics=par + par[:1])
    with pytest.raises(ValueError, match="one or two nets"):
        env.q_torch(critics=[])
    with pytest.raises(ValueError, match="n_hidden"):
        env.q_torch(critics=[par[0][-1:]])
    with pytest.raises(ValueError, match=r"critics\[0\]\[0\] weight"):
        env.q_torch(critics=[_params()["critic"]])  # a V critic: 13 inputs, not 15
    with pytest.raises(ValueError, match="hidden must be"):
        env.q_torch(critics=_q_params(hidden=129))
    with pytest.raises(ValueError, match=r"critics\[1\]: expected 2 hidden layers of width 16"):
        env.q_torch(critics=[par[0], _q_params(hidden=8)[0]])
    with pytest.raises(ValueError, match=r"critics\[1\]\[2\] weight"):
        env.q_torch(critics=[par[0], par[1][:2] + [(_z(2, 16), _z(1))]])
    with pytest.raises(ValueError, match=r"critics\[0\]\[1\] bias"):
        env.q_torch(critics=[[par[0][0], (par[0][1][0], _z(16, dtype=torch.float64)), par[0][2]]])
    with pytest.raises(ValueError, match=r"critics\[0\]\[0\] weight"):
        env.q_torch(critics=[[(torch.zeros((16, 15)), par[0][0][1])] + par[0][1:]])  # a CPU tensor
    with pytest.raises(ValueError, match=r"critics\[0\]\[0\] weight"):
        env.q_torch(critics=[[(_fake_cuda(torch.zeros((15, 16)).t()), par[0][0][1])] + par[0][1:]])  # not contiguous
    env.discrete = True
    with pytest.raises(ValueError, match="discrete ids are not served"):
        env.q_torch(critics=par)
    assert env._lib.names() == []


def test_evaluate_and_grad_check_their_tensors_before_the_native_call():
    env = _stub_env()
    par = _q_params()
    q, q_one = env.q_torch(critics=par), env.q_torch(critics=par[:1])
    n = 24  # a row count of its own, not num_envs (8)
    obs, act = _z(n, 13), _z(n, 2)
    out = dict(q1=_z(n), q2=_z(n))
    q1, q2 = env.q_evaluate_raw_torch(q, obs, act, out=out)
    assert q1 is out["q1"] and q2 is out["q2"]
    name, args = env._lib.calls[-1]
    assert name == "sg_q_evaluate_device" and args[2] == n and args[5].value == out["q1"].data_ptr() and args[6].value == out["q2"].data_ptr()
    assert env.q_evaluate_raw_torch(q_one, obs, act, out=dict(q1=out["q1"]))[1] is None and env._lib.calls[-1][1][6] is None
    # frozen critics: no gradient struct and no workspace are passed
    got = env.q_grad_torch(q, obs, act, g_q1=_z(n), params=False, action_grad=True, out=dict(action=_z(n, 2), critics="ignored"))
    name, args = env._lib.calls[-1]
    assert name == "sg_q_grad_device" and args[7] is None and args[8].value == got["action"].data_ptr() and args[9] is None and args[10] == 0
    assert got["critics"] is None and tuple(got["action"].shape) == (n, 2) and q.workspace is None
    env._lib.calls.clear()
    with pytest.raises(ValueError, match="handle q_torch returns"):
        env.q_evaluate_raw_torch(par, obs, act)
    with pytest.raises(ValueError, match="handle q_torch returns"):
        env.q_evaluate_torch(env.policy_torch(**_params()), obs, act)
    with pytest.raises(ValueError, match="obs"):
        env.q_evaluate_raw_torch(q, _z(n, 15), act)
    with pytest.raises(ValueError, match="obs"):
        env.q_evaluate_raw_torch(q, _z(0, 13), _z(0, 2))
    with pytest.raises(ValueError, match="action"):
        env.q_evaluate_raw_torch(q, obs, _z(n - 1, 2))
    with pytest.raises(ValueError, match="action"):
        env.q_evaluate_raw_torch(q, obs, _z(n, dtype=__import__("torch").int32))
    with pytest.raises(ValueError, match=r"out\['q2'\]: the handle has one critic"):
        env.q_evaluate_raw_torch(q_one, obs, act, out=out)
    with pytest.raises(ValueError, match="at least one"):
        env.q_evaluate_raw_torch(q, obs, act, out={})
    with pytest.raises(ValueError, match=r"out\['q1'\]"):
        env.q_evaluate_raw_torch(q, obs, act, out=dict(q1=_z(n + 1)))
    with pytest.raises(ValueError, match="g_q1"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n + 1))
    with pytest.raises(ValueError, match="g_q2: the handle has one critic"):
        env.q_grad_torch(q_one, obs, act, g_q2=_z(n))
    with pytest.raises(ValueError, match="nothing to compute"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), params=False)
    pairs = lambda net: [(_z(*w.shape), _z(*b.shape)) for w, b in net]
    good = dict(critics=[pairs(par[0]), pairs(par[1])], action=_z(n, 2))
    with pytest.raises(ValueError, match=r"out\['critics'\]: params is on"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), out=dict(action=good["action"]))
    with pytest.raises(ValueError, match=r"out\['action'\]: action_grad is on"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), action_grad=True, out=dict(critics=good["critics"]))
    with pytest.raises(ValueError, match=r"out\['critics'\]: expected 2 nets"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), out={**good, "critics": good["critics"][:1]})
    with pytest.raises(ValueError, match=r"out\['critics'\]\[1\]: expected 3"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), out={**good, "critics": [good["critics"][0], good["critics"][1][:2]]})
    with pytest.raises(ValueError, match=r"out\['critics'\]\[0\]\[0\] weight"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), out={**good, "critics": [[(_z(16, 13), _z(16))] + good["critics"][0][1:], good["critics"][1]]})
    with pytest.raises(ValueError, match=r"out\['action'\]"):
        env.q_grad_torch(q, obs, act, g_q1=_z(n), params=False, action_grad=True, out=dict(action=_z(n, 3)))
    assert env._lib.names() == []


def test_policy_action_calls_check_their_tensors_before_the_native_call():
    env = _stub_env()
    pol = env.policy_torch(**_params())
    n = 24
    obs, eps = _z(n, 13), _z(n, 2)
    a = env.policy_action_raw_torch(pol, obs, eps, out=_z(n, 2))
    name, args = env._lib.calls[-1]
    assert name == "sg_policy_action_device" and args[2] == n and args[4].value == eps.data_ptr() and args[5].value == a.data_ptr()
    env.policy_action_raw_torch(pol, obs, out=a)
    assert env._lib.calls[-1][1][4] is None
    env._lib.calls.clear()
    with pytest.raises(ValueError, match="handle policy_torch returns"):
        env.policy_action_raw_torch(None, obs)
    with pytest.raises(ValueError, match="obs"):
        env.policy_action_raw_torch(pol, _z(n, 14))
    with pytest.raises(ValueError, match="eps"):
        env.policy_action_raw_torch(pol, obs, _z(n, 3))
    with pytest.raises(ValueError, match="out"):
        env.policy_action_raw_torch(pol, obs, eps, out=_z(n + 1, 2))
    with pytest.raises(ValueError, match="g_action"):
        env.policy_action_grad_torch(pol, obs, _z(n))
    par = _params()
    good = dict(actor=[(_z(*w.shape), _z(*b.shape)) for w, b in par["actor"]], log_std=_z(2))
    with pytest.raises(ValueError, match=r"out\['actor'\]: expected 3"):
        env.policy_action_grad_torch(pol, obs, _z(n, 2), out={**good, "actor": good["actor"][:2]})
    with pytest.raises(ValueError, match=r"out\['actor'\]\[2\] bias"):
        env.policy_action_grad_torch(pol, obs, _z(n, 2), out={**good, "actor": good["actor"][:2] + [(_z(2, 16), _z(3))]})
    with pytest.raises(ValueError, match=r"out\['log_std'\]"):
        env.policy_action_grad_torch(pol, obs, _z(n, 2), out={**good, "log_std": None})
    with pytest.raises(ValueError, match="handle policy_torch returns"):
        env.policy_action_torch(env.q_torch(critics=_q_params()), obs)
    assert env._lib.names() == []
    env.discrete = True
    pol_d = env.policy_torch(**_params(head=6, log_std=None))
    for call in (env.policy_action_raw_torch, env.policy_action_torch):
        with pytest.raises(ValueError, match="needs a continuous id"):
            call(pol_d, obs)
    with pytest.raises(ValueError, match="needs a continuous id"):
        env.policy_action_grad_torch(pol_d, obs, _z(n, 2))
    assert env._lib.names() == []


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("q_torch", "q_evaluate_torch", "q_evaluate_raw_torch", "q_grad_torch", "policy_action_torch", "policy_action_raw_torch",
                     "policy_action_grad_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
