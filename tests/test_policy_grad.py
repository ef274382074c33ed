"""CPU tests of the policy evaluate / gradient entry points (sg_policy_evaluate_device / sg_policy_grad_device): the declarations, the
NumPy model (tests/policy_grad_model.py) against torch.autograd on float64 modules and distributions, the relu-at-zero convention, and
the Python argument checks of policy_evaluate_raw_torch / policy_grad_torch / policy_evaluate_torch with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from policy_grad_model import evaluate, flat, grad_tolerances
from policy_model import random_policy
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_snapshot_device import _header_args

NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    assert _header_args("sg_policy_evaluate_device") == [
        "sg_env *env", "const sg_policy *policy", "int64_t n", "const float *obs", "const void *action", "float *logp_out",
        "float *entropy_out", "float *value_out", "void *hip_stream"]
    assert _header_args("sg_policy_grad_device") == [
        "sg_env *env", "const sg_policy *policy", "int64_t n", "const float *obs", "const void *action", "const float *g_logp",
        "const float *g_entropy", "const float *g_value", "const sg_policy_grads *grads", "void *workspace", "size_t workspace_bytes",
        "void *hip_stream"]
    vp, P, G = C.c_void_p, C.POINTER(_native.SgPolicy), C.POINTER(_native.SgPolicyGrads)
    assert _native.SYMBOLS["sg_policy_evaluate_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_policy_grad_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp, vp, G, vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_policy_grad_workspace_bytes"] == (C.c_size_t, [vp, P, C.c_int64])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct sg_policy_grads {"):header.index("} sg_policy_grads;")], flags=re.S)
    names = [d.split()[-1].lstrip("*") for d in body.replace("typedef struct sg_policy_grads {", "").split(";") if d.strip()]
    assert names == [f for f, _ in _native.SgPolicyGrads._fields_]
    assert C.sizeof(_native.SgPolicyGrads) == 8 + 64 + 64 + 8 and _native.SgPolicyGrads.log_std.offset == 136
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_policy_grad.inc" in build.HEADERS and '#include "sg_policy_grad.inc"' in src


def _torch_reference(pol, obs, action, g, activation):
    """logp, entropy, value and every parameter gradient of sum(g . outputs) from torch.autograd on float64 modules"""
    import torch
    actor = _torch_net(pol["actor"], activation)
    critic = _torch_net(pol["critic"], activation)
    x = torch.from_numpy(obs.astype(np.float64))
    head = actor(x)
    if pol["log_std"] is not None:
        ls = torch.from_numpy(pol["log_std"].astype(np.float64)).requires_grad_()
        dist = torch.distributions.Normal(head, ls.exp().expand_as(head))
        logp, ent = dist.log_prob(torch.from_numpy(action.astype(np.float64))).sum(1), dist.entropy().sum(1)
    else:
        ls = None
        dist = torch.distributions.Categorical(logits=head)
        logp, ent = dist.log_prob(torch.from_numpy(action.astype(np.int64))), dist.entropy()
    value = critic(x)[:, 0]
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    (t(g[0]) * logp + t(g[1]) * ent + t(g[2]) * value).sum().backward()
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    res = dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(actor)],
               critic=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(critic)], log_std=ls.grad.numpy() if ls is not None else None)
    return logp.detach().numpy(), ent.detach().numpy(), value.detach().numpy(), flat(res)


@pytest.mark.parametrize("continuous", [True, False])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", NETS)
def test_model_equals_torch_autograd_in_float64(hidden, n_hidden, activation, continuous):
    rng = np.random.default_rng(hidden + 7 * n_hidden)
    D, n = 13, 37
    obs = rng.standard_normal((n, D)).astype(np.float32)
    pol = random_policy(rng, D, hidden, n_hidden, 2 if continuous else 6, critic=True, continuous=continuous)
    action = rng.standard_normal((n, 2)).astype(np.float32) if continuous else rng.integers(0, 6, n).astype(np.int32)
    g = [rng.standard_normal(n) for _ in range(3)]
    got = evaluate(pol, obs, action, *g, activation=activation)
    logp, ent, value, grads = _torch_reference(pol, obs, action, g, activation)
    rel = lambda a, b: float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))
    assert rel(got["logp"], logp) <= 1e-10 and rel(got["entropy"], ent) <= 1e-10 and rel(got["value"], value) <= 1e-10
    mine = flat(got)
    assert set(mine) == set(grads)
    for k in grads:
        assert mine[k].shape == grads[k].shape and rel(mine[k], grads[k]) <= 1e-10, (k, rel(mine[k], grads[k]))


def test_float32_mode_is_float32_and_close():
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((300, 13)).astype(np.float32)
    pol = random_policy(rng, 13, 33, 2, 2)
    action = rng.standard_normal((300, 2)).astype(np.float32)
    g = [rng.standard_normal(300).astype(np.float32) for _ in range(3)]
    g64, g32 = flat(evaluate(pol, obs, action, *g)), flat(evaluate(pol, obs, action, *g, dtype=np.float32))
    tol = grad_tolerances(g32, g64)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k


def test_relu_has_zero_slope_at_zero_as_torch():
    """a unit whose pre-activation is exactly 0 passes no gradient: relu'(0) = 0"""
    rng = np.random.default_rng(4)
    n, D = 9, 13
    obs = rng.standard_normal((n, D)).astype(np.float32)
    pol = random_policy(rng, D, 5, 2, 2)
    for net in ("actor", "critic"):
        W, b = pol[net][0]
        W[2] = 0.0
        b[2] = 0.0  # unit 2 of layer 0: pre-activation 0 for every row
    action = rng.standard_normal((n, 2)).astype(np.float32)
    g = [rng.standard_normal(n) for _ in range(3)]
    got = flat(evaluate(pol, obs, action, *g, activation="relu"))
    ref = _torch_reference(pol, obs, action, g, "relu")[3]
    for net in ("actor", "critic"):
        assert not got[f"{net}.0.weight"][2].any() and got[f"{net}.0.bias"][2] == 0 and not got[f"{net}.1.weight"][:, 2].any()
        assert got[f"{net}.0.weight"][[0, 1, 3, 4]].any()
    for k in ref:
        assert np.allclose(got[k], ref[k], rtol=1e-10, atol=1e-14), k


def _rows(n=24, D=13, discrete=False):
    import torch
    z = lambda *shape, dtype=torch.float32: _fake_cuda(torch.zeros(shape, dtype=dtype))
    return z(n, D), (z(n, dtype=torch.int32) if discrete else z(n, 2)), z


def test_evaluate_and_grad_check_their_tensors_before_the_native_call():
    env = _stub_env()
    pol, pol_nc = env.policy_torch(**_params()), env.policy_torch(**_params(critic=None))
    obs, action, z = _rows()
    n = 24  # a row count of its own, not num_envs (8)
    out = dict(logp=z(n), entropy=z(n), value=z(n))
    lp, ent, v = env.policy_evaluate_raw_torch(pol, obs, action, out=out)
    assert lp is out["logp"] and ent is out["entropy"] and v is out["value"]
    name, args = env._lib.calls[-1]
    assert name == "sg_policy_evaluate_device" and args[2] == n and args[7].value == out["value"].data_ptr()
    env.policy_evaluate_raw_torch(pol, obs, action, out=dict(entropy=out["entropy"]))
    assert env._lib.calls[-1][1][5] is None and env._lib.calls[-1][1][7] is None
    env._lib.calls.clear()
    with pytest.raises(ValueError, match="handle policy_torch returns"):
        env.policy_evaluate_raw_torch(_params(), obs, action)
    with pytest.raises(ValueError, match="obs"):
        env.policy_evaluate_raw_torch(pol, z(n, 14), action)
    with pytest.raises(ValueError, match="obs"):
        env.policy_evaluate_raw_torch(pol, z(0, 13), z(0, 2))
    with pytest.raises(ValueError, match="action"):
        env.policy_evaluate_raw_torch(pol, obs, z(n - 1, 2))
    with pytest.raises(ValueError, match="action"):
        env.policy_evaluate_raw_torch(pol, obs, _rows(discrete=True)[1])
    with pytest.raises(ValueError, match="no critic"):
        env.policy_evaluate_raw_torch(pol_nc, obs, action, out=out)
    with pytest.raises(ValueError, match="at least one"):
        env.policy_evaluate_raw_torch(pol, obs, action, out={})
    with pytest.raises(ValueError, match=r"out\['logp'\]"):
        env.policy_evaluate_raw_torch(pol, obs, action, out=dict(logp=z(n + 1)))
    with pytest.raises(ValueError, match="g_logp"):
        env.policy_grad_torch(pol, obs, action, g_logp=z(n + 1))
    with pytest.raises(ValueError, match="g_value: the policy has no critic"):
        env.policy_grad_torch(pol_nc, obs, action, g_value=z(n))
    pairs = lambda p: [(z(*w.shape), z(*b.shape)) for w, b in p]
    par = _params()
    good = dict(actor=pairs(par["actor"]), critic=pairs(par["critic"]), log_std=z(2))
    with pytest.raises(ValueError, match=r"out\['actor'\]\[1\] weight"):
        env.policy_grad_torch(pol, obs, action, g_logp=z(n), out={**good, "actor": [good["actor"][0], (z(16, 15), z(16)), good["actor"][2]]})
    with pytest.raises(ValueError, match=r"out\['actor'\]: expected 3"):
        env.policy_grad_torch(pol, obs, action, g_logp=z(n), out={**good, "actor": good["actor"][:2]})
    with pytest.raises(ValueError, match=r"out\['critic'\]: g_value is given"):
        env.policy_grad_torch(pol, obs, action, g_value=z(n), out={**good, "critic": None})
    with pytest.raises(ValueError, match=r"out\['critic'\]: the policy has no critic"):
        env.policy_grad_torch(pol_nc, obs, action, g_logp=z(n), out=good)
    with pytest.raises(ValueError, match=r"out\['log_std'\]"):
        env.policy_grad_torch(pol, obs, action, g_logp=z(n), out={**good, "log_std": None})
    with pytest.raises(ValueError, match="handle policy_torch returns"):
        env.policy_evaluate_torch(None, obs, action)
    assert env._lib.names() == []
    env.discrete = True
    pol_d = env.policy_torch(**_params(head=6, log_std=None))
    with pytest.raises(ValueError, match="the discrete ids have none"):
        env.policy_grad_torch(pol_d, obs, _rows(discrete=True)[1], g_logp=z(n), out={**good, "actor": pairs(_params(head=6)["actor"])})
    assert env._lib.names() == []


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("policy_evaluate_torch", "policy_evaluate_raw_torch", "policy_grad_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
