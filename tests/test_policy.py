"""CPU tests of the actor-critic policy entry points (sg_policy_act_device / sg_rollout_policy_device): the declarations and struct
layouts, the NumPy model (tests/policy_model.py) against torch's float64 modules and distributions, the moments of its noise, and the
Python argument checks of policy_torch / policy_act_torch / rollout_policy_torch with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from policy_model import STREAM_POLICY, act, mlp, random_policy, words
from test_episode_stats import _fake_cuda, _stub_env
from test_snapshot_device import _header_args


# ---------------------------------------------------------------------------------------------- declarations
def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    assert _header_args("sg_policy_act_device") == [
        "sg_env *env", "const sg_policy *policy", "const float *obs_dev", "uint64_t seed", "uint64_t step", "int32_t deterministic",
        "void *action_out", "float *logp_out", "float *value_out", "void *hip_stream"]
    assert _header_args("sg_rollout_policy_device") == [
        "sg_env *env", "int32_t n_steps", "const sg_policy *policy", "uint64_t seed", "uint64_t first_step", "int32_t deterministic",
        "float *obs", "void *action", "float *logp", "float *value", "float *reward", "uint8_t *done", "uint8_t *truncated",
        "const sg_terminal_list *terminal_list", "float *terminal_value", "void *hip_stream"]
    vp, P = C.c_void_p, C.POINTER(_native.SgPolicy)
    assert _native.SYMBOLS["sg_policy_act_device"] == (C.c_int, [vp, P, vp, C.c_uint64, C.c_uint64, C.c_int32, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_rollout_policy_device"] == (
        C.c_int, [vp, C.c_int32, P, C.c_uint64, C.c_uint64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(_native.SgTerminalList), vp, vp])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct sg_policy {"):header.index("} sg_policy;")], flags=re.S)
    names = [d.split()[-1].lstrip("*") for d in body.replace("typedef struct sg_policy {", "").split(";") if d.strip()]
    assert names == [f for f, _ in _native.SgPolicy._fields_]
    assert C.sizeof(_native.SgPolicyMlp) == 64 and C.sizeof(_native.SgPolicy) == 24 + 64 + 64 + 8
    assert _native.SgPolicy.log_std.offset == 152 and _native.SgPolicy.actor.offset == 24
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    inc = open(os.path.join(build.CSRC, "sg_policy.inc")).read()
    assert "sg_policy.inc" in build.HEADERS and '#include "sg_policy.inc"' in src
    assert re.search(r"constexpr uint32_t kStreamPolicy = 5u;", inc) and STREAM_POLICY == 5
    assert "kStreamPolicy, o)" in inc


# ---------------------------------------------------------------------------------------------- the model
def _torch_net(layers, activation):
    import torch
    mods = []
    for l, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W.astype(np.float64)))
            lin.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        mods.append(lin)
        if l < len(layers) - 1:
            mods.append(torch.nn.Tanh() if activation == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", [(1, 1), (33, 2), (128, 3)])
def test_model_forward_equals_a_torch_float64_sequential(hidden, n_hidden, activation):
    import torch
    rng = np.random.default_rng(hidden * 10 + n_hidden)
    D, B = 13, 50
    obs = rng.standard_normal((B, D)).astype(np.float32)
    for continuous in (True, False):
        pol = random_policy(rng, D, hidden, n_hidden, 2 if continuous else 6, critic=True, continuous=continuous)
        got = act(pol, obs, seed=3, step=4, activation=activation)
        with torch.no_grad():
            x = torch.from_numpy(obs.astype(np.float64))
            head = _torch_net(pol["actor"], activation)(x).numpy()
            value = _torch_net(pol["critic"], activation)(x).numpy()[:, 0]
        assert np.allclose(got["mean" if continuous else "logits"], head, rtol=0, atol=1e-13)
        assert np.allclose(got["value"], value, rtol=0, atol=1e-13)
        assert np.array_equal(mlp(pol["actor"], obs, activation), got["mean" if continuous else "logits"])


def test_model_log_probs_equal_torch_distributions():
    import torch
    rng = np.random.default_rng(5)
    D, B = 10, 300
    obs = rng.standard_normal((B, D)).astype(np.float32)
    pol = random_policy(rng, D, 64, 2, 2)
    for det in (False, True):
        got = act(pol, obs, seed=11, step=7, deterministic=det)
        dist = torch.distributions.Normal(torch.from_numpy(got["mean"]), torch.from_numpy(np.exp(pol["log_std"].astype(np.float64))))
        want = dist.log_prob(torch.from_numpy(got["action"])).sum(-1).numpy()
        assert np.allclose(got["logp"], want, rtol=0, atol=1e-12)
        if det:
            assert np.array_equal(got["action"], got["mean"])
    pol = random_policy(rng, D, 64, 2, 6, continuous=False)
    for det in (False, True):
        got = act(pol, obs, seed=11, step=7, deterministic=det)
        cat = torch.distributions.Categorical(logits=torch.from_numpy(got["logits"]))
        want = cat.log_prob(torch.from_numpy(got["action"].astype(np.int64))).numpy()
        assert np.allclose(got["logp"], want, rtol=0, atol=1e-12)
        if det:
            assert np.array_equal(got["action"], got["logits"].argmax(axis=1))
    # the draw: the first index whose running sum reaches u * total, i.e. the inverse CDF of softmax(logits) at u
    got = act(pol, obs, seed=11, step=7)
    probs = np.exp(got["logits"] - got["logits"].max(axis=1, keepdims=True))
    probs /= probs.sum(axis=1, keepdims=True)
    u = got["want"] / got["total"]
    cdf = np.cumsum(probs, axis=1)
    a = got["action"]
    lower = np.where(a > 0, cdf[np.arange(B), np.maximum(a - 1, 0)], 0.0)
    assert (u <= cdf[np.arange(B), a] + 1e-12).all() and (u > lower - 1e-12).all()
    # scoring given actions
    again = act(pol, obs, seed=11, step=7, action=a)
    assert np.array_equal(again["logp"], got["logp"])


def test_model_noise_is_standard_normal_and_keyed_by_seed_step_and_global_env():
    n = 100_000
    pol = dict(actor=[(np.zeros((4, 3), np.float32), np.zeros(4, np.float32)), (np.zeros((2, 4), np.float32), np.zeros(2, np.float32))],
               critic=None, log_std=np.zeros(2, np.float32))
    obs = np.zeros((n, 3), np.float32)
    eps = act(pol, obs, seed=123, step=9)["eps"]
    se = 1.0 / np.sqrt(n)
    for d in range(2):
        assert abs(eps[:, d].mean()) <= 4 * se, eps[:, d].mean()
        assert abs(eps[:, d].var() - 1.0) <= 4 * np.sqrt(2.0) * se, eps[:, d].var()
    assert abs((eps[:, 0] * eps[:, 1]).mean()) <= 4 * se
    # an env's draw depends on its global index only: a shard that starts at 64 sees rows 64 .. of the whole batch
    assert np.array_equal(act(pol, obs[:50], seed=123, step=9, env_index_base=64)["eps"], eps[64:114])
    assert not np.array_equal(act(pol, obs[:50], seed=123, step=10)["eps"], eps[:50])
    assert not np.array_equal(act(pol, obs[:50], seed=124, step=9)["eps"], eps[:50])
    assert [int(x[0]) for x in words(2 ** 40 + 5, 2 ** 33 + 1, [7])] == [int(x[1]) for x in words(2 ** 40 + 5, 2 ** 33 + 1, [6, 7])]
    assert int(words(1, 2, [3])[0][0]) != int(words(1, 2 + 2 ** 32, [3])[0][0])  # the high word of the step is part of the counter


# ---------------------------------------------------------------------------------------------- the front end, stubbed
def _params(D=13, hidden=16, n_hidden=2, head=2, **over):
    import torch
    dims = [D] + [hidden] * n_hidden
    net = [(_fake_cuda(torch.zeros((o, i))), _fake_cuda(torch.zeros(o))) for i, o in zip(dims[:-1], dims[1:])]
    p = dict(actor=net + [(_fake_cuda(torch.zeros((head, hidden))), _fake_cuda(torch.zeros(head)))],
             critic=[(_fake_cuda(torch.zeros_like(w)), _fake_cuda(torch.zeros_like(b))) for w, b in net]
             + [(_fake_cuda(torch.zeros((1, hidden))), _fake_cuda(torch.zeros(1)))],
             log_std=_fake_cuda(torch.zeros(2)))
    p.update(over)
    return p


def test_policy_torch_builds_the_struct_over_the_callers_tensors():
    env = _stub_env()
    p = _params()
    pol = env.policy_torch(**p)
    s = pol.struct
    assert (s.struct_size, s.n_hidden, s.hidden, s.activation, s.head) == (160, 2, 16, 0, 2) and pol.has_critic
    for l in range(3):
        assert s.actor.weight[l] == p["actor"][l][0].data_ptr() and s.actor.bias[l] == p["actor"][l][1].data_ptr()
        assert s.critic.weight[l] == p["critic"][l][0].data_ptr() and s.critic.bias[l] == p["critic"][l][1].data_ptr()
    assert s.actor.weight[3] is None and s.log_std == p["log_std"].data_ptr()
    assert env.policy_torch(**_params(critic=None), activation="relu").struct.activation == 1
    assert not env.policy_torch(**_params(critic=None)).has_critic
    assert env._lib.names() == []  # a handle is made without a native call


def test_policy_torch_refuses_what_the_kernel_cannot_take():
    import torch
    env = _stub_env()
    bad_chain = _params()
    bad_chain["actor"][1] = (_fake_cuda(torch.zeros((16, 15))), bad_chain["actor"][1][1])
    with pytest.raises(ValueError, match=r"actor\[1\] weight"):
        env.policy_torch(**bad_chain)
    bad_head = _params(head=3)
    with pytest.raises(ValueError, match=r"actor\[2\] weight"):
        env.policy_torch(**bad_head)
    p = _params()
    p["actor"][0] = (_fake_cuda(torch.zeros((16, 13), dtype=torch.float64)), p["actor"][0][1])
    with pytest.raises(ValueError, match=r"actor\[0\] weight"):
        env.policy_torch(**p)
    p = _params()
    p["critic"][0] = (torch.zeros((16, 13)), p["critic"][0][1])  # not on the device
    with pytest.raises(ValueError, match="CUDA tensor"):
        env.policy_torch(**p)
    p = _params()
    p["actor"][2] = (_fake_cuda(torch.zeros((16, 2)).t()), p["actor"][2][1])  # a transposed view
    with pytest.raises(ValueError, match="not contiguous"):
        env.policy_torch(**p)
    with pytest.raises(ValueError, match="hidden must be 1 .. 128, got 129"):
        env.policy_torch(**_params(hidden=129))
    with pytest.raises(ValueError, match="n_hidden must be 1 .. 3"):
        env.policy_torch(**_params(n_hidden=0))
    with pytest.raises(ValueError, match="n_hidden must be 1 .. 3"):
        env.policy_torch(**_params(n_hidden=4))
    with pytest.raises(ValueError, match="log_std: a continuous id needs"):
        env.policy_torch(**_params(log_std=None))
    with pytest.raises(ValueError, match="activation"):
        env.policy_torch(**_params(), activation="gelu")
    p = _params()
    p["critic"] = _params(hidden=8)["critic"]
    with pytest.raises(ValueError, match="like the actor"):
        env.policy_torch(**p)
    env.discrete = True
    with pytest.raises(ValueError, match=r"actor\[2\] weight"):
        env.policy_torch(**_params(log_std=None))  # a head of 2 on a discrete id
    with pytest.raises(ValueError, match="the discrete ids take none"):
        env.policy_torch(**_params(head=6))
    assert env.policy_torch(**_params(head=6, log_std=None)).struct.head == 6
    assert env._lib.names() == []


def _rollout_buffers(env, K=4, value=True):
    import torch
    B, D = env.num_envs, env.obs_dim
    z = lambda *shape, dtype=torch.float32: _fake_cuda(torch.zeros(shape, dtype=dtype))
    return dict(obs=z(K + 1, B, D), action=z(K, B, 2), logp=z(K, B), value=z(K + 1, B) if value else None, reward=z(K, B),
                done=z(K, B, dtype=torch.uint8), trunc=z(K, B, dtype=torch.uint8))


def test_act_and_rollout_check_their_tensors_before_the_native_call():
    import torch
    env = _stub_env()
    B, D = env.num_envs, env.obs_dim
    pol, pol_nc = env.policy_torch(**_params()), env.policy_torch(**_params(critic=None))
    obs = _fake_cuda(torch.zeros((B, D)))
    out = dict(action=_fake_cuda(torch.zeros((B, 2))), logp=_fake_cuda(torch.zeros(B)), value=_fake_cuda(torch.zeros(B)))
    a, lp, v = env.policy_act_torch(pol, obs, seed=5, step=6, out=out)
    assert a is out["action"] and lp is out["logp"] and v is out["value"]
    name, args = env._lib.calls[-1]
    assert name == "sg_policy_act_device" and args[3:6] == (5, 6, 0) and args[8].value == out["value"].data_ptr()
    with pytest.raises(ValueError, match="obs"):
        env.policy_act_torch(pol, _fake_cuda(torch.zeros((B, D + 1))), out=out)
    with pytest.raises(ValueError, match="no critic"):
        env.policy_act_torch(pol_nc, obs, out=out)
    with pytest.raises(ValueError, match="handle policy_torch returns"):
        env.policy_act_torch(_params(), obs, out=out)
    env._lib.calls.clear()
    b = _rollout_buffers(env)
    with pytest.raises(ValueError, match="the policy has a critic"):
        env.rollout_policy_torch(pol, **{**b, "value": None})
    with pytest.raises(ValueError, match="the policy has no critic"):
        env.rollout_policy_torch(pol_nc, **b)
    with pytest.raises(ValueError, match="obs"):
        env.rollout_policy_torch(pol, **{**b, "obs": b["obs"][:-1]})  # K rows: the row the last step writes is missing
    with pytest.raises(ValueError, match="logp"):
        env.rollout_policy_torch(pol, **{**b, "logp": b["value"]})
    assert env._lib.names() == []
    term = dict(count=_fake_cuda(torch.zeros(1, dtype=torch.int32)), step_env=_fake_cuda(torch.zeros((32, 2), dtype=torch.int32)),
                obs=_fake_cuda(torch.zeros((32, D))), value=_fake_cuda(torch.zeros(32)))
    env.rollout_policy_torch(pol, seed=9, first_step=100, terminal=term, **b)
    name, args = env._lib.calls[-1]
    assert name == "sg_rollout_policy_device" and args[1] == 4 and args[3:6] == (9, 100, 0)
    assert args[14].value == term["value"].data_ptr() and args[9].value == b["value"].data_ptr()
    env.rollout_policy_torch(pol_nc, terminal={k: term[k] for k in ("count", "step_env", "obs")}, **_rollout_buffers(env, value=False))
    assert env._lib.calls[-1][1][14] is None and env._lib.calls[-1][1][9] is None
    with pytest.raises(ValueError, match=r"terminal\['value'\]"):
        env.rollout_policy_torch(pol, terminal={**term, "value": _fake_cuda(torch.zeros(31))}, **b)


def test_the_multi_device_front_ends_refuse_the_policy_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("policy_torch", "policy_act_torch", "rollout_policy_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
