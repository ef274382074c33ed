"""CPU tests of the SAC actor (sg_squashed_act_device / sg_squashed_sample_device / sg_squashed_grad_device /
sg_rollout_squashed_device): the declarations, the NumPy model (tests/squashed_model.py) against torch.autograd and
torch.distributions in float64, the clamp's slope at and outside its bounds, saturation, the noise of stream tag 6, the float32 mode,
the 1 % cap of every gradient case the GPU tests run, and the Python argument checks with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from squashed_model import BOUNDS, MARGIN, NETS, SELECTIONS, STREAM_SQUASHED, act, case, flat, grad_cases, grad_reference, grad_tolerances
from squashed_model import noise, random_squashed, sample, words
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_snapshot_device import _header_args

REL = 1e-10  # float64 model against float64 autograd: section 18's figure for the same kind of comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    assert _header_args("sg_squashed_act_device") == [
        "sg_env *env", "const sg_squashed_policy *sp", "const float *obs_dev", "uint64_t seed", "uint64_t step", "int32_t deterministic",
        "float *action_out", "float *logp_out", "void *hip_stream"]
    assert _header_args("sg_squashed_sample_device") == [
        "sg_env *env", "const sg_squashed_policy *sp", "int64_t n", "const float *obs", "const float *eps", "float *action_out",
        "float *logp_out", "void *hip_stream"]
    assert _header_args("sg_squashed_grad_device") == [
        "sg_env *env", "const sg_squashed_policy *sp", "int64_t n", "const float *obs", "const float *eps", "const float *g_action",
        "const float *g_logp", "const sg_squashed_grads *grads", "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_squashed_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_squashed_policy *sp", "int64_t n"]
    assert _header_args("sg_rollout_squashed_device") == [
        "sg_env *env", "int32_t n_steps", "const sg_squashed_policy *sp", "uint64_t seed", "uint64_t first_step", "int32_t deterministic",
        "float *obs", "float *action", "float *logp", "float *reward", "uint8_t *done", "uint8_t *truncated",
        "const sg_terminal_list *terminal_list", "void *hip_stream"]
    vp, P, G = C.c_void_p, C.POINTER(_native.SgSquashedPolicy), C.POINTER(_native.SgSquashedGrads)
    assert _native.SYMBOLS["sg_squashed_act_device"] == (C.c_int, [vp, P, vp, C.c_uint64, C.c_uint64, C.c_int32, vp, vp, vp])
    assert _native.SYMBOLS["sg_squashed_sample_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_squashed_grad_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp, G, vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_squashed_grad_workspace_bytes"] == (C.c_size_t, [vp, P, C.c_int64])
    assert _native.SYMBOLS["sg_rollout_squashed_device"] == (
        C.c_int, [vp, C.c_int32, P, C.c_uint64, C.c_uint64, C.c_int32, vp, vp, vp, vp, vp, vp, C.POINTER(_native.SgTerminalList), vp])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls in (("sg_squashed_policy", _native.SgSquashedPolicy), ("sg_squashed_grads", _native.SgSquashedGrads)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_], name
    assert C.sizeof(_native.SgSquashedPolicy) == 96 and _native.SgSquashedPolicy.actor.offset == 24 and _native.SgSquashedPolicy.reserved.offset == 88
    assert C.sizeof(_native.SgSquashedGrads) == 8 + 64 and _native.SgSquashedGrads.actor.offset == 8
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_squashed.inc" in build.HEADERS and '#include "sg_squashed.inc"' in src
    inc = open(os.path.join(build.CSRC, "sg_squashed.inc")).read()
    assert re.search(r"constexpr uint32_t kStreamSquashed = 6u;", inc) and STREAM_SQUASHED == 6
    assert "kStreamSquashed, o)" in inc
    assert "1e-6" in header[header.index("The SAC actor"):header.index("typedef struct sg_squashed_policy")]  # the header says what it is not


def _torch_sample(actor, obs, eps, ga, gl, bounds, activation):
    """(action, logp), TransformedDistribution's logp, and every parameter gradient of sum_i (ga . a + gl logp), from float64 torch"""
    import torch
    from torch.distributions import Normal, TransformedDistribution
    from torch.distributions.transforms import TanhTransform
    net = _torch_net(actor, activation)
    head = net(torch.from_numpy(obs.astype(np.float64)))
    mean, raw = head[:, :2], head[:, 2:]
    ls = torch.clamp(raw, float(np.float32(bounds[0])), float(np.float32(bounds[1])))
    e = torch.from_numpy(eps.astype(np.float64))
    u = mean + ls.exp() * e
    a = torch.tanh(u)
    logp = (-0.5 * e * e - ls - 0.5 * np.log(2 * np.pi) - 2.0 * (np.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(-1)
    dist = TransformedDistribution(Normal(mean, ls.exp()), TanhTransform(cache_size=1))
    logp_dist = dist.log_prob(a).sum(-1).detach().numpy()  # (cache_size 1: the transform returns the u it made a from, no atanh)
    loss = 0.0
    if ga is not None:
        loss = loss + (torch.from_numpy(np.asarray(ga, np.float64)) * a).sum()
    if gl is not None:
        loss = loss + (torch.from_numpy(np.asarray(gl, np.float64)) * logp).sum()
    loss.backward()
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    grads = flat(dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin]))
    return a.detach().numpy(), logp.detach().numpy(), logp_dist, grads


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", NETS)
def test_model_equals_torch_autograd_and_distributions_in_float64(hidden, n_hidden, activation):
    c = case(13, 37, hidden, n_hidden, seed=1)
    raw = sample(c["actor"], c["obs"], bounds=BOUNDS, activation=activation)["raw"]
    if hidden > 1:  # the clamp is exercised on every side
        assert (raw < BOUNDS[0]).any() and (raw > BOUNDS[1]).any() and ((raw > BOUNDS[0]) & (raw < BOUNDS[1])).any()
    for sel in SELECTIONS:
        ga = c["g_action"] if sel in ("both", "action") else None
        gl = c["g_logp"] if sel in ("both", "logp") else None
        got = sample(c["actor"], c["obs"], c["eps"], ga, gl, bounds=BOUNDS, activation=activation)
        a, logp, logp_dist, grads = _torch_sample(c["actor"], c["obs"], c["eps"], ga, gl, BOUNDS, activation)
        assert rel(got["action"], a) <= REL and rel(got["logp"], logp) <= REL
        assert rel(got["logp"], logp_dist) <= REL
        mine = flat(got)
        assert set(mine) == set(grads)
        for k in grads:
            assert mine[k].shape == grads[k].shape and rel(mine[k], grads[k]) <= REL, (sel, k, rel(mine[k], grads[k]))
    plain = sample(c["actor"], c["obs"], None, c["g_action"], None, bounds=BOUNDS, activation=activation)
    a0, lp0, _, g0 = _torch_sample(c["actor"], c["obs"], np.zeros((37, 2), np.float32), c["g_action"], None, BOUNDS, activation)
    assert rel(plain["action"], a0) <= REL and rel(plain["logp"], lp0) <= REL
    assert not flat(plain)["actor.%d.weight" % n_hidden][2:].any() and not flat(plain)["actor.%d.bias" % n_hidden][2:].any()
    for k in g0:
        assert np.allclose(flat(plain)[k], g0[k], rtol=1e-10, atol=1e-14), k
    wide = sample(c["actor"], c["obs"], c["eps"], activation=activation)  # the default bounds are SB3's: nothing is clamped here
    assert np.array_equal(wide["ls"], wide["raw"])


def test_the_clamp_has_slope_one_at_its_bounds_and_zero_outside():
    """raw == bound exactly (zero head weights, bias = bound): the gradient passes, as torch.clamp's backward; just outside: nothing"""
    import torch
    D, n = 5, 4
    rng = np.random.default_rng(2)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    eps, gl = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal(n)
    lo, hi = np.float32(-0.5), np.float32(0.5)

    def actor(raw0, raw1):
        layers = random_squashed(rng, D, 3, 1)
        W, b = layers[-1]
        W[2:] = 0.0
        b[2], b[3] = raw0, raw1
        return layers

    at = actor(lo, hi)
    got = flat(sample(at, obs, eps, None, gl, bounds=(lo, hi), activation="tanh"))
    assert got["actor.1.bias"][2] != 0 and got["actor.1.bias"][3] != 0
    _, _, _, ref = _torch_sample(at, obs, eps, None, gl, (lo, hi), "tanh")
    t = torch.tensor([float(lo), float(hi)], dtype=torch.float64, requires_grad=True)
    torch.clamp(t, float(lo), float(hi)).sum().backward()
    assert t.grad.tolist() == [1.0, 1.0]  # torch's own convention
    for k in ref:
        assert np.allclose(got[k], ref[k], rtol=1e-10, atol=1e-14), k
    out = actor(np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1)))
    got = flat(sample(out, obs, eps, None, gl, bounds=(lo, hi), activation="tanh"))
    assert not got["actor.1.bias"][2:].any() and not got["actor.1.weight"][2:].any() and got["actor.1.bias"][:2].all()
    r32 = flat(sample(at, obs, eps, None, gl, bounds=(lo, hi), activation="tanh", dtype=np.float32))
    assert r32["actor.1.bias"][2] != 0 and r32["actor.1.bias"][3] != 0  # the float32 mode sees the same mask


def test_saturated_actions_keep_a_finite_log_prob_and_gradient():
    """|u| = 30: a = +-1 exactly, log(1 - a^2) would be -inf; the model's ldj is -2 |u| + 2 ln 2, finite, and so is every gradient"""
    D = 3
    layers = [(np.zeros((2, D), np.float32), np.zeros(2, np.float32)),
              (np.zeros((4, 2), np.float32), np.array([30.0, -30.0, 0.0, 0.0], np.float32))]
    obs = np.ones((2, D), np.float32)
    for dtype in (np.float64, np.float32):
        got = sample(layers, obs, np.zeros((2, 2), np.float32), np.ones((2, 2)), np.ones(2), dtype=dtype)
        assert np.array_equal(got["action"], [[1.0, -1.0]] * 2)
        ldj = 2 * (np.log(2.0) - 30.0)
        assert np.isfinite(got["logp"]).all() and np.allclose(got["logp"], -np.log(2 * np.pi) - 2 * ldj, rtol=1e-6)
        g = flat(got)
        assert all(np.isfinite(v).all() for v in g.values())
        assert np.allclose(g["actor.1.bias"][:2], [4.0, -4.0], rtol=1e-6)  # d logp / d u = 2 a per row, two rows; 1 - a^2 ~ 0
        assert np.allclose(g["actor.1.bias"][2:], [-2.0, -2.0])  # d logp / d ls = -1 per row (eps = 0)


def test_model_noise_is_standard_normal_and_keyed_by_seed_step_global_env_and_tag_6():
    from policy_model import words as policy_words
    n = 100_000
    eps = noise(123, 9, np.arange(n))
    se = 1.0 / np.sqrt(n)
    for d in range(2):
        assert abs(eps[:, d].mean()) <= 4 * se, eps[:, d].mean()
        assert abs(eps[:, d].var() - 1.0) <= 4 * np.sqrt(2.0) * se, eps[:, d].var()
    assert abs((eps[:, 0] * eps[:, 1]).mean()) <= 4 * se
    layers = [(np.zeros((4, 3), np.float32), np.zeros(4, np.float32)), (np.zeros((4, 4), np.float32), np.zeros(4, np.float32))]
    obs = np.zeros((50, 3), np.float32)
    assert np.array_equal(act(layers, obs, seed=123, step=9, env_index_base=64)["eps"], eps[64:114])
    assert np.allclose(act(layers, obs, seed=123, step=9, env_index_base=64)["action"], np.tanh(eps[64:114]), rtol=0, atol=1e-15)  # mean 0, sigma 1
    assert not np.array_equal(act(layers, obs, seed=123, step=10)["eps"], eps[:50])
    assert not np.array_equal(act(layers, obs, seed=124, step=9)["eps"], eps[:50])
    assert not act(layers, obs, seed=123, step=9, deterministic=True)["eps"].any()
    assert int(words(1, 2, [3])[0][0]) != int(policy_words(1, 2, [3])[0][0])  # another stream than the on-policy actor's
    assert int(words(1, 2, [3])[0][0]) != int(words(1, 2 + 2 ** 32, [3])[0][0])  # the high word of the step is part of the counter


def test_float32_mode_is_float32_and_close():
    c = case(13, 300, 33, 2, seed=3)
    r64 = sample(c["actor"], c["obs"], c["eps"], c["g_action"], c["g_logp"], bounds=BOUNDS)
    r32 = sample(c["actor"], c["obs"], c["eps"], c["g_action"], c["g_logp"], bounds=BOUNDS, dtype=np.float32)
    g64, g32 = flat(r64), flat(r32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
    for k in ("action", "logp"):
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64 and 0 < np.abs(r32[k] - r64[k]).max() < 1e-4


@pytest.mark.parametrize("obs_dim,n,hidden,n_hidden,activation", grad_cases())
def test_every_gpu_gradient_case_has_a_tolerance_of_at_most_one_percent(obs_dim, n, hidden, n_hidden, activation):
    """8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) <= 1 % of max|G64| per tensor, for the very cases (the same generator, the same
    seed) tests/test_gpu_squashed.py runs: a GPU failure cannot be the inputs' fault.  No row sits within MARGIN of a clamp bound."""
    c = case(obs_dim, n, hidden, n_hidden, seed=n + hidden)
    raw = sample(c["actor"], c["obs"], bounds=BOUNDS, activation=activation)["raw"]
    assert (np.minimum(np.abs(raw - BOUNDS[0]), np.abs(raw - BOUNDS[1])) >= MARGIN).all()
    r32 = sample(c["actor"], c["obs"], bounds=BOUNDS, activation=activation, dtype=np.float32)["raw"]
    assert np.array_equal((raw >= BOUNDS[0]) & (raw <= BOUNDS[1]), (r32 >= np.float32(BOUNDS[0])) & (r32 <= np.float32(BOUNDS[1])))
    for sel in SELECTIONS:
        g64, g32 = grad_reference(c, activation, sel, np.float64), grad_reference(c, activation, sel, np.float32)
        tol = grad_tolerances(g32, g64)
        for k in g64:
            top = float(np.abs(g64[k]).max())
            assert top > 0 and tol[k] <= 0.01 * top, (sel, k, tol[k], top)


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _actor(D=13, hidden=16, n_hidden=2, head=4):
    return _params(D=D, hidden=hidden, n_hidden=n_hidden, head=head)["actor"]


def test_squashed_policy_torch_builds_the_struct_over_the_callers_tensors():
    import space_gym_amd as sg
    env = _stub_env()
    par = _actor()
    sp = env.squashed_policy_torch(actor=par)
    s = sp.struct
    assert isinstance(sp, sg.SquashedPolicy)
    assert (s.struct_size, s.n_hidden, s.hidden, s.activation, s.log_std_min, s.log_std_max, s.reserved) == (96, 2, 16, 1, -20.0, 2.0, 0)
    assert sp.activation == "relu" and sp.log_std_bounds == (-20.0, 2.0)
    for l in range(3):
        assert s.actor.weight[l] == par[l][0].data_ptr() and s.actor.bias[l] == par[l][1].data_ptr()
    assert s.actor.weight[3] is None and len(sp.tensors) == 6 and sp.tensors[4] is par[2][0] and sp.workspace is None
    other = env.squashed_policy_torch(actor=par, log_std_bounds=(-5, 0.5), activation="tanh")
    assert other.struct.activation == 0 and other.log_std_bounds == (-5.0, 0.5)
    assert env._lib.names() == []  # a handle is made without a native call


def test_squashed_policy_torch_refuses_what_the_kernel_cannot_take():
    import torch
    env = _stub_env()
    par = _actor()
    with pytest.raises(ValueError, match="activation"):
        env.squashed_policy_torch(actor=par, activation="gelu")
    for bad in ((1.0, 0.0), (float("-inf"), 2.0), (-20.0, float("nan")), (1.0,), None):
        with pytest.raises(ValueError, match="log_std_bounds"):
            env.squashed_policy_torch(actor=par, log_std_bounds=bad)
    with pytest.raises(ValueError, match="n_hidden"):
        env.squashed_policy_torch(actor=par[-1:])
    with pytest.raises(ValueError, match="hidden must be"):
        env.squashed_policy_torch(actor=_actor(hidden=129))
    with pytest.raises(ValueError, match=r"actor\[2\] weight"):
        env.squashed_policy_torch(actor=_actor(head=2))  # a head of means alone
    with pytest.raises(ValueError, match=r"actor\[0\] weight"):
        env.squashed_policy_torch(actor=_actor(D=15))
    with pytest.raises(ValueError, match=r"actor\[1\] bias"):
        env.squashed_policy_torch(actor=[par[0], (par[1][0], _z(16, dtype=torch.float64)), par[2]])
    with pytest.raises(ValueError, match=r"actor\[0\] weight"):
        env.squashed_policy_torch(actor=[(torch.zeros((16, 13)), par[0][1])] + par[1:])  # a CPU tensor
    with pytest.raises(ValueError, match=r"actor\[0\] weight"):
        env.squashed_policy_torch(actor=[(_fake_cuda(torch.zeros((13, 16)).t()), par[0][1])] + par[1:])  # not contiguous
    env.discrete = True
    with pytest.raises(ValueError, match="discrete ids are not served"):
        env.squashed_policy_torch(actor=par)
    assert env._lib.names() == []


def test_the_calls_check_their_tensors_before_the_native_call():
    import torch
    env = _stub_env()
    par = _actor()
    sp = env.squashed_policy_torch(actor=par)
    B, n, K = env.num_envs, 24, 4
    obs_b, obs, eps = _z(B, 13), _z(n, 13), _z(n, 2)
    out = dict(action=_z(B, 2), logp=_z(B))
    a, lp = env.squashed_act_torch(sp, obs_b, seed=3, step=2 ** 33, deterministic=True, out=out)
    name, args = env._lib.calls[-1]
    assert a is out["action"] and lp is out["logp"] and name == "sg_squashed_act_device"
    assert args[3:6] == (3, 2 ** 33, 1) and args[6].value == a.data_ptr() and args[7].value == lp.data_ptr()
    assert env.squashed_act_torch(sp, obs_b, out=dict(action=out["action"]))[1] is None and env._lib.calls[-1][1][7] is None
    a, lp = env.squashed_sample_raw_torch(sp, obs, eps, out=dict(action=_z(n, 2), logp=_z(n)))
    name, args = env._lib.calls[-1]
    assert name == "sg_squashed_sample_device" and args[2] == n and args[4].value == eps.data_ptr() and args[5].value == a.data_ptr()
    env.squashed_sample_raw_torch(sp, obs, out=dict(action=a, logp=lp))
    assert env._lib.calls[-1][1][4] is None
    roll = dict(obs=_z(K + 1, B, 13), action=_z(K, B, 2), reward=_z(K, B), done=_z(K, B, dtype=torch.uint8), trunc=_z(K, B, dtype=torch.uint8))
    env.rollout_squashed_torch(sp, **roll, seed=5, first_step=7)
    name, args = env._lib.calls[-1]
    assert name == "sg_rollout_squashed_device" and args[1] == K and args[3:6] == (5, 7, 0) and args[8] is None and args[12] is None
    env.rollout_squashed_torch(sp, **roll, logp=_z(K, B))
    assert env._lib.calls[-1][1][8] is not None
    env._lib.calls.clear()
    pol = env.policy_torch(**_params())
    for call in (lambda h: env.squashed_act_torch(h, obs_b), lambda h: env.squashed_sample_raw_torch(h, obs), lambda h: env.squashed_sample_torch(h, obs),
                 lambda h: env.squashed_grad_torch(h, obs, g_logp=_z(n)), lambda h: env.rollout_squashed_torch(h, **roll)):
        for h in (pol, par, None):
            with pytest.raises(ValueError, match="handle squashed_policy_torch returns"):
                call(h)
    with pytest.raises(ValueError, match="obs"):
        env.squashed_act_torch(sp, obs)  # n rows, not num_envs
    with pytest.raises(ValueError, match=r"out\['action'\]"):
        env.squashed_act_torch(sp, obs_b, out=dict(logp=_z(B)))
    with pytest.raises(ValueError, match=r"out\['logp'\]"):
        env.squashed_act_torch(sp, obs_b, out=dict(action=_z(B, 2), logp=_z(B + 1)))
    with pytest.raises(ValueError, match="obs"):
        env.squashed_sample_raw_torch(sp, _z(n, 14))
    with pytest.raises(ValueError, match="obs"):
        env.squashed_sample_raw_torch(sp, _z(0, 13))
    with pytest.raises(ValueError, match="eps"):
        env.squashed_sample_raw_torch(sp, obs, _z(n, 3))
    with pytest.raises(ValueError, match="eps"):
        env.squashed_sample_torch(sp, obs, _z(n + 1, 2))
    with pytest.raises(ValueError, match=r"out\['action'\]"):
        env.squashed_sample_raw_torch(sp, obs, eps, out=dict(action=_z(n + 1, 2)))
    with pytest.raises(ValueError, match="nothing to compute"):
        env.squashed_grad_torch(sp, obs, eps)
    with pytest.raises(ValueError, match="g_action"):
        env.squashed_grad_torch(sp, obs, eps, g_action=_z(n))
    with pytest.raises(ValueError, match="g_logp"):
        env.squashed_grad_torch(sp, obs, eps, g_logp=_z(n, 2))
    good = dict(actor=[(_z(*w.shape), _z(*b.shape)) for w, b in par])
    with pytest.raises(ValueError, match=r"out\['actor'\]: expected 3"):
        env.squashed_grad_torch(sp, obs, eps, g_logp=_z(n), out=dict(actor=good["actor"][:2]))
    with pytest.raises(ValueError, match=r"out\['actor'\]\[2\] bias"):
        env.squashed_grad_torch(sp, obs, eps, g_logp=_z(n), out=dict(actor=good["actor"][:2] + [(_z(4, 16), _z(2))]))
    with pytest.raises(ValueError, match="action"):
        env.rollout_squashed_torch(sp, **{**roll, "action": _z(K, B)})
    with pytest.raises(ValueError, match="obs"):
        env.rollout_squashed_torch(sp, **{**roll, "obs": _z(K, B, 13)})
    with pytest.raises(ValueError, match="logp"):
        env.rollout_squashed_torch(sp, **roll, logp=_z(K + 1, B))
    with pytest.raises(ValueError, match="done"):
        env.rollout_squashed_torch(sp, **{**roll, "done": _z(K, B)})
    assert env._lib.names() == []
    env.discrete = True
    for call in (lambda: env.squashed_act_torch(sp, obs_b), lambda: env.squashed_sample_raw_torch(sp, obs), lambda: env.squashed_sample_torch(sp, obs),
                 lambda: env.squashed_grad_torch(sp, obs, g_logp=_z(n)), lambda: env.rollout_squashed_torch(sp, **roll)):
        with pytest.raises(ValueError, match="discrete ids are not served"):
            call()
    assert env._lib.names() == []


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("squashed_policy_torch", "squashed_act_torch", "rollout_squashed_torch", "squashed_sample_torch", "squashed_sample_raw_torch",
                     "squashed_grad_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
