"""CPU tests of the policy-population calls (sg_policy_population_* / sg_rollout_policy_population_device): the declarations and their
ctypes mirrors, the NumPy model (tests/population_model.py) against torch.autograd on P float64 module stacks, the grouping rule of the
gradient workgroups as arithmetic, the 1 % cap of every beyond-the-cap gradient case the GPU tests run, and the Python argument checks
with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from policy_grad_model import grad_tolerances
from population_model import (BEYOND_CASES, BEYOND_P, GROUP_CAP, OBS_DIM, act, beyond_case, beyond_n, beyond_reference, bit_equal_to_single,
                              evaluate, flat_member, grad_rows, groups, groups_single, member, members, random_population, workspace_floats)
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _torch_net
from test_snapshot_device import _header_args

REL = 1e-10  # float64 model against float64 autograd: the figure of tests/test_q.py, test_squashed.py and test_dqn.py for the same comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    assert _header_args("sg_policy_population_act_device") == [
        "sg_env *env", "const sg_policy *policy", "int32_t members", "const float *obs_dev", "uint64_t seed", "uint64_t step",
        "int32_t deterministic", "void *action_out", "float *logp_out", "float *value_out", "void *hip_stream"]
    assert _header_args("sg_rollout_policy_population_device") == [
        "sg_env *env", "int32_t n_steps", "const sg_policy *policy", "int32_t members", "uint64_t seed", "uint64_t first_step",
        "int32_t deterministic", "float *obs", "void *action", "float *logp", "float *value", "float *reward", "uint8_t *done",
        "uint8_t *truncated", "const sg_terminal_list *terminal_list", "float *terminal_value", "void *hip_stream"]
    assert _header_args("sg_policy_population_evaluate_device") == [
        "sg_env *env", "const sg_policy *policy", "int32_t members", "int64_t n", "const float *obs", "const void *action", "float *logp_out",
        "float *entropy_out", "float *value_out", "void *hip_stream"]
    assert _header_args("sg_policy_population_grad_device") == [
        "sg_env *env", "const sg_policy *policy", "int32_t members", "int64_t n", "const float *obs", "const void *action",
        "const float *g_logp", "const float *g_entropy", "const float *g_value", "const sg_policy_grads *grads", "void *workspace",
        "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_policy_population_grad_workspace_bytes", "size_t") == [
        "sg_env *env", "const sg_policy *policy", "int32_t members", "int64_t n"]
    # the single-policy calls with `members` after the policy
    assert [a for a in _header_args("sg_policy_population_act_device") if a != "int32_t members"] == _header_args("sg_policy_act_device")
    assert [a for a in _header_args("sg_rollout_policy_population_device") if a != "int32_t members"] == _header_args("sg_rollout_policy_device")
    vp, P, G, i32, i64, u64 = C.c_void_p, C.POINTER(_native.SgPolicy), C.POINTER(_native.SgPolicyGrads), C.c_int32, C.c_int64, C.c_uint64
    assert _native.SYMBOLS["sg_policy_population_act_device"] == (C.c_int, [vp, P, i32, vp, u64, u64, i32, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_rollout_policy_population_device"] == (
        C.c_int, [vp, i32, P, i32, u64, u64, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(_native.SgTerminalList), vp, vp])
    assert _native.SYMBOLS["sg_policy_population_evaluate_device"] == (C.c_int, [vp, P, i32, i64, vp, vp, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_policy_population_grad_device"] == (C.c_int, [vp, P, i32, i64, vp, vp, vp, vp, vp, G, vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_policy_population_grad_workspace_bytes"] == (C.c_size_t, [vp, P, i32, i64])
    assert C.sizeof(_native.SgPolicy) == 160  # sg_policy keeps its size: `members` is an argument
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_population.inc" in build.HEADERS and '#include "sg_population.inc"' in src
    assert re.search(r"kNetsPopulation = 32\b", src)
    inc = open(os.path.join(build.CSRC, "sg_population.inc")).read()
    for kernel in ("population_act_kernel", "population_evaluate_kernel", "population_grad_kernel", "population_grad_reduce_kernel"):
        assert re.search(r"void %s\(" % kernel, inc), kernel
    # no arithmetic of its own: the shared device functions are what the kernels call
    assert inc.count("policy_act_tail(") == 1 and inc.count("policy_score(") == 2 and inc.count("policy_grad_net<NT>(") == 2
    assert inc.count("policy_grad_reduce_element(") == 1 and inc.count("policy_net<NT>(") == 4
    assert not re.search(r"\b(fmaf|expf|logf|__expf|philox4x32_10|box_muller)\(", inc)
    assert "atomic" not in inc


def _torch_member(pol, obs, action, g, activation, continuous):
    """logp, entropy, value and every parameter gradient of sum_i (g_logp logp + g_entropy entropy + g_value value) of one member, from
    float64 torch modules"""
    import torch
    actor, critic = _torch_net(pol["actor"], activation), _torch_net(pol["critic"], activation)
    x = torch.from_numpy(obs.astype(np.float64))
    head = actor(x)
    log_std = None
    if continuous:
        log_std = torch.nn.Parameter(torch.from_numpy(pol["log_std"].astype(np.float64)))
        dist = torch.distributions.Normal(head, log_std.exp().expand_as(head))
        logp, ent = dist.log_prob(torch.from_numpy(action.astype(np.float64))).sum(1), dist.entropy().sum(1)
    else:
        dist = torch.distributions.Categorical(logits=head)
        logp, ent = dist.log_prob(torch.from_numpy(action.astype(np.int64))), dist.entropy()
    value = critic(x)[:, 0]
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    (t(g["logp"]) * logp + t(g["entropy"]) * ent + t(g["value"]) * value).sum().backward()
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    grads = {}
    for name, net in (("actor", actor), ("critic", critic)):
        for l, m in enumerate(lin(net)):
            grads[f"{name}.{l}.weight"], grads[f"{name}.{l}.bias"] = m.weight.grad.numpy(), m.bias.grad.numpy()
    if continuous:
        grads["log_std"] = log_std.grad.numpy()
    return logp.detach().numpy(), ent.detach().numpy(), value.detach().numpy(), grads


@pytest.mark.parametrize("continuous", [True, False])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", [(1, 1), (33, 2), (128, 3)])
def test_model_equals_torch_autograd_on_float64_module_stacks(hidden, n_hidden, activation, continuous):
    P, n = 3, 37
    rng = np.random.default_rng([hidden, n_hidden, int(continuous)])
    pop = random_population(rng, P, OBS_DIM, hidden, n_hidden, 2 if continuous else 6, continuous=continuous)
    assert members(pop) == P and pop["actor"][0][0].shape == (P, hidden, OBS_DIM) and pop["actor"][-1][1].shape == (P, 2 if continuous else 6)
    assert (pop["log_std"].shape == (P, 2)) if continuous else pop["log_std"] is None
    obs = rng.standard_normal((P, n, OBS_DIM)).astype(np.float32)
    action = rng.standard_normal((P, n, 2)).astype(np.float32) if continuous else rng.integers(0, 6, (P, n)).astype(np.int32)
    g = {k: rng.standard_normal((P, n)).astype(np.float32) for k in ("logp", "entropy", "value")}
    got = evaluate(pop, obs, action, g["logp"], g["entropy"], g["value"], activation=activation)
    assert got["logp"].shape == got["entropy"].shape == got["value"].shape == (P, n)
    assert got["actor"][0][0].shape == pop["actor"][0][0].shape and got["critic"][-1][1].shape == (P, 1)
    for m in range(P):
        logp, ent, value, grads = _torch_member(member(pop, m), obs[m], action[m], {k: v[m] for k, v in g.items()}, activation, continuous)
        assert rel(got["logp"][m], logp) <= REL and rel(got["entropy"][m], ent) <= REL and rel(got["value"][m], value) <= REL
        mine = flat_member(got, m)
        assert set(mine) == set(grads)
        for k in grads:
            assert mine[k].shape == grads[k].shape and rel(mine[k], grads[k]) <= REL, (m, k, rel(mine[k], grads[k]))
    # members are independent: another member's parameters do not reach member 0's results
    other = random_population(rng, P, OBS_DIM, hidden, n_hidden, 2 if continuous else 6, continuous=continuous)
    for key in ("actor", "critic"):
        for (W, b), (W0, b0) in zip(other[key], pop[key]):
            W[0], b[0] = W0[0], b0[0]
    if continuous:
        other["log_std"][0] = pop["log_std"][0]
    again = evaluate(other, obs, action, g["logp"], g["entropy"], g["value"], activation=activation)
    a, b = flat_member(got, 0), flat_member(again, 0)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(got["logp"][1], again["logp"][1])


def test_act_blocks_follow_the_local_index_and_the_noise_the_global_one():
    import policy_model
    P, B, base = 3, 12, 1000
    rng = np.random.default_rng(2)
    pop = random_population(rng, P, OBS_DIM, 8, 1, 2)
    obs = rng.standard_normal((B, OBS_DIM)).astype(np.float32)
    got = act(pop, obs, seed=7, step=2 ** 32 + 1, env_index_base=base)
    for m in range(P):
        rows = slice(m * 4, (m + 1) * 4)
        one = policy_model.act(member(pop, m), obs, seed=7, step=2 ** 32 + 1, env_index_base=base)  # the whole batch under member m
        for k in ("action", "logp", "value"):
            assert np.array_equal(got[k][rows], one[k][rows]), (m, k)
    assert not np.array_equal(got["value"][4:8], policy_model.act(member(pop, 0), obs)["value"][4:8])


def test_the_grouping_rule_and_its_bit_equality_condition():
    """G = min(ceil(n / R), max(1, 256 / P)): equal to the single call's min(ceil(n / R), 256) exactly when ceil(n / R) <= 256 / P (for
    P <= 256), which is the condition under which a member's gradient is the single call's bits"""
    assert [grad_rows(h) for h in (1, 32, 33, 64, 65, 97, 128)] == [256, 256, 128, 128, 64, 64, 64]
    for R in (256, 128, 64):
        for P in (1, 2, 3, 4, 16, 64, 85, 86, 255, 256, 257, 1000, 65535):
            cap = max(1, GROUP_CAP // P)
            for tiles in (1, 2, cap - 1, cap, cap + 1, 85, 86, 256, 257, 5000):
                if tiles < 1:
                    continue
                for n in {(tiles - 1) * R + 1, tiles * R}:
                    G = groups(n, R, P)
                    assert 1 <= G <= cap and G <= tiles and G == min(tiles, cap)
                    same = G == groups_single(n, R)
                    if P <= GROUP_CAP:
                        assert bit_equal_to_single(n, R, P) == (tiles <= GROUP_CAP // P)
                        assert same == (bit_equal_to_single(n, R, P) or P == 1), (R, P, tiles)
                    else:
                        assert not bit_equal_to_single(n, R, P) and G == 1
                    assert workspace_floats(n, R, P, 7) <= max(GROUP_CAP, P) * 7  # the bound a per-member cap of 256 would not keep
    assert groups(10 ** 7, 64, 1) == 256 and groups(10 ** 7, 64, 256) == 1 and groups(10 ** 7, 64, 3) == 85
    # the GPU suite's shapes: n = 1, 200, 2049 at P = 3 are within the cap for every R; n = 85 R + 300 is beyond it
    for R in (256, 128, 64):
        assert all(bit_equal_to_single(n, R, 3) for n in (1, 200, 2049))
        assert not bit_equal_to_single(beyond_n(R), R, BEYOND_P) and -(-beyond_n(R) // R) in (87, 88, 90) and groups(beyond_n(R), R, BEYOND_P) == 85
        assert beyond_n(R) - 85 * R == 300  # workgroups 0 .. of a member take a second row tile: of their own member only


@pytest.mark.parametrize("hidden,R", BEYOND_CASES)
def test_every_beyond_the_cap_gradient_case_has_a_tolerance_of_at_most_one_percent(hidden, R):
    """8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) <= 1 % of max|G64| per tensor and per member, for the very cases (the same generator,
    the same seed) tests/test_gpu_population.py runs: a GPU failure cannot be the inputs' fault"""
    c = beyond_case(hidden, R)
    assert c["n"] == 85 * R + 300 and c["obs"].shape == (BEYOND_P, c["n"], OBS_DIM)
    r64, r32 = beyond_reference(c, np.float64), beyond_reference(c, np.float32)
    for m in range(BEYOND_P):
        g64, g32 = flat_member(r64, m), flat_member(r32, m)
        tol = grad_tolerances(g32, g64)
        assert len(g64) == 2 * 2 * 2 + 1
        for k in g64:
            top = float(np.abs(g64[k]).max())
            assert top > 0 and tol[k] <= 0.01 * top, (m, k, tol[k], top)


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _stacked(P=4, D=13, hidden=16, n_hidden=2, head=2, **over):
    dims = [D] + [hidden] * n_hidden
    net = lambda out: [(_z(P, o, i), _z(P, o)) for i, o in zip(dims[:-1], dims[1:])] + [(_z(P, out, hidden), _z(P, out))]
    p = dict(actor=net(head), critic=net(1), log_std=_z(P, 2))
    p.update(over)
    return p


def test_policy_population_torch_builds_the_struct_over_the_stacked_tensors():
    import space_gym_amd as sg
    env = _stub_env()
    par = _stacked()
    pop = env.policy_population_torch(4, **par)
    s = pop.struct
    assert isinstance(pop, sg.PolicyPopulation) and pop.members == 4 and pop.has_critic and pop.workspace is None
    assert (s.struct_size, s.n_hidden, s.hidden, s.activation, s.head, s.reserved) == (160, 2, 16, 0, 2, 0)
    for l in range(3):
        assert s.actor.weight[l] == par["actor"][l][0].data_ptr() and s.actor.bias[l] == par["actor"][l][1].data_ptr()
        assert s.critic.weight[l] == par["critic"][l][0].data_ptr() and s.critic.bias[l] == par["critic"][l][1].data_ptr()
    assert s.actor.weight[3] is None and s.log_std == par["log_std"].data_ptr() and len(pop.tensors) == 13
    # a member is a plain Policy over views: no copy
    one = env.population_member_torch(pop, 2)
    assert isinstance(one, sg.Policy) and one.has_critic and (one.n_hidden, one.hidden, one.activation) == (2, 16, "tanh")
    for l in range(3):
        assert one.struct.actor.weight[l] == par["actor"][l][0][2].data_ptr() == par["actor"][l][0].data_ptr() + 2 * 4 * par["actor"][l][0][0].numel()
        assert one.struct.critic.bias[l] == par["critic"][l][1][2].data_ptr()
    assert one.struct.log_std == par["log_std"].data_ptr() + 2 * 2 * 4
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="member index"):
            env.population_member_torch(pop, bad)
    assert env.policy_population_torch(2, **_stacked(P=2, critic=None), activation="relu").struct.activation == 1
    assert env._lib.names() == []  # a handle is made without a native call


def test_policy_population_torch_refuses_what_the_kernels_cannot_take():
    import torch
    env = _stub_env()
    par = _stacked()
    with pytest.raises(ValueError, match=r"actor\[0\] weight"):
        env.policy_population_torch(2, **par)  # the wrong leading dimension
    with pytest.raises(ValueError, match=r"actor\[1\] bias"):
        env.policy_population_torch(4, **dict(par, actor=[par["actor"][0], (par["actor"][1][0], _z(2, 16)), par["actor"][2]]))
    with pytest.raises(ValueError, match=r"log_std"):
        env.policy_population_torch(4, **dict(par, log_std=_z(2)))
    with pytest.raises(ValueError, match=r"actor\[0\]"):
        env.policy_population_torch(4, **dict(par, actor=[(_z(16, 13), _z(16))] + par["actor"][1:]))  # not stacked
    w = _fake_cuda(torch.zeros((16, 4, 16)).transpose(0, 1))  # [4, 16, 16], not contiguous
    assert tuple(w.shape) == (4, 16, 16) and not w.is_contiguous()
    with pytest.raises(ValueError, match=r"actor\[1\] weight.*not contiguous"):
        env.policy_population_torch(4, **dict(par, actor=[par["actor"][0], (w, par["actor"][1][1]), par["actor"][2]]))
    with pytest.raises(ValueError, match=r"critic\[0\] bias.*not contiguous"):
        env.policy_population_torch(4, **dict(par, critic=[(par["critic"][0][0], _fake_cuda(torch.zeros((16, 4)).t()))] + par["critic"][1:]))
    with pytest.raises(ValueError, match="does not divide num_envs"):
        env.policy_population_torch(3, **_stacked(P=3))  # 8 envs
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="members must be"):
            env.policy_population_torch(bad, **par)
    with pytest.raises(ValueError, match="critic: expected 2 hidden layers of width 16"):
        env.policy_population_torch(4, **dict(par, critic=_stacked(hidden=8)["critic"]))
    with pytest.raises(ValueError, match="critic: expected 2 hidden layers"):
        env.policy_population_torch(4, **dict(par, critic=_stacked(n_hidden=1)["critic"]))
    with pytest.raises(ValueError, match=r"critic\[2\] weight"):
        env.policy_population_torch(4, **dict(par, critic=par["actor"]))  # a head of 2
    with pytest.raises(ValueError, match="activation"):
        env.policy_population_torch(4, **par, activation="gelu")
    with pytest.raises(ValueError, match="hidden must be"):
        env.policy_population_torch(4, **_stacked(hidden=129))
    with pytest.raises(ValueError, match="log_std: a continuous id needs"):
        env.policy_population_torch(4, **dict(par, log_std=None))
    env.discrete = True
    with pytest.raises(ValueError, match="log_std: the discrete ids take none"):
        env.policy_population_torch(4, **_stacked(head=6))
    assert env.policy_population_torch(4, **_stacked(head=6, log_std=None)).struct.head == 6
    assert env._lib.names() == []


def test_the_calls_check_their_tensors_before_the_native_call():
    import torch
    env = _stub_env()
    par = _stacked()
    pop = env.policy_population_torch(4, **par)
    B, P, n, K = env.num_envs, 4, 24, 3
    u8 = torch.uint8
    obs_b = _z(B, 13)
    out = dict(action=_z(B, 2), logp=_z(B), value=_z(B))
    a, lp, v = env.population_act_torch(pop, obs_b, seed=3, step=2 ** 33, deterministic=True, out=out)
    name, args = env._lib.calls[-1]
    assert name == "sg_policy_population_act_device" and a is out["action"] and lp is out["logp"] and v is out["value"]
    assert args[2] == 4 and args[4:7] == (3, 2 ** 33, 1) and [x.value for x in args[7:10]] == [a.data_ptr(), lp.data_ptr(), v.data_ptr()]
    assert env.population_act_torch(pop, obs_b, out=dict(value=out["value"]))[:2] == (None, None)  # values only
    assert env._lib.calls[-1][1][7:9] == (None, None)
    roll = dict(obs=_z(K + 1, B, 13), action=_z(K, B, 2), logp=_z(K, B), value=_z(K + 1, B), reward=_z(K, B), done=_z(K, B, dtype=u8),
                trunc=_z(K, B, dtype=u8))
    env.rollout_population_torch(pop, **roll, seed=5, first_step=7, terminal_value=_z(K, B))
    name, args = env._lib.calls[-1]
    assert name == "sg_rollout_policy_population_device" and args[1] == K and args[3] == 4 and args[4:7] == (5, 7, 0)
    assert args[14] is None and args[15] is not None
    env.rollout_population_torch(pop, **roll)
    assert env._lib.calls[-1][1][15] is None
    obs, action = _z(P, n, 13), _z(P, n, 2)
    lo, en, va = env.population_evaluate_raw_torch(pop, obs, action, out=dict(logp=_z(P, n), entropy=_z(P, n), value=_z(P, n)))
    name, args = env._lib.calls[-1]
    assert name == "sg_policy_population_evaluate_device" and args[2:4] == (4, n) and tuple(lo.shape) == tuple(va.shape) == (P, n)
    env._lib.calls.clear()
    plain = env.population_member_torch(pop, 0)
    for call in (lambda x: env.population_act_torch(x, obs_b), lambda x: env.population_evaluate_raw_torch(x, obs, action),
                 lambda x: env.population_evaluate_torch(x, obs, action), lambda x: env.population_grad_torch(x, obs, action),
                 lambda x: env.rollout_population_torch(x, **roll), lambda x: env.population_member_torch(x, 0)):
        for x in (plain, par, None):
            with pytest.raises(ValueError, match="handle policy_population_torch returns"):
                call(x)
    with pytest.raises(ValueError, match="handle policy_torch returns"):
        env.policy_act_torch(pop, obs_b)  # and a population is no Policy
    with pytest.raises(ValueError, match="obs"):
        env.population_act_torch(pop, _z(B + 4, 13))
    with pytest.raises(ValueError, match=r"out\['logp'\]"):
        env.population_act_torch(pop, obs_b, out=dict(action=_z(B, 2), logp=_z(B + 1)))
    with pytest.raises(ValueError, match="expected action"):
        env.population_act_torch(pop, obs_b, out={})
    with pytest.raises(ValueError, match="obs"):
        env.population_evaluate_raw_torch(pop, _z(n, 13), _z(n, 2))  # not [P, n, D]
    with pytest.raises(ValueError, match="obs"):
        env.population_evaluate_raw_torch(pop, _z(3, n, 13), _z(3, n, 2))  # another P
    with pytest.raises(ValueError, match="action"):
        env.population_evaluate_raw_torch(pop, obs, _z(P, n))
    with pytest.raises(ValueError, match=r"out\['entropy'\]"):
        env.population_evaluate_raw_torch(pop, obs, action, out=dict(entropy=_z(n, P)))
    with pytest.raises(ValueError, match="at least one"):
        env.population_evaluate_raw_torch(pop, obs, action, out={})
    with pytest.raises(ValueError, match="g_logp"):
        env.population_grad_torch(pop, obs, action, g_logp=_z(P * n))
    with pytest.raises(ValueError, match=r"out\['critic'\]"):
        env.population_grad_torch(pop, obs, action, g_value=_z(P, n), out=dict(actor=[(_z(*w.shape), _z(*b.shape)) for w, b in par["actor"]],
                                                                                  log_std=_z(P, 2)))
    with pytest.raises(ValueError, match=r"out\['actor'\]\[0\] weight"):
        env.population_grad_torch(pop, obs, action, out=dict(actor=[(_z(16, 13), _z(16)), (_z(16, 16), _z(16)), (_z(2, 16), _z(2))], log_std=_z(P, 2)))
    with pytest.raises(ValueError, match=r"out\['log_std'\]"):
        env.population_grad_torch(pop, obs, action, out=dict(actor=[(_z(*w.shape), _z(*b.shape)) for w, b in par["actor"]], log_std=_z(2)))
    with pytest.raises(ValueError, match="terminal_value"):
        env.rollout_population_torch(pop, **roll, terminal_value=_z(100))  # a list-shaped terminal_value is not served
    with pytest.raises(ValueError, match="value"):
        env.rollout_population_torch(pop, **{**roll, "value": None})
    nc = env.policy_population_torch(4, **dict(par, critic=None))
    with pytest.raises(ValueError, match="no critic"):
        env.rollout_population_torch(nc, **{**roll, "value": None}, terminal_value=_z(K, B))
    with pytest.raises(ValueError, match="no critic"):
        env.population_grad_torch(nc, obs, action, g_value=_z(P, n))
    with pytest.raises(ValueError, match="no critic"):
        env.population_act_torch(nc, obs_b, out=dict(value=_z(B)))
    assert env._lib.names() == []
    # a handle made on another batch: its members must divide THIS handle's envs
    env.num_envs = 6
    with pytest.raises(ValueError, match="do not divide num_envs"):
        env.population_act_torch(pop, _z(6, 13))
    with pytest.raises(ValueError, match="do not divide num_envs"):
        env.rollout_population_torch(pop, **roll)
    assert env._lib.names() == []


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("policy_population_torch", "population_member_torch", "population_act_torch", "rollout_population_torch",
                     "population_evaluate_raw_torch", "population_grad_torch", "population_evaluate_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
