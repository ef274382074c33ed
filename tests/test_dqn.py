"""CPU tests of the DQN head (sg_dqn_act_device / sg_rollout_dqn_device / sg_dqn_evaluate_device / sg_dqn_grad_device): the
declarations, the NumPy model (tests/dqn_model.py) against torch.autograd in float64, relu'(0) = 0, the statistics of the epsilon-greedy
draw of stream tag 7, the float32 mode, the 1 % cap of every gradient case the GPU tests run, and the Python argument checks with the
native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dqn_model import ACTIONS, NETS, SELECTIONS, STREAM_DQN, act, case, evaluate, first_argmax, flat, grad_case, grad_cases, grad_reference
from dqn_model import grad_tolerances, words
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_snapshot_device import _header_args

REL = 1e-10  # float64 model against float64 autograd: the figure of tests/test_q.py and tests/test_squashed.py for the same comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    assert _header_args("sg_dqn_act_device") == [
        "sg_env *env", "const sg_dqn *dqn", "const float *obs_dev", "uint64_t seed", "uint64_t step", "float epsilon",
        "const float *epsilon_dev", "int32_t *action_out", "float *q_out", "void *hip_stream"]
    assert _header_args("sg_rollout_dqn_device") == [
        "sg_env *env", "int32_t n_steps", "const sg_dqn *dqn", "uint64_t seed", "uint64_t first_step", "float epsilon",
        "const float *epsilon_dev", "float *obs", "int32_t *action", "float *q", "float *reward", "uint8_t *done", "uint8_t *truncated",
        "const sg_terminal_list *terminal_list", "void *hip_stream"]
    assert _header_args("sg_dqn_evaluate_device") == [
        "sg_env *env", "const sg_dqn *dqn", "int64_t n", "const float *obs", "const int32_t *action", "float *q_all_out",
        "float *q_taken_out", "float *q_max_out", "int32_t *argmax_out", "void *hip_stream"]
    assert _header_args("sg_dqn_grad_device") == [
        "sg_env *env", "const sg_dqn *dqn", "int64_t n", "const float *obs", "const int32_t *action", "const float *g_taken",
        "const float *g_all", "const sg_dqn_grads *grads", "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_dqn_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_dqn *dqn", "int64_t n"]
    vp, P, G = C.c_void_p, C.POINTER(_native.SgDqn), C.POINTER(_native.SgDqnGrads)
    assert _native.SYMBOLS["sg_dqn_act_device"] == (C.c_int, [vp, P, vp, C.c_uint64, C.c_uint64, C.c_float, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_rollout_dqn_device"] == (
        C.c_int, [vp, C.c_int32, P, C.c_uint64, C.c_uint64, C.c_float, vp, vp, vp, vp, vp, vp, vp, C.POINTER(_native.SgTerminalList), vp])
    assert _native.SYMBOLS["sg_dqn_evaluate_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp, vp, vp, vp])
    assert _native.SYMBOLS["sg_dqn_grad_device"] == (C.c_int, [vp, P, C.c_int64, vp, vp, vp, vp, G, vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_dqn_grad_workspace_bytes"] == (C.c_size_t, [vp, P, C.c_int64])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls in (("sg_dqn", _native.SgDqn), ("sg_dqn_grads", _native.SgDqnGrads)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_], name
    assert C.sizeof(_native.SgDqn) == 24 + 64 and _native.SgDqn.reserved.offset == 16 and _native.SgDqn.net.offset == 24
    assert C.sizeof(_native.SgDqnGrads) == 8 + 64 and _native.SgDqnGrads.net.offset == 8
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_dqn.inc" in build.HEADERS and '#include "sg_dqn.inc"' in src
    assert re.search(r"kNetsDqn = 16\b", src)
    inc = open(os.path.join(build.CSRC, "sg_dqn.inc")).read()
    assert re.search(r"constexpr uint32_t kStreamDqn = 7u;", inc) and STREAM_DQN == 7
    assert "kStreamDqn, o)" in inc
    for kernel in ("dqn_act_kernel", "dqn_evaluate_kernel", "dqn_grad_kernel"):
        assert re.search(r"void %s\(" % kernel, inc), kernel
    assert inc.count("dqn_argmax(out, mx)") == 2  # ONE argmax, in the act and in the evaluate kernel


def _torch_dqn(net, obs, action, gt, ga, activation):
    """q_all, q_taken via gather, and every parameter gradient of sum_i (gt q_taken + ga . q_all), from float64 torch"""
    import torch
    mod = _torch_net(net, activation)
    q = mod(torch.from_numpy(obs.astype(np.float64)))
    taken = q.gather(1, torch.from_numpy(action.astype(np.int64))[:, None])[:, 0]
    loss = 0.0
    if gt is not None:
        loss = loss + (torch.from_numpy(np.asarray(gt, np.float64)) * taken).sum()
    if ga is not None:
        loss = loss + (torch.from_numpy(np.asarray(ga, np.float64)) * q).sum()
    loss.backward()
    lin = [m for m in mod if isinstance(m, torch.nn.Linear)]
    grads = flat(dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin]))
    return q.detach().numpy(), taken.detach().numpy(), grads


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,n_hidden", NETS)
def test_model_equals_torch_autograd_in_float64(hidden, n_hidden, activation):
    import torch
    c = case(13, 37, hidden, n_hidden, seed=1)
    assert set(c["action"].tolist()) == set(range(ACTIONS))
    for sel in SELECTIONS:
        gt = c["g_taken"] if sel in ("both", "taken") else None
        ga = c["g_all"] if sel in ("both", "all") else None
        got = evaluate(c["net"], c["obs"], c["action"], gt, ga, activation=activation)
        q, taken, grads = _torch_dqn(c["net"], c["obs"], c["action"], gt, ga, activation)
        assert got["q_all"].shape == (37, ACTIONS) and rel(got["q_all"], q) <= REL and rel(got["q_taken"], taken) <= REL
        assert np.array_equal(got["argmax"], torch.from_numpy(got["q_all"]).argmax(1).numpy())
        assert np.array_equal(got["q_max"], got["q_all"].max(axis=1))
        mine = flat(got)
        assert set(mine) == set(grads) and len(mine) == 2 * (n_hidden + 1)
        for k in grads:
            assert mine[k].shape == grads[k].shape and rel(mine[k], grads[k]) <= REL, (sel, k, rel(mine[k], grads[k]))
    plain = evaluate(c["net"], c["obs"], activation=activation)
    assert plain["q_taken"] is None and "actor" not in plain and np.array_equal(plain["q_all"], got["q_all"])
    # g_all of zeros beside g_taken is g_taken alone
    a = flat(evaluate(c["net"], c["obs"], c["action"], c["g_taken"], np.zeros((37, ACTIONS), np.float32), activation=activation))
    b = flat(evaluate(c["net"], c["obs"], c["action"], c["g_taken"], None, activation=activation))
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_the_first_of_equal_maxima_is_the_argmax_and_relu_has_slope_zero_at_zero():
    import torch
    q = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, 0.0], [5.0, 5.0, 5.0, 5.0, 5.0, 5.0], [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    assert first_argmax(q).tolist() == [1, 0, 5]
    # a hidden unit whose pre-activation is exactly 0 passes no gradient, as torch's ReLU
    D = 3
    net = [(np.zeros((2, D), np.float32), np.array([0.0, 1.0], np.float32)),
           (np.ones((ACTIONS, 2), np.float32), np.zeros(ACTIONS, np.float32))]
    obs = np.ones((4, D), np.float32)
    action = np.array([0, 1, 2, 3], np.int32)
    for dtype in (np.float64, np.float32):
        g = flat(evaluate(net, obs, action, np.ones(4, np.float32), None, activation="relu", dtype=dtype))
        assert not g["actor.0.weight"][0].any() and g["actor.0.bias"][0] == 0 and g["actor.0.bias"][1] == 4
    _, _, ref = _torch_dqn(net, obs, action, np.ones(4), None, "relu")
    assert all(np.array_equal(g[k], ref[k]) for k in ref)
    t = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    torch.relu(t).sum().backward()
    assert t.grad.item() == 0.0  # torch's own convention


def test_exploration_statistics_and_the_per_env_epsilon():
    """2^16 envs at epsilon 0.25: the explored share and every random action's share within 4 standard deviations; 0 explores nowhere,
    1 everywhere; a per-env vector decides as the scalar wherever the two agree"""
    from policy_model import words as policy_words
    from squashed_model import words as squashed_words
    B, D = 2 ** 16, 3
    net = [(np.zeros((2, D), np.float32), np.zeros(2, np.float32)), (np.zeros((ACTIONS, 2), np.float32), np.arange(ACTIONS, dtype=np.float32))]
    obs = np.zeros((B, D), np.float32)
    got = act(net, obs, seed=123, step=9, epsilon=0.25)
    share = got["explore"].mean()
    assert abs(share - 0.25) <= 4 * np.sqrt(0.25 * 0.75 / B), share
    assert got["random_action"].min() == 0 and got["random_action"].max() == ACTIONS - 1
    for j in range(ACTIONS):
        s = (got["random_action"] == j).mean()
        assert abs(s - 1 / 6) <= 4 * np.sqrt((1 / 6) * (5 / 6) / B), (j, s)
        s = (got["random_action"][got["explore"]] == j).mean()  # and among the envs that explore
        assert abs(s - 1 / 6) <= 4 * np.sqrt((1 / 6) * (5 / 6) / got["explore"].sum()), (j, s)
    assert (got["argmax"] == ACTIONS - 1).all()  # the bias makes action 5 the greedy one
    assert np.array_equal(got["action"], np.where(got["explore"], got["random_action"], ACTIONS - 1))
    assert not act(net, obs, seed=123, step=9, epsilon=0.0)["explore"].any()
    assert act(net, obs, seed=123, step=9, epsilon=1.0)["explore"].all()
    vec = np.where(np.arange(B) % 3 == 0, 0.25, np.where(np.arange(B) % 3 == 1, 0.0, 1.0)).astype(np.float32)
    per = act(net, obs, seed=123, step=9, epsilon=vec)
    assert np.array_equal(per["explore"][0::3], got["explore"][0::3]) and not per["explore"][1::3].any() and per["explore"][2::3].all()
    assert np.array_equal(per["random_action"], got["random_action"])
    assert not act(net, obs[:8], epsilon=np.full(8, np.nan, np.float32))["explore"].any()  # a NaN never explores
    # the draw is keyed by (seed, step, global env) and the tag 7
    part = act(net, obs[:50], seed=123, step=9, epsilon=0.25, env_index_base=64)
    assert np.array_equal(part["explore"], got["explore"][64:114]) and np.array_equal(part["random_action"], got["random_action"][64:114])
    assert not np.array_equal(act(net, obs, seed=123, step=10, epsilon=0.25)["explore"], got["explore"])
    assert not np.array_equal(act(net, obs, seed=124, step=9, epsilon=0.25)["random_action"], got["random_action"])
    assert int(words(1, 2, [3])[0][0]) not in (int(policy_words(1, 2, [3])[0][0]), int(squashed_words(1, 2, [3])[0][0]))
    assert int(words(1, 2, [3])[0][0]) != int(words(1, 2 + 2 ** 32, [3])[0][0])  # the high word of the step is part of the counter


def test_float32_mode_is_float32_and_close():
    c = case(13, 300, 33, 2, seed=3)
    r64 = evaluate(c["net"], c["obs"], c["action"], c["g_taken"], c["g_all"])
    r32 = evaluate(c["net"], c["obs"], c["action"], c["g_taken"], c["g_all"], dtype=np.float32)
    g64, g32 = flat(r64), flat(r32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
    for k in ("q_all", "q_taken", "q_max"):
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64 and 0 < np.abs(r32[k] - r64[k]).max() < 1e-4


@pytest.mark.parametrize("obs_dim,n,hidden,n_hidden,activation", grad_cases())
def test_every_gpu_gradient_case_has_a_tolerance_of_at_most_one_percent(obs_dim, n, hidden, n_hidden, activation):
    """8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) <= 1 % of max|G64| per tensor, for the very cases (the same generator, the same
    seed) tests/test_gpu_dqn.py runs: a GPU failure cannot be the inputs' fault"""
    c = grad_case(obs_dim, n, hidden, n_hidden)
    for sel in SELECTIONS:
        g64, g32 = grad_reference(c, activation, sel, np.float64), grad_reference(c, activation, sel, np.float32)
        tol = grad_tolerances(g32, g64)
        for k in g64:
            top = float(np.abs(g64[k]).max())
            assert top > 0 and tol[k] <= 0.01 * top, (sel, k, tol[k], top)


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _net(D=13, hidden=16, n_hidden=2, head=ACTIONS):
    return _params(D=D, hidden=hidden, n_hidden=n_hidden, head=head)["actor"]


def _discrete_env():
    env = _stub_env()
    env.discrete = True
    return env


def test_dqn_torch_builds_the_struct_over_the_callers_tensors():
    import space_gym_amd as sg
    env = _discrete_env()
    par = _net()
    h = env.dqn_torch(net=par)
    s = h.struct
    assert isinstance(h, sg.Dqn)
    assert (s.struct_size, s.n_hidden, s.hidden, s.activation, s.reserved) == (88, 2, 16, 1, 0) and h.activation == "relu"
    for l in range(3):
        assert s.net.weight[l] == par[l][0].data_ptr() and s.net.bias[l] == par[l][1].data_ptr()
    assert s.net.weight[3] is None and len(h.tensors) == 6 and h.tensors[4] is par[2][0] and h.workspace is None
    assert env.dqn_torch(net=par, activation="tanh").struct.activation == 0
    assert env._lib.names() == []  # a handle is made without a native call


def test_dqn_torch_refuses_what_the_kernel_cannot_take():
    import torch
    env = _discrete_env()
    par = _net()
    with pytest.raises(ValueError, match="activation"):
        env.dqn_torch(net=par, activation="gelu")
    with pytest.raises(ValueError, match="n_hidden"):
        env.dqn_torch(net=par[-1:])
    with pytest.raises(ValueError, match="hidden must be"):
        env.dqn_torch(net=_net(hidden=129))
    with pytest.raises(ValueError, match=r"net\[2\] weight"):
        env.dqn_torch(net=_net(head=2))
    with pytest.raises(ValueError, match=r"net\[0\] weight"):
        env.dqn_torch(net=_net(D=15))
    with pytest.raises(ValueError, match=r"net\[1\] bias"):
        env.dqn_torch(net=[par[0], (par[1][0], _z(16, dtype=torch.float64)), par[2]])
    with pytest.raises(ValueError, match=r"net\[0\] weight"):
        env.dqn_torch(net=[(torch.zeros((16, 13)), par[0][1])] + par[1:])  # a CPU tensor
    with pytest.raises(ValueError, match=r"net\[0\] weight"):
        env.dqn_torch(net=[(_fake_cuda(torch.zeros((13, 16)).t()), par[0][1])] + par[1:])  # not contiguous
    env.discrete = False
    with pytest.raises(ValueError, match="continuous ids are not served"):
        env.dqn_torch(net=par)
    assert env._lib.names() == []


def test_the_calls_check_their_tensors_before_the_native_call():
    import torch
    env = _discrete_env()
    par = _net()
    h = env.dqn_torch(net=par)
    B, n, K = env.num_envs, 24, 4
    i32 = torch.int32
    obs_b, obs, action = _z(B, 13), _z(n, 13), _z(n, dtype=i32)
    out = dict(action=_z(B, dtype=i32), q=_z(B))
    a, q = env.dqn_act_torch(h, obs_b, seed=3, step=2 ** 33, epsilon=0.25, out=out)
    name, args = env._lib.calls[-1]
    assert a is out["action"] and q is out["q"] and name == "sg_dqn_act_device"
    assert args[3:6] == (3, 2 ** 33, 0.25) and args[6] is None and args[7].value == a.data_ptr() and args[8].value == q.data_ptr()
    eps = _z(B)
    assert env.dqn_act_torch(h, obs_b, epsilon=eps, out=dict(action=out["action"]))[1] is None
    args = env._lib.calls[-1][1]
    assert args[5] == 0.0 and args[6].value == eps.data_ptr() and args[8] is None
    for good in (0, 1, 0.0, 1.0, np.float32(0.5)):
        env.dqn_act_torch(h, obs_b, epsilon=good, out=out)
    qa, qt, qm, am = env.dqn_evaluate_raw_torch(h, obs, action, out=dict(q_all=_z(n, ACTIONS), q_taken=_z(n), q_max=_z(n), argmax=_z(n, dtype=i32)))
    name, args = env._lib.calls[-1]
    assert name == "sg_dqn_evaluate_device" and args[2] == n and args[4].value == action.data_ptr()
    assert [x.value for x in args[5:9]] == [qa.data_ptr(), qt.data_ptr(), qm.data_ptr(), am.data_ptr()]
    assert env.dqn_evaluate_raw_torch(h, obs, out=dict(argmax=am)) == (None, None, None, am)
    assert env._lib.calls[-1][1][4:8] == (None, None, None, None)
    roll = dict(obs=_z(K + 1, B, 13), action=_z(K, B, dtype=i32), reward=_z(K, B), done=_z(K, B, dtype=torch.uint8), trunc=_z(K, B, dtype=torch.uint8))
    env.rollout_dqn_torch(h, **roll, seed=5, first_step=7, epsilon=0.5)
    name, args = env._lib.calls[-1]
    assert name == "sg_rollout_dqn_device" and args[1] == K and args[3:6] == (5, 7, 0.5) and args[6] is None and args[9] is None and args[13] is None
    env.rollout_dqn_torch(h, **roll, q=_z(K, B), epsilon=eps)
    assert env._lib.calls[-1][1][9] is not None and env._lib.calls[-1][1][6].value == eps.data_ptr()
    env._lib.calls.clear()
    pol = env.policy_torch(**_params(head=ACTIONS, log_std=None))
    for call in (lambda x: env.dqn_act_torch(x, obs_b), lambda x: env.dqn_evaluate_raw_torch(x, obs), lambda x: env.dqn_evaluate_torch(x, obs),
                 lambda x: env.dqn_grad_torch(x, obs, g_all=_z(n, ACTIONS)), lambda x: env.rollout_dqn_torch(x, **roll)):
        for x in (pol, par, None):
            with pytest.raises(ValueError, match="handle dqn_torch returns"):
                call(x)
    with pytest.raises(ValueError, match="obs"):
        env.dqn_act_torch(h, obs)  # n rows, not num_envs
    with pytest.raises(ValueError, match=r"out\['action'\]"):
        env.dqn_act_torch(h, obs_b, out=dict(q=_z(B)))
    with pytest.raises(ValueError, match=r"out\['action'\]"):
        env.dqn_act_torch(h, obs_b, out=dict(action=_z(B)))  # float32 actions
    with pytest.raises(ValueError, match=r"out\['q'\]"):
        env.dqn_act_torch(h, obs_b, out=dict(action=_z(B, dtype=i32), q=_z(B + 1)))
    for bad in (_z(B + 1), _z(B, dtype=torch.float64), torch.zeros(B), _z(B, 1)):  # the wrong length, dtype, device, shape
        with pytest.raises(ValueError, match="epsilon"):
            env.dqn_act_torch(h, obs_b, epsilon=bad)
        with pytest.raises(ValueError, match="epsilon"):
            env.rollout_dqn_torch(h, **roll, epsilon=bad)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match="epsilon"):
            env.dqn_act_torch(h, obs_b, epsilon=bad)
        with pytest.raises(ValueError, match="epsilon"):
            env.rollout_dqn_torch(h, **roll, epsilon=bad)
    with pytest.raises(ValueError, match="obs"):
        env.dqn_evaluate_raw_torch(h, _z(n, 14))
    with pytest.raises(ValueError, match="obs"):
        env.dqn_evaluate_raw_torch(h, _z(0, 13))
    with pytest.raises(ValueError, match="obs"):
        env.dqn_evaluate_raw_torch(h, torch.zeros((n, 13)))
    with pytest.raises(ValueError, match="action"):
        env.dqn_evaluate_raw_torch(h, obs, _z(n))  # float32 actions
    with pytest.raises(ValueError, match="action"):
        env.dqn_evaluate_torch(h, obs, _z(n + 1, dtype=i32))
    with pytest.raises(ValueError, match="action"):
        env.dqn_evaluate_raw_torch(h, obs, out=dict(q_taken=_z(n)))
    with pytest.raises(ValueError, match="at least one"):
        env.dqn_evaluate_raw_torch(h, obs, action, out={})
    with pytest.raises(ValueError, match=r"out\['q_all'\]"):
        env.dqn_evaluate_raw_torch(h, obs, out=dict(q_all=_z(n, 5)))
    with pytest.raises(ValueError, match=r"out\['argmax'\]"):
        env.dqn_evaluate_raw_torch(h, obs, out=dict(argmax=_z(n)))
    with pytest.raises(ValueError, match="nothing to compute"):
        env.dqn_grad_torch(h, obs, action)
    with pytest.raises(ValueError, match="action"):
        env.dqn_grad_torch(h, obs, None, g_taken=_z(n))  # action missing with g_taken
    with pytest.raises(ValueError, match="g_taken"):
        env.dqn_grad_torch(h, obs, action, g_taken=_z(n, 1))
    with pytest.raises(ValueError, match="g_all"):
        env.dqn_grad_torch(h, obs, action, g_all=_z(n))
    with pytest.raises(ValueError, match="g_all"):
        env.dqn_grad_torch(h, obs, g_all=_z(n, ACTIONS, dtype=torch.float64))
    good = dict(net=[(_z(*w.shape), _z(*b.shape)) for w, b in par])
    with pytest.raises(ValueError, match=r"out\['net'\]: expected 3"):
        env.dqn_grad_torch(h, obs, g_all=_z(n, ACTIONS), out=dict(net=good["net"][:2]))
    with pytest.raises(ValueError, match=r"out\['net'\]\[2\] bias"):
        env.dqn_grad_torch(h, obs, g_all=_z(n, ACTIONS), out=dict(net=good["net"][:2] + [(_z(ACTIONS, 16), _z(2))]))
    with pytest.raises(ValueError, match="action"):
        env.rollout_dqn_torch(h, **{**roll, "action": _z(K, B, 2)})
    with pytest.raises(ValueError, match="action"):
        env.rollout_dqn_torch(h, **{**roll, "action": _z(K, B)})  # float32 actions
    with pytest.raises(ValueError, match="obs"):
        env.rollout_dqn_torch(h, **{**roll, "obs": _z(K, B, 13)})
    with pytest.raises(ValueError, match=r"^q:"):
        env.rollout_dqn_torch(h, **roll, q=_z(K + 1, B))
    with pytest.raises(ValueError, match="done"):
        env.rollout_dqn_torch(h, **{**roll, "done": _z(K, B)})
    assert env._lib.names() == []
    env.discrete = False  # a continuous id: every call is refused
    for call in (lambda: env.dqn_act_torch(h, obs_b), lambda: env.dqn_evaluate_raw_torch(h, obs), lambda: env.dqn_evaluate_torch(h, obs),
                 lambda: env.dqn_grad_torch(h, obs, g_all=_z(n, ACTIONS)), lambda: env.rollout_dqn_torch(h, **roll)):
        with pytest.raises(ValueError, match="continuous ids are not served"):
            call()
    assert env._lib.names() == []


def test_q_torch_points_a_discrete_id_to_the_dqn_head():
    env = _discrete_env()
    with pytest.raises(ValueError, match="discrete ids are not served.*dqn_torch"):
        env.q_torch(critics=[_net(D=15, head=1)])


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("dqn_torch", "dqn_act_torch", "rollout_dqn_torch", "dqn_evaluate_torch", "dqn_evaluate_raw_torch", "dqn_grad_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
