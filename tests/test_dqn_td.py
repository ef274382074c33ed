"""CPU tests of the fused DQN / Double DQN TD update (sg_dqn_td_grad_device / dqn_td_grad_torch / dqn_update_torch): the declarations,
the NumPy model (tests/dqn_td_model.py) against torch.autograd on float64 modules with the loss written in plain torch, the conditions
every case the GPU tests run must keep (the 1 % cap of the gradient tolerance, no TD error at the Huber kink, hardly any near-tie of the
online argmax), the bad-action rule, and the Python argument checks with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dqn_model import ACTIONS, flat, grad_tolerances
from dqn_td_model import GAP, GAP_SHARE, HUBER_MARGIN, ROWS, STATS, WIDTH_FAMILY, case, grad_case, grad_cases, reference, register_width_family, td
from dqn_td_model import width_cases
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_snapshot_device import _header_args

register_width_family()  # (before any test runs: tests/test_net_widths.py counts the engine's kernel templates against the families)

REL = 1e-10  # float64 model against float64 autograd: the figure of tests/test_dqn.py for the same comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    assert _header_args("sg_dqn_td_grad_device") == [
        "sg_env *env", "const sg_dqn *online", "const sg_dqn *target", "const sg_dqn_td_config *cfg", "const sg_dqn_td_batch *batch", "int64_t n",
        "const sg_dqn_grads *grads", "float *stats_out", "const sg_dqn_td_rows *row_out", "void *workspace", "size_t workspace_bytes",
        "void *hip_stream"]
    assert _header_args("sg_dqn_td_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_dqn *online", "int64_t n"]
    assert _header_args("sg_dqn_td_config_init", "void") == ["sg_dqn_td_config *cfg"]
    vp, P = C.c_void_p, C.POINTER
    assert _native.SYMBOLS["sg_dqn_td_grad_device"] == (
        C.c_int, [vp, P(_native.SgDqn), P(_native.SgDqn), P(_native.SgDqnTdConfig), P(_native.SgDqnTdBatch), C.c_int64, P(_native.SgDqnGrads), vp,
                  P(_native.SgDqnTdRows), vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_dqn_td_grad_workspace_bytes"] == (C.c_size_t, [vp, P(_native.SgDqn), C.c_int64])
    assert _native.SYMBOLS["sg_dqn_td_config_init"] == (None, [P(_native.SgDqnTdConfig)])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls, size in (("sg_dqn_td_config", _native.SgDqnTdConfig, 16), ("sg_dqn_td_batch", _native.SgDqnTdBatch, 56),
                            ("sg_dqn_td_rows", _native.SgDqnTdRows, 40)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [d.split()[-1].lstrip("*") for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_] and C.sizeof(cls) == size, name
    assert [f for f, _ in _native.SgDqnTdRows._fields_] == list(ROWS)
    assert _native.SgDqnTdConfig.struct_size.offset == 0 and _native.SgDqnTdConfig.reserved.offset == 12
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_dqn_td.inc" in build.HEADERS and build.HEADERS.index("sg_dqn_td.inc") == build.HEADERS.index("sg_dqn.inc") + 1
    assert src.index('#include "sg_dqn.inc"') < src.index('#include "sg_dqn_td.inc"') < src.index('#include "sg_population.inc"')
    assert re.search(r"kNetsDqnTd = 256\b", src)
    inc = open(os.path.join(build.CSRC, "sg_dqn_td.inc")).read()
    code = re.sub(r"//.*", "", inc)
    for kernel in ("dqn_td_target_kernel", "dqn_td_grad_kernel", "dqn_td_reduce_kernel"):
        assert re.search(r"void %s\(" % kernel, code), kernel
    assert "policy_grad_net<NT>" in code and "policy_grad_reduce_element(" in code and code.count("policy_net<NT>(") == 2
    assert "dqn_argmax(" in code and "dqn_select(" in code and "__fadd_rn(r, __fmul_rn(" in code and "atomic" not in code.lower()
    assert SpaceGymVectorEnv.dqn_td_stats_names == STATS and len(STATS) == 8
    assert {"dqn_td_grad_torch", "dqn_update_torch"} <= set(NET_METHODS)
    assert all(callable(getattr(SpaceGymVectorEnv, n)) for n in ("dqn_td_grad_torch", "dqn_update_torch"))


def test_the_two_kernel_templates_are_a_width_family_with_a_test_at_every_class():
    """what tests/test_net_widths.py asks of a net kernel, for the two added here: four instantiations in the compiler's report, named
    as a family in test_gpu_net_widths.FAMILY_KERNELS, and a GPU test that runs them at net_widths' table -- every class NT = 1 .. 4
    and each class's widest net, 32 NT wide with three hidden layers on the 4P id"""
    import engine_asm
    import net_widths
    import test_gpu_dqn_td
    import test_gpu_net_widths
    name, kernels = WIDTH_FAMILY
    assert test_gpu_net_widths.FAMILY_KERNELS[name] == kernels
    assert sum(k in kernels for ks in test_gpu_net_widths.FAMILY_KERNELS.values() for k in ks) == 2
    classes = {k: [] for k in kernels}
    for row in engine_asm.resource_rows():
        m = re.match(r"_Z\d+(\w+_kernel)ILi(\d+)EE", row["name"])
        if m and m.group(1) in classes:
            classes[m.group(1)].append(int(m.group(2)))
            assert row["ScratchSize [bytes/lane]"] == "0" and row["VGPRs Spill"] == "0" and row["Dynamic Stack"] == "False", row
    assert all(sorted(v) == [1, 2, 3, 4] for v in classes.values()), classes
    nets = [(hidden, n_hidden) for hidden, n_hidden, _ in width_cases()]
    assert set(net_widths.WIDTH_NETS) <= set(nets) and {net_widths.tile_class(h) for h, _ in nets} == {1, 2, 3, 4}
    assert all((32 * c, 3) in nets for c in (1, 2, 3, 4))
    assert test_gpu_dqn_td.test_both_kernels_at_every_width_class.pytestmark[0].args[1] == width_cases()


def _torch_td(c, activation, double_q, huber_delta, weighted):
    """the update in plain torch on float64 modules: (statistics by name, gradients by name, per-row target and td)"""
    import torch
    b = c["batch"]
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    online, target = _torch_net(c["online"], activation), _torch_net(c["target"], activation)
    n = b["obs"].shape[0]
    with torch.no_grad():
        qt = target(t(b["next_obs"]))
        q_next = qt.gather(1, online(t(b["next_obs"])).argmax(1)[:, None])[:, 0] if double_q else qt.max(1).values
        y = torch.where(torch.from_numpy(b["terminated"] != 0), t(b["reward"]), t(b["reward"]) + t(b["discount"]) * q_next)
    q_taken = online(t(b["obs"])).gather(1, torch.from_numpy(b["action"].astype(np.int64))[:, None])[:, 0]
    w = t(c["weight"]) if weighted else torch.ones(n, dtype=torch.float64)
    if np.isinf(huber_delta):
        per_row = 0.5 * (q_taken - y) ** 2
    else:
        per_row = torch.nn.functional.huber_loss(q_taken, y, reduction="none", delta=huber_delta)
    loss = (w * per_row).sum() / n
    loss.backward()
    lin = [m for m in online if isinstance(m, torch.nn.Linear)]
    grads = flat(dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin]))
    err = (q_taken - y).detach()
    stats = dict(loss=loss.item(), td_abs_mean=err.abs().mean().item(), td_abs_max=err.abs().max().item(), q_mean=q_taken.mean().item(),
                 target_mean=y.mean().item(), clip_fraction=(err.abs() > huber_delta).double().mean().item(), weight_mean=w.mean().item(), bad_rows=0.0)
    return stats, grads, y.numpy(), err.numpy()


VARIANTS = [(dq, delta, weighted) for dq in (True, False) for delta in (1.0, float("inf")) for weighted in (True, False)]


@pytest.mark.parametrize("double_q,huber_delta,weighted", VARIANTS)
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_model_equals_torch_autograd_in_float64(activation, double_q, huber_delta, weighted):
    """the per-row target and td, the eight statistics and every gradient, for Double and plain, Huber and the squared loss, with and
    without weights; a terminated row's target is its reward"""
    c = case(13, 96, 33, 2, seed=4)
    b = c["batch"]
    b["terminated"][1] = 1
    got = reference(c, activation, double_q, huber_delta, weighted, np.float64)
    stats, grads, y, err = _torch_td(c, activation, double_q, huber_delta, weighted)
    what = (activation, double_q, huber_delta, weighted)
    assert rel(got["rows"]["target"], y) <= REL and rel(got["rows"]["td_error"], err) <= REL, what
    for k, name in enumerate(STATS):
        assert abs(float(got["stats"][k]) - stats[name]) <= REL * abs(stats[name]), (what, name, float(got["stats"][k]), stats[name])
    mine = flat(got)
    assert set(mine) == set(grads) and len(mine) == 6
    for k in grads:
        assert mine[k].shape == grads[k].shape and np.abs(grads[k]).max() > 0 and rel(mine[k], grads[k]) <= REL, (what, k, rel(mine[k], grads[k]))
    assert got["stats"].dtype == np.float64 and got["stats"][7] == 0
    if np.isfinite(huber_delta):  # both branches of the loss are taken by at least a tenth of the rows
        assert 0.1 <= got["clipped"].mean() <= 0.9, got["clipped"].mean()
    else:
        assert not got["clipped"].any()
    assert 0 < b["terminated"].sum() < 96 and np.array_equal(got["rows"]["target"][b["terminated"] != 0], b["reward"][b["terminated"] != 0].astype(np.float64))


@pytest.mark.parametrize("double_q", [True, False])
def test_a_terminated_row_with_an_infinite_q_next_has_its_reward_as_target(double_q):
    """the target is a where, not a product with (1 - terminated): 0 x inf would be NaN.  The target net's head bias of action 0 is
    +inf, so q_next is inf on every row whose a* is 0 (plain DQN: on every row); the terminated ones keep y = reward and finite
    gradients, in the model and in torch alike"""
    c = case(13, 64, 16, 1, seed=9)
    b = c["batch"]
    c["target"][-1][1][0] = np.float32(np.inf)
    if double_q:
        c["online"][-1][1][0] = np.float32(50.0)  # the online argmax of next_obs is action 0 everywhere
    b["terminated"][:] = 1
    got = reference(c, "relu", double_q, 1.0, True, np.float64)
    assert np.isinf(got["rows"]["q_next"]).all() and np.array_equal(got["rows"]["target"], b["reward"].astype(np.float64))
    stats, grads, y, err = _torch_td(c, "relu", double_q, 1.0, True)
    assert np.array_equal(y, got["rows"]["target"]) and np.isfinite(err).all()
    for k, v in flat(got).items():
        assert np.isfinite(v).all() and rel(v, grads[k]) <= REL, k
    g32 = reference(c, "relu", double_q, 1.0, True, np.float32)
    assert np.isfinite(g32["stats"]).all() and all(np.isfinite(v).all() for v in flat(g32).values())
    b["terminated"][::2] = 0  # and a live row with an infinite q_next has an infinite target: nothing hides it
    assert np.isinf(reference(c, "relu", double_q, 1.0, True, np.float64)["rows"]["target"][::2]).all()


def test_per_row_derivative_is_the_stated_one():
    """g of the model against autograd of the torch loss by q_taken, with weights: clipped rows carry +-delta w / n"""
    import torch
    c = case(13, 96, 33, 2, seed=4)
    got = reference(c, "relu", True, 1.0, True, np.float64)
    q = torch.from_numpy(got["rows"]["q_taken"]).requires_grad_()
    w = torch.from_numpy(c["weight"].astype(np.float64))
    (w * torch.nn.functional.huber_loss(q, torch.from_numpy(got["rows"]["target"]), reduction="none", delta=1.0)).mean().backward()
    assert np.allclose(got["rows"]["g"], q.grad.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(np.abs(got["rows"]["g"][got["clipped"]]), c["weight"][got["clipped"]].astype(np.float64) / 96, rtol=1e-12, atol=0)


def test_an_action_outside_the_six_changes_nothing_but_the_count():
    c = case(13, 60, 33, 2, seed=3)
    where = [0, 7, 31, 59]
    results = []
    for bad in ((7, -1, 6, 2 ** 31 - 1), (-1, 7, -2 ** 31, 100)):
        b = dict(c["batch"], action=c["batch"]["action"].copy())
        b["action"][where] = bad
        results.append(td(c["online"], c["target"], b, weight=c["weight"]))
        r = results[-1]
        assert r["stats"][7] == 4 and not r["rows"]["g"][where].any() and not r["rows"]["td_error"][where].any() and r["rows"]["g"].any()
    a, b2 = results
    assert a["stats"].tobytes() == b2["stats"].tobytes()  # which way an action is outside, and how far, is all the same
    for k, v in flat(a).items():
        assert v.tobytes() == flat(b2)[k].tobytes(), k
    # the same rows without the bad ones, summed by hand: they add nothing, the divisor stays n
    keep = np.delete(np.arange(60), where)
    alone = td(c["online"], c["target"], {k: v[keep] for k, v in c["batch"].items()}, weight=c["weight"][keep])
    for k, v in flat(alone).items():
        assert np.allclose(flat(a)[k] * 60, v * 56, rtol=1e-12, atol=1e-300), k
    for s in (0, 1, 3, 4, 5, 6):
        assert np.isclose(a["stats"][s] * 60, alone["stats"][s] * 56, rtol=1e-12, atol=0), STATS[s]
    assert a["stats"][2] == alone["stats"][2] and alone["stats"][7] == 0


def test_float32_mode_is_float32_and_close():
    c = case(13, 300, 33, 2, seed=8)
    m64 = reference(c, "tanh", True, 1.0, True, np.float64)
    m32 = reference(c, "tanh", True, 1.0, True, np.float32, a_star=m64["a_star"])
    g64, g32 = flat(m64), flat(m32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
    assert m32["stats"].dtype == np.float32 and all(m32["rows"][k].dtype == np.float32 for k in ROWS)
    for k in range(8):
        assert abs(float(m32["stats"][k]) - m64["stats"][k]) <= 1e-4 * (1 + abs(m64["stats"][k])), STATS[k]


@pytest.mark.parametrize("obs_dim,n,hidden,n_hidden,activation,double_q,huber_delta,weighted", grad_cases())
def test_every_gpu_case_keeps_the_conditions_its_tolerances_rest_on(obs_dim, n, hidden, n_hidden, activation, double_q, huber_delta, weighted):
    """for the very cases (the same generator, the same seed) tests/test_gpu_dqn_td.py runs: 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|)
    <= 1 % of max|G64| per tensor; no row's |td| within 1e-4 of huber_delta (float32 decides the branch as float64 does); at most 1 %
    of the rows with the two largest online Q values of next_obs closer than 1e-5.  A GPU failure cannot be the inputs' fault"""
    c = grad_case(obs_dim, n, hidden, n_hidden)
    m64 = reference(c, activation, double_q, huber_delta, weighted, np.float64)
    m32 = reference(c, activation, double_q, huber_delta, weighted, np.float32, a_star=m64["a_star"])
    g64, g32 = flat(m64), flat(m32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        top = float(np.abs(g64[k]).max())
        assert top > 0 and tol[k] <= 0.01 * top, (k, tol[k], top)
    if np.isfinite(huber_delta):
        assert np.abs(np.abs(m64["rows"]["td_error"]) - huber_delta).min() >= HUBER_MARGIN
        assert np.array_equal(m32["clipped"], m64["clipped"])
    if double_q:
        assert (m64["gap"] < GAP).mean() <= GAP_SHARE, (m64["gap"] < GAP).mean()
    assert m64["good"].all() and m64["stats"][7] == 0


def test_the_cases_cover_every_option_at_every_row_count():
    from dqn_model import BIG_N, GRAD_NS, NETS
    from dqn_td_model import CLASS3_NET
    cases = grad_cases()
    assert {(c[2], c[3]) for c in cases} == set(NETS) | {CLASS3_NET, (128, 1)} and {c[1] for c in cases} == set(GRAD_NS) | {BIG_N}
    assert {c[0] for c in cases} == {10, 15}
    for n in GRAD_NS:
        mine = [c for c in cases if c[1] == n]
        assert {c[5] for c in mine} == {True, False} and {c[7] for c in mine} == {True, False} and {c[4] for c in mine} == {"tanh", "relu"}
        assert {np.isinf(c[6]) for c in mine} == {True, False}, n
    assert [c for c in cases if c[1] == BIG_N] == [(15, BIG_N, 128, 1, "tanh", True, 1.0, True)] and BIG_N > 256 * 64


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _net(D=13, hidden=16, n_hidden=2):
    return _params(D=D, hidden=hidden, n_hidden=n_hidden, head=ACTIONS)["actor"]


def _discrete_env():
    env = _stub_env()
    env.discrete = True
    return env


def _batch(n=24, D=13):
    import torch
    return dict(obs=_z(n, D), action=_z(n, dtype=torch.int32), reward=_z(n), next_obs=_z(n, D), terminated=_z(n, dtype=torch.uint8), discount=_z(n),
                truncated=_z(n, dtype=torch.uint8), steps=_z(n, dtype=torch.uint8), index=_z(n, dtype=torch.int64), cell=_z(n, dtype=torch.int64),
                weight=_z(n))


class _Sized:
    """the stub library with the workspace query answering 64 bytes"""

    def __init__(self, lib):
        self._lib, self.calls = lib, lib.calls

    def __getattr__(self, name):
        if name == "sg_dqn_td_grad_workspace_bytes":
            return lambda *a: 64
        return getattr(self._lib, name)

    def names(self):
        return self._lib.names()


def test_dqn_td_grad_torch_checks_its_arguments_before_the_native_call():
    import torch
    env = _discrete_env()
    online, target = env.dqn_torch(net=_net()), env.dqn_torch(net=_net())
    batch, n = _batch(), 24
    refused = [
        ("handle dqn_torch returns", lambda: env.dqn_td_grad_torch(_net(), target, batch)),
        ("handle dqn_torch returns", lambda: env.dqn_td_grad_torch(online, None, batch)),
        ("target: expected a net of the online net's architecture", lambda: env.dqn_td_grad_torch(online, env.dqn_torch(net=_net(hidden=17)), batch)),
        ("target: expected a net of the online net's architecture", lambda: env.dqn_td_grad_torch(online, env.dqn_torch(net=_net(n_hidden=1)), batch)),
        ("target: expected a net of the online net's architecture", lambda: env.dqn_td_grad_torch(online, env.dqn_torch(net=_net(), activation="tanh"), batch)),
        ("batch: expected the dict", lambda: env.dqn_td_grad_torch(online, target, [batch["obs"]])),
        (r"batch\['obs'\]", lambda: env.dqn_td_grad_torch(online, target, dict(batch, obs=_z(n, 14)))),
        (r"batch\['obs'\]", lambda: env.dqn_td_grad_torch(online, target, dict(batch, obs=_z(0, 13)))),
        (r"batch\['action'\]", lambda: env.dqn_td_grad_torch(online, target, dict(batch, action=_z(n)))),
        (r"batch\['reward'\]", lambda: env.dqn_td_grad_torch(online, target, dict(batch, reward=_z(n + 1)))),
        (r"batch\['next_obs'\]: missing", lambda: env.dqn_td_grad_torch(online, target, {k: v for k, v in batch.items() if k != "next_obs"})),
        (r"batch\['next_obs'\]", lambda: env.dqn_td_grad_torch(online, target, dict(batch, next_obs=_z(n, 12)))),
        (r"batch\['terminated'\]", lambda: env.dqn_td_grad_torch(online, target, dict(batch, terminated=_z(n)))),
        (r"batch\['discount'\]: missing", lambda: env.dqn_td_grad_torch(online, target, dict(batch, discount=None))),
        ("weight", lambda: env.dqn_td_grad_torch(online, target, batch, weight=_z(n, 1))),
        ("weight", lambda: env.dqn_td_grad_torch(online, target, batch, weight=torch.zeros(n))),
        ("huber_delta", lambda: env.dqn_td_grad_torch(online, target, batch, huber_delta=0.0)),
        ("huber_delta", lambda: env.dqn_td_grad_torch(online, target, batch, huber_delta=-1.0)),
        ("huber_delta", lambda: env.dqn_td_grad_torch(online, target, batch, huber_delta=float("nan"))),
        ("huber_delta", lambda: env.dqn_td_grad_torch(online, target, batch, huber_delta=None)),
        (r"rows\['g'\]", lambda: env.dqn_td_grad_torch(online, target, batch, rows=dict(g=_z(n + 1)))),
        (r"rows\['ratio'\]", lambda: env.dqn_td_grad_torch(online, target, batch, rows=dict(ratio=_z(n)))),
        ("stats", lambda: env.dqn_td_grad_torch(online, target, batch, stats=_z(7))),
        (r"out\['net'\]: expected 3", lambda: env.dqn_td_grad_torch(online, target, batch, out=dict(net=[(_z(16, 13), _z(16))]))),
    ]
    for match, call in refused:
        with pytest.raises(ValueError, match=match):
            call()
    assert env._lib.names() == []
    env.discrete = False
    with pytest.raises(ValueError, match="continuous ids are not served"):
        env.dqn_td_grad_torch(online, target, batch)
    assert env._lib.names() == []


def test_the_call_passes_the_columns_and_the_configuration():
    import torch
    from space_gym_amd import _native
    env = _discrete_env()
    online, target = env.dqn_torch(net=_net()), env.dqn_torch(net=_net())
    batch, n = _batch(), 24
    online.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    lib = env._lib
    env._lib = _Sized(lib)
    rows = dict(td_error=_z(n), q_next=_z(n), g=None)
    grads, stats = env.dqn_td_grad_torch(online, target, batch, double_q=False, huber_delta=float("inf"), weight=batch["weight"], rows=rows)
    name, args = lib.calls[-1]
    assert name == "sg_dqn_td_grad_device" and args[5] == n and args[10] == 64 and args[9].value == online.workspace.data_ptr()
    assert args[1]._obj is online.struct and args[2]._obj is target.struct
    cfg, b, g, r = args[3]._obj, args[4]._obj, args[6]._obj, args[8]._obj
    assert isinstance(cfg, _native.SgDqnTdConfig) and cfg.double_q == 0 and cfg.huber_delta == float("inf") and cfg.reserved == 0
    assert (b.obs, b.action, b.reward, b.next_obs, b.terminated, b.discount, b.weight) == tuple(
        batch[k].data_ptr() for k in ("obs", "action", "reward", "next_obs", "terminated", "discount", "weight"))
    assert (r.td_error, r.q_taken, r.target, r.q_next, r.g) == (rows["td_error"].data_ptr(), None, None, rows["q_next"].data_ptr(), None)
    assert stats.shape == (8,) and args[7].value == stats.data_ptr() and len(grads["net"]) == 3
    assert all(g.net.weight[l] == grads["net"][l][0].data_ptr() and g.net.bias[l] == grads["net"][l][1].data_ptr() for l in range(3))
    assert g.struct_size == C.sizeof(_native.SgDqnGrads)
    # the defaults: Double DQN, delta 1, no weights, no rows
    env.dqn_td_grad_torch(online, target, batch, out=grads, stats=stats)
    args = lib.calls[-1][1]
    assert args[3]._obj.double_q == 1 and args[3]._obj.huber_delta == 1.0 and args[4]._obj.weight is None and args[8] is None
    # the gradient dict is what adam_step_torch and _flat_grads take
    from space_gym_amd.vector_env import _flat_grads
    assert [t.data_ptr() for t in _flat_grads(online, grads)] == [t.data_ptr() for pair in grads["net"] for t in pair]


def test_dqn_update_torch_composes_the_existing_calls(monkeypatch):
    """the native calls in order, and torch._foreach_lerp_ on (the target's tensors, the online ones, tau); the stand-in applies it to
    the plain tensors beneath the fake CUDA ones, which the foreach kernels do not take"""
    import torch
    real, plain = torch._foreach_lerp_, lambda ts: [t.as_subclass(torch.Tensor) for t in ts]
    lerps = []

    def lerp(a, b, w):
        lerps.append((list(a), list(b), w))
        real(plain(a), plain(b), plain(w) if isinstance(w, list) else w)
    monkeypatch.setattr(torch, "_foreach_lerp_", lerp)
    from space_gym_amd.vector_env import AdamState
    env = _discrete_env()
    par_o, par_t = _net(), _net()
    for (w, b), (w2, b2) in zip(par_o, par_t):
        w.fill_(1.0); b.fill_(1.0)
    online, target = env.dqn_torch(net=par_o), env.dqn_torch(net=par_t)
    batch, n = _batch(), 24
    online.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    zeros = lambda: tuple(_fake_cuda(torch.zeros_like(t)) for t in online.tensors)
    opt = AdamState(online, 1, _z(1, 8), _z(1, 8, dtype=torch.float64), zeros(), zeros())
    lib = env._lib
    env._lib = _Sized(lib)
    stats, rows, grads = env.dqn_update_torch(online, target, opt, batch, weight=batch["weight"], tau=0.25)
    assert lib.names() == ["sg_dqn_td_config_init", "sg_dqn_td_grad_device", "sg_adam_step_device"] and rows == {}
    assert all(float(t.min()) == float(t.max()) == 0.25 for t in target.tensors) and all(float(t.min()) == 1.0 for t in online.tensors)
    assert len(lerps) == 1 and lerps[0][2] == 0.25 and all(a is b for a, b in zip(lerps[0][0], target.tensors))
    assert all(a is b for a, b in zip(lerps[0][1], online.tensors))
    one = _z()
    one.fill_(1.0)
    env.dqn_update_torch(online, target, opt, batch, grads=grads, stats=stats, tau=one)  # a device scalar of 1: the hard sync
    assert all(float(t.min()) == float(t.max()) == 1.0 for t in target.tensors) and all(w is one for w in lerps[1][2])
    env.dqn_update_torch(online, target, opt, batch, grads=grads, stats=stats)  # no tau: the target is the caller's to move
    assert len(lerps) == 2
    assert lib.calls[-2][1][7].value == stats.data_ptr()
    with pytest.raises(ValueError, match="opt: expected the AdamState"):
        env.dqn_update_torch(online, target, AdamState(target, 1, opt.hyper, opt.state, zeros(), zeros()), batch)
    for bad in (-0.1, 1.5, float("nan"), "soft", _z(1), _z(dtype=torch.float64)):
        with pytest.raises(ValueError, match="tau"):
            env.dqn_update_torch(online, target, opt, batch, tau=bad)
    with pytest.raises(ValueError, match=r"batch\['cell'\]: missing"):
        env.dqn_update_torch(online, target, opt, {k: v for k, v in batch.items() if k != "cell"}, prio=object())


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("dqn_td_grad_torch", "dqn_update_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
