"""CPU tests of the fused TD critic update of SAC / TD3 / DDPG (sg_q_td_grad_device / q_td_grad_torch / q_update_torch): the
declarations, the NumPy model (tests/q_td_model.py) against torch.autograd on float64 modules with the loss written in plain torch, the
conditions every case the GPU tests run must keep (the 1 % cap of the gradient tolerance, no TD error at the Huber kink, every branch
of the loss and of the two clamps taken by a tenth of the rows), and the Python argument checks with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from q_model import grad_tolerances
from q_td_model import BIG_N, BRANCH_SHARE, CLASS3_NET, FORMS, GRAD_NS, HUBER_MARGIN, NETS, ROWS, STATS, WIDTH_FAMILY, case, flat, grad_case
from q_td_model import grad_cases, options, reference, regime_case, regime_reference, register_width_family, td, width_cases
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _torch_net
from test_q import _q_params
from test_snapshot_device import _header_args

register_width_family()  # (before any test runs: tests/test_net_widths.py counts the engine's kernel templates against the families)

REL = 1e-10  # float64 model against float64 autograd: the figure of tests/test_q.py for the same comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    assert _header_args("sg_q_td_grad_device") == [
        "sg_env *env", "const sg_qnet *online", "const sg_qnet *target", "const sg_q_td_config *cfg", "const sg_q_td_batch *batch", "int64_t n",
        "const sg_qnet_grads *grads", "float *stats_out", "const sg_q_td_rows *row_out", "void *workspace", "size_t workspace_bytes",
        "void *hip_stream"]
    assert _header_args("sg_q_td_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_qnet *online", "int64_t n"]
    assert _header_args("sg_q_td_config_init", "void") == ["sg_q_td_config *cfg"]
    vp, P = C.c_void_p, C.POINTER
    assert _native.SYMBOLS["sg_q_td_grad_device"] == (
        C.c_int, [vp, P(_native.SgQnet), P(_native.SgQnet), P(_native.SgQTdConfig), P(_native.SgQTdBatch), C.c_int64, P(_native.SgQnetGrads), vp,
                  P(_native.SgQTdRows), vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_q_td_grad_workspace_bytes"] == (C.c_size_t, [vp, P(_native.SgQnet), C.c_int64])
    assert _native.SYMBOLS["sg_q_td_config_init"] == (None, [P(_native.SgQTdConfig)])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls, size in (("sg_q_td_config", _native.SgQTdConfig, 32), ("sg_q_td_batch", _native.SgQTdBatch, 88), ("sg_q_td_rows", _native.SgQTdRows, 72)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_] and C.sizeof(cls) == size, name
    assert [f for f, _ in _native.SgQTdRows._fields_] == list(ROWS)
    cfg = _native.SgQTdConfig
    assert [(f, getattr(cfg, f).offset) for f, _ in cfg._fields_] == [("struct_size", 0), ("huber_delta", 4), ("alpha", 8), ("noise_std", 12),
                                                                      ("noise_clip", 16), ("action_clip", 20), ("reserved", 24)]
    assert [f for f, _ in _native.SgQTdBatch._fields_] == ["obs", "action", "reward", "next_obs", "terminated", "discount", "next_action", "weight",
                                                           "next_logp", "alpha_dev", "noise"]
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_q_td.inc" in build.HEADERS and build.HEADERS.index("sg_q_td.inc") == build.HEADERS.index("sg_squashed.inc") + 1
    assert src.index('#include "sg_squashed.inc"') < src.index('#include "sg_q_td.inc"') < src.index('#include "sg_dqn.inc"')
    assert re.search(r"kNetsQTd = 512\b", src) and "case kNetsQTd:" in src
    assert "raise_lds_limit(kQTdTargetKernel, fwd(Q))" in src and "raise_lds_limit(kQTdGradKernel, bwd(Q))" in src
    inc = open(os.path.join(build.CSRC, "sg_q_td.inc")).read()
    code = re.sub(r"//.*", "", inc)
    for kernel in ("q_td_target_kernel", "q_td_grad_kernel", "q_td_reduce_kernel"):
        assert re.search(r"void %s\(" % kernel, code), kernel
    assert code.count("policy_grad_net<NT>(") == 1 and "policy_grad_reduce_element(" in code and code.count("policy_net<NT>(") == 2
    assert "__fadd_rn(r, __fmul_rn(" in code and "__fsub_rn(qn, __fmul_rn(alpha" in code and "__fadd_rn(a[d], ed)" in code
    assert "__fmul_rn(q.noise_std" in code and "atomic" not in inc.lower()
    assert SpaceGymVectorEnv.q_td_stats_names == STATS and len(STATS) == 9
    assert {"q_td_grad_torch", "q_update_torch"} <= set(NET_METHODS)
    assert all(callable(getattr(SpaceGymVectorEnv, n)) for n in ("q_td_grad_torch", "q_update_torch"))


def test_the_two_kernel_templates_are_a_width_family_with_a_test_at_every_class():
    """what tests/test_net_widths.py asks of a net kernel, for the two added here: four instantiations in the compiler's report with no
    scratch, no spill and no dynamic stack (the reduction kernel too), named as a family in test_gpu_net_widths.FAMILY_KERNELS, and a
    GPU test that runs them at net_widths' table -- every class NT = 1 .. 4 and each class's widest net"""
    import engine_asm
    import net_widths
    import test_gpu_net_widths
    import test_gpu_q_td
    name, kernels = WIDTH_FAMILY
    assert test_gpu_net_widths.FAMILY_KERNELS[name] == kernels
    assert sum(k in kernels for ks in test_gpu_net_widths.FAMILY_KERNELS.values() for k in ks) == 2
    classes, clean = {k: [] for k in kernels}, 0
    for row in engine_asm.resource_rows():
        m = re.match(r"_Z\d+(\w+_kernel)ILi(\d+)EE", row["name"])
        mine = m and m.group(1) in classes
        if mine:
            classes[m.group(1)].append(int(m.group(2)))
        if mine or "q_td_reduce_kernel" in row["name"]:
            assert row["ScratchSize [bytes/lane]"] == "0" and row["VGPRs Spill"] == "0" and row["Dynamic Stack"] == "False", row
            clean += 1
    assert all(sorted(v) == [1, 2, 3, 4] for v in classes.values()) and clean == 9, (classes, clean)
    nets = [(hidden, n_hidden) for hidden, n_hidden, _ in width_cases()]
    assert set(net_widths.WIDTH_NETS) <= set(nets) and {net_widths.tile_class(h) for h, _ in nets} == {1, 2, 3, 4}
    assert all((32 * c, 3) in nets for c in (1, 2, 3, 4))
    assert test_gpu_q_td.test_both_kernels_at_every_width_class.pytestmark[0].args[1] == width_cases()


def _torch_td(c, activation, form, huber_delta, weighted):
    """the update in plain torch on float64 modules: (statistics by name, gradients by name, per-row y, [td_c], [q_c])"""
    import torch
    b, kw = c["batch"], options(c, form, huber_delta, weighted)
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    f32 = lambda v: float(np.float32(v))  # the scalars as the engine holds them
    online, target = [_torch_net(net, activation) for net in c["online"]], [_torch_net(net, activation) for net in c["target"]]
    n = b["obs"].shape[0]
    with torch.no_grad():
        a2 = t(kw["next_action"])
        if "noise" in kw:
            e = torch.clamp(f32(kw["noise_std"]) * t(kw["noise"]), -f32(kw["noise_clip"]), f32(kw["noise_clip"]))
            a2 = torch.clamp(a2 + e, -f32(kw["action_clip"]), f32(kw["action_clip"]))
        x2 = torch.cat([t(b["next_obs"]), a2], 1)
        qt = [net(x2)[:, 0] for net in target]
        q_next = qt[0] if len(qt) == 1 else torch.minimum(qt[0], qt[1])
        if "next_logp" in kw:
            q_next = q_next - f32(kw["alpha"]) * t(kw["next_logp"])
        y = torch.where(torch.from_numpy(b["terminated"] != 0), t(b["reward"]), t(b["reward"]) + t(b["discount"]) * q_next)
    x = torch.cat([t(b["obs"]), t(b["action"])], 1)
    qs = [net(x)[:, 0] for net in online]
    w = t(c["weight"]) if weighted else torch.ones(n, dtype=torch.float64)
    per_row = lambda q: 0.5 * (q - y) ** 2 if np.isinf(huber_delta) else torch.nn.functional.huber_loss(q, y, reduction="none", delta=huber_delta)
    loss = sum((w * per_row(q)).sum() / n for q in qs)
    loss.backward()
    grads = {}
    for k, net in enumerate(online):
        for l, m in enumerate(mod for mod in net if isinstance(mod, torch.nn.Linear)):
            grads[f"critic{k}.{l}.weight"], grads[f"critic{k}.{l}.bias"] = m.weight.grad.numpy(), m.bias.grad.numpy()
    errs = [(q - y).detach() for q in qs]
    two = len(qs) == 2
    stats = dict(loss=loss.item(), td1_abs_mean=errs[0].abs().mean().item(), td2_abs_mean=errs[1].abs().mean().item() if two else 0.0,
                 td_abs_max=max(e.abs().max().item() for e in errs), q1_mean=qs[0].mean().item(), q2_mean=qs[1].mean().item() if two else 0.0,
                 target_mean=y.mean().item(), clip_fraction=sum((e.abs() > huber_delta).double().sum().item() for e in errs) / (len(qs) * n),
                 weight_mean=w.mean().item())
    return stats, grads, y.numpy(), [e.numpy() for e in errs], [q.detach().numpy() for q in qs]


VARIANTS = [(form, delta, weighted) for form in FORMS for delta in (1.0, float("inf")) for weighted in (True, False)]


@pytest.mark.parametrize("form,huber_delta,weighted", VARIANTS)
@pytest.mark.parametrize("n_critics", [1, 2])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_model_equals_torch_autograd_in_float64(activation, n_critics, form, huber_delta, weighted):
    """the per-row target and td, the nine statistics and every gradient, for one and two critics, the SAC form (logp, alpha), the TD3
    form (noise, clips) and the plain one, Huber and the squared loss, with and without weights; a terminated row's target is its
    reward"""
    c = case(13, 96, 33, 2, n_critics, seed=4)
    b = c["batch"]
    b["terminated"][1] = 1
    got = reference(c, activation, form, huber_delta, weighted, np.float64)
    stats, grads, y, errs, qs = _torch_td(c, activation, form, huber_delta, weighted)
    what = (activation, n_critics, form, huber_delta, weighted)
    assert rel(got["rows"]["target"], y) <= REL, what
    for k in range(n_critics):
        assert rel(got["rows"]["td%d" % (k + 1)], errs[k]) <= REL and rel(got["rows"]["q%d" % (k + 1)], qs[k]) <= REL, what
    for k, name in enumerate(STATS):
        assert abs(float(got["stats"][k]) - stats[name]) <= REL * abs(stats[name]), (what, name, float(got["stats"][k]), stats[name])
    mine = flat(got)
    assert set(mine) == set(grads) and len(mine) == 6 * n_critics
    for k in grads:
        assert mine[k].shape == grads[k].shape and np.abs(grads[k]).max() > 0 and rel(mine[k], grads[k]) <= REL, (what, k, rel(mine[k], grads[k]))
    assert got["stats"].dtype == np.float64
    if n_critics == 1:
        assert got["stats"][2] == 0 and got["stats"][5] == 0 and all(got["rows"][k] is None for k in ("td2", "q2", "g2"))
        assert np.array_equal(got["rows"]["td_abs"], np.abs(got["rows"]["td1"]))
    else:
        assert np.allclose(got["rows"]["td_abs"], 0.5 * (np.abs(errs[0]) + np.abs(errs[1])), rtol=1e-12, atol=0)
    for cl in got["clipped"]:  # both branches of the loss are taken by at least a tenth of the rows
        assert (BRANCH_SHARE <= cl.mean() <= 1 - BRANCH_SHARE) if np.isfinite(huber_delta) else not cl.any(), cl.mean()
    if form == "td3":
        assert all(BRANCH_SHARE <= m.mean() <= 1 - BRANCH_SHARE for m in (got["noise_clamped"], got["action_clamped"]))
    else:  # without noise a' is next_action as given, beyond the action clip too
        assert not got["action_clamped"].any() and np.abs(c["next_action"]).max() > 1.0
    assert 0 < b["terminated"].sum() < 96 and np.array_equal(got["rows"]["target"][b["terminated"] != 0], b["reward"][b["terminated"] != 0].astype(np.float64))


@pytest.mark.parametrize("n_critics", [1, 2])
def test_a_terminated_row_with_an_infinite_q_next_has_its_reward_as_target(n_critics):
    """the target is a where, not a product with (1 - terminated): 0 x inf would be NaN.  A target critic's head bias is +inf (with two
    critics both, or the minimum would hide it), so q_next is inf on every row; all rows terminated keep y = reward and finite
    gradients, in the model and in torch alike"""
    c = case(13, 64, 16, 1, n_critics, seed=9)
    b = c["batch"]
    for net in c["target"]:
        net[-1][1][0] = np.float32(np.inf)
    b["terminated"][:] = 1
    got = reference(c, "relu", "plain", 1.0, True, np.float64)
    assert np.isinf(got["rows"]["q_next"]).all() and np.array_equal(got["rows"]["target"], b["reward"].astype(np.float64))
    stats, grads, y, errs, _ = _torch_td(c, "relu", "plain", 1.0, True)
    assert np.array_equal(y, got["rows"]["target"]) and all(np.isfinite(e).all() for e in errs)
    for k, v in flat(got).items():
        assert np.isfinite(v).all() and rel(v, grads[k]) <= REL, k
    g32 = reference(c, "relu", "plain", 1.0, True, np.float32)
    assert np.isfinite(g32["stats"]).all() and all(np.isfinite(v).all() for v in flat(g32).values())
    b["terminated"][::2] = 0  # and a live row with an infinite q_next has an infinite target: nothing hides it
    assert np.isinf(reference(c, "relu", "plain", 1.0, True, np.float64)["rows"]["target"][::2]).all()


def test_per_row_derivative_is_the_stated_one():
    """g_c of the model against autograd of the torch loss by q_c, with weights: clipped rows carry +-delta w / n"""
    import torch
    c = case(13, 96, 33, 2, 2, seed=4)
    got = reference(c, "relu", "sac", 1.0, True, np.float64)
    w = torch.from_numpy(c["weight"].astype(np.float64))
    y = torch.from_numpy(got["rows"]["target"])
    qs = [torch.from_numpy(got["rows"][k]).requires_grad_() for k in ("q1", "q2")]
    sum((w * torch.nn.functional.huber_loss(q, y, reduction="none", delta=1.0)).mean() for q in qs).backward()
    for k, q in enumerate(qs):
        g, cl = got["rows"]["g%d" % (k + 1)], got["clipped"][k]
        assert np.allclose(g, q.grad.numpy(), rtol=1e-12, atol=0)
        assert cl.any() and np.allclose(np.abs(g[cl]), c["weight"][cl].astype(np.float64) / 96, rtol=1e-12, atol=0)


def test_float32_mode_is_float32_and_close():
    c = case(13, 300, 33, 2, 2, seed=8)
    for form in FORMS:
        m64, m32 = (reference(c, "tanh", form, 1.0, True, dt) for dt in (np.float64, np.float32))
        g64, g32 = flat(m64), flat(m32)
        tol = grad_tolerances(g32, g64)
        for k in g64:
            assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
            assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
        assert m32["stats"].dtype == np.float32 and all(m32["rows"][k].dtype == np.float32 for k in ROWS)
        for k in range(9):
            assert abs(float(m32["stats"][k]) - m64["stats"][k]) <= 1e-4 * (1 + abs(m64["stats"][k])), STATS[k]


def _conditions(m64, m32, form, huber_delta):
    """what a GPU case's tolerances rest on, of its two models"""
    g64, g32 = flat(m64), flat(m32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        top = float(np.abs(g64[k]).max())
        assert top > 0 and tol[k] <= 0.01 * top, (k, tol[k], top)
    n = m64["rows"]["td1"].shape[0]
    if np.isfinite(huber_delta):
        for k, cl in enumerate(m64["clipped"]):
            assert np.abs(np.abs(m64["rows"]["td%d" % (k + 1)]) - huber_delta).min() >= HUBER_MARGIN
            assert np.array_equal(m32["clipped"][k], cl)
            assert n < 200 or BRANCH_SHARE <= cl.mean() <= 1 - BRANCH_SHARE, cl.mean()
    if form == "td3" and n >= 200:
        for name in ("noise_clamped", "action_clamped"):
            assert BRANCH_SHARE <= m64[name].mean() <= 1 - BRANCH_SHARE and np.array_equal(m32[name], m64[name]), name


@pytest.mark.parametrize("obs_dim,n,hidden,n_hidden,n_critics,activation,form,huber_delta,weighted", grad_cases())
def test_every_gpu_case_keeps_the_conditions_its_tolerances_rest_on(obs_dim, n, hidden, n_hidden, n_critics, activation, form, huber_delta, weighted):
    """for the very cases (the same generator, the same seed) tests/test_gpu_q_td.py runs: 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|)
    <= 1 % of max|G64| per tensor; no row's |td| within 1e-4 of huber_delta and the float32 model clips the same rows; both Huber
    branches, both noise-clamp branches and both action-clamp branches each hold a tenth of the rows (of the draws, for the clamps)
    wherever there are at least 200 rows, and the float32 model takes the same ones.  A GPU failure cannot be the inputs' fault"""
    c = grad_case(obs_dim, n, hidden, n_hidden, n_critics)
    m64, m32 = (reference(c, activation, form, huber_delta, weighted, dt) for dt in (np.float64, np.float32))
    _conditions(m64, m32, form, huber_delta)


def test_the_trained_regime_case_keeps_the_cap():
    """the 1 % cap of the one trained-regime case tests/test_gpu_q_td.py runs (tests/net_regimes.py's q family: Q values in the
    hundreds), and TD errors that are large against huber_delta = 1 on most rows"""
    c, activation, form, huber_delta, weighted = regime_case()
    m64, m32 = (regime_reference(dt) for dt in (np.float64, np.float32))
    g64, tol = flat(m64), grad_tolerances(flat(m32), flat(m64))
    assert all(tol[k] <= 0.01 * float(np.abs(g64[k]).max()) for k in g64), {k: tol[k] / float(np.abs(g64[k]).max()) for k in g64}
    assert np.abs(m64["rows"]["q1"]).max() > 100 and all(cl.mean() > 0.5 for cl in m64["clipped"])
    assert all(np.array_equal(a, b) for a, b in zip(m32["clipped"], m64["clipped"]))


def test_the_cases_cover_every_option_at_every_row_count():
    cases = grad_cases()
    assert {(c[2], c[3]) for c in cases} == set(NETS) | {CLASS3_NET, (128, 1)} and {c[1] for c in cases} == set(GRAD_NS) | {BIG_N}
    assert {c[0] for c in cases} == {10, 15}
    for n in GRAD_NS:
        mine = [c for c in cases if c[1] == n]
        assert {c[6] for c in mine} == set(FORMS) and {c[8] for c in mine} == {True, False} and {c[5] for c in mine} == {"tanh", "relu"}
        assert {np.isinf(c[7]) for c in mine} == {True, False}, n
    assert [(c[1], c[6]) for c in cases if c[4] == 1] == [(200, "plain"), (2049, "td3")] and BIG_N > 256 * 64  # DDPG, and TD3 with one critic
    assert [c for c in cases if c[1] == BIG_N] == [(15, BIG_N, 128, 1, 2, "tanh", "sac", 1.0, True)]


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _batch(n=24, D=13):
    import torch
    return dict(obs=_z(n, D), action=_z(n, 2), reward=_z(n), next_obs=_z(n, D), terminated=_z(n, dtype=torch.uint8), discount=_z(n),
                truncated=_z(n, dtype=torch.uint8), steps=_z(n, dtype=torch.uint8), index=_z(n, dtype=torch.int64), cell=_z(n, dtype=torch.int64),
                weight=_z(n))


class _Sized:
    """the stub library with the workspace query answering 64 bytes"""

    def __init__(self, lib):
        self._lib, self.calls = lib, lib.calls

    def __getattr__(self, name):
        if name == "sg_q_td_grad_workspace_bytes":
            return lambda *a: 64
        return getattr(self._lib, name)

    def names(self):
        return self._lib.names()


def test_q_td_grad_torch_checks_its_arguments_before_the_native_call():
    import torch
    env = _stub_env()
    online, target = env.q_torch(critics=_q_params()), env.q_torch(critics=_q_params())
    batch, n = _batch(), 24
    na = _z(n, 2)
    call = lambda o=online, t=target, b=batch, a=na, **kw: (lambda: env.q_td_grad_torch(o, t, b, a, **kw))
    one = env.q_torch(critics=_q_params(n_critics=1))
    refused = [
        ("handle q_torch returns", call(o=_q_params())),
        ("handle q_torch returns", call(t=None)),
        ("target: expected critics of the online handle's shape", call(t=env.q_torch(critics=_q_params(hidden=17)))),
        ("target: expected critics of the online handle's shape", call(t=env.q_torch(critics=_q_params(n_hidden=1)))),
        ("target: expected critics of the online handle's shape", call(t=env.q_torch(critics=_q_params(), activation="tanh"))),
        ("target: expected critics of the online handle's shape", call(t=one)),
        ("batch: expected the dict", call(b=[batch["obs"]])),
        (r"batch\['obs'\]", call(b=dict(batch, obs=_z(n, 14)))),
        (r"batch\['obs'\]", call(b=dict(batch, obs=_z(0, 13)))),
        (r"batch\['action'\]", call(b=dict(batch, action=_z(n, dtype=torch.int32)))),
        (r"batch\['action'\]", call(b=dict(batch, action=_z(n)))),
        (r"batch\['reward'\]", call(b=dict(batch, reward=_z(n + 1)))),
        (r"batch\['next_obs'\]: missing", call(b={k: v for k, v in batch.items() if k != "next_obs"})),
        (r"batch\['next_obs'\]", call(b=dict(batch, next_obs=_z(n, 12)))),
        (r"batch\['terminated'\]", call(b=dict(batch, terminated=_z(n)))),
        (r"batch\['discount'\]: missing", call(b=dict(batch, discount=None))),
        ("next_action", call(a=None)),
        ("next_action", call(a=_z(n))),
        ("next_action", call(a=torch.zeros(n, 2))),
        ("next_logp", call(next_logp=_z(n, 1))),
        ("noise", call(noise=_z(n))),
        ("weight", call(weight=_z(n, 1))),
        ("weight", call(weight=torch.zeros(n))),
        ("huber_delta", call(huber_delta=0.0)),
        ("huber_delta", call(huber_delta=-1.0)),
        ("huber_delta", call(huber_delta=float("nan"))),
        ("huber_delta", call(huber_delta=None)),
        ("noise_std", call(noise_std=-0.1)),
        ("noise_clip", call(noise_clip=float("nan"))),
        ("action_clip", call(action_clip=-1.0)),
        ("action_clip", call(action_clip="one")),
        ("alpha", call(alpha="auto", next_logp=_z(n))),
        ("alpha", call(alpha=float("nan"), next_logp=_z(n))),
        ("alpha: a tensor is read only with next_logp", call(alpha=_z(1))),
        ("alpha", call(alpha=_z(2), next_logp=_z(n))),
        ("alpha", call(alpha=_z(1, dtype=torch.float64), next_logp=_z(n))),
        ("alpha", call(alpha=torch.zeros(1), next_logp=_z(n))),
        (r"rows\['g1'\]", call(rows=dict(g1=_z(n + 1)))),
        (r"rows\['td_error'\]", call(rows=dict(td_error=_z(n)))),
        (r"rows\['q2'\]: the handle has one critic", call(o=one, t=one, rows=dict(q2=_z(n)))),
        ("stats", call(stats=_z(8))),
        (r"out\['critics'\]: expected 2 nets", call(out=dict(critics=[[(_z(16, 15), _z(16))]]))),
        (r"out\['critics'\]\[1\]: expected 3", call(out=dict(critics=[[(_z(16, 15), _z(16)), (_z(16, 16), _z(16)), (_z(1, 16), _z(1))], [(_z(16, 15), _z(16))]]))),
        (r"out\['critics'\]: the critics' gradients need tensors", call(out=dict(action=None))),
    ]
    for match, bad in refused:
        with pytest.raises(ValueError, match=match):
            bad()
    assert env._lib.names() == []
    env.discrete = True
    with pytest.raises(ValueError, match="discrete ids are not served"):
        env.q_td_grad_torch(online, target, batch, na)
    assert env._lib.names() == []


def test_the_call_passes_the_columns_and_the_configuration():
    import torch
    from space_gym_amd import _native
    env = _stub_env()
    online, target = env.q_torch(critics=_q_params()), env.q_torch(critics=_q_params())
    batch, n = _batch(), 24
    na, logp, noise, alpha = _z(n, 2), _z(n), _z(n, 2), _z(1)
    online.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    lib = env._lib
    env._lib = _Sized(lib)
    rows = dict(td1=_z(n), q_next=_z(n), td_abs=_z(n), g2=None)
    grads, stats = env.q_td_grad_torch(online, target, batch, na, next_logp=logp, alpha=alpha, noise=noise, noise_std=0.1, noise_clip=0.3,
                                       action_clip=float("inf"), huber_delta=2.0, weight=batch["weight"], rows=rows)
    assert lib.names()[-2:] == ["sg_q_td_config_init", "sg_q_td_grad_device"]
    name, args = lib.calls[-1]
    assert name == "sg_q_td_grad_device" and args[5] == n and args[10] == 64 and args[9].value == online.workspace.data_ptr()
    assert args[1]._obj is online.struct and args[2]._obj is target.struct
    cfg, b, g, r = args[3]._obj, args[4]._obj, args[6]._obj, args[8]._obj
    assert isinstance(cfg, _native.SgQTdConfig) and tuple(cfg.reserved) == (0, 0)
    assert (cfg.huber_delta, cfg.noise_std, cfg.noise_clip, cfg.action_clip) == (2.0, np.float32(0.1), np.float32(0.3), float("inf"))
    assert (b.obs, b.action, b.reward, b.next_obs, b.terminated, b.discount, b.weight) == tuple(
        batch[k].data_ptr() for k in ("obs", "action", "reward", "next_obs", "terminated", "discount", "weight"))
    assert (b.next_action, b.next_logp, b.alpha_dev, b.noise) == (na.data_ptr(), logp.data_ptr(), alpha.data_ptr(), noise.data_ptr())
    assert tuple(getattr(r, k) for k in ROWS) == (rows["td1"].data_ptr(), None, None, None, None, rows["q_next"].data_ptr(), None, None,
                                                  rows["td_abs"].data_ptr())
    assert stats.shape == (9,) and args[7].value == stats.data_ptr() and len(grads["critics"]) == 2 and grads["action"] is None
    for c in range(2):
        assert all(g.critic[c].weight[l] == grads["critics"][c][l][0].data_ptr() and g.critic[c].bias[l] == grads["critics"][c][l][1].data_ptr()
                   for l in range(3))
    assert g.struct_size == C.sizeof(_native.SgQnetGrads)
    # the defaults: the squared loss, alpha 0.2 on the host, TD3's noise figures, no weights, no rows, no optional column
    env.q_td_grad_torch(online, target, batch, na, out=grads, stats=stats)
    args = lib.calls[-1][1]
    cfg, b = args[3]._obj, args[4]._obj
    assert cfg.huber_delta == float("inf") and (b.weight, b.next_logp, b.alpha_dev, b.noise) == (None,) * 4 and args[8] is None
    env.q_td_grad_torch(online, target, batch, na, next_logp=logp, alpha=0.25, out=grads, stats=stats)
    args = lib.calls[-1][1]
    assert args[3]._obj.alpha == 0.25 and args[4]._obj.alpha_dev is None and args[4]._obj.next_logp == logp.data_ptr()
    # the gradient dict is what adam_step_torch and _flat_grads take
    from space_gym_amd.vector_env import _flat_grads
    assert [t.data_ptr() for t in _flat_grads(online, grads)] == [t.data_ptr() for net in grads["critics"] for pair in net for t in pair]


def test_q_update_torch_composes_the_existing_calls(monkeypatch):
    """the native calls in order, and torch._foreach_lerp_ on (the target's tensors, the online ones, tau); the stand-in applies it to
    the plain tensors beneath the fake CUDA ones, which the foreach kernels do not take"""
    import torch
    real, plain = torch._foreach_lerp_, lambda ts: [t.as_subclass(torch.Tensor) for t in ts]
    lerps = []

    def lerp(a, b, w):
        lerps.append((list(a), list(b), w))
        real(plain(a), plain(b), plain(w) if isinstance(w, list) else w)
    monkeypatch.setattr(torch, "_foreach_lerp_", lerp)
    from space_gym_amd.vector_env import AdamState, SpaceGymVectorEnv
    env = _stub_env()
    par_o, par_t = _q_params(), _q_params()
    for net in par_o:
        for w, b in net:
            w.fill_(1.0); b.fill_(1.0)
    online, target = env.q_torch(critics=par_o), env.q_torch(critics=par_t)
    batch, n = _batch(), 24
    na = _z(n, 2)
    online.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    zeros = lambda: tuple(_fake_cuda(torch.zeros_like(t)) for t in online.tensors)
    opt = AdamState(online, 1, _z(1, 8), _z(1, 8, dtype=torch.float64), zeros(), zeros())
    lib = env._lib
    env._lib = _Sized(lib)
    stats, rows, grads = env.q_update_torch(online, target, opt, batch, na, weight=batch["weight"], tau=0.25)
    assert lib.names() == ["sg_q_td_config_init", "sg_q_td_grad_device", "sg_adam_step_device"] and rows == {}
    assert all(float(t.min()) == float(t.max()) == 0.25 for t in target.tensors) and all(float(t.min()) == 1.0 for t in online.tensors)
    assert len(lerps) == 1 and lerps[0][2] == 0.25 and all(a is b for a, b in zip(lerps[0][0], target.tensors))
    assert all(a is b for a, b in zip(lerps[0][1], online.tensors))
    one = _z()
    one.fill_(1.0)
    env.q_update_torch(online, target, opt, batch, na, grads=grads, stats=stats, tau=one)  # a device scalar of 1: the hard sync
    assert all(float(t.min()) == float(t.max()) == 1.0 for t in target.tensors) and all(w is one for w in lerps[1][2])
    env.q_update_torch(online, target, opt, batch, na, grads=grads, stats=stats)  # no tau: the target is the caller's to move
    assert len(lerps) == 2
    assert lib.calls[-2][1][7].value == stats.data_ptr()
    # with prio: the priority update reads rows['td_abs'], which the call makes when the caller gave none
    seen = []
    monkeypatch.setattr(SpaceGymVectorEnv, "_priority_arg", lambda self, prio, ring=None: seen.append(("arg", prio)))
    monkeypatch.setattr(SpaceGymVectorEnv, "replay_update_priorities_torch",
                        lambda self, prio, cell, td_error=None, alpha=0.6, epsilon=1e-6: seen.append(("update", prio, cell, td_error, alpha, epsilon)))
    before = len(lib.calls)
    prio = object()
    _, rows, _ = env.q_update_torch(online, target, opt, batch, na, grads=grads, stats=stats, prio=prio, priority_alpha=0.7, priority_epsilon=1e-3)
    assert [c[0] for c in lib.calls[before:]] == ["sg_q_td_config_init", "sg_q_td_grad_device", "sg_adam_step_device"]
    assert seen[0] == ("arg", prio) and seen[1][:3] == ("update", prio, batch["cell"]) and seen[1][3] is rows["td_abs"] and seen[1][4:] == (0.7, 1e-3)
    assert lib.calls[before + 1][1][8]._obj.td_abs == rows["td_abs"].data_ptr() and rows["td_abs"].shape == (n,)
    with pytest.raises(ValueError, match="opt: expected the AdamState"):
        env.q_update_torch(online, target, AdamState(target, 1, opt.hyper, opt.state, zeros(), zeros()), batch, na)
    for bad in (-0.1, 1.5, float("nan"), "soft", _z(1), _z(dtype=torch.float64)):
        with pytest.raises(ValueError, match="tau"):
            env.q_update_torch(online, target, opt, batch, na, tau=bad)
    with pytest.raises(ValueError, match=r"batch\['cell'\]: missing"):
        env.q_update_torch(online, target, opt, {k: v for k, v in batch.items() if k != "cell"}, na, prio=object())


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("q_td_grad_torch", "q_update_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
