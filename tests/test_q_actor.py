"""CPU tests of the fused actor update of SAC / TD3 / DDPG (sg_q_actor_squashed_grad_device / sg_q_actor_gaussian_grad_device /
q_actor_grad_torch / q_actor_update_torch): the declarations, the NumPy model (tests/q_actor_model.py) against torch.autograd on
float64 modules with the loss written in plain torch, the conditions every case the GPU tests run must keep (no row with its two critics
alike, the float32 model selecting the same critic and clamping the same components, every branch taken by a tenth of the rows, the 1 %
cap of the tolerances), and the Python argument checks with the native calls stubbed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from q_actor_model import ALPHA, BIG_N, BOUNDS, CASE_SEED, CLASS3_NET, FORMS, GRAD_NS, MIXED, MIXED_N, NETS, ROWS, STATS, WIDTH_FAMILY, actor_grad
from q_actor_model import case, conditions, flat, grad_case, grad_cases, grad_tolerances, reference, regime_case, regime_reference
from q_actor_model import register_width_family, same_tile, width_cases
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_q import _q_params
from test_snapshot_device import _header_args

register_width_family()  # (before any test runs: tests/test_net_widths.py counts the engine's kernel templates against the families)

REL = 1e-10  # float64 model against float64 autograd: the figure of tests/test_q.py for the same comparison


def rel(a, b):
    return float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    tail = ["const sg_q_actor_config *cfg", "int64_t n", "const float *obs", "const float *eps", "const float *alpha_dev"]
    rest = ["float *stats_out", "const sg_q_actor_rows *row_out", "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_q_actor_squashed_grad_device") == ["sg_env *env", "const sg_squashed_policy *actor", "const sg_qnet *qnet"] + tail + [
        "const sg_squashed_grads *grads"] + rest
    assert _header_args("sg_q_actor_gaussian_grad_device") == ["sg_env *env", "const sg_policy *actor", "const sg_qnet *qnet"] + tail + [
        "const sg_policy_grads *grads"] + rest
    assert _header_args("sg_q_actor_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_squashed_policy *squashed",
                                                                         "const sg_policy *gaussian", "const sg_qnet *qnet", "int64_t n"]
    assert _header_args("sg_q_actor_config_init", "void") == ["sg_q_actor_config *cfg"]
    vp, P = C.c_void_p, C.POINTER
    for name, actor, grads in (("sg_q_actor_squashed_grad_device", _native.SgSquashedPolicy, _native.SgSquashedGrads),
                               ("sg_q_actor_gaussian_grad_device", _native.SgPolicy, _native.SgPolicyGrads)):
        assert _native.SYMBOLS[name] == (C.c_int, [vp, P(actor), P(_native.SgQnet), P(_native.SgQActorConfig), C.c_int64, vp, vp, vp, P(grads), vp,
                                                   P(_native.SgQActorRows), vp, C.c_size_t, vp]), name
    assert _native.SYMBOLS["sg_q_actor_grad_workspace_bytes"] == (C.c_size_t, [vp, P(_native.SgSquashedPolicy), P(_native.SgPolicy), P(_native.SgQnet),
                                                                               C.c_int64])
    assert _native.SYMBOLS["sg_q_actor_config_init"] == (None, [P(_native.SgQActorConfig)])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls, size in (("sg_q_actor_config", _native.SgQActorConfig, 24), ("sg_q_actor_rows", _native.SgQActorRows, 64)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_] and C.sizeof(cls) == size, name
    assert [f for f, _ in _native.SgQActorRows._fields_] == list(ROWS) and all(t is vp for _, t in _native.SgQActorRows._fields_)
    cfg = _native.SgQActorConfig
    assert [(f, getattr(cfg, f).offset) for f, _ in cfg._fields_] == [("struct_size", 0), ("alpha", 4), ("target_entropy", 8), ("q_select", 12),
                                                                      ("reserved", 16)]
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert build.HEADERS.index("sg_q_actor.inc") == build.HEADERS.index("sg_q_td.inc") + 1 == build.HEADERS.index("sg_dqn.inc") - 1
    assert src.index('#include "sg_q_td.inc"') < src.index('#include "sg_q_actor.inc"') < src.index('#include "sg_dqn.inc"')
    assert re.search(r"kNetsQActor = 1024\b", src) and "case kNetsQActor:" in src
    assert "raise_lds_limit(kQActorSquashedGradKernel, bwd(Q))" in src and "raise_lds_limit(kQActorGaussianGradKernel, bwd(Q))" in src
    inc = open(os.path.join(build.CSRC, "sg_q_actor.inc")).read()
    code = re.sub(r"//.*", "", inc)
    for kernel in ("q_actor_squashed_grad_kernel", "q_actor_gaussian_grad_kernel", "q_actor_reduce_kernel"):
        assert re.search(r"void %s\(" % kernel, code), kernel
    assert len(re.findall(r"template <int NT>\s*__global__", code)) == 2 and code.count("q_actor_grad_body<NT>(") == 2
    assert "__fsub_rn(__fmul_rn(alpha, logp), q_sel)" in code and "q2 < q1 || q2 != q2" in code and "squashed_tail(" in code
    assert "policy_grad_reduce_element(" in code and "atomic" not in inc.lower()
    assert SpaceGymVectorEnv.q_actor_stats_names == STATS and len(STATS) == 9 and tuple(SpaceGymVectorEnv._Q_ACTOR_ROWS) == ROWS
    assert {"q_actor_grad_torch", "q_actor_update_torch"} <= set(NET_METHODS)
    assert all(callable(getattr(SpaceGymVectorEnv, n)) for n in ("q_actor_grad_torch", "q_actor_update_torch"))


def test_the_two_kernel_templates_are_a_width_family_with_a_test_at_every_class():
    """what tests/test_net_widths.py asks of a net kernel, for the two added here: four instantiations each in the compiler's report
    with no scratch, no spill and no dynamic stack (the reduction kernel too), named as a family in test_gpu_net_widths.FAMILY_KERNELS,
    and a GPU test that runs them at net_widths' table -- every class NT = 1 .. 4 and each class's widest net"""
    import engine_asm
    import net_widths
    import test_gpu_net_widths
    import test_gpu_q_actor
    name, kernels = WIDTH_FAMILY
    assert test_gpu_net_widths.FAMILY_KERNELS[name] == kernels
    assert sum(k in kernels for ks in test_gpu_net_widths.FAMILY_KERNELS.values() for k in ks) == 2
    classes, clean = {k: [] for k in kernels}, 0
    for row in engine_asm.resource_rows():
        m = re.match(r"_Z\d+(\w+_kernel)ILi(\d+)EE", row["name"])
        mine = m and m.group(1) in classes
        if mine:
            classes[m.group(1)].append(int(m.group(2)))
        if mine or "q_actor_reduce_kernel" in row["name"]:
            assert row["ScratchSize [bytes/lane]"] == "0" and row["VGPRs Spill"] == "0" and row["Dynamic Stack"] == "False", row
            clean += 1
    assert all(sorted(v) == [1, 2, 3, 4] for v in classes.values()) and clean == 9, (classes, clean)
    nets = [(hidden, n_hidden) for hidden, n_hidden, _ in width_cases()]
    assert set(net_widths.WIDTH_NETS) <= set(nets) and {net_widths.tile_class(h) for h, _ in nets} == {1, 2, 3, 4}
    assert all((32 * c, 3) in nets for c in (1, 2, 3, 4))
    assert test_gpu_q_actor.test_both_kernels_at_every_width_class.pytestmark[0].args[1] == width_cases()


def _torch_actor_loss(c, activation, eps_given, alpha, q_select, target_entropy=-2.0, bounds=BOUNDS):
    """the update in plain torch on float64 modules: (statistics by name, the actor's gradients by name, per-row arrays by name)"""
    import torch
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    f32 = lambda v: float(np.float32(v))  # the scalars as the engine holds them
    squashed = c["form"] == "squashed"
    obs, n = t(c["obs"]), c["obs"].shape[0]
    eps = t(c["eps"]) if eps_given else torch.zeros(n, 2, dtype=torch.float64)
    critics = [_torch_net(net, activation) for net in c["critics"]]
    if squashed:
        actor = _torch_net(c["actor"], activation)
        head = actor(obs)
        ls = torch.clamp(head[:, 2:], f32(bounds[0]), f32(bounds[1]))
        u = head[:, :2] + torch.exp(ls) * eps
        a = torch.tanh(u)
        ldj = 2.0 * (math.log(2.0) - u.abs() - torch.nn.functional.softplus(-2.0 * u.abs()))  # log(1 - tanh(u)^2)
        logp = (-0.5 * eps * eps - ls - 0.5 * math.log(2.0 * math.pi) - ldj).sum(1)
        log_std = None
    else:
        actor = _torch_net(c["actor"]["actor"], activation)
        log_std = t(c["actor"]["log_std"]).requires_grad_()
        a = actor(obs) + torch.exp(log_std) * eps
        logp = torch.zeros(n, dtype=torch.float64)
    a.retain_grad()
    x = torch.cat([obs, a], 1)
    q1 = critics[0](x)[:, 0]
    q2 = critics[1](x)[:, 0] if q_select else None
    q_sel = torch.minimum(q1, q2) if q_select else q1
    loss = (f32(alpha) * logp - q_sel).mean()
    loss.backward()
    grads = {}
    for l, m in enumerate(mod for mod in actor if isinstance(mod, torch.nn.Linear)):
        grads[f"actor.{l}.weight"], grads[f"actor.{l}.bias"] = m.weight.grad.numpy(), m.bias.grad.numpy()
    if log_std is not None:
        grads["log_std"] = log_std.grad.numpy() if log_std.grad is not None else np.zeros(2)
    assert all(p.grad is None or True for net in critics for p in net.parameters())
    dq = []
    for q in (q1, q2):
        if q is None:
            dq.append(None)
            continue
        a2 = a.detach().clone().requires_grad_()
        net = critics[0] if q is q1 else critics[1]
        net(torch.cat([obs, a2], 1))[:, 0].sum().backward()
        dq.append(a2.grad.numpy())
    sel2 = (q2 < q1).numpy() if q_select else np.zeros(n, bool)
    stats = dict(loss=loss.item(), logp_mean=logp.mean().item(), q1_mean=q1.mean().item(), q2_mean=q2.mean().item() if q_select else 0.0,
                 q_sel_mean=q_sel.mean().item(), critic2_fraction=float(sel2.mean()), action_abs_mean=a.abs().mean().item(),
                 dq_da_abs_max=max(float(np.abs(d).max()) for d in dq if d is not None),
                 log_alpha_grad=-(logp.mean().item() + f32(target_entropy)) if squashed else 0.0)
    # d loss / d a of the path through the critics alone is g_action; with the squashed actor a.grad holds that path only (logp's goes through u)
    rows = dict(action=a.detach().numpy(), logp=logp.detach().numpy(), q1=q1.detach().numpy(), q2=q2.detach().numpy() if q_select else None,
                q_sel=q_sel.detach().numpy(), dq1_da=dq[0], dq2_da=dq[1], g_action=-np.where(sel2[:, None], dq[1], dq[0]) / n if q_select else -dq[0] / n)
    return stats, grads, rows


VARIANTS = [(form, n_critics, q_select) for form in FORMS for n_critics, q_select in ((1, 0), (2, 1), (2, 0))]


@pytest.mark.parametrize("form,n_critics,q_select", VARIANTS)
@pytest.mark.parametrize("eps_given", [True, False])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_model_equals_torch_autograd_in_float64(activation, eps_given, form, n_critics, q_select):
    """the loss alpha logp - minimum(q1, q2) and -q1 (and alpha logp - q1 on two critics), every statistic, dq_c, g_action and every
    actor gradient, for tanh and relu, one and two critics, both actor forms, eps given and None"""
    c = case(13, 200, (33, 2), (17, 2), n_critics, form, activation, eps_given, seed=4)
    alpha = 0.3 if form == "squashed" else 0.0
    got = actor_grad(c["actor"], c["critics"], c["obs"], c["eps"] if eps_given else None, alpha=alpha, q_select=q_select, target_entropy=-1.5,
                     form=form, activation=activation)
    stats, grads, rows = _torch_actor_loss(c, activation, eps_given, alpha, q_select, target_entropy=-1.5)
    what = (activation, eps_given, form, n_critics, q_select)
    for k in ROWS:
        if rows[k] is None:
            assert got["rows"][k] is None, (what, k)
        elif np.abs(rows[k]).max() > 0:
            assert rel(got["rows"][k], rows[k]) <= REL, (what, k, rel(got["rows"][k], rows[k]))
        else:
            assert not got["rows"][k].any(), (what, k)
    for k, name in enumerate(STATS):
        assert abs(float(got["stats"][k]) - stats[name]) <= REL * max(abs(stats[name]), 1e-3), (what, name, float(got["stats"][k]), stats[name])
    mine = flat(got)
    assert set(mine) == set(grads) and len(mine) == 6 + (form == "gaussian")
    for k in grads:
        if k == "log_std" and not eps_given:
            assert not mine[k].any() and not grads[k].any()
            continue
        assert mine[k].shape == grads[k].shape and np.abs(grads[k]).max() > 0 and rel(mine[k], grads[k]) <= REL, (what, k, rel(mine[k], grads[k]))
    assert got["stats"].dtype == np.float64
    if q_select:
        assert 20 <= got["sel2"].sum() <= 180 and got["stats"][5] == got["sel2"].mean()
    else:
        assert got["stats"][3] == 0 and got["stats"][5] == 0 and not got["sel2"].any()
    if form == "squashed":
        assert 0 < got["inside"].sum() < got["inside"].size and got["stats"][8] == -(got["stats"][1] + (-1.5))
    else:
        assert got["stats"][8] == 0 and got["stats"][1] == 0 and got["stats"][0] == -got["stats"][4]


def test_alpha_zero_without_noise_is_the_deterministic_tanh_actor():
    """eps None and alpha 0 on the squashed actor: the loss is -mean Q(obs, tanh(mean)) and the raw log_std rows of the head get nothing"""
    c = case(13, 64, (16, 1), (16, 1), 2, "squashed", "relu", False, seed=2)
    got = actor_grad(c["actor"], c["critics"], c["obs"], None, alpha=0.0, form="squashed", activation="relu")
    g = flat(got)
    assert got["stats"][0] == -got["stats"][4] and not g["actor.1.weight"][2:].any() and g["actor.1.weight"][:2].any()
    stats, grads, _ = _torch_actor_loss(c, "relu", False, 0.0, 1)
    assert all(rel(g[k], grads[k]) <= REL for k in grads)


def test_float32_mode_is_float32_and_close():
    for form in FORMS:
        c = case(13, 300, (33, 2), (33, 2), 2, form, "tanh", True, seed=8)
        m64, m32 = (reference(c, "tanh", True, 1, dt) for dt in (np.float64, np.float32))
        g64, g32 = flat(m64), flat(m32)
        tol = grad_tolerances(g32, g64)
        for k in g64:
            assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
            assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
        assert m32["stats"].dtype == np.float32 and all(m32["rows"][k].dtype == np.float32 for k in ROWS)
        for k in range(9):
            assert abs(float(m32["stats"][k]) - m64["stats"][k]) <= 1e-4 * (1 + abs(m64["stats"][k])), STATS[k]


@pytest.mark.parametrize("gc", grad_cases(), ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_every_gpu_case_keeps_the_conditions_its_tolerances_rest_on(gc):
    """for the very cases (the same generator, the same seed) tests/test_gpu_q_actor.py runs: no row's two critics within 1e-4 max(1, |q|)
    of each other in float64, the float32 model selects the same critic on every row and clamps the same components; wherever n >= 200
    each critic is selected on at least a tenth of the rows and the log-std clamp is inside and outside on at least a tenth of the
    components each; 8 x max|x32seq - x64| + 1e-6 (1 + max|x64|) <= 1 % of max|x64| per gradient tensor and per row array (g_action
    through dq_c: see q_actor_model.conditions).  A GPU failure cannot be the inputs' fault"""
    obs_dim, n, a, q, n_critics, form, activation, eps_given, q_select = gc
    c = grad_case(obs_dim, n, a, q, n_critics, form, activation, eps_given)
    m64, m32 = (reference(c, activation, eps_given, q_select, dt) for dt in (np.float64, np.float32))
    assert conditions(m64, m32, n) is None


def test_the_case_seed_is_the_first_that_keeps_every_condition():
    """q_actor_model.find_seed, the search on the model alone that chose CASE_SEED, run again over 0 .. CASE_SEED: it returns CASE_SEED,
    with one failed condition recorded for every seed before it"""
    from q_actor_model import find_seed
    seed, failed = find_seed(CASE_SEED + 1)
    assert seed == CASE_SEED and [f[0] for f in failed] == list(range(CASE_SEED))


def test_the_trained_regime_case_keeps_the_cap():
    """the 1 % cap of the one trained-regime case tests/test_gpu_q_actor.py runs (tests/net_regimes.py's squashed actor and q critics: Q
    values in the hundreds)"""
    c, activation, eps_given, q_select = regime_case()
    m64, m32 = (regime_reference(dt) for dt in (np.float64, np.float32))
    g64, tol = flat(m64), grad_tolerances(flat(m32), flat(m64))
    assert all(tol[k] <= 0.01 * float(np.abs(g64[k]).max()) for k in g64), {k: tol[k] / float(np.abs(g64[k]).max()) for k in g64}
    assert np.abs(m64["rows"]["q1"]).max() > 100 and np.array_equal(m32["sel2"], m64["sel2"]) and np.array_equal(m32["inside"], m64["inside"])


def test_the_cases_cover_every_option_at_every_row_count():
    cases = grad_cases()
    assert {(c[2], c[3]) for c in cases} == {(net, net) for net in NETS + [CLASS3_NET, (128, 1)]} | set(MIXED)
    assert {c[1] for c in cases} == set(GRAD_NS) | {BIG_N, MIXED_N} and {c[0] for c in cases} == {10, 15}
    for n in GRAD_NS:
        mine = [c for c in cases if c[1] == n and c[2] == c[3]]
        assert {c[5] for c in mine} == set(FORMS) and {c[6] for c in mine} == {"tanh", "relu"} and {c[2] for c in mine} == set(NETS + [CLASS3_NET]), n
    assert {c[7] for c in cases} == {True, False} and {c[4] for c in cases} == {1, 2} and {c[8] for c in cases} == {None, 0, 1}
    assert any(c[8] == 0 and c[4] == 2 for c in cases) and any(c[8] == 1 and c[5] == "gaussian" for c in cases)
    assert [c for c in cases if c[1] == BIG_N][0][2:4] == ((128, 1), (128, 1)) and BIG_N > 256 * 64
    # the classes' tiles are 256 / 64, 64 / 128 and 64 / 64 rows; the kernel walks the larger class's, which in the second pair is the actor's own
    assert [same_tile(a, q) for a, q in MIXED] == [False, True, True]


def _z(*shape, dtype=None):
    import torch
    return _fake_cuda(torch.zeros(shape, dtype=dtype or torch.float32))


def _squashed_params(D=13, hidden=16, n_hidden=2):
    dims = [D] + [hidden] * n_hidden + [4]
    return [(_z(o, i), _z(o)) for i, o in zip(dims[:-1], dims[1:])]


class _Sized:
    """the stub library with the workspace query answering 64 bytes"""

    def __init__(self, lib):
        self._lib, self.calls, self.queries = lib, lib.calls, []

    def __getattr__(self, name):
        if name == "sg_q_actor_grad_workspace_bytes":
            return lambda *a: self.queries.append(a) or 64
        return getattr(self._lib, name)

    def names(self):
        return self._lib.names()


def _handles(env):
    sp = env.squashed_policy_torch(actor=_squashed_params())
    par = _params()
    pol = env.policy_torch(actor=par["actor"], critic=par["critic"], log_std=par["log_std"])
    return sp, pol, env.q_torch(critics=_q_params()), env.q_torch(critics=_q_params(n_critics=1))


def test_q_actor_grad_torch_checks_its_arguments_before_the_native_call():
    import torch
    env = _stub_env()
    sp, pol, q, one = _handles(env)
    n = 24
    obs = _z(n, 13)
    call = lambda a=sp, qq=q, o=obs, **kw: (lambda: env.q_actor_grad_torch(a, qq, o, **kw))
    refused = [
        ("actor: expected the handle", call(a=_squashed_params())),
        ("actor: expected the handle", call(a=q)),
        ("handle q_torch returns", call(qq=sp)),
        ("handle q_torch returns", call(qq=None)),
        ("obs", call(o=_z(n, 14))),
        ("obs", call(o=_z(0, 13))),
        ("obs", call(o=torch.zeros(n, 13))),
        ("eps", call(eps=_z(n))),
        ("eps", call(eps=_z(n, 2, dtype=torch.float64))),
        ("q_select", call(q_select=2)),
        ("q_select", call(q_select=True)),
        ("q_select", call(q_select="min")),
        ("q_select: 1 takes the minimum of two critics", call(qq=one, q_select=1)),
        ("alpha", call(alpha=-0.1)),
        ("alpha", call(alpha=float("nan"))),
        ("alpha", call(alpha="auto")),
        ("alpha", call(alpha=_z(2))),
        ("alpha", call(alpha=_z(1, dtype=torch.float64))),
        ("alpha", call(alpha=torch.zeros(1))),
        ("alpha: the policy_torch actor has no log-prob term", call(a=pol, alpha=0.2)),
        ("alpha: the policy_torch actor has no log-prob term", call(a=pol, alpha=_z(1))),
        ("target_entropy", call(target_entropy=float("nan"))),
        ("target_entropy", call(target_entropy=None)),
        (r"rows\['g_action'\]", call(rows=dict(g_action=_z(n)))),
        (r"rows\['logp'\]", call(rows=dict(logp=_z(n, 2)))),
        (r"rows\['td_abs'\]", call(rows=dict(td_abs=_z(n)))),
        (r"rows\['q2'\]: critic 2 does not run", call(q_select=0, rows=dict(q2=_z(n)))),
        (r"rows\['dq2_da'\]: critic 2 does not run", call(qq=one, rows=dict(dq2_da=_z(n, 2)))),
        (r"rows\['q2'\]: critic 2 does not run", call(a=pol, alpha=0.0, rows=dict(q2=_z(n)))),
        ("stats", call(stats=_z(8))),
        (r"out\['actor'\]: expected 3", call(out=dict(actor=[(_z(16, 13), _z(16))]))),
        (r"out\['actor'\]\[2\] weight", call(out=dict(actor=[(_z(16, 13), _z(16)), (_z(16, 16), _z(16)), (_z(2, 16), _z(4))]))),
        (r"out\['log_std'\]", call(a=pol, alpha=0.0, out=dict(actor=[(_z(16, 13), _z(16)), (_z(16, 16), _z(16)), (_z(2, 16), _z(2))]))),
    ]
    for match, bad in refused:
        with pytest.raises(ValueError, match=match):
            bad()
    assert env._lib.names() == []
    env.discrete = True
    with pytest.raises(ValueError, match="discrete ids are not served"):
        env.q_actor_grad_torch(sp, q, obs)
    assert env._lib.names() == []


def test_the_call_passes_the_handles_and_the_configuration():
    import torch
    from space_gym_amd import _native
    from space_gym_amd.vector_env import _flat_grads
    env = _stub_env()
    sp, pol, q, one = _handles(env)
    n = 24
    obs, eps, alpha = _z(n, 13), _z(n, 2), _z(1)
    for h in (sp, pol):
        h.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    lib = env._lib
    env._lib = sized = _Sized(lib)
    rows = dict(action=_z(n, 2), q_sel=_z(n), dq2_da=_z(n, 2), logp=None)
    grads, stats = env.q_actor_grad_torch(sp, q, obs, eps, alpha=alpha, target_entropy=-3.0, rows=rows)
    assert lib.names()[-2:] == ["sg_q_actor_config_init", "sg_q_actor_squashed_grad_device"]
    args = lib.calls[-1][1]
    assert args[1]._obj is sp.struct and args[2]._obj is q.struct and args[4] == n and args[12] == 64 and args[11].value == sp.workspace.data_ptr()
    cfg, g, r = args[3]._obj, args[8]._obj, args[10]._obj
    assert isinstance(cfg, _native.SgQActorConfig) and tuple(cfg.reserved) == (0, 0)
    assert (cfg.alpha, cfg.target_entropy, cfg.q_select) == (0.0, -3.0, 1)  # the default on two critics: the minimum
    assert (args[5].value, args[6].value, args[7].value, args[9].value) == (obs.data_ptr(), eps.data_ptr(), alpha.data_ptr(), stats.data_ptr())
    assert tuple(getattr(r, k) for k in ROWS) == (rows["action"].data_ptr(), None, None, None, rows["q_sel"].data_ptr(), None,
                                                  rows["dq2_da"].data_ptr(), None)
    assert stats.shape == (9,) and set(grads) == {"actor"} and g.struct_size == C.sizeof(_native.SgSquashedGrads)
    assert all(g.actor.weight[l] == grads["actor"][l][0].data_ptr() and g.actor.bias[l] == grads["actor"][l][1].data_ptr() for l in range(3))
    query = sized.queries[-1]
    assert query[1]._obj is sp.struct and query[2] is None and query[3]._obj is q.struct and query[4] == n
    assert [t.data_ptr() for t in _flat_grads(sp, grads)] == [t.data_ptr() for pair in grads["actor"] for t in pair]
    # the defaults: alpha 0.2 on the host, target_entropy -2, no eps, no rows; one critic: critic 1
    env.q_actor_grad_torch(sp, one, obs, out=grads, stats=stats)
    args = lib.calls[-1][1]
    cfg = args[3]._obj
    assert (cfg.alpha, cfg.target_entropy, cfg.q_select) == (np.float32(0.2), -2.0, 0) and args[6] is None and args[7] is None and args[10] is None
    env.q_actor_grad_torch(sp, q, obs, q_select=0, out=grads, stats=stats)
    assert lib.calls[-1][1][3]._obj.q_select == 0
    # the Gaussian form: the other entry point, sg_policy_grads with log_std, critic 1 by default and the minimum on request
    g2, s2 = env.q_actor_grad_torch(pol, q, obs, eps, alpha=0)
    name, args = lib.calls[-1]
    assert name == "sg_q_actor_gaussian_grad_device" and args[1]._obj is pol.struct and args[3]._obj.q_select == 0 and args[3]._obj.alpha == 0.0
    assert set(g2) == {"actor", "log_std"} and args[8]._obj.log_std == g2["log_std"].data_ptr() and args[11].value == pol.workspace.data_ptr()
    assert isinstance(args[8]._obj, _native.SgPolicyGrads) and len(g2["actor"]) == 3 and g2["actor"][2][0].shape == (2, 16)
    query = sized.queries[-1]
    assert query[1] is None and query[2]._obj is pol.struct
    env.q_actor_grad_torch(pol, q, obs, alpha=0.0, q_select=1, out=g2, stats=s2)
    assert lib.calls[-1][1][3]._obj.q_select == 1
    assert [t.data_ptr() for t in _flat_grads(pol, g2) if t is not None] == [t.data_ptr() for pair in g2["actor"] for t in pair] + [
        g2["log_std"].data_ptr()]  # (the policy's own critic: None, as behind policy_action_grad_torch)


def test_q_actor_update_torch_is_the_gradient_call_and_the_adam_step():
    import torch
    from space_gym_amd.vector_env import AdamState
    env = _stub_env()
    sp, pol, q, one = _handles(env)
    n = 24
    obs, eps = _z(n, 13), _z(n, 2)
    sp.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    zeros = lambda h: tuple(_fake_cuda(torch.zeros_like(t)) for t in h.tensors)
    opt = AdamState(sp, 1, _z(1, 8), _z(1, 8, dtype=torch.float64), zeros(sp), zeros(sp))
    lib = env._lib
    env._lib = _Sized(lib)
    stats, rows, grads = env.q_actor_update_torch(sp, q, opt, obs, eps, alpha=0.1)
    assert lib.names() == ["sg_q_actor_config_init", "sg_q_actor_squashed_grad_device", "sg_adam_step_device"] and rows == {}
    grad_args = lib.calls[1][1]
    assert grad_args[6].value == eps.data_ptr() and grad_args[3]._obj.alpha == np.float32(0.1) and grad_args[10] is None
    mine = dict(q_sel=_z(n))
    s2, r2, g2 = env.q_actor_update_torch(sp, q, opt, obs, rows=mine, grads=grads, stats=stats, q_select=0, target_entropy=-1.0)
    assert s2 is stats and g2 is grads and r2 == mine and r2 is not mine
    assert [c[0] for c in lib.calls[3:]] == ["sg_q_actor_config_init", "sg_q_actor_squashed_grad_device", "sg_adam_step_device"]
    args = lib.calls[4][1]
    assert args[9].value == stats.data_ptr() and args[10]._obj.q_sel == mine["q_sel"].data_ptr() and args[6] is None
    assert (args[3]._obj.q_select, args[3]._obj.target_entropy) == (0, -1.0)
    assert args[8]._obj.actor.weight[0] == grads["actor"][0][0].data_ptr()
    for bad in (AdamState(q, 1, opt.hyper, opt.state, zeros(q), zeros(q)), None):
        with pytest.raises(ValueError, match="opt: expected the AdamState"):
            env.q_actor_update_torch(sp, q, bad, obs)
    with pytest.raises(ValueError, match="alpha"):
        env.q_actor_update_torch(sp, q, opt, obs, alpha=-1.0)
    assert len(lib.calls) == 6


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("q_actor_grad_torch", "q_actor_update_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
