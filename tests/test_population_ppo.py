"""CPU tests of the fused PPO minibatch update for policy populations (sg_ppo_population_grad_device / population_ppo_grad_torch; DESIGN
section 25): the declarations, the NumPy statement (tests/population_ppo_model.py) against torch.autograd on float64 module stacks with
the loss written in plain torch and summed over the members, the members' independence, the grouping rule, the 1 % cap of the GPU
file's beyond-the-cap cases, and the Python argument checks with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from policy_grad_model import flat, grad_tolerances
from population_model import GROUP_CAP, grad_rows, groups, groups_single, member, random_population
from population_ppo_model import (ADV_CAP, BEYOND_CASES, BEYOND_KW, BEYOND_P, COEF, adv_groups, adv_groups_single, beyond_case,
                                  beyond_reference, bit_equal_to_single, magnitudes, member_kwargs, population_ppo, stats, synthetic_batch,
                                  workspace_bytes)
from ppo_model import STATS
from test_episode_stats import _fake_cuda, _stub_env
from test_population import _stacked, _z
from test_ppo import _assert_equal_to_torch, _torch_ppo
from test_snapshot_device import _header_args

D, ROWS, P, N = 13, 450, 3, 150
# per-member coefficients (COEF's order) of each variant; None: the call's scalars
COEFS = np.array([[0.2, 0.2, 0.01, 0.5], [0.1, 0.0, 0.0, 1.0], [0.3, 0.15, 0.03, 0.25]], np.float32)
VARIANTS = {
    "coef": dict(coef=COEFS),
    "scalars": dict(clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.25),
    "no_vclip": dict(ent_coef=0.02),
    "raw_adv": dict(coef=COEFS, normalize_advantage=False),
    "nocritic": dict(coef=COEFS),
}


def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    assert _header_args("sg_ppo_population_grad_device") == [
        "sg_env *env", "const sg_policy *policy", "int32_t members", "const sg_ppo_config *cfg", "const sg_ppo_batch *batch",
        "const float *member_coef", "int64_t rows", "int64_t n", "const sg_policy_grads *grads", "float *stats_out", "const sg_ppo_rows *row_out",
        "void *workspace", "size_t workspace_bytes", "void *hip_stream"]
    assert _header_args("sg_ppo_population_grad_workspace_bytes", "size_t") == [
        "sg_env *env", "const sg_policy *policy", "int32_t members", "int64_t n"]
    # the single-policy call with `members` after the policy and `member_coef` after the batch
    assert [a for a in _header_args("sg_ppo_population_grad_device") if a not in ("int32_t members", "const float *member_coef")] == _header_args(
        "sg_ppo_grad_device")
    vp, Pt = C.c_void_p, C.POINTER
    assert _native.SYMBOLS["sg_ppo_population_grad_device"] == (
        C.c_int, [vp, Pt(_native.SgPolicy), C.c_int32, Pt(_native.SgPpoConfig), Pt(_native.SgPpoBatch), vp, C.c_int64, C.c_int64,
                  Pt(_native.SgPolicyGrads), vp, Pt(_native.SgPpoRows), vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_ppo_population_grad_workspace_bytes"] == (C.c_size_t, [vp, Pt(_native.SgPolicy), C.c_int32, C.c_int64])
    # the structs keep their sizes: members and member_coef are arguments
    assert [C.sizeof(c) for c in (_native.SgPolicy, _native.SgPpoConfig, _native.SgPpoBatch, _native.SgPpoRows)] == [160, 32, 56, 32]
    assert SpaceGymVectorEnv.ppo_coef_names == COEF and "population_ppo_grad_torch" in NET_METHODS
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert re.search(r"kNetsPpo = 64\b", src) and re.search(r"kNetsPpoPopulation = 128\b", src)
    header = open(os.path.join(build.ROOT, "include", "spacegym.h")).read()
    assert "ceil(n / R) <= 256 / members" in header and "ceil(n / 1024) <= 256 / members" in header


def test_the_kernels_live_in_sg_ppo_inc_and_use_no_atomics():
    from space_gym_amd import build
    inc = open(os.path.join(build.CSRC, "sg_ppo.inc")).read()
    for kernel in ("ppo_population_adv_stats_kernel", "ppo_population_grad_kernel", "ppo_population_reduce_kernel", "ppo_adv_stats_kernel",
                   "ppo_grad_kernel", "ppo_reduce_kernel"):
        assert re.search(r"void %s\(" % kernel, inc), kernel
    code = re.sub(r"//.*", "", inc)
    assert "atomic" not in code.lower()
    # one statistics body and one advantage body serve both forms (the definition and two calls); the backward has two frames over
    # the same device functions, the critic's and the actor's walk and the two scoring calls in each
    assert code.count("ppo_stats_finish(") == 3 and code.count("ppo_adv_stats(") == 3 and code.count("policy_grad_reduce_element(") == 2
    assert code.count("policy_grad_net<NT>(") == 4 and code.count("policy_score(") == 4 and code.count("ppo_adv_finish(") == 4
    pop = open(os.path.join(build.CSRC, "sg_population.inc")).read()
    assert "ppo" not in pop.lower()


def _case(continuous, critic, activation, seed=11, hidden=33, n_hidden=2):
    """P dense members, one shared batch, distinct index rows (member m draws from the rows r with r % P == m, around whose stored logp
    and value its own lie)"""
    rng = np.random.default_rng(seed)
    pop = random_population(rng, P, D, hidden, n_hidden, 2 if continuous else 6, critic=critic, continuous=continuous)
    batch = synthetic_batch(rng, pop, ROWS, continuous, activation)
    index = np.stack([m + P * rng.integers(0, ROWS // P, N) for m in range(P)]).astype(np.int64)
    return pop, batch, index, rng


def _model_kwargs(kw, m):
    rest = {k: v for k, v in kw.items() if k not in ("coef", "clip_range", "clip_range_vf", "ent_coef", "vf_coef")}
    return dict(rest, **member_kwargs(kw.get("coef"), m, **{k: kw[k] for k in ("clip_range", "clip_range_vf", "ent_coef", "vf_coef") if k in kw}))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("continuous", [True, False])
def test_model_equals_torch_autograd_on_float64_module_stacks(continuous, activation, variant):
    """the loss of every member in plain torch on its own float64 modules (tests/test_ppo.py's), summed over the members -- the members
    share no parameter, so the gradient of the sum by member m's parameters is the gradient of member m's loss"""
    kw = VARIANTS[variant]
    pop, batch, index, rng = _case(continuous, variant != "nocritic", activation)
    got = population_ppo(pop, batch, index, activation=activation, **kw)
    assert len(got) == P and stats(got).shape == (P, 12)
    for m in range(P):
        mk = _model_kwargs(kw, m)
        want_stats, want_grads = _torch_ppo(member(pop, m), batch, index[m], activation, **mk)
        _assert_equal_to_torch(got[m], want_stats, want_grads, (continuous, activation, variant, m))  # 1e-10 relative
        # both branches of both max hold at least 10 % of every member's rows
        assert 0.1 <= got[m]["pg_unclipped"].mean() <= 0.9, (m, got[m]["pg_unclipped"].mean())
        if mk["clip_range_vf"] is not None and variant != "nocritic":
            assert 0.1 <= got[m]["v_unclipped"].mean() <= 0.9, (m, got[m]["v_unclipped"].mean())
        else:
            assert got[m]["v_unclipped"].all()
        if not kw.get("normalize_advantage", True):
            assert got[m]["stats"][7] == 0 and got[m]["stats"][8] == 0
        if variant == "nocritic":
            assert got[m]["critic"] is None and got[m]["stats"][2] == 0
    # the members' results differ: coefficients, parameters and rows all do
    assert len({got[m]["stats"][:7].tobytes() for m in range(P)}) == P


def test_index_none_gives_member_m_the_rows_m_n_onwards():
    pop, batch, index, rng = _case(True, True, "tanh")
    a = population_ppo(pop, batch, None, coef=COEFS)
    n = ROWS // P
    b = population_ppo(pop, batch, np.arange(P * n).reshape(P, n), coef=COEFS)
    for m in range(P):
        assert a[m]["stats"].tobytes() == b[m]["stats"].tobytes() and a[m]["rows"]["logp"].shape == (n,)


def _bits(r):
    out = {k: v.tobytes() for k, v in flat(r).items()}
    out["stats"] = r["stats"].tobytes()
    out.update({"rows." + k: v.tobytes() for k, v in r["rows"].items() if v is not None})
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_members_outputs_depend_on_nothing_of_another_member(dtype):
    """changing member 1's parameters, index row or coefficients -- a NaN ent_coef among them -- leaves members 0 and 2 bit-equal"""
    pop, batch, index, rng = _case(True, True, "tanh", seed=4)
    base = population_ppo(pop, batch, index, coef=COEFS, dtype=dtype)
    other = random_population(np.random.default_rng(99), P, D, 33, 2, 2)
    swap = lambda a, b: [(np.concatenate([W[:1], W2[1:2], W[2:]]), np.concatenate([c[:1], c2[1:2], c[2:]])) for (W, c), (W2, c2) in zip(a, b)]
    changed_pop = dict(actor=swap(pop["actor"], other["actor"]), critic=swap(pop["critic"], other["critic"]),
                       log_std=np.concatenate([pop["log_std"][:1], other["log_std"][1:2], pop["log_std"][2:]]))
    idx2 = index.copy()
    idx2[1] = rng.integers(0, ROWS, N)
    idx2[1, :3] = (-1, ROWS, 10 ** 12)
    coef2, coef3 = COEFS.copy(), COEFS.copy()
    coef2[1] = (0.05, 0.5, 0.1, 2.0)
    coef3[1, 2] = np.nan
    for what, r in (("parameters", population_ppo(changed_pop, batch, index, coef=COEFS, dtype=dtype)),
                    ("index", population_ppo(pop, batch, idx2, coef=COEFS, dtype=dtype)),
                    ("coefficients", population_ppo(pop, batch, index, coef=coef2, dtype=dtype)),
                    ("nan", population_ppo(pop, batch, index, coef=coef3, dtype=dtype))):
        assert _bits(r[0]) == _bits(base[0]) and _bits(r[2]) == _bits(base[2]), what
        assert _bits(r[1]) != _bits(base[1]), what
    nan = population_ppo(pop, batch, index, coef=coef3, dtype=dtype)
    assert np.isnan(nan[1]["stats"][0]) and np.isnan(flat(nan[1])["log_std"]).any() and np.isfinite(stats([nan[0], nan[2]])).all()
    assert population_ppo(pop, batch, idx2, coef=COEFS, dtype=dtype)[1]["stats"][9] == 3


def test_the_grouping_rule_and_its_two_bit_equality_conditions():
    """G = min(ceil(n / R), max(1, 256 / P)) workgroups per member for the parameter partials, Gadv = min(ceil(n / 1024), max(1, 256 / P))
    for the advantage partials; a member's bits are the single call's while BOTH equal the single call's counts"""
    for R in (256, 128, 64):
        for members in (1, 2, 3, 4, 16, 64, 100, 256, 257, 1000, 65535):
            cap = max(1, GROUP_CAP // members)
            for n in (1, 2, R - 1, R, R + 1, 200, 1024, 1025, 2049, 4 * R, 4 * R + 1, 4096, 4097, 4396, cap * R, cap * R + 1, cap * 1024,
                      cap * 1024 + 1, 65536, 300000):
                G, Ga = groups(n, R, members), adv_groups(n, members)
                assert 1 <= G <= cap and 1 <= Ga <= cap and G <= -(-n // R) and Ga <= -(-n // 1024)
                same = G == groups_single(n, R) and Ga == adv_groups_single(n)
                if members <= GROUP_CAP:
                    # the stated conditions are sufficient; they are necessary too unless the single call is itself at its cap of 256,
                    # which only one member's workgroups can equal
                    assert not bit_equal_to_single(n, R, members) or same, (R, members, n)
                    assert bit_equal_to_single(n, R, members) == same or members == 1, (R, members, n)
                    assert members * G <= GROUP_CAP and members * Ga <= ADV_CAP
                else:  # one workgroup per member; the single call's grouping only where it takes one workgroup as well
                    assert G == Ga == 1 and not bit_equal_to_single(n, R, members)
                total = 1234
                need = workspace_bytes(n, R, members, total)
                assert need % 4 == 0 and need >= 4 * members * G * total + 16 * members * Ga + 32 * members * G
                assert need <= 4 * max(GROUP_CAP, members) * total + 7 + 16 * max(ADV_CAP, members) + 32 * max(GROUP_CAP, members)
    # P = 1 is the single call's grouping at every n; the GPU file's shapes: bit-equal ones and the four beyond the cap
    assert all(groups(n, R, 1) == groups_single(n, R) and adv_groups(n, 1) == adv_groups_single(n) for R in (256, 128, 64) for n in (1, 4097, 10 ** 6))
    assert all(bit_equal_to_single(n, R, 3) for R in (256, 128, 64) for n in (2, 200, 2049))
    assert all(grad_rows(h) == R and not bit_equal_to_single(n, R, BEYOND_P) for h, R, n in BEYOND_CASES)
    assert -(-4396 // 1024) > ADV_CAP // BEYOND_P and -(-(4 * 256 + 300) // 1024) <= ADV_CAP // BEYOND_P


@pytest.mark.parametrize("continuous", [True, False], ids=["continuous", "discrete"])
@pytest.mark.parametrize("hidden,R,n", BEYOND_CASES)
def test_every_beyond_the_cap_case_has_a_tolerance_of_at_most_one_percent(hidden, R, n, continuous):
    """DESIGN section 18's tolerance, 8 x |m32 - m64| + 1e-6 (1 + |m64|), is at most 1 % of the float64 magnitude for every gradient
    tensor, per-row vector and statistic 0 .. 8 of the GPU file's beyond-the-cap cases (the same seeds): every eighth member, which
    takes in members with and without value clipping"""
    c = beyond_case(hidden, R, n, continuous)
    chosen = list(range(1, BEYOND_P, 8)) + [0]
    m64s, m32s = beyond_reference(c, np.float64, chosen), beyond_reference(c, np.float32, chosen)
    worst = 0.0
    for m in chosen:
        m64, m32 = m64s[m], m32s[m]
        g64, g32 = flat(m64), flat(m32)
        tol = grad_tolerances(g32, g64)
        for k in g64:
            top = float(np.abs(g64[k]).max())
            assert top > 0 and tol[k] <= 0.01 * top, (m, k, tol[k], top)
            worst = max(worst, tol[k] / top)
        for k in ("g_logp", "g_value"):
            want = m64["rows"][k]
            top = float(np.abs(want).max())
            t = 8.0 * float(np.abs(m32["rows"][k].astype(np.float64) - want).max()) + 1e-6 * (1.0 + top)
            assert t <= 0.01 * top, (m, k, t, top)
        kw = member_kwargs(c["coef"], m)
        mags = magnitudes(m64, kw, True)
        for k in range(9):
            if mags[k] == 0.0:
                continue
            t = 8.0 * abs(float(m32["stats"][k]) - float(m64["stats"][k])) + 1e-6 * (1.0 + abs(float(m64["stats"][k])))
            assert t <= 0.01 * mags[k], (m, STATS[k], t, mags[k])
    print("worst gradient tolerance / magnitude %.4f" % worst)


def _args(P=4, n=24, rows=120, discrete=False):
    import torch
    batch = dict(obs=_z(rows, D), action=_z(rows, dtype=torch.int32) if discrete else _z(rows, 2), logp=_z(rows), advantage=_z(rows), ret=_z(rows),
                 value=_z(rows))
    return batch, _z(P, n, dtype=torch.int64), _z(P, 4)


def test_population_ppo_grad_torch_checks_its_arguments_before_the_native_call():
    import torch
    env = _stub_env()
    par = _stacked()
    pop, nc = env.policy_population_torch(4, **par), env.policy_population_torch(4, **dict(par, critic=None))
    batch, index, coef = _args()
    n = 24
    call = env.population_ppo_grad_torch
    no_value = {k: v for k, v in batch.items() if k != "value"}
    pairs = lambda p: [(_z(*w.shape), _z(*b.shape)) for w, b in p]
    good = dict(actor=pairs(par["actor"]), critic=pairs(par["critic"]), log_std=_z(4, 2))
    refused = [
        ("handle policy_population_torch returns", lambda: call(env.population_member_torch(pop, 0), batch, index)),
        ("handle policy_population_torch returns", lambda: call(par, batch, index)),
        ("batch: expected a dict", lambda: call(pop, [batch["obs"]], index)),
        (r"batch\['obs'\]", lambda: call(pop, dict(batch, obs=_z(120, 14)), index)),
        (r"batch\['action'\]", lambda: call(pop, dict(batch, action=_z(119, 2)), index)),
        (r"batch\['logp'\]", lambda: call(pop, dict(batch, logp=_z(4, 30)), index)),
        (r"batch\['ret'\]: missing", lambda: call(pop, {k: v for k, v in batch.items() if k != "ret"}, index)),
        (r"batch\['value'\]: missing \(clip_range_vf", lambda: call(pop, no_value, index, clip_range_vf=0.2)),
        (r"batch\['value'\]: missing \(coef is given", lambda: call(pop, no_value, index, coef=coef)),
        (r"index: expected an int64 CUDA tensor of shape \(4, n\)", lambda: call(pop, batch, _z(n, dtype=torch.int64))),
        (r"index: expected an int64 CUDA tensor of shape \(4, n\)", lambda: call(pop, batch, _z(3, n, dtype=torch.int64))),
        (r"index: expected an int64 CUDA tensor of shape \(4, n\)", lambda: call(pop, batch, _z(4, 0, dtype=torch.int64))),
        ("index", lambda: call(pop, batch, _z(4, n, dtype=torch.int32))),
        ("index", lambda: call(pop, batch, _fake_cuda(torch.zeros((n, 4), dtype=torch.int64).t()))),
        ("index: None gives member m", lambda: call(pop, {k: v[:3] for k, v in batch.items()})),
        ("coef", lambda: call(pop, batch, index, coef=_z(4, 3))),
        ("coef", lambda: call(pop, batch, index, coef=_z(3, 4))),
        ("coef", lambda: call(pop, batch, index, coef=_z(4, 4, dtype=torch.float64))),
        ("coef: expected a CUDA tensor", lambda: call(pop, batch, index, coef=torch.zeros(4, 4))),
        ("coef.*not contiguous", lambda: call(pop, batch, index, coef=_fake_cuda(torch.zeros(4, 4).t()))),
        ("clip_range: expected", lambda: call(pop, batch, index, coef=coef, clip_range=0.0)),  # the scalars are checked beside a tensor
        ("clip_range_vf: expected", lambda: call(pop, batch, index, clip_range_vf=-0.1)),
        ("ent_coef", lambda: call(pop, batch, index, coef=coef, ent_coef=-1e-3)),
        ("vf_coef", lambda: call(pop, batch, index, vf_coef=float("nan"))),
        ("normalize_advantage: needs n >= 2", lambda: call(pop, batch, _z(4, 1, dtype=torch.int64))),
        ("stats", lambda: call(pop, batch, index, stats=_z(12))),
        ("stats", lambda: call(pop, batch, index, stats=_z(4, 11))),
        (r"rows\['g_logp'\]", lambda: call(pop, batch, index, rows=dict(g_logp=_z(n)))),
        (r"rows\['logp'\]", lambda: call(pop, batch, index, rows=dict(logp=_z(4, n + 1)))),
        (r"rows\['ratio'\]", lambda: call(pop, batch, index, rows=dict(ratio=_z(4, n)))),
        (r"rows\['value'\]: the population has no critic", lambda: call(nc, batch, index, rows=dict(value=_z(4, n)))),
        (r"out\['actor'\]\[0\] weight", lambda: call(pop, batch, index, out={**good, "actor": [(_z(16, 13), _z(16))] + good["actor"][1:]})),
        (r"out\['critic'\]: the population has a critic", lambda: call(pop, batch, index, out={**good, "critic": None})),
        (r"out\['critic'\]: the population has no critic", lambda: call(nc, batch, index, out=good)),
        (r"out\['log_std'\]", lambda: call(pop, batch, index, out={**good, "log_std": _z(2)})),
    ]
    for match, f in refused:
        with pytest.raises(ValueError, match=match):
            f()
    assert [c for c in env._lib.names() if c != "sg_ppo_config_init"] == []


def test_the_call_passes_members_the_coefficients_and_the_shared_batch():
    import torch
    from space_gym_amd import _native
    env = _stub_env()
    par = _stacked()
    pop = env.policy_population_torch(4, **par)
    batch, index, coef = _args()
    pop.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    lib = env._lib
    real = lib.__getattr__

    class Sized(type(lib)):
        def __getattr__(self, name):
            if name == "sg_ppo_population_grad_workspace_bytes":
                return lambda *a: 64
            return real(name)
    env._lib = Sized()
    env._lib.calls = lib.calls
    rows = dict(g_logp=_z(4, 24))
    grads, st = env.population_ppo_grad_torch(pop, batch, index, coef=coef, rows=rows, normalize_advantage=False)
    name, args = lib.calls[-1]
    assert name == "sg_ppo_population_grad_device" and args[2] == 4 and args[5].value == coef.data_ptr() and args[6:8] == (120, 24) and args[12] == 64
    cfg, b, r = args[3]._obj, args[4]._obj, args[10]._obj
    assert isinstance(cfg, _native.SgPpoConfig) and cfg.normalize_advantage == 0 and cfg.reserved == 0
    assert (b.obs, b.old_value, b.index) == (batch["obs"].data_ptr(), batch["value"].data_ptr(), index.data_ptr())
    assert (r.logp, r.g_logp) == (None, rows["g_logp"].data_ptr())
    assert tuple(st.shape) == (4, 12) and tuple(grads["actor"][0][0].shape) == (4, 16, 13) and tuple(grads["log_std"].shape) == (4, 2)
    # scalars only, no index: n = rows // P, no coefficient tensor, no old_value without value clipping
    env.population_ppo_grad_torch(pop, batch, ent_coef=0.01)
    args = lib.calls[-1][1]
    assert args[5] is None and args[6:8] == (120, 30) and args[4]._obj.old_value is None and args[4]._obj.index is None and args[10] is None
    # ppo_assign_grads hands the stacked tensors to the stacked parameters
    env.ppo_assign_grads(pop, grads)
    flat_grads = [t for pair in grads["actor"] + grads["critic"] for t in pair] + [grads["log_std"]]
    assert len(pop.tensors) == len(flat_grads) == 13
    assert all(p.grad is g and p.grad.shape == p.shape for p, g in zip(pop.tensors, flat_grads))
    nc = env.policy_population_torch(4, **dict(par, critic=None))
    for p in nc.tensors:
        p.grad = None
    g_nc = dict(actor=grads["actor"], critic=None, log_std=grads["log_std"])
    env.ppo_assign_grads(nc, g_nc)
    assert len(nc.tensors) == 7 and all(p.grad is g for p, g in zip(nc.tensors, [t for pair in grads["actor"] for t in pair] + [grads["log_std"]]))


def test_the_multi_device_front_ends_refuse_the_call():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        with pytest.raises(NotImplementedError, match="single-device front end only"):
            cls.population_ppo_grad_torch(object.__new__(cls))
