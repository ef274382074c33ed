"""CPU tests of the return targets with per-group discounts (sg_returns_config_init / sg_gae_groups_device / sg_vtrace_device): the
declarations and the struct layout, the Python argument checks of gae_groups_torch / vtrace_torch with the native calls stubbed (nothing
reaches a kernel), the NumPy models (tests/returns_model.py) against independent formulations, the inputs of the GPU cases, and the
resources of the new kernels in the gfx950 build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import engine_asm
from gae_model import gae_model, synthetic
from returns_model import CASES, STAGE_ROWS, gae_groups_model, returns_case, vtrace_model, vtrace_model_f64
from test_episode_stats import _fake_cuda, _stub_env
from test_gae import _struct_fields
from test_snapshot_device import _header_args

HEAD = ["sg_env *env", "int32_t n_steps", "const sg_returns_config *cfg", "const float *reward_dev", "const uint8_t *done_dev",
        "const uint8_t *truncated_dev", "const float *value_dev", "const float *last_value_dev"]
TERMINAL = ["const float *terminal_value_dense_dev", "const sg_value_list *terminal_value_list"]
FIELDS = [("struct_size", "uint32_t", C.c_uint32), ("groups", "int32_t", C.c_int32), ("discounts", "const float", C.c_void_p),
          ("gamma", "double", C.c_double), ("lambda", "double", C.c_double), ("bootstrap_truncated", "int32_t", C.c_int32),
          ("rho_bar", "double", C.c_double), ("c_bar", "double", C.c_double), ("pg_rho_bar", "double", C.c_double),
          ("reserved", "int32_t", C.c_int32)]


def test_entry_points_and_the_struct_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_gae_groups_device") == HEAD + TERMINAL + ["float *advantage_dev", "float *ret_dev", "void *hip_stream"]
    assert _header_args("sg_vtrace_device") == HEAD + ["const float *ratio_dev"] + TERMINAL + ["float *vs_dev", "float *pg_advantage_dev",
                                                                                                "void *hip_stream"]
    assert _header_args("sg_returns_config_init", "void") == ["sg_returns_config *cfg"]
    vp, cfg, vl = C.c_void_p, C.POINTER(_native.SgReturnsConfig), C.POINTER(_native.SgValueList)
    assert _native.SYMBOLS["sg_gae_groups_device"] == (C.c_int, [vp, C.c_int32, cfg, vp, vp, vp, vp, vp, vp, vl, vp, vp, vp])
    assert _native.SYMBOLS["sg_vtrace_device"] == (C.c_int, [vp, C.c_int32, cfg, vp, vp, vp, vp, vp, vp, vp, vl, vp, vp, vp])
    assert _native.SYMBOLS["sg_returns_config_init"] == (None, [cfg])
    # the ctypes mirror: the header's fields in the header's order, field by field
    decls = _struct_fields("sg_returns_config")
    assert len(decls) == len(FIELDS) == len(_native.SgReturnsConfig._fields_)
    for d, (name, ctype_name, ctype), (pname, ptype) in zip(decls, FIELDS, _native.SgReturnsConfig._fields_):
        assert d.split()[-1].lstrip("*") == name == pname.rstrip("_"), d
        assert d.startswith(ctype_name) and ("*" in d) == (ctype is C.c_void_p) and ptype is ctype, d
    assert C.sizeof(_native.SgReturnsConfig) == 72
    assert [(f, getattr(_native.SgReturnsConfig, f).offset) for f, _ in _native.SgReturnsConfig._fields_] == [
        ("struct_size", 0), ("groups", 4), ("discounts", 8), ("gamma", 16), ("lambda_", 24), ("bootstrap_truncated", 32), ("rho_bar", 40),
        ("c_bar", 48), ("pg_rho_bar", 56), ("reserved", 64)]


def test_the_kernels_file_is_built_and_included_after_the_gae_kernels_and_the_defaults_are_the_issue_s():
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_returns.inc" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "sg_returns.inc"))
    assert 0 < src.index('#include "sg_gae.inc"') < src.index('#include "sg_returns.inc"')
    init = engine_asm.function_body(src, 'extern "C" void sg_returns_config_init(sg_returns_config *cfg)')
    for line in ("cfg->gamma = 0.99;", "cfg->lambda = 0.95;", "cfg->bootstrap_truncated = 1;", "cfg->rho_bar = cfg->c_bar = cfg->pg_rho_bar = 1.0;",
                 "std::memset(cfg, 0, sizeof(*cfg));"):
        assert line in init, line
    inc = open(os.path.join(build.CSRC, "sg_returns.inc")).read()
    # one statement of the GAE arithmetic: the grouped kernel calls sg_gae.inc's device functions, and no kernel here calls exp
    body = engine_asm.function_body(inc, "void discounted_gae_kernel(")
    assert all(f in body for f in ("gae_load_raw<HAS_V>", "gae_load_terminal(", "gae_compute<HAS_V, HAS_TV>"))
    assert not re.search(r"\bexp\w*\(", inc)
    rows = (int(re.search(r"constexpr int kGaeRows = (\d+);", open(os.path.join(build.CSRC, "sg_gae.inc")).read()).group(1)),
            int(re.search(r"constexpr int kVtraceRows = (\d+);", inc).group(1)))
    assert rows == STAGE_ROWS  # (what the stage boundaries of the GPU cases are worked out from)


# ---------------------------------------------------------------------------------------------- the Python front end
K, B = 5, 8


def _args(**over):
    import torch
    a = dict(reward=torch.zeros((K, B)), done=torch.zeros((K, B), dtype=torch.uint8), trunc=torch.zeros((K, B), dtype=torch.uint8),
             value=torch.zeros((K, B)), last_value=torch.zeros(B), terminal_value=torch.zeros((K, B)), discounts=torch.zeros((4, 2)))
    a = {k: _fake_cuda(v) for k, v in a.items()}
    a.update(over)
    return a


def _out(*names):
    import torch
    return {n: _fake_cuda(torch.zeros((K, B))) for n in names}


def _list(cap=16, **over):
    import torch
    t = dict(count=torch.zeros(1, dtype=torch.int32), step_env=torch.zeros((cap, 2), dtype=torch.int32), value=torch.zeros(cap))
    t.update(over)
    return {k: _fake_cuda(v) for k, v in t.items()}


@pytest.mark.parametrize("form", ["dense", "list", "none"])
def test_gae_groups_torch_arguments_reach_the_native_call_in_order(form):
    env = _stub_env(B=B)
    a = _args(out=_out("advantage", "returns"))
    term = _list() if form == "list" else None
    if form != "dense":
        a["terminal_value"] = None
    adv, ret = env.gae_groups_torch(terminal=term, bootstrap_truncated=False, **a)
    assert env._lib.names() == ["sg_gae_groups_device"]
    args = env._lib.calls[-1][1]
    assert len(args) == 13 and args[1] == K
    cfg = args[2]._obj
    assert (cfg.struct_size, cfg.groups, cfg.discounts, cfg.bootstrap_truncated, cfg.reserved) == (72, 4, a["discounts"].data_ptr(), 0, 0)
    for k, name in ((3, "reward"), (4, "done"), (5, "trunc"), (6, "value"), (7, "last_value")):
        assert args[k].value == a[name].data_ptr(), name
    assert (args[8].value == a["terminal_value"].data_ptr()) if form == "dense" else args[8] is None
    if form == "list":
        vl = args[9]._obj
        assert (vl.count, vl.step_env, vl.value, vl.capacity) == (term["count"].data_ptr(), term["step_env"].data_ptr(), term["value"].data_ptr(), 16)
    else:
        assert args[9] is None
    assert args[10].value == a["out"]["advantage"].data_ptr() and args[11].value == a["out"]["returns"].data_ptr()
    assert adv is a["out"]["advantage"] and ret is a["out"]["returns"]


@pytest.mark.parametrize("table", [True, False])
def test_vtrace_torch_arguments_reach_the_native_call_in_order(table):
    import torch
    env = _stub_env(B=B)
    a = _args(out=_out("vs", "pg_advantage"), ratio=_fake_cuda(torch.ones((K, B))))
    if not table:
        a["discounts"] = None
    vs, pg = env.vtrace_torch(gamma=0.9, lam=0.8, rho_bar=2.0, c_bar=float("inf"), pg_rho_bar=0.5, **a)
    assert env._lib.names() == ["sg_vtrace_device"]
    args = env._lib.calls[-1][1]
    assert len(args) == 14 and args[1] == K
    cfg = args[2]._obj
    assert (cfg.struct_size, cfg.bootstrap_truncated, cfg.rho_bar, cfg.c_bar, cfg.pg_rho_bar, cfg.reserved) == (72, 1, 2.0, float("inf"), 0.5, 0)
    if table:
        assert (cfg.groups, cfg.discounts) == (4, a["discounts"].data_ptr())
    else:
        assert (cfg.groups, cfg.discounts, cfg.gamma, cfg.lambda_) == (0, None, 0.9, 0.8)
    for k, name in ((3, "reward"), (4, "done"), (5, "trunc"), (6, "value"), (7, "last_value"), (8, "ratio"), (9, "terminal_value")):
        assert args[k].value == a[name].data_ptr(), name
    assert args[10] is None
    assert args[11].value == a["out"]["vs"].data_ptr() and args[12].value == a["out"]["pg_advantage"].data_ptr()
    assert vs is a["out"]["vs"] and pg is a["out"]["pg_advantage"]


def test_vtrace_torch_defaults_and_optional_arguments():
    env = _stub_env(B=B)
    a = _args(last_value=None, terminal_value=None, discounts=None, out=_out("vs", "pg_advantage"))
    env.vtrace_torch(rho_bar=3.0, **a)
    args = env._lib.calls[-1][1]
    assert args[7] is None and args[8] is None and args[9] is None and args[10] is None
    cfg = args[2]._obj
    assert (cfg.gamma, cfg.lambda_, cfg.rho_bar, cfg.c_bar, cfg.pg_rho_bar, cfg.bootstrap_truncated) == (0.99, 1.0, 3.0, 1.0, 3.0, 1)  # pg_rho_bar: rho_bar
    env.vtrace_torch(terminal=_list(), **a)
    assert env._lib.calls[-1][1][10]._obj.capacity == 16


def _bad_shared():
    import torch
    z = torch.zeros
    return {
        "reward dtype": dict(reward=_fake_cuda(z((K, B), dtype=torch.float64))),
        "reward shape": dict(reward=_fake_cuda(z((K, B + 1)))),
        "reward 1d": dict(reward=_fake_cuda(z(B))),
        "reward host": dict(reward=z((K, B))),
        "reward stride": dict(reward=_fake_cuda(z((K, 2 * B))[:, ::2])),
        "done dtype": dict(done=_fake_cuda(z((K, B), dtype=torch.bool))),
        "trunc shape": dict(trunc=_fake_cuda(z((K - 1, B), dtype=torch.uint8))),
        "value dtype": dict(value=_fake_cuda(z((K, B), dtype=torch.float16))),
        "value host": dict(value=z((K, B))),
        "last_value shape": dict(last_value=_fake_cuda(z((1, B)))),
        "terminal_value stride": dict(terminal_value=_fake_cuda(z((K, 2 * B))[:, ::2])),
        "terminal both": dict(terminal=_list()),
        "count dtype": dict(terminal_value=None, terminal=_list(count=z(1, dtype=torch.int64))),
        "step_env shape": dict(terminal_value=None, terminal=_list(step_env=z((16, 3), dtype=torch.int32))),
        "value length": dict(terminal_value=None, terminal=_list(value=z(15))),
        "discounts dtype": dict(discounts=_fake_cuda(z((4, 2), dtype=torch.float64))),
        "discounts shape": dict(discounts=_fake_cuda(z((4, 3)))),
        "discounts 1d": dict(discounts=_fake_cuda(z(8))),
        "discounts host": dict(discounts=z((4, 2))),
        "discounts stride": dict(discounts=_fake_cuda(z((4, 4))[:, ::2])),
        "discounts divide": dict(discounts=_fake_cuda(z((3, 2)))),
        "discounts rows": dict(discounts=_fake_cuda(z((0, 2)))),
        "discounts many": dict(discounts=_fake_cuda(z((2 * B, 2)))),
    }


def _bad_gae_groups():
    import torch
    z = torch.zeros
    return {**_bad_shared(),
            "discounts none": dict(discounts=None),
            "advantage dtype": dict(out=dict(advantage=_fake_cuda(z((K, B), dtype=torch.float64)), returns=_fake_cuda(z((K, B))))),
            "returns shape": dict(out=dict(advantage=_fake_cuda(z((K, B))), returns=_fake_cuda(z((K, 1)))))}


def _bad_vtrace():
    import torch
    z = torch.zeros
    nan = float("nan")
    return {**_bad_shared(),
            "value none": dict(value=None),
            "ratio dtype": dict(ratio=_fake_cuda(z((K, B), dtype=torch.float64))),
            "ratio shape": dict(ratio=_fake_cuda(z((K, B - 1)))),
            "ratio host": dict(ratio=z((K, B))),
            "vs shape": dict(out=dict(vs=_fake_cuda(z((K + 1, B))), pg_advantage=_fake_cuda(z((K, B))))),
            "pg_advantage host": dict(out=dict(vs=_fake_cuda(z((K, B))), pg_advantage=z((K, B)))),
            "gamma high": dict(discounts=None, gamma=1.5), "gamma nan": dict(discounts=None, gamma=nan),
            "lam negative": dict(discounts=None, lam=-1.0), "lam nan": dict(discounts=None, lam=nan),
            "rho_bar zero": dict(rho_bar=0.0), "rho_bar nan": dict(rho_bar=nan), "rho_bar negative": dict(rho_bar=-1.0),
            "c_bar zero": dict(c_bar=0.0), "c_bar nan": dict(c_bar=nan),
            "pg_rho_bar negative": dict(pg_rho_bar=-2.0), "pg_rho_bar nan": dict(pg_rho_bar=nan)}


@pytest.mark.parametrize("bad", sorted(_bad_gae_groups()))
def test_gae_groups_torch_refuses_bad_arguments_before_any_native_call(bad):
    env = _stub_env(B=B)
    a = _args(**_bad_gae_groups()[bad])
    with pytest.raises(ValueError, match=bad.split()[0]):
        env.gae_groups_torch(**a)
    assert env._lib.calls == []


@pytest.mark.parametrize("bad", sorted(_bad_vtrace()))
def test_vtrace_torch_refuses_bad_arguments_before_any_native_call(bad):
    env = _stub_env(B=B)
    a = _args(**_bad_vtrace()[bad])
    with pytest.raises(ValueError, match=bad.split()[0]):
        env.vtrace_torch(**a)
    assert env._lib.calls == []


# ---------------------------------------------------------------------------------------------- the models
def _paper_sum(s, ratio, gamma, lam, rho_bar, c_bar):
    """Equation (1) of Espeholt et al. 2018, summed explicitly in float64 per env and episode segment (a segment ends at a done step or
    at the last step): v_s = V(x_s) + sum_{t >= s} gamma^(t-s) (prod_{s <= i < t} c_i) rho_t (r_t + gamma V(x_{t+1}) - V(x_t)), with
    c_i = lam min(c_bar, ratio_i), rho_t = min(rho_bar, ratio_t)."""
    K, B = s["reward"].shape
    done, trunc = s["done"].astype(bool), s["trunc"].astype(bool)
    r, v, tv = s["reward"].astype(np.float64), s["value"].astype(np.float64), s["terminal_value"].astype(np.float64)
    rho, c = np.minimum(rho_bar, ratio.astype(np.float64)), lam * np.minimum(c_bar, ratio.astype(np.float64))
    vs = np.zeros((K, B))
    for i in range(B):
        nv = np.array([(tv[t, i] if trunc[t, i] else 0.0) if done[t, i] else (v[t + 1, i] if t + 1 < K else float(s["last_value"][i]))
                       for t in range(K)])
        dV = rho[:, i] * (r[:, i] + gamma * nv - v[:, i])
        start = 0
        for end in [t for t in range(K) if done[t, i] or t == K - 1]:
            for t0 in range(start, end + 1):
                w = np.concatenate([[1.0], np.cumprod(c[t0:end, i])]) * gamma ** np.arange(end + 1 - t0)
                vs[t0, i] = v[t0, i] + np.sum(w * dV[t0:end + 1])
            start = end + 1
    return vs


@pytest.mark.parametrize("K", [9, 49])
def test_vtrace_model_equals_the_paper_s_explicit_sum(K):
    """within 1e-12 (1 + max|vs|): both add the same <= 49 float64 terms in different orders (the recurrence nests them); the
    re-association error of 49 terms is ~49 * 2^-53 ~ 5e-15 of the sum of their magnitudes.  pg_advantage is one more step of the same
    recurrence on vs[t + 1] (rp <= pg_rho_bar = 1 here, gamma <= 1), so it gets the same bound."""
    s, _, ratio = returns_case(K, 65, 1, seed=31 + K)
    for gamma, lam, rho_bar, c_bar in ((0.99, 1.0, 1.0, 1.0), (0.97, 0.9, 2.0, 0.7), (1.0, 1.0, np.inf, np.inf)):
        vs, pg = vtrace_model_f64(**s, ratio=ratio, gamma=gamma, lam=lam, rho_bar=rho_bar, c_bar=c_bar, pg_rho_bar=1.0)
        want = _paper_sum(s, ratio, gamma, lam, rho_bar, c_bar)
        bound = 1e-12 * (1.0 + np.abs(want).max())
        assert np.abs(vs - want).max() <= bound, (gamma, lam, np.abs(vs - want).max(), bound)
        done, trunc = s["done"].astype(bool), s["trunc"].astype(bool)
        nxt = np.concatenate([want[1:], s["last_value"].astype(np.float64)[None]])
        nxt = np.where(done, np.where(trunc, s["terminal_value"].astype(np.float64), 0.0), nxt)
        want_pg = np.minimum(1.0, ratio.astype(np.float64)) * (s["reward"].astype(np.float64) + gamma * nxt - s["value"].astype(np.float64))
        assert np.abs(pg - want_pg).max() <= bound, (gamma, lam, np.abs(pg - want_pg).max(), bound)


def test_on_policy_vtrace_is_gae_s_return_bit_for_bit():
    """ratio None (or all ones) and the three bars >= 1: rc = cc = 1, so delta and gl are GAE's and acc is GAE's A -- already in float64"""
    from gae_model import gae_model_f64
    s, _, _ = returns_case(49, 65, 1, seed=5)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
        for bars in ((1.0, 1.0, 1.0), (np.inf, 2.0, 1.5)):
            for ratio in (None, np.ones((49, 65), np.float32)):
                for kw in (dict(), dict(bootstrap_truncated=False), dict(terminal_value=None), dict(last_value=None)):
                    a = {**s, **kw}
                    A, R = gae_model_f64(gamma=gamma, lam=lam, **a)
                    vs, pg = vtrace_model_f64(ratio=ratio, gamma=gamma, lam=lam, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2], **a)
                    assert np.array_equal(vs, R), (gamma, lam, bars, kw)
    # at lambda = 1 the on-policy pg_advantage is GAE's advantage up to re-association: (r + gamma (v' + A')) - v against (r + gamma v' - v) + gamma A'
    A, _ = gae_model_f64(gamma=0.99, lam=1.0, **s)
    _, pg = vtrace_model_f64(gamma=0.99, lam=1.0, **s)
    assert np.abs(pg - A).max() <= 1e-12 * (1.0 + np.abs(A).max())


def test_a_clipped_ratio_and_a_nan_ratio():
    s, _, ratio = returns_case(17, 65, 1, seed=6)
    # bars far above every ratio: the unclipped importance weights; a bar below every ratio: the bar itself
    big, _ = vtrace_model(**s, ratio=ratio, rho_bar=1e9, c_bar=1e9)
    inf, _ = vtrace_model(**s, ratio=ratio, rho_bar=np.inf, c_bar=np.inf)
    assert np.array_equal(big, inf)
    low = np.float32(ratio.min() / 2)
    a, _ = vtrace_model(**s, ratio=ratio, rho_bar=low, c_bar=low)
    b, _ = vtrace_model(**s, ratio=np.full_like(ratio, low), rho_bar=np.inf, c_bar=np.inf)
    assert np.array_equal(a, b)
    # a NaN ratio stays NaN (it is not clipped to the bar) and stays inside its episode and env
    t0, i0 = 9, 11
    bad = ratio.copy()
    bad[t0, i0] = np.nan
    base, base_pg = vtrace_model(**s, ratio=ratio)
    got, got_pg = vtrace_model(**s, ratio=bad)
    done = s["done"].astype(bool)[:, i0]
    first = max([t + 1 for t in range(t0) if done[t]], default=0)
    inside = np.zeros((17, 65), bool)
    inside[first:t0 + 1, i0] = True
    assert np.isnan(got[inside]).all() and np.array_equal(got[~inside], base[~inside])
    assert np.isnan(got_pg[t0, i0]) and np.array_equal(got_pg[~inside], base_pg[~inside])


def test_grouped_model_with_equal_rows_is_the_gae_model_bit_for_bit():
    s = synthetic(25, 240, seed=7, p_done=0.1)
    g, l = np.float32(0.97), np.float32(0.93)
    for G in (1, 3, 240):
        table = np.tile(np.array([[g, l]], np.float32), (G, 1))
        for kw in (dict(), dict(value=None, last_value=None), dict(bootstrap_truncated=False), dict(terminal_value=None)):
            a = {**s, **kw}
            got = gae_groups_model(a.pop("reward"), a.pop("done"), a.pop("trunc"), table, **a)
            want = gae_model(gamma=float(g), lam=float(l), **{**s, **kw})
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (G, kw)
    # the table form's gl, (double) g * (double) l, is exact: rounding it changes nothing
    assert np.float64(g) * np.float64(l) == float(g) * float(l)
    # distinct rows: each block is the scalar model on that block, and the V-trace model reads the same rows
    s, table, _ = returns_case(25, 240, 3)
    adv, ret = gae_groups_model(s["reward"], s["done"], s["trunc"], table, s["value"], s["last_value"], s["terminal_value"])
    vs, _ = vtrace_model(**s, discounts=table)
    assert np.array_equal(vs, ret)
    for k in range(3):
        c = slice(80 * k, 80 * k + 80)
        want = gae_model(gamma=float(table[k, 0]), lam=float(table[k, 1]), **{n: v[..., c] for n, v in s.items()})
        assert np.array_equal(adv[:, c], want[0]) and np.array_equal(ret[:, c], want[1])


@pytest.mark.parametrize("K,B,G", CASES)
def test_the_inputs_of_every_gpu_case_exercise_what_the_case_is_for(K, B, G):
    """Built with the generator and seed of tests/test_gpu_returns.py.  Where the shape admits it -- two kinds of done step need two
    steps (every shape but K = B = 1), a stage boundary needs a second stage (K > 8 in the GAE kernel, K > 6 in the V-trace kernel) -- the inputs hold a done-and-truncated step, a
    done-not-truncated step, and an env that is not done at the first row of a later stage, so that the carried A, acc and v_next cross
    the boundary.  With more than one group the rows are distinct and moving every row by one group changes more than half of every
    output, so a wrong group index cannot pass."""
    s, table, ratio = returns_case(K, B, G)
    done, trunc = s["done"].astype(bool), s["trunc"].astype(bool)
    assert table.shape == (G, 2) and table.dtype == np.float32 and ratio.shape == (K, B) and ratio.dtype == np.float32
    assert (table[:, 0] >= 0.9).all() and (table[:, 0] <= 0.999).all() and (table[:, 1] >= 0.8).all() and (table[:, 1] <= 1.0).all()
    if K * B >= 2:
        assert (done & trunc).any() and (done & ~trunc).any()
    if K * B >= 64:
        assert 0.3 < (ratio > 1.0).mean() < 0.7
    for rows in STAGE_ROWS:
        boundaries = [K - 1 - rows * c for c in range(1, (K + rows - 1) // rows)]
        assert (len(boundaries) > 0) == (K > rows)
        if boundaries:
            assert (~done[boundaries]).any()
    if G > 1:
        assert len({tuple(r) for r in table.tolist()}) == G and len(set(table[:, 0].tolist())) == G and len(set(table[:, 1].tolist())) == G
        moved = np.roll(table, 1, axis=0)
        a = (s["reward"], s["done"], s["trunc"])
        rest = dict(value=s["value"], last_value=s["last_value"], terminal_value=s["terminal_value"])
        for model, kw in ((gae_groups_model, {}), (lambda *x, **k: vtrace_model(*x[:3], discounts=x[3], **k), dict(ratio=ratio))):
            for got, other in zip(model(*a, table, **rest, **kw), model(*a, moved, **rest, **kw)):
                assert (got != other).mean() > 0.5, (model, (got != other).mean())


# ---------------------------------------------------------------------------------------------- the build
NEW = r"\S*(?:discounted_gae_kernel|vtrace_kernel)\S*"


def test_the_new_kernels_build_for_gfx950_without_scratch_lds_or_spills():
    """build() makes the library with the entry points and the kernels.  In the code object discounted_gae_kernel<value?, terminal?> x 4
    and vtrace_kernel<terminal?, table?> x 4 use no scratch, need no LDS and spill neither vector nor scalar registers; every
    instruction of theirs that writes memory is a global_store_dword of one element and no float64 operation is fused; and the four
    instantiations of gae_scan_kernel still report what tests/test_gae.py pins (the new file is included after them and shares their
    device functions)."""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    for name in (b"sg_returns_config_init", b"sg_gae_groups_device", b"sg_vtrace_device", b"discounted_gae_kernel", b"vtrace_kernel"):
        assert name in lib
    kernels = engine_asm.descriptors(NEW)
    assert len([k for k, _ in kernels if "discounted_gae_kernel" in k]) == 4 and len([k for k, _ in kernels if "vtrace_kernel" in k]) == 4
    assert len(kernels) == 8, [k for k, _ in kernels]
    for name, field in kernels:
        assert "gae_scan_kernel" not in name and "gae_scatter_kernel" not in name
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == 0, name
    spills = engine_asm.spill_counts(NEW)  # (vector registers, as tests/test_gae.py counts them: nothing goes to memory)
    assert len(spills) == 8 and all(n == 0 for _, n in spills), spills
    for name, _ in kernels:
        fn = engine_asm.function(name)
        writes = re.findall(r"^\s+(\w*(?:store|atomic)\w*)\s", fn, flags=re.M)
        assert writes and all(w == "global_store_dword" for w in writes), (name, sorted(set(writes)))
        loads = re.findall(r"^\s+(global_load_\w+)\s", fn, flags=re.M)
        assert set(loads) <= {"global_load_dword", "global_load_ubyte", "global_load_dwordx2"}, (name, set(loads))
        # one element per lane everywhere but the lane's table row, (gamma, lambda), which may be read as a pair, once
        table = "discounted_gae_kernel" in name or name.startswith("_Z13vtrace_kernelILb0ELb1E") or name.startswith("_Z13vtrace_kernelILb1ELb1E")
        assert loads.count("global_load_dwordx2") <= (1 if table else 0), name
        assert not re.search(r"\bv_fma_f64\b", fn), name  # every float64 operation rounds on its own
        assert not re.search(r"\bscratch_", fn), name
    scan = engine_asm.descriptors(r"\S*gae_scan_kernel\S*")
    assert len(scan) == 4
    for name, field in scan:
        assert field["private_segment_fixed_size"] == 0 and field["group_segment_fixed_size"] == 0 and field["next_free_vgpr"] <= 128, name
    assert all(n == 0 for _, n in engine_asm.spill_counts(r"\S*gae_scan_kernel\S*"))
