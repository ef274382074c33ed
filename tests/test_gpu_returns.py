"""GPU tests of gae_groups_torch / vtrace_torch (sg_gae_groups_device / sg_vtrace_device) against the NumPy models of
tests/returns_model.py and against gae_torch.  "Equal" is bitwise: the same float32 bit patterns, and NaN exactly where the model has NaN.
The shapes are returns_model.CASES; tests/test_returns.py checks on the CPU that their inputs exercise what each case is for."""
import ctypes as C

import numpy as np
import pytest

from gae_model import gae_model
from returns_model import CASES, gae_groups_model, group_columns, returns_case, vtrace_model
from test_gpu_gae import ENV_ID, _dev, _equal, _list_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def envs():
    """one handle per batch size for the whole module (the result depends on the arguments only: the handle gives B)"""
    import space_gym_amd as sg
    made = {}

    def get(B):
        if B not in made:
            made[B] = sg.make_vec(ENV_ID, B, device=0)
        return made[B]
    yield get
    for env in made.values():
        env.check_status()
        env.close()


def _nan_out(K, B, *names):
    import torch
    return {n: torch.full((K, B), float("nan"), device="cuda") for n in names}


def _host(pair):
    import torch
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in pair)


def _term(s, seed=0, extra_capacity=5):
    import torch
    n, step_env, value = _list_of(s, np.random.default_rng(seed), extra_capacity)
    return dict(count=torch.tensor([n], dtype=torch.int32, device="cuda"), step_env=_dev(step_env), value=_dev(value))


def _gae_groups(env, s, table, terminal=None, **kw):
    """the call on inputs given as NumPy arrays (None: left out), into NaN-prefilled outputs"""
    K, B = s["reward"].shape
    t = {k: _dev(v) for k, v in s.items() if v is not None}
    got = env.gae_groups_torch(t["reward"], t["done"], t["trunc"], table if hasattr(table, "data_ptr") else _dev(table), value=t.get("value"),
                               last_value=t.get("last_value"), terminal_value=None if terminal is not None else t.get("terminal_value"),
                               terminal=terminal, out=_nan_out(K, B, "advantage", "returns"), **kw)
    return _host(got)


def _vtrace(env, s, ratio=None, table=None, terminal=None, **kw):
    K, B = s["reward"].shape
    t = {k: _dev(v) for k, v in s.items() if v is not None}
    got = env.vtrace_torch(t["reward"], t["done"], t["trunc"], t["value"], last_value=t.get("last_value"),
                           ratio=None if ratio is None else _dev(ratio), terminal_value=None if terminal is not None else t.get("terminal_value"),
                           terminal=terminal, discounts=None if table is None else _dev(table), out=_nan_out(K, B, "vs", "pg_advantage"), **kw)
    return _host(got)


def _same(got, want, what):
    for g, w, k in zip(got, want, (0, 1)):
        assert _equal(g, w), (what, k, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


def _gae_groups_want(s, table, **kw):
    return gae_groups_model(s["reward"], s["done"], s["trunc"], table, s.get("value"), s.get("last_value"), s.get("terminal_value"), **kw)


@pytest.mark.parametrize("K,B,G", CASES)
def test_both_calls_equal_the_model(envs, K, B, G):
    """1: with and without value (GAE), last_value and ratio; dense, list and no terminal values; bootstrap_truncated off; V-trace with
    the table and with scalar discounts, bars below, at and above the ratios; 5: the list form equals the dense form"""
    env = envs(B)
    s, table, ratio = returns_case(K, B, G)
    no_tv, bare = {**s, "terminal_value": None}, {**s, "value": None, "last_value": None}
    dense = _gae_groups(env, s, table)
    _same(dense, _gae_groups_want(s, table), "gae dense")
    _same(_gae_groups(env, s, table, terminal=_term(s, K)), dense, "gae list")
    _same(_gae_groups(env, no_tv, table), _gae_groups_want(no_tv, table), "gae no terminal")
    _same(_gae_groups(env, bare, table), _gae_groups_want(bare, table), "gae no value")
    _same(_gae_groups(env, {**bare, "terminal_value": None}, table), _gae_groups_want({**bare, "terminal_value": None}, table), "gae rewards only")
    off = _gae_groups(env, s, table, bootstrap_truncated=False)
    _same(off, _gae_groups_want(s, table, bootstrap_truncated=False), "gae bootstrap off")
    _same(_gae_groups(env, s, table, terminal=_term(s, K), bootstrap_truncated=False), off, "gae bootstrap off, list")
    bars = dict(rho_bar=1.0, c_bar=0.9, pg_rho_bar=1.5)
    dense = _vtrace(env, s, ratio, table, **bars)
    _same(dense, vtrace_model(**s, ratio=ratio, discounts=table, **bars), "vtrace dense")
    _same(_vtrace(env, s, ratio, table, terminal=_term(s, K + 1), **bars), dense, "vtrace list")
    _same(_vtrace(env, no_tv, ratio, table), vtrace_model(**no_tv, ratio=ratio, discounts=table), "vtrace no terminal")
    _same(_vtrace(env, {**s, "last_value": None}, None, table), vtrace_model(**{**s, "last_value": None}, discounts=table), "vtrace on-policy")
    _same(_vtrace(env, s, ratio, table, bootstrap_truncated=False, rho_bar=float("inf"), c_bar=float("inf")),
          vtrace_model(**s, ratio=ratio, discounts=table, bootstrap_truncated=False, rho_bar=np.inf, c_bar=np.inf), "vtrace bootstrap off, no clip")
    for kw in (dict(gamma=0.97, lam=0.9, rho_bar=2.0, c_bar=0.5), dict()):
        _same(_vtrace(env, s, ratio, None, **kw), vtrace_model(**s, ratio=ratio, **kw), ("vtrace scalar", kw))
    _same(_vtrace(env, no_tv, None, None, gamma=1.0, lam=1.0), vtrace_model(**no_tv, gamma=1.0, lam=1.0), "vtrace scalar on-policy")
    env.check_status()


@pytest.mark.parametrize("K,B,G", [c for c in CASES if c[0] in (9, 49)])
def test_equal_rows_and_on_policy_vtrace_equal_gae_torch(envs, K, B, G):
    """2: equal rows give gae_torch at gamma = float(float32), lam likewise; 4: V-trace on-policy gives gae_torch's returns (the table
    form through equal rows; the scalar form directly, bars at and above 1)"""
    env = envs(B)
    s, _, _ = returns_case(K, B, G)
    g, l = np.float32(0.987), np.float32(0.913)
    table = np.tile(np.array([[g, l]], np.float32), (G, 1))
    t = {k: _dev(v) for k, v in s.items()}
    want = _host(env.gae_torch(t["reward"], t["done"], t["trunc"], value=t["value"], last_value=t["last_value"],
                               terminal_value=t["terminal_value"], gamma=float(g), lam=float(l)))
    _same(_gae_groups(env, s, table), want, "table")
    assert _equal(_vtrace(env, s, None, table)[0], want[1])
    assert _equal(_vtrace(env, s, None, None, gamma=float(g), lam=float(l), rho_bar=float("inf"), c_bar=3.0)[0], want[1])
    assert _equal(_vtrace(env, s, np.ones((K, B), np.float32), None, gamma=float(g), lam=float(l))[0], want[1])


@pytest.mark.parametrize("K", [9, 49])
def test_each_block_equals_gae_torch_on_a_handle_of_that_block(envs, K):
    """3: G = 3, B = 240: each block of 80 equals gae_torch on a second handle of 80 envs, fed contiguous copies of the block"""
    s, table, _ = returns_case(K, 240, 3)
    adv, ret = _gae_groups(envs(240), s, table)
    small = envs(80)
    for g, cols in enumerate(group_columns(240, 3)):
        t = {k: _dev(np.ascontiguousarray(v[..., cols])) for k, v in s.items()}
        want = _host(small.gae_torch(t["reward"], t["done"], t["trunc"], value=t["value"], last_value=t["last_value"],
                                     terminal_value=t["terminal_value"], gamma=float(table[g, 0]), lam=float(table[g, 1])))
        _same((np.ascontiguousarray(adv[:, cols]), np.ascontiguousarray(ret[:, cols])), want, g)


@pytest.mark.parametrize("call", ["gae_groups", "vtrace"])
def test_a_list_with_count_past_capacity_sets_the_status_word(call):
    """5: the scatter launch is sg_gae_device's, and so is its report"""
    import torch
    import space_gym_amd as sg
    from space_gym_amd._native import NativeError
    K, B, G = 17, 65, 5
    env = sg.make_vec(ENV_ID, B, device=0)
    s, table, ratio = returns_case(K, B, G)
    n, se, val = _list_of(s, np.random.default_rng(0), extra_capacity=0)
    term = dict(count=torch.tensor([n], dtype=torch.int32, device="cuda"), step_env=_dev(se[:n - 2]), value=_dev(val[:n - 2]))
    if call == "gae_groups":
        _gae_groups(env, s, table, terminal=term)
    else:
        _vtrace(env, s, ratio, table, terminal=term)
    with pytest.raises(NativeError, match="a value list with count > capacity"):
        env.check_status()
    env.check_status()  # reported once; the handle works afterwards
    _same(_gae_groups(env, s, table), _gae_groups_want(s, table), "afterwards")
    env.check_status()
    env.close()


def _episode(s, t0, i0):
    done = s["done"].astype(bool)[:, i0]
    first = max([t + 1 for t in range(t0) if done[t]], default=0)
    inside = np.zeros(s["done"].shape, bool)
    inside[first:t0 + 1, i0] = True
    return inside


def test_a_nan_reward_stays_inside_its_episode(envs):
    """6a: in both calls, outputs of the NaN's episode at and before its step are NaN; every other element keeps its bits"""
    K, B, G = 49, 240, 3
    env = envs(B)
    s, table, ratio = returns_case(K, B, G)
    t0 = 30
    i0 = next(i for i in range(B) if s["done"][:t0, i].any() and not s["done"][t0, i] and s["done"][t0 + 1:, i].any())
    inside = _episode(s, t0, i0)
    bad = {k: v.copy() for k, v in s.items()}
    bad["reward"][t0, i0] = np.nan
    for run, model in ((lambda x: _gae_groups(env, x, table), lambda x: _gae_groups_want(x, table)),
                       (lambda x: _vtrace(env, x, ratio, table), lambda x: vtrace_model(**x, ratio=ratio, discounts=table))):
        base, got = run(s), run(bad)
        _same(got, model(bad), "nan")
        for g, b in zip(got, base):  # (pg_advantage[t] reads vs[t + 1] of its own episode only: a done step reads the terminal value)
            assert np.isnan(g[inside]).all() and not np.isnan(g[~inside]).any()
            assert np.array_equal(g.view(np.uint32)[~inside], b.view(np.uint32)[~inside])


@pytest.mark.parametrize("row", [(np.nan, 0.9), (0.95, np.nan), (1.5, 0.9), (0.95, -2.0), (np.inf, 1.0)])
def test_a_bad_table_row_changes_that_group_s_columns_only(envs, row):
    """6b: the table is not checked on the device; a NaN or out-of-range row reaches the envs of its group and no other (and the kernel
    still does what the model does with it)"""
    K, B, G = 25, 240, 3
    env = envs(B)
    s, table, ratio = returns_case(K, B, G)
    bad = table.copy()
    bad[1] = row
    own = np.zeros(B, bool)
    own[group_columns(B, G)[1]] = True
    with np.errstate(all="ignore"):
        for run, model in ((lambda tb: _gae_groups(env, s, tb), lambda tb: _gae_groups_want(s, tb)),
                           (lambda tb: _vtrace(env, s, ratio, tb), lambda tb: vtrace_model(**s, ratio=ratio, discounts=tb))):
            base, got = run(table), run(bad)
            _same(got, model(bad), row)
            for b, g in zip(base, got):
                assert np.array_equal(b.view(np.uint32)[:, ~own], g.view(np.uint32)[:, ~own])
                assert (b.view(np.uint32)[:, own] != g.view(np.uint32)[:, own]).mean() > 0.5


def test_two_calls_give_the_same_bits(envs):
    """7: each call writes NaN-prefilled outputs of its own"""
    K, B, G = 49, 240, 240
    env = envs(B)
    s, table, ratio = returns_case(K, B, G)
    for form in ("dense", "list"):
        term = (lambda: _term(s, 3)) if form == "list" else (lambda: None)
        a, b = _gae_groups(env, s, table, terminal=term()), _gae_groups(env, s, table, terminal=term())
        _same(a, b, ("gae", form))
        assert not np.isnan(a[0]).any() and not np.isnan(a[1]).any()
        a, b = _vtrace(env, s, ratio, table, terminal=term()), _vtrace(env, s, ratio, table, terminal=term())
        _same(a, b, ("vtrace", form))
        assert not np.isnan(a[0]).any() and not np.isnan(a[1]).any()


@pytest.mark.parametrize("form", ["dense", "list"])
def test_a_captured_graph_reads_the_table_at_every_replay(form):
    """8: both calls captured once; the graph is replayed after new values were written into `discounts` (and nothing else changed)"""
    import torch
    import space_gym_amd as sg
    K, B, G = 25, 240, 3
    env = sg.make_vec(ENV_ID, B, device=0)
    s, table, ratio = returns_case(K, B, G)
    t = {k: _dev(v) for k, v in s.items()}
    d_ratio, d_table = _dev(ratio), _dev(table)
    gae_out, vt_out = _nan_out(K, B, "advantage", "returns"), _nan_out(K, B, "vs", "pg_advantage")
    kw = dict(terminal=_term(s, 1)) if form == "list" else dict(terminal_value=t["terminal_value"])

    def call():
        env.gae_groups_torch(t["reward"], t["done"], t["trunc"], d_table, value=t["value"], last_value=t["last_value"], out=gae_out, **kw)
        env.vtrace_torch(t["reward"], t["done"], t["trunc"], t["value"], last_value=t["last_value"], ratio=d_ratio, discounts=d_table,
                         out=vt_out, **kw)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    newer = np.stack([np.linspace(0.91, 0.99, G), np.linspace(1.0, 0.8, G)], 1).astype(np.float32)
    seen = []
    for values in (table, newer, table[::-1].copy()):
        d_table.copy_(torch.from_numpy(values))
        for out in (gae_out, vt_out):
            for x in out.values():
                x.fill_(float("nan"))
        g.replay()
        got = _host((gae_out["advantage"], gae_out["returns"], vt_out["vs"], vt_out["pg_advantage"]))
        _same(got[:2], _gae_groups_want(s, values), ("gae", form))
        _same(got[2:], vtrace_model(**s, ratio=ratio, discounts=values), ("vtrace", form))
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
    env.check_status()
    env.close()


def test_native_refusals_write_nothing(envs):
    """9: every refusal of the two C calls, into NaN-prefilled outputs; then the same arguments, accepted"""
    import torch
    from space_gym_amd import _native
    K, B, G = 9, 240, 3
    env = envs(B)
    s, table, ratio = returns_case(K, B, G)
    t = {k: _dev(v) for k, v in s.items()}
    d_ratio, d_table = _dev(ratio), _dev(table)
    out = _nan_out(K, B, "a", "b")
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    term = _term(s)
    vl = _native.SgValueList(term["count"].data_ptr(), term["step_env"].data_ptr(), term["value"].data_ptr(), int(term["value"].shape[0]))

    def cfg(**over):
        c = _native.SgReturnsConfig()
        env._lib.sg_returns_config_init(C.byref(c))
        c.groups, c.discounts = G, d_table.data_ptr()
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)

    def gae(c, n_steps=K, reward=t["reward"], adv=out["a"], dense=t["terminal_value"], lst=None):
        return env._lib.sg_gae_groups_device(env._h, n_steps, c, p(reward), p(t["done"]), p(t["trunc"]), p(t["value"]), p(t["last_value"]),
                                             p(dense), lst, p(adv), p(out["b"]), None)

    def vtrace(c, value=t["value"], pg=out["b"], dense=t["terminal_value"], lst=None):
        return env._lib.sg_vtrace_device(env._h, K, c, p(t["reward"]), p(t["done"]), p(t["trunc"]), p(value), p(t["last_value"]), p(d_ratio),
                                         p(dense), lst, p(out["a"]), p(pg), None)
    c0 = _native.SgReturnsConfig()
    env._lib.sg_returns_config_init(C.byref(c0))
    assert (c0.struct_size, c0.groups, c0.discounts, c0.gamma, c0.lambda_, c0.bootstrap_truncated, c0.rho_bar, c0.c_bar, c0.pg_rho_bar,
            c0.reserved) == (72, 0, None, 0.99, 0.95, 1, 1.0, 1.0, 1.0, 0)
    nan, inf = float("nan"), float("inf")
    cases = [("null cfg", lambda: gae(None)), ("null cfg", lambda: vtrace(None)),
             ("struct_size", lambda: gae(cfg(struct_size=64))), ("struct_size", lambda: vtrace(cfg(struct_size=0))),
             ("reserved", lambda: gae(cfg(reserved=1))), ("reserved", lambda: vtrace(cfg(reserved=-1))),
             ("n_steps", lambda: gae(cfg(), n_steps=0)),
             ("null reward", lambda: gae(cfg(), reward=None)), ("null reward", lambda: gae(cfg(), adv=None)),
             ("null reward", lambda: vtrace(cfg(), pg=None)),
             ("both", lambda: gae(cfg(), lst=C.byref(vl))), ("both", lambda: vtrace(cfg(), lst=C.byref(vl))),
             ("value list", lambda: gae(cfg(), dense=None, lst=C.byref(_native.SgValueList(None, vl.step_env, vl.value, vl.capacity)))),
             ("groups must be at least 0", lambda: gae(cfg(groups=-1))), ("groups must be at least 0", lambda: vtrace(cfg(groups=-3))),
             ("groups must divide", lambda: gae(cfg(groups=7))), ("groups must divide", lambda: vtrace(cfg(groups=480))),
             ("null discounts", lambda: gae(cfg(discounts=None))), ("null discounts", lambda: vtrace(cfg(discounts=None))),
             ("groups must be at least 1", lambda: gae(cfg(groups=0))),
             ("gamma", lambda: vtrace(cfg(groups=0, gamma=1.5))), ("gamma", lambda: vtrace(cfg(groups=0, gamma=nan))),
             ("lambda", lambda: vtrace(cfg(groups=0, lambda_=-0.5))), ("lambda", lambda: vtrace(cfg(groups=0, lambda_=nan))),
             ("must be > 0", lambda: vtrace(cfg(rho_bar=0.0))), ("must be > 0", lambda: vtrace(cfg(c_bar=-1.0))),
             ("must be > 0", lambda: vtrace(cfg(pg_rho_bar=nan))), ("must be > 0", lambda: gae(cfg(rho_bar=nan))),
             ("null value", lambda: vtrace(cfg(), value=None))]
    for match, call in cases:
        assert call() == -1, match
        assert match in env._lib.sg_last_error(env._h).decode(), (match, env._lib.sg_last_error(env._h))
    torch.cuda.synchronize()
    assert torch.isnan(out["a"]).all() and torch.isnan(out["b"]).all()
    env.check_status()
    # accepted: out-of-range scalars beside a table (not read), bars of +inf
    assert gae(cfg(gamma=7.0, lambda_=nan)) == 0
    _same(_host((out["a"], out["b"])), _gae_groups_want(s, table), "accepted gae")
    assert vtrace(cfg(gamma=-1.0, rho_bar=inf, c_bar=inf, pg_rho_bar=inf)) == 0
    _same(_host((out["a"], out["b"])), vtrace_model(**s, ratio=ratio, discounts=table, rho_bar=np.inf, c_bar=np.inf), "accepted vtrace")
    env.check_status()
