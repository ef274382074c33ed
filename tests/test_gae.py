"""CPU tests of the GAE entry points (sg_gae_config_init / sg_gae_device / sg_gae): the declarations and struct layouts, the Python
argument checks of gae_torch / gae with the native calls stubbed (nothing reaches a kernel), the NumPy model (tests/gae_model.py)
against an independent formulation, and the resources of the new kernels in the gfx950 build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import engine_asm
from gae_model import dense_from_list, gae_model, gae_model_f64, synthetic
from test_episode_stats import _fake_cuda, _stub_env
from test_snapshot_device import _header_args

DEVICE_ARGS = ["sg_env *env", "int32_t n_steps", "const sg_gae_config *cfg", "const float *reward_dev", "const uint8_t *done_dev",
               "const uint8_t *truncated_dev", "const float *value_dev", "const float *last_value_dev",
               "const float *terminal_value_dense_dev", "const sg_value_list *terminal_value_list", "float *advantage_dev",
               "float *ret_dev", "void *hip_stream"]


def _struct_fields(name):
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct %s {" % name, "")
    return [d.strip() for d in body.split(";") if d.strip()]


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_gae_device") == DEVICE_ARGS
    host = [a.replace("_dev", "_host") for a in DEVICE_ARGS[:-1]]
    assert _header_args("sg_gae") == host
    assert _header_args("sg_gae_config_init", "void") == ["sg_gae_config *cfg"]
    vp = C.c_void_p
    assert _native.SYMBOLS["sg_gae_device"] == (C.c_int, [vp, C.c_int32, C.POINTER(_native.SgGaeConfig), vp, vp, vp, vp, vp, vp,
                                                          C.POINTER(_native.SgValueList), vp, vp, vp])
    assert _native.SYMBOLS["sg_gae"] == (C.c_int, _native.SYMBOLS["sg_gae_device"][1][:-1])
    assert _native.SYMBOLS["sg_gae_config_init"] == (None, [C.POINTER(_native.SgGaeConfig)])
    # the ctypes mirrors: the header's fields in the header's order
    decls = _struct_fields("sg_gae_config")
    assert [d.split()[-1] for d in decls] == ["struct_size", "gamma", "lambda", "bootstrap_truncated"]
    assert [d.split()[0] for d in decls] == ["uint32_t", "double", "double", "int32_t"]
    assert [(f.rstrip("_"), t) for f, t in _native.SgGaeConfig._fields_] == [
        ("struct_size", C.c_uint32), ("gamma", C.c_double), ("lambda", C.c_double), ("bootstrap_truncated", C.c_int32)]
    assert C.sizeof(_native.SgGaeConfig) == 32
    decls = _struct_fields("sg_value_list")
    assert [d.split()[-1].lstrip("*") for d in decls] == [f for f, _ in _native.SgValueList._fields_] == ["count", "step_env", "value", "capacity"]
    for d, (_, ctype) in zip(decls, _native.SgValueList._fields_):
        assert ("*" in d) == (ctype is C.c_void_p), d
    assert _native.SgValueList._fields_[-1][1] is C.c_uint32 and C.sizeof(_native.SgValueList) == 32


K, B = 5, 8


def _args(**over):
    import torch
    a = dict(reward=torch.zeros((K, B)), done=torch.zeros((K, B), dtype=torch.uint8), trunc=torch.zeros((K, B), dtype=torch.uint8),
             value=torch.zeros((K, B)), last_value=torch.zeros(B), terminal_value=torch.zeros((K, B)))
    a = {k: _fake_cuda(v) for k, v in a.items()}
    a["out"] = dict(advantage=_fake_cuda(torch.zeros((K, B))), returns=_fake_cuda(torch.zeros((K, B))))
    a.update(over)
    return a


def _list(cap=16, **over):
    import torch
    t = dict(count=torch.zeros(1, dtype=torch.int32), step_env=torch.zeros((cap, 2), dtype=torch.int32), value=torch.zeros(cap))
    t.update(over)
    return {k: _fake_cuda(v) for k, v in t.items()}


@pytest.mark.parametrize("form", ["dense", "list", "none"])
def test_gae_torch_arguments_reach_the_native_call_in_order(form):
    env = _stub_env(B=B)
    a = _args()
    term = _list() if form == "list" else None
    if form != "dense":
        a["terminal_value"] = None
    adv, ret = env.gae_torch(terminal=term, gamma=0.9, lam=0.8, bootstrap_truncated=False, **a)
    assert env._lib.names() == ["sg_gae_device"]
    args = env._lib.calls[-1][1]
    assert len(args) == 13 and args[1] == K
    cfg = args[2]._obj
    assert (cfg.struct_size, cfg.gamma, cfg.lambda_, cfg.bootstrap_truncated) == (32, 0.9, 0.8, 0)
    for k, name in ((3, "reward"), (4, "done"), (5, "trunc"), (6, "value"), (7, "last_value")):
        assert args[k].value == a[name].data_ptr(), name
    assert (args[8].value == a["terminal_value"].data_ptr()) if form == "dense" else args[8] is None
    if form == "list":
        vl = args[9]._obj
        assert (vl.count, vl.step_env, vl.value, vl.capacity) == (term["count"].data_ptr(), term["step_env"].data_ptr(),
                                                                  term["value"].data_ptr(), 16)
    else:
        assert args[9] is None
    assert args[10].value == a["out"]["advantage"].data_ptr() and args[11].value == a["out"]["returns"].data_ptr()
    assert adv is a["out"]["advantage"] and ret is a["out"]["returns"]


def test_gae_torch_optional_arguments_go_as_null_and_the_defaults_are_the_headers():
    env = _stub_env(B=B)
    a = _args(value=None, last_value=None, terminal_value=None)
    env.gae_torch(**a)
    args = env._lib.calls[-1][1]
    assert args[6] is None and args[7] is None and args[8] is None and args[9] is None
    cfg = args[2]._obj
    assert (cfg.gamma, cfg.lambda_, cfg.bootstrap_truncated) == (0.99, 0.95, 1)


def test_value_list_torch_takes_count_and_step_env_from_the_terminal_list():
    import torch
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    term = dict(count=torch.zeros(1, dtype=torch.int32), step_env=torch.zeros((4, 2), dtype=torch.int32), obs=torch.zeros((4, 13)))
    v = torch.zeros(4)
    got = SpaceGymVectorEnv.value_list_torch(term, v)
    assert got["count"] is term["count"] and got["step_env"] is term["step_env"] and got["value"] is v and set(got) == {"count", "step_env", "value"}


def _bad_cases():
    import torch
    z = torch.zeros
    host = lambda *a, **k: z(*a, **k)  # noqa: E731  (a CPU tensor: not on the device)
    return {
        "reward dtype": dict(reward=_fake_cuda(z((K, B), dtype=torch.float64))),
        "reward shape": dict(reward=_fake_cuda(z((K, B + 1)))),
        "reward 1d": dict(reward=_fake_cuda(z(B))),
        "reward host": dict(reward=host((K, B))),
        "reward stride": dict(reward=_fake_cuda(z((K, 2 * B))[:, ::2])),
        "done dtype": dict(done=_fake_cuda(z((K, B), dtype=torch.bool))),
        "done shape": dict(done=_fake_cuda(z((K + 1, B), dtype=torch.uint8))),
        "trunc host": dict(trunc=host((K, B), dtype=torch.uint8)),
        "trunc stride": dict(trunc=_fake_cuda(z((B, K), dtype=torch.uint8).t())),
        "value dtype": dict(value=_fake_cuda(z((K, B), dtype=torch.float16))),
        "value shape": dict(value=_fake_cuda(z((K - 1, B)))),
        "last_value shape": dict(last_value=_fake_cuda(z((1, B)))),
        "last_value host": dict(last_value=host(B)),
        "terminal_value shape": dict(terminal_value=_fake_cuda(z((K, B, 1)))),
        "terminal_value stride": dict(terminal_value=_fake_cuda(z((K, 2 * B))[:, ::2])),
        "advantage dtype": dict(out=dict(advantage=_fake_cuda(z((K, B), dtype=torch.float64)), returns=_fake_cuda(z((K, B))))),
        "returns shape": dict(out=dict(advantage=_fake_cuda(z((K, B))), returns=_fake_cuda(z((K, 1))))),
        "returns host": dict(out=dict(advantage=_fake_cuda(z((K, B))), returns=host((K, B)))),
        "terminal both": dict(terminal=_list()),
        "count dtype": dict(terminal_value=None, terminal=_list(count=z(1, dtype=torch.int64))),
        "count host": dict(terminal_value=None, terminal={**_list(), "count": host(1, dtype=torch.int32)}),
        "step_env shape": dict(terminal_value=None, terminal=_list(step_env=z((16, 3), dtype=torch.int32))),
        "step_env dtype": dict(terminal_value=None, terminal=_list(step_env=z((16, 2), dtype=torch.int64))),
        "value length": dict(terminal_value=None, terminal=_list(value=z(15))),
        "value host": dict(terminal_value=None, terminal={**_list(), "value": host(16)}),
        "gamma high": dict(gamma=1.5), "gamma negative": dict(gamma=-0.1), "gamma nan": dict(gamma=float("nan")),
        "lam high": dict(lam=1.0001), "lam negative": dict(lam=-1.0), "lam nan": dict(lam=float("nan")),
    }


@pytest.mark.parametrize("bad", sorted(_bad_cases()))
def test_gae_torch_refuses_bad_arguments_before_any_native_call(bad):
    env = _stub_env(B=B)
    a = _args(**_bad_cases()[bad])
    with pytest.raises(ValueError, match=bad.split()[0]):
        env.gae_torch(**a)
    assert env._lib.calls == []


@pytest.mark.parametrize("bad", [dict(reward=np.zeros((K, B + 1), np.float32)), dict(reward=np.zeros((K, B))), dict(done=np.zeros((K, B), np.int32)),
                                 dict(trunc=np.zeros((K - 1, B), np.uint8)), dict(value=np.zeros((K, B))), dict(last_value=np.zeros((B, 1), np.float32)),
                                 dict(terminal_value=np.zeros((K, B), np.float32), terminal=dict(count=0, step_env=np.zeros((0, 2), np.int32), value=np.zeros(0, np.float32))),
                                 dict(terminal=dict(count=1, step_env=np.zeros((1, 2), np.int64), value=np.zeros(1, np.float32))),
                                 dict(terminal=dict(count=-1, step_env=np.zeros((1, 2), np.int32), value=np.zeros(1, np.float32))),
                                 dict(gamma=2.0), dict(lam=float("nan"))])
def test_numpy_gae_refuses_bad_arguments_before_any_native_call(bad):
    env = _stub_env(B=B)
    a = dict(reward=np.zeros((K, B), np.float32), done=np.zeros((K, B), np.uint8), trunc=np.zeros((K, B), bool))
    a.update(bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        env.gae(**a)
    assert env._lib.calls == []


def test_numpy_gae_reaches_sg_gae_with_a_list():
    env = _stub_env(B=B)
    term = dict(count=np.array([2], np.int32), step_env=np.array([[0, 1], [4, 7], [9, 9]], np.int32), value=np.ones(3, np.float32))
    adv, ret = env.gae(np.zeros((K, B), np.float32), np.zeros((K, B), bool), np.zeros((K, B), np.uint8), terminal=term, lam=1.0)
    assert env._lib.names() == ["sg_gae"] and adv.shape == ret.shape == (K, B) and adv.dtype == np.float32
    args = env._lib.calls[-1][1]
    assert len(args) == 12 and args[1] == K and args[6] is None and args[7] is None and args[8] is None
    vl = args[9]._obj
    assert vl.capacity == 3 and C.cast(vl.count, C.POINTER(C.c_uint32))[0] == 2


# ---------------------------------------------------------------------------------------------- the model itself
def _direct(reward, done, trunc, value, last_value, terminal_value, gamma, lam):
    """Independent formulation: per env the rollout is cut into episode segments (a segment ends at a done step or at the last
    step); within a segment A_t = sum_k (gamma lam)^k delta_{t+k}, summed directly in float64 with explicit powers.  Also
    returns the sum of the magnitudes of the terms, the scale the rounding errors of either formulation are proportional to."""
    K, B = reward.shape
    r, v, tv = reward.astype(np.float64), value.astype(np.float64), terminal_value.astype(np.float64)
    A, S = np.zeros((K, B)), np.zeros((K, B))
    for i in range(B):
        nv = np.empty(K)
        for t in range(K):
            if done[t, i]:
                nv[t] = tv[t, i] if trunc[t, i] else 0.0
            else:
                nv[t] = v[t + 1, i] if t + 1 < K else float(last_value[i])
        delta = r[:, i] + gamma * nv - v[:, i]
        ends = [t for t in range(K) if done[t, i] or t == K - 1]
        start = 0
        for end in ends:
            for t in range(start, end + 1):
                w = (gamma * lam) ** np.arange(end + 1 - t)
                A[t, i] = np.sum(w * delta[t:end + 1])
                S[t, i] = np.sum(w * np.abs(delta[t:end + 1]))
            start = end + 1
    return A, S


def test_model_equals_the_direct_sum_over_episode_segments():
    """relative difference <= 1e-12, relative to the sum of the magnitudes of the terms (>= |A|): both formulations add the same
    <= 64 float64 terms in different orders, so they differ by at most about 64 * 2^-53 ~ 7e-15 of that sum; relative to |A|
    itself the difference has no bound (the terms cancel)"""
    s = synthetic(64, 512, seed=11)
    done, trunc = s["done"].astype(bool), s["trunc"].astype(bool)
    assert 0.015 < done.mean() < 0.025 and (done & trunc).sum() > 100 and (done & ~trunc).sum() > 100 and not (trunc & ~done).any()
    assert abs(int((done & trunc).sum()) - int((done & ~trunc).sum())) <= 1
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.5)):
        A, R = gae_model_f64(gamma=gamma, lam=lam, **s)
        want, scale = _direct(s["reward"], done, trunc, s["value"], s["last_value"], s["terminal_value"], gamma, lam)
        rel = np.abs(A - want) / scale
        assert rel.max() <= 1e-12, (gamma, lam, rel.max())
        assert np.array_equal(R, A + s["value"].astype(np.float64))
        adv, ret = gae_model(gamma=gamma, lam=lam, **s)
        assert adv.dtype == ret.dtype == np.float32 and np.array_equal(adv, A.astype(np.float32)) and np.array_equal(ret, R.astype(np.float32))


def _delta(s, gamma):
    done, trunc = s["done"].astype(bool), s["trunc"].astype(bool)
    v = s["value"].astype(np.float64)
    nxt = np.concatenate([v[1:], s["last_value"].astype(np.float64)[None]])
    nv = np.where(done, np.where(trunc, s["terminal_value"].astype(np.float64), 0.0), nxt)
    return (s["reward"].astype(np.float64) + gamma * nv) - v


def test_model_special_cases():
    s = synthetic(64, 512, seed=12)
    # lambda = 0: the advantage is the one-step TD error
    A, _ = gae_model_f64(gamma=0.97, lam=0.0, **s)
    assert np.array_equal(A, _delta(s, 0.97))
    # gamma = 0: the advantage is reward - value
    A, R = gae_model_f64(gamma=0.0, lam=0.95, **s)
    assert np.array_equal(A, s["reward"].astype(np.float64) - s["value"].astype(np.float64))
    assert np.array_equal(R.astype(np.float32), s["reward"])
    # lambda = 1 without values: the discounted reward-to-go of the episode (no terminal values: a truncation ends it)
    gamma = 0.9
    A, R = gae_model_f64(s["reward"], s["done"], s["trunc"], gamma=gamma, lam=1.0)
    K, B = s["reward"].shape
    done = s["done"].astype(bool)
    togo, run = np.zeros((K, B)), np.zeros(B)
    for t in range(K - 1, -1, -1):
        run = s["reward"][t].astype(np.float64) + gamma * np.where(done[t], 0.0, run)
        togo[t] = run
    assert np.allclose(A, togo, rtol=1e-13, atol=1e-13) and np.array_equal(A, R)


def test_model_keeps_a_nan_inside_its_episode_and_bootstrap_off_ignores_terminal_values():
    s = synthetic(32, 16, seed=13, p_done=0.1)
    base, _ = gae_model(**s)
    t0, i0 = 17, 5
    bad = {k: v.copy() for k, v in s.items()}
    bad["reward"][t0, i0] = np.nan
    got, _ = gae_model(**bad)
    done = s["done"].astype(bool)[:, i0]
    first = max([t + 1 for t in range(t0) if done[t]], default=0)  # the episode of (t0, i0) began here; its steps <= t0 see the NaN
    inside = np.zeros_like(done)
    inside[first:t0 + 1] = True
    assert np.isnan(got[inside, i0]).all() and np.array_equal(got[~inside, i0], base[~inside, i0])
    others = np.arange(16) != i0
    assert np.array_equal(got[:, others], base[:, others])
    off, _ = gae_model(bootstrap_truncated=False, **s)
    none, _ = gae_model(**{**s, "terminal_value": None})
    assert np.array_equal(off, none) and not np.array_equal(off, base)


def test_dense_from_list_places_the_records_and_ignores_the_bad_ones():
    se = np.array([[0, 1], [2, 3], [5, 0], [1, -1], [1, 4], [4, 2]], np.int32)
    val = np.arange(1, 7, dtype=np.float32)
    d = dense_from_list(5, 4, 5, se, val)  # count 5: the last record is not in the list
    want = np.zeros((5, 4), np.float32)
    want[0, 1], want[2, 3] = 1, 2
    assert np.array_equal(d, want)
    assert np.array_equal(dense_from_list(5, 4, 9, se, val)[4, 2], np.float32(6))  # count past the capacity: what the list holds


# ---------------------------------------------------------------------------------------------- the build
def test_the_status_message_of_a_refused_value_list_is_reachable():
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    inc = open(os.path.join(build.CSRC, "sg_gae.inc")).read()
    assert "sg_gae.inc" in build.HEADERS and '#include "sg_gae.inc"' in src
    code = int(re.search(r"constexpr int kStatusGaeList = (\d+);", inc).group(1))
    others = [int(v) for v in re.findall(r"constexpr int kStatus\w+ = (\d+);", src)]
    assert code not in others and code > 3  # (1 .. 3: the rollout kernels' hand-off waits)
    assert len(re.findall(r"\*status = kStatusGaeList;", engine_asm.function_body(inc, "void gae_scatter_kernel("))) == 2  # count, record
    for sig in ("static int status_error(sg_env *e, const char *who)", 'extern "C" int sg_check_status(sg_env *e)'):
        assert re.search(r"if \(st == kStatusGaeList\)\s*return fail\(", engine_asm.function_body(src, sig)), sig
    lib = open(build.build(), "rb").read()
    assert b"sg_gae_device: a value list with count > capacity" in lib
    assert b"an earlier sg_gae_device was given a value list" in lib


def test_the_new_kernels_build_for_gfx950_without_scratch():
    """build() makes the library with the entry points and the kernels; in the code object the four scan kernels and the scatter
    kernel use no scratch, spill no vector register and need no LDS; the scan kernels fit 4 waves per SIMD (<= 128 VGPRs), so a
    batch of 1 048 576 envs hides latency by occupancy as well; every instruction of theirs that writes memory is a
    global_store_* of one element (dword), and none is wider: nothing assumes more than 4-byte alignment"""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    for name in (b"sg_gae_config_init", b"sg_gae_device", b"sg_gae", b"gae_scan_kernel", b"gae_scatter_kernel"):
        assert name in lib
    kernels = engine_asm.descriptors(r"\S*(?:gae_scan_kernel|gae_scatter_kernel)\S*")
    assert len(kernels) == 5, [k for k, _ in kernels]  # gae_scan_kernel<value?, terminal?> x 4, gae_scatter_kernel
    for name, field in kernels:
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == 0, name
        assert field["next_free_vgpr"] <= 128, name
    spills = engine_asm.spill_counts(r"\S*(?:gae_scan_kernel|gae_scatter_kernel)\S*")
    assert len(spills) == 5 and all(n == 0 for _, n in spills), spills
    for name, _ in kernels:
        fn = engine_asm.function(name)
        writes = re.findall(r"^\s+(\w*(?:store|atomic)\w*)\s", fn, flags=re.M)
        assert writes and all(w == "global_store_dword" for w in writes), (name, sorted(set(writes)))
        loads = set(re.findall(r"^\s+(global_load_\w+)\s", fn, flags=re.M))
        assert loads <= {"global_load_dword", "global_load_ubyte", "global_load_dwordx2"}, (name, loads)
        if "gae_scan" in name:
            assert "global_load_dwordx2" not in loads, name  # (the scatter kernel reads a (step, env) pair, 8-byte aligned rows)
            assert not re.search(r"\bv_fma_f64\b", fn), name  # every float64 operation rounds on its own
