"""CPU tests of the per-member Adam step with gradient clipping and the PBT exploit copy (sg_adam_step_device / sg_adam_exploit_device,
adam_torch / adam_step_torch / adam_exploit_torch): the declarations, the NumPy statement (tests/adam_model.py) in its
float64 form against torch.optim.Adam / AdamW with clip_grad_norm_ per member, the skip rule, the members' independence, the exploit
rule, and the Python argument checks with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adam_model as am
from test_episode_stats import _fake_cuda, _stub_env
from test_snapshot_device import _header_args

P = 3
SHAPES = [(7, 5), (7,), (2, 7), (2,), (1, 7), (1,), (2,)]  # per member: odd sizes, a head of 2, a head of 1, log_std


def _tensors(rng, dtype, scale=0.3):
    return [(scale * rng.standard_normal((P,) + s)).astype(dtype) for s in SHAPES]


def _zeros(like):
    return [np.zeros_like(t) for t in like]


def _member_norm(grads, m):
    return float(np.sqrt(sum(float((np.asarray(g[m], np.float64) ** 2).sum()) for g in grads)))


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import NET_METHODS, SpaceGymVectorEnv
    assert _header_args("sg_adam_step_device") == ["sg_env *env", "int32_t members", "int32_t n_tensors", "const sg_adam_tensor *tensors",
                                                   "const float *hyper", "double *state", "void *hip_stream"]
    assert _header_args("sg_adam_exploit_device") == ["sg_env *env", "int32_t members", "int32_t n_tensors", "const sg_adam_tensor *tensors",
                                                      "double *state", "const int32_t *src", "int32_t *refused_out", "void *hip_stream"]
    vp, Pt = C.c_void_p, C.POINTER
    assert _native.SYMBOLS["sg_adam_step_device"] == (C.c_int, [vp, C.c_int32, C.c_int32, Pt(_native.SgAdamTensor), vp, vp, vp])
    assert _native.SYMBOLS["sg_adam_exploit_device"] == (C.c_int, [vp, C.c_int32, C.c_int32, Pt(_native.SgAdamTensor), vp, vp, vp, vp])
    header = open(os.path.join(build.ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct sg_adam_tensor {"):header.index("} sg_adam_tensor;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct sg_adam_tensor {", "")
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert [d.split()[-1].lstrip("*") for d in decls] == [f for f, _ in _native.SgAdamTensor._fields_] == ["param", "grad", "exp_avg", "exp_avg_sq", "numel"]
    assert [("*" in d) for d in decls] == [t is C.c_void_p for _, t in _native.SgAdamTensor._fields_]
    assert decls[-1].startswith("int64_t") and _native.SgAdamTensor._fields_[-1][1] is C.c_int64 and C.sizeof(_native.SgAdamTensor) == 40
    assert SpaceGymVectorEnv.adam_hyper_names == am.HYPER and SpaceGymVectorEnv.adam_state_names == am.STATE
    assert len(am.HYPER) == len(am.STATE) == 8
    assert {"adam_torch", "adam_step_torch", "adam_exploit_torch"} <= set(NET_METHODS)
    # the header states the hyper and state rows in the model's order
    flat = " ".join(header.split())
    assert "(lr, beta1, beta2, eps, weight_decay, max_grad_norm, reserved, reserved)" in flat.replace(" * ", " ")
    assert "(steps, beta1_pow, beta2_pow, skipped, grad_norm, clip_scale, step_size, applied)" in flat.replace(" * ", " ")


def test_the_kernels_live_in_sg_adam_inc_and_use_no_atomics():
    from space_gym_amd import build
    assert "sg_adam.inc" in build.HEADERS
    assert '#include "sg_adam.inc"' in open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    inc = open(os.path.join(build.CSRC, "sg_adam.inc")).read()
    for kernel in ("adam_prepare_kernel", "adam_update_kernel", "adam_exploit_kernel"):
        assert re.search(r"void %s\(" % kernel, inc), kernel
    code = re.sub(r"//.*", "", inc)
    assert "atomic" not in code.lower()
    # correctly rounded square roots and divisions only; the model's lane count
    assert "__fsqrt_rn" not in code and "rsqrt" not in code and "__fdividef" not in code and "pow" not in code.replace("Pow", "")
    assert re.search(r"kAdamPrepareBlock = %d\b" % am.LANES, code) and re.search(r"kAdamMaxTensors = 32\b", code)


# ---------------------------------------------------------------------------------------------------------------- the model against torch
def _torch_reference(tensors, grad_steps, hyper, adamw):
    """torch.optim.Adam / AdamW on float64 CPU tensors, one optimizer per member, clip_grad_norm_ over the member's tensors"""
    import torch
    out, norms = [], []
    for m in range(P):
        lr, b1, b2, eps, wd, mx = (float(x) for x in hyper[m][:6])
        params = [torch.tensor(t[m], dtype=torch.float64, requires_grad=True) for t in tensors]
        opt = (torch.optim.AdamW if adamw else torch.optim.Adam)(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        norms.append([])
        for grads in grad_steps:
            for p, g in zip(params, grads):
                p.grad = torch.tensor(g[m], dtype=torch.float64)
            if 0 < mx < np.inf:
                norms[-1].append(float(torch.nn.utils.clip_grad_norm_(params, mx)))
            opt.step()
        st = [opt.state[p] for p in params]
        out.append(([p.detach().numpy() for p in params], [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st]))
    return out, norms


@pytest.mark.parametrize("off", [None, np.inf, 0.0], ids=["none", "inf", "zero"])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_float64_model_equals_torch_adam_over_five_steps(weight_decay, off):
    """member 0 clips, member 1 has a bound that never binds, member 2 has clipping off; every member its own row of hyper"""
    rng = np.random.default_rng(5)
    tensors = _tensors(rng, np.float64)
    grad_steps = [_tensors(rng, np.float64, scale=1.0) for _ in range(5)]
    for grads in grad_steps:  # member m's gradients scaled by 10^m: norms that differ
        for g in grads:
            g *= np.array([1.0, 10.0, 0.1]).reshape((P,) + (1,) * (g.ndim - 1))
    hyper = am.make_hyper(P, lr=[3e-4, 1e-3, 2.5e-4], betas=([0.9, 0.8, 0.95], [0.999, 0.99, 0.98]), eps=[1e-8, 1e-5, 1e-7],
                          weight_decay=weight_decay, max_grad_norm=[0.5, 1e4, np.inf if off is None else off], dtype=np.float64)
    if off is None:
        assert np.array_equal(am.make_hyper(1, max_grad_norm=None)[:, am.MAX_GRAD_NORM], [np.inf])
    want, norms = _torch_reference(tensors, grad_steps, hyper, adamw=weight_decay > 0)
    t, ea, es, st = tensors, _zeros(tensors), _zeros(tensors), am.fresh_state(P)
    scales = []
    for grads in grad_steps:
        t, ea, es, st = am.adam_step(t, grads, ea, es, hyper, st, dtype=np.float64)
        scales.append(st[:, am.CLIP_SCALE].copy())
        for m in range(P):
            np.testing.assert_allclose(st[m, am.GRAD_NORM], _member_norm(grads, m), rtol=1e-12)
    scales = np.array(scales)
    assert (scales[:, 0] < 0.5).all() and (scales[:, 1] == 1).all() and (scales[:, 2] == 1).all()
    np.testing.assert_allclose(scales[:, 0], [0.5 / (n + 1e-6) for n in norms[0]], rtol=1e-12)
    assert np.array_equal(st[:, am.STEPS], [5] * P) and np.array_equal(st[:, am.APPLIED], [1] * P) and not st[:, am.SKIPPED].any()
    np.testing.assert_allclose(st[:, am.BETA1_POW], hyper[:, am.BETA1] ** 5, rtol=1e-12)
    np.testing.assert_allclose(st[:, am.BETA2_POW], hyper[:, am.BETA2] ** 5, rtol=1e-12)
    for m in range(P):
        for got, ref in zip((t, ea, es), want[m]):
            for k in range(len(SHAPES)):
                np.testing.assert_allclose(got[k][m], ref[k], rtol=1e-12, atol=0, err_msg=str((m, k)))
    # and the update moved every parameter
    assert all((a != b).all() for a, b in zip(t, tensors))


def test_a_tensor_without_a_gradient_stays_out_of_the_norm_and_of_the_update():
    rng = np.random.default_rng(6)
    tensors, grads = _tensors(rng, np.float32), _tensors(rng, np.float32, scale=1.0)
    hyper = am.make_hyper(P, max_grad_norm=0.5)
    frozen = list(grads)
    frozen[4] = frozen[5] = None
    t, ea, es, st = am.adam_step(tensors, frozen, _zeros(tensors), _zeros(tensors), hyper, am.fresh_state(P))
    live = [g for g in frozen if g is not None]
    for m in range(P):
        np.testing.assert_allclose(st[m, am.GRAD_NORM], _member_norm(live, m), rtol=2.0 ** -23)
        assert st[m, am.GRAD_NORM] < _member_norm(grads, m)
    for k in (4, 5):
        assert t[k].tobytes() == tensors[k].tobytes() and not ea[k].any() and not es[k].any()
    assert all((t[k] != tensors[k]).all() for k in (0, 1, 2, 3, 6))


def test_the_float32_model_rounds_every_operation_and_is_close_to_the_float64_form():
    rng = np.random.default_rng(7)
    tensors, grads = _tensors(rng, np.float32), _tensors(rng, np.float32, scale=1.0)
    hyper = am.make_hyper(P, lr=1e-3, weight_decay=0.01, max_grad_norm=[0.5, 100.0, None])
    a = am.adam_step(tensors, grads, _zeros(tensors), _zeros(tensors), hyper, am.fresh_state(P))
    b = am.adam_step(tensors, grads, _zeros(tensors), _zeros(tensors), hyper.astype(np.float64), am.fresh_state(P), dtype=np.float64)
    for x, y in zip(a[:3], b[:3]):
        for k in range(len(SHAPES)):
            assert x[k].dtype == np.float32 and y[k].dtype == np.float64
            np.testing.assert_allclose(x[k], y[k], rtol=1e-5, atol=1e-9)
    for col in (am.GRAD_NORM, am.CLIP_SCALE, am.STEP_SIZE):  # float32 values, stored exactly
        assert np.array_equal(a[3][:, col], a[3][:, col].astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(a[3], b[3], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- skip, independence
def _bits(result):
    t, ea, es, st = result
    return [[b"".join(x[m].tobytes() for x in (*t, *ea, *es)) + st[m].tobytes() for m in range(P)]][0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_member_with_a_non_finite_gradient_is_skipped_and_counted(bad, dtype):
    rng = np.random.default_rng(8)
    tensors, ea, es = _tensors(rng, dtype), _tensors(rng, dtype, 0.01), [np.abs(x) for x in _tensors(rng, dtype, 0.01)]
    grads = _tensors(rng, dtype, 1.0)
    hyper = am.make_hyper(P, max_grad_norm=[0.5, 0.5, None], dtype=dtype)
    state = am.fresh_state(P)
    state[:, :4] = [[3, 0.9 ** 3, 0.999 ** 3, 0], [4, 0.9 ** 4, 0.999 ** 4, 2], [5, 0.9 ** 5, 0.999 ** 5, 0]]
    clean = am.adam_step(tensors, grads, ea, es, hyper, state, dtype=dtype)
    grads[2][1].reshape(-1)[3] = bad
    t, a, s, st = am.adam_step(tensors, grads, ea, es, hyper, state, dtype=dtype)
    for new, old in ((t, tensors), (a, ea), (s, es)):
        for k in range(len(SHAPES)):
            assert new[k][1].tobytes() == old[k][1].tobytes()
    assert st[1, :3].tobytes() == state[1, :3].tobytes() and st[1, am.SKIPPED] == 3 and st[1, am.APPLIED] == 0
    assert not np.isfinite(st[1, am.GRAD_NORM]) and st[1, am.CLIP_SCALE] == 0 and st[1, am.STEP_SIZE] == 0
    got, want = _bits((t, a, s, st)), _bits(clean)
    assert got[0] == want[0] and got[2] == want[2] and got[1] != want[1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_members_step_depends_on_nothing_of_another_member(dtype):
    """changing member 1's gradients, hyperparameters -- a NaN learning rate among them -- or state leaves members 0 and 2 bit-equal"""
    rng = np.random.default_rng(9)
    tensors, ea, es = _tensors(rng, dtype), _tensors(rng, dtype, 0.01), [np.abs(x) for x in _tensors(rng, dtype, 0.01)]
    grads = _tensors(rng, dtype, 1.0)
    hyper = am.make_hyper(P, lr=[3e-4, 1e-3, 1e-4], weight_decay=0.01, max_grad_norm=[0.5, 0.5, None], dtype=dtype)
    state = am.fresh_state(P)
    base = _bits(am.adam_step(tensors, grads, ea, es, hyper, state, dtype=dtype))

    def changed(what):
        g, h, s = [x.copy() for x in grads], hyper.copy(), state.copy()
        if what == "grads":
            for x in g:
                x[1] *= 1000.0
        elif what == "hyper":
            h[1, :6] = [1e-2, 0.5, 0.9, 1e-3, 0.1, 1e-3]
        elif what == "nan_lr":
            h[1, am.LR] = np.nan
        else:
            s[1, :4] = [100, 1e-3, 0.5, 7]
        return _bits(am.adam_step(tensors, g, ea, es, h, s, dtype=dtype))

    for what in ("grads", "hyper", "nan_lr", "state"):
        got = changed(what)
        assert got[0] == base[0] and got[2] == base[2], what
        assert got[1] != base[1], what


def test_clipping_is_off_by_the_comparison():
    for mx in (0.0, -1.0, np.inf, np.nan):
        assert am.clip_scale(np.float32(3.0), np.float32(mx)) == 1 and am.clip_scale(3.0, mx, np.float64) == 1
    assert am.clip_scale(np.float32(3.0), np.float32(6.0)) == 1
    assert am.clip_scale(np.float32(3.0), np.float32(1.5)) == np.float32(1.5 / (3.0 + 1e-6))
    assert am.clip_scale(np.float32(0.0), np.float32(1.5)) == 1
    assert np.array_equal(am.make_hyper(3, max_grad_norm=[0.5, None, 0.0])[:, am.MAX_GRAD_NORM], np.array([0.5, np.inf, 0.0], np.float32))


def test_the_sum_of_squares_follows_the_lane_order():
    rng = np.random.default_rng(10)
    gs = [rng.standard_normal(n).astype(np.float32) for n in (1, 1023, 1025, 4096, 70)]
    got = am.sum_of_squares(gs)
    lanes = np.zeros(am.LANES)
    for g in gs:
        for i, x in enumerate(g):
            lanes[i % am.LANES] += float(x) * float(x)
    s = am.LANES // 2
    while s:
        for i in range(s):
            lanes[i] += lanes[i + s]
        s //= 2
    assert got == lanes[0]
    import math
    exact = math.fsum(float(x) * float(x) for g in gs for x in g)
    assert abs(got - exact) <= exact * 2.0 ** -40


# ---------------------------------------------------------------------------------------------------------------- exploit
def _exploit_case(Pm, seed=11):
    rng = np.random.default_rng(seed)
    mk = lambda: [rng.standard_normal((Pm,) + s).astype(np.float32) for s in SHAPES[:3]]
    state = rng.random((Pm, 8))
    return mk(), mk(), mk(), state


@pytest.mark.parametrize("src,performed,refused", [
    ([0, 1, 2, 3], [-1, -1, -1, -1], 0),            # identity
    ([0, 1, 0, 1], [-1, -1, 0, 1], 0),              # truncation: the bottom two copy the top two
    ([2, 0, 2], [2, -1, -1], 1),                    # a chain: member 1's copy from 0 is refused, 0 is a destination
    ([1, 0], [-1, -1], 2),                          # a swap: both sources are destinations
    ([-1, 4, 2 ** 31 - 1, 3], [-1, -1, -1, -1], 3),  # out of range
    ([3, 3, 3, 3], [3, 3, 3, -1], 0),               # everyone copies the best
])
def test_exploit_model(src, performed, refused):
    Pm = len(src)
    t, ea, es, st = _exploit_case(Pm)
    assert am.exploit_sources(src)[0].tolist() == performed and am.exploit_sources(src)[1] == refused
    t2, ea2, es2, st2, r = am.adam_exploit(t, ea, es, st, src)
    assert r == refused
    for m in range(Pm):
        s = performed[m] if performed[m] >= 0 else m
        for new, old in ((t2, t), (ea2, ea), (es2, es)):
            for k in range(len(new)):
                assert new[k][m].tobytes() == old[k][s].tobytes()
        assert st2[m, :4].tobytes() == st[s, :4].tobytes() and st2[m, 4:].tobytes() == st[m, 4:].tobytes()


# ---------------------------------------------------------------------------------------------------------------- Python checks, native calls stubbed
def _handles(Pm=P):
    import torch
    from space_gym_amd import _native
    from space_gym_amd.vector_env import Policy, PolicyPopulation
    shapes = [(4, 13), (4,), (2, 4), (2,), (4, 13), (4,), (1, 4), (1,), (2,)]
    struct = _native.SgPolicy(n_hidden=1, hidden=4)
    pop = PolicyPopulation(struct, [_fake_cuda(torch.zeros((Pm,) + s)) for s in shapes], True, Pm)
    one = Policy(struct, [_fake_cuda(torch.zeros(s)) for s in shapes], True)
    return one, pop


def _opt(handle):
    import torch
    from space_gym_amd.vector_env import AdamState
    Pm = getattr(handle, "members", 1)
    z = lambda: [_fake_cuda(torch.zeros(tuple(t.shape))) for t in handle.tensors]
    return AdamState(handle, Pm, _fake_cuda(torch.zeros((Pm, 8))), _fake_cuda(torch.zeros((Pm, 8), dtype=torch.float64)), z(), z())


def _grads(handle, critic=True):
    import torch
    t = [_fake_cuda(torch.zeros(tuple(x.shape))) for x in handle.tensors]
    return dict(actor=[(t[0], t[1]), (t[2], t[3])], critic=[(t[4], t[5]), (t[6], t[7])] if critic else None, log_std=t[8])


@pytest.mark.parametrize("kw,match", [
    (dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr=float("inf")), "lr"), (dict(lr=[1e-3, 1e-3]), "lr"),
    (dict(betas=(1.0, 0.999)), "beta1"), (dict(betas=(0.9, -0.1)), "beta2"), (dict(betas=(0.9,)), "betas"),
    (dict(eps=-1e-8), "eps"), (dict(weight_decay=-0.01), "weight_decay"), (dict(weight_decay=float("nan")), "weight_decay"),
    (dict(max_grad_norm=-0.5), "max_grad_norm"), (dict(max_grad_norm=float("nan")), "max_grad_norm"),
    (dict(max_grad_norm=[0.5] * 4), "max_grad_norm"),
])
def test_adam_torch_refuses_bad_hyperparameters(kw, match):
    env = _stub_env()
    one, pop = _handles()
    with pytest.raises(ValueError, match=match):
        env.adam_torch(pop, **kw)
    assert not env._lib.calls


def test_adam_torch_refuses_what_is_no_handle():
    import torch
    env = _stub_env()
    one, pop = _handles()
    with pytest.raises(ValueError, match="handle"):
        env.adam_torch([torch.zeros(3)])
    host = type(one)(one.struct, [torch.zeros(tuple(t.shape)) for t in one.tensors], True)
    with pytest.raises(ValueError, match="CUDA tensor"):
        env.adam_torch(host)


def test_adam_step_torch_reaches_the_native_call_with_the_table():
    env = _stub_env()
    for handle, Pm in zip(_handles(), (1, P)):
        opt = _opt(handle)
        grads = _grads(handle)
        assert env.adam_step_torch(opt, grads) is opt.state
        name, args = env._lib.calls[-1]
        assert name == "sg_adam_step_device" and args[1] == Pm and args[2] == 9 == len(args[3])
        assert args[4].value == opt.hyper.data_ptr() and args[5].value == opt.state.data_ptr()
        flat = [*grads["actor"][0], *grads["actor"][1], *grads["critic"][0], *grads["critic"][1], grads["log_std"]]
        for k, row in enumerate(args[3]):
            assert (row.param, row.grad, row.exp_avg, row.exp_avg_sq) == (handle.tensors[k].data_ptr(), flat[k].data_ptr(),
                                                                           opt.exp_avg[k].data_ptr(), opt.exp_avg_sq[k].data_ptr())
            assert row.numel == handle.tensors[k].numel() // Pm
        # a frozen critic: its four tensors leave the table
        frozen = _grads(handle, critic=False)
        env.adam_step_torch(opt, frozen)
        args = env._lib.calls[-1][1]
        assert args[2] == 5 and [r.param for r in args[3]] == [handle.tensors[k].data_ptr() for k in (0, 1, 2, 3, 8)]
        # the same gradient tensors again: the same table object
        env.adam_step_torch(opt, frozen)
        assert env._lib.calls[-1][1][3] is args[3]


def test_adam_step_torch_refusals():
    import torch
    env = _stub_env()
    one, pop = _handles()
    opt = _opt(pop)
    with pytest.raises(ValueError, match="AdamState"):
        env.adam_step_torch(pop, _grads(pop))
    g = _grads(pop)
    g["log_std"] = _fake_cuda(torch.zeros((P, 3)))
    with pytest.raises(ValueError, match="grads"):
        env.adam_step_torch(opt, g)
    g = _grads(pop)
    g["actor"][0] = (torch.zeros((P, 4, 13)), g["actor"][0][1])  # host memory
    with pytest.raises(ValueError, match="CUDA tensor"):
        env.adam_step_torch(opt, g)
    g = _grads(pop)
    g["actor"][1] = (_fake_cuda(torch.zeros((P, 2, 4), dtype=torch.float64)), g["actor"][1][1])
    with pytest.raises(ValueError, match="grads"):
        env.adam_step_torch(opt, g)
    with pytest.raises(ValueError, match="no tensor has a gradient"):
        env.adam_step_torch(opt, dict(actor=None, critic=None, log_std=None))
    bad = _opt(pop)
    bad.hyper = _fake_cuda(torch.zeros((P, 6)))
    with pytest.raises(ValueError, match="opt.hyper"):
        env.adam_step_torch(bad, _grads(pop))
    bad = _opt(pop)
    bad.state = _fake_cuda(torch.zeros((P, 8)))  # float32
    with pytest.raises(ValueError, match="opt.state"):
        env.adam_step_torch(bad, _grads(pop))
    assert not env._lib.calls


def test_adam_exploit_torch_checks_and_reaches_the_native_call():
    import torch
    env = _stub_env()
    one, pop = _handles()
    opt = _opt(pop)
    src = _fake_cuda(torch.zeros(P, dtype=torch.int32))
    refused = _fake_cuda(torch.zeros(1, dtype=torch.int32))
    for bad in (_fake_cuda(torch.zeros(P, dtype=torch.int64)), _fake_cuda(torch.zeros(P + 1, dtype=torch.int32)), torch.zeros(P, dtype=torch.int32), [0, 1, 2]):
        with pytest.raises(ValueError, match="src"):
            env.adam_exploit_torch(opt, bad)
    for bad in (_fake_cuda(torch.zeros(2, dtype=torch.int32)), _fake_cuda(torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(ValueError, match="refused"):
            env.adam_exploit_torch(opt, src, refused=bad)
    with pytest.raises(ValueError, match="AdamState"):
        env.adam_exploit_torch(None, src)
    assert not env._lib.calls
    assert env.adam_exploit_torch(opt, src, refused=refused) is refused
    name, args = env._lib.calls[-1]
    assert name == "sg_adam_exploit_device" and args[1] == P and args[2] == 9 == len(args[3])
    assert all(r.grad is None and r.numel == t.numel() // P for r, t in zip(args[3], pop.tensors))
    assert (args[4].value, args[5].value, args[6].value) == (opt.state.data_ptr(), src.data_ptr(), refused.data_ptr())
    env.adam_exploit_torch(opt, src)
    assert env._lib.calls[-1][1][6] is None


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("adam_torch", "adam_step_torch", "adam_exploit_torch"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
