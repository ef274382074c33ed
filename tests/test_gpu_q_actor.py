"""GPU tests of q_actor_grad_torch / q_actor_update_torch (sg_q_actor_squashed_grad_device / sg_q_actor_gaussian_grad_device) against the
calls they fuse and against the NumPy model tests/q_actor_model.py.

 1. action and logp are squashed_sample_raw_torch's (policy_action_raw_torch's) bits;
 2. q1 and q2 are q_evaluate_raw_torch's bits at that action;
 3. dq1_da / dq2_da equal q_grad_torch's action gradient for g_q1 / g_q2 = ones with the critics frozen;
 4. g_action is (-dq_sel) / n to the bit;
 5. the gradients are squashed_grad_torch's (policy_action_grad_torch's) bits for the reported g_action and g_logp = alpha / n wherever
    the row tile of the larger width class is the actor's own (every pair of one class, and the mixed pairs whose actor is the wider
    net or whose classes tile alike); in the mixed pair where it is not, within the tolerance rule;
 6. every row array, statistic and gradient within 8 x max|x32seq - x64| + 1e-6 (1 + max|x64|) of the float64 model (tests/test_q_actor.py
    checks each case's 1 % cap and the other conditions on the CPU); the device selects the critics the model selects;
 7. q_select = 0 on two critics leaves the critic-2 statistics at 0;
 8. a float alpha and a tensor alpha give the same bits;
 9. two calls into NaN-prefilled outputs and workspace give equal bits;
10. the whole update replays as a graph; 11. the native refusals and the workspace query; 12. the width family; 13. a trained regime."""
import ctypes as C
import functools

import numpy as np
import pytest

from net_widths import N as WIDTH_N, OBS_DIM, ids_of
from q_actor_model import ALPHA, BIG_N, BOUNDS, GRAD_ROWS, MIXED, ROWS, STATS, case as actor_case, flat, grad_case, grad_cases, grad_tolerances
from q_actor_model import reference, regime_case, regime_reference, register_width_family, same_tile, width_cases
from test_gpu_policy import _dev, _handle as _policy_handle, _np, make

pytestmark = pytest.mark.gpu
register_width_family()  # (tests/test_net_widths.py counts the engine's kernel templates against the families: see q_actor_model)

GOAL, KEPLER, DISCRETE = "GoalContinuous3P-v0", "KeplerCircleOrbit-v0", "GoalDiscrete3-v0"
WORST = []  # (error / tolerance, error, tolerance, what): printed by the last test of the file
COLS = dict(action=2, logp=1, q1=1, q2=1, q_sel=1, dq1_da=2, dq2_da=2, g_action=2)


def _handles(env, c, activation, bounds=BOUNDS):
    """(actor handle, q handle) over device copies of a case's nets"""
    if c["form"] == "squashed":
        actor = env.squashed_policy_torch(actor=[(_dev(W), _dev(b)) for W, b in c["actor"]], log_std_bounds=bounds, activation=activation)
    else:
        actor = _policy_handle(env, c["actor"], activation)
    return actor, env.q_torch(critics=[[(_dev(W), _dev(b)) for W, b in net] for net in c["critics"]], activation=activation)


def _env_for(obs_dim, n):
    env = make(GOAL if obs_dim == 15 else KEPLER, min(n, 256))  # (the net calls take any n: the env count only sizes the handle)
    assert env.obs_dim == obs_dim and not env.discrete
    return env


def _tol(x32, x64):
    x64 = np.asarray(x64, np.float64)
    return 8.0 * float(np.abs(np.asarray(x32, np.float64) - x64).max()) + 1e-6 * (1.0 + float(np.abs(x64).max()))


def _close(got, x32, x64, what):
    t, err = _tol(x32, x64), float(np.abs(np.asarray(got, np.float64) - x64).max())
    print(what, "error %.3g tolerance %.3g" % (err, t))
    WORST.append((err / t, err, t, what))
    assert err <= t, (what, err, t)


def _grads_np(out):
    import torch
    torch.cuda.synchronize()
    return flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]],
                     log_std=out["log_std"].cpu().numpy() if out.get("log_std") is not None else None))


def _check_grads(got, g32, g64, what):
    tol = grad_tolerances(g32, g64)
    assert set(got) == set(g64), what
    for k in g64:
        top = float(np.abs(g64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - g64[k]).max())
        print("gradient", what, k, "error %.3g tolerance %.3g max|G64| %.3g" % (err, tol[k], top))
        WORST.append((err / tol[k], err, tol[k], what + (k,)))
        if top > 0:  # (the log_std gradient without noise is 0, written as 0)
            assert tol[k] <= 0.01 * top, (what, k, tol[k], top)
        assert err <= tol[k], (what, k, err, tol[k])


def _rows(n, two, fill=float("nan")):
    import torch
    return {k: torch.full((n, 2) if COLS[k] == 2 else (n,), fill, device="cuda") for k in ROWS if two or k not in ("q2", "dq2_da")}


def _bits(t):
    return _np(t)[0].tobytes()


@functools.lru_cache(maxsize=None)
def _models(gc):
    """the float64 and the float32 model of a case (computed once per case, shared, never written)"""
    obs_dim, n, a, q, n_critics, form, activation, eps_given, q_select = gc
    c = grad_case(obs_dim, n, a, q, n_critics, form, activation, eps_given)
    return tuple(reference(c, activation, eps_given, q_select, dt) for dt in (np.float64, np.float32))


def _two(form, n_critics, q_select):
    return bool(q_select) if q_select is not None else (form == "squashed" and n_critics == 2)


def _check_composed(env, actor, q, obs, eps, alpha, two, grads, rows, what, exact):
    """1 .. 5 of the module's list, for one call's outputs; returns the fused gradients as NumPy"""
    import torch
    n = obs.shape[0]
    squashed = "log_std" not in grads
    if squashed:
        action, logp = env.squashed_sample_raw_torch(actor, obs, eps)
        assert _bits(rows["logp"]) == _bits(logp), what
    else:
        action = env.policy_action_raw_torch(actor, obs, eps)
        assert not rows["logp"].any(), what
    assert _bits(rows["action"]) == _bits(action), what
    qs = env.q_evaluate_raw_torch(q, obs, action)
    ones = torch.ones(n, device="cuda")
    assert _bits(rows["q1"]) == _bits(qs[0]), what
    dq1 = env.q_grad_torch(q, obs, action, g_q1=ones, params=False, action_grad=True)["action"]
    assert torch.equal(rows["dq1_da"], dq1) and rows["dq1_da"].abs().max() > 0, what
    if two:
        assert _bits(rows["q2"]) == _bits(qs[1]), what
        dq2 = env.q_grad_torch(q, obs, action, g_q2=ones, params=False, action_grad=True)["action"]
        assert torch.equal(rows["dq2_da"], dq2), what
        sel2 = qs[1] < qs[0]
        assert _bits(rows["q_sel"]) == _bits(torch.minimum(qs[0], qs[1])) and _bits(rows["q_sel"]) == _bits(torch.where(sel2, qs[1], qs[0])), what
        dq_sel = torch.where(sel2[:, None], rows["dq2_da"], rows["dq1_da"])
    else:
        assert _bits(rows["q_sel"]) == _bits(qs[0]), what
        dq_sel = rows["dq1_da"]
    # (a tensor divided by a Python number is multiplied by its rounded reciprocal in torch: the quotients are formed against a tensor of n)
    assert _bits(rows["g_action"]) == _bits((-dq_sel) / torch.full_like(dq_sel, float(n))), what
    got = _grads_np(grads)
    if squashed:
        composed = env.squashed_grad_torch(actor, obs, eps, g_action=rows["g_action"], g_logp=torch.full((n,), alpha, device="cuda") / torch.full((n,), float(n), device="cuda"))
    else:
        composed = env.policy_action_grad_torch(actor, obs, rows["g_action"], eps)
    composed = _grads_np(composed)
    assert set(got) == set(composed) and len(got) == 2 * (actor.n_hidden + 1) + (not squashed), what
    for k in got:
        if exact:
            assert got[k].tobytes() == composed[k].tobytes(), (what, k)
        assert np.abs(got[k]).max() > 0 or (k == "log_std" and eps is None), (what, k)
    return got, composed


def _run(env, actor, q, obs, eps, form, q_select, n_critics, **more):
    two = _two(form, n_critics, q_select)
    rows = more.pop("rows", None) or _rows(obs.shape[0], two)
    kw = dict(alpha=ALPHA if form == "squashed" else 0.0, q_select=q_select, rows=rows)
    kw.update(more)
    grads, stats = env.q_actor_grad_torch(actor, q, obs, eps, **kw)
    return grads, stats, rows, two


@pytest.mark.parametrize("gc", grad_cases(), ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_fused_outputs_are_the_composed_calls_bits_and_the_models_values(gc):
    """1 .. 9 for every case: n = 1, 200 and 2 049 over the five nets, the second row tile at hidden 128 and the three mixed pairs"""
    import torch
    obs_dim, n, a_net, q_net, n_critics, form, activation, eps_given, q_select = gc
    assert n != BIG_N or (a_net[0] == 128 and n > 256 * GRAD_ROWS[4])
    env = _env_for(obs_dim, n)
    c = grad_case(obs_dim, n, a_net, q_net, n_critics, form, activation, eps_given)
    actor, q = _handles(env, c, activation)
    obs, eps = _dev(c["obs"]), _dev(c["eps"]) if eps_given else None
    grads, stats, rows, two = _run(env, actor, q, obs, eps, form, q_select, n_critics)
    torch.cuda.synchronize()
    exact = same_tile(a_net, q_net)
    alpha = ALPHA if form == "squashed" else 0.0
    got, composed = _check_composed(env, actor, q, obs, eps, alpha, two, grads, rows, gc, exact)
    assert not any(t.isnan().any() for t in rows.values())
    # 6: the model
    m64, m32 = _models(gc)
    names = [k for k in ROWS if k in rows]
    got_rows = dict(zip(names, _np(*[rows[k] for k in names])))
    for k in names:
        _close(got_rows[k], m32["rows"][k], m64["rows"][k], gc + (k,))
    s = _np(stats)[0]
    for k, name in enumerate(STATS):
        _close(s[k], m32["stats"][k], m64["stats"][k], gc + (name,))
    _check_grads(got, flat(m32), flat(m64), gc)
    if not exact:  # 5, the unequal mixed pairs: the composed call's other grouping of the same sums under the same rule
        _check_grads(composed, flat(m32), flat(m64), gc + ("composed",))
    if two:
        assert np.array_equal(got_rows["q2"] < got_rows["q1"], m64["sel2"]) and s[5] == np.float32(m64["sel2"].sum()) / np.float32(n), gc
    assert s[7] == max(np.abs(got_rows[k]).max() for k in ("dq1_da", "dq2_da") if k in got_rows), gc  # dq_da_abs_max: exactly the largest entry
    if form == "squashed":
        assert s[8] == -(s[1] + np.float32(-2.0)), gc
    else:
        assert s[8] == 0 and s[1] == 0 and s[0] == -s[4], gc
    # 7
    if not two:
        assert s[3] == 0 and s[5] == 0 and _bits(rows["q_sel"]) == _bits(rows["q1"]), gc
    first, first_stats = {k: _bits(t) for k, t in rows.items()}, _bits(stats)
    if n_critics == 2 and two:
        g0, s0, r0, _ = _run(env, actor, q, obs, eps, form, 0, n_critics)
        z = _np(s0)[0]
        assert z[3] == 0 and z[5] == 0 and z[2] == s[2] and z[4] == z[2] and _bits(r0["q_sel"]) == first["q1"] and set(r0) == set(ROWS) - {"q2", "dq2_da"}, gc
    # 8
    if form == "squashed":
        g2, s2, r2, _ = _run(env, actor, q, obs, eps, form, q_select, n_critics, alpha=torch.tensor([ALPHA], device="cuda"))
        assert _bits(s2) == first_stats and all(_bits(r2[k]) == first[k] for k in r2), gc
        for k, v in _grads_np(g2).items():
            assert v.tobytes() == got[k].tobytes(), (gc, k)
    # 9
    actor.workspace.view(torch.float32).fill_(float("nan"))
    for t in [x for pair in grads["actor"] for x in pair] + [stats] + list(rows.values()) + ([grads["log_std"]] if "log_std" in grads else []):
        t.fill_(float("nan"))
    again_g, again_s, _, _ = _run(env, actor, q, obs, eps, form, q_select, n_critics, rows=rows, out=grads, stats=stats)
    again = _grads_np(again_g)
    assert again_g is grads and again_s is stats and _bits(stats) == first_stats and not stats.isnan().any()
    for k in got:
        assert not np.isnan(again[k]).any() and again[k].tobytes() == got[k].tobytes(), (gc, k)
    assert all(_bits(rows[k]) == first[k] for k in rows)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", width_cases())
def test_both_kernels_at_every_width_class(hidden, n_hidden, activation):
    """12: the family's width test (tests/net_widths.py): every class NT = 1 .. 4 and each class's widest net, three hidden layers on the
    4P id, at n = 200 -- ragged row tiles in every class -- both actor forms, held to the single calls' bits, which
    tests/test_gpu_net_widths.py holds to their models at the same widths; and the workspace query's terms"""
    env_id = ids_of(hidden, n_hidden)[0]
    env = make(env_id, WIDTH_N)
    assert env.obs_dim == OBS_DIM[env_id] and not env.discrete
    for form, n_critics, q_select in (("squashed", 2, None), ("gaussian", 2, 1), ("gaussian", 1, None)):
        c = actor_case(env.obs_dim, WIDTH_N, (hidden, n_hidden), (hidden, n_hidden), n_critics, form, activation, True, seed=WIDTH_N + hidden)
        actor, q = _handles(env, c, activation)
        obs, eps = _dev(c["obs"]), _dev(c["eps"])
        grads, stats, rows, two = _run(env, actor, q, obs, eps, form, q_select, n_critics)
        _check_composed(env, actor, q, obs, eps, ALPHA if form == "squashed" else 0.0, two, grads, rows, (hidden, n_hidden, activation, form), True)
        ref = C.byref(actor.struct)
        need = env._lib.sg_q_actor_grad_workspace_bytes(env._h, ref if form == "squashed" else None, None if form == "squashed" else ref,
                                                        C.byref(q.struct), WIDTH_N)
        groups = -(-WIDTH_N // GRAD_ROWS[-(-hidden // 32)])
        own = "sg_squashed_grad_workspace_bytes" if form == "squashed" else "sg_policy_grad_workspace_bytes"
        assert need == getattr(env._lib, own)(env._h, ref, WIDTH_N) + 32 * groups <= actor.workspace.numel()
    env.check_status()
    env.close()


def test_a_trained_regime_case_equals_the_model():
    """13: tests/net_regimes.py's squashed actor and q critics -- hidden gains of 5, Q values in the hundreds, the default clamp -- under
    the same rule; tests/test_q_actor.py checks its 1 % cap on the CPU"""
    c, activation, eps_given, q_select = regime_case()
    n = c["obs"].shape[0]
    env = make(c["env_id"], n)
    actor, q = _handles(env, c, activation, bounds=c["bounds"])
    obs, eps = _dev(c["obs"]), _dev(c["eps"])
    grads, stats, rows, two = _run(env, actor, q, obs, eps, "squashed", q_select, 2)
    got, _ = _check_composed(env, actor, q, obs, eps, ALPHA, two, grads, rows, ("regime",), True)
    m64, m32 = regime_reference(np.float64), regime_reference(np.float32)
    for k in ROWS:
        _close(_np(rows[k])[0], m32["rows"][k], m64["rows"][k], ("regime", k))
    s = _np(stats)[0]
    for k, name in enumerate(STATS):
        _close(s[k], m32["stats"][k], m64["stats"][k], ("regime", name))
    _check_grads(got, flat(m32), flat(m64), ("regime",))
    env.check_status()
    env.close()


def test_the_whole_update_replays_as_a_graph():
    """10: after one warm-up, the noise drawn into eps, q_actor_update_torch, the three-line temperature step and q_update_torch are
    captured; two replays change the actor's parameters and alpha; alpha written as 0 makes the next replay's loss -q_sel_mean to the
    bit; a workspace that would have to grow inside a capture raises with nothing written"""
    import torch
    n, lr = 256, 1e-2
    env = make(GOAL, n)
    c = actor_case(env.obs_dim, n, (64, 2), (64, 2), 2, "squashed", "relu", True, seed=7)
    sp, q = _handles(env, c, "relu")
    target = env.q_torch(critics=[[(_dev(W), _dev(b)) for W, b in net] for net in c["critics"]], activation="relu")
    opt_a, opt_q = env.adam_torch(sp, lr=1e-3), env.adam_torch(q, lr=1e-3)
    rng = np.random.default_rng(3)
    f = lambda *shape: _dev(rng.standard_normal(shape).astype(np.float32))
    obs = _dev(c["obs"])
    batch = dict(obs=obs, action=torch.tanh(f(n, 2)), reward=f(n), next_obs=f(n, env.obs_dim),
                 terminated=_dev((rng.uniform(size=n) < 0.1).astype(np.uint8)), discount=torch.full((n,), 0.99, device="cuda"))
    next_action, next_logp = torch.tanh(f(n, 2)), f(n)
    eps = torch.empty(n, 2, device="cuda")
    log_alpha = torch.tensor([np.log(ALPHA)], dtype=torch.float32, device="cuda")
    alpha = log_alpha.exp()

    def step(a_out, c_out):
        eps.normal_()
        a_stats, a_rows, a_grads = env.q_actor_update_torch(sp, q, opt_a, obs, eps, alpha=alpha, **a_out)
        log_alpha.sub_(lr * a_stats[8:9])  # the temperature step, the caller's three lines
        alpha.copy_(log_alpha.exp())
        c_stats, _, c_grads = env.q_update_torch(q, target, opt_q, batch, next_action, next_logp=next_logp, alpha=alpha, tau=0.005, **c_out)
        return dict(rows=a_rows, grads=a_grads, stats=a_stats), dict(grads=c_grads, stats=c_stats)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream: sizes the workspaces, makes the buffers
        a_out, c_out = step(dict(rows=dict(q_sel=torch.empty(n, device="cuda"))), {})
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(a_out, c_out)
    torch.cuda.synchronize()
    assert int(opt_a.state[0, 0]) == 1  # (capturing ran nothing)
    stats = a_out["stats"]
    seen, alphas, noise = [[t.detach().clone() for t in sp.tensors]], [alpha.clone()], [eps.clone()]
    for rep in range(2):
        stats.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        seen.append([t.detach().clone() for t in sp.tensors])
        alphas.append(alpha.clone())
        noise.append(eps.clone())
        assert all(not torch.equal(a, b) for a, b in zip(seen[-2], seen[-1])) and int(opt_a.state[0, 0]) == 2 + rep == int(opt_q.state[0, 0])
        assert not stats.isnan().any() and not torch.equal(alphas[-2], alphas[-1]) and not torch.equal(noise[-2], noise[-1])
        assert stats[0] != -stats[4]
    alpha.fill_(0.0)  # read on the device by the actor's call of the next replay, before the temperature step writes it again
    graph.replay()
    torch.cuda.synchronize()
    s = _np(stats)[0]
    assert s[0] == -s[4] and s[4] != 0, s
    assert float(alpha) > 0
    env.check_status()
    fresh = env.squashed_policy_torch(actor=[(sp.tensors[l], sp.tensors[l + 1]) for l in range(0, len(sp.tensors), 2)], log_std_bounds=BOUNDS)
    stats.fill_(7.0)
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.q_actor_grad_torch(fresh, q, obs, eps, out=a_out["grads"], stats=stats)
    torch.cuda.synchronize()
    assert fresh.workspace is None and (stats == 7).all()
    env.check_status()
    env.close()


def test_native_refusals():
    """11: every refusal returns the error with a message that names the argument and leaves the outputs untouched; the workspace
    query's terms at n = 40, 257 and 10^7"""
    import torch
    from space_gym_amd import _native
    n = 40
    env = make(GOAL, n)
    c = actor_case(env.obs_dim, n, (16, 1), (16, 1), 2, "squashed", "relu", True, seed=16)
    g = actor_case(env.obs_dim, n, (16, 1), (16, 1), 1, "gaussian", "relu", True, seed=16)
    sp, q = _handles(env, c, "relu")
    pol, single = _handles(env, g, "relu")
    f = lambda *shape: torch.full(shape, 7.0, device="cuda")
    obs, eps, alpha, spare = f(n, env.obs_dim), f(n, 2), f(1), f(n, 2)
    grads, stats = env.q_actor_grad_torch(sp, q, obs, eps)
    g_grads, _ = env.q_actor_grad_torch(pol, q, obs, eps, alpha=0.0)
    every = [x for pair in grads["actor"] + g_grads["actor"] for x in pair] + [stats, g_grads["log_std"]]
    for t in every:
        t.fill_(7.0)
    ws = sp.workspace
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()
    ref = lambda h: C.byref(h.struct) if h is not None else None
    query = lambda e, a, b, qq, rows: lib.sg_q_actor_grad_workspace_bytes(e._h, ref(a), ref(b), ref(qq), rows)
    need = query(env, sp, None, q, n)
    per_group = 4 * (sum(int(W.size + b.size) for W, b in c["actor"]) + 2)  # (the layout's two log_std floats: unused by this form)
    assert per_group == lib.sg_squashed_grad_workspace_bytes(env._h, ref(sp), n)
    assert need == per_group + 32 <= ws.numel()  # one workgroup's partial sums and its eight statistics sums
    assert query(env, sp, None, q, 257) == 2 * (per_group + 32) and query(env, sp, None, q, 10 ** 7) == 256 * (per_group + 32)
    assert query(env, None, pol, q, 257) == lib.sg_policy_grad_workspace_bytes(env._h, ref(pol), 257) + 2 * 32
    said = lambda e, match: match in lib.sg_last_error(e._h)
    for bad in (0, 2 ** 31):
        assert query(env, sp, None, q, bad) == 0 and said(env, b"n must be")
    assert query(env, sp, pol, q, n) == 0 and said(env, b"exactly one") and query(env, None, None, q, n) == 0 and said(env, b"exactly one")
    assert query(env, sp, None, None, n) == 0 and said(env, b"null qnet")

    def cfg(**over):
        k = _native.SgQActorConfig()
        lib.sg_q_actor_config_init(C.byref(k))
        assert (k.struct_size, k.alpha, k.target_entropy, k.q_select, tuple(k.reserved)) == (24, np.float32(0.2), -2.0, -1, (0, 0))
        for name, v in over.items():
            setattr(k, name, v)
        return k

    def gr(gaussian=False, **over):
        cls = _native.SgPolicyGrads if gaussian else _native.SgSquashedGrads
        out = cls(struct_size=C.sizeof(cls))
        for l, (w, b) in enumerate((g_grads if gaussian else grads)["actor"]):
            out.actor.weight[l], out.actor.bias[l] = w.data_ptr(), b.data_ptr()
        if gaussian:
            out.log_std = g_grads["log_std"].data_ptr()
        for k, v in over.items():
            setattr(out, k, v)
        return out

    def call(match, e=env, actor=sp, qq=q, k=True, rows=n, o=obs, ep=eps, al=None, g=True, st=stats, r=None, w=ws, wbytes=None, at=0):
        gaussian = actor is pol
        k = cfg(**(dict(alpha=0.0) if gaussian else {})) if k is True else k
        g = gr(gaussian) if g is True else g
        fn = lib.sg_q_actor_gaussian_grad_device if gaussian else lib.sg_q_actor_squashed_grad_device
        rc = fn(e._h, ref(actor), ref(qq), C.byref(k) if k is not None else None, rows, ptr(o), ptr(ep), ptr(al),
                C.byref(g) if g is not None else None, ptr(st), C.byref(r) if r is not None else None,
                C.c_void_p(w.data_ptr() + at) if w is not None else None, ws.numel() - at if wbytes is None else wbytes, s)
        assert rc == -1 and said(e, match), lib.sg_last_error(e._h)

    call(b"null policy", actor=None)
    call(b"null qnet", qq=None)
    for h, field, bad, good, match in ((sp, "hidden", 129, 16, b"hidden"), (sp, "n_hidden", 0, 1, b"n_hidden"), (sp, "reserved", 1, 0, b"reserved"),
                                       (sp, "log_std_min", 3.0, BOUNDS[0], b"log_std bounds"), (q, "n_critics", 3, 2, b"n_critics"),
                                       (q, "activation", 2, 1, b"activation"), (q, "struct_size", 8, C.sizeof(_native.SgQnet), b"struct_size")):
        setattr(h.struct, field, bad)
        call(match)
        setattr(h.struct, field, good)
    pol.struct.head = 6
    call(b"head", actor=pol)
    pol.struct.head = 2
    call(b"null cfg", k=None)
    call(b"struct_size", k=cfg(struct_size=8))
    for word in ((1, 0), (0, 1)):
        call(b"reserved", k=cfg(reserved=(C.c_int32 * 2)(*word)))
    for bad in (-2, 2):
        call(b"q_select must be", k=cfg(q_select=bad))
    call(b"the qnet has one critic", qq=single, k=cfg(q_select=1))
    for bad in (-0.1, float("nan")):
        call(b"alpha must be >= 0", k=cfg(alpha=bad))
    call(b"the Gaussian form has no log-prob term", actor=pol, k=cfg(alpha=0.2))
    call(b"the Gaussian form has no log-prob term", actor=pol, al=alpha)
    call(b"target_entropy is NaN", k=cfg(target_entropy=float("nan")))
    call(b"n must be", rows=0)
    call(b"n must be", rows=2 ** 31)
    call(b"null obs", o=None)
    call(b"null stats_out", st=None)
    call(b"null grads", g=None)
    call(b"struct_size", g=gr(struct_size=8))
    call(b"reserved", g=gr(reserved=1))
    hole = gr()
    hole.actor.bias[1] = None
    call(b"layer 1 of the actor", g=hole)
    call(b"null log_std gradient", actor=pol, g=gr(True, log_std=None))
    for k in ("q2", "dq2_da"):
        call(b"critic 2 does not run", k=cfg(q_select=0), r=_native.SgQActorRows(**{k: spare.data_ptr()}))
        call(b"critic 2 does not run", qq=single, r=_native.SgQActorRows(**{k: spare.data_ptr()}))
        call(b"critic 2 does not run", actor=pol, r=_native.SgQActorRows(**{k: spare.data_ptr()}))
    call(b"null workspace", w=None)
    call(b"workspace of", wbytes=need - 1)
    call(b"aligned to 4", w=torch.empty(need + 8, dtype=torch.uint8, device="cuda"), wbytes=need, at=2)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in every) and (spare == 7).all()
    env.check_status()
    # a discrete id: refused by the library and by the method
    dis = make(DISCRETE, n)
    call(b"discrete", e=dis)
    assert query(dis, sp, None, q, n) == 0 and said(dis, b"discrete")
    with pytest.raises(ValueError, match="discrete ids are not served"):
        dis.q_actor_grad_torch(sp, q, obs)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in every)
    dis.check_status()
    dis.close()
    # the handles still work: an alpha on the device, the Gaussian form on one critic
    env.q_actor_grad_torch(sp, q, obs, eps, alpha=alpha, out=grads, stats=stats)
    torch.cuda.synchronize()
    assert not stats.isnan().any() and float(stats[5]) in (0.0, 1.0)  # (equal rows: one critic is the smaller on all of them)
    _, s1 = env.q_actor_grad_torch(pol, single, obs, None, alpha=0.0, out=g_grads)
    torch.cuda.synchronize()
    assert not s1.isnan().any() and not g_grads["log_std"].any()
    env.check_status()
    env.close()


def test_report_the_worst_error_to_tolerance_ratios():
    """prints the three largest error / tolerance ratios the tests above met (they asserted each one at its place)"""
    WORST.sort(key=lambda r: -r[0])
    for ratio, err, tol, what in WORST[:3]:
        print("error / tolerance %.3f (error %.3g, tolerance %.3g) at" % (ratio, err, tol), what)
    assert all(r[0] <= 1.0 for r in WORST)
