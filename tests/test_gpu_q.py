"""GPU tests of q_torch / q_evaluate_raw_torch / q_grad_torch / q_evaluate_torch and policy_action_torch / policy_action_raw_torch /
policy_action_grad_torch (sg_q_evaluate_device / sg_q_grad_device / sg_policy_action_device / sg_policy_action_grad_device) against the
NumPy model tests/q_model.py.

Forward tolerances are DESIGN section 17's rule: 8 x max|float32 CPU - float64| + 1e-6 (_tol), computed here.  A gradient tensor's
tolerance -- a parameter's or the [n, 2] action gradient's -- is section 18's: 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|), G32seq the
model in float32 with the batch summed sequentially (the action gradient has no sum over the batch: there it is the float32 model as it
is); every such tolerance must also be at most 1 % of max|G64| of its tensor, so that a wrong index cannot hide.  A gradient that is
identically zero in the model (a NULL g) must be exactly zero on the device.

Row counts: 1 (a partial wave), 200 (no multiple of a workgroup), 2049 (9 .. 33 workgroups whose partials are reduced), and for the
smallest workgroup (64 rows) 256 x 64 + 300 rows, where the capped grid makes workgroups take a second row tile."""
import ctypes as C

import numpy as np
import pytest

from policy_model import random_policy
from q_model import action as action_model
from q_model import flat, grad_tolerances, q_evaluate, q_flat, random_qnet
from test_gpu_policy import DISCRETE, GOAL, KEPLER, NETS, _dev, _handle, _np, _tol, make

pytestmark = pytest.mark.gpu

NS = [1, 200, 2049]


def _q_handle(env, critics, activation="relu"):
    return env.q_torch(critics=[[(_dev(W), _dev(b)) for W, b in layers] for layers in critics], activation=activation)


def _case(env_id, n, hidden, n_hidden, seed, n_critics=2):
    env = make(env_id, n)
    rng = np.random.default_rng(seed)
    critics = random_qnet(rng, env.obs_dim, hidden, n_hidden, n_critics)
    obs = rng.standard_normal((n, env.obs_dim)).astype(np.float32)
    act = rng.standard_normal((n, 2)).astype(np.float32)
    return env, rng, critics, obs, act


def _q_grads_np(out):
    import torch
    torch.cuda.synchronize()
    return q_flat(dict(critics=[[(w.cpu().numpy(), b.cpu().numpy()) for w, b in pairs] for pairs in out["critics"]]))


def _check_grads(got, g32, g64, what, worst):
    tol = grad_tolerances(g32, g64)
    assert set(got) == set(g64), what
    for k in g64:
        top = float(np.abs(g64[k]).max())
        if top == 0.0:
            assert not got[k].any(), (what, k)
            continue
        err = float(np.abs(got[k].astype(np.float64) - g64[k]).max())
        worst.append((err / tol[k], err, tol[k], top, what, k))
        assert tol[k] <= 0.01 * top, (what, k, tol[k], top)
        assert err <= tol[k], (what, k, err, tol[k])


def _report(worst):
    worst.sort(reverse=True)
    for ratio, err, tol, top, what, k in worst[:3]:
        print("gradient error / tolerance %.3f (error %.3g, tolerance %.3g, max|G64| %.3g) at" % (ratio, err, tol, top), what, k)


@pytest.mark.parametrize("n", NS)
def test_forward_equals_the_model_and_a_shard_gives_the_same_bits(n):
    """1: q1, q2 within _tol of the float64 model, every net, both activations spread over the nets; rows [lo:hi] alone: the same bits"""
    worst = 0.0
    for i, (hidden, n_hidden) in enumerate(NETS):
        activation = ("tanh", "relu")[i % 2]
        env, rng, critics, obs, act = _case(GOAL if i % 2 == 0 else KEPLER, n, hidden, n_hidden, seed=n + hidden)
        h = _q_handle(env, critics, activation)
        q1, q2 = _np(*env.q_evaluate_raw_torch(h, _dev(obs), _dev(act)))
        m64 = q_evaluate(critics, obs, act, activation=activation, grads=False)
        m32 = q_evaluate(critics, obs, act, activation=activation, grads=False, dtype=np.float32)
        for c, q in enumerate((q1, q2)):
            t = _tol(m32["q"][c], m64["q"][c])
            worst = max(worst, t)
            assert np.abs(q - m64["q"][c]).max() <= t, (n, hidden, n_hidden, activation, c, np.abs(q - m64["q"][c]).max(), t)
        lo, hi = n // 3, n // 3 + max(1, n // 2)
        s1, s2 = _np(*env.q_evaluate_raw_torch(h, _dev(obs[lo:hi]), _dev(act[lo:hi])))
        assert s1.tobytes() == q1[lo:hi].tobytes() and s2.tobytes() == q2[lo:hi].tobytes()
        one = _q_handle(env, critics[:1], activation)  # one critic: the same q1, no q2
        o1, o2 = env.q_evaluate_raw_torch(one, _dev(obs), _dev(act))
        assert o2 is None and _np(o1)[0].tobytes() == q1.tobytes()
        env.check_status()
        env.close()
    print("largest forward tolerance (8 x |float32 CPU - float64| + 1e-6):", n, "%.3g" % worst)


def _run_grad_case(env_id, n, hidden, n_hidden, activation, worst, which=("both", "q1", "q2"), n_critics=2):
    env, rng, critics, obs, act = _case(env_id, n, hidden, n_hidden, seed=n + hidden, n_critics=n_critics)
    g = [rng.standard_normal(n).astype(np.float32) for _ in range(n_critics)]
    h = _q_handle(env, critics, activation)
    d_obs, d_act = _dev(obs), _dev(act)
    # the model once per critic (the critics share nothing): a selection's reference is put together from these
    ref = {dt: [q_evaluate([critics[c]], obs, act, g[c], activation=activation, dtype=dt) for c in range(n_critics)] for dt in (np.float64, np.float32)}
    for sel in which:
        on = [sel in ("both", "q%d" % (c + 1)) for c in range(n_critics)]
        out = env.q_grad_torch(h, d_obs, d_act, *[_dev(g[c]) if on[c] else None for c in range(n_critics)], action_grad=True)
        assert len(out["critics"]) == n_critics
        got = _q_grads_np(out)
        got["action"] = out["action"].cpu().numpy()
        want = {}
        for dt in ref:
            named, da = {}, np.zeros((n, 2), dt)
            for c in range(n_critics):
                for k, v in q_flat(ref[dt][c]).items():
                    named[k.replace("critic0", "critic%d" % c)] = v if on[c] else np.zeros_like(v)  # a critic without g: exactly zero
                if on[c]:
                    da = da + ref[dt][c]["action"]  # the first critic's term before the second's
            named["action"] = da
            want[dt] = named
        _check_grads(got, want[np.float32], want[np.float64], (env_id, n, hidden, n_hidden, activation, sel, n_critics), worst)
    env.check_status()
    env.close()


@pytest.mark.parametrize("n", NS)
def test_parameter_and_action_gradients_equal_the_model(n):
    """2, 3: dense random g_q1, g_q2 together and each alone, every net, both activations spread over the nets; one critic only"""
    worst = []
    for i, (hidden, n_hidden) in enumerate(NETS):
        _run_grad_case(GOAL if i % 2 == 0 else KEPLER, n, hidden, n_hidden, ("tanh", "relu")[i % 2], worst)
    _run_grad_case(GOAL, n, 33, 2, "tanh", worst, which=("q1",), n_critics=1)
    _report(worst)


def test_gradients_when_workgroups_take_a_second_row_tile():
    """2, past the grid cap: 256 workgroups of 64 rows (the smallest R) and 300 rows more, so the first workgroups load their partial
    sums back"""
    worst = []
    _run_grad_case(GOAL, 256 * 64 + 300, 97, 1, "tanh", worst, which=("both",))
    _report(worst)


def test_action_gradient_is_a_function_of_the_row_alone():
    """3: params off gives the same bits as params on; rows [lo:hi] evaluated alone give the same bits; both g None: exact zeros"""
    n = 2049
    for hidden, n_hidden, activation in ((33, 2, "relu"), (128, 3, "tanh")):
        env, rng, critics, obs, act = _case(GOAL, n, hidden, n_hidden, seed=31 + hidden)
        h = _q_handle(env, critics, activation)
        g1, g2 = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
        d = _dev
        full = env.q_grad_torch(h, d(obs), d(act), d(g1), d(g2), action_grad=True)
        frozen = env.q_grad_torch(h, d(obs), d(act), d(g1), d(g2), params=False, action_grad=True)
        assert frozen["critics"] is None
        a_full, a_frozen = _np(full["action"], frozen["action"])
        assert a_full.tobytes() == a_frozen.tobytes() and np.abs(a_full).max() > 1e-3
        for lo, hi in ((0, 1), (700, 1900), (n - 65, n)):
            part = env.q_grad_torch(h, d(obs[lo:hi]), d(act[lo:hi]), d(g1[lo:hi]), d(g2[lo:hi]), params=False, action_grad=True)
            assert _np(part["action"])[0].tobytes() == a_full[lo:hi].tobytes(), (hidden, lo, hi)
            both = env.q_grad_torch(h, d(obs[lo:hi]), d(act[lo:hi]), d(g1[lo:hi]), d(g2[lo:hi]), action_grad=True)
            assert _np(both["action"])[0].tobytes() == a_full[lo:hi].tobytes(), (hidden, lo, hi)
        import torch
        pre = dict(action=torch.full((n, 2), float("nan"), device="cuda"))
        zero = env.q_grad_torch(h, d(obs), d(act), params=False, action_grad=True, out=pre)
        assert zero["action"] is pre["action"] and not _np(zero["action"])[0].any()
        zero = env.q_grad_torch(h, d(obs), d(act), action_grad=True)
        assert not _np(zero["action"])[0].any() and not any(v.any() for v in _q_grads_np(zero).values())
        env.check_status()
        env.close()


@pytest.mark.parametrize("env_id", [GOAL, KEPLER])
def test_actor_chain(env_id):
    """4: the action without eps is policy_act_torch(deterministic=True)'s bit for bit; with eps within _tol of the model; the
    gradients within section 18's rule, log_std included; the policy's critic slots are not touched"""
    import torch
    from space_gym_amd import _native
    n = 200
    env = make(env_id, n)
    rng = np.random.default_rng(41)
    obs = rng.standard_normal((n, env.obs_dim)).astype(np.float32)
    eps, ga = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    worst = []
    for i, (hidden, n_hidden) in enumerate(NETS):
        activation = ("tanh", "relu")[i % 2]
        pol = random_policy(rng, env.obs_dim, hidden, n_hidden, 2)
        h = _handle(env, pol, activation)
        what = (env_id, hidden, n_hidden, activation)
        det = _np(env.policy_act_torch(h, _dev(obs), deterministic=True)[0])[0]
        assert _np(env.policy_action_raw_torch(h, _dev(obs)))[0].tobytes() == det.tobytes(), what
        a = _np(env.policy_action_raw_torch(h, _dev(obs), _dev(eps)))[0]
        m64, m32 = action_model(pol, obs, eps, ga, activation=activation), action_model(pol, obs, eps, ga, activation=activation, dtype=np.float32)
        t = _tol(m32["action"], m64["action"])
        assert np.abs(a - m64["action"]).max() <= t, (what, np.abs(a - m64["action"]).max(), t)
        out = env.policy_action_grad_torch(h, _dev(obs), _dev(ga), _dev(eps))
        torch.cuda.synchronize()
        got = flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]], log_std=out["log_std"].cpu().numpy()))
        _check_grads(got, flat(m32), flat(m64), what, worst)
        none = env.policy_action_grad_torch(h, _dev(obs), _dev(ga))  # no noise: log_std gets exactly nothing
        assert not _np(none["log_std"])[0].any()
        p64 = flat(action_model(pol, obs, None, ga, activation=activation))
        p32 = flat(action_model(pol, obs, None, ga, activation=activation, dtype=np.float32))
        torch.cuda.synchronize()
        _check_grads(flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in none["actor"]], log_std=none["log_std"].cpu().numpy())),
                     p32, p64, what + ("no eps",), worst)
    # the critic's slots of an sg_policy_grads are neither read nor written: NaN-filled tensors behind them stay NaN
    L = h.n_hidden + 1
    g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
    crit = [(torch.full_like(h.tensors[2 * L + 2 * l], float("nan")), torch.full_like(h.tensors[2 * L + 2 * l + 1], float("nan"))) for l in range(L)]
    for l in range(L):
        g.actor.weight[l], g.actor.bias[l] = out["actor"][l][0].data_ptr(), out["actor"][l][1].data_ptr()
        g.critic.weight[l], g.critic.bias[l] = crit[l][0].data_ptr(), crit[l][1].data_ptr()
    g.log_std = out["log_std"].data_ptr()
    before = flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]], log_std=out["log_std"].cpu().numpy()))
    for w, b in out["actor"]:
        w.fill_(float("nan"))
        b.fill_(float("nan"))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    d_obs, d_eps, d_ga = _dev(obs), _dev(eps), _dev(ga)
    assert env._lib.sg_policy_action_grad_device(env._h, C.byref(h.struct), n, ptr(d_obs), ptr(d_eps), ptr(d_ga), C.byref(g), ptr(h.workspace),
                                                 h.workspace.numel(), env._stream()) == 0
    torch.cuda.synchronize()
    after = flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]], log_std=out["log_std"].cpu().numpy()))
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)
    assert all(w.isnan().all() and b.isnan().all() for w, b in crit)
    _report(worst)
    env.check_status()
    env.close()


def test_results_are_deterministic_and_written_not_accumulated():
    """5: two calls give the same bits; buffers (and the workspace) pre-filled with NaN come out finite and equal"""
    import torch
    n = 2049
    for hidden, n_hidden in ((33, 2), (128, 3)):
        env, rng, critics, obs, act = _case(GOAL, n, hidden, n_hidden, seed=6)
        h = _q_handle(env, critics)
        g = [_dev(rng.standard_normal(n).astype(np.float32)) for _ in range(2)]
        first = env.q_grad_torch(h, _dev(obs), _dev(act), *g, action_grad=True)
        a, a_act = _q_grads_np(first), first["action"].cpu().numpy()
        h.workspace.view(torch.float32).fill_(float("nan"))
        for t in [x for pairs in first["critics"] for pair in pairs for x in pair] + [first["action"]]:
            t.fill_(float("nan"))
        again = env.q_grad_torch(h, _dev(obs), _dev(act), *g, action_grad=True, out=first)
        b, b_act = _q_grads_np(again), again["action"].cpu().numpy()
        for k in a:
            assert not np.isnan(b[k]).any() and a[k].tobytes() == b[k].tobytes(), (hidden, k)
        assert not np.isnan(b_act).any() and a_act.tobytes() == b_act.tobytes()
        pol = random_policy(rng, env.obs_dim, hidden, n_hidden, 2)
        hp = _handle(env, pol)
        eps, ga = _dev(rng.standard_normal((n, 2)).astype(np.float32)), _dev(rng.standard_normal((n, 2)).astype(np.float32))
        o1 = env.policy_action_grad_torch(hp, _dev(obs), ga, eps)
        keep = [t.clone() for pair in o1["actor"] for t in pair] + [o1["log_std"].clone()]
        hp.workspace.view(torch.float32).fill_(float("nan"))
        for t in [x for pair in o1["actor"] for x in pair] + [o1["log_std"]]:
            t.fill_(float("nan"))
        o2 = env.policy_action_grad_torch(hp, _dev(obs), ga, eps, out=o1)
        now = [t for pair in o2["actor"] for t in pair] + [o2["log_std"]]
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) and not y.isnan().any() for x, y in zip(keep, now))
        env.close()


def _modules(layers_list, activation, dtype, device):
    import torch
    def net(layers):
        mods = []
        for l, (W, b) in enumerate(layers):
            lin = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(W))
                lin.bias.copy_(torch.from_numpy(b))
            mods.append(lin)
            if l < len(layers) - 1:
                mods.append(torch.nn.Tanh() if activation == "tanh" else torch.nn.ReLU())
        return torch.nn.Sequential(*mods).to(dtype=dtype, device=device)
    return [net(layers) for layers in layers_list]


def test_td3_step_through_autograd():
    """6: the critic loss and the actor loss of a TD3 update through q_evaluate_torch / policy_action_torch and backward(), every .grad
    against float64 CPU torch modules fed the same numbers, under the per-tensor rule with g = d loss / d outputs"""
    import torch
    n = 200
    env, rng, critics, obs, act = _case(GOAL, n, 64, 2, seed=14)
    pol = random_policy(rng, env.obs_dim, 64, 2, 2, critic=False)
    y = rng.standard_normal(n).astype(np.float32)
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    pairs = lambda net: [(m.weight, m.bias) for m in lin(net)]
    named = lambda nets, prefix: {f"{prefix}{c}.{l}.{kind}": getattr(m, kind).grad.detach().cpu().numpy()
                                  for c, net in enumerate(nets) for l, m in enumerate(lin(net)) for kind in ("weight", "bias")}
    # float64 on the CPU
    c64 = _modules(critics, "relu", torch.float64, "cpu")
    a64 = _modules([pol["actor"]], "tanh", torch.float64, "cpu")[0]
    ls64 = torch.from_numpy(pol["log_std"]).double().requires_grad_()
    x, a, t = torch.from_numpy(obs).double(), torch.from_numpy(act).double(), torch.from_numpy(y).double()
    q = [net(torch.cat([x, a], 1))[:, 0] for net in c64]
    for v in q:
        v.retain_grad()
    ((q[0] - t).square().mean() + (q[1] - t).square().mean()).backward()
    critic64 = named(c64, "critic")
    g_critic = [v.grad.numpy().astype(np.float32) for v in q]
    for net in c64:
        net.zero_grad()
    api = a64(x)
    api.retain_grad()
    q1pi = c64[0](torch.cat([x, api], 1))[:, 0]
    q1pi.retain_grad()
    (-q1pi.mean()).backward()
    actor64 = {**named([a64], "actor"), **named(c64[:1], "critic")}
    g_q1pi, g_api, api_np = q1pi.grad.numpy().astype(np.float32), api.grad.numpy().astype(np.float32), api.detach().numpy().astype(np.float32)
    # the float32 sequential model with the same g: the yardstick
    critic32 = q_flat(q_evaluate(critics, obs, act, *g_critic, dtype=np.float32))
    actor32 = {**{k.replace("actor.", "actor0."): v for k, v in flat(action_model(pol, obs, None, g_api, dtype=np.float32)).items() if k != "log_std"},
               **{k: v for k, v in q_flat(q_evaluate(critics[:1], obs, api_np, g_q1pi, dtype=np.float32)).items()}}
    # the device
    cd = _modules(critics, "relu", torch.float32, "cuda")
    ad = _modules([pol["actor"]], "tanh", torch.float32, "cuda")[0]
    lsd = torch.nn.Parameter(_dev(pol["log_std"]))
    hq = env.q_torch(critics=[pairs(net) for net in cd], activation="relu")
    hp = env.policy_torch(actor=pairs(ad), log_std=lsd, activation="tanh")
    d_obs, d_act, d_y = _dev(obs), _dev(act), _dev(y)
    q1, q2 = env.q_evaluate_torch(hq, d_obs, d_act)
    assert q1.grad_fn is not None and q2.grad_fn is not None
    ((q1 - d_y).square().mean() + (q2 - d_y).square().mean()).backward()
    worst = []
    _check_grads(named(cd, "critic"), critic32, critic64, "critic loss", worst)
    for net in cd:
        net.zero_grad()
    q1pi_d, _ = env.q_evaluate_torch(hq, d_obs, env.policy_action_torch(hp, d_obs))
    (-q1pi_d.mean()).backward()
    got = {**named([ad], "actor"), **named(cd[:1], "critic")}  # the first critic's .grad from the actor loss is present, as torch's
    _check_grads(got, actor32, actor64, "actor loss", worst)
    assert lsd.grad is not None and not lsd.grad.any()  # no noise: nothing reaches log_std
    with torch.no_grad():
        p1, p2 = env.q_evaluate_torch(hq, d_obs, d_act)
    assert p1.grad_fn is None and not p1.requires_grad and torch.equal(p1, q1.detach())
    _report(worst)
    env.check_status()
    env.close()


def test_a_captured_update_replays_the_eager_results():
    """7: evaluate + grad + action-grad captured after a warm-up call, replayed on new contents of the same buffers; a workspace that
    would have to grow inside a capture raises and launches nothing"""
    import torch
    n = 2049
    env, rng, critics, obs, act = _case(GOAL, n, 64, 2, seed=15)
    pol = random_policy(rng, env.obs_dim, 64, 2, 2)
    hq, hp = _q_handle(env, critics), _handle(env, pol)
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    d_obs, d_act, d_eps = _dev(obs), _dev(act), _dev(draw(n, 2))
    g1, g2 = _dev(draw(n)), _dev(draw(n))
    side = torch.cuda.Stream()
    fwd = dict(q1=torch.empty(n, device="cuda"), q2=torch.empty(n, device="cuda"))
    a_out = torch.empty((n, 2), device="cuda")
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream
        out = env.q_grad_torch(hq, d_obs, d_act, g1, g2, action_grad=True)
        aout = env.policy_action_grad_torch(hp, d_obs, out["action"], d_eps)
    side.synchronize()

    def update():
        env.q_evaluate_raw_torch(hq, d_obs, d_act, out=fwd)
        env.q_grad_torch(hq, d_obs, d_act, g1, g2, action_grad=True, out=out)
        env.policy_action_raw_torch(hp, d_obs, d_eps, out=a_out)
        env.policy_action_grad_torch(hp, d_obs, out["action"], d_eps, out=aout)

    every = lambda: (list(fwd.values()) + [x for pairs in out["critics"] for pair in pairs for x in pair] + [out["action"], a_out]
                     + [x for pair in aout["actor"] for x in pair] + [aout["log_std"]])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        update()
    for _ in range(2):
        for t, shape in ((d_obs, obs.shape), (d_act, (n, 2)), (d_eps, (n, 2)), (g1, (n,)), (g2, (n,))):  # new contents, the same buffers
            t.copy_(_dev(draw(*shape)))
        update()
        torch.cuda.synchronize()
        want = [t.clone() for t in every()]
        for t in every():
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(w, t) and not t.isnan().any() for w, t in zip(want, every()))
    # fresh handles have no workspace: inside a capture the calls must raise before anything is enqueued
    hq2, hp2 = _q_handle(env, critics), _handle(env, pol)
    out["critics"][0][0][0].fill_(float("nan"))
    aout["log_std"].fill_(float("nan"))
    torch.cuda.synchronize()
    for call in (lambda: env.q_grad_torch(hq2, d_obs, d_act, g1, g2, out=dict(critics=out["critics"])),
                 lambda: env.policy_action_grad_torch(hp2, d_obs, d_act, d_eps, out=aout)):
        graph2 = torch.cuda.CUDAGraph()
        with pytest.raises(ValueError, match="warm-up"):
            with torch.cuda.graph(graph2, stream=side):
                call()
        torch.cuda.synchronize()
    assert hq2.workspace is None and hp2.workspace is None
    assert out["critics"][0][0][0].isnan().all() and aout["log_std"].isnan().all()
    env.check_status()
    env.close()


def test_native_refusals():
    """8: every refusal of the calls returns the error with a message and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    n = 40
    env, rng, critics, obs, act = _case(GOAL, n, 16, 1, seed=16)
    pol = random_policy(rng, env.obs_dim, 16, 1, 2)
    h, h1, hp = _q_handle(env, critics), _q_handle(env, critics[:1]), _handle(env, pol)
    d_obs, d_act = _dev(obs), _dev(act)
    outs = [torch.full((n,), 7.0, device="cuda") for _ in range(2)]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()
    said = lambda match: match in lib.sg_last_error(env._h)

    def ev(q, rows, o, a, o1, o2, match):
        assert lib.sg_q_evaluate_device(env._h, C.byref(q.struct) if q is not None else None, rows, ptr(o), ptr(a), ptr(o1), ptr(o2), s) == -1
        assert said(match), lib.sg_last_error(env._h)

    ev(None, n, d_obs, d_act, *outs, b"null qnet")
    ev(h, 0, d_obs, d_act, *outs, b"n must be")
    ev(h, n, None, d_act, *outs, b"null obs")
    ev(h, n, d_obs, None, *outs, b"null action")
    ev(h, n, d_obs, d_act, None, None, b"no output")
    ev(h1, n, d_obs, d_act, *outs, b"q2_out given, but the qnet has one critic")
    for field, bad, good, match in (("hidden", 129, 16, b"hidden"), ("n_hidden", 4, 1, b"n_hidden"), ("n_critics", 3, 2, b"n_critics"),
                                    ("n_critics", 0, 2, b"n_critics"), ("activation", 2, 1, b"activation"), ("struct_size", 8, 152, b"struct_size")):
        setattr(h.struct, field, bad)
        ev(h, n, d_obs, d_act, *outs, match)
        setattr(h.struct, field, good)
    keep = h.struct.critic[1].bias[0]
    h.struct.critic[1].bias[0] = None
    ev(h, n, d_obs, d_act, *outs, b"layer 0 of critic 1")
    h.struct.critic[1].bias[0] = keep
    # the grad call
    ones = torch.ones(n, device="cuda")
    full = env.q_grad_torch(h, d_obs, d_act, ones, ones, action_grad=True)
    every = [x for pairs in full["critics"] for pair in pairs for x in pair] + [full["action"]]
    for t in every:
        t.fill_(7.0)
    ws = h.workspace
    need = lib.sg_q_grad_workspace_bytes(env._h, C.byref(h.struct), n)
    assert 0 < need <= ws.numel() and need == lib.sg_q_grad_workspace_bytes(env._h, C.byref(h.struct), 256)
    assert lib.sg_q_grad_workspace_bytes(env._h, C.byref(h.struct), 257) == 2 * need  # a second workgroup's partial sums
    assert lib.sg_q_grad_workspace_bytes(env._h, C.byref(h.struct), 10 ** 7) == 256 * need  # the grid cap bounds it
    assert lib.sg_q_grad_workspace_bytes(env._h, C.byref(h.struct), 0) == 0 and said(b"n must be")

    def struct(second=True, **over):
        g = _native.SgQnetGrads(struct_size=C.sizeof(_native.SgQnetGrads))
        for c in range(2 if second else 1):
            for l, (w, b) in enumerate(full["critics"][c]):
                g.critic[c].weight[l], g.critic[c].bias[l] = w.data_ptr(), b.data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def gr(q, rows, o, a, g2, g, ga, w, wbytes, match):
        rc = lib.sg_q_grad_device(env._h, C.byref(q.struct), rows, ptr(o), ptr(a), ptr(ones), ptr(g2), C.byref(g) if g is not None else None,
                                  ptr(ga), ptr(w), wbytes, s)
        assert rc == -1 and said(match), lib.sg_last_error(env._h)

    ga = full["action"]
    gr(h, 0, d_obs, d_act, ones, struct(), ga, ws, ws.numel(), b"n must be")
    gr(h, n, None, d_act, ones, struct(), ga, ws, ws.numel(), b"null obs")
    gr(h, n, d_obs, None, ones, struct(), ga, ws, ws.numel(), b"null action")
    gr(h, n, d_obs, d_act, ones, None, None, ws, ws.numel(), b"no output")
    gr(h, n, d_obs, d_act, ones, struct(struct_size=8), ga, ws, ws.numel(), b"struct_size")
    gr(h, n, d_obs, d_act, ones, struct(reserved=1), ga, ws, ws.numel(), b"reserved")
    bad = struct()
    bad.critic[0].bias[1] = None
    gr(h, n, d_obs, d_act, ones, bad, ga, ws, ws.numel(), b"layer 1 of critic 0")
    gr(h, n, d_obs, d_act, ones, struct(second=False), ga, ws, ws.numel(), b"layer 0 of critic 1")
    gr(h, n, d_obs, d_act, ones, struct(), ga, None, ws.numel(), b"null workspace")
    gr(h, n, d_obs, d_act, ones, struct(), ga, ws, need - 1, b"workspace of")
    gr(h1, n, d_obs, d_act, ones, struct(second=False), ga, ws, ws.numel(), b"g_q2 given, but the qnet has one critic")
    gr(h1, n, d_obs, d_act, None, struct(), ga, ws, ws.numel(), b"gradients of critic 1 given")
    # the actor's calls
    a_out = torch.full((n, 2), 7.0, device="cuda")
    pg = env.policy_action_grad_torch(hp, d_obs, d_act)
    p_every = [x for pair in pg["actor"] for x in pair] + [pg["log_std"]]
    for t in p_every:
        t.fill_(7.0)
    assert lib.sg_policy_action_device(env._h, C.byref(hp.struct), 0, ptr(d_obs), None, ptr(a_out), s) == -1 and said(b"n must be")
    assert lib.sg_policy_action_device(env._h, C.byref(hp.struct), n, None, None, ptr(a_out), s) == -1 and said(b"null obs")
    assert lib.sg_policy_action_device(env._h, C.byref(hp.struct), n, ptr(d_obs), None, None, s) == -1 and said(b"null action_out")

    def pstruct(**over):
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        for l, (w, b) in enumerate(pg["actor"]):
            g.actor.weight[l], g.actor.bias[l] = w.data_ptr(), b.data_ptr()
        g.log_std = pg["log_std"].data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def ag(rows, o, g_a, g, w, wbytes, match):
        rc = lib.sg_policy_action_grad_device(env._h, C.byref(hp.struct), rows, ptr(o), None, ptr(g_a), C.byref(g) if g is not None else None,
                                              ptr(w), wbytes, s)
        assert rc == -1 and said(match), lib.sg_last_error(env._h)

    pws = hp.workspace
    pneed = lib.sg_policy_grad_workspace_bytes(env._h, C.byref(hp.struct), n)
    ag(0, d_obs, d_act, pstruct(), pws, pws.numel(), b"n must be")
    ag(n, None, d_act, pstruct(), pws, pws.numel(), b"null obs")
    ag(n, d_obs, None, pstruct(), pws, pws.numel(), b"null g_action")
    ag(n, d_obs, d_act, None, pws, pws.numel(), b"null grads")
    ag(n, d_obs, d_act, pstruct(struct_size=8), pws, pws.numel(), b"struct_size")
    ag(n, d_obs, d_act, pstruct(log_std=None), pws, pws.numel(), b"log_std")
    ag(n, d_obs, d_act, pstruct(), None, pws.numel(), b"null workspace")
    ag(n, d_obs, d_act, pstruct(), pws, pneed - 1, b"workspace of")
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in outs + every + p_every + [a_out])
    env.check_status()
    # a discrete id: every call is refused
    dis = make(DISCRETE, n)
    d_obs_dis = torch.zeros((n, dis.obs_dim), device="cuda")
    hd = dis.policy_torch(actor=[(torch.zeros((16, dis.obs_dim), device="cuda"), torch.zeros(16, device="cuda")),
                                 (torch.zeros((6, 16), device="cuda"), torch.zeros(6, device="cuda"))])
    with pytest.raises(ValueError, match="discrete ids are not served"):
        dis.q_torch(critics=[[(w, b) for w, b in zip(h.tensors[0:4:2], h.tensors[1:4:2])]])
    said_dis = lambda match: match in lib.sg_last_error(dis._h)
    assert lib.sg_q_evaluate_device(dis._h, C.byref(h.struct), n, ptr(d_obs_dis), ptr(d_act), ptr(outs[0]), None, s) == -1 and said_dis(b"discrete")
    assert lib.sg_q_grad_device(dis._h, C.byref(h.struct), n, ptr(d_obs_dis), ptr(d_act), ptr(ones), None, None, ptr(ga), None, 0, s) == -1
    assert said_dis(b"discrete")
    assert lib.sg_q_grad_workspace_bytes(dis._h, C.byref(h.struct), n) == 0 and said_dis(b"discrete")
    assert lib.sg_policy_action_device(dis._h, C.byref(hd.struct), n, ptr(d_obs_dis), None, ptr(a_out), s) == -1 and said_dis(b"discrete")
    assert lib.sg_policy_action_grad_device(dis._h, C.byref(hd.struct), n, ptr(d_obs_dis), None, ptr(d_act), C.byref(pstruct()), ptr(pws),
                                            pws.numel(), s) == -1 and said_dis(b"discrete")
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in outs + every + p_every + [a_out])
    dis.check_status()
    dis.close()
    # the handles still work
    assert env.q_evaluate_raw_torch(h1, d_obs, d_act)[1] is None
    env.q_grad_torch(h, d_obs, d_act, ones)
    torch.cuda.synchronize()
    env.check_status()
    env.close()
