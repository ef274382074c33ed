"""GPU tests of policy_evaluate_torch / policy_evaluate_raw_torch / policy_grad_torch (sg_policy_evaluate_device /
sg_policy_grad_device) against the NumPy model tests/policy_grad_model.py.

Forward tolerances are DESIGN section 17's rule: 8 x max|float32 CPU - float64| + 1e-6, computed here.  A gradient tensor's tolerance
is 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|), G32seq the model in float32 with the batch summed sequentially; every such tolerance
must also be at most 1 % of max|G64| of its tensor, so that a wrong index (which moves entries by their own magnitude) cannot hide.  A
gradient that is identically zero in the model (a NULL g_*) must be exactly zero on the device.

Row counts: 1 (a partial wave), 200 (no multiple of a workgroup), 2049 (9 .. 33 workgroups whose partials are reduced), and per
workgroup size one n just above 256 workgroups' worth of rows, where the capped grid makes workgroups take a second row tile."""
import ctypes as C

import numpy as np
import pytest

from policy_grad_model import evaluate, flat, grad_tolerances
from policy_model import random_policy
from test_gpu_policy import DISCRETE, GOAL, KEPLER, NETS, _dev, _handle, _np, _tol, make

pytestmark = pytest.mark.gpu

NS = [1, 200, 2049]


def _case(env_id, n, hidden, n_hidden, seed, critic=True):
    env = make(env_id, n)
    rng = np.random.default_rng(seed)
    continuous = not env.discrete
    pol = random_policy(rng, env.obs_dim, hidden, n_hidden, 2 if continuous else 6, critic=critic, continuous=continuous)
    obs = rng.standard_normal((n, env.obs_dim)).astype(np.float32)
    return env, rng, pol, obs


def _grads_np(out):
    import torch
    torch.cuda.synchronize()
    cpu = lambda pairs: None if pairs is None else [(w.cpu().numpy(), b.cpu().numpy()) for w, b in pairs]
    return flat(dict(actor=cpu(out["actor"]), critic=cpu(out.get("critic")),
                     log_std=out["log_std"].cpu().numpy() if out.get("log_std") is not None else None))


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


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_forward_is_the_act_kernels_arithmetic(env_id, n):
    """1: on act's own (obs, action): value and the discrete logp bit for bit; the continuous logp and both entropies against the model"""
    env = make(env_id, n)
    rng = np.random.default_rng(n)
    continuous = not env.discrete
    obs = rng.standard_normal((n, env.obs_dim)).astype(np.float32)
    for hidden, n_hidden in NETS:
        for activation in ("tanh", "relu"):
            pol = random_policy(rng, env.obs_dim, hidden, n_hidden, 2 if continuous else 6, continuous=continuous)
            h = _handle(env, pol, activation)
            d_obs = _dev(obs)
            action, logp_act, value_act = env.policy_act_torch(h, d_obs, seed=5, step=3)
            logp, entropy, value = env.policy_evaluate_raw_torch(h, d_obs, action)
            a_np, logp_act, value_act, logp, entropy, value = _np(action, logp_act, value_act, logp, entropy, value)
            what = (env_id, n, hidden, n_hidden, activation)
            assert np.array_equal(value, value_act), what
            m64 = evaluate(pol, obs, a_np, activation=activation, grads=False)
            m32 = evaluate(pol, obs, a_np, activation=activation, grads=False, dtype=np.float32)
            if continuous:
                t = _tol(m32["logp"], m64["logp"])
                assert np.abs(logp - m64["logp"]).max() <= t, (what, np.abs(logp - m64["logp"]).max(), t)
            else:
                assert np.array_equal(logp, logp_act), what  # the PPO ratio of the first minibatch is exactly 1
            t = _tol(m32["entropy"], m64["entropy"])
            assert np.abs(entropy - m64["entropy"]).max() <= t, (what, np.abs(entropy - m64["entropy"]).max(), t)
    env.close()


def _run_grad_case(env_id, n, hidden, n_hidden, activation, worst, which=("all", "logp", "entropy", "value")):
    env, rng, pol, obs = _case(env_id, n, hidden, n_hidden, seed=n + hidden)
    continuous = not env.discrete
    action = (rng.standard_normal((n, 2)).astype(np.float32) if continuous else rng.integers(0, 6, n).astype(np.int32))
    g = {k: rng.standard_normal(n).astype(np.float32) for k in ("logp", "entropy", "value")}
    h = _handle(env, pol, activation)
    d_obs, d_action = _dev(obs), _dev(action)
    for sel in which:
        use = {k: (g[k] if sel in ("all", k) else None) for k in g}
        kw = dict(g_logp=use["logp"], g_entropy=use["entropy"], g_value=use["value"])
        out = env.policy_grad_torch(h, d_obs, d_action, **{k: (_dev(v) if v is not None else None) for k, v in kw.items()})
        got = _grads_np(out)
        g64 = flat(evaluate(pol, obs, action, activation=activation, **kw))
        g32 = flat(evaluate(pol, obs, action, activation=activation, dtype=np.float32, **kw))
        if use["value"] is None:  # the critic's slots are not in use
            assert out["critic"] is None
            g64 = {k: v for k, v in g64.items() if not k.startswith("critic")}
        _check_grads(got, g32, g64, (env_id, n, hidden, n_hidden, activation, sel), worst)
    env.check_status()
    env.close()


def _report(worst):
    worst.sort(reverse=True)
    for ratio, err, tol, top, what, k in worst[:3]:
        print("gradient error / tolerance %.3f (error %.3g, tolerance %.3g, max|G64| %.3g) at" % (ratio, err, tol, top), what, k)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_gradients_equal_the_model(env_id, n):
    """2: dense random g_logp, g_entropy, g_value together and each alone, every net, both activations spread over the nets"""
    worst = []
    for i, (hidden, n_hidden) in enumerate(NETS):
        _run_grad_case(env_id, n, hidden, n_hidden, ("tanh", "relu")[i % 2], worst, which=("all",))
        _run_grad_case(env_id, n, hidden, n_hidden, ("relu", "tanh")[i % 2], worst, which=("logp", "entropy", "value"))
    _report(worst)


def test_gradients_equal_the_model_on_kepler():
    worst = []
    _run_grad_case(KEPLER, 200, 33, 2, "tanh", worst)
    _report(worst)


@pytest.mark.parametrize("hidden,rows", [(5, 256), (40, 128), (97, 64)])
def test_gradients_when_workgroups_take_a_second_row_tile(hidden, rows):
    """2, past the grid cap: 256 workgroups of `rows` rows and 300 rows more, so the first workgroups load their partial sums back"""
    worst = []
    _run_grad_case(GOAL, 256 * rows + 300, hidden, 1, "tanh", worst, which=("all",))
    _report(worst)


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_gradients_are_deterministic_and_written_not_accumulated(env_id):
    """3: two calls give the same bits; buffers (and the workspace) pre-filled with NaN hold no NaN afterwards"""
    import torch
    n = 2049
    for hidden, n_hidden in ((33, 2), (128, 3)):
        env, rng, pol, obs = _case(env_id, n, hidden, n_hidden, seed=6)
        action = rng.standard_normal((n, 2)).astype(np.float32) if not env.discrete else rng.integers(0, 6, n).astype(np.int32)
        h = _handle(env, pol)
        g = [_dev(rng.standard_normal(n).astype(np.float32)) for _ in range(3)]
        first = env.policy_grad_torch(h, _dev(obs), _dev(action), *g)
        a = _grads_np(first)
        h.workspace.view(torch.float32).fill_(float("nan"))
        for pairs in (first["actor"], first["critic"]):
            for w, b in pairs:
                w.fill_(float("nan"))
                b.fill_(float("nan"))
        if first["log_std"] is not None:
            first["log_std"].fill_(float("nan"))
        again = env.policy_grad_torch(h, _dev(obs), _dev(action), *g, out=first)
        b = _grads_np(again)
        for k in a:
            assert not np.isnan(b[k]).any() and a[k].tobytes() == b[k].tobytes(), (env_id, hidden, k)
        env.close()


def _modules(pol, activation, dtype, device):
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
    actor, critic = net(pol["actor"]), net(pol["critic"]) if pol["critic"] is not None else None
    log_std = torch.nn.Parameter(torch.from_numpy(pol["log_std"]).to(dtype=dtype, device=device)) if pol["log_std"] is not None else None
    return actor, critic, log_std


def _ppo_loss(logp, entropy, value, old_logp, adv, ret):
    import torch
    ratio = torch.exp(logp - old_logp)
    loss = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() - 0.01 * entropy.mean()
    return loss + 0.5 * ((value - ret) ** 2).mean() if value is not None else loss


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_autograd_end_to_end(env_id):
    """4: a clipped-PPO loss through policy_evaluate_torch and backward() against float64 CPU modules with the same parameters (test
    2's rule with g = d loss / d outputs); two minibatches accumulate in .grad; no_grad; a policy without a critic"""
    import torch
    n = 200
    env, rng, pol, obs = _case(env_id, n, 64, 2, seed=14)
    continuous = not env.discrete
    action = rng.standard_normal((n, 2)).astype(np.float32) if continuous else rng.integers(0, 6, n).astype(np.int32)
    old_logp = (evaluate(pol, obs, action, grads=False)["logp"] + 0.3 * rng.standard_normal(n)).astype(np.float32)  # some ratios are clipped
    adv, ret = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    # float64 on the CPU: outputs as leaves of the loss give g, the modules give G64
    actor, critic, log_std = _modules(pol, "tanh", torch.float64, "cpu")
    x = torch.from_numpy(obs).double()
    head = actor(x)
    if continuous:
        dist = torch.distributions.Normal(head, log_std.exp().expand_as(head))
        logp, ent = dist.log_prob(torch.from_numpy(action).double()).sum(1), dist.entropy().sum(1)
    else:
        dist = torch.distributions.Categorical(logits=head)
        logp, ent = dist.log_prob(torch.from_numpy(action).long()), dist.entropy()
    value = critic(x)[:, 0]
    for t in (logp, ent, value):
        t.retain_grad()
    _ppo_loss(logp, ent, value, torch.from_numpy(old_logp).double(), torch.from_numpy(adv).double(), torch.from_numpy(ret).double()).backward()
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    g64 = flat(dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(actor)],
                    critic=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(critic)],
                    log_std=log_std.grad.numpy() if continuous else None))
    g = [t.grad.numpy() for t in (logp, ent, value)]
    g32 = flat(evaluate(pol, obs, action, *[v.astype(np.float32) for v in g], dtype=np.float32))
    # the device
    d_actor, d_critic, d_log_std = _modules(pol, "tanh", torch.float32, "cuda")
    pairs = lambda net: [(m.weight, m.bias) for m in lin(net)]
    h = env.policy_torch(actor=pairs(d_actor), critic=pairs(d_critic), log_std=d_log_std)
    d_obs, d_action, d_old, d_adv, d_ret = _dev(obs), _dev(action), _dev(old_logp), _dev(adv), _dev(ret)
    out = env.policy_evaluate_torch(h, d_obs, d_action)
    assert all(t.grad_fn is not None and not t.isnan().any() for t in out)
    _ppo_loss(*out, d_old, d_adv, d_ret).backward()
    grads = lambda: flat(dict(actor=[(w.grad.cpu().numpy(), b.grad.cpu().numpy()) for w, b in pairs(d_actor)],
                              critic=[(w.grad.cpu().numpy(), b.grad.cpu().numpy()) for w, b in pairs(d_critic)],
                              log_std=d_log_std.grad.cpu().numpy() if continuous else None))
    worst = []
    once = grads()
    _check_grads(once, g32, g64, (env_id, "ppo"), worst)
    _report(worst)
    # a second minibatch (the first half of the rows) accumulates
    half = n // 2
    out = env.policy_evaluate_torch(h, d_obs[:half].contiguous(), d_action[:half].contiguous())
    _ppo_loss(*out, d_old[:half], d_adv[:half], d_ret[:half]).backward()
    alone = _grads_np(env.policy_grad_torch(h, d_obs[:half].contiguous(), d_action[:half].contiguous(),
                                            *_loss_grads(env, h, d_obs, d_action, d_old, d_adv, d_ret, half)))
    twice = grads()
    for k in once:
        assert np.array_equal(twice[k], once[k] + alone[k]), k
    with torch.no_grad():
        out = env.policy_evaluate_torch(h, d_obs, d_action)
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    # without a critic: value is None and the actor's gradients are what they were
    for p in list(d_actor.parameters()) + ([d_log_std] if continuous else []):
        p.grad = None
    h_nc = env.policy_torch(actor=pairs(d_actor), log_std=d_log_std)
    logp_nc, ent_nc, v_nc = env.policy_evaluate_torch(h_nc, d_obs, d_action)
    assert v_nc is None
    _ppo_loss(logp_nc, ent_nc, None, d_old, d_adv, d_ret).backward()
    now = grads()
    for k in once:
        if not k.startswith("critic"):
            assert np.array_equal(now[k], once[k]), k
    env.close()


def _loss_grads(env, h, d_obs, d_action, d_old, d_adv, d_ret, half):
    """d loss / d (logp, entropy, value) of the PPO loss on the first `half` rows, from torch on the raw outputs"""
    import torch
    raw = env.policy_evaluate_raw_torch(h, d_obs[:half].contiguous(), d_action[:half].contiguous())
    leaves = [t.clone().requires_grad_() for t in raw]
    _ppo_loss(*leaves, d_old[:half], d_adv[:half], d_ret[:half]).backward()
    return [t.grad.contiguous() for t in leaves]


def test_a_captured_evaluate_and_grad_replay_the_eager_results():
    """5: raw evaluate + raw grad captured after a warm-up call that sizes the workspace; without one the call raises inside the
    capture and launches nothing"""
    import torch
    n = 2049
    env, rng, pol, obs = _case(GOAL, n, 64, 2, seed=15)
    action = rng.standard_normal((n, 2)).astype(np.float32)
    h = _handle(env, pol)
    d_obs, d_action = _dev(obs), _dev(action)
    g = [_dev(rng.standard_normal(n).astype(np.float32)) for _ in range(3)]
    want_fwd = _np(*env.policy_evaluate_raw_torch(h, d_obs, d_action))
    want = _grads_np(env.policy_grad_torch(h, d_obs, d_action, *g))
    side = torch.cuda.Stream()
    fwd = {k: torch.empty(n, device="cuda") for k in ("logp", "entropy", "value")}
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream
        env.policy_evaluate_raw_torch(h, d_obs, d_action, out=fwd)
        out = env.policy_grad_torch(h, d_obs, d_action, *g)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        env.policy_evaluate_raw_torch(h, d_obs, d_action, out=fwd)
        env.policy_grad_torch(h, d_obs, d_action, *g, out=out)
    for _ in range(2):
        for t in list(fwd.values()) + [x for pairs in (out["actor"], out["critic"]) for pair in pairs for x in pair] + [out["log_std"]]:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        got = _grads_np(out)
        for k in want:
            assert want[k].tobytes() == got[k].tobytes(), k
        for w, t in zip(want_fwd, _np(fwd["logp"], fwd["entropy"], fwd["value"])):
            assert w.tobytes() == t.tobytes()
    # a fresh handle has no workspace: inside a capture the call must raise before anything is enqueued
    h2 = _handle(env, pol)
    for t in out["actor"][0]:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.policy_grad_torch(h2, d_obs, d_action, *g, out=out)
    torch.cuda.synchronize()
    assert h2.workspace is None and all(t.isnan().all() for t in out["actor"][0])
    env.check_status()
    env.close()


def test_native_refusals():
    """6: every refusal of the two calls returns the error with a message and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    n = 40
    env, rng, pol, obs = _case(GOAL, n, 16, 1, seed=16)
    h = _handle(env, pol)
    h_nc = _handle(env, dict(pol, critic=None))
    d_obs, d_action = _dev(obs), torch.zeros((n, 2), device="cuda")
    outs = [torch.full((n,), 7.0, device="cuda") for _ in range(3)]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()

    def ev(policy, rows, o, a, lp, en, v, match):
        assert lib.sg_policy_evaluate_device(env._h, C.byref(policy.struct), rows, ptr(o), ptr(a), ptr(lp), ptr(en), ptr(v), s) == -1
        assert match in lib.sg_last_error(env._h), lib.sg_last_error(env._h)

    ev(h, 0, d_obs, d_action, *outs, b"n must be")
    ev(h, n, None, d_action, *outs, b"null obs")
    ev(h, n, d_obs, None, *outs, b"null action")
    ev(h, n, d_obs, d_action, None, None, None, b"no output")
    ev(h_nc, n, d_obs, d_action, *outs, b"no critic")
    h.struct.hidden = 129
    ev(h, n, d_obs, d_action, *outs, b"hidden")
    h.struct.hidden = 16
    # the grad call
    full = env.policy_grad_torch(h, d_obs, d_action, *[torch.ones(n, device="cuda") for _ in range(3)])
    every = [x for pairs in (full["actor"], full["critic"]) for pair in pairs for x in pair] + [full["log_std"]]
    for t in every:
        t.fill_(7.0)
    ws = h.workspace
    need = lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), n)
    assert 0 < need <= ws.numel() and need == lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), 256)
    assert lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), 257) == 2 * need  # a second workgroup's partial sums
    assert lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), 10 ** 7) == 256 * need  # the grid cap bounds it
    ones = torch.ones(n, device="cuda")

    def struct(critic=True, **over):
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        for l, (w, b) in enumerate(full["actor"]):
            g.actor.weight[l], g.actor.bias[l] = w.data_ptr(), b.data_ptr()
        if critic:
            for l, (w, b) in enumerate(full["critic"]):
                g.critic.weight[l], g.critic.bias[l] = w.data_ptr(), b.data_ptr()
        g.log_std = full["log_std"].data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def gr(policy, rows, o, a, gv, g, w, wbytes, match):
        rc = lib.sg_policy_grad_device(env._h, C.byref(policy.struct), rows, ptr(o), ptr(a), ptr(ones), None, ptr(gv), C.byref(g) if g is not None else None,
                                       ptr(w), wbytes, s)
        assert rc == -1 and match in lib.sg_last_error(env._h), lib.sg_last_error(env._h)

    gr(h, 0, d_obs, d_action, ones, struct(), ws, ws.numel(), b"n must be")
    gr(h, n, None, d_action, ones, struct(), ws, ws.numel(), b"null obs")
    gr(h, n, d_obs, None, ones, struct(), ws, ws.numel(), b"null action")
    gr(h, n, d_obs, d_action, ones, None, ws, ws.numel(), b"null grads")
    gr(h, n, d_obs, d_action, ones, struct(struct_size=8), ws, ws.numel(), b"struct_size")
    gr(h, n, d_obs, d_action, ones, struct(log_std=None), ws, ws.numel(), b"log_std")
    bad = struct()
    bad.actor.bias[1] = None
    gr(h, n, d_obs, d_action, ones, bad, ws, ws.numel(), b"layer 1 of the actor")
    gr(h, n, d_obs, d_action, ones, struct(critic=False), ws, ws.numel(), b"of the critic")
    gr(h, n, d_obs, d_action, ones, struct(), None, ws.numel(), b"null workspace")
    gr(h, n, d_obs, d_action, ones, struct(), ws, need - 1, b"workspace of")
    gr(h_nc, n, d_obs, d_action, ones, struct(critic=False), ws, ws.numel(), b"g_value given, but the policy has no critic")
    gr(h_nc, n, d_obs, d_action, None, struct(), ws, ws.numel(), b"critic gradients given")
    h.struct.activation = 2
    gr(h, n, d_obs, d_action, ones, struct(), ws, ws.numel(), b"activation")
    h.struct.activation = 0
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in outs + every)
    assert env.policy_evaluate_raw_torch(h_nc, d_obs, d_action)[2] is None  # the handles still work
    env.policy_grad_torch(h, d_obs, d_action, ones)
    torch.cuda.synchronize()
    env.check_status()
    env.close()
