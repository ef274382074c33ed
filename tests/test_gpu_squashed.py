"""GPU tests of squashed_policy_torch / squashed_act_torch / squashed_sample_raw_torch / squashed_grad_torch / squashed_sample_torch /
rollout_squashed_torch (sg_squashed_act_device / sg_squashed_sample_device / sg_squashed_grad_device / sg_rollout_squashed_device)
against the NumPy model tests/squashed_model.py.

Forward tolerances are DESIGN section 17's rule: 8 x max|float32 CPU - float64| + 1e-6 (_tol), computed here.  A gradient tensor's
tolerance is section 18's: 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|), G32seq the model in float32 with the batch summed sequentially;
every such tolerance must also be at most 1 % of max|G64| of its tensor, so that a wrong index cannot hide (tests/test_squashed.py
checks that cap on the CPU for the very cases run here).  The cases come from squashed_model.case: tight clamp bounds, and no row whose
raw log_std lies within 1e-3 of a bound.

Row counts: 1 (a partial wave), 200 (no multiple of a workgroup), 2049 (9 .. 33 workgroups whose partials are reduced), and for the
smallest workgroup (64 rows, hidden = 128) 256 x 64 + 300 rows, where the capped grid makes workgroups take a second row tile."""
import ctypes as C

import numpy as np
import pytest

from q_model import q_evaluate, random_qnet
from squashed_model import BIG_N, BOUNDS, GRAD_NS, SELECTIONS, act, case, flat, grad_cases, grad_reference, grad_tolerances, random_squashed, sample
from test_gpu_policy import DISCRETE, GOAL, KEPLER, NETS, _dev, _np, _tol, make

pytestmark = pytest.mark.gpu


def _handle(env, actor, activation="relu", bounds=BOUNDS):
    return env.squashed_policy_torch(actor=[(_dev(W), _dev(b)) for W, b in actor], log_std_bounds=bounds, activation=activation)


def _env_for(obs_dim, n):
    env = make(GOAL if obs_dim == 15 else KEPLER, n)
    assert env.obs_dim == obs_dim
    return env


def _grads_np(out):
    import torch
    torch.cuda.synchronize()
    return flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]]))


def _check_grads(got, g32, g64, what, worst):
    tol = grad_tolerances(g32, g64)
    assert set(got) == set(g64), what
    for k in g64:
        top = float(np.abs(g64[k]).max())
        if top == 0.0:
            assert not got[k].any(), (what, k)
            continue
        err = float(np.abs(got[k].astype(np.float64) - g64[k]).max())
        print("gradient", what, k, "error %.3g tolerance %.3g max|G64| %.3g" % (err, tol[k], top))
        worst.append((err / tol[k], err, tol[k], top, what, k))
        assert tol[k] <= 0.01 * top, (what, k, tol[k], top)
        assert err <= tol[k], (what, k, err, tol[k])


def _report(worst):
    worst.sort(reverse=True)
    for ratio, err, tol, top, what, k in worst[:3]:
        print("gradient error / tolerance %.3f (error %.3g, tolerance %.3g, max|G64| %.3g) at" % (ratio, err, tol, top), what, k)


@pytest.mark.parametrize("B", [1, 200])
@pytest.mark.parametrize("env_id", [GOAL, KEPLER])
def test_act_equals_the_model(env_id, B):
    """1: action and logp against the float64 model, every net, both activations; a shard (env_index_base) gives the same bits; the
    deterministic act equals squashed_sample_raw_torch(eps=None) bit for bit"""
    env = make(env_id, B, env_index_base=1000)
    part = make(env_id, 64, env_index_base=1064) if B == 200 else None
    rng = np.random.default_rng(B + len(env_id))
    obs = rng.standard_normal((B, env.obs_dim)).astype(np.float32)
    worst = {}
    for hidden, n_hidden in NETS:
        for activation in ("tanh", "relu"):
            actor = random_squashed(rng, env.obs_dim, hidden, n_hidden)
            h = _handle(env, actor, activation)
            kw = dict(seed=77, step=2 ** 32 + 5)
            what = (env_id, B, hidden, n_hidden, activation)
            a, lp = _np(*env.squashed_act_torch(h, _dev(obs), **kw))
            a_det, lp_det = _np(*env.squashed_act_torch(h, _dev(obs), deterministic=True, **kw))
            for det, (ga, gl) in ((False, (a, lp)), (True, (a_det, lp_det))):
                m64 = act(actor, obs, env_index_base=1000, deterministic=det, bounds=BOUNDS, activation=activation, **kw)
                m32 = act(actor, obs, env_index_base=1000, deterministic=det, bounds=BOUNDS, activation=activation, dtype=np.float32, **kw)
                for k, got in (("action", ga), ("logp", gl)):
                    t = _tol(m32[k], m64[k])
                    err = float(np.abs(got - m64[k]).max())
                    worst[k] = max(worst.get(k, 0.0), t)
                    assert err <= t, (what, det, k, err, t)
            assert np.abs(a).max() <= 1.0 and (B == 1 or (a != a_det).mean() > 0.9)
            s_a, s_lp = _np(*env.squashed_sample_raw_torch(h, _dev(obs)))
            assert s_a.tobytes() == a_det.tobytes() and s_lp.tobytes() == lp_det.tobytes(), what
            a2, lp2 = _np(*env.squashed_act_torch(h, _dev(obs), **kw))
            assert a2.tobytes() == a.tobytes() and lp2.tobytes() == lp.tobytes()
            b, _ = _np(*env.squashed_act_torch(h, _dev(obs), seed=77, step=5))  # another high word of the step: other noise
            assert B == 1 or (b != a).mean() > 0.5
            only_a = env.squashed_act_torch(h, _dev(obs), out=dict(action=_dev(np.zeros((B, 2), np.float32))), **kw)
            assert only_a[1] is None and _np(only_a[0])[0].tobytes() == a.tobytes()
            if part is not None:
                hp = _handle(part, actor, activation)
                pa, plp = _np(*part.squashed_act_torch(hp, _dev(obs[64:128]), **kw))
                assert pa.tobytes() == a[64:128].tobytes() and plp.tobytes() == lp[64:128].tobytes(), what
    print("tolerances (8 x |float32 CPU - float64| + 1e-6), largest over the nets:", env_id, B, {k: "%.3g" % t for k, t in worst.items()})
    env.check_status()
    env.close()
    if part is not None:
        part.close()


def test_a_discrete_id_is_refused():
    env = make(DISCRETE, 8)
    with pytest.raises(ValueError, match="discrete ids are not served"):
        env.squashed_policy_torch(actor=[(_dev(np.zeros((4, env.obs_dim), np.float32)), _dev(np.zeros(4, np.float32))),
                                         (_dev(np.zeros((4, 4), np.float32)), _dev(np.zeros(4, np.float32)))])
    env.close()


@pytest.mark.parametrize("n", GRAD_NS)
def test_sample_equals_the_model_and_rows_alone_give_the_same_bits(n):
    """2: (action, logp) with the caller's eps within _tol of the float64 model, every net with both activations; rows [lo:hi] alone:
    the same bits"""
    worst = {}
    for i, (hidden, n_hidden) in enumerate(NETS):
        obs_dim = 15 if i % 2 == 0 else 10
        env = _env_for(obs_dim, n)
        c = case(obs_dim, n, hidden, n_hidden, seed=n + hidden)
        for activation in ("tanh", "relu"):
            h = _handle(env, c["actor"], activation)
            a, lp = _np(*env.squashed_sample_raw_torch(h, _dev(c["obs"]), _dev(c["eps"])))
            m64 = sample(c["actor"], c["obs"], c["eps"], bounds=BOUNDS, activation=activation)
            m32 = sample(c["actor"], c["obs"], c["eps"], bounds=BOUNDS, activation=activation, dtype=np.float32)
            for k, got in (("action", a), ("logp", lp)):
                t = _tol(m32[k], m64[k])
                worst[k] = max(worst.get(k, 0.0), t)
                assert np.abs(got - m64[k]).max() <= t, (n, hidden, n_hidden, activation, k, np.abs(got - m64[k]).max(), t)
            lo, hi = n // 3, n // 3 + max(1, n // 2)
            s_a, s_lp = _np(*env.squashed_sample_raw_torch(h, _dev(c["obs"][lo:hi]), _dev(c["eps"][lo:hi])))
            assert s_a.tobytes() == a[lo:hi].tobytes() and s_lp.tobytes() == lp[lo:hi].tobytes()
        env.check_status()
        env.close()
    print("largest forward tolerances (8 x |float32 CPU - float64| + 1e-6):", n, {k: "%.3g" % t for k, t in worst.items()})


@pytest.mark.parametrize("obs_dim,n,hidden,n_hidden,activation", grad_cases())
def test_gradients_equal_the_model(obs_dim, n, hidden, n_hidden, activation):
    """3: g_action only, g_logp only and both, within section 18's tolerance with the 1 % cap; two calls into NaN-prefilled buffers
    give the same bits; a NULL g_logp with zero eps gives exact zeros in the raw rows of the head.  n = 256 x 64 + 300 at hidden = 128:
    workgroups take a second row tile."""
    import torch
    assert n != BIG_N or (hidden == 128 and n > 256 * 64)
    env = _env_for(obs_dim, n)
    c = case(obs_dim, n, hidden, n_hidden, seed=n + hidden)
    h = _handle(env, c["actor"], activation)
    d_obs, d_eps, d_ga, d_gl = _dev(c["obs"]), _dev(c["eps"]), _dev(c["g_action"]), _dev(c["g_logp"])
    worst = []
    what = (obs_dim, n, hidden, n_hidden, activation)
    for sel in SELECTIONS:
        ga = d_ga if sel in ("both", "action") else None
        gl = d_gl if sel in ("both", "logp") else None
        out = env.squashed_grad_torch(h, d_obs, d_eps, ga, gl)
        got = _grads_np(out)
        _check_grads(got, grad_reference(c, activation, sel, np.float32), grad_reference(c, activation, sel, np.float64), what + (sel,), worst)
        h.workspace.view(torch.float32).fill_(float("nan"))
        for w, b in out["actor"]:
            w.fill_(float("nan"))
            b.fill_(float("nan"))
        again = _grads_np(env.squashed_grad_torch(h, d_obs, d_eps, ga, gl, out=out))
        for k in got:
            assert not np.isnan(again[k]).any() and again[k].tobytes() == got[k].tobytes(), (what, sel, k)
    plain = _grads_np(env.squashed_grad_torch(h, d_obs, None, d_ga, None))  # no noise, no g_logp: nothing reaches the raw log_std outputs
    L = n_hidden
    assert not plain["actor.%d.weight" % L][2:].any() and not plain["actor.%d.bias" % L][2:].any() and plain["actor.%d.bias" % L][:2].any()
    _report(worst)
    env.check_status()
    env.close()


K, B = 4, 200


def _buffers(env, K):
    import torch
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    return dict(obs=z(K + 1, B, env.obs_dim), action=z(K, B, 2), logp=z(K, B), reward=z(K, B), done=z(K, B, dtype=torch.uint8),
                trunc=z(K, B, dtype=torch.uint8))


def _hand_loop(env, h, K, seed, first_step, obs0=None):
    """squashed_act_torch then step_torch(terminal_obs=...) K times; the terminal records as a set of (step, env, obs bytes)"""
    import torch
    b = _buffers(env, K)
    b["obs"][0].copy_(env.reset_torch() if obs0 is None else obs0)
    tobs = torch.zeros((B, env.obs_dim), dtype=torch.float32, device="cuda")
    records = set()
    for t in range(K):
        env.squashed_act_torch(h, b["obs"][t], seed=seed, step=first_step + t, out=dict(action=b["action"][t], logp=b["logp"][t]))
        env.step_torch(b["action"][t], out=dict(obs=b["obs"][t + 1], reward=b["reward"][t], done=b["done"][t], trunc=b["trunc"][t]),
                       terminal_obs=tobs)
        d, to = _np(b["done"][t], tobs)
        for i in np.nonzero(d)[0]:
            records.add((t, int(i), to[i].tobytes()))
    return b, records


@pytest.mark.parametrize("normalize_obs", [False, True])
def test_rollout_equals_the_hand_written_loop(normalize_obs):
    """4: every output of rollout_squashed_torch, bit for bit, with a terminal list; max_episode_steps = 3 puts truncations and
    auto-resets inside the call (the list is unordered: compared as a set); with observation normalization on as well"""
    kw = dict(seed=21, max_episode_steps=3, normalize_obs=normalize_obs)
    ea, eb = make(GOAL, B, **kw), make(GOAL, B, **kw)
    rng = np.random.default_rng(10)
    actor = random_squashed(rng, ea.obs_dim, 64, 2)
    ha, hb = _handle(ea, actor), _handle(eb, actor)
    want, records = _hand_loop(ea, ha, K, seed=4, first_step=100)
    got, term = _buffers(eb, K), eb.terminal_list_torch(1000)
    got["obs"][0].copy_(eb.reset_torch())
    eb.rollout_squashed_torch(hb, seed=4, first_step=100, terminal=term, **got)
    eb.check_status()
    for name in want:
        w, g = _np(want[name], got[name])
        assert w.tobytes() == g.tobytes(), (name, int((w != g).sum()))
    trunc, done, count, se, ob = _np(got["trunc"], got["done"], term["count"], term["step_env"], term["obs"])
    assert trunc[2].mean() > 0.9 and done.sum() >= 0.9 * B  # (nearly) every env runs into the time limit at t = 2
    n = int(count[0])
    listed = {(int(se[k, 0]), int(se[k, 1]), ob[k].tobytes()) for k in range(n)}
    assert n == int(done.sum()) == len(records) and listed == records
    # without logp and without a list: the same actions and observations
    ec = make(GOAL, B, **kw)
    hc = _handle(ec, actor)
    bare = _buffers(ec, K)
    bare["obs"][0].copy_(ec.reset_torch())
    bare.pop("logp")
    ec.rollout_squashed_torch(hc, seed=4, first_step=100, **bare)
    for name in bare:
        w, g = _np(want[name], bare[name])
        assert w.tobytes() == g.tobytes(), name
    for e in (ea, eb, ec):
        e.close()


def test_rollout_into_a_replay_ring():
    """4: the call's buffers are a replay ring's rows: obs = the ring's slots head - 1 .. head + K - 1, the others ring.rows(K),
    followed by replay_commit_torch; the ring then holds the hand-written loop's transitions"""
    import torch
    kw = dict(seed=22, max_episode_steps=3)
    ea, eb = make(GOAL, B, **kw), make(GOAL, B, **kw)
    rng = np.random.default_rng(11)
    actor = random_squashed(rng, ea.obs_dim, 33, 2)
    ha, hb = _handle(ea, actor), _handle(eb, actor)
    want, _ = _hand_loop(ea, ha, 2 * K, seed=6, first_step=0)
    ring = eb.replay_torch(2 * K)
    eb.replay_begin_torch(ring, eb.reset_torch())
    term = eb.terminal_list_torch(K * B)
    # the first chunk: the observation the first action is taken from is the ring's last slot, not adjacent to slot 0
    rows = ring.rows(K)
    first = torch.empty((K + 1, B, eb.obs_dim), device="cuda")
    first[0].copy_(ring.obs[2 * K - 1])
    eb.rollout_squashed_torch(hb, first, rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=6, first_step=0, terminal=term)
    rows["obs"].copy_(first[1:])
    eb.replay_commit_torch(ring, K, terminal=term)
    # the second chunk: every buffer is the ring's own memory
    rows = ring.rows(K)
    assert ring.head == K
    eb.rollout_squashed_torch(hb, ring.obs[K - 1:2 * K], rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=6, first_step=K,
                              terminal=term)
    eb.replay_commit_torch(ring, K, terminal=term)
    eb.check_status()
    assert ring.filled == 2 * K and len(ring) == (2 * K - 1) * B
    for name, full in (("obs", want["obs"][1:]), ("action", want["action"]), ("reward", want["reward"]), ("done", want["done"]),
                       ("trunc", want["trunc"])):
        w, g = _np(full, getattr(ring, name))
        assert w.tobytes() == g.tobytes(), name
    assert _np(want["done"])[0].any()
    ea.close()
    eb.close()


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


def _torch_squashed(net, x, e, bounds):
    import torch
    head = net(x)
    mean, raw = head[:, :2], head[:, 2:]
    ls = torch.clamp(raw, float(np.float32(bounds[0])), float(np.float32(bounds[1])))
    u = mean + ls.exp() * e
    a = torch.tanh(u)
    logp = (-0.5 * e * e - ls - 0.5 * np.log(2 * np.pi) - 2.0 * (np.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(-1)
    return a, logp


def test_sac_actor_step_and_critic_target_through_autograd():
    """5: the SAC actor loss (alpha logp - min(Q1, Q2)).mean() through squashed_sample_torch + q_evaluate_torch and backward(), the
    actor's .grad against float64 CPU torch modules fed the same numbers, under the per-tensor rule with g = d loss / d outputs; and
    the critic target r + gamma (min Q'(s', a') - alpha logp') on next_obs under no_grad, under the forward rule"""
    import torch
    n, alpha, gamma = 200, 0.2, 0.99
    env = make(GOAL, n)
    c = case(env.obs_dim, n, 64, 2, seed=14)
    rng = np.random.default_rng(14)
    critics = random_qnet(rng, env.obs_dim, 64, 2)
    next_obs = rng.standard_normal((n, env.obs_dim)).astype(np.float32)
    eps2, reward = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    pairs = lambda net: [(m.weight, m.bias) for m in lin(net)]
    named = lambda net: {f"actor.{l}.{kind}": getattr(m, kind).grad.detach().cpu().numpy() for l, m in enumerate(lin(net)) for kind in ("weight", "bias")}
    # float64 on the CPU
    c64 = _modules(critics, "relu", torch.float64, "cpu")
    a64 = _modules([c["actor"]], "relu", torch.float64, "cpu")[0]
    x, e = torch.from_numpy(c["obs"]).double(), torch.from_numpy(c["eps"]).double()
    a, lp = _torch_squashed(a64, x, e, BOUNDS)
    a.retain_grad()
    lp.retain_grad()
    q = [net(torch.cat([x, a], 1))[:, 0] for net in c64]
    assert (q[0] - q[1]).abs().min() > 1e-4  # no row whose min() a float32 rounding could turn
    (alpha * lp - torch.min(q[0], q[1])).mean().backward()
    actor64 = named(a64)
    g_a, g_lp = a.grad.numpy().astype(np.float32), lp.grad.numpy().astype(np.float32)
    actor32 = flat(sample(c["actor"], c["obs"], c["eps"], g_a, g_lp, bounds=BOUNDS, activation="relu", dtype=np.float32))
    with torch.no_grad():
        x2, e2 = torch.from_numpy(next_obs).double(), torch.from_numpy(eps2).double()
        a2, lp2 = _torch_squashed(a64, x2, e2, BOUNDS)
        q2 = [net(torch.cat([x2, a2], 1))[:, 0] for net in c64]
        target64 = (torch.from_numpy(reward).double() + gamma * (torch.min(q2[0], q2[1]) - alpha * lp2)).numpy()
    s32 = sample(c["actor"], next_obs, eps2, bounds=BOUNDS, activation="relu", dtype=np.float32)
    q32 = q_evaluate(critics, next_obs, s32["action"], activation="relu", grads=False, dtype=np.float32)["q"]
    target32 = reward + np.float32(gamma) * (np.minimum(q32[0], q32[1]) - np.float32(alpha) * s32["logp"])
    # the device
    cd = _modules(critics, "relu", torch.float32, "cuda")
    ad = _modules([c["actor"]], "relu", torch.float32, "cuda")[0]
    hq = env.q_torch(critics=[pairs(net) for net in cd], activation="relu")
    sp = env.squashed_policy_torch(actor=pairs(ad), log_std_bounds=BOUNDS, activation="relu")
    d_obs, d_eps = _dev(c["obs"]), _dev(c["eps"])
    a_d, lp_d = env.squashed_sample_torch(sp, d_obs, d_eps)
    assert a_d.grad_fn is not None and lp_d.grad_fn is not None
    (alpha * lp_d - torch.min(*env.q_evaluate_torch(hq, d_obs, a_d))).mean().backward()
    worst = []
    _check_grads(named(ad), actor32, actor64, "actor loss", worst)
    # an output the loss does not use: the backward passes a NULL g for it
    ad.zero_grad()
    a_d, lp_d = env.squashed_sample_torch(sp, d_obs, d_eps)
    (alpha * lp_d).mean().backward()
    only_lp = flat(sample(c["actor"], c["obs"], c["eps"], None, np.full(n, alpha / n), bounds=BOUNDS, activation="relu"))
    only_lp32 = flat(sample(c["actor"], c["obs"], c["eps"], None, np.full(n, alpha / n, np.float32), bounds=BOUNDS, activation="relu", dtype=np.float32))
    _check_grads(named(ad), only_lp32, only_lp, "logp alone", worst)
    with torch.no_grad():
        a2_d, lp2_d = env.squashed_sample_torch(sp, _dev(next_obs), _dev(eps2))
        t_d = _dev(reward) + gamma * (torch.min(*env.q_evaluate_torch(hq, _dev(next_obs), a2_d)) - alpha * lp2_d)
    assert a2_d.grad_fn is None and not t_d.requires_grad
    t = _tol(target32, target64)
    err = float(np.abs(_np(t_d)[0] - target64).max())
    print("critic target: error %.3g tolerance %.3g" % (err, t))
    assert err <= t
    _report(worst)
    env.check_status()
    env.close()


def test_captured_calls_replay_the_eager_results():
    """6: squashed_act_torch, and squashed_sample_raw_torch + squashed_grad_torch, captured after a warm-up and replayed on new contents
    of the same buffers; a workspace that would have to grow inside a capture raises and launches nothing"""
    import torch
    n = 2049
    env = make(GOAL, n)
    c = case(env.obs_dim, n, 64, 2, seed=15)
    rng = np.random.default_rng(15)
    h = _handle(env, c["actor"])
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    d_obs, d_eps, d_ga, d_gl = _dev(c["obs"]), _dev(c["eps"]), _dev(c["g_action"]), _dev(c["g_logp"])
    side = torch.cuda.Stream()
    z = lambda *shape: torch.empty(shape, device="cuda")
    act_out, smp_out = dict(action=z(n, 2), logp=z(n)), dict(action=z(n, 2), logp=z(n))
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream
        env.squashed_act_torch(h, d_obs, seed=3, step=9, out=act_out)
        g_out = env.squashed_grad_torch(h, d_obs, d_eps, d_ga, d_gl)
    side.synchronize()

    def update():
        env.squashed_act_torch(h, d_obs, seed=3, step=9, out=act_out)
        env.squashed_sample_raw_torch(h, d_obs, d_eps, out=smp_out)
        env.squashed_grad_torch(h, d_obs, d_eps, d_ga, d_gl, out=g_out)

    every = lambda: list(act_out.values()) + list(smp_out.values()) + [x for pair in g_out["actor"] for x in pair]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        update()
    for _ in range(2):
        for t, shape in ((d_obs, (n, env.obs_dim)), (d_eps, (n, 2)), (d_ga, (n, 2)), (d_gl, (n,))):  # new contents, the same buffers
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
    h2 = _handle(env, c["actor"])  # a fresh handle has no workspace: inside a capture the call must raise before anything is enqueued
    g_out["actor"][0][0].fill_(float("nan"))
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.squashed_grad_torch(h2, d_obs, d_eps, d_ga, d_gl, out=g_out)
    torch.cuda.synchronize()
    assert h2.workspace is None and g_out["actor"][0][0].isnan().all()
    env.check_status()
    env.close()


def test_native_refusals():
    """7: every refusal of the calls returns the error with a message and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    n = 40
    env = make(GOAL, n)
    rng = np.random.default_rng(16)
    actor = random_squashed(rng, env.obs_dim, 16, 1)
    h = _handle(env, actor)
    d_obs = _dev(rng.standard_normal((n, env.obs_dim)).astype(np.float32))
    d_eps = _dev(rng.standard_normal((n, 2)).astype(np.float32))
    a_out, lp_out = torch.full((n, 2), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
    ones, ones2 = torch.ones(n, device="cuda"), torch.ones((n, 2), device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()
    said = lambda match: match in lib.sg_last_error(env._h)
    ref = lambda hh: C.byref(hh.struct) if hh is not None else None

    def ac(hh, o, a, match):
        assert lib.sg_squashed_act_device(env._h, ref(hh), ptr(o), 0, 0, 0, ptr(a), ptr(lp_out), s) == -1 and said(match), lib.sg_last_error(env._h)

    def sm(hh, rows, o, a, match):
        assert lib.sg_squashed_sample_device(env._h, ref(hh), rows, ptr(o), ptr(d_eps), ptr(a), ptr(lp_out), s) == -1 and said(match), \
            lib.sg_last_error(env._h)

    ac(None, d_obs, a_out, b"null policy")
    ac(h, None, a_out, b"null obs")
    ac(h, d_obs, None, b"null action_out")
    sm(None, n, d_obs, a_out, b"null policy")
    sm(h, 0, d_obs, a_out, b"n must be")
    sm(h, n, None, a_out, b"null obs")
    sm(h, n, d_obs, None, b"null action_out")
    nan, inf = float("nan"), float("inf")
    for field, bad, good, match in (("hidden", 129, 16, b"hidden"), ("hidden", 0, 16, b"hidden"), ("n_hidden", 4, 1, b"n_hidden"),
                                    ("n_hidden", 0, 1, b"n_hidden"), ("activation", 2, 1, b"activation"),
                                    ("struct_size", 8, C.sizeof(_native.SgSquashedPolicy), b"struct_size"),
                                    ("reserved", 1, 0, b"reserved"), ("log_std_min", 1.0, BOUNDS[0], b"log_std bounds"),
                                    ("log_std_min", nan, BOUNDS[0], b"log_std bounds"), ("log_std_max", inf, BOUNDS[1], b"log_std bounds"),
                                    ("log_std_min", -inf, BOUNDS[0], b"log_std bounds")):
        setattr(h.struct, field, bad)
        ac(h, d_obs, a_out, match)
        sm(h, n, d_obs, a_out, match)
        assert lib.sg_squashed_grad_workspace_bytes(env._h, ref(h), n) == 0 and said(match)
        setattr(h.struct, field, good)
    keep = h.struct.actor.bias[1]
    h.struct.actor.bias[1] = None
    ac(h, d_obs, a_out, b"layer 1 of the actor")
    h.struct.actor.bias[1] = keep
    # the grad call
    full = env.squashed_grad_torch(h, d_obs, d_eps, ones2, ones)
    every = [x for pair in full["actor"] for x in pair]
    for t in every:
        t.fill_(7.0)
    ws = h.workspace
    need = lib.sg_squashed_grad_workspace_bytes(env._h, ref(h), n)
    assert 0 < need <= ws.numel() and need == lib.sg_squashed_grad_workspace_bytes(env._h, ref(h), 256)
    assert lib.sg_squashed_grad_workspace_bytes(env._h, ref(h), 257) == 2 * need  # a second workgroup's partial sums
    assert lib.sg_squashed_grad_workspace_bytes(env._h, ref(h), 10 ** 7) == 256 * need  # the grid cap bounds it
    assert lib.sg_squashed_grad_workspace_bytes(env._h, ref(h), 0) == 0 and said(b"n must be")

    def struct(**over):
        g = _native.SgSquashedGrads(struct_size=C.sizeof(_native.SgSquashedGrads))
        for l, (w, b) in enumerate(full["actor"]):
            g.actor.weight[l], g.actor.bias[l] = w.data_ptr(), b.data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def gr(rows, o, ga, gl, g, w, wbytes, match):
        rc = lib.sg_squashed_grad_device(env._h, ref(h), rows, ptr(o), ptr(d_eps), ptr(ga), ptr(gl), C.byref(g) if g is not None else None, ptr(w),
                                         wbytes, s)
        assert rc == -1 and said(match), lib.sg_last_error(env._h)

    gr(0, d_obs, ones2, ones, struct(), ws, ws.numel(), b"n must be")
    gr(n, None, ones2, ones, struct(), ws, ws.numel(), b"null obs")
    gr(n, d_obs, None, None, struct(), ws, ws.numel(), b"both NULL")
    gr(n, d_obs, ones2, ones, None, ws, ws.numel(), b"null grads")
    gr(n, d_obs, ones2, ones, struct(struct_size=8), ws, ws.numel(), b"struct_size")
    gr(n, d_obs, ones2, ones, struct(reserved=1), ws, ws.numel(), b"reserved")
    bad = struct()
    bad.actor.bias[1] = None
    gr(n, d_obs, ones2, ones, bad, ws, ws.numel(), b"layer 1 of the actor")
    gr(n, d_obs, ones2, ones, struct(), None, ws.numel(), b"null workspace")
    gr(n, d_obs, ones2, ones, struct(), ws, need - 1, b"workspace of")
    # the rollout
    b = {k: torch.full_like(v[:, :n].contiguous(), 7) for k, v in _buffers(env, 2).items()}

    def ro(steps, bufs, tl, match):
        rc = lib.sg_rollout_squashed_device(env._h, steps, ref(h), 0, 0, 0, ptr(bufs["obs"]), ptr(bufs["action"]), ptr(bufs["logp"]),
                                            ptr(bufs["reward"]), ptr(bufs["done"]), ptr(bufs["trunc"]), C.byref(tl) if tl is not None else None, s)
        assert rc == -1 and said(match), lib.sg_last_error(env._h)

    ro(0, b, None, b"n_steps")
    for k in ("obs", "action", "reward", "done", "trunc"):
        ro(2, {**b, k: None}, None, b"null buffer")
    ro(2, b, _native.SgTerminalList(None, None, None, 4), b"incomplete terminal list")
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in [a_out, lp_out] + every + list(b.values()))
    env.check_status()
    # a discrete id: every call is refused
    dis = make(DISCRETE, n)
    d_obs_dis = torch.zeros((n, dis.obs_dim), device="cuda")
    said_dis = lambda match: match in lib.sg_last_error(dis._h)
    assert lib.sg_squashed_act_device(dis._h, ref(h), ptr(d_obs_dis), 0, 0, 0, ptr(a_out), None, s) == -1 and said_dis(b"discrete")
    assert lib.sg_squashed_sample_device(dis._h, ref(h), n, ptr(d_obs_dis), None, ptr(a_out), None, s) == -1 and said_dis(b"discrete")
    assert lib.sg_squashed_grad_device(dis._h, ref(h), n, ptr(d_obs_dis), None, ptr(ones2), None, C.byref(struct()), ptr(ws), ws.numel(), s) == -1
    assert said_dis(b"discrete")
    assert lib.sg_squashed_grad_workspace_bytes(dis._h, ref(h), n) == 0 and said_dis(b"discrete")
    assert lib.sg_rollout_squashed_device(dis._h, 2, ref(h), 0, 0, 0, ptr(b["obs"]), ptr(b["action"]), None, ptr(b["reward"]), ptr(b["done"]),
                                          ptr(b["trunc"]), None, s) == -1 and said_dis(b"discrete")
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in [a_out, lp_out] + every + list(b.values()))
    dis.check_status()
    dis.close()
    # the handle still works
    env.squashed_sample_raw_torch(h, d_obs, d_eps)
    env.squashed_grad_torch(h, d_obs, d_eps, ones2)
    torch.cuda.synchronize()
    env.check_status()
    env.close()
