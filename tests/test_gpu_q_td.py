"""GPU tests of q_td_grad_torch / q_update_torch (sg_q_td_grad_device) against the calls they fuse and against the NumPy model
tests/q_td_model.py.

What the fused call shares with sg_q_evaluate_device and sg_q_grad_device is checked EXACTLY: q_next and the target against the
composition of q_evaluate_raw_torch on the target handle with torch.clamp / torch.minimum / torch.where, q1 and q2 against the evaluate
call on the online handle, the parameter gradients against q_grad_torch fed the g1 / g2 the kernel reports.  Against the float64 model
every per-row array, every statistic and every gradient tensor x is checked under DESIGN section 18's rule,
    |x - x64| <= 8 x max|x32seq - x64| + 1e-6 (1 + max|x64|),
x32seq the model in float32 with the batch summed sequentially, and every gradient tensor's tolerance must also be at most 1 % of
max|G64| (tests/test_q_td.py checks that cap, the distance of every |td| from huber_delta and the branch shares on the CPU, for the
very cases run here).

Row counts: 1, 200, 2049 over the nets (1, 1), (33, 2), (64, 2), (128, 3); 256 x 64 + 300 rows at hidden 128 (workgroups of 64 rows:
past the grid cap of 256 they take a second row tile); one net of width class 3 (hidden 80).  The family's width test runs
tests/net_widths.py's table and (128, 3) at n = 200, held to the single calls' bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from net_widths import N as WIDTH_N, OBS_DIM, ids_of
from q_model import grad_tolerances, random_qnet
from q_td_model import ACTION_CLIP, ALPHA, BIG_N, NOISE_CLIP, NOISE_STD, ROWS, STATS, case as td_case, flat, grad_case, grad_cases, options, reference
from q_td_model import regime_case, regime_reference, register_width_family, td, width_cases
from squashed_model import random_squashed
from test_gpu_policy import _dev, _np, make

pytestmark = pytest.mark.gpu
register_width_family()  # (tests/test_net_widths.py counts the engine's kernel templates against the families: see q_td_model)

GOAL, KEPLER, DISCRETE = "GoalContinuous3P-v0", "KeplerCircleOrbit-v0", "GoalDiscrete3-v0"
WORST = []  # (error / tolerance, error, tolerance, what): printed by the last test of the file


def _handle(env, critics, activation="relu"):
    return env.q_torch(critics=[[(_dev(W), _dev(b)) for W, b in net] for net in critics], activation=activation)


def _env_for(obs_dim, n):
    env = make(GOAL if obs_dim == 15 else KEPLER, min(n, 256))  # (the net calls take any n: the env count only sizes the handle)
    assert env.obs_dim == obs_dim and not env.discrete
    return env


def _tol(x32, x64):
    x64 = np.asarray(x64, np.float64)
    return 8.0 * float(np.abs(np.asarray(x32, np.float64) - x64).max()) + 1e-6 * (1.0 + float(np.abs(x64).max()))


def _close(got, x32, x64, what):
    t, err = _tol(x32, x64), float(np.abs(np.asarray(got, np.float64) - x64).max())
    WORST.append((err / t, err, t, what))
    assert err <= t, (what, err, t)


def _grads_np(out):
    import torch
    torch.cuda.synchronize()
    return flat(dict(critics=[[(w.cpu().numpy(), b.cpu().numpy()) for w, b in net] for net in out["critics"]]))


def _check_grads(got, g32, g64, what):
    tol = grad_tolerances(g32, g64)
    assert set(got) == set(g64), what
    for k in g64:
        top = float(np.abs(g64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - g64[k]).max())
        print("gradient", what, k, "error %.3g tolerance %.3g max|G64| %.3g" % (err, tol[k], top))
        WORST.append((err / tol[k], err, tol[k], what + (k,)))
        assert top > 0 and tol[k] <= 0.01 * top, (what, k, tol[k], top)
        assert err <= tol[k], (what, k, err, tol[k])


def _device_batch(c):
    return {k: _dev(v) for k, v in c["batch"].items()}


def _device_options(c, form, huber_delta, weighted):
    """q_td_model.options with the arrays on the device; the first entry, next_action, is positional in the method"""
    return {k: _dev(v) if isinstance(v, np.ndarray) else v for k, v in options(c, form, huber_delta, weighted).items()}


def _rows(n, critics=2, fill=float("nan")):
    import torch
    return {k: torch.full((n,), fill, device="cuda") for k in ROWS if critics == 2 or k not in ("td2", "q2", "g2")}


def _bits(t):
    return _np(t)[0].tobytes()


@functools.lru_cache(maxsize=None)
def _models(case):
    """the float64 and the float32 model of a case (computed once per case, shared, never written)"""
    obs_dim, n, hidden, n_hidden, n_critics, activation, form, huber_delta, weighted = case
    c = grad_case(obs_dim, n, hidden, n_hidden, n_critics)
    return tuple(reference(c, activation, form, huber_delta, weighted, dt) for dt in (np.float64, np.float32))


def _call(env, ho, ht, b, kw, **more):
    kw = dict(kw, **more)
    rows = kw.pop("rows", None) or _rows(b["obs"].shape[0], ho.n_critics)
    grads, stats = env.q_td_grad_torch(ho, ht, b, kw.pop("next_action"), rows=rows, **kw)
    return grads, stats, rows


def _composed_target(env, ht, b, kw):
    """q_next and y of the composed calls: the clamps, q_evaluate_raw_torch on the target handle, minimum, the entropy term, where"""
    import torch
    a2 = kw["next_action"]
    if kw.get("noise") is not None:
        a2 = torch.clamp(a2 + torch.clamp(kw["noise_std"] * kw["noise"], -kw["noise_clip"], kw["noise_clip"]), -kw["action_clip"], kw["action_clip"])
    q = env.q_evaluate_raw_torch(ht, b["next_obs"], a2.contiguous())
    q_next = q[0] if ht.n_critics == 1 else torch.minimum(*q)
    if kw.get("next_logp") is not None:
        alpha = kw["alpha"]
        q_next = q_next - (alpha if isinstance(alpha, torch.Tensor) else torch.tensor(alpha, dtype=torch.float32, device="cuda")) * kw["next_logp"]
    return q_next, torch.where(b["terminated"] != 0, b["reward"], b["reward"] + b["discount"] * q_next)


def _check_composed(env, ho, ht, b, kw, grads, rows, what):
    """1 and 2 of the module's list, for one call's outputs"""
    q_next, target = _composed_target(env, ht, b, kw)
    assert _bits(rows["q_next"]) == _bits(q_next), what
    assert _bits(rows["target"]) == _bits(target), what
    q = env.q_evaluate_raw_torch(ho, b["obs"], b["action"])
    for c in range(ho.n_critics):
        assert _bits(rows["q%d" % (c + 1)]) == _bits(q[c]), (what, c)
        assert _bits(rows["td%d" % (c + 1)]) == _bits(q[c] - rows["target"]), (what, c)
    got = _grads_np(grads)
    composed = _grads_np(env.q_grad_torch(ho, b["obs"], b["action"], g_q1=rows["g1"], g_q2=rows.get("g2")))
    assert len(got) == 2 * (ho.n_hidden + 1) * ho.n_critics
    for k in got:
        assert np.abs(got[k]).max() > 0 and got[k].tobytes() == composed[k].tobytes(), (what, k)
    return got


@pytest.mark.parametrize("case", grad_cases(), ids=lambda c: "-".join(map(str, c)))
def test_fused_outputs_are_the_composed_calls_bits(case):
    """1, 2, 4, 5: q_next and target against the composed calls; q1 / q2 against q_evaluate_raw_torch on the online handle; the gradients
    against q_grad_torch fed the reported g1 / g2 at the same n; a float alpha and a tensor alpha; one critic: zero critic-2
    statistics and td_abs = |td1|; two calls into NaN-prefilled buffers; weights of ones"""
    import torch
    obs_dim, n, hidden, n_hidden, n_critics, activation, form, huber_delta, weighted = case
    assert n != BIG_N or (hidden == 128 and n > 256 * 64)
    env = _env_for(obs_dim, n)
    c = grad_case(obs_dim, n, hidden, n_hidden, n_critics)
    ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
    b, kw = _device_batch(c), _device_options(c, form, huber_delta, weighted)
    grads, stats, rows = _call(env, ho, ht, b, kw)
    torch.cuda.synchronize()
    assert n == 1 or bool(b["terminated"].any())
    got = _check_composed(env, ho, ht, b, kw, grads, rows, case)
    assert not any(t.isnan().any() for t in rows.values()) and rows["g1"].abs().max() > 0
    s = _np(stats)[0]
    if n_critics == 1:  # 4
        assert s[2] == 0 and s[5] == 0 and _bits(rows["td_abs"]) == _bits(rows["td1"].abs()), case
        assert s[3] == _np(rows["td1"].abs().max())[0], case
    else:
        assert s[2] > 0 and _bits(rows["td_abs"]) == _bits(0.5 * (rows["td1"].abs() + rows["td2"].abs())), case
        assert s[3] == _np(torch.maximum(rows["td1"].abs().max(), rows["td2"].abs().max()))[0], case
    first = {k: _bits(t) for k, t in rows.items()}
    first_stats = _bits(stats)
    if form == "sac":  # a tensor alpha gives the float's bits
        g2, s2, r2 = _call(env, ho, ht, b, kw, alpha=torch.tensor([ALPHA], device="cuda"))
        assert _bits(s2) == first_stats and all(_bits(r2[k]) == first[k] for k in r2), case
        for k, v in _grads_np(g2).items():
            assert v.tobytes() == got[k].tobytes(), (case, k)
    # 5
    ho.workspace.view(torch.float32).fill_(float("nan"))
    for t in [x for net in grads["critics"] for pair in net for x in pair] + [stats] + list(rows.values()):
        t.fill_(float("nan"))
    again_g, again_s, _ = _call(env, ho, ht, b, kw, rows=rows, out=grads, stats=stats)
    again = _grads_np(again_g)
    assert again_g is grads and again_s is stats and _bits(stats) == first_stats and not stats.isnan().any()
    for k in got:
        assert not np.isnan(again[k]).any() and again[k].tobytes() == got[k].tobytes(), (case, k)
    assert all(_bits(rows[k]) == first[k] for k in rows)
    if not weighted:
        ones_g, ones_s, ones_r = _call(env, ho, ht, b, kw, weight=torch.ones(n, device="cuda"))
        assert _bits(ones_s) == first_stats and all(_bits(ones_r[k]) == first[k] for k in ones_r)
        for k, v in _grads_np(ones_g).items():
            assert v.tobytes() == got[k].tobytes(), (case, k)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", width_cases())
def test_both_kernels_at_every_width_class(hidden, n_hidden, activation):
    """9: the family's width test (tests/net_widths.py): every class NT = 1 .. 4 and each class's widest net, three hidden layers on
    the 4P id, at n = 200 -- ragged forward workgroups and row tiles in every class -- with two critics and with one.  Held to the
    single calls' bits: q_next, target, q1 and q2 are the evaluate kernel's, the gradients q_grad_torch's with the reported g, at these
    widths too; those calls are held to their models at the same widths by tests/test_gpu_net_widths.py"""
    env_id = ids_of(hidden, n_hidden)[0]
    env = make(env_id, WIDTH_N)
    assert env.obs_dim == OBS_DIM[env_id] and not env.discrete
    for n_critics, form in ((2, "td3"), (1, "sac")):
        c = td_case(env.obs_dim, WIDTH_N, hidden, n_hidden, n_critics, seed=WIDTH_N + hidden)
        ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
        b, kw = _device_batch(c), _device_options(c, form, 1.0, True)
        grads, stats, rows = _call(env, ho, ht, b, kw)
        _check_composed(env, ho, ht, b, kw, grads, rows, (hidden, n_hidden, activation, n_critics))
        need = env._lib.sg_q_td_grad_workspace_bytes(env._h, C.byref(ho.struct), WIDTH_N)
        groups = -(-WIDTH_N // {1: 256, 2: 128, 3: 64, 4: 64}[-(-hidden // 32)])  # policy_grad_block by class
        params = sum(int(W.size + bias.size) for net in c["online"] for W, bias in net) + 2  # (the layout's two log_std floats: unused)
        assert need == 4 * (groups * (params + 9) + WIDTH_N) <= ho.workspace.numel()
        assert need == env._lib.sg_q_grad_workspace_bytes(env._h, C.byref(ho.struct), WIDTH_N) + 36 * groups + 4 * WIDTH_N
    env.check_status()
    env.close()


def _check_against_model(what, m64, m32, grads, stats, rows):
    names = [k for k in ROWS if k in rows]
    got_rows = dict(zip(names, _np(*[rows[k] for k in names])))
    for k in names:
        _close(got_rows[k], m32["rows"][k], m64["rows"][k], what + (k,))
    s = _np(stats)[0]
    for k, name in enumerate(STATS):
        _close(s[k], m32["stats"][k], m64["stats"][k], what + (name,))
    assert s[3] == max(np.abs(got_rows[k]).max() for k in ("td1", "td2") if k in got_rows), what  # td_abs_max: exactly the largest row
    _check_grads(_grads_np(grads), flat(m32), flat(m64), what)
    return got_rows


@pytest.mark.parametrize("case", grad_cases(), ids=lambda c: "-".join(map(str, c)))
def test_outputs_equal_the_model(case):
    """3: every per-row array, the nine statistics and every gradient against the float64 model"""
    obs_dim, n, hidden, n_hidden, n_critics, activation, form, huber_delta, weighted = case
    env = _env_for(obs_dim, n)
    c = grad_case(obs_dim, n, hidden, n_hidden, n_critics)
    ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
    grads, stats, rows = _call(env, ho, ht, _device_batch(c), _device_options(c, form, huber_delta, weighted))
    m64, m32 = _models(case)
    got = _check_against_model(case, m64, m32, grads, stats, rows)
    if np.isfinite(huber_delta):  # the device clips the rows the model clips
        for k in range(n_critics):
            assert np.array_equal(np.abs(got["td%d" % (k + 1)]) > huber_delta, m64["clipped"][k]), case
    env.check_status()
    env.close()


def test_a_trained_regime_case_equals_the_model():
    """10: tests/net_regimes.py's q family -- hidden gains of 5, Q values in the hundreds, most rows clipped -- under the same rule;
    tests/test_q_td.py checks its 1 % cap on the CPU"""
    c, activation, form, huber_delta, weighted = regime_case()
    n = c["batch"]["obs"].shape[0]
    env = make(c["env_id"], n)
    ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
    b, kw = _device_batch(c), _device_options(c, form, huber_delta, weighted)
    grads, stats, rows = _call(env, ho, ht, b, kw)
    _check_composed(env, ho, ht, b, kw, grads, rows, ("regime",))
    _check_against_model(("regime", activation, form), regime_reference(np.float64), regime_reference(np.float32), grads, stats, rows)
    env.check_status()
    env.close()


K, B, N_DRAW, LR, TAU = 6, 256, 256, 1e-3, 0.005


def _modules(net, device="cuda"):
    import torch
    mods = []
    for l, (W, b) in enumerate(net):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] + ([torch.nn.ReLU()] if l < len(net) - 1 else [])
    return torch.nn.Sequential(*mods).to(device)


def _learner(seed):
    """an env of 256 (the draws are as many, so that the actor's act call takes next_obs) with episodes of 3 steps, a squashed actor,
    online and target twin critics with their handles, an Adam state, and a ring of 2 K = 12 slots with priorities, filled by
    rollout_squashed_torch in two chunks of K = 6 steps"""
    import torch
    env = make(GOAL, B, seed=seed, max_episode_steps=3)
    rng = np.random.default_rng(seed)
    pairs = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, torch.nn.Linear)]
    nets = random_qnet(rng, env.obs_dim, 64, 2), random_qnet(rng, env.obs_dim, 64, 2)
    om, tm = [_modules(net) for net in nets[0]], [_modules(net) for net in nets[1]]
    ho, ht = env.q_torch(critics=[pairs(m) for m in om]), env.q_torch(critics=[pairs(m) for m in tm])
    sp = env.squashed_policy_torch(actor=[(_dev(W), _dev(b)) for W, b in random_squashed(rng, env.obs_dim, 64, 2)], activation="relu")
    opt = env.adam_torch(ho, lr=LR)
    T = 2 * K
    ring = env.replay_torch(T, term_capacity=T * B)
    prio = env.replay_priority_torch(ring)
    env.replay_begin_torch(ring, env.reset_torch())
    env.replay_priority_begin_torch(prio)
    term = env.terminal_list_torch(K * B)
    rows = ring.rows(K)
    first = torch.empty((K + 1, B, env.obs_dim), device="cuda")  # the first action's observation is the ring's last slot
    first[0].copy_(ring.obs[T - 1])
    env.rollout_squashed_torch(sp, first, rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=seed, first_step=0, terminal=term)
    rows["obs"].copy_(first[1:])
    env.replay_commit_torch(ring, K, terminal=term, priority=prio)
    rows = ring.rows(K)
    env.rollout_squashed_torch(sp, ring.obs[K - 1:T], rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=seed, first_step=K, terminal=term)
    env.replay_commit_torch(ring, K, terminal=term, priority=prio)
    return env, nets, sp, ho, ht, opt, ring, prio


def _state(ho, ht, opt, prio):
    return [t.detach().clone() for t in (*ho.tensors, *ht.tensors, opt.state, *opt.exp_avg, *opt.exp_avg_sq, prio.leaf, prio.node, prio.hdr)]


def _restore(ho, ht, opt, prio, saved):
    import torch
    with torch.no_grad():
        for t, s in zip((*ho.tensors, *ht.tensors, opt.state, *opt.exp_avg, *opt.exp_avg_sq, prio.leaf, prio.node, prio.hdr), saved):
            t.copy_(s)


def test_one_learner_step_equals_the_step_composed_through_autograd():
    """6: a ring of 12 slots filled by rollout_squashed_torch, episodes of 3 steps, 256 prioritized draws with n_step = 3;
    q_update_torch (SAC form) with prio and tau = 0.005 against the same step made of q_evaluate_torch autograd, adam_step_torch, the
    torch priority formula and a lerp.  Both gradients are within the model's tolerance of the float64 gradient, so they are within
    twice that of each other; an Adam step from zero moments moves a parameter by lr u(g), u(g) = g / (|g| + eps): the parameters may
    differ by lr max |u(g +- 2 tol) - u(g)| plus two roundings (DESIGN section 31's bound).  Priorities agree on every cell whose
    td_abs agrees"""
    import torch
    env, nets, sp, ho, ht, opt, ring, prio = _learner(33)
    batch = env.replay_sample_prioritized_torch(ring, prio, N_DRAW, seed=3, beta=0.4, n_step=3, gamma=0.97)
    na, logp = env.squashed_act_torch(sp, batch["next_obs"], seed=5, step=0)
    torch.cuda.synchronize()
    assert len(set(_np(batch["steps"])[0].tolist())) > 1 and len(set(_np(batch["discount"])[0].tolist())) > 1  # (episodes of 3 steps cut the 3-step returns)
    before = _state(ho, ht, opt, prio)
    stats, rows, grads = env.q_update_torch(ho, ht, opt, batch, na, next_logp=logp, alpha=ALPHA, huber_delta=1.0, weight=batch["weight"], prio=prio, tau=TAU)
    torch.cuda.synchronize()
    fused = _state(ho, ht, opt, prio)
    fused_grads, abs_fused = [t.clone() for net in grads["critics"] for pair in net for t in pair], rows["td_abs"].clone()
    assert int(opt.state[0, 0]) == 1 and all(not torch.equal(a, b) for a, b in zip(before[:24], fused[:24]))
    _restore(ho, ht, opt, prio, before)
    # the same step, composed
    with torch.no_grad():
        y = _composed_target(env, ht, batch, dict(next_action=na, next_logp=logp, alpha=ALPHA))[1]
    q1, q2 = env.q_evaluate_torch(ho, batch["obs"], batch["action"])
    huber = lambda q: (batch["weight"] * torch.nn.functional.huber_loss(q, y, reduction="none", delta=1.0)).mean()
    (huber(q1) + huber(q2)).backward()
    L = len(ho.tensors) // 2
    auto = dict(critics=[[(ho.tensors[l].grad, ho.tensors[l + 1].grad) for l in range(c * L, (c + 1) * L, 2)] for c in range(2)], action=None)
    auto_grads = [t for net in auto["critics"] for pair in net for t in pair]
    env.adam_step_torch(opt, auto)
    abs_auto = (0.5 * ((q1 - y).abs() + (q2 - y).abs())).detach()
    env.replay_update_priorities_torch(prio, batch["cell"], abs_auto, alpha=0.6, epsilon=1e-6)
    with torch.no_grad():
        torch._foreach_lerp_(list(ht.tensors), list(ho.tensors), TAU)
    torch.cuda.synchronize()
    composed = _state(ho, ht, opt, prio)
    # the tolerance of the gradients, from the model on the sampled batch
    nb = {k: _np(batch[k])[0] for k in ("obs", "action", "reward", "next_obs", "terminated", "discount")}
    kw = dict(next_action=_np(na)[0], next_logp=_np(logp)[0], alpha=ALPHA, huber_delta=1.0, weight=_np(batch["weight"])[0])
    m64, m32 = (td(nets[0], nets[1], nb, dtype=dt, **kw) for dt in (np.float64, np.float32))
    tol = grad_tolerances(flat(m32), flat(m64))
    names = [f"critic{c}.{l}.{kind}" for c in range(2) for l in range(3) for kind in ("weight", "bias")]
    u = lambda g: g / (np.abs(g) + 1e-8)
    for i, name in enumerate(names):
        g_f, g_a, g64 = _np(fused_grads[i])[0].astype(np.float64), _np(auto_grads[i])[0].astype(np.float64), flat(m64)[name]
        for what, g in (("fused", g_f), ("autograd", g_a)):
            err = float(np.abs(g - g64).max())
            WORST.append((err / tol[name], err, tol[name], ("learner step", what, name)))
            assert tol[name] <= 0.01 * np.abs(g64).max() and err <= tol[name], (what, name, err, tol[name])
        p_f, p_c, p_0 = (_np(s[i])[0].astype(np.float64) for s in (fused, composed, before))
        bound = LR * np.maximum(np.abs(u(g_a + 2 * tol[name]) - u(g_a)), np.abs(u(g_a - 2 * tol[name]) - u(g_a))) + 2 * np.spacing(np.abs(p_0).astype(np.float32))
        assert (np.abs(p_f - p_c) <= bound).all(), (name, float((np.abs(p_f - p_c) - bound).max()))
        assert np.abs(p_f - p_0).max() > 0.5 * LR and np.median(bound) < 0.01 * LR  # the step is there, and the bound is a small part of it
        t_f, t_c, t_0 = (_np(s[12 + i])[0].astype(np.float64) for s in (fused, composed, before))
        assert (np.abs(t_f - t_c) <= TAU * bound + 2 * np.spacing(np.abs(t_0).astype(np.float32))).all() and not np.array_equal(t_f, t_0), name
    # the priorities: equal wherever every draw of the cell carries the same td_abs in both paths; elsewhere the cells still moved
    cell, same = _np(batch["cell"])[0], _np(abs_fused == abs_auto)[0]
    leaf_f, leaf_c, leaf_0 = (_np(s[-3])[0].ravel() for s in (fused, composed, before))
    agree = np.array([same[cell == k].all() for k in cell])
    assert agree.mean() > 0.5 and np.array_equal(leaf_f[cell[agree]], leaf_c[cell[agree]])
    assert (leaf_f[cell] != leaf_0[cell]).mean() > 0.9
    other = np.ones(leaf_f.size, bool)
    other[cell] = False
    assert np.array_equal(leaf_f[other], leaf_0[other]) and np.array_equal(leaf_c[other], leaf_0[other])
    env.check_status()
    env.close()


def test_the_whole_critic_step_replays_as_a_graph():
    """7: the prioritized draw, squashed_act_torch on next_obs and q_update_torch with prio, a device-scalar tau and a tensor alpha,
    captured after a warm-up; two replays change the parameters, advance the optimizer and draw other cells; alpha written between
    replays changes the next replay's target; a workspace that would have to grow inside a capture raises with nothing written"""
    import torch
    env, nets, sp, ho, ht, opt, ring, prio = _learner(34)
    tau, alpha = torch.tensor(TAU, device="cuda"), torch.tensor([ALPHA], device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream: sizes the workspace, makes the buffers
        batch = env.replay_sample_prioritized_torch(ring, prio, N_DRAW, seed=3, beta=0.4, n_step=3, gamma=0.97)
        na, logp = env.squashed_act_torch(sp, batch["next_obs"], seed=5, step=0)
        rows = dict(td_abs=torch.empty(N_DRAW, device="cuda"), target=torch.empty(N_DRAW, device="cuda"), q_next=torch.empty(N_DRAW, device="cuda"))
        stats, rows, grads = env.q_update_torch(ho, ht, opt, batch, na, next_logp=logp, alpha=alpha, weight=batch["weight"], rows=rows, prio=prio, tau=tau)
    side.synchronize()

    def step():
        env.replay_sample_prioritized_torch(ring, prio, N_DRAW, seed=3, beta=0.4, n_step=3, gamma=0.97, out=batch)
        env.squashed_act_torch(sp, batch["next_obs"], seed=5, step=0, out=dict(action=na, logp=logp))
        env.q_update_torch(ho, ht, opt, batch, na, next_logp=logp, alpha=alpha, weight=batch["weight"], rows=rows, grads=grads, stats=stats, prio=prio, tau=tau)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()
    assert int(opt.state[0, 0]) == 1  # (capturing ran nothing)
    seen = [[t.detach().clone() for t in ho.tensors]]
    cells = [batch["cell"].clone()]
    for rep in range(2):
        stats.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        seen.append([t.detach().clone() for t in ho.tensors])
        cells.append(batch["cell"].clone())
        assert all(not torch.equal(a, b) for a, b in zip(seen[-2], seen[-1])) and int(opt.state[0, 0]) == 2 + rep
        assert not stats.isnan().any() and not torch.equal(cells[-2], cells[-1])
    live = batch["terminated"] == 0
    assert bool(live.any()) and torch.equal(rows["target"][live], (batch["reward"] + batch["discount"] * rows["q_next"])[live])
    tau.fill_(0.0)  # (the target stays as it is, so that it can be evaluated after the replay)
    for value in (0.0, 0.5):  # alpha is read on the device at every replay: 0 leaves the target critics' minimum itself
        alpha.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        q_min = torch.minimum(*env.q_evaluate_raw_torch(ht, batch["next_obs"], na))
        assert torch.equal(rows["q_next"], q_min - alpha * logp) and (value == 0.0) == torch.equal(rows["q_next"], q_min), value
    tau.fill_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ho.tensors, ht.tensors))
    env.check_status()
    L = len(ho.tensors) // 2
    h2 = env.q_torch(critics=[[(ho.tensors[l], ho.tensors[l + 1]) for l in range(c * L, (c + 1) * L, 2)] for c in range(2)])  # a fresh handle has no workspace
    stats.fill_(7.0)
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.q_td_grad_torch(h2, ht, batch, na, out=grads, stats=stats)
    torch.cuda.synchronize()
    assert h2.workspace is None and (stats == 7).all()
    env.check_status()
    env.close()


def test_native_refusals():
    """8: every refusal returns the error with a message that names the argument and leaves the outputs untouched; the workspace
    query's three terms"""
    import torch
    from space_gym_amd import _native
    n = 40
    env = make(GOAL, n)
    rng = np.random.default_rng(16)
    nets = random_qnet(rng, env.obs_dim, 16, 1)
    ho, ht = _handle(env, nets), _handle(env, nets)
    f = lambda *shape: torch.full(shape, 7.0, device="cuda")
    batch = dict(obs=f(n, env.obs_dim), action=f(n, 2), reward=f(n), next_obs=f(n, env.obs_dim),
                 terminated=torch.zeros(n, dtype=torch.uint8, device="cuda"), discount=f(n))
    na, logp, alpha = f(n, 2), f(n), f(1)
    grads, stats = env.q_td_grad_torch(ho, ht, batch, na)
    every = [x for net in grads["critics"] for pair in net for x in pair] + [stats]
    for t in every:
        t.fill_(7.0)
    ws = ho.workspace
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()
    ref = lambda h: C.byref(h.struct) if h is not None else None
    need = lib.sg_q_td_grad_workspace_bytes(env._h, ref(ho), n)
    per_group = 4 * (sum(int(W.size + b.size) for net in nets for W, b in net) + 2)  # (the layout's two log_std floats: unused)
    assert per_group == lib.sg_q_grad_workspace_bytes(env._h, ref(ho), n)
    assert need == per_group + 36 + 4 * n <= ws.numel()  # one workgroup's partial sums, its nine statistics sums, y [n]
    assert lib.sg_q_td_grad_workspace_bytes(env._h, ref(ho), 257) == 2 * per_group + 2 * 36 + 4 * 257
    assert lib.sg_q_td_grad_workspace_bytes(env._h, ref(ho), 10 ** 7) == 256 * per_group + 256 * 36 + 4 * 10 ** 7
    said = lambda e, match: match in lib.sg_last_error(e._h)
    for bad in (0, 2 ** 31):
        assert lib.sg_q_td_grad_workspace_bytes(env._h, ref(ho), bad) == 0 and said(env, b"n must be")

    def cfg(**over):
        c = _native.SgQTdConfig()
        lib.sg_q_td_config_init(C.byref(c))
        assert (c.struct_size, c.huber_delta, c.alpha, c.noise_std, c.noise_clip, c.action_clip, tuple(c.reserved)) == (
            32, float("inf"), np.float32(0.2), np.float32(0.2), 0.5, 1.0, (0, 0))
        for k, v in over.items():
            setattr(c, k, v)
        return c

    def bat(**over):
        cols = {k: batch[k].data_ptr() for k in batch}
        cols.update(next_action=na.data_ptr())
        cols.update(over)
        return _native.SgQTdBatch(**cols)

    def gr(**over):
        g = _native.SgQnetGrads(struct_size=C.sizeof(_native.SgQnetGrads))
        for c, net in enumerate(grads["critics"]):
            for l, (w, b) in enumerate(net):
                g.critic[c].weight[l], g.critic[c].bias[l] = w.data_ptr(), b.data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def call(match, e=env, online=ho, target=ht, c=True, b=True, rows=n, g=True, st=stats, r=None, w=ws, wbytes=None, at=0):
        c = cfg() if c is True else c
        b = bat() if b is True else b
        g = gr() if g is True else g
        rc = lib.sg_q_td_grad_device(e._h, ref(online), ref(target), C.byref(c) if c is not None else None, C.byref(b) if b is not None else None,
                                     rows, C.byref(g) if g is not None else None, ptr(st), C.byref(r) if r is not None else None,
                                     C.c_void_p(w.data_ptr() + at) if w is not None else None, ws.numel() - at if wbytes is None else wbytes, s)
        assert rc == -1 and said(e, match), lib.sg_last_error(e._h)

    call(b"null qnet", online=None)
    call(b"null target", target=None)
    wide, deep = _handle(env, random_qnet(rng, env.obs_dim, 17, 1)), _handle(env, random_qnet(rng, env.obs_dim, 16, 2))
    single = _handle(env, nets[:1])
    call(b"differ in shape", target=wide)
    call(b"differ in shape", target=deep)
    call(b"differ in shape", target=_handle(env, nets, "tanh"))
    call(b"differ in shape", target=single)
    for field, bad, good, match in (("hidden", 129, 16, b"hidden"), ("n_hidden", 0, 1, b"n_hidden"), ("activation", 2, 1, b"activation"),
                                    ("n_critics", 3, 2, b"n_critics"), ("struct_size", 8, C.sizeof(_native.SgQnet), b"struct_size")):
        for h in (ho, ht):
            setattr(h.struct, field, bad)
            call(match)
            setattr(h.struct, field, good)
    call(b"null cfg", c=None)
    call(b"struct_size", c=cfg(struct_size=8))
    for word in ((1, 0), (0, 1)):
        call(b"reserved", c=cfg(reserved=(C.c_int32 * 2)(*word)))
    for bad in (0.0, -1.0, float("nan")):
        call(b"huber_delta must be > 0", c=cfg(huber_delta=bad))
    for field in ("noise_std", "noise_clip", "action_clip"):
        for bad in (-0.5, float("nan")):
            call(b"must be >= 0", c=cfg(**{field: bad}))
    call(b"n must be", rows=0)
    call(b"n must be", rows=2 ** 31)
    call(b"null batch", b=None)
    call(b"null obs", b=bat(obs=None))
    for k in ("action", "reward", "next_obs", "terminated", "discount", "next_action"):
        call(b"null batch." + k.encode(), b=bat(**{k: None}))
    call(b"alpha_dev given without batch.next_logp", b=bat(alpha_dev=alpha.data_ptr()))
    call(b"null stats_out", st=None)
    call(b"null grads", g=None)
    call(b"struct_size", g=gr(struct_size=8))
    call(b"reserved", g=gr(reserved=1))
    hole = gr()
    hole.critic[1].bias[1] = None
    call(b"layer 1 of critic 1", g=hole)
    call(b"null workspace", w=None)
    call(b"workspace of", wbytes=need - 1)
    call(b"aligned to 4", w=torch.empty(need + 8, dtype=torch.uint8, device="cuda"), wbytes=need, at=2)
    # one critic: no row output and no gradient slot of critic 2
    one_grads = gr()
    for k in ("td2", "q2", "g2"):
        call(b"row output of critic 2", online=single, target=single, r=_native.SgQTdRows(**{k: logp.data_ptr()}))
    call(b"gradients of critic 1 given", online=single, target=single, g=one_grads)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in every) and (logp == 7).all()
    env.check_status()
    # a discrete id: refused by the library and by the method
    dis = make(DISCRETE, n)
    call(b"discrete", e=dis)
    assert lib.sg_q_td_grad_workspace_bytes(dis._h, ref(ho), n) == 0 and said(dis, b"discrete")
    with pytest.raises(ValueError, match="discrete ids are not served"):
        dis.q_td_grad_torch(ho, ht, batch, na)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in every)
    dis.check_status()
    dis.close()
    # the handles still work, and the accepted edges: an infinite action clip, an alpha on the device
    env.q_td_grad_torch(ho, ht, batch, na, next_logp=logp, alpha=alpha, noise=f(n, 2), action_clip=float("inf"), out=grads, stats=stats)
    torch.cuda.synchronize()
    assert not stats.isnan().any() and float(stats[8]) == 1.0
    env.check_status()
    env.close()


def test_report_the_worst_error_to_tolerance_ratios():
    """prints the three largest error / tolerance ratios the tests above met (they asserted each one at its place)"""
    WORST.sort(key=lambda r: -r[0])
    for ratio, err, tol, what in WORST[:3]:
        print("error / tolerance %.3f (error %.3g, tolerance %.3g) at" % (ratio, err, tol), what)
    assert all(r[0] <= 1.0 for r in WORST)
