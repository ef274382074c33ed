"""GPU tests of dqn_td_grad_torch / dqn_update_torch (sg_dqn_td_grad_device) against the calls they fuse and against the NumPy model
tests/dqn_td_model.py.

What the fused call shares with sg_dqn_evaluate_device and sg_dqn_grad_device is checked EXACTLY: q_next and the target against the
two-call composition, q_taken against the evaluate call, the parameter gradients against dqn_grad_torch fed the g the kernel reports.
Against the float64 model every per-row array, every statistic and every gradient tensor x is checked under DESIGN section 18's rule,
    |x - x64| <= 8 x max|x32seq - x64| + 1e-6 (1 + max|x64|),
x32seq the model in float32 with the batch summed sequentially, and every gradient tensor's tolerance must also be at most 1 % of
max|G64| (tests/test_dqn_td.py checks that cap, the distance of every |td| from huber_delta and the share of near-ties on the CPU, for
the very cases run here).  The model takes the DEVICE's a*: a near-tie of two online Q values may round either way in float32; the
target is compared with the model's own a* on the rows whose two largest online Q values are at least 1e-5 apart.

Row counts: dqn_model.GRAD_NS = 1, 200, 2049 over dqn_model.NETS; 256 x 64 + 300 rows at hidden 128 (workgroups of 64 rows: past the
grid cap of 256 they take a second row tile); one net of width class 3 (hidden 80).  The family's width test runs tests/net_widths.py's
table and (128, 3) at n = 200, held to the single calls' bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from dqn_model import BIG_N, flat, grad_tolerances, random_dqn
from dqn_td_model import GAP, ROWS, STATS, case as td_case, grad_case, grad_cases, reference, register_width_family, td, width_cases
from net_widths import N as WIDTH_N, OBS_DIM, ids_of
from test_gpu_policy import _dev, _np, make

pytestmark = pytest.mark.gpu
register_width_family()  # (tests/test_net_widths.py counts the engine's kernel templates against the families: see dqn_td_model)

GOAL, KEPLER, CONTINUOUS = "GoalDiscrete3-v0", "KeplerDiscrete-v0", "GoalContinuous3P-v0"
WORST = []  # (error / tolerance, error, tolerance, what): printed by the last test of the file


def _handle(env, net, activation="relu"):
    return env.dqn_torch(net=[(_dev(W), _dev(b)) for W, b in net], activation=activation)


def _env_for(obs_dim, n):
    env = make(GOAL if obs_dim == 15 else KEPLER, min(n, 256))  # (the net calls take any n: the env count only sizes the handle)
    assert env.obs_dim == obs_dim and env.discrete
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
    return flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["net"]]))


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


def _rows(n, fill=float("nan")):
    import torch
    return {k: torch.full((n,), fill, device="cuda") for k in ROWS}


def _bits(t):
    return _np(t)[0].tobytes()


@functools.lru_cache(maxsize=None)
def _models(case, a_star_bytes):
    """the float64 and the float32 model of a case under the device's a* (computed once per case, shared, never written)"""
    obs_dim, n, hidden, n_hidden, activation, double_q, huber_delta, weighted = case
    c = grad_case(obs_dim, n, hidden, n_hidden)
    a_star = np.frombuffer(a_star_bytes, np.int32) if double_q else None
    return tuple(reference(c, activation, double_q, huber_delta, weighted, dt, a_star=a_star) for dt in (np.float64, np.float32))


def _call(env, ho, ht, b, case, weight, **kw):
    _, n, _, _, _, double_q, huber_delta, _ = case
    rows = _rows(n)
    grads, stats = env.dqn_td_grad_torch(ho, ht, b, double_q=double_q, huber_delta=huber_delta, weight=weight, rows=rows, **kw)
    return grads, stats, rows


@pytest.mark.parametrize("case", grad_cases(), ids=lambda c: "-".join(map(str, c)))
def test_fused_outputs_are_the_composed_calls_bits(case):
    """1, 2, 5: q_next and target against the two-call composition and torch.where; q_taken against dqn_evaluate_raw_torch; the
    gradients against dqn_grad_torch fed the reported g at the same n; two calls into NaN-prefilled buffers; weights of ones"""
    import torch
    obs_dim, n, hidden, n_hidden, activation, double_q, huber_delta, weighted = case
    assert n != BIG_N or (hidden == 128 and n > 256 * 64)
    env = _env_for(obs_dim, n)
    c = grad_case(obs_dim, n, hidden, n_hidden)
    ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
    b, w = _device_batch(c), _dev(c["weight"]) if weighted else None
    grads, stats, rows = _call(env, ho, ht, b, case, w)
    torch.cuda.synchronize()
    # 1
    if double_q:
        a_star = env.dqn_evaluate_raw_torch(ho, b["next_obs"])[3]
        q_next = env.dqn_evaluate_raw_torch(ht, b["next_obs"], a_star)[1]
    else:
        q_next = env.dqn_evaluate_raw_torch(ht, b["next_obs"])[2]
    assert _bits(rows["q_next"]) == _bits(q_next), case
    target = torch.where(b["terminated"] != 0, b["reward"], b["reward"] + b["discount"] * rows["q_next"])
    assert _bits(rows["target"]) == _bits(target) and (n == 1 or bool(b["terminated"].any())), case
    # 2
    assert _bits(rows["q_taken"]) == _bits(env.dqn_evaluate_raw_torch(ho, b["obs"], b["action"])[1]), case
    assert not any(t.isnan().any() for t in rows.values()) and rows["g"].abs().max() > 0
    got = _grads_np(grads)
    composed = _grads_np(env.dqn_grad_torch(ho, b["obs"], b["action"], g_taken=rows["g"]))
    for k in got:
        assert got[k].tobytes() == composed[k].tobytes(), (case, k)
    # 5
    first = {k: _bits(t) for k, t in rows.items()}
    ho.workspace.view(torch.float32).fill_(float("nan"))
    for t in [x for pair in grads["net"] for x in pair] + [stats] + list(rows.values()):
        t.fill_(float("nan"))
    s1 = _bits(stats.clone())
    again_g, again_s = env.dqn_td_grad_torch(ho, ht, b, double_q=double_q, huber_delta=huber_delta, weight=w, rows=rows, out=grads, stats=stats)
    again = _grads_np(again_g)
    assert again_g is grads and again_s is stats and s1 != _bits(stats) and not stats.isnan().any()
    fresh, fresh_stats, _ = _call(env, ho, ht, b, case, w)
    assert _bits(fresh_stats) == _bits(stats)
    for k in got:
        assert not np.isnan(again[k]).any() and again[k].tobytes() == got[k].tobytes(), (case, k)
    assert all(_bits(rows[k]) == first[k] for k in ROWS)
    if not weighted:
        ones_g, ones_s, ones_r = _call(env, ho, ht, b, case, torch.ones(n, device="cuda"))
        assert _bits(ones_s) == _bits(stats) and all(_bits(ones_r[k]) == first[k] for k in ROWS)
        for k, v in _grads_np(ones_g).items():
            assert v.tobytes() == got[k].tobytes(), (case, k)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", width_cases())
def test_both_kernels_at_every_width_class(hidden, n_hidden, activation):
    """the family's width test (tests/net_widths.py): every class NT = 1 .. 4 and each class's widest net, three hidden layers on the
    4P id, at n = 200 -- ragged forward workgroups and row tiles in every class.  Held to the single calls' bits, as the population
    families are: q_next, target and q_taken are the evaluate kernel's, the gradients dqn_grad_torch's with the reported g, at these
    widths too; those calls are held to their models at the same widths by tests/test_gpu_net_widths.py"""
    import torch
    env_id = ids_of(hidden, n_hidden)[1]
    env = make(env_id, WIDTH_N)
    assert env.obs_dim == OBS_DIM[env_id] and env.discrete
    c = td_case(env.obs_dim, WIDTH_N, hidden, n_hidden, seed=WIDTH_N + hidden)
    ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
    b, w = _device_batch(c), _dev(c["weight"])
    for double_q in (True, False):
        rows = _rows(WIDTH_N)
        grads, stats = env.dqn_td_grad_torch(ho, ht, b, double_q=double_q, weight=w, rows=rows)
        if double_q:
            q_next = env.dqn_evaluate_raw_torch(ht, b["next_obs"], env.dqn_evaluate_raw_torch(ho, b["next_obs"])[3])[1]
        else:
            q_next = env.dqn_evaluate_raw_torch(ht, b["next_obs"])[2]
        what = (hidden, n_hidden, activation, double_q)
        assert _bits(rows["q_next"]) == _bits(q_next), what
        assert _bits(rows["target"]) == _bits(torch.where(b["terminated"] != 0, b["reward"], b["reward"] + b["discount"] * q_next)), what
        assert _bits(rows["q_taken"]) == _bits(env.dqn_evaluate_raw_torch(ho, b["obs"], b["action"])[1]), what
        assert _bits(rows["td_error"]) == _bits(rows["q_taken"] - rows["target"]) and float(stats[7]) == 0, what
        got, composed = _grads_np(grads), _grads_np(env.dqn_grad_torch(ho, b["obs"], b["action"], g_taken=rows["g"]))
        for k in got:
            assert np.abs(got[k]).max() > 0 and got[k].tobytes() == composed[k].tobytes(), (what, k)
    need = env._lib.sg_dqn_td_grad_workspace_bytes(env._h, C.byref(ho.struct), WIDTH_N)
    groups = -(-WIDTH_N // {1: 256, 2: 128, 3: 64, 4: 64}[-(-hidden // 32)])  # policy_grad_block by class
    assert need == 4 * (groups * (sum(int(W.size + bias.size) for W, bias in c["online"]) + 8) + WIDTH_N) <= ho.workspace.numel()
    env.check_status()
    env.close()


def _check_against_model(case, m64, m32, grads, stats, rows):
    got_rows = dict(zip(ROWS, _np(*[rows[k] for k in ROWS])))
    for k in ("g", "td_error"):
        _close(got_rows[k], m32["rows"][k], m64["rows"][k], case + (k,))
    s = _np(stats)[0]
    for k, name in enumerate(STATS):
        _close(s[k], m32["stats"][k], m64["stats"][k], case + (name,))
    assert s[2] == np.abs(got_rows["td_error"]).max() and s[7] == m64["stats"][7], case  # td_abs_max: exactly the largest row
    _check_grads(_grads_np(grads), flat(m32), flat(m64), case)
    return got_rows


@pytest.mark.parametrize("case", grad_cases(), ids=lambda c: "-".join(map(str, c)))
def test_outputs_equal_the_model(case):
    """3: g, td_error, the eight statistics and every gradient against the float64 model under the device's a*; the target against
    the pure model on the rows whose online gap is at least 1e-5, where the two argmaxes must agree"""
    obs_dim, n, hidden, n_hidden, activation, double_q, huber_delta, weighted = case
    env = _env_for(obs_dim, n)
    c = grad_case(obs_dim, n, hidden, n_hidden)
    ho, ht = _handle(env, c["online"], activation), _handle(env, c["target"], activation)
    b, w = _device_batch(c), _dev(c["weight"]) if weighted else None
    grads, stats, rows = _call(env, ho, ht, b, case, w)
    a_dev = _np(env.dqn_evaluate_raw_torch(ho, b["next_obs"])[3])[0]
    m64, m32 = _models(case, a_dev.tobytes())
    got_rows = _check_against_model(case, m64, m32, grads, stats, rows)
    pure64, pure32 = (reference(c, activation, double_q, huber_delta, weighted, dt) for dt in (np.float64, np.float32))
    clear = pure64["gap"] >= GAP if double_q else np.ones(n, bool)
    assert clear.mean() >= 0.99 and (not double_q or np.array_equal(a_dev[clear], pure64["a_star"][clear])), case
    same32 = clear if not double_q else clear & (pure32["a_star"] == pure64["a_star"])  # (the float32 model's own near-ties are its own)
    t = _tol(pure32["rows"]["target"][same32], pure64["rows"]["target"][same32])
    err = float(np.abs(got_rows["target"][clear] - pure64["rows"]["target"][clear]).max())
    WORST.append((err / t, err, t, case + ("target",)))
    assert err <= t, (case, "target", err, t)
    env.check_status()
    env.close()


def test_actions_outside_the_six_add_nothing_and_are_counted():
    """4: an action of 7 and one of -1: their g is exactly 0, bad_rows is 2, everything else within test 3's tolerances of the model,
    which drops the rows the same way"""
    import torch
    case = (15, 200, 33, 2, "relu", True, 1.0, True)
    env = _env_for(15, 200)
    c = grad_case(15, 200, 33, 2)
    c["batch"] = dict(c["batch"], action=c["batch"]["action"].copy())
    c["batch"]["action"][[3, 150]] = (7, -1)
    ho, ht = _handle(env, c["online"]), _handle(env, c["target"])
    b, w = _device_batch(c), _dev(c["weight"])
    grads, stats, rows = _call(env, ho, ht, b, case, w)
    a_dev = _np(env.dqn_evaluate_raw_torch(ho, b["next_obs"])[3])[0]
    m64, m32 = (td(c["online"], c["target"], c["batch"], weight=c["weight"], dtype=dt, a_star=a_dev) for dt in (np.float64, np.float32))
    got = _check_against_model(case + ("bad actions",), m64, m32, grads, stats, rows)
    s = _np(stats)[0]
    assert s[7] == 2 and got["g"][3] == 0 and got["g"][150] == 0 and got["td_error"][3] == 0 and got["td_error"][150] == 0
    assert np.count_nonzero(got["g"]) == 198
    # the bad rows' q_taken is Q_0, as sg_dqn_evaluate_device's
    assert _bits(rows["q_taken"]) == _bits(env.dqn_evaluate_raw_torch(ho, b["obs"], b["action"])[1])
    env.check_status()
    env.close()


K, B, N_DRAW, LR, TAU = 6, 200, 256, 1e-3, 0.005


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
    """an env with episodes of 3 steps, online and target modules with their handles, an Adam state, and a ring of 2 K slots with
    priorities, filled by rollout_dqn_torch in two chunks of K = 6 steps"""
    import torch
    env = make(GOAL, B, seed=seed, max_episode_steps=3)
    rng = np.random.default_rng(seed)
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    pairs = lambda net: [(m.weight, m.bias) for m in lin(net)]
    nets = random_dqn(rng, env.obs_dim, 64, 2), random_dqn(rng, env.obs_dim, 64, 2)
    om, tm = _modules(nets[0]), _modules(nets[1])
    ho, ht = env.dqn_torch(net=pairs(om)), env.dqn_torch(net=pairs(tm))
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
    env.rollout_dqn_torch(ho, first, rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=seed, first_step=0, epsilon=0.5, terminal=term)
    rows["obs"].copy_(first[1:])
    env.replay_commit_torch(ring, K, terminal=term, priority=prio)
    rows = ring.rows(K)
    env.rollout_dqn_torch(ho, ring.obs[K - 1:T], rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=seed, first_step=K, epsilon=0.5,
                          terminal=term)
    env.replay_commit_torch(ring, K, terminal=term, priority=prio)
    return env, nets, om, tm, ho, ht, opt, ring, prio


def _state(ho, ht, opt, prio):
    return [t.detach().clone() for t in (*ho.tensors, *ht.tensors, opt.state, *opt.exp_avg, *opt.exp_avg_sq, prio.leaf, prio.node, prio.hdr)]


def _restore(ho, ht, opt, prio, saved):
    import torch
    with torch.no_grad():
        for t, s in zip((*ho.tensors, *ht.tensors, opt.state, *opt.exp_avg, *opt.exp_avg_sq, prio.leaf, prio.node, prio.hdr), saved):
            t.copy_(s)


def test_one_learner_step_equals_the_step_composed_through_autograd():
    """6: a ring filled with K = 6 twice, episodes of 3 steps, 256 prioritized draws with n_step = 3; dqn_update_torch with prio and
    tau = 0.005 against the same step made of dqn_evaluate_torch autograd, adam_step_torch, the torch priority formula and a lerp.
    Both gradients are within the model's tolerance of the float64 gradient, so they are within twice that of each other; an Adam
    step from zero moments moves a parameter by lr u(g), u(g) = g / (|g| + eps): the parameters may differ by
    lr max |u(g +- 2 tol) - u(g)| plus two roundings.  Priorities agree on every cell whose |td| agrees"""
    import torch
    env, nets, om, tm, ho, ht, opt, ring, prio = _learner(31)
    batch = env.replay_sample_prioritized_torch(ring, prio, N_DRAW, seed=3, beta=0.4, n_step=3, gamma=0.97)
    torch.cuda.synchronize()
    assert len(set(_np(batch["steps"])[0].tolist())) > 1 and len(set(_np(batch["discount"])[0].tolist())) > 1  # (episodes of 3 steps cut the 3-step returns)
    before = _state(ho, ht, opt, prio)
    stats, rows, grads = env.dqn_update_torch(ho, ht, opt, batch, weight=batch["weight"], prio=prio, tau=TAU)
    torch.cuda.synchronize()
    fused = _state(ho, ht, opt, prio)
    fused_grads, td_fused = [t.clone() for pair in grads["net"] for t in pair], rows["td_error"].clone()
    assert int(opt.state[0, 0]) == 1 and all(not torch.equal(a, b) for a, b in zip(before[:12], fused[:12]))
    _restore(ho, ht, opt, prio, before)
    # the same step, composed
    with torch.no_grad():
        a2 = env.dqn_evaluate_raw_torch(ho, batch["next_obs"])[3]
        boot = env.dqn_evaluate_raw_torch(ht, batch["next_obs"], a2)[1]
        y = torch.where(batch["terminated"] != 0, batch["reward"], batch["reward"] + batch["discount"] * boot)
    q_taken = env.dqn_evaluate_torch(ho, batch["obs"], batch["action"])[1]
    (batch["weight"] * torch.nn.functional.huber_loss(q_taken, y, reduction="none", delta=1.0)).mean().backward()
    auto = dict(net=[(ho.tensors[l].grad, ho.tensors[l + 1].grad) for l in range(0, len(ho.tensors), 2)])
    env.adam_step_torch(opt, auto)
    td_auto = (q_taken - y).detach()
    env.replay_update_priorities_torch(prio, batch["cell"], td_auto, alpha=0.6, epsilon=1e-6)
    with torch.no_grad():
        torch._foreach_lerp_(list(ht.tensors), list(ho.tensors), TAU)
    torch.cuda.synchronize()
    composed = _state(ho, ht, opt, prio)
    # the tolerance of the gradients, from the model on the sampled batch
    nb = {k: _np(batch[k])[0] for k in ("obs", "action", "reward", "next_obs", "terminated", "discount")}
    wt = _np(batch["weight"])[0]
    m64, m32 = (td(nets[0], nets[1], nb, weight=wt, dtype=dt, a_star=_np(a2)[0]) for dt in (np.float64, np.float32))
    tol = grad_tolerances(flat(m32), flat(m64))
    names = [f"actor.{l}.{kind}" for l in range(3) for kind in ("weight", "bias")]
    u = lambda g: g / (np.abs(g) + 1e-8)
    for i, name in enumerate(names):
        g_f, g_a, g64 = _np(fused_grads[i])[0].astype(np.float64), _np(auto["net"][i // 2][i % 2])[0].astype(np.float64), flat(m64)[name]
        for what, g in (("fused", g_f), ("autograd", g_a)):
            err = float(np.abs(g - g64).max())
            WORST.append((err / tol[name], err, tol[name], ("learner step", what, name)))
            assert tol[name] <= 0.01 * np.abs(g64).max() and err <= tol[name], (what, name, err, tol[name])
        p_f, p_c, p_0 = (_np(s[i])[0].astype(np.float64) for s in (fused, composed, before))
        bound = LR * np.maximum(np.abs(u(g_a + 2 * tol[name]) - u(g_a)), np.abs(u(g_a - 2 * tol[name]) - u(g_a))) + 2 * np.spacing(np.abs(p_0).astype(np.float32))
        assert (np.abs(p_f - p_c) <= bound).all(), (name, float((np.abs(p_f - p_c) - bound).max()))
        assert np.abs(p_f - p_0).max() > 0.5 * LR and np.median(bound) < 0.01 * LR  # the step is there, and the bound is a small part of it
        t_f, t_c, t_0 = (_np(s[6 + i])[0].astype(np.float64) for s in (fused, composed, before))
        assert (np.abs(t_f - t_c) <= TAU * bound + 2 * np.spacing(np.abs(t_0).astype(np.float32))).all() and not np.array_equal(t_f, t_0), name
    # the priorities: equal wherever every draw of the cell carries the same |td| in both paths; elsewhere the cells still moved
    cell, same = _np(batch["cell"])[0], _np(td_fused.abs() == td_auto.abs())[0]
    leaf_f, leaf_c, leaf_0 = (_np(s[-3])[0].ravel() for s in (fused, composed, before))
    agree = np.array([same[cell == k].all() for k in cell])
    assert agree.mean() > 0.5 and np.array_equal(leaf_f[cell[agree]], leaf_c[cell[agree]])
    assert (leaf_f[cell] != leaf_0[cell]).mean() > 0.9
    other = np.ones(leaf_f.size, bool)
    other[cell] = False
    assert np.array_equal(leaf_f[other], leaf_0[other]) and np.array_equal(leaf_c[other], leaf_0[other])
    env.check_status()
    env.close()


def test_the_whole_learner_step_replays_as_a_graph():
    """7: the prioritized draw and dqn_update_torch with prio and a device-scalar tau, captured after a warm-up; two replays change
    the parameters, advance the optimizer and draw afresh; tau written as 1 between replays makes the next one a hard sync; a
    workspace that would have to grow inside a capture raises"""
    import torch
    env, nets, om, tm, ho, ht, opt, ring, prio = _learner(32)
    tau = torch.tensor(TAU, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream: sizes the workspace, makes the buffers
        batch = env.replay_sample_prioritized_torch(ring, prio, N_DRAW, seed=3, beta=0.4, n_step=3, gamma=0.97)
        stats, rows, grads = env.dqn_update_torch(ho, ht, opt, batch, weight=batch["weight"], prio=prio, tau=tau)
    side.synchronize()

    def step():
        env.replay_sample_prioritized_torch(ring, prio, N_DRAW, seed=3, beta=0.4, n_step=3, gamma=0.97, out=batch)
        env.dqn_update_torch(ho, ht, opt, batch, weight=batch["weight"], rows=rows, grads=grads, stats=stats, prio=prio, tau=tau)

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
        assert not stats.isnan().any() and float(stats[7]) == 0 and not torch.equal(cells[-2], cells[-1])
    assert all(not torch.equal(a, b) for a, b in zip(ho.tensors, ht.tensors))
    tau.fill_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ho.tensors, ht.tensors))
    env.check_status()
    h2 = env.dqn_torch(net=[(ho.tensors[l], ho.tensors[l + 1]) for l in range(0, 6, 2)])  # a fresh handle has no workspace
    stats.fill_(7.0)
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.dqn_td_grad_torch(h2, ht, batch, out=grads, stats=stats)
    torch.cuda.synchronize()
    assert h2.workspace is None and (stats == 7).all()
    env.check_status()
    env.close()


def test_native_refusals():
    """8: every refusal returns the error with a message that names the argument and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    n = 40
    env = make(GOAL, n)
    rng = np.random.default_rng(16)
    net = random_dqn(rng, env.obs_dim, 16, 1)
    ho, ht = _handle(env, net), _handle(env, net)
    f = lambda *shape: torch.full(shape, 7.0, device="cuda")
    batch = dict(obs=f(n, env.obs_dim), action=torch.zeros(n, dtype=torch.int32, device="cuda"), reward=f(n), next_obs=f(n, env.obs_dim),
                 terminated=torch.zeros(n, dtype=torch.uint8, device="cuda"), discount=f(n))
    grads, stats = env.dqn_td_grad_torch(ho, ht, batch)
    every = [x for pair in grads["net"] for x in pair] + [stats]
    for t in every:
        t.fill_(7.0)
    ws = ho.workspace
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()
    ref = lambda h: C.byref(h.struct) if h is not None else None
    need = lib.sg_dqn_td_grad_workspace_bytes(env._h, ref(ho), n)
    per_group = 4 * sum(int(W.size + b.size) for W, b in net)
    assert need == per_group + 4 * (8 + n) <= ws.numel()  # one workgroup's partial sums, its eight statistics sums, y [n]
    assert lib.sg_dqn_td_grad_workspace_bytes(env._h, ref(ho), 257) == 2 * per_group + 4 * (16 + 257)
    assert lib.sg_dqn_td_grad_workspace_bytes(env._h, ref(ho), 10 ** 7) == 256 * per_group + 4 * (256 * 8 + 10 ** 7)
    said = lambda e, match: match in lib.sg_last_error(e._h)
    for bad in (0, 2 ** 31):
        assert lib.sg_dqn_td_grad_workspace_bytes(env._h, ref(ho), bad) == 0 and said(env, b"n must be")

    def cfg(**over):
        c = _native.SgDqnTdConfig()
        lib.sg_dqn_td_config_init(C.byref(c))
        assert (c.struct_size, c.double_q, c.huber_delta, c.reserved) == (16, 1, 1.0, 0)
        for k, v in over.items():
            setattr(c, k, v)
        return c

    def bat(**over):
        cols = {k: batch[k].data_ptr() for k in batch}
        cols.update(over)
        return _native.SgDqnTdBatch(weight=None, **cols)

    def gr(**over):
        g = _native.SgDqnGrads(struct_size=C.sizeof(_native.SgDqnGrads))
        for l, (w, b) in enumerate(grads["net"]):
            g.net.weight[l], g.net.bias[l] = w.data_ptr(), b.data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def call(match, e=env, online=ho, target=ht, c=True, b=True, rows=n, g=True, st=stats, w=ws, wbytes=None):
        c = cfg() if c is True else c
        b = bat() if b is True else b
        g = gr() if g is True else g
        rc = lib.sg_dqn_td_grad_device(e._h, ref(online), ref(target), C.byref(c) if c is not None else None, C.byref(b) if b is not None else None,
                                       rows, C.byref(g) if g is not None else None, ptr(st), None, ptr(w), ws.numel() if wbytes is None else wbytes, s)
        assert rc == -1 and said(e, match), lib.sg_last_error(e._h)

    call(b"null dqn", online=None)
    call(b"null target", target=None)
    wide = _handle(env, random_dqn(rng, env.obs_dim, 17, 1))
    deep = _handle(env, random_dqn(rng, env.obs_dim, 16, 2))
    call(b"differ in shape", target=wide)
    call(b"differ in shape", target=deep)
    call(b"differ in shape", target=_handle(env, net, "tanh"))
    for field, bad, good, match in (("hidden", 129, 16, b"hidden"), ("n_hidden", 0, 1, b"n_hidden"), ("activation", 2, 1, b"activation"),
                                    ("struct_size", 8, C.sizeof(_native.SgDqn), b"struct_size"), ("reserved", 1, 0, b"reserved")):
        for h in (ho, ht):
            setattr(h.struct, field, bad)
            call(match)
            setattr(h.struct, field, good)
    call(b"null cfg", c=None)
    call(b"struct_size", c=cfg(struct_size=8))
    call(b"reserved", c=cfg(reserved=1))
    for bad in (0.0, -1.0, float("nan")):
        call(b"huber_delta must be > 0", c=cfg(huber_delta=bad))
    call(b"n must be", rows=0)
    call(b"n must be", rows=2 ** 31)
    call(b"null batch", b=None)
    call(b"null obs", b=bat(obs=None))
    for k in ("action", "reward", "next_obs", "terminated", "discount"):
        call(b"null batch." + k.encode(), b=bat(**{k: None}))
    call(b"null stats_out", st=None)
    call(b"null grads", g=None)
    call(b"struct_size", g=gr(struct_size=8))
    call(b"reserved", g=gr(reserved=1))
    hole = gr()
    hole.net.bias[1] = None
    call(b"layer 1 of the net", g=hole)
    call(b"null workspace", w=None)
    call(b"workspace of", wbytes=need - 1)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in every)
    env.check_status()
    # a continuous id: refused by the library and by the method
    con = make(CONTINUOUS, n)
    call(b"continuous", e=con)
    assert lib.sg_dqn_td_grad_workspace_bytes(con._h, ref(ho), n) == 0 and said(con, b"continuous")
    with pytest.raises(ValueError, match="continuous ids are not served"):
        con.dqn_td_grad_torch(ho, ht, batch)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in every)
    con.check_status()
    con.close()
    # the handles still work
    env.dqn_td_grad_torch(ho, ht, batch, out=grads, stats=stats)
    torch.cuda.synchronize()
    assert float(stats[7]) == 0 and float(stats[3]) == float(stats[3])
    env.check_status()
    env.close()


def test_report_the_worst_error_to_tolerance_ratios():
    """prints the three largest error / tolerance ratios the tests above met (they asserted each one at its place)"""
    WORST.sort(key=lambda r: -r[0])
    for ratio, err, tol, what in WORST[:3]:
        print("error / tolerance %.3f (error %.3g, tolerance %.3g) at" % (ratio, err, tol), what)
    assert all(r[0] <= 1.0 for r in WORST)
