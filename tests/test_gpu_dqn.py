"""GPU tests of dqn_torch / dqn_act_torch / rollout_dqn_torch / dqn_evaluate_raw_torch / dqn_grad_torch / dqn_evaluate_torch
(sg_dqn_act_device / sg_rollout_dqn_device / sg_dqn_evaluate_device / sg_dqn_grad_device) against the NumPy model tests/dqn_model.py.

q_all is checked under DESIGN section 17's rule: 8 x max|float32 CPU - float64| + 1e-6 (_tol), computed here.  Everything discrete is
checked EXACTLY and on every row: argmax, q_max and q_taken against the kernel's own q_all (a comparison with the model's argmax would
trip on near-ties of two Q values), the explore mask and the random actions against the model's integers.  A gradient tensor's tolerance
is section 18's: 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|), G32seq the model in float32 with the batch summed sequentially; every such
tolerance must also be at most 1 % of max|G64| of its tensor, so that a wrong index cannot hide (tests/test_dqn.py checks that cap on
the CPU for the very cases run here).

Row counts: 1 (a partial wave), 200 (more than one workgroup at every tile, no multiple of 64), 2049 (a last workgroup of one live
lane), and for the smallest workgroup (64 rows, hidden = 128) 256 x 64 + 300 rows, where the capped grid makes workgroups take a second
row tile."""
import ctypes as C

import numpy as np
import pytest

from dqn_model import ACTIONS, BIG_N, NETS, SELECTIONS, act, case, evaluate, flat, grad_case, grad_cases, grad_reference, grad_tolerances, random_dqn
from test_gpu_policy import _dev, _np, _tol, make

pytestmark = pytest.mark.gpu

GOAL, KEPLER, CONTINUOUS = "GoalDiscrete3-v0", "KeplerDiscrete-v0", "GoalContinuous3P-v0"


def _handle(env, net, activation="relu"):
    return env.dqn_torch(net=[(_dev(W), _dev(b)) for W, b in net], activation=activation)


def _env_for(obs_dim, n):
    env = make(GOAL if obs_dim == 15 else KEPLER, n)
    assert env.obs_dim == obs_dim and env.discrete
    return env


def _grads_np(out):
    import torch
    torch.cuda.synchronize()
    return flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["net"]]))


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


def _first_max(q):
    """(argmax, max) of a q_all tensor with the first maximum made explicit; torch.argmax has to point at a maximum too"""
    import torch
    mx = q.max(dim=1).values
    cols = torch.arange(q.shape[1], device=q.device).expand_as(q)
    first = torch.where(q == mx[:, None], cols, q.shape[1]).min(dim=1).values
    assert torch.equal(q.gather(1, torch.argmax(q, dim=1)[:, None])[:, 0], mx)
    return first.to(torch.int32), mx


def _check_discrete_outputs(env, h, d_obs, d_action, what):
    """argmax / q_max / q_taken are elements of the kernel's own q_all, bit for bit, on every row; returns (q_all, argmax) tensors"""
    import torch
    q_all, q_taken, q_max, argmax = env.dqn_evaluate_raw_torch(h, d_obs, d_action)
    torch.cuda.synchronize()
    first, mx = _first_max(q_all)
    assert torch.equal(argmax, first), what
    assert q_max.cpu().numpy().tobytes() == mx.cpu().numpy().tobytes(), what
    taken = q_all.gather(1, d_action.long()[:, None])[:, 0]
    assert q_taken.cpu().numpy().tobytes() == taken.cpu().numpy().tobytes(), what
    return q_all, argmax


@pytest.mark.parametrize("n", [1, 200, 2049])
@pytest.mark.parametrize("env_id", [GOAL, KEPLER])
def test_forward_argmax_and_the_greedy_act(env_id, n):
    """1: q_all against the float64 model, every net, both activations; argmax, q_max, q_taken exactly from the kernel's own q_all;
    dqn_act_torch(epsilon=0) returns that argmax and its Q value; rows alone and single outputs give the same bits"""
    import torch
    env = make(env_id, n, env_index_base=1000)
    rng = np.random.default_rng(n + len(env_id))
    obs = rng.standard_normal((n, env.obs_dim)).astype(np.float32)
    action = rng.integers(0, ACTIONS, n).astype(np.int32)
    d_obs, d_action = _dev(obs), _dev(action)
    worst = 0.0
    for hidden, n_hidden in NETS:
        for activation in ("tanh", "relu"):
            net = random_dqn(rng, env.obs_dim, hidden, n_hidden)
            h = _handle(env, net, activation)
            what = (env_id, n, hidden, n_hidden, activation)
            q_all, argmax = _check_discrete_outputs(env, h, d_obs, d_action, what)
            m64 = evaluate(net, obs, activation=activation)["q_all"]
            m32 = evaluate(net, obs, activation=activation, dtype=np.float32)["q_all"]
            t = _tol(m32, m64)
            err = float(np.abs(_np(q_all)[0] - m64).max())
            worst = max(worst, err / t)
            assert err <= t, (what, err, t)
            a, q = env.dqn_act_torch(h, d_obs, seed=5, step=9)  # epsilon 0: greedy
            torch.cuda.synchronize()
            assert torch.equal(a, argmax), what
            assert q.cpu().numpy().tobytes() == q_all.gather(1, argmax.long()[:, None])[:, 0].cpu().numpy().tobytes(), what
            only = env.dqn_evaluate_raw_torch(h, d_obs, out=dict(argmax=torch.full((n,), -1, dtype=torch.int32, device="cuda")))
            assert only[:3] == (None, None, None) and torch.equal(only[3], argmax)
            lo, hi = n // 3, n // 3 + max(1, n // 2)
            part = env.dqn_evaluate_raw_torch(h, d_obs[lo:hi].contiguous())[0]
            assert _np(part)[0].tobytes() == _np(q_all)[0][lo:hi].tobytes(), what
    print("q_all: largest error / tolerance (8 x |float32 CPU - float64| + 1e-6) over the nets:", env_id, n, "%.3f" % worst)
    env.check_status()
    env.close()


def test_equal_q_values_give_the_first_argmax():
    """1: ties are exact here (zero head weights, the biases are the Q values): the first maximum wins in evaluate and in act"""
    env = make(GOAL, 3)
    D = env.obs_dim
    obs = _dev(np.random.default_rng(0).standard_normal((3, D)).astype(np.float32))
    for bias, first in (([1, 3, 3, 2, 3, 0], 1), ([5, 5, 5, 5, 5, 5], 0), ([0, 0, 0, 0, 0, 1], 5), ([-1, -1, -2, -1, -3, -1], 0)):
        net = [(np.ones((4, D), np.float32), np.zeros(4, np.float32)), (np.zeros((ACTIONS, 4), np.float32), np.array(bias, np.float32))]
        h = _handle(env, net)
        q_all, _, q_max, argmax = _np(*env.dqn_evaluate_raw_torch(h, obs))
        assert np.array_equal(q_all, np.tile(np.array(bias, np.float32), (3, 1))) and argmax.tolist() == [first] * 3 and (q_max == max(bias)).all()
        a, q = _np(*env.dqn_act_torch(h, obs))
        assert a.tolist() == [first] * 3 and (q == max(bias)).all()
    env.check_status()
    env.close()


@pytest.mark.parametrize("env_id", [GOAL, KEPLER])
def test_epsilon_greedy_equals_the_models_integers(env_id):
    """2: B = 200 at epsilon 0.5: the action of EVERY env is the model's random action where the model explores and the kernel's own
    argmax elsewhere; q is the Q value of the action taken; a per-env epsilon of zeros and ones splits the batch exactly; two shards
    with their env_index_base reproduce the full batch; (seed, step) changes the draw"""
    import torch
    B = 200
    env = make(env_id, B, env_index_base=1000)
    parts = [make(env_id, 64, env_index_base=1064), make(env_id, 72, env_index_base=1128)]
    rng = np.random.default_rng(20 + len(env_id))
    obs = rng.standard_normal((B, env.obs_dim)).astype(np.float32)
    d_obs = _dev(obs)
    for (hidden, n_hidden), activation in zip(NETS, ("tanh", "relu", "relu", "tanh")):
        net = random_dqn(rng, env.obs_dim, hidden, n_hidden)
        h = _handle(env, net, activation)
        kw = dict(seed=77, step=2 ** 32 + 5)
        what = (env_id, hidden, n_hidden, activation)
        q_all, _, _, argmax = _np(*env.dqn_evaluate_raw_torch(h, d_obs))
        m = act(net, obs, epsilon=0.5, env_index_base=1000, activation=activation, **kw)
        assert 60 <= int(m["explore"].sum()) <= 140  # (0.5 +- 5.7 standard deviations: both branches are taken)
        a, q = _np(*env.dqn_act_torch(h, d_obs, epsilon=0.5, **kw))
        want = np.where(m["explore"], m["random_action"], argmax)
        assert np.array_equal(a, want), (what, int((a != want).sum()))
        assert a.dtype == np.int32 and a.min() >= 0 and a.max() < ACTIONS
        assert q.tobytes() == q_all[np.arange(B), a].tobytes(), what
        assert np.array_equal(a[~m["explore"]], argmax[~m["explore"]])  # rows that do not explore carry the greedy action
        a2, q2 = _np(*env.dqn_act_torch(h, d_obs, epsilon=0.5, **kw))
        assert a2.tobytes() == a.tobytes() and q2.tobytes() == q.tobytes()
        # a per-env epsilon: zeros never explore, ones always do; mixed with 0.5 it decides as the scalar where they agree
        eps = np.zeros(B, np.float32)
        eps[B // 2:] = 1.0
        pa, pq = _np(*env.dqn_act_torch(h, d_obs, epsilon=_dev(eps), **kw))
        assert np.array_equal(pa[:B // 2], argmax[:B // 2]) and np.array_equal(pa[B // 2:], m["random_action"][B // 2:]), what
        assert pq.tobytes() == q_all[np.arange(B), pa].tobytes()
        eps[::3] = 0.5
        mixed = act(net, obs, epsilon=eps, env_index_base=1000, activation=activation, **kw)
        ma = _np(env.dqn_act_torch(h, d_obs, epsilon=_dev(eps), **kw)[0])[0]
        assert np.array_equal(ma, np.where(mixed["explore"], mixed["random_action"], argmax)) and np.array_equal(ma[::3], a[::3]), what
        only_a = env.dqn_act_torch(h, d_obs, epsilon=0.5, out=dict(action=torch.zeros(B, dtype=torch.int32, device="cuda")), **kw)
        assert only_a[1] is None and _np(only_a[0])[0].tobytes() == a.tobytes()
        # the shards: rows 64 .. 127 and 128 .. 199 on handles of their own
        for part, (lo, hi) in zip(parts, ((64, 128), (128, 200))):
            hp = _handle(part, net, activation)
            sa, sq = _np(*part.dqn_act_torch(hp, _dev(obs[lo:hi]), epsilon=0.5, **kw))
            assert sa.tobytes() == a[lo:hi].tobytes() and sq.tobytes() == q[lo:hi].tobytes(), (what, lo)
            sa, _ = _np(*part.dqn_act_torch(hp, _dev(obs[lo:hi]), epsilon=_dev(eps[lo:hi]), **kw))
            assert sa.tobytes() == ma[lo:hi].tobytes(), (what, lo)
        # all explore: the actions are the draws themselves, and they follow seed and both words of the step
        ones = _dev(np.ones(B, np.float32))
        r0 = _np(env.dqn_act_torch(h, d_obs, epsilon=1.0, **kw)[0])[0]
        assert np.array_equal(r0, m["random_action"]) and np.array_equal(r0, _np(env.dqn_act_torch(h, d_obs, epsilon=ones, **kw)[0])[0])
        for other in (dict(seed=78, step=2 ** 32 + 5), dict(seed=77, step=2 ** 32 + 6), dict(seed=77, step=5)):
            r1 = _np(env.dqn_act_torch(h, d_obs, epsilon=1.0, **other)[0])[0]
            assert (r1 != r0).mean() > 0.5 and np.array_equal(r1, act(net, obs, epsilon=1.0, env_index_base=1000, activation=activation, **other)["random_action"])
    env.check_status()
    for e in [env] + parts:
        e.close()


@pytest.mark.parametrize("obs_dim,n,hidden,n_hidden,activation", grad_cases())
def test_gradients_equal_the_model(obs_dim, n, hidden, n_hidden, activation):
    """3: g_taken only, g_all only and both, within section 18's tolerance with the 1 % cap; two calls into NaN-prefilled buffers give
    the same bits; g_all of zeros beside g_taken gives the bits of g_taken alone.  n = 256 x 64 + 300 at hidden = 128: workgroups take
    a second row tile."""
    import torch
    assert n != BIG_N or (hidden == 128 and n > 256 * 64)
    env = _env_for(obs_dim, n)
    c = grad_case(obs_dim, n, hidden, n_hidden)
    h = _handle(env, c["net"], activation)
    d_obs, d_action, d_gt, d_ga = _dev(c["obs"]), _dev(c["action"]), _dev(c["g_taken"]), _dev(c["g_all"])
    worst = []
    what = (obs_dim, n, hidden, n_hidden, activation)
    taken_alone = None
    for sel in SELECTIONS:
        gt = d_gt if sel in ("both", "taken") else None
        ga = d_ga if sel in ("both", "all") else None
        out = env.dqn_grad_torch(h, d_obs, d_action if gt is not None else None, gt, ga)
        got = _grads_np(out)
        _check_grads(got, grad_reference(c, activation, sel, np.float32), grad_reference(c, activation, sel, np.float64), what + (sel,), worst)
        h.workspace.view(torch.float32).fill_(float("nan"))
        for w, b in out["net"]:
            w.fill_(float("nan"))
            b.fill_(float("nan"))
        again = _grads_np(env.dqn_grad_torch(h, d_obs, d_action, gt, ga, out=out))  # (an action beside a NULL g_taken is not looked at)
        for k in got:
            assert not np.isnan(again[k]).any() and again[k].tobytes() == got[k].tobytes(), (what, sel, k)
        if sel == "taken":
            taken_alone = got
    zeros = _grads_np(env.dqn_grad_torch(h, d_obs, d_action, d_gt, torch.zeros_like(d_ga)))
    for k in taken_alone:
        assert zeros[k].tobytes() == taken_alone[k].tobytes(), (what, k)
    _report(worst)
    env.check_status()
    env.close()


K, B = 6, 200


def _buffers(env, K):
    import torch
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    return dict(obs=z(K + 1, B, env.obs_dim), action=z(K, B, dtype=torch.int32), q=z(K, B), reward=z(K, B), done=z(K, B, dtype=torch.uint8),
                trunc=z(K, B, dtype=torch.uint8))


def _hand_loop(env, h, K, seed, first_step, epsilon):
    """dqn_act_torch then step_torch(terminal_obs=...) K times; the terminal records as a set of (step, env, obs bytes)"""
    import torch
    b = _buffers(env, K)
    b["obs"][0].copy_(env.reset_torch())
    tobs = torch.zeros((B, env.obs_dim), dtype=torch.float32, device="cuda")
    records = set()
    for t in range(K):
        env.dqn_act_torch(h, b["obs"][t], seed=seed, step=first_step + t, epsilon=epsilon, out=dict(action=b["action"][t], q=b["q"][t]))
        env.step_torch(b["action"][t], out=dict(obs=b["obs"][t + 1], reward=b["reward"][t], done=b["done"][t], trunc=b["trunc"][t]),
                       terminal_obs=tobs)
        d, to = _np(b["done"][t], tobs)
        for i in np.nonzero(d)[0]:
            records.add((t, int(i), to[i].tobytes()))
    return b, records


@pytest.mark.parametrize("env_id,normalize_obs", [(GOAL, False), (GOAL, True), (KEPLER, False)])
def test_rollout_equals_the_hand_written_loop(env_id, normalize_obs):
    """4: every output of rollout_dqn_torch, bit for bit, with a terminal list; max_episode_steps = 3 puts truncations and auto-resets
    inside the call (the list is unordered: compared as a set); with observation normalization on as well; a per-env epsilon tensor
    in the normalized run, the scalar in the others"""
    kw = dict(seed=21, max_episode_steps=3, normalize_obs=normalize_obs)
    ea, eb = make(env_id, B, **kw), make(env_id, B, **kw)
    rng = np.random.default_rng(10)
    net = random_dqn(rng, ea.obs_dim, 64, 2)
    ha, hb = _handle(ea, net), _handle(eb, net)
    epsilon = _dev(rng.uniform(0, 1, B).astype(np.float32)) if normalize_obs else 0.5
    want, records = _hand_loop(ea, ha, K, seed=4, first_step=100, epsilon=epsilon)
    got, term = _buffers(eb, K), eb.terminal_list_torch(1000)
    got["obs"][0].copy_(eb.reset_torch())
    eb.rollout_dqn_torch(hb, seed=4, first_step=100, epsilon=epsilon, terminal=term, **got)
    eb.check_status()
    for name in want:
        w, g = _np(want[name], got[name])
        assert w.tobytes() == g.tobytes(), (name, int((w != g).sum()))
    action, trunc, done, count, se, ob = _np(got["action"], got["trunc"], got["done"], term["count"], term["step_env"], term["obs"])
    assert len(set(action.ravel().tolist())) == ACTIONS  # every action is taken somewhere
    assert trunc[2].mean() > 0.9 and done.sum() >= 0.9 * B  # (nearly) every env runs into the time limit at t = 2
    n = int(count[0])
    listed = {(int(se[k, 0]), int(se[k, 1]), ob[k].tobytes()) for k in range(n)}
    assert n == int(done.sum()) == len(records) and listed == records
    # without q and without a list: the same actions and observations
    ec = make(env_id, B, **kw)
    hc = _handle(ec, net)
    bare = _buffers(ec, K)
    bare["obs"][0].copy_(ec.reset_torch())
    bare.pop("q")
    ec.rollout_dqn_torch(hc, seed=4, first_step=100, epsilon=epsilon, **bare)
    for name in bare:
        w, g = _np(want[name], bare[name])
        assert w.tobytes() == g.tobytes(), name
    for e in (ea, eb, ec):
        e.close()


def _fill_ring(env, h, steps, seed, epsilon):
    """a ring of `steps` slots filled by rollout_dqn_torch in two chunks of K = steps / 2, as a learner would"""
    import torch
    Kc = steps // 2
    ring = env.replay_torch(steps, term_capacity=steps * B)  # (episodes of 3 steps: up to a third of the live env-steps are terminal)
    env.replay_begin_torch(ring, env.reset_torch())
    term = env.terminal_list_torch(Kc * B)
    rows = ring.rows(Kc)
    first = torch.empty((Kc + 1, B, env.obs_dim), device="cuda")  # the first action's observation is the ring's last slot, not adjacent to slot 0
    first[0].copy_(ring.obs[steps - 1])
    env.rollout_dqn_torch(h, first, rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=seed, first_step=0, epsilon=epsilon, terminal=term)
    rows["obs"].copy_(first[1:])
    env.replay_commit_torch(ring, Kc, terminal=term)
    rows = ring.rows(Kc)
    assert ring.head == Kc
    env.rollout_dqn_torch(h, ring.obs[Kc - 1:steps], rows["action"], rows["reward"], rows["done"], rows["trunc"], seed=seed, first_step=Kc,
                          epsilon=epsilon, terminal=term)  # every buffer is the ring's own memory
    env.replay_commit_torch(ring, Kc, terminal=term)
    return ring


def test_rollout_into_a_replay_ring_and_a_sampled_batch():
    """4: the call's buffers are a replay ring's rows(K), followed by replay_commit_torch; the ring then holds the hand-written loop's
    transitions, and a replay_sample_torch batch carries int32 actions that dqn_evaluate_raw_torch takes as they are"""
    import torch
    kw = dict(seed=22, max_episode_steps=3)
    ea, eb = make(GOAL, B, **kw), make(GOAL, B, **kw)
    rng = np.random.default_rng(11)
    net = random_dqn(rng, ea.obs_dim, 33, 2)
    ha, hb = _handle(ea, net), _handle(eb, net)
    want, _ = _hand_loop(ea, ha, 2 * K, seed=6, first_step=0, epsilon=0.5)
    ring = _fill_ring(eb, hb, 2 * K, seed=6, epsilon=0.5)
    eb.check_status()
    assert ring.filled == 2 * K and len(ring) == (2 * K - 1) * B and ring.action.dtype == torch.int32
    for name, full in (("obs", want["obs"][1:]), ("action", want["action"]), ("reward", want["reward"]), ("done", want["done"]),
                       ("trunc", want["trunc"])):
        w, g = _np(full, getattr(ring, name))
        assert w.tobytes() == g.tobytes(), name
    assert _np(want["done"])[0].any()
    batch = eb.replay_sample_torch(ring, 256, seed=3)
    assert batch["action"].dtype == torch.int32 and tuple(batch["action"].shape) == (256,)
    q_all, q_taken, _, _ = _np(*eb.dqn_evaluate_raw_torch(hb, batch["obs"], batch["action"]))
    a = _np(batch["action"])[0]
    assert a.min() >= 0 and a.max() < ACTIONS and q_taken.tobytes() == q_all[np.arange(256), a].tobytes()
    ea.close()
    eb.close()


def _modules(net, activation, dtype, device):
    import torch
    mods = []
    for l, (W, b) in enumerate(net):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if l < len(net) - 1:
            mods.append(torch.nn.Tanh() if activation == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods).to(dtype=dtype, device=device)


def test_double_dqn_step_through_autograd():
    """5: a sampled batch of 256; the target is the online net's argmax on next_obs followed by the target net's q_taken with it, under
    no_grad; the Huber loss on q_taken goes through dqn_evaluate_torch(...).backward(); every .grad against float64 CPU modules fed the
    same numbers, under the per-tensor rule with g = d loss / d q_taken; then a loss on q_all alone, logsumexp(q_all).mean(), through
    the same Function.  The float64 target takes the device's argmax (a near-tie may round either way); the two argmaxes must agree on
    every row whose float64 gap between the two largest Q values is at least 1e-5."""
    import torch
    n, steps = 256, 8
    env = make(GOAL, B, seed=23, max_episode_steps=3)
    rng = np.random.default_rng(14)
    online, target = random_dqn(rng, env.obs_dim, 64, 2), random_dqn(rng, env.obs_dim, 64, 2)
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    pairs = lambda net: [(m.weight, m.bias) for m in lin(net)]
    named = lambda net: {f"actor.{l}.{kind}": getattr(m, kind).grad.detach().cpu().numpy() for l, m in enumerate(lin(net)) for kind in ("weight", "bias")}
    od, td = _modules(online, "relu", torch.float32, "cuda"), _modules(target, "relu", torch.float32, "cuda")
    ho, ht = env.dqn_torch(net=pairs(od)), env.dqn_torch(net=pairs(td))
    ring = _fill_ring(env, ho, steps, seed=7, epsilon=0.5)
    batch = env.replay_sample_torch(ring, n, seed=5)
    with torch.no_grad():
        a2 = env.dqn_evaluate_raw_torch(ho, batch["next_obs"])[3]
        boot = env.dqn_evaluate_torch(ht, batch["next_obs"], a2)[1]
        t_d = batch["reward"] + batch["discount"] * (1.0 - batch["terminated"].float()) * boot
    assert boot.grad_fn is None and not t_d.requires_grad
    q_all_d, q_taken_d = env.dqn_evaluate_torch(ho, batch["obs"], batch["action"])
    assert q_all_d.grad_fn is not None and q_taken_d.grad_fn is not None
    torch.nn.functional.smooth_l1_loss(q_taken_d, t_d).backward()
    obs, action, reward, next_obs, terminated, discount, a2_np, t_np = _np(batch["obs"], batch["action"], batch["reward"], batch["next_obs"],
                                                                           batch["terminated"], batch["discount"], a2, t_d)
    # float64 on the CPU, fed the batch the device sampled
    o64, t64 = _modules(online, "relu", torch.float64, "cpu"), _modules(target, "relu", torch.float64, "cpu")
    with torch.no_grad():
        x2 = torch.from_numpy(next_obs).double()
        q2 = o64(x2)
        top = q2.topk(2, dim=1).values
        clear = ((top[:, 0] - top[:, 1]) >= 1e-5).numpy()
        assert clear.mean() > 0.9 and np.array_equal(q2.argmax(1).numpy()[clear], a2_np[clear])
        boot64 = t64(x2).gather(1, torch.from_numpy(a2_np.astype(np.int64))[:, None])[:, 0]
        target64 = torch.from_numpy(reward).double() + torch.from_numpy(discount).double() * (1.0 - torch.from_numpy(terminated).double()) * boot64
    boot32 = evaluate(target, next_obs, a2_np, activation="relu", dtype=np.float32)["q_taken"]
    target32 = reward + discount * (np.float32(1) - terminated.astype(np.float32)) * boot32
    t = _tol(target32, target64.numpy())
    err = float(np.abs(t_np - target64.numpy()).max())
    print("Double DQN target: error %.3g tolerance %.3g" % (err, t))
    assert err <= t
    q64 = o64(torch.from_numpy(obs).double())
    taken64 = q64.gather(1, torch.from_numpy(action.astype(np.int64))[:, None])[:, 0]
    taken64.retain_grad()
    torch.nn.functional.smooth_l1_loss(taken64, target64).backward()
    g_t = taken64.grad.numpy().astype(np.float32)
    assert np.abs(g_t).max() > 0
    g32 = flat(evaluate(online, obs, action, g_t, None, activation="relu", dtype=np.float32))
    worst = []
    _check_grads(named(od), g32, named(o64), "Huber loss on q_taken", worst)
    assert all(m.weight.grad is None for m in lin(td))  # the target net took no gradient
    # a loss on q_all alone: the backward passes a NULL g_taken
    od.zero_grad()
    o64.zero_grad()
    torch.logsumexp(env.dqn_evaluate_torch(ho, batch["obs"]), dim=1).mean().backward()
    q64 = o64(torch.from_numpy(obs).double())
    q64.retain_grad()
    torch.logsumexp(q64, dim=1).mean().backward()
    g32 = flat(evaluate(online, obs, None, None, q64.grad.numpy().astype(np.float32), activation="relu", dtype=np.float32))
    _check_grads(named(od), g32, named(o64), "logsumexp(q_all)", worst)
    # with an action given but only q_all used: the same gradients (g_taken arrives as None)
    od.zero_grad()
    torch.logsumexp(env.dqn_evaluate_torch(ho, batch["obs"], batch["action"])[0], dim=1).mean().backward()
    _check_grads(named(od), g32, named(o64), "logsumexp(q_all), action given", worst)
    _report(worst)
    env.check_status()
    env.close()


def test_captured_calls_replay_the_eager_results_and_follow_the_epsilon_tensor():
    """6: dqn_act_torch + step_torch, and dqn_evaluate_raw_torch + dqn_grad_torch, captured after a warm-up and replayed: a new value
    written into the epsilon tensor between replays moves the explore mask without a re-capture; new contents of the learner's buffers
    give the eager results; a workspace that would have to grow inside a capture raises and launches nothing"""
    import torch
    n = 2049
    env = make(GOAL, n, seed=24)
    c = case(env.obs_dim, n, 64, 2, seed=15)
    rng = np.random.default_rng(15)
    h = _handle(env, c["net"])
    d_obs, d_action, d_gt, d_ga = _dev(c["obs"]), _dev(c["action"]), _dev(c["g_taken"]), _dev(c["g_all"])
    side = torch.cuda.Stream()
    z = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")
    eps = torch.zeros(n, device="cuda")
    obs0 = env.reset_torch().clone()
    snap = env.snapshot_torch()
    act_out = dict(action=z(n, dtype=torch.int32), q=z(n))
    step_out = dict(obs=z(n, env.obs_dim), reward=z(n), done=z(n, dtype=torch.uint8), trunc=z(n, dtype=torch.uint8))
    ev_out = dict(q_all=z(n, ACTIONS), q_taken=z(n), q_max=z(n), argmax=z(n, dtype=torch.int32))

    def actor():
        env.dqn_act_torch(h, obs0, seed=3, step=9, epsilon=eps, out=act_out)
        env.step_torch(act_out["action"], out=step_out)

    with torch.cuda.stream(side):  # the warm-up, on the capture's stream
        actor()
        g_out = env.dqn_grad_torch(h, d_obs, d_action, d_gt, d_ga)
    side.synchronize()

    def learner():
        env.dqn_evaluate_raw_torch(h, d_obs, d_action, out=ev_out)
        env.dqn_grad_torch(h, d_obs, d_action, d_gt, d_ga, out=g_out)

    act_graph, learn_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    env.restore_torch(snap)
    with torch.cuda.graph(act_graph, stream=side):
        actor()
    with torch.cuda.graph(learn_graph, stream=side):
        learner()
    greedy = env.dqn_evaluate_raw_torch(h, obs0)[3].clone()
    drawn = torch.from_numpy(act(c["net"], _np(obs0)[0], seed=3, step=9, epsilon=1.0)["random_action"]).cuda()
    masks = []
    for value in (0.0, 1.0, 0.3):
        eps.fill_(value)  # the only thing that changes between the replays
        env.restore_torch(snap)
        actor()
        torch.cuda.synchronize()
        want = [t.clone() for t in list(act_out.values()) + list(step_out.values())]
        for t in list(act_out.values()) + list(step_out.values()):
            t.zero_()
        env.restore_torch(snap)
        torch.cuda.synchronize()
        act_graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(w, t) for w, t in zip(want, list(act_out.values()) + list(step_out.values())))
        m = act(c["net"], _np(obs0)[0], seed=3, step=9, epsilon=value)["explore"]
        assert torch.equal(act_out["action"], torch.where(torch.from_numpy(m).cuda(), drawn, greedy))
        masks.append(float(m.mean()))
    assert masks[0] == 0.0 and masks[1] == 1.0 and 0.2 < masks[2] < 0.4
    every = lambda: list(ev_out.values()) + [x for pair in g_out["net"] for x in pair]
    draw = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    for _ in range(2):
        for t, shape in ((d_obs, (n, env.obs_dim)), (d_gt, (n,)), (d_ga, (n, ACTIONS))):  # new contents, the same buffers
            t.copy_(_dev(draw(*shape)))
        d_action.copy_(_dev(rng.integers(0, ACTIONS, n).astype(np.int32)))
        learner()
        torch.cuda.synchronize()
        want = [t.clone() for t in every()]
        for t in every():
            t.fill_(-1 if t.dtype == torch.int32 else float("nan"))
        torch.cuda.synchronize()
        learn_graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(w, t) and not (t.is_floating_point() and t.isnan().any()) for w, t in zip(want, every()))
    h2 = _handle(env, c["net"])  # a fresh handle has no workspace: inside a capture the call must raise before anything is enqueued
    g_out["net"][0][0].fill_(float("nan"))
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.dqn_grad_torch(h2, d_obs, d_action, d_gt, d_ga, out=g_out)
    torch.cuda.synchronize()
    assert h2.workspace is None and g_out["net"][0][0].isnan().all()
    env.check_status()
    env.close()


def test_native_refusals():
    """7: every refusal of the calls returns the error with a message that names the argument and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    n = 40
    env = make(GOAL, n)
    rng = np.random.default_rng(16)
    net = random_dqn(rng, env.obs_dim, 16, 1)
    h = _handle(env, net)
    d_obs = _dev(rng.standard_normal((n, env.obs_dim)).astype(np.float32))
    d_action = _dev(rng.integers(0, ACTIONS, n).astype(np.int32))
    a_out, q_out = torch.full((n,), 7, dtype=torch.int32, device="cuda"), torch.full((n,), 7.0, device="cuda")
    qa_out = torch.full((n, ACTIONS), 7.0, device="cuda")
    ones, ones6, eps_dev = torch.ones(n, device="cuda"), torch.ones((n, ACTIONS), device="cuda"), torch.ones(n, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, s = env._lib, env._stream()
    said = lambda match: match in lib.sg_last_error(env._h)
    ref = lambda hh: C.byref(hh.struct) if hh is not None else None

    def ac(hh, o, a, match, epsilon=0.5, e_dev=None):
        assert lib.sg_dqn_act_device(env._h, ref(hh), ptr(o), 0, 0, epsilon, ptr(e_dev), ptr(a), ptr(q_out), s) == -1 and said(match), \
            lib.sg_last_error(env._h)

    def ev(hh, rows, o, act_, outs, match):
        assert lib.sg_dqn_evaluate_device(env._h, ref(hh), rows, ptr(o), ptr(act_), *[ptr(t) for t in outs], s) == -1 and said(match), \
            lib.sg_last_error(env._h)

    all_out = (qa_out, q_out, q_out, a_out)
    ac(None, d_obs, a_out, b"null dqn")
    ac(h, None, a_out, b"null obs")
    ac(h, d_obs, None, b"null action_out")
    for bad in (float("nan"), -0.5, 1.5, float("inf")):
        ac(h, d_obs, a_out, b"epsilon must be in [0, 1]", epsilon=bad)
        ac(h, d_obs, a_out, b"epsilon must be in [0, 1]", epsilon=bad, e_dev=eps_dev)
    ev(None, n, d_obs, d_action, all_out, b"null dqn")
    ev(h, 0, d_obs, d_action, all_out, b"n must be")
    ev(h, n, None, d_action, all_out, b"null obs")
    ev(h, n, d_obs, d_action, (None, None, None, None), b"no output")
    ev(h, n, d_obs, None, all_out, b"null action (q_taken_out given)")
    for field, bad, good, match in (("hidden", 129, 16, b"hidden"), ("hidden", 0, 16, b"hidden"), ("n_hidden", 4, 1, b"n_hidden"),
                                    ("n_hidden", 0, 1, b"n_hidden"), ("activation", 2, 1, b"activation"),
                                    ("struct_size", 8, C.sizeof(_native.SgDqn), b"struct_size"), ("reserved", 1, 0, b"reserved")):
        setattr(h.struct, field, bad)
        ac(h, d_obs, a_out, match)
        ev(h, n, d_obs, d_action, all_out, match)
        assert lib.sg_dqn_grad_workspace_bytes(env._h, ref(h), n) == 0 and said(match)
        setattr(h.struct, field, good)
    keep = h.struct.net.bias[1]
    h.struct.net.bias[1] = None
    ac(h, d_obs, a_out, b"layer 1 of the net")
    h.struct.net.bias[1] = keep
    # the grad call
    full = env.dqn_grad_torch(h, d_obs, d_action, ones, ones6)
    every = [x for pair in full["net"] for x in pair]
    for t in every:
        t.fill_(7.0)
    ws = h.workspace
    need = lib.sg_dqn_grad_workspace_bytes(env._h, ref(h), n)
    per_group = 4 * sum(int(W.size + b.size) for W, b in net)  # the partial sums of one workgroup: every parameter, nothing else
    assert need == per_group <= ws.numel() and need == lib.sg_dqn_grad_workspace_bytes(env._h, ref(h), 256)
    assert lib.sg_dqn_grad_workspace_bytes(env._h, ref(h), 257) == 2 * need  # a second workgroup's partial sums
    assert lib.sg_dqn_grad_workspace_bytes(env._h, ref(h), 10 ** 7) == 256 * need  # the grid cap bounds it
    assert lib.sg_dqn_grad_workspace_bytes(env._h, ref(h), 0) == 0 and said(b"n must be")

    def struct(**over):
        g = _native.SgDqnGrads(struct_size=C.sizeof(_native.SgDqnGrads))
        for l, (w, b) in enumerate(full["net"]):
            g.net.weight[l], g.net.bias[l] = w.data_ptr(), b.data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def gr(rows, o, act_, gt, ga, g, w, wbytes, match):
        rc = lib.sg_dqn_grad_device(env._h, ref(h), rows, ptr(o), ptr(act_), ptr(gt), ptr(ga), C.byref(g) if g is not None else None, ptr(w), wbytes, s)
        assert rc == -1 and said(match), lib.sg_last_error(env._h)

    gr(0, d_obs, d_action, ones, ones6, struct(), ws, ws.numel(), b"n must be")
    gr(n, None, d_action, ones, ones6, struct(), ws, ws.numel(), b"null obs")
    gr(n, d_obs, d_action, None, None, struct(), ws, ws.numel(), b"both NULL")
    gr(n, d_obs, None, ones, ones6, struct(), ws, ws.numel(), b"null action (g_taken given)")
    gr(n, d_obs, d_action, ones, ones6, None, ws, ws.numel(), b"null grads")
    gr(n, d_obs, d_action, ones, ones6, struct(struct_size=8), ws, ws.numel(), b"struct_size")
    gr(n, d_obs, d_action, ones, ones6, struct(reserved=1), ws, ws.numel(), b"reserved")
    bad = struct()
    bad.net.bias[1] = None
    gr(n, d_obs, d_action, ones, ones6, bad, ws, ws.numel(), b"layer 1 of the net")
    gr(n, d_obs, d_action, ones, ones6, struct(), None, ws.numel(), b"null workspace")
    gr(n, d_obs, d_action, ones, ones6, struct(), ws, need - 1, b"workspace of")
    # the rollout
    b = {k: torch.full_like(v[:, :n].contiguous(), 7) for k, v in _buffers(env, 2).items()}

    def ro(steps, bufs, tl, match, epsilon=0.5):
        rc = lib.sg_rollout_dqn_device(env._h, steps, ref(h), 0, 0, epsilon, None, ptr(bufs["obs"]), ptr(bufs["action"]), ptr(bufs["q"]),
                                       ptr(bufs["reward"]), ptr(bufs["done"]), ptr(bufs["trunc"]), C.byref(tl) if tl is not None else None, s)
        assert rc == -1 and said(match), lib.sg_last_error(env._h)

    ro(0, b, None, b"n_steps")
    for k in ("obs", "action", "reward", "done", "trunc"):
        ro(2, {**b, k: None}, None, b"null buffer")
    ro(2, b, None, b"epsilon must be in [0, 1]", epsilon=float("nan"))
    ro(2, b, None, b"epsilon must be in [0, 1]", epsilon=1.25)
    ro(2, b, _native.SgTerminalList(None, None, None, 4), b"incomplete terminal list")
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in [a_out, q_out, qa_out] + every + list(b.values()))
    env.check_status()
    # a continuous id: every call is refused, by the library and by the methods
    con = make(CONTINUOUS, n)
    d_obs_con = torch.zeros((n, con.obs_dim), device="cuda")
    said_con = lambda match: match in lib.sg_last_error(con._h)
    assert lib.sg_dqn_act_device(con._h, ref(h), ptr(d_obs_con), 0, 0, 0.0, None, ptr(a_out), None, s) == -1 and said_con(b"continuous")
    assert lib.sg_dqn_evaluate_device(con._h, ref(h), n, ptr(d_obs_con), None, ptr(qa_out), None, None, None, s) == -1 and said_con(b"continuous")
    assert lib.sg_dqn_grad_device(con._h, ref(h), n, ptr(d_obs_con), None, None, ptr(ones6), C.byref(struct()), ptr(ws), ws.numel(), s) == -1
    assert said_con(b"continuous")
    assert lib.sg_dqn_grad_workspace_bytes(con._h, ref(h), n) == 0 and said_con(b"continuous")
    assert lib.sg_rollout_dqn_device(con._h, 2, ref(h), 0, 0, 0.0, None, ptr(b["obs"]), ptr(b["action"]), None, ptr(b["reward"]), ptr(b["done"]),
                                     ptr(b["trunc"]), None, s) == -1 and said_con(b"continuous")
    with pytest.raises(ValueError, match="continuous ids are not served"):
        con.dqn_torch(net=[(_dev(np.zeros((4, con.obs_dim), np.float32)), _dev(np.zeros(4, np.float32))),
                           (_dev(np.zeros((ACTIONS, 4), np.float32)), _dev(np.zeros(ACTIONS, np.float32)))])
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in [a_out, q_out, qa_out] + every + list(b.values()))
    con.check_status()
    con.close()
    # the handle still works
    env.dqn_evaluate_raw_torch(h, d_obs, d_action)
    env.dqn_grad_torch(h, d_obs, d_action, ones)
    torch.cuda.synchronize()
    env.check_status()
    env.close()
