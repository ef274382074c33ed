"""GPU tests of adam_torch / adam_step_torch / adam_exploit_torch (sg_adam_step_device / sg_adam_exploit_device).

The oracle is tests/adam_model.py in its float32 form, BIT FOR BIT: parameters, both moments and the whole state row.  The model is
checked against torch.optim.Adam / AdamW and clip_grad_norm_ on float64 tensors by tests/test_adam.py.  The nets are small enough that
every element is compared."""
import ctypes as C
import math

import numpy as np
import pytest

import adam_model as am
from dqn_model import random_dqn
from policy_model import random_policy
from population_model import random_population
from q_model import random_qnet
from squashed_model import random_squashed
from test_gpu_policy import DISCRETE, GOAL, _dev, _handle, _np, make
from test_gpu_population import _pop_handle

pytestmark = pytest.mark.gpu

P3_HYPER = dict(lr=[3e-4, 1e-3, 2.5e-4], betas=([0.9, 0.8, 0.9], [0.999, 0.99, 0.999]), eps=[1e-8, 1e-5, 1e-8],
                weight_decay=[0.0, 0.01, 0.0], max_grad_norm=[0.5, 1e4, None])  # member 0 clips, 1 never does, 2 has clipping off
NORMAL_MIN = 1.1754944e-38  # the smallest normal float32


def _flat(handle, grads):
    from space_gym_amd.vector_env import _flat_grads
    flat = list(_flat_grads(handle, grads))
    return flat + [None] * (len(handle.tensors) - len(flat))


def _grads_dict(handle, ts):
    """tensors shaped like handle.tensors as the dict an actor-critic's *_grad_torch returns"""
    L = handle.n_hidden + 1
    pairs = lambda xs: [(xs[2 * l], xs[2 * l + 1]) for l in range(L)]
    return dict(actor=pairs(ts[:2 * L]), critic=pairs(ts[2 * L:4 * L]) if handle.has_critic else None, log_std=ts[-1] if len(ts) % 2 else None)


def _lead(arrays, P, stacked):
    return [a if stacked else a.reshape((1,) + a.shape) for a in arrays]


def _read(opt):
    """(tensors, exp_avg, exp_avg_sq, state, hyper) as NumPy arrays [P, ...]"""
    stacked = hasattr(opt.handle, "members")
    t, ea, es = (_lead(_np(*ts), opt.members, stacked) for ts in (opt.handle.tensors, opt.exp_avg, opt.exp_avg_sq))
    st, hy = _np(opt.state, opt.hyper)
    return t, ea, es, st, hy


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _eq(got, want):
    """the same bits, a NaN standing for any NaN (its sign and payload are the processor's choice, not the contract's)"""
    nan = np.isnan(got)
    return got.shape == want.shape and np.array_equal(nan, np.isnan(want)) and got[~nan].tobytes() == want[~nan].tobytes()


def _step_and_compare(env, opt, grads, what):
    """one adam_step_torch against the float32 model from the state before it; returns the state read back after it"""
    stacked = hasattr(opt.handle, "members")
    t0, ea0, es0, st0, hy = _read(opt)
    flat = _flat(opt.handle, grads)
    g_np = [None if g is None else _lead(_np(g), opt.members, stacked)[0] for g in flat]
    before = [g.copy() for g in g_np if g is not None]
    assert env.adam_step_torch(opt, grads) is opt.state
    t1, ea1, es1, st1, hy1 = _read(opt)
    wt, wea, wes, wst = am.adam_step(t0, g_np, ea0, es0, hy, st0)
    for name, got, want in (("param", t1, wt), ("exp_avg", ea1, wea), ("exp_avg_sq", es1, wes)):
        for k in range(len(got)):
            assert _eq(got[k], want[k]), (what, name, k, int((got[k] != want[k]).sum()), got[k].size)
    assert _eq(st1, wst), (what, st1, wst)
    assert hy1.tobytes() == hy.tobytes()
    assert _same([g for g in _lead(_np(*[g for g in flat if g is not None]), opt.members, stacked)], before), "the gradients are read only"
    # the reported norm against the exactly summed squares: one float32 rounding (2^-24) plus the float64 sum's error (N 2^-53 <= 2^-36)
    for m in range(opt.members):
        exact = math.sqrt(math.fsum(float(x) * float(x) for g in g_np if g is not None for x in g[m].reshape(-1)))
        if math.isfinite(exact):
            assert abs(st1[m, am.GRAD_NORM] - exact) <= exact * 2.0 ** -23, (what, m, st1[m, am.GRAD_NORM], exact)
    return t1, ea1, es1, st1


def _p3_grads(rng, handle, special):
    """dense N(0, 1) gradients for three members; tensor `special` of member 2 holds zeros and |g| between 1e-22 and 1e-20"""
    out = []
    for k, t in enumerate(handle.tensors):
        g = rng.standard_normal(tuple(t.shape)).astype(np.float32)
        g[1] *= np.float32(3.0)
        if k == special:
            tiny = (10.0 ** rng.uniform(-22, -20, g[2].shape) * rng.choice([-1.0, 1.0], g[2].shape)).astype(np.float32)
            g[2] = np.where(rng.random(g[2].shape) < 0.3, np.float32(0), tiny)
        out.append(_dev(g))
    return _grads_dict(handle, out)


def _p3_case(env_id, hidden, n_hidden, activation, seed, P=3, **hyper):
    env = make(env_id, 2 * P)
    rng = np.random.default_rng(seed)
    continuous = not env.discrete
    pop = random_population(rng, P, env.obs_dim, hidden, n_hidden, 2 if continuous else 6, critic=True, continuous=continuous)
    h = _pop_handle(env, pop, activation)
    return env, rng, pop, h, env.adam_torch(h, **(hyper or P3_HYPER))


@pytest.mark.parametrize("env_id,hidden,n_hidden,activation", [(GOAL, 33, 1, "relu"), (DISCRETE, 64, 2, "tanh")])
def test_three_steps_of_a_population_are_the_models_bits(env_id, hidden, n_hidden, activation):
    """1: odd sizes and unaligned member slices (weight 33 x 15, head 2 x 33, log_std 2) and the four-wide path (64 x 64)"""
    env, rng, pop, h, opt = _p3_case(env_id, hidden, n_hidden, activation, seed=21)
    assert opt.members == 3 and tuple(opt.hyper.shape) == (3, 8) and tuple(opt.state.shape) == (3, 8)
    assert _np(opt.state)[0].tobytes() == am.fresh_state(3).tobytes()
    assert _np(opt.hyper)[0].tobytes() == am.make_hyper(3, **P3_HYPER).tobytes()
    assert all(not x.any() for x in _np(*opt.exp_avg, *opt.exp_avg_sq))
    for step in range(3):
        t, ea, es, st = _step_and_compare(env, opt, _p3_grads(rng, h, special=0), (env_id, step))
        assert st[0, am.CLIP_SCALE] < 0.1 and st[1, am.CLIP_SCALE] == 1 and st[2, am.CLIP_SCALE] == 1, st
        assert np.array_equal(st[:, am.STEPS], [step + 1] * 3) and np.array_equal(st[:, am.APPLIED], [1, 1, 1])
        if step == 0:  # member 2's second moments of the tiny gradients are subnormal: neither flushed nor approximately rooted
            v = es[0][2]
            sub = (v > 0) & (v < NORMAL_MIN)
            assert sub.sum() >= 10 and (v == 0).any(), (int(sub.sum()), v.size)
            assert (ea[0][2][sub] != 0).all()
    env.check_status()
    env.close()


def _family_case(family):
    """(env, handle, grads of the family's own *_grad_torch on 64 rows)"""
    import torch
    n = 64
    rng = np.random.default_rng(len(family))
    env = make(DISCRETE if family == "dqn" else GOAL, n)
    D = env.obs_dim
    obs = _dev(rng.standard_normal((n, D)).astype(np.float32))
    vec = lambda *s: _dev(rng.standard_normal(s).astype(np.float32))
    if family == "policy":
        h = _handle(env, random_policy(rng, D, 33, 1, 2, critic=True, continuous=True), "relu")
        grads = env.policy_grad_torch(h, obs, vec(n, 2), vec(n), vec(n), vec(n))
    elif family == "q":
        h = env.q_torch(critics=[[(_dev(W), _dev(b)) for W, b in layers] for layers in random_qnet(rng, D, 33, 2)], activation="relu")
        grads = env.q_grad_torch(h, obs, vec(n, 2), vec(n), vec(n))
    elif family == "squashed":
        h = env.squashed_policy_torch(actor=[(_dev(W), _dev(b)) for W, b in random_squashed(rng, D, 33, 1)], activation="relu")
        grads = env.squashed_grad_torch(h, obs, vec(n, 2), vec(n, 2), vec(n))
    else:
        h = env.dqn_torch(net=[(_dev(W), _dev(b)) for W, b in random_dqn(rng, D, 33, 2)], activation="relu")
        grads = env.dqn_grad_torch(h, obs, _dev(rng.integers(0, 6, n).astype(np.int32)), vec(n))
    torch.cuda.synchronize()
    return env, h, grads


@pytest.mark.parametrize("family", ["policy", "q", "squashed", "dqn"])
def test_one_step_of_every_family_is_the_models_bits(family):
    """2: P = 1 on a Policy, a twin QNet, a SquashedPolicy and a Dqn handle; the gradients are the family's own"""
    env, h, grads = _family_case(family)
    opt = env.adam_torch(h, lr=1e-3, weight_decay=0.01, max_grad_norm=0.5)
    assert opt.members == 1 and len(opt.exp_avg) == len(h.tensors)
    t, ea, es, st = _step_and_compare(env, opt, grads, family)
    assert st[0, am.APPLIED] == 1 and 0 < st[0, am.CLIP_SCALE] < 1, st  # sums over 64 rows: the norm is far above 0.5
    assert all(x.any() for x in ea)
    env.check_status()
    env.close()


def test_a_frozen_critic_keeps_its_bits_and_stays_out_of_the_norm():
    env, h, grads = _family_case("policy")
    opt = env.adam_torch(h, lr=1e-3, max_grad_norm=0.5)
    before = _np(*h.tensors)
    whole = math.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in _np(*_flat(h, grads))))
    frozen = dict(grads, critic=None)
    t, ea, es, st = _step_and_compare(env, opt, frozen, "frozen")
    L = h.n_hidden + 1
    for k in range(len(h.tensors)):
        critic = 2 * L <= k < 4 * L
        assert (t[k][0].tobytes() == before[k].tobytes()) == critic, k
        assert ea[k].any() != critic and es[k].any() != critic, k
    assert st[0, am.GRAD_NORM] < 0.999 * whole
    env.close()


def test_a_nan_stays_inside_its_member():
    """3: a NaN gradient element of member 1 skips member 1 only; a NaN learning rate of member 1 changes member 1 only"""
    results = {}
    for what in ("clean", "nan_grad", "nan_lr"):
        env, rng, pop, h, opt = _p3_case(GOAL, 33, 1, "relu", seed=22)
        grads = _p3_grads(rng, h, special=0)
        _step_and_compare(env, opt, grads, what)  # (a first step: the moments and the state are not the fresh ones)
        start = _read(opt)
        grads = _p3_grads(rng, h, special=0)
        if what == "nan_grad":
            grads["actor"][1][0][1, 1, 5] = float("nan")
        elif what == "nan_lr":
            opt.hyper[1, 0] = float("nan")
        results[what] = (start, _step_and_compare(env, opt, grads, what))
        env.check_status()
        env.close()
    member = lambda r, m: b"".join(x[m].tobytes() for part in r[:3] for x in part) + r[3][m].tobytes()
    clean = results["clean"][1]
    for what in ("nan_grad", "nan_lr"):
        start, got = results[what]
        assert member(got, 0) == member(clean, 0) and member(got, 2) == member(clean, 2), what
        assert member(got, 1) != member(clean, 1), what
    start, got = results["nan_grad"]
    assert all(_same([x[1] for x in a], [x[1] for x in b]) for a, b in zip(got[:3], start[:3]))
    st = got[3]
    assert st[1, :3].tobytes() == start[3][1, :3].tobytes() and st[1, am.SKIPPED] == 1 and st[1, am.APPLIED] == 0 and np.isnan(st[1, am.GRAD_NORM])
    assert np.array_equal(st[:, am.STEPS], [2, 1, 2])
    st = results["nan_lr"][1][3]
    assert st[1, am.APPLIED] == 1 and np.isnan(st[1, am.STEP_SIZE]) and all(np.isnan(x[1]).all() for x in results["nan_lr"][1][0])


def test_two_runs_give_the_same_bits_and_a_captured_step_follows_hyper():
    """4a: determinism; the step captured and replayed three times against three eager steps, hyper[:, 0] rewritten between replays"""
    import torch
    runs = []
    for mode in ("eager", "eager", "graph"):
        env, rng, pop, h, opt = _p3_case(DISCRETE, 64, 2, "tanh", seed=23)
        grads = _p3_grads(rng, h, special=2)
        lrs = [_dev(np.array(x, np.float32)) for x in ([3e-4, 1e-3, 2.5e-4], [1e-2, 1e-4, 0.0], [5e-3, 5e-3, 5e-3])]
        if mode == "graph":
            saved = [x.clone() for x in (*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state)]
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                env.adam_step_torch(opt, grads)
            side.synchronize()
            for x, s in zip((*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state), saved):
                x.copy_(s)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                env.adam_step_torch(opt, grads)
            assert _same(_np(*h.tensors, opt.state), _np(*saved[:len(h.tensors)], saved[-1])), "a capture runs nothing"
        seen = []
        for lr in lrs:
            opt.hyper[:, 0].copy_(lr)
            if mode == "graph":
                torch.cuda.synchronize()
                graph.replay()
            else:
                env.adam_step_torch(opt, grads)
            seen.append(_np(*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state))
        runs.append(seen)
        env.check_status()
        env.close()
    for a, b, c in zip(*runs):
        assert _same(a, b) and _same(a, c)
    assert not _same(runs[0][0], runs[0][1])
    # the rewritten learning rates were seen: step_size = lr / (1 - beta1_pow) of the third step
    st = runs[2][2][-1]
    want = [np.float32(np.float64(np.float32(5e-3)) / (1.0 - st[m, am.BETA1_POW])) for m in range(3)]
    assert np.array_equal(st[:, am.STEP_SIZE], want)


def test_one_ppo_iteration_in_a_single_graph():
    """4b: rollout, GAE, two minibatches of gradients each followed by the Adam step, captured as ONE graph on the discrete id; the
    replays give the eager sequence's parameters bit for bit, and the next rollout's first PPO ratio is exactly 1: the kernels read
    the parameters where the optimizer wrote them"""
    import torch
    B, P, K, n = 64, 2, 4, 64
    env = make(DISCRETE, B, seed=5, max_episode_steps=6)
    rng = np.random.default_rng(24)
    pop = random_population(rng, P, env.obs_dim, 64, 2, 6, critic=True, continuous=False)
    h = _pop_handle(env, pop, "tanh")
    opt = env.adam_torch(h, lr=[1e-3, 3e-3], max_grad_norm=[0.5, None])
    D = env.obs_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, dtype=torch.int32), logp=z(K, B), value=z(K + 1, B), reward=z(K, B),
             done=z(K, B, dtype=torch.uint8), trunc=z(K, B, dtype=torch.uint8))
    tv, adv, ret = z(K, B), z(K, B), z(K, B)
    per = B // P
    index = [_dev(np.stack([rng.integers(0, K, n) * B + per * m + rng.integers(0, per, n) for m in range(P)]).astype(np.int64)) for _ in range(2)]
    batch = dict(obs=b["obs"][:-1].reshape(K * B, D), action=b["action"].reshape(K * B), logp=b["logp"].reshape(K * B),
                 value=b["value"][:-1].reshape(K * B), advantage=adv.reshape(K * B), ret=ret.reshape(K * B))
    b["obs"][-1].copy_(env.reset_torch())
    grads, stats = env.population_ppo_grad_torch(h, batch, index[0])  # (the output tensors and the workspace, before any capture)

    def iteration():
        b["obs"][0].copy_(b["obs"][-1])
        env.rollout_population_torch(h, seed=3, terminal_value=tv, **b)
        env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1], terminal_value=tv, out=dict(advantage=adv, returns=ret))
        for idx in index:
            env.population_ppo_grad_torch(h, batch, idx, ent_coef=0.01, out=grads, stats=stats)
            env.adam_step_torch(opt, grads)

    live = (*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state, b["obs"])
    snap = env.snapshot_torch()
    saved = [x.clone() for x in live]

    def rewind():
        env.restore_torch(snap)
        for x, s in zip(live, saved):
            x.copy_(s)
        torch.cuda.synchronize()

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        iteration()
    side.synchronize()
    rewind()
    eager = []
    for _ in range(2):
        iteration()
        eager.append(_np(*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state))
    assert not _same(eager[0], eager[1]) and np.array_equal(eager[1][-1][:, am.STEPS], [4, 4])
    assert all(np.isfinite(x).all() for x in eager[1])
    rewind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        iteration()
    assert _same(_np(*h.tensors), _np(*saved[:len(h.tensors)])), "a capture runs nothing"
    for want in eager:
        graph.replay()
        assert _same(_np(*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state), want)
    # the next rollout under the updated parameters: every stored logp is the update's recomputed one, ratio exactly 1
    b["obs"][0].copy_(b["obs"][-1])
    env.rollout_population_torch(h, seed=4, terminal_value=tv, **b)
    rows = {k: torch.full((P, n), float("nan"), device="cuda") for k in ("logp", "value", "g_logp", "g_value")}
    env.population_ppo_grad_torch(h, batch, index[0], rows=rows, out=grads, stats=stats)
    new, old, idx = _np(rows["logp"], batch["logp"], index[0])
    assert new.tobytes() == old[idx].tobytes()
    env.check_status()
    env.close()


def _exploit_case():
    """P = 4 after two different steps: every member's parameters, moments and state differ"""
    env, rng, pop, h, opt = _p3_case(GOAL, 33, 1, "relu", seed=25, P=4, lr=[1e-3, 2e-3, 3e-3, 4e-3], betas=([0.9, 0.8, 0.85, 0.95], [0.999, 0.99, 0.98, 0.995]),
                                      max_grad_norm=[0.5, None, 1.0, None])
    for _ in range(2):
        gs = [_dev(rng.standard_normal(tuple(t.shape)).astype(np.float32)) for t in h.tensors]
        gs[0][3, 0, 0] = float("inf") if _ else 1.0  # member 3 skips its second step: the skipped counts differ
        env.adam_step_torch(opt, _grads_dict(h, gs))
    return env, rng, h, opt


def _assert_exploit(before, after, src):
    wt, wea, wes, wst, refused = am.adam_exploit(*before[:4], src)
    for got, want in zip(after[:3], (wt, wea, wes)):
        assert _same(got, want)
    assert after[3].tobytes() == wst.tobytes() and after[4].tobytes() == before[4].tobytes()
    return refused


def test_exploit_copies_parameters_moments_and_the_running_state():
    """5a: truncation on P = 4, then a step of losers and winners with equal gradients and hyper"""
    import torch
    env, rng, h, opt = _exploit_case()
    before = _read(opt)
    assert len({before[3][m, :4].tobytes() for m in range(4)}) == 4 and before[3][3, am.SKIPPED] == 1
    refused = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    src = [0, 1, 0, 1]
    assert env.adam_exploit_torch(opt, _dev(np.array(src, np.int32)), refused=refused) is refused
    after = _read(opt)
    assert _assert_exploit(before, after, src) == 0 == int(refused.item())
    for parts in after[:3]:
        assert all(x[2].tobytes() == x[0].tobytes() and x[3].tobytes() == x[1].tobytes() for x in parts)
    assert after[3][2, :4].tobytes() == after[3][0, :4].tobytes() and after[3][3, :4].tobytes() == after[3][1, :4].tobytes()
    # loser and winner with equal gradients and equal hyper: equal bits after the next step
    opt.hyper[2:].copy_(opt.hyper[:2])
    gs = [rng.standard_normal(tuple(t.shape)).astype(np.float32) for t in h.tensors]
    for g in gs:
        g[2:] = g[:2]
    t, ea, es, st = _step_and_compare(env, opt, _grads_dict(h, [_dev(g) for g in gs]), "after exploit")
    for parts in (t, ea, es):
        assert all(x[2].tobytes() == x[0].tobytes() and x[3].tobytes() == x[1].tobytes() and x[0].tobytes() != x[1].tobytes() for x in parts)
    assert st[2].tobytes() == st[0].tobytes() and st[3].tobytes() == st[1].tobytes()
    env.check_status()
    env.close()


def test_exploit_refuses_chains_and_sources_outside_the_population_also_when_captured():
    """5b: one captured exploit replayed with src rewritten: the chain, the swap and the out-of-range entries are not performed and are counted"""
    import torch
    env, rng, h, opt = _exploit_case()
    refused = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_src = torch.arange(4, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.adam_exploit_torch(opt, d_src, refused=refused)  # the identity
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        env.adam_exploit_torch(opt, d_src, refused=refused)
    for src, want_refused in (([0, 1, 2, 3], 0), ([2, 0, 2, 3], 1), ([-1, 4, 2 ** 31 - 1, 3], 3), ([1, 0, 2, 2], 2), ([3, 3, 3, 3], 0)):
        before = _read(opt)
        d_src.copy_(_dev(np.array(src, np.int32)))
        refused.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        after = _read(opt)
        assert _assert_exploit(before, after, src) == want_refused == int(refused.item()), src
        performed = am.exploit_sources(src)[0]
        changed = [m for m in range(4) if after[0][0][m].tobytes() != before[0][0][m].tobytes()]
        assert set(changed) <= {m for m in range(4) if performed[m] >= 0}, src  # (a source may already hold the destination's bits)
        if src == [2, 0, 2, 3]:
            assert changed == [0]
    env.adam_exploit_torch(opt, d_src)  # without the count
    env.check_status()
    env.close()


def test_native_refusals_write_nothing():
    """6: every refusal of the C calls, into NaN-prefilled state"""
    import torch
    from space_gym_amd import _native
    env, rng, pop, h, opt = _p3_case(GOAL, 33, 1, "relu", seed=26)
    grads = _p3_grads(rng, h, special=0)
    opt.state.fill_(float("nan"))
    before = _np(*h.tensors, *opt.exp_avg, *opt.exp_avg_sq)
    tab = env._adam_table(opt, _flat(h, grads))
    n = len(tab)
    src = torch.zeros(3, dtype=torch.int32, device="cuda")  # (every member would copy member 0)
    hy, st, sp = opt.hyper.data_ptr(), opt.state.data_ptr(), src.data_ptr()

    def edited(k, **fields):
        t = (_native.SgAdamTensor * n)()
        C.memmove(t, tab, C.sizeof(tab))
        for f, v in fields.items():
            setattr(t[k], f, v)
        return t

    step = lambda members, nt, t, hyper, state: env._lib.sg_adam_step_device(env._h, members, nt, t, hyper, state, None)
    exploit = lambda members, nt, t, state, s: env._lib.sg_adam_exploit_device(env._h, members, nt, t, state, s, None, None)
    cases = [("members", lambda: step(0, n, tab, hy, st)), ("members", lambda: step(65536, n, tab, hy, st)),
             ("n_tensors", lambda: step(3, 0, tab, hy, st)), ("n_tensors", lambda: step(3, 33, tab, hy, st)),
             ("null tensors", lambda: step(3, n, None, hy, st)),
             ("null pointer", lambda: step(3, n, edited(1, grad=None), hy, st)), ("null pointer", lambda: step(3, n, edited(n - 1, exp_avg_sq=None), hy, st)),
             ("null pointer", lambda: step(3, n, edited(0, param=None), hy, st)), ("null pointer", lambda: step(3, n, edited(2, exp_avg=None), hy, st)),
             ("numel", lambda: step(3, n, edited(1, numel=0), hy, st)), ("numel", lambda: step(3, n, edited(1, numel=-4), hy, st)),
             ("2^31 - 1", lambda: step(3, n, edited(0, numel=2 ** 30), hy, st)),
             ("null hyper", lambda: step(3, n, tab, None, st)), ("null state", lambda: step(3, n, tab, hy, None)),
             ("aligned", lambda: step(3, n, tab, hy, st + 4)),
             ("members", lambda: exploit(0, n, tab, st, sp)), ("n_tensors", lambda: exploit(3, 33, tab, st, sp)),
             ("null pointer", lambda: exploit(3, n, edited(0, exp_avg=None), st, sp)), ("2^31 - 1", lambda: exploit(3, n, edited(0, numel=2 ** 30), st, sp)),
             ("null state", lambda: exploit(3, n, tab, None, sp)), ("null src", lambda: exploit(3, n, tab, st, None)),
             ("aligned", lambda: exploit(3, n, tab, st + 4, sp))]
    for match, call in cases:
        assert call() == -1, match
        assert match in env._lib.sg_last_error(env._h).decode(), (match, env._lib.sg_last_error(env._h))
    assert exploit(3, n, edited(0, grad=None), st, sp) == 0  # (the exploit does not look at the gradients) ...
    torch.cuda.synchronize()
    after = _np(*h.tensors, *opt.exp_avg, *opt.exp_avg_sq)
    for k in range(len(h.tensors)):  # ... and copied member 0 over members 1 and 2: nothing else was written
        assert after[k][0].tobytes() == before[k][0].tobytes() and after[k][1].tobytes() == before[k][0].tobytes()
    st_np = _np(opt.state)[0]
    assert np.isnan(st_np).all()
    env.check_status()
    env.close()
