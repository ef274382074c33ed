"""GPU tests of the PBT calls (pbt_fitness_torch / pbt_fitness_update_torch / pbt_fitness_clear_torch / pbt_select_torch /
pbt_explore_torch) against tests/pbt_model.py: every table column, running return and length, source, rank and
stored hyperparameter bit for bit; the engine's own episode statistics as a second reference; one captured PBT generation replayed
twice; the native refusals."""
import math

import numpy as np
import pytest

import adam_model as am
import pbt_model as pm
from population_model import random_population
from test_gpu_adam import _read
from test_gpu_policy import GOAL, _dev, _np, make
from test_gpu_population import _pop_handle

pytestmark = pytest.mark.gpu


def _eq(got, want):
    """the same bits, a NaN standing for any NaN (its sign and payload are the processor's choice, not the contract's)"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(got)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(nan, np.isnan(want)) and got[~nan].tobytes() == want[~nan].tobytes()


def _rows(rng, K, B, nan_at=None):
    """done at 10 %, rewards over a wide exponent range (so that a wrong summation order shows)"""
    reward = (rng.standard_normal((K, B)) * 10.0 ** rng.integers(-6, 7, (K, B))).astype(np.float32)
    done = (rng.random((K, B)) < 0.1).astype(np.uint8)
    if nan_at is not None:
        reward[nan_at] = np.nan
    return reward, done


def _fit_np(fit):
    return _np(fit.table, fit.env_return, fit.env_length)


# ---------------------------------------------------------------------------------------------------------------- fitness
@pytest.mark.parametrize("B,P", [(192, 3), (1040, 2), (256, 256), (512, 1)])
def test_fitness_is_the_models_bits_over_two_calls_and_clear(B, P):
    """E = 64 (one ragged chunk), 520 (three chunks, the last with 8), 1 and 512; K = 1, 7, 20; two consecutive calls per K so that
    episodes span the boundary; one NaN reward, which changes only its member; clear with and without src"""
    import torch
    env = make(GOAL, B)
    rng = np.random.default_rng(B + P)
    for K in (1, 7, 20):
        fit = env.pbt_fitness_torch(P)
        assert fit.members == P and fit.workspace.numel() * 8 == pm.workspace_bytes(B, P)
        table, run, ln = _fit_np(fit)
        assert _eq(table, pm.fresh_table(P)) and not run.any() and not ln.any() and ln.dtype == np.int32
        for call in range(2):
            nan_at = (K // 2, B - 1) if call == 1 else None  # (an env of the last member)
            reward, done = _rows(rng, K, B, nan_at)
            if nan_at:
                done[K - 1, B - 1] = 1  # its episode finishes inside the rows
            d_done = _dev(done).view(torch.bool) if call else _dev(done)
            assert env.pbt_fitness_update_torch(fit, _dev(reward), d_done) is fit.table
            got = _fit_np(fit)
            want = pm.fitness_update(table, run, ln, reward, done)
            for g, w, what in zip(got, want, ("table", "env_return", "env_length")):
                assert _eq(g, w), (K, call, what, np.argwhere(g != w)[:4].tolist())
            if nan_at:
                without = np.where(np.isnan(reward), np.float32(0), reward)
                clean = pm.fitness_update(table, run, ln, without, done)[0]
                assert all(_eq(got[0][m], clean[m]) for m in range(P - 1)) and np.isnan(got[0][P - 1, pm.RETURN_SUM])
            table, run, ln = want
        assert table[:, pm.EPISODES].sum() > 0 or K == 1
        src = np.arange(P, dtype=np.int32)
        src[P // 2:] = 0  # (P = 1: the identity)
        env.pbt_fitness_clear_torch(fit, _dev(src))
        got = _fit_np(fit)
        assert _eq(got[0], pm.fitness_clear(table, src)) and _eq(got[1], run) and _eq(got[2], ln)
        if P > 1:
            assert _eq(got[0][0], table[0]) and _eq(got[0][P - 1], pm.fresh_table(1)[0])
        env.pbt_fitness_clear_torch(fit)
        got = _fit_np(fit)
        assert _eq(got[0], pm.fresh_table(P)) and _eq(got[1], run) and _eq(got[2], ln)
    env.check_status()
    env.close()


def _population_rollout(env, P, K, seed):
    import torch
    B, D = env.num_envs, env.obs_dim
    rng = np.random.default_rng(seed)
    pop = random_population(rng, P, D, 33, 1, 2, critic=True, continuous=True)
    h = _pop_handle(env, pop, "tanh")
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, 2), logp=z(K, B), value=z(K + 1, B), reward=z(K, B), done=z(K, B, dtype=torch.uint8),
             trunc=z(K, B, dtype=torch.uint8))
    b["obs"][0].copy_(env.reset_torch())
    return h, b


def test_fitness_of_real_population_rollout_rows():
    """rollout_population_torch on GoalContinuous3P-v0, 256 envs, P = 4, max_episode_steps = 5, K = 12, twice: episodes span the calls"""
    B, P, K = 256, 4, 12
    env = make(GOAL, B, seed=3, max_episode_steps=5)
    h, b = _population_rollout(env, P, K, seed=31)
    fit = env.pbt_fitness_torch(P)
    table, run, ln = _fit_np(fit)
    for call in range(2):
        if call:
            b["obs"][0].copy_(b["obs"][-1])
        env.rollout_population_torch(h, seed=3, first_step=call * K, **b)
        env.pbt_fitness_update_torch(fit, b["reward"], b["done"])
        reward, done = _np(b["reward"], b["done"])
        assert done.sum() >= 2 * B and (done[-1] == 0).any()
        want = pm.fitness_update(table, run, ln, reward, done)
        for g, w in zip(_fit_np(fit), want):
            assert _eq(g, w)
        table, run, ln = want
    assert (table[:, pm.EPISODES] >= 4 * 64).all() and np.isfinite(table[:, pm.FITNESS]).all()
    assert (table[:, pm.LENGTH_SUM] <= 2 * K * 64).all() and run.any()
    env.check_status()
    env.close()


def test_fitness_against_the_engines_own_episode_statistics():
    """the NumPy step() route with episode_statistics=True reports info["episode"]["r"]: with P = B and five rows every env's one
    finished episode gives return_sum[m] == r of env m bit for bit; with P = 4 and twelve rows episodes is exact and return_sum
    within 1e-12 relative of the sum of the reported returns"""
    B, K = 64, 12
    env = make(GOAL, B, seed=8, max_episode_steps=5, episode_statistics=True)
    env.reset()
    rng = np.random.default_rng(8)
    reward, done, rep = np.zeros((K, B), np.float32), np.zeros((K, B), np.uint8), []
    for t in range(K):
        _, rw, dn, info = env.step(rng.uniform(-1, 1, (B, 2)).astype(np.float32))
        reward[t], done[t] = rw, dn
        rep.append(np.array(info["episode"]["r"], np.float64))
    rep = np.stack(rep)
    assert np.array_equal(np.isnan(rep), done == 0) and done[4].mean() > 0.5
    each = env.pbt_fitness_torch(B)
    env.pbt_fitness_update_torch(each, _dev(reward[:5]), _dev(done[:5]))
    table = _np(each.table)[0]
    once = done[:5].sum(axis=0) == 1
    assert once.mean() > 0.5 and np.array_equal(table[:, pm.EPISODES], done[:5].sum(axis=0))
    r_once = np.nansum(np.where(once[None, :], rep[:5], np.nan), axis=0)  # (one term per env: exact)
    assert table[once, pm.RETURN_SUM].tobytes() == r_once[once].tobytes()
    assert table[once, pm.FITNESS].tobytes() == r_once[once].tobytes()
    four = env.pbt_fitness_torch(4)
    env.pbt_fitness_update_torch(four, _dev(reward), _dev(done))
    table = _np(four.table)[0]
    for m in range(4):
        blk = slice(m * 16, (m + 1) * 16)
        assert table[m, pm.EPISODES] == done[:, blk].sum()
        want = math.fsum(rep[:, blk][done[:, blk] != 0].tolist())
        assert abs(table[m, pm.RETURN_SUM] - want) <= 1e-12 * abs(want), (m, table[m, pm.RETURN_SUM], want)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- select
def _fitness_cases(P, rng):
    base = rng.standard_normal(P)
    ties = np.round(base * 2) / 2
    wild = base.copy()
    wild[rng.random(P) < 0.2] = np.inf
    wild[rng.random(P) < 0.2] = -np.inf
    wild[rng.random(P) < 0.2] = np.nan
    ready = (rng.random(P) < 0.7).astype(np.uint8)
    return [(base, None), (ties, None), (wild, None), (wild, ready), (ties, ready), (np.full(P, np.nan), None), (np.zeros(P), None)]


@pytest.mark.parametrize("P", [1, 2, 5, 7, 64, 256])
def test_select_gives_the_models_integers_and_exploit_refuses_nothing(P):
    """ties, +-inf, NaN, a ready mask, a strided fitness view, a seed with both words, both words of step, step_dev; the result
    goes into adam_exploit_torch with refused == 0"""
    import torch
    env = make(GOAL, 2 * P)
    rng = np.random.default_rng(300 + P)
    pop = random_population(rng, P, env.obs_dim, 8, 1, 2, critic=True, continuous=True)
    opt = env.adam_torch(_pop_handle(env, pop, "tanh"))
    refused = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    out, rank, count = (torch.full((n,), -9, dtype=torch.int32, device="cuda") for n in (P, P, 2))
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    table = torch.zeros((P, 8), dtype=torch.float64, device="cuda")
    seeds = [(0, 0, 0), (7, 3, 0), (7 + (5 << 32), 3 + (9 << 32), 0), (7, 2 ** 32 - 1, 1), (7, 3, 11), (2 ** 64 - 1, 2 ** 64 - 1, 2)]
    moved = 0
    for n, (f, ready) in enumerate(_fitness_cases(P, rng)):
        for fraction in (0.2, 0.5):
            seed, step, bump = seeds[(n + (fraction == 0.5)) % len(seeds)]
            k = pm.truncation_count(fraction, P)
            want_src, want_rank, want_count = pm.select(f, ready, k, seed, step, bump)
            step_dev.fill_(bump)
            table[:, 6].copy_(_dev(f))
            d_ready = None if ready is None else (_dev(ready).view(torch.bool) if n % 2 else _dev(ready))
            strided = (n + (fraction == 0.5)) % 2 == 0
            d_f = table[:, 6] if strided else _dev(f)
            got = env.pbt_select_torch(d_f, ready=d_ready, fraction=fraction, seed=seed, step=step, step_dev=step_dev if bump else None,
                                       out=out, rank=rank, count=count)
            assert got is out
            g_src, g_rank, g_count = _np(out, rank, count)
            assert g_src.dtype == np.int32 and np.array_equal(g_src, want_src), (P, n, fraction, g_src.tolist(), want_src.tolist())
            assert np.array_equal(g_rank, want_rank) and tuple(g_count.tolist()) == want_count
            env.adam_exploit_torch(opt, out, refused=refused)
            assert int(refused.item()) == 0
            moved += int((g_src != np.arange(P)).sum())
    fresh = env.pbt_select_torch(_dev(np.arange(P, dtype=np.float64)), fraction=0.5, seed=1)  # without the optional outputs
    assert np.array_equal(_np(fresh)[0], pm.select(np.arange(P, dtype=np.float64), None, P // 2, 1)[0])
    assert moved > 0 or P == 1
    env.check_status()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- explore
def _columns(P, rng):
    hyper = am.make_hyper(P, lr=(10.0 ** rng.uniform(-5, -2, P)).tolist(), betas=(rng.uniform(0.8, 0.95, P).tolist(), rng.uniform(0.98, 0.9999, P).tolist()),
                          eps=(10.0 ** rng.uniform(-8, -5, P)).tolist())
    coef = rng.random((P, 4)).astype(np.float32)
    disc = (0.9 + 0.1 * rng.random((P, 2))).astype(np.float32)
    specs = [(0, 0, dict(mode="scale", lo=1e-4, hi=5e-3)), (0, 1, dict(mode="scale_complement")), (0, 2, dict(mode="scale_complement", down=0.5, up=2.0, hi=0.9995)),
             (0, 3, dict(mode="copy")), (1, 2, dict(mode="scale", down=0.5, up=2.0)), (1, 0, dict(mode="copy", lo=0.25, hi=0.75)),
             (2, 0, dict(mode="scale_complement", lo=0.9, hi=0.9999)), (2, 1, dict(mode="copy"))]
    return [hyper, coef, disc], specs


def _model_columns(arrays, specs):
    return [pm.column(arrays[a], c, SpaceGymModes[s["mode"]], **{k: v for k, v in s.items() if k != "mode"}) for a, c, s in specs]


SpaceGymModes = dict(copy=pm.COPY, scale=pm.SCALE, scale_complement=pm.SCALE_COMPLEMENT)


@pytest.mark.parametrize("P", [6, 256])
def test_explore_stores_the_models_floats_and_counts_refused_copies(P):
    """three modes, the clamp, opt.hyper / coef / discounts in one call; untouched members against a clone; an out-of-range src and
    a chained src are counted and not applied"""
    import torch
    env = make(GOAL, 256)
    rng = np.random.default_rng(40 + P)
    arrays, specs = _columns(P, rng)
    f = rng.standard_normal(P)
    good = pm.select(f, None, P // 3, seed=2, step=1)[0]
    chained = good.copy()
    dest = np.flatnonzero(good != np.arange(P))
    chained[good[dest[0]]] = dest[1]          # a source that is itself a destination: dest[0]'s copy and its own are refused
    chained[np.flatnonzero(good == np.arange(P))[-1]] = P + 3  # out of range
    refused = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    step_dev = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    for src, seed, step, bump in ((good, 3, 4, 0), (chained, 3 + (1 << 32), 2 ** 32 - 2, 5), (np.arange(P, dtype=np.int32), 0, 0, 0)):
        dev = [_dev(a) for a in arrays]
        clones = [d.clone() for d in dev]
        want = [a.copy() for a in arrays]
        want_refused = pm.explore(src, _model_columns(want, specs), seed, step, bump)
        got_r = env.pbt_explore_torch(_dev(src.astype(np.int32)), [(dev[a], c, s) for a, c, s in specs], seed=seed, step=step,
                                      step_dev=step_dev if bump else None, refused=refused)
        assert got_r is refused and int(refused.item()) == want_refused
        performed = pm.exploit_sources(src)[0]
        for g, w, before in zip(_np(*dev), want, _np(*clones)):
            assert g.tobytes() == w.tobytes(), np.argwhere(g != w)[:4].tolist()
            assert g[performed < 0].tobytes() == before[performed < 0].tobytes()
        if src is good:
            assert want_refused == 0 and (performed >= 0).sum() == P // 3
            up = pm.explore_bits(P, len(specs), seed, step)[:, performed >= 0]
            assert up.any() and not up.all()
            assert any((w[performed >= 0] != b[performed >= 0]).any() for w, b in zip(want, arrays))
        if src is chained:
            assert want_refused >= 2
    env.pbt_explore_torch(_dev(good), [(_dev(arrays[0]), 0, dict(mode="copy"))])  # without the count
    env.check_status()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- one captured generation
def test_one_generation_in_a_single_graph_replayed_twice():
    """rollout_population_torch, fitness update, select, adam_exploit_torch, explore, clear and the bump of step_dev captured as ONE
    graph; both replays equal the model run on the rows the replay recorded, and the two replays draw differently"""
    import torch
    B, P, K = 256, 8, 12
    env = make(GOAL, B, seed=5, max_episode_steps=5)
    h, b = _population_rollout(env, P, K, seed=51)
    opt = env.adam_torch(h, lr=[1e-4 * (m + 1) for m in range(P)], betas=([0.9 - 0.01 * m for m in range(P)], [0.999] * P))
    arrays, specs = _columns(P, np.random.default_rng(52))
    coef, disc = _dev(arrays[1]), _dev(arrays[2])
    tensors = [opt.hyper, coef, disc]
    columns = [(tensors[a], c, s) for a, c, s in specs]
    fit = env.pbt_fitness_torch(P)
    src, rank, count = (torch.zeros(n, dtype=torch.int32, device="cuda") for n in (P, P, 2))
    refused = torch.zeros(2, dtype=torch.int32, device="cuda")
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")

    def generation():
        b["obs"][0].copy_(b["obs"][-1])
        env.rollout_population_torch(h, seed=3, **b)
        env.pbt_fitness_update_torch(fit, b["reward"], b["done"])
        env.pbt_select_torch(fit.fitness, fraction=0.25, seed=9, step=100, step_dev=step_dev, out=src, rank=rank, count=count)
        env.adam_exploit_torch(opt, src, refused=refused[:1])
        env.pbt_explore_torch(src, columns, seed=9, step=100, step_dev=step_dev, refused=refused[1:])
        env.pbt_fitness_clear_torch(fit, src)
        step_dev.add_(1)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        generation()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    before_capture = _np(fit.table, opt.hyper, step_dev)
    with torch.cuda.graph(graph, stream=side):
        generation()
    assert all(_eq(x, y) for x, y in zip(_np(fit.table, opt.hyper, step_dev), before_capture)), "a capture runs nothing"
    seen = []
    for replay in range(2):
        table, run, ln = _fit_np(fit)
        params = _read(opt)
        hy, cf, dc, sd = _np(opt.hyper, coef, disc, step_dev)
        assert int(sd[0]) == 1 + replay
        graph.replay()
        reward, done = _np(b["reward"], b["done"])
        w_table, w_run, w_ln = pm.fitness_update(table, run, ln, reward, done)
        w_src, w_rank, w_count = pm.select(w_table[:, pm.FITNESS], None, 2, seed=9, step=100, step_dev=int(sd[0]))
        assert w_count == (2, 2) and (w_src != np.arange(P)).sum() == 2
        g_src, g_rank, g_count, g_refused = _np(src, rank, count, refused)
        assert np.array_equal(g_src, w_src) and np.array_equal(g_rank, w_rank) and tuple(g_count.tolist()) == w_count
        assert g_refused.tolist() == [0, 0]
        wt, wea, wes, wst, _ = am.adam_exploit(*params[:4], w_src)
        after = _read(opt)
        for got, want in zip(after[:3], (wt, wea, wes)):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        assert after[3].tobytes() == wst.tobytes()
        want = [hy.copy(), cf.copy(), dc.copy()]
        assert pm.explore(w_src, _model_columns(want, specs), seed=9, step=100, step_dev=int(sd[0])) == 0
        for g, w in zip(_np(opt.hyper, coef, disc), want):
            assert g.tobytes() == w.tobytes()
        got = _fit_np(fit)
        assert _eq(got[0], pm.fitness_clear(w_table, w_src)) and _eq(got[1], w_run) and _eq(got[2], w_ln)
        seen.append((g_src.tolist(), pm.explore_bits(P, len(specs), 9, 100, int(sd[0])).tolist()))
    assert seen[0][1] != seen[1][1] and int(_np(step_dev)[0][0]) == 3
    # the same fitness and another step_dev: the winners are drawn afresh
    f = np.arange(P, dtype=np.float64)
    draws = {tuple(pm.select(f, None, 2, seed=9, step=100, step_dev=s)[0].tolist()) for s in range(8)}
    assert len(draws) > 1
    env.check_status()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- native refusals
def test_native_refusals_write_nothing():
    import torch
    from space_gym_amd import _native
    B, P, K = 192, 3, 4
    env = make(GOAL, B)
    lib, h = env._lib, env._h
    fit = env.pbt_fitness_torch(P)
    fit.table.fill_(float("nan"))
    reward, done = torch.ones((K, B), device="cuda"), torch.ones((K, B), dtype=torch.uint8, device="cuda")
    src = torch.zeros(P, dtype=torch.int32, device="cuda")
    out = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    hyper = torch.full((P, 8), 0.5, device="cuda")
    p = lambda t: t.data_ptr()
    ws, wsb = p(fit.workspace), fit.workspace.numel() * 8
    assert wsb == lib.sg_pbt_fitness_workspace_bytes(h, P) == P * 48

    def col(**fields):
        t = (_native.SgPbtColumn * 1)()
        t[0].data, t[0].stride, t[0].mode, t[0].down, t[0].up, t[0].lo, t[0].hi = p(hyper), 8, pm.SCALE, 0.8, 1.25, -np.inf, np.inf
        for f, v in fields.items():
            setattr(t[0], f, v)
        return t

    fitness = lambda members=P, k=K, r=p(reward), d=p(done), er=p(fit.env_return), el=p(fit.env_length), t=p(fit.table), w=ws, wb=wsb: \
        lib.sg_pbt_fitness_device(h, members, k, r, d, er, el, t, w, wb, None)
    clear = lambda members=P, t=p(fit.table): lib.sg_pbt_fitness_clear_device(h, members, t, None, None)
    select = lambda members=P, f=p(fit.table) + 48, stride=8, k=1, o=p(out): lib.sg_pbt_select_device(h, members, f, stride, None, k, 0, 0, None, o, None, None, None)
    explore = lambda members=P, s=p(src), n=1, c=None: lib.sg_pbt_explore_device(h, members, s, n, col() if c is None else c, 0, 0, None, None, None)
    nan = float("nan")
    cases = [("members", lambda: fitness(members=0)), ("members", lambda: fitness(members=257)), ("divide", lambda: fitness(members=5)),
             ("n_steps", lambda: fitness(k=0)), ("null", lambda: fitness(r=None)), ("null", lambda: fitness(d=None)), ("null", lambda: fitness(er=None)),
             ("null", lambda: fitness(el=None)), ("null", lambda: fitness(t=None)), ("aligned", lambda: fitness(t=p(fit.table) + 4)),
             ("workspace", lambda: fitness(w=None)), ("workspace", lambda: fitness(wb=wsb - 1)), ("aligned", lambda: fitness(w=ws + 4, wb=wsb + 8)),
             ("members", lambda: clear(members=0)), ("members", lambda: clear(members=257)), ("null table", lambda: clear(t=None)),
             ("aligned", lambda: clear(t=p(fit.table) + 4)),
             ("members", lambda: select(members=0)), ("members", lambda: select(members=257)), ("null", lambda: select(f=None)),
             ("null", lambda: select(o=None)), ("fitness_stride", lambda: select(stride=0)), ("k must be", lambda: select(k=2)),
             ("k must be", lambda: select(k=-1)), ("aligned", lambda: select(f=p(fit.table) + 4)),
             ("members", lambda: explore(members=0)), ("members", lambda: explore(members=257)), ("null", lambda: explore(s=None)),
             ("n_columns", lambda: explore(n=0)), ("n_columns", lambda: explore(n=17)), ("null data", lambda: explore(c=col(data=None))),
             ("stride", lambda: explore(c=col(stride=0))), ("mode", lambda: explore(c=col(mode=3))), ("mode", lambda: explore(c=col(mode=-1))),
             ("NaN", lambda: explore(c=col(down=nan))), ("NaN", lambda: explore(c=col(up=nan))), ("NaN", lambda: explore(c=col(lo=nan))),
             ("NaN", lambda: explore(c=col(hi=nan))), ("above", lambda: explore(c=col(lo=2.0, hi=1.0)))]
    for match, call in cases:
        assert call() == -1, match
        assert match in lib.sg_last_error(h).decode(), (match, lib.sg_last_error(h))
    assert lib.sg_pbt_explore_device(h, P, p(src), 1, None, 0, 0, None, None, None) == -1 and "null" in lib.sg_last_error(h).decode()
    assert lib.sg_pbt_fitness_workspace_bytes(h, 5) == 0 and "divide" in lib.sg_last_error(h).decode()
    assert lib.sg_pbt_fitness_workspace_bytes(h, 0) == 0 and "members" in lib.sg_last_error(h).decode()
    torch.cuda.synchronize()
    table, run, ln, o, hy = _np(fit.table, fit.env_return, fit.env_length, out, hyper)
    assert np.isnan(table).all() and not run.any() and not ln.any() and (o == -9).all() and (hy == 0.5).all()
    for fraction in (0.0, 0.6):
        with pytest.raises(ValueError, match="fraction"):
            env.pbt_select_torch(fit.fitness, fraction=fraction)
    with pytest.raises(ValueError, match="members"):
        env.pbt_fitness_torch(5)
    assert fitness() == 0 and select() == 0 and explore() == 0 and clear() == 0  # (and the accepted forms of the same calls)
    env.check_status()
    env.close()
