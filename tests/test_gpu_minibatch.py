"""GPU tests of the minibatch index call and the one-call PPO update (sg_minibatch_index_device, minibatch_index_torch /
ppo_update_torch), everything bit for bit: the index against tests/minibatch_model.py over both units, seeds and
steps with both words set and a step_dev that carries; ppo_update_torch against the hand-written loop of the calls it is made of;
one captured graph of rollout, GAE, update and the bump of step_dev whose replays shuffle afresh; the native refusals."""
import numpy as np
import pytest

import minibatch_model as mm
from policy_model import random_policy
from population_model import random_population
from test_gpu_policy import GOAL, _dev, _handle, _np, make
from test_gpu_population import _pop_handle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1), (3, 5, 1, 2, 2), (4, 192, 3, 4, 2), (7, 1040, 2, 3, 3), (17, 241, 1, 5, 1), (1, 256, 256, 1, 64)]  # (K, B, P, M, epochs)
KEYS = [(0x123456789, 2 ** 32 + 5, None), (2 ** 63 + 11, 2 ** 64 - 3, 5), (7, 2 ** 32 - 1, 1), (3, 2 ** 40, -(2 ** 40) + 2)]  # (seed, step, step_dev)
GUARD = -7


def _guarded(shape):
    """an int64 tensor of `shape` inside a buffer with a guard word on either side"""
    import torch
    buf = torch.full((int(np.prod(shape)) + 2,), GUARD, dtype=torch.int64, device="cuda")
    return buf, buf[1:-1].view(shape)


@pytest.mark.parametrize("K,B,P,M,epochs", SHAPES)
def test_the_index_is_the_models_bits(K, B, P, M, epochs):
    import torch
    env = make(GOAL, B)
    ran = 0
    for unit, name in ((mm.ROW, "row"), (mm.ENV, "env")):
        n = mm.size(K, B, P, M, unit)
        assert env._lib.sg_minibatch_size(env._h, K, P, M, unit) == n
        if n < 1:
            with pytest.raises(ValueError, match="minibatches"):
                env.minibatch_index_torch(K, members=P, epochs=epochs, minibatches=M, unit=name)
            continue
        for seed, step, dev in KEYS:
            step_dev = None if dev is None else torch.tensor([dev], dtype=torch.int64, device="cuda")
            buf, out = _guarded((epochs, M, P, n))
            got = env.minibatch_index_torch(K, members=P, epochs=epochs, minibatches=M, unit=name, seed=seed, step=step, step_dev=step_dev, out=out)
            assert got is out  # out= is filled in place
            g, whole = _np(got, buf)
            want = mm.index(K, B, P, epochs, M, unit, seed, step, 0 if dev is None else dev)
            assert g.shape == want.shape == (epochs, M, P, n) and np.array_equal(g, want), (name, seed, step, dev)
            assert whole[0] == GUARD and whole[-1] == GUARD
            ran += 1
        # a fresh tensor; members None is P = 1 without the member axis; the unit by its number
        seed, step, _ = KEYS[0]
        fresh = env.minibatch_index_torch(K, members=P, epochs=epochs, minibatches=M, unit=unit, seed=seed, step=step)
        assert fresh.dtype == torch.int64 and fresh.is_contiguous() and np.array_equal(_np(fresh)[0], mm.index(K, B, P, epochs, M, unit, seed, step))
        if P == 1:
            flat = env.minibatch_index_torch(K, epochs=epochs, minibatches=M, unit=name, seed=seed, step=step)
            assert tuple(flat.shape) == (epochs, M, n) and np.array_equal(_np(flat)[0], _np(fresh)[0][:, :, 0])
    assert ran >= len(KEYS)
    env.check_status()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- ppo_update_torch
B, K, D_HIDDEN = 256, 8, 33


def _rollout_batch(env, h, population, seed):
    """K closed-loop steps and their GAE targets: (the rollout buffers, the flattened batch, (terminal_value, advantage, returns))"""
    import torch
    D = env.obs_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, 2), logp=z(K, B), value=z(K + 1, B), reward=z(K, B), done=z(K, B, dtype=torch.uint8),
             trunc=z(K, B, dtype=torch.uint8))
    tv, adv, ret = z(K, B), z(K, B), z(K, B)
    b["obs"][0].copy_(env.reset_torch())
    if population:
        env.rollout_population_torch(h, seed=seed, terminal_value=tv, **b)
        env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1], terminal_value=tv, out=dict(advantage=adv, returns=ret))
    else:
        env.rollout_policy_torch(h, seed=seed, **b)
        env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1], out=dict(advantage=adv, returns=ret))
    batch = dict(obs=b["obs"][:-1].reshape(K * B, D), action=b["action"].reshape(K * B, 2), logp=b["logp"].reshape(K * B),
                 value=b["value"][:-1].reshape(K * B), advantage=adv.reshape(K * B), ret=ret.reshape(K * B))
    return b, batch, (tv, adv, ret)


def _live(h, opt):
    return (*h.tensors, *opt.exp_avg, *opt.exp_avg_sq, opt.state)


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["single", "population-row", "population-env"])
def test_ppo_update_torch_is_the_hand_written_loop(case):
    import torch
    population = case != "single"
    unit = "env" if case.endswith("env") else "row"
    P, epochs, M = (4, 2, 2) if population else (None, 2, 4)
    env = make(GOAL, B, seed=5, max_episode_steps=5)
    rng = np.random.default_rng(30)
    if population:
        h = _pop_handle(env, random_population(rng, P, env.obs_dim, D_HIDDEN, 1, 2, critic=True, continuous=True), "tanh")
        opt = env.adam_torch(h, lr=[1e-3 * (m + 1) for m in range(P)], max_grad_norm=[0.5, None, 1.0, 0.25])
        coef = _dev(np.array([[0.2, 0.2, 0.01, 0.5], [0.1, 0.0, 0.0, 1.0], [0.3, 0.15, 0.03, 0.25], [0.25, 0.1, 0.02, 0.75]], np.float32))
        kw = dict(coef=coef)
    else:
        h = _handle(env, random_policy(rng, env.obs_dim, D_HIDDEN, 1, 2, critic=True, continuous=True), "tanh")
        opt = env.adam_torch(h, lr=2e-3, max_grad_norm=0.5)
        kw = dict(clip_range=0.15, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.25)
    _, batch, _ = _rollout_batch(env, h, population, seed=3)
    saved = [x.clone() for x in _live(h, opt)]
    seed, step = 2 ** 40 + 9, 2 ** 33 + 1
    step_dev = torch.tensor([4], dtype=torch.int64, device="cuda")
    # the loop, written out
    idx = env.minibatch_index_torch(K, members=P, epochs=epochs, minibatches=M, unit=unit, seed=seed, step=step, step_dev=step_dev)
    assert np.array_equal(_np(idx)[0].reshape(epochs, M, P or 1, -1), mm.index(K, B, P or 1, epochs, M, mm.ENV if unit == "env" else mm.ROW, seed, step, 4))
    want_stats = []
    for e in range(epochs):
        for b in range(M):
            if population:
                grads, st = env.population_ppo_grad_torch(h, batch, idx[e, b], **kw)
            else:
                grads, st = env.ppo_grad_torch(h, batch, idx[e, b], **kw)
            env.adam_step_torch(opt, grads)
            want_stats.append(_np(st)[0])
    want = _np(*_live(h, opt))
    assert not _same(want, _np(*saved)) and all(np.isfinite(x).all() for x in want)
    assert np.array_equal(want[-1][:, 0], [epochs * M] * (P or 1))  # every member stepped epochs x M times
    for x, s in zip(_live(h, opt), saved):
        x.copy_(s)
    # the one call
    stats, index = env.ppo_update_torch(h, opt, batch, K, epochs, M, unit=unit, seed=seed, step=step, step_dev=step_dev, **kw)
    assert tuple(stats.shape) == ((epochs, M, P, 12) if population else (epochs, M, 12)) and index.shape == idx.shape
    assert _np(index)[0].tobytes() == _np(idx)[0].tobytes()
    assert _np(stats)[0].tobytes() == np.stack(want_stats).reshape(stats.shape).tobytes()
    assert _same(_np(*_live(h, opt)), want)
    # into the caller's tensors, from the same start: the same bits again
    for x, s in zip(_live(h, opt), saved):
        x.copy_(s)
    mine = (torch.zeros_like(stats), torch.zeros_like(index))
    got = env.ppo_update_torch(h, opt, batch, K, epochs, M, unit=unit, seed=seed, step=step, step_dev=step_dev, stats=mine[0], index=mine[1],
                               grads=grads, **kw)
    assert got[0] is mine[0] and got[1] is mine[1] and _same(_np(*mine), _np(stats, index)) and _same(_np(*_live(h, opt)), want)
    env.check_status()
    env.close()


def test_one_ppo_iteration_with_its_shuffle_in_a_single_graph():
    """rollout_population_torch, gae_torch, ppo_update_torch and the bump of step_dev captured as ONE graph and replayed twice: after
    each replay the index is the model's at step + replay number, the two differ, and the parameters are those of an eager run of
    the same two iterations"""
    import torch
    P, epochs, M, seed, step = 4, 2, 2, 7, 2 ** 32 - 1
    env = make(GOAL, B, seed=5, max_episode_steps=5)
    rng = np.random.default_rng(31)
    h = _pop_handle(env, random_population(rng, P, env.obs_dim, D_HIDDEN, 1, 2, critic=True, continuous=True), "tanh")
    opt = env.adam_torch(h, lr=[1e-3, 2e-3, 3e-3, 4e-3], max_grad_norm=0.5)
    b, batch, (tv, adv, ret) = _rollout_batch(env, h, True, seed=3)
    n = mm.size(K, B, P, M, mm.ROW)
    index = torch.zeros((epochs, M, P, n), dtype=torch.int64, device="cuda")
    stats = torch.zeros((epochs, M, P, 12), device="cuda")
    grads, _ = env.population_ppo_grad_torch(h, batch, index[0, 0])  # (the gradient tensors and the workspace, before any capture)
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")

    def iteration():
        b["obs"][0].copy_(b["obs"][-1])
        env.rollout_population_torch(h, seed=3, terminal_value=tv, **b)
        env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1], terminal_value=tv, out=dict(advantage=adv, returns=ret))
        env.ppo_update_torch(h, opt, batch, K, epochs, M, seed=seed, step=step, step_dev=step_dev, ent_coef=0.01, index=index, stats=stats, grads=grads)
        step_dev.add_(1)

    live = (*_live(h, opt), b["obs"], step_dev)
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
        eager.append(_np(*_live(h, opt), index))
    assert not _same(eager[0], eager[1]) and all(np.isfinite(x).all() for x in eager[1][:-1])
    rewind()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        iteration()
    assert _same(_np(*live), _np(*saved)), "a capture runs nothing"
    seen = []
    for replay in range(2):
        graph.replay()
        got = _np(*_live(h, opt), index)
        assert np.array_equal(got[-1], mm.index(K, B, P, epochs, M, mm.ROW, seed, step + replay))  # (the second step carries into the high word)
        assert _same(got, eager[replay])
        seen.append(got[-1])
    assert not np.array_equal(seen[0], seen[1]) and int(_np(step_dev)[0][0]) == 2
    env.check_status()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- native refusals
def test_native_refusals_write_nothing():
    import torch
    Bn, Kn, P = 192, 4, 3
    env = make(GOAL, Bn)
    lib, h = env._lib, env._h
    out = torch.full((2 * 4 * P * 64,), GUARD, dtype=torch.int64, device="cuda")  # (room for every call below, were it not refused)
    p = out.data_ptr()
    call = lambda steps=Kn, members=P, epochs=2, minibatches=4, unit=mm.ROW, o=p: lib.sg_minibatch_index_device(
        h, steps, members, epochs, minibatches, unit, 1, 2, None, o, None)
    cases = [("steps", dict(steps=0)), ("steps", dict(steps=-1)), ("members", dict(members=0)), ("members", dict(members=257)),
             ("divide", dict(members=5)), ("epochs", dict(epochs=0)), ("epochs", dict(epochs=65)), ("minibatches", dict(minibatches=0)),
             ("minibatches", dict(minibatches=-2)), ("leave none", dict(minibatches=Kn * 64 + 1)), ("leave none", dict(minibatches=65, unit=mm.ENV)),
             ("2^31", dict(steps=2 ** 31 // Bn + 1)), ("unit", dict(unit=2)), ("unit", dict(unit=-1)), ("null", dict(o=None)),
             ("aligned", dict(o=p + 4))]
    for match, kw in cases:
        assert call(**kw) == -1, (match, kw)
        assert match in lib.sg_last_error(h).decode(), (match, lib.sg_last_error(h))
    for kw in (dict(steps=0), dict(members=0), dict(members=257), dict(members=5), dict(minibatches=0), dict(minibatches=Kn * 64 + 1),
               dict(minibatches=65, unit=mm.ENV), dict(steps=2 ** 31 // Bn + 1), dict(unit=2)):
        args = dict(dict(steps=Kn, members=P, minibatches=4, unit=mm.ROW), **kw)
        assert lib.sg_minibatch_size(h, args["steps"], args["members"], args["minibatches"], args["unit"]) == -1, kw
        assert mm.size(args["steps"], Bn, args["members"], args["minibatches"], args["unit"]) == -1, kw
    assert lib.sg_minibatch_size(h, 2 ** 31 // Bn, 1, 1, mm.ROW) == (2 ** 31 // Bn) * Bn  # the largest rollout: K B = 2^31 - 128
    torch.cuda.synchronize()
    assert (_np(out)[0] == GUARD).all()
    assert call() == 0 and call(minibatches=64, unit=mm.ENV) == 0  # the same calls, not refused
    assert (_np(out)[0][:2 * 4 * P * 64] != GUARD).all()
    env.check_status()
    env.close()
