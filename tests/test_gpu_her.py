"""GPU tests of hindsight goal relabelling (replay_relabel_torch / replay_sample_her_torch / sg_replay_relabel_device) against the
NumPy model tests/her_model.py on rings filled by real rollouts: 200 envs, T = 16, four-step rollouts of random actions until the ring
has wrapped, episodes of at most 6 steps, started out of phase, so that truncations and terminal records fall inside the windows.
"Equal" is bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest

import her_model as hm
import replay_model

pytestmark = pytest.mark.gpu

B, T, K, ROLLOUTS = 200, 16, 4, 6
IDS = ("GoalContinuous3P-v0", "GoalContinuous4P-v0", "GoalDiscrete3-v0")
BATCH_KEYS = ("obs", "action", "reward", "next_obs", "terminated", "truncated", "discount", "steps", "index")
PROFILES = [dict(goal_vel_reward_scale=5.0, goal_sparse_reward=5.0), dict(goal_vel_reward_scale=2.0, goal_sparse_reward=11.0)]


def make(n, env_id, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _np(batch, keys=None):
    return {k: v.cpu().numpy() for k, v in batch.items() if keys is None or k in keys}


@functools.lru_cache(maxsize=None)
def _consts(env_id):
    from oracle import Oracle
    p = Oracle(env_id).params
    return dict(goal_scale=p.goal_vel_reward_scale * p.distance_fctr, sparse=p.goal_sparse_reward, goal_r2=p.goal_radius * p.goal_radius,
                two_over_world=np.float32(2.0 / p.world_size), half_world=np.float32(p.world_size / 2))


def _host_ring(env, ring):
    """the device ring as tests/replay_model.Ring: the members copied, the header's integers"""
    import torch
    torch.cuda.synchronize()
    m = replay_model.Ring(ring.steps, env.num_envs, env.obs_dim, ring.term_capacity, env.discrete)
    for k in ("obs", "action", "reward", "done", "trunc", "term_obs"):
        getattr(m, k)[...] = getattr(ring, k).cpu().numpy()
    m.term_idx[...] = ring.term_idx.cpu().numpy().view(np.uint32)
    h = ring.hdr.cpu().numpy().view(np.uint32)
    m.head, m.filled, m.term_head, m.sample_calls = int(h[4]), int(h[5]), int(h[6]), int(h[7])
    return m


def _filled(env_id, profiles=False, **kw):
    """(env, ring, prio): the ring wrapped by ROLLOUTS rollouts of K random steps, committed with priorities"""
    import torch
    env = make(B, env_id, seed=5, max_episode_steps=6, **kw)
    if profiles:
        env.set_reward_profiles(PROFILES)
        env.set_env_profiles(np.arange(B) % 2)
    ring = env.replay_torch(T, term_capacity=T * B)  # (a sixth of the steps end an episode: the default capacity is for 1 in 16)
    prio = env.replay_priority_torch(ring)
    env.reset_torch(out=ring.obs[T - 1])
    env.set_state(elapsed=np.arange(B) % 6)  # episodes out of phase: every slot holds ends of some envs and not of others
    env.replay_begin_torch(ring)
    env.replay_priority_begin_torch(prio)
    term = env.terminal_list_torch(K * B)
    for c in range(ROLLOUTS):
        rows = ring.rows(K)
        env.random_actions_torch(K, seed=3, first_step=c * K, out=rows["action"])
        env.rollout_torch(rows["action"], rows["obs"], rows["reward"], rows["done"], rows["trunc"], terminal=term)
        env.replay_commit_torch(ring, K, terminal=term, priority=prio)
    torch.cuda.synchronize()
    env.check_status()
    assert ring.filled == T and ROLLOUTS * K > T
    done, trunc = ring.done.cpu().numpy(), ring.trunc.cpu().numpy()
    ends = (done != 0).sum(1)
    assert (done != 0).mean() > 0.1 and (trunc != 0).any() and ends.min() >= B // 10 and ends.max() <= B // 2, ends
    return env, ring, prio


def _draw(env, ring, prio, n, seed):
    if prio is None:
        return env.replay_sample_torch(ring, n, seed=seed)
    return env.replay_sample_prioritized_torch(ring, prio, n, seed=seed, beta=0.5)


def _assert_relabel(env, ring, model, before, after, what, profile=None, reused=False, **kw):
    """`after` (the device's batch and optional outputs) against the model's relabel of `before`; returns the model's mask.
    reused: offset and goal are tensors an earlier call wrote into; they are written where relabelled only, so only there compared
    (freshly allocated ones are zero elsewhere, as the model's are)"""
    want, rel, off, goal, ok = hm.relabel(model, before, _consts(env.env_id), profile=profile, **kw)
    assert ok.all()
    for k in BATCH_KEYS:
        assert _same(after[k], want[k]), (what, k, int((_bits(after[k]) != _bits(want[k])).sum()))
    on = rel == 1 if reused else np.ones(rel.shape, bool)
    assert _same(after["relabelled"], rel) and _same(after["offset"][on], off[on]) and _same(after["goal"][on], goal[on]), what
    return rel, off


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
@pytest.mark.parametrize("env_id", IDS)
def test_relabelled_batches_equal_the_model_bit_for_bit(env_id, prioritized):
    """n = 1, 200, 2049; H = 1, 5, T - 1; her_ratio 0, 0.8, 1; future and final; uniform and prioritized batches: every column of the
    batch and the three optional outputs equal tests/her_model.py; the call leaves the ring's counter alone"""
    import torch
    env, ring, prio = _filled(env_id)
    model = _host_ring(env, ring)
    assert env.obs_dim == (17 if "4P" in env_id else 15)
    calls, seen = 0, dict(rel=0, kept=0, later=0, fin=0)
    for n in (1, 200, 2049):
        for H in (1, 5, T - 1):
            for ratio in (0.0, 0.8, 1.0):
                for name, code in (("future", hm.FUTURE), ("final", hm.FINAL)):
                    seed = 1000 * n + 10 * H + code
                    batch = _draw(env, ring, prio if prioritized else None, n, seed)
                    before = _np(batch)
                    calls += 1
                    got = env.replay_relabel_torch(ring, batch, her_ratio=ratio, horizon=H, strategy=name, seed=seed)
                    assert got is batch
                    model.sample_calls = calls  # the sampler's tick is in; the relabel reads the counter as it stands
                    rel, off = _assert_relabel(env, ring, model, before, _np(batch), (n, H, ratio, name), her_ratio=ratio, horizon=H,
                                               strategy=code, seed=seed)
                    if prioritized:
                        assert _same(batch["weight"].cpu().numpy(), before["weight"]) and _same(batch["cell"].cpu().numpy(), before["cell"])
                    assert (rel == 1).all() if ratio == 1.0 else not rel.any() if ratio == 0.0 else True
                    assert off.max() <= H - 1
                    seen["rel"] += int((rel == 1).sum()); seen["kept"] += int((rel == 0).sum()); seen["later"] += int((off > 0).sum())
                    q, i = before["index"] // B, before["index"] % B
                    p = ((model.head - model.valid) % T + q + off) % T
                    seen["fin"] += int(((rel == 1) & (model.done[p, i] != 0)).sum())  # the goal came from a terminal record
    assert min(seen["rel"], seen["kept"], seen["later"], seen["fin"]) > 100, seen
    assert int(ring.hdr.cpu().numpy().view(np.uint32)[7]) == calls
    env.check_status()
    env.close()


def test_the_her_sampler_is_the_sampler_followed_by_the_relabel():
    import torch
    env, ring, prio = _filled(IDS[0])
    n, kw = 777, dict(her_ratio=0.6, horizon=7, strategy="future", seed=42)
    for p in (None, prio):
        hdr = ring.hdr.clone()
        phdr = prio.hdr.clone()
        one = _np(env.replay_sample_her_torch(ring, n, prio=p, beta=0.5, **kw))
        ring.hdr.copy_(hdr)  # the same call numbers again
        prio.hdr.copy_(phdr)
        batch = _draw(env, ring, p, n, 42)
        two = _np(env.replay_relabel_torch(ring, batch, **kw))
        assert set(one) == set(two) and {"relabelled", "offset", "goal"} <= set(one)
        for k in one:
            assert _same(one[k], two[k]), k
        assert 0.5 < (one["relabelled"] == 1).mean() < 0.7
    env.check_status()
    env.close()


def test_rows_outside_the_ring_or_of_several_steps_are_left_untouched():
    import torch
    from space_gym_amd._native import NativeError
    env, ring, _ = _filled(IDS[0])
    model = _host_ring(env, ring)
    cells = len(ring)
    index = np.array([0, -1, cells, cells - 1, 17, 2 ** 40, 5, 6], np.int64)
    ok = (index >= 0) & (index < cells)
    batch = env.replay_sample_torch(ring, index.size, index=torch.from_numpy(np.where(ok, index, 0)).cuda())
    batch["index"].copy_(torch.from_numpy(index).cuda())
    batch["steps"][4] = 3
    before = _np(batch)
    out = dict(relabelled=torch.full((8,), 77, dtype=torch.uint8, device="cuda"), offset=torch.full((8,), 77, dtype=torch.int32, device="cuda"),
               goal=torch.full((8, 2), 77.0, device="cuda"))
    env.replay_relabel_torch(ring, batch, her_ratio=1.0, horizon=5, seed=9, out=out)
    torch.cuda.synchronize()
    model.sample_calls = 1
    want, rel, off, goal, mok = hm.relabel(model, before, _consts(env.env_id), her_ratio=1.0, horizon=5, seed=9)
    assert mok.tolist() == ok.tolist() and rel.tolist() == [1, 0, 0, 1, 2, 0, 1, 1]
    after = _np(batch)
    for k in BATCH_KEYS:
        assert _same(after[k], want[k]), k
    for j in (1, 2, 4, 5):
        assert all(_same(after[k][j], before[k][j]) for k in BATCH_KEYS)
    got = after["relabelled"]
    assert got[ok].tolist() == rel[ok].tolist() and (got[~ok] == 77).all()  # rows outside the ring: not even the flag is written
    live = rel == 1
    assert _same(after["offset"][live], off[live]) and _same(after["goal"][live], goal[live])
    assert (after["offset"][~live] == 77).all() and (after["goal"][~live] == 77.0).all()
    # status code 8: the next call fails, check_status reports and clears
    with pytest.raises(NativeError, match=r"\(-2\).*an earlier sg_replay_\*_device call refused"):
        env.replay_begin_torch(ring)
    with pytest.raises(NativeError, match=r"\(-1\)"):
        env.check_status()
    env.check_status()
    env.close()


def test_every_row_is_relabelled_under_its_envs_reward_profile():
    """two profiles with different goal_vel_reward_scale / goal_sparse_reward, alternating over the envs: the model with each env's
    coefficients is matched bit for bit, the handle's own coefficients would not be; swapping the indices afterwards swaps the result"""
    import torch
    env, ring, _ = _filled(IDS[0], profiles=True)
    model = _host_ring(env, ring)
    n, kw = 2049, dict(her_ratio=1.0, horizon=5, seed=3)
    tab = (np.array([p["goal_vel_reward_scale"] * 100.0 for p in PROFILES]), np.array([p["goal_sparse_reward"] for p in PROFILES]))
    for calls, idx in ((1, np.arange(B) % 2), (2, (np.arange(B) + 1) % 2)):
        env.set_env_profiles(idx)
        batch = env.replay_sample_torch(ring, n, seed=3)
        before = _np(batch)
        env.replay_relabel_torch(ring, batch, **kw)
        model.sample_calls = calls
        _assert_relabel(env, ring, model, before, _np(batch), ("profiles", calls), profile=(tab[0][idx], tab[1][idx]), **kw)
        plain, *_ = hm.relabel(model, before, _consts(env.env_id), **kw)
        odd = (before["index"] % B) % 2 == (1 if calls == 1 else 0)  # rows of profile 1
        assert not _same(_np(batch)["reward"][odd], plain["reward"][odd]) and odd.sum() > 500
    env.check_status()
    env.close()


def test_a_captured_sample_and_relabel_replays_with_fresh_masks():
    import torch
    env, ring, _ = _filled(IDS[0])
    model = _host_ring(env, ring)
    n, kw = 2049, dict(her_ratio=0.5, horizon=T - 1, strategy="future", seed=2 ** 40 + 7)
    out = env.replay_sample_her_torch(ring, n, **kw)  # (call 0: allocates the shapes)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.replay_sample_her_torch(ring, n, out=out, **kw)  # (call 1, warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.replay_sample_her_torch(ring, n, out=out, **kw)
    assert int(ring.hdr.cpu().numpy().view(np.uint32)[7]) == 2  # (capturing ran nothing)
    masks = []
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        model.sample_calls = 2 + rep
        before, ok = replay_model.sample(model, n, seed=kw["seed"])  # (advances the model's counter, as the device's tick does)
        assert ok.all() and model.sample_calls == 3 + rep
        got = _np(out)
        assert _same(got["index"], before["index"])
        rel, _ = _assert_relabel(env, ring, model, before, got, ("replay", rep), reused=True, her_ratio=0.5, horizon=T - 1,
                                 strategy=hm.FUTURE, seed=kw["seed"])
        masks.append(rel)
    assert not np.array_equal(masks[0], masks[1]) and int(ring.hdr.cpu().numpy().view(np.uint32)[7]) == 4
    env.check_status()
    env.close()


def test_a_relabelled_batch_feeds_the_td_updates():
    import torch
    from dqn_model import random_dqn
    from q_model import random_qnet
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rng = np.random.default_rng(4)
    env, ring, _ = _filled(IDS[0])
    batch = env.replay_sample_her_torch(ring, 512, her_ratio=0.8, seed=1)
    handles = [env.q_torch(critics=[[(dev(W), dev(b)) for W, b in net] for net in random_qnet(rng, env.obs_dim, 16, 1)]) for _ in range(2)]
    grads, stats = env.q_td_grad_torch(handles[0], handles[1], batch, torch.zeros((512, 2), device="cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and all(torch.isfinite(g).all() for net in grads["critics"] for pair in net for g in pair)
    env.check_status()
    env.close()
    env, ring, _ = _filled(IDS[2])
    batch = env.replay_sample_her_torch(ring, 512, her_ratio=0.8, strategy="final", seed=1)
    assert batch["action"].dtype == torch.int32
    handles = [env.dqn_torch(net=[(dev(W), dev(b)) for W, b in random_dqn(rng, env.obs_dim, 16, 1)]) for _ in range(2)]
    grads, stats = env.dqn_td_grad_torch(handles[0], handles[1], batch)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and all(torch.isfinite(g).all() for pair in grads["net"] for g in pair)
    env.check_status()
    env.close()


def _raw(env, ring, batch, out, n, ratio=0.8, horizon=5, strategy=0, struct_size=None):
    """sg_replay_relabel_device as a C caller reaches it: no Python check in front"""
    from space_gym_amd import _native
    r = env._replay_arg(ring)
    cfg = _native.SgReplayRelabelConfig(C.sizeof(_native.SgReplayRelabelConfig) if struct_size is None else struct_size, 0, ratio, horizon, strategy)
    b = _native.SgReplayBatch(**{k: batch[k].data_ptr() for k in BATCH_KEYS if batch.get(k) is not None})
    o = _native.SgReplayRelabelOut(*(out[k].data_ptr() for k in ("relabelled", "offset", "goal")))
    return env._lib.sg_replay_relabel_device(env._h, C.byref(r), C.byref(cfg), n, C.byref(b), C.byref(o), env._stream())


def test_native_refusals_enqueue_and_write_nothing():
    import torch
    from space_gym_amd._native import NativeError
    n = 64
    sentinel = lambda: dict(relabelled=torch.full((n,), 77, dtype=torch.uint8, device="cuda"),  # noqa: E731
                            offset=torch.full((n,), 77, dtype=torch.int32, device="cuda"), goal=torch.full((n, 2), 77.0, device="cuda"))

    def refused(env, ring, batch, match, **kw):
        batch = {k: v for k, v in batch.items() if v is not None}
        out, before = sentinel(), _np(batch)
        assert _raw(env, ring, batch, out, n, **kw) == -1 and match in env._lib.sg_last_error(env._h).decode()
        torch.cuda.synchronize()
        assert all(_same(v.cpu().numpy(), before[k]) for k, v in batch.items())
        assert (out["relabelled"] == 77).all() and (out["offset"] == 77).all() and (out["goal"] == 77.0).all()

    env, ring, _ = _filled(IDS[0])
    batch = env.replay_sample_torch(ring, n, seed=1)
    for kw, match in ((dict(ratio=-0.01), "her_ratio"), (dict(ratio=1.01), "her_ratio"), (dict(ratio=float("nan")), "her_ratio"),
                      (dict(horizon=0), "horizon"), (dict(horizon=T), "horizon"), (dict(strategy=2), "strategy"),
                      (dict(struct_size=28), "struct_size")):
        refused(env, ring, batch, match, **kw)
    for k in ("index", "steps", "obs", "next_obs", "reward"):
        refused(env, ring, {**batch, k: None}, "null batch")
    out = sentinel()
    assert _raw(env, ring, batch, out, 0) == 0  # n = 0: accepted, nothing enqueued
    torch.cuda.synchronize()
    assert (out["relabelled"] == 77).all()
    env.set_normalization(obs=True, reward=False)
    refused(env, ring, batch, "normalization")
    with pytest.raises(NativeError, match="normalization"):
        env.replay_relabel_torch(ring, batch)
    env.set_normalization(obs=False, reward=True)
    refused(env, ring, batch, "normalization")
    env.set_normalization(obs=False, reward=False)
    assert _raw(env, ring, batch, sentinel(), n) == 0
    env.check_status()
    env.close()
    # a Kepler id has no goal: refused by the library too
    kep = make(B, "KeplerCircleOrbit-v0")
    kring = kep.replay_torch(T, term_capacity=T * B)
    kep.reset_torch(out=kring.obs[T - 1])
    kep.replay_begin_torch(kring)
    rows = kring.rows(K)
    kep.random_actions_torch(K, seed=3, out=rows["action"])
    term = kep.terminal_list_torch(K * B)
    kep.rollout_torch(rows["action"], rows["obs"], rows["reward"], rows["done"], rows["trunc"], terminal=term)
    kep.replay_commit_torch(kring, K, terminal=term)
    kbatch = kep.replay_sample_torch(kring, n, seed=1)
    refused(kep, kring, kbatch, "no goal")
    with pytest.raises(ValueError, match="no goal"):
        kep.replay_relabel_torch(kring, kbatch)
    kep.check_status()
    kep.close()
