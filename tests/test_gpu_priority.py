"""GPU tests of prioritized replay sampling (replay_priority_torch / replay_commit_torch(priority=...) / replay_update_priorities_torch /
replay_priority_draw_torch / replay_sample_prioritized_torch) against the NumPy model tests/priority_model.py.  The integer state
(leaf, total, max_q, head, filled) and index, cell, leaf of every draw are compared bit for bit; weight within 1 unit in the last
place of float32: both sides round one float64 value to float32, and the only inexact step is one float64 pow.

The float64 value itself does not leave the device; every draw prints how far the float32 weight lies from the model's float64
value in float32 spacings (at most 0.5 when the two float64 values agree).  DESIGN.md section 16 records the largest seen."""
import numpy as np
import pytest

from priority_model import Priorities, numbers, quantise

pytestmark = pytest.mark.gpu


def make(n, env_id="GoalContinuous3P-v0", **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hdr(prio):
    h = prio.hdr.cpu().numpy().view(np.uint32)
    return dict(T=int(h[1]), B=int(h[2]), frac_bits=int(h[3]), head=int(h[4]), filled=int(h[5]), max_q=int(h[6]), sample_calls=int(h[7]),
                total=int(h[8]) | int(h[9]) << 32)


def _empty_list(env):
    import torch
    return dict(count=torch.zeros(1, dtype=torch.int32, device="cuda"), step_env=torch.zeros((4, 2), dtype=torch.int32, device="cuda"),
                obs=torch.zeros((4, env.obs_dim), device="cuda"))


def _state_equals(prio, m, what):
    import torch
    torch.cuda.synchronize()
    leaf = prio.leaf.cpu().numpy().view(np.uint32).reshape(-1)
    assert np.array_equal(leaf, m.q), (what, int((leaf != m.q).sum()))
    h = _hdr(prio)
    want = dict(T=m.T, B=m.B, frac_bits=m.frac_bits, head=m.head, filled=m.filled, max_q=m.max_q, sample_calls=m.sample_calls, total=m.total)
    assert h == want, (what, h, want)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _draw_equals(env, ring, prio, m, n, what, **kw):
    import torch
    got = env.replay_priority_draw_torch(ring, prio, n, **kw)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    want = m.sample(n, ring_head=ring.head, ring_filled=ring.filled, **kw)
    assert want is not None, what
    for k in ("index", "cell"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    assert np.array_equal(got["leaf"].view(np.uint32), want["leaf"]), what
    worst = int(_ulps(got["weight"], want["weight"]).max()) if n else 0
    # the float64 value behind the device's float32 is not returned; what can be seen of it: the distance of the float32 weight from
    # the model's float64 value in float32 spacings -- 0.5 at the most if the two float64 values were equal, and any excess over 0.5
    # bounds their discrepancy from below
    off = float((np.abs(got["weight"].astype(np.float64) - want["weight64"]) / np.spacing(np.abs(want["weight"])).astype(np.float64)).max()) if n else 0.0
    print(f"{what}: weight differs by at most {worst} ulp of float32; distance from the float64 value {off:.6f} float32 spacings")
    assert worst <= 1, (what, worst)
    return got


CASES = [("GoalContinuous3P-v0", 8, 1000, 16, 2), ("KeplerCircleOrbit-v0", 12, 70001, 16, 4), ("GoalDiscrete3-v0", 6, 77, 8, 2),
         ("GoalContinuous3P-v0", 4, 9, 0, 1), ("KeplerCircleOrbit-v0", 16, 4097, 31, 4)]


@pytest.mark.parametrize("env_id,T,B,frac_bits,K", CASES)
def test_commits_updates_and_draws_equal_the_model(env_id, T, B, frac_bits, K):
    """two and a half laps of commits of K slots (ring and priorities together), after each one an update of random cells with
    duplicates and with cells of the hole and of never-filled slots, then a stratified and an independent draw: after every call
    the integer state equals the model's bit for bit, and so do index, cell and leaf of the draws; weight within 1 ulp.
    T B is 8 000, 840 012, 462, 36 (one level) and 65 552 (one cell past 16 * 64^2): none a power of the fan-out, B never a
    multiple of 64; continuous and discrete ids"""
    import torch
    env = make(B, env_id)
    env.reset()
    rng = np.random.default_rng(T * B + frac_bits)
    ring = env.replay_torch(T)
    prio = env.replay_priority_torch(ring, frac_bits=frac_bits)
    assert tuple(prio.leaf.shape) == (T, B) and prio.frac_bits == frac_bits
    env.replay_begin_torch(ring)
    env.replay_priority_begin_torch(prio)
    m = Priorities(T, B, frac_bits)
    _state_equals(prio, m, "begin")
    tl = _empty_list(env)
    N = T * B
    for c in range(int(2.5 * T / K)):
        first, filled = ring.head, ring.filled
        env.replay_commit_torch(ring, K, terminal=tl, priority=prio)
        m.commit(first, filled, K)
        _state_equals(prio, m, ("commit", c))
        n_up = min(3000, max(8, N // 3))
        cell = rng.integers(0, N, n_up)
        cell[: n_up // 4] = cell[n_up // 4: 2 * (n_up // 4)]  # duplicates
        cell[-1] = np.flatnonzero(m.q)[-1]                      # (a tiny ring: at least one live cell is named)
        scale = 40000.0 if frac_bits <= 8 else 4.0
        pri = (rng.uniform(0, 1, n_up) ** 3 * scale).astype(np.float32)
        pri[rng.random(n_up) < 0.02] = 0.0
        stale = ~m.slot_valid(cell // B)
        assert stale.any() or T * B < 64
        env.replay_update_priorities_torch(prio, _dev(cell), priority=_dev(pri))
        on = m.update(cell, pri)
        assert on.sum() > 0 and not m.status
        _state_equals(prio, m, ("update", c))
        n = int(min(5000, m.total))
        _draw_equals(env, ring, prio, m, n, (env_id, T, B, "stratified", c), seed=7 + c, beta=0.4, stratified=True)
        _draw_equals(env, ring, prio, m, 5000, (env_id, T, B, "independent", c), seed=2 ** 40 + c, beta=1.0, stratified=False)
        one = _draw_equals(env, ring, prio, m, 333, (env_id, T, B, "beta 0", c), seed=3, beta=0.0, stratified=False)
        assert (one["weight"] == np.float32(1.0)).all()
    # td errors go through (|delta| + epsilon) ** alpha in torch, on the device (the exponent is inexact and stays out of the
    # integer state: the model is given the float32 priorities that expression yields there)
    cell = np.flatnonzero(m.q)[:50].astype(np.int64)
    td = rng.standard_normal(cell.size).astype(np.float32)
    env.replay_update_priorities_torch(prio, _dev(cell), td_error=_dev(td), alpha=0.6, epsilon=1e-6)
    m.update(cell, ((_dev(td).abs() + 1e-6) ** 0.6).cpu().numpy())
    _state_equals(prio, m, "td_error")
    env.check_status()
    env.close()


def test_the_headline_ring_draws_what_a_cumulative_sum_over_the_leaves_gives():
    """65 536 envs x 256 slots (16.7 M cells), full, 2^20 updated cells with duplicates: the leaves equal an amax scatter of the
    quantised priorities, total equals their int64 sum, and every drawn cell equals searchsorted over the int64 cumulative sum of
    the leaves on the device (exact) for numbers r computed by the model"""
    import torch
    B, T, K = 65536, 256, 64
    env = make(B)
    env.reset()
    ring = env.replay_torch(T, term_capacity=1024)
    prio = env.replay_priority_torch(ring)
    env.replay_begin_torch(ring)
    env.replay_priority_begin_torch(prio)
    tl = _empty_list(env)
    for c in range(5):
        env.replay_commit_torch(ring, K, terminal=tl, priority=prio)
    assert (ring.head, ring.filled) == (64, 256)
    rng = np.random.default_rng(1)
    n_up = 2 ** 20
    cell = rng.integers(0, T * B, n_up)
    cell[:1000] = cell[1000:2000]
    pri = (rng.uniform(0, 1, n_up) ** 4 * 8.0).astype(np.float32)
    env.replay_update_priorities_torch(prio, _dev(cell), priority=_dev(pri))
    torch.cuda.synchronize()
    env.check_status()
    q, ok = quantise(pri, 16)
    assert ok.all()
    want = torch.full((T * B,), 65536, dtype=torch.int64, device="cuda")
    want[64 * B:65 * B] = 0  # the hole
    c_dev, q_dev = _dev(cell), _dev(q.astype(np.int64))
    live = (c_dev // B) != 64
    new = torch.zeros_like(want).scatter_reduce(0, c_dev[live], q_dev[live], "amax", include_self=True)
    named = torch.zeros(T * B, dtype=torch.bool, device="cuda")
    named[c_dev[live]] = True
    want = torch.where(named, new, want)
    leaf = prio.leaf.reshape(-1).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(leaf, want)
    csum = torch.cumsum(leaf, 0)
    h = _hdr(prio)
    assert h["total"] == int(csum[-1]) and h["max_q"] == max(65536, int(q_dev[live].max())) and (h["head"], h["filled"]) == (64, 256)
    for call, (n, strat) in enumerate(((2 ** 20, True), (100_000, False))):
        got = env.replay_priority_draw_torch(ring, prio, n, seed=11, beta=0.5, stratified=strat)
        r = numbers(h["total"], call, n, 11, strat)
        assert int(r.max()) < 2 ** 63
        want_cell = torch.searchsorted(csum, _dev(r.astype(np.int64)), right=True)
        assert torch.equal(got["cell"], want_cell)
        p, i = want_cell // B, want_cell % B
        assert torch.equal(got["index"], ((p - 65) % T) * B + i)  # head - v = 64 - 255
        assert torch.equal(got["leaf"].to(torch.int64) & 0xFFFFFFFF, leaf[want_cell])
        w = ((255.0 * B) * leaf[want_cell].double() / float(h["total"])) ** -0.5
        assert int(_ulps(got["weight"].cpu().numpy(), w.float().cpu().numpy()).max()) <= 1
    env.check_status()
    env.close()


def test_rollouts_committed_with_priorities_sample_what_the_index_path_gathers():
    """6 rollouts of 20 steps into a ring of 60 slots with priority=prio; priorities updated from the drawn cells; the prioritized
    batch equals replay_sample_torch(index=batch['index']) in every output, cell names slot and env of the transition, and
    normalize=True divides the weights by their maximum"""
    import torch
    B, T, K = 512, 60, 20
    env = make(B, seed=5, max_episode_steps=30)
    ring = env.replay_torch(T)
    prio = env.replay_priority_torch(ring)
    env.reset_torch(out=ring.obs[T - 1])
    env.replay_begin_torch(ring)
    env.replay_priority_begin_torch(prio)
    term = env.terminal_list_torch(K * B)
    m = Priorities(T, B, 16)
    for c in range(6):
        rows = ring.rows(K)
        env.random_actions_torch(K, seed=3, first_step=c * K, out=rows["action"])
        env.rollout_torch(rows["action"], rows["obs"], rows["reward"], rows["done"], rows["trunc"], terminal=term)
        first, filled = ring.head, ring.filled
        env.replay_commit_torch(ring, K, terminal=term, priority=prio)
        m.commit(first, filled, K)
        batch = env.replay_sample_prioritized_torch(ring, prio, 4096, seed=c, beta=0.4, n_step=3, gamma=0.97, normalize=False)
        want = m.sample(4096, seed=c, beta=0.4, ring_head=ring.head, ring_filled=ring.filled)
        assert np.array_equal(batch["cell"].cpu().numpy(), want["cell"]) and np.array_equal(batch["index"].cpu().numpy(), want["index"])
        again = env.replay_sample_torch(ring, 4096, n_step=3, gamma=0.97, index=batch["index"])
        for k, v in again.items():
            assert torch.equal(batch[k].view(torch.uint8), v.view(torch.uint8)), k
        v = min(ring.filled, T - 1)
        p, i = batch["cell"] // B, batch["cell"] % B
        assert torch.equal(batch["obs"], ring.obs[(p - 1) % T, i]) and torch.equal(batch["action"], ring.action[p, i])
        assert torch.equal(batch["index"], ((p - (ring.head - v)) % T) * B + i)
        td = batch["reward"].abs()
        env.replay_update_priorities_torch(prio, batch["cell"], td_error=td, alpha=0.6)
        m.update(batch["cell"].cpu().numpy(), ((td + 1e-6) ** 0.6).cpu().numpy())
        _state_equals(prio, m, ("rollout", c))
    norm = env.replay_sample_prioritized_torch(ring, prio, 4096, seed=99, beta=0.4)
    raw = m.sample(4096, seed=99, beta=0.4)["weight"]
    assert float(norm["weight"].max()) == 1.0 and set(norm) == set(again) | {"cell", "weight"}
    assert np.array_equal(norm["weight"].cpu().numpy(), (torch.from_numpy(raw) / torch.from_numpy(raw).max()).numpy()) or \
        int(_ulps(norm["weight"].cpu().numpy(), raw / raw.max()).max()) <= 2  # (the raw weights may differ by 1 ulp; then the division)
    env.check_status()
    env.close()


def test_a_captured_draw_and_update_replays_with_fresh_draws_and_a_consistent_total():
    import torch
    T, B, n = 8, 1000, 2048
    env = make(B, "KeplerCircleOrbit-v0")
    env.reset()
    ring = env.replay_torch(T)
    prio = env.replay_priority_torch(ring)
    env.replay_begin_torch(ring)
    env.replay_priority_begin_torch(prio)
    m = Priorities(T, B, 16)
    tl = _empty_list(env)
    for c in range(5):
        first, filled = ring.head, ring.filled
        env.replay_commit_torch(ring, 2, terminal=tl, priority=prio)
        m.commit(first, filled, 2)
    pri_np = (np.random.default_rng(3).uniform(0, 1, n) ** 2 * 3).astype(np.float32)
    pri = _dev(pri_np)
    kw = dict(seed=2 ** 40 + 7, beta=0.6, stratified=True)
    out = env.replay_priority_draw_torch(ring, prio, n, **kw)  # (call 0: allocates the shapes)
    m.sample(n, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up on the capture stream)
        env.replay_priority_draw_torch(ring, prio, n, out=out, **kw)
        env.replay_update_priorities_torch(prio, out["cell"], priority=pri)
    torch.cuda.current_stream().wait_stream(side)
    m.update(m.sample(n, **kw)["cell"], pri_np)
    _state_equals(prio, m, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.replay_priority_draw_torch(ring, prio, n, out=out, **kw)
        env.replay_update_priorities_torch(prio, out["cell"], priority=pri)
    assert _hdr(prio)["sample_calls"] == 2 == m.sample_calls  # (capturing ran nothing)
    seen = []
    for rep in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want = m.sample(n, **kw)
        assert np.array_equal(out["cell"].cpu().numpy(), want["cell"]) and np.array_equal(out["index"].cpu().numpy(), want["index"]), rep
        assert int(_ulps(out["weight"].cpu().numpy(), want["weight"]).max()) <= 1
        m.update(want["cell"], pri_np)
        _state_equals(prio, m, ("replay", rep))
        assert _hdr(prio)["total"] == int(prio.leaf.to(torch.int64).bitwise_and(0xFFFFFFFF).sum())
        seen.append(want["cell"])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and _hdr(prio)["sample_calls"] == 5
    env.check_status()
    env.close()


def _expect_refusal(env, prio):
    """the status word is 9: the next call fails with SG_ERR_HIP, check_status raises with the priority message and clears it"""
    import torch
    from space_gym_amd._native import NativeError
    torch.cuda.synchronize()
    with pytest.raises(NativeError, match=r"\(-2\).*an earlier sg_priority_\*_device call refused"):
        env.replay_priority_commit_torch(prio, 0, 0, 1)
    with pytest.raises(NativeError, match=r"\(-1\).*sg_priority_\*_device: priorities without a matching header"):
        env.check_status()
    env.check_status()


def test_a_draw_from_a_total_of_zero_sets_code_9_and_writes_nothing():
    """ring and priorities begun, nothing committed: head and filled agree (0, 0) and total = 0.  The Python front end refuses an
    empty ring on the host, so the C entry point is called as a C caller would, with valid arguments"""
    import ctypes as C
    import torch
    from space_gym_amd import _native
    env = make(9)
    env.reset()
    ring = env.replay_torch(4)
    prio = env.replay_priority_torch(ring)
    env.replay_begin_torch(ring)
    env.replay_priority_begin_torch(prio)
    torch.cuda.synchronize()
    assert _hdr(prio)["total"] == 0 and len(ring) == 0
    out = dict(index=torch.full((10,), 77, dtype=torch.int64, device="cuda"), cell=torch.full((10,), 77, dtype=torch.int64, device="cuda"),
               weight=torch.full((10,), 77.0, device="cuda"), leaf=torch.full((10,), 77, dtype=torch.int32, device="cuda"))
    before = {k: getattr(prio, k).clone() for k in prio.MEMBERS}
    r, p = env._replay_arg(ring), env._priority_arg(prio, ring)
    for strat in (0, 1):
        cfg = _native.SgPrioritySampleConfig(C.sizeof(_native.SgPrioritySampleConfig), 0, 0.4, strat)
        draw = _native.SgPriorityDraw(*(out[k].data_ptr() for k in ("index", "cell", "weight", "leaf")))
        assert env._lib.sg_priority_sample_device(env._h, C.byref(r), C.byref(p), C.byref(cfg), 10, C.byref(draw), env._stream()) == 0
        _expect_refusal(env, prio)
        for k, v in out.items():
            assert (v == 77).all(), k
    h0, h1 = before["hdr"].clone(), prio.hdr.clone()
    assert int(h1[7]) == 2
    h0[7] = h1[7] = 0  # (sample_calls moves on)
    assert torch.equal(prio.leaf, before["leaf"]) and torch.equal(prio.node, before["node"]) and torch.equal(h0, h1)
    m = Priorities(4, 9)
    assert m.sample(10, stratified=False) is None and m.status
    env.check_status()
    env.close()


@pytest.mark.parametrize("what", ["lag", "strata", "no header", "bad rows"])
def test_device_refusals_set_code_9_write_nothing_and_clear(what):
    import torch
    T, B = 4, 9
    env = make(B)
    env.reset()
    ring = env.replay_torch(T)
    prio = env.replay_priority_torch(ring, frac_bits=0)
    env.replay_begin_torch(ring)
    tl = _empty_list(env)
    m = Priorities(T, B, 0)
    if what != "no header":
        env.replay_priority_begin_torch(prio)
        env.replay_commit_torch(ring, 1, terminal=tl, priority=prio)
        m.commit(0, 0, 1)
    else:
        env.replay_commit_torch(ring, 1, terminal=tl)
    out = dict(index=torch.full((10,), 77, dtype=torch.int64, device="cuda"), cell=torch.full((10,), 77, dtype=torch.int64, device="cuda"),
               weight=torch.full((10,), 77.0, device="cuda"), leaf=torch.full((10,), 77, dtype=torch.int32, device="cuda"))
    before = {k: v.clone() for k, v in (("leaf", prio.leaf), ("node", prio.node), ("hdr", prio.hdr))}
    if what == "lag":  # a commit of the ring without its priorities
        env.replay_commit_torch(ring, 1, terminal=tl)
        env.replay_priority_draw_torch(ring, prio, 10, stratified=False, out=out)
        assert m.sample(10, stratified=False, ring_head=ring.head, ring_filled=ring.filled) is None
    elif what == "strata":  # total = 9 units, 10 strata; 10 independent draws are fine
        assert _hdr(prio)["total"] == 9 == m.total
        env.replay_priority_draw_torch(ring, prio, 10, stratified=True, out=out)
        assert m.sample(10, stratified=True) is None
    elif what == "no header":
        env.replay_priority_draw_torch(ring, prio, 10, out=out)
    else:
        cell = np.array([0, -1, 36, 1, 2, 3, 4], np.int64)
        pri = np.array([5.0, 1.0, 1.0, np.nan, -1.0, np.inf, 2.0], np.float32)
        env.replay_update_priorities_torch(prio, _dev(cell), priority=_dev(pri))
        on = m.update(cell, pri)
        assert on.tolist() == [True, False, False, False, False, False, True] and m.status
        _state_equals(prio, m, what)
        assert m.q[:5].tolist() == [5, 1, 1, 1, 2] and m.total == 14 and m.max_q == 5
    _expect_refusal(env, prio)
    if what != "bad rows":
        for k, v in out.items():
            assert (v == 77).all(), k
        h0, h1 = before["hdr"].clone(), prio.hdr.clone()
        h0[7] = h1[7] = 0  # (sample_calls moves on)
        assert torch.equal(prio.leaf, before["leaf"]) and torch.equal(prio.node, before["node"]) and torch.equal(h0, h1)
    if what == "strata":
        m.status = False
        _draw_equals(env, ring, prio, m, 10, what, stratified=False)
        _draw_equals(env, ring, prio, m, 9, what, stratified=True)
    env.check_status()
    env.close()
