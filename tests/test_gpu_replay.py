"""GPU tests of the replay ring (replay_torch / replay_begin_torch / replay_commit_torch / replay_sample_torch) against the NumPy model
tests/replay_model.py.  "Equal" is bitwise: the same bit patterns in every output."""
import numpy as np
import pytest

from replay_model import sample, synthetic

pytestmark = pytest.mark.gpu

KEYS = ("obs", "action", "reward", "next_obs", "terminated", "truncated", "discount", "steps", "index")


def make(n, env_id="GoalContinuous3P-v0", **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _apply(env, ring, com):
    """what a caller does with one commit of tests/replay_model.synthetic: rows into the slots at the head, then the commit"""
    rows = ring.rows(com["K"])
    for k, v in com["rows"].items():
        rows[k].copy_(_dev(v))
    if "terminal_obs" in com:
        env.replay_commit_torch(ring, 1, terminal_obs=_dev(com["terminal_obs"]))
    else:
        term = dict(count=_dev(np.array([com["count"]], np.int32)), step_env=_dev(com["step_env"]), obs=_dev(com["tobs"]))
        env.replay_commit_torch(ring, com["K"], terminal=term)


def _header(ring):
    h = ring.hdr.cpu().numpy().view(np.uint32)
    return dict(T=int(h[1]), B=int(h[2]), D=int(h[3]), head=int(h[4]), filled=int(h[5]), term_head=int(h[6]), sample_calls=int(h[7]))


def _sample(env, ring, n, **kw):
    import torch
    out = env.replay_sample_torch(ring, n, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_batch(got, want, what):
    for k in KEYS:
        assert _same(got[k], want[k]), (what, k, int((_bits(got[k]) != _bits(want[k])).sum()))


CASES = [("GoalContinuous3P-v0", 8, 70001, False), ("GoalContinuous3P-v0", 64, 1000, True), ("GoalContinuous4P-v0", 8, 1000, False),
         ("KeplerCircleOrbit-v0", 64, 1000, False), ("KeplerCircleOrbit-v0", 8, 1000, True), ("GoalDiscrete3-v0", 8, 1000, False),
         ("GoalDiscrete3-v0", 8, 70001, True)]


@pytest.mark.parametrize("env_id,T,B,dense", CASES)
def test_synthetic_rings_sample_what_the_model_samples(env_id, T, B, dense):
    """commits in the list form (K = T / 4 slots each) or the dense form (one slot each), two and a half laps; then random draws
    and index= over every valid transition, n_step 1, 3 and 16: every output equals the model bit for bit"""
    import torch
    env = make(B, env_id)
    env.reset()
    state0 = env.get_state()
    D = env.obs_dim
    model, commits, extra = synthetic(T, B, D, laps=2.5, p_done=0.05, seed=T + B, discrete=env.discrete, dense=dense)
    assert not model.status and model.filled == T and model.done.any() and (model.done & model.trunc).any()
    ring = env.replay_torch(T)
    assert ring.term_capacity == model.C == max(2 * B, T * B // 16)
    env.replay_begin_torch(ring, _dev(extra["obs0"]))
    for com in commits:
        _apply(env, ring, com)
    torch.cuda.synchronize()
    env.check_status()
    assert (ring.head, ring.filled, len(ring)) == (model.head, model.filled, len(model)) and len(ring) == (T - 1) * B
    assert _header(ring) == dict(T=T, B=B, D=D, head=model.head, filled=T, term_head=model.term_head, sample_calls=0)
    assert np.array_equal(ring.slot_seq.cpu().numpy().view(np.uint32), model.slot_seq)
    if not dense:  # (the dense form's order of sequence numbers is free: its samples are compared instead)
        d = model.done != 0
        assert np.array_equal(ring.term_idx.cpu().numpy().view(np.uint32)[d], model.term_idx[d])
    every = np.arange(len(model), dtype=np.int64)
    every_dev = _dev(every)
    for n_step in (1, 3, 16):
        want, ok = sample(model, 5000, seed=99, n_step=n_step, gamma=0.97)
        assert ok.all()
        _assert_batch(_sample(env, ring, 5000, seed=99, n_step=n_step, gamma=0.97), want, ("random", n_step))
        want, ok = sample(model, every.size, n_step=n_step, gamma=0.97, index=every)
        assert ok.all() and (n_step == 1 or (want["steps"] > 1).any())
        got = _sample(env, ring, every.size, n_step=n_step, gamma=0.97, index=every_dev)
        _assert_batch(got, want, ("every", n_step))
        if n_step == 1:  # the stored transition: s' of a finished step is the terminal observation, not obs[p]
            q, i = every // B, every % B
            p = (model.head - model.valid + q) % T
            fin = model.done[p, i] != 0
            assert fin.any() and _same(got["next_obs"][fin], extra["term_dense"][p, i][fin])
            assert _same(got["reward"], model.reward[p, i]) and (got["discount"] == np.float32(0.97)).all()
    assert _header(ring)["sample_calls"] == 6 == model.sample_calls
    env.check_status()
    for a, b in zip(state0, env.get_state()):  # nothing of the env moved
        assert a is b is None or np.array_equal(a, b)
    env.close()


def test_rollouts_written_into_the_ring_give_the_transitions_a_stepped_env_saw():
    """reset, begin, 6 rollouts of 20 steps straight into ring.rows(20) with a terminal list, each committed (T = 60: two laps);
    every valid transition gathered by index= equals what a second env of the same seed, stepped with the same actions through
    step_torch(terminal_obs=...), saw: s, a, r, s', flags bit for bit; s' of a finished step is the terminal observation"""
    import torch
    B, T, K, n_roll = 512, 60, 20, 6
    env = make(B, seed=5, max_episode_steps=30)
    ring = env.replay_torch(T)
    env.reset_torch(out=ring.obs[T - 1])
    env.replay_begin_torch(ring)
    state_free = make(B, seed=5, max_episode_steps=30)
    obs = state_free.reset_torch().cpu().numpy().copy()
    term = env.terminal_list_torch(K * B)
    hist = []
    for c in range(n_roll):
        rows = ring.rows(K)
        env.random_actions_torch(K, seed=3, first_step=c * K, out=rows["action"])
        env.rollout_torch(rows["action"], rows["obs"], rows["reward"], rows["done"], rows["trunc"], terminal=term)
        env.replay_commit_torch(ring, K, terminal=term)
        torch.cuda.synchronize()
        acts = rows["action"].clone()
        for t in range(K):
            tobs = torch.full((B, env.obs_dim), float("nan"), device="cuda")
            o, r, d, tr = state_free.step_torch(acts[t], terminal_obs=tobs)
            torch.cuda.synchronize()
            o, r, d, tr, tb = o.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy(), tr.cpu().numpy().copy(), tobs.cpu().numpy()
            hist.append(dict(s=obs, a=acts[t].cpu().numpy(), r=r, s2=np.where(d[:, None] != 0, tb, o), done=d, trunc=tr))
            obs = o
    env.check_status()
    v = T - 1
    assert len(ring) == v * B
    every = torch.arange(v * B, dtype=torch.int64, device="cuda")
    got = {k: x.cpu().numpy() for k, x in env.replay_sample_torch(ring, v * B, n_step=1, gamma=0.99, index=every).items()}
    torch.cuda.synchronize()
    env.check_status()
    newest = hist[-v:]
    cat = lambda k: np.concatenate([h[k] for h in newest])  # noqa: E731
    done, trunc = cat("done"), cat("trunc")
    assert (done != 0).sum() > 50 and (trunc != 0).any() and ((done != 0) & (trunc == 0)).any()
    assert _same(got["obs"], cat("s")) and _same(got["action"], cat("a")) and _same(got["reward"], cat("r"))
    assert _same(got["next_obs"], cat("s2")) and not np.isnan(got["next_obs"]).any()
    assert np.array_equal(got["truncated"], trunc) and np.array_equal(got["terminated"], ((done != 0) & (trunc == 0)).astype(np.uint8))
    fin = done != 0
    ring_obs = ring.obs.cpu().numpy()
    p = (ring.head - v + np.arange(v * B) // B) % T
    assert not _same(got["next_obs"][fin], ring_obs[p, np.arange(v * B) % B][fin])  # obs[p] there is the next episode's first row
    env.close()
    state_free.close()


def test_calls_in_a_row_differ_and_a_captured_sampler_draws_fresh_indices():
    import torch
    T, B = 8, 1000
    env = make(B, "KeplerCircleOrbit-v0")
    model, commits, extra = synthetic(T, B, env.obs_dim, laps=1.5, p_done=0.05, seed=21)
    ring = env.replay_torch(T)
    env.replay_begin_torch(ring, _dev(extra["obs0"]))
    for com in commits:
        _apply(env, ring, com)
    n, kw = 4096, dict(seed=2 ** 40 + 7, n_step=3, gamma=0.9)
    a, b = _sample(env, ring, n, **kw), _sample(env, ring, n, **kw)
    assert not np.array_equal(a["index"], b["index"])
    _assert_batch(a, sample(model, n, **kw)[0], "call 0")
    _assert_batch(b, sample(model, n, **kw)[0], "call 1")
    out = {k: torch.zeros_like(v) for k, v in env.replay_sample_torch(ring, n, **kw).items()}  # (call 2: allocates the shapes)
    sample(model, n, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.replay_sample_torch(ring, n, out=out, **kw)  # (call 3, warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    sample(model, n, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.replay_sample_torch(ring, n, out=out, **kw)
    assert _header(ring)["sample_calls"] == 4 == model.sample_calls  # (capturing ran nothing)
    for rep in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _assert_batch({k: v.cpu().numpy() for k, v in out.items()}, sample(model, n, **kw)[0], ("replay", rep))
    assert _header(ring)["sample_calls"] == 7
    env.check_status()
    env.close()


def _small(env, C=None, p_done=0.05, laps=1.0, seed=31):
    model, commits, extra = synthetic(8, env.num_envs, env.obs_dim, laps=laps, p_done=p_done, seed=seed, C=C)
    ring = env.replay_torch(8, term_capacity=C)
    env.replay_begin_torch(ring, _dev(extra["obs0"]))
    return model, commits, ring


def _expect_refusal(env, ring):
    """the status word is set: the next call fails with SG_ERR_HIP, check_status raises with the replay message and clears it"""
    import torch
    from space_gym_amd._native import NativeError
    torch.cuda.synchronize()
    with pytest.raises(NativeError, match=r"\(-2\).*an earlier sg_replay_\*_device call refused"):
        env.replay_begin_torch(ring)
    with pytest.raises(NativeError, match=r"\(-1\).*sg_replay_\*_device: a ring without a matching header, a terminal list"):
        env.check_status()
    env.check_status()


@pytest.mark.parametrize("what", ["count", "record"])
def test_a_bad_terminal_list_sets_the_status_word(what):
    import torch
    env = make(1000, "KeplerCircleOrbit-v0")
    model, commits, ring = _small(env)
    com = dict(commits[0])
    assert com["count"] >= 3
    if what == "count":
        com["count"] = com["capacity"] + 1  # records are missing
    else:
        com["step_env"] = com["step_env"].copy()
        com["step_env"][1] = (com["K"], 0)  # one step past the commit
        com["step_env"][2] = (0, 1000)      # one env past the batch
    term_obs0 = torch.full_like(ring.term_obs, -5.0)
    ring.term_obs.copy_(term_obs0)
    _apply(env, ring, com)
    _expect_refusal(env, ring)
    true_count = commits[0]["count"]
    placed = com["capacity"] if what == "count" else true_count
    # (the rows of the list past its true count name (step, env) = (-7, -7): they are ignored like any record outside the commit)
    ignored = np.arange(true_count, placed) if what == "count" else np.array([1, 2])
    assert _header(ring)["term_head"] == placed and _header(ring)["head"] == com["K"]
    got = ring.term_obs.cpu().numpy()
    keep = np.ones(ring.term_capacity, bool)
    keep[:placed] = False
    keep[ignored] = True  # the ignored records' rows keep the sentinel
    ok = np.setdiff1d(np.arange(placed), ignored)
    assert ok.size >= 1 and _same(got[ok], com["tobs"][ok]) and (got[keep] == -5.0).all()
    env.close()


def test_an_index_outside_the_valid_transitions_leaves_its_row_untouched():
    import torch
    env = make(1000, "KeplerCircleOrbit-v0")
    model, commits, ring = _small(env)
    for com in commits:
        _apply(env, ring, com)
    n_valid = len(model)
    index = np.array([0, -1, n_valid, n_valid - 1, 2 ** 40, 17], np.int64)
    want, ok = sample(model, index.size, n_step=3, index=index)
    assert ok.tolist() == [True, False, False, True, False, True]
    spec = env.replay_sample_torch(ring, index.size, index=_dev(np.zeros(6, np.int64)))
    sample(model, 6, index=np.zeros(6, np.int64))
    out = {k: torch.full_like(v, 77) for k, v in spec.items()}
    env.replay_sample_torch(ring, index.size, n_step=3, index=_dev(index), out=out)
    _expect_refusal(env, ring)
    for k in KEYS:
        got = out[k].cpu().numpy()
        assert _same(got[ok], want[k][ok]) and (got[~ok] == 77).all(), k
    env.close()


def test_a_terminal_ring_too_small_for_the_live_window_is_loud():
    import torch
    from space_gym_amd._native import NativeError
    B = 1000
    env = make(B, "KeplerCircleOrbit-v0")
    model, commits, ring = _small(env, C=B // 4, p_done=0.5, laps=2.0)
    assert model.status and ring.term_capacity == B // 4
    hit = None
    for com in commits:
        try:
            _apply(env, ring, com)
            torch.cuda.synchronize()
        except NativeError as err:
            hit = err
            break
    assert hit is not None and "(-2)" in str(hit) and "terminal ring too small" in str(hit)
    with pytest.raises(NativeError, match="terminal ring too small"):
        env.check_status()
    env.check_status()
    env.close()
