"""GPU tests of population_ppo_grad_torch (sg_ppo_population_grad_device).

The oracle is the engine's own single-policy update: member m's gradient slices, twelve statistics and per-row outputs must be, BIT FOR
BIT, what ppo_grad_torch gives with population_member_torch(pop, m), index[m] and member m's coefficients -- and that call is checked
against the NumPy model and eager torch by tests/test_gpu_ppo.py.  The members' parameters are drawn independently and dense, so a wrong
member offset moves a result by ~1e-1.

The shared rows come from rollout_population_torch (dense terminal_value) plus gae_torch on B = 240 envs, P = 3, K = 8, flattened to
1 920 rows; the stored logp and value are moved away from the current ones as tests/test_gpu_ppo.py moves them, so that both branches of
both max are taken.  Member m's index row draws from its own rows t B + 80 m + j: a member boundary falls inside what a plain launch
makes one workgroup.

Beyond the grouping caps (P = 64: 256 // P = 4 workgroups per member) the yardstick is the float64 model tests/population_ppo_model.py
under DESIGN section 18's rule, 8 x |float32-sequential model - float64 model| + 1e-6 (1 + |float64 value|) per gradient tensor, per-row
vector and statistic, each at most 1 % of the float64 magnitude (tests/test_gpu_ppo.py's magnitudes)."""
import ctypes as C

import numpy as np
import pytest

from policy_grad_model import flat, grad_tolerances
from population_model import flat_member, member, random_population
from population_ppo_model import BEYOND_CASES, BEYOND_P, beyond_coef, bit_equal_to_single, member_kwargs
from ppo_model import ppo
from test_gpu_policy import DISCRETE, GOAL, _dev, _np, make
from test_gpu_policy_grad import _check_grads, _grads_np, _report
from test_gpu_population import _copy_member, _pop_handle, _stacked_np
from test_gpu_ppo import _check_rows_and_stats

pytestmark = pytest.mark.gpu

K = 8
KW = dict(clip_range_vf=0.2, ent_coef=0.01)
COEF3 = np.array([[0.2, 0.2, 0.01, 0.5], [0.1, 0.0, 0.0, 1.0], [0.3, 0.15, 0.03, 0.25]], np.float32)  # the rows differ; member 1 does not clip values
ROW_KEYS = ("logp", "value", "g_logp", "g_value")
_cache = {}


def _shared(env_id, hidden, n_hidden, activation, B=240, P=3, critic=True):
    """env, the population handle, the population as NumPy, and the flattened rollout of the population as device tensors (batch) and
    NumPy arrays (host); computed once per key and left unchanged"""
    import torch
    key = (env_id, hidden, n_hidden, activation, B, P, critic)
    if key in _cache:
        return _cache[key]
    env = make(env_id, B, seed=7, max_episode_steps=5)
    rng = np.random.default_rng([hidden, n_hidden, B, P])
    continuous = not env.discrete
    pop = random_population(rng, P, env.obs_dim, hidden, n_hidden, 2 if continuous else 6, critic=True, continuous=continuous)
    h_roll = _pop_handle(env, pop, activation)
    D = env.obs_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, dtype=torch.int32) if env.discrete else z(K, B, 2), logp=z(K, B), value=z(K + 1, B),
             reward=z(K, B), done=z(K, B, dtype=torch.uint8), trunc=z(K, B, dtype=torch.uint8))
    tv = z(K, B)
    b["obs"][0].copy_(env.reset_torch())
    env.rollout_population_torch(h_roll, seed=3, terminal_value=tv, **b)
    adv, ret = env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1], terminal_value=tv)
    env.check_status()
    rows = K * B
    # the [K, B] buffers reshaped: no permuting copy
    host = dict(zip(("obs", "action", "logp", "value", "advantage", "ret"),
                    _np(b["obs"][:-1].reshape(rows, D), b["action"].reshape((rows,) if env.discrete else (rows, 2)), b["logp"].reshape(rows),
                        b["value"][:-1].reshape(rows), adv.reshape(rows), ret.reshape(rows))))
    assert np.isfinite(host["advantage"]).all() and host["advantage"].std() > 0
    host["logp"] = (host["logp"] + 0.05 + 0.3 * rng.standard_normal(rows)).astype(np.float32)
    host["value"] = (host["value"] + 0.3 * rng.standard_normal(rows)).astype(np.float32)
    if not critic:
        pop = dict(pop, critic=None)
    h = _pop_handle(env, pop, activation)
    batch = {k: _dev(v) for k, v in host.items()}
    _cache[key] = (env, h, pop, batch, host)
    return _cache[key]


def teardown_module(module):
    for entry in _cache.values():
        entry[0].close()
    _cache.clear()


def _own_rows_index(rng, P, n, B):
    """member m's entries from its own rows t B + (B / P) m + j, with repeats"""
    per = B // P
    return np.stack([rng.integers(0, K, n) * B + per * m + rng.integers(0, per, n) for m in range(P)]).astype(np.int64)


def _row_outputs(P, n, critic=True):
    import torch
    return {k: torch.full((P, n) if P else (n,), float("nan"), device="cuda") for k in (ROW_KEYS if critic else ("logp", "g_logp"))}


def _single_kwargs(coef, m, kw):
    """ppo_grad_torch's keywords for member m: its row of the coefficient tensor, or the call's scalars"""
    rest = {k: v for k, v in kw.items() if k not in ("clip_range", "clip_range_vf", "ent_coef", "vf_coef")}
    if coef is None:
        return kw
    return dict(rest, **member_kwargs(coef, m))


def _assert_members_equal_single_calls(env, h, batch, d_index, coef, kw, what, critic=True, branches=False):
    """the population call against ppo_grad_torch of every member's own handle; returns the population's (grads as NumPy, stats, rows)"""
    import torch
    P = h.members
    n = int(d_index.shape[1]) if d_index is not None else int(batch["obs"].shape[0]) // P
    rows = _row_outputs(P, n, critic)
    grads, stats = env.population_ppo_grad_torch(h, batch, d_index, coef=_dev(coef) if coef is not None else None, rows=rows, **kw)
    got, got_stats = _stacked_np(grads), _np(stats)[0]
    got_rows = dict(zip(rows, _np(*rows.values())))
    assert got_stats.shape == (P, 12) and all(v.shape == (P, n) for v in got_rows.values())
    for m in range(P):
        idx_m = d_index[m] if d_index is not None else torch.arange(m * n, (m + 1) * n, device="cuda")
        rows_m = _row_outputs(0, n, critic)
        g_m, s_m = env.ppo_grad_torch(env.population_member_torch(h, m), batch, idx_m, rows=rows_m, **_single_kwargs(coef, m, kw))
        want, mine = _grads_np(g_m), flat_member(got, m)
        assert set(want) == set(mine), (what, m)
        for k in want:
            assert mine[k].tobytes() == want[k].tobytes(), (what, m, k, int((mine[k] != want[k]).sum()))
        assert got_stats[m].tobytes() == _np(s_m)[0].tobytes(), (what, m, got_stats[m], _np(s_m)[0])
        for k, v in zip(rows_m, _np(*rows_m.values())):
            assert got_rows[k][m].tobytes() == v.tobytes(), (what, m, k)
        assert np.isfinite(got_stats[m]).all() and got_stats[m][9] == 0, (what, m)
        if branches:  # both branches of both max occur in every member
            gl = got_rows["g_logp"][m]
            assert (gl == 0).any() and (gl != 0).any(), (what, m)
            if critic and (coef is None or coef[m][1] > 0):
                gv = got_rows["g_value"][m]
                assert (gv == 0).any() and (gv != 0).any(), (what, m)
    return got, got_stats, got_rows


@pytest.mark.parametrize("n", [2, 200, 2049])
@pytest.mark.parametrize("hidden,n_hidden,activation", [(64, 2, "tanh"), (33, 1, "relu"), (128, 2, "tanh")])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_every_member_is_ppo_grad_torch_bit_for_bit(env_id, hidden, n_hidden, activation, n):
    """1: gradients, the 12 statistics and the four per-row outputs, with a coefficient tensor whose rows differ and with the scalars
    only; n = 2, 200 and 2 049 per member: a partial tile, full tiles plus a partial one and several tiles at R = 128 / 256 / 64"""
    env, h, pop, batch, host = _shared(env_id, hidden, n_hidden, activation)
    from population_model import grad_rows
    assert bit_equal_to_single(n, grad_rows(hidden), 3)
    index = _own_rows_index(np.random.default_rng(n + hidden), 3, n, 240)
    d_index = _dev(index)
    what = (env_id, hidden, n_hidden, activation, n)
    a = _assert_members_equal_single_calls(env, h, batch, d_index, COEF3, {}, what + ("coef",), branches=n >= 200)
    b = _assert_members_equal_single_calls(env, h, batch, d_index, None, KW, what + ("scalars",), branches=n >= 200)
    assert a[1].tobytes() != b[1].tobytes()
    # the members differ: member 1's rows under member 0's slices are something else
    assert np.abs(a[2]["logp"][0] - a[2]["logp"][1]).max() > 1e-3
    env.check_status()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_one_member_is_ppo_grad_torch_on_the_whole_batch(env_id):
    """1: P = 1 against ppo_grad_torch, with an index and on all rows in order"""
    env, h, pop, batch, host = _shared(env_id, 64, 2, "tanh", P=1)
    index = _dev(np.random.default_rng(5).integers(0, K * 240, (1, 777)).astype(np.int64))
    _assert_members_equal_single_calls(env, h, batch, index, COEF3[:1], {}, (env_id, "P = 1"), branches=True)
    _assert_members_equal_single_calls(env, h, batch, None, None, KW, (env_id, "P = 1, all rows"), branches=True)
    env.check_status()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_no_index_gives_member_m_the_rows_m_n_onwards(env_id):
    """1: index=None on the batch laid out [P, n]: member m takes rows [640 m, 640 (m + 1))"""
    env, h, pop, batch, host = _shared(env_id, 33, 1, "relu")
    _assert_members_equal_single_calls(env, h, batch, None, COEF3, {}, (env_id, "index=None"))
    env.check_status()


def _beyond(env_id, hidden):
    """the P = 64 population on B = 256 envs (four envs per member) and its rollout of 2 048 rows"""
    return _shared(env_id, hidden, 1, "tanh", B=256, P=BEYOND_P)


@pytest.mark.parametrize("hidden,R,n", BEYOND_CASES)
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_beyond_the_caps_every_member_equals_the_model(env_id, hidden, R, n):
    """2: P = 64, 256 // P = 4 workgroups per member: n = 4 R + 300 regroups the parameter partials, n = 4 396 the advantage partials as
    well.  Random indices over the rollout, with repeats; per member and per tensor against the float64 model, the 1 % cap asserted; run
    twice into NaN-prefilled outputs: the second run is bit-equal and every output overwritten"""
    import torch
    env, h, pop, batch, host = _beyond(env_id, hidden)
    P, rows_total = BEYOND_P, K * 256
    assert not bit_equal_to_single(n, R, P) and bit_equal_to_single(n, R, 1)
    rng = np.random.default_rng([3, hidden, n])
    index = rng.integers(0, rows_total, (P, n)).astype(np.int64)
    coef = beyond_coef(rng, P)
    d_index, d_coef = _dev(index), _dev(coef)
    rows = _row_outputs(P, n)
    grads, stats = env.population_ppo_grad_torch(h, batch, d_index, coef=d_coef, rows=rows)
    got, got_stats = _stacked_np(grads), _np(stats)[0]
    got_rows = dict(zip(rows, _np(*rows.values())))
    h.workspace.fill_(255)  # every float of it a NaN
    every = [x for pairs in (grads["actor"], grads["critic"]) for pair in pairs for x in pair] + list(rows.values()) + [stats] + (
        [grads["log_std"]] if grads["log_std"] is not None else [])
    for t in every:
        t.fill_(float("nan"))
    again, stats2 = env.population_ppo_grad_torch(h, batch, d_index, coef=d_coef, out=grads, stats=stats, rows=rows)
    assert again is grads and stats2 is stats
    torch.cuda.synchronize()
    assert not any(bool(t.isnan().any()) for t in every)
    second, second_rows = _stacked_np(again), dict(zip(rows, _np(*rows.values())))
    assert _np(stats2)[0].tobytes() == got_stats.tobytes()
    for k in ROW_KEYS:
        assert second_rows[k].tobytes() == got_rows[k].tobytes(), k
    worst = []
    for m in range(P):
        a, b = flat_member(got, m), flat_member(second, m)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a), m
        kw = member_kwargs(coef, m)
        pol = member(pop, m)
        m64, m32 = ppo(pol, host, index[m], **kw), ppo(pol, host, index[m], dtype=np.float32, **kw)
        what = (env_id, hidden, n, m)
        _check_rows_and_stats({k: got_rows[k][m] for k in ROW_KEYS}, got_stats[m], m32, m64, kw, what, worst)
        _check_grads(a, flat(m32), flat(m64), what, worst)
    _report(worst)
    env.check_status()


def _bits(got, stats, rows, m):
    out = {k: v.tobytes() for k, v in flat_member(got, m).items()}
    out["stats"] = stats[m].tobytes()
    out.update({"rows." + k: v[m].tobytes() for k, v in rows.items()})
    return out


def _run(env, h, batch, d_index, coef, P, n, **kw):
    rows = _row_outputs(P, n)
    grads, stats = env.population_ppo_grad_torch(h, batch, d_index, coef=_dev(coef) if coef is not None else None, rows=rows, **kw)
    return _stacked_np(grads), _np(stats)[0], dict(zip(rows, _np(*rows.values())))


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_a_members_nan_and_bad_indices_stay_in_that_member(env_id):
    """3: NaN in member 1's ent_coef, or in one of its weights, leaves members 0 and 2 bit-equal to the clean run; indices outside the
    rows (the clamped, defined case of the contract) in member 2's row change member 2's outputs only, are counted in its bad_rows, and
    which way and how far outside is all the same to the gradients, the statistics and the per-row g_logp / g_value"""
    import torch
    env, h, pop, batch, host = _shared(env_id, 64, 2, "tanh")
    P, n, rows_total = 3, 300, K * 240
    index = _own_rows_index(np.random.default_rng(8), P, n, 240)
    d_index = _dev(index)
    clean = _run(env, h, batch, d_index, COEF3, P, n)
    assert np.isfinite(clean[1]).all()
    nan_coef = COEF3.copy()
    nan_coef[1, 2] = np.nan
    r = _run(env, h, batch, d_index, nan_coef, P, n)
    assert _bits(*r, 0) == _bits(*clean, 0) and _bits(*r, 2) == _bits(*clean, 2)
    assert np.isnan(r[1][1][0]) and np.isnan(r[1][1]).sum() == 1 and any(np.isnan(v).any() for v in flat_member(r[0], 1).values())
    w = h.tensors[2 * h.n_hidden + 1]  # the bias of the actor's head, stacked [P, head]: linear, so a NaN in it reaches the loss
    kept = w[1, 0].item()
    with torch.no_grad():
        w[1, 0] = float("nan")
    r = _run(env, h, batch, d_index, COEF3, P, n)
    with torch.no_grad():
        w[1, 0] = kept
    # (the clamp of the ratio keeps the NaN out of member 1's loss; its approx_kl, (ratio - 1) - lr, carries it)
    assert _bits(*r, 0) == _bits(*clean, 0) and _bits(*r, 2) == _bits(*clean, 2) and np.isnan(r[1][1][4]) and np.isfinite(r[1][[0, 2]]).all()
    assert _bits(*_run(env, h, batch, d_index, COEF3, P, n), 1) == _bits(*clean, 1)  # the weight is back
    where = [0, 7, 131, 299]
    results = []
    for bad in (-1, rows_total, rows_total + 10 ** 12, -2 ** 62):
        idx = index.copy()
        idx[2, where] = bad
        r = _run(env, h, batch, _dev(idx), COEF3, P, n)
        assert _bits(*r, 0) == _bits(*clean, 0) and _bits(*r, 1) == _bits(*clean, 1), bad
        assert r[1][2][9] == 4 and r[1][0][9] == 0 and r[1][1][9] == 0 and np.isfinite(r[1]).all(), bad
        assert not r[2]["g_logp"][2][where].any() and not r[2]["g_value"][2][where].any() and r[2]["g_logp"][2].any()
        results.append(_bits(*r, 2))
    # gradients, statistics and the per-row g_logp / g_value: the same bits for all four.  The per-row logp / value of a bad entry are
    # those of the row it was clamped to, row 0 below the rows and the last row above them: the same bits on the same side
    forward = ("rows.logp", "rows.value")
    rest = lambda bits: {k: v for k, v in bits.items() if k not in forward}
    assert rest(results[0]) != rest(_bits(*clean, 2)) and all(rest(x) == rest(results[0]) for x in results[1:])
    assert results[0] == results[3] and results[1] == results[2] and results[0] != results[1]
    env.check_status()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_a_population_without_a_critic_and_other_configurations(env_id):
    """4: without a critic value_loss is 0 and ret and value are not needed; clip_range = inf; normalize_advantage=False has adv_mean
    and adv_std 0.  Each against the members' single calls, bit for bit"""
    env, h, pop, batch, host = _shared(env_id, 64, 2, "tanh", critic=False)
    n = 200
    d_index = _dev(_own_rows_index(np.random.default_rng(2), 3, n, 240))
    few = {k: batch[k] for k in ("obs", "action", "logp", "advantage")}
    for b in (batch, few):
        got, stats, rows = _assert_members_equal_single_calls(env, h, b, d_index, COEF3, {}, (env_id, "no critic"), critic=False, branches=True)
        assert got["critic"] is None and (stats[:, 2] == 0).all() and (stats[:, 0] != 0).all()
    env, h, pop, batch, host = _shared(env_id, 64, 2, "tanh")
    got, stats, rows = _assert_members_equal_single_calls(env, h, batch, d_index, None, dict(clip_range=float("inf"), vf_coef=1.0), (env_id, "inf"))
    assert (stats[:, 6] == 0).all() and (rows["g_logp"] != 0).all()
    got, stats, rows = _assert_members_equal_single_calls(env, h, batch, d_index, COEF3, dict(normalize_advantage=False), (env_id, "raw"),
                                                          branches=True)
    assert (stats[:, 7] == 0).all() and (stats[:, 8] == 0).all()
    env.check_status()


def test_captured_act_and_step_and_a_captured_update_follow_the_callers_tensors():
    """5: population_act_torch + step_torch in one capture and the update in another, after one warm-up call each; between replays
    W[1].copy_(W[0]) on every tensor and a rewritten coefficient tensor; each replay equals the eager call on the same state"""
    import torch
    B, P, n = 240, 3, 300
    rng = np.random.default_rng(12)
    kw = dict(seed=8, max_episode_steps=3)
    ea, eb = make(GOAL, B, **kw), make(GOAL, B, **kw)
    pop = random_population(rng, P, ea.obs_dim, 64, 2, 2)
    h = _pop_handle(eb, pop)
    obs = eb.reset_torch().clone()
    ea.reset_torch()
    act = dict(action=torch.zeros((B, 2), device="cuda"), logp=torch.zeros(B, device="cuda"), value=torch.zeros(B, device="cuda"))
    step = dict(obs=torch.zeros((B, eb.obs_dim), device="cuda"), reward=torch.zeros(B, device="cuda"),
                done=torch.zeros(B, dtype=torch.uint8, device="cuda"), trunc=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    _, _, _, batch, host = _shared(GOAL, 64, 2, "tanh")
    d_index = _dev(_own_rows_index(rng, P, n, B))
    d_coef = _dev(COEF3)
    snap = eb.snapshot_torch()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream: the LDS limits, the workspace
        eb.population_act_torch(h, obs, seed=2, step=7, out=act)
        eb.step_torch(act["action"], out=step)
        out, s_out = eb.population_ppo_grad_torch(h, batch, d_index, coef=d_coef)
    side.synchronize()
    eb.restore_torch(snap)
    torch.cuda.synchronize()
    g_act, g_upd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_act, stream=side):
        eb.population_act_torch(h, obs, seed=2, step=7, out=act)
        eb.step_torch(act["action"], out=step)
    with torch.cuda.graph(g_upd, stream=side):
        eb.population_ppo_grad_torch(h, batch, d_index, coef=d_coef, out=out, stats=s_out)
    every = [x for pairs in (out["actor"], out["critic"]) for pair in pairs for x in pair] + [out["log_std"], s_out]
    for copied in (False, True):
        if copied:
            _copy_member(h.tensors, 1, 0)
            d_coef.copy_(_dev(COEF3[[2, 0, 1]] * np.float32(0.5)))
        for t in list(act.values()) + [step["obs"], step["reward"]] + every:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        g_act.replay()
        g_upd.replay()
        torch.cuda.synchronize()
        want = _np(*ea.population_act_torch(h, obs, seed=2, step=7))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(_np(act["action"], act["logp"], act["value"]), want)), copied
        twin = ea.step_torch(act["action"].clone())  # the eager twin takes the replay's actions
        for name, w in zip(("obs", "reward", "done", "trunc"), twin):
            assert _np(step[name])[0].tobytes() == _np(w)[0].tobytes(), (copied, name)
        got, got_stats = _stacked_np(out), _np(s_out)[0]
        eager, e_stats = ea.population_ppo_grad_torch(h, batch, d_index, coef=d_coef)
        e, e_stats = _stacked_np(eager), _np(e_stats)[0]
        for m in range(P):
            a, b = flat_member(got, m), flat_member(e, m)
            assert all(a[k].tobytes() == b[k].tobytes() for k in a), (copied, m)
        assert got_stats.tobytes() == e_stats.tobytes() and np.isfinite(got_stats).all(), copied
        if copied:  # member 1 is member 0 now, up to its rows and coefficients: the update saw the copy and the new coefficients
            assert got_stats.tobytes() != first_stats.tobytes()
        first_stats = got_stats
    h2 = _pop_handle(eb, pop)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(g2, stream=side):
            eb.population_ppo_grad_torch(h2, batch, d_index, coef=d_coef, out=out, stats=s_out)
    torch.cuda.synchronize()
    assert h2.workspace is None
    ea.check_status()
    eb.check_status()
    ea.close()
    eb.close()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_one_pbt_shaped_update_equals_eager_torch(env_id):
    """6: the loss of the three members summed in torch over population_evaluate_torch, each member's advantages normalised on its own
    minibatch, and backward(): the stacked .grad against the fused call's tensors within DESIGN section 18's tolerance (from the model, per
    member and tensor); each member's loss statistic within 1e-4 (1 + |loss|); ppo_assign_grads hands the stacked tensors over"""
    import torch
    env, h, pop, batch, host = _shared(env_id, 64, 2, "tanh")
    P, n = 3, 777
    index = _own_rows_index(np.random.default_rng(21), P, n, 240)
    d_index = _dev(index)
    grads, stats = env.population_ppo_grad_torch(h, batch, d_index, coef=_dev(COEF3))
    got, got_stats = _stacked_np(grads), _np(stats)[0]
    for t in h.tensors:
        t.requires_grad_(True)
        t.grad = None
    try:
        logp, ent, value = env.population_evaluate_torch(h, batch["obs"][d_index].contiguous(), batch["action"][d_index].contiguous())
        c = _dev(COEF3)
        col = lambda k: batch[k][d_index]
        lr = logp - col("logp")
        ratio = lr.exp()
        adv, ret, ov = col("advantage"), col("ret"), col("value")
        adv = (adv - adv.mean(1, keepdim=True)) / (adv.std(1, keepdim=True) + 1e-8)
        cr, cv = c[:, 0:1], c[:, 1:2]
        pg = torch.max(-adv * ratio, -adv * torch.minimum(torch.maximum(ratio, 1 - cr), 1 + cr)).mean(1)
        clipped = 0.5 * torch.max((value - ret) ** 2, (ov + torch.minimum(torch.maximum(value - ov, -cv), cv) - ret) ** 2)
        vl = torch.where(cv > 0, clipped, 0.5 * (value - ret) ** 2).mean(1)
        losses = pg - c[:, 2] * ent.mean(1) + c[:, 3] * vl
        losses.sum().backward()
        L = h.n_hidden + 1
        t = [x.grad.cpu().numpy() for x in h.tensors]
        pairs = lambda ts: [(ts[2 * l], ts[2 * l + 1]) for l in range(L)]
        eager = dict(actor=pairs(t[:2 * L]), critic=pairs(t[2 * L:4 * L]), log_std=t[-1] if not env.discrete else None)
        worst = []
        for m in range(P):
            kw = member_kwargs(COEF3, m)
            m64, m32 = flat(ppo(member(pop, m), host, index[m], **kw)), flat(ppo(member(pop, m), host, index[m], dtype=np.float32, **kw))
            tol = grad_tolerances(m32, m64)
            mine, theirs = flat_member(got, m), flat_member(eager, m)
            assert set(mine) == set(theirs) == set(m64)
            for k in m64:
                err = float(np.abs(mine[k].astype(np.float64) - theirs[k]).max())
                worst.append((err / tol[k], err, tol[k], float(np.abs(m64[k]).max()), (env_id, "eager", m), k))
                assert tol[k] <= 0.01 * np.abs(m64[k]).max() and err <= tol[k], (m, k, err, tol[k])
            loss = float(losses[m].detach())
            assert abs(got_stats[m][0] - loss) <= 1e-4 * (1 + abs(loss)), (m, got_stats[m][0], loss)
        _report(worst)
        for x in h.tensors:
            x.grad = None
        env.ppo_assign_grads(h, grads)
        flat_grads = [x for pair in grads["actor"] + grads["critic"] for x in pair] + ([grads["log_std"]] if grads["log_std"] is not None else [])
        assert len(flat_grads) == len(h.tensors) and all(p.grad is g and p.grad.shape == p.shape for p, g in zip(h.tensors, flat_grads))
    finally:
        for x in h.tensors:
            x.grad = None
            x.requires_grad_(False)
    env.check_status()


def test_native_refusals():
    """7: every refusal returns the error with its message and writes nothing: the outputs prefilled with NaN stay NaN"""
    import torch
    from space_gym_amd import _native
    env, h, pop, batch, host = _shared(GOAL, 64, 2, "tanh")
    h_nc = _pop_handle(env, dict(pop, critic=None))
    P, n, rows = 3, 40, K * 240
    d_index = _dev(_own_rows_index(np.random.default_rng(51), P, n, 240))
    d_coef = _dev(COEF3)
    full, stats = env.population_ppo_grad_torch(h, batch, d_index, coef=d_coef)
    row_t = torch.full((P, n), float("nan"), device="cuda")
    every = [x for pairs in (full["actor"], full["critic"]) for pair in pairs for x in pair] + [full["log_std"], stats, row_t]
    for t in every:
        t.fill_(float("nan"))
    lib, s, ws = env._lib, env._stream(), h.workspace
    need = lib.sg_ppo_population_grad_workspace_bytes(env._h, C.byref(h.struct), P, n)
    params = lib.sg_policy_population_grad_workspace_bytes(env._h, C.byref(h.struct), P, n)
    # the parameter partials, double [P][Gadv = 1][2], float [P][G = 1][8]
    assert need == (params + 7) // 8 * 8 + 8 * 2 * P + 4 * 8 * P and need <= ws.numel()
    one = lib.sg_ppo_population_grad_workspace_bytes(env._h, C.byref(h.struct), 64, 4396)
    assert one == (lib.sg_policy_population_grad_workspace_bytes(env._h, C.byref(h.struct), 64, 4396) + 7) // 8 * 8 + 8 * 2 * 64 * 4 + 4 * 8 * 64 * 4
    assert lib.sg_ppo_population_grad_workspace_bytes(env._h, C.byref(h.struct), P, 0) == 0 and b"n must be" in lib.sg_last_error(env._h)
    assert lib.sg_ppo_population_grad_workspace_bytes(env._h, C.byref(h.struct), 0, n) == 0 and b"members must be" in lib.sg_last_error(env._h)
    assert lib.sg_ppo_population_grad_workspace_bytes(env._h, C.byref(h.struct), 3, 2 ** 30) == 0 and b"members x n" in lib.sg_last_error(env._h)

    def grads_struct(critic=True):
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        for l, (w, b) in enumerate(full["actor"]):
            g.actor.weight[l], g.actor.bias[l] = w.data_ptr(), b.data_ptr()
        if critic:
            for l, (w, b) in enumerate(full["critic"]):
                g.critic.weight[l], g.critic.bias[l] = w.data_ptr(), b.data_ptr()
        g.log_std = full["log_std"].data_ptr()
        return g

    def refused(match, policy=h, members=P, cfg=(), drop=(), n_rows=rows, count=n, g="given", st=stats, row_out=None, w=ws, wbytes=None,
                w_offset=0, index=d_index, coef=d_coef, no_batch=False, no_cfg=False):
        c = _native.SgPpoConfig()
        lib.sg_ppo_config_init(C.byref(c))
        c.clip_range_vf, c.ent_coef = 0.2, 0.01
        for k, v in cfg:
            setattr(c, k, v)
        cols = dict(obs=batch["obs"], action=batch["action"], old_logp=batch["logp"], advantage=batch["advantage"], ret=batch["ret"],
                    old_value=batch["value"], index=index)
        b = _native.SgPpoBatch(**{k: (v.data_ptr() if v is not None and k not in drop else None) for k, v in cols.items()})
        gs = grads_struct(critic=policy is h) if g == "given" else g
        rc = lib.sg_ppo_population_grad_device(
            env._h, C.byref(policy.struct), members, None if no_cfg else C.byref(c), None if no_batch else C.byref(b),
            C.c_void_p(coef.data_ptr()) if coef is not None else None, n_rows, count, C.byref(gs) if gs is not None else None,
            C.c_void_p(st.data_ptr()) if st is not None else None, C.byref(row_out) if row_out is not None else None,
            C.c_void_p(w.data_ptr() + w_offset) if w is not None else None, ws.numel() - w_offset if wbytes is None else wbytes, s)
        assert rc == -1 and match in lib.sg_last_error(env._h), (match, rc, lib.sg_last_error(env._h))

    # whatever population_check refuses
    refused(b"members must be 1 .. 65535", members=0)
    refused(b"members must be 1 .. 65535", members=65536)
    # whatever sg_ppo_grad_device refuses, under this entry point's name
    refused(b"sg_ppo_population_grad_device: null cfg", no_cfg=True)
    refused(b"struct_size", cfg=[("struct_size", 28)])
    refused(b"reserved", cfg=[("reserved", 1)])
    refused(b"clip_range must be > 0", cfg=[("clip_range", 0.0)])  # the host scalars are checked beside a coefficient tensor
    refused(b"clip_range must be > 0", cfg=[("clip_range", float("nan"))], coef=None)
    refused(b"ent_coef and vf_coef must be >= 0", cfg=[("ent_coef", -0.5)])
    refused(b"ent_coef and vf_coef must be >= 0", cfg=[("vf_coef", float("nan"))])
    refused(b"clip_range_vf is NaN", cfg=[("clip_range_vf", float("nan"))])
    refused(b"adv_epsilon", cfg=[("adv_epsilon", -1.0)])
    refused(b"rows must be", n_rows=0)
    refused(b"n must be", count=0)
    refused(b"normalize_advantage needs n >= 2", count=1)
    refused(b"null batch", no_batch=True)
    for col in ("obs", "action", "old_logp", "advantage", "ret"):
        refused(b"null batch." + col.encode(), drop=(col,))
    refused(b"needs batch.old_value", drop=("old_value",), coef=None)  # the scalar clip_range_vf is on
    refused(b"member_coef with a critic needs batch.old_value", drop=("old_value",), cfg=[("clip_range_vf", 0.0)])
    refused(b"members x n must be at most 2^31 - 1", count=2 ** 30)
    refused(b"members x n = 3 x 641 rows without an index", drop=("index",), count=641)
    refused(b"null stats_out", st=None)
    refused(b"null grads", g=None)
    refused(b"of the critic", g=grads_struct(critic=False))
    refused(b"null workspace", w=None)
    refused(b"workspace of", wbytes=need - 1)
    big = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    refused(b"aligned to 8 bytes", w=big, w_offset=4, wbytes=need + 32)
    refused(b"critic gradients given", policy=h_nc, g=grads_struct())
    r = _native.SgPpoRows(value=row_t.data_ptr())
    refused(b"row_out.value / row_out.g_value given, but the policy has no critic", policy=h_nc, row_out=r)
    torch.cuda.synchronize()
    assert all(bool(t.isnan().all()) for t in every)
    # without a critic a coefficient tensor needs no old_value; and the handle still works
    few = {k: batch[k] for k in ("obs", "action", "logp", "advantage")}
    _, st_nc = env.population_ppo_grad_torch(h_nc, few, d_index, coef=d_coef)
    _, st = env.population_ppo_grad_torch(h, batch, d_index, coef=d_coef, rows=dict(value=row_t))
    torch.cuda.synchronize()
    assert np.isfinite(_np(st_nc)[0]).all() and np.isfinite(_np(st)[0]).all() and not bool(row_t.isnan().any())
    env.check_status()
