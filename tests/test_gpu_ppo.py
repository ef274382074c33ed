"""GPU tests of ppo_grad_torch (sg_ppo_grad_device) against policy_grad_torch / policy_evaluate_raw_torch (bit for bit), the NumPy
model tests/ppo_model.py and eager torch.

The rows come from a short rollout_policy_torch plus gae_torch on 256 envs, flattened (8 steps: 2048 rows); minibatches larger than
that index the buffer with repeats.  Except in the first-epoch test the stored logp and value are moved away from the current ones
(by 0.05 + 0.3 N(0, 1) and 0.3 N(0, 1)), as after some optimizer steps, so that both branches of both max are taken.

Tolerances are DESIGN section 18's form: 8 x |float32-sequential model - float64 model| + 1e-6 (1 + |float64 value|), per gradient
tensor, per per-row vector and per statistic.  Each must also be at most 1 % of the float64 magnitude: max|.| of a tensor or vector, and
for a mean the float64 mean of the absolute per-row terms (for loss: of its three parts, weighted by the coefficients), which is what a
wrong row moves it by; adv_mean is measured against adv_std.

Measured on an MI355X, the three worst error / tolerance ratios of test 2 are recorded in DESIGN section 24."""
import ctypes as C

import numpy as np
import pytest

from policy_grad_model import flat, grad_tolerances
from policy_model import random_policy
from ppo_model import STATS, ppo
from test_gpu_policy import DISCRETE, GOAL, _dev, _np, make
from test_gpu_policy_grad import _check_grads, _grads_np, _modules, _report

pytestmark = pytest.mark.gpu

B, K = 256, 8
KW = dict(clip_range_vf=0.2, ent_coef=0.01)
_cache = {}


def _pairs(net):
    import torch
    return [(m.weight, m.bias) for m in net if isinstance(m, torch.nn.Linear)]


def _rollout(env_id, hidden, n_hidden, activation, critic=True, moved=True):
    """env, handle, the policy as NumPy and as float32 CUDA modules (the handle reads the modules' parameters), and the flattened rollout as
    device tensors (batch) and NumPy arrays (host); computed once per key and left unchanged"""
    import torch
    key = (env_id, hidden, n_hidden, activation, critic, moved)
    if key in _cache:
        return _cache[key]
    env = make(env_id, B, seed=7, max_episode_steps=5)
    rng = np.random.default_rng(hidden + 3 * n_hidden)
    continuous = not env.discrete
    pol = random_policy(rng, env.obs_dim, hidden, n_hidden, 2 if continuous else 6, critic=True, continuous=continuous)
    actor, critic_net, log_std = _modules(pol, activation, torch.float32, "cuda")
    h_roll = env.policy_torch(actor=_pairs(actor), critic=_pairs(critic_net), log_std=log_std, activation=activation)
    D = env.obs_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, dtype=torch.int32) if env.discrete else z(K, B, 2), logp=z(K, B), value=z(K + 1, B),
             reward=z(K, B), done=z(K, B, dtype=torch.uint8), trunc=z(K, B, dtype=torch.uint8))
    term = env.terminal_list_torch(K * B)
    b["obs"][0].copy_(env.reset_torch())
    env.rollout_policy_torch(h_roll, seed=3, terminal=term, **b)
    adv, ret = env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1],
                             terminal=env.value_list_torch(terminal=term, values=term["value"]))
    env.check_status()
    rows = K * B
    host = dict(zip(("obs", "action", "logp", "value", "advantage", "ret"),
                    _np(b["obs"][:-1].reshape(rows, D), b["action"].reshape((rows,) if env.discrete else (rows, 2)), b["logp"].reshape(rows),
                        b["value"][:-1].reshape(rows), adv.reshape(rows), ret.reshape(rows))))
    assert np.isfinite(host["advantage"]).all() and host["advantage"].std() > 0
    if moved:
        host["logp"] = (host["logp"] + 0.05 + 0.3 * rng.standard_normal(rows)).astype(np.float32)
        host["value"] = (host["value"] + 0.3 * rng.standard_normal(rows)).astype(np.float32)
    if not critic:
        pol = dict(pol, critic=None)
    h = env.policy_torch(actor=_pairs(actor), critic=_pairs(critic_net) if critic else None, log_std=log_std, activation=activation)
    batch = {k: _dev(v) for k, v in host.items()}
    _cache[key] = (env, h, pol, (actor, critic_net if critic else None, log_std), batch, host)
    return _cache[key]


def teardown_module(module):
    for entry in _cache.values():
        entry[0].close()
    _cache.clear()


def _index(n, seed, rows=K * B):
    return np.random.default_rng(seed).integers(0, rows, n).astype(np.int64)


def _row_outputs(n, critic=True):
    import torch
    return {k: torch.full((n,), float("nan"), device="cuda") for k in (("logp", "value", "g_logp", "g_value") if critic else ("logp", "g_logp"))}


def _assert_same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k] != b[k]).sum()))


def _bit_exact_core(env_id, hidden, n_hidden, activation, n):
    import torch
    env, h, pol, _, batch, host = _rollout(env_id, hidden, n_hidden, activation)
    index = _index(n, n + hidden)
    d_index = _dev(index)
    rows = _row_outputs(n)
    grads, stats = env.ppo_grad_torch(h, batch, d_index, rows=rows, **KW)
    got = _grads_np(grads)
    obs_g, action_g = batch["obs"][d_index].contiguous(), batch["action"][d_index].contiguous()
    g_entropy = torch.full((n,), float(-np.float32(KW["ent_coef"]) / np.float32(n)), device="cuda")
    want = _grads_np(env.policy_grad_torch(h, obs_g, action_g, g_logp=rows["g_logp"], g_entropy=g_entropy, g_value=rows["g_value"]))
    what = (env_id, hidden, n_hidden, activation, n)
    _assert_same_bits(got, want, what)
    logp, _, value = _np(*env.policy_evaluate_raw_torch(h, obs_g, action_g))
    r_logp, r_value, r_gl, r_gv, s = _np(rows["logp"], rows["value"], rows["g_logp"], rows["g_value"], stats)
    assert r_logp.tobytes() == logp.tobytes() and r_value.tobytes() == value.tobytes(), what
    assert np.isfinite(s).all() and s[9] == 0 and np.isfinite(r_gl).all() and np.isfinite(r_gv).all(), what
    if n >= 200:  # both branches of both max are taken
        assert (r_gl == 0).any() and (r_gl != 0).any() and (r_gv == 0).any() and (r_gv != 0).any(), what
    env.check_status()


@pytest.mark.parametrize("n", [2, 200, 2049])
@pytest.mark.parametrize("hidden,n_hidden,activation", [(64, 2, "tanh"), (33, 1, "relu")])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_gradients_are_policy_grad_torchs_bit_for_bit(env_id, hidden, n_hidden, activation, n):
    """1: with the per-row g_logp / g_value the kernel reports, policy_grad_torch on the gathered rows gives the same bits at the same n;
    the reported logp / value are policy_evaluate_raw_torch's bits"""
    _bit_exact_core(env_id, hidden, n_hidden, activation, n)


def test_bit_for_bit_when_workgroups_take_a_second_row_tile():
    """1, past the grid cap: hidden 128 has workgroups of 64 rows; 256 of them and 300 rows more, indexed with repeats into the 2048 rows"""
    _bit_exact_core(GOAL, 128, 2, "tanh", 256 * 64 + 300)


def _magnitudes(m64, kw, critic):
    """the float64 magnitude of each statistic 0 .. 8 (see the module docstring)"""
    t = [float(np.abs(v).mean()) for v in m64["terms"]]
    loss = t[0] + kw.get("ent_coef", 0.0) * t[2] + (kw.get("vf_coef", 0.5) * t[1] if critic else 0.0)
    std = float(m64["stats"][8])
    return [loss] + t + [max(abs(float(m64["stats"][7])), std), std]


def _check_rows_and_stats(rows, stats, m32, m64, kw, what, worst):
    critic = m64["rows"]["value"] is not None
    for k in ("g_logp", "g_value") if critic else ("g_logp",):
        want, got = m64["rows"][k], rows[k].astype(np.float64)
        top = float(np.abs(want).max())
        tol = 8.0 * float(np.abs(m32["rows"][k].astype(np.float64) - want).max()) + 1e-6 * (1.0 + top)
        err = float(np.abs(got - want).max())
        worst.append((err / tol, err, tol, top, what, k))
        assert tol <= 0.01 * top, (what, k, tol, top)
        assert err <= tol, (what, k, err, tol)
    mags = _magnitudes(m64, kw, critic)
    for k, name in enumerate(STATS):
        want, got = float(m64["stats"][k]), float(stats[k])
        if k >= 9 or mags[k] == 0.0:  # bad_rows, the reserved zeros, value_loss without a critic, the advantage statistics when off
            assert got == want, (what, name, got, want)
            continue
        tol = 8.0 * abs(float(m32["stats"][k]) - want) + 1e-6 * (1.0 + abs(want))
        err = abs(got - want)
        worst.append((err / tol, err, tol, mags[k], what, name))
        assert tol <= 0.01 * mags[k], (what, name, tol, mags[k])
        assert err <= tol, (what, name, err, tol)


def _model_case(env_id, hidden, n_hidden, activation, n, kw, worst, critic=True, index=True):
    env, h, pol, _, batch, host = _rollout(env_id, hidden, n_hidden, activation, critic=critic)
    idx = _index(n, 5 * n + hidden) if index else None
    rows = _row_outputs(n if index else K * B, critic)
    grads, stats = env.ppo_grad_torch(h, batch, _dev(idx) if index else None, rows=rows, **kw)
    got = _grads_np(grads)
    rows_np = dict(zip(rows, _np(*rows.values())))
    stats = _np(stats)[0]
    m64 = ppo(pol, host, idx, activation=activation, **kw)
    m32 = ppo(pol, host, idx, activation=activation, dtype=np.float32, **kw)
    what = (env_id, hidden, n_hidden, activation, n, critic, tuple(sorted(kw)))
    _check_rows_and_stats(rows_np, stats, m32, m64, kw, what, worst)
    _check_grads(got, flat(m32), flat(m64), what, worst)
    env.check_status()
    return m64


@pytest.mark.parametrize("n", [200, 2049])
@pytest.mark.parametrize("hidden,n_hidden,activation", [(64, 2, "tanh"), (33, 1, "relu")])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_rows_statistics_and_gradients_equal_the_model(env_id, hidden, n_hidden, activation, n):
    """2: the per-row g_logp / g_value, the twelve statistics and every gradient against the float64 model"""
    worst = []
    m64 = _model_case(env_id, hidden, n_hidden, activation, n, KW, worst)
    print("branches: unclipped policy term %.2f, unclipped value square %.2f of the rows" % (m64["pg_unclipped"].mean(), m64["v_unclipped"].mean()))
    assert 0 < m64["pg_unclipped"].mean() < 1 and 0 < m64["v_unclipped"].mean() < 1
    _report(worst)


def test_first_epoch_has_ratio_one():
    """3: on the discrete id, with old_logp as policy_act_torch stored it and unchanged parameters, the ratio is exactly 1"""
    env, h, pol, _, batch, host = _rollout(DISCRETE, 64, 2, "tanh", moved=False)
    n = 700
    index = _index(n, 9)
    rows = _row_outputs(n)
    grads, stats = env.ppo_grad_torch(h, batch, _dev(index), normalize_advantage=False, rows=rows, **KW)
    r_logp, r_gl, s = _np(rows["logp"], rows["g_logp"], stats)
    assert r_logp.tobytes() == host["logp"][index].tobytes()  # lr = 0, ratio = 1
    assert s[4] == 0 and s[5] == 0 and s[6] == 0 and s[7] == 0 and s[8] == 0 and s[9] == 0
    want = -host["advantage"][index] / np.float32(n)
    assert want.dtype == np.float32 and np.abs(want).max() > 0 and r_gl.tobytes() == want.tobytes()
    env.check_status()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_one_update_equals_eager_torch(env_id):
    """4: the same update on the float32 CUDA modules with the loss in torch and backward(): the gradients agree within test 2's
    tolerances; the helper hands the fused call's tensors to the parameters"""
    import torch
    env, h, pol, (actor, critic, log_std), batch, host = _rollout(env_id, 64, 2, "tanh")
    n = 777
    index = _index(n, 21)
    d_index = _dev(index)
    grads, stats = env.ppo_grad_torch(h, batch, d_index, **KW)
    got = _grads_np(grads)
    params = [p for net in (actor, critic) for p in net.parameters()] + ([log_std] if log_std is not None else [])
    for p in params:
        p.grad = None
    x = batch["obs"][d_index]
    head = actor(x)
    if env.discrete:
        dist = torch.distributions.Categorical(logits=head)
        logp, ent = dist.log_prob(batch["action"][d_index].long()), dist.entropy()
    else:
        dist = torch.distributions.Normal(head, log_std.exp().expand_as(head))
        logp, ent = dist.log_prob(batch["action"][d_index]).sum(1), dist.entropy().sum(1)
    value = critic(x)[:, 0]
    lr = logp - batch["logp"][d_index]
    ratio = lr.exp()
    adv, ret, ov = batch["advantage"][d_index], batch["ret"][d_index], batch["value"][d_index]
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    vl = 0.5 * torch.max((value - ret) ** 2, (ov + torch.clamp(value - ov, -0.2, 0.2) - ret) ** 2).mean()
    loss = pg - 0.01 * ent.mean() + 0.5 * vl
    loss.backward()
    eager = flat(dict(actor=[(w.grad.cpu().numpy(), b.grad.cpu().numpy()) for w, b in _pairs(actor)],
                      critic=[(w.grad.cpu().numpy(), b.grad.cpu().numpy()) for w, b in _pairs(critic)],
                      log_std=log_std.grad.cpu().numpy() if log_std is not None else None))
    m64, m32 = flat(ppo(pol, host, index, **KW)), flat(ppo(pol, host, index, dtype=np.float32, **KW))
    tol = grad_tolerances(m32, m64)
    worst = []
    assert set(got) == set(eager) == set(m64)
    for k in m64:
        err = float(np.abs(got[k].astype(np.float64) - eager[k]).max())
        worst.append((err / tol[k], err, tol[k], float(np.abs(m64[k]).max()), (env_id, "eager"), k))
        assert tol[k] <= 0.01 * np.abs(m64[k]).max() and err <= tol[k], (k, err, tol[k])
    _report(worst)
    s = _np(stats)[0]
    assert abs(s[0] - float(loss.detach())) <= 1e-4 * (1 + abs(float(loss.detach())))
    for p in params:
        p.grad = None
    env.ppo_assign_grads(h, grads)
    flat_grads = [t for pair in grads["actor"] + grads["critic"] for t in pair] + ([grads["log_std"]] if log_std is not None else [])
    assert all(p.grad is g for p, g in zip(params, flat_grads))
    for p in params:
        p.grad = None
    env.check_status()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_two_calls_give_the_same_bits_and_every_output_is_overwritten(env_id):
    """5: determinism; outputs, row outputs, statistics and the workspace pre-filled with NaN hold no NaN afterwards"""
    import torch
    env, h, pol, _, batch, host = _rollout(env_id, 64, 2, "tanh")
    n = 2049
    d_index = _dev(_index(n, 31))
    rows = _row_outputs(n)
    grads, stats = env.ppo_grad_torch(h, batch, d_index, rows=rows, **KW)
    a, a_rows, a_stats = _grads_np(grads), dict(zip(rows, _np(*rows.values()))), _np(stats)[0]
    h.workspace.fill_(255)  # every float of it a NaN
    for t in [x for pairs in (grads["actor"], grads["critic"]) for pair in pairs for x in pair] + list(rows.values()) + [stats] + (
            [grads["log_std"]] if grads["log_std"] is not None else []):
        t.fill_(float("nan"))
    again, stats2 = env.ppo_grad_torch(h, batch, d_index, out=grads, stats=stats, rows=rows, **KW)
    assert again is grads and stats2 is stats
    b, b_rows, b_stats = _grads_np(again), dict(zip(rows, _np(*rows.values()))), _np(stats2)[0]
    _assert_same_bits(a, b, env_id)
    _assert_same_bits(a_rows, b_rows, env_id)
    assert a_stats.tobytes() == b_stats.tobytes() and not np.isnan(b_stats).any() and b_stats[10] == 0 and b_stats[11] == 0
    assert not any(np.isnan(v).any() for v in list(b.values()) + list(b_rows.values()))
    env.check_status()


def test_no_index_is_the_identity_index():
    import torch
    env, h, pol, _, batch, host = _rollout(GOAL, 33, 1, "relu")
    rows = K * B
    g0, s0 = env.ppo_grad_torch(h, batch, **KW)
    a, sa = _grads_np(g0), _np(s0)[0]
    g1, s1 = env.ppo_grad_torch(h, batch, torch.arange(rows, device="cuda"), **KW)
    b, sb = _grads_np(g1), _np(s1)[0]
    _assert_same_bits(a, b, "index=None")
    assert sa.tobytes() == sb.tobytes()
    env.check_status()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_a_policy_without_a_critic(env_id):
    """5: vf_coef is ignored, value_loss is 0, ret and value are not needed; rows, statistics and the actor's gradients against the model"""
    worst = []
    _model_case(env_id, 64, 2, "tanh", 200, dict(ent_coef=0.01, vf_coef=123.0), worst, critic=False)
    env, h, pol, _, batch, host = _rollout(env_id, 64, 2, "tanh", critic=False)
    few = {k: batch[k] for k in ("obs", "action", "logp", "advantage")}
    d_index = _dev(_index(200, 5 * 200 + 64))
    g0, s0 = env.ppo_grad_torch(h, batch, d_index, ent_coef=0.01, vf_coef=123.0)
    g1, s1 = env.ppo_grad_torch(h, few, d_index, ent_coef=0.01, vf_coef=0.0)
    assert g0["critic"] is None and g1["critic"] is None
    _assert_same_bits(_grads_np(g0), _grads_np(g1), env_id)
    sa, sb = _np(s0, s1)
    assert sa.tobytes() == sb.tobytes() and sa[2] == 0
    _report(worst)


@pytest.mark.parametrize("kw", [dict(normalize_advantage=False, ent_coef=0.01), dict(clip_range=float("inf"), vf_coef=1.0)],
                         ids=["raw_advantage", "no_clipping"])
def test_other_configurations_equal_the_model(kw):
    """5: normalize_advantage=False (adv_mean and adv_std are 0), and clip_range = inf with an unclipped value term, on all rows in order"""
    worst = []
    m64 = _model_case(GOAL, 33, 1, "relu", K * B, kw, worst, index=False)
    if "clip_range" in kw:
        assert m64["pg_unclipped"].all() and m64["stats"][6] == 0
    _report(worst)


@pytest.mark.parametrize("normalize_advantage", [True, False], ids=["normalized", "raw_advantage"])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_indices_outside_the_rows_are_clamped_counted_and_contribute_nothing(env_id, normalize_advantage):
    """5: indices outside the rows (the clamped, defined case of the contract) in four entries of the minibatch: counted in bad_rows,
    their per-row g_logp / g_value exactly 0, and rows, statistics and gradients against the model on the same index within test 2's
    tolerances; which way and how far outside is all the same to every output; without those entries bad_rows is 0"""
    env, h, pol, _, batch, host = _rollout(env_id, 64, 2, "tanh")
    n, rows_total = 200, K * B
    kw = dict(KW, normalize_advantage=normalize_advantage)
    index = _index(n, 61)
    where = [0, 7, 131, 199]  # in both row tiles of R = 128

    def run(idx):
        rows = _row_outputs(len(idx))
        grads, stats = env.ppo_grad_torch(h, batch, _dev(idx), rows=rows, **kw)
        return _grads_np(grads), _np(stats)[0], dict(zip(rows, _np(*rows.values())))

    bad = index.copy()
    bad[where] = [-1, rows_total, -2 ** 40, 2 ** 40]
    got, stats, r = run(bad)
    what = (env_id, n, normalize_advantage, "bad index")
    assert stats[9] == 4 and np.isfinite(stats).all(), (what, stats)
    assert not r["g_logp"][where].any() and not r["g_value"][where].any() and r["g_logp"].any() and r["g_value"].any(), what
    m64, m32 = ppo(pol, host, bad, **kw), ppo(pol, host, bad, dtype=np.float32, **kw)
    assert m64["stats"][9] == 4
    worst = []
    _check_rows_and_stats(r, stats, m32, m64, kw, what, worst)
    _check_grads(got, flat(m32), flat(m64), what, worst)
    _report(worst)
    # each entry stays on its side of the rows, so it is clamped to the same row: every output has the same bits
    other = index.copy()
    other[where] = [-7, rows_total + 5, np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    got2, stats2, r2 = run(other)
    _assert_same_bits(got, got2, what)
    _assert_same_bits(r, r2, what)
    assert stats.tobytes() == stats2.tobytes(), (what, stats, stats2)
    clean = np.delete(index, where)
    got3, stats3, r3 = run(clean)
    assert len(clean) == n - 4 and stats3[9] == 0 and np.isfinite(stats3).all(), (what, stats3)
    assert any(got3[k].tobytes() != got[k].tobytes() for k in got)
    env.check_status()


def test_a_captured_update_replays_the_eager_results():
    """5: captured after a warm-up call that sizes the workspace; without one the call raises inside the capture and launches nothing"""
    import torch
    env, h, pol, nets, batch, host = _rollout(GOAL, 64, 2, "tanh")
    n = 2049
    d_index = _dev(_index(n, 41))
    eager, stats = env.ppo_grad_torch(h, batch, d_index, **KW)
    want, want_stats = _grads_np(eager), _np(stats)[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream
        out, s_out = env.ppo_grad_torch(h, batch, d_index, **KW)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        env.ppo_grad_torch(h, batch, d_index, out=out, stats=s_out, **KW)
    every = [x for pairs in (out["actor"], out["critic"]) for pair in pairs for x in pair] + [out["log_std"], s_out]
    for _ in range(2):
        for t in every:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        _assert_same_bits(want, _grads_np(out), "replay")
        assert want_stats.tobytes() == _np(s_out)[0].tobytes()
    actor, critic, log_std = nets
    h2 = env.policy_torch(actor=_pairs(actor), critic=_pairs(critic), log_std=log_std)
    for t in every:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.ppo_grad_torch(h2, batch, d_index, out=out, stats=s_out, **KW)
    torch.cuda.synchronize()
    assert h2.workspace is None and all(t.isnan().all() for t in every)
    env.check_status()


def test_native_refusals():
    """5: every refusal returns the error with its message and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    env, h, pol, nets, batch, host = _rollout(GOAL, 64, 2, "tanh")
    actor, critic, log_std = nets
    h_nc = env.policy_torch(actor=_pairs(actor), log_std=log_std)
    n, rows = 40, K * B
    d_index = _dev(_index(n, 51))
    full, stats = env.ppo_grad_torch(h, batch, d_index, **KW)
    every = [x for pairs in (full["actor"], full["critic"]) for pair in pairs for x in pair] + [full["log_std"], stats]
    for t in every:
        t.fill_(7.0)
    lib, s, ws = env._lib, env._stream(), h.workspace
    need = lib.sg_ppo_grad_workspace_bytes(env._h, C.byref(h.struct), n)
    params = lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), n)
    assert need == (params + 7) // 8 * 8 + 8 * 2 * 256 + 4 * 8 and need <= ws.numel()  # the advantage partials, one workgroup's sums
    assert lib.sg_ppo_grad_workspace_bytes(env._h, C.byref(h.struct), 0) == 0 and b"n must be" in lib.sg_last_error(env._h)

    def grads_struct(critic=True):
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        for l, (w, b) in enumerate(full["actor"]):
            g.actor.weight[l], g.actor.bias[l] = w.data_ptr(), b.data_ptr()
        if critic:
            for l, (w, b) in enumerate(full["critic"]):
                g.critic.weight[l], g.critic.bias[l] = w.data_ptr(), b.data_ptr()
        g.log_std = full["log_std"].data_ptr()
        return g

    def refused(match, policy=h, cfg=(), drop=(), n_rows=rows, count=n, g="given", st=stats, row_out=None, w=ws, wbytes=None, index=d_index,
                no_batch=False, no_cfg=False):
        c = _native.SgPpoConfig()
        lib.sg_ppo_config_init(C.byref(c))
        c.clip_range_vf, c.ent_coef = 0.2, 0.01
        for k, v in cfg:
            setattr(c, k, v)
        cols = dict(obs=batch["obs"], action=batch["action"], old_logp=batch["logp"], advantage=batch["advantage"], ret=batch["ret"],
                    old_value=batch["value"], index=index)
        b = _native.SgPpoBatch(**{k: (v.data_ptr() if v is not None and k not in drop else None) for k, v in cols.items()})
        gs = grads_struct(critic=policy is h) if g == "given" else g
        rc = lib.sg_ppo_grad_device(env._h, C.byref(policy.struct), None if no_cfg else C.byref(c), None if no_batch else C.byref(b), n_rows, count,
                                    C.byref(gs) if gs is not None else None, C.c_void_p(st.data_ptr()) if st is not None else None,
                                    C.byref(row_out) if row_out is not None else None, C.c_void_p(w.data_ptr()) if w is not None else None,
                                    ws.numel() if wbytes is None else wbytes, s)
        assert rc == -1 and match in lib.sg_last_error(env._h), (match, rc, lib.sg_last_error(env._h))

    assert C.sizeof(_native.SgPpoConfig) == 32
    refused(b"null cfg", no_cfg=True)
    refused(b"struct_size", cfg=[("struct_size", 28)])
    refused(b"reserved", cfg=[("reserved", 1)])
    refused(b"clip_range must be > 0", cfg=[("clip_range", 0.0)])
    refused(b"clip_range must be > 0", cfg=[("clip_range", float("nan"))])
    refused(b"needs batch.old_value", drop=("old_value",))
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
    refused(b"without an index", drop=("index",), count=rows + 1)
    refused(b"null stats_out", st=None)
    refused(b"null grads", g=None)
    refused(b"of the critic", g=grads_struct(critic=False))
    refused(b"null workspace", w=None)
    refused(b"workspace of", wbytes=need - 1)
    refused(b"critic gradients given", policy=h_nc, g=grads_struct())
    r = _native.SgPpoRows(value=stats.data_ptr())
    refused(b"row_out.value / row_out.g_value given, but the policy has no critic", policy=h_nc, row_out=r)
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in every)
    env.ppo_grad_torch(h, batch, d_index, **KW)  # the handle still works
    torch.cuda.synchronize()
    env.check_status()
