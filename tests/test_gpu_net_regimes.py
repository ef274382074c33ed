"""GPU tests of every net family on the trained-regime cases of tests/net_regimes.py: saturated tanh units and mostly dead relu layers,
logits tens to hundreds apart (exp(logit - max) underflows, p log p is 0 x (-100)), log_std (-4, 1.5) with actions six sigma out, the
squashed actor at its default clamp (-20, 2) with actions that round to +-1, Q values in the hundreds.  The older files run freshly
initialised nets on unit-scale data only.

Nothing here has a rule of its own.  A forward quantity is held to test_gpu_policy._tol, 8 x max|float32 CPU - float64| + 1e-6, applied
PER STRATUM: the maxima are taken over the rows of each stratum the case names (and over all rows), so that one loose stratum does not
set the tolerance of the others; a stratum with fewer than net_regimes.STRATUM_ROWS rows is held with all rows only.  A gradient tensor is held to its model's grad_tolerances, 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|),
which must be at most 1 % of max|G64| (tests/test_net_regimes.py checks that cap, and the strata's occupancy, on the CPU for the very
inputs used here).  Populations and the fused PPO update are held to the single calls' bits.  n = 200 rows everywhere."""
import numpy as np
import pytest

import dqn_model
import net_regimes as R
import policy_grad_model
import policy_model
import q_model
import squashed_model
import test_gpu_dqn as gpu_dqn
import test_gpu_policy_grad as gpu_policy_grad
import test_gpu_population as gpu_population
import test_gpu_ppo as gpu_ppo
import test_gpu_q as gpu_q
import test_gpu_squashed as gpu_squashed
from net_widths import OBS_DIM
from population_model import bit_equal_to_single, flat_member, grad_rows, stack
from test_gpu_policy import _dev, _handle, _np, _tol, make

pytestmark = pytest.mark.gpu

N = R.N
BASE = 1000  # env_index_base: the noise is keyed by the global env index
NOISE = dict(seed=77, step=2 ** 32 + 5)
KINDS = ["continuous", "discrete"]
_records = []  # (ratio, error, tolerance, magnitude, what, name) of every quantity held to a tolerance, for the last test


def _env(env_id, n=N):
    env = make(env_id, n, env_index_base=BASE)
    assert env.obs_dim == OBS_DIM[env_id]
    return env


def _forward(worst, got, m32, m64, strata, what, name):
    """a forward quantity under _tol over all rows and over the rows alone of each stratum that has at least R.STRATUM_ROWS of them"""
    got, m64 = np.asarray(got, np.float64), np.asarray(m64, np.float64)
    assert np.isfinite(got).all(), (what, name)
    for stratum, rows in [("all", np.ones(got.shape[0], bool))] + [(k, v) for k, v in strata.items() if v.sum() >= R.STRATUM_ROWS]:
        tol, err = _tol(np.asarray(m32)[rows], m64[rows]), float(np.abs(got[rows] - m64[rows]).max())
        worst.append((err / tol, err, tol, float(np.abs(m64[rows]).max()), what, "%s [%s, %d rows]" % (name, stratum, int(rows.sum()))))
        assert err <= tol, (what, name, stratum, err, tol)


def _tensors(out):
    """the tensors of a result: a tensor, a tuple / list or a dict of results; None left out"""
    if out is None:
        return []
    if isinstance(out, dict):
        return [t for v in out.values() for t in _tensors(v)]
    if isinstance(out, (tuple, list)):
        return [t for v in out for t in _tensors(v)]
    return [out]


def _poison(t):
    t.fill_(float("nan") if t.is_floating_point() else -1)


def _same_bits_into_poisoned_outputs(call, first, names, what):
    """forward calls: a second call into NaN-prefilled (integers: -1) outputs gives the first call's bits and leaves no NaN"""
    import torch
    torch.cuda.synchronize()
    out = {k: torch.empty_like(t) for k, t in zip(names, first) if t is not None}
    for t in out.values():
        _poison(t)
    again = call(out)
    torch.cuda.synchronize()
    for k, a, b in zip(names, first, again):
        if a is not None:
            assert b.data_ptr() == out[k].data_ptr() and torch.equal(a, b) and not (b.is_floating_point() and b.isnan().any()), (what, k)


def _same_bits_again(call, h, first, what):
    """gradient calls: the first result's tensors and the handle's workspace NaN-prefilled, a second call into them gives the same bits"""
    import torch
    torch.cuda.synchronize()
    keep = [t.clone() for t in _tensors(first)]
    h.workspace.view(torch.float32).fill_(float("nan"))
    for t in _tensors(first):
        _poison(t)
    again = call(first)
    torch.cuda.synchronize()
    now = _tensors(again)
    assert len(now) == len(keep) > 0, what
    assert all(torch.equal(a, b) and not b.isnan().any() for a, b in zip(keep, now)), what


def _finish(worst, report):
    _records.extend(worst)
    report(worst)


@pytest.mark.parametrize("hidden,n_hidden,activation", R.cases())
@pytest.mark.parametrize("kind", KINDS)
def test_policy(kind, hidden, n_hidden, activation):
    """policy_act_torch, deterministic and drawn, and policy_evaluate_raw_torch on act's own action (value and the discrete logp are
    act's bits) and on the case's actions (six sigma out; uniform over the six, so unlikely actions are scored) against the float64
    model per stratum; the greedy argmax on the clear rows and the categorical draw away from the boundaries; policy_grad_torch with
    the three g together and each alone"""
    env_id = R.ids_of(hidden, n_hidden)[KINDS.index(kind)]
    c = R.case("policy", env_id, hidden, n_hidden, activation)
    pol, obs, strata = c["policy"], c["obs"], c["strata"]
    env = _env(env_id)
    continuous = not env.discrete
    h = _handle(env, pol, activation)
    d_obs = _dev(obs)
    what, worst = ("policy", env_id, hidden, n_hidden, activation), []
    m64 = policy_model.act(pol, obs, env_index_base=BASE, activation=activation, **NOISE)
    m32 = policy_model.act(pol, obs, env_index_base=BASE, activation=activation, dtype=np.float32, **NOISE)
    a_det, lp_det, v = _np(*env.policy_act_torch(h, d_obs, deterministic=True, **NOISE))
    drawn = env.policy_act_torch(h, d_obs, **NOISE)
    _same_bits_into_poisoned_outputs(lambda out: env.policy_act_torch(h, d_obs, out=out, **NOISE), drawn, ("action", "logp", "value"), what)
    action, logp_act, value_act = drawn
    a, lp, v2 = _np(action, logp_act, value_act)
    _forward(worst, v, m32["value"], m64["value"], strata, what, "value")
    assert np.array_equal(v, v2), what
    if continuous:
        _forward(worst, a_det, m32["mean"], m64["mean"], strata, what, "mean")
        _forward(worst, lp, m32["logp"], m64["logp"], strata, what, "logp")
        d64 = policy_model.act(pol, obs, deterministic=True, activation=activation)["logp"]
        d32 = policy_model.act(pol, obs, deterministic=True, activation=activation, dtype=np.float32)["logp"]
        _forward(worst, lp_det, d32, d64, strata, what, "logp (deterministic)")
        std = np.exp(pol["log_std"].astype(np.float64))
        eps32 = (m32["action"].astype(np.float64) - m32["mean"].astype(np.float64)) / std  # recovered as from the device
        _forward(worst, (a.astype(np.float64) - a_det.astype(np.float64)) / std, eps32, m64["eps"], strata, what, "eps")
    else:
        t = _tol(m32["logits"], m64["logits"])
        top = np.sort(m64["logits"], axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * t  # (an argmax within the tolerance of a tie may go either way)
        assert clear.mean() >= 0.9 and np.array_equal(a_det[clear], m64["logits"].argmax(axis=1)[clear]), what
        for acts, logp in ((a_det, lp_det), (a, lp)):  # logp at the device's own action
            assert acts.dtype == np.int32 and acts.min() >= 0 and acts.max() <= 5
            s32 = policy_model.act(pol, obs, activation=activation, dtype=np.float32, action=acts)["logp"]
            s64 = policy_model.act(pol, obs, activation=activation, action=acts)["logp"]
            _forward(worst, logp, s32, s64, strata, what, "logp at its own action")
        # the draw, by tests/test_gpu_policy.py's rule: the model's action wherever u * total is farther than 1e-5 * total from every
        # running sum (which here stands still over the actions whose exp underflows); at most 1 % of the draws may be that close
        compared = left_out = 0
        for step in range(4):
            m = policy_model.act(pol, obs, seed=3, step=step, env_index_base=BASE, activation=activation)
            drew, = _np(env.policy_act_torch(h, d_obs, seed=3, step=step)[0])
            far = (np.abs(m["cum"] - m["want"][:, None]) > 1e-5 * m["total"][:, None]).all(axis=1)
            assert np.array_equal(drew[far], m["action"][far]), (what, step)
            compared, left_out = compared + int(far.sum()), left_out + int((~far).sum())
        assert left_out <= 0.01 * (compared + left_out), (what, left_out)
    # evaluate on act's own action
    own = env.policy_evaluate_raw_torch(h, d_obs, action)
    _same_bits_into_poisoned_outputs(lambda out: env.policy_evaluate_raw_torch(h, d_obs, action, out=out), own, ("logp", "entropy", "value"), what)
    logp, entropy, value = _np(*own)
    assert np.array_equal(value, v), what
    e64 = policy_grad_model.evaluate(pol, obs, a, activation=activation, grads=False)
    e32 = policy_grad_model.evaluate(pol, obs, a, activation=activation, grads=False, dtype=np.float32)
    if continuous:
        _forward(worst, logp, e32["logp"], e64["logp"], strata, what, "evaluate logp at act's action")
    else:
        assert np.array_equal(logp, lp), what  # the PPO ratio of the first minibatch is exactly 1
    _forward(worst, entropy, e32["entropy"], e64["entropy"], strata, what, "entropy")
    # evaluate on the case's actions
    d_action = _dev(c["action"])
    logp, entropy2, value = _np(*env.policy_evaluate_raw_torch(h, d_obs, d_action))
    f64, f32 = R.forward_models("policy", c, activation, np.float64), R.forward_models("policy", c, activation, np.float32)
    _forward(worst, logp, f32["logp"], f64["logp"], strata, what, "evaluate logp")
    assert np.array_equal(value, v) and np.array_equal(entropy2, entropy), what
    g = c["g"]
    for sel in ("all", "logp", "entropy", "value"):
        use = {k: (_dev(g[k]) if sel in ("all", k) else None) for k in g}
        call = lambda out=None: env.policy_grad_torch(h, d_obs, d_action, g_logp=use["logp"], g_entropy=use["entropy"], g_value=use["value"], out=out)
        out = call()
        reference = R.policy_reference if sel == "all" else (lambda c_, a_, d_: R.policy_reference_of(c_, a_, d_, sel))
        g64, g32 = reference(c, activation, np.float64), reference(c, activation, np.float32)
        if use["value"] is None:  # the critic's slots are not in use
            assert out["critic"] is None
            g64 = {k: x for k, x in g64.items() if not k.startswith("critic")}
        gpu_policy_grad._check_grads(gpu_policy_grad._grads_np(out), g32, g64, what + (sel,), worst)
        if sel == "all":
            _same_bits_again(call, h, out, what)
    _finish(worst, gpu_policy_grad._report)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", R.cases())
def test_q(hidden, n_hidden, activation):
    """q_evaluate_raw_torch against the model per stratum; q_grad_torch(action_grad=True) with both critics; the actor chain: the action
    without eps is the deterministic act's bits, with eps within _tol per stratum, its gradients against the model"""
    env_id = R.ids_of(hidden, n_hidden)[0]
    c = R.case("q", env_id, hidden, n_hidden, activation)
    env = _env(env_id)
    what, worst = ("q", env_id, hidden, n_hidden, activation), []
    d_obs, d_act = _dev(c["obs"]), _dev(c["action"])
    h = gpu_q._q_handle(env, c["critics"], activation)
    first = env.q_evaluate_raw_torch(h, d_obs, d_act)
    _same_bits_into_poisoned_outputs(lambda out: env.q_evaluate_raw_torch(h, d_obs, d_act, out=out), first, ("q1", "q2"), what)
    q = _np(*first)
    m64, m32 = R.forward_models("q", c, activation, np.float64), R.forward_models("q", c, activation, np.float32)
    for got, k in zip(q, ("q1", "q2")):
        _forward(worst, got, m32[k], m64[k], c["strata"], what, k)
    assert max(np.abs(q[0]).max(), np.abs(q[1]).max()) >= 100
    call = lambda out=None: env.q_grad_torch(h, d_obs, d_act, _dev(c["g"][0]), _dev(c["g"][1]), action_grad=True, out=out)
    out = call()
    got = gpu_q._q_grads_np(out)
    got["action"] = out["action"].cpu().numpy()
    gpu_q._check_grads(got, R.q_reference(c, activation, np.float32), R.q_reference(c, activation, np.float64), what + ("q_grad",), worst)
    _same_bits_again(call, h, out, what)
    # the actor chain
    pol, eps, ga = c["policy"], c["eps"], c["g_action"]
    hp = _handle(env, pol, activation)
    det = _np(env.policy_act_torch(hp, d_obs, deterministic=True)[0])[0]
    assert _np(env.policy_action_raw_torch(hp, d_obs))[0].tobytes() == det.tobytes(), what
    a = _np(env.policy_action_raw_torch(hp, d_obs, _dev(eps)))[0]
    _forward(worst, a, m32["action"], m64["action"], c["actor_strata"], what, "action")
    call = lambda out=None: env.policy_action_grad_torch(hp, d_obs, _dev(ga), _dev(eps), out=out)
    out = call()
    got = q_model.flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]], log_std=out["log_std"].cpu().numpy()))
    gpu_q._check_grads(got, R.actor_chain_reference(c, activation, np.float32), R.actor_chain_reference(c, activation, np.float64),
                       what + ("action_grad",), worst)
    _same_bits_again(call, hp, out, what)
    _finish(worst, gpu_q._report)
    env.check_status()
    env.close()


def _squashed_strata(c, m32):
    """the case's strata with unit_action read off this call's float32 model action (the noise is the call's)"""
    strata = {k: v for k, v in c["strata"].items() if k not in ("unit_action", "plain")}
    strata["unit_action"] = (np.abs(m32["action"]) == 1).any(axis=1)
    return R.with_plain(strata)


@pytest.mark.parametrize("hidden,n_hidden,activation", R.cases())
def test_squashed(hidden, n_hidden, activation):
    """at the default clamp (-20, 2): squashed_act_torch (drawn and deterministic, against squashed_model.act) and
    squashed_sample_raw_torch with the caller's eps against the model per stratum; every output finite, |a| <= 1, some action component
    exactly +-1 with a finite logp on its row; a sample without eps is the deterministic act's bits; squashed_grad_torch under each
    selection"""
    env_id = R.ids_of(hidden, n_hidden)[0]
    c = R.case("squashed", env_id, hidden, n_hidden, activation)
    env = _env(env_id)
    what, worst = ("squashed", env_id, hidden, n_hidden, activation), []
    actor, obs, bounds = c["actor"], c["obs"], R.SQUASHED_BOUNDS
    h = gpu_squashed._handle(env, actor, activation, bounds=bounds)
    d_obs, d_eps = _dev(obs), _dev(c["eps"])
    units = 0
    for det in (False, True):
        first = env.squashed_act_torch(h, d_obs, deterministic=det, **NOISE)
        _same_bits_into_poisoned_outputs(lambda out: env.squashed_act_torch(h, d_obs, deterministic=det, out=out, **NOISE), first, ("action", "logp"), what)
        a, lp = _np(*first)
        m64 = squashed_model.act(actor, obs, env_index_base=BASE, deterministic=det, bounds=bounds, activation=activation, **NOISE)
        m32 = squashed_model.act(actor, obs, env_index_base=BASE, deterministic=det, bounds=bounds, activation=activation, dtype=np.float32, **NOISE)
        strata = _squashed_strata(c, m32)
        for k, got in (("action", a), ("logp", lp)):
            _forward(worst, got, m32[k], m64[k], strata, what, "act %s%s" % (k, " (deterministic)" if det else ""))
        unit = (np.abs(a) == 1).any(axis=1)
        assert np.abs(a).max() <= 1 and np.isfinite(lp).all() and np.isfinite(lp[unit]).all(), what
        units += int(unit.sum())
        if det:
            s_a, s_lp = _np(*env.squashed_sample_raw_torch(h, d_obs))
            assert s_a.tobytes() == a.tobytes() and s_lp.tobytes() == lp.tobytes(), what
    first = env.squashed_sample_raw_torch(h, d_obs, d_eps)
    _same_bits_into_poisoned_outputs(lambda out: env.squashed_sample_raw_torch(h, d_obs, d_eps, out=out), first, ("action", "logp"), what)
    a, lp = _np(*first)
    m64, m32 = R.forward_models("squashed", c, activation, np.float64), R.forward_models("squashed", c, activation, np.float32)
    for k, got in (("action", a), ("logp", lp)):
        _forward(worst, got, m32[k], m64[k], c["strata"], what, "sample " + k)
    unit = (np.abs(a) == 1).any(axis=1)
    units += int(unit.sum())
    assert np.abs(a).max() <= 1 and np.isfinite(lp).all() and units > 0, (what, units)
    print("rows with an action component of exactly +-1, over the three calls:", units, what)
    d_ga, d_gl = _dev(c["g_action"]), _dev(c["g_logp"])
    for sel in squashed_model.SELECTIONS:
        ga = d_ga if sel in ("both", "action") else None
        gl = d_gl if sel in ("both", "logp") else None
        call = lambda out=None: env.squashed_grad_torch(h, d_obs, d_eps, ga, gl, out=out)
        out = call()
        gpu_squashed._check_grads(gpu_squashed._grads_np(out), R.squashed_reference(c, activation, np.float32, sel),
                                  R.squashed_reference(c, activation, np.float64, sel), what + (sel,), worst)
        _same_bits_again(call, h, out, what + (sel,))
    _finish(worst, gpu_squashed._report)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", R.cases())
def test_dqn(hidden, n_hidden, activation):
    """Q values in the hundreds: dqn_evaluate_raw_torch's q_all, q_taken and q_max against the model per stratum, q_taken / q_max / argmax
    from the kernel's own q_all on every row, the model's argmax on the clear rows; the greedy dqn_act_torch; dqn_grad_torch under each
    selection"""
    import torch
    env_id = R.ids_of(hidden, n_hidden)[1]
    c = R.case("dqn", env_id, hidden, n_hidden, activation)
    env = _env(env_id)
    assert env.discrete
    what, worst = ("dqn", env_id, hidden, n_hidden, activation), []
    net, obs = c["net"], c["obs"]
    h = gpu_dqn._handle(env, net, activation)
    d_obs, d_action = _dev(obs), _dev(c["action"])
    q_all, argmax = gpu_dqn._check_discrete_outputs(env, h, d_obs, d_action, what)
    first = env.dqn_evaluate_raw_torch(h, d_obs, d_action)
    _same_bits_into_poisoned_outputs(lambda out: env.dqn_evaluate_raw_torch(h, d_obs, d_action, out=out), first, ("q_all", "q_taken", "q_max", "argmax"), what)
    m64, m32 = R.forward_models("dqn", c, activation, np.float64), R.forward_models("dqn", c, activation, np.float32)
    for k, got in zip(("q_all", "q_taken", "q_max"), _np(*first[:3])):
        _forward(worst, got, m32[k], m64[k], c["strata"], what, k)
    assert np.abs(_np(q_all)[0]).max() >= 100
    top = np.sort(m64["q_all"], axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * _tol(m32["q_all"], m64["q_all"])  # (an argmax within the tolerance of a tie may go either way)
    assert clear.mean() >= 0.9 and np.array_equal(_np(argmax)[0][clear], dqn_model.first_argmax(m64["q_all"])[clear]), what
    greedy = env.dqn_act_torch(h, d_obs, seed=5, step=9)  # epsilon 0
    _same_bits_into_poisoned_outputs(lambda out: env.dqn_act_torch(h, d_obs, seed=5, step=9, out=out), greedy, ("action", "q"), what)
    a, q = greedy
    assert torch.equal(a, argmax), what
    assert q.cpu().numpy().tobytes() == q_all.gather(1, argmax.long()[:, None])[:, 0].cpu().numpy().tobytes(), what
    d_gt, d_ga = _dev(c["g_taken"]), _dev(c["g_all"])
    for sel in dqn_model.SELECTIONS:
        gt = d_gt if sel in ("both", "taken") else None
        ga = d_ga if sel in ("both", "all") else None
        call = lambda out=None: env.dqn_grad_torch(h, d_obs, d_action, gt, ga, out=out)
        out = call()
        gpu_dqn._check_grads(gpu_dqn._grads_np(out), R.dqn_reference_of(c, activation, np.float32, sel),
                             R.dqn_reference_of(c, activation, np.float64, sel), what + (sel,), worst)
        _same_bits_again(call, h, out, what + (sel,))
    _finish(worst, gpu_dqn._report)
    env.check_status()
    env.close()


FUSED = (64, 2, "tanh")  # the case of the stacked and the fused paths


@pytest.mark.parametrize("kind", KINDS)
def test_population(kind):
    """P = 2 on the (64, 2) tanh case: member 0 is the case's policy on the case's rows, member 1 the same constructor's policy and rows
    under another seed.  population_evaluate_raw_torch and population_grad_torch are the single calls' bits on
    population_member_torch(pop, m)"""
    hidden, n_hidden, activation = FUSED
    P = 2
    env_id = R.ids_of(hidden, n_hidden)[KINDS.index(kind)]
    members = [R.case("policy", env_id, hidden, n_hidden, activation), R.policy_case(env_id, N + 1, hidden, n_hidden, activation)]
    assert bit_equal_to_single(N, grad_rows(hidden), P)
    env = _env(env_id)
    pop = stack([m["policy"] for m in members])
    h = gpu_population._pop_handle(env, pop, activation)
    what = (env_id, hidden, n_hidden, activation)
    d_obs = _dev(np.stack([m["obs"][:N] for m in members]))
    d_action = _dev(np.stack([m["action"][:N] for m in members]))
    got = _np(*env.population_evaluate_raw_torch(h, d_obs, d_action))
    assert all(x.shape == (P, N) and np.isfinite(x).all() for x in got)
    for m in range(P):
        want = _np(*env.policy_evaluate_raw_torch(env.population_member_torch(h, m), d_obs[m], d_action[m]))
        for name, x, w in zip(("logp", "entropy", "value"), got, want):
            assert x[m].tobytes() == w.tobytes(), (what, m, name)
    assert np.abs(got[2][0] - got[2][1]).max() > 1  # the members differ
    g = [_dev(np.stack([m["g"][k][:N] for m in members])) for k in ("logp", "entropy", "value")]
    stacked = gpu_population._stacked_np(env.population_grad_torch(h, d_obs, d_action, *g))
    for m in range(P):
        mine, want = flat_member(stacked, m), gpu_population._single_grads(env, h, m, d_obs, d_action, g)
        assert set(mine) == set(want) and all(np.isfinite(x).all() for x in mine.values()) and any(np.abs(x).max() > 0 for x in mine.values())
        for k in want:
            assert mine[k].tobytes() == want[k].tobytes(), (what, m, k)
    env.check_status()
    env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ppo(kind):
    """ppo_grad_torch on the (64, 2) tanh case's rows, the stored logp and value the float64 model's moved as tests/test_gpu_ppo.py moves
    them: the gradients are policy_grad_torch's bits on the same rows fed the per-row g_logp / g_value the kernel reports; its logp /
    value are policy_evaluate_raw_torch's bits; both branches of both max are taken"""
    import torch
    hidden, n_hidden, activation = FUSED
    env_id = R.ids_of(hidden, n_hidden)[KINDS.index(kind)]
    c = R.case("policy", env_id, hidden, n_hidden, activation)
    m64 = R.forward_models("policy", c, activation, np.float64)
    rng = np.random.default_rng([N + hidden, 2])
    host = dict(obs=c["obs"], action=c["action"], logp=(m64["logp"] + 0.05 + 0.3 * rng.standard_normal(N)).astype(np.float32),
                value=(m64["value"] + 0.3 * rng.standard_normal(N)).astype(np.float32), advantage=rng.standard_normal(N).astype(np.float32),
                ret=(m64["value"] + rng.standard_normal(N)).astype(np.float32))
    env = _env(env_id)
    h = _handle(env, c["policy"], activation)
    batch = {k: _dev(v) for k, v in host.items()}
    rows = gpu_ppo._row_outputs(N)
    grads, stats = env.ppo_grad_torch(h, batch, None, rows=rows, **gpu_ppo.KW)
    got = gpu_policy_grad._grads_np(grads)
    g_entropy = torch.full((N,), float(-np.float32(gpu_ppo.KW["ent_coef"]) / np.float32(N)), device="cuda")
    want = gpu_policy_grad._grads_np(env.policy_grad_torch(h, batch["obs"], batch["action"], g_logp=rows["g_logp"], g_entropy=g_entropy,
                                                           g_value=rows["g_value"]))
    what = (env_id, hidden, n_hidden, activation)
    gpu_ppo._assert_same_bits(got, want, what)
    assert all(np.isfinite(x).all() for x in got.values()) and any(np.abs(x).max() > 0 for x in got.values())
    logp, _, value = _np(*env.policy_evaluate_raw_torch(h, batch["obs"], batch["action"]))
    r_logp, r_value, r_gl, r_gv, s = _np(rows["logp"], rows["value"], rows["g_logp"], rows["g_value"], stats)
    assert r_logp.tobytes() == logp.tobytes() and r_value.tobytes() == value.tobytes(), what
    assert np.isfinite(s).all() and s[9] == 0 and np.isfinite(r_gl).all() and np.isfinite(r_gv).all(), what
    assert (r_gl == 0).any() and (r_gl != 0).any() and (r_gv == 0).any() and (r_gv != 0).any(), what
    env.check_status()
    env.close()


def test_report_the_worst_ratios():
    """prints the three worst error / tolerance ratios of this file's run, over everything and per family (nothing to hold: every
    quantity was asserted where it was measured)"""
    _records.sort(key=lambda r: r[0], reverse=True)
    assert all(r[0] <= 1 for r in _records)
    for family in ("all", "policy", "q", "squashed", "dqn"):
        for ratio, err, tol, top, what, k in [r for r in _records if family in ("all", r[4][0])][:3]:
            print("%s: error / tolerance %.3f (error %.3g, tolerance %.3g, magnitude %.3g) at" % (family, ratio, err, tol, top), what, k)
    print("quantities held to a tolerance:", len(_records))
