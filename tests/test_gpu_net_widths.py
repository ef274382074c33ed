"""GPU tests of every net family at the widths of tests/net_widths.py: each class NT = ceil(hidden / 32) of the four kernel
instantiations, each class's widest net (32 NT wide, three hidden layers, on the 4P ids with the widest observation), the widths whose
bias is the last column of an MFMA column tile (31, 127), and the 2P and 4P observation widths.  The older files run hidden 1, 5, 16,
33, 40, 64, 97 and 128 only, so the NT = 3 instantiation of every kernel template ran nowhere.

Nothing here has a rule of its own.  A forward quantity is held to test_gpu_policy._tol, 8 x max|float32 CPU - float64| + 1e-6; a
gradient tensor to its model's grad_tolerances, 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|), which must be at most 1 % of max|G64|
(tests/test_net_widths.py checks that cap on the CPU for the very inputs used here); populations and the fused PPO update to the
single calls' bits and, for PPO, to tests/test_gpu_ppo.py's own assertions.  n = 200 rows everywhere: two ragged forward workgroups for
classes 3 and 4, one partial one for classes 1 and 2; four ragged row tiles of the backward at R = 64, two at 128, one partial at 256.
Two more things are pinned per class: the workspace size through the ABI, and that the widest net of a 4P handle keeps running, with the
same bits, after a Kepler handle alive beside it has had the kernels' dynamic-LDS limits set for its narrower observation.

FAMILY_KERNELS says which kernel templates each family's test launches; tests/test_net_widths.py holds it against the compiled
engine, so a new net kernel fails the CPU suite until it is named here and its family's test runs it at these widths."""
import ctypes as C

import numpy as np
import pytest

import dqn_model
import policy_grad_model
import policy_model
import q_model
import squashed_model
import test_gpu_dqn as gpu_dqn
import test_gpu_policy_grad as gpu_policy_grad
import test_gpu_population as gpu_population
import test_gpu_population_ppo as gpu_population_ppo
import test_gpu_ppo as gpu_ppo
import test_gpu_q as gpu_q
import test_gpu_squashed as gpu_squashed
from net_widths import (BIG, GRAD_ROWS, N, NARROW_ID, OBS_DIM, TWO_HANDLE_WIDTHS, WIDE_ID, actor_chain_reference, cases, dqn_case,
                        dqn_reference, ids_of, policy_case, policy_reference, q_case, q_reference, squashed_case, squashed_reference,
                        tile_class)
from population_model import bit_equal_to_single, flat_member, grad_rows, random_population
from test_gpu_policy import _dev, _handle, _np, _tol, make

pytestmark = pytest.mark.gpu

FAMILY_KERNELS = {
    "policy": ("policy_act_kernel", "policy_evaluate_kernel", "policy_grad_kernel"),
    "q": ("q_evaluate_kernel", "q_grad_kernel", "policy_action_kernel", "policy_action_grad_kernel"),
    "squashed": ("squashed_act_kernel", "squashed_sample_kernel", "squashed_grad_kernel"),
    "dqn": ("dqn_act_kernel", "dqn_evaluate_kernel", "dqn_grad_kernel"),
    "population": ("population_act_kernel", "population_evaluate_kernel", "population_grad_kernel"),
    "ppo": ("ppo_grad_kernel",),
    "population_ppo": ("ppo_population_grad_kernel",),
}

BASE = 1000  # env_index_base: the noise is keyed by the global env index
NOISE = dict(seed=77, step=2 ** 32 + 5)
KINDS = ["continuous", "discrete"]
_ppo_keys, _population_ppo_keys = [], []  # the keys of the rollouts asked of the two PPO files' caches


def _env(env_id, n=N):
    env = make(env_id, n, env_index_base=BASE)
    assert env.obs_dim == OBS_DIM[env_id]
    return env


def _forward(worst, got, m32, m64, what, name):
    """a forward quantity under _tol, noted with the gradients' records"""
    tol, err = _tol(m32, m64), float(np.abs(got - m64).max())
    worst.append((err / tol, err, tol, float(np.abs(m64).max()), what, name))
    assert err <= tol, (what, name, err, tol)


def teardown_module(module):
    """the rollouts this file asked tests/test_gpu_ppo.py and tests/test_gpu_population_ppo.py to make are closed here"""
    for cache, keys in ((gpu_ppo._cache, _ppo_keys), (gpu_population_ppo._cache, _population_ppo_keys)):
        for key in keys:
            if key in cache:
                cache.pop(key)[0].close()
        keys.clear()


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
@pytest.mark.parametrize("kind", KINDS)
def test_policy(kind, hidden, n_hidden, activation):
    """policy_act_torch against the float64 model (the deterministic mean or argmax, value, logp at the call's own action);
    policy_evaluate_raw_torch on act's own action: value and the discrete logp are act's bits, entropy and the continuous logp within
    _tol; policy_grad_torch with dense g_logp, g_entropy and g_value together"""
    env_id = ids_of(hidden, n_hidden)[KINDS.index(kind)]
    c = policy_case(env_id, N, hidden, n_hidden)
    pol, obs = c["policy"], c["obs"]
    env = _env(env_id)
    continuous = not env.discrete
    h = _handle(env, pol, activation)
    d_obs = _dev(obs)
    what, worst = (env_id, hidden, n_hidden, activation), []
    m64 = policy_model.act(pol, obs, env_index_base=BASE, activation=activation, **NOISE)
    m32 = policy_model.act(pol, obs, env_index_base=BASE, activation=activation, dtype=np.float32, **NOISE)
    a_det, lp_det, v = _np(*env.policy_act_torch(h, d_obs, deterministic=True, **NOISE))
    action, logp_act, value_act = env.policy_act_torch(h, d_obs, **NOISE)
    a, lp, v2 = _np(action, logp_act, value_act)
    _forward(worst, v, m32["value"], m64["value"], what, "value")
    assert np.array_equal(v, v2), what
    if continuous:
        _forward(worst, a_det, m32["mean"], m64["mean"], what, "mean")
        _forward(worst, lp, m32["logp"], m64["logp"], what, "logp")
        std = np.exp(pol["log_std"].astype(np.float64))
        eps32 = (m32["action"].astype(np.float64) - m32["mean"].astype(np.float64)) / std  # recovered as from the device
        _forward(worst, (a.astype(np.float64) - a_det.astype(np.float64)) / std, eps32, m64["eps"], what, "eps")
    else:
        t = _tol(m32["logits"], m64["logits"])
        top = np.sort(m64["logits"], axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * t  # (an argmax within the tolerance of a tie may go either way)
        assert clear.mean() >= 0.9 and np.array_equal(a_det[clear], m64["logits"].argmax(axis=1)[clear]), what
        for acts, logp in ((a_det, lp_det), (a, lp)):  # logp at the device's own action
            assert acts.dtype == np.int32 and acts.min() >= 0 and acts.max() <= 5
            s32 = policy_model.act(pol, obs, activation=activation, dtype=np.float32, action=acts)["logp"]
            s64 = policy_model.act(pol, obs, activation=activation, action=acts)["logp"]
            _forward(worst, logp, s32, s64, what, "logp at its own action")
    logp, entropy, value = _np(*env.policy_evaluate_raw_torch(h, d_obs, action))
    assert np.array_equal(value, v), what
    e64 = policy_grad_model.evaluate(pol, obs, a, activation=activation, grads=False)
    e32 = policy_grad_model.evaluate(pol, obs, a, activation=activation, grads=False, dtype=np.float32)
    if continuous:
        _forward(worst, logp, e32["logp"], e64["logp"], what, "evaluate logp")
    else:
        assert np.array_equal(logp, lp), what  # the PPO ratio of the first minibatch is exactly 1
    _forward(worst, entropy, e32["entropy"], e64["entropy"], what, "entropy")
    g = c["g"]
    out = env.policy_grad_torch(h, d_obs, _dev(c["action"]), g_logp=_dev(g["logp"]), g_entropy=_dev(g["entropy"]), g_value=_dev(g["value"]))
    gpu_policy_grad._check_grads(gpu_policy_grad._grads_np(out), policy_reference(c, activation, np.float32),
                                 policy_reference(c, activation, np.float64), what, worst)
    gpu_policy_grad._report(worst)
    env.check_status()
    env.close()


def test_policy_gradients_when_class_3_workgroups_take_a_second_row_tile():
    """past the grid cap at class 3: 256 workgroups of R = 64 rows and 300 rows more, so the first five load their partial sums back"""
    hidden, n_hidden, activation, n = BIG
    assert tile_class(hidden) == 3 and n > 256 * GRAD_ROWS[3]
    env_id = "GoalContinuous3P-v0"
    c = policy_case(env_id, n, hidden, n_hidden)
    env = _env(env_id, n)
    h = _handle(env, c["policy"], activation)
    g = c["g"]
    out = env.policy_grad_torch(h, _dev(c["obs"]), _dev(c["action"]), g_logp=_dev(g["logp"]), g_entropy=_dev(g["entropy"]), g_value=_dev(g["value"]))
    worst = []
    gpu_policy_grad._check_grads(gpu_policy_grad._grads_np(out), policy_reference(c, activation, np.float32),
                                 policy_reference(c, activation, np.float64), (env_id, n, hidden, n_hidden, activation), worst)
    gpu_policy_grad._report(worst)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
def test_q(hidden, n_hidden, activation):
    """q_evaluate_raw_torch against the model; q_grad_torch(action_grad=True) with both critics; the actor chain as
    test_gpu_q.test_actor_chain: the action without eps is the deterministic act's bits, with eps within _tol, its gradients against the
    model"""
    import torch
    env_id = ids_of(hidden, n_hidden)[0]
    c = q_case(env_id, N, hidden, n_hidden)
    env = _env(env_id)
    what, worst = (env_id, hidden, n_hidden, activation), []
    d_obs, d_act = _dev(c["obs"]), _dev(c["action"])
    h = gpu_q._q_handle(env, c["critics"], activation)
    q = _np(*env.q_evaluate_raw_torch(h, d_obs, d_act))
    m64 = q_model.q_evaluate(c["critics"], c["obs"], c["action"], activation=activation, grads=False)
    m32 = q_model.q_evaluate(c["critics"], c["obs"], c["action"], activation=activation, grads=False, dtype=np.float32)
    for k in range(2):
        _forward(worst, q[k], m32["q"][k], m64["q"][k], what, "q%d" % (k + 1))
    out = env.q_grad_torch(h, d_obs, d_act, _dev(c["g"][0]), _dev(c["g"][1]), action_grad=True)
    got = gpu_q._q_grads_np(out)
    got["action"] = out["action"].cpu().numpy()
    gpu_q._check_grads(got, q_reference(c, activation, np.float32), q_reference(c, activation, np.float64), what + ("q_grad",), worst)
    # the actor chain
    pol, eps, ga = c["policy"], c["eps"], c["g_action"]
    hp = _handle(env, pol, activation)
    det = _np(env.policy_act_torch(hp, d_obs, deterministic=True)[0])[0]
    assert _np(env.policy_action_raw_torch(hp, d_obs))[0].tobytes() == det.tobytes(), what
    a = _np(env.policy_action_raw_torch(hp, d_obs, _dev(eps)))[0]
    a64 = q_model.action(pol, c["obs"], eps, ga, activation=activation)
    a32 = q_model.action(pol, c["obs"], eps, ga, activation=activation, dtype=np.float32)
    _forward(worst, a, a32["action"], a64["action"], what, "action")
    out = env.policy_action_grad_torch(hp, d_obs, _dev(ga), _dev(eps))
    torch.cuda.synchronize()
    got = q_model.flat(dict(actor=[(w.cpu().numpy(), b.cpu().numpy()) for w, b in out["actor"]], log_std=out["log_std"].cpu().numpy()))
    gpu_q._check_grads(got, actor_chain_reference(c, activation, np.float32), actor_chain_reference(c, activation, np.float64),
                       what + ("action_grad",), worst)
    gpu_q._report(worst)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
def test_squashed(hidden, n_hidden, activation):
    """squashed_act_torch (stochastic and deterministic) and squashed_sample_raw_torch with the caller's eps against the model;
    squashed_grad_torch with g_action and g_logp together, on squashed_model.case's inputs"""
    env_id = ids_of(hidden, n_hidden)[0]
    c = squashed_case(env_id, N, hidden, n_hidden)
    env = _env(env_id)
    what, worst = (env_id, hidden, n_hidden, activation), []
    actor, obs, bounds = c["actor"], c["obs"], squashed_model.BOUNDS
    h = gpu_squashed._handle(env, actor, activation)
    d_obs, d_eps = _dev(obs), _dev(c["eps"])
    for det in (False, True):
        a, lp = _np(*env.squashed_act_torch(h, d_obs, deterministic=det, **NOISE))
        m64 = squashed_model.act(actor, obs, env_index_base=BASE, deterministic=det, bounds=bounds, activation=activation, **NOISE)
        m32 = squashed_model.act(actor, obs, env_index_base=BASE, deterministic=det, bounds=bounds, activation=activation, dtype=np.float32, **NOISE)
        for k, got in (("action", a), ("logp", lp)):
            _forward(worst, got, m32[k], m64[k], what, "act %s%s" % (k, " (deterministic)" if det else ""))
    a, lp = _np(*env.squashed_sample_raw_torch(h, d_obs, d_eps))
    m64 = squashed_model.sample(actor, obs, c["eps"], bounds=bounds, activation=activation)
    m32 = squashed_model.sample(actor, obs, c["eps"], bounds=bounds, activation=activation, dtype=np.float32)
    for k, got in (("action", a), ("logp", lp)):
        _forward(worst, got, m32[k], m64[k], what, "sample " + k)
    out = env.squashed_grad_torch(h, d_obs, d_eps, _dev(c["g_action"]), _dev(c["g_logp"]))
    gpu_squashed._check_grads(gpu_squashed._grads_np(out), squashed_reference(c, activation, np.float32),
                              squashed_reference(c, activation, np.float64), what + ("both",), worst)
    gpu_squashed._report(worst)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
def test_dqn(hidden, n_hidden, activation):
    """dqn_evaluate_raw_torch: q_all against the model, q_taken / q_max / argmax from the kernel's own q_all on every row, and the
    model's argmax away from ties; the greedy dqn_act_torch; dqn_grad_torch with g_taken and g_all together, on dqn_model.case's inputs"""
    import torch
    env_id = ids_of(hidden, n_hidden)[1]
    c = dqn_case(env_id, N, hidden, n_hidden)
    env = _env(env_id)
    assert env.discrete
    what, worst = (env_id, hidden, n_hidden, activation), []
    net, obs = c["net"], c["obs"]
    h = gpu_dqn._handle(env, net, activation)
    d_obs, d_action = _dev(obs), _dev(c["action"])
    q_all, argmax = gpu_dqn._check_discrete_outputs(env, h, d_obs, d_action, what)
    m64 = dqn_model.evaluate(net, obs, activation=activation)
    m32 = dqn_model.evaluate(net, obs, activation=activation, dtype=np.float32)["q_all"]
    _forward(worst, _np(q_all)[0], m32, m64["q_all"], what, "q_all")
    top = np.sort(m64["q_all"], axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * _tol(m32, m64["q_all"])  # (an argmax within the tolerance of a tie may go either way)
    assert clear.mean() >= 0.9 and np.array_equal(_np(argmax)[0][clear], m64["argmax"][clear]), what
    a, q = env.dqn_act_torch(h, d_obs, seed=5, step=9)  # epsilon 0: greedy
    torch.cuda.synchronize()
    assert torch.equal(a, argmax), what
    assert q.cpu().numpy().tobytes() == q_all.gather(1, argmax.long()[:, None])[:, 0].cpu().numpy().tobytes(), what
    out = env.dqn_grad_torch(h, d_obs, d_action, _dev(c["g_taken"]), _dev(c["g_all"]))
    gpu_dqn._check_grads(gpu_dqn._grads_np(out), dqn_reference(c, activation, np.float32), dqn_reference(c, activation, np.float64),
                         what + ("both",), worst)
    gpu_dqn._report(worst)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
@pytest.mark.parametrize("kind", KINDS)
def test_population(kind, hidden, n_hidden, activation):
    """P = 3 on B = 240 envs, blocks of 80: a member boundary falls inside a workgroup.  Act on the blocks, evaluate and grad on
    [P, 200] rows: every member's outputs are the bits of the single-policy call on population_member_torch(pop, m)"""
    P, B = 3, 240
    env_id = ids_of(hidden, n_hidden)[KINDS.index(kind)]
    env = _env(env_id, B)
    assert bit_equal_to_single(N, grad_rows(hidden), P) and grad_rows(hidden) == GRAD_ROWS[tile_class(hidden)]
    rng = np.random.default_rng([N, hidden, n_hidden])
    pop = random_population(rng, P, env.obs_dim, hidden, n_hidden, 6 if env.discrete else 2, continuous=not env.discrete)
    h = gpu_population._pop_handle(env, pop, activation)
    what = (env_id, hidden, n_hidden, activation)
    block_obs = _dev(rng.standard_normal((B, env.obs_dim)).astype(np.float32))
    a, lp, v = gpu_population._check_act(env, h, P, block_obs, what, **NOISE)
    a_det, lp_det, v_det = gpu_population._check_act(env, h, P, block_obs, what, deterministic=True, **NOISE)
    assert v.tobytes() == v_det.tobytes() and a.tobytes() != a_det.tobytes()
    v0 = _np(env.policy_act_torch(env.population_member_torch(h, 0), block_obs, **NOISE)[2])[0]
    assert np.abs(v0[80:160] - v[80:160]).max() > 1e-3, what  # the members differ: block 1 under member 0's parameters is something else
    obs, action = gpu_population._rows(env, rng, P, N)
    d_obs, d_action = _dev(obs), _dev(action)
    got = _np(*env.population_evaluate_raw_torch(h, d_obs, d_action))
    assert all(x.shape == (P, N) for x in got)
    for m in range(P):
        want = _np(*env.policy_evaluate_raw_torch(env.population_member_torch(h, m), d_obs[m], d_action[m]))
        for name, x, w in zip(("logp", "entropy", "value"), got, want):
            assert x[m].tobytes() == w.tobytes(), (what, m, name)
    g = [_dev(rng.standard_normal((P, N)).astype(np.float32)) for _ in range(3)]
    stacked = gpu_population._stacked_np(env.population_grad_torch(h, d_obs, d_action, *g))
    for m in range(P):
        mine, want = flat_member(stacked, m), gpu_population._single_grads(env, h, m, d_obs, d_action, g)
        assert set(mine) == set(want) and any(np.abs(x).max() > 0 for x in mine.values())
        for k in want:
            assert mine[k].tobytes() == want[k].tobytes(), (what, m, k)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
@pytest.mark.parametrize("kind", KINDS)
def test_ppo(kind, hidden, n_hidden, activation):
    """tests/test_gpu_ppo.py's two cores at the width, with its KW: the gradients are policy_grad_torch's bits on the gathered rows with
    the per-row g_logp / g_value the kernel reports; per-row vectors, the twelve statistics and every gradient against ppo_model"""
    env_id = ids_of(hidden, n_hidden)[KINDS.index(kind)]
    _ppo_keys.append((env_id, hidden, n_hidden, activation, True, True))
    gpu_ppo._bit_exact_core(env_id, hidden, n_hidden, activation, N)
    worst = []
    m64 = gpu_ppo._model_case(env_id, hidden, n_hidden, activation, N, gpu_ppo.KW, worst)
    assert 0 < m64["pg_unclipped"].mean() < 1 and 0 < m64["v_unclipped"].mean() < 1
    gpu_ppo._report(worst)


@pytest.mark.parametrize("hidden,n_hidden,activation", cases())
@pytest.mark.parametrize("kind", KINDS)
def test_population_ppo(kind, hidden, n_hidden, activation):
    """every member of a P = 3 population is ppo_grad_torch on its member handle, bit for bit: gradients, the twelve statistics and the
    per-row outputs, with a coefficient tensor whose rows differ (tests/test_gpu_population_ppo.py's first test at the width)"""
    env_id = ids_of(hidden, n_hidden)[KINDS.index(kind)]
    _population_ppo_keys.append((env_id, hidden, n_hidden, activation, 240, 3, True))
    env, h, pop, batch, host = gpu_population_ppo._shared(env_id, hidden, n_hidden, activation)
    assert gpu_population_ppo.bit_equal_to_single(N, grad_rows(hidden), 3)
    d_index = _dev(gpu_population_ppo._own_rows_index(np.random.default_rng(N + hidden), 3, N, 240))
    got = gpu_population_ppo._assert_members_equal_single_calls(env, h, batch, d_index, gpu_population_ppo.COEF3, {},
                                                                (env_id, hidden, n_hidden, activation, N), branches=True)
    assert np.abs(got[2]["logp"][0] - got[2]["logp"][1]).max() > 1e-3  # the members differ
    env.check_status()


@pytest.mark.parametrize("hidden", TWO_HANDLE_WIDTHS)
def test_a_narrower_id_on_a_second_handle_leaves_the_widest_net_of_the_first_its_lds(hidden):
    """nets_begin raises the limit of a kernel instantiation once per handle, sized by that handle's observation width, but the limit
    belongs to the kernel: with a 4P handle (observation 17) and a Kepler handle (10) alive together, the Kepler handle's first
    gradient call sets a smaller limit than the 4P handle's widest net of the class uses.  That net must go on running, with the same
    bits"""
    wide_id, narrow_id = WIDE_ID, NARROW_ID
    wide, narrow = _env(wide_id), _env(narrow_id)
    cw, cn = policy_case(wide_id, N, hidden, 3), policy_case(narrow_id, N, hidden, 1)
    hw, hn = _handle(wide, cw["policy"]), _handle(narrow, cn["policy"])

    def grads(env, h, c):
        g = c["g"]
        out = env.policy_grad_torch(h, _dev(c["obs"]), _dev(c["action"]), g_logp=_dev(g["logp"]), g_entropy=_dev(g["entropy"]), g_value=_dev(g["value"]))
        env.check_status()
        return gpu_policy_grad._grads_np(out)

    first = grads(wide, hw, cw)
    worst = []
    gpu_policy_grad._check_grads(grads(narrow, hn, cn), policy_reference(cn, "tanh", np.float32), policy_reference(cn, "tanh", np.float64),
                                 (narrow_id, hidden, 1), worst)
    again = grads(wide, hw, cw)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), (hidden, k)
    gpu_policy_grad._check_grads(again, policy_reference(cw, "tanh", np.float32), policy_reference(cw, "tanh", np.float64), (wide_id, hidden, 3), worst)
    gpu_policy_grad._report(worst)
    wide.close()
    narrow.close()


@pytest.mark.parametrize("hidden", [16, 32, 64, 96, 128])
def test_workspace_bytes_follow_the_row_tile_of_the_class(hidden):
    """through the ABI: one workgroup's partial sums up to n = R, two from R + 1, and the grid cap of 256 bounds them, for R = 256, 128,
    64, 64 rows of classes 1 .. 4"""
    R = GRAD_ROWS[tile_class(hidden)]
    env = make("GoalContinuous3P-v0", 8)
    pol = policy_model.random_policy(np.random.default_rng(hidden), env.obs_dim, hidden, 2, 2)
    h = _handle(env, pol)
    need = lambda n: env._lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), n)
    total = sum(W.size + b.size for net in ("actor", "critic") for W, b in pol[net]) + 2
    assert need(1) == 4 * total and need(R) == need(1), (hidden, R)
    assert need(R + 1) == 2 * need(1), (hidden, R)  # a second workgroup's partial sums
    assert need(10 ** 7) == 256 * need(1), (hidden, R)  # the grid cap bounds it
    env.close()
