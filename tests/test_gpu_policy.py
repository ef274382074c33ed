"""GPU tests of policy_torch / policy_act_torch / rollout_policy_torch (sg_policy_act_device / sg_rollout_policy_device) against the
NumPy float64 model tests/policy_model.py.

Tolerance, wherever one is needed: the same net and formulas evaluated in float32 on the CPU (policy_model with dtype=float32) are the
yardstick of "a correct float32 implementation"; a quantity's tolerance is 8 x max|float32 CPU - float64 model| + 1e-6, computed in the
test from the test's own inputs and printed.  The 8 x leaves room for another (fixed) summation order and FMA contraction; correct
float32 deviates by ~1e-6, a wrong index by ~1e-1 (the parameters are dense and random)."""
import numpy as np
import pytest

from gae_model import dense_from_list, gae_model
from policy_model import act, random_policy

pytestmark = pytest.mark.gpu

GOAL, KEPLER, DISCRETE = "GoalContinuous3P-v0", "KeplerCircleOrbit-v0", "GoalDiscrete3-v0"
NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]


def make(env_id, n, **kw):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _handle(env, pol, activation="tanh"):
    """policy_torch over device copies of a policy_model policy"""
    net = lambda layers: [(_dev(W), _dev(b)) for W, b in layers]
    return env.policy_torch(actor=net(pol["actor"]), critic=net(pol["critic"]) if pol["critic"] is not None else None,
                            log_std=_dev(pol["log_std"]) if pol["log_std"] is not None else None, activation=activation)


def _tol(f32, f64):
    return 8.0 * float(np.abs(np.asarray(f32, np.float64) - f64).max()) + 1e-6


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in ts]


@pytest.mark.parametrize("B", [1, 200])
@pytest.mark.parametrize("env_id", [GOAL, KEPLER, DISCRETE])
def test_act_equals_the_model(env_id, B):
    """1: mean (deterministic=True), value, logp and eps = (action - mean) / exp(log_std) against the float64 model; every net
    shape, both activations, with and without a critic; B = 1 (a partial wave) and 200 (no multiple of the workgroup)"""
    env = make(env_id, B, env_index_base=1000)
    continuous = not env.discrete
    D = env.obs_dim
    rng = np.random.default_rng(B + len(env_id))
    obs = rng.standard_normal((B, D)).astype(np.float32)
    worst = {}
    for hidden, n_hidden in NETS:
        for activation in ("tanh", "relu"):
            for critic in (True, False):
                pol = random_policy(rng, D, hidden, n_hidden, 2 if continuous else 6, critic=critic, continuous=continuous)
                h = _handle(env, pol, activation)
                kw = dict(seed=77, step=2 ** 32 + 5)
                m64 = act(pol, obs, env_index_base=1000, activation=activation, **kw)
                m32 = act(pol, obs, env_index_base=1000, activation=activation, dtype=np.float32, **kw)
                a_det, lp_det, v = _np(*env.policy_act_torch(h, _dev(obs), deterministic=True, **kw))
                a, lp, v2 = _np(*env.policy_act_torch(h, _dev(obs), **kw))
                what = (env_id, B, hidden, n_hidden, activation, critic)
                tols = {}
                if critic:
                    tols["value"] = _tol(m32["value"], m64["value"])
                    assert np.abs(v - m64["value"]).max() <= tols["value"], what
                    assert np.array_equal(v, v2)
                else:
                    assert v is None and v2 is None
                if continuous:
                    std = np.exp(pol["log_std"].astype(np.float64))
                    tols["mean"] = _tol(m32["mean"], m64["mean"])
                    assert np.abs(a_det - m64["mean"]).max() <= tols["mean"], what
                    eps32 = (m32["action"].astype(np.float64) - m32["mean"].astype(np.float64)) / std  # recovered as from the device
                    tols["eps"] = _tol(eps32, m64["eps"])
                    eps = (a.astype(np.float64) - a_det.astype(np.float64)) / std
                    assert np.abs(eps - m64["eps"]).max() <= tols["eps"], (what, np.abs(eps - m64["eps"]).max(), tols["eps"])
                    tols["logp"] = _tol(m32["logp"], m64["logp"])
                    assert np.abs(lp - m64["logp"]).max() <= tols["logp"], what
                    det64 = act(pol, obs, deterministic=True, activation=activation)["logp"]
                    assert np.abs(lp_det - det64).max() <= tols["logp"], what
                else:
                    tols["logits"] = _tol(m32["logits"], m64["logits"])
                    top = np.sort(m64["logits"], axis=1)
                    clear = top[:, -1] - top[:, -2] > 2 * tols["logits"]  # (an argmax within the tolerance of a tie may go either way)
                    assert (B == 1 or clear.mean() >= 0.9) and np.array_equal(a_det[clear], m64["logits"].argmax(axis=1)[clear]), what
                    for acts, logp in ((a_det, lp_det), (a, lp)):  # logp at the device's own action
                        assert acts.dtype == np.int32 and acts.min() >= 0 and acts.max() <= 5
                        s32 = act(pol, obs, activation=activation, dtype=np.float32, action=acts)["logp"]
                        s64 = act(pol, obs, activation=activation, action=acts)["logp"]
                        tols["logp"] = _tol(s32, s64)
                        assert np.abs(logp - s64).max() <= tols["logp"], what
                for k, t in tols.items():
                    worst[k] = max(worst.get(k, 0.0), t)
    print("tolerances (8 x |float32 CPU - float64| + 1e-6), largest over the nets:", env_id, B, {k: "%.3g" % t for k, t in worst.items()})
    env.close()


def test_discrete_draws_equal_the_model_away_from_the_boundaries():
    """2: the sampled action is the model's wherever u * total is farther than 1e-5 * total from every running sum; at most 1 % of
    the draws may be that close (5 boundaries x 2e-5: about 1e-4 of them are)"""
    B, steps = 200, 20
    env = make(DISCRETE, B)
    rng = np.random.default_rng(8)
    obs = rng.standard_normal((B, env.obs_dim)).astype(np.float32)
    pol = random_policy(rng, env.obs_dim, 64, 2, 6, critic=False, continuous=False)
    pol["actor"][-1] = (pol["actor"][-1][0] * 8, pol["actor"][-1][1])  # logits a few units apart: every action is drawn, none dominates
    h = _handle(env, pol)
    compared = left_out = 0
    seen = np.zeros(6, np.int64)
    for step in range(steps):
        m = act(pol, obs, seed=3, step=step)
        a, = _np(env.policy_act_torch(h, _dev(obs), seed=3, step=step)[0])
        far = (np.abs(m["cum"] - m["want"][:, None]) > 1e-5 * m["total"][:, None]).all(axis=1)
        assert np.array_equal(a[far], m["action"][far]), step
        compared += int(far.sum())
        left_out += int((~far).sum())
        seen += np.bincount(a, minlength=6)
    print("discrete draws compared:", compared, "left out:", left_out, "histogram:", seen.tolist())
    assert left_out <= 0.01 * (compared + left_out) and (seen > 0).all()
    env.close()


def test_results_do_not_depend_on_the_batch_and_follow_seed_and_step():
    """3: envs 64 .. 127 of a handle of 200 equal, bit for bit, a handle of 64 with env_index_base = 64 given those rows; a
    repeated call is bit-identical; another step or seed changes the noise"""
    rng = np.random.default_rng(9)
    for env_id in (GOAL, DISCRETE):
        whole, part = make(env_id, 200), make(env_id, 64, env_index_base=64)
        continuous = not whole.discrete
        D = whole.obs_dim
        obs = rng.standard_normal((200, D)).astype(np.float32)
        pol = random_policy(rng, D, 33, 2, 2 if continuous else 6, continuous=continuous)
        hw, hp = _handle(whole, pol), _handle(part, pol)
        a, lp, v = _np(*whole.policy_act_torch(hw, _dev(obs), seed=5, step=6))
        a2, lp2, v2 = _np(*whole.policy_act_torch(hw, _dev(obs), seed=5, step=6))
        assert a.tobytes() == a2.tobytes() and lp.tobytes() == lp2.tobytes() and v.tobytes() == v2.tobytes()
        pa, plp, pv = _np(*part.policy_act_torch(hp, _dev(obs[64:128]), seed=5, step=6))
        assert pa.tobytes() == a[64:128].tobytes() and plp.tobytes() == lp[64:128].tobytes() and pv.tobytes() == v[64:128].tobytes()
        for kw in (dict(seed=5, step=7), dict(seed=6, step=6), dict(seed=5, step=6 + 2 ** 32)):
            b, blp, bv = _np(*whole.policy_act_torch(hw, _dev(obs), **kw))
            assert (b != a).mean() > (0.5 if continuous else 0.2), kw
            assert bv.tobytes() == v.tobytes()
        whole.close()
        part.close()


K, B = 5, 200


def _buffers(env, K, cap):
    import torch
    D = env.obs_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, dtype=torch.int32) if env.discrete else z(K, B, 2), logp=z(K, B), value=z(K + 1, B),
             reward=z(K, B), done=z(K, B, dtype=torch.uint8), trunc=z(K, B, dtype=torch.uint8))
    return b, env.terminal_list_torch(cap)


def _hand_loop(env, h, K, seed, first_step):
    """policy_act_torch then step_torch(terminal_obs=...) K times; the terminal records as a set of (step, env, obs bytes, value bits)"""
    import torch
    b, _ = _buffers(env, K, 1)
    b["obs"][0].copy_(env.reset_torch())
    tobs = torch.zeros((B, env.obs_dim), dtype=torch.float32, device="cuda")
    records = set()
    for t in range(K):
        out = dict(action=b["action"][t], logp=b["logp"][t], value=b["value"][t])
        env.policy_act_torch(h, b["obs"][t], seed=seed, step=first_step + t, out=out)
        env.step_torch(b["action"][t], out=dict(obs=b["obs"][t + 1], reward=b["reward"][t], done=b["done"][t], trunc=b["trunc"][t]),
                       terminal_obs=tobs)
        tv = env.policy_act_torch(h, tobs, seed=seed, step=0)[2]
        d, to, tvn = _np(b["done"][t], tobs, tv)
        for i in np.nonzero(d)[0]:
            records.add((t, int(i), to[i].tobytes(), tvn[i].tobytes()))
    b["value"][K].copy_(env.policy_act_torch(h, b["obs"][K], seed=seed, step=0)[2])
    return b, records


def _list_records(term):
    count, se, ob, va = _np(term["count"], term["step_env"], term["obs"], term["value"])
    n = int(count[0])
    assert n <= se.shape[0]
    return {(int(se[k, 0]), int(se[k, 1]), ob[k].tobytes(), va[k].tobytes()) for k in range(n)}, n


@pytest.mark.parametrize("normalize_obs", [False, True])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_rollout_equals_the_hand_written_loop(env_id, normalize_obs):
    """4: every output of rollout_policy_torch, bit for bit; max_episode_steps = 3 puts truncations and auto-resets inside the call,
    so the terminal list and terminal["value"] are exercised (the list is unordered: compared as a set)"""
    kw = dict(seed=21, max_episode_steps=3, normalize_obs=normalize_obs)
    ea, eb = make(env_id, B, **kw), make(env_id, B, **kw)
    rng = np.random.default_rng(10)
    pol = random_policy(rng, ea.obs_dim, 64, 2, 6 if ea.discrete else 2, continuous=not ea.discrete)
    ha, hb = _handle(ea, pol), _handle(eb, pol)
    want, records = _hand_loop(ea, ha, K, seed=4, first_step=100)
    got, term = _buffers(eb, K, 1000)
    got["obs"][0].copy_(eb.reset_torch())
    eb.rollout_policy_torch(hb, seed=4, first_step=100, terminal=term, **got)
    eb.check_status()
    for name in want:
        w, g = _np(want[name], got[name])
        assert w.tobytes() == g.tobytes(), (name, int((w != g).sum()))
    trunc, done = _np(got["trunc"], got["done"])
    assert trunc[2].mean() > 0.9 and done.sum() >= 0.9 * B  # (nearly) every env runs into the time limit at t = 2
    listed, n = _list_records(term)
    assert n == int(done.sum()) == len(records) and listed == records
    ea.close()
    eb.close()


def test_rollout_feeds_gae_without_anything_in_between():
    """5: the rollout's outputs, passed to gae_torch as they are, give what tests/gae_model.py gives on the same arrays"""
    env = make(GOAL, B, seed=3, max_episode_steps=3)
    rng = np.random.default_rng(11)
    pol = random_policy(rng, env.obs_dim, 33, 2, 2)
    h = _handle(env, pol)
    b, term = _buffers(env, K, 1000)
    b["obs"][0].copy_(env.reset_torch())
    env.rollout_policy_torch(h, seed=1, terminal=term, **b)
    adv, ret = env.gae_torch(b["reward"], b["done"], b["trunc"], b["value"][:-1], b["value"][-1],
                             terminal=env.value_list_torch(terminal=term, values=term["value"]), gamma=0.97, lam=0.9)
    env.check_status()
    reward, done, trunc, value, count, se, tv, adv, ret = _np(b["reward"], b["done"], b["trunc"], b["value"], term["count"],
                                                              term["step_env"], term["value"], adv, ret)
    assert (done & trunc).any() and np.abs(tv[:int(count[0])]).max() > 0
    dense = dense_from_list(K, B, int(count[0]), se, tv)
    wa, wr = gae_model(reward, done, trunc, value[:-1], value[-1], dense, gamma=0.97, lam=0.9)
    assert wa.tobytes() == adv.tobytes() and wr.tobytes() == ret.tobytes()
    env.close()


def test_a_captured_rollout_replays_the_eager_results():
    """6: one torch.cuda.graph capture of a K = 4 rollout (a linear chain on one stream), replayed twice from the same start, gives
    the eager call's outputs both times"""
    import torch
    Kg = 4
    rng = np.random.default_rng(12)
    kw = dict(seed=8, max_episode_steps=3)
    ea, eb = make(GOAL, B, **kw), make(GOAL, B, **kw)
    pol = random_policy(rng, ea.obs_dim, 64, 2, 2)
    ha, hb = _handle(ea, pol), _handle(eb, pol)
    want, wterm = _buffers(ea, Kg, 1000)
    want["obs"][0].copy_(ea.reset_torch())
    ea.rollout_policy_torch(ha, seed=2, first_step=0, terminal=wterm, **want)
    wrec, _ = _list_records(wterm)
    got, term = _buffers(eb, Kg, 1000)
    term["value"] = torch.zeros(1000, dtype=torch.float32, device="cuda")
    obs0 = eb.reset_torch().clone()
    snap = eb.snapshot_torch()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (warm-up on the capture's stream: the first call raises the kernels' LDS limit)
        eb.rollout_policy_torch(hb, seed=2, first_step=0, terminal=term, **got)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eb.rollout_policy_torch(hb, seed=2, first_step=0, terminal=term, **got)
    for _ in range(2):
        eb.restore_torch(snap)
        for t in got.values():
            t.zero_()
        got["obs"][0].copy_(obs0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for name in want:
            w, g = _np(want[name], got[name])
            assert w.tobytes() == g.tobytes(), name
        assert _list_records(term)[0] == wrec
    eb.check_status()
    ea.close()
    eb.close()


def test_native_refusals():
    """7: a head of the wrong width for the id, and a value buffer with a policy that has no critic, are refused by the library"""
    import ctypes as C

    import torch
    from space_gym_amd._native import NativeError
    env = make(GOAL, 8)
    rng = np.random.default_rng(13)
    h = _handle(env, random_policy(rng, env.obs_dim, 16, 1, 2, critic=False))
    obs = torch.zeros((8, env.obs_dim), device="cuda")
    a, lp, v = torch.zeros((8, 2), device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    args = (env._h, C.byref(h.struct), C.c_void_p(obs.data_ptr()), 0, 0, 0, C.c_void_p(a.data_ptr()), C.c_void_p(lp.data_ptr()))
    assert env._lib.sg_policy_act_device(*args, C.c_void_p(v.data_ptr()), env._stream()) == -1
    assert b"no critic" in env._lib.sg_last_error(env._h)
    b, _ = _buffers(env, 2, 1)
    b = {k: t[:, :8].contiguous() for k, t in b.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = env._lib.sg_rollout_policy_device(env._h, 2, C.byref(h.struct), 0, 0, 0, ptr(b["obs"]), ptr(b["action"]), ptr(b["logp"]), ptr(b["value"]),
                                           ptr(b["reward"]), ptr(b["done"]), ptr(b["trunc"]), None, None, env._stream())
    assert rc == -1 and b"no critic" in env._lib.sg_last_error(env._h)
    h.struct.head = 6
    assert env._lib.sg_policy_act_device(*args, None, env._stream()) == -1
    assert b"head has 6 outputs" in env._lib.sg_last_error(env._h)
    h.struct.head = 2
    for field, bad in (("hidden", 129), ("n_hidden", 0), ("activation", 2), ("struct_size", 8)):
        keep = getattr(h.struct, field)
        setattr(h.struct, field, bad)
        with pytest.raises(NativeError, match=field if field != "struct_size" else "struct_size"):
            env.policy_act_torch(h, obs)
        setattr(h.struct, field, keep)
    assert env.policy_act_torch(h, obs)[2] is None  # the handle still works
    torch.cuda.synchronize()
    env.check_status()
    env.close()
