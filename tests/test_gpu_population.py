"""GPU tests of the policy-population calls (policy_population_torch / population_act_torch / rollout_population_torch /
population_evaluate_raw_torch / population_grad_torch / population_evaluate_torch).

The oracle is the engine's own single-policy path: member m's rows must be, BIT FOR BIT, what policy_act_torch / policy_evaluate_raw_torch
/ policy_grad_torch give with population_member_torch(pop, m) -- a plain Policy over the views W[m], b[m], log_std[m] -- and those calls
are checked against the NumPy model by tests/test_gpu_policy.py and tests/test_gpu_policy_grad.py.  The members' parameters are drawn
independently and dense, so a wrong member offset moves a result by ~1e-1.  The one place a tolerance is needed is the gradient beyond the
grouping cap (ceil(n / R) > 256 // P), where a member's sums group otherwise than the single call's: there the yardstick is the float64
model and tests/test_gpu_policy_grad.py's rule, 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|), at most 1 % of max|G64| (checked for these
very cases on the CPU by tests/test_population.py)."""
import ctypes as C

import numpy as np
import pytest

from gae_model import dense_from_list
from policy_grad_model import flat, grad_tolerances
from population_model import (BEYOND_CASES, BEYOND_P, OBS_DIM, beyond_case, beyond_reference, bit_equal_to_single, evaluate, flat_member,
                              grad_rows, groups, member, random_population)
from test_gpu_policy import DISCRETE, GOAL, NETS, _dev, _handle, _np, make
from test_gpu_policy_grad import _check_grads, _modules, _ppo_loss, _report

pytestmark = pytest.mark.gpu


def _stack_dev(pop):
    """device copies of a population_model population: (actor pairs, critic pairs or None, log_std or None)"""
    net = lambda layers: None if layers is None else [(_dev(W), _dev(b)) for W, b in layers]
    return net(pop["actor"]), net(pop["critic"]), _dev(pop["log_std"]) if pop["log_std"] is not None else None


def _pop_handle(env, pop, activation="tanh"):
    actor, critic, log_std = _stack_dev(pop)
    return env.policy_population_torch(pop["actor"][0][0].shape[0], actor=actor, critic=critic, log_std=log_std, activation=activation)


def _population(env, rng, P, hidden, n_hidden, critic=True):
    continuous = not env.discrete
    return random_population(rng, P, env.obs_dim, hidden, n_hidden, 2 if continuous else 6, critic=critic, continuous=continuous)


def _same(a, b):
    return (a is None and b is None) or a.tobytes() == b.tobytes()


def _check_act(env, h, P, obs, what, **kw):
    """population_act_torch against policy_act_torch of every member's handle on that member's block; returns the population's outputs"""
    B = env.num_envs
    n = B // P
    got = _np(*env.population_act_torch(h, obs, **kw))
    for m in range(P):
        want = _np(*env.policy_act_torch(env.population_member_torch(h, m), obs, **kw))
        rows = slice(m * n, (m + 1) * n)
        for name, g, w in zip(("action", "logp", "value"), got, want):
            assert (g is None) == (w is None) and (g is None or g[rows].tobytes() == w[rows].tobytes()), (what, kw, m, name)
    return got


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_act_equals_every_members_own_handle_on_its_block(env_id):
    """1: B = 240, P = 3 -- blocks of 80, so a member boundary falls inside what a plain launch makes one workgroup; the four nets, both
    activations; stochastic and deterministic, values only, and the seed and both words of the step"""
    B, P = 240, 3
    env = make(env_id, B, env_index_base=1000)
    assert env.obs_dim == OBS_DIM
    rng = np.random.default_rng(31)
    obs = _dev(rng.standard_normal((B, env.obs_dim)).astype(np.float32))
    base = dict(seed=77, step=2 ** 32 + 5)
    for i, (hidden, n_hidden) in enumerate(NETS):
        for activation in ("tanh", "relu"):
            pop = _population(env, rng, P, hidden, n_hidden)
            h = _pop_handle(env, pop, activation)
            what = (env_id, hidden, n_hidden, activation)
            a, lp, v = _check_act(env, h, P, obs, what, **base)
            a_det, lp_det, v_det = _check_act(env, h, P, obs, what, deterministic=True, **base)
            assert _same(v, v_det) and not _same(a, a_det)
            # the members differ: block 1 under member 0's parameters is something else
            v0 = _np(env.policy_act_torch(env.population_member_torch(h, 0), obs, **base)[2])[0]
            assert hidden == 1 or np.abs(v0[80:160] - v[80:160]).max() > 1e-3, what
            import torch
            only = torch.full((B,), float("nan"), device="cuda")
            assert env.population_act_torch(h, obs, out=dict(value=only), **base)[:2] == (None, None)
            assert _same(_np(only)[0], v), what  # values only
            if activation == "tanh":
                for kw in (dict(seed=78, step=2 ** 32 + 5), dict(seed=77, step=2 ** 32 + 6), dict(seed=77, step=5)):
                    b, blp, bv = _check_act(env, h, P, obs, what, **kw)
                    assert (b != a).mean() > (0.5 if not env.discrete else 0.1 if hidden > 1 else 0.0), (what, kw)
                    assert _same(bv, v)
    # without critics
    pop = _population(env, rng, P, 33, 2, critic=False)
    h = _pop_handle(env, pop)
    assert _check_act(env, h, P, obs, "no critic", **base)[2] is None
    env.check_status()
    env.close()


@pytest.mark.parametrize("B,P", [(600, 2), (200, 1), (6, 6)])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_act_on_other_block_shapes(env_id, B, P):
    """2: blocks of 300 (a full workgroup and a partial one per member at both workgroup sizes, 256 and 128 lanes); P = 1 equals
    policy_act_torch on the whole batch; one env per member"""
    env = make(env_id, B, env_index_base=64)
    rng = np.random.default_rng(B + P)
    obs = _dev(rng.standard_normal((B, env.obs_dim)).astype(np.float32))
    for hidden, n_hidden, activation in ((1, 1, "relu"), (33, 2, "tanh"), (128, 3, "relu")):
        pop = _population(env, rng, P, hidden, n_hidden)
        h = _pop_handle(env, pop, activation)
        for kw in (dict(seed=3, step=9), dict(seed=3, step=9, deterministic=True)):
            got = _check_act(env, h, P, obs, (env_id, B, P, hidden), **kw)
            if P == 1:  # a plain handle over copies of the one member's parameters, on the whole batch
                want = _np(*env.policy_act_torch(_handle(env, member(pop, 0), activation), obs, **kw))
                assert all(_same(g, w) for g, w in zip(got, want))
    env.check_status()
    env.close()


def _rows(env, rng, P, n):
    obs = rng.standard_normal((P, n, env.obs_dim)).astype(np.float32)
    action = rng.standard_normal((P, n, 2)).astype(np.float32) if not env.discrete else rng.integers(0, 6, (P, n)).astype(np.int32)
    return obs, action


@pytest.mark.parametrize("n", [1, 200, 2049])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_evaluate_equals_every_members_own_handle_and_acts_own_rows(env_id, n):
    """3: [P, n] outputs bit for bit policy_evaluate_raw_torch of the member's handle on obs[m]; value and the discrete logp bit-equal to
    population_act_torch's on its own rows and actions"""
    P = 3
    env = make(env_id, P * n)
    rng = np.random.default_rng(n)
    obs, action = _rows(env, rng, P, n)
    d_obs, d_action = _dev(obs), _dev(action)
    for i, (hidden, n_hidden) in enumerate(NETS):
        activation = ("tanh", "relu")[i % 2]
        pop = _population(env, rng, P, hidden, n_hidden)
        h = _pop_handle(env, pop, activation)
        got = _np(*env.population_evaluate_raw_torch(h, d_obs, d_action))
        assert all(g.shape == (P, n) for g in got)
        for m in range(P):
            want = _np(*env.policy_evaluate_raw_torch(env.population_member_torch(h, m), d_obs[m], d_action[m]))
            for name, g, w in zip(("logp", "entropy", "value"), got, want):
                assert g[m].tobytes() == w.tobytes(), (env_id, n, hidden, m, name)
        # each output alone
        import torch
        for k, name in enumerate(("logp", "entropy", "value")):
            one = torch.full((P, n), float("nan"), device="cuda")
            env.population_evaluate_raw_torch(h, d_obs, d_action, out={name: one})
            assert _same(_np(one)[0], got[k]), name
        # act's own rows: the env blocks are the rows [m]
        a, lp, v = env.population_act_torch(h, d_obs.view(P * n, -1), seed=5, step=3)
        lp2, _, v2 = env.population_evaluate_raw_torch(h, d_obs, a.view((P, n) if env.discrete else (P, n, 2)))
        lp, v, lp2, v2 = _np(lp, v, lp2, v2)
        assert v2.reshape(-1).tobytes() == v.tobytes(), (env_id, n, hidden)
        if env.discrete:
            assert lp2.reshape(-1).tobytes() == lp.tobytes(), (env_id, n, hidden)  # the PPO ratio of the first minibatch is exactly 1
    env.check_status()
    env.close()


def _stacked_np(out):
    import torch
    torch.cuda.synchronize()
    cpu = lambda pairs: None if pairs is None else [(w.cpu().numpy(), b.cpu().numpy()) for w, b in pairs]
    return dict(actor=cpu(out["actor"]), critic=cpu(out.get("critic")), log_std=out["log_std"].cpu().numpy() if out.get("log_std") is not None else None)


def _single_grads(env, h, m, d_obs, d_action, g):
    out = env.policy_grad_torch(env.population_member_torch(h, m), d_obs[m], d_action[m], *[None if x is None else x[m] for x in g])
    return flat(_stacked_np(out))


@pytest.mark.parametrize("n", [1, 200, 2049])
@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_gradients_within_the_cap_are_the_single_calls_bits(env_id, n):
    """4: ceil(n / R) <= 85 = 256 // 3 for every R, so each member's rows group as policy_grad_torch's at the same n: every tensor bit for
    bit, with g_logp, g_entropy and g_value together and singly; g_value=None leaves zeros in critic slots that are given"""
    import torch
    P = 3
    env = make(env_id, P)
    rng = np.random.default_rng(100 + n)
    obs, action = _rows(env, rng, P, n)
    d_obs, d_action = _dev(obs), _dev(action)
    d_g = {k: _dev(rng.standard_normal((P, n)).astype(np.float32)) for k in ("logp", "entropy", "value")}
    for i, (hidden, n_hidden) in enumerate(NETS):
        assert bit_equal_to_single(n, grad_rows(hidden), P)
        pop = _population(env, rng, P, hidden, n_hidden)
        h = _pop_handle(env, pop, ("relu", "tanh")[i % 2])
        for sel in ("all", "logp", "entropy", "value"):
            g = [d_g[k] if sel in ("all", k) else None for k in ("logp", "entropy", "value")]
            out = env.population_grad_torch(h, d_obs, d_action, *g)
            assert (out["critic"] is None) == (g[2] is None)
            got = _stacked_np(out)
            assert got["actor"][0][0].shape == pop["actor"][0][0].shape and (env.discrete or got["log_std"].shape == (P, 2))
            for m in range(P):
                mine, want = flat_member(got, m), _single_grads(env, h, m, d_obs, d_action, g)
                assert set(mine) == set(want)
                for k in want:
                    assert mine[k].tobytes() == want[k].tobytes(), (env_id, n, hidden, sel, m, k)
                if sel == "all":
                    assert any(np.abs(v).max() > 0 for v in mine.values())
        # critic slots given without g_value: written with zeros
        full = env.population_grad_torch(h, d_obs, d_action, d_g["logp"], d_g["entropy"], d_g["value"])
        for w, b in full["critic"]:
            w.fill_(float("nan")); b.fill_(float("nan"))
        again = env.population_grad_torch(h, d_obs, d_action, d_g["logp"], None, None, out=full)
        torch.cuda.synchronize()
        assert all(not w.any() and not b.any() for w, b in again["critic"]), (env_id, n, hidden)
    env.check_status()
    env.close()


@pytest.mark.parametrize("hidden,R", BEYOND_CASES)
def test_gradients_beyond_the_cap_equal_the_model(hidden, R):
    """5: n = 85 R + 300 rows per member: 85 workgroups per member, the first of which take a second row tile of their own member only.
    Per tensor and per member against the float64 model within 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|); twice into NaN-prefilled
    buffers (and workspace): the same bits, no NaN left"""
    import torch
    c = beyond_case(hidden, R)
    n, P = c["n"], BEYOND_P
    assert not bit_equal_to_single(n, R, P) and groups(n, R, P) == 85
    env = make(GOAL, P)
    assert env.obs_dim == OBS_DIM
    h = _pop_handle(env, c["pop"])
    d_obs, d_action = _dev(c["obs"]), _dev(c["action"])
    g = [_dev(c["g"][k]) for k in ("logp", "entropy", "value")]
    out = env.population_grad_torch(h, d_obs, d_action, *g)
    got = _stacked_np(out)
    assert h.workspace.numel() == 4 * P * 85 * sum(t.numel() for t in h.tensors) // P
    r64, r32 = beyond_reference(c, np.float64), beyond_reference(c, np.float32)
    worst = []
    for m in range(P):
        _check_grads(flat_member(got, m), flat_member(r32, m), flat_member(r64, m), (hidden, R, n, "member", m), worst)
    _report(worst)
    h.workspace.view(torch.float32).fill_(float("nan"))
    for t in [x for pairs in (out["actor"], out["critic"]) for pair in pairs for x in pair] + [out["log_std"]]:
        t.fill_(float("nan"))
    again = _stacked_np(env.population_grad_torch(h, d_obs, d_action, *g, out=out))
    for m in range(P):
        a, b = flat_member(got, m), flat_member(again, m)
        for k in a:
            assert not np.isnan(b[k]).any() and a[k].tobytes() == b[k].tobytes(), (hidden, m, k)
    env.check_status()
    env.close()


@pytest.mark.parametrize("env_id", [GOAL, DISCRETE])
def test_autograd_end_to_end(env_id):
    """6: a clipped-PPO loss summed over 3 members through population_evaluate_torch and backward(), against 3 float64 CPU module stacks
    with the members' parameters (tests/test_gpu_policy_grad.py's rule, g = d loss / d outputs); .grad accumulates on the stacked tensors"""
    import torch
    P, n = 3, 200
    env = make(env_id, P)
    continuous = not env.discrete
    rng = np.random.default_rng(14)
    pop = _population(env, rng, P, 64, 2)
    obs, action = _rows(env, rng, P, n)
    old_logp = (evaluate(pop, obs, action, grads=False)["logp"] + 0.3 * rng.standard_normal((P, n))).astype(np.float32)  # some ratios are clipped
    adv, ret = rng.standard_normal((P, n)).astype(np.float32), rng.standard_normal((P, n)).astype(np.float32)
    # float64 on the CPU, member by member: outputs as leaves of the loss give g, the modules give G64
    lin = lambda net: [x for x in net if isinstance(x, torch.nn.Linear)]
    g64, g_out = [], []
    for m in range(P):
        actor, critic, log_std = _modules(member(pop, m), "tanh", torch.float64, "cpu")
        x = torch.from_numpy(obs[m]).double()
        head = actor(x)
        if continuous:
            dist = torch.distributions.Normal(head, log_std.exp().expand_as(head))
            logp, ent = dist.log_prob(torch.from_numpy(action[m]).double()).sum(1), dist.entropy().sum(1)
        else:
            dist = torch.distributions.Categorical(logits=head)
            logp, ent = dist.log_prob(torch.from_numpy(action[m]).long()), dist.entropy()
        value = critic(x)[:, 0]
        for t in (logp, ent, value):
            t.retain_grad()
        _ppo_loss(logp, ent, value, torch.from_numpy(old_logp[m]).double(), torch.from_numpy(adv[m]).double(), torch.from_numpy(ret[m]).double()).backward()
        g64.append(flat(dict(actor=[(x.weight.grad.numpy(), x.bias.grad.numpy()) for x in lin(actor)],
                             critic=[(x.weight.grad.numpy(), x.bias.grad.numpy()) for x in lin(critic)],
                             log_std=log_std.grad.numpy() if continuous else None)))
        g_out.append([t.grad.numpy().astype(np.float32) for t in (logp, ent, value)])
    g = [np.stack([g_out[m][k] for m in range(P)]) for k in range(3)]
    r32 = evaluate(pop, obs, action, *g, dtype=np.float32)
    # the device: the stacked tensors are the leaves
    actor, critic, log_std = _stack_dev(pop)
    leaves = [t for pair in actor + critic for t in pair] + ([log_std] if continuous else [])
    for t in leaves:
        t.requires_grad_()
    h = env.policy_population_torch(P, actor=actor, critic=critic, log_std=log_std)
    d_obs, d_action, d_old, d_adv, d_ret = _dev(obs), _dev(action), _dev(old_logp), _dev(adv), _dev(ret)

    def loss():
        logp, ent, value = env.population_evaluate_torch(h, d_obs, d_action)
        assert all(t.grad_fn is not None and tuple(t.shape) == (P, n) for t in (logp, ent, value))
        return sum(_ppo_loss(logp[m], ent[m], value[m], d_old[m], d_adv[m], d_ret[m]) for m in range(P))

    loss().backward()
    grads = lambda: _stacked_np(dict(actor=[(w.grad, b.grad) for w, b in actor], critic=[(w.grad, b.grad) for w, b in critic],
                                     log_std=log_std.grad if continuous else None))
    once = grads()
    worst = []
    for m in range(P):
        _check_grads(flat_member(once, m), flat_member(r32, m), g64[m], (env_id, "ppo", "member", m), worst)
    _report(worst)
    loss().backward()  # a second backward accumulates: x + x is exact
    twice = grads()
    for m in range(P):
        a, b = flat_member(once, m), flat_member(twice, m)
        for k in a:
            assert np.array_equal(b[k], a[k] + a[k]), (m, k)
    # a loss that uses the value alone: NULL g_logp / g_entropy, and the actor's gradients are zeros
    for t in leaves:
        t.grad = None
    env.population_evaluate_torch(h, d_obs, d_action)[2].sum().backward()
    only = grads()
    assert all(not w.any() and not b.any() for w, b in only["actor"]) and all(np.abs(w).max() > 0 for w, _ in only["critic"])
    with torch.no_grad():
        out = env.population_evaluate_torch(h, d_obs, d_action)
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    env.check_status()
    env.close()


K, B, P = 6, 240, 3


def _buffers(env, cap):
    import torch
    D = env.obs_dim
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    b = dict(obs=z(K + 1, B, D), action=z(K, B, dtype=torch.int32) if env.discrete else z(K, B, 2), logp=z(K, B), value=z(K + 1, B),
             reward=z(K, B), done=z(K, B, dtype=torch.uint8), trunc=z(K, B, dtype=torch.uint8))
    return b, env.terminal_list_torch(cap)


def _hand_loop(env, h, seed, first_step):
    """population_act_torch then step_torch(terminal_obs=...) K times; the terminal records as a set of (step, env, obs bytes)"""
    import torch
    b, _ = _buffers(env, 1)
    b["obs"][0].copy_(env.reset_torch())
    tobs = torch.zeros((B, env.obs_dim), dtype=torch.float32, device="cuda")
    records = set()
    for t in range(K):
        env.population_act_torch(h, b["obs"][t], seed=seed, step=first_step + t, out=dict(action=b["action"][t], logp=b["logp"][t], value=b["value"][t]))
        env.step_torch(b["action"][t], out=dict(obs=b["obs"][t + 1], reward=b["reward"][t], done=b["done"][t], trunc=b["trunc"][t]),
                       terminal_obs=tobs)
        d, to = _np(b["done"][t], tobs)
        for i in np.nonzero(d)[0]:
            records.add((t, int(i), to[i].tobytes()))
    env.population_act_torch(h, b["obs"][K], seed=seed, step=0, out=dict(value=b["value"][K]))
    return b, records


@pytest.mark.parametrize("env_id,variant", [(GOAL, "plain"), (DISCRETE, "plain"), (GOAL, "normalize_obs"), (GOAL, "reward_profiles")])
def test_rollout_equals_the_hand_written_loop(env_id, variant):
    """7: every output of rollout_population_torch bit for bit the loop of population_act_torch + step_torch; max_episode_steps = 3 puts
    truncations and auto-resets inside the call.  The terminal list is that loop's; terminal_value[t, i] of every record is member
    i // (B / P)'s critic on the record's observation; and gae_torch reads the dense values as it reads the list built from them"""
    import torch
    kw = dict(seed=21, max_episode_steps=3)
    if variant == "normalize_obs":
        kw["normalize_obs"] = True
    if variant == "reward_profiles":
        kw["reward_profiles"] = [dict(goal_sparse_reward=1.0 + m, survival_reward_scale=0.1 * m) for m in range(P)]
    ea, eb = make(env_id, B, **kw), make(env_id, B, **kw)
    if variant == "reward_profiles":
        idx = (np.arange(B) // (B // P)).astype(np.uint8)
        ea.set_env_profiles(idx); eb.set_env_profiles(idx)
    rng = np.random.default_rng(10)
    pop = _population(ea, rng, P, 64, 2)
    ha, hb = _pop_handle(ea, pop), _pop_handle(eb, pop)
    want, records = _hand_loop(ea, ha, seed=4, first_step=100)
    got, term = _buffers(eb, 1000)
    got["obs"][0].copy_(eb.reset_torch())
    dense = torch.full((K, B), float("nan"), device="cuda")
    eb.rollout_population_torch(hb, seed=4, first_step=100, terminal=term, terminal_value=dense, **got)
    eb.check_status()
    for name in want:
        w, g = _np(want[name], got[name])
        assert w.tobytes() == g.tobytes(), (name, int((w != g).sum()))
    trunc, done = _np(got["trunc"], got["done"])
    assert trunc[2].mean() > 0.9 and done.sum() >= 0.9 * B and (done & trunc).any()
    count, se, ob, tv = _np(term["count"], term["step_env"], term["obs"], dense)
    cnt = int(count[0])
    assert cnt == int(done.sum()) == len(records) <= 1000
    assert {(int(se[k, 0]), int(se[k, 1]), ob[k].tobytes()) for k in range(cnt)} == records
    # V of every record under its env's member: the member's handle, evaluated on the records of its block
    dummy = torch.zeros((cnt,), dtype=torch.int32, device="cuda") if eb.discrete else torch.zeros((cnt, 2), device="cuda")
    for m in range(P):
        v_m = _np(eb.policy_evaluate_raw_torch(eb.population_member_torch(hb, m), term["obs"][:cnt].contiguous(), dummy, out=dict(
            value=torch.empty(cnt, device="cuda")))[2])[0]
        mine = np.nonzero(se[:cnt, 1] // (B // P) == m)[0]
        assert len(mine) > 0
        assert tv[se[mine, 0], se[mine, 1]].tobytes() == v_m[mine].tobytes(), (variant, m)
    # the rollout without a list serves the same dense values where an env finished (the staging block is requested all the same)
    ec = make(env_id, B, **kw)
    if variant == "reward_profiles":
        ec.set_env_profiles(idx)
    hc = _pop_handle(ec, pop)
    again, _ = _buffers(ec, 1)
    again["obs"][0].copy_(ec.reset_torch())
    dense2 = torch.full((K, B), float("nan"), device="cuda")
    ec.rollout_population_torch(hc, seed=4, first_step=100, terminal_value=dense2, **again)
    tv2 = _np(dense2)[0]
    assert tv2[done != 0].tobytes() == tv[done != 0].tobytes() and _same(*_np(again["reward"], got["reward"]))
    ec.close()
    # GAE: dense as it stands, against the value list built from the records
    values = torch.zeros(1000, device="cuda")
    values[:cnt] = dense[term["step_env"][:cnt, 0].long(), term["step_env"][:cnt, 1].long()]
    a1, r1 = eb.gae_torch(got["reward"], got["done"], got["trunc"], got["value"][:-1], got["value"][-1], terminal_value=dense, gamma=0.97, lam=0.9)
    a2, r2 = eb.gae_torch(got["reward"], got["done"], got["trunc"], got["value"][:-1], got["value"][-1],
                          terminal=eb.value_list_torch(term, values), gamma=0.97, lam=0.9)
    a1, r1, a2, r2 = _np(a1, r1, a2, r2)
    assert not np.isnan(a1).any() and a1.tobytes() == a2.tobytes() and r1.tobytes() == r2.tobytes()
    both = (done != 0) & (trunc != 0)
    assert np.array_equal(dense_from_list(K, B, cnt, se, _np(values)[0])[both], tv[both])
    eb.check_status()
    ea.close()
    eb.close()


def _copy_member(tensors, dst, src):
    import torch
    with torch.no_grad():
        for t in tensors:
            t[dst].copy_(t[src])


def test_captured_act_and_step_follow_the_callers_tensors():
    """8a: one capture of population_act_torch + step_torch, replayed; between replays W[1].copy_(W[0]) on every tensor (PBT's exploit
    step): after it member 1's rows are the single handle's with member 0's parameters"""
    import torch
    rng = np.random.default_rng(12)
    kw = dict(seed=8, max_episode_steps=3)
    ea, eb = make(GOAL, B, **kw), make(GOAL, B, **kw)
    pop = _population(ea, rng, P, 64, 2)
    h = _pop_handle(eb, pop)
    h0 = _handle(ea, member(pop, 0))  # member 0 as a plain handle over copies
    n = B // P
    obs = eb.reset_torch().clone()
    ea.reset_torch()
    act = dict(action=torch.zeros((B, 2), device="cuda"), logp=torch.zeros(B, device="cuda"), value=torch.zeros(B, device="cuda"))
    step = dict(obs=torch.zeros((B, eb.obs_dim), device="cuda"), reward=torch.zeros(B, device="cuda"),
                done=torch.zeros(B, dtype=torch.uint8, device="cuda"), trunc=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    snap = eb.snapshot_torch()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (warm-up on the capture's stream: the first call raises the kernels' LDS limit)
        eb.population_act_torch(h, obs, seed=2, step=7, out=act)
        eb.step_torch(act["action"], out=step)
    side.synchronize()
    eb.restore_torch(snap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eb.population_act_torch(h, obs, seed=2, step=7, out=act)
        eb.step_torch(act["action"], out=step)
    for copied in (False, True):
        if copied:
            _copy_member(h.tensors, 1, 0)
        for t in list(act.values()) + [step["obs"], step["reward"]]:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = _np(act["action"], act["logp"], act["value"])
        for m in range(P):
            want = _np(*ea.policy_act_torch(_handle(ea, member(pop, m)) if not (copied and m == 1) else h0, obs, seed=2, step=7))
            rows = slice(m * n, (m + 1) * n)
            assert all(g[rows].tobytes() == w[rows].tobytes() for g, w in zip(got, want)), (copied, m)
        twin = ea.step_torch(act["action"].clone())  # the eager twin takes the replay's actions
        for name, w in zip(("obs", "reward", "done", "trunc"), twin):
            assert _same(*_np(step[name], w)), (copied, name)
    eb.check_status()
    ea.close()
    eb.close()


def test_captured_evaluate_and_grad_follow_the_callers_tensors():
    """8b: population_evaluate_raw_torch + population_grad_torch captured after the warm-up call that sizes the workspace; replays equal the
    members' single calls, before and after W[1].copy_(W[0]); without a warm-up the grad call raises inside the capture"""
    import torch
    n = 200
    env = make(GOAL, P)
    rng = np.random.default_rng(15)
    pop = _population(env, rng, P, 64, 2)
    h = _pop_handle(env, pop)
    obs, action = _rows(env, rng, P, n)
    d_obs, d_action = _dev(obs), _dev(action)
    g = [_dev(rng.standard_normal((P, n)).astype(np.float32)) for _ in range(3)]
    fwd = {k: torch.empty((P, n), device="cuda") for k in ("logp", "entropy", "value")}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # the warm-up, on the capture's stream
        env.population_evaluate_raw_torch(h, d_obs, d_action, out=fwd)
        out = env.population_grad_torch(h, d_obs, d_action, *g)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        env.population_evaluate_raw_torch(h, d_obs, d_action, out=fwd)
        env.population_grad_torch(h, d_obs, d_action, *g, out=out)
    for copied in (False, True):
        if copied:
            _copy_member(h.tensors, 1, 0)
        for t in list(fwd.values()) + [x for pairs in (out["actor"], out["critic"]) for pair in pairs for x in pair] + [out["log_std"]]:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        got, got_fwd = _stacked_np(out), _np(fwd["logp"], fwd["entropy"], fwd["value"])
        for m in range(P):
            src = 0 if copied and m == 1 else m
            single = _handle(env, member(pop, src))  # a plain handle over copies of the source member's parameters
            want_fwd = _np(*env.policy_evaluate_raw_torch(single, d_obs[m], d_action[m]))
            assert all(gf[m].tobytes() == w.tobytes() for gf, w in zip(got_fwd, want_fwd)), (copied, m)
            want = flat(_stacked_np(env.policy_grad_torch(single, d_obs[m], d_action[m], *[x[m] for x in g])))
            mine = flat_member(got, m)
            for k in want:
                assert mine[k].tobytes() == want[k].tobytes(), (copied, m, k)
    h2 = _pop_handle(env, pop)
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="warm-up"):
        with torch.cuda.graph(graph2, stream=side):
            env.population_grad_torch(h2, d_obs, d_action, *g, out=out)
    torch.cuda.synchronize()
    assert h2.workspace is None
    env.check_status()
    env.close()


def test_native_refusals():
    """9: every refusal returns the error with a message, enqueues nothing and leaves the outputs untouched"""
    import torch
    from space_gym_amd import _native
    n, Bn = 40, 12
    env = make(GOAL, Bn)
    rng = np.random.default_rng(16)
    pop = _population(env, rng, 3, 16, 1)
    h = _pop_handle(env, pop)
    h_nc = _pop_handle(env, dict(pop, critic=None))
    lib, s = env._lib, env._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    obs_b = torch.zeros((Bn, env.obs_dim), device="cuda")
    a, lp, v = torch.full((Bn, 2), 7.0, device="cuda"), torch.full((Bn,), 7.0, device="cuda"), torch.full((Bn,), 7.0, device="cuda")

    def act(policy, members, o, ao, lo, vo, match):
        assert lib.sg_policy_population_act_device(env._h, C.byref(policy.struct), members, ptr(o), 0, 0, 0, ptr(ao), ptr(lo), ptr(vo), s) == -1
        assert match in lib.sg_last_error(env._h), lib.sg_last_error(env._h)

    act(h, 0, obs_b, a, lp, v, b"members must be 1 .. 65535")
    act(h, -1, obs_b, a, lp, v, b"members must be 1 .. 65535")
    act(h, 65536, obs_b, a, lp, v, b"members must be 1 .. 65535")
    act(h, 5, obs_b, a, lp, v, b"must divide num_envs")
    act(h, 24, obs_b, a, lp, v, b"must divide num_envs")
    act(h, 3, None, a, lp, v, b"null obs")
    act(h, 3, obs_b, None, None, None, b"no output")
    act(h, 3, obs_b, None, lp, v, b"logp_out without action_out")
    act(h_nc, 3, obs_b, a, lp, v, b"no critic")
    for field, bad in (("hidden", 129), ("n_hidden", 0), ("activation", 2), ("struct_size", 8), ("head", 6), ("reserved", 1)):
        keep = getattr(h.struct, field)
        setattr(h.struct, field, bad)
        act(h, 3, obs_b, a, lp, v, {"head": b"head has 6 outputs"}.get(field, field.encode()))  # whatever policy_check refuses
        setattr(h.struct, field, keep)
    # the rollout
    Kr = 2
    z = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device="cuda")
    r = dict(obs=z(Kr + 1, Bn, env.obs_dim), action=z(Kr, Bn, 2), logp=z(Kr, Bn), value=z(Kr + 1, Bn), reward=z(Kr, Bn),
             done=z(Kr, Bn, dtype=torch.uint8), trunc=z(Kr, Bn, dtype=torch.uint8))
    tv = z(Kr, Bn)

    def roll(policy, members, steps, match, value=r["value"], terminal_value=tv, obs=r["obs"]):
        rc = lib.sg_rollout_policy_population_device(env._h, steps, C.byref(policy.struct), members, 0, 0, 0, ptr(obs), ptr(r["action"]), ptr(r["logp"]),
                                                     ptr(value), ptr(r["reward"]), ptr(r["done"]), ptr(r["trunc"]), None, ptr(terminal_value), s)
        assert rc == -1 and match in lib.sg_last_error(env._h), lib.sg_last_error(env._h)

    roll(h, 0, Kr, b"members must be")
    roll(h, 5, Kr, b"must divide num_envs")
    roll(h, 3, 0, b"n_steps must be at least 1")
    roll(h, 3, Kr, b"null buffer", obs=None)
    roll(h_nc, 3, Kr, b"no critic")
    roll(h_nc, 3, Kr, b"no critic", value=None)  # terminal_value alone needs the critic too
    # evaluate and grad
    obs, action = torch.zeros((3, n, env.obs_dim), device="cuda"), torch.zeros((3, n, 2), device="cuda")
    outs = [torch.full((3, n), 7.0, device="cuda") for _ in range(3)]

    def ev(policy, members, rows, o, ac, lo, en, vo, match):
        assert lib.sg_policy_population_evaluate_device(env._h, C.byref(policy.struct), members, rows, ptr(o), ptr(ac), ptr(lo), ptr(en), ptr(vo), s) == -1
        assert match in lib.sg_last_error(env._h), lib.sg_last_error(env._h)

    ev(h, 0, n, obs, action, *outs, b"members must be")
    ev(h, 65536, n, obs, action, *outs, b"members must be")
    ev(h, 3, 0, obs, action, *outs, b"n must be")
    ev(h, 3, 2 ** 30, obs, action, *outs, b"members x n must be at most 2^31 - 1")
    ev(h, 3, n, None, action, *outs, b"null obs")
    ev(h, 3, n, obs, None, *outs, b"null action")
    ev(h, 3, n, obs, action, None, None, None, b"no output")
    ev(h_nc, 3, n, obs, action, *outs, b"no critic")
    ones = torch.ones((3, n), device="cuda")
    full = env.population_grad_torch(h, obs, action, ones, ones, ones)
    every = [x for pairs in (full["actor"], full["critic"]) for pair in pairs for x in pair] + [full["log_std"]]
    for t in every:
        t.fill_(7.0)
    ws = h.workspace
    total = sum(t.numel() for t in h.tensors) // 3
    need = lambda members, rows: lib.sg_policy_population_grad_workspace_bytes(env._h, C.byref(h.struct), members, rows)
    assert need(3, n) == 4 * 3 * total == ws.numel() and need(1, n) == lib.sg_policy_grad_workspace_bytes(env._h, C.byref(h.struct), n)
    assert need(3, 257) == 2 * need(3, n) and need(3, 10 ** 7) == 85 * need(3, n)  # G = min(ceil(n / 256), 256 // 3)
    assert need(256, 10 ** 6) == 4 * 256 * total and need(1000, 10 ** 6) == 4 * 1000 * total  # one workgroup per member from P = 129 on
    assert need(0, n) == 0 and b"members must be" in lib.sg_last_error(env._h) and need(3, 0) == 0

    def struct(critic=True, **over):
        g = _native.SgPolicyGrads(struct_size=C.sizeof(_native.SgPolicyGrads))
        for l, (w, b) in enumerate(full["actor"]):
            g.actor.weight[l], g.actor.bias[l] = w.data_ptr(), b.data_ptr()
        if critic:
            for l, (w, b) in enumerate(full["critic"]):
                g.critic.weight[l], g.critic.bias[l] = w.data_ptr(), b.data_ptr()
        g.log_std = full["log_std"].data_ptr()
        for k, val in over.items():
            setattr(g, k, val)
        return g

    def gr(policy, members, rows, o, ac, gv, g, w, wbytes, match):
        rc = lib.sg_policy_population_grad_device(env._h, C.byref(policy.struct), members, rows, ptr(o), ptr(ac), ptr(ones), None, ptr(gv),
                                                  C.byref(g) if g is not None else None, ptr(w), wbytes, s)
        assert rc == -1 and match in lib.sg_last_error(env._h), lib.sg_last_error(env._h)

    gr(h, 0, n, obs, action, ones, struct(), ws, ws.numel(), b"members must be")
    gr(h, 65536, n, obs, action, ones, struct(), ws, ws.numel(), b"members must be")
    gr(h, 3, 0, obs, action, ones, struct(), ws, ws.numel(), b"n must be")
    gr(h, 3, 2 ** 30, obs, action, ones, struct(), ws, ws.numel(), b"members x n")
    gr(h, 3, n, None, action, ones, struct(), ws, ws.numel(), b"null obs")
    gr(h, 3, n, obs, None, ones, struct(), ws, ws.numel(), b"null action")
    gr(h, 3, n, obs, action, ones, None, ws, ws.numel(), b"null grads")
    gr(h, 3, n, obs, action, ones, struct(struct_size=8), ws, ws.numel(), b"struct_size")
    gr(h, 3, n, obs, action, ones, struct(log_std=None), ws, ws.numel(), b"log_std")
    gr(h, 3, n, obs, action, ones, struct(critic=False), ws, ws.numel(), b"of the critic")
    gr(h, 3, n, obs, action, ones, struct(), None, ws.numel(), b"null workspace")
    gr(h, 3, n, obs, action, ones, struct(), ws, ws.numel() - 1, b"workspace of")
    gr(h_nc, 3, n, obs, action, ones, struct(critic=False), ws, ws.numel(), b"g_value given, but the policy has no critic")
    gr(h_nc, 3, n, obs, action, None, struct(), ws, ws.numel(), b"critic gradients given")
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in [a, lp, v, tv] + list(r.values()) + outs + every)
    # the handles still work
    assert env.population_act_torch(h_nc, obs_b)[2] is None
    env.population_grad_torch(h, obs, action, ones)
    torch.cuda.synchronize()
    env.check_status()
    env.close()
