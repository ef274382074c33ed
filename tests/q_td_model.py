"""The contract of sg_q_td_grad_device (include/spacegym.h) in NumPy: the TD critic update of SAC, TD3 and DDPG on a
replay batch -- target, Huber loss, statistics, the loss gradient by each critic's output and, through tests/q_model.py, the gradient
of every parameter of the online critics.  The target action is an input.  For row i, Qc the critic c on [obs | action]:
    a'_d    = next_action[i][d]
              noise given:  e = clip(noise_std * noise[i][d], -noise_clip, noise_clip);  a'_d = clip(a'_d + e, -action_clip, action_clip)
              (no noise: a' used as given, never clamped)
    q_next  = minimum(Q1_target(next_obs[i], a'), Q2_target(next_obs[i], a'))            (one critic: Q1_target)
              next_logp given:  q_next = q_next - alpha * next_logp[i]
    y       = terminated[i] ? reward[i] : reward[i] + discount[i] * q_next                (a where: a terminated row never multiplies its q_next)
    per critic c of the online nets:  q_c = Qc(obs[i], action[i]);  td_c = q_c - y
              cl_c = clip(td_c, -delta, delta);  w = weight[i] (1 without weights);  g_c = (w * cl_c) / n
              l_c  = w * (|td_c| <= delta ? 0.5 td_c^2 : delta (|td_c| - 0.5 delta))
    loss    = (1 / n) sum_i (l_1 + l_2)
delta = inf gives 0.5 td^2 per critic: half of the sum of the two mean squared errors of CleanRL's and SB3's TD3.  np.minimum and
np.clip hand a NaN on, as torch.minimum and torch.clamp do and as the kernels do; no row is set aside.

float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every per-row term is formed
in float32, one rounding per operation as written above, and every sum over the rows is plain sequential float32 accumulation, as
q_model's.  The scalars (alpha, noise_std, the clips, delta) are the float32 values the engine holds, in either mode.

The module also holds the cases tests/test_q_td.py (CPU) and tests/test_gpu_q_td.py share."""
import numpy as np

from q_model import _sum_rows, q_evaluate, q_flat, random_qnet

STATS = ("loss", "td1_abs_mean", "td2_abs_mean", "td_abs_max", "q1_mean", "q2_mean", "target_mean", "clip_fraction", "weight_mean")
ROWS = ("td1", "td2", "q1", "q2", "target", "q_next", "g1", "g2", "td_abs")
flat = q_flat


def target_action(next_action, noise=None, noise_std=0.2, noise_clip=0.5, action_clip=1.0, dtype=np.float64):
    """(a', e clamped bool [n, 2], a' clamped bool [n, 2]); without noise a' is next_action and nothing is clamped"""
    dtype = np.dtype(dtype).type
    a = np.asarray(next_action).astype(dtype)
    none = np.zeros(a.shape, bool)
    if noise is None:
        return a, none, none
    std, nc, ac = (dtype(np.float32(v)) for v in (noise_std, noise_clip, action_clip))
    raw = (std * np.asarray(noise).astype(dtype)).astype(dtype)
    e = np.clip(raw, -nc, nc)
    moved = (a + e).astype(dtype)
    return np.clip(moved, -ac, ac).astype(dtype), np.abs(raw) > nc, np.abs(moved) > ac


def td(online, target, batch, next_action, next_logp=None, alpha=0.2, noise=None, noise_std=0.2, noise_clip=0.5, action_clip=1.0,
       huber_delta=float("inf"), weight=None, activation="relu", dtype=np.float64):
    """online, target: lists of one or two nets [(W, b), ...] on obs_dim + 2 inputs with a head of 1.  batch: dict obs [n, D] / action
    [n, 2] / reward / next_obs / terminated / discount of NumPy arrays.  Returns dict critics: per online critic [(dW, db), ...]
    (q_model.q_flat takes it), stats [9] named by STATS, rows (dict of [n] arrays named by ROWS; the critic-2 ones None with one
    critic), clipped: per critic bool [n], noise_clamped / action_clamped bool [n, 2]."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(batch["obs"])
    n, C = obs.shape[0], len(online)
    assert len(target) == C
    col = lambda k: np.asarray(batch[k]).astype(dtype)
    a2, noise_clamped, action_clamped = target_action(next_action, noise, noise_std, noise_clip, action_clip, dtype)
    qt = q_evaluate(target, batch["next_obs"], a2, activation=activation, dtype=dtype, grads=False)["q"]
    with np.errstate(invalid="ignore", over="ignore"):
        q_next = qt[0] if C == 1 else np.minimum(qt[0], qt[1])
        if next_logp is not None:
            q_next = (q_next - (dtype(np.float32(alpha)) * np.asarray(next_logp).astype(dtype)).astype(dtype)).astype(dtype)
        r, d = col("reward"), col("discount")
        y = np.where(np.asarray(batch["terminated"]) != 0, r, r + (d * q_next).astype(dtype)).astype(dtype)
    delta, nf, half = dtype(np.float32(huber_delta)), dtype(n), dtype(0.5)
    w = np.ones(n, dtype) if weight is None else np.asarray(weight).astype(dtype)
    qs = q_evaluate(online, obs, batch["action"], activation=activation, dtype=dtype, grads=False)["q"]
    tds, gs, ls, clipped = [], [], [], []
    for c in range(C):
        err = (qs[c] - y).astype(dtype)
        ad = np.abs(err)
        gs.append(((w * np.clip(err, -delta, delta)).astype(dtype) / nf).astype(dtype))
        with np.errstate(invalid="ignore"):
            ls.append((w * np.where(ad <= delta, half * (err * err), delta * (ad - half * delta)).astype(dtype)).astype(dtype))
        tds.append(err)
        clipped.append(ad > delta)
    grads = q_evaluate(online, obs, batch["action"], gs[0], gs[1] if C == 2 else None, activation=activation, dtype=dtype)["critics"]
    mean_of = lambda v: _sum_rows(np.asarray(v, dtype), dtype) / nf
    s = np.zeros(len(STATS), dtype)
    s[0] = mean_of(ls[0] if C == 1 else (ls[0] + ls[1]).astype(dtype))
    s[1], s[4] = mean_of(np.abs(tds[0])), mean_of(qs[0])
    s[3] = max(float(np.abs(t).max()) for t in tds)
    if C == 2:
        s[2], s[5] = mean_of(np.abs(tds[1])), mean_of(qs[1])
    s[6], s[8] = mean_of(y), mean_of(w)
    s[7] = _sum_rows(sum(cl.astype(dtype) for cl in clipped).astype(dtype), dtype) / (dtype(C) * nf)
    td_abs = np.abs(tds[0]) if C == 1 else (half * (np.abs(tds[0]) + np.abs(tds[1])).astype(dtype)).astype(dtype)
    second = lambda v: v[1] if C == 2 else None
    rows = dict(td1=tds[0], td2=second(tds), q1=qs[0], q2=second(qs), target=y, q_next=q_next, g1=gs[0], g2=second(gs), td_abs=td_abs)
    return dict(critics=grads, stats=s, rows=rows, clipped=clipped, noise_clamped=noise_clamped, action_clamped=action_clamped)


def case(obs_dim, n, hidden, n_hidden, n_critics, seed):
    """The shared inputs of a (net, n) case, CPU and GPU tests alike: online and target critics, a batch with the continuous sampler's
    columns and dtypes (a tenth of the rows terminated, discounts gamma^steps of a 3-step sampler), the target action in +-1.3 (so that
    the action clamp binds on a share of the rows), its log-prob, the smoothing noise and importance weights in (0.2, 1]"""
    rng = np.random.default_rng([seed, obs_dim, n, hidden, n_hidden, n_critics, 32])
    online, target = random_qnet(rng, obs_dim, hidden, n_hidden, n_critics), random_qnet(rng, obs_dim, hidden, n_hidden, n_critics)
    batch = dict(obs=rng.standard_normal((n, obs_dim)).astype(np.float32), action=rng.uniform(-1, 1, (n, 2)).astype(np.float32),
                 reward=(1.5 * rng.standard_normal(n)).astype(np.float32), next_obs=rng.standard_normal((n, obs_dim)).astype(np.float32),
                 terminated=(rng.uniform(size=n) < 0.1).astype(np.uint8),
                 discount=(np.float32(0.99) ** rng.integers(1, 4, n)).astype(np.float32))
    return dict(online=online, target=target, batch=batch, weight=rng.uniform(0.2, 1.0, n).astype(np.float32),
                next_action=rng.uniform(-1.3, 1.3, (n, 2)).astype(np.float32), next_logp=(-1.0 + 1.5 * rng.standard_normal(n)).astype(np.float32),
                noise=rng.standard_normal((n, 2)).astype(np.float32))


# The options of a case by its form.  The smoothing noise is clipped at 1.25 of its standard deviation, not at TD3's 2.5, so that both
# branches of the noise clamp hold a tenth of the draws at every row count
FORMS = ("sac", "td3", "plain")
ALPHA, NOISE_STD, NOISE_CLIP, ACTION_CLIP = 0.2, 0.2, 0.25, 1.0


def options(c, form, huber_delta, weighted):
    """the keyword arguments td() and q_td_grad_torch share, of NumPy arrays"""
    kw = dict(next_action=c["next_action"], huber_delta=huber_delta, weight=c["weight"] if weighted else None)
    if form == "sac":
        kw.update(next_logp=c["next_logp"], alpha=ALPHA)
    elif form == "td3":
        kw.update(noise=c["noise"], noise_std=NOISE_STD, noise_clip=NOISE_CLIP, action_clip=ACTION_CLIP)
    return kw


NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS
GRAD_NS = [1, 200, 2049]
BIG_N = 256 * 64 + 300  # hidden 128 has workgroups of 64 rows: past the grid cap of 256 they take a second row tile
CLASS3_NET = (80, 2)  # tests/net_widths.py's class of hidden 65 .. 96: NT = 3
# case(..., seed=CASE_SEED + n + hidden): chosen on the CPU, by a search over 0, 1, 2, ... on this model alone, as the first seed at
# which every case keeps tests/test_q_td.py's conditions.  Seeds 0 .. 29 fail them, nearly all at the Huber margin of the BIG_N case:
# with 2 x 16 684 TD errors of density about 0.3 near 1, two are expected within 1e-4 of huber_delta
CASE_SEED = 30
HUBER_MARGIN, BRANCH_SHARE = 1e-4, 0.1


def grad_cases():
    """(obs_dim, n, hidden, n_hidden, n_critics, activation, form, huber_delta, weighted): GRAD_NS over NETS, the second row tile past
    the grid cap at hidden 128, and one net of width class 3; the options rotate over the cases so that the three forms, Huber and the
    squared loss, weights and none each meet every row count, and two cases have one critic (DDPG).  obs_dim 15: GoalContinuous3P-v0,
    10: KeplerCircleOrbit-v0."""
    shapes = [(15 if i % 2 == 0 else 10, n, hidden, n_hidden) for n in GRAD_NS for i, (hidden, n_hidden) in enumerate(NETS)]
    shapes += [(15, BIG_N, 128, 1), (10, 200) + CLASS3_NET]
    cases = []
    for v, (obs_dim, n, hidden, n_hidden) in enumerate(shapes):
        cases.append((obs_dim, n, hidden, n_hidden, 1 if v in (5, 10) else 2, ("tanh", "relu")[(v // 2) % 2], FORMS[v % 3],
                      float("inf") if (v // 3) % 2 else 1.0, v % 4 < 2))
    return cases


def grad_case(obs_dim, n, hidden, n_hidden, n_critics):
    return case(obs_dim, n, hidden, n_hidden, n_critics, seed=CASE_SEED + n + hidden)


def reference(c, activation, form, huber_delta, weighted, dtype):
    return td(c["online"], c["target"], c["batch"], activation=activation, dtype=dtype, **options(c, form, huber_delta, weighted))


_regime = {}


def regime_case():
    """(case, activation, form, huber_delta, weighted) of the one trained-regime case: tests/net_regimes.py's q family at (64, 2, relu)
    -- its critics (Q values in the hundreds) as the online nets, its rows as (obs, action); the target critics are the online ones
    swapped and shrunk by 3 %, the rest of the batch is case()'s.  TD3 form, huber_delta 1 (most rows clipped), weights.  Made once"""
    if not _regime:
        import net_regimes
        hidden, n_hidden, activation = net_regimes.NETS[1]
        env_id = net_regimes.ids_of(hidden, n_hidden)[0]
        r = net_regimes.case("q", env_id, hidden, n_hidden, activation)
        c = case(r["obs"].shape[1], net_regimes.N, hidden, n_hidden, 2, seed=net_regimes.N + hidden)
        shrink = np.float32(0.97)
        c.update(online=r["critics"], target=[[(W * shrink, b * shrink) for W, b in net] for net in r["critics"][::-1]], env_id=env_id)
        c["batch"].update(obs=r["obs"], action=r["action"])
        _regime["case"] = (c, activation, "td3", 1.0, True)
    return _regime["case"]


def regime_reference(dtype):
    """the model of regime_case() in float64 or float32, computed once per process and left unchanged"""
    key = np.dtype(dtype).name
    if key not in _regime:
        c, activation, form, huber_delta, weighted = regime_case()
        _regime[key] = reference(c, activation, form, huber_delta, weighted, dtype)
    return _regime[key]


# The width classes (tests/net_widths.py): the family's entry in test_gpu_net_widths.FAMILY_KERNELS, which tests/test_net_widths.py holds
# against the compiled engine's kernel templates, and the nets tests/test_gpu_q_td.py runs for it: net_widths' table and the widest
# net of class 4, each on net_widths.ids_of's continuous id
WIDTH_FAMILY = ("q_td", ("q_td_target_kernel", "q_td_grad_kernel"))


def register_width_family():
    """names the two kernel templates of sg_q_td.inc in FAMILY_KERNELS.  Both new test modules call it when they are imported, which
    pytest does for every module it collects before it runs a test; tests/test_gpu_q_td.py's width test is the family's test"""
    import test_gpu_net_widths
    test_gpu_net_widths.FAMILY_KERNELS.setdefault(*WIDTH_FAMILY)


def width_cases():
    """[(hidden, n_hidden, activation)]: net_widths.cases() and (128, 3)"""
    import net_widths
    return net_widths.cases() + [(128, 3, "relu")]
