"""The contract of sg_q_actor_squashed_grad_device / sg_q_actor_gaussian_grad_device (include/spacegym.h) in NumPy:
the actor update of SAC, TD3 and DDPG through one or two Q critics -- action, log-prob, the critics' values and action gradients, the
loss, its statistics and, through tests/squashed_model.py and tests/q_model.py, the gradient of every parameter of the actor.  For row i:
    squashed: (a, logp) = squashed_model.sample(actor, obs, eps)            (eps None: zeros)
    gaussian: a = q_model.action(policy, obs, eps): mean + exp(log_std) eps;  logp = 0, alpha is 0
    critic c: q_c = Qc(obs[i], a);  dq_c = d Qc / d a                       (q_model.q_evaluate with g_qc = 1)
    q_select = 1: sel2 = q2 < q1 or q2 is NaN (torch.minimum's choice, ties to critic 1);  q_select = 0: critic 1 alone
    q_sel = sel2 ? q2 : q1;  loss_i = alpha logp - q_sel;  loss = mean_i loss_i
    g_action = -dq_sel / n;  g_logp = alpha / n  ->  the actor's backward of squashed_model.sample / q_model.action
    log_alpha_grad = -(mean logp + target_entropy)                          (SB3's temperature loss by log_alpha; gaussian: 0)

float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every per-row term is formed
in float32, one rounding per operation as written above, and every sum over the rows is plain sequential float32 accumulation.  alpha
and target_entropy are the float32 values the engine holds, in either mode.

The module also holds the cases tests/test_q_actor.py (CPU) and tests/test_gpu_q_actor.py share."""
import numpy as np

import q_model
import squashed_model
from policy_grad_model import _sum_rows, flat, grad_tolerances  # noqa: F401  (flat, grad_tolerances: re-exported)
from policy_model import random_policy
from q_model import random_qnet

STATS = ("loss", "logp_mean", "q1_mean", "q2_mean", "q_sel_mean", "critic2_fraction", "action_abs_mean", "dq_da_abs_max", "log_alpha_grad")
ROWS = ("action", "logp", "q1", "q2", "q_sel", "dq1_da", "dq2_da", "g_action")
FORMS = ("squashed", "gaussian")
BOUNDS = squashed_model.BOUNDS  # the cases' clamp of the raw log_std: dense random heads land below, inside and above it
ALPHA, TARGET_ENTROPY = 0.2, -2.0
Q_MARGIN, BRANCH_SHARE = 1e-4, 0.1


def default_select(form, n_critics):
    return 1 if form == "squashed" and n_critics == 2 else 0


def actor_grad(actor, critics, obs, eps=None, alpha=ALPHA, q_select=None, target_entropy=TARGET_ENTROPY, form="squashed", bounds=BOUNDS,
               activation="relu", q_activation=None, dtype=np.float64):
    """actor: [(W, b), ...] with a head of 4 (squashed), or policy_model's dict (gaussian).  critics: one or two nets on obs_dim + 2
    inputs with a head of 1.  Returns dict actor: [(dW, db), ...] (gaussian: and log_std [2]; flat() takes it), stats [9] named by STATS,
    rows (dict named by ROWS; q2 / dq2_da None when critic 2 does not run), sel2 bool [n], inside bool [n, 2] (squashed: raw within the
    clamp)."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(obs)
    n = obs.shape[0]
    q_activation = q_activation or activation
    two = default_select(form, len(critics)) if q_select is None else int(q_select)
    assert not two or len(critics) == 2
    al, te, nf = dtype(np.float32(alpha)), dtype(np.float32(target_entropy)), dtype(n)
    if form == "squashed":
        fwd = squashed_model.sample(actor, obs, eps, bounds=bounds, activation=activation, dtype=dtype)
        a, logp = fwd["action"], fwd["logp"]
        lo, hi = dtype(np.float32(bounds[0])), dtype(np.float32(bounds[1]))
        inside = (fwd["raw"] >= lo) & (fwd["raw"] <= hi)
    else:
        assert float(al) == 0.0
        a = q_model.action(actor, obs, eps, activation=activation, dtype=dtype)["action"].astype(dtype)
        logp, inside = np.zeros(n, dtype), None
    ones = np.ones(n, dtype)
    qs, dqs = [], []
    for c in range(2 if two else 1):
        r = q_model.q_evaluate([critics[c]], obs, a, ones, activation=q_activation, dtype=dtype)
        qs.append(r["q"][0].astype(dtype))
        dqs.append(r["action"].astype(dtype))
    with np.errstate(invalid="ignore"):
        sel2 = ((qs[1] < qs[0]) | np.isnan(qs[1])) if two else np.zeros(n, bool)
    q_sel = np.where(sel2, qs[1], qs[0]) if two else qs[0]
    dq_sel = np.where(sel2[:, None], dqs[1], dqs[0]) if two else dqs[0]
    loss_i = ((al * logp).astype(dtype) - q_sel).astype(dtype)
    ga = ((-dq_sel) / nf).astype(dtype)
    gl = np.full(n, al / nf, dtype)
    if form == "squashed":
        out = dict(actor=squashed_model.sample(actor, obs, eps, ga, gl, bounds=bounds, activation=activation, dtype=dtype)["actor"])
    else:
        back = q_model.action(actor, obs, eps, ga, activation=activation, dtype=dtype)
        out = dict(actor=back["actor"], log_std=back["log_std"] if eps is not None else np.zeros(2, dtype))
    mean_of = lambda v: _sum_rows(np.asarray(v, dtype), dtype) / nf
    s = np.zeros(len(STATS), dtype)
    s[0], s[1], s[2], s[4] = mean_of(loss_i), mean_of(logp), mean_of(qs[0]), mean_of(q_sel)
    if two:
        s[3], s[5] = mean_of(qs[1]), mean_of(sel2.astype(dtype))
    s[6] = mean_of((dtype(0.5) * (np.abs(a[:, 0]) + np.abs(a[:, 1])).astype(dtype)).astype(dtype))
    s[7] = np.max([np.abs(d).max() for d in dqs])  # (np.max hands a NaN on, as the kernel's maximum does)
    s[8] = -(s[1] + te) if form == "squashed" else dtype(0)
    second = lambda v: v[1] if two else None
    rows = dict(action=a, logp=logp, q1=qs[0], q2=second(qs), q_sel=q_sel, dq1_da=dqs[0], dq2_da=second(dqs), g_action=ga)
    out.update(stats=s, rows=rows, sel2=sel2, inside=inside)
    return out


def case(obs_dim, n, actor_net, q_net, n_critics, form, activation, eps_given, seed, bounds=BOUNDS):
    """The shared inputs of a case, CPU and GPU tests alike: the actor (squashed: squashed_model.random_squashed's; gaussian:
    policy_model.random_policy's, with its own critic, which the call leaves alone), obs [n, D], eps [n, 2] and the critics, all float32.
    Where n >= 200 the squashed actor's two raw log_std outputs are shifted and scaled to mean 0 and spread 0.75 over the case's rows
    (both branches of the clamp (-0.5, 0.5) then hold a good share of the components), and each critic's head bias is moved so that its
    float64 mean over the case's rows, at the case's own actions, is 0: a dense random head bias would put one critic below the other
    on every row.  Then any row whose float64 raw_d lies within
    squashed_model.MARGIN of a clamp bound, or whose two critics lie within twice Q_MARGIN max(1, |q|) of each other, is redrawn
    (observation and noise, deterministically, from the case's own generator) until none does: a float32 / float64 disagreement about
    the clamp mask or the selected critic would move a summed gradient by O(1).  No row is left out."""
    (hidden, n_hidden), (q_hidden, q_layers) = actor_net, q_net
    rng = np.random.default_rng([seed, obs_dim, n, hidden, n_hidden, q_hidden, q_layers, n_critics, FORMS.index(form), 33])
    if form == "squashed":
        actor = squashed_model.random_squashed(rng, obs_dim, hidden, n_hidden)
    else:
        actor = random_policy(rng, obs_dim, hidden, n_hidden, 2, critic=True, continuous=True)
    obs, eps = rng.standard_normal((n, obs_dim)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    critics = random_qnet(rng, obs_dim, q_hidden, q_layers, n_critics)
    lo, hi = float(np.float32(bounds[0])), float(np.float32(bounds[1]))

    def forward():
        """float64: (near a clamp bound bool [n], [q_c])"""
        e = eps if eps_given else None
        if form == "squashed":
            f = squashed_model.sample(actor, obs, e, bounds=bounds, activation=activation)
            near = (np.minimum(np.abs(f["raw"] - lo), np.abs(f["raw"] - hi)) < squashed_model.MARGIN).any(axis=1)
        else:
            f, near = q_model.action(actor, obs, e, activation=activation), np.zeros(n, bool)
        return near, [q_model.q_evaluate([net], obs, f["action"], activation=activation, grads=False)["q"][0] for net in critics]
    if n >= 200 and form == "squashed":  # the raw log_std outputs about 0 with a spread of 0.75: about half of them inside the clamp
        raw = squashed_model.sample(actor, obs, None, bounds=bounds, activation=activation)["raw"]
        W, b = actor[-1]
        gain = (np.float32(0.75) / np.maximum(raw.std(axis=0), 1e-3)).astype(np.float32)
        W[2:] *= gain[:, None]
        b[2:] = ((b[2:] - raw.mean(axis=0)) * gain).astype(np.float32)
    if n >= 200:
        for net, q in zip(critics, forward()[1]):
            net[-1][1][0] -= np.float32(q.mean())
    for _ in range(100):
        near, qs = forward()
        if n_critics == 2:
            near = near | (np.abs(qs[0] - qs[1]) <= 2 * Q_MARGIN * np.maximum(1.0, np.maximum(np.abs(qs[0]), np.abs(qs[1]))))
        if not near.any():
            break
        k = int(near.sum())
        obs[near], eps[near] = rng.standard_normal((k, obs_dim)).astype(np.float32), rng.standard_normal((k, 2)).astype(np.float32)
    else:
        raise AssertionError("case: rows near a clamp bound or with two critics alike remain")
    return dict(actor=actor, critics=critics, obs=obs, eps=eps, form=form)


NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS
CLASS3_NET = (80, 2)  # tests/net_widths.py's class of hidden 65 .. 96: NT = 3
GRAD_NS = [1, 200, 2049]
BIG_N = 256 * 64 + 300  # hidden 128 has workgroups of 64 rows: past the grid cap of 256 they take a second row tile (first = false)
# (actor net, critic net): the row counts of the two classes' tiles differ (256 against 64), differ the other way (64 against 128), and
# are both 64 in two different classes
MIXED = [((32, 1), (128, 3)), ((128, 2), (33, 2)), ((96, 2), (128, 3))]
MIXED_N = 200
GRAD_ROWS = {1: 256, 2: 128, 3: 64, 4: 64}  # policy_grad_block by class


def same_tile(actor_net, q_net):
    """the fused kernel's row tile (of the larger class) is the actor's own grad call's: the gradients are then equal to the bit"""
    ca, cq = -(-actor_net[0] // 32), -(-q_net[0] // 32)
    return GRAD_ROWS[max(ca, cq)] == GRAD_ROWS[ca]


def grad_cases():
    """(obs_dim, n, actor net, critic net, n_critics, form, activation, eps given, q_select): GRAD_NS over NETS and CLASS3_NET for both
    nets, the second row tile past the grid cap at hidden 128, and the three mixed pairs; the options rotate so that both forms, both
    activations, eps given and None, one and two critics and q_select 0 on two critics each meet every row count.  q_select None is the
    default of the form.  obs_dim 15: GoalContinuous3P-v0, 10: KeplerCircleOrbit-v0."""
    shapes = [(15 if i % 2 == 0 else 10, n, net, net) for n in GRAD_NS for i, net in enumerate(NETS + [CLASS3_NET])]
    shapes += [(15, BIG_N, (128, 1), (128, 1))] + [(10 if i == 1 else 15, MIXED_N, a, q) for i, (a, q) in enumerate(MIXED)]
    cases = []
    for v, (obs_dim, n, a, q) in enumerate(shapes):
        form = FORMS[0] if v % 3 != 2 else FORMS[1]
        n_critics = 1 if v in (4, 8, 11) else 2
        q_select = 0 if v in (6, 13) else (1 if form == "gaussian" and n_critics == 2 and v % 2 else None)
        cases.append((obs_dim, n, a, q, n_critics, form, ("tanh", "relu")[(v // 2) % 2], v % 5 != 3, q_select))
    return cases


def options(c, activation, eps_given, q_select):
    """the keyword arguments actor_grad() takes of a case"""
    return dict(eps=c["eps"] if eps_given else None, alpha=ALPHA if c["form"] == "squashed" else 0.0, q_select=q_select, form=c["form"],
                activation=activation)


def reference(c, activation, eps_given, q_select, dtype):
    return actor_grad(c["actor"], c["critics"], c["obs"], dtype=dtype, **options(c, activation, eps_given, q_select))


def conditions(m64, m32, n):
    """None, or what a case's tolerances do not rest on: a row whose two critics lie within Q_MARGIN max(1, |q|) of each other in
    float64, a row on which the float32 model selects another critic, a critic selected (a clamp branch taken) on less than a tenth of
    the rows (components) where n >= 200, or a tensor whose tolerance passes 1 % of its largest float64 entry"""
    r = m64["rows"]
    if r["q2"] is not None:
        gap = np.abs(r["q1"] - r["q2"])
        if (gap <= Q_MARGIN * np.maximum(1.0, np.maximum(np.abs(r["q1"]), np.abs(r["q2"])))).any():
            return "a row's critics within the margin"
        if not np.array_equal(m32["sel2"], m64["sel2"]):
            return "the float32 model selects another critic"
        if n >= 200 and not BRANCH_SHARE <= m64["sel2"].mean() <= 1 - BRANCH_SHARE:
            return "a critic selected on %.3f of the rows" % m64["sel2"].mean()
    if m64["inside"] is not None:
        if not np.array_equal(m32["inside"], m64["inside"]):
            return "the float32 model clamps other components"
        if n >= 200 and not BRANCH_SHARE <= m64["inside"].mean() <= 1 - BRANCH_SHARE:
            return "the clamp inside on %.3f of the components" % m64["inside"].mean()
    g64, g32 = flat(m64), flat(m32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        if k == "log_std" and not np.abs(g64[k]).max() > 0:
            continue  # (no eps: the log_std gradient is 0 and written as 0)
        if not tol[k] <= 0.01 * float(np.abs(g64[k]).max()):
            return "the tolerance of %s is %.3g of its largest entry" % (k, tol[k] / float(np.abs(g64[k]).max()))
    if not row_tolerance(m32["stats"], m64["stats"]) <= 0.01 * float(np.abs(m64["stats"]).max()):
        return "the tolerance of the statistics is %.3g of their largest" % (row_tolerance(m32["stats"], m64["stats"]) / float(np.abs(m64["stats"]).max()))
    for k, x64 in r.items():
        top = 0.0 if x64 is None else float(np.abs(x64).max())
        if k == "g_action":
            continue  # (1 / n times dq_sel, whose own cap is held: at these n the rule's floor of 1e-6 alone passes 1 % of |dq| / n)
        if top > 0 and not row_tolerance(m32["rows"][k], x64) <= 0.01 * top:  # (the Gaussian form's logp is 0 everywhere)
            return "the tolerance of the row array %s is %.3g of its largest entry" % (k, row_tolerance(m32["rows"][k], x64) / top)
    return None


def row_tolerance(x32, x64):
    """the project's rule for one array: 8 x max|x32seq - x64| + 1e-6 (1 + max|x64|)"""
    x64 = np.asarray(x64, np.float64)
    return 8.0 * float(np.abs(np.asarray(x32, np.float64) - x64).max()) + 1e-6 * (1.0 + float(np.abs(x64).max()))


# case(..., seed=CASE_SEED + n + the two widths): chosen on the CPU, by a search over 0, 1, 2, ... on this model alone (find_seed), as the
# first seed at which every case of grad_cases() keeps conditions()
CASE_SEED = 0


def grad_case(obs_dim, n, actor_net, q_net, n_critics, form, activation, eps_given, seed=None):
    return case(obs_dim, n, actor_net, q_net, n_critics, form, activation, eps_given,
                seed=(CASE_SEED if seed is None else seed) + n + actor_net[0] + q_net[0])


def find_seed(limit=200):
    """the first seed under which every case keeps its conditions, and what the earlier ones failed (the cases in order of cost)"""
    failed = []
    for seed in range(limit):
        for gc in sorted(grad_cases(), key=lambda gc: gc[1]):
            obs_dim, n, a, q, n_critics, form, activation, eps_given, q_select = gc
            c = grad_case(obs_dim, n, a, q, n_critics, form, activation, eps_given, seed=seed)
            why = conditions(*(reference(c, activation, eps_given, q_select, dt) for dt in (np.float64, np.float32)), n)
            if why:
                failed.append((seed, gc[:4], why))
                break
        else:
            return seed, failed
    raise AssertionError(failed)


_regime = {}


def regime_case():
    """(case, activation, eps given, q_select) of the one trained-regime case: tests/net_regimes.py's squashed family at (64, 2, relu) --
    its scaled actor under the engine's default clamp, its rows and noise -- with that table's q family's critics (Q values in the
    hundreds) at the same id.  Made once"""
    if not _regime:
        import net_regimes
        hidden, n_hidden, activation = net_regimes.NETS[1]
        env_id = net_regimes.ids_of(hidden, n_hidden)[0]
        s, q = (net_regimes.case(f, env_id, hidden, n_hidden, activation) for f in ("squashed", "q"))
        c = dict(actor=s["actor"], critics=q["critics"], obs=s["obs"], eps=s["eps"], form="squashed", env_id=env_id,
                 bounds=net_regimes.SQUASHED_BOUNDS)
        _regime["case"] = (c, activation, True, None)
    return _regime["case"]


def regime_reference(dtype):
    """the model of regime_case() in float64 or float32, computed once per process and left unchanged"""
    key = np.dtype(dtype).name
    if key not in _regime:
        c, activation, eps_given, q_select = regime_case()
        _regime[key] = actor_grad(c["actor"], c["critics"], c["obs"], bounds=c["bounds"], dtype=dtype, **options(c, activation, eps_given, q_select))
    return _regime[key]


# The width classes (tests/net_widths.py): the family's entry in test_gpu_net_widths.FAMILY_KERNELS, which tests/test_net_widths.py holds
# against the compiled engine's kernel templates, and the nets tests/test_gpu_q_actor.py runs for it: net_widths' table and the widest
# net of class 4, each on net_widths.ids_of's continuous id
WIDTH_FAMILY = ("q_actor", ("q_actor_squashed_grad_kernel", "q_actor_gaussian_grad_kernel"))


def register_width_family():
    """names the two kernel templates of sg_q_actor.inc in FAMILY_KERNELS.  Both new test modules call it when they are imported, which
    pytest does for every module it collects before it runs a test; tests/test_gpu_q_actor.py's width test is the family's test"""
    import test_gpu_net_widths
    test_gpu_net_widths.FAMILY_KERNELS.setdefault(*WIDTH_FAMILY)


def width_cases():
    """[(hidden, n_hidden, activation)]: net_widths.cases() and (128, 3)"""
    import net_widths
    return net_widths.cases() + [(128, 3, "relu")]
