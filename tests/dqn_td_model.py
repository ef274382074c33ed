"""The contract of sg_dqn_td_grad_device (include/spacegym.h) in NumPy: the DQN / Double DQN TD update on a replay
batch -- target, Huber loss, statistics, the loss gradient by q_taken and, through tests/dqn_model.py, the gradient of every parameter
of the online net.  For row i:
    a*      = first argmax of Q_online(next_obs[i])                          (double_q)
    q_next  = Q_target(next_obs[i])[a*]                                      (else max_j Q_target(next_obs[i])[j])
    y       = terminated[i] ? reward[i] : reward[i] + discount[i] * q_next   (a where: a terminated row never multiplies its q_next)
    q_taken = Q_online(obs[i])[action[i]];  td = q_taken - y
    c       = clip(td, -delta, +delta);  w = weight[i] (1 without weights);  g = (w * c) / n
    loss    = (1 / n) sum_i w * (|td| <= delta ? 0.5 td^2 : delta (|td| - 0.5 delta))
An action outside 0 .. 5 selects Q_0 for q_taken and otherwise contributes nothing: g = 0, td_error = 0, no term in any statistic, one
more in bad_rows; the means still divide by n.

float64 by default.  With dtype=np.float32 it is the yardstick the GPU tests derive their tolerances from: every per-row term is formed
in float32 and every sum over the rows is plain sequential float32 accumulation, as dqn_model's.  a_star: the argmax to use in place
of the model's own (the device's: a near-tie of two Q values may round either way in float32).

The module also holds the cases tests/test_dqn_td.py (CPU) and tests/test_gpu_dqn_td.py share."""
import numpy as np

from dqn_model import ACTIONS, BIG_N, GRAD_NS, NETS, _sum_rows, evaluate, random_dqn

STATS = ("loss", "td_abs_mean", "td_abs_max", "q_mean", "target_mean", "clip_fraction", "weight_mean", "bad_rows")
ROWS = ("td_error", "q_taken", "target", "q_next", "g")


def td(online, target, batch, double_q=True, huber_delta=1.0, weight=None, activation="relu", dtype=np.float64, a_star=None):
    """online, target: [(W, b), ...] with a head of 6.  batch: dict obs [n, D] / action int [n] / reward / next_obs / terminated /
    discount of NumPy arrays.  Returns dict actor: [(dW, db), ...] (dqn_model.flat takes it), stats [8] named by STATS, rows (dict of
    [n] arrays named by ROWS), a_star int32 [n] (None for plain DQN), gap [n] (the two largest online Q values of next_obs apart;
    None for plain DQN), good bool [n] (the action is in 0 .. 5) and clipped bool [n]."""
    dtype = np.dtype(dtype).type
    obs = np.asarray(batch["obs"])
    n = obs.shape[0]
    col = lambda k: np.asarray(batch[k]).astype(dtype)
    rows = np.arange(n)
    nxt = evaluate(target, batch["next_obs"], activation=activation, dtype=dtype)
    a2 = gap = None
    if double_q:
        on = evaluate(online, batch["next_obs"], activation=activation, dtype=dtype)
        top = np.sort(on["q_all"], axis=1)
        gap = top[:, -1] - top[:, -2]
        a2 = on["argmax"] if a_star is None else np.asarray(a_star, np.int32)
        q_next = nxt["q_all"][rows, a2]
    else:
        q_next = nxt["q_max"]
    r, d = col("reward"), col("discount")
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(np.asarray(batch["terminated"]) != 0, r, r + d * q_next).astype(dtype)
    a = np.asarray(batch["action"], np.int64)
    good = (a >= 0) & (a < ACTIONS)
    a_sel = np.where(good, a, 0)
    q_taken = evaluate(online, obs, a_sel, activation=activation, dtype=dtype)["q_taken"]
    delta, nf, zero, half = dtype(huber_delta), dtype(n), dtype(0), dtype(0.5)
    w = np.ones(n, dtype) if weight is None else np.asarray(weight).astype(dtype)
    err = q_taken - y
    ad = np.abs(err)
    g = np.where(good, (w * np.clip(err, -delta, delta)) / nf, zero).astype(dtype)
    with np.errstate(invalid="ignore"):
        huber = np.where(ad <= delta, half * (err * err), delta * (ad - half * delta)).astype(dtype)
    clipped = ad > delta
    grads = evaluate(online, obs, a_sel, g, None, activation=activation, dtype=dtype)["actor"]
    mean_of = lambda v: _sum_rows(np.where(good, v, zero).astype(dtype), dtype) / nf
    s = np.zeros(len(STATS), dtype)
    s[0], s[1], s[2] = mean_of(w * huber), mean_of(ad), np.where(good, ad, zero).max()
    s[3], s[4], s[5], s[6], s[7] = mean_of(q_taken), mean_of(y), mean_of(clipped.astype(dtype)), mean_of(w), dtype((~good).sum())
    return dict(actor=grads, stats=s, a_star=a2, gap=gap, good=good, clipped=clipped & good,
                rows=dict(td_error=np.where(good, err, zero).astype(dtype), q_taken=q_taken, target=y, q_next=q_next, g=g))


def case(obs_dim, n, hidden, n_hidden, seed):
    """The shared inputs of a (net, n) case, CPU and GPU tests alike: online and target nets, a batch with the sampler's columns and
    dtypes (a tenth of the rows terminated, discounts gamma^steps of a 3-step sampler) and importance weights in (0.2, 1]"""
    rng = np.random.default_rng([seed, obs_dim, n, hidden, n_hidden, 31])
    online, target = random_dqn(rng, obs_dim, hidden, n_hidden), random_dqn(rng, obs_dim, hidden, n_hidden)
    batch = dict(obs=rng.standard_normal((n, obs_dim)).astype(np.float32), action=rng.integers(0, ACTIONS, n).astype(np.int32),
                 reward=(1.5 * rng.standard_normal(n)).astype(np.float32), next_obs=rng.standard_normal((n, obs_dim)).astype(np.float32),
                 terminated=(rng.uniform(size=n) < 0.1).astype(np.uint8),
                 discount=(np.float32(0.99) ** rng.integers(1, 4, n)).astype(np.float32))
    weight = rng.uniform(0.2, 1.0, n).astype(np.float32)
    return dict(online=online, target=target, batch=batch, weight=weight)


CLASS3_NET = (80, 2)  # tests/net_widths.py's class of hidden 65 .. 96: NT = 3
CASE_SEED = 5  # case(..., seed=CASE_SEED + n + hidden): chosen on the CPU so that every case keeps tests/test_dqn_td.py's conditions
HUBER_MARGIN, GAP, GAP_SHARE = 1e-4, 1e-5, 0.01


def grad_cases():
    """(obs_dim, n, hidden, n_hidden, activation, double_q, huber_delta, weighted): dqn_model.GRAD_NS over dqn_model.NETS, the second row
    tile past the grid cap at hidden 128, and one net of width class 3; the options rotate over the cases so that Double and plain,
    Huber and the squared loss, weights and none each meet every row count.  obs_dim 15: GoalDiscrete3-v0, 10: KeplerDiscrete-v0."""
    shapes = [(15 if i % 2 == 0 else 10, n, hidden, n_hidden) for n in GRAD_NS for i, (hidden, n_hidden) in enumerate(NETS)]
    shapes += [(15, BIG_N, 128, 1), (10, 200) + CLASS3_NET]
    cases = []
    for v, shape in enumerate(shapes):
        cases.append(shape + (("tanh", "relu")[(v // 2) % 2], v % 2 == 0, float("inf") if v % 3 == 2 else 1.0, v % 4 < 2))
    return cases


# The width classes (tests/net_widths.py): the family's entry in test_gpu_net_widths.FAMILY_KERNELS, which tests/test_net_widths.py holds
# against the compiled engine's kernel templates, and the nets tests/test_gpu_dqn_td.py runs for it: net_widths' table and the widest
# net of class 4, each on net_widths.ids_of's discrete id (three hidden layers: the 4P id, the largest LDS footprint of its class)
WIDTH_FAMILY = ("dqn_td", ("dqn_td_target_kernel", "dqn_td_grad_kernel"))


def register_width_family():
    """names the two kernel templates of sg_dqn_td.inc in FAMILY_KERNELS.  Both new test modules call it when they are imported, which
    pytest does for every module it collects before it runs a test; tests/test_gpu_dqn_td.py's width test is the family's test"""
    import test_gpu_net_widths
    test_gpu_net_widths.FAMILY_KERNELS.setdefault(*WIDTH_FAMILY)


def width_cases():
    """[(hidden, n_hidden, activation)]: net_widths.cases() and (128, 3)"""
    import net_widths
    return net_widths.cases() + [(128, 3, "relu")]


def grad_case(obs_dim, n, hidden, n_hidden):
    return case(obs_dim, n, hidden, n_hidden, seed=CASE_SEED + n + hidden)


def reference(c, activation, double_q, huber_delta, weighted, dtype, a_star=None):
    return td(c["online"], c["target"], c["batch"], double_q=double_q, huber_delta=huber_delta, weight=c["weight"] if weighted else None,
              activation=activation, dtype=dtype, a_star=a_star)
