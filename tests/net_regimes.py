"""The trained-regime inputs of the small-MLP kernels, for tests/test_gpu_net_regimes.py (GPU) and tests/test_net_regimes.py (CPU).

Every older GPU test of the net kernels draws from one regime: a freshly initialised net (weights and biases uniform in +-1 / sqrt(fan_in))
on N(0, 1) observations, log_std in [-1, 0], the squashed actor's clamp at (-0.5, 0.5).  There no hidden pre-activation passes |x| = 2.5,
no two logits of a row are 2.5 apart and every Q value is O(1).  The cases here start from the same constructors and seeds and then scale
layers by the named gains below, weights and biases alike, so that tanh units saturate (the float32 tanh rounds to 1 from |x| = 9.02 on),
logits lie tens to hundreds apart (exp(logit - max) underflows below -104), log_std spans (-4, 1.5), the squashed actor runs at its
default clamp (-20, 2) with actions that round to +-1, and Q values reach the hundreds.

The gains were chosen on the CPU so that every condition of tests/test_net_regimes.py holds: each gradient tensor's tolerance within the
1 % cap, every stratum occupied, and a second float32 implementation (the models summed in the kernels' forward order: kernel_order)
inside the tolerances the first one gives.  Each case names its strata as boolean row masks computed from the float64 model; the GPU
file applies the forward tolerance per stratum, so that one loose stratum does not set the tolerance of every other row."""
import numpy as np

import dqn_model
import net_widths
import squashed_model
from net_widths import OBS_DIM
from policy_grad_model import _forward

N = 200  # rows: ragged at every row tile (net_widths.N)

# The gains, chosen on the CPU (tests/test_net_regimes.py asserts what they were chosen for; profiles/net_regime_tests.txt has the scan).
# 5 on the hidden layers puts a first-layer tanh unit past 9.02 in 15 .. 35 % of a case's rows, leaves about half of them plain and 18 %
# of the first-layer units past 4; at 4 eight of the ten tanh cases have fewer than the 10 saturated rows a stratum needs (0 .. 14) and
# 10 % of the units are past 4, at 6 two thirds of the rows are saturated.
HIDDEN_GAIN = 5.0  # every hidden layer of every family
# Scaling weights and biases alike leaves the sign of every relu pre-activation where it was: half the units dead in every row, the
# fresh-init share.  A trained relu layer is sparser, so under relu the first layer's bias is also lowered, by this much in the units
# of the unscaled layer (its pre-activations have a standard deviation of about 0.6): about 65 % of the units are dead, and a tenth of
# the rows have three quarters dead.
RELU_BIAS_SHIFT = 0.22
POLICY_HEAD_GAIN = 40.0  # the critic's head of the policy family: values of tens to hundreds
# The Gaussian actors' head (the continuous policy, the q family's actor chain): means of O(1), as the ids' actions live in [-1, 1].
# d logp / d mean = (a - mean) / sigma^2 multiplies the rounding of the mean by e^8 = 2981 at log_std -4; with a head gain of 40 the
# means reach 200, their float32 rounding 1e-5, and the summed gradient of the head's bias carries an error of 0.1 .. 0.4 whatever the
# order of the float32 sums: fma_forward below missed the tolerance the float32 model gives by 3.4 x at (96, 3) tanh.
MEAN_HEAD_GAIN = 2.0
# The discrete actor's head: top-two gaps up to 73 (tanh) and 175 (relu), exp(logit - max) underflows in a tenth of a tanh case's rows
# and in most of a relu case's.  (At 80 the (64, 2) relu case keeps 2 plain rows, at 50 a tanh case 3 underflow rows.)
DISCRETE_HEAD_GAIN = 60.0
LOG_STD = (-4.0, 1.5)  # the two components' log_std of the continuous policy and of the actor chain
FAR_SIGMAS = 6.0  # the far stratum: every tenth row's action lies this many sigma farther from the mean
Q_HEAD_GAIN = 150.0  # the critics' heads: Q values in the hundreds
DQN_HEAD_GAIN = 150.0
# head rows 0, 1 (mean) and 2, 3 (raw log_std, which random_squashed has scaled by 3 already); the raw rows' bias moves to the clamp's
# middle.  (With 8 and 10 on top of the hidden gain fewer than 5 % of a relu case's rows stay plain; with 4 and 6 the engine's action
# came to 0.96 of its tolerance in the plain rows of (96, 3) tanh, and fma_forward to 0.71.)
SQUASHED_MEAN_GAIN, SQUASHED_RAW_GAIN, SQUASHED_RAW_BIAS = 4.0, 5.0, -9.0
SQUASHED_BOUNDS = (-20.0, 2.0)  # the engine's default clamp

TANH_ROUNDS_TO_ONE = 9.02  # float32 tanh(x) = 1 from here on
TANH_DEEP = 4.0  # tanh' < 1.4e-3
RELU_DEAD_SHARE = 0.75
PEAKED_GAP = 20.0
UNDERFLOW = -104.0  # float32 exp(x) = 0 below (denormals included)
STRATUM_ROWS = 4  # a stratum with fewer rows is not held to a tolerance of its own: its rows are in `all`

KEPLER = ("KeplerCircleOrbit-v0", "KeplerDiscrete-v0")
NETS = [(64, 2, "tanh"), (64, 2, "relu"), (96, 3, "tanh"), (33, 1, "relu")]  # (hidden, n_hidden, activation)


def ids_of(hidden, n_hidden):
    """(continuous id, discrete id): (64, 2) on the 3P ids, (96, 3) on the 4P ids as net_widths.ids_of, one hidden layer on the Kepler ids"""
    return KEPLER if n_hidden == 1 else net_widths.ids_of(hidden, n_hidden)


def cases():
    return list(NETS)


def scaled(layers, hidden_gain, head_gain, activation):
    """a net with every hidden layer's weight and bias times hidden_gain and the head's times head_gain (float32); under relu the first
    layer's bias is lowered by RELU_BIAS_SHIFT before it is scaled"""
    L = len(layers) - 1
    out = [(W * np.float32(head_gain if l == L else hidden_gain), b * np.float32(head_gain if l == L else hidden_gain)) for l, (W, b) in enumerate(layers)]
    if activation == "relu":
        out[0] = (out[0][0], out[0][1] - np.float32(RELU_BIAS_SHIFT * hidden_gain))
    return out


def saturated(layers, x, activation):
    """rows in which some first-layer tanh unit has |pre| > 9.02, or at least 75 % of the first layer's relu units are dead (float64)"""
    pre = _forward(layers, x, activation, np.float64)[1][0]
    if activation == "tanh":
        return (np.abs(pre) > TANH_ROUNDS_TO_ONE).any(axis=1)
    return (pre <= 0).mean(axis=1) >= RELU_DEAD_SHARE


def deep_share(layers, x):
    """the share of first-layer units over the batch with |pre| > 4"""
    return float((np.abs(_forward(layers, x, "tanh", np.float64)[1][0]) > TANH_DEEP).mean())


def with_plain(strata):
    """adds `plain`: the rows in none of the named strata"""
    out = dict(strata)
    out["plain"] = ~np.logical_or.reduce(list(strata.values()))
    return out


def occupancy(strata):
    return {k: int(v.sum()) for k, v in strata.items()}


# ---- the cases: each the older constructor's draws under its seed convention (n + hidden), then scaled
def policy_case(env_id, n, hidden, n_hidden, activation):
    """net_widths.policy_case scaled; log_std (-4, 1.5); continuous: action = float32(mean64 + sigma z), z N(0, 1), every tenth row
    (`far`) another FAR_SIGMAS out; discrete: uniform actions, so unlikely ones are scored"""
    c = net_widths.policy_case(env_id, n, hidden, n_hidden)
    pol, obs = c["policy"], c["obs"]
    continuous = pol["log_std"] is not None
    pol = dict(actor=scaled(pol["actor"], HIDDEN_GAIN, MEAN_HEAD_GAIN if continuous else DISCRETE_HEAD_GAIN, activation),
               critic=scaled(pol["critic"], HIDDEN_GAIN, POLICY_HEAD_GAIN, activation),
               log_std=np.asarray(LOG_STD, np.float32) if continuous else None)
    rng = np.random.default_rng([n + hidden, 1])
    head = _forward(pol["actor"], obs, activation, np.float64)[2]
    strata = dict(saturated=saturated(pol["actor"], obs, activation) | saturated(pol["critic"], obs, activation))
    if continuous:
        z = rng.standard_normal((n, 2))
        far = np.arange(n) % 10 == 3
        z[far] += FAR_SIGMAS * np.where(z[far] < 0, -1.0, 1.0)
        action = (head + np.exp(np.asarray(LOG_STD, np.float64)) * z).astype(np.float32)
        strata["far"] = far
    else:
        action = rng.integers(0, 6, n).astype(np.int32)
        top = np.sort(head, axis=1)
        strata["peaked"] = top[:, -1] - top[:, -2] >= PEAKED_GAP
        strata["underflow"] = (head - head.max(axis=1, keepdims=True) < UNDERFLOW).any(axis=1)
    return dict(policy=pol, obs=obs, action=action, g=c["g"], strata=with_plain(strata))


def q_case(env_id, n, hidden, n_hidden, activation):
    """net_widths.q_case scaled: two critics whose outputs reach the hundreds; the actor of the chain with log_std (-4, 1.5).  strata:
    the critics' rows; actor_strata: the actor's"""
    c = net_widths.q_case(env_id, n, hidden, n_hidden)
    critics = [scaled(net, HIDDEN_GAIN, Q_HEAD_GAIN, activation) for net in c["critics"]]
    pol = dict(actor=scaled(c["policy"]["actor"], HIDDEN_GAIN, MEAN_HEAD_GAIN, activation), critic=None, log_std=np.asarray(LOG_STD, np.float32))
    x = np.concatenate([c["obs"], c["action"]], axis=1)
    strata = dict(saturated=saturated(critics[0], x, activation) | saturated(critics[1], x, activation))
    return dict(c, critics=critics, policy=pol, strata=with_plain(strata),
                actor_strata=with_plain(dict(saturated=saturated(pol["actor"], c["obs"], activation))))


def _squashed_prepare(actor, activation):
    layers = scaled(actor, HIDDEN_GAIN, 1.0, activation)
    W, b = (a.copy() for a in layers[-1])
    W[:2] *= np.float32(SQUASHED_MEAN_GAIN)
    b[:2] *= np.float32(SQUASHED_MEAN_GAIN)
    W[2:] *= np.float32(SQUASHED_RAW_GAIN)
    b[2:] = b[2:] * np.float32(SQUASHED_RAW_GAIN) + np.float32(SQUASHED_RAW_BIAS)
    layers[-1] = (W, b)
    return layers


def squashed_case(env_id, n, hidden, n_hidden, activation):
    """squashed_model.case's draws with the actor scaled and the default clamp; its redraw rule (MARGIN) against these bounds; no row
    dropped.  unit_action is read off the float32 model's action with the case's eps"""
    c = squashed_model.case_of(OBS_DIM[env_id], n, hidden, n_hidden, seed=n + hidden, bounds=SQUASHED_BOUNDS,
                                prepare=lambda actor: _squashed_prepare(actor, activation))
    m64 = squashed_model.sample(c["actor"], c["obs"], c["eps"], bounds=SQUASHED_BOUNDS, activation=activation)
    m32 = squashed_model.sample(c["actor"], c["obs"], c["eps"], bounds=SQUASHED_BOUNDS, activation=activation, dtype=np.float32)
    lo, hi = SQUASHED_BOUNDS
    strata = dict(saturated=saturated(c["actor"], c["obs"], activation), below=(m64["raw"] < lo).any(axis=1), above=(m64["raw"] > hi).any(axis=1),
                  unit_action=(np.abs(m32["action"]) == 1).any(axis=1))
    return dict(c, strata=with_plain(strata))


def dqn_case(env_id, n, hidden, n_hidden, activation):
    """dqn_model.case scaled: Q values in the hundreds"""
    c = dqn_model.case(OBS_DIM[env_id], n, hidden, n_hidden, seed=n + hidden)
    net = scaled(c["net"], HIDDEN_GAIN, DQN_HEAD_GAIN, activation)
    return dict(c, net=net, strata=with_plain(dict(saturated=saturated(net, c["obs"], activation))))


CONSTRUCTORS = dict(policy=policy_case, q=q_case, squashed=squashed_case, dqn=dqn_case)
_made = {}


def case(family, env_id, hidden, n_hidden, activation):
    """the case at n = N rows, made once per process and left unchanged"""
    key = (family, env_id, hidden, n_hidden, activation)
    if key not in _made:
        _made[key] = CONSTRUCTORS[family](env_id, N, hidden, n_hidden, activation)
    return _made[key]


def forward_models(family, c, activation, dtype):
    """{name: [n, ...] array}: every forward quantity of the family's model on the case's own inputs"""
    import policy_grad_model
    import q_model
    if family == "policy":
        e = policy_grad_model.evaluate(c["policy"], c["obs"], c["action"], activation=activation, grads=False, dtype=dtype)
        head = _forward(c["policy"]["actor"], c["obs"], activation, np.dtype(dtype).type)[2]
        return dict(logp=e["logp"], entropy=e["entropy"], value=e["value"], head=head)
    if family == "q":
        q = q_model.q_evaluate(c["critics"], c["obs"], c["action"], activation=activation, grads=False, dtype=dtype)["q"]
        return dict(q1=q[0], q2=q[1], action=q_model.action(c["policy"], c["obs"], c["eps"], activation=activation, dtype=dtype)["action"])
    if family == "squashed":
        m = squashed_model.sample(c["actor"], c["obs"], c["eps"], bounds=SQUASHED_BOUNDS, activation=activation, dtype=dtype)
        return dict(action=m["action"], logp=m["logp"])
    m = dqn_model.evaluate(c["net"], c["obs"], c["action"], activation=activation, dtype=dtype)
    return dict(q_all=m["q_all"], q_taken=m["q_taken"], q_max=m["q_max"])


# ---- a second float32 implementation: the models with every layer accumulated in the kernels' forward order
def fma_forward(layers, x, activation, dtype):
    """policy_grad_model._forward in float32 with each output accumulated as policy_layer (sg_policy.inc) does: acc = b[j], then
    acc = fma(W[j][k], h[k], acc) for k ascending (the product of two float32 is exact in float64; one rounding per step)"""
    hs, pre = [np.asarray(x, np.float32)], []
    for l, (W, b) in enumerate(layers):
        W64, h64 = np.asarray(W, np.float64), hs[-1].astype(np.float64)
        acc = np.broadcast_to(np.asarray(b, np.float32), (h64.shape[0], W64.shape[0])).copy()
        for k in range(W64.shape[1]):
            acc = (W64[None, :, k] * h64[:, k, None] + acc).astype(np.float32)
        if l == len(layers) - 1:
            return hs, pre, acc
        pre.append(acc)
        hs.append(np.tanh(acc) if activation == "tanh" else np.maximum(acc, np.float32(0)))


class kernel_order:
    """with kernel_order(): the models' float32 forward passes run fma_forward.  Two correct float32 implementations then differ as
    the engine and the float32 model do, by their summation order; tests/test_net_regimes.py holds the second one to the tolerances
    the first one gives, which the gains must leave room for"""

    def __enter__(self):
        import policy_grad_model
        import policy_model
        import q_model
        plain, plain_mlp = policy_grad_model._forward, policy_model.mlp
        forward = lambda layers, x, activation, dtype: (fma_forward if np.dtype(dtype) == np.float32 else plain)(layers, x, activation, dtype)
        mlp = lambda layers, x, activation, dtype=np.float64: (fma_forward(layers, x, activation, dtype)[2] if np.dtype(dtype) == np.float32
                                                               else plain_mlp(layers, x, activation, dtype))
        self.saved = [(m, "_forward", m._forward) for m in (policy_grad_model, q_model, squashed_model, dqn_model, _this())] + [(policy_model, "mlp", plain_mlp)]
        for m, name, _ in self.saved:
            setattr(m, name, mlp if name == "mlp" else forward)
        return self

    def __exit__(self, *exc):
        for m, name, f in self.saved:
            setattr(m, name, f)


def _this():
    import sys
    return sys.modules[__name__]


def act_models(family, c, activation, dtype, noise):
    """{name: array} of the act paths' forward quantities under the engine's own noise (policy: the discrete logp is scored at the
    float64 model's drawn action)"""
    import policy_model
    if family == "policy":
        m = policy_model.act(c["policy"], c["obs"], activation=activation, dtype=dtype, **noise)
        if c["policy"]["log_std"] is not None:
            return dict(mean=m["mean"], act_logp=m["logp"])
        a = policy_model.act(c["policy"], c["obs"], activation=activation, **noise)["action"]
        return dict(act_logp=policy_model.act(c["policy"], c["obs"], activation=activation, dtype=dtype, action=a)["logp"])
    if family == "squashed":
        out = {}
        for det in (False, True):
            m = squashed_model.act(c["actor"], c["obs"], deterministic=det, bounds=SQUASHED_BOUNDS, activation=activation, dtype=dtype, **noise)
            out.update({"act_action_%d" % det: m["action"], "act_logp_%d" % det: m["logp"]})
        return out
    return {}


def kernel_order_ratios(family, c, activation, references, noise):
    """[(error / tolerance, name)]: the float32 model in the kernels' forward order held to the tolerances the GPU file derives from the
    float32 model as it is -- forward quantities per stratum (8 x max|m32 - m64| + 1e-6 over the stratum's rows), gradient tensors per
    tensor (grad_tolerances)"""
    from policy_grad_model import grad_tolerances
    both = lambda f: (f(np.float64), f(np.float32))
    out = []
    for models in (lambda d: forward_models(family, c, activation, d), lambda d: act_models(family, c, activation, d, noise)):
        m64, m32 = both(models)
        with kernel_order():
            other = models(np.float32)
        for k in m64:
            strata = c["actor_strata"] if (family, k) == ("q", "action") else c["strata"]
            for s, rows in [("all", np.ones(N, bool))] + [(s, v) for s, v in strata.items() if v.sum() >= STRATUM_ROWS]:
                tol = 8.0 * float(np.abs(m32[k][rows].astype(np.float64) - m64[k][rows]).max()) + 1e-6
                out.append((float(np.abs(other[k][rows].astype(np.float64) - m64[k][rows]).max()) / tol, "%s [%s]" % (k, s)))
    for name, reference in references:
        g64, g32 = both(lambda d: reference(c, activation, d))
        with kernel_order():
            other = reference(c, activation, np.float32)
        tol = grad_tolerances(g32, g64)
        out += [(float(np.abs(other[k].astype(np.float64) - g64[k]).max()) / tol[k], "%s %s" % (name, k)) for k in g64 if np.abs(g64[k]).max() > 0]
    return out


# ---- the float64 / float32-sequential gradient references, as flat {name: array} dicts (net_widths' forms)
policy_reference, q_reference, actor_chain_reference, dqn_reference = (net_widths.policy_reference, net_widths.q_reference,
                                                                       net_widths.actor_chain_reference, net_widths.dqn_reference)


def policy_reference_of(c, activation, dtype, which):
    """one g alone: which in ("logp", "entropy", "value")"""
    import policy_grad_model
    g = {k: (c["g"][k] if k == which else None) for k in ("logp", "entropy", "value")}
    return policy_grad_model.flat(policy_grad_model.evaluate(c["policy"], c["obs"], c["action"], g["logp"], g["entropy"], g["value"],
                                                             activation=activation, dtype=dtype))


def squashed_reference(c, activation, dtype, selection="both"):
    return squashed_model.grad_reference(c, activation, selection, dtype, bounds=SQUASHED_BOUNDS)


def dqn_reference_of(c, activation, dtype, selection):
    return dqn_model.grad_reference(c, activation, selection, dtype)


def gradient_cases():
    """[(family, env_id, hidden, n_hidden, activation, case constructor, [(name, reference(c, activation, dtype)), ...])]: every gradient
    case tests/test_gpu_net_regimes.py holds to a tolerance"""
    out = []
    for hidden, n_hidden, activation in cases():
        cont, disc = ids_of(hidden, n_hidden)
        each = [(k, lambda c, a, d, k=k: policy_reference_of(c, a, d, k)) for k in ("logp", "entropy", "value")]
        out.append(("policy", cont, hidden, n_hidden, activation, policy_case, [("all", policy_reference)] + each))
        out.append(("policy", disc, hidden, n_hidden, activation, policy_case, [("all", policy_reference)] + each))
        out.append(("q", cont, hidden, n_hidden, activation, q_case, [("q_grad", q_reference), ("action_grad", actor_chain_reference)]))
        out.append(("squashed", cont, hidden, n_hidden, activation, squashed_case,
                    [(s, lambda c, a, d, s=s: squashed_reference(c, a, d, s)) for s in squashed_model.SELECTIONS]))
        out.append(("dqn", disc, hidden, n_hidden, activation, dqn_case,
                    [(s, lambda c, a, d, s=s: dqn_reference_of(c, a, d, s)) for s in dqn_model.SELECTIONS]))
    return out
