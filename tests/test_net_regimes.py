"""CPU tests of the trained-regime cases the net kernels are run on (tests/net_regimes.py, tests/test_gpu_net_regimes.py): the conditions
the GPU file's tolerances rest on, from the float64 and float32 models alone and on the very arrays the GPU file runs, so that a GPU
failure cannot be the inputs' fault.  Conditions, not measurements: the 1 % cap of every gradient tensor, the occupancy of every stratum,
the share of deeply saturated tanh units, finite float32 models, clear argmaxes, and the magnitudes the regime is named for."""
import numpy as np
import pytest

import net_regimes as R
from dqn_td_model import GAP, GAP_SHARE
from policy_grad_model import _forward, grad_tolerances
from test_gpu_policy import _tol

MIN_SHARE = 0.05  # of a case's rows, in every stratum its family names
RARE = ("underflow", "unit_action")  # at least RARE_ROWS rows in at least one case of the family
RARE_ROWS = 4
DEEP_SHARE = 0.10  # of the first-layer tanh units over the batch: |pre| > 4
CLEAR_SHARE = 0.90
ROOM = 0.75  # of a tolerance, for a second float32 implementation on the CPU
NOISE = dict(seed=77, step=2 ** 32 + 5, env_index_base=1000)  # tests/test_gpu_net_regimes.py's NOISE and BASE
CASES = R.gradient_cases()


def _id(case):
    family, env_id, hidden, n_hidden, activation = case[:5]
    return "%s-%s-%d-%d-%s" % (family, env_id, hidden, n_hidden, activation)


def _nets(family, c):
    """the nets of a case with their input rows"""
    if family == "policy":
        return [(c["policy"]["actor"], c["obs"]), (c["policy"]["critic"], c["obs"])]
    if family == "q":
        x = np.concatenate([c["obs"], c["action"]], axis=1)
        return [(c["critics"][0], x), (c["critics"][1], x), (c["policy"]["actor"], c["obs"])]
    return [(c["actor" if family == "squashed" else "net"], c["obs"])]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_gradient_tensor_keeps_the_one_percent_cap(case):
    """8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) <= 1 % of max|G64| per tensor, under every selection of the loss gradients the GPU file
    runs; a tensor that is identically zero in the float64 model (a g left out) is zero in the float32 one"""
    family, env_id, hidden, n_hidden, activation, _, references = case
    c = R.case(family, env_id, hidden, n_hidden, activation)
    worst = 0.0
    for name, reference in references:
        g64, g32 = reference(c, activation, np.float64), reference(c, activation, np.float32)
        tol = grad_tolerances(g32, g64)
        assert set(g32) == set(g64)
        live = 0
        for k in g64:
            top = float(np.abs(g64[k]).max())
            assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64 and np.isfinite(g32[k]).all(), (name, k)
            if top == 0.0:
                assert not g32[k].any(), (name, k)
                continue
            live += 1
            assert tol[k] <= 0.01 * top, (name, k, tol[k], top)
            worst = max(worst, tol[k] / (0.01 * top))
        assert live, name
    print("largest tolerance / cap: %.4f" % worst, _id(case))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_second_float32_implementation_keeps_every_tolerance(case):
    """The GPU file's tolerances are 8 x the error of ONE float32 implementation, the model as NumPy sums it.  Where a quantity's error
    comes from a few rows only (a small stratum; the log-prob of a drawn action under peaked logits, exact wherever the action is the
    argmax) or a tensor has two entries (log_std, the head's bias), that error is one draw of the rounding noise and may be small by
    chance.  So the same model with every layer summed in the kernels' forward order (net_regimes.fma_forward) is held to those
    tolerances here, per stratum and per tensor as on the GPU, and must stay below ROOM of each: the rest is left to what else differs on
    the device (its tanh and exp, the backward pass's order).  A case that misses is the inputs' fault: another gain, never a tolerance"""
    family, env_id, hidden, n_hidden, activation, _, references = case
    c = R.case(family, env_id, hidden, n_hidden, activation)
    ratios = sorted(R.kernel_order_ratios(family, c, activation, references, NOISE), reverse=True)
    print(_id(case), "kernel-order float32 model, error / tolerance, the three largest of %d:" % len(ratios),
          ", ".join("%.2f %s" % r for r in ratios[:3]))
    assert ratios and ratios[0][0] <= ROOM, ratios[:3]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_stratum_is_occupied_and_the_float32_model_is_finite(case):
    family, env_id, hidden, n_hidden, activation = case[:5]
    c = R.case(family, env_id, hidden, n_hidden, activation)
    every = [("", c["strata"])] + ([("actor ", c["actor_strata"])] if family == "q" else [])
    for prefix, strata in every:
        print(_id(case), prefix + "strata:", R.occupancy(strata))
        assert "plain" in strata and all(v.dtype == bool and v.shape == (R.N,) for v in strata.values())
        assert np.array_equal(strata["plain"], ~np.logical_or.reduce([v for k, v in strata.items() if k != "plain"]))
        for k, v in strata.items():
            assert k in RARE or v.sum() >= MIN_SHARE * R.N, (prefix, k, int(v.sum()))
    for net, x in _nets(family, c):
        if activation == "tanh":
            share = R.deep_share(net, x)
            print(_id(case), "first-layer tanh units with |pre| > 4: %.3f" % share)
            assert share >= DEEP_SHARE, share
        else:
            dead = (_forward(net, x, "relu", np.float64)[1][0] <= 0).mean()
            print(_id(case), "first-layer relu units dead: %.3f" % dead)
            assert dead > 0.55, dead
    m32, m64 = R.forward_models(family, c, activation, np.float32), R.forward_models(family, c, activation, np.float64)
    for k, v in m32.items():
        assert v.dtype == np.float32 and np.isfinite(v).all() and np.isfinite(m64[k]).all(), k


@pytest.mark.parametrize("family", ["policy", "squashed"])
def test_the_rare_strata_have_rows_in_some_case_of_the_family(family):
    seen = {}
    for case in CASES:
        if case[0] == family:
            for k, v in R.case(*case[:5])["strata"].items():
                if k in RARE:
                    seen[k] = max(seen.get(k, 0), int(v.sum()))
    print(family, seen)
    assert seen and all(rows >= RARE_ROWS for rows in seen.values()), seen
    assert set(seen) == ({"underflow"} if family == "policy" else {"unit_action"})


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("policy", "dqn") and "Discrete" in c[1]], ids=_id)
def test_the_argmax_is_clear_on_nine_rows_in_ten(case):
    """the older files' rule: the two largest logits (Q values) more than twice the forward tolerance apart; and tests/dqn_td_model.py's
    near-tie rule for the Q head: at most GAP_SHARE of the rows with a gap below GAP"""
    family, env_id, hidden, n_hidden, activation = case[:5]
    c = R.case(family, env_id, hidden, n_hidden, activation)
    k = "head" if family == "policy" else "q_all"
    m32, m64 = R.forward_models(family, c, activation, np.float32)[k], R.forward_models(family, c, activation, np.float64)[k]
    top = np.sort(m64, axis=1)
    gap = top[:, -1] - top[:, -2]
    clear = gap > 2 * _tol(m32, m64)
    print(_id(case), "clear rows: %.3f, largest gap %.1f, largest |.| %.0f" % (clear.mean(), gap.max(), np.abs(m64).max()))
    assert clear.mean() >= CLEAR_SHARE
    if family == "dqn":
        assert (gap < GAP).mean() <= GAP_SHARE and np.abs(m64).max() >= 100


def test_the_regime_is_the_one_the_module_names():
    """log_std (-4, 1.5) and the default clamp; logit gaps reach 80 and entropies 1e-20 in the policy family, exp(logit - max) underflows;
    both critics reach the hundreds; squashed raw values on both sides of the clamp, actions that round to +-1 with a finite log-prob;
    n = 200 is ragged at every row tile; the nets are the issue's"""
    assert R.LOG_STD == (-4.0, 1.5) and R.SQUASHED_BOUNDS == (-20.0, 2.0) and R.N == 200 and all(R.N % rows for rows in (64, 128, 256))
    assert R.cases() == [(64, 2, "tanh"), (64, 2, "relu"), (96, 3, "tanh"), (33, 1, "relu")]
    assert [R.ids_of(h, L) for h, L, _ in R.cases()] == [("GoalContinuous3P-v0", "GoalDiscrete3-v0")] * 2 + [
        ("GoalContinuous4P-v0", "GoalDiscrete4-v0"), ("KeplerCircleOrbit-v0", "KeplerDiscrete-v0")]
    gaps, entropies = [], []
    for case in CASES:
        family, env_id, hidden, n_hidden, activation = case[:5]
        c = R.case(family, env_id, hidden, n_hidden, activation)
        m64 = R.forward_models(family, c, activation, np.float64)
        if family == "policy" and "Discrete" in env_id:
            top = np.sort(m64["head"], axis=1)
            gaps.append(float((top[:, -1] - top[:, -2]).max()))
            entropies.append(float(m64["entropy"].min()))
            assert np.bincount(c["action"], minlength=6).min() >= 10 and m64["logp"].min() < -R.PEAKED_GAP  # uniform actions: unlikely ones are scored
        elif family == "policy":
            assert c["policy"]["log_std"].tolist() == [-4.0, 1.5] and c["strata"]["far"].sum() == R.N // 10
            z = (c["action"].astype(np.float64) - m64["head"]) / np.exp(np.asarray(R.LOG_STD))
            assert np.abs(z[c["strata"]["far"]]).min() >= R.FAR_SIGMAS - 1e-2 and np.abs(z[~c["strata"]["far"]]).max() < R.FAR_SIGMAS
        elif family == "q":
            assert min(np.abs(m64["q1"]).max(), np.abs(m64["q2"]).max()) >= 100 and c["policy"]["log_std"].tolist() == [-4.0, 1.5]
        elif family == "squashed":
            m32 = R.forward_models(family, c, activation, np.float32)
            unit = np.abs(m32["action"]) == 1
            assert unit.any() and np.isfinite(m32["logp"][unit.any(axis=1)]).all() and np.abs(m32["action"]).max() <= 1
            assert c["strata"]["below"].any() and c["strata"]["above"].any()
    print("largest logit gaps:", gaps, "smallest entropies:", entropies)
    assert max(gaps) >= 80 and min(entropies) <= 1e-20
