"""CPU tests of the width table the net kernels are run at (tests/net_widths.py, tests/test_gpu_net_widths.py): the 1 % cap of every
gradient case the GPU file holds to a tolerance, checked on the very inputs (the same constructors, the same seeds); the table's cover
of the four instantiation classes; and the family table against the kernels the compiled engine has."""
import collections
import os
import re

import numpy as np
import pytest

import engine_asm
from net_widths import BIG, GRAD_ROWS, N, OBS_DIM, WHY, WIDTH_NETS, cases, gradient_cases, ids_of, tile_class
from policy_grad_model import grad_tolerances

NETS = [(1, 1), (33, 2), (64, 2), (128, 3)]  # test_gpu_policy.NETS, which the older GPU files loop over


def _id(case):
    family, env_id, n, hidden, n_hidden, activation = case[:6]
    return "%s-%s-%d-%d-%d-%s" % (family, env_id, n, hidden, n_hidden, activation)


@pytest.mark.parametrize("case", gradient_cases(), ids=_id)
def test_every_gpu_gradient_case_has_a_tolerance_of_at_most_one_percent(case):
    """8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) <= 1 % of max|G64| per tensor, from the float32-sequential and float64 models alone:
    a GPU failure cannot be the inputs' fault"""
    family, env_id, n, hidden, n_hidden, activation, make_case, references = case
    c = make_case(env_id, n, hidden, n_hidden)
    worst = 0.0
    for reference in references:
        g64, g32 = reference(c, activation, np.float64), reference(c, activation, np.float32)
        tol = grad_tolerances(g32, g64)
        assert set(g32) == set(g64)
        for k in g64:
            top = float(np.abs(g64[k]).max())
            assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64, k
            assert top > 0 and tol[k] <= 0.01 * top, (reference.__name__, k, tol[k], top)
            worst = max(worst, tol[k] / (0.01 * top))
    print("largest tolerance / cap: %.4f" % worst, _id(case))


def test_the_table_is_the_issue_of_record():
    """seven nets, each with its reason; the ids follow the layers and the width; n = 200 is ragged at every row tile"""
    assert WIDTH_NETS == [(31, 2), (32, 3), (64, 3), (65, 1), (80, 2), (96, 3), (127, 2)] and set(WHY) == set(WIDTH_NETS) and all(WHY.values())
    assert [a for _, _, a in cases()] == ["tanh", "relu", "tanh", "relu", "tanh", "relu", "tanh"]
    for hidden, n_hidden in WIDTH_NETS:
        cont, disc = ids_of(hidden, n_hidden)
        width = 17 if n_hidden == 3 else 13 if hidden == 31 else 15
        assert OBS_DIM[cont] == OBS_DIM[disc] == width, (hidden, n_hidden)
    assert [tile_class(h) for h in (1, 32, 33, 64, 65, 96, 97, 128)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert GRAD_ROWS == {1: 256, 2: 128, 3: 64, 4: 64} and all(N % R for R in GRAD_ROWS.values()) and N % 128 and N % 256
    assert tile_class(BIG[0]) == 3 and BIG[3] == 256 * GRAD_ROWS[3] + 300


def test_the_ids_have_the_observation_widths_the_table_assumes():
    from conftest import load_golden
    for env_id, golden in (("GoalContinuous2P-v0", "step_goal2p"), ("GoalContinuous3P-v0", "step_goal3p"), ("GoalContinuous4P-v0", "step_goal4p"),
                           ("GoalDiscrete2-v0", "step_goal_discrete2"), ("GoalDiscrete3-v0", "step_goal_discrete3"),
                           ("GoalDiscrete4-v0", "step_goal_discrete4"), ("KeplerCircleOrbit-v0", "step_kepler_circle"),
                           ("KeplerDiscrete-v0", "step_kepler_discrete")):
        obs = [v for k, v in load_golden(golden).items() if k.startswith("obs")]
        assert obs and all(v.shape[-1] == OBS_DIM[env_id] for v in obs), (env_id, [v.shape for v in obs])


def test_the_widths_cover_every_class_and_each_class_filled_with_three_layers():
    """WIDTH_NETS together with NETS: every class NT = 1 .. 4, and 32 NT with three hidden layers, the net nets_begin sizes the
    instantiation's LDS limit for"""
    every = WIDTH_NETS + NETS
    assert {tile_class(hidden) for hidden, _ in every} == {1, 2, 3, 4}
    for c in (1, 2, 3, 4):
        assert (32 * c, 3) in every, c
    assert {31, 127} <= {hidden for hidden, _ in WIDTH_NETS}  # in + 1 a multiple of 32: the bias closes an MFMA column tile
    assert all(1 <= hidden <= 128 and 1 <= n_hidden <= 3 for hidden, n_hidden in every)


def test_every_net_kernel_template_has_four_instantiations_and_a_width_test():
    """The net kernels are the templates on the class alone: in the source, the kernels whose launch bounds are policy_block(NT) or
    policy_grad_block(NT); in the compiler's resource report, the names _Z<len><name>_kernelILi<c>EE with exactly the four
    instantiations c = 1 .. 4.  (Other kernels have names of that form -- the reset kernels on the planet count 2 .. 4, the replay
    sampler on 1 and 4 -- so the form alone does not tell.)  Both views must give the same templates, and they must be the ones
    tests/test_gpu_net_widths.py says its families launch -- another net kernel fails here until its width test exists"""
    from space_gym_amd import build
    from test_gpu_net_widths import FAMILY_KERNELS
    classes = collections.defaultdict(list)
    for row in engine_asm.resource_rows():
        m = re.match(r"_Z\d+(\w+_kernel)ILi(\d+)EE", row["name"])
        if m:
            classes[m.group(1)].append(int(m.group(2)))
    reported = {k for k, cs in classes.items() if sorted(cs) == [1, 2, 3, 4]}
    declared = set()
    for name in build.HEADERS:
        if name.endswith(".inc"):
            src = open(os.path.join(build.CSRC, name)).read()
            declared |= set(re.findall(r"__launch_bounds__\(policy(?:_grad)?_block\(NT\)\)\s+void\s+(\w+)\(", src))
    assert declared and declared == reported, (sorted(declared - reported), sorted(reported - declared))
    assert all(sorted(classes[k]) == [1, 2, 3, 4] for k in declared), {k: classes[k] for k in declared}
    named = [k for kernels in FAMILY_KERNELS.values() for k in kernels]
    assert len(named) == len(set(named)), named
    assert declared == set(named), (sorted(declared - set(named)), sorted(set(named) - declared))
