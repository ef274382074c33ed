"""The edge nets of the small-MLP kernels, for tests/test_gpu_net_widths.py (GPU) and tests/test_net_widths.py (CPU).

Every net entry point launches one of four instantiations of its kernel template, chosen by select_policy_tiles (sg_engine.hip) from
NT = ceil(hidden / 32) = 1 .. 4: the 32-output tiles a lane keeps in registers.  NT fixes the forward workgroup (policy_block: 256, 256,
128, 128 lanes), the row tile of the MFMA backward (policy_grad_block: R = 256, 128, 64, 64) and the dynamic-LDS limit nets_begin raises
for the instantiation, sized for its widest net: 32 NT wide with three hidden layers.  test_gpu_policy.NETS (hidden 1, 33, 64, 128) and
the other files' 5, 16, 40 and 97 leave class 3 and every class's widest net but the fourth's unvisited; WIDTH_NETS are the widths at
which a chunk bound, an LDS size, a tile-to-wave assignment or the bias column of the backward changes.

The inputs of every gradient case are built here, from NumPy alone, so that the CPU file can check each case's 1 % cap on the very
arrays the GPU file runs."""
import numpy as np

import dqn_model
import squashed_model
from policy_model import random_policy
from q_model import random_qnet

# (hidden, n_hidden, why)
_TABLE = [
    (31, 2, "in + 1 = 32: the bias is the last column of an MFMA column tile"),
    (32, 3, "class 1 full, no padding, the staging loop's power-of-two range equal to `in`, largest LDS of the class"),
    (64, 3, "largest LDS of class 2 (64 has run with 2 layers only)"),
    (65, 1, "first width of class 3: the third chunk holds one output"),
    (80, 2, "inside class 3"),
    (96, 3, "class 3 full, largest LDS of the class"),
    (127, 2, "in + 1 = 128: four full column tiles, bias last"),
]
WIDTH_NETS = [(hidden, n_hidden) for hidden, n_hidden, _ in _TABLE]
WHY = {(hidden, n_hidden): why for hidden, n_hidden, why in _TABLE}

N = 200  # rows: two ragged forward workgroups at 128 lanes, one partial at 256; four ragged row tiles at R = 64, two at 128, one partial at 256
BIG = (80, 1, "tanh", 256 * 64 + 300)  # class 3 past the grid cap of 256 workgroups of R = 64 rows: the first 5 take a second row tile
GRAD_ROWS = {1: 256, 2: 128, 3: 64, 4: 64}  # policy_grad_block by class
TWO_HANDLE_WIDTHS = [32, 64, 96, 128]  # each class filled, on two handles alive together:
WIDE_ID, NARROW_ID = "GoalContinuous4P-v0", "KeplerCircleOrbit-v0"  # the widest observation (17) and the narrowest (10)

OBS_DIM = {"GoalContinuous2P-v0": 13, "GoalDiscrete2-v0": 13, "GoalContinuous3P-v0": 15, "GoalDiscrete3-v0": 15, "GoalContinuous4P-v0": 17,
           "GoalDiscrete4-v0": 17, "KeplerCircleOrbit-v0": 10, "KeplerDiscrete-v0": 10}


def tile_class(hidden):
    """NT of select_policy_tiles"""
    return -(-hidden // 32)


def activation_of(i):
    """both activations alternate over the table"""
    return ("tanh", "relu")[i % 2]


def ids_of(hidden, n_hidden):
    """(continuous id, discrete id) of a net: three hidden layers on the 4P ids (observation 17, a Q critic's input 19: the largest LDS
    footprint a class can have), width 31 on the 2P ids (observation 13), the others on the ids the older files use"""
    planets = 4 if n_hidden == 3 else 2 if hidden == 31 else 3
    return "GoalContinuous%dP-v0" % planets, "GoalDiscrete%d-v0" % planets


def cases():
    """[(hidden, n_hidden, activation)] over the table"""
    return [(hidden, n_hidden, activation_of(i)) for i, (hidden, n_hidden) in enumerate(WIDTH_NETS)]


# ---- the inputs of the gradient cases, seeded n + hidden as the older files' cases
def policy_case(env_id, n, hidden, n_hidden):
    """test_gpu_policy_grad._run_grad_case's draws: policy, obs, action, g (logp, entropy, value)"""
    D, continuous = OBS_DIM[env_id], "Discrete" not in env_id
    rng = np.random.default_rng(n + hidden)
    pol = random_policy(rng, D, hidden, n_hidden, 2 if continuous else 6, critic=True, continuous=continuous)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    action = rng.standard_normal((n, 2)).astype(np.float32) if continuous else rng.integers(0, 6, n).astype(np.int32)
    g = {k: rng.standard_normal(n).astype(np.float32) for k in ("logp", "entropy", "value")}
    return dict(policy=pol, obs=obs, action=action, g=g)


def q_case(env_id, n, hidden, n_hidden):
    """test_gpu_q._run_grad_case's draws: two critics, obs, action, g (q1, q2); then an actor, eps and g_action for the actor chain"""
    D = OBS_DIM[env_id]
    rng = np.random.default_rng(n + hidden)
    critics = random_qnet(rng, D, hidden, n_hidden, 2)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    action = rng.standard_normal((n, 2)).astype(np.float32)
    g = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    pol = random_policy(rng, D, hidden, n_hidden, 2)
    eps, ga = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    return dict(critics=critics, obs=obs, action=action, g=g, policy=pol, eps=eps, g_action=ga)


def squashed_case(env_id, n, hidden, n_hidden):
    return squashed_model.case(OBS_DIM[env_id], n, hidden, n_hidden, seed=n + hidden)


def dqn_case(env_id, n, hidden, n_hidden):
    return dqn_model.case(OBS_DIM[env_id], n, hidden, n_hidden, seed=n + hidden)


# ---- the float64 / float32-sequential references of those cases, as flat {name: array} dicts
def policy_reference(c, activation, dtype):
    import policy_grad_model
    g = c["g"]
    return policy_grad_model.flat(policy_grad_model.evaluate(c["policy"], c["obs"], c["action"], g["logp"], g["entropy"], g["value"],
                                                             activation=activation, dtype=dtype))


def q_reference(c, activation, dtype):
    """both critics' parameters and the [n, 2] action gradient, the first critic's term before the second's (test_gpu_q's composition)"""
    import q_model
    named, da = {}, np.zeros((c["obs"].shape[0], 2), dtype)
    for k in range(2):
        r = q_model.q_evaluate([c["critics"][k]], c["obs"], c["action"], c["g"][k], activation=activation, dtype=dtype)
        named.update({name.replace("critic0", "critic%d" % k): v for name, v in q_model.q_flat(r).items()})
        da = da + r["action"]
    named["action"] = da
    return named


def actor_chain_reference(c, activation, dtype):
    import q_model
    return q_model.flat(q_model.action(c["policy"], c["obs"], c["eps"], c["g_action"], activation=activation, dtype=dtype))


def squashed_reference(c, activation, dtype):
    return squashed_model.grad_reference(c, activation, "both", dtype)


def dqn_reference(c, activation, dtype):
    return dqn_model.grad_reference(c, activation, "both", dtype)


def gradient_cases():
    """[(family, env_id, n, hidden, n_hidden, activation, case constructor, [reference, ...])]: every gradient case of
    tests/test_gpu_net_widths.py that is held to a tolerance (the population cases are held to the single call's bits, the PPO cases
    take their rows from a rollout on the device and assert their caps where they run)"""
    out = []
    for hidden, n_hidden, activation in cases():
        cont, disc = ids_of(hidden, n_hidden)
        out.append(("policy", cont, N, hidden, n_hidden, activation, policy_case, [policy_reference]))
        out.append(("policy", disc, N, hidden, n_hidden, activation, policy_case, [policy_reference]))
        out.append(("q", cont, N, hidden, n_hidden, activation, q_case, [q_reference, actor_chain_reference]))
        out.append(("squashed", cont, N, hidden, n_hidden, activation, squashed_case, [squashed_reference]))
        out.append(("dqn", disc, N, hidden, n_hidden, activation, dqn_case, [dqn_reference]))
    hidden, n_hidden, activation, n = BIG
    out.append(("policy", "GoalContinuous3P-v0", n, hidden, n_hidden, activation, policy_case, [policy_reference]))
    for hidden in TWO_HANDLE_WIDTHS:  # the two handles alive together: the widest net of the class on the 4P id, one layer on a Kepler id
        for env_id, n_hidden in ((WIDE_ID, 3), (NARROW_ID, 1)):
            if not any(c[:6] == ("policy", env_id, N, hidden, n_hidden, "tanh") for c in out):
                out.append(("policy", env_id, N, hidden, n_hidden, "tanh", policy_case, [policy_reference]))
    return out
