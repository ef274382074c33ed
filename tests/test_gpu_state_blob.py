"""GPU tests of the host snapshot blob (save_state / load_state, sg_state_bytes / sg_save_state / sg_load_state) against
tests/golden/state_blobs.npz: blobs of 5 envs of four ids under every combination of episode statistics, normalization and
reward profiles (tools/gen_state_blobs.py), taken from the library as it was before the blob's layout was described in one
place.  The bytes of every version must stay what they are and every blob must still load.  The layout the tests expect is
spelled out here by concatenation, independently of the package's own table.  All assertions are equalities."""
import re

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

B = 5
EPISODES, NORMALIZE, PROFILES = 1, 2, 4
F4, U4, F8 = np.float32, np.uint32, np.float64
_STATE = [("q0", F4, 4), ("q1", F4, 4), ("ctr", U4, 2), ("aux", U4, 4)]
COLUMNS = {
    "GoalContinuous2P-v0": _STATE + [("pl0", F4, 4), ("cshift", F4, 4)],
    "GoalContinuous4P-v0": _STATE + [("pl0", F4, 4), ("pl1", F4, 4), ("cshift", F4, 4)],
    "KeplerCircleOrbit-v0": _STATE,
    "KeplerRandomOrbits-v0": _STATE + [("orbd", F8, 2)],
}
CASES = [(env_id, bits) for env_id in COLUMNS for bits in range(8)]
HEADER_BYTES, NORMALIZE_BYTES, PROFILE_BYTES, N_PROFILES = 48, 48, 72, 3
REFUSED_SHORT = r"bytes, \d+ expected|truncated snapshot"


@pytest.fixture(scope="module")
def golden():
    return load_golden("state_blobs")


def make(env_id, n=B, seed=4242):
    import space_gym_amd as sg
    return sg.make_vec(env_id, n, device=0, seed=seed, max_episode_steps=10)


def expected_blocks(env_id, bits, obs_dim):
    """[(name, dtype, shape, offset)] of the blob of a combination, and its length"""
    S = obs_dim + 1
    blocks = [("header", np.uint8, (HEADER_BYTES,))] + [(name, dt, (B, w)) for name, dt, w in COLUMNS[env_id]]
    if bits >= 2:  # version 3
        blocks += [("flags", U4, (1, 2))]
    if bits & EPISODES:
        blocks += [("ep_ret", F8, (B, 1)), ("ep_len", np.int32, (B, 1))]
    if bits & NORMALIZE:
        blocks += [("norm_config", np.uint8, (NORMALIZE_BYTES,)), ("norm_mean", F8, (S,)), ("norm_var", F8, (S,)),
                   ("norm_count", F8, (S,)), ("norm_returns", F8, (B,))]
    if bits & PROFILES:
        blocks += [("profile_count", U4, (2,)), ("profiles", np.uint8, (N_PROFILES * PROFILE_BYTES,)), ("profile_index", np.uint8, (B,))]
    out, off = [], 0
    for name, dt, shape in blocks:
        out.append((name, dt, shape, off))
        off += int(np.prod(shape)) * np.dtype(dt).itemsize
    return out, off


@pytest.mark.parametrize("env_id,bits", CASES)
def test_a_golden_blob_loads_and_is_saved_again_byte_for_byte(golden, env_id, bits):
    blob = golden[f"{env_id}_{bits}"]
    env = make(env_id)
    env.load_state(blob)
    again = env.save_state()
    assert again.size == int(env._lib.sg_state_bytes(env._h)) == blob.size
    assert np.array_equal(again, blob)
    env.close()


@pytest.mark.parametrize("env_id,bits", CASES)
def test_snapshot_columns_serves_every_block_where_it_lies(golden, env_id, bits):
    blob = golden[f"{env_id}_{bits}"]
    env = make(env_id)
    blocks, end = expected_blocks(env_id, bits, env.obs_dim)
    assert end == blob.size
    assert int(blob[4:8].view(U4)[0]) == (3 if bits >= 2 else 2 if bits & EPISODES else 1)
    out = env.snapshot_columns(blob)
    assert list(out) == [name for name, _, _, _ in blocks[1:]]
    for name, dt, shape, off in blocks[1:]:
        view = out[name]
        assert view.dtype == dt and view.shape == shape, name
        assert view.tobytes() == blob[off:off + view.nbytes].tobytes(), name
    if bits >= 2:
        assert out["flags"].tolist() == [[bits, 0]]
    if bits & PROFILES:
        assert out["profile_count"].tolist() == [N_PROFILES, 0] and out["profile_index"].tolist() == [2, 0, 1, 1, 2]
    env.close()


@pytest.mark.parametrize("env_id,bits", CASES)
def test_a_blob_cut_short_of_a_block_boundary_is_refused_and_changes_nothing(golden, env_id, bits):
    from space_gym_amd._native import NativeError
    blob = golden[f"{env_id}_{bits}"]
    env = make(env_id)
    env.reset()
    before = env.save_state()
    blocks, end = expected_blocks(env_id, bits, env.obs_dim)
    for boundary in [off for _, _, _, off in blocks[1:]] + [end]:
        with pytest.raises(NativeError) as err:
            env.load_state(blob[:boundary - 1])
        assert re.search(REFUSED_SHORT, str(err.value)) is not None, (boundary, str(err.value))
        assert np.array_equal(env.save_state(), before), boundary
    env.close()


@pytest.mark.parametrize("env_id,bits", [c for c in CASES if c[1] >= 2])
def test_a_flags_word_with_an_unknown_bit_is_refused(golden, env_id, bits):
    from space_gym_amd._native import NativeError
    bad = golden[f"{env_id}_{bits}"].copy()
    (flags_off,) = [off for name, _, _, off in expected_blocks(env_id, bits, 0)[0] if name == "flags"]
    bad[flags_off:flags_off + 4] = np.frombuffer(np.uint32(bits | 8).tobytes(), np.uint8)
    env = make(env_id)
    env.reset()
    before = env.save_state()
    with pytest.raises(NativeError, match="unknown blocks"):
        env.load_state(bad)
    assert np.array_equal(env.save_state(), before)
    env.close()


@pytest.mark.parametrize("bits", [0, 7])
@pytest.mark.parametrize("env_id,other_id,other_n", [("GoalContinuous2P-v0", "GoalContinuous4P-v0", B), ("GoalContinuous4P-v0", "KeplerCircleOrbit-v0", B),
                                                     ("KeplerCircleOrbit-v0", "KeplerRandomOrbits-v0", B), ("KeplerRandomOrbits-v0", "KeplerRandomOrbits-v0", B + 1),
                                                     ("GoalContinuous4P-v0", "GoalContinuous4P-v0", B - 1)])
def test_a_blob_of_another_id_or_batch_size_is_refused(golden, env_id, other_id, other_n, bits):
    from space_gym_amd._native import NativeError
    env = make(other_id, n=other_n)
    env.reset()
    before = env.save_state()
    with pytest.raises(NativeError, match="the snapshot was taken from a different env id or batch size"):
        env.load_state(golden[f"{env_id}_{bits}"])
    assert np.array_equal(env.save_state(), before)
    env.close()
