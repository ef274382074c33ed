"""Reward profiles without a GPU: the ctypes mirror of sg_reward_profile, the Python argument checks, the multi-device front
ends' refusal, and the device assembly of the profiled one-wave step kernels (no GPU needed to compile it)."""
import os

import numpy as np
import pytest

from conftest import ROOT


def _bare_env(family="goal", num_envs=8):
    """a SpaceGymVectorEnv without a handle: enough for the checks made before the library is called"""
    from space_gym_amd import _native
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    env = object.__new__(SpaceGymVectorEnv)
    env._lib = _native.load()
    env._pending = False
    env._h = None
    env.num_envs = num_envs
    env.spec = {"family": family}
    return env


def test_sg_reward_profile_layout_matches_the_header():
    """the ctypes mirror of sg_reward_profile has the fields of include/spacegym.h in the same order"""
    import ctypes
    import re
    from space_gym_amd import _native
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct sg_reward_profile {"):header.index("} sg_reward_profile;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct sg_reward_profile {", "").strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        names += [n.strip() for n in rest.split(",")]
    assert names == [f for f, _ in _native.SgRewardProfile._fields_], names
    assert ctypes.sizeof(_native.SgRewardProfile) == 72


def test_reward_keywords_are_the_reference_reward_keywords():
    from space_gym_amd.vector_env import REWARD_KWARGS, REWARD_PROFILES_MAX
    from space_gym_amd import _native
    fields = [f for f, _ in _native.SgRewardProfile._fields_][1:]
    assert fields == list(REWARD_KWARGS["goal"]) + list(REWARD_KWARGS["kepler"])
    assert REWARD_PROFILES_MAX == 256


@pytest.mark.parametrize("bad, what", [({"survival_reward_scal": 1.0}, "unknown keyword"),
                                       ({"max_engine_force": 1.0}, "physics keyword"),
                                       ({"ship_moi": 2.0}, "physics keyword"),
                                       ({"step_size": 0.05}, "physics keyword"),
                                       ({"n_planets": 3}, "physics keyword"),
                                       ({"ref_orbit_a": 1.5}, "physics keyword")])
def test_profile_keywords_are_checked(bad, what):
    env = _bare_env("goal")
    with pytest.raises(ValueError, match=what):
        env.set_reward_profiles([{}, bad])
    with pytest.raises(TypeError):
        env.set_reward_profiles([("survival_reward_scale", 1.0)])


def test_at_most_256_profiles():
    env = _bare_env("kepler")
    with pytest.raises(ValueError, match="at most 256"):
        env.set_reward_profiles([{}] * 257)


def test_env_profile_indices_are_checked():
    env = _bare_env("goal", num_envs=8)
    env.reward_profiles = lambda: [{}] * 4  # four profiles on
    with pytest.raises(ValueError, match="shape"):
        env.set_env_profiles(np.zeros(7, np.uint8))
    with pytest.raises(ValueError, match="shape"):
        env.set_env_profiles(np.zeros((8, 1), np.uint8))
    with pytest.raises(ValueError, match="integers"):
        env.set_env_profiles(np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="integers"):
        env.set_env_profiles(np.zeros(8, bool))
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        env.set_env_profiles(np.array([0, 1, 2, 3, 4, 0, 0, 0]))
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        env.set_env_profiles([0, 1, 2, 3, -1, 0, 0, 0])
    env.reward_profiles = lambda: []
    with pytest.raises(ValueError, match="off"):
        env.set_env_profiles(np.zeros(8, np.uint8))


def test_multi_device_front_ends_refuse_profiles():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    with pytest.raises(NotImplementedError, match="reward_profiles"):
        MultiDeviceVectorEnv("GoalContinuous3P-v0", 64, [0, 0], reward_profiles=[{"survival_reward_scale": 0.5}])
    with pytest.raises(NotImplementedError, match="reward_profiles"):
        ShardedVectorEnv("GoalContinuous3P-v0", 64, reward_profiles=[{"survival_reward_scale": 0.5}])


def test_profiled_step_kernels_wait_for_memory_only_at_the_top_of_a_pass():
    """goal_step_profiled_kernel / kepler_step_profiled_kernel keep what test_host_logic checks of the one-wave step kernels:
    the profile indices come with the subtile's LDS-DMA group and the table is in LDS, so behind the loop's group of
    global_load_lds at least 300 instructions follow without an `s_waitcnt vmcnt`.  Every new kernel: no spill, no scratch; the
    one-wave step kernels at two waves per SIMD and the wave-pair rollout kernels at most 256 registers."""
    import engine_asm
    # 2P / 3P / 4P x two steerings, Kepler x two steerings; the prologue's group and the loop's, each with the profile indices
    engine_asm.assert_no_memory_wait_behind_dma(r"^_Z\d+(goal|kepler)_step_profiled_kernelI\w*:", n_kernels=8, min_dma=16)
    # resources of every profiled kernel, from the code object's kernel descriptors
    kernels = engine_asm.descriptors(r"\S*profile\S*")
    assert len(kernels) == 8 + 8 + 12 + 2 + 1  # one-wave and wave-pair step kernels, the rollout kernels, the index copy
    for name, field in kernels:
        assert field["private_segment_fixed_size"] == 0, name
        if ("_step_profiled_kernel" in name and "pair" not in name) or "_rollout_profiled_kernel" in name:
            assert field["next_free_vgpr"] <= 256, name
    spills = engine_asm.spill_counts(r"\S*profile\S*")
    assert len(spills) == 31 and all(n == 0 for _, n in spills), spills
