"""CPU tests of the masked reset (sg_reset_masked / sg_reset_masked_device): the declarations of the two entry points, and the
Python argument checks of reset(mask=...) / reset_torch(mask=...) with the native calls stubbed (nothing reaches a kernel)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_episode_stats import _fake_cuda, _stub_env


def _header_args(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spacegym.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    for name, n in (("sg_reset_masked", 3), ("sg_reset_masked_device", 4)):
        assert len(_header_args(name)) == n
        assert name in _native.SYMBOLS and len(_native.SYMBOLS[name][1]) == n
    assert "uint8_t *mask_host" in _header_args("sg_reset_masked")[1]
    assert "uint8_t *mask_dev" in _header_args("sg_reset_masked_device")[1]


def _env(B=8, D=13):
    env = _stub_env(B=B, D=D)
    env._obs = np.zeros((B, D), np.float32)
    env._last_obs = None
    return env


@pytest.mark.parametrize("dtype", [np.bool_, np.uint8])
def test_numpy_mask_reaches_the_native_call(dtype):
    env = _env()
    mask = np.array([1, 0, 0, 1, 0, 0, 0, 1], dtype)
    env.reset(mask=mask)
    name, args = env._lib.calls[-1]
    assert name == "sg_reset_masked"
    assert args[1].value != args[2].value and args[2].value == env._obs.ctypes.data
    env.reset()
    assert env._lib.calls[-1][0] == "sg_reset"  # without mask=: the full reset


def test_numpy_mask_keeps_the_last_step_rows():
    """the other rows of the returned buffer are what the last NumPy-path call returned (here: a step's block)"""
    env = _env()
    env._last_obs = np.arange(8 * 13, dtype=np.float32).reshape(8, 13)
    out = env.reset(mask=np.zeros(8, bool))
    assert np.array_equal(out, env._last_obs) and env._last_obs is env._obs


@pytest.mark.parametrize("bad", [np.zeros(7, bool), np.zeros((8, 1), np.uint8), np.zeros(8, np.int64), np.zeros(8, np.float32)])
def test_numpy_mask_is_checked(bad):
    env = _env()
    with pytest.raises(ValueError, match="mask"):
        env.reset(mask=bad)
    assert "sg_reset_masked" not in env._lib.names()


@pytest.mark.parametrize("dtype", ["bool", "uint8"])
def test_torch_mask_reaches_the_native_call(dtype):
    import torch
    env = _env()
    out = _fake_cuda(torch.zeros((8, 13)))
    m = torch.tensor([1, 0, 1, 0, 0, 0, 0, 1], dtype=getattr(torch, dtype))
    mask = _fake_cuda(m)
    got = env.reset_torch(out=out, mask=mask)
    name, args = env._lib.calls[-1]
    assert name == "sg_reset_masked_device" and got is out
    assert args[1].value == m.data_ptr() and args[2].value == out.data_ptr()  # a bool mask is taken as it is (no copy)


@pytest.mark.parametrize("bad", ["length", "dtype", "host", "2d", "stride"])
def test_torch_mask_is_checked(bad):
    import torch
    env = _env()
    out = _fake_cuda(torch.zeros((8, 13)))
    mask = {"length": _fake_cuda(torch.zeros(9, dtype=torch.uint8)),
            "dtype": _fake_cuda(torch.zeros(8, dtype=torch.int32)),
            "host": torch.zeros(8, dtype=torch.uint8),
            "2d": _fake_cuda(torch.zeros((8, 1), dtype=torch.uint8)),
            "stride": _fake_cuda(torch.zeros(16, dtype=torch.uint8)[::2])}[bad]
    with pytest.raises(ValueError, match="mask"):
        env.reset_torch(out=out, mask=mask)
    assert "sg_reset_masked_device" not in env._lib.names()


def test_multi_device_front_ends_refuse_a_mask():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    md = MultiDeviceVectorEnv.__new__(MultiDeviceVectorEnv)
    with pytest.raises(NotImplementedError, match="mask"):
        md.reset_torch(mask=np.ones(16, bool))
    with pytest.raises(NotImplementedError, match="mask"):
        md.reset(mask=np.ones(16, bool))
    with pytest.raises(NotImplementedError, match="mask"):
        ShardedVectorEnv.__new__(ShardedVectorEnv).reset(mask=np.ones(16, bool))
