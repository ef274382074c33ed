"""CPU tests of the episode statistics (sg_set_episode_stats): the ctypes mirror of sg_episode_list, and the Python argument
checks of the public API with the native calls stubbed (they run without a GPU: nothing reaches a kernel)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_sg_episode_list_layout_matches_the_header():
    """the ctypes mirror of sg_episode_list has the fields of include/spacegym.h in the same order, with the same widths"""
    from space_gym_amd import _native
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct sg_episode_list {"):header.index("} sg_episode_list;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct sg_episode_list {", "")
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [d.split()[-1].lstrip("*") for d in decls]
    assert names == [f for f, _ in _native.SgEpisodeList._fields_], names
    for d, (_, ctype) in zip(decls, _native.SgEpisodeList._fields_):
        assert ("*" in d) == (ctype is C.c_void_p), d
    assert _native.SgEpisodeList._fields_[-1][1] is C.c_uint32
    assert C.sizeof(_native.SgEpisodeList) == 6 * 8  # five pointers and a uint32, padded like the C struct


def test_episode_entry_points_are_declared():
    from space_gym_amd import _native
    for name in ("sg_set_episode_stats", "sg_step_device_episodes", "sg_step_episodes", "sg_step_end_episodes",
                 "sg_rollout_device_episodes"):
        assert name in _native.SYMBOLS
    from space_gym_amd.vector_env import _ENGINE_KWARGS
    assert "episode_statistics" in _ENGINE_KWARGS


class _StubLib:
    """stands in for the native library: records the calls, returns success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("sg_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return b"" if name == "sg_last_error" else 0
        return fn

    def names(self):
        return [c[0] for c in self.calls]


def _fake_cuda(t):
    """a CPU tensor that passes for a CUDA tensor on device 0 (the checks read is_cuda / device; nothing dereferences it)"""
    import torch

    class FakeCuda(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))
    return t.as_subclass(FakeCuda)


def _stub_env(B=8, D=13, stats=False):
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    env = SpaceGymVectorEnv.__new__(SpaceGymVectorEnv)
    env._lib = _StubLib()
    env._h = C.c_void_p(1)
    env.num_envs, env.obs_dim, env.device, env.discrete = B, D, 0, False
    env.copy, env.want_terminal_obs, env.validate_actions = True, False, True
    env._pending, env._blocks, env._torch_bufs, env._pinned = False, {}, {}, []  # (_torch_bufs: no default CUDA buffers)
    env._episode_stats = stats
    env._stream = lambda: None
    return env


def _step_args(env):
    import torch
    B, D = env.num_envs, env.obs_dim
    a = _fake_cuda(torch.zeros((B, 2), dtype=torch.float32))
    out = dict(obs=_fake_cuda(torch.zeros((B, D))), reward=_fake_cuda(torch.zeros(B)),
               done=_fake_cuda(torch.zeros(B, dtype=torch.uint8)), trunc=_fake_cuda(torch.zeros(B, dtype=torch.uint8)))
    return a, out


def _rollout_args(env, K=4):
    import torch
    B, D = env.num_envs, env.obs_dim
    return (_fake_cuda(torch.zeros((K, B, 2))), _fake_cuda(torch.zeros((K, B, D))), _fake_cuda(torch.zeros((K, B))),
            _fake_cuda(torch.zeros((K, B), dtype=torch.uint8)), _fake_cuda(torch.zeros((K, B), dtype=torch.uint8)))


def _episode_list(cap=16, **over):
    import torch
    el = dict(count=torch.zeros(1, dtype=torch.int32), step_env=torch.zeros((cap, 2), dtype=torch.int32),
              r=torch.zeros(cap, dtype=torch.float64), l=torch.zeros(cap, dtype=torch.int32), truncated=torch.zeros(cap, dtype=torch.uint8))
    el.update(over)
    return {k: _fake_cuda(v) for k, v in el.items()}


def test_step_torch_episodes_refused_while_statistics_are_off():
    import torch
    env = _stub_env(stats=False)
    a, out = _step_args(env)
    rows = dict(r=_fake_cuda(torch.zeros(8, dtype=torch.float64)), l=_fake_cuda(torch.zeros(8, dtype=torch.int32)))
    with pytest.raises(ValueError, match="episode statistics are off"):
        env.step_torch(a, out=out, episodes=rows)
    assert "sg_step_device_episodes" not in env._lib.names()


@pytest.mark.parametrize("bad", ["r_dtype", "l_dtype", "r_shape", "l_shape", "r_host"])
def test_step_torch_episodes_rows_are_checked(bad):
    import torch
    env = _stub_env(stats=True)
    a, out = _step_args(env)
    r, l = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32)
    rows = dict(r=_fake_cuda(r), l=_fake_cuda(l))
    if bad == "r_dtype":
        rows["r"] = _fake_cuda(r.float())
    elif bad == "l_dtype":
        rows["l"] = _fake_cuda(l.long())
    elif bad == "r_shape":
        rows["r"] = _fake_cuda(torch.zeros(9, dtype=torch.float64))
    elif bad == "l_shape":
        rows["l"] = _fake_cuda(torch.zeros((8, 1), dtype=torch.int32))
    else:
        rows["r"] = r  # host memory
    with pytest.raises(ValueError):
        env.step_torch(a, out=out, episodes=rows)
    assert "sg_step_device_episodes" not in env._lib.names()


def test_step_torch_episodes_reach_the_native_call():
    import torch
    env = _stub_env(stats=True)
    a, out = _step_args(env)
    rows = dict(r=_fake_cuda(torch.zeros(8, dtype=torch.float64)), l=_fake_cuda(torch.zeros(8, dtype=torch.int32)))
    env.step_torch(a, out=out, episodes=rows)
    name, args = env._lib.calls[-1]
    assert name == "sg_step_device_episodes"
    assert args[7].value == rows["r"].data_ptr() and args[8].value == rows["l"].data_ptr()
    env.step_torch(a, out=out)  # without episodes=: the plain entry point (the sums still advance on the device)
    assert env._lib.calls[-1][0] == "sg_step_device"


def test_rollout_episodes_refused_while_statistics_are_off():
    env = _stub_env(stats=False)
    args = _rollout_args(env)
    with pytest.raises(ValueError, match="episode statistics are off"):
        env.rollout_torch(*args, episodes=_episode_list())
    with pytest.raises(ValueError, match="episode statistics are off"):
        env.prepare_rollout(*args, episodes=_episode_list())
    assert not any(n.startswith("sg_rollout") for n in env._lib.names())


@pytest.mark.parametrize("field,bad", [("r", "float32"), ("l", "int64"), ("truncated", "bool"), ("step_env", "shape"),
                                       ("count", "float32"), ("count", "shape")])
def test_rollout_episode_list_is_checked(field, bad):
    import torch
    env = _stub_env(stats=True)
    args = _rollout_args(env)
    cap = 16
    if bad == "shape":
        t = torch.zeros(cap, dtype=torch.int32) if field == "step_env" else torch.zeros(2, dtype=torch.int32)
    else:
        t = torch.zeros(cap, dtype=getattr(torch, bad))
    el = _episode_list(cap, **{field: t})
    with pytest.raises(ValueError):
        env.rollout_torch(*args, episodes=el)
    with pytest.raises(ValueError):
        env.prepare_rollout(*args, episodes=el)
    assert not any(n.startswith("sg_rollout") for n in env._lib.names())


def test_rollout_episode_list_reaches_the_native_call(monkeypatch):
    import torch
    env = _stub_env(stats=True)
    args = _rollout_args(env)
    el = _episode_list(16)
    env.rollout_torch(*args, episodes=el)
    name, a = env._lib.calls[-1]
    assert name == "sg_rollout_device_episodes" and a[1] == 4 and a[7] is None
    lst = a[8]._obj
    assert (lst.count, lst.step_env, lst.ret, lst.length, lst.truncated, lst.capacity) == (
        el["count"].data_ptr(), el["step_env"].data_ptr(), el["r"].data_ptr(), el["l"].data_ptr(), el["truncated"].data_ptr(), 16)
    term = {k: _fake_cuda(v) for k, v in dict(count=torch.zeros(1, dtype=torch.int32), step_env=torch.zeros((5, 2), dtype=torch.int32),
                                               obs=torch.zeros((5, env.obs_dim))).items()}
    env.rollout_torch(*args, terminal=term, episodes=el)
    name, a = env._lib.calls[-1]
    assert name == "sg_rollout_device_episodes" and a[7]._obj.capacity == 5
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev: type("S", (), {"cuda_stream": 0})())
    call = env.prepare_rollout(*args, episodes=el)
    n0 = len(env._lib.calls)
    call()
    assert len(env._lib.calls) == n0 + 1 and env._lib.calls[-1][0] == "sg_rollout_device_episodes"
    assert env._lib.calls[-1][1][8]._obj.capacity == 16


def test_episode_records_sorts_and_reports_overflow():
    import torch
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    el = dict(count=torch.tensor([3], dtype=torch.int32), step_env=torch.tensor([[2, 5], [0, 7], [2, 1], [9, 9]], dtype=torch.int32),
              r=torch.tensor([1.5, -2.0, 0.25, 0.0], dtype=torch.float64), l=torch.tensor([3, 1, 45, 0], dtype=torch.int32),
              truncated=torch.tensor([0, 0, 1, 0], dtype=torch.uint8))
    rec = SpaceGymVectorEnv.episode_records(el)
    assert rec["step"].tolist() == [0, 2, 2] and rec["env"].tolist() == [7, 1, 5]
    assert rec["r"].tolist() == [-2.0, 0.25, 1.5] and rec["l"].tolist() == [1, 45, 3]
    assert rec["truncated"].tolist() == [False, True, False] and rec["r"].dtype == np.float64
    el["count"][0] = 5
    with pytest.raises(OverflowError):
        SpaceGymVectorEnv.episode_records(el)


def test_set_episode_statistics_switches_the_handle():
    env = _stub_env(stats=False)
    env.set_episode_statistics(True)
    assert env.episode_statistics and env._lib.calls[-1] == ("sg_set_episode_stats", (env._h, 1))
    env._pending = True
    with pytest.raises(RuntimeError):
        env.set_episode_statistics(False)
    env._pending = False
    env.set_episode_statistics(False)
    assert not env.episode_statistics and env._lib.calls[-1][1][1] == 0


@pytest.mark.parametrize("copy", [True, False])
def test_step_info_carries_the_episode_rows(copy):
    """step() with statistics on: info["episode"] = {"r": float64 [B], "l": int32 [B]} and info["_episode"] = done, taken from
    the rows sg_step_end_episodes points at (copies or views, as the other outputs)"""
    B, D = 4, 13
    env = _stub_env(B, D, stats=True)
    env.copy = copy
    blk = dict(obs=np.zeros((B, D), np.float32), rew=np.arange(B, dtype=np.float32), done=np.array([0, 1, 0, 1], np.uint8),
               trunc=np.array([0, 0, 0, 1], np.uint8), r=np.array([np.nan, 2.5, np.nan, -1.25]), l=np.array([-1, 7, -1, 45], np.int32))

    def step_end(h, *outs):
        for o, k in zip(outs, ("obs", "rew", "done", "trunc")):
            o._obj.value = blk[k].ctypes.data
        outs[4]._obj.value = None
        return 0

    def step_end_episodes(h, r, l):
        r._obj.value, l._obj.value = blk["r"].ctypes.data, blk["l"].ctypes.data
        return 0
    env._lib = type("L", (), {"sg_step_begin": lambda self, *a: 0, "sg_step_end": lambda self, *a: step_end(*a),
                              "sg_step_end_episodes": lambda self, *a: step_end_episodes(*a),
                              "sg_last_error": lambda self, h: b"", "sg_destroy": lambda self, h: 0})()
    env._act = np.zeros((B, 2), np.float32)
    obs, rew, done, info = env.step(np.zeros((B, 2), np.float32))
    ep = info["episode"]
    assert ep["r"].dtype == np.float64 and ep["l"].dtype == np.int32 and info["_episode"].dtype == np.bool_
    assert info["_episode"].tolist() == [False, True, False, True]
    assert np.array_equal(ep["r"], blk["r"], equal_nan=True) and ep["l"].tolist() == [-1, 7, -1, 45]
    assert np.shares_memory(ep["r"], blk["r"]) == (not copy)


def test_multi_device_front_ends_refuse_episode_statistics():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    with pytest.raises(NotImplementedError, match="episode_statistics"):
        MultiDeviceVectorEnv("GoalContinuous3P-v0", 16, [0, 0], episode_statistics=True)
