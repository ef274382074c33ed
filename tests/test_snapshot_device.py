"""CPU tests of the device-resident snapshots (sg_snapshot_bytes / sg_snapshot_device / sg_restore_device): the declarations of
the entry points, the Python argument checks of snapshot_torch / restore_torch / snapshot / restore with the native calls stubbed
(nothing reaches a kernel), the resources of the new kernels in the gfx950 build, and the status message of a refused restore."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import engine_asm
from test_episode_stats import _fake_cuda, _stub_env

ENV_ID = "GoalContinuous3P-v0"


def _header_args(name, ret=r"int"):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spacegym.h")).read(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_snapshot_bytes", "size_t") == ["const sg_env *env"]
    assert _header_args("sg_snapshot_device") == ["sg_env *env", "void *snap_dev", "size_t bytes", "void *hip_stream"]
    assert _header_args("sg_restore_device") == ["sg_env *env", "const void *snap_dev", "size_t bytes", "const uint8_t *mask_dev",
                                                 "const int32_t *src_dev", "float *obs_dev", "void *hip_stream"]
    for name, n in (("sg_snapshot_bytes", 1), ("sg_snapshot_device", 4), ("sg_restore_device", 7)):
        assert name in _native.SYMBOLS and len(_native.SYMBOLS[name][1]) == n
    import ctypes as C
    assert _native.SYMBOLS["sg_snapshot_bytes"][0] is C.c_size_t
    assert _native.SYMBOLS["sg_snapshot_device"][1][2] is C.c_size_t and _native.SYMBOLS["sg_restore_device"][1][2] is C.c_size_t


def _env(B=8, D=13):
    env = _stub_env(B=B, D=D)
    env.env_id = ENV_ID
    env._obs = np.zeros((B, D), np.float32)
    env._last_obs = None
    return env


def _snap(B=8, nbytes=64, env_id=ENV_ID):
    import torch
    from space_gym_amd import DeviceSnapshot
    return DeviceSnapshot(_fake_cuda(torch.zeros(nbytes, dtype=torch.uint8)), B, env_id)


def test_snapshot_torch_reuses_the_buffer_of_out():
    env = _env()
    snap = _snap()
    got = env.snapshot_torch(out=snap)
    assert got is snap and snap.num_envs == 8 and snap.env_id == ENV_ID
    name, args = env._lib.calls[-1]
    assert name == "sg_snapshot_device" and args[1].value == snap.buffer.data_ptr()
    assert env._lib.names()[-2] == "sg_snapshot_bytes"


@pytest.mark.parametrize("mask_dtype", [None, "bool", "uint8"])
@pytest.mark.parametrize("with_src", [False, True])
def test_restore_torch_arguments_reach_the_native_call(mask_dtype, with_src):
    import torch
    env = _env()
    snap = _snap()
    out = _fake_cuda(torch.zeros((8, 13)))
    m = torch.tensor([1, 0, 1, 0, 0, 0, 0, 1], dtype=getattr(torch, mask_dtype)) if mask_dtype else None
    s = torch.arange(8, dtype=torch.int32).flip(0).contiguous() if with_src else None
    got = env.restore_torch(snap, mask=_fake_cuda(m) if m is not None else None, src=_fake_cuda(s) if s is not None else None, out=out)
    name, args = env._lib.calls[-1]
    assert name == "sg_restore_device" and got is out
    assert args[1].value == snap.buffer.data_ptr() and args[2].value == snap.buffer.numel()
    assert (args[3].value == m.data_ptr()) if m is not None else args[3] is None  # a bool mask is taken as it is (no copy)
    assert (args[4].value == s.data_ptr()) if s is not None else args[4] is None
    assert args[5].value == out.data_ptr()


@pytest.mark.parametrize("bad", ["mask length", "mask dtype", "mask host", "mask 2d", "mask stride", "src dtype", "src length",
                                 "src host", "src stride", "out shape", "out dtype", "out host"])
def test_restore_torch_arguments_are_checked(bad):
    import torch
    env = _env()
    kw = dict(mask=None, src=None, out=_fake_cuda(torch.zeros((8, 13))))
    arg = bad.split()[0]
    kw[arg] = {"mask length": _fake_cuda(torch.zeros(9, dtype=torch.uint8)),
               "mask dtype": _fake_cuda(torch.zeros(8, dtype=torch.int32)),
               "mask host": torch.zeros(8, dtype=torch.uint8),
               "mask 2d": _fake_cuda(torch.zeros((8, 1), dtype=torch.uint8)),
               "mask stride": _fake_cuda(torch.zeros(16, dtype=torch.uint8)[::2]),
               "src dtype": _fake_cuda(torch.zeros(8, dtype=torch.int64)),
               "src length": _fake_cuda(torch.zeros(7, dtype=torch.int32)),
               "src host": torch.zeros(8, dtype=torch.int32),
               "src stride": _fake_cuda(torch.zeros(16, dtype=torch.int32)[::2]),
               "out shape": _fake_cuda(torch.zeros((8, 12))),
               "out dtype": _fake_cuda(torch.zeros((8, 13), dtype=torch.float64)),
               "out host": torch.zeros((8, 13))}[bad]
    with pytest.raises(ValueError, match=arg):
        env.restore_torch(_snap(), **kw)
    assert "sg_restore_device" not in env._lib.names()


@pytest.mark.parametrize("bad", ["batch", "id", "type", "host buffer", "buffer dtype"])
def test_the_snapshot_is_checked_against_the_handle(bad):
    import torch
    from space_gym_amd import DeviceSnapshot
    env = _env()
    snap = {"batch": _snap(B=9), "id": _snap(env_id="KeplerCircleOrbit-v0"), "type": torch.zeros(64, dtype=torch.uint8),
            "host buffer": DeviceSnapshot(torch.zeros(64, dtype=torch.uint8), 8, ENV_ID),
            "buffer dtype": DeviceSnapshot(_fake_cuda(torch.zeros(64, dtype=torch.int32)), 8, ENV_ID)}[bad]
    with pytest.raises(ValueError, match="snap"):
        env.restore_torch(snap, out=_fake_cuda(torch.zeros((8, 13))))
    with pytest.raises(ValueError, match="out"):
        env.snapshot_torch(out=snap)
    assert "sg_restore_device" not in env._lib.names() and "sg_snapshot_device" not in env._lib.names()


def test_a_buffer_smaller_than_the_handle_needs_is_refused():
    import ctypes as C
    import torch
    env = _env()
    real = env._lib.__getattr__

    class Lib:
        calls = env._lib.calls
        names = env._lib.names

        def __getattr__(self, name):
            return (lambda *a: 128) if name == "sg_snapshot_bytes" else real(name)
    env._lib = Lib()
    with pytest.raises(ValueError, match="snap.buffer"):
        env.restore_torch(_snap(nbytes=64), out=_fake_cuda(torch.zeros((8, 13))))
    env.restore_torch(_snap(nbytes=128), out=_fake_cuda(torch.zeros((8, 13))))
    assert env._lib.names() == ["sg_restore_device"] and isinstance(env._lib.calls[-1][1][2], C.c_size_t)


@pytest.mark.parametrize("bad", [dict(mask=np.zeros(7, bool)), dict(mask=np.zeros(8, np.int64)), dict(src=np.zeros(7, np.int32)),
                                 dict(src=np.zeros(8, np.float32)), dict(src=np.zeros((8, 1), np.int64))])
def test_numpy_restore_arguments_are_checked(bad):
    env = _env()
    with pytest.raises(ValueError, match=next(iter(bad))):
        env.restore(_snap(), **bad)
    assert "sg_restore_device" not in env._lib.names()


def test_multi_device_front_ends_refuse_snapshots():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        env = cls.__new__(cls)
        for call in (lambda: env.snapshot_torch(), lambda: env.snapshot(), lambda: env.restore_torch(None, mask=None),
                     lambda: env.restore(None, src=None)):
            with pytest.raises(NotImplementedError, match="snapshot / restore"):
                call()


def test_the_status_message_of_a_refused_restore_is_reachable():
    """the restore kernels set the status word to kStatusSnapshot; both readers of the word -- status_error (every later call)
    and sg_check_status (which clears it) -- have a message of their own for it, and the built library carries them"""
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    code = int(re.search(r"constexpr int kStatusSnapshot = (\d+);", src).group(1))
    others = [int(v) for v in re.findall(r"constexpr int kStatus(?!Snapshot)\w+ = (\d+);", src)]
    assert code not in others and code > 3  # (1 .. 3: the rollout kernels' hand-off waits)
    assert len(re.findall(r"\*status = kStatusSnapshot;", engine_asm.function_body(src, "void restore_envs("))) == 2  # header, source index
    for sig in ("static int status_error(sg_env *e, const char *who)", 'extern "C" int sg_check_status(sg_env *e)'):
        body = engine_asm.function_body(src, sig)
        assert re.search(r"if \(st == kStatusSnapshot\)\s*return fail\(", body), sig
    lib = open(build.build(), "rb").read()
    assert b"sg_restore_device: a snapshot of another env id, batch size or configuration" in lib
    assert b"an earlier sg_restore_device was given a snapshot of another env id" in lib


def test_the_new_kernels_build_for_gfx950_without_scratch():
    """build() makes the library with the three entry points; the code object's kernel descriptors of snapshot_kernel and the
    four restore kernels: no scratch, no spill, no LDS, and few enough registers for full occupancy (<= 64 VGPRs: 8 waves per
    SIMD) -- these kernels only move bytes."""
    from space_gym_amd import build
    engine_asm.text()  # (skips without a compiler)
    lib = open(build.build(), "rb").read()
    for name in (b"sg_snapshot_bytes", b"sg_snapshot_device", b"sg_restore_device"):
        assert name in lib
    kernels = engine_asm.descriptors(r"\S*(?:snapshot_kernel|_restore_kernel)\S*")
    assert len(kernels) == 5, [k for k, _ in kernels]  # snapshot_kernel, goal_restore_kernel<2|3|4>, kepler_restore_kernel
    for name, field in kernels:
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == 0, name
        assert field["next_free_vgpr"] <= 64, name
    spills = engine_asm.spill_counts(r"\S*(?:snapshot_kernel|_restore_kernel)\S*")
    assert len(spills) == 5 and all(n == 0 for _, n in spills), spills
    # every instruction of the new kernels that writes memory is a global_store_*: the columns, and the one-lane writes of the
    # header, the status word and the render epoch word alike
    for name, _ in kernels:
        fn = engine_asm.function(name)
        writes = re.findall(r"^\s+(\w*(?:store|atomic)\w*)\s", fn, flags=re.M)  # (instructions are indented, labels are not)
        assert len(writes) >= 4 and all(w.startswith("global_store_") for w in writes), (name, sorted(set(writes)))
        # the 16-byte columns move as 16-byte loads and stores
        assert re.search(r"global_load_dwordx4", fn) and re.search(r"global_store_dwordx4", fn), name
