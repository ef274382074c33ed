"""CPU tests of the running normalization (sg_set_normalize): the ctypes mirror of sg_normalize, the declared entry points and
keywords, the Python argument checks with the native calls stubbed (nothing reaches a kernel), the refusal by the multi-device
front ends, and the NumPy model the GPU tests compare against, checked on a hand-computed example."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from normalize_model import NormalizeModel, RunningMeanStd

_CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}


def test_sg_normalize_layout_matches_the_header():
    from space_gym_amd import _native
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct sg_normalize {"):header.index("} sg_normalize;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct sg_normalize {", "")
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert [(d[-1], _CTYPES[d[0]]) for d in decls] == list(_native.SgNormalize._fields_)
    assert C.sizeof(_native.SgNormalize) == 16 + 4 * 8


def test_normalize_entry_points_and_keywords_are_declared():
    from space_gym_amd import _native
    from space_gym_amd.vector_env import _ENGINE_KWARGS
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name in ("sg_normalize_init", "sg_set_normalize", "sg_get_normalize", "sg_normalize_reserve", "sg_get_normalize_state",
                 "sg_set_normalize_state"):
        assert name in _native.SYMBOLS and re.search(r"\b" + name + r"\(", header), name
    for k in ("normalize_obs", "normalize_reward", "norm_gamma", "norm_epsilon", "clip_obs", "clip_reward"):
        assert k in _ENGINE_KWARGS


class _StubLib:
    """stands in for the native library: records the calls, returns success (sg_get_normalize reports `current`)"""

    def __init__(self, current=None):
        self.calls, self.current = [], current

    def __getattr__(self, name):
        if not name.startswith("sg_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "sg_get_normalize" and self.current is not None:
                C.memmove(args[1], C.byref(self.current), C.sizeof(self.current))
            return b"" if name == "sg_last_error" else 0
        return fn

    def last(self, name):
        return [a for n, a in self.calls if n == name][-1]


def _defaults(on=False):
    from space_gym_amd import _native
    n = _native.SgNormalize(C.sizeof(_native.SgNormalize), int(on), int(on), 1, 0.99, 1e-8, float("inf"), float("inf"))
    return n


def _stub_env(B=8, D=15, current=None):
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    env = SpaceGymVectorEnv.__new__(SpaceGymVectorEnv)
    env._lib = _StubLib(current if current is not None else _defaults())
    env._h = C.c_void_p(1)
    env.num_envs, env.obs_dim, env.device, env.discrete = B, D, 0, False
    env._pending, env._blocks, env._torch_bufs, env._pinned = False, {}, {}, []
    return env


def test_set_normalization_passes_the_configuration():
    env = _stub_env()
    env.set_normalization(obs=True, reward=True, gamma=0.9, epsilon=1e-6, clip_obs=10.0)
    n = env._lib.last("sg_set_normalize")[1]._obj
    assert (n.obs, n.reward, n.update, n.gamma, n.epsilon, n.clip_obs, n.clip_reward) == (1, 1, 1, 0.9, 1e-6, 10.0, float("inf"))
    env._lib.current = _defaults(on=True)
    env._lib.current.clip_obs = 5.0
    env.set_normalization(update=False)  # the rest is kept
    n = env._lib.last("sg_set_normalize")[1]._obj
    assert (n.obs, n.reward, n.update, n.gamma, n.clip_obs) == (1, 1, 0, 0.99, 5.0)
    env.set_normalization(clip_obs=None)  # None: no clipping
    assert env._lib.last("sg_set_normalize")[1]._obj.clip_obs == float("inf")
    assert env.normalization()["clip_obs"] == 5.0 and env.normalization()["clip_reward"] is None


@pytest.mark.parametrize("kw", [dict(gamma=1.5), dict(gamma=-0.1), dict(epsilon=-1.0), dict(epsilon=float("inf")),
                                dict(clip_obs=0.0), dict(clip_reward=-2.0), dict(clip_obs=float("nan"))])
def test_set_normalization_checks_its_arguments(kw):
    env = _stub_env()
    with pytest.raises(ValueError):
        env.set_normalization(obs=True, **kw)
    assert not any(n == "sg_set_normalize" for n, _ in env._lib.calls)


def test_set_normalization_refused_while_a_step_is_in_flight():
    env = _stub_env()
    env._pending = True
    with pytest.raises(RuntimeError):
        env.set_normalization(obs=True)
    assert not any(n == "sg_set_normalize" for n, _ in env._lib.calls)


def test_normalizer_state_shapes_and_checks():
    env = _stub_env(B=8, D=15)
    st = env.normalizer_state()
    assert st["obs_mean"].shape == (15,) and st["returns"].shape == (8,) and st["obs_count"].shape == ()
    assert all(v.dtype == np.float64 for v in st.values())
    with pytest.raises(ValueError):
        env.set_normalizer_state(dict(obs_mean=np.zeros(14)))
    env.set_normalizer_state(dict(ret_var=2.0))  # missing keys: NULL (kept)
    args = env._lib.last("sg_set_normalize_state")
    assert [a is None for a in args[1:]] == [True, True, True, True, False, True, True]


def test_prepare_rollout_reserves_the_scratch(monkeypatch):
    import torch
    from test_episode_stats import _fake_cuda
    env = _stub_env(B=8, D=13)
    K = 6
    args = (_fake_cuda(torch.zeros((K, 8, 2))), _fake_cuda(torch.zeros((K, 8, 13))), _fake_cuda(torch.zeros((K, 8))),
            _fake_cuda(torch.zeros((K, 8), dtype=torch.uint8)), _fake_cuda(torch.zeros((K, 8), dtype=torch.uint8)))
    env.prepare_rollout(*args)
    assert env._lib.last("sg_normalize_reserve")[1] == K


@pytest.mark.parametrize("kw", [dict(normalize_obs=True), dict(normalize_reward=True)])
def test_multi_device_front_ends_refuse_normalization(kw):
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    with pytest.raises(NotImplementedError, match="normaliz"):
        MultiDeviceVectorEnv("GoalContinuous3P-v0", 16, [0, 0], **kw)
    with pytest.raises(NotImplementedError, match="normaliz"):
        ShardedVectorEnv("GoalContinuous3P-v0", 16, **kw)


def test_snapshot_columns_reads_a_version_3_blob():
    """the layout sg_save_state documents for version 3: columns, flags word, episode block, normalization block"""
    from space_gym_amd import _native
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    env = _stub_env(B=4, D=10)
    env.spec, env.env_id, env.n_planets = {"family": "kepler"}, "KeplerCircleOrbit-v0", 0
    B, S = 4, 11
    cols = np.zeros(B * (16 + 16 + 8 + 16), np.uint8)
    norm = bytes(_defaults(on=True))
    state = np.arange(3 * S, dtype=np.float64)
    returns = np.arange(B, dtype=np.float64) + 0.5
    for flags in (2, 3):
        hdr = np.zeros(SpaceGymVectorEnv.SNAPSHOT_HEADER_BYTES, np.uint8)
        hdr[4:8] = np.frombuffer(np.uint32(3).tobytes(), np.uint8)
        eps = (np.full(B, 1.25).tobytes() + np.full(B, 7, np.int32).tobytes()) if flags & 1 else b""
        blob = np.frombuffer(hdr.tobytes() + cols.tobytes() + np.array([flags, 0], np.uint32).tobytes() + eps + norm
                             + state.tobytes() + returns.tobytes(), np.uint8)
        out = env.snapshot_columns(blob)
        assert out["norm_config"].tobytes() == norm and C.sizeof(_native.SgNormalize) == len(norm)
        assert np.array_equal(out["norm_count"], state[2 * S:]) and np.array_equal(out["norm_returns"], returns)
        assert ("ep_len" in out) == bool(flags & 1)
        assert env._snapshot_has_episodes(blob) == bool(flags & 1)


@pytest.mark.parametrize("version,flags", [(1, 0), (2, 1)] + [(3, f) for f in range(8)])
@pytest.mark.parametrize("stub", ["goal4p", "kepler_random"])
def test_snapshot_columns_reads_every_version_and_combination_of_blocks(stub, version, flags):
    """blobs put together by hand, block after block, for every flags word and for versions 1 and 2 (flags 0 and 1 without the
    word); 5 envs, so the int32 lengths leave every later float64 block at an offset that is no multiple of 8"""
    from space_gym_amd import _native
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    B, D, P = 5, {"goal4p": 14, "kepler_random": 7}[stub], 3
    env = _stub_env(B=B, D=D)
    if stub == "goal4p":
        env.spec, env.env_id, env.n_planets = {"family": "goal"}, "GoalContinuous4P-v0", 4
        columns = [("q0", np.float32, 4), ("q1", np.float32, 4), ("ctr", np.uint32, 2), ("aux", np.uint32, 4),
                   ("pl0", np.float32, 4), ("pl1", np.float32, 4), ("cshift", np.float32, 4)]
    else:
        env.spec, env.env_id, env.n_planets = {"family": "kepler"}, "KeplerRandomOrbits-v0", 0
        columns = [("q0", np.float32, 4), ("q1", np.float32, 4), ("ctr", np.uint32, 2), ("aux", np.uint32, 4), ("orbd", np.float64, 2)]
    rng = np.random.default_rng(version * 8 + flags)

    def block(dtype, shape):
        raw = rng.integers(0, 256, int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=np.uint8)
        return raw.view(dtype).reshape(shape)

    expect = {name: block(dt, (B, w)) for name, dt, w in columns}
    if version == 3:
        expect["flags"] = np.array([[flags, 0]], np.uint32)
    if flags & 1:
        expect.update(ep_ret=block(np.float64, (B, 1)), ep_len=block(np.int32, (B, 1)))
    if flags & 2:
        expect.update(norm_config=block(np.uint8, (C.sizeof(_native.SgNormalize),)), norm_mean=block(np.float64, (D + 1,)),
                      norm_var=block(np.float64, (D + 1,)), norm_count=block(np.float64, (D + 1,)), norm_returns=block(np.float64, (B,)))
    if flags & 4:
        expect.update(profile_count=np.array([P, 0], np.uint32), profiles=block(np.uint8, (P * C.sizeof(_native.SgRewardProfile),)),
                      profile_index=block(np.uint8, (B,)))
    hdr = np.zeros(SpaceGymVectorEnv.SNAPSHOT_HEADER_BYTES, np.uint8)
    hdr[4:8] = np.frombuffer(np.uint32(version).tobytes(), np.uint8)
    blob = np.frombuffer(hdr.tobytes() + b"".join(v.tobytes() for v in expect.values()), np.uint8)
    out = env.snapshot_columns(blob)
    assert list(out) == list(expect)
    for name, want in expect.items():
        assert out[name].dtype == want.dtype and out[name].shape == want.shape, name
        assert out[name].tobytes() == want.tobytes(), name
    assert env._snapshot_version(blob) == version and env._snapshot_flags(blob) == flags
    assert env._snapshot_has_episodes(blob) == bool(flags & 1)
    with pytest.raises(AssertionError):  # the blocks must add up to the blob
        env.snapshot_columns(np.concatenate([blob, np.zeros(1, np.uint8)]))


def _pooled(batches, ddof_prior=True):
    """RunningMeanStd after updates with `batches` is the pooled mean / variance of the prior (count 1e-4 at mean 0, var 1)
    and every value seen -- exactly, in rational arithmetic"""
    c0 = Fraction(1, 10000)
    xs = [Fraction(float(v)) for b in batches for v in b]
    tot = c0 + len(xs)
    mean = sum(xs) / tot
    m2 = c0 * (1 + mean * mean) + sum((x - mean) ** 2 for x in xs)
    return mean, m2 / tot, tot


def test_running_mean_std_is_the_pooled_moments():
    rms = RunningMeanStd(())
    b1, b2 = np.array([1.0, 3.0]), np.array([-2.0, 0.5, 4.0])
    rms.update(b1)
    rms.update(b2)
    mean, var, count = _pooled([b1, b2])
    assert rms.count == pytest.approx(float(count), rel=0, abs=0)
    assert rms.mean == pytest.approx(float(mean), rel=1e-14) and rms.var == pytest.approx(float(var), rel=1e-14)


def test_model_two_steps_by_hand():
    """B = 2, D = 1: obs [1, 3] then [5, -1]; rewards [1, 2] then [3, 4]; env 1 done at step 0.  returns: [1, 2] -> reset of
    env 1 -> [0.99 + 3, 0 + 4] = [3.99, 4]; each normalized value is the raw one over (and, observations, minus) the pooled
    statistics of everything seen up to and including its step"""
    m = NormalizeModel(2, 1, gamma=0.99, epsilon=1e-8)
    o0, r0, _ = m.step(np.array([[1.0], [3.0]], np.float32), np.array([1.0, 2.0], np.float32), np.array([0, 1]))
    mean, var, _ = _pooled([[1.0, 3.0]])
    assert np.allclose(o0[:, 0], (np.array([1.0, 3.0]) - float(mean)) / np.sqrt(float(var) + 1e-8), rtol=1e-6)
    rmean, rvar, _ = _pooled([[1.0, 2.0]])
    assert np.allclose(r0, np.array([1.0, 2.0]) / np.sqrt(float(rvar) + 1e-8), rtol=1e-6)
    assert m.returns.tolist() == [1.0, 0.0]
    o1, r1, t1 = m.step(np.array([[5.0], [-1.0]], np.float32), np.array([3.0, 4.0], np.float32), np.array([0, 0]),
                        terminal_obs=np.array([[2.0], [2.0]], np.float32))
    mean, var, count = _pooled([[1.0, 3.0], [5.0, -1.0]])
    assert m.obs_rms.count == float(count) == 4.0001
    assert m.obs_rms.mean[0] == pytest.approx(float(mean), rel=1e-14) and m.obs_rms.var[0] == pytest.approx(float(var), rel=1e-14)
    scale = np.sqrt(float(var) + 1e-8)
    assert np.allclose(o1[:, 0], (np.array([5.0, -1.0]) - float(mean)) / scale, rtol=1e-6)
    assert np.allclose(t1[:, 0], (2.0 - float(mean)) / scale, rtol=1e-6)  # this step's statistics, not an update
    assert m.returns.tolist() == [1.0 * 0.99 + 3.0, 4.0]
    rmean, rvar, _ = _pooled([[1.0, 2.0], [3.99, 4.0]])
    assert m.ret_rms.var == pytest.approx(float(rvar), rel=1e-12)
    assert np.allclose(r1, np.array([3.0, 4.0]) / np.sqrt(float(rvar) + 1e-8), rtol=1e-6)
    assert o1.dtype == np.float32 and r1.dtype == np.float32


def test_model_clips_and_freezes():
    m = NormalizeModel(3, 2, clip_obs=0.5, clip_reward=0.25)
    o, r, _ = m.step(np.array([[0, 10], [1, -10], [2, 0]], np.float32), np.array([100, -100, 0], np.float32), np.zeros(3))
    assert np.abs(o).max() == np.float32(0.5) and np.abs(r).max() == np.float32(0.25)
    m.update = False
    before = (m.obs_rms.mean.copy(), m.obs_rms.count, m.returns.copy())
    m.step(np.ones((3, 2), np.float32), np.ones(3, np.float32), np.ones(3))
    assert np.array_equal(before[0], m.obs_rms.mean) and before[1] == m.obs_rms.count and np.array_equal(before[2], m.returns)
