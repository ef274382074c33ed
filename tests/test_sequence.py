"""CPU tests of the sequence sampler of the replay ring (sg_replay_sequence_device / replay_sample_sequences_torch): the declarations
and struct layouts, the NumPy model (tests/sequence_model.py) held against the single-transition model (tests/replay_model.py), the
draw, the Python front end with the native call stubbed (nothing reaches a kernel), and the resources of the new kernel in the gfx950
build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import engine_asm
import replay_model
from sequence_model import STREAM_SEQUENCE, draws, sample_sequences, starts, synthetic
from test_episode_stats import _fake_cuda, _stub_env
from test_gae import _struct_fields
from test_snapshot_device import _header_args

B, D, T = 8, 13, 12


# ---------------------------------------------------------------------------------------------- declarations
def test_entry_point_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native
    assert _header_args("sg_replay_sequence_device") == [
        "sg_env *env", "const sg_replay *ring", "const sg_replay_sequence_config *cfg", "int64_t n", "const int64_t *index_in_dev",
        "const sg_replay_sequences *out", "void *hip_stream"]
    assert _header_args("sg_replay_sequence_config_init", "void") == ["sg_replay_sequence_config *cfg"]
    vp = C.c_void_p
    S = _native.SYMBOLS
    assert S["sg_replay_sequence_device"] == (C.c_int, [vp, C.POINTER(_native.SgReplay), C.POINTER(_native.SgReplaySequenceConfig), C.c_int64,
                                                        vp, C.POINTER(_native.SgReplaySequences), vp])
    assert S["sg_replay_sequence_config_init"] == (None, [C.POINTER(_native.SgReplaySequenceConfig)])
    assert "sg_replay_sequence" not in S  # no host-array form: the ring is device memory
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64}
    for name, mirror, size in (("sg_replay_sequence_config", _native.SgReplaySequenceConfig, 24),
                               ("sg_replay_sequences", _native.SgReplaySequences, 120)):
        decls = _struct_fields(name)
        assert len(decls) == len(mirror._fields_), name
        for d, (field, ct) in zip(decls, mirror._fields_):
            m = re.fullmatch(r"(.*?)(\w+)(?:\[(\d+)\])?", d)
            kind, ident, count = m.group(1), m.group(2), m.group(3)
            assert ident == field, (name, d)
            want = C.c_void_p if "*" in kind else ctype[kind.split()[0]]
            assert ct is want or (count and ct._type_ is want and ct._length_ == int(count)), (name, d)
        assert C.sizeof(mirror) == size, name
    assert [f for f, _ in _native.SgReplaySequences._fields_] == ["obs", "action", "reward", "done", "trunc", "terminal_obs", "index",
                                                                 "extra_in", "extra_out"]
    assert [(f, getattr(_native.SgReplaySequenceConfig, f).offset) for f, _ in _native.SgReplaySequenceConfig._fields_] == [
        ("struct_size", 0), ("seed", 8), ("length", 16), ("n_extra", 20)]
    assert (_native.SgReplaySequences.extra_in.offset, _native.SgReplaySequences.extra_out.offset) == (56, 88)


def test_the_kernel_file_is_listed_and_included_and_its_stream_tag_is_its_own():
    from space_gym_amd import build
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_sequence.inc" in build.HEADERS
    assert src.index('#include "sg_replay.inc"') < src.index('#include "sg_sequence.inc"') < src.index('#include "sg_priority.inc"')
    inc = open(os.path.join(build.CSRC, "sg_sequence.inc")).read()
    assert re.search(r"constexpr uint32_t kStreamSequence = 8u;", inc) and STREAM_SEQUENCE == 8
    tags = {}
    for f in sorted(os.listdir(build.CSRC)):
        for name, v in re.findall(r"\bkStream(\w+) = (\d+)u", open(os.path.join(build.CSRC, f)).read()):
            assert tags.setdefault(name, int(v)) == int(v), name
    assert tags["Sequence"] == 8 and tags["Replay"] == replay_model.STREAM_REPLAY and len(tags) >= 9
    assert len(set(tags.values())) == len(tags), tags
    assert sorted(v for k, v in tags.items() if k != "Sequence") == list(range(8))  # 0 .. 7 are taken
    # the kernel is no replay_*_kernel (tests/test_replay.py counts those) and refuses through the ring's status code
    assert re.findall(r"void (\w+_kernel)\(", inc) == ["sequence_sample_kernel"] and "template" not in inc
    assert len(re.findall(r"\*status = kStatusReplay;", engine_asm.function_body(inc, "void sequence_sample_kernel("))) == 2
    body = engine_asm.function_body(src, 'extern "C" int sg_replay_sequence_device(')
    assert body.count("<<<") == 2 and "replay_tick_kernel<<<1, 64, 0, s>>>(r.hdr);" in body
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", body)


# ---------------------------------------------------------------------------------------------- the model
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# (T, B, D, K, laps, dense, L)
MODEL_CASES = [(16, 8, 15, 4, 2.5, False, 5), (16, 8, 17, 4, 0.5, False, 7), (12, 5, 10, 1, 2.5, True, 11), (16, 8, 15, 4, 2.5, False, 1),
               (16, 8, 15, 4, 2.5, False, 15)]


@pytest.mark.parametrize("Tn,Bn,Dn,K,laps,dense,L", MODEL_CASES)
def test_every_step_of_a_sequence_is_the_stored_transition_of_the_existing_model(Tn, Bn, Dn, K, laps, dense, L):
    """for every column and every k, the n_step = 1 transition of replay_model.sample(index = index + k B) is, bit for bit,
    (obs[k], action[k], reward[k], terminal_obs[k] where done else obs[k + 1], done & ~trunc, trunc)"""
    n = 67
    # (C = T B: at this finish rate the default terminal capacity would be too small for the live window)
    ring, _, extra = synthetic(Tn, Bn, Dn, laps=laps, K=K, p_done=0.15, seed=3, dense=dense, C=Tn * Bn)
    assert not ring.status
    v = ring.valid
    assert v == (Tn - 1 if laps > 1 else int(laps * Tn)) and starts(ring, L) == (v - L + 1) * Bn > 0
    rng = np.random.default_rng(11)
    cols = [rng.standard_normal((Tn, Bn)).astype(np.float32) for _ in range(2)]
    out, ok, written = sample_sequences(ring, n, L, seed=3, columns=cols)
    assert ok.all() and ring.sample_calls == 1 and not ring.status
    assert out["obs"].shape == (L + 1, n, Dn) and out["terminal_obs"].shape == (L, n, Dn) and out["reward"].shape == (L, n)
    q, i = out["index"] // Bn, out["index"] % Bn
    assert (q + L <= v).all() and (q >= 0).all()
    first = (ring.head - v) % Tn
    for k in range(L):
        one, ok1 = replay_model.sample(ring, n, n_step=1, index=out["index"] + k * Bn, advance=False)
        assert ok1.all()
        fin = out["done"][k] != 0
        assert np.array_equal(fin, written[k])
        nxt = np.where(fin[:, None], out["terminal_obs"][k], out["obs"][k + 1])
        assert _same(one["obs"], out["obs"][k]) and _same(one["action"], out["action"][k]) and _same(one["reward"], out["reward"][k])
        assert _same(one["next_obs"], nxt), k
        assert np.array_equal(one["terminated"], (fin & (out["trunc"][k] == 0)).astype(np.uint8))
        assert np.array_equal(one["truncated"], out["trunc"][k])
        p = (first + q + k) % Tn
        assert _same(out["terminal_obs"][k][fin], extra["term_dense"][p, i][fin])  # the independent dense copy
        assert not out["terminal_obs"][k][~fin].any()
        for c, got in zip(cols, out["columns"]):
            assert _same(got[k], c[p, i])
    # the data has the boundaries the property is about
    if L > 1:
        inner = (out["done"][:L - 1] != 0).any(0)
        assert inner.mean() >= 0.25, inner.mean()
    if laps > 1:
        slots = (first + q[None, :] + np.arange(-1, L)[:, None]) % Tn  # [L + 1, n]: the row of obs[0], then p_0 .. p_{L-1}
        wraps = (np.diff(slots, axis=0) < 0).any(0)
        assert wraps.sum() >= 1, wraps.sum()


def test_refusals_of_the_model_and_the_call_counter():
    ring, _, _ = synthetic(16, 8, 5, laps=0.5, K=4, p_done=0.15, seed=3, C=128)
    assert ring.valid == 8 and starts(ring, 9) == 0
    assert sample_sequences(ring, 4, 9) == (None, None, None) and ring.status and ring.sample_calls == 1
    ring.status = False
    S = starts(ring, 5)
    assert S == 4 * 8
    index = np.array([0, -1, S, S - 1, 2 ** 40, -2 ** 63], np.int64)
    out, ok, written = sample_sequences(ring, 6, 5, index=index)
    assert ok.tolist() == [True, False, False, True, False, False] and ring.status and ring.sample_calls == 2
    assert not out["obs"][:, ~ok].any() and not written[:, ~ok].any() and out["index"].tolist() == [0, 0, 0, S - 1, 0, 0]
    # the last start's last step is the newest transition
    one, _ = replay_model.sample(ring, 1, index=[len(ring) - 1], advance=False)
    assert _same(one["obs"][0], out["obs"][4, 3]) and _same(one["reward"][0], out["reward"][4, 3])
    # the two samplers share the ring's counter and differ in their stream tag
    a = draws(7, 2, 100, S)
    assert not np.array_equal(a, replay_model.draws(7, 2, 100, S)) and not np.array_equal(a, draws(7, 3, 100, S))


def test_draws_are_uniform_over_the_starts():
    """10^6 draws over S = 1 000 cells: every cell within 5 sigma of n / S (sigma^2 = n p (1 - p)), and the chi-square statistic
    within 5 sigma of its mean (999 degrees of freedom: mean 999, variance 1 998) -- the bounds of tests/test_replay.py"""
    n, cells = 10 ** 6, 1000
    u = draws(seed=12345, call=7, n=n, cells=cells)
    assert u.min() >= 0 and u.max() < cells
    hist = np.bincount(u, minlength=cells)
    p = 1.0 / cells
    assert np.abs(hist - n * p).max() <= 5.0 * np.sqrt(n * p * (1 - p))
    chi2 = ((hist - n * p) ** 2 / (n * p)).sum()
    assert abs(chi2 - (cells - 1)) <= 5.0 * np.sqrt(2.0 * (cells - 1))
    assert not np.array_equal(u, draws(seed=12345, call=8, n=n, cells=cells))  # the call number is part of the counter


# ---------------------------------------------------------------------------------------------- the front end, stubbed
def _env(discrete=False, auto_reset=1):
    from space_gym_amd import _native
    env = _stub_env(B=B, D=D)
    env.discrete = discrete
    env._cfg = _native.SgConfig(auto_reset=auto_reset)
    return env


def _ring(env, steps=T, cap=5, filled=8):
    import torch
    from space_gym_amd.vector_env import ReplayRing
    z = lambda shape, dtype: _fake_cuda(torch.zeros(shape, dtype=dtype))  # noqa: E731
    ring = ReplayRing(steps=steps, num_envs=B, obs_dim=D, term_capacity=cap, discrete=env.discrete, obs=z((steps, B, D), torch.float32),
                      action=z((steps, B), torch.int32) if env.discrete else z((steps, B, 2), torch.float32),
                      reward=z((steps, B), torch.float32), done=z((steps, B), torch.uint8), trunc=z((steps, B), torch.uint8),
                      term_idx=z((steps, B), torch.int32), term_obs=z((cap, D), torch.float32), slot_seq=z((steps,), torch.int32),
                      hdr=z((8,), torch.int32))
    ring.head, ring.filled = filled % steps, filled  # (as after two commits of 4 slots)
    return ring


def _out(n, L, discrete=False, **over):
    import torch
    o = dict(obs=torch.zeros((L + 1, n, D)), action=torch.zeros((L, n), dtype=torch.int32) if discrete else torch.zeros((L, n, 2)),
             reward=torch.zeros((L, n)), done=torch.zeros((L, n), dtype=torch.uint8), trunc=torch.zeros((L, n), dtype=torch.uint8))
    o.update(over)
    return {k: [_fake_cuda(c) for c in v] if isinstance(v, list) else _fake_cuda(v) for k, v in o.items()}


def test_the_call_reaches_the_native_entry_point_with_the_header_structs():
    import torch
    env = _env()
    ring = _ring(env)
    idx = _fake_cuda(torch.zeros(7, dtype=torch.int64))
    cols = [_fake_cuda(torch.zeros((T, B))) for _ in range(2)]
    out = _out(7, 5, columns=[torch.zeros((5, 7)), torch.zeros((5, 7))], index=torch.zeros(7, dtype=torch.int64))
    assert env.replay_sample_sequences_torch(ring, 7, 5, seed=2 ** 63 + 5, index=idx, columns=cols, out=out) is out
    assert env._lib.names() == ["sg_replay_sequence_device"]
    a = env._lib.calls[0][1]
    assert len(a) == 7 and a[3] == 7 and a[4].value == idx.data_ptr()
    r, cfg, seqs = a[1]._obj, a[2]._obj, a[5]._obj
    assert (r.struct_size, r.steps, r.term_capacity) == (88, T, 5) and r.obs == ring.obs.data_ptr() and r.hdr == ring.hdr.data_ptr()
    assert (cfg.struct_size, cfg.seed, cfg.length, cfg.n_extra) == (24, 2 ** 63 + 5, 5, 2)
    for k in ("obs", "action", "reward", "done", "trunc", "index"):
        assert getattr(seqs, k) == out[k].data_ptr(), k
    assert seqs.terminal_obs is None
    assert list(seqs.extra_in) == [cols[0].data_ptr(), cols[1].data_ptr(), None, None]
    assert list(seqs.extra_out) == [out["columns"][0].data_ptr(), out["columns"][1].data_ptr(), None, None]
    # the defaults: seed 0, no index, no columns; a discrete handle takes int32 [L, n] actions; L = the steps the ring holds is allowed
    env = _env(discrete=True)
    ring = _ring(env)
    env.replay_sample_sequences_torch(ring, 3, 8, out=_out(3, 8, discrete=True))
    a = env._lib.calls[-1][1]
    assert (a[2]._obj.seed, a[2]._obj.length, a[2]._obj.n_extra) == (0, 8, 0) and a[4] is None
    assert list(a[5]._obj.extra_in) == [None] * 4 and a[5]._obj.index is None
    with pytest.raises(ValueError, match="action"):
        env.replay_sample_sequences_torch(ring, 3, 8, out=_out(3, 8, discrete=False))
    # a full ring holds T - 1 steps
    full = _ring(_env(), filled=T)
    _env().replay_sample_sequences_torch(full, 2, T - 1, out=_out(2, T - 1))


def _refusals():
    import torch
    z = torch.zeros

    def smp(**kw):
        return lambda env, ring: env.replay_sample_sequences_torch(ring, **{"n": 4, "length": 5, **kw})
    col = lambda: _fake_cuda(z((T, B)))  # noqa: E731
    return {
        "n negative": ("^n: 0", smp(n=-1)), "n large": ("^n: 0", smp(n=2 ** 31)),
        "length zero": ("^length: 1 .. 11 expected", smp(length=0)), "length the slots": ("^length: 1 .. 11 expected", smp(length=T)),
        "length above the fill": ("the ring holds 8 steps", smp(length=9)),
        "rows": (r"\(length \+ 1\) \* n", smp(n=2 ** 29)),
        "seed negative": ("^seed:", smp(seed=-1)), "seed large": ("^seed:", smp(seed=2 ** 64)),
        "index dtype": ("^index", smp(index=_fake_cuda(z(4, dtype=torch.int32)))), "index shape": ("^index", smp(index=_fake_cuda(z(5, dtype=torch.int64)))),
        "index host": ("^index", smp(index=z(4, dtype=torch.int64))),
        "columns five": ("^columns: at most 4", smp(columns=[col() for _ in range(5)])),
        "column shape": (r"^columns\[1\]", smp(columns=[col(), _fake_cuda(z((T, B + 1)))])),
        "column dtype": (r"^columns\[0\]", smp(columns=[_fake_cuda(z((T, B), dtype=torch.float64))])),
        "column host": (r"^columns\[0\]", smp(columns=[z((T, B))])),
        "out obs": (r"^out\['obs'\]", smp(out=_out(4, 5, obs=z((5, 4, D))))),
        "out done": (r"^out\['done'\]", smp(out=_out(4, 5, done=z((5, 4))))),
        "out terminal_obs": (r"^out\['terminal_obs'\]", smp(out=_out(4, 5, terminal_obs=z((6, 4, D))))),
        "out index": (r"^out\['index'\]", smp(out=_out(4, 5, index=z(4, dtype=torch.int32)))),
        "out columns count": (r"^out\['columns'\]: 1 tensors", smp(columns=[col()], out=_out(4, 5, columns=[z((5, 4)), z((5, 4))]))),
        "out columns shape": (r"^out\['columns'\]\[0\]", smp(columns=[col()], out=_out(4, 5, columns=[z((4, 5))]))),
        "ring": ("expected the object", lambda env, ring: env.replay_sample_sequences_torch(dict(obs=ring.obs), 4, 5)),
    }


@pytest.mark.parametrize("bad", sorted(_refusals()))
def test_host_refusals_raise_before_the_native_call(bad):
    env = _env()
    ring = _ring(env)
    match, call = _refusals()[bad]
    with pytest.raises(ValueError, match=match):
        call(env, ring)
    assert env._lib.calls == [] and (ring.head, ring.filled) == (8, 8)


def test_an_empty_ring_and_auto_reset_off_are_refused():
    env = _env()
    with pytest.raises(ValueError, match="the ring holds 0 steps"):
        env.replay_sample_sequences_torch(_ring(env, filled=0), 4, 1)
    off = _env(auto_reset=0)
    with pytest.raises(ValueError, match="auto_reset"):
        off.replay_sample_sequences_torch(_ring(off), 4, 5)
    assert env._lib.calls == [] and off._lib.calls == []


# ---------------------------------------------------------------------------------------------- the build
def test_the_kernel_builds_for_gfx950_without_scratch_lds_or_spills():
    """from the compiler's report: no scratch, no LDS, no spilled register, at most 128 VGPRs (4 waves per SIMD)"""
    kernels = engine_asm.descriptors(r"\S*sequence_\w+_kernel\S*")
    assert len(kernels) == 1, [k for k, _ in kernels]
    for name, field in kernels:
        assert field["private_segment_fixed_size"] == 0, name
        assert field["group_segment_fixed_size"] == 0, name
        assert field["next_free_vgpr"] <= 128, (name, field["next_free_vgpr"])
    for kind in ("vgpr", "sgpr"):
        spills = engine_asm.spill_counts(r"\S*sequence_\w+_kernel\S*", kind)
        assert len(spills) == 1 and all(n == 0 for _, n in spills), (kind, spills)
