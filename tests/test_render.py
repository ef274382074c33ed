"""CPU tests of render(mode="rgb_array") (sg_render): the ctypes mirror of sg_render_config, its defaults, the Python argument
checks that need no handle, and the NumPy model the GPU tests compare against, checked on hand-computed geometry."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import render_model as rm

_CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double}
F = np.float32


def test_sg_render_config_layout_matches_the_header():
    from space_gym_amd import _native
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    body = header[header.index("typedef struct sg_render_config {"):header.index("} sg_render_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct sg_render_config {", "")
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert [(d[-1], _CTYPES[d[0]]) for d in decls] == list(_native.SgRenderConfig._fields_)
    assert C.sizeof(_native.SgRenderConfig) == 24
    for name in ("sg_render_config_init", "sg_set_render", "sg_render_device", "sg_render"):
        assert name in _native.SYMBOLS and re.search(r"\b" + name + r"\(", header), name


def test_sg_render_config_init_defaults():
    from space_gym_amd import _native
    lib = _native.load()
    cfg = _native.SgRenderConfig()
    lib.sg_render_config_init(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_native.SgRenderConfig)
    assert (cfg.capacity, cfg.trace_len, cfg.debug_lidar) == (1, -1, -1)
    assert math.isnan(cfg.trace_decay)


def test_render_keyword_and_metadata():
    from space_gym_amd.vector_env import _ENGINE_KWARGS, SpaceGymVectorEnv
    assert "render" in _ENGINE_KWARGS
    assert SpaceGymVectorEnv.metadata["render.modes"] == ["rgb_array"]


def test_render_config_checks():
    from space_gym_amd.vector_env import render_config
    d = render_config("goal")
    assert d["capacity"] == 16 and d["trace_len"] == -1 and d["debug_lidar"] == -1 and math.isnan(d["trace_decay"])
    assert render_config("kepler", capacity=3, trace_len=0, trace_decay=1.0, debug_lidar=False) == dict(
        capacity=3, trace_len=0, trace_decay=1.0, debug_lidar=0)
    for bad in (dict(capacity=0), dict(capacity=(1 << 20) + 1), dict(trace_len=257), dict(trace_len=-2),
                dict(trace_decay=1.5), dict(trace_decay=-0.1)):
        with pytest.raises(ValueError):
            render_config("goal", **bad)
    with pytest.raises(ValueError, match="no lidar"):
        render_config("kepler", debug_lidar=True)


def test_render_size_and_mode_checks():
    from space_gym_amd.vector_env import SpaceGymVectorEnv, check_render_size
    assert check_render_size(16) == 16 and check_render_size(2048) == 2048
    for bad in (15, 2049, 0):
        with pytest.raises(ValueError):
            check_render_size(bad)
    env = SpaceGymVectorEnv.__new__(SpaceGymVectorEnv)  # no handle: the checks come first
    with pytest.raises(NotImplementedError):
        env.render(mode="human")
    with pytest.raises(ValueError):
        env.render(mode="ansi")
    with pytest.raises(ValueError):
        env.render(size=8)


def _centre_scene(**kw):
    """Goal 3P at 600 px, ship at the world's centre with theta = 0, no trace, no lidar lines, planets off-screen"""
    args = dict(planets=np.full((3, 2), 50.0, np.float32), goal=(F(-0.5), F(-0.5)), lidars=None, thrust=F(0.0),
                torque=F(0.0), trace=(), lidar_on=False, n_planets=3)
    args.update(kw)
    return rm.rasterize(rm.scene(600, "goal", (F(0.0), F(0.0)), (F(1.0), F(0.0)), **args))[::-1, :, 0]  # [j (y up), i]


def test_model_ship_at_the_centre():
    """Ship centre at screen (300, 300): the white body covers the pixel centres well inside radius 15, its outline the pixels
    near radius 15, the engine triangle (edge 25.5 at +-pi/8) the part outside the body, the grey centre pixel (300, 300)."""
    g = _centre_scene()
    assert g[300, 300] == 128  # rint(255 * 0.5), half to even
    j, i = np.mgrid[0:600, 0:600]
    dx, dy = i + 0.5 - 300.0, j + 0.5 - 300.0
    r = np.hypot(dx, dy)
    body = (r < 13.5) & ~((i == 300) & (j == 300))
    assert np.all(g[body] == 255)
    ang = np.arctan2(dy, dx)
    tri = (r > 16.5) & (np.abs(ang) < np.pi / 8 - 0.05) & (dx < 25.5 * np.cos(np.pi / 8) - 1.0)
    assert tri.sum() > 20 and np.all(g[tri] == 0)
    outside = (r > 16.5) & ~((np.abs(ang) < np.pi / 8 + 0.05) & (dx < 26.5)) & (r < 40)
    assert np.all(g[outside] == 255)
    # the outline: every row and column through the disc has black pixels near radius 15 on both sides
    for k in range(290, 311):
        assert (g[k, 280:300] == 0).any() and (g[280:300, k] == 0).any()


def test_model_goal_cross_pixels():
    """The goal at world (-0.5, -0.5) is screen (200, 200): its x is the two diagonals (+-10, +-10) px around it, one pixel per
    column, columns 190 .. 209 (half-open at the right end)."""
    g = _centre_scene()
    region = g[180:221, 180:221] == 0
    expect = np.zeros_like(region)
    for i in range(190, 210):
        expect[i - 180, i - 180] = True          # (190,190) .. (209,209)
        expect[399 - i - 180, i - 180] = True    # (190,209) .. (209,190)
    assert np.array_equal(region, expect)


def test_model_exhaust_blends_with_thrust():
    """thrust 0.5: the exhaust lines at 28.5 .. 33 px are black at alpha 0.5 over white: rint(255 * 0.5) = 128"""
    g = _centre_scene(thrust=F(0.5))
    assert set(np.unique(g[300, 329:333])) == {128}
    assert g[300, 334] == 255 and g[300, 327] == 255
    assert np.all(_centre_scene(thrust=F(0.0))[300, 327:334] == 255)


def test_model_trace_decays():
    """two trace segments: the newest opaque, the one behind it at alpha 0.85 (rint(255 * 0.15) = 38)"""
    tr = [(F(0.0), F(-0.6)), (F(0.3), F(-0.6)), (F(0.6), F(-0.6))]
    g = _centre_scene(trace=tr)
    j = int((-0.6 + 1.5) * 200)  # screen y 180
    assert np.all(g[j, 300:360] == 0) and np.all(g[j, 360:420] == 38)


def test_trace_slots_restart():
    t = rm.TraceSlots(2, 3)
    assert len(t.update(0, 5, 0, (1, 1))) == 1
    assert len(t.update(0, 5, 0, (2, 2))) == 2
    assert len(t.update(0, 5, 0, (3, 3))) == 3
    assert t.update(0, 5, 0, (4, 4))[0] == (4, 4) and len(t.slots[0][2]) == 3  # ring limit
    assert len(t.update(0, 5, 1, (5, 5))) == 1  # new episode
    assert len(t.update(0, 6, 1, (5, 5))) == 1  # new env id
    assert rm.TraceSlots(1, 0).update(0, 1, 0, (0, 0)) == []
