"""NumPy model of the engine's renderer (sg_render / sg_render_device): the scene of the reference's Renderer
(gym_space/rendering.py:15-182) with the rules of DESIGN section 11 -- float32 geometry rounded op by op as the kernel rounds it,
vertices snapped to a 1/16 px grid, coverage decided in integer arithmetic, source-alpha blending in float32.  Frames from it are
compared bit for bit with the device's.  cos / sin come from the engine's sincos_acc through the host twin (tests/host_twin)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_twin"))

F = np.float32
FIX = 16
CLAMP = F(65536.0)
STEP30 = F(2 * np.pi / 30)
PI8, PI16 = F(np.pi / 8), F(np.pi / 16)
ARC_SEGS = 20
LINE, POLY, POINT = 0, 1, 2
INK = {"black": F(0.0), "white": F(1.0), "grey": F(0.5)}


def sincos(a):
    """sincos_acc of float32 angles (the observation's own cos / sin)"""
    from pytwin import sincos as twin_sincos
    s, c = twin_sincos(2, np.atleast_1d(np.asarray(a, np.float32)))
    return s, c


_UNIT30 = None


def unit30():
    """gym make_circle's 30 unit vectors: vertex k at angle 2 pi k / 30, (cos, sin) by sincos_acc"""
    global _UNIT30
    if _UNIT30 is None:
        s, c = sincos(np.arange(30, dtype=np.float32) * STEP30)
        _UNIT30 = [(F(c[k]), F(s[k])) for k in range(30)]
    return _UNIT30


def goal_planet_radius(n_planets):
    """HexagonalTiling.planets_radius (hexagonal_tiling.py:37,45-48) as the engine fills it in (float32 of the float64 value)"""
    s3 = math.sqrt(3.0)
    min_tiles = n_planets + 2 if n_planets == 2 else math.ceil((n_planets + 2) / 0.6)
    r = math.ceil(math.sqrt(72.0 * s3 * min_tiles - 6.0 * s3 + 12.0) / 12.0 - 0.25 + s3 / 12.0)
    while True:
        c = math.floor(2.0 * s3 * r / 3.0 - 1.0 / 3.0 + s3 / 3.0)
        if r * c >= min_tiles:
            break
        r += 1
    a = 2.0 * s3 * 3.0 / (3.0 * (2.0 * r + 1.0))
    return F(0.75 * (a * s3) / 2)


def translate_action(discrete, action):
    """(thrust, torque) the step uses (spaceship_env.py:189-202,210-214), after the device's clamp; None: (0, 0)"""
    if action is None:
        return F(0.0), F(0.0)
    if discrete:
        k = int(action)
        a0 = F(1.0) if k in (1, 4, 5) else F(-1.0)
        a1 = F(-1.0) if k in (2, 4) else F(1.0) if k in (3, 5) else F(0.0)
    else:
        a0 = np.fmin(np.fmax(F(action[0]), F(-1.0)), F(1.0))
        a1 = np.fmin(np.fmax(F(action[1]), F(-1.0)), F(1.0))
    return (a0 + F(1.0)) * F(0.5), a1


def snap(v):
    return int(np.rint(np.fmin(np.fmax(F(v), -CLAMP), CLAMP) * F(FIX)))


class Prims:
    """a frame's primitive list, in draw order, as the setup kernel writes it"""

    def __init__(self, size):
        self.size, self.items = size, []

    def _box(self, x0, y0, x1, y1):
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, self.size - 1), min(y1, self.size - 1)
        return None if x0 > x1 or y0 > y1 else (x0, y0, x1, y1)

    def line(self, fax, fay, fbx, fby, ink="black", alpha=F(1.0)):
        ax, ay, bx, by = snap(fax), snap(fay), snap(fbx), snap(fby)
        ymajor = abs(by - ay) > abs(bx - ax)
        if (ay == by) if ymajor else (ax == bx):
            return
        if (ay > by) if ymajor else (ax > bx):
            ax, ay, bx, by = bx, by, ax, ay
        box = self._box((min(ax, bx) >> 4) - 1, (min(ay, by) >> 4) - 1, (max(ax, bx) >> 4) + 1, (max(ay, by) >> 4) + 1)
        if box:
            self.items.append((LINE, (ax, ay, bx, by, ymajor), box, ink, F(alpha)))

    def point(self, fx, fy, ink):
        x, y = snap(fx), snap(fy)
        box = self._box(x >> 4, y >> 4, x >> 4, y >> 4)
        if box:
            self.items.append((POINT, (x, y), box, ink, F(1.0)))

    def poly(self, fx, fy, ink):
        x, y = [snap(v) for v in fx], [snap(v) for v in fy]
        k = len(x)
        area = sum(x[v] * y[(v + 1) % k] - x[(v + 1) % k] * y[v] for v in range(k))
        if area == 0:
            return
        box = self._box((min(x) >> 4) - 1, (min(y) >> 4) - 1, (max(x) >> 4) + 1, (max(y) >> 4) + 1)
        if not box:
            return
        verts = list(zip(x, y)) if area > 0 else list(zip(x, y))[::-1]
        self.items.append((POLY, verts, box, ink, F(1.0)))


def coverage(kind, geo, cx, cy):
    """the pixel centres (cx, cy) (int64 arrays, 1/16 px) the primitive covers"""
    if kind == LINE:
        ax, ay, bx, by, ymajor = geo
        u, v = (cy, cx) if ymajor else (cx, cy)
        if ymajor:
            ax, ay, bx, by = ay, ax, by, bx
        dx = bx - ax
        t = (u - ax) * (by - ay)
        lo = (v - FIX // 2 - ay) * dx
        return (u >= ax) & (u < bx) & (lo <= t) & (t < lo + FIX * dx)
    if kind == POINT:
        return ((cx >> 4) == (geo[0] >> 4)) & ((cy >> 4) == (geo[1] >> 4))
    inside = np.ones(cx.shape, bool)
    k = len(geo)
    for j in range(k):
        (ax, ay), (bx, by) = geo[j - 1], geo[j]
        dx, dy = bx - ax, by - ay
        e = dx * (cy - ay) - dy * (cx - ax)
        tie = (dx == 0 and dy == 0) or dy < 0 or (dy == 0 and dx < 0)
        inside &= (e > 0) | ((e == 0) & tie)
    return inside


def rasterize(prims):
    """uint8 [size, size, 3], row 0 the top"""
    size = prims.size
    img = np.ones((size, size), np.float32)  # [j (y up), i]
    for kind, geo, (x0, y0, x1, y1), ink, a in prims.items:
        j, i = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
        m = coverage(kind, geo, FIX * i + FIX // 2, FIX * j + FIX // 2)
        sub = img[y0:y1 + 1, x0:x1 + 1]
        sub[m] = INK[ink] * a + sub[m] * (F(1.0) - a)
    g = np.rint(img * F(255.0)).astype(np.uint8)[::-1]
    return np.repeat(g[:, :, None], 3, axis=2)


def scene(size, family, ship, cs, planets=None, goal=None, lidars=None, thrust=F(0.0), torque=F(0.0), trace=(), decay=0.85,
          lidar_on=False, n_planets=0):
    """The frame's primitives (the setup kernel's draw order).
    ship: float32 (x, y); cs: float32 (cos, sin) of the heading (obs[2:4]); planets: float32 [N, 2] (Goal); goal: float32 (x, y);
    lidars: float32 [N + 1, 2], the goal's then the planets' lidar vectors (as goal_observe forms them); trace: float32 world positions,
    newest first (the current position included)."""
    hw = F(1.5) if family == "goal" else F(3.0)
    ws = F(size) / (hw + hw)
    ps = F(size) / F(600.0)
    P = Prims(size)
    scr = lambda w: (F(w) + hw) * ws  # noqa: E731  Renderer._world_to_screen
    tx, ty = scr(ship[0]), scr(ship[1])
    c, s = F(cs[0]), F(cs[1])

    def ship_frame(vx, vy):
        return tx + (c * vx - s * vy), ty + (s * vx + c * vy)

    U = unit30()
    # 1. planets
    if family == "goal":
        pr = goal_planet_radius(n_planets)
        circles = [(scr(p[0]), scr(p[1]), pr * ws) for p in planets]
    else:
        circles = [(scr(0.0), scr(0.0), F(0.2) * ws), (scr(0.0), scr(0.0), F(3.0) * ws)]
    for cx, cy, r in circles:
        pts = [(cx + r * U[v % 30][0], cy + r * U[v % 30][1]) for v in range(31)]
        for v in range(30):
            P.line(*pts[v], *pts[v + 1])
    # 2. engine
    e = F(25.5) * ps
    sm, cm = sincos([-PI8, PI8])
    tri = [ship_frame(F(0.0), F(0.0)), ship_frame(e * F(cm[0]), e * F(sm[0])), ship_frame(e * F(cm[1]), e * F(sm[1]))]
    P.poly([p[0] for p in tri], [p[1] for p in tri], "black")
    # 3. exhaust
    if thrust > 0:
        r0, r1 = F(28.5) * ps, F(33.0) * ps
        sa, ca = sincos([F(-1.0) * PI16, F(0.0) * PI16, F(1.0) * PI16])
        for a in range(3):
            ux, uy = F(ca[a]), F(sa[a])
            P.line(*ship_frame(r0 * ux, r0 * uy), *ship_frame(r1 * ux, r1 * uy), "black", thrust)
    # 4. / 5. body and outline
    rb = F(15.0) * ps
    body = [ship_frame(rb * U[v][0], rb * U[v][1]) for v in range(30)]
    P.poly([p[0] for p in body], [p[1] for p in body], "white")
    for v in range(30):
        P.line(*body[v], *body[(v + 1) % 30])
    # 6. centre
    P.point(tx, ty, "grey")
    # 7. goal
    if family == "goal":
        gx, gy, d = scr(goal[0]), scr(goal[1]), F(10.0) * ps
        P.line(gx - d, gy - d, gx + d, gy + d)
        P.line(gx - d, gy + d, gx + d, gy - d)
    # 8. torque indicator (stand-in for assets/torque_img.png)
    if torque != 0:
        s4, c4 = sincos([F(4.0)])
        s4, c4 = F(s4[0]), F(c4[0])
        r, sx, sy = F(8.0) * ps, -F(torque), np.abs(F(torque))
        pts = []
        for v in range(ARC_SEGS + 1):
            ix, iy = sx * (r * U[v][0]), sy * (r * U[v][1])
            pts.append(ship_frame(c4 * ix - s4 * iy, s4 * ix + c4 * iy))
        for v in range(ARC_SEGS):
            P.line(*pts[v], *pts[v + 1])
    # 9. trace
    alpha = F(1.0)
    for i in range(1, len(trace)):
        p, q = trace[i - 1], trace[i]
        P.line(scr(p[0]), scr(p[1]), scr(q[0]), scr(q[1]), "black", alpha)
        alpha = alpha * F(decay)
    # 10. lidar lines
    if family == "goal" and lidar_on:
        for lv in lidars:
            P.line(tx, ty, scr(F(ship[0]) + F(lv[0])), scr(F(ship[1]) + F(lv[1])))
    return P


class TraceSlots:
    """The trace slots of a handle: slot k of a call belongs to env_ids[k]; `key` names the env's episode (and the handle's
    resets): a slot whose env or key changed since its previous call starts empty."""

    def __init__(self, capacity, trace_len):
        self.slots, self.trace_len = [None] * capacity, trace_len

    def update(self, k, env, key, pos):
        s = self.slots[k]
        if s is None or s[0] != env or s[1] != key:
            s = [env, key, []]
        if self.trace_len > 0:
            s[2] = [tuple(F(v) for v in pos)] + s[2][:self.trace_len - 1]
        self.slots[k] = s
        return list(s[2])


def render_env(size, spec, obs_row, planets, goal, action, trace, trace_decay, lidar_on, discrete):
    """one frame from an env's observation row (ship position, cos / sin, lidar vectors), its planets and goal, the last
    action and the trace positions (newest first).  spec: {"family", "n_planets"}."""
    thrust, torque = translate_action(discrete, action)
    fam, N = spec["family"], spec.get("n_planets") or 0
    lidars = None
    if fam == "goal":
        # the planets' lidar vectors are the observation's; the goal's is formed as goal_observe forms it, from the goal in the
        # state: after a goal hit the step's observation still points at the old goal (goal.py:154-157 resamples after
        # _make_observation), and the device draws from the state
        o = np.asarray(obs_row, np.float32)
        two_over_world = F(2.0 / 3.0)
        lg = np.array([(F(goal[0]) - o[0]) * two_over_world, (F(goal[1]) - o[1]) * two_over_world], np.float32)
        lidars = [lg] + [o[7 + 2 * j:9 + 2 * j] for j in range(N)]
    P = scene(size, fam, obs_row[:2], obs_row[2:4], planets, goal, lidars, thrust, torque, trace, trace_decay, lidar_on, N)
    return rasterize(P)
