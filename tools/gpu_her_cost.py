#!/usr/bin/env python3
"""Measurement: what hindsight goal relabelling of a replay batch costs (replay_relabel_torch), on a full ring of T = 256 slots of
B = 65 536 envs (GoalContinuous3P-v0, D = 15) filled with random rows, ~2 % of the steps done, at n = 4 096 and 65 536 rows and horizons
H = 8 and 64, her_ratio 0.8, strategy "future".  Every form works on the same batch, gathered once from the same `index`:
  * relabel   replay_relabel_torch(ring, batch, out=): one launch
  * eager     the same relabelling composed in eager torch with no host synchronisation: the mask and the offset's uniform number from
              torch.rand, the strided gather of the window's done bytes [H - 1, n] and the first one set, the terminal join through
              term_idx, the goal columns in float32 and the reward's delta in float64, written back with torch.where.  Checked once
              per shape against the call: handed the call's own mask and offsets, it gives the call's obs, next_obs and reward
              (`bit_equal_to_eager`; `max_abs_reward_diff` otherwise), and the windows it finds hold every offset the call chose
  * copy      one copy_ of as many bytes as the call writes (per relabelled row four goal floats, the reward, the offset and the
              goal position; per row the flag): the floor for the write side alone
  * sample    the replay_sample_torch(index=) call that made the batch: what the relabel is added to
Stream events around back-to-back calls after a warm-up; the forms alternate window by window within one run; median, 10th and 90th
percentile over the windows, microseconds per call, host side included.  No figure was fixed in advance; the tool prints whether the
call is under the eager composition at each shape.  One JSON line per shape.
    python tools/gpu_her_cost.py profiles/her_cost.txt"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

T, B, K = 256, 65536, 64
ENV_ID = "GoalContinuous3P-v0"
SHAPES = ((4096, 8), (4096, 64), (65536, 8), (65536, 64))
RATIO = 0.8
GOAL_SCALE, SPARSE, GOAL_R2, TWO_OVER_WORLD, HALF_WORLD = 500.0, 5.0, 0.1607142857142857 ** 2, 2.0 / 3.0, 1.5


def fill(env, seed=0):
    """a full ring: T / K commits of K slots of random rows (positions inside the world), ~2 % done, list-form terminal records"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    D = env.obs_dim
    ring = env.replay_torch(T)
    rows_of = lambda *lead: torch.rand((*lead, D), device=dev, generator=g) * 3.0 - 1.5  # noqa: E731
    env.replay_begin_torch(ring, rows_of(B))
    for _ in range(T // K + 1):  # one commit more than a lap: the ring has wrapped
        rows = ring.rows(K)
        rows["obs"].copy_(rows_of(K, B))
        rows["action"].copy_(torch.rand((K, B, 2), device=dev, generator=g) * 2 - 1)
        rows["reward"].copy_(torch.randn((K, B), device=dev, generator=g))
        done = torch.rand((K, B), device=dev, generator=g) < 0.02
        rows["done"].copy_(done.to(torch.uint8))
        rows["trunc"].copy_((done & (torch.rand((K, B), device=dev, generator=g) < 0.5)).to(torch.uint8))
        se = done.nonzero().to(torch.int32).contiguous()
        term = dict(count=torch.tensor([se.shape[0]], dtype=torch.int32, device=dev), step_env=se, obs=rows_of(se.shape[0]))
        env.replay_commit_torch(ring, K, terminal=term)
    env.check_status()
    return ring


def eager(ring, batch, H, u_mask, u_off, mask=None, ks=None):
    """the relabelling in eager torch; returns (obs, next_obs, reward, mask, ks, m).  mask / ks given: used instead of the draws"""
    Bn, C, Tn = ring.num_envs, ring.term_capacity, ring.steps
    index = batch["index"]
    v = min(ring.filled, Tn - 1)
    q, i = index // Bn, index % Bn
    first = (ring.head - v) % Tn
    if mask is None:
        mask = (u_mask < RATIO) & (batch["steps"] == 1)
    m = torch.clamp(v - 1 - q, max=H - 1)
    if H > 1:
        k = torch.arange(H - 1, device=index.device)[:, None]
        dn = ring.done[(first + q[None, :] + k) % Tn, i[None, :].expand(H - 1, -1)] != 0  # [H - 1, n]: the strided scan
        dn = dn & (k < m[None, :])
        m = torch.where(dn.any(0), dn.to(torch.uint8).argmax(0), m)
    if ks is None:
        ks = torch.clamp((u_off * (m + 1).to(torch.float32)).to(torch.int64), max=m)
    p = (first + q + ks) % Tn
    fin = ring.done[p, i] != 0
    rec = (ring.term_idx[p, i].to(torch.int64) & 0xFFFFFFFF) % C
    a = torch.where(fin[:, None], ring.term_obs[rec, :2], ring.obs[p, i, :2])
    obs, nxt = batch["obs"], batch["next_obs"]
    x0, x1 = obs[:, :2], nxt[:, :2]
    tow = torch.tensor(TWO_OVER_WORLD, dtype=torch.float32, device=index.device)
    g0, g1 = (a - x0) * tow, (a - x1) * tow
    x0d, x1d, ad = x0.double(), x1.double(), a.double()
    vo1 = nxt[:, -2:].double() * HALF_WORLD
    vo0 = vo1 + (x1d - x0d)
    vn0, vn1 = ad - x0d, ad - x1d

    def term(va, vb):
        b2 = vb[:, 0] * vb[:, 0] + vb[:, 1] * vb[:, 1]
        la = torch.sqrt(va[:, 0] * va[:, 0] + va[:, 1] * va[:, 1])
        return GOAL_SCALE * (la - torch.sqrt(b2)) + torch.where(b2 < GOAL_R2, SPARSE, 0.0)
    r = ((batch["reward"].double() - term(vo0, vo1)) + term(vn0, vn1)).float()
    new_obs = torch.cat([obs[:, :-2], torch.where(mask[:, None], g0, obs[:, -2:])], 1)
    new_nxt = torch.cat([nxt[:, :-2], torch.where(mask[:, None], g1, nxt[:, -2:])], 1)
    return new_obs, new_nxt, torch.where(mask, r, batch["reward"]), mask, ks, m


def timed(fns, windows, per):
    """the forms alternate window by window; {name: [median, p10, p90]} in microseconds per call"""
    got = {k: [] for k in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _k in range(per[name]):
                fn()
            b.record()
            torch.cuda.synchronize()
            got[name].append(a.elapsed_time(b) * 1000.0 / per[name])
    return {k: [round(float(x), 2) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))] for k, v in got.items()}


def measure(env, ring, n, H):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n + H)
    index = torch.randint(0, len(ring), (n,), device=dev, generator=g)
    u_mask, u_off = torch.rand(n, device=dev, generator=g), torch.rand(n, device=dev, generator=g)
    fresh = env.replay_sample_torch(ring, n, index=index)
    work = {k: v.clone() for k, v in fresh.items()}
    env.replay_relabel_torch(ring, work, her_ratio=RATIO, horizon=H, seed=7)
    mask, ks = work["relabelled"] == 1, work["offset"].to(torch.int64)
    want = eager(ring, fresh, H, u_mask, u_off, mask=mask, ks=ks)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    same = all(torch.equal(bits(a), bits(b)) for a, b in zip(want[:3], (work["obs"], work["next_obs"], work["reward"])))
    diff = float((want[2].double() - work["reward"].double()).abs().max())
    inside = bool((ks <= want[5]).all())
    share = float(mask.float().mean())
    written = int(share * n) * (16 + 4 + 4 + 8) + n
    src, dst = torch.empty(written, dtype=torch.uint8, device=dev), torch.empty(written, dtype=torch.uint8, device=dev)
    out = {k: work[k] for k in ("relabelled", "offset", "goal")}
    fns = {"relabel": lambda: env.replay_relabel_torch(ring, work, her_ratio=RATIO, horizon=H, seed=7, out=out),
           "eager": lambda: eager(ring, fresh, H, u_mask, u_off), "copy": lambda: dst.copy_(src),
           "sample": lambda: env.replay_sample_torch(ring, n, index=index, out=fresh)}
    per = {"relabel": 100, "eager": 10, "copy": 100, "sample": 100}
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = dict(env_id=ENV_ID, n=n, H=H, her_ratio=RATIO, relabelled_share=round(share, 4), bytes_written=written,
               device=torch.cuda.get_device_name(0), calls_per_window=per, unit="us per call: median, p10, p90",
               bit_equal_to_eager=bool(same), max_abs_reward_diff=diff, offsets_inside_eager_windows=inside)
    res.update(timed(fns, 9, per))
    rel = res["relabel"][0]
    res["summary"] = {"under_eager": bool(rel < res["eager"][0]), "eager_over_relabel": round(res["eager"][0] / rel, 2),
                      "relabel_over_copy": round(rel / res["copy"][0], 2), "relabel_over_sample": round(rel / res["sample"][0], 2)}
    env.check_status()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    env = sg.make_vec(ENV_ID, B, device=0, seed=0)
    ring = fill(env)
    lines = []
    for n, H in SHAPES:
        line = json.dumps(measure(env, ring, n, H))
        print(line, flush=True)
        lines.append(line)
    env.close()
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
