#!/usr/bin/env python3
"""Measurement: what the return targets with per-group discounts cost (gae_groups_torch / vtrace_torch) next to gae_torch, at
(K, B) = (20, 65 536), (128, 65 536) and (1 000, 65 536), on synthetic rows with ~2 % of the steps done and half of those truncated, dense
terminal values, value and last_value given.  Stream events around back-to-back calls after a warm-up: median, 10th and 90th percentile
over the repetitions, microseconds per call, the host side of each call included.  Every form is one launch, so at the two larger
shapes the figure is the kernel's duration; at K = 20 it is the host side of back-to-back calls.
  * gae_torch                         the existing scalar kernel, the baseline of the same process
  * gae_groups_torch G = 1, 256, B    the table form: one row for all, a population of 256, per-env discounts
  * vtrace_torch with / without ratio table form, G = 256

EXPECTATION, written before the first run (nobody had measured either figure):
  * the table form costs what the scalar form costs: the same 18 B per env-step (reward 4, value 4, done 1, truncated 1 read; advantage
    4, return 4 written) and 8 more bytes per env once per call, 0.4 / K of a step's traffic; G changes which cache line a lane's two
    floats come from, not how many bytes move.  gae_torch's own p10 .. p90 spread is printed beside the ratios.
  * V-trace costs about 22 / 18 = 1.22 x GAE with a ratio (14 B read, 8 B written per env-step) and about 18 / 18 without one, if both
    scans are bound by memory traffic as DESIGN section 14 found the scalar scan to be.
The tool prints the measured ratios beside these and says for each whether it held (--tolerance, default 10 %).
One JSON line per shape.
    python tools/gpu_returns_cost.py profiles/returns_cost.txt"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

SHAPES = ((20, 65536), (128, 65536), (1000, 65536))
GAMMA, LAM = 0.99, 0.95
EXPECTED = {"groups_1": 1.0, "groups_256": 1.0, "groups_B": 1.0, "vtrace_ratio": 22.0 / 18.0, "vtrace_on_policy": 1.0}


def inputs(K, B, seed=0):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)  # noqa: E731
    done = torch.rand((K, B), device=dev, generator=g) < 0.02
    trunc = done & (torch.rand((K, B), device=dev, generator=g) < 0.5)
    return dict(reward=rnd(K, B), value=rnd(K, B), last_value=rnd(B), done=done.to(torch.uint8), trunc=trunc.to(torch.uint8),
                terminal_value=rnd(K, B), ratio=torch.exp(0.5 * rnd(K, B)))


def table(G):
    """G rows near (GAMMA, LAM), all distinct: float32 [G, 2] on the device"""
    k = torch.arange(G, device="cuda", dtype=torch.float32) / max(G, 1)
    return torch.stack([GAMMA - 0.05 * k, LAM - 0.1 * k], 1).contiguous()


def timed(fn, reps, per):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _k in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / per)
    return [round(float(v), 3) for v in (np.median(out), np.percentile(out, 10), np.percentile(out, 90))]


def measure(K, B, tolerance):
    env = sg.make_vec("GoalContinuous3P-v0", B, device=0, seed=0)
    s = inputs(K, B)
    a = (s["reward"], s["done"], s["trunc"])
    kw = dict(last_value=s["last_value"], terminal_value=s["terminal_value"])
    gae_out = dict(advantage=torch.empty_like(s["reward"]), returns=torch.empty_like(s["reward"]))
    vt_out = dict(vs=torch.empty_like(s["reward"]), pg_advantage=torch.empty_like(s["reward"]))
    tables = {"groups_1": table(1), "groups_256": table(256), "groups_B": table(B)}
    fns = {"gae_torch": lambda: env.gae_torch(*a, value=s["value"], gamma=GAMMA, lam=LAM, out=gae_out, **kw)}
    for name, tb in tables.items():
        fns[name] = lambda tb=tb: env.gae_groups_torch(*a, tb, value=s["value"], out=gae_out, **kw)
    fns["vtrace_ratio"] = lambda: env.vtrace_torch(*a, s["value"], ratio=s["ratio"], discounts=tables["groups_256"], out=vt_out, **kw)
    fns["vtrace_on_policy"] = lambda: env.vtrace_torch(*a, s["value"], discounts=tables["groups_256"], out=vt_out, **kw)
    per = max(4, min(200, int(2.0e10 / (18 * K * B) / 10)))
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = dict(K=K, B=B, device=torch.cuda.get_device_name(0), calls_per_timing=per, unit="us per call: median, p10, p90")
    # two rounds over the forms, interleaved, so that a drift of the machine shows as a difference between a form's two figures
    for rnd in (0, 1):
        for name, fn in fns.items():
            res[f"{name}#{rnd}"] = timed(fn, 9, per)
    base = 0.5 * (res["gae_torch#0"][0] + res["gae_torch#1"][0])
    res["gae_torch_spread_p10_p90_over_median"] = [round(res[f"gae_torch#{r}"][k] / base, 3) for r in (0, 1) for k in (1, 2)]
    for name, want in EXPECTED.items():
        got = 0.5 * (res[f"{name}#0"][0] + res[f"{name}#1"][0]) / base
        res[f"{name}_over_gae_torch"] = dict(measured=round(got, 3), expected=round(want, 3), held=bool(abs(got / want - 1.0) <= tolerance))
    env.check_status()
    env.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    tolerance = next((float(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--tolerance=")), 0.10)
    lines = []
    for K, B in SHAPES:
        line = json.dumps(measure(K, B, tolerance))
        print(line, flush=True)
        lines.append(line)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
