#!/usr/bin/env python3
"""Measurement: what the Retrace(lambda) / Q(lambda) targets cost (retrace_torch) next to vtrace_torch with a ratio -- the nearest
kernel there was before -- at the same [K, B] = [L, n], and next to the same recurrence as an eager torch loop over L, at
(L, n) = (16, 4 096), (64, 65 536) and (1 000, 65 536), on synthetic rows with ~2 % of the steps done and half of those truncated, dense
terminal values, last_value given.  The env of each shape has num_envs = n, so that vtrace_torch takes the same tensors.  Stream events
around back-to-back calls after a warm-up: median, 10th and 90th percentile over the repetitions, microseconds per call, the host side of
each call included; two interleaved rounds over the forms, the median of a form being the mean of its two rounds' medians.  Every kernel
form is one launch.
  * vtrace_torch, ratio, scalar discounts   the baseline of the same process: 22 B per step-column (reward 4, value 4, ratio 4, done 1,
                                            truncated 1 read; vs 4, pg_advantage 4 written)
  * retrace_torch, ratio                    target only: 22 B (reward, q, value, ratio 4 each, done 1, truncated 1 read; target 4 written)
  * retrace_torch, no ratio (Peng)          target only: 18 B
  * retrace_torch, ratio, loss outputs      34 B (q_online 4 more read; td_error 4 and g 4 more written), weights and huber_delta 1
  * eager torch loop over L                 the recurrence in float64 tensor operations, target only, with a ratio

EXPECTATION, written before the first run (nobody had measured any of these figures):
  * at the two shapes of 65 536 columns the scans are bound by memory traffic, as DESIGN sections 14 and 27 found GAE and V-trace to be,
    so the cost scales with the bytes per step-column relative to V-trace's 22 B: 22 / 22 = 1.00 for the target-only form with a ratio,
    18 / 22 = 0.82 without one, 34 / 22 = 1.55 with the loss outputs.
  * at (16, 4 096) everything is 1.4 MB in 64 waves and each form is one launch: the host side of back-to-back calls decides, and every
    kernel form costs what vtrace_torch costs, 1.00.
  * the eager loop is some 13 tensor operations per step: hundreds of times the kernel at L = 1 000, as section 14 measured for GAE.
The tool prints the measured ratios beside these and says for each whether it HELD or was MISSED (--tolerance, default 10 %), next to
vtrace_torch's own p10 .. p90 spread in the run.  No absolute figure is fixed in advance.  One JSON line per shape.
    python tools/gpu_retrace_cost.py profiles/retrace_cost.txt"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

SHAPES = ((16, 4096), (64, 65536), (1000, 65536))
GAMMA, LAM = 0.99, 0.95
VTRACE_BYTES = 22.0
BYTES = {"retrace_ratio": 22.0, "retrace_peng": 18.0, "retrace_loss": 34.0}
LAUNCH_BOUND = {(16, 4096)}  # expectation 1.00 for every kernel form


def inputs(L, n, seed=0):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)  # noqa: E731
    done = torch.rand((L, n), device=dev, generator=g) < 0.02
    trunc = done & (torch.rand((L, n), device=dev, generator=g) < 0.5)
    return dict(reward=rnd(L, n), q=rnd(L, n), value=rnd(L, n), last_value=rnd(n), done=done.to(torch.uint8), trunc=trunc.to(torch.uint8),
                terminal_value=rnd(L, n), ratio=torch.exp(0.5 * rnd(L, n)), q_online=rnd(L, n), weight=torch.rand(n, device=dev, generator=g))


def eager_loop(s, out, gamma, lam, c_bar):
    """the recurrence of sg_retrace_device as tensor operations, one step of the time axis at a time"""
    f64 = lambda k: s[k].double()  # noqa: E731
    r, q, v, tv, rho = f64("reward"), f64("q"), f64("value"), f64("terminal_value"), f64("ratio")
    done, trunc = s["done"].bool(), s["trunc"].bool()
    carry, v_next = torch.zeros_like(r[0]), s["last_value"].double()
    zero = torch.zeros_like(r[0])
    for t in range(r.shape[0] - 1, -1, -1):
        boot = torch.where(done[t], torch.where(trunc[t], tv[t], zero), v_next + carry)
        G = r[t] + gamma * boot
        out[t] = G.float()
        carry = (lam * torch.clamp(rho[t], max=c_bar)) * (G - q[t])
        v_next = v[t]
    return out


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


def measure(L, n, tolerance):
    env = sg.make_vec("GoalContinuous3P-v0", n, device=0, seed=0)
    s = inputs(L, n)
    a = (s["reward"], s["done"], s["trunc"])
    kw = dict(last_value=s["last_value"], terminal_value=s["terminal_value"], gamma=GAMMA, lam=LAM)
    new = lambda: torch.empty_like(s["reward"])  # noqa: E731
    vt_out, target, eager_out = dict(vs=new(), pg_advantage=new()), new(), new()
    loss = dict(q_online=s["q_online"], weight=s["weight"], huber_delta=1.0, td_error=new(), g=new())
    fns = {"vtrace_torch": lambda: env.vtrace_torch(*a, s["value"], ratio=s["ratio"], out=vt_out, **kw),
           "retrace_ratio": lambda: env.retrace_torch(*a, s["q"], s["value"], ratio=s["ratio"], out=target, **kw),
           "retrace_peng": lambda: env.retrace_torch(*a, s["q"], s["value"], out=target, **kw),
           "retrace_loss": lambda: env.retrace_torch(*a, s["q"], s["value"], ratio=s["ratio"], out=target, loss=loss, **kw)}
    per = max(4, min(200, int(2.0e10 / (22 * L * n) / 10)))
    for fn in fns.values():
        for _ in range(3):
            fn()
    eager = lambda: eager_loop(s, eager_out, GAMMA, LAM, 1.0)  # noqa: E731
    eager()
    torch.cuda.synchronize()
    # the loop is the kernel's recurrence: float32 targets that agree to rounding (torch may fuse or reorder a float64 operation)
    fns["retrace_ratio"]()
    torch.cuda.synchronize()
    worst = float((eager_out - target).abs().max())
    res = dict(L=L, n=n, device=torch.cuda.get_device_name(0), calls_per_timing=per, unit="us per call: median, p10, p90",
               eager_loop_max_abs_difference=worst)
    # two rounds over the forms, interleaved, so that a drift of the machine shows as a difference between a form's two figures
    for rnd in (0, 1):
        for name, fn in fns.items():
            res[f"{name}#{rnd}"] = timed(fn, 9, per)
        res[f"eager_loop#{rnd}"] = timed(eager, 3, 1)
    base = 0.5 * (res["vtrace_torch#0"][0] + res["vtrace_torch#1"][0])
    res["vtrace_torch_spread_p10_p90_over_median"] = [round(res[f"vtrace_torch#{r}"][k] / base, 3) for r in (0, 1) for k in (1, 2)]
    for name, nbytes in BYTES.items():
        want = 1.0 if (L, n) in LAUNCH_BOUND else nbytes / VTRACE_BYTES
        got = 0.5 * (res[f"{name}#0"][0] + res[f"{name}#1"][0]) / base
        res[f"{name}_over_vtrace_torch"] = dict(measured=round(got, 3), expected=round(want, 3),
                                                verdict="HELD" if abs(got / want - 1.0) <= tolerance else "MISSED")
    res["eager_loop_over_retrace_ratio"] = round(0.5 * (res["eager_loop#0"][0] + res["eager_loop#1"][0])
                                                 / (0.5 * (res["retrace_ratio#0"][0] + res["retrace_ratio#1"][0])), 1)
    env.check_status()
    env.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    tolerance = next((float(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--tolerance=")), 0.10)
    lines = []
    for L, n in SHAPES:
        line = json.dumps(measure(L, n, tolerance))
        print(line, flush=True)
        lines.append(line)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
