#!/usr/bin/env python3
"""Measurement: what the GAE pass costs (gae_torch / sg_gae_device) at (K, B) = (20, 65 536), (128, 65 536), (1 000, 65 536) and
(32, 1 048 576), on synthetic rows with ~2 % of the steps done and half of those truncated.
  * gae_dense / gae_list / gae_no_terminal: stream events around back-to-back calls after a warm-up -- median, 10th and 90th
    percentile over the repetitions, microseconds per call, the host side of each call included.  The dense form is one launch,
    so at the larger shapes its figure is the scan kernel's duration; `--kernel-trace` gives the kernels' own durations.
  * torch_loop: the same recurrence the way a user writes it without this feature -- the terminal values of the list scattered
    into a dense [K, B] tensor, then a Python loop of K iterations of torch elementwise operations in float64 on the device;
    wall clock around the call, ending in a synchronise.  Its result is compared with gae_torch's (not bitwise: torch's
    a + b * c may contract).
  * traffic: 18 B x K x B (reward 4, value 4, done 1, truncated 1 read; advantage 4, return 4 written) over the dense form's
    time, as a rate and as a share of 8 TB/s; next to it the rate a torch copy_ that moves the same number of bytes (9 K B read +
    9 K B written) reaches in the same run.
One JSON line per shape.
    python tools/gpu_gae_cost.py [out.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_gae_cost.py --kernel-trace"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

SHAPES = ((20, 65536), (128, 65536), (1000, 65536), (32, 1048576))
GAMMA, LAM = 0.99, 0.95
PEAK = 8.0e12


def inputs(K, B, seed=0):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)  # noqa: E731
    done = torch.rand((K, B), device=dev, generator=g) < 0.02
    trunc = done & (torch.rand((K, B), device=dev, generator=g) < 0.5)
    s = dict(reward=rnd(K, B), value=rnd(K, B), last_value=rnd(B), done=done.to(torch.uint8), trunc=trunc.to(torch.uint8))
    # the terminal list of such a rollout: every done step, in no particular order, with the value of its last observation
    se = done.nonzero().to(torch.int32)
    se = se[torch.randperm(se.shape[0], device=dev, generator=g)].contiguous()
    n, cap = int(se.shape[0]), int(se.shape[0]) + 1024
    step_env = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    step_env[:n] = se
    val = rnd(cap)
    s["terminal"] = dict(count=torch.tensor([n], dtype=torch.int32, device=dev), step_env=step_env, value=val)
    dense = torch.zeros((K, B), device=dev)
    dense[se[:, 0].long(), se[:, 1].long()] = val[:n]
    s["terminal_value"] = dense
    return s


def torch_loop(s, gamma=GAMMA, lam=LAM):
    """what a user writes at the parent commit: scatter the list, then the backward loop in float64"""
    reward, value, done, trunc, term = s["reward"], s["value"], s["done"], s["trunc"], s["terminal"]
    K, B = reward.shape
    n = int(term["count"].item())
    se = term["step_env"][:n].long()
    tv = torch.zeros((K, B), dtype=torch.float32, device=reward.device)
    tv[se[:, 0], se[:, 1]] = term["value"][:n]
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    A = torch.zeros(B, dtype=torch.float64, device=reward.device)
    v_next = s["last_value"].double()
    zero = torch.zeros(B, dtype=torch.float64, device=reward.device)
    gl = gamma * lam
    for t in range(K - 1, -1, -1):
        d, v = done[t].bool(), value[t].double()
        nv = torch.where(d, torch.where(trunc[t].bool(), tv[t].double(), zero), v_next)
        delta = reward[t].double() + gamma * nv - v
        A = torch.where(d, delta, delta + gl * A)
        adv[t] = A.float()
        ret[t] = (A + v).float()
        v_next = v
    return adv, ret


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


def calls(env, s, out):
    a = (s["reward"], s["done"], s["trunc"])
    kw = dict(value=s["value"], last_value=s["last_value"], gamma=GAMMA, lam=LAM, out=out)
    return {"gae_dense": lambda: env.gae_torch(*a, terminal_value=s["terminal_value"], **kw),
            "gae_list": lambda: env.gae_torch(*a, terminal=s["terminal"], **kw),
            "gae_no_terminal": lambda: env.gae_torch(*a, **kw)}


def measure(K, B):
    env = sg.make_vec("GoalContinuous3P-v0", B, device=0, seed=0)
    s = inputs(K, B)
    out = dict(advantage=torch.empty_like(s["reward"]), returns=torch.empty_like(s["reward"]))
    fns = calls(env, s, out)
    src = torch.empty(9 * K * B, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    fns["copy_same_bytes"] = lambda: dst.copy_(src)
    per = max(4, min(200, int(2.0e10 / (18 * K * B) / 10)))
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = dict(K=K, B=B, device=torch.cuda.get_device_name(0), done_steps=int(s["terminal"]["count"].item()),
               traffic_bytes=18 * K * B, calls_per_timing=per, unit="us per call: median, p10, p90")
    for k, fn in fns.items():
        res[k] = timed(fn, 9, per)
    # the torch loop: wall clock, a synchronise at both ends; checked against the feature
    want = fns["gae_list"]()
    want = (want[0].clone(), want[1].clone())
    got = torch_loop(s)
    torch.cuda.synchronize()
    res["torch_loop_max_abs_diff"] = float(max((got[0] - want[0]).abs().max().item(), (got[1] - want[1]).abs().max().item()))
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_loop(s)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    res["torch_loop_wall"] = [round(float(v), 1) for v in (np.median(wall), np.min(wall), np.max(wall))]
    feat = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fns["gae_list"]()
        torch.cuda.synchronize()
        feat.append((time.perf_counter() - t0) * 1e6)
    res["gae_list_wall"] = [round(float(v), 1) for v in (np.median(feat), np.min(feat), np.max(feat))]
    res["torch_loop_over_gae_list_wall"] = round(res["torch_loop_wall"][0] / res["gae_list_wall"][0], 1)
    rate = lambda us: 18.0 * K * B / (us * 1e-6)  # noqa: E731
    res["gae_dense_TBps"] = round(rate(res["gae_dense"][0]) / 1e12, 3)
    res["gae_dense_share_of_8TBps"] = round(rate(res["gae_dense"][0]) / PEAK, 3)
    res["copy_TBps"] = round(rate(res["copy_same_bytes"][0]) / 1e12, 3)
    res["gae_dense_over_copy_time"] = round(res["gae_dense"][0] / res["copy_same_bytes"][0], 2)
    env.check_status()
    env.close()
    return res


def kernel_trace_phase():
    for K, B in SHAPES:
        env = sg.make_vec("GoalContinuous3P-v0", B, device=0, seed=0)
        s = inputs(K, B)
        out = dict(advantage=torch.empty_like(s["reward"]), returns=torch.empty_like(s["reward"]))
        fns = calls(env, s, out)
        for name in ("gae_dense", "gae_list"):
            for _ in range(20):
                fns[name]()
        torch.cuda.synchronize()
        print("traced", K, B, flush=True)
        env.close()


def main():
    if "--kernel-trace" in sys.argv:
        return kernel_trace_phase()
    lines = []
    for K, B in SHAPES:
        line = json.dumps(measure(K, B))
        print(line, flush=True)
        lines.append(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
