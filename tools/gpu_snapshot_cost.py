#!/usr/bin/env python3
"""Measurement: what a device snapshot and a restore cost (snapshot_torch / restore_torch, sg_snapshot_device /
sg_restore_device).  GoalContinuous3P-v0 and KeplerCircleOrbit-v0 at 65 536 and 1 048 576 envs: the snapshot; the restore with
no mask (with and without the observation rows), with a 10 % mask and with a permutation `src`; in the same run a
hipMemcpyAsync device-to-device copy of sg_snapshot_bytes and the launch of a one-element fill kernel as yardsticks; and the
host round trip save_state() + load_state(), the only way back to an earlier state without this feature.  Stream events around
back-to-back calls after a warm-up: median, 10th and 90th percentile over the repetitions, microseconds per call.  One JSON line
per (id, batch).  --kernel-trace only issues, per id at 1 048 576 envs, 100 snapshots, 100 identity restores without obs and
100 copies, to be run under `rocprofv3 --kernel-trace --stats` for the kernels' own durations.
    python tools/gpu_snapshot_cost.py [out.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_snapshot_cost.py --kernel-trace"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

_hip = C.CDLL("libamdhip64.so")
_hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
_hip.hipMemcpyAsync.restype = C.c_int
D2D = 3  # hipMemcpyDeviceToDevice


def timed(fn, reps, per):
    """`reps` timings of `per` back-to-back calls of fn(): (median, p10, p90) in microseconds per call"""
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


def setup(env_id, B):
    dev = torch.device("cuda", 0)
    env = sg.make_vec(env_id, B, device=0, seed=0)
    env.reset_torch()
    acts = env.random_actions_torch(8, seed=1)
    for t in range(40):
        env.step_torch(acts[t % 8])
    snap = env.snapshot_torch()
    for t in range(8):
        env.step_torch(acts[t])
    return dev, env, snap


def restore_no_obs(env, snap):
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    buf, n = C.c_void_p(snap.buffer.data_ptr()), C.c_size_t(snap.buffer.numel())

    def call():
        rc = env._lib.sg_restore_device(env._h, buf, n, None, None, None, stream)
        assert rc == 0, rc
    return call


def d2d_copy(snap):
    other = torch.empty_like(snap.buffer)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    dst, src, n = C.c_void_p(other.data_ptr()), C.c_void_p(snap.buffer.data_ptr()), C.c_size_t(snap.buffer.numel())

    def call():
        rc = _hip.hipMemcpyAsync(dst, src, n, D2D, stream)
        assert rc == 0, rc
    call.keep = other
    return call


def measure(env_id, B):
    dev, env, snap = setup(env_id, B)
    gen = torch.Generator(device=dev).manual_seed(2)
    mask = (torch.rand(B, device=dev, generator=gen) < 0.1).view(torch.uint8)
    perm = torch.randperm(B, device=dev, generator=gen).to(torch.int32)
    obs = torch.empty((B, env.obs_dim), device=dev)
    one = torch.zeros(1, device=dev)
    calls = {
        "snapshot": lambda: env.snapshot_torch(out=snap),
        "restore": lambda: env.restore_torch(snap, out=obs),
        "restore_no_obs": restore_no_obs(env, snap),
        "restore_mask_10pct": lambda: env.restore_torch(snap, mask=mask, out=obs),
        "restore_permutation": lambda: env.restore_torch(snap, src=perm, out=obs),
        "d2d_copy": d2d_copy(snap),
        "one_element_fill_launch": lambda: one.zero_(),
    }
    reps, per = (15, 50) if B <= 65536 else (11, 20)
    for fn in calls.values():  # warm
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0), snapshot_bytes=int(snap.buffer.numel()),
               bytes_per_env=round(snap.buffer.numel() / B, 2), mask_bits=int(mask.sum().item()), unit="us per call: median, p10, p90")
    for k, fn in calls.items():
        res[k] = timed(fn, reps, per)
    # the host round trip (synchronises twice; wall clock around it)
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blob = env.save_state()
        env.load_state(blob)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    res["host_save_plus_load"] = [round(float(v), 1) for v in (np.median(host), np.min(host), np.max(host))]
    res["host_blob_bytes"] = int(blob.size)
    copy = res["d2d_copy"][0]
    res["snapshot_over_d2d"] = round(res["snapshot"][0] / copy, 2)
    res["restore_no_obs_over_d2d"] = round(res["restore_no_obs"][0] / copy, 2)
    res["permutation_over_identity_restore"] = round(res["restore_permutation"][0] / res["restore"][0], 2)
    res["host_over_snapshot_plus_restore"] = round(res["host_save_plus_load"][0] / (res["snapshot"][0] + res["restore"][0]), 1)
    env.check_status()
    env.close()
    return res


def kernel_trace_phase():
    for env_id in ("GoalContinuous3P-v0", "KeplerCircleOrbit-v0"):
        _, env, snap = setup(env_id, 1048576)
        no_obs, copy = restore_no_obs(env, snap), d2d_copy(snap)
        for fn in (lambda: env.snapshot_torch(out=snap), no_obs, copy):
            for _ in range(100):
                fn()
        torch.cuda.synchronize()
        print(env_id, "snapshot bytes", int(snap.buffer.numel()), flush=True)
        env.close()


def main():
    if "--kernel-trace" in sys.argv:
        return kernel_trace_phase()
    lines = []
    for env_id in ("GoalContinuous3P-v0", "KeplerCircleOrbit-v0"):
        for B in (65536, 1048576):
            line = json.dumps(measure(env_id, B))
            print(line, flush=True)
            lines.append(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
