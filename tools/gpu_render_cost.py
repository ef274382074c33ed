#!/usr/bin/env python3
"""Measurement: what one render call (sg_render_device: render_setup_kernel + render_raster_kernel) costs.  GoalContinuous3P-v0,
65 536 envs, frames of the first n envs: n = 1, 64, 1024 at 600 px and n = 65 536 at 84 px.  Stream events around each call,
median over the repetitions; achieved write bandwidth = frame bytes / time, against the ~6.3 TB/s a float4 copy reaches (a
copy of the same byte count is timed as well).  For context: frames/s of the NumPy model (tests/render_model.py) on one core.
Run under `rocprofv3 --kernel-trace --stats` for the two kernels' own durations.
    python tools/gpu_render_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

COPY_TBS = 6.3


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ts.append(start.elapsed_time(stop) * 1e3)
    return float(np.median(ts))


def main():
    env_id, B = "GoalContinuous3P-v0", 65536
    env = sg.make_vec(env_id, B, device=0, seed=1, render=dict(capacity=B))
    env.reset_torch()
    act = torch.rand((B, 2), device="cuda") * 2 - 1
    for _ in range(20):  # traces of some length
        env.step_torch(act)
        env.render_torch(torch.arange(1024, dtype=torch.int32, device="cuda"), actions=act, size=84)
    res = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0), cases=[])
    for n, size, reps in ((1, 600, 200), (64, 600, 50), (1024, 600, 20), (65536, 84, 10)):
        ids = torch.arange(n, dtype=torch.int32, device="cuda")
        out = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            env.render_torch(ids, actions=act, size=size, out=out)
        us = timed(lambda: env.render_torch(ids, actions=act, size=size, out=out), reps)
        nbytes = out.numel()
        words = nbytes // 16
        src = torch.empty(words * 4, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        copy_us = timed(lambda: dst.copy_(src), reps)  # reads and writes nbytes each
        res["cases"].append(dict(n=n, size=size, us=us, frame_bytes=nbytes, write_TBs=nbytes / us / 1e6,
                                 share_of_copy_rate=nbytes / us / 1e6 / COPY_TBS, same_bytes_copy_us=copy_us,
                                 frames_per_s=n / us * 1e6))
        del out, src, dst
    env.check_status()
    # the NumPy model, one core, after reset-like inputs
    import render_model as rm
    obs = env.reset()
    st = env.get_state()
    spec = dict(family="goal", n_planets=3)
    for size in (600, 84):
        t0, k = time.perf_counter(), 0
        while time.perf_counter() - t0 < 2.0:
            rm.render_env(size, spec, obs[k], st["planets"][k], st["goal"][k], None, [tuple(obs[k, :2])], 0.85, True, False)
            k += 1
        res[f"numpy_model_frames_per_s_{size}px"] = k / (time.perf_counter() - t0)
    env.close()
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
