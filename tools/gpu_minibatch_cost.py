#!/usr/bin/env python3
"""Measurement: what minibatch_index_torch costs next to the floor and next to what a PPO user would write without it, at 65 536
envs, K = 20 rows, 4 epochs, M = 4 and 32 minibatches, P = 1, 4 and 256 members, unit "row".  Stream events around back-to-back calls
after a warm-up; the forms alternate window by window within one run; median, 10th and 90th percentile over nine windows, microseconds
per call, the host side of each call included.
  * index        minibatch_index_torch into a given tensor: one launch that writes 8 epochs M P n bytes and reads nothing
  * fill         index.fill_(1): a device fill of the same bytes, the floor
  * eager_torch  a torch.randperm per (epoch, member) (a sort of random keys), its first M n entries, and the row arithmetic
                 (j // E) B + m E + j % E into the same [epochs, M, P, n] tensor; checked once to satisfy the same properties
                 (every entry in its member's block, no repeat within one (epoch, member))
  * index_graph  one replay of a captured graph of the call and the bump of step_dev
  * index_env    the call with unit "env" (K stores per lane, one walk per env column); no expectation, to see the other path

EXPECTATION, written before the first run (nothing had been measured).  The kernel is compute-bound, not store-bound: per 8 bytes
stored a lane runs 8 Feistel rounds of about a dozen vector instructions (two of them 32-bit multiplies), 1.3 - 2 times over for the
cycle walk at these N, and a wave runs as long as its slowest lane; counting instructions gives about 35 us for the 5.2 M entries
against 10 - 15 us for storing 42 MB.  So:
  * index <= 4 x fill at every shape (and at least the fill);
  * index < eager_torch at every shape -- by more than 10 x at P = 256, where the eager form is 1 024 sorts;
  * index_graph <= index: a replay does not pay the Python method.
The tool prints the measured ratios beside these and says for each whether it held.  One JSON line per shape.
Added after the first run, which missed the first expectation (6.6 - 6.8 x) and the third (1.12 x), to see where the time goes; no
expectation was written for it: index_k16, the same call at K = 16, where N = K E is a power of two and no element walks (it writes
0.8 x the bytes), reported beside index in picoseconds per entry.  That run (index 65.9 - 67.0 us, index_k16 28.8 - 29.5 us, 12.6 and
6.9 ps per entry) showed a cost per wave that no walk explains: every wave formed both Philox blocks on the scalar unit.  The kernel
was then changed to form them once per workgroup of up to sixteen waves and pass them through LDS; the profile is of that kernel
(index_k16 19.3 - 20.4 us; index itself did not gain: at K = 20 the walks are the cost).
    python tools/gpu_minibatch_cost.py profiles/minibatch_cost.txt"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

B, K, EPOCHS = 65536, 20, 4
SHAPES = tuple((M, P) for M in (4, 32) for P in (1, 4, 256))


def window(fn, per):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(per):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / per


def alternating(fns, per, windows=9):
    """every form once per round, `windows` rounds: a drift of the machine lands on every form alike"""
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, per[k]))
    return {k: [round(float(x), 2) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))] for k, v in out.items()}


def eager_index(out, M, P, n):
    E = B // P
    for e in range(EPOCHS):
        for m in range(P):
            j = torch.randperm(K * E, device=out.device)[:M * n].view(M, n)
            out[e, :, m] = (j // E) * B + m * E + j % E
    return out


def properties(index, P):
    """every entry in its member's block of a row of the rollout; no repeat within one (epoch, member)"""
    epochs, M, _, n = index.shape
    E = B // P
    member = torch.arange(P, device=index.device).view(1, 1, P, 1)
    inside = bool(((index >= 0) & (index < K * B) & ((index % B) // E == member)).all())
    rows = index.permute(0, 2, 1, 3).reshape(epochs * P, M * n).sort(1).values
    return inside and bool((rows[:, 1:] != rows[:, :-1]).all())


def measure(M, P):
    env = sg.make_vec("GoalContinuous3P-v0", B, device=0, seed=0)
    dev = torch.device("cuda", 0)
    n = (K * (B // P)) // M
    index = torch.zeros((EPOCHS, M, P, n), dtype=torch.int64, device=dev)
    other = torch.zeros_like(index)
    n_env = K * ((B // P) // M)
    index_env = torch.zeros((EPOCHS, M, P, n_env), dtype=torch.int64, device=dev)
    step = [0]

    def call():
        step[0] += 1
        env.minibatch_index_torch(K, members=P, epochs=EPOCHS, minibatches=M, seed=1, step=step[0], out=index)

    def call_env():
        step[0] += 1
        env.minibatch_index_torch(K, members=P, epochs=EPOCHS, minibatches=M, unit="env", seed=1, step=step[0], out=index_env)

    n16 = (16 * (B // P)) // M
    index_k16 = torch.zeros((EPOCHS, M, P, n16), dtype=torch.int64, device=dev)

    def call_k16():
        step[0] += 1
        env.minibatch_index_torch(16, members=P, epochs=EPOCHS, minibatches=M, seed=1, step=step[0], out=index_k16)

    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)

    def captured():
        env.minibatch_index_torch(K, members=P, epochs=EPOCHS, minibatches=M, seed=1, step_dev=step_dev, out=index)
        step_dev.add_(1)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        captured()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured()
    fns = {"index": call, "fill": lambda: other.fill_(1), "eager_torch": lambda: eager_index(other, M, P, n), "index_graph": graph.replay,
           "index_env": call_env, "index_k16": call_k16}
    per = {"index": 50, "fill": 50, "eager_torch": 2, "index_graph": 50, "index_env": 50, "index_k16": 50}
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    call()
    ok = properties(index, P) and properties(eager_index(other, M, P, n), P)
    graph.replay()
    first = index.clone()
    graph.replay()
    res = dict(K=K, B=B, epochs=EPOCHS, M=M, P=P, n=n, device=torch.cuda.get_device_name(0), calls_per_window=per, properties_hold=ok,
               replays_differ=bool((first != index).any()), bytes_written=index.numel() * 8, unit="us per call: median, p10, p90")
    res.update(alternating(fns, per))
    i, f = res["index"][0], res["fill"][0]
    res["index_TBps"] = round(index.numel() * 8 / (i * 1e-6) / 1e12, 3)
    res["fill_TBps"] = round(index.numel() * 8 / (f * 1e-6) / 1e12, 3)
    res["ps_per_entry"] = dict(index=round(i * 1e6 / index.numel(), 2), index_k16=round(res["index_k16"][0] * 1e6 / index_k16.numel(), 2))
    res["expectations"] = {
        "fill <= index <= 4 x fill": dict(measured=round(i / f, 2), held=bool(f <= i <= 4 * f)),
        "index < eager_torch" + (" by more than 10 x" if P == 256 else ""): dict(
            measured=round(res["eager_torch"][0] / i, 1), held=bool(i * (10 if P == 256 else 1) < res["eager_torch"][0])),
        "index_graph <= index": dict(measured=round(res["index_graph"][0] / i, 2), held=bool(res["index_graph"][0] <= i)),
    }
    env.check_status()
    env.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = []
    for M, P in SHAPES:
        line = json.dumps(measure(M, P))
        print(line, flush=True)
        lines.append(line)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
