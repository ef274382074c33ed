#!/usr/bin/env python3
"""Measurement: what a batch of fixed-length sequences out of the replay ring costs (replay_sample_sequences_torch), on a full ring of
T = 256 slots of B = 65 536 envs (GoalContinuous3P-v0, D = 15, and KeplerCircleOrbit-v0, D = 10) filled with random rows, ~2 % of the
steps done, two extra [T, B] columns gathered along, at (n, L) = (4 096, 16), (65 536, 16), (65 536, 64) and -- for the third
expectation, which speaks of at most 65 536 rows -- (3 840, 16).  The same `index` is handed to every form:
  * sequences     replay_sample_sequences_torch(index=, columns=, out=): one launch and the one-lane tick
  * eager         the same batch in eager torch: index arithmetic, advanced-indexing gathers over the ring's [T, B, ...] members and
                  the terminal join through term_idx, with no host synchronisation (torch.where, not a boolean mask).  Checked once
                  per shape to be BIT-EQUAL to the call's outputs
  * single_loop   L calls of replay_sample_torch(index = index + k B, n_step = 1, out=): what the ring offered before
  * copy          one copy_ of as many bytes as the call writes (observation rows, step members, columns, index; terminal rows not
                  counted): the floor for the write side alone
  * single        one replay_sample_torch(n = 4 096, n_step = 1) call: the host cost of one call of the existing sampler
Stream events around back-to-back calls after a warm-up; the forms alternate window by window within one run; median, 10th and 90th
percentile over the windows, microseconds per call, host side included.

EXPECTATION, written before the first run (nothing here had been measured):
  (1) under the eager composition at every shape;
  (2) under the loop of L single-transition calls at every shape;
  (3) near the host cost of one call (about 22 us, the existing sampler's) while (L + 1) n is at most 65 536 rows: "near" is taken as
      at most 1.5 x `single` of the same run.
The tool prints for each whether it held.  One JSON line per env id and shape.
    python tools/gpu_sequence_cost.py profiles/sequence_cost.txt"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

T, B, K = 256, 65536, 64
IDS = ("GoalContinuous3P-v0", "KeplerCircleOrbit-v0")
SHAPES = ((3840, 16), (4096, 16), (65536, 16), (65536, 64))
NEAR = 1.5


def fill(env, seed=0):
    """a full ring: T / K commits of K slots of random rows, ~2 % done, half of those truncated, list-form terminal records"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    D = env.obs_dim
    ring = env.replay_torch(T)
    env.replay_begin_torch(ring, torch.randn((B, D), device=dev, generator=g))
    for _ in range(T // K + 1):  # one commit more than a lap: the ring has wrapped
        rows = ring.rows(K)
        rows["obs"].copy_(torch.randn((K, B, D), device=dev, generator=g))
        rows["action"].copy_(torch.rand((K, B, 2), device=dev, generator=g) * 2 - 1)
        rows["reward"].copy_(torch.randn((K, B), device=dev, generator=g))
        done = torch.rand((K, B), device=dev, generator=g) < 0.02
        rows["done"].copy_(done.to(torch.uint8))
        rows["trunc"].copy_((done & (torch.rand((K, B), device=dev, generator=g) < 0.5)).to(torch.uint8))
        se = done.nonzero().to(torch.int32).contiguous()
        term = dict(count=torch.tensor([se.shape[0]], dtype=torch.int32, device=dev), step_env=se,
                    obs=torch.randn((se.shape[0], D), device=dev, generator=g))
        env.replay_commit_torch(ring, K, terminal=term)
    env.check_status()
    cols = [torch.randn((T, B), device=dev, generator=g) for _ in range(2)]
    return ring, cols


def eager(ring, cols, index, L):
    """the batch of the call, composed in eager torch without a host synchronisation"""
    Bn, C = ring.num_envs, ring.term_capacity
    v = min(ring.filled, ring.steps - 1)
    q, i = index // Bn, index % Bn
    first = (ring.head - v) % ring.steps
    p = (first + q[None, :] + torch.arange(-1, L, device=index.device)[:, None]) % ring.steps  # [L + 1, n]
    ii = i[None, :].expand(L, -1)
    ps = p[1:]
    out = dict(obs=ring.obs[p, i[None, :].expand(L + 1, -1)], action=ring.action[ps, ii], reward=ring.reward[ps, ii],
               done=ring.done[ps, ii], trunc=ring.trunc[ps, ii], index=index.clone(), columns=[c[ps, ii] for c in cols])
    rec = (ring.term_idx[ps, ii].to(torch.int64) & 0xFFFFFFFF) % C
    out["terminal_obs"] = torch.where((out["done"] != 0)[..., None], ring.term_obs[rec], torch.zeros((), device=index.device))
    return out


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


def measure(env, ring, cols, n, L):
    dev = torch.device("cuda", 0)
    D = env.obs_dim
    S = len(ring) - (L - 1) * B
    index = torch.randint(0, S, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(n + L))
    out = env.replay_sample_sequences_torch(ring, n, L, index=index, columns=cols)
    want = eager(ring, cols, index, L)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for k in ("obs", "action", "reward", "done", "trunc", "terminal_obs", "index") for a, b in [(out[k], want[k])])
    same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out["columns"], want["columns"]))
    one = env.replay_sample_torch(ring, n, n_step=1, index=index)
    small = env.replay_sample_torch(ring, 4096, n_step=1, seed=1)
    shifted = [index + k * B for k in range(L)]
    written = (L + 1) * n * D * 4 + L * n * (8 + 4 + 1 + 1 + 2 * 4) + n * 8
    src, dst = torch.empty(written, dtype=torch.uint8, device=dev), torch.empty(written, dtype=torch.uint8, device=dev)

    def single_loop():
        for k in range(L):
            env.replay_sample_torch(ring, n, n_step=1, index=shifted[k], out=one)
    fns = {"sequences": lambda: env.replay_sample_sequences_torch(ring, n, L, index=index, columns=cols, out=out),
           "eager": lambda: eager(ring, cols, index, L), "single_loop": single_loop, "copy": lambda: dst.copy_(src),
           "single": lambda: env.replay_sample_torch(ring, 4096, n_step=1, seed=1, out=small)}
    rows = (L + 1) * n
    per = {"sequences": max(4, min(200, 2 ** 22 // rows)), "eager": max(2, min(20, 2 ** 19 // rows)),
           "single_loop": max(2, min(20, 2 ** 22 // (rows * 4))), "copy": max(4, min(200, 2 ** 22 // rows)), "single": 100}
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = dict(env_id=None, n=n, L=L, rows=rows, bytes_written=written,
               device=torch.cuda.get_device_name(0), calls_per_window=per, unit="us per call: median, p10, p90", bit_equal_to_eager=bool(same))
    res.update(timed(fns, 9, per))
    seq = res["sequences"][0]
    res["expectation"] = {"under_eager": bool(seq < res["eager"][0]), "eager_over_sequences": round(res["eager"][0] / seq, 2),
                          "under_single_loop": bool(seq < res["single_loop"][0]),
                          "single_loop_over_sequences": round(res["single_loop"][0] / seq, 2),
                          "sequences_over_copy": round(seq / res["copy"][0], 2),
                          "near_one_call": bool(seq <= NEAR * res["single"][0]) if rows <= 65536 else None,
                          "sequences_over_single": round(seq / res["single"][0], 2)}
    env.check_status()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = []
    for env_id in IDS:
        env = sg.make_vec(env_id, B, device=0, seed=0)
        ring, cols = fill(env)
        for n, L in SHAPES:
            res = measure(env, ring, cols, n, L)
            res["env_id"] = env_id
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
        env.close()
        del ring, cols
        torch.cuda.empty_cache()
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
