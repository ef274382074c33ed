#!/usr/bin/env python3
"""Measurement: what the replay ring costs (replay_sample_torch / replay_commit_torch) for GoalContinuous3P-v0 and
KeplerCircleOrbit-v0 at B = 65 536, T = 256, ring full (synthetic rows, ~2 % of the steps done, half of those truncated).
  * sample: n = 4 096, 65 536, 1 048 576 draws with n_step = 1 and 5; commit_list: a 20-step rollout with its terminal list;
    commit_dense: one step with dense terminal rows.  Stream events around back-to-back calls after a warm-up -- median, 10th and
    90th percentile over the repetitions, microseconds per call, the host side of each call included.
  * torch_eager: the same batch the way a user writes it without this feature -- index arithmetic, advanced indexing on the
    [T * B, D] views, the terminal join through a dense [T, B] index, the n-step loop with masks; the same indices (the kernel's
    `index` output of the same call number), timed the same way; its output must equal the kernel's bit for bit at n_step = 1
    (checked here; at n_step = 5 torch's a + b * c may contract, so the returns are compared to 1e-6).
  * copy_same_bytes: a copy_ of as many bytes as the batch writes;  empty_launch: a one-lane torch kernel (fill_ of one element).
One JSON line per shape.
    python tools/gpu_replay_cost.py [out.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_replay_cost.py --kernel-trace"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

IDS = ("GoalContinuous3P-v0", "KeplerCircleOrbit-v0")
B, T, K = 65536, 256, 20
DRAWS = (4096, 65536, 1048576)
N_STEPS = (1, 5)
GAMMA = 0.99


def fill(env, ring, seed=0):
    """a full ring of synthetic rows: K-step commits with their lists, a lap and a bit"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    D = env.obs_dim
    env.replay_begin_torch(ring, torch.randn((B, D), device=dev, generator=g))
    lists = []
    k_fill = 16  # divides T
    for _ in range(T // k_fill + 2):
        rows = ring.rows(k_fill)
        rows["obs"].copy_(torch.randn((k_fill, B, D), device=dev, generator=g))
        rows["action"].copy_(torch.rand((k_fill, B, 2), device=dev, generator=g) * 2 - 1)
        rows["reward"].copy_(torch.randn((k_fill, B), device=dev, generator=g))
        done = torch.rand((k_fill, B), device=dev, generator=g) < 0.02
        rows["done"].copy_(done)
        rows["trunc"].copy_(done & (torch.rand((k_fill, B), device=dev, generator=g) < 0.5))
        se = done.nonzero().to(torch.int32)
        n = int(se.shape[0])
        term = env.terminal_list_torch(n + 1024)
        term["count"].fill_(n)
        term["step_env"][:n] = se[torch.randperm(n, device=dev, generator=g)]
        term["obs"].copy_(torch.randn(term["obs"].shape, device=dev, generator=g))
        env.replay_commit_torch(ring, k_fill, terminal=term)
        lists.append(term)
    torch.cuda.synchronize()
    env.check_status()
    return lists


def torch_eager(ring, u, n_step, gamma=GAMMA):
    """what a user writes at the parent commit, from the same ring tensors and the same transition numbers u (int64 [n])"""
    Tn, Bn, D = ring.steps, ring.num_envs, ring.obs_dim
    v, h = min(ring.filled, Tn - 1), ring.head
    q, i = u // Bn, u % Bn
    first = (h - v) % Tn
    p0 = (first + q) % Tn
    flat = lambda p: p * Bn + i  # noqa: E731
    obs2, rew, done, trunc = ring.obs.view(Tn * Bn, D), ring.reward.view(-1), ring.done.view(-1), ring.trunc.view(-1)
    s = obs2[flat((p0 - 1) % Tn)]
    a = ring.action.view(Tn * Bn, -1)[flat(p0)]
    R = rew[flat(p0)].double()
    g = torch.full_like(R, gamma)
    last = torch.zeros_like(u)
    open_ = torch.ones_like(u, dtype=torch.bool)
    for k in range(1, n_step):
        open_ = open_ & (done[flat((first + q + k - 1) % Tn)] == 0) & (q + k < v)
        R = torch.where(open_, R + g * rew[flat((first + q + k) % Tn)].double(), R)
        g = torch.where(open_, g * gamma, g)
        last = torch.where(open_, torch.full_like(last, k), last)
    fl = flat((first + q + last) % Tn)
    fin, tr = done[fl] != 0, trunc[fl] != 0
    slot = torch.where(fin, ring.term_idx.view(-1)[fl].long() % ring.term_capacity, torch.zeros_like(fl))
    s2 = torch.where(fin[:, None], ring.term_obs[slot], obs2[fl])
    return dict(obs=s, action=a, reward=R.float(), next_obs=s2, terminated=(fin & ~tr).to(torch.uint8), truncated=tr.to(torch.uint8),
                discount=g.float(), steps=(last + 1).to(torch.uint8))


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


def measure(env_id):
    env = sg.make_vec(env_id, B, device=0, seed=0)
    ring = env.replay_torch(T)
    fill(env, ring)
    D = env.obs_dim
    res = []
    one = torch.zeros(1, device="cuda")
    empty = timed(lambda: one.fill_(1.0), 9, 200)
    for n in DRAWS:
        for n_step in N_STEPS:
            out = env.replay_sample_torch(ring, n, seed=1, n_step=n_step, gamma=GAMMA)
            torch.cuda.synchronize()
            u = out["index"].clone()
            kern = {k: v.clone() for k, v in env.replay_sample_torch(ring, n, n_step=n_step, gamma=GAMMA, index=u, out=out).items()}
            eager = torch_eager(ring, u, n_step)
            torch.cuda.synchronize()
            if n_step == 1:
                equal = all(torch.equal(kern[k].view(torch.int32) if kern[k].dtype == torch.float32 else kern[k],
                                        eager[k].view(torch.int32) if eager[k].dtype == torch.float32 else eager[k]) for k in eager)
            else:
                equal = all(torch.equal(kern[k], eager[k]) for k in eager if k not in ("reward", "discount")) and bool(
                    torch.allclose(kern["reward"], eager["reward"], rtol=1e-6, atol=1e-6) and torch.allclose(kern["discount"], eager["discount"]))
            batch_bytes = n * (2 * D * 4 + 8 + 4 + 1 + 1 + 4 + 1 + 8)
            src = torch.empty(batch_bytes, dtype=torch.uint8, device="cuda").random_(0, 255)
            dst = torch.empty_like(src)
            per = max(4, min(200, (1 << 22) // n))
            fns = {"sample": lambda: env.replay_sample_torch(ring, n, seed=1, n_step=n_step, gamma=GAMMA, out=out),
                   "sample_index": lambda: env.replay_sample_torch(ring, n, n_step=n_step, gamma=GAMMA, index=u, out=out),
                   "torch_eager": lambda: torch_eager(ring, u, n_step), "copy_same_bytes": lambda: dst.copy_(src)}
            line = dict(env_id=env_id, B=B, T=T, n=n, n_step=n_step, device=torch.cuda.get_device_name(0), batch_bytes=batch_bytes,
                        eager_equals_kernel=bool(equal), calls_per_timing=per, unit="us per call: median, p10, p90", empty_launch=empty)
            for name, fn in fns.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                line[name] = timed(fn, 9, per)
            line["torch_eager_over_sample"] = round(line["torch_eager"][0] / line["sample_index"][0], 1)
            line["sample_over_copy"] = round(line["sample"][0] / line["copy_same_bytes"][0], 2)
            res.append(line)
            print(json.dumps(line), flush=True)
    # commits: the host mirror is put back to an empty ring before every call, so that each call commits the same slots again (the
    # device work is the same; the live window stays one commit long, so the repeated records never trip the capacity check)
    se = (ring.done[:K] != 0).nonzero().to(torch.int32)
    n_rec = int(se.shape[0])
    term = env.terminal_list_torch(n_rec + 1024)
    term["count"].fill_(n_rec)
    term["step_env"][:n_rec] = se[torch.randperm(n_rec, device="cuda")]
    term["obs"].normal_()
    tobs = torch.randn((B, D), device="cuda")

    def commit(k, **kw):
        ring.head, ring.filled = 0, 0
        env.replay_commit_torch(ring, k, **kw)
    line = dict(env_id=env_id, B=B, T=T, device=torch.cuda.get_device_name(0), list_records=n_rec,
                dense_records=int((ring.done[0] != 0).sum().item()), unit="us per call: median, p10, p90", empty_launch=empty)
    for name, fn in (("commit_list_20_steps", lambda: commit(K, terminal=term)), ("commit_dense_1_step", lambda: commit(1, terminal_obs=tobs))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        line[name] = timed(fn, 9, 100)
    torch.cuda.synchronize()
    env.check_status()
    res.append(line)
    print(json.dumps(line), flush=True)
    env.close()
    return res


def kernel_trace_phase():
    for env_id in IDS:
        env = sg.make_vec(env_id, B, device=0, seed=0)
        ring = env.replay_torch(T)
        fill(env, ring)
        for n in DRAWS:
            for n_step in N_STEPS:
                out = env.replay_sample_torch(ring, n, seed=1, n_step=n_step)
                for _ in range(20):
                    env.replay_sample_torch(ring, n, seed=1, n_step=n_step, out=out)
        torch.cuda.synchronize()
        print("traced", env_id, flush=True)
        env.close()


def main():
    if "--kernel-trace" in sys.argv:
        return kernel_trace_phase()
    lines = []
    for env_id in IDS:
        lines += [json.dumps(x) for x in measure(env_id)]
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
