#!/usr/bin/env python3
"""Measurement: what prioritized replay sampling costs for GoalContinuous3P-v0 and KeplerCircleOrbit-v0 at B = 65 536, T = 256,
ring full (the synthetic ring of tools/gpu_replay_cost.py), priorities spread by an update of 4 M random cells.  Same method as
tools/gpu_replay_cost.py: stream events around back-to-back calls after a warm-up, median / p10 / p90 in microseconds per call,
the host side of each call included.
  * sample_prioritized (draw + gather + weight normalisation) and draw alone at n = 4 096, 65 536, 1 048 576, n_step 1 and 5;
    update at the same n; commit of a 20-step rollout with and without priority=, and the priorities' commit alone.
  * yardsticks: uniform = replay_sample_torch at the same shape (`--uniform` prints only these, so that the same numbers can be
    taken from another build of the library through SPACEGYM_LIB); torch_eager = the same draw written in torch (float64 cumsum
    over all T B priorities + searchsorted + the eager gather of tools/gpu_replay_cost.py), and for the update the same semantics in
    torch (quantise, window mask, amax scatter, running maximum), for the commit two slice assignments (the eager design leaves
    the total to the next draw's cumulative sum; torch_eager_commit_with_total also sums all T B priorities); copy_same_bytes = a copy_ of the bytes the batch writes.
One JSON line per shape.
    python tools/gpu_priority_cost.py [--uniform] [out.jsonl]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402
from gpu_replay_cost import B, DRAWS, GAMMA, IDS, K, N_STEPS, T, fill, timed, torch_eager  # noqa: E402


def bench(fn, per):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return timed(fn, 9, per)


def eager_draw(pri64, n, v_cells):
    """the draw a user writes without the feature: float64 cumulative sum over every cell, stratified uniform numbers, searchsorted"""
    csum = torch.cumsum(pri64, 0)
    total = csum[-1]
    r = (torch.arange(n, device=pri64.device, dtype=torch.float64) + torch.rand(n, device=pri64.device, dtype=torch.float64)) * (total / n)
    cell = torch.searchsorted(csum, r, right=True).clamp_(max=pri64.numel() - 1)
    w = (v_cells * pri64[cell] / total) ** -0.4
    return cell, (w / w.max()).float()


def eager_update(pri64, state, cell, p, head, v):
    """the update's semantics in torch: quantise, skip cells outside the window, the largest of duplicates wins, running maximum"""
    q = torch.clamp(torch.round(p.double() * 65536.0), 1.0, 4294967295.0)
    on = ((head - 1 - cell // B) % T) < v
    c, q = cell[on], q[on]
    new = torch.zeros_like(pri64).scatter_reduce(0, c, q, "amax", include_self=True)
    pri64[c] = new[c]
    state["max_q"] = torch.maximum(state["max_q"], q.max())


def measure(env_id, uniform_only):
    env = sg.make_vec(env_id, B, device=0, seed=0)
    ring = env.replay_torch(T)
    fill(env, ring)
    D = env.obs_dim
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    one = torch.zeros(1, device=dev)
    empty = timed(lambda: one.fill_(1.0), 9, 200)
    lines = []
    if not uniform_only:
        prio = env.replay_priority_torch(ring)
        env.replay_priority_begin_torch(prio)
        head, filled = ring.head, ring.filled
        env.replay_priority_commit_torch(prio, 0, 0, T)          # every slot, then the ring's own last commit puts the hole in place
        env.replay_priority_commit_torch(prio, (head - 16) % T, T, 16)
        spread = torch.randint(0, T * B, (1 << 22,), device=dev, generator=g)
        env.replay_update_priorities_torch(prio, spread, priority=torch.rand(1 << 22, device=dev, generator=g) ** 3 * 4)
        torch.cuda.synchronize()
        env.check_status()
        pri64 = (prio.leaf.reshape(-1).to(torch.int64) & 0xFFFFFFFF).double() / 65536.0
        v = min(filled, T - 1)
    for n in DRAWS:
        per = max(4, min(200, (1 << 22) // n))
        for n_step in N_STEPS:
            out = env.replay_sample_torch(ring, n, seed=1, n_step=n_step, gamma=GAMMA)
            line = dict(env_id=env_id, B=B, T=T, n=n, n_step=n_step, device=torch.cuda.get_device_name(0), calls_per_timing=per,
                        lib=os.environ.get("SPACEGYM_LIB", "product"), unit="us per call: median, p10, p90", empty_launch=empty)
            line["uniform"] = bench(lambda: env.replay_sample_torch(ring, n, seed=1, n_step=n_step, gamma=GAMMA, out=out), per)
            if not uniform_only:
                pout = env.replay_sample_prioritized_torch(ring, prio, n, seed=1, n_step=n_step, gamma=GAMMA)
                dout = {k: pout[k] for k in ("index", "cell", "weight")}
                batch_bytes = n * (2 * D * 4 + 8 + 4 + 1 + 1 + 4 + 1 + 8 + 8 + 4)
                src = torch.empty(batch_bytes, dtype=torch.uint8, device=dev).random_(0, 255)
                dst = torch.empty_like(src)

                def eager():
                    cell, w = eager_draw(pri64, n, float(v * B))
                    p, i = cell // B, cell % B
                    return torch_eager(ring, ((p - (head - v)) % T) * B + i, n_step), w
                line["sample_prioritized"] = bench(lambda: env.replay_sample_prioritized_torch(ring, prio, n, seed=1, n_step=n_step,
                                                                                              gamma=GAMMA, out=pout), per)
                line["draw"] = bench(lambda: env.replay_priority_draw_torch(ring, prio, n, seed=1, out=dout), per)
                line["draw_independent"] = bench(lambda: env.replay_priority_draw_torch(ring, prio, n, seed=1, stratified=False, out=dout), per)
                line["torch_eager"] = bench(eager, max(2, per // 8))
                line["copy_same_bytes"] = bench(lambda: dst.copy_(src), per)
                line["batch_bytes"] = batch_bytes
                line["prioritized_over_uniform"] = round(line["sample_prioritized"][0] / line["uniform"][0], 2)
                line["torch_eager_over_prioritized"] = round(line["torch_eager"][0] / line["sample_prioritized"][0], 1)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if not uniform_only:
        for n in DRAWS:
            per = max(4, min(200, (1 << 22) // n))
            cell = env.replay_priority_draw_torch(ring, prio, n, seed=5)["cell"].clone()
            p = torch.rand(n, device=dev, generator=g) * 3
            td = torch.randn(n, device=dev, generator=g)
            eager_pri, state = pri64.clone(), dict(max_q=torch.tensor(65536.0, dtype=torch.float64, device=dev))
            line = dict(env_id=env_id, B=B, T=T, n=n, device=torch.cuda.get_device_name(0), calls_per_timing=per,
                        unit="us per call: median, p10, p90", empty_launch=empty)
            line["update"] = bench(lambda: env.replay_update_priorities_torch(prio, cell, priority=p), per)
            line["update_td_error"] = bench(lambda: env.replay_update_priorities_torch(prio, cell, td_error=td), per)
            line["torch_eager_update"] = bench(lambda: eager_update(eager_pri, state, cell, p, head, v), max(2, per // 8))
            line["torch_eager_over_update"] = round(line["torch_eager_update"][0] / line["update"][0], 1)
            lines.append(line)
            print(json.dumps(line), flush=True)
        term = env.terminal_list_torch(1024)

        def commit(with_prio):
            ring.head, ring.filled = 0, 0
            env.replay_commit_torch(ring, K, terminal=term, priority=prio if with_prio else None)
        line = dict(env_id=env_id, B=B, T=T, device=torch.cuda.get_device_name(0), unit="us per call: median, p10, p90", empty_launch=empty)
        line["commit_20_steps_ring_only"] = bench(lambda: commit(False), 100)
        line["commit_20_steps_with_priorities"] = bench(lambda: commit(True), 100)
        eager_pri = pri64.clone()

        def eager_commit():
            eager_pri[:K * B] = 65536.0
            eager_pri[K * B:(K + 1) * B] = 0.0
        line["torch_eager_commit"] = bench(eager_commit, 100)
        tot = dict(total=eager_pri.sum())

        def eager_commit_total():  # the same with the total kept current, as the tree's commit leaves it
            eager_commit()
            tot["total"] = eager_pri.sum()
        line["torch_eager_commit_with_total"] = bench(eager_commit_total, 100)
        line["priority_commit_alone"] = bench(lambda: env.replay_priority_commit_torch(prio, 0, 0, K), 100)
        lines.append(line)
        print(json.dumps(line), flush=True)
    torch.cuda.synchronize()
    env.check_status()
    env.close()
    return lines


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = []
    for env_id in IDS:
        lines += [json.dumps(x) for x in measure(env_id, "--uniform" in sys.argv)]
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
