#!/usr/bin/env python3
"""Measurement: what one PPO minibatch update of a whole population costs at GoalContinuous3P-v0 on 65 536 envs, every member an actor and
a critic of two hidden layers of 64 (tanh), P = 1 / 4 / 16 / 64 / 256 members on 65 536 rows in total (n = 65 536 / P entries per member),
and P = 4 and 16 at 4 096 entries per member -- in the same run, on the same rows, with the same objective (clip 0.2, value clip 0.2,
ent_coef 0.01, vf_coef 0.5, normalised advantages; the population call takes them as a coefficient tensor of equal rows):
  * population:  population_ppo_grad_torch(pop, batch, index [P, n], coef): two or three launches for all members
  * loop:        P ppo_grad_torch calls on population_member_torch views with index[m]: what there was before
  * eager:       the gathers, population_evaluate_torch, the loss in torch with per-member advantage normalisation, summed, backward()
  * grad:        population_grad_torch alone on gathered rows, for scale
Expectations, stated before the first run (nobody had measured either):
  1. P = 1 costs what ppo_grad_torch costs at the same n (DESIGN section 24 has 634 us at 65 536 rows; re-measured here as `loop` at P = 1).
  2. Larger P costs about what population_grad_torch costs at that P, plus the advantage pass (a few microseconds).
The yardstick is the loop of P calls in the same run; no threshold is fixed.

Stream events around back-to-back calls after a warm-up of every timed shape; the forms are timed in alternating windows of the same run;
median, 10th and 90th percentile over the windows, microseconds per update of the whole population, the host side of every call
included.  Writes the text profile (default profiles/population_ppo_cost.txt) and prints one JSON line per shape.
    python tools/gpu_population_ppo_cost.py [profile.txt]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

ENV_ID, HIDDEN, ENVS = "GoalContinuous3P-v0", 64, 65536
CLIP, CLIP_VF, ENT, VF = 0.2, 0.2, 0.01, 0.5
REPS = 10
SHAPES = [(1, 65536), (4, 16384), (16, 4096), (64, 1024), (256, 256), (4, 4096)]  # (P, n per member); (16, 4096) is both kinds of row


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def alternating(fns):
    """{name: [median, p10, p90]} microseconds per call; fns: {name: (function, calls per window)}, timed in alternating windows"""
    for fn, _ in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(REPS):
        for k, (fn, inner) in fns.items():
            out[k].append(window(fn, inner))
    return {k: [round(float(x), 2) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))] for k, v in out.items()}


def measure(env, batch, P, n):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(P)
    D = env.obs_dim

    def net(out):
        dims = [D, HIDDEN, HIDDEN, out]
        return [((torch.rand((P, o, i), device=dev, generator=g) * 2 - 1) / i ** 0.5, (torch.rand((P, o), device=dev, generator=g) * 2 - 1) / i ** 0.5)
                for i, o in zip(dims[:-1], dims[1:])]
    actor, critic = net(2), net(1)
    log_std = torch.full((P, 2), -0.5, device=dev)
    pop = env.policy_population_torch(P, actor=actor, critic=critic, log_std=log_std)
    members = [env.population_member_torch(pop, m) for m in range(P)]
    index = torch.stack([torch.randperm(ENVS, device=dev, generator=g)[:n] for _ in range(P)]) if P * n != ENVS else torch.randperm(
        ENVS, device=dev, generator=g).reshape(P, n)
    coef = torch.tensor([[CLIP, CLIP_VF, ENT, VF]] * P, device=dev)
    kw = dict(clip_range=CLIP, clip_range_vf=CLIP_VF, ent_coef=ENT, vf_coef=VF)
    grads, stats = env.population_ppo_grad_torch(pop, batch, index, coef=coef)
    singles = [env.ppo_grad_torch(members[m], batch, index[m], **kw) for m in range(P)]

    def population():
        env.population_ppo_grad_torch(pop, batch, index, coef=coef, out=grads, stats=stats)

    def loop():
        for m in range(P):
            env.ppo_grad_torch(members[m], batch, index[m], out=singles[m][0], stats=singles[m][1], **kw)

    def eager():
        for t in pop.tensors:
            t.grad = None
        o, a, old, adv, ret, ov = (batch[k][index] for k in ("obs", "action", "logp", "advantage", "ret", "value"))
        lp, ent, v = env.population_evaluate_torch(pop, o, a)
        adv = (adv - adv.mean(1, keepdim=True)) / (adv.std(1, keepdim=True) + 1e-8)
        ratio = torch.exp(lp - old)
        pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean(1)
        vl = 0.5 * torch.max((v - ret) ** 2, (ov + torch.clamp(v - ov, -CLIP_VF, CLIP_VF) - ret) ** 2).mean(1)
        (pg - ENT * ent.mean(1) + VF * vl).sum().backward()

    obs_g, action_g = batch["obs"][index].contiguous(), batch["action"][index].contiguous()
    gs = [torch.randn((P, n), device=dev, generator=g) / n for _ in range(3)]
    alone = env.population_grad_torch(pop, obs_g, action_g, *gs)
    for t in pop.tensors:
        t.requires_grad_(True)
    eager()
    population()
    flat = [t for pair in grads["actor"] + grads["critic"] for t in pair] + [grads["log_std"]]
    agree = max(float((a - p.grad).abs().max()) for a, p in zip(flat, pop.tensors))
    top = max(float(p.grad.abs().max()) for p in pop.tensors)
    same = all(torch.equal(stats[m], singles[m][1]) for m in range(P))  # the statistics of the loop's calls, bit for bit
    us = alternating(dict(population=(population, 20), loop=(loop, max(1, 20 // P)), eager=(eager, 5),
                          grad=(lambda: env.population_grad_torch(pop, obs_g, action_g, *gs, out=alone), 20)))
    for t in pop.tensors:
        t.grad = None
        t.requires_grad_(False)
    return dict(env_id=ENV_ID, members=P, n=n, rows=P * n, hidden=HIDDEN, n_hidden=2, population_us=us["population"], loop_us=us["loop"],
                eager_us=us["eager"], grad_us=us["grad"], population_over_loop=round(us["population"][0] / us["loop"][0], 3),
                population_over_eager=round(us["population"][0] / us["eager"][0], 3),
                population_minus_grad_us=round(us["population"][0] - us["grad"][0], 2), stats_equal_loop_bits=same,
                max_abs_grad_diff_vs_eager=agree, max_abs_grad=top)


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")] or [os.path.join(ROOT, "profiles", "population_ppo_cost.txt")]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, ENVS, device=0, seed=1)
    obs = env.reset_torch().clone()
    rnd = lambda *s: torch.randn(s, device=dev)  # noqa: E731
    batch = dict(obs=obs, action=rnd(ENVS, 2), logp=-2.0 + 0.3 * rnd(ENVS), value=0.3 * rnd(ENVS), advantage=rnd(ENVS), ret=rnd(ENVS))
    lines = ["Cost of one PPO minibatch update of a population: population_ppo_grad_torch against the loop of P ppo_grad_torch calls on member views",
             "and against the update composed in torch over population_evaluate_torch -- the same rows, indices and objective, timed in",
             "alternating windows of one run.  %s, tools/gpu_population_ppo_cost.py; stream events around back-to-back calls after a warm-up,"
             % torch.cuda.get_device_name(0),
             "%d windows each; microseconds per update of ALL members: median [p10, p90], the host side of every call included." % REPS,
             "Expected before the run: (1) P = 1 costs what ppo_grad_torch costs at the same n; (2) larger P costs about what",
             "population_grad_torch costs at that P, plus the advantage pass.", "",
             "%s, %d envs, every member an actor and a critic of two hidden layers of %d" % (ENV_ID, ENVS, HIDDEN)]
    row = lambda name, v: "  %-56s %10.2f  [%10.2f, %10.2f]" % (name, *v)  # noqa: E731
    for P, n in SHAPES:
        rec = measure(env, batch, P, n)
        print(json.dumps(rec), flush=True)
        verdict = "faster" if rec["population_over_loop"] < 1 else "NOT faster"
        lines += ["", "P = %d members x n = %d entries (%d rows)" % (P, n, P * n),
                  row("population_ppo_grad_torch (two or three launches)", rec["population_us"]),
                  row("loop of %d ppo_grad_torch calls" % P, rec["loop_us"]),
                  row("eager torch over population_evaluate_torch", rec["eager_us"]),
                  row("population_grad_torch alone (two launches)", rec["grad_us"]),
                  "  population / loop = %.3f (the population call is %s than the loop); population / eager = %.3f; population - grad alone = %.2f us"
                  % (rec["population_over_loop"], verdict, rec["population_over_eager"], rec["population_minus_grad_us"]),
                  "  statistics bit-equal to the loop's: %s; largest gradient difference to the eager update %.2g (largest entry %.2g)"
                  % (rec["stats_equal_loop_bits"], rec["max_abs_grad_diff_vs_eager"], rec["max_abs_grad"])]
    env.check_status()
    env.close()
    for p in paths:
        os.makedirs(os.path.dirname(os.path.abspath(p)), exist_ok=True)
        with open(p, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
