#!/usr/bin/env python3
"""Measurement: what the parameter update of a whole population costs at GoalContinuous3P-v0, every member an actor and a critic of two
hidden layers of 64 (tanh) -- 13 stacked tensors, 10 565 parameters per member -- for P = 1 / 4 / 16 / 64 / 256 members, in the same run,
on the same stacked tensors and gradients:
  * adam_step:   adam_step_torch(opt, grads): two launches for all members, per-member norm, clip and hyperparameters
  * fused:       clip_grad_norm_ + torch.optim.Adam(fused=True) on the stacked tensors: the cheapest torch offers, and OTHER semantics
                 (one norm over the whole population, one learning rate)
  * composed:    the per-member semantics in eager torch on the stacked tensors: per-member norms, [P, 1, 1] hyperparameters
  * loop:        P torch.optim.Adam optimizers over member views W[m], clip_grad_norm_ per member: what a caller had before
Expectation, stated before the first run (nobody had measured any of it): adam_step is flat in P up to where its traffic shows -- 32 B per
parameter (4 for the norm pass, 28 for the update), 86 MB at P = 256, about 11 us at the 8 TB/s roofline -- lies under the composed form at
every P, and far under the loop for P >= 4.  No time is fixed; the profile reports hit or miss.

Stream events around back-to-back calls after a warm-up of every timed form; the forms are timed in alternating windows of the same run;
median, 10th and 90th percentile over the windows, microseconds per update of the whole population, the host side of every call
included.  Writes the text profile (default profiles/adam_cost.txt) and prints one JSON line per P.
    python tools/gpu_adam_cost.py [profile.txt]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

ENV_ID, HIDDEN = "GoalContinuous3P-v0", 64
LR, BETAS, EPS, MAX_NORM = 3e-4, (0.9, 0.999), 1e-8, 0.5
REPS = 10
MEMBERS = [1, 4, 16, 64, 256]
BYTES_PER_PARAMETER = 32  # the gradient once for the norm; gradient, parameter and both moments read, parameter and both moments written


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


def measure(env, P):
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
    opt = env.adam_torch(pop, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM)
    gs = [torch.randn(t.shape, device=dev, generator=g) for t in pop.tensors]
    L = pop.n_hidden + 1
    pairs = lambda xs: [(xs[2 * l], xs[2 * l + 1]) for l in range(L)]  # noqa: E731
    grads = dict(actor=pairs(gs[:2 * L]), critic=pairs(gs[2 * L:]), log_std=gs[-1])
    per_member = sum(t.numel() for t in pop.tensors) // P

    # the torch forms work on their own copies of the parameters, with the same gradients
    def copies():
        ps = [t.clone() for t in pop.tensors]
        for p, x in zip(ps, gs):
            p.grad = x.clone()  # (clip_grad_norm_ scales .grad in place: every form owns its gradients; all forms pay the same)
        return ps
    fused_p = copies()
    fused_opt = torch.optim.Adam(fused_p, lr=LR, betas=BETAS, eps=EPS, fused=True)
    comp_p = copies()
    comp_m, comp_v = [torch.zeros_like(p) for p in comp_p], [torch.zeros_like(p) for p in comp_p]
    shape = lambda p: (P,) + (1,) * (p.dim() - 1)  # noqa: E731
    lr_t, b1_t, b2_t, eps_t, mx_t = (torch.full((P,), v, device=dev) for v in (LR, BETAS[0], BETAS[1], EPS, MAX_NORM))
    b1pow, b2pow = torch.ones(P, device=dev, dtype=torch.float64), torch.ones(P, device=dev, dtype=torch.float64)
    loop_p = copies()
    views = [[p[m] for p in loop_p] for m in range(P)]
    for m in range(P):
        for v, p in zip(views[m], loop_p):
            v.grad = p.grad[m]
    loop_opts = [torch.optim.Adam(views[m], lr=LR, betas=BETAS, eps=EPS, fused=True) for m in range(P)]

    def adam_step():
        env.adam_step_torch(opt, grads)

    def fused():
        torch.nn.utils.clip_grad_norm_(fused_p, MAX_NORM)
        fused_opt.step()

    def composed():
        with torch.no_grad():
            norm = torch.sqrt(sum((p.grad.double() ** 2).reshape(P, -1).sum(1) for p in comp_p)).float()
            scale = torch.clamp(mx_t / (norm + 1e-6), max=1.0)
            b1pow.mul_(b1_t.double())
            b2pow.mul_(b2_t.double())
            step_size = (lr_t.double() / (1 - b1pow)).float()
            bc2s = torch.sqrt(1 - b2pow).float()
            for p, m, v in zip(comp_p, comp_m, comp_v):
                s = shape(p)
                gc = p.grad * scale.reshape(s)
                m.mul_(b1_t.reshape(s)).add_((1 - b1_t).reshape(s) * gc)
                v.mul_(b2_t.reshape(s)).add_((1 - b2_t).reshape(s) * gc * gc)
                p.sub_(step_size.reshape(s) * m / (v.sqrt() / bc2s.reshape(s) + eps_t.reshape(s)))

    def loop():
        for m in range(P):
            torch.nn.utils.clip_grad_norm_(views[m], MAX_NORM)
            loop_opts[m].step()

    # agreement before timing: one step of the composed form against one adam_step_torch, from equal parameters
    composed()
    adam_step()
    agree = max(float((a - b).abs().max()) for a, b in zip(pop.tensors, comp_p))
    top = max(float((a - b).abs().max()) for a, b in zip(pop.tensors, loop_p))  # (loop_p still holds the initial parameters)
    us = alternating(dict(adam_step=(adam_step, 20), fused=(fused, 10), composed=(composed, 5), loop=(loop, max(1, 8 // P))))
    skipped = int(opt.state[:, 3].sum().item())
    mb = P * per_member * BYTES_PER_PARAMETER / 1e6
    return dict(env_id=ENV_ID, members=P, parameters_per_member=per_member, tensors=len(pop.tensors), traffic_mb=round(mb, 3),
                adam_step_us=us["adam_step"], fused_us=us["fused"], composed_us=us["composed"], loop_us=us["loop"],
                adam_over_composed=round(us["adam_step"][0] / us["composed"][0], 4), adam_over_loop=round(us["adam_step"][0] / us["loop"][0], 5),
                adam_over_fused=round(us["adam_step"][0] / us["fused"][0], 4), max_abs_diff_vs_composed=agree, max_abs_first_update=top,
                skipped=skipped)


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")] or [os.path.join(ROOT, "profiles", "adam_cost.txt")]
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, 256, device=0, seed=1)
    lines = ["Cost of the parameter update of a population: adam_step_torch against torch's fused Adam on the stacked tensors (other semantics:",
             "one norm, one learning rate), the per-member semantics composed in eager torch, and the loop of P optimizers over member views --",
             "the same tensors and gradients, timed in alternating windows of one run.  %s, tools/gpu_adam_cost.py; stream events around"
             % torch.cuda.get_device_name(0),
             "back-to-back calls after a warm-up, %d windows each; microseconds per update of ALL members: median [p10, p90], the host side of"
             % REPS,
             "every call included.",
             "Expected before the run: adam_step_torch flat in P up to where its traffic shows (32 B per parameter: 86 MB at P = 256, about",
             "11 us at 8 TB/s), under the composed form at every P, far under the loop for P >= 4.", "",
             "%s, every member an actor and a critic of two hidden layers of %d, max_grad_norm %.1f" % (ENV_ID, HIDDEN, MAX_NORM)]
    row = lambda name, v: "  %-64s %10.2f  [%10.2f, %10.2f]" % (name, *v)  # noqa: E731
    recs = []
    for P in MEMBERS:
        rec = measure(env, P)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        lines += ["", "P = %d members x %d parameters in %d tensors (%.2f MB of traffic)" % (P, rec["parameters_per_member"], rec["tensors"], rec["traffic_mb"]),
                  row("adam_step_torch (two launches)", rec["adam_step_us"]),
                  row("clip_grad_norm_ + Adam(fused=True), stacked (other semantics)", rec["fused_us"]),
                  row("per-member semantics composed in eager torch", rec["composed_us"]),
                  row("loop of %d clip_grad_norm_ + Adam(fused=True) over member views" % P, rec["loop_us"]),
                  "  adam_step / composed = %.4f; adam_step / loop = %.5f; adam_step / fused = %.4f" % (
                      rec["adam_over_composed"], rec["adam_over_loop"], rec["adam_over_fused"]),
                  "  largest parameter difference to the composed form after one step %.2g (largest first update %.2g); skipped steps: %d"
                  % (rec["max_abs_diff_vs_composed"], rec["max_abs_first_update"], rec["skipped"])]
    base = recs[0]["adam_step_us"][0]
    flat = [r["members"] for r in recs if r["adam_step_us"][0] <= 1.5 * base]
    lines += ["", "Against the expectation: adam_step_torch within 1.5 x its P = 1 time for P in %s; under the composed form at %s; under a tenth of the"
              % (flat, "every P" if all(r["adam_over_composed"] < 1 for r in recs) else "P in %s ONLY" % [r["members"] for r in recs if r["adam_over_composed"] < 1]),
              "loop at P in %s (P >= 4 expected)." % [r["members"] for r in recs if r["adam_over_loop"] < 0.1]]
    env.check_status()
    env.close()
    for p in paths:
        os.makedirs(os.path.dirname(os.path.abspath(p)), exist_ok=True)
        with open(p, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
