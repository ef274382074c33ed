#!/usr/bin/env python3
"""Measurement: what the fused TD critic update (q_td_grad_torch: sg_q_td_grad_device, three launches) costs at GoalContinuous3P-v0
with twin critics of two hidden layers of 64 (relu), n = 4 096 and n = 65 536 rows, against the same critic update through autograd as
tools/gpu_q_cost.py composes it -- q_evaluate_raw_torch on the target handle and the target in torch under no_grad, the two squared
losses on q_evaluate_torch's outputs, backward() -- on the same batch, in TD3's form (target smoothing, no entropy term), with the
factor 0.5 on the loss that makes the two forms one function.
  * td:        q_td_grad_torch(online, target, batch, next_action, noise=...), the squared loss, no weights, no per-row outputs
  * td_rows:   the same with importance weights and all nine per-row outputs
  * autograd:  the composition above
  * learner:   q_update_torch: td_rows' call, adam_step_torch, tau = 0.005 (no prio)
ROUNDS rounds alternate the three; within a round every figure is the median over 15 repetitions of 20 back-to-back calls between
stream events after a warm-up, the host side of every call included.  Reported per n: the median over the rounds and the spread over
the rounds (largest minus smallest round median) of each, microseconds, and whether td beats autograd by more than autograd's spread.
The two forms' parameter gradients are held to the float64 model of tests/q_td_model.py under the project's rule, 8 x max|G32seq - G64|
+ 1e-6 (1 + max|G64|) per tensor.  Each n runs in a child process of its own under a time limit.  One JSON line per n.

Expected, written down before the first run: the target launch is q_evaluate_kernel's frame on both critics, 89 us at either n
(profiles/q_cost.txt) and a little more for a'; the backward and the reduction are q_grad_torch's two launches without the walk's last
step to the action (273 / 593 us with it, 188 / 375 us for that walk alone without the parameters' MFMA), so about 255 / 560 us.  td
should cost about 345 us at 4 096 rows and 650 us at 65 536.  The composition runs the same three net launches -- one more forward,
89 us, because autograd's forward is a launch of its own -- and about seventeen elementwise launches of some 6 us: about 535 us and
840 us.  So td should be some 190 us under it at either size.
    python tools/gpu_q_td_cost.py [out.jsonl]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID, HIDDEN, LIMIT_S, ROUNDS = "GoalContinuous3P-v0", 64, 400, 5
NOISE_STD, NOISE_CLIP, ACTION_CLIP = 0.2, 0.5, 1.0
EXPECTED_US = {"td": {4096: 345.0, 65536: 650.0}, "autograd": {4096: 535.0, 65536: 840.0}}


def measure(n):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import space_gym_amd as sg
    from gpu_policy_cost import timed
    import q_td_model

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, n, device=0, seed=1)
    D = env.obs_dim
    mlp = lambda: torch.nn.Sequential(torch.nn.Linear(D + 2, HIDDEN), torch.nn.ReLU(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.ReLU(),
                                      torch.nn.Linear(HIDDEN, 1)).to(dev)
    pairs = lambda net: [(l.weight, l.bias) for l in net if isinstance(l, torch.nn.Linear)]
    online, target = [mlp(), mlp()], [mlp(), mlp()]
    for net in target:
        for p in net.parameters():
            p.requires_grad_(False)
    params = [p for net in online for p in net.parameters()]
    ho, ht = env.q_torch(critics=[pairs(m) for m in online], activation="relu"), env.q_torch(critics=[pairs(m) for m in target], activation="relu")
    obs = env.reset_torch().clone()
    next_obs = obs + 0.01 * torch.randn_like(obs)
    action, next_action, noise = torch.randn((n, 2), device=dev).clamp(-1, 1), torch.randn((n, 2), device=dev).clamp(-1, 1), torch.randn((n, 2), device=dev)
    reward, discount = torch.randn(n, device=dev), torch.full((n,), 0.99, device=dev)
    terminated = (torch.rand(n, device=dev) < 0.1).to(torch.uint8)
    batch = dict(obs=obs, action=action, reward=reward, next_obs=next_obs, terminated=terminated, discount=discount)
    weight = torch.rand(n, device=dev)
    fwd = dict(q1=torch.empty(n, device=dev), q2=torch.empty(n, device=dev))
    rows = {k: torch.empty(n, device=dev) for k in env._Q_TD_ROWS}
    smooth = dict(noise=noise, noise_std=NOISE_STD, noise_clip=NOISE_CLIP, action_clip=ACTION_CLIP)
    grads, stats = env.q_td_grad_torch(ho, ht, batch, next_action, **smooth)

    def td():
        env.q_td_grad_torch(ho, ht, batch, next_action, out=grads, stats=stats, **smooth)

    def td_rows():
        env.q_td_grad_torch(ho, ht, batch, next_action, weight=weight, rows=rows, out=grads, stats=stats, **smooth)

    def autograd():  # tools/gpu_q_cost.py's critic step, with the target it takes as given formed the way a TD3 learner forms it
        for p in params:
            p.grad = None
        with torch.no_grad():
            a2 = (next_action + (NOISE_STD * noise).clamp(-NOISE_CLIP, NOISE_CLIP)).clamp(-ACTION_CLIP, ACTION_CLIP)
            t1, t2 = env.q_evaluate_raw_torch(ht, next_obs, a2, out=fwd)
            y = torch.where(terminated != 0, reward, reward + discount * torch.minimum(t1, t2))
        q1, q2 = env.q_evaluate_torch(ho, obs, action)
        (0.5 * ((q1 - y).square().mean() + (q2 - y).square().mean())).backward()
        return y

    y = autograd()
    td()
    torch.cuda.synchronize()
    flat_grads = [t for net in grads["critics"] for pair in net for t in pair]
    agree = max(float((g - p.grad).abs().max()) for g, p in zip(flat_grads, params))
    with torch.no_grad():
        q1, q2 = env.q_evaluate_raw_torch(ho, obs, action)
        loss_diff = abs(float(stats[0]) - float(0.5 * ((q1 - y).square().mean() + (q2 - y).square().mean())))
    # both forms' gradients against the float64 model, under the rule of DESIGN section 18
    host = lambda t: t.detach().cpu().numpy()
    nets = lambda ms: [[(host(w), host(b)) for w, b in pairs(m)] for m in ms]
    nb = {k: host(v) for k, v in batch.items()}
    kw = dict(next_action=host(next_action), noise=host(noise), noise_std=NOISE_STD, noise_clip=NOISE_CLIP, action_clip=ACTION_CLIP)
    g64, g32 = (q_td_model.flat(q_td_model.td(nets(online), nets(target), nb, dtype=dt, **kw)) for dt in (np.float64, np.float32))
    worst = {"td": 0.0, "autograd": 0.0}
    for (name, ref), g, p in zip(g64.items(), flat_grads, params):
        tol = 8.0 * float(np.abs(g32[name].astype(np.float64) - ref).max()) + 1e-6 * (1.0 + float(np.abs(ref).max()))
        worst["td"] = max(worst["td"], float(np.abs(host(g).astype(np.float64) - ref).max()) / tol)
        worst["autograd"] = max(worst["autograd"], float(np.abs(host(p.grad).astype(np.float64) - ref).max()) / tol)
    # the learner step moves the parameters: measured last
    opt = env.adam_torch(ho, lr=1e-4)

    def learner():
        env.q_update_torch(ho, ht, opt, batch, next_action, weight=weight, rows=rows, grads=grads, stats=stats, tau=0.005, **smooth)

    reps, inner = 15, 20
    rounds = {"td": [], "td_rows": [], "autograd": []}
    for _ in range(ROUNDS):
        for name, fn in (("td", td), ("autograd", autograd), ("td_rows", td_rows)):
            rounds[name].append(timed(fn, reps, inner)[0])
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, n_critics=2, rounds=ROUNDS, max_abs_grad_diff_vs_autograd=agree,
               loss_diff_vs_autograd=loss_diff, worst_grad_error_over_tolerance=worst,
               gradients_within_the_rule=bool(max(worst.values()) <= 1.0))
    for name, v in rounds.items():
        rec[name + "_us"] = round(float(np.median(v)), 2)
        rec[name + "_spread_us"] = round(float(max(v) - min(v)), 2)
        rec[name + "_rounds_us"] = v
    rec["learner_us"] = timed(learner, reps, inner)
    rec["saved_us"] = round(rec["autograd_us"] - rec["td_us"], 2)
    rec["beats_autograd_by_more_than_its_spread"] = bool(max(rounds["td"]) + rec["autograd_spread_us"] < min(rounds["autograd"]))
    rec["expected_us"] = dict(td=EXPECTED_US["td"][n], autograd=EXPECTED_US["autograd"][n])
    rec["expectation_held_within_10_percent"] = {k: bool(abs(rec[k + "_us"] - EXPECTED_US[k][n]) <= 0.1 * EXPECTED_US[k][n]) for k in EXPECTED_US}
    env.check_status()
    env.close()
    return rec


def main():
    if "--n" in sys.argv:  # the child: one n
        print(json.dumps(measure(int(sys.argv[sys.argv.index("--n") + 1]))), flush=True)
        return 0
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    for n in (4096, 65536):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(n)], stdout=subprocess.PIPE, text=True, timeout=LIMIT_S)
        if done.returncode != 0:  # nothing more is started on the device after a failure
            print(f"n = {n}: the measurement ended with status {done.returncode}", file=sys.stderr)
            return 1
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        for p in paths:
            with open(p, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
