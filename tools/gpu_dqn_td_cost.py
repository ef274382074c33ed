#!/usr/bin/env python3
"""Measurement: what the fused Double DQN TD update (dqn_td_grad_torch: sg_dqn_td_grad_device, three launches) costs at GoalDiscrete3-v0
with two hidden layers of 64 (relu), n = 4 096 and n = 65 536 rows, against the Double DQN update through autograd that
tools/gpu_dqn_cost.py measures as "update" -- two dqn_evaluate_raw_torch launches and the target in torch under no_grad, the Huber loss
on dqn_evaluate_torch's q_taken, backward() -- which is existing code, written here exactly as it stands there.
  * td:        dqn_td_grad_torch(online, target, batch), Double DQN, huber_delta 1, no weights, no per-row outputs
  * td_rows:   the same with importance weights and all five per-row outputs
  * autograd:  the composition above
  * learner:   dqn_update_torch: td_rows' call, adam_step_torch, the priority formula's torch ops left out (no prio), tau = 0.005
ROUNDS rounds alternate the three; within a round every figure is the median over 15 repetitions of 20 back-to-back calls between
stream events after a warm-up, the host side of every call included.  Reported per n: the median over the rounds and the spread over
the rounds (largest minus smallest round median) of each, microseconds, and whether td beats autograd by more than autograd's spread.
Each n runs in a child process of its own under a time limit.  One JSON line per n.

Expected, written down before the first run: the target launch is dqn_evaluate_kernel's frame with two nets in one launch, so
about 38 us (profiles/dqn_cost.txt) plus a second policy_net, ~50 us at either n; the backward and the reduction are dqn_grad_torch's
two launches with a few more flops at the head and eight statistics sums, ~146 us at 4 096 rows and ~334 us at 65 536.  So td should
cost about 195 us at 4 096 and 385 us at 65 536, against 275 us and 475 us for the autograd composition: 80 to 90 us less at either
size -- the third forward launch, one evaluate launch and the ten elementwise torch launches of the target and the loss.
    python tools/gpu_dqn_td_cost.py [out.jsonl]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID, HIDDEN, LIMIT_S, ROUNDS = "GoalDiscrete3-v0", 64, 300, 5
EXPECTED_US = {"td": {4096: 195.0, 65536: 385.0}, "autograd": {4096: 275.0, 65536: 475.0}}


def measure(n):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import space_gym_amd as sg
    from gpu_policy_cost import timed

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, n, device=0, seed=1)
    D = env.obs_dim
    mlp = lambda: torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), torch.nn.ReLU(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.ReLU(),
                                      torch.nn.Linear(HIDDEN, 6)).to(dev)
    pairs = lambda net: [(l.weight, l.bias) for l in net if isinstance(l, torch.nn.Linear)]
    online, target = mlp(), mlp()
    for p in target.parameters():
        p.requires_grad_(False)
    params = list(online.parameters())
    ho, ht = env.dqn_torch(net=pairs(online)), env.dqn_torch(net=pairs(target))
    obs = env.reset_torch().clone()
    next_obs = obs + 0.01 * torch.randn_like(obs)
    action = torch.randint(0, 6, (n,), device=dev, dtype=torch.int32)
    reward, discount = torch.randn(n, device=dev), torch.full((n,), 0.99, device=dev)
    batch = dict(obs=obs, action=action, reward=reward, next_obs=next_obs, terminated=torch.zeros(n, dtype=torch.uint8, device=dev), discount=discount)
    weight = torch.rand(n, device=dev)
    ev_out = dict(q_taken=torch.empty(n, device=dev), argmax=torch.empty(n, dtype=torch.int32, device=dev))
    rows = {k: torch.empty(n, device=dev) for k in ("td_error", "q_taken", "target", "q_next", "g")}
    huber = torch.nn.functional.smooth_l1_loss
    grads, stats = env.dqn_td_grad_torch(ho, ht, batch)

    def td():
        env.dqn_td_grad_torch(ho, ht, batch, out=grads, stats=stats)

    def td_rows():
        env.dqn_td_grad_torch(ho, ht, batch, weight=weight, rows=rows, out=grads, stats=stats)

    def autograd():  # tools/gpu_dqn_cost.py's fused_update, as it stands there
        for p in params:
            p.grad = None
        with torch.no_grad():
            a2 = env.dqn_evaluate_raw_torch(ho, next_obs, out=dict(argmax=ev_out["argmax"]))[3]
            t = reward + discount * env.dqn_evaluate_raw_torch(ht, next_obs, a2, out=dict(q_taken=ev_out["q_taken"]))[1]
        huber(env.dqn_evaluate_torch(ho, obs, action)[1], t).backward()

    autograd()
    td()
    torch.cuda.synchronize()
    agree = max(float((g - p.grad).abs().max()) for g, p in zip([t for pair in grads["net"] for t in pair], params))
    loss_diff = abs(float(stats[0]) - float(huber(env.dqn_evaluate_raw_torch(ho, obs, action)[1],
                                                  reward + discount * env.dqn_evaluate_raw_torch(ht, next_obs, ev_out["argmax"])[1])))
    # the learner step moves the parameters: measured last, on copies of the state it changes
    opt = env.adam_torch(ho, lr=1e-4)

    def learner():
        env.dqn_update_torch(ho, ht, opt, batch, weight=weight, rows=rows, grads=grads, stats=stats, tau=0.005)

    reps, inner = 15, 20
    rounds = {"td": [], "td_rows": [], "autograd": []}
    for _ in range(ROUNDS):
        for name, fn in (("td", td), ("autograd", autograd), ("td_rows", td_rows)):
            rounds[name].append(timed(fn, reps, inner)[0])
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, rounds=ROUNDS, max_abs_grad_diff_vs_autograd=agree, loss_diff_vs_autograd=loss_diff)
    for name, v in rounds.items():
        rec[name + "_us"] = round(float(np.median(v)), 2)
        rec[name + "_spread_us"] = round(float(max(v) - min(v)), 2)
        rec[name + "_rounds_us"] = v
    rec["learner_us"] = timed(learner, reps, inner)
    rec["saved_us"] = round(rec["autograd_us"] - rec["td_us"], 2)
    rec["beats_autograd_by_more_than_its_spread"] = bool(max(rounds["td"]) + rec["autograd_spread_us"] < min(rounds["autograd"]))
    rec["expected_us"] = dict(td=EXPECTED_US["td"][n], autograd=EXPECTED_US["autograd"][n])
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
