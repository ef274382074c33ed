"""GPU test of the host side's kernel selection: every (family, planets, steering) variant through every plan -- one-wave and
wave-pair step kernels, the wave-pair K-step kernel with and without a terminal list, the one-wave K-step kernel, K launches of
the step kernel -- without and with the identity reward profile (which routes through every *_profiled_kernel and changes
nothing).  All of them must give the bits of K one-wave steps, and rollout_kernel() must name what the plan launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K, EPISODE = 257, 12, 5  # a full tile of 256 and a ragged one; every env ends two episodes
ENV_IDS = ["GoalContinuous2P-v0", "GoalContinuous3P-v0", "GoalContinuous4P-v0", "KeplerCircleOrbit-v0"]
GOAL_QUEUE_DEPTH, KEPLER_PAIR_QUEUE_DEPTH = 3, 4

# (what runs, SPACEGYM_STEP_KERNEL, SPACEGYM_ROLLOUT_KERNEL, unfused, terminal list)
HANDLES = [("steps", "single", "pair", False, True),
           ("steps", "pair", "pair", False, True),
           ("rollout", "pair", "pair", False, True),
           ("rollout", "pair", "pair", False, False),
           ("rollout", "single", "single", False, True),
           ("rollout", "pair", "pair", True, True)]


def _kernel_name(env_id, steering, profiled, step, rollout, unfused):
    """the name sg_rollout_kernel prints for this handle"""
    goal = env_id.startswith("Goal")
    acc = "true" if steering == "acceleration" else "false"
    head = f"{env_id[len('GoalContinuous')]}, {acc}" if goal else acc
    fam, prof = "goal" if goal else "kepler", "_profiled" if profiled else ""
    if unfused or (profiled and rollout == "single"):  # (the one-wave K-step kernels have no profiled variant)
        return f"{fam}{'_pair' if step == 'pair' else ''}_step{prof}_kernel<{head}>"
    if rollout == "single":
        return f"goal_rollout_kernel<{head}, {GOAL_QUEUE_DEPTH}>" if goal else f"kepler_rollout_kernel<{head}>"
    if goal:
        return f"goal_pair_rollout{prof}_kernel<{head}, {GOAL_QUEUE_DEPTH}, false>"
    return f"kepler_pair_rollout{prof}_kernel<{head}, {KEPLER_PAIR_QUEUE_DEPTH}>"


def _bits(x):
    """floats as integers: NaN-free and -0.0 exact"""
    import torch
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _steps(env, acts):
    """K step_torch calls -> dict of [K, N, ...] tensors, and the terminal records (step, env, last observation) in order"""
    import torch
    D = env.obs_dim
    out = dict(obs=torch.empty((K, N, D), device="cuda"), reward=torch.empty((K, N), device="cuda"),
               done=torch.empty((K, N), dtype=torch.uint8, device="cuda"), trunc=torch.empty((K, N), dtype=torch.uint8, device="cuda"))
    tobs = torch.full((N, D), float("nan"), device="cuda")
    steps, envs, rows = [], [], []
    for t in range(K):
        env.step_torch(acts[t], out={k: v[t] for k, v in out.items()}, terminal_obs=tobs)
        i = torch.nonzero(out["done"][t]).flatten()
        steps.append(torch.full_like(i, t)); envs.append(i); rows.append(tobs[i].clone())
    return out, (torch.cat(steps).cpu().numpy(), torch.cat(envs).cpu().numpy(), torch.cat(rows).cpu().numpy())


def _rollout(env, acts, with_list):
    import torch
    D = env.obs_dim
    out = dict(obs=torch.empty((K, N, D), device="cuda"), reward=torch.empty((K, N), device="cuda"),
               done=torch.empty((K, N), dtype=torch.uint8, device="cuda"), trunc=torch.empty((K, N), dtype=torch.uint8, device="cuda"))
    term = env.terminal_list_torch(N * K) if with_list else None
    env.rollout_torch(acts, out["obs"], out["reward"], out["done"], out["trunc"], terminal=term)
    return out, env.terminal_records(term) if with_list else None


@pytest.mark.timeout(120)
@pytest.mark.parametrize("steering", [None, "acceleration"])
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_every_plan_of_a_variant_gives_the_bits_of_one_wave_steps(env_id, steering, monkeypatch):
    import torch
    import space_gym_amd as sg
    kw = dict(device=0, seed=31, max_episode_steps=EPISODE)
    if steering:
        kw["steering"] = steering

    def make(profiled, step, rollout, unfused):
        monkeypatch.setenv("SPACEGYM_STEP_KERNEL", step)
        monkeypatch.setenv("SPACEGYM_ROLLOUT_KERNEL", rollout)
        env = sg.make_vec(env_id, N, **kw, **(dict(reward_profiles=[{}]) if profiled else {}))
        if unfused:
            env.set_unfused_rollout(True)
        want = _kernel_name(env_id, steering, profiled, step, rollout, unfused)
        assert env.rollout_kernel(K) == want and env.rollout_kernel(1) == want, (env.rollout_kernel(K), env.rollout_kernel(1), want)
        return env

    base = make(False, "single", "pair", False)
    obs0 = base.reset_torch().clone()
    gen = torch.Generator(device="cuda").manual_seed(7)
    acts = torch.rand((K, N, 2), device="cuda", generator=gen) * 2 - 1
    want, want_term = _steps(base, acts)
    assert len(want_term[0]) > 0  # finished episodes: the terminal-list kernels have work
    base.check_status()
    base.close()
    for profiled in (False, True):
        for what, step, rollout, unfused, with_list in HANDLES:
            if (profiled, what, step) == (False, "steps", "single"):
                continue  # (the baseline itself)
            tag = (env_id, steering, profiled, what, step, rollout, unfused, with_list)
            env = make(profiled, step, rollout, unfused)
            assert torch.equal(_bits(env.reset_torch()), _bits(obs0)), tag
            got, term = _steps(env, acts) if what == "steps" else _rollout(env, acts, with_list)
            for k in ("obs", "reward", "done", "trunc"):
                assert torch.equal(_bits(got[k]), _bits(want[k])), tag + (k,)
            if term is not None:
                assert np.array_equal(term[0], want_term[0]) and np.array_equal(term[1], want_term[1]), tag
                assert np.array_equal(term[2].view(np.int32), want_term[2].view(np.int32)), tag
            env.check_status()
            env.close()
