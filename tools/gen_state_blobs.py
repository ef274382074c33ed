#!/usr/bin/env python3
"""Writes tests/golden/state_blobs.npz: save_state() blobs of every combination of the switchable blocks, taken from the library
the package loads (SPACEGYM_LIB: the build whose bytes are to be pinned, e.g. a parent commit's from tools/build_rev.sh).
Four ids (Goal without pl1, Goal with every column, Kepler without and with orbd) x episode statistics, normalization (obs and
reward), 3 reward profiles with mixed indices: 32 blobs of 5 envs.  5 is odd on purpose: the int32 length block is 20 bytes,
so every float64 block after it sits at an offset that is no multiple of 8.  Each handle is reset and stepped 25 times with
random actions under max_episode_steps=10 (episodes end, statistics move) before its blob is taken.  Every blob must round-trip
on that library -- loaded into a second handle with another seed, saved again, equal bytes -- or nothing is written.
    python tools/gen_state_blobs.py [out.npz]
Needs a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import space_gym_amd as sg  # noqa: E402

IDS = ("GoalContinuous2P-v0", "GoalContinuous4P-v0", "KeplerCircleOrbit-v0", "KeplerRandomOrbits-v0")
NUM_ENVS, STEPS, MAX_EPISODE_STEPS = 5, 25, 10
EPISODES, NORMALIZE, PROFILES = 1, 2, 4  # the bits of a combination (the blob's own flags word uses the same)
PROFILE_TABLES = {
    "Goal": [dict(survival_reward_scale=0.25), dict(goal_vel_reward_scale=1.5, danger_zone=0.3),
             dict(safety_reward_scale=2.0, goal_sparse_reward=7.0)],
    "Kepl": [dict(numerator_C=0.02), dict(rad_penalty_C=2.5, act_penalty_C=0.5), dict(numerator_C=0.05, act_penalty_C=0.125)],
}
PROFILE_INDEX = np.array([2, 0, 1, 1, 2], np.uint8)


def key(env_id, bits):
    return f"{env_id}_{bits}"


def make(env_id, bits, seed):
    kw = dict(device=0, seed=seed, max_episode_steps=MAX_EPISODE_STEPS, episode_statistics=bool(bits & EPISODES),
              normalize_obs=bool(bits & NORMALIZE), normalize_reward=bool(bits & NORMALIZE))
    if bits & PROFILES:
        kw["reward_profiles"] = PROFILE_TABLES[env_id[:4]]
    env = sg.make_vec(env_id, NUM_ENVS, **kw)
    if bits & PROFILES:
        env.set_env_profiles(PROFILE_INDEX)
    return env


def take(env_id, bits):
    env = make(env_id, bits, seed=100 + bits)
    env.reset()
    rng = np.random.default_rng(bits)
    for _ in range(STEPS):
        env.step(rng.uniform(-1, 1, (NUM_ENVS, 2)).astype(np.float32))
    blob = env.save_state()
    env.close()
    return blob


def round_trips(env_id, blob):
    other = sg.make_vec(env_id, NUM_ENVS, device=0, seed=999, max_episode_steps=MAX_EPISODE_STEPS)
    other.load_state(blob)
    again = other.save_state()
    other.close()
    return np.array_equal(again, blob)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "state_blobs.npz")
    blobs = {key(env_id, bits): take(env_id, bits) for env_id in IDS for bits in range(8)}
    failed = [k for k, blob in blobs.items() if not round_trips(k.rsplit("_", 1)[0], blob)]
    for k, blob in blobs.items():
        print(k, blob.size, "bytes", "ROUND TRIP FAILED" if k in failed else "ok", flush=True)
    if failed:
        sys.exit(f"no file written: {len(failed)} blobs do not round-trip on this library: {failed}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **blobs)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
