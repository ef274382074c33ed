/*
 * spacegym.h -- C ABI of the MI355X batched Space-Gym step engine (libspacegym_hip.so).
 *
 * The reference (MIMUW-RL/space-gym) has no FFI; the seam this library sits behind is its gym.Env
 * protocol.  Each entry point names the reference interface it replaces (paths under the reference
 * repo root).  One handle advances `num_envs` independent (ship, planets, goal/orbit) instances in
 * lock-step on one GPU; envs never interact (gym_space/dynamic_model.py:145-165 sums only an env's
 * own planets), so a multi-GPU job is one handle per device with disjoint `env_index_base`.
 *
 * Conventions
 *   - every function returns 0 on success or a negative SG_ERR_* code; sg_last_error() gives the text;
 *   - plain pointers and sizes only; "host" pointers are ordinary memory, "device" pointers are HIP
 *     device memory on the handle's GPU, owned by the caller;
 *   - no allocation, no host synchronisation and no host<->device copy inside the *_device calls:
 *     they only enqueue kernels on the given stream (hipGraph-capturable);
 *   - the host-buffer calls (sg_reset, sg_reset_masked, sg_step, sg_get_state, sg_set_state, sg_vector_field, sg_save_state, sg_load_state,
 *     sg_seed, sg_set_auto_reset, sg_set_episode_stats, sg_step_episodes, sg_set_normalize, sg_get_normalize_state,
 *     sg_set_normalize_state, sg_render, sg_gae) run on the handle's own stream, wait for whatever the *_device calls have enqueued on
 *     the caller's streams before, and return when they are complete -- no manual synchronisation between the two kinds;
 *   - a handle is not thread-safe; independent handles are.
 *   - observations/rewards are float32 (the reference returns float64; parity tolerance in DESIGN.md).
 */
#ifndef SPACEGYM_H
#define SPACEGYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_OK 0
#define SG_ERR_INVALID -1   /* bad argument / unknown env id */
#define SG_ERR_HIP -2       /* HIP runtime error (message has the HIP text) */
#define SG_ERR_NO_DEVICE -3 /* no usable GPU: the engine has no CPU path */

typedef struct sg_env sg_env; /* opaque handle */

typedef struct sg_config {
    /* Registered id, as in gym_space/__init__.py:26-146: GoalContinuous{2,3,4}P-v0,
     * Kepler{CircleOrbit,EllipseEasy,EllipseHard,RandomOrbits}-v0; and the discrete-action ids of keyboard_agent.py:10-74:
     * GoalDiscrete{2,3,4}-v0, KeplerDiscrete-v0. */
    char env_id[64];
    int64_t num_envs;          /* batch on this device */
    uint64_t seed;             /* SpaceshipEnv.seed, spaceship_env.py:92-94 / goal.py:74-77 */
    uint32_t env_index_base;   /* global index of local env 0; the RNG is keyed by the global index */
    int32_t max_episode_steps; /* 0 -> the id's registered value (500): gym TimeLimit, __init__.py:29 */
    int32_t auto_reset;        /* 1: finished envs restart inside step (VectorEnv semantics); 0: they keep
                                  their terminal state, like a bare reference env */
    int32_t steering;          /* 0: Steering.velocity, what every registered id passes (ship_steering=1, __init__.py:32);
                                  1: Steering.acceleration (ship_steering=0, the constructor default of GoalEnv / KeplerEnv:
                                  goal.py:27, kepler.py:198): omega is integrated, the thruster is a torque
                                  (dynamic_model.py:138-141,160-161) and the angular-velocity event (:210-212) is live */
} sg_config;

/* The keyword arguments of the reference's constructors, GoalEnv.__init__ (gym_space/envs/goal.py:18-31) and
 * KeplerEnv.__init__ (gym_space/envs/kepler.py:189-203), on top of what gym_space/__init__.py:26-146 registers for the id --
 * what gym.make(id, **kwargs) does.  sg_params_init() sets every field to "keep the id's registered value" (NaN; the integers
 * -1); set the ones to override.  ship_steering is sg_config.steering; fixed_position, reward_value and renderer_kwargs are
 * read by nothing on the step path of the reference and have no field.  Keywords of the other family are refused, as Python
 * refuses an unexpected keyword argument. */
typedef struct sg_params {
    uint32_t struct_size;          /* sizeof(sg_params), set by sg_params_init */
    int32_t n_planets;             /* GoalEnv: 2, 3 or 4 (goal.py:25; 1 is a different sampler, :78-107, not served) */
    int32_t randomize;             /* KeplerEnv: 0 / 1 (kepler.py:191,257-259: a new reference orbit every episode) */
    int32_t reserved;
    /* GoalEnv._reward, goal.py:147-158 */
    double goal_vel_reward_scale;  /* goal.py:20,49 (x _distance_fctr = 100, :16,163) */
    double safety_reward_scale;    /* goal.py:21,51 (x 100, :226) */
    double goal_sparse_reward;     /* goal.py:22,50,155 */
    double survival_reward_scale;  /* goal.py:25,48,150 */
    double danger_zone;            /* goal.py:24,32,221: the safety term acts within this distance of the nearest planet's surface */
    /* KeplerEnv._dense_reward5, kepler.py:111-150 */
    double ref_orbit_a, ref_orbit_eccentricity, ref_orbit_angle; /* kepler.py:192-194 */
    double numerator_C, rad_penalty_C, act_penalty_C;             /* kepler.py:196-198,138-150 */
    double step_size;              /* kepler.py:199 (the constructor default is 0.1, every registered id passes 0.07); GoalEnv's is
                                      fixed at 0.07 (goal.py:66).  Up to 0.072 the env-step is one Nystrom step with the thrust in
                                      closed form; longer ones go through the Dormand-Prince kernels; refused where the heading
                                      could advance by more than pi / 4 within one env-step (Steering.velocity: above 0.157) */
    /* ShipParams (goal.py:45-47, kepler.py:207-209) */
    double ship_moi;               /* moment of inertia (Steering.acceleration only: dynamic_model.py:160-161) */
    double max_engine_force;       /* dynamic_model.py:171; 0 .. 4 */
} sg_params;
void sg_params_init(sg_params *params);

/* GoalContinuousEnv(**kwargs) / KeplerContinuousEnv(**kwargs) construction (goal.py:18-72,
 * kepler.py:189-231) for num_envs instances on GPU `device`: sg_create with the kwargs the id was registered with
 * (gym_space/__init__.py:26-146), sg_create_ex with `params` on top of them (NULL: none).
 * num_envs is at most 4 194 304 per handle (the episode queue of the rollout kernels is addressed by 32-bit offsets); larger
 * batches are several handles with disjoint env_index_base.  Besides its device columns (~100-490 B per env) a handle owns two
 * page-locked result blocks for sg_step_begin / sg_step_end of (2 obs_dim + 1.5) * 4 B per env each. */
int sg_create(const sg_config *cfg, int device, sg_env **out);
int sg_create_ex(const sg_config *cfg, const sg_params *params, int device, sg_env **out);
/* The parameters a handle was built with, every field filled in (the effective values). */
int sg_get_params(const sg_env *env, sg_params *out);
int sg_destroy(sg_env *env);
/* The same for a batch of cfg->num_envs envs cut into contiguous blocks over n_devices GPUs (one handle per device, the
 * remainder spread over the first ones; env_index_base of block k = cfg->env_index_base + its first env): envs never
 * interact (gym_space/dynamic_model.py:145-165) and the RNG is keyed by the global env index, so the blocks together are the
 * same envs as one handle of the whole batch.  handles_out has n_devices entries; on failure none is left allocated.  The
 * exchange a single-process VectorEnv view needs on top (a rooted gather of obs | reward | done per step) is
 * space_gym_amd/sharded.py's, over torch.distributed (RCCL). */
int sg_create_sharded(const sg_config *cfg, int n_devices, const int *devices, sg_env **handles_out);
int sg_create_sharded_ex(const sg_config *cfg, const sg_params *params, int n_devices, const int *devices, sg_env **handles_out);
const char *sg_last_error(const sg_env *env); /* env may be NULL: last error of a failed sg_create */

int64_t sg_num_envs(const sg_env *env);
int32_t sg_obs_dim(const sg_env *env);      /* 7 + 2N + 2 (Goal, spaceship_env.py:102-111,124-131); 10 (Kepler, kepler.py:158-187) */
int32_t sg_num_planets(const sg_env *env);  /* planets with a per-env position: N (Goal), 0 (Kepler) */
int32_t sg_discrete_actions(const sg_env *env); /* 1 for the ids with Discrete(6) actions (spaceship_env.py:184-187) */

/* SpaceshipEnv.seed (spaceship_env.py:92-94): takes effect at the next reset. */
int sg_seed(sg_env *env, uint64_t seed);
int sg_set_auto_reset(sg_env *env, int32_t on);

/* SpaceshipEnv.reset (spaceship_env.py:59-66) for every env; obs is float32 [num_envs, obs_dim]. */
int sg_reset(sg_env *env, float *obs_host);
int sg_reset_device(sg_env *env, float *obs_dev, void *hip_stream);

/* SpaceshipEnv.reset for the envs whose mask byte is nonzero (what auto-reset would start next for each of them);
 * rows of obs of the other envs are left untouched.  mask uint8 [num_envs], obs float32 [num_envs, obs_dim].
 * gymnasium's reset(options={"reset_mask": mask}) / envpool's reset(env_id) / reset_idx, for a loop with auto_reset off.
 * Env i with a nonzero byte starts episode e = (its episode counter) + 1 -- the one auto-reset would start, the one a full
 * sg_reset starts -- from the reset sampler keyed by (seed, env_index_base + i, e), bit-identical to what auto-reset would write
 * (the step kernels' own restart code); its elapsed counter goes to 0, its episode queue (rollout kernels) is emptied and
 * row i of obs receives the episode's first observation.  Envs with byte 0: no column, counter or obs row changes.
 *   episode statistics (on): the masked envs' running return and length go back to 0; the abandoned episodes give no record;
 *   normalization (on): the observation statistics are updated with the masked rows only (a batch of popcount(mask) rows; none:
 *     no update), then those rows are normalized; update = 0 only normalizes; the returns and their statistics stay;
 *   rendering: a masked env's trace starts afresh (its episode changed), the other envs' traces stay;
 *   event counters count nothing.
 * Refused (SG_ERR_INVALID) on a handle not reset since sg_create / sg_seed.  sg_reset_masked_device enqueues a few kernels and
 * allocates nothing (hipGraph-capturable); sg_reset_masked (host arrays) sends obs up and back, so its other rows come back as
 * they were. */
int sg_reset_masked(sg_env *env, const uint8_t *mask_host, float *obs_host);
int sg_reset_masked_device(sg_env *env, const uint8_t *mask_dev, float *obs_dev, void *hip_stream);

/* SpaceshipEnv.step (spaceship_env.py:68-78) for every env, plus what gym.wrappers.TimeLimit and a
 * VectorEnv add around it (elapsed-step counter, truncation, auto-reset).
 *   actions     continuous ids: float32 [num_envs, 2] raw policy output in [-1, 1]^2 (clamped into range on the device;
 *               the reference asserts, spaceship_env.py:71); discrete ids: int32 [num_envs] indices 0..5
 *               (spaceship_env.py:183-202; out-of-range indices act as 0, the reference raises ValueError)
 *   obs         float32 [num_envs, obs_dim]; for a finished env (auto_reset on) the first observation of
 *               its next episode
 *   reward      float32 [num_envs]
 *   done        uint8   [num_envs]  terminal event or truncation
 *   truncated   uint8   [num_envs]  elapsed == max_episode_steps without a terminal event ("TimeLimit.truncated")
 *   terminal_obs  optional float32 [num_envs, obs_dim]; rows of finished envs receive the last observation of
 *               the episode that ended, other rows are left untouched.  May be NULL. */
int sg_step(sg_env *env, const void *actions_host, float *obs_host, float *reward_host, uint8_t *done_host,
            uint8_t *truncated_host, float *terminal_obs_host);
int sg_step_device(sg_env *env, const void *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                   uint8_t *truncated_dev, float *terminal_obs_dev, void *hip_stream);

/* The same step in two halves, for callers that have something else to do while it runs -- gym.vector's
 * step_async() / step_wait() around SpaceshipEnv.step (spaceship_env.py:68-78).
 *   sg_step_begin  enqueues, on the handle's stream, the step kernel with a page-locked result block owned by the handle as
 *                  its output (the kernel stores across PCIe itself: no copy commands behind it), and returns without
 *                  waiting.  `actions_host` must stay unchanged until sg_step_end: page-locked memory (sg_host_alloc) is
 *                  read by the kernel where it is, anything else is copied to the device first.  want_terminal_obs != 0 adds the terminal observations to the block (rows of envs that did
 *                  not finish read NaN).
 *   sg_step_end    waits for that step and returns pointers into its result block: obs [num_envs, obs_dim], reward, done,
 *                  truncated as in sg_step, terminal_obs or NULL (any out pointer may be NULL).  The handle alternates
 *                  between two blocks: the pointers stay valid until the sg_step_begin after next -- the results of step t can
 *                  be read while step t + 1 is in flight, and the kernel enqueued by the sg_step_begin of step t + 2 writes
 *                  them again (it stores into the block while it runs).
 * One step may be in flight per handle; any other call on the handle between the two is ordered behind the step. */
/* (The two result blocks are allocated by the first sg_step_begin -- callers of the device-pointer entry points never pay for
 *  them; where device-mapped page-locked memory of that size cannot be had the handle falls back to a device block and copies.
 *  Whether `actions_host` is page-locked is asked on every call.  If sg_step_end fails the step is no longer in flight: the
 *  handle accepts the next sg_step_begin.) */
int sg_step_begin(sg_env *env, const void *actions_host, int32_t want_terminal_obs);
int sg_step_end(sg_env *env, const float **obs, const float **reward, const uint8_t **done, const uint8_t **truncated,
                const float **terminal_obs);

/* `n_steps` consecutive steps for pre-supplied actions (open-loop rollout, e.g. random-action benchmarking or replaying an
 * action tape): actions [n_steps, num_envs, 2] (discrete ids: int32 [n_steps, num_envs]), obs [n_steps, num_envs, obs_dim], reward/done/truncated [n_steps, num_envs].
 * Bit-identical to n_steps calls of sg_step_device.  All steps run in ONE kernel launch with the env state held in
 * registers; sg_set_unfused_rollout(env, 1) switches to n_steps launches of the step kernel. */
int sg_rollout_device(sg_env *env, int32_t n_steps, const void *actions_dev, float *obs_dev, float *reward_dev,
                      uint8_t *done_dev, uint8_t *truncated_dev, void *hip_stream);
int sg_set_unfused_rollout(sg_env *env, int32_t on);

/* The same rollout, also returning what a finished env's LAST observation was: in obs[t] a finished env already shows the
 * first observation of its next episode (VectorEnv convention), so the observation SpaceshipEnv.step returned with
 * done=True (spaceship_env.py:75-78) -- needed to bootstrap from truncated episodes -- would otherwise be lost.  One record
 * per finished env-step is appended to the list, in no particular order (device memory, owned by the caller):
 *   count     uint32 [1]            records appended by this call (set to 0 first); it keeps counting past `capacity`, the
 *                                   excess records are dropped -- size the list for n_steps * num_envs * (finish rate ~2 %)
 *   step_env  int32  [capacity, 2]  (step within this call, env index) of each record
 *   obs       float32 [capacity, obs_dim]
 * With auto_reset off nothing is appended (obs[t] is the terminal observation itself). */
typedef struct sg_terminal_list {
    uint32_t *count;
    int32_t *step_env;
    float *obs;
    uint32_t capacity;
} sg_terminal_list;
int sg_rollout_device_terminal(sg_env *env, int32_t n_steps, const void *actions_dev, float *obs_dev, float *reward_dev,
                               uint8_t *done_dev, uint8_t *truncated_dev, const sg_terminal_list *list, void *hip_stream);

/* The wave-pair rollout kernels bound every wait between their waves; a wait that runs out (never, on working hardware)
 * invalidates that rollout and is recorded on the handle: every later call on the handle then fails with SG_ERR_HIP until
 * sg_check_status -- which waits for the work enqueued so far, reports the condition and clears it -- has been called. */
int sg_check_status(sg_env *env);

/* Event counters of a handle (SURVEY section 5 "metrics"; the reference itself only keeps KeplerEnv's last penalties as
 * attributes, kepler.py:146-149): env-steps taken, episodes finished (terminal event or truncation), truncations
 * (gym.wrappers.TimeLimit), goals reached (GoalEnv._reward's `goal_pos` test, goal.py:154-157; 0 for the Kepler ids) since
 * counting was switched on or last reset.  Off by default -- the step and rollout kernels then do nothing for it; on, every
 * step / rollout call is followed by a pass over the done / truncated flags it wrote, and the reward code adds its goal hits. */
typedef struct sg_counters {
    uint64_t env_steps, episodes_finished, truncations, goal_hits;
} sg_counters;
/* (All four are counted on the device by the work the calls enqueue, so a replayed hipGraph of *_device calls counts as
 *  well; switching the counters on or off after a graph was captured does not change that graph.) */
int sg_set_counters(sg_env *env, int32_t on);                              /* switching (on or off) zeroes the counters */
int sg_get_counters(sg_env *env, sg_counters *out, int32_t reset);         /* waits for the enqueued work first */

/* Episode statistics -- what gym.wrappers.RecordEpisodeStatistics (SB3 VecMonitor, info["episode"]) adds around a bare
 * SpaceshipEnv, which keeps none itself: per env the return (float64 sum of the step rewards since the episode began, added in
 * step order, one add per step: bit-identical to a float64 loop over the float32 rewards the calls return) and the length (steps
 * in the episode); both start again from zero after every step with done (a terminal event or a truncation; with auto_reset
 * off as well: every done row closes exactly one episode).  Off by default: nothing is allocated or launched for it then.  On,
 * the handle keeps the two running sums per env on the device (12 B per env; sg_reset / sg_reset_device and switching on or
 * off zero them, sg_set_state leaves them alone), and every stepping call -- sg_step, sg_step_device, sg_step_begin,
 * sg_rollout_device, sg_rollout_device_terminal and the *_episodes calls below -- is followed, on the same stream, by a pass
 * over the reward / done / truncated rows it wrote.  Calls that return no statistics still advance the sums (the episodes they
 * finish are dropped), so the sums never depend on which entry point stepped the env.  Captured graphs stay linear (one stream).
 * The *_episodes entry points fail with SG_ERR_INVALID while the statistics are off.  Switching them on or off invalidates the
 * pointers sg_step_end returned (the result blocks grow by the two rows) and is refused while a step is in flight. */
int sg_set_episode_stats(sg_env *env, int32_t on);
/* sg_step_device / sg_step plus the episodes finished in this step, as dense rows like terminal_obs: ep_return float64
 * [num_envs] and ep_length int32 [num_envs]; rows of envs with done receive the finished episode's return and length, other rows
 * are left untouched.  Device pointers (on hip_stream) / host pointers. */
int sg_step_device_episodes(sg_env *env, const void *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                            uint8_t *truncated_dev, float *terminal_obs_dev, double *ep_return_dev, int32_t *ep_length_dev,
                            void *hip_stream);
int sg_step_episodes(sg_env *env, const void *actions_host, float *obs_host, float *reward_host, uint8_t *done_host,
                     uint8_t *truncated_host, float *terminal_obs_host, double *ep_return_host, int32_t *ep_length_host);
/* With statistics on, the result block of sg_step_begin also carries the two rows (12 B per env more); sg_step_end_episodes
 * returns pointers to them for the step sg_step_end collected last, valid under the same rules as sg_step_end's: ep_return
 * float64 [num_envs], ep_length int32 [num_envs]; rows of envs that did not finish read NaN / -1. */
int sg_step_end_episodes(sg_env *env, const double **ep_return, const int32_t **ep_length);
/* The finished episodes of a rollout, one record per env-step with done, appended in no particular order (device memory, owned
 * by the caller), as sg_terminal_list:
 *   count      uint32 [1]            records appended by this call (set to 0 first); keeps counting past `capacity`, the excess
 *                                    records are dropped
 *   step_env   int32  [capacity, 2]  (step within this call, env index)
 *   ret        float64 [capacity]    the episode's return
 *   length     int32  [capacity]     its length
 *   truncated  uint8  [capacity]     1 if it ended by the time limit ("TimeLimit.truncated") */
typedef struct sg_episode_list {
    uint32_t *count;
    int32_t *step_env;
    double *ret;
    int32_t *length;
    uint8_t *truncated;
    uint32_t capacity;
} sg_episode_list;
/* sg_rollout_device (terminal == NULL) / sg_rollout_device_terminal plus the list of the episodes it finished. */
int sg_rollout_device_episodes(sg_env *env, int32_t n_steps, const void *actions_dev, float *obs_dev, float *reward_dev,
                               uint8_t *done_dev, uint8_t *truncated_dev, const sg_terminal_list *terminal,
                               const sg_episode_list *episodes, void *hip_stream);

/* Running normalization of observations and rewards -- gym 0.21's NormalizeObservation and NormalizeReward (gym/wrappers/
 * normalize.py; SB3 VecNormalize, CleanRL's PPO) around the vector env, on the device.  With RunningMeanStd(mean 0, var 1,
 * count 1e-4) and update(x [B, ...]) = { bm, bv = mean and variance (ddof 0) of x over axis 0, n = B; delta = bm - mean;
 * tot = count + n; mean += delta * n / tot; var = (var * count + bv * n + delta^2 * count * n / tot) / tot; count = tot }:
 *   observations (obs):  obs_rms.update(obs); obs = (obs - obs_rms.mean) / sqrt(obs_rms.var + epsilon) -- on every step
 *                        and every reset (the reset batch updates the observation statistics, nothing else);
 *   rewards (reward):    returns = returns * gamma + reward (float64 [B], one per env); return_rms.update(returns);
 *                        reward = reward / sqrt(return_rms.var + epsilon); returns[done] = 0 -- on every step, not on reset.
 * Decisions:
 *   - statistics and normalized values are float64; each output element is rounded to float32 once; the batch moments of
 *     the observations are taken over the float32 values promoted to float64 (more exact than NumPy's float32 np.mean);
 *   - `returns` is a separate multiply and add in float64 per step, in step order: bit-identical to that NumPy loop;
 *   - a K-step rollout updates K times, once per step row, in step order: exactly what K single steps give.  The reductions
 *     depend only on (num_envs, obs_dim), so every entry point and rollout kernel gives the same bits;
 *   - terminal observations (the dense terminal_obs rows of envs with done, sg_terminal_list records, the sg_step_begin block)
 *     are normalized with the statistics of their own step, after its update, and do not enter it (SB3 VecNormalize);
 *   - episode statistics and event counters see the raw rewards (RecordEpisodeStatistics inside the normalizers);
 *   - optional clipping after normalization to [-clip_obs, clip_obs] / [-clip_reward, clip_reward] (+inf: none, the default;
 *     SB3's clip_obs); update = 0 freezes statistics and returns (evaluation, SB3 training=False): outputs use the statistics
 *     as they are;
 *   - sg_reset / sg_seed keep the statistics and returns (as gym).  Switching normalization on from off starts them afresh;
 *     switching it off frees them; changing gamma / epsilon / clip / update or one of the two flags while on keeps them.
 * Every call that returns observations or rewards is normalized in place: sg_reset[_device], sg_step[_device], sg_step_begin /
 * sg_step_end (on the device block, before it is copied: the kernel no longer stores into page-locked memory itself),
 * sg_rollout_device[_terminal|_episodes] with every rollout plan.  Three kernels follow the call on its stream (per-workgroup
 * moments of every step row, the running update, the normalization in place); with normalization off nothing is launched or
 * allocated.  Scratch: about 16 (obs_dim + 1) B per 256 envs and step, allocated for one step when switched on and grown by the
 * first longer call outside stream capture (or sg_normalize_reserve): a call captured into a graph fails if it would need more.
 * A captured graph keeps the configuration it was captured with, and switching normalization off invalidates it. */
typedef struct sg_normalize {
    uint32_t struct_size;  /* sizeof(sg_normalize), set by sg_normalize_init */
    int32_t obs;           /* 1: NormalizeObservation */
    int32_t reward;        /* 1: NormalizeReward */
    int32_t update;        /* 1: the statistics advance (training); 0: frozen (evaluation) */
    double gamma;          /* NormalizeReward's discount, in [0, 1] (0.99) */
    double epsilon;        /* added to the variance under the square root (1e-8) */
    double clip_obs;       /* > 0; +inf: no clipping (default) */
    double clip_reward;    /* > 0; +inf: no clipping (default) */
} sg_normalize;
/* gym's defaults: obs = reward = update = 1, gamma 0.99, epsilon 1e-8, no clipping. */
void sg_normalize_init(sg_normalize *cfg);
/* cfg NULL, or obs and reward both 0: off.  Refused while a step is in flight. */
int sg_set_normalize(sg_env *env, const sg_normalize *cfg);
int sg_get_normalize(sg_env *env, sg_normalize *out);  /* obs = reward = 0 while off */
/* Grows the scratch for calls of up to n_steps steps now, so that such a call can be captured into a graph. */
int sg_normalize_reserve(sg_env *env, int32_t n_steps);
/* The running statistics, float64 host arrays (any pointer may be NULL to skip it): obs_mean / obs_var [obs_dim], obs_count,
 * ret_mean, ret_var, ret_count [1], returns [num_envs].  The getter waits for the enqueued work; the setter (NULL: keep) puts a
 * policy's statistics into an evaluation env.  Both fail with SG_ERR_INVALID while normalization is off. */
int sg_get_normalize_state(sg_env *env, double *obs_mean, double *obs_var, double *obs_count, double *ret_mean, double *ret_var,
                           double *ret_count, double *returns);
int sg_set_normalize_state(sg_env *env, const double *obs_mean, const double *obs_var, const double *obs_count,
                           const double *ret_mean, const double *ret_var, const double *ret_count, const double *returns);

/* render(mode="rgb_array") -- SpaceshipEnv.render (spaceship_env.py:80-90) with gym_space/rendering.py:15-182 -- for chosen envs
 * of the batch, drawn on the device: uint8 frames [n, size, size, 3] (HWC, row 0 the top, as gym's rgb_array).  The scene is the
 * reference's: planet outlines (rendering.py:79-86; Kepler: the planet and the border circle, kepler.py:204-206,215), the ship's
 * engine, exhaust with alpha = thrust, body, outline and centre (:88-132), the goal's x (:140-146), a procedural stand-in for
 * the torque image (assets/torque_img.png is not shipped, :53-54,134-138), the trace of the last positions (:21-22,158-165) and,
 * for the Goal ids (debug_mode, goal.py:71), the lidar lines (:72-76,170-182).  Lengths the reference gives in pixels are scaled
 * by size / 600 (MAX_SCREEN_SIZE, :11).  DESIGN section 11 states the scene, the rasterisation rules (fixed-point, integer
 * coverage) and the trace semantics; tests/render_model.py implements them in NumPy, bit for bit.
 *
 * The trace (Renderer.prev_ship_pos) lives in `capacity` slots: slot k of a call belongs to env_ids[k]; each call appends the
 * env's current position to it.  A slot starts empty again when its env id differs from its previous call's, when the env's
 * episode changed since (Renderer.reset on env.reset(), auto-reset inside the stepping calls included), or after sg_reset,
 * sg_reset_device, sg_set_state or sg_load_state.  The trace is presentation state: snapshots do not carry it.
 * With rendering off (the default) nothing is allocated or launched for it. */
typedef struct sg_render_config {
    uint32_t struct_size;  /* sizeof(sg_render_config), set by sg_render_config_init */
    int32_t capacity;      /* trace slots = most frames per call (1 .. 1048576) */
    int32_t trace_len;     /* num_prev_pos_vis (rendering.py:21); -1: the family's (Goal 30, Kepler 75, kepler.py:222); 0: no trace; <= 256 */
    int32_t debug_lidar;   /* -1: the family's (Goal 1, goal.py:71; Kepler 0); 1 is refused for Kepler, which has no lidar */
    double trace_decay;    /* prev_pos_color_decay (rendering.py:22) in [0, 1]; NaN: the family's (0.85 / 0.95, kepler.py:222) */
} sg_render_config;
/* capacity 1, every other field "the family's". */
void sg_render_config_init(sg_render_config *cfg);
/* cfg NULL: off, frees the slots.  Switching on (again) starts every slot empty.  Waits for the handle's enqueued work. */
int sg_set_render(sg_env *env, const sg_render_config *cfg);
/* n frames (n <= capacity) of the envs env_ids [n] (int32), size x size pixels (16 .. 2048), into frames [n, size, size, 3] uint8.
 * actions: the step's own layout for the whole batch ([num_envs, 2] float32, or [num_envs] int32 for the discrete ids), read for
 * the exhaust and the torque indicator of the frames' envs -- the last action, as the reference's last_action
 * (spaceship_env.py:73); NULL: none (thrust = torque = 0, as before the first step).
 * sg_render_device enqueues two kernels on the stream and allocates nothing (hipGraph-capturable); an env id outside the batch
 * gives a white frame and sets the handle's status word, which sg_check_status reports (SG_ERR_INVALID) and clears.  sg_render
 * (host arrays) refuses such ids up front. */
int sg_render_device(sg_env *env, int32_t n, const int32_t *env_ids_dev, const void *actions_dev, int32_t size,
                     uint8_t *frames_dev, void *hip_stream);
int sg_render(sg_env *env, int32_t n, const int32_t *env_ids_host, const void *actions_host, int32_t size, uint8_t *frames_host);

/* Reward profiles: different reward coefficients for different envs of one batch (reward-shaping sweeps, population-based
 * training, curricula, reward-weight randomization).  A profile is a set of values for the reference's reward-only constructor
 * keywords: Goal ids survival_reward_scale, goal_vel_reward_scale, safety_reward_scale, goal_sparse_reward, danger_zone
 * (goal.py:147-158,204-227); Kepler ids numerator_C, rad_penalty_C, act_penalty_C (kepler.py:111-150).  A field left NaN takes
 * the handle's own value; a keyword of the other family or an invalid value is refused with sg_create_ex's message.  Each
 * profile's derived constants are those of sg_create_ex with its keywords, so env i under profile p gives bit for bit what env
 * i of a handle created with p's keywords gives: the physics, resets, RNG and `done` do not depend on the profile.
 * A handle holds up to 256 profiles and one uint8 profile index per env (all 0 when switched on).  An index change applies
 * from the next env-step's reward, also in mid-episode (a curriculum that wants episode boundaries selects with `done` on the
 * device).  sg_reset, sg_seed and masked reset keep table and indices.  Episode statistics, counters and normalization see the
 * profiled rewards; rendering and sg_vector_field do not depend on them.  Every step entry point runs profiled step kernels,
 * sg_rollout_device* the profiled wave-pair K-step kernels.  Off by default: then
 * nothing is allocated or launched for them.  Snapshots taken while they are on carry table and indices (sg_save_state).
 * The multi-device Python front ends do not serve them. */
typedef struct sg_reward_profile {
    uint32_t struct_size;          /* sizeof(sg_reward_profile), set by sg_reward_profile_init */
    double survival_reward_scale;  /* Goal */
    double goal_vel_reward_scale;
    double safety_reward_scale;
    double goal_sparse_reward;
    double danger_zone;
    double numerator_C;            /* Kepler */
    double rad_penalty_C;
    double act_penalty_C;
} sg_reward_profile;
/* every field NaN: the handle's own values */
void sg_reward_profile_init(sg_reward_profile *p);
/* n = 0 (profiles NULL): off, frees table and indices.  1 <= n <= 256: uploads the table (waits for the handle's work).  Indices
 * are kept while profiles stay on; a table shorter than an index in use is refused. */
int sg_set_reward_profiles(sg_env *env, int32_t n, const sg_reward_profile *profiles);
/* *n = number of profiles (0: off); out (NULL to skip, else n entries) receives the effective values of every field of the
 * handle's family (the other family's stay NaN). */
int sg_get_reward_profiles(sg_env *env, int32_t *n, sg_reward_profile *out, int32_t capacity);
/* The env's profile index, uint8 [num_envs].  The host form refuses an index >= n.  The device form enqueues one kernel on the
 * stream and allocates and synchronizes nothing (hipGraph-capturable); an index >= n makes that env use profile 0 and sets the
 * handle's status word, which sg_check_status reports (SG_ERR_INVALID) and clears.  Both fail while profiles are off. */
int sg_set_env_profiles(sg_env *env, const uint8_t *idx_host);
int sg_set_env_profiles_device(sg_env *env, const uint8_t *idx_dev, void *hip_stream);
int sg_get_env_profiles(sg_env *env, uint8_t *idx_host);

/* On-device action source for sg_rollout_device: the uniformly random policy (what the reference's README loop and the
 * benchmark use: env.action_space.sample(), gym spaces Box / Discrete).  Fills actions_dev [n_steps, num_envs, 2] float32
 * with i.i.d. U(-1, 1) values (discrete ids: int32 [n_steps, num_envs] uniform in 0..5).  Entry (t, i) is a function of
 * (seed, env_index_base + i, first_step + t) only (Philox4x32-10), so it does not depend on how a job is sharded over
 * GPUs or cut into calls.  Enqueues one kernel on the stream. */
int sg_random_actions_device(sg_env *env, int32_t n_steps, uint64_t seed, uint64_t first_step, void *actions_dev, void *hip_stream);

/* State access (the reference exposes env._ship_state._state_vec, planet.center_pos, env.goal_pos as plain
 * attributes; golden-vector injection needs the same).  Host arrays, any may be NULL to skip:
 *   ship    float32 [num_envs, 6]   x, y, theta, vx, vy, omega   (dynamic_model.py:40)
 *   planets float32 [num_envs, N, 2]                              (Goal only)
 *   goal    float32 [num_envs, 2]   Goal: goal position; KeplerRandomOrbits: (ref_orbit_angle, ref_orbit_eccentricity)
 *   elapsed int32   [num_envs]      steps taken in the current episode */
int sg_get_state(sg_env *env, float *ship, float *planets, float *goal, int32_t *elapsed);
int sg_set_state(sg_env *env, const float *ship, const float *planets, const float *goal, const int32_t *elapsed);

/* Complete snapshot of a handle (checkpoint / restore), as an opaque blob of sg_state_bytes(env) bytes of host memory: every
 * per-env column -- ship, planets, goal / orbit, step and episode counters, and the tiling state HexagonalTiling keeps
 * between goal hits (hexagonal_tiling.py:99-128: free-tile list, ship / goal tile, column shifts) -- plus the RNG key.
 * Loading it into a handle of the same env id and batch size makes the following steps bit-identical to those that
 * followed the save.  While episode statistics are on the blob also carries the running return and length of every env
 * (sg_state_bytes grows by 12 B per env; with them off it is what it was before they existed); loading such a blob switches
 * the statistics on and resumes them bit-identically, loading one without them into a handle that has them on zeroes them.
 * While normalization is on the blob is header version 3: the version-1 columns, a flags word naming the blocks that follow
 * (episode statistics, normalization), then those blocks: the configuration, the running statistics and `returns`.  Loading it
 * switches normalization on with that configuration and resumes it bit-identically; loading a version-1 / 2 blob into a
 * handle with normalization on starts its statistics afresh and keeps the configuration.  With normalization off the blob is
 * byte for byte what it was before normalization existed.  While reward profiles are on the blob is version 3 with one more
 * block (the profiles as given and every env's index); loading it switches them on with that table and those indices, loading
 * one without them leaves a handle's profiles as they are. */
size_t sg_state_bytes(const sg_env *env);
int sg_save_state(sg_env *env, void *blob_host, size_t bytes);
int sg_load_state(sg_env *env, const void *blob_host, size_t bytes);

/* Device-resident snapshots: the per-env data of a handle in a buffer of the caller's in device memory (16-byte aligned, at
 * least sg_snapshot_bytes(env) bytes for the handle as it is configured now), for rollback, search and branching inside the
 * training loop (the reference: copy.deepcopy(env)).  Both calls enqueue on the caller's stream, allocate nothing, never
 * synchronise and are hipGraph-capturable; any number of snapshots of one handle can exist at once.
 * A snapshot holds: a 32-byte header written by the snapshot kernel (magic, family, n_planets, randomize_orbit, num_envs, a
 * flags word naming the optional blocks), then the per-env columns of the blob above (q0, q1, ctr, aux, pl0, pl1, cshift, orbd, as
 * the id has them); with episode statistics on the running return (float64) and length (int32) of every env; with
 * normalization on `returns` (float64).  Every block starts 16-byte aligned.  It does NOT hold the seed, the normalizer's
 * running mean / var / count, the reward-profile table or the per-env profile index: those are configuration and learning
 * state of the handle and stay as they are on restore (a restored env keeps the profile of its slot; copy the index with
 * sg_set_env_profiles[_device] for the other behaviour).
 * sg_restore_device: for every env i with mask_dev[i] != 0 (NULL: every env), with j = src_dev[i] (NULL: j = i), env i's
 * columns (and running episode statistics / returns when on) become those of the snapshot's env j; its episode queue is
 * emptied; with rendering on the traces of ALL slots start afresh at the next render call (also when a captured restore is
 * replayed); if obs_dev [num_envs, obs_dim] is given, row i becomes the observation of the restored state (normalized and
 * clipped with the statistics as they are when observation normalization is on; the statistics are not updated).  Nothing of
 * the other envs is written.  Episode counters are part of the state: done / truncated come out as they would have after the
 * snapshot; sg_get_counters totals are not rewound.  No RNG state is copied (the RNG is keyed by seed, global env index,
 * episode, block, stream): with j = i and the seed unchanged everything after the restore is bit-identical to what followed the
 * snapshot under the same actions; with j != i env i continues j's trajectory bit for bit until its next random draw (goal hit
 * or reset), which comes from its own stream -- what sg_load_state does with a blob whose columns were gathered on the host.
 * Duplicate sources are allowed.  A buffer that overlaps the handle's own memory is the caller's error.
 * Refused on the host (SG_ERR_INVALID, nothing enqueued): a null or misaligned buffer, bytes < sg_snapshot_bytes, a handle not
 * reset since sg_create / sg_seed, a step in flight.  Checked on the device, before anything is written: a header that does
 * not match the handle (other family, planets, batch size or blocks) restores nothing; a src_dev[i] outside [0, num_envs)
 * leaves env i as it is.  Both set the handle's status word: every later call on the handle fails with SG_ERR_HIP until
 * sg_check_status has reported the condition (SG_ERR_INVALID) and cleared it. */
size_t sg_snapshot_bytes(const sg_env *env);
int sg_snapshot_device(sg_env *env, void *snap_dev, size_t bytes, void *hip_stream);
int sg_restore_device(sg_env *env, const void *snap_dev, size_t bytes, const uint8_t *mask_dev, const int32_t *src_dev,
                      float *obs_dev, void *hip_stream);

/* Advantages and returns of a rollout by generalized advantage estimation (Schulman et al. 2016; SB3
 * RolloutBuffer.compute_returns_and_advantage, CleanRL's PPO) -- what an on-policy learner computes next from the rows
 * sg_rollout_device* wrote and its value estimates.  The reference has no counterpart.  For a rollout of K = n_steps steps of
 * B = num_envs envs, in the rollout's own layout:
 *   reward          float32 [K, B]   as returned (raw, profiled or normalized: whatever the caller passes)
 *   done, truncated uint8   [K, B]   as returned
 *   value           float32 [K, B]   V of the observation action t was taken from (the obs before the rollout for t = 0, obs[t - 1]
 *                                    after); NULL: all zero -- the advantage is then the discounted reward-to-go
 *   last_value      float32 [B]      V of obs[K - 1]; NULL: zero
 *   terminal values                  V of the LAST observation of the episode that ended at (t, i), in one of two forms (or neither):
 *     dense         float32 [K, B]   read only where done and truncated are both set;
 *     list          sg_value_list    a rollout's sg_terminal_list with the caller's V(obs[k]) beside it: the same count and
 *                                    step_env, `value` float32 [capacity], in any order
 *   advantage, ret  float32 [K, B]   outputs
 * Per env i, in float64, every operation rounded on its own (no fused multiply-add), gl = gamma * lambda rounded once on the host:
 *   A = 0
 *   for t = K - 1 .. 0:
 *       if done[t, i]:  nv = the terminal value of (t, i) if truncated[t, i] and bootstrap_truncated and terminal values are given,
 *                            else 0
 *                       A  = (reward[t, i] + gamma * nv) - value[t, i]               -- nothing crosses an episode boundary
 *       else:           nv = value[t + 1, i], or last_value[i] for t = K - 1
 *                       A  = ((reward[t, i] + gamma * nv) - value[t, i]) + gl * A
 *       advantage[t, i] = (float) A;  ret[t, i] = (float) (A + value[t, i])
 * With auto-reset on, value[t + 1] at a finished step belongs to the next episode and is never used; a truncated episode
 * bootstraps from the value of its own last observation, which is what sg_rollout_device_terminal's list is for.  A NaN or inf
 * inside one episode stays inside that episode.  The result depends on the arguments only: not on the handle's state or env id
 * (the handle gives B, the device and the status word).  tests/gae_model.py is the same recurrence in NumPy, bit for bit.
 * sg_gae_device enqueues on the caller's stream -- one kernel, or two with a list (the first scatters the list's values into
 * `advantage`, where the second reads each one before it overwrites it: no scratch) -- allocates nothing, never synchronises, is
 * hipGraph-capturable (one stream) and leaves every env untouched.  Pointers need only their type's alignment (rows of odd B,
 * views into larger buffers).  Inputs must not overlap the outputs.
 * Refused on the host (SG_ERR_INVALID, nothing enqueued): n_steps < 1; a null reward, done, truncated, advantage or ret; both
 * terminal forms at once; gamma or lambda outside [0, 1] or NaN; a wrong struct_size.  Checked on the device: a list whose count
 * exceeds its capacity (values are missing: those steps bootstrap from garbage) and a step_env record outside [0, K) x [0, B)
 * (ignored) set the handle's status word: every later call on the handle fails with SG_ERR_HIP until sg_check_status has reported
 * the condition (SG_ERR_INVALID) and cleared it.
 * sg_gae is the same for host arrays (a list's pointers are host pointers too), on the handle's stream like the other
 * host-buffer calls; it allocates a device block for the call and refuses a bad list up front. */
typedef struct sg_gae_config {
    uint32_t struct_size;         /* sizeof(sg_gae_config), set by sg_gae_config_init */
    double gamma;                 /* discount, in [0, 1] */
    double lambda;                /* GAE's lambda, in [0, 1] */
    int32_t bootstrap_truncated;  /* 1: a truncated episode bootstraps from its terminal value; 0: a truncation ends the episode
                                     like a terminal event (next value 0) and the terminal values are not read */
} sg_gae_config;
/* gamma 0.99, lambda 0.95, bootstrap_truncated 1 */
void sg_gae_config_init(sg_gae_config *cfg);
typedef struct sg_value_list {
    const uint32_t *count;    /* [1]: records in the list (sg_terminal_list.count of the rollout) */
    const int32_t *step_env;  /* [capacity, 2]: (step, env) of each record (sg_terminal_list.step_env) */
    const float *value;       /* [capacity]: V of the record's terminal observation */
    uint32_t capacity;
} sg_value_list;
/* cfg NULL: sg_gae_config_init's values */
int sg_gae_device(sg_env *env, int32_t n_steps, const sg_gae_config *cfg, const float *reward_dev, const uint8_t *done_dev,
                  const uint8_t *truncated_dev, const float *value_dev, const float *last_value_dev,
                  const float *terminal_value_dense_dev, const sg_value_list *terminal_value_list, float *advantage_dev,
                  float *ret_dev, void *hip_stream);
int sg_gae(sg_env *env, int32_t n_steps, const sg_gae_config *cfg, const float *reward_host, const uint8_t *done_host,
           const uint8_t *truncated_host, const float *value_host, const float *last_value_host,
           const float *terminal_value_dense_host, const sg_value_list *terminal_value_list, float *advantage_host, float *ret_host);

/* Return targets with PER-GROUP discounts read on the device, for populations whose members explore gamma or lambda and for schedules
 * inside a captured graph: GAE as above, and V-trace, the importance-corrected value target (Espeholt et al. 2018, IMPALA) for rollout
 * rows that the policy being updated did not generate (another member's env block, a later epoch over the same rollout).  Device calls
 * only; tests/returns_model.py is both recurrences in NumPy, bit for bit; DESIGN section 27 has the kernels.
 *   discounts  float32 DEVICE [groups, 2], row g = (gamma, lambda) of group g.  groups >= 1 divides num_envs and env i reads row
 *              i / (num_envs / groups): the population's block rule, so groups = members gives per-member discounts and groups = num_envs
 *              per-env discounts.  Read by the kernel at every launch, each lane its two floats once: a captured graph changes a discount
 *              by writing the tensor.  ITS VALUES ARE NOT CHECKED (as sg_adam_step_device's hyper): a NaN or a value outside [0, 1]
 *              affects the envs of that group only.  Per env, in float64: gamma = (double) row[0], gl = (double) row[0] * (double) row[1]
 *              (exact: two float32 factors), so a table whose rows are equal gives the bits of the scalar form at
 *              gamma = (double)(float) g, lambda = (double)(float) l.
 * sg_gae_groups_device is sg_gae_device -- its arguments, both terminal forms, bootstrap_truncated, a NULL value or last_value, its
 * recurrence, its list check through the status word, its guarantees (caller's stream, one launch or two, nothing allocated, no
 * synchronisation, hipGraph-capturable) -- with gamma and gl taken from the env's row.  groups >= 1 is required; cfg's gamma and lambda are
 * not read, its bars are checked and not used.
 * sg_vtrace_device adds
 *   ratio         float32 [K, B]   the caller's exp(log pi(a | x) - log mu(a | x)) of the target policy pi over the behaviour policy mu;
 *                                  NULL: on-policy, every ratio 1.  No exp runs on the device.
 *   value         float32 [K, B]   required
 *   vs            float32 [K, B]   output: the V-trace value targets
 *   pg_advantage  float32 [K, B]   output: the policy gradient's advantage, min(pg_rho_bar, ratio) (r + gamma vs[t + 1] - V)
 * and takes its discounts from the table (groups >= 1) or from cfg's gamma and lambda (groups = 0; gl = gamma * lambda rounded once on the
 * host).  Per env i, in float64, every operation rounded on its own (no fused multiply-add):
 *   acc = 0;  v_next = last_value[i] (0 if NULL)
 *   for t = K - 1 .. 0:
 *       rho = ratio[t, i] (1 if NULL)
 *       rc = rho_bar < rho ? rho_bar : rho;  cc likewise with c_bar;  rp likewise with pg_rho_bar     -- a NaN ratio stays NaN
 *       if done[t, i]:  term = the terminal value of (t, i) if truncated[t, i] and bootstrap_truncated and terminal values are given, else 0
 *                       nv = term;    vs_next = term
 *       else:           nv = v_next;  vs_next = v_next + acc
 *       delta = rc * ((reward[t, i] + gamma * nv) - value[t, i])
 *       acc   = done[t, i] ? delta : delta + (gl * cc) * acc                                           -- nothing crosses an episode boundary
 *       vs[t, i] = (float) (acc + value[t, i])
 *       pg_advantage[t, i] = (float) (rp * ((reward[t, i] + gamma * vs_next) - value[t, i]))
 *       v_next = value[t, i]
 * which is the paper's equation (1) with c_t = lambda min(c_bar, ratio).  With ratio NULL and the three bars >= 1, vs equals
 * sg_gae_device's ret bit for bit.  The list form scatters into vs, where the scan reads each value before it overwrites it.
 * Refused on the host (SG_ERR_INVALID, nothing enqueued): a null cfg, a wrong struct_size or reserved; n_steps < 1; a null reward, done,
 * truncated or output; both terminal forms at once; groups < 0, groups that do not divide num_envs, groups >= 1 with a null discounts;
 * with groups = 0, gamma or lambda outside [0, 1] or NaN (sg_gae_groups_device refuses groups = 0 itself); a bar that is <= 0 or NaN
 * (+inf: no clipping); a null value (sg_vtrace_device). */
typedef struct sg_returns_config {
    uint32_t struct_size;         /* sizeof(sg_returns_config), set by sg_returns_config_init */
    int32_t groups;               /* rows of discounts; 0: the scalars gamma and lambda below (sg_vtrace_device only) */
    const float *discounts;       /* DEVICE float32 [groups, 2]: (gamma, lambda) per group; not read when groups = 0 */
    double gamma;                 /* groups = 0: discount, in [0, 1] */
    double lambda;                /* groups = 0: the trace's lambda, in [0, 1] */
    int32_t bootstrap_truncated;  /* as sg_gae_config's */
    double rho_bar;               /* V-trace: clips the ratio of the temporal difference; > 0, +inf allowed */
    double c_bar;                 /* V-trace: clips the ratio of the trace; > 0, +inf allowed */
    double pg_rho_bar;            /* V-trace: clips the ratio of pg_advantage; > 0, +inf allowed */
    int32_t reserved;             /* 0 */
} sg_returns_config;
/* gamma 0.99, lambda 0.95, bootstrap_truncated 1, the three bars 1.0, groups 0 and a null discounts */
void sg_returns_config_init(sg_returns_config *cfg);
int sg_gae_groups_device(sg_env *env, int32_t n_steps, const sg_returns_config *cfg, const float *reward_dev, const uint8_t *done_dev,
                         const uint8_t *truncated_dev, const float *value_dev, const float *last_value_dev,
                         const float *terminal_value_dense_dev, const sg_value_list *terminal_value_list, float *advantage_dev,
                         float *ret_dev, void *hip_stream);
int sg_vtrace_device(sg_env *env, int32_t n_steps, const sg_returns_config *cfg, const float *reward_dev, const uint8_t *done_dev,
                     const uint8_t *truncated_dev, const float *value_dev, const float *last_value_dev, const float *ratio_dev,
                     const float *terminal_value_dense_dev, const sg_value_list *terminal_value_list, float *vs_dev,
                     float *pg_advantage_dev, void *hip_stream);

/* Retrace(lambda) and Q(lambda) targets over replayed sequences: what turns a sampled [L, n] sequence batch (sg_replay_sequence_device)
 * into multi-step, off-policy-corrected targets for Q(s_t, a_t) -- the action-value counterpart of sg_vtrace_device, for a DQN, an
 * R2D2-style or a SAC-critic learner (Munos et al. 2016, "Safe and efficient off-policy reinforcement learning").  Device call only;
 * tests/retrace_model.py is the recurrence and the loss outputs in NumPy, bit for bit; DESIGN section 35 has the kernel.
 * Unlike sg_vtrace_device it takes the column count n explicitly (1 .. 2^31 - 1, with length * n <= 2^31 - 1): a sequence batch is not
 * num_envs wide.  All arrays are time-major DEVICE tensors:
 *   reward          float32 [L, n]   required
 *   done, truncated uint8   [L, n]   required
 *   q               float32 [L, n]   required: Q(s_t, a_t) of the net the targets are built from (normally the target net)
 *   value           float32 [L, n]   required: V_pi(s_t) = E_{a ~ pi} Q(s_t, a) under the target policy
 *   last_value      float32 [n]      V_pi(s_L); NULL: zeros
 *   ratio           float32 [L, n]   the caller's per-step trace ratio; NULL: ones.  No exp runs on the device.
 *   terminal_value  float32 [L, n]   dense; read ONLY where done && truncated (sg_replay_sequence_device leaves terminal_obs unwritten
 *                                    elsewhere, so nothing else is read); NULL: a truncation bootstraps from 0
 *   target          float32 [L, n]   output, required
 *   q_online        float32 [L, n]   optional input: the online net's Q(s_t, a_t)
 *   weight          float32 [n]      optional input: per-sequence importance weights
 *   td_error        float32 [L, n]   optional output: q_online - target
 *   g               float32 [L, n]   optional output: the Huber loss' gradient by q_online (below); flattened, it is the g_taken of
 *                                    sg_dqn_grad_device / sg_q_grad_device
 * Per column i, in float64, every operation rounded on its own (no fused multiply-add):
 *   carry = 0;  v_next = last_value[i] (0 if NULL)
 *   for t = L - 1 .. 0:
 *       if done[t, i]:  boot = (truncated[t, i] && bootstrap_truncated && terminal_value) ? terminal_value[t, i] : 0
 *       else:           boot = v_next + carry
 *       G  = reward[t, i] + gamma * boot                                -- product rounded, then sum
 *       target[t, i] = (float) G
 *       rho = ratio ? ratio[t, i] : 1;   cc = c_bar < rho ? c_bar : rho    -- a NaN ratio stays NaN
 *       carry  = (lambda * cc) * (G - q[t, i])
 *       v_next = value[t, i]
 * which is the Retrace operator with c_t = lambda min(c_bar, ratio_t),
 *   G_t = r_t + gamma [V_pi(s_{t+1}) + c_{t+1} (G_{t+1} - Q(s_{t+1}, a_{t+1}))],
 * cut at episode ends and bootstrapped from last_value at the sequence's end.  ratio and c_bar pick the estimator; the kernel has no mode:
 *   Retrace(lambda)        ratio = pi / mu, c_bar = 1          tree backup(lambda)    ratio = pi(a_t | s_t)
 *   Peng's Q(lambda)       ratio = NULL                        Watkins' Q(lambda)     ratio = [a_t greedy]
 *   importance sampling    ratio = pi / mu, c_bar = inf        one-step TD            lambda = 0
 * Where td_error or g is given, in float32 with sg_dqn_td_grad_device's arithmetic:
 *   td = q_online[t, i] - target[t, i];  c = min(max(td, -huber_delta), huber_delta);  w = weight ? weight[i] : 1
 *   td_error[t, i] = td;  g[t, i] = (w * c) / (float)(L * n)              -- the product rounded, then the quotient
 * No statistics are written: the reductions stay with the caller or the TD calls.
 *   discounts  optional DEVICE float32 [2] of (gamma, lambda), read by the kernel at every launch -- a captured graph anneals both by
 *              writing the tensor.  ITS VALUES ARE NOT CHECKED.  The two floats are widened to float64 (exact); the recurrence has no
 *              gamma * lambda product, so the tensor form gives the bits of the scalar form at gamma = (double)(float) g, lambda
 *              likewise.  When it is given, cfg's gamma and lambda are not read.
 * One launch on the caller's stream: no workspace, no atomics, no LDS, nothing allocated, no synchronisation, hipGraph-capturable.  Every
 * load and store is one element per lane, so an odd n and views at odd offsets work.
 * Refused on the host (SG_ERR_INVALID, nothing enqueued): a null cfg, a wrong struct_size or a non-zero reserved; length < 1, n < 1,
 * length * n > 2^31 - 1; a null reward, done, truncated, q, value or target; with a null discounts, gamma or lambda outside [0, 1] or NaN;
 * c_bar or huber_delta <= 0 or NaN (+inf allowed: no clipping, the squared loss); td_error or g without q_online; weight without g. */
typedef struct sg_retrace_config {
    uint32_t struct_size;         /* sizeof(sg_retrace_config), set by sg_retrace_config_init */
    double gamma;                 /* discount, in [0, 1]; not read when discounts is given */
    double lambda;                /* the trace's lambda, in [0, 1]; not read when discounts is given */
    double c_bar;                 /* clips the ratio of the trace; > 0, +inf allowed */
    int32_t bootstrap_truncated;  /* as sg_gae_config's */
    float huber_delta;            /* the loss outputs' Huber threshold; > 0, +inf: the squared loss */
    const float *discounts;       /* optional DEVICE float32 [2]: (gamma, lambda), read at every launch */
    int32_t reserved;             /* 0 */
} sg_retrace_config;
/* gamma 0.99, lambda 1.0, c_bar 1.0, bootstrap_truncated 1, huber_delta +inf and a null discounts */
void sg_retrace_config_init(sg_retrace_config *cfg);
int sg_retrace_device(sg_env *env, int32_t length, int32_t n, const sg_retrace_config *cfg, const float *reward_dev, const uint8_t *done_dev,
                      const uint8_t *truncated_dev, const float *q_dev, const float *value_dev, const float *last_value_dev,
                      const float *ratio_dev, const float *terminal_value_dev, float *target_dev, const float *q_online_dev,
                      const float *weight_dev, float *td_error_dev, float *g_dev, void *hip_stream);

/* Replay ring with uniform n-step sampling -- what an off-policy learner (SAC, TD3: the learners the reference's README names) keeps
 * around the step: the last transitions (s, a, r, s', terminated), where s' of a finished step is the LAST observation of the episode
 * that ended (not the first one of the next episode, which auto-reset put into obs[t]) and a truncated step still bootstraps (SB3
 * ReplayBuffer with handle_timeout_termination, optimize_memory_usage layout).  The reference has no counterpart.
 * The ring is device memory of the caller's in the rollout's own layout, T = steps time slots of B = num_envs envs, D = obs_dim:
 *   obs         float32 [T, B, D]   obs[p] = the observation rows the step stored at slot p wrote (after auto-reset)
 *   action      float32 [T, B, 2]   (discrete ids: int32 [T, B]) the action of slot p
 *   reward      float32 [T, B]      as the stepping call wrote it
 *   done, trunc uint8   [T, B]      as the stepping call wrote them
 *   term_idx    uint32  [T, B]      sequence number of the terminal record of (p, i); written and read ONLY where done[p, i]
 *   term_obs    float32 [C, D]      C = term_capacity: ring of terminal observations, record seq lives at seq mod C
 *   slot_seq    uint32  [T]         term_head as it was before the commit that filled slot p
 *   hdr         32 bytes            uint32 magic, T, B, D, head, filled, term_head, sample_calls (written by the kernels only)
 * so sg_rollout_device* / sg_step_device write straight into rows of the ring (no copy on insert) and the transition stored at
 * slot p, env i is
 *   s  = obs[(p - 1) mod T, i]     a = action[p, i]     r = reward[p, i]
 *   s' = term_obs[term_idx[p, i] mod C] if done[p, i], else obs[p, i]
 *   terminated = done[p, i] and not trunc[p, i]         truncated = trunc[p, i]
 * With filled = f and head = h the valid transitions are the v = min(f, T - 1) newest slots (h - v) mod T .. (h - 1) mod T: the
 * oldest slot of a full ring has lost its s to the newest write, so a full ring holds T - 1 transitions per env; transition u in
 * [0, v B) is env u mod B of slot (h - v + u / B) mod T.  Results depend on the arguments and the ring's contents only: the handle
 * gives B, D, the action type, the device and the status word, and no env is touched.  Version 1 needs auto_reset on (the case in
 * which the terminal observation would otherwise be lost): a handle with it off is refused.  tests/replay_model.py states all of
 * this in NumPy, bit for bit.
 * Every call enqueues on the caller's stream, allocates nothing, never synchronises and is hipGraph-capturable on one stream.
 * Refused on the host by all three (SG_ERR_INVALID, nothing enqueued): a wrong struct_size, a null member, steps < 2,
 * term_capacity outside 1 .. 2^31 - 1, steps * num_envs > 2^31 - 1, auto_reset off.  The header lives in device memory, so a ring
 * that sg_replay_begin_device has not initialised for this T, B, D (no magic) is found on the device: such a call writes nothing
 * and sets the status word.  Device-side refusals use status code 8: every later call on the handle fails with SG_ERR_HIP until
 * sg_check_status has reported the condition (SG_ERR_INVALID) and cleared it. */
typedef struct sg_replay {
    uint32_t struct_size;    /* sizeof(sg_replay) */
    int32_t steps;           /* T >= 2 */
    uint32_t term_capacity;  /* C >= 1 */
    uint32_t reserved;       /* 0 */
    float *obs;
    void *action;
    float *reward;
    uint8_t *done;
    uint8_t *trunc;
    uint32_t *term_idx;
    float *term_obs;
    uint32_t *slot_seq;
    void *hdr;
} sg_replay;
/* Bytes of each member for a ring of `steps` slots on this handle, in the order of the struct (obs, action, reward, done, trunc,
 * term_idx, term_obs, slot_seq, hdr) into member_bytes [9] (NULL to skip); returns the sum with every member rounded up to 16 bytes
 * (one allocation cut into 16-byte aligned members), 0 for invalid arguments.  Members need their element type's alignment only. */
size_t sg_replay_bytes(const sg_env *env, int32_t steps, uint32_t term_capacity, size_t *member_bytes);
/* Writes the header (head = filled = term_head = sample_calls = 0) and, if obs0_dev is given, copies the [B, D] observation the
 * first action will be taken from into obs[T - 1] (NULL: the caller wrote that row itself, e.g. sg_reset_device(obs + (T - 1) B D)). */
int sg_replay_begin_device(sg_env *env, const sg_replay *ring, const float *obs0_dev, void *hip_stream);
/* The caller has just had n_steps consecutive steps written into slots first_slot .. first_slot + n_steps - 1 (rollout rows, or one
 * sg_step_device with terminal_obs) and their actions into action[...]; this makes them part of the ring.  Exactly one terminal form:
 *   list   (a rollout's sg_terminal_list, `step` relative to first_slot): record k < min(count, capacity) gets seq = term_head + k,
 *          its D floats go to term_obs[seq mod C] and term_idx[first_slot + t_k, i_k] = seq; then term_head += min(count, capacity).
 *          Two launches: the records (one 16-lane group each), then one wave for the header.
 *   dense  (n_steps == 1, float32 [B, D] as sg_step_device fills it): every env with done[first_slot, i] gets the next free sequence
 *          number, in no particular order, and its row is copied.  Three launches (term_head noted, records, header).
 * Then slot_seq[p] = the term_head before this commit for every committed slot, hdr.head = (first_slot + n_steps) mod T and
 * hdr.filled = min(filled_before + n_steps, T).  The host is the authority on first_slot and filled_before: the C caller keeps the
 * two integers (first_slot of the next commit = hdr.head of this one).  A replayed captured commit writes the same head and filled
 * again and appends its records again: capture a commit together with the stepping call that feeds it, per slot range.
 * Refused on the host (besides the above): first_slot < 0, n_steps < 1, first_slot + n_steps > T (a commit may not cross the end of
 * the ring: choose T a multiple of the rollout length), filled_before outside [0, T], both or neither terminal form, the dense form
 * with n_steps != 1, a null pointer in the list.  Checked on the device (status code 8): a list with count > capacity (records are
 * missing); a record outside [0, n_steps) x [0, B) (ignored); and a terminal ring too small: after the commit, term_head -
 * slot_seq[oldest valid slot] > C (unsigned, modulo 2^32; conservative by at most one commit's records), i.e. a record that a valid
 * transition still names may have been overwritten.  That check is what lets the sampler trust term_idx. */
int sg_replay_commit_device(sg_env *env, const sg_replay *ring, int32_t first_slot, int32_t filled_before, int32_t n_steps,
                            const sg_terminal_list *terminal_list, const float *terminal_obs_dense_dev, void *hip_stream);
/* A minibatch of n transitions, drawn uniformly with replacement, with n-step returns, in one launch (plus one lane that advances
 * hdr.sample_calls on the device: a replayed captured call draws fresh indices and sees the ring grow, since head and filled are
 * read from the header).  For draw j of the ring's call number c = hdr.sample_calls, h = hdr.head, v as above:
 *   w      = philox4x32_10(key = seed, counter = (j lo, j hi, c, 3))        -- the engine's Philox, stream tag 3
 *   u      = umul64hi(w0 | w1 << 32, v B)                                   -- or index_in[j] when index_in is given
 *   q, i   = u / B, u mod B;   p_k = (h - v + q + k) mod T
 *   k = 0:             R = (double) reward[p_0, i];  g = gamma
 *   k = 1 .. n_step-1: stop before k if done[p_{k-1}, i] or q + k >= v (the newest edge)
 *                      R = R + g * (double) reward[p_k, i];  g = g * gamma  -- float64, each operation rounded on its own
 *   last = the last k included
 *   obs = obs[(p_0 - 1) mod T, i];  action = action[p_0, i];  reward = (float) R;  discount = (float) g;  steps = last + 1
 *   next_obs, terminated, truncated = s', terminated, truncated of (p_last, i);  index = u
 * so the learner's target is reward + discount (1 - terminated) Q(next_obs), and with n_step = 1 the batch is the stored transition
 * bit for bit.  index_in (int64 [n], values of u) replaces the random draw: the hook for prioritized or stratified sampling done by
 * the caller.  A value outside [0, v B) leaves row j of every output untouched and sets status code 8; so does v = 0 with n > 0
 * (nothing is written).  n = 0 enqueues nothing.  Refused on the host: n_step outside 1 .. 16, gamma outside [0, 1] or NaN, n < 0
 * or > 2^31 - 1, a null batch or a null obs, action, reward, next_obs, terminated or truncated (discount, steps, index may be NULL). */
typedef struct sg_replay_sample_config {
    uint32_t struct_size;  /* sizeof(sg_replay_sample_config), set by sg_replay_sample_config_init */
    uint64_t seed;         /* Philox key of the draws */
    int32_t n_step;        /* 1 .. 16 */
    double gamma;          /* discount, in [0, 1] */
} sg_replay_sample_config;
/* seed 0, n_step 1, gamma 0.99 */
void sg_replay_sample_config_init(sg_replay_sample_config *cfg);
typedef struct sg_replay_batch {
    float *obs;           /* [n, D] */
    void *action;         /* float32 [n, 2]; discrete ids: int32 [n] */
    float *reward;        /* [n] */
    float *next_obs;      /* [n, D] */
    uint8_t *terminated;  /* [n] */
    uint8_t *truncated;   /* [n] */
    float *discount;      /* [n], may be NULL */
    uint8_t *steps;       /* [n], may be NULL */
    int64_t *index;       /* [n], may be NULL */
} sg_replay_batch;
/* cfg NULL: sg_replay_sample_config_init's values */
int sg_replay_sample_device(sg_env *env, const sg_replay *ring, const sg_replay_sample_config *cfg, int64_t n,
                            const int64_t *index_in_dev, const sg_replay_batch *out, void *hip_stream);

/* Fixed-length sequences from the replay ring: n columns of L = length consecutive steps of one env each, time-major, so that column
 * j is one pseudo-env of an L-step rollout -- what V-trace (sg_vtrace_device), Retrace, Q(lambda), a multi-epoch PPO over old
 * rollouts or a sequence model read.  With T, B, D, C, h = hdr.head, v = min(hdr.filled, T - 1) as above, first = (h - v) mod T the
 * oldest valid slot and transition number u = q B + i the transition of env i at slot (first + q) mod T (sg_replay_sample_device's
 * index_in, sg_priority_sample_device's index), a sequence of L in 1 .. T - 1 steps may start at q in [0, v - L + 1): its last step
 * q + L - 1 is still a valid transition, so it never crosses the newest edge.  S = (v - L + 1) B.  For column j of the ring's call
 * number c = hdr.sample_calls:
 *   w      = philox4x32_10(key = seed, counter = (j lo, j hi, c, 8))        -- the engine's Philox, stream tag 8
 *   u      = umul64hi(w0 | w1 << 32, S)                                     -- or index_in[j] when index_in is given
 *   q, i   = u / B, u mod B;   p_k = (first + q + k) mod T,  k = 0 .. L - 1
 *   obs[0, j]          = ring.obs[(p_0 - 1) mod T, i]
 *   obs[k + 1, j]      = ring.obs[p_k, i]        -- what the rollout stored: after a done, the next episode's first observation
 *   action[k, j], reward[k, j], done[k, j], trunc[k, j] = the ring's members at (p_k, i), bits unchanged
 *   terminal_obs[k, j] = ring.term_obs[term_idx[p_k, i] mod C]  where done[p_k, i];  NOT WRITTEN elsewhere
 *   extra_out[e][k, j] = extra_in[e][p_k, i]     -- e < n_extra <= 4
 *   index[j]           = u
 * Outputs: obs [L + 1, n, D], action [L, n, 2] (discrete ids: int32 [L, n]), reward, done, trunc [L, n]; with n = num_envs they go
 * straight into sg_gae_device / sg_gae_groups_device / sg_vtrace_device, with terminal_value = V(terminal_obs) in the dense form; with
 * any n into sg_retrace_device (Retrace, Q(lambda)).
 * terminal_obs [L, n, D], index [n] and the extras may be NULL; the learner reads terminal_obs only where done.  extra_in[e] are
 * caller-owned float32 [T, B] device arrays in the ring's slot layout (a closed-loop rollout's logp / value buffers are slices of
 * them: they are how the behaviour log-prob reaches V-trace); the ring does not own them and commits do not touch them.
 * One launch, plus the one lane that advances hdr.sample_calls (the ring's one counter, shared with sg_replay_sample_device), so a
 * replayed captured call draws afresh and sees the ring grow.  The call allocates nothing, never synchronises and is capturable.
 * Status code 8: no matching header, or v < L with n > 0 (nothing is written); an index_in[j] outside [0, S) (every row of column j
 * of every output is left untouched).  n = 0 enqueues nothing.  Refused on the host (besides what every replay call refuses): a null
 * cfg or a wrong struct_size, length outside 1 .. T - 1, n outside 0 .. 2^31 - 1, (length + 1) n > 2^31 - 1, a null out or a null
 * obs, action, reward, done or trunc, n_extra outside 0 .. 4, a null extra_in[e] or extra_out[e] with e < n_extra.
 * tests/sequence_model.py states all of this in NumPy, bit for bit. */
typedef struct sg_replay_sequence_config {
    uint32_t struct_size;  /* sizeof(sg_replay_sequence_config), set by sg_replay_sequence_config_init */
    uint64_t seed;         /* Philox key of the draws */
    int32_t length;        /* L: 1 .. T - 1 */
    int32_t n_extra;       /* 0 .. 4 */
} sg_replay_sequence_config;
/* seed 0, length 1, n_extra 0 */
void sg_replay_sequence_config_init(sg_replay_sequence_config *cfg);
typedef struct sg_replay_sequences {
    float *obs;                 /* [L + 1, n, D] */
    void *action;               /* float32 [L, n, 2]; discrete ids: int32 [L, n] */
    float *reward;              /* [L, n] */
    uint8_t *done;              /* [L, n] */
    uint8_t *trunc;             /* [L, n] */
    float *terminal_obs;        /* [L, n, D], may be NULL; written only where done */
    int64_t *index;             /* [n], may be NULL */
    const float *extra_in[4];   /* [T, B] each; the first n_extra are read */
    float *extra_out[4];        /* [L, n] each */
} sg_replay_sequences;
int sg_replay_sequence_device(sg_env *env, const sg_replay *ring, const sg_replay_sequence_config *cfg, int64_t n,
                              const int64_t *index_in_dev, const sg_replay_sequences *out, void *hip_stream);

/* Hindsight goal relabelling (Hindsight Experience Replay, Andrychowicz et al. 2017; SB3's HerReplayBuffer) of a batch of the Goal
 * ids, in place, in one launch: with probability her_ratio a row's goal becomes the position the ship reached k* steps later in the
 * same episode.  `batch` is what sg_replay_sample_device (with or without index_in: the prioritized path) has just written from
 * this ring with n_step = 1; no commit may lie between that call and this one (index names transitions relative to the ring's
 * head).  batch->index and batch->steps are required here.  The goal is the last two observation columns, (goal - position) *
 * two_over_world; the achieved position is columns 0, 1.  With h, v, B, T, C as above and c = hdr.sample_calls as the header holds
 * it when the kernel runs (this call does not advance it: the sampler's own tick is what makes a replayed captured pair draw
 * afresh), for row j:
 *   u      = index[j];  outside [0, v B): the row is left untouched and status code 8 is set (relabelled[j] is not written)
 *   steps[j] != 1: the row is left untouched, relabelled[j] = 2
 *   q, i   = u / B, u mod B;   p_k = (h - v + q + k) mod T
 *   w      = philox4x32_10(key = seed, counter = (j lo, j hi, c, 12))       -- the engine's Philox, stream tag 12
 *   relabel iff (uint64) w2 < thr,  thr = floor(her_ratio * 2^32 + 0.5) computed on the host; else untouched, relabelled[j] = 0
 *   m      = min(horizon - 1, v - 1 - q, the first k with done[p_k, i])     -- the n-step walk's stopping rule: the window
 *            0 .. m never crosses an episode end or the newest edge
 *   k*     = umul64hi(w0 | w1 << 32, m + 1) (strategy 0, "future": 0 .. m, the step's own end position included, as SB3's);
 *            m (strategy 1, "final")
 *   a      = columns 0, 1 of s' of (p_k*, i): term_obs[term_idx[p_k*, i] mod C] where done[p_k*, i], else ring.obs[p_k*, i]
 *   x0, x1 = columns 0, 1 of batch.obs[j], batch.next_obs[j];  o = columns D - 2, D - 1 of batch.next_obs[j] as they were
 *   batch.obs[j, D - 2 + d]      = (a_d - x0_d) * two_over_world            -- float32: one subtract, one multiply (the engine's
 *   batch.next_obs[j, D - 2 + d] = (a_d - x1_d) * two_over_world               goal_observe)
 *   the reward, float64, every operation rounded on its own (no fused multiply-add), d = 0, 1:
 *     vo1_d = (double) o_d * (double) half_world                            -- old goal - x1
 *     vo0_d = vo1_d + ((double) x1_d - (double) x0_d)                       -- old goal - x0
 *     vn0_d = (double) a_d - (double) x0_d;   vn1_d = (double) a_d - (double) x1_d
 *     |v|^2 = v_0 v_0 + v_1 v_1;   |v| = sqrt(|v|^2)
 *     term(v0, v1) = goal_scale * (|v0| - |v1|) + (|v1|^2 < goal_r2 ? sparse : 0.0)
 *     batch.reward[j] = (float) (((double) reward[j] - term(vo0, vo1)) + term(vn0, vn1))
 *   relabelled[j] = 1, offset[j] = k*, goal[j] = a                          -- offset and goal are written only where relabelled
 * goal_scale (goal_vel_reward_scale * 100) and sparse (goal_sparse_reward) are those of env i's CURRENT reward profile
 * (sg_set_reward_profiles / sg_set_env_profiles; the handle's own values while profiles are off), goal_r2 the handle's.  The
 * survival and safety terms do not depend on the goal and ride along inside reward.  terminated, truncated, discount and action
 * are not touched: crashes and time limits do not depend on the goal.
 * The old goal is taken from next_obs, not from obs: the engine writes the observation before it resamples a goal that was hit, so
 * the obs of the step after a hit still names the goal that was hit, while its reward was formed under the new one, which its
 * next_obs names.  Two properties follow from working on a stored batch: the old term is re-formed from float32 observations,
 * whereas the engine formed it from the unrounded end position, so reward' differs from what the engine would have returned under
 * the new goal by about goal_scale * ulp(position) (measured: DESIGN section 34); and a stored reward whose goal distance lies
 * within that rounding of goal_radius may have its sparse bonus mis-subtracted.  With k* = 0 the new goal columns of next_obs are
 * exactly 0 and the sparse bonus is always present.
 * The optional outputs (members of `out`, or a NULL `out`): relabelled uint8 [n], offset int32 [n], goal float32 [n, 2].
 * One launch; the call allocates nothing, never synchronises and is hipGraph-capturable.  n = 0 enqueues nothing.  Status code 8:
 * no matching header or v = 0 with n > 0 (nothing is written); an index[j] outside [0, v B).  Refused on the host (SG_ERR_INVALID,
 * nothing enqueued; besides what every replay call refuses, auto_reset off among it): a null cfg or a wrong struct_size, her_ratio
 * outside [0, 1] or NaN, horizon outside 1 .. T - 1, a strategy other than 0 and 1, n outside 0 .. 2^31 - 1, a null batch or a
 * null index, steps, obs, next_obs or reward, a Kepler id (no goal), observation or reward normalization on (the ring then holds
 * normalized values that cannot be decoded).  tests/her_model.py states all of this in NumPy, bit for bit. */
typedef struct sg_replay_relabel_config {
    uint32_t struct_size;  /* sizeof(sg_replay_relabel_config), set by sg_replay_relabel_config_init */
    uint64_t seed;         /* Philox key of the draws */
    double her_ratio;      /* share of the rows relabelled, in [0, 1] */
    int32_t horizon;       /* H: 1 .. T - 1, the steps of the future the new goal is drawn from (1: the step's own end position) */
    int32_t strategy;      /* 0: future, 1: final */
} sg_replay_relabel_config;
/* seed 0, her_ratio 0.8, horizon 1, strategy 0 */
void sg_replay_relabel_config_init(sg_replay_relabel_config *cfg);
typedef struct sg_replay_relabel_out {
    uint8_t *relabelled;  /* [n], may be NULL: 0 left as drawn, 1 relabelled, 2 refused (steps != 1) */
    int32_t *offset;      /* [n], may be NULL: k*, written where relabelled */
    float *goal;          /* [n, 2], may be NULL: the new goal position, written where relabelled */
} sg_replay_relabel_out;
int sg_replay_relabel_device(sg_env *env, const sg_replay *ring, const sg_replay_relabel_config *cfg, int64_t n,
                             const sg_replay_batch *batch, const sg_replay_relabel_out *out, void *hip_stream);

/* Prioritized sampling from the replay ring (Schaul et al. 2016, proportional variant) with an exact integer sum tree.  A
 * caller-owned device object next to the ring holds one priority per cell c = p B + i (slot p, env i: by slot, so nothing moves when
 * the ring wraps) as an UNSIGNED FIXED-POINT INTEGER q with frac_bits fractional bits; every sum over them is a 64-bit integer.
 * Integer addition is associative: the contents do not depend on reduction order or on the arrival order of atomics, never drift,
 * and the draw is defined without reference to any tree:
 *     the cell chosen for a number r in [0, total) is the smallest cell c with q[0] + ... + q[c] > r.
 * `node` holds partial sums that serve that definition: opaque memory whose layout is the library's business.  q = 0 marks a cell
 * that holds no valid transition (the hole slot whose s the newest write destroyed, a slot never filled): it is never drawn.
 * Exponents (|delta|^alpha, (N P)^-beta) are the only inexact arithmetic and are kept out of the integer state: the priority
 * handed to sg_priority_update_device is already raised to alpha.  tests/priority_model.py states all of this in NumPy.
 * Every call enqueues on the caller's stream, allocates nothing, never synchronises and is hipGraph-capturable on one stream (no
 * parallel branches).  Refused on the host by every call (SG_ERR_INVALID, nothing enqueued): a wrong struct_size, a null member,
 * leaf or node not 16-byte aligned, steps < 2, steps * num_envs > 2^31 - 1, frac_bits outside 0 .. 31, auto_reset off.  An object
 * that sg_priority_begin_device has not initialised for this T, B, frac_bits (no magic) is found on the device.  Device-side
 * refusals use status code 9: every later call on the handle fails with SG_ERR_HIP until sg_check_status has reported the
 * condition (SG_ERR_INVALID) and cleared it. */
typedef struct sg_priority {
    uint32_t struct_size;  /* sizeof(sg_priority) */
    int32_t steps;         /* T of the ring */
    int32_t frac_bits;     /* 0 .. 31: priority 1.0 is q = 1 << frac_bits */
    uint32_t reserved;     /* 0 */
    uint32_t *leaf;        /* [T, B]  q of cell c = p * B + i, ring layout */
    uint64_t *node;        /* opaque partial sums, size from sg_priority_bytes */
    void *hdr;             /* 64 bytes: uint32 magic, T, B, frac_bits, head, filled, max_q, sample_calls; uint64 total; reserved */
} sg_priority;
/* Bytes of leaf, node and hdr for a ring of `steps` slots on this handle into member_bytes [3] (NULL to skip); returns the sum with
 * every member rounded up to 16 bytes, 0 for invalid arguments. */
size_t sg_priority_bytes(const sg_env *env, int32_t steps, size_t *member_bytes);
/* All leaves and nodes 0, total = 0, head = filled = sample_calls = 0, max_q = 1 << frac_bits (priority 1.0). */
int sg_priority_begin_device(sg_env *env, const sg_priority *prio, void *hip_stream);
/* Called after sg_replay_commit_device, with the same three integers: every cell of slots first_slot .. first_slot + n_steps - 1
 * gets max_q (a new transition is seen at least once), every cell of slot (first_slot + n_steps) mod T gets 0 (the hole: the slot
 * whose s the newest write destroyed; on a ring that is not yet full it is 0 already), and total, the nodes, head and filled follow.
 * Host refusals are those of sg_replay_commit_device: first_slot < 0, n_steps < 1, first_slot + n_steps > T, filled_before outside
 * [0, T]. */
int sg_priority_commit_device(sg_env *env, const sg_priority *prio, int32_t first_slot, int32_t filled_before, int32_t n_steps,
                              void *hip_stream);
/* New priorities for n cells: cell_dev int64 [n] (the `cell` a draw returned: unlike `index` it does not shift with the next
 * commit), priority_dev float32 [n], already raised to alpha.  q = clamp(rint((double) p * 2^frac_bits), 1, 2^32 - 1), exact in
 * float64 (p = 0 gives q = 1).  Duplicates of a cell within one call: the LARGEST q wins, so the result does not depend on order.
 * A cell outside the current valid window (the hole, or a never-filled slot) is skipped silently: that is the ordinary race between
 * a learner and the collector overwriting the ring, and it never makes an invalid cell samplable.  Status code 9 (row skipped) for a
 * cell outside [0, T B) and for a p that is NaN, negative or infinite.  max_q = max(max_q, every applied q).  n = 0 enqueues nothing.
 * Refused on the host: n outside 0 .. 2^31 - 1, a null cell_dev or priority_dev with n > 0. */
int sg_priority_update_device(sg_env *env, const sg_priority *prio, int64_t n, const int64_t *cell_dev, const float *priority_dev,
                              void *hip_stream);
/* n draws in proportion to q.  For draw j of the object's call number c = hdr.sample_calls, with v = min(filled, T - 1):
 *   w = philox4x32_10(key = seed, counter = (j lo, j hi, c, 4))                  -- the engine's Philox, stream tag 4
 *   x = w0 | w1 << 32
 *   stratified:   len_j = total / n + (j < total mod n);  lo_j = j (total / n) + min(j, total mod n);  r = lo_j + umul64hi(x, len_j)
 *                 (the strata tile [0, total) exactly; 64-bit arithmetic only)
 *   independent:  r = umul64hi(x, total)
 *   cell   = the smallest c with q[0] + ... + q[c] > r;   p, i = cell / B, cell mod B;   leaf = q[cell]
 *   index  = ((p - (head - v)) mod T) B + i               -- the transition number sg_replay_sample_device takes as index_in
 *   weight = (float) pow(((double) (v B) * (double) q) / (double) total, -beta)  -- each operation rounded on its own; unnormalised;
 *                                                                                   beta = 0 gives exactly 1
 * sample_calls advances on the device, so a replayed captured call draws afresh.  The gather of the drawn transitions is
 * sg_replay_sample_device with index_in = index, enqueued by the caller.  Status code 9, nothing written: no matching header;
 * total = 0 with n > 0; stratified with total < n; hdr.head / hdr.filled of the priorities different from the ring's (a commit was
 * forgotten); and, for its own row, a drawn cell outside the valid window (impossible if the structure is right: a check, not a
 * path).  n = 0 enqueues nothing.  Refused on the host: a null ring, cfg struct_size, steps different from the ring's, beta negative
 * or NaN, n outside 0 .. 2^31 - 1, a null out, index or weight (cell and leaf may be NULL). */
typedef struct sg_priority_sample_config {
    uint32_t struct_size;  /* sizeof(sg_priority_sample_config), set by sg_priority_sample_config_init */
    uint64_t seed;         /* Philox key of the draws */
    double beta;           /* importance exponent, >= 0 */
    int32_t stratified;    /* 1: one draw per stratum of [0, total); 0: independent draws */
} sg_priority_sample_config;
/* seed 0, beta 0.4, stratified 1 */
void sg_priority_sample_config_init(sg_priority_sample_config *cfg);
typedef struct sg_priority_draw {
    int64_t *index;   /* [n] */
    int64_t *cell;    /* [n], may be NULL */
    float *weight;    /* [n] */
    uint32_t *leaf;   /* [n], may be NULL */
} sg_priority_draw;
/* cfg NULL: sg_priority_sample_config_init's values */
int sg_priority_sample_device(sg_env *env, const sg_replay *ring, const sg_priority *prio, const sg_priority_sample_config *cfg,
                              int64_t n, const sg_priority_draw *out, void *hip_stream);

/* Closed-loop rollouts: a small MLP actor-critic evaluated, sampled and scored on the device, so that a PPO / A2C learner's
 * collection loop is the engine's own work: one launch per env-step beside the step kernel instead of an eager forward, a
 * torch.distributions sample and a log_prob.  The reference has no counterpart.  The parametrisation is SB3's / CleanRL's:
 *   actor    obs_dim -> hidden (x n_hidden) -> head     head = 2 (continuous ids: the mean) or 6 (discrete ids: the logits)
 *   critic   obs_dim -> hidden (x n_hidden) -> 1        optional, a net of its own (nothing is shared with the actor)
 *   log_std  [2], state-independent                     continuous ids only
 * Every hidden layer is followed by the activation; the heads are linear.  All parameters are float32 DEVICE pointers in
 * torch.nn.Linear layout -- weight [out, in] row-major, bias [out] -- owned by the caller and read in place at every call: a
 * learner's parameters are used where they are, no copy, no transpose, and an optimizer step is seen by the next call.
 * Arithmetic: float32 throughout.  Output neuron j of a layer is fmaf(W[j][k], h[k], .) over k = 0, 1, ... starting from b[j], one
 * env per lane: no atomics, no cross-lane reduction, so env i's results depend on its own observation row, the parameters and
 * (seed, step, env_index_base + i) only -- not on the batch size, the env's position in the batch or how a job is sharded.
 * Randomness: o = philox4x32_10(key = seed, counter = (env_index_base + i, step lo, step hi, 5)) -- the engine's Philox, stream tag 5,
 * one block per env-step; u23(w) = ((w >> 9) + 0.5) / 2^23.
 *   continuous  eps0 = sqrt(-2 ln u23(o0)) cos(2 pi u23(o1)), eps1 the same with sin (o2, o3 would serve a second pair)
 *               action = mean + exp(log_std) * eps          stored UNCLAMPED: the step clamps on the device itself, and
 *               logp   = sum(-eps^2 / 2 - log_std - ln(2 pi) / 2)   is that of the unclamped Gaussian, as SB3 computes it
 *   discrete    p_j = exp(logit_j - max logit), total = p_0 + ... + p_5; action = the first j with p_0 + ... + p_j >= u23(o0) * total
 *               logp = log_softmax(logits)[action]
 *   deterministic != 0: action = the mean / the first argmax, logp = that action's log-prob; nothing is drawn.
 * tests/policy_model.py states this in NumPy float64; DESIGN section 17 has the kernel and the tolerances. */
#define SG_POLICY_TANH 0
#define SG_POLICY_RELU 1
typedef struct sg_policy_mlp {
    const float *weight[4];  /* layer l < n_hidden: [hidden, in_l] (in_0 = obs_dim, then hidden); layer n_hidden: the head [head, hidden] */
    const float *bias[4];    /* [hidden] ... , [head]; entries past n_hidden are ignored */
} sg_policy_mlp;
typedef struct sg_policy {
    uint32_t struct_size;  /* sizeof(sg_policy) */
    int32_t n_hidden;      /* hidden layers of each net, 1 .. 3 */
    int32_t hidden;        /* their width, 1 .. 128 */
    int32_t activation;    /* SG_POLICY_TANH / SG_POLICY_RELU */
    int32_t head;          /* outputs of the actor: 2 for the continuous ids, 6 for the discrete ones (anything else is refused) */
    int32_t reserved;      /* 0 */
    sg_policy_mlp actor;
    sg_policy_mlp critic;  /* weight[0] == NULL: no critic (every other pointer of it is then ignored) */
    const float *log_std;  /* [2], continuous ids; must be NULL for the discrete ids */
} sg_policy;
/* (action, logp, value) of the observation rows obs_dev float32 [num_envs, obs_dim] in ONE launch on the stream: action_out float32
 * [num_envs, 2] (discrete ids: int32 [num_envs]), logp_out float32 [num_envs] (may be NULL), value_out float32 [num_envs] (NULL
 * without a critic; may be NULL with one: the critic is then not evaluated).  action_out may be NULL when value_out is given (values
 * only).  Allocates nothing, never synchronises, reads nothing of the envs' state and is hipGraph-capturable.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): a wrong struct_size, n_hidden outside 1 .. 3, hidden outside 1 .. 128,
 * an unknown activation, a head that is not the id's, a null weight or bias among the layers in use, a log_std missing (continuous)
 * or given (discrete), a value_out without a critic, no output at all. */
int sg_policy_act_device(sg_env *env, const sg_policy *policy, const float *obs_dev, uint64_t seed, uint64_t step,
                         int32_t deterministic, void *action_out, float *logp_out, float *value_out, void *hip_stream);
/* n_steps closed-loop steps without a host synchronisation.  obs float32 [n_steps + 1, num_envs, obs_dim]: the caller puts the
 * current observations into row 0; step t reads row t and writes row t + 1.  action float32 [n_steps, num_envs, 2] (discrete ids:
 * int32 [n_steps, num_envs]); logp (may be NULL), reward, done, truncated [n_steps, num_envs]; value float32 [n_steps + 1, num_envs].
 * For every t the call enqueues the act kernel above with step = first_step + t and then the single step that sg_step_device
 * enqueues, so episode statistics, normalization, reward profiles and counters behave exactly as for n_steps calls of
 * sg_step_device, and every output is bit for bit what that hand-written loop gives.  Then one launch of the critic alone writes
 * value[n_steps] -- sg_gae_device's last_value, its `value` being rows 0 .. n_steps - 1.
 * terminal_list (may be NULL) is filled as by sg_rollout_device_terminal -- one record per finished env-step, `step` = t, the count
 * running past the capacity, the excess dropped; nothing with auto_reset off -- and, when terminal_value (float32 [capacity]) is
 * given too, one more launch of the critic over the list's records writes V of each record's observation beside it: count, step_env
 * and terminal_value together are a ready sg_value_list.  With observation normalization on the records are normalized with the
 * statistics of their own step, like sg_step_device's terminal_obs rows, and so are the rows the policy reads.
 * Refused as sg_policy_act_device refuses, and: n_steps < 1, a null obs, action, reward, done or truncated, a value or
 * terminal_value without a critic, a terminal_value without a terminal_list, an incomplete list.  (A critic with a NULL value is
 * accepted: it is not evaluated for the rows; terminal_value is still served.) */
int sg_rollout_policy_device(sg_env *env, int32_t n_steps, const sg_policy *policy, uint64_t seed, uint64_t first_step,
                             int32_t deterministic, float *obs, void *action, float *logp, float *value, float *reward,
                             uint8_t *done, uint8_t *truncated, const sg_terminal_list *terminal_list, float *terminal_value,
                             void *hip_stream);

/* The learner's half of an on-policy update: log-prob, entropy and value of GIVEN (obs, action) rows under the current parameters,
 * and the gradients of a loss on those three vectors with respect to the parameters.  The loss itself stays the caller's code on
 * [n] vectors; everything that touches the [n, hidden] activations is the engine's.  n is a row count of its own, any n >= 1 (a
 * minibatch of the flattened rollout, not num_envs).
 *   obs     float32 [n, obs_dim]
 *   action  float32 [n, 2], unclamped as sg_policy_act_device stored it (discrete ids: int32 [n], 0 .. 5; any other value is the
 *           caller's error -- the kernels select by comparison and never index with it, so it cannot reach out of bounds)
 * Forward.  value, and the discrete logp, are sg_policy_act_device's arithmetic: for the rows and actions it produced they are its
 * outputs bit for bit (exp(logp_new - logp_old) is exactly 1 before the first optimizer step).
 *   continuous  z_d = (a_d - mean_d) exp(-log_std_d);  logp = sum_d(-z_d^2 / 2 - log_std_d - ln(2 pi) / 2)   (close to act's, which
 *               scores its own eps, not bit-equal);  entropy = sum_d log_std_d + 1 + ln(2 pi), the same for every row
 *   discrete    logp = (logit_a - max) - log(total);  entropy = -sum_j p_j log p_j of the softmax
 * Every output is float32 [n] and may be NULL (the critic is not evaluated without value_out, the actor not without logp_out or
 * entropy_out).  One launch; allocates nothing, never synchronises, hipGraph-capturable.
 * Refused: whatever sg_policy_act_device refuses of the policy; n < 1; a null obs or action; no output; value_out without a critic. */
int sg_policy_evaluate_device(sg_env *env, const sg_policy *policy, int64_t n, const float *obs, const void *action, float *logp_out,
                              float *entropy_out, float *value_out, void *hip_stream);
/* Writable float32 device pointers, one per parameter of an sg_policy and of its shape */
typedef struct sg_policy_grads_mlp {
    float *weight[4];
    float *bias[4];
} sg_policy_grads_mlp;
typedef struct sg_policy_grads {
    uint32_t struct_size;  /* sizeof(sg_policy_grads) */
    uint32_t reserved;     /* 0 */
    sg_policy_grads_mlp actor;
    sg_policy_grads_mlp critic;  /* may be all NULL when g_value is NULL; given without g_value it is written with zeros */
    float *log_std;              /* [2], continuous ids; must be NULL for the discrete ids */
} sg_policy_grads;
/* grads = sum_i (g_logp[i] d logp_i + g_entropy[i] d entropy_i + g_value[i] d value_i) / d theta for every parameter theta: WRITTEN,
 * not accumulated.  g_* float32 [n], the loss's gradients by the three outputs of sg_policy_evaluate_device; each may be NULL (zeros).
 * There is no gradient with respect to obs or action.
 *   continuous  d logp / d mean_d = z_d / sigma_d;  d logp / d log_std_d = z_d^2 - 1;  d entropy / d log_std_d = 1
 *   discrete    d logp / d logit_j = [j = a] - p_j;  d entropy / d logit_j = -p_j (log p_j + H)
 *   tanh' = 1 - h^2 of the activation h;  relu' = [pre-activation > 0]: 0 at 0, as torch.
 * The forward pass is recomputed inside the backward launch: no [n, hidden] activation goes to memory between the two calls.
 * Two launches: the backward, whose workgroups leave partial sums in `workspace` (at least sg_policy_grad_workspace_bytes(env,
 * policy, n) bytes of device memory, any content), and a reduction of the partials in workgroup order.  Allocates nothing, never
 * synchronises, hipGraph-capturable.
 * Arithmetic: float32 throughout, no floating-point atomics, a fixed summation order over the rows -- two calls with the same
 * inputs and the same n give bit-identical gradients.  The order is a function of n (how rows group into workgroups), so the same
 * rows inside a batch of another n may round differently; the forward outputs have no such dependence.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): whatever sg_policy_act_device refuses of the policy; n < 1; a null obs
 * or action; a null grads, a wrong struct_size or reserved; a null pointer among the gradient slots in use (the actor's layers,
 * log_std for the continuous ids, the critic's layers when g_value is given); a log_std gradient for a discrete id; a null workspace
 * or one smaller than the query's answer; g_value or critic gradients given for a policy without a critic. */
int sg_policy_grad_device(sg_env *env, const sg_policy *policy, int64_t n, const float *obs, const void *action, const float *g_logp,
                          const float *g_entropy, const float *g_value, const sg_policy_grads *grads, void *workspace,
                          size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_policy_grad_device needs for n rows (it grows with n up to a cap); 0 and an error message for an invalid policy or n */
size_t sg_policy_grad_workspace_bytes(sg_env *env, const sg_policy *policy, int64_t n);

/* The PPO minibatch update in one call: from stored rollout rows and a minibatch index to the parameter gradients and the loss
 * statistics -- the gathers, sg_policy_evaluate_device, the loss and sg_policy_grad_device of a hand-composed update, without autograd.
 * The objective is the CleanRL / SB3 form.  For entry i of the minibatch, r = index[i] (r = i when index is NULL); logp, entropy and
 * value are sg_policy_evaluate_device's values of row r, bit for bit:
 *     lr = logp - old_logp[r];  ratio = exp(lr);  A = (advantage[r] - mean) * rstd when normalising, else advantage[r]
 *     pg = max(-A ratio, -A clamp(ratio, 1 - c, 1 + c))                                        c = clip_range
 *     vl = 0.5 max((value - ret[r])^2, (vclip - ret[r])^2),  vclip = old_value[r] + clamp(value - old_value[r], -cv, cv)
 *          with cv = clip_range_vf > 0; otherwise vl = 0.5 (value - ret[r])^2
 *     loss = mean(pg) - ent_coef mean(entropy) + vf_coef mean(vl)
 * and what goes to sg_policy_grad_device's backward:
 *     g_logp = -A ratio / n where the unclipped term is >= the clipped one, else 0;  g_entropy = -ent_coef / n
 *     g_value = vf_coef (value - ret[r]) / n where the unclipped square is >= the clipped one; otherwise vf_coef (vclip - ret[r]) / n
 *               inside the clamp (its bounds included) and 0 outside it
 * -- torch's subgradients: clamp passes the gradient at its bounds; the two branches of a max tie only where both give the same
 * derivative, or where A = 0.  clip_range = +inf is allowed and gives the unclipped policy gradient (A2C).  mean and rstd = 1 /
 * (std + adv_epsilon) are those of advantage[index[i]], i < n, std unbiased (torch's .std()), accumulated in float64 in a fixed
 * order and rounded to float32; everything else is float32, and (n) enters as (float)n. */
typedef struct sg_ppo_config {
    uint32_t struct_size;        /* sizeof(sg_ppo_config) */
    float clip_range;            /* c > 0; +inf: no clipping.  Default 0.2 */
    float clip_range_vf;         /* cv; <= 0: the value term is not clipped (default 0) */
    float ent_coef;              /* >= 0, default 0 */
    float vf_coef;               /* >= 0, default 0.5; ignored for a policy without a critic */
    int32_t normalize_advantage; /* default 1; needs n >= 2 */
    float adv_epsilon;           /* >= 0, default 1e-8 */
    int32_t reserved;            /* 0 */
} sg_ppo_config;
void sg_ppo_config_init(sg_ppo_config *cfg);
/* Device pointers into the flattened rollout of `rows` rows */
typedef struct sg_ppo_batch {
    const float *obs;        /* float32 [rows, obs_dim] */
    const void *action;      /* float32 [rows, 2] (discrete ids: int32 [rows]) as sg_policy_act_device stored it */
    const float *old_logp;   /* float32 [rows] */
    const float *advantage;  /* float32 [rows] */
    const float *ret;        /* float32 [rows]; may be NULL for a policy without a critic */
    const float *old_value;  /* float32 [rows]; may be NULL unless clip_range_vf > 0 */
    const int64_t *index;    /* int64 [n] rows of the minibatch, repeats allowed; NULL: rows 0 .. n - 1 */
} sg_ppo_batch;
/* Optional per-row outputs, float32 [n], each may be NULL: the numbers the kernel used for entry i, for tests and for learners that
 * log them (value and g_value need a critic) */
typedef struct sg_ppo_rows {
    float *logp;
    float *value;
    float *g_logp;
    float *g_value;
} sg_ppo_rows;
/* grads (an sg_policy_grads with every slot of the policy's nets given: the actor, log_std for the continuous ids, the critic when
 * the policy has one) receives d loss / d theta, WRITTEN, not accumulated: bit for bit what sg_policy_grad_device gives at the same n
 * for the gathered rows with row_out's g_logp / g_value and g_entropy = -ent_coef / n.
 * stats_out float32 [12]: loss, policy_loss = mean(pg), value_loss = mean(vl) (0 without a critic), entropy = mean(entropy),
 * approx_kl = mean((ratio - 1) - lr), old_approx_kl = mean(-lr), clip_fraction = mean(|ratio - 1| > c), adv_mean, adv_std (both 0
 * when not normalising), bad_rows, and two reserved zeros.
 * An index outside [0, rows) is clamped before any address is formed from it; such an entry contributes zero to every gradient and
 * statistic (to the advantage statistics it counts as advantage 0), is counted in bad_rows, and the means still divide by n.
 * Launches: the advantage statistics (only when normalising), the backward -- sg_policy_grad_device's kernel frame, with the critic
 * first and the loss formed from the head outputs, every workgroup leaving its statistics sums beside its partial sums in
 * `workspace` (at least sg_ppo_grad_workspace_bytes(env, policy, n) bytes, any content) -- and the reduction in workgroup order.
 * Allocates nothing, never synchronises, hipGraph-capturable.  No atomics: the same inputs and the same n give the same bits.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): whatever sg_policy_act_device refuses of the policy; a null cfg, a
 * wrong struct_size or reserved; n < 1; rows < 1; clip_range not > 0; a negative or NaN ent_coef, vf_coef or adv_epsilon; a NaN
 * clip_range_vf; normalize_advantage with n = 1; a null batch, obs, action, old_logp or advantage; a null ret with a critic;
 * clip_range_vf > 0 without old_value; n > rows without an index; a null stats_out; row_out's value or g_value without a critic;
 * what sg_policy_grad_device refuses of grads; a null workspace, one smaller than the query's answer or not aligned to 8 bytes. */
int sg_ppo_grad_device(sg_env *env, const sg_policy *policy, const sg_ppo_config *cfg, const sg_ppo_batch *batch, int64_t rows, int64_t n,
                       const sg_policy_grads *grads, float *stats_out, const sg_ppo_rows *row_out, void *workspace, size_t workspace_bytes,
                       void *hip_stream);
/* Bytes of workspace sg_ppo_grad_device needs for n rows: sg_policy_grad_workspace_bytes' and the statistics partials; 0 and an error
 * message for an invalid policy or n */
size_t sg_ppo_grad_workspace_bytes(sg_env *env, const sg_policy *policy, int64_t n);

/* Policy populations: P = `members` actor-critics of ONE architecture served by one launch per call, for hyper-parameter and seed
 * sweeps and population-based training over many small learners on one batch of envs.  The reference has no counterpart.
 * The parameters are stacked along a leading dimension, the layout of torch.func.stack_module_state: every weight float32
 * [P, out, in], every bias [P, out], log_std [P, 2], each contiguous.  The calls take an ordinary sg_policy, and an ordinary sg_policy_grads, whose
 * pointers address member 0 -- the start of each stacked tensor -- and `members` beside it; member m's tensor is at pointer + m x
 * numel(tensor).  sg_policy keeps its size and reserved stays 0.  An optimizer step, or a copy of one member's slices over another's
 * (PBT's exploit step), is seen by the next call.
 * Member m owns the contiguous block of rows [m n, (m + 1) n): in the act and rollout calls n = num_envs / members of the handle's
 * local envs (members must divide num_envs; the block is by the env's index WITHIN the handle, while the noise stays keyed by the
 * global index env_index_base + i, stream tag 5, exactly as sg_policy_act_device's), in the evaluate and grad calls n is the argument.
 * Arithmetic: none of its own.  One workgroup serves one member and runs sg_policy's kernels' device functions on that member's rows
 * with that member's parameters: every output row of member m is bit for bit what the single-policy call gives for that row with an
 * sg_policy over member m's slices (for the act call: on a handle in which the env has the same global index).
 * Scope: the on-policy family only (sg_policy, continuous and discrete ids); sg_qnet, sg_squashed_policy and sg_dqn have no
 * population calls.
 * Refused by every call (SG_ERR_INVALID, with a message, nothing enqueued): whatever sg_policy_act_device refuses of the policy;
 * members < 1 or members > 65535; then what the single-policy call of the same name refuses. */
/* sg_policy_act_device for `members` members: obs_dev [num_envs, obs_dim]; action_out, logp_out, value_out as there, row i by member
 * i / (num_envs / members).  One launch.  Refused also: members not dividing num_envs. */
int sg_policy_population_act_device(sg_env *env, const sg_policy *policy, int32_t members, const float *obs_dev, uint64_t seed,
                                    uint64_t step, int32_t deterministic, void *action_out, float *logp_out, float *value_out,
                                    void *hip_stream);
/* sg_rollout_policy_device for `members` members: the same buffers, the same loop -- for every t the population act launch with step =
 * first_step + t, then the single step sg_step_device enqueues -- then one critic-only population launch for value[n_steps]; every
 * output is bit for bit what the hand-written loop of sg_policy_population_act_device and sg_step_device gives.  terminal_list (may be
 * NULL) is filled exactly as sg_rollout_policy_device fills it (observation records).
 * terminal_value is served DENSE here: float32 [n_steps, num_envs], the form sg_gae_device reads "only where done and trunc are both
 * set"; when given, every step adds one critic-only population launch over that step's dense terminal rows (sg_step_device's
 * terminal_obs, normalized like them), with or without a list.  terminal_value[t, i] is V, under env i's member, of the last
 * observation of the episode env i finished at step t; rows of envs that did not finish at step t hold UNSPECIFIED values.  A
 * list-shaped terminal_value ([capacity], one per record) is not served: a record's member varies from lane to lane.
 * Refused as sg_policy_population_act_device refuses, and: n_steps < 1, a null obs, action, reward, done or truncated, a value or
 * terminal_value without a critic, an incomplete list. */
int sg_rollout_policy_population_device(sg_env *env, int32_t n_steps, const sg_policy *policy, int32_t members, uint64_t seed,
                                        uint64_t first_step, int32_t deterministic, float *obs, void *action, float *logp, float *value,
                                        float *reward, uint8_t *done, uint8_t *truncated, const sg_terminal_list *terminal_list,
                                        float *terminal_value, void *hip_stream);
/* sg_policy_evaluate_device for `members` members on n rows each: obs float32 [members, n, obs_dim], action float32 [members, n, 2]
 * (discrete ids: int32 [members, n]), outputs float32 [members, n], each may be NULL.  One launch.  Refused also: members x n above
 * 2^31 - 1. */
int sg_policy_population_evaluate_device(sg_env *env, const sg_policy *policy, int32_t members, int64_t n, const float *obs,
                                         const void *action, float *logp_out, float *entropy_out, float *value_out, void *hip_stream);
/* sg_policy_grad_device for `members` members on n rows each: g_* float32 [members, n] (each may be NULL); grads holds the pointers of
 * STACKED gradient tensors of the parameters' shapes ([members, out, in], [members, out], [members, 2]), addressed at member 0 like
 * the policy's; WRITTEN, not accumulated.  sg_policy_grad_device's scheme per member: partial sums workspace[m][group][parameter], a
 * reduction in group order, no atomics -- the same inputs and the same n give the same bits.  A member's rows go to
 *     G = min(ceil(n / R), max(1, 256 / members))   (integer division)
 * workgroups of R rows (R as sg_policy_grad_device's: 256, 128 or 64 by the hidden width), so the workspace stays within about
 * max(256, members) x the parameters' floats.  Consequence: member m's gradient is bit for bit sg_policy_grad_device's for the same
 * n rows and member m's parameters whenever ceil(n / R) <= 256 / members; beyond that it is the same sum in another grouping (close,
 * not bit-equal).  Two launches.  Refused also: members x n above 2^31 - 1; a workspace smaller than
 * sg_policy_population_grad_workspace_bytes(env, policy, members, n). */
int sg_policy_population_grad_device(sg_env *env, const sg_policy *policy, int32_t members, int64_t n, const float *obs, const void *action,
                                     const float *g_logp, const float *g_entropy, const float *g_value, const sg_policy_grads *grads,
                                     void *workspace, size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_policy_population_grad_device needs for n rows per member; 0 and an error message for an invalid policy, members or n */
size_t sg_policy_population_grad_workspace_bytes(sg_env *env, const sg_policy *policy, int32_t members, int64_t n);

/* sg_ppo_grad_device for `members` members in one call: population-based training's update.  policy and grads are the stacked structs of
 * the population calls above; cfg, batch and row_out are sg_ppo_grad_device's structs, unchanged in size.
 * batch is ONE flattened rollout of `rows` rows shared by all members -- the six columns as there; the [K, num_envs] buffers of
 * sg_rollout_policy_population_device and sg_gae_device serve reshaped, without a permuting copy.  batch.index is int64 [members, n]:
 * entry (m, i) is the row member m's minibatch entry i reads, so the gather is what puts a member's env block into its minibatch;
 * repeats are allowed and nothing checks that a row "belongs" to the member.  A NULL index gives member m the rows [m n, (m + 1) n),
 * which needs members x n <= rows.  An index outside [0, rows) is handled as there: clamped before any address is formed from it, zero
 * in every gradient and statistic, counted in THAT member's bad_rows.
 * Per member: the advantage mean and std (float64, unbiased) over member m's n entries; the clipped objective and the subgradients
 * exactly sg_ppo_grad_device's; stats_out float32 [members, 12]; the gradients WRITTEN into slice m of the stacked tensors; row_out's
 * vectors float32 [members, n].
 * member_coef (may be NULL): float32 DEVICE [members, 4], row m = (clip_range, clip_range_vf, ent_coef, vf_coef) of member m.  Given, it
 * replaces those four members of cfg for every member and is read by the kernels at every launch, so a captured graph changes the
 * coefficients by writing the tensor.  cfg's four are still checked as sg_ppo_grad_device checks them; the tensor's VALUES ARE NOT
 * CHECKED (as sg_dqn_act_device's epsilon_dev): clip_range_vf <= 0 or NaN turns value clipping off for that member, by the comparison,
 * and a value the host would have refused -- a NaN or negative ent_coef, say -- affects that member's outputs only.  With member_coef
 * and a critic, batch.old_value is required: any member may turn value clipping on.  normalize_advantage and adv_epsilon are per call.
 * Launches: the advantage statistics (when normalising) with Gadv = min(ceil(n / 1024), max(1, 256 / members)) workgroups per member,
 * the backward with sg_policy_population_grad_device's G = min(ceil(n / R), max(1, 256 / members)) per member, and the reduction with
 * one statistics workgroup per member.  Allocates nothing, never synchronises, hipGraph-capturable; no atomics: the same inputs and the
 * same n give the same bits.
 * BIT-EQUALITY RULE.  Member m's gradient slices, its twelve statistics and its per-row outputs are bit for bit sg_ppo_grad_device's
 * on an sg_policy over member m's parameter slices with index[m] and member m's coefficients whenever the member's entries group as the
 * single call groups them, that is when both
 *     ceil(n / R) <= 256 / members      (the parameter partials and the statistics sums; R = 256, 128 or 64 by the hidden width)
 *     ceil(n / 1024) <= 256 / members   (the advantage partials)
 * hold (integer division).  Beyond either it is the same sums in another grouping: close, not bit-equal.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): whatever the population calls refuse of policy and members; whatever
 * sg_ppo_grad_device refuses; members x n above 2^31 - 1; members x n > rows without an index; a workspace smaller than
 * sg_ppo_population_grad_workspace_bytes(env, policy, members, n) or not aligned to 8 bytes; member_coef with a critic and no old_value. */
int sg_ppo_population_grad_device(sg_env *env, const sg_policy *policy, int32_t members, const sg_ppo_config *cfg, const sg_ppo_batch *batch,
                                  const float *member_coef, int64_t rows, int64_t n, const sg_policy_grads *grads, float *stats_out,
                                  const sg_ppo_rows *row_out, void *workspace, size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_ppo_population_grad_device needs for n entries per member: the parameter partials [members][G][parameters]
 * rounded up to 8 bytes, double [members][Gadv][2], float [members][G][8]; 0 and an error message for an invalid policy, members or n */
size_t sg_ppo_population_grad_workspace_bytes(sg_env *env, const sg_policy *policy, int32_t members, int64_t n);

/* The parameter update: one Adam / AdamW step with global-norm gradient clipping for every member of a population (members = 1: a single
 * net), each member with its own hyperparameters, independently of every other member.  The optimizer is elementwise over a table of
 * tensors and knows nothing about nets: entry k is one parameter tensor stacked [members, numel], contiguous float32, with its gradient
 * and its two moments in the same layout.  All device memory is the caller's; the gradients are READ ONLY (the clipped gradient is never
 * written back).  tests/adam_model.py states every operation and its order in NumPy and is the contract; DESIGN section 26 has the kernels.
 *   hyper   float32 DEVICE [members, 8], row m = (lr, beta1, beta2, eps, weight_decay, max_grad_norm, reserved, reserved) of member m.
 *           Read by the kernels at every launch: a captured graph changes a learning rate by writing the tensor.  ITS VALUES ARE NOT
 *           CHECKED (as member_coef above); a bad value affects that member only.
 *   state   float64 DEVICE [members, 8], 8-byte aligned, row m = (steps, beta1_pow, beta2_pow, skipped, grad_norm, clip_scale, step_size,
 *           applied).  The first four are the member's running state (a fresh member: 0, 1, 1, 0); the last four are what the most
 *           recent call used, each a float32 value stored exactly (applied: 0 or 1), and are how the first launch hands the member's
 *           constants to the second.
 * Per member m, one call:
 *   1. grad_norm = float32(sqrt(S)), S the float64 sum of the float64 squares of ALL of member m's gradient elements of the table (the
 *      global norm over actor, critic and log_std together), summed in a fixed order: lane l of 1024 takes elements l, l + 1024, ...
 *      of entry 0, then of entry 1, ...; then lane[i] += lane[i + s] for s = 512, 256, ..., 1.  No atomics.
 *   2. clip_scale = float32(min(1, max_grad_norm / (grad_norm + 1e-6))), in float64, when 0 < max_grad_norm < inf (torch's
 *      clip_grad_norm_); any other max_grad_norm (0, negative, inf, NaN) gives exactly 1, by the comparison.
 *   3. grad_norm not finite (an inf or NaN anywhere in the member's gradient): the member's step is SKIPPED -- parameters, moments,
 *      steps and the beta powers keep their bits, skipped goes up by one, clip_scale = step_size = applied = 0.
 *   4. Otherwise, in float64 with each operation rounded: beta1_pow *= beta1, beta2_pow *= beta2 (running products: device pow is not
 *      correctly rounded, and a product is right when a member's beta changes between steps), steps += 1,
 *      step_size = float32(lr / (1 - beta1_pow)), bc2s = float32(sqrt(1 - beta2_pow)), applied = 1; and per element in float32, every
 *      operation rounded on its own, 1 - beta and lr weight_decay formed in float32:
 *          g' = g clip_scale;  m' = beta1 m + (1 - beta1) g';  v' = beta2 v + ((1 - beta2) g') g';
 *          den = sqrt(v') / bc2s + eps;  p' = (p - (lr weight_decay) p) - (step_size m') / den
 *      (decoupled weight decay, AdamW; weight_decay = 0 is Adam).  Float32 denormals are kept.
 * Two launches: one workgroup per member for 1 .. 4's per-member part, then the elementwise update, which reads no state that its own
 * launch writes.  Allocates nothing, never synchronises, hipGraph-capturable; the same inputs give the same bits.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): members outside 1 .. 65535; n_tensors outside 1 .. 32; a NULL tensors, or
 * a NULL pointer in a table entry; numel < 1, or members x numel above 2^31 - 1; a NULL hyper or state; state not 8-byte aligned. */
typedef struct sg_adam_tensor {
    float *param;        /* [members, numel] */
    const float *grad;   /* [members, numel]; read only.  sg_adam_exploit_device does not look at it (may be NULL there) */
    float *exp_avg;      /* [members, numel]; zeros before the first step */
    float *exp_avg_sq;   /* [members, numel]; zeros before the first step */
    int64_t numel;       /* elements PER MEMBER */
} sg_adam_tensor;
int sg_adam_step_device(sg_env *env, int32_t members, int32_t n_tensors, const sg_adam_tensor *tensors, const float *hyper, double *state,
                        void *hip_stream);
/* PBT's exploit step with the optimizer state carried along.  src int32 DEVICE [members]: for every m with src[m] != m, member m's
 * parameter, exp_avg and exp_avg_sq slices of every table entry and columns 0 .. 3 of its state row become those of member src[m].
 * hyper is not touched: explore is the caller's write.  One launch, no staging buffer, race-free by this rule: a copy is performed only
 * if its source is not itself a destination (src[src[m]] == src[m]) -- truncation selection (the bottom k copy the top k) always
 * satisfies it.  A copy that breaks the rule, or whose src[m] is outside [0, members), is NOT PERFORMED (the test is made before any
 * address is formed from src[m]) and is counted in refused_out (int32 DEVICE [1], may be NULL; written, not accumulated).
 * Allocates nothing, never synchronises, hipGraph-capturable.  Refused as sg_adam_step_device refuses members, n_tensors and the table
 * (grad aside); a NULL state or src; state not 8-byte aligned. */
int sg_adam_exploit_device(sg_env *env, int32_t members, int32_t n_tensors, const sg_adam_tensor *tensors, double *state, const int32_t *src,
                           int32_t *refused_out, void *hip_stream);

/* The rest of a PBT generation on the device: member fitness from the rows a closed-loop rollout wrote, truncation selection, and
 * explore.  With them a generation -- K closed-loop steps, returns, update, Adam, fitness, select, exploit, explore -- is one graph
 * replay without a host synchronisation.  None of the calls reads the handle's env state: they depend on their arguments and on
 * num_envs = B.  Every call takes the stream, allocates nothing, never synchronises, is hipGraph-capturable and uses no atomics; the
 * same inputs give the same bits.  members = P is 1 .. 256 everywhere.  tests/pbt_model.py states every rule below in NumPy and is the
 * contract; DESIGN section 29 has the kernels.
 *
 * FITNESS.  P must divide B; member m owns the envs [m E, (m + 1) E), E = B / P (the block rule of the population calls).
 *   reward      float32 DEVICE [n_steps, B], done uint8 DEVICE [n_steps, B]: rows as a rollout wrote them, any n_steps >= 1; done
 *               includes truncations.  THE VALUES OF reward ARE NOT CHECKED: a NaN stays within its env's member.
 *   env_return  float64 DEVICE [B], env_length int32 DEVICE [B]: the running return and length of every env's unfinished episode,
 *               read and written back, so that an episode may span calls (zeros before the first).
 *   table       float64 DEVICE [P, 8], 8-byte aligned, row m = (episodes, return_sum, length_sum, return_sq_sum, return_max, return_min,
 *               fitness, reserved) over the episodes member m's envs finished since the row was cleared.
 * Pass 1, one lane per env, rows walked forward in t: run = run + (double) r in float64, each operation rounded on its own;
 * len += 1; at done, in this order, cnt += 1, s += run, l += len, q += run run, mx = fmax(mx, run), mn = fmin(mn, run), then
 * run = 0, len = 0 (identities 0, 0, 0, 0, -inf, +inf; fmax / fmin return the other operand of a NaN).  Pass 2: the per-env values
 * of a member are reduced in chunks of 256 consecutive envs of its block, lanes past E holding the identities, by the fixed tree
 * x[l] = x[l] (+) x[l + s] for s = 128, 64, ..., 1; one lane per member combines the chunk results in ascending order, starting
 * from chunk 0's, then combines that window onto the table row (add, add, add, add, max, min) and writes
 * fitness = return_sum / episodes when episodes >= 1, else NaN.  reserved is left alone.  The order is a function of (B, P) only.
 * Two launches.  workspace: at least sg_pbt_fitness_workspace_bytes(env, members) bytes of device memory, 8-byte aligned, any content.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): members outside 1 .. 256 or not dividing num_envs; n_steps < 1; a null
 * reward, done, env_return, env_length or table; table or env_return not 8-byte aligned; a null, short or misaligned workspace. */
int sg_pbt_fitness_device(sg_env *env, int32_t members, int32_t n_steps, const float *reward, const uint8_t *done, double *env_return,
                          int32_t *env_length, double *table, void *workspace, size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_pbt_fitness_device needs: double [members][ceil(E / 256)][6]; 0 and an error message for invalid members */
size_t sg_pbt_fitness_workspace_bytes(sg_env *env, int32_t members);
/* Table rows back to (0, 0, 0, 0, -inf, +inf, NaN, 0).  src NULL: every row.  src int32 DEVICE [members], as sg_pbt_select_device
 * wrote it: the rows with src[m] != m, the members that were replaced.  The per-env running values are not touched.  One launch.
 * Refused: members outside 1 .. 256; a null table or one not 8-byte aligned. */
int sg_pbt_fitness_clear_device(sg_env *env, int32_t members, double *table, const int32_t *src, void *hip_stream);

/* SELECTION (truncation selection).  fitness float64 DEVICE, member m's value at fitness[m fitness_stride] (fitness_stride in
 * elements, >= 1: 8 reads the table's fitness column in place); ready uint8 DEVICE [members] or NULL.  Member m TAKES PART if and only
 * if ready[m] != 0 (or ready is NULL) and fitness[m] is not NaN; r is the number taking part.  k is the host's
 * floor(fraction members), 0 <= k <= members / 2; the kernel uses k_eff = min(k, r / 2) (integer division).
 *   rank[m] = #{ j taking part : f_j > f_m or (f_j == f_m and j < m) }: all pairs are compared, so it is exact; infinities compare
 *   as floats do.  The top members are those with rank < k_eff, the bottom members those with rank >= r - k_eff.
 * Each bottom member m draws one Philox block, key = seed, counter = (m, step lo, step hi, 9) -- stream tag 9, after the sequence
 * sampler's 8 -- and src_out[m] is the member whose rank is floor(o0 k_eff / 2^32).  Every other member, taking part or not, gets
 * src_out[m] = m.  So src_out[src_out[m]] == src_out[m] by construction: sg_adam_exploit_device refuses nothing of it.
 *   src_out    int32 DEVICE [members]
 *   rank_out   int32 DEVICE [members], may be NULL; -1 for the members not taking part
 *   count_out  int32 DEVICE [2], may be NULL: (copies, k_eff)
 *   step_dev   int64 DEVICE [1], may be NULL: its value is added to step (a 64-bit sum) by the kernel, so a captured graph draws
 *              afresh when the caller bumps it inside the graph.
 * One launch of one workgroup.  Refused: members outside 1 .. 256; a null fitness or src_out; fitness not 8-byte aligned;
 * fitness_stride < 1; k outside 0 .. members / 2. */
int sg_pbt_select_device(sg_env *env, int32_t members, const double *fitness, int64_t fitness_stride, const uint8_t *ready, int32_t k,
                         uint64_t seed, uint64_t step, const int64_t *step_dev, int32_t *src_out, int32_t *rank_out, int32_t *count_out,
                         void *hip_stream);

/* EXPLORE.  One column of a float32 DEVICE tensor [members, C] of hyperparameters -- sg_adam_step_device's hyper, the PPO member_coef,
 * a discounts table with one group per member, or any tensor of the caller's: data points at the column's element of row 0, stride
 * is C.  For every m with src[m] != m, src[m] in [0, members) and src[src[m]] == src[m] (sg_adam_exploit_device's rule), and every
 * column c = 0, 1, ...:
 *   v = data[src[m] stride];  one Philox block, key = seed, counter = ((c << 16) | m, step lo, step hi, 10) -- stream tag 10;
 *   f = (o0 >> 31) ? up : down;
 *   SG_PBT_COPY: x = v;   SG_PBT_SCALE: x = v f;   SG_PBT_SCALE_COMPLEMENT: x = 1 - (1 - v) f   (gamma, lambda, beta: the distance
 *   to 1 is scaled); every float32 operation rounded on its own; data[m stride] = fminf(fmaxf(x, lo), hi).
 * A copy that the rule refuses is not made and is counted in refused_out (int32 DEVICE [1], may be NULL; written, not accumulated).
 * Sources are never destinations, so no element is read and written in one launch; members with src[m] == m keep their bits.
 * step_dev as above.  One launch of one workgroup; the columns travel by value.
 * Refused: members outside 1 .. 256; a null src or columns; n_columns outside 1 .. 16; in a column, a null data, stride < 1, an
 * unknown mode, a NaN down, up, lo or hi, or lo > hi. */
#define SG_PBT_COPY 0
#define SG_PBT_SCALE 1
#define SG_PBT_SCALE_COMPLEMENT 2
typedef struct sg_pbt_column {
    float *data;      /* the column's element of member 0 */
    int64_t stride;   /* elements between two members' rows */
    int32_t mode;     /* SG_PBT_COPY / SG_PBT_SCALE / SG_PBT_SCALE_COMPLEMENT */
    float down;       /* the factor drawn with probability 1/2 (0.8) */
    float up;         /* the other one (1.25) */
    float lo;         /* the clamp; -inf: none */
    float hi;         /* +inf: none */
} sg_pbt_column;
int sg_pbt_explore_device(sg_env *env, int32_t members, const int32_t *src, int32_t n_columns, const sg_pbt_column *columns, uint64_t seed,
                          uint64_t step, const int64_t *step_dev, int32_t *refused_out, void *hip_stream);

/* SHUFFLED MINIBATCH INDICES of an on-policy update, drawn on the device: the int64 index that sg_ppo_grad_device and
 * sg_ppo_population_grad_device gather by, a fresh shuffle of the rollout's rows per epoch cut into minibatches, as a pure function
 * of (seed, step + step_dev[0], epoch, member, position).  One launch, no sort, no workspace, no atomics; takes the stream,
 * allocates nothing, never synchronises, hipGraph-capturable; the env's state is not read.  tests/minibatch_model.py states all of
 * it in NumPy and is the contract; DESIGN section 30 has the kernel.
 *   B = num_envs, P = members (1 .. 256, dividing B), E = B / P: member m owns the envs [m E, (m + 1) E) (the block rule of the
 *   population calls).  The rollout is K = steps rows of B envs flattened to rows t B + i, K B < 2^31.  M = minibatches.
 *   index_out  int64 DEVICE [epochs, M, P, n]: every [e, b] is a contiguous [P, n] block, sg_ppo_population_grad_device's index
 *              (with P = 1, sg_ppo_grad_device's [n]).
 * KEYS.  step' = step + step_dev[0] (a 64-bit wrapping sum; step_dev int64 DEVICE [1], may be NULL), so a captured graph draws
 * afresh when the caller bumps it inside the graph.  For member m and epoch e (0 .. 63), two Philox4x32-10 blocks, key = seed,
 * counter = ((e << 16) | (blk << 8) | m, step' lo, step' hi, 11) for blk = 0, 1 -- stream tag 11, after explore's 10 -- give the
 * round keys k[4 blk + i] = o_i.
 * ONE ENCRYPTION of x in [0, 2^bits), bits = max(2, bit_length(N - 1)), wa = bits / 2, wb = bits - wa: L = x >> wb,
 * R = x & (2^wb - 1), (a, b) = (wa, wb); for r = 0 .. 7: t = fmix32(R + k[r] mod 2^32) >> (32 - a), (L, R) = (R, L ^ t),
 * (a, b) = (b, a); the result is (L << b) | R.  fmix32 is murmur3's finaliser (x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13,
 * x *= 0xC2B2AE35, x ^= x >> 16).  An 8-round unbalanced Feistel network: a bijection of [0, 2^bits).
 * pi(j) encrypts j and encrypts again while the value is >= N (cycle walking): a bijection of [0, N); 2^bits < 2 N for N >= 3, so
 * fewer than 2 encryptions are expected.  (The kernel stops a walk after 64 encryptions, which no element is expected to reach.)
 * NOT CLAIMED: uniformity over all N! orders -- at tiny N the network is visibly non-uniform over them.  Single positions and pairs
 * are uniform at the sizes anyone trains with; tests/test_minibatch.py states the conditions.
 *   SG_MINIBATCH_ROW  N = K E, n = N / M (integer division); index[e, b, m, i] = (j / E) B + m E + (j mod E), j = pi_{m,e}(b n + i).
 *                     The N - M n < M rows left over are another set in every epoch.
 *   SG_MINIBATCH_ENV  whole env columns stay together: N = E, c = E / M, n = K c; index[e, b, m, t c + i] = t B + m E + pi_{m,e}(b c + i):
 *                     a time-major [K, c] view.
 * Within one (e, m) all M n entries are distinct and lie in member m's env block.
 * sg_minibatch_size returns n, or -1 and a message for a shape that sg_minibatch_index_device refuses.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): steps < 1; members outside 1 .. 256 or not dividing num_envs; epochs
 * outside 1 .. 64; minibatches < 1; n < 1; K B >= 2^31; an unknown unit; a null index_out. */
#define SG_MINIBATCH_ROW 0
#define SG_MINIBATCH_ENV 1
int64_t sg_minibatch_size(sg_env *env, int32_t steps, int32_t members, int32_t minibatches, int32_t unit);
int sg_minibatch_index_device(sg_env *env, int32_t steps, int32_t members, int32_t epochs, int32_t minibatches, int32_t unit, uint64_t seed,
                              uint64_t step, const int64_t *step_dev, int64_t *index_out, void *hip_stream);

/* The off-policy learner's nets (TD3 / DDPG): one or two Q critics on (obs, action) rows, their parameter gradients and d Q / d action,
 * and the actor's action as a differentiable function of its parameters, so that a critic's d Q / d a reaches the actor on the device.
 * Continuous ids only (a 2-vector action); a discrete id is refused with a message.  The reference has no counterpart.
 *   critic c   x = [obs[0 .. obs_dim) | action[0 .. 2)]:  obs_dim + 2 -> hidden (x n_hidden) -> 1
 * Every hidden layer is followed by the activation; the head is linear.  Parameters are float32 DEVICE pointers in torch.nn.Linear
 * layout (weight[0] is [hidden, obs_dim + 2]), owned by the caller and read in place at every call, like sg_policy's; a target
 * network is simply a second sg_qnet.  The action is used AS GIVEN: nothing here clamps it -- the caller decides whether a critic
 * sees the stored unclamped action or a clamped one.  Arithmetic: sg_policy's -- float32 throughout, output neuron j starts at b[j]
 * and takes fmaf(W[j][k], x[k], .) for k = 0, 1, ..., one row per lane, no atomics: a row's Q depends on that row and the parameters
 * only.  tests/q_model.py states all of it in NumPy; DESIGN section 19 has the kernels and the tolerances. */
typedef struct sg_qnet {
    uint32_t struct_size;  /* sizeof(sg_qnet) */
    int32_t n_critics;     /* 1 or 2 */
    int32_t n_hidden;      /* hidden layers of each critic, 1 .. 3 */
    int32_t hidden;        /* their width, 1 .. 128 */
    int32_t activation;    /* SG_POLICY_TANH / SG_POLICY_RELU */
    sg_policy_mlp critic[2];  /* critic[1] is ignored when n_critics is 1 */
} sg_qnet;
/* q1_out, q2_out float32 [n] = Q_1, Q_2 of the rows obs float32 [n, obs_dim], action float32 [n, 2], any n >= 1, in ONE launch on the
 * stream, one critic after the other.  Either may be NULL (that critic is not evaluated), not both; q2_out needs n_critics == 2.
 * Allocates nothing, never synchronises, hipGraph-capturable.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): a discrete id; a null qnet or a wrong struct_size; n_critics outside
 * 1 .. 2, n_hidden outside 1 .. 3, hidden outside 1 .. 128, an unknown activation; a null weight or bias among the layers in use;
 * n < 1; a null obs or action; no output; q2_out with one critic. */
int sg_q_evaluate_device(sg_env *env, const sg_qnet *qnet, int64_t n, const float *obs, const float *action, float *q1_out,
                         float *q2_out, void *hip_stream);
/* Writable float32 device pointers, one per parameter of an sg_qnet and of its shape */
typedef struct sg_qnet_grads {
    uint32_t struct_size;  /* sizeof(sg_qnet_grads) */
    uint32_t reserved;     /* 0 */
    sg_policy_grads_mlp critic[2];  /* a critic's slots may be all NULL when its g_q is NULL; given without it they are written with zeros */
} sg_qnet_grads;
/* g_q1, g_q2 float32 [n]: the loss's gradients by the two outputs of sg_q_evaluate_device; each may be NULL (zeros).
 *   grads         receives sum_i g_qc[i] d Q_c[i] / d theta for every weight and bias of critic c: WRITTEN, not accumulated.  NULL: the
 *                 critics are frozen and only the action gradient is wanted; then no weight-gradient work and no reduction is enqueued
 *                 and the workspace is not looked at.
 *   g_action_out  float32 [n, 2], may be NULL: receives sum_c g_qc[i] d Q_c[i] / d action[i], critic 1's term added to critic 0's.  Per
 *                 row, no reduction over the batch: a function of the row, its g values and the parameters only -- it does not depend
 *                 on n, on the row's position or on whether grads is given (same bits).
 * tanh' = 1 - h^2 of the activation h; relu' = [pre-activation > 0]: 0 at 0, as torch.  The forward pass is recomputed inside the
 * launch.  With grads: two launches, the backward, whose workgroups leave partial sums in `workspace` (at least
 * sg_q_grad_workspace_bytes(env, qnet, n) bytes of device memory, any content), and a reduction of the partials in workgroup order;
 * float32 throughout, no atomics, a fixed summation order over the rows that is a function of n: the same inputs and the same n give
 * the same bits.  Allocates nothing, never synchronises, hipGraph-capturable.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): whatever sg_q_evaluate_device refuses of the qnet and the rows; g_q2, or
 * gradient slots of critic 1, with one critic; neither grads nor g_action_out; a wrong struct_size or reserved of grads; a null
 * pointer among the slots of a critic whose g_q is given; with grads, a null workspace or one smaller than the query's answer. */
int sg_q_grad_device(sg_env *env, const sg_qnet *qnet, int64_t n, const float *obs, const float *action, const float *g_q1,
                     const float *g_q2, const sg_qnet_grads *grads, float *g_action_out, void *workspace, size_t workspace_bytes,
                     void *hip_stream);
/* Bytes of workspace sg_q_grad_device needs for n rows when grads is given (it grows with n up to a cap); 0 and an error message for
 * an invalid qnet or n */
size_t sg_q_grad_workspace_bytes(sg_env *env, const sg_qnet *qnet, int64_t n);
/* The actor's side of the chain, on an sg_policy of a continuous id (a discrete id is refused; the policy's critic is not used).
 * action_out float32 [n, 2] = mean(obs) + exp(log_std) * eps for the rows obs float32 [n, obs_dim] and the caller's noise eps float32
 * [n, 2], UNCLAMPED.  eps NULL: the mean -- for the same rows bit for bit sg_policy_act_device's deterministic action; exp(log_std) is
 * that kernel's own expression.  One launch; allocates nothing, never synchronises, hipGraph-capturable.
 * Refused: whatever sg_policy_act_device refuses of the policy; a discrete id; n < 1; a null obs or action_out. */
int sg_policy_action_device(sg_env *env, const sg_policy *policy, int64_t n, const float *obs, const float *eps, float *action_out,
                            void *hip_stream);
/* grads->actor and grads->log_std receive sum_i sum_d g_action[i][d] d action[i][d] / d theta, g_action float32 [n, 2] (e.g.
 * sg_q_grad_device's g_action_out times the loss's sign): d a_d / d mean_d = 1, d a_d / d log_std_d = exp(log_std_d) eps[i][d] (0 with
 * a NULL eps).  WRITTEN, not accumulated; grads->critic is neither read nor written.  sg_policy_grad_device's two launches with another
 * score: the same workspace (sg_policy_grad_workspace_bytes(env, policy, n)), reduction and determinism.
 * Refused: whatever sg_policy_action_device refuses of the policy and the rows; a null g_action or grads, a wrong struct_size or
 * reserved; a null pointer among the actor's slots or log_std; a null workspace or one smaller than the query's answer. */
int sg_policy_action_grad_device(sg_env *env, const sg_policy *policy, int64_t n, const float *obs, const float *eps,
                                 const float *g_action, const sg_policy_grads *grads, void *workspace, size_t workspace_bytes,
                                 void *hip_stream);

/* The SAC actor: a Gaussian whose mean AND log_std depend on the state, squashed by tanh, with its log-prob (Jacobian term included)
 * and the reparametrised gradients of (action, logp) by the actor's parameters.  Continuous ids only (a discrete id is refused with a
 * message); the continuous ids clamp actions to [-1, 1]^2 on the device, so tanh needs no action scale.  The reference has no
 * counterpart.
 *   actor   obs_dim -> hidden (x n_hidden) -> 4     head outputs 0, 1: mean_d;  outputs 2, 3: raw_d (the unclamped log_std)
 * Parameters are float32 DEVICE pointers in torch.nn.Linear layout (the head is [4, hidden]), owned by the caller and read in place at
 * every call, like sg_policy's.  Per row, for d = 0, 1:
 *   ls_d  = min(max(raw_d, log_std_min), log_std_max)           (torch.clamp; SB3 uses -20, 2)
 *   u_d   = mean_d + exp(ls_d) * eps_d
 *   e_d   = exp(-2 |u_d|)
 *   a_d   = sign(u_d) (1 - e_d) / (1 + e_d)                     (= tanh u_d)
 *   ldj_d = 2 (ln 2 - |u_d| - log1p(e_d))                       (= log(1 - a_d^2), exact: finite when a_d rounds to +-1)
 *   logp  = sum_d(-eps_d^2 / 2 - ls_d - ln(2 pi) / 2 - ldj_d)
 * This is the log-prob of torch.distributions.TransformedDistribution(Normal, TanhTransform).  It is NOT SB3's log(1 - a^2 + 1e-6),
 * which loses all its digits in float32 once 1 - a^2 is near 1e-6 and caps the correction instead of following it.
 * Gradients treat eps as a constant (reparametrisation).  With g_action [n, 2] and g_logp [n], the loss's gradients by the outputs:
 *   gu_d      = g_action_d * 4 e_d / (1 + e_d)^2 + g_logp * 2 a_d
 *   dz_mean_d = gu_d
 *   dz_raw_d  = (gu_d * exp(ls_d) * eps_d - g_logp) * [log_std_min <= raw_d <= log_std_max]     (bounds inclusive, as torch.clamp's backward)
 * Arithmetic: sg_policy's -- float32 throughout, output neuron j starts at b[j] and takes fmaf(W[j][k], h[k], .) for k = 0, 1, ...,
 * one row per lane; exp(ls), log1p and the Box-Muller are the precise library forms, e_d the fast exponential the tanh activation
 * uses.  Every call takes the stream, allocates nothing, never synchronises and is hipGraph-capturable.
 * tests/squashed_model.py states all of it in NumPy float64; DESIGN section 20 has the kernels and the tolerances. */
typedef struct sg_squashed_policy {
    uint32_t struct_size;  /* sizeof(sg_squashed_policy) */
    int32_t n_hidden;      /* hidden layers, 1 .. 3 */
    int32_t hidden;        /* their width, 1 .. 128 */
    int32_t activation;    /* SG_POLICY_TANH / SG_POLICY_RELU */
    float log_std_min;     /* the clamp of raw_d; finite, log_std_min <= log_std_max */
    float log_std_max;
    sg_policy_mlp actor;   /* the head is [4, hidden] */
    int32_t reserved;      /* 0 */
} sg_squashed_policy;
/* (action, logp) of the observation rows obs_dev float32 [num_envs, obs_dim] in ONE launch: action_out float32 [num_envs, 2] in
 * [-1, 1]; logp_out float32 [num_envs], may be NULL.  eps is the Box-Muller pair of one Philox block, key = seed, counter =
 * (env_index_base + i, step lo, step hi, 6) -- stream tag 6, after sg_policy's 5; deterministic != 0: eps = 0, nothing drawn.  Env i's
 * results depend on its row, the parameters and (seed, step, env_index_base + i) only.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): a discrete id; a null policy or a wrong struct_size or reserved; n_hidden
 * outside 1 .. 3, hidden outside 1 .. 128, an unknown activation; log_std_min > log_std_max or a bound that is not finite; a null weight
 * or bias among the layers in use; a null obs or action_out. */
int sg_squashed_act_device(sg_env *env, const sg_squashed_policy *sp, const float *obs_dev, uint64_t seed, uint64_t step,
                           int32_t deterministic, float *action_out, float *logp_out, void *hip_stream);
/* The same with the caller's noise eps float32 [n, 2] on rows obs float32 [n, obs_dim], any n >= 1 -- the update's actor loss, and the
 * critic target's (a', logp') on next_obs.  eps NULL: zeros; for the same rows bit for bit the deterministic sg_squashed_act_device.
 * One launch.  Refused: whatever sg_squashed_act_device refuses of the policy; n < 1; a null obs or action_out. */
int sg_squashed_sample_device(sg_env *env, const sg_squashed_policy *sp, int64_t n, const float *obs, const float *eps,
                              float *action_out, float *logp_out, void *hip_stream);
typedef struct sg_squashed_grads {
    uint32_t struct_size;  /* sizeof(sg_squashed_grads) */
    uint32_t reserved;     /* 0 */
    sg_policy_grads_mlp actor;
} sg_squashed_grads;
/* grads->actor receives sum_i (g_action[i] . d action[i] + g_logp[i] d logp[i]) / d theta for every weight and bias: WRITTEN, not
 * accumulated.  g_action float32 [n, 2] and g_logp float32 [n] are the loss's gradients by sg_squashed_sample_device's outputs at the
 * same (obs, eps); each may be NULL (zeros), not both.  The forward pass is recomputed inside the launch.  Two launches, exactly
 * sg_policy_grad_device's scheme: the backward, whose workgroups leave partial sums in `workspace` (at least
 * sg_squashed_grad_workspace_bytes(env, sp, n) bytes of device memory, any content), and a reduction of the partials in workgroup
 * order; no atomics, a fixed summation order that is a function of n: the same inputs and the same n give the same bits.
 * Refused: whatever sg_squashed_sample_device refuses of the policy and the rows; both g NULL; a null grads, a wrong struct_size or
 * reserved; a null pointer among the actor's slots in use; a null workspace or one smaller than the query's answer. */
int sg_squashed_grad_device(sg_env *env, const sg_squashed_policy *sp, int64_t n, const float *obs, const float *eps,
                            const float *g_action, const float *g_logp, const sg_squashed_grads *grads, void *workspace,
                            size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_squashed_grad_device needs for n rows (it grows with n up to a cap); 0 and an error message for an invalid
 * policy or n */
size_t sg_squashed_grad_workspace_bytes(sg_env *env, const sg_squashed_policy *sp, int64_t n);
/* n_steps closed-loop steps without a host synchronisation: sg_rollout_policy_device's loop with sg_squashed_act_device and no critic.
 * obs float32 [n_steps + 1, num_envs, obs_dim] with the current observations in row 0; action float32 [n_steps, num_envs, 2]; logp (may
 * be NULL), reward, done, truncated [n_steps, num_envs].  For every t the call enqueues the act kernel with step = first_step + t, then
 * the single step sg_step_device enqueues, then the terminal list's records (terminal_list may be NULL; filled as by
 * sg_rollout_policy_device): every output is bit for bit what that hand-written loop gives, with normalization on as well.  The
 * buffers may be a replay ring's rows.
 * Refused as sg_squashed_act_device refuses, and: n_steps < 1, a null obs, action, reward, done or truncated, an incomplete list. */
int sg_rollout_squashed_device(sg_env *env, int32_t n_steps, const sg_squashed_policy *sp, uint64_t seed, uint64_t first_step,
                               int32_t deterministic, float *obs, float *action, float *logp, float *reward, uint8_t *done,
                               uint8_t *truncated, const sg_terminal_list *terminal_list, void *hip_stream);

/* The DQN head: one MLP Q(obs) -> 6 on the discrete ids (GoalDiscrete{2,3,4}-v0, KeplerDiscrete-v0), epsilon-greedy acting, the Q values
 * a TD target and a TD loss need, and the gradients of a loss on them by the net's parameters -- DQN / Double DQN, with a per-env epsilon
 * as Ape-X runs it on a wide vector env.  Discrete ids only (a continuous id is refused with a message).  The reference has no counterpart.
 *   net   obs_dim -> hidden (x n_hidden) -> 6       head output j: Q(obs, action j)
 * Every hidden layer is followed by the activation; the head is linear.  Parameters are float32 DEVICE pointers in torch.nn.Linear
 * layout (the head is [6, hidden]), owned by the caller and read in place at every call, like sg_policy's; a target network is simply
 * a second sg_dqn.  Arithmetic: sg_policy's -- float32 throughout, output neuron j starts at b[j] and takes fmaf(W[j][k], h[k], .) for
 * k = 0, 1, ..., one row per lane, no atomics: a row's six Q values depend on that row and the parameters only.  "argmax" is always the
 * FIRST j whose Q_j is the largest (a NaN Q_0 gives 0).  Every call takes the stream, allocates nothing, never synchronises and is
 * hipGraph-capturable.  tests/dqn_model.py states all of it in NumPy; DESIGN section 22 has the kernels and the tolerances. */
typedef struct sg_dqn {
    uint32_t struct_size;  /* sizeof(sg_dqn) */
    int32_t n_hidden;      /* hidden layers, 1 .. 3 */
    int32_t hidden;        /* their width, 1 .. 128 */
    int32_t activation;    /* SG_POLICY_TANH / SG_POLICY_RELU */
    int32_t reserved;      /* 0 */
    sg_policy_mlp net;     /* the head is [6, hidden] */
} sg_dqn;
/* Epsilon-greedy actions of the observation rows obs_dev float32 [num_envs, obs_dim] in ONE launch: action_out int32 [num_envs];
 * q_out float32 [num_envs], may be NULL: the Q value of the action TAKEN.  Env i draws one Philox block o, key = seed, counter =
 * (env_index_base + i, step lo, step hi, 7) -- stream tag 7, after the squashed actor's 6 -- and
 *   explores iff u23(o0) < eps_i, u23(w) = ((w >> 9) + 0.5) / 2^23;  its action is then floor(o1 * 6 / 2^32), uniform on 0 .. 5 in exact
 *   integer arithmetic;  otherwise it takes the argmax.
 * eps_i is epsilon_dev[i] when epsilon_dev (float32 [num_envs], DEVICE memory) is given, else the host scalar epsilon: a captured graph
 * anneals epsilon by writing that tensor, and every env may have its own (Ape-X).  With epsilon_dev NULL and epsilon == 0 nothing is
 * drawn.  The values of epsilon_dev are not checked: <= 0 (or NaN) never explores, >= 1 always does, by the comparison.  Env i's
 * results depend on its row, the parameters, eps_i and (seed, step, env_index_base + i) only.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): a continuous id; a null dqn or a wrong struct_size or reserved; n_hidden
 * outside 1 .. 3, hidden outside 1 .. 128, an unknown activation; a null weight or bias among the layers in use; a null obs_dev or
 * action_out; an epsilon that is NaN or outside [0, 1] (checked with epsilon_dev given as well). */
int sg_dqn_act_device(sg_env *env, const sg_dqn *dqn, const float *obs_dev, uint64_t seed, uint64_t step, float epsilon,
                      const float *epsilon_dev, int32_t *action_out, float *q_out, void *hip_stream);
/* n_steps closed-loop steps without a host synchronisation: sg_rollout_squashed_device's loop with sg_dqn_act_device.  obs float32
 * [n_steps + 1, num_envs, obs_dim] with the current observations in row 0; action int32 [n_steps, num_envs]; q (may be NULL), reward,
 * done, truncated [n_steps, num_envs].  For every t the call enqueues the act kernel with step = first_step + t (epsilon_dev is read by
 * every one of them), then the single step sg_step_device enqueues, then the terminal list's records (terminal_list may be NULL;
 * filled as by sg_rollout_policy_device): every output is bit for bit what that hand-written loop gives, with normalization on as
 * well.  The buffers may be a replay ring's rows.
 * Refused as sg_dqn_act_device refuses, and: n_steps < 1, a null obs, action, reward, done or truncated, an incomplete list. */
int sg_rollout_dqn_device(sg_env *env, int32_t n_steps, const sg_dqn *dqn, uint64_t seed, uint64_t first_step, float epsilon,
                          const float *epsilon_dev, float *obs, int32_t *action, float *q, float *reward, uint8_t *done,
                          uint8_t *truncated, const sg_terminal_list *terminal_list, void *hip_stream);
/* The Q values of the rows obs float32 [n, obs_dim], any n >= 1, in ONE launch:
 *   q_all_out    float32 [n, 6]
 *   q_taken_out  float32 [n] = Q[i][action[i]], action int32 [n], 0 .. 5 (any other value is the caller's error -- the kernels select by
 *                comparison and never index with it, so it cannot reach out of bounds)
 *   q_max_out    float32 [n] = max_j Q[i][j];  argmax_out int32 [n], the first argmax
 * Each output may be NULL, not all four; action may be NULL when q_taken_out is.  q_taken, q_max and argmax are elements of q_all, bit
 * for bit, and for the rows sg_dqn_act_device saw q_all / argmax are that kernel's bits (one device function serves both).  Plain DQN's
 * target is q_max_out of the target net; Double DQN's is two calls: argmax_out of the online net on next_obs, then q_taken_out of the
 * target net with it as action.
 * Refused: whatever sg_dqn_act_device refuses of the dqn; n < 1; a null obs; no output; q_taken_out with a null action. */
int sg_dqn_evaluate_device(sg_env *env, const sg_dqn *dqn, int64_t n, const float *obs, const int32_t *action, float *q_all_out,
                           float *q_taken_out, float *q_max_out, int32_t *argmax_out, void *hip_stream);
typedef struct sg_dqn_grads {
    uint32_t struct_size;  /* sizeof(sg_dqn_grads) */
    uint32_t reserved;     /* 0 */
    sg_policy_grads_mlp net;
} sg_dqn_grads;
/* grads->net receives sum_i sum_j dz_ij d Q_j[i] / d theta for every weight and bias, dz_ij = g_all[i][j] + [j == action[i]] g_taken[i]:
 * WRITTEN, not accumulated.  g_taken float32 [n] and g_all float32 [n, 6] are the loss's gradients by sg_dqn_evaluate_device's q_taken_out
 * and q_all_out at the same (obs, action); each may be NULL (zeros), not both; action is needed when g_taken is given and not looked at
 * otherwise.  g_all serves losses on all six values (a CQL logsumexp term, discrete SAC / soft Q) without another kernel.
 * tanh' = 1 - h^2 of the activation h; relu' = [pre-activation > 0]: 0 at 0, as torch.  The forward pass is recomputed inside the
 * launch.  Two launches, exactly sg_policy_grad_device's scheme: the backward, whose workgroups leave partial sums in `workspace` (at
 * least sg_dqn_grad_workspace_bytes(env, dqn, n) bytes of device memory, any content), and a reduction of the partials in workgroup
 * order; no atomics, a fixed summation order that is a function of n: the same inputs and the same n give the same bits.
 * Refused: whatever sg_dqn_evaluate_device refuses of the dqn and the rows; both g NULL; g_taken with a null action; a null grads, a wrong
 * struct_size or reserved; a null pointer among the net's gradient slots in use; a null workspace or one smaller than the query's answer. */
int sg_dqn_grad_device(sg_env *env, const sg_dqn *dqn, int64_t n, const float *obs, const int32_t *action, const float *g_taken,
                       const float *g_all, const sg_dqn_grads *grads, void *workspace, size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_dqn_grad_device needs for n rows (it grows with n up to a cap); 0 and an error message for an invalid dqn or n */
size_t sg_dqn_grad_workspace_bytes(sg_env *env, const sg_dqn *dqn, int64_t n);

/* THE DQN / DOUBLE DQN TD UPDATE IN ONE CALL: from a replay batch (sg_replay_sample_device's columns), an online and a target sg_dqn of
 * one architecture to the TD target, the Huber loss, its statistics and the ONLINE net's parameter gradients -- the two
 * sg_dqn_evaluate_device calls on next_obs, the target arithmetic, the loss and sg_dqn_grad_device of a hand-composed update, without
 * autograd.  For row i, with Q the six head outputs, argmax and Q[a] exactly sg_dqn_evaluate_device's:
 *     a*      = argmax Q_online(next_obs[i])                                   (double_q; the first maximum)
 *     q_next  = Q_target(next_obs[i])[a*]                                      (double_q == 0: max_j Q_target(next_obs[i])[j])
 *     y       = terminated[i] ? reward[i] : reward[i] + discount[i] * q_next   the product rounded, then the sum: never an fma
 *     q_taken = Q_online(obs[i])[action[i]];  td = q_taken - y
 *     c       = min(max(td, -huber_delta), +huber_delta);  w = weight ? weight[i] : 1
 *     g       = (w * c) / (float)n                                             the product rounded, then the quotient
 *     loss    = (1 / n) sum_i w * (|td| <= huber_delta ? 0.5 td^2 : huber_delta (|td| - 0.5 huber_delta))
 * and g goes to sg_dqn_grad_device's backward as g_taken.  discount is the batch's per-row column (gamma^steps as the n-step sampler
 * writes it): there is no separate gamma.  A terminated row never multiplies its q_next (an infinite one leaves y = reward).
 * huber_delta = +inf gives the squared loss 0.5 td^2.  Everything is float32.  Every other loss on the Q values goes through
 * sg_dqn_evaluate_device / sg_dqn_grad_device. */
typedef struct sg_dqn_td_config {
    uint32_t struct_size; /* sizeof(sg_dqn_td_config) */
    int32_t double_q;     /* default 1; 0: plain DQN, the target net's maximum */
    float huber_delta;    /* > 0; +inf: the squared loss.  Default 1 */
    int32_t reserved;     /* 0 */
} sg_dqn_td_config;
void sg_dqn_td_config_init(sg_dqn_td_config *cfg);
/* Device pointers to the n rows of the batch */
typedef struct sg_dqn_td_batch {
    const float *obs;          /* float32 [n, obs_dim] */
    const int32_t *action;     /* int32 [n], 0 .. 5 */
    const float *reward;       /* float32 [n] (the n-step return's reward part) */
    const float *next_obs;     /* float32 [n, obs_dim] */
    const uint8_t *terminated; /* uint8 [n] */
    const float *discount;     /* float32 [n] */
    const float *weight;       /* float32 [n] importance weights on the loss; may be NULL (ones) */
} sg_dqn_td_batch;
/* Optional per-row outputs, float32 [n], each may be NULL: the numbers the kernels used for row i */
typedef struct sg_dqn_td_rows {
    float *td_error; /* q_taken - y, signed: what sg_priority_update_device's caller raises to alpha */
    float *q_taken;
    float *target;   /* y */
    float *q_next;
    float *g;
} sg_dqn_td_rows;
/* grads (an sg_dqn_grads with every slot of the net given) receives d loss / d theta of the ONLINE net, WRITTEN, not accumulated: bit
 * for bit what sg_dqn_grad_device gives at the same n for (obs, action) with g_taken = row_out->g.  row_out->q_next / q_taken are
 * sg_dqn_evaluate_device's bits for the same rows.
 * stats_out float32 [8]: loss, td_abs_mean = mean |td|, td_abs_max = max |td| (exactly the largest |row_out->td_error|), q_mean = mean
 * q_taken, target_mean = mean y, clip_fraction = mean(|td| > huber_delta), weight_mean, bad_rows.
 * An action outside 0 .. 5 is never an index (every selection compares); such a row contributes zero to every gradient and statistic,
 * reports g = 0 and td_error = 0, is counted in bad_rows, and the means still divide by n.
 * Launches: the target (sg_dqn_evaluate_device's kernel frame; with double_q the online net, then the target net in the same LDS),
 * which leaves y in `workspace`; the backward -- sg_dqn_grad_device's kernel frame with the loss gradient formed from the head outputs,
 * every workgroup leaving its statistics sums beside its partial sums; the reduction in workgroup order.  `workspace`: at least
 * sg_dqn_td_grad_workspace_bytes(env, online, n) bytes of device memory, any content.  Allocates nothing, never synchronises,
 * hipGraph-capturable.  No atomics: the same inputs and the same n give the same bits.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): whatever sg_dqn_act_device refuses of either dqn (a continuous id
 * among it); nets that differ in n_hidden, hidden or activation; a null cfg, a wrong struct_size or reserved; a huber_delta that is
 * NaN or not > 0; n outside 1 .. 2^31 - 1; a null batch, obs, action, reward, next_obs, terminated or discount; a null stats_out; what
 * sg_dqn_grad_device refuses of grads; a null workspace or one smaller than the query's answer. */
int sg_dqn_td_grad_device(sg_env *env, const sg_dqn *online, const sg_dqn *target, const sg_dqn_td_config *cfg, const sg_dqn_td_batch *batch,
                          int64_t n, const sg_dqn_grads *grads, float *stats_out, const sg_dqn_td_rows *row_out, void *workspace,
                          size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_dqn_td_grad_device needs for n rows: sg_dqn_grad_workspace_bytes', the statistics partials and y float32 [n];
 * 0 and an error message for an invalid dqn or n */
size_t sg_dqn_td_grad_workspace_bytes(sg_env *env, const sg_dqn *online, int64_t n);

/* THE TD CRITIC UPDATE OF SAC, TD3 AND DDPG IN ONE CALL: from a replay batch (sg_replay_sample_device's columns), the target action the
 * caller formed, an online and a target sg_qnet of one shape to the TD target, the Huber loss, its statistics and the ONLINE critics'
 * parameter gradients -- the target critics' sg_q_evaluate_device, the minimum, SAC's entropy term or TD3's target smoothing, the loss and
 * sg_q_grad_device of a hand-composed update, without autograd.  THE TARGET ACTION IS AN INPUT: next_action (and SAC's next_logp) come
 * from one launch of the caller's actor on next_obs (sg_squashed_act_device, or sg_policy_action_device on the target actor), so the
 * call fixes no actor's form.  For row i, with Qc the critic c of sg_q_evaluate_device on [obs | action], bit for bit:
 *     a'_d    = next_action[i][d]
 *               noise given:  e = min(max(noise_std * noise[i][d], -noise_clip), noise_clip)
 *                             a'_d = min(max(a'_d + e, -action_clip), action_clip)            (noise NULL: a' used as given, never clamped)
 *     q_next  = min(Q1_target(next_obs[i], a'), Q2_target(next_obs[i], a'))                   (one critic: Q1_target)
 *               next_logp given:  q_next = q_next - alpha * next_logp[i]                      (alpha = *alpha_dev when given, else cfg.alpha)
 *     y       = terminated[i] ? reward[i] : reward[i] + discount[i] * q_next                  a select; every product rounded, never an fma
 *     per critic c of the ONLINE qnet:  q_c = Qc(obs[i], action[i]);  td_c = q_c - y
 *               cl_c = min(max(td_c, -huber_delta), huber_delta);  w = weight ? weight[i] : 1;  g_c = (w * cl_c) / (float)n
 *               l_c  = w * (|td_c| <= huber_delta ? 0.5 td_c^2 : huber_delta (|td_c| - 0.5 huber_delta))
 *     loss    = (1 / n) sum_i (l_1 + l_2)
 * and g_c goes to sg_q_grad_device's backward as g_qc.  discount is the batch's per-row column (gamma^steps as the n-step sampler writes
 * it): there is no separate gamma.  A terminated row never multiplies its q_next (an infinite one leaves y = reward).  huber_delta =
 * +inf, the default, gives 0.5 td^2 per critic: HALF of the sum of the two mean squared errors that CleanRL's and SB3's TD3 / SAC
 * minimise (their gradients are twice these); there is no scale parameter -- fold the factor into the learning rate.  Every min, max
 * and clamp hands a NaN on, as torch.minimum and torch.clamp do: non-finite inputs propagate as they do in torch, and no row is set
 * aside.  Everything is float32.  The actor's and alpha's steps are not part of this: the actor's is sg_q_actor_squashed_grad_device /
 * sg_q_actor_gaussian_grad_device.  tests/q_td_model.py states all of it in NumPy; DESIGN section 32 has the kernels and the
 * tolerances. */
typedef struct sg_q_td_config {
    uint32_t struct_size; /* sizeof(sg_q_td_config) */
    float huber_delta;    /* > 0; +inf: the squared loss.  Default +inf */
    float alpha;          /* the entropy coefficient when batch.alpha_dev is NULL; read only with batch.next_logp.  Default 0.2 */
    float noise_std;      /* >= 0; read only with batch.noise.  Default 0.2 */
    float noise_clip;     /* >= 0, +inf: none.  Default 0.5 */
    float action_clip;    /* >= 0, +inf: none; a' is clamped only when batch.noise is given.  Default 1 */
    int32_t reserved[2];  /* 0 */
} sg_q_td_config;
void sg_q_td_config_init(sg_q_td_config *cfg);
/* Device pointers to the n rows of the batch */
typedef struct sg_q_td_batch {
    const float *obs;          /* float32 [n, obs_dim] */
    const float *action;       /* float32 [n, 2] */
    const float *reward;       /* float32 [n] (the n-step return's reward part) */
    const float *next_obs;     /* float32 [n, obs_dim] */
    const uint8_t *terminated; /* uint8 [n] */
    const float *discount;     /* float32 [n] */
    const float *next_action;  /* float32 [n, 2]: the actor's action at next_obs */
    const float *weight;       /* float32 [n] importance weights on the loss; may be NULL (ones) */
    const float *next_logp;    /* float32 [n] log-prob of next_action (SAC); may be NULL: no entropy term */
    const float *alpha_dev;    /* one float32 on the device, read by the kernel, so that a learned alpha changes inside a captured graph;
                                  may be NULL (cfg.alpha); needs next_logp */
    const float *noise;        /* float32 [n, 2] standard normal draws (TD3's target smoothing); may be NULL: a' = next_action */
} sg_q_td_batch;
/* Optional per-row outputs, float32 [n], each may be NULL: the numbers the kernels used for row i */
typedef struct sg_q_td_rows {
    float *td1;    /* q_1 - y, signed */
    float *td2;
    float *q1;
    float *q2;
    float *target; /* y */
    float *q_next; /* after the entropy term */
    float *g1;
    float *g2;
    float *td_abs; /* 0.5 (|td1| + |td2|); one critic: |td1|.  What sg_priority_update_device's caller raises to alpha */
} sg_q_td_rows;
/* grads (an sg_qnet_grads with every slot of every critic in use given) receives d loss / d theta of the ONLINE critics, WRITTEN, not
 * accumulated: bit for bit what sg_q_grad_device gives at the same n for (obs, action) with g_q1 = row_out->g1, g_q2 = row_out->g2.
 * row_out->q1 / q2 are sg_q_evaluate_device's bits of the online qnet for the same rows; row_out->q_next before the entropy term is
 * the minimum of the target qnet's at (next_obs, a').
 * stats_out float32 [9]: loss, td1_abs_mean = mean |td1|, td2_abs_mean, td_abs_max = max over both critics (exactly the largest of
 * |row_out->td1| and |row_out->td2|), q1_mean, q2_mean, target_mean = mean y, clip_fraction = #(|td_c| > huber_delta) / (critics * n),
 * weight_mean.  With one critic the critic-2 entries are 0.
 * Launches: the target (sg_q_evaluate_device's kernel frame on the target qnet, a' in registers, critic 0 and then critic 1 in the same
 * LDS), which leaves y in `workspace`; the backward -- sg_q_grad_device's kernel frame with no action gradient and the loss gradient
 * formed from the head output, every workgroup leaving its statistics sums beside its partial sums; the reduction in workgroup order.
 * `workspace`: at least sg_q_td_grad_workspace_bytes(env, online, n) bytes of device memory aligned to 4, any content.  Allocates
 * nothing, never synchronises, hipGraph-capturable.  Every sum has a fixed order that is a function of n: the same inputs and the same
 * n give the same bits.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): a discrete id; whatever sg_q_evaluate_device refuses of either qnet; qnets
 * that differ in n_critics, n_hidden, hidden or activation; a null cfg, a wrong struct_size or reserved; a huber_delta that is NaN or
 * not > 0; a negative or NaN noise_std, noise_clip or action_clip; n outside 1 .. 2^31 - 1; a null batch, obs, action, reward, next_obs,
 * terminated, discount or next_action; alpha_dev without next_logp; td2, q2 or g2 of row_out with one critic; a null stats_out; what
 * sg_q_grad_device refuses of grads (grads is mandatory here); a null, short or misaligned workspace. */
int sg_q_td_grad_device(sg_env *env, const sg_qnet *online, const sg_qnet *target, const sg_q_td_config *cfg, const sg_q_td_batch *batch,
                        int64_t n, const sg_qnet_grads *grads, float *stats_out, const sg_q_td_rows *row_out, void *workspace,
                        size_t workspace_bytes, void *hip_stream);
/* Bytes of workspace sg_q_td_grad_device needs for n rows: sg_q_grad_workspace_bytes', 36 bytes of statistics partials per workgroup and
 * y float32 [n]; 0 and an error message for an invalid qnet or n */
size_t sg_q_td_grad_workspace_bytes(sg_env *env, const sg_qnet *online, int64_t n);

/* THE ACTOR UPDATE OF SAC, TD3 AND DDPG THROUGH THE TWIN Q CRITICS IN ONE CALL: from observations, the actor and an sg_qnet to the
 * action, the critics' values and action gradients, the loss mean(alpha logp - Q), its statistics and the ACTOR's parameter gradients --
 * sg_squashed_sample_device, sg_q_evaluate_device, the selection of the smaller critic, sg_q_grad_device for d Q / d action and
 * sg_squashed_grad_device (or sg_policy_action_device / sg_policy_action_grad_device) of a hand-composed step, without autograd and with
 * the critics run once.  Two entry points, one per actor struct, share everything else.  For row i, bit for bit:
 *     head     = actor MLP(obs[i])
 *     squashed: (a, logp) = sg_squashed_sample_device's of (head, eps[i])              (eps NULL: zeros)
 *     gaussian: a_d = fmaf(expf(log_std_d), eps[i][d], head_d), sg_policy_action_device's;  logp = 0 and alpha must be 0
 *     critic c: q_c = Qc(obs[i], a), sg_q_evaluate_device's;  dq_c[d] = 0.0f + d Qc / d a_d, sg_q_grad_device's g_action_out for g_qc = 1
 *     q_select = 1: both critics run, sel2 = q2 < q1 || q2 != q2 (ties to critic 1; a NaN q2 is taken, as torch.minimum hands it on)
 *     q_select = 0: critic 1 alone, sel2 = false
 *     q_sel = sel2 ? q2 : q1;  loss_i = alpha * logp - q_sel                     two roundings, never an fma; alpha = *alpha_dev when given
 *     g_action[d] = (-dq_sel[d]) / (float)n;  g_logp = alpha / (float)n
 * and (g_action, g_logp) go to sg_squashed_grad_device's backward (g_action to sg_policy_action_grad_device's).  The critics' parameters
 * get no gradient.  Everything is float32.  tests/q_actor_model.py states all of it in NumPy; DESIGN section 33 has the kernels. */
typedef struct sg_q_actor_config {
    uint32_t struct_size; /* sizeof(sg_q_actor_config) */
    float alpha;          /* >= 0: the entropy coefficient when alpha_dev is NULL; 0 for the Gaussian form.  Default 0.2 */
    float target_entropy; /* stats_out[8] = -(logp_mean + target_entropy).  Default -2 (minus the action dimensions) */
    int32_t q_select;     /* 1: the minimum of two critics; 0: critic 1; -1, the default: 1 for the squashed actor on two critics, else 0 */
    int32_t reserved[2];  /* 0 */
} sg_q_actor_config;
void sg_q_actor_config_init(sg_q_actor_config *cfg);
/* Optional per-row outputs, each may be NULL: the numbers the kernel used for row i */
typedef struct sg_q_actor_rows {
    float *action;   /* float32 [n, 2] */
    float *logp;     /* float32 [n] (the Gaussian form: 0) */
    float *q1;       /* float32 [n] */
    float *q2;       /* float32 [n]; q_select = 1 only */
    float *q_sel;    /* float32 [n] */
    float *dq1_da;   /* float32 [n, 2] */
    float *dq2_da;   /* float32 [n, 2]; q_select = 1 only */
    float *g_action; /* float32 [n, 2] */
} sg_q_actor_rows;
/* grads receives d loss / d theta of the actor (the Gaussian form: and of log_std), WRITTEN, not accumulated: bit for bit what
 * sg_squashed_grad_device gives for (obs, eps, g_action = row_out->g_action, g_logp = alpha / n) wherever the row tile of the larger of
 * the two nets' width classes (hidden up to 32 / 64 / 96 / 128: 256 / 128 / 64 / 64 rows) is the actor's own class's; with another tile
 * the same sums are grouped differently.  alpha_dev: one float32 on the device, read by the kernel, so that a learned temperature
 * changes inside a captured graph; may be NULL (cfg.alpha).
 * stats_out float32 [9]: loss, logp_mean, q1_mean, q2_mean (0 when critic 2 did not run), q_sel_mean, critic2_fraction = #sel2 / n,
 * action_abs_mean = mean 0.5 (|a_0| + |a_1|), dq_da_abs_max over the critics run and both components (a NaN entry makes it NaN, as it
 * makes the sums), log_alpha_grad = -(logp_mean + target_entropy): the gradient of SB3's temperature loss by log_alpha (the Gaussian
 * form: 0).  eps and the [n, 2] row outputs are read and written as pairs: aligned to 8 bytes, as a tensor's rows are.
 * Launches: the gradient kernel (sg_q_grad_device's kernel frame with both nets; per row tile the actor's forward, each critic's
 * forward and walk to the action, the actor's backward) and the reduction in workgroup order.  `workspace`: at least
 * sg_q_actor_grad_workspace_bytes(...) bytes of device memory aligned to 4, any content.  Allocates nothing, never synchronises,
 * hipGraph-capturable.  Every sum has a fixed order that is a function of n: the same inputs and the same n give the same bits.
 * Refused (SG_ERR_INVALID, with a message, nothing enqueued): a discrete id; whatever sg_squashed_sample_device / sg_policy_action_device
 * refuses of the actor and sg_q_evaluate_device of the qnet; a null cfg, a wrong struct_size or reserved; q_select outside -1 .. 1, or 1
 * with one critic; alpha NaN or negative; a non-zero alpha or an alpha_dev with the Gaussian form; a NaN target_entropy; n outside
 * 1 .. 2^31 - 1; a null obs, stats_out or grads; q2 or dq2_da of row_out when critic 2 does not run; what sg_squashed_grad_device /
 * sg_policy_action_grad_device refuse of grads; a null, short or misaligned workspace. */
int sg_q_actor_squashed_grad_device(sg_env *env, const sg_squashed_policy *actor, const sg_qnet *qnet, const sg_q_actor_config *cfg,
                                    int64_t n, const float *obs, const float *eps, const float *alpha_dev,
                                    const sg_squashed_grads *grads, float *stats_out, const sg_q_actor_rows *row_out, void *workspace,
                                    size_t workspace_bytes, void *hip_stream);
int sg_q_actor_gaussian_grad_device(sg_env *env, const sg_policy *actor, const sg_qnet *qnet, const sg_q_actor_config *cfg, int64_t n,
                                    const float *obs, const float *eps, const float *alpha_dev, const sg_policy_grads *grads,
                                    float *stats_out, const sg_q_actor_rows *row_out, void *workspace, size_t workspace_bytes,
                                    void *hip_stream);
/* Bytes of workspace either call needs for n rows, exactly one of the two actors given: per workgroup (of the larger class's tile, at
 * most 256) the actor's partial sums as its own grad call lays them out and 32 bytes of statistics partials; 0 and an error message for
 * an invalid actor, qnet or n */
size_t sg_q_actor_grad_workspace_bytes(sg_env *env, const sg_squashed_policy *squashed, const sg_policy *gaussian, const sg_qnet *qnet,
                                       int64_t n);

/* SpaceshipEnv.vector_field(raw_action, state_vec=None) (spaceship_env.py:96-100): the RHS of the ODE,
 * out float32 [num_envs, 6] = (vx, vy, omega', ax, ay, angular acceleration) at each env's current planets and either its
 * current ship state (ship == NULL) or the given one (float32 [num_envs, 6]).  Host arrays; actions as in sg_step. */
int sg_vector_field(sg_env *env, const void *actions_host, const float *ship_host, float *out_host);

/* Page-locked host memory for the arrays passed to sg_reset / sg_step (optional: any host memory works, pinned memory
 * makes the per-step copies plain DMA).  sg_host_alloc returns NULL on failure. */
void *sg_host_alloc(size_t bytes);
void sg_host_free(void *ptr);

/* Measurement aid (no reference counterpart): with profiling on, each step-kernel launch carries start/stop events
 * that timestamp the dispatch itself; sg_get_profile returns and clears the durations recorded so far (milliseconds).
 * The caller synchronises the stream(s) first. */
int sg_set_profiling(sg_env *env, int32_t on);
int sg_get_profile(sg_env *env, int64_t *launches, double *total_ms, double *min_ms, double *max_ms);

/* Measurement aid: name of the kernel (as rocprofv3 --kernel-trace prints it) that sg_rollout_device launches for n_steps
 * steps on this handle; valid until the next call on the handle. */
const char *sg_rollout_kernel(sg_env *env, int32_t n_steps);

/* The HIP stream the host-buffer calls run on (hipStream_t), for callers that want to order work after it.  Created by
 * sg_create, destroyed by sg_destroy: the value is valid for the lifetime of the handle and must not be destroyed by the caller. */
void *sg_stream(const sg_env *env);

const char *sg_version(void);

#ifdef __cplusplus
}
#endif
#endif
