// The body of goal_pair_rollout_kernel and goal_pair_rollout_profiled_kernel (sg_engine.hip), included by both.  A copy in each
// kernel rather than one inlined function: the kernel without profiles then compiles to the instructions it had before reward
// profiles existed.  SG_ROLLOUT_PROFILED 1: the reward's coefficients are the lane's env's profile (`rs`, a ProfileSource), and
// the replays read the profile of the env they replay (SG_ROLLOUT_RS: ", rs"; empty without profiles).

    const SgBuffers &b = *bufs;
    using Spare = SpareEpisode<N>;
    using Queue = EpisodeQueue<N>;
    using Integ = Integrator<N, N, true, ACCEL>;
    using Replay = GoalReplay<N>;
    __shared__ float spare[kSpare * Spare::kFields * kBlock];
    __shared__ float ring[kRing * kHand * kBlock];
    __shared__ float rbuf[(kBlock / 64) * Replay::kWords * kReplayCap];  // [pair][word][slot]
    __shared__ uint32_t spare_hi[kBlock];                    // per env: highest episode index present in `spare`
    __shared__ uint32_t handed[kBlock / 64], taken[kBlock / 64];  // per wave pair: steps published / steps read
    __shared__ uint32_t rp_tail[kBlock / 64];  // per wave pair: replay records read by the finisher (the pilot counts those it wrote)
    __shared__ uint32_t rp_claim[kBlock / 64], rp_done[kBlock / 64];  // records claimed for replaying; set once the pilot has integrated its share
    constexpr int D = 7 + 2 * N + 2;
    SG_REAL(0);
    const int tid = threadIdx.x & (kBlock - 1), pair = tid >> 6, lane = tid & 63;
    const bool pilot = threadIdx.x < kBlock;
    const int i = blockIdx.x * kBlock + tid;
    const bool live = i < num_envs;  // (num_envs comes with the kernel arguments: the state loads do not wait for the parameter block)
    const int ii = live ? i : 0;
    const int64_t B = num_envs;
    GoalEnv<N> e;
    load_goal_env<N>(b, ii, e);
    uint2 ct = b.ctr[ii];
    const SgDev &c = *cfg;
    {   // Touch every cache line of the parameter block now, all at once and under the state loads: its fields are read
        // where they are first needed, and in a fresh launch each first touch of a line is a cold miss in the middle of the
        // first step.
        const uint32_t *cw = reinterpret_cast<const uint32_t *>(cfg);
        uint32_t touch = 0u;
#pragma unroll
        for (int k = 0; k < (int)(sizeof(SgDev) / 4); k += 16) touch ^= cw[k];
        touch ^= cw[sizeof(SgDev) / 4 - 1];
        asm volatile("" ::"s"(touch));
    }
    const bool discrete = c.discrete_actions != 0;  // read once: inside the step loop it would be re-loaded every step
    float *const rb = rbuf + pair * Replay::kWords * kReplayCap;
    if (!pilot) spare_hi[tid] = ct.y;  // nothing beyond the current episode in LDS yet
    if (threadIdx.x < kBlock / 64) { handed[threadIdx.x] = 0u; taken[threadIdx.x] = 0u; rp_tail[threadIdx.x] = 0u; rp_claim[threadIdx.x] = 0u; rp_done[threadIdx.x] = 0u; }
    __syncthreads();  // the only workgroup barrier: flags and spare_hi initialised
    SG_REAL(1);

    if (pilot) {
        SG_ACC_DECL;
        __builtin_amdgcn_s_setprio(3);  // the pilot is the serial critical path of the pair (measured: -0.5 % at 1000 steps per launch)
        const bool hand_over = c.auto_reset && live;  // (read once) the env restarts after a terminal step: its terminal state is the finisher's
        const bool auto_reset = c.auto_reset != 0;
        // the parameters of a step, pinned in vector registers: left to the compiler they are re-read from the parameter block
        // at the top of every step (scalar registers are short), with the load's latency on this wave's critical path
        StepConsts kc = step_consts(c);
        asm volatile("" : "+v"(kc.max_engine_force), "+v"(kc.h), "+v"(kc.half_world), "+v"(kc.gm), "+v"(kc.omega_limit), "+v"(kc.planet_r),
                          "+v"(kc.max_thruster_force), "+v"(kc.inv_moi), "+v"(kc.planet_r_d));
        int max_steps = c.max_episode_steps;
        asm volatile("" : "+v"(max_steps));
        float2 a_next = load_action_raw(discrete, actions, ii);
        uint32_t taken_seen = 0u;  // the finisher's progress as last read (re-read only when the ring would wrap)
        uint32_t head = 0u, tail_seen = 0u;  // replay records written; read by the finisher (as last seen)
        for (int t = 0; t < n_steps; t++) {
            const float2 a = decode_action(discrete, a_next);
            if (t + 1 < n_steps) a_next = load_action_raw(discrete, actions, (int64_t)(t + 1) * B + ii);
            // ring slot of step t - kRing must have been read
            if (t - (int)taken_seen >= kRing && !wait_flag<SG_PILOT_SLEEP>(&taken[pair], (uint32_t)(t - kRing + 1), &taken_seen)) { *status = 1; break; }
            // room for 64 more replay records?  (else this step's terminal states are worked out here)
            if (head + 64u - tail_seen > (uint32_t)kReplayCap) tail_seen = lds_flag_load_uniform(&rp_tail[pair]);
            const bool defer = hand_over && head + 64u - tail_seen <= (uint32_t)kReplayCap;

            const int slot = t % kRing;
            StepResult r;
            int rk;
            {
                Integ I;
                SG_ACC(0);
                goal_env_begin<N, ACCEL>(kc, e, a.x, a.y, I);
                SG_ACC(1);
                rk = I.run(r, [&]() __attribute__((always_inline)) -> bool { return defer; });
                SG_ACC_ADD(7, __any(r.done) ? 1 : 0);
                SG_ACC_ADD(10, __any(r.path == kPathScipyErr || r.path == kPathScipyClear) ? 1 : 0);
                SG_ACC_ADD(11, __any((r.path == kPathScipyErr || r.path == kPathScipyClear) && r.n_rk > 1) ? 1 : 0);
                SG_ACC(2);
            }
            const bool replayed = rk == kRkEventDeferred;
            uint32_t rslot = 0u;  // this lane's replay record
            {   // replay records of the lanes whose terminal state is left to the finisher (the env as it was BEFORE the step)
                const unsigned long long dm = __ballot(replayed);
                if (dm) {
                    rslot = (head + (uint32_t)__popcll(dm & ((1ull << lane) - 1ull))) % (uint32_t)kReplayCap;
                    if (replayed) Replay::put(rb, rslot, ((uint32_t)t << 6) | (uint32_t)lane, e, a);
                    head += (uint32_t)__popcll(dm);
                }
            }
            // the state update of goal_env_finish (an env whose terminal state is replayed restarts below)
            e.x = (float)((double)e.x + r.dXd); e.y = (float)((double)e.y + r.dYd); e.vx = r.vx; e.vy = r.vy; e.om = r.om;
            e.th = wrap_two_pi(e.th + r.dth);
            SG_ACC(3);
            SG_ACC(4);
            {
                float *q = ring + (slot * kHand) * kBlock + tid;
                const uint64_t ux = __double_as_longlong(r.dXd), uy = __double_as_longlong(r.dYd);
                q[0 * kBlock] = __uint_as_float((uint32_t)ux); q[1 * kBlock] = __uint_as_float((uint32_t)(ux >> 32));
                q[2 * kBlock] = __uint_as_float((uint32_t)uy); q[3 * kBlock] = __uint_as_float((uint32_t)(uy >> 32));
                q[4 * kBlock] = e.th; q[5 * kBlock] = e.vx; q[6 * kBlock] = e.vy; q[7 * kBlock] = e.om;
                q[8 * kBlock] = __uint_as_float((uint32_t)r.done | (replayed ? 2u | (rslot << 8) : 0u));
            }
            lds_flag_store(&handed[pair], (uint32_t)(t + 1));  // release: the step record and the replay records are visible before the counter
            SG_ACC(5);
            // gym.wrappers.TimeLimit + auto-reset, as in pair_step
            const uint32_t el = ct.x + 1u;
            const int trunc = !r.done && (int)el >= max_steps;
            const bool restart = live && (r.done | trunc) && auto_reset;
            if (live) ct.x = el;
            if (restart) {
                const uint32_t k = ct.y + 1u;
                if ((int32_t)(lds_flag_load(&spare_hi[tid]) - k) >= 0) {
                    const float *q = spare + ((int)(k % (uint32_t)kSpare) * Spare::kFields) * kBlock + tid;
                    e.x = q[0 * kBlock]; e.y = q[1 * kBlock]; e.th = q[2 * kBlock]; e.vx = q[3 * kBlock];
                    e.vy = q[4 * kBlock]; e.om = q[5 * kBlock];
#pragma unroll
                    for (int j = 0; j < N; j++) { e.px[j] = q[(8 + 2 * j) * kBlock]; e.py[j] = q[(9 + 2 * j) * kBlock]; }
                } else {  // not generated yet (start of a launch, or restarts in consecutive steps)
                    Tiling T;
                    T.episode = k;
                    ShipInit s;
                    float gx, gy;
                    goal_reset<N>(c, c.env_index_base + (uint32_t)i, T, s, e.px, e.py, gx, gy);
                    e.x = s.x; e.y = s.y; e.th = s.th; e.vx = s.vx; e.vy = s.vy; e.om = s.om;
                }
                ct = make_uint2(0u, k);
            }
            SG_ACC(8);
        }
        SG_ACC_WRITE(blockIdx.x * 8 + pair);
        SG_REAL(2);
        if (live) {  // final hot state; the goal half of q1 belongs to the finisher
            b.q0[i] = make_float4(e.x, e.y, e.th, e.vx);
            reinterpret_cast<float2 *>(b.q1 + i)[0] = make_float2(e.vy, e.om);
            store_goal_planets<N>(b, i, e);
            b.ctr[i] = ct;
        }
        {   // the replay records nobody has claimed yet are integrated here, while the finisher goes through its last steps
            uint32_t lo = 0u;
            if (lane == 0) lo = atomicMax(&rp_claim[pair], head);
            lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the records were written by other lanes of this wave
#pragma unroll 1
            while ((int32_t)(head - lo) > 0) {
                const uint32_t n = min(head - lo, 64u);
                goal_replay_integrate<N, ACCEL>(c, rb, lo, n, lane);
                lo += n;
            }
            lds_flag_store(&rp_done[pair], 1u);  // release: the results are in the records
        }
        SG_REAL(3);
        return;
    }

    // ---- finisher
    SG_ACC_DECL;
    const bool auto_reset = c.auto_reset != 0;
    const int wave_env0 = i - lane;
    unsigned long long *const cnt = b.cnt;  // NULL unless the handle counts events (sg_set_counters)
    // what every step reads of the parameter block, pinned in vector registers (as for the pilot: left to the compiler these
    // are scalar loads at the top of every step, each with its latency in front of this wave's instructions)
    GoalStepConsts fc = goal_step_consts(c);
#if SG_ROLLOUT_PROFILED
    {  // the reward's coefficients: this lane's env's profile
        const GoalRewardView v = rs.goal(c, ii);
        fc.danger_r2 = v.danger_r2; fc.survival = v.survival; fc.goal_scale = v.goal_scale; fc.safety_scale = v.safety_scale;
        fc.sparse = v.sparse;
    }
#endif
    asm volatile("" : "+v"(fc.goal_r2), "+v"(fc.danger_r2), "+v"(fc.survival), "+v"(fc.goal_scale), "+v"(fc.safety_scale),
                      "+v"(fc.sparse), "+v"(fc.planet_r), "+v"(fc.two_over_world));
    int max_steps = c.max_episode_steps;
    asm volatile("" : "+v"(max_steps));
    uint32_t hi = ct.y;  // == spare_hi[tid]
    uint4 aux = b.aux[ii];      // the tiling's cold state (goal_draws, tiles | flags, free multiset) stays in registers:
    float4 cs = b.cshift[ii];   // read by goal resamples, replaced on a restart, written back at the end
    // The LDS queue starts from what earlier launches left in the HBM copy (EpisodeQueue): kSpare records per lane at most,
    // all loads first, then the LDS writes -- done while the pilot integrates its first step.
    if (auto_reset) {
        const uint32_t q_hi = b.ephi[ii];  // highest episode index in the HBM copy (<= ct.y, or stale: nothing usable)
        const int n_have = live ? min(max((int32_t)(q_hi - ct.y), 0), kSpare) : 0;
        float4 rec[kSpare][kQCols];
#pragma unroll
        for (int s = 0; s < kSpare; s++)
            if (s < n_have) {
                const float4 *p = Queue::slot(b.epq, B, i, ct.y + 1u + (uint32_t)s);
#pragma unroll
                for (int col = 0; col < kQCols; col++)
                    if (col != 3 || N > 2) rec[s][col] = p[(uint32_t)col * (uint32_t)B];
            }
#pragma unroll
        for (int s = 0; s < kSpare; s++)
            if (s < n_have) Spare::put_record(spare, (int)((ct.y + 1u + (uint32_t)s) % (uint32_t)kSpare), tid, rec[s]);
        hi = ct.y + (uint32_t)n_have;
        lds_flag_store(&spare_hi[tid], hi);
    }
    auto refill = [&]() {  // one more episode for every lane whose queue is not full
        SG_ACC_ADD(10, 1);
        if (live && hi - ct.y < (uint32_t)kSpare) {
            Tiling T;
            T.episode = hi + 1u;
            ShipInit s;
            float px[N], py[N], gx, gy;
            goal_reset<N>(c, c.env_index_base + (uint32_t)i, T, s, px, py, gx, gy);
            Spare::put(spare, (int)(T.episode % (uint32_t)kSpare), tid, s, px, py, gx, gy, T);
            Queue::put(b.epq, B, i, s, px, py, gx, gy, T);  // and into the copy that outlives the launch
            hi = T.episode;
            lds_flag_store(&spare_hi[tid], hi);  // release: after the episode itself (the LDS one is what this launch reads)
        }
    };
    // Keep one episode per lane beyond the one a restarting lane takes now: the pilot runs ahead of the finisher (by less
    // than kRing steps) and needs the NEXT episode of a lane only when the one started here has ended, i.e. it finds the
    // queue empty only if an env restarts twice within that lead (then it generates the episode itself).
    constexpr uint32_t kKeep = 1u;
    if (auto_reset && __any(live && hi - ct.y < kKeep)) refill();  // (a fresh handle: while the pilot integrates its first step)
    uint32_t tail = 0u, complete = 0u;  // replay records read so far; records of the steps gone through here (complete with their goals)
    bool mine = true;  // the replay passes are this wave's, until the pilot claims what is left at the end
    // this lane's place in row t of the outputs, as four running pointers in vector registers (advanced by one row per step):
    // formed from t every step they cost three 64-bit multiplies and the re-loading of four spilled base pointers
    // (explicitly global pointers: behind the asm barrier the compiler no longer infers the address space and would fall
    //  back to flat stores)
    typedef __attribute__((address_space(1))) float gfloat;
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    gfloat *obs_p = (gfloat *)obs + (int64_t)ii * D, *rew_p = (gfloat *)reward + ii;
    gbyte *done_p = (gbyte *)done + ii, *trunc_p = (gbyte *)truncated + ii;
    asm volatile("" : "+v"(obs_p), "+v"(rew_p), "+v"(done_p), "+v"(trunc_p));
    for (int t = 0; t < n_steps; t++) {
        SG_ACC(0);
        if (!wait_flag(&handed[pair], (uint32_t)(t + 1))) { *status = 2; break; }
        SG_ACC(1);
        double dXd, dYd;
        float th, vx, vy, om;
        int dn;
        bool replayed;
        {
            const int slot = t % kRing;
            const float *q = ring + (slot * kHand) * kBlock + tid;
            const uint64_t ux = (uint64_t)__float_as_uint(q[0 * kBlock]) | ((uint64_t)__float_as_uint(q[1 * kBlock]) << 32);
            const uint64_t uy = (uint64_t)__float_as_uint(q[2 * kBlock]) | ((uint64_t)__float_as_uint(q[3 * kBlock]) << 32);
            dXd = __longlong_as_double((long long)ux); dYd = __longlong_as_double((long long)uy);
            th = q[4 * kBlock]; vx = q[5 * kBlock]; vy = q[6 * kBlock]; om = q[7 * kBlock];
            const uint32_t w8 = __float_as_uint(q[8 * kBlock]);
            dn = (int)(w8 & 1u);
            replayed = (w8 & 2u) != 0u;
            if (replayed) Replay::put_goal(rb, w8 >> 8, e.gx, e.gy);  // the goal of this env's replay record (see GoalReplay)
            complete += (uint32_t)__popcll(__ballot(replayed));  // (records are appended step by step)
        }
        lds_flag_store(&taken[pair], (uint32_t)(t + 1));  // the record is in registers: its slot may be reused
        SG_ACC(3);
        // goal_env_finish, TimeLimit and the stores, with ONE observation per step: an env that restarts takes its next episode out
        // of the queue before the observation is formed (the first observation of the new episode is what the step returns)
        float o[D], r;
        int hit;
        r = goal_reward<N>(fc, e.x, e.y, dXd, dYd, e.px, e.py, e.gx, e.gy, hit);
        count_hits(cnt, live && hit && !replayed);  // (a replayed env-step's goal hit is known to its replay)
        e.x = (float)((double)e.x + dXd); e.y = (float)((double)e.y + dYd); e.vx = vx; e.vy = vy; e.om = om; e.th = th;
        const uint32_t el = ct.x + 1u;
        const int trunc = !dn && (int)el >= max_steps;  // gym.wrappers.TimeLimit
        const int fin = dn | trunc;
        const bool restart = live && fin && auto_reset;
        if (live) ct.x = el;
        SG_ACC(4);
        if constexpr (TOBS) {  // the last observation of an episode that ends here, before the env takes its next episode
            // (a replayed env-step's comes out of its replay)
            if (__any(restart && !replayed)) {
                goal_observe<N>(fc, e, o);
                term_append<D>(tl, restart && !replayed, t, i, o);
            }
        }
        // (after the launch's last step nobody runs ahead any more: the spare episode is left to the next launch, whose
        //  finisher generates it while its pilot integrates the first step)
        const uint32_t keep = t + 1 < n_steps ? kKeep : 0u;
        if (auto_reset && __any(live && hi - ct.y < (restart ? keep + 1u : keep))) refill();
        SG_ACC(6);
        if (restart) {  // take the next episode out of the queue
            ct = make_uint2(0u, ct.y + 1u);
            Spare::get(spare, (int)(ct.y % (uint32_t)kSpare), tid, e, aux, cs);
        }
        SG_ACC(12);
        goal_observe<N>(fc, e, o);
        SG_ACC(13);
        if (live) {
#pragma unroll
            for (int k = 0; k < D; k++) obs_p[k] = o[k];
            if (!replayed) *rew_p = r;  // (a replayed env-step's reward comes out of its replay)
            *done_p = (uint8_t)fin;
            *trunc_p = (uint8_t)trunc;
        }
        obs_p += B * D; rew_p += B; done_p += B; trunc_p += B;
        asm volatile("" : "+v"(obs_p), "+v"(rew_p), "+v"(done_p), "+v"(trunc_p));
        SG_ACC(5);
        SG_ACC(7);
        SG_ACC_ADD(11, __any(live && hit && !restart) ? 1 : 0);
        if (live && hit && !restart) {  // GoalEnv._resample_goal on a hit (goal.py:154-157): shows in the next observation
            Tiling T;
            T.episode = ct.y; T.goal_draws = aux.x;
            T.ship_tile = aux.y & 0xffu; T.goal_tile = (aux.y >> 8) & 0xffu; T.case_b = (aux.y >> 16) & 1u; T.flip = (aux.y >> 17) & 1u;
            T.free_counts = (uint64_t)aux.z | ((uint64_t)aux.w << 32);
            T.cs0 = cs.x; T.cs1 = cs.y; T.cs2 = cs.z; T.cs3 = cs.w;
            goal_resample(c, c.env_index_base + (uint32_t)i, T, e.gx, e.gy);
            aux = pack_aux(T);
        }
        SG_ACC(2);
        // terminal env-steps waiting to be replayed: those of steps <= t, complete with their goals
        if (complete - tail >= (uint32_t)kReplayAt && mine) {
            const uint32_t n = min(complete - tail, 64u);
            uint32_t got = 0u;  // (claimed, unless the pilot -- past its last step -- has taken the rest)
            if (lane == 0) got = atomicCAS(&rp_claim[pair], tail, tail + n);
            mine = (uint32_t)__builtin_amdgcn_readfirstlane((int)got) == tail;
            if (mine) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup", "local");
                goal_replay_pass<N, ACCEL, TOBS>(c, rb, tail, n, lane, wave_env0, B, reward, tl, &rp_tail[pair], cnt SG_ROLLOUT_RS);
                tail += n;
            }
        }
        SG_ACC(9);
    }
    SG_ACC_WRITE(blockIdx.x * 8 + 4 + pair);
    SG_REAL(2);
    if (live) {  // the finisher's share of the state: goal, the tiling's cold state, the fill level of the queue's HBM copy
        reinterpret_cast<float2 *>(b.q1 + i)[1] = make_float2(e.gx, e.gy);
        b.aux[i] = aux;
        b.cshift[i] = cs;
        if (auto_reset) b.ephi[i] = hi;
    }
    if (tail != complete) {  // the terminal env-steps still waiting: integrated by the pilot, which claimed them after its last step
        if (!wait_flag(&rp_done[pair], 1u)) *status = 3;
#pragma unroll 1
        while (tail != complete) {
            const uint32_t n = min(complete - tail, 64u);
            goal_replay_reward<N, TOBS>(c, rb, tail, n, lane, wave_env0, B, reward, tl, cnt SG_ROLLOUT_RS);
            tail += n;
        }
    }
    SG_REAL(3);
