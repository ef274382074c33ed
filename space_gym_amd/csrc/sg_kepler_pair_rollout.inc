// The body of kepler_pair_rollout_kernel and kepler_pair_rollout_profiled_kernel (sg_engine.hip), included by both, as
// sg_goal_pair_rollout.inc (see there).

    using Integ = Integrator<2, 1, false, ACCEL>;
    __shared__ float spare[kSpare * kKeplerSpareFields * kBlock];
    __shared__ float ring[kRing * kHand * kBlock];
    __shared__ float rbuf[(kBlock / 64) * kKeplerReplayWords * kReplayCap];  // terminal env-steps to replay, as in goal_pair_rollout_kernel
    __shared__ uint32_t spare_hi[kBlock];
    __shared__ uint32_t handed[kBlock / 64], taken[kBlock / 64];
    __shared__ uint32_t rp_tail[kBlock / 64], rp_claim[kBlock / 64];  // replay records read by the finisher / claimed for replaying
    const SgDev &c = *cfg;
    const bool discrete = c.discrete_actions != 0;  // read once: inside the step loop it would be re-loaded every step
    const int tid = threadIdx.x & (kBlock - 1), pair = tid >> 6, lane = tid & 63;
    const bool pilot = threadIdx.x < kBlock;
    const int i = blockIdx.x * kBlock + tid;
    const bool live = i < c.num_envs;
    const int ii = live ? i : 0;
    const int64_t B = c.num_envs;
    KeplerEnv e;
    load_kepler_env(b, ii, e);
    uint2 ct = b.ctr[ii];
    float *const rb = rbuf + pair * kKeplerReplayWords * kReplayCap;
    if (!pilot) spare_hi[tid] = ct.y;
    if (threadIdx.x < kBlock / 64) { handed[threadIdx.x] = 0u; taken[threadIdx.x] = 0u; rp_tail[threadIdx.x] = 0u; rp_claim[threadIdx.x] = 0u; }
    __syncthreads();  // the only workgroup barrier

    if (pilot) {
        __builtin_amdgcn_s_setprio(3);
        const bool hand_over = c.auto_reset && live;  // (read once) the env restarts after a terminal step: its terminal state is the finisher's
        const bool auto_reset = c.auto_reset != 0;
        const bool rnd_orbit = c.randomize_orbit != 0;
        // the parameters of a step, pinned in vector registers (see goal_pair_rollout_kernel)
        StepConsts kc = step_consts(c);
        float border_r = c.border_r;
        int max_steps = c.max_episode_steps;
        asm volatile("" : "+v"(kc.max_engine_force), "+v"(kc.h), "+v"(kc.half_world), "+v"(kc.gm), "+v"(kc.omega_limit), "+v"(kc.planet_r),
                          "+v"(kc.max_thruster_force), "+v"(kc.inv_moi), "+v"(kc.planet_r_d), "+v"(border_r), "+v"(max_steps));
        double2 orb = rnd_orbit ? b.orbd[ii] : make_double2(1.0, 0.0);  // (the replay record carries the env's orbit)
        float2 a_next = load_action_raw(discrete, actions, ii);
        uint32_t taken_seen = 0u;
        uint32_t head = 0u, tail_seen = 0u;  // replay records written; read by the finisher (as last seen)
        for (int t = 0; t < n_steps; t++) {
            const float2 a_raw = decode_action(discrete, a_next);
            float a0 = a_raw.x, a1 = a_raw.y;
            if (t + 1 < n_steps) a_next = load_action_raw(discrete, actions, (int64_t)(t + 1) * B + ii);
            if (t - (int)taken_seen >= kRing && !wait_flag<SG_PILOT_SLEEP>(&taken[pair], (uint32_t)(t - kRing + 1), &taken_seen)) { *status = 1; break; }
            if (head + 64u - tail_seen > (uint32_t)kReplayCap) tail_seen = lds_flag_load_uniform(&rp_tail[pair]);
            const bool defer = hand_over && head + 64u - tail_seen <= (uint32_t)kReplayCap;
            const int slot = t % kRing;
            StepResult r;
            int rk;
            {  // the integration of kepler_env_step; terminal states are left to the finisher
                float engine, F, om, om0, alpha;
                translate_action(a0, a1, kc.max_engine_force, engine, F, om);
                if (ACCEL && kc.steering_acceleration) { om0 = e.om; alpha = (a1 * kc.max_thruster_force) * kc.inv_moi; }  // steering<ACCEL>
                else { om0 = om; alpha = 0.0f; }
                const float cax[2] = {0.0f, 0.0f}, cay[2] = {0.0f, 0.0f}, cR[2] = {kc.planet_r, border_r};
                const double cRd[2] = {kc.planet_r_d, (double)border_r};
                Integ I;
                I.begin(kc.h, kc.half_world, kc.gm, F, om0, alpha, kc.omega_limit, e.x, e.y, e.th, e.vx, e.vy, cax, cay, cR, cRd);
                rk = I.run(r, [&]() __attribute__((always_inline)) -> bool { return defer; });
            }
            const bool replayed = rk == kRkEventDeferred;
            {
                const unsigned long long dm = __ballot(replayed);
                if (dm) {
                    if (replayed) {
                        float *q = rb + (head + (uint32_t)__popcll(dm & ((1ull << lane) - 1ull))) % (uint32_t)kReplayCap;
                        const uint64_t uc = __double_as_longlong(orb.x), us = __double_as_longlong(orb.y);
                        q[0] = __uint_as_float(((uint32_t)t << 6) | (uint32_t)lane);
                        q[1 * kReplayCap] = e.x; q[2 * kReplayCap] = e.y; q[3 * kReplayCap] = e.th; q[4 * kReplayCap] = e.vx;
                        q[5 * kReplayCap] = e.vy; q[6 * kReplayCap] = e.om; q[7 * kReplayCap] = a_raw.x; q[8 * kReplayCap] = a_raw.y;
                        q[9 * kReplayCap] = e.phi; q[10 * kReplayCap] = e.ecc;
                        q[11 * kReplayCap] = __uint_as_float((uint32_t)uc); q[12 * kReplayCap] = __uint_as_float((uint32_t)(uc >> 32));
                        q[13 * kReplayCap] = __uint_as_float((uint32_t)us); q[14 * kReplayCap] = __uint_as_float((uint32_t)(us >> 32));
                    }
                    head += (uint32_t)__popcll(dm);
                }
            }
            e.x = (float)((double)e.x + r.dXd); e.y = (float)((double)e.y + r.dYd); e.vx = r.vx; e.vy = r.vy; e.om = r.om;
            e.th = wrap_two_pi(e.th + r.dth);
            {
                float *q = ring + (slot * kHand) * kBlock + tid;
                const uint64_t ux = __double_as_longlong(r.dXd), uy = __double_as_longlong(r.dYd);
                q[0 * kBlock] = __uint_as_float((uint32_t)ux); q[1 * kBlock] = __uint_as_float((uint32_t)(ux >> 32));
                q[2 * kBlock] = __uint_as_float((uint32_t)uy); q[3 * kBlock] = __uint_as_float((uint32_t)(uy >> 32));
                q[4 * kBlock] = e.th; q[5 * kBlock] = e.vx; q[6 * kBlock] = e.vy; q[7 * kBlock] = e.om;
                q[8 * kBlock] = __uint_as_float((uint32_t)r.done | (replayed ? 2u : 0u));
            }
            lds_flag_store(&handed[pair], (uint32_t)(t + 1));  // release: the step record and the replay records are visible before the counter
            const uint32_t el = ct.x + 1u;
            const int trunc = !r.done && (int)el >= max_steps;
            const bool restart = live && (r.done | trunc) && auto_reset;
            if (live) ct.x = el;
            if (restart) {
                const uint32_t k = ct.y + 1u;
                if ((int32_t)(lds_flag_load(&spare_hi[tid]) - k) >= 0) {
                    const float *q = spare + ((int)(k % (uint32_t)kSpare) * kKeplerSpareFields) * kBlock + tid;
                    e.x = q[0 * kBlock]; e.y = q[1 * kBlock]; e.th = q[2 * kBlock]; e.vx = q[3 * kBlock];
                    e.vy = q[4 * kBlock]; e.om = q[5 * kBlock];
                    if (rnd_orbit) {
                        e.phi = q[6 * kBlock]; e.ecc = q[7 * kBlock];
                        const uint64_t uc = (uint64_t)__float_as_uint(q[8 * kBlock]) | ((uint64_t)__float_as_uint(q[9 * kBlock]) << 32);
                        const uint64_t us = (uint64_t)__float_as_uint(q[10 * kBlock]) | ((uint64_t)__float_as_uint(q[11 * kBlock]) << 32);
                        orb = make_double2(__longlong_as_double((long long)uc), __longlong_as_double((long long)us));
                    }
                } else {
                    ShipInit s;
                    kepler_reset(c, c.env_index_base + (uint32_t)i, k, s, e.phi, e.ecc);
                    e.x = s.x; e.y = s.y; e.th = s.th; e.vx = s.vx; e.vy = s.vy; e.om = s.om;
                    if (rnd_orbit) orb = make_double2(cos((double)e.phi), sin((double)e.phi));
                }
                ct = make_uint2(0u, k);
            }
        }
        if (live) {  // final hot state; the orbit half of q1 belongs to the finisher
            b.q0[i] = make_float4(e.x, e.y, e.th, e.vx);
            reinterpret_cast<float2 *>(b.q1 + i)[0] = make_float2(e.vy, e.om);
            b.ctr[i] = ct;
        }
        {   // the replay records nobody has claimed yet are replayed here (a Kepler record holds all a replay needs), while the
            // finisher goes through its last steps: see goal_pair_rollout_kernel
            uint32_t lo = 0u;
            if (lane == 0) lo = atomicMax(&rp_claim[pair], head);
            lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the records were written by other lanes of this wave
#pragma unroll 1
            while ((int32_t)(head - lo) > 0) {
                const uint32_t n = min(head - lo, 64u);
                kepler_replay_pass<ACCEL>(c, rb, lo, n, lane, i - lane, B, reward, tl, nullptr SG_ROLLOUT_RS);
                lo += n;
            }
        }
        return;
    }

    // ---- finisher
    const int wave_env0 = i - lane;
    // what every step reads of the parameter block, pinned in vector registers (see goal_pair_rollout_kernel): the constants of
    // the reward and the observation, and the fixed reference orbit with its derived quantities (three fp64 divisions)
    KeplerStepConsts fc = kepler_step_consts(c);
#if SG_ROLLOUT_PROFILED
    {  // the reward's coefficients: this lane's env's profile
        const KeplerRewardView v = rs.kepler(c, ii);
        fc.k_C = v.k_C; fc.k_Cr = v.k_Cr; fc.k_Ca = v.k_Ca;
    }
#endif
    asm volatile("" : "+v"(fc.k_gm), "+v"(fc.k_C), "+v"(fc.k_Cr), "+v"(fc.k_phi), "+v"(fc.k_ecc), "+v"(fc.k_a), "+v"(fc.k_Ca));
    Orbit ob_fixed = fixed_orbit(c);
    asm volatile("" : "+v"(ob_fixed.a), "+v"(ob_fixed.b), "+v"(ob_fixed.c), "+v"(ob_fixed.ecc), "+v"(ob_fixed.cosphi), "+v"(ob_fixed.sinphi),
                      "+v"(ob_fixed.a_over_b), "+v"(ob_fixed.b_over_a), "+v"(ob_fixed.inv_a));
    float max_engine_force = c.max_engine_force;
    int max_steps = c.max_episode_steps;
    asm volatile("" : "+v"(max_engine_force), "+v"(max_steps));
    const bool rnd_orbit = c.randomize_orbit != 0, auto_reset = c.auto_reset != 0;
    uint32_t hi = ct.y;
    double2 orb = c.randomize_orbit ? b.orbd[ii] : make_double2(1.0, 0.0);  // cos / sin of the env's reference-orbit angle
    auto refill = [&]() {
        if (hi - ct.y < (uint32_t)kSpare) {
            ShipInit s;
            float phi = e.phi, ecc = e.ecc;  // fixed-orbit ids keep their (unused) orbit slots
            kepler_reset(c, c.env_index_base + (uint32_t)ii, hi + 1u, s, phi, ecc);
            float *q = spare + ((int)((hi + 1u) % (uint32_t)kSpare) * kKeplerSpareFields) * kBlock + tid;
            q[0 * kBlock] = s.x; q[1 * kBlock] = s.y; q[2 * kBlock] = s.th; q[3 * kBlock] = s.vx; q[4 * kBlock] = s.vy;
            q[5 * kBlock] = s.om; q[6 * kBlock] = phi; q[7 * kBlock] = ecc;
            if (c.randomize_orbit) {
                const uint64_t uc = __double_as_longlong(cos((double)phi)), us = __double_as_longlong(sin((double)phi));
                q[8 * kBlock] = __uint_as_float((uint32_t)uc); q[9 * kBlock] = __uint_as_float((uint32_t)(uc >> 32));
                q[10 * kBlock] = __uint_as_float((uint32_t)us); q[11 * kBlock] = __uint_as_float((uint32_t)(us >> 32));
            }
            hi += 1u;
            lds_flag_store(&spare_hi[tid], hi);
        }
    };
    constexpr uint32_t kKeep = 1u;
    if (c.auto_reset) refill();
    uint32_t tail = 0u, complete = 0u;  // replay records read so far; records of the steps gone through here
    bool mine = true;  // the replay passes are this wave's, until the pilot claims what is left at the end
    for (int t = 0; t < n_steps; t++) {
        float a0, a1;
        load_action(discrete, actions, (int64_t)t * B + ii, a0, a1);  // the reward's action term needs it (kepler.py:150-152)
        if (!wait_flag(&handed[pair], (uint32_t)(t + 1))) { *status = 2; break; }
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
            complete += (uint32_t)__popcll(__ballot(replayed));  // (records are appended step by step)
        }
        lds_flag_store(&taken[pair], (uint32_t)(t + 1));
        // the rest of kepler_env_step + kepler_step_body, with one observation per step (a restarting env takes its next
        // episode first) and the per-env orbit's cos / sin phi in registers (KeplerRandomOrbits)
        float engine, F, om_cmd;
        translate_action(a0, a1, max_engine_force, engine, F, om_cmd);
        Orbit ob = ob_fixed;
        if (rnd_orbit) ob = make_orbit(fc.k_a, (double)e.ecc, orb.x, orb.y);
        const float r = kepler_reward(fc, ob, e.x, e.y, dXd, dYd, vx, vy, engine, a1);
        e.x = (float)((double)e.x + dXd); e.y = (float)((double)e.y + dYd); e.vx = vx; e.vy = vy; e.om = om; e.th = th;
        const uint32_t el = ct.x + 1u;
        const int trunc = !dn && (int)el >= max_steps;
        const int fin = dn | trunc;
        const bool restart = live && fin && auto_reset;
        ct.x = el;
        if (tl.count && __any(restart && !replayed)) {  // the last observation of an episode that ends here (a replayed step's comes out of its replay)
            float ot[10];
            kepler_observe(fc, e, ot);
            term_append<10>(tl, restart && !replayed, t, i, ot);
        }
        if (auto_reset && __any(live && hi - ct.y < (restart ? kKeep + 1u : kKeep))) refill();
        if (restart) {
            ct = make_uint2(0u, ct.y + 1u);
            const float *q = spare + ((int)(ct.y % (uint32_t)kSpare) * kKeplerSpareFields) * kBlock + tid;
            e.x = q[0 * kBlock]; e.y = q[1 * kBlock]; e.th = q[2 * kBlock]; e.vx = q[3 * kBlock]; e.vy = q[4 * kBlock];
            e.om = q[5 * kBlock]; e.phi = q[6 * kBlock]; e.ecc = q[7 * kBlock];
            if (rnd_orbit) {
                const uint64_t uc = (uint64_t)__float_as_uint(q[8 * kBlock]) | ((uint64_t)__float_as_uint(q[9 * kBlock]) << 32);
                const uint64_t us = (uint64_t)__float_as_uint(q[10 * kBlock]) | ((uint64_t)__float_as_uint(q[11 * kBlock]) << 32);
                orb = make_double2(__longlong_as_double((long long)uc), __longlong_as_double((long long)us));
            }
        }
        float o[10];
        kepler_observe(fc, e, o);
        if (live) {
            const int64_t row = (int64_t)t * B + i;
            store_row(obs, row, o);
            if (!replayed) reward[row] = r;  // (a replayed env-step's reward comes out of its replay)
            done[row] = (uint8_t)fin;
            truncated[row] = (uint8_t)trunc;
        }
        if (complete - tail >= (uint32_t)kReplayAt && mine) {  // terminal env-steps waiting to be replayed
            const uint32_t n = min(complete - tail, 64u);
            uint32_t got = 0u;  // (claimed, unless the pilot -- past its last step -- has taken the rest)
            if (lane == 0) got = atomicCAS(&rp_claim[pair], tail, tail + n);
            mine = (uint32_t)__builtin_amdgcn_readfirstlane((int)got) == tail;
            if (mine) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                kepler_replay_pass<ACCEL>(c, rb, tail, n, lane, wave_env0, B, reward, tl, &rp_tail[pair] SG_ROLLOUT_RS);
                tail += n;
            }
        }
    }
    if (live && c.randomize_orbit) b.orbd[i] = orb;
    if (live) reinterpret_cast<float2 *>(b.q1 + i)[1] = make_float2(e.phi, e.ecc);
    // (the terminal env-steps still waiting are the pilot's: it claimed them after its last step)
