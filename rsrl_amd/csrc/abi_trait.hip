// abi_trait.hip -- the trait-granular entry points: Domain::transition, Function / Enumerable, Policy, Handler::handle, and the deferred
// trait loop (kernels_trait.hpp) that runs a batch-step's four calls as one launch.
#include "ctx.hpp"

RSRL_DEFINE_FX_READER(fx_saturations_trait)

// ---- the trait-granular loop (kernels_trait.hpp) --------------------------------------------------------------------------------------
// the hand-over cache is keyed by the state an entry belongs to; whenever the weights changed behind it (train, set / load weights) the keys are
// emptied (NaN: never equal to a state) before the next kernel that looks at them
int trait_cache_ready(rsrl_hip_ctx* c) {
    if (c->tq_valid) return RSRL_HIP_OK;
    HIP_TRY(hipMemsetAsync(c->tq_key, 0xFF, sizeof(float) * (size_t)c->D * (size_t)c->cfg.n_envs, c->stream));
    c->tq_valid = true;
    return RSRL_HIP_OK;
}
int launch_domain_step(rsrl_hip_ctx* c, const Common& k, const int32_t* d_act, float* from, float* next, float* rew, uint8_t* term) {
    const dim3 g(grid_for(c->cfg.n_envs)), b(kBlock);
    if (c->hiv_y) { launch_hiv_domain_step(c->stream, k, c->hiv_y, d_act, from, next, rew, term); KCHECK(); return RSRL_HIP_OK; }
    if (c->family == AgentFamily::CliffTable) { launch_table_domain_step(c->stream, k, d_act, from, next, rew, term); KCHECK(); return RSRL_HIP_OK; }
    if (c->cfg.domain == RSRL_CONTINUOUS_MOUNTAIN_CAR) return fail(RSRL_HIP_ESTATE, "ContinuousMountainCar steps on f32 actions (rsrl_hip_domain_step_f32)");
    if (!for_domain3(c->cfg.domain, [&](auto d) { hipLaunchKernelGGL(k_domain_step<d.value>, g, b, 0, c->stream, k, d_act, from, next, rew, term); })) return NO_MODEL(c);
    KCHECK();
    return RSRL_HIP_OK;
}
int launch_domain_reset(rsrl_hip_ctx* c, const Common& k, const uint8_t* d_mask) {
    const dim3 g(grid_for(c->cfg.n_envs)), b(kBlock);
    if (c->hiv_y) { launch_hiv_domain_reset(c->stream, k, c->hiv_y, d_mask); KCHECK(); return RSRL_HIP_OK; }
    if (c->family == AgentFamily::CliffTable) { launch_table_domain_reset(c->stream, k, d_mask); KCHECK(); return RSRL_HIP_OK; }
    // (ContinuousMountainCar: MountainCar's state space and start state)
    const int domain = c->cfg.domain == RSRL_CONTINUOUS_MOUNTAIN_CAR ? RSRL_MOUNTAIN_CAR : c->cfg.domain;
    if (!for_domain3(domain, [&](auto d) { hipLaunchKernelGGL(k_domain_reset<d.value>, g, b, 0, c->stream, k, d_mask); })) return NO_MODEL(c);
    KCHECK();
    return RSRL_HIP_OK;
}
// Handler::handle on the fast path: one pass over the learners' weight images, the hand-over left for the sample that follows
int launch_trait_handle(rsrl_hip_ctx* c, const Common& k, const float* from, const int32_t* act, const float* rew, const float* to,
                               const uint8_t* term, int64_t M, uint64_t t, float* td) {
    TRY(trait_cache_ready(c));
    TraitIo io{};
    io.from = from; io.act = act; io.rew = rew; io.to = to; io.termf = term; io.td_out = td; io.qkey = c->tq_key; io.qval = c->tq_q; io.Mn = M;
    TRY(timing_begin(c));
    if (!launch_trait_lm(c->cfg.domain, c->cfg.order, c->cfg.algo, -1, c->stream, k, io, t)) return NO_MODEL(c);
    KCHECK();
    c->kernel_name = "k_trait_lm<handle>";
    return timing_end(c);
}
// the deferred calls, one kernel per call, in the order they were made
int trait_flush(rsrl_hip_ctx* c) {
    if (c->tp.stage == 0) return RSRL_HIP_OK;
    const rsrl_hip_ctx::TraitPend p = c->tp;
    c->tp.stage = 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const Common k = make_common(c);
    TRY(launch_domain_step(c, k, p.act, p.from, p.to, p.rew, p.term));
    if (p.stage >= 2) TRY(launch_trait_handle(c, k, p.from, p.act, p.rew, p.to, p.term, c->cfg.n_envs, p.t_handle, p.td));
    if (p.stage >= 3) TRY(launch_domain_reset(c, k, p.term));
    return RSRL_HIP_OK;
}

int flush_pending(rsrl_hip_ctx* c) {
    if (!c) return RSRL_HIP_OK;
    if (c->tp.stage) TRY(trait_flush(c));
    if (c->pending == 0) return RSRL_HIP_OK;
    const int64_t n = c->pending;
    c->pending = 0;
    return train_now(c, n, nullptr);
}
// Domain::transition's five arrays, as the kernels take them.  Act: int32_t indices or f32 actions (rsrl_hip_domain_step_f32)
template <class Act>
struct StepArrays { const Act* act; float* from; float* next; float* rew; uint8_t* term; };
template <class Act>
static int stage_step(CallFrame& f, const Act* actions, float* from, float* next, float* rew, uint8_t* term, StepArrays<Act>* s) {
    const size_t N = (size_t)f.c->cfg.n_envs, DN = (size_t)f.c->D * N;
    TRY(f.in(actions, N, &s->act));
    TRY(f.out(from, DN, &s->from)); TRY(f.out(next, DN, &s->next));
    TRY(f.out(rew, N, &s->rew)); TRY(f.out(term, N, &s->term));
    return RSRL_HIP_OK;
}
// Handler::handle's M transitions (launch.hpp), int32 or f32 actions alike
template <class Act>
static int stage_transitions(CallFrame& f, const float* from, const Act* act, const float* rew, const float* to, const uint8_t* term, int64_t M, float* td_out,
                             TransitionsOf<Act>* io) {
    const size_t DM = (size_t)f.c->D * M;
    TRY(f.in(from, DM, &io->from)); TRY(f.in(act, (size_t)M, &io->act)); TRY(f.in(rew, (size_t)M, &io->rew));
    TRY(f.in(to, DM, &io->to)); TRY(f.in(term, (size_t)M, &io->term));
    TRY(f.out(td_out, (size_t)M, &io->td_out));
    io->M = M;
    return RSRL_HIP_OK;
}

RSRL_API_BEGIN

int rsrl_hip_domain_step(rsrl_hip_ctx* c, const int32_t* actions, float* from_states, float* next_states,
                         float* rewards, uint8_t* terminal) {
    CHECK_CTX(c); FLUSH(c);
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_domain_step");
    c->q_valid = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    // the trait-granular loop on a ctx-owned stream: a transition handed over in device arrays is ACCEPTED here and launched with the calls that
    // follow it (rsrl_hip_handle on exactly these arrays, rsrl_hip_domain_reset on the terminal flags, rsrl_hip_policy_sample of the ctx's envs) as
    // one kernel -- or, by whatever other call comes next, as the kernel it would have been now.  Same results, same order (kernels_trait.hpp).
    CallFrame f(c);
    if (trait_fast(c) && c->own_stream && !c->sw.no_trait_defer && f.device(actions) && f.device(from_states) && f.device(next_states) && f.device(rewards) &&
        f.device(terminal)) {
        c->tp = rsrl_hip_ctx::TraitPend{};
        c->tp.stage = 1; c->tp.act = actions; c->tp.from = from_states; c->tp.to = next_states; c->tp.rew = rewards; c->tp.term = terminal;
        return RSRL_HIP_OK;
    }
    TRY(check_host_actions(f, actions, (size_t)c->cfg.n_envs, c->A));
    StepArrays<int32_t> s;
    TRY(stage_step(f, actions, from_states, next_states, rewards, terminal, &s));
    const Common k = make_common(c);
    TRY(launch_domain_step(c, k, s.act, s.from, s.next, s.rew, s.term));
    return f.finish();
}

int rsrl_hip_domain_reset(rsrl_hip_ctx* c, const uint8_t* mask) {
    CHECK_CTX(c);
    if (c->tp.stage == 2 && mask && mask == c->tp.term) { c->tp.stage = 3; return RSRL_HIP_OK; }      // the new episodes of the transition just handled
    FLUSH(c);
    c->q_valid = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs;
    CallFrame f(c);
    const uint8_t* d_mask;
    TRY(f.in(mask, (size_t)N, &d_mask));
    const Common k = make_common(c);
    TRY(launch_domain_reset(c, k, d_mask));
    // REINFORCE: the restarted learners begin new episodes, sampled from theta as it stands (theta_b <- theta, g <- 0)
    if (c->family == AgentFamily::ReinforceReg) { launch_reinforce_restart(c->stream, make_reinforce(c), N, (int64_t)c->F * c->A, d_mask); KCHECK(); }
    return f.finish();
}

static int qop(rsrl_hip_ctx* c, int op, const float* states, int64_t M_, float* fout, size_t fcount, int32_t* iout,
               size_t icount = 0, const float* fin = nullptr, size_t fin_count = 0, const int32_t* iin = nullptr, uint64_t step_t = 0) {
    CHECK_CTX(c); FLUSH(c);
    if (!states || M_ < 1 || M_ > c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "bad batch (M=%lld, n_envs=%lld)", (long long)M_, (long long)c->cfg.n_envs);
    // a continuous ctx: the value side is V (iLSTD's theta), the projection is MountainCar's; its policy side has entry points of its own
    if (is_continuous(c) && op != QOP_EVALUATE && op != QOP_FEATURES)
        return fail(RSRL_HIP_ESTATE, "this ctx's domain (ContinuousMountainCar) has one f32 action, not an enumerable set: no action values to search, weigh or "
                                     "index, no action probabilities (the policy side: rsrl_hip_policy_sample_f32 / _mode_f32 / _params / _pdf; V(s): rsrl_hip_q_evaluate)");
    if (is_nac(c->cfg.algo) && op == QOP_EVALUATE)
        return fail(RSRL_HIP_ESTATE, "NAC's critic is Q(s, a) over the stable compatible basis: it needs an action (rsrl_hip_q_evaluate_f32)");
    if (is_v_only(c->cfg.algo) && op != QOP_EVALUATE && op != QOP_FEATURES)
        return fail(RSRL_HIP_ESTATE, "a prediction agent has a state-value function only (use rsrl_hip_q_evaluate for V(s))");
    // the TD ActorCritic: its value side is V(s) (no action values to search or weigh), its policy side the actor's theta
    if (is_v_actor_critic(c) && (op == QOP_FIND_MAX || op == QOP_FIND_MIN || op == QOP_EXPECTED))
        return fail(RSRL_HIP_ESTATE, "the TD ActorCritic's critic is a state-value function (use rsrl_hip_q_evaluate for V(s), the policy operations for the actor)");
    // NAC over the Gibbs policy: the critic is Q(s, a) = <w, psi(s, a)> over the stable compatible basis -- evaluated for every action (k_gibbs_nac_q); W is
    // one column of (A+1) F rows, not the A columns the searches and the weighted sum read
    if (is_gibbs_nac(c->cfg.algo) && (op == QOP_FIND_MAX || op == QOP_FIND_MIN || op == QOP_EXPECTED))
        return fail(RSRL_HIP_ESTATE, "RSRL_GIBBS_NAC's critic is Q(s, a) over the stable compatible basis: rsrl_hip_q_evaluate writes it for every action "
                                     "(no search or weighted sum over it; the policy operations read the actor)");
    // REINFORCE has no value function (BaselineREINFORCE's is the baseline B): only the policy's operations and the projection
    if (c->cfg.algo == RSRL_REINFORCE && (op == QOP_EVALUATE || op == QOP_FIND_MAX || op == QOP_FIND_MIN || op == QOP_EXPECTED))
        return fail(RSRL_HIP_ESTATE, "REINFORCE has no value function (use the policy operations; BaselineREINFORCE's value side is its baseline)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    CallFrame f(c);
    const float* d_states; float* d_fout; int32_t* d_iout; const float* d_fin; const int32_t* d_iin;
    TRY(f.in(states, (size_t)c->D * M_, &d_states));
    TRY(f.out(fout, fcount, &d_fout));
    TRY(f.out(iout, icount ? icount : (size_t)M_, &d_iout));
    TRY(check_host_actions(f, iin, (size_t)M_, c->A));
    TRY(f.in(fin, fin_count, &d_fin));
    TRY(f.in(iin, (size_t)M_, &d_iin));
    // the policy's operations read the policy's weights (ActorCritic: the Gibbs actor's theta), the rest the action-value function
    const bool policy_op = op == QOP_SAMPLE || op == QOP_SAMPLE_STEP || op == QOP_SAMPLE_INIT || op == QOP_MODE || op == QOP_PROBS || op == QOP_PROB_SA;
    Common k = policy_op ? make_policy_common(c) : make_common(c);
    // REINFORCE's driver-loop sample of an open episode is the behaviour policy's, pi_theta_b (kernels_reinforce.hpp): what train drew for batch-step t
    if (c->family == AgentFamily::ReinforceReg && op == QOP_SAMPLE_STEP) k.W = c->Zb;
    const uint64_t call = (op == QOP_SAMPLE_STEP || op == QOP_SAMPLE_INIT) ? step_t : c->api_calls;      // (the driver loop's sample: addressed by the batch-step)
    if (op == QOP_SAMPLE) c->api_calls++;
    const BasisGeom g = make_geom(c);
    if (is_gibbs_nac(c->cfg.algo) && op == QOP_EVALUATE) {                // Q(s, b) for every b: f32[A][M] against the learners' w and theta
        if (!launch_gibbs_nac_q(c->cfg.domain, c->cfg.order, c->stream, k, c->Z, d_states, M_, d_fout)) return NO_MODEL(c);
    } else if (has_lstd_state(c) && op == QOP_EVALUATE) {                 // V(s) = f32(phi(s) . theta), in f64 (k_lstd_v)
        if (!launch_lstd_v(feature_domain(c), c->cfg.order, c->stream, c->lstd_theta, d_states, M_, d_fout)) return NO_MODEL(c);
    } else if (is_td_v_continuous(c->cfg.algo) && op == QOP_EVALUATE) {   // V(s) of CACLA's / the continuous TD ActorCritic's TD learner: k_v_evaluate on MountainCar's projection
        if (!launch_v_evaluate(feature_domain(c), c->cfg.order, dim3(grid_for(M_)), dim3(kBlock), c->stream, k, d_states, M_, d_fout)) return NO_MODEL(c);
    } else if (is_continuous(c)) {                                        // QOP_FEATURES: MountainCar's projection at the same order
        if (!for_reg_fourier(RSRL_MOUNTAIN_CAR, c->cfg.order, [&](auto m) {
                hipLaunchKernelGGL((k_qop<typename decltype(m)::type>), dim3(grid_for(M_)), dim3(kBlock), 0, c->stream, k, g, op, d_states, M_, call, d_fout, d_iout, d_fin, d_iin);
            })) return NO_MODEL(c);
    } else if ((is_pred(c->cfg.algo) || is_tdac(c->cfg.algo) || is_gmc(c->cfg.algo) || is_gtd(c->cfg.algo)) && op == QOP_EVALUATE) {      // V(s) (the TD ActorCritic, GradientMC: their w; GTD2 / TDC: theta; k_v_evaluate)
        bool ok = true;
        switch (c->family) {
        case AgentFamily::WaveAux:
            for_wave(c, [&](auto tag) {
                using T = decltype(tag); using WT = typename T::wt;
                hipLaunchKernelGGL((k_wave_v_evaluate<T::domain, WT>), dim3(wave_grid_for(M_)), dim3(kBlock), 0, c->stream, (const WT*)c->W, d_states, M_, d_fout);
            });
            break;
        case AgentFamily::TdTile: ok = launch_v_tile(c->cfg.domain, c->cfg.n_tilings, c->stream, k, g, d_states, M_, d_fout); break;
        case AgentFamily::TdGeneric: ok = launch_v_model(c->cfg, dim3(grid_for(M_)), dim3(kBlock), c->stream, k, g, d_states, M_, d_fout); break;
        default: ok = launch_v_evaluate(c->cfg.domain, c->cfg.order, dim3(grid_for(M_)), dim3(kBlock), c->stream, k, d_states, M_, d_fout); break;
        }
        if (!ok) return NO_MODEL(c);
    } else if (c->family == AgentFamily::Hiv) {
        launch_hiv_qop(c->stream, k, g, op, d_states, M_, call, d_fout, d_iout, d_fin, d_iin);
    } else if (c->family == AgentFamily::CliffTable) {
        launch_table_qop(c->stream, k, op, d_states, M_, call, d_fout, d_iout, d_fin, d_iin);
    } else if (is_wave_family(c->family)) {
        for_wave(c, [&](auto tag) {
            using T = decltype(tag); using WT = typename T::wt;
            hipLaunchKernelGGL((k_wave_qop<T::domain, WT>), dim3(wave_grid_for(M_)), dim3(kBlock), 0, c->stream, k, (const WT*)c->W, op, d_states, M_, call, d_fout, d_iout,
                               d_fin, d_iin);
        });
    } else if (!for_model(c, [&](auto tag) {
            using M = typename decltype(tag)::type;
            hipLaunchKernelGGL((k_qop<M>), dim3(grid_for(M_)), dim3(kBlock), 0, c->stream, k, g, op, d_states, M_, call, d_fout, d_iout, d_fin, d_iin);
        })) return NO_MODEL(c);
    KCHECK();
    return f.finish();
}

int rsrl_hip_q_find_min(rsrl_hip_ctx* c, const float* states, int64_t M, int32_t* idx_out, float* val_out) {
    return qop(c, QOP_FIND_MIN, states, M, val_out, (size_t)M, idx_out);
}
int rsrl_hip_q_expected_value(rsrl_hip_ctx* c, const float* states, int64_t M, const float* probs, float* out) {
    if (!probs || !out) return fail(RSRL_HIP_EINVAL, "null argument");
    return qop(c, QOP_EXPECTED, states, M, out, (size_t)M, nullptr, 0, probs, c ? (size_t)c->A * M : 0);
}
int rsrl_hip_policy_prob(rsrl_hip_ctx* c, const float* states, const int32_t* actions, int64_t M, float* prob_out) {
    if (!actions || !prob_out) return fail(RSRL_HIP_EINVAL, "null argument");
    return qop(c, QOP_PROB_SA, states, M, prob_out, (size_t)M, nullptr, 0, nullptr, 0, actions);
}
int rsrl_hip_q_evaluate(rsrl_hip_ctx* c, const float* states, int64_t M, float* q_out) {
    if (!q_out) return fail(RSRL_HIP_EINVAL, "null argument");
    // (RSRL_GIBBS_NAC: one weight column, but a value per action)
    return qop(c, QOP_EVALUATE, states, M, q_out, c ? (size_t)(is_gibbs_nac(c->cfg.algo) ? c->A : c->Aw) * M : 0, nullptr);
}
int rsrl_hip_q_find_max(rsrl_hip_ctx* c, const float* states, int64_t M, int32_t* idx_out, float* val_out) {
    return qop(c, QOP_FIND_MAX, states, M, val_out, (size_t)M, idx_out);
}
// states == NULL: policy.sample(rng, env.emit().state()) for the ctx's OWN envs (M = n_envs) -- the driver loop's behaviour sample: it draws what
// batch-step step_count - 1 of rsrl_hip_train draws (the initial sample's stream before the first handle), and the actions also become the ctx's pending ones
static int sample_emit(rsrl_hip_ctx* c, int64_t M, int32_t* actions_out) {
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_policy_sample");
    if (M != c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "policy_sample(states = NULL) samples for the ctx's own envs: M must be n_envs (%lld), got %lld", (long long)c->cfg.n_envs, (long long)M);
    if (is_pred(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "a prediction agent has a state-value function only (use rsrl_hip_q_evaluate for V(s))");
    CallFrame f(c);
    int32_t* d_out;
    if (c->family == AgentFamily::LstdReg || c->family == AgentFamily::GmcReg || c->family == AgentFamily::LstdBatchReg || c->family == AgentFamily::GtdReg) {
        // RecursiveLSTD / iLSTD / GradientMC / LSTD / LSTDLambda / GTD2 / TDC: the driver loop's Random sample (what rsrl_hip_train draws at batch-step step_count - 1; the initial sample's stream
        // before the first handle), so that the trait-granular loop runs on the driver loop's draws
        FLUSH(c);
        HIP_TRY(hipSetDevice(c->cfg.device));
        TRY(f.out(actions_out, (size_t)M, &d_out));
        const Common k = make_common(c);
        launch_lstd_sample(c->cfg.domain, c->stream, k, c->t ? c->t - 1 : 0, c->t ? BLK_STEP : BLK_INIT, d_out);
        KCHECK();
        return f.finish();
    }
    if (c->tp.stage == 3 && f.device(actions_out)) {
        // the whole batch-step -- transition, handle, new episodes, sample -- as ONE kernel
        const rsrl_hip_ctx::TraitPend p = c->tp;
        c->tp.stage = 0;
        HIP_TRY(hipSetDevice(c->cfg.device));
        TRY(trait_cache_ready(c));
        const Common k = make_common(c);
        TraitIo io{};
        io.act = p.act; io.td_out = p.td; io.o_from = p.from; io.o_to = p.to; io.o_rew = p.rew; io.o_term = p.term; io.o_act = actions_out;
        io.qkey = c->tq_key; io.qval = c->tq_q; io.Mn = M;
        TRY(timing_begin(c));
        if (!launch_trait_lm(c->cfg.domain, c->cfg.order, c->cfg.algo, c->cfg.policy, c->stream, k, io, p.t_handle)) return NO_MODEL(c);
        KCHECK();
        c->kernel_name = "k_trait_lm<step>";
        return timing_end(c);
    }
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const uint64_t t = c->t ? c->t - 1 : 0;
    const uint32_t blk = c->t ? BLK_STEP : BLK_INIT;
    TRY(f.out(actions_out, (size_t)M, &d_out));
    if (trait_fast(c)) {
        TRY(trait_cache_ready(c));
        const Common k = make_common(c);
        TRY(timing_begin(c));
        if (!launch_trait_sample(c->cfg.domain, c->cfg.order, c->stream, k, nullptr, M, t, blk, c->tq_key, c->tq_q, d_out)) return NO_MODEL(c);
        KCHECK();
        TRY(timing_end(c));
        return f.finish();
    }
    TRY(qop(c, c->t ? QOP_SAMPLE_STEP : QOP_SAMPLE_INIT, c->state, M, nullptr, 0, d_out, 0, nullptr, 0, nullptr, t));      // (device pointers: the frame is this call's)
    HIP_TRY(hipMemcpyAsync(c->action, d_out, sizeof(int32_t) * (size_t)M, hipMemcpyDefault, c->stream));
    return f.finish();
}
int rsrl_hip_policy_sample(rsrl_hip_ctx* c, const float* states, int64_t M, int32_t* actions_out) {
    CHECK_CTX(c);
    if (!actions_out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!states) return sample_emit(c, M, actions_out);
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_policy_sample");
    if (trait_fast(c) && M >= 1 && M <= c->cfg.n_envs) {
        // the fast path's sample: a state the hand-over cache holds costs 20 B instead of the learner's 432 B of weights; same bits either way
        FLUSH(c);
        HIP_TRY(hipSetDevice(c->cfg.device));
        CallFrame f(c);
        const float* d_states; int32_t* d_out;
        TRY(f.in(states, (size_t)c->D * M, &d_states));
        TRY(f.out(actions_out, (size_t)M, &d_out));
        TRY(trait_cache_ready(c));
        const Common k = make_common(c);
        const uint64_t call = c->api_calls++;
        if (!launch_trait_sample(c->cfg.domain, c->cfg.order, c->stream, k, d_states, M, call, BLK_API, c->tq_key, c->tq_q, d_out)) return NO_MODEL(c);
        KCHECK();
        return f.finish();
    }
    return qop(c, QOP_SAMPLE, states, M, nullptr, 0, actions_out);
}
int rsrl_hip_policy_mode(rsrl_hip_ctx* c, const float* states, int64_t M, int32_t* actions_out) {
    CHECK_CTX(c);
    if (!actions_out) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_policy_mode");
    if (c->cfg.policy == RSRL_RANDOM) return fail(RSRL_HIP_EINVAL, "Random policy has no mode.");   // random.rs:47
    return qop(c, QOP_MODE, states, M, nullptr, 0, actions_out);
}
int rsrl_hip_policy_probs(rsrl_hip_ctx* c, const float* states, int64_t M, float* probs_out) {
    if (!probs_out) return fail(RSRL_HIP_EINVAL, "null argument");
    return qop(c, QOP_PROBS, states, M, probs_out, c ? (size_t)c->A * M : 0, nullptr);
}

int rsrl_hip_project(rsrl_hip_ctx* c, const float* states, int64_t M, float* phi_out) {
    CHECK_CTX(c);
    if (!phi_out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (c->cfg.basis != RSRL_FOURIER) return fail(RSRL_HIP_EINVAL, "dense projection needs a Fourier basis");
    return qop(c, QOP_FEATURES, states, M, phi_out, (size_t)c->F * M, nullptr);
}

int rsrl_hip_tile_indices(rsrl_hip_ctx* c, const float* states, int64_t M, int32_t* idx_out) {
    CHECK_CTX(c);
    if (!idx_out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (c->cfg.basis != RSRL_TILE_CODING) return fail(RSRL_HIP_EINVAL, "tile indices need a tile-coding basis");
    return qop(c, QOP_FEATURES, states, M, nullptr, 0, idx_out, (size_t)c->cfg.n_tilings * M);
}

int rsrl_hip_handle(rsrl_hip_ctx* c, const float* from_states, const int32_t* actions, const float* rewards,
                    const float* to_states, const uint8_t* terminal, int64_t M, float* td_error_out) {
    CHECK_CTX(c);
    if (!from_states || !actions || !rewards || !to_states || !terminal) return fail(RSRL_HIP_EINVAL, "null argument");
    if (M < 1 || M > c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "bad batch size");
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_handle");
    if (c->family == AgentFamily::ReinforceReg)
        return fail(RSRL_HIP_ESTATE, "REINFORCE and BaselineREINFORCE handle whole batches only (Handler<&Batch>): use rsrl_hip_handle_batch");
    if (c->family == AgentFamily::GmcReg)
        return fail(RSRL_HIP_ESTATE, "GradientMC handles whole trajectories only (Handler<&Trajectory>, visited last to first): use rsrl_hip_handle_batch");
    if (c->family == AgentFamily::LstdBatchReg)
        return fail(RSRL_HIP_ESTATE, "LSTD, LSTDLambda and LambdaLSPE handle whole batches only (Handler<&Batch>, then solve()): use rsrl_hip_handle_transitions");
    // the transition rsrl_hip_domain_step has just been handed (same arrays, every learner): accepted, launched with it (rsrl_hip_domain_step)
    CallFrame f(c);
    if (c->tp.stage == 1 && from_states == c->tp.from && actions == c->tp.act && rewards == c->tp.rew && to_states == c->tp.to && terminal == c->tp.term &&
        M == c->cfg.n_envs && !f.host(td_error_out)) {
        c->tp.stage = 2; c->tp.td = td_error_out; c->tp.t_handle = c->t;
        c->t += 1;
        return RSRL_HIP_OK;
    }
    FLUSH(c);
    if (c->st_rccl_group) return fail(RSRL_HIP_ESTATE, "this ctx is a rank of a single-thread RCCL group: handle() all-reduces the mini-batch delta, and one thread "
                                                       "cannot issue that for one rank at a time -- use one thread / process per rank, or RSRL_EXCHANGE_PEER");
    HIP_TRY(hipSetDevice(c->cfg.device));
    TRY(check_host_actions(f, actions, (size_t)M, c->A));
    Transitions io;
    TRY(stage_transitions(f, from_states, actions, rewards, to_states, terminal, M, td_error_out, &io));
    const Common k = make_common(c);
    const BasisGeom g = make_geom(c);
    if (c->family == AgentFamily::SharedSparseLambda) {
        // transition i is LEARNER i's (round 6): its residual against the shared table, its trace, the mini-batch's delta -- the driver loop's three launches on
        // the caller's transitions (kernels_sparse_lambda.hpp)
        const float step_size = (float)c->cfg.alpha;
        Common ks = k;
        ks.alg.kind = c->cfg.algo == RSRL_SARSA_LAMBDA ? ALG_SARSA : ALG_QLEARNING; ks.alg.lr = step_size;
        if (!for_model(c, [&](auto tag) {
                using Mo = typename decltype(tag)::type;
                if constexpr (Mo::kSparse) {
                    hipLaunchKernelGGL((k_sparse_handle<Mo>), dim3(grid_for(M)), dim3(kBlock), 0, c->stream, ks, g, io.from, io.act, io.rew, io.to, io.term, M, c->t,
                                       c->cfg.algo == RSRL_Q_LAMBDA ? 1 : 0, c->flags, c->sc_keys, c->sc_terms, io.td_out);
                    launch_sparse_trace_scatter(c, M, 0);
                }
            })) return NO_MODEL(c);
        KCHECK();
        const int n = (int)c->dw_elems;
        hipLaunchKernelGGL(k_apply_rep, dim3(((n + 1) / 2 + 255) / 256), dim3(256), 0, c->stream, c->multi ? (float*)nullptr : c->W, c->dW, c->dW_rep, c->n_rep, n,
                           tile_lsb(step_size));
        KCHECK();
        if (c->multi) {
            TRY(exchange_dw(c, c->t, nullptr, k.xdelta));
            if (c->cfg.exchange == RSRL_EXCHANGE_PEER) c->peer_seq += 1;
            hipLaunchKernelGGL(k_apply_dw, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->W, c->dW, n);
            KCHECK();
        }
        c->q_valid = false; c->tq_valid = false;
        c->t += 1;
        return f.finish();
    }
    if (trait_fast(c)) {
        TRY(launch_trait_handle(c, k, io.from, io.act, io.rew, io.to, io.term, M, c->t, io.td_out));
    } else {
        switch (family_row(c).handle) {
        case Handle::Wave:
            for_wave(c, [&](auto tag) {
                using T = decltype(tag); using WT = typename T::wt;
                hipLaunchKernelGGL((k_wave_handle<T::domain, WT>), dim3(wave_grid_for(M)), dim3(kBlock), 0, c->stream, k, (WT*)c->W, io.from, io.act, io.rew, io.to, io.term, M, c->t,
                                   io.td_out);
            });
            break;
        case Handle::Model:
            if (!for_model(c, [&](auto tag) {
                    using Mo = typename decltype(tag)::type;
                    hipLaunchKernelGGL((k_handle<Mo>), dim3(grid_for(M)), dim3(kBlock), 0, c->stream, k, g, io.from, io.act, io.rew, io.to, io.term, M, c->t, io.td_out, c->h_fx);
                })) return NO_MODEL(c);
            break;
        case Handle::Agent: TRY(launch_agent(c, k, g, c->t, 1, nullptr, &io));
        }
    }
    KCHECK();
    if (c->cfg.weight_mode == RSRL_W_SHARED) {
        // the mini-batch delta (accumulated in fixed point: exact, reproducible) of ALL ranks is applied by every rank (replicas
        // of W stay bit-identical): same exchange step as inside rsrl_hip_train
        const int n = (int)c->dw_elems;
        hipLaunchKernelGGL(k_fx_finalize, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->h_fx, c->dW, n, tile_lsb((float)c->cfg.lr));
        KCHECK();
        TRY(exchange_dw(c, c->t, nullptr, k.xdelta));
        if (c->multi && c->cfg.exchange == RSRL_EXCHANGE_PEER) c->peer_seq += 1;
        hipLaunchKernelGGL(k_apply_dw, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->W, c->dW, n);
        KCHECK();
    }
    c->q_valid = false;
    if (!trait_fast(c)) c->tq_valid = false;
    c->t += 1;          // one handle call = one batch-step of learning: the agent-side draws (SARSA's inner sample,
                        // bf16 stochastic rounding) advance exactly as they do inside rsrl_hip_train
    return f.finish();
}

// ---- f32 actions: the twins of the calls above for a continuous ctx (ContinuousMountainCar; cont_policy.hpp)
int rsrl_hip_domain_step_f32(rsrl_hip_ctx* c, const float* actions, float* from_states, float* next_states, float* rewards, uint8_t* terminal) {
    CHECK_CTX(c); FLUSH(c);
    NEEDS_F32_ACTIONS(c, "rsrl_hip_domain_step");
    c->q_valid = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    CallFrame f(c);
    TRY(check_host_actions_f32(f, actions, (size_t)c->cfg.n_envs, false));      // (Domain::transition maps the action onto its bounds itself)
    StepArrays<float> s;
    TRY(stage_step(f, actions, from_states, next_states, rewards, terminal, &s));
    const Common k = make_common(c);
    // (NAC and the continuous TD ActorCritic with Beta: explicit actions are the domain's, the pending ones the agent's -- stepped on through the loop's
    // 2a - 1; the Gaussian loops map nothing)
    launch_cmc_domain_step(c->stream, k, s.act, c->action_f, maps_beta_action(c), s.from, s.next, s.rew, s.term);
    KCHECK();
    return f.finish();
}

int rsrl_hip_handle_f32(rsrl_hip_ctx* c, const float* from_states, const float* actions, const float* rewards, const float* to_states,
                        const uint8_t* terminal, int64_t M, float* td_error_out) {
    CHECK_CTX(c);
    if (!from_states || !actions || !rewards || !to_states || !terminal) return fail(RSRL_HIP_EINVAL, "null argument");
    if (M < 1 || M > c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "bad batch size");
    NEEDS_F32_ACTIONS(c, "rsrl_hip_handle");
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    CallFrame f(c);
    TRY(check_host_actions_f32(f, actions, (size_t)M, false));      // (the update clamps the action to the sample's interval; Gaussian: taken as it is)
    TransitionsF32 io;
    TRY(stage_transitions(f, from_states, actions, rewards, to_states, terminal, M, td_error_out, &io));
    const Common k = make_common(c);
    const int order = c->cfg.order;
    if (!(is_nac(c->cfg.algo)           ? launch_nac(order, cont_policy(c), c->stream, k, make_cont(c), nac_period(c), c->t, 1, nullptr, &io)      // critic.handle: SARSA over SCB
          : has_lstd_state(c)           ? launch_tdac_beta(order, c->stream, k, make_tdac_beta(c), c->t, 1, nullptr, &io)
                                        : launch_td0_cont(order, is_cacla(c->cfg.algo), cont_policy(c), c->stream, k, make_cont(c), c->t, 1, nullptr, &io)))      // eval.handle, then the agent's
        return NO_MODEL(c);
    KCHECK();
    c->q_valid = false;
    c->t += 1;          // one handle call = one batch-step, as rsrl_hip_handle
    return f.finish();
}

// the policy side on explicit states (or, for the sample, the ctx's own envs): one launch of k_cont_policy
static int beta_op(rsrl_hip_ctx* c, int op, const float* states, int64_t M, uint64_t t, uint32_t purpose, const float* act_in, float* out0, float* out1, float* keep) {
    CallFrame f(c);
    TRY(check_host_actions_f32(f, act_in, (size_t)M, false));      // (rsrl_hip_policy_pdf's actions, the one caller with any)
    HIP_TRY(hipSetDevice(c->cfg.device));
    const float* d_states; const float* d_act; float* d_out0; float* d_out1;
    TRY(f.in(states, (size_t)c->D * M, &d_states));
    TRY(f.in(act_in, (size_t)M, &d_act));
    TRY(f.out(out0, (size_t)M, &d_out0));
    TRY(f.out(out1, (size_t)M, &d_out1));
    const Common k = make_common(c);
    if (!launch_cont_policy(c->cfg.order, cont_policy(c), c->stream, k, c->Z, op, d_states, M, t, purpose, d_act, d_out0, d_out1, keep)) return NO_MODEL(c);
    KCHECK();
    return f.finish();
}
static int beta_batch(rsrl_hip_ctx* c, const float* states, int64_t M) {
    if (!states || M < 1 || M > c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "bad batch (M=%lld, n_envs=%lld)", (long long)M, (long long)c->cfg.n_envs);
    return RSRL_HIP_OK;
}
int rsrl_hip_policy_sample_f32(rsrl_hip_ctx* c, const float* states, int64_t M, float* actions_out) {
    CHECK_CTX(c);
    if (!actions_out) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_F32_ACTIONS(c, "rsrl_hip_policy_sample");
    FLUSH(c);
    if (!states) {
        // the ctx's OWN envs: the driver loop's behaviour sample -- what batch-step step_count - 1 of rsrl_hip_train draws (the initial sample's
        // stream before the first handle) --, and the actions become the ctx's pending ones
        if (M != c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "policy_sample(states = NULL) samples for the ctx's own envs: M must be n_envs (%lld), got %lld", (long long)c->cfg.n_envs, (long long)M);
        return beta_op(c, BETA_OP_SAMPLE, nullptr, M, c->t ? c->t - 1 : 0, c->t ? BLK_STEP : BLK_INIT, nullptr, actions_out, nullptr, c->action_f);
    }
    TRY(beta_batch(c, states, M));
    return beta_op(c, BETA_OP_SAMPLE, states, M, c->api_calls++, BLK_API, nullptr, actions_out, nullptr, nullptr);
}
int rsrl_hip_policy_mode_f32(rsrl_hip_ctx* c, const float* states, int64_t M, float* actions_out) {
    CHECK_CTX(c);
    if (!actions_out) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_F32_ACTIONS(c, "rsrl_hip_policy_mode");
    FLUSH(c);
    TRY(beta_batch(c, states, M));
    return beta_op(c, BETA_OP_MODE, states, M, 0, 0, nullptr, actions_out, nullptr, nullptr);
}
static const char* const kNoBetaPolicy = "only the Beta policy (RSRL_BETA, on ContinuousMountainCar) has shape parameters and a density (and the Gaussian policy, "
                                         "RSRL_GAUSSIAN, a mean, a standard deviation and a density)";
int rsrl_hip_policy_params(rsrl_hip_ctx* c, const float* states, int64_t M, float* alpha_out, float* beta_out) {
    CHECK_CTX(c);
    if (!alpha_out || !beta_out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!is_continuous(c)) return fail(RSRL_HIP_ESTATE, "%s", kNoBetaPolicy);
    FLUSH(c);
    TRY(beta_batch(c, states, M));
    return beta_op(c, BETA_OP_PARAMS, states, M, 0, 0, nullptr, alpha_out, beta_out, nullptr);
}
int rsrl_hip_policy_pdf(rsrl_hip_ctx* c, const float* states, const float* actions, int64_t M, float* out) {
    CHECK_CTX(c);
    if (!actions || !out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!is_continuous(c)) return fail(RSRL_HIP_ESTATE, "%s", kNoBetaPolicy);
    FLUSH(c);
    TRY(beta_batch(c, states, M));
    return beta_op(c, BETA_OP_PDF, states, M, 0, 0, actions, out, nullptr, nullptr);
}

// ---- NAC (kernels_cont.hpp): the critic's Function<(S, A)> and the actor's update
static const char* const kNoNac = "only NAC (RSRL_NAC) has a critic over the stable compatible basis and an actor update of its own";
int rsrl_hip_q_evaluate_f32(rsrl_hip_ctx* c, const float* states, const float* actions, int64_t M, float* q_out) {
    CHECK_CTX(c);
    if (!actions || !q_out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!is_nac(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "%s", kNoNac);
    FLUSH(c);
    TRY(beta_batch(c, states, M));
    CallFrame f(c);
    TRY(check_host_actions_f32(f, actions, (size_t)M, false));      // (the score clamps the action to the sample's interval; Gaussian: taken as it is)
    HIP_TRY(hipSetDevice(c->cfg.device));
    const float* d_states; const float* d_act; float* d_q;
    TRY(f.in(states, (size_t)c->D * M, &d_states));
    TRY(f.in(actions, (size_t)M, &d_act));
    TRY(f.out(q_out, (size_t)M, &d_q));
    if (!launch_nac_q(c->cfg.order, cont_policy(c), c->stream, make_common(c), make_cont(c), d_states, d_act, M, d_q)) return NO_MODEL(c);
    KCHECK();
    return f.finish();
}
int rsrl_hip_nac_update(rsrl_hip_ctx* c, const uint8_t* mask, float* norm_out) {
    CHECK_CTX(c);
    if (!has_nac_update(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "%s", kNoNac);
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t N = (size_t)c->cfg.n_envs;
    CallFrame f(c);
    const uint8_t* d_mask; float* d_norm;
    TRY(f.in(mask, N, &d_mask));
    TRY(f.out(norm_out, N, &d_norm));
    // (k_nac_update reads w's first 2F rows and the two columns, whatever the policy: the Gaussian ctx runs it too)
    if (!(is_gibbs_nac(c->cfg.algo) ? launch_gibbs_nac_update(c->cfg.domain, c->cfg.order, c->stream, make_common(c), c->Z, d_mask, d_norm)      // (theta steps along w's first F A rows)
                                    : launch_nac_update(c->cfg.order, c->stream, make_common(c), make_cont(c), d_mask, d_norm))) return NO_MODEL(c);
    KCHECK();
    c->q_valid = false;
    return f.finish();
}

int rsrl_hip_handle_batch(rsrl_hip_ctx* c, int64_t T, const float* states, const int32_t* actions, const float* rewards, const uint32_t* lengths,
                          float* returns_out) {
    CHECK_CTX(c);
    const bool gmc = c->family == AgentFamily::GmcReg;      // Handler<&Trajectory>: reads no actions
    if (c->family != AgentFamily::ReinforceReg && !gmc)
        return fail(RSRL_HIP_ESTATE, "only REINFORCE, BaselineREINFORCE (Handler<&Batch>) and GradientMC (Handler<&Trajectory>) handle batches of (state, action, "
                                     "reward) rows; LSTD and LSTDLambda read whole transitions (rsrl_hip_handle_transitions), the other agents handle "
                                     "transitions one at a time (rsrl_hip_handle)");
    if (T < 0) return fail(RSRL_HIP_EINVAL, "bad batch length T = %lld", (long long)T);
    if (gmc) actions = nullptr;
    if (!lengths || (T > 0 && (!states || (!actions && !gmc) || !rewards))) return fail(RSRL_HIP_EINVAL, "null argument");
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs;
    // host arrays are validated where a learner's batch reads them (its rows 0 .. lengths[i]-1); device arrays are clamped by the kernel instead
    CallFrame f(c);
    const bool host_len = f.host(lengths), host_act = f.host(actions);
    if (host_len)
        for (int64_t i = 0; i < N; ++i)
            if ((int64_t)lengths[i] > T) return fail(RSRL_HIP_EINVAL, "lengths[%lld] = %u is more than the batch's %lld rows", (long long)i, lengths[i], (long long)T);
    if (host_len && host_act)
        for (int64_t i = 0; i < N; ++i)
            for (int64_t t = 0; t < (int64_t)lengths[i]; ++t)
                if (actions[t * N + i] < 0 || actions[t * N + i] >= c->A)
                    return fail(RSRL_HIP_EINVAL, "actions[%lld][%lld] = %d is outside [0, %d)", (long long)t, (long long)i, actions[t * N + i], c->A);
    ReinforceBatch io;
    const size_t TN = (size_t)T * (size_t)N;      // (T == 0: no rows to read, an empty copy back)
    TRY(f.in(T > 0 ? states : nullptr, TN * (size_t)c->D, &io.states));
    TRY(f.in(T > 0 ? actions : nullptr, TN, &io.act));
    TRY(f.in(T > 0 ? rewards : nullptr, TN, &io.rew));
    TRY(f.in(lengths, (size_t)N, &io.len));
    TRY(f.out(returns_out, TN, &io.ret_out));
    io.T = T;
    if (T > 0) {
        const Common k = make_common(c);
        const GmcBatch gio{io.states, io.rew, io.len, io.T, io.ret_out};
        if (gmc ? !launch_gmc(c->cfg.domain, c->cfg.order, dim3(grid_for(N)), dim3(kBlock), c->stream, k, make_gmc(c), c->t, 1, nullptr, &gio)
                : !launch_reinforce(c->cfg.domain, c->cfg.order, c->cfg.algo == RSRL_BASELINE_REINFORCE, dim3(grid_for(N)), dim3(kBlock), c->stream, k,
                                    make_reinforce(c), c->t, 1, nullptr, &io))
            return NO_MODEL(c);
        KCHECK();
    }
    c->q_valid = false;
    c->t += 1;          // one handle_batch call = one batch-step, as rsrl_hip_handle: the trait loop stays on the driver loop's draw streams
    return f.finish();
}

// Handler<&Batch>::handle of LSTD / LSTDLambda / LambdaLSPE for every learner (kernels_lstd_batch.hpp): whole transitions, then solve()
int rsrl_hip_handle_transitions(rsrl_hip_ctx* c, int64_t T, const float* from_states, const int32_t* actions, const float* rewards, const float* to_states,
                                const uint8_t* terminal, const uint32_t* lengths, float* td_out) {
    CHECK_CTX(c);
    (void)actions;      // (neither agent reads them)
    if (c->family != AgentFamily::LstdBatchReg)
        return fail(RSRL_HIP_ESTATE, "only LSTD, LSTDLambda and LambdaLSPE handle batches of whole transitions (Handler<&Batch> reading from, to, reward and the terminal "
                                     "flag); see rsrl_hip_handle and rsrl_hip_handle_batch for the other agents");
    if (T < 0) return fail(RSRL_HIP_EINVAL, "bad batch length T = %lld", (long long)T);
    if (!lengths || (T > 0 && (!from_states || !rewards || !to_states || !terminal))) return fail(RSRL_HIP_EINVAL, "null argument");
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs;
    CallFrame f(c);
    if (f.host(lengths))      // host lengths are validated; device ones are clamped by the kernel
        for (int64_t i = 0; i < N; ++i)
            if ((int64_t)lengths[i] > T) return fail(RSRL_HIP_EINVAL, "lengths[%lld] = %u is more than the batch's %lld rows", (long long)i, lengths[i], (long long)T);
    TransitionBatch io;
    const size_t TN = (size_t)T * (size_t)N;      // (T == 0: no rows to read, an empty copy back)
    TRY(f.in(T > 0 ? from_states : nullptr, TN * (size_t)c->D, &io.from));
    TRY(f.in(T > 0 ? rewards : nullptr, TN, &io.rew));
    TRY(f.in(T > 0 ? to_states : nullptr, TN * (size_t)c->D, &io.to));
    TRY(f.in(T > 0 ? terminal : nullptr, TN, &io.term));
    TRY(f.in(lengths, (size_t)N, &io.len));
    TRY(f.out(td_out, TN, &io.td_out));
    io.T = T;
    if (T > 0) {
        const Common k = make_common(c);
        const bool launched = c->cfg.algo == RSRL_LAMBDA_LSPE
            ? launch_lspe(c->cfg.domain, c->cfg.order, c->stream, k, make_lspe(c), c->t, 1, nullptr, &io)
            : launch_lstd_batch(c->cfg.domain, c->cfg.order, c->cfg.algo == RSRL_LSTD_LAMBDA, c->stream, k, make_lstd_batch(c), c->t, 1, nullptr, &io);
        if (!launched) return NO_MODEL(c);
        KCHECK();
    }
    c->q_valid = false;
    c->t += 1;          // one call = one batch-step, as rsrl_hip_handle_batch: the trait loop stays on the driver loop's draw streams
    return f.finish();
}

// the agents' public solve() (lstd.rs:40, lstd_lambda.rs:44) for every learner; LambdaLSPE's private one (lambda_lspe.rs:47) as handle ends with it
int rsrl_hip_lstd_solve(rsrl_hip_ctx* c) {
    CHECK_CTX(c); FLUSH(c);
    if (c->family != AgentFamily::LstdBatchReg) return fail(RSRL_HIP_ESTATE, "only LSTD, LSTDLambda and LambdaLSPE have a solve() of their own");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const bool launched = c->cfg.algo == RSRL_LAMBDA_LSPE
        ? launch_lspe_solve(c->cfg.domain, c->cfg.order, c->stream, make_lspe(c), c->cfg.n_envs)
        : launch_lstd_batch_solve(c->cfg.domain, c->cfg.order, c->cfg.algo == RSRL_LSTD_LAMBDA, c->stream, make_lstd_batch(c), c->cfg.n_envs);
    if (!launched) return NO_MODEL(c);
    KCHECK();
    c->q_valid = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
RSRL_API_END
