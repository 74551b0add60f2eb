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
    switch (c->cfg.domain) {
    case 0: hipLaunchKernelGGL(k_domain_step<0>, g, b, 0, c->stream, k, d_act, from, next, rew, term); break;
    case 1: hipLaunchKernelGGL(k_domain_step<1>, g, b, 0, c->stream, k, d_act, from, next, rew, term); break;
    case RSRL_CONTINUOUS_MOUNTAIN_CAR: return fail(RSRL_HIP_ESTATE, "ContinuousMountainCar steps on f32 actions (rsrl_hip_domain_step_f32)");
    default: hipLaunchKernelGGL(k_domain_step<2>, g, b, 0, c->stream, k, d_act, from, next, rew, term); break;
    }
    KCHECK();
    return RSRL_HIP_OK;
}
int launch_domain_reset(rsrl_hip_ctx* c, const Common& k, const uint8_t* d_mask) {
    const dim3 g(grid_for(c->cfg.n_envs)), b(kBlock);
    if (c->hiv_y) { launch_hiv_domain_reset(c->stream, k, c->hiv_y, d_mask); KCHECK(); return RSRL_HIP_OK; }
    switch (c->cfg.domain) {
    case 0: case RSRL_CONTINUOUS_MOUNTAIN_CAR:      // (ContinuousMountainCar: MountainCar's state space and start state)
        hipLaunchKernelGGL(k_domain_reset<0>, g, b, 0, c->stream, k, d_mask); break;
    case 1: hipLaunchKernelGGL(k_domain_reset<1>, g, b, 0, c->stream, k, d_mask); break;
    default: hipLaunchKernelGGL(k_domain_reset<2>, g, b, 0, c->stream, k, d_mask); break;
    }
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
// fused register-family loop: any split of n batch-steps into launches gives bit-identical results (Q(s,.) is carried between

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
    if (trait_fast(c) && c->own_stream && actions && from_states && next_states && rewards && terminal && is_device_ptr(actions) &&
        is_device_ptr(from_states) && is_device_ptr(next_states) && is_device_ptr(rewards) && is_device_ptr(terminal) && !c->sw.no_trait_defer) {
        c->tp = rsrl_hip_ctx::TraitPend{};
        c->tp.stage = 1; c->tp.act = actions; c->tp.from = from_states; c->tp.to = next_states; c->tp.rew = rewards; c->tp.term = terminal;
        return RSRL_HIP_OK;
    }
    const int64_t N = c->cfg.n_envs; const size_t DN = (size_t)c->D * N;
    const int32_t* d_act; OutBuf<float> ofrom, onext, orew; OutBuf<uint8_t> oterm;
    TRY(check_host_actions(actions, (size_t)N, c->A));
    TRY(stage_in(c, 0, actions, (size_t)N, &d_act));
    TRY(stage_out(c, 1, from_states, DN, &ofrom));
    TRY(stage_out(c, 2, next_states, DN, &onext));
    TRY(stage_out(c, 3, rewards, (size_t)N, &orew));
    TRY(stage_out(c, 4, terminal, (size_t)N, &oterm));
    const Common k = make_common(c);
    TRY(launch_domain_step(c, k, d_act, ofrom.dev, onext.dev, orew.dev, oterm.dev));
    bool sync = false;
    TRY(flush_out(c, &ofrom, &sync)); TRY(flush_out(c, &onext, &sync));
    TRY(flush_out(c, &orew, &sync)); TRY(flush_out(c, &oterm, &sync));
    if (sync || (actions && !is_device_ptr(actions))) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

int rsrl_hip_domain_reset(rsrl_hip_ctx* c, const uint8_t* mask) {
    CHECK_CTX(c);
    if (c->tp.stage == 2 && mask && mask == c->tp.term) { c->tp.stage = 3; return RSRL_HIP_OK; }      // the new episodes of the transition just handled
    FLUSH(c);
    c->q_valid = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs;
    const uint8_t* d_mask;
    TRY(stage_in(c, 0, mask, (size_t)N, &d_mask));
    const Common k = make_common(c);
    TRY(launch_domain_reset(c, k, d_mask));
    // REINFORCE: the restarted learners begin new episodes, sampled from theta as it stands (theta_b <- theta, g <- 0)
    if (c->family == AgentFamily::ReinforceReg) { launch_reinforce_restart(c->stream, make_reinforce(c), N, (int64_t)c->F * c->A, d_mask); KCHECK(); }
    if (mask && !is_device_ptr(mask)) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
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
    // REINFORCE has no value function (BaselineREINFORCE's is the baseline B): only the policy's operations and the projection
    if (c->cfg.algo == RSRL_REINFORCE && (op == QOP_EVALUATE || op == QOP_FIND_MAX || op == QOP_FIND_MIN || op == QOP_EXPECTED))
        return fail(RSRL_HIP_ESTATE, "REINFORCE has no value function (use the policy operations; BaselineREINFORCE's value side is its baseline)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const float* d_states; OutBuf<float> of; OutBuf<int32_t> oi;
    TRY(stage_in(c, 0, states, (size_t)c->D * M_, &d_states));
    TRY(stage_out(c, 1, fout, fcount, &of));
    TRY(stage_out(c, 2, iout, icount ? icount : (size_t)M_, &oi));
    const float* d_fin = nullptr; const int32_t* d_iin = nullptr;
    if (iin) TRY(check_host_actions(iin, (size_t)M_, c->A));
    TRY(stage_in(c, 3, fin, fin_count, &d_fin));
    TRY(stage_in(c, 4, iin, (size_t)M_, &d_iin));
    // the policy's operations read the policy's weights (ActorCritic: the Gibbs actor's theta), the rest the action-value function
    const bool policy_op = op == QOP_SAMPLE || op == QOP_SAMPLE_STEP || op == QOP_SAMPLE_INIT || op == QOP_MODE || op == QOP_PROBS || op == QOP_PROB_SA;
    Common k = policy_op ? make_policy_common(c) : make_common(c);
    // REINFORCE's driver-loop sample of an open episode is the behaviour policy's, pi_theta_b (kernels_reinforce.hpp): what train drew for batch-step t
    if (c->family == AgentFamily::ReinforceReg && op == QOP_SAMPLE_STEP) k.W = c->Zb;
    const uint64_t call = (op == QOP_SAMPLE_STEP || op == QOP_SAMPLE_INIT) ? step_t : c->api_calls;      // (the driver loop's sample: addressed by the batch-step)
    if (op == QOP_SAMPLE) c->api_calls++;
    const BasisGeom g = make_geom(c);
    if (has_lstd_state(c) && op == QOP_EVALUATE) {                        // V(s) = f32(phi(s) . theta), in f64 (k_lstd_v)
        if (!launch_lstd_v(feature_domain(c), c->cfg.order, c->stream, c->lstd_theta, d_states, M_, of.dev)) return NO_MODEL(c);
    } else if (is_continuous(c)) {                                        // QOP_FEATURES: MountainCar's projection at the same order
        bool ok = false;
#define X(DM, OR) if (DM == RSRL_MOUNTAIN_CAR && c->cfg.order == OR) { \
            hipLaunchKernelGGL((k_qop<FourierModel<DM, OR>>), dim3(grid_for(M_)), dim3(kBlock), 0, c->stream, k, g, op, d_states, M_, call, of.dev, oi.dev, d_fin, d_iin); ok = true; }
        RSRL_REG_FOURIER(X)
#undef X
        if (!ok) return NO_MODEL(c);
    } else if ((is_pred(c->cfg.algo) || is_tdac(c->cfg.algo) || is_gmc(c->cfg.algo) || is_gtd(c->cfg.algo)) && op == QOP_EVALUATE) {      // V(s) (the TD ActorCritic, GradientMC: their w; GTD2 / TDC: theta; k_v_evaluate)
        bool ok = true;
        switch (c->family) {
        case AgentFamily::WaveAux:
            for_wave(c, [&](auto tag) {
                using T = decltype(tag); using WT = typename T::wt;
                hipLaunchKernelGGL((k_wave_v_evaluate<T::domain, WT>), dim3(wave_grid_for(M_)), dim3(kBlock), 0, c->stream, (const WT*)c->W, d_states, M_, of.dev);
            });
            break;
        case AgentFamily::TdTile: ok = launch_v_tile(c->cfg.domain, c->cfg.n_tilings, c->stream, k, g, d_states, M_, of.dev); break;
        case AgentFamily::TdGeneric: ok = launch_v_model(c->cfg, dim3(grid_for(M_)), dim3(kBlock), c->stream, k, g, d_states, M_, of.dev); break;
        default: ok = launch_v_evaluate(c->cfg.domain, c->cfg.order, dim3(grid_for(M_)), dim3(kBlock), c->stream, k, d_states, M_, of.dev); break;
        }
        if (!ok) return NO_MODEL(c);
    } else if (c->family == AgentFamily::Hiv) {
        launch_hiv_qop(c->stream, k, g, op, d_states, M_, call, of.dev, oi.dev, d_fin, d_iin);
    } else if (is_wave_family(c->family)) {
        for_wave(c, [&](auto tag) {
            using T = decltype(tag); using WT = typename T::wt;
            hipLaunchKernelGGL((k_wave_qop<T::domain, WT>), dim3(wave_grid_for(M_)), dim3(kBlock), 0, c->stream, k, (const WT*)c->W, op, d_states, M_, call, of.dev, oi.dev,
                               d_fin, d_iin);
        });
    } else if (!for_model(c, [&](auto tag) {
            using M = typename decltype(tag)::type;
            hipLaunchKernelGGL((k_qop<M>), dim3(grid_for(M_)), dim3(kBlock), 0, c->stream, k, g, op, d_states, M_, call, of.dev, oi.dev, d_fin, d_iin);
        })) return NO_MODEL(c);
    KCHECK();
    bool sync = !is_device_ptr(states) || (fin && !is_device_ptr(fin)) || (iin && !is_device_ptr(iin));
    TRY(flush_out(c, &of, &sync)); TRY(flush_out(c, &oi, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
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
    return qop(c, QOP_EVALUATE, states, M, q_out, c ? (size_t)c->Aw * M : 0, nullptr);
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
    const bool dev_out = is_device_ptr(actions_out);
    if (c->family == AgentFamily::LstdReg || c->family == AgentFamily::GmcReg || c->family == AgentFamily::LstdBatchReg || c->family == AgentFamily::GtdReg) {
        // RecursiveLSTD / iLSTD / GradientMC / LSTD / LSTDLambda / GTD2 / TDC: the driver loop's Random sample (what rsrl_hip_train draws at batch-step step_count - 1; the initial sample's stream
        // before the first handle), so that the trait-granular loop runs on the driver loop's draws
        FLUSH(c);
        HIP_TRY(hipSetDevice(c->cfg.device));
        OutBuf<int32_t> oa;
        TRY(stage_out(c, 2, actions_out, (size_t)M, &oa));
        const Common k = make_common(c);
        launch_lstd_sample(c->cfg.domain, c->stream, k, c->t ? c->t - 1 : 0, c->t ? BLK_STEP : BLK_INIT, oa.dev);
        KCHECK();
        bool sync = false;
        TRY(flush_out(c, &oa, &sync));
        if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
        return RSRL_HIP_OK;
    }
    if (c->tp.stage == 3 && dev_out) {
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
    if (trait_fast(c)) {
        OutBuf<int32_t> oa;
        TRY(stage_out(c, 2, actions_out, (size_t)M, &oa));
        TRY(trait_cache_ready(c));
        const Common k = make_common(c);
        TRY(timing_begin(c));
        if (!launch_trait_sample(c->cfg.domain, c->cfg.order, c->stream, k, nullptr, M, t, blk, c->tq_key, c->tq_q, oa.dev)) return NO_MODEL(c);
        KCHECK();
        TRY(timing_end(c));
        bool sync = false;
        TRY(flush_out(c, &oa, &sync));
        if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
        return RSRL_HIP_OK;
    }
    TRY(qop(c, c->t ? QOP_SAMPLE_STEP : QOP_SAMPLE_INIT, c->state, M, nullptr, 0, actions_out, 0, nullptr, 0, nullptr, t));
    HIP_TRY(hipMemcpyAsync(c->action, actions_out, sizeof(int32_t) * (size_t)M, hipMemcpyDefault, c->stream));
    if (!dev_out) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
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
        const float* d_states; OutBuf<int32_t> oa;
        TRY(stage_in(c, 0, states, (size_t)c->D * M, &d_states));
        TRY(stage_out(c, 2, actions_out, (size_t)M, &oa));
        TRY(trait_cache_ready(c));
        const Common k = make_common(c);
        const uint64_t call = c->api_calls++;
        if (!launch_trait_sample(c->cfg.domain, c->cfg.order, c->stream, k, d_states, M, call, BLK_API, c->tq_key, c->tq_q, oa.dev)) return NO_MODEL(c);
        KCHECK();
        bool sync = !is_device_ptr(states);
        TRY(flush_out(c, &oa, &sync));
        if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
        return RSRL_HIP_OK;
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
        return fail(RSRL_HIP_ESTATE, "LSTD and LSTDLambda handle whole batches only (Handler<&Batch>, then solve()): use rsrl_hip_handle_transitions");
    // the transition rsrl_hip_domain_step has just been handed (same arrays, every learner): accepted, launched with it (rsrl_hip_domain_step)
    if (c->tp.stage == 1 && from_states == c->tp.from && actions == c->tp.act && rewards == c->tp.rew && to_states == c->tp.to && terminal == c->tp.term &&
        M == c->cfg.n_envs && (!td_error_out || is_device_ptr(td_error_out))) {
        c->tp.stage = 2; c->tp.td = td_error_out; c->tp.t_handle = c->t;
        c->t += 1;
        return RSRL_HIP_OK;
    }
    FLUSH(c);
    if (c->st_rccl_group) return fail(RSRL_HIP_ESTATE, "this ctx is a rank of a single-thread RCCL group: handle() all-reduces the mini-batch delta, and one thread "
                                                       "cannot issue that for one rank at a time -- use one thread / process per rank, or RSRL_EXCHANGE_PEER");
    HIP_TRY(hipSetDevice(c->cfg.device));
    TRY(check_host_actions(actions, (size_t)M, c->A));
    const float *d_from, *d_rew, *d_to; const int32_t* d_act; const uint8_t* d_term; OutBuf<float> otd;
    const bool all_device = is_device_ptr(from_states) && is_device_ptr(actions) && is_device_ptr(rewards) && is_device_ptr(to_states) && is_device_ptr(terminal) &&
                            (!td_error_out || is_device_ptr(td_error_out));
    TRY(stage_in(c, 0, from_states, (size_t)c->D * M, &d_from));
    TRY(stage_in(c, 1, actions, (size_t)M, &d_act));
    TRY(stage_in(c, 2, rewards, (size_t)M, &d_rew));
    TRY(stage_in(c, 3, to_states, (size_t)c->D * M, &d_to));
    TRY(stage_in(c, 4, terminal, (size_t)M, &d_term));
    TRY(stage_out(c, 5, td_error_out, (size_t)M, &otd));
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
                    hipLaunchKernelGGL((k_sparse_handle<Mo>), dim3(grid_for(M)), dim3(kBlock), 0, c->stream, ks, g, d_from, d_act, d_rew, d_to, d_term, M, c->t,
                                       c->cfg.algo == RSRL_Q_LAMBDA ? 1 : 0, c->flags, c->sc_keys, c->sc_terms, otd.dev);
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
        bool sync = !all_device;
        TRY(flush_out(c, &otd, &sync));
        if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
        return RSRL_HIP_OK;
    }
    if (trait_fast(c)) {
        TRY(launch_trait_handle(c, k, d_from, d_act, d_rew, d_to, d_term, M, c->t, otd.dev));
    } else {
        switch (family_row(c).handle) {
        case Handle::Wave:
            for_wave(c, [&](auto tag) {
                using T = decltype(tag); using WT = typename T::wt;
                hipLaunchKernelGGL((k_wave_handle<T::domain, WT>), dim3(wave_grid_for(M)), dim3(kBlock), 0, c->stream, k, (WT*)c->W, d_from, d_act, d_rew, d_to, d_term, M, c->t,
                                   otd.dev);
            });
            break;
        case Handle::Model:
            if (!for_model(c, [&](auto tag) {
                    using Mo = typename decltype(tag)::type;
                    hipLaunchKernelGGL((k_handle<Mo>), dim3(grid_for(M)), dim3(kBlock), 0, c->stream, k, g, d_from, d_act, d_rew, d_to, d_term, M, c->t, otd.dev, c->h_fx);
                })) return NO_MODEL(c);
            break;
        case Handle::Agent: {
            const Transitions io{d_from, d_act, d_rew, d_to, d_term, M, otd.dev};
            TRY(launch_agent(c, k, g, c->t, 1, nullptr, &io));
        }
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
    bool sync = !all_device;   // host inputs are staged asynchronously: they must have been read when the call returns; device arrays are asynchronous
    TRY(flush_out(c, &otd, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

// ---- f32 actions: the twins of the calls above for a continuous ctx (ContinuousMountainCar with the Beta policy; kernels_tdac_beta.hpp)
int rsrl_hip_domain_step_f32(rsrl_hip_ctx* c, const float* actions, float* from_states, float* next_states, float* rewards, uint8_t* terminal) {
    CHECK_CTX(c); FLUSH(c);
    NEEDS_F32_ACTIONS(c, "rsrl_hip_domain_step");
    c->q_valid = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs; const size_t DN = (size_t)c->D * N;
    const float* d_act; OutBuf<float> ofrom, onext, orew; OutBuf<uint8_t> oterm;
    TRY(check_host_actions_f32(actions, (size_t)N, false));      // (Domain::transition maps the action onto its bounds itself)
    TRY(stage_in(c, 0, actions, (size_t)N, &d_act));
    TRY(stage_out(c, 1, from_states, DN, &ofrom));
    TRY(stage_out(c, 2, next_states, DN, &onext));
    TRY(stage_out(c, 3, rewards, (size_t)N, &orew));
    TRY(stage_out(c, 4, terminal, (size_t)N, &oterm));
    const Common k = make_common(c);
    // (NAC: explicit actions are the domain's, the pending ones the agent's -- stepped on through the loop's 2a - 1)
    if (is_nac(c->cfg.algo)) launch_nac_domain_step(c->stream, k, d_act, c->action_f, ofrom.dev, onext.dev, orew.dev, oterm.dev);
    else launch_cmc_domain_step(c->stream, k, d_act, c->action_f, ofrom.dev, onext.dev, orew.dev, oterm.dev);
    KCHECK();
    bool sync = false;
    TRY(flush_out(c, &ofrom, &sync)); TRY(flush_out(c, &onext, &sync));
    TRY(flush_out(c, &orew, &sync)); TRY(flush_out(c, &oterm, &sync));
    if (sync || (actions && !is_device_ptr(actions))) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

int rsrl_hip_handle_f32(rsrl_hip_ctx* c, const float* from_states, const float* actions, const float* rewards, const float* to_states,
                        const uint8_t* terminal, int64_t M, float* td_error_out) {
    CHECK_CTX(c);
    if (!from_states || !actions || !rewards || !to_states || !terminal) return fail(RSRL_HIP_EINVAL, "null argument");
    if (M < 1 || M > c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "bad batch size");
    NEEDS_F32_ACTIONS(c, "rsrl_hip_handle");
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    TRY(check_host_actions_f32(actions, (size_t)M, false));      // (the update clamps the action to the sample's interval)
    TransitionsF32 io;
    OutBuf<float> otd;
    const bool all_device = is_device_ptr(from_states) && is_device_ptr(actions) && is_device_ptr(rewards) && is_device_ptr(to_states) && is_device_ptr(terminal) &&
                            (!td_error_out || is_device_ptr(td_error_out));
    TRY(stage_in(c, 0, from_states, (size_t)c->D * M, &io.from));
    TRY(stage_in(c, 1, actions, (size_t)M, &io.act));
    TRY(stage_in(c, 2, rewards, (size_t)M, &io.rew));
    TRY(stage_in(c, 3, to_states, (size_t)c->D * M, &io.to));
    TRY(stage_in(c, 4, terminal, (size_t)M, &io.term));
    TRY(stage_out(c, 5, td_error_out, (size_t)M, &otd));
    io.M = M; io.td_out = otd.dev;
    const Common k = make_common(c);
    if (!(is_nac(c->cfg.algo) ? launch_nac_beta(c->cfg.order, c->stream, k, make_nac_beta(c), c->t, 1, nullptr, &io)      // critic.handle: SARSA over SCB
                              : launch_tdac_beta(c->cfg.order, c->stream, k, make_tdac_beta(c), c->t, 1, nullptr, &io))) return NO_MODEL(c);
    KCHECK();
    c->q_valid = false;
    c->t += 1;          // one handle call = one batch-step, as rsrl_hip_handle
    bool sync = !all_device;
    TRY(flush_out(c, &otd, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

// the policy side on explicit states (or, for the sample, the ctx's own envs): one launch of k_beta_policy
static int beta_op(rsrl_hip_ctx* c, int op, const float* states, int64_t M, uint64_t t, uint32_t purpose, const float* act_in, float* out0, float* out1, float* keep) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    const float* d_states; const float* d_act; OutBuf<float> o0, o1;
    TRY(stage_in(c, 0, states, (size_t)c->D * M, &d_states));
    TRY(stage_in(c, 3, act_in, (size_t)M, &d_act));
    TRY(stage_out(c, 1, out0, (size_t)M, &o0));
    TRY(stage_out(c, 2, out1, (size_t)M, &o1));
    const Common k = make_common(c);
    if (!launch_beta_policy(c->cfg.order, c->stream, k, c->Z, op, d_states, M, t, purpose, d_act, o0.dev, o1.dev, keep)) return NO_MODEL(c);
    KCHECK();
    bool sync = (states && !is_device_ptr(states)) || (act_in && !is_device_ptr(act_in));
    TRY(flush_out(c, &o0, &sync)); TRY(flush_out(c, &o1, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
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
static const char* const kNoBetaPolicy = "only the Beta policy (RSRL_BETA, on ContinuousMountainCar) has shape parameters and a density";
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
    TRY(check_host_actions_f32(actions, (size_t)M, false));
    return beta_op(c, BETA_OP_PDF, states, M, 0, 0, actions, out, nullptr, nullptr);
}

// ---- NAC (kernels_nac_beta.hpp): the critic's Function<(S, A)> and the actor's update
static const char* const kNoNac = "only NAC (RSRL_NAC) has a critic over the stable compatible basis and an actor update of its own";
int rsrl_hip_q_evaluate_f32(rsrl_hip_ctx* c, const float* states, const float* actions, int64_t M, float* q_out) {
    CHECK_CTX(c);
    if (!actions || !q_out) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!is_nac(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "%s", kNoNac);
    FLUSH(c);
    TRY(beta_batch(c, states, M));
    TRY(check_host_actions_f32(actions, (size_t)M, false));      // (the score clamps the action to the sample's interval)
    HIP_TRY(hipSetDevice(c->cfg.device));
    const float* d_states; const float* d_act; OutBuf<float> oq;
    TRY(stage_in(c, 0, states, (size_t)c->D * M, &d_states));
    TRY(stage_in(c, 1, actions, (size_t)M, &d_act));
    TRY(stage_out(c, 2, q_out, (size_t)M, &oq));
    if (!launch_nac_q(c->cfg.order, c->stream, make_common(c), make_nac_beta(c), d_states, d_act, M, oq.dev)) return NO_MODEL(c);
    KCHECK();
    bool sync = !is_device_ptr(states) || !is_device_ptr(actions);
    TRY(flush_out(c, &oq, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_nac_update(rsrl_hip_ctx* c, const uint8_t* mask, float* norm_out) {
    CHECK_CTX(c);
    if (!is_nac(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "%s", kNoNac);
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t N = (size_t)c->cfg.n_envs;
    const uint8_t* d_mask; OutBuf<float> on;
    TRY(stage_in(c, 0, mask, N, &d_mask));
    TRY(stage_out(c, 1, norm_out, N, &on));
    if (!launch_nac_update(c->cfg.order, c->stream, make_common(c), make_nac_beta(c), d_mask, on.dev)) return NO_MODEL(c);
    KCHECK();
    c->q_valid = false;
    bool sync = mask && !is_device_ptr(mask);
    TRY(flush_out(c, &on, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
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
    const bool host_len = !is_device_ptr(lengths), host_act = actions && !is_device_ptr(actions);
    if (host_len)
        for (int64_t i = 0; i < N; ++i)
            if ((int64_t)lengths[i] > T) return fail(RSRL_HIP_EINVAL, "lengths[%lld] = %u is more than the batch's %lld rows", (long long)i, lengths[i], (long long)T);
    if (host_len && host_act)
        for (int64_t i = 0; i < N; ++i)
            for (int64_t t = 0; t < (int64_t)lengths[i]; ++t)
                if (actions[t * N + i] < 0 || actions[t * N + i] >= c->A)
                    return fail(RSRL_HIP_EINVAL, "actions[%lld][%lld] = %d is outside [0, %d)", (long long)t, (long long)i, actions[t * N + i], c->A);
    const bool all_device = !host_len && (T == 0 || (is_device_ptr(states) && !host_act && is_device_ptr(rewards))) && (!returns_out || is_device_ptr(returns_out));
    ReinforceBatch io;
    const size_t TN = (size_t)T * (size_t)N;
    TRY(stage_in(c, 0, T > 0 ? states : nullptr, TN * (size_t)c->D, &io.states));
    TRY(stage_in(c, 1, T > 0 ? actions : nullptr, TN, &io.act));
    TRY(stage_in(c, 2, T > 0 ? rewards : nullptr, TN, &io.rew));
    TRY(stage_in(c, 3, lengths, (size_t)N, &io.len));
    OutBuf<float> oret;
    TRY(stage_out(c, 4, T > 0 ? returns_out : nullptr, TN, &oret));
    io.T = T; io.ret_out = oret.dev;
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
    bool sync = !all_device;
    TRY(flush_out(c, &oret, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

// Handler<&Batch>::handle of LSTD / LSTDLambda for every learner (kernels_lstd_batch.hpp): whole transitions, then solve()
int rsrl_hip_handle_transitions(rsrl_hip_ctx* c, int64_t T, const float* from_states, const int32_t* actions, const float* rewards, const float* to_states,
                                const uint8_t* terminal, const uint32_t* lengths, float* td_out) {
    CHECK_CTX(c);
    (void)actions;      // (neither agent reads them)
    if (c->family != AgentFamily::LstdBatchReg)
        return fail(RSRL_HIP_ESTATE, "only LSTD and LSTDLambda handle batches of whole transitions (Handler<&Batch> reading from, to, reward and the terminal "
                                     "flag); see rsrl_hip_handle and rsrl_hip_handle_batch for the other agents");
    if (T < 0) return fail(RSRL_HIP_EINVAL, "bad batch length T = %lld", (long long)T);
    if (!lengths || (T > 0 && (!from_states || !rewards || !to_states || !terminal))) return fail(RSRL_HIP_EINVAL, "null argument");
    FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs;
    const bool host_len = !is_device_ptr(lengths);      // host lengths are validated; device ones are clamped by the kernel
    if (host_len)
        for (int64_t i = 0; i < N; ++i)
            if ((int64_t)lengths[i] > T) return fail(RSRL_HIP_EINVAL, "lengths[%lld] = %u is more than the batch's %lld rows", (long long)i, lengths[i], (long long)T);
    const bool all_device = !host_len && (T == 0 || (is_device_ptr(from_states) && is_device_ptr(rewards) && is_device_ptr(to_states) && is_device_ptr(terminal))) &&
                            (!td_out || is_device_ptr(td_out));
    TransitionBatch io;
    const size_t TN = (size_t)T * (size_t)N;
    TRY(stage_in(c, 0, T > 0 ? from_states : nullptr, TN * (size_t)c->D, &io.from));
    TRY(stage_in(c, 1, T > 0 ? rewards : nullptr, TN, &io.rew));
    TRY(stage_in(c, 2, T > 0 ? to_states : nullptr, TN * (size_t)c->D, &io.to));
    TRY(stage_in(c, 3, T > 0 ? terminal : nullptr, TN, &io.term));
    TRY(stage_in(c, 4, lengths, (size_t)N, &io.len));
    OutBuf<float> otd;
    TRY(stage_out(c, 5, T > 0 ? td_out : nullptr, TN, &otd));
    io.T = T; io.td_out = otd.dev;
    if (T > 0) {
        const Common k = make_common(c);
        if (!launch_lstd_batch(c->cfg.domain, c->cfg.order, c->cfg.algo == RSRL_LSTD_LAMBDA, c->stream, k, make_lstd_batch(c), c->t, 1, nullptr, &io)) return NO_MODEL(c);
        KCHECK();
    }
    c->q_valid = false;
    c->t += 1;          // one call = one batch-step, as rsrl_hip_handle_batch: the trait loop stays on the driver loop's draw streams
    bool sync = !all_device;
    TRY(flush_out(c, &otd, &sync));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

// the agents' public solve() (lstd.rs:40, lstd_lambda.rs:44) for every learner
int rsrl_hip_lstd_solve(rsrl_hip_ctx* c) {
    CHECK_CTX(c); FLUSH(c);
    if (c->family != AgentFamily::LstdBatchReg) return fail(RSRL_HIP_ESTATE, "only LSTD and LSTDLambda have a solve() of their own");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (!launch_lstd_batch_solve(c->cfg.domain, c->cfg.order, c->cfg.algo == RSRL_LSTD_LAMBDA, c->stream, make_lstd_batch(c), c->cfg.n_envs)) return NO_MODEL(c);
    KCHECK();
    c->q_valid = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
RSRL_API_END
