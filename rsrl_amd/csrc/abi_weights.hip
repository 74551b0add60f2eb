// abi_weights.hip -- Parameterised (params/mod.rs:116-134): weights, traces, fa_td's weights in the reference's (F, A) order; the checkpoint
// format (include/rsrl_hip.h); checksums.
#include "ctx.hpp"

// One learner's array between the caller's memory (host or device) and the device: launch(d_out, d_in) enqueues the kernel that fills d_out (a read,
// d_in null) or consumes d_in (a write, d_out null), n floats either way.  The call's frame is this helper's: a host array is staged and costs one
// synchronise; *synced says that a read waited for the device.
template <class Launch>
static int staged_rw(rsrl_hip_ctx* c, size_t n, float* out, const float* in, Launch&& launch, bool* synced = nullptr) {
    CallFrame f(c);
    float* d_out = nullptr; const float* d_in = nullptr;
    if (out) TRY(f.out(out, n, &d_out));
    else TRY(f.in(in, n, &d_in));
    launch(d_out, d_in);
    KCHECK();
    TRY(f.finish());
    if (synced && out) *synced = !f.all_device();
    return RSRL_HIP_OK;
}
// one learner's dense f32[F][cols] matrix out of, or into, a device buffer of W's layout (tile: the tile-coded tables'); wi = the learner's offset in it
// (rows: F, or the weight matrix's own count -- NAC's 3F)
static int matrix_rw(rsrl_hip_ctx* c, float* buf, bool tile, int cols, int64_t wi, float* out, const float* in, bool* synced = nullptr, int rows = 0) {
    const int F = rows ? rows : c->F, n = F * cols;
    return staged_rw(c, (size_t)n, out, in, [&](float* d_out, const float* d_in) {
        if (d_out) hipLaunchKernelGGL(k_weights_get, dim3((n + 255) / 256), dim3(256), 0, c->stream, buf, tile, c->w_stride, wi, F, cols, d_out);
        else hipLaunchKernelGGL(k_weights_set, dim3((n + 255) / 256), dim3(256), 0, c->stream, buf, tile, c->w_stride, wi, F, cols, d_in);
    }, synced);
}
// ... of the order-7 wave family's layout (kernels_wave.hpp): W in the ctx's storage type, the auxiliary matrix always f32
template <class WT>
static int wave_matrix_rw(rsrl_hip_ctx* c, WT* buf, int64_t env_index, float* out, const float* in, bool* synced = nullptr) {
    const int n = c->F * c->Aw;
    return staged_rw(c, (size_t)n, out, in, [&](float* d_out, const float* d_in) {
        if (d_out) hipLaunchKernelGGL((k_wave_weights_get<WT>), dim3((n + 255) / 256), dim3(256), 0, c->stream, (const WT*)buf + env_index * (int64_t)n, c->F, c->Aw, d_out);
        else hipLaunchKernelGGL((k_wave_weights_set<WT>), dim3((unsigned)(((int64_t)c->Aw * (c->F / 8) + 255) / 256)), dim3(256), 0, c->stream, buf, env_index, (int64_t)1, c->F, c->Aw, d_in);
    }, synced);
}
RSRL_API_BEGIN

static int no_value_function(rsrl_hip_ctx* c) {
    return fail(RSRL_HIP_ESTATE, "REINFORCE has no value function (its policy's weights: rsrl_hip_get/set_policy_weights)");
}
// RecursiveLSTD / iLSTD: the weights are theta (the reference's #[weights]), f64 on the device -- rounded to f32 on the way out, widened exactly on the
// way in; the matrix and mu are not touched
static int lstd_weights_rw(rsrl_hip_ctx* c, int64_t first, int64_t count, float* out, const float* in) {
    if (first < 0 || first + count > c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "env_index out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    return staged_rw(c, (size_t)c->F, out, in, [&](float* d_out, const float* d_in) {
        if (d_out) launch_lstd_theta_get(c->stream, c->lstd_theta, c->F, first, d_out);
        else launch_lstd_theta_set(c->stream, c->lstd_theta, c->F, first, count, d_in);
    });
}
// Parameterised::weights of one learner, read (out) or written (in)
static int weights_rw(rsrl_hip_ctx* c, int64_t env_index, float* out, const float* in) {
    if (c->cfg.algo == RSRL_REINFORCE) return no_value_function(c);
    if (has_lstd_state(c)) return lstd_weights_rw(c, env_index, 1, out, in);
    const bool shared = c->cfg.weight_mode == RSRL_W_SHARED;
    if (!shared && (env_index < 0 || env_index >= c->cfg.n_envs)) return fail(RSRL_HIP_EINVAL, "env_index out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    bool synced = false; int rc = RSRL_HIP_OK;
    if (is_wave(c->cfg)) {
        for_wave(c, [&](auto tag) {
            using WT = typename decltype(tag)::wt;
            rc = wave_matrix_rw(c, (WT*)c->W, env_index, out, in, &synced);
        });
    } else rc = matrix_rw(c, c->W, c->cfg.basis == RSRL_TILE_CODING, c->Aw, (shared ? 0 : env_index) * c->w_ls, out, in, &synced, c->Fw);
    return rc == RSRL_HIP_OK && synced ? peer_check(c) : rc;      // a failed exchange must not pass for weights
}
int rsrl_hip_get_weights(rsrl_hip_ctx* c, int64_t env_index, float* w) {
    CHECK_CTX(c); FLUSH(c); if (!w) return fail(RSRL_HIP_EINVAL, "null argument");
    return weights_rw(c, env_index, w, nullptr);
}
int rsrl_hip_set_weights(rsrl_hip_ctx* c, int64_t env_index, const float* w) {
    CHECK_CTX(c); FLUSH(c);
    c->q_valid = false; c->tq_valid = false; if (!w) return fail(RSRL_HIP_EINVAL, "null argument");
    return weights_rw(c, env_index, nullptr, w);
}
int traces_rw(rsrl_hip_ctx* c, int64_t env_index, float* out, const float* in) {
    CHECK_CTX(c); FLUSH(c);
    if (c->sp_keys) {
        // a learner's SPARSE trace over the shared table, shown as the dense (F, A) matrix it stands for; the list itself is not settable
        if (!out) return fail(RSRL_HIP_ESTATE, "the sparse traces of a shared-table lambda agent cannot be set from a dense matrix");
        if (env_index < 0 || env_index >= c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "env_index out of range");
        HIP_TRY(hipSetDevice(c->cfg.device));
        const int n = c->F * c->Aw;
        CallFrame f(c);
        float* d_out;
        TRY(f.out(out, (size_t)n, &d_out));
        HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(float) * (size_t)n, c->stream));
        hipLaunchKernelGGL(k_sparse_trace_get, dim3(kSparseCap / 256), dim3(256), 0, c->stream, SparseTrace{c->sp_keys, c->sp_vals, c->sp_len}, c->cfg.n_tilings, n / c->cfg.n_tilings, env_index, d_out);
        KCHECK();
        return f.finish();
    }
    if (!c->Z) return fail(RSRL_HIP_ESTATE, "this agent has no auxiliary matrix (eligibility trace / fa_td weights)");
    if (env_index < 0 || env_index >= c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "env_index out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (is_wave(c->cfg)) return wave_matrix_rw(c, c->Z, env_index, out, in);
    return matrix_rw(c, c->Z, c->cfg.basis == RSRL_TILE_CODING, aux_cols(c), env_index, out, in);
}
// the auxiliary matrix under its three public names: each refuses the agents that have no such matrix
static int aux_entry(rsrl_hip_ctx* c, int64_t env_index, float* out, const float* in, bool (*has)(const rsrl_hip_ctx*), const char* refusal) {
    if (!out && !in) return fail(RSRL_HIP_EINVAL, "null argument");
    CHECK_CTX(c);
    if (!has(c)) return fail(RSRL_HIP_ESTATE, "%s", refusal);
    return traces_rw(c, env_index, out, in);
}
static bool has_traces(const rsrl_hip_ctx* c) { return is_lambda(c->cfg.algo) || c->cfg.algo == RSRL_TD_LAMBDA; }
static bool has_td_weights(const rsrl_hip_ctx* c) { return c->cfg.algo == RSRL_GREEDY_GQ || is_gtd(c->cfg.algo); }      // (fa_td; GTD2's fa_w, TDC's td_est)
static const char* const kNoPolicyWeights = "only ActorCritic and REINFORCE have policy weights of their own (the policy reads Q otherwise)";
int rsrl_hip_get_traces(rsrl_hip_ctx* c, int64_t env_index, float* z) { return aux_entry(c, env_index, z, nullptr, has_traces, "this agent has no eligibility trace"); }
int rsrl_hip_set_traces(rsrl_hip_ctx* c, int64_t env_index, const float* z) { return aux_entry(c, env_index, nullptr, z, has_traces, "this agent has no eligibility trace"); }
int rsrl_hip_get_td_weights(rsrl_hip_ctx* c, int64_t env_index, float* v) { return aux_entry(c, env_index, v, nullptr, has_td_weights, "only GreedyGQ has a second approximator (fa_td)"); }
int rsrl_hip_set_td_weights(rsrl_hip_ctx* c, int64_t env_index, const float* v) { return aux_entry(c, env_index, nullptr, v, has_td_weights, "only GreedyGQ has a second approximator (fa_td)"); }
int rsrl_hip_get_policy_weights(rsrl_hip_ctx* c, int64_t env_index, float* theta) { return aux_entry(c, env_index, theta, nullptr, has_policy_weights, kNoPolicyWeights); }
int rsrl_hip_set_policy_weights(rsrl_hip_ctx* c, int64_t env_index, const float* theta) { return aux_entry(c, env_index, nullptr, theta, has_policy_weights, kNoPolicyWeights); }
// REINFORCE's open episode: the behaviour snapshot theta_b of one learner (f32[F][A], the weights' order) and every learner's running return g
static int behaviour_rw(rsrl_hip_ctx* c, int64_t env_index, float* out, const float* in) {
    if (!out && !in) return fail(RSRL_HIP_EINVAL, "null argument");
    CHECK_CTX(c); FLUSH(c);
    if (c->family != AgentFamily::ReinforceReg) return fail(RSRL_HIP_ESTATE, "only REINFORCE and BaselineREINFORCE carry a behaviour snapshot of their policy");
    if (env_index < 0 || env_index >= c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "env_index out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    return matrix_rw(c, c->Zb, false, c->A, env_index, out, in);
}
int rsrl_hip_get_behaviour_weights(rsrl_hip_ctx* c, int64_t env_index, float* theta_b) { return behaviour_rw(c, env_index, theta_b, nullptr); }
int rsrl_hip_set_behaviour_weights(rsrl_hip_ctx* c, int64_t env_index, const float* theta_b) { return behaviour_rw(c, env_index, nullptr, theta_b); }
// RecursiveLSTD / iLSTD: one learner's exact f64 state (theta [F], the matrix [F][F], iLSTD's mu [F]; mu may be null).  Host or device arrays
static int lstd_state_rw(rsrl_hip_ctx* c, int64_t env_index, double* theta, double* mat, double* mu, const double* theta_in, const double* mat_in,
                         const double* mu_in) {
    CHECK_CTX(c); FLUSH(c);
    if (!has_lstd_state(c)) return fail(RSRL_HIP_ESTATE, "only RecursiveLSTD and iLSTD (the iLSTD ActorCritic's critic included) carry a least-squares state");
    if (has_batch_lstd_state(c)) return fail(RSRL_HIP_ESTATE, "LSTD, LSTDLambda and LambdaLSPE carry A, b, z and singular_solves: rsrl_hip_get/set_lstd_batch_state");
    if (env_index < 0 || env_index >= c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "env_index out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    c->q_valid = false;
    const size_t F = (size_t)c->F, i = (size_t)env_index;
    const struct { double* dev; double* out; const double* in; size_t n; } parts[3] = {
        {c->lstd_theta + i * F, theta, theta_in, F}, {c->lstd_mat + i * F * F, mat, mat_in, F * F}, {c->lstd_mu ? c->lstd_mu + i * F : nullptr, mu, mu_in, F}};
    for (const auto& p : parts)      // (mu: iLSTD's only, and the caller's is optional)
        if (p.dev && (p.out || p.in)) HIP_TRY(hipMemcpyAsync(p.out ? (void*)p.out : p.dev, p.out ? (const void*)p.dev : p.in, 8 * p.n, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_get_lstd_state(rsrl_hip_ctx* c, int64_t env_index, double* theta, double* mat, double* mu) {
    if (!theta || !mat) return fail(RSRL_HIP_EINVAL, "null argument");
    return lstd_state_rw(c, env_index, theta, mat, mu, nullptr, nullptr, nullptr);
}
int rsrl_hip_set_lstd_state(rsrl_hip_ctx* c, int64_t env_index, const double* theta, const double* mat, const double* mu) {
    if (!theta || !mat) return fail(RSRL_HIP_EINVAL, "null argument");
    return lstd_state_rw(c, env_index, nullptr, nullptr, nullptr, theta, mat, mu);
}
// LSTD / LSTDLambda / LambdaLSPE: one learner's exact f64 state (theta [F], A [F][F], b [F], z [F] -- may be null: LSTDLambda's trace, or
// LambdaLSPE's z[0] = delta and z[1] = rows with zeros behind them) and its count of abandoned solves.  Host or device arrays
static int lstd_batch_state_rw(rsrl_hip_ctx* c, int64_t env_index, double* const out[4], const double* const in[4], uint32_t* sing, const uint32_t* sing_in) {
    CHECK_CTX(c); FLUSH(c);
    if (!has_batch_lstd_state(c)) return fail(RSRL_HIP_ESTATE, "only LSTD, LSTDLambda and LambdaLSPE carry the batch least-squares state (theta, A, b, z)");
    if (env_index < 0 || env_index >= c->cfg.n_envs) return fail(RSRL_HIP_EINVAL, "env_index out of range");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t F = (size_t)c->F, i = (size_t)env_index;
    const size_t nz = lstd_z_per_learner(c->cfg.algo, c->F);      // (of the caller's F: LambdaLSPE's pair leads it)
    const std::vector<double> zeros(out && out[3] && c->lstd_z && nz < F ? F - nz : 0, 0.0);      // (get: LambdaLSPE's z[2 ..]; alive until the synchronise below)
    if (in && in[3] && c->cfg.algo == RSRL_LAMBDA_LSPE) {
        // the row count steers the solve: checked before anything is installed (a device array through a host copy)
        double pair[2];
        HIP_TRY(hipMemcpyAsync(pair, in[3], sizeof(pair), hipMemcpyDefault, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!(pair[1] >= 0.0 && pair[1] <= (double)F && pair[1] == std::floor(pair[1])))
            return fail(RSRL_HIP_EINVAL, "LambdaLSPE: z[1] is the learner's row count, an integer in [0, %zu] (got %g)", F, pair[1]);
    }
    c->q_valid = false;
    const struct { double* dev; size_t n; } parts[4] = {
        {c->lstd_theta + i * F, F}, {c->lstd_mat + i * F * F, F * F}, {c->lstd_mu + i * F, F}, {c->lstd_z ? c->lstd_z + i * nz : nullptr, nz}};
    if (!zeros.empty()) HIP_TRY(hipMemcpyAsync(out[3] + nz, zeros.data(), 8 * zeros.size(), hipMemcpyDefault, c->stream));
    for (int p = 0; p < 4; ++p) {      // (z: LSTDLambda's only, and the caller's is optional)
        if (!parts[p].dev) continue;
        if (out && out[p]) HIP_TRY(hipMemcpyAsync(out[p], parts[p].dev, 8 * parts[p].n, hipMemcpyDefault, c->stream));
        if (in && in[p]) HIP_TRY(hipMemcpyAsync(parts[p].dev, in[p], 8 * parts[p].n, hipMemcpyDefault, c->stream));
    }
    if (sing) HIP_TRY(hipMemcpyAsync(sing, c->lstd_sing + i, sizeof(uint32_t), hipMemcpyDefault, c->stream));
    if (sing_in) HIP_TRY(hipMemcpyAsync(c->lstd_sing + i, sing_in, sizeof(uint32_t), hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_get_lstd_batch_state(rsrl_hip_ctx* c, int64_t env_index, double* theta, double* A, double* b, double* z, uint32_t* singular_solves) {
    if (!theta || !A || !b || !singular_solves) return fail(RSRL_HIP_EINVAL, "null argument");
    double* const out[4] = {theta, A, b, z};
    return lstd_batch_state_rw(c, env_index, out, nullptr, singular_solves, nullptr);
}
int rsrl_hip_set_lstd_batch_state(rsrl_hip_ctx* c, int64_t env_index, const double* theta, const double* A, const double* b, const double* z,
                                  const uint32_t* singular_solves) {
    if (!theta || !A || !b || !singular_solves) return fail(RSRL_HIP_EINVAL, "null argument");
    const double* const in[4] = {theta, A, b, z};
    return lstd_batch_state_rw(c, env_index, nullptr, in, nullptr, singular_solves);
}
static int return_carry_rw(rsrl_hip_ctx* c, float* out, const float* in) {
    CHECK_CTX(c); FLUSH(c); if (!out && !in) return fail(RSRL_HIP_EINVAL, "null argument");
    if (c->family != AgentFamily::ReinforceReg) return fail(RSRL_HIP_ESTATE, "only REINFORCE and BaselineREINFORCE carry an episode's running return");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(out ? out : c->ret_g, out ? c->ret_g : in, sizeof(float) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_get_return_carry(rsrl_hip_ctx* c, float* g) { return return_carry_rw(c, g, nullptr); }
int rsrl_hip_set_return_carry(rsrl_hip_ctx* c, const float* g) { return return_carry_rw(c, nullptr, g); }

RSRL_API_END
// ---- checkpoint: header, then the payload sections of the ctx's aux_kind ---------------------------------------------
// The header is serialised FIELD BY FIELD (little-endian, no implicit padding); layout in include/rsrl_hip.h.
namespace {
constexpr uint32_t kCkptVersionEps = 4;       // the file of a ctx that runs the per-learner epsilon schedule, whatever its aux_kind: f32 eps[N] follows the payload
constexpr int64_t kSparseChunk = 4096;        // learners per staging chunk of the sparse lists
constexpr size_t kCkptHeaderBytes = 72;
struct Ckpt {
    int32_t domain, basis, order, n_tilings, tiles_per_dim, weight_mode, F, A, algo, weight_dtype, aux_kind;
    int64_t n_learners; uint64_t step_count;
    bool has_eps;                                 // (not a header field: the file version says it)
};
// the payload sections (what each holds: kSection below); S_EPS is never a row's member -- it ends the file of any ctx that runs the schedule
enum SectionId : uint8_t { S_NONE = 0, S_WEIGHTS, S_AUX, S_BEHAVIOUR, S_LSTD, S_LSTD_BATCH, S_RING, S_SPARSE, S_EPS, S_COUNT };
// THE table: what a file of each aux_kind is.  An agent with state of its own adds a row here (its number: the agent's aux_kind in ctx.hpp kAlgo) and, if no section fits, a section below.
struct CkptKind {
    uint32_t version, older;     // written as `version` (the epsilon schedule's files: kCkptVersionEps); `older`, no longer written, is still read (0: none)
    bool eps;                    // configurations of this kind can run the epsilon schedule: version kCkptVersionEps is theirs too
    bool reads_kind0;            // a ctx of this kind also reads its configuration's version-2 / aux_kind-0 file, written before the kind's own section
    SectionId sections[3];       // travelled: the weights load, that section's state starts empty
};
constexpr int kCkptKinds = 20;
constexpr CkptKind kCkptKind[kCkptKinds] = {
    /* 0 weights only                           */ {2, 0, true, false, {S_WEIGHTS}},
    /* 1 eligibility traces                     */ {2, 0, true, false, {S_WEIGHTS, S_AUX}},
    /* 2 GreedyGQ's fa_td weights               */ {2, 0, false, false, {S_WEIGHTS, S_AUX}},
    /* 3 QSigma's n-step backups                */ {3, 0, false, true, {S_WEIGHTS, S_RING}},
    /* 4 sparse traces over a shared table      */ {6, 5, false, true, {S_WEIGHTS, S_SPARSE}},      // (5: no owner prefix in front of the lengths)
    /* 5 ActorCritic's theta                    */ {7, 0, false, false, {S_WEIGHTS, S_AUX}},
    /* 6 the TD ActorCritic's theta (A columns) */ {8, 0, false, false, {S_WEIGHTS, S_AUX}},
    /* 7 REINFORCE's theta and open episode     */ {9, 0, false, false, {S_WEIGHTS, S_AUX, S_BEHAVIOUR}},
    /* 8 the LSTD agents' f64 state             */ {10, 0, false, false, {S_LSTD}},
    /* 9 the iLSTD ActorCritic: f64 state, theta */ {10, 0, false, false, {S_LSTD, S_AUX}},      // (version 10 too: the aux_kind tells the two apart)
    /* 10 LSTD / LSTDLambda: f64 theta, A, b, z  */ {10, 0, false, false, {S_LSTD, S_LSTD_BATCH}},      // (version 10 as well; S_LSTD: theta, A, then b in mu's place)
    /* 11 the Beta iLSTD ActorCritic: f64 state, the policy's two columns */ {10, 0, false, false, {S_LSTD, S_AUX}},      // (kind 9's sections with f32[F][2] behind them)
    /* 12 NAC: the critic's w (3F rows), the policy's two columns */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},      // (version 10 as well: load's message names
                                                                                                                      // the versions read, and tests hold its text)
    /* 13 GTD2 / TDC: theta, the second column w */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},      // (version 10 as well; the header's algo tells the two agents apart)
    /* 14 NAC with the Gaussian policy: kind 12's sections */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},      // (the kind alone tells the two policies' files apart)
    /* 15 CACLA: the V learner's w, the Gaussian policy's two columns */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},      // (version 10 as well)
    /* 16 the continuous TD ActorCritic with the Beta policy: kind 15's sections */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},
    /* 17 ... with the Gaussian policy */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},      // (the kind alone tells the two policies' files, and CACLA's, apart)
    /* 18 NAC over the Gibbs policy: the critic's w ((A+1) F rows), theta (A columns) */ {10, 0, false, false, {S_WEIGHTS, S_AUX}},
    /* 19 LambdaLSPE: f64 theta, A, b, (delta, rows) */ {10, 0, false, false, {S_LSTD, S_LSTD_BATCH}},      // (kind 10's sections; the pair in z's place)
};
// (the kinds the configuration decides, not the algo: SARSALambda / QLambda over ONE shared tile table keep sparse traces instead of Z; the iLSTD
// ActorCritic with the Beta policy keeps two policy columns instead of the Gibbs actor's A; NAC's columns are the Gaussian policy's, not Beta's)
int aux_kind_of(const rsrl_hip_ctx* c) {
    if (c->family == AgentFamily::NacGaussReg) return 14;
    if (c->family == AgentFamily::TdAcGaussReg) return 17;
    return c->sp_keys ? 4 : (c->family == AgentFamily::TdAcBetaReg ? 11 : kAlgo[c->cfg.algo].aux_kind);
}
// is (version, aux_kind) a header this library writes, or ever wrote?
bool ckpt_pairing(uint32_t version, int32_t kind) {
    if (kind < 0 || kind >= kCkptKinds) return false;
    const CkptKind& k = kCkptKind[kind];
    return version == k.version || (k.older != 0 && version == k.older) || (k.eps && version == kCkptVersionEps);
}
// ... or the version-2 / aux_kind-0 file that a ctx of `kind` still reads (reads_kind0)?
bool ckpt_kind0_file(int32_t kind, uint32_t version, int32_t file_kind) { return kCkptKind[kind].reads_kind0 && file_kind == 0 && version == kCkptKind[0].version; }
bool ckpt_version_read(uint32_t version) {
    for (int k = 0; k < kCkptKinds; ++k) if (ckpt_pairing(version, k)) return true;
    return false;
}
// "2, 3, ... and 10": every version load reads
std::string ckpt_versions_read() {
    std::vector<uint32_t> vs;
    for (uint32_t v = 0; v < 256; ++v) if (ckpt_version_read(v)) vs.push_back(v);
    std::string s;
    for (size_t i = 0; i < vs.size(); ++i) s += (i == 0 ? "" : i + 1 == vs.size() ? " and " : ", ") + std::to_string(vs[i]);
    return s;
}
Ckpt ckpt_of(const rsrl_hip_ctx* c) {
    Ckpt h{};
    h.domain = c->cfg.domain; h.basis = c->cfg.basis; h.order = c->cfg.order; h.n_tilings = c->cfg.n_tilings;
    h.tiles_per_dim = c->cfg.tiles_per_dim; h.weight_mode = c->cfg.weight_mode; h.F = c->F; h.A = c->Aw;
    h.algo = c->cfg.algo; h.weight_dtype = c->cfg.weight_dtype; h.aux_kind = aux_kind_of(c);
    h.n_learners = c->cfg.weight_mode == RSRL_W_SHARED ? 1 : c->cfg.n_envs; h.step_count = c->t;
    h.has_eps = c->eps != nullptr;
    return h;
}
void put32(uint8_t*& p, uint32_t v) { for (int i = 0; i < 4; ++i) *p++ = (uint8_t)(v >> (8 * i)); }
void put64(uint8_t*& p, uint64_t v) { for (int i = 0; i < 8; ++i) *p++ = (uint8_t)(v >> (8 * i)); }
uint32_t get32(const uint8_t*& p) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)*p++ << (8 * i); return v; }
uint64_t get64(const uint8_t*& p) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= (uint64_t)*p++ << (8 * i); return v; }
void ckpt_encode(const Ckpt& h, uint8_t (&buf)[kCkptHeaderBytes]) {
    uint8_t* p = buf;
    memcpy(p, "RSRLHIPW", 8); p += 8;
    put32(p, h.has_eps ? kCkptVersionEps : kCkptKind[h.aux_kind].version);
    const int32_t f[11] = {h.domain, h.basis, h.order, h.n_tilings, h.tiles_per_dim, h.weight_mode, h.F, h.A, h.algo, h.weight_dtype, h.aux_kind};
    for (int32_t v : f) put32(p, (uint32_t)v);
    put64(p, (uint64_t)h.n_learners); put64(p, h.step_count);
}
bool ckpt_decode(const uint8_t (&buf)[kCkptHeaderBytes], Ckpt* h, uint32_t* version) {
    const uint8_t* p = buf;
    if (memcmp(p, "RSRLHIPW", 8) != 0) return false;
    p += 8;
    *version = get32(p);
    int32_t* f[11] = {&h->domain, &h->basis, &h->order, &h->n_tilings, &h->tiles_per_dim, &h->weight_mode, &h->F, &h->A, &h->algo, &h->weight_dtype, &h->aux_kind};
    for (int32_t* v : f) *v = (int32_t)get32(p);
    h->n_learners = (int64_t)get64(p); h->step_count = get64(p);
    h->has_eps = *version == kCkptVersionEps;
    return true;
}
// One save or load in flight: what the sections' operations share.  A load's staging lives here between a section's read and its install.
struct CkptIo {
    rsrl_hip_ctx* c; FILE* f; const char* path;
    int64_t n_learners;                           // 1 in shared mode
    uint32_t version = 0;                         // load: the file's
    bool kind0 = false;                           // load: a version-2 / aux_kind-0 file into a ctx whose row says reads_kind0 -- the kind's own section is not in it
    long long expect = (long long)kCkptHeaderBytes;      // load: the file's length, summed section by section
    std::vector<float> theta_b, g, ring, eps; std::vector<uint32_t> ring_hl, lstd_sing; std::vector<double> lstd, lstd_z;
    std::vector<uint32_t> sp_len_in, sp_len_t;    // sparse traces: a learner's entries in the file; its sub-lists' lengths on the device
    long sp_prefix = 0;
    uint16_t* spk_new = nullptr; float* spv_new = nullptr;      // sparse traces: shadow lists, switched in at the end like W
};
template <class T> int put(CkptIo& io, const T* p, size_t n) { return fwrite(p, sizeof(T), n, io.f) == n ? RSRL_HIP_OK : fail(RSRL_HIP_EINVAL, "short write to %s", io.path); }
template <class T> int get(CkptIo& io, T* p, size_t n) { return fread(p, sizeof(T), n, io.f) == n ? RSRL_HIP_OK : fail(RSRL_HIP_EINVAL, "%s: read error", io.path); }
// a section's arrays between the host and the device, then one synchronise (an array the ctx does not have is skipped); `what` opens the failure's message
struct Copy { void* dst; const void* src; size_t bytes; };
int copy_sync(rsrl_hip_ctx* c, hipMemcpyKind kind, std::initializer_list<Copy> copies, const char* what) {
    hipError_t e = hipSuccess;
    for (const Copy& x : copies) if (e == hipSuccess && x.dst && x.src) e = hipMemcpyAsync(x.dst, x.src, x.bytes, kind, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? RSRL_HIP_OK : fail(RSRL_HIP_EHIP, "%s: %s", what, hipGetErrorString(e));
}
int nothing(CkptIo&) { return RSRL_HIP_OK; }
// ---- matrices, learner by learner through the accessors above (the files' independence of the device layout rests on them) ----
using LearnerRw = int (*)(rsrl_hip_ctx*, int64_t, float*, const float*);
// (a load has switched the ctx to shadow copies of W and Z: the accessors fill those)
int matrices_io(CkptIo& io, size_t per, LearnerRw rw, bool write) {
    std::vector<float> w(per);
    int rc = RSRL_HIP_OK;
    for (int64_t i = 0; rc == RSRL_HIP_OK && per && i < io.n_learners; ++i) {
        rc = write ? rw(io.c, i, w.data(), nullptr) : get(io, w.data(), per);
        if (rc == RSRL_HIP_OK) rc = write ? put(io, w.data(), per) : rw(io.c, i, nullptr, w.data());
    }
    return rc;
}
int matrices_size(CkptIo& io, size_t per) { io.expect += io.n_learners * (long long)per * 4; return RSRL_HIP_OK; }
size_t weights_per(const rsrl_hip_ctx* c) { return c->cfg.algo == RSRL_REINFORCE ? 0 : (size_t)c->Fw * c->Aw; }
int weights_via_abi(rsrl_hip_ctx* c, int64_t i, float* out, const float* in) { return out ? rsrl_hip_get_weights(c, i, out) : rsrl_hip_set_weights(c, i, in); }
int weights_size(CkptIo& io) { return matrices_size(io, weights_per(io.c)); }
int weights_write(CkptIo& io) { return matrices_io(io, weights_per(io.c), weights_via_abi, true); }
int weights_read(CkptIo& io) { return matrices_io(io, weights_per(io.c), weights_via_abi, false); }
size_t aux_per(const rsrl_hip_ctx* c) { return (size_t)c->F * aux_cols(c); }
int aux_size(CkptIo& io) { return matrices_size(io, aux_per(io.c)); }
int aux_write(CkptIo& io) { return matrices_io(io, aux_per(io.c), traces_rw, true); }
int aux_read(CkptIo& io) { return matrices_io(io, aux_per(io.c), traces_rw, false); }
// ---- REINFORCE's open episode: read whole, installed (into Zb and ret_g themselves) only when everything has been read ----
size_t behaviour_per(const rsrl_hip_ctx* c) { return (size_t)c->F * c->A; }
int behaviour_size(CkptIo& io) { matrices_size(io, behaviour_per(io.c)); io.expect += (long long)io.c->cfg.n_envs * 4; return RSRL_HIP_OK; }
int behaviour_write(CkptIo& io) {
    int rc = matrices_io(io, behaviour_per(io.c), behaviour_rw, true);
    std::vector<float> g((size_t)io.c->cfg.n_envs);
    if (rc == RSRL_HIP_OK) rc = rsrl_hip_get_return_carry(io.c, g.data());
    return rc == RSRL_HIP_OK ? put(io, g.data(), g.size()) : rc;
}
int behaviour_read(CkptIo& io) {
    io.theta_b.resize((size_t)io.n_learners * behaviour_per(io.c)); io.g.resize((size_t)io.c->cfg.n_envs);
    const int rc = get(io, io.theta_b.data(), io.theta_b.size());
    return rc == RSRL_HIP_OK ? get(io, io.g.data(), io.g.size()) : rc;
}
int behaviour_install(CkptIo& io) {
    int rc = RSRL_HIP_OK;
    for (int64_t i = 0; rc == RSRL_HIP_OK && i < io.n_learners; ++i) rc = behaviour_rw(io.c, i, nullptr, io.theta_b.data() + (size_t)i * behaviour_per(io.c));
    return rc == RSRL_HIP_OK ? rsrl_hip_set_return_carry(io.c, io.g.data()) : rc;
}
// ---- the LSTD agents: the device arrays as they are, f64, learner-major ----
size_t lstd_doubles(const rsrl_hip_ctx* c) { const size_t nv = (size_t)c->F * (size_t)c->cfg.n_envs; return nv + nv * (size_t)c->F + (c->lstd_mu ? nv : 0); }
int lstd_size(CkptIo& io) { io.expect += (long long)lstd_doubles(io.c) * 8; return RSRL_HIP_OK; }
int lstd_write(CkptIo& io) {
    rsrl_hip_ctx* c = io.c; const size_t nv = (size_t)c->F * (size_t)c->cfg.n_envs;
    std::vector<double> buf(lstd_doubles(c));
    const int rc = copy_sync(c, hipMemcpyDeviceToHost, {{buf.data(), c->lstd_theta, 8 * nv}, {buf.data() + nv, c->lstd_mat, 8 * nv * c->F}, {buf.data() + nv + nv * c->F, c->lstd_mu, 8 * nv}}, "reading the LSTD state");
    return rc == RSRL_HIP_OK ? put(io, buf.data(), buf.size()) : rc;
}
int lstd_read(CkptIo& io) { io.lstd.resize(lstd_doubles(io.c)); return get(io, io.lstd.data(), io.lstd.size()); }
int lstd_install(CkptIo& io) {
    rsrl_hip_ctx* c = io.c; const size_t nv = (size_t)c->F * (size_t)c->cfg.n_envs; const double* in = io.lstd.data();
    return copy_sync(c, hipMemcpyHostToDevice, {{c->lstd_theta, in, 8 * nv}, {c->lstd_mat, in + nv, 8 * nv * c->F}, {c->lstd_mu, in + nv + nv * c->F, 8 * nv}}, "installing the LSTD state");
}
// ---- LSTD / LSTDLambda / LambdaLSPE, behind S_LSTD's theta, A and b: f64 z[N][F] (LSTDLambda) or f64 (delta, rows)[N] (LambdaLSPE), then u32
// singular_solves[N] ----
size_t lstd_z_doubles(const rsrl_hip_ctx* c) { return lstd_z_per_learner(c->cfg.algo, c->F) * (size_t)c->cfg.n_envs; }
int lstd_batch_size(CkptIo& io) { io.expect += (long long)lstd_z_doubles(io.c) * 8 + (long long)io.c->cfg.n_envs * 4; return RSRL_HIP_OK; }
int lstd_batch_write(CkptIo& io) {
    rsrl_hip_ctx* c = io.c;
    std::vector<double> z(lstd_z_doubles(c)); std::vector<uint32_t> sing((size_t)c->cfg.n_envs);
    int rc = copy_sync(c, hipMemcpyDeviceToHost, {{z.data(), c->lstd_z, 8 * z.size()}, {sing.data(), c->lstd_sing, 4 * sing.size()}}, "reading the LSTD batch state");
    if (rc == RSRL_HIP_OK) rc = put(io, z.data(), z.size());
    return rc == RSRL_HIP_OK ? put(io, sing.data(), sing.size()) : rc;
}
int lstd_batch_read(CkptIo& io) {
    io.lstd_z.resize(lstd_z_doubles(io.c)); io.lstd_sing.resize((size_t)io.c->cfg.n_envs);
    int rc = get(io, io.lstd_z.data(), io.lstd_z.size());
    for (size_t i = 0; rc == RSRL_HIP_OK && io.c->cfg.algo == RSRL_LAMBDA_LSPE && i < io.lstd_sing.size(); ++i) {
        const double rows = io.lstd_z[2 * i + 1];      // (the solve is steered by it)
        if (!(rows >= 0.0 && rows <= (double)io.c->F && rows == std::floor(rows))) rc = fail(RSRL_HIP_EINVAL, "%s: corrupt LambdaLSPE row count of learner %zu", io.path, i);
    }
    return rc == RSRL_HIP_OK ? get(io, io.lstd_sing.data(), io.lstd_sing.size()) : rc;
}
int lstd_batch_install(CkptIo& io) {
    rsrl_hip_ctx* c = io.c;
    return copy_sync(c, hipMemcpyHostToDevice, {{c->lstd_z, io.lstd_z.data(), 8 * io.lstd_z.size()}, {c->lstd_sing, io.lstd_sing.data(), 4 * io.lstd_sing.size()}},
                     "installing the LSTD batch state");
}
// ---- QSigma: every learner's Backup ring.  A kind-0 file has none: the run resumes from EMPTY backups, as after a terminal transition (q_sigma.rs:154) ----
size_t qs_floats(const rsrl_hip_ctx* c) { return (size_t)(c->D + 5) * (size_t)c->cfg.n_steps * (size_t)c->cfg.n_envs; }
int ring_size(CkptIo& io) { if (!io.kind0) io.expect += (long long)io.c->cfg.n_envs * 8 + (long long)qs_floats(io.c) * 4; return RSRL_HIP_OK; }
int ring_write(CkptIo& io) {
    rsrl_hip_ctx* c = io.c; const size_t N = (size_t)c->cfg.n_envs, nf = qs_floats(c);
    std::vector<uint32_t> hl(2 * N); std::vector<float> buf(nf);
    int rc = copy_sync(c, hipMemcpyDeviceToHost, {{hl.data(), c->qs_head, 4 * N}, {hl.data() + N, c->qs_len, 4 * N}, {buf.data(), c->qs_buf, 4 * nf}}, "reading the QSigma backups");
    if (rc == RSRL_HIP_OK) rc = put(io, hl.data(), 2 * N);
    return rc == RSRL_HIP_OK ? put(io, buf.data(), nf) : rc;
}
int ring_read(CkptIo& io) {
    if (io.kind0) return RSRL_HIP_OK;
    rsrl_hip_ctx* c = io.c; const size_t N = (size_t)c->cfg.n_envs;
    io.ring_hl.resize(2 * N); io.ring.resize(qs_floats(c));
    int rc = get(io, io.ring_hl.data(), 2 * N);
    if (rc == RSRL_HIP_OK) rc = get(io, io.ring.data(), io.ring.size());
    for (size_t i = 0; rc == RSRL_HIP_OK && i < N; ++i)
        if (io.ring_hl[i] >= (uint32_t)c->cfg.n_steps || io.ring_hl[N + i] > (uint32_t)c->cfg.n_steps) rc = fail(RSRL_HIP_EINVAL, "%s: corrupt QSigma backup of learner %zu", io.path, i);
    return rc;
}
int ring_install(CkptIo& io) {
    rsrl_hip_ctx* c = io.c; const size_t N = (size_t)c->cfg.n_envs;
    if (io.kind0) {
        hipError_t e = hipMemsetAsync(c->qs_len, 0, sizeof(uint32_t) * N, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->qs_head, 0, sizeof(uint32_t) * N, c->stream);
        return e == hipSuccess ? RSRL_HIP_OK : fail(RSRL_HIP_EHIP, "clearing the QSigma backups: %s", hipGetErrorString(e));
    }
    return copy_sync(c, hipMemcpyHostToDevice, {{c->qs_head, io.ring_hl.data(), 4 * N}, {c->qs_len, io.ring_hl.data() + N, 4 * N}, {c->qs_buf, io.ring.data(), 4 * io.ring.size()}}, "installing the QSigma backups");
}
// ---- sparse traces: u64 n_envs, u64 env_offset (whose learners these are), u32 len[N], then per learner its len keys and its len values -- the
// sub-lists concatenated in tiling order (a key says which tiling it belongs to: the file does not depend on the cap per tiling).  A kind-0 file has
// none: the run resumes from EMPTY lists (Trace::zeros) ----
// the lists are compact: their lengths, read here, say how long the file is
int sparse_size(CkptIo& io) {
    if (io.kind0) return RSRL_HIP_OK;
    rsrl_hip_ctx* c = io.c; const size_t N = (size_t)c->cfg.n_envs;
    int rc = RSRL_HIP_OK;
    io.sp_len_in.resize(N);
    io.sp_prefix = io.version == kCkptKind[4].older ? 0 : 16;
    uint8_t who[16];
    if (fseek(io.f, (long)io.expect, SEEK_SET) != 0 || (io.sp_prefix && fread(who, 1, 16, io.f) != 16))
        rc = fail(RSRL_HIP_EINVAL, "%s is truncated (the sparse traces' owner)", io.path);
    if (rc == RSRL_HIP_OK && io.sp_prefix) {                            // whose lists these are: the writer's shard, not only its size
        const uint8_t* wp = who; const uint64_t n_in = get64(wp), off_in = get64(wp);
        if (n_in != (uint64_t)N || off_in != (uint64_t)c->cfg.env_offset)
            rc = fail(RSRL_HIP_EINVAL, "%s was written by a different configuration (sparse traces of %llu learners at env_offset %llu; this ctx: %zu at %lld)", io.path,
                      (unsigned long long)n_in, (unsigned long long)off_in, N, (long long)c->cfg.env_offset);
    }
    if (rc == RSRL_HIP_OK && fread(io.sp_len_in.data(), 4, N, io.f) != N) rc = fail(RSRL_HIP_EINVAL, "%s is truncated (the sparse traces' lengths)", io.path);
    io.expect += io.sp_prefix + 4 * (long long)N;
    for (size_t i = 0; rc == RSRL_HIP_OK && i < N; ++i) {
        if (io.sp_len_in[i] > (uint32_t)kSparseCap) rc = fail(RSRL_HIP_EINVAL, "%s: corrupt sparse trace of learner %zu (%u entries)", io.path, i, io.sp_len_in[i]);
        io.expect += 8 * (long long)io.sp_len_in[i];
    }
    return rc;
}
int sparse_write(CkptIo& io) {
    rsrl_hip_ctx* c = io.c;
    const int64_t N = c->cfg.n_envs; const int T = c->cfg.n_tilings, cap = kSparseCap / T;
    const uint32_t slice = (uint32_t)c->F * (uint32_t)c->Aw / (uint32_t)T;                 // entries of one tiling's slice: the device's keys are relative to it
    std::vector<uint32_t> lens((size_t)N * T), tot((size_t)N);
    std::vector<uint16_t> keys((size_t)(kSparseChunk * kSparseCap));
    std::vector<float> vals((size_t)(kSparseChunk * kSparseCap));
    int rc = copy_sync(c, hipMemcpyDeviceToHost, {{lens.data(), c->sp_len, 4 * (size_t)N * T}}, "reading the sparse traces");
    for (int64_t i = 0; rc == RSRL_HIP_OK && i < N; ++i) {
        uint32_t sum = 0;
        for (int t = 0; t < T; ++t) {
            if (lens[(size_t)i * T + t] > (uint32_t)cap) rc = fail(RSRL_HIP_ESTATE, "learner %lld's sparse trace has %u entries in tiling %d", (long long)i, lens[(size_t)i * T + t], t);
            sum += lens[(size_t)i * T + t];
        }
        tot[(size_t)i] = sum;
    }
    uint8_t who[16]; uint8_t* wp = who; put64(wp, (uint64_t)N); put64(wp, (uint64_t)c->cfg.env_offset);
    if (rc == RSRL_HIP_OK) rc = put(io, who, 16);
    if (rc == RSRL_HIP_OK) rc = put(io, tot.data(), (size_t)N);
    std::vector<uint32_t> kk((size_t)kSparseCap); std::vector<float> vv((size_t)kSparseCap);
    for (int64_t i0 = 0; rc == RSRL_HIP_OK && i0 < N; i0 += kSparseChunk) {
        const int64_t n = std::min<int64_t>(kSparseChunk, N - i0);
        rc = copy_sync(c, hipMemcpyDeviceToHost, {{keys.data(), c->sp_keys + i0 * kSparseCap, 2 * (size_t)(n * kSparseCap)}, {vals.data(), c->sp_vals + i0 * kSparseCap, 4 * (size_t)(n * kSparseCap)}}, "reading the sparse traces");
        for (int64_t i = 0; rc == RSRL_HIP_OK && i < n; ++i) {
            size_t l = 0;
            for (int t = 0; t < T; ++t)
                for (uint32_t j = 0; j < lens[(size_t)(i0 + i) * T + t]; ++j, ++l) {
                    kk[l] = (uint32_t)t * slice + (uint32_t)keys[(size_t)(i * kSparseCap + t * cap) + j];      // (the file holds FULL keys: tile index * A + action)
                    vv[l] = vals[(size_t)(i * kSparseCap + t * cap) + j];
                }
            rc = put(io, kk.data(), l);
            if (rc == RSRL_HIP_OK) rc = put(io, vv.data(), l);
        }
    }
    return rc;
}
// into shadow lists (io.spk_new / spv_new: the load switches them in, or frees them); the sub-lists' lengths stay in io.sp_len_t for the install
int sparse_read(CkptIo& io) {
    if (io.kind0) return RSRL_HIP_OK;
    rsrl_hip_ctx* c = io.c; const char* path = io.path;
    int rc = RSRL_HIP_OK;
    const int64_t N = c->cfg.n_envs;
    hipError_t e2 = hipMalloc((void**)&io.spk_new, 2 * (size_t)kSparseCap * (size_t)N);
    if (e2 == hipSuccess) e2 = hipMalloc((void**)&io.spv_new, 4 * (size_t)kSparseCap * (size_t)N);
    if (e2 != hipSuccess) rc = fail(e2 == hipErrorOutOfMemory ? RSRL_HIP_ENOMEM : RSRL_HIP_EHIP, "staging buffers for the sparse traces: %s", hipGetErrorString(e2));
    std::vector<uint16_t> keys((size_t)(kSparseChunk * kSparseCap));
    std::vector<uint32_t> kk((size_t)kSparseCap);
    std::vector<float> vals((size_t)(kSparseChunk * kSparseCap)), vv((size_t)kSparseCap);
    if (rc == RSRL_HIP_OK && fseek(io.f, io.sp_prefix + 4 * (long)N, SEEK_CUR) != 0) rc = fail(RSRL_HIP_EINVAL, "%s: read error", path);      // (owner and lengths: read by sparse_size)
    const int T = c->cfg.n_tilings, cap = kSparseCap / T;
    const uint32_t n_keys = (uint32_t)c->F * (uint32_t)c->Aw, slice = n_keys / (uint32_t)T;
    io.sp_len_t.assign((size_t)N * T, 0u);
    for (int64_t i0 = 0; rc == RSRL_HIP_OK && i0 < N; i0 += kSparseChunk) {
        const int64_t n = std::min<int64_t>(kSparseChunk, N - i0);
        std::fill(keys.begin(), keys.end(), (uint16_t)0); std::fill(vals.begin(), vals.end(), 0.0f);
        for (int64_t i = 0; rc == RSRL_HIP_OK && i < n; ++i) {
            const size_t l = io.sp_len_in[(size_t)(i0 + i)];
            rc = get(io, kk.data(), l);
            if (rc == RSRL_HIP_OK) rc = get(io, vv.data(), l);
            for (size_t k = 0; rc == RSRL_HIP_OK && k < l; ++k) {         // every entry into the sub-list of its key's tiling
                if (kk[k] >= n_keys) { rc = fail(RSRL_HIP_EINVAL, "%s: corrupt sparse trace of learner %lld (key out of range)", path, (long long)(i0 + i)); break; }
                const uint32_t t = kk[k] / slice; uint32_t& lt = io.sp_len_t[(size_t)(i0 + i) * T + t];
                if (lt >= (uint32_t)cap) { rc = fail(RSRL_HIP_EINVAL, "%s: learner %lld's sparse trace holds more than %d entries of tiling %u (this library keeps "
                                                                        "%d entries per learner as %d per tiling)", path, (long long)(i0 + i), cap, t, kSparseCap, cap); break; }
                keys[(size_t)(i * kSparseCap + (int64_t)t * cap) + lt] = (uint16_t)(kk[k] - t * slice);      // (relative to the tiling's slice: < slice <= 65 536)
                vals[(size_t)(i * kSparseCap + (int64_t)t * cap) + lt] = vv[k];
                lt += 1;
            }
        }
        if (rc != RSRL_HIP_OK) break;
        rc = copy_sync(c, hipMemcpyHostToDevice, {{io.spk_new + i0 * kSparseCap, keys.data(), 2 * (size_t)(n * kSparseCap)}, {io.spv_new + i0 * kSparseCap, vals.data(), 4 * (size_t)(n * kSparseCap)}}, "installing the sparse traces");      // (synchronised: the next chunk reuses the staging vectors)
    }
    return rc;
}
// the lengths: the last step of a load that can fail (kCkptKind[4]: the row's last section, and no eps behind it)
int sparse_install(CkptIo& io) {
    rsrl_hip_ctx* c = io.c;
    if (io.kind0) {
        hipError_t e = hipMemsetAsync(c->sp_len, 0, sizeof(uint32_t) * (size_t)c->cfg.n_tilings * (size_t)c->cfg.n_envs, c->stream);
        return e == hipSuccess ? RSRL_HIP_OK : fail(RSRL_HIP_EHIP, "clearing the sparse traces: %s", hipGetErrorString(e));
    }
    return copy_sync(c, hipMemcpyHostToDevice, {{c->sp_len, io.sp_len_t.data(), 4 * io.sp_len_t.size()}}, "installing the sparse traces");
}
// ---- the epsilon schedule's state: every learner's current epsilon ----
int eps_size(CkptIo& io) { io.expect += (long long)io.c->cfg.n_envs * 4; return RSRL_HIP_OK; }
int eps_write(CkptIo& io) {
    std::vector<float> e((size_t)io.c->cfg.n_envs);
    const int rc = rsrl_hip_get_epsilons(io.c, e.data());
    return rc == RSRL_HIP_OK ? put(io, e.data(), e.size()) : rc;
}
int eps_read(CkptIo& io) {
    io.eps.resize((size_t)io.c->cfg.n_envs);
    int rc = get(io, io.eps.data(), io.eps.size());
    for (size_t i = 0; rc == RSRL_HIP_OK && i < io.eps.size(); ++i)
        if (!(io.eps[i] >= 0.0f && io.eps[i] <= 1.0f)) rc = fail(RSRL_HIP_EINVAL, "%s: epsilon of learner %zu is outside [0, 1]", io.path, i);
    return rc;
}
int eps_install(CkptIo& io) { return copy_sync(io.c, hipMemcpyHostToDevice, {{io.c->eps, io.eps.data(), 4 * io.eps.size()}}, "installing the learners' epsilons"); }
// A section: its bytes on file added to io.expect; written to the file; read into staging and validated; the staging installed into the ctx.
// The matrices of W and Z are "read" straight into the load's shadow copies and have nothing left to install.
struct Section { int (*size)(CkptIo&); int (*write)(CkptIo&); int (*read)(CkptIo&); int (*install)(CkptIo&); };
const Section kSection[S_COUNT] = {
    /* S_NONE      */ {nothing, nothing, nothing, nothing},
    /* S_WEIGHTS   */ {weights_size, weights_write, weights_read, nothing},                      // n_learners x f32[F][Aw]; absent for REINFORCE (no value function)
    /* S_AUX       */ {aux_size, aux_write, aux_read, nothing},                                  // n_learners x f32[F][aux_cols]: traces / fa_td's weights / the actor's theta
    /* S_BEHAVIOUR */ {behaviour_size, behaviour_write, behaviour_read, behaviour_install},      // n_learners x f32[F][A] of theta_b, then g[N]
    /* S_LSTD      */ {lstd_size, lstd_write, lstd_read, lstd_install},                          // f64: every learner's theta, then matrix, then (iLSTD) mu
    /* S_LSTD_BATCH */ {lstd_batch_size, lstd_batch_write, lstd_batch_read, lstd_batch_install},     // f64 z (LSTDLambda) or (delta, rows) (LambdaLSPE), then u32 singular_solves[N]
    /* S_RING      */ {ring_size, ring_write, ring_read, ring_install},                          // head[N], len[N], entries (SoA [field][slot][learner])
    /* S_SPARSE    */ {sparse_size, sparse_write, sparse_read, sparse_install},                  // owner prefix, len[N], every learner's keys and values
    /* S_EPS       */ {eps_size, eps_write, eps_read, eps_install},                              // eps[N]
};
// one operation of every section of h's file in turn (file order: its kind's row, then eps if the ctx runs the schedule), as long as none has failed
int for_sections(const Ckpt& h, int (*Section::*op)(CkptIo&), CkptIo& io, int rc = RSRL_HIP_OK) {
    for (SectionId id : kCkptKind[h.aux_kind].sections) if (rc == RSRL_HIP_OK) rc = (kSection[id].*op)(io);
    return rc == RSRL_HIP_OK && h.has_eps ? (kSection[S_EPS].*op)(io) : rc;
}
}  // namespace

RSRL_API_BEGIN

int rsrl_hip_save_weights(rsrl_hip_ctx* c, const char* path) {
    CHECK_CTX(c); FLUSH(c);
    if (!path) return fail(RSRL_HIP_EINVAL, "null path");
    FILE* f = fopen(path, "wb");
    if (!f) return fail(RSRL_HIP_EINVAL, "cannot open %s for writing", path);
    const Ckpt h = ckpt_of(c);
    CkptIo io{c, f, path, h.n_learners};
    uint8_t hdr[kCkptHeaderBytes]; ckpt_encode(h, hdr);
    int rc = for_sections(h, &Section::write, io, put(io, hdr, sizeof(hdr)));
    if (fclose(f) != 0 && rc == RSRL_HIP_OK) rc = fail(RSRL_HIP_EINVAL, "closing %s failed", path);
    return rc;
}
int rsrl_hip_load_weights(rsrl_hip_ctx* c, const char* path) {
    CHECK_CTX(c); FLUSH(c);
    if (!path) return fail(RSRL_HIP_EINVAL, "null path");
    HIP_TRY(hipSetDevice(c->cfg.device));
    FILE* f = fopen(path, "rb");
    if (!f) return fail(RSRL_HIP_EINVAL, "cannot open %s", path);
    const Ckpt want = ckpt_of(c);
    CkptIo io{c, f, path, want.n_learners};
    Ckpt h{}; uint8_t hdr[kCkptHeaderBytes];
    int rc = RSRL_HIP_OK;
    if (fread(hdr, 1, sizeof(hdr), f) != sizeof(hdr) || !ckpt_decode(hdr, &h, &io.version)) rc = fail(RSRL_HIP_EINVAL, "%s is not a rsrl_hip weight file", path);
    else if (!ckpt_version_read(io.version))
        rc = fail(RSRL_HIP_EINVAL, "%s has checkpoint version %u, this library reads versions %s", path, io.version, ckpt_versions_read().c_str());
    else if (!ckpt_pairing(io.version, h.aux_kind))      // not a file this library wrote
        rc = fail(RSRL_HIP_EINVAL, "%s: checkpoint version %u with aux_kind %d is not a valid pairing", path, io.version, h.aux_kind);
    io.kind0 = rc == RSRL_HIP_OK && ckpt_kind0_file(want.aux_kind, io.version, h.aux_kind);
    if (rc == RSRL_HIP_OK &&
        (h.domain != want.domain || h.basis != want.basis || h.order != want.order || h.n_tilings != want.n_tilings ||
         h.tiles_per_dim != want.tiles_per_dim || h.weight_mode != want.weight_mode || h.F != want.F || h.A != want.A ||
         h.algo != want.algo || h.weight_dtype != want.weight_dtype || (h.aux_kind != want.aux_kind && !io.kind0) || h.n_learners != want.n_learners ||
         h.has_eps != want.has_eps))
        rc = fail(RSRL_HIP_EINVAL, "%s was written by a different configuration%s", path,
                  h.has_eps != want.has_eps ? " (the per-learner epsilon schedule, config.epsilon_decay, is part of it)" : "");
    // the file's sections are the ctx's own (a kind-0 file's: the kind's own section counts as empty).  A truncated file is refused before anything is touched
    rc = for_sections(want, &Section::size, io, rc);
    if (rc == RSRL_HIP_OK && (fseek(f, 0, SEEK_END) != 0 || ftell(f) != io.expect || fseek(f, (long)kCkptHeaderBytes, SEEK_SET) != 0))
        rc = fail(RSRL_HIP_EINVAL, "%s is truncated or has trailing bytes (expected %lld bytes)", path, io.expect);
    if (rc != RSRL_HIP_OK) { fclose(f); return rc; }
    // staged: the file goes into shadow copies of W (and of the auxiliary matrix); the ctx switches to them only when
    // every learner has been read -- a failing load leaves the ctx exactly as it was
    float* W_old = c->W; float* Z_old = c->Z; float* W_new = nullptr; float* Z_new = nullptr;
    hipError_t e = hipMalloc((void**)&W_new, c->w_bytes);
    if (e == hipSuccess && Z_old) e = hipMalloc((void**)&Z_new, c->z_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(W_new, W_old, c->w_bytes, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && Z_old) e = hipMemcpyAsync(Z_new, Z_old, c->z_bytes, hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) {
        if (W_new) (void)hipFree(W_new);
        if (Z_new) (void)hipFree(Z_new);
        fclose(f);
        return fail(e == hipErrorOutOfMemory ? RSRL_HIP_ENOMEM : RSRL_HIP_EHIP, "staging buffers for %s: %s", path, hipGetErrorString(e));
    }
    c->W = W_new; c->Z = Z_new;
    // every section is read and validated before any of them installs into arrays that have no shadow (eps, the ring, theta_b, g, the LSTD state, the
    // sparse lengths)
    rc = for_sections(want, &Section::read, io);
    fclose(f);
    (void)hipStreamSynchronize(c->stream);
    rc = for_sections(want, &Section::install, io, rc);
    if (rc == RSRL_HIP_OK) {
        (void)hipFree(W_old); if (Z_old) (void)hipFree(Z_old);
        if (io.spk_new) { (void)hipFree(c->sp_keys); (void)hipFree(c->sp_vals); c->sp_keys = io.spk_new; c->sp_vals = io.spv_new; }
        c->t = h.step_count; c->q_valid = false; c->tq_valid = false;
    } else {
        std::string keep = g_last_error;
        c->W = W_old; c->Z = Z_old;
        (void)hipFree(W_new); if (Z_new) (void)hipFree(Z_new);
        if (io.spk_new) (void)hipFree(io.spk_new);
        if (io.spv_new) (void)hipFree(io.spv_new);
        g_last_error = keep;
    }
    return rc;
}

int rsrl_hip_set_weights_all(rsrl_hip_ctx* c, const float* w) {
    CHECK_CTX(c); FLUSH(c);
    c->q_valid = false; c->tq_valid = false; if (!w) return fail(RSRL_HIP_EINVAL, "null argument");
    if (c->cfg.algo == RSRL_REINFORCE) return no_value_function(c);
    if (has_lstd_state(c)) return lstd_weights_rw(c, 0, c->cfg.n_envs, nullptr, w);
    if (c->cfg.weight_mode == RSRL_W_SHARED) return rsrl_hip_set_weights(c, 0, w);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int n = c->Fw * c->Aw, gy = n < 1024 ? n : 1024;
    return staged_rw(c, (size_t)n, nullptr, w, [&](float*, const float* d_w) {
        if (is_wave(c->cfg)) {
            for_wave(c, [&](auto tag) {
                using WT = typename decltype(tag)::wt;
                const int64_t groups = c->cfg.n_envs * (int64_t)c->Aw * (c->F / 8);
                hipLaunchKernelGGL((k_wave_weights_set<WT>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, c->stream, (WT*)c->W, (int64_t)0, c->cfg.n_envs, c->F, c->Aw, d_w);
            });
        } else
        hipLaunchKernelGGL(k_weights_set_all, dim3(grid_for(c->cfg.n_envs), gy), dim3(kBlock), 0, c->stream, c->W, c->cfg.basis == RSRL_TILE_CODING, c->cfg.n_envs, c->cfg.basis == RSRL_TILE_CODING ? c->cfg.n_envs : c->w_stride, c->w_ls,
                           c->Fw, c->Aw, d_w);
    });
}

int rsrl_hip_checksum(rsrl_hip_ctx* c, uint64_t out[2]) {
    CHECK_CTX(c); FLUSH(c);
    if (!out) return fail(RSRL_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    TRY(scratch_reserve(c, 7, 2 * sizeof(unsigned long long)));
    unsigned long long* d = (unsigned long long*)c->scratch[7].p;
    HIP_TRY(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), c->stream));
    auto run = [&](const void* p, size_t bytes, size_t off, int slot) {
        const size_t n = bytes / 4;
        if (!p || n == 0) return;
        const unsigned g = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(k_checksum, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)p, n, off, d + slot);
    };
    const size_t N = (size_t)c->cfg.n_envs;
    if (c->w_ls != 1) hipLaunchKernelGGL(k_checksum_lm, dim3(4096), dim3(256), 0, c->stream, (const uint32_t*)c->W, (int64_t)N, c->A * c->F, d);
    else run(c->W, c->w_bytes, 0, 0);
    run(c->Z, c->Z ? c->z_bytes : 0, (size_t)1 << 40, 0);
    run(c->state, sizeof(float) * c->D * N, 0, 1);
    run(c->action, sizeof(int32_t) * N, (size_t)1 << 36, 1);
    run(c->ep_step, sizeof(uint32_t) * N, (size_t)1 << 37, 1);
    run(c->action_f, c->action_f ? sizeof(float) * N : 0, (size_t)1 << 39, 1);      // a continuous ctx's f32 actions
    run(c->hiv_y, c->hiv_y ? sizeof(double) * 6 * N : 0, (size_t)1 << 38, 1);      // HIVTreatment's hidden states (f64: two words each)
    // the LSTD agents' f64 state (two words per double) with the weights: theta, the matrices, iLSTD's mu
    run(c->lstd_theta, c->lstd_theta ? sizeof(double) * c->F * N : 0, (size_t)1 << 41, 0);
    run(c->lstd_mat, c->lstd_mat ? sizeof(double) * c->F * c->F * N : 0, (size_t)1 << 42, 0);
    run(c->lstd_mu, c->lstd_mu ? sizeof(double) * c->F * N : 0, (size_t)1 << 43, 0);
    run(c->lstd_z, c->lstd_z ? sizeof(double) * lstd_z_per_learner(c->cfg.algo, c->F) * N : 0, (size_t)1 << 44, 0);      // LSTDLambda's trace or LambdaLSPE's (delta, rows); the batch agents' abandoned solves
    run(c->lstd_sing, c->lstd_sing ? sizeof(uint32_t) * N : 0, (size_t)1 << 45, 0);
    KCHECK();
    unsigned long long h[2];
    HIP_TRY(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out[0] = h[0]; out[1] = h[1];
    return peer_check(c);
}

int rsrl_hip_fx_saturations(rsrl_hip_ctx* c, uint64_t* count_out) {
    CHECK_CTX(c); FLUSH(c);
    if (!count_out) return fail(RSRL_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned int n[4] = {0, 0, 0, 0};
    if (fx_saturations_train(&n[0]) || fx_saturations_trait(&n[1]) || fx_saturations_util(&n[2]) || fx_saturations_launch(&n[3])) { (void)hipGetLastError(); return fail(RSRL_HIP_EHIP, "reading the saturation counters"); }
    *count_out = (uint64_t)n[0] + n[1] + n[2] + n[3];
    return RSRL_HIP_OK;
}
RSRL_API_END
