// rsrl.hpp -- C++ host-side mirror of the rsrl trait surface for the TD-control hot path, on top of the
// C ABI (include/rsrl_hip.h).  The reference is Rust and this image has no Rust toolchain, so the host
// side above the ABI is C++ with the reference's names, argument meaning and error behaviour:
//
//   rsrl::domains::{MountainCar, CartPole, Acrobot}      rsrl_domains/src/{mountain_car/discrete,cart_pole,acrobot}.rs
//   rsrl::domains::ContinuousMountainCar, rsrl::policies::Beta      rsrl_domains/src/mountain_car/continuous.rs, rsrl/src/policies/beta.rs
//   rsrl::policies::Gaussian                                        rsrl/src/policies/gaussian/{mod,general}.rs
//   rsrl::control::cacla::CACLA                                     rsrl/src/control/cacla.rs
//   rsrl::control::ac::ActorCritic::tdac(TD, Gaussian | Beta, ..)    rsrl/src/control/ac.rs over prediction/td/td.rs (RSRL_CONTINUOUS_TD_ACTOR_CRITIC)
//   rsrl::fa::linear::{basis::Fourier, optim::SGD, LFA}  rsrl/src/fa/linear.rs (re-exports of crate lfa)
//   rsrl::domains::CliffWalk, rsrl::fa::tabular::Table              rsrl_domains/src/cliff_walk.rs, rsrl/src/fa/tabular/dense.rs
//   rsrl::policies::{Greedy, EpsilonGreedy, Softmax, Random}   rsrl/src/policies/*.rs
//   rsrl::control::td::{QLearning, SARSA, ExpectedSARSA, PAL, SARSALambda, QLambda, GreedyGQ, QSigma}   rsrl/src/control/td/*.rs
//   rsrl::prediction::td::{TD, TDLambda, GTD2, TDC}         rsrl/src/prediction/td/*.rs
//   rsrl::control::nac::NAC, rsrl::fa::linear::basis::SCB, LFA::scalar, control::td::SARSA over them      rsrl/src/control/nac.rs, fa/linear.rs:79-103
//   (over policies::Beta, policies::Gaussian and policies::Gibbs: examples/nac_beta.rs, nac.rs, nac_softmax.rs)
//   rsrl::make_shared / Shared<T>                            rsrl/src/core.rs:13-44
//
// Everything is BATCHED: a Domain is N environments, a state is a column of a [D][N] array.  The objects
// are light descriptors until `bind()` creates the device context (one per (domain, q_func, agent, policy)
// composition, exactly the object graph of examples/q_learning.rs:19-32).  Errors: the reference panics /
// returns Err; here every failure throws rsrl::Error carrying the ABI status and message.
#pragma once

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rsrl_hip.h"

namespace rsrl {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
    if (rc != RSRL_HIP_OK) throw Error(rc, rsrl_hip_last_error());
}

// core.rs:13-44 -- Shared<T> is Rc<RefCell<T>>; clones alias the same object
template <class T> using Shared = std::shared_ptr<T>;
template <class T> Shared<T> make_shared(T t) { return std::make_shared<T>(std::move(t)); }

// ---- rsrl_domains ---------------------------------------------------------------------------------
namespace domains {
struct Transition {                       // lib.rs:130-142, batched SoA
    std::vector<float> from, to;          // [D][N]
    std::vector<int32_t> action;          // [N]
    std::vector<float> reward;            // [N]
    std::vector<uint8_t> terminal;        // [N]  (Observation::Terminal flag of `to`, lib.rs:170)
};
struct Batch {                            // Batch = Vec<Transition> (lib.rs:210), one per learner, batched SoA: learner i's is rows 0 .. lengths[i]-1
    int64_t T = 0;                        // rows
    std::vector<float> states;            // [T][D][N]  each transition's `from` state
    std::vector<int32_t> actions;         // [T][N]
    std::vector<float> rewards;           // [T][N]
    std::vector<uint32_t> lengths;        // [N]  0 = no batch
    std::vector<float> to;                // [T][D][N]  each transition's `to` state      (read by LSTD / LSTDLambda only: whole transitions)
    std::vector<uint8_t> terminal;        // [T][N]     ... and its Observation::Terminal flag
};
struct Trajectory {                       // lib.rs:334-409, batched: `start` = states row 0, steps[k] = (states row k+1, actions[k], rewards[k])
    std::vector<uint32_t> n_states;       // [N]  Trajectory::n_states()  (:340); n_transitions = n_states - 1
    std::vector<float> total_reward;      // [N]  Trajectory::total_reward()  (:391)
    std::vector<float> states;            // [step_limit][D][N], rows past n_states are zero
    std::vector<int32_t> actions;         // [step_limit - 1][N]
    std::vector<float> rewards;           // [step_limit - 1][N]
    std::vector<uint8_t> terminal;        // [N]  the last observation is Observation::Terminal
};
struct Domain { int kind; int64_t n_envs; };
struct MountainCar : Domain { explicit MountainCar(int64_t n = 1) : Domain{RSRL_MOUNTAIN_CAR, n} {} };
struct CartPole : Domain { explicit CartPole(int64_t n = 1) : Domain{RSRL_CART_POLE, n} {} };
struct Acrobot : Domain { explicit Acrobot(int64_t n = 1) : Domain{RSRL_ACROBOT, n} {} };
struct HIVTreatment : Domain { explicit HIVTreatment(int64_t n = 1) : Domain{RSRL_HIV_TREATMENT, n} {} };     // hiv.rs: f64 hidden state (rsrl_hip_get_hidden_states)
// mountain_car/continuous.rs: MountainCar's state space with one f32 action in [-1, 1] (Session::transition_f32 / sample_f32; n_actions() is 0)
struct ContinuousMountainCar : Domain { explicit ContinuousMountainCar(int64_t n = 1) : Domain{RSRL_CONTINUOUS_MOUNTAIN_CAR, n} {} };
// cliff_walk.rs: CliffWalk::default(), height 5, width 12; states (x, y) as exact integers in f32, 4 actions (North, East, South, West); with
// fa::tabular::Table only
struct CliffWalk : Domain { explicit CliffWalk(int64_t n = 1) : Domain{RSRL_CLIFF_WALK, n} {} };
}  // namespace domains

// ---- rsrl::fa::linear ------------------------------------------------------------------------------
namespace fa { namespace linear {
namespace basis {
struct Fourier {                          // Fourier::from_space(order, space).with_bias()  (q_learning.rs:24)
    int order;
    bool bias = false;
    static Fourier from_space(int order, const domains::Domain&) { return Fourier{order}; }
    Fourier with_bias() const { Fourier f = *this; f.bias = true; return f; }
};
struct TileCoding { int n_tilings, tiles_per_dim; };
struct SCB;                               // (below namespace policies: it holds one)
}  // namespace basis
namespace optim { struct SGD { double lr; explicit SGD(double l) : lr(l) {} }; }
struct LFA {                              // LFA::vector(basis, SGD(lr), n_actions)  (q_learning.rs:25)
    int basis_kind, order, n_tilings, tiles_per_dim;
    double lr;
    bool shared_weights = false;          // one approximator for all envs (synchronous mini-batch rule)
    static LFA vector(const basis::Fourier& b, optim::SGD o, int /*n_actions*/) {
        if (!b.bias) throw Error(RSRL_HIP_EINVAL, "the device basis always carries the constant feature: call with_bias()");
        return LFA{RSRL_FOURIER, b.order, 0, 0, o.lr};
    }
    static LFA vector(const basis::TileCoding& b, optim::SGD o, int /*n_actions*/) {
        return LFA{RSRL_TILE_CODING, 0, b.n_tilings, b.tiles_per_dim, o.lr};
    }
    static inline LFA scalar(const basis::SCB& b, optim::SGD o);      // LFA::scalar(SCB{policy, basis}, SGD(lr)) (nac_beta.rs:38-42; defined below SCB)
};
}}  // namespace fa::linear

// ---- rsrl::fa::tabular (fa/tabular/dense.rs) ---------------------------------------------------------
// Table::zeros((n_rows, n_actions)): Q(s, .) is a row, the update adds the error to one entry.  The reference's Table has no optimiser (its agents step
// with size 1): `step` scales the error on the device, 1.0 being the reference's literal rule.  For domains::CliffWalk, 60 rows (row = x * 5 + y) of 4
namespace fa { namespace tabular {
struct Table : linear::LFA {
    static Table zeros(int n_rows, int n_actions, double step = 1.0) {
        if (n_rows != 60 || n_actions != 4) throw Error(RSRL_HIP_EINVAL, "the device table is CliffWalk::default()'s: 60 rows of 4 actions");
        Table t;
        t.basis_kind = RSRL_TABLE; t.order = 0; t.n_tilings = 0; t.tiles_per_dim = 0; t.lr = step;
        return t;
    }
};
}}  // namespace fa::tabular

// ---- rsrl::policies --------------------------------------------------------------------------------
namespace policies {
struct Policy {
    int kind; double epsilon = 0.0, tau = 1.0;
    // the reference drivers' schedule on the pub field: `agent.policy.epsilon *= decay` after every EPISODE of a learner
    // (examples/sarsa_lambda.rs:68); with N learners in one ctx every learner carries its own field.  1.0 = no schedule.
    double epsilon_decay = 1.0, epsilon_min = 0.0;
};
struct Random : Policy { explicit Random(int /*n_actions*/) : Policy{RSRL_RANDOM} {} };
struct Greedy : Policy {
    Shared<fa::linear::LFA> q;
    explicit Greedy(Shared<fa::linear::LFA> q_func) : Policy{RSRL_GREEDY}, q(std::move(q_func)) {}
};
struct EpsilonGreedy : Policy {           // EpsilonGreedy::new(greedy, random, epsilon)  (epsilon_greedy.rs:22-31)
    Shared<fa::linear::LFA> q;
    EpsilonGreedy(const Greedy& g, const Random&, double eps) : Policy{RSRL_EPSILON_GREEDY, eps}, q(g.q) {}
    // the driver's per-episode `policy.epsilon *= decay` (floored at `floor`) as part of the policy object
    EpsilonGreedy& decayed_per_episode(double decay, double floor = 0.0) { epsilon_decay = decay; epsilon_min = floor; return *this; }
};
struct Softmax : Policy {                 // Softmax::new(fa, tau) panics for |tau| < 1e-7 (softmax.rs:63-66)
    Shared<fa::linear::LFA> q;
    Softmax(Shared<fa::linear::LFA> q_func, double tau_) : Policy{RSRL_SOFTMAX, 0.0, tau_}, q(std::move(q_func)) {
        if (tau_ < 1e-7 && tau_ > -1e-7) throw Error(RSRL_HIP_EINVAL, "Tau parameter in Softmax must be non-zero.");
    }
};
// Gibbs::standard(fa) = Softmax over the actor's OWN approximator with tau 1 (softmax.rs:46-61); the actor of ActorCritic, whose weights are
// read through Session::policy_weights (its LFA's SGD rate never acts: ScaledGradientUpdate bypasses the optimiser, softmax.rs:216-222)
struct Gibbs : Softmax {
    explicit Gibbs(Shared<fa::linear::LFA> fa, double tau_ = 1.0) : Softmax(std::move(fa), tau_) {}
    static Gibbs standard(Shared<fa::linear::LFA> fa) { return Gibbs(std::move(fa)); }
};
// Beta::new(alpha, beta) (policies/beta.rs) with alpha = beta = Composition<ScalarLFA, Softplus> over the basis, zero weights: the policy of
// examples/tdac_beta.rs on ContinuousMountainCar.  Its two weight columns are read through Session::policy_weights ([F][2])
struct Beta : Policy {
    Shared<fa::linear::LFA> q;
    explicit Beta(const fa::linear::basis::Fourier& basis)
        : Policy{RSRL_BETA}, q(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 1))) {}
};
// Gaussian::new(mean, stddev) (policies/gaussian/mod.rs) with mean = ScalarLFA and stddev = Composition<ScalarLFA, Softplus> over the basis, SGD(1.0)
// on both, zero weights: the policy of examples/nac.rs on ContinuousMountainCar.  Its two weight columns (the mean's, the stddev's) are read through
// Session::policy_weights ([F][2]); Session::policy_params gives (mu, sd)
struct Gaussian : Policy {
    Shared<fa::linear::LFA> q;
    explicit Gaussian(const fa::linear::basis::Fourier& basis)
        : Policy{RSRL_GAUSSIAN}, q(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 1))) {}
};
}  // namespace policies

// SCB { policy, basis } (fa/linear.rs:79-103), the stable compatible basis: project((s, a)) = grad_log pi(a|s) chained with basis.project(s), 3F
// features over policies::Beta or policies::Gaussian, (A + 1) F over policies::Gibbs (held as the Policy they are: its kind is all the descriptor reads).  LFA::scalar(SCB, SGD(lr))
// is the q_func of NAC's SARSA critic (examples/nac_beta.rs, examples/nac.rs)
namespace fa { namespace linear {
namespace basis {
struct SCB { policies::Policy policy; Fourier basis; };
}  // namespace basis
inline LFA LFA::scalar(const basis::SCB& b, optim::SGD o) { return LFA::vector(b.basis, o, 1); }
}}  // namespace fa::linear

// ---- rsrl::control::td -----------------------------------------------------------------------------
namespace control { namespace td {
struct Agent {
    int algo; Shared<fa::linear::LFA> q_func; double gamma; double alpha = 1.0;
    int trace = RSRL_TRACE_ACCUMULATE; double lambda = 0.0;      // SARSALambda / QLambda
    double lr_td = 0.0;                                          // GreedyGQ: SGD rate of fa_td
    // the policy the AGENT owns (SARSA / ExpectedSARSA / SARSALambda / QSigma: pub field `policy`).  Unset: the behaviour
    // policy object itself, as in the reference's examples, which share one policy through make_shared.
    bool owns_policy = false; policies::Policy policy{RSRL_GREEDY};
    double sigma = 0.0; int n_steps = 1;                         // QSigma
    Agent& with_policy(const policies::Policy& p) { owns_policy = true; policy = p; return *this; }
};
struct QLearning : Agent { QLearning(Shared<fa::linear::LFA> q, double gamma) : Agent{RSRL_QLEARNING, std::move(q), gamma} {} };
// SARSA { q_func, policy, gamma }                                                  (control/td/sarsa.rs:35-41)
struct SARSA : Agent {
    SARSA(Shared<fa::linear::LFA> q, double gamma) : Agent{RSRL_SARSA, std::move(q), gamma} {}
    SARSA(Shared<fa::linear::LFA> q, const policies::Policy& p, double gamma) : Agent{RSRL_SARSA, std::move(q), gamma} { with_policy(p); }
};
// ExpectedSARSA { q_func, policy, alpha, gamma }                                   (control/td/expected_sarsa.rs:22-29)
struct ExpectedSARSA : Agent {
    ExpectedSARSA(Shared<fa::linear::LFA> q, double alpha_, double gamma) : Agent{RSRL_EXPECTED_SARSA, std::move(q), gamma, alpha_} {}
    ExpectedSARSA(Shared<fa::linear::LFA> q, const policies::Policy& p, double alpha_, double gamma)
        : Agent{RSRL_EXPECTED_SARSA, std::move(q), gamma, alpha_} { with_policy(p); }
};
// QSigma::new(q_func, policy, alpha, gamma, sigma, n_steps)                         (control/td/q_sigma.rs:94-105)
struct QSigma : Agent {
    QSigma(Shared<fa::linear::LFA> q, const policies::Policy& p, double alpha_, double gamma, double sigma_, int n_steps_)
        : Agent{RSRL_Q_SIGMA, std::move(q), gamma, alpha_} { with_policy(p); sigma = sigma_; n_steps = n_steps_; }
};
// PAL { q_func, alpha, gamma }                                                    (control/td/pal.rs:18-24)
struct PAL : Agent { PAL(Shared<fa::linear::LFA> q, double alpha_, double gamma) : Agent{RSRL_PAL, std::move(q), gamma, alpha_} {} };
}}  // namespace control::td

// ---- rsrl::traces: Trace::{accumulating, replacing, dutch}(dim, gamma, lambda)       (traces.rs:38-70)
namespace traces {
struct Trace {
    int rule; double gamma, lambda;
    static Trace accumulating(double gamma, double lambda) { return Trace{RSRL_TRACE_ACCUMULATE, gamma, lambda}; }
    static Trace replacing(double gamma, double lambda) { return Trace{RSRL_TRACE_SATURATE, gamma, lambda}; }
    static Trace dutch(double gamma, double lambda) { return Trace{RSRL_TRACE_DUTCH, gamma, lambda}; }
};
}  // namespace traces

namespace control { namespace td {
// SARSALambda { q_func, policy, trace, alpha, gamma } / QLambda                   (sarsa_lambda.rs:37-51, q_lambda.rs:37-54)
struct SARSALambda : Agent {
    SARSALambda(Shared<fa::linear::LFA> q, const traces::Trace& tr, double alpha_, double gamma)
        : Agent{RSRL_SARSA_LAMBDA, std::move(q), gamma, alpha_, tr.rule, tr.lambda} {}
    SARSALambda(Shared<fa::linear::LFA> q, const policies::Policy& p, const traces::Trace& tr, double alpha_, double gamma)
        : Agent{RSRL_SARSA_LAMBDA, std::move(q), gamma, alpha_, tr.rule, tr.lambda} { with_policy(p); }
};
struct QLambda : Agent {
    QLambda(Shared<fa::linear::LFA> q, const traces::Trace& tr, double alpha_, double gamma)
        : Agent{RSRL_Q_LAMBDA, std::move(q), gamma, alpha_, tr.rule, tr.lambda} {}
};
// GreedyGQ { fa_q, fa_td, behaviour_policy, gamma }                                (greedy_gq.rs:49-58)
struct GreedyGQ : Agent {
    GreedyGQ(Shared<fa::linear::LFA> fa_q, const fa::linear::LFA& fa_td, double gamma)
        : Agent{RSRL_GREEDY_GQ, std::move(fa_q), gamma, 1.0, RSRL_TRACE_ACCUMULATE, 0.0, fa_td.lr} {}
};
}}  // namespace control::td

// ---- rsrl::control::ac: ActorCritic { critic, policy, alpha } with the Gibbs actor and a SARSA critic    (control/ac.rs:49-115, examples/a2c.rs)
// critic: the SARSA evaluator (its q_func and gamma; it shares the actor as its policy, as the example does); the target is a2c.rs's closure
// Q(s,a) - sum_b Q(s,b) pi(b|s), or Q(s,a) for ActorCritic::qac (QCritic).  The Session's policy must be the same Gibbs object.
namespace prediction { namespace lstd { struct iLSTD; } namespace td { struct TD; } }
namespace control { namespace ac {
// TDCritic { gamma, v_func } (ac.rs:32-52): the target r + gamma V(s') - V(s), or r - V(s') on a terminal transition
struct TDCritic {
    double gamma; Shared<fa::linear::LFA> v_func;
};
struct ActorCritic : td::Agent {
    ActorCritic(const td::SARSA& critic, const policies::Gibbs& /*policy*/, double alpha_)
        : td::Agent{RSRL_ACTOR_CRITIC, critic.q_func, critic.gamma, alpha_} {}
    static ActorCritic qac(const td::SARSA& critic, const policies::Gibbs& policy, double alpha_) {
        ActorCritic a(critic, policy, alpha_); a.algo = RSRL_Q_ACTOR_CRITIC; return a;
    }
    // ActorCritic::tdac (ac.rs:87-98): TDCritic over a state-value function v_func (a ScalarLFA, one weight column), which the library learns
    // with TD(0) at v_func's SGD rate -- the `eval` of examples/tdac.rs.  The Session's weights are then V's [F][1]
    ActorCritic(const TDCritic& critic, const policies::Gibbs& /*policy*/, double alpha_)
        : td::Agent{RSRL_TD_ACTOR_CRITIC, critic.v_func, critic.gamma, alpha_} {}
    static ActorCritic tdac(Shared<fa::linear::LFA> v_func, const policies::Gibbs& policy, double alpha_, double gamma) {
        return ActorCritic(TDCritic{gamma, std::move(v_func)}, policy, alpha_);
    }
    // ActorCritic::tdac with examples/tdac.rs's own evaluator: TDCritic reads phi(s) . eval.theta, and iLSTD::handle runs before the actor's on
    // every transition (RSRL_ILSTD_ACTOR_CRITIC).  eval's alpha, gamma and n_updates are iLSTD's; gamma is TDCritic's and must be eval's.  The
    // Session's weights are iLSTD's theta as f32 [F][1]; Session::lstd_state(env, true) is the exact f64 state  (defined below iLSTD)
    static inline ActorCritic tdac(const prediction::lstd::iLSTD& eval, const policies::Gibbs& policy, double alpha_, double gamma);
    // ... generic over the policy: with policies::Beta on domains::ContinuousMountainCar, the agent of examples/tdac_beta.rs (same algo)
    static inline ActorCritic tdac(const prediction::lstd::iLSTD& eval, const policies::Beta& policy, double alpha_, double gamma);
    // ActorCritic::tdac over the continuous policies with TD(0) as `eval` (RSRL_CONTINUOUS_TD_ACTOR_CRITIC): prediction::td::TD{v_func, gamma}
    // handled before the agent on every transition, on domains::ContinuousMountainCar.  gamma is TDCritic's and must be eval's: the library runs
    // both with one.  The Session's weights are V's [F][1]; Session::handle(TransitionF32) is eval.handle then agent.handle.  The loop hands the
    // domain the action itself under Gaussian and 2a - 1 under Beta (include/rsrl_hip.h)  (defined below TD)
    static inline ActorCritic tdac(const prediction::td::TD& eval, const policies::Gaussian& policy, double alpha_, double gamma);
    static inline ActorCritic tdac(const prediction::td::TD& eval, const policies::Beta& policy, double alpha_, double gamma);
private:
    static inline ActorCritic tdac_cont(const prediction::td::TD& eval, double alpha_, double gamma);
};
}}  // namespace control::ac

// ---- rsrl::control::nac: NAC::new(critic, policy, alpha) (control/nac.rs) with policies::Beta or policies::Gaussian and a SARSA critic over
// fa::linear::basis::SCB on domains::ContinuousMountainCar, the agents of examples/nac_beta.rs and examples/nac.rs (whose loop hands the domain the
// action itself: Session::train and rollout_total_reward follow the policy's kind).  critic: its q_func (the SGD rate) and gamma; it shares the policy, as the
// example does.  `period`: the loop runs agent.handle(()) at every period-th step of an episode (nac_beta.rs:69 hard-codes 100).  The Session's
// weights are the critic's w [3F][1]; Session::handle(TransitionF32) is critic.handle, Session::nac_update() agent.handle(())
namespace control { namespace nac {
struct NAC : td::Agent {
    NAC(const td::SARSA& critic, const policies::Beta& /*policy*/, double alpha_, int period = 100)
        : td::Agent{RSRL_NAC, critic.q_func, critic.gamma, alpha_} { n_steps = period; }
    NAC(const td::SARSA& critic, const policies::Gaussian& /*policy*/, double alpha_, int period = 100)
        : td::Agent{RSRL_NAC, critic.q_func, critic.gamma, alpha_} { n_steps = period; }
    // NAC over policies::Gibbs on the domains with an enumerable action set, the agent of examples/nac_softmax.rs (RSRL_GIBBS_NAC): SCB's features are
    // grad_log flattened row-major, then phi -- (A + 1) F of them (include/rsrl_hip.h states the one line of SCB::project this restores).  The Session's
    // weights are the critic's w [(A + 1) F][1], Session::policy_weights the Gibbs policy's theta [F][A]; Session::handle(Transition) is critic.handle,
    // Session::nac_update() agent.handle(()), Session::evaluate Q(s, b) for every action b ([A][N])
    NAC(const td::SARSA& critic, const policies::Gibbs& /*policy*/, double alpha_, int period = 100)
        : td::Agent{RSRL_GIBBS_NAC, critic.q_func, critic.gamma, alpha_} { n_steps = period; }
};
}}  // namespace control::nac

// ---- rsrl::control::mc: REINFORCE { policy, alpha, gamma } / BaselineREINFORCE { baseline, policy, alpha, gamma }
// (control/mc/reinforce.rs, control/mc/baseline_reinforce.rs).  Handler<&Batch> only: Session::handle(const Batch&).  The policy is a Gibbs over its
// own LFA (Session::policy_weights); the baseline is a read-only VectorLFA (Session::weights).  The Session's policy must be the same Gibbs object
namespace control { namespace mc {
struct REINFORCE : td::Agent {
    REINFORCE(const policies::Gibbs& policy, double alpha_, double gamma_) : td::Agent{RSRL_REINFORCE, policy.q, gamma_, alpha_} {}
};
struct BaselineREINFORCE : td::Agent {
    BaselineREINFORCE(Shared<fa::linear::LFA> baseline, const policies::Gibbs& /*policy*/, double alpha_, double gamma_)
        : td::Agent{RSRL_BASELINE_REINFORCE, std::move(baseline), gamma_, alpha_} {}
};
}}  // namespace control::mc

// ---- rsrl::prediction::td: TD { v_func, gamma } / TDLambda { fa_theta, trace, gamma } / GTD2 / TDC   (td.rs:25-30, td_lambda.rs:25-32)
// The value function is a ScalarLFA (one weight column); drive these with policies::Random.
namespace prediction { namespace td {
struct TD : control::td::Agent {
    TD(Shared<fa::linear::LFA> v_func, double gamma) : control::td::Agent{RSRL_TD, std::move(v_func), gamma} {}
};
struct TDLambda : control::td::Agent {
    TDLambda(Shared<fa::linear::LFA> fa_theta, const traces::Trace& tr, double gamma)
        : control::td::Agent{RSRL_TD_LAMBDA, std::move(fa_theta), gamma, 1.0, tr.rule, tr.lambda} {}
};
// GTD2 { fa_theta, fa_w, gamma } / TDC { q_func, td_est, gamma }                    (gtd2.rs:27-33, tdc.rs:41-47)
// Gradient TD over two ScalarLFAs on one basis: the first is the value function (Session::weights), the second the correction's estimator
// (Session::td_weights).  The second LFA's rate goes to lr_td, as GreedyGQ's fa_td does.  The reference applies theta's updates -- and GTD2's w
// update -- past the optimiser, with step size 1, which diverges on a Fourier basis: here the first LFA's rate scales every move of theta and the
// second's every move of w (include/rsrl_hip.h, RSRL_GTD2); SGD(1.0) on both is the literal GTD2, SGD(1.0) on q_func the literal TDC.
struct GTD2 : control::td::Agent {
    GTD2(Shared<fa::linear::LFA> fa_theta, const fa::linear::LFA& fa_w, double gamma)
        : control::td::Agent{RSRL_GTD2, std::move(fa_theta), gamma, 1.0, RSRL_TRACE_ACCUMULATE, 0.0, fa_w.lr} {}
};
struct TDC : control::td::Agent {
    TDC(Shared<fa::linear::LFA> q_func, const fa::linear::LFA& td_est, double gamma)
        : control::td::Agent{RSRL_TDC, std::move(q_func), gamma, 1.0, RSRL_TRACE_ACCUMULATE, 0.0, td_est.lr} {}
};
}}  // namespace prediction::td

// ---- rsrl::prediction::mc: GradientMC { v_func, gamma }   (prediction/mc.rs:26-58)
// Every-visit Monte-Carlo prediction through v_func's SGD rate.  Handler<&Trajectory> only: Session::handle(const Trajectory&) walks each learner's
// trajectory last transition to first.  Drive it with policies::Random and a max_episode_steps >= 1 (the device records the open episodes).
namespace prediction { namespace mc {
struct GradientMC : control::td::Agent {
    GradientMC(Shared<fa::linear::LFA> v_func, double gamma) : control::td::Agent{RSRL_GRADIENT_MC, std::move(v_func), gamma} {}
};
}}  // namespace prediction::mc

// ---- rsrl::prediction::lstd: RecursiveLSTD::new(basis, gamma) / iLSTD::new(basis, alpha, gamma, n_updates)   (recursive_lstd.rs, ilstd.rs)
// theta and the F x F matrix are f64 on the device (Session::lstd_state); weights() is theta rounded to f32.  Drive these with policies::Random.
namespace prediction { namespace lstd {
struct RecursiveLSTD : control::td::Agent {
    RecursiveLSTD(const fa::linear::basis::Fourier& basis, double gamma)
        : control::td::Agent{RSRL_RECURSIVE_LSTD, make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.0), 1)), gamma} {}
};
struct iLSTD : control::td::Agent {
    iLSTD(const fa::linear::basis::Fourier& basis, double alpha_, double gamma, int n_updates)
        : control::td::Agent{RSRL_ILSTD, make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.0), 1)), gamma, alpha_} { n_steps = n_updates; }
};
// LSTD::new(basis, gamma) / LSTDLambda::new(basis, gamma, lambda)   (lstd.rs:23-37, lstd_lambda.rs:25-41).  Handler<&Batch> on whole transitions:
// Session::handle(const Batch&) with the batch's `to` and `terminal` filled; Session::solve() is their public solve().  theta, A, b and z are f64
// on the device (Session::lstd_batch_state).  The solve is the library's own elimination: no SVD fallback, a zero pivot keeps theta and counts in
// singular_solves.  Drive these with policies::Random and a max_episode_steps >= 1 (the device records the open episodes)
struct LSTD : control::td::Agent {
    LSTD(const fa::linear::basis::Fourier& basis, double gamma)
        : control::td::Agent{RSRL_LSTD, make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.0), 1)), gamma} {}
};
struct LSTDLambda : control::td::Agent {
    LSTDLambda(const fa::linear::basis::Fourier& basis, double gamma, double lambda_)
        : control::td::Agent{RSRL_LSTD_LAMBDA, make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.0), 1)), gamma, 1.0, RSRL_TRACE_ACCUMULATE, lambda_} {}
};
// LambdaLSPE::new(basis, alpha, gamma, lambda)   (lambda_lspe.rs:28-43).  Driven as LSTDLambda; Session::solve() is the agent's (private) solve() as
// handle ends with it.  Session::lstd_batch_state(env, true): z[0] is the return correction delta and z[1] the learner's row count -- the solve is
// deferred until A holds F rows (include/rsrl_hip.h RSRL_LAMBDA_LSPE, the row rule), then theta <- (1 - alpha) theta + alpha A^-1 b
struct LambdaLSPE : control::td::Agent {
    LambdaLSPE(const fa::linear::basis::Fourier& basis, double alpha_, double gamma, double lambda_)
        : control::td::Agent{RSRL_LAMBDA_LSPE, make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.0), 1)), gamma, alpha_, RSRL_TRACE_ACCUMULATE, lambda_} {}
};
}}  // namespace prediction::lstd
// ---- rsrl::control::cacla: CACLA::new(critic, policy, alpha, gamma) (control/cacla.rs:11-29) with policies::Gaussian on
// domains::ContinuousMountainCar.  critic: the reference's is any Function<(S,)> the agent reads and never writes; here it is the TD learner the
// caller would train beside it -- prediction::td::TD{v_func, gamma}, handled before the agent on every transition (the order of tdac.rs and nac.rs;
// the reference has no example for CACLA).  gamma must be the critic's: the library runs both with one.  The Session's weights are V's [F][1];
// Session::handle(TransitionF32) is eval.handle then agent.handle.  The rule is the reference's, literally: the mean's step is
// alpha (a - mu)^2 / Sigma >= 0 on either side of the mean (include/rsrl_hip.h, RSRL_CACLA)
namespace control { namespace cacla {
struct CACLA : td::Agent {
    CACLA(const prediction::td::TD& critic, const policies::Gaussian& /*policy*/, double alpha_, double gamma_)
        : td::Agent{RSRL_CACLA, critic.q_func, gamma_, alpha_} {
        if (gamma_ != critic.gamma) throw Error(RSRL_HIP_EINVAL, "CACLA over a TD critic: the library runs CACLA and TD with one gamma");
    }
};
}}  // namespace control::cacla

inline control::ac::ActorCritic control::ac::ActorCritic::tdac(const prediction::lstd::iLSTD& eval, const policies::Gibbs& policy, double alpha_, double gamma) {
    if (gamma != eval.gamma) throw Error(RSRL_HIP_EINVAL, "ActorCritic::tdac over iLSTD: the library runs TDCritic and iLSTD with one gamma");
    fa::linear::LFA v = *eval.q_func;
    v.lr = eval.alpha;                                            // the critic's rate travels as config.lr, ActorCritic.alpha as config.alpha
    ActorCritic a(TDCritic{gamma, make_shared(v)}, policy, alpha_);
    a.algo = RSRL_ILSTD_ACTOR_CRITIC; a.n_steps = eval.n_steps;
    return a;
}

inline control::ac::ActorCritic control::ac::ActorCritic::tdac(const prediction::lstd::iLSTD& eval, const policies::Beta&, double alpha_, double gamma) {
    return tdac(eval, policies::Gibbs::standard(eval.q_func), alpha_, gamma);      // (the Session's policy decides the kind)
}

inline control::ac::ActorCritic control::ac::ActorCritic::tdac_cont(const prediction::td::TD& eval, double alpha_, double gamma) {
    if (gamma != eval.gamma) throw Error(RSRL_HIP_EINVAL, "ActorCritic::tdac over TD: the library runs TDCritic and TD with one gamma");
    ActorCritic a(TDCritic{gamma, eval.q_func}, policies::Gibbs::standard(eval.q_func), alpha_);      // (the Session's policy decides the kind)
    a.algo = RSRL_CONTINUOUS_TD_ACTOR_CRITIC;
    return a;
}
inline control::ac::ActorCritic control::ac::ActorCritic::tdac(const prediction::td::TD& eval, const policies::Gaussian&, double alpha_, double gamma) {
    return tdac_cont(eval, alpha_, gamma);
}
inline control::ac::ActorCritic control::ac::ActorCritic::tdac(const prediction::td::TD& eval, const policies::Beta&, double alpha_, double gamma) {
    return tdac_cont(eval, alpha_, gamma);
}

// ---- the bound object graph: env + agent + policy sharing one q_func on one MI355X -------------------
class Session {
public:
    Session(const domains::Domain& env, const control::td::Agent& agent, const policies::Policy& policy,
            uint64_t seed = 0, uint32_t max_episode_steps = 0, int device = 0, int64_t env_offset = 0) {
        rsrl_hip_config cfg;
        check(rsrl_hip_config_init(&cfg));
        cfg.device = device; cfg.domain = env.kind; cfg.n_envs = env.n_envs; cfg.env_offset = env_offset;
        const fa::linear::LFA& q = *agent.q_func;
        cfg.basis = q.basis_kind; cfg.order = q.order; cfg.n_tilings = q.n_tilings; cfg.tiles_per_dim = q.tiles_per_dim;
        cfg.lr = q.lr; cfg.weight_mode = q.shared_weights ? RSRL_W_SHARED : RSRL_W_PER_ENV;
        cfg.algo = agent.algo; cfg.gamma = agent.gamma; cfg.alpha = agent.alpha;
        cfg.trace = agent.trace; cfg.lambda = agent.lambda; cfg.lr_td = agent.lr_td;
        cfg.policy = policy.kind; cfg.epsilon = policy.epsilon; cfg.tau = policy.tau;
        cfg.epsilon_decay = policy.epsilon_decay; cfg.epsilon_min = policy.epsilon_min;
        // an agent-owned policy equal to the behaviour policy IS the shared object of the reference's examples
        if (agent.owns_policy && (agent.policy.kind != policy.kind || agent.policy.epsilon != policy.epsilon || agent.policy.tau != policy.tau)) {
            cfg.agent_policy = agent.policy.kind; cfg.agent_epsilon = agent.policy.epsilon; cfg.agent_tau = agent.policy.tau;
        }
        cfg.sigma = agent.sigma; cfg.n_steps = agent.n_steps;
        cfg.seed = seed; cfg.max_episode_steps = max_episode_steps;
        check(rsrl_hip_create(&cfg, &ctx_));
        D_ = rsrl_hip_state_dim(ctx_); A_ = rsrl_hip_n_actions(ctx_); F_ = rsrl_hip_n_features(ctx_); N_ = env.n_envs;
        O_ = rsrl_hip_n_outputs(ctx_); P_ = rsrl_hip_n_policy_outputs(ctx_); R_ = rsrl_hip_n_weight_rows(ctx_);
        Q_ = agent.algo == RSRL_GIBBS_NAC ? A_ : O_;
    }
    ~Session() { rsrl_hip_destroy(ctx_); }
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;

    int state_dim() const { return D_; }
    int n_actions() const { return A_; }              // env.action_space().card()
    int n_features() const { return F_; }
    int64_t n_envs() const { return N_; }

    // per-episode `Domain::default()` + `policy.sample(rng, env.emit().state())`   (q_learning.rs:37-38)
    void reset() { check(rsrl_hip_reset(ctx_)); }
    // Domain::emit().state()
    std::vector<float> emit() { std::vector<float> s((size_t)D_ * N_); check(rsrl_hip_get_states(ctx_, s.data())); return s; }
    // Domain::transition(a)                                                       (lib.rs:436-446)
    domains::Transition transition(const std::vector<int32_t>& a) {
        domains::Transition t;
        t.from.resize((size_t)D_ * N_); t.to.resize((size_t)D_ * N_); t.reward.resize(N_); t.terminal.resize(N_);
        t.action = a;
        check(rsrl_hip_domain_step(ctx_, a.data(), t.from.data(), t.to.data(), t.reward.data(), t.terminal.data()));
        return t;
    }
    // Handler<&Transition>::handle -> Response.error                              (q_learning.rs:51-71)
    std::vector<float> handle(const domains::Transition& t) {
        std::vector<float> td(N_);
        check(rsrl_hip_handle(ctx_, t.from.data(), t.action.data(), t.reward.data(), t.to.data(), t.terminal.data(), N_, td.data()));
        return td;
    }
    // ... with f32 actions, a continuous domain's (ContinuousMountainCar): Domain::transition, Handler<&Transition>::handle, Policy::sample / mode,
    // Beta's compute_alpha / compute_beta
    struct TransitionF32 { std::vector<float> from, action, reward, to; std::vector<uint8_t> terminal; };
    TransitionF32 transition_f32(const std::vector<float>& a) {
        TransitionF32 t;
        t.from.resize((size_t)D_ * N_); t.to.resize((size_t)D_ * N_); t.reward.resize(N_); t.terminal.resize(N_);
        t.action = a;
        check(rsrl_hip_domain_step_f32(ctx_, a.data(), t.from.data(), t.to.data(), t.reward.data(), t.terminal.data()));
        return t;
    }
    std::vector<float> handle(const TransitionF32& t) {
        std::vector<float> td(N_);
        check(rsrl_hip_handle_f32(ctx_, t.from.data(), t.action.data(), t.reward.data(), t.to.data(), t.terminal.data(), N_, td.data()));
        return td;
    }
    std::vector<float> sample_f32() { std::vector<float> a(N_); check(rsrl_hip_policy_sample_f32(ctx_, nullptr, N_, a.data())); return a; }
    std::vector<float> sample_f32(const std::vector<float>& states) {
        std::vector<float> a(N_); check(rsrl_hip_policy_sample_f32(ctx_, states.data(), N_, a.data())); return a;
    }
    std::vector<float> mode_f32(const std::vector<float>& states) {
        std::vector<float> a(N_); check(rsrl_hip_policy_mode_f32(ctx_, states.data(), N_, a.data())); return a;
    }
    std::pair<std::vector<float>, std::vector<float>> policy_params(const std::vector<float>& states) {
        std::vector<float> a(N_), b(N_); check(rsrl_hip_policy_params(ctx_, states.data(), N_, a.data(), b.data())); return {a, b};
    }
    // control::nac::NAC: agent.handle(()) for every learner -> Response.norm; the critic's Function<(S, A)>::evaluate, Q(s_i, a_i) of learner i
    std::vector<float> nac_update() { std::vector<float> n(N_); check(rsrl_hip_nac_update(ctx_, nullptr, n.data())); return n; }
    std::vector<float> q_evaluate(const std::vector<float>& states, const std::vector<float>& actions) {
        std::vector<float> q(N_); check(rsrl_hip_q_evaluate_f32(ctx_, states.data(), actions.data(), N_, q.data())); return q;
    }
    // Domain::rollout(|s| policy.mode(s), Some(limit)).total_reward() for every learner (NAC with Beta: the loop's |s| 2 * policy.mode(s) - 1)
    std::vector<float> rollout_total_reward(int64_t step_limit) {
        std::vector<uint32_t> n(N_); std::vector<float> tot(N_); check(rsrl_hip_rollout_greedy(ctx_, step_limit, n.data(), tot.data())); return tot;
    }
    // Handler<&Batch>::handle of REINFORCE / BaselineREINFORCE -> the running return at each handled transition, [T][N] (reinforce.rs)
    // ... and of LSTD / LSTDLambda, which read whole transitions (b.to and b.terminal filled; lstd.rs:59-81, lstd_lambda.rs:66-103) -> the
    // diagnostic r + gamma V(s') - V(s) at each handled transition, [T][N]
    std::vector<float> handle(const domains::Batch& b) {
        std::vector<float> g((size_t)b.T * N_);
        if (!b.to.empty() || !b.terminal.empty()) {
            check(rsrl_hip_handle_transitions(ctx_, b.T, b.states.data(), b.actions.empty() ? nullptr : b.actions.data(), b.rewards.data(), b.to.data(),
                                              b.terminal.data(), b.lengths.data(), b.T > 0 ? g.data() : nullptr));
            return g;
        }
        check(rsrl_hip_handle_batch(ctx_, b.T, b.states.data(), b.actions.data(), b.rewards.data(), b.lengths.data(), g.data()));
        return g;
    }
    // Handler<&Trajectory>::handle of GradientMC -> the backward sum at each handled transition, [T][N] with T = the trajectory's rows of rewards
    // (mc.rs:40-57).  Transition k's `from` is states row k (`start`, then steps[k-1].0) and its reward rewards row k; learner i has n_states[i] - 1
    std::vector<float> handle(const domains::Trajectory& tr) {
        const int64_t T = (int64_t)(tr.rewards.size() / (size_t)N_);
        std::vector<uint32_t> len((size_t)N_);
        for (int64_t i = 0; i < N_; ++i) len[(size_t)i] = tr.n_states[(size_t)i] > 0 ? tr.n_states[(size_t)i] - 1 : 0;
        std::vector<float> g((size_t)T * N_);
        check(rsrl_hip_handle_batch(ctx_, T, tr.states.data(), nullptr, tr.rewards.data(), len.data(), T > 0 ? g.data() : nullptr));
        return g;
    }
    // policy.sample(rng, env.emit().state()): the driver loop's behaviour sample for the session's own envs (the actions become the pending ones)
    std::vector<int32_t> sample() {
        std::vector<int32_t> a(N_); check(rsrl_hip_policy_sample(ctx_, nullptr, N_, a.data())); return a;
    }
    // Policy::sample / Policy::mode                                               (policies/mod.rs:65-78)
    std::vector<int32_t> sample(const std::vector<float>& states) {
        std::vector<int32_t> a(N_); check(rsrl_hip_policy_sample(ctx_, states.data(), N_, a.data())); return a;
    }
    std::vector<int32_t> mode(const std::vector<float>& states) {
        std::vector<int32_t> a(N_); check(rsrl_hip_policy_mode(ctx_, states.data(), N_, a.data())); return a;
    }
    // Function<(S,)>::evaluate                                                    (fa/linear.rs:303-311)
    std::vector<float> evaluate(const std::vector<float>& states) {
        std::vector<float> q((size_t)Q_ * N_); check(rsrl_hip_q_evaluate(ctx_, states.data(), N_, q.data())); return q;
    }
    // Enumerable::find_max / find_min -> (index, value), ties -> last index        (core.rs:86-105)
    std::pair<std::vector<int32_t>, std::vector<float>> find_max(const std::vector<float>& states) {
        std::vector<int32_t> i(N_); std::vector<float> v(N_); check(rsrl_hip_q_find_max(ctx_, states.data(), N_, i.data(), v.data())); return {i, v};
    }
    std::pair<std::vector<int32_t>, std::vector<float>> find_min(const std::vector<float>& states) {
        std::vector<int32_t> i(N_); std::vector<float> v(N_); check(rsrl_hip_q_find_min(ctx_, states.data(), N_, i.data(), v.data())); return {i, v};
    }
    // Enumerable::expected_value(args, ps)                                        (core.rs:107-116); ps is [A][N]
    std::vector<float> expected_value(const std::vector<float>& states, const std::vector<float>& ps) {
        std::vector<float> e(N_); check(rsrl_hip_q_expected_value(ctx_, states.data(), N_, ps.data(), e.data())); return e;
    }
    // Function<(S,)> / Function<(S, A)> of the policy                              (greedy.rs:30-60, epsilon_greedy.rs:38-63)
    std::vector<float> policy_probs(const std::vector<float>& states) {
        std::vector<float> p((size_t)A_ * N_); check(rsrl_hip_policy_probs(ctx_, states.data(), N_, p.data())); return p;
    }
    std::vector<float> policy_prob(const std::vector<float>& states, const std::vector<int32_t>& actions) {
        std::vector<float> p(N_); check(rsrl_hip_policy_prob(ctx_, states.data(), actions.data(), N_, p.data())); return p;
    }
    void set_epsilon(double eps) { check(rsrl_hip_set_epsilon(ctx_, eps)); }      // pub field EpsilonGreedy.epsilon
    std::vector<float> epsilons() { std::vector<float> e(N_); check(rsrl_hip_get_epsilons(ctx_, e.data())); return e; }   // ... of every learner
    // Parameterised::weights()                                                    (params/mod.rs:118)
    std::vector<float> weights(int64_t env = 0) {
        std::vector<float> w((size_t)R_ * O_); check(rsrl_hip_get_weights(ctx_, env, w.data())); return w;
    }
    // the pub field `trace` of SARSALambda / QLambda                                (sarsa_lambda.rs:41)
    std::vector<float> trace(int64_t env = 0) {
        std::vector<float> z((size_t)F_ * O_); check(rsrl_hip_get_traces(ctx_, env, z.data())); return z;
    }
    // the pub field `fa_td` of GreedyGQ (greedy_gq.rs:52), [F][A]; `fa_w` of GTD2 / `td_est` of TDC (gtd2.rs:29, tdc.rs:43), [F][1]
    std::vector<float> td_weights(int64_t env = 0) {
        std::vector<float> v((size_t)F_ * O_); check(rsrl_hip_get_td_weights(ctx_, env, v.data())); return v;
    }
    // RecursiveLSTD / iLSTD (and ActorCritic::tdac over iLSTD): one learner's exact f64 state -- theta [F], the matrix [F][F] (C / A, row-major), iLSTD's mu [F] (empty otherwise)
    struct LstdState { std::vector<double> theta, mat, mu; };
    LstdState lstd_state(int64_t env = 0, bool with_mu = false) {
        LstdState st{std::vector<double>((size_t)F_), std::vector<double>((size_t)F_ * F_), std::vector<double>(with_mu ? (size_t)F_ : 0)};
        check(rsrl_hip_get_lstd_state(ctx_, env, st.theta.data(), st.mat.data(), with_mu ? st.mu.data() : nullptr));
        return st;
    }
    // LSTD / LSTDLambda: solve() (lstd.rs:40, lstd_lambda.rs:44) for every learner, and one learner's exact f64 state -- theta [F], A [F][F]
    // (row-major), b [F], LSTDLambda's z [F] (empty otherwise) and its count of abandoned solves
    void solve() { check(rsrl_hip_lstd_solve(ctx_)); }
    struct LstdBatchState { std::vector<double> theta, A, b, z; uint32_t singular_solves = 0; };
    LstdBatchState lstd_batch_state(int64_t env = 0, bool with_z = false) {
        LstdBatchState st{std::vector<double>((size_t)F_), std::vector<double>((size_t)F_ * F_), std::vector<double>((size_t)F_),
                          std::vector<double>(with_z ? (size_t)F_ : 0)};
        check(rsrl_hip_get_lstd_batch_state(ctx_, env, st.theta.data(), st.A.data(), st.b.data(), with_z ? st.z.data() : nullptr, &st.singular_solves));
        return st;
    }
    // the pub field `policy` of ActorCritic: the Gibbs actor's weights               (ac.rs:61)
    std::vector<float> policy_weights(int64_t env = 0) {
        std::vector<float> v((size_t)F_ * (P_ ? P_ : A_)); check(rsrl_hip_get_policy_weights(ctx_, env, v.data())); return v;
    }
    // serde analogue: checkpoint of every learner's approximator(s)                  (rsrl/Cargo.toml:26)
    void save_weights(const std::string& path) { check(rsrl_hip_save_weights(ctx_, path.c_str())); }
    void load_weights(const std::string& path) { check(rsrl_hip_load_weights(ctx_, path.c_str())); }
    // the fused driver loop: n_steps of {transition, handle, sample} for every env, auto-reset
    rsrl_hip_stats train(int64_t n_steps) { rsrl_hip_stats st; check(rsrl_hip_train(ctx_, n_steps, &st)); return st; }
    // Domain::rollout(|s| policy.mode(s), Some(limit)).n_states()                 (lib.rs:448-479, :340)
    std::vector<uint32_t> rollout_n_states(int64_t step_limit) {
        std::vector<uint32_t> n(N_); check(rsrl_hip_rollout_greedy(ctx_, step_limit, n.data(), nullptr)); return n;
    }
    // Domain::rollout(..) as the Trajectory it returns                             (lib.rs:334-409, 448-479)
    domains::Trajectory rollout(int64_t step_limit) {
        domains::Trajectory tr;
        tr.n_states.resize(N_); tr.total_reward.resize(N_); tr.terminal.resize(N_);
        tr.states.assign((size_t)step_limit * D_ * N_, 0.0f);
        tr.actions.assign((size_t)(step_limit - 1) * N_, 0); tr.rewards.assign((size_t)(step_limit - 1) * N_, 0.0f);
        check(rsrl_hip_rollout_trajectory(ctx_, step_limit, N_, tr.n_states.data(), tr.total_reward.data(), tr.states.data(),
                                          step_limit > 1 ? tr.actions.data() : nullptr, step_limit > 1 ? tr.rewards.data() : nullptr, tr.terminal.data()));
        return tr;
    }
    // Domain::rollout(|s| policy.sample(rng, s), Some(limit)) for any policy over this session's Q function   (lib.rs:448-479)
    domains::Trajectory rollout(const policies::Policy& pi, int64_t step_limit) {
        domains::Trajectory tr;
        tr.n_states.resize(N_); tr.total_reward.resize(N_); tr.terminal.resize(N_);
        tr.states.assign((size_t)step_limit * D_ * N_, 0.0f);
        tr.actions.assign((size_t)(step_limit - 1) * N_, 0); tr.rewards.assign((size_t)(step_limit - 1) * N_, 0.0f);
        check(rsrl_hip_rollout_policy(ctx_, pi.kind, pi.epsilon, pi.tau, step_limit, N_, tr.n_states.data(), tr.total_reward.data(), tr.states.data(),
                                      step_limit > 1 ? tr.actions.data() : nullptr, step_limit > 1 ? tr.rewards.data() : nullptr, tr.terminal.data()));
        return tr;
    }
    rsrl_hip_ctx* raw() { return ctx_; }

private:
    rsrl_hip_ctx* ctx_ = nullptr;
    int D_ = 0, A_ = 0, F_ = 0, O_ = 0, P_ = 0, R_ = 0;      // O_: weight columns (A_, or 1 for the prediction agents); P_: the policy's own (A_, or Beta's 2); R_: weight rows (F_, or NAC's 3 F_)
    int Q_ = 0;                                              // rows of evaluate(): O_, or A_ for NAC over the Gibbs policy (one weight column, a value per action)
    int64_t N_ = 0;
};

}  // namespace rsrl
