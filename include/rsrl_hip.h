/*
 * rsrl_hip.h -- C ABI of librsrl_hip.so: the MI355X (gfx950) implementation of
 * tspooner/rsrl's per-step TD-control hot path
 *
 *     env.transition(a) -> agent.handle(&t) -> policy.sample(s')
 *                                   (rsrl/examples/q_learning.rs:34-55)
 *
 * vectorised over N independent environments.  The reference has no FFI of its
 * own: its extension surface is Rust traits (Domain / Function / Enumerable /
 * Handler / Policy / Parameterised).  Every entry point below stands in for one
 * trait method on the path and cites it (paths relative to the reference
 * repository).  INTEGRATION.md shows the Rust `extern "C"` block and the trait
 * impls a maintainer would write on top of it.
 *
 * Conventions
 *   - every function returns rsrl_hip_status (0 = OK, <0 = error); the message of
 *     the last error on the calling thread is rsrl_hip_last_error().
 *   - a ctx is NOT thread-safe (mirrors `&mut self` + Rc<RefCell>, core.rs:13-15);
 *     distinct ctxs may be used from distinct threads.
 *   - batched arrays are SoA, component-major: states f32[D][M], Q f32[A][M];
 *     actions int32[M]; terminal flags uint8[M]; rewards / td errors f32[M].
 *     A batch of M items addresses learners 0..M-1 of the ctx (M <= n_envs).
 *   - array arguments may be HOST or DEVICE pointers (detected per call with
 *     hipPointerGetAttributes); device pointers are used in place, host pointers
 *     are staged through ctx-owned device buffers.  Nothing is freed by the
 *     other side.
 *   - all kernels of a ctx run on ONE HIP stream (the caller's, if given in the
 *     config, else a ctx-owned one).  Calls taking host output pointers return
 *     after the data has landed; calls with device pointers are asynchronous on
 *     that stream (use rsrl_hip_sync).  On a CALLER-supplied stream every call has
 *     enqueued all of its work when it returns: hipStreamSynchronize / an event on
 *     that stream orders the caller's own work after it (launch coalescing, below,
 *     is for ctx-owned streams only).
 *   - there is no CPU fallback: without a usable HIP device rsrl_hip_create fails.
 */
#ifndef RSRL_HIP_H
#define RSRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSRL_HIP_ABI_VERSION 9

typedef enum {
    RSRL_HIP_OK      = 0,
    RSRL_HIP_EINVAL  = -1,   /* bad argument / unsupported combination              */
    RSRL_HIP_EHIP    = -2,   /* HIP runtime error (incl. no device)                  */
    RSRL_HIP_ENOMEM  = -3,   /* allocation failed                                    */
    RSRL_HIP_ERCCL   = -4,   /* RCCL error                                           */
    RSRL_HIP_ESTATE  = -5    /* call not valid in the ctx's current state            */
} rsrl_hip_status;

/* rsrl_domains::{MountainCar, CartPole, Acrobot, HIVTreatment}
 *   mountain_car/discrete.rs:8-102, cart_pole.rs:7-121, acrobot.rs:8-152, hiv.rs:1-146 (exported at lib.rs:498-499)
 * HIVTreatment: a hidden state [T1, T1*, T2, T2*, V, E] in f64 (hiv.rs:42-52) that every env-step integrates with 1 000 classical RK4
 *   sub-steps (:54-71, ode.rs:1-43) in the reference's operation order -- the same bits as the reference; the env state the API carries
 *   (D = 6) is its observation clip(-5, log10 y, 8) (:112-119) rounded to f32, the reward is taken from the observation in f64 (:121-135);
 *   4 actions (:35), no terminal state (episodes end at max_episode_steps only).  Supported: QLearning, SARSA, ExpectedSARSA, PAL on the
 *   Fourier basis of order 1-3, per-learner f32 weights, no epsilon schedule; every other combination is EINVAL at create.  The hidden
 *   state: rsrl_hip_get_hidden_states / _set_hidden_states.
 * ContinuousMountainCar (mountain_car/continuous.rs): MountainCar's state bounds and start state (-0.5, 0) -- the Fourier features of a state are
 *   MountainCar's at the same order -- with ONE f32 action in [-1, 1] instead of an index:  a' = clip(-1, a, 1) (the reference's
 *   action_space.map_onto, from the `spaces` crate that is not in the reference tree: recalled as a clip);
 *   v = clip(-0.07, v + 0.0015 a' - 0.0025 cos(3x), 0.07); x = clip(-1.2, x + v, 0.6); terminal iff x >= 0.6; reward 0 on a terminal step, -1
 *   otherwise.  The action set is not enumerable: rsrl_hip_n_actions is 0, rsrl_hip_action_bounds gives (-1, 1), and every action of the ctx is
 *   f32 (the *_f32 entry points below; their int32 twins are ESTATE, as the *_f32 calls are on the other domains).  Supported:
 *   RSRL_ILSTD_ACTOR_CRITIC, RSRL_NAC and RSRL_CONTINUOUS_TD_ACTOR_CRITIC with policy RSRL_BETA, and RSRL_NAC, RSRL_CACLA and
 *   RSRL_CONTINUOUS_TD_ACTOR_CRITIC with policy RSRL_GAUSSIAN, on the Fourier orders 1-5;
 *   every other combination is EINVAL at create.
 * CliffWalk (cliff_walk.rs:9-75 over grid_world.rs:87-125): CliffWalk::default() = CliffWalk::new(5, 12), height 5, width 12.  The state is
 *   loc = [x, y] (D = 2), carried as two f32 that hold the exact integers x in 0..11 and y in 0..4 (rsrl_hip_state_bounds: (0, 11) and (0, 4)), the
 *   start state [0, 0]; 4 actions, ALL_ACTIONS: 0 North (y <- min(y + 1, 4)), 1 East (x <- min(x + 1, 11)), 2 South (y <- max(y - 1, 0)), 3 West
 *   (x <- max(x - 1, 0)); terminal iff x > 0 && y == 0 on the new location (cliff_walk.rs:41-47); reward +50 on a terminal step with x == 11, -50 on
 *   any other terminal step, 0 otherwise (:49-62).  A state component a caller hands in (set_states, handle's from / to, the query calls) is read as
 *   floor(clamp(s, 0, size - 1)), NaN as 0.  Supported: QLearning, SARSA, ExpectedSARSA, PAL with basis RSRL_TABLE, per-learner f32 tables, no epsilon
 *   schedule; every other combination that names the domain or the basis is EINVAL at create. */
typedef enum { RSRL_MOUNTAIN_CAR = 0, RSRL_CART_POLE = 1, RSRL_ACROBOT = 2, RSRL_HIV_TREATMENT = 3, RSRL_CONTINUOUS_MOUNTAIN_CAR = 4,
               RSRL_CLIFF_WALK = 5 } rsrl_domain;
/* lfa::basis::{Fourier (+with_bias), TileCoding}  (re-exported by rsrl/src/fa/linear.rs:11-14)
 * RSRL_TABLE: the tabular function approximator, rsrl/src/fa/tabular/dense.rs, Table<Array2<f64>> -- with RSRL_CLIFF_WALK only, and CliffWalk with it
 *   only.  F = 60 rows and 4 columns, zero-initialised (Table::zeros); Q(s, .) is the row of s (dense.rs:79-83), the update Q[row, a] += error
 *   (:118-127).  The reference gives no map from the domain's [usize; 2] to the usize Table is indexed by: here row = x * 5 + y, first component
 *   major (as the Fourier coefficient order).  Table has no optimiser, so the reference's agents step with size 1; config.lr scales the error (as
 *   for GTD2 / TDC), and at lr = 1 -- an exact multiplication -- the rule is the reference's literal one.  rsrl_hip_get/set_weights carry the
 *   (60, 4) matrix row-major; order, n_tilings and tiles_per_dim are not read. */
typedef enum { RSRL_FOURIER = 0, RSRL_TILE_CODING = 1, RSRL_TABLE = 2 } rsrl_basis;
/* rsrl::control::td::{QLearning, SARSA, ExpectedSARSA}
 *   q_learning.rs:35-71, sarsa.rs:35-75, expected_sarsa.rs:22-66
 * the eligibility-trace agents {SARSALambda, QLambda}
 *   sarsa_lambda.rs:37-98, q_lambda.rs:37-99 (per-learner weights; register-family Fourier bases, every other Fourier order (round 5: W and
 *   the trace in memory, one thread per learner, rsrl_amd/csrc/kernels_lambda_mem.hpp), the order-7 Fourier bases of
 *   the 4-D domains with f32 weights (W and the trace streamed from memory every step), or tile coding with one dense trace
 *   table of W's shape per learner -- the reference's traces are generic over the gradient buffer, traces.rs:6-12;
 *   round 5: weight_mode = RSRL_W_SHARED on tile coding -- ONE shared table, every learner its own SPARSE trace as params/sparse.rs:13-97
 *   offers: at most 512 (entry, value) pairs, kept as one sub-list of 512 / n_tilings per tiling (n_tilings 4, 8 or 16; a tiling's slice of the
 *   table, cells * actions, at most 65 536 entries), the entry with the smallest |value| of a full sub-list making room; the table moves by the
 *   synchronous mini-batch rule W += sum_i alpha * residual_i * z_i in exact 64-bit fixed point.  Stepped by rsrl_hip_train, or by
 *   rsrl_hip_handle with transition i taken as LEARNER i's (its trace is the one that moves; M <= n_envs: ABI unchanged, round 6);
 *   rsrl_hip_get_traces shows a learner's list as the dense (F, A) matrix it stands for; the lists travel with a checkpoint, file version 6)
 * PAL (persistent advantage learning), pal.rs:18-60 -- a drop-in sibling of QLearning (uses `alpha`)
 * and GreedyGQ, greedy_gq.rs:49-142 -- fa_q (SGD(lr)) plus a second approximator fa_td (SGD(lr_td), weights through
 *   rsrl_hip_get/set_td_weights); per-learner weights: register-family Fourier bases, the generic Fourier orders, tile coding, and (round 5)
 *   the order-7 wave family (one wavefront per learner, W and V streamed: kernels_wave_aux.hpp; round 6: W as bf16 with stochastic rounding too -- for every agent of
 *   that family: the trace / fa_td's weights / QSigma's backups stay f32) */
typedef enum { RSRL_QLEARNING = 0, RSRL_SARSA = 1, RSRL_EXPECTED_SARSA = 2, RSRL_SARSA_LAMBDA = 3, RSRL_Q_LAMBDA = 4,
               RSRL_PAL = 5, RSRL_GREEDY_GQ = 6,
               /* prediction (state-value function on a ScalarLFA, ONE weight column; behaviour policy RSRL_RANDOM):
                *   TD prediction/td/td.rs:25-59 (SGD(lr)), TDLambda prediction/td/td_lambda.rs:25-78 (step = the TD error);
                *   per-learner weights: register-family Fourier bases (fused, register-resident), the other Fourier orders (one thread
                *   per learner, w and z in memory), tile coding (one block per learner) or (round 5) the order-7 wave family (f32 weights; bf16 since round 6)
                *   (one wavefront per learner, w and z streamed: kernels_wave_aux.hpp) */
               RSRL_TD = 7, RSRL_TD_LAMBDA = 8,
               /* QSigma, the n-step Q(sigma) agent (control/td/q_sigma.rs:80-202; config.sigma, config.n_steps, alpha, gamma, and the
                * agent's own policy).  The reference panics at its first full backup -- Backup::propagate reads entries[n_steps]
                * (q_sigma.rs:52-53 vs :113-114) -- so the library implements it with that one dead out-of-bounds read removed
                * (rsrl_amd/csrc/kernels_qsigma.hpp).  Per-learner f32 weights on every basis: register-family and generic Fourier orders, tile
                * coding, and (round 5) the order-7 wave family (one wavefront per learner, kernels_wave_aux.hpp k_wave_qsigma). */
               RSRL_Q_SIGMA = 9,
               /* ActorCritic (control/ac.rs:49-115) with a Gibbs actor, policy = Gibbs::standard(LFA::vector(basis, SGD(1.0), A)) (softmax.rs:113-130,
                * :154-163, :216-222), and the SARSA critic of examples/a2c.rs:22-67: SARSA{q_func = LFA::vector(basis, SGD(lr), A), policy, gamma}
                * (sarsa.rs:43-73) handles each transition first -- its inner draw na ~ pi_theta(s') -- then the actor moves by
                * theta[:,b] += alpha * c * (1[b==a] - p_b) * phi(s), p = softmax(theta^T phi(s) / tau) before the update (grad_log does not divide by tau,
                * kept literally), c the critic's target with the UPDATED q_func:
                *   RSRL_ACTOR_CRITIC     a2c.rs's closure (:38-49): c = Q(s,a) - sum_b Q(s,b) p_b
                *   RSRL_Q_ACTOR_CRITIC   ActorCritic::qac, QCritic (ac.rs:23-31, :77-84): c = Q(s,a)
                * config: lr = the critic's SGD rate, alpha = ActorCritic.alpha, gamma = SARSA.gamma, tau = Softmax.tau; policy must be RSRL_SOFTMAX and
                * agent_policy -1 (the critic shares the actor).  Both matrices start at zero (LFA::vector).  The POLICY side of the ABI reads the actor's
                * preferences theta^T phi(s) (policy_sample / _mode / _probs / _prob, reset's initial sample, the rollouts); the VALUE side reads the critic
                * (q_evaluate, q_find_max / _min, q_expected_value, get / set_weights).  theta: rsrl_hip_get/set_policy_weights.  rsrl_hip_handle's
                * td_error_out and the statistics' sum |delta| are the critic's.  Supported: per-learner f32 weights on the register-family Fourier orders
                * (MountainCar 1-5, CartPole 1, Acrobot 1), no epsilon schedule; everything else is EINVAL at create (kernels_ac.hpp) */
               RSRL_ACTOR_CRITIC = 10, RSRL_Q_ACTOR_CRITIC = 11,
               /* (12 is no algo.)  ActorCritic::tdac (ac.rs:32-52, :87-98): the same Gibbs actor with TDCritic over a state-value function V, the loop of
                * examples/tdac.rs with the project's TD(0) prediction agent as its `eval` (TD{v_func = ScalarLFA(basis, SGD(lr)), gamma},
                * prediction/td/td.rs:31-59; tdac.rs's own evaluator is iLSTD: RSRL_ILSTD_ACTOR_CRITIC).  Per transition (s, a, r, s', term), p = softmax(theta^T phi(s) / tau) before the update:
                *   TD(0)   delta = r - V(s) (terminal) | r + gamma*V(s') - V(s);   w += lr*delta*phi(s)        (bit for bit a RSRL_TD ctx's w and delta)
                *   critic  c = r - V'(s') (terminal: V of the terminal state s' itself) | r + gamma*V'(s') - V'(s), V' with the UPDATED w
                *   actor   theta[:,b] += alpha * c * (1[b==a] - p_b) * phi(s)
                * No inner draw.  config: lr = V's SGD rate, gamma = TD's and TDCritic's, alpha = ActorCritic.alpha, tau = Softmax.tau; policy must be
                * RSRL_SOFTMAX and agent_policy -1.  Both start at zero.  The VALUE side is V, as for the prediction agents: q_evaluate writes f32[1][M],
                * get / set_weights are [F][1], n_outputs is 1, q_find_max / _min / q_expected_value are ESTATE.  The POLICY side reads theta [F][A]
                * (policy_sample / _mode / _probs / _prob, reset's initial sample, the rollouts; rsrl_hip_get/set_policy_weights).  rsrl_hip_handle's
                * td_error_out and the statistics' sum |delta| are TD(0)'s delta.  Supported: as RSRL_ACTOR_CRITIC; everything else is EINVAL at create
                * (kernels_tdac.hpp) */
               RSRL_TD_ACTOR_CRITIC = 13,
               /* (14 is no algo.)  REINFORCE<Gibbs> (control/mc/reinforce.rs) and BaselineREINFORCE<B, Gibbs> (control/mc/baseline_reinforce.rs): Handler<&Batch>::handle
                * walks the batch FORWARD and applies each transition's update in order, with theta as it stands after the previous one:
                *   g = r + gamma * g  (0 before the first transition: the discounted sum of the rewards seen so far, NOT the return-to-go -- literal)
                *   e = alpha * g  |  BaselineREINFORCE: alpha * (g - <B[:,a], phi(s)>)      p = softmax(theta^T phi(s) / tau)
                *   theta[:,b] += e * (1[b==a] - p_b) * phi(s)                                (grad_log without 1/tau, as RSRL_ACTOR_CRITIC)
                * The driver loop samples each episode from theta as it stood when the episode began (Trajectory::into_batch) and applies the updates
                * online, which gives the bits of handling the episode's batch at its end: per learner it carries theta, the behaviour snapshot theta_b
                * and the open episode's running return g; an episode's end (terminal or max_episode_steps) sets theta_b <- theta, g <- 0, as do
                * rsrl_hip_reset and rsrl_hip_domain_reset for the learners they restart.  config: alpha, gamma, tau (lr is unused); policy must be
                * RSRL_SOFTMAX and agent_policy -1.  theta starts at zero.  The POLICY side reads theta (policy_sample / _mode / _probs / _prob, reset's
                * initial sample, the rollouts; rsrl_hip_get/set_policy_weights).  BaselineREINFORCE's baseline B (a VectorLFA, read-only) is the ctx's
                * weights: get / set_weights and the Q operations read it.  REINFORCE has no value function: those are ESTATE.  rsrl_hip_handle is ESTATE
                * (there is no Handler<&Transition>): rsrl_hip_handle_batch.  The statistics' sum |delta| is sum |g|.  Supported: as RSRL_ACTOR_CRITIC;
                * everything else is EINVAL at create (kernels_reinforce.hpp) */
               RSRL_REINFORCE = 15, RSRL_BASELINE_REINFORCE = 16,
               /* (17 is no algo.)  Least-squares prediction, Handler<&Transition> (prediction/lstd/recursive_lstd.rs, prediction/lstd/ilstd.rs): a
                * state-value function V(s) = phi(s) . theta with f64 theta and a f64 F x F matrix per learner; the Fourier features are evaluated in
                * f64 on the device.  pd = phi(s) - gamma * phi(s'); every product is rounded, dot products are summed in index order.
                *   RecursiveLSTD::new(basis, gamma): theta = 0, C = 1e-5 I.
                *     non-terminal  g = C pd; a = 1 + g . phi(s); v = C phi(s); C += (-1/a) (v g^T), each v_r * g_j rounded before it is scaled;
                *                   theta += (residual / a) v, residual = r + gamma theta.phi(s') - theta.phi(s)
                *     terminal      v = C phi(s); a = 1 + v . phi(s); C.fill(0); theta += ((r - theta.phi(s)) / a) v.  As in the reference: after a
                *                   learner's first terminal transition C is zero and theta never moves again.
                *   iLSTD::new(basis, alpha, gamma, n_updates = config.n_steps): theta = 0, A = I, mu = 0.
                *     mu += r phi(s); A += phi(s) pd^T (terminal: pd = phi(s)); mu -= (phi(s) pd^T) theta, computed as phi(s)_i * (pd . theta) (a
                *     rounding difference); then n_updates rounds of solve(): idx = argmaxima(|mu|) (utils.rs: tolerance 1e-7 first, from f64::MIN;
                *     a later larger value within 1e-7 is appended without raising the max), and for each j in idx IN ORDER u = alpha mu_j,
                *     theta_j += u, mu -= u A[:,j] (a later j reads the mu an earlier one changed).
                * config: gamma (both), alpha and n_steps 1..32 (iLSTD); lr is unused.  Supported: per-learner f32 weights (the f32 view of theta),
                * policy RSRL_RANDOM, agent_policy -1, no epsilon schedule, the register-family Fourier orders (MountainCar 1-5, CartPole 1, Acrobot 1);
                * everything else is EINVAL at create (kernels_lstd.hpp).  The driver loop is TD's: transition, handle, Random sample, auto-reset;
                * truncation at max_episode_steps is not terminal.  rsrl_hip_reset does not touch the agents' state.  The value side is V
                * (n_outputs 1): q_evaluate writes f32(phi(s) . theta) evaluated in f64; get/set_weights carry theta as f32[F][1] (rounded out,
                * widened exactly in; C / A / mu untouched); rsrl_hip_get/set_lstd_state read and write the exact f64 state.  q_find_max / _min,
                * q_expected_value, traces, td / policy weights and handle_batch are ESTATE.  rsrl_hip_handle's td_error_out and the statistics'
                * sum |delta| are RecursiveLSTD's residual; iLSTD computes no TD error and reports, as a diagnostic, r + gamma V(s') - V(s) (terminal:
                * r - V(s)) with theta from before the update */
               RSRL_RECURSIVE_LSTD = 18, RSRL_ILSTD = 19,
               /* (20 is no algo.)  ActorCritic::tdac (control/ac.rs:87-98) with the Gibbs actor and TDCritic over the V that iLSTD learns: the agent
                * and the loop of examples/tdac.rs (eval.handle, agent.handle, sample).  RSRL_ILSTD's f64 state (theta = 0, A = I, mu = 0) beside the
                * actor's f32 theta (zero), per learner.  Per transition:
                *   p       = softmax(theta_a^T phi(s) / tau), theta_a before its update                 (f32, RSRL_TD_ACTOR_CRITIC's arithmetic)
                *   iLSTD   RSRL_ILSTD's handle, bit for bit (f64 features; terminal: pd = phi(s))
                *   critic  c = r - V'(s') (terminal: V of the terminal state s' itself) | r + gamma*V'(s') - V'(s), V' = phi . theta with the UPDATED
                *           f64 theta, summed in index order
                *   actor   e = (float)(alpha * c), the one rounding out of f64; theta_a[:,b] += e * (1[b==a] - p_b) * phi(s)         (f32)
                * No inner draw.  config: lr = iLSTD's alpha (the critic's rate, as for the other actor-critics), gamma = iLSTD's and TDCritic's,
                * n_steps = iLSTD's n_updates in 1..32, alpha = ActorCritic.alpha, tau = Softmax.tau; policy must be RSRL_SOFTMAX and agent_policy -1.
                * The VALUE side is RSRL_ILSTD's: q_evaluate writes f32(phi(s) . theta) as f32[1][M], get / set_weights carry theta as f32[F][1],
                * rsrl_hip_get/set_lstd_state are exact, n_outputs is 1, q_find_max / _min / q_expected_value are ESTATE.  The POLICY side is
                * RSRL_TD_ACTOR_CRITIC's: it reads theta_a [F][A] (policy_sample / _mode / _probs / _prob, reset's initial sample, the rollouts;
                * rsrl_hip_get/set_policy_weights).  handle_batch, traces and td weights are ESTATE.  rsrl_hip_handle's td_error_out and the
                * statistics' sum |delta| are iLSTD's diagnostic.  rsrl_hip_reset leaves both agents' state alone.  Supported: as
                * RSRL_TD_ACTOR_CRITIC; everything else is EINVAL at create (kernels_tdac_lstd.hpp).
                * On RSRL_CONTINUOUS_MOUNTAIN_CAR the same agent runs with policy RSRL_BETA (the agent and the loop of examples/tdac_beta.rs:
                * ActorCritic::tdac is generic over the policy): Fourier orders 1-5, per-learner f32 weights, agent_policy -1, no epsilon schedule.
                * The critic half is unchanged -- theta / A / mu and the diagnostic are the bits of an RSRL_ILSTD ctx's on the same transitions -- and
                * the actor is RSRL_BETA's update below with e = (float)(alpha * c).  The policy side reads the policy's two columns [F][2]
                * (rsrl_hip_policy_sample_f32 / _mode_f32 / _params / _pdf, reset's initial sample, rsrl_hip_rollout_greedy = Domain::rollout with
                * policy.mode, tdac_beta.rs:66); rsrl_hip_rollout_trajectory / _policy (int32 actions), policy_probs / _prob, q_find_max / _min,
                * q_expected_value, traces, td weights and handle_batch are ESTATE.  The checkpoint is aux_kind 11 (kernels_tdac_beta.hpp) */
               RSRL_ILSTD_ACTOR_CRITIC = 21,
               /* (22 is no algo.)  GradientMC (prediction/mc.rs:26-58): every-visit Monte-Carlo prediction, v_func = ScalarLFA(basis, SGD(lr)).
                * Handler<&Trajectory>::handle visits the transitions LAST TO FIRST (TrajectoryIter::next_back, rsrl_domains/src/lib.rs:289-319):
                *   sum = 0;  for k = n-1 .. 0:  sum = r_k + gamma * sum;  w += lr * (sum - <w, phi(s_k)>) * phi(s_k)       (w as the previous visit left it)
                * Only a transition's `from` and its reward are read; a trajectory cut by a step limit gets no bootstrap.  One visit is RSRL_TD's
                * terminal-transition update with r := sum (the return an f32 multiply followed by an add).  The return runs backwards, so the driver
                * loop keeps every learner's OPEN EPISODE on the device -- transition k's (from, reward) in row k, episode_steps[i] rows, at most
                * max_episode_steps -- and sweeps it when the episode ends (terminal or max_episode_steps), then restarts; the environment side is
                * RSRL_TD's draw for draw.  config: lr, gamma; max_episode_steps >= 1 (EINVAL for 0: an unbounded episode has no record size).
                * Supported: as RSRL_RECURSIVE_LSTD (per-learner f32 weights, the register-family Fourier orders, policy RSRL_RANDOM, agent_policy
                * -1, no epsilon schedule); everything else is EINVAL at create (kernels_gmc.hpp).  The value side is V (n_outputs 1): q_evaluate
                * writes f32[1][M], get / set_weights are f32[F][1]; q_find_max / _min, q_expected_value, traces, td / policy weights, the lstd state
                * and return_carry are ESTATE.  rsrl_hip_handle is ESTATE (there is no Handler<&Transition>): rsrl_hip_handle_batch.  The record is
                * read and written with rsrl_hip_get/set_episode_record; rsrl_hip_reset and rsrl_hip_domain_reset empty the restarted learners'
                * (episode_steps = 0), and rsrl_hip_set_episode_steps refuses a value above max_episode_steps.  The statistics' sum |delta| is the
                * sum of |sum - pred| over the sweeps, booked at the step that ended the episode.  The checkpoint holds the weights only (RSRL_TD's
                * layout): the open record is the caller's to carry, like the states, actions and episode steps */
               RSRL_GRADIENT_MC = 23,
               /* (24 is no algo.)  The batch least-squares prediction agents (prediction/lstd), Handler<&Batch>: every transition's from, to, reward and
                * terminal flag are read.  All arithmetic is f64, the features included (as RSRL_RECURSIVE_LSTD); every product is rounded.
                * LSTD::new(basis, gamma) (lstd.rs:23-37): theta = 0, A = 1e-6 I, b = 0.  handle (lstd.rs:59-81) walks the batch FIRST TO LAST:
                *   b += r phi(s);   non-terminal: pd = gamma phi(s') - phi(s), A -= phi(s) (x) pd;   terminal: A += phi(s) (x) phi(s);   then solve().
                * LSTDLambda::new(basis, gamma, lambda) (lstd_lambda.rs:25-41): the same start and z = 0.  handle (lstd_lambda.rs:66-103) walks the batch
                * LAST TO FIRST (`batch.iter().rev()`: the trace runs backwards in time); z survives from batch to batch, only a terminal transition zeroes it:
                *   c = lambda gamma;  z = c z + phi(s);  b += r z;   non-terminal: pd = phi(s) - gamma phi(s'), A += z (x) pd;
                *   terminal: A += z (x) phi(s), z = 0;   then solve().
                * solve() (lstd.rs:40-50, lstd_lambda.rs:44-54) is theta <- A.solve(b) by LAPACK, with an SVD pseudo-inverse when LAPACK reports an exactly
                * zero pivot.  Here it is ONE fixed operation order (kernels_lstd_batch.hpp; tests/lstd_batch_numpy.py restates it, bit for bit): Gaussian
                * elimination with partial pivoting on a copy of A and b -- the pivot of column k is the first row in index order, among the rows not yet
                * used, with the largest |a[i][k]| -- and back substitution with ascending j.  DEPARTURE: there is NO SVD fallback.  A solve whose pivot
                * candidates hold no value above 0 is abandoned: theta keeps its value (what the reference does when both attempts fail) and the learner's
                * singular_solves counter (u32) goes up by one.
                * The driver loop is RSRL_GRADIENT_MC's on the f64 state: the transition's (from, reward) is appended to the learner's open episode (row
                * k's `to` is row k+1's `from`; the last row's `to` and terminal flag are the step's own), at the episode's end (terminal or
                * max_episode_steps) the batch is handled and solved, then the restart and the Random sample; the environment side is RSRL_TD's draw for
                * draw.  config: gamma, lambda (RSRL_LSTD_LAMBDA); max_episode_steps >= 1 (EINVAL for 0).  Supported: as RSRL_GRADIENT_MC; everything else
                * is EINVAL at create.  The value side is V, as RSRL_RECURSIVE_LSTD (n_outputs 1; q_evaluate writes f32(phi . theta); get / set_weights carry
                * theta as f32[F][1]).  rsrl_hip_handle and rsrl_hip_handle_batch are ESTATE: rsrl_hip_handle_transitions.  rsrl_hip_lstd_solve is the
                * public solve(); rsrl_hip_get/set_lstd_batch_state carry the exact state (rsrl_hip_get/set_lstd_state is ESTATE);
                * rsrl_hip_get/set_episode_record, set_episode_steps, reset and domain_reset behave as for RSRL_GRADIENT_MC (a reset leaves the agent's
                * state alone).  td_out and the statistics' sum |delta| are the diagnostic r + gamma V(s') - V(s) (terminal: r - V(s)) with theta as it
                * stood before the batch's solve, booked at the step that ended the episode: the agents compute no TD error.  The checkpoint is aux_kind 10;
                * the open record is the caller's to carry.  (LambdaLSPE, the third batch agent of prediction/lstd, is RSRL_LAMBDA_LSPE.) */
               RSRL_LSTD = 25, RSRL_LSTD_LAMBDA = 26,
               /* (27 is no algo.)  NAC (control/nac.rs:47-59), natural actor-critic, with the Beta policy and a SARSA critic over the stable
                * compatible basis: the agent and the loop of examples/nac_beta.rs.  critic = SARSA{q_func: LFA::scalar(SCB{policy, basis},
                * SGD(lr)), policy, gamma} (control/td/sarsa.rs:53-75); SCB::project((s, a)) (fa/linear.rs:79-103) is grad_log pi(a|s)
                * (policies/beta.rs:119-129) chained with basis.project(s): 3F features
                *   psi(s, a) = [ g_a sigma(x_a) phi(s) ; g_b sigma(x_b) phi(s) ; phi(s) ]     (x, g, sigma: RSRL_BETA's, below)
                * and Q(s, a) = <w, psi(s, a)>, w f32[3F] per learner, zero at create (linear.rs:253-261); evaluated as three length-F dots
                * combined, fma(c_a, d_0, fma(c_b, d_1, d_2)).  Per transition (SARSA::handle): delta = r - Q(s, a) on a terminal transition, else
                * r + gamma Q(s', na) - Q(s, a) with na = policy.sample(s') on the agent's own stream (the reference: thread_rng()); then
                * w += lr delta psi(s, a) (linear.rs:277-288).  The policy's columns do not move.  NAC::handle(()): g = w[0 .. 2F-1],
                * norm = max(sqrt(sum g_j^2), 1e-3), w_a += (alpha / norm) g[0 .. F-1], w_b += (alpha / norm) g[F .. 2F-1] (beta.rs:247-276,
                * fa/composition.rs:55-66, linear.rs:184-196); the response is norm; the critic's weights are not reset.
                * config: lr = the critic's SGD rate (0.01 in the example), gamma = SARSA.gamma (0.999), alpha = NAC.alpha (0.1, rounded to f32
                * once), n_steps = the actor's period P in [1, 65 536] (the example hard-codes 100); max_episode_steps may be 0.
                * rsrl_hip_train is nac_beta.rs:55-76 with i the 0-based index of the step in its episode: t = env.transition(2a - 1) with the
                * agent's action a in t's place; critic.handle(t); a = policy.sample(s') (after the restart when the episode ended); then
                * NAC::handle(()) if i % P == 0 -- i = 0 included: the sample is drawn from the columns BEFORE the actor's step, the next
                * transition's psi(s, a) is evaluated with the columns AFTER it.  The statistics' sum |delta| is SARSA's.
                * The value side is the critic: rsrl_hip_get/set_weights carry w as f32[3F][1], rsrl_hip_n_outputs is 1, rsrl_hip_n_weight_rows
                * is 3F (SCB::n_features); Q needs an action: rsrl_hip_q_evaluate_f32; rsrl_hip_q_evaluate / q_find_max / _min / q_expected_value
                * are ESTATE.  The policy side is RSRL_BETA's unchanged (policy_sample_f32 / _mode_f32 / _params / _pdf, get/set_policy_weights
                * f32[F][2], n_policy_outputs 2, reset's initial sample).  rsrl_hip_handle_f32 is critic.handle alone (td_error_out = delta; it does
                * NOT move the actor); rsrl_hip_nac_update is NAC::handle(()); rsrl_hip_domain_step_f32 with actions == NULL applies the loop's
                * 2a - 1 to the pending actions; rsrl_hip_rollout_greedy is Domain::rollout(|s| 2 * policy.mode(s) - 1) (nac_beta.rs:81-82);
                * rsrl_hip_rollout_trajectory / _policy, handle_batch, handle_transitions, traces, td weights and the lstd state are ESTATE.
                * Supported: RSRL_CONTINUOUS_MOUNTAIN_CAR with policy RSRL_BETA, agent_policy -1 (the critic shares the policy), Fourier orders
                * 1-5, per-learner f32 weights, no epsilon schedule; everything else is EINVAL at create.  The checkpoint is aux_kind 12.
                * DEPARTURES: f32 for the reference's f64; the score, modes() and map_onto recalled (RSRL_BETA, RSRL_CONTINUOUS_MOUNTAIN_CAR); the
                * action clamped to [2^-24, 1 - 2^-24] before its logarithms; SARSA's thread_rng() draw is a keyed stream (distribution parity is
                * the contract); the period is a parameter (kernels_cont.hpp).
                * With policy RSRL_GAUSSIAN the same algo is the agent and the loop of examples/nac.rs (kernels_cont.hpp): the critic, the
                * actor's update (w_m, w_s in w_a's and w_b's place), the value side, the accessors and the ESTATE list are the ones above, with
                *   psi(s, a) = [ g_mu phi(s) ; g_Sigma sigma(x_s) phi(s) ; phi(s) ]     (g_mu, g_Sigma, x_s, sigma: RSRL_GAUSSIAN's, below)
                * and ONE difference in the loop: the domain sees the action itself (nac.rs:63), no 2a - 1 -- rsrl_hip_domain_step_f32 with
                * actions == NULL steps on the pending actions literally, rsrl_hip_rollout_greedy is Domain::rollout(|s| policy.mode(s))
                * (nac.rs:81).  The inner draw na is the Gaussian sample on BLK_INNER; a caller's action is any finite f32, not clamped.  The
                * example's constants: lr 0.01, gamma 0.999, alpha 0.01, order 3, P = 100, cap 1 000.  Supported: as above with RSRL_GAUSSIAN in
                * RSRL_BETA's place.  The checkpoint is aux_kind 14 (aux_kind 12's sections): a Beta NAC file does not load into a Gaussian ctx, nor
                * the other way round.  DEPARTURES: f32; the score DEFINED (RSRL_GAUSSIAN); the keyed stream; the period a parameter.
                * (nac_softmax.rs, NAC over the Gibbs policy, is RSRL_GIBBS_NAC.)  Not built: Gaussian<M, f64> (the fixed-variance policy, policies/gaussian/fixed_var.rs); the Gaussian policy
                * under RSRL_ILSTD_ACTOR_CRITIC; IPP */
               RSRL_NAC = 28,
               /* (29 is no algo.)  GTD2 (prediction/td/gtd2.rs:27-86) and TDC (prediction/td/tdc.rs:41-101): gradient-TD prediction over TWO
                * ScalarLFAs on one basis, theta (fa_theta / q_func: the value function) and w (fa_w / td_est: the second weight column), per
                * learner f32[F] each, zero at create.  With phi = phi(s), phi' = phi(s'), all three products read BEFORE anything moves:
                *   w_s = <w, phi>, th_s = <theta, phi>, th_n = <theta, phi'>;   td = r - th_s (terminal) | r + gamma th_n - th_s
                *   w     += lr_td (td - w_s) phi                                                         (both)
                *   GTD2:  theta += lr w_s phi;   theta -= gamma (lr w_s) phi'      (ScaledGradientUpdate{w_s, phi - gamma phi'})
                *   TDC :  theta += lr td phi;    theta -= (lr w_s) phi'            (GradientUpdate(td phi - w_s phi'): no gamma, tdc.rs:91)
                * Neither rule has a terminal case for the gradient: phi' of a terminal transition is the terminal state's own features (what
                * rsrl_hip_domain_step reports) and is subtracted as on any other step.  The f32 operation order is fixed (kernels_gtd.hpp;
                * tests/gtd_numpy.py restates it bit for bit): RSRL_TD's dot products and TD error, then one fused multiply-add per element and
                * column move, theta's two moves one after the other.  RSRL_TDC with w = 0 and lr_td = 0 is RSRL_TD's arithmetic.
                * DEPARTURE: the reference applies these updates past the optimiser (fa/linear.rs:170-196: scaled_addto / addto), so every move
                * has the literal step size 1 -- except TDC's td_est, which goes through its SGD (linear.rs:237-248).  On a Fourier basis, where
                * ||phi||^2 reaches F, both rules then diverge (f64, MountainCar order 1, random transitions: |theta| and |w| pass 1e6 within 64
                * transitions).  Here config.lr scales every move of theta and config.lr_td every move of w: lr = lr_td = 1 is the reference's
                * GTD2, lr = 1 the reference's TDC with td_est = SGD(lr_td); a multiplication by 1.0f is exact, so those settings are the literal
                * rules.  config: lr, lr_td (>= 0, else EINVAL), gamma.  The driver loop is RSRL_TD's: transition, handle, Random sample,
                * auto-reset -- the environment side is RSRL_TD's draw for draw; truncation at max_episode_steps is not terminal; rsrl_hip_reset
                * leaves both columns alone.  Supported: as RSRL_RECURSIVE_LSTD (per-learner f32 weights, the register-family Fourier orders,
                * policy RSRL_RANDOM, agent_policy -1, no epsilon schedule); everything else is EINVAL at create (kernels_gtd.hpp).  The value
                * side is V (n_outputs 1): q_evaluate writes f32[1][M] from theta, get / set_weights carry theta as f32[F][1],
                * rsrl_hip_get/set_td_weights carry w as f32[F][1]; q_find_max / _min and q_expected_value are ESTATE.  rsrl_hip_handle takes
                * transitions as RSRL_TD's does; td_error_out and the statistics' sum |delta| are td.  handle_batch, handle_transitions, traces,
                * policy weights and the lstd state are ESTATE.  The checkpoint is aux_kind 13 (theta, then w); a file of one of the two agents
                * does not load into a ctx of the other */
               RSRL_GTD2 = 30, RSRL_TDC = 31,
               /* (34 is no algo.)  The continuous TD ActorCritic: ActorCritic::tdac(v_func, policy, alpha, gamma) (control/ac.rs:32-52, :87-115) with a
                * TD(0) state-value critic over the Gaussian or the Beta policy on RSRL_CONTINUOUS_MOUNTAIN_CAR -- RSRL_TD_ACTOR_CRITIC's arithmetic for
                * the critic half, RSRL_CACLA's layout for everything else.  (Listed before RSRL_CACLA, which stays the enum's last enumerator; a new
                * number and not RSRL_TD_ACTOR_CRITIC on this domain, which stays refused there.)  eval = TD{v_func: LFA::scalar(basis, SGD(lr)), gamma}
                * (prediction/td/td.rs:38-58), w f32[F] per learner, zero at create; the policy's two columns f32[F][2], zero at create, read as
                * get/set_policy_weights read them for each policy (RSRL_GAUSSIAN: the mean's, the stddev's; RSRL_BETA: alpha's, beta's).
                * The loop is that of tdac.rs and tdac_beta.rs: t = env.transition(..); eval.handle(&t); agent.handle(&t), whose critic reads eval's
                * UPDATED weights; a = policy.sample(s') with the updated columns, taken after the restart if the episode ended (terminal or cut by
                * max_episode_steps: one sample per step, on BLK_STEP).  There is no inner draw.  The domain sees the action itself under
                * RSRL_GAUSSIAN (nac.rs:63's convention, as RSRL_CACLA) and 2a - 1 under RSRL_BETA (nac_beta.rs:63's mapping of the sample's [0, 1] onto
                * the domain's [-1, 1]; tdac_beta.rs itself hands the domain a, which RSRL_ILSTD_ACTOR_CRITIC keeps); the agent sees a.
                * The f32 operation order is fixed (kernels_cont.hpp, tdac_cont_step; tests/tdac_cont_numpy.py restates it in f64).  Per
                * transition (s, a, r, s', term):
                *   1. x0 = <col0, phi(s)>, x1 = <col1, phi(s)>, the columns before any move
                *   2. RSRL_TD's arithmetic: v_s = <w, phi(s)>, v_n = <w, phi(s')>; td = r - v_s (terminal) | r + gamma v_n - v_s;
                *      w += (lr td) phi(s), one fused multiply-add per element
                *   3. TDCritic::target with the updated w (ac.rs:40-50), literally: nv = <w, phi(s')>; c = r - nv on a terminal transition (it reads
                *      V of the terminal state itself, as RSRL_TD_ACTOR_CRITIC does), else c = r + gamma nv - <w, phi(s)>; e = alpha c, alpha rounded
                *      to f32 once
                *   4. policy.handle(StateActionUpdate{s, a, error: e}), always (no gate):
                *      RSRL_GAUSSIAN  (mu, sd) from (x0, x1); c_m = g_mu, c_s = g_Sigma sigma(x1); w_m += (e c_m) phi(s), w_s += (e c_s) phi(s) --
                *                     RSRL_CACLA's expressions with this e (general.rs:196-212)
                *      RSRL_BETA      ac = the action clamped to [2^-24, 1 - 2^-24]; g_a = ln ac - psi(alpha) + psi(alpha + beta), g_b = ln(1 - ac) -
                *                     psi(beta) + psi(alpha + beta), one shared psi(alpha + beta); s_a = e g_a sigma(x_a), s_b likewise;
                *                     w_a += s_a phi(s), w_b += s_b phi(s) -- RSRL_ILSTD_ACTOR_CRITIC's actor expressions, left to right
                *   There is no safeguard: a coefficient that is not finite propagates, as in the reference.
                * w and td are the bits of an RSRL_TD ctx's on the same transitions, whatever the columns hold.  With c < 0 and a > mu the Gaussian
                * mean's preference <w_m, phi(s)> DECREASES (e c_m = alpha c (a - mu) / Sigma < 0): the standard policy-gradient step, where
                * RSRL_CACLA's literal rule moves it up on either side.
                * config: lr = TD's SGD rate, gamma = TD's and TDCritic's, alpha = ActorCritic.alpha; n_steps is not read; max_episode_steps may be
                * 0, truncation is not terminal.  The statistics' sum |delta| is TD's.
                * The value side is V, as RSRL_CACLA's: rsrl_hip_n_outputs is 1, rsrl_hip_q_evaluate writes f32(phi . w), rsrl_hip_get/set_weights
                * carry w as f32[F][1]; q_find_max / _min, q_expected_value and q_evaluate_f32 are ESTATE.  The policy side is the chosen policy's,
                * unchanged (policy_sample_f32 / _mode_f32 / _params / _pdf, get/set_policy_weights f32[F][2], n_policy_outputs 2, reset's initial
                * sample on BLK_INIT; reset leaves all three columns alone).  rsrl_hip_handle_f32 is eval.handle then ActorCritic::handle on caller
                * transitions (td_error_out = TD's error; host actions by each policy's rule: Beta clamps, a NaN or infinite one is EINVAL);
                * rsrl_hip_domain_step_f32 with actions == NULL applies each policy's loop convention to the pending actions;
                * rsrl_hip_rollout_greedy is each policy's mode rollout (2 mode - 1 under RSRL_BETA, mode under RSRL_GAUSSIAN); rsrl_hip_nac_update,
                * rsrl_hip_handle, handle_batch, handle_transitions, rollout_trajectory / _policy, traces, td weights and the lstd state are ESTATE.
                * Supported: RSRL_CONTINUOUS_MOUNTAIN_CAR with policy RSRL_GAUSSIAN or RSRL_BETA, agent_policy -1, Fourier orders 1-5, per-learner
                * f32 weights, no epsilon schedule; everything else is EINVAL at create.  The checkpoint is aux_kind 16 (Beta) / 17 (Gaussian), w then
                * the two columns as aux_kind 15: a file of either loads into no other ctx, and no other kind into these.  DEPARTURES: f32 for the
                * reference's f64; the scores as defined for each policy (RSRL_BETA, RSRL_GAUSSIAN); the Gaussian loop is this library's (the
                * reference has no tdac example over its Gaussian policy), the Beta loop tdac_beta.rs's order with nac_beta.rs's action mapping */
               RSRL_CONTINUOUS_TD_ACTOR_CRITIC = 35,
               /* (36 is no algo, and neither is 38.)  NAC over the Gibbs policy: the agent and the loop of examples/nac_softmax.rs (control/nac.rs:47-59)
                * on the domains with an enumerable action set.  (Listed before RSRL_CACLA, which stays the enum's last enumerator; a new number and
                * not RSRL_NAC with RSRL_SOFTMAX: RSRL_NAC keeps refusing Softmax and the discrete domains.)  policy = Gibbs::standard(LFA::vector(
                * basis, SGD(1.0), A)) = Softmax(tau), theta f32[F][A] per learner, zero at create; the critic is SARSA{q_func: LFA::scalar(
                * SCB{policy, basis}, SGD(lr)), policy, gamma} (control/td/sarsa.rs:53-75), w f32[(A+1) F] per learner, zero at create.
                * Softmax::grad_log((s, a)) (policies/softmax.rs:113-128) is the (F, A) matrix whose column b is (1[b==a] - p_b) phi(s), p =
                * softmax_stable(theta^T phi(s) / tau) -- no 1/tau, as for RSRL_ACTOR_CRITIC; SCB::n_features() (fa/linear.rs:85-89) is
                * policy.n_weights() + basis.dim() = (A+1) F; NAC::handle(()) takes cw[0 .. F A], reshapes it row-major to (F, A) and steps the
                * policy by (alpha / max(||grad||, 1e-3)) grad (softmax.rs:208-221).
                * THE ONE DEFECT TAKEN OUT: SCB::project (fa/linear.rs:91-102) chains grad_log(..).index_axis_move(Axis(1), 0) -- column 0 only, F
                * values -- with phi: 2F features against (A+1) F weights.  The Beta and Gaussian policies have one-column Jacobians, for Gibbs with
                * A > 1 it is a length mismatch and the example stops at its first critic.handle.  Built with the flattening of the sibling
                * CompatibleBasis::project (:42-46), grad_log(args).into_shape(n_features), row-major -- exactly the order NAC::handle reads back:
                *   psi(s, a)[f*A + b] = (1[b==a] - p_b) * phi(s)[f]      (f < F, b < A)
                *   psi(s, a)[F*A + f] = phi(s)[f]
                *   Q(s, a) = <w, psi(s, a)>
                * The f32 operation order is fixed (kernels_gibbs_nac.hpp; tests/gnac_numpy.py restates it):
                *   p(s) = RSRL_ACTOR_CRITIC's probabilities on theta;  c_b = 1[b==a] - p_b;  d_b = <w_b, phi> for the A score blocks (w_b[f] =
                *   w[f*A + b]), d_v = <w_v, phi> for the basis block, each in the weight dots' summation order;
                *   Q(s, a) = fma(c_0, d_0, fma(c_1, d_1, ... fma(c_{A-1}, d_{A-1}, d_v)))
                *   SARSA::handle: na = the sample from p(s') on the agent's own keyed draw (BLK_INNER, not consumed by a terminal transition);
                *     delta = r - Q(s,a) (terminal) | fma(gamma, Q(s',na), r) - Q(s,a);  sc = lr delta;  block b += (sc c_b) phi, the basis block
                *     += sc phi, one fused multiply-add per entry;  theta does not move
                *   NAC::handle(()): ss = sum over j = 0 .. F A - 1 in that order of w[j] w[j], each square rounded before it is added;  norm =
                *     max(sqrtf(ss), 1e-3f);  scale = alpha32 / norm;  theta[f][b] = fma(scale, w[f*A + b], theta[f][b]);  the critic is not
                *     reset;  the response is norm
                * The driver loop (nac_softmax.rs:57-78), i the 0-based index of the step in its episode: env.transition(a); critic.handle; a =
                * policy.sample(s'), taken after the restart if the episode ended or was cut (BLK_STEP / BLK_RESET as the other loops); then
                * NAC::handle(()) if i % P == 0, i = 0 included.  The statistics' sum |delta| is SARSA's.
                * config: lr = the critic's SGD rate (0.01 in the example), gamma (0.999), alpha = NAC.alpha (0.01, rounded to f32 once), tau (1.0),
                * n_steps = the actor's period P in [1, 65 536] (else EINVAL); max_episode_steps may be 0.
                * rsrl_hip_n_outputs is 1 and rsrl_hip_n_weight_rows (A+1) F: rsrl_hip_get/set_weights carry w as f32[(A+1) F][1] in the row order
                * above; theta travels through rsrl_hip_get/set_policy_weights as f32[F][A].  rsrl_hip_handle is critic.handle alone (td_error_out =
                * delta; the actor does not move; the inner draw is batch-step t's); rsrl_hip_nac_update is NAC::handle(()); rsrl_hip_q_evaluate
                * writes f32[A][M], row b = Q(s_i, b) against learner i's w and theta, read-only.  The policy side is RSRL_ACTOR_CRITIC's,
                * unchanged (policy_sample / _mode / _probs / _prob on theta, reset's initial sample on BLK_INIT, the rollouts, n_policy_outputs =
                * A).  q_find_max / _min, q_expected_value, every *_f32 call, handle_batch, handle_transitions, traces, td, behaviour and lstd
                * accessors and the episode record are ESTATE; the q carry is EINVAL.
                * Supported: policy RSRL_SOFTMAX, agent_policy -1, the register-family Fourier orders (MountainCar 1-5, CartPole 1, Acrobot 1),
                * per-learner f32 weights, no epsilon schedule; everything else -- shared or bf16 weights, RSRL_HIV_TREATMENT,
                * RSRL_CONTINUOUS_MOUNTAIN_CAR -- is EINVAL at create.  The checkpoint is aux_kind 18 (w, then theta): it loads into no other
                * agent's ctx, and no other agent's file into this one.  DEPARTURES: f32 for the reference's f64; psi flattened as stated; SARSA's
                * thread_rng() draw is a keyed stream (distribution parity is the contract); the period is a parameter (the example hard-codes it) */
               RSRL_GIBBS_NAC = 37,
               /* (40 is no algo.)  LambdaLSPE (prediction/lstd/lambda_lspe.rs:27-107), least-squares policy evaluation: the last agent of
                * prediction/lstd, Handler<&Batch> as RSRL_LSTD_LAMBDA.  Everything is f64 on RSRL_LSTD's features and every product is rounded.
                * LambdaLSPE::new(basis, alpha, gamma, lambda) (:28-43): theta = 0, A = 1e-6 I, b = 0, and the scalar return correction delta = 0.
                * handle (:71-106) walks the batch LAST TO FIRST; theta does not move during the walk.  For each transition:
                *   delta = delta * (gamma * lambda)                                                                        (:76)
                *   terminal (:78-86):  b += (delta + r) phi(s);  A += phi(s) (x) phi(s);  delta = 0      -- theta . phi(s) is NOT added here
                *   otherwise (:87-100): v_s = phi(s) . theta and v_n = phi(s') . theta (ascending index, the sum starting at 0);
                *     delta = delta + (r + gamma * v_n - v_s);  b += (v_s + delta) phi(s);  A += phi(s) (x) phi(s)
                * The scalar in front of phi(s) is one rounded sum; each element of b and A is one rounded product, then added.  Then solve()
                * (:47-62; PRIVATE in the reference, served here as rsrl_hip_lstd_solve exactly as handle ends with it): x = A.solve(b) by RSRL_LSTD's
                * fixed elimination (no SVD); on success theta_r = (1 - alpha) * theta_r + alpha * x_r -- 1 - alpha computed once in f64, three rounded
                * operations per element -- and A, b and delta are set to zero.  An abandoned elimination keeps theta, A, b AND delta (what the
                * reference does when both of its attempts fail) and counts in singular_solves.
                * DEPARTURE, THE ROW RULE.  The reference's solve() zeroes A and b, so a batch shorter than F leaves a Gram matrix of fewer than F
                * vectors: singular in exact arithmetic and answered there by the SVD fallback, which this library does not have -- and which plain
                * elimination does not even report (in rounding such a system gets pivots near 1e-17 and one arbitrary member of its solution set
                * comes back).  So every learner holds a row count `rows` in 0 .. F: F at create (the identity's F rows make the first system full
                * rank); every handled batch sets rows = min(rows + len, F); a successful solve sets it to 0.  solve() runs the elimination only when
                * rows == F.  Otherwise the solve is DEFERRED: nothing moves, singular_solves does not count, and the next batch adds to the same A,
                * b and delta.
                * The driver loop is RSRL_LSTD's, draw for draw.  config: alpha (finite, else EINVAL), gamma, lambda; max_episode_steps >= 1.  Supported:
                * exactly as RSRL_LSTD_LAMBDA.  rsrl_hip_get/set_lstd_batch_state carry the state through RSRL_LSTD_LAMBDA's signature: z[0] = delta and
                * z[1] = rows as an exact integer; get writes z[2 ..] as 0 and set does not read it; z == NULL: neither is read or written; a set whose rows
                * is not an integer in 0 .. F is EINVAL and moves nothing.  The value side, handle_transitions, the episode record, reset, domain_reset,
                * the ESTATE refusals (handle, handle_batch, get/set_lstd_state), td_out and the statistics are RSRL_LSTD's.  The checkpoint is
                * aux_kind 19: RSRL_LSTD's sections, then f64 (delta, rows)[N], then u32 singular_solves[N].  Not built: the SVD fallback */
               RSRL_LAMBDA_LSPE = 39,
               /* (32 is no algo.)  CACLA (control/cacla.rs:42-64), the continuous actor-critic learning automaton, over the Gaussian policy with a
                * TD(0) state-value critic.  CACLA{critic, policy, alpha, gamma}: the critic is a closure over V that the agent reads and never
                * writes -- a caller trains it; here it is eval = TD{v_func: LFA::scalar(basis, SGD(lr)), gamma} (prediction/td/td.rs:38-58), w
                * f32[F] per learner, zero at create.  Per transition (s, a, r, s', term), cacla.rs:42-64:
                *   v = critic(s);   target = r (terminal: r alone) | r + gamma critic(s');   if target > v (strict):
                *   policy.handle(StateActionUpdate{s, a, error: (a - policy.mode(s)) * alpha})
                * and Gaussian::handle (policies/gaussian/general.rs:196-212) is  w_m += (error g_mu) phi(s),  w_s += (error g_Sigma) grad stddev(s)
                * with grad stddev(s) = sigma(x_s) phi(s) for the Softplus composition (g_mu, g_Sigma, x_s, sigma: RSRL_GAUSSIAN's, below).
                * The reference has no example for CACLA, so the loop is this library's, in the order tdac.rs, tdac_beta.rs and nac.rs all use:
                * t = env.transition(a) -- the domain sees the action itself, as in nac.rs:63 --; eval.handle(&t); agent.handle(&t), whose critic
                * reads eval's UPDATED weights; a = policy.sample(s') with the updated columns, taken after the restart if the episode ended
                * (terminal or cut by max_episode_steps: one sample per step, on BLK_STEP).  There is no inner draw.
                * The f32 operation order is fixed (kernels_cont.hpp, cacla_step; tests/cacla_numpy.py restates it):
                *   1. x_m = <w_m, phi(s)>, x_s = <w_s, phi(s)>
                *   2. RSRL_TD's arithmetic: v_s = <w, phi(s)>, v_n = <w, phi(s')>; td = r - v_s (terminal) | r + gamma v_n - v_s;
                *      w += (lr td) phi(s), one fused multiply-add per element
                *   3. with the updated w: v = <w, phi(s)>; target = r (terminal) | r + gamma <w, phi(s')>; gate = target > v (a NaN closes it)
                *   4. gate open: (mu, sd) from (x_m, x_s); e = (a - mu) alpha; c_m = g_mu, c_s = g_Sigma sigma(x_s);
                *      w_m += (e c_m) phi(s), w_s += (e c_s) phi(s), one fused multiply-add per element
                * w and td are the bits of an RSRL_TD ctx's on the same transitions whatever the columns are; a closed gate leaves both columns'
                * bits as they were, even where the coefficients would not be finite (the update sits behind the gate, not behind a product with 0).
                * THE LITERAL RULE, a statement about the reference: the mean's step is e c_m = alpha (a - mu)^2 / Sigma >= 0 whatever side of the
                * mean the action lay on -- the error already holds (a - mu), and the policy multiplies it by its score once more.  This is not
                * van Hasselt's mu += alpha (a - mu).  The reference's rule is what is built (the stance taken for RSRL_GTD2 and for the Gaussian
                * RSRL_NAC), with no safeguard: sd is floored at 0.01 only, so the coefficients reach 1e4 and a run need not stay finite.
                * config: lr = TD's SGD rate, gamma = TD's and CACLA's, alpha = CACLA.alpha (rounded to f32 once); n_steps is not read;
                * max_episode_steps may be 0, truncation is not terminal.  The statistics' sum |delta| is TD's.
                * The value side is V, as RSRL_TD's: rsrl_hip_n_outputs is 1, rsrl_hip_n_weight_rows is F, rsrl_hip_q_evaluate writes f32(phi . w),
                * rsrl_hip_get/set_weights carry w as f32[F][1]; q_find_max / _min, q_expected_value and q_evaluate_f32 are ESTATE.  The policy
                * side is RSRL_GAUSSIAN's unchanged (policy_sample_f32 / _mode_f32 / _params / _pdf, get/set_policy_weights f32[F][2],
                * n_policy_outputs 2, reset's initial sample on BLK_INIT; reset leaves all three columns alone).  rsrl_hip_handle_f32 is eval.handle
                * then CACLA::handle on caller transitions (td_error_out = TD's error; a NaN or infinite host action: EINVAL);
                * rsrl_hip_domain_step_f32 with actions == NULL steps on the pending actions literally; rsrl_hip_rollout_greedy is
                * Domain::rollout(|s| policy.mode(s)); rsrl_hip_nac_update, rollout_trajectory / _policy, handle_batch, handle_transitions, traces,
                * td weights and the lstd state are ESTATE.  Supported: RSRL_CONTINUOUS_MOUNTAIN_CAR with policy RSRL_GAUSSIAN, agent_policy -1,
                * Fourier orders 1-5, per-learner f32 weights, no epsilon schedule; everything else is EINVAL at create -- RSRL_BETA included (no
                * reference loop says whether the domain would see a or 2a - 1).  The checkpoint is aux_kind 15 (w, then the two columns): a CACLA
                * file does not load into an RSRL_NAC ctx, nor the other way round.  DEPARTURES: f32 for the reference's f64; the score DEFINED
                * (RSRL_GAUSSIAN); the loop is this library's.  Not built: Gaussian<M, f64>, the fixed-variance policy */
               RSRL_CACLA = 33 } rsrl_algo;
/* rsrl::traces::{Accumulate, Saturate (Trace::replacing), Dutch}      traces.rs:188-240 */
typedef enum { RSRL_TRACE_ACCUMULATE = 0, RSRL_TRACE_SATURATE = 1, RSRL_TRACE_DUTCH = 2 } rsrl_trace;
/* rsrl::policies::{Greedy, EpsilonGreedy, Softmax, Random}
 *   greedy.rs:16-84, epsilon_greedy.rs:14-83, softmax.rs:55-143, random.rs:13-48
 * Beta (policies/beta.rs) over two Composition<ScalarLFA, Softplus> (fa/composition.rs:98-115, fa/transforms.rs:196-218): a CONTINUOUS policy, for
 *   RSRL_ILSTD_ACTOR_CRITIC and RSRL_NAC on RSRL_CONTINUOUS_MOUNTAIN_CAR only (EINVAL elsewhere, and as agent_policy).  Per learner two weight columns w_a, w_b
 *   f32[F] (zero at create; rsrl_hip_get/set_policy_weights carry them as f32[F][2], column 0 = alpha's; rsrl_hip_n_policy_outputs = 2).  With
 *   x_a = <w_a, phi(s)>, x_b likewise (f32): alpha = softplus(x_a) + 1, beta = softplus(x_b) + 1, softplus(x) = x for x >= 10 else ln(1 + exp(x))
 *   (MIN_TOL = 1.0, beta.rs:19, :58-67): both >= 1.
 *   sample  X = Ga / (Ga + Gb), Ga ~ Gamma(alpha, 1), Gb ~ Gamma(beta, 1) by Marsaglia-Tsang with at most 8 rounds per gamma (then the value is
 *           d = k - 1/3), clamped to [2^-24, 1 - 2^-24].  Round j of the sample for purpose P (the step's draw, the initial sample, an API call)
 *           takes the whole Philox block at block word P + 256 (j + 1): a function of (seed, global learner id, t, purpose) only.  The reference
 *           samples through rstat / rand_distr from thread_rng(): distribution parity is the contract, as for every other policy.
 *   mode    (alpha - 1) / (alpha + beta - 2) if both exceed 1, else the mean alpha / (alpha + beta) (beta.rs:141-150; rstat's modes() is not in the
 *           reference tree: this is the library's definition).
 *   update  g_a = ln a - psi(alpha) + psi(alpha + beta), g_b = ln(1 - a) - psi(beta) + psi(alpha + beta) (psi = digamma; the score is recalled from
 *           rstat::univariate::beta, not pinned by the reference tree);  w_a += e g_a sigma(x_a) phi(s),  w_b += e g_b sigma(x_b) phi(s), sigma =
 *           Softplus's gradient (1 for x >= 10, else the logistic), SGD(1.0) (beta.rs:153-187); both parameters are read before either column
 *           moves.  DEPARTURE: a caller-supplied action is clamped to the sample's interval before its logarithms (the reference would produce
 *           infinities for 0 and 1), in the spirit of the index actions' clamp.
 * (5 is no policy.)  Gaussian (policies/gaussian/{mod,general}.rs), Gaussian<ScalarLFA, Composition<ScalarLFA, Softplus>> with SGD(1.0) on both
 *   (nac.rs:31-35): the second CONTINUOUS policy, for RSRL_NAC, RSRL_CACLA and RSRL_CONTINUOUS_TD_ACTOR_CRITIC on RSRL_CONTINUOUS_MOUNTAIN_CAR only (EINVAL elsewhere, RSRL_ILSTD_ACTOR_CRITIC
 *   included, and as agent_policy).  Per learner two weight columns w_m, w_s f32[F] (zero at create; get/set_policy_weights: f32[F][2], column 0 =
 *   the mean's, column 1 = the stddev's; rsrl_hip_n_policy_outputs = 2).  With x_m = <w_m, phi(s)>, x_s likewise (f32):
 *   params  mu = x_m, sd = softplus(x_s) + 0.01 (MIN_TOL, mod.rs:37, :67), Sigma = sd * sd (into_cov: mod.rs:82 builds the distribution from the
 *           VARIANCE).  rsrl_hip_policy_params writes (mu, sd).
 *   sample  a = fma(sd, z, mu), z = sqrt(-2 ln u1) cos(2 pi u2) from the whole Philox block at block word P + 256 (P: the step's draw, the critic's
 *           inner draw, the initial sample, an API call), words x and y converted as Beta's (u1 in (0, 1], u2 in [0, 1)): one block, no loop, so
 *           |z| <= sqrt(48 ln 2) < 5.77.  NOT clamped: the domain clips (map_onto).  A function of (seed, global learner id, t, purpose) only.
 *   mode    mu (general.rs:177).
 *   density exp(-(a - mu)^2 / (2 Sigma)) / sqrt(2 pi Sigma) (rsrl_hip_policy_pdf).
 *   score   g_mu = (a - mu) / Sigma, g_Sigma = ((a - mu)^2 - Sigma) / (2 Sigma^2): the derivatives of the log density in the builder's two
 *           arguments, the mean and the variance.  DEFINED here: rstat's normal::Grad is not in the reference tree.  grad_log (general.rs:142-157)
 *           is [ g_mu phi ; g_Sigma sigma(x_s) phi ], literally: the reference does not multiply the second block by d Sigma / d sd = 2 sd.
 *   A caller-supplied action is any finite f32, taken as it is (NaN or infinity in a host array: EINVAL). */
typedef enum { RSRL_GREEDY = 0, RSRL_EPSILON_GREEDY = 1, RSRL_SOFTMAX = 2, RSRL_RANDOM = 3, RSRL_BETA = 4, RSRL_GAUSSIAN = 6 } rsrl_policy;
/* one LFA per learner (independent replicas) or one LFA shared by all learners
 * (synchronous mini-batch rule; N=1 == the reference rule) */
typedef enum { RSRL_W_PER_ENV = 0, RSRL_W_SHARED = 1 } rsrl_weight_mode;
typedef enum { RSRL_W_F32 = 0, RSRL_W_BF16 = 1 } rsrl_weight_dtype;
/* multi-rank shared-W: the per-batch-step exchange of the (F x A) weight delta (no reference counterpart)
 *   RCCL : ncclAllReduce(sum) on the ctx's stream (one process per GPU, any topology)
 *   PEER : one-hop peer-write -- every rank stores its delta into a slot of every other rank's receive buffer
 *          (hipIpc-mapped memory: xGMI stores across GPUs) and each rank sums the slots in rank order: deterministic,
 *          ring-free, one fabric hop (single node)
 *   AUTO : (the default) decided when the exchange is attached: rsrl_hip_comm_init makes it RCCL, rsrl_hip_peer_export makes it PEER,
 *          rsrl_hip_group_create takes PEER whenever every device of the group can access every other one's memory (one hop over xGMI
 *          beats a ring of latency-bound all-reduces at 432 B; the persistent kernel exchanges inside its one launch) and RCCL, the
 *          any-topology fallback, otherwise.  rsrl_hip_can_access_peer lets a multi-process host make the same choice. */
typedef enum { RSRL_EXCHANGE_RCCL = 0, RSRL_EXCHANGE_PEER = 1, RSRL_EXCHANGE_AUTO = 2 } rsrl_exchange;

typedef struct rsrl_hip_ctx rsrl_hip_ctx;

/* Everything the reference spreads over its constructors
 *   MountainCar::default(), Fourier::from_space(n, space).with_bias(),
 *   LFA::vector(basis, SGD(lr), n_actions), make_shared, Greedy::new /
 *   EpsilonGreedy::new / Softmax::new, QLearning{q_func, gamma} ...
 *   (rsrl/examples/q_learning.rs:19-32)                                      */
typedef struct {
    uint32_t struct_size;        /* = sizeof(rsrl_hip_config); checked                      */
    int32_t  device;             /* HIP device ordinal                                       */
    int32_t  domain;             /* rsrl_domain                                              */
    int32_t  basis;              /* rsrl_basis                                               */
    int32_t  order;              /* Fourier order n: F = (n+1)^D                             */
    int32_t  n_tilings;          /* tile coding: T tilings ...                               */
    int32_t  tiles_per_dim;      /*   ... x B^D cells: F = T*B^D                             */
    int32_t  algo;               /* rsrl_algo                                                */
    int32_t  policy;             /* rsrl_policy (behaviour policy; also SARSA's / ExpectedSARSA's) */
    int32_t  weight_mode;        /* rsrl_weight_mode                                         */
    int32_t  weight_dtype;       /* rsrl_weight_dtype (storage; arithmetic is always f32)    */
    uint32_t max_episode_steps;  /* 0 = unbounded (examples/q_learning.rs:40); else cap + auto-reset
                                    (examples/greedy_gq.rs:46 uses 1000)                     */
    int64_t  n_envs;             /* learners owned by this ctx                                */
    int64_t  env_offset;         /* global id of local learner 0: RNG streams are keyed by the
                                    GLOBAL id, so results do not depend on the sharding       */
    uint64_t seed;               /* StdRng::seed_from_u64 analogue (q_learning.rs:22)        */
    double   gamma;              /* QLearning.gamma etc.                                      */
    double   lr;                 /* SGD(lr)                                                   */
    double   alpha;              /* ExpectedSARSA.alpha (expected_sarsa.rs:26,64)             */
    double   epsilon;            /* EpsilonGreedy.epsilon (pub field, epsilon_greedy.rs:19)  */
    double   tau;                /* Softmax.tau (softmax.rs:52); |tau| < 1e-7 is rejected (:63-66).  POSITIVE only: the reference admits any
                                    non-zero tau, this library refuses tau < 0 with RSRL_HIP_EINVAL -- the kernels evaluate
                                    exp((q - max q) / tau), which overflows fp32 for tau < 0 once (max q - min q) / |tau| > 88.7 */
    uint32_t steps_per_launch;   /* fuse depth of rsrl_hip_train (0 = library default: 4096 for the register-resident loops,
                                    256 for the memory-resident and wave-family ones). 1 = one batch-step per launch:
                                    the ctx then keeps W learner-major and streams it once per step (the 608 B/env-step
                                    formulation), replayed as a hipGraph; results are bit-identical for every depth */
    int32_t  trace;              /* rsrl_trace (lambda agents)                                */
    void*    stream;             /* hipStream_t to run on; NULL = ctx-owned stream           */
    double   lambda;             /* Trace::{accumulating,replacing,dutch}(dim, gamma, lambda) (examples/sarsa_lambda.rs:37);
                                    the lambda agents step with `alpha` and bypass SGD(lr) (fa/linear.rs:184-196) */
    double   lr_td;              /* GreedyGQ: SGD rate of fa_td (examples/greedy_gq.rs:27 uses 0.001 next to SGD(0.1) for fa_q) */
    /* ---- ABI 4 (struct_size-versioned: a caller built against ABI 3 passes the shorter struct and gets the defaults) ---- */
    int32_t  agent_policy;       /* the policy OWNED BY THE AGENT: SARSA{q_func, policy, gamma} draws its inner a' from it
                                    (sarsa.rs:35-41,61), ExpectedSARSA{.., policy, ..} takes its expectation under it
                                    (expected_sarsa.rs:22-29,52-58), SARSALambda likewise (sarsa_lambda.rs:37-44).
                                    -1 (default) = the behaviour policy object itself (the examples share one policy through
                                    make_shared); otherwise an rsrl_policy with its own parameters below, e.g. a Greedy
                                    target under an EpsilonGreedy behaviour = off-policy ExpectedSARSA                   */
    int32_t  exchange;           /* rsrl_exchange: how ranks exchange the shared-W delta (rsrl_hip_comm_init)            */
    double   agent_epsilon;      /* EpsilonGreedy.epsilon of the agent's policy                                          */
    double   agent_tau;          /* Softmax.tau of the agent's policy; positive only, as `tau`                           */
    double   sigma;              /* QSigma.sigma in [0, 1]: 1 = SARSA-like sampling, 0 = tree backup (q_sigma.rs:66-72)          */
    int32_t  n_steps;            /* QSigma: Backup::new(n_steps), 1..32 (q_sigma.rs:94-104).  RSRL_ILSTD / RSRL_ILSTD_ACTOR_CRITIC: iLSTD's n_updates, the
                                    rounds of solve() per transition, 1..32                                                      */
    int32_t  peer_timeout_ms;    /* ABI 5 (was reserved0): bound of every in-kernel wait for a peer / block of the shared-W exchange, in
                                    milliseconds; 0 = RSRL_PEER_TIMEOUT_MS from the environment, else 4000.  Make it longer than the
                                    longest time one rank may spend away from the others (a rollout, a checkpoint) */
    /* ---- ABI 6 ---- */
    double   epsilon_decay;      /* the reference drivers' epsilon schedule, `agent.policy.epsilon *= 0.995` once per EPISODE of the learner
                                    (examples/sarsa_lambda.rs:48-75, :68; the pub field epsilon_greedy.rs:19).  1.0 (default) = no
                                    schedule: one epsilon for the whole ctx (rsrl_hip_set_epsilon).  In (0, 1): EpsilonGreedy.epsilon is
                                    a field of every LEARNER; whenever an episode of learner i ends (terminal transition or step cap),
                                    after that episode's last handle and before the next episode's initial sample,
                                    eps_i <- max(eps_i * epsilon_decay, epsilon_min).  One learner reproduces the reference loop's
                                    schedule step for step.  The agent's policy follows when it IS the behaviour policy object
                                    (agent_policy = -1, as in the example).  Needs policy = RSRL_EPSILON_GREEDY, per-learner weights and a
                                    fused driver loop: the one-step agents and SARSALambda / QLambda on a register-family Fourier basis,
                                    or any one-step agent on tile coding / a generic Fourier order.
                                    Precision: the per-learner field is fp32 and eps * decay is rounded to fp32 once per episode, where the
                                    reference decays an f64 field: gen_bool's threshold (eps * 2^24, truncated) can differ from the f64
                                    schedule's by a few units after many episodes (relative 6e-8 per episode at most; ~1e-4 of a threshold of
                                    1.7e6 after 1 000 episodes) -- bit parity of the schedule is against the oracle's f32 instantiation, the f64
                                    oracle is matched to that tolerance (tests/test_gpu_round4.py). */
    double   epsilon_min;        /* floor of the schedule (0 = none) */
} rsrl_hip_config;
/* size of the ABI 3 struct: the oldest layout rsrl_hip_create accepts */
#define RSRL_HIP_CONFIG_SIZE_V3 ((uint32_t)offsetof(rsrl_hip_config, agent_policy))

/* per-call statistics of rsrl_hip_train (the println! / Response{error} of the
 * reference drivers, examples/q_learning.rs:54, control/td/q_learning.rs:17-20) */
typedef struct {
    uint64_t env_steps;            /* n_steps * n_envs                                        */
    uint64_t episodes;             /* episodes finished (terminal or step cap)                */
    uint64_t episodes_truncated;   /*   ... of which ended by the step cap                    */
    uint64_t sum_episode_steps;    /* sum of lengths of the finished episodes                 */
    double   sum_abs_td_error;     /* sum |delta|                                             */
    double   sum_reward;
} rsrl_hip_stats;

int         rsrl_hip_abi_version(void);
/* number of visible HIP devices (>= 0) or a negative status */
int         rsrl_hip_device_count(void);
const char* rsrl_hip_last_error(void);
/* README example values: MountainCar, Fourier(5), QLearning, gamma 0.9, SGD(0.001), Greedy */
int rsrl_hip_config_init(rsrl_hip_config* cfg);

int rsrl_hip_create(const rsrl_hip_config* cfg, rsrl_hip_ctx** out);
int rsrl_hip_destroy(rsrl_hip_ctx* ctx);
int rsrl_hip_sync(rsrl_hip_ctx* ctx);

/* Space queries: Domain::state_space().dim(), action_space().card(), basis.n_features()
 *   (examples/q_learning.rs:20; Parameterised::weights_dim, params/mod.rs:128) */
int rsrl_hip_state_dim(const rsrl_hip_ctx* ctx);
int rsrl_hip_n_actions(const rsrl_hip_ctx* ctx);
/* columns of the weight matrix: n_actions for the control agents (VectorLFA), 1 for TD / TDLambda (ScalarLFA,
 * Parameterised::weights_dim = (F, 1), fa/linear.rs:201-203) */
int rsrl_hip_n_outputs(const rsrl_hip_ctx* ctx);
/* columns of the policy's own weight matrix (rsrl_hip_get/set_policy_weights): n_actions for the Gibbs actors, 2 for RSRL_BETA (alpha's, beta's);
 * 0 for the agents whose policy reads Q */
int rsrl_hip_n_policy_outputs(const rsrl_hip_ctx* ctx);
int rsrl_hip_n_features(const rsrl_hip_ctx* ctx);
/* rows of the weight matrix (rsrl_hip_get/set_weights carry f32[n_weight_rows][n_outputs]): 3 n_features for RSRL_NAC and (n_actions + 1)
 * n_features for RSRL_GIBBS_NAC, whose critic's basis is the stable compatible basis (SCB::n_features, fa/linear.rs:79-103); n_features on every
 * other ctx */
int rsrl_hip_n_weight_rows(const rsrl_hip_ctx* ctx);
int64_t rsrl_hip_n_envs(const rsrl_hip_ctx* ctx);
/* state_space() bounds: mountain_car/discrete.rs:97-99, cart_pole.rs:112-118, acrobot.rs:143-149 */
int rsrl_hip_state_bounds(const rsrl_hip_ctx* ctx, double* lo /*[D]*/, double* hi /*[D]*/);
/* action_space() bounds of a continuous domain: (-1, 1) on RSRL_CONTINUOUS_MOUNTAIN_CAR (mountain_car/continuous.rs); EINVAL on the domains whose
 * actions are indices (rsrl_hip_n_actions) */
int rsrl_hip_action_bounds(const rsrl_hip_ctx* ctx, double* lo, double* hi);

/* per-episode `Domain::default()` + initial `policy.sample(rng, env.emit().state())`
 *   examples/q_learning.rs:37-38 -- for every learner of the ctx */
int rsrl_hip_reset(rsrl_hip_ctx* ctx);

/* Domain::emit (state part)                         rsrl_domains/src/lib.rs:430 */
int rsrl_hip_get_states(rsrl_hip_ctx* ctx, float* states /*[D][N]*/);
int rsrl_hip_set_states(rsrl_hip_ctx* ctx, const float* states /*[D][N]*/);
/*   (set_states: the array must hold finite values within 1000 widths of each dimension's bounds, else EINVAL and the ctx is untouched -- the reference's
 *    wrap! macro, rsrl_domains/src/macros.rs:14-24, loops without end on an infinite angle; a HOST array is checked on the host, a DEVICE array on the
 *    device by the same rule (ABI 9: it used to be clamped silently, NaN passing)) */
/*   (HIVTreatment: the states are the observations; set_states sets every hidden component to pow(10.0, (double)obs) -- inside (-5, 8) the exact
 *    inverse of the observation, a clipped component (-5 or 8) cannot be inverted -- and requires every value within [-5, 8]) */
/* HIVTreatment's hidden states, f64[6][N] (learner fastest), host or device memory.  set: the observations become emit() of the given states.
 * EINVAL ("domain has no hidden state") on the other domains. */
int rsrl_hip_get_hidden_states(rsrl_hip_ctx* ctx, double* y /*[6][N]*/);
int rsrl_hip_set_hidden_states(rsrl_hip_ctx* ctx, const double* y /*[6][N]*/);
int rsrl_hip_get_actions(rsrl_hip_ctx* ctx, int32_t* actions /*[N]*/);
int rsrl_hip_set_actions(rsrl_hip_ctx* ctx, const int32_t* actions /*[N]*/);
/* ---- f32 actions: the twins of the int32 calls for a ctx on a continuous domain (RSRL_CONTINUOUS_MOUNTAIN_CAR), with their conventions -- host or
 * device pointers, the same asynchrony, the same meaning of the step counter.  A HOST array of actions is validated (EINVAL unless every value is
 * finite; rsrl_hip_set_actions_f32: inside the action bounds too), a DEVICE array is clamped by the kernels.  (RSRL_GAUSSIAN: an action is any
 * finite f32 -- a sample is not bounded --, so rsrl_hip_set_actions_f32 checks a host array for finite values only and clamps nothing; a device
 * array is the caller's.)  On such a ctx the int32 calls --
 * rsrl_hip_get/set_actions, _domain_step, _handle, _policy_sample, _policy_mode -- are ESTATE; on every other ctx the f32 calls are.
 *   rsrl_hip_domain_step_f32      rsrl_hip_domain_step            rsrl_hip_policy_sample_f32   rsrl_hip_policy_sample (states == NULL as there)
 *   rsrl_hip_handle_f32           rsrl_hip_handle                 rsrl_hip_policy_mode_f32     rsrl_hip_policy_mode
 * rsrl_hip_policy_params is beta.rs's pub compute_alpha / compute_beta, rsrl_hip_policy_pdf its Function<(S, A)> (the density, of the action
 * clamped to [2^-24, 1 - 2^-24]); both read-only, state i against learner i's columns.  With RSRL_GAUSSIAN rsrl_hip_policy_params is
 * compute_mean / compute_stddev (gaussian/mod.rs:56-68): alpha_out receives mu, beta_out sd; rsrl_hip_policy_pdf is the normal density of the action as given.
 * On an RSRL_NAC ctx (the loop of nac_beta.rs: the domain sees 2a - 1, the agent a) rsrl_hip_domain_step_f32 takes explicit actions literally, as the
 * DOMAIN's, and with actions == NULL applies the loop's 2a - 1 to the ctx's pending actions (the agent's); rsrl_hip_handle_f32 is critic.handle.
 * With RSRL_GAUSSIAN (the loop of nac.rs) there is no mapping: actions == NULL steps on the pending actions as they are, which the domain clips.
 * rsrl_hip_q_evaluate_f32 is Function<(S, A)>::evaluate of RSRL_NAC's critic, Q(s_i, a_i) = <w_i, psi(s_i, a_i)> against learner i's w and columns
 * (read-only; the action is clamped as above -- RSRL_GAUSSIAN: taken as it is); rsrl_hip_nac_update is NAC::handle(()) (control/nac.rs:47-59) for the learners whose mask byte is
 * non-zero (mask == NULL: every learner): norm_out, which may be NULL, receives Response.norm, 0 for a learner left out.  Both are ESTATE on
 * every other algo */
int rsrl_hip_get_actions_f32(rsrl_hip_ctx* ctx, float* actions /*[N]*/);
int rsrl_hip_set_actions_f32(rsrl_hip_ctx* ctx, const float* actions /*[N]*/);
int rsrl_hip_domain_step_f32(rsrl_hip_ctx* ctx, const float* actions, float* from_states, float* next_states, float* rewards, uint8_t* terminal);
int rsrl_hip_handle_f32(rsrl_hip_ctx* ctx, const float* from_states, const float* actions, const float* rewards, const float* to_states,
                        const uint8_t* terminal, int64_t M, float* td_error_out);
int rsrl_hip_policy_sample_f32(rsrl_hip_ctx* ctx, const float* states, int64_t M, float* actions_out);
int rsrl_hip_policy_mode_f32(rsrl_hip_ctx* ctx, const float* states, int64_t M, float* actions_out);
int rsrl_hip_policy_params(rsrl_hip_ctx* ctx, const float* states, int64_t M, float* alpha_out, float* beta_out);
int rsrl_hip_policy_pdf(rsrl_hip_ctx* ctx, const float* states, const float* actions, int64_t M, float* out);
int rsrl_hip_q_evaluate_f32(rsrl_hip_ctx* ctx, const float* states /*[D][M]*/, const float* actions /*[M]*/, int64_t M, float* q_out /*[M]*/);
int rsrl_hip_nac_update(rsrl_hip_ctx* ctx, const uint8_t* mask /*[N], NULL = every learner*/, float* norm_out /*[N], may be NULL*/);
/* (ABI 8) The rest of a learner's state between two driver calls, so that a run can be carried into another ctx EXACTLY (with the checkpoint of
 * rsrl_hip_save_weights, the states and the actions above):
 *   - the steps every learner's current episode has taken (what the driver loop's `for j in 0..step_limit` counter would hold,
 *     rsrl/src/lib.rs:82-88 as the examples drive it): without it a resumed run counts its step cap from zero;
 *   - the register-family loops (one-step agents on MountainCar Fourier 1-5, CartPole / Acrobot Fourier 1) CARRY Q(s,.) of the current state from
 *     launch to launch as the fused loop left it (the pre-update value plus the rank-1 term of the last update).  rsrl_hip_set_states / _set_weights /
 *     _load_weights drop it and the next launch evaluates Q(s,.) from the weights: equal in exact arithmetic, not always in the last bit -- enough to
 *     part a Softmax / ExpectedSARSA run from the uninterrupted one.  get: *valid = 1 and q filled while something is carried, 0 (q untouched)
 *     otherwise -- always 0 for the families that evaluate Q from the weights every step; set (AFTER the states and weights are in place): the next
 *     launch continues from it.  EINVAL for a ctx whose kernels carry nothing. */
int rsrl_hip_get_episode_steps(rsrl_hip_ctx* ctx, uint32_t* steps /*[N]*/);
int rsrl_hip_set_episode_steps(rsrl_hip_ctx* ctx, const uint32_t* steps /*[N]*/);
/* (RSRL_GRADIENT_MC, RSRL_LSTD, RSRL_LSTD_LAMBDA: set_episode_steps refuses a value above max_episode_steps with EINVAL and changes nothing -- the kernel indexes the record by it.)
 * RSRL_GRADIENT_MC's (and RSRL_LSTD's, RSRL_LSTD_LAMBDA's) open episodes, cap = max_episode_steps rows: learner i's record is rows 0 .. episode_steps[i]-1 of its column, row k holding
 * transition k's `from` state and reward.  get writes NaN in the rows past that; set installs both arrays whole (what lies past a learner's
 * episode_steps is never read).  Host or device arrays.  ESTATE on every other agent */
int rsrl_hip_get_episode_record(rsrl_hip_ctx* ctx, float* states /*[cap][D][N]*/, float* rewards /*[cap][N]*/);
int rsrl_hip_set_episode_record(rsrl_hip_ctx* ctx, const float* states /*[cap][D][N]*/, const float* rewards /*[cap][N]*/);
int rsrl_hip_get_q_carry(rsrl_hip_ctx* ctx, float* q /*[A][N]*/, int32_t* valid);
int rsrl_hip_set_q_carry(rsrl_hip_ctx* ctx, const float* q /*[A][N]*/);

/* ---- The trait-granular loop (examples/q_learning.rs:40-52), one call per trait method, every learner of the ctx:
 *
 *        rsrl_hip_domain_step(ctx, act, from, to, rew, term);          t  = env.transition(a)
 *        rsrl_hip_handle(ctx, from, act, rew, to, term, n_envs, td);        agent.handle(&t)
 *        rsrl_hip_domain_reset(ctx, term);                                  terminal -> a new episode (q_learning.rs:37, :47-51)
 *        rsrl_hip_policy_sample(ctx, NULL, n_envs, act);               a' = policy.sample(rng, env.emit().state())
 *
 *   reproduces the reference's call pattern -- every action value evaluated afresh from the weights -- bit for bit against the CPU oracle's
 *   reference-order loop (tests/test_gpu_trait_loop.py), on every basis / agent with a handle.  A ctx created with steps_per_launch = 1 on a
 *   register-family Fourier basis (MountainCar order 1 / 3 / 5, CartPole / Acrobot order 1) with per-learner f32 weights and a one-step agent
 *   (QLearning, SARSA, ExpectedSARSA, PAL) keeps W learner-major and serves the loop as an HBM stream (rsrl_amd/csrc/kernels_trait.hpp): handle
 *   makes ONE pass over the learners' weights and hands Q(s',.) under the updated weights over to the sample that follows (a cache keyed by the
 *   state itself: a hit returns the bits a fresh evaluation returns).  With DEVICE arrays on a CTX-OWNED stream such a ctx ACCEPTS the four
 *   calls above and launches them as one kernel when they arrive in this order on the same arrays; any other call launches the accepted ones
 *   first, one kernel each -- same results, same order; as with rsrl_hip_train's coalescing, acceptance is not completion: rsrl_hip_sync (or
 *   any call that returns data to the host) completes them.  On a caller-supplied stream every call enqueues its own kernel before it returns.
 *   RSRL_NO_TRAIT_DEFER=1 in the environment when the ctx is created switches the deferral off (A/B runs).  (ABI 9)
 *
 * Domain::transition                                rsrl_domains/src/lib.rs:436-446
 * Steps every env of the ctx with `actions` (NULL: the ctx's pending actions).  Outputs are
 * optional (NULL to skip).  The ctx's env state becomes s'; no auto-reset. */
int rsrl_hip_domain_step(rsrl_hip_ctx* ctx, const int32_t* actions,
                         float* from_states, float* next_states, float* rewards, uint8_t* terminal);
/* `MountainCar::default()` for the envs whose mask byte is non-zero (NULL: all) */
int rsrl_hip_domain_reset(rsrl_hip_ctx* ctx, const uint8_t* mask);

/* Function<(S,)>::evaluate for VectorLFA: Q(s,.) = W^T phi(s)      rsrl/src/fa/linear.rs:303-311
 * state m is evaluated with learner m's weights (or the shared weights).  An RSRL_GIBBS_NAC ctx writes f32[n_actions][M] although its
 * n_outputs is 1: row b = Q(s_m, b) of the critic over the stable compatible basis, against learner m's w and theta. */
int rsrl_hip_q_evaluate(rsrl_hip_ctx* ctx, const float* states /*[D][M]*/, int64_t M, float* q_out /*[A][M]*/);
/*   prediction agents: the same call is Function<(S,)>::evaluate of the ScalarLFA (fa/linear.rs:213-221), q_out = V f32[1][M];
 *   find_max / policy_mode / policy_probs / policy_sample / rollout_greedy return RSRL_HIP_ESTATE for them (no Q function). */
/* Enumerable::find_max (ties -> last index)                         rsrl/src/core.rs:96-105 */
int rsrl_hip_q_find_max(rsrl_hip_ctx* ctx, const float* states, int64_t M, int32_t* idx_out, float* val_out);
/* Enumerable::find_min (the minimum; ties -> last index)            rsrl/src/core.rs:86-94 */
int rsrl_hip_q_find_min(rsrl_hip_ctx* ctx, const float* states, int64_t M, int32_t* idx_out, float* val_out);
/* Enumerable::expected_value(args, ps) = fold(0.0, acc + Q(s,a)*p_a) rsrl/src/core.rs:107-116; probs f32[A][M], out f32[M] */
int rsrl_hip_q_expected_value(rsrl_hip_ctx* ctx, const float* states, int64_t M, const float* probs, float* out);
/* basis.project(s): dense features phi f32[F][M] (Fourier) -- lfa Basis::project */
int rsrl_hip_project(rsrl_hip_ctx* ctx, const float* states, int64_t M, float* phi_out /*[F][M]*/);
/* tile coding: active indices int32[T][M] */
int rsrl_hip_tile_indices(rsrl_hip_ctx* ctx, const float* states, int64_t M, int32_t* idx_out /*[T][M]*/);

/* Handler<&Transition>::handle for QLearning / SARSA / ExpectedSARSA
 *   control/td/q_learning.rs:51-71, sarsa.rs:53-75, expected_sarsa.rs:45-66
 * td_error_out (optional) = Response.error (q_learning.rs:17-20).  Each call counts as one batch-step: it advances
 * rsrl_hip_step_count, the counter that addresses the agent-side random draws (SARSA's inner policy sample,
 * sarsa.rs:61; bf16 stochastic rounding), exactly as one step of rsrl_hip_train does.
 * With device arrays only the call is asynchronous on the ctx's stream (ABI 9; it used to synchronise); host arrays are staged and the call
 * returns when they have been consumed / filled. */
int rsrl_hip_handle(rsrl_hip_ctx* ctx, const float* from_states, const int32_t* actions,
                    const float* rewards, const float* to_states, const uint8_t* terminal,
                    int64_t M, float* td_error_out);
/* Handler<&Batch>::handle (rsrl_domains/src/lib.rs:210; reinforce.rs, baseline_reinforce.rs) for every learner of a REINFORCE ctx: learner i's batch
 * is rows 0 .. lengths[i]-1 of its column (lengths[i] = 0: no batch, lengths[i] <= T), handled first to last with its own g from 0.  returns_out
 * (optional) receives g at each handled transition and NaN in the rows past a learner's length.  theta_b and the carried g are not touched.  Like
 * rsrl_hip_handle, one call is one batch-step (it advances rsrl_hip_step_count): the trait loop
 *     domain_step -> (append the transition) -> handle_batch(lengths = episode length of the learners whose episode just ended, else 0)
 *     -> domain_reset(ended) -> policy_sample(NULL)
 * runs on the driver loop's draws.  Host or device arrays, as rsrl_hip_handle (host actions of the handled rows and host lengths are validated,
 * device ones clamped).
 * RSRL_GRADIENT_MC: Handler<&Trajectory>::handle for every learner.  Row k of states is transition k's `from`, learner i's trajectory is rows
 * 0 .. lengths[i]-1, visited LAST TO FIRST; actions may be NULL and are ignored when given.  returns_out receives `sum` at each handled row and NaN
 * past a learner's length; a learner of length 0 keeps its bytes.  The ctx's own open record is not touched.  The trait loop is the one above.
 * ESTATE on every other agent. */
int rsrl_hip_handle_batch(rsrl_hip_ctx* ctx, int64_t T, const float* states /*[T][D][N]*/, const int32_t* actions /*[T][N]*/,
                          const float* rewards /*[T][N]*/, const uint32_t* lengths /*[N]*/, float* returns_out /*[T][N], optional*/);
/* RSRL_LSTD / RSRL_LSTD_LAMBDA / RSRL_LAMBDA_LSPE (last to first): Handler<&Batch>::handle for every learner, on whole transitions.  Learner i's batch is rows 0 .. lengths[i]-1 of its
 * column; any row may be terminal; LSTD walks the rows first to last, LSTDLambda last to first, and both end in solve().  lengths[i] = 0 means no
 * call: the learner keeps its bytes and no solve runs.  actions are not read.  td_out receives the diagnostic r + gamma V(s') - V(s) (terminal:
 * r - V(s)) with theta as it stood before the solve at each handled row, NaN past a learner's length.  The ctx's own open record is not touched.
 * The conventions are rsrl_hip_handle_batch's: host or device arrays (host lengths validated, device ones clamped), one call is one batch-step, and
 *     domain_step -> (append the transition) -> handle_transitions(lengths = episode length of the learners whose episode just ended, else 0)
 *     -> domain_reset(ended) -> policy_sample(NULL)
 * runs on the driver loop's draws and leaves its bits.  ESTATE on every other agent; rsrl_hip_handle and rsrl_hip_handle_batch are ESTATE on these */
int rsrl_hip_handle_transitions(rsrl_hip_ctx* ctx, int64_t T, const float* from_states /*[T][D][N]*/, const int32_t* actions /*[T][N], may be NULL, ignored*/,
                                const float* rewards /*[T][N]*/, const float* to_states /*[T][D][N]*/, const uint8_t* terminal /*[T][N]*/,
                                const uint32_t* lengths /*[N]*/, float* td_out /*[T][N], optional*/);

/* Policy::sample / Policy::mode / Function<(S,)> of the policy (action probabilities)
 *   policies/mod.rs:65-78; greedy.rs:30-44,77-83; epsilon_greedy.rs:38-45,74-82;
 *   softmax.rs:74-82,131-143; random.rs:19-48 (mode of Random: RSRL_HIP_EINVAL, random.rs:47 panics) */
/* states == NULL (ABI 9; M must be n_envs): policy.sample(rng, env.emit().state()) for the ctx's OWN envs -- the driver loop's behaviour sample
 *   (examples/q_learning.rs:38, :45).  It draws what batch-step rsrl_hip_step_count() - 1 of rsrl_hip_train draws (before the first handle: the initial
 *   sample's stream, as rsrl_hip_reset), and the actions also become the ctx's pending ones.  With explicit states the draws are a stream of their own,
 *   addressed by the number of such calls made on the ctx. */
int rsrl_hip_policy_sample(rsrl_hip_ctx* ctx, const float* states, int64_t M, int32_t* actions_out);
int rsrl_hip_policy_mode(rsrl_hip_ctx* ctx, const float* states, int64_t M, int32_t* actions_out);
int rsrl_hip_policy_probs(rsrl_hip_ctx* ctx, const float* states, int64_t M, float* probs_out /*[A][M]*/);
/* Function<(S, A)> of the policy: the probability of action a in state s for Greedy / EpsilonGreedy / Random
 *   (greedy.rs:46-60, epsilon_greedy.rs:49-63, random.rs:28-32) and -- faithfully -- the raw action value Q(s, a) for Softmax
 *   (softmax.rs:84-92 forwards to the approximator).  actions int32[M] in [0, A), prob_out f32[M]. */
int rsrl_hip_policy_prob(rsrl_hip_ctx* ctx, const float* states, const int32_t* actions, int64_t M, float* prob_out);
/* the pub field EpsilonGreedy.epsilon (decayed by drivers, examples/sarsa_lambda.rs:68); with config.epsilon_decay it sets every
 * learner's field */
int rsrl_hip_set_epsilon(rsrl_hip_ctx* ctx, double epsilon);
/* every learner's current epsilon, f32[N] (config.epsilon_decay: each learner's own field; otherwise N copies of the ctx's) */
int rsrl_hip_get_epsilons(rsrl_hip_ctx* ctx, float* eps_out /*[N]*/);

/* Parameterised::weights / weights_view_mut               rsrl/src/params/mod.rs:116-134
 * w is row-major f32[F][A] (ndarray Array2 (F, A), fa/linear.rs:293-301); env_index is
 * ignored in shared mode.  Also the checkpoint hook. */
int rsrl_hip_get_weights(rsrl_hip_ctx* ctx, int64_t env_index, float* w /*[F][A]*/);
int rsrl_hip_set_weights(rsrl_hip_ctx* ctx, int64_t env_index, const float* w /*[F][A]*/);
/* the pub field `trace` of SARSALambda / QLambda (sarsa_lambda.rs:41, q_lambda.rs:40): one learner's eligibility trace,
 * row-major f32[F][A] like the weights */
int rsrl_hip_get_traces(rsrl_hip_ctx* ctx, int64_t env_index, float* z /*[F][A]*/);
int rsrl_hip_set_traces(rsrl_hip_ctx* ctx, int64_t env_index, const float* z /*[F][A]*/);
/* the pub field `fa_td` of GreedyGQ (greedy_gq.rs:52): one learner's second approximator, row-major f32[F][A]; RSRL_GTD2's fa_w and RSRL_TDC's
 * td_est (gtd2.rs:29, tdc.rs:43): the second weight column w, f32[F][1].  ESTATE on every other agent */
int rsrl_hip_get_td_weights(rsrl_hip_ctx* ctx, int64_t env_index, float* v /*[F][A]*/);
int rsrl_hip_set_td_weights(rsrl_hip_ctx* ctx, int64_t env_index, const float* v /*[F][A]*/);
/* the pub field `policy` of ActorCritic (ac.rs:61): the Gibbs actor's weights theta of one learner, row-major f32[F][A] like the weights
 * (RSRL_TD_ACTOR_CRITIC: f32[F][n_actions], while its weights are V's f32[F][1]).
 * ESTATE on every ctx that is not an ActorCritic one (whose get/set_traces and get/set_td_weights are ESTATE in turn) */
int rsrl_hip_get_policy_weights(rsrl_hip_ctx* ctx, int64_t env_index, float* theta /*[F][A]*/);
int rsrl_hip_set_policy_weights(rsrl_hip_ctx* ctx, int64_t env_index, const float* theta /*[F][A]*/);
/* REINFORCE / BaselineREINFORCE: the open episode's state, so that a caller can save and restore it exactly (as get/set_q_carry): the behaviour
 * snapshot theta_b of one learner (row-major f32[F][A], the policy theta when its episode began) and every learner's running return g.
 * ESTATE on every other agent */
int rsrl_hip_get_behaviour_weights(rsrl_hip_ctx* ctx, int64_t env_index, float* theta_b /*[F][A]*/);
int rsrl_hip_set_behaviour_weights(rsrl_hip_ctx* ctx, int64_t env_index, const float* theta_b /*[F][A]*/);
int rsrl_hip_get_return_carry(rsrl_hip_ctx* ctx, float* g /*[N]*/);
int rsrl_hip_set_return_carry(rsrl_hip_ctx* ctx, const float* g /*[N]*/);
/* RecursiveLSTD / iLSTD (and the iLSTD ActorCritic's critic): the exact f64 state of one learner -- theta, the matrix (row-major: C for RecursiveLSTD, A for iLSTD) and iLSTD's mu
 * (may be NULL: not read or written; ignored by RecursiveLSTD).  Host or device arrays.  ESTATE on every other agent */
int rsrl_hip_get_lstd_state(rsrl_hip_ctx* ctx, int64_t env_index, double* theta /*[F]*/, double* mat /*[F][F]*/, double* mu /*[F], iLSTD only, may be NULL*/);
int rsrl_hip_set_lstd_state(rsrl_hip_ctx* ctx, int64_t env_index, const double* theta /*[F]*/, const double* mat /*[F][F]*/,
                            const double* mu /*[F], iLSTD only, may be NULL*/);
/* LSTD / LSTDLambda / LambdaLSPE: the exact f64 state of one learner -- theta, A (row-major), b, LSTDLambda's z (may be NULL: not read or written;
 * ignored by LSTD) -- and its count of abandoned solves.  RSRL_LAMBDA_LSPE: z[0] = delta and z[1] = rows, an exact integer in 0 .. F; get writes
 * z[2 ..] as 0, set does not read it and refuses any other rows with EINVAL before anything moves.  Host or device arrays.  ESTATE on every other
 * agent */
int rsrl_hip_get_lstd_batch_state(rsrl_hip_ctx* ctx, int64_t env_index, double* theta /*[F]*/, double* A /*[F][F]*/, double* b /*[F]*/,
                                  double* z /*[F], LSTDLambda only, may be NULL*/, uint32_t* singular_solves);
int rsrl_hip_set_lstd_batch_state(rsrl_hip_ctx* ctx, int64_t env_index, const double* theta /*[F]*/, const double* A /*[F][F]*/, const double* b /*[F]*/,
                                  const double* z /*[F], LSTDLambda only, may be NULL*/, const uint32_t* singular_solves);
/* LSTD / LSTDLambda: the agents' public solve() (lstd.rs:40, lstd_lambda.rs:44) for every learner: theta <- A.solve(b) in the library's fixed
 * operation order; A, b and z are not written.  An abandoned solve keeps theta and counts in singular_solves.  RSRL_LAMBDA_LSPE: the agent's
 * solve() exactly as handle ends with it (lambda_lspe.rs:47-62, a PRIVATE function in the reference): the row rule, the relaxed step, the
 * zeroing of A, b, delta and rows.  ESTATE on every other agent */
int rsrl_hip_lstd_solve(rsrl_hip_ctx* ctx);
/* Checkpoint of the approximator(s) (the reference's only persistence story is the optional serde
 * derive on the agents, rsrl/Cargo.toml:26).  The file version follows from the header's aux_kind:
 *   aux_kind                                        written as   payload after the header
 *   0 none                                           2           weights
 *   1 eligibility traces                             2           weights, auxiliary matrix
 *   2 GreedyGQ's fa_td weights                       2           weights, auxiliary matrix
 *   3 QSigma's n-step backups                        3           weights, backups       (version 2 / aux_kind 0 of a QSigma ctx: still read)
 *   4 sparse traces over a shared table              6           weights, sparse lists  (version 5, and version 2 / aux_kind 0: still read)
 *   5 ActorCritic's theta                            7           weights, auxiliary matrix
 *   6 the TD ActorCritic's theta                     8           weights, auxiliary matrix
 *   7 REINFORCE's theta and open episode             9           weights (BaselineREINFORCE only), auxiliary matrix, theta_b, g
 *   8 the LSTD agents' f64 state                     10          f64 theta, matrices, mu
 *   9 the iLSTD ActorCritic's f64 state and theta    10          f64 theta, matrices, mu, auxiliary matrix
 *   10 LSTD / LSTDLambda's f64 state                 10          f64 theta, A, b, z (LSTDLambda), u32 singular_solves
 *   11 the Beta iLSTD ActorCritic's state            10          f64 theta, matrices, mu, the policy's columns
 *   12 NAC's critic and the policy's columns         10          weights (3F rows), the policy's columns
 *   13 GTD2 / TDC: theta and the second column w     10          weights, auxiliary matrix
 *   14 NAC with RSRL_GAUSSIAN: critic and columns    10          weights (3F rows), the policy's columns
 *   15 CACLA: the V learner's w and the columns      10          weights, the policy's columns
 *   16 the continuous TD ActorCritic with RSRL_BETA  10          weights, the policy's columns
 *   17 ... with RSRL_GAUSSIAN                        10          weights, the policy's columns
 * and a ctx with config.epsilon_decay (aux_kind 0 or 1) writes version 4 instead, with f32 eps[N] behind the payload.  No other pairing of
 * version and aux_kind is a file of this library; load refuses it.  Little-endian, serialised field by field (no padding):
 *   offset  0  char magic[8] = "RSRLHIPW"
 *           8  u32  version (the table above)
 *          12  i32  domain, basis, order, n_tilings, tiles_per_dim, weight_mode, F, A (weight columns),
 *                   algo, weight_dtype, aux_kind (0 none, 1 eligibility traces, 2 GreedyGQ's fa_td weights,
 *                   3 QSigma's n-step backups, 4 sparse traces over a shared table, 5 ActorCritic's theta,
 *                   6 the TD ActorCritic's theta, 7 REINFORCE's theta and open episode, 8 the LSTD agents' f64 state,
 *                   9 the iLSTD ActorCritic's f64 state and theta, 10 LSTD / LSTDLambda's f64 state,
 *                   11 the Beta iLSTD ActorCritic's f64 state and policy columns, 12 NAC's critic and policy columns,
 *                   13 GTD2's / TDC's second weight column, 14 the Gaussian NAC's critic and policy columns,
 *                   15 CACLA's V weights and policy columns, 16 / 17 the continuous TD ActorCritic's V weights and its Beta / Gaussian policy
 *                   columns)
 *                                                                                                                 [11 x i32]
 *          56  i64  n_learners (1 in shared mode)
 *          64  u64  step_count
 *          72  n_learners x f32[F][A] weights in the reference's row-major (F, A) order (Parameterised::weights,
 *              params/mod.rs:118), independent of the device layout and storage dtype;
 *              then, if aux_kind is 1, 2 or 5, n_learners x f32[F][A] of the auxiliary matrix (traces / fa_td / the actor's theta; aux_kind 5 is
 *              written as file version 7, which no other configuration reads);
 *              if aux_kind is 6 (file version 8, which no other configuration reads; A = 1, the weights are V's w): n_learners x f32[F][n_actions]
 *              of the actor's theta;
 *              if aux_kind is 7 (file version 9, which no other configuration reads; RSRL_REINFORCE / RSRL_BASELINE_REINFORCE): the weights section
 *              is BaselineREINFORCE's baseline B, and is ABSENT for REINFORCE (no value function); then n_learners x f32[F][A] of theta,
 *              n_learners x f32[F][A] of theta_b, f32 g[N];
 *              if aux_kind is 8 (file version 10, which no other configuration reads; RSRL_RECURSIVE_LSTD / RSRL_ILSTD): the weights section is
 *              ABSENT (theta is f64); then n_learners x f64[F] of theta, n_learners x f64[F][F] of the matrix (C / A, row-major) and, for
 *              iLSTD, n_learners x f64[F] of mu;
 *              if aux_kind is 9 (file version 10 too; RSRL_ILSTD_ACTOR_CRITIC): aux_kind 8's sections of its iLSTD critic (mu included), then
 *              n_learners x f32[F][n_actions] of the actor's theta;
 *              if aux_kind is 10 (file version 10 too; RSRL_LSTD / RSRL_LSTD_LAMBDA): the weights section is ABSENT;
 *              then n_learners x f64[F] of theta, n_learners x f64[F][F] of A (row-major), n_learners x f64[F] of b, for LSTDLambda
 *              n_learners x f64[F] of z, then u32 singular_solves[N].  The open episodes are not in the file (as RSRL_GRADIENT_MC's);
 *              if aux_kind is 19 (file version 10 too; RSRL_LAMBDA_LSPE): aux_kind 10's theta, A and b, then n_learners x f64[2] of (delta, rows),
 *              then u32 singular_solves[N]; a row count that is no integer in 0 .. F is EINVAL at load;
 *              if aux_kind is 11 (file version 10 too; RSRL_ILSTD_ACTOR_CRITIC with RSRL_BETA on RSRL_CONTINUOUS_MOUNTAIN_CAR): aux_kind 8's
 *              sections of its iLSTD critic (mu included), then n_learners x f32[F][2] of the policy's columns (alpha's, beta's);
 *              if aux_kind is 12 (file version 10 too; RSRL_NAC; the header's F is n_features, A = 1): the weights
 *              are the critic's w, n_learners x f32[3F][1], then n_learners x f32[F][2] of the policy's columns;
 *              if aux_kind is 14 (file version 10 too; RSRL_NAC with RSRL_GAUSSIAN): aux_kind 12's sections, the columns the mean's and the
 *              stddev's -- the kind alone tells the two policies' files apart, and neither loads into a ctx of the other;
 *              if aux_kind is 15 (file version 10 too; RSRL_CACLA; A = 1, the weights are the V learner's w): n_learners x f32[F][2] of the
 *              Gaussian policy's columns (the mean's, the stddev's);
 *              if aux_kind is 16 or 17 (file version 10 too; RSRL_CONTINUOUS_TD_ACTOR_CRITIC with RSRL_BETA / RSRL_GAUSSIAN): aux_kind 15's sections,
 *              the columns alpha's and beta's / the mean's and the stddev's;
 *              if aux_kind is 18 (file version 10 too; RSRL_GIBBS_NAC; the header's F is n_features, A = 1): the weights are n_learners x
 *              f32[(n_actions + 1) F][1] of the critic's w, then n_learners x f32[F][n_actions] of the Gibbs policy's theta;
 *              if aux_kind is 13 (file version 10 too; RSRL_GTD2 / RSRL_TDC; A = 1, the weights are theta): n_learners x f32[F][1] of the
 *              second weight column w (fa_w / td_est);
 *              if aux_kind is 3 (file version 3): u32 head[N], u32 len[N], f32 entries[D + 5][n_steps][N] -- every learner's
 *              Backup ring {s, a, q, residual, pi, mu} (q_sigma.rs:30-63), so that a QSigma run with n_steps > 1 resumes
 *              bit-identically too.  A QSigma ctx still reads its configuration's version-2 file without them (aux_kind 0): the backups start empty.
 *              if aux_kind is 4 (file version 6; SARSALambda / QLambda over ONE shared tile-coded table): u64 n_envs, u64 env_offset (whose
 *              learners the lists belong to: a file of another shard is refused as a different configuration), u32 len[N], then for every
 *              learner in turn u32 key[len] (= feature index * A + action) and f32 value[len] -- its sparse trace (params/sparse.rs:13-97),
 *              the tilings' sub-lists one after the other, each in slot order, so that the run resumes bit-identically (the slot order decides
 *              which entry a full sub-list overwrites).  Version 5 (never written any more: no n_envs / env_offset, one list per learner) is still read; its
 *              entries go to the sub-lists of their keys' tilings, and a file with more than 512 / n_tilings entries of one tiling is refused.
 *              A ctx with config.epsilon_decay writes file version 4: everything above, then f32 eps[N], every learner's current
 *              epsilon (the schedule's state), so that a resumed run continues the schedule.
 * load refuses a file whose header does not match the ctx's configuration or whose size is not exactly what the header
 * implies, and stages the data: a failing load leaves the ctx's weights untouched.  A loaded run's LEARNING resumes bit-identically (weights, traces,
 * backups, epsilons, step counter -- with the env states restored through rsrl_hip_set_states / _set_actions, the episodes' step counts through
 * rsrl_hip_set_episode_steps, for the register-family loops, the carried Q(s,.) through rsrl_hip_set_q_carry: ABI 8, and, for HIVTreatment,
 * rsrl_hip_set_hidden_states); the evaluation-rollout draw
 * counter of rsrl_hip_rollout_policy is not part of the file (see there). */
int rsrl_hip_save_weights(rsrl_hip_ctx* ctx, const char* path);
int rsrl_hip_load_weights(rsrl_hip_ctx* ctx, const char* path);
/* same weights broadcast to every learner (per-env mode) */
int rsrl_hip_set_weights_all(rsrl_hip_ctx* ctx, const float* w /*[F][A]*/);

/* The fused driver loop (examples/q_learning.rs:40-52) x n_envs x n_steps with auto-reset
 * on terminal / step cap.  stats_out is a HOST pointer (optional). */
int rsrl_hip_train(rsrl_hip_ctx* ctx, int64_t n_steps, rsrl_hip_stats* stats_out);
/*   Without stats_out the call is ASYNCHRONOUS: it returns once the work is enqueued.  On a CTX-OWNED stream (config.stream
 *   NULL) short calls (a driver loop's 20 batch-steps) that arrive while the stream is still busy are coalesced -- held back and
 *   launched fuse-depth (4096 batch-steps) at a time, when anything observes or changes the ctx (every other entry point,
 *   rsrl_hip_sync included, flushes first), or when a call finds the stream idle.  Results are bit-identical to one launch per
 *   call (the fused loop carries Q(s,.) between launches and addresses the RNG by the batch-step); RSRL_NO_COALESCE=1 in the
 *   environment disables it.  On a caller-supplied stream nothing is ever held back.
 *   Shared dense weights (RSRL_W_SHARED on a register-family Fourier basis, at most one 512-learner block per CU): the whole
 *   call is ONE persistent launch; the ranks of a peer group exchange inside it (RSRL_NO_PERSIST=1: one launch per batch-step).
 *   That kernel needs every block of its grid -- and of its peers' grids -- resident at once.  The library guarantees it: the grid
 *   is checked against the device's occupancy (and once per ctx by a cooperative launch); a peer group decides COLLECTIVELY in
 *   rsrl_hip_peer_connect (ranks that share a device must fit together; RSRL_NO_PERSIST on any rank counts for all), so that no
 *   two ranks ever take different paths; unrelated persistent ctxs of one process take turns on a device.  Whenever the guarantee
 *   cannot be given the per-step path runs instead -- same results, bit for bit.
 *   Launch coalescing contract: steps a call has ACCEPTED but not launched (rsrl_hip_pending_steps) are launched by the next call
 *   on the ctx, whichever it is; a host that stops calling and wants them to run calls rsrl_hip_sync (as with any asynchronous
 *   queue, acceptance is not completion). */
/* batch-steps executed so far by rsrl_hip_train and rsrl_hip_handle (the RNG counter) */
uint64_t rsrl_hip_step_count(const rsrl_hip_ctx* ctx);
/* batch-steps rsrl_hip_train has accepted but not enqueued yet (launch coalescing); always 0 on a caller-supplied stream */
int64_t rsrl_hip_pending_steps(const rsrl_hip_ctx* ctx);

/* Domain::rollout with the closure s -> policy.mode(s) and Some(step_limit), + n_states
 *   rsrl_domains/src/lib.rs:448-479, :340; one fresh default env per learner, the ctx's
 *   training envs are untouched.  step_limit >= 1.
 *   step_limit == 0 (all three rollout calls): Domain::rollout(.., None), lib.rs:469-476 -- no limit, the trajectory ends at the first
 *   Terminal observation.  A device loop needs a bound, so config.max_episode_steps (> 0, else RSRL_HIP_EINVAL) caps it at that many
 *   transitions: outputs are sized as for step_limit = max_episode_steps + 1, and a trajectory that terminates within the cap
 *   (terminal_out = 1) is exactly the reference's unbounded one.  (ABI 7) */
int rsrl_hip_rollout_greedy(rsrl_hip_ctx* ctx, int64_t step_limit,
                            uint32_t* n_states_out /*[N]*/, float* total_reward_out /*[N]*/);
/* The same rollout for learners 0..M-1 with the Trajectory itself (rsrl_domains/src/lib.rs:334-409): every output but
 * n_states_out is optional.
 *   states_out   f32[step_limit][D][M]     row 0 = Trajectory.start, row k = the observation of steps[k-1]
 *   actions_out  i32[step_limit-1][M]      steps[k].1        rewards_out f32[step_limit-1][M]   steps[k].2
 *   terminal_out u8[M]                     the last observation is Observation::Terminal
 * Rows past a learner's n_states are zero (host buffers) / untouched (device buffers).  Trajectory::total_reward (:391) =
 * total_reward_out, n_states (:340) = n_states_out, n_transitions = n_states - 1. */
int rsrl_hip_rollout_trajectory(rsrl_hip_ctx* ctx, int64_t step_limit, int64_t M, uint32_t* n_states_out, float* total_reward_out,
                                float* states_out, int32_t* actions_out, float* rewards_out, uint8_t* terminal_out);

/* Domain::rollout with ANY of the four policies as the closure, s -> policy.sample(rng, s)  (lib.rs:448-479 takes any
 * FnMut(&S) -> A; policies/mod.rs:65-78): an epsilon-greedy or softmax evaluation run next to the greedy one.  `policy` is an
 * rsrl_policy over the ctx's Q function with its own parameters (epsilon for RSRL_EPSILON_GREEDY, tau for RSRL_SOFTMAX; the ctx's
 * behaviour policy is not touched; tau > 0 as in the config: a negative Softmax temperature is RSRL_HIP_EINVAL).  Outputs as rsrl_hip_rollout_trajectory (every one but n_states_out optional).  The draws
 * are a stream of their own, addressed by (number of rollout_policy calls made on the ctx so far, action selection k, global
 * learner id): a call is reproducible, successive calls are independent samples.  The call counter belongs to the ctx OBJECT: it starts
 * at 0 when the ctx is created and is neither saved by rsrl_hip_save_weights nor changed by rsrl_hip_load_weights / rsrl_hip_reset -- the n-th
 * evaluation rollout of a process that restored a checkpoint draws what the n-th rollout of any fresh ctx draws (training draws are keyed by
 * the checkpointed step counter; evaluation draws are not part of the learning state). */
int rsrl_hip_rollout_policy(rsrl_hip_ctx* ctx, int policy, double epsilon, double tau, int64_t step_limit, int64_t M,
                            uint32_t* n_states_out, float* total_reward_out, float* states_out, int32_t* actions_out,
                            float* rewards_out, uint8_t* terminal_out);

/* Order-independent 64-bit checksums of the ctx's device state (sum of the 32-bit words, each multiplied by an odd
 * function of its index): out[0] weights (+traces), out[1] env states/actions/episode counters (+ HIVTreatment's hidden states, a continuous ctx's f32 actions).  For determinism /
 * sharding / fusion-invariance checks at sizes where copying the weights out is not practical. */
int rsrl_hip_checksum(rsrl_hip_ctx* ctx, uint64_t out[2]);

/* Shared weights: every cross-learner sum is 64-bit fixed point (lsb = 2^(floor(log2 lr) - 28)); a term or block sum beyond
 * +-2^42 lsb (|lr*e*phi| > 16384 * 2^floor(log2 lr): a diverged learner) is CLAMPED, and counted here -- terms clamped so far by
 * the shared-W kernels on this ctx's device, all ctxs of the process included (0 in every healthy run: the update then is
 * exactly W += fl(sum of the quantised terms)). */
int rsrl_hip_fx_saturations(rsrl_hip_ctx* ctx, uint64_t* count_out);

/* ---- multi-GPU (one process per GPU; no reference counterpart) -------------------------
 * Shared-W mode across ranks: every batch-step all-reduces the (F x A) f32 weight delta
 * over RCCL.  id_bytes is an ncclUniqueId (128 bytes) produced on rank 0 and distributed
 * by the caller's control plane (torch.distributed / MPI / files). */
int rsrl_hip_comm_unique_id(uint8_t* id_bytes /*[128]*/);
int rsrl_hip_comm_init(rsrl_hip_ctx* ctx, const uint8_t* id_bytes, int world_size, int rank);
/* A communicator of size 1 is valid and runs the SAME finalize -> all-reduce -> apply sequence as world_size > 1.
 *
 * RSRL_EXCHANGE_PEER (config.exchange): the one-hop peer-write exchange instead of RCCL.  Every rank calls
 * rsrl_hip_peer_export (allocates its receive buffer for world_size ranks and describes it in a 128-byte handle: an
 * hipIpcMemHandle plus the owner's pid), the caller's control plane all-gathers the handles, then every rank calls
 * rsrl_hip_peer_connect with all of them in rank order.  Ranks may live in different processes (one per GPU; the
 * buffers are mapped with hipIpcOpenMemHandle) or in one process (several ctxs, any devices: peer access between the
 * devices is enabled by the call, RSRL_HIP_EINVAL if the hardware cannot).  A rank that waits more than 4 s
 * (RSRL_PEER_TIMEOUT_MS in the environment) for a peer's delta gives up: that update is NOT applied as a partial sum (the
 * persistent kernel skips it and ends; the per-step exchange kernels poison the weights with NaN), and the next call that
 * synchronises (rsrl_hip_sync, get_weights / get_states / checksum into host memory, save_weights) returns RSRL_HIP_ERCCL.
 * Slot parity and granule tags follow the number of exchanges performed, not the batch-step counter: a restored checkpoint
 * (rsrl_hip_load_weights sets the counter back) cannot make a stale slot look current. */
#define RSRL_HIP_PEER_HANDLE_BYTES 128
int rsrl_hip_peer_export(rsrl_hip_ctx* ctx, int world_size, uint8_t* handle_out /*[128]*/);
/* 1 if `device` can read and write `peer_device`'s memory directly (hipDeviceCanAccessPeer; a device can always access itself), 0 if not,
 * a negative status on error: what a host needs to choose RSRL_EXCHANGE_PEER for its ranks (every pair must say 1) */
int rsrl_hip_can_access_peer(int device, int peer_device);
/* Which PHYSICAL device is ordinal `device` of this process: PCI domain << 32 | bus << 16 | device (bit 63 set), the same number in every
 * process of a node whatever HIP_VISIBLE_DEVICES it runs under.  With the host's identity it is what a multi-process launcher all-gathers to
 * decide RSRL_EXCHANGE_AUTO the same way on every rank: the peer exchange only if all ranks share ONE host and every rank sees, and can access,
 * every other rank's device (rsrl_amd/distributed.py: choose_exchange); RCCL otherwise.  (ABI 7) */
int rsrl_hip_device_identity(int device, uint64_t* identity_out);
int rsrl_hip_peer_connect(rsrl_hip_ctx* ctx, const uint8_t* handles /*[world_size][128]*/, int world_size, int rank);

/* All ranks in ONE process (a single-threaded host, like the reference's Rc<RefCell> owner graph, rsrl/src/core.rs:13-15):
 * attaches the exchange configured in the ctxs (all alike) to ctxs[0..n), rank = index.  PEER: export + connect of every
 * ctx; RCCL: ncclCommInitAll over the ctxs' devices (one device per rank) plus a grouped warm-up all-reduce, so that no
 * later call blocks on a rank the same thread has not driven yet.  Afterwards the host calls rsrl_hip_train(ctxs[i], ..)
 * for each i in turn (the calls only enqueue) and rsrl_hip_sync(ctxs[i]) at the end. */
int rsrl_hip_group_create(rsrl_hip_ctx* const* ctxs, int n);
/* Step every rank of such a group from that one thread: n_steps batch-steps on ctxs[0..n) (exactly the group's ranks, in rank
 * order); results are those of rsrl_hip_train on every rank from a thread of its own, bit for bit.
 *   RCCL: REQUIRED for n > 1 -- a thread driving several communicators must issue each collective for all of them inside one
 *         ncclGroupStart / End, so the ranks advance in lock-step here and rsrl_hip_train / rsrl_hip_handle on a rank of such a group
 *         return RSRL_HIP_ESTATE.
 *   PEER: feeds the ranks in turns of at most 32 batch-steps, so that no rank's launch queue fills up in front of a peer whose
 *         kernels the same thread has not enqueued yet (calling rsrl_hip_train rank by rank stays valid for short calls). */
int rsrl_hip_group_train(rsrl_hip_ctx* const* ctxs, int n, int64_t n_steps);
/* what is attached: world size and rank as the exchange itself reports them (ncclCommCount / ncclCommUserRank for RCCL),
 * exchange = -1 (none), RSRL_EXCHANGE_RCCL or RSRL_EXCHANGE_PEER.  Any output pointer may be NULL. */
int rsrl_hip_comm_info(rsrl_hip_ctx* ctx, int* world_size, int* rank, int* exchange);

/* ---- measurement hooks (bench.py) --------------------------------------------------------
 * HIP-event timing of the kernels launched by train since the last reset, on the ctx's
 * stream.  ms_total / launches = average launch duration of the dominant kernel. */
int rsrl_hip_timing_enable(rsrl_hip_ctx* ctx, int enable);
int rsrl_hip_timing_read(rsrl_hip_ctx* ctx, double* ms_total, uint64_t* launches, const char** kernel_name);
/* (ABI 9) what this box's memory system delivers: a float4 device-to-device copy of `bytes` bytes (rounded down to 16), `reps` times, by HIP events ->
 * GB/s counting read + write.  No ctx: allocates and frees its own two buffers.  bench.py quotes every HBM fraction against it next to the published peak. */
int rsrl_hip_measure_copy(int device, size_t bytes, int reps, double* gbps_out);

#ifdef __cplusplus
}
#endif
#endif /* RSRL_HIP_H */
