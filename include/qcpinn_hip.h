/* libqcpinn_hip.so — C ABI of the MI355X (gfx950) QCPINN hot path.
 *
 * The reference (masapasa/qcpinn-convection-diffusion-qiskit) has no FFI: its hot path is Python
 * calling PennyLane + torch autograd.  These entry points are what a binding for that path binds
 * instead; each one names the reference code whose arithmetic it replaces.  Plain pointers and
 * sizes only — no torch types.  Every pointer marked "dev" is a device (HBM) pointer owned by the
 * caller; the library never allocates or frees caller memory, never synchronises the stream, and
 * only enqueues work on `stream` (a hipStream_t passed as void*; NULL = default stream).
 * Every function returns 0 on success or a negative QC_ERR_* code; nothing throws.
 *
 * Layouts (all fp32):
 *   [f][B]      "batch-minor": feature f of point p at f*B + p (coalesced over the batch).
 *   jets        6 derivative channels {value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2} x n wires: [6][n][B].
 *   flat params W1[H][3] b1[H] W2[n][H] b2[n] W3[H][n] b3[H] W4[H] b4 theta[n_theta]
 *               (= torch's model.parameters() order of the reference DVPDESolver).
 *   partial rows [rows][stride] gradients, one row per 64-point tile, columns in flat-param order
 *               followed by 3 loss columns (residual, BC, IC); reduced in fixed order (no atomics).
 */
#ifndef QCPINN_HIP_H
#define QCPINN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QC_ABI_VERSION 4

typedef struct qc_program qc_program; /* device-resident gate program (opaque) */

int qc_version(void);
const char* qc_error_string(int code);
int qc_last_hip_error(void); /* hipError_t of the last failing runtime call, 0 if none */

/* ---- gate program: the lowered ansatz of DVQuantumLayer._quantum_circuit
 * (reference nn/DVQuantumLayer.py:176-214 and the builders :246-371).
 * gate_rows: host int32 [n_gates][4] = (opcode, wire_a, wire_b, slot); opcodes
 * RX=0 RY=1 RZ=2 H=3 CNOT=4 CRX=5 CRZ=6 U4=7 (fixed two-wire unitary, slot 0 on wires [0,1],
 * slot 1 on wires [2,3]).  The embedding RX(x_i) is implicit.
 * EMBED=8 (wire_a = wire, wire_b = -1, slot = -1): data re-uploading, RX(x_wire) of the SAME per-point angle (and angle
 * jet) at this position of the program.  A program that holds one is served for 2 <= n_qubits <= 5 by its own kernel
 * family (run-time interpreter, angle encoding, nothing kept between the forward and the adjoint pass, the fused step in
 * its two-stream form); for any other n_qubits the program is created but every circuit and step entry point returns
 * QC_ERR_UNSUPPORTED, and so does qc_program_set_encoding(prog, 1).
 * EMBEDS=9 (wire_a = wire, wire_b = -1, 0 <= slot < n_params): the same gate with a trainable input scaling,
 * RX(theta[slot] * x_wire); theta[slot] is a parameter like a gate angle (its gradient comes back in the same d_theta
 * entry, several gates may share a slot).  Any other row with opcode 9 is QC_ERR_ARG.  It counts as an EMBED gate in
 * everything above: the same family, the same refusals; an EMBED gate beside it keeps scale 1. */
int qc_program_create(const int32_t* gate_rows, int n_gates, int n_qubits, int n_params, qc_program** out);
int qc_program_destroy(qc_program* prog);
size_t qc_trig_bytes(const qc_program* prog); /* size of the per-gate cos/sin workspace */
/* 0 (default): AngleEmbedding, RX(x_i) on wire i (nn/DVQuantumLayer.py:182).  1: AmplitudeEmbedding(normalize=True,
 * pad_with=0) (:177-180); the circuit entry points then take the jets of the INITIAL AMPLITUDES (see
 * qc_amp_forward) where they take angle jets otherwise, and return cotangents w.r.t. them. */
int qc_program_set_encoding(qc_program* prog, int amplitude);
/* angle-jet layout [nch][n][B] -> jets of u = a/|a| (same layout), and the pull-back of their cotangents */
int qc_amp_forward(const float* ajets_dev, float* ujets_dev, int n, int64_t B, int nch, void* stream);
int qc_amp_backward(const float* ajets_dev, const float* ubar_dev, float* abar_dev, int n, int64_t B, int nch,
                    void* stream);

/* cos/sin(theta/2) per gate; call after theta changes (the fused step does it itself). */
int qc_prepare_gates(const qc_program* prog, const float* theta_dev, void* trig_dev, void* stream);

/* Scratch the circuit entry points need for this program (0 for n <= 8: registers / lanes only;
 * for 9 <= n <= 20 the statevectors of one 64-point tile live in HBM).  nch = 1 or 6. */
size_t qc_circuit_workspace_bytes(const qc_program* prog, int nch, int backward);
/* The same for a batch of B points: 9 <= n <= 20 with angle encoding processes every 64-point tile that fits the
 * workspace in ONE launch per stage, so more scratch than the one-tile minimum above buys fewer, larger launches;
 * this returns the bytes that keep the whole batch resident (capped by the QC_HBM_KEEP_GB budget, default 96). */
size_t qc_circuit_workspace_bytes_batch(const qc_program* prog, int nch, int backward, int64_t B);
/* Execution plan of the HBM-resident family (9 <= n <= 20, angle encoding) for the gate rows of qc_program_create, as
 * a flat int32 record: stages (local bit sets), rounds (register bit sets), gates and diagonal tables -- the schedule
 * the kernels run for DVQuantumLayer._quantum_circuit (nn/DVQuantumLayer.py:176-214), which is NOT program order (gates
 * on disjoint wires and diagonal gates are commuted).  Host-only (no GPU needed).  Returns the number of int32 values
 * of the record (written up to `cap`), 0 on invalid input.  Layout: csrc/qc_hbm2_plan.h::h2_describe;
 * tests/test_hbm_plan.py re-executes the record on the CPU against the gate-by-gate program. */
int qc_hbm_plan_describe(const int32_t* gate_rows, int n_gates, int n_qubits, int n_params, int32_t* out, int cap);

/* The execution order of the compile-time programs of the n = 6..8 family (csrc/qc_wave_sched.h): RZ / CRZ gates of the
 * reference circuit (nn/DVQuantumLayer.py:246-262, :348-371) that commute into each other are collected into runs, each
 * applied as one phase-table multiply.  Host-only; the same function the kernels evaluate at compile time.  Record:
 * {n_items, n_runs, items[n_items] (gate index, or -(run + 1)), then per run {count, gate indices}}.  Returns the
 * number of int32 values (written up to `cap`), 0 on invalid input; tests/test_wave_sched.py re-executes it on the CPU. */
int qc_wave_sched_describe(const int32_t* gate_rows, int n_gates, int n_qubits, int n_params, int32_t* out, int cap);

/* ---- DVQuantumLayer.forward, simulator batch branch (nn/DVQuantumLayer.py:151-154):
 * angles [n][B] -> <Z_w> [n][B].  umat_dev: [2 slots][fwd, adjoint][4x4 complex] floats or NULL.
 * ws_dev / ws_bytes: caller-owned scratch of at least qc_circuit_workspace_bytes() (may be NULL/0 if that is 0). */
int qc_forward_expval(const qc_program* prog, const void* trig_dev, const float* umat_dev,
                      const float* angles_dev, float* expval_dev, int64_t B, void* ws_dev, size_t ws_bytes,
                      void* stream);
/* its vector-Jacobian product (what loss.backward() asks of PennyLane's backprop):
 * cot [n][B] -> d_angles [n][B] and d_theta as partial rows at columns [0, n_params) of `part`. */
int qc_backward_expval(const qc_program* prog, const void* trig_dev, const float* umat_dev,
                       const float* angles_dev, const float* cot_dev, float* d_angles_dev,
                       float* part_dev, int64_t part_stride, int64_t row0, int64_t B, void* ws_dev, size_t ws_bytes,
                       void* stream);

/* ---- the same layer carrying the derivative channels that nn/pde.py:59-70 obtains with five
 * torch.autograd.grad(create_graph=True) calls through the simulator. */
int qc_forward_jets(const qc_program* prog, const void* trig_dev, const float* umat_dev,
                    const float* ajets_dev, float* qjets_dev, int64_t B, void* ws_dev, size_t ws_bytes, void* stream);
int qc_backward_jets(const qc_program* prog, const void* trig_dev, const float* umat_dev,
                     const float* ajets_dev, const float* qbar_dev, float* abar_dev, float* part_dev,
                     int64_t part_stride, int64_t row0, int64_t B, void* ws_dev, size_t ws_bytes, void* stream);

/* Register-family (2 <= n <= 5) pair that passes the forward pass's final statevectors to the adjoint
 * pass through chi_dev [6][2*2^n][B] floats instead of recomputing them; both calls must see the same
 * angle jets and parameters (the fused step uses them back to back). */
int qc_forward_jets_keep(const qc_program* prog, const void* trig_dev, const float* umat_dev, const float* ajets_dev,
                         float* qjets_dev, int64_t B, float* chi_dev, void* stream);
int qc_backward_jets_kept(const qc_program* prog, const void* trig_dev, const float* umat_dev, const float* ajets_dev,
                          const float* qbar_dev, float* abar_dev, float* part_dev, int64_t part_stride, int64_t row0,
                          int64_t B, const float* chi_dev, void* stream);

/* ---- classical pre/post networks of DVPDESolver.forward (nn/DVPDESolver.py:37-51,81-110) with
 * the same channels.  nch = 6 (residual points) or 1 (boundary/initial points).
 * Supported shapes (qc_pre_*, qc_post, qc_post_multi and the fused step): 1 <= H <= 1024 hidden units and
 * 1 <= n <= 16 qubits; any other H or n returns QC_ERR_ARG before anything is launched. */
int qc_pre_forward(const float* X_dev /*[B][3]*/, const float* params_dev, int H, int n, int n_theta,
                   float* ajets_dev, int64_t B, int nch, void* stream);
int qc_pre_backward(const float* X_dev, const float* params_dev, int H, int n, int n_theta,
                    const float* abar_dev, float* part_dev, int64_t part_stride, int64_t row0, int64_t B,
                    int nch, void* stream);

/* Output map of the pre network.  QC_ANGLE_MAP_TANH_PI: the encoder of trainer/train.py ends in Tanh and its circuit
 * embeds RX(pi * tanh(v_i)) (:150-155, :206), so the angle jets are those of a = pi tanh(v), v the network's output:
 * a = pi tau, a_k = pi s v_k, a_kk = pi s (v_kk - 2 tau v_k^2) with tau = tanh v, s = 1 - tau^2.  The reverse pass pulls
 * the angle cotangents back through the map from the stored angle jets alone.  qc_pre_forward / qc_pre_backward are the
 * QC_ANGLE_MAP_NONE case; the _map forms take the map explicitly, and the backward form the forward pass's angle jets
 * (read only when the map is not the identity). */
#define QC_ANGLE_MAP_NONE 0
#define QC_ANGLE_MAP_TANH_PI 1
int qc_pre_forward_map(const float* X_dev, const float* params_dev, int H, int n, int n_theta, int angle_map,
                       float* ajets_dev, int64_t B, int nch, void* stream);
int qc_pre_backward_map(const float* X_dev, const float* params_dev, int H, int n, int n_theta, int angle_map,
                        const float* ajets_dev, const float* abar_dev, float* part_dev, int64_t part_stride, int64_t row0,
                        int64_t B, int nch, void* stream);
/* The map the fused step applies between this program's pre network and its embedding (default QC_ANGLE_MAP_NONE). */
int qc_program_set_angle_map(qc_program* prog, int angle_map);

/* Fourier-feature input encoding of the pre network (Tancik et al. 2020; the reference's FourierFeatures modules):
 *   gamma(X) = [sin(2 pi X B), cos(2 pi X B)],  B = freq [3][m] fp32 (rows t, x, y), not trained,
 * in front of Linear(2m, H): W1 is then [H][2m] row-major (sines, then cosines, the order of torch.cat) and the flat
 * vector is  W1[H][2m] b1[H] W2[n][H] b2[n] | W3 ... as before, every later offset (2m - 3) H further on.  The derivative
 * channels of the first layer follow in closed form, with r_j = sum_k B_kj X_k reduced by its nearest integer before
 * the sine and cosine (exact in fp32), so the scale of B costs no accuracy in the argument reduction.
 * qc_program_set_input_map: the library keeps its own device copy of freq_host; m = 0 removes the map; m < 0,
 * m > QC_FF_MAX or a non-finite frequency: QC_ERR_ARG.  Every fused step entry point and qc_fused_step_stage read the
 * map from desc->prog, in the merged and in the two-stream form, as does qc_dataset_scores; the system step refuses a
 * program with a map (QC_ERR_UNSUPPORTED).  Amplitude encoding is supported: its pre stage goes through the same
 * launchers.  part_stride and the optimiser follow the longer vector: NP + 3 > 3072 takes the two-launch tail.
 * The _ff forms are the _map forms with the map given explicitly (freq_dev on the device, 1 <= m <= QC_FF_MAX, else
 * QC_ERR_ARG); shape limits and error codes are those of the _map forms, checked before any launch. */
#define QC_FF_MAX 64
int qc_program_set_input_map(qc_program* prog, const float* freq_host /*[3][m]*/, int m);
int qc_pre_forward_ff(const float* X_dev, const float* params_dev, int H, int n, int n_theta, int angle_map,
                      const float* freq_dev /*[3][m]*/, int m, float* ajets_dev, int64_t B, int nch, void* stream);
int qc_pre_backward_ff(const float* X_dev, const float* params_dev, int H, int n, int n_theta, int angle_map,
                       const float* freq_dev /*[3][m]*/, int m, const float* ajets_dev, const float* abar_dev,
                       float* part_dev, int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream);

typedef struct qc_pde {
  float D, vx, vy;        /* nn/pde.py:53-55 defaults 0.01, 1, 1: the constants of the analytic targets (mode 2) */
  /* operator coefficients, residual = c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy): with the sigma scalings of
   * nn/pde.py:60-70 folded in, c_t = 1/sigma_t, c_x = v_x/sigma_x, c_y = v_y/sigma_y, d_xx = D/sigma_x^2, d_yy = D/sigma_y^2 */
  float c_t, c_x, c_y, d_xx, d_yy;
  float w_res;            /* d loss / d residual scale: 2*weight/N (weight 2, trainer/diffusion_train.py:47) */
  float inv_n_res;        /* 1/N for the logged MSE */
  float w_val_a, w_val_b; /* same for the value segments: a = IC (weight 2), b = BC (weight 4) */
  float inv_n_a, inv_n_b;
  int problem;            /* analytic targets of mode 2: QC_PROBLEM_CONVECTION_DIFFUSION (0), QC_PROBLEM_PURE_DIFFUSION (1)
                             or QC_PROBLEM_GAUSSIAN_PULSE (2) */
  int64_t n_seg_a;        /* leading value points that are IC points */
} qc_pde;

/* 0: trainer/diffusion_train.py + data/diffusion_dataset.py:20-38 (Gaussian u on IC and BC1 points, forcing
 *    term r incl. its -400 constant on residual points);
 * 1: the reference's second workload train_hybrid_qpinn.py:116-131,159-203: u = sin(pi x) sin(pi y) exp(-2 pi^2 D t)
 *    on IC points, 0 on the four boundary faces, residual target 0 (pure diffusion: set vx = vy = 0);
 * 2: trainer/train.py:55-93: the Gaussian pulse u = exp(-100((x-1/2)^2 + (y-1/2)^2)) e^{-t} (the u of problem 0) on IC and
 *    BC points, residual target 0 (no forcing term).
 * Any other id is refused (QC_ERR_ARG) by qc_post mode 2 and the fused step. */
#define QC_PROBLEM_CONVECTION_DIFFUSION 0
#define QC_PROBLEM_PURE_DIFFUSION 1
#define QC_PROBLEM_GAUSSIAN_PULSE 2
/* 3: no analytic target at all.  The targets are DATA, one float per point of the batch: what the reference's
 *    Sampler(dim, coords, func) (data/diffusion_dataset.py:12-19) returns for ANY callable `func`, and what its train()
 *    (trainer/diffusion_train.py:40-47) compares against whatever u and r it is handed.  Accepted only by the *_data entry
 *    points below; the entry points above keep refusing it. */
#define QC_PROBLEM_TABULATED 3

/* mode 0: qjets -> u [B], residual [B] (nn/pde.py:71);
 * mode 1: cotangents (ubar, rbar) [B] -> qbar jets + weight-gradient partial rows;
 * mode 2: forward + analytic targets (data/diffusion_dataset.py:20-38) + squared error + reverse;
 *         out_u_dev / out_res_dev are then B-float scratch buffers (per-point cotangents);
 * mode 4 (nch = 6): qjets -> all six derivative channels of u, out_u_dev = [6][B] (value, d/dt, d/dx, d/dy, d2/dx2,
 *         d2/dy2): operators that are not linear in the channels (Navier-Stokes, nn/pde.py:2-27) combine them outside;
 * mode 3 (nch = 6): its reverse: in_ubar_dev = [6][B] cotangents of those channels -> qbar jets + partial rows. */
int qc_post(int mode, const float* X_dev, const float* params_dev, int H, int n, int n_theta,
            const qc_pde* pde, const float* qjets_dev, float* out_u_dev, float* out_res_dev,
            const float* in_ubar_dev, const float* in_rbar_dev, float* qbar_dev, float* part_dev,
            int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream);

/* qc_post mode 2 on tabulated targets (pde->problem = QC_PROBLEM_TABULATED; any other id is refused): replaces the
 * func(x) of Sampler.sample (data/diffusion_dataset.py:16-19) by target_dev[B], read per point (value points: IC points
 * first, then BC, like X_val), and the residual of nn/pde.py:71 by its form with a zeroth-order term,
 *   residual = c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy)
 * (the reaction term of the Helmholtz operator u_xx + u_yy + lambda u, nn/pde.py:73-95: c_u = lambda, d_xx = d_yy = -1).  c_u is
 * an argument, not a field of qc_pde, whose layout is fixed.  The points themselves are not read.  out_u_dev / out_res_dev
 * are the B-float cotangent scratch buffers of mode 2; a residual point's cotangent on u is c_u times its cotangent on the
 * residual. */
int qc_post_data(const float* params_dev, int H, int n, int n_theta, const qc_pde* pde, const float* qjets_dev,
                 const float* target_dev, float c_u, float* out_u_dev, float* out_res_dev, float* qbar_dev, float* part_dev,
                 int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream);

/* K outputs behind one shared network: a post network Linear(n, H) -> Tanh -> Linear(H, K), 1 <= K <= 4 (the (u, v, p)
 * model nn/pde.py:2-27 differentiates for Navier-Stokes).  params_dev: the flat vector of the single-output layout
 * (its W4 / b4 slots are not read); w4k_dev = [K][H + 1] rows (W4[k][0..H-1], b4[k]).
 * mode 4: out_u_dev = [K][6][B], the six derivative channels of every output, from ONE evaluation of the hidden layer;
 * mode 3: its reverse, in_ubar_dev = [K][6][B] -> qbar jets [6][n][B], the tile rows of the shared parameters in
 * part_dev (W3, b3 columns; the W4 / b4 columns are zeroed) and of the last layer in partk_dev ([rows][K * (H + 1)]). */
int qc_post_multi(int mode, const float* params_dev, int H, int n, int n_theta, int K, const float* w4k_dev,
                  const float* qjets_dev, float* out_u_dev, const float* in_ubar_dev, float* qbar_dev, float* part_dev,
                  int64_t part_stride, float* partk_dev, int64_t partk_stride, int64_t row0, int64_t B, void* stream);

/* ---- optimiser block of the step (trainer/diffusion_train.py:81-90) */
int qc_reduce_rows(const float* part_dev, int64_t rows, int64_t stride, int ncols, float* out_dev, void* stream);

typedef struct qc_opt_hyper {
  double beta1, beta2;
  float eps, max_norm;
  float sched_factor, sched_threshold, sched_min_lr, sched_eps;
  int sched_patience;
  float w_res, w_bc, w_ic;
} qc_opt_hyper;

/* opt_state_dev: 64-byte record {float lr, best; int num_bad, step; float last_loss, last_norm, loss_parts[3];
 * int hist_base; pad}.  flat_dev = [grad[NP] | L_r, L_bc, L_ic].  Clips, applies Adam, steps the plateau
 * scheduler, writes the loss of (1-based) step s to hist_dev[s - 1 - hist_base] when that index lies in
 * [0, hist_cap) (hist_base = steps taken before this history buffer started, e.g. by an earlier train() call on
 * the same optimiser state) and refreshes the trig table from the new theta. */
int qc_adam_step(float* flat_dev, int NP, float* params_dev, float* m_dev, float* v_dev, void* opt_state_dev,
                 const qc_opt_hyper* hp, float* hist_dev, int hist_cap, const qc_program* prog, int theta_off,
                 void* trig_dev, void* stream);

/* ---- L-BFGS on the device: the second training phase (Adam first, then L-BFGS on a fixed batch; the "Adam / L-BFGS"
 * update of the reference's design note hybrid_testing/hybrid_qpinn.md).  qc_lbfgs_step is the counterpart of qc_adam_step:
 * it reads flat_dev = [grad[NP] | L_r, L_bc, L_ic] evaluated at the CURRENT params_dev (what a step call with QC_PHASE_GRADS
 * leaves, for every kind of step: NP is whatever that step's flat vector counts), advances a state machine that lives
 * entirely in ws_dev, and writes the NEXT point to evaluate into params_dev; the trig table and the diagonal-run tables are
 * refreshed from the new theta as qc_adam_step does.  One single-block launch; nothing is read back by the host; flat_dev is
 * not written.  Fixed summation order: two runs of the same sequence are bit-identical.
 *
 * Workspace, 4-byte words, qc_lbfgs_workspace_bytes = 4 (32 + 3 NP + 2 m NP + m + 4 m^2), m = history:
 *   words 0..31, the record (128 bytes):
 *     int   0 phase            0: the next call is a first evaluation; 1: a trial point is pending
 *     int   1 n_eval           calls so far (never reset by qc_lbfgs_restart)
 *     int   2 n_iter           accepted points so far, first evaluations included
 *     int   3 n_pairs          kept curvature pairs, <= m
 *     int   4 head             ring slot the next kept pair is written to; the pairs, oldest first, sit in slots
 *                              (head - n_pairs + k) mod m, k = 0 .. n_pairs - 1
 *     int   5 ls_trials        rejected trials of the running line search
 *     int   6 n_rejected   7 n_skipped_pairs   8 n_resets   9 stalled
 *     int  10 sd_failed        the running search is the steepest-descent restart behind an exhausted search
 *     int  11 NP  12 history  13 accepted (of the last call: 0 / 1)   14, 15 zero
 *     float 16 t               step of the pending trial: params = x_k + t d (FIXED: the step the next pair is formed with)
 *     float 17 f0  18 gtd0     loss at x_k and g_k . d
 *     float 19 gamma           y.s / y.y of the newest kept pair (1 before the first)
 *     float 20 f  21..23 L_r, L_bc, L_ic of the last call
 *     float 24 t_led           the step that led from x_k to the pending point (0: the pending point is x_k)
 *     25..31 zero
 *   x_k[NP], g_k[NP], d[NP]    the last accepted point, its gradient, the search direction
 *   S[m][NP], Y[m][NP]         the pairs s = t d, y = g - g_k by ring slot;  rho[m] = 1 / (y.s)
 *   SY[m][m][2], YY[m][m][2]   Gram entries s_i . y_j and y_i . y_j by ring slot, each a (high, low) float pair whose sum in
 *                              double is the entry: only the new pair's row and column are computed per call, together
 *                              with S.g and Y.g, in ONE batched reduction; the two-loop recursion then runs on these
 *                              scalars and d is one combination of [S, Y, g].  Scalars, recursion and combination are
 *                              double; every stored vector is fp32.
 *
 * The rule.  f = w_res L_r + w_bc L_bc + w_ic L_ic; g = grad; no gradient clipping.  tfirst(v) = lr min(1, 1 / |v|_1).
 *   push(s, y): keep the pair iff y.s > curv_eps (the oldest drops when m are kept) and then gamma = y.s / y.y; else count
 *     it in n_skipped_pairs (ARMIJO) and keep gamma.
 *   dir(g): d = -H g by the two-loop recursion over the kept pairs with H0 = gamma I (newest to oldest a_i = rho_i s_i.q,
 *     q -= a_i y_i; r = gamma q; oldest to newest b_i = rho_i y_i.r, r += (a_i - b_i) s_i; d = -r).
 *   First evaluation (after qc_lbfgs_init or qc_lbfgs_restart): x_k = params, g_k = g, f0 = f, d = -g, gtd0 = -g.g,
 *     t = tfirst(g), params = x_k + t d, phase = 1, ls_trials = 0.  History row (f, 0, 1).
 *   QC_LBFGS_FIXED, every later call: push(t d, g - g_k); x_k = params, g_k = g, f0 = f; d = dir(g); t = lr; gtd0 = g.d;
 *     params += t d unless g.d >= 0, when params stays (t_led = 0; t, d, g_k are still replaced).  This is
 *     torch.optim.LBFGS(lr, max_iter=1, history_size=m, tolerance_grad=0, tolerance_change=0, line_search_fn=None) called
 *     once per evaluation.
 *   QC_LBFGS_ARMIJO, a later call, not stalled: the trial is ACCEPTED iff f and every gradient entry are finite and
 *     f <= f0 + c1 t gtd0.
 *     accepted: push(t d, g - g_k); x_k = params, g_k = g, f0 = f, ls_trials = 0, sd_failed = 0.  With no kept pair:
 *       d = -g, t = tfirst(g), gtd0 = -g.g.  Else d = dir(g), gtd0 = g.d, t = lr; if not gtd0 < 0: all pairs are dropped,
 *       n_resets += 1, and d, t, gtd0 are those of the no-pair case.  params = x_k + t d.
 *     rejected (n_rejected += 1), ls_trials + 1 < max_ls: ls_trials += 1; t_q = -gtd0 t^2 / (2 (f - f0 - gtd0 t));
 *       t <- min(max(t_q, shrink_lo t), shrink_hi t), and t <- shrink_hi t when f or t_q is not finite;
 *       params = x_k + t d.
 *     rejected, ls_trials + 1 >= max_ls (the search is exhausted): if sd_failed is set and no pair is kept: stalled = 1,
 *       params = x_k.  Else n_resets += 1, all pairs dropped, sd_failed = 1, ls_trials = 0, d = -g_k, t = tfirst(g_k),
 *       gtd0 = -g_k.g_k, params = x_k + t d  (x_k, g_k, f0 stay).
 *     stalled: params = x_k on every call; only n_eval, f and the loss parts change.
 *   So an accepted iteration costs one evaluation, and every rejected trial one more.
 *   History: hist_dev[e] = (f, t_led before the call, accepted 0 / 1) for the 0-based evaluation e = n_eval < hist_cap.
 * qc_lbfgs_restart makes the next call a first evaluation at the current params (a new batch); keep_history = 0 also drops
 * the pairs and sets gamma = 1.  Both clear stalled, sd_failed and ls_trials.
 * QC_ERR_ARG, without a GPU: a NULL or misaligned buffer (hist_dev may be NULL), history outside 1..QC_LBFGS_MAX_HISTORY,
 * NP < 1, an unknown line_search, max_ls < 1, lr, c1, shrink_lo, shrink_hi or curv_eps not finite or not positive,
 * shrink_lo > shrink_hi, shrink_hi >= 1, a non-finite weight; prog with trig_dev NULL or theta_off + n_params > NP.
 * qc_lbfgs_workspace_bytes returns 0 for a refused shape.  NP + 3 <= 3072 keeps a call's vectors in registers; larger NP
 * strides over them. */
#define QC_LBFGS_MAX_HISTORY 32
#define QC_LBFGS_FIXED  0   /* torch.optim.LBFGS(line_search_fn=None): every trial is accepted */
#define QC_LBFGS_ARMIJO 1   /* backtracking with safeguarded quadratic interpolation */
typedef struct qc_lbfgs_hyper {
  int history, line_search, max_ls;
  float lr, c1, shrink_lo, shrink_hi, curv_eps;   /* defaults 1, 1e-4, 0.1, 0.5, 1e-10 */
  float w_res, w_bc, w_ic;
} qc_lbfgs_hyper;
size_t qc_lbfgs_workspace_bytes(int NP, int history);
int qc_lbfgs_init(void* ws_dev, int NP, int history, void* stream);
int qc_lbfgs_restart(void* ws_dev, int keep_history, void* stream);
int qc_lbfgs_step(float* flat_dev, int NP, float* params_dev, void* ws_dev, const qc_lbfgs_hyper* hp,
                  float* hist_dev /*[hist_cap][3]*/, int hist_cap,
                  const qc_program* prog, int theta_off, void* trig_dev, void* stream);

/* ---- the three uniform batches of a step (trainer/diffusion_train.py:9-20,34-36: IC t=0 face, BC1 x=0
 * face, residual in [0,1]^3; data/diffusion_dataset.py:12-19) drawn on device with Philox4x32-10 keyed by
 * (seed, step, batch) and indexed by the GLOBAL point index off_* + i: ranks of a data-parallel run fill
 * disjoint shards of the batch a single GPU would draw.  X_val holds the IC points first, then BC. */
int qc_sample_collocation(float* X_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev, int64_t n_ic,
                          int64_t off_ic, int64_t n_bc, int64_t off_bc, uint64_t seed, uint64_t step, void* stream);
/* Same, with the boundary batch spread over the four faces x=0, x=1, y=0, y=1 in that order
 * (train_hybrid_qpinn.py:166-176,689-697): GLOBAL boundary point g lies on face g / bc_face_points.
 * bc_face_points = 0 is the single x=0 face of qc_sample_collocation.  bc_face_points = QC_BC_RANDOM_FACE: every
 * boundary point lies on one of the four faces drawn uniformly at random, per point (trainer/train.py:118-135: t and
 * the free coordinate stay uniform); the face comes from the same Philox draw as the point. */
#define QC_BC_RANDOM_FACE (-1)
int qc_sample_collocation_faces(float* X_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev, int64_t n_ic,
                                int64_t off_ic, int64_t n_bc, int64_t off_bc, int64_t bc_face_points, uint64_t seed,
                                uint64_t step, void* stream);

/* ---- one whole training step (trainer/diffusion_train.py:30-49,81-90) on resident batches:
 * residual batch through the 6-channel pipeline, IC+BC batch through the value pipeline,
 * row reduction, then (phase 2) clip + Adam + scheduler.  With `phases` = 1 it stops after the
 * reduction so the caller can all-reduce `flat_dev` across ranks, then calls again with 2. */
typedef struct qc_step_desc {
  const qc_program* prog;
  void* trig_dev;
  const float* umat_dev;
  int H, n, n_theta;
  float* params_dev; float* m_dev; float* v_dev; void* opt_state_dev;
  float* hist_dev; int hist_cap;
  const float* X_res_dev; int64_t B_res;
  const float* X_val_dev; int64_t B_val;   /* IC points first, then BC points */
  float* ajets_res_dev; float* qjets_res_dev; float* qbar_res_dev; float* abar_res_dev; /* 6*n*B_res each */
  float* ajets_val_dev; float* qjets_val_dev; float* qbar_val_dev; float* abar_val_dev; /* n*B_val each */
  float* part_dev; int64_t part_stride; int64_t part_rows_cap;   /* scratch: rewritten and folded in place every step */
  float* flat_dev;                                                                       /* NP+3 */
  qc_pde pde;
  qc_opt_hyper hyper;
  /* on-device sampler (QC_PHASE_SAMPLE): global index of this rank's first point in each batch */
  int64_t n_ic;                 /* leading IC points of the value batch (== pde.n_seg_a) */
  int64_t sample_off_res, sample_off_ic, sample_off_bc;
  uint64_t sample_seed, sample_step;
  int64_t sample_bc_face_points; /* 0: BC batch on the x=0 face; > 0 or QC_BC_RANDOM_FACE: four faces, see
                                    qc_sample_collocation_faces; smaller values are refused (QC_ERR_ARG) */
  void* circ_ws_dev; size_t circ_ws_bytes;   /* qc_step_workspace_bytes(prog, B_res, B_val); NULL/0 allowed for angle encoding at n <= 8 */
  /* data parallelism inside the library: a communicator of qc_comm_create (or NULL).  With it a call with
   * QC_PHASE_GRADS | QC_PHASE_UPDATE all-reduces flat_dev across the ranks between the two phases, on `stream`. */
  void* comm;
} qc_step_desc;

/* Scratch for one fused step on B_res residual points: the HBM statevector tile for n >= 9; for the
 * register family (2 <= n <= 5) an optional [6][2*2^n][B_res] store of the forward pass's final states
 * that lets the adjoint kernel skip recomputing them (pass less and it recomputes); with amplitude encoding
 * additionally the initial-amplitude jets and their cotangents of both pipelines (required). */
size_t qc_step_workspace_bytes(const qc_program* prog, int64_t B_res, int64_t B_val);

/* One stage of the step above when it runs in its merged form (2 <= n <= 5, angle encoding, both batches non-empty,
 * workspace present): each stage is a single launch over the value tiles and the residual tiles together.  For
 * per-kernel timing; QC_ERR_UNSUPPORTED when the step would take the two-stream form instead. */
#define QC_STAGE_PRE_FWD 0
#define QC_STAGE_CIRCUIT_FWD 1
#define QC_STAGE_POST 2          /* one kernel: point values, cotangents and weight gradients */
#define QC_STAGE_CIRCUIT_BWD 3
#define QC_STAGE_PRE_BWD 4
#define QC_STAGE_COUNT 5
int qc_fused_step_stage(const qc_step_desc* desc, int stage, void* stream);

/* ---- data-parallel collective (collocation batches shard over the GPUs of a node, ONE all-reduce of the
 * flat [gradient | L_r, L_bc, L_ic] vector per step; the reference is single-process and has no counterpart).  RCCL over
 * xGMI, loaded on first use (QC_ERR_UNSUPPORTED when librccl is not available).  Call with the rank's device current.
 * id: 128 bytes (ncclUniqueId), produced on one rank and distributed to the others by the caller's own means. */
int qc_comm_unique_id(void* id_out_128_bytes);
int qc_comm_create(const void* id_128_bytes, int world_size, int rank, void** comm_out);
int qc_comm_destroy(void* comm);
/* in-place sum over the ranks of `count` floats (fp32) on `stream` */
int qc_allreduce_grads(float* buf_dev, int64_t count, void* comm, void* stream);

#define QC_PHASE_GRADS 1
#define QC_PHASE_UPDATE 2
#define QC_PHASE_SAMPLE 4 /* fill X_res / X_val first (see qc_sample_collocation) */
int qc_fused_pinn_residual_step(const qc_step_desc* desc, int phases, void* stream);

/* ---- the same step on a user's own problem: targets as data (QC_PROBLEM_TABULATED), batches from a resident dataset.
 * Replaces, for a target that is not one of the three analytic problems, the Sampler(dim, coords, func) objects and the
 * fetch_minibatch calls of trainer/diffusion_train.py:22-36 (func evaluated once, up front, on the dataset's points) and
 * the u / r arguments of its loss (:44-47). */
typedef struct qc_step_data {
  float* target_res_dev;            /* [B_res] residual targets of the current batch */
  float* target_val_dev;            /* [B_val] value targets, IC points first, then BC */
  float  c_u;                       /* zeroth-order coefficient of the residual (see qc_post_data) */
  /* resident dataset for QC_PHASE_SAMPLE (all NULL/0: SAMPLE is refused) */
  const float* ds_X_res; const float* ds_r;    int64_t ds_n_res;   /* [N][3], [N] */
  const float* ds_X_ic;  const float* ds_u_ic; int64_t ds_n_ic;
  const float* ds_X_bc;  const float* ds_u_bc; int64_t ds_n_bc;
} qc_step_data;

/* The dataset form of qc_sample_collocation (same batch buffers, counts and GLOBAL offsets): point i of a segment
 * (0 residual, 1 IC, 2 BC) with global index g = off + i draws the Philox4x32-10 block of the coordinate draw, counter
 * (g lo, g hi, step lo, step hi ^ segment << 30) and key = seed, and takes row idx = (word 0 * N_seg) >> 32 of that
 * segment's dataset: X_batch[i] = ds_X[idx], target_batch[i] = ds_target[idx] (sampling with replacement, the
 * torch.randint minibatch of a tabulated Sampler).  1 <= N_seg < 2^31 for every non-empty batch, else QC_ERR_ARG. */
int qc_sample_dataset(float* X_res_dev, float* target_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev,
                      float* target_val_dev, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                      const qc_step_data* data, uint64_t seed, uint64_t step, void* stream);

/* qc_fused_pinn_residual_step with desc->pde.problem = QC_PROBLEM_TABULATED (required): the post stage reads its targets
 * from data->target_*_dev and applies data->c_u; QC_PHASE_SAMPLE fills the points AND the targets from the dataset
 * (one launch ahead of the stages) where the analytic step draws coordinates.  Same forms, phases, workspace and flat
 * vector.  QC_ERR_ARG before any launch: a missing target buffer of a non-empty batch; QC_PHASE_SAMPLE with an absent or
 * empty dataset segment behind a non-empty batch, or one of 2^31 rows or more; any other problem id. */
int qc_fused_pinn_data_step(const qc_step_desc* desc, const qc_step_data* data, int phases, void* stream);

/* ---- the tabulated step with the OPERATOR as data too: one coefficient row per residual point, next to its target,
 *   res_p = c_u[p] u + c_3[p] u^3 + c_t[p] u_t + c_x[p] u_x + c_y[p] u_y - (d_xx[p] u_xx + d_yy[p] u_yy).
 * Covers velocity / diffusivity fields v(x, y), D(x); derivative conditions (a Neumann point is the row (0, 0, 1, 0, 0, 0, 0)
 * with the prescribed flux as its target; Robin: c_u and one derivative column); and the cubic term of
 * klein_gordon_operator, u_tt + alpha u_xx + beta u + gamma u**3 (nn/pde.py:28-41): with (t, x) on the x / y slots
 * d_xx = -1, d_yy = -alpha, c_u = beta, c_3 = gamma.  A per-point loss weight w is the row AND its target scaled by sqrt(w).
 * Value points keep comparing u with their target. */
#define QC_COEF_COLS 7   /* c_u, c_t, c_x, c_y, d_xx, d_yy, c_3 -- signs as in qc_post_data, c_3 multiplies u^3 */
typedef struct qc_step_coef {
  float* coef_res_dev;      /* [7][B_res] batch-minor: the rows of the CURRENT residual batch */
  const float* ds_coef;     /* [ds_n_res][7] row-major, beside data->ds_X_res / ds_r: gathered with them under SAMPLE */
} qc_step_coef;

/* qc_post mode 2 on residual points (nch = 6) with per-point operator rows coef_dev[7][B] and targets target_dev[B]
 * (pde->problem = QC_PROBLEM_TABULATED; pde->c_t .. d_yy are not read, w_res and inv_n_res are).  cot_dev[6][B] receives the
 * per-point cotangents of the six channels of u: with g = w_res (res - target),
 *   (c_u + 3 c_3 u^2) g,  g c_t,  g c_x,  g c_y,  -d_xx g,  -d_yy g.
 * The b4 column of a tile row is the sum of the first; the three loss columns are those of qc_post_data. */
int qc_post_coef(const float* params_dev, int H, int n, int n_theta, const qc_pde* pde, const float* qjets_dev,
                 const float* target_dev, const float* coef_dev, float* cot_dev, float* qbar_dev, float* part_dev,
                 int64_t part_stride, int64_t row0, int64_t B, void* stream);

/* qc_sample_dataset that also gathers the operator rows of the residual points, in the same launch and with the same
 * Philox index (so the same batches as qc_sample_dataset on the same seed): coef_res_dev[k * n_res + i] =
 * coef->ds_coef[idx * 7 + k].  coef_res_dev and coef->ds_coef may be NULL only with n_res = 0. */
int qc_sample_dataset_coef(float* X_res_dev, float* target_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev,
                           float* target_val_dev, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                           float* coef_res_dev, const qc_step_data* data, const qc_step_coef* coef, uint64_t seed,
                           uint64_t step, void* stream);

/* qc_fused_pinn_data_step with the residual operator read from coef->coef_res_dev: desc->pde.c_t .. d_yy and data->c_u
 * are not read.  Value tiles, targets, phases, both forms, circuit families, encodings, workspace and flat vector are those
 * of the data step (the split form's [6][B_res] cotangent scratch is the head of abar_res_dev).  QC_PHASE_SAMPLE fills
 * points, targets and coefficient rows in one launch.  QC_ERR_ARG before any launch: coef NULL; coef_res_dev NULL with
 * B_res > 0; QC_PHASE_SAMPLE with ds_coef NULL and B_res > 0; whatever qc_fused_pinn_data_step refuses.  With B_res = 0
 * both pointers may be NULL. */
int qc_fused_pinn_coef_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_coef* coef, int phases,
                            void* stream);

/* ---- residual-adaptive sampling of the dataset's residual rows (RAD / RAR: Wu et al. 2023, Lu et al. 2021): every so many
 * steps the residual is evaluated on the whole candidate pool, and the residual batch is then drawn with probability
 * proportional to |res|^power / mean + floor instead of uniformly.  Three calls, all enqueued on `stream`, no host read:
 * scores of the rows, scores -> an integer CDF, and the gather (or the step) that draws from it.  IC and BC rows stay
 * uniform.  The loss is not reweighted.
 *
 * Scores.  score_dev[j] = | res_j - ds_r[j] | in fp32 for the rows row0 <= j < row0 + rows of data's residual segment
 * (1 <= rows, row0 + rows <= ds_n_res; the other entries of score_dev [ds_n_res] are not touched), res_j the residual the
 * step applies under the current parameters and trig table: coef NULL, that of qc_post_data with data->c_u and desc->pde;
 * else the per-row form of qc_fused_pinn_coef_step on the rows of coef->ds_coef (coef_res_dev is not read).  It runs the
 * forward half of the residual pipeline over chunks of at most B_res rows through the step's own residual scratch:
 * ajets_res_dev, qjets_res_dev, the head of qbar_res_dev ([6][chunk] channels of u) and circ_ws_dev.  Between steps all
 * of these are scratch.  QC_ERR_ARG before any launch: B_res = 0; a NULL buffer; rows or row0 out of range; a problem id
 * other than QC_PROBLEM_TABULATED; coef given with ds_coef NULL; a workspace the step itself would refuse. */
int qc_dataset_scores(const qc_step_desc* desc, const qc_step_data* data, const qc_step_coef* coef, int64_t row0,
                      int64_t rows, float* score_dev, void* stream);

/* Scores -> CDF, every bit defined (integers behind the power, so no result depends on a summation order):
 *  1. p_j = score_j^power, 1 <= power <= 4, by left-to-right fp32 multiplication; a p_j that is NaN or negative counts as 0,
 *     one above FLT_MAX as FLT_MAX.
 *  2. M = max_j p_j.  M = 0: q_j = 1 for every row (uniform).  Otherwise s = 23 - ilogb M and q_j = floor(p_j 2^s) as a
 *     64-bit integer, so that the largest lies in [2^23, 2^24); the scaling and the truncation are exact.
 *  3. Q = sum_j q_j; a = (uint64)((double)floor_c * (double)Q / (double)n_rows), raised to 1 when floor_c > 0 and the
 *     quotient truncates to 0; w_j = q_j + a.  floor_c = 0 is sampling proportional to the residual alone; a row with
 *     w_j = 0 is never drawn.  0 <= floor_c <= QC_ADAPT_FLOOR_MAX (the CDF then stays below 2^64 for every n_rows < 2^31).
 *  4. cdf_j = sum of w_i over i <= j (uint64), and a coarse table with one entry per QC_ADAPT_BLOCK rows,
 *     coarse[b] = cdf[min(n_rows, (b + 1) QC_ADAPT_BLOCK) - 1].
 * adapt_dev: 8-byte aligned, qc_adapt_bytes of n_rows bytes: a 64-byte record {uint64 total = cdf[n_rows - 1], q_sum = Q,
 * add = a; float max_p = M; int32 shift = s (0 when M = 0); pad}, then cdf[n_rows], then coarse[ceil(n_rows / QC_ADAPT_BLOCK)].
 * QC_ERR_ARG: a NULL or misaligned buffer, n_rows outside [1, 2^31), power outside 1..4, floor_c negative, not finite or
 * above QC_ADAPT_FLOOR_MAX.  qc_adapt_bytes returns 0 for an n_rows outside that range. */
#define QC_ADAPT_BLOCK 1024
#define QC_ADAPT_FLOOR_MAX 256.0f
size_t qc_adapt_bytes(int64_t n_rows);
int qc_adapt_build(const float* score_dev, int64_t n_rows, int power, float floor_c, void* adapt_dev, void* stream);

typedef struct qc_step_adapt {
  const void* adapt_dev;   /* the buffer qc_adapt_build filled (or one of the same layout; only cdf and coarse are read) */
  int64_t n_rows;          /* == data->ds_n_res */
} qc_step_adapt;

/* qc_sample_dataset_coef with the residual rows drawn from the CDF: same launch shape, segments, counters and IC / BC
 * draws, so the value batches are bit-identical to the uniform gather's on the same seed.  Residual point i with global
 * index g = off_res + i takes the Philox block it takes there (segment 0 counter, key = seed), forms
 * r64 = word 0 << 32 | word 1 and t = the high 64 bits of r64 * T, T = cdf[n_rows - 1], and copies row
 * idx = min{j : cdf_j > t} (coarse table first, then one block of the CDF).  coef NULL (then coef_res_dev is not written):
 * rows and targets only.  QC_ERR_ARG: adapt NULL, adapt_dev NULL or misaligned, adapt->n_rows != data->ds_n_res, and
 * whatever qc_sample_dataset_coef refuses. */
int qc_sample_dataset_adaptive(float* X_res_dev, float* target_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev,
                               float* target_val_dev, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                               float* coef_res_dev, const qc_step_data* data, const qc_step_coef* coef,
                               const qc_step_adapt* adapt, uint64_t seed, uint64_t step, void* stream);

/* qc_fused_pinn_data_step (coef NULL) or qc_fused_pinn_coef_step whose QC_PHASE_SAMPLE is that gather: still one launch
 * ahead of the stages, and nothing else in the step differs.  QC_ERR_ARG before any launch: adapt NULL, adapt_dev NULL or
 * misaligned, adapt->n_rows != data->ds_n_res, B_res = 0, and whatever the data or the coefficient step refuses. */
int qc_fused_pinn_adaptive_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_coef* coef,
                                const qc_step_adapt* adapt, int phases, void* stream);

/* ---- systems of equations behind one shared network: a model with K outputs (W4[K][H], b4[K]) trained on n_eq
 * residuals, the operator given as DATA, one term list per step.  Replaces navier_stokes_2D_operator (nn/pde.py:2-27: u, v, p
 * from one network, continuity and two momentum equations), the three MSEs, autograd and the optimiser of its training
 * loop by one fused step; Burgers systems, shallow water, Gray-Scott and Lotka-Volterra have the same shape.
 *   res_e(p) = sum over the terms t with t.eq == e of
 *              t.coef * q[t.out][t.chan](p) * (t.mul0 >= 0 ? u[t.mul0](p) : 1) * (t.mul1 >= 0 ? u[t.mul1](p) : 1),
 * q[k][c] channel c (value, t, x, y, xx, yy) of output k and u[k] = q[k][0].  Navier-Stokes takes 14 terms; two
 * multipliers cover cubic reactions such as u v^2.  The loss columns stay three:
 *   L_r = sum_e w_eq[e] mean_p (res_e - r_e)^2,   L_bc, L_ic = sum_k w_out[k] mean (u_k - target_k)^2
 * over the BC / IC points (w_out[k] = 0: output k is not prescribed there, e.g. the pressure), and the loss is
 * w_res L_r + w_bc L_bc + w_ic L_ic of qc_opt_hyper as in every other step.
 * Flat parameter layout (= model.parameters() of the K-output model): W1 b1 W2 b2 | W3 b3 W4[K][H] b4[K] | theta,
 * NP_K = NP + (K - 1)(H + 1) entries; K = 1 is the layout at the head of this file. */
#define QC_KMAX 4         /* outputs */
#define QC_EQMAX 4        /* equations */
#define QC_TERMS_MAX 32   /* terms of all equations together */
typedef struct qc_sys_term {
  int32_t eq, out, chan;   /* 0 <= eq < n_eq, 0 <= out < K, 0 <= chan <= 5 */
  int32_t mul0, mul1;      /* -1 (no factor) or an output 0 .. K - 1 */
  float coef;              /* finite */
} qc_sys_term;

typedef struct qc_step_system {
  int32_t K, n_eq, n_terms;
  qc_sys_term terms[QC_TERMS_MAX];
  float w_eq[QC_EQMAX], w_out[QC_KMAX];   /* finite; entries from n_eq / K on are not read */
  float* target_res_dev;   /* [n_eq][B_res] batch-minor residual targets of the current batch, or NULL: zero */
  float* target_val_dev;   /* [K][B_val] batch-minor value targets, IC points first, then BC (required with B_val > 0) */
  /* resident dataset for QC_PHASE_SAMPLE: the point arrays of qc_step_data and row-major target tables */
  const float* ds_X_res; const float* ds_r;    int64_t ds_n_res;   /* [N][3], [N][n_eq] or NULL (zero targets: then
                                                                      target_res_dev is not written) */
  const float* ds_X_ic;  const float* ds_u_ic; int64_t ds_n_ic;    /* [N][3], [N][K] */
  const float* ds_X_bc;  const float* ds_u_bc; int64_t ds_n_bc;
} qc_step_system;

/* The post stage of the system step alone (the analogue of qc_post_data / qc_post_coef): ONE kernel per 64-point tile for
 * the hidden layer, the channels of the K outputs, residuals, loss columns, cotangents and the reverse pass.
 * params_dev: the K-row flat layout.  nch = 6, residual points: target_dev = [n_eq][B] or NULL (zero); per point and
 * equation g_e = pde->w_res w_eq[e] (res_e - r_e), loss column 0 gets sum_e w_eq[e] (res_e - r_e)^2 pde->inv_n_res.
 * nch = 1, value points (the first pde->n_seg_a are IC points): target_dev = [K][B], required; the cotangent of u_k is
 * (w_val_a | w_val_b) w_out[k] (u_k - target_k), loss columns 2 (IC) / 1 (BC) get w_out[k] (u_k - target_k)^2 inv_n_a | inv_n_b.
 * Writes qbar_dev [nch][n][B] and, in row row0 + tile of part_dev, the columns of W3, b3, W4[K][H], b4[K] and the three
 * loss columns at NP_K .. NP_K + 2 (part_stride >= NP_K + 3); nothing else.  sys->target_* and sys->ds_* are not read.
 * QC_ERR_ARG: K, n_eq, n_terms or a term field out of range, a non-finite coef / w_eq / w_out, a NULL buffer. */
int qc_post_system(const float* params_dev, int H, int n, int n_theta, const qc_step_system* sys, const qc_pde* pde,
                   const float* qjets_dev, const float* target_dev, float* qbar_dev, float* part_dev, int64_t part_stride,
                   int64_t row0, int64_t B, int nch, void* stream);

/* qc_sample_dataset for a system's dataset: the same Philox counter and the same row index, so for the same seed, step and
 * offsets the same rows; target rows are written batch-minor, target_res_dev[e * n_res + i] = ds_r[idx * n_eq + e],
 * target_val_dev[k * (n_ic + n_bc) + i] = ds_u[idx * K + k].  With sys->ds_r or target_res_dev NULL the residual
 * targets are not written.  The buffers are arguments; sys->target_* are not read.  QC_ERR_ARG as qc_sample_dataset,
 * and for K or n_eq out of range. */
int qc_sample_dataset_system(float* X_res_dev, float* target_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev,
                             float* target_val_dev, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                             const qc_step_system* sys, uint64_t seed, uint64_t step, void* stream);

/* The fused step on a system: same descriptor, phases (QC_PHASE_SAMPLE gathers points and target rows from sys->ds_*),
 * workspace rules and comm handling as qc_fused_pinn_data_step; params_dev, m_dev, v_dev hold NP_K entries, flat_dev =
 * [grad[NP_K] | L_r, L_bc, L_ic].  desc->pde supplies w_res, inv_n_res, w_val_*, inv_n_* and n_seg_a (its operator
 * coefficients and problem id are not read).  All circuit families and both encodings; the step runs in the two-stream form.
 * QC_ERR_ARG before any launch: sys NULL; K, n_eq or n_terms out of range; a term field out of range; a non-finite coef,
 * w_eq or w_out; target_val_dev NULL with B_val > 0; QC_PHASE_SAMPLE with an absent or empty segment behind a non-empty
 * batch, or one of 2^31 rows or more; part_stride < NP_K + 3; whatever qc_fused_pinn_data_step refuses of the descriptor. */
int qc_fused_pinn_system_step(const qc_step_desc* desc, const qc_step_system* sys, int phases, void* stream);

/* ---- inverse problems: the tabulated step with a TRAINABLE global operator.  Measurements of u are given (value points
 * anywhere in the domain, through the IC / BC segments of qc_step_data) and coefficients of the operator are identified
 * with the network: what the reference's generic loop would do by handing the coefficient to Adam as one more
 * nn.Parameter.
 *   res_p = c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy),
 *   c_k   = fmaf(scale[k], p[k], base[k]),   k in QC_COEF_COLS order (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3).
 * The trainable vector p[7] lives on the device in the seven flat entries behind theta,
 *   W1 b1 W2 b2 | W3 b3 W4 b4 | theta | p[7],      NP_L = NP + 7,
 * so the optimiser moves it with everything else and no offset of the layout at the head of this file moves.  base and
 * scale are constants of the step.  scale[k] = 0 freezes c_k at base[k] whatever p[k] holds (its gradient entry is exactly 0).
 * scale[k] is also the coefficient's learning-rate multiplier: Adam moves every p[k] by about lr per step, so set scale[k]
 * to the expected magnitude of c_k (a diffusivity of 0.01 cannot be learnt in steps of 0.005).
 * coef_hist_dev (optional, [coef_hist_cap][7]): row s - 1 - hist_base receives the seven c_k used in 1-based step s, next
 * to hist_dev[s - 1 - hist_base], the loss of the same parameters; step and hist_base are read from the optimiser record,
 * the store rides in the residual launch.  It is skipped when desc->opt_state_dev or the buffer is NULL, and in a step
 * without residual points. */
typedef struct qc_step_learn {
  float base[QC_COEF_COLS], scale[QC_COEF_COLS];   /* finite */
  float* coef_hist_dev; int coef_hist_cap;         /* [cap][7] or NULL/0 */
} qc_step_learn;

/* qc_post mode 2 on residual points (nch = 6) under that operator (pde->problem = QC_PROBLEM_TABULATED; pde->c_t .. d_yy
 * are not read, w_res and inv_n_res are).  params_dev holds NP_L entries, p in its last seven.  cot_dev[6][B] receives the
 * per-point cotangents of qc_post_coef with the uniform c_k.  Row row0 + tile of part_dev receives the columns of W3, b3,
 * W4, b4, the seven operator columns at NP_L - 7 + k,
 *   scale[k] * sum over the tile's points of g * (u, u_t, u_x, u_y, -u_xx, -u_yy, u^3)[k],   g = w_res (res - target),
 * (0 where scale[k] = 0; summed in a fixed order, no atomics) and the three loss columns at NP_L .. NP_L + 2
 * (part_stride >= NP_L + 3); nothing else.  learn->coef_hist_dev is not written.  QC_ERR_ARG: a NULL buffer, a non-finite
 * base or scale, part_stride < NP_L + 3. */
int qc_post_learn(const float* params_dev /*NP_L*/, int H, int n, int n_theta, const qc_pde* pde,
                  const qc_step_learn* learn, const float* qjets_dev, const float* target_dev, float* cot_dev /*[6][B]*/,
                  float* qbar_dev, float* part_dev, int64_t part_stride, int64_t row0, int64_t B, void* stream);

/* qc_fused_pinn_data_step under that operator: desc->pde.c_t .. d_yy and data->c_u are not read.  params_dev, m_dev and
 * v_dev hold NP_L entries, flat_dev = [grad[NP_L] | L_r, L_bc, L_ic], part_stride >= NP_L + 3.  Value tiles write zeros to
 * the seven operator columns of their rows; the clip's global norm includes the seven entries.  Everything else (both
 * forms, phases, sampler, circuit families, encodings, workspace, comm) is the data step's.  With B_res = 0 the step runs
 * and the seven gradient entries are exactly 0.  QC_ERR_ARG before any launch: learn NULL; a non-finite base or scale;
 * coef_hist_cap < 0, or a NULL buffer with a positive cap; part_stride < NP_L + 3; whatever qc_fused_pinn_data_step
 * refuses. */
int qc_fused_pinn_inverse_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_learn* learn,
                               int phases, void* stream);

/* ---- learned loss weights (uncertainty balancing): the tabulated step with one trainable log-variance per loss term,
 * in the order of the loss columns and of qc_opt_hyper's weights: residual, BC, IC.  The step minimises
 *   F = sum_k ( w_k e_k L_k + s_k ),   s_k = scale[k] * p[k],   e_k = expf(-s_k) (fp32, the precise exponential),
 *   w_k = hyper.w_res, w_bc, w_ic,
 * over the network and over p[3], which lives on the device in the three flat entries behind theta,
 *   W1 b1 W2 b2 | W3 b3 W4 b4 | theta | p[3],      NP_B = NP + 3.
 * Network entries: the gradient is sum_k w_k e_k grad L_k: every point's cotangent is scaled by the e of its class (e_res
 * on residual points, e_ic on value points below pde.n_seg_a, e_bc on the others).  Entry NP + k: scale[k] * (1 - w_k e_k
 * L_k), formed in the optimiser launch from the reduced loss columns (after the all-reduce under a communicator); every
 * tile row holds 0 in these three columns, so after a GRADS-only call the three entries of flat_dev are exactly 0, and
 * UPDATE leaves their values visible there next to the clipped network gradient.  The clip's norm and factor cover the first NP
 * entries only (last_norm is that norm); the three entries are not scaled.  The step's Adam moves all NP_B entries.
 * scale[k] = 0 freezes term k (gradient exactly 0; p[k], m, v bit-unchanged from a zero start); scale[k] is also the
 * learning-rate multiplier of s_k.  The plateau scheduler, hist_dev and last_loss see F, which may be negative; loss_parts
 * stay the raw L_r, L_bc, L_ic.  weight_hist_dev (optional, [weight_hist_cap][3]): row s - 1 - hist_base receives the
 * effective weights w_k e_k used in 1-based step s; the store rides in the optimiser launch, which reads p before moving it. */
#define QC_BAL_TERMS 3
typedef struct qc_step_balance {
  float scale[QC_BAL_TERMS];                   /* finite */
  float* weight_hist_dev; int weight_hist_cap; /* [cap][3] or NULL/0 */
} qc_step_balance;

/* qc_post_data under those weights: params_dev holds NP_B entries, p in its last three; nch = 6 scales the cotangents by
 * pde->w_res * e_res, nch = 1 by pde->w_val_a * e_ic (points below pde->n_seg_a) or pde->w_val_b * e_bc.  The tile rows
 * receive what qc_post_data writes, the loss columns (unweighted) at NP_B .. NP_B + 2 (part_stride >= NP_B + 3) and 0 in
 * columns NP_B - 3 .. NP_B - 1.  bal->weight_hist_dev is not written.  QC_ERR_ARG: bal NULL or not valid (below), and
 * whatever qc_post_data refuses. */
int qc_post_balance(const float* params_dev /*NP_B*/, int H, int n, int n_theta, const qc_pde* pde,
                    const qc_step_balance* bal, const float* qjets_dev, const float* target_dev, float c_u, float* out_u,
                    float* out_res, float* qbar_dev, float* part_dev, int64_t part_stride, int64_t row0, int64_t B, int nch,
                    void* stream);

/* qc_adam_step for flat_dev = [grad[NP_B] | L_r, L_bc, L_ic] under those weights: the three entries in front of the loss
 * columns are formed here (whatever flat_dev holds there) and written back, F goes to the scheduler, hist_dev and
 * last_loss, and the weight row is stored.  One launch (NP_B + 3 <= 3072: the single-round-trip kernel), nothing is read
 * back.  QC_ERR_ARG: bal NULL; a non-finite scale; weight_hist_cap < 0, or a NULL buffer with a positive cap; NP_B < 4;
 * theta_off + prog->n_params > NP_B - 3; whatever qc_adam_step refuses. */
int qc_balance_adam_step(float* flat_dev, int NP_B, float* params_dev, float* m_dev, float* v_dev, void* opt_state_dev,
                         const qc_opt_hyper* hp, const qc_step_balance* bal, float* hist_dev, int hist_cap,
                         const qc_program* prog, int theta_off, void* trig_dev, void* stream);

/* qc_fused_pinn_data_step under those weights: params_dev, m_dev and v_dev hold NP_B entries, flat_dev = [grad[NP_B] | L_r,
 * L_bc, L_ic], part_stride >= NP_B + 3.  Everything else (both forms, phases, sampler, circuit families, encodings,
 * workspace, comm) is the data step's, and a GRADS | UPDATE call has its launch count.  QC_ERR_ARG before any launch: bal
 * NULL; a non-finite scale; weight_hist_cap < 0, or a NULL buffer with a positive cap; part_stride < NP_B + 3; whatever
 * qc_fused_pinn_data_step refuses. */
int qc_fused_pinn_balanced_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_balance* bal,
                                int phases, void* stream);

/* ---- causal training (Wang, Sankaran, Perdikaris 2022): the tabulated step on a time-dependent problem, with the
 * residual of a late time slab held back until the earlier slabs are fitted.  The residual rows of the dataset are sorted
 * by t and cut into M = n_slabs slabs of equal width in t; slab_lo_dev[M + 1] (int64, device) holds the first row of each
 * slab and the row count behind the last.  Every 64-point tile of the residual batch holds points of ONE slab: the tile of
 * global point index g is tau = g / 64 and its slab is tau mod M.  With L_i the mean squared residual of the batch's
 * points of slab i, the step minimises
 *   w_res L_r^c + w_bc L_bc + w_ic L_ic,   L_r^c = (1/M) sum_i W_i L_i,   W_i = exp(-eps sum_{k<i} L_k),   W_0 = 1,
 * the W_i taken as constants when differentiating.  Nothing in the stages changes: each writes one partial row per tile
 * and the reverse pass is linear in the per-point cotangent, so the causal gradient is the ordinary partial rows summed
 * with one scalar per residual row, known when the row fold runs.  A single-block launch ahead of the fold forms the L_i
 * from the L_r column of the residual rows (L_i = M * the sum of the column over the rows of slab i; lane l of the wave
 * that owns the slab adds the slab's rows l, l + 64, ... in ascending order in double, the 64 lane sums are added by a
 * butterfly over lane distances 32, 16, .. 1; the cumulative sums run over the slabs in ascending order, in double; W_i is
 * the double exponential rounded to fp32), and the fold scales residual row r by W[(r + off_res / 64) mod M] as it loads
 * it, value rows by nothing, in the summation order of the plain fold.  The folded L_r column is L_r^c, which the
 * unchanged optimiser launch weighs with w_res; loss_parts[0] and the history see it.  eps = 0 gives W = 1 exactly and
 * the data step bit for bit.
 * state_dev: the record of 4 + 2 M 4-byte words {float eps; int32 n_raised; int32 n_steps; int32 hist_base; float W[M];
 * float L[M]}, seeded by the init call below.  Every causal fold reads eps, writes the W and L it used, stores the row
 * [eps, W[M], L[M]] to row n_steps - hist_base of hist_dev ([hist_cap][1 + 2 M], optional) when that row lies in the buffer,
 * adds 1 to n_steps and anneals eps for the NEXT fold: if W[M - 1] (the smallest weight, as L >= 0) exceeds delta (compared
 * in fp32) and eps < eps_max then eps = min(eps * eps_growth, eps_max) (formed in double, stored in fp32) and n_raised
 * grows by 1. */
#define QC_CAUSAL_MAX_SLABS 64
#define QC_CAUSAL_STATE_WORDS(M) (4 + 2 * (M))
typedef struct qc_step_causal {
  int32_t n_slabs;                              /* M: 2 .. QC_CAUSAL_MAX_SLABS */
  float eps0, eps_growth, eps_max, delta;       /* eps0 >= 0 (read by the init call only); the others finite and > 0 */
  const int64_t* slab_lo_dev;                   /* [M + 1] row offsets of the slabs (QC_PHASE_SAMPLE and the gather only) */
  void* state_dev;                              /* the record above, 4-byte aligned */
  float* hist_dev; int32_t hist_cap;            /* [cap][1 + 2 M] or NULL/0 */
} qc_step_causal;

/* Seeds the record: eps = eps0, n_raised = n_steps = hist_base = 0, W = 1, L = 0.  QC_ERR_ARG: a NULL or misaligned
 * state_dev, causal NULL or not valid (as the causal step refuses it). */
int qc_causal_init(void* state_dev, const qc_step_causal* causal, void* stream);

/* qc_sample_dataset with the residual rows stratified by slab: a residual point with global index g takes row
 *   slab_lo[s] + ((word 0 * (slab_lo[s + 1] - slab_lo[s])) >> 32),   s = (g / 64) mod n_slabs,
 * word 0 of the block qc_sample_dataset draws for it; IC and BC points draw as there, so the value batches are bit-identical.
 * QC_ERR_ARG without a GPU: n_res not a multiple of 64 * n_slabs, off_res not a multiple of 64, n_slabs outside
 * 2..QC_CAUSAL_MAX_SLABS, slab_lo_dev NULL, whatever qc_sample_dataset refuses.  An empty slab is NOT refused on the
 * device: its points take the row at the slab's offset, and every row index is clamped into the residual segment, so a
 * wrong table cannot read outside it (data.tabulated.CausalWeighting raises on an empty slab). */
int qc_sample_dataset_slabs(float* X_res_dev, float* target_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev,
                            float* target_val_dev, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                            const qc_step_data* data, int n_slabs, const int64_t* slab_lo_dev, uint64_t seed, uint64_t step,
                            void* stream);

/* The causal reduction of a partial-row matrix on its own: weights from column ncols - 3 of rows [0, rows_res), the
 * weighted first level in place (part_dev is overwritten like the step's own matrix), the second level into
 * flat_dev[ncols]; the tile offset is 0.  Two runs on equal inputs and records are bit-identical.  QC_ERR_ARG: a NULL
 * buffer, ncols < 3, stride < ncols, rows outside [1, 2^31), rows_res outside [1, rows] or not a multiple of n_slabs,
 * causal NULL or not valid. */
int qc_causal_fold(float* part_dev, int64_t rows, int64_t rows_res, int64_t stride, int ncols, const qc_step_causal* causal,
                   float* flat_dev, void* stream);

/* qc_fused_pinn_data_step under causal weights: QC_PHASE_SAMPLE gathers with the slab rule above, and the causal fold
 * stands in place of the plain row fold; every other launch, both forms (merged and two-stream) and all three circuit
 * families are the data step's (in each family row r of the residual pipeline holds exactly points [64 r, 64 r + 64)).  A
 * GRADS | UPDATE call has one launch more than the data step's.  Refused before any launch: desc->comm set:
 * QC_ERR_UNSUPPORTED (the slab losses would need a reduction of their own); QC_ERR_ARG: causal NULL, n_slabs out of range,
 * a NULL or misaligned state_dev, a non-finite or non-positive eps_growth, eps_max or delta, a negative or non-finite
 * eps0, hist_cap < 0 or a NULL hist_dev with a positive cap, B_res not a positive multiple of 64 * n_slabs, sample_off_res
 * not a multiple of 64, QC_PHASE_SAMPLE with slab_lo_dev NULL, whatever qc_fused_pinn_data_step refuses. */
int qc_fused_pinn_causal_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_causal* causal, int phases,
                              void* stream);

/* ---- gradient-norm loss weights (Wang, Teng, Perdikaris 2021, "learning-rate annealing", Algorithm 1): the analytic, the
 * tabulated or the coefficient step with the two data terms weighted from this step's own per-class gradients,
 *   hat_k = max_j |G_res[j]| / mean_j |G_k[j]|,   lam_k <- (1 - alpha) lam_k + alpha hat_k,   k in {BC, IC},
 * and the descent direction G_res + lam_bc G_bc + lam_ic G_ic.  G_c is the gradient of class c as the rows carry it, the
 * loss weight and the mean included (G_k = w_k grad L_k): with unit loss weights the rule is the paper's.
 * Nothing in the stages changes.  Every stage writes one partial row per 64-point tile, the residual tiles rows
 * [0, rows_res), value tile k row rows_res + k, and the value batch holds its IC points first: with n_ic a multiple of 64
 * (or one value class empty) every row belongs to ONE class.  The class fold reduces the rows of each class in place to
 * at most 32 (block (cb, rs, c) folds rows lo_c + rs, lo_c + rs + RS_c, .. into row lo_c + rs, RS_c = min(n_c, 32), in the
 * summation order of the plain fold on the class's rows alone).  A single-block launch then forms G_c[j], the left-to-right
 * sum of the class's surviving rows, for all NP + 3 columns, and, when n_steps % every == 0,
 *   m_r = max_{j<NP} |G_res[j]|,   a_k = (1/NP) sum_{j<NP} |G_k[j]|   (sums in double, fixed order),
 *   lam_k = min(lam_max, (1 - alpha) lam_k + alpha m_r / a_k)          (formed in double, stored in fp32);
 * lam_k keeps its value when class k is empty, when a_k = 0 and when m_r or a_k is not finite (hat_k is then recorded as
 * 0).  It writes flat[j] = fmaf(lam_ic, G_ic[j], fmaf(lam_bc, G_bc[j], G_res[j])) for j < NP with the weights AFTER this
 * update, and flat[NP..NP+2] = L_r, L_bc, L_ic, the unscaled column sums (G_res + G_ic) + G_bc.  The unchanged optimiser
 * launch follows on flat: it clips the combined gradient, and its record, the loss history and the plateau scheduler see
 * w_res L_r + w_bc L_bc + w_ic L_ic as in every other step, comparable from step to step while lam moves.
 * state_dev: the record of QC_GRADNORM_STATE_WORDS 4-byte words
 *   {float lam_bc, lam_ic; int32 n_steps, hist_base, n_updates; float m_r, a_bc, a_ic, hat_bc, hat_ic; 6 words of 0},
 * seeded by the init call below: lam of the NEXT step, the counters, and the statistics of the last update.  Every call
 * stores the row {lam_bc, lam_ic, m_r, a_bc, a_ic, wl, updated} (QC_GRADNORM_HIST_COLS floats) to row n_steps - hist_base
 * of hist_dev ([hist_cap][QC_GRADNORM_HIST_COLS], optional) when that row lies in the buffer: the weights the step used,
 * the statistics of the record (this step's when updated = 1, else those of the last update),
 * wl = w_res L_r + lam_bc w_bc L_bc + lam_ic w_ic L_ic, and 1 or 0; then n_steps grows by 1. */
#define QC_GRADNORM_STATE_WORDS 16
#define QC_GRADNORM_HIST_COLS 7
typedef struct qc_step_gradnorm {
  float alpha;                         /* in [0, 1]; 0 keeps the weights */
  float lam_max;                       /* finite and > 0 */
  int32_t every;                       /* >= 1: the weights move on the steps with n_steps % every == 0 */
  float lam0_bc, lam0_ic;              /* finite and > 0 (read by the init call only) */
  float* state_dev;                    /* the record above, 4-byte aligned */
  float* hist_dev; int32_t hist_cap;   /* [cap][QC_GRADNORM_HIST_COLS] or NULL/0 */
} qc_step_gradnorm;

/* Seeds the record: lam = lam0, every counter and statistic 0.  QC_ERR_ARG: a NULL or misaligned state_dev, gn NULL or not
 * valid (as the gradient-norm step refuses it). */
int qc_gradnorm_init(float* state_dev, const qc_step_gradnorm* gn, void* stream);

/* The two launches above on any row matrix: rows [0, rows_res) are the residual class, the next rows_ic rows the IC class,
 * the remaining rows - rows_res - rows_ic the BC class; the first level is in place (part_dev is overwritten like the
 * step's own matrix, rows outside the classes' survivors and columns >= ncols are not written), flat_dev[ncols] receives
 * the combination (the last three columns are the loss columns, wl is formed with unit loss weights) and class_dev
 * ([3][ncols]: G_res, G_ic, G_bc; or NULL) the class sums.  Two runs on equal inputs and records are bit-identical.
 * QC_ERR_ARG: a NULL part_dev or flat_dev, ncols < 4, stride < ncols, rows outside [1, 2^31), rows_res or rows_ic negative
 * or rows_res + rows_ic > rows, gn NULL or not valid. */
int qc_gradnorm_fold(float* part_dev, int64_t rows, int64_t rows_res, int64_t rows_ic, int64_t stride, int ncols,
                     const qc_step_gradnorm* gn, float* flat_dev, float* class_dev, void* stream);

/* The fused step under gradient-norm weights.  data NULL: the analytic step (the problems and the draw of the residual
 * step); data alone: the tabulated step; data and coef: the coefficient step.  All three circuit families, both encodings
 * and both forms (merged and two-stream) are the underlying step's.  QC_PHASE_GRADS: the stages, the class fold and the
 * combination; the weights move here and flat_dev then holds the combined gradient and the loss columns.
 * QC_PHASE_UPDATE: the plain optimiser launch on flat_dev.  A GRADS | UPDATE call has two launches more than the
 * tabulated step's.  Refused before any launch: desc->comm set: QC_ERR_UNSUPPORTED (the class gradients of the ranks
 * would need a reduction of 3 (NP + 3) entries ahead of the ratio); QC_ERR_ARG: gn NULL, a NULL or misaligned state_dev,
 * alpha outside [0, 1], every < 1, a non-finite or non-positive lam_max, lam0_bc or lam0_ic, hist_cap < 0 or a NULL
 * hist_dev with a positive cap, n_ic not a multiple of 64 while both n_ic and B_val - n_ic are positive (a value tile
 * would mix the classes), coef without data, whatever the underlying step refuses. */
int qc_fused_pinn_gradnorm_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_coef* coef,
                                const qc_step_gradnorm* gn, int phases, void* stream);

/* ---- a seventh derivative channel, d2/dt2: equations that are second order in time over TWO space dimensions.  The
 * reference's wave_operator and klein_gordon_operator (nn/pde.py:28-52) differentiate a two-input model twice in each of its
 * inputs, so with the six channels above they are 1-D in space ((t, x) on the x / y slots); a three-input model needs u_tt
 * beside u_xx and u_yy.  Every entry point below is its six-channel counterpart on jets [7][n][B]: channels 0..5 as at the
 * head of this file, channel 6 = d2/dt2.  Operator rows have 8 columns, the seven of QC_COEF_COLS and d_tt:
 *   res_p = c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy + d_tt u_tt)
 * (wave equation u_tt - c^2 (u_xx + u_yy) = 0: d_tt = -1, d_xx = d_yy = c^2; telegraph: c_t = a as well; 2-D Klein-Gordon
 * u_tt + alpha (u_xx + u_yy) + beta u + gamma u^3: d_tt = -1, d_xx = d_yy = -alpha, c_u = beta, c_3 = gamma).  A condition on
 * u_t (the second initial condition of a wave problem) is a residual row (0, 1, 0, 0, 0, 0, 0, 0) with the prescribed
 * velocity as its target.  Flat parameter vector, partial rows and loss columns are unchanged.
 * Served: programs of the register family (2 <= n <= 5) without EMBED / EMBEDS gates, angle encoding, no input map
 * (qc_program_set_input_map), angle map QC_ANGLE_MAP_NONE; the circuit stages run the gate program as run-time data and
 * recompute the forward sweep in the adjoint kernel (nothing is kept between them, no workspace).  Anything else:
 * QC_ERR_UNSUPPORTED before any launch, nothing written; the pre / post stages alone return it for n outside 2..5. */
#define QC_NCH_TT 7
#define QC_COEF_TT_COLS 8   /* c_u, c_t, c_x, c_y, d_xx, d_yy, c_3, d_tt */

/* qc_pre_forward / qc_pre_backward with nch fixed at 7: ajets_dev / abar_dev are [7][n][B];
 * a_tt[i] = sum_j W2[i][j] tanh''(s_j) W1[j][0]^2.  The reverse stage writes the W1, b1, W2, b2 columns of the tile rows. */
int qc_pre_forward_tt(const float* X_dev /*[B][3]*/, const float* params_dev, int H, int n, int n_theta, float* ajets_dev,
                      int64_t B, void* stream);
int qc_pre_backward_tt(const float* X_dev, const float* params_dev, int H, int n, int n_theta, const float* abar_dev,
                       float* part_dev, int64_t part_stride, int64_t row0, int64_t B, void* stream);

/* qc_forward_jets / qc_backward_jets on [7][n][B]: q_tt[w] = 2 Re<chi_0|Z_w|chi_tt> + 2 <chi_t|Z_w|chi_t> with chi_tt built
 * from (a_t, a_tt).  The reverse stage writes d_theta as partial rows at columns [0, n_params) of part_dev.  Two calls on
 * equal inputs give the same bits. */
int qc_forward_jets_tt(const qc_program* prog, const void* trig_dev, const float* umat_dev, const float* ajets_dev,
                       float* qjets_dev, int64_t B, void* stream);
int qc_backward_jets_tt(const qc_program* prog, const void* trig_dev, const float* umat_dev, const float* ajets_dev,
                        const float* qbar_dev, float* abar_dev, float* part_dev, int64_t part_stride, int64_t row0, int64_t B,
                        void* stream);

/* qc_post_coef with coef_dev[8][B], cot_dev[7][B] and qjets / qbar [7][n][B] (pde->problem = QC_PROBLEM_TABULATED; w_res and
 * inv_n_res are read).  cot_dev receives the per-point cotangents of the seven channels of u: with g = w_res (res - target),
 *   (c_u + 3 c_3 u^2) g,  g c_t,  g c_x,  g c_y,  -d_xx g,  -d_yy g,  -d_tt g.
 * The tile rows receive the W3, b3, W4, b4 columns (b4: the sum of the first cotangent) and the three loss columns. */
int qc_post_coef_tt(const float* params_dev, int H, int n, int n_theta, const qc_pde* pde, const float* qjets_dev,
                    const float* target_dev, const float* coef_dev, float* cot_dev, float* qbar_dev, float* part_dev,
                    int64_t part_stride, int64_t row0, int64_t B, void* stream);
/* qc_post modes 4 and 3 with seven channels (what a model's jets_tt and its backward ask for): mode 4: qjets -> the seven
 * channels of u, io_dev = [7][B] (written); mode 3: io_dev = [7][B] cotangents of those channels (read) -> qbar jets and the
 * W3, b3, W4, b4 columns of the tile rows.  Any other mode: QC_ERR_ARG. */
int qc_post_jets_tt(int mode, const float* params_dev, int H, int n, int n_theta, const float* qjets_dev, float* io_dev,
                    float* qbar_dev, float* part_dev, int64_t part_stride, int64_t row0, int64_t B, void* stream);

typedef struct qc_step_coef_tt {
  float* coef_res_dev;      /* [8][B_res] batch-minor: the rows of the CURRENT residual batch */
  const float* ds_coef;     /* [ds_n_res][8] row-major, beside data->ds_X_res / ds_r: gathered with them under SAMPLE */
} qc_step_coef_tt;

/* qc_sample_dataset_coef for 8-column rows: coef_res_dev[k * n_res + i] = coef->ds_coef[idx * 8 + k], idx the row index
 * qc_sample_dataset draws on the same seed, step and offsets (same Philox counters), so points and targets are bit-identical
 * to its.  The rows travel through the dataset gather kernel in a second launch on the same counters.  coef_res_dev and
 * coef->ds_coef may be NULL only with n_res = 0. */
int qc_sample_dataset_coef_tt(float* X_res_dev, float* target_res_dev, int64_t n_res, int64_t off_res, float* X_val_dev,
                              float* target_val_dev, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                              float* coef_res_dev, const qc_step_data* data, const qc_step_coef_tt* coef, uint64_t seed,
                              uint64_t step, void* stream);

/* qc_fused_pinn_coef_step with the seven-channel residual pipeline: the four residual buffers of desc hold 7 n B_res floats
 * each (the [7][B_res] cotangent scratch is the head of abar_res_dev), coef->coef_res_dev is [8][B_res]; desc->pde.c_t .. d_yy
 * and data->c_u are not read.  The value batch goes through the one-channel kernels of every other step.  Always the
 * two-stream form; row fold, optimiser launch, phases and desc->comm as in the data step.  No circuit workspace is needed:
 * circ_ws_dev / circ_ws_bytes may be NULL / 0 and are not read.
 * QC_ERR_UNSUPPORTED before any launch: what the head of this section lists.  QC_ERR_ARG before any launch: desc, data or
 * coef NULL; a problem id other than QC_PROBLEM_TABULATED; coef_res_dev NULL with B_res > 0; QC_PHASE_SAMPLE with ds_coef NULL
 * and B_res > 0; a NULL residual buffer with B_res > 0; whatever qc_fused_pinn_coef_step refuses. */
int qc_fused_pinn_coef_tt_step(const qc_step_desc* desc, const qc_step_data* data, const qc_step_coef_tt* coef, int phases,
                               void* stream);

/* ---- ensembles: M independent models of ONE architecture and ONE gate program per launch sequence.  A seed / learning-rate /
 * loss-weight / operator-constant sweep or a deep ensemble of the reference's small model (trainer/diffusion_train.py with
 * batch_size 64: one residual tile and one value tile per stage) is M times a step that leaves the chip idle; the ensemble
 * step has the single-model step's launches, each over the tiles of all M members (grid = tiles of one member x M).
 *
 * The contract: member m computes what qc_fused_pinn_residual_step computes on a descriptor whose buffers are member m's
 * slices, whose sampler key is desc->sample_seed + m, and whose pde and hyper are member m's.
 *
 * desc describes member 0.  Every per-model buffer of it is the first of M consecutive slices; member m's slice starts m
 * strides behind it:
 *   params_dev, m_dev, v_dev          params_stride floats, >= NP
 *   flat_dev                          flat_stride floats, >= NP + 3
 *   opt_state_dev                     64-byte records, back to back
 *   hist_dev                          hist_stride floats, >= hist_cap (not read when hist_dev is NULL)
 *   trig_dev                          trig_stride BYTES, >= qc_trig_bytes(prog) and a multiple of 256
 *   X_res_dev / X_val_dev             x_res_stride / x_val_stride floats, >= 3 B_res / 3 B_val
 *   the four residual jet buffers     jets_res_stride floats, >= 6 n B_res
 *   the four value jet buffers        jets_val_stride floats, >= n B_val
 *   part_dev                          part_rows_cap * part_stride floats: [M][part_rows_cap][part_stride]
 *   circ_ws_dev                       ws_stride BYTES, >= qc_step_workspace_bytes(prog, B_res, B_val) and a multiple of 256;
 *                                     desc->circ_ws_bytes is the size of ONE slice
 * prog and umat_dev are shared.  pde_dev / hyper_dev: device tables of M qc_pde / qc_opt_hyper records (8-byte aligned), or
 * NULL: every member takes desc->pde / desc->hyper.  A table entry's problem id and n_seg_a must be desc->pde's (they are
 * not checked: the tables live on the device).  The learning rate is per member already: it lives in the state record.
 * qc_ensemble_strides fills the smallest strides for desc and M and leaves both tables NULL.
 *
 * Phases as in the single-model step; QC_PHASE_GRADS alone leaves member m's [gradient | L_r, L_bc, L_ic] in its flat slice.
 * Scope: what the merged form of the single-model step covers with analytic targets: register family (2 <= n <= 5, no EMBED
 * gates), angle encoding, no Fourier-feature map, B_res > 0 and B_val > 0, every buffer and the final-state store present,
 * problems 0 .. 2, points drawn on the device or given, H <= 128 (the fused post kernel); compile-time programs where the
 * single-model step uses them.  QC_ERR_UNSUPPORTED before any launch: another family, amplitude encoding, a Fourier-feature
 * map, EMBED gates, H > 128.  QC_ERR_ARG before any launch: desc or ens NULL; desc->comm set; M < 1 or M > 65535; a stride
 * below its bound or a trig / workspace stride that is no multiple of 256; a NULL buffer, an empty batch or a workspace
 * slice smaller than the final-state store; a misaligned table; a problem id outside 0 .. 2 (tabulated targets have no
 * ensemble form); and whatever qc_fused_pinn_residual_step refuses. */
typedef struct qc_step_ensemble {
  int M;
  int64_t params_stride, flat_stride, hist_stride;
  int64_t trig_stride;                      /* bytes */
  int64_t x_res_stride, x_val_stride, jets_res_stride, jets_val_stride;
  int64_t ws_stride;                        /* bytes */
  const qc_pde* pde_dev;
  const qc_opt_hyper* hyper_dev;
} qc_step_ensemble;
int qc_ensemble_strides(const qc_step_desc* desc, int M, qc_step_ensemble* ens_out);
int qc_fused_pinn_ensemble_step(const qc_step_desc* desc, const qc_step_ensemble* ens, int phases, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QCPINN_HIP_H */
