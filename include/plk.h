/* plk.h -- C-ABI of libplk, the MI355X (gfx950) Felsenstein-pruning engine.
 *
 * This is the drop-in boundary under the Bio++ likelihood classes.  The
 * reference (bpp-phyl) has no FFI: its hot path is a set of C++ virtuals, and
 * each entry point below replaces one of them (paths relative to
 * /root/reference/src/Bpp/Phyl/):
 *
 *   plk_set_tip_codes / plk_set_code_table
 *       DRASRTreeLikelihoodData::initLikelihoods leaf init
 *       (Likelihood/DRASRTreeLikelihoodData.cpp:160-191) with
 *       AbstractTransitionModel::getInitValue (Model/AbstractSubstitutionModel.cpp:98-112)
 *   plk_set_pattern_weights
 *       rootWeights_ (Likelihood/AbstractTreeLikelihoodData.h:91)
 *   plk_set_eigen
 *       SubstitutionModel::getEigenValues / getColumnRightEigenVectors /
 *       getRowLeftEigenVectors (Model/SubstitutionModel.h:498-525)
 *   plk_update_pmatrices
 *       AbstractHomogeneousTreeLikelihood::computeTransitionProbabilitiesForNode
 *       (Likelihood/AbstractHomogeneousTreeLikelihood.cpp:354-414) and
 *       AbstractSubstitutionModel::getPij_t / getdPij_dt / getd2Pij_dt2
 *       (Model/AbstractSubstitutionModel.cpp:426-641); NH twin
 *       Likelihood/AbstractNonHomogeneousTreeLikelihood.cpp:407-470
 *   plk_set_pmatrix
 *       closed-form getPij_t models computed on the host (T92::getPij_t,
 *       Model/Nucleotide/T92.cpp:355-386) copied into pxy_
 *   plk_update_partials
 *       RHomogeneousTreeLikelihood::computeSubtreeLikelihood
 *       (Likelihood/RHomogeneousTreeLikelihood.cpp:802-863); NH twin
 *       Likelihood/RNonHomogeneousTreeLikelihood.cpp:1286-1350
 *   plk_root_loglik
 *       RHomogeneousTreeLikelihood::getLogLikelihood / getLogLikelihoodForASite /
 *       getLikelihoodForASiteForARateClass (Likelihood/RHomogeneousTreeLikelihood.cpp:162-216);
 *       NH Likelihood/RNonHomogeneousTreeLikelihood.cpp:168-233
 *
 * Conventions
 *   - Node indices: tips are [0, n_tips), internal nodes [n_tips, n_tips + n_internal).
 *     The transition matrix of a branch is indexed by its CHILD node index.
 *   - Matrices are row-major fp64; P[c][x][y] = Prob(y at child | x at parent).
 *   - Host buffers are borrowed for the duration of the call only; device buffers
 *     are owned by the handle.  One handle per host thread.  All work is ordered
 *     on the handle's HIP stream; plk_root_loglik and plk_get_* synchronise.
 *   - Every function returns PLK_OK (0) or a negative PLK_ERR_* code; the
 *     message of the last error is available from plk_last_error().  No C++
 *     exception crosses this boundary.
 *   - There is no CPU fallback: plk_create fails with PLK_ERR_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef PLK_H
#define PLK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: plk_timing gained `evaluations` and `host_us` (a caller built against 1 must not pass
 * its smaller struct to plk_get_timing_ex).  Added entry points (the plk_pars_* calls, then
 * plk_simulate and plk_sim_*) change no struct or signature and leave the version as it is. */
#define PLK_ABI_VERSION 2

enum {
  PLK_OK = 0,
  PLK_ERR_ARG = -1,         /* bad argument (index out of range, null pointer, size) */
  PLK_ERR_DEVICE = -2,      /* HIP runtime / device error or no usable GPU */
  PLK_ERR_OOM = -3,         /* device allocation failed */
  PLK_ERR_UNSUPPORTED = -4, /* state count / class count / flag not supported */
  PLK_ERR_STATE = -5,       /* call order violated (e.g. partials before P matrices) */
  PLK_ERR_BAD_CODE = -6     /* tip code outside the code table (BadIntException) */
};

/* plk_create flags */
enum {
  PLK_FLAG_SCALING = 1u << 0,    /* exact power-of-two per-pattern rescaling (deviation,
                                    needed where the reference underflows).  Every stored L
                                    and U has its joint maximum over classes and states in
                                    [2^-256, 1]: a check multiplies the vector by 2^256 until
                                    it is, and counts the steps.  A node's sons are taken
                                    three at a time; the running product is checked after
                                    each group, at the node's end and, from the second group
                                    on, after the group's second son, so at most three such
                                    vectors enter it between two checks and it stays above
                                    2^-768.  For PLK_OP_ACCUMULATE ops that is a check after
                                    the op's second son and one at every op's end; every
                                    traversal path checks at the same sons, so stored values
                                    and counts agree across them. */
  PLK_FLAG_NONNEG_GUARD = 1u << 1 /* homogeneous root guards: drop terms <= 0
                                    (RHomogeneousTreeLikelihood.cpp:197-198,212-213);
                                    without it the NH rule clamps l<0 -> 0
                                    (RNonHomogeneousTreeLikelihood.cpp:206) */,
  PLK_FLAG_LNL_ONLY = 1u << 2,   /* 4-state fused traversal keeps interior partials in
                                    registers and materialises only fragment roots; other
                                    partials are recomputed on demand by plk_get_partials */
  PLK_FLAG_LEVELWISE = 1u << 3,  /* force one launch per tree level (every child partial
                                    re-read from HBM); for A/B measurements */
  PLK_FLAG_SUBTREE_PATTERNS = 1u << 4 /* per-subtree site-pattern compression, the reference's
                                    usePatterns = true (DRASRTreeLikelihoodData.cpp:218-332):
                                    each internal node is computed once per distinct pattern of
                                    its subtree and read through pattern links.  Links are
                                    built on the host from the tip codes and the op list (all
                                    internal children must be produced by the same call); any
                                    state count, polytomies of any degree */,
  PLK_FLAG_DOUBLE_RECURSIVE = 1u << 5 /* DRHomogeneousTreeLikelihood: keep one "upper" conditional
                                    likelihood per branch (the reference's father-side arrays,
                                    DRHomogeneousTreeLikelihood.cpp:543-651) so that
                                    plk_all_branch_derivatives serves every branch from one
                                    preorder pass; n_nodes extra partial slots in HBM */
};

/* plk_update_pmatrices deriv_mask */
enum { PLK_DERIV_P = 1u, PLK_DERIV_DP = 2u, PLK_DERIV_D2P = 4u };

/* plk_op flags */
enum { PLK_OP_ACCUMULATE = 1 /* multiply into the parent's existing partial (polytomies) */ };

/* One partial update: parent = prod_k (P_branch(child_k) . L_child_k).
 * Ops handed to one plk_update_partials call must be in postorder; the engine
 * batches consecutive independent ops into one launch. */
typedef struct plk_op {
  int32_t parent;
  int32_t n_children; /* 1..3 */
  int32_t child[3];
  int32_t flags;
} plk_op;

typedef struct plk_handle_s* plk_handle;

/* Library / device */
int plk_abi_version(void);
/* First 16 hex digits of the SHA-256 of the library's sources (the .hip and .hpp files of csrc in
 * sorted order, then this header), fixed at compile time: lets a caller check that the
 * loaded binary was built from the sources it ships with. */
const char* plk_build_id(void);
int plk_device_count(int* count);
const char* plk_last_error(plk_handle h); /* h may be NULL: last global error */

/* Create an engine instance on HIP device `device`.  (Several devices: plk_create_multi
 * below; several processes: plk_comm_init.)
 *   n_states: 2..64, n_classes: 1..16, n_patterns >= 1 (padded internally),
 *   n_models: number of eigen systems (1 for homogeneous; one per branch for NH). */
int plk_create(int device, int n_states, int n_classes, int64_t n_patterns, int n_tips, int n_internal,
               int n_models, unsigned flags, plk_handle* out);
int plk_destroy(plk_handle h);

/* Multi-GPU at the boundary (SURVEY 8(b) device_mask, 8(e)).  Site patterns are
 * independent, so a run is sharded into contiguous pattern ranges whose boundaries are
 * multiples of plk_block_size(); each device evaluates its range with no traffic during
 * the traversal, and the only exchange of an evaluation is the fixed-order block sums of
 * the root reduction, summed in global block order -- the lnL is bitwise identical for any
 * device count.
 *
 * One process, several devices: plk_create_multi takes the device list (a device may be
 * listed twice: two shards on one GPU, for tests) and the TOTAL pattern count; the handle
 * it returns accepts every call of this header with whole-alignment arguments (tip codes,
 * weights, per-pattern outputs span all patterns) and fans them out: every shard after the
 * first has a persistent host worker thread (the caller's thread runs the first), so the
 * shards' launch calls and stream waits run side by side; each device's block sums arrive in
 * mapped host memory and the caller sums them in global order (the result is needed on the
 * host, so an in-process collective would only add a hop).  Derivatives are summed over
 * shards in shard order.  Timing and plk_kernel_path report shard 0; plk_traversal_work sums
 * the shards. */
int plk_create_multi(const int* devices, int n_devices, int n_states, int n_classes, int64_t n_patterns, int n_tips,
                     int n_internal, int n_models, unsigned flags, plk_handle* out);
int plk_shard_count(plk_handle h, int* n_shards);
/* Fan-out of a multi-device handle's plk_evaluate calls since plk_reset_timing: for each of its
 * n_shards shards (plk_shard_count), the mean offset in microseconds from the caller posting
 * the evaluation to [3i] the shard's worker starting it, [3i+1] its traversal launch call
 * returning and [3i+2] its completion wait returning; spread_us[0] / [1] = mean / max over the
 * evaluations of the last minus the first shard's traversal launch.  A single-device handle
 * reports zeros (n_shards = 1). */
int plk_get_fanout(plk_handle h, int n_shards, double* offsets_us, double* spread_us, int64_t* evaluations);

/* One process per GPU (torch.distributed / MPI launch): rank r creates its handle with
 * plk_create for ITS pattern range, one rank gets an id with plk_comm_get_id and shares
 * it (any channel), and every rank calls plk_comm_init.  From then on plk_root_loglik and
 * plk_evaluate all-gather every rank's block sums over RCCL (xGMI) on the handle's stream
 * -- one fixed-size ncclAllGather per evaluation -- and return the GLOBAL lnL on every
 * rank (block_sums / site_lnl stay per rank).  Ranks must hold consecutive pattern ranges
 * in rank order with block-aligned boundaries.  Replaces nothing in the reference (which
 * is single-threaded); it is the single reduce north_star names. */
typedef struct plk_comm_id {
  char internal[128];
} plk_comm_id;
int plk_comm_get_id(plk_comm_id* id);
int plk_comm_init(plk_handle h, int n_ranks, int rank, const plk_comm_id* id);

/* The exchange's host-side bookkeeping, the same code the communicator path runs
 * (csrc/plk_exchange.hpp); host only, no GPU needed -- for callers with their own
 * collective (MPI, gloo) and for the CPU tests.  Rank r's record is `stride` doubles:
 * its block sums, zero padding, its underflow flag (1.0 / 0.0); stride = max block
 * count + 1.  reduce: the global lnL as ONE chain of adds in rank order then block order
 * (the one-process fixed-order sum of RNonHomogeneousTreeLikelihood.cpp:168-182, bitwise
 * for any rank count) and the OR of the flags.  rank_sums: v[i] = sum over ranks in rank
 * order of gathered[r * n + i] (the derivative sums). */
int plk_exchange_stride(const int64_t* counts /* n_ranks */, int n_ranks, int64_t* stride);
int plk_exchange_pack(const double* block_sums, int64_t n_blocks, int uflow, int64_t stride,
                      double* record /* stride */);
int plk_exchange_reduce(const double* gathered /* n_ranks x stride */, const int64_t* counts, int n_ranks,
                        int64_t stride, double* lnl, int* uflow);
int plk_exchange_rank_sums(const double* gathered /* n_ranks x n */, int n_ranks, int64_t n, double* v /* n */);

/* Data */
int plk_set_code_table(plk_handle h, int n_codes, const double* code_to_vec /* n_codes x S */);
int plk_set_tip_codes(plk_handle h, int tip, const uint8_t* codes /* n_patterns */);
int plk_set_pattern_weights(plk_handle h, const double* weights /* n_patterns */);
int plk_set_category_rates(plk_handle h, const double* rates /* C */, const double* probs /* C */);
int plk_set_root_frequencies(plk_handle h, const double* pi /* S */);

/* Models and transition matrices */
int plk_set_eigen(plk_handle h, int model, const double* V /* S x S */, const double* Vinv /* S x S */,
                  const double* lambda /* S */);
/* For each i < n: branch[i] (a child node index) gets P = V_m exp(lambda_m * r_c * t_i) Vinv_m
 * for every class c, with m = model[i] (model may be NULL: model 0).  Optional
 * first/second derivatives follow the reference: dP = r_c dP/dt, d2P = r_c^2 d2P/dt2. */
int plk_update_pmatrices(plk_handle h, int n, const int32_t* branch, const int32_t* model,
                         const double* t, unsigned deriv_mask);
int plk_set_pmatrix(plk_handle h, int branch, const double* P /* C x S x S */);
int plk_get_pmatrix(plk_handle h, int branch, double* P /* C x S x S */);
/* The derivative matrices plk_update_pmatrices stored with PLK_DERIV_DP (order 1: r_c dP/dt)
 * or PLK_DERIV_D2P (order 2: r_c^2 d2P/dt2) -- the reference's getdPij_dt / getd2Pij_dt2
 * (Model/AbstractSubstitutionModel.cpp:499-641) scaled as computeTransitionProbabilitiesForNode
 * stores them (Likelihood/AbstractHomogeneousTreeLikelihood.cpp:375-413). */
int plk_get_dpmatrix(plk_handle h, int branch, int order, double* dP /* C x S x S */);

/* Partials */
int plk_update_partials(plk_handle h, const plk_op* ops, int n_ops);
int plk_get_partials(plk_handle h, int node, double* out /* n_patterns x C x S, reference order */);

/* Root reduction.  lnl = sum_p w_p log(sum_c prob_c sum_s pi_s L_root[p][c][s]).
 * site_lnl (nullable) receives the per-pattern log-likelihoods (n_patterns).
 * block_sums (nullable) receives the per-4096-pattern-block weighted sums in
 * pattern order (ceil(n_patterns / 4096) values): summing them in a fixed order
 * gives a result independent of how patterns are sharded across devices. */
int plk_root_loglik(plk_handle h, int root, double* lnl, double* site_lnl, double* block_sums);

/* Underflow check of an UNSCALED handle (created without PLK_FLAG_SCALING): *flag = 1 when the
 * last root reduction (plk_evaluate, plk_root_loglik, or a fused traversal's) met a site
 * likelihood below 2^-255, or <= 0, or NaN; 0 otherwise.  Call it after the evaluation
 * returned (plk_evaluate and plk_root_loglik synchronise).  A 0 proves that a handle with
 * PLK_FLAG_SCALING would have returned bitwise the same lnL: partials are <= 1 and every
 * node's joint maximum over (class, state) is <= each of its children's (P rows sum to 1), and
 * a site's likelihood is <= its root's joint maximum, so every node's maximum was >= 2^-255
 * (one bit of rounding margin above the 2^-256 rescaling threshold) and no rescale would have
 * fired.  The Bio++ mirror evaluates unscaled first and falls back to a scaled handle only when
 * the flag is set.  Under a communicator the flag is global (every rank's, carried in the
 * block-sum all-gather), so all ranks take the same fallback decision.  PLK_ERR_STATE on a
 * scaled handle.  Replaces nothing in the reference, which has no scaling. */
int plk_root_underflow(plk_handle h, int* flag);

/* Diagnostic (PLK_DEBUG_CLOCK=1 when the traversal kernel is generated): every jit_tree4
 * workgroup stamps the shader clock counter and the constant 100 MHz counter at its start and
 * end, and each evaluation leaves one record of 5 doubles: the shader clock in MHz over all
 * workgroups, the slowest and fastest workgroup's MHz, the traversal's first-start-to-last-end
 * span in us, and the workgroup count.  *n = records held; up to cap are copied to out, and
 * the held records are cleared when all fit.  Replaces nothing in the reference. */
int plk_clock_records(plk_handle h, double* out /* cap x 5 */, int cap, int* n);

/* Diagnostic (PLK_DEBUG_CLOCK=3): the waves of the last traversal that a root reduction
 * summarised, two doubles each -- the wave's loop time in shader-clock ticks and the tasks (or
 * super-block rounds) it walked; 0, 0 for a wave that walked none.  Stamp order: wave w of
 * workgroup k at k * *waves_per_wg + w, the workgroups of a launch x-fastest with *wgs_x of them
 * per fragment and class (the last launch's, where tiers differ).  *n = waves held; up to cap are
 * copied to out.  They stay until the next summarised traversal.  Replaces nothing in the
 * reference. */
int plk_clock_waves(plk_handle h, double* out /* cap x 2 */, int cap, int* n, int* waves_per_wg, int* wgs_x);

/* Diagnostic (PLK_DEBUG_CLOCK=3, one class per workgroup): the same waves in the same order, one
 * double each -- the wave's task tail in shader-clock ticks, summed over its tasks: from the end
 * of a task's last contraction (in front of the root reduction and the rotation of the
 * prefetched codes) to the top of the next task, or to the end of the loop.  The kernel's record
 * keeps its four 64-bit words per wave: the tail travels in the fourth, above the rounds' 24
 * bits.  *n = waves held; up to cap are copied to out.  Replaces nothing in the reference. */
int plk_clock_wave_tails(plk_handle h, double* out /* cap */, int cap, int* n);

/* One likelihood evaluation as RHomogeneousTreeLikelihood::fireParameterChanged does it
 * (Likelihood/RHomogeneousTreeLikelihood.cpp:255-283): P(t) of the listed branches
 * (plk_update_pmatrices, P only), the postorder traversal (plk_update_partials) and the
 * root reduction (plk_root_loglik without per-site output), in one call. */
int plk_evaluate(plk_handle h, int n, const int32_t* branch, const int32_t* model, const double* t,
                 const plk_op* ops, int n_ops, int root, double* lnl, double* block_sums);

/* First and second derivatives of lnL with respect to the length of `branch` (a child
 * node index) for the tree of the last plk_update_partials call:
 *   d1 = d lnL / dt,  d2 = d2 lnL / dt2   (the reference's getFirstOrderDerivative
 *   returns -d1, RHomogeneousTreeLikelihood.cpp:346-360, 596-610).
 * Requires dP and d2P of the branch (plk_update_pmatrices with PLK_DERIV_DP | PLK_DERIV_D2P).
 * Replaces computeTreeDLikelihood / computeTreeD2Likelihood (:365-541, :615-791).
 * Any state and class count: 4 states with 1, 2 or 4 classes propagate L, dL, d2L up the
 * path in registers; other shapes recompute the path with dP / d2P substituted on the
 * branch (lnL is linear in one branch's P).  PLK_ERR_UNSUPPORTED with
 * PLK_FLAG_SUBTREE_PATTERNS. */
int plk_branch_derivatives(plk_handle h, int branch, double* d1, double* d2);
int plk_block_size(void);

/* Directional derivatives for two sons a, b of the traversal's root whose lengths move
 * together, t_a + alpha s and t_b + beta s:  d1 = d lnL/ds, d2 = d2 lnL/ds2 at s = 0
 * (d2 includes the mixed term 2 alpha beta d2 lnL/(dt_a dt_b)).  The reference's root
 * reparametrisation of a rooted non-homogeneous tree (reparametrizeRoot = true,
 * Likelihood/AbstractNonHomogeneousTreeLikelihood.cpp:312-330, 377-389) uses
 *   BrLenRoot:    alpha = RootPosition, beta = 1 - RootPosition
 *   RootPosition: alpha = BrLenRoot,    beta = -BrLenRoot
 * and replaces computeTreeDLikelihood / computeTreeD2Likelihood for those two variables
 * (Likelihood/RNonHomogeneousTreeLikelihood.cpp:391-560, 862-1100).  Requires dP and d2P of
 * both branches.  Any state and class count.
 * Under an RCCL communicator (plk_comm_init) this, plk_branch_derivatives and
 * plk_all_branch_derivatives return GLOBAL values on every rank: each rank's d1 and d2 are
 * all-gathered (one fixed-size ncclAllGather on the handle's stream) and summed in rank
 * order, so every rank holds the same doubles.  A multi-device handle (plk_create_multi)
 * returns the sum over its devices in shard order. */
int plk_root_pair_derivatives(plk_handle h, int a, int b, double alpha, double beta, double* d1, double* d2);

/* Double-recursive derivatives (handle created with PLK_FLAG_DOUBLE_RECURSIVE): d lnL/dt and
 * d2 lnL/dt2 for EVERY branch of the last plk_update_partials tree, written to d1[node] and
 * d2[node] (n_nodes entries each, 0 at the root).  One preorder pass computes each branch's
 * upper vector U_v (everything outside v's subtree, conditional on the state at v's father,
 * root frequencies folded in), then per branch and pattern
 *   l = sum_c p_c sum_y U_v[c][y] (P_v L_v)[c][y],  l' and l'' with r_c dP_v and r_c^2 d2P_v,
 *   d1 += w l'/l,  d2 += w (l''/l - (l'/l)^2).
 * Replaces DRHomogeneousTreeLikelihood::computeSubtreeLikelihoodPrefix (:543-651),
 * computeTreeDLikelihoodAtNode / computeTreeDLikelihoods (:287-338) and the D2 twins
 * (:373-423).  Requires dP and d2P of every branch.  Any state count the partial kernels
 * support; not with PLK_FLAG_SUBTREE_PATTERNS. */
int plk_all_branch_derivatives(plk_handle h, double* d1, double* d2);

/* Marginal posteriors of internal nodes for the tree of the last plk_update_partials call: per
 * pattern and node v, with up_v[c][x] = sum_y U_v[c][y] P_v[c][y][x] (pi folded in as in
 * plk_all_branch_derivatives),
 *   J_v[c][x] = p_c up_v[c][x] L_v[c][x]   (the root: p_c pi_x L_r[c][x]),   l = sum_c sum_x J_v[c][x],
 *   joint = J / l,  state_post[x] = sum_c joint,  class_post[c] = sum_x joint,
 *   best_state = the lowest index among the maxima of state_post.
 * Each output may be NULL (not all four).  A pattern whose l is not a positive finite number (an
 * unscaled underflow) gets probabilities 0 and best_state 255; no error is reported.  Scale
 * counts cancel in J / l, so scaled and unscaled handles answer alike.
 * Replaces MarginalAncestralStateReconstruction::getAncestralStatesForNode
 * (Likelihood/MarginalAncestralStateReconstruction.cpp), DRTreeLikelihoodTools::
 * getPosteriorProbabilitiesForEachStateForEachRate (Likelihood/DRTreeLikelihoodTools.cpp) and
 * AbstractDiscreteRatesAcrossSitesTreeLikelihood::getPosteriorProbabilitiesOfEachRate
 * (Likelihood/AbstractDiscreteRatesAcrossSitesTreeLikelihood.cpp).  Deviation: p_c is always in J
 * (the true posterior); DRTreeLikelihoodTools leaves it out at internal nodes, which is the same
 * thing whenever the class probabilities are equal.
 * Preconditions and error codes are those of plk_all_branch_derivatives; its preorder pass is run
 * here, unless no P(t), partial, tip code, pi or rate has changed since the last one.  A request that names only the root needs none of them -- no PLK_FLAG_DOUBLE_RECURSIVE,
 * no dP/d2P, no preorder pass, any traversal mode -- and leaves plk_kernel_path, the partials and
 * the next plk_root_loglik as they were (after an lnL-only traversal the partials are written as
 * plk_get_partials does, then the traversal is run once more as it was).
 * PLK_ERR_ARG: a tip, an index out of range, a node outside the current tree, n_nodes <= 0, all
 * outputs NULL.  A multi-device handle fills the caller's arrays shard by shard (bitwise the
 * single-device result); under a communicator a rank returns its own patterns, with no
 * collective call.  Device staging is bounded (256 MiB): longer node lists run in chunks. */
int plk_node_posteriors(plk_handle h, int n_nodes, const int32_t* nodes,
                        double* joint /* n_nodes x n_patterns x C x S, or NULL */,
                        double* state_post /* n_nodes x n_patterns x S, or NULL */,
                        double* class_post /* n_nodes x n_patterns x C, or NULL */,
                        uint8_t* best_state /* n_nodes x n_patterns, or NULL */);

/* Probabilistic substitution mapping: the posterior expected number of substitutions of each
 * type, on each branch, at each pattern.  A type k (1..T) of a model is a matrix B_k with zero
 * diagonal: B_k[x][y] = Q[x][y] (times an optional weight) where the register puts x -> y in
 * type k, 0 elsewhere (DecompositionSubstitutionCount::fillBMatrices_).  With tau = r_c t_v and
 * the real eigen system (V, Vinv, lambda) of plk_set_eigen,
 *   G_k = Vinv B_k V,   J[i][j] = int_0^tau exp(lambda_i s) exp(lambda_j (tau - s)) ds,
 *   W^k_{v,c} = V (J o G_k) Vinv = int_0^tau e^{Qs} B_k e^{Q(tau-s)} ds     (o: elementwise),
 * W^k[x][y] = E[count of type k, end state y | start state x], the reference's
 * getAllNumbersOfSubstitutions(tau, k)[x][y] * P(tau)[x][y].  Per branch v (a child node index,
 * tips included), pattern and type, with u = U_v (pi folded in as in plk_node_posteriors),
 *   l   = sum_c p_c sum_xy u[c][x] P_v[c][x][y]   L_v[c][y],
 *   n_k = sum_c p_c sum_xy u[c][x] W^k_{v,c}[x][y] L_v[c][y],      count[v][p][k] = n_k / l.
 * Scale counts multiply n_k and l alike and are never read.
 * Replaces SubstitutionMappingTools::computeSubstitutionVectors (Mapping/
 * SubstitutionMappingTools.cpp:63-372) over DecompositionSubstitutionCount / DecompositionMethods
 * (Mapping/DecompositionMethods.cpp:88-165).  Deviations:
 *   - J is formed as tau exp(max(lambda_i, lambda_j) tau) phi(-|lambda_i - lambda_j| tau),
 *     phi(z) = expm1(z) / z, phi(0) = 1.  The reference's (e_i - e_j) / (lambda_i - lambda_j)
 *     with an exact == 0 test (:112-125) cancels catastrophically for nearly equal eigenvalues,
 *     which is what a numeric eigensolver returns for K80- / HKY-like models.
 *   - An entry of W that rounding leaves below 0 counts as 0.  The reference zeroes negative,
 *     infinite and NaN quotients N = W / P (DecompositionSubstitutionCount.cpp:100-114); where
 *     P > 0 the two agree.
 *   - A pattern whose l is not a positive finite number (an unscaled underflow) gets counts 0
 *     and no error, as the posteriors do.
 *   - Real eigen systems only.
 *
 * plk_set_count_types: T types for model `model`; B is T x S x S.  T is 1..16 and is fixed per
 * handle by the first call of plk_set_count_types or plk_set_count_matrix: later calls with
 * another T are PLK_ERR_ARG.  Forms G_k (again after a later plk_set_eigen of the model). */
int plk_set_count_types(plk_handle h, int model, int n_types, const double* B);

/* As plk_update_pmatrices: W^k_{branch,c} for every listed branch, class and type, from the
 * eigen system.  t = 0 gives W = 0.  PLK_ERR_STATE if the model has no types.  Count matrices
 * are no input of L or U: the preorder pass is not run again because of them. */
int plk_update_count_matrices(plk_handle h, int n, const int32_t* branch, const int32_t* model, const double* t);

/* Host-computed counts (naive, Laplace, uniformisation: N o P, already times P), as
 * plk_set_pmatrix; plk_get_count_matrix reads a branch's matrices back.  W lives on the device
 * as [n_nodes][T][C][S][S], allocated by the first count-matrix call (PLK_ERR_OOM). */
int plk_set_count_matrix(plk_handle h, int branch, int n_types, const double* W /* T x C x S x S */);
int plk_get_count_matrix(plk_handle h, int branch, double* W /* T x C x S x S */);

/* counts[b][p][k] for the listed branches of the last plk_update_partials tree, and
 * totals[b][k] = sum_p w_p counts[b][p][k], summed per plk_block_size() patterns on the device
 * and over the blocks in pattern order on the host (the root reduction's rule, so the value does
 * not depend on sharding).  Either output may be NULL (not both); without `counts` no
 * per-pattern row is written.  Preconditions and error codes follow plk_all_branch_derivatives
 * and plk_node_posteriors: PLK_ERR_STATE without PLK_FLAG_DOUBLE_RECURSIVE, before a traversal,
 * without dP / d2P, or for a branch without a count matrix; PLK_ERR_UNSUPPORTED with
 * PLK_FLAG_SUBTREE_PATTERNS; PLK_ERR_ARG for the root, an index out of range, a node outside the
 * current tree, n_branches <= 0 or both outputs NULL.  The preorder pass runs only if a P(t),
 * partial, tip code, pi or rate has changed since the last one; the upper vectors of requested
 * tip branches, which that pass does not keep, are formed once per such change.  A multi-device
 * handle fills `counts` shard by shard and adds block totals in global block order (both outputs
 * bitwise the single-device ones); under a communicator a rank returns its own patterns and
 * totals, with no collective call.  Device staging of `counts` is bounded (256 MiB): longer
 * branch lists run in chunks. */
int plk_branch_counts(plk_handle h, int n_branches, const int32_t* branches,
                      double* counts /* n_branches x n_patterns x T, or NULL */,
                      double* totals /* n_branches x T, or NULL */);

/* Nearest-neighbour interchanges of the last plk_update_partials tree, scored with the length of
 * the move's branch re-estimated.  A move is (son s, uncle u): p is the father of s, g the father
 * of p and u another son of g; s and u change places and branch p gets the length t.  Per
 * pattern and class, with q_v = P_v L_v (a tip: its code row), up_g = pi at the root and else
 * sum_y u_g[y] P_g[y][x] with u_g = U_g (pi folded in as in plk_node_posteriors),
 *   A1 = up_g q_s prod_{o son of g, o not p, u} q_o,   A2 = q_u prod_{o son of p, o not s} q_o,
 *   B1 = up_g q_u prod_o q_o,  B2 = q_s prod_o q_o,    l_cur = sum_c p_c B1^T P_p B2,
 * and with the real eigen system (V, Vinv, lambda) of `model` (that of branch p),
 *   gamma[c][k] = p_c (A1^T V)[k] (Vinv A2)[k] / l_cur,
 *   rho(t)   = sum_c sum_k gamma[c][k] exp(lambda_k r_c t),
 *   delta(t) = sum_p w_p log rho(t) = lnL(swapped tree, branch p of length t) - lnL(current tree),
 *   d1 = sum_p w_p rho'/rho,   d2 = sum_p w_p (rho''/rho - (rho'/rho)^2).
 * l_cur and gamma come from the same stored vectors, so scale counts cancel and are never read.
 * Before the product an exact power of two (the exponent of its joint maximum over classes and
 * states) is taken out of each of those vectors -- U_g and the L of s, u, the third son of g and
 * the other sons of p -- so the product of four to six vectors that PLK_FLAG_SCALING leaves
 * anywhere in [2^-256, 1) stays a normal double; l_cur, gamma and d share the factor and results
 * are bitwise those of the plain product wherever that one did not underflow.
 * The matrix-vector products are paid once per move; every trial length is one streaming pass
 * over C S + 2 coefficients per pattern.  While t max|lambda_k r_c| <= 1, rho is summed as
 * d + sum gamma expm1(lambda r t) with d = sum_c p_c A1 . A2 / l_cur = sum gamma, which is formed
 * without a subtraction: where the two sides of a move disagree rho is small against the gamma
 * it is summed from, and at t = 1e-6 the plain sum lost six digits of d1 on 20 states.
 *
 * max_iter == 0: every move is evaluated at t0 (t_opt = t0; status 0).  max_iter > 0: a
 * safeguarded Newton ascent, all moves in lockstep, at most max_iter evaluation passes after the
 * first.  From a point (t, F, d1, d2) the proposal is t' = t - d1 / d2 when d2 < 0, else 2 t when
 * d1 > 0, else t / 2, clamped to [t_min, t_max]; after a rejected trial it is the midpoint of t
 * and that trial.  A move is converged when |t' - t| <= tol max(t, t_min) and then drops out of
 * the later passes; otherwise t' is evaluated and accepted when F(t') >= F(t).  That comparison
 * is taken on F(t') - F(t) = sum_p w_p log1p((rho(t') - rho(t)) / rho(t)), summed per pattern in
 * the same pass from rho(t') - rho(t) = sum gamma exp(lambda r t) expm1(lambda r (t' - t)): near
 * the optimum a step changes F by less than the rounding of F itself, and the difference of two
 * sums of logs would let rounding decide.  t_opt, d1 and d2 are those of the last accepted
 * point and delta is delta(t0) plus the accepted changes, so delta >= delta(t0) and delta is
 * delta(t_opt) (to rounding).
 * status: 0 converged, 1 iteration budget spent.  t0 is required: the engine stores P(t), not t.
 * The three sums are formed per plk_block_size() patterns on the device in fixed order and over
 * the blocks in pattern order on the host (the root reduction's rule), and every decision is
 * taken on them, so no result depends on sharding.
 *
 * Replaces NNIHomogeneousTreeLikelihood::testNNI (Likelihood/NNIHomogeneousTreeLikelihood.cpp:
 * 205-309) and its BranchLikelihood (:93-120), for every move of a round of NNITopologySearch
 * (NNITopologySearch.cpp:97-212) at once.  Deviations:
 *   - Newton to `tol` in the place of Brent at tolerance 0.1: t_opt is closer to the optimum and
 *     delta at least as large.  The reference returns -delta.
 *   - A pattern whose l_cur or rho is not a positive finite number adds 0 to all three sums and
 *     raises no error, as posteriors and mapping have it.  With the powers of two taken out as
 *     above, l_cur is zero only where one of the stored vectors is zero in every class and
 *     state: a pattern the traversal itself lost (an underflow of a handle without
 *     PLK_FLAG_SCALING; -inf or 0 weight in plk_root_loglik's site_lnl) or one the data make
 *     impossible on the current tree.  No product of stored vectors that are each representable
 *     drops a pattern; l_cur is never a denormal number short of that.
 *   - Real eigen systems only; p and g of at most three sons.
 * PLK_ERR_STATE without PLK_FLAG_DOUBLE_RECURSIVE, before a traversal, without dP / d2P (the
 * preorder pass demands them) or for a model without an eigen system; PLK_ERR_UNSUPPORTED with
 * PLK_FLAG_SUBTREE_PATTERNS, under a communicator, or when p or g has more than three sons;
 * PLK_ERR_ARG when s is the root or a son of the root, u is not a son of g other than p, an index
 * is out of range or outside the current tree, n_moves <= 0, t_min <= 0, t_max < t_min or a t0
 * outside the bounds.  The preorder pass runs only if a P(t), partial, tip code, pi or rate has
 * changed since the last one; the call changes no partial, U, P(t), plk_kernel_path or the next
 * plk_root_loglik.  Device staging of the coefficients is bounded (2 GiB): longer move lists
 * run in chunks, each built and then optimised.  A multi-device handle builds and evaluates
 * shard by shard and the parent drives the Newton loop over the block sums in global block order
 * (bitwise the single-device result). */
int plk_nni_scores(plk_handle h, int n_moves, const int32_t* son, const int32_t* uncle,
                   const int32_t* model /* n_moves, or NULL: model 0 */,
                   const double* t0 /* n_moves */,
                   double t_min, double t_max, double tol, int max_iter,
                   double* t_opt, double* delta, double* d1, double* d2 /* each n_moves; d1, d2 nullable */,
                   int32_t* status /* n_moves, nullable */);
/* Evaluation passes of the last plk_nni_scores on this handle (the first pass of every chunk
 * included). */
int plk_nni_passes(plk_handle h, int64_t* passes);

/* RELL resampling (resampling of estimated log-likelihoods): per-pattern log-likelihood rows kept
 * on the device, replicate weights, and the product of the two.  Replaces the triple host loop of
 * PairedSiteLikelihoods::computeExpectedLikelihoodWeights (Likelihood/PairedSiteLikelihoods.cpp:
 * 124-176; the counts of ::bootstrap, :178-188): Y += lnL[model][site] * count[site] for every
 * replicate and model is G = W . L^T.
 *
 * A site row is a device vector of n_patterns doubles (padding 0.0).  Rows belong to the handle
 * and are numbered from 0.  plk_site_rows_reserve allocates n_rows of them, all 0.0 (the rows of
 * an earlier reservation are lost); 0 frees them.  PLK_ERR_OOM, PLK_ERR_ARG for n_rows < 0.
 * plk_site_row_set / _get move n_patterns host values (a multi-device handle scatters / gathers by
 * shard); PLK_ERR_ARG for a row that is not reserved, here and in every call below. */
int plk_site_rows_reserve(plk_handle h, int n_rows);
int plk_site_row_set(plk_handle h, int row, const double* v /* n_patterns */);
int plk_site_row_get(plk_handle h, int row, double* v /* n_patterns */);
/* The row receives what plk_root_loglik returns in site_lnl for the current partials: the same
 * kernels, the same values bitwise (scale counts included), nothing through the host.  A
 * non-finite value (an underflowed pattern) is stored as 0.0 and counted in *n_bad (nullable),
 * the rule of posteriors, mapping and NNI.  Leaves plk_kernel_path, plk_root_underflow and the
 * next plk_root_loglik as they were.  Errors of plk_root_loglik; PLK_ERR_UNSUPPORTED under a
 * communicator. */
int plk_site_row_from_root(plk_handle h, int root, int row, int64_t* n_bad);
/* Row first_row + i receives log rho_i(t_i) per pattern for the move (son[i], uncle[i]): exactly
 * the terms plk_nni_scores weights and sums into delta at max_iter == 0, t0 = t (the same
 * coefficient build, the same short-length expm1 form under the same condition); a pattern whose
 * l_cur or rho is not a positive finite number gets 0.0 -- as in plk_nni_scores only a pattern
 * that the traversal itself lost (a stored vector of zeros), never one whose stored vectors are
 * each representable and merely small.  So lnL_site(swapped tree, branch p of
 * length t_i) = lnL_site(current tree) + row.  Preconditions, error codes, the reuse of an
 * up-to-date preorder pass, the staging bound (2 GiB, PLK_TUNE NNI_CAP_KB) and multi-device
 * behaviour are those of plk_nni_scores; t_i must be positive and finite (PLK_ERR_ARG). */
int plk_nni_site_rows(plk_handle h, int n_moves, const int32_t* son, const int32_t* uncle,
                      const int32_t* model /* n_moves, or NULL: model 0 */, const double* t /* n_moves */,
                      int first_row);
/* R replicates of per-pattern weights, replicate-major (R x n_patterns), copied to the device
 * (padding 0.0); R == 0 frees them.  Any finite weights: integer counts are the bootstrap,
 * Dirichlet weights the Bayesian bootstrap.  Independent of plk_set_pattern_weights and read by
 * plk_replicate_sums only. */
int plk_set_replicate_weights(plk_handle h, int R, const double* W /* R x n_patterns */);
/* G[r][m] = sum_p W[r][p] row[first_row + m][p]; Gabs (nullable) the same sum of |W| |row|, the
 * scale a rounding bound is stated in (|G - exact| <= n_patterns 2^-53 Gabs for any order).
 * Summation rule: per plk_block_size() patterns a partial starts from +0.0 and takes the block's
 * patterns by fused multiply-add -- 32-pattern segments ascending, inside a segment q = 0..7,
 * inside q the patterns 32 seg + 8 k + q, k = 0..3 (one v_mfma_f64_16x16x4f64 per q) -- and the
 * partials of an element are added in global block order, one chain from +0.0.  A multi-device
 * handle forms the partials on all shards side by side and runs the chains shard after shard, each
 * seeded with the shard before.  So sharding, the chunking of replicates and rows that bounds
 * the staging (2 GiB; PLK_TUNE RELL_CAP_KB lowers it) and the place of a replicate or row in the
 * call change no bit of any element.  PLK_ERR_STATE without weights or rows, PLK_ERR_ARG for a
 * row range outside the reserved rows, PLK_ERR_UNSUPPORTED under a communicator or for more than
 * 65535 pattern blocks (268 M patterns) on one device -- the blocks are the third grid dimension;
 * shard a longer alignment with plk_create_multi.  Synchronises.
 * plk_replicate_passes: the block-partial launches (per shard) of the last plk_replicate_sums. */
int plk_replicate_sums(plk_handle h, int first_row, int n_rows, double* G /* R x n_rows */,
                       double* Gabs /* R x n_rows, or NULL */);
int plk_replicate_passes(plk_handle h, int64_t* launches);

/* Pairwise sufficient statistics: for every listed pair of tips the table
 *   N[pair][a][b] = sum_p w_p [code of tip_a at p = a][code of tip_b at p = b],
 * ordered (a is the code at tip_a; the table of (b, a) is the transpose), n_codes x n_codes in the
 * numbering of plk_set_code_table, zero rows and columns for codes no tip uses.  The likelihood
 * of two sequences joined by one branch depends on a pattern through its two codes only, so the
 * table is all plk_pair_distances reads.  It is formed on the device over the codes in use
 * (4096-pattern blocks into LDS bins, the blocks added in block order); padding patterns add
 * nothing.
 * Exactness: when every weight is an integer and the weights sum to less than 2^53, every
 * partial sum is exact, so the table equals an integer histogram and is bitwise independent of
 * summation order, chunking and sharding.  For other weights the sums agree to rounding only,
 * and the order in which the patterns of one block reach a bin is not fixed.
 * At most 90 codes may be in use over the uploaded tips (PLK_ERR_UNSUPPORTED beyond: the bins of
 * a workgroup are 8 U^2 bytes of LDS); the code table itself may be longer.
 * PLK_ERR_ARG: tip_a == tip_b, an index outside [0, n_tips), n_pairs <= 0, a null pointer.
 * PLK_ERR_STATE: before plk_set_code_table or the codes of a named tip.  PLK_ERR_UNSUPPORTED
 * under a communicator.  Needs no traversal, partial, P(t) or flag and changes none, nor
 * plk_kernel_path or the next plk_root_loglik.  Device staging is bounded (256 MiB; PLK_TUNE
 * PAIR_CAP_KB lowers it): longer pair lists run chunk by chunk.  On a multi-device handle every
 * shard counts its own patterns and the parent adds the tables in shard order. */
int plk_pair_counts(plk_handle h, int n_pairs, const int32_t* tip_a, const int32_t* tip_b,
                    double* counts /* n_pairs x n_codes x n_codes, caller's code numbering */);

/* Maximum-likelihood distance of every listed pair: the branch length t that maximises the
 * likelihood of the two sequences under `model` (its real eigen system V, Vinv, lambda), the
 * rate classes and pi.  With init the code table,
 *   alpha[a][k] = sum_x pi_x init[a][x] V[x][k],   beta[k][b] = sum_y Vinv[k][y] init[b][y],
 *   delta[a][b] = sum_x pi_x init[a][x] init[b][x],
 *   l_ab(t) = sum_c p_c sum_k alpha[a][k] beta[k][b] exp(lambda_k r_c t),
 *   F(t) = sum_ab N_ab log l_ab,  d1 = sum N l'/l,  d2 = sum N (l''/l - (l'/l)^2)
 * over the entries with N > 0 of the pair's table (plk_pair_counts), formed on the device and
 * never brought to the host.  While t max|lambda_k r_c| <= 1, l_ab is summed as
 * delta_ab + sum alpha beta expm1(lambda r t): for a != b it is O(t), summed from O(1) terms
 * (plk_nni_scores has the same switch).  An entry whose l is not a positive finite number adds 0
 * to all sums.
 * max_iter == 0: every pair is evaluated at its start (t_opt = t0; status 0).  max_iter > 0: the
 * ascent of plk_nni_scores, one workgroup per pair, wholly on the device -- from a point
 * (t, F, d1, d2) the proposal is t' = t - d1 / d2 when d2 < 0, else 2 t when d1 > 0, else t / 2,
 * clamped to [t_min, t_max]; after a rejected trial it is the midpoint of t and that trial.  A
 * pair is converged when |t' - t| <= tol max(t, t_min); otherwise t' is evaluated, at most
 * max_iter times after the first evaluation, and accepted when F(t') >= F(t), decided on
 * F(t') - F(t) = sum N log1p((l(t') - l(t)) / l(t)) with l(t') - l(t) from
 * expm1(lambda r (t' - t)).  t_opt, d1, d2 are those of the last accepted point, lnl is F there
 * (F(t0) plus the accepted changes): the two-sequence log-likelihood.  status: 0 converged,
 * 1 budget spent.  All sums run in a fixed order, so a pair's result does not depend on its
 * place in the list, on chunking or (integer weights) on sharding.
 * t0 == NULL: the start comes from the table on the device.  A code is resolved when its
 * code-table row has exactly one non-zero entry; g is the weight of the entries with both codes
 * resolved, d the weight of those whose states differ; t0 = d / g clamped to [t_min, t_max], or
 * t_min when g = 0.
 * Replaces DistanceEstimation::computeMatrix (Distance/DistanceEstimation.cpp:647-687) and its
 * TwoTreeLikelihood (:474-521).  Deviations: Newton to `tol` in the place of the reference's
 * optimiser; the d / g start of the reference (:671-673) compares raw characters, so an
 * ambiguity code against a state counts as a difference there and is left out here (a start
 * only); real eigen systems only.
 * PLK_ERR_ARG as plk_pair_counts, and for t_min <= 0, t_max < t_min, tol < 0, max_iter < 0, a
 * model out of range or a t0 outside the bounds.  PLK_ERR_STATE as plk_pair_counts, and before
 * the rates and pi are set or when `model` has no eigen system (only plk_set_pmatrix).
 * PLK_ERR_UNSUPPORTED as plk_pair_counts.  A multi-device handle sums the shards' tables on the
 * host and runs the ascent on its first shard.  With plk_set_timing the count launches are timed
 * as PLK_TIME_TABLES and the Newton launches as PLK_TIME_ROOT. */
int plk_pair_distances(plk_handle h, int n_pairs, const int32_t* tip_a, const int32_t* tip_b,
                       int model, const double* t0 /* n_pairs, or NULL */,
                       double t_min, double t_max, double tol, int max_iter,
                       double* t_opt, double* lnl, double* d1, double* d2 /* each n_pairs; d1, d2 nullable */,
                       int32_t* status /* n_pairs, nullable */);
/* Evaluation passes of the slowest pair of the last plk_pair_distances on this handle. */
int plk_pair_passes(plk_handle h, int64_t* passes);

/* Maximum parsimony (Fitch, unordered states): DRTreeParsimonyScore of the reference
 * (Parsimony/DRTreeParsimonyScore.cpp, with DRTreeParsimonyData and AbstractTreeParsimonyScore),
 * all in integers.  A set is a bit mask over S_p <= 64 parsimony states; a pair is (set, score).
 * F(x_1, ..., x_k) is the reference's sequential fold (:276-311): start from x_1; for each further
 * x_j add its score and intersect the sets; where the intersection is empty take the union and add
 * 1.  The score of F does not depend on the order of its inputs, the set does, so the order below
 * is part of the definition.  For the tree of an op list (sons in the ops' order; an
 * PLK_OP_ACCUMULATE op appends its sons to the parent's):
 *   low(tip) = (mask[code], 0),   low(v) = F(low(c_1), ..., low(c_k))             (:132-182)
 *   up(v)    = F([up(f), unless f is the root], low(c) for every son c of f other than v, in
 *              order) for every internal v other than the root, f its father      (:184-238)
 *   score    = sum_p w_p low(root).score[p]                                       (:240-256)
 * and for a move (son s, uncle u), p the father of s, g the father of p, u a son of g other than p
 * (:314-383):
 *   gf = F([up(g), unless g is the root], low(o) for o son of g, o not p, o not u, in order, low(s))
 *   pp = F(low(o) for o son of p, o not s, in order, low(u), gf)
 *   delta = sum_p w_p pp.score[p] - score,
 * which is the score of the tree with s and u exchanged minus the current score wherever every
 * internal node but the root has two sons (the root: two or three); the fold is not associative,
 * so around an internal node of three sons delta is what the fold gives and no more.
 *
 * The parsimony calls keep a tree and arrays of their own (per internal node a lower and an upper
 * array of sets -- 1, 4 or 8 bytes by S_p -- and of 16-bit scores): they change no partial, P(t),
 * plk_kernel_path or later likelihood result of the handle, and need no model, rate or P(t).
 * Deliberate limit: PLK_ERR_UNSUPPORTED on a multi-device handle, under a communicator and with
 * PLK_FLAG_SUBTREE_PATTERNS -- the work is too light to need more than one device.
 *
 * plk_pars_set_code_masks: one mask per tip code of plk_set_code_table's numbering; n_states_pars
 * may differ from the handle's state count (a gap as a state of its own: S + 1).  Never called:
 * bit s of a code's mask is set where code_to_vec[code][s] != 0.  PLK_ERR_UNSUPPORTED for
 * n_states_pars > 64; PLK_ERR_ARG for a zero mask, bits at or above n_states_pars, n_codes outside
 * 1..256.  New masks, a new code table, new tip codes and new pattern weights drop the pairs of
 * an earlier plk_pars_update: the calls that read them return PLK_ERR_STATE until the next one. */
int plk_pars_set_code_masks(plk_handle h, int n_states_pars, int n_codes, const uint64_t* masks);
/* Lower pairs, upper pairs and the root of the whole tree in one kernel launch (a lane keeps its
 * patterns from the first op to the last).  Ops in postorder with at most 3 sons each, as for
 * plk_update_partials, every internal son formed by an earlier op of the same call; the last op's
 * parent is the root, which has at least two sons.  Weights are the pattern weights plk_root_loglik
 * reads; each must be a non-negative integer below 2^32 (PLK_ERR_STATE otherwise), and sums are
 * taken in uint64_t, so no result depends on the launch geometry.  PLK_ERR_STATE for a tip without
 * codes or a tip code without a mask; PLK_ERR_UNSUPPORTED for a handle of more than 65535 nodes
 * (the 16-bit scores).  Synchronises. */
int plk_pars_update(plk_handle h, const plk_op* ops, int n_ops);
/* The weighted score of the last plk_pars_update and (nullable) low(root).score per pattern. */
int plk_pars_score(plk_handle h, uint64_t* score, uint32_t* site_scores /* n_patterns, or NULL */);
/* low(node) (upper == 0; a tip is allowed) or up(node) of the last plk_pars_update; either output
 * may be NULL (not both).  PLK_ERR_ARG for up of the root or of a tip and for a node outside the
 * tree. */
int plk_pars_get_edge(plk_handle h, int node, int upper, uint64_t* sets /* n_patterns, or NULL */,
                      uint32_t* scores /* n_patterns, or NULL */);
/* delta of every listed move of the last plk_pars_update tree, one workgroup per move and pattern
 * block, one launch for all moves (DRTreeParsimonyScore::testNNI, :314-383, for every move of a
 * round of NNITopologySearch at once).  PLK_ERR_ARG as plk_nni_scores: s the root or a son of the
 * root, u not a son of g other than p, an index out of range or outside the tree, n_moves <= 0;
 * PLK_ERR_UNSUPPORTED when g has more than 8 sons or p more than 7.  Synchronises. */
int plk_pars_nni_scores(plk_handle h, int n_moves, const int32_t* son, const int32_t* uncle,
                        int64_t* delta /* n_moves */);
/* Kernel launches of the last plk_pars_update or plk_pars_nni_scores on this handle.
 * Every parsimony call: PLK_ERR_STATE before plk_pars_update (where it reads its tree). */
int plk_pars_launches(plk_handle h, int64_t* launches);

/* Simulation of an alignment under the handle's model: per site a rate class, a root state and,
 * down the tree, a state per node.  Replaces NonHomogeneousSequenceSimulator::simulate
 * (Simulation/NonHomogeneousSequenceSimulator.cpp: the cumulative tables of the constructor,
 * :110-160, the per-site walk, :306-353, and the draw, :433-483) and the host pass and copy of
 * plk_set_tip_codes that would follow it: the tip codes are written where the next traversal
 * reads them.
 *
 * The draw is a pure function of (seed, replicate, global site index, node); it depends neither
 * on the launch geometry, nor on sharding, nor on the order in which the ops describe the tree.
 *   Generator: Philox4x64-10 (Salmon et al. 2011), multipliers 0xD2E7470EE14C6C93 and
 *     0xCA5A826395121157, key increments 0x9E3779B97F4A7C15 and 0xBB67AE8584CAA73B; per round,
 *     with hi/lo of the products M0 c0 and M1 c2,  c = [hi1^c1^k0, lo1, hi0^c3^k1, lo0], the key
 *     incremented between rounds.  Counter 0, key 0 gives 16554d9eca36314c db20fe9d672d0fdc
 *     d7e772cee186176b 7e68b68aec7ba23b.
 *   Uniform number: u(site, k) = (w >> 11) * 2^-53 in [0, 1), w the word k & 3 of
 *     Philox(counter = (site, k >> 2, replicate, 0), key = (seed, 0)), site = site0 + the local
 *     index.
 *   Draw index k: 0 the site's rate class, 1 the root state, 2 + v the state of node v, for every
 *     node v of the tree other than the root.
 *   Inverse CDF: for a probability row p[0 .. n) the cumulative sums are sequential in fp64
 *     (cum[0] = p[0], cum[y] = cum[y-1] + p[y]); the drawn index is the first y with u < cum[y]
 *     (the reference's rule, :433-440) and, where there is none (rounding, a row that does not sum
 *     to 1), the largest y with p[y] > 0 (0 for a row without one).  Rows are expected
 *     non-negative.
 *   Rows: the class row is the class probabilities of plk_set_category_rates (the reference draws
 *     the class uniformly, which is the same thing for the equiprobable classes of a discretised
 *     gamma law); the root row is plk_set_root_frequencies; node v's row is P_v[c][x_father][.] as
 *     stored on the device (plk_update_pmatrices or plk_set_pmatrix, per-branch models included).
 * Two launches: the cumulative tables of the tree's branches, and one walk with a lane per site.
 *
 * Ops as for plk_pars_update: postorder, at most 3 sons per op (PLK_OP_ACCUMULATE ops append sons
 * to their father: polytomies of any degree), every internal son formed by an earlier op of the
 * same call; the last op's parent must equal `root` (PLK_ERR_ARG otherwise, and for a node of
 * two fathers or outside [0, n_nodes)).  PLK_ERR_STATE when a branch of the tree has no P(t) or
 * when the rates or the root frequencies are unset.
 *
 * flags = PLK_SIM_SET_TIPS: the state s of a tip is stored as the tip code state_code[s]
 * (state_code == NULL: state s is code s), exactly as if plk_set_tip_codes had been called for
 * every tip of the tree: every state_code[s] enters the compact numbering (in increasing code),
 * every tip counts as set, and whatever new tip codes invalidate is invalidated.  Pattern weights
 * are not touched.  PLK_ERR_STATE before plk_set_code_table, PLK_ERR_ARG for a state_code entry
 * outside the code table.  Without the flag nothing of the handle but the simulation's own
 * arrays changes.
 *
 * A multi-device handle fans the call out with each shard's site0 advanced by its first pattern,
 * so states and codes are those of one device; one process per GPU passes its rank's first site
 * as site0 and needs no communication.  Stream-ordered; synchronises before returning.  With
 * plk_set_timing the table build is timed as PLK_TIME_TABLES and the walk as PLK_TIME_PARTIALS. */
enum { PLK_SIM_SET_TIPS = 1u };
int plk_simulate(plk_handle h, const plk_op* ops, int n_ops, int root, uint64_t seed, uint64_t replicate,
                 int64_t site0, const uint8_t* state_code /* S, or NULL: state s is code s */, unsigned flags);
/* The states (indices 0 .. S-1, not codes) of `node` and the rate classes of the last plk_simulate,
 * one per pattern (a multi-device handle gathers the whole alignment).  PLK_ERR_STATE before any
 * plk_simulate, PLK_ERR_ARG for a node outside the last simulated tree. */
int plk_sim_get_states(plk_handle h, int node, uint8_t* states /* n_patterns, state indices */);
int plk_sim_get_classes(plk_handle h, uint8_t* classes /* n_patterns */);
/* Kernel launches (per shard) of the last plk_simulate on this handle. */
int plk_sim_launches(plk_handle h, int64_t* launches);

/* Stochastic mapping (csrc/plk_smap.hpp): histories of substitutions along every branch, drawn
 * from their posterior given the tips (Nielsen 2002; the reference's Mapping/StochasticMapping.cpp
 * samples a site at a time and a branch by rejection).  Ancestral states are drawn down the tree
 * from the stored lower partials, then an endpoint-conditioned path per branch by uniformisation
 * (Hobolth & Stone 2009): the number of jumps, the chain of states, the spacings.
 *
 * Definition.  All draws use plk_simulate's generator and uniform: u = (w >> 11) 2^-53 of word
 * k & 3 of Philox4x64-10(counter = (site, k >> 2, replicate, c3), key = (seed, 0)); plk_simulate has
 * c3 = 0, here c3 = 1 for the ancestral draws and c3 = 2 + v for the path on branch v (a child node
 * index), so no draw is shared with a simulation of the same seed.  Every result is a pure function
 * of (seed, replicate, global site = site0 + pattern, node): launch geometry, sharding and the
 * batching of replicates into calls change nothing.
 *   Weighted draw, the one rule used below: weights w[0..n), each formed as stated and replaced by
 *     0 unless it is > 0; cum the sequential fp64 sum; thr = u * cum[n-1] (one rounded multiply); the
 *     result is the first y with thr < cum[y], else the largest y with w[y] > 0 (0 if there is none).
 *     A weight that is a product p * q is rounded before it enters a sum (no fused multiply-add).
 *   Ancestral states (c3 = 1; k = 0 the class, 1 the root, 2 + v node v), with L the stored lower
 *     partial (a tip: its code's row of the code table) and P the device P(t):
 *       class  w_c = p_c * (sum_x pi_x * L_root[c][x]), the inner sum sequential in x;
 *       root   w_x = pi_x * L_root[c][x];
 *       node v with father state f: w_y = P_v[c][f][y] * L_v[c][y], tips included (an ambiguous or
 *       gap tip gets a sampled state, a resolved tip its own).
 *     Under PLK_FLAG_SCALING a stored vector carries one power of two over all classes and states,
 *     which multiplies thr and cum alike: nothing is unscaled.  A site whose class total is not a
 *     positive finite number is bad: its states and class are 255, its counts and dwelling times 0,
 *     the sums skip it, and each of its replicates is counted in n_bad (no error, as the posteriors).
 *   Tables, built on the device.  Q_m is the generator of plk_smap_set_generator; mu_m =
 *     max_x(-Q_m[x][x]); R_m = I + Q_m / mu_m; Rpow_m[0] = I, Rpow_m[n] = Rpow_m[n-1] R_m for
 *     n <= PLK_SMAP_MAX_JUMPS; per branch and class lambda = mu_m r_c t_v, pois[v][c][0] =
 *     exp(-lambda), pois[n] = pois[n-1] lambda / n.  lambda > 32 is PLK_ERR_UNSUPPORTED (below it the
 *     Poisson tail beyond 128 is under 1e-30).  plk_smap_get_tables reads them back.
 *   Path on branch v from a = the father's state to b = v's state in class c (c3 = 2 + v):
 *     number of jumps (k = 0): the weighted draw over n = 0..128 of w_n = pois[v][c][n] *
 *       Rpow[n][a][b] with thr = u * P_v[c][a][b] in the place of u * cum[128] (the two agree to
 *       rounding, and a scan can stop at the first hit); the fallback is the largest n with w_n > 0;
 *       with no w_n > 0 at all n = 0 where a = b, else n = 1 (the direct jump, counted in n_bad);
 *     states (k = 2i - 1, i = 1..n-1): x_0 = a, x_n = b, x_i the weighted draw of w_y =
 *       R[x_{i-1}][y] * Rpow[n-i][y][b];
 *     spacings (k = 2i + 2, i = 0..n): e_i = -log(1 - u); segment i lasts (t_v * e_i) / sum_i e_i
 *       (the sum sequential in i) in state x_i.  n = 0: no draw, the whole of t_v in state a.
 *     A jump with x_i = x_{i-1} is virtual and no event; a real one x -> y has the type
 *     type_of[x][y] of plk_smap_set_types (0: not counted, k: type k - 1 of the outputs).
 *   Per (replicate, site, branch): n_jumps (virtual ones included), counts[T], dwell[S] (summing to
 *   t_v); per (replicate, site): the class and the state of every node.
 *
 * plk_smap_sample draws replicates replicate0 .. replicate0 + n_replicates - 1 on the tree of the
 * last plk_update_partials, whose root must be `root`; (branch, model, t) as for
 * plk_update_count_matrices (model NULL: model 0) must list every non-root node of that tree once,
 * t the length its P(t) was formed for.  Sums over replicates always stay on the device:
 * count_sum[branch][pattern][T] (uint32), dwell_sum[branch][pattern][S] (double, a replicate's dwell
 * added per site in increasing replicate order), state_tally[node][pattern][S] and
 * class_tally[pattern][C] (uint32), the weighted totals over patterns of the count sums (workgroup
 * sums per block of plk_block_size() patterns added in global block order: plk_branch_counts' rule)
 * and n_bad.  PLK_SMAP_ACCUMULATE adds to the sums of the earlier calls, without it they start at 0.
 * PLK_SMAP_KEEP also keeps this call's per-replicate rows for the plk_smap_get_* getters that take
 * a replicate (its absolute number); PLK_ERR_OOM when they do not fit.
 *
 * PLK_ERR_STATE before a traversal, without P(t) of a listed branch, rates, root frequencies, a
 * generator of a listed model or types; PLK_ERR_UNSUPPORTED on a handle with PLK_FLAG_LNL_ONLY or
 * PLK_FLAG_SUBTREE_PATTERNS; PLK_ERR_ARG for a list that misses a branch of the tree, names one
 * twice or names a node outside it, for n_replicates <= 0, and from a getter for a replicate that
 * is not kept.  PLK_FLAG_DOUBLE_RECURSIVE is not needed (no upper vectors are read).
 *
 * At most three launches per call (tables, sampling, totals: plk_smap_launches).  A multi-device
 * handle fans the call out with each shard's site0 advanced by its first pattern, outputs bitwise
 * those of one device; one process per GPU passes its rank's first site and needs no collective. */
#define PLK_SMAP_MAX_JUMPS 128
enum { PLK_SMAP_ACCUMULATE = 1u, PLK_SMAP_KEEP = 2u };
/* Off-diagonal entries below 0, or a generator without a positive rate, are PLK_ERR_ARG. */
int plk_smap_set_generator(plk_handle h, int model, const double* Q /* S x S */);
int plk_smap_set_types(plk_handle h, int n_types /* 1..16 */, const uint8_t* type_of /* S x S, entries 0..n_types */);
int plk_smap_sample(plk_handle h, int root, int n, const int32_t* branch, const int32_t* model, const double* t,
                    uint64_t seed, uint64_t replicate0, int n_replicates, int64_t site0, unsigned flags);
/* Sums of the sampled replicates; either output may be NULL. */
int plk_smap_get_sums(plk_handle h, int n_branches, const int32_t* branches,
                      uint32_t* count_sum /* [branch][pattern][T] */, double* dwell_sum /* [branch][pattern][S] */);
int plk_smap_get_tallies(plk_handle h, int n_nodes, const int32_t* nodes, uint32_t* state_tally /* [node][pattern][S] */,
                         uint32_t* class_tally /* [pattern][C] */);
int plk_smap_get_totals(plk_handle h, int n_branches, const int32_t* branches, double* totals /* [branch][T] */);
/* Kept rows of one replicate (PLK_SMAP_KEEP). */
int plk_smap_get_states(plk_handle h, uint64_t replicate, int node, uint8_t* states /* n_patterns */);
int plk_smap_get_classes(plk_handle h, uint64_t replicate, uint8_t* classes /* n_patterns */);
int plk_smap_get_jumps(plk_handle h, uint64_t replicate, int branch, uint16_t* n_jumps /* n_patterns */);
int plk_smap_get_counts(plk_handle h, uint64_t replicate, int branch, uint16_t* counts /* [pattern][T] */);
int plk_smap_get_dwell(plk_handle h, uint64_t replicate, int branch, double* dwell /* [pattern][S] */);
/* The tables of the last plk_smap_sample (any output may be NULL): R and Rpow of `model`, the
 * Poisson terms of `branch`. */
int plk_smap_get_tables(plk_handle h, int model, double* R /* S x S */,
                        double* Rpow /* [PLK_SMAP_MAX_JUMPS + 1][S][S] */, int branch,
                        double* pois /* [C][PLK_SMAP_MAX_JUMPS + 1] */);
/* Bad samples behind the current sums: replicates of bad sites plus forced direct jumps. */
int plk_smap_bad(plk_handle h, int64_t* n_bad);
/* Kernel launches (per shard) of the last plk_smap_sample on this handle. */
int plk_smap_launches(plk_handle h, int64_t* launches);

/* Instrumentation: HIP-event timing on the handle's stream of the kernels selected
 * by the mask given to plk_set_timing (0 = off).  Each timed launch adds an event
 * pair to the stream, so time only what is needed. */
enum { PLK_TIME_PARTIALS = 1u, PLK_TIME_PMAT = 2u, PLK_TIME_ROOT = 4u, PLK_TIME_TABLES = 8u };
int plk_set_timing(plk_handle h, int mask);
/* n_launches: partials launches issued while PLK_TIME_PARTIALS was set (the timed ones) */
int plk_get_timing(plk_handle h, int64_t* n_launches, double* partials_ms, double* pmat_ms, double* root_ms);
/* All timers: PLK_TIME_TABLES times the per-traversal table builds that feed a fused
 * traversal (the 20/64-state cherry contribution tables, cherry_table_kernel), which
 * belong to the traversal's cost but are separate launches. */
typedef struct plk_timing {
  int64_t partials_launches;  /* traversal launches timed */
  double partials_ms, pmat_ms, root_ms, tables_ms;
  int64_t table_launches;     /* table-build launches timed */
  /* host side of plk_evaluate (single-device handles, always on): evaluations counted and
   * the summed wall time in microseconds of its segments -- [0] the P(t) launch call,
   * [1] the traversal launch call, [2] the block-sum launch call, [3] the completion wait,
   * [4] the host sum, [5] the caller's time between the end of one plk_evaluate and the
   * start of the next */
  int64_t evaluations;
  double host_us[6];
} plk_timing;
int plk_get_timing_ex(plk_handle h, plk_timing* out);
int plk_reset_timing(plk_handle h);
int plk_synchronize(plk_handle h);

/* Name of the kernel that served the last plk_update_partials call ("jit_tree4",
 * "tree4", "treeS", "treeM" or "levelwise"); "" before the first call. */
const char* plk_kernel_path(plk_handle h);

/* Work of the last traversal, counted on the host from the program that ran (no device
 * call).  A node update is one site pattern of one internal node's partial; the
 * reference computes n_patterns x n_internal of them per traversal
 * (RHomogeneousTreeLikelihood.cpp:839-861).  Here some are table lookups instead:
 *   - cherry tables: the partial of a cherry (two tip sons) -- and, for an unstored
 *     cherry, its contribution to the parent -- is read from a row precomputed per code
 *     pair (table_rows rows per traversal);
 *   - per-subtree pattern compression: a node is computed once per distinct pattern of
 *     its subtree.
 * node_updates counts only the updates computed per pattern.  flops are fp64 operations
 * (an FMA is 2) of the traversal kernel(s) per traversal over the padded patterns:
 * useful = on live states, issued = including MFMA padding rows (20 states run
 * 32-row tiles); table_flops = the table builds (every workgroup of the fused 4-state
 * kernel forms its own tables).  exact = 1 when counted from the fused program that
 * ran, 0 for the levelwise / interpreter paths (then the algorithmic count
 * 2 C S^2 per internal child + (k - 1) C S per combine is reported). */
typedef struct plk_work {
  int64_t patterns;       /* patterns of the handle */
  int64_t node_updates;   /* computed per pattern, summed over patterns and internal nodes */
  int64_t table_nodes;    /* internal nodes served from cherry tables (per pattern) */
  int64_t table_rows;     /* cherry-table rows built per traversal (code pairs x classes x cherries) */
  double useful_flops, issued_flops, table_flops;
  int32_t exact;
  int32_t internal_nodes; /* internal nodes of the traversal */
} plk_work;
int plk_traversal_work(plk_handle h, plk_work* out);

/* With PLK_FLAG_SUBTREE_PATTERNS: the node updates the last traversal actually computed,
 * i.e. the sum over its internal nodes of their distinct subtree patterns (the
 * uncompressed traversal computes n_patterns per node). */
int plk_compressed_work(plk_handle h, int64_t* updates);

#ifdef __cplusplus
}
#endif

#endif /* PLK_H */
