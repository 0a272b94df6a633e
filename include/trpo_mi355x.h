/*
 * trpo_mi355x.h -- drop-in C ABI of the MI355X Fisher-vector-product /
 * conjugate-gradient path (libtrpo_mi355x.so).
 *
 * Part 1 replaces, symbol for symbol, the reference's L3 numerical core
 * declared in src/include/TRPO.h of custom-computing-ic/TRPO-Robot-Control:
 *
 *   TRPOparam      <- src/include/TRPO.h:6-49   (field-for-field identical layout)
 *   NumParamsCalc  <- src/include/TRPO.h:81     (impl. src/TRPO_Util.c:7-17)
 *   FVP            <- src/include/TRPO.h:89     (impl. src/TRPO_FVP.c:11-545)
 *   FVPFast        <- src/include/TRPO.h:93     (impl. src/TRPO_FVP.c:548-949)
 *   CG             <- src/include/TRPO.h:96     (impl. src/TRPO_CG.c:11-113)
 *   FVP_FPGA       <- src/include/TRPO.h:98     (accelerator twin, same signature)
 *   CG_FPGA        <- src/include/TRPO.h:101    (accelerator twin, same signature)
 *   TRPO_Update    <- src/include/TRPO.h:104    (impl. src/TRPO_Update.c:10-1011: policy
 *                     gradient, CG step, FVP(x) step size, backtracking line search)
 *   TRPOBaselineParam <- src/include/TRPO.h:50-77 (field-for-field identical layout)
 *   evaluate       <- src/TRPO_Baseline.c:29    (the value-baseline objective + gradient that
 *                     liblbfgs calls back, lbfgs_evaluate_t of src/include/lbfgs.h:378)
 *
 * Same prototypes, same by-value TRPOparam, same ownership (caller owns Input/b
 * and Result, fp64, length NumParamsCalc()), same return convention (elapsed
 * compute seconds >= 0, or -1 when a file cannot be opened / the request is
 * invalid), same stdout lines from CG.  Model and data still arrive by path
 * and may change between calls: the parsed, device-resident copy is cached
 * keyed on (path, size, mtime, NumSamples, layer shape).
 *
 * Part 2 is the in-memory context API the trainers need: no
 * per-call file I/O, observations uploaded once per update, P-vectors resident
 * in HBM through the whole CG solve, optional RCCL sample sharding.
 *
 * Linkage.  The library exports every Part-1 entry point TWICE: with C linkage
 * (FVPFast, CG, ...) and with C++ linkage (_Z7FVPFast9TRPOparamPdS0_m, ...;
 * csrc/trpo_cxx_abi.cpp forwards those to the C ones).  The reference's own
 * build/Makefile.cpuonly:5,11 compiles its callers with g++ against
 * src/include/TRPO.h:81-104, which has no extern "C", so an UNCHANGED caller
 * imports the mangled names and links as it is.  Included from C++, this
 * header declares the C names by default; define TRPO_MI355X_CXX_LINKAGE to
 * get the reference header's (C++-linkage) declarations of Part 1 instead.
 * evaluate() and Part 2 are C linkage either way (src/include/lbfgs.h:32-34
 * wraps the liblbfgs callback in extern "C").
 */
#ifndef TRPO_MI355X_H
#define TRPO_MI355X_H

#include <stddef.h>

#if defined(__cplusplus) && !defined(TRPO_MI355X_CXX_LINKAGE)
extern "C" {
#endif

#ifndef TRPO_H /* the reference's own TRPO.h already defines the struct */
typedef struct {
    char *ModelFile;         /* model: W[i] [in][out], B[i] per layer, LogStd */
    char *BaselineFile;      /* unused by this path */
    char *ResultFile;        /* unused by this path */
    char *DataFile;          /* per sample: Mean[A] Std[A] Obs[O] Action[A] Adv */
    size_t NumLayers;        /* e.g. 4 for [Input]->[H1]->[H2]->[Output] */
    char *AcFunc;            /* per layer: 'l' linear, 't' tanh, 's' sigmoid, 'o' 0.1x */
    size_t *LayerSize;       /* NumLayers sizes, input first */
    size_t NumSamples;
    double CG_Damping;
    size_t *PaddedLayerSize; /* FPGA only; ignored */
    size_t *NumBlocks;       /* FPGA only; ignored */
} TRPOparam;

size_t NumParamsCalc(size_t *LayerSize, size_t NumLayers);
double FVP(TRPOparam param, double *Result, double *Input);
double FVPFast(TRPOparam param, double *Result, double *Input, size_t NumThreads);
double CG(TRPOparam param, double *Result, double *b, size_t MaxIter, double ResidualTh, size_t NumThreads);
double FVP_FPGA(TRPOparam param, double *Result, double *Input);
double CG_FPGA(TRPOparam param, double *Result, double *b, size_t MaxIter, double ResidualTh, size_t NumThreads);
double TRPO_Update(TRPOparam param, double *Result, size_t NumThreads);

typedef struct {
    size_t NumLayers;
    size_t ObservSpaceDim;   /* the baseline's input is [Obs, step / EpLen]: LayerSizeBase[0] = this + 1 */
    size_t NumEpBatch;
    size_t EpLen;
    size_t NumSamples;       /* NumEpBatch * EpLen */
    size_t NumParams;        /* weights + biases (no LogStd) */
    int PaddedParams;        /* NumParams rounded up to 16 (the L-BFGS vector length) */
    char *AcFunc;
    size_t *LayerSizeBase;
    double **WBase;          /* written from x on every call, like the reference */
    double **BBase;
    double **LayerBase;      /* reference scratch; untouched */
    double **GWBase;
    double **GBBase;
    double **GLayerBase;
    double *Observ;          /* [NumSamples][ObservSpaceDim] */
    double *Target;          /* [NumSamples] */
    double *Predict;         /* [NumSamples], written on every call */
} TRPOBaselineParam;
#endif

#if defined(__cplusplus) && !defined(TRPO_MI355X_CXX_LINKAGE)
} /* extern "C" (Part 1) */
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* liblbfgs callback (double precision lbfgsfloatval_t): instance = TRPOBaselineParam*.
 * Objective 0.01 * mean((Predict - Target)^2) + 0.001 * |x[0:NumParams]|^2 and its gradient
 * (zero beyond NumParams).  Returns -1 for an unsupported activation like the reference. */
double evaluate(void *instance, const double *x, double *g, const int n, const double step);

/* ------------------------------------------------------------------------- */
/* Part 2: in-memory context API                                             */
/* ------------------------------------------------------------------------- */

typedef struct trpo_ctx trpo_ctx;

/* Error codes (negative) returned by the int-valued functions. */
enum {
    TRPO_OK = 0,
    TRPO_E_INVALID = -1,   /* bad shape, activation, NULL pointer */
    TRPO_E_DEVICE = -2,    /* no usable MI355X / HIP error */
    TRPO_E_NOMEM = -3,
    TRPO_E_COMM = -4,      /* collective failure (RCCL, peer exchange timed out, aborted) */
    TRPO_E_IO = -5,
    TRPO_E_TIMEOUT = -6,   /* a bounded wait expired (RCCL init, self-check, trpo_ctx_wait) */
    TRPO_E_VERIFY = -7     /* the collective's self-check summed wrong */
};

/* Create a context on HIP device `device` (-1: current / $TRPO_DEVICE / 0).
 * theta: flat parameters (W, B per layer, LogStd), fp64, NumParamsCalc long.
 * obs: [n][layer_size[0]] fp64 row-major (this rank's samples).
 * stdv: [layer_size[nl-1]] action std (the data file's Std column).
 * Returns NULL on failure (trpo_last_error() has the message).
 * The default solver holds at most 32 768 parameters.  A larger policy (e.g. 376-128-64-17: 57 634) gets from
 * this call a context that serves policy inference only: the setters, trpo_ctx_act, trpo_ctx_act_clear and the
 * rollout record (trpo_ctx_record_*, trpo_ctx_act_record; a commit there is what trpo_ctx_set_obs is there) work;
 * every call that runs the FVP, the CG, the update path (its rollout uploads and surrogates included), the timers
 * or attaches a collective returns TRPO_E_INVALID (-1 for the trpo_ctx_enqueue_* / trpo_ctx_time helpers).  To
 * solve and update such a policy create the context with trpo_ctx_create_wide. */
trpo_ctx *trpo_ctx_create(size_t num_layers, const size_t *layer_size, const char *acfunc,
                          const double *theta, const double *obs, size_t n, const double *stdv,
                          double cg_damping, int device);
/* The same arguments, a context of the wide-policy path: any shape trpo_ctx_create takes, up to
 * 16 777 216 parameters, with the FVP run layer by layer as fp32 MFMA GEMMs over per-sample activation buffers
 * kept in device memory (4 bytes x n x about three times the sum of the layer widths: 224 MB for 376-128-64-17
 * at n = 50 000 -- the reason the path is chosen by the caller) and the CG step distributed over the device.
 * It serves every call of a context but three groups, which return TRPO_E_INVALID with a message naming the
 * path: the collectives (attach_comm, attach_group, the peer windows), the fp64 precision mode
 * (TRPO_PRECISION=fp64: NULL here) and the kernel-only timers (trpo_ctx_enqueue_fvp_kernel_only, trpo_ctx_time
 * what 0 and 3).  The stall guard reports the Ritz residual (trpo_ctx_cg_status) and warns on stderr below its
 * threshold, as on sharded contexts; it does not re-solve.  The file entry points of Part 1 take this path by
 * themselves for a model of more than 32 768 parameters. */
trpo_ctx *trpo_ctx_create_wide(size_t num_layers, const size_t *layer_size, const char *acfunc,
                               const double *theta, const double *obs, size_t n, const double *stdv,
                               double cg_damping, int device);
void trpo_ctx_destroy(trpo_ctx *ctx);

int trpo_ctx_set_theta(trpo_ctx *ctx, const double *theta);
int trpo_ctx_set_obs(trpo_ctx *ctx, const double *obs, size_t n);
int trpo_ctx_set_std(trpo_ctx *ctx, const double *stdv);
int trpo_ctx_set_damping(trpo_ctx *ctx, double cg_damping);
size_t trpo_ctx_num_params(const trpo_ctx *ctx);

/* Attach an RCCL communicator: the context's samples are this rank's shard;
 * every FVP all-reduces the P-sized partial sum once (fp64, sum) and divides
 * by the GLOBAL sample count.  unique_id: 128 bytes from trpo_comm_unique_id()
 * on rank 0, broadcast by the caller. */
int trpo_comm_unique_id(void *unique_id_128);
int trpo_ctx_attach_comm(trpo_ctx *ctx, int rank, int world, const void *unique_id_128);
/* The same with RCCL's initialisation bounded: ncclCommInitRank runs in a helper thread and the call
 * returns TRPO_E_TIMEOUT when it has not completed after timeout_ms (<= 0: $TRPO_COMM_TIMEOUT_MS,
 * default 120 000) -- e.g. a rank that never calls in; the plain attach uses that default too. */
int trpo_ctx_attach_comm_timeout(trpo_ctx *ctx, int rank, int world, const void *unique_id_128, long timeout_ms);

/* In-process sharding without RCCL: `world` contexts of ONE process, each driven by its own
 * thread (any devices, the same one included), attach to a host group and run the sharded code
 * path with a host-staged all-reduce (rank-order sums: identical bits on every rank).  Meant for
 * tests and debugging of the multi-rank logic on one GPU; CG runs eagerly under a group.
 * trpo_ctx_attach_group must be called by all ranks concurrently (it all-reduces N). */
typedef struct trpo_group trpo_group;
trpo_group *trpo_group_create(int world);
void trpo_group_destroy(trpo_group *g);
int trpo_ctx_attach_group(trpo_ctx *ctx, trpo_group *g, int rank);

/* The attached communicator as the collective library reports it: this context's rank, the rank
 * count (RCCL's ncclCommCount; 1 without a communicator) and the fp64 atomic replica sets each FVP
 * all-reduces (0 when the block-slab reduction is in use). */
int trpo_ctx_comm_info(const trpo_ctx *ctx, int *rank, int *world, int *replicas);

/* Peer-window exchange over xGMI (one-shot all-reduce; no reference counterpart -- it replaces the
 * collective under the sharded CG of src/TRPO_CG.c:45-104).  Each rank allocates an exchange window
 * in its own HBM and exports it: trpo_ctx_peer_handle() writes TRPO_PEER_HANDLE_BYTES; the caller
 * all-gathers the handles (its own bootstrap, as for the RCCL unique id) and every rank calls
 * trpo_ctx_attach_peers() concurrently with the world's handles in rank order.  Every collective of
 * the context then goes through the exchange kernel (rank-order sums: identical bits on every rank);
 * the CG graph's per-FVP all-reduce is one kernel.  Contexts of ONE process (tests; any devices)
 * attach with trpo_ctx_attach_peers_local() after each has called trpo_ctx_peer_handle(ctx, NULL).
 * A rank that never arrives makes the exchange give up after 3 s: later calls return an error.
 * Attach once per context: the exchange numbering lives with the windows, so all ranks of a world
 * must be fresh contexts attached together (re-attaching one rank alone desynchronises it). */
#define TRPO_PEER_HANDLE_BYTES 64
#define TRPO_PEER_MAX_RANKS 16
int trpo_ctx_peer_handle(trpo_ctx *ctx, void *handle_64);
int trpo_ctx_attach_peers(trpo_ctx *ctx, int rank, int world, const void *handles);
int trpo_ctx_attach_peers_local(trpo_ctx *ctx, int rank, int world, trpo_ctx *const *all);
/* Self-check of the attached collective (any backend), called by ALL ranks together before it carries
 * results: one eager all-reduce, as long as the per-FVP message, of a rank-dependent test vector whose
 * exact sum is known; completion awaited at most timeout_ms (<= 0: the default above), every element
 * compared bit for bit.  0, TRPO_E_TIMEOUT (call trpo_ctx_comm_abort), TRPO_E_VERIFY or TRPO_E_COMM.
 * No reference counterpart: the reference's CG (src/TRPO_CG.c:45-104) is single-process. */
int trpo_ctx_comm_verify(trpo_ctx *ctx, long timeout_ms);
/* Wait for the context's enqueued work (e.g. trpo_ctx_enqueue_cg) at most timeout_ms: 0,
 * TRPO_E_TIMEOUT, or the collective's error. */
int trpo_ctx_wait(trpo_ctx *ctx, long timeout_ms);
/* Give up on the collective: ncclCommAbort (kernels blocked in it exit) or the peer exchange's error
 * flag, the stream drained (bounded); every later result call fails with TRPO_E_COMM.  Destroy the
 * context afterwards. */
int trpo_ctx_comm_abort(trpo_ctx *ctx);
/* "rccl", "peer-xgmi (...)", "host-group", "aborted" or "none" */
const char *trpo_ctx_comm_backend(const trpo_ctx *ctx);
/* Path of the HIP runtime (libamdhip64) this library's calls resolved to.  The library is built and
 * validated against the system ROCm (/opt/rocm); a process that loads another copy with the same
 * soname first (e.g. the one a PyTorch wheel bundles, imported before this library) makes the
 * library run on that one instead. */
const char *trpo_hip_runtime_path(void);

/* Host-pointer convenience entry points (copy in / compute / copy out).
 * Return elapsed seconds (>= 0) or a negative error code. */
double trpo_ctx_fvp(trpo_ctx *ctx, const double *v, double *out);
double trpo_ctx_cg(trpo_ctx *ctx, const double *b, size_t max_iter, double residual_th, double *x,
                   int verbose);
/* Per-iteration values CG prints: rdotr[i], |x|[i] for i = 0..iters. */
int trpo_ctx_cg_history(const trpo_ctx *ctx, double *rdotr, double *xnorm, size_t cap, size_t *iters);
/* The fp32 stall guard of the last trpo_ctx_cg / trpo_ctx_update (and the file entry points), DESIGN §3:
 * ritz_residual = the smallest relative Ritz residual of the solve's Lanczos matrix (from its CG
 * coefficients); below $TRPO_RITZ_RERUN (default 1e-14) the reference's fp64 CG loses orthogonality and
 * its step is its rounding's, so the solve was repeated in fp64 (*fp64_rerun = 1; one-rank contexts; a
 * "[WARN]" line on stderr).  orth_loss = the largest fraction of a new residual the fp32 path's
 * reorthogonalisation removed.  Any pointer may be NULL.  No reference counterpart. */
int trpo_ctx_cg_status(const trpo_ctx *ctx, double *ritz_residual, double *orth_loss, int *fp64_rerun);

/* Device-resident benchmarking hooks: b stays in HBM, no host round trip.  trpo_ctx_enqueue_cg is the
 * plain device solve: the fp32 stall guard (trpo_ctx_cg_status) never re-solves it.  After a
 * trpo_ctx_cg that the guard re-solved in fp64, slot X (trpo_ctx_download_x) holds the returned fp64 x. */
int trpo_ctx_upload_b(trpo_ctx *ctx, const double *b);
int trpo_ctx_upload_v(trpo_ctx *ctx, const double *v);
int trpo_ctx_enqueue_fvp(trpo_ctx *ctx);                                  /* z = F v */
int trpo_ctx_enqueue_cg(trpo_ctx *ctx, size_t max_iter, double residual_th); /* eager, or a graph under RCCL */
int trpo_ctx_enqueue_fvp_kernel_only(trpo_ctx *ctx);                      /* dominant kernel */
int trpo_ctx_synchronize(trpo_ctx *ctx);
/* Average duration (ms) of `reps` back-to-back launches of `what`
 * (0 = FVP kernel alone, 1 = full FVP, 2 = CG solve of max_iter), measured with
 * HIP events on the context's stream. */
double trpo_ctx_time(trpo_ctx *ctx, int what, int reps, size_t max_iter, double residual_th);
int trpo_ctx_download_x(trpo_ctx *ctx, double *x);
int trpo_ctx_download_z(trpo_ctx *ctx, double *z);

/* One TRPO policy update on the context's samples (src/TRPO_Update.c:254-1007):
 * policy gradient b from the rollout, CG (F + damping I) x = b, shs = x.Fx / 2,
 * lagrange = sqrt(shs / max_kl), fullstep = x / lagrange, backtracking line search
 * over step fractions 0.5^k (k < max_backtracks) accepting the first with
 * ratio > accept_ratio and positive improvement.  theta_out receives the new
 * parameters -- or, as in the reference, the CG step direction x itself when no
 * step fraction is accepted (src/TRPO_Update.c:850-852).  b_out / x_out / info may
 * be NULL.  Requires trpo_ctx_set_rollout() for the current samples.  verbose != 0
 * prints the reference's stdout lines (CG Iter, shs, lagrange multiplier, fval
 * before, a/e/r).  Returns elapsed seconds or a negative error code. */
#define TRPO_MAX_BACKTRACKS 32
typedef struct {
    double shs, lagrange, gnorm, fval_before, expected_improve_rate;
    int evaluated;           /* step fractions evaluated (printed) */
    int accepted;            /* accepted k (step fraction 0.5^k), or -1 */
    double actual[TRPO_MAX_BACKTRACKS], expected[TRPO_MAX_BACKTRACKS], ratio[TRPO_MAX_BACKTRACKS];
    size_t cg_iters;
} trpo_update_info;

/* Rollout of this rank's samples for the update: mean [n][A] (the policy mean the
 * actions were drawn with), action [n][A], adv [n]. */
int trpo_ctx_set_rollout(trpo_ctx *ctx, const double *mean, const double *action, const double *adv);
double trpo_ctx_update(trpo_ctx *ctx, size_t cg_max_iter, double cg_residual_th, double max_kl,
                       int max_backtracks, double accept_ratio, double *theta_out, double *b_out,
                       double *x_out, trpo_update_info *info, int verbose);
/* The line search's surrogate sums (src/TRPO_Update.c:951-981) on their own: surr[j] =
 * sum over ALL ranks' samples of Adv exp(LLD) at theta + 0.5^(k0 + j) fullstep, j < nk (nk <= 64),
 * for the context's current theta and rollout. */
int trpo_ctx_surrogate(trpo_ctx *ctx, const double *fullstep, int k0, int nk, double *surr);

/* Trust-region check (no reference counterpart: the reference's line search never forms the KL).
 * Old policy N(rollout Mean, diag(stdv^2)), stdv the context's std; candidate k: theta_k = theta +
 * 0.5^(k0 + k) fullstep, N(mean(theta_k), diag(exp(2 ls))), ls = theta_k's LogStd; N = all ranks' samples:
 *   kl[k] = sum_i [ ls_i - log stdv_i + stdv_i^2 / (2 exp(2 ls_i)) - 1/2 ]
 *           + (1 / 2N) sum_s sum_i (Mean[s][i] - mean_k[s][i])^2 exp(-2 ls_i)
 *   entropy(theta) = sum_i (LogStd_i + log(2 pi e) / 2);  the old policy's uses log stdv_i.
 * The sample sum comes from the surrogate kernels' own pass (fixed-order sums: the same inputs give the
 * same bits), the sigma-only term from the host in fp64.
 *
 * trpo_ctx_surrogate plus the mean KL(old || candidate) over ALL ranks' samples; surr has the bits
 * trpo_ctx_surrogate returns.  surr or kl may be NULL (not both). */
int trpo_ctx_surrogate_kl(trpo_ctx *ctx, const double *fullstep, int k0, int nk, double *surr, double *kl);

typedef struct {
    double kl[TRPO_MAX_BACKTRACKS];   /* k < info.evaluated */
    double kl_cap;
    double entropy_old, entropy_new;  /* entropy_new at theta_out when a step was accepted, else = old */
    int kl_rejected;                  /* candidates that passed ratio/improvement and exceeded the cap */
} trpo_trust_info;

/* trpo_ctx_update whose line search also requires kl[k] <= kl_cap (kl_cap > 0; INFINITY: no cap, and then
 * theta_out, b_out, x_out and *info are trpo_ctx_update's bit for bit).  trust may be NULL.  verbose: after
 * each a/e/r line one "kl %.14f" line.  TRPO_E_INVALID also for kl_cap <= 0 or NaN. */
double trpo_ctx_update_kl(trpo_ctx *ctx, size_t cg_max_iter, double cg_residual_th, double max_kl,
                          int max_backtracks, double accept_ratio, double kl_cap, double *theta_out,
                          double *b_out, double *x_out, trpo_update_info *info, trpo_trust_info *trust,
                          int verbose);

/* Value-baseline context: data uploaded once per fit, then one device evaluation per L-BFGS
 * callback.  layer_size[0] = observation dim + 1 (the time feature). */
typedef struct trpo_baseline trpo_baseline;
trpo_baseline *trpo_baseline_create(size_t num_layers, const size_t *layer_size, const char *acfunc, int device);
void trpo_baseline_destroy(trpo_baseline *b);
/* observ [num_ep * ep_len][layer_size[0] - 1], target [num_ep * ep_len] */
int trpo_baseline_set_data(trpo_baseline *b, const double *observ, const double *target, size_t num_ep,
                           size_t ep_len);
/* objective at x (n >= NumParams entries, L-BFGS padding allowed); g (n) and predict (may be NULL) */
double trpo_baseline_evaluate(trpo_baseline *b, const double *x, double *g, int n, double *predict);

/* Advantage stage on the device (generalised advantage estimation, Schulman et al. 2016; fp64).  The
 * batch is num_ep episodes of ep_len steps, sample s = ep * ep_len + t; V[t] is the baseline at weights x
 * on [observ[s], t / ep_len] (the predictions trpo_baseline_evaluate returns for x, bit for bit):
 *   ret[t] = reward[t] + gamma ret[t+1]                  ret[ep_len] = 0
 *   d[t]   = reward[t] + gamma V[t+1] - V[t]             V[ep_len]   = 0
 *   A[t]   = d[t] + gamma lam A[t+1]                     A[ep_len]   = 0
 *   adv    = (A - adv_mean) / adv_std                    mean and population std (/ n) of A over the batch
 * ep_rew_mean / ep_rew_std: mean and population std of the episodes' reward sums.  Fixed-order sums: the
 * same inputs give the same bits on every call. */
typedef struct { double ep_rew_mean, ep_rew_std, adv_mean, adv_std; } trpo_adv_info;

/* Upload one batch, make ret the baseline's fit target, compute adv at baseline weights x.
 * adv_out [n], ret_out [n], info may be NULL.  Returns elapsed seconds or a negative code.
 * Afterwards b holds (observ, target = ret) as after trpo_baseline_set_data(b, observ, ret, num_ep,
 * ep_len) -- the fit's trpo_baseline_evaluate calls need no upload -- and keeps adv on the device for
 * trpo_ctx_set_rollout_adv; adv_out receives the bits the device keeps.  TRPO_E_INVALID for a NULL b, x,
 * observ or reward, an empty batch, an evaluation still in flight, and an adv_std that is zero or not
 * finite (one sample, constant advantages): then b holds the batch but no advantage.
 * trpo_baseline_set_data and trpo_baseline_destroy drop the stored advantage. */
double trpo_baseline_advantage(trpo_baseline *b, const double *x, const double *observ,
                               const double *reward, size_t num_ep, size_t ep_len,
                               double gamma, double lam,
                               double *adv_out, double *ret_out, trpo_adv_info *info);

/* The same stage for episodes of their own lengths, some of them cut by a time limit.  The batch is num_ep
 * episodes packed back to back: episode e has ep_len[e] >= 1 steps from sample off[e] = sum of the lengths
 * before it, n = sum ep_len[e].  horizon >= max ep_len[e] scales the time feature: the baseline's input row
 * of step t of any episode is [observ[s], (double)t / (double)horizon].  An episode e with boot[e] != 0 is
 * truncated: boot_observ[e] (layer_size[0] - 1 values) is the observation after its last step, and
 * Vb[e] = the baseline at weights x on [boot_observ[e], ep_len[e] / horizon] stands behind that step;
 * Vb[e] = 0 for every other episode (boot == NULL: for all; boot_observ may then be NULL too):
 *   ret[t] = reward[t] + gamma ret[t+1]                  ret[len] = Vb
 *   d[t]   = reward[t] + gamma V[t+1] - V[t]             V[len]   = Vb
 *   A[t]   = d[t] + gamma lam A[t+1]                     A[len]   = 0
 * adv, adv_mean, adv_std over all n samples; ep_rew_mean / ep_rew_std over the episodes' raw reward sums.
 * Equal lengths with horizon = ep_len and no truncation give trpo_baseline_advantage's bits.
 * Return value, b afterwards and failures as for trpo_baseline_advantage (set_data_ragged in place of
 * set_data); TRPO_E_INVALID also, with b untouched, for a NULL ep_len, an ep_len[e] of 0, horizon below
 * the longest episode, more than INT_MAX samples, and boot without boot_observ. */
int trpo_baseline_set_data_ragged(trpo_baseline *b, const double *observ, const double *target,
                                  size_t num_ep, const size_t *ep_len, size_t horizon);
double trpo_baseline_advantage_ragged(trpo_baseline *b, const double *x, const double *observ,
                                      const double *reward, size_t num_ep, const size_t *ep_len,
                                      size_t horizon, const double *boot_observ /* [num_ep][O] or NULL */,
                                      const unsigned char *boot /* [num_ep] or NULL */,
                                      double gamma, double lam,
                                      double *adv_out, double *ret_out, trpo_adv_info *info);

/* trpo_ctx_set_rollout with adv taken on the device from b's last advantage stage:
 * this context's sample i uses b's sample first + i (a rank of a sharded batch computes the global
 * batch's advantages on its replica of the baseline and takes its own contiguous slice).  mean and
 * action go up through pinned memory.  TRPO_E_INVALID, with the context's rollout left as it was, unless
 * b holds a valid advantage, is on the context's HIP device and first + n <= b's samples. */
int trpo_ctx_set_rollout_adv(trpo_ctx *ctx, const double *mean, const double *action,
                             const trpo_baseline *b, size_t first);

/* Policy inference at the context's current theta (fp64).  obs [m][L0] host rows.  Sample i of the call is
 * ROW r_i = row0 + i * row_stride of the batch (row_stride >= 1; a vectorised environment at time t of
 * equal-length episodes passes row0 = t, row_stride = ep_len, so rows come out episode-major as the advantage
 * stage wants them).
 *   mean_i   = the network's output on obs_i: every neuron bias first, inputs ascending, then the activation
 *   z[i][a]  : Philox4x32-10, key = (seed lo32, seed hi32),
 *              counter = (r_i lo32, r_i hi32, step lo32, (step >> 32) << 16 | j), pair j = a / 2,
 *              outputs (o0, o1, o2, o3):
 *              u1 = (((uint64)o0 << 21 | o1 >> 11) + 1) * 2^-53,  u2 = ((uint64)o2 << 21 | o3 >> 11) * 2^-53,
 *              z[2j] = sqrt(-2 ln u1) cos(2 pi u2),  z[2j+1] = sqrt(-2 ln u1) sin(2 pi u2)
 *   action   = mean + exp(LogStd) z          LogStd = theta's last A entries
 *   logp     = -1/2 sum_a z_a^2 - sum_a LogStd_a - (A/2) ln(2 pi)        (a ascending)
 * A result depends on (theta, obs_i, seed, step, r_i) alone: the same row gives the same bits in any batch,
 * position or call.  action_out == NULL: means only, no generator (evaluation mode); logp_out then must be
 * NULL too (with action_out, logp_out may still be NULL).
 * keep != 0: the device also keeps (mean, action) of row r_i for trpo_ctx_set_rollout_acted; rows must be
 * < the context's n.  Returns elapsed seconds or a negative code.  TRPO_E_INVALID before any device work for
 * NULL ctx / obs / mean_out, m == 0, row_stride == 0, step >= 2^48, a last row >= 2^48, keep without
 * action_out, a kept row >= n.  TRPO_E_TIMEOUT when the launch has not finished after $TRPO_ACT_TIMEOUT_MS
 * (default 10 000).  No collective: on a sharded context the call is local to the rank.
 * $TRPO_ACT_FORM = lane | neuron, read at trpo_ctx_create, forces one of the two kernel forms (same bits). */
double trpo_ctx_act(trpo_ctx *ctx, const double *obs, size_t m, unsigned long long seed,
                    unsigned long long step, size_t row0, size_t row_stride, int keep,
                    double *mean_out, double *action_out, double *logp_out);
/* forget the kept rows (also done by trpo_ctx_set_obs) */
int trpo_ctx_act_clear(trpo_ctx *ctx);
/* trpo_ctx_set_rollout with Mean and Action taken on the device from the kept rows; exactly one of adv (host
 * [n]) and b (then adv = b's stored advantages [first, first + n), as trpo_ctx_set_rollout_adv).
 * TRPO_E_INVALID, rollout left as it was, unless every row 0..n-1 has been kept since the last clear. */
int trpo_ctx_set_rollout_acted(trpo_ctx *ctx, const double *adv, const trpo_baseline *b, size_t first);

/* The rollout record: a batch that is acted on the device stays there.  Between trpo_ctx_record_begin and a
 * commit the context holds, beside its current batch, device rows [rows][L0] of observations and [rows][2A] of
 * (mean, action); trpo_ctx_act_record fills them as the environment is stepped, and a commit makes them the
 * context's batch.  No observation goes up a second time and no row's forward pass is run a second time:
 *   trpo_ctx_record_begin(ctx, n);  per step: trpo_ctx_act_record(ctx, obs_t, ...);  trpo_ctx_record_commit(ctx)
 * leaves ctx in the state -- bit for bit: the observations, every layout derived from them, the kept rows --
 * that trpo_ctx_set_obs(ctx, Observ, n) followed by trpo_ctx_act(ctx, Observ, n, seed, step, 0, 1, keep = 1, ...)
 * leaves it in, so trpo_ctx_set_rollout_acted works straight after the commit.  As trpo_ctx_set_obs does, a
 * commit drops the rollout, invalidates the forward cache, and on a sharded context is called by every rank.
 * Works on every context trpo_ctx_set_obs works on (default, wide, fp64, inference-only).
 *
 * trpo_ctx_record_begin: start recording `rows` (1 .. 2^30) sample rows.  The context's current observations,
 * rollout and kept rows stay valid and usable until a commit succeeds.  A recording in progress is discarded
 * by a new trpo_ctx_record_begin, trpo_ctx_set_obs, trpo_ctx_act_clear and trpo_ctx_destroy; trpo_ctx_set_theta
 * does not discard it (the old policy of an update is the caller's business, as with kept rows). */
int trpo_ctx_record_begin(trpo_ctx *ctx, size_t rows);
/* trpo_ctx_act with action_out required, which also stores obs_i and (mean_i, action_i) of row
 * r_i = row0 + i * row_stride into the record.  The outputs are trpo_ctx_act's bits; the Philox row is the record
 * row r_i (for slots of a ragged batch the slot row: (seed, step, row) stays unique).  A row recorded twice holds
 * the last call's values.  TRPO_E_INVALID, with trpo_last_error() naming the call, for everything trpo_ctx_act
 * refuses, action_out == NULL, no recording in progress, a row >= rows. */
double trpo_ctx_act_record(trpo_ctx *ctx, const double *obs, size_t m, unsigned long long seed,
                           unsigned long long step, size_t row0, size_t row_stride,
                           double *mean_out, double *action_out, double *logp_out);
/* make the record the context's batch: n = rows.  The record's buffers become the context's; nothing is copied.
 * TRPO_E_INVALID with no recording in progress or a row that was never recorded (the message names the first
 * one).  A refused commit changes nothing: batch, rollout and kept rows are as they were and the recording
 * stays open, so the caller can fill the gap and commit again. */
int trpo_ctx_record_commit(trpo_ctx *ctx);
/* episodes of their own lengths: episode e was recorded at rows e * slot_rows + t, t < ep_len[e]; the commit
 * packs them back to back, sample off[e] + t <- record row e * slot_rows + t, n = sum ep_len[e]: the order the
 * ragged advantage stage wants.  Rows of a slot past its episode's length may have been recorded; they do not
 * appear.  Refused as trpo_ctx_record_commit, and for ep_len[e] == 0, ep_len[e] > slot_rows,
 * num_ep * slot_rows > rows, a sum above INT_MAX. */
int trpo_ctx_record_commit_ragged(trpo_ctx *ctx, size_t num_ep, const size_t *ep_len, size_t slot_rows);
/* rows of the recording in progress (0: none) and how many distinct rows have been recorded; either may be NULL */
int trpo_ctx_record_info(const trpo_ctx *ctx, size_t *rows, size_t *recorded);

/* trpo_baseline_advantage / _ragged with the observations read on the device from the context's current batch
 * (however it got there: a commit or trpo_ctx_set_obs); only rewards, weights and the truncated episodes' last
 * observations go up.  With the same observation values: the host-observation call's bits in adv, ret and info,
 * and b afterwards in the same state.  TRPO_E_INVALID for everything those calls refuse, a NULL ctx, a context
 * on another HIP device than b, layer_size[0] - 1 of b != the context's L0, and a context whose n is not the
 * batch's num_ep * ep_len (sum ep_len[e]) -- a rank of a sharded context holds a slice and is refused. */
double trpo_baseline_advantage_ctx(trpo_baseline *b, const double *x, const trpo_ctx *ctx,
                                   const double *reward, size_t num_ep, size_t ep_len, double gamma, double lam,
                                   double *adv_out, double *ret_out, trpo_adv_info *info);
double trpo_baseline_advantage_ragged_ctx(trpo_baseline *b, const double *x, const trpo_ctx *ctx,
                                          const double *reward, size_t num_ep, const size_t *ep_len,
                                          size_t horizon, const double *boot_observ, const unsigned char *boot,
                                          double gamma, double lam,
                                          double *adv_out, double *ret_out, trpo_adv_info *info);

/* The device-resident loop: the same calls for a caller whose environment lives on the GPU.  Its arrays are
 * device memory, its work is ordered by a stream of its own, and no observation, action or reward crosses the
 * host link.  The header stays free of HIP types: hip_stream is a hipStream_t (NULL: the context's own stream --
 * the caller then calls trpo_ctx_synchronize before it reads), dtype names the element type of the caller's
 * floating-point device arrays.
 *
 * Stream contract of the two act calls: they are asynchronous and return 0, or a negative code, as soon as the
 * work is enqueued.  The launch is ordered after everything already enqueued on hip_stream and after the
 * context's own pending work; whatever is enqueued on hip_stream afterwards sees the outputs; every later call
 * on the context (a commit, trpo_ctx_set_rollout_acted, an update) is ordered after it.  The host never waits.
 * The arrays must stay allocated until the work has run.  One call at a time per context, as everywhere in this
 * interface.  Capturing these calls into a hipGraph is not supported.
 *
 * TRPO_DT_F32: every observation is widened exactly to fp64 on load and all arithmetic is the fp64 chain;
 * mean, action and logp are rounded once, to nearest even, on store; the record and the kept rows hold the
 * fp64 values (the widened observation, the unrounded mean and action), so an update after the commit is, bit
 * for bit, the update of the host path fed the widened observations.  TRPO_DT_F64: the host calls' bits.
 *
 * Refusals (TRPO_E_INVALID before any device work, trpo_last_error() names the call and the argument): whatever
 * the host-pointer twin refuses; a dtype other than the two; an array that is not device memory of the
 * context's (baseline's) HIP device -- host, pinned and managed memory are refused; an array whose extent, by
 * the call's own arguments, does not lie inside its allocation. */
#define TRPO_DT_F64 0
#define TRPO_DT_F32 1
/* trpo_ctx_act / trpo_ctx_act_record on device arrays: obs_dev [m][L0], mean_dev [m][A], action_dev [m][A] or
 * NULL (means only; trpo_ctx_act_dev alone), logp_dev [m] or NULL, all of element type dtype. */
int trpo_ctx_act_dev(trpo_ctx *ctx, const void *obs_dev, size_t m, unsigned long long seed, unsigned long long step,
                     size_t row0, size_t row_stride, int keep, int dtype,
                     void *mean_dev, void *action_dev, void *logp_dev, void *hip_stream);
int trpo_ctx_act_record_dev(trpo_ctx *ctx, const void *obs_dev, size_t m, unsigned long long seed,
                            unsigned long long step, size_t row0, size_t row_stride, int dtype,
                            void *mean_dev, void *action_dev, void *logp_dev, void *hip_stream);
/* Episode ends from the environment's flags, uint8 device arrays [num_env * slot_rows] in record-row layout
 * (row = e * slot_rows + t; truncated_dev may be NULL).  For slot e, t* = the first t with terminated[e][t] != 0
 * or truncated[e][t] != 0: ep_len_out[e] = t* + 1 and truncated_out[e] = (terminated[e][t*] == 0); with no flag
 * set ep_len_out[e] = slot_rows and truncated_out[e] = 1 (the slot ran out).  These are the ep_len and boot
 * arrays of trpo_ctx_record_commit_ragged and the ragged advantage calls.  Needs no recording in progress;
 * ordered after hip_stream; synchronous (one host wait).  num_env * slot_rows <= 2^30. */
int trpo_ctx_record_episodes_dev(trpo_ctx *ctx, const unsigned char *terminated_dev, const unsigned char *truncated_dev,
                                 size_t num_env, size_t slot_rows, void *hip_stream,
                                 size_t *ep_len_out, unsigned char *truncated_out);
/* trpo_baseline_advantage_ctx / _ragged_ctx with the rewards in device memory, complete in hip_stream's order
 * (NULL: already complete); synchronous like those calls.  Fixed form: reward_dev [n] in sample order.  Ragged
 * form: reward_slots_dev [num_ep * slot_rows] in record-row layout, packed on the device as the ragged commit
 * packs the rows (sample off[e] + t <- slot row e * slot_rows + t); last_obs_dev [num_ep][layer_size[0] - 1]
 * stands for boot_observ (may be NULL when boot is); ep_len and boot stay host arrays.  With the same values:
 * the host-reward call's bits in adv, ret and info, and b in the same state.  Also refused: ep_len[e] >
 * slot_rows. */
double trpo_baseline_advantage_ctx_dev(trpo_baseline *b, const double *x, const trpo_ctx *ctx, const void *reward_dev,
                                       int dtype, size_t num_ep, size_t ep_len, double gamma, double lam,
                                       void *hip_stream, double *adv_out, double *ret_out, trpo_adv_info *info);
double trpo_baseline_advantage_ragged_ctx_dev(trpo_baseline *b, const double *x, const trpo_ctx *ctx,
                                              const void *reward_slots_dev, const void *last_obs_dev, int dtype,
                                              size_t num_ep, const size_t *ep_len, size_t slot_rows, size_t horizon,
                                              const unsigned char *boot, double gamma, double lam, void *hip_stream,
                                              double *adv_out, double *ret_out, trpo_adv_info *info);

/* The observation filter: while it is enabled the policy sees (obs - running mean) / running std, clipped, and the
 * rollout record holds those normalised rows, so an update after a commit runs on what the policy saw.  No
 * reference counterpart (Welford 1962; batches merged as Chan, Golub and LeVeque 1983).  This is the contract.
 *
 * State, per context, fp64, on the device, for the L0 = layer_size[0] columns:
 *   live     (count, mean[L0], M2[L0])      M2 = sum of squared deviations from mean
 *   derived  (shift[L0], scale[L0])         count < 2: shift = 0, scale = 1 (the identity);
 *                                           else shift = mean, scale = 1 / (sqrt(M2 / (count - 1)) + eps)
 *   pending  (count, mean[L0], M2[L0])      what the record calls have seen since the last fold
 * One element x of column k is normalised by exactly these fp64 operations, in this order:
 *   y = (x - shift[k]) * scale[k]           a subtraction, then a multiplication: never one fma
 *   y = fmin(fmax(y, -clip), clip)          clip = +inf clips nothing
 * An fp32 input is widened exactly first.  What a NaN input gives is unspecified.
 *
 * Which rows count.  trpo_ctx_act_record / _act_record_dev normalise their rows with the derived pair, store the
 * NORMALISED rows into the record, and add the call's RAW rows to pending.  trpo_ctx_act / trpo_ctx_act_dev
 * normalise and never touch the statistics (evaluation, kept rows).  Every row passed to a record call counts,
 * whether or not a later commit keeps it (a ragged commit drops the rows past an episode's end: they have counted),
 * and a row recorded twice counts twice.
 *
 * One call's m rows enter pending as a batch, column by column: the rows are cut into chunks of
 * TRPO_OBSNORM_CHUNK consecutive rows; sum_c = the chunk's values in row order, starting from 0, as a compensated
 * sum (Kahan 1965: y = x - e, t = s + y, e = (t - s) - y, s = t); mean_b = (the sum_c in chunk order, starting
 * from 0, compensated in the same way) / m; M2_b = the same two-level sum of (x - mean_b)^2, the square entering
 * its step unrounded (y = fma(d, d, -e)).  Two passes: squares are taken of deviations, never of values.  Then, with (n_p, mean_p, M2_p)
 * the pending moments before the call,
 *   d = mean_b - mean_p,  n = n_p + m,  mean = mean_p + d (m / n),  M2 = M2_p + M2_b + d d (n_p m / n)
 * each operation rounded on its own.  The result depends on the values and on m alone: not on the kernel form,
 * the launch geometry, host rows against device fp64 rows, or the kind of context; fp32 rows give the moments
 * of their widened values.  The same calls in the same order give the same bits.
 *
 * Frozen within a batch.  The derived pair changes in trpo_ctx_obsnorm_fold and trpo_ctx_obsnorm_set alone.  fold
 * merges pending into live by the formula above (live in the place of pending, pending in the place of the batch),
 * derives the pair anew and empties pending.  trpo_ctx_record_begin empties pending, so a recording that is
 * discarded leaves no trace.  The caller's order is: record ... commit, the advantage stage (truncated episodes'
 * boot observations normalised by trpo_ctx_obsnorm_apply[_dev] first), then fold.
 * Everything is enqueued on the context's stream and the host does not wait; get and the host-pointer apply do.
 * A context without the filter launches exactly the kernels it launched before the filter existed.
 * On a sharded context the statistics are local to the rank and no call here is a collective: a trainer merges
 * the ranks' states itself, through get and set.
 *
 * Refusals: TRPO_E_INVALID before any device work, trpo_last_error() names the call -- a NULL context; any call
 * but enable on a context without the filter; and what each call lists. */
#define TRPO_OBSNORM_CHUNK 64
/* clip > 0 (+inf allowed) and eps >= 0, else refused (NaN too).  Live and pending empty, the pair the identity:
 * until the first fold every act call gives the bits it gives without the filter.  A second call starts over. */
int trpo_ctx_obsnorm_enable(trpo_ctx *ctx, double clip, double eps);
/* back to a context without the filter; the state is gone */
int trpo_ctx_obsnorm_disable(trpo_ctx *ctx);
int trpo_ctx_obsnorm_fold(trpo_ctx *ctx);
/* which: 0 live, 1 pending.  count [1], mean [L0], m2 [L0]; shift [L0], scale [L0] with which = 0 only (refused
 * otherwise); any of them may be NULL.  Waits for the context's stream. */
int trpo_ctx_obsnorm_get(const trpo_ctx *ctx, int which, double *count, double *mean, double *m2,
                         double *shift, double *scale);
/* checkpoint restore: live = (count, mean, m2), the pair derived from it, pending emptied.  Refused: a count that
 * is negative, not whole or above 2^53; a mean that is not finite; an m2 that is negative or not finite. */
int trpo_ctx_obsnorm_set(trpo_ctx *ctx, double count, const double *mean, const double *m2);
/* out [m][L0] = in [m][L0] normalised with the derived pair, host rows (out may be in); synchronous */
int trpo_ctx_obsnorm_apply(const trpo_ctx *ctx, const double *in, size_t m, double *out);
/* the same on device arrays of dtype, rounded once on the store, in place when out_dev == in_dev; asynchronous,
 * under the stream contract of the act calls above.  Also refused: a dtype other than the two, an array that is
 * not device memory of the context's device or does not hold m * L0 elements. */
int trpo_ctx_obsnorm_apply_dev(trpo_ctx *ctx, const void *in_dev, size_t m, int dtype,
                               void *out_dev, void *hip_stream);

/* Trust-region fit of the baseline, resident on the device (Schulman et al. 2016, GAE, section 5; no
 * reference counterpart -- the L-BFGS fit through evaluate() stays the caller's).  fp64; phi = the NumParams
 * weights and biases, V_phi(s) the prediction, y the object's fit target, N its samples (bootstrap rows of a
 * ragged batch never count), j_s = grad_phi V_phi(s):
 *   L(phi) = (1/N) sum (V_phi(s) - y_s)^2                loss_before = sigma^2 = L(x)
 *   g      = (1/N) sum (V_x(s) - y_s) j_s                gnorm = |g|
 *   H v    = (1/N) sum j_s (j_s . v) + damping v         Gauss-Newton product at x
 *   CG     : s = 0, r = p = -g; at most cg_max_iter times  z = H p, a = r.r / p.z, s += a p, r -= a z,
 *            stop when r.r < cg_residual_th, p = r + (r.r new / r.r old) p
 *   q = s . H s (shs = q / 2),  alpha_tr = sqrt(2 eps sigma^2 / q),  alpha0 = min(1, alpha_tr)
 * alpha_tr puts the linearised (1/N) sum (dV)^2 / (2 sigma^2) on eps; the step is capped at the Gauss-Newton
 * step itself (alpha0 <= 1), beyond which the quadratic model only gets worse.  Candidates x + alpha0 0.5^k s,
 * k < max_backtracks: loss[k] = L there, shift[k] = (1/N) sum (V_k - V_x)^2 / (2 sigma^2); accepted = the first
 * k with loss[k] < loss_before and shift[k] <= shift_cap (INFINITY: no cap), else -1 and x_out = x bit for bit.
 * All candidates are evaluated in one pass: evaluated = max_backtracks.  rdotr[i] = r.r before iteration i,
 * i <= cg_iters, zero beyond.  Every sum has a fixed order: the same inputs give the same bits on every call. */
#define TRPO_VFIT_MAX_CG 64
typedef struct {
    double loss_before;            /* = sigma^2 */
    double gnorm, shs /* q/2 */, alpha_tr, alpha0;
    double loss[TRPO_MAX_BACKTRACKS], shift[TRPO_MAX_BACKTRACKS];
    double rdotr[TRPO_VFIT_MAX_CG + 1];     /* r.r before iteration i, i <= cg_iters */
    size_t cg_iters;
    int evaluated, accepted;
} trpo_vfit_info;

/* out = H v at weights x on b's data (n >= NumParams, padding of out zeroed); seconds or a negative code */
double trpo_baseline_gnvp(trpo_baseline *b, const double *x, const double *v, int n, double damping, double *out);

/* the fit above; x_out (n, padding zeroed), step_out (s, may be NULL), info (may be NULL).  TRPO_E_INVALID
 * before any device work for a NULL b, x or x_out (checked first), n < NumParams, no data in b, an evaluation
 * still in flight, eps <= 0, damping < 0, shift_cap <= 0 (or NaN), cg_max_iter outside 1..TRPO_VFIT_MAX_CG,
 * max_backtracks outside 1..TRPO_MAX_BACKTRACKS; and after the first pass, with x_out = x, when sigma^2 is
 * zero or not finite.  Neither call changes b's data, target or stored advantage. */
double trpo_baseline_fit_tr(trpo_baseline *b, const double *x, int n, double eps, size_t cg_max_iter,
                            double cg_residual_th, double damping, int max_backtracks, double shift_cap,
                            double *x_out, double *step_out, trpo_vfit_info *info);

/* Introspection: which kernel family serves this context ("mfma-mlp3 T0xT1xT2xT3"
 * or "generic"), and the FVP launch geometry. */
const char *trpo_ctx_kernel_name(const trpo_ctx *ctx);
/* The same for a baseline, valid once it holds a batch (trpo_baseline_set_data[_ragged], an advantage stage;
 * "" before): "eval=F predict=F gnvp=F cand=F" names the kernel form that trpo_baseline_evaluate, the advantage
 * stage's prediction pass, the Gauss-Newton product (trpo_baseline_gnvp and the fit's CG) and the fit's
 * candidate pass take for the object's shape.  F is "lane" (the lane-parallel kernels of [L0, L1, L2, 1] nets
 * with widths <= 16; the prediction pass has none) or a form of the one-sample-per-lane kernels: "lds+theta"
 * (activations and weights in LDS), "lds" (activations in LDS, weights read from global memory), "scratch"
 * (activations in a global scratch buffer; the prediction pass then runs at the evaluate's row stride).  The
 * candidate pass never stages weights: "lds" or "scratch".  The string lives as long as b and is rewritten
 * by the calls that set a batch. */
const char *trpo_baseline_kernel_name(const trpo_baseline *b);
int trpo_ctx_launch_geometry(const trpo_ctx *ctx, int *blocks, int *threads, int *lds_bytes);
/* Diagnostics: *count = launches, enqueued by this context so far, of a tile kernel that computed the
 * network's forward pass from the observations (the FVP kernel when it recomputes, the policy-gradient
 * kernel) -- launches on the forward-activation cache are not counted.  One update() on the
 * one-wave path adds 1; a solve on a cache that is still valid adds 0.  Generic-path contexts
 * (no tile kernel) stay at 0.  Returns 0, or TRPO_E_INVALID. */
int trpo_ctx_forward_passes(const trpo_ctx *ctx, unsigned long long *count);

const char *trpo_last_error(void);
/* Drop every cached file-based context (FVPFast/FVP/CG cache). */
void trpo_cache_clear(void);

/* ------------------------------------------------------------------------- */
/* Part 3: the reference's text formats, as the Part-1 entry points read them */
/* ------------------------------------------------------------------------- */
/* Up to `want` doubles from whitespace-separated text with fscanf("%lf") semantics (stops at the end
 * or at the first token that is not a number); returns how many were parsed. */
size_t trpo_text_parse_doubles(const char *txt, double *out, size_t want);
/* Model file (src/TRPO_FVP.c:670-699): theta[P] (W, B per layer, then the LogStd line, which the
 * reference reads as Std); entries the file lacks are 0.  0, or -1 if it cannot be opened. */
int trpo_text_load_model(const char *path, size_t P, double *theta);
/* Data file (src/TRPO_FVP.c:731-762, src/TRPO_Update.c:228-249): the first n rows of
 * Mean[A] Std[A] Obs[O] Action[A] Adv; stdv = the LAST row's Std; mean / action / adv may be NULL. */
int trpo_text_load_data(const char *path, size_t O, size_t A, size_t n, double *obs, double *stdv, double *mean,
                        double *action, double *adv);

#ifdef __cplusplus
}
#endif
#endif /* TRPO_MI355X_H */
