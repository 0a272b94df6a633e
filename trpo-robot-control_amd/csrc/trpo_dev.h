/*
 * trpo_dev.h -- the thin C ABI between the C host layer (trpo_host.c) and the
 * hand-written gfx950 kernels (trpo_kernels.hip and its sections dev_*.h).  Plain pointers and sizes
 * only.  One trpo_dev owns everything that lives in HBM for one network and
 * one sample shard on one GPU: packed weights, observations, the CG vectors,
 * the per-block partial-sum slabs, the captured CG graph and (optionally) an
 * RCCL communicator.
 */
#ifndef TRPO_DEV_H
#define TRPO_DEV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trpo_dev trpo_dev;

enum { TRPO_VEC_V = 0, TRPO_VEC_Z = 1, TRPO_VEC_X = 2, TRPO_VEC_B = 3, TRPO_VEC_P = 4 };

/* device < 0: $TRPO_DEVICE or 0.  Returns NULL and fills err on failure. */
trpo_dev *trpo_dev_create(int device, size_t nl, const size_t *ls, const char *ac, char *err, size_t errlen);
/* the same with the precision forced (f64 != 0: the fp64 mode) instead of read from $TRPO_PRECISION */
trpo_dev *trpo_dev_create_prec(int device, size_t nl, const size_t *ls, const char *ac, int f64, char *err,
                               size_t errlen);
/* the wide-policy path (dev_wide.h) for any shape the generic kernel takes: layer-wise MFMA GEMM FVP, the
 * distributed CG step, no bound from one workgroup; fp32 only (NULL with the reason under TRPO_PRECISION=fp64).
 * The caller has checked NumParams <= TRPO_WIDE_MAX_PARAMS: parameter offsets are ints, also in the padded
 * copies (at most 7 (P + 2^21 + 256) elements), and a slab is P floats per 512 samples. */
#define TRPO_WIDE_MAX_PARAMS ((size_t)1 << 24)
trpo_dev *trpo_dev_create_wide(int device, size_t nl, const size_t *ls, const char *ac, char *err, size_t errlen);
int trpo_dev_device(const trpo_dev *d);
int trpo_dev_is_f64(const trpo_dev *d);
/* copies of the problem a context holds (fp64): obs [n][L0], std [A], rollout (trpo_update.hip) */
int trpo_dev_get_obs(trpo_dev *d, double *host);
int trpo_dev_get_std(trpo_dev *d, double *host);
int trpo_dev_get_rollout(trpo_dev *d, double *mean, double *action, double *adv);
void trpo_dev_destroy(trpo_dev *d);

int trpo_dev_set_theta(trpo_dev *d, const double *theta);
int trpo_dev_set_std(trpo_dev *d, const double *stdv);
int trpo_dev_set_obs(trpo_dev *d, const double *obs, size_t n);
/* set_obs for a batch already on the device: buf [n][L0] (the allocator the context uses, n >= 1, written on the
 * context's stream) becomes the context's; no copy.  -1 (buf still the caller's) for bad arguments. */
int trpo_dev_set_obs_device(trpo_dev *d, double *buf, size_t n);
int trpo_dev_set_damping(trpo_dev *d, double damping);

int trpo_dev_comm_unique_id(void *id128);
/* RCCL init bounded by timeout_ms (<= 0: $TRPO_COMM_TIMEOUT_MS or 120 s); -6 on time-out */
int trpo_dev_set_comm(trpo_dev *d, int rank, int world, const void *id128, long timeout_ms);
/* bounded self-check / wait / abort of the attached collective (dev_comm.h) */
int trpo_dev_comm_verify(trpo_dev *d, long timeout_ms, long *bad);
int trpo_dev_wait(trpo_dev *d, long timeout_ms);
// the closing wait of a synchronous call: hipStreamSynchronize on one rank, bounded (and the
// collective's error reported) with a collective attached
int trpo_dev_wait_done(trpo_dev *d);
#define DSYNC(d)                                     \
    do {                                             \
        const int dsync_rc_ = trpo_dev_wait_done(d); \
        if (dsync_rc_) return dsync_rc_;             \
    } while (0)
int trpo_dev_comm_abort(trpo_dev *d);
/* in-process host-staged group of `world` contexts (one thread each): the sharded code path
 * without RCCL, for tests (dev_comm.h) */
typedef struct trpo_hgroup trpo_hgroup;
trpo_hgroup *trpo_hgroup_create(int world);
void trpo_hgroup_destroy(trpo_hgroup *g);
int trpo_dev_set_group(trpo_dev *d, trpo_hgroup *g, int rank);
int trpo_dev_comm_info(const trpo_dev *d, int *rank, int *world, int *replicas);
/* peer-window exchange over xGMI (trpo_peer.hip): open the own window (its 64-byte IPC handle into
 * handle64 when non-NULL), then attach with the world's handles (rank order) or, in one process,
 * the contexts' window pointers; replaces RCCL / the host group for this context */
int trpo_dev_peer_open(trpo_dev *d, void *handle64);
void *trpo_dev_peer_window(trpo_dev *d);
int trpo_dev_set_peers(trpo_dev *d, int rank, int world, const void *handles, void *const *local);
int trpo_dev_comm_error(const trpo_dev *d);
const char *trpo_dev_comm_backend(const trpo_dev *d);

int trpo_dev_upload(trpo_dev *d, int slot, const double *host);
int trpo_dev_download(trpo_dev *d, int slot, double *host);
/* x and the last CG solve's statistics, one synchronisation: stats[0] = the largest fraction of a new
 * residual the reorthogonalisation removed (0 without it), stats[1 + k] = alpha_k, k < 64; rdotr[0..iters]
 * the residual history (cap entries at most) */
#define TRPO_CG_STATS 65
int trpo_dev_download_x_cg(trpo_dev *d, double *host, double *stats, double *rdotr, size_t cap, size_t *iters);

int trpo_dev_fvp(trpo_dev *d);                 /* enqueue z = F v  (slots V -> Z) */
int trpo_dev_fvp_src(trpo_dev *d, const double *src);   /* enqueue z = F src (any device vector) -> Z */
int trpo_dev_fvp_host(trpo_dev *d, double *host); /* z = F v (V -> Z) and z -> host, one wait */
int trpo_dev_fvp_kernel(trpo_dev *d);         /* enqueue the dominant kernel alone */
int trpo_dev_cg(trpo_dev *d, size_t maxiter, double resth); /* enqueue CG on slot B -> X */
int trpo_dev_cg_history(trpo_dev *d, double *rdotr, double *xnorm, size_t cap, size_t *iters);
int trpo_dev_sync(trpo_dev *d);
/* what: 0 FVP kernel, 1 full FVP, 2 CG(maxiter) -- average ms over reps */
double trpo_dev_time(trpo_dev *d, int what, int reps, size_t maxiter, double resth);

/* TRPO_Update path (src/TRPO_Update.c), fp64.  Rollout = per local sample Mean[A],
 * Action[A], Adv.  policy_gradient leaves b in slot B (and copies it / the global
 * sum of Adv to the host when non-NULL); surrogate returns the global sums
 * sum_n Adv exp(LLD) for candidates theta + 2^-k fullstep, k = k0 .. k0+nk-1. */
int trpo_dev_set_rollout(trpo_dev *d, const double *mean, const double *action, const double *adv, size_t n);
int trpo_dev_policy_gradient(trpo_dev *d, double *b_host, double *adv_sum);
int trpo_dev_surrogate(trpo_dev *d, const double *fullstep, int k0, int nk, double *surr_host);
/* the same from the KL kernel variants: sq_host[2 j] = the surrogate sum (trpo_dev_surrogate's bits),
 * sq_host[2 j + 1] = q = sum_n sum_i (Mean_old - mean_k)^2 exp(-2 LogStd_k,i), both over all ranks */
int trpo_dev_surrogate_kl(trpo_dev *d, const double *fullstep, int k0, int nk, double *sq_host);
/* The device phase of one update with ONE host synchronisation: policy gradient -> slot B,
 * CG(maxiter, resth) -> slot X, FVP(x) -> slot Z; then b, x, z, sum(Adv), the CG iteration count and
 * (optional, capacity maxiter + 1) its rdotr / |x| history to the host, written by one kernel into
 * pinned host memory. */
int trpo_dev_update_solve(trpo_dev *d, size_t maxiter, double resth, double *b, double *x, double *z,
                          double *adv_sum, size_t *iters, double *rdotr_hist, double *xnorm_hist,
                          double max_kl, double *surr0, double *shs_lm, double *stats, double *q0);
/* shs_lm (optional, 2): the step size shs = 0.5 x.Fx and lm = sqrt(shs / max_kl) as the device computed
 * them (fullstep = x / lm, fixed-order sum); surr0 (optional): the surrogate sum of the full step
 * theta + fullstep, the line search's first candidate, in the same synchronisation; q0 (optional, needs
 * surr0): the full step's q as trpo_dev_surrogate_kl gives it, from the KL kernel variant in the same launch. */

/* Value-baseline objective (src/TRPO_Baseline.c), its own small device object. */
typedef struct trpo_bdev trpo_bdev;
trpo_bdev *trpo_bdev_create(int device, size_t nl, const size_t *ls, const char *ac, char *err, size_t errlen);
void trpo_bdev_destroy(trpo_bdev *b);
int trpo_bdev_set_data(trpo_bdev *b, const double *obs, const double *target, size_t n);
int trpo_bdev_eval(trpo_bdev *b, const double *theta, double *gsum, double *pred);
int trpo_bdev_eval_start(trpo_bdev *b, const double *theta, int want_pred);
int trpo_bdev_eval_finish(trpo_bdev *b, double *gsum, double *pred);
/* Advantage stage (trpo_update.hip): upload (observ [n][L0 - 1], reward [n]), V at theta, returns -> the fit
 * target, standardised GAE advantages kept on the device; stats4 = ep_rew_mean, ep_rew_std, adv_mean,
 * adv_std.  -7: an evaluation is in flight; -8: adv_std is zero or not finite (no advantage is kept). */
int trpo_bdev_advantage(trpo_bdev *b, const double *theta, const double *obs, const double *reward, size_t num_ep,
                        size_t ep_len, double gamma, double lam, double *adv_out, double *ret_out, double *stats4);
/* The same for episodes of len[e] >= 1 steps packed back to back, n = their sum, time feature t / horizon
 * (the caller has checked len, n and horizon >= max len); boot (or NULL) flags the truncated episodes, whose
 * value behind the last step is the baseline at [boot_obs[e], len[e] / horizon] instead of 0. */
int trpo_bdev_advantage_ragged(trpo_bdev *b, const double *theta, const double *obs, const double *reward,
                               size_t num_ep, const size_t *len, size_t n, size_t horizon, const double *boot_obs,
                               const unsigned char *boot, double gamma, double lam, double *adv_out, double *ret_out,
                               double *stats4);
/* trpo_dev_set_rollout with adv = b's advantages [first, first + n), interleaved on the device; -1 with the
 * cause in err when b holds none, lives on another device or the slice does not fit */
int trpo_dev_set_rollout_adv(trpo_dev *d, const double *mean, const double *action, const trpo_bdev *b, size_t first,
                             char *err, size_t errlen);
/* Policy inference (trpo_update.hip): mean [m][A] of the policy at the context's theta on obs [m][L0], and with
 * action != NULL the sampled actions [m][A] and (logp != NULL) their log-densities [m]; sample i is row
 * row0 + i * stride of the Philox counter space (the caller has checked the ranges).  keep: (mean, action) of
 * those rows also into the device's kept buffer [n][2A] (every row < n).  form: 0 the measured rule, 1 sample
 * per lane, 2 neuron per lane.  One launch; -6 when it does not finish within $TRPO_ACT_TIMEOUT_MS (10 s). */
int trpo_dev_act(trpo_dev *d, const double *obs, size_t m, unsigned long long seed, unsigned long long step,
                 size_t row0, size_t stride, int keep, int form, double *mean, double *action, double *logp, char *err,
                 size_t errlen);
/* trpo_dev_set_rollout with Mean and Action = the kept rows (all n of them, the caller's bitmap says); exactly
 * one of adv (host [n]) and b (its advantages [first, first + n)); -1 with the cause in err, rollout untouched */
int trpo_dev_set_rollout_acted(trpo_dev *d, const double *adv, const trpo_bdev *b, size_t first, char *err,
                               size_t errlen);
/* Rollout record (trpo_update.hip): device buffers rec_obs [rows][L0] and rec_kept [rows][2A] that
 * trpo_dev_act fills (rec != 0: obs_i and (mean_i, action_i) of row r_i, every r_i < rows, checked by the caller)
 * and a commit turns into the context's batch and kept rows.  begin drops a record in progress and allocates
 * (rows >= 1); drop frees one.  commit (len == NULL): the record as it stands, n = rows, no copy.  commit with
 * len [num_ep]: sample off[e] + t <- record row e * slot + t, t < len[e], n = sum len (the caller has checked
 * the lengths, num_ep * slot <= rows and n <= INT_MAX), gathered by one kernel.  Which rows are recorded is the
 * caller's bookkeeping.  A commit that returns -1 has changed nothing. */
int trpo_dev_record_begin(trpo_dev *d, size_t rows);
void trpo_dev_record_drop(trpo_dev *d);
int trpo_dev_record_commit(trpo_dev *d, size_t num_ep, const size_t *len, size_t slot, size_t n);
/* the advantage stage with the observations read on the device from d's batch [n][L0 - 1] (len == NULL: the
 * fixed form, n = num_ep * ep_len); -1 with the cause in err where d does not fit b or the batch */
int trpo_bdev_advantage_dev(trpo_bdev *b, const double *theta, trpo_dev *d, const double *reward, size_t num_ep,
                            size_t ep_len, const size_t *len, size_t n, size_t horizon, const double *boot_obs,
                            const unsigned char *boot, double gamma, double lam, double *adv_out, double *ret_out,
                            double *stats4, char *err, size_t errlen);
/* The device-resident loop (trpo_update.hip): the caller's arrays are device memory (dtype: 0 double,
 * 1 float) and `stream` (a hipStream_t; NULL: the context's own) orders its work.  Each call checks that every
 * array is device memory of the object's device and lies inside its allocation: -1 with the cause in err.
 * act_dev: trpo_dev_act on device arrays, asynchronous.  record_episodes: per slot e of flags [num_env][slot] the
 * first step with a flag set -> len_out[e], trunc_out[e]; one host wait.  advantage_dev_rewards:
 * trpo_bdev_advantage_dev with the rewards [n] (slot == 0) or [num_ep][slot] (ragged) and the ragged form's last
 * observations [num_ep][L0 - 1] on the device. */
int trpo_dev_act_dev(trpo_dev *d, const void *obs, size_t m, unsigned long long seed, unsigned long long step,
                     size_t row0, size_t stride, int keep, int form, int dtype, void *mean, void *action, void *logp,
                     void *stream, char *err, size_t errlen);
int trpo_dev_record_episodes(trpo_dev *d, const unsigned char *term, const unsigned char *trunc, size_t num_env,
                             size_t slot, void *stream, size_t *len_out, unsigned char *trunc_out, char *err,
                             size_t errlen);
int trpo_bdev_advantage_dev_rewards(trpo_bdev *b, const double *theta, trpo_dev *d, const void *reward,
                                    const void *last_obs, int dtype, size_t slot, void *stream, size_t num_ep,
                                    size_t ep_len, const size_t *len, size_t n, size_t horizon,
                                    const unsigned char *boot, double gamma, double lam, double *adv_out,
                                    double *ret_out, double *stats4, char *err, size_t errlen);
/* The observation filter (trpo_update.hip; the contract is the public header's): running moments of
 * the raw rows of the record calls and the frozen (shift, scale) pair the act kernels apply while it is enabled.
 * The caller has checked clip, eps and set's arguments.  -1: bad arguments or the filter is not enabled (apply_dev:
 * or the cause in err).  get: which 0 live, 1 pending; any output may be NULL.  get and apply wait for the
 * stream; everything else is only enqueued. */
#define TRPO_DEV_OBSNORM_CHUNK 64   /* rows per chunk of the statistics' fixed summation order (ON_CHUNK) */
int trpo_dev_obsnorm_enabled(trpo_dev *d);
int trpo_dev_obsnorm_enable(trpo_dev *d, double clip, double eps);
int trpo_dev_obsnorm_disable(trpo_dev *d);
int trpo_dev_obsnorm_fold(trpo_dev *d);
int trpo_dev_obsnorm_get(trpo_dev *d, int which, double *count, double *mean, double *m2, double *shift,
                         double *scale);
int trpo_dev_obsnorm_set(trpo_dev *d, double count, const double *mean, const double *m2);
int trpo_dev_obsnorm_apply(trpo_dev *d, const double *in, size_t m, double *out);
int trpo_dev_obsnorm_apply_dev(trpo_dev *d, const void *in, size_t m, int dtype, void *out, void *stream, char *err,
                               size_t errlen);
/* Trust-region fit of the baseline (trpo_update.hip): Gauss-Newton product, CG, rescale onto the trust region,
 * candidate search, one host wait.  gnvp: out [P] = (1/N) sum j (j.v) + damping v at weights x.  fit_tr: x_out
 * [P], step_out [P] or NULL, info [TRPO_BDEV_VFIT_INFO] or NULL = loss_before, gnorm, shs, alpha_tr, alpha0,
 * cg_iters, accepted, (spare), loss[32], shift[32], rdotr[TRPO_BDEV_VFIT_MAX_CG + 1] (zero beyond cg_iters).
 * -1: bad arguments or no data; -7: an evaluation is in flight; -8: sigma^2 is zero or not finite
 * (x_out = x).  Neither touches the object's data, target or advantages. */
#define TRPO_BDEV_VFIT_MAX_CG 64
#define TRPO_BDEV_VFIT_INFO (8 + 32 + 32 + TRPO_BDEV_VFIT_MAX_CG + 1)
int trpo_bdev_gnvp(trpo_bdev *b, const double *x, const double *v, double damping, double *out);
int trpo_bdev_fit_tr(trpo_bdev *b, const double *x, double eps, size_t maxiter, double resth, double damping, int nk,
                     double shift_cap, double *x_out, double *step_out, double *info);
/* "eval=F predict=F gnvp=F cand=F": the kernel form the evaluate, the advantage stage's prediction pass, the
 * Gauss-Newton product and the fit's candidates take for the object's shape (lane | lds+theta | lds | scratch);
 * "" until the object has seen a batch (the lane rule is read there) */
const char *trpo_bdev_kernel_name(const trpo_bdev *b);

const char *trpo_dev_kernel_name(const trpo_dev *d);
int trpo_dev_geometry(const trpo_dev *d, int *blocks, int *threads, int *lds_bytes);
size_t trpo_dev_num_params(const trpo_dev *d);
double trpo_dev_n_total(const trpo_dev *d);    /* global sample count (all ranks) */
/* launches so far of a tile kernel that ran the forward pass from the observations (not from the cache) */
unsigned long long trpo_dev_forward_passes(const trpo_dev *d);

#ifdef __cplusplus
}
#endif
#endif
