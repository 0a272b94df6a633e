/*
 * trpo_host.c -- C host layer of libtrpo_mi355x.so.
 *
 * Implements the reference's C entry points (src/include/TRPO.h:81-101) and the
 * in-memory context API of include/trpo_mi355x.h on top of the thin device ABI
 * (csrc/trpo_dev.h).  Everything numerical runs on the GPU; this file parses
 * the reference's text formats, caches parsed + uploaded problems, keeps the
 * reference's side effects (CG progress lines, "[ERROR] ..." messages, return
 * conventions) and times the compute region the way the reference does
 * (file parsing excluded).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/time.h>

#include "../../include/trpo_mi355x.h"
#include "trpo_dev.h"
#include "trpo_textio.h"

#define MAX_LAYERS 8

static __thread char g_err[512];

static void set_err(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

const char *trpo_last_error(void) { return g_err; }

static double now_s(void) {
    struct timeval tv;
    gettimeofday(&tv, NULL);
    return (double)tv.tv_sec + 1e-6 * (double)tv.tv_usec;
}

/* src/TRPO_Util.c:7-17 */
size_t NumParamsCalc(size_t *LayerSize, size_t NumLayers) {
    size_t p = 0;
    if (!LayerSize || NumLayers < 1) return 0;
    for (size_t i = 0; i + 1 < NumLayers; ++i) p += LayerSize[i] * LayerSize[i + 1] + LayerSize[i + 1];
    return p + LayerSize[NumLayers - 1];
}

/* ------------------------------------------------------------------------- */
/* contexts                                                                  */
/* ------------------------------------------------------------------------- */
struct trpo_ctx {
    trpo_dev *dev;
    size_t nl;
    size_t ls[MAX_LAYERS];
    char ac[MAX_LAYERS + 1];
    size_t P;
    size_t n;
    double damping;
    double *theta;             /* host copy of the current parameters (line search base) */
    int have_roll;             /* rollout uploaded for the current samples */
    double *stdv;              /* host copy of the action std (the old policy of the KL), valid with have_std */
    int have_std;
    trpo_dev *twin;            /* fp64 twin of the problem (the fp32 stall guard's re-solve), lazily built */
    unsigned long long twin_fwd;   /* forward passes of the twins dropped so far (trpo_ctx_forward_passes) */
    double last_orth;         /* the last CG solve's orthogonality-loss statistic (ctl->orth) */
    double last_ritz;          /* its smallest relative Ritz residual (the stall guard's test) */
    int last_rerun;            /* 1 when the last solve's result came from the fp64 twin */
    int act_form;              /* trpo_ctx_act's kernel form: 0 the measured rule, 1 lane, 2 neuron ($TRPO_ACT_FORM) */
    unsigned char *kept;       /* bitmap of the rows trpo_ctx_act has kept on the device since the last clear */
    size_t kept_count;
    unsigned char *rec;        /* bitmap of the rows recorded since trpo_ctx_record_begin; NULL: no recording */
    size_t rec_rows, rec_count;
    int wide;                  /* a wide-policy context (trpo_ctx_create_wide): solver at any size, one rank, fp32 */
};

/* The default device solver holds at most 32 768 parameters (the CG kernels: 32 per thread of one 1024-thread
 * block).  A larger policy gets from trpo_ctx_create a context that serves policy inference only -- trpo_ctx_act,
 * trpo_ctx_act_clear and the setters, whose kernels and buffers are sized by the parameter count alone; every
 * entry point that runs the FVP, the CG, the update path or a collective refuses it with TRPO_E_INVALID.
 * trpo_ctx_create_wide gives a context of the wide-policy path, whose solver has no such bound. */
#define TRPO_SOLVER_MAX_PARAMS 32768
static int solver_refused(const trpo_ctx *c, const char *who) {
    if (!c || c->wide || c->P <= TRPO_SOLVER_MAX_PARAMS) return 0;
    set_err("%s: NumParams=%zu exceeds the %d supported by the device CG; this context serves inference only", who,
            c->P, TRPO_SOLVER_MAX_PARAMS);
    return 1;
}

/* what a wide-policy context does not serve: collectives and the kernel-only timing launch */
static int wide_refused(const trpo_ctx *c, const char *who, const char *what) {
    if (!c || !c->wide) return 0;
    set_err("%s: the wide-policy path (trpo_ctx_create_wide) %s", who, what);
    return 1;
}
#define WIDE_NO_COLLECTIVE "runs on one rank: it has no collectives"

/* fp32 stall guard.  The fp32 path reorthogonalises every new CG residual
 * and so converges like exact-arithmetic CG.  The reference's plain fp64 recurrence
 * (src/TRPO_CG.c:65-103) does not where its residuals lose orthogonality -- which, by Paige's theory of
 * the Lanczos process, happens once a Ritz value of the solve has converged to near machine precision:
 * |q . r_k| ~ eps ||A|| / (Ritz residual).  The solve's own CG coefficients give that test: alpha_k and
 * beta_k = rdotr_{k+1} / rdotr_k form the Lanczos matrix T_k, and a Ritz pair (theta, s) of T_k has the
 * residual sqrt(beta_k) / alpha_k |s_k|.  When the smallest one, relative to the largest Ritz value,
 * falls below TRPO_RITZ_RERUN (default 1e-15, about 10 eps64) the reference's own step is its rounding's,
 * not the exact one (random-shape draw 23: 7e-17, the fp32 step 1.2e-3 from the reference; the next
 * smallest case 1.6e-15, 7e-6; tools/diag/ritz_probe.py), and the solve is repeated in fp64 on a twin of
 * the context (the reference's arithmetic, no reorthogonalisation), built on first use from the
 * context's own device-resident problem.  One rank only: a sharded context reports the statistic
 * (trpo_ctx_cg_status) and warns.  The coefficients of the fp32 trajectory carry ~1e-7 relative noise;
 * the Ritz residual is insensitive to it (the probe perturbs them: unchanged to 2 digits). */
static double ritz_threshold(void) {
    const char *e = getenv("TRPO_RITZ_RERUN");
    return e ? atof(e) : 1e-14;
}

/* eigenvalues d[] of the symmetric tridiagonal matrix (diagonal d, e[i] = T[i][i+1] for i < n - 1) and
 * the LAST components zl[] of its eigenvectors: implicit QL with Wilkinson shifts, the last row of the
 * eigenvector matrix carried alone (O(n^2)); -1 if it does not converge */
static int tql_last(double *d, double *e, double *zl, int n) {
    for (int i = 0; i < n; ++i) zl[i] = i == n - 1 ? 1.0 : 0.0;
    e[n - 1] = 0.0;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) {
                const double dd = fabs(d[m]) + fabs(d[m + 1]);
                if (fabs(e[m]) <= 2.2e-16 * dd) break;
            }
            if (m != l) {
                if (iter++ == 60) return -1;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + copysign(r, g));
                double sn = 1.0, cs = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; --i) {
                    double f = sn * e[i];
                    const double b = cs * e[i];
                    e[i + 1] = (r = hypot(f, g));
                    if (r == 0.0) {
                        d[i + 1] -= p;
                        e[m] = 0.0;
                        break;
                    }
                    sn = f / r;
                    cs = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * sn + 2.0 * cs * b;
                    d[i + 1] = g + (p = sn * r);
                    g = cs * r - b;
                    f = zl[i + 1];                       /* the last eigenvector row, rotated alone */
                    zl[i + 1] = sn * zl[i] + cs * f;
                    zl[i] = cs * zl[i] - sn * f;
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[m] = 0.0;
            }
        } while (m != l);
    }
    return 0;
}

/* smallest relative Ritz residual of the Lanczos matrix T_iters of a CG solve (alpha_k, rdotr_k as the
 * device recorded them; iters <= 64); 1 when there is nothing to test.  Only the last T: a Ritz value
 * that has converged stays converged, and over the goldens and the 36 random draws the minimum over
 * T_1 .. T_iters always sat at the last one (tools/diag/ritz_probe.py); ~1 us on the host for 10 steps. */
static double ritz_min(const double *alpha, const double *rdotr, size_t iters) {
    int K = iters > 64 ? 64 : (int)iters;
    for (int j = 0; j < K; ++j)                /* the valid prefix (a converged solve stops early) */
        if (!(alpha[j] > 0.0) || !(rdotr[j] > 0.0) || !isfinite(alpha[j]) || !(rdotr[j + 1] >= 0.0)) {
            K = j;
            break;
        }
    if (K < 1) return 1.0;
    double d[64], e[64], zl[64];
    for (int j = 0; j < K; ++j) {
        d[j] = 1.0 / alpha[j] + (j > 0 ? (rdotr[j] / rdotr[j - 1]) / alpha[j - 1] : 0.0);
        e[j] = j + 1 < K ? sqrt(rdotr[j + 1] / rdotr[j]) / alpha[j] : 0.0;
    }
    if (tql_last(d, e, zl, K)) return 1.0;
    double wmax = 0.0, best = 1.0;
    for (int i = 0; i < K; ++i) wmax = fabs(d[i]) > wmax ? fabs(d[i]) : wmax;
    const double bk = sqrt(rdotr[K] / rdotr[K - 1]) / alpha[K - 1];
    for (int i = 0; i < K && wmax > 0.0; ++i) {
        const double res = bk * fabs(zl[i]) / wmax;
        best = res < best ? res : best;
    }
    return best;
}

static void drop_twin(trpo_ctx *c) {
    if (c && c->twin) {
        c->twin_fwd += trpo_dev_forward_passes(c->twin);
        trpo_dev_destroy(c->twin);
        c->twin = NULL;
    }
}

/* stats = [orth, alpha_0 .. alpha_63] and the rdotr history of the solve just run */
static int needs_rerun(trpo_ctx *c, const double *stats, const double *rdotr, size_t iters) {
    c->last_orth = stats[0];
    c->last_ritz = ritz_min(stats + 1, rdotr, iters);
    const double th = ritz_threshold();
    if (!(th > 0.0) || !(c->last_ritz < th) || trpo_dev_is_f64(c->dev)) return 0;
    if (c->wide) {                             /* no fp64 twin of this path: report and warn, as sharded contexts */
        fprintf(stderr, "[WARN] CG: a Ritz value converged to %.1e (relative residual): the reference's fp64 CG "
                        "loses orthogonality here; wide-policy context, not re-solved in fp64\n", c->last_ritz);
        return 0;
    }
    int world = 1;
    trpo_dev_comm_info(c->dev, NULL, &world, NULL);
    if (world > 1) {
        fprintf(stderr, "[WARN] CG: a Ritz value converged to %.1e (relative residual): the reference's fp64 CG "
                        "loses orthogonality here; sharded context, not re-solved in fp64\n", c->last_ritz);
        return 0;
    }
    return 1;
}

static trpo_dev *get_twin(trpo_ctx *c) {
    if (c->twin) return c->twin;
    char err[256] = {0};
    trpo_dev *t = trpo_dev_create_prec(trpo_dev_device(c->dev), c->nl, c->ls, c->ac, 1, err, sizeof err);
    if (!t) {
        set_err("fp64 twin: %s", err);
        return NULL;
    }
    const size_t L0 = c->ls[0], A = c->ls[c->nl - 1], n = c->n;
    double *obs = (double *)malloc(sizeof(double) * (n * L0 + 1)), *stdv = (double *)malloc(sizeof(double) * A);
    double *roll = c->have_roll ? (double *)malloc(sizeof(double) * (n * (2 * A + 1) + 1)) : NULL;
    int rc = (!obs || !stdv || (c->have_roll && !roll)) ? TRPO_E_NOMEM : trpo_dev_get_obs(c->dev, obs);
    if (!rc) rc = trpo_dev_get_std(c->dev, stdv);
    if (!rc) rc = trpo_dev_set_theta(t, c->theta);
    if (!rc) rc = trpo_dev_set_std(t, stdv);
    if (!rc) rc = trpo_dev_set_obs(t, obs, n);
    if (!rc) rc = trpo_dev_set_damping(t, c->damping);
    if (!rc && c->have_roll) {
        rc = trpo_dev_get_rollout(c->dev, roll, roll + n * A, roll + 2 * n * A);
        if (!rc) rc = trpo_dev_set_rollout(t, roll, roll + n * A, roll + 2 * n * A, n);
    }
    free(obs);
    free(stdv);
    free(roll);
    if (rc) {
        set_err("fp64 twin: rebuilding the problem failed (code %d)", rc);
        trpo_dev_destroy(t);
        return NULL;
    }
    c->twin = t;
    return t;
}

static int check_shape(size_t nl, const size_t *ls, const char *ac) {
    if (nl < 2 || nl > MAX_LAYERS || !ls || !ac) {
        set_err("unsupported NumLayers=%zu (2..%d)", nl, MAX_LAYERS);
        return -1;
    }
    for (size_t i = 0; i < nl; ++i)
        if (ls[i] == 0) {
            set_err("LayerSize[%zu] is 0", i);
            return -1;
        }
    for (size_t i = 1; i < nl; ++i)
        if (ac[i] != 'l' && ac[i] != 't' && ac[i] != 'o' && ac[i] != 's') {
            set_err("AC Function for Layer[%zu] is %c. Unsupported.", i, ac[i]);
            return -1;
        }
    return 0;
}

static trpo_ctx *ctx_create(size_t num_layers, const size_t *layer_size, const char *acfunc, const double *theta,
                            const double *obs, size_t n, const double *stdv, double cg_damping, int device, int wide) {
    if (check_shape(num_layers, layer_size, acfunc)) return NULL;
    trpo_ctx *c = (trpo_ctx *)calloc(1, sizeof(trpo_ctx));
    if (!c) return NULL;
    c->nl = num_layers;
    memcpy(c->ls, layer_size, num_layers * sizeof(size_t));
    memcpy(c->ac, acfunc, num_layers);
    c->P = NumParamsCalc(c->ls, c->nl);
    c->wide = wide;
    char err[256] = {0};
    if (wide) {
        /* the bound of the path's index arithmetic (trpo_dev.h), checked in size_t before any int holds P */
        size_t p = 0;
        for (size_t i = 0; i + 1 < num_layers && p <= TRPO_WIDE_MAX_PARAMS; ++i) {
            if (layer_size[i] > TRPO_WIDE_MAX_PARAMS || layer_size[i + 1] > TRPO_WIDE_MAX_PARAMS) p = TRPO_WIDE_MAX_PARAMS + 1;
            else p += layer_size[i] * layer_size[i + 1] + layer_size[i + 1];
        }
        if (p + layer_size[num_layers - 1] > TRPO_WIDE_MAX_PARAMS) {
            set_err("trpo_ctx_create_wide: the wide-policy path takes at most %zu parameters", TRPO_WIDE_MAX_PARAMS);
            free(c);
            return NULL;
        }
    }
    c->dev = wide ? trpo_dev_create_wide(device, num_layers, layer_size, acfunc, err, sizeof err)
                  : trpo_dev_create(device, num_layers, layer_size, acfunc, err, sizeof err);
    if (!c->dev) {
        set_err("%s", err);
        free(c);
        return NULL;
    }
    c->theta = (double *)calloc(c->P, sizeof(double));
    if (!c->theta) {
        trpo_dev_destroy(c->dev);
        free(c);
        return NULL;
    }
    if (theta) memcpy(c->theta, theta, c->P * sizeof(double));
    c->stdv = (double *)calloc(c->ls[c->nl - 1], sizeof(double));
    if (c->stdv && stdv) {
        memcpy(c->stdv, stdv, c->ls[c->nl - 1] * sizeof(double));
        c->have_std = 1;
    }
    if ((theta && trpo_dev_set_theta(c->dev, theta)) || (stdv && trpo_dev_set_std(c->dev, stdv)) ||
        ((obs || n == 0) && trpo_dev_set_obs(c->dev, obs, n)) || trpo_dev_set_damping(c->dev, cg_damping)) {
        set_err("device initialisation failed (theta/std/obs upload)");
        trpo_ctx_destroy(c);
        return NULL;
    }
    c->n = n;
    c->damping = cg_damping;
    const char *af = getenv("TRPO_ACT_FORM");
    c->act_form = af && !strcmp(af, "lane") ? 1 : (af && !strcmp(af, "neuron") ? 2 : 0);
    return c;
}

trpo_ctx *trpo_ctx_create(size_t num_layers, const size_t *layer_size, const char *acfunc, const double *theta,
                          const double *obs, size_t n, const double *stdv, double cg_damping, int device) {
    return ctx_create(num_layers, layer_size, acfunc, theta, obs, n, stdv, cg_damping, device, 0);
}

trpo_ctx *trpo_ctx_create_wide(size_t num_layers, const size_t *layer_size, const char *acfunc, const double *theta,
                               const double *obs, size_t n, const double *stdv, double cg_damping, int device) {
    return ctx_create(num_layers, layer_size, acfunc, theta, obs, n, stdv, cg_damping, device, 1);
}

void trpo_ctx_destroy(trpo_ctx *c) {
    if (!c) return;
    drop_twin(c);
    trpo_dev_destroy(c->dev);
    free(c->theta);
    free(c->stdv);
    free(c->kept);
    free(c->rec);              /* (the record's device buffers go with the device context) */
    free(c);
}

int trpo_ctx_set_theta(trpo_ctx *c, const double *theta) {
    if (!c || !theta) return TRPO_E_INVALID;
    drop_twin(c);
    int rc = trpo_dev_set_theta(c->dev, theta);
    if (!rc) memcpy(c->theta, theta, c->P * sizeof(double));
    return rc;
}
int trpo_ctx_set_obs(trpo_ctx *c, const double *obs, size_t n) {
    if (!c || (!obs && n)) return TRPO_E_INVALID;
    drop_twin(c);
    int rc = trpo_dev_set_obs(c->dev, obs, n);
    if (!rc) c->n = n;
    c->have_roll = 0;                  /* a rollout belongs to one set of samples */
    trpo_ctx_act_clear(c);             /* and so do the kept rows */
    return rc;
}
int trpo_ctx_set_std(trpo_ctx *c, const double *stdv) {
    if (!c || !stdv) return TRPO_E_INVALID;
    drop_twin(c);
    const int rc = trpo_dev_set_std(c->dev, stdv);
    c->have_std = 0;
    if (!rc && c->stdv) {
        memcpy(c->stdv, stdv, c->ls[c->nl - 1] * sizeof(double));
        c->have_std = 1;
    }
    return rc;
}
int trpo_ctx_set_damping(trpo_ctx *c, double d) {
    if (!c) return TRPO_E_INVALID;
    c->damping = d;
    if (c->twin) trpo_dev_set_damping(c->twin, d);
    return trpo_dev_set_damping(c->dev, d);
}
size_t trpo_ctx_num_params(const trpo_ctx *c) { return c ? c->P : 0; }

int trpo_comm_unique_id(void *id) {
    if (!id) return TRPO_E_INVALID;
    return trpo_dev_comm_unique_id(id);
}
int trpo_ctx_attach_comm(trpo_ctx *c, int rank, int world, const void *id) {
    return trpo_ctx_attach_comm_timeout(c, rank, world, id, 0);
}
int trpo_ctx_attach_comm_timeout(trpo_ctx *c, int rank, int world, const void *id, long timeout_ms) {
    if (!c || (world > 1 && !id)) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_attach_comm")) return TRPO_E_INVALID;
    if (wide_refused(c, "trpo_ctx_attach_comm", WIDE_NO_COLLECTIVE)) return TRPO_E_INVALID;
    drop_twin(c);
    const int rc = trpo_dev_set_comm(c->dev, rank, world, id, timeout_ms);
    if (rc == TRPO_E_TIMEOUT) set_err("RCCL init (rank %d of %d) did not complete within its time limit", rank, world);
    else if (rc) set_err("RCCL attach (rank %d of %d) failed (code %d; ncclCommInitRank's reason on stderr)", rank, world, rc);
    return rc;
}
int trpo_ctx_comm_verify(trpo_ctx *c, long timeout_ms) {
    if (!c) return TRPO_E_INVALID;
    long bad = 0;
    const int rc = trpo_dev_comm_verify(c->dev, timeout_ms, &bad);
    if (rc == TRPO_E_VERIFY) set_err("collective self-check: %ld elements of the test all-reduce differ from the exact sum", bad);
    else if (rc == TRPO_E_TIMEOUT) set_err("collective self-check: the test all-reduce did not complete in time");
    return rc;
}
int trpo_ctx_wait(trpo_ctx *c, long timeout_ms) {
    if (!c) return TRPO_E_INVALID;
    const int rc = trpo_dev_wait(c->dev, timeout_ms);
    if (rc == TRPO_E_TIMEOUT) set_err("the context's stream did not complete in time");
    return rc;
}
int trpo_ctx_comm_abort(trpo_ctx *c) { return c ? trpo_dev_comm_abort(c->dev) : TRPO_E_INVALID; }

trpo_group *trpo_group_create(int world) { return (trpo_group *)trpo_hgroup_create(world); }
void trpo_group_destroy(trpo_group *g) { trpo_hgroup_destroy((trpo_hgroup *)g); }
int trpo_ctx_attach_group(trpo_ctx *c, trpo_group *g, int rank) {
    if (!c || !g) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_attach_group")) return TRPO_E_INVALID;
    if (wide_refused(c, "trpo_ctx_attach_group", WIDE_NO_COLLECTIVE)) return TRPO_E_INVALID;
    const int rc = trpo_dev_set_group(c->dev, (trpo_hgroup *)g, rank);
    if (rc) set_err("attach_group(rank %d) failed (code %d)", rank, rc);
    return rc;
}
int trpo_ctx_comm_info(const trpo_ctx *c, int *rank, int *world, int *replicas) {
    return c ? trpo_dev_comm_info(c->dev, rank, world, replicas) : TRPO_E_INVALID;
}

int trpo_ctx_peer_handle(trpo_ctx *c, void *handle_64) {
    if (!c) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_peer_handle")) return TRPO_E_INVALID;
    if (wide_refused(c, "trpo_ctx_peer_handle", WIDE_NO_COLLECTIVE)) return TRPO_E_INVALID;
    const int rc = trpo_dev_peer_open(c->dev, handle_64);
    if (rc) set_err("peer window open / IPC export failed (code %d)", rc);
    return rc;
}
int trpo_ctx_attach_peers(trpo_ctx *c, int rank, int world, const void *handles) {
    if (!c || !handles) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_attach_peers")) return TRPO_E_INVALID;
    if (wide_refused(c, "trpo_ctx_attach_peers", WIDE_NO_COLLECTIVE)) return TRPO_E_INVALID;
    int rc = trpo_dev_peer_open(c->dev, NULL);
    if (!rc) rc = trpo_dev_set_peers(c->dev, rank, world, handles, NULL);
    if (rc) set_err("attach_peers(rank %d of %d) failed (code %d)", rank, world, rc);
    return rc;
}
int trpo_ctx_attach_peers_local(trpo_ctx *c, int rank, int world, trpo_ctx *const *all) {
    if (!c || !all || world < 1 || world > TRPO_PEER_MAX_RANKS) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_attach_peers_local")) return TRPO_E_INVALID;
    if (wide_refused(c, "trpo_ctx_attach_peers_local", WIDE_NO_COLLECTIVE)) return TRPO_E_INVALID;
    void *w[TRPO_PEER_MAX_RANKS];
    for (int r = 0; r < world; ++r) {
        w[r] = all[r] ? trpo_dev_peer_window(all[r]->dev) : NULL;
        if (!w[r]) {
            set_err("attach_peers_local: rank %d has no open peer window (trpo_ctx_peer_handle first)", r);
            return TRPO_E_INVALID;
        }
    }
    const int rc = trpo_dev_set_peers(c->dev, rank, world, NULL, w);
    if (rc) set_err("attach_peers_local(rank %d of %d) failed (code %d)", rank, world, rc);
    return rc;
}
const char *trpo_ctx_comm_backend(const trpo_ctx *c) { return c ? trpo_dev_comm_backend(c->dev) : ""; }

int trpo_ctx_surrogate(trpo_ctx *c, const double *fullstep, int k0, int nk, double *surr) {
    if (!c || !fullstep || !surr || k0 < 0 || nk < 1 || nk > 64) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_surrogate")) return TRPO_E_INVALID;
    if (!c->have_roll) {
        set_err("surrogate: no rollout uploaded for the current samples (trpo_ctx_set_rollout)");
        return TRPO_E_INVALID;
    }
    const int rc = trpo_dev_surrogate(c->dev, fullstep, k0, nk, surr);
    if (rc) set_err("surrogate failed on the device (code %d)", rc);
    return rc;
}

/* ------------------------------------------------------------------------- */
/* trust-region check (include/trpo_mi355x.h)                   */
/* ------------------------------------------------------------------------- */
#define HALF_LOG_2PIE 1.4189385332046727      /* log(2 pi e) / 2 */

/* the context's std on the host (kept at create / set_std; read back once where the caller never set one) */
static const double *host_std(trpo_ctx *c) {
    if (!c->stdv) return NULL;
    if (!c->have_std) {
        if (trpo_dev_get_std(c->dev, c->stdv)) return NULL;
        c->have_std = 1;
    }
    return c->stdv;
}

/* LogStd i of the candidate theta + stepfrac fullstep, rounded as the device's candidates are */
static double cand_logstd(const trpo_ctx *c, const double *fullstep, double stepfrac, size_t i) {
    const size_t at = c->P - c->ls[c->nl - 1] + i;
    return c->theta[at] + stepfrac * fullstep[at];
}

/* the sample-independent part of KL(old || candidate): sum_i [ls_i - log stdv_i + stdv_i^2 / (2 e^{2 ls_i}) - 1/2] */
static double kl_sigma_term(const trpo_ctx *c, const double *stdv, const double *fullstep, double stepfrac) {
    const size_t A = c->ls[c->nl - 1];
    double t = 0.0;
    for (size_t i = 0; i < A; ++i) {
        const double ls = cand_logstd(c, fullstep, stepfrac, i);
        t += ls - log(stdv[i]) + stdv[i] * stdv[i] / (2.0 * exp(2.0 * ls)) - 0.5;
    }
    return t;
}

int trpo_ctx_surrogate_kl(trpo_ctx *c, const double *fullstep, int k0, int nk, double *surr, double *kl) {
    if (!c || !fullstep || (!surr && !kl) || k0 < 0 || nk < 1 || nk > 64) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_surrogate_kl")) return TRPO_E_INVALID;
    if (!c->have_roll) {
        set_err("surrogate_kl: no rollout uploaded for the current samples (trpo_ctx_set_rollout)");
        return TRPO_E_INVALID;
    }
    const double *stdv = host_std(c);
    if (!stdv) {
        set_err("surrogate_kl: the context's std is unavailable");
        return TRPO_E_DEVICE;
    }
    double sq[128];
    const int rc = trpo_dev_surrogate_kl(c->dev, fullstep, k0, nk, sq);
    if (rc) {
        set_err("surrogate_kl failed on the device (code %d)", rc);
        return rc;
    }
    const double N = trpo_dev_n_total(c->dev);
    for (int j = 0; j < nk; ++j) {
        if (surr) surr[j] = sq[2 * j];
        if (kl) kl[j] = kl_sigma_term(c, stdv, fullstep, pow(0.5, (double)(k0 + j))) + sq[2 * j + 1] / (2.0 * N);
    }
    return 0;
}

double trpo_ctx_fvp(trpo_ctx *c, const double *v, double *out) {
    if (!c || !v || !out) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_fvp")) return TRPO_E_INVALID;
    const double t0 = now_s();
    int rc = trpo_dev_upload(c->dev, TRPO_VEC_V, v);
    if (!rc) rc = trpo_dev_fvp_host(c->dev, out);
    if (rc) {
        set_err("FVP failed on the device (code %d)", rc);
        return rc < 0 ? rc : TRPO_E_DEVICE;
    }
    return now_s() - t0;
}

double trpo_ctx_cg(trpo_ctx *c, const double *b, size_t max_iter, double th, double *x, int verbose) {
    if (!c || !b || !x) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_cg")) return TRPO_E_INVALID;
    const double t0 = now_s();
    double stats[TRPO_CG_STATS], rdh[66];
    size_t its = 0;
    trpo_dev *hd = c->dev;                             /* the context whose solve x comes from */
    c->last_rerun = 0;
    int rc = trpo_dev_upload(c->dev, TRPO_VEC_B, b);
    if (!rc) rc = trpo_dev_cg(c->dev, max_iter, th);
    if (!rc) rc = trpo_dev_download_x_cg(c->dev, x, stats, rdh, 66, &its);
    if (!rc && needs_rerun(c, stats, rdh, its)) {
        trpo_dev *t = get_twin(c);
        if (t) {
            rc = trpo_dev_upload(t, TRPO_VEC_B, b);
            if (!rc) rc = trpo_dev_cg(t, max_iter, th);
            if (!rc) rc = trpo_dev_download(t, TRPO_VEC_X, x);
            /* the context's own slot X then holds the x this call returns (trpo_ctx_download_x agrees) */
            if (!rc) rc = trpo_dev_upload(c->dev, TRPO_VEC_X, x);
            if (!rc) {
                c->last_rerun = 1;
                hd = t;
                fprintf(stderr, "[WARN] CG: a Ritz value converged to %.1e (relative residual), where the "
                                "reference's fp64 CG loses orthogonality; solved again in fp64\n", c->last_ritz);
            }
        } else {
            fprintf(stderr, "[WARN] CG: a Ritz value converged to %.1e and the fp64 re-solve is unavailable: %s\n",
                    c->last_ritz, g_err);
        }
    }
    const double t1 = now_s();
    if (rc) {
        set_err("CG failed on the device (code %d)", rc);
        return rc < 0 ? rc : TRPO_E_DEVICE;
    }
    if (verbose) {
        /* src/TRPO_CG.c:56 -- one line per iteration, rdotr is the squared norm */
        size_t iters = 0;
        double *rr = (double *)malloc(sizeof(double) * (max_iter + 1));
        double *xn = (double *)malloc(sizeof(double) * (max_iter + 1));
        if (rr && xn && !trpo_dev_cg_history(hd, rr, xn, max_iter + 1, &iters)) {
            for (size_t i = 0; i <= iters; ++i)
                printf("CG Iter[%zu] Residual Norm=%.12e, Soln Norm=%.12e\n", i, rr[i], xn[i]);
        }
        free(rr);
        free(xn);
    }
    return t1 - t0;
}

int trpo_ctx_cg_history(const trpo_ctx *c, double *rdotr, double *xnorm, size_t cap, size_t *iters) {
    if (!c) return TRPO_E_INVALID;
    return trpo_dev_cg_history(c->last_rerun && c->twin ? c->twin : c->dev, rdotr, xnorm, cap, iters);
}

int trpo_ctx_cg_status(const trpo_ctx *c, double *ritz_residual, double *orth_loss, int *fp64_rerun) {
    if (!c) return TRPO_E_INVALID;
    if (ritz_residual) *ritz_residual = c->last_ritz;
    if (orth_loss) *orth_loss = c->last_orth;
    if (fp64_rerun) *fp64_rerun = c->last_rerun;
    return 0;
}

/* ------------------------------------------------------------------------- */
/* one TRPO policy update (src/TRPO_Update.c:254-1007)                       */
/* ------------------------------------------------------------------------- */
int trpo_ctx_set_rollout(trpo_ctx *c, const double *mean, const double *action, const double *adv) {
    if (!c || (c->n && (!mean || !action || !adv))) return TRPO_E_INVALID;
    if (solver_refused(c, "trpo_ctx_set_rollout")) return TRPO_E_INVALID;
    drop_twin(c);
    int rc = trpo_dev_set_rollout(c->dev, mean, action, adv, c->n);
    c->have_roll = rc == 0;
    if (rc) set_err("rollout upload failed (code %d)", rc);
    return rc;
}

static trpo_bdev *baseline_bdev(const trpo_baseline *b);

int trpo_ctx_set_rollout_adv(trpo_ctx *c, const double *mean, const double *action, const trpo_baseline *b,
                             size_t first) {
    if (!c || !b) {
        set_err("trpo_ctx_set_rollout_adv: NULL context or baseline");
        return TRPO_E_INVALID;
    }
    if (solver_refused(c, "trpo_ctx_set_rollout_adv")) return TRPO_E_INVALID;
    char err[256] = {0};
    const int rc = trpo_dev_set_rollout_adv(c->dev, mean, action, baseline_bdev(b), first, err, sizeof err);
    if (rc == -1) {                           /* refused: the context's rollout is as it was */
        set_err("trpo_ctx_set_rollout_adv: %s", err[0] ? err : "invalid argument");
        return TRPO_E_INVALID;
    }
    drop_twin(c);
    c->have_roll = rc == 0;
    if (rc) set_err("rollout hand-off failed on the device (code %d)", rc);
    return rc;
}

/* ------------------------------------------------------------------------- */
/* policy inference (no reference counterpart)                  */
/* ------------------------------------------------------------------------- */
static size_t ragged_samples(const char *who, size_t num_ep, const size_t *ep_len, size_t horizon);

static void record_discard(trpo_ctx *c) {
    if (!c->rec) return;
    free(c->rec);
    c->rec = NULL;
    c->rec_rows = c->rec_count = 0;
    trpo_dev_record_drop(c->dev);
}

int trpo_ctx_act_clear(trpo_ctx *c) {
    if (!c) return TRPO_E_INVALID;
    free(c->kept);
    c->kept = NULL;
    c->kept_count = 0;
    record_discard(c);                 /* a recording in progress is a set of kept rows in the making */
    return 0;
}

/* the rows row0 + i * row_stride, i < m, into a bitmap and its count */
static void mark_rows(unsigned char *map, size_t *count, size_t row0, size_t row_stride, size_t m) {
    for (size_t i = 0; i < m; ++i) {
        const size_t r = row0 + i * row_stride;
        if (!(map[r >> 3] >> (r & 7) & 1)) {
            map[r >> 3] |= (unsigned char)(1u << (r & 7));
            ++*count;
        }
    }
}

/* A device call's rc as the public code: 0, or with "who: err (code rc)" as the last error (err NULL or empty:
 * "the device call failed") -1 -> TRPO_E_INVALID, other negatives as they are, anything else TRPO_E_DEVICE. */
static int dev_rc_public(const char *who, int rc, const char *err) {
    if (!rc) return 0;
    set_err("%s: %s (code %d)", who, err && err[0] ? err : "the device call failed", rc);
    return rc == -1 ? TRPO_E_INVALID : (rc < 0 ? rc : TRPO_E_DEVICE);
}

/* The refusals and the bookkeeping of the four act calls around their device call.  keep 0 / 1: trpo_ctx_act and
 * trpo_ctx_act_dev; keep 2: trpo_ctx_act_record and _dev, the rows go into the recording.  dev: the caller's arrays
 * are device memory of dtype (trpo_dev_act_dev, an asynchronous launch ordered against stream) and the messages name
 * its parameters *_dev, not *_out.  Returns what the entry point returns: the host calls the seconds, or the device
 * layer's own negative code; the _dev calls 0, or the public code. */
static double act_body(const char *who, int dev, trpo_ctx *c, const void *obs, size_t m, unsigned long long seed,
                       unsigned long long step, size_t row0, size_t row_stride, int keep, int dtype, void *mean,
                       void *action, void *logp, void *stream) {
    const unsigned long long lim = 1ull << 48;
    const int rec = keep == 2;
    const char *sfx = dev ? "dev" : "out", *fmt = NULL, *why = NULL;    /* fmt: a message that names parameters */
    char named[64];
    if (!c || !obs || !mean) fmt = dev ? "NULL context, obs_dev or mean_%s" : "NULL context, obs or mean_%s";
    else if (dev && dtype != TRPO_DT_F64 && dtype != TRPO_DT_F32) why = "dtype must be TRPO_DT_F64 or TRPO_DT_F32";
    else if (!m || !row_stride) why = "m and row_stride must be at least 1";
    else if (rec && !action) fmt = "action_%s is required";
    else if (!action && logp) fmt = "logp_%s without action_%s";
    else if (!action && keep) fmt = "keep without action_%s";
    else if (step >= lim) why = "step must be below 2^48";
    else if (row0 >= lim || m - 1 > (lim - 1 - row0) / row_stride) why = "the last row must be below 2^48";
    else if (rec && !c->rec) why = "no recording in progress (trpo_ctx_record_begin)";
    else if (rec && row0 + (m - 1) * row_stride >= c->rec_rows) why = "a row is beyond the recording's rows";
    else if (keep == 1 && row0 + (m - 1) * row_stride >= c->n) why = "a kept row is beyond the context's samples";
    if (fmt) {
        snprintf(named, sizeof named, fmt, sfx, sfx);
        why = named;
    }
    if (why) {
        set_err("%s: %s", who, why);
        return TRPO_E_INVALID;
    }
    if (keep == 1 && !c->kept) {
        c->kept = (unsigned char *)calloc((c->n + 7) / 8, 1);
        if (!c->kept) return TRPO_E_NOMEM;
    }
    const double t0 = now_s();
    char err[256] = {0};
    const int rc = dev ? trpo_dev_act_dev(c->dev, obs, m, seed, step, row0, row_stride, keep, c->act_form, dtype, mean,
                                          action, logp, stream, err, sizeof err)
                       : trpo_dev_act(c->dev, (const double *)obs, m, seed, step, row0, row_stride, keep, c->act_form,
                                      (double *)mean, (double *)action, (double *)logp, err, sizeof err);
    if (rc) {
        const int code = dev_rc_public(who, rc, err);
        return dev ? code : rc;
    }
    if (rec) mark_rows(c->rec, &c->rec_count, row0, row_stride, m);
    else if (keep) mark_rows(c->kept, &c->kept_count, row0, row_stride, m);
    return dev ? 0.0 : now_s() - t0;
}

double trpo_ctx_act(trpo_ctx *c, const double *obs, size_t m, unsigned long long seed, unsigned long long step,
                    size_t row0, size_t row_stride, int keep, double *mean_out, double *action_out,
                    double *logp_out) {
    return act_body("trpo_ctx_act", 0, c, obs, m, seed, step, row0, row_stride, keep != 0, 0, mean_out, action_out,
                    logp_out, NULL);
}

/* ------------------------------------------------------------------------- */
/* the rollout record: a batch acted on the device stays there */
/* ------------------------------------------------------------------------- */
int trpo_ctx_record_begin(trpo_ctx *c, size_t rows) {
    if (!c || !rows || rows > (size_t)1 << 30) {
        set_err("trpo_ctx_record_begin: %s", !c ? "NULL context" : "rows must be between 1 and 2^30");
        return TRPO_E_INVALID;
    }
    record_discard(c);
    unsigned char *map = (unsigned char *)calloc((rows + 7) / 8, 1);
    if (!map) return TRPO_E_NOMEM;
    const int rc = trpo_dev_record_begin(c->dev, rows);
    if (rc) {
        free(map);
        char err[96];
        snprintf(err, sizeof err, "the record's device buffers for %zu rows could not be made", rows);
        return dev_rc_public("trpo_ctx_record_begin", rc, err);
    }
    c->rec = map;
    c->rec_rows = rows;
    c->rec_count = 0;
    return 0;
}

double trpo_ctx_act_record(trpo_ctx *c, const double *obs, size_t m, unsigned long long seed, unsigned long long step,
                           size_t row0, size_t row_stride, double *mean_out, double *action_out, double *logp_out) {
    return act_body("trpo_ctx_act_record", 0, c, obs, m, seed, step, row0, row_stride, 2, 0, mean_out, action_out,
                    logp_out, NULL);
}

/* ------------------------------------------------------------------------- */
/* the device-resident loop: the caller's arrays are device memory */
/* ------------------------------------------------------------------------- */
int trpo_ctx_act_dev(trpo_ctx *c, const void *obs_dev, size_t m, unsigned long long seed, unsigned long long step,
                     size_t row0, size_t row_stride, int keep, int dtype, void *mean_dev, void *action_dev,
                     void *logp_dev, void *hip_stream) {
    return (int)act_body("trpo_ctx_act_dev", 1, c, obs_dev, m, seed, step, row0, row_stride, keep != 0, dtype, mean_dev,
                         action_dev, logp_dev, hip_stream);
}

int trpo_ctx_act_record_dev(trpo_ctx *c, const void *obs_dev, size_t m, unsigned long long seed,
                            unsigned long long step, size_t row0, size_t row_stride, int dtype, void *mean_dev,
                            void *action_dev, void *logp_dev, void *hip_stream) {
    return (int)act_body("trpo_ctx_act_record_dev", 1, c, obs_dev, m, seed, step, row0, row_stride, 2, dtype, mean_dev,
                         action_dev, logp_dev, hip_stream);
}

int trpo_ctx_record_episodes_dev(trpo_ctx *c, const unsigned char *terminated_dev, const unsigned char *truncated_dev,
                                 size_t num_env, size_t slot_rows, void *hip_stream, size_t *ep_len_out,
                                 unsigned char *truncated_out) {
    const char *who = "trpo_ctx_record_episodes_dev", *why = NULL;
    if (!c || !terminated_dev || !ep_len_out || !truncated_out)
        why = "NULL context, terminated_dev, ep_len_out or truncated_out";
    else if (!num_env || !slot_rows) why = "num_env and slot_rows must be at least 1";
    if (why) {
        set_err("%s: %s", who, why);
        return TRPO_E_INVALID;
    }
    char err[256] = {0};
    return dev_rc_public(who, trpo_dev_record_episodes(c->dev, terminated_dev, truncated_dev, num_env, slot_rows,
                                                       hip_stream, ep_len_out, truncated_out, err, sizeof err), err);
}

int trpo_ctx_record_info(const trpo_ctx *c, size_t *rows, size_t *recorded) {
    if (!c) {
        set_err("trpo_ctx_record_info: NULL context");
        return TRPO_E_INVALID;
    }
    if (rows) *rows = c->rec ? c->rec_rows : 0;
    if (recorded) *recorded = c->rec ? c->rec_count : 0;
    return 0;
}

/* ------------------------------------------------------------------------- */
/* the observation filter: the refusals, then the device call  */
/* ------------------------------------------------------------------------- */
_Static_assert(TRPO_OBSNORM_CHUNK == TRPO_DEV_OBSNORM_CHUNK, "the header's chunk is the kernel's");

/* NULL context, or (need != 0) a context without the filter: the message names the call */
static int obsnorm_refused(const char *who, const trpo_ctx *c, int need) {
    if (!c) set_err("%s: NULL context", who);
    else if (need && !trpo_dev_obsnorm_enabled(c->dev)) set_err("%s: the filter is not enabled (trpo_ctx_obsnorm_enable)", who);
    else return 0;
    return 1;
}

int trpo_ctx_obsnorm_enable(trpo_ctx *c, double clip, double eps) {
    const char *who = "trpo_ctx_obsnorm_enable";
    if (obsnorm_refused(who, c, 0)) return TRPO_E_INVALID;
    if (!(clip > 0.0) || !(eps >= 0.0)) {              /* NaN fails both comparisons */
        set_err("%s: %s", who, !(clip > 0.0) ? "clip must be above 0 (inf: no clipping)" : "eps must be at least 0");
        return TRPO_E_INVALID;
    }
    return dev_rc_public(who, trpo_dev_obsnorm_enable(c->dev, clip, eps), NULL);
}

int trpo_ctx_obsnorm_disable(trpo_ctx *c) {
    const char *who = "trpo_ctx_obsnorm_disable";
    if (obsnorm_refused(who, c, 1)) return TRPO_E_INVALID;
    return dev_rc_public(who, trpo_dev_obsnorm_disable(c->dev), NULL);
}

int trpo_ctx_obsnorm_fold(trpo_ctx *c) {
    const char *who = "trpo_ctx_obsnorm_fold";
    if (obsnorm_refused(who, c, 1)) return TRPO_E_INVALID;
    return dev_rc_public(who, trpo_dev_obsnorm_fold(c->dev), NULL);
}

int trpo_ctx_obsnorm_get(const trpo_ctx *c, int which, double *count, double *mean, double *m2, double *shift,
                         double *scale) {
    const char *who = "trpo_ctx_obsnorm_get";
    if (obsnorm_refused(who, c, 1)) return TRPO_E_INVALID;
    if ((which != 0 && which != 1) || (which == 1 && (shift || scale))) {
        set_err("%s: %s", who, which == 1 ? "shift and scale belong to the live statistics (which = 0)"
                                          : "which must be 0 (live) or 1 (pending)");
        return TRPO_E_INVALID;
    }
    return dev_rc_public(who, trpo_dev_obsnorm_get(c->dev, which, count, mean, m2, shift, scale), NULL);
}

int trpo_ctx_obsnorm_set(trpo_ctx *c, double count, const double *mean, const double *m2) {
    const char *who = "trpo_ctx_obsnorm_set", *why = NULL;
    if (obsnorm_refused(who, c, 1)) return TRPO_E_INVALID;
    if (!mean || !m2) why = "NULL mean or m2";
    else if (!(count >= 0.0) || count != floor(count) || count > 9007199254740992.0)
        why = "count must be a whole number between 0 and 2^53";
    for (size_t k = 0; !why && k < c->ls[0]; ++k) {
        if (!isfinite(mean[k])) why = "mean must be finite";
        else if (!(m2[k] >= 0.0) || !isfinite(m2[k])) why = "m2 must be finite and at least 0";
    }
    if (why) {
        set_err("%s: %s", who, why);
        return TRPO_E_INVALID;
    }
    return dev_rc_public(who, trpo_dev_obsnorm_set(c->dev, count, mean, m2), NULL);
}

int trpo_ctx_obsnorm_apply(const trpo_ctx *c, const double *in, size_t m, double *out) {
    const char *who = "trpo_ctx_obsnorm_apply";
    if (obsnorm_refused(who, c, 1)) return TRPO_E_INVALID;
    if (!in || !out || !m || m > ((size_t)1 << 40) / c->ls[0]) {
        set_err("%s: %s", who, !in || !out ? "NULL in or out" : "m must be at least 1 and m * L0 at most 2^40");
        return TRPO_E_INVALID;
    }
    return dev_rc_public(who, trpo_dev_obsnorm_apply(c->dev, in, m, out), NULL);
}

int trpo_ctx_obsnorm_apply_dev(trpo_ctx *c, const void *in_dev, size_t m, int dtype, void *out_dev, void *hip_stream) {
    const char *who = "trpo_ctx_obsnorm_apply_dev", *why = NULL;
    if (obsnorm_refused(who, c, 1)) return TRPO_E_INVALID;
    if (!in_dev || !out_dev) why = "NULL in_dev or out_dev";
    else if (dtype != TRPO_DT_F64 && dtype != TRPO_DT_F32) why = "dtype must be TRPO_DT_F64 or TRPO_DT_F32";
    else if (!m || m > ((size_t)1 << 40) / c->ls[0]) why = "m must be at least 1 and m * L0 at most 2^40";
    if (why) {
        set_err("%s: %s", who, why);
        return TRPO_E_INVALID;
    }
    char err[256] = {0};
    return dev_rc_public(who, trpo_dev_obsnorm_apply_dev(c->dev, in_dev, m, dtype, out_dev, hip_stream, err, sizeof err),
                         err);
}

static int rec_has(const trpo_ctx *c, size_t r) { return c->rec[r >> 3] >> (r & 7) & 1; }

/* The validated commit: kept (n bits, all set; ownership passes here) becomes the kept rows' bitmap.  What
 * trpo_ctx_set_obs does to the context happens here too: n, the rollout, the twin. */
static int record_finish(const char *who, trpo_ctx *c, size_t num_ep, const size_t *ep_len, size_t slot_rows, size_t n,
                         unsigned char *kept) {
    const int rc = trpo_dev_record_commit(c->dev, num_ep, ep_len, slot_rows, n);
    if (rc == -1) {                            /* refused on the device: nothing has changed */
        if (kept != c->rec) free(kept);
        set_err("%s: the batch of %zu rows is beyond the device kernels' indexing", who, n);
        return TRPO_E_INVALID;
    }
    drop_twin(c);
    free(c->kept);
    c->kept = kept;
    c->kept_count = n;
    if (c->rec != kept) free(c->rec);
    c->rec = NULL;
    c->rec_rows = c->rec_count = 0;
    if (!rc) c->n = n;
    c->have_roll = 0;
    if (rc) set_err("%s: the commit failed on the device (code %d)", who, rc);
    return rc;
}

int trpo_ctx_record_commit(trpo_ctx *c) {
    if (!c || !c->rec) {
        set_err("trpo_ctx_record_commit: %s", !c ? "NULL context" : "no recording in progress (trpo_ctx_record_begin)");
        return TRPO_E_INVALID;
    }
    if (c->rec_count != c->rec_rows) {
        size_t r = 0;
        while (r < c->rec_rows && rec_has(c, r)) ++r;
        set_err("trpo_ctx_record_commit: row %zu has not been recorded (%zu of %zu rows have)", r, c->rec_count,
                c->rec_rows);
        return TRPO_E_INVALID;
    }
    return record_finish("trpo_ctx_record_commit", c, 0, NULL, 0, c->rec_rows, c->rec);   /* every bit is set */
}

int trpo_ctx_record_commit_ragged(trpo_ctx *c, size_t num_ep, const size_t *ep_len, size_t slot_rows) {
    const char *who = "trpo_ctx_record_commit_ragged";
    if (!c || !c->rec) {
        set_err("%s: %s", who, !c ? "NULL context" : "no recording in progress (trpo_ctx_record_begin)");
        return TRPO_E_INVALID;
    }
    for (size_t e = 0; ep_len && e < num_ep; ++e)
        if (ep_len[e] > slot_rows) {
            set_err("%s: ep_len[%zu] = %zu exceeds slot_rows = %zu", who, e, ep_len[e], slot_rows);
            return TRPO_E_INVALID;
        }
    const size_t n = ragged_samples(who, num_ep, ep_len, slot_rows);     /* ep_len[e] >= 1, the sum <= INT_MAX */
    if (!n) return TRPO_E_INVALID;
    if (slot_rows > c->rec_rows / num_ep) {
        set_err("%s: %zu episodes of %zu slot rows exceed the recording's %zu rows", who, num_ep, slot_rows,
                c->rec_rows);
        return TRPO_E_INVALID;
    }
    for (size_t e = 0; e < num_ep; ++e)
        for (size_t t = 0; t < ep_len[e]; ++t)
            if (!rec_has(c, e * slot_rows + t)) {
                set_err("%s: row %zu (episode %zu, step %zu) has not been recorded", who, e * slot_rows + t, e, t);
                return TRPO_E_INVALID;
            }
    unsigned char *kept = (unsigned char *)calloc((n + 7) / 8, 1);
    if (!kept) return TRPO_E_NOMEM;
    memset(kept, 0xff, n / 8);
    if (n & 7) kept[n / 8] = (unsigned char)((1u << (n & 7)) - 1);
    return record_finish(who, c, num_ep, ep_len, slot_rows, n, kept);
}

int trpo_ctx_set_rollout_acted(trpo_ctx *c, const double *adv, const trpo_baseline *b, size_t first) {
    const char *why = NULL;
    if (!c) why = "NULL context";
    else if ((adv == NULL) == (b == NULL)) why = "exactly one of adv and the baseline must be given";
    else if (c->kept_count != c->n) why = "not every row of the context has been kept since the last clear";
    if (why) {
        set_err("trpo_ctx_set_rollout_acted: %s", why);
        return TRPO_E_INVALID;
    }
    if (solver_refused(c, "trpo_ctx_set_rollout_acted")) return TRPO_E_INVALID;
    char err[256] = {0};
    const int rc = trpo_dev_set_rollout_acted(c->dev, adv, b ? baseline_bdev(b) : NULL, first, err, sizeof err);
    if (rc == -1) {                           /* refused: the context's rollout is as it was */
        set_err("trpo_ctx_set_rollout_acted: %s", err[0] ? err : "invalid argument");
        return TRPO_E_INVALID;
    }
    drop_twin(c);
    c->have_roll = rc == 0;
    if (rc) set_err("rollout hand-off failed on the device (code %d)", rc);
    return rc;
}

/* The one body of trpo_ctx_update (with_kl = 0: the reference's line search, no KL formed anywhere) and
 * trpo_ctx_update_kl (with_kl = 1: every candidate's {surr, q} from the KL kernel variants, acceptance also
 * requires kl <= kl_cap). */
static double update_body(trpo_ctx *c, size_t max_iter, double resth, double max_kl, int max_bt, double accept,
                          double *theta_out, double *b_out, double *x_out, trpo_update_info *info, int verbose,
                          int with_kl, double kl_cap, trpo_trust_info *trust) {
    const char *who = with_kl ? "trpo_ctx_update_kl" : "trpo_ctx_update";
    if (!c || !theta_out || max_bt < 0 || max_bt > TRPO_MAX_BACKTRACKS || !(max_kl > 0)) return TRPO_E_INVALID;
    if (solver_refused(c, who)) return TRPO_E_INVALID;
    if (with_kl && !(kl_cap > 0)) {
        set_err("%s: kl_cap must be positive (INFINITY: no cap)", who);
        return TRPO_E_INVALID;
    }
    if (!c->have_roll) {
        set_err("%s: no rollout for the current samples (trpo_ctx_set_rollout)", who);
        return TRPO_E_INVALID;
    }
    const double *stdv = with_kl ? host_std(c) : NULL;
    if (with_kl && !stdv) {
        set_err("%s: the context's std is unavailable", who);
        return TRPO_E_DEVICE;
    }
    trpo_trust_info tr;
    memset(&tr, 0, sizeof tr);
    tr.kl_cap = kl_cap;
    const size_t P = c->P;
    double *b = (double *)malloc(sizeof(double) * P), *x = (double *)malloc(sizeof(double) * P);
    double *z = (double *)malloc(sizeof(double) * P), *fullstep = (double *)malloc(sizeof(double) * P);
    trpo_update_info inf;
    memset(&inf, 0, sizeof inf);
    inf.accepted = -1;
    double ret = TRPO_E_NOMEM;
    if (!b || !x || !z || !fullstep) goto out;
    const double t0 = now_s();
    double adv_sum = 0.0, surr0 = 0.0, q0 = 0.0, shs_lm[2] = {0.0, 0.0};
    double *const q0p = (with_kl && max_bt > 0) ? &q0 : NULL;
    /* policy gradient (:254-378), CG (:383-628) and FVP(x) (:633-832) on the device, one sync */
    double *rr = (double *)malloc(sizeof(double) * (max_iter + 1));
    double *xn = (double *)malloc(sizeof(double) * (max_iter + 1));
    double stats[TRPO_CG_STATS];
    trpo_dev *dv = c->dev;                 /* the context the update's results come from */
    c->last_rerun = 0;
    int rc = (!rr || !xn) ? TRPO_E_NOMEM
                          : trpo_dev_update_solve(c->dev, max_iter, resth, b, x, z, &adv_sum, &inf.cg_iters, rr, xn,
                                                  max_kl, max_bt > 0 ? &surr0 : NULL, shs_lm, stats, q0p);
    if (!rc && needs_rerun(c, stats, rr, inf.cg_iters < max_iter ? inf.cg_iters : max_iter)) {
        /* the fp32 stall guard: the whole device phase again on the fp64 twin (its line search too) */
        trpo_dev *t = get_twin(c);
        if (t) {
            rc = trpo_dev_update_solve(t, max_iter, resth, b, x, z, &adv_sum, &inf.cg_iters, rr, xn, max_kl,
                                       max_bt > 0 ? &surr0 : NULL, shs_lm, NULL, q0p);
            if (!rc) {
                dv = t;
                c->last_rerun = 1;
                fprintf(stderr, "[WARN] TRPO_Update: a Ritz value of the CG solve converged to %.1e (relative "
                                "residual), where the reference's fp64 CG loses orthogonality; update solved again "
                                "in fp64\n", c->last_ritz);
            }
        } else {
            fprintf(stderr, "[WARN] TRPO_Update: a Ritz value converged to %.1e and the fp64 re-solve is "
                            "unavailable: %s\n", c->last_ritz, g_err);
        }
    }
    if (!rc && verbose) /* src/TRPO_CG.c:56 -- one line per iteration */
        for (size_t i = 0; i <= inf.cg_iters && i <= max_iter; ++i)
            printf("CG Iter[%zu] Residual Norm=%.12e, Soln Norm=%.12e\n", i, rr[i], xn[i]);
    free(rr);
    free(xn);
    if (rc) {
        set_err("TRPO update failed on the device (code %d)", rc);
        ret = rc < 0 ? rc : TRPO_E_DEVICE;
        goto out;
    }
    /* step size (src/TRPO_Update.c:834-868), fp64 on the host, reference order */
    /* shs = 0.5 x.Fx and lm = sqrt(shs / max_kl) (:836-846) as the device summed them: its fullstep
     * x / lm -- the first line-search candidate it already evaluated -- is the one below, bit for bit */
    const double shs = shs_lm[0];
    if (verbose) printf("shs: %.14f\n", shs);
    const double lm = shs_lm[1];
    double gnorm = 0;
    for (size_t i = 0; i < P; ++i) gnorm += b[i] * b[i];
    gnorm = sqrt(gnorm);
    if (verbose) printf("lagrange multiplier: %.14f, gnorm: %.14f\n", lm, gnorm);
    for (size_t i = 0; i < P; ++i) fullstep[i] = x[i] / lm;
    double neggdotstepdir = 0;
    for (size_t i = 0; i < P; ++i) neggdotstepdir += b[i] * x[i];
    memcpy(theta_out, x, P * sizeof(double));        /* reference quirk: theta starts as x */
    const double rate = neggdotstepdir / lm;
    const double N = trpo_dev_n_total(dv);
    const double fval = -adv_sum / N;
    if (verbose) printf("fval before %.14e\n", fval);
    inf.shs = shs;
    inf.lagrange = lm;
    inf.gnorm = gnorm;
    inf.fval_before = fval;
    inf.expected_improve_rate = rate;
    /* backtracking line search (src/TRPO_Update.c:884-1007): fraction 1 alone first
     * (the usual outcome), then every remaining fraction in one launch; the accepted
     * one is the first in order, exactly as the sequential reference loop finds it */
    for (int k0 = 0; k0 < max_bt && inf.accepted < 0;) {
        const int nk = k0 == 0 ? 1 : max_bt - k0;
        double surr[TRPO_MAX_BACKTRACKS], q[TRPO_MAX_BACKTRACKS];
        if (k0 == 0) {
            surr[0] = surr0;       /* evaluated by the device with the solve (same fullstep, bit for bit) */
            q[0] = q0;
        } else if (with_kl) {
            double sq[2 * TRPO_MAX_BACKTRACKS];
            rc = trpo_dev_surrogate_kl(dv, fullstep, k0, nk, sq);
            for (int j = 0; j < nk && !rc; ++j) surr[j] = sq[2 * j], q[j] = sq[2 * j + 1];
        } else {
            rc = trpo_dev_surrogate(dv, fullstep, k0, nk, surr);
        }
        if (rc) {
            set_err("line search failed on the device (code %d)", rc);
            ret = rc < 0 ? rc : TRPO_E_DEVICE;
            goto out;
        }
        for (int j = 0; j < nk; ++j) {
            const int k = k0 + j;
            const double stepfrac = pow(0.5, (double)k);
            const double newfval = -surr[j] / N;
            const double actual = fval - newfval, expected = rate * stepfrac, ratio = actual / expected;
            if (verbose) printf("a/e/r %.14f / %.14f / %.14f\n", actual, expected, ratio);
            inf.actual[k] = actual;
            inf.expected[k] = expected;
            inf.ratio[k] = ratio;
            inf.evaluated = k + 1;
            if (with_kl) {
                tr.kl[k] = kl_sigma_term(c, stdv, fullstep, stepfrac) + q[j] / (2.0 * N);
                if (verbose) printf("kl %.14f\n", tr.kl[k]);
            }
            if (ratio > accept && actual > 0) {
                if (with_kl && !(tr.kl[k] <= kl_cap)) {
                    ++tr.kl_rejected;      /* outside the trust region: the next fraction */
                    continue;
                }
                for (size_t i = 0; i < P; ++i) theta_out[i] = c->theta[i] + stepfrac * fullstep[i];
                inf.accepted = k;
                break;
            }
        }
        k0 += nk;
    }
    ret = now_s() - t0;
    if (b_out) memcpy(b_out, b, P * sizeof(double));
    if (x_out) memcpy(x_out, x, P * sizeof(double));
    if (info) *info = inf;
    if (with_kl && trust) {
        const size_t A = c->ls[c->nl - 1];
        for (size_t i = 0; i < A; ++i) {
            tr.entropy_old += log(stdv[i]) + HALF_LOG_2PIE;
            tr.entropy_new += theta_out[P - A + i] + HALF_LOG_2PIE;
        }
        if (inf.accepted < 0) tr.entropy_new = tr.entropy_old;
        *trust = tr;
    }
out:
    free(b);
    free(x);
    free(z);
    free(fullstep);
    return ret;
}

double trpo_ctx_update(trpo_ctx *c, size_t max_iter, double resth, double max_kl, int max_bt, double accept,
                       double *theta_out, double *b_out, double *x_out, trpo_update_info *info, int verbose) {
    return update_body(c, max_iter, resth, max_kl, max_bt, accept, theta_out, b_out, x_out, info, verbose, 0, 0.0,
                       NULL);
}

double trpo_ctx_update_kl(trpo_ctx *c, size_t max_iter, double resth, double max_kl, int max_bt, double accept,
                          double kl_cap, double *theta_out, double *b_out, double *x_out, trpo_update_info *info,
                          trpo_trust_info *trust, int verbose) {
    return update_body(c, max_iter, resth, max_kl, max_bt, accept, theta_out, b_out, x_out, info, verbose, 1, kl_cap,
                       trust);
}

int trpo_ctx_upload_b(trpo_ctx *c, const double *b) { return c ? trpo_dev_upload(c->dev, TRPO_VEC_B, b) : -1; }
int trpo_ctx_upload_v(trpo_ctx *c, const double *v) { return c ? trpo_dev_upload(c->dev, TRPO_VEC_V, v) : -1; }
int trpo_ctx_enqueue_fvp(trpo_ctx *c) {
    return c && !solver_refused(c, "trpo_ctx_enqueue_fvp") ? trpo_dev_fvp(c->dev) : -1;
}
int trpo_ctx_enqueue_cg(trpo_ctx *c, size_t m, double th) {
    return c && !solver_refused(c, "trpo_ctx_enqueue_cg") ? trpo_dev_cg(c->dev, m, th) : -1;
}
int trpo_ctx_enqueue_fvp_kernel_only(trpo_ctx *c) {
    if (wide_refused(c, "trpo_ctx_enqueue_fvp_kernel_only", "runs the FVP layer by layer: there is no single kernel"))
        return TRPO_E_INVALID;
    return c && !solver_refused(c, "trpo_ctx_enqueue_fvp_kernel_only") ? trpo_dev_fvp_kernel(c->dev) : -1;
}
int trpo_ctx_synchronize(trpo_ctx *c) { return c ? trpo_dev_sync(c->dev) : -1; }
double trpo_ctx_time(trpo_ctx *c, int what, int reps, size_t m, double th) {
    if ((what == 0 || what == 3) && wide_refused(c, "trpo_ctx_time", "runs the FVP layer by layer: there is no single kernel"))
        return TRPO_E_INVALID;
    return c && !solver_refused(c, "trpo_ctx_time") ? trpo_dev_time(c->dev, what, reps, m, th) : -1;
}
int trpo_ctx_download_x(trpo_ctx *c, double *x) { return c ? trpo_dev_download(c->dev, TRPO_VEC_X, x) : -1; }
int trpo_ctx_download_z(trpo_ctx *c, double *z) { return c ? trpo_dev_download(c->dev, TRPO_VEC_Z, z) : -1; }
const char *trpo_ctx_kernel_name(const trpo_ctx *c) { return c ? trpo_dev_kernel_name(c->dev) : ""; }
int trpo_ctx_launch_geometry(const trpo_ctx *c, int *b, int *t, int *l) {
    return c ? trpo_dev_geometry(c->dev, b, t, l) : -1;
}
int trpo_ctx_forward_passes(const trpo_ctx *c, unsigned long long *count) {
    if (!c || !count) return TRPO_E_INVALID;
    /* the fp64 twin is a context of its own (own cache, own counter): its launches count while it lives
     * and stay counted once it is dropped (drop_twin) */
    *count = trpo_dev_forward_passes(c->dev) + c->twin_fwd + (c->twin ? trpo_dev_forward_passes(c->twin) : 0);
    return 0;
}

/* ------------------------------------------------------------------------- */
/* reference text formats                                                    */
/* ------------------------------------------------------------------------- */
/* slurp / load_model / load_data live in trpo_textio.c (a CPU-only unit, also built under
 * AddressSanitizer + UBSan by `make -C oracle asan`) */
#define load_model trpo_text_load_model
#define load_data trpo_text_load_data

/* Optional forward-pass check of the data file's Mean column (src/TRPO_FVP.c:839-844),
 * enabled with TRPO_CHECK_MEAN=1; done once when a data file is (re)loaded. */
static void check_mean(const trpo_ctx *c, const double *theta, const double *obs, const double *mean, size_t n) {
    size_t maxw = 0;
    for (size_t i = 0; i < c->nl; ++i) maxw = c->ls[i] > maxw ? c->ls[i] : maxw;
    double *a = (double *)malloc(maxw * sizeof(double)), *b = (double *)malloc(maxw * sizeof(double));
    for (size_t s = 0; s < n; ++s) {
        memcpy(a, obs + s * c->ls[0], c->ls[0] * sizeof(double));
        size_t pos = 0;
        for (size_t i = 0; i + 1 < c->nl; ++i) {
            const size_t in = c->ls[i], out = c->ls[i + 1];
            for (size_t j = 0; j < out; ++j) {
                double x = theta[pos + in * out + j];
                for (size_t k = 0; k < in; ++k) x += a[k] * theta[pos + k * out + j];
                switch (c->ac[i + 1]) {
                case 't': x = tanh(x); break;
                case 'o': x = 0.1 * x; break;
                case 's': x = 1.0 / (1 + exp(-x)); break;
                default: break;
                }
                b[j] = x;
            }
            memcpy(a, b, out * sizeof(double));
            pos += in * out + out;
        }
        const size_t A = c->ls[c->nl - 1];
        for (size_t i = 0; i < A; ++i) {
            const double e = mean[s * A + i], err = fabs((a[i] - e) / e) * 100;
            if (err > 1) printf("out[%zu] = %e, mean = %e => %.4f%% Difference\n", i, a[i], e, err);
        }
    }
    free(a);
    free(b);
}

/* ------------------------------------------------------------------------- */
/* file-keyed cache for the TRPOparam entry points                           */
/* ------------------------------------------------------------------------- */
#define CACHE_SLOTS 4

typedef struct {
    int used;
    unsigned long long stamp;
    char *model, *data;
    off_t msize, dsize;
    struct timespec mmtime, dmtime;
    size_t nsamples, nl, ls[MAX_LAYERS];
    char ac[MAX_LAYERS + 1];
    trpo_ctx *ctx;
    int has_roll;              /* Mean/Action/Adv uploaded (TRPO_Update) */
} cache_entry;

static cache_entry g_cache[CACHE_SLOTS];
static unsigned long long g_clock;
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;

static void entry_free(cache_entry *e) {
    if (!e->used) return;
    trpo_ctx_destroy(e->ctx);
    free(e->model);
    free(e->data);
    memset(e, 0, sizeof *e);
}

void trpo_cache_clear(void) {
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < CACHE_SLOTS; ++i) entry_free(&g_cache[i]);
    pthread_mutex_unlock(&g_lock);
}

static int same_ts(struct timespec a, struct timespec b) { return a.tv_sec == b.tv_sec && a.tv_nsec == b.tv_nsec; }

/* Upload Mean/Action/Adv of the data file into a cached context (TRPO_Update). */
static int load_rollout(cache_entry *e, const TRPOparam *prm) {
    const size_t nl = prm->NumLayers, O = prm->LayerSize[0], A = prm->LayerSize[nl - 1], n = prm->NumSamples;
    double *obs = (double *)calloc(n * O + 1, sizeof(double)), *stdv = (double *)calloc(A, sizeof(double));
    double *mean = (double *)calloc(n * A + 1, sizeof(double)), *act = (double *)calloc(n * A + 1, sizeof(double));
    double *adv = (double *)calloc(n + 1, sizeof(double));
    int rc = -1;
    if (obs && stdv && mean && act && adv && !load_data(prm->DataFile, O, A, n, obs, stdv, mean, act, adv))
        rc = trpo_ctx_set_rollout(e->ctx, mean, act, adv);
    if (!rc) e->has_roll = 1;
    free(obs);
    free(stdv);
    free(mean);
    free(act);
    free(adv);
    return rc;
}

/* Returns a context for param (parsing + uploading on a miss), or NULL with the
 * reference's "[ERROR] Cannot open ..." message on stderr.  need_roll: also make
 * sure the rollout columns are on the device (TRPO_Update). */
static trpo_ctx *ctx_for_param(const TRPOparam *prm, int need_roll) {
    if (!prm->ModelFile || !prm->DataFile) {
        fprintf(stderr, "[ERROR] Model/Data file name missing.\n");
        return NULL;
    }
    if (check_shape(prm->NumLayers, prm->LayerSize, prm->AcFunc)) {
        fprintf(stderr, "[ERROR] %s\n", g_err);
        return NULL;
    }
    struct stat sm, sd;
    if (stat(prm->ModelFile, &sm) != 0) {
        fprintf(stderr, "[ERROR] Cannot open Model File [%s]. \n", prm->ModelFile);
        return NULL;
    }
    if (stat(prm->DataFile, &sd) != 0) {
        fprintf(stderr, "[ERROR] Cannot open Data File [%s]. \n", prm->DataFile);
        return NULL;
    }
    cache_entry *hit = NULL, *victim = &g_cache[0];
    for (int i = 0; i < CACHE_SLOTS; ++i) {
        cache_entry *e = &g_cache[i];
        if (!e->used) {
            if (victim->used) victim = e;
            continue;
        }
        if (victim->used && e->stamp < victim->stamp) victim = e;
        if (strcmp(e->model, prm->ModelFile) || strcmp(e->data, prm->DataFile)) continue;
        if (e->msize != sm.st_size || e->dsize != sd.st_size || !same_ts(e->mmtime, sm.st_mtim) ||
            !same_ts(e->dmtime, sd.st_mtim))
            continue;
        if (e->nsamples != prm->NumSamples || e->nl != prm->NumLayers) continue;
        if (memcmp(e->ls, prm->LayerSize, prm->NumLayers * sizeof(size_t)) ||
            memcmp(e->ac, prm->AcFunc, prm->NumLayers))
            continue;
        hit = e;
        break;
    }
    if (hit) {
        hit->stamp = ++g_clock;
        if (need_roll && !hit->has_roll && load_rollout(hit, prm)) return NULL;
        return hit->ctx;
    }
    /* miss: parse both files, upload, replace the LRU slot */
    const size_t nl = prm->NumLayers, O = prm->LayerSize[0], A = prm->LayerSize[nl - 1], n = prm->NumSamples;
    const size_t P = NumParamsCalc(prm->LayerSize, nl);
    double *theta = (double *)calloc(P, sizeof(double));
    double *obs = (double *)calloc(n * O + 1, sizeof(double));
    double *stdv = (double *)calloc(A, sizeof(double));
    const char *cm = getenv("TRPO_CHECK_MEAN");
    const int want_mean = cm && atoi(cm);
    double *mean = want_mean ? (double *)calloc(n * A + 1, sizeof(double)) : NULL;
    trpo_ctx *ctx = NULL;
    if (!theta || !obs || !stdv) goto out;
    if (load_model(prm->ModelFile, P, theta)) goto out;
    /* FVPFast reads "LogStd" from the model into Std; the data file overwrites it */
    for (size_t k = 0; k < A; ++k) stdv[k] = theta[P - A + k];
    if (load_data(prm->DataFile, O, A, n, obs, stdv, mean, NULL, NULL)) goto out;
    /* beyond the default solver's size these entry points could only fail: they take the wide-policy path */
    ctx = P > TRPO_SOLVER_MAX_PARAMS
              ? trpo_ctx_create_wide(nl, prm->LayerSize, prm->AcFunc, theta, obs, n, stdv, prm->CG_Damping, -1)
              : trpo_ctx_create(nl, prm->LayerSize, prm->AcFunc, theta, obs, n, stdv, prm->CG_Damping, -1);
    if (!ctx) {
        fprintf(stderr, "[ERROR] %s\n", g_err);
        goto out;
    }
    if (want_mean) check_mean(ctx, theta, obs, mean, n);
    entry_free(victim);
    victim->used = 1;
    victim->stamp = ++g_clock;
    victim->model = strdup(prm->ModelFile);
    victim->data = strdup(prm->DataFile);
    victim->msize = sm.st_size;
    victim->dsize = sd.st_size;
    victim->mmtime = sm.st_mtim;
    victim->dmtime = sd.st_mtim;
    victim->nsamples = n;
    victim->nl = nl;
    memcpy(victim->ls, prm->LayerSize, nl * sizeof(size_t));
    memset(victim->ac, 0, sizeof victim->ac);
    memcpy(victim->ac, prm->AcFunc, nl);
    victim->ctx = ctx;
    victim->has_roll = 0;
    if (need_roll && load_rollout(victim, prm)) ctx = NULL;
out:
    free(theta);
    free(obs);
    free(stdv);
    free(mean);
    return ctx;
}

/* ------------------------------------------------------------------------- */
/* the reference entry points                                                */
/* ------------------------------------------------------------------------- */

/* src/TRPO_FVP.c:548-949.  NumThreads sized the reference's OpenMP team; the
 * GPU path has no host compute, so it is accepted and ignored. */
double FVPFast(TRPOparam param, double *Result, double *Input, size_t NumThreads) {
    (void)NumThreads;
    if (!Result || !Input) return -1;
    pthread_mutex_lock(&g_lock);
    trpo_ctx *c = ctx_for_param(&param, 0);
    double t = -1;
    if (c) {
        if (c->damping != param.CG_Damping) trpo_ctx_set_damping(c, param.CG_Damping);
        t = trpo_ctx_fvp(c, Input, Result);
        if (t < 0) {
            fprintf(stderr, "[ERROR] %s\n", g_err);
            t = -1;
        }
    }
    pthread_mutex_unlock(&g_lock);
    return t;
}

/* src/TRPO_FVP.c:11-545: the 4-pass original; mathematically identical to
 * FVPFast because the KL gradient at the old parameters is zero (GLayer=0,
 * src/TRPO_FVP.c:326).  Prints its timing line like the reference (:525). */
double FVP(TRPOparam param, double *Result, double *Input) {
    double t = FVPFast(param, Result, Input, 1);
    if (t >= 0) printf("[INFO] FVP Computing Time is %f seconds.\n", t);
    return t;
}

/* src/TRPO_CG.c:11-113. */
double CG(TRPOparam param, double *Result, double *b, size_t MaxIter, double ResidualTh, size_t NumThreads) {
    (void)NumThreads;
    if (!Result || !b) return -1;
    pthread_mutex_lock(&g_lock);
    trpo_ctx *c = ctx_for_param(&param, 0);
    double t = -1;
    if (c) {
        if (c->damping != param.CG_Damping) trpo_ctx_set_damping(c, param.CG_Damping);
        t = trpo_ctx_cg(c, b, MaxIter, ResidualTh, Result, 1);
        if (t < 0) {
            fprintf(stderr, "[ERROR] Fisher Vector Product Calculation Failed.\n");
            t = -1;
        }
    } else {
        fprintf(stderr, "[ERROR] Fisher Vector Product Calculation Failed.\n");
    }
    fflush(stdout);
    pthread_mutex_unlock(&g_lock);
    return t;
}

/* Accelerator twins (src/include/TRPO.h:98,101): same contract, the MI355X
 * path serves them; PaddedLayerSize / NumBlocks are FPGA-only and ignored. */
double FVP_FPGA(TRPOparam param, double *Result, double *Input) { return FVPFast(param, Result, Input, 1); }

double CG_FPGA(TRPOparam param, double *Result, double *b, size_t MaxIter, double ResidualTh, size_t NumThreads) {
    return CG(param, Result, b, MaxIter, ResidualTh, NumThreads);
}

/* src/TRPO_Update.c:10-1011 with its hard-wired settings: CG MaxIter 10 and
 * ResidualTh 1e-10, MaxKL 0.01, 10 backtracks, AcceptRatio 0.1.  Result receives
 * the updated parameters (or the CG step direction if no backtrack is accepted,
 * like the reference).  The Std of the data file's last line is the FVP sigma;
 * exp(LogStd) of the model is the policy sigma of the gradient and line search. */
double TRPO_Update(TRPOparam param, double *Result, size_t NumThreads) {
    (void)NumThreads;
    if (!Result) return -1;
    pthread_mutex_lock(&g_lock);
    trpo_ctx *c = ctx_for_param(&param, 1);
    double t = -1;
    if (c) {
        if (c->damping != param.CG_Damping) trpo_ctx_set_damping(c, param.CG_Damping);
        t = trpo_ctx_update(c, 10, 1e-10, 0.01, 10, 0.1, Result, NULL, NULL, NULL, 1);
        if (t < 0) {
            fprintf(stderr, "[ERROR] %s\n", g_err);
            t = -1;
        }
    }
    fflush(stdout);
    pthread_mutex_unlock(&g_lock);
    return t;
}

/* ------------------------------------------------------------------------- */
/* value-baseline objective for L-BFGS (src/TRPO_Baseline.c:29-240)          */
/* ------------------------------------------------------------------------- */
struct trpo_baseline {
    trpo_bdev *dev;
    size_t nl, ls[MAX_LAYERS];
    char ac[MAX_LAYERS + 1];
    size_t np;                 /* weights + biases */
    size_t n;
    size_t num_ep, ep_len;     /* the batch's episode structure (n = num_ep * ep_len) */
    double *gsum;              /* np + 2 */
    double *obs_h, *tgt_h;     /* last uploaded data (drop-in change detection) */
    size_t cap;
};

trpo_baseline *trpo_baseline_create(size_t num_layers, const size_t *layer_size, const char *acfunc, int device) {
    if (check_shape(num_layers, layer_size, acfunc)) return NULL;
    for (size_t i = 1; i < num_layers; ++i)
        if (acfunc[i] != 'l' && acfunc[i] != 't') {   /* evaluate() knows only these (:120-128) */
            set_err("Activation Function for Layer [%zu] is %c. Unsupported.", i, acfunc[i]);
            return NULL;
        }
    if (layer_size[num_layers - 1] != 1) {
        set_err("the baseline predicts one value (LayerSizeBase[last] = 1)");
        return NULL;
    }
    trpo_baseline *b = (trpo_baseline *)calloc(1, sizeof(trpo_baseline));
    if (!b) return NULL;
    b->nl = num_layers;
    memcpy(b->ls, layer_size, num_layers * sizeof(size_t));
    memcpy(b->ac, acfunc, num_layers);
    b->np = NumParamsCalc(b->ls, b->nl) - 1;
    b->gsum = (double *)calloc(b->np + 2, sizeof(double));
    char err[256] = {0};
    b->dev = trpo_bdev_create(device, num_layers, layer_size, acfunc, err, sizeof err);
    if (!b->dev || !b->gsum) {
        set_err("%s", err[0] ? err : "baseline allocation failed");
        trpo_baseline_destroy(b);
        return NULL;
    }
    return b;
}

static trpo_bdev *baseline_bdev(const trpo_baseline *b) { return b->dev; }

const char *trpo_baseline_kernel_name(const trpo_baseline *b) { return b ? trpo_bdev_kernel_name(b->dev) : ""; }

void trpo_baseline_destroy(trpo_baseline *b) {
    if (!b) return;
    trpo_bdev_destroy(b->dev);
    free(b->gsum);
    free(b->obs_h);
    free(b->tgt_h);
    free(b);
}

int trpo_baseline_set_data(trpo_baseline *b, const double *observ, const double *target, size_t num_ep,
                           size_t ep_len) {
    if (!b || !observ || !target || !num_ep || !ep_len) return TRPO_E_INVALID;
    const size_t n = num_ep * ep_len, O = b->ls[0] - 1, L0 = b->ls[0];
    double *x = (double *)malloc(sizeof(double) * n * L0);
    if (!x) return TRPO_E_NOMEM;
    for (size_t s = 0; s < n; ++s) {          /* input = [Obs, currentStep / EpLen] (:96-100) */
        memcpy(x + s * L0, observ + s * O, O * sizeof(double));
        x[s * L0 + O] = (double)(s % ep_len) / (double)ep_len;
    }
    int rc = trpo_bdev_set_data(b->dev, x, target, n);
    free(x);
    if (rc) {
        set_err("baseline data upload failed (code %d)", rc);
        return rc < 0 ? rc : TRPO_E_DEVICE;
    }
    b->n = n;
    b->num_ep = num_ep;
    b->ep_len = ep_len;
    return 0;
}

/* What both advantage entry points do with the device stage's code rc and statistics st: the object's
 * batch, info, the error text; the call's return value (seconds since t0, or the error code). */
static double advantage_done(const char *who, trpo_baseline *b, int rc, const double *st, size_t n, size_t num_ep,
                             size_t ep_len, trpo_adv_info *info, double t0) {
    if (rc != -1 && rc != -7) {               /* the batch was replaced (even when the stage then failed) */
        b->n = rc == 0 || rc == -8 ? n : 0;
        b->num_ep = num_ep;
        b->ep_len = ep_len;
    }
    if (info) {
        info->ep_rew_mean = st[0];
        info->ep_rew_std = st[1];
        info->adv_mean = st[2];
        info->adv_std = st[3];
    }
    if (rc == -7) {
        set_err("%s: a baseline evaluation is still in flight", who);
        return TRPO_E_INVALID;
    }
    if (rc == -8) {
        set_err("%s: the advantages' standard deviation is %g over %zu samples; "
                "they cannot be standardised", who, st[3], n);
        return TRPO_E_INVALID;
    }
    if (rc) {
        set_err("advantage stage failed on the device (code %d)", rc);
        return rc < 0 ? rc : TRPO_E_DEVICE;
    }
    return now_s() - t0;
}

/* Returns, GAE(gamma, lam) advantages and their standardisation on the device (trpo_bdev_advantage). */
double trpo_baseline_advantage(trpo_baseline *b, const double *x, const double *observ, const double *reward,
                               size_t num_ep, size_t ep_len, double gamma, double lam, double *adv_out,
                               double *ret_out, trpo_adv_info *info) {
    if (!b || !x || !observ || !reward || !num_ep || !ep_len) {
        set_err("trpo_baseline_advantage: NULL argument or empty batch");
        return TRPO_E_INVALID;
    }
    const double t0 = now_s();
    const size_t n = num_ep * ep_len;
    double st[4] = {0, 0, 0, 0};
    /* the device adds the time feature to the rows (trpo_baseline_set_data's input rows) */
    const int rc = trpo_bdev_advantage(b->dev, x, observ, reward, num_ep, ep_len, gamma, lam, adv_out, ret_out, st);
    return advantage_done("trpo_baseline_advantage", b, rc, st, n, num_ep, ep_len, info, t0);
}

/* The sample count of a ragged batch: num_ep episodes of ep_len[e] >= 1 steps, none longer than horizon,
 * at most INT_MAX samples in all.  0 with the cause in trpo_last_error() otherwise. */
static size_t ragged_samples(const char *who, size_t num_ep, const size_t *ep_len, size_t horizon) {
    if (!num_ep || !ep_len) {
        set_err("%s: NULL ep_len or no episode", who);
        return 0;
    }
    size_t n = 0;
    for (size_t e = 0; e < num_ep; ++e) {
        if (!ep_len[e]) {
            set_err("%s: ep_len[%zu] is 0 (every episode has at least one step)", who, e);
            return 0;
        }
        if (ep_len[e] > horizon) {
            set_err("%s: ep_len[%zu] = %zu exceeds horizon = %zu", who, e, ep_len[e], horizon);
            return 0;
        }
        if (ep_len[e] > (size_t)0x7fffffff - n) {
            set_err("%s: more than %d samples", who, 0x7fffffff);
            return 0;
        }
        n += ep_len[e];
    }
    return n;
}

int trpo_baseline_set_data_ragged(trpo_baseline *b, const double *observ, const double *target, size_t num_ep,
                                  const size_t *ep_len, size_t horizon) {
    /* the lengths first: their check needs no object (and so no device) */
    const size_t n = ragged_samples("trpo_baseline_set_data_ragged", num_ep, ep_len, horizon);
    if (!n) return TRPO_E_INVALID;
    if (!b || !observ || !target) {
        set_err("trpo_baseline_set_data_ragged: NULL argument");
        return TRPO_E_INVALID;
    }
    const size_t O = b->ls[0] - 1, L0 = b->ls[0];
    double *x = (double *)malloc(sizeof(double) * n * L0);
    if (!x) return TRPO_E_NOMEM;
    size_t s = 0;
    for (size_t e = 0; e < num_ep; ++e)
        for (size_t t = 0; t < ep_len[e]; ++t, ++s) {  /* input = [Obs, step / horizon] */
            memcpy(x + s * L0, observ + s * O, O * sizeof(double));
            x[s * L0 + O] = (double)t / (double)horizon;
        }
    int rc = trpo_bdev_set_data(b->dev, x, target, n);
    free(x);
    if (rc) {
        set_err("baseline data upload failed (code %d)", rc);
        return rc < 0 ? rc : TRPO_E_DEVICE;
    }
    b->n = n;
    b->num_ep = num_ep;
    b->ep_len = 0;
    return 0;
}

/* trpo_baseline_advantage for episodes of their own lengths, truncated ones bootstrapped
 * (trpo_bdev_advantage_ragged). */
double trpo_baseline_advantage_ragged(trpo_baseline *b, const double *x, const double *observ, const double *reward,
                                      size_t num_ep, const size_t *ep_len, size_t horizon, const double *boot_observ,
                                      const unsigned char *boot, double gamma, double lam, double *adv_out,
                                      double *ret_out, trpo_adv_info *info) {
    const size_t n = ragged_samples("trpo_baseline_advantage_ragged", num_ep, ep_len, horizon);
    if (!n) return TRPO_E_INVALID;
    if (!b || !x || !observ || !reward) {
        set_err("trpo_baseline_advantage_ragged: NULL argument");
        return TRPO_E_INVALID;
    }
    if (boot && !boot_observ) {
        set_err("trpo_baseline_advantage_ragged: boot is set and boot_observ is NULL");
        return TRPO_E_INVALID;
    }
    const double t0 = now_s();
    double st[4] = {0, 0, 0, 0};
    const int rc = trpo_bdev_advantage_ragged(b->dev, x, observ, reward, num_ep, ep_len, n, horizon, boot_observ, boot,
                                              gamma, lam, adv_out, ret_out, st);
    return advantage_done("trpo_baseline_advantage_ragged", b, rc, st, n, num_ep, 0, info, t0);
}

/* advantage_done for the stages that take a context: rc == -1 is a refusal with its cause in err, and leaves b
 * and info as they were */
static double advantage_ctx_done(const char *who, trpo_baseline *b, int rc, const double *st, const char *err, size_t n,
                                 size_t num_ep, size_t ep_len, trpo_adv_info *info, double t0) {
    if (rc == -1) {
        set_err("%s: %s", who, err[0] ? err : "the batch is beyond the device kernels' indexing");
        return TRPO_E_INVALID;
    }
    return advantage_done(who, b, rc, st, n, num_ep, ep_len, info, t0);
}

/* Both stages with the observations read on the device from the context's batch (trpo_bdev_advantage_dev);
 * ep_len_ragged == NULL: the fixed form. */
static double advantage_ctx(const char *who, trpo_baseline *b, const double *x, const trpo_ctx *c, const double *reward,
                            size_t num_ep, size_t ep_len, const size_t *ep_len_ragged, size_t n, size_t horizon,
                            const double *boot_observ, const unsigned char *boot, double gamma, double lam,
                            double *adv_out, double *ret_out, trpo_adv_info *info) {
    const double t0 = now_s();
    double st[4] = {0, 0, 0, 0};
    char err[256] = {0};
    const int rc = trpo_bdev_advantage_dev(b->dev, x, c->dev, reward, num_ep, ep_len, ep_len_ragged, n, horizon,
                                           boot_observ, boot, gamma, lam, adv_out, ret_out, st, err, sizeof err);
    return advantage_ctx_done(who, b, rc, st, err, n, num_ep, ep_len, info, t0);
}

double trpo_baseline_advantage_ctx(trpo_baseline *b, const double *x, const trpo_ctx *ctx, const double *reward,
                                   size_t num_ep, size_t ep_len, double gamma, double lam, double *adv_out,
                                   double *ret_out, trpo_adv_info *info) {
    if (!b || !x || !ctx || !reward || !num_ep || !ep_len || num_ep > (size_t)0x7fffffff / ep_len) {
        set_err("trpo_baseline_advantage_ctx: NULL argument, empty batch or more than %d samples", 0x7fffffff);
        return TRPO_E_INVALID;
    }
    return advantage_ctx("trpo_baseline_advantage_ctx", b, x, ctx, reward, num_ep, ep_len, NULL, num_ep * ep_len, 0,
                         NULL, NULL, gamma, lam, adv_out, ret_out, info);
}

double trpo_baseline_advantage_ragged_ctx(trpo_baseline *b, const double *x, const trpo_ctx *ctx, const double *reward,
                                          size_t num_ep, const size_t *ep_len, size_t horizon,
                                          const double *boot_observ, const unsigned char *boot, double gamma,
                                          double lam, double *adv_out, double *ret_out, trpo_adv_info *info) {
    const char *who = "trpo_baseline_advantage_ragged_ctx";
    if (!b || !x || !ctx || !reward) {        /* the objects first: the NULL refusals need no lengths */
        set_err("%s: NULL argument", who);
        return TRPO_E_INVALID;
    }
    const size_t n = ragged_samples(who, num_ep, ep_len, horizon);
    if (!n) return TRPO_E_INVALID;
    if (boot && !boot_observ) {
        set_err("%s: boot is set and boot_observ is NULL", who);
        return TRPO_E_INVALID;
    }
    return advantage_ctx(who, b, x, ctx, reward, num_ep, 0, ep_len, n, horizon, boot_observ, boot, gamma, lam, adv_out,
                         ret_out, info);
}

/* Both stages again with the rewards (and the ragged form's last observations) in device memory
 * (trpo_bdev_advantage_dev_rewards); slot_rows == 0: the fixed form. */
static double advantage_ctx_dev(const char *who, trpo_baseline *b, const double *x, const trpo_ctx *c,
                                const void *reward, const void *last_obs, int dtype, size_t slot_rows, void *stream,
                                size_t num_ep, size_t ep_len, const size_t *ep_len_ragged, size_t n, size_t horizon,
                                const unsigned char *boot, double gamma, double lam, double *adv_out, double *ret_out,
                                trpo_adv_info *info) {
    const double t0 = now_s();
    double st[4] = {0, 0, 0, 0};
    char err[256] = {0};
    const int rc = trpo_bdev_advantage_dev_rewards(b->dev, x, c->dev, reward, last_obs, dtype, slot_rows, stream, num_ep,
                                                   ep_len, ep_len_ragged, n, horizon, boot, gamma, lam, adv_out,
                                                   ret_out, st, err, sizeof err);
    return advantage_ctx_done(who, b, rc, st, err, n, num_ep, ep_len, info, t0);
}

double trpo_baseline_advantage_ctx_dev(trpo_baseline *b, const double *x, const trpo_ctx *ctx, const void *reward_dev,
                                       int dtype, size_t num_ep, size_t ep_len, double gamma, double lam,
                                       void *hip_stream, double *adv_out, double *ret_out, trpo_adv_info *info) {
    const char *who = "trpo_baseline_advantage_ctx_dev";
    if (!b || !x || !ctx || !reward_dev || !num_ep || !ep_len || num_ep > (size_t)0x7fffffff / ep_len) {
        set_err("%s: NULL argument, empty batch or more than %d samples", who, 0x7fffffff);
        return TRPO_E_INVALID;
    }
    if (dtype != TRPO_DT_F64 && dtype != TRPO_DT_F32) {
        set_err("%s: dtype must be TRPO_DT_F64 or TRPO_DT_F32", who);
        return TRPO_E_INVALID;
    }
    return advantage_ctx_dev(who, b, x, ctx, reward_dev, NULL, dtype, 0, hip_stream, num_ep, ep_len, NULL,
                             num_ep * ep_len, 0, NULL, gamma, lam, adv_out, ret_out, info);
}

double trpo_baseline_advantage_ragged_ctx_dev(trpo_baseline *b, const double *x, const trpo_ctx *ctx,
                                              const void *reward_slots_dev, const void *last_obs_dev, int dtype,
                                              size_t num_ep, const size_t *ep_len, size_t slot_rows, size_t horizon,
                                              const unsigned char *boot, double gamma, double lam, void *hip_stream,
                                              double *adv_out, double *ret_out, trpo_adv_info *info) {
    const char *who = "trpo_baseline_advantage_ragged_ctx_dev";
    if (!b || !x || !ctx || !reward_slots_dev) {      /* the objects first: the NULL refusals need no lengths */
        set_err("%s: NULL argument", who);
        return TRPO_E_INVALID;
    }
    if (dtype != TRPO_DT_F64 && dtype != TRPO_DT_F32) {
        set_err("%s: dtype must be TRPO_DT_F64 or TRPO_DT_F32", who);
        return TRPO_E_INVALID;
    }
    const size_t n = ragged_samples(who, num_ep, ep_len, horizon);
    if (!n) return TRPO_E_INVALID;
    for (size_t e = 0; e < num_ep; ++e)
        if (ep_len[e] > slot_rows) {
            set_err("%s: ep_len[%zu] = %zu exceeds slot_rows = %zu", who, e, ep_len[e], slot_rows);
            return TRPO_E_INVALID;
        }
    if (slot_rows > (size_t)0x7fffffff / num_ep) {
        set_err("%s: num_ep * slot_rows exceeds %d", who, 0x7fffffff);
        return TRPO_E_INVALID;
    }
    if (boot && !last_obs_dev) {
        set_err("%s: boot is set and last_obs_dev is NULL", who);
        return TRPO_E_INVALID;
    }
    return advantage_ctx_dev(who, b, x, ctx, reward_slots_dev, last_obs_dev, dtype, slot_rows, hip_stream, num_ep, 0,
                             ep_len, n, horizon, boot, gamma, lam, adv_out, ret_out, info);
}

/* the objective and gradient from the device's sums in b->gsum */
static double baseline_finish(const trpo_baseline *b, const double *x, double *g, int n) {
    /* gradient (:210-224): sum / N + 0.002 * parameter; zero on the L-BFGS padding */
    const double N = (double)b->n;
    for (size_t q = 0; q < b->np; ++q) g[q] = b->gsum[q] / N + 0.002 * x[q];
    for (int q = (int)b->np; q < n; ++q) g[q] = 0;
    /* objective (:227-240): 0.01 * mean squared error + 0.001 * |x|^2 over the real parameters */
    const double mse = 0.01 * b->gsum[b->np] / N;
    double l2 = 0;
    for (size_t q = 0; q < b->np; ++q) l2 += x[q] * x[q];
    return mse + 0.001 * l2;
}

double trpo_baseline_evaluate(trpo_baseline *b, const double *x, double *g, int n, double *predict) {
    if (!b || !x || !g || n < (int)b->np || !b->n) return TRPO_E_INVALID;
    int rc = trpo_bdev_eval(b->dev, x, b->gsum, predict);
    if (rc) {
        set_err("baseline evaluation failed on the device (code %d)", rc);
        return rc < 0 ? rc : TRPO_E_DEVICE;
    }
    return baseline_finish(b, x, g, n);
}

/* H v of the trust-region fit (trpo_bdev_gnvp): the Gauss-Newton matrix of the baseline at x plus damping. */
double trpo_baseline_gnvp(trpo_baseline *b, const double *x, const double *v, int n, double damping, double *out) {
    if (!b || !x || !v || !out) {
        set_err("trpo_baseline_gnvp: NULL argument");
        return TRPO_E_INVALID;
    }
    if (n < (int)b->np || !b->n || !(damping >= 0)) {
        set_err("trpo_baseline_gnvp: n = %d below NumParams = %zu, no data, or damping = %g", n, b->np, damping);
        return TRPO_E_INVALID;
    }
    const double t0 = now_s();
    const int rc = trpo_bdev_gnvp(b->dev, x, v, damping, out);
    if (rc) {
        set_err(rc == -7 ? "trpo_baseline_gnvp: a baseline evaluation is still in flight"
                         : "Gauss-Newton product failed on the device (code %d)", rc);
        return rc == -7 || rc == -1 ? TRPO_E_INVALID : (rc < 0 ? rc : TRPO_E_DEVICE);
    }
    for (int q = (int)b->np; q < n; ++q) out[q] = 0;
    return now_s() - t0;
}

/* The device-resident fit: product -> CG -> rescale onto the trust region -> candidate search
 * (trpo_bdev_fit_tr; the math stands in include/trpo_mi355x.h). */
double trpo_baseline_fit_tr(trpo_baseline *b, const double *x, int n, double eps, size_t cg_max_iter,
                            double cg_residual_th, double damping, int max_backtracks, double shift_cap,
                            double *x_out, double *step_out, trpo_vfit_info *info) {
    if (!b || !x || !x_out) {
        set_err("trpo_baseline_fit_tr: NULL baseline, x or x_out");
        return TRPO_E_INVALID;
    }
    if (n < (int)b->np || !b->n) {
        set_err("trpo_baseline_fit_tr: n = %d below NumParams = %zu, or the baseline holds no data", n, b->np);
        return TRPO_E_INVALID;
    }
    if (!(eps > 0) || !(damping >= 0) || !(shift_cap > 0) || cg_max_iter < 1 || cg_max_iter > TRPO_VFIT_MAX_CG ||
        max_backtracks < 1 || max_backtracks > TRPO_MAX_BACKTRACKS) {
        set_err("trpo_baseline_fit_tr: eps = %g, damping = %g, shift_cap = %g, cg_max_iter = %zu or "
                "max_backtracks = %d out of range", eps, damping, shift_cap, cg_max_iter, max_backtracks);
        return TRPO_E_INVALID;
    }
    const double t0 = now_s();
    double raw[TRPO_BDEV_VFIT_INFO];
    memset(raw, 0, sizeof raw);
    const int rc = trpo_bdev_fit_tr(b->dev, x, eps, cg_max_iter, cg_residual_th, damping, max_backtracks, shift_cap,
                                    x_out, step_out, raw);
    if (rc && rc != -8) {
        set_err(rc == -7 ? "trpo_baseline_fit_tr: a baseline evaluation is still in flight"
                         : "trust-region fit failed on the device (code %d)", rc);
        return rc == -7 || rc == -1 ? TRPO_E_INVALID : (rc < 0 ? rc : TRPO_E_DEVICE);
    }
    for (int q = (int)b->np; q < n; ++q) {
        x_out[q] = 0;
        if (step_out) step_out[q] = 0;
    }
    if (info) {
        memset(info, 0, sizeof *info);
        info->loss_before = raw[0];
        info->gnorm = raw[1];
        info->shs = raw[2];
        info->alpha_tr = raw[3];
        info->alpha0 = raw[4];
        info->cg_iters = (size_t)raw[5];
        info->accepted = rc ? -1 : (int)raw[6];
        info->evaluated = rc ? 0 : max_backtracks;     /* one pass evaluates every candidate */
        memcpy(info->loss, raw + 8, sizeof info->loss);
        memcpy(info->shift, raw + 40, sizeof info->shift);
        memcpy(info->rdotr, raw + 72, sizeof info->rdotr);
    }
    if (rc) {
        set_err("trpo_baseline_fit_tr: the loss at x is %g over %zu samples; there is no trust region to scale to",
                raw[0], b->n);
        return TRPO_E_INVALID;
    }
    return now_s() - t0;
}

/* The drop-in for src/TRPO_Baseline.c:29 (liblbfgs callback).  One cached device context per
 * network shape; the sample data is re-uploaded only when its contents change (compared with
 * the last upload), so the ~25 callbacks of one lbfgs() fit upload once. */
static trpo_baseline *g_base;

double evaluate(void *instance, const double *x, double *g, const int n, const double step) {
    (void)step;
    TRPOBaselineParam *p = (TRPOBaselineParam *)instance;
    if (!p || !x || !g || !p->LayerSizeBase || !p->AcFunc || !p->Observ || !p->Target) return -1;
    if (p->NumLayers < 2 || p->LayerSizeBase[0] != p->ObservSpaceDim + 1 ||
        p->NumSamples != p->NumEpBatch * p->EpLen) {
        fprintf(stderr, "[ERROR] inconsistent TRPOBaselineParam (LayerSizeBase[0] = ObservSpaceDim + 1, "
                        "NumSamples = NumEpBatch * EpLen)\n");
        return -1;
    }
    for (size_t i = 1; i < p->NumLayers; ++i)
        if (p->AcFunc[i] != 'l' && p->AcFunc[i] != 't') {
            printf("[ERROR] Activation Function for Layer [%zu] is %c. Unsupported.\n", i, p->AcFunc[i]);
            return -1;
        }
    pthread_mutex_lock(&g_lock);
    double f = -1;
    trpo_baseline *b = g_base;
    if (b && (b->nl != p->NumLayers || memcmp(b->ls, p->LayerSizeBase, p->NumLayers * sizeof(size_t)) ||
              memcmp(b->ac, p->AcFunc, p->NumLayers))) {
        trpo_baseline_destroy(b);
        b = g_base = NULL;
    }
    if (!b) b = g_base = trpo_baseline_create(p->NumLayers, p->LayerSizeBase, p->AcFunc, -1);
    if (b) {
        const size_t N = p->NumSamples, O = p->ObservSpaceDim;
        int rc = 0;
        /* with data already uploaded for this N, the device evaluates on it while the host compares the
         * caller's arrays with that upload (the comparison, ~5 us at 20 x 150, leaves the critical path);
         * if they differ, that result is dropped and the evaluation runs again on the new data */
        const int have = b->n == N && b->cap >= N && b->obs_h && n >= (int)b->np;
        const int started = have && trpo_bdev_eval_start(b->dev, x, p->Predict != NULL) == 0;
        const int same = have && !memcmp(b->obs_h, p->Observ, N * O * sizeof(double)) &&
                         !memcmp(b->tgt_h, p->Target, N * sizeof(double));
        if (started) {
            rc = trpo_bdev_eval_finish(b->dev, b->gsum, p->Predict);
            if (rc) set_err("baseline evaluation failed on the device (code %d)", rc);
            else if (same) f = baseline_finish(b, x, g, n);
        } else if (same) {
            f = trpo_baseline_evaluate(b, x, g, n, p->Predict);   /* the start was refused: its error */
        }
        if (!same && !rc) {
            rc = trpo_baseline_set_data(b, p->Observ, p->Target, p->NumEpBatch, p->EpLen);
            if (!rc && N > b->cap) {
                free(b->obs_h);
                free(b->tgt_h);
                b->obs_h = (double *)malloc(sizeof(double) * N * O + 1);
                b->tgt_h = (double *)malloc(sizeof(double) * N + 1);
                b->cap = (b->obs_h && b->tgt_h) ? N : 0;
            }
            if (!rc && b->cap >= N) {
                memcpy(b->obs_h, p->Observ, N * O * sizeof(double));
                memcpy(b->tgt_h, p->Target, N * sizeof(double));
            }
            if (!rc) f = trpo_baseline_evaluate(b, x, g, n, p->Predict);
        }
        /* the reference leaves W/B = x in the param's arrays (:64-81) */
        if (f >= 0 && p->WBase && p->BBase) {
            size_t pos = 0;
            for (size_t i = 0; i + 1 < p->NumLayers; ++i) {
                const size_t cur = p->LayerSizeBase[i], nxt = p->LayerSizeBase[i + 1];
                if (p->WBase[i]) memcpy(p->WBase[i], x + pos, cur * nxt * sizeof(double));
                pos += cur * nxt;
                if (p->BBase[i]) memcpy(p->BBase[i], x + pos, nxt * sizeof(double));
                pos += nxt;
            }
        }
        if (f < 0) fprintf(stderr, "[ERROR] %s\n", g_err);
    } else {
        fprintf(stderr, "[ERROR] %s\n", g_err);
    }
    pthread_mutex_unlock(&g_lock);
    return f;
}
