// Section of trpo_kernels.hip, included once behind dev_xfer.h: the collective backends (in-process group,
// RCCL, peer windows), allreduce() and the global sample count.
// Relies on, from trpo_kernels.hip above the include: struct trpo_dev, has_collective, choose_replicas,
// sync_ctl_scalars; from dev_xfer.h: ensure_hst, vcopy64_kernel; from trpo_common.h: HCHK, cdiv, trpo_malloc,
// TRPO_HOST_COHERENT, PEER_WMAX and the trpo_peer_* interface; from trpo_dev.h: DSYNC and the entry points'
// declarations.
//
// ---------------------------------------------------------------------------
// In-process host-staged all-reduce (trpo_dev_set_group).  The contexts of one process -- one
// thread per context, on any devices -- exchange their partial sums through host memory: every rank
// copies its buffer in, waits for all ranks, sums the slots in rank order (so every rank gets the
// same bits, as RCCL's all-reduce guarantees) and copies the sum back.  It exists to run the
// library's sharded code path (global N, replica sizing from the largest shard, lockstep CG) on a
// single GPU in tests; the collective is a host round trip, so CG runs eagerly under it.
// ---------------------------------------------------------------------------
struct trpo_hgroup {
    int world;
    pthread_barrier_t bar;
    pthread_mutex_t mu;
    double **slot;              // per-rank host views of the buffers being reduced
    size_t *count;
    int *attached;
};

extern "C" trpo_hgroup *trpo_hgroup_create(int world) {
    if (world < 1 || world > 1024) return NULL;
    trpo_hgroup *g = (trpo_hgroup *)calloc(1, sizeof(trpo_hgroup));
    if (!g) return NULL;
    g->world = world;
    g->slot = (double **)calloc(world, sizeof(double *));
    g->count = (size_t *)calloc(world, sizeof(size_t));
    g->attached = (int *)calloc(world, sizeof(int));
    if (!g->slot || !g->count || !g->attached || pthread_barrier_init(&g->bar, NULL, (unsigned)world) ||
        pthread_mutex_init(&g->mu, NULL)) {
        free(g->slot);
        free(g->count);
        free(g->attached);
        free(g);
        return NULL;
    }
    return g;
}

extern "C" void trpo_hgroup_destroy(trpo_hgroup *g) {
    if (!g) return;
    pthread_barrier_destroy(&g->bar);
    pthread_mutex_destroy(&g->mu);
    free(g->slot);
    free(g->count);
    free(g->attached);
    free(g);
}

// in-place sum of buf[count] (device, on d's stream) over the group; every rank must call it with
// the same count, in the same order as the others (the library's fixed launch sequences do)
static int hgroup_allreduce(trpo_dev *d, double *buf, size_t count) {
    trpo_hgroup *g = d->group;
    // a local failure before the exchange still takes part in both barriers (a rank that returned
    // early would leave the others waiting forever): it publishes count (size_t)-1, which every rank
    // reads as a mismatch, so all of them return -4 together
    bool ok = true;
    if (count > d->gbuf_cap) {
        if (d->gbuf) hipHostFree(d->gbuf);
        d->gbuf = NULL;
        d->gbuf_cap = 0;
        ok = hipHostMalloc((void **)&d->gbuf, sizeof(double) * count, TRPO_HOST_COHERENT) == hipSuccess &&
             hipHostGetDevicePointer((void **)&d->gbuf_dev, d->gbuf, 0) == hipSuccess;
        if (ok) d->gbuf_cap = count;
    }
    // copies by KERNEL through the mapped buffer, not hipMemcpyAsync: a host-to-device hipMemcpyAsync
    // into buf followed by kernels reading buf gave intermittently stale reads (ranks diverging in
    // whole 512-element cg_axpy slices, 6 of 10 sharded 2x64 solves; tools/diag/shard_race.py)
    if (ok) hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv((long)count, 256)), dim3(256), 0, d->stream,
                               (const double *)buf, d->gbuf_dev, (int)count);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = ok && hipStreamSynchronize(d->stream) == hipSuccess;
    g->slot[d->rank] = ok ? d->gbuf : NULL;
    g->count[d->rank] = ok ? count : (size_t)-1;
    pthread_barrier_wait(&g->bar);                 // every rank's partial (or failure) is published
    int bad = 0;
    for (int r = 0; r < g->world; ++r) bad |= g->count[r] != count;
    double *sum = bad ? NULL : (double *)malloc(sizeof(double) * (count ? count : 1));
    if (sum) {
        for (size_t i = 0; i < count; ++i) {
            double s = g->slot[0][i];
            for (int r = 1; r < g->world; ++r) s += g->slot[r][i];   // rank order: identical bits everywhere
            sum[i] = s;
        }
    }
    pthread_barrier_wait(&g->bar);                 // every rank has read every slot
    if (!sum) return -4;
    memcpy(d->gbuf, sum, sizeof(double) * count);
    free(sum);
    hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv((long)count, 256)), dim3(256), 0, d->stream,
                       (const double *)d->gbuf_dev, buf, (int)count);
    HCHK(hipGetLastError());
    DSYNC(d);
    return 0;
}

// the one place every collective of the library goes through: RCCL, the in-process host group, or
// nothing (one rank)
static int allreduce(trpo_dev *d, double *buf, size_t count) {
    if (d->peer_on) {
        // in place through the staging vector (the exchange kernel's output must not alias its input)
        if (count > trpo_peer_slot(d->peer)) return -1;
        // a copy kernel (stream-ordered like the exchange that follows)
        hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv((long)count, 256)), dim3(256), 0, d->stream, (const double *)buf,
                           d->ptmp, (int)count);
        HCHK(hipGetLastError());
        return trpo_peer_allreduce(d->peer, d->stream, d->ptmp, 1, 0, (int)count, buf, nullptr);
    }
    if (d->group) return hgroup_allreduce(d, buf, count);
    if (!d->comm) return 0;
    return ncclAllReduce(buf, buf, count, ncclFloat64, ncclSum, d->comm, d->stream) == ncclSuccess ? 0 : -4;
}

// N is the global sample count: local n, or the all-reduced n under RCCL
static int refresh_n_total(trpo_dev *d) {
    const size_t n = d->n;
    if (has_collective(d)) {
        // every rank's shard size in one sum-all-reduce (rank r contributes n at slot r): N is the
        // total, and the replica sizing below reads the LARGEST shard -- both identical on all ranks
        const int W = d->world;
        double *hn = (double *)calloc(W, sizeof(double)), *dn = d->peer_on ? d->pn : NULL;
        if (!hn) return -3;
        hn[d->rank] = (double)n;
        // the peer exchange uses a buffer allocated with its window: no allocation (which may wait for
        // the whole device) while another context of this process already spins in its exchange
        if (!dn && trpo_malloc((void **)&dn, sizeof(double) * W) != hipSuccess) {
            free(hn);
            return -2;
        }
        int rc = hipMemcpyAsync(dn, hn, sizeof(double) * W, hipMemcpyHostToDevice, d->stream) ? -2 : 0;
        if (!rc) rc = allreduce(d, dn, (size_t)W);
        if (!rc && hipMemcpyAsync(hn, dn, sizeof(double) * W, hipMemcpyDeviceToHost, d->stream)) rc = -2;
        if (!rc && hipStreamSynchronize(d->stream)) rc = -2;
        if (dn != d->pn) hipFree(dn);
        if (!rc) {
            double tot = 0.0, mx = 0.0;
            for (int r = 0; r < W; ++r) {
                tot += hn[r];
                mx = hn[r] > mx ? hn[r] : mx;
            }
            d->n_total = tot;
            d->n_max = mx;
        }
        free(hn);
        if (rc) return rc;
    } else {
        d->n_total = (double)n;
        d->n_max = (double)n;
    }
    if (choose_replicas(d)) return -2;
    return sync_ctl_scalars(d);
}

extern "C" int trpo_dev_comm_unique_id(void *id128) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -4;
    memcpy(id128, &id, sizeof(id) < 128 ? sizeof(id) : 128);
    return 0;
}

extern "C" int trpo_dev_set_group(trpo_dev *d, trpo_hgroup *g, int rank) {
    if (!d || !g || rank < 0 || rank >= g->world) return -1;
    HCHK(hipSetDevice(d->device));
    if (d->comm) {
        ncclCommDestroy(d->comm);
        d->comm = NULL;
    }
    pthread_mutex_lock(&g->mu);
    const int taken = g->attached[rank];
    g->attached[rank] = 1;
    pthread_mutex_unlock(&g->mu);
    if (taken) return -1;
    d->peer_on = 0;
    d->group = g;
    d->rank = rank;
    d->world = g->world;
    cg_graph_drop(d);               // the host exchange cannot live in a graph: CG runs eagerly
    return refresh_n_total(d);
}

// ranks of the attached communicator as the collective library itself reports them (RCCL's
// ncclCommCount), the context's rank, and the atomic replica sets in use
extern "C" int trpo_dev_comm_info(const trpo_dev *d, int *rank, int *world, int *replicas) {
    if (!d) return -1;
    int w = d->world;
    if (d->comm) {
        int c = 0;
        if (ncclCommCount(d->comm, &c) != ncclSuccess) return -4;
        w = c;
    }
    if (rank) *rank = d->rank;
    if (world) *world = w;
    if (replicas) *replicas = d->atomic ? d->Rc : 0;
    return 0;
}

// Bounded RCCL initialisation.  ncclCommInitRank blocks until every rank of the unique id has joined;
// a rank that never arrives (crashed, or failed before the call) would hold the others forever.  The
// call therefore runs in a helper thread and the caller waits at most timeout_ms: on time-out the
// attach fails (-6) and the helper is abandoned -- if its init completes later, it aborts the
// communicator itself.  The communicator stays a BLOCKING one, so the data path (eager and
// graph-captured ncclAllReduce) is exactly that of an ordinary ncclCommInitRank.
struct CommInitJob {
    pthread_mutex_t mu;
    int device, world, rank;
    ncclUniqueId id;
    ncclComm_t comm;
    ncclResult_t res;
    int done, abandoned;
};

static void *comm_init_thread(void *arg) {
    CommInitJob *j = (CommInitJob *)arg;
    ncclComm_t c = NULL;
    ncclResult_t r = hipSetDevice(j->device) == hipSuccess ? ncclCommInitRank(&c, j->world, j->id, j->rank)
                                                             : ncclUnhandledCudaError;
    pthread_mutex_lock(&j->mu);
    j->comm = c;
    j->res = r;
    j->done = 1;
    const int abandoned = j->abandoned;
    pthread_mutex_unlock(&j->mu);
    if (abandoned) {
        if (r == ncclSuccess && c) ncclCommAbort(c);
        pthread_mutex_destroy(&j->mu);
        free(j);
    }
    return NULL;
}

static double mono_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec;
}

static long comm_timeout_ms(long given) {
    if (given > 0) return given;
    const char *e = getenv("TRPO_COMM_TIMEOUT_MS");
    return e && atol(e) > 0 ? atol(e) : 120000;
}

static int comm_init_bounded(trpo_dev *d, int rank, int world, const void *id128, long timeout_ms) {
    CommInitJob *j = (CommInitJob *)calloc(1, sizeof(CommInitJob));
    if (!j) return -3;
    pthread_mutex_init(&j->mu, NULL);
    j->device = d->device;
    j->world = world;
    j->rank = rank;
    memcpy(&j->id, id128, sizeof(j->id));
    pthread_t th;
    if (pthread_create(&th, NULL, comm_init_thread, j) != 0) {
        pthread_mutex_destroy(&j->mu);
        free(j);
        return -3;
    }
    pthread_detach(th);
    const double t_end = mono_ms() + (double)timeout_ms;
    for (;;) {
        pthread_mutex_lock(&j->mu);
        const int done = j->done;
        if (!done && mono_ms() > t_end) j->abandoned = 1;       // the helper frees the job
        const int abandoned = j->abandoned;
        pthread_mutex_unlock(&j->mu);
        if (done) break;
        if (abandoned) {
            fprintf(stderr, "[trpo_mi355x] ncclCommInitRank(rank %d of %d, device %d): no completion within %ld ms\n",
                    rank, world, d->device, timeout_ms);
            return -6;
        }
        struct timespec ts = {0, 1000000};
        nanosleep(&ts, NULL);
    }
    const ncclResult_t nr = j->res;
    ncclComm_t c = j->comm;
    pthread_mutex_destroy(&j->mu);
    free(j);
    if (nr != ncclSuccess) {
        fprintf(stderr, "[trpo_mi355x] ncclCommInitRank(rank %d of %d, device %d): %s\n", rank, world, d->device,
                ncclGetErrorString(nr));
        return -4;
    }
    d->comm = c;
    return 0;
}

extern "C" int trpo_dev_set_comm(trpo_dev *d, int rank, int world, const void *id128, long timeout_ms) {
    if (!d || world < 1 || rank < 0 || rank >= world || (world > 1 && !id128)) return -1;
    HCHK(hipSetDevice(d->device));
    d->group = NULL;
    d->peer_on = 0;
    d->comm_aborted = 0;
    if (d->comm) {
        ncclCommDestroy(d->comm);
        d->comm = NULL;
    }
    if (world > 1) {
        const int rc = comm_init_bounded(d, rank, world, id128, comm_timeout_ms(timeout_ms));
        if (rc) return rc;
    }
    d->rank = rank;
    d->world = world;
    cg_graph_drop(d);
    return refresh_n_total(d);
}

// Wait for everything enqueued on the context's stream, at most timeout_ms (<= 0: the default of
// TRPO_COMM_TIMEOUT_MS / 120 s): 0 when it completed (or the collective's error), -6 on time-out.
// spin: poll without sleeping for the first WAIT_SPIN_MS (a timed region's closing wait must not add a
// sleep quantum), then 50 us between polls, so a slow or hung collective does not hold a host core at
// 100 % for the whole bound; otherwise 50 us between polls from the start.
#define WAIT_SPIN_MS 250.0
static int wait_stream(trpo_dev *d, long timeout_ms, bool spin) {
    const double t0 = mono_ms();
    const double t_end = t0 + (double)comm_timeout_ms(timeout_ms);
    for (;;) {
        const hipError_t e = hipStreamQuery(d->stream);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) {
            fprintf(stderr, "[trpo_mi355x] HIP error %s while waiting for the stream\n", hipGetErrorString(e));
            return -2;
        }
        const double now = mono_ms();
        if (now > t_end) return -6;
        if (!spin || now - t0 > WAIT_SPIN_MS) {
            struct timespec ts = {0, 50000};
            nanosleep(&ts, NULL);
        }
    }
}

// The host's wait at the end of a synchronous call (update, FVP, surrogate, ...): a plain stream
// synchronisation on one rank; with a collective attached a peer that never arrives must not hang the
// caller, so the wait is bounded (TRPO_COMM_TIMEOUT_MS / 120 s) and reports -6 / the collective's error.
int trpo_dev_has_collective(const trpo_dev *d) { return has_collective(d) ? 1 : 0; }

extern "C" int trpo_dev_wait_done(trpo_dev *d) {
    if (!has_collective(d)) return hipStreamSynchronize(d->stream) == hipSuccess ? 0 : -2;
    const int rc = wait_stream(d, 0, true);
    return rc ? rc : trpo_dev_comm_error(d);
}

extern "C" int trpo_dev_wait(trpo_dev *d, long timeout_ms) {
    if (!d) return -1;
    HCHK(hipSetDevice(d->device));
    const int rc = wait_stream(d, timeout_ms, true);
    return rc ? rc : trpo_dev_comm_error(d);
}

// Give up on the attached collective: RCCL's abort (its kernels, eager or inside a captured graph, see
// the abort flag and exit), or the peer exchange's error word (later exchanges skip their waits); the
// CG graph holding the old collective is dropped, the stream drained (bounded), and every later result
// call of this context reports -4.  The context is then only good for trpo_ctx_destroy.
extern "C" int trpo_dev_comm_abort(trpo_dev *d) {
    if (!d) return -1;
    hipSetDevice(d->device);
    if (d->comm) {
        ncclCommAbort(d->comm);
        d->comm = NULL;
    }
    if (d->peer) trpo_peer_set_error(d->peer);
    d->comm_aborted = 1;
    const int rc = wait_stream(d, 10000, false);
    cg_graph_drop(d);
    return rc;
}

// Self-check of the attached collective before it carries results: ONE eager all-reduce, through the
// same allreduce() every FVP uses, of a vector as long as the per-FVP message (Rc x Ps replica values
// in the atomic mode, the reduced vector otherwise).  Rank r contributes 2^r (1 + i mod 251) at
// element i, so the sum is (2^world - 1)(1 + i mod 251) exactly, and a lost, doubled or misplaced
// contribution changes it.  The wait is bounded (timeout_ms); every element is compared bit for bit.
// Returns 0, -6 (no completion: the caller aborts), -7 (wrong sum; *bad = mismatching elements) or the
// collective's error.  TRPO_COMM_FAULT=verify:R / hang:R (testing) makes rank R contribute a wrong
// value / skip the all-reduce.
static int comm_fault(const trpo_dev *d, const char *kind) {
    const char *e = getenv("TRPO_COMM_FAULT");
    const size_t k = strlen(kind);
    const int hit = e && !strncmp(e, kind, k) && e[k] == ':' && atoi(e + k + 1) == d->rank;
    if (hit)            // a test-only hook: never silent when it fires
        fprintf(stderr, "[trpo_mi355x] WARNING: TRPO_COMM_FAULT=%s is set: rank %d %s its self-check "
                        "all-reduce on purpose (fault injection for tests)\n", e, d->rank,
                !strcmp(kind, "hang") ? "skips" : "corrupts");
    return hit;
}

extern "C" int trpo_dev_comm_verify(trpo_dev *d, long timeout_ms, long *bad) {
    if (bad) *bad = 0;
    if (!d) return -1;
    if (d->comm_aborted) return -4;
    if (!has_collective(d)) return 0;
    HCHK(hipSetDevice(d->device));
    const size_t count = d->atomic ? (size_t)d->Rc * d->Ps : (size_t)d->nw;
    // a buffer that exists already (no allocation while another rank's exchange may be waiting):
    // the atomic sink set (never consumed) or the slab-path reduced vector (rewritten by every FVP)
    double *buf = d->atomic ? d->pacc + (long)RMAX * d->Ps : d->zacc;
    if (const int hrc = ensure_hst(d, count, true)) return hrc;
    for (size_t i = 0; i < count; ++i) d->hst[i] = ldexp((double)(1 + i % 251), d->rank);
    if (comm_fault(d, "verify")) d->hst[0] += 1.0;
    hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv((long)count, 256)), dim3(256), 0, d->stream,
                       (const double *)d->hst_dev, buf, (int)count);
    HCHK(hipGetLastError());
    int rc = comm_fault(d, "hang") ? 0 : allreduce(d, buf, count);
    if (rc) return rc;
    hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv((long)count, 256)), dim3(256), 0, d->stream, (const double *)buf,
                       d->hst_dev, (int)count);
    HCHK(hipGetLastError());
    rc = wait_stream(d, timeout_ms, false);
    d->hst_pending = 0;
    if (rc) return rc;
    rc = trpo_dev_comm_error(d);
    if (rc) return rc;
    const double f = ldexp(1.0, d->world) - 1.0;
    long nbad = 0;
    for (size_t i = 0; i < count; ++i) nbad += d->hst[i] != f * (double)(1 + i % 251);
    if (bad) *bad = nbad;
    return nbad ? -7 : 0;
}

// ---------------------------------------------------------------------------
// Peer-window exchange (trpo_peer.hip).  Two steps, like RCCL's unique id: every rank opens its
// window and hands the exported handle to the caller's bootstrap; then every rank attaches with the
// world's handles in rank order (or, for contexts of one process, their window pointers).  Attaching
// replaces an RCCL communicator or host group: all collectives of the context then go through the
// exchange kernel.  All ranks must attach concurrently (the attach all-reduces the shard sizes).
// ---------------------------------------------------------------------------
static size_t peer_slot_doubles(const trpo_dev *d) {
    size_t s = (size_t)RMAX * d->Ps;                       // a standalone FVP's replica sets
    if (s < (size_t)d->P + 1) s = (size_t)d->P + 1;        // the policy-gradient sums
    if (s < 64) s = 64;                                    // line-search sums, shard sizes
    return s;
}

// Round 4 refused the peer exchange under any HIP runtime but the one the library was built against: under
// the ROCm 7.0 copy a PyTorch wheel bundles, contexts created AFTER peer-attached contexts had run and been
// destroyed computed wrong FVPs.  Round 5 found the trigger -- returning the uncached peer window to that
// runtime (hipFree); none of the later contexts' own buffers reuses the freed range and no kernel reads
// memory the library never wrote (profiles/r05_peer_diag/) -- and trpo_peer.hip now keeps uncached windows
// for the life of the process (a pool reused by later peer contexts), so the exchange runs under either
// runtime (tests/test_gpu_peer.py::test_peer_slab_paths_torch_runtime_first).
extern "C" int trpo_dev_peer_open(trpo_dev *d, void *handle64) {
    if (!d) return -1;
    HCHK(hipSetDevice(d->device));
    if (!d->peer) {
        d->peer = trpo_peer_create(d->device, peer_slot_doubles(d));
        if (!d->peer) return -2;
        HCHK(trpo_malloc((void **)&d->zred, sizeof(double) * 2 * RMAX * d->Ps));
        HCHK(hipMemset(d->zred, 0, sizeof(double) * 2 * RMAX * d->Ps));
        HCHK(trpo_malloc((void **)&d->ptmp, sizeof(double) * trpo_peer_slot(d->peer)));
        HCHK(trpo_malloc((void **)&d->pn, sizeof(double) * PEER_WMAX));
    }
    return handle64 ? trpo_peer_handle(d->peer, handle64) : 0;
}

extern "C" void *trpo_dev_peer_window(trpo_dev *d) { return d && d->peer ? trpo_peer_window(d->peer) : NULL; }

extern "C" int trpo_dev_set_peers(trpo_dev *d, int rank, int world, const void *handles, void *const *local) {
    if (!d || !d->peer || world < 1 || world > PEER_WMAX || rank < 0 || rank >= world) return -1;
    HCHK(hipSetDevice(d->device));
    DSYNC(d);
    const int rc = trpo_peer_connect(d->peer, rank, world, handles, local, d->stream);
    if (rc) return rc;
    if (d->comm) {
        ncclCommDestroy(d->comm);
        d->comm = NULL;
    }
    d->group = NULL;
    d->peer_on = world > 1;
    d->rank = rank;
    d->world = world;
    // contexts of ONE process sharing a device: the CG runs eagerly -- instantiating a graph may
    // allocate (and wait for the device) while another rank's exchange already spins for this one
    if (local) d->no_graph = 1;
    cg_graph_drop(d);
    const int rn = refresh_n_total(d);
    return rn ? rn : trpo_dev_comm_error(d);
}

// -4 after a peer exchange whose wait timed out (a rank missing) or an abort; 0 otherwise.  A timed-out
// exchange's records (rank, workgroup, exchange, missing peer, tag seen) go to stderr the first time.
extern "C" int trpo_dev_comm_error(const trpo_dev *d) {
    if (d && d->comm_aborted) return -4;
    if (!(d && d->peer_on && trpo_peer_error(d->peer))) return 0;
    trpo_peer_report(d->peer);
    return -4;
}

extern "C" const char *trpo_hip_runtime_path(void) {
    Dl_info info;
    if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &info) && info.dli_fname) return info.dli_fname;
    return "";
}

extern "C" const char *trpo_dev_comm_backend(const trpo_dev *d) {
    if (!d) return "";
    if (d->comm_aborted) return "aborted";
    if (d->peer_on)
        return trpo_peer_proto(d->peer) != 1 && d->world <= 8 ? "peer-xgmi (uncached window, tagged granules)"
                                                                : "peer-xgmi (uncached window, fenced hand-off)";
    if (d->comm) return "rccl";
    if (d->group) return "host-group";
    return "none";
}
