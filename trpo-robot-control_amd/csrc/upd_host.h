// upd_host.h -- section of trpo_update.hip: the host scaffolding every stage of the update path shares
// (device and pinned buffers that grow, where a block's activation rows live, the kernels' LDS limit) and
// the per-context state of the policy side.  Host code only.

// a device buffer of at least `count` doubles, zeroed when it is (re)allocated
static int ensure(double **p, size_t *cap, size_t count, hipStream_t st) {
    if (count <= *cap && *p) return 0;
    if (*p) hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HCHK(trpo_malloc((void **)p, sizeof(double) * (count ? count : 1)));
    HCHK(hipMemsetAsync(*p, 0, sizeof(double) * (count ? count : 1), st));
    *cap = count;
    return 0;
}

// A pinned, device-mapped host buffer: results are written into it by a kernel (no copy-engine round trips
// through pageable memory) and small inputs go the other way through it.  Growing it frees the old one and
// zero-fills the new one: the flag words the host spins on (export_solve_kernel's, sum_slabs64_host_kernel's,
// the inference kernels') live in these buffers and must start below any sequence number.
struct PinBuf {
    double *host = nullptr, *dev = nullptr;
    size_t cap = 0;
};
static int pin_reserve(PinBuf *b, size_t count) {
    if (count <= b->cap && b->host) return 0;
    if (b->host) hipHostFree(b->host);
    b->host = b->dev = nullptr;
    b->cap = 0;
    HCHK(hipHostMalloc((void **)&b->host, sizeof(double) * count, TRPO_HOST_COHERENT));
    HCHK(hipHostGetDevicePointer((void **)&b->dev, b->host, 0));
    b->cap = count;
    memset(b->host, 0, sizeof(double) * count);
    return 0;
}
static void pin_free(PinBuf *b) {
    if (b->host) hipHostFree(b->host);
}

// Where the `rows` activation rows [row][RS] of one block of a one-sample-per-lane kernel live: in LDS when
// 8 rows RS bytes fit LDS_CAP -- and `theta` doubles of parameters staged behind them when those fit too --,
// else in a global scratch of rows RS doubles per block (rows_scratch).  lds: the launch's dynamic LDS bytes.
struct RowsPlan {
    int use_lds = 0, theta_lds = 0, lds = 0;
};
static RowsPlan rows_plan(int rows, size_t theta = 0) {
    const size_t bytes = sizeof(double) * (size_t)rows * RS, tbytes = sizeof(double) * theta;
    RowsPlan p;
    p.use_lds = bytes <= (size_t)LDS_CAP;
    p.theta_lds = p.use_lds && bytes + tbytes <= (size_t)LDS_CAP;
    p.lds = p.use_lds ? (int)(bytes + (p.theta_lds ? tbytes : 0)) : 0;
    return p;
}
static int rows_scratch(const RowsPlan &p, double **ws, size_t *cap, int rows, long blocks, hipStream_t st) {
    return p.use_lds ? 0 : ensure(ws, cap, (size_t)rows * RS * blocks, st);
}
// the kernel form of a plan: theta and Y in LDS, Y in LDS, Y in global scratch
#define ROWS_FORM(k, p) ((p).theta_lds ? k<true, true> : ((p).use_lds ? k<true, false> : k<false, false>))

// raises the dynamic-LDS limit of `kernels` to LDS_CAP, once per *done
static hipError_t lds_limit_once(int *done, std::initializer_list<const void *> kernels) {
    if (*done) return hipSuccess;
    for (const void *k : kernels)
        if (const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CAP)) return e;
    *done = 1;
    return hipSuccess;
}

// `bytes` from p must be device memory of `device`, inside one allocation: 0, or -1 with the cause in err.
// A host address makes the query fail: the error is cleared, not handed on.
static int devptr_check(int device, const void *p, size_t bytes, const char *name, char *err, size_t errlen) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    const char *why = nullptr;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        why = "is not device memory";
    } else if (at.type != hipMemoryTypeDevice || at.isManaged) {
        why = "is not device memory (host, pinned and managed memory are refused)";
    } else if (at.device != device) {
        why = "is memory of another HIP device";
    } else {
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
            (void)hipGetLastError();
            why = "has no known allocation";
        } else {
            const size_t at0 = (size_t)((const char *)p - (const char *)base);
            if (at0 > size || bytes > size - at0) why = "extends past the end of its allocation";
        }
    }
    if (why && err) snprintf(err, errlen, "%s %s", name, why);
    return why ? -1 : 0;
}
// the policy side's state, one per device context (trpo_dev_update_state)
struct UpdState {
    double *roll = nullptr;                // [n][2A+1]: Mean[A], Action[A], Adv
    size_t roll_cap = 0, roll_n = 0;
    int have_roll = 0;
    double *ws = nullptr;                  // global activation scratch (big nets only)
    size_t ws_cap = 0;
    double *slabs = nullptr;               // per-block partial sums
    size_t slab_cap = 0;
    double *sum = nullptr;                 // [P + 1]
    double *fs = nullptr;                  // fullstep [P]
    double *sums = nullptr;                // [64]
    double *sums_kl = nullptr;             // [128]: {surr, q} per candidate (the KL variants)
    double *tpad = nullptr;                // register path: padded parameters [nk][PADW]
    size_t tpad_cap = 0;
    double *tk = nullptr;                  // generic path: the line-search candidates [nk][P]
    size_t tk_cap = 0;
    int lds_set = 0;
    PinBuf hst;                            // the update's results out, fullstep in
    unsigned seq = 0;                       // export_solve_kernel's flags: the last update's sequence number
    size_t flag_at = 0;                     // where they were zeroed last (they move with maxiter)
    unsigned roll_gen = 0;                 // bumped by every rollout upload
    // policy inference (trpo_dev_act): its own pinned buffer [flags | obs in | mean, action, logp out] (the
    // update's flag words live in hst and must not be disturbed), the device buffers of a batch too large for
    // it, and the kept (mean, action) rows [n][2A] of the rollout hand-off
    PinBuf ah;
    unsigned aseq = 0;
    double *aobs = nullptr, *aout = nullptr, *kept = nullptr;
    size_t aobs_cap = 0, aout_cap = 0, kept_cap = 0;
    int act_lds_set[6] = {};               // per IO of the inference kernels (act_launch): its LDS limit is raised
    // the rollout record (trpo_dev_record_begin .. _commit): observation rows [rec_rows][L0] and
    // kept rows [rec_rows][2A] the REC inference kernels fill; a commit hands them to the context (obs64, kept)
    // or gathers them into packed buffers that it hands over; the ragged commit's episode offsets as ints
    double *rec_obs = nullptr, *rec_kept = nullptr, *rec_off = nullptr;
    size_t rec_rows = 0, rec_off_cap = 0;
    // the device-resident loop (trpo_dev_act_dev, trpo_dev_record_episodes): the two events that
    // order the context's stream and the caller's against each other, and the episode scan's pinned results
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    PinBuf eh;
    // the observation filter (trpo_dev_obsnorm_*; the layout is in upd_act.h): on_st is NULL while
    // the filter is not enabled; on_nl / on_np are the host's copies of the live and pending counts; on_part the
    // statistics kernel's chunk sums
    double *on_st = nullptr, *on_part = nullptr;
    size_t on_part_cap = 0;
    PinBuf onh;                            // set's staging buffer [mean | m2], on_set_ev behind the copy out of it
    hipEvent_t on_set_ev = nullptr;
    double on_clip = 0.0, on_eps = 0.0, on_nl = 0.0, on_np = 0.0;
};

static UpdState *state(trpo_dev *d) {
    void **slot = trpo_dev_update_state(d);
    if (!*slot) *slot = new UpdState();
    return (UpdState *)*slot;
}

void trpo_update_state_free(void *state) {
    UpdState *u = (UpdState *)state;
    if (!u) return;
    void *ptrs[] = {u->roll, u->ws, u->slabs, u->sum, u->fs, u->sums, u->sums_kl, u->tpad, u->tk, u->aobs, u->aout,
                    u->kept, u->rec_obs, u->rec_kept, u->rec_off, u->on_st, u->on_part};
    for (void *p : ptrs)
        if (p) hipFree(p);
    pin_free(&u->hst);
    pin_free(&u->ah);
    pin_free(&u->eh);
    pin_free(&u->onh);
    if (u->on_set_ev) hipEventDestroy(u->on_set_ev);
    if (u->ev_in) hipEventDestroy(u->ev_in);
    if (u->ev_out) hipEventDestroy(u->ev_out);
    delete u;
}
