// upd_act.h -- section of trpo_update.hip: policy inference on the device and the rollout hand-off from it.

// ===========================================================================
// Policy inference on the device (no reference counterpart): for a batch of m observation rows,
// sample i being ROW r_i = row0 + i * stride of the rollout,
//   mean_i  = the policy MLP at the context's theta (forward64's arithmetic: bias first, inputs ascending,
//             one fma per input, then the activation)
//   z[i][a] = Box-Muller normals from Philox4x32-10 (Salmon et al., SC'11), key = seed, counter =
//             (r_i lo, r_i hi, step lo, (step >> 32) << 16 | pair), pair = a / 2
//   action  = mean + exp(LogStd) z,   logp = -1/2 sum z^2 - sum LogStd - (A/2) ln(2 pi)
// A result depends on (theta, obs row, seed, step, r_i) alone: both kernel forms below run the same
// operations in the same order per row, so block, lane and call geometry never show in the bits.
//   act_kernel<LDSY>    sample per lane: forward64 on 64-row passes, Y rows in LDS or the ws scratch
//   act_neuron_kernel   neuron per lane: one wave per row, lane j owns outputs j, j + 64, ...; the previous
//                       layer's activations are broadcast from LDS, W[k * out + j] is read coalesced over j
// One call is one launch: obs is read through the pinned mapped buffer, the results are stored into it at
// system scope, and each block raises its flag word behind its drained stores; the host spins on the flags
// under a time bound.  No kernel waits for anything.
// The REC instantiations of both forms (trpo_ctx_act_record) also store the observation row into
// the rollout record rec_obs[r_i][L0], and (mean, action) into its kept rows through O.kept: plain stores to
// HBM, read by later launches on the same stream.  The row comes from what the kernel already loaded -- obs may
// be host memory behind the link and is read once.  The other instantiations keep their code.
// The ActDev instantiations of both forms (trpo_ctx_act_dev / _act_record_dev) read obs from and
// store the results to the caller's device arrays, fp64 or fp32, with plain stores and no flag word.
// ===========================================================================
struct ActRng {
    unsigned k0, k1;                 // key: seed lo32, hi32
    unsigned s0, s1;                 // counter words 2, 3: step lo32, (step >> 32) << 16 (| pair)
    unsigned long long row0, stride; // sample i is row row0 + i * stride
};
struct ActOut {
    double *mean, *action, *logp;    // [m][A], [m][A] or NULL (means only), [m] or NULL
    double *kept;                    // [n][2A] or NULL (REC: the record's kept rows [rows][2A])
    double *rec_obs;                 // REC: the record's observation rows [rows][L0]
    unsigned *flags;                 // one word per block, or NULL (the host synchronises the stream)
    unsigned seq;
};

// one Philox4x32-10 block: 32-bit mulhi / mullo, ten rounds, the key bumped between rounds
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const unsigned n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0;
        c1 = l1;
        c2 = n2;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0;
    o[1] = c1;
    o[2] = c2;
    o[3] = c3;
}

// the two standard normals of (row, pair): u1 in (0, 1], u2 in [0, 1), 53 bits each
__device__ __forceinline__ void act_normal_pair(const ActRng &g, unsigned long long row, int pair, double &z0,
                                                double &z1) {
    unsigned o[4];
    philox4x32_10((unsigned)row, (unsigned)(row >> 32), g.s0, g.s1 | (unsigned)pair, g.k0, g.k1, o);
    const double u1 = (double)((((unsigned long long)o[0] << 21) | (o[1] >> 11)) + 1ull) * 0x1p-53;
    const double u2 = (double)(((unsigned long long)o[2] << 21) | (o[3] >> 11)) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}
// explicit fmas: the two forms must round alike whatever the compiler contracts around them
__device__ __forceinline__ double act_action(double mean, double logstd, double z) { return fma(exp(logstd), z, mean); }
__device__ __forceinline__ double act_logp(double sz2, double sls, int A) {
    return fma(-0.5 * (double)A, 1.8378770664093453 /* ln(2 pi) */, fma(-0.5, sz2, -sls));
}
__device__ __forceinline__ void act_store(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// every result of the block is in memory before its flag word says so
__device__ __forceinline__ void act_publish(const ActOut &O) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (O.flags && threadIdx.x == 0)
        __hip_atomic_store(O.flags + blockIdx.x, O.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Where a launch's rows come from and go to (the IO parameter of both forms).  ActHost: the pinned mapped
// buffer, fp64, system-scope stores and the flag words above.  ActDev<T> (the trpo_ctx_act*_dev calls, DESIGN
// §5.13): the caller's device arrays of T = double or float -- obs widened exactly on load, mean / action / logp
// rounded once (to nearest even) on a plain store, no drain and no flag word: the stream orders the readers.
// The record and the kept rows hold the fp64 values in either case.
template <class T>
struct ActOutDev {
    T *mean, *action, *logp;         // as ActOut's, in the caller's element type
    double *kept, *rec_obs;
};
struct ActHost {
    using T = double;
    using Out = ActOut;
    static constexpr bool dev = false;
    static __device__ __forceinline__ void store(double *p, double v) { act_store(p, v); }
};
template <class T_>
struct ActDev {
    using T = T_;
    using Out = ActOutDev<T_>;
    static constexpr bool dev = true;
    static __device__ __forceinline__ void store(T_ *p, double v) { *p = (T_)v; }
};

template <bool LDSY, bool REC = false, class IO = ActHost>
__global__ void __launch_bounds__(UT)
act_kernel(Net net, const double *__restrict__ th, const typename IO::T *__restrict__ obs, int m, ActRng g,
           double *ws, int rows, typename IO::Out O) {
    extern __shared__ double lds64[];
    const int tid = threadIdx.x;
    double *Y = LDSY ? lds64 : ws + (long)blockIdx.x * rows * RS;
    int roff[MAXL + 1];
    row_offsets(net, roff);
    const int P = net.P, A = net.A, mrow = roff[net.nl - 1];
    const ThetaPlain T{th};
    const int npass = (m + UT - 1) / UT;
    for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        const int s = pass * UT + tid;
        const bool live = s < m;
        forward64(net, T, obs, s, live, Y, roff, tid);
        if constexpr (REC) {
            // the pass's rows from the first L0 rows of Y, where forward64 put them: one element per thread,
            // a row's L0 values by adjacent lanes (the trip count is block-uniform: every lane is here)
            __syncthreads();
            const int L0 = net.L[0], nrow = m - pass * UT < UT ? m - pass * UT : UT;
            for (int q = tid; q < nrow * L0; q += UT) {
                const int i = q / L0, k = q - i * L0;
                const unsigned long long ri = g.row0 + (unsigned long long)(pass * UT + i) * g.stride;
                O.rec_obs[ri * L0 + k] = Y[k * RS + i];
            }
        }
        if (!live) continue;
        for (int a = 0; a < A; ++a) IO::store(O.mean + (long)s * A + a, Y[(mrow + a) * RS + tid]);
        if (!O.action) continue;
        const unsigned long long row = g.row0 + (unsigned long long)s * g.stride;
        double *kp = O.kept ? O.kept + row * (2 * A) : nullptr;
        double sz2 = 0.0, sls = 0.0;
        for (int a = 0; a < A; a += 2) {
            double z[2];
            act_normal_pair(g, row, a >> 1, z[0], z[1]);
            for (int e = 0; e < 2 && a + e < A; ++e) {
                const double mu = Y[(mrow + a + e) * RS + tid], ls = th[P - A + a + e];
                const double ac = act_action(mu, ls, z[e]);
                IO::store(O.action + (long)s * A + a + e, ac);
                if (kp) {
                    kp[a + e] = mu;
                    kp[A + a + e] = ac;
                }
                sz2 = fma(z[e], z[e], sz2);
                sls += ls;
            }
        }
        if (O.logp) IO::store(O.logp + s, act_logp(sz2, sls, A));
    }
    if constexpr (!IO::dev) act_publish(O);
}

// one wave per row.  LDS per wave: the row's activations of every layer [roff[i] + j], then z [2 pairs]
constexpr int AN_WAVES = 4;
template <bool REC, class IO = ActHost>
__global__ void __launch_bounds__(64 * AN_WAVES)
act_neuron_kernel(Net net, const double *__restrict__ th, const typename IO::T *__restrict__ obs, int m, ActRng g,
                  int wstride, typename IO::Out O) {
    extern __shared__ double lds64[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int roff[MAXL + 1];
    row_offsets(net, roff);
    const int P = net.P, A = net.A, L0 = net.L[0], tot = roff[net.nl];
    double *Yw = lds64 + (long)w * wstride, *Zw = Yw + tot;
    const double *mu = Yw + roff[net.nl - 1];
    // block-uniform trip count: the barriers below are reached by every wave
    for (int base = blockIdx.x * AN_WAVES; base < m; base += gridDim.x * AN_WAVES) {
        const int s = base + w;
        const bool live = s < m;
        for (int k = lane; k < L0; k += 64) {
            const double o = live ? (double)obs[(long)s * L0 + k] : 0.0;
            Yw[k] = o;
            if constexpr (REC)
                if (live) O.rec_obs[(g.row0 + (unsigned long long)s * g.stride) * L0 + k] = o;
        }
        __syncthreads();
        for (int i = 0; i + 1 < net.nl; ++i) {
            const int in = net.L[i], out = net.L[i + 1], a = net.act[i + 1];
            const double *W = th + net.woff[i], *yi = Yw + roff[i];
            for (int j = lane; j < out; j += 64) {
                double x = th[net.boff[i] + j];
#pragma unroll 8
                for (int k = 0; k < in; ++k) x = fma(yi[k], W[k * out + j], x);   // forward64's chain
                Yw[roff[i + 1] + j] = act_y64(a, x);
            }
            __syncthreads();
        }
        if (live)
            for (int a = lane; a < A; a += 64) IO::store(O.mean + (long)s * A + a, mu[a]);
        if (!O.action) continue;                     // kernel-uniform
        const unsigned long long row = g.row0 + (unsigned long long)s * g.stride;
        for (int pr = lane; 2 * pr < A; pr += 64) act_normal_pair(g, row, pr, Zw[2 * pr], Zw[2 * pr + 1]);
        __syncthreads();
        if (!live) continue;                         // wave-uniform; no barrier follows in this trip
        double *kp = O.kept ? O.kept + row * (2 * A) : nullptr;
        for (int a = lane; a < A; a += 64) {
            const double ac = act_action(mu[a], th[P - A + a], Zw[a]);
            IO::store(O.action + (long)s * A + a, ac);
            if (kp) {
                kp[a] = mu[a];
                kp[A + a] = ac;
            }
        }
        if (lane == 0 && O.logp) {
            double sz2 = 0.0, sls = 0.0;
            for (int a = 0; a < A; ++a) {
                sz2 = fma(Zw[a], Zw[a], sz2);
                sls += th[P - A + a];
            }
            IO::store(O.logp + s, act_logp(sz2, sls, A));
        }
    }
    if constexpr (!IO::dev) act_publish(O);
}

// roll rows [kept mean_i, kept action_i, adv[i]] (roll_interleave_kernel with both halves already on the device)
__global__ void roll_from_kept_kernel(const double *__restrict__ kept, const double *__restrict__ adv, int n, int A,
                                      double *__restrict__ roll) {
    const int W = 2 * A + 1;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)n * W) return;
    const int s = (int)(q / W), c = (int)(q % W);
    roll[q] = c < 2 * A ? kept[(long)s * 2 * A + c] : adv[s];
}

constexpr int ACT_MAXG = 1024;                      // blocks of one launch == flag words
constexpr size_t ACT_PIN = (size_t)1 << 18;         // doubles of obs + results that go through the pinned buffer
constexpr size_t ACT_NEURON_LDS = 64 * 1024;        // neuron form: AN_WAVES rows of activations must fit
constexpr size_t ACT_DEV_LANE_FROM = 16384;         // device rows: the lane form from this many (trpo_dev_act_dev)

// the flag words under a time bound ($TRPO_ACT_TIMEOUT_MS, default 10 s): -6 past it; after 2 ms the stream is
// queried between spins, so a launch that failed returns its error instead of spinning
static int act_wait_flags(hipStream_t st, const unsigned *flags, int nf, unsigned seq) {
    const char *e = getenv("TRPO_ACT_TIMEOUT_MS");
    const long limit_ms = e && atol(e) > 0 ? atol(e) : 10000;
    const auto t0 = std::chrono::steady_clock::now();
    int k = 0;
    for (unsigned long i = 1;; ++i) {
        while (k < nf && __atomic_load_n(flags + k, __ATOMIC_ACQUIRE) == seq) ++k;
        if (k == nf) return 0;
        if ((i & 63) == 0) {
            const auto dt = std::chrono::steady_clock::now() - t0;
            if (dt > std::chrono::milliseconds(limit_ms)) return -6;
            if (dt > std::chrono::microseconds(2000)) {
                const hipError_t q = hipStreamQuery(st);
                if (q == hipSuccess) {
                    while (k < nf && __atomic_load_n(flags + k, __ATOMIC_ACQUIRE) == seq) ++k;
                    return k == nf ? 0 : -2;
                }
                if (q != hipErrorNotReady) return -2;
            }
        }
        __builtin_ia32_pause();
    }
}

// form: 0 by the measured rule, 1 sample per lane, 2 neuron per lane.  keep: (mean, action) of
// row r_i also into the kept buffer [n][2A] (the caller has checked every r_i < n); keep == 2: obs_i and
// (mean, action) of row r_i into the rollout record instead (every r_i < its rows).  action == NULL: means only.
extern "C" int trpo_dev_act(trpo_dev *d, const double *obs, size_t m, unsigned long long seed, unsigned long long step,
                            size_t row0, size_t stride, int keep, int form, double *mean, double *action,
                            double *logp, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!d || !obs || !mean || !m || !stride || (!action && (logp || keep))) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    const Net &net = v.net;
    const int A = net.A, L0 = net.L[0];
    int tot = 0;
    for (int i = 0; i < net.nl; ++i) tot += net.L[i];
    if (m > (size_t)0x7fffffff / (size_t)(L0 > 2 * A ? L0 : 2 * A) || A > 2 * 65536) {
        if (err) snprintf(err, errlen, "batch of %zu rows (or %d actions) is beyond the kernels' indexing", m, A);
        return -1;
    }
    const int wstride = tot + A + (A & 1);
    const size_t nlds = sizeof(double) * AN_WAVES * (size_t)wstride;
    if (form == 2 && nlds > ACT_NEURON_LDS) {
        if (err) snprintf(err, errlen, "TRPO_ACT_FORM=neuron: the network's %d activations per row exceed its LDS", tot);
        return -1;
    }
    // a batch whose obs and results fit the pinned buffer goes through it; the measured rule
    // (profiles/act_stage.json): the neuron form for those, the lane form for the staged ones
    const size_t nin = m * (size_t)L0, nout = m * (size_t)(action ? 2 * A + 1 : A);
    const bool pinned = nin + nout <= ACT_PIN;
    const bool neuron = form ? form == 2 : (nlds <= ACT_NEURON_LDS && pinned);
    HCHK(hipSetDevice(v.device));
    UpdState *u = state(d);
    const bool rec = keep == 2;
    if (rec && (!u->rec_obs || !u->rec_kept)) {
        if (err) snprintf(err, errlen, "no recording in progress");
        return -1;
    }
    if (pin_reserve(&u->ah, ACT_MAXG / 2 + ACT_PIN)) return -2;     // once: the flag words start below any seq
    HCHK(lds_limit_once(&u->act_lds_set, {(const void *)act_kernel<true>, (const void *)act_kernel<true, true>}));
    if (keep && !rec && ensure(&u->kept, &u->kept_cap, v.n * 2 * (size_t)A, v.stream)) return -2;
    double *din, *dout;
    if (pinned) {
        din = u->ah.dev + ACT_MAXG / 2;
        dout = din + nin;
        memcpy(u->ah.host + ACT_MAXG / 2, obs, sizeof(double) * nin);
    } else {
        if (ensure(&u->aobs, &u->aobs_cap, nin, v.stream) || ensure(&u->aout, &u->aout_cap, nout, v.stream)) return -2;
        din = u->aobs;
        dout = u->aout;
        HCHK(hipMemcpyAsync(din, obs, sizeof(double) * nin, hipMemcpyHostToDevice, v.stream));
    }
    if (++u->aseq == 0) u->aseq = 1;
    ActRng g{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)step, (unsigned)(step >> 32) << 16, row0, stride};
    ActOut O{dout, action ? dout + m * (size_t)A : nullptr, action && logp ? dout + 2 * m * (size_t)A : nullptr,
             rec ? u->rec_kept : (keep ? u->kept : nullptr), rec ? u->rec_obs : nullptr,
             pinned ? (unsigned *)u->ah.dev : nullptr, u->aseq};
    int G;
    if (neuron) {
        G = cdiv((long)m, AN_WAVES) < ACT_MAXG ? cdiv((long)m, AN_WAVES) : ACT_MAXG;
        hipLaunchKernelGGL(rec ? act_neuron_kernel<true> : act_neuron_kernel<false>, dim3(G), dim3(64 * AN_WAVES),
                           nlds, v.stream, net, v.theta64, (const double *)din, (int)m, g, wstride, O);
    } else {
        G = cdiv((long)m, UT) < ACT_MAXG ? cdiv((long)m, UT) : ACT_MAXG;
        RowsPlan y;
        if (act_storage(u, tot, G, v.stream, &y)) return -2;
        const auto k = rec ? (y.use_lds ? act_kernel<true, true> : act_kernel<false, true>)
                           : (y.use_lds ? act_kernel<true> : act_kernel<false>);
        hipLaunchKernelGGL(k, dim3(G), dim3(UT), y.lds, v.stream, net, v.theta64, (const double *)din, (int)m, g,
                           u->ws, tot, O);
    }
    HCHK(hipGetLastError());
    const size_t mA = m * (size_t)A;
    if (pinned) {
        if (const int rc = act_wait_flags(v.stream, (const unsigned *)u->ah.host, G, u->aseq)) {
            // nothing of the launch is handed out; later work queues behind it on the stream
            if (rc == -6 && err) snprintf(err, errlen, "the inference kernel did not finish within its time bound");
            return rc;
        }
        const double *res = u->ah.host + ACT_MAXG / 2 + nin;
        memcpy(mean, res, sizeof(double) * mA);
        if (action) memcpy(action, res + mA, sizeof(double) * mA);
        if (action && logp) memcpy(logp, res + 2 * mA, sizeof(double) * m);
        return 0;
    }
    HCHK(hipMemcpyAsync(mean, dout, sizeof(double) * mA, hipMemcpyDeviceToHost, v.stream));
    if (action) HCHK(hipMemcpyAsync(action, dout + mA, sizeof(double) * mA, hipMemcpyDeviceToHost, v.stream));
    if (action && logp) HCHK(hipMemcpyAsync(logp, dout + 2 * mA, sizeof(double) * m, hipMemcpyDeviceToHost, v.stream));
    DSYNC(d);
    return 0;
}

// ===========================================================================
// The device-resident loop: the caller's arrays are device memory and its work is ordered by a
// stream of its own.  Every launch still runs on the context's stream: an event recorded on the caller's stream is
// waited on there before the launch, and an event recorded behind the launch is waited on by the caller's stream.
// The host never waits; the context's later calls are ordered by their own stream as before.
// ===========================================================================

// the context's stream behind the caller's (st == NULL or the context's own: nothing to order)
static int dev_loop_enter(UpdState *u, hipStream_t own, hipStream_t st) {
    if (!st || st == own) return 0;
    if (!u->ev_in) {
        HCHK(hipEventCreateWithFlags(&u->ev_in, hipEventDisableTiming));
        HCHK(hipEventCreateWithFlags(&u->ev_out, hipEventDisableTiming));
    }
    HCHK(hipEventRecord(u->ev_in, st));
    HCHK(hipStreamWaitEvent(own, u->ev_in, 0));
    return 0;
}
// and the caller's stream behind what the context has just enqueued
static int dev_loop_leave(UpdState *u, hipStream_t own, hipStream_t st) {
    if (!st || st == own) return 0;
    HCHK(hipEventRecord(u->ev_out, own));
    HCHK(hipStreamWaitEvent(st, u->ev_out, 0));
    return 0;
}

template <class T>
static int act_dev_launch(trpo_dev *d, const trpo_dev_view &v, UpdState *u, const void *obs, size_t m,
                          const ActRng &g, int keep, bool neuron, int tot, int wstride, size_t nlds, void *mean,
                          void *action, void *logp, hipStream_t st) {
    using IO = ActDev<T>;
    const bool rec = keep == 2;
    const Net &net = v.net;
    ActOutDev<T> O{(T *)mean, (T *)action, (T *)logp, rec ? u->rec_kept : (keep ? u->kept : nullptr),
                   rec ? u->rec_obs : nullptr};
    // everything that can fail or must allocate comes before the streams are tied
    RowsPlan y;
    int G;
    if (neuron) {
        G = cdiv((long)m, AN_WAVES) < ACT_MAXG ? cdiv((long)m, AN_WAVES) : ACT_MAXG;
    } else {
        G = cdiv((long)m, UT) < ACT_MAXG ? cdiv((long)m, UT) : ACT_MAXG;
        if (act_storage(u, tot, G, v.stream, &y)) return -2;
        HCHK(lds_limit_once(&u->act_dev_lds_set,
                            {(const void *)act_kernel<true, false, ActDev<double>>,
                             (const void *)act_kernel<true, true, ActDev<double>>,
                             (const void *)act_kernel<true, false, ActDev<float>>,
                             (const void *)act_kernel<true, true, ActDev<float>>}));
    }
    if (const int rc = dev_loop_enter(u, v.stream, st)) return rc;
    if (neuron) {
        const auto k = rec ? act_neuron_kernel<true, IO> : act_neuron_kernel<false, IO>;
        hipLaunchKernelGGL(k, dim3(G), dim3(64 * AN_WAVES), nlds, v.stream, net, v.theta64, (const T *)obs, (int)m, g,
                           wstride, O);
    } else {
        const auto k = rec ? (y.use_lds ? act_kernel<true, true, IO> : act_kernel<false, true, IO>)
                           : (y.use_lds ? act_kernel<true, false, IO> : act_kernel<false, false, IO>);
        hipLaunchKernelGGL(k, dim3(G), dim3(UT), y.lds, v.stream, net, v.theta64, (const T *)obs, (int)m, g, u->ws, tot,
                           O);
    }
    HCHK(hipGetLastError());
    return dev_loop_leave(u, v.stream, st);
}

// trpo_dev_act on the caller's device arrays (element type by dtype: 0 double, 1 float), asynchronous: returns
// once the launch is enqueued.  keep and form as trpo_dev_act's.  The form rule of these calls is their own:
// the host rule was measured over the link (profiles/device_loop.md).
extern "C" int trpo_dev_act_dev(trpo_dev *d, const void *obs, size_t m, unsigned long long seed,
                                unsigned long long step, size_t row0, size_t stride, int keep, int form, int dtype,
                                void *mean, void *action, void *logp, void *stream, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!d || !obs || !mean || !m || !stride || (!action && (logp || keep)) || (dtype != 0 && dtype != 1)) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    const Net &net = v.net;
    const int A = net.A, L0 = net.L[0];
    int tot = 0;
    for (int i = 0; i < net.nl; ++i) tot += net.L[i];
    if (m > (size_t)0x7fffffff / (size_t)(L0 > 2 * A ? L0 : 2 * A) || A > 2 * 65536) {
        if (err) snprintf(err, errlen, "batch of %zu rows (or %d actions) is beyond the kernels' indexing", m, A);
        return -1;
    }
    const int wstride = tot + A + (A & 1);
    const size_t nlds = sizeof(double) * AN_WAVES * (size_t)wstride;
    if (form == 2 && nlds > ACT_NEURON_LDS) {
        if (err) snprintf(err, errlen, "TRPO_ACT_FORM=neuron: the network's %d activations per row exceed its LDS", tot);
        return -1;
    }
    HCHK(hipSetDevice(v.device));
    UpdState *u = state(d);
    const bool rec = keep == 2;
    if (rec && (!u->rec_obs || !u->rec_kept)) {
        if (err) snprintf(err, errlen, "no recording in progress");
        return -1;
    }
    const size_t es = dtype ? sizeof(float) : sizeof(double);
    if (devptr_check(v.device, obs, es * m * L0, "obs_dev", err, errlen) ||
        devptr_check(v.device, mean, es * m * A, "mean_dev", err, errlen) ||
        (action && devptr_check(v.device, action, es * m * A, "action_dev", err, errlen)) ||
        (logp && devptr_check(v.device, logp, es * m, "logp_dev", err, errlen)))
        return -1;
    // the rule for device rows, measured (profiles/device_loop.md): one wave per row won at every
    // size up to 4 096 rows on all three nets, the lane form at 50 000; the lane form from 64 rows per CU on
    const bool neuron = form ? form == 2 : (nlds <= ACT_NEURON_LDS && m < ACT_DEV_LANE_FROM);
    if (keep && !rec && ensure(&u->kept, &u->kept_cap, v.n * 2 * (size_t)A, v.stream)) return -2;
    const ActRng g{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)step, (unsigned)(step >> 32) << 16, row0, stride};
    return dtype ? act_dev_launch<float>(d, v, u, obs, m, g, keep, neuron, tot, wstride, nlds, mean, action, logp,
                                         (hipStream_t)stream)
                 : act_dev_launch<double>(d, v, u, obs, m, g, keep, neuron, tot, wstride, nlds, mean, action, logp,
                                          (hipStream_t)stream);
}

// The episode scan: slot e's flags stand at rows e * slot + t.  One wave per slot walks it in 64-step chunks;
// the first chunk with a set flag ends the walk: t* = its first set lane (ballot, find-first).  out[2 e] = the
// length t* + 1 (slot when no flag is set), out[2 e + 1] = 1 when the episode was cut (terminated[t*] == 0, or
// the slot ran out), as doubles into the pinned buffer.
constexpr int EPS_WAVES = 4;
__global__ void __launch_bounds__(64 * EPS_WAVES)
episode_scan_kernel(const unsigned char *__restrict__ term, const unsigned char *__restrict__ trunc, int num_env,
                    long slot, double *out) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * EPS_WAVES + (threadIdx.x >> 6);
    if (e >= num_env) return;                      // wave-uniform; the kernel has no barrier
    const unsigned char *te = term + (long)e * slot, *tr = trunc ? trunc + (long)e * slot : nullptr;
    long len = slot;
    int cut = 1;
    for (long t0 = 0; t0 < slot; t0 += 64) {
        const long t = t0 + lane;
        const bool in = t < slot;
        const int a = in ? te[t] : 0, b = in && tr ? tr[t] : 0;
        const unsigned long long any = __ballot(a != 0 || b != 0);
        if (any) {                                 // wave-uniform
            const int first = __ffsll((long long)any) - 1;
            len = t0 + first + 1;
            cut = __shfl(a, first) == 0;
            break;
        }
    }
    if (lane == 0) {
        out[2 * (long)e] = (double)len;
        out[2 * (long)e + 1] = (double)cut;
    }
}

extern "C" int trpo_dev_record_episodes(trpo_dev *d, const unsigned char *term, const unsigned char *trunc,
                                        size_t num_env, size_t slot, void *stream, size_t *len_out,
                                        unsigned char *trunc_out, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!d || !term || !num_env || !slot || !len_out || !trunc_out) return -1;
    if (num_env > (size_t)1 << 30 || slot > ((size_t)1 << 30) / num_env) {
        if (err) snprintf(err, errlen, "num_env * slot_rows must be at most 2^30");
        return -1;
    }
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    if (devptr_check(v.device, term, num_env * slot, "terminated_dev", err, errlen) ||
        (trunc && devptr_check(v.device, trunc, num_env * slot, "truncated_dev", err, errlen)))
        return -1;
    UpdState *u = state(d);
    if (pin_reserve(&u->eh, 2 * num_env)) return -2;
    if (const int rc = dev_loop_enter(u, v.stream, (hipStream_t)stream)) return rc;
    hipLaunchKernelGGL(episode_scan_kernel, dim3(cdiv((long)num_env, EPS_WAVES)), dim3(64 * EPS_WAVES), 0, v.stream,
                       term, trunc, (int)num_env, (long)slot, u->eh.dev);
    HCHK(hipGetLastError());
    DSYNC(d);                                          // the one host wait: the pinned results are complete
    for (size_t e = 0; e < num_env; ++e) {
        len_out[e] = (size_t)u->eh.host[2 * e];
        trunc_out[e] = u->eh.host[2 * e + 1] != 0.0;
    }
    return 0;
}

// trpo_dev_set_rollout with (mean, action) = the kept rows of trpo_dev_act (the caller has checked that every
// row 0..n-1 was kept); adv from the host [n], or b's advantages [first, first + n) as trpo_dev_set_rollout_adv
extern "C" int trpo_dev_set_rollout_acted(trpo_dev *d, const double *adv, const trpo_bdev *b, size_t first, char *err,
                                          size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!d || (!adv) == (!b)) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    const size_t n = v.n;
    UpdState *u = state(d);
    const int A = v.net.A, W = 2 * A + 1;
    const char *why = nullptr;
    if (n && (!u->kept || u->kept_cap < n * 2 * (size_t)A)) why = "no kept rows on the device";
    else if (n * (size_t)W > (size_t)0x7fffffff) why = "the rollout is beyond the kernel's indexing";
    else if (b && !b->have_adv) why = "the baseline holds no advantages (trpo_baseline_advantage first)";
    else if (b && b->device != v.device) why = "the baseline is on another HIP device than the context";
    else if (b && (first > b->n || n > b->n - first)) why = "first + n exceeds the baseline's batch";
    if (why) {
        if (err) snprintf(err, errlen, "%s", why);
        return -1;
    }
    HCHK(hipSetDevice(v.device));
    // everything that can fail comes before the rollout is touched
    if (n > u->roll_cap / W || !u->roll) {
        double *nr = nullptr;
        HCHK(trpo_malloc((void **)&nr, sizeof(double) * (n * W ? n * W : 1)));
        if (u->roll) hipFree(u->roll);
        u->roll = nr;
        u->roll_cap = n * W;
        u->have_roll = 0;
    }
    const double *adv_dev = b ? b->adv + first : nullptr;
    if (!b) {
        if (pin_reserve(&u->hst, n + 1)) return -2;
        u->flag_at = 0;                                // export_solve_kernel's flag words are overwritten here
        memcpy(u->hst.host, adv, sizeof(double) * n);
        adv_dev = u->hst.dev;
    }
    if (n) {
        hipLaunchKernelGGL(roll_from_kept_kernel, dim3(cdiv((long)n * W, 256)), dim3(256), 0, v.stream,
                           (const double *)u->kept, adv_dev, (int)n, A, u->roll);
        HCHK(hipGetLastError());
    }
    DSYNC(d);
    u->roll_n = n;
    u->have_roll = 1;
    ++u->roll_gen;
    return 0;
}

// ===========================================================================
// The rollout record: a batch that is acted on the device stays there.  trpo_dev_act with
// keep == 2 fills rec_obs / rec_kept row by row; a commit makes them the context's batch and kept rows --
// the state trpo_dev_set_obs followed by the batched keep = 1 call leaves, without the upload and without
// the second forward pass.  Which rows have been recorded is the host layer's bitmap (trpo_host.c).
// ===========================================================================
extern "C" void trpo_dev_record_drop(trpo_dev *d) {
    if (!d) return;
    UpdState *u = state(d);
    if (u->rec_obs || u->rec_kept) {
        trpo_dev_view v;
        trpo_dev_get_view(d, &v);
        (void)hipSetDevice(v.device);
        if (u->rec_obs) hipFree(u->rec_obs);       // (hipFree waits for the launches that write them)
        if (u->rec_kept) hipFree(u->rec_kept);
    }
    u->rec_obs = u->rec_kept = nullptr;
    u->rec_rows = 0;
}

extern "C" int trpo_dev_record_begin(trpo_dev *d, size_t rows) {
    if (!d || !rows || rows > (size_t)1 << 30) return -1;        // trpo_dev_set_obs's bound on n
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    trpo_dev_record_drop(d);
    UpdState *u = state(d);
    const size_t L0 = v.net.L[0], A2 = 2 * (size_t)v.net.A;
    if (trpo_malloc((void **)&u->rec_obs, sizeof(double) * rows * L0) != hipSuccess ||
        trpo_malloc((void **)&u->rec_kept, sizeof(double) * rows * A2) != hipSuccess) {
        (void)hipGetLastError();
        trpo_dev_record_drop(d);
        return -2;
    }
    u->rec_rows = rows;
    return 0;
}

// The ragged commit's gather: packed sample s of episode e (the last e with off[e] <= s, the binary search of
// baseline_rows_ragged_kernel over the device copy of the offsets) <- record row e * slot + (s - off[e]).  One
// thread per element of the packed observation rows [n][L0] and kept rows [n][A2].
__global__ void record_gather_kernel(const double *__restrict__ rec_obs, const double *__restrict__ rec_kept,
                                     const int *__restrict__ off, int num_ep, long slot, int n, int L0, int A2,
                                     double *__restrict__ obs, double *__restrict__ kept) {
    const int W = L0 + A2;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)n * W) return;
    const int s = (int)(q / W), c = (int)(q % W);
    int lo = 0, hi = num_ep - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    const long r = (long)lo * slot + (s - off[lo]);
    if (c < L0) obs[(long)s * L0 + c] = rec_obs[r * L0 + c];
    else kept[(long)s * A2 + c - L0] = rec_kept[r * A2 + c - L0];
}

extern "C" int trpo_dev_record_commit(trpo_dev *d, size_t num_ep, const size_t *len, size_t slot, size_t n) {
    if (!d) return -1;
    UpdState *u = state(d);
    if (!u->rec_obs || !u->rec_kept || !u->rec_rows) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    const size_t L0 = v.net.L[0], A2 = 2 * (size_t)v.net.A;
    HCHK(hipSetDevice(v.device));
    if (!len) {
        // the record as it stands: the buffers change hands, nothing is copied
        double *ro = u->rec_obs, *rk = u->rec_kept;
        const size_t rows = u->rec_rows;
        u->rec_obs = u->rec_kept = nullptr;
        u->rec_rows = 0;
        const int rc = trpo_dev_set_obs_device(d, ro, rows);
        if (u->kept) hipFree(u->kept);
        u->kept = rk;
        u->kept_cap = rows * A2;
        return rc;
    }
    if (!num_ep || !n || n > (size_t)1 << 30 || num_ep > n || slot > u->rec_rows / num_ep ||
        n * (L0 + A2) > (size_t)0x7fffffff)
        return -1;
    // everything that can fail without a trace comes before the context is touched
    double *po = nullptr, *pk = nullptr;
    const size_t ntab = (size_t)cdiv((long)num_ep, 2);
    if (trpo_malloc((void **)&po, sizeof(double) * n * L0) != hipSuccess ||
        trpo_malloc((void **)&pk, sizeof(double) * n * A2) != hipSuccess ||
        ensure(&u->rec_off, &u->rec_off_cap, ntab, v.stream) || pin_reserve(&u->hst, ntab + 1)) {
        (void)hipGetLastError();
        if (po) hipFree(po);
        if (pk) hipFree(pk);
        return -2;
    }
    u->flag_at = 0;                                    // export_solve_kernel's flag words are overwritten here
    int *t = (int *)u->hst.host;
    size_t at = 0;
    for (size_t e = 0; e < num_ep; ++e) {
        t[e] = (int)at;
        at += len[e];
    }
    if (num_ep & 1) t[num_ep] = 0;                     // the table's last double, whole
    hipLaunchKernelGGL(copy64_kernel, dim3(cdiv((long)ntab, 256)), dim3(256), 0, v.stream,
                       (const double *)u->hst.dev, u->rec_off, (int)ntab);
    hipLaunchKernelGGL(record_gather_kernel, dim3(cdiv((long)(n * (L0 + A2)), 256)), dim3(256), 0, v.stream,
                       (const double *)u->rec_obs, (const double *)u->rec_kept, (const int *)u->rec_off, (int)num_ep,
                       (long)slot, (int)n, (int)L0, (int)A2, po, pk);
    if (hipGetLastError() != hipSuccess) {
        hipFree(po);
        hipFree(pk);
        return -2;
    }
    const int rc = trpo_dev_set_obs_device(d, po, n);  // synchronises the stream: the gather has run
    if (u->kept) hipFree(u->kept);
    u->kept = pk;
    u->kept_cap = n * A2;
    trpo_dev_record_drop(d);
    return rc;
}
