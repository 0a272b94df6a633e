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
//   act_kernel (LDSY)   sample per lane: forward64 on 64-row passes, Y rows in LDS or the ws scratch
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
// The ActNorm instantiations of both forms (the observation filter, trpo_ctx_obsnorm_*) pass every
// observation through the filter's frozen (shift, scale, clip) where it is loaded, so the network and the record
// see the normalised row.  A context without the filter launches none of them.
// On the host side every call of every IO goes through one prologue (act_prologue: the shared refusals and sizes)
// and one launcher (act_launch<IO>: the grid, where the lane form's rows live, the LDS limit, the instantiation);
// trpo_dev_act and trpo_dev_act_dev keep what is theirs -- the form rule, where the rows come from and go to, and
// on which side of the act launch the filter's statistics launch stands.
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
    static constexpr bool dev = false, norm = false;
    static __device__ __forceinline__ void store(double *p, double v) { act_store(p, v); }
};
template <class T_>
struct ActDev {
    using T = T_;
    using Out = ActOutDev<T_>;
    static constexpr bool dev = true, norm = false;
    static __device__ __forceinline__ void store(T_ *p, double v) { *p = (T_)v; }
};
// The observation filter's frozen pair.  One element, exactly: y = (x - shift[k]) * scale[k] as a
// subtraction and a multiplication (never one fma), then fmin(fmax(y, -clip), clip); clip = +inf clips nothing.
// shift and scale are uniform over a launch, like theta.
struct ObsNorm {
    static constexpr bool on = true;
    const double *__restrict__ shift, *__restrict__ scale;
    double clip;
    __device__ __forceinline__ double operator()(double x, int k) const {
#pragma clang fp contract(off)
        const double y = (x - shift[k]) * scale[k];
        return fmin(fmax(y, -clip), clip);
    }
};
// IO = ActNorm<B>: B's rows with the filter applied at the observation load; the pair rides behind B's outputs
template <class B>
struct ActNorm : B {
    static constexpr bool norm = true;
    struct Out : B::Out {
        ObsNorm flt;
    };
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
        if constexpr (IO::norm) forward64(net, T, obs, s, live, Y, roff, tid, O.flt);
        else forward64(net, T, obs, s, live, Y, roff, tid);
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
            double o = live ? (double)obs[(long)s * L0 + k] : 0.0;
            if constexpr (IO::norm)
                if (live) o = O.flt(o, k);
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

// ===========================================================================
// The observation filter (trpo_ctx_obsnorm_*): running per-column moments of the raw observations
// (Welford 1962; batches merged as Chan, Golub and LeVeque 1983) and the (shift, scale) pair derived from them.
// The contract is the public header's.  State, fp64, in one device array on_st for L0 columns:
//   live    [count, mean[L0], M2[L0]]     what the derived pair was computed from
//   pending [count, mean[L0], M2[L0]]     the raw rows of the record calls since the last fold / record_begin
//   derived [shift[L0], scale[L0]]        frozen between folds: the act kernels read nothing else
// The two counts are exact small integers the host knows (every call adds its m), so it passes them to the
// kernels as arguments and the device words are written, never read, by the kernels.
//
// The moments of one call's m rows, column k (obs_stats_kernel), in an order that depends on (values, m) alone:
// rows are cut into chunks of ON_CHUNK = 64 consecutive rows; a chunk's sum is a compensated sum (obs_sum_step)
// over its rows ascending from 0.0; the call's sum is a compensated sum of the chunk sums ascending from 0.0;
// mean_b = sum / m.  Then the same again for M2_b = sum (x - mean_b)^2, the square entering its step's fma
// unrounded.  Two passes over the rows: the squares are of deviations, never of the values.  The compensation is
// there for the merge: d = mean_b - mean_p is a small difference of large means, and a plain sum of 130 rows
// leaves mean_b some ten ulp off, which the d d term of M2 shows to first order (measured on the test's rows,
// offset / spread = 1e5: 3e-12 relative in M2 with plain sums, 5e-13 with these).  One launch: lane <-> column (a wave reads 64 adjacent columns of a row at once), one block per 64
// columns, its waves take the chunks round-robin and leave their sums in the scratch on_part [chunk][L0]; which
// wave summed a chunk does not show in the bits.  No atomics.  Then the merge into pending, by obs_merge below.
// ===========================================================================
constexpr int ON_CHUNK = TRPO_DEV_OBSNORM_CHUNK;    // rows per chunk of the fixed summation order (64)
constexpr int ON_WAVES = 16;                        // waves per block of obs_stats_kernel, at most

// (n_p, mean_p, M2_p) merged with a batch (m, mean_b, M2_b): d = mean_b - mean_p, n = n_p + m,
// mean = mean_p + d (m / n), M2 = M2_p + M2_b + d d (n_p m / n); every operation rounds on its own
__device__ __forceinline__ void obs_merge(double np, double mean_p, double m2_p, double mb, double mean_b, double m2_b,
                                          double &mean, double &m2) {
#pragma clang fp contract(off)
    if (mb == 0.0) {
        mean = mean_p;
        m2 = m2_p;
        return;
    }
    const double n = np + mb, d = mean_b - mean_p;
    mean = mean_p + d * (mb / n);
    m2 = m2_p + m2_b + d * d * (np * mb / n);
}

// one step of a compensated sum (Kahan 1965) of the products a b: e carries what the last addition lost
__device__ __forceinline__ void obs_sum_step(double &s, double &e, double a, double b) {
#pragma clang fp contract(off)
    const double y = fma(a, b, -e), t = s + y;
    e = (t - s) - y;
    s = t;
}

template <class T>
__global__ void __launch_bounds__(64 * ON_WAVES)
obs_stats_kernel(const T *__restrict__ rows, int m, int L0, double np, double *__restrict__ pend, double *part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int k = blockIdx.x * 64 + lane, nch = (m + ON_CHUNK - 1) / ON_CHUNK;
    const bool col = k < L0;
    double mean_b = 0.0;
    // pass 0: the chunk sums of x, then mean_b; pass 1: the chunk sums of (x - mean_b)^2.  Every barrier is
    // reached by every thread: the chunk loop's trip count is wave-uniform and no thread leaves early.
    for (int pass = 0; pass < 2; ++pass) {
        for (int c = w; c < nch; c += nw) {
            const int r0 = c * ON_CHUNK, r1 = r0 + ON_CHUNK < m ? r0 + ON_CHUNK : m;
            double s = 0.0, e = 0.0;
            if (col) {
#pragma unroll 8
                for (int r = r0; r < r1; ++r) {
                    const double x = (double)rows[(long)r * L0 + k], d = x - mean_b;
                    obs_sum_step(s, e, pass == 0 ? x : d, pass == 0 ? 1.0 : d);
                }
                part[(long)c * L0 + k] = s;
            }
        }
        __syncthreads();
        double t = 0.0, e = 0.0;
        if (col && (pass == 0 || w == 0))
            for (int c = 0; c < nch; ++c) obs_sum_step(t, e, part[(long)c * L0 + k], 1.0);
        if (pass == 0) {
            mean_b = t / (double)m;
            __syncthreads();                         // every wave has read the sums before pass 1 overwrites them
        } else if (col && w == 0) {
            double mean, m2;
            obs_merge(np, pend[1 + k], pend[1 + L0 + k], (double)m, mean_b, t, mean, m2);
            pend[1 + k] = mean;
            pend[1 + L0 + k] = m2;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) pend[0] = np + (double)m;
}

// pending into live by obs_merge, the derived pair from the new live moments, pending cleared.  count < 2: the
// identity (shift 0, scale 1); else shift = mean, scale = 1 / (sqrt(M2 / (count - 1)) + eps).
__global__ void obs_fold_kernel(double *__restrict__ st, int L0, double nl, double np, double eps) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, S = 1 + 2 * L0;
    double *live = st, *pend = st + S, *der = st + 2 * S;
    const double n = nl + np;
    if (k == 0) {
        live[0] = n;
        pend[0] = 0.0;
    }
    if (k >= L0) return;
    double mean, m2;
    obs_merge(nl, live[1 + k], live[1 + L0 + k], np, pend[1 + k], pend[1 + L0 + k], mean, m2);
    live[1 + k] = mean;
    live[1 + L0 + k] = m2;
    pend[1 + k] = pend[1 + L0 + k] = 0.0;
    der[k] = n < 2.0 ? 0.0 : mean;
    der[L0 + k] = n < 2.0 ? 1.0 : 1.0 / (sqrt(m2 / (n - 1.0)) + eps);
}

// out = the filter of in, element by element ([rows][L0], T = double or float: widened exactly, rounded once on
// the store); in place when out == in
template <class T>
__global__ void obs_apply_kernel(const T *in, T *out, size_t nel, int L0, ObsNorm flt) {
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nel; q += (size_t)gridDim.x * blockDim.x)
        out[q] = (T)flt((double)in[q], (int)(q % (size_t)L0));
}

static ObsNorm obs_norm_pair(const UpdState *u, int L0) {
    const double *der = u->on_st + 2 * (1 + 2 * (size_t)L0);
    return ObsNorm{der, der + L0, u->on_clip};
}
// out = the filter of in, nel elements of T on the stream
template <class T>
static void obs_apply_launch(const UpdState *u, hipStream_t st, const void *in, void *out, size_t nel, int L0) {
    const size_t nb = (nel + 255) / 256;
    hipLaunchKernelGGL(obs_apply_kernel<T>, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, st, (const T *)in,
                       (T *)out, nel, L0, obs_norm_pair(u, L0));
}

// the chunk sums' scratch for a call of m rows (may allocate: before the streams are tied)
static int obs_stats_reserve(UpdState *u, hipStream_t st, size_t m, int L0) {
    return ensure(&u->on_part, &u->on_part_cap, (size_t)cdiv((long)m, ON_CHUNK) * L0, st);
}
// the raw rows [m][L0] of a record call into the pending moments, on the context's stream
template <class T>
static int obs_stats_launch(UpdState *u, hipStream_t st, const T *rows, size_t m, int L0) {
    if (obs_stats_reserve(u, st, m, L0)) return -2;
    const int nch = cdiv((long)m, ON_CHUNK), nw = nch < ON_WAVES ? nch : ON_WAVES;
    hipLaunchKernelGGL(obs_stats_kernel<T>, dim3(cdiv(L0, 64)), dim3(64 * nw), 0, st, rows, (int)m, L0, u->on_np,
                       u->on_st + 1 + 2 * (size_t)L0, u->on_part);
    HCHK(hipGetLastError());
    u->on_np += (double)m;
    return 0;
}

// pending emptied (trpo_dev_record_begin: a recording that is discarded leaves nothing behind)
static int obs_pending_clear(UpdState *u, hipStream_t st, int L0) {
    HCHK(hipMemsetAsync(u->on_st + 1 + 2 * (size_t)L0, 0, sizeof(double) * (1 + 2 * (size_t)L0), st));
    u->on_np = 0.0;
    return 0;
}

// What trpo_dev_act and trpo_dev_act_dev derive from their arguments before they differ
struct ActPlan {
    int tot, wstride;                // activations per row over all layers; the neuron form's LDS doubles per wave
    size_t nlds;                     // the neuron form's dynamic LDS bytes: AN_WAVES rows
    bool rec;                        // keep == 2: the rows go into the rollout record
    ActRng g;
};
// The refusals both calls share (-1, with the cause in err where there is one to name), the context's device made
// current, the kept buffer of a keep == 1 call (may allocate: -2), the derived sizes and the generator's words.
static int act_prologue(trpo_dev *d, const void *obs, size_t m, unsigned long long seed, unsigned long long step,
                        size_t row0, size_t stride, int keep, int form, const void *mean, const void *action,
                        const void *logp, trpo_dev_view *v, UpdState **up, ActPlan *p, char *err, size_t errlen) {
    if (!d || !obs || !mean || !m || !stride || (!action && (logp || keep))) return -1;
    trpo_dev_get_view(d, v);
    const Net &net = v->net;
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
    HCHK(hipSetDevice(v->device));
    UpdState *u = *up = state(d);
    const bool rec = keep == 2;
    if (rec && (!u->rec_obs || !u->rec_kept)) {
        if (err) snprintf(err, errlen, "no recording in progress");
        return -1;
    }
    if (keep && !rec && ensure(&u->kept, &u->kept_cap, v->n * 2 * (size_t)A, v->stream)) return -2;
    *p = ActPlan{tot, wstride, nlds, rec,
                 ActRng{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)step, (unsigned)(step >> 32) << 16, row0, stride}};
    return 0;
}

// blocks of one launch: one per AN_WAVES rows (neuron) or per UT rows (lane); past ACT_MAXG the blocks take more trips
static int act_grid(bool neuron, size_t m) {
    const int g = cdiv((long)m, neuron ? AN_WAVES : UT);
    return g < ACT_MAXG ? g : ACT_MAXG;
}

static int dev_loop_enter(UpdState *u, hipStream_t own, hipStream_t st);

// The one launch of an act call, on the context's stream, for every IO: the grid (*G: the host path's flag words), the
// lane form's rows in LDS or in the scratch u->ws, the dynamic-LDS limit of this IO's two LDS-row instantiations
// raised at its first lane launch, the instantiation.  Everything that can fail or must allocate comes first; then
// the context's stream is tied behind st, the caller's (NULL on the host path: nothing to tie); then the launch.
template <class IO>
static int act_launch(UpdState *u, const trpo_dev_view &v, const ActPlan &p, bool neuron, const typename IO::T *obs,
                      size_t m, const typename IO::Out &O, hipStream_t st, int *G) {
    constexpr int io = (IO::norm ? 3 : 0) + (IO::dev ? (sizeof(typename IO::T) == sizeof(float) ? 2 : 1) : 0);
    *G = act_grid(neuron, m);
    RowsPlan y;
    if (!neuron) {
        if (act_storage(u, p.tot, *G, v.stream, &y)) return -2;
        HCHK(lds_limit_once(&u->act_lds_set[io], {(const void *)act_kernel<true, false, IO>,
                                                  (const void *)act_kernel<true, true, IO>}));
    }
    if (const int rc = dev_loop_enter(u, v.stream, st)) return rc;
    if (neuron) {
        const auto k = p.rec ? act_neuron_kernel<true, IO> : act_neuron_kernel<false, IO>;
        hipLaunchKernelGGL(k, dim3(*G), dim3(64 * AN_WAVES), p.nlds, v.stream, v.net, v.theta64, obs, (int)m, p.g,
                           p.wstride, O);
    } else {
        const auto k = p.rec ? (y.use_lds ? act_kernel<true, true, IO> : act_kernel<false, true, IO>)
                             : (y.use_lds ? act_kernel<true, false, IO> : act_kernel<false, false, IO>);
        hipLaunchKernelGGL(k, dim3(*G), dim3(UT), y.lds, v.stream, v.net, v.theta64, obs, (int)m, p.g, u->ws, p.tot, O);
    }
    HCHK(hipGetLastError());
    return 0;
}
// B's rows through the filter at the observation load (the ActNorm forms) while the context has one, B's own forms
// otherwise.  B: ActHost, ActDev<double> or ActDev<float>.
template <class B>
static int act_launch_rows(UpdState *u, const trpo_dev_view &v, const ActPlan &p, bool neuron, const typename B::T *obs,
                           size_t m, const typename B::Out &O, hipStream_t st, int *G) {
    if (!u->on_st) return act_launch<B>(u, v, p, neuron, obs, m, O, st, G);
    const typename ActNorm<B>::Out On{O, obs_norm_pair(u, v.net.L[0])};
    return act_launch<ActNorm<B>>(u, v, p, neuron, obs, m, On, st, G);
}

// form: 0 by the measured rule, 1 sample per lane, 2 neuron per lane.  keep: (mean, action) of
// row r_i also into the kept buffer [n][2A] (the caller has checked every r_i < n); keep == 2: obs_i and
// (mean, action) of row r_i into the rollout record instead (every r_i < its rows).  action == NULL: means only.
extern "C" int trpo_dev_act(trpo_dev *d, const double *obs, size_t m, unsigned long long seed, unsigned long long step,
                            size_t row0, size_t stride, int keep, int form, double *mean, double *action,
                            double *logp, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    trpo_dev_view v;
    UpdState *u;
    ActPlan p;
    if (const int rc = act_prologue(d, obs, m, seed, step, row0, stride, keep, form, mean, action, logp, &v, &u, &p, err,
                                    errlen))
        return rc;
    const int A = v.net.A, L0 = v.net.L[0];
    // a batch whose obs and results fit the pinned buffer goes through it; the measured rule
    // (profiles/act_stage.json): the neuron form for those, the lane form for the staged ones
    const size_t nin = m * (size_t)L0, nout = m * (size_t)(action ? 2 * A + 1 : A);
    const bool pinned = nin + nout <= ACT_PIN;
    const bool neuron = form ? form == 2 : (p.nlds <= ACT_NEURON_LDS && pinned);
    if (pin_reserve(&u->ah, ACT_MAXG / 2 + ACT_PIN)) return -2;     // once: the flag words start below any seq
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
    const ActOut O{dout, action ? dout + m * (size_t)A : nullptr, action && logp ? dout + 2 * m * (size_t)A : nullptr,
                   p.rec ? u->rec_kept : (keep ? u->kept : nullptr), p.rec ? u->rec_obs : nullptr,
                   pinned ? (unsigned *)u->ah.dev : nullptr, u->aseq};
    // A record call's raw rows go into the filter's pending moments AHEAD of the act launch: the pinned input is the
    // next call's to overwrite as soon as this launch's flag words are up
    if (u->on_st && p.rec && obs_stats_launch(u, v.stream, (const double *)din, m, L0)) return -2;
    int G;
    if (const int rc = act_launch_rows<ActHost>(u, v, p, neuron, din, m, O, nullptr, &G)) return rc;
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

// the rows of one device call in the caller's arrays of T, the filter's statistics launch of a record call behind
// the act launch, the caller's stream behind both
template <class T>
static int act_dev_rows(UpdState *u, const trpo_dev_view &v, const ActPlan &p, bool neuron, const void *obs, size_t m,
                        int keep, void *mean, void *action, void *logp, hipStream_t st) {
    const int L0 = v.net.L[0];
    const ActOutDev<T> O{(T *)mean, (T *)action, (T *)logp, p.rec ? u->rec_kept : (keep ? u->kept : nullptr),
                         p.rec ? u->rec_obs : nullptr};
    // the chunk sums' scratch too is there before the launcher ties the streams
    if (u->on_st && p.rec && obs_stats_reserve(u, v.stream, m, L0)) return -2;
    int G;
    if (const int rc = act_launch_rows<ActDev<T>>(u, v, p, neuron, (const T *)obs, m, O, st, &G)) return rc;
    // a record call's raw rows go into the pending moments behind the act launch
    if (u->on_st && p.rec && obs_stats_launch(u, v.stream, (const T *)obs, m, L0)) return -2;
    return dev_loop_leave(u, v.stream, st);
}

// trpo_dev_act on the caller's device arrays (element type by dtype: 0 double, 1 float), asynchronous: returns
// once the launch is enqueued.  keep and form as trpo_dev_act's.  The form rule of these calls is their own:
// the host rule was measured over the link (profiles/device_loop.md).
extern "C" int trpo_dev_act_dev(trpo_dev *d, const void *obs, size_t m, unsigned long long seed,
                                unsigned long long step, size_t row0, size_t stride, int keep, int form, int dtype,
                                void *mean, void *action, void *logp, void *stream, char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (dtype != 0 && dtype != 1) return -1;
    trpo_dev_view v;
    UpdState *u;
    ActPlan p;
    if (const int rc = act_prologue(d, obs, m, seed, step, row0, stride, keep, form, mean, action, logp, &v, &u, &p, err,
                                    errlen))
        return rc;
    const size_t A = v.net.A, L0 = v.net.L[0], es = dtype ? sizeof(float) : sizeof(double);
    if (devptr_check(v.device, obs, es * m * L0, "obs_dev", err, errlen) ||
        devptr_check(v.device, mean, es * m * A, "mean_dev", err, errlen) ||
        (action && devptr_check(v.device, action, es * m * A, "action_dev", err, errlen)) ||
        (logp && devptr_check(v.device, logp, es * m, "logp_dev", err, errlen)))
        return -1;
    // the rule for device rows, measured (profiles/device_loop.md): one wave per row won at every
    // size up to 4 096 rows on all three nets, the lane form at 50 000; the lane form from 64 rows per CU on
    const bool neuron = form ? form == 2 : (p.nlds <= ACT_NEURON_LDS && m < ACT_DEV_LANE_FROM);
    return dtype ? act_dev_rows<float>(u, v, p, neuron, obs, m, keep, mean, action, logp, (hipStream_t)stream)
                 : act_dev_rows<double>(u, v, p, neuron, obs, m, keep, mean, action, logp, (hipStream_t)stream);
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
    if (u->on_st && obs_pending_clear(u, v.stream, (int)L0)) return -2;    // the filter's pending moments start over
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

// ===========================================================================
// The observation filter's calls (kernels and state layout above, by obs_stats_kernel).  Everything is enqueued
// on the context's stream; get and the host-pointer apply wait for it.
// ===========================================================================
extern "C" int trpo_dev_obsnorm_enabled(trpo_dev *d) { return d && state(d)->on_st != nullptr; }

static int obs_fold_launch(UpdState *u, hipStream_t st, int L0) {
    hipLaunchKernelGGL(obs_fold_kernel, dim3(cdiv(L0, 256)), dim3(256), 0, st, u->on_st, L0, u->on_nl, u->on_np,
                       u->on_eps);
    HCHK(hipGetLastError());
    u->on_nl += u->on_np;
    u->on_np = 0.0;
    return 0;
}

// empty moments, the identity pair; a second call starts over
extern "C" int trpo_dev_obsnorm_enable(trpo_dev *d, double clip, double eps) {
    if (!d) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    UpdState *u = state(d);
    const int L0 = v.net.L[0];
    const size_t cnt = 2 * (1 + 2 * (size_t)L0) + 2 * (size_t)L0;
    if (!u->on_st) HCHK(trpo_malloc((void **)&u->on_st, sizeof(double) * cnt));
    HCHK(hipMemsetAsync(u->on_st, 0, sizeof(double) * cnt, v.stream));
    u->on_clip = clip;
    u->on_eps = eps;
    u->on_nl = u->on_np = 0.0;
    return obs_fold_launch(u, v.stream, L0);
}

extern "C" int trpo_dev_obsnorm_disable(trpo_dev *d) {
    if (!d) return -1;
    UpdState *u = state(d);
    if (!u->on_st) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    HCHK(hipFree(u->on_st));                           // (waits for the launches that read it)
    u->on_st = nullptr;
    return 0;
}

extern "C" int trpo_dev_obsnorm_fold(trpo_dev *d) {
    if (!d || !state(d)->on_st) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    return obs_fold_launch(state(d), v.stream, v.net.L[0]);
}

// which: 0 live (shift / scale may be asked for), 1 pending; any output may be NULL
extern "C" int trpo_dev_obsnorm_get(trpo_dev *d, int which, double *count, double *mean, double *m2, double *shift,
                                    double *scale) {
    if (!d || !state(d)->on_st || (which != 0 && which != 1) || (which && (shift || scale))) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    DSYNC(d);
    const UpdState *u = state(d);
    const size_t L0 = v.net.L[0], S = 1 + 2 * L0;
    const double *at = u->on_st + (which ? S : 0), *der = u->on_st + 2 * S;
    if (count) HCHK(hipMemcpy(count, at, sizeof(double), hipMemcpyDeviceToHost));
    if (mean) HCHK(hipMemcpy(mean, at + 1, sizeof(double) * L0, hipMemcpyDeviceToHost));
    if (m2) HCHK(hipMemcpy(m2, at + 1 + L0, sizeof(double) * L0, hipMemcpyDeviceToHost));
    if (shift) HCHK(hipMemcpy(shift, der, sizeof(double) * L0, hipMemcpyDeviceToHost));
    if (scale) HCHK(hipMemcpy(scale, der + L0, sizeof(double) * L0, hipMemcpyDeviceToHost));
    return 0;
}

// live = (count, mean, m2) as given (the caller has checked them), pending emptied, the pair derived anew; enqueued
extern "C" int trpo_dev_obsnorm_set(trpo_dev *d, double count, const double *mean, const double *m2) {
    if (!d || !state(d)->on_st || !mean || !m2) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    UpdState *u = state(d);
    const size_t L0 = v.net.L[0];
    // through a pinned staging buffer and a copy kernel on the stream: the host does not wait -- except for the
    // copy of an earlier set that has not run yet, which still reads the buffer
    if (u->on_set_ev) HCHK(hipEventSynchronize(u->on_set_ev));
    else HCHK(hipEventCreateWithFlags(&u->on_set_ev, hipEventDisableTiming));
    if (pin_reserve(&u->onh, 2 * L0)) return -2;
    memcpy(u->onh.host, mean, sizeof(double) * L0);
    memcpy(u->onh.host + L0, m2, sizeof(double) * L0);
    hipLaunchKernelGGL(copy64_kernel, dim3(cdiv((long)(2 * L0), 256)), dim3(256), 0, v.stream,
                       (const double *)u->onh.dev, u->on_st + 1, (int)(2 * L0));
    HCHK(hipGetLastError());
    HCHK(hipEventRecord(u->on_set_ev, v.stream));
    if (obs_pending_clear(u, v.stream, (int)L0)) return -2;
    u->on_nl = count;
    return obs_fold_launch(u, v.stream, (int)L0);
}

// out [m][L0] = the filter of in [m][L0], host rows; synchronous
extern "C" int trpo_dev_obsnorm_apply(trpo_dev *d, const double *in, size_t m, double *out) {
    if (!d || !state(d)->on_st || !in || !out || !m) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    UpdState *u = state(d);
    const int L0 = v.net.L[0];
    const size_t nel = m * (size_t)L0;
    if (ensure(&u->aobs, &u->aobs_cap, nel, v.stream)) return -2;
    HCHK(hipMemcpyAsync(u->aobs, in, sizeof(double) * nel, hipMemcpyHostToDevice, v.stream));
    obs_apply_launch<double>(u, v.stream, u->aobs, u->aobs, nel, L0);
    HCHK(hipGetLastError());
    HCHK(hipMemcpyAsync(out, u->aobs, sizeof(double) * nel, hipMemcpyDeviceToHost, v.stream));
    DSYNC(d);
    return 0;
}

// the same on the caller's device arrays of dtype (0 double, 1 float), in place when out == in; asynchronous,
// ordered against `stream` as the act calls are
extern "C" int trpo_dev_obsnorm_apply_dev(trpo_dev *d, const void *in, size_t m, int dtype, void *out, void *stream,
                                          char *err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!d || !state(d)->on_st || !in || !out || !m || (dtype != 0 && dtype != 1)) return -1;
    trpo_dev_view v;
    trpo_dev_get_view(d, &v);
    HCHK(hipSetDevice(v.device));
    UpdState *u = state(d);
    const int L0 = v.net.L[0];
    const size_t nel = m * (size_t)L0, es = dtype ? sizeof(float) : sizeof(double);
    if (devptr_check(v.device, in, es * nel, "in_dev", err, errlen) ||
        devptr_check(v.device, out, es * nel, "out_dev", err, errlen))
        return -1;
    if (const int rc = dev_loop_enter(u, v.stream, (hipStream_t)stream)) return rc;
    if (dtype) obs_apply_launch<float>(u, v.stream, in, out, nel, L0);
    else obs_apply_launch<double>(u, v.stream, in, out, nel, L0);
    HCHK(hipGetLastError());
    return dev_loop_leave(u, v.stream, (hipStream_t)stream);
}
