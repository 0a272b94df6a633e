// upd_vfit.h -- section of trpo_update.hip: the trust-region value fit on the baseline object.

// ===========================================================================
// Trust-region fit of the value baseline on the device (Schulman et al. 2016, GAE, section 5; no reference
// counterpart): with j_s = grad_phi V_phi(s), N = the object's samples, y its target, all fp64,
//   L(phi) = (1/N) sum (V - y)^2,  sigma^2 = L(phi_old),  g = (1/N) sum (V_old - y) j_s,
//   H v    = (1/N) sum j_s (j_s . v) + lambda v                      (Gauss-Newton, damping lambda)
//   CG on H s = -g from s = 0 (at most K iterations, stop once r.r < th),  q = s . H s,
//   alpha_tr = sqrt(2 eps sigma^2 / q), alpha0 = min(1, alpha_tr),  candidates phi + alpha0 0.5^k s.
// Launch sequence of one fit (fixed by K; the host waits once, with hipStreamSynchronize, at its end):
//   copy phi in | first pass (g, sigma^2, V_old) | slab sum, init | K x (product, slab sum, CG step) | product of s |
//   scale | candidates | slab sum, select.
// Once r.r < th the remaining products and steps return at once on the device flag ctl[0]; a sigma^2 that is
// zero or not finite sets ctl[1], on which everything behind the init returns and the select hands phi back.
// Every cross-sample sum is slabs summed in block order, every dot product the fixed tree of vfit_block_sum:
// the same inputs give the same bits on every call.
// ===========================================================================
enum { VSC_RR = 0, VSC_SIG2, VSC_ALPHA0, VSC_ALPHATR, VSC_Q, VSC_GNORM, VSC_N };
// the pinned result block behind x_out [PA] and s [PA]
enum { VI_LOSS0 = 0, VI_GNORM, VI_SHS, VI_ALPHATR, VI_ALPHA0, VI_ITERS, VI_ACCEPTED, VI_BAD, VI_LOSS,
       VI_SHIFT = VI_LOSS + 32, VI_RDOTR = VI_SHIFT + 32, VI_N = VI_RDOTR + TRPO_BDEV_VFIT_MAX_CG + 1 };
static_assert(VI_N == TRPO_BDEV_VFIT_INFO, "the fit's result block is what trpo_dev.h announces");
constexpr int VF_T = 1024;                 // threads of the one-workgroup kernels
constexpr int VF_CS = 64;                  // candidate slab: {sum (V_k - y)^2, sum (V_k - V_old)^2} x 32

__device__ __forceinline__ bool vfit_skip(const int *__restrict__ ctl, int mask) {
    return ((mask & 1) && ctl[0]) || ((mask & 2) && ctl[1]);
}

// Gauss-Newton product (or, FIRST, the fit's first pass) in the lane form of baseline_lane_kernel: per
// sample the forward pass, then the tangent forward with v (bias first, inputs ascending; the weight term
// before the v term at each input) to the scalar j.v, then the backward sweep seeded with j.v.  The last
// accumulator holds sum (j.v)^2, so v.Hv comes from the same pass and cannot be negative.  FIRST: the seed
// is d = V - y, the last accumulator sum d^2, and V goes to vold.  phi and v come from device memory.
template <bool FIRST>
__global__ void __launch_bounds__(256)
vfit_lane_kernel(Net net, const double *__restrict__ phi, const double *__restrict__ v,
                 const double *__restrict__ obs, const double *__restrict__ target, int n, double *__restrict__ slabs,
                 double *__restrict__ vold, const int *__restrict__ ctl, int mask) {
    __shared__ double tl[BL_PA_MAX + 1], tv[BL_PA_MAX + 1];
    __shared__ double acc[16][BLK_NE][16];
    if (vfit_skip(ctl, mask)) return;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, base = lane & ~15;
    const int gi = tid >> 4;
    const LaneNet c = lane_net(net);
    for (int q = tid; q < c.PA; q += 256) {
        tl[q] = phi[q];
        if constexpr (!FIRST) tv[q] = v[q];
    }
    __syncthreads();
    LaneSums S;
    lane_zero(S);
    const int ngroups = gridDim.x * 16;
    for (int s = blockIdx.x * 16 + gi; s < n; s += ngroups) {
        LaneAct A;
        lane_forward(c, tl, obs, s, j, base, A);
        double seed;
        if constexpr (FIRST) {
            seed = A.y3 - target[s];
            if (j == 0) vold[s] = A.y3;
        } else {
            double t = lane_dot(j < c.L1 ? tv[c.B0 + j] : 0.0, c.L0, A.xk,
                                [&](int k) { return j < c.L1 ? tv[c.W0 + k * c.L1 + j] : 0.0; });
            const double r1 = j < c.L1 ? act_d64(c.a1, A.y1, t) : 0.0;
            double rk[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) rk[k] = __shfl(r1, base + k, 64);
            t = lane_dot2(j < c.L2 ? tv[c.B1 + j] : 0.0, c.L1, rk,
                          [&](int k) { return j < c.L2 ? tl[c.W1 + k * c.L2 + j] : 0.0; }, A.y1k,
                          [&](int k) { return j < c.L2 ? tv[c.W1 + k * c.L2 + j] : 0.0; });
            const double r2 = j < c.L2 ? act_d64(c.a2, A.y2, t) : 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) rk[k] = __shfl(r2, base + k, 64);
            t = lane_dot2(tv[c.B2], c.L2, rk, [&](int k) { return tl[c.W2 + k]; }, A.y2k,
                          [&](int k) { return tv[c.W2 + k]; });
            seed = act_d64(c.a3, A.y3, t);             // j.v
        }
        double g1, g2, g3;
        lane_backward(c, tl, A, seed, j, base, g1, g2, g3);
        lane_add(S, A, g1, g2, g3, seed * seed);
    }
    lane_slab(c, S, acc, gi, j, tid, net.P, slabs + (long)blockIdx.x * (net.P + 1));
}

// The same for any depth and widths, one sample per lane, on baseline_kernel's plan: tangent rows (T0 ..)
// behind the activation rows, the gradient rows and the two scalar rows of Y; Y in LDS (LDSY) or in ws, phi
// and v staged in LDS behind it (THL) when they fit too.  first != 0: the first pass (seed d, V to vold).
template <bool LDSY, bool THL>
__global__ void __launch_bounds__(UT)
vfit_kernel(Net net, const double *__restrict__ phig, const double *__restrict__ vg, const double *__restrict__ obs,
            const double *__restrict__ target, int n, double *ws, int rows, double *__restrict__ slabs,
            double *__restrict__ vold, int first, const int *__restrict__ ctl, int mask) {
    extern __shared__ double lds64[];
    if (vfit_skip(ctl, mask)) return;
    const int tid = threadIdx.x;
    double *Y = LDSY ? lds64 : ws + (long)blockIdx.x * rows * RS;
    const double *th = phig, *tv = vg;
    const int PA = net.P - net.A;
    if constexpr (LDSY && THL) {
        double *tl = lds64 + rows * RS;
        for (int q = tid; q < PA; q += UT) {
            tl[q] = phig[q];
            tl[PA + q] = first ? 0.0 : vg[q];
        }
        __syncthreads();
        th = tl;
        tv = tl + PA;
    }
    int roff[MAXL + 1];
    row_offsets(net, roff);
    const int tot = roff[net.nl], P = net.P, last = net.nl - 1;
    const int G0 = tot, GL = 2 * tot, T0 = 2 * tot + 2;
    int goff[MAXL];
    for (int i = 0; i + 1 < net.nl; ++i) goff[i] = G0 + roff[i + 1];
    double *slab = slabs + (long)blockIdx.x * (P + 1);
    const ThetaPlain T{th};
    for (int q = tid; q <= P; q += UT) slab[q] = 0.0;
    const int npass = (n + UT - 1) / UT;
    for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        const int s = pass * UT + tid;
        const bool live = s < n;
        forward64(net, T, obs, s, live, Y, roff, tid);
        double seed;
        if (first) {
            const double y = Y[roff[last] * RS + tid];
            seed = live ? y - target[s] : 0.0;
            if (live) vold[s] = y;
        } else {
            // tangent forward: R x_j = v_b[j] + sum_k (R y_k W[k][j] + y_k v_W[k][j]), R y_j = act'(x_j) R x_j
            for (int i = 0; i + 1 < net.nl; ++i) {
                const int in = net.L[i], out = net.L[i + 1], a = net.act[i + 1];
                const int wo = net.woff[i], bo = net.boff[i];
                for (int j = 0; j < out; ++j) {
                    double t = tv[bo + j];
                    for (int k = 0; k < in; ++k) {
                        if (i > 0) t += Y[(T0 + roff[i] + k) * RS + tid] * th[wo + k * out + j];
                        t += Y[(roff[i] + k) * RS + tid] * tv[wo + k * out + j];
                    }
                    Y[(T0 + roff[i + 1] + j) * RS + tid] = act_d64(a, Y[(roff[i + 1] + j) * RS + tid], t);
                }
            }
            seed = live ? Y[(T0 + roff[last]) * RS + tid] : 0.0;
        }
        Y[(G0 + roff[last]) * RS + tid] = seed;
        Y[GL * RS + tid] = seed * seed;
        Y[(GL + 1) * RS + tid] = 0.0;
        backward64(net, th, Y, roff, G0, tid);
        __syncthreads();
        contract_pass(net, Y, roff, goff, GL, slab, tid);
        __syncthreads();
    }
}

// column q of G slabs of `len` entries in block order: four interleaved chains (blocks b mod 4), then the tail
__device__ __forceinline__ double vfit_col_sum(const double *__restrict__ slabs, int G, int len, int q) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int b = 0;
    for (; b + 4 <= G; b += 4) {
        a0 += slabs[(long)b * len + q];
        a1 += slabs[(long)(b + 1) * len + q];
        a2 += slabs[(long)(b + 2) * len + q];
        a3 += slabs[(long)(b + 3) * len + q];
    }
    double t = (a0 + a1) + (a2 + a3);
    for (; b < G; ++b) t += slabs[(long)b * len + q];
    return t;
}
// the workgroup's sum of v in a fixed order (xor tree in a wave, the waves in order), in every thread
__device__ __forceinline__ double vfit_block_sum(double v, double *wpart) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                   // wpart's previous readers are done
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < VF_T / 64; ++w) t += wpart[w];
    return t;
}

// one column of the slabs: block b to thread b mod 1024, then vfit_block_sum's tree
__device__ __forceinline__ double vfit_one_col(const double *__restrict__ slabs, int G, int len, int q, double *wpart) {
    double v = 0.0;
    for (int b = threadIdx.x; b < G; b += VF_T) v += slabs[(long)b * len + q];
    return vfit_block_sum(v, wpart);
}

// The slabs are summed by sum_slabs64_kernel in a launch of its own before each of the one-workgroup kernels
// (cs = the column sums): one workgroup reading 188 slabs of 563 doubles is bound by its compute unit's load
// path (~10 of the 16-18 us these kernels took with the sum inside), 36 workgroups are not, and a launch
// boundary on one stream costs ~0.5 us here.
// after the first pass: g = slab sum / N, sigma^2, r = p = -g, s = 0, r.r; the flags
__global__ void __launch_bounds__(VF_T)
vfit_init_kernel(int PA, double N, double *__restrict__ g, double *__restrict__ s, double *__restrict__ r,
                 double *__restrict__ p, const double *__restrict__ cs,
                 double *__restrict__ sc, int *__restrict__ ctl, double *__restrict__ info) {
    __shared__ double wpart[VF_T / 64];
    const int tid = threadIdx.x;
    const double *__restrict__ sum = cs;               // the slabs' column sums (sum_slabs64_kernel, the launch before)
    double rr = 0.0;
    for (int q = tid; q < PA; q += VF_T) {
        const double gq = sum[q] / N;
        g[q] = gq;
        s[q] = 0.0;
        r[q] = -gq;
        p[q] = -gq;
        rr += gq * gq;
    }
    rr = vfit_block_sum(rr, wpart);
    if (tid == 0) {
        const double sig2 = sum[PA] / N;
        const int bad = !(sig2 > 0.0) || isinf(sig2);
        sc[VSC_RR] = rr;
        sc[VSC_SIG2] = sig2;
        sc[VSC_GNORM] = sqrt(rr);
        ctl[0] = bad || !(rr > 0.0);                   // nothing to solve: no iteration runs
        ctl[1] = bad;
        ctl[2] = 0;
        info[VI_LOSS0] = sig2;
        info[VI_GNORM] = sqrt(rr);
        info[VI_RDOTR] = rr;
    }
}

// one CG iteration behind the product of p: z = slab sum / N + lambda p, p.z = sum (j.p)^2 / N + lambda p.p,
// a = r.r / p.z, s += a p, r -= a z, the new r.r -> rdotr[i + 1]; below th the flag, else p = r + beta p
__global__ void __launch_bounds__(VF_T)
vfit_step_kernel(int PA, double N, double lambda, double th, int it, double *__restrict__ s, double *__restrict__ r,
                 double *__restrict__ p, double *__restrict__ z, const double *__restrict__ cs,
                 double *__restrict__ sc, int *__restrict__ ctl, double *__restrict__ info) {
    __shared__ double wpart[VF_T / 64];
    const int tid = threadIdx.x;
    // each thread's first element stays in registers
    const double rr = sc[VSC_RR];
    const bool own = tid < PA;
    const double p0 = own ? p[tid] : 0.0, r0 = own ? r[tid] : 0.0, s0 = own ? s[tid] : 0.0;
    if (ctl[0]) return;
    const double *__restrict__ sum = cs;               // the slabs' column sums (sum_slabs64_kernel, the launch before)
    double pp = 0.0, z0 = 0.0;
    for (int q = tid; q < PA; q += VF_T) {
        const double pq = q == tid ? p0 : p[q];
        const double zq = sum[q] / N + lambda * pq;
        if (q == tid) z0 = zq;
        else z[q] = zq;
        pp += pq * pq;
    }
    pp = vfit_block_sum(pp, wpart);
    const double pz = sum[PA] / N + lambda * pp;
    if (!(pz > 0.0)) {                                 // p in H's null space (lambda = 0): stop where we are
        __syncthreads();
        if (tid == 0) ctl[0] = 1;
        return;
    }
    const double a = rr / pz;
    double rn = 0.0, r1 = 0.0;
    for (int q = tid; q < PA; q += VF_T) {
        const bool f = q == tid;
        const double pq = f ? p0 : p[q];
        s[q] = (f ? s0 : s[q]) + a * pq;
        const double rq = (f ? r0 : r[q]) - a * (f ? z0 : z[q]);
        if (f) r1 = rq;
        r[q] = rq;
        rn += rq * rq;
    }
    rn = vfit_block_sum(rn, wpart);
    const bool stop = rn < th;
    if (!stop) {
        const double beta = rn / rr;
        for (int q = tid; q < PA; q += VF_T) p[q] = q == tid ? r1 + beta * p0 : r[q] + beta * p[q];
    }
    if (tid == 0) {
        sc[VSC_RR] = rn;
        ctl[2] = it + 1;
        if (stop) ctl[0] = 1;
        info[VI_RDOTR + it + 1] = rn;
    }
}

// behind the product of s: q = s.Hs, alpha_tr = sqrt(2 eps sigma^2 / q), alpha0 = min(1, alpha_tr)
__global__ void __launch_bounds__(VF_T)
vfit_scale_kernel(const double *__restrict__ slabs, int G, int PA, int len, double N, double lambda, double eps,
                  const double *__restrict__ s, double *__restrict__ sc, const int *__restrict__ ctl,
                  double *__restrict__ info) {
    __shared__ double wpart[VF_T / 64];
    if (ctl[1]) return;
    double ss = 0.0;
    for (int q = threadIdx.x; q < PA; q += VF_T) ss += s[q] * s[q];
    ss = vfit_block_sum(ss, wpart);
    const double jj = vfit_one_col(slabs, G, len, PA, wpart);
    if (threadIdx.x == 0) {
        const double q = jj / N + lambda * ss;
        const double atr = sqrt(2.0 * eps * sc[VSC_SIG2] / q);     // q = 0 (s = 0): infinite, alpha0 = 1
        const double a0 = atr < 1.0 ? atr : 1.0;
        sc[VSC_Q] = q;
        sc[VSC_ALPHATR] = atr;
        sc[VSC_ALPHA0] = a0;
        info[VI_SHS] = 0.5 * q;
        info[VI_ALPHATR] = atr;
        info[VI_ALPHA0] = a0;
    }
}

// All nk candidates phi + alpha0 0.5^k s, forward only, lane form: VF_CB candidates' weights at a time go to
// LDS (phi and s are read from device memory once), and every group runs its samples through them; sum
// (V_k - y)^2 and sum (V_k - V_old)^2 per group in sample order, the groups in group order into the block's
// candidate slab.
constexpr int VF_CB = 8;
__global__ void __launch_bounds__(256)
vfit_cand_lane_kernel(Net net, const double *__restrict__ phi, const double *__restrict__ st,
                      const double *__restrict__ sc, int nk, const double *__restrict__ obs,
                      const double *__restrict__ target, const double *__restrict__ vold, int n,
                      double *__restrict__ cslabs, const int *__restrict__ ctl) {
    __shared__ double tl[VF_CB][BL_PA_MAX + 1];
    __shared__ double red[16][VF_CS];
    if (ctl[1]) return;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, base = lane & ~15;
    const int gi = tid >> 4;
    const LaneNet c = lane_net(net);
    const double a0 = sc[VSC_ALPHA0];
    const int ngroups = gridDim.x * 16;
    for (int k0 = 0; k0 < nk; k0 += VF_CB) {
        const int kb = nk - k0 < VF_CB ? nk - k0 : VF_CB;
        __syncthreads();                               // the previous batch's readers of tl are done
        for (int q = tid; q < c.PA; q += 256) {
            const double pq = phi[q], sq = st[q];
            for (int k = 0; k < kb; ++k) tl[k][q] = pq + ldexp(a0, -(k0 + k)) * sq;
        }
        __syncthreads();
        double e0[VF_CB], e1[VF_CB];
#pragma unroll
        for (int k = 0; k < VF_CB; ++k) e0[k] = e1[k] = 0.0;
        for (int s = blockIdx.x * 16 + gi; s < n; s += ngroups) {
            const double y = target[s], v0 = vold[s];
#pragma unroll
            for (int k = 0; k < VF_CB; ++k) {
                if (k < kb) {
                    LaneAct A;
                    lane_forward(c, tl[k], obs, s, j, base, A);
                    const double d = A.y3 - y, w = A.y3 - v0;
                    e0[k] += d * d;
                    e1[k] += w * w;
                }
            }
        }
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < VF_CB; ++k)
                if (k < kb) {
                    red[gi][2 * (k0 + k)] = e0[k];
                    red[gi][2 * (k0 + k) + 1] = e1[k];
                }
        }
    }
    __syncthreads();
    if (tid < 2 * nk) {
        double t = 0.0;
        for (int g = 0; g < 16; ++g) t += red[g][tid];
        cslabs[(long)blockIdx.x * VF_CS + tid] = t;
    }
}

// the same for any depth and widths, one sample per lane (baseline_predict_kernel's pass with the
// candidate's weights formed on the fly); lanes in the xor tree's order, passes in order
template <bool LDSY>
__global__ void __launch_bounds__(UT)
vfit_cand_kernel(Net net, const double *__restrict__ phi, const double *__restrict__ st, const double *__restrict__ sc,
                 int nk, const double *__restrict__ obs, const double *__restrict__ target,
                 const double *__restrict__ vold, int n, double *ws, int rows, double *__restrict__ cslabs,
                 const int *__restrict__ ctl) {
    extern __shared__ double lds64[];
    if (ctl[1]) return;
    const int tid = threadIdx.x;
    double *Y = LDSY ? lds64 : ws + (long)blockIdx.x * rows * RS;
    int roff[MAXL + 1];
    row_offsets(net, roff);
    const int last = net.nl - 1;
    const double a0 = sc[VSC_ALPHA0];
    const int npass = (n + UT - 1) / UT;
    for (int k = 0; k < nk; ++k) {
        const ThetaStep T{phi, st, ldexp(a0, -k)};
        double e0 = 0.0, e1 = 0.0;
        for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
            const int s = pass * UT + tid;
            const bool live = s < n;
            forward64(net, T, obs, s, live, Y, roff, tid);
            const double y = Y[roff[last] * RS + tid];
            const double d = live ? y - target[s] : 0.0, w = live ? y - vold[s] : 0.0;
            e0 += d * d;
            e1 += w * w;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            e0 += __shfl_xor(e0, off, 64);
            e1 += __shfl_xor(e1, off, 64);
        }
        if (tid == 0) {
            cslabs[(long)blockIdx.x * VF_CS + 2 * k] = e0;
            cslabs[(long)blockIdx.x * VF_CS + 2 * k + 1] = e1;
        }
    }
}

// loss[k], shift[k] from the candidate slabs in block order; the first k with loss[k] < loss_before and
// shift[k] <= cap; x_out = that candidate (the weights its forward pass used) or phi itself, s and the rest
// of the result block into pinned memory
__global__ void __launch_bounds__(VF_T)
vfit_select_kernel(int nk, double N, double cap, int PA, const double *__restrict__ phi,
                   const double *__restrict__ s, const double *__restrict__ cs,
                   const double *__restrict__ sc, const int *__restrict__ ctl, double *__restrict__ out) {
    __shared__ double ls[2 * 32];
    __shared__ int acc_s;
    const int tid = threadIdx.x, bad = ctl[1];
    double *info = out + 2 * PA;
    const double sig2 = sc[VSC_SIG2];
    const double a0 = sc[VSC_ALPHA0];
    const bool own = tid < PA;
    const double ph0 = own ? phi[tid] : 0.0, s0 = own ? s[tid] : 0.0;
    const int iters = ctl[2];
    const double *__restrict__ sum = cs;               // the candidate slabs' column sums
    if (!bad && tid < 2 * nk) {
        const double t = sum[tid] / N;
        ls[tid] = (tid & 1) ? t / (2.0 * sig2) : t;
        info[(tid & 1 ? VI_SHIFT : VI_LOSS) + (tid >> 1)] = ls[tid];
    }
    __syncthreads();
    if (tid == 0) {
        int k = -1;
        if (!bad)
            for (int i = 0; i < nk && k < 0; ++i)
                if (ls[2 * i] < sig2 && ls[2 * i + 1] <= cap) k = i;
        acc_s = k;
        info[VI_ACCEPTED] = (double)k;
        info[VI_ITERS] = (double)iters;
        info[VI_BAD] = (double)bad;
    }
    __syncthreads();
    const int k = acc_s;
    const double sf = k < 0 ? 0.0 : ldexp(a0, -k);
    for (int q = tid; q < PA; q += VF_T) {
        const double pq = q == tid ? ph0 : phi[q], sq = q == tid ? s0 : s[q];
        out[q] = k < 0 ? pq : pq + sf * sq;
        out[PA + q] = bad ? 0.0 : sq;
    }
}

// trpo_bdev_gnvp's result: out = slab sum / N + lambda v into pinned memory
__global__ void __launch_bounds__(256)
vfit_gnvp_out_kernel(const double *__restrict__ slabs, int G, int PA, int len, double N, double lambda,
                     const double *__restrict__ v, double *__restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < PA) out[q] = vfit_col_sum(slabs, G, len, q) / N + lambda * v[q];
}

// device vectors of the fit: phi, v, g, s, r, p, z [PA each], the column sums, the scalars, the flag words, V_old
static size_t vfit_vec(const trpo_bdev *b, int i) { return (size_t)i * (b->net.P - b->net.A); }
// slot 7: the column sums of the one-workgroup kernels (P + 1, or the candidates' 64); then the scalars
static size_t vfit_sc_off(const trpo_bdev *b) { return 8 * (size_t)(b->net.P - b->net.A) + 72; }
static int vfit_lane(const trpo_bdev *b) { return b->lane_ok && b->net.P - b->net.A <= BL_PA_MAX; }

// vfit_kernel's rows (Y, the tangent and the gradient rows of the product) and where they live, phi and v behind them
static int vfit_rows(const Net &net) { return rows_for(net, false) * 3 + 2; }
static RowsPlan vfit_plan(const Net &net) { return rows_plan(vfit_rows(net), 2 * (size_t)(net.P - net.A)); }
// vfit_cand_kernel's: the forward rows, the candidate's weights formed on the fly from global memory
static RowsPlan vfit_cand_plan(const Net &net) { return rows_plan(rows_for(net, false)); }

// trpo_bdev_kernel_name's text, from the plans the launches use: "eval=F predict=F gnvp=F cand=F", F = lane
// (the lane kernels), lds+theta, lds, scratch (the forms of the one-sample-per-lane kernels, ROWS_FORM)
static const char *rows_form_name(const RowsPlan &p) {
    return p.theta_lds ? "lds+theta" : (p.use_lds ? "lds" : "scratch");
}
static void bdev_name(trpo_bdev *b) {
    const int lane = vfit_lane(b);
    snprintf(b->name, sizeof b->name, "eval=%s predict=%s gnvp=%s cand=%s", lane ? "lane" : rows_form_name(b->y),
             rows_form_name(predict_plan(b)), lane ? "lane" : rows_form_name(vfit_plan(b->net)),
             lane ? "lane" : (vfit_cand_plan(b->net).use_lds ? "lds" : "scratch"));
}
extern "C" const char *trpo_bdev_kernel_name(const trpo_bdev *b) { return b ? b->name : ""; }

static int vfit_reserve(trpo_bdev *b) {
    const Net &net = b->net;
    const size_t PA = net.P - net.A;
    HCHK(hipSetDevice(b->device));
    if (ensure(&b->vf, &b->vf_cap, vfit_sc_off(b) + VSC_N + 4 + b->n, b->stream)) return -2;
    const int G = vfit_lane(b) ? b->Gl : b->G;
    if (ensure(&b->vcs, &b->vcs_cap, (size_t)G * VF_CS, b->stream)) return -2;
    const size_t need = 4 * PA + VI_N;                 // x_out, s, the result block | phi in, v in
    if (pin_reserve(&b->vh, need)) return -2;
    if (!vfit_lane(b)) {
        if (rows_scratch(vfit_plan(net), &b->ws, &b->ws_cap, vfit_rows(net), b->G, b->stream)) return -2;
        HCHK(lds_limit_once(&b->vf_lds_set, {(const void *)vfit_kernel<true, false>, (const void *)vfit_kernel<true, true>,
                                             (const void *)vfit_cand_kernel<true>}));
    }
    return 0;
}

// one product (or the first pass) of vector slot vi into b->slabs
static void vfit_product(trpo_bdev *b, int vi, int first, int mask) {
    const Net &net = b->net;
    const double *phi = b->vf + vfit_vec(b, 0), *v = b->vf + vfit_vec(b, vi);
    double *vold = b->vf + vfit_sc_off(b) + VSC_N + 4;
    const int *ctl = (const int *)(b->vf + vfit_sc_off(b) + VSC_N);
    if (vfit_lane(b)) {
        if (first)
            hipLaunchKernelGGL(vfit_lane_kernel<true>, dim3(b->Gl), dim3(256), 0, b->stream, net, phi, v,
                               (const double *)b->obs, (const double *)b->target, (int)b->n, b->slabs, vold, ctl, mask);
        else
            hipLaunchKernelGGL(vfit_lane_kernel<false>, dim3(b->Gl), dim3(256), 0, b->stream, net, phi, v,
                               (const double *)b->obs, (const double *)b->target, (int)b->n, b->slabs, vold, ctl, mask);
        return;
    }
    const RowsPlan y = vfit_plan(net);
    hipLaunchKernelGGL(ROWS_FORM(vfit_kernel, y), dim3(b->G), dim3(UT), y.lds, b->stream, net, phi, v,
                       (const double *)b->obs, (const double *)b->target, (int)b->n, b->ws, vfit_rows(net), b->slabs,
                       vold, first, ctl, mask);
}

// out [PA] = H v at weights x on the object's data; -1 bad arguments or no data, -7 an evaluation in flight
extern "C" int trpo_bdev_gnvp(trpo_bdev *b, const double *x, const double *v, double damping, double *out) {
    if (!b || !x || !v || !out || !b->n) return -1;
    if (b->started) return -7;
    if (const int rc = vfit_reserve(b)) return rc;
    const Net &net = b->net;
    const int PA = net.P - net.A, len = net.P + 1, G = vfit_lane(b) ? b->Gl : b->G;
    memcpy(b->vh.host + 2 * PA + VI_N, x, sizeof(double) * PA);
    memcpy(b->vh.host + 3 * PA + VI_N, v, sizeof(double) * PA);
    hipLaunchKernelGGL(copy64_kernel, dim3(cdiv(2 * PA, 256)), dim3(256), 0, b->stream,
                       (const double *)(b->vh.dev + 2 * PA + VI_N), b->vf, 2 * PA);
    vfit_product(b, 1, 0, 0);
    hipLaunchKernelGGL(vfit_gnvp_out_kernel, dim3(cdiv(PA, 256)), dim3(256), 0, b->stream, (const double *)b->slabs, G,
                       PA, len, (double)b->n, damping, (const double *)(b->vf + vfit_vec(b, 1)), b->vh.dev);
    HCHK(hipGetLastError());
    HCHK(hipStreamSynchronize(b->stream));
    memcpy(out, b->vh.host, sizeof(double) * PA);
    return 0;
}

// The fit.  x_out [PA], step_out [PA] (or NULL), info [TRPO_BDEV_VFIT_INFO] (or NULL) = loss_before, gnorm,
// shs, alpha_tr, alpha0, cg_iters, accepted, loss[32], shift[32], rdotr[maxiter + 1 ...] (zero beyond
// cg_iters).  -1 / -7 as above; -8: sigma^2 is zero or not finite (x_out = x).  The caller has checked the
// ranges of maxiter (1 .. TRPO_BDEV_VFIT_MAX_CG) and nk (1 .. 32).
extern "C" int trpo_bdev_fit_tr(trpo_bdev *b, const double *x, double eps, size_t maxiter, double resth, double damping,
                                int nk, double shift_cap, double *x_out, double *step_out, double *info) {
    if (!b || !x || !x_out || !b->n || maxiter < 1 || maxiter > TRPO_BDEV_VFIT_MAX_CG || nk < 1 || nk > 32) return -1;
    if (b->started) return -7;
    if (const int rc = vfit_reserve(b)) return rc;
    const Net &net = b->net;
    const int PA = net.P - net.A, len = net.P + 1, lane = vfit_lane(b), G = lane ? b->Gl : b->G;
    const double N = (double)b->n;
    double *phi = b->vf, *g = b->vf + vfit_vec(b, 2), *s = b->vf + vfit_vec(b, 3), *r = b->vf + vfit_vec(b, 4);
    double *p = b->vf + vfit_vec(b, 5), *z = b->vf + vfit_vec(b, 6), *cs = b->vf + vfit_vec(b, 7);
    double *sc = b->vf + vfit_sc_off(b);
    int *ctl = (int *)(sc + VSC_N);
    double *vold = sc + VSC_N + 4, *hinfo = b->vh.dev + 2 * PA;
    memcpy(b->vh.host + 2 * PA + VI_N, x, sizeof(double) * PA);
    memset(b->vh.host + 2 * PA, 0, sizeof(double) * VI_N);
    hipLaunchKernelGGL(copy64_kernel, dim3(cdiv(PA, 256)), dim3(256), 0, b->stream,
                       (const double *)(b->vh.dev + 2 * PA + VI_N), phi, PA);
    vfit_product(b, 0, 1, 0);
    const dim3 sg(cdiv(len, 16));
    hipLaunchKernelGGL(sum_slabs64_kernel, sg, dim3(256), 0, b->stream, (const double *)b->slabs, G, len, cs);
    hipLaunchKernelGGL(vfit_init_kernel, dim3(1), dim3(VF_T), 0, b->stream, PA, N, g, s, r, p, (const double *)cs, sc,
                       ctl, hinfo);
    for (size_t it = 0; it < maxiter; ++it) {
        vfit_product(b, 5, 0, 1);
        hipLaunchKernelGGL(sum_slabs64_kernel, sg, dim3(256), 0, b->stream, (const double *)b->slabs, G, len, cs);
        hipLaunchKernelGGL(vfit_step_kernel, dim3(1), dim3(VF_T), 0, b->stream, PA, N, damping, resth, (int)it, s, r, p,
                           z, (const double *)cs, sc, ctl, hinfo);
    }
    vfit_product(b, 3, 0, 2);
    hipLaunchKernelGGL(vfit_scale_kernel, dim3(1), dim3(VF_T), 0, b->stream, (const double *)b->slabs, G, PA, len, N,
                       damping, eps, (const double *)s, sc, (const int *)ctl, hinfo);
    if (lane) {
        hipLaunchKernelGGL(vfit_cand_lane_kernel, dim3(b->Gl), dim3(256), 0, b->stream, net, (const double *)phi,
                           (const double *)s, (const double *)sc, nk, (const double *)b->obs, (const double *)b->target,
                           (const double *)vold, (int)b->n, b->vcs, (const int *)ctl);
    } else {
        const int rows = rows_for(net, false);
        const RowsPlan y = vfit_cand_plan(net);
        if (rows_scratch(y, &b->ws, &b->ws_cap, rows, b->G, b->stream)) return -2;
        hipLaunchKernelGGL(y.use_lds ? vfit_cand_kernel<true> : vfit_cand_kernel<false>, dim3(b->G), dim3(UT), y.lds,
                           b->stream, net, (const double *)phi, (const double *)s,
                           (const double *)sc, nk, (const double *)b->obs, (const double *)b->target,
                           (const double *)vold, (int)b->n, b->ws, rows, b->vcs, (const int *)ctl);
    }
    hipLaunchKernelGGL(sum_slabs64_kernel, dim3(cdiv(VF_CS, 16)), dim3(256), 0, b->stream, (const double *)b->vcs, G,
                       VF_CS, cs);
    hipLaunchKernelGGL(vfit_select_kernel, dim3(1), dim3(VF_T), 0, b->stream, nk, N, shift_cap, PA, (const double *)phi,
                       (const double *)s, (const double *)cs, (const double *)sc, (const int *)ctl, b->vh.dev);
    HCHK(hipGetLastError());
    HCHK(hipStreamSynchronize(b->stream));
    memcpy(x_out, b->vh.host, sizeof(double) * PA);
    if (step_out) memcpy(step_out, b->vh.host + PA, sizeof(double) * PA);
    if (info) memcpy(info, b->vh.host + 2 * PA, sizeof(double) * VI_N);
    return b->vh.host[2 * PA + VI_BAD] != 0.0 ? -8 : 0;
}
