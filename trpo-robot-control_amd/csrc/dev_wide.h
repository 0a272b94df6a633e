// Section of trpo_kernels.hip, included once behind struct trpo_dev and ahead of create and the setters, which
// call into it: the wide-policy solver path.
// Relies on, from trpo_kernels.hip above the include: struct trpo_dev, Ctl, CgSt, MFMA, f4, act_y, act_r,
// block_sum, CGS_T, CGS_K, RS_POS and the declaration of launch_sliced_step (defined with the CG launch
// sequences below); from trpo_common.h: Net, MAXL, HCHK, cdiv, trpo_malloc.
//
// Any policy shape the generic kernel takes, with no bound from one workgroup: the FVP runs layer by layer as
// GEMMs over all samples on v_mfma_f32_16x16x4_f32, the CG step is the distributed one over natural-order
// slices (launch_sliced_step), and the CG start below is a strided single block.
//
// Buffers (fp32, row-major over N_pad = samples rounded up to WIDE_TS rows; layer i has the padded width
// wd[i] = 16 ceil((L_i + 1) / 16), the last layer 16 ceil(A / 16)):
//   Y_i  [N_pad][wd[i]]   the forward cache; Y_0 holds the observations.  Column L_i of every Y_i but the
//                         last is the constant 1, the columns behind it are 0
//   Ry_i [N_pad][wd[i]]   i = 1 .. nl - 2 (Ry_0 = 0 is never formed, Ry of the last layer never stored)
//   G_i  [N_pad][wd[i]]   i = 1 .. nl - 1; the rows >= n and the columns >= L_i are 0
// theta and the direction as zero-padded copies: layer i a [wd[i]][wd[i + 1]] row-major block whose row L_i
// holds the bias, so that with the 1 column of Y_i
//   forward   Y_{i+1}  = act([Y_i 1] [W_i; b_i])
//   R-forward Rx_{i+1} = Ry_i [W_i; b_i] + [Y_i 1] [VW_i; vb_i]     (column L_i of Ry_i is 0)
//   backward  G_i      = act_i'(Y_i) . (G_{i+1} W_i^T)             (column L_i forced to 0)
//   contract  [dW_i; db_i] = [Y_i 1]^T G_{i+1}                     rows 0 .. L_i: the natural W_i, b_i block
// are plain GEMMs whose extents are all multiples of 16 and whose rows are 64-byte aligned: every global load
// is a whole in-range float4, no operand is read past its buffer, and edges need a guard only where a
// 16-column tile lies wholly beyond a buffer's width (zero-filled) and at the stores.
//
// One GEMM core (wide_mac): a block of 4 waves owns WIDE_TS = 64 rows of the product and 16 NT columns (NT 1,
// 2, 4 by the width), wave w rows 16 w .. 16 w + 15.  K runs in chunks of 16 through two LDS tiles As
// [64][WIDE_LD], Bs [16 NT][WIDE_LD], both k-contiguous with the padded row stride WIDE_LD = 20 floats: the
// MFMA operand read of lane l -- row l & 15, k = kk + (l >> 4) -- then touches the 64 banks 20 (l & 15) +
// (l >> 4) once each.  The three orientations differ only in how a tile reaches LDS: a k-contiguous operand
// (A of A.B and A.B^T, B of A.B^T) moves as float4 rows; a k-major one (B of A.B, both of A^T.B) is loaded
// with the lanes along k and stored transposed, 4 scalar stores per lane, bank (80 j + 20 e + k) mod 64 --
// again once each.  The next chunk's global loads are issued before the current chunk's MFMAs.
constexpr int WIDE_TS = 64;            // sample rows per block of the layer kernels (N_pad is a multiple)
constexpr int WIDE_SPLIT = 512;        // samples per block of the contraction: its split depends on N alone
constexpr int WIDE_KC = 16, WIDE_LD = 20;
static_assert(WIDE_SPLIT % WIDE_TS == 0 && WIDE_TS % WIDE_KC == 0, "whole chunks");

struct WideNet {
    int wd[MAXL];                      // padded widths
    int poff[MAXL];                    // layer i's block in the padded parameter copies
    int plen;
};

static inline int wide_pad16(int x) { return (x + 15) & ~15; }

// dst (fp32, padded layout) <- src (fp64, natural order); the LogStd block has no place in it
__global__ void wide_pack_kernel(float *__restrict__ dst, const double *__restrict__ src, Net net, WideNet wn) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= wn.plen) return;
    int i = 0;
    while (i + 2 < net.nl && e >= wn.poff[i + 1]) ++i;
    const int ld = wn.wd[i + 1], r = (e - wn.poff[i]) / ld, c = (e - wn.poff[i]) % ld;
    const int in = net.L[i], out = net.L[i + 1];
    double v = 0.0;
    if (c < out && r < in) v = src[net.woff[i] + r * out + c];
    else if (c < out && r == in) v = src[net.boff[i] + c];
    dst[e] = (float)v;
}

// Y_0 <- the observations: [N_pad][wd0], rows >= n zero, column L0 one
__global__ void wide_obs_kernel(float *__restrict__ dst, const double *__restrict__ src, int n, long total, int L0,
                                int wd0) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long s = e / wd0;
    const int c = (int)(e % wd0);
    dst[e] = c == L0 ? 1.0f : (s < n && c < L0) ? (float)src[s * L0 + c] : 0.0f;
}

template <bool KMAJOR>
struct WideTile;
// k-contiguous operand [rows][K] (ld = its row stride): a float4 of row t / 4; rows >= lim read as zero
template <>
struct WideTile<false> {
    static __device__ __forceinline__ float4 load(const float *__restrict__ M, int ld, int row0, int lim, long k0,
                                                  int t) {
        const int r = row0 + (t >> 2);
        if (r >= lim) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4 *>(M + (long)r * ld + k0 + (t & 3) * 4);
    }
    static __device__ __forceinline__ void store(float *S, float4 v, int t) {
        *reinterpret_cast<float4 *>(S + (t >> 2) * WIDE_LD + (t & 3) * 4) = v;
    }
};
// k-major operand [K][cols] (ld = its row stride): lane t & 15 along k, a float4 of columns 4 (t / 16);
// columns >= lim (a multiple of 4) read as zero; stored transposed
template <>
struct WideTile<true> {
    static __device__ __forceinline__ float4 load(const float *__restrict__ M, int ld, int col0, int lim, long k0,
                                                  int t) {
        const int c = col0 + (t >> 4) * 4;
        if (c >= lim) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4 *>(M + (k0 + (t & 15)) * ld + c);
    }
    static __device__ __forceinline__ void store(float *S, float4 v, int t) {
        float *p = S + (t >> 4) * 4 * WIDE_LD + (t & 15);
        p[0] = v.x;
        p[WIDE_LD] = v.y;
        p[2 * WIDE_LD] = v.z;
        p[3 * WIDE_LD] = v.w;
    }
};

// acc[nt] += op(A)[row0 + 16 w + . ][k] op(B)[k][col0 + 16 nt + . ] over k in [k0, k1) (whole chunks of 16).
// alim / blim: the extent of A's rows / B's columns (tiles beyond read as zero).  256 threads.
template <int NT, bool AK, bool BK>
__device__ __forceinline__ void wide_mac(f4 (&acc)[NT], const float *__restrict__ A, int lda, int row0, int alim,
                                         const float *__restrict__ B, int ldb, int col0, int blim, long k0, long k1,
                                         float *As, float *Bs) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const bool bt = t < 64 * NT;                           // the threads that move B's 16 x 16 NT tile
    float4 a4 = WideTile<AK>::load(A, lda, row0, alim, k0, t);
    float4 b4 = bt ? WideTile<BK>::load(B, ldb, col0, blim, k0, t) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float *ar = As + (w * 16 + (lane & 15)) * WIDE_LD + (lane >> 4);
    const float *br = Bs + (lane & 15) * WIDE_LD + (lane >> 4);
    for (long k = k0; k < k1; k += WIDE_KC) {
        __syncthreads();                                   // the previous chunk's operand reads are done
        WideTile<AK>::store(As, a4, t);
        if (bt) WideTile<BK>::store(Bs, b4, t);
        __syncthreads();
        if (k + WIDE_KC < k1) {
            a4 = WideTile<AK>::load(A, lda, row0, alim, k + WIDE_KC, t);
            if (bt) b4 = WideTile<BK>::load(B, ldb, col0, blim, k + WIDE_KC, t);
        }
#pragma unroll
        for (int kk = 0; kk < WIDE_KC; kk += 4) {
            const float a = ar[kk];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = MFMA(a, br[nt * 16 * WIDE_LD + kk], acc[nt]);
        }
    }
}

// The layer kernels' epilogues (EPI), applied to x = the accumulator at (row, col), col < ldo:
//   WIDE_FWD    out = act(x); the 1 column behind the last neuron where `ones`
//   WIDE_RFWD   out = act'(yo) x                                  (yo = the layer's own Y)
//   WIDE_RLAST  out = act'(yo) (act'(yo) x / sigma^2), rows >= n zero: G of the last layer from its Rx
//   WIDE_BWD    out = act'(yo) x
enum { WIDE_FWD = 0, WIDE_RFWD = 1, WIDE_RLAST = 2, WIDE_BWD = 3 };

// One layer product over all samples.  grid (N_pad / 64, ceil(ldo / 16 NT)).
//   EPI FWD:          A1 = Y_i,     B1 = theta block i (k-major), K = wd[i]
//   EPI RFWD / RLAST: A1 = Y_i,     B1 = direction block i; with A2: A2 = Ry_i, B2 = theta block i (same K)
//   EPI BWD:          A1 = G_{i+1}, B1 = theta block i read as [wd[i]][K = wd[i+1]] (k-contiguous: A.B^T)
template <int NT, int EPI>
__global__ void __launch_bounds__(256)
wide_layer_kernel(const float *__restrict__ A1, const float *__restrict__ B1, const float *__restrict__ A2,
                  const float *__restrict__ B2, int K, float *__restrict__ out, int ldo, int nv, int act, int ones,
                  const float *__restrict__ yo, const float *__restrict__ iv, int n, const int *__restrict__ skip) {
    __shared__ __attribute__((aligned(16))) float As[WIDE_TS * WIDE_LD];
    __shared__ __attribute__((aligned(16))) float Bs[16 * NT * WIDE_LD];
    if (*skip) return;
    const int row0 = blockIdx.x * WIDE_TS, col0 = blockIdx.y * 16 * NT;
    f4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f4){0.f, 0.f, 0.f, 0.f};
    constexpr bool BKM = EPI != WIDE_BWD;
    const int ldb = BKM ? ldo : K;
    wide_mac<NT, false, BKM>(acc, A1, K, row0, row0 + WIDE_TS, B1, ldb, col0, ldo, 0, K, As, Bs);
    if (EPI != WIDE_FWD && EPI != WIDE_BWD && A2)
        wide_mac<NT, false, BKM>(acc, A2, K, row0, row0 + WIDE_TS, B2, ldb, col0, ldo, 0, K, As, Bs);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = col0 + nt * 16 + (lane & 15);
        if (col >= ldo) continue;
        const float ivc = EPI == WIDE_RLAST ? iv[min(col, nv - 1)] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + w * 16 + (lane >> 4) * 4 + r;
            const long at = (long)row * ldo + col;
            const float x = acc[nt][r];
            float o;
            if (EPI == WIDE_FWD) {
                o = col < nv ? act_y(act, x) : (ones && col == nv) ? 1.0f : 0.0f;
            } else {
                const float y = yo[at];
                o = act_r(act, y, x);
                if (EPI == WIDE_RLAST) o = row < n ? act_r(act, y, o * ivc) : 0.0f;
                if (col >= nv) o = 0.0f;
            }
            out[at] = o;
        }
    }
}

// [dW_i; db_i] = [Y_i 1]^T G_{i+1} over this block's WIDE_SPLIT samples, fp32, into its slab in natural
// parameter order.  grid (blocks of the split, ceil((in + 1) / 64), ceil(out / 16 NT)); every slab position
// of the layer is written by exactly one block of a split, so the slabs need no zeroing.
template <int NT>
__global__ void __launch_bounds__(256)
wide_contract_kernel(const float *__restrict__ Y, int ldy, const float *__restrict__ G, int ldg, int npad, int in,
                     int out, float *__restrict__ slabs, int slab, int woff, const int *__restrict__ skip) {
    __shared__ __attribute__((aligned(16))) float As[WIDE_TS * WIDE_LD];
    __shared__ __attribute__((aligned(16))) float Bs[16 * NT * WIDE_LD];
    if (*skip) return;
    const int m0 = blockIdx.y * WIDE_TS, col0 = blockIdx.z * 16 * NT;
    const long k0 = (long)blockIdx.x * WIDE_SPLIT;
    const long k1 = k0 + WIDE_SPLIT < npad ? k0 + WIDE_SPLIT : npad;
    f4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f4){0.f, 0.f, 0.f, 0.f};
    wide_mac<NT, true, true>(acc, Y, ldy, m0, ldy, G, ldg, col0, ldg, k0, k1, As, Bs);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float *dst = slabs + (long)blockIdx.x * slab + woff;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int j = col0 + nt * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + w * 16 + (lane >> 4) * 4 + r;
            if (m <= in && j < out) dst[(long)m * out + j] = acc[nt][r];
        }
    }
}

// The CG start at any P (src/TRPO_CG.c:24-40; the fields of cg_init_kernel): x = 0, r = p = b, q_0 = b / |b|,
// rdotr = b.b summed in a fixed order (thread t takes elements t, t + 1024, ...; then block_sum).  One block.
__global__ void __launch_bounds__(1024)
wide_cg_init_kernel(const double *__restrict__ b, double *__restrict__ x, double *__restrict__ r,
                    double *__restrict__ p, int P, Ctl *ctl, CgSt *st, double *hist, int maxiter, double resth,
                    float *__restrict__ qbuf) {
#pragma clang fp contract(off)
    __shared__ double sh[16];
    double s = 0.0;
    for (int q = threadIdx.x; q < P; q += 1024) {
        const double v = b[q];
        s = __builtin_fma(v, v, s);
    }
    const double rr = block_sum(s, sh);
    const double inv = rr > 0.0 ? 1.0 / sqrt(rr) : 0.0;
    for (int q = threadIdx.x; q < P; q += 1024) {
        const double v = b[q];
        x[q] = 0.0;
        r[q] = v;
        p[q] = v;
        if (qbuf) qbuf[q] = (float)(v * inv);
    }
    if (threadIdx.x == 0) {
        ctl->maxiter = maxiter;
        ctl->resth = resth;
        ctl->rdotr = rr;
        ctl->iter = 0;
        ctl->orth = 0.0;
        st->rdotr = rr;
        st->xx = 0.0;
        st->iter = 0;
        hist[0] = rr;
        hist[1] = 0.0;
        ctl->done = (rr < resth || maxiter == 0) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct WideState {
    WideNet wn;
    float *tp, *vp;                    // zero-padded theta and direction
    float *act;                        // Y | Ry | G, one allocation
    size_t act_cap;                    // floats
    long npad;
    float *Y[MAXL], *Ry[MAXL], *G[MAXL];
};

static void wide_free(trpo_dev *d) {
    WideState *w = d->wide;
    if (!w) return;
    if (w->tp) hipFree(w->tp);
    if (w->vp) hipFree(w->vp);
    if (w->act) hipFree(w->act);
    free(w);
    d->wide = NULL;
}

// creation: the padded layout, the parameter copies, the sliced step's buffers (as the cooperative path's)
static int wide_init(trpo_dev *d) {
    WideState *w = (WideState *)calloc(1, sizeof(WideState));
    if (!w) return -3;
    d->wide = w;
    const Net &n = d->net;
    for (int i = 0; i < n.nl; ++i) w->wn.wd[i] = wide_pad16(i + 1 < n.nl ? n.L[i] + 1 : n.L[i]);
    int pos = 0;
    for (int i = 0; i + 1 < n.nl; ++i) {
        w->wn.poff[i] = pos;
        pos += w->wn.wd[i] * w->wn.wd[i + 1];
    }
    w->wn.plen = pos;
    HCHK(trpo_malloc((void **)&w->tp, sizeof(float) * pos));
    HCHK(trpo_malloc((void **)&w->vp, sizeof(float) * pos));
    HCHK(hipMemsetAsync(w->tp, 0, sizeof(float) * pos, d->stream));
    HCHK(hipMemsetAsync(w->vp, 0, sizeof(float) * pos, d->stream));
    HCHK(trpo_malloc((void **)&d->zbuf, sizeof(double) * d->Ps));
    HCHK(hipMemsetAsync(d->zbuf, 0, sizeof(double) * d->Ps, d->stream));
    const int gd = cdiv(d->Ps / 2, CGS_T), gr = d->slab / RS_POS;        // cg_dots / reduce_dots partials
    HCHK(trpo_malloc((void **)&d->dotsbuf, sizeof(double) * CGS_K * (gd > gr ? gd : gr)));
    HCHK(hipMemsetAsync(d->dotsbuf, 0, sizeof(double) * CGS_K * (gd > gr ? gd : gr), d->stream));
    int len = snprintf(d->name, sizeof d->name, "wide mfma ");
    for (int i = 0; i < n.nl && len < (int)sizeof d->name; ++i)
        len += snprintf(d->name + len, sizeof d->name - len, i ? "-%d" : "%d", n.L[i]);
    return 0;
}

static void wide_pack(trpo_dev *d, float *dst, const double *src) {
    const WideState *w = d->wide;
    hipLaunchKernelGGL(wide_pack_kernel, dim3(cdiv(w->wn.plen, 256)), dim3(256), 0, d->stream, dst, src, d->net, w->wn);
}

// blocks of the contraction's sample split (the slab count) for n samples
static int wide_blocks(size_t n) {
    const long npad = (long)cdiv((long)n, WIDE_TS) * WIDE_TS;
    return npad ? cdiv(npad, WIDE_SPLIT) : 1;
}

// set_obs: size the activation buffers for n samples and fill Y_0 from obs64 (device, [n][L0])
static int wide_set_obs(trpo_dev *d, const double *obs64, size_t n) {
    WideState *w = d->wide;
    const Net &net = d->net;
    const long npad = (long)cdiv((long)n, WIDE_TS) * WIDE_TS;
    const int last = net.nl - 1;
    size_t cols = 0;
    for (int i = 0; i <= last; ++i) cols += (size_t)w->wn.wd[i] * (1 + (i >= 1 && i < last) + (i >= 1));
    const size_t need = cols * (size_t)npad;
    if (need > w->act_cap) {
        if (w->act) hipFree(w->act);
        w->act = NULL;
        w->act_cap = 0;
        HCHK(trpo_malloc((void **)&w->act, sizeof(float) * need));
        w->act_cap = need;
    }
    w->npad = npad;
    float *at = w->act;
    for (int i = 0; i <= last; ++i) {
        w->Y[i] = at;
        at += (size_t)w->wn.wd[i] * npad;
    }
    for (int i = 1; i < last; ++i) {
        w->Ry[i] = at;
        at += (size_t)w->wn.wd[i] * npad;
    }
    for (int i = 1; i <= last; ++i) {
        w->G[i] = at;
        at += (size_t)w->wn.wd[i] * npad;
    }
    if (npad) {
        const long total = npad * w->wn.wd[0];
        hipLaunchKernelGGL(wide_obs_kernel, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, w->Y[0], obs64, (int)n,
                           total, net.L[0], w->wn.wd[0]);
    }
    return 0;
}

static inline int wide_nt(int width) { return width > 32 ? 4 : width > 16 ? 2 : 1; }

#define WIDE_LAYER(EPI, width, ...)                                                                              \
    do {                                                                                                         \
        const int nt_ = wide_nt(width);                                                                          \
        const dim3 g_((unsigned)(w->npad / WIDE_TS), (unsigned)cdiv(width, 16 * nt_));                           \
        if (nt_ == 4) hipLaunchKernelGGL((wide_layer_kernel<4, EPI>), g_, dim3(256), 0, d->stream, __VA_ARGS__); \
        else if (nt_ == 2) hipLaunchKernelGGL((wide_layer_kernel<2, EPI>), g_, dim3(256), 0, d->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((wide_layer_kernel<1, EPI>), g_, dim3(256), 0, d->stream, __VA_ARGS__);          \
    } while (0)

// The FVP's launches up to the block partials in d->slabs (d->grid of them): the direction src (fp64, natural
// order) into its padded copy, the forward sweep where the cache is not valid (never skipped: it is what
// makes the cache valid for everything enqueued behind it), the R-forward, backward and contraction launches
static int wide_fvp_launches(trpo_dev *d, const double *src, const int *skip) {
    WideState *w = d->wide;
    const Net &net = d->net;
    const int *wd = w->wn.wd, *po = w->wn.poff, last = net.nl - 1, n = (int)d->n;
    const float *nof = nullptr;
    if (!w->npad) return -1;
    wide_pack(d, w->vp, src);
    if (!d->yc_valid) {
        for (int i = 0; i < last; ++i)
            WIDE_LAYER(WIDE_FWD, wd[i + 1], (const float *)w->Y[i], (const float *)(w->tp + po[i]), nof, nof, wd[i],
                       w->Y[i + 1], wd[i + 1], net.L[i + 1], net.act[i + 1], i + 1 < last ? 1 : 0, nof, nof, n,
                       (const int *)&d->ctl->zero);
        ++d->fwd_passes;
        d->yc_valid = 1;
    }
    for (int i = 0; i < last; ++i) {
        const float *a2 = i ? w->Ry[i] : nof, *b2 = i ? w->tp + po[i] : nof;
        if (i + 1 < last)
            WIDE_LAYER(WIDE_RFWD, wd[i + 1], (const float *)w->Y[i], (const float *)(w->vp + po[i]), a2, b2, wd[i],
                       w->Ry[i + 1], wd[i + 1], net.L[i + 1], net.act[i + 1], 0, (const float *)w->Y[i + 1], nof, n,
                       skip);
        else
            WIDE_LAYER(WIDE_RLAST, wd[i + 1], (const float *)w->Y[i], (const float *)(w->vp + po[i]), a2, b2, wd[i],
                       w->G[i + 1], wd[i + 1], net.L[i + 1], net.act[i + 1], 0, (const float *)w->Y[i + 1],
                       (const float *)d->giv, n, skip);
    }
    for (int i = last - 1; i >= 1; --i)
        WIDE_LAYER(WIDE_BWD, wd[i], (const float *)w->G[i + 1], (const float *)(w->tp + po[i]), nof, nof, wd[i + 1],
                   w->G[i], wd[i], net.L[i], net.act[i], 0, (const float *)w->Y[i], nof, n, skip);
    for (int i = 0; i < last; ++i) {
        const int nt = wide_nt(net.L[i + 1]);
        const dim3 g((unsigned)d->grid, (unsigned)cdiv(net.L[i] + 1, WIDE_TS), (unsigned)cdiv(net.L[i + 1], 16 * nt));
#define WIDE_CONTRACT(NT)                                                                                          \
    hipLaunchKernelGGL(wide_contract_kernel<NT>, g, dim3(256), 0, d->stream, (const float *)w->Y[i], wd[i],        \
                       (const float *)w->G[i + 1], wd[i + 1], (int)w->npad, net.L[i], net.L[i + 1], (float *)d->slabs, \
                       d->slab, net.woff[i], skip)
        if (nt == 4) WIDE_CONTRACT(4);
        else if (nt == 2) WIDE_CONTRACT(2);
        else WIDE_CONTRACT(1);
#undef WIDE_CONTRACT
    }
    HCHK(hipGetLastError());
    return 0;
}
#undef WIDE_LAYER

// CG(maxiter) on the wide path, eager launches: the start, then per iteration the FVP of p_j (never skipped
// for j = 0, so that a solve that starts converged still leaves a valid forward cache where it ran the
// sweep) and the distributed step, which reads the slabs, forms z and the dots, and writes x, r', p' and the
// basis (launch_sliced_step with no fragment pack: the next FVP packs p' itself)
static int wide_cg_body(trpo_dev *d, size_t maxiter, double resth) {
    hipLaunchKernelGGL(wide_cg_init_kernel, dim3(1), dim3(1024), 0, d->stream, (const double *)d->vec[TRPO_VEC_B],
                       d->vec[TRPO_VEC_X], d->rbuf[0], d->pbuf[0], d->P, d->ctl, d->st, d->hist, (int)maxiter,
                       resth, d->reorth ? (float *)d->qbuf : nullptr);
    for (long j = 0; j < (long)maxiter; ++j) {
        if (const int rc = wide_fvp_launches(d, d->pbuf[j & 1], &d->ctl->done)) return rc;
        if (const int rc = launch_sliced_step(d, j)) return rc;
    }
    HCHK(hipGetLastError());
    return 0;
}
