// Section of trpo_kernels.hip, included once behind struct trpo_dev and its setters: staged copies.
// Relies on, from trpo_kernels.hip above the include: struct trpo_dev, has_collective, coop_dist, Ctl, CG_AMAX;
// from trpo_common.h: HCHK, cdiv, TRPO_HOST_COHERENT, trpo_wait_host_flags; from trpo_dev.h: the
// declarations of trpo_dev_wait_done and trpo_dev_comm_error (defined in dev_comm.h) and the TRPO_VEC_* slots.
//
// Host <-> device vector moves through a pinned, device-mapped host buffer and a copy kernel: a
// pageable hipMemcpyAsync costs ~20 us per call (staged through a driver bounce buffer), this ~5.
__global__ void vcopy64_kernel(const double *__restrict__ src, double *__restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
// the upload of a direction for the cooperative kernel: the natural-order copy, and the same values in the
// fp32 fragment-order pack (slot pslot[i], -1 for LogStd), so the FVP loads the pack coalesced instead of
// every block gathering it (round 5; the CG's cg_axpy does the same for p')
__global__ void vcopy_pack_kernel(const double *__restrict__ src, double *__restrict__ dst, int n,
                                  float *__restrict__ vpk, const int *__restrict__ pslot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double v = src[i];
        dst[i] = v;
        const int s = pslot[i];
        if (s >= 0) vpk[s] = (float)v;
    }
}
// host_writes: the caller is about to write the buffer from the host (an upload); device-side
// writers (downloads) are ordered after a pending upload's copy by the stream and need no wait
// (its return code is passed on unchanged: -4 when the wait it needed found the collective failed)
// The wait of the calls whose results come back through the pinned staging buffer (copy kernels, no
// hipMemcpy to pageable memory pending): without a collective a stream write of a sequence number into
// pinned memory behind the enqueued work and a spin on it -- ~2.5 us sooner than hipStreamSynchronize per
// host round trip (tools/micro/host_wait: 9.1 vs 11.6 us for one small launch; profiles/r06_host_wait.log);
// the stream is queried after 2 ms, so a failed launch still returns its error.  Where the write is
// refused, and with a collective, trpo_dev_wait_done.
static int wait_staged(trpo_dev *d) {
    if (!has_collective(d) && d->wflag_dev) {
        if (++d->wseq == 0) d->wseq = 1;
        if (hipStreamWriteValue32(d->stream, d->wflag_dev, d->wseq, 0) == hipSuccess)
            return trpo_wait_host_flags(d->stream, d->wflag, 1, d->wseq, 2000);
    }
    return trpo_dev_wait_done(d);
}
#define DSYNC_STAGED(d)                            \
    do {                                           \
        const int dsync_rc_ = wait_staged(d);      \
        if (dsync_rc_) return dsync_rc_;           \
    } while (0)

static int ensure_hst(trpo_dev *d, size_t count, bool host_writes = false) {
    if (d->hst_pending && (host_writes || count > d->hst_cap || !d->hst)) {
        DSYNC_STAGED(d);
        d->hst_pending = 0;
    }
    if (count <= d->hst_cap && d->hst) return 0;
    if (d->hst) hipHostFree(d->hst);
    d->hst = d->hst_dev = NULL;
    d->hst_cap = 0;
    HCHK(hipHostMalloc((void **)&d->hst, sizeof(double) * count, TRPO_HOST_COHERENT));
    HCHK(hipHostGetDevicePointer((void **)&d->hst_dev, d->hst, 0));
    d->hst_cap = count;
    return 0;
}

extern "C" int trpo_dev_upload(trpo_dev *d, int slot, const double *host) {
    if (!d || slot < 0 || slot > 4 || !host) return -1;
    HCHK(hipSetDevice(d->device));
    if (const int hrc = ensure_hst(d, (size_t)d->P + 2 * (size_t)(d->hist_cap + 8), true)) return hrc;
    memcpy(d->hst, host, sizeof(double) * d->P);
    if (slot == TRPO_VEC_V && coop_dist(d)) {
        hipLaunchKernelGGL(vcopy_pack_kernel, dim3(cdiv(d->P, 256)), dim3(256), 0, d->stream,
                           (const double *)d->hst_dev, d->vec[slot], d->P, (float *)d->vpack, (const int *)d->pslot);
        d->vpack_v = 1;
    } else {
        hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv(d->P, 256)), dim3(256), 0, d->stream, (const double *)d->hst_dev,
                           d->vec[slot], d->P);
    }
    HCHK(hipGetLastError());
    // no wait here: the stream orders the copy before every later kernel, and the next host-side
    // write to the staging buffer (ensure_hst) waits for it
    d->hst_pending = 1;
    return 0;
}

extern "C" int trpo_dev_download(trpo_dev *d, int slot, double *host) {
    if (!d || slot < 0 || slot > 4 || !host) return -1;
    HCHK(hipSetDevice(d->device));
    if (const int hrc = ensure_hst(d, (size_t)d->P + 2 * (size_t)(d->hist_cap + 8))) return hrc;
    hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv(d->P, 256)), dim3(256), 0, d->stream, (const double *)d->vec[slot],
                       d->hst_dev, d->P);
    HCHK(hipGetLastError());
    DSYNC_STAGED(d);
    d->hst_pending = 0;
    memcpy(host, d->hst, sizeof(double) * d->P);
    return trpo_dev_comm_error(d);
}

// x (slot X) and what the fp32 stall guard reads of the last solve -- ctl->iter, ctl->orth, alpha[] and
// the rdotr history -- in one synchronisation
extern "C" int trpo_dev_download_x_cg(trpo_dev *d, double *host, double *stats, double *rdotr, size_t cap,
                                      size_t *iters) {
    if (!d || !host || !stats || !rdotr || !iters) return -1;
    HCHK(hipSetDevice(d->device));
    const int cw = (int)cdiv(sizeof(Ctl), sizeof(double)), hw = 2 * d->hist_cap;
    if (const int hrc = ensure_hst(d, (size_t)d->P + cw + hw)) return hrc;
    hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv(d->P, 256)), dim3(256), 0, d->stream,
                       (const double *)d->vec[TRPO_VEC_X], d->hst_dev, d->P);
    hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv(cw, 256)), dim3(256), 0, d->stream, (const double *)d->ctl,
                       d->hst_dev + d->P, cw);
    if (hw) hipLaunchKernelGGL(vcopy64_kernel, dim3(cdiv(hw, 256)), dim3(256), 0, d->stream,
                               (const double *)d->hist, d->hst_dev + d->P + cw, hw);
    HCHK(hipGetLastError());
    DSYNC_STAGED(d);
    d->hst_pending = 0;
    memcpy(host, d->hst, sizeof(double) * d->P);
    Ctl c;
    memcpy(&c, d->hst + d->P, sizeof c);
    stats[0] = c.orth;
    memcpy(stats + 1, c.alpha, sizeof(double) * CG_AMAX);
    *iters = (size_t)c.iter;
    for (size_t k = 0; k <= (size_t)c.iter && k < cap && (int)k < d->hist_cap; ++k)
        rdotr[k] = d->hst[d->P + cw + 2 * k];
    return trpo_dev_comm_error(d);
}
