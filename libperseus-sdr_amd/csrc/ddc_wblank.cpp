/*
 * ddc_wblank.cpp -- host side of the wideband blanker (include/perseus_ddc.h, pddc_wblank_*): the object, what it
 * carries, and the launches of a batch.  The carried samples are a PackedCarry (ddc_packed.h) whose tail always holds
 * wb_tail_len(D) samples (zeros in front of the stream); the kernels are in ddc_wblank.hip, the arithmetic both sides
 * share in ddc_wblank_gate.h.
 */
#include "ddc_wblank.h"
#include "ddc_kernels.h"

#include <new>

using namespace pddc;

struct pddc_wblank {
    int device = 0;
    int B = 0, b = 0, H = 0, W = 0, r = 0, D = 0, TL = 0;
    uint32_t thr16 = 16, flags = 0;
    int ncu = 256;
    PackedCarry in;                                 /* the tail's length (TL always), the stream length N, and per round
                                                     * the two tail buffers the round reads and writes              */
    /* what is carried lies in THREE sets of buffers: [cur] is what the accepted batches left; the rounds of a batch
     * write the other two in turn, so [cur] stays whole until the batch's last launch was accepted */
    uint8_t *d_tail[3] = { nullptr, nullptr, nullptr };     /* (TL + 8) * 6 bytes                                   */
    uint8_t *d_bits[3] = { nullptr, nullptr, nullptr };     /* the tail's trigger bits, a byte per group of 8       */
    WbState *d_state[3] = { nullptr, nullptr, nullptr };
    int cur = 0;
    uint64_t *d_sums = nullptr, *d_means = nullptr;
};

static void wb_free(pddc_wblank *w)
{
    w->in.d_tail[0] = w->d_tail[0];
    w->in.d_tail[1] = w->d_tail[1];
    w->in.free();
    hipFree(w->d_tail[2]);
    for (int i = 0; i < 3; ++i) {
        hipFree(w->d_bits[i]);
        hipFree(w->d_state[i]);
    }
    hipFree(w->d_sums);
    hipFree(w->d_means);
    delete w;
}

/* everything carried, as a fresh stream has it */
static int wb_clear(pddc_wblank *w)
{
    WbState st{};
    for (uint64_t &h : st.hist)
        h = kWbNoBlock;
    for (int i = 0; i < 3; ++i) {
        PDDC_HIP_TRY(hipMemset(w->d_tail[i], 0, (size_t)(w->TL + 8) * 6));
        PDDC_HIP_TRY(hipMemset(w->d_bits[i], 0, (size_t)wb_tail_bit_bytes(w->D) + 16));
        PDDC_HIP_TRY(hipMemcpy(w->d_state[i], &st, sizeof st, hipMemcpyHostToDevice));
    }
    w->in.reset();
    w->in.tail_len = (uint64_t)w->TL;
    w->cur = 0;
    return PDDC_OK;
}

static int wb_create(pddc_wblank *w)
{
    PDDC_HIP_TRY(hipSetDevice(w->device));
    int ncu = 0;
    PDDC_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, w->device));
    w->ncu = ncu > 0 ? ncu : 256;
    const hipError_t e = w->in.alloc((size_t)w->TL + 8);
    w->d_tail[0] = w->in.d_tail[0];
    w->d_tail[1] = w->in.d_tail[1];
    PDDC_HIP_TRY(e);
    PDDC_HIP_TRY(hipMalloc(&w->d_tail[2], ((size_t)w->TL + 8) * 6));
    for (int i = 0; i < 3; ++i) {
        PDDC_HIP_TRY(hipMalloc(&w->d_bits[i], (size_t)wb_tail_bit_bytes(w->D) + 16));
        PDDC_HIP_TRY(hipMalloc(&w->d_state[i], sizeof(WbState)));
    }
    PDDC_HIP_TRY(hipMalloc(&w->d_sums, wblank_sums_len(w->b) * sizeof(uint64_t)));
    PDDC_HIP_TRY(hipMalloc(&w->d_means, wblank_sums_len(w->b) * sizeof(uint64_t)));
    return wb_clear(w);
}

/* the samples one round of launches takes, and the samples one workgroup of k_wblank_gate walks */
static long long wb_chunk()
{
    const long long c = tunables().wblank_chunk.load();
    return c > 0 && c + 7 < kWbMaxChunk ? (c + 7) & ~7ll : kWbMaxChunk;
}
static long long wb_forced_run()
{
    const long long v = tunables().wblank_run.load();
    return v > 0 ? (v + kWbTile - 1) / kWbTile * kWbTile : 0;
}
/* automatic: one tile.  Measured on a batch of 2^28 (profiles/r27/wblank_runs.txt): runs of 1, 2, 16 and 128 tiles took 2.07,
 * 2.16, 2.32 and 3.01 times the copy's time -- a workgroup does not overlap one tile's loads with the tile before, so
 * more and shorter workgroups hide them better */
static long long wb_run()
{
    const long long forced = wb_forced_run();
    return forced ? forced : kWbTile;
}

static bool wb_batch_ok(const void *p, size_t nsamples) { return !nsamples || (p && !((uintptr_t)p & 15)); }

extern "C" {

int pddc_wblank_tile_samples(void) { return kWbTile; }

int pddc_wblank_run_samples(void)
{
    const long long forced = wb_forced_run();
    return forced ? (int)(forced < (1ll << 30) ? forced : (1ll << 30)) : kWbTile;
}

int pddc_wblank_delay(const pddc_wblank *w) { return w ? w->D : 0; }

int pddc_wblank_create(pddc_wblank **out, int device, const pddc_wblank_params *params, uint32_t thr16, uint32_t flags)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (!params)
        return pddc_set_error_(PDDC_EINVAL, "wblank: null params");
    if (!wb_params_ok(params->block, params->history, params->guard, params->ramp_log2))
        return pddc_set_error_(PDDC_EINVAL,
                               "wblank: block %d (a power of two 64 .. 4096), history %d (1 .. 16), guard %d (0 .. 128), "
                               "ramp_log2 %d (0 .. 7), guard + 2^ramp_log2 - 1 at most 255",
                               params->block, params->history, params->guard, params->ramp_log2);
    if (!wb_thr_ok(thr16))
        return pddc_set_error_(PDDC_EINVAL, "wblank: thr16 %u (16 .. 65536)", thr16);
    if (flags & ~PDDC_WB_ON)
        return pddc_set_error_(PDDC_EINVAL, "wblank: unknown flags 0x%x", flags);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_wblank *w = new (std::nothrow) pddc_wblank;
    if (!w)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    w->device = device;
    w->B = params->block;
    w->b = wb_log2_block(w->B);
    w->H = params->history;
    w->W = params->guard;
    w->r = params->ramp_log2;
    w->D = wb_delay(w->W, w->r);
    w->TL = wb_tail_len(w->D);
    w->thr16 = thr16;
    w->flags = flags;
    const int rc = wb_create(w);
    if (rc) {
        wb_free(w);
        return rc;
    }
    *out = w;
    return PDDC_OK;
}

int pddc_wblank_destroy(pddc_wblank *w)
{
    if (!w)
        return PDDC_OK;
    (void)hipSetDevice(w->device);
    (void)hipDeviceSynchronize();
    wb_free(w);
    return PDDC_OK;
}

int pddc_wblank_reset(pddc_wblank *w)
{
    if (!w)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(w->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    return wb_clear(w);
}

int pddc_wblank_set(pddc_wblank *w, uint32_t thr16, uint32_t flags)
{
    if (!w)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (!wb_thr_ok(thr16))
        return pddc_set_error_(PDDC_EINVAL, "wblank: thr16 %u (16 .. 65536)", thr16);
    if (flags & ~PDDC_WB_ON)
        return pddc_set_error_(PDDC_EINVAL, "wblank: unknown flags 0x%x", flags);
    w->thr16 = thr16;
    w->flags = flags;
    return PDDC_OK;
}

int pddc_wblank_process(pddc_wblank *w, const void *d_packed, size_t nsamples, void *d_out, void *stream)
{
    if (!w)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (const int rc = PackedCarry::check(d_packed, nsamples))
        return rc;
    if (!wb_batch_ok(d_out, nsamples))
        return pddc_set_error_(PDDC_EINVAL, "wblank: d_out must be a 16-byte aligned device pointer");
    if (!nsamples)
        return PDDC_OK;
    const uintptr_t i0 = (uintptr_t)d_packed, o0 = (uintptr_t)d_out, bytes = (uintptr_t)nsamples * 6;
    if (i0 < o0 + bytes && o0 < i0 + bytes)
        return pddc_set_error_(PDDC_EINVAL, "wblank: d_out overlaps d_packed (there is no in-place form)");
    PDDC_HIP_TRY(hipSetDevice(w->device));
    hipStream_t st = (hipStream_t)stream;

    /* rounds of at most wb_chunk() samples, each a batch of its own: a round reads set `src` of the carried buffers and
     * writes a set that is neither `src` nor the object's [cur], so whatever happens to a later launch the object still
     * has what the accepted batches left; it moves behind the last round */
    PackedCarry in = w->in;
    int src_set = w->cur;
    const long long chunk = wb_chunk();
    for (size_t done = 0; done < nsamples;) {
        const size_t n = nsamples - done < (size_t)chunk ? nsamples - done : (size_t)chunk;
        const uint8_t *src = static_cast<const uint8_t *>(d_packed) + done * 6;
        int dst_set = 0;
        while (dst_set == src_set || dst_set == w->cur)
            ++dst_set;
        in.d_tail[0] = w->d_tail[src_set];
        in.d_tail[1] = w->d_tail[dst_set];
        in.cur = 0;
        const PackedCarry::Plan plan = in.plan(n, w->TL + 8, 8);      /* keeps the last TL samples */
        WbArgs a{};
        a.in = in.stream(src);
        a.n = (long long)n;
        a.N = in.samples;
        a.b = w->b, a.H = w->H, a.W = w->W, a.r = w->r, a.D = w->D, a.TL = w->TL;
        a.thr16 = w->thr16;
        a.on = w->flags & PDDC_WB_ON;
        a.st = w->d_state[src_set];
        a.new_st = w->d_state[dst_set];
        a.sums = w->d_sums;
        a.means = w->d_means;
        a.nblocks = (long long)wb_blocks_touched(a.N, n, w->b);
        a.bits = w->d_bits[src_set];
        a.new_bits = w->d_bits[dst_set];
        a.out = static_cast<uint8_t *>(d_out) + done * 6;
        a.run = wb_run();
        a.tile_blocks = (int)((a.n + a.run - 1) / a.run);
        a.carry = in.carry(plan, src);
        PDDC_HIP_TRY(hipMemsetAsync(w->d_sums, 0, (size_t)(a.nblocks + 1) * sizeof(uint64_t), st));
        PDDC_HIP_TRY(launch_wblank_sums(a, 8 * w->ncu, st));
        PDDC_HIP_TRY(launch_wblank_means(a, st));
        PDDC_HIP_TRY(launch_wblank_gate(a, st));
        in.commit(plan, n);
        src_set = dst_set;
        done += n;
    }
    /* every launch was accepted: only now does the object move */
    w->in = in;
    w->cur = src_set;
    return PDDC_OK;
}

int pddc_wblank_read(pddc_wblank *w, pddc_wblank_status *host, void *stream)
{
    if (!w || !host)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(w->device));
    WbState st;
    PDDC_HIP_TRY(hipMemcpyAsync(&st, w->d_state[w->cur], sizeof st, hipMemcpyDeviceToHost, (hipStream_t)stream));
    PDDC_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    host->mean = st.mean;
    host->triggers = st.triggers;
    host->blanked = st.blanked;
    host->samples = w->in.samples;
    return PDDC_OK;
}

} // extern "C"
