/*
 * ddc_blanker.cpp -- host side of the noise blanker (include/perseus_ddc.h, pddc_blanker_*): the object, its receiver
 * table, the sample counter, the launch of a batch and the status read.  The kernel is in ddc_blanker.hip.
 * What is carried per receiver (partial sum, reference, the two counters; the last D inputs; the trigger bits of the
 * last 512 inputs, of which 2 D are looked at) lives on the device in two sets of records, read and written in turn;
 * nothing on the device is cleared from the host: create and reset set `fresh` (the next launch does not read the
 * records, their values are the create values).  Thresholds and flags live in the table, which is uploaded in stream
 * order when it changed.
 */
#include "ddc_host.h"
#include "ddc_blanker.h"

#include <cmath>
#include <new>
#include <vector>

using namespace pddc;

struct pddc_blanker {
    int device = 0;
    int nrx = 0;
    pddc_blanker_params par{};
    float invB = 0.0f, invR1 = 0.0f;
    std::vector<BlankerRx> table;                   /* uploaded when `dirty`                                       */
    std::vector<BlankerRx> staged;                  /* the copy an upload reads: touched by the next upload only   */
    std::vector<BlankerState> host_state;           /* where read() lands the records                              */
    bool dirty = true;
    bool fresh = true;                              /* no launch since create / reset                              */
    BlankerRx *d_table = nullptr;
    BlankerState *d_state[2] = { nullptr, nullptr };/* process() reads [cur] and writes [cur ^ 1]                  */
    float2 *d_hist[2] = { nullptr, nullptr };
    unsigned long long *d_bits[2] = { nullptr, nullptr };
    int cur = 0;
    uint64_t N = 0;                                 /* samples per receiver since create / reset                   */
};

static_assert(PDDC_NB_ON == kBlankerOn, "the kernel's flag bit is the header's");
static_assert(sizeof(pddc_blanker_status) == 12, "pddc_blanker_status is three 4-byte values");

/* written so that a NaN fails it */
static bool blanker_rx_ok(float thr, uint32_t flags)
{
    return !(flags & ~kBlankerOn) && thr > 0.0f && thr <= 3.4028234e38f;
}

static void blanker_free(pddc_blanker *b)
{
    hipFree(b->d_table);
    for (int i = 0; i < 2; ++i) {
        hipFree(b->d_state[i]);
        hipFree(b->d_hist[i]);
        hipFree(b->d_bits[i]);
    }
    delete b;
}

static int blanker_alloc(pddc_blanker *b)
{
    PDDC_HIP_TRY(hipSetDevice(b->device));
    const size_t rows = (size_t)b->nrx;
    const size_t sb = sizeof(BlankerState) * rows, hb = sizeof(float2) * kBlankerMaxDelay * rows,
                 bb = sizeof(unsigned long long) * kBlankerCarryWords * rows;
    PDDC_HIP_TRY(hipMalloc(&b->d_table, sizeof(BlankerRx) * rows));
    for (int i = 0; i < 2; ++i) {
        PDDC_HIP_TRY(hipMalloc(&b->d_state[i], sb));
        PDDC_HIP_TRY(hipMalloc(&b->d_hist[i], hb));
        PDDC_HIP_TRY(hipMalloc(&b->d_bits[i], bb));
        PDDC_HIP_TRY(hipMemset(b->d_state[i], 0, sb));
        PDDC_HIP_TRY(hipMemset(b->d_hist[i], 0, hb));
        PDDC_HIP_TRY(hipMemset(b->d_bits[i], 0, bb));
    }
    return PDDC_OK;
}

/* byte ranges [p, p + bytes) and [q, q + qbytes) share a byte */
static bool ranges_overlap(const void *p, size_t bytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + bytes;
}

extern "C" {

int pddc_blanker_tile_outputs(void) { return kBlankerTile; }

int pddc_blanker_create(pddc_blanker **out, int device, int nrx, const pddc_blanker_params *par, const pddc_blanker_rx *rx)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (nrx < 1 || nrx > kBlankerMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "blanker: %d receivers (1 .. %d) and their thresholds", nrx, kBlankerMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "blanker: null parameters");
    if (par->block < 1 || par->block > kBlankerMaxBlock || par->guard < 0 || par->guard > kBlankerMaxGuard || par->ramp < 0 ||
        par->ramp > kBlankerMaxRamp)
        return pddc_set_error_(PDDC_EINVAL, "blanker: block %d (1 .. %d), guard %d (0 .. %d), ramp %d (0 .. %d)", par->block,
                               kBlankerMaxBlock, par->guard, kBlankerMaxGuard, par->ramp, kBlankerMaxRamp);
    if (!(par->beta > 0.0f && par->beta <= 1.0f) || !(par->cap >= 1.0f && par->cap <= 3.4028234e38f))
        return pddc_set_error_(PDDC_EINVAL, "blanker: beta %g (0 < beta <= 1), cap %g (finite, >= 1)", (double)par->beta,
                               (double)par->cap);
    for (int j = 0; j < nrx; ++j)
        if (!blanker_rx_ok(rx[j].thr, rx[j].flags))
            return pddc_set_error_(PDDC_EINVAL, "blanker: receiver %d: threshold %g (finite, > 0), flags 0x%x", j,
                                   (double)rx[j].thr, rx[j].flags);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_blanker *b = new (std::nothrow) pddc_blanker;
    if (!b)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    b->device = device;
    b->nrx = nrx;
    b->par = *par;
    b->invB = 1.0f / (float)par->block;
    b->invR1 = 1.0f / (float)(par->ramp + 1);
    b->table.resize((size_t)nrx);
    b->host_state.resize((size_t)nrx);
    for (int j = 0; j < nrx; ++j)
        b->table[(size_t)j] = BlankerRx{ rx[j].thr, rx[j].flags };
    const int rc = blanker_alloc(b);
    if (rc) {
        blanker_free(b);
        return rc;
    }
    *out = b;
    return PDDC_OK;
}

int pddc_blanker_destroy(pddc_blanker *b)
{
    if (!b)
        return PDDC_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    blanker_free(b);
    return PDDC_OK;
}

int pddc_blanker_reset(pddc_blanker *b)
{
    if (!b)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(b->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    b->N = 0;
    b->fresh = true;
    return PDDC_OK;
}

int pddc_blanker_set_rx(pddc_blanker *b, int rx, float thr, uint32_t flags)
{
    if (!b)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (rx < 0 || rx >= b->nrx)
        return pddc_set_error_(PDDC_EINVAL, "blanker: receiver %d (0 .. %d)", rx, b->nrx - 1);
    if (!blanker_rx_ok(thr, flags))
        return pddc_set_error_(PDDC_EINVAL, "blanker: threshold %g (finite, > 0), flags 0x%x", (double)thr, flags);
    /* nothing carried is reset */
    b->table[(size_t)rx] = BlankerRx{ thr, flags };
    b->dirty = true;
    return PDDC_OK;
}

int pddc_blanker_delay(const pddc_blanker *b)
{
    if (!b)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    return b->par.guard + b->par.ramp;
}

int pddc_blanker_process(pddc_blanker *b, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                         void *stream)
{
    if (!b)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (n && (!d_z || ((uintptr_t)d_z & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_z must be an 8-byte aligned device pointer");
    if (n && (!d_out || ((uintptr_t)d_out & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_out must be an 8-byte aligned device pointer");
    if (n > z_stride || n > out_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "blanker: %zu samples per receiver, z_stride %zu, out_stride %zu", n, z_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    const size_t rows = (size_t)b->nrx - 1;
    if (ranges_overlap(d_out, (rows * out_stride + n) * 8, d_z, (rows * z_stride + n) * 8))
        return pddc_set_error_(PDDC_EINVAL, "blanker: out overlaps z (there is no in-place form: out[n] is made from z[n - D])");
    PDDC_HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)stream;
    if (b->dirty) {
        b->staged = b->table;
        PDDC_HIP_TRY(hipMemcpyAsync(b->d_table, b->staged.data(), sizeof(BlankerRx) * (size_t)b->nrx, hipMemcpyHostToDevice, st));
        b->dirty = false;
    }
    BlankerArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.out = static_cast<float2 *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = b->d_table;
    a.nrx = b->nrx;
    a.old = b->d_state[b->cur];
    a.new_state = b->d_state[b->cur ^ 1];
    a.old_hist = b->d_hist[b->cur];
    a.new_hist = b->d_hist[b->cur ^ 1];
    a.old_bits = b->d_bits[b->cur];
    a.new_bits = b->d_bits[b->cur ^ 1];
    a.B = (uint32_t)b->par.block;
    a.W = (uint32_t)b->par.guard;
    a.D = (uint32_t)(b->par.guard + b->par.ramp);
    a.ph0 = (uint32_t)(b->N % (uint64_t)b->par.block);
    a.magic = ((1u << kBlankerDivShift) + a.B - 1u) / a.B;
    a.invB = b->invB;
    a.invR1 = b->invR1;
    a.beta = b->par.beta;
    a.cap = b->par.cap;
    a.fresh = b->fresh ? 1u : 0u;
    PDDC_HIP_TRY(launch_blanker(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    b->cur ^= 1;
    b->N += n;
    b->fresh = false;
    return PDDC_OK;
}

int pddc_blanker_read(pddc_blanker *b, pddc_blanker_status *host, void *stream)
{
    if (!b || !host)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)stream;
    if (!b->fresh)
        PDDC_HIP_TRY(hipMemcpyAsync(b->host_state.data(), b->d_state[b->cur], sizeof(BlankerState) * (size_t)b->nrx,
                                    hipMemcpyDeviceToHost, st));
    PDDC_HIP_TRY(hipStreamSynchronize(st));
    for (int j = 0; j < b->nrx; ++j) {
        const BlankerState &r = b->host_state[(size_t)j];
        host[j] = b->fresh ? pddc_blanker_status{ 0.0f, 0u, 0u } : pddc_blanker_status{ r.ref, r.triggers, r.blanked };
    }
    return PDDC_OK;
}

} // extern "C"
