/*
 * ddc_adapt.cpp -- host side of the adaptive filter (include/perseus_ddc.h, pddc_adapt_*): the object, its receiver
 * table, the launch of a batch and the read of the weights.  The kernel is in ddc_adapt.hip.
 * What is carried per receiver (T weights, the last D + T - 1 inputs) lives on the device in two records, read and
 * written in turn; nothing on the device is cleared from the host: create and reset set `fresh` (the next launch does not
 * read the record, its values are 0), set_rx(PDDC_ADAPT_RESTART) leaves a mark in the receiver's table entry (the next
 * launch takes that receiver's weights as 0), which goes once a launch was accepted.  Mode, step and leak live in the
 * table, which is uploaded in stream order when it changed.
 */
#include "ddc_host.h"
#include "ddc_adapt.h"

#include <cstring>
#include <new>
#include <vector>

using namespace pddc;

struct pddc_adapt {
    int device = 0;
    int nrx = 0;
    pddc_adapt_params par{};
    std::vector<AdaptRx> table;                     /* flags carry kAdaptRestart; uploaded when `dirty`            */
    std::vector<AdaptRx> staged;                    /* the copy an upload reads: touched by the next upload only   */
    bool dirty = true;
    bool fresh = true;                              /* no launch since create / reset                              */
    AdaptRx *d_table = nullptr;
    float *d_w[2] = { nullptr, nullptr };           /* [nrx][T]: process() reads [cur] and writes [cur ^ 1]        */
    float *d_h[2] = { nullptr, nullptr };           /* [nrx][D + T - 1], the same                                  */
    int cur = 0;
};

static_assert(PDDC_ADAPT_OFF == kAdaptOff && PDDC_ADAPT_NR == kAdaptNr && PDDC_ADAPT_NOTCH == kAdaptNotch,
              "the kernel's modes are the header's");
static_assert(PDDC_ADAPT_RESTART == kAdaptRestart, "the kernel's flag bits are the header's");

/* written so that a NaN fails it */
static bool adapt_rx_ok(uint32_t mode, float mu, float leak, uint32_t flags)
{
    return mode < kAdaptModes && !(flags & ~kAdaptRestart) && mu > 0.0f && mu < 2.0f && leak >= 0.0f && leak < 1.0f;
}

static bool adapt_taps_ok(int T) { return T == 16 || T == 32 || T == 64 || T == 128; }

static size_t adapt_hist(const pddc_adapt *s) { return (size_t)(s->par.delay + s->par.taps - 1); }

static void adapt_free(pddc_adapt *s)
{
    hipFree(s->d_table);
    for (int i = 0; i < 2; ++i) {
        hipFree(s->d_w[i]);
        hipFree(s->d_h[i]);
    }
    delete s;
}

static int adapt_alloc(pddc_adapt *s)
{
    PDDC_HIP_TRY(hipSetDevice(s->device));
    const size_t wb = sizeof(float) * (size_t)s->nrx * (size_t)s->par.taps, hb = sizeof(float) * (size_t)s->nrx * adapt_hist(s);
    PDDC_HIP_TRY(hipMalloc(&s->d_table, sizeof(AdaptRx) * (size_t)s->nrx));
    for (int i = 0; i < 2; ++i) {
        PDDC_HIP_TRY(hipMalloc(&s->d_w[i], wb));
        PDDC_HIP_TRY(hipMalloc(&s->d_h[i], hb));
        PDDC_HIP_TRY(hipMemset(s->d_w[i], 0, wb));
        PDDC_HIP_TRY(hipMemset(s->d_h[i], 0, hb));
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

int pddc_adapt_tile_outputs(void) { return kAdaptTile; }

int pddc_adapt_create(pddc_adapt **out, int device, int nrx, const pddc_adapt_params *par, const pddc_adapt_rx *rx)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (nrx < 1 || nrx > kAdaptMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "adapt: %d receivers (1 .. %d) and their modes", nrx, kAdaptMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "adapt: null parameters");
    if (!adapt_taps_ok(par->taps) || par->delay < 1 || par->delay > kAdaptMaxDelay)
        return pddc_set_error_(PDDC_EINVAL, "adapt: %d taps (16, 32, 64, 128), delay %d (1 .. %d)", par->taps, par->delay,
                               kAdaptMaxDelay);
    if (!(par->eps > 0.0f && par->eps <= 3.4028234e38f))
        return pddc_set_error_(PDDC_EINVAL, "adapt: eps %g (finite, > 0)", (double)par->eps);
    for (int j = 0; j < nrx; ++j)
        if (!adapt_rx_ok(rx[j].mode, rx[j].mu, rx[j].leak, rx[j].flags))
            return pddc_set_error_(PDDC_EINVAL, "adapt: receiver %d: mode %u, mu %g (0 < mu < 2), leak %g (0 <= leak < 1), flags 0x%x",
                                   j, rx[j].mode, (double)rx[j].mu, (double)rx[j].leak, rx[j].flags);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_adapt *s = new (std::nothrow) pddc_adapt;
    if (!s)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    s->device = device;
    s->nrx = nrx;
    s->par = *par;
    s->table.resize((size_t)nrx);
    /* a restart at create has nothing to restart */
    for (int j = 0; j < nrx; ++j)
        s->table[(size_t)j] = AdaptRx{ rx[j].mode, rx[j].mu, 1.0f - rx[j].leak, 0u };
    const int rc = adapt_alloc(s);
    if (rc) {
        adapt_free(s);
        return rc;
    }
    *out = s;
    return PDDC_OK;
}

int pddc_adapt_destroy(pddc_adapt *s)
{
    if (!s)
        return PDDC_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    adapt_free(s);
    return PDDC_OK;
}

int pddc_adapt_reset(pddc_adapt *s)
{
    if (!s)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(s->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    s->fresh = true;
    for (AdaptRx &r : s->table)
        r.flags &= ~kAdaptRestart;
    s->dirty = true;
    return PDDC_OK;
}

int pddc_adapt_set_rx(pddc_adapt *s, int rx, uint32_t mode, float mu, float leak, uint32_t flags)
{
    if (!s)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (rx < 0 || rx >= s->nrx)
        return pddc_set_error_(PDDC_EINVAL, "adapt: receiver %d (0 .. %d)", rx, s->nrx - 1);
    if (!adapt_rx_ok(mode, mu, leak, flags))
        return pddc_set_error_(PDDC_EINVAL, "adapt: mode %u, mu %g (0 < mu < 2), leak %g (0 <= leak < 1), flags 0x%x", mode,
                               (double)mu, (double)leak, flags);
    AdaptRx &r = s->table[(size_t)rx];
    /* a restart asked for earlier and not yet honoured stays asked for */
    r = AdaptRx{ mode, mu, 1.0f - leak, r.flags | (flags & kAdaptRestart) };
    s->dirty = true;
    return PDDC_OK;
}

int pddc_adapt_process(pddc_adapt *s, const void *d_a, size_t n, size_t a_stride, void *d_out, size_t out_stride, void *stream)
{
    if (!s)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (n && (!d_a || ((uintptr_t)d_a & 3)))
        return pddc_set_error_(PDDC_EINVAL, "d_a must be a 4-byte aligned device pointer");
    if (n && (!d_out || ((uintptr_t)d_out & 3)))
        return pddc_set_error_(PDDC_EINVAL, "d_out must be a 4-byte aligned device pointer");
    if (n > a_stride || n > out_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "adapt: %zu samples per receiver, a_stride %zu, out_stride %zu", n, a_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    {
        const size_t rows = (size_t)s->nrx - 1;
        const size_t ab = (rows * a_stride + n) * 4, ob = (rows * out_stride + n) * 4;
        if (!(d_out == d_a && out_stride == a_stride) && ranges_overlap(d_out, ob, d_a, ab))
            return pddc_set_error_(PDDC_EINVAL, "adapt: out overlaps a (in place is out == a with equal strides)");
    }
    PDDC_HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (s->dirty) {
        s->staged = s->table;
        PDDC_HIP_TRY(hipMemcpyAsync(s->d_table, s->staged.data(), sizeof(AdaptRx) * (size_t)s->nrx, hipMemcpyHostToDevice, st));
        s->dirty = false;
    }
    AdaptArgs a{};
    a.a = static_cast<const float *>(d_a);
    a.a_stride = (long long)a_stride;
    a.out = static_cast<float *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = s->d_table;
    a.nrx = s->nrx;
    a.T = s->par.taps;
    a.D = s->par.delay;
    a.eps = s->par.eps;
    a.old_w = s->d_w[s->cur];
    a.old_h = s->d_h[s->cur];
    a.new_w = s->d_w[s->cur ^ 1];
    a.new_h = s->d_h[s->cur ^ 1];
    a.fresh = s->fresh ? 1u : 0u;
    PDDC_HIP_TRY(launch_adapt(a, st));
    /* the launch was accepted: only now do the buffers turn; the restart marks go, and the table on the device follows
     * with the next batch */
    s->cur ^= 1;
    s->fresh = false;
    for (AdaptRx &r : s->table)
        if (r.flags & kAdaptRestart) {
            r.flags &= ~kAdaptRestart;
            s->dirty = true;
        }
    return PDDC_OK;
}

int pddc_adapt_read_weights(pddc_adapt *s, float *host, void *stream)
{
    if (!s || !host)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t count = (size_t)s->nrx * (size_t)s->par.taps;
    if (s->fresh)
        std::memset(host, 0, sizeof(float) * count);
    else
        PDDC_HIP_TRY(hipMemcpyAsync(host, s->d_w[s->cur], sizeof(float) * count, hipMemcpyDeviceToHost, st));
    PDDC_HIP_TRY(hipStreamSynchronize(st));
    return PDDC_OK;
}

} // extern "C"
