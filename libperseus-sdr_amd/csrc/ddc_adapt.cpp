/*
 * ddc_adapt.cpp -- host side of the adaptive filter (include/perseus_ddc.h, pddc_adapt_*): the object, its receiver
 * table, the launch of a batch and the read of the weights.  The kernel is in ddc_adapt.hip.
 * What is carried per receiver (T weights, the last D + T - 1 inputs) lives on the device in two records, read and
 * written in turn; nothing on the device is cleared from the host: create and reset set `fresh` (the next launch does not
 * read the record, its values are 0), set_rx(PDDC_ADAPT_RESTART) leaves a mark in the receiver's table entry (the next
 * launch takes that receiver's weights as 0), which goes once a launch was accepted.  Mode, step and leak live in the
 * table, which is uploaded in stream order when it changed.
 */
#include "ddc_stage.h"
#include "ddc_adapt.h"

#include <cstring>

using namespace pddc;

struct pddc_adapt : StageBase {
    PDDC_LOCAL ~pddc_adapt() = default;
    pddc_adapt_params par{};
    RxTable<AdaptRx> table;                         /* flags carry kAdaptRestart                                   */
    bool fresh = true;                              /* no launch since create / reset                              */
    Carried<float> w;                               /* [nrx][T]                                                    */
    Carried<float> h;                               /* [nrx][D + T - 1]                                            */
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

extern "C" {

int pddc_adapt_tile_outputs(void) { return kAdaptTile; }

int pddc_adapt_create(pddc_adapt **out, int device, int nrx, const pddc_adapt_params *par, const pddc_adapt_rx *rx)
{
    if (!out)
        return null_argument();
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
    return stage_create(out, device, nrx, [&](pddc_adapt &s) {
        s.par = *par;
        /* a restart at create has nothing to restart */
        for (int j = 0; j < nrx; ++j)
            s.table.host.push_back(AdaptRx{ rx[j].mode, rx[j].mu, 1.0f - rx[j].leak, 0u });
        PDDC_TRY(s.table.alloc());
        PDDC_TRY(s.w.alloc((size_t)nrx * (size_t)par->taps));
        return s.h.alloc((size_t)nrx * (size_t)(par->delay + par->taps - 1));
    });
}

int pddc_adapt_destroy(pddc_adapt *s) { return stage_destroy(s); }

int pddc_adapt_reset(pddc_adapt *s)
{
    PDDC_TRY(stage_quiesce(s));
    s->fresh = true;
    for (AdaptRx &r : s->table.host)
        r.flags &= ~kAdaptRestart;
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_adapt_set_rx(pddc_adapt *s, int rx, uint32_t mode, float mu, float leak, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(s, "adapt", rx));
    if (!adapt_rx_ok(mode, mu, leak, flags))
        return pddc_set_error_(PDDC_EINVAL, "adapt: mode %u, mu %g (0 < mu < 2), leak %g (0 <= leak < 1), flags 0x%x", mode,
                               (double)mu, (double)leak, flags);
    AdaptRx &r = s->table.host[(size_t)rx];
    /* a restart asked for earlier and not yet honoured stays asked for */
    r = AdaptRx{ mode, mu, 1.0f - leak, r.flags | (flags & kAdaptRestart) };
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_adapt_process(pddc_adapt *s, const void *d_a, size_t n, size_t a_stride, void *d_out, size_t out_stride, void *stream)
{
    if (!s)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_a, 4, "d_a"));
        PDDC_TRY(device_ptr_ok(d_out, 4, "d_out"));
    }
    if (over_capacity(n, a_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "adapt: %zu samples per receiver, a_stride %zu, out_stride %zu", n, a_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    if (!(d_out == d_a && out_stride == a_stride) &&
        ranges_overlap(d_out, rows_extent(s->nrx, n, out_stride, 4), d_a, rows_extent(s->nrx, n, a_stride, 4)))
        return pddc_set_error_(PDDC_EINVAL, "adapt: out overlaps a (in place is out == a with equal strides)");
    PDDC_TRY(set_device(s->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(s->table.upload(st));
    AdaptArgs a{};
    a.a = static_cast<const float *>(d_a);
    a.a_stride = (long long)a_stride;
    a.out = static_cast<float *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = s->table.dev();
    a.nrx = s->nrx;
    a.T = s->par.taps;
    a.D = s->par.delay;
    a.eps = s->par.eps;
    a.old_w = s->w.old();
    a.old_h = s->h.old();
    a.new_w = s->w.next();
    a.new_h = s->h.next();
    a.fresh = s->fresh ? 1u : 0u;
    PDDC_HIP_TRY(launch_adapt(a, st));
    /* the launch was accepted: only now do the buffers turn; the restart marks go, and the table on the device follows
     * with the next batch */
    s->w.turn();
    s->h.turn();
    s->fresh = false;
    for (AdaptRx &r : s->table.host)
        if (r.flags & kAdaptRestart) {
            r.flags &= ~kAdaptRestart;
            s->table.dirty = true;
        }
    return PDDC_OK;
}

int pddc_adapt_read_weights(pddc_adapt *s, float *host, void *stream)
{
    if (!s || !host)
        return null_argument();
    PDDC_TRY(set_device(s->device));
    const size_t count = (size_t)s->nrx * (size_t)s->par.taps;
    if (s->fresh)
        std::memset(host, 0, sizeof(float) * count);
    return read_back(host, s->fresh ? nullptr : s->w.old(), count, (hipStream_t)stream);
}

} // extern "C"
