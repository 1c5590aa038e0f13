/*
 * ddc_blanker.cpp -- host side of the noise blanker (include/perseus_ddc.h, pddc_blanker_*): the object, its receiver
 * table, the sample counter, the launch of a batch and the status read.  The kernel is in ddc_blanker.hip.
 * What is carried per receiver (partial sum, reference, the two counters; the last D inputs; the trigger bits of the
 * last 512 inputs, of which 2 D are looked at) lives on the device in two sets of records, read and written in turn;
 * nothing on the device is cleared from the host: create and reset set `fresh` (the next launch does not read the
 * records, their values are the create values).  Thresholds and flags live in the table, which is uploaded in stream
 * order when it changed.
 */
#include "ddc_stage.h"
#include "ddc_blanker.h"

#include <cmath>

using namespace pddc;

struct pddc_blanker : StageBase {
    PDDC_LOCAL ~pddc_blanker() = default;
    pddc_blanker_params par{};
    float invB = 0.0f, invR1 = 0.0f;
    RxTable<BlankerRx> table;
    std::vector<BlankerState> host_state;           /* where read() lands the records                              */
    bool fresh = true;                              /* no launch since create / reset                              */
    Carried<BlankerState> state;                    /* [nrx]                                                       */
    Carried<float2> hist;                           /* [nrx][kBlankerMaxDelay]                                     */
    Carried<unsigned long long> bits;               /* [nrx][kBlankerCarryWords]                                   */
    uint64_t N = 0;                                 /* samples per receiver since create / reset                   */
};

static_assert(PDDC_NB_ON == kBlankerOn, "the kernel's flag bit is the header's");
static_assert(sizeof(pddc_blanker_status) == 12, "pddc_blanker_status is three 4-byte values");

/* written so that a NaN fails it */
static bool blanker_rx_ok(float thr, uint32_t flags)
{
    return !(flags & ~kBlankerOn) && thr > 0.0f && thr <= 3.4028234e38f;
}

extern "C" {

int pddc_blanker_tile_outputs(void) { return kBlankerTile; }

int pddc_blanker_create(pddc_blanker **out, int device, int nrx, const pddc_blanker_params *par, const pddc_blanker_rx *rx)
{
    if (!out)
        return null_argument();
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
    return stage_create(out, device, nrx, [&](pddc_blanker &b) {
        b.par = *par;
        b.invB = 1.0f / (float)par->block;
        b.invR1 = 1.0f / (float)(par->ramp + 1);
        b.host_state.resize((size_t)nrx);
        for (int j = 0; j < nrx; ++j)
            b.table.host.push_back(BlankerRx{ rx[j].thr, rx[j].flags });
        PDDC_TRY(b.table.alloc());
        PDDC_TRY(b.state.alloc((size_t)nrx));
        PDDC_TRY(b.hist.alloc((size_t)nrx * kBlankerMaxDelay));
        return b.bits.alloc((size_t)nrx * kBlankerCarryWords);
    });
}

int pddc_blanker_destroy(pddc_blanker *b) { return stage_destroy(b); }

int pddc_blanker_reset(pddc_blanker *b)
{
    PDDC_TRY(stage_quiesce(b));
    b->N = 0;
    b->fresh = true;
    return PDDC_OK;
}

int pddc_blanker_set_rx(pddc_blanker *b, int rx, float thr, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(b, "blanker", rx));
    if (!blanker_rx_ok(thr, flags))
        return pddc_set_error_(PDDC_EINVAL, "blanker: threshold %g (finite, > 0), flags 0x%x", (double)thr, flags);
    /* nothing carried is reset */
    b->table.host[(size_t)rx] = BlankerRx{ thr, flags };
    b->table.dirty = true;
    return PDDC_OK;
}

int pddc_blanker_delay(const pddc_blanker *b)
{
    if (!b)
        return null_argument();
    return b->par.guard + b->par.ramp;
}

int pddc_blanker_process(pddc_blanker *b, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                         void *stream)
{
    if (!b)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_out, 8, "d_out"));
    }
    if (over_capacity(n, z_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "blanker: %zu samples per receiver, z_stride %zu, out_stride %zu", n, z_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    if (ranges_overlap(d_out, rows_extent(b->nrx, n, out_stride, 8), d_z, rows_extent(b->nrx, n, z_stride, 8)))
        return pddc_set_error_(PDDC_EINVAL, "blanker: out overlaps z (there is no in-place form: out[n] is made from z[n - D])");
    PDDC_TRY(set_device(b->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(b->table.upload(st));
    BlankerArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.out = static_cast<float2 *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = b->table.dev();
    a.nrx = b->nrx;
    a.old = b->state.old();
    a.new_state = b->state.next();
    a.old_hist = b->hist.old();
    a.new_hist = b->hist.next();
    a.old_bits = b->bits.old();
    a.new_bits = b->bits.next();
    a.B = (uint32_t)b->par.block;
    a.W = (uint32_t)b->par.guard;
    a.D = (uint32_t)(b->par.guard + b->par.ramp);
    a.ph0 = (uint32_t)(b->N % (uint64_t)b->par.block);
    a.magic = meter_magic(a.B);
    a.invB = b->invB;
    a.invR1 = b->invR1;
    a.beta = b->par.beta;
    a.cap = b->par.cap;
    a.fresh = b->fresh ? 1u : 0u;
    PDDC_HIP_TRY(launch_blanker(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    b->state.turn();
    b->hist.turn();
    b->bits.turn();
    b->N += n;
    b->fresh = false;
    return PDDC_OK;
}

int pddc_blanker_read(pddc_blanker *b, pddc_blanker_status *host, void *stream)
{
    if (!b || !host)
        return null_argument();
    PDDC_TRY(set_device(b->device));
    PDDC_TRY(read_back(b->host_state.data(), b->fresh ? nullptr : b->state.old(), (size_t)b->nrx, (hipStream_t)stream));
    for (int j = 0; j < b->nrx; ++j) {
        const BlankerState &r = b->host_state[(size_t)j];
        host[j] = b->fresh ? pddc_blanker_status{ 0.0f, 0u, 0u } : pddc_blanker_status{ r.ref, r.triggers, r.blanked };
    }
    return PDDC_OK;
}

} // extern "C"
