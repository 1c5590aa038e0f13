/*
 * ddc_carrier.cpp -- host side of the carrier stage (include/perseus_ddc.h, pddc_carrier_*): the object, its receiver
 * table, the launch of a batch and the status read.  The kernel is in ddc_carrier.hip.
 * What is carried per receiver (theta, v, q and the last L - 1 values of w) lives on the device in two pairs of
 * records, read and written in turn; nothing on the device is cleared from the host: the "fresh" mark (create, reset,
 * a change of mode: the records are not read, their values are zero) lives in the table, which is uploaded in stream
 * order when it changed.  The Hilbert taps are uploaded once, at create.
 */
#include "ddc_stage.h"
#include "ddc_carrier.h"

#include <cmath>

using namespace pddc;

struct pddc_carrier : StageBase {
    PDDC_LOCAL ~pddc_carrier() = default;
    pddc_carrier_params par{};
    int L = 0;
    RxTable<CarrierRx> table;                       /* flags carry kCarrierFresh                                   */
    DevBuf<float> taps;                             /* [kCarrierTapSlots]                                          */
    std::vector<CarrierState> host_state;           /* where read() lands the records                              */
    bool launched = false;                          /* a batch since create / reset: the records were written      */
    Carried<CarrierState> state;
    Carried<float2> hist;                           /* [nrx][L - 1]                                                */
    uint64_t m = 0;                                 /* outputs per receiver since create / reset                   */
};

static_assert(PDDC_CARRIER_OFF == kCarrierOff && PDDC_CARRIER_DSB == kCarrierDsb && PDDC_CARRIER_USB == kCarrierUsb &&
                  PDDC_CARRIER_LSB == kCarrierLsb && kCarrierModes == 4,
              "the kernel's mode numbers are the header's");

/* written so that a NaN fails it */
static bool carrier_rx_ok(int mode, float kp, float ki)
{
    return mode >= 0 && (uint32_t)mode < kCarrierModes && kp > 0.0f && kp <= 0.5f && ki >= 0.0f && ki <= 0.25f;
}

extern "C" {

int pddc_carrier_tile_outputs(void) { return kCarrierTile; }

int pddc_carrier_group(void) { return kCarrierGroup; }

int pddc_carrier_create(pddc_carrier **out, int device, int nrx, const pddc_carrier_params *par, const pddc_carrier_rx *rx,
                        const float *hilbert, int ntaps)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kCarrierMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "carrier: %d receivers (1 .. %d) and their modes", nrx, kCarrierMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "carrier: null parameters");
    if (!(par->vmax > 0.0f && par->vmax < 0.5f) || !(par->gamma > 0.0f && par->gamma <= 1.0f) ||
        !(par->lock_thr > 0.0f && par->lock_thr <= 3.4028234e38f))
        return pddc_set_error_(PDDC_EINVAL, "carrier: vmax %g (0 < . < 0.5), gamma %g (0 < . <= 1), lock_thr %g (finite, > 0)",
                               (double)par->vmax, (double)par->gamma, (double)par->lock_thr);
    if (!hilbert || ntaps < 3 || ntaps > kCarrierMaxTaps || !(ntaps & 1))
        return pddc_set_error_(PDDC_EINVAL, "carrier: %d Hilbert taps (odd, 3 .. %d)", ntaps, kCarrierMaxTaps);
    for (int k = 0; k < ntaps; ++k)
        if (!std::isfinite(hilbert[k]))
            return pddc_set_error_(PDDC_EINVAL, "carrier: tap %d is not finite", k);
    for (int j = 0; j < nrx; ++j)
        if (!carrier_rx_ok(rx[j].mode, rx[j].kp, rx[j].ki))
            return pddc_set_error_(PDDC_EINVAL, "carrier: receiver %d: mode %d, kp %g (0 < . <= 0.5), ki %g (0 .. 0.25)", j,
                                   rx[j].mode, (double)rx[j].kp, (double)rx[j].ki);
    return stage_create(out, device, nrx, [&](pddc_carrier &c) {
        c.par = *par;
        c.L = ntaps;
        c.host_state.resize((size_t)nrx);
        for (int j = 0; j < nrx; ++j)
            c.table.host.push_back(CarrierRx{ (uint32_t)rx[j].mode, rx[j].kp, rx[j].ki, kCarrierFresh });
        std::vector<float> h((size_t)kCarrierTapSlots, 0.0f);
        for (int k = 0; k < ntaps; ++k)
            h[(size_t)k] = hilbert[k];
        PDDC_TRY(c.taps.alloc_copy(h));
        PDDC_TRY(c.table.alloc());
        PDDC_TRY(c.state.alloc((size_t)nrx));
        return c.hist.alloc((size_t)nrx * (size_t)(ntaps - 1));
    });
}

int pddc_carrier_destroy(pddc_carrier *c) { return stage_destroy(c); }

int pddc_carrier_reset(pddc_carrier *c)
{
    PDDC_TRY(stage_quiesce(c));
    c->m = 0;
    c->launched = false;
    for (CarrierRx &r : c->table.host)
        r.flags |= kCarrierFresh;
    c->table.dirty = true;
    return PDDC_OK;
}

int pddc_carrier_set_rx(pddc_carrier *c, int rx, int mode, float kp, float ki)
{
    PDDC_TRY(stage_rx_ok(c, "carrier", rx));
    if (!carrier_rx_ok(mode, kp, ki))
        return pddc_set_error_(PDDC_EINVAL, "carrier: mode %d, kp %g (0 < . <= 0.5), ki %g (0 .. 0.25)", mode, (double)kp,
                               (double)ki);
    CarrierRx &r = c->table.host[(size_t)rx];
    /* another mode: theta, v, q and the w history return to their create values, m goes on; the gains alone: nothing
     * carried is touched */
    if ((uint32_t)mode != r.mode)
        r.flags |= kCarrierFresh;
    r.mode = (uint32_t)mode;
    r.kp = kp;
    r.ki = ki;
    c->table.dirty = true;
    return PDDC_OK;
}

int pddc_carrier_process(pddc_carrier *c, const void *d_z, size_t n, size_t z_stride, void *d_u, size_t u_stride, void *stream)
{
    if (!c)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_u, 8, "d_u"));
    }
    if (over_capacity(n, z_stride, u_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "carrier: %zu outputs per receiver, z_stride %zu, u_stride %zu", n, z_stride,
                               u_stride);
    if (!n)
        return PDDC_OK;
    if (!(d_u == d_z && u_stride == z_stride) &&
        ranges_overlap(d_u, rows_extent(c->nrx, n, u_stride, 8), d_z, rows_extent(c->nrx, n, z_stride, 8)))
        return pddc_set_error_(PDDC_EINVAL, "carrier: u overlaps z (in place is u == z with equal strides)");
    PDDC_TRY(set_device(c->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(c->table.upload(st));
    CarrierArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.u = static_cast<float2 *>(d_u);
    a.u_stride = (long long)u_stride;
    a.n = (long long)n;
    a.rx = c->table.dev();
    a.nrx = c->nrx;
    a.old = c->state.old();
    a.new_state = c->state.next();
    a.old_hist = c->hist.old();
    a.new_hist = c->hist.next();
    a.taps = c->taps.get();
    a.L = c->L;
    a.vmax = c->par.vmax;
    a.gamma = c->par.gamma;
    PDDC_HIP_TRY(launch_carrier(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    c->state.turn();
    c->hist.turn();
    c->m += n;
    c->launched = true;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    for (CarrierRx &r : c->table.host)
        if (r.flags & kCarrierFresh) {
            r.flags &= ~kCarrierFresh;
            c->table.dirty = true;
        }
    return PDDC_OK;
}

int pddc_carrier_read(pddc_carrier *c, pddc_carrier_status *host, void *stream)
{
    if (!c || !host)
        return null_argument();
    PDDC_TRY(set_device(c->device));
    PDDC_TRY(read_back(c->host_state.data(), c->launched ? c->state.old() : nullptr, (size_t)c->nrx, (hipStream_t)stream));
    for (int j = 0; j < c->nrx; ++j) {
        /* a receiver whose mode changed since the last batch has its create values */
        const bool fresh = !c->launched || (c->table.host[(size_t)j].flags & kCarrierFresh);
        const CarrierState r = fresh ? CarrierState{ 0u, 0.0f, 0.0f, 0u } : c->host_state[(size_t)j];
        host[j] = pddc_carrier_status{ r.theta, r.v, r.q, r.q < c->par.lock_thr ? 1u : 0u };
    }
    return PDDC_OK;
}

} // extern "C"
