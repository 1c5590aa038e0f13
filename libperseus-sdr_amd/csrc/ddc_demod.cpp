/*
 * ddc_demod.cpp -- host side of the demodulator (include/perseus_ddc.h, pddc_demod_*): the object, its receiver table,
 * the output counter and the launch of a batch.  The kernel is in ddc_demod.hip.
 * What is carried per receiver (z, d, y, e of the last output) lives on the device in two records, read and written in
 * turn; psi and the "fresh" mark (create, reset, a mode or flag change: the record is not read, its values are zero)
 * live in the table, which is uploaded in stream order when it changed.
 */
#include "ddc_stage.h"
#include "ddc_demod.h"

#include <algorithm>

using namespace pddc;

struct pddc_demod : StageBase {
    PDDC_LOCAL ~pddc_demod() = default;
    int target_blocks = 0;
    pddc_demod_params par{};
    RxTable<DemodRx> table;                         /* flags carry kDemodFresh                                    */
    Carried<DemodState> state;
    uint64_t m = 0;                                 /* outputs per receiver since create / reset                  */
};

static_assert(PDDC_DEMOD_AM == 0 && PDDC_DEMOD_FM == 1 && PDDC_DEMOD_SSB == 2 && kDemodModes == 3,
              "the kernel's mode numbers are the header's");
static_assert(PDDC_DEMOD_DCBLOCK == kDemodDc && PDDC_DEMOD_AGC == kDemodAgc, "the kernel's flag bits are the header's");

static bool demod_rx_ok(int mode, uint32_t flags)
{
    return mode >= 0 && (uint32_t)mode < kDemodModes && !(flags & ~(kDemodDc | kDemodAgc));
}

extern "C" {

int pddc_demod_tile_outputs(void) { return kDemodTile; }

int pddc_demod_create(pddc_demod **out, int device, int nrx, const pddc_demod_rx *rx, const pddc_demod_params *par)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kDemodMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "demod: %d receivers (1 .. %d) and their modes", nrx, kDemodMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "demod: null parameters");
    /* written so that a NaN fails them */
    if (!(par->rho >= 0.0f && par->rho < 1.0f) || !(par->lambda >= 0.0f && par->lambda < 1.0f) ||
        !(par->target > 0.0f && par->target <= 3.0e38f) || !(par->gmax > 0.0f && par->gmax <= 3.0e38f))
        return pddc_set_error_(PDDC_EINVAL, "demod: rho %g, lambda %g (0 <= . < 1), target %g, gmax %g (finite, > 0)",
                               (double)par->rho, (double)par->lambda, (double)par->target, (double)par->gmax);
    for (int j = 0; j < nrx; ++j)
        if (!demod_rx_ok(rx[j].mode, rx[j].flags))
            return pddc_set_error_(PDDC_EINVAL, "demod: receiver %d: mode %d, flags 0x%x", j, rx[j].mode, rx[j].flags);
    return stage_create(out, device, nrx, [&](pddc_demod &d) {
        d.par = *par;
        for (int j = 0; j < nrx; ++j)
            d.table.host.push_back(DemodRx{ (uint32_t)rx[j].mode, rx[j].bfo, 0u, rx[j].flags | kDemodFresh });
        int ncu = 0;
        PDDC_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
        d.target_blocks = 4 * (ncu > 0 ? ncu : 256);
        PDDC_TRY(d.table.alloc());
        return d.state.alloc((size_t)nrx);
    });
}

int pddc_demod_destroy(pddc_demod *d) { return stage_destroy(d); }

int pddc_demod_reset(pddc_demod *d)
{
    PDDC_TRY(stage_quiesce(d));
    d->m = 0;
    for (DemodRx &r : d->table.host) {
        r.psi = 0u;
        r.flags |= kDemodFresh;
    }
    d->table.dirty = true;
    return PDDC_OK;
}

int pddc_demod_set_rx(pddc_demod *d, int rx, int mode, uint32_t bfo, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(d, "demod", rx));
    if (!demod_rx_ok(mode, flags))
        return pddc_set_error_(PDDC_EINVAL, "demod: mode %d, flags 0x%x", mode, flags);
    DemodRx &r = d->table.host[(size_t)rx];
    if ((uint32_t)mode != r.mode || flags != (r.flags & ~kDemodFresh)) {
        /* another detector or post stage: the carried values return to their create values, m goes on */
        r = DemodRx{ (uint32_t)mode, bfo, 0u, flags | kDemodFresh };
    } else {
        /* the word alone: the increment changes at the next output m0, the phase does not (the tuner's rule) */
        r.psi += (r.beta - bfo) * (uint32_t)d->m;
        r.beta = bfo;
    }
    d->table.dirty = true;
    return PDDC_OK;
}

int pddc_demod_process(pddc_demod *d, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride, void *stream)
{
    if (!d)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_out, 4, "d_out"));
    }
    if (over_capacity(n, z_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "demod: %zu outputs per receiver, z_stride %zu, out_stride %zu", n, z_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    PDDC_TRY(set_device(d->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(d->table.upload(st));
    DemodArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.out = static_cast<float *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = d->table.dev();
    a.nrx = d->nrx;
    a.state = d->state.old();
    a.new_state = d->state.next();
    a.m0 = (uint32_t)d->m;
    a.rho = d->par.rho;
    a.lambda = d->par.lambda;
    a.target = d->par.target;
    a.gmax = d->par.gmax;
    /* runs matter to the groups without a post stage only: the batch spread over the blocks that keep the device busy.
     * If every group has one, a single run (its blocks x > 0 would leave at once) */
    const int G = kDemodGroup;
    bool plain_group = false;
    for (int g0 = 0; g0 < d->nrx && !plain_group; g0 += G) {
        uint32_t any = 0u;
        for (int j = g0; j < std::min(g0 + G, d->nrx); ++j)
            any |= d->table.host[(size_t)j].flags;
        plain_group = !(any & (kDemodDc | kDemodAgc));
    }
    const long long groups = (d->nrx + G - 1) / G;
    const long long runs = plain_group ? std::max(1LL, (long long)d->target_blocks / groups) : 1LL;
    const long long run = ((long long)n + runs - 1) / runs;
    a.run = (run + kDemodTile - 1) / kDemodTile * kDemodTile;
    PDDC_HIP_TRY(launch_demod(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    d->state.turn();
    d->m += n;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    for (DemodRx &r : d->table.host)
        if (r.flags & kDemodFresh) {
            r.flags &= ~kDemodFresh;
            d->table.dirty = true;
        }
    return PDDC_OK;
}

} // extern "C"
