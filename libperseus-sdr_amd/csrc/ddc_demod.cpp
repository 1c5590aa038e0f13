/*
 * ddc_demod.cpp -- host side of the demodulator (include/perseus_ddc.h, pddc_demod_*): the object, its receiver table,
 * the output counter and the launch of a batch.  The kernel is in ddc_demod.hip.
 * What is carried per receiver (z, d, y, e of the last output) lives on the device in two records, read and written in
 * turn; psi and the "fresh" mark (create, reset, a mode or flag change: the record is not read, its values are zero)
 * live in the table, which is uploaded in stream order when it changed.
 */
#include "ddc_host.h"
#include "ddc_demod.h"

#include <algorithm>
#include <new>
#include <vector>

using namespace pddc;

struct pddc_demod {
    int device = 0;
    int nrx = 0;
    int target_blocks = 0;
    pddc_demod_params par{};
    std::vector<DemodRx> table;                     /* flags carry kDemodFresh; uploaded when `dirty`             */
    std::vector<DemodRx> staged;                    /* the copy an upload reads: touched by the next upload only  */
    bool dirty = true;
    DemodRx *d_table = nullptr;
    DemodState *d_state[2] = { nullptr, nullptr };  /* process() reads [cur] and writes [cur ^ 1]                 */
    int cur = 0;
    uint64_t m = 0;                                 /* outputs per receiver since create / reset                  */
};

static_assert(PDDC_DEMOD_AM == 0 && PDDC_DEMOD_FM == 1 && PDDC_DEMOD_SSB == 2 && kDemodModes == 3,
              "the kernel's mode numbers are the header's");
static_assert(PDDC_DEMOD_DCBLOCK == kDemodDc && PDDC_DEMOD_AGC == kDemodAgc, "the kernel's flag bits are the header's");

static bool demod_rx_ok(int mode, uint32_t flags)
{
    return mode >= 0 && (uint32_t)mode < kDemodModes && !(flags & ~(kDemodDc | kDemodAgc));
}

static void demod_free(pddc_demod *d)
{
    hipFree(d->d_table);
    hipFree(d->d_state[0]);
    hipFree(d->d_state[1]);
    delete d;
}

static int demod_alloc(pddc_demod *d)
{
    PDDC_HIP_TRY(hipSetDevice(d->device));
    int ncu = 0;
    PDDC_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, d->device));
    d->target_blocks = 4 * (ncu > 0 ? ncu : 256);
    const size_t bytes = sizeof(DemodState) * (size_t)d->nrx;
    PDDC_HIP_TRY(hipMalloc(&d->d_table, sizeof(DemodRx) * (size_t)d->nrx));
    PDDC_HIP_TRY(hipMalloc(&d->d_state[0], bytes));
    PDDC_HIP_TRY(hipMalloc(&d->d_state[1], bytes));
    PDDC_HIP_TRY(hipMemset(d->d_state[0], 0, bytes));
    PDDC_HIP_TRY(hipMemset(d->d_state[1], 0, bytes));
    return PDDC_OK;
}

extern "C" {

int pddc_demod_tile_outputs(void) { return kDemodTile; }

int pddc_demod_create(pddc_demod **out, int device, int nrx, const pddc_demod_rx *rx, const pddc_demod_params *par)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
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
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_demod *d = new (std::nothrow) pddc_demod;
    if (!d)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    d->device = device;
    d->nrx = nrx;
    d->par = *par;
    d->table.resize((size_t)nrx);
    for (int j = 0; j < nrx; ++j)
        d->table[(size_t)j] = DemodRx{ (uint32_t)rx[j].mode, rx[j].bfo, 0u, rx[j].flags | kDemodFresh };
    const int rc = demod_alloc(d);
    if (rc) {
        demod_free(d);
        return rc;
    }
    *out = d;
    return PDDC_OK;
}

int pddc_demod_destroy(pddc_demod *d)
{
    if (!d)
        return PDDC_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    demod_free(d);
    return PDDC_OK;
}

int pddc_demod_reset(pddc_demod *d)
{
    if (!d)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(d->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    d->m = 0;
    for (DemodRx &r : d->table) {
        r.psi = 0u;
        r.flags |= kDemodFresh;
    }
    d->dirty = true;
    return PDDC_OK;
}

int pddc_demod_set_rx(pddc_demod *d, int rx, int mode, uint32_t bfo, uint32_t flags)
{
    if (!d)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (rx < 0 || rx >= d->nrx)
        return pddc_set_error_(PDDC_EINVAL, "demod: receiver %d (0 .. %d)", rx, d->nrx - 1);
    if (!demod_rx_ok(mode, flags))
        return pddc_set_error_(PDDC_EINVAL, "demod: mode %d, flags 0x%x", mode, flags);
    DemodRx &r = d->table[(size_t)rx];
    if ((uint32_t)mode != r.mode || flags != (r.flags & ~kDemodFresh)) {
        /* another detector or post stage: the carried values return to their create values, m goes on */
        r = DemodRx{ (uint32_t)mode, bfo, 0u, flags | kDemodFresh };
    } else {
        /* the word alone: the increment changes at the next output m0, the phase does not (the tuner's rule) */
        r.psi += (r.beta - bfo) * (uint32_t)d->m;
        r.beta = bfo;
    }
    d->dirty = true;
    return PDDC_OK;
}

int pddc_demod_process(pddc_demod *d, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride, void *stream)
{
    if (!d)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (n && (!d_z || ((uintptr_t)d_z & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_z must be an 8-byte aligned device pointer");
    if (n && (!d_out || ((uintptr_t)d_out & 3)))
        return pddc_set_error_(PDDC_EINVAL, "d_out must be a 4-byte aligned device pointer");
    if (n > z_stride || n > out_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "demod: %zu outputs per receiver, z_stride %zu, out_stride %zu", n, z_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    PDDC_HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = (hipStream_t)stream;
    if (d->dirty) {
        d->staged = d->table;
        PDDC_HIP_TRY(hipMemcpyAsync(d->d_table, d->staged.data(), sizeof(DemodRx) * (size_t)d->nrx, hipMemcpyHostToDevice, st));
    }
    DemodArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.out = static_cast<float *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = d->d_table;
    a.nrx = d->nrx;
    a.state = d->d_state[d->cur];
    a.new_state = d->d_state[d->cur ^ 1];
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
            any |= d->table[(size_t)j].flags;
        plain_group = !(any & (kDemodDc | kDemodAgc));
    }
    const long long groups = (d->nrx + G - 1) / G;
    const long long runs = plain_group ? std::max(1LL, (long long)d->target_blocks / groups) : 1LL;
    const long long run = ((long long)n + runs - 1) / runs;
    a.run = (run + kDemodTile - 1) / kDemodTile * kDemodTile;
    PDDC_HIP_TRY(launch_demod(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    d->cur ^= 1;
    d->m += n;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    bool fresh = false;
    for (DemodRx &r : d->table) {
        fresh |= (r.flags & kDemodFresh) != 0u;
        r.flags &= ~kDemodFresh;
    }
    d->dirty = fresh;
    return PDDC_OK;
}

} // extern "C"
