/*
 * ddc_rxfilter.cpp -- host side of the receiver filter (include/perseus_ddc.h, pddc_rxfilter_*): the object, its bank
 * and receiver table, the output counter and the launch of a batch.  The kernel is in ddc_rxfilter.hip.
 * What is carried per receiver (its last T - 1 inputs) lives on the device in two records, read and written in turn;
 * the filter index and the "fresh" mark (create, reset: the record is not read, its values are zero) live in the table,
 * which is uploaded in stream order when it changed.  The bank is uploaded once, at create.
 */
#include "ddc_host.h"
#include "ddc_rxfilter.h"

#include <cmath>
#include <new>
#include <vector>

using namespace pddc;

struct pddc_rxfilter {
    int device = 0;
    int nrx = 0, nfilters = 0, taps = 0;
    std::vector<RxfRx> table;                       /* uploaded when `dirty`                                      */
    std::vector<RxfRx> staged;                      /* the copy an upload reads: touched by the next upload only  */
    bool dirty = true;
    float *d_bank = nullptr;                        /* [nfilters][rxf_row(T)]                                     */
    RxfRx *d_table = nullptr;
    float2 *d_state[2] = { nullptr, nullptr };      /* [nrx][T - 1]; process() reads [cur] and writes [cur ^ 1]   */
    int cur = 0;
    uint64_t m = 0;                                 /* outputs per receiver since create / reset                  */
};

static void rxfilter_free(pddc_rxfilter *f)
{
    hipFree(f->d_bank);
    hipFree(f->d_table);
    hipFree(f->d_state[0]);
    hipFree(f->d_state[1]);
    delete f;
}

static int rxfilter_alloc(pddc_rxfilter *f, const std::vector<float> &rows)
{
    PDDC_HIP_TRY(hipSetDevice(f->device));
    const size_t bytes = sizeof(float2) * (size_t)f->nrx * (size_t)(f->taps > 1 ? f->taps - 1 : 1);
    PDDC_HIP_TRY(hipMalloc(&f->d_bank, sizeof(float) * rows.size()));
    PDDC_HIP_TRY(hipMalloc(&f->d_table, sizeof(RxfRx) * (size_t)f->nrx));
    PDDC_HIP_TRY(hipMalloc(&f->d_state[0], bytes));
    PDDC_HIP_TRY(hipMalloc(&f->d_state[1], bytes));
    PDDC_HIP_TRY(hipMemcpy(f->d_bank, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice));
    PDDC_HIP_TRY(hipMemset(f->d_state[0], 0, bytes));
    PDDC_HIP_TRY(hipMemset(f->d_state[1], 0, bytes));
    return PDDC_OK;
}

extern "C" {

int pddc_rxfilter_tile_outputs(void) { return kRxfTile; }

int pddc_rxfilter_create(pddc_rxfilter **out, int device, int nrx, const float *bank, int nfilters, int ntaps, const int *sel)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (nrx < 1 || nrx > kRxfMaxRx)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: %d receivers (1 .. %d)", nrx, kRxfMaxRx);
    if (nfilters < 1 || nfilters > kRxfMaxFilters || ntaps < 1 || ntaps > kRxfMaxTaps)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: %d filters (1 .. %d) of %d taps (1 .. %d)", nfilters, kRxfMaxFilters,
                               ntaps, kRxfMaxTaps);
    if (!bank || !sel)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: null bank or filter indices");
    for (int i = 0; i < nfilters * ntaps; ++i)
        if (!std::isfinite(bank[i]))
            return pddc_set_error_(PDDC_EINVAL, "rxfilter: tap %d of filter %d is not finite", i % ntaps, i / ntaps);
    for (int j = 0; j < nrx; ++j)
        if (sel[j] < 0 || sel[j] >= nfilters)
            return pddc_set_error_(PDDC_EINVAL, "rxfilter: receiver %d: filter %d (0 .. %d)", j, sel[j], nfilters - 1);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_rxfilter *f = new (std::nothrow) pddc_rxfilter;
    if (!f)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    f->device = device;
    f->nrx = nrx;
    f->nfilters = nfilters;
    f->taps = ntaps;
    f->table.resize((size_t)nrx);
    for (int j = 0; j < nrx; ++j)
        f->table[(size_t)j] = RxfRx{ sel[j], 1u };
    const size_t row = (size_t)rxf_row(ntaps);
    std::vector<float> rows((size_t)nfilters * row, 0.0f);
    for (int b = 0; b < nfilters; ++b)
        for (int t = 0; t < ntaps; ++t)
            rows[(size_t)b * row + kRxfPad + (size_t)t] = bank[(size_t)b * (size_t)ntaps + (size_t)t];
    const int rc = rxfilter_alloc(f, rows);
    if (rc) {
        rxfilter_free(f);
        return rc;
    }
    *out = f;
    return PDDC_OK;
}

int pddc_rxfilter_destroy(pddc_rxfilter *f)
{
    if (!f)
        return PDDC_OK;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();
    rxfilter_free(f);
    return PDDC_OK;
}

int pddc_rxfilter_reset(pddc_rxfilter *f)
{
    if (!f)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(f->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    f->m = 0;
    for (RxfRx &r : f->table)
        r.fresh = 1u;
    f->dirty = true;
    return PDDC_OK;
}

int pddc_rxfilter_set_rx(pddc_rxfilter *f, int rx, int filter)
{
    if (!f)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (rx < 0 || rx >= f->nrx)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: receiver %d (0 .. %d)", rx, f->nrx - 1);
    if (filter < 0 || filter >= f->nfilters)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: filter %d (0 .. %d)", filter, f->nfilters - 1);
    /* the carried inputs stay: from the next output on the new taps run over them */
    f->table[(size_t)rx].filter = filter;
    f->dirty = true;
    return PDDC_OK;
}

int pddc_rxfilter_process(pddc_rxfilter *f, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                          void *stream)
{
    if (!f)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (n && (!d_z || ((uintptr_t)d_z & 7) || !d_out || ((uintptr_t)d_out & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_z and d_out must be 8-byte aligned device pointers");
    if (n > z_stride || n > out_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "rxfilter: %zu values per receiver, z_stride %zu, out_stride %zu", n, z_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    if (n > (size_t)1 << 40 || z_stride > (size_t)1 << 40 || out_stride > (size_t)1 << 40)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: %zu values per receiver are too many for one batch", n);
    /* tiles read their neighbours' inputs: the bytes read and the bytes written must not meet */
    const uintptr_t z0 = (uintptr_t)d_z, z1 = z0 + ((size_t)(f->nrx - 1) * z_stride + n) * sizeof(float2);
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((size_t)(f->nrx - 1) * out_stride + n) * sizeof(float2);
    if (z0 < o1 && o0 < z1)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: input and output overlap (in place is not supported)");
    PDDC_HIP_TRY(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (f->dirty) {
        f->staged = f->table;
        PDDC_HIP_TRY(hipMemcpyAsync(f->d_table, f->staged.data(), sizeof(RxfRx) * (size_t)f->nrx, hipMemcpyHostToDevice, st));
    }
    RxfArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.out = static_cast<float2 *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.bank = f->d_bank;
    a.rx = f->d_table;
    a.state = f->d_state[f->cur];
    a.new_state = f->d_state[f->cur ^ 1];
    a.nrx = f->nrx;
    a.nfilters = f->nfilters;
    a.taps = f->taps;
    PDDC_HIP_TRY(launch_rxfilter(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    f->cur ^= 1;
    f->m += n;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    bool fresh = false;
    for (RxfRx &r : f->table) {
        fresh |= r.fresh != 0u;
        r.fresh = 0u;
    }
    f->dirty = fresh;
    return PDDC_OK;
}

} // extern "C"
