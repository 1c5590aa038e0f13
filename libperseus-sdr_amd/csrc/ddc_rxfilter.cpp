/*
 * ddc_rxfilter.cpp -- host side of the receiver filter (include/perseus_ddc.h, pddc_rxfilter_*): the object, its bank
 * and receiver table, the output counter and the launch of a batch.  The kernel is in ddc_rxfilter.hip.
 * What is carried per receiver (its last T - 1 inputs) lives on the device in two records, read and written in turn;
 * the filter index and the "fresh" mark (create, reset: the record is not read, its values are zero) live in the table,
 * which is uploaded in stream order when it changed.  The bank is uploaded once, at create.
 */
#include "ddc_stage.h"
#include "ddc_rxfilter.h"

#include <cmath>

using namespace pddc;

struct pddc_rxfilter : StageBase {
    PDDC_LOCAL ~pddc_rxfilter() = default;
    int nfilters = 0, taps = 0;
    RxTable<RxfRx> table;
    DevBuf<float> bank;                             /* [nfilters][rxf_row(T)]                                     */
    Carried<float2> state;                          /* [nrx][T - 1]                                               */
    uint64_t m = 0;                                 /* outputs per receiver since create / reset                  */
};

extern "C" {

int pddc_rxfilter_tile_outputs(void) { return kRxfTile; }

int pddc_rxfilter_create(pddc_rxfilter **out, int device, int nrx, const float *bank, int nfilters, int ntaps, const int *sel)
{
    if (!out)
        return null_argument();
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
    return stage_create(out, device, nrx, [&](pddc_rxfilter &f) {
        f.nfilters = nfilters;
        f.taps = ntaps;
        for (int j = 0; j < nrx; ++j)
            f.table.host.push_back(RxfRx{ sel[j], 1u });
        const size_t row = (size_t)rxf_row(ntaps);
        std::vector<float> rows((size_t)nfilters * row, 0.0f);
        for (int b = 0; b < nfilters; ++b)
            for (int t = 0; t < ntaps; ++t)
                rows[(size_t)b * row + kRxfPad + (size_t)t] = bank[(size_t)b * (size_t)ntaps + (size_t)t];
        PDDC_TRY(f.bank.alloc_copy(rows));
        PDDC_TRY(f.table.alloc());
        return f.state.alloc((size_t)nrx * (size_t)(ntaps > 1 ? ntaps - 1 : 1));
    });
}

int pddc_rxfilter_destroy(pddc_rxfilter *f) { return stage_destroy(f); }

int pddc_rxfilter_reset(pddc_rxfilter *f)
{
    PDDC_TRY(stage_quiesce(f));
    f->m = 0;
    for (RxfRx &r : f->table.host)
        r.fresh = 1u;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_rxfilter_set_rx(pddc_rxfilter *f, int rx, int filter)
{
    PDDC_TRY(stage_rx_ok(f, "rxfilter", rx));
    if (filter < 0 || filter >= f->nfilters)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: filter %d (0 .. %d)", filter, f->nfilters - 1);
    /* the carried inputs stay: from the next output on the new taps run over them */
    f->table.host[(size_t)rx].filter = filter;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_rxfilter_process(pddc_rxfilter *f, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                          void *stream)
{
    if (!f)
        return null_argument();
    if (n && !(aligned_ptr(d_z, 8) && aligned_ptr(d_out, 8)))
        return pddc_set_error_(PDDC_EINVAL, "d_z and d_out must be 8-byte aligned device pointers");
    if (over_capacity(n, z_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "rxfilter: %zu values per receiver, z_stride %zu, out_stride %zu", n, z_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    if (n > (size_t)1 << 40 || z_stride > (size_t)1 << 40 || out_stride > (size_t)1 << 40)
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: %zu values per receiver are too many for one batch", n);
    /* tiles read their neighbours' inputs: the bytes read and the bytes written must not meet */
    if (ranges_overlap(d_z, rows_extent(f->nrx, n, z_stride, sizeof(float2)), d_out,
                       rows_extent(f->nrx, n, out_stride, sizeof(float2))))
        return pddc_set_error_(PDDC_EINVAL, "rxfilter: input and output overlap (in place is not supported)");
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(f->table.upload(st));
    RxfArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.out = static_cast<float2 *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.bank = f->bank.get();
    a.rx = f->table.dev();
    a.state = f->state.old();
    a.new_state = f->state.next();
    a.nrx = f->nrx;
    a.nfilters = f->nfilters;
    a.taps = f->taps;
    PDDC_HIP_TRY(launch_rxfilter(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    f->state.turn();
    f->m += n;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    for (RxfRx &r : f->table.host)
        if (r.fresh) {
            r.fresh = 0u;
            f->table.dirty = true;
        }
    return PDDC_OK;
}

} // extern "C"
