/*
 * ddc_channelizer.cpp -- host side of the channelizer (include/perseus_ddc.h, pddc_channelizer_*): the object, its
 * counters, and the two launches of a batch.  The carried tail is a PackedCarry (ddc_packed.h); the kernels are in
 * ddc_channelizer.hip.
 * List mode: the list lives on the host; the kernel reads slot[bin] (the column of bin k, -1: not listed).  A new list's
 * table is uploaded by the next process() that has rows, on its stream -- ordered behind the launch before it, which
 * therefore never sees it (one stream per object) -- as the tuner uploads its receiver table.
 */
#include "ddc_channelizer.h"
#include "ddc_kernels.h"
#include "ddc_spectrum.h"

#include <new>
#include <vector>

using namespace pddc;

struct pddc_channelizer {
    int device = 0;
    int nchan = 0, hop = 0, proto_len = 0;
    int first = 0, count = 0;                       /* list mode: count = channels.size()                         */
    std::vector<int> channels;                      /* list mode: the list; empty: range mode                     */
    std::vector<short> h_slot;                      /* the slot table; rebuilt and uploaded when `slot_dirty`     */
    short *d_slot = nullptr;
    bool slot_dirty = false;
    int target_blocks = 0, target_blocks_list = 0;
    float *d_proto = nullptr, *d_tw = nullptr;
    PackedCarry in;                                 /* the carried tail (a window of proto_len) and the stream length */
    uint64_t rows = 0;                              /* rows delivered since create / reset     */
};

static bool chan_sizes_ok(int nchan, int hop, int proto_len)
{
    if (nchan != 1024 && nchan != 2048 && nchan != 4096)
        return false;
    if (hop != nchan && hop != nchan / 2)
        return false;
    if (proto_len <= 0 || proto_len > kChanMaxProto || proto_len % nchan)
        return false;
    const int p = proto_len / nchan;
    return p == 1 || p == 2 || p == 4 || p == 8;
}

static void chan_free(pddc_channelizer *c)
{
    hipFree(c->d_proto);
    hipFree(c->d_tw);
    hipFree(c->d_slot);
    c->in.free();
    delete c;
}

static int chan_create(pddc_channelizer *c, const float *proto)
{
    PDDC_HIP_TRY(hipSetDevice(c->device));
    int ncu = 0;
    PDDC_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
    c->target_blocks = channelize_target_blocks(c->nchan, c->proto_len / c->nchan, c->hop, ncu > 0 ? ncu : 256);
    c->target_blocks_list = channelize_target_blocks(c->nchan, c->proto_len / c->nchan, c->hop, ncu > 0 ? ncu : 256, true);
    std::vector<float> tw((size_t)spectrum_twiddle_len(c->nchan));
    spectrum_build_twiddles(c->nchan, tw.data());
    PDDC_HIP_TRY(hipMalloc(&c->d_proto, (size_t)c->proto_len * sizeof(float)));
    PDDC_HIP_TRY(hipMalloc(&c->d_tw, tw.size() * sizeof(float)));
    PDDC_HIP_TRY(c->in.alloc((size_t)c->proto_len));
    PDDC_HIP_TRY(hipMalloc(&c->d_slot, (size_t)c->nchan * sizeof(short)));
    PDDC_HIP_TRY(hipMemcpy(c->d_proto, proto, (size_t)c->proto_len * sizeof(float), hipMemcpyHostToDevice));
    PDDC_HIP_TRY(hipMemcpy(c->d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
    return PDDC_OK;
}

extern "C" {

uint64_t pddc_channelizer_rows(int nchan, int hop, int proto_len, uint64_t samples_before, size_t nsamples)
{
    if (!chan_sizes_ok(nchan, hop, proto_len))
        return 0;
    return windows_complete(proto_len, hop, samples_before + nsamples) - windows_complete(proto_len, hop, samples_before);
}

uint64_t pddc_channelizer_next_rows(const pddc_channelizer *c, size_t nsamples)
{
    return c ? pddc_channelizer_rows(c->nchan, c->hop, c->proto_len, c->in.samples, nsamples) : 0;
}

int pddc_channelizer_create(pddc_channelizer **out, int device, int nchan, int hop, const float *proto, int proto_len,
                            int first, int count, uint32_t flags)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (!chan_sizes_ok(nchan, hop, proto_len))
        return pddc_set_error_(PDDC_EINVAL,
                               "channelizer: nchan %d (1024, 2048 or 4096), hop %d (nchan or nchan/2), prototype of %d taps "
                               "(1, 2, 4 or 8 times nchan, at most %d)",
                               nchan, hop, proto_len, kChanMaxProto);
    if (!proto)
        return pddc_set_error_(PDDC_EINVAL, "channelizer: null prototype");
    if (!channel_range_ok(nchan, first, count))
        return pddc_set_error_(PDDC_EINVAL, "channelizer: first %d (0 .. nchan-1), count %d (1 .. nchan)", first, count);
    if (flags)
        return pddc_set_error_(PDDC_EINVAL, "channelizer: unknown flags 0x%x", flags);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_channelizer *c = new (std::nothrow) pddc_channelizer;
    if (!c)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    c->device = device;
    c->nchan = nchan;
    c->hop = hop;
    c->proto_len = proto_len;
    c->first = first;
    c->count = count;
    const int rc = chan_create(c, proto);
    if (rc) {
        chan_free(c);
        return rc;
    }
    *out = c;
    return PDDC_OK;
}

int pddc_channelizer_destroy(pddc_channelizer *c)
{
    if (!c)
        return PDDC_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    chan_free(c);
    return PDDC_OK;
}

int pddc_channelizer_reset(pddc_channelizer *c)
{
    if (!c)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(c->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    c->in.reset();
    c->rows = 0;
    return PDDC_OK;
}

int pddc_channelizer_set_range(pddc_channelizer *c, int first, int count)
{
    if (!c)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (!channel_range_ok(c->nchan, first, count))
        return pddc_set_error_(PDDC_EINVAL, "channelizer: first %d (0 .. nchan-1), count %d (1 .. nchan)", first, count);
    c->first = first;
    c->count = count;
    c->channels.clear();        /* range mode; the device table is of no use to a later list: set_channels marks it stale */
    return PDDC_OK;
}

int pddc_channelizer_set_channels(pddc_channelizer *c, const int *channels, int n)
{
    if (!c)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (!channel_list_ok(c->nchan, channels, n))
        return pddc_set_error_(PDDC_EINVAL, "channelizer: a list of %d channels (1 .. %d, each 0 .. nchan-1, no duplicates)",
                               n, kChannelListMax);
    c->channels.assign(channels, channels + n);
    c->count = n;
    c->slot_dirty = true;
    return PDDC_OK;
}

int pddc_channelizer_process(pddc_channelizer *c, const void *d_packed, size_t nsamples, void *d_out,
                             size_t out_capacity_rows, size_t *n_rows, void *stream)
{
    if (!c)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (const int rc = PackedCarry::check(d_packed, nsamples))
        return rc;
    const PackedCarry::Plan plan = c->in.plan(nsamples, c->proto_len, c->hop);
    const uint64_t nrows = plan.n_complete;
    if (nrows && (!d_out || ((uintptr_t)d_out & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_out must be an 8-byte aligned device pointer");
    if (nrows > out_capacity_rows)
        return pddc_set_error_(PDDC_ECAPACITY, "channelizer: %llu rows, room for %zu", (unsigned long long)nrows,
                               out_capacity_rows);
    if (n_rows)
        *n_rows = 0;
    if (!nsamples)
        return PDDC_OK;
    PDDC_HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const bool list = !c->channels.empty();
    if (nrows) {
        const int taps = c->proto_len / c->nchan, units = taps * (c->nchan / c->hop);
        const int target = list ? c->target_blocks_list : c->target_blocks;
        if (list && c->slot_dirty) {
            c->h_slot.assign((size_t)c->nchan, (short)-1);
            for (size_t i = 0; i < c->channels.size(); ++i)
                c->h_slot[(size_t)c->channels[i]] = (short)i;
            PDDC_HIP_TRY(hipMemcpyAsync(c->d_slot, c->h_slot.data(), c->h_slot.size() * sizeof(short), hipMemcpyHostToDevice, st));
        }
        /* rows per block: the stream spread over the blocks that fit side by side, but never runs so short that the
         * porch (units - 1 re-read units per run) outweighs them -- at least 4 rows per re-read unit (porch <= 25 %) */
        long long run = tunables().chan_run.load();
        if (run <= 0) {
            run = (long long)((nrows + (uint64_t)target - 1) / (uint64_t)target);
            const long long floor_rows = 4LL * (units - 1);
            run = run < floor_rows ? floor_rows : run;
        }
        ChannelizeArgs a{};
        a.in = c->in.stream(d_packed);
        a.nrows = (long long)nrows;
        a.run = run < 1 ? 1 : run;
        a.row_parity = (unsigned)(c->rows & 1);
        a.first = c->first;
        a.count = c->count;
        a.proto = c->d_proto;
        a.twiddles = c->d_tw;
        a.out = static_cast<float *>(d_out);
        a.slot = list ? c->d_slot : nullptr;
        PDDC_HIP_TRY(launch_channelize(c->nchan, taps, c->hop, a, st));
    }
    PDDC_HIP_TRY(launch_channelize_tail(c->in.carry(plan, d_packed), st));
    /* both launches were accepted: only now do the host-side counters move */
    c->in.commit(plan, nsamples);
    if (nrows && list)
        c->slot_dirty = false;
    c->rows += nrows;
    if (n_rows)
        *n_rows = (size_t)nrows;
    return PDDC_OK;
}

} // extern "C"
