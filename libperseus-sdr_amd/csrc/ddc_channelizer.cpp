/*
 * ddc_channelizer.cpp -- host side of the channelizer (include/perseus_ddc.h, pddc_channelizer_*): the object, its
 * carried tail and counters, and the two launches of a batch.  The kernels are in ddc_channelizer.hip.
 */
#include "../../include/perseus_ddc.h"
#include "ddc_channelizer.h"
#include "ddc_kernels.h"
#include "ddc_spectrum.h"

#include <new>
#include <vector>

using namespace pddc;

extern "C" int pddc_set_error_(int code, const char *fmt, ...);

#define CHAN_TRY(expr)                                                                                          \
    do {                                                                                                        \
        hipError_t e__ = (expr);                                                                                \
        if (e__ != hipSuccess)                                                                                  \
            return pddc_set_error_(e__ == hipErrorOutOfMemory ? PDDC_ENOMEM                                     \
                                   : (e__ == hipErrorNoDevice || e__ == hipErrorInvalidDevice) ? PDDC_ENODEV    \
                                                                                               : PDDC_EHIP,     \
                                   "%s: %s", #expr, hipGetErrorString(e__));                                    \
    } while (0)

struct pddc_channelizer {
    int device = 0;
    int nchan = 0, hop = 0, proto_len = 0;
    int first = 0, count = 0;
    int target_blocks = 0;
    float *d_proto = nullptr, *d_tw = nullptr;
    uint8_t *d_tail[2] = { nullptr, nullptr };      /* proto_len * 6 bytes each; process() reads [cur] and writes [cur ^ 1] */
    int cur = 0;
    uint64_t tail_len = 0;                          /* samples in d_tail[cur], < proto_len     */
    uint64_t samples = 0;                           /* stream length since create / reset      */
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

static bool chan_range_ok(int nchan, int first, int count)
{
    return first >= 0 && first < nchan && count >= 1 && count <= nchan;
}

static uint64_t chan_complete(int hop, int proto_len, uint64_t len)
{
    return len >= (uint64_t)proto_len ? (len - (uint64_t)proto_len) / (uint64_t)hop + 1 : 0;
}

static void chan_free(pddc_channelizer *c)
{
    hipFree(c->d_proto);
    hipFree(c->d_tw);
    hipFree(c->d_tail[0]);
    hipFree(c->d_tail[1]);
    delete c;
}

static int chan_create(pddc_channelizer *c, const float *proto)
{
    CHAN_TRY(hipSetDevice(c->device));
    int ncu = 0;
    CHAN_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
    c->target_blocks = channelize_target_blocks(c->nchan, c->proto_len / c->nchan, c->hop, ncu > 0 ? ncu : 256);
    std::vector<float> tw((size_t)spectrum_twiddle_len(c->nchan));
    spectrum_build_twiddles(c->nchan, tw.data());
    CHAN_TRY(hipMalloc(&c->d_proto, (size_t)c->proto_len * sizeof(float)));
    CHAN_TRY(hipMalloc(&c->d_tw, tw.size() * sizeof(float)));
    CHAN_TRY(hipMalloc(&c->d_tail[0], (size_t)c->proto_len * 6));
    CHAN_TRY(hipMalloc(&c->d_tail[1], (size_t)c->proto_len * 6));
    CHAN_TRY(hipMemcpy(c->d_proto, proto, (size_t)c->proto_len * sizeof(float), hipMemcpyHostToDevice));
    CHAN_TRY(hipMemcpy(c->d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
    return PDDC_OK;
}

extern "C" {

uint64_t pddc_channelizer_rows(int nchan, int hop, int proto_len, uint64_t samples_before, size_t nsamples)
{
    if (!chan_sizes_ok(nchan, hop, proto_len))
        return 0;
    return chan_complete(hop, proto_len, samples_before + nsamples) - chan_complete(hop, proto_len, samples_before);
}

uint64_t pddc_channelizer_next_rows(const pddc_channelizer *c, size_t nsamples)
{
    return c ? pddc_channelizer_rows(c->nchan, c->hop, c->proto_len, c->samples, nsamples) : 0;
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
    if (!chan_range_ok(nchan, first, count))
        return pddc_set_error_(PDDC_EINVAL, "channelizer: first %d (0 .. nchan-1), count %d (1 .. nchan)", first, count);
    if (flags)
        return pddc_set_error_(PDDC_EINVAL, "channelizer: unknown flags 0x%x", flags);
    const int ndev = pddc_device_count();
    if (ndev < 0)
        return ndev;
    if (ndev == 0)
        return pddc_set_error_(PDDC_ENODEV, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev)
        return pddc_set_error_(PDDC_ENODEV, "device %d out of range (%d visible)", device, ndev);
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
    CHAN_TRY(hipSetDevice(c->device));
    CHAN_TRY(hipDeviceSynchronize());
    c->tail_len = 0;
    c->samples = 0;
    c->rows = 0;
    return PDDC_OK;
}

int pddc_channelizer_set_range(pddc_channelizer *c, int first, int count)
{
    if (!c)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (!chan_range_ok(c->nchan, first, count))
        return pddc_set_error_(PDDC_EINVAL, "channelizer: first %d (0 .. nchan-1), count %d (1 .. nchan)", first, count);
    c->first = first;
    c->count = count;
    return PDDC_OK;
}

int pddc_channelizer_process(pddc_channelizer *c, const void *d_packed, size_t nsamples, void *d_out,
                             size_t out_capacity_rows, size_t *n_rows, void *stream)
{
    if (!c)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (nsamples % 8)
        return pddc_set_error_(PDDC_EINVAL, "nsamples (%zu) must be a multiple of 8", nsamples);
    if (nsamples && (!d_packed || ((uintptr_t)d_packed & 15)))
        return pddc_set_error_(PDDC_EINVAL, "d_packed must be a 16-byte aligned device pointer");
    const uint64_t len = c->tail_len + nsamples;           /* tail-then-batch */
    const uint64_t nrows = chan_complete(c->hop, c->proto_len, len);
    if (nrows && (!d_out || ((uintptr_t)d_out & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_out must be an 8-byte aligned device pointer");
    if (nrows > out_capacity_rows)
        return pddc_set_error_(PDDC_ECAPACITY, "channelizer: %llu rows, room for %zu", (unsigned long long)nrows,
                               out_capacity_rows);
    if (n_rows)
        *n_rows = 0;
    if (!nsamples)
        return PDDC_OK;
    CHAN_TRY(hipSetDevice(c->device));
    const uint64_t keep_from = nrows * (uint64_t)c->hop;
    hipStream_t st = (hipStream_t)stream;
    if (nrows) {
        const int taps = c->proto_len / c->nchan, units = taps * (c->nchan / c->hop);
        /* rows per block: the stream spread over the blocks that fit side by side, but never runs so short that the
         * porch (units - 1 re-read units per run) outweighs them -- at least 4 rows per re-read unit (porch <= 25 %) */
        long long run = tunables().chan_run.load();
        if (run <= 0) {
            run = (long long)((nrows + (uint64_t)c->target_blocks - 1) / (uint64_t)c->target_blocks);
            const long long floor_rows = 4LL * (units - 1);
            run = run < floor_rows ? floor_rows : run;
        }
        ChannelizeArgs a{};
        a.tail = c->d_tail[c->cur];
        a.batch = static_cast<const uint8_t *>(d_packed);
        a.tail_len = (long long)c->tail_len;
        a.nrows = (long long)nrows;
        a.run = run < 1 ? 1 : run;
        a.row_parity = (unsigned)(c->rows & 1);
        a.first = c->first;
        a.count = c->count;
        a.proto = c->d_proto;
        a.twiddles = c->d_tw;
        a.out = static_cast<float *>(d_out);
        CHAN_TRY(launch_channelize(c->nchan, taps, c->hop, a, st));
    }
    ChannelizeTailArgs t{};
    t.tail = c->d_tail[c->cur];
    t.batch = static_cast<const uint8_t *>(d_packed);
    t.new_tail = c->d_tail[c->cur ^ 1];
    t.tail_len = (long long)c->tail_len;
    t.keep_from = (long long)keep_from;
    t.new_len = (long long)(len - keep_from);
    CHAN_TRY(launch_channelize_tail(t, st));
    /* both launches were accepted: only now do the host-side counters move */
    c->cur ^= 1;
    c->tail_len = len - keep_from;
    c->samples += nsamples;
    c->rows += nrows;
    if (n_rows)
        *n_rows = (size_t)nrows;
    return PDDC_OK;
}

} // extern "C"
