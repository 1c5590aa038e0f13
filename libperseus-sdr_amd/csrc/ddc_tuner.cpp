/*
 * ddc_tuner.cpp -- host side of the tuner (include/perseus_ddc.h, pddc_tuner_*): the object, its receiver table, the
 * carried z values and counters, and the launches of a batch.  The kernels are in ddc_tuner.hip.
 * List mode (pddc_tuner_set_channels) is host logic only: a receiver's column is the index of its channel in the list and
 * `count` the list's length; k_tune takes any count and any column.  The table is rebuilt and uploaded by the next
 * process(), as after any other change.
 */
#include "ddc_host.h"
#include "ddc_tuner.h"

#include <algorithm>
#include <new>
#include <vector>

using namespace pddc;

struct pddc_tuner {
    int device = 0;
    int nchan = 0, hop = 0, first = 0, count = 0;
    int nrx = 0, ntaps = 0, decim = 0;
    std::vector<short> slot;                        /* list mode: [nchan], column of channel k, -1: not listed; empty: range mode */
    int carry_cap = 1;                              /* max(ntaps - 1, 1) z values per receiver                    */
    int target_blocks = 0;
    std::vector<uint32_t> freg, phi;
    std::vector<TuneRx> table;                      /* sorted by column; rebuilt and uploaded when `dirty`        */
    bool dirty = true;
    TuneRx *d_table = nullptr;
    float *d_taps = nullptr;
    float2 *d_carry[2] = { nullptr, nullptr };      /* process() reads [cur] and writes [cur ^ 1]                 */
    int cur = 0;
    uint64_t rows = 0;                              /* rows taken since create / reset                            */
};

static_assert(kChannelListMax == kTuneMaxRx, "a channel list holds as many channels as a tuner has receivers");

static int tune_log2(int nchan) { return nchan == 1024 ? 10 : nchan == 2048 ? 11 : nchan == 4096 ? 12 : 0; }

static void tune_split(int b, uint32_t freg, int *channel, int32_t *residue)
{
    const uint32_t k = (uint32_t)(freg + (1u << (31 - b))) >> (32 - b);
    if (channel)
        *channel = (int)k;
    if (residue)
        *residue = (int32_t)(freg - (k << (32 - b)));
}

static bool tune_in_range(int nchan, int first, int count, uint32_t freg)
{
    int k;
    tune_split(tune_log2(nchan), freg, &k, nullptr);
    return ((k - first) & (nchan - 1)) < count;
}

/* the column table of a list */
static std::vector<short> tune_slots(int nchan, const int *channels, int n)
{
    std::vector<short> slot((size_t)nchan, (short)-1);
    for (int i = 0; i < n; ++i)
        slot[(size_t)channels[i]] = (short)i;
    return slot;
}

static bool tune_listed(int nchan, const std::vector<short> &slot, uint32_t freg)
{
    int k;
    tune_split(tune_log2(nchan), freg, &k, nullptr);
    return slot[(size_t)k] >= 0;
}

static void tune_build_table(pddc_tuner *t)
{
    const int b = tune_log2(t->nchan);
    t->table.resize((size_t)t->nrx);
    for (int j = 0; j < t->nrx; ++j) {
        int k;
        int32_t r;
        tune_split(b, t->freg[(size_t)j], &k, &r);
        const int col = t->slot.empty() ? (k - t->first) & (t->nchan - 1) : (int)t->slot[(size_t)k];
        t->table[(size_t)j] = TuneRx{ col, r, t->phi[(size_t)j], j };
    }
    std::stable_sort(t->table.begin(), t->table.end(), [](const TuneRx &x, const TuneRx &y) { return x.col < y.col; });
}

/* what a batch of nrows launches: process() launches it, pddc_tuner_schedule reports it */
struct TunePlan {
    uint64_t m0, nout;                              /* outputs before this batch, outputs of this batch           */
    int group, tile;                                /* receivers per block, outputs per tile                      */
    long long run, blocks;                          /* outputs per block (a multiple of tile), blocks along them  */
    uint64_t carried;                               /* rows the next batch's first output still needs             */
};

static TunePlan tune_plan(const pddc_tuner *t, size_t nrows)
{
    TunePlan p{};
    const uint64_t R = (uint64_t)t->decim, total = t->rows + nrows;
    p.m0 = windows_complete(t->ntaps, t->decim, t->rows);
    const uint64_t m1 = windows_complete(t->ntaps, t->decim, total);
    p.nout = m1 - p.m0;
    p.group = tune_group(t->ntaps);
    p.tile = tune_tile_outputs(t->ntaps, t->decim);
    if (p.nout) {
        /* outputs per block: the batch spread over the blocks that keep the device busy, but never runs so short that
         * the porch (ntaps - 1 rows read again per run) outweighs them -- at least 4 (ntaps - 1) rows per run */
        const long long groups = (t->nrx + p.group - 1) / p.group;
        const long long runs = std::max(1LL, (long long)t->target_blocks / groups);
        long long run = ((long long)p.nout + runs - 1) / runs;
        run = std::max(run, (4LL * (t->ntaps - 1) + t->decim - 1) / t->decim);
        p.run = (std::max(run, 1LL) + p.tile - 1) / p.tile * p.tile;
        p.blocks = ((long long)p.nout + p.run - 1) / p.run;
    }
    p.carried = total > m1 * R ? total - m1 * R : 0;     /* m1 R: the first row the next output needs */
    return p;
}

static void tune_free(pddc_tuner *t)
{
    hipFree(t->d_table);
    hipFree(t->d_taps);
    hipFree(t->d_carry[0]);
    hipFree(t->d_carry[1]);
    delete t;
}

static int tune_alloc(pddc_tuner *t, const float *taps)
{
    PDDC_HIP_TRY(hipSetDevice(t->device));
    int ncu = 0;
    PDDC_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, t->device));
    t->target_blocks = 4 * (ncu > 0 ? ncu : 256);
    const size_t carry = sizeof(float2) * (size_t)t->nrx * (size_t)t->carry_cap;
    PDDC_HIP_TRY(hipMalloc(&t->d_table, sizeof(TuneRx) * (size_t)t->nrx));
    PDDC_HIP_TRY(hipMalloc(&t->d_taps, sizeof(float) * (size_t)t->ntaps));
    PDDC_HIP_TRY(hipMalloc(&t->d_carry[0], carry));
    PDDC_HIP_TRY(hipMalloc(&t->d_carry[1], carry));
    PDDC_HIP_TRY(hipMemcpy(t->d_taps, taps, sizeof(float) * (size_t)t->ntaps, hipMemcpyHostToDevice));
    return PDDC_OK;
}

extern "C" {

int pddc_tuner_channel(int nchan, uint32_t freg, int *channel, int32_t *residue)
{
    const int b = tune_log2(nchan);
    if (!b)
        return pddc_set_error_(PDDC_EINVAL, "tuner: nchan %d (1024, 2048 or 4096)", nchan);
    tune_split(b, freg, channel, residue);
    return PDDC_OK;
}

uint64_t pddc_tuner_outputs(int ntaps, int decim, uint64_t rows_before, size_t nrows)
{
    if (ntaps < 1 || ntaps > kTuneMaxTaps || decim < 1 || decim > kTuneMaxDecim)
        return 0;
    return windows_complete(ntaps, decim, rows_before + nrows) - windows_complete(ntaps, decim, rows_before);
}

uint64_t pddc_tuner_next_outputs(const pddc_tuner *t, size_t nrows)
{
    return t ? pddc_tuner_outputs(t->ntaps, t->decim, t->rows, nrows) : 0;
}

int pddc_tuner_create(pddc_tuner **out, int device, int nchan, int hop, int first, int count, const uint32_t *freg,
                      int nrx, const float *taps, int ntaps, int decim, uint32_t flags)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (!tune_log2(nchan) || (hop != nchan && hop != nchan / 2))
        return pddc_set_error_(PDDC_EINVAL, "tuner: nchan %d (1024, 2048 or 4096), hop %d (nchan or nchan/2)", nchan, hop);
    if (!channel_range_ok(nchan, first, count))
        return pddc_set_error_(PDDC_EINVAL, "tuner: first %d (0 .. nchan-1), count %d (1 .. nchan)", first, count);
    if (nrx < 1 || nrx > kTuneMaxRx || !freg)
        return pddc_set_error_(PDDC_EINVAL, "tuner: %d receivers (1 .. %d) and their words", nrx, kTuneMaxRx);
    if (ntaps < 1 || ntaps > kTuneMaxTaps || decim < 1 || decim > kTuneMaxDecim || !taps)
        return pddc_set_error_(PDDC_EINVAL, "tuner: %d taps (1 .. %d), decimation %d (1 .. %d) and the taps", ntaps,
                               kTuneMaxTaps, decim, kTuneMaxDecim);
    if (flags)
        return pddc_set_error_(PDDC_EINVAL, "tuner: unknown flags 0x%x", flags);
    for (int j = 0; j < nrx; ++j)
        if (!tune_in_range(nchan, first, count, freg[j]))
            return pddc_set_error_(PDDC_EINVAL, "tuner: receiver %d (word 0x%08x) lies outside the channel range", j, freg[j]);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_tuner *t = new (std::nothrow) pddc_tuner;
    if (!t)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    t->device = device;
    t->nchan = nchan;
    t->hop = hop;
    t->first = first;
    t->count = count;
    t->nrx = nrx;
    t->ntaps = ntaps;
    t->decim = decim;
    t->carry_cap = ntaps > 1 ? ntaps - 1 : 1;
    t->freg.assign(freg, freg + nrx);
    t->phi.assign((size_t)nrx, 0u);
    const int rc = tune_alloc(t, taps);
    if (rc) {
        tune_free(t);
        return rc;
    }
    *out = t;
    return PDDC_OK;
}

int pddc_tuner_destroy(pddc_tuner *t)
{
    if (!t)
        return PDDC_OK;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    tune_free(t);
    return PDDC_OK;
}

int pddc_tuner_reset(pddc_tuner *t)
{
    if (!t)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(t->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    t->rows = 0;
    std::fill(t->phi.begin(), t->phi.end(), 0u);
    t->dirty = true;
    return PDDC_OK;
}

int pddc_tuner_set_freq(pddc_tuner *t, int rx, uint32_t freg)
{
    if (!t)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (rx < 0 || rx >= t->nrx)
        return pddc_set_error_(PDDC_EINVAL, "tuner: receiver %d (0 .. %d)", rx, t->nrx - 1);
    if (!t->slot.empty() && !tune_listed(t->nchan, t->slot, freg))
        return pddc_set_error_(PDDC_EINVAL, "tuner: the channel of word 0x%08x is not in the channel list", freg);
    if (t->slot.empty() && !tune_in_range(t->nchan, t->first, t->count, freg))
        return pddc_set_error_(PDDC_EINVAL, "tuner: word 0x%08x lies outside the channel range", freg);
    /* the accumulator is continuous: the increment changes at the next row, s0 = rows so far, the phase does not */
    const uint32_t sd = (uint32_t)(t->rows * (uint64_t)t->hop);
    t->phi[(size_t)rx] += (t->freg[(size_t)rx] - freg) * sd;
    t->freg[(size_t)rx] = freg;
    t->dirty = true;
    return PDDC_OK;
}

int pddc_tuner_set_range(pddc_tuner *t, int first, int count)
{
    if (!t)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (!channel_range_ok(t->nchan, first, count))
        return pddc_set_error_(PDDC_EINVAL, "tuner: first %d (0 .. nchan-1), count %d (1 .. nchan)", first, count);
    for (int j = 0; j < t->nrx; ++j)
        if (!tune_in_range(t->nchan, first, count, t->freg[(size_t)j]))
            return pddc_set_error_(PDDC_EINVAL, "tuner: receiver %d (word 0x%08x) lies outside that channel range", j,
                                   t->freg[(size_t)j]);
    t->first = first;
    t->count = count;
    t->slot.clear();
    t->dirty = true;
    return PDDC_OK;
}

int pddc_tuner_set_channels(pddc_tuner *t, const int *channels, int n)
{
    if (!t)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (!channel_list_ok(t->nchan, channels, n))
        return pddc_set_error_(PDDC_EINVAL, "tuner: a list of %d channels (1 .. %d, each 0 .. nchan-1, no duplicates)", n,
                               kChannelListMax);
    std::vector<short> slot = tune_slots(t->nchan, channels, n);
    for (int j = 0; j < t->nrx; ++j)
        if (!tune_listed(t->nchan, slot, t->freg[(size_t)j]))
            return pddc_set_error_(PDDC_EINVAL, "tuner: the channel of receiver %d (word 0x%08x) is not in that list", j,
                                   t->freg[(size_t)j]);
    t->slot.swap(slot);
    t->first = 0;
    t->count = n;
    t->dirty = true;
    return PDDC_OK;
}

int pddc_tuner_channel_list(int nchan, const uint32_t *freg, int nrx, int *channels)
{
    const int b = tune_log2(nchan);
    if (!b)
        return pddc_set_error_(PDDC_EINVAL, "tuner: nchan %d (1024, 2048 or 4096)", nchan);
    if (!freg || !channels || nrx < 1)
        return pddc_set_error_(PDDC_EINVAL, "tuner: %d words and room for as many channels", nrx);
    std::vector<bool> seen((size_t)nchan, false);
    for (int j = 0; j < nrx; ++j) {
        int k;
        tune_split(b, freg[j], &k, nullptr);
        seen[(size_t)k] = true;
    }
    int n = 0;
    for (int k = 0; k < nchan; ++k)
        if (seen[(size_t)k])
            channels[n++] = k;
    return n;
}

int pddc_tuner_schedule(const pddc_tuner *t, size_t nrows, int out[5])
{
    if (!t || !out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    const TunePlan p = tune_plan(t, nrows);
    out[0] = p.group;
    out[1] = p.tile;
    out[2] = (int)p.run;
    out[3] = (int)p.blocks;
    out[4] = (int)p.carried;
    return PDDC_OK;
}

int pddc_tuner_process(pddc_tuner *t, const void *d_rows, size_t nrows, void *d_out, size_t out_stride, size_t *n_out,
                       void *stream)
{
    if (!t)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (nrows && (!d_rows || ((uintptr_t)d_rows & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_rows must be an 8-byte aligned device pointer");
    const uint64_t R = (uint64_t)t->decim;
    const TunePlan plan = tune_plan(t, nrows);
    const uint64_t m0 = plan.m0, nout = plan.nout;
    if (nout && (!d_out || ((uintptr_t)d_out & 7)))
        return pddc_set_error_(PDDC_EINVAL, "d_out must be an 8-byte aligned device pointer");
    if (nout > out_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "tuner: %llu outputs per receiver, out_stride %zu", (unsigned long long)nout,
                               out_stride);
    if (n_out)
        *n_out = 0;
    if (!nrows)
        return PDDC_OK;
    PDDC_HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    if (t->dirty) {
        tune_build_table(t);
        PDDC_HIP_TRY(hipMemcpyAsync(t->d_table, t->table.data(), sizeof(TuneRx) * (size_t)t->nrx, hipMemcpyHostToDevice, st));
    }
    const uint64_t total = t->rows + nrows;
    TuneArgs a{};
    a.rows = static_cast<const float2 *>(d_rows);
    a.nrows = (long long)nrows;
    a.count = t->count;
    a.rx = t->d_table;
    a.nrx = t->nrx;
    a.carry = t->d_carry[t->cur];
    a.carry_cap = t->carry_cap;
    a.off = (long long)t->rows - (long long)(m0 * R);
    a.phase0 = (uint32_t)(m0 * R * (uint64_t)t->hop);
    a.hop = (uint32_t)t->hop;
    a.taps = t->d_taps;
    a.ntaps = t->ntaps;
    a.decim = t->decim;
    a.nout = (long long)nout;
    a.out = static_cast<float2 *>(d_out);
    a.out_stride = (long long)out_stride;
    if (nout) {
        a.co = plan.tile;
        a.run = plan.run;
        PDDC_HIP_TRY(launch_tune(a, st));
    }
    const bool carries = plan.carried > 0;
    if (carries) {
        TuneCarryArgs c{};
        c.t = a;
        c.new_carry = t->d_carry[t->cur ^ 1];
        c.keep_u = (long long)(nout * R);
        c.new_len = (int)plan.carried;
        PDDC_HIP_TRY(launch_tune_carry(c, st));
    }
    /* every launch was accepted: only now do the host-side counters move */
    if (carries)
        t->cur ^= 1;
    t->dirty = false;
    t->rows = total;
    if (n_out)
        *n_out = (size_t)nout;
    return PDDC_OK;
}

} // extern "C"
