/*
 * ddc_fsk.cpp -- host side of the FSK decoder (include/perseus_ddc.h, pddc_fsk_*): the object, its modem bank and
 * receiver table, the capacity bound, the launch of a batch and the status read.  The kernel is in ddc_fsk.hip.
 * What is carried per receiver (its last W - 1 inputs, the start-stop receiver's registers and the counters) lives on
 * the device in two pairs of records, read and written in turn; nothing on the device is cleared from the host: the
 * marks (fresh: create, reset; clear: RESTART, OFF -> ON; idle: another modem) live in the table, which is uploaded in
 * stream order when it changed, and go once a launch that read them was accepted.  The bank is uploaded once, at create.
 */
#include "ddc_stage.h"
#include "ddc_fsk.h"

#include <cmath>

using namespace pddc;

struct pddc_fsk : StageBase {
    PDDC_LOCAL ~pddc_fsk() = default;
    int nmodems = 0, window = 0;
    std::vector<FskModem> bank;                     /* the host's copy: set_rx, max_chars                          */
    RxTable<FskRx> table;
    DevBuf<float> taps;                             /* [nmodems][fsk_row(W)][4]                                    */
    DevBuf<FskModem> modems;
    std::vector<FskState> host_state;               /* where read() lands the records                              */
    bool launched = false;                          /* a batch since create / reset: the records were written      */
    Carried<FskState> state;
    Carried<float2> hist;                           /* [nrx][W - 1]                                                */
    uint64_t m = 0;                                 /* samples per receiver since create / reset                   */
};

static_assert(PDDC_FSK_ON == kFskOn && PDDC_FSK_REVERSE == kFskReverse && !(PDDC_FSK_RESTART & (kFskOn | kFskReverse | kFskMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_FSK_FRAMING == 1, "the kernel stores the stop element's `space` as the character's flags");
static_assert(PDDC_FSK_IDLE == kFskStIdle && PDDC_FSK_START == kFskStStart && PDDC_FSK_DATA == kFskStData &&
                  PDDC_FSK_STOP == kFskStStop,
              "the kernel's state numbers are the header's");
static_assert(sizeof(pddc_fsk_char) == 16 && sizeof(FskChar) == 16 && offsetof(pddc_fsk_char, code) == offsetof(FskChar, code) &&
                  offsetof(pddc_fsk_char, flags) == offsetof(FskChar, flags) &&
                  offsetof(pddc_fsk_char, quality) == offsetof(FskChar, quality),
              "the kernel's character record is the header's");

static constexpr uint32_t kFskUserFlags = PDDC_FSK_ON | PDDC_FSK_REVERSE | PDDC_FSK_RESTART;

/* samples from the edge to the STOP strobe: the (nbits + 2)-th carry of an accumulator that starts at 2^31 and moves
 * by inc, ceil((nbits + 1.5) 2^32 / inc) */
static uint64_t fsk_period(const FskModem &mo)
{
    const uint64_t num = (uint64_t)(2u * mo.nbits + 3u) << 31;
    return (num + mo.inc - 1u) / mo.inc;
}

static uint64_t fsk_bound(const pddc_fsk *f, uint64_t n)
{
    uint64_t most = 0;
    for (const FskModem &mo : f->bank) {
        const uint64_t c = n / fsk_period(mo) + 1u;
        most = c > most ? c : most;
    }
    return most;
}

extern "C" {

int pddc_fsk_tile_outputs(void) { return kFskTile; }

int pddc_fsk_create(pddc_fsk **out, int device, int nrx, int window, int nmodems, const float *taps, const uint32_t *inc,
                    const int *nbits, const pddc_fsk_rx *rx)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kFskMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "fsk: %d receivers (1 .. %d) and their modems", nrx, kFskMaxRx);
    if (window < 1 || window > kFskMaxWindow || nmodems < 1 || nmodems > kFskMaxModems)
        return pddc_set_error_(PDDC_EINVAL, "fsk: %d modems (1 .. %d) with a window of %d (1 .. %d)", nmodems, kFskMaxModems,
                               window, kFskMaxWindow);
    if (!taps || !inc || !nbits)
        return pddc_set_error_(PDDC_EINVAL, "fsk: null taps, inc or nbits");
    for (int i = 0; i < nmodems * 4 * window; ++i)
        if (!std::isfinite(taps[i]))
            return pddc_set_error_(PDDC_EINVAL, "fsk: modem %d: a tap is not finite", i / (4 * window));
    for (int b = 0; b < nmodems; ++b)
        if (inc[b] < 1u || inc[b] > (1u << 30) || nbits[b] < 5 || nbits[b] > 8)
            return pddc_set_error_(PDDC_EINVAL, "fsk: modem %d: inc %u (1 .. 2^30), nbits %d (5 .. 8)", b, inc[b], nbits[b]);
    for (int j = 0; j < nrx; ++j)
        if (rx[j].modem < 0 || rx[j].modem >= nmodems || (rx[j].flags & ~kFskUserFlags))
            return pddc_set_error_(PDDC_EINVAL, "fsk: receiver %d: modem %d (0 .. %d), flags 0x%x", j, rx[j].modem, nmodems - 1,
                                   rx[j].flags);
    return stage_create(out, device, nrx, [&](pddc_fsk &f) {
        f.nmodems = nmodems;
        f.window = window;
        f.host_state.resize((size_t)nrx);
        for (int b = 0; b < nmodems; ++b)
            f.bank.push_back(FskModem{ inc[b], (uint32_t)nbits[b] });
        for (int j = 0; j < nrx; ++j)
            f.table.host.push_back(FskRx{ rx[j].modem, (rx[j].flags & (kFskOn | kFskReverse)) | kFskFresh });
        /* taps[b][0][t] = hm, taps[b][1][t] = hs (re, im) -> per tap (hm.re, hm.im, hs.re, hs.im) */
        const size_t row = (size_t)fsk_row(window), Wz = (size_t)window;
        std::vector<float> rows((size_t)nmodems * row * 4, 0.0f);
        for (size_t b = 0; b < (size_t)nmodems; ++b)
            for (size_t t = 0; t < Wz; ++t)
                for (size_t c = 0; c < 4; ++c)
                    rows[(b * row + t) * 4 + c] = taps[((b * 2 + c / 2) * Wz + t) * 2 + c % 2];
        PDDC_TRY(f.taps.alloc_copy(rows));
        PDDC_TRY(f.modems.alloc_copy(f.bank));
        PDDC_TRY(f.table.alloc());
        PDDC_TRY(f.state.alloc((size_t)nrx));
        return f.hist.alloc((size_t)nrx * (size_t)(window > 1 ? window - 1 : 1));
    });
}

int pddc_fsk_destroy(pddc_fsk *f) { return stage_destroy(f); }

int pddc_fsk_reset(pddc_fsk *f)
{
    PDDC_TRY(stage_quiesce(f));
    f->m = 0;
    f->launched = false;
    for (FskRx &r : f->table.host)
        r.flags = (r.flags & ~kFskMarks) | kFskFresh;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_fsk_set_rx(pddc_fsk *f, int rx, int modem, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(f, "fsk", rx));
    if (modem < 0 || modem >= f->nmodems || (flags & ~kFskUserFlags))
        return pddc_set_error_(PDDC_EINVAL, "fsk: modem %d (0 .. %d), flags 0x%x", modem, f->nmodems - 1, flags);
    FskRx &r = f->table.host[(size_t)rx];
    uint32_t marks = r.flags & kFskMarks;
    /* RESTART, OFF -> ON: the carried inputs and the start-stop receiver start afresh, the counters stay; another
     * modem: the inputs stay, a character in progress is dropped */
    if ((flags & PDDC_FSK_RESTART) || (!(r.flags & kFskOn) && (flags & kFskOn)))
        marks |= kFskClear;
    if (modem != r.modem)
        marks |= kFskIdle;
    r.modem = modem;
    r.flags = (flags & (kFskOn | kFskReverse)) | marks;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_fsk_max_chars(const pddc_fsk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)fsk_bound(f, n);
    return PDDC_OK;
}

int pddc_fsk_process(pddc_fsk *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                     void *d_counts, void *d_d, size_t d_stride, void *stream)
{
    if (!f)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_chars, 8, "d_chars"));
        PDDC_TRY(device_ptr_ok(d_counts, 4, "d_counts"));
    } else
        PDDC_TRY(device_ptr_ok(d_counts, 4, "d_counts", true));
    PDDC_TRY(device_ptr_ok(d_d, 4, "d_d", true));
    if (over_capacity(n, z_stride) || (d_d && over_capacity(n, d_stride)))
        return pddc_set_error_(PDDC_ECAPACITY, "fsk: %zu samples per receiver, z_stride %zu, d_stride %zu", n, z_stride, d_stride);
    if (n > (size_t)1 << 40 || z_stride > (size_t)1 << 40 || d_stride > (size_t)1 << 40 || char_stride > (size_t)1 << 40)
        return pddc_set_error_(PDDC_EINVAL, "fsk: %zu samples per receiver are too many for one batch", n);
    const uint64_t bound = fsk_bound(f, n);
    if (char_stride < bound)
        return pddc_set_error_(PDDC_ECAPACITY, "fsk: room for %zu characters per receiver, %zu samples can end %llu", char_stride,
                               n, (unsigned long long)bound);
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n) {
        /* nothing is launched and nothing carried moves; the counts of an empty batch are 0 */
        if (d_counts)
            PDDC_HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)f->nrx, st));
        return PDDC_OK;
    }
    /* tiles read their neighbours' inputs: the bytes read and the bytes written must not meet */
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    if ((d_d && ranges_overlap(d_z, zbytes, d_d, rows_extent(f->nrx, n, d_stride, sizeof(float)))) ||
        ranges_overlap(d_z, zbytes, d_chars, rows_extent(f->nrx, (size_t)bound, char_stride, sizeof(FskChar))) ||
        ranges_overlap(d_z, zbytes, d_counts, sizeof(uint32_t) * (size_t)f->nrx))
        return pddc_set_error_(PDDC_EINVAL, "fsk: an output overlaps the input");
    PDDC_TRY(f->table.upload(st));
    FskArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.n = (long long)n;
    a.m0 = f->m;
    a.chars = static_cast<FskChar *>(d_chars);
    a.char_stride = (long long)char_stride;
    a.counts = static_cast<uint32_t *>(d_counts);
    a.d = static_cast<float *>(d_d);
    a.d_stride = (long long)d_stride;
    a.taps = f->taps.get();
    a.modems = f->modems.get();
    a.rx = f->table.dev();
    a.state = f->state.old();
    a.new_state = f->state.next();
    a.hist = f->hist.old();
    a.new_hist = f->hist.next();
    a.nrx = f->nrx;
    a.nmodems = f->nmodems;
    a.window = f->window;
    PDDC_HIP_TRY(launch_fsk(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    f->state.turn();
    f->hist.turn();
    f->m += n;
    f->launched = true;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    for (FskRx &r : f->table.host)
        if (r.flags & kFskMarks) {
            r.flags &= ~kFskMarks;
            f->table.dirty = true;
        }
    return PDDC_OK;
}

int pddc_fsk_read(pddc_fsk *f, pddc_fsk_status *host, void *stream)
{
    if (!f || !host)
        return null_argument();
    PDDC_TRY(set_device(f->device));
    PDDC_TRY(read_back(f->host_state.data(), f->launched ? f->state.old() : nullptr, (size_t)f->nrx, (hipStream_t)stream));
    for (int j = 0; j < f->nrx; ++j) {
        /* a mark that no batch has read yet: the receiver reads as the next batch will find it */
        const uint32_t marks = f->table.host[(size_t)j].flags & kFskMarks;
        const bool fresh = !f->launched || (marks & kFskFresh);
        const FskState r = fresh ? FskState{} : f->host_state[(size_t)j];
        host[j] = pddc_fsk_status{ r.chars, r.framing, r.false_starts, marks ? (uint32_t)PDDC_FSK_IDLE : r.state, r.d_last };
    }
    return PDDC_OK;
}

} // extern "C"
