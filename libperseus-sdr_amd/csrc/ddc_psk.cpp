/*
 * ddc_psk.cpp -- host side of the PSK decoder (include/perseus_ddc.h, pddc_psk_*): the object, its modem bank and
 * receiver table, the two capacity bounds, the launch of a batch and the status read.  The kernel is in ddc_psk.hip, the
 * clock, the framing and the bounds' arithmetic in ddc_psk_bits.h.
 * What is carried per receiver (its last W - 1 inputs and 128 filter outputs, the clock, the differential pair, the
 * framing and the counters) lives on the device in two pairs of records, read and written in turn; nothing on the device
 * is cleared from the host: the marks (fresh: create, reset; clear: RESTART, OFF -> ON, another modem) live in the table,
 * which is uploaded in stream order when it changed, and go once a launch that read them was accepted.  The bank is
 * uploaded once, at create.
 */
#include "ddc_stage.h"
#include "ddc_psk.h"

#include <cmath>

using namespace pddc;

struct pddc_psk : StageBase {
    PDDC_LOCAL ~pddc_psk() = default;
    int nmodems = 0, window = 0;
    std::vector<PskModem> bank;                     /* the host's copy: set_rx and the bounds                      */
    uint64_t distance = 0;                          /* the least samples between two strobes, over the bank        */
    RxTable<PskRx> table;
    DevBuf<float> taps;                             /* [nmodems][psk_row(W)]                                       */
    DevBuf<PskModem> modems;
    std::vector<PskState> host_state;               /* where read() lands the records                              */
    bool launched = false;                          /* a batch since create / reset: the records were written      */
    Carried<PskState> state;
    Carried<float2> hist;                           /* [nrx][psk_hist_slots(W)]                                    */
    uint64_t m = 0;                                 /* samples per receiver since create / reset                   */
};

static_assert(PDDC_PSK_ON == kPskOn && !(PDDC_PSK_RESTART & (kPskOn | kPskMarks)), "the kernel's flag bits are the header's");
static_assert(PDDC_PSK_LONG == kPskLongFlag, "the framing's character flag is the header's");
static_assert(sizeof(pddc_psk_char) == 16 && sizeof(PskChar) == 16 && offsetof(pddc_psk_char, code) == offsetof(PskChar, code) &&
                  offsetof(pddc_psk_char, nbits) == offsetof(PskChar, nbits) && offsetof(pddc_psk_char, flags) == offsetof(PskChar, flags) &&
                  offsetof(pddc_psk_char, quality) == offsetof(PskChar, quality),
              "the kernel's character record is the header's");
static_assert(sizeof(pddc_psk_modem) == sizeof(PskModem) && offsetof(pddc_psk_modem, step) == offsetof(PskModem, step),
              "the clock's modem is the header's");

static constexpr uint32_t kPskUserFlags = PDDC_PSK_ON | PDDC_PSK_RESTART;

static uint64_t psk_sym_bound(const pddc_psk *f, uint64_t n) { return psk_most(n, f->distance); }
static uint64_t psk_char_bound(const pddc_psk *f, uint64_t n) { return psk_most_chars(psk_sym_bound(f, n)); }

extern "C" {

int pddc_psk_tile_outputs(void) { return kPskTile; }

int pddc_psk_create(pddc_psk **out, int device, int nrx, int window, int nmodems, const float *taps, const pddc_psk_modem *modems,
                    const pddc_psk_rx *rx)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kPskMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "psk: %d receivers (1 .. %d) and their modems", nrx, kPskMaxRx);
    if (window < 1 || window > kPskMaxWindow || nmodems < 1 || nmodems > kPskMaxModems)
        return pddc_set_error_(PDDC_EINVAL, "psk: %d modems (1 .. %d) with a window of %d (1 .. %d)", nmodems, kPskMaxModems, window,
                               kPskMaxWindow);
    if (!taps || !modems)
        return pddc_set_error_(PDDC_EINVAL, "psk: null taps or modems");
    for (int i = 0; i < nmodems * window; ++i)
        if (!std::isfinite(taps[i]))
            return pddc_set_error_(PDDC_EINVAL, "psk: modem %d: a tap is not finite", i / window);
    for (int b = 0; b < nmodems; ++b)
        if (!psk_modem_ok(PskModem{ modems[b].inc, modems[b].q, modems[b].step }))
            return pddc_set_error_(PDDC_EINVAL, "psk: modem %d: 1 <= inc %u <= 2^29, 1 <= q %u <= 64 with 4 q inc <= 2^32, step %u <= inc", b,
                                   modems[b].inc, modems[b].q, modems[b].step);
    for (int j = 0; j < nrx; ++j)
        if (rx[j].modem < 0 || rx[j].modem >= nmodems || (rx[j].flags & ~kPskUserFlags))
            return pddc_set_error_(PDDC_EINVAL, "psk: receiver %d: modem %d (0 .. %d), flags 0x%x", j, rx[j].modem, nmodems - 1,
                                   rx[j].flags);
    return stage_create(out, device, nrx, [&](pddc_psk &f) {
        f.nmodems = nmodems;
        f.window = window;
        f.host_state.resize((size_t)nrx);
        f.distance = ~(uint64_t)0;
        for (int b = 0; b < nmodems; ++b) {
            f.bank.push_back(PskModem{ modems[b].inc, modems[b].q, modems[b].step });
            const uint64_t d = psk_distance(f.bank.back());
            f.distance = d < f.distance ? d : f.distance;
        }
        for (int j = 0; j < nrx; ++j)
            f.table.host.push_back(PskRx{ rx[j].modem, (rx[j].flags & kPskOn) | kPskFresh });
        const size_t row = (size_t)psk_row(window), Wz = (size_t)window;
        std::vector<float> rows((size_t)nmodems * row, 0.0f);
        for (size_t b = 0; b < (size_t)nmodems; ++b)
            for (size_t t = 0; t < Wz; ++t)
                rows[b * row + t] = taps[b * Wz + t];
        PDDC_TRY(f.taps.alloc_copy(rows));
        PDDC_TRY(f.modems.alloc_copy(f.bank));
        PDDC_TRY(f.table.alloc());
        PDDC_TRY(f.state.alloc((size_t)nrx));
        return f.hist.alloc((size_t)nrx * (size_t)psk_hist_slots(window));
    });
}

int pddc_psk_destroy(pddc_psk *f) { return stage_destroy(f); }

int pddc_psk_reset(pddc_psk *f)
{
    PDDC_TRY(stage_quiesce(f));
    f->m = 0;
    f->launched = false;
    for (PskRx &r : f->table.host)
        r.flags = (r.flags & ~kPskMarks) | kPskFresh;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_psk_set_rx(pddc_psk *f, int rx, int modem, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(f, "psk", rx));
    if (modem < 0 || modem >= f->nmodems || (flags & ~kPskUserFlags))
        return pddc_set_error_(PDDC_EINVAL, "psk: modem %d (0 .. %d), flags 0x%x", modem, f->nmodems - 1, flags);
    PskRx &r = f->table.host[(size_t)rx];
    uint32_t marks = r.flags & kPskMarks;
    /* RESTART, OFF -> ON, another modem: the carried inputs and outputs, the clock, the pair and the framing start afresh,
     * the counters stay */
    if ((flags & PDDC_PSK_RESTART) || (!(r.flags & kPskOn) && (flags & kPskOn)) || modem != r.modem)
        marks |= kPskClear;
    r.modem = modem;
    r.flags = (flags & kPskOn) | marks;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_psk_max_syms(const pddc_psk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)psk_sym_bound(f, n);
    return PDDC_OK;
}

int pddc_psk_max_chars(const pddc_psk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)psk_char_bound(f, n);
    return PDDC_OK;
}

int pddc_psk_process(pddc_psk *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride, void *d_counts,
                     void *d_sym, size_t sym_stride, void *d_nsym, void *stream)
{
    if (!f)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_chars, 8, "d_chars"));
        PDDC_TRY(device_ptr_ok(d_counts, 4, "d_counts"));
        PDDC_TRY(device_ptr_ok(d_sym, 8, "d_sym", true));
        PDDC_TRY(device_ptr_ok(d_nsym, 4, "d_nsym", !d_sym));
    } else {
        PDDC_TRY(device_ptr_ok(d_counts, 4, "d_counts", true));
        PDDC_TRY(device_ptr_ok(d_nsym, 4, "d_nsym", true));
    }
    if (over_capacity(n, z_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "psk: %zu samples per receiver, z_stride %zu", n, z_stride);
    if (n > (size_t)1 << 40 || z_stride > (size_t)1 << 40 || sym_stride > (size_t)1 << 40 || char_stride > (size_t)1 << 40)
        return pddc_set_error_(PDDC_EINVAL, "psk: %zu samples per receiver are too many for one batch", n);
    const uint64_t sbound = psk_sym_bound(f, n), bound = psk_char_bound(f, n);
    if (char_stride < bound)
        return pddc_set_error_(PDDC_ECAPACITY, "psk: room for %zu characters per receiver, %zu samples can end %llu", char_stride, n,
                               (unsigned long long)bound);
    if (n && d_sym && sym_stride < sbound)
        return pddc_set_error_(PDDC_ECAPACITY, "psk: room for %zu symbols per receiver, %zu samples can hold %llu", sym_stride, n,
                               (unsigned long long)sbound);
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n) {
        /* nothing is launched and nothing carried moves; the counts of an empty batch are 0 */
        if (d_counts)
            PDDC_HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)f->nrx, st));
        if (d_nsym)
            PDDC_HIP_TRY(hipMemsetAsync(d_nsym, 0, sizeof(uint32_t) * (size_t)f->nrx, st));
        return PDDC_OK;
    }
    /* tiles read their neighbours' inputs: the bytes read and the bytes written must not meet */
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    if ((d_sym && (ranges_overlap(d_z, zbytes, d_sym, rows_extent(f->nrx, (size_t)sbound, sym_stride, sizeof(float2))) ||
                   ranges_overlap(d_z, zbytes, d_nsym, sizeof(uint32_t) * (size_t)f->nrx))) ||
        ranges_overlap(d_z, zbytes, d_chars, rows_extent(f->nrx, (size_t)bound, char_stride, sizeof(PskChar))) ||
        ranges_overlap(d_z, zbytes, d_counts, sizeof(uint32_t) * (size_t)f->nrx))
        return pddc_set_error_(PDDC_EINVAL, "psk: an output overlaps the input");
    PDDC_TRY(f->table.upload(st));
    PskArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.n = (long long)n;
    a.m0 = f->m;
    a.chars = static_cast<PskChar *>(d_chars);
    a.char_stride = (long long)char_stride;
    a.counts = static_cast<uint32_t *>(d_counts);
    a.sym = static_cast<float2 *>(d_sym);
    a.sym_stride = (long long)sym_stride;
    a.nsym = d_sym ? static_cast<uint32_t *>(d_nsym) : nullptr;
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
    PDDC_HIP_TRY(launch_psk(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    f->state.turn();
    f->hist.turn();
    f->m += n;
    f->launched = true;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    for (PskRx &r : f->table.host)
        if (r.flags & kPskMarks) {
            r.flags &= ~kPskMarks;
            f->table.dirty = true;
        }
    return PDDC_OK;
}

int pddc_psk_read(pddc_psk *f, pddc_psk_status *host, void *stream)
{
    if (!f || !host)
        return null_argument();
    PDDC_TRY(set_device(f->device));
    PDDC_TRY(read_back(f->host_state.data(), f->launched ? f->state.old() : nullptr, (size_t)f->nrx, (hipStream_t)stream));
    for (int j = 0; j < f->nrx; ++j) {
        /* a mark that no batch has read yet: the receiver reads as the next batch will find it */
        const uint32_t marks = f->table.host[(size_t)j].flags & kPskMarks;
        const bool fresh = !f->launched || (marks & kPskFresh);
        const PskState r = fresh ? PskState{} : f->host_state[(size_t)j];
        const bool afresh = fresh || marks;
        host[j] = pddc_psk_status{ r.f.chars, r.f.symbols, afresh ? 0u : r.acc, afresh ? 0u : r.f.reg, afresh ? 0.0f : r.d_last,
                                   afresh ? 0.0f : r.x_last };
    }
    return PDDC_OK;
}

} // extern "C"
