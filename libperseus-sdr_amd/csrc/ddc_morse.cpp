/*
 * ddc_morse.cpp -- host side of the Morse decoder (include/perseus_ddc.h, pddc_morse_*): the object, its keyer bank and
 * receiver table, the capacity bound, the launch of a batch and the status read.  The kernel is in ddc_morse.hip, the
 * element timing and the bound's arithmetic in ddc_morse_timing.h.
 * What is carried per receiver (its last W - 1 inputs, the meter, the key, the timing and the counters) lives on the
 * device in two pairs of records, read and written in turn; nothing on the device is cleared from the host: the marks
 * (fresh: create, reset; clear: RESTART, OFF -> ON; rekey: another keyer) live in the table, which is uploaded in stream
 * order when it changed, and go once a launch that read them was accepted.  The bank is uploaded once, at create.
 */
#include "ddc_stage.h"
#include "ddc_morse.h"

#include <cmath>

using namespace pddc;

struct pddc_morse : StageBase {
    PDDC_LOCAL ~pddc_morse() = default;
    int nkeyers = 0, window = 0;
    MorseParams par{};
    std::vector<MorseKeyer> bank;                   /* the host's copy: set_rx, max_chars, read                    */
    uint64_t distance = 0;                          /* the least samples between two emissions, over the bank      */
    RxTable<MorseRx> table;
    DevBuf<float> taps;                             /* [nkeyers][morse_row(W)]                                     */
    DevBuf<MorseKeyer> keyers;
    std::vector<MorseState> host_state;             /* where read() lands the records                              */
    bool launched = false;                          /* a batch since create / reset: the records were written      */
    Carried<MorseState> state;
    Carried<float2> hist;                           /* [nrx][W - 1]                                                */
    uint64_t m = 0;                                 /* samples per receiver since create / reset                   */
};

static_assert(PDDC_MORSE_ON == kMorseOn && PDDC_MORSE_FIXED == kMorseFixed &&
                  !(PDDC_MORSE_RESTART & (kMorseOn | kMorseFixed | kMorseMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_MORSE_WORD == kMorseWordFlag && PDDC_MORSE_LONG == kMorseLongFlag, "the timing's character flags are the header's");
static_assert(sizeof(pddc_morse_char) == 16 && sizeof(MorseChar) == 16 && offsetof(pddc_morse_char, code) == offsetof(MorseChar, code) &&
                  offsetof(pddc_morse_char, nel) == offsetof(MorseChar, nel) && offsetof(pddc_morse_char, flags) == offsetof(MorseChar, flags) &&
                  offsetof(pddc_morse_char, two) == offsetof(MorseChar, two),
              "the kernel's character record is the header's");
static_assert(sizeof(pddc_morse_keyer) == sizeof(MorseKeyer) && offsetof(pddc_morse_keyer, shift) == offsetof(MorseKeyer, shift),
              "the timing's keyer is the header's");

static constexpr uint32_t kMorseUserFlags = PDDC_MORSE_ON | PDDC_MORSE_FIXED | PDDC_MORSE_RESTART;

static uint64_t morse_bound(const pddc_morse *f, uint64_t n) { return morse_most(n, f->distance); }

extern "C" {

int pddc_morse_tile_outputs(void) { return kMorseTile; }

int pddc_morse_create(pddc_morse **out, int device, int nrx, int window, int nkeyers, const float *taps,
                      const pddc_morse_keyer *keyers, const pddc_morse_params *par, const pddc_morse_rx *rx)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kMorseMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "morse: %d receivers (1 .. %d) and their keyers", nrx, kMorseMaxRx);
    if (window < 1 || window > kMorseMaxWindow || nkeyers < 1 || nkeyers > kMorseMaxKeyers)
        return pddc_set_error_(PDDC_EINVAL, "morse: %d keyers (1 .. %d) with a window of %d (1 .. %d)", nkeyers, kMorseMaxKeyers,
                               window, kMorseMaxWindow);
    if (!taps || !keyers || !par)
        return pddc_set_error_(PDDC_EINVAL, "morse: null taps, keyers or parameters");
    for (int i = 0; i < nkeyers * window; ++i)
        if (!std::isfinite(taps[i]))
            return pddc_set_error_(PDDC_EINVAL, "morse: keyer %d: a tap is not finite", i / window);
    for (int b = 0; b < nkeyers; ++b)
        if (!morse_keyer_ok(MorseKeyer{ keyers[b].two0, keyers[b].two_min, keyers[b].two_max, keyers[b].shift }))
            return pddc_set_error_(PDDC_EINVAL, "morse: keyer %d: 512 <= two_min %u <= two0 %u <= two_max %u <= 2^28, shift %u (0 .. 8)",
                                   b, keyers[b].two_min, keyers[b].two0, keyers[b].two_max, keyers[b].shift);
    if (!(par->a_off > 0.0f && par->a_off <= par->a_on && par->a_on < 1.0f))
        return pddc_set_error_(PDDC_EINVAL, "morse: 0 < a_off %g <= a_on %g < 1", (double)par->a_off, (double)par->a_on);
    if (!(par->rel >= 0.0f && par->rel <= 1.0f && par->relf >= 0.0f && par->relf <= 1.0f && par->ratio >= 1.0f))
        return pddc_set_error_(PDDC_EINVAL, "morse: rel %g and relf %g in [0, 1], ratio %g >= 1", (double)par->rel,
                               (double)par->relf, (double)par->ratio);
    for (int j = 0; j < nrx; ++j)
        if (rx[j].keyer < 0 || rx[j].keyer >= nkeyers || (rx[j].flags & ~kMorseUserFlags))
            return pddc_set_error_(PDDC_EINVAL, "morse: receiver %d: keyer %d (0 .. %d), flags 0x%x", j, rx[j].keyer, nkeyers - 1,
                                   rx[j].flags);
    return stage_create(out, device, nrx, [&](pddc_morse &f) {
        f.nkeyers = nkeyers;
        f.window = window;
        f.par = MorseParams{ par->a_on, par->a_off, par->rel, par->relf, par->ratio };
        f.host_state.resize((size_t)nrx);
        f.distance = ~(uint64_t)0;
        for (int b = 0; b < nkeyers; ++b) {
            f.bank.push_back(MorseKeyer{ keyers[b].two0, keyers[b].two_min, keyers[b].two_max, keyers[b].shift });
            const uint64_t d = morse_distance(keyers[b].two_min);
            f.distance = d < f.distance ? d : f.distance;
        }
        for (int j = 0; j < nrx; ++j)
            f.table.host.push_back(MorseRx{ rx[j].keyer, (rx[j].flags & (kMorseOn | kMorseFixed)) | kMorseFresh });
        const size_t row = (size_t)morse_row(window), Wz = (size_t)window;
        std::vector<float> rows((size_t)nkeyers * row, 0.0f);
        for (size_t b = 0; b < (size_t)nkeyers; ++b)
            for (size_t t = 0; t < Wz; ++t)
                rows[b * row + t] = taps[b * Wz + t];
        PDDC_TRY(f.taps.alloc_copy(rows));
        PDDC_TRY(f.keyers.alloc_copy(f.bank));
        PDDC_TRY(f.table.alloc());
        PDDC_TRY(f.state.alloc((size_t)nrx));
        return f.hist.alloc((size_t)nrx * (size_t)(window > 1 ? window - 1 : 1));
    });
}

int pddc_morse_destroy(pddc_morse *f) { return stage_destroy(f); }

int pddc_morse_reset(pddc_morse *f)
{
    PDDC_TRY(stage_quiesce(f));
    f->m = 0;
    f->launched = false;
    for (MorseRx &r : f->table.host)
        r.flags = (r.flags & ~kMorseMarks) | kMorseFresh;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_morse_set_rx(pddc_morse *f, int rx, int keyer, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(f, "morse", rx));
    if (keyer < 0 || keyer >= f->nkeyers || (flags & ~kMorseUserFlags))
        return pddc_set_error_(PDDC_EINVAL, "morse: keyer %d (0 .. %d), flags 0x%x", keyer, f->nkeyers - 1, flags);
    MorseRx &r = f->table.host[(size_t)rx];
    uint32_t marks = r.flags & kMorseMarks;
    /* RESTART, OFF -> ON: the carried inputs, the meter, the key and the timing start afresh, the counters stay;
     * another keyer: the same, but the inputs stay */
    if ((flags & PDDC_MORSE_RESTART) || (!(r.flags & kMorseOn) && (flags & kMorseOn)))
        marks |= kMorseClear;
    if (keyer != r.keyer)
        marks |= kMorseRekey;
    r.keyer = keyer;
    r.flags = (flags & (kMorseOn | kMorseFixed)) | marks;
    f->table.dirty = true;
    return PDDC_OK;
}

int pddc_morse_max_chars(const pddc_morse *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)morse_bound(f, n);
    return PDDC_OK;
}

int pddc_morse_process(pddc_morse *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                       void *d_counts, void *d_p, size_t p_stride, void *stream)
{
    if (!f)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_chars, 8, "d_chars"));
        PDDC_TRY(device_ptr_ok(d_counts, 4, "d_counts"));
    } else
        PDDC_TRY(device_ptr_ok(d_counts, 4, "d_counts", true));
    PDDC_TRY(device_ptr_ok(d_p, 4, "d_p", true));
    if (over_capacity(n, z_stride) || (d_p && over_capacity(n, p_stride)))
        return pddc_set_error_(PDDC_ECAPACITY, "morse: %zu samples per receiver, z_stride %zu, p_stride %zu", n, z_stride, p_stride);
    if (n > (size_t)1 << 40 || z_stride > (size_t)1 << 40 || p_stride > (size_t)1 << 40 || char_stride > (size_t)1 << 40)
        return pddc_set_error_(PDDC_EINVAL, "morse: %zu samples per receiver are too many for one batch", n);
    const uint64_t bound = morse_bound(f, n);
    if (char_stride < bound)
        return pddc_set_error_(PDDC_ECAPACITY, "morse: room for %zu characters per receiver, %zu samples can end %llu", char_stride,
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
    if ((d_p && ranges_overlap(d_z, zbytes, d_p, rows_extent(f->nrx, n, p_stride, sizeof(float)))) ||
        ranges_overlap(d_z, zbytes, d_chars, rows_extent(f->nrx, (size_t)bound, char_stride, sizeof(MorseChar))) ||
        ranges_overlap(d_z, zbytes, d_counts, sizeof(uint32_t) * (size_t)f->nrx))
        return pddc_set_error_(PDDC_EINVAL, "morse: an output overlaps the input");
    PDDC_TRY(f->table.upload(st));
    MorseArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.n = (long long)n;
    a.m0 = f->m;
    a.chars = static_cast<MorseChar *>(d_chars);
    a.char_stride = (long long)char_stride;
    a.counts = static_cast<uint32_t *>(d_counts);
    a.p = static_cast<float *>(d_p);
    a.p_stride = (long long)p_stride;
    a.taps = f->taps.get();
    a.keyers = f->keyers.get();
    a.rx = f->table.dev();
    a.state = f->state.old();
    a.new_state = f->state.next();
    a.hist = f->hist.old();
    a.new_hist = f->hist.next();
    a.par = f->par;
    a.nrx = f->nrx;
    a.nkeyers = f->nkeyers;
    a.window = f->window;
    PDDC_HIP_TRY(launch_morse(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    f->state.turn();
    f->hist.turn();
    f->m += n;
    f->launched = true;
    /* the records are written now: the marks go, and the table on the device follows with the next batch */
    for (MorseRx &r : f->table.host)
        if (r.flags & kMorseMarks) {
            r.flags &= ~kMorseMarks;
            f->table.dirty = true;
        }
    return PDDC_OK;
}

int pddc_morse_read(pddc_morse *f, pddc_morse_status *host, void *stream)
{
    if (!f || !host)
        return null_argument();
    PDDC_TRY(set_device(f->device));
    PDDC_TRY(read_back(f->host_state.data(), f->launched ? f->state.old() : nullptr, (size_t)f->nrx, (hipStream_t)stream));
    for (int j = 0; j < f->nrx; ++j) {
        /* a mark that no batch has read yet: the receiver reads as the next batch will find it */
        const MorseRx &rx = f->table.host[(size_t)j];
        const uint32_t marks = rx.flags & kMorseMarks;
        const bool fresh = !f->launched || (marks & kMorseFresh);
        const MorseState r = fresh ? MorseState{} : f->host_state[(size_t)j];
        const bool afresh = fresh || marks;
        host[j] = pddc_morse_status{ r.t.chars, r.t.marks, afresh ? f->bank[(size_t)rx.keyer].two0 : r.t.two, afresh ? 0u : r.t.nel,
                                     afresh ? 0u : r.key, afresh ? 0.0f : r.pk, afresh ? 0.0f : r.fl };
    }
    return PDDC_OK;
}

} // extern "C"
