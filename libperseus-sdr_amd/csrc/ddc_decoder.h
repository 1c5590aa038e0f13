/*
 * ddc_decoder.h -- what the host files of the decoders (fsk, morse, psk, sitor; fax, whose records are lines) share on top of ddc_stage.h: the
 * handle's common members and the common ends of create / reset / set_rx / process / read.  A decoder's own file keeps
 * its bank entries with their validation and `distance`, its extra outputs, its kernel arguments and its status record.
 * What is carried per receiver lives on the device in two pairs of records, read and written in turn; nothing on the
 * device is cleared from the host: the marks (kDecFresh: create, reset; kDecClear: RESTART, OFF -> ON; the decoder's
 * third, if it has one) live in the table, which is uploaded in stream order when it changed, and go once a launch that
 * read them was accepted.  The bank is uploaded once, at create.
 * Host only; internal, nothing here is exported.
 */
#ifndef PDDC_DDC_DECODER_H
#define PDDC_DDC_DECODER_H

#include "ddc_stage.h"
#include "ddc_decoder_rx.h"

namespace pddc {

/* how the messages name a decoder and its bank entries, and its receiver flags */
struct DecoderKind {
    const char *stage, *noun; /* "fsk", "modem"                                                                  */
    int coef;                 /* floats per tap on the device                                                    */
    uint32_t keep;            /* the header's flags the table holds (ON and the decoder's own)                   */
    uint32_t restart;         /* the header's RESTART: with `keep`, what a caller may pass                       */
    uint32_t marks;           /* the marks this decoder uses                                                     */
    uint32_t rebank;          /* the mark that another bank entry sets                                           */
};

template <class State, class Bank> struct DecoderBase : StageBase {
    int nbank = 0, window = 0;
    std::vector<Bank> bank;                         /* the host's copy: set_rx, the bounds, read                   */
    uint64_t distance = 0;                          /* the least samples between two characters (psk: strobes), over the bank */
    RxTable<DecRx> table;
    DevBuf<float> taps;                             /* [nbank][dec_row(W)][coef]                                   */
    DevBuf<Bank> dev_bank;
    std::vector<State> host_state;                  /* where read() lands the records                              */
    bool launched = false;                          /* a batch since create / reset: the records were written      */
    Carried<State> state;
    Carried<float2> hist;                           /* [nrx][W - 1], psk: and its filter outputs                   */
    uint64_t m = 0;                                 /* samples per receiver since create / reset                   */
};

/* create: what is tested first (then the decoder's own arrays, decoder_taps_ok, its bank entries, decoder_rx_ok) */
template <class H> int decoder_create_ok(const DecoderKind &k, H **out, int nrx, const void *rx, int window, int nbank)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kDecMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "%s: %d receivers (1 .. %d) and their %ss", k.stage, nrx, kDecMaxRx, k.noun);
    if (window < 1 || window > kDecMaxWindow || nbank < 1 || nbank > kDecMaxBank)
        return pddc_set_error_(PDDC_EINVAL, "%s: %d %ss (1 .. %d) with a window of %d (1 .. %d)", k.stage, nbank, k.noun, kDecMaxBank,
                               window, kDecMaxWindow);
    return PDDC_OK;
}

/* taps: nbank entries of `per` floats each */
inline int decoder_taps_ok(const DecoderKind &k, const float *taps, int nbank, int per)
{
    for (int i = 0; i < nbank * per; ++i)
        if (!std::isfinite(taps[i]))
            return pddc_set_error_(PDDC_EINVAL, "%s: %s %d: a tap is not finite", k.stage, k.noun, i / per);
    return PDDC_OK;
}

/* the header's receiver entries, whose bank index is the member `bank` */
template <class Rx> int decoder_rx_ok(const DecoderKind &k, const Rx *rx, int Rx::*bank, int nrx, int nbank)
{
    for (int j = 0; j < nrx; ++j)
        if (rx[j].*bank < 0 || rx[j].*bank >= nbank || (rx[j].flags & ~(k.keep | k.restart)))
            return pddc_set_error_(PDDC_EINVAL, "%s: receiver %d: %s %d (0 .. %d), flags 0x%x", k.stage, j, k.noun, rx[j].*bank,
                                   nbank - 1, rx[j].flags);
    return PDDC_OK;
}

/* the taps as the tap loop reads them: per entry dec_row(W) taps of k.coef floats, tap(b, t, c) in front and zeros behind */
template <class Tap> std::vector<float> decoder_rows(const DecoderKind &k, int nbank, int window, Tap tap)
{
    const size_t row = (size_t)dec_row(window), coef = (size_t)k.coef;
    std::vector<float> rows((size_t)nbank * row * coef, 0.0f);
    for (size_t b = 0; b < (size_t)nbank; ++b)
        for (size_t t = 0; t < (size_t)window; ++t)
            for (size_t c = 0; c < coef; ++c)
                rows[(b * row + t) * coef + c] = tap(b, t, c);
    return rows;
}

/* ... from taps[b][t][c], the caller's own layout where the kernel's is the same */
inline std::vector<float> decoder_rows(const DecoderKind &k, int nbank, int window, const float *taps)
{
    const size_t per = (size_t)window * (size_t)k.coef;
    return decoder_rows(k, nbank, window, [=](size_t b, size_t t, size_t c) { return taps[b * per + t * (size_t)k.coef + c]; });
}

/* `distance`: the least dist(entry) over the bank */
template <class Bank, class Dist> uint64_t decoder_distance(const std::vector<Bank> &bank, Dist dist)
{
    uint64_t least = ~(uint64_t)0;
    for (const Bank &b : bank)
        least = dist(b) < least ? dist(b) : least;
    return least;
}

/* create's fill behind f.bank: the members, the table (every receiver fresh) and the allocations; `hist_slots`: float2
 * a receiver carries in front of a batch */
template <class D, class Rx>
int decoder_fill(D &f, const DecoderKind &k, int window, const std::vector<float> &rows, const Rx *rx, int Rx::*bank, size_t hist_slots)
{
    f.nbank = (int)f.bank.size();
    f.window = window;
    f.host_state.resize((size_t)f.nrx);
    for (int j = 0; j < f.nrx; ++j)
        f.table.host.push_back(DecRx{ rx[j].*bank, (rx[j].flags & k.keep) | kDecFresh });
    PDDC_TRY(f.taps.alloc_copy(rows));
    PDDC_TRY(f.dev_bank.alloc_copy(f.bank));
    PDDC_TRY(f.table.alloc());
    PDDC_TRY(f.state.alloc((size_t)f.nrx));
    return f.hist.alloc((size_t)f.nrx * hist_slots);
}

template <class D> int decoder_reset(D *f, const DecoderKind &k)
{
    PDDC_TRY(stage_quiesce(f));
    f->m = 0;
    f->launched = false;
    for (DecRx &r : f->table.host)
        r.flags = (r.flags & ~k.marks) | kDecFresh;
    f->table.dirty = true;
    return PDDC_OK;
}

/* RESTART, OFF -> ON: kDecClear (the carried inputs and the decoder's state start afresh, the counters stay); another
 * bank entry: k.rebank */
template <class D> int decoder_set_rx(D *f, const DecoderKind &k, int rx, int bank, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(f, k.stage, rx));
    if (bank < 0 || bank >= f->nbank || (flags & ~(k.keep | k.restart)))
        return pddc_set_error_(PDDC_EINVAL, "%s: %s %d (0 .. %d), flags 0x%x", k.stage, k.noun, bank, f->nbank - 1, flags);
    DecRx &r = f->table.host[(size_t)rx];
    uint32_t marks = r.flags & k.marks;
    if ((flags & k.restart) || (!(r.flags & kDecOn) && (flags & kDecOn)))
        marks |= kDecClear;
    if (bank != r.bank)
        marks |= k.rebank;
    r.bank = bank;
    r.flags = (flags & k.keep) | marks;
    f->table.dirty = true;
    return PDDC_OK;
}

/* process(): the pointers every decoder takes */
inline int decoder_ptrs_ok(size_t n, const void *d_z, const void *d_chars, const void *d_counts)
{
    if (!n)
        return device_ptr_ok(d_counts, 4, "d_counts", true);
    PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
    PDDC_TRY(device_ptr_ok(d_chars, 8, "d_chars"));
    return device_ptr_ok(d_counts, 4, "d_counts");
}

/* ... the sizes (`extra_stride`: of the decoder's own output), and the room for `bound` characters */
inline int decoder_sizes_ok(const DecoderKind &k, size_t n, size_t z_stride, size_t extra_stride, size_t char_stride, uint64_t bound)
{
    const size_t most = (size_t)1 << 40;
    if (n > most || z_stride > most || extra_stride > most || char_stride > most)
        return pddc_set_error_(PDDC_EINVAL, "%s: %zu samples per receiver are too many for one batch", k.stage, n);
    if (char_stride < bound)
        return pddc_set_error_(PDDC_ECAPACITY, "%s: room for %zu characters per receiver, %zu samples can end %llu", k.stage,
                               char_stride, n, (unsigned long long)bound);
    return PDDC_OK;
}

/* ... an empty batch: nothing is launched and nothing carried moves; its counts are 0 */
inline int decoder_zero_counts(void *d_counts, int nrx, hipStream_t st)
{
    if (d_counts)
        PDDC_HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)nrx, st));
    return PDDC_OK;
}

/* ... tiles read their neighbours' inputs: the bytes read and the bytes written must not meet.  `extra`: the decoder's
 * own outputs meet z; the characters are records of 16 bytes */
inline int decoder_overlap_ok(const DecoderKind &k, int nrx, const void *d_z, size_t zbytes, bool extra, const void *d_chars,
                              uint64_t bound, size_t char_stride, const void *d_counts)
{
    if (extra || ranges_overlap(d_z, zbytes, d_chars, rows_extent(nrx, (size_t)bound, char_stride, 16)) ||
        ranges_overlap(d_z, zbytes, d_counts, sizeof(uint32_t) * (size_t)nrx))
        return pddc_set_error_(PDDC_EINVAL, "%s: an output overlaps the input", k.stage);
    return PDDC_OK;
}

/* ... the kernel arguments every decoder has */
template <class Args, class D>
void decoder_args(Args &a, const D &f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride, void *d_counts)
{
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.n = (long long)n;
    a.m0 = f.m;
    a.chars = static_cast<decltype(a.chars)>(d_chars);
    a.char_stride = (long long)char_stride;
    a.counts = static_cast<uint32_t *>(d_counts);
    a.taps = f.taps.get();
    a.bank = f.dev_bank.get();
    a.rx = f.table.dev();
    a.state = f.state.old();
    a.new_state = f.state.next();
    a.hist = f.hist.old();
    a.new_hist = f.hist.next();
    a.nrx = f.nrx;
    a.nbank = f.nbank;
    a.window = f.window;
}

/* ... the launch was accepted: only now do the host-side counters move.  The records are written now: the marks go,
 * and the table on the device follows with the next batch */
template <class D> void decoder_accepted(D *f, const DecoderKind &k, size_t n)
{
    f->state.turn();
    f->hist.turn();
    f->m += n;
    f->launched = true;
    for (DecRx &r : f->table.host)
        if (r.flags & k.marks) {
            r.flags &= ~k.marks;
            f->table.dirty = true;
        }
}

/* read(): the records behind the batches submitted so far (it waits for them) into f->host_state */
template <class D> int decoder_read_back(D *f, const void *host, void *stream)
{
    if (!f || !host)
        return null_argument();
    PDDC_TRY(set_device(f->device));
    return read_back(f->host_state.data(), f->launched ? f->state.old() : nullptr, (size_t)f->nrx, (hipStream_t)stream);
}

/* ... receiver j as the next batch will find it: *marks, the marks no batch has read yet, and its record (zero where it
 * is fresh) */
template <class State, class Bank>
State decoder_record(const DecoderBase<State, Bank> &f, const DecoderKind &k, int j, uint32_t *marks)
{
    *marks = f.table.host[(size_t)j].flags & k.marks;
    return !f.launched || (*marks & kDecFresh) ? State{} : f.host_state[(size_t)j];
}

} // namespace pddc
#endif
