/*
 * ddc_morse.cpp -- host side of the Morse decoder (include/perseus_ddc.h, pddc_morse_*) on ddc_decoder.h: its keyer bank
 * and parameters, the capacity bound, its p output, the launch of a batch and the status read.  The kernel is in
 * ddc_morse.hip, the element timing and the bound's arithmetic in ddc_morse_timing.h.
 * Carried per receiver: its last W - 1 inputs, the meter, the key, the timing and the counters.
 */
#include "ddc_decoder.h"
#include "ddc_morse.h"

using namespace pddc;

struct pddc_morse : DecoderBase<MorseState, MorseKeyer> {
    PDDC_LOCAL ~pddc_morse() = default;
    MorseParams par{};
};

static_assert(PDDC_MORSE_ON == kDecOn && PDDC_MORSE_FIXED == kMorseFixed &&
                  !(PDDC_MORSE_RESTART & (kDecOn | kMorseFixed | kMorseMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_MORSE_WORD == kMorseWordFlag && PDDC_MORSE_LONG == kMorseLongFlag, "the timing's character flags are the header's");
static_assert(sizeof(pddc_morse_char) == 16 && sizeof(MorseChar) == 16 && offsetof(pddc_morse_char, code) == offsetof(MorseChar, code) &&
                  offsetof(pddc_morse_char, nel) == offsetof(MorseChar, nel) && offsetof(pddc_morse_char, flags) == offsetof(MorseChar, flags) &&
                  offsetof(pddc_morse_char, two) == offsetof(MorseChar, two),
              "the kernel's character record is the header's");
static_assert(sizeof(pddc_morse_keyer) == sizeof(MorseKeyer) && offsetof(pddc_morse_keyer, shift) == offsetof(MorseKeyer, shift),
              "the timing's keyer is the header's");

/* RESTART, OFF -> ON: the meter, the key and the timing start afresh with the inputs; another keyer: the same, but
 * the inputs stay */
static constexpr DecoderKind kMorse{ "morse", "keyer", 1, kDecOn | kMorseFixed, PDDC_MORSE_RESTART, kMorseMarks, kMorseRekey };

static uint64_t morse_bound(const pddc_morse &f, uint64_t n) { return morse_most(n, f.distance); }

extern "C" {

int pddc_morse_tile_outputs(void) { return kDecTile; }

int pddc_morse_create(pddc_morse **out, int device, int nrx, int window, int nkeyers, const float *taps,
                      const pddc_morse_keyer *keyers, const pddc_morse_params *par, const pddc_morse_rx *rx)
{
    PDDC_TRY(decoder_create_ok(kMorse, out, nrx, rx, window, nkeyers));
    if (!taps || !keyers || !par)
        return pddc_set_error_(PDDC_EINVAL, "morse: null taps, keyers or parameters");
    PDDC_TRY(decoder_taps_ok(kMorse, taps, nkeyers, window));
    for (int b = 0; b < nkeyers; ++b)
        if (!morse_keyer_ok(MorseKeyer{ keyers[b].two0, keyers[b].two_min, keyers[b].two_max, keyers[b].shift }))
            return pddc_set_error_(PDDC_EINVAL, "morse: keyer %d: 512 <= two_min %u <= two0 %u <= two_max %u <= 2^28, shift %u (0 .. 8)",
                                   b, keyers[b].two_min, keyers[b].two0, keyers[b].two_max, keyers[b].shift);
    if (!(par->a_off > 0.0f && par->a_off <= par->a_on && par->a_on < 1.0f))
        return pddc_set_error_(PDDC_EINVAL, "morse: 0 < a_off %g <= a_on %g < 1", (double)par->a_off, (double)par->a_on);
    if (!(par->rel >= 0.0f && par->rel <= 1.0f && par->relf >= 0.0f && par->relf <= 1.0f && par->ratio >= 1.0f))
        return pddc_set_error_(PDDC_EINVAL, "morse: rel %g and relf %g in [0, 1], ratio %g >= 1", (double)par->rel,
                               (double)par->relf, (double)par->ratio);
    PDDC_TRY(decoder_rx_ok(kMorse, rx, &pddc_morse_rx::keyer, nrx, nkeyers));
    return stage_create(out, device, nrx, [&](pddc_morse &f) {
        f.par = MorseParams{ par->a_on, par->a_off, par->rel, par->relf, par->ratio };
        for (int b = 0; b < nkeyers; ++b)
            f.bank.push_back(MorseKeyer{ keyers[b].two0, keyers[b].two_min, keyers[b].two_max, keyers[b].shift });
        f.distance = decoder_distance(f.bank, [](const MorseKeyer &k) { return morse_distance(k.two_min); });
        return decoder_fill(f, kMorse, window, decoder_rows(kMorse, nkeyers, window, taps), rx, &pddc_morse_rx::keyer, (size_t)(window > 1 ? window - 1 : 1));
    });
}

int pddc_morse_destroy(pddc_morse *f) { return stage_destroy(f); }

int pddc_morse_reset(pddc_morse *f) { return decoder_reset(f, kMorse); }

int pddc_morse_set_rx(pddc_morse *f, int rx, int keyer, uint32_t flags) { return decoder_set_rx(f, kMorse, rx, keyer, flags); }

int pddc_morse_max_chars(const pddc_morse *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)morse_bound(*f, n);
    return PDDC_OK;
}

int pddc_morse_process(pddc_morse *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                       void *d_counts, void *d_p, size_t p_stride, void *stream)
{
    if (!f)
        return null_argument();
    PDDC_TRY(decoder_ptrs_ok(n, d_z, d_chars, d_counts));
    PDDC_TRY(device_ptr_ok(d_p, 4, "d_p", true));
    if (over_capacity(n, z_stride) || (d_p && over_capacity(n, p_stride)))
        return pddc_set_error_(PDDC_ECAPACITY, "morse: %zu samples per receiver, z_stride %zu, p_stride %zu", n, z_stride, p_stride);
    const uint64_t bound = morse_bound(*f, n);
    PDDC_TRY(decoder_sizes_ok(kMorse, n, z_stride, p_stride, char_stride, bound));
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n)
        return decoder_zero_counts(d_counts, f->nrx, st);
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    const bool p_meets = d_p && ranges_overlap(d_z, zbytes, d_p, rows_extent(f->nrx, n, p_stride, sizeof(float)));
    PDDC_TRY(decoder_overlap_ok(kMorse, f->nrx, d_z, zbytes, p_meets, d_chars, bound, char_stride, d_counts));
    PDDC_TRY(f->table.upload(st));
    MorseArgs a{};
    decoder_args(a, *f, d_z, n, z_stride, d_chars, char_stride, d_counts);
    a.p = static_cast<float *>(d_p);
    a.p_stride = (long long)p_stride;
    a.par = f->par;
    PDDC_HIP_TRY(launch_morse(a, st));
    decoder_accepted(f, kMorse, n);
    return PDDC_OK;
}

int pddc_morse_read(pddc_morse *f, pddc_morse_status *host, void *stream)
{
    PDDC_TRY(decoder_read_back(f, host, stream));
    for (int j = 0; j < f->nrx; ++j) {
        uint32_t marks;
        const MorseState r = decoder_record(*f, kMorse, j, &marks);
        const bool afresh = !f->launched || marks;
        host[j] = pddc_morse_status{ r.t.chars, r.t.marks, afresh ? f->bank[(size_t)f->table.host[(size_t)j].bank].two0 : r.t.two,
                                     afresh ? 0u : r.t.nel, afresh ? 0u : r.key, afresh ? 0.0f : r.pk, afresh ? 0.0f : r.fl };
    }
    return PDDC_OK;
}

} // extern "C"
