/*
 * ddc_psk.cpp -- host side of the PSK decoder (include/perseus_ddc.h, pddc_psk_*) on ddc_decoder.h: its modem bank, the
 * two capacity bounds, its sym output, the launch of a batch and the status read.  The kernel is in ddc_psk.hip, the
 * clock, the framing and the bounds' arithmetic in ddc_psk_bits.h.
 * Carried per receiver: its last W - 1 inputs and 128 filter outputs, the clock, the differential pair, the framing and
 * the counters.
 */
#include "ddc_decoder.h"
#include "ddc_psk.h"

using namespace pddc;

struct pddc_psk : DecoderBase<PskState, PskModem> {
    PDDC_LOCAL ~pddc_psk() = default;
};

static_assert(PDDC_PSK_ON == kDecOn && !(PDDC_PSK_RESTART & (kDecOn | kPskMarks)), "the kernel's flag bits are the header's");
static_assert(PDDC_PSK_LONG == kPskLongFlag, "the framing's character flag is the header's");
static_assert(sizeof(pddc_psk_char) == 16 && sizeof(PskChar) == 16 && offsetof(pddc_psk_char, code) == offsetof(PskChar, code) &&
                  offsetof(pddc_psk_char, nbits) == offsetof(PskChar, nbits) && offsetof(pddc_psk_char, flags) == offsetof(PskChar, flags) &&
                  offsetof(pddc_psk_char, quality) == offsetof(PskChar, quality),
              "the kernel's character record is the header's");
static_assert(sizeof(pddc_psk_modem) == sizeof(PskModem) && offsetof(pddc_psk_modem, step) == offsetof(PskModem, step),
              "the clock's modem is the header's");

/* RESTART, OFF -> ON, another modem: the carried inputs and outputs, the clock, the pair and the framing start afresh */
static constexpr DecoderKind kPsk{ "psk", "modem", 1, kDecOn, PDDC_PSK_RESTART, kPskMarks, kDecClear };

static uint64_t psk_sym_bound(const pddc_psk &f, uint64_t n) { return psk_most(n, f.distance); }
static uint64_t psk_char_bound(const pddc_psk &f, uint64_t n) { return psk_most_chars(psk_sym_bound(f, n)); }

extern "C" {

int pddc_psk_tile_outputs(void) { return kDecTile; }

int pddc_psk_create(pddc_psk **out, int device, int nrx, int window, int nmodems, const float *taps, const pddc_psk_modem *modems,
                    const pddc_psk_rx *rx)
{
    PDDC_TRY(decoder_create_ok(kPsk, out, nrx, rx, window, nmodems));
    if (!taps || !modems)
        return pddc_set_error_(PDDC_EINVAL, "psk: null taps or modems");
    PDDC_TRY(decoder_taps_ok(kPsk, taps, nmodems, window));
    for (int b = 0; b < nmodems; ++b)
        if (!psk_modem_ok(PskModem{ modems[b].inc, modems[b].q, modems[b].step }))
            return pddc_set_error_(PDDC_EINVAL, "psk: modem %d: 1 <= inc %u <= 2^29, 1 <= q %u <= 64 with 4 q inc <= 2^32, step %u <= inc", b,
                                   modems[b].inc, modems[b].q, modems[b].step);
    PDDC_TRY(decoder_rx_ok(kPsk, rx, &pddc_psk_rx::modem, nrx, nmodems));
    return stage_create(out, device, nrx, [&](pddc_psk &f) {
        for (int b = 0; b < nmodems; ++b)
            f.bank.push_back(PskModem{ modems[b].inc, modems[b].q, modems[b].step });
        f.distance = decoder_distance(f.bank, psk_distance);
        return decoder_fill(f, kPsk, window, decoder_rows(kPsk, nmodems, window, taps), rx, &pddc_psk_rx::modem, (size_t)psk_hist_slots(window));
    });
}

int pddc_psk_destroy(pddc_psk *f) { return stage_destroy(f); }

int pddc_psk_reset(pddc_psk *f) { return decoder_reset(f, kPsk); }

int pddc_psk_set_rx(pddc_psk *f, int rx, int modem, uint32_t flags) { return decoder_set_rx(f, kPsk, rx, modem, flags); }

int pddc_psk_max_syms(const pddc_psk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)psk_sym_bound(*f, n);
    return PDDC_OK;
}

int pddc_psk_max_chars(const pddc_psk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)psk_char_bound(*f, n);
    return PDDC_OK;
}

int pddc_psk_process(pddc_psk *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride, void *d_counts,
                     void *d_sym, size_t sym_stride, void *d_nsym, void *stream)
{
    if (!f)
        return null_argument();
    PDDC_TRY(decoder_ptrs_ok(n, d_z, d_chars, d_counts));
    if (n)
        PDDC_TRY(device_ptr_ok(d_sym, 8, "d_sym", true));
    PDDC_TRY(device_ptr_ok(d_nsym, 4, "d_nsym", !n || !d_sym));
    if (over_capacity(n, z_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "psk: %zu samples per receiver, z_stride %zu", n, z_stride);
    const uint64_t sbound = psk_sym_bound(*f, n), bound = psk_char_bound(*f, n);
    PDDC_TRY(decoder_sizes_ok(kPsk, n, z_stride, sym_stride, char_stride, bound));
    if (n && d_sym && sym_stride < sbound)
        return pddc_set_error_(PDDC_ECAPACITY, "psk: room for %zu symbols per receiver, %zu samples can hold %llu", sym_stride, n,
                               (unsigned long long)sbound);
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n) {
        PDDC_TRY(decoder_zero_counts(d_counts, f->nrx, st));
        return decoder_zero_counts(d_nsym, f->nrx, st);
    }
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    const bool sym_meets = d_sym && (ranges_overlap(d_z, zbytes, d_sym, rows_extent(f->nrx, (size_t)sbound, sym_stride, sizeof(float2))) ||
                                     ranges_overlap(d_z, zbytes, d_nsym, sizeof(uint32_t) * (size_t)f->nrx));
    PDDC_TRY(decoder_overlap_ok(kPsk, f->nrx, d_z, zbytes, sym_meets, d_chars, bound, char_stride, d_counts));
    PDDC_TRY(f->table.upload(st));
    PskArgs a{};
    decoder_args(a, *f, d_z, n, z_stride, d_chars, char_stride, d_counts);
    a.sym = static_cast<float2 *>(d_sym);
    a.sym_stride = (long long)sym_stride;
    a.nsym = d_sym ? static_cast<uint32_t *>(d_nsym) : nullptr;
    PDDC_HIP_TRY(launch_psk(a, st));
    decoder_accepted(f, kPsk, n);
    return PDDC_OK;
}

int pddc_psk_read(pddc_psk *f, pddc_psk_status *host, void *stream)
{
    PDDC_TRY(decoder_read_back(f, host, stream));
    for (int j = 0; j < f->nrx; ++j) {
        uint32_t marks;
        const PskState r = decoder_record(*f, kPsk, j, &marks);
        const bool afresh = !f->launched || marks;
        host[j] = pddc_psk_status{ r.f.chars, r.f.symbols, afresh ? 0u : r.acc, afresh ? 0u : r.f.reg, afresh ? 0.0f : r.d_last,
                                   afresh ? 0.0f : r.x_last };
    }
    return PDDC_OK;
}

} // extern "C"
