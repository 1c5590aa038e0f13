/*
 * ddc_fsk.cpp -- host side of the FSK decoder (include/perseus_ddc.h, pddc_fsk_*) on ddc_decoder.h: its modem bank, the
 * capacity bound, its d output, the launch of a batch and the status read.  The kernel is in ddc_fsk.hip.
 * Carried per receiver: its last W - 1 inputs, the start-stop receiver's registers and the counters.
 */
#include "ddc_decoder.h"
#include "ddc_fsk.h"

using namespace pddc;

struct pddc_fsk : DecoderBase<FskState, FskModem> {
    PDDC_LOCAL ~pddc_fsk() = default;
};

static_assert(PDDC_FSK_ON == kDecOn && PDDC_FSK_REVERSE == kFskReverse && !(PDDC_FSK_RESTART & (kDecOn | kFskReverse | kFskMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_FSK_FRAMING == 1, "the kernel stores the stop element's `space` as the character's flags");
static_assert(PDDC_FSK_IDLE == kFskStIdle && PDDC_FSK_START == kFskStStart && PDDC_FSK_DATA == kFskStData &&
                  PDDC_FSK_STOP == kFskStStop,
              "the kernel's state numbers are the header's");
static_assert(sizeof(pddc_fsk_char) == 16 && sizeof(FskChar) == 16 && offsetof(pddc_fsk_char, code) == offsetof(FskChar, code) &&
                  offsetof(pddc_fsk_char, flags) == offsetof(FskChar, flags) &&
                  offsetof(pddc_fsk_char, quality) == offsetof(FskChar, quality),
              "the kernel's character record is the header's");

/* another modem: the inputs stay, a character in progress is dropped */
static constexpr DecoderKind kFsk{ "fsk", "modem", 4, kDecOn | kFskReverse, PDDC_FSK_RESTART, kFskMarks, kFskIdle };

/* samples from the edge to the STOP strobe: the (nbits + 2)-th carry of an accumulator that starts at 2^31 and moves
 * by inc, ceil((nbits + 1.5) 2^32 / inc) */
static uint64_t fsk_period(const FskModem &mo)
{
    const uint64_t num = (uint64_t)(2u * mo.nbits + 3u) << 31;
    return (num + mo.inc - 1u) / mo.inc;
}

/* the most over the bank of n div P + 1: the shortest period's */
static uint64_t fsk_bound(const pddc_fsk &f, uint64_t n) { return n / f.distance + 1u; }

extern "C" {

int pddc_fsk_tile_outputs(void) { return kDecTile; }

int pddc_fsk_create(pddc_fsk **out, int device, int nrx, int window, int nmodems, const float *taps, const uint32_t *inc,
                    const int *nbits, const pddc_fsk_rx *rx)
{
    PDDC_TRY(decoder_create_ok(kFsk, out, nrx, rx, window, nmodems));
    if (!taps || !inc || !nbits)
        return pddc_set_error_(PDDC_EINVAL, "fsk: null taps, inc or nbits");
    PDDC_TRY(decoder_taps_ok(kFsk, taps, nmodems, 4 * window));
    for (int b = 0; b < nmodems; ++b)
        if (inc[b] < 1u || inc[b] > (1u << 30) || nbits[b] < 5 || nbits[b] > 8)
            return pddc_set_error_(PDDC_EINVAL, "fsk: modem %d: inc %u (1 .. 2^30), nbits %d (5 .. 8)", b, inc[b], nbits[b]);
    PDDC_TRY(decoder_rx_ok(kFsk, rx, &pddc_fsk_rx::modem, nrx, nmodems));
    return stage_create(out, device, nrx, [&](pddc_fsk &f) {
        for (int b = 0; b < nmodems; ++b)
            f.bank.push_back(FskModem{ inc[b], (uint32_t)nbits[b] });
        f.distance = decoder_distance(f.bank, fsk_period);
        /* taps[b][0][t] = hm, taps[b][1][t] = hs (re, im) -> per tap (hm.re, hm.im, hs.re, hs.im) */
        const size_t Wz = (size_t)window;
        const std::vector<float> rows =
            decoder_rows(kFsk, nmodems, window, [&](size_t b, size_t t, size_t c) { return taps[((b * 2 + c / 2) * Wz + t) * 2 + c % 2]; });
        return decoder_fill(f, kFsk, window, rows, rx, &pddc_fsk_rx::modem, (size_t)(window > 1 ? window - 1 : 1));
    });
}

int pddc_fsk_destroy(pddc_fsk *f) { return stage_destroy(f); }

int pddc_fsk_reset(pddc_fsk *f) { return decoder_reset(f, kFsk); }

int pddc_fsk_set_rx(pddc_fsk *f, int rx, int modem, uint32_t flags) { return decoder_set_rx(f, kFsk, rx, modem, flags); }

int pddc_fsk_max_chars(const pddc_fsk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)fsk_bound(*f, n);
    return PDDC_OK;
}

int pddc_fsk_process(pddc_fsk *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                     void *d_counts, void *d_d, size_t d_stride, void *stream)
{
    if (!f)
        return null_argument();
    PDDC_TRY(decoder_ptrs_ok(n, d_z, d_chars, d_counts));
    PDDC_TRY(device_ptr_ok(d_d, 4, "d_d", true));
    if (over_capacity(n, z_stride) || (d_d && over_capacity(n, d_stride)))
        return pddc_set_error_(PDDC_ECAPACITY, "fsk: %zu samples per receiver, z_stride %zu, d_stride %zu", n, z_stride, d_stride);
    const uint64_t bound = fsk_bound(*f, n);
    PDDC_TRY(decoder_sizes_ok(kFsk, n, z_stride, d_stride, char_stride, bound));
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n)
        return decoder_zero_counts(d_counts, f->nrx, st);
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    const bool d_meets = d_d && ranges_overlap(d_z, zbytes, d_d, rows_extent(f->nrx, n, d_stride, sizeof(float)));
    PDDC_TRY(decoder_overlap_ok(kFsk, f->nrx, d_z, zbytes, d_meets, d_chars, bound, char_stride, d_counts));
    PDDC_TRY(f->table.upload(st));
    FskArgs a{};
    decoder_args(a, *f, d_z, n, z_stride, d_chars, char_stride, d_counts);
    a.d = static_cast<float *>(d_d);
    a.d_stride = (long long)d_stride;
    PDDC_HIP_TRY(launch_fsk(a, st));
    decoder_accepted(f, kFsk, n);
    return PDDC_OK;
}

int pddc_fsk_read(pddc_fsk *f, pddc_fsk_status *host, void *stream)
{
    PDDC_TRY(decoder_read_back(f, host, stream));
    for (int j = 0; j < f->nrx; ++j) {
        uint32_t marks;
        const FskState r = decoder_record(*f, kFsk, j, &marks);
        host[j] = pddc_fsk_status{ r.chars, r.framing, r.false_starts, marks ? (uint32_t)PDDC_FSK_IDLE : r.state, r.d_last };
    }
    return PDDC_OK;
}

} // extern "C"
