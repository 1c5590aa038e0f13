/*
 * ddc_sitor.cpp -- host side of the SITOR decoder (include/perseus_ddc.h, pddc_sitor_*) on ddc_decoder.h: its modem bank,
 * the two capacity bounds, its soft output, the launch of a batch and the status read.  The kernel is in ddc_sitor.hip,
 * the clock, the framing and the bounds' arithmetic in ddc_sitor_bits.h.
 * Carried per receiver: its last W - 1 inputs, the clock, the previous decision, the framing and the counters.
 */
#include "ddc_decoder.h"
#include "ddc_sitor.h"

using namespace pddc;

struct pddc_sitor : DecoderBase<SitorState, SitorModem> {
    PDDC_LOCAL ~pddc_sitor() = default;
};

static_assert(PDDC_SITOR_ON == kDecOn && PDDC_SITOR_REVERSE == kSitorReverse &&
                  !(PDDC_SITOR_RESTART & (kDecOn | kSitorReverse | kSitorMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_SITOR_VALID == kSitorValid, "the framing's character flag is the header's");
static_assert(sizeof(pddc_sitor_char) == 16 && sizeof(SitorChar) == 16 && offsetof(pddc_sitor_char, code) == offsetof(SitorChar, code) &&
                  offsetof(pddc_sitor_char, flags) == offsetof(SitorChar, flags) &&
                  offsetof(pddc_sitor_char, quality) == offsetof(SitorChar, quality),
              "the kernel's character record is the header's");
static_assert(sizeof(pddc_sitor_modem) == sizeof(SitorModem) && offsetof(pddc_sitor_modem, step) == offsetof(SitorModem, step) &&
                  offsetof(pddc_sitor_modem, lock) == offsetof(SitorModem, lock) &&
                  offsetof(pddc_sitor_modem, unlock) == offsetof(SitorModem, unlock),
              "the clock's modem is the header's");

/* another modem: the inputs, the clock and the previous decision stay, the framing starts afresh */
static constexpr DecoderKind kSitor{ "sitor", "modem", 4, kDecOn | kSitorReverse, PDDC_SITOR_RESTART, kSitorMarks, kSitorReframe };

static uint64_t sitor_sym_bound(const pddc_sitor &f, uint64_t n) { return sitor_most(n, f.distance); }
static uint64_t sitor_char_bound(const pddc_sitor &f, uint64_t n) { return sitor_most_chars(sitor_sym_bound(f, n)); }

extern "C" {

int pddc_sitor_tile_outputs(void) { return kDecTile; }

int pddc_sitor_create(pddc_sitor **out, int device, int nrx, int window, int nmodems, const float *taps,
                      const pddc_sitor_modem *modems, const pddc_sitor_rx *rx)
{
    PDDC_TRY(decoder_create_ok(kSitor, out, nrx, rx, window, nmodems));
    if (!taps || !modems)
        return pddc_set_error_(PDDC_EINVAL, "sitor: null taps or modems");
    PDDC_TRY(decoder_taps_ok(kSitor, taps, nmodems, 4 * window));
    for (int b = 0; b < nmodems; ++b)
        if (!sitor_modem_ok(SitorModem{ modems[b].inc, modems[b].step, modems[b].lock, modems[b].unlock }))
            return pddc_set_error_(PDDC_EINVAL, "sitor: modem %d: 1 <= inc %u <= 2^29, step %u <= inc, lock %u (0, 2 .. 4), unlock %u (1 .. 15)",
                                   b, modems[b].inc, modems[b].step, modems[b].lock, modems[b].unlock);
    PDDC_TRY(decoder_rx_ok(kSitor, rx, &pddc_sitor_rx::modem, nrx, nmodems));
    return stage_create(out, device, nrx, [&](pddc_sitor &f) {
        for (int b = 0; b < nmodems; ++b)
            f.bank.push_back(SitorModem{ modems[b].inc, modems[b].step, modems[b].lock, modems[b].unlock });
        f.distance = decoder_distance(f.bank, sitor_distance);
        /* taps[b][0][t] = hm, taps[b][1][t] = hs (re, im) -> per tap (hm.re, hm.im, hs.re, hs.im), as fsk */
        const size_t Wz = (size_t)window;
        const std::vector<float> rows =
            decoder_rows(kSitor, nmodems, window, [&](size_t b, size_t t, size_t c) { return taps[((b * 2 + c / 2) * Wz + t) * 2 + c % 2]; });
        return decoder_fill(f, kSitor, window, rows, rx, &pddc_sitor_rx::modem, (size_t)(window > 1 ? window - 1 : 1));
    });
}

int pddc_sitor_destroy(pddc_sitor *f) { return stage_destroy(f); }

int pddc_sitor_reset(pddc_sitor *f) { return decoder_reset(f, kSitor); }

int pddc_sitor_set_rx(pddc_sitor *f, int rx, int modem, uint32_t flags) { return decoder_set_rx(f, kSitor, rx, modem, flags); }

int pddc_sitor_max_syms(const pddc_sitor *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)sitor_sym_bound(*f, n);
    return PDDC_OK;
}

int pddc_sitor_max_chars(const pddc_sitor *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)sitor_char_bound(*f, n);
    return PDDC_OK;
}

int pddc_sitor_process(pddc_sitor *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride, void *d_counts,
                       void *d_soft, size_t soft_stride, void *d_nsoft, void *stream)
{
    if (!f)
        return null_argument();
    PDDC_TRY(decoder_ptrs_ok(n, d_z, d_chars, d_counts));
    if (n)
        PDDC_TRY(device_ptr_ok(d_soft, 4, "d_soft", true));
    PDDC_TRY(device_ptr_ok(d_nsoft, 4, "d_nsoft", !n || !d_soft));
    if (over_capacity(n, z_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "sitor: %zu samples per receiver, z_stride %zu", n, z_stride);
    const uint64_t sbound = sitor_sym_bound(*f, n), bound = sitor_char_bound(*f, n);
    PDDC_TRY(decoder_sizes_ok(kSitor, n, z_stride, soft_stride, char_stride, bound));
    if (n && d_soft && soft_stride < sbound)
        return pddc_set_error_(PDDC_ECAPACITY, "sitor: room for %zu soft values per receiver, %zu samples can hold %llu", soft_stride, n,
                               (unsigned long long)sbound);
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n) {
        PDDC_TRY(decoder_zero_counts(d_counts, f->nrx, st));
        return decoder_zero_counts(d_nsoft, f->nrx, st);
    }
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    const bool soft_meets = d_soft && (ranges_overlap(d_z, zbytes, d_soft, rows_extent(f->nrx, (size_t)sbound, soft_stride, sizeof(float))) ||
                                       ranges_overlap(d_z, zbytes, d_nsoft, sizeof(uint32_t) * (size_t)f->nrx));
    PDDC_TRY(decoder_overlap_ok(kSitor, f->nrx, d_z, zbytes, soft_meets, d_chars, bound, char_stride, d_counts));
    PDDC_TRY(f->table.upload(st));
    SitorArgs a{};
    decoder_args(a, *f, d_z, n, z_stride, d_chars, char_stride, d_counts);
    a.soft = static_cast<float *>(d_soft);
    a.soft_stride = (long long)soft_stride;
    a.nsoft = d_soft ? static_cast<uint32_t *>(d_nsoft) : nullptr;
    PDDC_HIP_TRY(launch_sitor(a, st));
    decoder_accepted(f, kSitor, n);
    return PDDC_OK;
}

int pddc_sitor_read(pddc_sitor *f, pddc_sitor_status *host, void *stream)
{
    PDDC_TRY(decoder_read_back(f, host, stream));
    for (int j = 0; j < f->nrx; ++j) {
        uint32_t marks;
        const SitorState r = decoder_record(*f, kSitor, j, &marks);
        /* what the next batch will find: a pending restart clears the clock and the framing, another modem the framing */
        const bool reframed = marks != 0u, cleared = (marks & (kDecFresh | kDecClear)) != 0u;
        host[j] = pddc_sitor_status{ r.f.chars, r.f.symbols, r.f.errors, r.f.reframes, reframed ? 0u : r.f.locked,
                                     cleared ? 0u : r.acc, reframed ? 0u : r.f.reg, r.d_last };
    }
    return PDDC_OK;
}

} // extern "C"
