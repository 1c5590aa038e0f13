/*
 * ddc_mfsk.cpp -- host side of the MFSK decoder (include/perseus_ddc.h, pddc_mfsk_*) on ddc_decoder.h: its modem bank, the
 * capacity bound, its best output, the launch of a batch and the status read.  The kernel is in ddc_mfsk.hip, the clock
 * and the bound's arithmetic in ddc_mfsk_bits.h.  The skeleton's "characters" are this decoder's symbol records.
 * Carried per receiver: its last W - 1 inputs, (a, second, b, r) of its last 128 samples, the clock and the counter.
 */
#include "ddc_decoder.h"
#include "ddc_mfsk.h"

using namespace pddc;

struct pddc_mfsk : DecoderBase<MfskState, MfskModem> {
    PDDC_LOCAL ~pddc_mfsk() = default;
};

static_assert(PDDC_MFSK_ON == kDecOn && PDDC_MFSK_REVERSE == kMfskReverse && !(PDDC_MFSK_RESTART & (kDecOn | kMfskReverse | kMfskMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_MFSK_MAX_TONES == kMfskTonesMost, "the taps' tone rows are the header's");
static_assert(sizeof(pddc_mfsk_sym) == 16 && sizeof(MfskSym) == 16 && offsetof(pddc_mfsk_sym, tone) == offsetof(MfskSym, tone) &&
                  offsetof(pddc_mfsk_sym, second) == offsetof(MfskSym, second) && offsetof(pddc_mfsk_sym, flags) == offsetof(MfskSym, flags) &&
                  offsetof(pddc_mfsk_sym, quality) == offsetof(MfskSym, quality),
              "the kernel's symbol record is the header's");
static_assert(sizeof(pddc_mfsk_modem) == sizeof(MfskModem) && offsetof(pddc_mfsk_modem, step) == offsetof(MfskModem, step),
              "the clock's modem is the header's");

/* RESTART, OFF -> ON, another modem: the carried inputs and results and the clock start afresh */
static constexpr DecoderKind kMfsk{ "mfsk", "modem", 2 * (int)kMfskTonesMost, kDecOn | kMfskReverse, PDDC_MFSK_RESTART, kMfskMarks, kDecClear };

static uint64_t mfsk_bound(const pddc_mfsk &f, uint64_t n) { return mfsk_most(n, f.distance); }

extern "C" {

int pddc_mfsk_tile_outputs(void) { return kDecTile; }

int pddc_mfsk_create(pddc_mfsk **out, int device, int nrx, int window, int nmodems, const float *taps, const pddc_mfsk_modem *modems,
                     const pddc_mfsk_rx *rx)
{
    PDDC_TRY(decoder_create_ok(kMfsk, out, nrx, rx, window, nmodems));
    if (!taps || !modems)
        return pddc_set_error_(PDDC_EINVAL, "mfsk: null taps or modems");
    PDDC_TRY(decoder_taps_ok(kMfsk, taps, nmodems, kMfsk.coef * window));
    for (int b = 0; b < nmodems; ++b)
        if (!mfsk_modem_ok(MfskModem{ modems[b].ntones, modems[b].inc, modems[b].q, modems[b].step }))
            return pddc_set_error_(PDDC_EINVAL,
                                   "mfsk: modem %d: 2 <= ntones %u <= 32, 1 <= inc %u <= 2^29, 1 <= q %u <= 64 with 4 q inc <= 2^32, step %u <= inc",
                                   b, modems[b].ntones, modems[b].inc, modems[b].q, modems[b].step);
    PDDC_TRY(decoder_rx_ok(kMfsk, rx, &pddc_mfsk_rx::modem, nrx, nmodems));
    return stage_create(out, device, nrx, [&](pddc_mfsk &f) {
        for (int b = 0; b < nmodems; ++b)
            f.bank.push_back(MfskModem{ modems[b].ntones, modems[b].inc, modems[b].q, modems[b].step });
        f.distance = decoder_distance(f.bank, mfsk_distance);
        /* taps[b][k][t] (re, im) -> per pair p and tap t (h_2p.re, h_2p.im, h_2p+1.re, h_2p+1.im), a pair's row of
         * dec_row(W) taps with zeros behind the W-th; a tone at or above the modem's M is a zero tone whatever the caller gave */
        const size_t Wz = (size_t)window, R = (size_t)dec_row(window);
        std::vector<float> rows((size_t)nmodems * (size_t)mfsk_modem_floats((int)R), 0.0f);
        for (size_t b = 0; b < (size_t)nmodems; ++b)
            for (size_t k = 0; k < f.bank[b].ntones; ++k)
                for (size_t t = 0; t < Wz; ++t)
                    for (size_t c = 0; c < 2; ++c)
                        rows[b * (size_t)mfsk_modem_floats((int)R) + (k / 2) * (size_t)mfsk_pair_floats((int)R) + 4 * t + 2 * (k % 2) + c] =
                            taps[((b * kMfskTonesMost + k) * Wz + t) * 2 + c];
        return decoder_fill(f, kMfsk, window, rows, rx, &pddc_mfsk_rx::modem, (size_t)mfsk_hist_slots(window));
    });
}

int pddc_mfsk_destroy(pddc_mfsk *f) { return stage_destroy(f); }

int pddc_mfsk_reset(pddc_mfsk *f) { return decoder_reset(f, kMfsk); }

int pddc_mfsk_set_rx(pddc_mfsk *f, int rx, int modem, uint32_t flags) { return decoder_set_rx(f, kMfsk, rx, modem, flags); }

int pddc_mfsk_max_syms(const pddc_mfsk *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)mfsk_bound(*f, n);
    return PDDC_OK;
}

int pddc_mfsk_process(pddc_mfsk *f, const void *d_z, size_t n, size_t z_stride, void *d_syms, size_t sym_stride, void *d_counts,
                      void *d_best, size_t best_stride, void *stream)
{
    if (!f)
        return null_argument();
    PDDC_TRY(decoder_ptrs_ok(n, d_z, d_syms, d_counts));
    PDDC_TRY(device_ptr_ok(d_best, 4, "d_best", true));
    if (over_capacity(n, z_stride) || (d_best && over_capacity(n, best_stride)))
        return pddc_set_error_(PDDC_ECAPACITY, "mfsk: %zu samples per receiver, z_stride %zu, best_stride %zu", n, z_stride, best_stride);
    const uint64_t bound = mfsk_bound(*f, n);
    PDDC_TRY(decoder_sizes_ok(kMfsk, n, z_stride, best_stride, sym_stride, bound));
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n)
        return decoder_zero_counts(d_counts, f->nrx, st);
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    const bool best_meets = d_best && ranges_overlap(d_z, zbytes, d_best, rows_extent(f->nrx, n, best_stride, sizeof(float)));
    PDDC_TRY(decoder_overlap_ok(kMfsk, f->nrx, d_z, zbytes, best_meets, d_syms, bound, sym_stride, d_counts));
    PDDC_TRY(f->table.upload(st));
    MfskArgs a{};
    decoder_args(a, *f, d_z, n, z_stride, d_syms, sym_stride, d_counts);
    a.best = static_cast<float *>(d_best);
    a.best_stride = (long long)best_stride;
    PDDC_HIP_TRY(launch_mfsk(a, st));
    decoder_accepted(f, kMfsk, n);
    return PDDC_OK;
}

int pddc_mfsk_read(pddc_mfsk *f, pddc_mfsk_status *host, void *stream)
{
    PDDC_TRY(decoder_read_back(f, host, stream));
    for (int j = 0; j < f->nrx; ++j) {
        uint32_t marks;
        const MfskState r = decoder_record(*f, kMfsk, j, &marks);
        const bool afresh = !f->launched || marks;
        host[j] = pddc_mfsk_status{ r.symbols, afresh ? 0u : r.acc, afresh ? 0u : r.skip, afresh ? 0u : r.tone_last,
                                    afresh ? 0.0f : r.q_last };
    }
    return PDDC_OK;
}

} // extern "C"
