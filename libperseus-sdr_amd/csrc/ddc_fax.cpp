/*
 * ddc_fax.cpp -- host side of the radiofax decoder (include/perseus_ddc.h, pddc_fax_*) on ddc_decoder.h: its modem bank,
 * the two capacity bounds, its pixel and disc outputs, the launch of a batch and the status read.  The kernel is in
 * ddc_fax.hip, the clock, the line structure and the bounds' arithmetic in ddc_fax_bits.h.
 * The skeleton's `chars` are this decoder's lines: records of 16 bytes, at most pddc_fax_max_lines a batch.
 * Carried per receiver: its last W - 1 inputs, the filter's last output, the last 16 discriminator values, the clock,
 * the line in progress, the run and the counters.
 */
#include "ddc_decoder.h"
#include "ddc_fax.h"

using namespace pddc;

struct pddc_fax : DecoderBase<FaxState, FaxModem> {
    uint32_t inc_most = 0, width_least = 0;       /* over the bank: what the bounds are made of                  */
    PDDC_LOCAL ~pddc_fax() = default;
};

static_assert(PDDC_FAX_ON == kDecOn && PDDC_FAX_REVERSE == kFaxReverse && !(PDDC_FAX_RESTART & (kDecOn | kFaxReverse | kFaxMarks)),
              "the kernel's flag bits are the header's");
static_assert(PDDC_FAX_START == kFaxStart && PDDC_FAX_STOP == kFaxStop && PDDC_FAX_ACTIVE == kFaxActive,
              "the line record's flags are the header's");
static_assert(sizeof(pddc_fax_line) == 16 && sizeof(FaxLineRec) == 16 && offsetof(pddc_fax_line, crossings) == offsetof(FaxLineRec, crossings) &&
                  offsetof(pddc_fax_line, white) == offsetof(FaxLineRec, white) && offsetof(pddc_fax_line, flags) == offsetof(FaxLineRec, flags) &&
                  offsetof(pddc_fax_line, run) == offsetof(FaxLineRec, run),
              "the kernel's line record is the header's");
static_assert(sizeof(pddc_fax_modem) == sizeof(FaxModem) && offsetof(pddc_fax_modem, box) == offsetof(FaxModem, box) &&
                  offsetof(pddc_fax_modem, bias) == offsetof(FaxModem, bias) && offsetof(pddc_fax_modem, stop_hi) == offsetof(FaxModem, stop_hi) &&
                  offsetof(pddc_fax_modem, need) == offsetof(FaxModem, need),
              "the kernel's modem is the header's");

/* another modem: the inputs, y, f, the clock and the level stay, the line structure starts afresh */
static constexpr DecoderKind kFax{ "fax", "modem", 1, kDecOn | kFaxReverse, PDDC_FAX_RESTART, kFaxMarks, kFaxReline };

static FaxModem fax_modem_of(const pddc_fax_modem &m)
{
    return FaxModem{ m.inc, m.width, m.box, m.scale, m.bias, m.start_lo, m.start_hi, m.stop_lo, m.stop_hi, m.need };
}

static uint64_t fax_pixel_bound(const pddc_fax &f, uint64_t n) { return fax_most_pixels(n, f.inc_most); }
static uint64_t fax_line_bound(const pddc_fax &f, uint64_t n) { return fax_most_lines(fax_pixel_bound(f, n), f.width_least); }

extern "C" {

int pddc_fax_tile_outputs(void) { return kDecTile; }

int pddc_fax_create(pddc_fax **out, int device, int nrx, int window, int nmodems, const float *taps, const pddc_fax_modem *modems,
                    const pddc_fax_rx *rx)
{
    PDDC_TRY(decoder_create_ok(kFax, out, nrx, rx, window, nmodems));
    if (!taps || !modems)
        return pddc_set_error_(PDDC_EINVAL, "fax: null taps or modems");
    PDDC_TRY(decoder_taps_ok(kFax, taps, nmodems, window));
    for (int b = 0; b < nmodems; ++b)
        if (!fax_modem_ok(fax_modem_of(modems[b])))
            return pddc_set_error_(PDDC_EINVAL,
                                   "fax: modem %d: 1 <= inc %u <= 2^31, width %u (16 .. 8192), box %u (1 .. 16), finite scale and bias, "
                                   "start %u .. %u and stop %u .. %u apart, need %u (1 .. 255)",
                                   b, modems[b].inc, modems[b].width, modems[b].box, modems[b].start_lo, modems[b].start_hi,
                                   modems[b].stop_lo, modems[b].stop_hi, modems[b].need);
    PDDC_TRY(decoder_rx_ok(kFax, rx, &pddc_fax_rx::modem, nrx, nmodems));
    return stage_create(out, device, nrx, [&](pddc_fax &f) {
        f.width_least = kFaxWidthMost;
        for (int b = 0; b < nmodems; ++b) {
            f.bank.push_back(fax_modem_of(modems[b]));
            f.inc_most = modems[b].inc > f.inc_most ? modems[b].inc : f.inc_most;
            f.width_least = modems[b].width < f.width_least ? modems[b].width : f.width_least;
        }
        return decoder_fill(f, kFax, window, decoder_rows(kFax, nmodems, window, taps), rx, &pddc_fax_rx::modem,
                            (size_t)(window > 1 ? window - 1 : 1));
    });
}

int pddc_fax_destroy(pddc_fax *f) { return stage_destroy(f); }

int pddc_fax_reset(pddc_fax *f) { return decoder_reset(f, kFax); }

int pddc_fax_set_rx(pddc_fax *f, int rx, int modem, uint32_t flags) { return decoder_set_rx(f, kFax, rx, modem, flags); }

int pddc_fax_max_pixels(const pddc_fax *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)fax_pixel_bound(*f, n);
    return PDDC_OK;
}

int pddc_fax_max_lines(const pddc_fax *f, size_t n, size_t *count)
{
    if (!f || !count)
        return null_argument();
    *count = (size_t)fax_line_bound(*f, n);
    return PDDC_OK;
}

int pddc_fax_process(pddc_fax *f, const void *d_z, size_t n, size_t z_stride, void *d_pix, size_t pix_stride, void *d_npix, void *d_lines,
                     size_t line_stride, void *d_counts, void *d_disc, size_t disc_stride, void *stream)
{
    if (!f)
        return null_argument();
    PDDC_TRY(decoder_ptrs_ok(n, d_z, d_lines, d_counts));
    PDDC_TRY(device_ptr_ok(d_npix, 4, "d_npix", !n));
    if (n) {
        PDDC_TRY(device_ptr_ok(d_pix, 1, "d_pix"));
        PDDC_TRY(device_ptr_ok(d_disc, 4, "d_disc", true));
    }
    if (over_capacity(n, z_stride) || (n && d_disc && over_capacity(n, disc_stride)))
        return pddc_set_error_(PDDC_ECAPACITY, "fax: %zu samples per receiver, z_stride %zu, disc_stride %zu", n, z_stride, disc_stride);
    const uint64_t pbound = fax_pixel_bound(*f, n), bound = fax_line_bound(*f, n);
    PDDC_TRY(decoder_sizes_ok(kFax, n, z_stride, pix_stride > disc_stride ? pix_stride : disc_stride, line_stride, bound));
    if (n && pix_stride < pbound)
        return pddc_set_error_(PDDC_ECAPACITY, "fax: room for %zu pixels per receiver, %zu samples can hold %llu", pix_stride, n,
                               (unsigned long long)pbound);
    PDDC_TRY(set_device(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (!n) {
        PDDC_TRY(decoder_zero_counts(d_counts, f->nrx, st));
        return decoder_zero_counts(d_npix, f->nrx, st);
    }
    const size_t zbytes = rows_extent(f->nrx, n, z_stride, sizeof(float2));
    const bool meets = ranges_overlap(d_z, zbytes, d_pix, rows_extent(f->nrx, (size_t)pbound, pix_stride, 1)) ||
                       ranges_overlap(d_z, zbytes, d_npix, sizeof(uint32_t) * (size_t)f->nrx) ||
                       (d_disc && ranges_overlap(d_z, zbytes, d_disc, rows_extent(f->nrx, n, disc_stride, sizeof(float))));
    PDDC_TRY(decoder_overlap_ok(kFax, f->nrx, d_z, zbytes, meets, d_lines, bound, line_stride, d_counts));
    PDDC_TRY(f->table.upload(st));
    FaxArgs a{};
    decoder_args(a, *f, d_z, n, z_stride, d_lines, line_stride, d_counts);
    a.pix = static_cast<uint8_t *>(d_pix);
    a.pix_stride = (long long)pix_stride;
    a.npix = static_cast<uint32_t *>(d_npix);
    a.disc = static_cast<float *>(d_disc);
    a.disc_stride = (long long)disc_stride;
    PDDC_HIP_TRY(launch_fax(a, st));
    decoder_accepted(f, kFax, n);
    return PDDC_OK;
}

int pddc_fax_read(pddc_fax *f, pddc_fax_status *host, void *stream)
{
    PDDC_TRY(decoder_read_back(f, host, stream));
    for (int j = 0; j < f->nrx; ++j) {
        uint32_t marks;
        const FaxState r = decoder_record(*f, kFax, j, &marks);
        /* what the next batch will find: a pending restart clears the clock, f and the line, another modem the line */
        const bool relined = marks != 0u, cleared = (marks & (kDecFresh | kDecClear)) != 0u;
        host[j] = pddc_fax_status{ r.l.lines, r.l.pixels, r.l.images, relined ? 0u : r.l.active, cleared ? 0u : r.acc,
                                   relined ? 0u : r.l.col, cleared ? 0.0f : r.f[kFaxBack - 1] };
    }
    return PDDC_OK;
}

} // extern "C"
