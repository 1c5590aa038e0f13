/*
 * ddc_fax_bits.h -- the radiofax decoder's pixel clock, its line structure (include/perseus_ddc.h, "fax", step 5) and the
 * arithmetic of its two capacity bounds, written once in plain integers: k_fax (ddc_fax.hip) takes the clock's closed
 * form and the rule of a line's end from here, ddc_fax.cpp the bounds and the modem test, tests/fax_bits_test.cpp runs
 * all of it under sanitizers.
 * No HIP header: PDDC_FAX_HD is empty for a host compiler and __host__ __device__ under hipcc.
 *
 * The clock is free-running: nothing corrects acc, so the strobes of a stretch of samples are a closed form of the
 * sample index (fax_carries).  One pixel of the definition is fax_pixel; the kernel makes crossings and white of a
 * whole line from bit masks instead and calls fax_line_end, which fax_pixel calls too: one rule, two ways to it.
 */
#ifndef PDDC_DDC_FAX_BITS_H
#define PDDC_DDC_FAX_BITS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PDDC_FAX_HD __host__ __device__
#else
#define PDDC_FAX_HD
#endif

namespace pddc {

static constexpr uint32_t kFaxIncMost = 1u << 31;         /* a pixel is at least 2 samples                         */
static constexpr uint32_t kFaxWidthLeast = 16u, kFaxWidthMost = 8192u;
static constexpr uint32_t kFaxBoxMost = 16u;
static constexpr uint32_t kFaxHigh = 192u, kFaxLow = 64u, kFaxWhite = 128u;   /* the hysteresis levels and the white count's */
static constexpr uint32_t kFaxStart = 0x1, kFaxStop = 0x2, kFaxActive = 0x4;  /* FaxLineRec.flags                      */
static constexpr uint32_t kFaxRunMost = 65535u;

/* a modem behind its taps: the pixel phase per sample, the line's pixels, the boxcar, the grey map and the tones */
struct FaxModem {
    uint32_t inc, width, box;
    float scale, bias;
    uint16_t start_lo, start_hi, stop_lo, stop_hi;
    uint32_t need;
};

/* pddc_fax_line, 16 bytes */
struct FaxLineRec {
    uint64_t start;
    uint16_t crossings, white, flags, run;
};

/* what the line structure carries, and the counters */
struct FaxLine {
    uint64_t start;           /* sample of the strobe of the line's column 0                                       */
    uint32_t col;             /* pixels of the line in progress, 0 .. width - 1                                    */
    uint32_t crossings, white;
    uint32_t level;           /* the hysteresis: 1 high                                                            */
    uint32_t run, cls;        /* lines of the class `cls` (0, kFaxStart, kFaxStop) in a row                        */
    uint32_t active;
    uint32_t lines, pixels, images;              /* counters: never cleared by a restart                           */
};

PDDC_FAX_HD inline bool fax_modem_ok(const FaxModem &k)
{
    return k.inc >= 1u && k.inc <= kFaxIncMost && k.width >= kFaxWidthLeast && k.width <= kFaxWidthMost && k.box >= 1u &&
           k.box <= kFaxBoxMost && k.scale - k.scale == 0.0f && k.bias - k.bias == 0.0f && k.start_lo <= k.start_hi &&
           k.stop_lo <= k.stop_hi && (k.start_hi < k.stop_lo || k.stop_hi < k.start_lo) && k.need >= 1u && k.need <= 255u;
}

/* one sample of the clock; -> true on a strobe */
PDDC_FAX_HD inline bool fax_clock(uint32_t &acc, uint32_t inc)
{
    const uint32_t a2 = acc + inc;
    const bool strobe = a2 < acc;
    acc = a2;
    return strobe;
}

/* the strobes among the first i samples behind acc = a: i <= 2^32 / 2 keeps a + i inc inside 64 bits (the kernel has
 * i <= 256).  Sample i strobes iff fax_carries(a, inc, i + 1) != fax_carries(a, inc, i), and it is that pixel's slot */
PDDC_FAX_HD inline uint32_t fax_carries(uint32_t a, uint32_t inc, uint32_t i) { return (uint32_t)(((uint64_t)a + (uint64_t)i * inc) >> 32); }

/* the line structure as a restart or another modem leaves it; the level goes with a restart only; the counters stay */
PDDC_FAX_HD inline void fax_line_restart(FaxLine &l, bool level_too)
{
    l.start = 0;
    l.col = l.crossings = l.white = l.run = l.cls = l.active = 0u;
    if (level_too)
        l.level = 0u;
}

/* the end of a line whose start, crossings and white are in l: class, run, active, the record, the counters */
PDDC_FAX_HD inline void fax_line_end(FaxLine &l, const FaxModem &k, FaxLineRec *out)
{
    uint32_t cls = 0u;
    if (l.crossings >= k.start_lo && l.crossings <= k.start_hi)
        cls = kFaxStart;
    else if (l.crossings >= k.stop_lo && l.crossings <= k.stop_hi)
        cls = kFaxStop;
    if (!cls)
        l.run = 0u;
    else if (cls != l.cls)
        l.run = 1u;
    else
        l.run = l.run < kFaxRunMost ? l.run + 1u : kFaxRunMost;
    l.cls = cls;
    if (cls == kFaxStart && l.run == k.need) {
        l.active = 1u;
        ++l.images;
    }
    if (cls == kFaxStop && l.run == k.need)
        l.active = 0u;
    out->start = l.start;
    out->crossings = (uint16_t)l.crossings;
    out->white = (uint16_t)l.white;
    out->flags = (uint16_t)(cls | (l.active ? kFaxActive : 0u));
    out->run = (uint16_t)l.run;
    ++l.lines;
    l.col = l.crossings = l.white = 0u;
}

/* one pixel, strobed at sample m: step 5 of the definition; -> true if a line ended and went into *out */
PDDC_FAX_HD inline bool fax_pixel(FaxLine &l, const FaxModem &k, uint32_t pixel, uint64_t m, FaxLineRec *out)
{
    ++l.pixels;
    if (l.col == 0u)
        l.start = m;
    if (pixel >= kFaxHigh && !l.level) {
        l.level = 1u;
        ++l.crossings;
    }
    if (pixel < kFaxLow)
        l.level = 0u;
    if (pixel >= kFaxWhite)
        ++l.white;
    if (++l.col < k.width)
        return false;
    fax_line_end(l, k, out);
    return true;
}

/* The capacity bounds.  n samples behind acc = a hold floor((a + n inc) / 2^32) strobes, at most with a = 2^32 - 1:
 * ((n inc - 1) >> 32) + 1.  n <= 2^40 and inc <= 2^31: the product is taken in two halves.  A line ends on every
 * width-th pixel, and a batch's first pixel can be a line's last */
PDDC_FAX_HD inline uint64_t fax_most_pixels(uint64_t n, uint32_t inc_most)
{
    if (!n)
        return 0u;
    const uint64_t hi = (n >> 32) * inc_most, lo = (n & 0xFFFFFFFFu) * inc_most;
    return (lo ? hi + ((lo - 1u) >> 32) : hi - 1u) + 1u;
}
PDDC_FAX_HD inline uint64_t fax_most_lines(uint64_t pixels, uint32_t width_least) { return pixels ? (pixels - 1u) / width_least + 1u : 0u; }

} // namespace pddc
#endif
