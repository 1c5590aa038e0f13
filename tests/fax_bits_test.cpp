/* tests/fax_bits_test.cpp -- the radiofax decoder's pixel clock, line structure and capacity arithmetic
 * (csrc/ddc_fax_bits.h: no HIP header, so a host compiler builds it alone): the closed form of the strobes against the
 * clock sample by sample for every class of inc (1, small, odd, powers of two, 2^31 - 1, 2^31) and acc; the strobes of
 * every window of n samples against fax_most_pixels, which the worst acc reaches; the product in two halves against
 * 128-bit arithmetic; fax_most_lines against lines counted pixel by pixel at widths 16 and 8192 from every column; the
 * modem test's bounds; the line rule on hand-made lines (hysteresis, classes, runs, need, saturation at 65535).
 * usage: fax_bits_test                                  -> prints "ok: <checks> checks", exit 0
 *        fax_bits_test width s_lo s_hi p_lo p_hi need file  -> the line rule over the file's bytes as pixels, pixel k
 *        strobed at sample 5 + 3 k: one "start crossings white flags run" per line, then "state col crossings white
 *        level run cls active lines pixels images"
 * The first failed check is printed, exit 1 */
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ddc_fax_bits.h"

using namespace pddc;

static long checks = 0;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        ++checks;                                                                                               \
        if (!(cond)) {                                                                                          \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                                                    \
            exit(1);                                                                                            \
        }                                                                                                       \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

static const uint32_t kIncs[] = { 1u, 2u, 3u, 65537u, 1u << 24, (1u << 24) + 1u, 1431655765u, 1592092837u, 1717986919u, (1u << 30), (1u << 31) - 1u, 1u << 31 };
static const uint32_t kAccs[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };

/* 256 samples of a tile: the closed form against the clock; -> the strobes */
static uint32_t tile_against_clock(uint32_t acc, uint32_t inc, uint32_t n)
{
    uint32_t a = acc, strobes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool strobe = fax_clock(a, inc);
        CHECK(strobe == (fax_carries(acc, inc, i + 1u) != fax_carries(acc, inc, i)));
        if (strobe)
            CHECK(fax_carries(acc, inc, i) == strobes);               /* the carries in front are the pixel's slot */
        strobes += strobe ? 1u : 0u;
    }
    CHECK(a == (uint32_t)((uint64_t)acc + (uint64_t)n * inc));
    CHECK(strobes == fax_carries(acc, inc, n) && strobes <= 128u);
    return strobes;
}

static void test_clock_and_pixels()
{
    for (uint32_t inc : kIncs) {
        for (uint32_t acc : kAccs)
            tile_against_clock(acc, inc, 256u);
        for (int r = 0; r < 50; ++r)
            tile_against_clock(rnd(), inc, 1u + rnd() % 256u);
        /* every n up to 600: the worst acc reaches the bound, no acc passes it */
        for (uint64_t n = 0; n <= 600; ++n) {
            const uint64_t bound = fax_most_pixels(n, inc);
            CHECK(bound == (n ? (((unsigned __int128)n * inc - 1u) >> 32) + 1u : 0u));
            CHECK((((uint64_t)0xFFFFFFFFu + n * inc) >> 32) == bound);
            for (int r = 0; r < 8; ++r)
                CHECK((((uint64_t)rnd() + n * inc) >> 32) <= bound);
        }
    }
    CHECK(tile_against_clock(0xFFFFFFFFu, 1u << 31, 256u) == 128u);
    /* the halves of the product, where it does not fit 64 bits */
    const uint64_t ns[] = { 1ull << 32, (1ull << 32) + 1u, (1ull << 40) - 1u, 1ull << 40, 0xFFFFFFFFull, 123456789012ull };
    for (uint64_t n : ns)
        for (uint32_t inc : kIncs)
            CHECK(fax_most_pixels(n, inc) == (uint64_t)((((unsigned __int128)n * inc - 1u) >> 32) + 1u));
    CHECK(fax_most_pixels(0u, 1u << 31) == 0u && fax_most_lines(0u, 16u) == 0u);
}

static FaxModem modem(uint32_t width)
{
    return FaxModem{ 1u << 30, width, 3u, 600.0f, 127.5f, 7, 9, 10, 14, 2u };
}

static void test_lines_bound()
{
    const uint32_t widths[] = { 16u, 8192u, 64u, 100u };
    for (uint32_t width : widths) {
        const FaxModem k = modem(width);
        for (uint32_t col0 : { 0u, 1u, width / 2u, width - 2u, width - 1u }) {
            FaxLine l{};
            l.col = col0;
            uint64_t lines = 0;
            FaxLineRec r;
            for (uint64_t p = 1; p <= 3u * width + 5u; ++p) {
                lines += fax_pixel(l, k, rnd() & 255u, p, &r) ? 1u : 0u;
                CHECK(lines <= fax_most_lines(p, width));
                if (col0 == width - 1u)
                    CHECK(lines == fax_most_lines(p, width));         /* the batch's first pixel is a line's last: the bound is met */
                CHECK(l.col < width);
            }
        }
    }
}

static void test_modem_ok()
{
    FaxModem k = modem(64u);
    CHECK(fax_modem_ok(k));
    for (uint32_t inc : { 0u, (1u << 31) + 1u, 0xFFFFFFFFu }) { FaxModem b = k; b.inc = inc; CHECK(!fax_modem_ok(b)); }
    for (uint32_t w : { 0u, 15u, 8193u }) { FaxModem b = k; b.width = w; CHECK(!fax_modem_ok(b)); }
    for (uint32_t w : { 16u, 8192u }) { FaxModem b = k; b.width = w; CHECK(fax_modem_ok(b)); }
    for (uint32_t x : { 0u, 17u }) { FaxModem b = k; b.box = x; CHECK(!fax_modem_ok(b)); }
    for (uint32_t x : { 0u, 256u }) { FaxModem b = k; b.need = x; CHECK(!fax_modem_ok(b)); }
    { FaxModem b = k; b.inc = 1u << 31; b.box = 16u; b.need = 255u; CHECK(fax_modem_ok(b)); }
    { FaxModem b = k; b.stop_lo = 9; CHECK(!fax_modem_ok(b)); }       /* the ranges share 9 */
    { FaxModem b = k; b.start_lo = 10; b.start_hi = 9; CHECK(!fax_modem_ok(b)); }
    { FaxModem b = k; b.start_lo = 15; b.start_hi = 20; CHECK(fax_modem_ok(b)); }   /* the start tone above the stop tone */
    { FaxModem b = k; b.start_lo = 12; b.start_hi = 20; CHECK(!fax_modem_ok(b)); }
    { FaxModem b = k; b.scale = 1.0f / 0.0f; CHECK(!fax_modem_ok(b)); }
    { FaxModem b = k; b.bias = 0.0f / 0.0f; CHECK(!fax_modem_ok(b)); }
}

/* a line of `width` pixels with `periods` periods of white and black; -> the record */
static FaxLineRec tone_line(FaxLine &l, const FaxModem &k, uint32_t periods, uint64_t m0)
{
    FaxLineRec r{};
    bool ended = false;
    for (uint32_t c = 0; c < k.width; ++c) {
        const uint32_t pixel = periods && (c * periods * 2u / k.width) % 2u == 0u ? 255u : 0u;
        ended = fax_pixel(l, k, pixel, m0 + c, &r);
        CHECK(ended == (c == k.width - 1u));
    }
    return r;
}

static void test_line_rule()
{
    const FaxModem k = modem(64u);
    FaxLine l{};
    FaxLineRec r = tone_line(l, k, 8u, 100u);
    CHECK(r.start == 100u && r.crossings == 8u && r.white == 32u && r.flags == kFaxStart && r.run == 1u && !l.active);
    r = tone_line(l, k, 8u, 200u);
    CHECK(r.flags == (kFaxStart | kFaxActive) && r.run == 2u && l.images == 1u && r.start == 200u);
    r = tone_line(l, k, 8u, 300u);
    CHECK(r.flags == (kFaxStart | kFaxActive) && r.run == 3u && l.images == 1u);   /* reaching need counts once */
    r = tone_line(l, k, 1u, 400u);
    CHECK(r.flags == kFaxActive && r.run == 0u && r.crossings == 1u);
    r = tone_line(l, k, 12u, 500u);
    CHECK(r.flags == (kFaxStop | kFaxActive) && r.run == 1u);
    r = tone_line(l, k, 0u, 600u);
    CHECK(r.flags == kFaxActive && r.run == 0u && r.white == 0u);    /* the run is broken */
    r = tone_line(l, k, 12u, 700u);
    CHECK(r.flags == (kFaxStop | kFaxActive) && r.run == 1u);
    r = tone_line(l, k, 12u, 800u);
    CHECK(r.flags == kFaxStop && r.run == 2u && !l.active && l.lines == 8u && l.pixels == 8u * 64u);
    /* the hysteresis: between 64 and 191 nothing moves; the level is carried over a line's end */
    FaxLine h{};
    const uint32_t seq[] = { 191u, 192u, 255u, 64u, 192u, 63u, 128u, 191u, 192u };
    uint32_t want_cross[] = { 0u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 2u };
    for (int i = 0; i < 9; ++i) {
        fax_pixel(h, k, seq[i], (uint64_t)i, &r);
        CHECK(h.crossings == want_cross[i]);
    }
    CHECK(h.white == 7u && h.level == 1u);
    for (uint32_t c = 9; c < 64u; ++c)
        fax_pixel(h, k, 255u, c, &r);
    CHECK(h.col == 0u && h.level == 1u && r.crossings == 2u);
    fax_pixel(h, k, 255u, 64u, &r);
    CHECK(h.crossings == 0u);                                         /* still high: no crossing */
    /* the run saturates */
    FaxLine s{};
    s.cls = kFaxStart;
    s.run = kFaxRunMost - 1u;
    r = tone_line(s, k, 8u, 0u);
    CHECK(r.run == 65535u);
    r = tone_line(s, k, 8u, 0u);
    CHECK(r.run == 65535u && s.run == kFaxRunMost);
    fax_line_restart(s, false);
    CHECK(s.run == 0u && s.cls == 0u && s.col == 0u && s.lines == 2u);
}

int main(int argc, char **argv)
{
    if (argc == 8) {
        FaxModem k = modem((uint32_t)atoi(argv[1]));
        k.start_lo = (uint16_t)atoi(argv[2]);
        k.start_hi = (uint16_t)atoi(argv[3]);
        k.stop_lo = (uint16_t)atoi(argv[4]);
        k.stop_hi = (uint16_t)atoi(argv[5]);
        k.need = (uint32_t)atoi(argv[6]);
        if (!fax_modem_ok(k))
            return 2;
        FILE *f = fopen(argv[7], "rb");
        if (!f)
            return 2;
        std::vector<unsigned char> px;
        for (int c; (c = fgetc(f)) != EOF;)
            px.push_back((unsigned char)c);
        fclose(f);
        FaxLine l{};
        FaxLineRec r;
        for (size_t i = 0; i < px.size(); ++i)
            if (fax_pixel(l, k, px[i], 5u + 3u * (uint64_t)i, &r))
                printf("%llu %u %u %u %u\n", (unsigned long long)r.start, r.crossings, r.white, r.flags, r.run);
        printf("state %u %u %u %u %u %u %u %u %u %u\n", l.col, l.crossings, l.white, l.level, l.run, l.cls, l.active, l.lines, l.pixels, l.images);
        return 0;
    }
    test_clock_and_pixels();
    test_lines_bound();
    test_modem_ok();
    test_line_rule();
    printf("ok: %ld checks\n", checks);
    return 0;
}
