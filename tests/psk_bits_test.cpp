/* tests/psk_bits_test.cpp -- the PSK decoder's symbol clock, framing and capacity arithmetic (csrc/ddc_psk_bits.h: no HIP
 * header, so a host compiler builds it alone) against the per-sample clock and vectors written out here: the jump to the
 * next strobe for random acc and inc, inc = 1 and inc = 2^29 included; both corrections at acc = 0 and acc = inc - 1;
 * idle zeros, "1 0 0", a run of 40 ones (LONG), nb's saturation; the modem test's bounds; the distance of two strobes
 * reached by a clock that is advanced every time, and the two bounds.
 * usage: psk_bits_test   -> prints "ok: <checks> checks", exit 0; the first failed check is printed, exit 1 */
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include "ddc_psk_bits.h"

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

/* the jump against the clock, sample by sample (at most `most` samples are walked) */
static void jump_against_clock(uint32_t acc, uint32_t inc, uint32_t most)
{
    const uint64_t k = psk_jump(acc, inc);
    CHECK(k >= 1u && k <= 1ull << 32);
    /* exact: the least k with acc + k inc >= 2^32 */
    CHECK((uint64_t)acc + k * inc >= (1ull << 32));
    CHECK((uint64_t)acc + (k - 1u) * inc < (1ull << 32));
    CHECK(psk_advance(acc, inc, (uint32_t)k) == (uint32_t)((uint64_t)acc + k * inc - (1ull << 32)));
    CHECK(psk_advance(acc, inc, (uint32_t)k) < inc);
    if (k > most)
        return;
    uint32_t a = acc;
    for (uint32_t i = 1; i <= (uint32_t)k; ++i) {
        const bool strobe = psk_clock(a, inc);
        CHECK(strobe == (i == k));
        CHECK(a == psk_advance(acc, inc, i));
    }
}

static void test_jump()
{
    const uint32_t incs[] = { 1u, 2u, 3u, 1u << 24, (1u << 24) + 1u, 268435456u, 268425483u, (1u << 29) - 1u, 1u << 29 };
    const uint32_t accs[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    for (uint32_t inc : incs)
        for (uint32_t acc : accs)
            jump_against_clock(acc, inc, 4096u);
    CHECK(psk_jump(0u, 1u) == 1ull << 32);                            /* the one jump that does not fit 32 bits */
    CHECK(psk_jump(1u, 1u) == 0xFFFFFFFFull);
    CHECK(psk_jump(0u, 1u << 29) == 8u);
    CHECK(psk_jump((1u << 29) - 1u, 1u << 29) == 8u && psk_jump(1u << 29, 1u << 29) == 7u);
    CHECK(psk_jump(0xFFFFFFFFu, 1u) == 1u && psk_jump(0xFFFFFFFFu, 1u << 29) == 1u);
    for (int i = 0; i < 20000; ++i) {
        uint32_t inc = rnd() >> (3 + rnd() % 24);
        inc = inc < 1u ? 1u : (inc > kPskIncMost ? kPskIncMost : inc);
        jump_against_clock(rnd(), inc, 2048u);
    }
    /* a whole run: strobes by jumps and by the clock are the same samples */
    for (uint32_t inc : { 1u << 29, 268425483u, 1u << 24, 300000000u }) {
        uint32_t a = 0u;
        uint64_t next = psk_jump(a, inc) - 1u, hits = 0;
        for (uint64_t m = 0; m < 20000; ++m) {
            const bool strobe = psk_clock(a, inc);
            CHECK(strobe == (m == next));
            if (strobe) {
                next = m + psk_jump(a, inc);
                ++hits;
            }
        }
        CHECK(hits == (20000ull * inc) >> 32);
    }
}

static void test_corrections()
{
    for (uint32_t inc : { 1u, 8u, 268425483u, 1u << 29 })
        for (uint32_t step : { 0u, 1u, inc / 16u, inc - 1u, inc }) {
            if (step > inc)
                continue;
            CHECK(psk_modem_ok(PskModem{ inc, 1u, step }));
            CHECK(psk_late(0u, step) == 0u);
            CHECK(psk_late(inc - 1u, step) == (inc - 1u >= step ? inc - 1u - step : 0u));
            CHECK(psk_early(0u, step) == step);
            CHECK(psk_early(inc - 1u, step) == inc - 1u + step);
            CHECK((uint64_t)(inc - 1u) + step < (1ull << 32));           /* no overflow */
            /* behind the early correction at its largest the next strobe is psk_distance samples away, never less */
            CHECK(psk_jump(psk_early(inc - 1u, step), inc) == psk_distance(PskModem{ inc, 1u, step }));
            CHECK(psk_jump(psk_late(0u, step), inc) == ((1ull << 32) + inc - 1u) / inc);
        }
    CHECK(psk_late(5u, 5u) == 0u && psk_late(5u, 6u) == 0u && psk_late(6u, 5u) == 1u);
}

static void test_modem_ok()
{
    CHECK(psk_modem_ok(PskModem{ 1u, 1u, 0u }) && psk_modem_ok(PskModem{ 1u, 64u, 1u }));
    CHECK(psk_modem_ok(PskModem{ 1u << 29, 1u, 1u << 29 }) && psk_modem_ok(PskModem{ 1u << 29, 2u, 0u }));
    CHECK(!psk_modem_ok(PskModem{ 0u, 1u, 0u }) && !psk_modem_ok(PskModem{ (1u << 29) + 1u, 1u, 0u }));
    CHECK(!psk_modem_ok(PskModem{ 1u << 29, 3u, 0u }));               /* 4 q inc > 2^32 */
    CHECK(psk_modem_ok(PskModem{ 1u << 24, 64u, 0u }) && !psk_modem_ok(PskModem{ (1u << 24) + 1u, 64u, 0u }));
    CHECK(!psk_modem_ok(PskModem{ 1u << 24, 0u, 0u }) && !psk_modem_ok(PskModem{ 1u << 24, 65u, 0u }));
    CHECK(!psk_modem_ok(PskModem{ 1u << 24, 1u, (1u << 24) + 1u }));
    CHECK(!psk_modem_ok(PskModem{ 0xFFFFFFFFu, 0xFFFFFFFFu, 0u }));    /* the product is taken in 64 bits */
}

struct Framer {
    PskFrame f{};
    PskChar rec[64];
    int n = 0;
    uint64_t c = 1000;
    void bit(uint32_t b, float ad = 0.5f)
    {
        PskChar ch;
        if (psk_frame(f, b, c, ad, &ch)) {
            CHECK(n < 64);
            rec[n++] = ch;
        }
        c += 16;
    }
};

static void test_framing()
{
    {   /* idle zeros emit nothing and leave nothing */
        Framer r;
        for (int i = 0; i < 1000; ++i)
            r.bit(0u);
        CHECK(r.n == 0 && r.f.reg == 0u && r.f.chars == 0u && r.f.nb == 0u);
    }
    {   /* 1 0 0: a space */
        Framer r;
        r.bit(0u, 0.9f);
        r.bit(1u, 0.8f);
        CHECK(r.f.reg == 1u && r.f.nb == 1u && r.f.start == 1016u);
        r.bit(0u, 0.25f);
        CHECK(r.n == 0 && r.f.reg == 2u);
        r.bit(0u, 0.75f);
        CHECK(r.n == 1 && r.rec[0].start == 1016u && r.rec[0].code == 1u && r.rec[0].nbits == 1u && r.rec[0].flags == 0u);
        CHECK(r.rec[0].quality == 0.25f && r.f.reg == 0u && r.f.chars == 1u);
        /* 1 0 1 1 0 0 behind it: "a" is 1011; the single 0 inside does not end it */
        for (uint32_t b : { 1u, 0u, 1u, 1u, 0u, 0u })
            r.bit(b);
        CHECK(r.n == 2 && r.rec[1].code == 0xBu && r.rec[1].nbits == 4u && r.rec[1].start == 1000u + 4u * 16u && r.f.chars == 2u);
        /* a NaN quality is skipped by the minimum, also as the first one */
        const float nan = __builtin_nanf("");
        r.bit(1u, nan);
        r.bit(0u, 0.5f);
        r.bit(0u, nan);
        CHECK(r.n == 3 && r.rec[2].quality == 0.5f);
    }
    {   /* 16 ones then 0 0: the longest code that is not LONG; 17: LONG, code holds the last 16 bits */
        for (int ones : { 16, 17, 40 }) {
            Framer r;
            for (int i = 0; i < ones; ++i)
                r.bit(1u);
            r.bit(0u);
            r.bit(0u);
            CHECK(r.n == 1 && r.rec[0].nbits == (uint8_t)ones && r.rec[0].code == 0xFFFFu);
            CHECK(r.rec[0].flags == (ones > 16 ? kPskLongFlag : 0u) && r.rec[0].start == 1000u);
        }
    }
    {   /* nb saturates at 255: 300 ones and 0 0 give nbits = 253, LONG; the register keeps shifting */
        Framer r;
        for (int i = 0; i < 300; ++i)
            r.bit(1u);
        CHECK(r.f.nb == 255u && r.f.reg == 0xFFFFFFFFu);
        r.bit(0u);
        r.bit(0u);
        CHECK(r.n == 1 && r.rec[0].nbits == 253u && r.rec[0].flags == kPskLongFlag && r.rec[0].code == 0xFFFFu && r.f.reg == 0u);
        /* 253 ones: nb = 255 without having saturated gives the same record */
        Framer s;
        for (int i = 0; i < 253; ++i)
            s.bit(1u);
        s.bit(0u);
        s.bit(0u);
        CHECK(s.n == 1 && s.rec[0].nbits == 253u);
    }
    {   /* restart: the framing goes, the counters stay */
        Framer r;
        for (uint32_t b : { 1u, 0u, 0u, 1u, 1u })
            r.bit(b);
        r.f.symbols = 5u;
        psk_frame_restart(r.f);
        CHECK(r.f.reg == 0u && r.f.nb == 0u && r.f.start == 0u && r.f.chars == 1u && r.f.symbols == 5u);
    }
}

static void test_bounds()
{
    CHECK(psk_distance(PskModem{ 1u << 29, 1u, 0u }) == 8u && psk_distance(PskModem{ 1u << 29, 1u, 1u << 29 }) == 7u);
    CHECK(psk_distance(PskModem{ 1u << 28, 4u, 1u << 24 }) == 15u && psk_distance(PskModem{ 268425483u, 4u, 0u }) == 16u);
    CHECK(psk_distance(PskModem{ 1u, 1u, 1u }) == 0xFFFFFFFFull && psk_distance(PskModem{ 1u, 1u, 0u }) == 1ull << 32);
    CHECK(psk_most(0, 7) == 0 && psk_most(1, 7) == 1 && psk_most(7, 7) == 1 && psk_most(8, 7) == 2 && psk_most(15, 7) == 3);
    CHECK(psk_most_chars(0) == 0 && psk_most_chars(1) == 1 && psk_most_chars(3) == 1 && psk_most_chars(4) == 2);
    CHECK(psk_most(~0ull, 1ull << 32) == (1ull << 32));
    /* a clock that is advanced by step behind every strobe: strobes are exactly psk_distance apart, and every window of
     * n samples holds at most psk_most(n, distance) of them -- exactly that many where step = inc, a power of two */
    for (const PskModem k : { PskModem{ 1u << 29, 1u, 1u << 29 }, PskModem{ 1u << 28, 4u, 1u << 28 }, PskModem{ 268425483u, 4u, 268425483u / 16u },
                              PskModem{ 300000000u, 1u, 12345u } }) {
        CHECK(psk_modem_ok(k));
        const uint64_t D = psk_distance(k);
        static bool hit[6000];
        uint32_t acc = 0u;
        uint64_t last = 0, hits = 0;
        for (uint64_t m = 0; m < 6000; ++m) {
            hit[m] = psk_clock(acc, k.inc);
            if (hit[m]) {
                if (hits)
                    CHECK(m - last >= D && m - last <= ((1ull << 32) + k.inc - 1u) / k.inc);
                last = m;
                ++hits;
                acc = psk_early(acc, k.step);
            }
        }
        for (uint64_t n : std::initializer_list<uint64_t>{ 1u, 2u, D - 1u, D, D + 1u, 2u * D, 2u * D + 1u, 255ull, 256ull, 257ull, 977ull }) {
            uint64_t most = 0, run = 0;
            for (uint64_t m = 0; m < 6000; ++m) {
                run += hit[m];
                if (m >= n)
                    run -= hit[m - n];
                if (m + 1u >= n && run > most)
                    most = run;
            }
            CHECK(most <= psk_most(n, D));
            if (k.step == k.inc && !(k.inc & (k.inc - 1u)))           /* every strobe exactly D behind the last: reached */
                CHECK(most == psk_most(n, D));
        }
    }
}

int main()
{
    test_jump();
    test_corrections();
    test_modem_ok();
    test_framing();
    test_bounds();
    printf("ok: %ld checks\n", checks);
    return 0;
}
