/* tests/mfsk_bits_test.cpp -- the MFSK decoder's symbol clock and capacity arithmetic (csrc/ddc_mfsk_bits.h: no HIP header,
 * so a host compiler builds it alone) against the per-sample clock and vectors written out here: the jump to the next wrap
 * for random acc and inc, inc = 1 and inc = 2^29 included; both corrections at acc = 0 and acc = inc - 1, the late one's
 * borrowed wrap against the phase kept in 64 signed bits; the modem test's bounds; the distance of two strobes reached by
 * a clock that is advanced every time, never undercut by one that is delayed, and the bound; the slot arithmetic.
 * usage: mfsk_bits_test   -> prints "ok: <checks> checks", exit 0; the first failed check is printed, exit 1 */
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include "ddc_mfsk_bits.h"

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
    const uint64_t k = mfsk_jump(acc, inc);
    CHECK(k >= 1u && k <= 1ull << 32);
    CHECK((uint64_t)acc + k * inc >= (1ull << 32));
    CHECK((uint64_t)acc + (k - 1u) * inc < (1ull << 32));
    CHECK(mfsk_advance(acc, inc, (uint32_t)k) == (uint32_t)((uint64_t)acc + k * inc - (1ull << 32)));
    CHECK(mfsk_advance(acc, inc, (uint32_t)k) < inc);
    if (k > most)
        return;
    for (uint32_t skip0 : { 0u, 1u }) {
        uint32_t a = acc, skip = skip0;
        for (uint32_t i = 1; i <= (uint32_t)k; ++i) {
            const bool strobe = mfsk_clock(a, skip, inc);
            CHECK(strobe == (i == k && !skip0));
            CHECK(a == mfsk_advance(acc, inc, i));
            CHECK(skip == (i == k ? 0u : skip0));
        }
    }
}

static void test_jump()
{
    const uint32_t incs[] = { 1u, 2u, 3u, 1u << 24, (1u << 24) + 1u, 268435456u, 268425483u, 54975581u, (1u << 29) - 1u, 1u << 29 };
    const uint32_t accs[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    for (uint32_t inc : incs)
        for (uint32_t acc : accs)
            jump_against_clock(acc, inc, 4096u);
    CHECK(mfsk_jump(0u, 1u) == 1ull << 32);                           /* the one jump that does not fit 32 bits */
    CHECK(mfsk_jump(0u, 1u << 29) == 8u && mfsk_jump(1u << 29, 1u << 29) == 7u);
    CHECK(mfsk_jump(0xFFFFFFFFu, 1u) == 1u && mfsk_jump(0xFFFFFFFFu, 1u << 29) == 1u);
    for (int i = 0; i < 20000; ++i) {
        uint32_t inc = rnd() >> (3 + rnd() % 24);
        inc = inc < 1u ? 1u : (inc > kMfskIncMost ? kMfskIncMost : inc);
        jump_against_clock(rnd(), inc, 2048u);
    }
}

/* A clock corrected at random behind every strobe, by the header's (acc, skip) and by a phase kept in 64 signed bits whose
 * strobes are the crossings of multiples of 2^32 that follow a non-negative phase: the same samples; two strobes are at
 * least mfsk_distance apart, and every window of n samples holds at most mfsk_most of them */
static void test_corrected_clock()
{
    for (const MfskModem k : { MfskModem{ 8u, 1u << 29, 1u, 1u << 29 }, MfskModem{ 8u, 1u << 29, 2u, 1u << 26 }, MfskModem{ 2u, 1u << 28, 4u, 1u << 28 },
                               MfskModem{ 8u, 54975581u, 19u, 54975581u / 2u }, MfskModem{ 32u, 268425483u, 4u, 268425483u / 64u },
                               MfskModem{ 3u, 300000000u, 1u, 12345u }, MfskModem{ 8u, 1u << 29, 1u, 0u } }) {
        CHECK(mfsk_modem_ok(k));
        const uint64_t D = mfsk_distance(k);
        for (int mode = 0; mode < 3; ++mode) {                        /* random, always early, always late */
            static bool hit[6000];
            uint32_t acc = 0u, skip = 0u;
            int64_t phase = 0;                                        /* the same clock without the borrow: may go below 0 */
            uint64_t last = 0, hits = 0;
            for (uint64_t m = 0; m < 6000; ++m) {
                const int64_t before = phase;
                phase += k.inc;
                const bool want = before >= 0 && phase >= (int64_t)(1ull << 32);
                if (phase >= (int64_t)(1ull << 32))
                    phase -= (int64_t)(1ull << 32);
                hit[m] = mfsk_clock(acc, skip, k.inc);
                CHECK(hit[m] == want);
                CHECK(acc == (uint32_t)(uint64_t)phase);
                if (!hit[m])
                    continue;
                CHECK(acc < k.inc && skip == 0u);
                if (hits)
                    CHECK(m - last >= D);
                last = m;
                ++hits;
                const uint32_t pick = mode == 0 ? rnd() % 3u : (uint32_t)mode;
                if (pick == 1u) {
                    acc = mfsk_early(acc, k.step);
                    phase += k.step;
                    CHECK((uint64_t)acc == (uint64_t)phase);          /* no overflow */
                } else if (pick == 2u) {
                    const uint32_t was = acc;
                    acc = mfsk_late(acc, skip, k.step);
                    phase -= k.step;
                    CHECK(skip == (was < k.step ? 1u : 0u));
                    CHECK(acc == (uint32_t)(uint64_t)phase);
                    CHECK(phase + (int64_t)k.inc >= 0);               /* one sample brings it back */
                }
            }
            CHECK(hits >= 6000u / (((1ull << 32) + k.inc - 1u) / k.inc + 1u) - 1u);
            for (uint64_t n : std::initializer_list<uint64_t>{ 1u, 2u, D - 1u, D, D + 1u, 2u * D, 2u * D + 1u, 255ull, 256ull, 257ull, 977ull }) {
                uint64_t most = 0, run = 0;
                for (uint64_t m = 0; m < 6000; ++m) {
                    run += hit[m];
                    if (m >= n)
                        run -= hit[m - n];
                    if (m + 1u >= n && run > most)
                        most = run;
                }
                CHECK(most <= mfsk_most(n, D));
                if (mode == 1 && k.step == k.inc && !(k.inc & (k.inc - 1u)))  /* every strobe exactly D behind the last: reached */
                    CHECK(most == mfsk_most(n, D));
            }
        }
    }
    uint32_t skip = 0u;
    CHECK(mfsk_late(5u, skip, 5u) == 0u && skip == 0u);
    CHECK(mfsk_late(6u, skip, 5u) == 1u && skip == 0u);
    CHECK(mfsk_late(5u, skip, 6u) == 0xFFFFFFFFu && skip == 1u);
    skip = 0u;
    CHECK(mfsk_late(0u, skip, 0u) == 0u && skip == 0u);               /* a fixed clock never borrows */
    CHECK(mfsk_early(0u, 7u) == 7u && mfsk_early((1u << 29) - 1u, 1u << 29) == 0x3FFFFFFFu);
}

static void test_modem_ok()
{
    CHECK(mfsk_modem_ok(MfskModem{ 2u, 1u, 1u, 0u }) && mfsk_modem_ok(MfskModem{ 32u, 1u, 64u, 1u }));
    CHECK(!mfsk_modem_ok(MfskModem{ 1u, 1u, 1u, 0u }) && !mfsk_modem_ok(MfskModem{ 33u, 1u, 1u, 0u }) && !mfsk_modem_ok(MfskModem{ 0u, 1u, 1u, 0u }));
    CHECK(mfsk_modem_ok(MfskModem{ 8u, 1u << 29, 1u, 1u << 29 }) && mfsk_modem_ok(MfskModem{ 8u, 1u << 29, 2u, 0u }));
    CHECK(!mfsk_modem_ok(MfskModem{ 8u, 0u, 1u, 0u }) && !mfsk_modem_ok(MfskModem{ 8u, (1u << 29) + 1u, 1u, 0u }));
    CHECK(!mfsk_modem_ok(MfskModem{ 8u, 1u << 29, 3u, 0u }));           /* 4 q inc > 2^32 */
    CHECK(mfsk_modem_ok(MfskModem{ 8u, 1u << 24, 64u, 0u }) && !mfsk_modem_ok(MfskModem{ 8u, (1u << 24) + 1u, 64u, 0u }));
    CHECK(!mfsk_modem_ok(MfskModem{ 8u, 1u << 24, 0u, 0u }) && !mfsk_modem_ok(MfskModem{ 8u, 1u << 24, 65u, 0u }));
    CHECK(!mfsk_modem_ok(MfskModem{ 8u, 1u << 24, 1u, (1u << 24) + 1u }));
    CHECK(!mfsk_modem_ok(MfskModem{ 8u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u })); /* the product is taken in 64 bits */
    CHECK(mfsk_modem_ok(MfskModem{ 8u, 54975581u, 19u, 0u }) && !mfsk_modem_ok(MfskModem{ 8u, 54975581u, 20u, 0u }));   /* 2G ALE at 9765.625 Hz */
}

static void test_bounds_and_slots()
{
    CHECK(mfsk_distance(MfskModem{ 8u, 1u << 29, 1u, 0u }) == 8u && mfsk_distance(MfskModem{ 8u, 1u << 29, 1u, 1u << 29 }) == 7u);
    CHECK(mfsk_distance(MfskModem{ 8u, 1u << 28, 4u, 1u << 24 }) == 15u && mfsk_distance(MfskModem{ 8u, 268425483u, 4u, 0u }) == 16u);
    CHECK(mfsk_distance(MfskModem{ 8u, 1u, 1u, 1u }) == 0xFFFFFFFFull && mfsk_distance(MfskModem{ 8u, 1u, 1u, 0u }) == 1ull << 32);
    CHECK(mfsk_most(0, 7) == 0 && mfsk_most(1, 7) == 1 && mfsk_most(7, 7) == 1 && mfsk_most(8, 7) == 2 && mfsk_most(15, 7) == 3);
    CHECK(mfsk_most(~0ull, 1ull << 32) == (1ull << 32));
    CHECK(mfsk_pairs(2u) == 1u && mfsk_pairs(3u) == 2u && mfsk_pairs(31u) == 16u && mfsk_pairs(32u) == 16u && kMfskPairsMost == 16u);
    CHECK(kMfskBack == 128u && mfsk_hist_slots(1) == 160 && mfsk_hist_slots(256) == 255 + 160);
    CHECK(mfsk_pair_floats(8) == 32 && mfsk_modem_floats(256) == 16 * 1024);
}

int main()
{
    test_jump();
    test_corrected_clock();
    test_modem_ok();
    test_bounds_and_slots();
    printf("ok: %ld checks\n", checks);
    return 0;
}
