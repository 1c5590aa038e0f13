/* tests/sitor_bits_test.cpp -- the SITOR decoder's bit clock, framing and capacity arithmetic (csrc/ddc_sitor_bits.h: no
 * HIP header, so a host compiler builds it alone) against the per-sample clock and bit series written out here: the jump
 * to the next strobe for random acc and inc, inc = 1 and inc = 2^29 included; both corrections at the edges of their
 * ranges; rules a - c on hand-made bit series (phasing at each of the 7 bit phases, an all-valid wrong phase that rule b
 * reframes, unlock after `unlock` bad characters, relock needing 7 lock fresh bits, lock = 0); the modem test's bounds;
 * both capacity bounds against every window of an adversarial series whose decision alternates at every sample of a
 * bit's first half.
 * usage: sitor_bits_test   -> prints "ok: <checks> checks, least strobe distance <d> against the bound <D>", exit 0; the
 * first failed check is printed, exit 1 */
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ddc_sitor_bits.h"

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
    const uint64_t k = sitor_jump(acc, inc);
    CHECK(k >= 1u && k <= 1ull << 32);
    CHECK((uint64_t)acc + k * inc >= (1ull << 32));
    CHECK((uint64_t)acc + (k - 1u) * inc < (1ull << 32));
    CHECK(sitor_advance(acc, inc, (uint32_t)k) == (uint32_t)((uint64_t)acc + k * inc - (1ull << 32)));
    CHECK(sitor_advance(acc, inc, (uint32_t)k) < inc);
    if (k > most)
        return;
    uint32_t a = acc;
    for (uint32_t i = 1; i <= (uint32_t)k; ++i) {
        const bool strobe = sitor_clock(a, inc);
        CHECK(strobe == (i == k));
        CHECK(a == sitor_advance(acc, inc, i));
    }
}

static void test_jump()
{
    const uint32_t incs[] = { 1u, 2u, 3u, 1u << 24, (1u << 24) + 1u, 268435456u, 268354925u, (1u << 29) - 161061u, (1u << 29) - 1u, 1u << 29 };
    const uint32_t accs[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    for (uint32_t inc : incs)
        for (uint32_t acc : accs)
            jump_against_clock(acc, inc, 4096u);
    CHECK(sitor_jump(0u, 1u) == 1ull << 32);                          /* the one jump that does not fit 32 bits */
    CHECK(sitor_jump(1u, 1u) == 0xFFFFFFFFull);
    CHECK(sitor_jump(0u, 1u << 29) == 8u);
    CHECK(sitor_jump(0xFFFFFFFFu, 1u) == 1u);
    for (int i = 0; i < 20000; ++i) {
        const uint32_t inc = 1u + rnd() % (1u << 29), acc = rnd();
        jump_against_clock(acc, inc, 64u);
    }
}

static void test_corrections()
{
    /* below 2^31 the clock is advanced, from 2^31 on it is held back; neither wraps for step <= inc <= 2^29 */
    const uint32_t most = kSitorIncMost;
    CHECK(sitor_correct(0u, 0u) == 0u);
    CHECK(sitor_correct(0u, most) == most);
    CHECK(sitor_correct(0x7FFFFFFFu, most) == 0x7FFFFFFFu + most);
    CHECK(sitor_correct(0x7FFFFFFFu, 1u) == 0x80000000u);
    CHECK(sitor_correct(0x80000000u, most) == 0x80000000u - most);
    CHECK(sitor_correct(0x80000000u, 1u) == 0x7FFFFFFFu);
    CHECK(sitor_correct(0xFFFFFFFFu, most) == 0xFFFFFFFFu - most);
    CHECK(sitor_correct(0xFFFFFFFFu, 0u) == 0xFFFFFFFFu);
    for (int i = 0; i < 20000; ++i) {
        const uint32_t step = rnd() % (most + 1u), acc = rnd();
        const uint64_t want = acc < 0x80000000u ? (uint64_t)acc + step : (uint64_t)acc - step;
        CHECK(want <= 0xFFFFFFFFull && sitor_correct(acc, step) == (uint32_t)want);
    }
}

static void test_modem_and_weight()
{
    CHECK(sitor_modem_ok(SitorModem{ 1u, 0u, 0u, 1u }));
    CHECK(sitor_modem_ok(SitorModem{ 1u << 29, 1u << 29, 4u, 15u }));
    CHECK(!sitor_modem_ok(SitorModem{ 0u, 0u, 3u, 4u }));
    CHECK(!sitor_modem_ok(SitorModem{ (1u << 29) + 1u, 0u, 3u, 4u }));
    CHECK(!sitor_modem_ok(SitorModem{ 100u, 101u, 3u, 4u }));
    CHECK(!sitor_modem_ok(SitorModem{ 100u, 1u, 1u, 4u }));
    CHECK(!sitor_modem_ok(SitorModem{ 100u, 1u, 5u, 4u }));
    CHECK(!sitor_modem_ok(SitorModem{ 100u, 1u, 3u, 0u }));
    CHECK(!sitor_modem_ok(SitorModem{ 100u, 1u, 3u, 16u }));
    int four = 0;
    for (uint32_t c = 0; c < 128u; ++c) {
        uint32_t w = 0;
        for (int b = 0; b < 7; ++b)
            w += (c >> b) & 1u;
        CHECK(sitor_weight(c) == w);
        CHECK(sitor_weight(c | 0x80u) == w);                          /* the low seven bits only */
        four += w == 4u;
    }
    CHECK(four == 35);
    CHECK(sitor_weight(kSitorAlpha) == 4u && sitor_weight(kSitorBeta) == 4u);
    CHECK(kSitorPhaseA == 0x1ECC7B3u && kSitorPhaseB == 0x663D98Fu);
}

/* a bit series through the framing, a strobe every 16 samples from m0 on; the records go to out */
struct Run {
    SitorFrame f{};
    SitorModem k{ 1u << 28, 0u, 3u, 4u };
    std::vector<SitorChar> out;
    uint64_t m = 0;
    void bit(uint32_t mark, float q = 1.0f)
    {
        SitorChar c{};
        if (sitor_strobe(f, k, mark ? 0u : 1u, m, q, &c))
            out.push_back(c);
        m += 16u;
    }
    void code(uint32_t c, float q = 1.0f)
    {
        for (int b = 0; b < 7; ++b)
            bit((c >> b) & 1u, q);
    }
};

static void test_phasing_at_every_phase()
{
    /* `lead` bits of mark in front: the phasing sequence begins at each of the 7 bit phases of the receiver's strobes.
     * Rule b locks on the first complete word, at the true phase, whatever rule c did before */
    for (uint32_t lock : { 0u, 2u, 3u, 4u })
        for (int lead = 0; lead < 7; ++lead) {
            Run r;
            r.k.lock = lock;
            for (int i = 0; i < lead; ++i)
                r.bit(1u);
            for (int p = 0; p < 4; ++p) {
                r.code(kSitorBeta);
                r.code(kSitorAlpha);
            }
            CHECK(r.f.locked == 1u && r.f.nb == 0u);
            const size_t before = r.out.size();
            const uint32_t text[] = { 0x63u, 0x1Du, 0x63u, 0x1Du };    /* Z C Z C */
            for (uint32_t c : text)
                r.code(c);
            CHECK(r.out.size() == before + 4u);
            for (int i = 0; i < 4; ++i) {
                CHECK(r.out[before + i].code == text[i] && r.out[before + i].flags == kSitorValid);
                CHECK(r.out[before + i].start == (uint64_t)(lead + 56 + 7 * i) * 16u);
            }
            CHECK(r.f.symbols == (uint32_t)(lead + 84));
            CHECK(r.f.chars == r.out.size());
        }
}

static void test_wrong_phase_reframed()
{
    /* from an empty register, lock = 2: behind beta alpha, read from bit 3 of the beta on, the groups are 0x66, 0x61 ...
     * find a phase whose groups are all valid by trying: the header says four of the seven are */
    int all_valid = 0, reframed = 0;
    for (int skip = 0; skip < 7; ++skip) {
        Run r;
        r.k.lock = 2u;
        std::vector<uint32_t> bits;
        for (int p = 0; p < 8; ++p)
            for (uint32_t c : { kSitorBeta, kSitorAlpha })
                for (int b = 0; b < 7; ++b)
                    bits.push_back((c >> b) & 1u);
        /* the receiver's register is empty when bit `skip` arrives: rule c sees groups at phase skip */
        size_t i = (size_t)skip;
        for (; i < (size_t)skip + 14u; ++i)
            r.bit(bits[i]);
        const bool wrong_lock = r.f.locked && skip != 0;
        all_valid += r.f.locked ? 1 : 0;
        for (; i < bits.size(); ++i)
            r.bit(bits[i]);
        /* the first complete phasing word behind the empty register comes 28 bits in at the latest + up to 6: rule b has
         * acted, the framing is at the true phase, and a wrong lock was counted as a reframe */
        CHECK(r.f.locked == 1u);
        CHECK(r.f.nb == (uint32_t)((bits.size()) % 7u));
        if (wrong_lock) {
            CHECK(r.f.reframes >= 1u);
            ++reframed;
        }
        r.code(0x63u);
        CHECK(r.out.back().code == 0x63u && r.out.back().flags == kSitorValid);
    }
    CHECK(all_valid == 4);                                            /* phase 0 and three wrong ones */
    CHECK(reframed == 3);
}

static void test_unlock_and_relock()
{
    for (uint32_t unlock : { 1u, 4u, 15u }) {
        Run r;
        r.k.unlock = unlock;
        r.k.lock = 3u;
        for (int p = 0; p < 2; ++p) {
            r.code(kSitorBeta);
            r.code(kSitorAlpha);
        }
        CHECK(r.f.locked == 1u);
        /* unlock - 1 bad characters, a good one, and the count starts again */
        for (uint32_t i = 0; i + 1u < unlock; ++i)
            r.code(0x7Fu, 0.25f);
        CHECK(r.f.locked == 1u && r.f.bad == unlock - 1u && r.f.errors == unlock - 1u);
        r.code(0x63u);
        CHECK(r.f.bad == 0u);
        for (uint32_t i = 0; i < unlock; ++i) {
            CHECK(r.f.locked == 1u);
            r.code(0x00u, 0.5f);
        }
        CHECK(r.f.locked == 0u && r.f.seen == 0u && r.f.errors == 2u * unlock - 1u);
        CHECK(r.out.back().flags == 0u && r.out.back().code == 0u && r.out.back().quality == 0.5f);
        /* relock by rule c needs 7 lock fresh bits: 20 valid-looking bits do not lock, the 21st does */
        const size_t n = r.out.size();
        const uint32_t text[] = { 0x63u, 0x1Du, 0x47u };
        for (int c = 0; c < 3; ++c)
            for (int b = 0; b < 7; ++b) {
                CHECK(r.f.locked == 0u);
                r.bit((text[c] >> b) & 1u);
            }
        CHECK(r.f.locked == 1u && r.f.nb == 0u && r.out.size() == n);
        r.code(0x4Bu);
        CHECK(r.out.size() == n + 1u && r.out.back().code == 0x4Bu);
    }
    /* lock = 0: valid characters alone never lock; the phasing word does */
    Run r;
    r.k.lock = 0u;
    for (int i = 0; i < 40; ++i)
        r.code(i & 1 ? 0x63u : 0x1Du);
    CHECK(r.f.locked == 0u && r.out.empty() && r.f.symbols == 280u && r.f.seen == 28u);
    for (int p = 0; p < 2; ++p) {
        r.code(kSitorBeta);
        r.code(kSitorAlpha);
    }
    CHECK(r.f.locked == 1u && r.f.reframes == 1u);
    /* quality: the least of the seven, a NaN among them dropped; start: the first strobe's sample */
    const uint64_t m = r.m;
    const float nan = __builtin_nanf("");
    const float q[7] = { 0.9f, nan, 0.3f, 0.8f, nan, 0.7f, 0.6f };
    for (int b = 0; b < 7; ++b)
        r.bit((0x63u >> b) & 1u, q[b]);
    CHECK(r.out.size() == 1u && r.out[0].start == m && r.out[0].quality == 0.3f && r.out[0].code == 0x63u);
    /* restart: the framing as at create, the counters stay */
    const uint32_t chars = r.f.chars, symbols = r.f.symbols;
    sitor_frame_restart(r.f);
    CHECK(r.f.locked == 0u && r.f.reg == 0u && r.f.seen == 0u && r.f.nb == 0u && r.f.bad == 0u);
    CHECK(r.f.chars == chars && r.f.symbols == symbols && r.f.reframes == 1u);
}

/* The adversarial series: the decision alternates at every sample of a bit's first half (acc < 2^31 behind the sample's
 * increment), so the clock is advanced there every time, and holds through the second half.  Every window of the strobes'
 * samples is held against sitor_most, every window of the emissions against sitor_most_chars. */
static uint64_t test_bounds(uint32_t inc, uint32_t step, uint32_t samples)
{
    const SitorModem k{ inc, step, 2u, 15u };
    const uint64_t D = sitor_distance(k);
    CHECK(D >= 4u);
    std::vector<uint32_t> strobes, emissions;
    SitorFrame f{};
    uint32_t acc = 0u, prev = 0u;
    for (uint32_t m = 0; m < samples; ++m) {
        const bool strobe = sitor_clock(acc, inc);
        const uint32_t space = acc < 0x80000000u ? prev ^ 1u : prev;
        if (strobe) {
            strobes.push_back(m);
            SitorChar c{};
            /* the framing is fed valid characters whatever the decisions are: the most emissions there can be */
            const uint32_t bit = (kSitorBeta >> (f.symbols % 7u)) & 1u;
            if (sitor_strobe(f, k, bit ^ 1u, m, 1.0f, &c))
                emissions.push_back(m);
        }
        if (space != prev)
            acc = sitor_correct(acc, step);
        prev = space;
    }
    CHECK(strobes.size() > 16u && emissions.size() > 2u);
    uint64_t least = ~0ull;
    for (size_t i = 1; i < strobes.size(); ++i)
        least = strobes[i] - strobes[i - 1] < least ? strobes[i] - strobes[i - 1] : least;
    CHECK(least >= D);
    for (size_t i = 1; i < emissions.size(); ++i)
        CHECK(emissions[i] - emissions[i - 1] >= 7u * D);
    /* every window [a, a + n) of the series holds at most the bounds */
    for (uint32_t n : { 1u, 2u, 3u, (uint32_t)D, (uint32_t)D + 1u, 7u * (uint32_t)D, 255u, 256u, 257u, 977u })
        for (uint32_t a = 0; a + n <= samples; ++a) {
            uint64_t s = 0, e = 0;
            for (uint32_t v : strobes)
                s += v >= a && v < a + n;
            for (uint32_t v : emissions)
                e += v >= a && v < a + n;
            CHECK(s <= sitor_most(n, D));
            CHECK(e <= sitor_most_chars(sitor_most(n, D)));
        }
    CHECK(sitor_most(0u, D) == 0u && sitor_most_chars(0u) == 0u && sitor_most(1u, D) == 1u && sitor_most_chars(1u) == 1u);
    CHECK(sitor_most_chars(7u) == 1u && sitor_most_chars(8u) == 2u);
    return least;
}

int main()
{
    test_jump();
    test_corrections();
    test_modem_and_weight();
    test_phasing_at_every_phase();
    test_wrong_phase_reframed();
    test_unlock_and_relock();
    const uint64_t least = test_bounds(1u << 29, 1u << 29, 1500u);
    test_bounds((1u << 29) - 161061u, (1u << 29) - 161061u, 1500u);
    test_bounds(1u << 28, 1u << 28, 1500u);
    test_bounds(1u << 28, 1u << 26, 1500u);
    test_bounds(268354925u, 268354925u / 4u, 1500u);
    printf("ok: %ld checks, least strobe distance %llu against the bound %llu\n", checks, (unsigned long long)least,
           (unsigned long long)sitor_distance(SitorModem{ 1u << 29, 1u << 29, 2u, 15u }));
    return 0;
}
