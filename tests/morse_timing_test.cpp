/* tests/morse_timing_test.cpp -- the Morse decoder's element timing and capacity arithmetic (csrc/ddc_morse_timing.h: no
 * HIP header, so a host compiler builds it alone) against vectors written out here: the tracker's negative step with
 * its arithmetic shift, both clamps, the element count at 15, 16 and 255 with LONG, a mark of 2^24 samples and more,
 * sample counts beyond 2^32, an emission and a rising edge on the same sample, WORD at exactly five dots, and the
 * bound on back-to-back characters.
 * usage: morse_timing_test   -> prints "ok: <checks> checks", exit 0; the first failed check is printed, exit 1 */
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include "ddc_morse_timing.h"

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

/* the receiver of the tests: the timing, the key of the previous sample, and what it emitted */
struct Rx {
    MorseTiming t{};
    MorseKeyer k{};
    bool fixed = false, prev = false;
    uint64_t m = 0;
    MorseChar rec[512];
    uint64_t at[512];
    int n = 0;

    Rx(uint32_t two0, uint32_t two_min, uint32_t two_max, uint32_t shift, bool fix = false, uint64_t m0 = 0)
    {
        k = MorseKeyer{ two0, two_min, two_max, shift };
        CHECK(morse_keyer_ok(k));
        morse_restart(t, two0);
        fixed = fix;
        m = m0;
    }
    /* `count` samples with this key */
    void run(bool key, uint64_t count)
    {
        for (uint64_t i = 0; i < count; ++i, ++m) {
            MorseChar c;
            if (morse_step(t, k, fixed, prev, key, m, &c)) {
                CHECK(n < 512);
                at[n] = m;
                rec[n++] = c;
            }
            prev = key;
        }
    }
};

static void test_restart_and_keyers()
{
    MorseTiming t{};
    t.chars = 7;
    t.marks = 9;
    t.nel = 3;
    t.code = 5;
    morse_restart(t, 8192);
    CHECK(t.two == 8192 && t.nel == 0 && t.code == 1 && t.first == 1 && t.last == 0 && t.word == 0);
    CHECK(t.start == 0 && t.t_up == 0 && t.t_down == 0 && t.chars == 7 && t.marks == 9);     /* the counters stay */
    CHECK(morse_keyer_ok(MorseKeyer{ 512, 512, 512, 0 }) && morse_keyer_ok(MorseKeyer{ 1u << 28, 512, 1u << 28, 8 }));
    CHECK(!morse_keyer_ok(MorseKeyer{ 511, 511, 512, 0 }) && !morse_keyer_ok(MorseKeyer{ 600, 601, 700, 0 }));
    CHECK(!morse_keyer_ok(MorseKeyer{ 701, 600, 700, 0 }) && !morse_keyer_ok(MorseKeyer{ 600, 600, (1u << 28) + 1, 0 }));
    CHECK(!morse_keyer_ok(MorseKeyer{ 600, 600, 700, 9 }));
    CHECK(morse_gap(512) == 2 && morse_gap(513) == 3 && morse_gap(768) == 3 && morse_gap(1u << 28) == 1u << 20);
}

static void test_tracker()
{
    /* marks of 10 and 31 samples: (41 << 7) - 8191 = -2943, >> 3 rounds down to -368 (a division would give -367) */
    Rx r(8191, 512, 1u << 28, 3);
    r.run(false, 100);
    r.run(true, 10);
    r.run(false, 10);
    CHECK(r.t.two == 8191 && r.t.last == 10 && r.t.marks == 1);      /* the first mark has no neighbour */
    r.run(true, 31);
    r.run(false, 1);
    CHECK(r.t.two == 8191 - 368 && r.t.last == 31 && r.t.marks == 2);
    /* a positive step: marks of 31 and 90 are no pair (90 > 4 x 31 is false: 124; 90 >= 62: a pair): (121 << 7) = 15488 */
    r.run(false, 9);
    r.run(true, 90);
    r.run(false, 1);
    CHECK(r.t.two == 7823 + ((15488 - 7823) >> 3));
    /* marks of 90 and 20: 90 > 4 x 20, no pair, two stays; marks of 20 and 39: 39 < 2 x 20, no pair */
    const uint32_t two = r.t.two;
    r.run(false, 5);
    r.run(true, 20);
    r.run(false, 5);
    CHECK(r.t.two == two && r.t.last == 20);
    r.run(true, 39);
    r.run(false, 5);
    CHECK(r.t.two == two && r.t.last == 39);
    /* the bounds of a pair themselves: 40 beside 20 (b = 2 a), 80 beside 20 (b = 4 a) */
    Rx e(8192, 512, 1u << 28, 0);
    e.run(true, 20);
    e.run(false, 3);
    e.run(true, 40);
    e.run(false, 3);
    CHECK(e.t.two == (60u << 7));
    Rx g(8192, 512, 1u << 28, 0);
    g.run(true, 20);
    g.run(false, 3);
    g.run(true, 80);
    g.run(false, 3);
    CHECK(g.t.two == (100u << 7));
    /* FIXED: the same marks, two stays */
    Rx f(8192, 512, 1u << 28, 0, true);
    f.run(true, 20);
    f.run(false, 3);
    f.run(true, 40);
    f.run(false, 3);
    CHECK(f.t.two == 8192 && f.t.marks == 2);
}

static void test_clamps()
{
    Rx lo(8192, 8000, 9000, 0);
    lo.run(true, 10);
    lo.run(false, 4);
    lo.run(true, 30);
    lo.run(false, 1);
    CHECK(lo.t.two == 8000);                                         /* (40 << 7) = 5120, below two_min */
    Rx hi(8192, 8000, 9000, 0);
    hi.run(true, 20);
    hi.run(false, 4);
    hi.run(true, 60);
    hi.run(false, 1);
    CHECK(hi.t.two == 9000);                                         /* (80 << 7) = 10240, above two_max */
    Rx top(1u << 28, 512, 1u << 28, 0);                              /* the widest bounds, the largest marks */
    morse_rise(top.t, 0);
    morse_fall(top.t, top.k, false, 1ull << 23);
    morse_rise(top.t, 1ull << 24);
    morse_fall(top.t, top.k, false, (1ull << 24) + (1ull << 24));
    CHECK(top.t.two == 1u << 28 && top.t.last == 1u << 24);          /* (2^23 + 2^24) << 7 = 3 x 2^30 clamps to 2^28 */
}

/* `marks` marks of one sample a sample apart (dots at two = 8192: the gap of 32 samples never passes), then silence */
static MorseChar many_elements(int marks, bool last_is_dash)
{
    Rx r(8192, 512, 1u << 28, 2, true);
    r.run(false, 3);
    for (int i = 0; i < marks; ++i) {
        r.run(true, last_is_dash && i == marks - 1 ? 32 : 1);
        r.run(false, 1);
    }
    CHECK(r.n == 0);
    const uint64_t up = r.t.t_up;
    r.run(false, 40);
    CHECK(r.n == 1 && r.at[0] == up + 32 && r.t.nel == 0 && r.t.code == 1 && r.t.chars == 1 && (int)r.t.marks == marks);
    CHECK(r.rec[0].start == 3 && r.rec[0].two == 8192);
    return r.rec[0];
}

static void test_element_count()
{
    MorseChar c = many_elements(15, true);
    CHECK(c.nel == 15 && c.code == 0x8001 && c.flags == kMorseWordFlag);                      /* 14 dots and a dash */
    c = many_elements(16, true);
    CHECK(c.nel == 16 && c.code == 0x8000 && c.flags == (kMorseWordFlag | kMorseLongFlag));  /* the 16th is not held */
    c = many_elements(255, false);
    CHECK(c.nel == 255 && c.code == 0x8000 && c.flags == (kMorseWordFlag | kMorseLongFlag));
    c = many_elements(300, false);
    CHECK(c.nel == 255 && c.flags == (kMorseWordFlag | kMorseLongFlag));                     /* saturated */
    c = many_elements(2, true);
    CHECK(c.nel == 2 && c.code == 5 && c.flags == kMorseWordFlag);                            /* "A": 1 0 1 */
}

static void test_long_mark()
{
    Rx r(1u << 28, 512, 1u << 28, 0);
    morse_rise(r.t, 1000);
    morse_fall(r.t, r.k, false, 1000 + (1ull << 24) - 1);
    CHECK(r.t.last == (1u << 24) - 1 && r.t.code == 3);              /* (2^24 - 1) << 8 >= 2^28: a dash */
    morse_rise(r.t, 1ull << 26);
    morse_fall(r.t, r.k, false, (1ull << 26) + (1ull << 24));
    CHECK(r.t.last == 1u << 24);
    morse_rise(r.t, 1ull << 27);
    morse_fall(r.t, r.k, false, (1ull << 27) + (1ull << 40) + 12345);  /* saturates, no overflow in dur << 8 */
    CHECK(r.t.last == 1u << 24 && r.t.code == 15 && r.t.nel == 3 && r.t.t_up == (1ull << 27) + (1ull << 40) + 12345);
    /* sample by sample across 2^24 */
    Rx s(8192, 512, 1u << 28, 0, true);
    s.run(true, (1ull << 24) + 3);
    s.run(false, 1);
    CHECK(s.t.last == 1u << 24 && s.t.code == 3);
}

static void test_beyond_2_32()
{
    for (uint64_t base : { (1ull << 32) - 20, (1ull << 32) + 5, (1ull << 40) + 77, (1ull << 63) + 9 }) {
        Rx r(8192, 512, 1u << 28, 2, false, base);
        r.run(false, 7);
        r.run(true, 16);                                             /* "A" at 16 samples per dot */
        r.run(false, 16);
        r.run(true, 48);
        r.run(false, 40);
        CHECK(r.n == 1 && r.rec[0].start == base + 7 && r.rec[0].code == 5 && r.rec[0].nel == 2);
        CHECK(r.rec[0].flags == kMorseWordFlag && r.rec[0].two == 8192);                      /* (16 + 48) << 7 = 8192 */
        CHECK(r.at[0] == base + 7 + 80 + 32 && r.t.t_up == base + 87 && r.t.t_down == base + 39);
        /* a gap of five dots and more behind it, far from zero: WORD */
        r.run(false, 60);
        r.run(true, 16);
        r.run(false, 40);
        CHECK(r.n == 2 && r.rec[1].flags == kMorseWordFlag && r.rec[1].code == 2 && r.rec[1].start == base + 187);
    }
}

static void test_emission_and_rise_on_one_sample()
{
    Rx r(8192, 512, 1u << 28, 2, true);
    r.run(false, 5);
    r.run(true, 16);
    const uint64_t up = r.m;                                         /* the falling edge's sample */
    r.run(false, 32);                                                /* up .. up + 31: the gap has not passed */
    CHECK(r.n == 0 && r.t.nel == 1);
    r.run(true, 48);                                                 /* the key goes down on sample up + 32 */
    CHECK(r.n == 1 && r.at[0] == up + 32 && r.rec[0].code == 2 && r.rec[0].start == 5);
    CHECK(r.t.start == up + 32 && r.t.t_down == up + 32 && r.t.word == 0);   /* 32 samples are two dots, not five */
    r.run(false, 33);
    CHECK(r.n == 2 && r.rec[1].code == 3 && r.rec[1].start == up + 32 && r.rec[1].flags == 0);
    /* one sample earlier the mark joins the character */
    Rx q(8192, 512, 1u << 28, 2, true);
    q.run(false, 5);
    q.run(true, 16);
    q.run(false, 31);
    q.run(true, 48);
    q.run(false, 33);
    CHECK(q.n == 1 && q.rec[0].code == 5 && q.rec[0].nel == 2);
}

static void test_word_at_five_dots()
{
    for (int gap : { 79, 80, 81 }) {
        Rx r(8192, 512, 1u << 28, 2, true);
        r.run(false, 5);
        r.run(true, 16);
        r.run(false, (uint64_t)gap);                                 /* 80 samples << 9 = 5 x 8192 exactly */
        r.run(true, 16);
        r.run(false, 40);
        CHECK(r.n == 2 && r.rec[0].flags == kMorseWordFlag);         /* the first character of a receiver */
        CHECK(r.rec[1].flags == (gap >= 80 ? kMorseWordFlag : 0u));
    }
}

static void test_capacity()
{
    CHECK(morse_distance(512) == 3 && morse_distance(513) == 4 && morse_distance(1u << 28) == (1u << 20) + 1);
    CHECK(morse_most(0, 3) == 0 && morse_most(1, 3) == 1 && morse_most(3, 3) == 1 && morse_most(4, 3) == 2 && morse_most(7, 3) == 3);
    CHECK(morse_most(1ull << 40, 3) == ((1ull << 40) - 1) / 3 + 1 && morse_most(~0ull, 3) == (~0ull - 1) / 3 + 1);
    /* back to back: marks of one sample, the next on the emission's own sample */
    for (uint32_t two : { 512u, 513u, 2048u }) {
        const uint64_t D = morse_distance(two);
        Rx r(two, two, two, 0, true);
        for (int i = 0; i < 100; ++i) {
            r.run(true, 1);
            r.run(false, D - 1);
        }
        CHECK(r.n == 99 && r.t.marks == 100);
        for (int i = 0; i < r.n; ++i)
            CHECK(r.at[i] == (uint64_t)(i + 1) * D && r.rec[i].nel == 1 && r.rec[i].start == (uint64_t)i * D);
        /* no window of n samples holds more emissions than the bound, and the one that begins on an emission reaches it */
        for (uint64_t n = 0; n < 40; ++n)
            for (uint64_t a = D - 2; a < 3 * D; ++a) {
                uint64_t got = 0;
                for (int i = 0; i < r.n; ++i)
                    got += r.at[i] >= a && r.at[i] < a + n;
                CHECK(got <= morse_most(n, D));
                if (a == D)
                    CHECK(got == morse_most(n, D));
            }
    }
}

int main()
{
    test_restart_and_keyers();
    test_tracker();
    test_clamps();
    test_element_count();
    test_long_mark();
    test_beyond_2_32();
    test_emission_and_rise_on_one_sample();
    test_word_at_five_dots();
    test_capacity();
    printf("ok: %ld checks\n", checks);
    return 0;
}
