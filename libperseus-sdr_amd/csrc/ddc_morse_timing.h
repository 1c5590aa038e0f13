/*
 * ddc_morse_timing.h -- the Morse decoder's element timing (include/perseus_ddc.h, "morse", step 4) and the arithmetic
 * of its capacity bound, written once in plain integers: k_morse (ddc_morse.hip) advances it from event to event,
 * ddc_morse.cpp uses the bound and the reset, tests/morse_timing_test.cpp runs it under sanitizers.
 * No HIP header: PDDC_MORSE_HD is empty for a host compiler and __host__ __device__ under hipcc.
 *
 * One sample of the definition is, in this order, with prev the previous sample's key:
 *   1. morse_emit_due -> morse_emit      a character whose gap has reached its length
 *   2. key && !prev   -> morse_rise
 *   3. !key && prev   -> morse_fall
 * morse_step does exactly that.  Between two events nothing of the record changes, which is why the kernel may jump.
 */
#ifndef PDDC_DDC_MORSE_TIMING_H
#define PDDC_DDC_MORSE_TIMING_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PDDC_MORSE_HD __host__ __device__
#else
#define PDDC_MORSE_HD
#endif

namespace pddc {

static constexpr uint32_t kMorseTwoLeast = 512u;          /* two dots of one sample each                           */
static constexpr uint32_t kMorseTwoMost = 1u << 28;
static constexpr uint32_t kMorseMaxShift = 8u;
static constexpr uint64_t kMorseMaxDur = 1ull << 24;      /* a mark's length saturates here                        */
static constexpr uint64_t kMorseMaxGap = 1ull << 40;      /* the word test's gap saturates here, far beyond 5 two  */
static constexpr uint32_t kMorseCodeBits = 15u;           /* elements a code holds under its sentinel              */
static constexpr uint32_t kMorseWordFlag = 0x1, kMorseLongFlag = 0x2;

/* a keyer's timing parameters: the length of TWO dots in samples times 256 */
struct MorseKeyer {
    uint32_t two0, two_min, two_max;
    uint32_t shift;
};

/* pddc_morse_char, 16 bytes */
struct MorseChar {
    uint64_t start;
    uint16_t code;
    uint8_t nel;
    uint8_t flags;
    uint32_t two;
};

/* what the timing carries */
struct MorseTiming {
    uint64_t start;           /* sample of the first rising edge of the character in progress                       */
    uint64_t t_up;            /* sample of the last falling edge: the key has been up since                         */
    uint64_t t_down;          /* sample of the last rising edge                                                     */
    uint32_t two;
    uint32_t last;            /* the previous mark's length, 0: none                                                */
    uint32_t nel;             /* elements of the character in progress, saturating at 255                           */
    uint32_t code;            /* 1, then an element per bit, dash = 1, the first element highest                    */
    uint32_t word;
    uint32_t first;
    uint32_t chars, marks;    /* counters: never cleared by a restart                                               */
};

PDDC_MORSE_HD inline bool morse_keyer_ok(const MorseKeyer &k)
{
    return k.two_min >= kMorseTwoLeast && k.two_min <= k.two0 && k.two0 <= k.two_max && k.two_max <= kMorseTwoMost &&
           k.shift <= kMorseMaxShift;
}

/* timing as at create with this keyer; the counters stay */
PDDC_MORSE_HD inline void morse_restart(MorseTiming &t, uint32_t two0)
{
    t.start = t.t_up = t.t_down = 0;
    t.two = two0;
    t.last = 0;
    t.nel = 0;
    t.code = 1;
    t.word = 0;
    t.first = 1;
}

/* samples of silence that end a character: two dots, rounded up */
PDDC_MORSE_HD inline uint64_t morse_gap(uint32_t two) { return ((uint64_t)two + 255u) >> 8; }

/* step 1's condition at sample m */
PDDC_MORSE_HD inline bool morse_emit_due(const MorseTiming &t, bool prev, uint64_t m)
{
    return !prev && t.nel > 0 && m - t.t_up == morse_gap(t.two);
}

PDDC_MORSE_HD inline MorseChar morse_emit(MorseTiming &t)
{
    MorseChar c;
    c.start = t.start;
    c.code = (uint16_t)t.code;
    c.nel = (uint8_t)t.nel;
    c.flags = (uint8_t)((t.word ? kMorseWordFlag : 0u) | (t.nel > kMorseCodeBits ? kMorseLongFlag : 0u));
    c.two = t.two;
    ++t.chars;
    t.nel = 0;
    t.code = 1;
    return c;
}

/* step 2: the key went down at sample m */
PDDC_MORSE_HD inline void morse_rise(MorseTiming &t, uint64_t m)
{
    t.t_down = m;
    if (t.nel == 0) {
        uint64_t gap = m - t.t_up;
        gap = gap > kMorseMaxGap ? kMorseMaxGap : gap;
        t.start = m;
        t.word = (t.first || (gap << 9) >= 5ull * t.two) ? 1u : 0u;
    }
}

/* step 3: the key came up at sample m */
PDDC_MORSE_HD inline void morse_fall(MorseTiming &t, const MorseKeyer &k, bool fixed, uint64_t m)
{
    uint64_t d = m - t.t_down;
    d = d > kMorseMaxDur ? kMorseMaxDur : d;
    const uint32_t dur = (uint32_t)d;
    const uint32_t dash = (d << 8) >= t.two ? 1u : 0u;
    if (t.nel < kMorseCodeBits)
        t.code = t.code << 1 | dash;
    if (t.nel < 255u)
        ++t.nel;
    ++t.marks;
    if (!fixed && t.last > 0) {
        const uint64_t a = dur < t.last ? dur : t.last, b = dur < t.last ? t.last : dur;
        if (b >= 2 * a && b <= 4 * a) {
            /* a dot beside a dash: their sum is two dots.  The shift of a negative difference is the arithmetic one
             * (it rounds down), as gcc, clang and hipcc define it; the host test holds a vector for it */
            const int64_t err = (int64_t)((a + b) << 7) - (int64_t)t.two;
            int64_t two = (int64_t)t.two + (err >> k.shift);
            two = two < (int64_t)k.two_min ? (int64_t)k.two_min : two;
            two = two > (int64_t)k.two_max ? (int64_t)k.two_max : two;
            t.two = (uint32_t)two;
        }
    }
    t.last = dur;
    t.t_up = m;
    t.first = 0;
}

/* one sample of the definition; -> true if a character was emitted into *out */
PDDC_MORSE_HD inline bool morse_step(MorseTiming &t, const MorseKeyer &k, bool fixed, bool prev, bool key, uint64_t m, MorseChar *out)
{
    bool emitted = false;
    if (morse_emit_due(t, prev, m)) {
        *out = morse_emit(t);
        emitted = true;
    }
    if (key && !prev)
        morse_rise(t, m);
    if (!key && prev)
        morse_fall(t, k, fixed, m);
    return emitted;
}

/* The capacity bound.  An emission at sample e leaves nel = 0; the next needs a rising edge at r >= e (the same sample
 * at the earliest), a falling edge at f >= r + 1 and then morse_gap(two) >= morse_gap(two_min) samples: two emissions
 * lie at least morse_distance(two_min) samples apart, and n consecutive samples hold at most morse_most(n, distance). */
PDDC_MORSE_HD inline uint64_t morse_distance(uint32_t two_min) { return 1u + morse_gap(two_min); }
PDDC_MORSE_HD inline uint64_t morse_most(uint64_t n, uint64_t distance) { return n ? (n - 1u) / distance + 1u : 0u; }

} // namespace pddc
#endif
