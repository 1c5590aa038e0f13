/*
 * ddc_sitor_bits.h -- the SITOR decoder's bit clock, its framing (include/perseus_ddc.h, "sitor", rules a - c) and the
 * arithmetic of its two capacity bounds, written once in plain integers: k_sitor (ddc_sitor.hip) goes with it from event
 * to event, ddc_sitor.cpp uses the bounds and the modem test, tests/sitor_bits_test.cpp runs it under sanitizers.
 * No HIP header: PDDC_SITOR_HD is empty for a host compiler and __host__ __device__ under hipcc.
 *
 * One sample of the definition is sitor_clock (-> strobe); on a strobe the caller gives the decision and |d| to
 * sitor_strobe; behind it, on a sample whose decision differs from the previous one's, sitor_correct moves the clock.
 * Between two events (strobes and transitions) the record does not change but for acc, which sitor_jump and
 * sitor_advance move by many samples at once.
 */
#ifndef PDDC_DDC_SITOR_BITS_H
#define PDDC_DDC_SITOR_BITS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PDDC_SITOR_HD __host__ __device__
#else
#define PDDC_SITOR_HD
#endif

namespace pddc {

static constexpr uint32_t kSitorIncMost = 1u << 29;       /* a bit is at least 8 samples                           */
static constexpr uint32_t kSitorUnlockMost = 15u;
static constexpr uint32_t kSitorValid = 0x1;              /* SitorChar.flags: four of the seven bits are ones      */
static constexpr uint32_t kSitorAlpha = 0x0F, kSitorBeta = 0x33;   /* phasing signals 1 and 2, first-received bit lowest */
static constexpr uint32_t kSitorRegBits = 28u, kSitorCharBits = 7u;
/* the register behind four phasing characters, the newest highest: it ends on alpha, or on beta */
static constexpr uint32_t kSitorPhaseA = kSitorAlpha << 21 | kSitorBeta << 14 | kSitorAlpha << 7 | kSitorBeta;
static constexpr uint32_t kSitorPhaseB = kSitorBeta << 21 | kSitorAlpha << 14 | kSitorBeta << 7 | kSitorAlpha;

/* a modem's clock and framing: the bit phase per sample, the correction per transition, the valid characters in a row
 * that lock without a phasing word (0: never), the invalid ones in a row that unlock */
struct SitorModem {
    uint32_t inc, step, lock, unlock;
};

/* pddc_sitor_char, 16 bytes */
struct SitorChar {
    uint64_t start;
    uint16_t code;
    uint16_t flags;
    float quality;
};

/* what the framing carries, and the counters */
struct SitorFrame {
    uint64_t start;           /* sample of the first strobe of the character in progress                           */
    uint32_t reg;             /* the last 28 bits, the newest in bit 27                                            */
    uint32_t seen;            /* bits since the register was empty, saturating at 28                               */
    uint32_t nb;              /* bits of the character in progress, 0 .. 6                                         */
    uint32_t bad;             /* invalid characters in a row                                                       */
    uint32_t locked;
    float qmin;               /* the least |d| among the character's strobes                                       */
    uint32_t chars, symbols, errors, reframes;   /* counters: never cleared by a restart                           */
};

PDDC_SITOR_HD inline bool sitor_modem_ok(const SitorModem &k)
{
    return k.inc >= 1u && k.inc <= kSitorIncMost && k.step <= k.inc && (k.lock == 0u || (k.lock >= 2u && k.lock <= 4u)) &&
           k.unlock >= 1u && k.unlock <= kSitorUnlockMost;
}

/* one sample of the clock; -> true on a strobe */
PDDC_SITOR_HD inline bool sitor_clock(uint32_t &acc, uint32_t inc)
{
    const uint32_t a2 = acc + inc;
    const bool strobe = a2 < acc;
    acc = a2;
    return strobe;
}

/* the samples to the next strobe of an uncorrected clock, that one included: the least k >= 1 with acc + k inc >= 2^32
 * (2^32 itself for acc = 0 and inc = 1, hence 64 bits; the division is one of 32) */
PDDC_SITOR_HD inline uint64_t sitor_jump(uint32_t acc, uint32_t inc) { return (uint64_t)(~acc / inc) + 1u; }

/* k samples of the clock at once (mod 2^32: sitor_jump samples end on the strobe's acc) */
PDDC_SITOR_HD inline uint32_t sitor_advance(uint32_t acc, uint32_t inc, uint32_t k) { return acc + k * inc; }

/* the correction on a transition: in a bit's first half the strobe comes sooner, in its second half later.  Neither
 * wraps: below 2^31 the sum stays below 2^31 + 2^29; from 2^31 on acc >= 2^31 > step */
PDDC_SITOR_HD inline uint32_t sitor_correct(uint32_t acc, uint32_t step) { return acc < 0x80000000u ? acc + step : acc - step; }

/* ones among the low 7 bits */
PDDC_SITOR_HD inline uint32_t sitor_weight(uint32_t code)
{
    uint32_t v = code & 0x7Fu;
    v = (v & 0x55u) + ((v >> 1) & 0x55u);
    v = (v & 0x33u) + ((v >> 2) & 0x33u);
    return (v & 0x0Fu) + (v >> 4);
}

/* fminf without a math header: a NaN gives the other value (|d| is never -0) */
PDDC_SITOR_HD inline float sitor_fmin(float a, float b) { return a != a ? b : (b < a ? b : a); }

/* the newest `count` (0 .. 4) 7-bit groups of the register have four ones each */
PDDC_SITOR_HD inline bool sitor_groups_valid(uint32_t reg, uint32_t count)
{
    for (uint32_t g = 0; g < count; ++g)
        if (sitor_weight(reg >> (21u - 7u * g)) != 4u)
            return false;
    return true;
}

/* a strobe at sample m with the decision `space` and q = |d|: step 2 of the definition, rules a - c; -> true if a
 * character went into *out */
PDDC_SITOR_HD inline bool sitor_strobe(SitorFrame &f, const SitorModem &k, uint32_t space, uint64_t m, float q, SitorChar *out)
{
    bool emitted = false;
    ++f.symbols;
    f.reg = (f.reg >> 1) | ((space ? 0u : 1u) << 27);
    if (f.seen < kSitorRegBits)
        ++f.seen;
    if (f.locked) {                                                   /* a */
        if (f.nb == 0u) {
            f.start = m;
            f.qmin = q;
        } else {
            f.qmin = sitor_fmin(f.qmin, q);
        }
        if (++f.nb == kSitorCharBits) {
            const uint32_t code = f.reg >> 21;
            const bool valid = sitor_weight(code) == 4u;
            out->start = f.start;
            out->code = (uint16_t)code;
            out->flags = (uint16_t)(valid ? kSitorValid : 0u);
            out->quality = f.qmin;
            emitted = true;
            ++f.chars;
            f.nb = 0u;
            if (valid) {
                f.bad = 0u;
            } else {
                ++f.errors;
                ++f.bad;
            }
            if (f.bad >= k.unlock) {
                f.locked = 0u;
                f.seen = 0u;
            }
        }
    }
    if (f.reg == kSitorPhaseA || f.reg == kSitorPhaseB) {             /* b */
        if (!(f.locked && f.nb == 0u))
            ++f.reframes;
        f.locked = 1u;
        f.nb = 0u;
        f.bad = 0u;
    } else if (!f.locked && k.lock > 0u && f.seen >= kSitorCharBits * k.lock && sitor_groups_valid(f.reg, k.lock)) {   /* c */
        f.locked = 1u;
        f.nb = 0u;
        f.bad = 0u;
    }
    return emitted;
}

/* framing as at create; the counters stay */
PDDC_SITOR_HD inline void sitor_frame_restart(SitorFrame &f)
{
    f.start = 0;
    f.reg = f.seen = f.nb = f.bad = f.locked = 0u;
    f.qmin = 0.0f;
}

/* The capacity bounds.  A strobe needs acc + inc >= 2^32, so acc >= 2^32 - 2^29 in front of it; behind it acc < inc, and
 * the correction on that sample adds at most step: acc < 2^30.  The clock is advanced (acc += step) below 2^31 only, and
 * a sample ends with acc in [2^31, 2^32) for the first time behind a strobe with acc < 2^31 + inc (it came from below
 * 2^31 by + inc, or by + inc + step and - 0, or by + inc < 2^31 and + step <= inc).  From there to the next strobe every
 * sample adds inc and a transition only subtracts (or, having fallen below 2^31 again, starts this count anew): at
 * least k samples with 2^31 + inc - 1 + k inc >= 2^32, k >= floor(2^31 / inc).  Two strobes lie at least sitor_distance
 * samples apart (at least 4), and n consecutive samples hold at most sitor_most(n, distance).  An emission needs seven
 * strobes behind the previous one (rule b only sets nb back, and a relock comes no sooner than the strobe behind the
 * unlock): sitor_most_chars. */
PDDC_SITOR_HD inline uint64_t sitor_distance(const SitorModem &k) { return (1ull << 31) / k.inc; }
PDDC_SITOR_HD inline uint64_t sitor_most(uint64_t n, uint64_t distance) { return n ? (n - 1u) / distance + 1u : 0u; }
PDDC_SITOR_HD inline uint64_t sitor_most_chars(uint64_t syms) { return syms ? (syms - 1u) / 7u + 1u : 0u; }

} // namespace pddc
#endif
