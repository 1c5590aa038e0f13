/*
 * ddc_psk_bits.h -- the PSK decoder's symbol clock, its framing (include/perseus_ddc.h, "psk") and the arithmetic of its
 * two capacity bounds, written once in plain integers: k_psk (ddc_psk.hip) jumps with it from strobe to strobe,
 * ddc_psk.cpp uses the bounds and the modem test, tests/psk_bits_test.cpp runs it under sanitizers.
 * No HIP header: PDDC_PSK_HD is empty for a host compiler and __host__ __device__ under hipcc.
 *
 * One sample of the definition is psk_clock (-> strobe); on a strobe the caller makes d, x and the bit from the filter's
 * outputs, corrects the clock on a reversal (psk_late / psk_early) and gives the bit to psk_frame.  Between two strobes
 * the record does not change but for acc, which psk_jump and psk_advance move by many samples at once.
 */
#ifndef PDDC_DDC_PSK_BITS_H
#define PDDC_DDC_PSK_BITS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PDDC_PSK_HD __host__ __device__
#else
#define PDDC_PSK_HD
#endif

namespace pddc {

static constexpr uint32_t kPskIncMost = 1u << 29;         /* a symbol is at least 8 samples                        */
static constexpr uint32_t kPskQMost = 64u;
static constexpr uint32_t kPskCodeBits = 16u;             /* bits a code holds                                     */
static constexpr uint32_t kPskLongFlag = 0x1;

/* a modem's clock: the symbol phase per sample, the early / late offset in samples, the correction per reversal */
struct PskModem {
    uint32_t inc, q, step;
};

/* pddc_psk_char, 16 bytes */
struct PskChar {
    uint64_t start;
    uint16_t code;
    uint8_t nbits;
    uint8_t flags;
    float quality;
};

/* what the framing carries, and the counters */
struct PskFrame {
    uint64_t start;           /* on-time sample of the first 1 of the character in progress                        */
    uint32_t reg;             /* the bits since then, the newest lowest; 0: between characters                     */
    uint32_t nb;              /* their number, saturating at 255                                                   */
    float qmin;               /* the least |d| among them                                                          */
    uint32_t chars, symbols;  /* counters: never cleared by a restart                                              */
};

PDDC_PSK_HD inline bool psk_modem_ok(const PskModem &k)
{
    return k.inc >= 1u && k.inc <= kPskIncMost && k.q >= 1u && k.q <= kPskQMost && 4ull * k.q * k.inc <= (1ull << 32) && k.step <= k.inc;
}

/* one sample of the clock; -> true on a strobe */
PDDC_PSK_HD inline bool psk_clock(uint32_t &acc, uint32_t inc)
{
    const uint32_t a2 = acc + inc;
    const bool strobe = a2 < acc;
    acc = a2;
    return strobe;
}

/* the samples to the next strobe, that one included: the least k >= 1 with acc + k inc >= 2^32 (2^32 itself for acc = 0
 * and inc = 1, hence 64 bits; the division is one of 32) */
PDDC_PSK_HD inline uint64_t psk_jump(uint32_t acc, uint32_t inc) { return (uint64_t)(~acc / inc) + 1u; }

/* k samples of the clock at once (mod 2^32: psk_jump samples end on the strobe's acc) */
PDDC_PSK_HD inline uint32_t psk_advance(uint32_t acc, uint32_t inc, uint32_t k) { return acc + k * inc; }

/* the two corrections behind a strobe: the peak lies later / earlier than the on-time sample */
PDDC_PSK_HD inline uint32_t psk_late(uint32_t acc, uint32_t step) { return acc >= step ? acc - step : 0u; }
/* (behind a strobe acc < inc <= 2^29 and step <= inc: no overflow) */
PDDC_PSK_HD inline uint32_t psk_early(uint32_t acc, uint32_t step) { return acc + step; }

/* fminf without a math header: a NaN gives the other value (|d| is never -0) */
PDDC_PSK_HD inline float psk_fmin(float a, float b) { return a != a ? b : (b < a ? b : a); }

/* the framing with one bit whose on-time sample is c and whose |d| is ad; -> true if a character went into *out */
PDDC_PSK_HD inline bool psk_frame(PskFrame &f, uint32_t bit, uint64_t c, float ad, PskChar *out)
{
    if (f.reg == 0u) {
        if (!bit)
            return false;
        f.start = c;
        f.nb = 0u;
        f.qmin = ad;
    }
    f.reg = f.reg << 1 | bit;
    if (f.nb < 255u)
        ++f.nb;
    f.qmin = psk_fmin(f.qmin, ad);
    if ((f.reg & 3u) != 0u)
        return false;
    const uint32_t nbits = f.nb - 2u;
    out->start = f.start;
    out->code = (uint16_t)((f.reg >> 2) & 0xFFFFu);
    out->nbits = (uint8_t)nbits;
    out->flags = (uint8_t)(nbits > kPskCodeBits ? kPskLongFlag : 0u);
    out->quality = f.qmin;
    ++f.chars;
    f.reg = 0u;
    return true;
}

/* framing as at create; the counters stay */
PDDC_PSK_HD inline void psk_frame_restart(PskFrame &f)
{
    f.start = 0;
    f.reg = 0u;
    f.nb = 0u;
    f.qmin = 0.0f;
}

/* The capacity bounds.  Behind a strobe acc = a2 < inc; a late correction only lowers it, an early one adds step:
 * acc <= inc - 1 + step.  The next strobe is the least k with acc + k inc >= 2^32, so k >= ceil((2^32 - (inc - 1 +
 * step)) / inc) = floor((2^32 - step) / inc): two strobes lie at least psk_distance samples apart (at least 7), and n
 * consecutive samples hold at most psk_most(n, distance).  A character ends with 0 0 behind a 1, and the register is 0
 * behind it: two emissions lie at least 3 strobes apart. */
PDDC_PSK_HD inline uint64_t psk_distance(const PskModem &k) { return ((1ull << 32) - k.step) / k.inc; }
PDDC_PSK_HD inline uint64_t psk_most(uint64_t n, uint64_t distance) { return n ? (n - 1u) / distance + 1u : 0u; }
PDDC_PSK_HD inline uint64_t psk_most_chars(uint64_t syms) { return syms ? (syms - 1u) / 3u + 1u : 0u; }

} // namespace pddc
#endif
