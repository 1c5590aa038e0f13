/*
 * ddc_mfsk_bits.h -- the MFSK decoder's symbol clock (include/perseus_ddc.h, "mfsk"), the test of a modem and the
 * arithmetic of its capacity bound and of what it keeps per receiver, written once in plain integers: k_mfsk
 * (ddc_mfsk.hip) jumps with it from strobe to strobe, ddc_mfsk.cpp uses the bound and the modem test,
 * tests/mfsk_bits_test.cpp runs it under sanitizers.
 * No HIP header: PDDC_MFSK_HD is empty for a host compiler and __host__ __device__ under hipcc.
 *
 * One sample of the definition is mfsk_clock (-> strobe); on a strobe the caller reads the tone, the runner-up and the
 * two powers at the on-time sample and corrects the clock from the early and the late power (mfsk_late / mfsk_early).
 * Between two strobes nothing of the record changes but acc, which mfsk_jump and mfsk_advance move by many samples at once.
 * The clock is psk's (ddc_psk_bits.h) under the decoder's own names: the two decoders share a scheme, not a header, so
 * that either can change its rule without the other.
 */
#ifndef PDDC_DDC_MFSK_BITS_H
#define PDDC_DDC_MFSK_BITS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PDDC_MFSK_HD __host__ __device__
#else
#define PDDC_MFSK_HD
#endif

namespace pddc {

static constexpr uint32_t kMfskIncMost = 1u << 29;        /* a symbol is at least 8 samples                        */
static constexpr uint32_t kMfskQMost = 64u;
static constexpr uint32_t kMfskTonesMost = 32u;
static constexpr uint32_t kMfskPairsMost = kMfskTonesMost / 2u;
static constexpr uint32_t kMfskBack = 2u * kMfskQMost;    /* per-sample results kept in front of a tile: 2 q at the most */

/* a modem: the number of tones and its clock (the symbol phase per sample, the early / late offset in samples, the
 * correction per strobe) */
struct MfskModem {
    uint32_t ntones, inc, q, step;
};

/* pddc_mfsk_sym, 16 bytes */
struct MfskSym {
    uint64_t start;
    uint8_t tone, second;
    uint16_t flags;
    float quality;
};

PDDC_MFSK_HD inline bool mfsk_modem_ok(const MfskModem &k)
{
    return k.ntones >= 2u && k.ntones <= kMfskTonesMost && k.inc >= 1u && k.inc <= kMfskIncMost && k.q >= 1u && k.q <= kMfskQMost &&
           4ull * k.q * k.inc <= (1ull << 32) && k.step <= k.inc;
}

/* tone pairs the filter loop runs: an odd M has a padded zero tone in its last pair, whose second half is skipped */
PDDC_MFSK_HD inline uint32_t mfsk_pairs(uint32_t ntones) { return (ntones + 1u) / 2u; }

/* one sample of the clock; -> true on a strobe: a wrap, unless a late correction borrowed from it (skip) */
PDDC_MFSK_HD inline bool mfsk_clock(uint32_t &acc, uint32_t &skip, uint32_t inc)
{
    const uint32_t a2 = acc + inc;
    const bool wrap = a2 < acc;
    acc = a2;
    if (!wrap)
        return false;
    const bool strobe = skip == 0u;
    skip = 0u;
    return strobe;
}

/* the samples to the next wrap, that one included: the least k >= 1 with acc + k inc >= 2^32 (2^32 itself for acc = 0
 * and inc = 1, hence 64 bits; the division is one of 32) */
PDDC_MFSK_HD inline uint64_t mfsk_jump(uint32_t acc, uint32_t inc) { return (uint64_t)(~acc / inc) + 1u; }

/* k samples of the clock at once (mod 2^32: mfsk_jump samples end on the wrap's acc) */
PDDC_MFSK_HD inline uint32_t mfsk_advance(uint32_t acc, uint32_t inc, uint32_t k) { return acc + k * inc; }

/* the two corrections behind a strobe: the peak lies later / earlier than the on-time sample.  Behind a strobe acc <
 * inc is the fraction of a sample the wrap overshot by; a late correction larger than that goes below zero: the next
 * sample wraps it back (acc - step + inc >= 0, since step <= inc), and skip keeps that wrap from being a strobe */
PDDC_MFSK_HD inline uint32_t mfsk_late(uint32_t acc, uint32_t &skip, uint32_t step)
{
    if (acc < step)
        skip = 1u;
    return acc - step;
}
/* (behind a strobe acc < inc <= 2^29 and step <= inc: no overflow) */
PDDC_MFSK_HD inline uint32_t mfsk_early(uint32_t acc, uint32_t step) { return acc + step; }

/* The capacity bound.  Behind a strobe acc = a2 < inc; a late correction only puts the next strobe off, an early one adds step:
 * acc <= inc - 1 + step.  The next strobe is the least k with acc + k inc >= 2^32, so k >= ceil((2^32 - (inc - 1 +
 * step)) / inc) = floor((2^32 - step) / inc): two strobes lie at least mfsk_distance samples apart (at least 7), and n
 * consecutive samples hold at most mfsk_most(n, distance). */
PDDC_MFSK_HD inline uint64_t mfsk_distance(const MfskModem &k) { return ((1ull << 32) - k.step) / k.inc; }
PDDC_MFSK_HD inline uint64_t mfsk_most(uint64_t n, uint64_t distance) { return n ? (n - 1u) / distance + 1u : 0u; }

/* What a receiver carries in front of a batch, in 8-byte slots: its last W - 1 inputs, then (b, r) of its last kMfskBack
 * samples, one slot each, then their two tone indices, two bytes a sample and four samples a slot */
PDDC_MFSK_HD inline int mfsk_hist_slots(int window) { return window - 1 + (int)kMfskBack + (int)kMfskBack / 4; }

/* the taps of a modem on the device, in floats: per tone pair and tap (h_2p.re, h_2p.im, h_2p+1.re, h_2p+1.im), the
 * taps of a pair in a row of `row` (the window rounded up to whole passes of the tap loop) */
PDDC_MFSK_HD inline long long mfsk_pair_floats(int row) { return 4ll * row; }
PDDC_MFSK_HD inline long long mfsk_modem_floats(int row) { return (long long)kMfskPairsMost * mfsk_pair_floats(row); }

} // namespace pddc
#endif
