/*
 * ddc_morse.h -- internal launch interface between the Morse decoder's host code (ddc_morse.cpp) and its gfx950 kernel
 * (ddc_morse.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The element timing both sides share is
 * in ddc_morse_timing.h.
 */
#ifndef PDDC_DDC_MORSE_H
#define PDDC_DDC_MORSE_H

#include "ddc_morse_timing.h"
#include "ddc_decoder_rx.h"

namespace pddc {

static constexpr int kMorseBlockLog2 = 6;               /* the meter's blocks: the samples with the same m >> 6: an output group */

/* LDS per receiver of the group: the input row */
inline size_t morse_lds_bytes(int window) { return (size_t)kDecGroup * (size_t)dec_in_slots(window) * sizeof(float2); }
static constexpr size_t kMorseLdsCap = (size_t)kDecGroup * (size_t)(kDecMaxWindow - 1 + kDecTile) * 8;

/* receiver flags beside kDecOn and the marks: kDecClear also means meter and timing afresh */
static constexpr uint32_t kMorseFixed = 0x2;
static constexpr uint32_t kMorseRekey = kDecThird;      /* another keyer: meter and timing afresh, the inputs stay   */
static constexpr uint32_t kMorseMarks = kDecFresh | kDecClear | kMorseRekey;

/* the object's float parameters */
struct MorseParams {
    float a_on, a_off, rel, relf, ratio;
};

/* what a receiver carries behind its inputs; read() reports from it */
struct MorseState {
    MorseTiming t;
    uint32_t key;             /* the last sample's key                                                            */
    uint32_t primed;          /* a block has ended since the meter started                                        */
    float hi, lo;             /* the running block's extremes                                                     */
    float pk, fl;             /* 0 until primed                                                                   */
    float on, off;            /* the thresholds that govern the running block                                     */
};

struct MorseArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    MorseChar *chars;         /* [nrx][char_stride]                                                              */
    long long char_stride;    /* >= the bound of pddc_morse_max_chars: the host refuses less                     */
    uint32_t *counts;         /* [nrx]                                                                           */
    float *p;                 /* [nrx][p_stride] or NULL                                                         */
    long long p_stride;
    const float *taps;        /* [nbank][dec_row(W)]                                                             */
    const MorseKeyer *bank;   /* [nbank]                                                                         */
    const DecRx *rx;          /* [nrx]                                                                           */
    const MorseState *state;  /* [nrx] (not read where fresh)                                                    */
    MorseState *new_state;
    const float2 *hist;       /* [nrx][W - 1]: the inputs before the batch's first (not read where fresh or cleared) */
    float2 *new_hist;
    MorseParams par;
    int nrx;
    int nbank;
    int window;               /* W                                                                               */
};

/* k_morse: grid ceil(nrx / kDecGroup) */
hipError_t launch_morse(const MorseArgs &a, hipStream_t s);

} // namespace pddc
#endif
