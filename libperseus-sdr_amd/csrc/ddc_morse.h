/*
 * ddc_morse.h -- internal launch interface between the Morse decoder's host code (ddc_morse.cpp) and its gfx950 kernel
 * (ddc_morse.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The element timing both sides share is
 * in ddc_morse_timing.h.
 */
#ifndef PDDC_DDC_MORSE_H
#define PDDC_DDC_MORSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_morse_timing.h"

namespace pddc {

static constexpr int kMorseMaxRx = 1024;
static constexpr int kMorseMaxKeyers = 16;
static constexpr int kMorseMaxWindow = 256;
static constexpr int kMorseGroup = 4;                   /* G: receivers per block, one wave each                   */
static constexpr int kMorseThreads = 64 * kMorseGroup;
static constexpr int kMorseOut = 4;                     /* O: outputs per lane and tile, 64 apart: a meter block each */
static constexpr int kMorseBlockLog2 = 6;               /* the meter's blocks: the samples with the same m >> 6    */
static constexpr int kMorseTile = 64 * kMorseOut;       /* TT: samples per tile, tiles aligned to m                */
static constexpr int kMorseStep = 8;                    /* taps per pass of the tap loop                           */
/* a keyer's taps on the device: W real taps rounded up to a whole number of passes, zeros behind the W-th */
inline __host__ __device__ int morse_row(int window) { return (window + kMorseStep - 1) / kMorseStep * kMorseStep; }

/* LDS per receiver of the group: W - 1 carried inputs and a tile of them (float2) */
inline __host__ __device__ int morse_row_slots(int window) { return window - 1 + kMorseTile; }
inline size_t morse_lds_bytes(int window) { return (size_t)kMorseGroup * (size_t)morse_row_slots(window) * sizeof(float2); }
static constexpr size_t kMorseLdsCap = (size_t)kMorseGroup * (size_t)(kMorseMaxWindow - 1 + kMorseTile) * 8;

/* receiver flags on the device: the header's two and the marks of the host */
static constexpr uint32_t kMorseOn = 0x1, kMorseFixed = 0x2;
static constexpr uint32_t kMorseFresh = 0x100;          /* create / reset: nothing carried is read, all of it is zero */
static constexpr uint32_t kMorseClear = 0x200;          /* RESTART, OFF -> ON: carried inputs zero, meter and timing afresh */
static constexpr uint32_t kMorseRekey = 0x400;          /* another keyer: meter and timing afresh, the inputs stay   */
static constexpr uint32_t kMorseMarks = kMorseFresh | kMorseClear | kMorseRekey;

struct MorseRx {
    int32_t keyer;
    uint32_t flags;
};

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
    const float *taps;        /* [nkeyers][morse_row(W)]                                                         */
    const MorseKeyer *keyers; /* [nkeyers]                                                                       */
    const MorseRx *rx;        /* [nrx]                                                                           */
    const MorseState *state;  /* [nrx] (not read where fresh)                                                    */
    MorseState *new_state;
    const float2 *hist;       /* [nrx][W - 1]: the inputs before the batch's first (not read where fresh or cleared) */
    float2 *new_hist;
    MorseParams par;
    int nrx;
    int nkeyers;
    int window;               /* W                                                                               */
};

/* k_morse: grid ceil(nrx / kMorseGroup) */
hipError_t launch_morse(const MorseArgs &a, hipStream_t s);

} // namespace pddc
#endif
