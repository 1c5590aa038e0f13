/*
 * ddc_mfsk.h -- internal launch interface between the MFSK decoder's host code (ddc_mfsk.cpp) and its gfx950 kernel
 * (ddc_mfsk.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The clock and the bounds both sides
 * share are in ddc_mfsk_bits.h.
 */
#ifndef PDDC_DDC_MFSK_H
#define PDDC_DDC_MFSK_H

#include "ddc_mfsk_bits.h"
#include "ddc_decoder_rx.h"

namespace pddc {

static constexpr int kMfskSamples = (int)kMfskBack + kDecTile;       /* per-sample results a wave's row holds */

/* LDS per receiver of the group, in 8-byte slots: the input row, then (b, r) of kMfskBack samples before the tile and of
 * the tile's, then their tone indices (best | runner-up << 8, 16 bits a sample) */
inline __host__ __device__ int mfsk_row_slots(int window) { return dec_in_slots(window) + kMfskSamples + kMfskSamples / 4; }
inline size_t mfsk_lds_bytes(int window) { return (size_t)kDecGroup * (size_t)mfsk_row_slots(window) * sizeof(float2); }
/* W = 256: 4 x (4088 + 3072 + 768) = 31712 bytes, half of the 64 KB a block may have */
static constexpr size_t kMfskLdsCap = (size_t)kDecGroup * (size_t)(kDecMaxWindow - 1 + kDecTile + kMfskSamples + kMfskSamples / 4) * 8;

static constexpr uint32_t kMfskReverse = 0x2;
/* the marks (no bit of its own): kDecClear is RESTART, OFF -> ON or another modem, all but the counter afresh */
static constexpr uint32_t kMfskMarks = kDecFresh | kDecClear;

/* what a receiver carries behind its inputs and per-sample results; read() reports from it */
struct MfskState {
    uint32_t symbols;         /* counter: never cleared by a restart                                             */
    uint32_t acc, skip;       /* the clock: skip = 1 while a late correction's borrowed wrap is still to come    */
    uint32_t tone_last;
    float q_last;
};

struct MfskArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    MfskSym *chars;           /* the symbol records [nrx][char_stride] (the skeleton's name for the records)     */
    long long char_stride;    /* >= the bound of pddc_mfsk_max_syms: the host refuses less                       */
    uint32_t *counts;         /* [nrx]                                                                           */
    float *best;              /* [nrx][best_stride] or NULL                                                      */
    long long best_stride;    /* >= n                                                                            */
    const float *taps;        /* [nbank][kMfskPairsMost][dec_row(W)][4]                                          */
    const MfskModem *bank;    /* [nbank]                                                                         */
    const DecRx *rx;          /* [nrx]                                                                           */
    const MfskState *state;   /* [nrx] (not read where fresh)                                                    */
    MfskState *new_state;
    const float2 *hist;       /* [nrx][mfsk_hist_slots(W)] (not read where fresh or cleared)                     */
    float2 *new_hist;
    int nrx;
    int nbank;
    int window;               /* W                                                                               */
};

/* k_mfsk: grid ceil(nrx / kDecGroup) */
hipError_t launch_mfsk(const MfskArgs &a, hipStream_t s);

} // namespace pddc
#endif
