/*
 * ddc_psk.h -- internal launch interface between the PSK decoder's host code (ddc_psk.cpp) and its gfx950 kernel
 * (ddc_psk.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The clock, the framing and the bounds both
 * sides share are in ddc_psk_bits.h.
 */
#ifndef PDDC_DDC_PSK_H
#define PDDC_DDC_PSK_H

#include "ddc_psk_bits.h"
#include "ddc_decoder_rx.h"

namespace pddc {

static constexpr int kPskBack = 2 * (int)kPskQMost;     /* filter outputs kept in front of a tile: 2 q at the most */

/* LDS per receiver of the group, in float2: the input row, then kPskBack filter outputs and a tile of them */
inline __host__ __device__ int psk_row_slots(int window) { return dec_in_slots(window) + kPskBack + kDecTile; }
inline size_t psk_lds_bytes(int window) { return (size_t)kDecGroup * (size_t)psk_row_slots(window) * sizeof(float2); }
static constexpr size_t kPskLdsCap = (size_t)kDecGroup * (size_t)(kDecMaxWindow - 1 + kDecTile + kPskBack + kDecTile) * 8;

/* what a receiver carries in front of a batch, in float2: its last W - 1 inputs, then its last kPskBack filter outputs */
inline __host__ __device__ int psk_hist_slots(int window) { return window - 1 + kPskBack; }

/* the marks (no bit of its own beside kDecOn): kDecClear is RESTART, OFF -> ON or another modem, all but the counters afresh */
static constexpr uint32_t kPskMarks = kDecFresh | kDecClear;

/* what a receiver carries behind its inputs and filter outputs; read() reports from it */
struct PskState {
    PskFrame f;
    uint32_t acc;
    float vr, vi, pv;         /* the previous strobe's on-time output and its power                               */
    float d_last, x_last;
    uint32_t pad;
};

struct PskArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    PskChar *chars;           /* [nrx][char_stride]                                                              */
    long long char_stride;    /* >= the bound of pddc_psk_max_chars: the host refuses less                       */
    uint32_t *counts;         /* [nrx]                                                                           */
    float2 *sym;              /* [nrx][sym_stride] or NULL                                                       */
    long long sym_stride;     /* >= the bound of pddc_psk_max_syms                                               */
    uint32_t *nsym;           /* [nrx], with sym                                                                 */
    const float *taps;        /* [nbank][dec_row(W)]                                                             */
    const PskModem *bank;     /* [nbank]                                                                         */
    const DecRx *rx;          /* [nrx]                                                                           */
    const PskState *state;    /* [nrx] (not read where fresh)                                                    */
    PskState *new_state;
    const float2 *hist;       /* [nrx][psk_hist_slots(W)] (not read where fresh or cleared)                      */
    float2 *new_hist;
    int nrx;
    int nbank;
    int window;               /* W                                                                               */
};

/* k_psk: grid ceil(nrx / kDecGroup) */
hipError_t launch_psk(const PskArgs &a, hipStream_t s);

} // namespace pddc
#endif
