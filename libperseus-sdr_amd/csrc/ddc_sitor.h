/*
 * ddc_sitor.h -- internal launch interface between the SITOR decoder's host code (ddc_sitor.cpp) and its gfx950 kernel
 * (ddc_sitor.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The clock, the framing and the bounds both
 * sides share are in ddc_sitor_bits.h.
 */
#ifndef PDDC_DDC_SITOR_H
#define PDDC_DDC_SITOR_H

#include "ddc_sitor_bits.h"
#include "ddc_decoder_rx.h"

namespace pddc {

/* LDS per receiver of the group: the input row (float2), the tile's d (float), and 2 O 64-bit masks, the tile's
 * decisions and transitions */
inline size_t sitor_lds_bytes(int window)
{
    return (size_t)kDecGroup * ((size_t)dec_in_slots(window) * sizeof(float2) + (size_t)kDecTile * sizeof(float) + 2 * kDecOut * 8);
}
static constexpr size_t kSitorLdsCap =
    (size_t)kDecGroup * ((size_t)(kDecMaxWindow - 1 + kDecTile) * 8 + (size_t)kDecTile * 4 + 2 * kDecOut * 8);

/* receiver flags beside kDecOn and the marks: kDecClear also means acc = 0, prev = mark and the framing as at create */
static constexpr uint32_t kSitorReverse = 0x2;
static constexpr uint32_t kSitorReframe = kDecThird;    /* another modem: the framing as at create, acc and prev stay */
static constexpr uint32_t kSitorMarks = kDecFresh | kDecClear | kSitorReframe;

/* what a receiver carries behind its inputs; read() reports from it */
struct SitorState {
    SitorFrame f;
    uint32_t acc;
    uint32_t prev;            /* the previous sample's `space`                                                   */
    float d_last;
    uint32_t pad;
};

struct SitorArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    SitorChar *chars;         /* [nrx][char_stride]                                                              */
    long long char_stride;    /* >= the bound of pddc_sitor_max_chars: the host refuses less                     */
    uint32_t *counts;         /* [nrx]                                                                           */
    float *soft;              /* [nrx][soft_stride] or NULL                                                      */
    long long soft_stride;    /* >= the bound of pddc_sitor_max_syms                                             */
    uint32_t *nsoft;          /* [nrx], with soft                                                                */
    const float *taps;        /* [nbank][dec_row(W)][4]                                                          */
    const SitorModem *bank;   /* [nbank]                                                                         */
    const DecRx *rx;          /* [nrx]                                                                           */
    const SitorState *state;  /* [nrx] (not read where fresh)                                                    */
    SitorState *new_state;
    const float2 *hist;       /* [nrx][W - 1]: the inputs before the batch's first (not read where fresh or cleared) */
    float2 *new_hist;
    int nrx;
    int nbank;
    int window;               /* W                                                                               */
};

/* k_sitor: grid ceil(nrx / kDecGroup) */
hipError_t launch_sitor(const SitorArgs &a, hipStream_t s);

} // namespace pddc
#endif
