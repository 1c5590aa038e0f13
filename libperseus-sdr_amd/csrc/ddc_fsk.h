/*
 * ddc_fsk.h -- internal launch interface between the FSK decoder's host code (ddc_fsk.cpp) and its gfx950 kernel
 * (ddc_fsk.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_FSK_H
#define PDDC_DDC_FSK_H

#include "ddc_decoder_rx.h"

namespace pddc {

/* LDS per receiver of the group: the input row (float2), the tile's d (float), and 2 O 64-bit masks, the tile's
 * decisions and rising edges */
inline size_t fsk_lds_bytes(int window)
{
    return (size_t)kDecGroup * ((size_t)dec_in_slots(window) * sizeof(float2) + (size_t)kDecTile * sizeof(float) + 2 * kDecOut * 8);
}
static constexpr size_t kFskLdsCap =
    (size_t)kDecGroup * ((size_t)(kDecMaxWindow - 1 + kDecTile) * 8 + (size_t)kDecTile * 4 + 2 * kDecOut * 8);

/* receiver flags beside kDecOn and the marks: kDecClear also means IDLE and prev = mark */
static constexpr uint32_t kFskReverse = 0x2;
static constexpr uint32_t kFskIdle = kDecThird;         /* another modem: IDLE, a character in progress is dropped  */
static constexpr uint32_t kFskMarks = kDecFresh | kDecClear | kFskIdle;

static constexpr uint32_t kFskStIdle = 0, kFskStStart = 1, kFskStData = 2, kFskStStop = 3;

struct FskModem {
    uint32_t inc;             /* bit phase per sample, 1 .. 2^30                                                 */
    uint32_t nbits;           /* 5 .. 8                                                                          */
};

/* what the start-stop receiver carries; read() reports from it */
struct FskState {
    uint64_t start;           /* sample index of the edge of the character in progress                           */
    uint32_t state;           /* kFskSt*                                                                         */
    uint32_t acc;
    uint32_t k;
    uint32_t shift;
    float qmin;
    uint32_t prev;            /* the previous sample's `space`                                                   */
    uint32_t chars, framing, false_starts;
    float d_last;
};

/* pddc_fsk_char, 16 bytes */
struct FskChar {
    uint64_t start;
    uint16_t code;
    uint16_t flags;
    float quality;
};

struct FskArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    FskChar *chars;           /* [nrx][char_stride]                                                              */
    long long char_stride;    /* >= the bound of pddc_fsk_max_chars: the host refuses less                       */
    uint32_t *counts;         /* [nrx]                                                                           */
    float *d;                 /* [nrx][d_stride] or NULL                                                         */
    long long d_stride;
    const float *taps;        /* [nbank][dec_row(W)][4]                                                          */
    const FskModem *bank;     /* [nbank]                                                                         */
    const DecRx *rx;          /* [nrx]                                                                           */
    const FskState *state;    /* [nrx] (not read where fresh)                                                    */
    FskState *new_state;
    const float2 *hist;       /* [nrx][W - 1]: the inputs before the batch's first (not read where fresh or cleared) */
    float2 *new_hist;
    int nrx;
    int nbank;
    int window;               /* W                                                                               */
};

/* k_fsk: grid ceil(nrx / kDecGroup) */
hipError_t launch_fsk(const FskArgs &a, hipStream_t s);

} // namespace pddc
#endif
