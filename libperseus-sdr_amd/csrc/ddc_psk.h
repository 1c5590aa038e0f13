/*
 * ddc_psk.h -- internal launch interface between the PSK decoder's host code (ddc_psk.cpp) and its gfx950 kernel
 * (ddc_psk.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The clock, the framing and the bounds both
 * sides share are in ddc_psk_bits.h.
 */
#ifndef PDDC_DDC_PSK_H
#define PDDC_DDC_PSK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_psk_bits.h"

namespace pddc {

static constexpr int kPskMaxRx = 1024;
static constexpr int kPskMaxModems = 16;
static constexpr int kPskMaxWindow = 256;
static constexpr int kPskGroup = 4;                     /* G: receivers per block, one wave each                   */
static constexpr int kPskThreads = 64 * kPskGroup;
static constexpr int kPskOut = 4;                       /* O: outputs per lane and tile, 64 apart                  */
static constexpr int kPskTile = 64 * kPskOut;           /* TT: samples per tile, tiles aligned to the batch        */
static constexpr int kPskStep = 8;                      /* taps per pass of the tap loop                           */
static constexpr int kPskBack = 2 * (int)kPskQMost;     /* filter outputs kept in front of a tile: 2 q at the most */
/* a modem's taps on the device: W real taps rounded up to a whole number of passes, zeros behind the W-th */
inline __host__ __device__ int psk_row(int window) { return (window + kPskStep - 1) / kPskStep * kPskStep; }

/* LDS per receiver of the group, in float2: W - 1 carried inputs and a tile of them, then kPskBack filter outputs and a
 * tile of them */
inline __host__ __device__ int psk_in_slots(int window) { return window - 1 + kPskTile; }
inline __host__ __device__ int psk_row_slots(int window) { return psk_in_slots(window) + kPskBack + kPskTile; }
inline size_t psk_lds_bytes(int window) { return (size_t)kPskGroup * (size_t)psk_row_slots(window) * sizeof(float2); }
static constexpr size_t kPskLdsCap = (size_t)kPskGroup * (size_t)(kPskMaxWindow - 1 + kPskTile + kPskBack + kPskTile) * 8;

/* what a receiver carries in front of a batch, in float2: its last W - 1 inputs, then its last kPskBack filter outputs */
inline __host__ __device__ int psk_hist_slots(int window) { return window - 1 + kPskBack; }

/* receiver flags on the device: the header's and the marks of the host */
static constexpr uint32_t kPskOn = 0x1;
static constexpr uint32_t kPskFresh = 0x100;            /* create / reset: nothing carried is read, all of it is zero */
static constexpr uint32_t kPskClear = 0x200;            /* RESTART, OFF -> ON, another modem: all but the counters afresh */
static constexpr uint32_t kPskMarks = kPskFresh | kPskClear;

struct PskRx {
    int32_t modem;
    uint32_t flags;
};

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
    const float *taps;        /* [nmodems][psk_row(W)]                                                           */
    const PskModem *modems;   /* [nmodems]                                                                       */
    const PskRx *rx;          /* [nrx]                                                                           */
    const PskState *state;    /* [nrx] (not read where fresh)                                                    */
    PskState *new_state;
    const float2 *hist;       /* [nrx][psk_hist_slots(W)] (not read where fresh or cleared)                      */
    float2 *new_hist;
    int nrx;
    int nmodems;
    int window;               /* W                                                                               */
};

/* k_psk: grid ceil(nrx / kPskGroup) */
hipError_t launch_psk(const PskArgs &a, hipStream_t s);

} // namespace pddc
#endif
