/*
 * ddc_carrier.h -- internal launch interface between the carrier stage's host code (ddc_carrier.cpp) and its gfx950
 * kernel (ddc_carrier.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_CARRIER_H
#define PDDC_DDC_CARRIER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kCarrierMaxRx = 1024;
static constexpr int kCarrierThreads = 256;
static constexpr int kCarrierGroup = 16;                /* G: receivers per block, one per lane of the recursion wave */
static constexpr int kCarrierTile = 128;                /* TT: outputs per tile                                        */
static constexpr int kCarrierMaxTaps = 255;             /* L                                                           */
static constexpr int kCarrierTapSlots = 256;            /* the device's tap array: L taps, then zeros                  */
static constexpr int kCarrierRing = 3 * kCarrierTile;   /* columns of a tile row: the tile and the 2 TT >= L - 1 before */
static constexpr int kCarrierPad = 4;                   /* row stride 388 dwords = 4 mod 64 (ddc_carrier.hip)          */
static constexpr uint32_t kCarrierOff = 0u, kCarrierDsb = 1u, kCarrierUsb = 2u, kCarrierLsb = 3u, kCarrierModes = 4u;
static constexpr uint32_t kCarrierFresh = 1u;           /* the carried values are not read: the create values          */

/* one receiver as the kernel sees it */
struct CarrierRx {
    uint32_t mode;
    float kp, ki;
    uint32_t flags;     /* kCarrierFresh */
};

/* what a receiver carries from one batch to the next, beside its L - 1 values of w */
struct CarrierState {
    uint32_t theta;     /* theta[m+1] behind the last output m */
    float v, q;
    uint32_t pad;
};

struct CarrierArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n: complex float32                                    */
    long long z_stride;
    float2 *u;                /* u[j * u_stride + i]; may be z itself (equal strides)                           */
    long long u_stride;
    long long n;              /* outputs per receiver of this launch, > 0                                       */
    const CarrierRx *rx;      /* [nrx]                                                                          */
    int nrx;
    const CarrierState *old;  /* [nrx] as the batch before left it (not read where kCarrierFresh)               */
    CarrierState *new_state;  /* [nrx] written by this launch                                                   */
    const float2 *old_hist;   /* [nrx][L - 1]: w of the L - 1 outputs before this launch, the latest last       */
    float2 *new_hist;
    const float *taps;        /* [kCarrierTapSlots]                                                             */
    int L;
    float vmax, gamma;
};

/* k_carrier: grid ceil(nrx / kCarrierGroup) */
hipError_t launch_carrier(const CarrierArgs &a, hipStream_t s);

} // namespace pddc
#endif
