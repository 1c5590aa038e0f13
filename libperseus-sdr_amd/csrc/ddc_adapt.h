/*
 * ddc_adapt.h -- internal launch interface between the adaptive filter's host code (ddc_adapt.cpp) and its gfx950 kernel
 * (ddc_adapt.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_ADAPT_H
#define PDDC_DDC_ADAPT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kAdaptMaxRx = 1024;
static constexpr int kAdaptMinTaps = 16, kAdaptMaxTaps = 128;  /* T: 16, 32, 64, 128                                */
static constexpr int kAdaptMaxDelay = 256;                     /* D                                                 */
static constexpr int kAdaptThreads = 64;                       /* one wave per block                                */
static constexpr int kAdaptTile = 256;                         /* TT: samples per tile                              */
static constexpr int kAdaptHist = 384;                         /* room for the D + T - 1 <= 383 samples before a tile */
/* lanes per receiver, at most: 64 = one receiver per wave at T >= 64 (T = 32 two, T = 16 four), 16 = four receivers per
 * wave at every T.  The same bits either way; NOTEBOOK.md has the measurement that chose.  (The macro is for a same-box
 * A/B build of the other layout, tools/ab.sh build lanes16:"-DPDDC_ADAPT_LANES=16") */
#ifndef PDDC_ADAPT_LANES
#define PDDC_ADAPT_LANES 64
#endif
static constexpr int kAdaptLanes = PDDC_ADAPT_LANES;
static_assert(kAdaptLanes == 16 || kAdaptLanes == 32 || kAdaptLanes == 64, "a receiver's lanes: 16, 32 or 64");
static constexpr uint32_t kAdaptOff = 0u, kAdaptNr = 1u, kAdaptNotch = 2u, kAdaptModes = 3u;   /* PDDC_ADAPT_OFF, _NR, _NOTCH */
static constexpr uint32_t kAdaptRestart = 1u;                  /* PDDC_ADAPT_RESTART                                */

constexpr int adapt_lanes(int taps) { return taps < kAdaptLanes ? taps : kAdaptLanes; }

/* one receiver as the kernel sees it */
struct AdaptRx {
    uint32_t mode;      /* kAdaptOff, kAdaptNr, kAdaptNotch                                    */
    float mu;
    float lam;          /* 1.0f - leak                                                         */
    uint32_t flags;     /* kAdaptRestart: this launch takes the carried weights as 0           */
};

struct AdaptArgs {
    const float *a;           /* a[j * a_stride + i], i < n                                                     */
    long long a_stride;
    float *out;               /* out[j * out_stride + i]; may be a itself (equal strides)                       */
    long long out_stride;
    long long n;              /* samples per receiver of this launch, > 0                                       */
    const AdaptRx *rx;        /* [nrx]                                                                          */
    int nrx;
    int T, D;
    float eps;
    const float *old_w;       /* [nrx][T] weights as the batch before left them (not read when `fresh`)         */
    const float *old_h;       /* [nrx][D + T - 1]: entry q is the input q + 1 samples before this launch's first */
    float *new_w, *new_h;     /* the same, written by this launch                                               */
    uint32_t fresh;           /* the carried records are not read: weights and inputs are 0                     */
};

/* k_adapt: grid ceil(nrx / (64 / adapt_lanes(T))) blocks of one wave */
hipError_t launch_adapt(const AdaptArgs &a, hipStream_t s);

} // namespace pddc
#endif
