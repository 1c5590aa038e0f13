/*
 * ddc_rxfilter.h -- internal launch interface between the receiver filter's host code (ddc_rxfilter.cpp) and its gfx950
 * kernel (ddc_rxfilter.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_RXFILTER_H
#define PDDC_DDC_RXFILTER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kRxfMaxRx = 1024;
static constexpr int kRxfMaxFilters = 64;
static constexpr int kRxfMaxTaps = 256;
static constexpr int kRxfThreads = 256;
static constexpr int kRxfGroup = 2;                     /* G: receivers per block                                  */
static constexpr int kRxfOut = 4;                       /* O: consecutive outputs per thread                       */
static constexpr int kRxfTile = kRxfThreads * kRxfOut;  /* TT: outputs per tile                                    */
static constexpr int kRxfStep = 8;                      /* inputs per pass of the tap loop, a multiple of O        */
/* a bank row on the device: kRxfPad zeros, the T taps, kRxfPad zeros -- the tap loop loads whole windows of h around
 * the taps it runs (it never runs a tap outside 0 .. T - 1) */
static constexpr int kRxfPad = 16;
inline int rxf_row(int taps) { return taps + 2 * kRxfPad; }

/* inputs staged before a tile's first output: T - 1 rounded up to a whole number of O */
inline __host__ __device__ int rxf_lead(int taps) { return (taps - 1 + kRxfOut - 1) / kRxfOut * kRxfOut; }
/* float2 slots of one of the O planes of a receiver's row in LDS: (lead + TT) / O rounded up to 16, plus 4 -- so that
 * the O planes start 4 slots apart modulo 16 (ddc_rxfilter.hip "LDS layout") */
inline __host__ __device__ int rxf_plane(int taps) { return ((rxf_lead(taps) + kRxfTile) / kRxfOut + 15) / 16 * 16 + 4; }
inline size_t rxf_lds_bytes(int taps) { return (size_t)kRxfGroup * kRxfOut * (size_t)rxf_plane(taps) * sizeof(float2); }
static constexpr size_t kRxfLdsCap = (size_t)kRxfGroup * kRxfOut * (((256 + kRxfTile) / kRxfOut + 15) / 16 * 16 + 4) * 8;

struct RxfRx {
    int32_t filter;           /* f_j, 0 <= f_j < nfilters                                                        */
    uint32_t fresh;           /* create / reset: the inputs before the batch's first are zero, the record not read */
};

struct RxfArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    float2 *out;              /* out[j * out_stride + i], i < n                                                  */
    long long out_stride;
    long long n;              /* values per receiver of this launch, > 0                                         */
    const float *bank;        /* [nfilters][rxf_row(T)]: tap t of filter f at f * rxf_row(T) + kRxfPad + t       */
    const RxfRx *rx;          /* [nrx]                                                                           */
    const float2 *state;      /* [nrx][T - 1]: the inputs before the batch's first (not read where fresh)        */
    float2 *new_state;        /* [nrx][T - 1] written by this launch                                             */
    int nrx;
    int nfilters;
    int taps;                 /* T                                                                               */
};

/* k_rxfilter: grid (ceil(n / kRxfTile), ceil(nrx / kRxfGroup)) */
hipError_t launch_rxfilter(const RxfArgs &a, hipStream_t s);

} // namespace pddc
#endif
