/*
 * ddc_denoise.h -- internal launch interface between the spectral noise reduction's host code (ddc_denoise.cpp) and its
 * gfx950 kernel (ddc_denoise.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_DENOISE_H
#define PDDC_DDC_DENOISE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kDenoiseMaxRx = 1024;
static constexpr uint32_t kDenoiseOff = 0u, kDenoiseNr = 1u, kDenoiseModes = 2u;   /* PDDC_DENOISE_OFF, _NR            */
static constexpr uint32_t kDenoiseRestart = 1u, kDenoiseHold = 2u;                 /* PDDC_DENOISE_RESTART, _HOLD      */
/* a block walks its receivers' frames one after the other: a block pass is one frame */
static constexpr int kDenoiseTileFrames = 1;

/* one receiver as the kernel sees it */
struct DenoiseRx {
    uint32_t mode;      /* kDenoiseOff, kDenoiseNr                                                                     */
    float beta, gmin, alpha;
    uint32_t flags;     /* kDenoiseRestart: the first frame this launch completes is a first frame (the mark create and
                         * reset leave as well); kDenoiseHold: S and N stay                                             */
};

/* The launch works on the receiver's series from the start of the oldest incomplete frame before the batch: index
 * v < clen is the carried sample v (zeros when `fresh`: x[m] = 0 for m < 0), index v >= clen is x[j][v - clen].  New frame
 * f (0 <= f < nseg) begins at v = f hop and is frame q0 + f of the series.  Ring slot of y[m]: m mod nfft. */
struct DenoiseArgs {
    const float *x;           /* x[j * x_stride + i], i < n                                                           */
    long long x_stride;
    float *out;               /* out[j * out_stride + i]                                                              */
    long long out_stride;
    long long n;              /* samples per receiver of this launch, > 0                                             */
    const DenoiseRx *rx;      /* [nrx]                                                                                */
    int nrx;
    int hop;
    float smooth, up, down, nmin, eps;
    const float *window;      /* [nfft]                                                                               */
    const float *twiddles;    /* spectrum_build_twiddles(nfft)                                                        */
    const float *old_carry;   /* [nrx][nfft]: the first clen are read (not when fresh)                                */
    float *new_carry;         /* ...: the first new_clen are written                                                  */
    const float *old_ola;     /* [nrx][nfft]: the ring of partial overlap sums (read when nseg > 0 and not fresh)     */
    float *new_ola;           /* ...: written when nseg > 0                                                           */
    const float *old_pend;    /* [nrx][hop]: y of the last frame's finished hop, entry i is out index q0 hop + i      */
    float *new_pend;          /* ...: entry i is out index (q0 + nseg) hop + i                                        */
    const float *old_sna;     /* [3][nrx][nfft/2 + 1]: S, N, A (read when nseg > 0, not of a receiver at a first frame) */
    float *new_sna;           /* ...: written when nseg > 0                                                           */
    int clen, new_clen;       /* nfft - hop <= .. < nfft                                                              */
    int pos;                  /* samples since the last frame boundary before the batch: m0 - q0 hop, < hop           */
    long long q0;             /* frames complete before this launch                                                   */
    long long nseg;           /* frames this launch completes                                                         */
    uint32_t fresh;           /* nothing carried is read: no sample since create / reset                              */
};

/* k_denoise<nfft>: a receiver is a group of nfft / 16 (at nfft = 512 of nfft / 8) threads; four receivers per block at
 * nfft = 256, one otherwise */
hipError_t launch_denoise(int nfft, const DenoiseArgs &a, hipStream_t s);

} // namespace pddc
#endif
