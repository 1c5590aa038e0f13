/*
 * ddc_spectrum.h -- internal launch interface between the panorama's host code (ddc_spectrum.cpp) and its gfx950
 * kernels (ddc_spectrum.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_SPECTRUM_H
#define PDDC_DDC_SPECTRUM_H

#include "ddc_packed.h"

namespace pddc {

static constexpr int kSpecMinN = 1024, kSpecMaxN = 8192;

/* floats (re, im pairs count as two) of the twiddle table of size n (the panorama's sizes, and 256 and 512 for the
 * scope, ddc_scope.hip): per pass after the first, [r - 1][k] for
 * r = 1 .. R-1, k = 0 .. Ns-1, holding exp(-2 pi i r k / (Ns R)) */
int spectrum_twiddle_len(int nfft);
/* fills tw[spectrum_twiddle_len(nfft)]: cos / sin in double, rounded once */
void spectrum_build_twiddles(int nfft, float *tw);
/* the most blocks a k_spectrum launch of this size uses (rows of the partial-sum array) */
int spectrum_max_blocks(int nfft, int ncu);

struct SpectrumArgs {
    PackedStream in;          /* tail-then-batch (ddc_packed.h); the tail is shorter than nfft          */
    long long nseg;           /* segments this launch completes; segment j starts at sample j*hop of tail-then-batch */
    int hop;
    const float *window;      /* [nfft]                                                                 */
    const float *twiddles;    /* spectrum_build_twiddles                                                */
    float *part_sum;          /* [gridDim.x][nfft]                                                      */
    float *part_peak;         /* the same, or nullptr                                                   */
};

/* k_spectrum<nfft, peak>: `blocks` <= min(nseg, spectrum_max_blocks); block b takes segments b, b + blocks, ... */
hipError_t launch_spectrum(int nfft, const SpectrumArgs &a, int blocks, hipStream_t s);

struct SpectrumFoldArgs {
    const float *part_sum, *part_peak;   /* [nparts][nfft]; nparts == 0: nothing to add                  */
    int nparts, nfft;
    double *acc_sum;                     /* [nfft] running sums                                          */
    float *acc_peak;                     /* [nfft] or nullptr                                            */
    PackedCarryArgs carry;               /* the carried tail for the NEXT batch (ddc_packed.h)           */
};
/* k_spectrum_fold: the second pass -- partial sums into the running sums (double, partials in ascending order), and the
 * tail carried on.  One launch.                                                                                */
hipError_t launch_spectrum_fold(const SpectrumFoldArgs &a, hipStream_t s);

/* k_spectrum_read: running sums -> float32; clear != 0 zeroes them afterwards */
hipError_t launch_spectrum_read(int nfft, double *acc_sum, float *acc_peak, float *d_sum, float *d_peak, int clear,
                                hipStream_t s);

} // namespace pddc
#endif
