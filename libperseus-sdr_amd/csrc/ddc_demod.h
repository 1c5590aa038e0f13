/*
 * ddc_demod.h -- internal launch interface between the demodulator's host code (ddc_demod.cpp) and its gfx950 kernel
 * (ddc_demod.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_DEMOD_H
#define PDDC_DDC_DEMOD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kDemodMaxRx = 1024;
static constexpr int kDemodThreads = 256;
static constexpr int kDemodGroup = 4;                   /* G: receivers per block                                  */
static constexpr int kDemodTile = 256;                  /* TT: outputs per tile, one per thread and receiver       */
static constexpr int kDemodPad = 4;                     /* a tile row is TT + 4 floats: rows stay 16-byte aligned  */
static constexpr uint32_t kDemodModes = 3;              /* PDDC_DEMOD_AM, _FM, _SSB = 0, 1, 2                      */
static constexpr uint32_t kDemodDc = 1u, kDemodAgc = 2u;/* PDDC_DEMOD_DCBLOCK, PDDC_DEMOD_AGC                      */
static constexpr uint32_t kDemodFresh = 0x80000000u;    /* internal: the carried record is not read, z d y e = 0   */

/* one receiver as the kernel sees it */
struct DemodRx {
    uint32_t mode;
    uint32_t beta;      /* SSB: theta[m] = beta m + psi (mod 2^32) */
    uint32_t psi;
    uint32_t flags;     /* kDemodDc | kDemodAgc | kDemodFresh       */
};

/* what a receiver carries from one batch to the next: the values at the batch's last output */
struct DemodState {
    float zx, zy;
    float d, y, e;
    float pad[3];
};

struct DemodArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n: complex float32                                    */
    long long z_stride;
    float *out;               /* out[j * out_stride + i]                                                        */
    long long out_stride;
    long long n;              /* outputs per receiver of this launch, > 0                                       */
    const DemodRx *rx;        /* [nrx]                                                                          */
    int nrx;
    const DemodState *state;  /* [nrx] as the batch before left it (not read where kDemodFresh is set)          */
    DemodState *new_state;    /* [nrx] written by this launch                                                   */
    uint32_t m0;              /* the launch's first output is m = m0 (mod 2^32)                                 */
    float rho, lambda, target, gmax;
    long long run;            /* a group without a post stage is cut into runs of this many outputs, one block
                                 each; a multiple of kDemodTile.  A group with one is walked by its block x = 0  */
};

/* k_demod: grid (ceil(n / run), ceil(nrx / kDemodGroup)) */
hipError_t launch_demod(const DemodArgs &a, hipStream_t s);

} // namespace pddc
#endif
