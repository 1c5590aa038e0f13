/*
 * ddc_blanker.h -- internal launch interface between the noise blanker's host code (ddc_blanker.cpp) and its gfx950
 * kernel (ddc_blanker.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_BLANKER_H
#define PDDC_DDC_BLANKER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kBlankerMaxRx = 1024;
static constexpr int kBlankerThreads = 256;
static constexpr int kBlankerGroup = 4;                 /* G: receivers per block                                  */
static constexpr int kBlankerTile = 256;                /* TT: samples per tile, one per thread and receiver       */
static constexpr int kBlankerMaxBlock = 4096;           /* B                                                       */
static constexpr int kBlankerMaxGuard = 128;            /* W                                                       */
static constexpr int kBlankerMaxRamp = 128;             /* R                                                       */
static constexpr int kBlankerMaxDelay = kBlankerMaxGuard + kBlankerMaxRamp;    /* D = W + R                        */
static constexpr int kBlankerCarryWords = 2 * kBlankerMaxDelay / 64;           /* trigger bits carried: 2 D <= 512 */
static constexpr int kBlankerMapWords = kBlankerCarryWords + kBlankerTile / 64;/* ... and a tile's behind them     */
static constexpr uint32_t kBlankerOn = 1u;              /* PDDC_NB_ON                                              */

/* one receiver as the kernel sees it */
struct BlankerRx {
    float thr;
    uint32_t flags;     /* kBlankerOn */
};

/* what a receiver carries from one batch to the next, beside its history and its trigger bits */
struct BlankerState {
    float s;            /* the partial sum of the block under way   */
    float ref;          /* the reference after the last whole block */
    uint32_t triggers, blanked;
};

struct BlankerArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n: complex float32                                    */
    long long z_stride;
    float2 *out;              /* out[j * out_stride + i]; never overlaps z                                      */
    long long out_stride;
    long long n;              /* samples per receiver of this launch, > 0                                       */
    const BlankerRx *rx;      /* [nrx]                                                                          */
    int nrx;
    const BlankerState *old;  /* [nrx] as the batch before left it (not read when `fresh`)                      */
    BlankerState *new_state;  /* [nrx] written by this launch                                                   */
    const float2 *old_hist;   /* [nrx][kBlankerMaxDelay]: entry i < D is input N - D + i (not read when `fresh`) */
    float2 *new_hist;
    const unsigned long long *old_bits;   /* [nrx][kBlankerCarryWords]: bit q is the trigger of input N - 512 + q */
    unsigned long long *new_bits;
    uint32_t B, W, D;
    uint32_t ph0;             /* N mod B: where in its block the launch's first sample lies                     */
    uint32_t magic;           /* meter_magic(B)                                                                 */
    float invB, invR1, beta, cap;
    uint32_t fresh;           /* nothing carried is read: the create values                                     */
};

/* k_blanker: grid ceil(nrx / kBlankerGroup) */
hipError_t launch_blanker(const BlankerArgs &a, hipStream_t s);

} // namespace pddc
#endif
