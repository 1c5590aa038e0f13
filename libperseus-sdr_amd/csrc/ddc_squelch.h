/*
 * ddc_squelch.h -- internal launch interface between the squelch's host code (ddc_squelch.cpp) and its gfx950 kernel
 * (ddc_squelch.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_SQUELCH_H
#define PDDC_DDC_SQUELCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kSquelchMaxRx = 1024;
static constexpr int kSquelchThreads = 256;
static constexpr int kSquelchGroup = 4;                 /* G: receivers per block                                  */
static constexpr int kSquelchTile = 256;                /* TT: samples per tile, one per thread and receiver       */
static constexpr int kSquelchMaxBlock = 4096;           /* B                                                       */
static constexpr int kSquelchMaxRamp = 65536;           /* R                                                       */
static constexpr int kSquelchMaxCount = 65535;          /* attack, hang                                            */
static constexpr uint32_t kSquelchGate = 1u, kSquelchRelative = 2u;   /* PDDC_SQL_GATE, PDDC_SQL_RELATIVE          */

/* one receiver as the kernel sees it */
struct SquelchRx {
    float open_thr, close_thr;
    uint32_t flags;     /* kSquelchGate | kSquelchRelative                                     */
    uint32_t c0;        /* the ramp counter at create / reset: 0 with GATE then, else R        */
};

/* what a receiver carries from one batch to the next */
struct SquelchState {
    float s;            /* the partial sum of the block under way   */
    float f;            /* floor                                    */
    float level, peak;
    uint32_t open, run, opens;
    uint32_t c;         /* ramp counter, 0 .. R                     */
};

struct SquelchArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n: complex float32                                    */
    long long z_stride;
    const float *a;           /* a[j * a_stride + i]                                                            */
    long long a_stride;
    float *out;               /* out[j * out_stride + i]; may be a itself (equal strides)                       */
    long long out_stride;
    float *level;             /* level[j * blk_stride + k], k < blocks completed in this launch, or null        */
    uint8_t *state;           /* the same shape, or null                                                        */
    long long blk_stride;
    long long n;              /* samples per receiver of this launch, > 0                                       */
    const SquelchRx *rx;      /* [nrx]                                                                          */
    int nrx;
    const SquelchState *old;  /* [nrx] as the batch before left it (not read when `fresh`)                      */
    SquelchState *new_state;  /* [nrx] written by this launch                                                   */
    uint32_t B, attack, hang, R;
    uint32_t ph0;             /* N mod B: where in its block the launch's first sample lies                     */
    uint32_t magic;           /* meter_magic(B)                                                                 */
    float invB, invR, up;
    uint32_t fresh;           /* the carried records are not read: the create values                            */
    uint32_t clear_peak;      /* the carried peak is taken as 0                                                 */
};

/* k_squelch: grid ceil(nrx / kSquelchGroup) */
hipError_t launch_squelch(const SquelchArgs &a, hipStream_t s);

} // namespace pddc
#endif
