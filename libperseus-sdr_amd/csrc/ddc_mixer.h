/*
 * ddc_mixer.h -- internal launch interface between the mixer's host code (ddc_mixer.cpp) and its gfx950 kernels
 * (ddc_mixer.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_MIXER_H
#define PDDC_DDC_MIXER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kMixMaxRx = 1024;
static constexpr int kMixMaxBus = 8;                    /* Q                                                       */
static constexpr int kMixChunk = 32;                    /* C: active receivers per chunk sum (pddc_mixer_chunk)    */
static constexpr int kMixTile = 64;                     /* samples per tile: one per lane of a wave                */
static constexpr int kMixMaxWaves = 16;                 /* waves of a k_mix block; chunk m runs on wave m mod waves */
static constexpr int kMixMaxRamp = 65536;               /* R                                                       */
static constexpr int kMixMinBlock = 8, kMixMaxBlock = 4096;   /* Lb                                                */
static constexpr int kMixMaxPiece = 32768;              /* samples of one launch: process() cuts a batch into pieces */
static constexpr int kMixMaxTiles = kMixMaxPiece / kMixTile;
static constexpr int kMixBusThreads = 1024;             /* k_mix_bus: one block per bus                            */
/* limiter blocks one launch can see: the carried samples (< 2 Lb) and a piece, in blocks of Lb >= 8 */
static constexpr int kMixMaxBlocks = (2 * kMixMinBlock + kMixMaxPiece) / kMixMinBlock;
static constexpr uint32_t kMixLimit = 1u;               /* PDDC_MIX_LIMIT                                          */

/* one ACTIVE receiver as k_mix sees it; the table holds them in ascending j, so its index is p */
struct MixRx {
    uint32_t j;                 /* the receiver's row of a                                                        */
    uint32_t c;                 /* its ramp counter in front of the launch's first sample, 0 .. R                 */
    float from[kMixMaxBus];     /* the gains the ramp leaves (buses >= Q: 0)                                      */
    float to[kMixMaxBus];       /* ... and reaches                                                                */
};

/* what a bus carries from one launch to the next, beside its held samples */
struct MixBus {
    float peak;                 /* fmaxf of |y|                                                                   */
    float gain;                 /* the latest E                                                                   */
    float min_gain;             /* the smallest E                                                                 */
    uint32_t pad;
};

struct MixArgs {
    const float *a;             /* a[j * a_stride + i], i < n                                                     */
    long long a_stride;
    int n;                      /* samples of this launch, 1 .. kMixMaxPiece                                      */
    const MixRx *rx;            /* [nact]                                                                         */
    int nact;                   /* active receivers, 0 .. kMixMaxRx                                               */
    int Q;
    uint32_t R;
    float invR;
    float *y;                   /* limiter: y[q * y_stride + i], the bus sums for k_mix_bus; else null            */
    long long y_stride;
    float *f32;                 /* no limiter: f32[q * f32_stride + i] or null                                    */
    long long f32_stride;
    int16_t *i16;               /* no limiter: i16[i * Q + q] or null                                             */
    float scale;
    float *tile_peak;           /* [tiles][kMixMaxBus]: fmaxf of |y| over the tile                                */
};

struct MixBusArgs {
    const float *y;             /* as k_mix left it (limiter only)                                                */
    long long y_stride;
    int n;
    const float *tile_peak;
    int tiles;
    int Q;
    const MixBus *old;          /* [Q], not read when `fresh`                                                     */
    MixBus *next;
    const float *held_old;      /* [Q][2 Lb]: the first `held` are samples not written yet (limiter only)         */
    float *held_next;
    int held;                   /* 0 .. 2 Lb - 1                                                                  */
    int write_blocks;           /* limiter blocks this launch writes: max(0, (held + n) / Lb - 1)                 */
    uint32_t fresh, clear, limit;
    int Lb;
    float invLb, ceil, rel;
    float *f32;                 /* f32[q * f32_stride + k], k < write_blocks Lb, or null                          */
    long long f32_stride;
    int16_t *i16;               /* i16[k * Q + q] or null                                                         */
    float scale;
};

/* k_mix: grid = tiles of kMixTile samples, block = 64 x min(kMixMaxWaves, max(1, chunks)) threads */
hipError_t launch_mix(const MixArgs &a, hipStream_t s);
/* k_mix_bus: grid = Q blocks of kMixBusThreads */
hipError_t launch_mix_bus(const MixBusArgs &a, hipStream_t s);

} // namespace pddc
#endif
