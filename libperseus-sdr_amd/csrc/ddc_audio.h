/*
 * ddc_audio.h -- internal launch interface between the audio resampler's host code (ddc_audio.cpp) and its gfx950 kernel
 * (ddc_audio.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_AUDIO_H
#define PDDC_DDC_AUDIO_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kAudioMaxRx = 1024;
static constexpr int kAudioThreads = 256;
static constexpr int kAudioGroup = 4;                   /* G: receivers per block                                  */
static constexpr int kAudioTile = 256;                  /* outputs per tile, one per thread and receiver           */
static constexpr uint32_t kAudioMaxRatio = 1u << 24;    /* 1 <= L, M <= 2^24                                       */
static constexpr uint32_t kAudioMaxDecim = 16;          /* M <= 16 L                                               */
static constexpr int kAudioMinPhases = 32, kAudioMaxPhases = 1024, kAudioMaxTaps = 64, kAudioMaxProto = 8192;

/* floats of a tile's input span per receiver: the inputs n_first - (T - 1) .. n_last of its <= 256 outputs, with
 * n_last - n_first <= floor(255 M / L) + 1 (the two remainders may carry); at most 255 * 16 + 1 + 64 = 4145 */
inline int audio_span(uint32_t L, uint32_t M, int taps)
{
    return (int)((uint64_t)(kAudioTile - 1) * M / L) + 1 + taps;
}
static constexpr int kAudioMaxSpan = (kAudioTile - 1) * (int)kAudioMaxDecim + 1 + kAudioMaxTaps;
/* dynamic LDS of a block in floats: g[0 .. P T] rounded up to whole float4, then G rows of `span` */
inline size_t audio_lds_floats(int phases, int taps, int span)
{
    return (size_t)((phases * taps + 1 + 3) & ~3) + (size_t)kAudioGroup * (size_t)span;
}
static constexpr size_t kAudioLdsCap = ((size_t)kAudioMaxProto + 4 + (size_t)kAudioGroup * kAudioMaxSpan) * sizeof(float);

struct AudioArgs {
    const float *x;           /* x[j * x_stride + i], i < n: real float32                                        */
    long long x_stride;
    float *f32;               /* f32[j * f32_stride + k], k < count; or NULL                                     */
    long long f32_stride;
    int16_t *i16;             /* i16[j * i16_stride + k], k < count; or NULL                                     */
    long long i16_stride;
    long long n;              /* inputs per receiver of this launch, > 0                                         */
    long long count;          /* outputs per receiver of this launch, >= 0                                       */
    const float *proto;       /* g[0 .. P T], g[P T] = 0                                                         */
    const float *state;       /* [nrx][T - 1]: the inputs before the batch's first (not read where `fresh`)      */
    float *new_state;         /* [nrx][T - 1] written by this launch                                             */
    int nrx;
    int fresh;                /* create / reset: the inputs before the batch's first are zero                    */
    uint32_t L, M;            /* reduced                                                                         */
    uint32_t n0, r0;          /* the launch's first output: at input n0 of the batch (<= M / L), r0 < L          */
    int phases, taps;         /* P, T                                                                            */
    int span;                 /* audio_span(L, M, T)                                                             */
    float scale;
};

/* k_audio: grid (max(1, ceil(count / kAudioTile)), ceil(nrx / kAudioGroup)) */
hipError_t launch_audio(const AudioArgs &a, hipStream_t s);

} // namespace pddc
#endif
