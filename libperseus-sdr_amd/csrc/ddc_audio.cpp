/*
 * ddc_audio.cpp -- host side of the audio resampler (include/perseus_ddc.h, pddc_audio_*): the object, the position of
 * the next output, the output counts and the launch of a batch.  The kernel is in ddc_audio.hip.
 * What is carried per receiver (its last T - 1 inputs) lives on the device in two records, read and written in turn;
 * the input counter N, the next output's input n and remainder r, and the "fresh" mark (create, reset: the record is not
 * read, its values are zero) live here.  The prototype is uploaded once, at create.
 */
#include "ddc_stage.h"
#include "ddc_audio.h"

#include <cmath>
#include <numeric>

using namespace pddc;

typedef unsigned __int128 u128;

struct pddc_audio : StageBase {
    PDDC_LOCAL ~pddc_audio() = default;
    uint32_t L = 1, M = 1;                          /* reduced                                                    */
    int phases = 0, taps = 0;
    float scale = 32767.0f;
    DevBuf<float> proto;                            /* g[0 .. P T], g[P T] = 0                                    */
    Carried<float> state;                           /* [nrx][T - 1]                                               */
    bool fresh = true;
    uint64_t N = 0;                                 /* inputs per receiver since create / reset                   */
    uint64_t n = 0;                                 /* the next output's input, n >= N, and                       */
    uint32_t r = 0;                                 /* its remainder: k M = n L + r                               */
};

/* ceil(a L / M) */
static u128 audio_ceil(u128 a, uint32_t L, uint32_t M)
{
    return (a * L + (M - 1)) / M;
}

static bool audio_ratio_ok(uint32_t L, uint32_t M)
{
    return L >= 1 && L <= kAudioMaxRatio && M >= 1 && M <= kAudioMaxRatio;
}

/* outputs of the next `n` inputs, from the carried position: those k with n_k < N + n */
static u128 audio_due(const pddc_audio *a, size_t n)
{
    if ((u128)a->n >= (u128)a->N + n)
        return 0;
    const u128 avail = (u128)a->N + n - a->n;       /* a->n >= a->N, so 0 < avail <= n */
    /* (r + i M) div L < avail  <=>  i < (avail L - r) / M */
    return (avail * a->L - a->r + (a->M - 1)) / a->M;
}

extern "C" {

uint64_t pddc_audio_outputs(uint32_t L, uint32_t M, uint64_t inputs_before, size_t n)
{
    if (!audio_ratio_ok(L, M))
        return 0;
    const u128 c = audio_ceil((u128)inputs_before + n, L, M) - audio_ceil(inputs_before, L, M);
    return c > (u128)UINT64_MAX ? 0 : (uint64_t)c;
}

int pddc_audio_create(pddc_audio **out, int device, int nrx, uint32_t L, uint32_t M, int phases, int taps, const float *proto,
                      float scale)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kAudioMaxRx)
        return pddc_set_error_(PDDC_EINVAL, "audio: %d receivers (1 .. %d)", nrx, kAudioMaxRx);
    if (!audio_ratio_ok(L, M) || (uint64_t)M > (uint64_t)kAudioMaxDecim * L)
        return pddc_set_error_(PDDC_EINVAL, "audio: ratio %u / %u (1 .. 2^24 each, M <= %u L)", L, M, kAudioMaxDecim);
    if (phases < kAudioMinPhases || phases > kAudioMaxPhases || (phases & (phases - 1)) || taps < 1 || taps > kAudioMaxTaps ||
        phases * taps > kAudioMaxProto)
        return pddc_set_error_(PDDC_EINVAL, "audio: %d phases (a power of two, %d .. %d), %d taps (1 .. %d), product <= %d",
                               phases, kAudioMinPhases, kAudioMaxPhases, taps, kAudioMaxTaps, kAudioMaxProto);
    if (!proto)
        return pddc_set_error_(PDDC_EINVAL, "audio: null prototype");
    for (int i = 0; i < phases * taps; ++i)
        if (!std::isfinite(proto[i]))
            return pddc_set_error_(PDDC_EINVAL, "audio: prototype value %d is not finite", i);
    /* written so that a NaN fails it */
    if (!(scale > 0.0f && scale <= 3.0e38f))
        return pddc_set_error_(PDDC_EINVAL, "audio: scale %g (finite, > 0)", (double)scale);
    const uint32_t d = std::gcd(L, M);
    std::vector<float> g(proto, proto + (size_t)phases * (size_t)taps);
    g.push_back(0.0f);
    return stage_create(out, device, nrx, [&](pddc_audio &a) {
        a.L = L / d;
        a.M = M / d;
        a.phases = phases;
        a.taps = taps;
        a.scale = scale;
        PDDC_TRY(a.proto.alloc_copy(g));
        return a.state.alloc((size_t)nrx * (size_t)(taps > 1 ? taps - 1 : 1));
    });
}

int pddc_audio_destroy(pddc_audio *a) { return stage_destroy(a); }

int pddc_audio_reset(pddc_audio *a)
{
    PDDC_TRY(stage_quiesce(a));
    a->N = 0;
    a->n = 0;
    a->r = 0;
    a->fresh = true;
    return PDDC_OK;
}

int pddc_audio_next_outputs(const pddc_audio *a, size_t n, size_t *count)
{
    if (!a || !count)
        return null_argument();
    const u128 c = audio_due(a, n);
    if (c > (u128)(SIZE_MAX >> 1))
        return pddc_set_error_(PDDC_EINVAL, "audio: %zu inputs per receiver are too many for one batch", n);
    *count = (size_t)c;
    return PDDC_OK;
}

int pddc_audio_process(pddc_audio *a, const void *d_x, size_t n, size_t x_stride, void *d_f32, size_t f32_stride, void *d_i16,
                       size_t i16_stride, size_t *count, void *stream)
{
    if (!a)
        return null_argument();
    /* the kernel's 64-bit r + k M: the batch's inputs times L stay below 2^62 */
    if ((u128)n * a->L >> 62)
        return pddc_set_error_(PDDC_EINVAL, "audio: %zu inputs per receiver are too many for one batch", n);
    const size_t c = (size_t)audio_due(a, n);
    if (n)
        PDDC_TRY(device_ptr_ok(d_x, 4, "d_x"));
    if (c && !d_f32 && !d_i16)
        return pddc_set_error_(PDDC_EINVAL, "audio: one of d_f32 and d_i16 must be given");
    if (c && !(aligned_or_null(d_f32, 4) && aligned_or_null(d_i16, 2)))
        return pddc_set_error_(PDDC_EINVAL, "d_f32 must be a 4-byte, d_i16 a 2-byte aligned device pointer");
    if (n > x_stride || (d_f32 && c > f32_stride) || (d_i16 && c > i16_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "audio: %zu inputs and %zu outputs per receiver, x_stride %zu, f32_stride %zu, "
                               "i16_stride %zu", n, c, x_stride, f32_stride, i16_stride);
    if (!n) {
        if (count)
            *count = 0;
        return PDDC_OK;
    }
    PDDC_TRY(set_device(a->device));
    AudioArgs k{};
    k.x = static_cast<const float *>(d_x);
    k.x_stride = (long long)x_stride;
    k.f32 = static_cast<float *>(d_f32);
    k.f32_stride = (long long)f32_stride;
    k.i16 = static_cast<int16_t *>(d_i16);
    k.i16_stride = (long long)i16_stride;
    k.n = (long long)n;
    k.count = (long long)c;
    k.proto = a->proto.get();
    k.state = a->state.old();
    k.new_state = a->state.next();
    k.nrx = a->nrx;
    k.fresh = a->fresh ? 1 : 0;
    k.L = a->L;
    k.M = a->M;
    k.n0 = (uint32_t)(a->n - a->N);                 /* <= M / L: the output before it lay inside the stream */
    k.r0 = a->r;
    k.phases = a->phases;
    k.taps = a->taps;
    k.span = audio_span(a->L, a->M, a->taps);
    k.scale = a->scale;
    PDDC_HIP_TRY(launch_audio(k, (hipStream_t)stream));
    /* the launch was accepted: only now do the host-side counters move */
    const u128 v = (u128)a->r + (u128)c * a->M;
    a->n += (uint64_t)(v / a->L);
    a->r = (uint32_t)(v % a->L);
    a->N += n;
    a->state.turn();
    a->fresh = false;
    if (count)
        *count = c;
    return PDDC_OK;
}

} // extern "C"
