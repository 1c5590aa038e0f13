/*
 * ddc_audio.hip -- the audio resampler: every receiver's real series at L/M times its rate, float32 and / or saturated
 * int16 PCM (gfx950 only).
 *
 *   k_audio   per receiver j and output k of the launch: v = r0 + k M (64 bits), n = n0 + v div L, r = v mod L;
 *             u = r P, q = u div L, alpha = float(u mod L) / float(L); then over t = 0 .. T-1 ascending
 *             w = fmaf(alpha, g[t P + q + 1] - g[t P + q], g[t P + q]), acc = fmaf(w, x[n - t], acc); y = acc;
 *             PCM p = clamp(rintf(y scale), -32768, 32767), NaN -> 0.  DESIGN.md 8 has the definition.
 *
 * Walk: every output is independent.  A block takes a tile of 256 consecutive outputs of G = 4 consecutive receivers:
 *   1. all threads stage g[0 .. P T] (the trailing zero included) into LDS, and for each receiver of the group the
 *      tile's input span n_first - (T - 1) .. n_last: consecutive threads, consecutive inputs, coalesced 4-byte loads;
 *      an input before the batch's first comes from the carried record (zero after create / reset), a receiver the
 *      group does not have stages zeros.
 *   2. thread i takes output i of the tile: position, q and alpha once (they are common to the receivers), then the tap
 *      loop with one w per tap and G accumulators, x from the G rows in LDS.
 *   3. one coalesced 4-byte float store and / or 2-byte int16 store per receiver, whichever pointers are given.
 *   The blocks of the last tile also write their receivers' new carried record, the last T - 1 values of
 *   [old record | batch], from global memory: a batch shorter than T - 1 keeps part of the old record.  A batch that
 *   gives no output (M > L) is one tile of 0 outputs, which does only that.
 * The reads of g are indexed by q, which differs from lane to lane: they are scattered across the LDS banks.
 * Bits: one thread makes each value with one operation sequence (contraction is off in this file, every fmaf is
 * spelled); the position arithmetic is exact integers; so y_j[k] does not depend on the batch cut, nrx, j's index, the
 * other receivers, the strides or the tile a value falls into.  No atomics, no scratch.
 * Bounds: x is indexed by receivers < nrx and inputs 0 <= i < n only, the outputs by receivers < nrx and k < count; a
 * row in LDS holds `span` floats and a tile's span is at most that (ddc_audio.h audio_span), the staging loop is
 * clamped to it; the records are indexed by receivers < nrx and 0 <= e < T - 1.
 */
#include "ddc_audio.h"
#include "ddc_dev.h"
#include "ddc_host.h"

#pragma clang fp contract(off)

namespace pddc {

/* input idx of receiver row `xr` (idx >= -(T - 1)): before the batch's first from the carried record `old` (H = T - 1
 * values, the newest last) */
__device__ __forceinline__ float audio_input(const float *xr, const float *old, long long idx, long long n, int H, bool fresh)
{
    if (idx < 0)
        return fresh ? 0.0f : old[H + idx];
    return idx < n ? xr[idx] : 0.0f;
}

__global__ __launch_bounds__(kAudioThreads) void k_audio(AudioArgs a)
{
    constexpr int G = kAudioGroup, TT = kAudioTile;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = (int)threadIdx.x;
    const int P = a.phases, T = a.taps, H = T - 1;
    const int glen = P * T + 1;
    float *sg = lds;
    float *sx = lds + ((glen + 3) & ~3);
    const int g0 = (int)blockIdx.y * G;
    const int ng = a.nrx - g0 < G ? a.nrx - g0 : G;
    const bool fresh = a.fresh != 0;
    const long long o0 = (long long)blockIdx.x * TT;
    const int cnt = (int)(a.count - o0 < TT ? a.count - o0 : TT);

    if (cnt > 0) {
        /* the tile's span: from T - 1 inputs before its first output's to its last output's */
        const uint64_t vf = (uint64_t)a.r0 + (uint64_t)o0 * a.M;
        const uint64_t vl = (uint64_t)a.r0 + (uint64_t)(o0 + cnt - 1) * a.M;
        const long long base = (long long)a.n0 + (long long)(vf / a.L) - H;
        const long long last = (long long)a.n0 + (long long)(vl / a.L);
        int len = (int)(last - base + 1);
        len = len < a.span ? len : a.span;
        for (int e = tid; e < glen; e += kAudioThreads)
            sg[e] = a.proto[e];
        for (int g = 0; g < G; ++g) {
            float *row = sx + g * a.span;
            const int j = g0 + (g < ng ? g : 0);
            const float *xr = a.x + (long long)j * a.x_stride;
            const float *old = a.state + (long long)j * H;
            for (int e = tid; e < len; e += kAudioThreads) {
                const float v = audio_input(xr, old, base + e, a.n, H, fresh);
                row[e] = g < ng ? v : 0.0f;
            }
        }
        __syncthreads();
        if (tid < cnt) {
            const uint64_t v = (uint64_t)a.r0 + (uint64_t)(o0 + tid) * a.M;
            const long long n = (long long)a.n0 + (long long)(v / a.L);
            const uint64_t u = (v % a.L) * (uint64_t)P;
            const int q = (int)(u / a.L);
            const float alpha = (float)(uint32_t)(u % a.L) / (float)a.L;
            const float *pg = sg + q;
            const float *px = sx + (int)(n - base);         /* x[n - t] of row g: px[g span - t], n - base - t >= 0 */
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g)
                acc[g] = 0.0f;
            for (int t = 0; t < T; ++t) {
                const float ga = pg[t * P], gb = pg[t * P + 1];
                const float w = fmaf(alpha, gb - ga, ga);
#pragma unroll
                for (int g = 0; g < G; ++g)
                    acc[g] = fmaf(w, px[g * a.span - t], acc[g]);
            }
            const long long k = o0 + tid;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g < ng) {
                    if (a.f32)
                        a.f32[(long long)(g0 + g) * a.f32_stride + k] = acc[g];
                    if (a.i16)
                        a.i16[(long long)(g0 + g) * a.i16_stride + k] = pcm16(acc[g], a.scale);
                }
            }
        }
    }

    /* the new carried record: the last T - 1 values of [old record | batch] */
    if (blockIdx.x == gridDim.x - 1 && tid < H) {
        for (int g = 0; g < ng; ++g) {
            const int j = g0 + g;
            a.new_state[(long long)j * H + tid] =
                audio_input(a.x + (long long)j * a.x_stride, a.state + (long long)j * H, a.n - H + tid, a.n, H, fresh);
        }
    }
}

hipError_t launch_audio(const AudioArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.count < 0 || a.nrx <= 0 || a.nrx > kAudioMaxRx || !a.x || a.x_stride < a.n || !a.proto || !a.state ||
        !a.new_state || (a.count > 0 && !a.f32 && !a.i16) || (a.f32 && a.f32_stride < a.count) ||
        (a.i16 && a.i16_stride < a.count))
        return hipErrorInvalidValue;
    if (a.L < 1 || a.L > kAudioMaxRatio || a.M < 1 || a.M > kAudioMaxRatio || (uint64_t)a.M > (uint64_t)kAudioMaxDecim * a.L ||
        a.r0 >= a.L || a.n0 > kAudioMaxDecim || a.phases < kAudioMinPhases || a.phases > kAudioMaxPhases ||
        (a.phases & (a.phases - 1)) || a.taps < 1 || a.taps > kAudioMaxTaps || a.phases * a.taps > kAudioMaxProto ||
        a.span != audio_span(a.L, a.M, a.taps))
        return hipErrorInvalidValue;
    /* the last output's input must lie in the batch: n0 + (r0 + (count - 1) M) div L < n */
    if (a.count > 0) {
        const unsigned __int128 v = (unsigned __int128)a.r0 + (unsigned __int128)(a.count - 1) * a.M;
        if (v >> 63 || (unsigned __int128)a.n0 + v / a.L >= (unsigned __int128)a.n)
            return hipErrorInvalidValue;
    }
    const long long nx = a.count > 0 ? (a.count + kAudioTile - 1) / kAudioTile : 1;
    if (nx > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nx, (unsigned)((a.nrx + kAudioGroup - 1) / kAudioGroup));
    const size_t lds = audio_lds_floats(a.phases, a.taps, a.span) * sizeof(float);
    return launch_dynamic_lds<&k_audio>(kAudioLdsCap, grid, dim3(kAudioThreads), lds, s, a);
}

} // namespace pddc
