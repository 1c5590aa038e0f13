/*
 * ddc_denoise.hip -- spectral noise reduction per receiver (gfx950 only).
 *
 *   k_denoise<N>   a group of N / R1 threads owns one receiver for the whole launch and walks the frames the batch completes
 *                  in ascending order: load (real float32, consecutive lanes consecutive samples), times the window,
 *                  N-point transform of (f, 0) inside the group (registers + LDS), the recursion of the definition per
 *                  bin 0 .. N/2 (S, N and A stay in the bin's thread from the first frame to the last), the gains
 *                  through LDS to the mirrored bins, the inverse transform, times the window, overlap-add into a ring
 *                  in LDS; the hop a frame finishes goes to out.  One launch per batch; no spectrum in global memory, no
 *                  atomics, nothing cleared.
 *
 * Transform: the Stockham passes of ddc_fft_dev.h (fft_load, fft_bfly, fft_put) with FramePlan's radices, the scope's;
 * dn_fft below composes them.  That header stays above this file's contraction pragma.  N = 256 is 16 x 16 with 16
 * threads per receiver and four receivers per block, N = 512 is 8 x 8 x 8 and N = 1024 16 x 16 x 4 with 64 threads and
 * one receiver.  A thread's loads are its first butterfly (samples t + r TS), and the bins the last pass leaves in a
 * thread (t + m TS) are again a first butterfly's inputs: the inverse is the same passes on (im, re), its real part is
 * the imaginary part that comes out, and forward and inverse meet in registers.  A frame's transform is a function of
 * that frame's N values alone: nothing is packed with a neighbour.
 * Bins above N/2 are not tracked: Y[N - k] = G[k] X[N - k], with X[N - k] as the full-size transform gave it.
 *
 * Ring: y[m] lives in slot m mod N.  Frame q adds its term i to slot ((q + 1) hop + i) mod N; its last hop values are
 * the first terms of their sums and are stored, not added; the sums of its first hop values are complete and leave:
 * out index (q + 1) hop + i, to out when the batch holds that index, to the carried hop otherwise.  Frames q < R - 1
 * finish y[m] with m < 0: zeros leave.
 * Bits: contraction is off below the transforms, divisions are the correctly rounded ones, and every value is made by
 * one operation sequence whatever the cut: a sample is selected from the carried samples or from x by its index, the
 * carried values from zeros by `fresh`, nothing else differs.
 */
#include "ddc_denoise.h"
#include "ddc_fft_dev.h"

namespace pddc {

/* The N-point transform of a[r] = point t + r TS; X[m] = bin t + m TS.  It writes the group's image and ends with reads
 * of it: the caller puts a barrier in front of the next call. */
template <int N> __device__ __forceinline__ void dn_fft(float2 (&a)[FramePlan<N>::R1], float2 *buf, const float2 *tw2, int t)
{
    using Plan = FramePlan<N>;
    constexpr int R1 = Plan::R1, R2 = Plan::R2, R3 = Plan::R3, TS = N / R1;
    fft_reg<R1>(a);
#pragma unroll
    for (int r = 0; r < R1; ++r)
        buf[fft_swz<R1>(t * R1 + r)] = a[fft_pos<R1>(r)];
    __syncthreads();
    float2 v[N / R2 / TS][R2];
    fft_load<N, TS, R2, R1>(buf, t, v);
    fft_bfly<N, TS, R2, R1>(tw2, t, v);
    if constexpr (R3 > 1) {
        constexpr int NB = N / R3 / TS;
        const float2 *tw3 = tw2 + (R2 - 1) * R1;
        __syncthreads();                          /* everybody has read */
        fft_put<N, TS, R2, R1, 0>(buf, t, v);
        __syncthreads();
        float2 y[NB][R3];
        fft_load<N, TS, R3, 0>(buf, t, y);
        fft_bfly<N, TS, R3, R1 * R2>(tw3, t, y);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < R3; ++r)
                a[b + NB * r] = y[b][fft_pos<R3>(r)];
    } else {
        static_assert(R3 > 1 || N / R2 / TS == 1, "one butterfly per thread in the last of two passes");
#pragma unroll
        for (int r = 0; r < R2; ++r)
            a[r] = v[0][fft_pos<R2>(r)];
    }
}

#pragma clang fp contract(off)

template <int N>
__global__ __launch_bounds__(N / FramePlan<N>::R1 * FramePlan<N>::G) void k_denoise(DenoiseArgs p)
{
    using Plan = FramePlan<N>;
    constexpr int R1 = Plan::R1, G = Plan::G;
    constexpr int TS = N / R1, STRIDE = N + (G > 1 ? 16 : 0);
    constexpr int NH = R1 / 2;                    /* a thread's bins t + m TS up to N/2: m < NH, and m == NH in thread 0 */
    constexpr int HB = N / 2 + 1;
    __shared__ __attribute__((aligned(16))) float2 lds[G * STRIDE];
    __shared__ float ring_s[G * N];
    __shared__ float gain_s[G * (N / 2 + TS)];

    const int tid = threadIdx.x, g = tid / TS, t = tid % TS;
    const int j = blockIdx.x * G + g;
    const bool valid = j < p.nrx;
    float2 *buf = lds + g * STRIDE;
    float *ring = ring_s + g * N, *gain = gain_s + g * (N / 2 + TS);
    const float2 *tw2 = reinterpret_cast<const float2 *>(p.twiddles);

    DenoiseRx rx = p.rx[valid ? j : 0];
    const bool off = rx.mode == kDenoiseOff, hold = (rx.flags & kDenoiseHold) != 0;
    bool first = p.fresh || (rx.flags & kDenoiseRestart);
    const bool carried = valid && !p.fresh;
    const int hop = p.hop, mh = hop / TS, rmask = N / hop - 1;
    const long long m0 = p.q0 * hop + p.pos;      /* the batch's first sample */
    const float *x = p.x + (size_t)(valid ? j : 0) * p.x_stride;
    float *out = p.out + (size_t)(valid ? j : 0) * p.out_stride;
    const size_t jN = (size_t)(valid ? j : 0) * N, jH = (size_t)(valid ? j : 0) * hop, jS = (size_t)(valid ? j : 0) * HB, pl = (size_t)p.nrx * HB;

    auto sample = [&](long long v) -> float {
        if (!valid)
            return 0.0f;
        if (v < p.clen)
            return p.fresh ? 0.0f : p.old_carry[jN + v];
        return x[v - p.clen];
    };

    /* the head of the batch: what the last frame before it finished and no batch has given out yet */
    if (valid) {
        const long long cnt = min(p.n, (long long)(hop - p.pos));
        for (int i = t; i < cnt; i += TS)
            out[i] = carried ? p.old_pend[jH + p.pos + i] : 0.0f;
        if (p.nseg == 0)
            for (int i = t; i < hop; i += TS)
                p.new_pend[jH + i] = carried ? p.old_pend[jH + i] : 0.0f;
        /* the samples from the start of the first frame this batch leaves incomplete */
        const long long shift = p.nseg * hop;
        for (int i = t; i < p.new_clen; i += TS)
            p.new_carry[jN + i] = sample(shift + i);
    }
    if (p.nseg == 0)
        return;

    float win[R1], S[NH + 1], Nn[NH + 1], A[NH + 1];
#pragma unroll
    for (int m = 0; m < R1; ++m)
        win[m] = p.window[t + m * TS];
#pragma unroll
    for (int m = 0; m <= NH; ++m) {
        const bool own = carried && !first && (m < NH || t == 0);
        const int k = t + m * TS;
        S[m] = own ? p.old_sna[jS + k] : 0.0f;
        Nn[m] = own ? p.old_sna[pl + jS + k] : 0.0f;
        A[m] = own ? p.old_sna[2 * pl + jS + k] : 0.0f;
    }
    for (int i = t; i < N; i += TS)
        ring[i] = carried ? p.old_ola[jN + i] : 0.0f;

    const float sm = p.smooth, up = p.up, down = p.down, nmin = p.nmin, eps = p.eps;
    const float beta = rx.beta, gmin = rx.gmin, alpha = rx.alpha;

    float raw[R1];
    auto load_seg = [&](long long f) {
        const long long v0 = f * hop + t;
#pragma unroll
        for (int r = 0; r < R1; ++r)
            raw[r] = sample(v0 + r * TS);
    };
    load_seg(0);
    for (long long f = 0; f < p.nseg; ++f) {
        const long long q = p.q0 + f;
        float2 a[R1];
#pragma unroll
        for (int r = 0; r < R1; ++r)
            a[r] = make_float2(raw[r] * win[r], 0.0f);
        if (f + 1 < p.nseg)
            load_seg(f + 1);                      /* in flight while this frame is transformed */
        dn_fft<N>(a, buf, tw2, t);

        /* the recursion, bins t + m TS <= N/2 (a thread other than 0 computes m == NH too, on a bin above N/2: never stored, never read) */
#pragma unroll
        for (int m = 0; m <= NH; ++m) {
            const float P = a[m].x * a[m].x + a[m].y * a[m].y;
            float s = S[m], nn = Nn[m], aa = A[m];
            if (first) {
                s = P;
                nn = P;
                aa = 0.0f;
            } else if (!hold) {
                s = s + sm * (P - s);
                if (s > nn) {
                    float r = nn + up * nn;
                    const float r2 = nmin * s;
                    if (r < r2)
                        r = r2;
                    nn = (r < s) ? r : s;
                } else {
                    nn = nn + down * (s - nn);
                }
            }
            const float nb = beta * nn + eps;
            const float tt = P / nb - 1.0f;
            const float xi = alpha * (aa / nb) + (1.0f - alpha) * (tt > 0.0f ? tt : 0.0f);
            const float gg = xi / (1.0f + xi);
            float Gk = (gg > gmin) ? gg : gmin;
            if (off)
                Gk = 1.0f;
            S[m] = s;
            Nn[m] = nn;
            A[m] = (Gk * Gk) * P;
            gain[t + m * TS] = Gk;                /* t + NH TS < N/2 + TS: inside the group's array */
        }
        first = false;
        __syncthreads();                          /* the gains are there, and everybody has read the image */

        /* Y = G X on (im, re): the forward passes then give (im, re) of the inverse */
#pragma unroll
        for (int m = 0; m < R1; ++m) {
            const int k = t + m * TS;
            const float Gk = gain[k <= N / 2 ? k : N - k];
            a[m] = make_float2(Gk * a[m].y, Gk * a[m].x);
        }
        dn_fft<N>(a, buf, tw2, t);

        const int offs = (int)((q + 1) & rmask) * hop;
        const long long o0 = (q + 1) * hop - m0;  /* where the frame's first finished value stands in the batch, > 0 */
        const bool early = q < rmask;             /* it finishes y[m], m < 0 */
#pragma unroll
        for (int m = 0; m < R1; ++m) {
            const int i = t + m * TS, slot = (offs + i) & (N - 1);
            const float term = (a[m].y * (1.0f / N)) * win[m];
            if (m >= R1 - mh) {
                ring[slot] = term;
            } else {
                const float sum = ring[slot] + term;
                if (m < mh) {
                    const float y = early ? 0.0f : sum;
                    if (valid) {
                        if (o0 + i < p.n)
                            out[o0 + i] = y;
                        else
                            p.new_pend[jH + i] = y;
                    }
                } else {
                    ring[slot] = sum;
                }
            }
        }
        __syncthreads();                          /* the next frame writes the image this one read; the ring's owners change */
    }

    if (!valid)
        return;
#pragma unroll
    for (int m = 0; m <= NH; ++m) {
        const int k = t + m * TS;
        if (m < NH || t == 0) {
            p.new_sna[jS + k] = S[m];
            p.new_sna[pl + jS + k] = Nn[m];
            p.new_sna[2 * pl + jS + k] = A[m];
        }
    }
    for (int i = t; i < N; i += TS)
        p.new_ola[jN + i] = ring[i];
}

/* ------------------------------------------------------------------------ */
template <int N> static hipError_t launch_denoise_t(const DenoiseArgs &a, hipStream_t s)
{
    constexpr int G = FramePlan<N>::G, NT = N / FramePlan<N>::R1 * G;
    hipLaunchKernelGGL(k_denoise<N>, dim3((unsigned)((a.nrx + G - 1) / G)), dim3(NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_denoise(int nfft, const DenoiseArgs &a, hipStream_t s)
{
    switch (nfft) {
    case 256: return launch_denoise_t<256>(a, s);
    case 512: return launch_denoise_t<512>(a, s);
    case 1024: return launch_denoise_t<1024>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace pddc
