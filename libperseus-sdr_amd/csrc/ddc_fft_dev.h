/*
 * ddc_fft_dev.h -- the in-workgroup Stockham transform of every transforming kernel: the panorama (ddc_spectrum.hip), the
 * channelizer (ddc_channelizer.hip), the scope (ddc_scope.hip) and the noise reduction (ddc_denoise.hip).  Plans, register
 * transforms, LDS images, and the three steps of a pass -- load, twiddle and transform, put -- each written once.
 * Internal; gfx950 only.
 *
 * Transform: Stockham autosort, decimation in time; a radix-R pass keeps a thread's R points in registers (radix 16 =
 * 4 x 4, radix 8 = 4 x 2 with the constants of W16), so a segment crosses LDS once per pass.
 *   pass p (sub-transforms of Ns done):  v[r] = in[j + r N/R] * W(Ns R)^(r k), k = j mod Ns;  FFT_R;
 *                                        out[(j / Ns) Ns R + k + r Ns] = v[r]
 * Natural order comes out of the last pass, whose outputs stay in registers: thread j holds bins j + r N/R.
 * Radices: SpecPlan (panorama, channelizer: a block of N/16 threads, at most 256, is one transform) 16 * 16 * {4, 8, 16}
 * for N = 1024, 2048, 4096 and 16 * 16 * 8 * 4 for 8192; FramePlan (scope, noise reduction: N / R1 threads per transform,
 * whose loads ARE the first butterfly) 16 * 16 for 256, 8 * 8 * 8 for 512, then the same.  Twiddles: one table per pass,
 * [r - 1][k], built on the host in double and rounded once (spectrum_build_twiddles, ddc_spectrum.h).
 * A kernel file that turns contraction off does so BELOW this header (ddc_denoise.hip): the transforms keep one setting.
 */
#ifndef PDDC_DDC_FFT_DEV_H
#define PDDC_DDC_FFT_DEV_H

#include "ddc_dev.h"

namespace pddc {

template <int N> struct SpecPlan;
template <> struct SpecPlan<1024> { static constexpr int NP = 3, R2 = 4, R3 = 1, BLOCKS_PER_CU = 8; };
template <> struct SpecPlan<2048> { static constexpr int NP = 3, R2 = 8, R3 = 1, BLOCKS_PER_CU = 4; };
template <> struct SpecPlan<4096> { static constexpr int NP = 3, R2 = 16, R3 = 1, BLOCKS_PER_CU = 2; };
template <> struct SpecPlan<8192> { static constexpr int NP = 4, R2 = 8, R3 = 4, BLOCKS_PER_CU = 1; };

/* radices R1 * R2 [* R3], N / R1 threads per transform, G transforms per block (every wave of N = 256 is full) */
template <int N> struct FramePlan;
template <> struct FramePlan<256> { static constexpr int R1 = 16, R2 = 16, R3 = 1, G = 4; };
template <> struct FramePlan<512> { static constexpr int R1 = 8, R2 = 8, R3 = 8, G = 1; };
template <> struct FramePlan<1024> { static constexpr int R1 = 16, R2 = 16, R3 = 4, G = 1; };
template <> struct FramePlan<2048> { static constexpr int R1 = 16, R2 = 16, R3 = 8, G = 1; };
template <> struct FramePlan<4096> { static constexpr int R1 = 16, R2 = 16, R3 = 16, G = 1; };

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmulw(float2 a, float2 w)
{
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

/* a * W16^M, M a compile-time constant: the trivial ones cost no multiply */
template <int M> __device__ __forceinline__ float2 mul_w16(float2 a)
{
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
    if (M == 0)
        return a;
    if (M == 4)
        return make_float2(a.y, -a.x);
    if (M == 2)
        return make_float2((a.x + a.y) * H, (a.y - a.x) * H);
    if (M == 6)
        return make_float2((a.y - a.x) * H, -(a.x + a.y) * H);
    if (M == 1)
        return cmulw(a, make_float2(C1, -S1));
    if (M == 3)
        return cmulw(a, make_float2(S1, -C1));
    if (M == 9)
        return cmulw(a, make_float2(-C1, S1));
    return a;
}

/* 4-point transform in place, natural order */
__device__ __forceinline__ void fft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3)
{
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = csub(a1, a3);
    a0 = cadd(t0, t2);
    a2 = csub(t0, t2);
    a1 = make_float2(t1.x + t3.y, t1.y - t3.x);
    a3 = make_float2(t1.x - t3.y, t1.y + t3.x);
}

/* R-point transform of v[0 .. R) in registers; X[k] ends up in v[fft_pos<R>(k)] */
template <int R> __device__ __forceinline__ constexpr int fft_pos(int k)
{
    return R == 16 ? 4 * (k & 3) + (k >> 2) : R == 8 ? 2 * (k & 3) + (k >> 2) : k;
}

template <int R> __device__ __forceinline__ void fft_reg(float2 (&v)[R]);
template <> __device__ __forceinline__ void fft_reg<4>(float2 (&v)[4]) { fft4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void fft_reg<8>(float2 (&v)[8])
{
    /* n = 2 n1 + n2: two 4-point transforms over n1, W8^(n2 k1), four 2-point ones over n2 */
    fft4(v[0], v[2], v[4], v[6]);
    fft4(v[1], v[3], v[5], v[7]);
    v[3] = mul_w16<2>(v[3]);
    v[5] = mul_w16<4>(v[5]);
    v[7] = mul_w16<6>(v[7]);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
        const float2 a = v[2 * k1], b = v[2 * k1 + 1];
        v[2 * k1] = cadd(a, b);
        v[2 * k1 + 1] = csub(a, b);
    }
}
template <> __device__ __forceinline__ void fft_reg<16>(float2 (&v)[16])
{
    /* n = 4 n1 + n2: four 4-point transforms over n1 (A[n2][k1] at v[4 k1 + n2]), W16^(n2 k1), four over n2 */
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2)
        fft4(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
    v[5] = mul_w16<1>(v[5]);
    v[6] = mul_w16<2>(v[6]);
    v[7] = mul_w16<3>(v[7]);
    v[9] = mul_w16<2>(v[9]);
    v[10] = mul_w16<4>(v[10]);
    v[11] = mul_w16<6>(v[11]);
    v[13] = mul_w16<3>(v[13]);
    v[14] = mul_w16<6>(v[14]);
    v[15] = mul_w16<9>(v[15]);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
        fft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
}

/* LDS images (indices in float2).  A first pass of radix S writes S consecutive points per lane (rows of S), and the
 * panorama's loaders write 8 consecutive samples per lane (4 x ds_write_b128); either would put a lane group on one bank
 * set, so both images are XOR-swizzled such that the writes AND the stride-1 b64 reads of the next pass are conflict
 * free.  The later images are plain.
 * The image a first pass of radix S writes: the low bits of a row XOR the row's number */
template <int S> __device__ __forceinline__ int fft_swz(int i) { return i ^ ((i / S) & (S - 1)); }

/* the loaders' image: a lane writes 4 chunks of 16 B = samples 8g .. 8g+7, the chunk's low two bits XOR bits 1..2 of g */
__device__ __forceinline__ int spec_swz0(int i) { return i ^ (((i >> 4) & 3) << 1); }

/* an image by number: 0 plain, S > 0 a radix-S first pass's, kImgLoaders the loaders' */
static constexpr int kImgLoaders = -1;
template <int IMG> __device__ __forceinline__ int fft_img(int i)
{
    return IMG == kImgLoaders ? spec_swz0(i) : IMG > 0 ? fft_swz<(IMG > 0 ? IMG : 1)>(i) : i;
}

/* The steps of a radix-R pass over sub-transforms of NS for thread t of the TS that share a transform of N: the thread's
 * N / R / TS butterflies are j = t + b TS.  A caller puts its barriers between them.
 * (a) the butterflies' points from the image: v[b][r] = point j + r N/R */
template <int N, int TS, int R, int IMG>
__device__ __forceinline__ void fft_load(const float2 *buf, int t, float2 (&v)[N / R / TS][R])
{
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b) {
        const int j = t + b * TS;
#pragma unroll
        for (int r = 0; r < R; ++r)
            v[b][r] = buf[fft_img<IMG>(j + r * (N / R))];
    }
}

/* (b) times W(NS R)^(r k), k = j mod NS (tw: the pass's table; none in the first pass, NS == 1), and the R-point
 * transform: X[r] at v[b][fft_pos<R>(r)]; then each(j, v[b]), for a caller that hands a butterfly on before the next */
struct FftNoEach {
    template <class V> __device__ __forceinline__ void operator()(int, const V &) const {}
};
template <int N, int TS, int R, int NS, class Each = FftNoEach>
__device__ __forceinline__ void fft_bfly(const float2 *tw, int t, float2 (&v)[N / R / TS][R], Each each = Each())
{
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b) {
        const int j = t + b * TS;
        if (NS > 1) {
            const int k = j & (NS - 1);
#pragma unroll
            for (int r = 1; r < R; ++r)
                v[b][r] = cmulw(v[b][r], tw[(r - 1) * NS + k]);
        }
        fft_reg<R>(v[b]);
        each(j, v[b]);
    }
}

/* (c) the outputs into the next pass's image: X[r] to point (j - k) R + k + r NS */
template <int N, int TS, int R, int NS, int IMG>
__device__ __forceinline__ void fft_put(float2 *buf, int t, const float2 (&v)[N / R / TS][R])
{
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b) {
        const int j = t + b * TS, k = j & (NS - 1), j0 = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r)
            buf[fft_img<IMG>(j0 + r * NS)] = v[b][fft_pos<R>(r)];
    }
}

/* one pass of the panorama's block-wide transform, image IN to image OUT; LAST: the outputs go to the thread's sums
 * instead of LDS (bin j + r N/R at acc[b * R + r]) */
template <int N, int NT, int R, int NS, int IN, int OUT, bool LAST, bool PEAK, int NACC>
__device__ __forceinline__ void spec_pass(float2 *buf, const float2 *tw, float (&acc)[NACC], float (&pk)[NACC])
{
    constexpr int NB = N / R / NT;
    const int tid = threadIdx.x;
    float2 v[NB][R];
    fft_load<N, NT, R, IN>(buf, tid, v);
    fft_bfly<N, NT, R, NS>(tw, tid, v);
    if (LAST) {
        static_assert(!LAST || NACC == NB * R, "a thread's bins");
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float2 x = v[b][fft_pos<R>(r)];
                const float p = x.x * x.x + x.y * x.y;
                acc[(b * R + r) % NACC] += p;
                if (PEAK)
                    pk[(b * R + r) % NACC] = fmaxf(pk[(b * R + r) % NACC], p);
            }
        __syncthreads();          /* the next segment's loaders write where this pass read */
    } else {
        __syncthreads();          /* everybody has read */
        fft_put<N, NT, R, NS, OUT>(buf, tid, v);
        __syncthreads();
    }
}

/* a pass between LDS images without the sums (the channelizer's passes before the last) */
template <int N, int NT, int R, int NS, int IN, int OUT>
__device__ __forceinline__ void spec_pass_mid(float2 *buf, const float2 *tw)
{
    float none[1], nonep[1];
    spec_pass<N, NT, R, NS, IN, OUT, false, false, 1>(buf, tw, none, nonep);
}

/* the LAST pass handing the bins to a store instead of to the sums: f(bin, X[bin]) for the thread's bins
 * j + b NT + r N/R, r outermost per b -- consecutive lanes hold consecutive bins */
template <int N, int NT, int R, int NS, int IN, class F>
__device__ __forceinline__ void spec_pass_out(float2 *buf, const float2 *tw, F f)
{
    constexpr int NB = N / R / NT;
    const int tid = threadIdx.x;
    float2 v[NB][R];
    fft_load<N, NT, R, IN>(buf, tid, v);
    __syncthreads();              /* everybody has read: the next row's loaders may write while the stores go out */
    fft_bfly<N, NT, R, NS>(tw, tid, v, [&](int j, const float2 (&x)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            f(j + r * (N / R), x[fft_pos<R>(r)]);
    });
}

} // namespace pddc
#endif
