/*
 * ddc_adapt.hip -- the adaptive line enhancer: per receiver a leaky normalised LMS predictor of T taps over the audio
 * delayed by D samples; the prediction is the noise-reduced audio, the prediction error the notched audio (gfx950 only).
 *
 *   k_adapt     per receiver j and sample m, with u_k = x[m - D - k]: y = tree sum of w_k u_k, P = tree sum of u_k u_k,
 *               e = x[m] - y, g = (mu e) / (P + eps), w_k = (w_k lam) + (g u_k); out = y (NR), e (NOTCH) or x[m] (OFF,
 *               which leaves the weights alone).  DESIGN.md 8 has the definition.
 *
 * Layout: a block is one wave.  A receiver has L = min(T, kAdaptLanes) lanes of it and a wave G = 64 / L receivers; lane
 * l of a receiver holds the P = T / L taps k = l + i L, i < P, in registers for the whole launch.  The halving tree's
 * levels h = T/2 .. L then add registers of one lane (i and i + h / L), the levels h = L/2 .. 1 are a lane-xor butterfly:
 * DPP row rotations and quad permutations for h <= 8, v_permlane16_swap / v_permlane32_swap for h = 16, 32.  After a
 * butterfly level h the values have the period h over the lanes -- a + b and b + a are the same bits -- so every lane of
 * the receiver ends with the tree's v_0: nothing is broadcast, and a rotation by h serves as the xor with h.
 * Walk: the wave takes its receivers through the launch tile by tile, TT = 256 samples a time.  Per receiver the LDS row
 * sx holds the kAdaptHist samples before the tile and the tile behind them, so lane l reads x[m - D - l - i L] at stride 1
 * with no wrap.
 *   1. the tile's inputs, loaded a tile ahead into registers (coalesced 4-byte loads), go to sx; the NEXT tile's loads
 *      are issued here and stay in registers over the chain.
 *   2. the chain, sample by sample, C = 4 samples' delay-line reads issued a chunk ahead; lane 0 of the receiver leaves
 *      out[m] in so.
 *   3. so is stored coalesced, once per tile; the last kAdaptHist samples of sx move to its front.
 *   The weights go to the new record at the end with the last D + T - 1 inputs, read back from sx.
 * Bits: every value is made by the definition's operation sequence (contraction is off in this file, the division is
 * the correctly rounded one, float32 denormals are kept: the target's default mode) from the receiver's own series,
 * weights and table entry, so nothing depends on the batch cut, K, j's index, the other receivers or the layout.  No
 * atomics, no scratch.
 * In place (out == a): a tile's inputs are in registers before the tile before it is stored, and a wave alone reads and
 * writes its receivers' rows.
 * Bounds: a and out are indexed by receivers < nrx and samples < n only; the records by receivers < nrx, taps < T and
 * inputs < D + T - 1; sx between kAdaptHist - D - (T - 1) >= 1 and kAdaptHist + TT + C - 2 < the row's length.
 */
#include "ddc_adapt.h"
#include "ddc_dev.h"

#pragma clang fp contract(off)

namespace pddc {

template <int CTRL> __device__ __forceinline__ float adapt_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

/* v + (v of lane ^ H), for v of period 2 H over the lanes where a rotation stands for the xor (H = 4) */
template <int H> __device__ __forceinline__ float adapt_xor_add(float v)
{
    if constexpr (H == 1) {
        return v + adapt_dpp<0xB1>(v);                  /* quad_perm [1, 0, 3, 2] */
    } else if constexpr (H == 2) {
        return v + adapt_dpp<0x4E>(v);                  /* quad_perm [2, 3, 0, 1] */
    } else if constexpr (H == 4) {
        return v + adapt_dpp<0x124>(v);                 /* row_ror:4: lane ^ 4 mod 8, and v has the period 8 */
    } else if constexpr (H == 8) {
        return v + adapt_dpp<0x128>(v);                 /* row_ror:8: lane ^ 8 within the row of 16 */
    } else if constexpr (H == 16) {
        /* rows 1, 3 of the first operand change places with rows 0, 2 of the second: (r0 r0 r2 r2) + (r1 r1 r3 r3) */
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else {
        static_assert(H == 32, "a wave has 64 lanes");
        /* lanes 32 .. 63 of the first operand change places with lanes 0 .. 31 of the second: (lo lo) + (hi hi) */
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}

/* the levels h = L/2 .. 1 of the two tree sums, side by side */
template <int L> __device__ __forceinline__ void adapt_butterfly(float &y, float &p)
{
    if constexpr (L >= 64) { y = adapt_xor_add<32>(y); p = adapt_xor_add<32>(p); }
    if constexpr (L >= 32) { y = adapt_xor_add<16>(y); p = adapt_xor_add<16>(p); }
    y = adapt_xor_add<8>(y); p = adapt_xor_add<8>(p);
    y = adapt_xor_add<4>(y); p = adapt_xor_add<4>(p);
    y = adapt_xor_add<2>(y); p = adapt_xor_add<2>(p);
    y = adapt_xor_add<1>(y); p = adapt_xor_add<1>(p);
}

/* one sample of one receiver on its L lanes: the definition's steps 1 .. 5 on this lane's P taps; -> out */
template <int P, int L>
__device__ __forceinline__ float adapt_sample(float (&w)[P], const float (&u)[P], float x, float mu, float lam, float eps,
                                              bool adapt, bool nr, bool notch)
{
    float vy[P], vp[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        vy[i] = w[i] * u[i];
        vp[i] = u[i] * u[i];
    }
#pragma unroll
    for (int h = P / 2; h >= 1; h /= 2)
#pragma unroll
        for (int i = 0; i < h; ++i) {
            vy[i] = vy[i] + vy[i + h];
            vp[i] = vp[i] + vp[i + h];
        }
    float y = vy[0], p = vp[0];
    adapt_butterfly<L>(y, p);
    const float e = x - y;
    const float g = (mu * e) / (p + eps);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const float wn = (w[i] * lam) + (g * u[i]);
        w[i] = adapt ? wn : w[i];
    }
    /* the modes differ from lane group to lane group: selects */
    float ov = nr ? y : x;
    ov = notch ? e : ov;
    return ov;
}

template <int T, int L> __global__ __launch_bounds__(kAdaptThreads) void k_adapt(AdaptArgs a)
{
    constexpr int P = T / L, G = 64 / L, TT = kAdaptTile, HB = kAdaptHist, C = 4;
    constexpr int GS = HB + TT + 16;    /* a receiver's row; the 16 keep two receivers of a half wave on different banks */
    constexpr int RT = TT / 64, RH = HB / 64;
    static_assert(L >= 16 && L <= 64 && P >= 1 && P * L == T && G * L == 64 && kAdaptThreads == 64, "the lanes of one wave");
    static_assert(HB >= kAdaptMaxDelay + kAdaptMaxTaps - 1 && TT % 64 == 0 && HB % 64 == 0 && TT % C == 0, "row layout");
    __shared__ float sx[G * GS];
    __shared__ float so[G][TT];
    const int lane = (int)threadIdx.x;
    const int grp = lane / L, l = lane % L;
    const int j0 = (int)blockIdx.x * G;
    const int j = j0 + grp;
    const bool live = j < a.nrx;
    const int H = a.D + T - 1;

    uint32_t mode = kAdaptOff;
    float mu = 0.0f, lam = 1.0f;
    bool keep = false;                  /* the carried weights are read */
    if (live) {
        const AdaptRx r = a.rx[j];
        mode = r.mode;
        mu = r.mu;
        lam = r.lam;
        keep = !a.fresh && !(r.flags & kAdaptRestart);
    }
    const bool adapt = mode != kAdaptOff, nr = mode == kAdaptNr, notch = mode == kAdaptNotch;
    float w[P];
#pragma unroll
    for (int i = 0; i < P; ++i)
        w[i] = keep ? a.old_w[(long long)j * T + l + i * L] : 0.0f;

    /* the inputs before the launch: entry q of the record is x[-1 - q] */
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            const int q = r * 64 + lane;
            float v = 0.0f;
            if (!a.fresh && j0 + g < a.nrx && q < H)
                v = a.old_h[(long long)(j0 + g) * H + q];
            sx[g * GS + HB - 1 - q] = v;
        }

    float pre[G][RT];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int i = r * 64 + lane;
            pre[g][r] = 0.0f;
            if (j0 + g < a.nrx && i < a.n)
                pre[g][r] = a.a[(long long)(j0 + g) * a.a_stride + i];
        }

    const float *const ub = sx + grp * GS + HB - a.D - l;   /* ub[i - k] is u_k of the tile's sample i */
    const float *const xb = sx + grp * GS + HB;
    int cnt = 0;
    for (long long o = 0;; o += TT) {
        cnt = (int)(a.n - o < TT ? a.n - o : TT);
        /* 1. this tile into its rows; the next tile's loads */
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RT; ++r)
                sx[g * GS + HB + r * 64 + lane] = pre[g][r];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const long long i = o + TT + r * 64 + lane;
                pre[g][r] = 0.0f;
                if (j0 + g < a.nrx && i < a.n)
                    pre[g][r] = a.a[(long long)(j0 + g) * a.a_stride + i];
            }
        __syncthreads();

        /* 2. the chain */
        float un[C][P], xn[C];
#pragma unroll
        for (int s = 0; s < C; ++s) {
            xn[s] = xb[s];
#pragma unroll
            for (int i = 0; i < P; ++i)
                un[s][i] = ub[s - i * L];
        }
        for (int i0 = 0; i0 < cnt; i0 += C) {
            float u[C][P], x[C];
#pragma unroll
            for (int s = 0; s < C; ++s) {
                x[s] = xn[s];
#pragma unroll
                for (int i = 0; i < P; ++i)
                    u[s][i] = un[s][i];
            }
            if (i0 + C < cnt) {
#pragma unroll
                for (int s = 0; s < C; ++s) {
                    xn[s] = xb[i0 + C + s];
#pragma unroll
                    for (int i = 0; i < P; ++i)
                        un[s][i] = ub[i0 + C + s - i * L];
                }
            }
            if (i0 + C <= cnt) {
#pragma unroll
                for (int s = 0; s < C; ++s) {
                    const float ov = adapt_sample<P, L>(w, u[s], x[s], mu, lam, a.eps, adapt, nr, notch);
                    if (l == 0)
                        so[grp][i0 + s] = ov;
                }
            } else {
#pragma unroll
                for (int s = 0; s < C - 1; ++s)
                    if (i0 + s < cnt) {
                        const float ov = adapt_sample<P, L>(w, u[s], x[s], mu, lam, a.eps, adapt, nr, notch);
                        if (l == 0)
                            so[grp][i0 + s] = ov;
                    }
            }
        }
        __syncthreads();

        /* 3. the tile's outputs; the row's end to its front */
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const int i = r * 64 + lane;
                if (j0 + g < a.nrx && i < cnt)
                    a.out[(long long)(j0 + g) * a.out_stride + o + i] = so[g][i];
            }
        if (o + TT >= a.n)
            break;
        float mv[G][RH];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RH; ++r)
                mv[g][r] = sx[g * GS + TT + r * 64 + lane];
        __syncthreads();
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RH; ++r)
                sx[g * GS + r * 64 + lane] = mv[g][r];
        /* the next tile's step 1 writes sx from HB on, which the move has read before its barrier, and so only after
         * its own barrier */
    }

    /* the records: the weights, and the last H inputs (the last tile held cnt samples) */
    if (live) {
#pragma unroll
        for (int i = 0; i < P; ++i)
            a.new_w[(long long)j * T + l + i * L] = w[i];
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            const int q = r * 64 + lane;
            if (j0 + g < a.nrx && q < H)
                a.new_h[(long long)(j0 + g) * H + q] = sx[g * GS + HB + cnt - 1 - q];
        }
}

template <int T> static hipError_t launch_adapt_t(const AdaptArgs &a, hipStream_t s)
{
    constexpr int L = adapt_lanes(T), G = 64 / L;
    hipLaunchKernelGGL((k_adapt<T, L>), dim3((unsigned)((a.nrx + G - 1) / G)), dim3(kAdaptThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_adapt(const AdaptArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kAdaptMaxRx || a.a_stride < a.n || a.out_stride < a.n || !a.a || !a.out || !a.rx ||
        !a.old_w || !a.old_h || !a.new_w || !a.new_h || a.D < 1 || a.D > kAdaptMaxDelay || !(a.eps > 0.0f))
        return hipErrorInvalidValue;
    switch (a.T) {
    case 16: return launch_adapt_t<16>(a, s);
    case 32: return launch_adapt_t<32>(a, s);
    case 64: return launch_adapt_t<64>(a, s);
    case 128: return launch_adapt_t<128>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace pddc
