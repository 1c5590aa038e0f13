/*
 * ddc_channelizer.hip -- the channelizer: M uniform channels of the packed ADC stream as time series (gfx950 only).
 *
 *   k_channelize<M, P, Q>   polyphase filter bank by weighted overlap-add: prototype of L = P M taps, hop D = M / Q
 *                (Q = 1 critically sampled, Q = 2 oversampled by 2).  Per row s: u[r] = sum_p w[r + p M] x[s D + r + p M],
 *                the M-point transform of u (ddc_fft_dev.h, the panorama's), times (-1)^(k s) for Q = 2, the channels
 *                (first + i) mod M, i < count, stored as complex float32, row-major.
 *   k_channelize_tail       the packed tail carried to the next batch (ddc_packed.h).
 *
 * Walk: block b owns the RUN of consecutive rows [b run, (b + 1) run).  The stream is cut into UNITS of D samples; row s
 * needs units s .. s + P Q - 1, of which only the newest comes from HBM (3 x global_load_dwordx4 per 8 samples, loaded
 * one row ahead into registers).  The P Q - 1 older ones sit PACKED (6 B/sample) in an LDS ring: 6 (L - D) bytes.  A
 * thread folds exactly the groups of 8 samples it loaded itself (unit t, group g  ->  point 8 g + (t - s mod Q) D of u),
 * so the ring is thread-private spill space: no barrier guards it, and a lane's b128 accesses are consecutive.  A run's
 * first row reads its P Q - 1 older units from HBM as well (the run's "porch": (P Q - 1) / run of the input re-read).
 * The window values a thread needs (16 P floats) stay in registers for the whole run.
 * Bits: a row's fold runs p = 0 .. P-1 with one multiply and P - 1 fused multiply-adds per component whatever the
 * source of a unit; nothing is shared between rows.  The bits of a row depend on (M, D, P, w, samples) alone -- not on
 * grid, run length, batch cut or channel range.  No atomics.
 * Stores: the last pass holds bins j + r M/R per thread: consecutive lanes, consecutive channels -- 512 contiguous
 * bytes per wave and register, nontemporal; the range is a rotation of the index and a predicate.
 * LDS and registers per (M, P, Q): DESIGN.md 4 "Channelizer".
 */
#include "ddc_channelizer.h"
#include "ddc_spectrum.h"
#include "ddc_fft_dev.h"

namespace pddc {

static constexpr size_t kChanLdsPerCu = 160 * 1024;

static int chan_r2(int m) { return m == 1024 ? 4 : m == 2048 ? 8 : 16; }

size_t channelize_lds_bytes(int nchan, int taps_per_branch, int hop)
{
    const size_t tw = (size_t)(15 * 16 + (chan_r2(nchan) - 1) * 256);
    return 8 * ((size_t)nchan + tw) + 6 * ((size_t)taps_per_branch * nchan - hop);
}

int channelize_target_blocks(int nchan, int taps_per_branch, int hop, int ncu)
{
    const int plan = nchan == 1024 ? SpecPlan<1024>::BLOCKS_PER_CU
                     : nchan == 2048 ? SpecPlan<2048>::BLOCKS_PER_CU
                                     : SpecPlan<4096>::BLOCKS_PER_CU;
    int fit = (int)(kChanLdsPerCu / channelize_lds_bytes(nchan, taps_per_branch, hop));
    fit = fit < 1 ? 1 : fit > plan ? plan : fit;
    return fit * ncu;
}

template <int M, int P, int Q>
__global__ __launch_bounds__(M / 16 < 256 ? M / 16 : 256) void k_channelize(ChannelizeArgs a)
{
    using Plan = SpecPlan<M>;
    constexpr int NT = M / 16 < 256 ? M / 16 : 256;
    constexpr int NG = M / 8 / NT;               /* 48-byte groups of a row's u a thread folds */
    constexpr int NGU = NG / Q;                  /* ... of one unit                            */
    constexpr int GU = NT * NGU;                 /* groups of a unit                           */
    constexpr int D = M / Q;
    constexpr int PQ = P * Q, NSL = PQ - 1;      /* units of a row, ring slots                 */
    constexpr int R2 = Plan::R2;
    constexpr int TW1 = 0, TW2 = 15 * 16, TWN = TW2 + (R2 - 1) * 256;
    static_assert(NG == 2 && NGU >= 1 && Plan::R3 == 1, "k_channelize: M in 1024, 2048, 4096");
    extern __shared__ __attribute__((aligned(16))) float2 chan_lds[];
    float2 *buf = chan_lds;                      /* [M] */
    float2 *tw = chan_lds + M;                   /* [TWN] */
    u32x4 *ring = reinterpret_cast<u32x4 *>(chan_lds + M + TWN);   /* [NSL][3][GU] */
    const int tid = threadIdx.x;

    const long long row0 = (long long)blockIdx.x * a.run;
    if (row0 >= a.nrows)
        return;
    const int nr = (int)(a.nrows - row0 < a.run ? a.nrows - row0 : a.run);

    for (int i = tid; i < TWN; i += NT)
        tw[i] = reinterpret_cast<const float2 *>(a.twiddles)[i];
    float win[P][NG][8];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const f32x4 *w = reinterpret_cast<const f32x4 *>(a.proto + p * M + 8 * (tid + u * NT));
            const f32x4 x = w[0], y = w[1];
            win[p][u][0] = x.x; win[p][u][1] = x.y; win[p][u][2] = x.z; win[p][u][3] = x.w;
            win[p][u][4] = y.x; win[p][u][5] = y.y; win[p][u][6] = y.z; win[p][u][7] = y.w;
        }

    u32x4 raw[NGU][3];
    auto load_unit = [&](long long t) {          /* unit t of the run: samples (row0 + t) D .. + D */
        const long long v0 = (row0 + t) * D;
#pragma unroll
        for (int uu = 0; uu < NGU; ++uu)
            a.in.load_group(v0 + 8LL * (tid + uu * NT), raw[uu]);
    };
    auto ring_put = [&](int slot) {
#pragma unroll
        for (int uu = 0; uu < NGU; ++uu)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                ring[(slot * 3 + c) * GU + tid + uu * NT] = raw[uu][c];
    };

    /* the porch: units 0 .. NSL-1 of the run, unit t in slot t */
    for (int t = 0; t < NSL; ++t) {
        load_unit(t);
        ring_put(t);
    }
    load_unit(NSL);
    __syncthreads();                             /* the twiddles are in place */

    int base = 0;                                /* the slot of the row's oldest unit: row mod NSL */
    for (int sl = 0; sl < nr; ++sl) {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int q = u / NGU, uu = u % NGU;
            const int g = tid + u * NT;
            float2 acc[8];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int j = p * Q + q;         /* the unit of the row */
                u32x4 x[3];
                if (j == NSL) {
                    x[0] = raw[uu][0]; x[1] = raw[uu][1]; x[2] = raw[uu][2];
                } else {
                    const int slot = base + j >= NSL ? base + j - NSL : base + j;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        x[c] = ring[(slot * 3 + c) * GU + tid + uu * NT];
                }
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    PDDC_UNPACK_GROUP_MSB(x, h, i0, q0, i1, q1);
                    const float fi0 = (float)i0 * kPackedUnpackScale, fq0 = (float)q0 * kPackedUnpackScale;
                    const float fi1 = (float)i1 * kPackedUnpackScale, fq1 = (float)q1 * kPackedUnpackScale;
                    const float w0 = win[p][u][2 * h], w1 = win[p][u][2 * h + 1];
                    if (p == 0) {
                        acc[2 * h] = make_float2(fi0 * w0, fq0 * w0);
                        acc[2 * h + 1] = make_float2(fi1 * w1, fq1 * w1);
                    } else {
                        acc[2 * h].x = fmaf(fi0, w0, acc[2 * h].x);
                        acc[2 * h].y = fmaf(fq0, w0, acc[2 * h].y);
                        acc[2 * h + 1].x = fmaf(fi1, w1, acc[2 * h + 1].x);
                        acc[2 * h + 1].y = fmaf(fq1, w1, acc[2 * h + 1].y);
                    }
                }
            }
            f32x4 *dst = reinterpret_cast<f32x4 *>(buf);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                f32x4 o;
                o.x = acc[2 * h].x; o.y = acc[2 * h].y; o.z = acc[2 * h + 1].x; o.w = acc[2 * h + 1].y;
                dst[4 * g + (h ^ ((g >> 1) & 3))] = o;
            }
        }
        /* the newest unit takes the oldest one's slot (this thread's own groups: program order is enough) */
        if (NSL > 0) {
            ring_put(base);
            base = base + 1 == NSL ? 0 : base + 1;
        }
        if (sl + 1 < nr)
            load_unit((long long)sl + 1 + NSL);
        __syncthreads();
        spec_pass_mid<M, NT, 16, 1, 0, 1>(buf, tw + TW1);
        spec_pass_mid<M, NT, 16, 16, 1, 2>(buf, tw + TW1);
        const bool neg_odd = Q == 2 && ((a.row_parity + (unsigned)(row0 + sl)) & 1u);
        f32x2 *orow = reinterpret_cast<f32x2 *>(a.out) + (size_t)(row0 + sl) * (size_t)a.count;
        spec_pass_out<M, NT, R2, 256, 2>(buf, tw + TW2, [&](int bin, float2 v) {
            const int i = (bin - a.first) & (M - 1);
            if (neg_odd && (bin & 1))
                v = make_float2(-v.x, -v.y);
            if (i < a.count) {
                f32x2 o;
                o.x = v.x; o.y = v.y;
                __builtin_nontemporal_store(o, orow + i);
            }
        });
    }
}

__global__ __launch_bounds__(256) void k_channelize_tail(PackedCarryArgs p)
{
    PDDC_CARRY_TAIL(p, 0)
}

/* ------------------------------------------------------------------------ */
template <int M, int P, int Q> static hipError_t launch_channelize_t(const ChannelizeArgs &a, hipStream_t s)
{
    constexpr int NT = M / 16 < 256 ? M / 16 : 256;
    const size_t lds = channelize_lds_bytes(M, P, M / Q);
    const long long blocks = (a.nrows + a.run - 1) / a.run;
    return launch_dynamic_lds<&k_channelize<M, P, Q>>(lds, dim3((unsigned)blocks), dim3(NT), lds, s, a);
}

template <int M, int P> static hipError_t launch_channelize_q(int q, const ChannelizeArgs &a, hipStream_t s)
{
    return q == 1 ? launch_channelize_t<M, P, 1>(a, s) : launch_channelize_t<M, P, 2>(a, s);
}

template <int M> static hipError_t launch_channelize_p(int p, int q, const ChannelizeArgs &a, hipStream_t s)
{
    switch (p) {
    case 1: return launch_channelize_q<M, 1>(q, a, s);
    case 2: return launch_channelize_q<M, 2>(q, a, s);
    case 4: return launch_channelize_q<M, 4>(q, a, s);
    case 8:
        if constexpr (8 * M <= kChanMaxProto)
            return launch_channelize_q<M, 8>(q, a, s);
        return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_channelize(int nchan, int taps_per_branch, int hop, const ChannelizeArgs &a, hipStream_t s)
{
    if (a.nrows <= 0 || a.run <= 0 || (hop != nchan && 2 * hop != nchan))
        return hipErrorInvalidValue;
    const int q = nchan / hop;
    switch (nchan) {
    case 1024: return launch_channelize_p<1024>(taps_per_branch, q, a, s);
    case 2048: return launch_channelize_p<2048>(taps_per_branch, q, a, s);
    case 4096: return launch_channelize_p<4096>(taps_per_branch, q, a, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_channelize_tail(const PackedCarryArgs &a, hipStream_t s)
{
    const int blocks = carry_tail_blocks(a.new_len);
    if (blocks <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_channelize_tail, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
