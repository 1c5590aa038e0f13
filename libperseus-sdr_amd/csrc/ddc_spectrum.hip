/*
 * ddc_spectrum.hip -- the panorama: averaged power spectrum of the packed ADC stream (gfx950 only).
 *
 *   k_spectrum<N, PEAK>   per segment of N samples: load packed (3 x global_load_dwordx4 per 8 samples), de-interleave
 *                with v_perm, convert (bit-exact pddc_unpack24_f32 values), times the window, N-point transform inside
 *                the workgroup (LDS + registers), |X|^2 added to per-thread per-bin sums.  No float copy of the input
 *                ever reaches HBM: 6 B read per sample, 4*N (8*N with the peak hold) written per BLOCK.
 *   k_spectrum_fold       second pass: the blocks' partial sums into the running sums (double, ascending block order),
 *                the peak partials into the running peak, and the packed tail carried to the next batch (ddc_packed.h).
 *   k_spectrum_read       running sums -> float32 (and the optional clear).
 *
 * Transform, twiddles and LDS images: ddc_fft_dev.h (shared with the channelizer).  The twiddle table lives in LDS beside
 * the data for the whole (persistent) launch -- consecutive lanes read consecutive k, conflict free.  No device sine or
 * cosine, no recurrence.  Bytes and registers per N: DESIGN.md 4 "Panorama".
 *
 * Walk: block b takes segments b, b + G, b + 2G, ... (G = grid) -- neighbouring blocks read neighbouring memory at
 * any moment; the next segment's 48-byte groups are loaded into registers before the present one is transformed.
 * Sums: a thread owns its bins for the whole launch, adds its segments in ascending order, and writes its row of the
 * partial array once; the fold adds the rows in ascending order in double.  No atomics: the bits depend on
 * (nseg, G) alone.
 */
#include "ddc_spectrum.h"
#include "ddc_fft_dev.h"

#include <cmath>

namespace pddc {

/* radices of the passes of size n: 16, 16, r2[, r3]; below the panorama's sizes (FramePlan, ddc_fft_dev.h) 16, 16 and
 * 8, 8, 8 */
static void spec_radices(int n, int (&r)[4], int &np)
{
    r[0] = r[1] = 16;
    r[3] = 1;
    np = 3;
    switch (n) {
    case 256: r[2] = 1; np = 2; break;
    case 512: r[0] = r[1] = r[2] = 8; break;
    case 1024: r[2] = 4; break;
    case 2048: r[2] = 8; break;
    case 4096: r[2] = 16; break;
    default: r[2] = 8; r[3] = 4; np = 4; break;
    }
}

int spectrum_twiddle_len(int nfft)
{
    int r[4], np, len = 0;
    spec_radices(nfft, r, np);
    int ns = r[0];
    for (int p = 1; p < np; ++p) {
        len += (r[p] - 1) * ns;
        ns *= r[p];
    }
    return 2 * len;
}

void spectrum_build_twiddles(int nfft, float *tw)
{
    int r[4], np;
    spec_radices(nfft, r, np);
    int ns = r[0];
    size_t o = 0;
    for (int p = 1; p < np; ++p) {
        for (int q = 1; q < r[p]; ++q)
            for (int k = 0; k < ns; ++k) {
                const double a = -2.0 * M_PI * (double)((long long)q * k) / (double)(ns * r[p]);
                tw[o++] = (float)cos(a);
                tw[o++] = (float)sin(a);
            }
        ns *= r[p];
    }
}

int spectrum_max_blocks(int nfft, int ncu)
{
    const int per = nfft == 1024 ? SpecPlan<1024>::BLOCKS_PER_CU
                    : nfft == 2048 ? SpecPlan<2048>::BLOCKS_PER_CU
                    : nfft == 4096 ? SpecPlan<4096>::BLOCKS_PER_CU
                                   : SpecPlan<8192>::BLOCKS_PER_CU;
    return per * ncu;
}

/* ------------------------------------------------------------------------ */
template <int N, bool PEAK>
__global__ __launch_bounds__(N / 16 < 256 ? N / 16 : 256) void k_spectrum(SpectrumArgs p)
{
    using Plan = SpecPlan<N>;
    constexpr int NT = N / 16 < 256 ? N / 16 : 256;
    constexpr int NG = N / 8 / NT;               /* 48-byte groups a thread loads per segment */
    constexpr int NACC = N / NT;                 /* bins a thread owns */
    constexpr int R2 = Plan::R2, R3 = Plan::R3;
    constexpr int TW1 = 0, TW2 = 15 * 16, TW3 = TW2 + (R2 - 1) * 256, TWN = TW3 + (R3 > 1 ? (R3 - 1) * 256 * R2 : 0);
    extern __shared__ __attribute__((aligned(16))) float2 spec_lds[];
    float2 *buf = spec_lds;                      /* [N] */
    float2 *tw = spec_lds + N;                   /* [TWN] */
    const int tid = threadIdx.x;

    for (int i = tid; i < TWN; i += NT)
        tw[i] = reinterpret_cast<const float2 *>(p.twiddles)[i];
    /* a thread's groups sit at the same place of every segment: its window values stay in registers */
    float win[NG][8];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const f32x4 *w = reinterpret_cast<const f32x4 *>(p.window + 8 * (tid + u * NT));
        const f32x4 a = w[0], b = w[1];
        win[u][0] = a.x; win[u][1] = a.y; win[u][2] = a.z; win[u][3] = a.w;
        win[u][4] = b.x; win[u][5] = b.y; win[u][6] = b.z; win[u][7] = b.w;
    }
    float acc[NACC], pk[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
        acc[i] = pk[i] = 0.0f;

    u32x4 raw[NG][3];
    auto load_seg = [&](long long seg) {
        const long long v0 = seg * p.hop;
#pragma unroll
        for (int u = 0; u < NG; ++u)
            p.in.load_group(v0 + 8LL * (tid + u * NT), raw[u]);
    };

    long long seg = blockIdx.x;
    if (seg < p.nseg)
        load_seg(seg);
    __syncthreads();                             /* the twiddles are in place */
    for (; seg < p.nseg; seg += gridDim.x) {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int g = tid + u * NT;
            f32x4 o[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                PDDC_UNPACK_GROUP_MSB(raw[u], h, i0, q0, i1, q1);
                o[h].x = ((float)i0 * kPackedUnpackScale) * win[u][2 * h];
                o[h].y = ((float)q0 * kPackedUnpackScale) * win[u][2 * h];
                o[h].z = ((float)i1 * kPackedUnpackScale) * win[u][2 * h + 1];
                o[h].w = ((float)q1 * kPackedUnpackScale) * win[u][2 * h + 1];
            }
            f32x4 *dst = reinterpret_cast<f32x4 *>(buf);
#pragma unroll
            for (int h = 0; h < 4; ++h)
                dst[4 * g + (h ^ ((g >> 1) & 3))] = o[h];
        }
        if (seg + gridDim.x < p.nseg)
            load_seg(seg + gridDim.x);
        __syncthreads();
        spec_pass<N, NT, 16, 1, kImgLoaders, 16, false, PEAK>(buf, tw + TW1, acc, pk);
        spec_pass<N, NT, 16, 16, 16, 0, false, PEAK>(buf, tw + TW1, acc, pk);
        if (R3 > 1) {
            spec_pass<N, NT, R2, 256, 0, 0, false, PEAK>(buf, tw + TW2, acc, pk);
            spec_pass<N, NT, (R3 > 1 ? R3 : 4), 256 * R2, 0, 0, true, PEAK>(buf, tw + TW3, acc, pk);
        } else {
            spec_pass<N, NT, R2, 256, 0, 0, true, PEAK>(buf, tw + TW2, acc, pk);
        }
    }
    /* the block's row of partial sums: thread j's bins are j + b NT + r N/R of the last pass */
    constexpr int RL = R3 > 1 ? R3 : R2;
    constexpr int NB = N / RL / NT;
    float *ps = p.part_sum + (size_t)blockIdx.x * N;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int bin = tid + b * NT + r * (N / RL);
            ps[bin] = acc[b * RL + r];
            if (PEAK)
                p.part_peak[(size_t)blockIdx.x * N + bin] = pk[b * RL + r];
        }
}

/* ------------------------------------------------------------------------ */
/* 256 threads: 32 bins x 8 slices of the partial rows; a slice adds its rows in ascending order, then slice 0 adds the
 * eight slice sums in ascending order -- all in double.  Blocks past the bins carry the tail (16-byte copies). */
__global__ __launch_bounds__(256) void k_spectrum_fold(SpectrumFoldArgs p)
{
    __shared__ double ssum[8][32];
    __shared__ float speak[8][32];
    const int nbin_blocks = p.nfft / 32;
    if ((int)blockIdx.x < nbin_blocks) {
        if (p.nparts == 0)
            return;
        const int kk = threadIdx.x & 31, sl = threadIdx.x >> 5;
        const int bin = blockIdx.x * 32 + kk;
        double s = 0.0;
        float m = 0.0f;
        for (int b = sl; b < p.nparts; b += 8) {
            s += (double)p.part_sum[(size_t)b * p.nfft + bin];
            if (p.part_peak)
                m = fmaxf(m, p.part_peak[(size_t)b * p.nfft + bin]);
        }
        ssum[sl][kk] = s;
        speak[sl][kk] = m;
        __syncthreads();
        if (sl == 0) {
            double t = ssum[0][kk];
            float mm = speak[0][kk];
            for (int i = 1; i < 8; ++i) {
                t += ssum[i][kk];
                mm = fmaxf(mm, speak[i][kk]);
            }
            p.acc_sum[bin] += t;
            if (p.part_peak)
                p.acc_peak[bin] = fmaxf(p.acc_peak[bin], mm);
        }
        return;
    }
    PDDC_CARRY_TAIL(p.carry, nbin_blocks)
}

__global__ __launch_bounds__(256) void k_spectrum_read(int nfft, double *acc_sum, float *acc_peak, float *d_sum,
                                                       float *d_peak, int clear)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nfft)
        return;
    if (d_sum)
        d_sum[k] = (float)acc_sum[k];
    if (d_peak && acc_peak)
        d_peak[k] = acc_peak[k];
    if (clear) {
        acc_sum[k] = 0.0;
        if (acc_peak)
            acc_peak[k] = 0.0f;
    }
}

/* ------------------------------------------------------------------------ */
template <int N, bool PEAK> static hipError_t launch_spectrum_t(const SpectrumArgs &a, int blocks, hipStream_t s)
{
    constexpr int NT = N / 16 < 256 ? N / 16 : 256;
    const size_t lds = sizeof(float) * ((size_t)2 * N + (size_t)spectrum_twiddle_len(N));
    return launch_dynamic_lds<&k_spectrum<N, PEAK>>(lds, dim3((unsigned)blocks), dim3(NT), lds, s, a);
}

hipError_t launch_spectrum(int nfft, const SpectrumArgs &a, int blocks, hipStream_t s)
{
    const bool peak = a.part_peak != nullptr;
    switch (nfft) {
    case 1024: return peak ? launch_spectrum_t<1024, true>(a, blocks, s) : launch_spectrum_t<1024, false>(a, blocks, s);
    case 2048: return peak ? launch_spectrum_t<2048, true>(a, blocks, s) : launch_spectrum_t<2048, false>(a, blocks, s);
    case 4096: return peak ? launch_spectrum_t<4096, true>(a, blocks, s) : launch_spectrum_t<4096, false>(a, blocks, s);
    case 8192: return peak ? launch_spectrum_t<8192, true>(a, blocks, s) : launch_spectrum_t<8192, false>(a, blocks, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_spectrum_fold(const SpectrumFoldArgs &a, hipStream_t s)
{
    const int nbin_blocks = a.nfft / 32;
    hipLaunchKernelGGL(k_spectrum_fold, dim3((unsigned)(nbin_blocks + carry_tail_blocks(a.carry.new_len))), dim3(256), 0, s,
                       a);
    return hipGetLastError();
}

hipError_t launch_spectrum_read(int nfft, double *acc_sum, float *acc_peak, float *d_sum, float *d_peak, int clear,
                                hipStream_t s)
{
    hipLaunchKernelGGL(k_spectrum_read, dim3((unsigned)((nfft + 255) / 256)), dim3(256), 0, s, nfft, acc_sum, acc_peak,
                       d_sum, d_peak, clear);
    return hipGetLastError();
}

} // namespace pddc
