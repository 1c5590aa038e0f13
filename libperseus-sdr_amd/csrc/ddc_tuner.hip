/*
 * ddc_tuner.hip -- the tuner: K freely tuned narrowband receivers behind the channelizer's rows (gfx950 only).
 *
 *   k_tune<G>      per receiver j (word F_j -> channel k_j, residue r_j, phase offset phi_j) and row s:
 *                  z_j[s] = y[s][k_j] exp(-2 pi i (r_j (s D) + phi_j) / 2^32), the phase word in exact 32-bit arithmetic
 *                  (nco_lo, ddc_dev.h); out_j[m] = sum_{t<T} h[t] z_j[m R + T - 1 - t].
 *   k_tune_carry   the z values of the rows the next batch's first outputs still need (< T of them per receiver),
 *                  double-buffered by the host.  The carried state is z, not rows: a retune or another channel range
 *                  between two batches then leaves what was carried as it was, which is the definition.
 *
 * Walk: the receivers are sorted by column; a block takes G consecutive ones and a RUN of consecutive outputs, tile by
 * tile.  A tile is `co` outputs: its (co - 1) R + T rows of z for the G receivers lie in LDS, [row][G] float2.  Loading,
 * thread (g, i) takes receiver g of rows i, i + 256/G, ..: consecutive lanes, consecutive sorted receivers of one row
 * (8 useful bytes each; neighbours share cache lines), eight loads in flight per thread, each mixed and written to LDS
 * once.  A run's first tile loads its T - 1 older rows as well (the porch: recomputed from the matrix or, at the head
 * of a batch, read from the carried z); between two tiles the last T - R rows are moved to the tile's front.  Then
 * every thread runs whole outputs: ascending t, one fmaf chain per component, h through the scalar cache, z by
 * ds_read_b64 at constant offsets (a half wave reads one row of G = 32 receivers: 64 banks, no conflict).
 * Bits: z depends on (s, j's word and phase offset, the row's value) alone and is computed by one function (tune_z)
 * wherever it is needed; an output is one thread's sum in a fixed order.  So out_j[m] does not depend on the batch cut,
 * the number or order of receivers, the channel range, G, the tile or the run length.  No atomics, no scratch.
 * Bounds: a row is read only if u < off + nrows (u - off >= 0 holds for every u >= 0 the host hands out); the table and
 * the output are indexed by receivers < nrx only.
 */
#include "ddc_tuner.h"
#include "ddc_dev.h"

namespace pddc {

/* y exp(-2 pi i theta / 2^32), theta = res sd + phi (mod 2^32), sd = (s D) mod 2^32.  One multiply and one fused
 * multiply-add per component, written out so that every caller gets the same bits (no contraction left to the compiler) */
__device__ __forceinline__ float2 tune_z(float2 y, int32_t res, uint32_t phi, uint32_t sd)
{
#pragma clang fp contract(off)
    float c, s;
    nco_lo((uint32_t)res * sd + phi, c, s);       /* c + i s = exp(-i theta) */
    const float a = y.y * s, b = y.y * c;
    return make_float2(fmaf(y.x, c, -a), fmaf(y.x, s, b));
}

int tune_group(int ntaps) { return ntaps <= 128 ? 32 : 8; }

int tune_tile_outputs(int ntaps, int decim)
{
    const int g = tune_group(ntaps);
    const int max_rows = (int)(kTuneLdsBytes / (sizeof(float2) * (size_t)g));     /* 256 or 1024 >= 2 ntaps */
    const int per_pass = kTuneThreads / g;
    int co = (max_rows - ntaps) / decim + 1;
    if (co >= per_pass)
        co -= co % per_pass;
    return co;
}

template <int G> __global__ __launch_bounds__(kTuneThreads) void k_tune(TuneArgs a)
{
    constexpr int NT = kTuneThreads, OP = NT / G, U = 8, KEEP = 16;
    static_assert(NT % G == 0 && (kTuneMaxTaps - 1) * 8 <= KEEP * NT && 127 * 32 <= KEEP * NT, "k_tune: the kept rows fit KEEP per thread");
    extern __shared__ __attribute__((aligned(16))) float2 tune_lds[];      /* [(co - 1) R + T][G] */
    const int tid = threadIdx.x, gl = tid % G, rl = tid / G;
    const int T = a.ntaps, R = a.decim;
    const long long o_begin = (long long)blockIdx.x * a.run;
    if (o_begin >= a.nout)
        return;
    const long long o_end = o_begin + a.run < a.nout ? o_begin + a.run : a.nout;
    const int gi = (int)blockIdx.y * G + gl;
    const bool live = gi < a.nrx;
    TuneRx me{ 0, 0, 0u, 0 };
    if (live)
        me = a.rx[gi];
    const float2 *col = a.rows + me.col;
    const float2 *car = a.carry + (long long)me.rx * a.carry_cap;
    float2 *dst = a.out + (long long)me.rx * a.out_stride;
    const long long ulim = a.off + a.nrows;
    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps;

    int have = 0;                                 /* rows of the tile that are in place, counted from its row 0 */
    for (long long o = o_begin; o < o_end; o += a.co) {
        const int co = (int)(o_end - o < a.co ? o_end - o : a.co);
        const long long u0 = o * R;               /* the tile's row 0 */
        const int need = (co - 1) * R + T;
        for (int i0 = have + rl; i0 < need; i0 += OP * U) {
            float2 y[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int i = i0 + k * OP;
                const long long u = u0 + i;
                y[k] = make_float2(0.0f, 0.0f);
                if (live && i < need && u < ulim)
                    y[k] = u < a.off ? car[u] : col[(u - a.off) * a.count];
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int i = i0 + k * OP;
                const long long u = u0 + i;
                if (i < need)
                    tune_lds[i * G + gl] = u < a.off ? y[k] : tune_z(y[k], me.res, me.phi, a.phase0 + (uint32_t)u * a.hop);
            }
        }
        __syncthreads();
        for (int oo = rl; oo < co; oo += OP) {
            const float2 *p = tune_lds + (oo * R) * G + gl;
            float ax = 0.0f, ay = 0.0f;
#pragma unroll 8
            for (int t = 0; t < T; ++t) {
                const float2 z = p[(T - 1 - t) * G];
                const float ht = h[t];
                ax = fmaf(ht, z.x, ax);
                ay = fmaf(ht, z.y, ay);
            }
            if (live)
                dst[o + oo] = make_float2(ax, ay);
        }
        __syncthreads();
        have = T > R ? T - R : 0;
        if (have && o + co < o_end) {             /* the rows the next tile shares with this one go to its front */
            const int n = have * G;
            const float2 *src = tune_lds + co * R * G;
            float2 keep[KEEP];
#pragma unroll
            for (int k = 0; k < KEEP; ++k) {
                const int e = tid + k * NT;
                keep[k] = e < n ? src[e] : make_float2(0.0f, 0.0f);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KEEP; ++k) {
                const int e = tid + k * NT;
                if (e < n)
                    tune_lds[e] = keep[k];
            }
        }
    }
}

__global__ __launch_bounds__(kTuneThreads) void k_tune_carry(TuneCarryArgs c)
{
    const int i = (int)blockIdx.x * kTuneThreads + (int)threadIdx.x;
    const int q = (int)blockIdx.y;
    if (i >= c.t.nrx || q >= c.new_len)
        return;
    const TuneRx me = c.t.rx[i];
    const long long u = c.keep_u + q;
    float2 z;
    if (u < c.t.off)
        z = c.t.carry[(long long)me.rx * c.t.carry_cap + u];
    else if (u < c.t.off + c.t.nrows)
        z = tune_z(c.t.rows[(u - c.t.off) * c.t.count + me.col], me.res, me.phi, c.t.phase0 + (uint32_t)u * c.t.hop);
    else
        return;
    c.new_carry[(long long)me.rx * c.t.carry_cap + q] = z;
}

/* ------------------------------------------------------------------------ */
hipError_t launch_tune(const TuneArgs &a, hipStream_t s)
{
    if (a.nout <= 0 || a.run <= 0 || a.co <= 0 || a.run % a.co || a.nrx <= 0 || a.ntaps < 1 || a.ntaps > kTuneMaxTaps ||
        a.decim < 1 || a.decim > kTuneMaxDecim || a.co != tune_tile_outputs(a.ntaps, a.decim))
        return hipErrorInvalidValue;
    const int g = tune_group(a.ntaps);
    const size_t lds = sizeof(float2) * (size_t)g * (size_t)((a.co - 1) * a.decim + a.ntaps);
    if (lds > kTuneLdsBytes)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nout + a.run - 1) / a.run), (unsigned)((a.nrx + g - 1) / g));
    if (g == 32)
        hipLaunchKernelGGL(k_tune<32>, grid, dim3(kTuneThreads), lds, s, a);
    else
        hipLaunchKernelGGL(k_tune<8>, grid, dim3(kTuneThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_tune_carry(const TuneCarryArgs &a, hipStream_t s)
{
    if (a.new_len <= 0)
        return hipSuccess;
    if (a.new_len > a.t.carry_cap || a.t.nrx <= 0 || a.keep_u < 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.t.nrx + kTuneThreads - 1) / kTuneThreads), (unsigned)a.new_len);
    hipLaunchKernelGGL(k_tune_carry, grid, dim3(kTuneThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
