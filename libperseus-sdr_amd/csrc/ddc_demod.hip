/*
 * ddc_demod.hip -- the demodulator: one real audio series per receiver from the tuner's complex series (gfx950 only).
 *
 *   k_demod   per receiver j and output m: the detector d_j[m] of its mode (AM |z|, FM the angle of z[m] conj(z[m-1])
 *             over pi, SSB the real part of z times the BFO phasor of the exact 32-bit word, nco_lo), then the post
 *             stage of its flags, sequential in m: y[m] = fmaf(rho, y[m-1], d[m] - d[m-1]) (DC block),
 *             e[m] = fmaxf(|y[m]|, lambda e[m-1]), a = y fminf(gmax, target / e[m]) (AGC).  DESIGN.md 8 has the definition.
 *
 * Walk: a block takes G = 4 consecutive receivers.
 * A group with a post stage is walked by ONE block over the whole batch, tile by tile, TT = 256 outputs a time:
 *   1. detect: thread i takes output i of the tile for one receiver after the other (consecutive lanes, consecutive m:
 *      coalesced 8-byte loads; the mode is uniform in the block, so its branch is a scalar one).  The one older z of FM
 *      comes from the lane below (a shuffle), for a wave's lane 0 from memory or, at m = 0, from the carried record.
 *      d goes to sy[g][i] in LDS, rows of TT + 4 floats.
 *   2. lanes 0 .. G-1 of wave 0 run their receiver's recursion over the row, four values per ds_read_b128 / ds_write_b128
 *      (row stride 260 dwords: the G lanes start 4 banks apart, no conflict), the next four read ahead of the chain;
 *      y replaces d in sy, e goes to se.  Only the two chains are sequential: fmaf for y, multiply and max for e.
 *   3. all threads finish: a = y or y fminf(gmax, target / e), one coalesced 4-byte store each.  The division is here,
 *      off the sequential chain.
 *   The recursion lanes keep d, y, e of the last output in registers from tile to tile and write the carried record
 *   (with the batch's last z) at the end.
 * A group without a post stage has nothing sequential: it is cut into runs along m, one block each, no LDS; the thread
 *   that holds the batch's last output writes the carried record.
 * Bits: every value is made by one thread with the same operation sequence whatever the walk (contraction is off in this
 * file; nco_lo spells its own fmaf); so a_j[m] does not depend on the batch cut, K, j's index, the other receivers, the
 * run length or which of the two walks the group takes.  No atomics, no scratch.
 * Bounds: z and out are indexed by receivers < nrx and outputs < n only; a tile row is read up to dword TT + 3, inside
 * its pad.
 */
#include "ddc_demod.h"
#include "ddc_dev.h"

#pragma clang fp contract(off)

namespace pddc {

static constexpr float kInvPi = 0.318309886183790672f;

/* d of one output; zp = z[m-1] (FM only), theta the BFO word (SSB only); `first`: there is no older z, d = 0 */
__device__ __forceinline__ float demod_detect(uint32_t mode, float2 z, float2 zp, bool first, uint32_t theta)
{
    if (mode == 0u)
        return sqrtf(z.x * z.x + z.y * z.y);
    if (mode == 1u) {
        const float pr = z.x * zp.x + z.y * zp.y;       /* p = z conj(zp) */
        const float pi = z.y * zp.x - z.x * zp.y;
        const float d = atan2f(pi, pr) * kInvPi;
        return first ? 0.0f : d;
    }
    float c, s;
    nco_lo(theta, c, s);                                /* c + i s = exp(-i theta) */
    return z.x * c - z.y * s;
}

/* z[m-1] for FM: the lane below holds it; a wave's lane 0 reads it, at m = 0 it is the carried one.  Called by whole
 * waves (the shuffle), `in` says whether this lane has an output */
__device__ __forceinline__ float2 demod_older(const float2 *zr, long long m, bool in, float2 zc, float2 carried)
{
    float2 zp = make_float2(__shfl_up(zc.x, 1), __shfl_up(zc.y, 1));
    if ((threadIdx.x & 63u) == 0u && in)
        zp = m > 0 ? zr[m - 1] : carried;
    return zp;
}

/* one step of the post stage */
__device__ __forceinline__ void demod_post(float d, bool dc, float rho, float lambda, float &dp, float &yp, float &ep,
                                           float &y, float &e)
{
    y = dc ? fmaf(rho, yp, d - dp) : d;
    e = fmaxf(fabsf(y), lambda * ep);
    dp = d;
    yp = y;
    ep = e;
}

__global__ __launch_bounds__(kDemodThreads) void k_demod(DemodArgs a)
{
    constexpr int G = kDemodGroup, TT = kDemodTile, LD = kDemodTile + kDemodPad;
    __shared__ __attribute__((aligned(16))) float sy[G][LD];
    __shared__ __attribute__((aligned(16))) float se[G][LD];
    const int tid = (int)threadIdx.x;
    const int g0 = (int)blockIdx.y * G;
    const int ng = a.nrx - g0 < G ? a.nrx - g0 : G;
    const DemodRx PDDC_CONSTANT *rx = (const DemodRx PDDC_CONSTANT *)a.rx + g0;
    const DemodState PDDC_CONSTANT *old = (const DemodState PDDC_CONSTANT *)a.state + g0;
    uint32_t any = 0u;
    for (int g = 0; g < ng; ++g)
        any |= rx[g].flags;
    const bool post = (any & (kDemodDc | kDemodAgc)) != 0u;

    if (!post) {
        const long long begin = (long long)blockIdx.x * a.run;
        const long long end = begin + a.run < a.n ? begin + a.run : a.n;
        for (long long o = begin; o < end; o += TT) {
            const long long m = o + tid;
            const bool in = m < end;
            for (int g = 0; g < ng; ++g) {
                const DemodRx r{ rx[g].mode, rx[g].beta, rx[g].psi, rx[g].flags };
                const bool fresh = (r.flags & kDemodFresh) != 0u;
                const float2 *zr = a.z + (long long)(g0 + g) * a.z_stride;
                const float2 zc = in ? zr[m] : make_float2(0.0f, 0.0f);
                float2 zp = make_float2(0.0f, 0.0f);
                if (r.mode == 1u)
                    zp = demod_older(zr, m, in, zc, fresh ? make_float2(0.0f, 0.0f) : make_float2(old[g].zx, old[g].zy));
                const float d = demod_detect(r.mode, zc, zp, fresh && m == 0, r.beta * (a.m0 + (uint32_t)m) + r.psi);
                if (in) {
                    a.out[(long long)(g0 + g) * a.out_stride + m] = d;
                    if (m == a.n - 1) {
                        DemodState s{};
                        s.zx = zc.x;
                        s.zy = zc.y;
                        s.d = d;
                        s.y = d;
                        a.new_state[g0 + g] = s;
                    }
                }
            }
        }
        return;
    }
    if (blockIdx.x != 0)
        return;

    /* the recursion lanes: lane g of wave 0 owns receiver g0 + g */
    const bool mine = tid < ng;
    bool dc = false;
    float dp = 0.0f, yp = 0.0f, ep = 0.0f;
    if (mine) {
        const uint32_t f = a.rx[g0 + tid].flags;
        dc = (f & kDemodDc) != 0u;
        if (!(f & kDemodFresh)) {
            const DemodState s = a.state[g0 + tid];
            dp = s.d;
            yp = s.y;
            ep = s.e;
        }
    }
    for (long long o = 0; o < a.n; o += TT) {
        const int cnt = (int)(a.n - o < TT ? a.n - o : TT);
        const long long m = o + tid;
        const bool in = tid < cnt;
        for (int g = 0; g < ng; ++g) {
            const DemodRx r{ rx[g].mode, rx[g].beta, rx[g].psi, rx[g].flags };
            const bool fresh = (r.flags & kDemodFresh) != 0u;
            const float2 *zr = a.z + (long long)(g0 + g) * a.z_stride;
            const float2 zc = in ? zr[m] : make_float2(0.0f, 0.0f);
            float2 zp = make_float2(0.0f, 0.0f);
            if (r.mode == 1u)
                zp = demod_older(zr, m, in, zc, fresh ? make_float2(0.0f, 0.0f) : make_float2(old[g].zx, old[g].zy));
            const float d = demod_detect(r.mode, zc, zp, fresh && m == 0, r.beta * (a.m0 + (uint32_t)m) + r.psi);
            if (in)
                sy[g][tid] = d;
        }
        __syncthreads();
        if (mine) {
            float *py = sy[tid], *pe = se[tid];
            int k = 0;
            float4 cur = *reinterpret_cast<const float4 *>(py);
            for (; k + 4 <= cnt; k += 4) {
                const float4 nxt = *reinterpret_cast<const float4 *>(py + k + 4);    /* <= TT: the row's pad */
                float4 y4, e4;
                demod_post(cur.x, dc, a.rho, a.lambda, dp, yp, ep, y4.x, e4.x);
                demod_post(cur.y, dc, a.rho, a.lambda, dp, yp, ep, y4.y, e4.y);
                demod_post(cur.z, dc, a.rho, a.lambda, dp, yp, ep, y4.z, e4.z);
                demod_post(cur.w, dc, a.rho, a.lambda, dp, yp, ep, y4.w, e4.w);
                *reinterpret_cast<float4 *>(py + k) = y4;
                *reinterpret_cast<float4 *>(pe + k) = e4;
                cur = nxt;
            }
            for (; k < cnt; ++k) {
                float y, e;
                demod_post(py[k], dc, a.rho, a.lambda, dp, yp, ep, y, e);
                py[k] = y;
                pe[k] = e;
            }
        }
        __syncthreads();
        if (in) {
            for (int g = 0; g < ng; ++g) {
                const float y = sy[g][tid];
                float v = y;
                if (rx[g].flags & kDemodAgc)
                    v = y * fminf(a.gmax, a.target / se[g][tid]);
                a.out[(long long)(g0 + g) * a.out_stride + m] = v;
            }
        }
        __syncthreads();
    }
    if (mine) {
        DemodState s{};
        const float2 zl = a.z[(long long)(g0 + tid) * a.z_stride + (a.n - 1)];
        s.zx = zl.x;
        s.zy = zl.y;
        s.d = dp;
        s.y = yp;
        s.e = ep;
        a.new_state[g0 + tid] = s;
    }
}

hipError_t launch_demod(const DemodArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kDemodMaxRx || a.run <= 0 || a.run % kDemodTile || a.z_stride < a.n ||
        a.out_stride < a.n || !a.z || !a.out || !a.rx || !a.state || !a.new_state)
        return hipErrorInvalidValue;
    const long long nx = (a.n + a.run - 1) / a.run;
    if (nx > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nx, (unsigned)((a.nrx + kDemodGroup - 1) / kDemodGroup));
    hipLaunchKernelGGL(k_demod, grid, dim3(kDemodThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
