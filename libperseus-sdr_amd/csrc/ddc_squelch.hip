/*
 * ddc_squelch.hip -- the squelch: per receiver a level meter over blocks of B samples, an open / closed decision with
 * hysteresis per block, and the audio gated through a linear ramp (gfx950 only).
 *
 *   k_squelch   per receiver j and sample m: p = re re + im im of z_j[m] summed over blocks of B samples in ascending m;
 *               at a block's end L = s invB, the floor f = fminf(L, f up) while closed, the thresholds (times f with
 *               RELATIVE), the run counters against attack / hang; per sample the ramp counter c steps towards R (open,
 *               or no GATE) or 0, and out = a g with g = 1, c invR or out = +0.  DESIGN.md 8 has the definition.
 *
 * Walk: a block takes G = 4 consecutive receivers and walks the whole batch tile by tile, TT = 256 samples a time.  The
 * block grid B of the level meter is common to the receivers, so a tile is cut into the same SEGMENTS for all of them:
 * segment 0 ends the block under way (or the tile), the following ones are whole blocks, the last may be the start of
 * one.  At most TT segments (B = 1).  The cut, step 2, the division by B and the next tile's phase: ddc_meter_dev.h.
 *   1. thread i takes sample i of the tile for one receiver after the other (coalesced 8-byte loads of z and 4-byte
 *      loads of a, those of the NEXT tile issued here and held in registers); p goes to sp[g][i] in LDS.
 *   2. one thread per receiver and segment adds the segment's p in ascending m -- segment 0 continues the carried partial
 *      sum, the others start at 0 -- and leaves L = s invB in sl[g][k] where the segment ends a block, else the partial
 *      sum for the next tile.  Few segments (B >= 4): receiver g's segments on wave g, so the four chains run on four SIMDs.
 *   3. lane g of wave 0 runs receiver g's state machine over the segments: it leaves per segment the ramp counter at the
 *      segment's start with the target (sc[g][k]), steps the counter over the segment in closed form, and where the
 *      segment ends a block takes the decision and leaves the state in so[g][k].
 *   4. all threads finish: c = clamp(c_start +- offset), g, one coalesced 4-byte store each; the tile's levels and
 *      states are stored coalesced from sl and so.
 *   The state lanes keep f, level, peak, open, run, opens, c in registers from tile to tile and write the carried record
 *   at the end.
 * Bits: every sum is made by one thread adding in ascending m from the carried value or 0, every other value by one
 * thread with the definition's operation sequence (contraction is off in this file), so nothing depends on the batch
 * cut, K, j's index, the other receivers or the tile.  No atomics, no scratch.
 * In place (out == a): a thread reads a[m] of the next tile before any thread stores out of this one, and stores out[m]
 * only at the m it has read.
 * Bounds: z, a and out are indexed by receivers < nrx and samples < n only; level and state by blocks < the launch's
 * count, which the host checked against blk_stride; the LDS rows by samples < TT and segments < TT.
 */
#include "ddc_squelch.h"
#include "ddc_meter_dev.h"

#pragma clang fp contract(off)

namespace pddc {

__global__ __launch_bounds__(kSquelchThreads) void k_squelch(SquelchArgs a)
{
    constexpr int G = kSquelchGroup, TT = kSquelchTile;
    static_assert(G * 64 == kSquelchThreads && TT == kSquelchThreads, "one wave per receiver, one thread per sample");
    __shared__ float sp[G][TT];
    __shared__ float sl[G][TT];
    __shared__ uint32_t sc[G][TT];
    __shared__ uint8_t so[G][TT];
    __shared__ float ssum[2][G];
    const int tid = (int)threadIdx.x;
    const int g0 = (int)blockIdx.x * G;
    const int ng = a.nrx - g0 < G ? a.nrx - g0 : G;
    const uint32_t B = a.B, R = a.R;

    /* the state lanes: lane g of wave 0 owns receiver g0 + g */
    const bool mine = tid < ng;
    float f = __builtin_inff(), level = 0.0f, peak = 0.0f, othr = 0.0f, cthr = 0.0f;
    uint32_t open = 0u, run = 0u, opens = 0u, c = 0u;
    bool gate = false, rel = false;
    if (mine) {
        const SquelchRx r = a.rx[g0 + tid];
        othr = r.open_thr;
        cthr = r.close_thr;
        gate = (r.flags & kSquelchGate) != 0u;
        rel = (r.flags & kSquelchRelative) != 0u;
        c = r.c0;
        float s = 0.0f;
        if (!a.fresh) {
            const SquelchState o = a.old[g0 + tid];
            s = o.s;
            f = o.f;
            level = o.level;
            peak = a.clear_peak ? 0.0f : o.peak;
            open = o.open;
            run = o.run;
            opens = o.opens;
            c = o.c;
        }
        ssum[0][tid] = s;
    }

    float2 zc[G];
    float ac[G];
    for (int g = 0; g < G; ++g) {
        zc[g] = make_float2(0.0f, 0.0f);
        ac[g] = 0.0f;
        if (g < ng && tid < a.n) {
            zc[g] = a.z[(long long)(g0 + g) * a.z_stride + tid];
            ac[g] = a.a[(long long)(g0 + g) * a.a_stride + tid];
        }
    }

    uint32_t ph = a.ph0;            /* where in its block the tile's first sample lies */
    long long kb0 = 0;              /* blocks completed before this tile               */
    int par = 0;
    for (long long o = 0; o < a.n; o += TT, par ^= 1) {
        const uint32_t cnt = (uint32_t)(a.n - o < TT ? a.n - o : TT);
        const long long m = o + tid;
        const bool in = (uint32_t)tid < cnt;
        const MeterCut cut = meter_cut<TT>(cnt, ph, B, a.magic);    /* the tile's segments */
        const uint32_t len0 = cut.len0, nseg = cut.nseg, nblk = cut.nblk;

        /* 1. p of this tile; the next tile's loads */
        float av[G];
        for (int g = 0; g < G; ++g) {
            av[g] = ac[g];
            if (in && g < ng)
                sp[g][tid] = zc[g].x * zc[g].x + zc[g].y * zc[g].y;
        }
        const long long mn = m + TT;
        for (int g = 0; g < G; ++g)
            if (g < ng && mn < a.n) {
                zc[g] = a.z[(long long)(g0 + g) * a.z_stride + mn];
                ac[g] = a.a[(long long)(g0 + g) * a.a_stride + mn];
            }
        __syncthreads();

        /* 2. the segment sums: sp -> sl, ssum */
        meter_sums<G, TT>(cut, B, a.invB, tid, ng, par, sp, sl, ssum);
        __syncthreads();

        /* 3. the state machine over the segments */
        if (mine) {
            for (uint32_t k = 0; k < nseg; ++k) {
                const uint32_t start = k ? len0 + (k - 1u) * B : 0u;
                const uint32_t len = k ? (cnt - start < B ? cnt - start : B) : len0;
                const bool rise = open != 0u || !gate;
                sc[tid][k] = c | (rise ? 0x80000000u : 0u);
                c = rise ? (c + len < R ? c + len : R) : (c > len ? c - len : 0u);
                if (k < nblk) {
                    const float L = sl[tid][k];
                    if (!open)
                        f = fminf(L, f * a.up);
                    const float to = rel ? f * othr : othr;
                    const float tc = rel ? f * cthr : cthr;
                    if (!open) {
                        run = L >= to ? run + 1u : 0u;
                        if (run >= a.attack) {
                            open = 1u;
                            run = 0u;
                            ++opens;
                        }
                    } else {
                        run = !(L >= tc) ? run + 1u : 0u;
                        if (run >= a.hang) {
                            open = 0u;
                            run = 0u;
                        }
                    }
                    peak = fmaxf(peak, L);
                    level = L;
                    so[tid][k] = (uint8_t)open;
                }
            }
        }
        __syncthreads();

        /* 4. the samples' gain, the stores */
        if (in) {
            const uint32_t i = (uint32_t)tid;
            const uint32_t k = i < len0 ? 0u : 1u + meter_div<TT>(i - len0, B, a.magic);
            const uint32_t off = k ? i - (len0 + (k - 1u) * B) + 1u : i + 1u;
            for (int g = 0; g < ng; ++g) {
                const uint32_t w = sc[g][k];
                const uint32_t cs = w & 0x7fffffffu;
                const uint32_t cm = (w >> 31) ? (cs + off < R ? cs + off : R) : (cs > off ? cs - off : 0u);
                float v = av[g];
                if (cm != R)
                    v = cm == 0u ? 0.0f : v * ((float)cm * a.invR);
                a.out[(long long)(g0 + g) * a.out_stride + m] = v;
            }
        }
        if ((uint32_t)tid < nblk) {
            for (int g = 0; g < ng; ++g) {
                const long long at = (long long)(g0 + g) * a.blk_stride + kb0 + tid;
                if (a.level)
                    a.level[at] = sl[g][tid];
                if (a.state)
                    a.state[at] = so[g][tid];
            }
        }
        kb0 += nblk;
        ph = meter_next_phase(cut, ph);
        /* the next tile's step 1 writes sp alone, which nobody reads any more; its barrier comes before sl, sc, so and
         * the partial sums are written again */
    }
    if (mine) {
        SquelchState s;
        s.s = ssum[par][tid];
        s.f = f;
        s.level = level;
        s.peak = peak;
        s.open = open;
        s.run = run;
        s.opens = opens;
        s.c = c;
        a.new_state[g0 + tid] = s;
    }
}

hipError_t launch_squelch(const SquelchArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kSquelchMaxRx || a.z_stride < a.n || a.a_stride < a.n || a.out_stride < a.n ||
        !a.z || !a.a || !a.out || !a.rx || !a.old || !a.new_state || a.B < 1u || a.B > (uint32_t)kSquelchMaxBlock ||
        a.ph0 >= a.B || a.R < 1u || a.R > (uint32_t)kSquelchMaxRamp || a.attack < 1u || a.hang < 1u ||
        a.magic != meter_magic(a.B))
        return hipErrorInvalidValue;
    if ((a.level || a.state) && (unsigned long long)a.blk_stride < ((unsigned long long)a.ph0 + (unsigned long long)a.n) / a.B)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nrx + kSquelchGroup - 1) / kSquelchGroup));
    hipLaunchKernelGGL(k_squelch, grid, dim3(kSquelchThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
