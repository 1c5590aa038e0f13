/*
 * ddc_blanker.hip -- the impulse noise blanker: per receiver a reference power over blocks of B samples, a trigger per
 * sample whose power exceeds the reference times the receiver's threshold, and the series delayed by D = W + R samples
 * with every trigger's neighbourhood taken to zero through a linear ramp (gfx950 only).
 *
 *   k_blanker   per receiver j and sample m: p = re re + im im of z_j[m] summed over blocks of B samples in ascending m;
 *               at a block's end L = s invB and ref = ref + beta (fminf(L, ref cap) - ref), or ref = L while ref is not
 *               positive; t[m] = ON && ref > 0 && p > ref thr; out[n] = z[n - D] g with g = 0 within W samples of a
 *               trigger, (dist - W) invR1 within D, else 1 (z's bits).  DESIGN.md 8 has the definition.
 *
 * Walk: k_squelch's, and the same code where it is the same: the cut of a tile, step 2, the division by B and the next
 * tile's phase are the block meter of ddc_meter_dev.h; steps 1, 3, 4 and 5 are this file's.  A block takes G = 4
 * consecutive receivers and walks the whole batch tile by tile, TT = 256 samples a time; the block grid B is common to the receivers, so a tile is cut into the same SEGMENTS for all of them: segment 0
 * ends the block under way (or the tile), the following ones are whole blocks, the last may be the start of one.
 *   1. thread i takes sample i of the tile for one receiver after the other (coalesced 8-byte loads of z, those of the
 *      NEXT tile issued here and held in registers); p stays in a register and goes to sp[g][i] in LDS.
 *   2. one thread per receiver and segment adds the segment's p in ascending m -- segment 0 continues the carried partial
 *      sum, the others start at 0 -- and leaves L = s invB in sl[g][k] where the segment ends a block, else the partial
 *      sum for the next tile.  Few segments (B >= 4): receiver g's segments on wave g.
 *   3. lane g of wave 0 runs receiver g's ref chain over the segments: per segment it leaves the limit ref thr that holds
 *      for the segment's samples (+inf when OFF or ref is not positive: nothing is greater) in slim[g][k].
 *   4. the triggers: every thread compares its p with its segment's limit, a __ballot per wave and receiver is one
 *      64-bit word of the receiver's BITMAP in LDS: words 0 .. 7 are the 512 trigger bits carried from before the tile
 *      (2 D <= 512 are ever looked at), words 8 .. 11 the tile's.  Bit 512 + i is sample i of the tile.
 *   5. all threads finish: output i has its centre at bit 512 + i - D; the nearest set bit at or after it (count trailing
 *      zeros over at most D / 64 + 2 words) and at or before it (count leading zeros) give dist, dist gives g; z[n - D]
 *      comes from this batch's row, read a second time, or from the carried history where n - D lies before the batch;
 *      one coalesced 8-byte store.  Eight threads per receiver shift the bitmap by the tile's length into the other of
 *      its two buffers: the next tile's carried bits.  The counters are sums of popcounts of ballots.
 *   Nothing is sequential in m except the sums of step 2 and the ref chain, once per block.
 * Bits: every sum is made by one thread adding in ascending m from the carried value or 0, every other value by one
 * thread with the definition's operation sequence (contraction is off in this file), the gate is integer arithmetic on
 * trigger bits, the counters are integer sums, so nothing depends on the batch cut, K, j's index, the other receivers
 * or the tile.  No atomics, no scratch.
 * out never overlaps z (the host refuses it): out[n] is made from z[n - D], which another thread has read or will read.
 * Bounds: z and out are indexed by receivers < nrx and samples < n only (z a second time at n - D >= 0); the carried
 * history by receivers < nrx and entries < D <= 256, the carried bits by words < 8; the LDS rows by samples < TT and
 * segments < TT, the bitmap by words < 12: the centre's word is at most (512 + 255) / 64 = 11, and the scans stop there
 * and at word 0.
 */
#include "ddc_blanker.h"
#include "ddc_meter_dev.h"

#pragma clang fp contract(off)

namespace pddc {

__global__ __launch_bounds__(kBlankerThreads) void k_blanker(BlankerArgs a)
{
    constexpr int G = kBlankerGroup, TT = kBlankerTile, CW = kBlankerCarryWords, MW = kBlankerMapWords;
    constexpr int HD = kBlankerMaxDelay;
    static_assert(G * 64 == kBlankerThreads && TT == kBlankerThreads, "one wave per receiver, one thread per sample");
    static_assert(G * CW <= kBlankerThreads && HD <= kBlankerThreads, "one thread per carried word and history entry");
    __shared__ float sp[G][TT];
    __shared__ float sl[G][TT];
    __shared__ float slim[G][TT];
    __shared__ unsigned long long bm[2][G][MW];
    __shared__ uint32_t sbl[G][TT / 64];
    __shared__ float ssum[2][G];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g0 = (int)blockIdx.x * G;
    const int ng = a.nrx - g0 < G ? a.nrx - g0 : G;
    const uint32_t B = a.B, W = a.W, D = a.D;
    const uint32_t nw = (D + 63u) / 64u + 1u;       /* words a scan of D bits from any bit can touch */

    /* the state lanes: lane g of wave 0 owns receiver g0 + g */
    const bool mine = tid < ng;
    float ref = 0.0f, thr = 0.0f;
    uint32_t triggers = 0u, blanked = 0u;
    bool on = false;
    if (mine) {
        const BlankerRx r = a.rx[g0 + tid];
        thr = r.thr;
        on = (r.flags & kBlankerOn) != 0u;
        float s = 0.0f;
        if (!a.fresh) {
            const BlankerState o = a.old[g0 + tid];
            s = o.s;
            ref = o.ref;
            triggers = o.triggers;
            blanked = o.blanked;
        }
        ssum[0][tid] = s;
    }
    if (tid < G * CW) {
        const int g = tid / CW, w = tid % CW;
        bm[0][g][w] = g < ng && !a.fresh ? a.old_bits[(long long)(g0 + g) * CW + w] : 0ull;
    }

    float2 zc[G];
    for (int g = 0; g < G; ++g) {
        zc[g] = make_float2(0.0f, 0.0f);
        if (g < ng && tid < a.n)
            zc[g] = a.z[(long long)(g0 + g) * a.z_stride + tid];
    }

    uint32_t ph = a.ph0;            /* where in its block the tile's first sample lies */
    int par = 0;
    for (long long o = 0; o < a.n; o += TT, par ^= 1) {
        const uint32_t cnt = (uint32_t)(a.n - o < TT ? a.n - o : TT);
        const long long m = o + tid;
        const bool in = (uint32_t)tid < cnt;
        const MeterCut cut = meter_cut<TT>(cnt, ph, B, a.magic);    /* the tile's segments */
        const uint32_t len0 = cut.len0, nseg = cut.nseg, nblk = cut.nblk;

        /* 1. p of this tile; the next tile's loads */
        float pv[G];
        for (int g = 0; g < G; ++g) {
            pv[g] = 0.0f;
            if (in && g < ng) {
                pv[g] = zc[g].x * zc[g].x + zc[g].y * zc[g].y;
                sp[g][tid] = pv[g];
            }
        }
        const long long mn = m + TT;
        for (int g = 0; g < G; ++g)
            if (g < ng && mn < a.n)
                zc[g] = a.z[(long long)(g0 + g) * a.z_stride + mn];
        __syncthreads();

        /* 2. the segment sums: sp -> sl, ssum */
        meter_sums<G, TT>(cut, B, a.invB, tid, ng, par, sp, sl, ssum);
        __syncthreads();

        /* 3. the ref chain over the segments; the tile before's count of blanked outputs */
        if (mine) {
            if (o)
                for (int w = 0; w < TT / 64; ++w)
                    blanked += sbl[tid][w];
            for (uint32_t k = 0; k < nseg; ++k) {
                slim[tid][k] = on && ref > 0.0f ? ref * thr : __builtin_inff();
                if (k < nblk) {
                    const float L = sl[tid][k];
                    if (ref > 0.0f) {
                        const float x = fminf(L, ref * a.cap);
                        const float d = x - ref;
                        ref = ref + a.beta * d;
                    } else {
                        ref = L;
                    }
                }
            }
        }
        __syncthreads();

        /* 4. the triggers: a ballot per wave is a word of the bitmap */
        {
            const uint32_t i = (uint32_t)tid;
            const uint32_t k = !in || i < len0 ? 0u : 1u + meter_div<TT>(i - len0, B, a.magic);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g >= ng)
                    break;
                const bool t = in && pv[g] > slim[g][k];
                const unsigned long long word = __builtin_amdgcn_ballot_w64(t);
                if (lane == 0)
                    bm[par][g][CW + wave] = word;
            }
        }
        __syncthreads();

        /* 5. the gate, the stores; the bitmap moves on by cnt bits into its other buffer */
        if (mine)
            for (int w = 0; w < TT / 64; ++w)
                triggers += (uint32_t)__popcll(bm[par][tid][CW + w]);
        if (tid < G * CW && tid / CW < ng) {
            const int g = tid / CW;
            const uint32_t at = cnt + 64u * (uint32_t)(tid % CW), w0 = at >> 6, sh = at & 63u;
            const unsigned long long lo = bm[par][g][w0];
            const unsigned long long hi = w0 + 1u < (uint32_t)MW ? bm[par][g][w0 + 1u] : 0ull;
            bm[par ^ 1][g][tid % CW] = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
        }
        const long long c = m - (long long)D;       /* the output's centre, counted from the batch's start */
        float2 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            v[g] = make_float2(0.0f, 0.0f);
            if (in && g < ng) {
                if (c >= 0)
                    v[g] = a.z[(long long)(g0 + g) * a.z_stride + c];
                else if (!a.fresh)
                    v[g] = a.old_hist[(long long)(g0 + g) * HD + ((long long)D + c)];
            }
        }
        const uint32_t q = (uint32_t)(CW * 64) + (uint32_t)tid - D;     /* the centre's bit: >= 256 */
        const uint32_t w0 = q >> 6, b0 = q & 63u;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g >= ng)
                break;
            bool bl = false;
            if (in) {
                const unsigned long long *mp = bm[par][g];
                uint32_t dist = 0xffffu;
                for (uint32_t j = 0; j < nw && w0 + j < (uint32_t)MW; ++j) {
                    unsigned long long x = mp[w0 + j];
                    if (j == 0)
                        x &= ~0ull << b0;
                    if (x) {
                        dist = ((w0 + j) << 6) + (uint32_t)__builtin_ctzll(x) - q;
                        break;
                    }
                }
                for (uint32_t j = 0; j < nw && j <= w0; ++j) {
                    unsigned long long x = mp[w0 - j];
                    if (j == 0)
                        x &= ~0ull >> (63u - b0);
                    if (x) {
                        const uint32_t back = q - (((w0 - j) << 6) + 63u - (uint32_t)__builtin_clzll(x));
                        dist = back < dist ? back : dist;
                        break;
                    }
                }
                float2 r = v[g];
                if (dist <= W) {
                    r = make_float2(0.0f, 0.0f);
                } else if (dist <= D) {
                    const float gain = (float)(dist - W) * a.invR1;
                    r.x = r.x * gain;
                    r.y = r.y * gain;
                }
                bl = dist <= D;
                a.out[(long long)(g0 + g) * a.out_stride + m] = r;
            }
            const unsigned long long word = __builtin_amdgcn_ballot_w64(bl);
            if (lane == 0)
                sbl[g][wave] = (uint32_t)__popcll(word);
        }
        ph = meter_next_phase(cut, ph);
        /* the next tile's step 1 writes sp alone, which nobody reads any more; its barriers come before sl, slim, the
         * partial sums, the bitmap's other buffer and sbl are written or read again */
    }
    __syncthreads();
    if (mine) {
        for (int w = 0; w < TT / 64; ++w)
            blanked += sbl[tid][w];
        BlankerState s;
        s.s = ssum[par][tid];
        s.ref = ref;
        s.triggers = triggers;
        s.blanked = blanked;
        a.new_state[g0 + tid] = s;
    }
    if (tid < G * CW && tid / CW < ng)
        a.new_bits[(long long)(g0 + tid / CW) * CW + tid % CW] = bm[par][tid / CW][tid % CW];
    /* the last D inputs: from this batch, and from the carried ones where the batch is shorter than D */
    if ((uint32_t)tid < D) {
        const long long c = a.n - (long long)D + tid;
        for (int g = 0; g < ng; ++g) {
            float2 h = make_float2(0.0f, 0.0f);
            if (c >= 0)
                h = a.z[(long long)(g0 + g) * a.z_stride + c];
            else if (!a.fresh)
                h = a.old_hist[(long long)(g0 + g) * HD + (tid + a.n)];
            a.new_hist[(long long)(g0 + g) * HD + tid] = h;
        }
    }
}

hipError_t launch_blanker(const BlankerArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kBlankerMaxRx || a.z_stride < a.n || a.out_stride < a.n || !a.z || !a.out ||
        !a.rx || !a.old || !a.new_state || !a.old_hist || !a.new_hist || !a.old_bits || !a.new_bits || a.B < 1u ||
        a.B > (uint32_t)kBlankerMaxBlock || a.ph0 >= a.B || a.W > (uint32_t)kBlankerMaxGuard || a.D < a.W ||
        a.D - a.W > (uint32_t)kBlankerMaxRamp || a.magic != meter_magic(a.B))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nrx + kBlankerGroup - 1) / kBlankerGroup));
    hipLaunchKernelGGL(k_blanker, grid, dim3(kBlankerThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
