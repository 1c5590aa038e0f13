/*
 * ddc_meter_dev.h -- the block power meter of the squelch (ddc_squelch.hip) and the noise blanker (ddc_blanker.hip): how a
 * tile of the walk is cut into segments along the grid of blocks of B samples, and the ordered sums of p over the
 * segments.  Internal; gfx950 only.
 *
 * A block of threads walks G receivers tile by tile, TT samples a time; the grid of B is common to the receivers, so a
 * tile is cut into the same SEGMENTS for all of them: segment 0 ends the block under way (or the tile), the following
 * ones are whole blocks, the last may be the start of one.  The kernels keep p = re re + im im (their step 1) and what
 * they do with a block's level.  The sums are compiled with contraction off wherever a kernel includes this header.
 */
#ifndef PDDC_DDC_METER_DEV_H
#define PDDC_DDC_METER_DEV_H

#include "ddc_dev.h"
#include "ddc_stage_checks.h"

namespace pddc {

/* x / B for x < 2 TT (magic: meter_magic(B), ddc_stage_checks.h): B >= TT has at most one whole block in reach */
template <int TT, int SHIFT = kMeterDivShift>
__device__ __forceinline__ uint32_t meter_div(uint32_t x, uint32_t B, uint32_t magic)
{
    return B >= (uint32_t)TT ? (x >= B ? 1u : 0u) : (x * magic) >> SHIFT;
}

/* a tile's segments: cnt samples; segment 0 has len0 and ends its block if done0; behind it rem samples = full whole
 * blocks and a tail; nseg segments, of which nblk complete a block */
struct MeterCut { uint32_t cnt, len0, rem, full, tail, done0, nseg, nblk; };

/* ph: where in its block the tile's first sample lies */
template <int TT> __device__ __forceinline__ MeterCut meter_cut(uint32_t cnt, uint32_t ph, uint32_t B, uint32_t magic)
{
    MeterCut c;
    c.cnt = cnt;
    c.len0 = cnt < B - ph ? cnt : B - ph;
    c.rem = cnt - c.len0;
    c.full = meter_div<TT>(c.rem, B, magic);
    c.tail = c.rem - c.full * B;
    c.done0 = ph + c.len0 == B ? 1u : 0u;
    c.nseg = 1u + c.full + (c.tail ? 1u : 0u);
    c.nblk = c.done0 + c.full;
    return c;
}

/* ... and where the next tile's does */
__device__ __forceinline__ uint32_t meter_next_phase(const MeterCut &c, uint32_t ph)
{
    return c.rem ? c.tail : (c.done0 ? 0u : ph + c.len0);
}

/* The segment sums of receivers g < ng, between two barriers of the caller: one thread per receiver and segment adds
 * sp[g] in ascending m -- segment 0 from the carried ssum[par][g], the others from 0 -- and leaves L = s invB in sl[g][k]
 * where the segment ends a block, else ssum[par ^ 1][g].  Few segments (B >= 4): receiver g's on wave g, G SIMDs busy. */
template <int G, int TT>
__device__ __forceinline__ void meter_sums(const MeterCut &c, uint32_t B, float invB, int tid, int ng, int par,
                                           const float (&sp)[G][TT], float (&sl)[G][TT], float (&ssum)[2][G])
{
#pragma clang fp contract(off)
    const bool few = c.nseg <= 64u;
    for (int gg = 0; gg < (few ? 1 : ng); ++gg) {
        const int g = few ? tid >> 6 : gg;
        const uint32_t k = few ? (uint32_t)tid & 63u : (uint32_t)tid;
        if (g < ng && k < c.nseg) {
            const uint32_t start = k ? c.len0 + (k - 1u) * B : 0u;
            const uint32_t len = k ? (c.cnt - start < B ? c.cnt - start : B) : c.len0;
            float s = k ? 0.0f : ssum[par][g];
            const float *p = sp[g] + start;
            uint32_t i = 0;
            for (; i + 4u <= len; i += 4u) {
                const float p0 = p[i], p1 = p[i + 1], p2 = p[i + 2], p3 = p[i + 3];
                s = s + p0;
                s = s + p1;
                s = s + p2;
                s = s + p3;
            }
            for (; i < len; ++i)
                s = s + p[i];
            const bool ends = k ? len == B : c.done0 != 0u;
            if (ends)
                sl[g][k] = s * invB;
            if (k == c.nseg - 1u)
                ssum[par ^ 1][g] = ends ? 0.0f : s;
        }
    }
}

} // namespace pddc
#endif
