/*
 * ddc_morse.hip -- the Morse decoder: every receiver's complex series through the real envelope filter of its keyer,
 * the block meter and the key decision behind the envelope power, and the element timing behind the key (gfx950 only).
 *
 *   k_morse   per ON receiver j and sample m, with (h, two0, two_min, two_max, shift) of the receiver's keyer:
 *             y = (0, 0); over t = 0 .. W-1 ascending, z = z_j[m - t]: y.re = fmaf(h[t], z.re, y.re); y.im likewise;
 *             p = fmaf(y.im, y.im, y.re y.re); p = 0 unless p <= FLT_MAX; key = p > on ? 1 : (p < off ? 0 : key);
 *             one step of the element timing (ddc_morse_timing.h); the block meter, whose levels govern the next block.
 *             DESIGN.md 8 and include/perseus_ddc.h have the definition.
 *
 * Walk: a block owns G = 4 consecutive receivers, one wave each, and goes through the batch in tiles of TT = 256
 * samples that are aligned to m, the object's sample count, not to the batch: tile k holds the samples with m >> 8 = k,
 * so the first and the last tile of a batch may be partial, and the lanes outside the batch are masked.  The waves share
 * nothing (each has its own row in LDS), the two barriers per tile are there for the reader.
 *   1. the wave stages its receiver's inputs from W - 1 before the tile's first sample of the batch to its last one:
 *      consecutive lanes, consecutive inputs, 8-byte loads; an input before the batch's first comes from the carried
 *      record (zero where the receiver is fresh or cleared).
 *   2. lane l makes the O = 4 outputs l, l + 64, l + 128, l + 192 of the tile, each with accumulators of its own that
 *      meet the taps in ascending t: the bits are the definition's whatever O is.  Per tap and output 8 bytes of LDS
 *      feed 2 fmaf (the compiler reads two outputs, 512 bytes apart, with one ds_read2_b64).  The taps are
 *      wave-uniform: the keyer index goes through readfirstlane and a pass of 8 real taps comes through the scalar
 *      cache into SGPRs; the last pass of a window that is no multiple of 8 tests every tap.
 *   3. output group o of a tile is exactly one meter block (the samples with the same m >> 6), so per group, in order:
 *      the masks p > on and p < off of its 64 samples (__ballot; the thresholds are the same in every lane); lane 0
 *      advances hysteresis and timing from event to event -- with the key up the next event is the lowest set bit of
 *      the on-mask at or behind the position or the emission sample t_up + gap, whichever is first (the emission first
 *      where they meet), with the key down the lowest set bit of the off-mask; the wave reduces the block's hi and lo
 *      (fmaxf / fminf of values that are never NaN: any order gives the same bits); where the block's last sample is
 *      in the batch every lane makes the new pk, fl, on and off for the next group.
 *   After the last tile lane 0 writes the receiver's record and the count, and the wave the new carried inputs, the last
 *   W - 1 of [old record | batch], from global memory into the other buffer.
 * OFF receivers: nothing of z is read; the record goes to the other buffer as it is (or as the host's marks say), the
 *   count is 0, the p row +0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled);
 *   nothing depends on the batch cut, nrx, j's index, the other receivers, the strides or the lane a sample falls into.
 *   No atomics, no scratch.
 * Bounds: z and p are indexed by receivers < nrx and 0 <= i < n only (a tile's samples lo .. hi - 1 with 0 <= o0 + lo and
 *   o0 + hi <= n); the records by receivers < nrx and 0 <= e < W - 1; a staged slot is < W - 1 + TT, a read one lies in
 *   0 .. W - 2 + TT (a masked lane may read a slot nobody staged: inside the wave's own row, and its value is dropped);
 *   the taps are read inside the keyer's morse_row(W) entries; the keyer index is checked by the host; chars[j][c] has
 *   c below char_stride, which the host has tested against the bound of pddc_morse_max_chars (DESIGN.md derives it: the
 *   kernel's own test is never taken).
 */
#include "ddc_morse.h"
#include "ddc_dev.h"
#include "ddc_host.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace pddc {

/* one pass of kMorseStep taps from tap t0; p points at the lane's slot of output 0, tap 0 */
template <bool Guard>
__device__ __forceinline__ void morse_pass(const float2 *p, int t0, int W, const float (&hw)[kMorseStep], float2 (&y)[kMorseOut])
{
#pragma unroll
    for (int s = 0; s < kMorseStep; ++s) {
        if (Guard && t0 + s >= W)
            break;
        const float h = hw[s];
#pragma unroll
        for (int o = 0; o < kMorseOut; ++o) {
            const float2 z = p[64 * o - (t0 + s)];
            y[o].x = fmaf(h, z.x, y[o].x);
            y[o].y = fmaf(h, z.y, y[o].y);
        }
    }
}

/* the meter, the key and the timing as a restart leaves them; the counters stay */
__device__ __forceinline__ void morse_state_restart(MorseState &s, uint32_t two0)
{
    morse_restart(s.t, two0);
    s.key = 0u;
    s.primed = 0u;
    s.hi = 0.0f;
    s.lo = INFINITY;
    s.pk = s.fl = 0.0f;
    s.on = s.off = INFINITY;
}

__global__ __launch_bounds__(kMorseThreads) void k_morse(MorseArgs a)
{
    constexpr int G = kMorseGroup, O = kMorseOut, TT = kMorseTile, U = kMorseStep;
    static_assert(64 == 1 << kMorseBlockLog2, "an output group is a meter block");
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int W = a.window, H = W - 1;
    const int RS = morse_row_slots(W);
    const int j = (int)blockIdx.x * G + wave;
    const bool have = j < a.nrx;
    float2 *row = lds2 + wave * RS;

    MorseRx r{ 0, 0u };
    if (have)
        r = a.rx[j];
    const uint32_t flags = __builtin_amdgcn_readfirstlane(r.flags);
    const int keyer = __builtin_amdgcn_readfirstlane(r.keyer);
    const bool on = have && (flags & kMorseOn);
    const bool fixed = (flags & kMorseFixed) != 0u;
    const bool keep = !(flags & (kMorseFresh | kMorseClear));         /* the carried inputs are read */
    const float2 *zr = a.z + (long long)(have ? j : 0) * a.z_stride;
    const float2 *old = a.hist + (long long)(have ? j : 0) * H;

    /* input idx of the receiver: before the batch's first from the carried record (H values, the newest last) */
    auto input = [&](long long idx) -> float2 {
        if (idx < 0)
            return (keep && idx >= -(long long)H) ? old[H + idx] : make_float2(0.0f, 0.0f);
        return zr[idx];
    };

    const MorseKeyer kp = a.keyers[keyer];
    const MorseParams par = a.par;
    /* the receiver's record, as the host's marks leave it */
    MorseState s{};
    if (have && !(flags & kMorseFresh))
        s = a.state[j];
    if (flags & kMorseMarks)
        morse_state_restart(s, kp.two0);

    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps + (long long)keyer * morse_row(W);
    MorseChar *chars = a.chars + (long long)(have ? j : 0) * a.char_stride;
    uint32_t nch = 0u;

    /* tiles are aligned to m: the first begins at or before the batch's first sample */
    const unsigned long long mtile0 = a.m0 & ~(unsigned long long)(TT - 1);
    const long long base = -(long long)(a.m0 - mtile0);
    for (long long o0 = base; o0 < a.n; o0 += TT) {
        const int lo_i = o0 < 0 ? (int)-o0 : 0;                       /* the tile's samples lo_i .. hi_i - 1 are the batch's */
        const int hi_i = (int)(a.n - o0 < TT ? a.n - o0 : TT);
        if (on)
            for (int e = lo_i + lane; e < H + hi_i; e += 64)
                row[e] = input(o0 - H + e);
        __syncthreads();

        if (on) {
            float2 y[O];
#pragma unroll
            for (int o = 0; o < O; ++o)
                y[o] = make_float2(0.0f, 0.0f);
            const float2 *p = row + H + lane;
            for (int t0 = 0; t0 < W; t0 += U) {
                float hw[U];
#pragma unroll
                for (int i = 0; i < U; ++i)
                    hw[i] = h[t0 + i];
                if (t0 + U <= W)
                    morse_pass<false>(p, t0, W, hw, y);
                else
                    morse_pass<true>(p, t0, W, hw, y);
            }
            const unsigned long long mtile = mtile0 + (unsigned long long)(o0 - base);
#pragma unroll
            for (int o = 0; o < O; ++o) {
                /* the group's samples of the batch: ga .. gb - 1 of its 64 (uniform) */
                const int ga = lo_i - 64 * o > 0 ? lo_i - 64 * o : 0;
                const int gb = hi_i - 64 * o < 64 ? hi_i - 64 * o : 64;
                if (ga >= gb)
                    continue;
                float pw = fmaf(y[o].y, y[o].y, y[o].x * y[o].x);
                if (!(pw <= FLT_MAX))
                    pw = 0.0f;
                const bool valid = lane >= ga && lane < gb;
                if (valid && a.p)
                    a.p[(long long)j * a.p_stride + o0 + 64 * o + lane] = pw;
                const unsigned long long onm = __ballot(valid && pw > s.on);
                const unsigned long long offm = __ballot(valid && pw < s.off);

                if (lane == 0) {
                    const unsigned long long mblk = mtile + (unsigned long long)(64 * o);
                    int pos = ga;
                    while (pos < gb) {
                        if (s.key) {
                            const unsigned long long v = offm & (~0ull << pos);
                            if (!v)
                                break;
                            const int e = __ffsll(v) - 1;
                            morse_fall(s.t, kp, fixed, mblk + (unsigned long long)e);
                            s.key = 0u;
                            pos = e + 1;
                            continue;
                        }
                        const unsigned long long v = onm & (~0ull << pos);
                        const int e = v ? __ffsll(v) - 1 : 64;
                        /* the emission sample, if it lies in pos .. gb - 1 (the key is up: prev = 0 there) */
                        int ei = 64;
                        if (s.t.nel > 0u) {
                            const unsigned long long em = s.t.t_up + morse_gap(s.t.two);
                            if (em >= mblk + (unsigned long long)pos && em - mblk < (unsigned long long)gb)
                                ei = (int)(em - mblk);
                        }
                        if (ei <= e) {
                            if (ei >= gb)
                                break;
                            const MorseChar c = morse_emit(s.t);
                            /* never refused: char_stride is at least the bound the host tests (pddc_morse_max_chars) */
                            if ((long long)nch < a.char_stride)
                                chars[nch++] = c;
                            pos = ei;                                 /* a rising edge may share the sample */
                            continue;
                        }
                        morse_rise(s.t, mblk + (unsigned long long)e);
                        s.key = 1u;
                        pos = e + 1;
                    }
                }

                float vh = valid ? pw : 0.0f, vl = valid ? pw : INFINITY;
#pragma unroll
                for (int x = 32; x > 0; x >>= 1) {
                    vh = fmaxf(vh, __shfl_xor(vh, x));
                    vl = fminf(vl, __shfl_xor(vl, x));
                }
                s.hi = fmaxf(s.hi, vh);
                s.lo = fminf(s.lo, vl);
                if (gb == 64) {                                       /* the block's last sample */
                    if (!s.primed) {
                        s.pk = s.hi;
                        s.fl = s.lo;
                        s.primed = 1u;
                    } else {
                        s.pk = fmaxf(s.hi, fmaf(par.rel, s.fl - s.pk, s.pk));
                        s.fl = fminf(s.lo, fmaf(par.relf, s.pk - s.fl, s.fl));
                    }
                    const float span = s.pk - s.fl;
                    if (s.pk >= par.ratio * s.fl && span > 0.0f) {
                        s.on = fmaf(par.a_on, span, s.fl);
                        s.off = fmaf(par.a_off, span, s.fl);
                    } else
                        s.on = s.off = INFINITY;
                    s.hi = 0.0f;
                    s.lo = INFINITY;
                }
            }
        } else if (have && a.p) {
            for (int i = lo_i + lane; i < hi_i; i += 64)
                a.p[(long long)j * a.p_stride + o0 + i] = 0.0f;
        }
        __syncthreads();
    }

    if (!have)
        return;
    if (lane == 0) {
        a.new_state[j] = s;
        a.counts[j] = nch;
    }
    /* the new carried record: the last W - 1 of [old record | batch]; an OFF receiver's batch is empty */
    const long long used = on ? a.n : 0;
    for (int e = lane; e < H; e += 64)
        a.new_hist[(long long)j * H + e] = input(used - H + e);
}

hipError_t launch_morse(const MorseArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kMorseMaxRx || a.nkeyers < 1 || a.nkeyers > kMorseMaxKeyers || a.window < 1 ||
        a.window > kMorseMaxWindow || !a.z || a.z_stride < a.n || !a.chars || a.char_stride < 1 || !a.counts ||
        (a.p && a.p_stride < a.n) || !a.taps || !a.keyers || !a.rx || !a.state || !a.new_state || !a.hist || !a.new_hist)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nrx + kMorseGroup - 1) / kMorseGroup));
    return launch_dynamic_lds<&k_morse>(kMorseLdsCap, grid, dim3(kMorseThreads), morse_lds_bytes(a.window), s, a);
}

} // namespace pddc
