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
 * Walk: ddc_decoder_dev.h's (steps 1 and 2: stage, filter; the compiler reads two outputs, 512 bytes apart, with one
 * ds_read2_b64), with tiles that are aligned to m, the object's sample count, not
 * to the batch: tile k holds the samples with m >> 8 = k, so the first and the last tile of a batch may be partial;
 * staging begins at the tile's first sample of the batch, and the lanes outside the batch are masked.  The waves share
 * nothing (each has its own row in LDS), the two barriers per tile are there for the reader.  Behind the filter, per tile:
 *   3. output group o of a tile is exactly one meter block (the samples with the same m >> 6), so per group, in order:
 *      the masks p > on and p < off of its 64 samples (__ballot; the thresholds are the same in every lane); lane 0
 *      advances hysteresis and timing from event to event -- with the key up the next event is the lowest set bit of
 *      the on-mask at or behind the position or the emission sample t_up + gap, whichever is first (the emission first
 *      where they meet), with the key down the lowest set bit of the off-mask; the wave reduces the block's hi and lo
 *      (fmaxf / fminf of values that are never NaN: any order gives the same bits); where the block's last sample is
 *      in the batch every lane makes the new pk, fl, on and off for the next group.
 *   After the last tile lane 0 writes the receiver's record and the count.
 * OFF receivers: nothing of z is read; the record goes to the other buffer as it is (or as the host's marks say), the
 *   count is 0, the p row +0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled);
 *   nothing depends on the batch cut, nrx, j's index, the other receivers, the strides or the lane a sample falls into.
 *   No atomics, no scratch.
 * Bounds: the walk's are in ddc_decoder_dev.h; a tile's samples of the batch are lo_i .. hi_i - 1 with 0 <= o0 + lo_i and
 *   o0 + hi_i <= n, hi_i <= TT, so staging (first = lo_i, end = hi_i) reads z at 0 <= idx < n only and a masked lane's
 *   read of a slot nobody staged stays inside the wave's own row, its value dropped (`valid`); the taps are read inside
 *   the keyer's dec_row(W) floats; the keyer index is checked by the host (receiver 0's entry, index 0, where the wave has
 *   none).  Here: p is indexed by receivers < nrx and o0 + 64 o + lane of valid lanes, 0 <= . < n; the state records by
 *   receivers < nrx; chars[j][c] has c below char_stride, which the host has tested against the bound of
 *   pddc_morse_max_chars (DESIGN.md derives it: the kernel's own test is never taken).
 */
#include "ddc_morse.h"
#include "ddc_decoder_dev.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace pddc {

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

__global__ __launch_bounds__(kDecThreads) void k_morse(MorseArgs a)
{
    constexpr int O = kDecOut, TT = kDecTile;
    static_assert(64 == 1 << kMorseBlockLog2, "an output group is a meter block");
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int W = a.window, H = W - 1;
    const DecWave w = dec_wave(a.rx, a.nrx);
    const int lane = w.lane, j = w.j;
    float2 *row = lds2 + w.wave * dec_in_slots(W);

    const bool on = w.have && (w.flags & kDecOn);
    const bool fixed = (w.flags & kMorseFixed) != 0u;
    const DecInput input = dec_input(w, a.z, a.z_stride, a.hist, H, H);

    const MorseKeyer kp = a.bank[w.bank];
    const MorseParams par = a.par;
    /* the receiver's record, as the host's marks leave it */
    MorseState s{};
    if (w.have && !(w.flags & kDecFresh))
        s = a.state[j];
    if (w.flags & kMorseMarks)
        morse_state_restart(s, kp.two0);

    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps + (long long)w.bank * dec_row(W);
    MorseChar *chars = a.chars + (long long)w.jr * a.char_stride;
    uint32_t nch = 0u;

    /* tiles are aligned to m: the first begins at or before the batch's first sample */
    const unsigned long long mtile0 = a.m0 & ~(unsigned long long)(TT - 1);
    const long long base = -(long long)(a.m0 - mtile0);
    for (long long o0 = base; o0 < a.n; o0 += TT) {
        const int lo_i = o0 < 0 ? (int)-o0 : 0;                       /* the tile's samples lo_i .. hi_i - 1 are the batch's */
        const int hi_i = (int)(a.n - o0 < TT ? a.n - o0 : TT);
        if (on)
            dec_stage(row, input, lane, o0, lo_i, hi_i);
        __syncthreads();

        if (on) {
            float2 y[O];
            dec_filter(row, lane, H, W, h, y);
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
        } else if (w.have && a.p) {
            for (int i = lo_i + lane; i < hi_i; i += 64)
                a.p[(long long)j * a.p_stride + o0 + i] = 0.0f;
        }
        __syncthreads();
    }

    if (!w.have)
        return;
    if (lane == 0) {
        a.new_state[j] = s;
        a.counts[j] = nch;
    }
    dec_carry(a.new_hist, H, w, input, on ? a.n : 0);
}

hipError_t launch_morse(const MorseArgs &a, hipStream_t s)
{
    return dec_launch<&k_morse>(a, !a.p || a.p_stride >= a.n, kMorseLdsCap, morse_lds_bytes(a.window), s);
}

} // namespace pddc
