/*
 * ddc_psk.hip -- the PSK decoder: every receiver's complex series through the real matched filter of its modem, a symbol
 * clock that follows the envelope at the phase reversals, the differential decision and the Varicode framing behind it
 * (gfx950 only).
 *
 *   k_psk     per ON receiver j and sample m, with (h, inc, q, step) of the receiver's modem:
 *             y = (0, 0); over t = 0 .. W-1 ascending, z = z_j[m - t]: y.re = fmaf(h[t], z.re, y.re); y.im likewise;
 *             p = fmaf(y.im, y.im, y.re y.re); one step of the clock, and on a strobe the pair (y[m - q], the previous
 *             strobe's), d, x, the bit, on a reversal the early / late correction from p[m] and p[m - 2 q], and the
 *             framing (ddc_psk_bits.h).  DESIGN.md 8 and include/perseus_ddc.h have the definition.
 *
 * Walk: ddc_decoder_dev.h's (steps 1 and 2: stage, filter), tiles from the batch's
 * first sample.  The waves share nothing (each has its own row in LDS: the input row, then B = 128 filter outputs before
 * the tile and the tile's), the barriers are there for the reader and for the order of a wave's own LDS traffic.
 * Behind the filter, per tile:
 *   3. the outputs go to the row's second part, behind the B outputs before the tile (2 q <= B of them are looked
 *      at); p is made from y where it is wanted, with the definition's one operation sequence.
 *   4. lane 0 walks the tile's strobes from one to the next: the clock jumps (~acc) / inc + 1 samples at once; a
 *      strobe reads y at m - q, m and m - 2 q from LDS.  Characters and (d, x) pairs go to global memory as they come.
 *   5. the wave moves the last B outputs of [the B before | the tile] to the front for the next tile.
 *   After the last tile lane 0 writes the receiver's record and the counts, and the wave, behind the walk's carried
 *   inputs, the B outputs in front of the row into the other buffer.
 *   y[m] is a function of the inputs alone, so a carried output has the bits a longer batch would have made.
 * OFF receivers: nothing of z is read; the record goes to the other buffer as it is (or as the host's marks say), the
 *   counts are 0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled);
 *   nothing depends on the batch cut, nrx, j's index, the other receivers, the strides or the lane a sample falls into.
 *   No atomics, no scratch.
 * Bounds: the walk's are in ddc_decoder_dev.h (staging ends at the tile's last sample, hi <= TT; a receiver's carried
 *   record has psk_hist_slots(W) = W - 1 + B float2, the inputs first; the taps are read inside the modem's dec_row(W)
 *   floats; the modem index is checked by the host).  Here: the records' outputs are read and written at W - 1 + e with
 *   0 <= e < B, of receivers < nrx; an output slot is B + i with 0 <= i < hi <= TT, a strobe reads B + i, B + i - q and
 *   B + i - 2 q >= 0 since 2 q <= B (the host tests q); the move reads hi + e < TT + B; chars[j][c] and sym[j][c] have c
 *   below their strides, which the host has tested against the bounds of pddc_psk_max_chars and pddc_psk_max_syms
 *   (DESIGN.md derives them: the kernel's own test is never taken).
 */
#include "ddc_psk.h"
#include "ddc_decoder_dev.h"

#pragma clang fp contract(off)

namespace pddc {

__device__ __forceinline__ float psk_power(float2 y) { return fmaf(y.y, y.y, y.x * y.x); }

/* the clock, the pair and the framing as a restart leaves them; the counters stay */
__device__ __forceinline__ void psk_state_restart(PskState &s)
{
    psk_frame_restart(s.f);
    s.acc = 0u;
    s.vr = s.vi = s.pv = 0.0f;
    s.d_last = s.x_last = 0.0f;
}

__global__ __launch_bounds__(kDecThreads) void k_psk(PskArgs a)
{
    constexpr int O = kDecOut, TT = kDecTile, B = kPskBack;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int W = a.window, H = W - 1;
    const DecWave w = dec_wave(a.rx, a.nrx);
    const int lane = w.lane, j = w.j;
    const int HS = psk_hist_slots(W);
    float2 *row = lds2 + w.wave * psk_row_slots(W);
    float2 *yb = row + dec_in_slots(W);                                /* B outputs before the tile, then the tile's */

    const bool on = w.have && (w.flags & kDecOn);
    const DecInput input = dec_input(w, a.z, a.z_stride, a.hist, HS, H);
    const bool keep = input.keep;

    const PskModem mp = a.bank[w.bank];
    const uint32_t inc = mp.inc, step = mp.step;
    const int q = (int)mp.q;
    /* the receiver's record, as the host's marks leave it */
    PskState s{};
    if (w.have && !(w.flags & kDecFresh))
        s = a.state[j];
    if (w.flags & kPskMarks)
        psk_state_restart(s);

    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps + (long long)w.bank * dec_row(W);
    PskChar *chars = a.chars + (long long)w.jr * a.char_stride;
    float2 *sym = a.sym ? a.sym + (long long)w.jr * a.sym_stride : nullptr;
    uint32_t nch = 0u, nsy = 0u;

    /* the B outputs before the batch's first */
    for (int e = lane; e < B; e += 64)
        yb[e] = (w.have && keep) ? input.old[H + e] : make_float2(0.0f, 0.0f);

    for (long long o0 = 0; o0 < a.n; o0 += TT) {
        const int hi = (int)(a.n - o0 < TT ? a.n - o0 : TT);          /* the tile's samples 0 .. hi - 1 */
        if (on)
            dec_stage(row, input, lane, o0, 0, hi);
        __syncthreads();

        if (on) {
            float2 y[O];
            dec_filter(row, lane, H, W, h, y);
#pragma unroll
            for (int o = 0; o < O; ++o)
                if (64 * o + lane < hi)
                    yb[B + 64 * o + lane] = y[o];
        }
        __syncthreads();

        if (on && lane == 0) {
            const unsigned long long mtile = a.m0 + (unsigned long long)o0;
            uint32_t pos = 0u;
            for (;;) {
                const uint32_t left = (uint32_t)hi - pos;
                const uint64_t jump = psk_jump(s.acc, inc);
                if (jump > left) {
                    s.acc = psk_advance(s.acc, inc, left);
                    break;
                }
                const uint32_t k = (uint32_t)jump;                    /* <= left <= TT */
                s.acc = psk_advance(s.acc, inc, k);
                const int i = (int)(pos + k - 1u);                    /* the strobe's sample, the late one */
                pos += k;
                const float2 u = yb[B + i - q];
                const float pu = psk_power(u);
                const float dot = fmaf(u.y, s.vi, u.x * s.vr);
                const float cross = fmaf(u.y, s.vr, -(u.x * s.vi));
                const float sum = pu + s.pv;
                const float d = sum > 0.0f ? (dot + dot) / sum : 0.0f;
                const float x = sum > 0.0f ? (cross + cross) / sum : 0.0f;
                const uint32_t bit = dot > 0.0f ? 1u : 0u;
                if (!bit) {
                    const float pm = psk_power(yb[B + i]), pe = psk_power(yb[B + i - 2 * q]);
                    if (pm > pe)
                        s.acc = psk_late(s.acc, step);
                    else if (pe > pm)
                        s.acc = psk_early(s.acc, step);
                }
                PskChar c;
                if (psk_frame(s.f, bit, mtile + (unsigned long long)i - (unsigned long long)q, fabsf(d), &c)) {
                    /* never refused: char_stride is at least the bound the host tests (pddc_psk_max_chars) */
                    if ((long long)nch < a.char_stride)
                        chars[nch++] = c;
                }
                if (sym && (long long)nsy < a.sym_stride)             /* likewise (pddc_psk_max_syms) */
                    sym[nsy++] = make_float2(d, x);
                s.vr = u.x;
                s.vi = u.y;
                s.pv = pu;
                s.d_last = d;
                s.x_last = x;
                ++s.f.symbols;
            }
        }
        __syncthreads();

        /* the last B of [B before | tile] to the front */
        float2 t0v = make_float2(0.0f, 0.0f), t1v = t0v;
        if (on) {
            t0v = yb[hi + lane];
            t1v = yb[hi + 64 + lane];
        }
        __syncthreads();
        if (on) {
            yb[lane] = t0v;
            yb[64 + lane] = t1v;
        }
        __syncthreads();
    }

    if (!w.have)
        return;
    if (lane == 0) {
        a.new_state[j] = s;
        a.counts[j] = nch;
        if (a.nsym)
            a.nsym[j] = nsy;
    }
    /* the new carried record: the inputs, and the B outputs in front of the row (an OFF receiver's are the old ones) */
    dec_carry(a.new_hist, HS, w, input, on ? a.n : 0);
    for (int e = lane; e < B; e += 64)
        a.new_hist[(long long)j * HS + H + e] = yb[e];
}

hipError_t launch_psk(const PskArgs &a, hipStream_t s)
{
    return dec_launch<&k_psk>(a, !a.sym || (a.sym_stride >= 1 && a.nsym), kPskLdsCap, psk_lds_bytes(a.window), s);
}

static_assert(kPskBack == 128, "the move to the front takes two slots per lane");

} // namespace pddc
