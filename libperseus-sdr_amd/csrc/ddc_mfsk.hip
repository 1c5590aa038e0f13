/*
 * ddc_mfsk.hip -- the MFSK decoder: every receiver's complex series through the M matched filters of its modem, the best
 * and the second best tone of every sample, and a symbol clock that looks a quarter symbol to either side of the decision
 * (gfx950 only).
 *
 *   k_mfsk    per ON receiver j and sample m, with (M, h_0 .. h_M-1, inc, q, step) of the receiver's modem:
 *             for k = 0 .. M-1: Y = (0, 0); over t = 0 .. W-1 ascending, z = z_j[m - t]:
 *                 Y.re = fmaf(h_k[t].re, z.re, Y.re); Y.re = fmaf(-h_k[t].im, z.im, Y.re);
 *                 Y.im = fmaf(h_k[t].re, z.im, Y.im); Y.im = fmaf(h_k[t].im, z.re, Y.im);      (fsk's sequence)
 *             p_k = fmaf(Y.im, Y.im, Y.re Y.re); the best (a, b) and the runner-up (s, r) over k ascending; one step of
 *             the clock, and on a strobe the record from (a, s, b, r) at m - q and the early / late correction from
 *             b[m] and b[m - 2 q].  DESIGN.md 4 and include/perseus_ddc.h have the definition.
 *
 * Walk: ddc_decoder_dev.h's (prologue, input, stage, carry, launch), tiles from the batch's first sample.  The waves share
 * nothing (each has its own row in LDS: the input row, then (b, r) of the B = 128 samples before the tile and of the
 * tile's, then their tone indices), the barriers are there for the reader and for the order of a wave's own LDS traffic.
 * Per tile:
 *   1. the wave stages its receiver's inputs (dec_stage).
 *   2. a loop over ceil(M / 2) tone pairs; inside it k_fsk's complex pair pass (a copy, as k_sitor's is: with the 32
 *      scalar coefficients of a pass live the tap loop sits at the edge of its registers, ddc_fsk.hip), the two tones of
 *      the pair in the places of mark and space.  Lane l makes the O = 4 samples l, l + 64, l + 128, l + 192 and keeps
 *      (a, s, b, r) of each in registers across the loop.  A pass of 8 taps of the pair, 32 floats, comes through the
 *      scalar cache: the modem index went through readfirstlane and the pair counter is uniform.  The input row is read
 *      from LDS once per pair: 32 lanes, 32 consecutive 8-byte slots, every bank once.  For odd M the host has padded a
 *      zero tone; the last pair's second half is skipped (uniform) and never enters the maximum.
 *   3. (b, r) and the indices go to the row's second and third part, behind those of the B samples before the tile, b
 *      to the caller's row if asked for.
 *   4. lane 0 walks the tile's wraps from one to the next: the clock jumps (~acc) / inc + 1 samples at once; a wrap is
 *      a strobe unless a late correction borrowed from it (skip); a strobe reads m - q, m and m - 2 q from LDS.  The
 *      records go to global memory as they come.
 *   5. the wave moves the last B of [the B before | the tile] to the front for the next tile.
 *   After the last tile lane 0 writes the receiver's record and the count, and the wave, behind the walk's carried
 *   inputs, the B per-sample results in front of the row into the other buffer.  They are functions of the inputs alone,
 *   so a carried one has the bits a longer batch would have made.
 * OFF receivers: nothing of z is read; the record goes to the other buffer as it is (or as the host's marks say), the
 *   count is 0, the b row +0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled,
 *   the division is the correctly rounded one); nothing depends on the batch cut, nrx, j's index, the other receivers,
 *   the strides or the lane a sample falls into.  No atomics, no scratch.
 * Bounds: the walk's are in ddc_decoder_dev.h (staging ends at the tile's last sample, hi <= TT; the filter reads slots
 *   0 .. W - 2 + TT of the wave's own input row; the taps are read inside the modem's 16 pairs of 4 dec_row(W) floats, pair
 *   p < ceil(M / 2) <= 16; the modem index and M are checked by the host).  Here: a receiver's carried record has
 *   mfsk_hist_slots(W) = W - 1 + B + B / 4 slots and is read and written at W - 1 + e, 0 <= e < B, and at 16-bit cell e of
 *   the B / 4 slots behind, of receivers < nrx; a result slot is B + i with 0 <= i < hi <= TT, a strobe reads B + i,
 *   B + i - q and B + i - 2 q >= 0 since 2 q <= B (the host tests q); the move reads hi + e < TT + B; best[j][o0 + i] has
 *   o0 + i < n <= best_stride; chars[j][c] has c below char_stride, which the host has tested against the bound of
 *   pddc_mfsk_max_syms (DESIGN.md derives it: the kernel's own test is never taken).
 */
#include "ddc_mfsk.h"
#include "ddc_decoder_dev.h"

#pragma clang fp contract(off)

namespace pddc {

/* one pass of kDecStep taps from tap t0: hw[4 s ..] = (h_2p.re, h_2p.im, h_2p+1.re, h_2p+1.im) of tap t0 + s; p points at
 * the lane's slot of output 0, tap 0 (k_fsk's fsk_pass) */
template <bool Guard>
__device__ __forceinline__ void mfsk_pass(const float2 *p, int t0, int W, const float (&hw)[4 * kDecStep], float2 (&E)[kDecOut],
                                          float2 (&D)[kDecOut])
{
#pragma unroll
    for (int s = 0; s < kDecStep; ++s) {
        if (Guard && t0 + s >= W)
            break;
        const float er = hw[4 * s], ei = hw[4 * s + 1], dr = hw[4 * s + 2], di = hw[4 * s + 3];
#pragma unroll
        for (int o = 0; o < kDecOut; ++o) {
            const float2 z = p[64 * o - (t0 + s)];
            E[o].x = fmaf(er, z.x, E[o].x);
            E[o].x = fmaf(-ei, z.y, E[o].x);
            E[o].y = fmaf(er, z.y, E[o].y);
            E[o].y = fmaf(ei, z.x, E[o].y);
            D[o].x = fmaf(dr, z.x, D[o].x);
            D[o].x = fmaf(-di, z.y, D[o].x);
            D[o].y = fmaf(dr, z.y, D[o].y);
            D[o].y = fmaf(di, z.x, D[o].y);
        }
    }
}

__device__ __forceinline__ float mfsk_power(float2 y) { return fmaf(y.y, y.y, y.x * y.x); }

/* tone k with power pk against the best (b, low byte of idx) and the runner-up (r, second byte): a NaN is never greater */
__device__ __forceinline__ void mfsk_pick(float pk, uint32_t k, float &b, float &r, uint32_t &idx)
{
    if (pk > b) {
        r = b;
        idx = (idx & 0xFFu) << 8 | k;
        b = pk;
    } else if (pk > r) {
        r = pk;
        idx = (idx & 0xFFu) | k << 8;
    }
}

__global__ __launch_bounds__(kDecThreads) void k_mfsk(MfskArgs a)
{
    constexpr int O = kDecOut, TT = kDecTile, B = (int)kMfskBack, U = kDecStep;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int W = a.window, H = W - 1;
    const DecWave w = dec_wave(a.rx, a.nrx);
    const int lane = w.lane, j = w.j;
    const int HS = mfsk_hist_slots(W);
    float2 *row = lds2 + w.wave * mfsk_row_slots(W);
    float2 *br = row + dec_in_slots(W);                               /* (b, r): B samples before the tile, then the tile's */
    uint16_t *tn = reinterpret_cast<uint16_t *>(br + kMfskSamples);   /* their indices: best | runner-up << 8            */

    const bool on = w.have && (w.flags & kDecOn);
    const bool reverse = (w.flags & kMfskReverse) != 0u;
    const DecInput input = dec_input(w, a.z, a.z_stride, a.hist, HS, H);
    const bool keep = input.keep;

    const MfskModem mp = a.bank[w.bank];
    const uint32_t inc = mp.inc, step = mp.step, M = mp.ntones, npair = mfsk_pairs(M);
    const int q = (int)mp.q;
    /* the receiver's record, as the host's marks leave it: a restart keeps the counter */
    MfskState s{};
    if (w.have && !(w.flags & kDecFresh))
        s = a.state[j];
    if (w.flags & kMfskMarks) {
        s.acc = s.skip = 0u;
        s.tone_last = 0u;
        s.q_last = 0.0f;
    }

    const int R = dec_row(W);
    const float PDDC_CONSTANT *hm = (const float PDDC_CONSTANT *)a.taps + (long long)w.bank * mfsk_modem_floats(R);
    MfskSym *syms = a.chars + (long long)w.jr * a.char_stride;
    uint32_t nsy = 0u;

    /* the B samples before the batch's first */
    const uint16_t *oldt = reinterpret_cast<const uint16_t *>(input.old + H + B);
    for (int e = lane; e < B; e += 64) {
        const bool rd = w.have && keep;
        br[e] = rd ? input.old[H + e] : make_float2(0.0f, 0.0f);
        tn[e] = rd ? oldt[e] : (uint16_t)0;
    }

    for (long long o0 = 0; o0 < a.n; o0 += TT) {
        const int hi = (int)(a.n - o0 < TT ? a.n - o0 : TT);          /* the tile's samples 0 .. hi - 1 */
        if (on)
            dec_stage(row, input, lane, o0, 0, hi);
        __syncthreads();

        if (on) {
            float b[O], r[O];
            uint32_t idx[O];
#pragma unroll
            for (int o = 0; o < O; ++o) {
                b[o] = r[o] = 0.0f;
                idx[o] = 0u;
            }
            const float2 *p = row + H + lane;
            for (uint32_t pr = 0; pr < npair; ++pr) {
                const float PDDC_CONSTANT *h = hm + (long long)pr * mfsk_pair_floats(R);
                float2 E[O], D[O];
#pragma unroll
                for (int o = 0; o < O; ++o)
                    E[o] = D[o] = make_float2(0.0f, 0.0f);
                for (int t0 = 0; t0 < W; t0 += U) {
                    float hw[4 * U];
#pragma unroll
                    for (int i = 0; i < 4 * U; ++i)
                        hw[i] = h[4 * t0 + i];
                    if (t0 + U <= W)
                        mfsk_pass<false>(p, t0, W, hw, E, D);
                    else
                        mfsk_pass<true>(p, t0, W, hw, E, D);
                }
                const bool both = 2u * pr + 1u < M;                   /* uniform: the padded tone of an odd M is skipped */
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    mfsk_pick(mfsk_power(E[o]), 2u * pr, b[o], r[o], idx[o]);
                    if (both)
                        mfsk_pick(mfsk_power(D[o]), 2u * pr + 1u, b[o], r[o], idx[o]);
                }
            }
#pragma unroll
            for (int o = 0; o < O; ++o) {
                const int i = 64 * o + lane;
                if (i < hi) {
                    br[B + i] = make_float2(b[o], r[o]);
                    tn[B + i] = (uint16_t)idx[o];
                    if (a.best)
                        a.best[(long long)j * a.best_stride + o0 + i] = b[o];
                }
            }
        } else if (w.have && a.best) {
            for (int i = lane; i < hi; i += 64)
                a.best[(long long)j * a.best_stride + o0 + i] = 0.0f;
        }
        __syncthreads();

        if (on && lane == 0) {
            const unsigned long long mtile = a.m0 + (unsigned long long)o0;
            uint32_t pos = 0u;
            for (;;) {
                const uint32_t left = (uint32_t)hi - pos;
                const uint64_t jump = mfsk_jump(s.acc, inc);
                if (jump > left) {
                    s.acc = mfsk_advance(s.acc, inc, left);
                    break;
                }
                const uint32_t k = (uint32_t)jump;                    /* <= left <= TT */
                s.acc = mfsk_advance(s.acc, inc, k);
                const int i = (int)(pos + k - 1u);                    /* the wrap's sample: a strobe's late one */
                pos += k;
                if (s.skip) {                                         /* the wrap a late correction borrowed from */
                    s.skip = 0u;
                    continue;
                }
                const float2 u = br[B + i - q];
                const uint32_t ix = tn[B + i - q];
                uint32_t tone = ix & 0xFFu, second = ix >> 8;
                if (reverse) {
                    tone = M - 1u - tone;
                    second = M - 1u - second;
                }
                const float sum = u.x + u.y;
                const float qual = sum > 0.0f ? (u.x - u.y) / sum : 0.0f;
                const float bl = br[B + i].x, be = br[B + i - 2 * q].x;
                if (bl > be)
                    s.acc = mfsk_late(s.acc, s.skip, step);
                else if (be > bl)
                    s.acc = mfsk_early(s.acc, step);
                /* never refused: char_stride is at least the bound the host tests (pddc_mfsk_max_syms) */
                if ((long long)nsy < a.char_stride) {
                    MfskSym c;
                    c.start = mtile + (unsigned long long)i - (unsigned long long)q;
                    c.tone = (uint8_t)tone;
                    c.second = (uint8_t)second;
                    c.flags = 0;
                    c.quality = qual;
                    syms[nsy++] = c;
                }
                s.tone_last = tone;
                s.q_last = qual;
                ++s.symbols;
            }
        }
        __syncthreads();

        /* the last B of [B before | tile] to the front */
        float2 v0 = make_float2(0.0f, 0.0f), v1 = v0;
        uint16_t t0v = 0, t1v = 0;
        if (on) {
            v0 = br[hi + lane];
            v1 = br[hi + 64 + lane];
            t0v = tn[hi + lane];
            t1v = tn[hi + 64 + lane];
        }
        __syncthreads();
        if (on) {
            br[lane] = v0;
            br[64 + lane] = v1;
            tn[lane] = t0v;
            tn[64 + lane] = t1v;
        }
        __syncthreads();
    }

    if (!w.have)
        return;
    if (lane == 0) {
        a.new_state[j] = s;
        a.counts[j] = nsy;
    }
    /* the new carried record: the inputs, and the B results in front of the row (an OFF receiver's are the old ones) */
    dec_carry(a.new_hist, HS, w, input, on ? a.n : 0);
    uint16_t *newt = reinterpret_cast<uint16_t *>(a.new_hist + (long long)j * HS + H + B);
    for (int e = lane; e < B; e += 64) {
        a.new_hist[(long long)j * HS + H + e] = br[e];
        newt[e] = tn[e];
    }
}

hipError_t launch_mfsk(const MfskArgs &a, hipStream_t s)
{
    return dec_launch<&k_mfsk>(a, !a.best || a.best_stride >= a.n, kMfskLdsCap, mfsk_lds_bytes(a.window), s);
}

static_assert(kMfskBack == 128, "the move to the front takes two slots per lane");
static_assert(sizeof(MfskSym) == 16, "the skeleton's records are 16 bytes");

} // namespace pddc
