/*
 * ddc_sitor.hip -- the SITOR decoder: every receiver's complex series through the mark and the space matched filter of
 * its modem, and the synchronous receiver of the 7-bit constant-ratio code behind the two powers (gfx950 only).
 *
 *   k_sitor per ON receiver j and sample m of the launch, with (hm, hs, inc, step, lock, unlock) of the receiver's modem:
 *           the discriminator of k_fsk, operation by operation (M, S by four spelled fmaf per tap, t ascending; pm, ps,
 *           REVERSE; space = ps > pm; s = pm + ps; d = s > 0 ? (pm - ps) / s : 0; q = |d|), then one step of the bit
 *           clock and, on a strobe, of the framing (ddc_sitor_bits.h: rules a - c), then the clock's correction where the
 *           decision differs from the previous sample's.  DESIGN.md 8 and include/perseus_ddc.h have the definition.
 *
 * Walk: ddc_decoder_dev.h's -- prologue, input accessor, staging, carry and launch are that header's functions.  The
 * complex two-filter pass is this file's own copy of k_fsk's (sitor_pass): k_fsk spells its walk out because every
 * function put in its place moved its registers and spills (ddc_fsk.hip says so), and a pass shared through a header
 * would have to leave k_fsk's listing line for line what it is; a copy cannot touch it.  A change to the pass is made
 * there and here.
 * A block owns G = 4 consecutive receivers, one wave each, and goes through the batch in tiles of TT = 256 samples; the
 * waves share nothing (each has its own rows in LDS), the barriers are there for the reader.
 *   1. the wave stages its receiver's inputs (dec_stage).
 *   2. lane l makes the O = 4 outputs l, l + 64, l + 128, l + 192 of the tile, each with accumulators of its own that
 *      meet the taps in ascending t; per tap and output one ds_read_b64 feeds 8 fmaf; a pass of 8 taps, 32 floats,
 *      comes through the scalar cache into SGPRs; the last pass of a window that is no multiple of 8 tests every tap.
 *   3. d goes to the wave's row in LDS; the four decisions become four 64-bit masks (__ballot), the transitions four
 *      more: sp ^ ((sp << 1) | carry-in), both ways, the carry-in being the previous tile's (or batch's) last decision.
 *   4. lane 0 advances the clock over the tile from event to event: the next event is the nearer of the next set
 *      transition bit at or behind the position and the next strobe, sitor_jump(acc, inc) samples ahead.  Between two
 *      events the definition's per-sample step changes acc alone (by inc, without a carry): the walk gives what the
 *      per-sample definition gives.  A strobe and a transition on one sample are taken in the definition's order:
 *      strobe, framing, then the correction.  A transition bit at or behind the tile's last sample is no event (the
 *      mask's bits behind the batch's end are zero, and what follows a set last decision is not known yet).
 *   After the last tile lane 0 writes the receiver's record and the counts, and the wave the new carried inputs.
 * OFF receivers: nothing of z is read; the record and the carried inputs go to the other buffer as they are (or as the
 *   host's marks say), count and nsoft are 0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled,
 *   the division is the correctly rounded one); nothing depends on the batch cut, nrx, j's index, the other receivers,
 *   the strides or the tile and lane a sample falls into.  No atomics, no scratch.
 * Bounds: ddc_decoder_dev.h's for z, the records and the staged row; the taps are read inside the modem's 4 dec_row(W)
 *   floats; the modem index is checked by the host; chars[j][c] has c below char_stride and soft[j][c] has c below
 *   soft_stride, which the host has tested against the bounds of pddc_sitor_max_chars and pddc_sitor_max_syms
 *   (DESIGN.md derives them: the kernel's own tests are never taken).
 */
#include "ddc_sitor.h"
#include "ddc_decoder_dev.h"

#pragma clang fp contract(off)

namespace pddc {

/* one pass of kDecStep taps from tap t0: hw[4 s ..] = (hm.re, hm.im, hs.re, hs.im) of tap t0 + s; p points at the
 * lane's slot of output 0, tap 0.  k_fsk's fsk_pass, copied (see above) */
template <bool Guard>
__device__ __forceinline__ void sitor_pass(const float2 *p, int t0, int W, const float (&hw)[4 * kDecStep], float2 (&M)[kDecOut],
                                           float2 (&S)[kDecOut])
{
#pragma unroll
    for (int s = 0; s < kDecStep; ++s) {
        if (Guard && t0 + s >= W)
            break;
        const float mr = hw[4 * s], mi = hw[4 * s + 1], sr = hw[4 * s + 2], si = hw[4 * s + 3];
#pragma unroll
        for (int o = 0; o < kDecOut; ++o) {
            const float2 z = p[64 * o - (t0 + s)];
            M[o].x = fmaf(mr, z.x, M[o].x);
            M[o].x = fmaf(-mi, z.y, M[o].x);
            M[o].y = fmaf(mr, z.y, M[o].y);
            M[o].y = fmaf(mi, z.x, M[o].y);
            S[o].x = fmaf(sr, z.x, S[o].x);
            S[o].x = fmaf(-si, z.y, S[o].x);
            S[o].y = fmaf(sr, z.y, S[o].y);
            S[o].y = fmaf(si, z.x, S[o].y);
        }
    }
}

/* bit i (0 .. TT - 1) of four 64-bit masks */
__device__ __forceinline__ uint32_t sitor_bit(const unsigned long long *w, int i)
{
    return (uint32_t)(w[i >> 6] >> (i & 63)) & 1u;
}

/* the lowest set bit at or behind `pos` (< TT) of four 64-bit masks, TT if there is none */
__device__ __forceinline__ int sitor_next(const unsigned long long *w, int pos)
{
    unsigned long long keep = ~0ull << (pos & 63);
    for (int o = pos >> 6; o < kDecOut; ++o) {
        const unsigned long long v = w[o] & keep;
        if (v)
            return 64 * o + __ffsll(v) - 1;
        keep = ~0ull;
    }
    return kDecTile;
}

__global__ __launch_bounds__(kDecThreads) void k_sitor(SitorArgs a)
{
    constexpr int G = kDecGroup, O = kDecOut, TT = kDecTile, U = kDecStep;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int W = a.window, H = W - 1;
    const int RS = dec_in_slots(W);
    const DecWave w = dec_wave(a.rx, a.nrx);
    const int lane = w.lane, j = w.j;
    float2 *row = lds2 + w.wave * RS;
    float *drow = reinterpret_cast<float *>(lds2 + G * RS) + w.wave * TT;
    /* the tile's decisions and transitions, a bit per sample: sp = mask[0 .. O), trans = mask[O .. 2 O) */
    unsigned long long *sp = reinterpret_cast<unsigned long long *>(lds2 + G * RS + G * TT / 2) + w.wave * 2 * O;
    unsigned long long *trans = sp + O;

    const bool on = w.have && (w.flags & kDecOn);
    const bool reverse = (w.flags & kSitorReverse) != 0u;
    const DecInput input = dec_input(w, a.z, a.z_stride, a.hist, H, H);

    const SitorModem mo = a.bank[w.bank];
    const uint32_t inc = mo.inc, step = mo.step;
    /* the receiver's record, as the host's marks leave it */
    SitorState s{};
    if (w.have && !(w.flags & kDecFresh))
        s = a.state[j];
    if (w.flags & (kDecClear | kSitorReframe))
        sitor_frame_restart(s.f);
    if (w.flags & kDecClear)
        s.acc = s.prev = 0u;

    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps + (long long)w.bank * (dec_row(W) * 4);
    SitorChar *chars = a.chars + (long long)w.jr * a.char_stride;
    float *soft = a.soft ? a.soft + (long long)w.jr * a.soft_stride : nullptr;
    uint32_t nch = 0u, nso = 0u;

    for (long long o0 = 0; o0 < a.n; o0 += TT) {
        const int cnt = (int)(a.n - o0 < TT ? a.n - o0 : TT);
        if (on)
            dec_stage(row, input, lane, o0, 0, cnt);
        __syncthreads();

        if (on) {
            unsigned long long spw[O];
            float2 M[O], S[O];
#pragma unroll
            for (int o = 0; o < O; ++o)
                M[o] = S[o] = make_float2(0.0f, 0.0f);
            const float2 *p = row + H + lane;
            for (int t0 = 0; t0 < W; t0 += U) {
                float hw[4 * U];
#pragma unroll
                for (int i = 0; i < 4 * U; ++i)
                    hw[i] = h[4 * t0 + i];
                if (t0 + U <= W)
                    sitor_pass<false>(p, t0, W, hw, M, S);
                else
                    sitor_pass<true>(p, t0, W, hw, M, S);
            }
#pragma unroll
            for (int o = 0; o < O; ++o) {
                float pm = fmaf(M[o].y, M[o].y, M[o].x * M[o].x);
                float ps = fmaf(S[o].y, S[o].y, S[o].x * S[o].x);
                if (reverse) {
                    const float x = pm;
                    pm = ps;
                    ps = x;
                }
                const float sum = pm + ps;
                const float d = sum > 0.0f ? (pm - ps) / sum : 0.0f;
                const int i = 64 * o + lane;
                const bool valid = i < cnt;
                if (valid)
                    drow[i] = d;
                spw[o] = __ballot(valid && ps > pm);
            }
            if (lane == 0) {
                unsigned long long cin = s.prev;
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    sp[o] = spw[o];
                    trans[o] = spw[o] ^ ((spw[o] << 1) | cin);
                    cin = spw[o] >> 63;
                }
            }
        }
        __syncthreads();

        if (on && lane == 0) {
            const unsigned long long mtile = a.m0 + (unsigned long long)o0;
            int pos = 0;
            while (pos < cnt) {
                const uint32_t left = (uint32_t)(cnt - pos);
                int t = sitor_next(trans, pos);
                if (t >= cnt)
                    t = TT + 1;                                        /* no transition among the tile's samples */
                const uint64_t jump = sitor_jump(s.acc, inc);
                const uint32_t ahead = (uint32_t)(t - pos) + 1u;       /* samples to the transition, that one counted */
                if (jump > left && ahead > left) {
                    s.acc = sitor_advance(s.acc, inc, left);
                    break;
                }
                if ((uint64_t)ahead < jump) {                          /* the transition comes first: no carry on the way */
                    s.acc = sitor_correct(sitor_advance(s.acc, inc, ahead), step);
                    pos = t + 1;
                    continue;
                }
                const uint32_t k = (uint32_t)jump;                     /* <= left <= TT */
                const int i = pos + (int)k - 1;                        /* the strobe's sample */
                s.acc = sitor_advance(s.acc, inc, k);
                pos = i + 1;
                const float d = drow[i];
                SitorChar c;
                if (sitor_strobe(s.f, mo, sitor_bit(sp, i), mtile + (unsigned long long)i, fabsf(d), &c)) {
                    /* never refused: char_stride is at least the bound the host tests (pddc_sitor_max_chars) */
                    if ((long long)nch < a.char_stride)
                        chars[nch++] = c;
                }
                if (soft && (long long)nso < a.soft_stride)            /* likewise (pddc_sitor_max_syms) */
                    soft[nso++] = d;
                if (t == i)
                    s.acc = sitor_correct(s.acc, step);
            }
            s.prev = sitor_bit(sp, cnt - 1);
            s.d_last = drow[cnt - 1];
        }
    }

    if (!w.have)
        return;
    if (lane == 0) {
        a.new_state[j] = s;
        a.counts[j] = nch;
        if (a.nsoft)
            a.nsoft[j] = nso;
    }
    /* the new carried record: the last W - 1 of [old record | batch]; an OFF receiver's batch is empty */
    dec_carry(a.new_hist, H, w, input, on ? a.n : 0);
}

hipError_t launch_sitor(const SitorArgs &a, hipStream_t s)
{
    return dec_launch<&k_sitor>(a, !a.soft || (a.soft_stride >= 1 && a.nsoft), kSitorLdsCap, sitor_lds_bytes(a.window), s);
}

} // namespace pddc
