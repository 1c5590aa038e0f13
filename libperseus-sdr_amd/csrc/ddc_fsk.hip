/*
 * ddc_fsk.hip -- the FSK decoder: every receiver's complex series through the mark and the space matched filter of its
 * modem, and the start-stop receiver behind the two powers (gfx950 only).
 *
 *   k_fsk   per ON receiver j and sample m of the launch, with (hm, hs, inc, nbits) of the receiver's modem:
 *           M = (0, 0); over t = 0 .. W-1 ascending, z = z_j[m - t]:
 *               M.re = fmaf(hm[t].re, z.re, M.re); M.re = fmaf(-hm[t].im, z.im, M.re);
 *               M.im = fmaf(hm[t].re, z.im, M.im); M.im = fmaf(hm[t].im, z.re, M.im);       S the same with hs
 *           pm = fmaf(M.im, M.im, M.re M.re), ps likewise (REVERSE: exchanged); space = ps > pm;
 *           s = pm + ps; d = s > 0 ? (pm - ps) / s : 0; q = |d|; then one step of the start-stop receiver.
 *           DESIGN.md 8 and include/perseus_ddc.h have the definition.
 *
 * Walk: ddc_decoder_dev.h's, tiles from the batch's first sample, but spelled out here and not made of that header's
 * functions: with the 32 scalar coefficients of a pass live this kernel sits at the edge of its registers (80 VGPRs, 106
 * SGPRs, 8 of them spilled to VGPR lanes), and each of those functions that was put in place of the text below -- the
 * prologue, the accessor with staging and carry, the tap loop -- moved the spills (5 .. 17), the VGPRs (79 .. 81) or
 * the time at W = 256 (up to 1 %; profiles/r28/decoder_refactor.txt).  A change to the walk is made there and here.
 * A block owns G = 4 consecutive receivers, one wave each, and goes through the batch in tiles of TT = 256
 * samples; the waves share nothing (each has its own rows in LDS), the two barriers per tile are there for the reader.
 *   1. the wave stages its receiver's inputs from W - 1 before the tile's first sample to its last one: consecutive
 *      lanes, consecutive inputs, 8-byte loads; an input before the batch's first comes from the carried record (zero
 *      where the receiver is fresh or cleared).
 *   2. lane l makes the O = 4 outputs l, l + 64, l + 128, l + 192 of the tile, each with accumulators of its own that
 *      meet the taps in ascending t: the bits are the definition's whatever O is.  Per tap and output one ds_read_b64
 *      (32 lanes read 32 consecutive slots: every bank once) feeds 8 fmaf.  The taps are wave-uniform: the modem index
 *      goes through readfirstlane and a pass of 8 taps, 32 floats, comes through the scalar cache into SGPRs; the last
 *      pass of a window that is no multiple of 8 tests every tap (uniform).
 *   3. d goes to the caller's row (if asked for) and to the wave's row in LDS; the four decisions become four 64-bit
 *      masks (__ballot), the rising edges four more.
 *   4. lane 0 advances the start-stop receiver over the tile from event to event: in IDLE the next rising edge is the
 *      lowest set bit of the edge masks at or behind the position; otherwise the next strobe is (~acc) / inc + 1
 *      samples ahead (the smallest s with acc + s inc >= 2^32), and acc moves by s inc in one step.  Between two
 *      events the definition's per-sample step changes acc (by inc, without a carry) and prev alone, and prev is read
 *      from the masks where it is needed: the walk gives what the per-sample definition gives.
 *   After the last tile lane 0 writes the receiver's registers and counters and the count, and the wave the new carried
 *   inputs, the last W - 1 of [old record | batch], from global memory into the other buffer.
 * OFF receivers: nothing of z is read; the registers and the carried inputs go to the other buffer as they are (or as
 *   the host's marks say), the count is 0, the d row +0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled,
 *   the division is the correctly rounded one); nothing depends on the batch cut, nrx, j's index, the other receivers,
 *   the strides or the tile and lane a sample falls into.  No atomics, no scratch.
 * Bounds: z and d are indexed by receivers < nrx and 0 <= i < n only; the records by receivers < nrx and 0 <= e < W - 1;
 *   a staged slot is < W - 1 + TT, a read one lies in 0 .. W - 2 + TT - 1; the taps are read inside the modem's
 *   4 dec_row(W) floats; the modem index is checked by the host; chars[j][c] has c below char_stride, which the host has
 *   tested against the bound of pddc_fsk_max_chars (DESIGN.md derives it: the kernel's own test is never taken).
 */
#include "ddc_fsk.h"
#include "ddc_decoder_dev.h"

#pragma clang fp contract(off)

namespace pddc {

/* one pass of kDecStep taps from tap t0: hw[4 s ..] = (hm.re, hm.im, hs.re, hs.im) of tap t0 + s; p points at the
 * lane's slot of output 0, tap 0 */
template <bool Guard>
__device__ __forceinline__ void fsk_pass(const float2 *p, int t0, int W, const float (&hw)[4 * kDecStep], float2 (&M)[kDecOut],
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
__device__ __forceinline__ uint32_t fsk_bit(const unsigned long long *w, int i)
{
    return (uint32_t)(w[i >> 6] >> (i & 63)) & 1u;
}

/* the lowest set bit at or behind `pos` of four 64-bit masks, TT if there is none */
__device__ __forceinline__ int fsk_next(const unsigned long long *w, int pos)
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

__global__ __launch_bounds__(kDecThreads) void k_fsk(FskArgs a)
{
    constexpr int G = kDecGroup, O = kDecOut, TT = kDecTile, U = kDecStep;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int W = a.window, H = W - 1;
    const int RS = dec_in_slots(W);
    const int j = (int)blockIdx.x * G + wave;
    const bool have = j < a.nrx;
    float2 *row = lds2 + wave * RS;
    float *drow = reinterpret_cast<float *>(lds2 + G * RS) + wave * TT;
    /* the tile's decisions and rising edges, a bit per sample: sp = mask[0 .. O), edge = mask[O .. 2 O) */
    unsigned long long *sp = reinterpret_cast<unsigned long long *>(lds2 + G * RS + G * TT / 2) + wave * 2 * O;
    unsigned long long *edge = sp + O;

    DecRx r{ 0, 0u };
    if (have)
        r = a.rx[j];
    const uint32_t flags = __builtin_amdgcn_readfirstlane(r.flags);
    const int modem = __builtin_amdgcn_readfirstlane(r.bank);
    const bool on = have && (flags & kDecOn);
    const bool reverse = (flags & kFskReverse) != 0u;
    const bool keep = !(flags & (kDecFresh | kDecClear));            /* the carried inputs are read */
    const float2 *zr = a.z + (long long)(have ? j : 0) * a.z_stride;
    const float2 *old = a.hist + (long long)(have ? j : 0) * H;

    /* input idx of the receiver: before the batch's first from the carried record (H values, the newest last) */
    auto input = [&](long long idx) -> float2 {
        if (idx < 0)
            return (keep && idx >= -(long long)H) ? old[H + idx] : make_float2(0.0f, 0.0f);
        return zr[idx];
    };

    /* the start-stop receiver's registers, as the host's marks leave them (scalars, not the record: no scratch) */
    unsigned long long st_start = 0ull;
    uint32_t st_state = kFskStIdle, st_acc = 0u, st_k = 0u, st_shift = 0u, st_prev = 0u;
    uint32_t st_chars = 0u, st_framing = 0u, st_false = 0u;
    float st_qmin = 0.0f, st_dlast = 0.0f;
    if (have && !(flags & kDecFresh)) {
        const FskState *o = a.state + j;
        st_chars = o->chars;
        st_framing = o->framing;
        st_false = o->false_starts;
        st_dlast = o->d_last;
        st_prev = o->prev;
        if (!(flags & (kDecClear | kFskIdle))) {
            st_start = o->start;
            st_state = o->state;
            st_acc = o->acc;
            st_k = o->k;
            st_shift = o->shift;
            st_qmin = o->qmin;
        }
        if (flags & kDecClear)
            st_prev = 0u;
    }
    uint32_t inc = 1u, nbits = 5u;
    if (on) {
        const FskModem mo = a.bank[modem];
        inc = mo.inc;
        nbits = mo.nbits;
    }
    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps + (long long)modem * (dec_row(W) * 4);
    FskChar *chars = a.chars + (long long)(have ? j : 0) * a.char_stride;
    uint32_t nch = 0u;

    for (long long o0 = 0; o0 < a.n; o0 += TT) {
        const int cnt = (int)(a.n - o0 < TT ? a.n - o0 : TT);
        if (on)
            for (int e = lane; e < H + cnt; e += 64)
                row[e] = input(o0 - H + e);
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
                    fsk_pass<false>(p, t0, W, hw, M, S);
                else
                    fsk_pass<true>(p, t0, W, hw, M, S);
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
                const float s = pm + ps;
                const float d = s > 0.0f ? (pm - ps) / s : 0.0f;
                const int i = 64 * o + lane;
                const bool valid = i < cnt;
                if (valid) {
                    drow[i] = d;
                    if (a.d)
                        a.d[(long long)j * a.d_stride + o0 + i] = d;
                }
                spw[o] = __ballot(valid && ps > pm);
            }
            if (lane == 0) {
                unsigned long long cin = st_prev;
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    sp[o] = spw[o];
                    edge[o] = spw[o] & ~((spw[o] << 1) | cin);
                    cin = spw[o] >> 63;
                }
            }
        } else if (have && a.d) {
            for (int i = lane; i < cnt; i += 64)
                a.d[(long long)j * a.d_stride + o0 + i] = 0.0f;
        }
        __syncthreads();

        if (on && lane == 0) {
            int pos = 0;
            while (pos < cnt) {
                if (st_state == kFskStIdle) {
                    const int e = fsk_next(edge, pos);
                    if (e >= cnt)
                        break;
                    st_state = kFskStStart;
                    st_acc = 0x80000000u;
                    st_start = a.m0 + (unsigned long long)(o0 + e);
                    pos = e + 1;
                    continue;
                }
                /* the strobe is s samples ahead, this one counted: the smallest s with acc + s inc >= 2^32 */
                const unsigned long long s = (unsigned long long)(~st_acc / inc) + 1ull;
                if (s > (unsigned long long)(cnt - pos)) {
                    st_acc += (uint32_t)(cnt - pos) * inc;
                    break;
                }
                const int i = pos + (int)s - 1;
                st_acc += (uint32_t)s * inc;
                pos = i + 1;
                const uint32_t space = fsk_bit(sp, i);
                const float q = fabsf(drow[i]);
                if (st_state == kFskStStart) {
                    if (space) {
                        st_state = kFskStData;
                        st_k = 0u;
                        st_shift = 0u;
                        st_qmin = q;
                    } else {
                        st_state = kFskStIdle;
                        ++st_false;
                    }
                } else if (st_state == kFskStData) {
                    st_shift |= (space ^ 1u) << st_k;
                    st_qmin = fminf(st_qmin, q);
                    if (++st_k == nbits)
                        st_state = kFskStStop;
                } else {
                    st_qmin = fminf(st_qmin, q);
                    /* never refused: char_stride is at least the bound the host tests (pddc_fsk_max_chars) */
                    if ((long long)nch < a.char_stride) {
                        FskChar *c = chars + nch;
                        c->start = st_start;
                        c->code = (uint16_t)st_shift;
                        c->flags = (uint16_t)space;
                        c->quality = st_qmin;
                        ++nch;
                    }
                    ++st_chars;
                    st_framing += space;
                    st_state = kFskStIdle;
                }
            }
            st_prev = fsk_bit(sp, cnt - 1);
            st_dlast = drow[cnt - 1];
        }
    }

    if (!have)
        return;
    if (lane == 0) {
        FskState *o = a.new_state + j;
        o->start = st_start;
        o->state = st_state;
        o->acc = st_acc;
        o->k = st_k;
        o->shift = st_shift;
        o->qmin = st_qmin;
        o->prev = st_prev;
        o->chars = st_chars;
        o->framing = st_framing;
        o->false_starts = st_false;
        o->d_last = st_dlast;
        a.counts[j] = nch;
    }
    /* the new carried record: the last W - 1 of [old record | batch]; an OFF receiver's batch is empty */
    const long long used = on ? a.n : 0;
    for (int e = lane; e < H; e += 64)
        a.new_hist[(long long)j * H + e] = input(used - H + e);
}

hipError_t launch_fsk(const FskArgs &a, hipStream_t s)
{
    return dec_launch<&k_fsk>(a, !a.d || a.d_stride >= a.n, kFskLdsCap, fsk_lds_bytes(a.window), s);
}

} // namespace pddc
