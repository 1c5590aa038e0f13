/*
 * ddc_fax.hip -- the radiofax decoder: every receiver's complex series through the real low-pass of its modem, an FM
 * discriminator behind it, a free-running pixel clock, the grey map and the line structure (gfx950 only).
 *
 *   k_fax     per ON receiver j and sample m, with (h, inc, width, box, scale, bias, the tone ranges, need) of the
 *             receiver's modem: y by dec_filter; w = y[m] conj(y[m - 1]) as k_demod's FM spells it; f = 0 where w is
 *             zero, atan2f(w.im, w.re) / pi + q elsewhere, q = (w.re - w.re) + (w.im - w.im) (0, or NaN where w is not
 *             finite), negated under REVERSE; one step of the clock and, on a strobe, the pixel from the last `box`
 *             values of f and one step of the line structure (ddc_fax_bits.h).  DESIGN.md 4 and include/perseus_ddc.h
 *             have the definition.
 *
 * Walk: ddc_decoder_dev.h's (prologue, input accessor, staging, filter, carry, launch), tiles of TT = 256 samples from
 * the batch's first.  The waves share nothing (each has its own rows in LDS), the barriers are there for the reader
 * and for the order of a wave's own LDS traffic.  Behind the filter nothing walks the samples: per tile
 *   3. y[m - 1] is the lane below's register (a ds_bpermute rotation; lane 0 takes lane 63's previous output, or the
 *      carried y); f goes to the wave's row in LDS behind kFaxBack = 16 values before the tile, and to disc.
 *   4. the clock is a closed form: with a = acc at the tile's first sample, sample i strobes iff the carries of
 *      a + (i + 1) inc and a + i inc differ (64-bit, i <= 256), and the carries of a + i inc ARE the pixel's slot in the
 *      tile: the prefix count the ballots would give, without them.  A strobing lane sums its `box` values of f from
 *      LDS in the definition's order and puts the pixel's byte at slot + mis, mis the low two bits of the byte's address
 *      in memory, and its sample index beside it.
 *   5. lanes 0 .. 33 store the tile's pixels, a whole aligned word each where all four bytes are the tile's, single
 *      bytes at the two ends only (at most 3 + 3 a tile).
 *   6. lane k takes pixels k and k + 64: three ballots per half (>= 192, < 64, >= 128).  The hysteresis level in front
 *      of a pixel is that of the nearest pixel below it that is not in between, found with a count-leading-zeros on
 *      the two masks; a fourth ballot holds the crossings.
 *   7. the line structure goes from line end to line end, not from pixel to pixel: a line's crossings and white are
 *      population counts of mask ranges, its start the sample index beside its first pixel; fax_line_end (class, run,
 *      active, the record) runs once per line end, at most TT / 2 / 16 = 8 times a tile and once in 19 tiles at
 *      120 lines a minute, IOC 576 and 2.7 samples a pixel.
 *   8. the wave moves the last 16 values of f to the front.
 *   After the last tile lane 0 writes the receiver's record and the counts, 16 lanes the carried f, the wave the inputs.
 * OFF receivers: nothing of z is read; the record and the carried values go to the other buffer as they are (or as the
 *   host's marks say), counts and npix are 0.
 * Bits: one lane makes each value with one operation sequence (contraction is off in this file, every fmaf is spelled,
 *   the division is the correctly rounded one); y[m - 1] and f have the bits a longer batch would have made, since both
 *   are functions of the inputs alone; nothing depends on the batch cut, nrx, j's index, the other receivers, the
 *   strides or the tile and lane a sample falls into.  No atomics, no scratch.
 * Bounds: ddc_decoder_dev.h's for z, the records and the staged row; the taps are read inside the modem's dec_row(W)
 *   floats; the modem index is checked by the host.  f slots: written at 16 + i, i < hi <= TT, read at 16 + i - b with
 *   b < box <= 16, and hi + lane < 16 + hi for the move.  A tile has at most (2^32 - 1 + 256 2^31) >> 32 = 128 pixels:
 *   slots 0 .. 127 of the sample bytes, bytes mis .. mis + 127 <= 130 of the kFaxPixBytes = 136 pixel bytes.  pix[j][c]
 *   has c below pix_stride and lines[j][c] has c below char_stride, which the host has tested against the bounds of
 *   pddc_fax_max_pixels and pddc_fax_max_lines; a tile that would pass them is not stored (never taken).  disc[j][i]
 *   has i < n <= disc_stride.
 */
#include "ddc_fax.h"
#include "ddc_decoder_dev.h"

#pragma clang fp contract(off)

namespace pddc {

static constexpr float kFaxInvPi = 0.318309886183790672f;

/* the low n (0 .. 64) bits of x */
__device__ __forceinline__ unsigned long long fax_below(unsigned long long x, uint32_t n)
{
    return n >= 64u ? x : x & ((1ull << n) - 1ull);
}

/* set bits among bits a .. b - 1 (a <= b <= 128) of a 128-bit mask */
__device__ __forceinline__ uint32_t fax_count(const unsigned long long (&m)[2], uint32_t a, uint32_t b)
{
    const uint32_t ca = (uint32_t)__popcll(fax_below(m[0], a < 64u ? a : 64u)) + (uint32_t)__popcll(fax_below(m[1], a > 64u ? a - 64u : 0u));
    const uint32_t cb = (uint32_t)__popcll(fax_below(m[0], b < 64u ? b : 64u)) + (uint32_t)__popcll(fax_below(m[1], b > 64u ? b - 64u : 0u));
    return cb - ca;
}

/* the level the nearest set bit of (hi | lo) gives, `level` if neither mask has one */
__device__ __forceinline__ uint32_t fax_level(unsigned long long hi, unsigned long long lo, uint32_t level)
{
    const unsigned long long any = hi | lo;
    return any ? (uint32_t)(hi >> (63 - __clzll((long long)any))) & 1u : level;
}

__global__ __launch_bounds__(kDecThreads) void k_fax(FaxArgs a)
{
    constexpr int G = kDecGroup, O = kDecOut, TT = kDecTile, BK = kFaxBack;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int W = a.window, H = W - 1;
    const int RS = dec_in_slots(W);
    const DecWave w = dec_wave(a.rx, a.nrx);
    const int lane = w.lane, j = w.j;
    float2 *row = lds2 + w.wave * RS;
    unsigned char *own = reinterpret_cast<unsigned char *>(lds2 + G * RS) + w.wave * (int)kFaxRowBytes;
    float *frow = reinterpret_cast<float *>(own);                      /* 16 values of f before the tile, then the tile's */
    unsigned char *pb = own + (BK + TT) * 4;                           /* the tile's pixels, from byte mis on */
    unsigned char *sidx = pb + kFaxPixBytes;                           /* the sample of the tile each was strobed at */

    const bool on = w.have && (w.flags & kDecOn);
    const bool reverse = (w.flags & kFaxReverse) != 0u;
    const DecInput input = dec_input(w, a.z, a.z_stride, a.hist, H, H);

    const FaxModem mo = a.bank[w.bank];
    const uint32_t inc = mo.inc, width = mo.width;
    const int B = (int)mo.box;
    const float rb = 1.0f / (float)B;
    /* the receiver's record, as the host's marks leave it */
    const bool old = w.have && !(w.flags & kDecFresh);
    FaxLine l{};
    uint32_t acc = 0u;
    float2 yp = make_float2(0.0f, 0.0f);
    if (old) {
        l = a.state[j].l;
        acc = a.state[j].acc;
        yp = a.state[j].y;
    }
    if (w.flags & (kDecClear | kFaxReline))
        fax_line_restart(l, (w.flags & kDecClear) != 0u);
    if (w.flags & kDecClear) {
        acc = 0u;
        yp = make_float2(0.0f, 0.0f);
    }
    if (lane < BK)
        frow[lane] = (old && !(w.flags & kDecClear)) ? a.state[j].f[lane] : 0.0f;

    const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.taps + (long long)w.bank * dec_row(W);
    FaxLineRec *lines = a.chars + (long long)w.jr * a.char_stride;
    unsigned char *pix = a.pix + (long long)w.jr * a.pix_stride;
    float *disc = a.disc ? a.disc + (long long)w.jr * a.disc_stride : nullptr;
    uint32_t nln = 0u, np = 0u;

    for (long long o0 = 0; o0 < a.n; o0 += TT) {
        const int hi = (int)(a.n - o0 < TT ? a.n - o0 : TT);          /* the tile's samples 0 .. hi - 1 */
        if (on)
            dec_stage(row, input, lane, o0, 0, hi);
        __syncthreads();

        if (on) {
            float2 y[O], rot[O], last = make_float2(0.0f, 0.0f);
            dec_filter(row, lane, H, W, h, y);
            const int below = (lane + 63) & 63;
#pragma unroll
            for (int o = 0; o < O; ++o) {
                rot[o].x = __shfl(y[o].x, below);
                rot[o].y = __shfl(y[o].y, below);
            }
#pragma unroll
            for (int o = 0; o < O; ++o) {
                const float2 p = lane ? rot[o] : (o ? rot[o > 0 ? o - 1 : 0] : yp);        /* lane 0: lane 63's previous output */
                const float pr = y[o].x * p.x + y[o].y * p.y;          /* w = y conj(p) */
                const float pi = y[o].y * p.x - y[o].x * p.y;
                const float q = (pr - pr) + (pi - pi);
                const float d = (pr == 0.0f && pi == 0.0f) ? 0.0f : atan2f(pi, pr) * kFaxInvPi + q;
                const float f = reverse ? -d : d;
                const int i = 64 * o + lane;
                if (i < hi) {
                    frow[BK + i] = f;
                    if (disc)
                        disc[o0 + i] = f;
                }
                if (i == hi - 1)
                    last = y[o];
            }
            /* the tile's last output, for the next tile's (or batch's) lane 0 */
            yp.x = __shfl(last.x, (hi - 1) & 63);
            yp.y = __shfl(last.y, (hi - 1) & 63);
        }
        __syncthreads();

        uint32_t cnt = 0u, mis = 0u;
        bool room = false;
        if (on) {
            cnt = fax_carries(acc, inc, (uint32_t)hi);                 /* the tile's pixels, <= 128 */
            mis = (uint32_t)(reinterpret_cast<uintptr_t>(pix + np) & 3u);
            room = (long long)np + (long long)cnt <= a.pix_stride;
#pragma unroll
            for (int o = 0; o < O; ++o) {
                const int i = 64 * o + lane;
                const uint32_t c0 = fax_carries(acc, inc, (uint32_t)i);
                if (i < hi && fax_carries(acc, inc, (uint32_t)i + 1u) != c0) {
                    const float *fp = frow + BK + i - (B - 1);
                    float v = fp[0];
                    for (int b = 1; b < B; ++b)
                        v = v + fp[b];
                    v = v * rb;
                    const float g = fmaf(mo.scale, v, mo.bias);
                    pb[mis + c0] = g > 0.0f ? (unsigned char)rintf(fminf(g, 255.0f)) : (unsigned char)0;
                    sidx[c0] = (unsigned char)i;
                }
            }
        }
        __syncthreads();

        if (on) {
            /* the pixels to memory: word `lane` of the LDS bytes is an aligned word of the row */
            const uint32_t w0 = 4u * (uint32_t)lane;
            const uint32_t b0 = w0 > mis ? w0 : mis, b1 = w0 + 4u < mis + cnt ? w0 + 4u : mis + cnt;
            if (room && lane < kFaxPixBytes / 4 && b1 > b0) {
                unsigned char *dst = pix + np;                         /* byte b of LDS goes to dst[b - mis] */
                if (b1 - b0 == 4u)
                    *reinterpret_cast<uint32_t *>(dst + ((long long)w0 - (long long)mis)) = *reinterpret_cast<const uint32_t *>(pb + w0);
                else
                    for (uint32_t b = b0; b < b1; ++b)
                        dst[b - mis] = pb[b];
            }
            /* the hysteresis and the white count as masks over the tile's pixels, lane k pixels k and k + 64 */
            unsigned long long hm[2], lm[2], wm[2], xm[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const uint32_t k = (uint32_t)(64 * g + lane);
                const uint32_t p = k < cnt ? pb[mis + k] : kFaxLow;    /* in between: no pixel */
                hm[g] = __ballot(p >= kFaxHigh);
                lm[g] = __ballot(p < kFaxLow);
                wm[g] = __ballot(p >= kFaxWhite);
            }
            const uint32_t before0 = fax_level(fax_below(hm[0], (uint32_t)lane), fax_below(lm[0], (uint32_t)lane), l.level);
            const uint32_t mid = fax_level(hm[0], lm[0], l.level);
            const uint32_t before1 = fax_level(fax_below(hm[1], (uint32_t)lane), fax_below(lm[1], (uint32_t)lane), mid);
            xm[0] = __ballot(((hm[0] >> lane) & 1ull) && !before0);
            xm[1] = __ballot(((hm[1] >> lane) & 1ull) && !before1);
            l.level = fax_level(hm[1], lm[1], mid);

            /* from line end to line end */
            const unsigned long long mtile = a.m0 + (unsigned long long)o0;
            uint32_t k = 0u;
            while (k < cnt) {
                const uint32_t rest = width - l.col, left = cnt - k;
                const uint32_t take = rest < left ? rest : left;
                if (l.col == 0u)
                    l.start = mtile + (unsigned long long)sidx[k];
                l.crossings += fax_count(xm, k, k + take);
                l.white += fax_count(wm, k, k + take);
                l.col += take;
                k += take;
                if (l.col == width) {
                    FaxLineRec r;
                    fax_line_end(l, mo, &r);
                    if (lane == 0 && (long long)nln < a.char_stride)
                        lines[nln] = r;
                    ++nln;
                }
            }
            l.pixels += cnt;
            if (room)
                np += cnt;
            acc = (uint32_t)((uint64_t)acc + (uint64_t)(uint32_t)hi * inc);
        }

        /* the last 16 of [16 before | tile] to the front */
        float keepf = 0.0f;
        if (on && lane < BK)
            keepf = frow[hi + lane];
        __syncthreads();
        if (on && lane < BK)
            frow[lane] = keepf;
        __syncthreads();
    }

    if (!w.have)
        return;
    if (lane == 0) {
        a.new_state[j].l = l;
        a.new_state[j].acc = acc;
        a.new_state[j].pad = 0u;
        a.new_state[j].y = yp;
        a.counts[j] = (long long)nln < a.char_stride ? nln : (uint32_t)a.char_stride;
        a.npix[j] = np;
    }
    if (lane < BK)
        a.new_state[j].f[lane] = frow[lane];
    /* the new carried record: the last W - 1 of [old record | batch]; an OFF receiver's batch is empty */
    dec_carry(a.new_hist, H, w, input, on ? a.n : 0);
}

hipError_t launch_fax(const FaxArgs &a, hipStream_t s)
{
    return dec_launch<&k_fax>(a, a.pix && a.pix_stride >= 1 && a.npix && (!a.disc || a.disc_stride >= a.n), kFaxLdsCap,
                              fax_lds_bytes(a.window), s);
}

static_assert(kFaxBack <= 64 && kFaxPixBytes / 4 <= 64 && kFaxTilePix == 128, "one lane per carried f and per pixel word, two pixels per lane");

} // namespace pddc
