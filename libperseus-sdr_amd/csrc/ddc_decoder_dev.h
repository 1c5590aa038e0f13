/*
 * ddc_decoder_dev.h -- the walk of the character decoders' kernels (gfx950 only): the filter in front of each decoder's
 * own part.  k_morse and k_psk are made of these functions, k_sitor of all but the filter (its complex pass is a copy of
 * k_fsk's); k_fsk walks the same way but spells it out (ddc_fsk.hip says why) and takes the launch from here; k_fax,
 * whose records are lines and not characters, is made of all of them.  The five
 * .hip files include it, behind their ddc_<decoder>.h, and nothing else
 * does; its constants and the receiver record are in ddc_decoder_rx.h, which the host files see too.
 *
 * Walk: a block owns G = 4 consecutive receivers, one wave each, and goes through the batch in tiles of TT = 256
 * samples.  The waves share nothing (each has its own row in LDS); a kernel's barriers are there for the reader and for
 * the order of a wave's own LDS traffic.
 *   prologue  dec_wave: the wave's receiver j and its table entry; the bank index and the flags go through readfirstlane,
 *             so whatever they select (the taps, the bank entry) is wave-uniform.
 *   input     DecInput: input idx of the receiver, idx >= -(W - 1); before the batch's first it comes from the carried
 *             record (W - 1 values, the newest last), zero where the receiver is fresh or cleared.
 *   stage     dec_stage: the wave stages its receiver's inputs from W - 1 before the tile's first sample of the batch to
 *             its last one: consecutive lanes, consecutive inputs, 8-byte loads.
 *   filter    dec_filter: lane l makes the O = 4 outputs l, l + 64, l + 128, l + 192 of the tile, each with accumulators
 *             of its own that meet the taps in ascending t: the bits are the definition's whatever O is.  A pass of 8
 *             real taps comes through the scalar cache into SGPRs; the last pass of a window that is no multiple of 8
 *             tests every tap (uniform).  Per tap and output 8 bytes of LDS feed 2 spelled fmaf.
 *   carry     dec_carry: after the last tile the wave writes the new carried inputs, the last W - 1 of [old record |
 *             batch] (an OFF receiver's batch is empty), from global memory into the other buffer.
 * Bits: one lane makes each value with one operation sequence (contraction is off from here on, every fmaf is spelled).
 * Bounds: DecInput reads z at 0 <= idx < n and the record at 0 <= e < W - 1, both of a receiver < nrx (receiver 0's
 *   where the wave has none: never dereferenced there, since such a wave is not ON and dec_carry is not reached);
 *   dec_stage writes slots first <= e < W - 1 + end with end <= TT, inside the row's dec_in_slots(W); dec_filter reads
 *   slot W - 1 + lane + 64 o - t, that is 0 .. W - 2 + TT (a lane outside the tile's samples may read a slot nobody
 *   staged: inside the wave's own row, and its value is dropped by the decoder), and the taps inside the bank entry's
 *   dec_row(W) floats, which the host pads; dec_carry writes 0 <= e < W - 1 of receiver j < nrx.
 */
#ifndef PDDC_DDC_DECODER_DEV_H
#define PDDC_DDC_DECODER_DEV_H

#include "ddc_decoder_rx.h"
#include "ddc_dev.h"
#include "ddc_host.h"

namespace pddc {

#pragma clang fp contract(off)

struct DecWave {
    int lane, wave, j;        /* j: the wave's receiver                                                          */
    bool have;                /* j < nrx                                                                         */
    int jr;                   /* j, or 0 without a receiver: what the wave's row pointers are made with          */
    uint32_t flags;           /* of the table entry, 0 without a receiver (uniform)                              */
    int bank;
};

__device__ __forceinline__ DecWave dec_wave(const DecRx *rx, int nrx)
{
    DecWave w;
    w.lane = (int)threadIdx.x & 63;
    w.wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    w.j = (int)blockIdx.x * kDecGroup + w.wave;
    w.have = w.j < nrx;
    w.jr = 0;
    DecRx r{ 0, 0u };
    if (w.have) {
        r = rx[w.j];
        w.jr = w.j;
    }
    w.flags = __builtin_amdgcn_readfirstlane(r.flags);
    w.bank = __builtin_amdgcn_readfirstlane(r.bank);
    return w;
}

struct DecInput {
    const float2 *zr, *old;   /* the receiver's row of z and its carried record                                  */
    int H;                    /* W - 1                                                                           */
    bool keep;                /* the carried inputs are read: the receiver is neither fresh nor cleared          */

    __device__ __forceinline__ float2 operator()(long long idx) const
    {
        if (idx < 0)
            return (keep && idx >= -(long long)H) ? old[H + idx] : make_float2(0.0f, 0.0f);
        return zr[idx];
    }
};

/* `hist_stride`: float2 per receiver of the carried record, whose first W - 1 are the inputs */
__device__ __forceinline__ DecInput dec_input(const DecWave &w, const float2 *z, long long z_stride, const float2 *hist,
                                              int hist_stride, int H)
{
    return DecInput{ z + (long long)w.jr * z_stride, hist + (long long)w.jr * hist_stride, H, !(w.flags & (kDecFresh | kDecClear)) };
}

/* the tile that begins at sample o0 of the batch (o0 < 0: in front of it), its samples first .. end - 1 the batch's */
__device__ __forceinline__ void dec_stage(float2 *row, const DecInput &in, int lane, long long o0, int first, int end)
{
    for (int e = first + lane; e < in.H + end; e += 64)
        row[e] = in(o0 - in.H + e);
}

/* one pass of kDecStep real taps hw[] from tap t0; p points at the lane's slot of output 0, tap 0 */
template <bool Guard>
__device__ __forceinline__ void dec_pass(const float2 *p, int t0, int W, const float (&hw)[kDecStep], float2 (&y)[kDecOut])
{
#pragma unroll
    for (int s = 0; s < kDecStep; ++s) {
        if (Guard && t0 + s >= W)
            break;
        const float h = hw[s];
#pragma unroll
        for (int o = 0; o < kDecOut; ++o) {
            const float2 z = p[64 * o - (t0 + s)];
            y[o].x = fmaf(h, z.x, y[o].x);
            y[o].y = fmaf(h, z.y, y[o].y);
        }
    }
}

/* y[o] = the filter's output at sample 64 o + lane of the staged tile; h: the bank entry's dec_row(W) real taps */
__device__ __forceinline__ void dec_filter(const float2 *row, int lane, int H, int W, const float PDDC_CONSTANT *h, float2 (&y)[kDecOut])
{
#pragma unroll
    for (int o = 0; o < kDecOut; ++o)
        y[o] = make_float2(0.0f, 0.0f);
    const float2 *p = row + H + lane;
    for (int t0 = 0; t0 < W; t0 += kDecStep) {
        float hw[kDecStep];
#pragma unroll
        for (int i = 0; i < kDecStep; ++i)
            hw[i] = h[t0 + i];
        if (t0 + kDecStep <= W)
            dec_pass<false>(p, t0, W, hw, y);
        else
            dec_pass<true>(p, t0, W, hw, y);
    }
}

/* the new carried inputs of receiver w.j (the wave has one) behind `used` samples of the batch */
__device__ __forceinline__ void dec_carry(float2 *new_hist, int hist_stride, const DecWave &w, const DecInput &in, long long used)
{
    for (int e = w.lane; e < in.H; e += 64)
        new_hist[(long long)w.j * hist_stride + e] = in(used - in.H + e);
}

/* Kernel<<<ceil(nrx / G), 64 G, lds>>>(a) for arguments whose common members are sound and whose own ones `extras_ok` says are */
template <auto Kernel, class Args> hipError_t dec_launch(const Args &a, bool extras_ok, size_t lds_cap, size_t lds, hipStream_t s)
{
    if (!extras_ok || a.n <= 0 || a.nrx <= 0 || a.nrx > kDecMaxRx || a.nbank < 1 || a.nbank > kDecMaxBank || a.window < 1 ||
        a.window > kDecMaxWindow || !a.z || a.z_stride < a.n || !a.chars || a.char_stride < 1 || !a.counts || !a.taps ||
        !a.bank || !a.rx || !a.state || !a.new_state || !a.hist || !a.new_hist)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nrx + kDecGroup - 1) / kDecGroup));
    return launch_dynamic_lds<Kernel>(lds_cap, grid, dim3(kDecThreads), lds, s, a);
}

} // namespace pddc
#endif
