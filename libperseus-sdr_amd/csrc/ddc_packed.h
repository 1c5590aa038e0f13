/*
 * ddc_packed.h -- the carried packed stream, the one home of its format: what a reader of the packed ADC stream that
 * works on overlapping windows (the panorama, the channelizer) knows about "tail-then-batch".  Internal.
 *
 * 6 bytes per sample.  The stream a batch sees is the TAIL (the samples the windows of the batches before left over,
 * fewer than a window) followed by the BATCH; every length is a multiple of 8 samples = 48 bytes = three 16-byte
 * chunks, so a group of 8 samples lies on one side of the seam and both sides are 16-byte aligned.  The tail is
 * double-buffered by the host: a batch's kernels read d_tail[cur] and its carry copies the samples from keep_from on
 * into d_tail[cur ^ 1]; `cur` flips and the counters move only after every launch of the batch was accepted.
 *
 *   device:  PackedStream (the view, load_group), PDDC_UNPACK_GROUP_MSB + kPackedUnpackScale, PackedCarryArgs +
 *            PDDC_CARRY_TAIL + carry_tail_blocks
 *   host:    PackedCarry (buffers and counters: alloc / free / reset, check, plan, stream, carry, commit)
 */
#ifndef PDDC_DDC_PACKED_H
#define PDDC_DDC_PACKED_H

#include "ddc_dev.h"
#include "ddc_host.h"

namespace pddc {

static constexpr float kPackedUnpackScale = 0x1.000002p-31f;   /* as k_unpack24: (float)(v24 * 256) * this */

struct PackedStream {
    const uint8_t *tail;      /* the packed samples carried from the batches before: tail_len of them   */
    const uint8_t *batch;     /* this batch                                                             */
    long long tail_len;       /* samples, a multiple of 8, less than a window                           */

    /* the 48 bytes of samples v .. v + 7 of tail-then-batch, v a multiple of 8: three nontemporal 16-byte loads */
    __device__ __forceinline__ void load_group(long long v, u32x4 (&raw)[3]) const
    {
        const uint8_t *src = v < tail_len ? tail + v * 6 : batch + (v - tail_len) * 6;
        const u32x4 *s = reinterpret_cast<const u32x4 *>(src);
        raw[0] = __builtin_nontemporal_load(s);
        raw[1] = __builtin_nontemporal_load(s + 1);
        raw[2] = __builtin_nontemporal_load(s + 2);
    }
};

/* Samples 2h and 2h + 1 (h = 0 .. 3) of a loaded group `raw` (u32x4[3]): declares int32_t i0, q0, i1, q1 and fills them.
 * 12 bytes = I0 Q0 I1 Q1, MSB-aligned (value * 256) as k_unpack24 places them; times kPackedUnpackScale they are the
 * bit-exact pddc_unpack24_f32 values.  A macro, like PDDC_CARRY_TAIL below, and not a function on purpose: a function
 * inlined into these kernels moves their stack slots, and with them the order in which the compiler numbers values --
 * the same operations then come out in another instruction order.  As text in the kernel they compile to the
 * instructions the kernels had when each held its own copy (profiles/r12/refactor_compare.txt). */
#define PDDC_UNPACK_GROUP_MSB(raw, h, i0, q0, i1, q1)                                                                  \
    const uint32_t a__ = (raw)[(3 * (h)) >> 2][(3 * (h)) & 3], b__ = (raw)[(3 * (h) + 1) >> 2][(3 * (h) + 1) & 3],     \
                   c__ = (raw)[(3 * (h) + 2) >> 2][(3 * (h) + 2) & 3];                                                 \
    int32_t i0, q0, i1, q1;                                                                                            \
    unpack2_msb(a__, b__, c__, i0, q0, i1, q1)

/* the carried tail for the NEXT batch: new_tail[0 .. new_len) = (tail-then-batch)[keep_from .. keep_from + new_len),
 * samples; all multiples of 8 */
struct PackedCarryArgs {
    const uint8_t *tail, *batch;
    uint8_t *new_tail;
    long long tail_len, keep_from, new_len;
};

/* The carry copy, the last statement of a kernel of 256-thread blocks: the blocks first_block .. gridDim.x - 1 of the
 * launch copy new_tail[c] = (tail-then-batch)[keep_from*6/16 + c], 16-byte chunks; `p` a PackedCarryArgs. */
#define PDDC_CARRY_TAIL(p, first_block)                                                                                \
    const long long nchunks = (p).new_len * 6 / 16;                                                                    \
    const long long tail_chunks = (p).tail_len * 6 / 16, from = (p).keep_from * 6 / 16;                                \
    const long long stride = (long long)(gridDim.x - (first_block)) * 256;                                             \
    for (long long c = (long long)(blockIdx.x - (first_block)) * 256 + threadIdx.x; c < nchunks; c += stride) {        \
        const long long v = from + c;                                                                                  \
        const u32x4 *src = v < tail_chunks ? reinterpret_cast<const u32x4 *>((p).tail) + v                             \
                                           : reinterpret_cast<const u32x4 *>((p).batch) + (v - tail_chunks);           \
        reinterpret_cast<u32x4 *>((p).new_tail)[c] = *src;                                                             \
    }

/* blocks a launch gives PDDC_CARRY_TAIL: one per 256 chunks, at most 32 (0: nothing to carry) */
inline int carry_tail_blocks(long long new_len)
{
    const long long nchunks = new_len * 6 / 16;
    return (int)((nchunks + 255) / 256 < 32 ? (nchunks + 255) / 256 : 32);
}

/* ---- host: the object's side of it ------------------------------------------------------------------------------- */
struct PackedCarry {
    uint8_t *d_tail[2] = { nullptr, nullptr };      /* window * 6 bytes each; a batch reads [cur] and writes [cur ^ 1] */
    int cur = 0;
    uint64_t tail_len = 0;                          /* samples in d_tail[cur], less than a window */
    uint64_t samples = 0;                           /* stream length since alloc / reset          */

    struct Plan {
        uint64_t len;                               /* tail-then-batch                                        */
        uint64_t n_complete;                        /* windows that end in it                                 */
        uint64_t keep_from, new_len;                /* the first sample the next window needs; the new tail   */
    };

    hipError_t alloc(size_t window)
    {
        const hipError_t e = hipMalloc(&d_tail[0], window * 6);
        return e != hipSuccess ? e : hipMalloc(&d_tail[1], window * 6);
    }
    void free()
    {
        hipFree(d_tail[0]);
        hipFree(d_tail[1]);
    }
    void reset() { tail_len = samples = 0; }

    /* a batch's arguments: PDDC_OK or PDDC_EINVAL with its message */
    static int check(const void *d_packed, size_t nsamples)
    {
        if (nsamples % 8)
            return pddc_set_error_(PDDC_EINVAL, "nsamples (%zu) must be a multiple of 8", nsamples);
        if (nsamples && (!d_packed || ((uintptr_t)d_packed & 15)))
            return pddc_set_error_(PDDC_EINVAL, "d_packed must be a 16-byte aligned device pointer");
        return PDDC_OK;
    }
    Plan plan(size_t nsamples, int window, int hop) const
    {
        Plan p;
        p.len = tail_len + nsamples;
        p.n_complete = windows_complete(window, hop, p.len);
        p.keep_from = p.n_complete * (uint64_t)hop;
        p.new_len = p.len - p.keep_from;
        return p;
    }
    PackedStream stream(const void *d_packed) const
    {
        return PackedStream{ d_tail[cur], static_cast<const uint8_t *>(d_packed), (long long)tail_len };
    }
    PackedCarryArgs carry(const Plan &p, const void *d_packed) const
    {
        return PackedCarryArgs{ d_tail[cur],         static_cast<const uint8_t *>(d_packed), d_tail[cur ^ 1],
                                (long long)tail_len, (long long)p.keep_from,                 (long long)p.new_len };
    }
    /* only after the batch's last launch was accepted */
    void commit(const Plan &p, size_t nsamples)
    {
        cur ^= 1;
        tail_len = p.new_len;
        samples += nsamples;
    }
};

} // namespace pddc
#endif
