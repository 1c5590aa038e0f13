/*
 * ddc_channelizer.h -- internal launch interface between the channelizer's host code (ddc_channelizer.cpp) and its
 * gfx950 kernels (ddc_channelizer.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_CHANNELIZER_H
#define PDDC_DDC_CHANNELIZER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kChanMaxProto = 16384;

struct ChannelizeArgs {
    const uint8_t *tail;      /* the packed samples carried from the batches before: tail_len of them          */
    const uint8_t *batch;     /* this batch                                                                    */
    long long tail_len;       /* samples, a multiple of 8, < proto_len                                         */
    long long nrows;          /* rows this launch completes; row j starts at sample j*hop of tail-then-batch   */
    long long run;            /* rows per block: block b owns rows [b run, min((b+1) run, nrows))              */
    unsigned row_parity;      /* the stream's index of row 0 of this launch, mod 2 (the hop M/2 sign)          */
    int first, count;         /* channels (first + i) mod M, i < count                                         */
    const float *proto;       /* [P M]                                                                         */
    const float *twiddles;    /* spectrum_build_twiddles(M)                                                    */
    float *out;               /* [nrows][count] complex float32                                                */
};

/* bytes of LDS a block of k_channelize<nchan, taps_per_branch, nchan / hop> takes */
size_t channelize_lds_bytes(int nchan, int taps_per_branch, int hop);
/* the block count the launcher aims at on a device of ncu compute units (what fits side by side) */
int channelize_target_blocks(int nchan, int taps_per_branch, int hop, int ncu);
/* k_channelize: ceil(nrows / run) blocks */
hipError_t launch_channelize(int nchan, int taps_per_branch, int hop, const ChannelizeArgs &a, hipStream_t s);

/* new_tail[0 .. new_len) = (tail-then-batch)[keep_from .. keep_from + new_len), samples; all multiples of 8 */
struct ChannelizeTailArgs {
    const uint8_t *tail, *batch;
    uint8_t *new_tail;
    long long tail_len, keep_from, new_len;
};
hipError_t launch_channelize_tail(const ChannelizeTailArgs &a, hipStream_t s);

} // namespace pddc
#endif
