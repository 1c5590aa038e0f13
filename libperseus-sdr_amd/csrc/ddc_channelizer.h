/*
 * ddc_channelizer.h -- internal launch interface between the channelizer's host code (ddc_channelizer.cpp) and its
 * gfx950 kernels (ddc_channelizer.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_CHANNELIZER_H
#define PDDC_DDC_CHANNELIZER_H

#include "ddc_packed.h"

namespace pddc {

static constexpr int kChanMaxProto = 16384;
static constexpr int kChanMaxList = kChannelListMax;   /* channels of a list: the host validation's limit (ddc_host.h) */

struct ChannelizeArgs {
    PackedStream in;          /* tail-then-batch (ddc_packed.h); the tail is shorter than proto_len            */
    long long nrows;          /* rows this launch completes; row j starts at sample j*hop of tail-then-batch   */
    long long run;            /* rows per block: block b owns rows [b run, min((b+1) run, nrows))              */
    unsigned row_parity;      /* the stream's index of row 0 of this launch, mod 2 (the hop M/2 sign)          */
    int first, count;         /* channels (first + i) mod M, i < count; list form: count = n, first unused      */
    const float *proto;       /* [P M]                                                                         */
    const float *twiddles;    /* spectrum_build_twiddles(M)                                                    */
    float *out;               /* [nrows][count] complex float32                                                */
    const short *slot;        /* NULL: the range form.  List form: [M], the column of bin k in a row, -1: not listed */
};

/* bytes of LDS a block of k_channelize<nchan, taps_per_branch, nchan / hop> takes (list: of k_channelize_list, which
 * keeps the slot table of 2 nchan bytes behind the ring) */
size_t channelize_lds_bytes(int nchan, int taps_per_branch, int hop, bool list = false);
/* the block count the launcher aims at on a device of ncu compute units (what fits side by side) */
int channelize_target_blocks(int nchan, int taps_per_branch, int hop, int ncu, bool list = false);
/* k_channelize, or k_channelize_list when a.slot is set: ceil(nrows / run) blocks */
hipError_t launch_channelize(int nchan, int taps_per_branch, int hop, const ChannelizeArgs &a, hipStream_t s);

/* k_channelize_tail: the carried tail for the next batch (ddc_packed.h), a launch of its own; none when new_len == 0 */
hipError_t launch_channelize_tail(const PackedCarryArgs &a, hipStream_t s);

} // namespace pddc
#endif
