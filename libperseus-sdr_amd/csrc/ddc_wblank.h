/*
 * ddc_wblank.h -- internal launch interface between the wideband blanker's host code (ddc_wblank.cpp) and its gfx950
 * kernels (ddc_wblank.hip).  Not part of the public ABI (that is include/perseus_ddc.h, pddc_wblank_*).
 *
 * A batch is three launches behind one memset of the sums: k_wblank_sums reads the batch and adds every group of 8
 * samples into its metering block's sum; k_wblank_means turns the sums into the blocks' references and writes the state
 * the device carries on; k_wblank_gate reads the references and the carried tail followed by the batch, takes the
 * triggers and writes the output, its last blocks copy the tail for the next batch.  No workgroup waits for another:
 * what a tile needs of its neighbours' triggers it takes again itself.
 */
#ifndef PDDC_DDC_WBLANK_H
#define PDDC_DDC_WBLANK_H

#include "ddc_packed.h"
#include "ddc_wblank_gate.h"

namespace pddc {

static constexpr int kWbTile = 2048;                      /* outputs of one tile: 256 threads, a group of 8 each      */
/* the most samples one round of launches takes: what the sums' and the references' buffers are made for.  Measured on a
 * batch of 2^28 (profiles/r27/wblank_time.txt): rounds of 2^21 and 2^23 samples, short enough for the second read to come
 * from the memory-side cache, are slower than rounds of 2^26 -- the cache gives nothing back and a round costs its launches
 * and the ramp of its grids; 2^26 keeps the two buffers at 8 MiB each for B = 64.  "wblank_chunk" can only shorten it. */
static constexpr long long kWbMaxChunk = 1ll << 26;

/* what the device carries between batches; three of them, like the tail and its trigger bits (ddc_wblank.cpp) */
struct WbState {
    uint64_t hist[kWbMaxHistory];     /* the last H complete block sums, oldest first; kWbNoBlock in front of the stream */
    uint64_t partial;                 /* the sum of the open block so far                                               */
    uint64_t triggers, blanked;
    uint64_t mean;                    /* the reference of the open block                                                */
};

/* block sums a round of n <= kWbMaxChunk samples can touch, with the open one behind them */
inline size_t wblank_sums_len(int b) { return (size_t)(kWbMaxChunk >> b) + 8; }

struct WbArgs {
    PackedStream in;            /* the carried tail, wb_tail_len(D) samples always, then the batch                    */
    long long n;                /* samples of the batch, a multiple of 8                                              */
    uint64_t N;                 /* stream index of the batch's first sample                                           */
    int b, H, W, r, D, TL;
    uint32_t thr16, on;
    const WbState *st;          /* as the batches before left it                                                      */
    WbState *new_st;
    uint64_t *sums;             /* wblank_sums_len(b): sums[i] of block (N >> b) + i; cleared in front of k_wblank_sums */
    uint64_t *means;            /* the same length: the blocks' references                                            */
    long long nblocks;          /* blocks the batch adds to or completes: wb_blocks_touched                           */
    const uint8_t *bits;        /* trigger bits of the tail, a byte per group of 8                                    */
    uint8_t *new_bits;
    uint8_t *out;               /* n samples                                                                          */
    long long run;              /* samples one workgroup of k_wblank_gate walks, a multiple of kWbTile                */
    int tile_blocks;            /* ceil(n / run); the blocks behind them carry the tail                               */
    PackedCarryArgs carry;
};

hipError_t launch_wblank_sums(const WbArgs &a, int max_blocks, hipStream_t s);
hipError_t launch_wblank_means(const WbArgs &a, hipStream_t s);
hipError_t launch_wblank_gate(const WbArgs &a, hipStream_t s);

} // namespace pddc
#endif
