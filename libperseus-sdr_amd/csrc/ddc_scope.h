/*
 * ddc_scope.h -- internal launch interface between the scope's host code (ddc_scope.cpp) and its gfx950 kernel
 * (ddc_scope.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_SCOPE_H
#define PDDC_DDC_SCOPE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kScopeMaxSlots = 1024, kScopeMaxSrc = 1024;
static constexpr int kScopeMinN = 256, kScopeMaxN = 4096;
static constexpr int kScopeMaxAvg = 4096;
static constexpr int kScopeMinHopDiv = 16;              /* hop >= nfft / 16                                         */
static constexpr uint32_t kScopeCentered = 1u;          /* PDDC_SCOPE_CENTERED                                      */

/* one display slot as the kernel sees it */
struct ScopeSlot {
    int row;            /* the watched row, or -1: off                                                               */
    uint32_t fresh;     /* retargeted since the last launch: its carried samples and partial line read as zeros       */
};

/* The launch works on the slot's series from the start of the first incomplete segment before the batch: index v < clen
 * is the carried sample v, index v >= clen is z[row][v - clen].  New segment q (0 <= q < nseg) begins at v = q hop; it
 * is segment i0 + q of the line under way, lines being `avg` segments long. */
struct ScopeArgs {
    const float2 *z;          /* z[row * z_stride + i], i < n: complex float32                                       */
    long long z_stride;
    long long n;              /* samples per row of this launch, > 0                                                 */
    const ScopeSlot *slots;   /* [nslots]                                                                            */
    int nslots;
    float *lines;             /* lines[(j * line_stride + m) * nfft + k], m < nlines                                 */
    long long line_stride;
    const float2 *old_carry;  /* [nslots][nfft]: the first clen are read (not of a fresh or an off slot)             */
    float2 *new_carry;        /* ...: the first new_clen are written                                                 */
    const float *old_part;    /* [nslots][nfft]: the sum of the i0 segments of the line under way (i0 > 0)           */
    float *new_part;          /* ...: written when the batch ends inside a line                                      */
    const float *window;      /* [nfft]                                                                              */
    const float *twiddles;    /* spectrum_build_twiddles(nfft)                                                       */
    int hop, avg;
    int clen, new_clen;       /* < nfft                                                                              */
    int i0;                   /* segments the line under way already holds, < avg                                    */
    long long nseg;           /* segments this launch completes                                                      */
    long long nlines;         /* lines this launch completes: (i0 + nseg) / avg                                      */
    int nunits;               /* nlines, + 1 when a partial line is left behind: (i0 + nseg) % avg != 0               */
    uint32_t flags;           /* kScopeCentered                                                                      */
};

/* segments of one block pass (a block's items are consecutive (slot, line) pairs, one per group of threads) */
int scope_items_per_block(int nfft);
/* blocks of the launch, 0 when it is past what a grid holds */
uint64_t scope_blocks(int nfft, int nslots, int nunits);
/* k_scope<nfft>: one launch -- the lines, the partial line and the carried samples */
hipError_t launch_scope(int nfft, const ScopeArgs &a, hipStream_t s);

} // namespace pddc
#endif
