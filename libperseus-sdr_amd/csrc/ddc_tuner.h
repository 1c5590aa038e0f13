/*
 * ddc_tuner.h -- internal launch interface between the tuner's host code (ddc_tuner.cpp) and its gfx950 kernels
 * (ddc_tuner.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_TUNER_H
#define PDDC_DDC_TUNER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kTuneMaxRx = 1024, kTuneMaxTaps = 512, kTuneMaxDecim = 64;
static constexpr int kTuneThreads = 256;
static constexpr size_t kTuneLdsBytes = 64 * 1024;      /* the z tile of a block: at most this much */

/* one receiver as the kernels see it; the table is sorted by column */
struct TuneRx {
    int col;            /* the column of its channel in the rows' matrix: (k - first) mod M, < count */
    int32_t res;        /* r: word minus channel centre                                               */
    uint32_t phi;       /* the phase offset                                                           */
    int rx;             /* the caller's index: row of the output and of the carried z                 */
};

/* Rows are counted in u: u = 0 is the first row the launch's first output needs (stream row m0 R).  Row u comes from
 * the carried z (u < off: carry[rx * carry_cap + u]) or from the matrix (rows[(u - off) * count + col]); off may be
 * negative (decim > ntaps: rows nobody needs lie between two outputs). */
struct TuneArgs {
    const float2 *rows;       /* [nrows][count] complex float32                                                */
    long long nrows;
    int count;
    const TuneRx *rx;         /* [nrx], sorted by col                                                          */
    int nrx;
    const float2 *carry;      /* [nrx][carry_cap] z values of the rows before this batch                       */
    int carry_cap;
    long long off;
    uint32_t phase0;          /* (m0 R D) mod 2^32: row u has s D = phase0 + u D (mod 2^32)                     */
    uint32_t hop;             /* D                                                                             */
    const float *taps;        /* [ntaps]                                                                       */
    int ntaps, decim;
    long long nout;           /* outputs per receiver of this launch                                           */
    long long run;            /* outputs per block: block x owns [x run, min((x + 1) run, nout)), a multiple of co */
    int co;                   /* outputs per tile of a block                                                   */
    float2 *out;              /* out[rx * out_stride + m]                                                      */
    long long out_stride;
};

/* receivers per block (consecutive entries of the sorted table) and outputs per tile for a filter of ntaps, decim */
int tune_group(int ntaps);
int tune_tile_outputs(int ntaps, int decim);
/* k_tune: grid (ceil(nout / run), ceil(nrx / group)) */
hipError_t launch_tune(const TuneArgs &a, hipStream_t s);

/* new_carry[rx][q] = z of row u = keep_u + q, q < new_len (from the old carry or mixed from the matrix) */
struct TuneCarryArgs {
    TuneArgs t;               /* rows, rx, carry, off, phase0, hop as above */
    float2 *new_carry;
    long long keep_u;
    int new_len;
};
hipError_t launch_tune_carry(const TuneCarryArgs &a, hipStream_t s);

} // namespace pddc
#endif
