/*
 * ddc_channelizer.hip -- the channelizer: M uniform channels of the packed ADC stream as time series (gfx950 only).
 *
 *   k_channelize<M, P, Q>   polyphase filter bank by weighted overlap-add: prototype of L = P M taps, hop D = M / Q
 *                (Q = 1 critically sampled, Q = 2 oversampled by 2).  Per row s: u[r] = sum_p w[r + p M] x[s D + r + p M],
 *                the M-point transform of u (ddc_fft_dev.h, the panorama's), times (-1)^(k s) for Q = 2, the channels
 *                (first + i) mod M, i < count, stored as complex float32, row-major.
 *   k_channelize_list<M, P, Q>   the same rows, but only the n <= 1024 channels of a LIST are written, n values per row in
 *                the list's order: out[s n + i] = y[s][channels[i]].  The body is k_channelize's (channelize_rows.inc);
 *                only the last pass's store differs: a table slot[bin] (int16, -1: not listed) sits in LDS behind the ring,
 *                2 M bytes, and a listed bin goes to column slot[bin].  A value's bits are the range form's.
 *   k_channelize_tail       the packed tail carried to the next batch (ddc_packed.h).
 *
 * Walk: block b owns the RUN of consecutive rows [b run, (b + 1) run).  The stream is cut into UNITS of D samples; row s
 * needs units s .. s + P Q - 1, of which only the newest comes from HBM (3 x global_load_dwordx4 per 8 samples, loaded
 * one row ahead into registers).  The P Q - 1 older ones sit PACKED (6 B/sample) in an LDS ring: 6 (L - D) bytes.  A
 * thread folds exactly the groups of 8 samples it loaded itself (unit t, group g  ->  point 8 g + (t - s mod Q) D of u),
 * so the ring is thread-private spill space: no barrier guards it, and a lane's b128 accesses are consecutive.  A run's
 * first row reads its P Q - 1 older units from HBM as well (the run's "porch": (P Q - 1) / run of the input re-read).
 * The window values a thread needs (16 P floats) stay in registers for the whole run.
 * Bits: a row's fold runs p = 0 .. P-1 with one multiply and P - 1 fused multiply-adds per component whatever the
 * source of a unit; nothing is shared between rows.  The bits of a row depend on (M, D, P, w, samples) alone -- not on
 * grid, run length, batch cut or channel range.  No atomics.
 * Stores: the last pass holds bins j + r M/R per thread: consecutive lanes, consecutive channels -- 512 contiguous
 * bytes per wave and register, nontemporal; the range is a rotation of the index and a predicate.  The list form
 * stores each listed bin on its own (8 bytes, nontemporal, wherever slot[bin] says): DESIGN.md 4 "Channel list".
 * LDS and registers per (M, P, Q): DESIGN.md 4 "Channelizer".
 */
#include "ddc_channelizer.h"
#include "ddc_spectrum.h"
#include "ddc_fft_dev.h"

namespace pddc {

static constexpr size_t kChanLdsPerCu = 160 * 1024;

static int chan_r2(int m) { return m == 1024 ? 4 : m == 2048 ? 8 : 16; }

size_t channelize_lds_bytes(int nchan, int taps_per_branch, int hop, bool list)
{
    const size_t tw = (size_t)(15 * 16 + (chan_r2(nchan) - 1) * 256);
    return 8 * ((size_t)nchan + tw) + 6 * ((size_t)taps_per_branch * nchan - hop) + (list ? 2 * (size_t)nchan : 0);
}

int channelize_target_blocks(int nchan, int taps_per_branch, int hop, int ncu, bool list)
{
    const int plan = nchan == 1024 ? SpecPlan<1024>::BLOCKS_PER_CU
                     : nchan == 2048 ? SpecPlan<2048>::BLOCKS_PER_CU
                                     : SpecPlan<4096>::BLOCKS_PER_CU;
    int fit = (int)(kChanLdsPerCu / channelize_lds_bytes(nchan, taps_per_branch, hop, list));
    fit = fit < 1 ? 1 : fit > plan ? plan : fit;
    return fit * ncu;
}

template <int M, int P, int Q>
__global__ __launch_bounds__(M / 16 < 256 ? M / 16 : 256) void k_channelize(ChannelizeArgs a)
{
#define PDDC_CHAN_LIST 0
#include "channelize_rows.inc"
#undef PDDC_CHAN_LIST
}

template <int M, int P, int Q>
__global__ __launch_bounds__(M / 16 < 256 ? M / 16 : 256) void k_channelize_list(ChannelizeArgs a)
{
#define PDDC_CHAN_LIST 1
#include "channelize_rows.inc"
#undef PDDC_CHAN_LIST
}

__global__ __launch_bounds__(256) void k_channelize_tail(PackedCarryArgs p)
{
    PDDC_CARRY_TAIL(p, 0)
}

/* ------------------------------------------------------------------------ */
template <int M, int P, int Q> static hipError_t launch_channelize_t(const ChannelizeArgs &a, hipStream_t s)
{
    constexpr int NT = M / 16 < 256 ? M / 16 : 256;
    const long long blocks = (a.nrows + a.run - 1) / a.run;
    if (a.slot) {
        if (a.count < 1 || a.count > kChanMaxList)
            return hipErrorInvalidValue;
        const size_t lds = channelize_lds_bytes(M, P, M / Q, true);
        return launch_dynamic_lds<&k_channelize_list<M, P, Q>>(lds, dim3((unsigned)blocks), dim3(NT), lds, s, a);
    }
    const size_t lds = channelize_lds_bytes(M, P, M / Q, false);
    return launch_dynamic_lds<&k_channelize<M, P, Q>>(lds, dim3((unsigned)blocks), dim3(NT), lds, s, a);
}

template <int M, int P> static hipError_t launch_channelize_q(int q, const ChannelizeArgs &a, hipStream_t s)
{
    return q == 1 ? launch_channelize_t<M, P, 1>(a, s) : launch_channelize_t<M, P, 2>(a, s);
}

template <int M> static hipError_t launch_channelize_p(int p, int q, const ChannelizeArgs &a, hipStream_t s)
{
    switch (p) {
    case 1: return launch_channelize_q<M, 1>(q, a, s);
    case 2: return launch_channelize_q<M, 2>(q, a, s);
    case 4: return launch_channelize_q<M, 4>(q, a, s);
    case 8:
        if constexpr (8 * M <= kChanMaxProto)
            return launch_channelize_q<M, 8>(q, a, s);
        return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_channelize(int nchan, int taps_per_branch, int hop, const ChannelizeArgs &a, hipStream_t s)
{
    if (a.nrows <= 0 || a.run <= 0 || (hop != nchan && 2 * hop != nchan))
        return hipErrorInvalidValue;
    const int q = nchan / hop;
    switch (nchan) {
    case 1024: return launch_channelize_p<1024>(taps_per_branch, q, a, s);
    case 2048: return launch_channelize_p<2048>(taps_per_branch, q, a, s);
    case 4096: return launch_channelize_p<4096>(taps_per_branch, q, a, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_channelize_tail(const PackedCarryArgs &a, hipStream_t s)
{
    const int blocks = carry_tail_blocks(a.new_len);
    if (blocks <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_channelize_tail, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
