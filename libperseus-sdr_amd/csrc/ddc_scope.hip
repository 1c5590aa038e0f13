/*
 * ddc_scope.hip -- the scope: averaged power-spectrum lines of the receivers' own complex series, per display slot
 * (gfx950 only).
 *
 *   k_scope<N>   one item per (line unit, slot): the unit's segments in ascending order -- load (complex float32, 8 B per
 *                sample and lane, consecutive lanes consecutive samples), times the window, N-point transform inside the
 *                item's group of threads (registers + LDS), |X|^2 added to per-thread per-bin sums -- then the line, staged
 *                through LDS and stored 16 B per lane, to the caller's lines or, for the unit the batch ends in, to the
 *                carried partial line.  Behind the items' blocks one block per slot copies the carried samples.  One
 *                launch per batch; no atomics, no scratch, nothing cleared.
 *
 * Transform: the Stockham passes of ddc_fft_dev.h with FramePlan's radices, the noise reduction's too.  scope_swz,
 * scope_bfly and scope_put below are this file's own copies of that header's fft_swz, fft_load + fft_bfly and fft_put, kept
 * on purpose: on the shared steps k_scope gave other bits at every size with three passes (NOTEBOOK R24.1).  A group has
 * N / R1 threads, so that the loads of a thread ARE its first butterfly (samples t + r N/R1): the first pass reads no LDS.  N = 256 is 16 x 16 with 16
 * threads per segment and N = 512 is 8 x 8 x 8 with 64; a block of N = 256 holds four items, so every wave is full;
 * from N = 512 on a block is one item of 64, 64, 128 and 256 threads.  The first pass's image is XOR-swizzled (its 16- or
 * 8-point rows would otherwise put a lane group on one bank set), the later images are plain.  Twiddles and window are
 * read from global memory (L1 / L2; the same few KB for every block); both are loop invariant.
 *
 * Walk: item w = unit * nslots + slot, so the items of a block share their unit (and with it the segment range) unless
 * nslots is no multiple of the block's items; the block walks the union of its items' ranges and an item outside its own
 * computes on zeros and adds nothing: every barrier is block uniform.  A line's sum stays in one thread per bin from its
 * first segment to its last, in ascending order; a line that began in an earlier batch starts from the carried partial
 * sum, every other from +0 (+0 + p has the bits of p for every p = re^2 + im^2).
 * Overlapping segments (hop < nfft) are consecutive iterations of one block: the re-read comes from L1 / L2.  The next
 * segment's samples are loaded into registers before the present one's later passes.
 * The same instruction sequence serves every segment: a sample is selected from the carried samples or from z by its
 * index, nothing else differs.
 */
#include "ddc_scope.h"
#include "ddc_fft_dev.h"

namespace pddc {

/* the image the first pass (radix S) writes: the low bits of a row XOR the row's number; 0: plain */
template <int S> __device__ __forceinline__ int scope_swz(int i) { return S ? i ^ ((i / (S ? S : 1)) & (S - 1)) : i; }

/* a pass after the first: the thread's N / R / TS butterflies from the image, twiddled and transformed */
template <int N, int TS, int R, int NS, int SWZ>
__device__ __forceinline__ void scope_bfly(const float2 *buf, const float2 *tw, int t, float2 (&v)[N / R / TS][R])
{
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b) {
        const int j = t + b * TS;
#pragma unroll
        for (int r = 0; r < R; ++r)
            v[b][r] = buf[scope_swz<SWZ>(j + r * (N / R))];
    }
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b) {
        const int k = (t + b * TS) & (NS - 1);
#pragma unroll
        for (int r = 1; r < R; ++r)
            v[b][r] = cmulw(v[b][r], tw[(r - 1) * NS + k]);
        fft_reg<R>(v[b]);
    }
}

/* ... and its outputs into the (plain) image of the next pass */
template <int N, int TS, int R, int NS>
__device__ __forceinline__ void scope_put(float2 *buf, int t, const float2 (&v)[N / R / TS][R])
{
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b) {
        const int j = t + b * TS, k = j & (NS - 1), j0 = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r)
            buf[j0 + r * NS] = v[b][fft_pos<R>(r)];
    }
}

/* the last pass's bins to the sums: bin t + b TS + r N/R at acc[b R + r] */
template <int N, int TS, int R>
__device__ __forceinline__ void scope_add(const float2 (&v)[N / R / TS][R], bool act, float (&acc)[N / TS])
{
#pragma unroll
    for (int b = 0; b < N / R / TS; ++b)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float2 x = v[b][fft_pos<R>(r)];
            const float pw = x.x * x.x + x.y * x.y;
            if (act)
                acc[b * R + r] += pw;
        }
}

template <int N>
__global__ __launch_bounds__(N / FramePlan<N>::R1 * FramePlan<N>::G) void k_scope(ScopeArgs p)
{
    using Plan = FramePlan<N>;
    constexpr int R1 = Plan::R1, R2 = Plan::R2, R3 = Plan::R3, G = Plan::G;
    constexpr int TS = N / R1, NT = TS * G;
    constexpr int STRIDE = N + (G > 1 ? 16 : 0);  /* neighbouring groups of a wave on different banks */
    constexpr int RL = R3 > 1 ? R3 : R2;          /* the last pass: bin t + b TS + r N/RL at acc[b RL + r] */
    constexpr int NACC = N / TS;
    static_assert(NACC == R1 && TS * R1 == N && (N / RL) % TS == 0, "a thread's loads are its first butterfly");
    __shared__ __attribute__((aligned(16))) float2 lds[G * STRIDE];

    const int tid = threadIdx.x, g = tid / TS, t = tid % TS;
    const long long nitems = (long long)p.nunits * p.nslots;
    const long long nwork = (nitems + G - 1) / G;
    const long long shift = p.nseg * p.hop;

    /* index v of the slot's series (ddc_scope.h): a carried sample, or one of this batch */
    auto sample = [&](int j, const ScopeSlot &sl, long long v) -> float2 {
        if (v < p.clen)
            return sl.fresh ? make_float2(0.0f, 0.0f) : p.old_carry[(size_t)j * N + v];
        return p.z[sl.row * p.z_stride + (v - p.clen)];
    };

    if ((long long)blockIdx.x >= nwork) {
        /* the samples from the start of the first segment this batch leaves incomplete: v = shift .. clen + n */
        const int j = (int)((long long)blockIdx.x - nwork);
        const ScopeSlot sl = p.slots[j];
        if (sl.row < 0)
            return;
        for (int i = tid; i < p.new_clen; i += NT)
            p.new_carry[(size_t)j * N + i] = sample(j, sl, shift + i);
        return;
    }

    float2 *buf = lds + g * STRIDE;
    const long long w0 = (long long)blockIdx.x * G, w = w0 + g;
    const bool valid = w < nitems;
    const int j = valid ? (int)(w % p.nslots) : 0;
    const long long u = valid ? w / p.nslots : 0;
    ScopeSlot sl = p.slots[j];
    if (!valid)
        sl.row = -1;
    const bool live = sl.row >= 0;
    /* the item's new segments q (ddc_scope.h), and the block's: the union over its items */
    const long long qlo = max(0LL, u * p.avg - p.i0), qhi = min(p.nseg, (u + 1) * p.avg - p.i0);
    const long long ua = w0 / p.nslots, ub = min(w0 + G - 1, nitems - 1) / p.nslots;
    const long long QLO = max(0LL, ua * p.avg - p.i0), QHI = min(p.nseg, (ub + 1) * p.avg - p.i0);

    const int half = (p.flags & kScopeCentered) ? N / 2 : 0;    /* bin b stands at position b ^ half */
    const float2 *tw2 = reinterpret_cast<const float2 *>(p.twiddles), *tw3 = tw2 + (R2 - 1) * R1;
    float win[R1], acc[NACC];
#pragma unroll
    for (int r = 0; r < R1; ++r)
        win[r] = p.window[t + r * TS];
    const bool resume = live && u == 0 && p.i0 > 0 && !sl.fresh;
#pragma unroll
    for (int b = 0; b < N / RL / TS; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r)
            acc[b * RL + r] = resume ? p.old_part[(size_t)j * N + ((t + b * TS + r * (N / RL)) ^ half)] : 0.0f;

    /* the thread's samples of segment q, zeros outside the item's own segments */
    float2 raw[R1];
    auto load_seg = [&](long long q) {
        const bool in = live && q >= qlo && q < qhi;
        const long long v0 = q * p.hop + t;
#pragma unroll
        for (int r = 0; r < R1; ++r)
            raw[r] = in ? sample(j, sl, v0 + r * TS) : make_float2(0.0f, 0.0f);
    };
    if (QLO < QHI)
        load_seg(QLO);
    for (long long q = QLO; q < QHI; ++q) {
        const bool act = live && q >= qlo && q < qhi;
        float2 a[R1];
#pragma unroll
        for (int r = 0; r < R1; ++r)
            a[r] = make_float2(raw[r].x * win[r], raw[r].y * win[r]);
        fft_reg<R1>(a);
#pragma unroll
        for (int r = 0; r < R1; ++r)
            buf[scope_swz<R1>(t * R1 + r)] = a[fft_pos<R1>(r)];
        if (q + 1 < QHI)
            load_seg(q + 1);                      /* in flight while this segment is transformed */
        __syncthreads();
        float2 v[N / R2 / TS][R2];
        scope_bfly<N, TS, R2, R1, R1>(buf, tw2, t, v);
        if constexpr (R3 > 1) {
            __syncthreads();                      /* everybody has read */
            scope_put<N, TS, R2, R1>(buf, t, v);
            __syncthreads();
            float2 y[N / RL / TS][RL];
            scope_bfly<N, TS, RL, R1 * R2, 0>(buf, tw3, t, y);
            scope_add<N, TS, RL>(y, act, acc);
        } else {
            scope_add<N, TS, R2>(v, act, acc);
        }
        __syncthreads();                          /* the next segment's first pass writes where this one read */
    }

    /* the line in place order through LDS, then 16 B per lane: complete lines to the caller, the unit the batch ends in
     * to the carried partial line; an off slot's are zeros */
    float *fb = reinterpret_cast<float *>(buf);
#pragma unroll
    for (int b = 0; b < N / RL / TS; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r)
            fb[(t + b * TS + r * (N / RL)) ^ half] = acc[b * RL + r];
    __syncthreads();
    if (!valid)
        return;
    float *dst = u < p.nlines ? p.lines + ((size_t)j * p.line_stride + u) * N : p.new_part + (size_t)j * N;
    for (int i = t; i < N / 4; i += TS)
        reinterpret_cast<f32x4 *>(dst)[i] = reinterpret_cast<const f32x4 *>(fb)[i];
}

/* ------------------------------------------------------------------------ */
int scope_items_per_block(int nfft) { return nfft == 256 ? FramePlan<256>::G : 1; }

uint64_t scope_blocks(int nfft, int nslots, int nunits)
{
    const uint64_t g = (uint64_t)scope_items_per_block(nfft);
    const uint64_t blocks = ((uint64_t)nslots * (uint64_t)nunits + g - 1) / g + (uint64_t)nslots;
    return blocks <= 0x7fffffffull ? blocks : 0;
}

template <int N> static hipError_t launch_scope_t(const ScopeArgs &a, hipStream_t s)
{
    constexpr int NT = N / FramePlan<N>::R1 * FramePlan<N>::G;
    const uint64_t blocks = scope_blocks(N, a.nslots, a.nunits);
    if (!blocks)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scope<N>, dim3((unsigned)blocks), dim3(NT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scope(int nfft, const ScopeArgs &a, hipStream_t s)
{
    switch (nfft) {
    case 256: return launch_scope_t<256>(a, s);
    case 512: return launch_scope_t<512>(a, s);
    case 1024: return launch_scope_t<1024>(a, s);
    case 2048: return launch_scope_t<2048>(a, s);
    case 4096: return launch_scope_t<4096>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace pddc
