/*
 * ddc_carrier.hip -- the carrier stage: per receiver a phase-locked loop on the carrier of its complex series, the
 * series rotated by the loop's phasor, and by the receiver's mode both sidebands or one of them through a Hilbert
 * filter (gfx950 only).
 *
 *   k_carrier   per receiver j and output m: w = z times the phasor of the exact 32-bit word theta (nco_lo),
 *               e = atan2f(w.im, w.re) / pi, v = clamp(fmaf(ki, e, v)), theta += rint(fmaf(kp, e, v) 2^31),
 *               q = fmaf(gamma, |e| - q, q); u = w (DSB), or u.re = w[m-D].re -+ sum h[k] w[m-k].im, u.im = w[m-D].im
 *               (USB / LSB), or u = z with the loop at rest (OFF).  DESIGN.md 8 has the definition.
 *
 * The recursion is nonlinear: nothing of it can be scanned, it is serial in m.  What is parallel is the receivers.
 * Walk: a block takes G = 16 consecutive receivers, one per lane of its recursion wave (wave 0), and walks the whole
 * batch tile by tile, TT = 128 outputs a time.
 *   1. load: thread i takes column i mod TT of the tile for 8 of the receivers (consecutive lanes, consecutive m:
 *      coalesced 8-byte loads), held in registers since the tile before; re and im go to the planar rows sre[g], sim[g]
 *      in LDS.  The NEXT tile's loads are issued here and stay in registers over steps 2 and 3.
 *   2. lane g of wave 0 walks receiver g's row: four z per ds_read_b128 of each plane, the next four read ahead of the
 *      chain, w written back in place (ds_write_b128).  On the chain are nco_lo, the rotation, atan2f, two fmaf, the
 *      clamp, one multiply, the conversion and the integer add; q is a chain of its own beside it.  OFF lanes skip the
 *      walk: their row keeps z.
 *   3. all threads form u: a thread takes four consecutive columns of one receiver (two receivers, one after the
 *      other).  For USB / LSB the L taps run in ascending k for each of the four outputs over a window of w.im that
 *      slides down the row four columns a time, one ds_read_b128 per 16 fmaf; the taps come through the scalar cache,
 *      four per load; the next group's taps and window are asked for ahead of a group's fmaf.
 *      The FIR, the delayed w and the stores are off the serial chain.
 * LDS: a row is a ring of 3 TT = 384 columns: the tile in one third, the two tiles before it -- 2 TT = 256 >= L - 1
 * columns of history -- in the other two; the next tile goes where the oldest third was, so nothing is ever moved.  At
 * the start of a batch the carried L - 1 values of w (or zeros) are put in front of column 0, that is at the ring's end.
 * Banks: the recursion lanes read and write 16 bytes each at the same column of G = 16 different rows.  A wave's
 * ds_read_b128 is served in groups of 16 lanes over 64 banks of 4 bytes, bank = dword address mod 64; lanes 0 .. 15 fall
 * into two of the groups (0-3 with 12-15, and 4-11).  The row stride is 384 + 4 = 388 dwords = 4 mod 64: lane g starts
 * at bank 4 g + const mod 64, so the 16 lanes cover the 64 banks once and no group sees a conflict (a stride of 384 = 0
 * mod 64 would put all 16 on the same four banks: 8-way in each group).  ds_write_b128 goes in groups of 8 consecutive
 * lanes over 32 banks: 8 lanes x 4 banks at stride 4 mod 32, again each bank once.  Step 3's ds_read_b128 has a wave's
 * lanes 0 .. 31 on consecutive quads of one row (16 lanes x 4 dwords = 64 banks per group) and lanes 32 .. 63 on
 * another row in groups of their own; the ring's wrap moves an address by 384 = 0 mod 64 and keeps its bank.  Steps 1
 * and 3 use 4-byte accesses at consecutive columns where they are not 16-byte ones.
 * Bits: every value is made by one thread with the definition's operation sequence (contraction is off in this file;
 * nco_lo spells its own fmaf), each FIR sum by one thread in ascending k from 0, so nothing depends on the batch cut,
 * K, j's index, the other receivers or the tile.  No atomics, no scratch.
 * In place (u == z, equal strides): a tile's z is in registers or LDS before any thread stores u of that tile, and the
 * next tile's loads touch columns no store of this tile reaches.
 * Bounds: z and u are indexed by receivers < nrx and outputs < n only; the carried records by receivers < nrx and
 * columns < L - 1; a row is read up to dword 384 + 3 (the read-ahead of step 2 at the ring's end), inside its pad; the
 * FIR's window reaches back 4 ceil(L / 4) <= 256 columns, inside the ring; the tap array has 256 entries.
 */
#include "ddc_carrier.h"
#include "ddc_dev.h"

#pragma clang fp contract(off)

namespace pddc {

static constexpr float kCarrierInvPi = 0.318309886183790672f;

/* one step of the loop: z -> w; theta, v, q move on */
__device__ __forceinline__ void carrier_step(float zr, float zi, float kp, float ki, float vmax, float gamma,
                                             uint32_t &theta, float &v, float &q, float &wr, float &wi)
{
    float c, s;
    nco_lo(theta, c, s);                                /* c + i s = exp(-i theta) */
    wr = zr * c - zi * s;
    wi = zr * s + zi * c;
    const float e = atan2f(wi, wr) * kCarrierInvPi;
    v = fminf(vmax, fmaxf(-vmax, fmaf(ki, e, v)));
    const float step = fmaf(kp, e, v);                  /* |step| < 1: kp <= 0.5, vmax < 0.5 */
    theta += (uint32_t)__float2int_rn(step * 2147483648.0f);
    q = fmaf(gamma, fabsf(e) - q, q);
}

/* the last nj taps h.x, h.y, h.z (nj uniform, 1 or 3) on four consecutive outputs: `a` holds w.im of the outputs' own
 * columns less the taps before, `b` the four columns below; per output the taps in ascending k */
__device__ __forceinline__ void carrier_fir3(const f32x4 h, int nj, const float4 a, const float4 b, float &s0, float &s1,
                                             float &s2, float &s3)
{
    s0 = fmaf(h.x, a.x, s0);
    s1 = fmaf(h.x, a.y, s1);
    s2 = fmaf(h.x, a.z, s2);
    s3 = fmaf(h.x, a.w, s3);
    if (nj > 1) {
        s0 = fmaf(h.y, b.w, s0);
        s1 = fmaf(h.y, a.x, s1);
        s2 = fmaf(h.y, a.y, s2);
        s3 = fmaf(h.y, a.z, s3);
        s0 = fmaf(h.z, b.z, s0);
        s1 = fmaf(h.z, b.w, s1);
        s2 = fmaf(h.z, a.x, s2);
        s3 = fmaf(h.z, a.y, s3);
    }
}

__global__ __launch_bounds__(kCarrierThreads) void k_carrier(CarrierArgs a)
{
    constexpr int G = kCarrierGroup, TT = kCarrierTile, RING = kCarrierRing, LD = kCarrierRing + kCarrierPad;
    constexpr int RA = G * TT / kCarrierThreads;        /* receivers per thread in step 1 */
    constexpr int RQ = G * (TT / 4) / kCarrierThreads;  /* receivers per thread in step 3 */
    static_assert(kCarrierThreads == 2 * TT && RA * kCarrierThreads == G * TT && RQ * kCarrierThreads == G * (TT / 4),
                  "the threads tile the block's receivers and a tile's columns");
    static_assert(RING - TT >= kCarrierMaxTaps + 1 && RING - TT == kCarrierThreads, "two tiles of history, one thread per column");
    static_assert(LD % 64 == 4 && G <= 16, "the recursion lanes start 4 banks apart");
    __shared__ __attribute__((aligned(16))) float sre[G][LD];
    __shared__ __attribute__((aligned(16))) float sim[G][LD];
    const int tid = (int)threadIdx.x;
    const int g0 = (int)blockIdx.x * G;
    const int ng = a.nrx - g0 < G ? a.nrx - g0 : G;
    const int L = a.L, H = L - 1, D = H >> 1;
    const CarrierRx PDDC_CONSTANT *rx = (const CarrierRx PDDC_CONSTANT *)a.rx + g0;
    const float PDDC_CONSTANT *taps = (const float PDDC_CONSTANT *)a.taps;

    /* the carried w (or zeros) in front of column 0: the ring's last 2 TT columns, one per thread */
    {
        const int h = tid - (RING - TT - H);
        for (int g = 0; g < ng; ++g) {
            float2 w = make_float2(0.0f, 0.0f);
            if (h >= 0 && !(rx[g].flags & kCarrierFresh))
                w = a.old_hist[(long long)(g0 + g) * H + h];
            sre[g][TT + tid] = w.x;
            sim[g][TT + tid] = w.y;
        }
    }

    /* the recursion lanes: lane g of wave 0 owns receiver g0 + g */
    const bool mine = tid < ng;
    uint32_t mode = kCarrierOff, theta = 0u;
    float kp = 0.0f, ki = 0.0f, v = 0.0f, q = 0.0f;
    if (mine) {
        const CarrierRx r = a.rx[g0 + tid];
        mode = r.mode;
        kp = r.kp;
        ki = r.ki;
        if (!(r.flags & kCarrierFresh)) {
            const CarrierState s = a.old[g0 + tid];
            theta = s.theta;
            v = s.v;
            q = s.q;
        }
    }

    const int ci = tid & (TT - 1);                      /* step 1: this thread's column, its first receiver */
    const int ra = (tid / TT) * RA;
    float2 zc[RA];
    for (int r = 0; r < RA; ++r) {
        zc[r] = make_float2(0.0f, 0.0f);
        if (ra + r < ng && ci < a.n)
            zc[r] = a.z[(long long)(g0 + ra + r) * a.z_stride + ci];
    }

    int base = 0, cnt = 0;
    for (long long o = 0; o < a.n; o += TT) {
        base = (int)(o % RING);
        cnt = (int)(a.n - o < TT ? a.n - o : TT);
        /* 1. this tile into its third of the ring; the next tile's loads */
        if (ci < cnt)
            for (int r = 0; r < RA; ++r)
                if (ra + r < ng) {
                    sre[ra + r][base + ci] = zc[r].x;
                    sim[ra + r][base + ci] = zc[r].y;
                }
        const long long mn = o + TT + ci;
        if (mn < a.n)
            for (int r = 0; r < RA; ++r)
                if (ra + r < ng)
                    zc[r] = a.z[(long long)(g0 + ra + r) * a.z_stride + mn];
        __syncthreads();

        /* 2. the loops */
        if (mine && mode != kCarrierOff) {
            float *pr = sre[tid] + base, *pi = sim[tid] + base;
            int k = 0;
            float4 cr = *reinterpret_cast<const float4 *>(pr), cm = *reinterpret_cast<const float4 *>(pi);
            for (; k + 4 <= cnt; k += 4) {
                const float4 nr = *reinterpret_cast<const float4 *>(pr + k + 4);     /* <= RING: the row's pad */
                const float4 nm = *reinterpret_cast<const float4 *>(pi + k + 4);
                float4 wr, wi;
                carrier_step(cr.x, cm.x, kp, ki, a.vmax, a.gamma, theta, v, q, wr.x, wi.x);
                carrier_step(cr.y, cm.y, kp, ki, a.vmax, a.gamma, theta, v, q, wr.y, wi.y);
                carrier_step(cr.z, cm.z, kp, ki, a.vmax, a.gamma, theta, v, q, wr.z, wi.z);
                carrier_step(cr.w, cm.w, kp, ki, a.vmax, a.gamma, theta, v, q, wr.w, wi.w);
                *reinterpret_cast<float4 *>(pr + k) = wr;
                *reinterpret_cast<float4 *>(pi + k) = wi;
                cr = nr;
                cm = nm;
            }
            for (; k < cnt; ++k) {
                float wr, wi;
                carrier_step(pr[k], pi[k], kp, ki, a.vmax, a.gamma, theta, v, q, wr, wi);
                pr[k] = wr;
                pi[k] = wi;
            }
        }
        __syncthreads();

        /* 3. u of four consecutive columns of one receiver, RQ receivers one after the other */
        const int cq = (tid & (TT / 4 - 1)) * 4;
        if (cq < cnt)
            for (int r = 0; r < RQ; ++r) {
                const int g = tid / (TT / 4) + r * (G / RQ);
                if (g >= ng)
                    break;
                const uint32_t md = rx[g].mode;
                const float *qr = sre[g], *qi = sim[g];
                float4 ur = *reinterpret_cast<const float4 *>(qr + base + cq);
                float4 um = *reinterpret_cast<const float4 *>(qi + base + cq);
                if (md == kCarrierUsb || md == kCarrierLsb) {
                    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                    /* groups of four taps: the next group's taps (one scalar 16-byte load) and window (one
                     * ds_read_b128) are asked for ahead of this group's 16 fmaf */
                    const f32x4 PDDC_CONSTANT *t4 = (const f32x4 PDDC_CONSTANT *)taps;
                    const int full = L >> 2;
                    float4 top = um;
                    int col = base + cq;
                    col = col >= 4 ? col - 4 : col - 4 + RING;
                    float4 low = *reinterpret_cast<const float4 *>(qi + col);
                    f32x4 hn = t4[0];
#pragma unroll 2
                    for (int i = 0; i < full; ++i) {
                        const f32x4 h = hn;
                        const float4 cur = low;
                        hn = t4[i + 1];                 /* <= group 63: inside the 256 slots */
                        col = col >= 4 ? col - 4 : col - 4 + RING;
                        low = *reinterpret_cast<const float4 *>(qi + col);
                        s0 = fmaf(h.x, top.x, s0);
                        s1 = fmaf(h.x, top.y, s1);
                        s2 = fmaf(h.x, top.z, s2);
                        s3 = fmaf(h.x, top.w, s3);
                        s0 = fmaf(h.y, cur.w, s0);
                        s1 = fmaf(h.y, top.x, s1);
                        s2 = fmaf(h.y, top.y, s2);
                        s3 = fmaf(h.y, top.z, s3);
                        s0 = fmaf(h.z, cur.z, s0);
                        s1 = fmaf(h.z, cur.w, s1);
                        s2 = fmaf(h.z, top.x, s2);
                        s3 = fmaf(h.z, top.y, s3);
                        s0 = fmaf(h.w, cur.y, s0);
                        s1 = fmaf(h.w, cur.z, s1);
                        s2 = fmaf(h.w, cur.w, s2);
                        s3 = fmaf(h.w, top.x, s3);
                        top = cur;
                    }
                    /* L is odd: one or three taps are left */
                    carrier_fir3(hn, L & 3, top, low, s0, s1, s2, s3);
                    /* w of D outputs before */
                    int cd = base + cq - D;
                    cd = cd < 0 ? cd + RING : cd;
                    float dr[4], dm[4];
                    for (int c = 0; c < 4; ++c) {
                        const int at = cd + c >= RING ? cd + c - RING : cd + c;
                        dr[c] = qr[at];
                        dm[c] = qi[at];
                    }
                    if (md == kCarrierUsb)
                        ur = make_float4(dr[0] - s0, dr[1] - s1, dr[2] - s2, dr[3] - s3);
                    else
                        ur = make_float4(dr[0] + s0, dr[1] + s1, dr[2] + s2, dr[3] + s3);
                    um = make_float4(dm[0], dm[1], dm[2], dm[3]);
                }
                float2 *up = a.u + (long long)(g0 + g) * a.u_stride + o + cq;
                up[0] = make_float2(ur.x, um.x);
                if (cq + 1 < cnt)
                    up[1] = make_float2(ur.y, um.y);
                if (cq + 2 < cnt)
                    up[2] = make_float2(ur.z, um.z);
                if (cq + 3 < cnt)
                    up[3] = make_float2(ur.w, um.w);
            }
        /* the next tile's step 1 writes the third that this step 3 has read as history */
        __syncthreads();
    }

    /* what is carried: the loops' values, and the last L - 1 columns of w behind the batch's end */
    if (mine) {
        CarrierState s;
        s.theta = theta;
        s.v = v;
        s.q = q;
        s.pad = 0u;
        a.new_state[g0 + tid] = s;
    }
    if (tid < H) {
        int col = base + cnt - H + tid;
        col = col < 0 ? col + RING : col;
        for (int g = 0; g < ng; ++g)
            a.new_hist[(long long)(g0 + g) * H + tid] = make_float2(sre[g][col], sim[g][col]);
    }
}

hipError_t launch_carrier(const CarrierArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kCarrierMaxRx || a.z_stride < a.n || a.u_stride < a.n || !a.z || !a.u || !a.rx ||
        !a.old || !a.new_state || !a.old_hist || !a.new_hist || !a.taps || a.L < 3 || a.L > kCarrierMaxTaps || !(a.L & 1))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nrx + kCarrierGroup - 1) / kCarrierGroup));
    hipLaunchKernelGGL(k_carrier, grid, dim3(kCarrierThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
