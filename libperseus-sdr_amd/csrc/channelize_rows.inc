/*
 * channelize_rows.inc -- the body of k_channelize<M, P, Q> and k_channelize_list<M, P, Q> (ddc_channelizer.hip), included
 * once in each with PDDC_CHAN_LIST 0 / 1: the two kernels are the same text up to the last pass's store, and the range
 * form compiles to the code it had before the list form existed (a shared device function moved its registers).
 * In scope: the template parameters M, P, Q and the kernel's argument `ChannelizeArgs a`.
 */
    using Plan = SpecPlan<M>;
    constexpr int NT = M / 16 < 256 ? M / 16 : 256;
    constexpr int NG = M / 8 / NT;               /* 48-byte groups of a row's u a thread folds */
    constexpr int NGU = NG / Q;                  /* ... of one unit                            */
    constexpr int GU = NT * NGU;                 /* groups of a unit                           */
    constexpr int D = M / Q;
    constexpr int PQ = P * Q, NSL = PQ - 1;      /* units of a row, ring slots                 */
    constexpr int R2 = Plan::R2;
    constexpr int TW1 = 0, TW2 = 15 * 16, TWN = TW2 + (R2 - 1) * 256;
    static_assert(NG == 2 && NGU >= 1 && Plan::R3 == 1, "k_channelize: M in 1024, 2048, 4096");
    extern __shared__ __attribute__((aligned(16))) float2 chan_lds[];
    float2 *buf = chan_lds;                      /* [M] */
    float2 *tw = chan_lds + M;                   /* [TWN] */
    u32x4 *ring = reinterpret_cast<u32x4 *>(chan_lds + M + TWN);   /* [NSL][3][GU] */
#if PDDC_CHAN_LIST
    short *col_of = reinterpret_cast<short *>(ring + NSL * 3 * GU);   /* [M]: the column of a bin, -1: not listed */
#endif
    const int tid = threadIdx.x;

    const long long row0 = (long long)blockIdx.x * a.run;
    if (row0 >= a.nrows)
        return;
    const int nr = (int)(a.nrows - row0 < a.run ? a.nrows - row0 : a.run);

    for (int i = tid; i < TWN; i += NT)
        tw[i] = reinterpret_cast<const float2 *>(a.twiddles)[i];
#if PDDC_CHAN_LIST
    for (int i = tid; i < M / 2; i += NT)        /* two entries a time; in place with the twiddles, at the barrier below */
        reinterpret_cast<unsigned *>(col_of)[i] = reinterpret_cast<const unsigned *>(a.slot)[i];
#endif
    float win[P][NG][8];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const f32x4 *w = reinterpret_cast<const f32x4 *>(a.proto + p * M + 8 * (tid + u * NT));
            const f32x4 x = w[0], y = w[1];
            win[p][u][0] = x.x; win[p][u][1] = x.y; win[p][u][2] = x.z; win[p][u][3] = x.w;
            win[p][u][4] = y.x; win[p][u][5] = y.y; win[p][u][6] = y.z; win[p][u][7] = y.w;
        }

    u32x4 raw[NGU][3];
    auto load_unit = [&](long long t) {          /* unit t of the run: samples (row0 + t) D .. + D */
        const long long v0 = (row0 + t) * D;
#pragma unroll
        for (int uu = 0; uu < NGU; ++uu)
            a.in.load_group(v0 + 8LL * (tid + uu * NT), raw[uu]);
    };
    auto ring_put = [&](int slot) {
#pragma unroll
        for (int uu = 0; uu < NGU; ++uu)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                ring[(slot * 3 + c) * GU + tid + uu * NT] = raw[uu][c];
    };

    /* the porch: units 0 .. NSL-1 of the run, unit t in slot t */
    for (int t = 0; t < NSL; ++t) {
        load_unit(t);
        ring_put(t);
    }
    load_unit(NSL);
    __syncthreads();                             /* the twiddles are in place */

    int base = 0;                                /* the slot of the row's oldest unit: row mod NSL */
    for (int sl = 0; sl < nr; ++sl) {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int q = u / NGU, uu = u % NGU;
            const int g = tid + u * NT;
            float2 acc[8];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int j = p * Q + q;         /* the unit of the row */
                u32x4 x[3];
                if (j == NSL) {
                    x[0] = raw[uu][0]; x[1] = raw[uu][1]; x[2] = raw[uu][2];
                } else {
                    const int slot = base + j >= NSL ? base + j - NSL : base + j;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        x[c] = ring[(slot * 3 + c) * GU + tid + uu * NT];
                }
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    PDDC_UNPACK_GROUP_MSB(x, h, i0, q0, i1, q1);
                    const float fi0 = (float)i0 * kPackedUnpackScale, fq0 = (float)q0 * kPackedUnpackScale;
                    const float fi1 = (float)i1 * kPackedUnpackScale, fq1 = (float)q1 * kPackedUnpackScale;
                    const float w0 = win[p][u][2 * h], w1 = win[p][u][2 * h + 1];
                    if (p == 0) {
                        acc[2 * h] = make_float2(fi0 * w0, fq0 * w0);
                        acc[2 * h + 1] = make_float2(fi1 * w1, fq1 * w1);
                    } else {
                        acc[2 * h].x = fmaf(fi0, w0, acc[2 * h].x);
                        acc[2 * h].y = fmaf(fq0, w0, acc[2 * h].y);
                        acc[2 * h + 1].x = fmaf(fi1, w1, acc[2 * h + 1].x);
                        acc[2 * h + 1].y = fmaf(fq1, w1, acc[2 * h + 1].y);
                    }
                }
            }
            f32x4 *dst = reinterpret_cast<f32x4 *>(buf);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                f32x4 o;
                o.x = acc[2 * h].x; o.y = acc[2 * h].y; o.z = acc[2 * h + 1].x; o.w = acc[2 * h + 1].y;
                dst[4 * g + (h ^ ((g >> 1) & 3))] = o;
            }
        }
        /* the newest unit takes the oldest one's slot (this thread's own groups: program order is enough) */
        if (NSL > 0) {
            ring_put(base);
            base = base + 1 == NSL ? 0 : base + 1;
        }
        if (sl + 1 < nr)
            load_unit((long long)sl + 1 + NSL);
        __syncthreads();
        spec_pass_mid<M, NT, 16, 1, kImgLoaders, 16>(buf, tw + TW1);
        spec_pass_mid<M, NT, 16, 16, 16, 0>(buf, tw + TW1);
        const bool neg_odd = Q == 2 && ((a.row_parity + (unsigned)(row0 + sl)) & 1u);
        f32x2 *orow = reinterpret_cast<f32x2 *>(a.out) + (size_t)(row0 + sl) * (size_t)a.count;
        spec_pass_out<M, NT, R2, 256, 0>(buf, tw + TW2, [&](int bin, float2 v) {
#if PDDC_CHAN_LIST
            const int i = col_of[bin];
#else
            const int i = (bin - a.first) & (M - 1);
#endif
            if (neg_odd && (bin & 1))
                v = make_float2(-v.x, -v.y);
#if PDDC_CHAN_LIST
            if (i >= 0) {
#else
            if (i < a.count) {
#endif
                f32x2 o;
                o.x = v.x; o.y = v.y;
                __builtin_nontemporal_store(o, orow + i);
            }
        });
    }
