/*
 * ddc_denoise.cpp -- host side of the spectral noise reduction (include/perseus_ddc.h, pddc_denoise_*): the object, its
 * receiver table, the sample counter, the frame arithmetic of a batch and its one launch, and the read of the noise
 * estimate.  The kernel is in ddc_denoise.hip.
 * What is carried per receiver lives on the device in pairs of buffers, read and written in turn: the inputs since the
 * start of the oldest incomplete frame and the finished values not yet given out turn with every accepted batch, the
 * ring of partial overlap sums and S, N, A with every batch that completes a frame.  Nothing on the device is cleared
 * from the host: at create and reset no sample is carried (`fresh`: the next launch reads nothing carried) and every
 * receiver's table entry holds the first-frame mark, which is also what set_rx(PDDC_DENOISE_RESTART) leaves; the marks go
 * once a launch that completed a frame was accepted.
 */
#include "ddc_stage.h"
#include "ddc_denoise.h"

#include <cstring>

using namespace pddc;

struct pddc_denoise : StageBase {
    PDDC_LOCAL ~pddc_denoise() = default;
    pddc_denoise_params par{};
    FrameTables tables;
    RxTable<DenoiseRx> table;                       /* flags: kDenoiseHold, and kDenoiseRestart as the first-frame mark */
    Carried<float> carry;                           /* [nrx][nfft]                                                 */
    Carried<float> pend;                            /* [nrx][hop]                                                  */
    Carried<float> ola;                             /* [nrx][nfft]                                                 */
    Carried<float> sna;                             /* [3][nrx][nfft/2 + 1]                                        */
    uint64_t N = 0;                                 /* samples per row since create / reset                        */
    bool tracked = false;                           /* a frame was completed since create / reset: sna.old() holds N */
};

static_assert(PDDC_DENOISE_OFF == kDenoiseOff && PDDC_DENOISE_NR == kDenoiseNr, "the kernel's modes are the header's");
static_assert(PDDC_DENOISE_RESTART == kDenoiseRestart && PDDC_DENOISE_HOLD == kDenoiseHold, "the kernel's flag bits are the header's");

static bool denoise_sizes_ok(int nfft, int hop)
{
    return (nfft == 256 || nfft == 512 || nfft == 1024) && (hop == nfft / 2 || hop == nfft / 4);
}

/* written so that a NaN fails it */
static bool unit_open(float v) { return v > 0.0f && v <= 1.0f; }

static bool denoise_rx_ok(uint32_t mode, float beta, float gmin, float alpha, uint32_t flags)
{
    return mode < kDenoiseModes && !(flags & ~(kDenoiseRestart | kDenoiseHold)) && beta > 0.0f && beta <= 3.4028234e38f &&
           gmin >= 0.0f && gmin <= 1.0f && alpha >= 0.0f && alpha < 1.0f;
}

extern "C" {

int pddc_denoise_delay(int nfft) { return denoise_sizes_ok(nfft, nfft / 2) ? nfft : 0; }

int pddc_denoise_tile_frames(void) { return kDenoiseTileFrames; }

int pddc_denoise_create(pddc_denoise **out, int device, int nrx, const pddc_denoise_params *par, const float *window,
                        const pddc_denoise_rx *rx)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kDenoiseMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "denoise: %d receivers (1 .. %d) and their modes", nrx, kDenoiseMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "denoise: null parameters");
    if (!denoise_sizes_ok(par->nfft, par->hop))
        return pddc_set_error_(PDDC_EINVAL, "denoise: nfft %d (256, 512 or 1024), hop %d (nfft/2 or nfft/4)", par->nfft, par->hop);
    if (!unit_open(par->smooth) || !unit_open(par->up) || !unit_open(par->down) || !(par->nmin >= 0.0f && par->nmin <= 1.0f))
        return pddc_set_error_(PDDC_EINVAL, "denoise: smooth %g, up %g, down %g (each 0 < . <= 1), nmin %g (0 .. 1)", (double)par->smooth,
                               (double)par->up, (double)par->down, (double)par->nmin);
    if (!(par->eps > 0.0f && par->eps <= 3.4028234e38f))
        return pddc_set_error_(PDDC_EINVAL, "denoise: eps %g (finite, > 0)", (double)par->eps);
    if (!window)
        return pddc_set_error_(PDDC_EINVAL, "denoise: null window");
    if (const int i = FrameTables::bad_window(window, par->nfft); i >= 0)
        return pddc_set_error_(PDDC_EINVAL, "denoise: window[%d] is not finite", i);
    for (int j = 0; j < nrx; ++j)
        if (!denoise_rx_ok(rx[j].mode, rx[j].beta, rx[j].gmin, rx[j].alpha, rx[j].flags))
            return pddc_set_error_(PDDC_EINVAL, "denoise: receiver %d: mode %u, beta %g (finite, > 0), gmin %g (0 .. 1), alpha %g (0 <= alpha < 1), flags 0x%x",
                                   j, rx[j].mode, (double)rx[j].beta, (double)rx[j].gmin, (double)rx[j].alpha, rx[j].flags);
    return stage_create(out, device, nrx, [&](pddc_denoise &s) {
        s.par = *par;
        const size_t nfft = (size_t)par->nfft;
        /* every receiver's next completed frame is a first frame */
        for (int j = 0; j < nrx; ++j)
            s.table.host.push_back(DenoiseRx{ rx[j].mode, rx[j].beta, rx[j].gmin, rx[j].alpha, rx[j].flags | kDenoiseRestart });
        PDDC_TRY(s.tables.alloc(par->nfft, window));
        PDDC_TRY(s.table.alloc());
        PDDC_TRY(s.carry.alloc((size_t)nrx * nfft));
        PDDC_TRY(s.pend.alloc((size_t)nrx * (size_t)par->hop));
        PDDC_TRY(s.ola.alloc((size_t)nrx * nfft));
        return s.sna.alloc((size_t)nrx * 3 * (nfft / 2 + 1));
    });
}

int pddc_denoise_destroy(pddc_denoise *s) { return stage_destroy(s); }

int pddc_denoise_reset(pddc_denoise *s)
{
    PDDC_TRY(stage_quiesce(s));
    s->N = 0;
    s->tracked = false;
    for (DenoiseRx &r : s->table.host)
        r.flags |= kDenoiseRestart;
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_denoise_set_rx(pddc_denoise *s, int rx, uint32_t mode, float beta, float gmin, float alpha, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(s, "denoise", rx));
    if (!denoise_rx_ok(mode, beta, gmin, alpha, flags))
        return pddc_set_error_(PDDC_EINVAL, "denoise: mode %u, beta %g (finite, > 0), gmin %g (0 .. 1), alpha %g (0 <= alpha < 1), flags 0x%x",
                               mode, (double)beta, (double)gmin, (double)alpha, flags);
    DenoiseRx &r = s->table.host[(size_t)rx];
    /* a first frame asked for earlier and not yet met stays asked for; HOLD lasts until a call without it */
    r = DenoiseRx{ mode, beta, gmin, alpha, flags | (r.flags & kDenoiseRestart) };
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_denoise_process(pddc_denoise *s, const void *d_x, size_t n, size_t x_stride, void *d_out, size_t out_stride, void *stream)
{
    if (!s)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_x, 4, "d_x"));
        PDDC_TRY(device_ptr_ok(d_out, 4, "d_out"));
    }
    if (over_capacity(n, x_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "denoise: %zu samples per receiver, x_stride %zu, out_stride %zu", n, x_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    if (ranges_overlap(d_out, rows_extent(s->nrx, n, out_stride, 4), d_x, rows_extent(s->nrx, n, x_stride, 4)))
        return pddc_set_error_(PDDC_EINVAL, "denoise: out overlaps x (in place is not offered)");
    PDDC_TRY(set_device(s->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(s->table.upload(st));
    const uint64_t hop = (uint64_t)s->par.hop, nfft = (uint64_t)s->par.nfft;
    const uint64_t q0 = s->N / hop, q1 = (s->N + n) / hop;      /* frame q is complete once (q + 1) hop samples arrived */
    DenoiseArgs a{};
    a.x = static_cast<const float *>(d_x);
    a.x_stride = (long long)x_stride;
    a.out = static_cast<float *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = s->table.dev();
    a.nrx = s->nrx;
    a.hop = s->par.hop;
    a.smooth = s->par.smooth;
    a.up = s->par.up;
    a.down = s->par.down;
    a.nmin = s->par.nmin;
    a.eps = s->par.eps;
    a.window = s->tables.window.get();
    a.twiddles = s->tables.twiddles.get();
    a.old_carry = s->carry.old();
    a.new_carry = s->carry.next();
    a.old_ola = s->ola.old();
    a.new_ola = s->ola.next();
    a.old_pend = s->pend.old();
    a.new_pend = s->pend.next();
    a.old_sna = s->sna.old();
    a.new_sna = s->sna.next();
    a.pos = (int)(s->N - q0 * hop);
    a.clen = (int)(nfft - hop) + a.pos;                         /* frame q0 begins at (q0 + 1) hop - nfft */
    a.new_clen = (int)(nfft - hop + (s->N + n - q1 * hop));
    a.q0 = (long long)q0;
    a.nseg = (long long)(q1 - q0);
    a.fresh = s->N == 0 ? 1u : 0u;
    PDDC_HIP_TRY(launch_denoise(s->par.nfft, a, st));
    /* the launch was accepted: only now do the host-side marks move */
    s->carry.turn();
    s->pend.turn();
    s->N += n;
    if (a.nseg) {
        s->ola.turn();
        s->sna.turn();
        s->tracked = true;
        for (DenoiseRx &r : s->table.host)
            if (r.flags & kDenoiseRestart) {
                r.flags &= ~kDenoiseRestart;
                s->table.dirty = true;
            }
    }
    return PDDC_OK;
}

int pddc_denoise_read_noise(pddc_denoise *s, float *host, void *stream)
{
    if (!s || !host)
        return null_argument();
    PDDC_TRY(set_device(s->device));
    const size_t B = (size_t)s->par.nfft / 2 + 1;
    if (!s->tracked)
        std::memset(host, 0, sizeof(float) * (size_t)s->nrx * B);
    return read_back(host, s->tracked ? s->sna.old() + (size_t)s->nrx * B : nullptr, (size_t)s->nrx * B, (hipStream_t)stream);
}

} // extern "C"
