/*
 * ddc_eq.cpp -- host side of the equaliser (include/perseus_ddc.h, pddc_eq_*): the object, its receiver table, the
 * launch of a batch, the read of the states and the section designs.  The kernel is in ddc_eq.hip, the design formulas
 * and the stability test in ddc_eq_design.h.
 * What is carried per receiver (two binary64 states per section) lives on the device in two records, read and written in
 * turn; nothing on the device is cleared from the host: create and reset set `fresh` (the next launch does not read the
 * record, its values are 0), set_rx(PDDC_EQ_RESTART) leaves a mark in the receiver's table entry (the next launch takes
 * that receiver's states as 0), which goes once a launch was accepted.  The sections live in the table, which is
 * uploaded in stream order when it changed.
 */
#include "ddc_stage.h"
#include "ddc_eq.h"
#include "ddc_eq_design.h"

#include <cstring>

using namespace pddc;

struct pddc_eq : StageBase {
    PDDC_LOCAL ~pddc_eq() = default;
    int S = 0;                                      /* sections per receiver at most                               */
    RxTable<EqRx> table;                            /* flags carry kEqRestart                                      */
    bool fresh = true;                              /* no launch since create / reset                              */
    Carried<double> state;                          /* [nrx][S][2]                                                 */
};

static_assert(PDDC_EQ_MAX_SECTIONS == kEqMaxSections && PDDC_EQ_RESTART == kEqRestart, "the kernel's constants are the header's");
static_assert(sizeof(pddc_eq_section) == sizeof(EqSection) && sizeof(EqSection) == 5 * sizeof(double),
              "a section is five doubles: b0, b1, b2, a1, a2");
static_assert(PDDC_EQ_LOWPASS == kEqLowpass && PDDC_EQ_HIGHPASS == kEqHighpass && PDDC_EQ_BANDPASS == kEqBandpass &&
              PDDC_EQ_NOTCH == kEqNotch && PDDC_EQ_PEAK == kEqPeak && PDDC_EQ_LOWSHELF == kEqLowshelf &&
              PDDC_EQ_HIGHSHELF == kEqHighshelf && PDDC_EQ_LOWPASS1 == kEqLowpass1 && PDDC_EQ_HIGHPASS1 == kEqHighpass1,
              "the design's kinds are the header's");

static bool eq_sections_ok(int S) { return S == 1 || S == 2 || S == 4 || S == 8; }

static EqSection eq_section_of(const pddc_eq_section &c) { return EqSection{ c.b0, c.b1, c.b2, c.a1, c.a2 }; }

/* the first of `nsec` sections that fails the stability test, or -1 */
static int eq_bad_section(const pddc_eq_section *sec, int nsec)
{
    for (int s = 0; s < nsec; ++s)
        if (!eq_section_ok(eq_section_of(sec[s])))
            return s;
    return -1;
}

static int eq_refuse_section(int rx, int s, const pddc_eq_section &c)
{
    return pddc_set_error_(PDDC_EINVAL, "eq: receiver %d, section %d: b %g %g %g, a %g %g (all finite, |a2| < 1, |a1| < 1 + a2)",
                           rx, s, c.b0, c.b1, c.b2, c.a1, c.a2);
}

static void eq_fill(EqRx &r, int nsec, const pddc_eq_section *sec, uint32_t flags)
{
    r = EqRx{};
    r.nsec = (uint32_t)nsec;
    r.flags = flags;
    for (int s = 0; s < nsec; ++s) {
        const double c[5] = { sec[s].b0, sec[s].b1, sec[s].b2, sec[s].a1, sec[s].a2 };
        std::memcpy(r.c[s], c, sizeof(c));
    }
}

extern "C" {

int pddc_eq_tile_outputs(void) { return kEqTile; }

int pddc_eq_design(int kind, double rate_hz, double f_hz, double q, double gain_db, pddc_eq_section *out)
{
    if (!out)
        return null_argument();
    EqSection c;
    if (!eq_design(kind, rate_hz, f_hz, q, gain_db, &c))
        return pddc_set_error_(PDDC_EINVAL, "eq: design %d at %g Hz of %g Hz, q %g, %g dB (a kind 0 .. %d, 0 < f < rate / 2, q > 0, "
                               "all finite, and a section double holds)", kind, f_hz, rate_hz, q, gain_db, kEqKinds - 1);
    *out = pddc_eq_section{ c.b0, c.b1, c.b2, c.a1, c.a2 };
    return PDDC_OK;
}

int pddc_eq_create(pddc_eq **out, int device, int nrx, const pddc_eq_params *par, const int *nsec, const pddc_eq_section *sec)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kEqMaxRx || !nsec || !sec)
        return pddc_set_error_(PDDC_EINVAL, "eq: %d receivers (1 .. %d), their section counts and sections", nrx, kEqMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "eq: null parameters");
    const int S = par->sections;
    if (!eq_sections_ok(S))
        return pddc_set_error_(PDDC_EINVAL, "eq: %d sections (1, 2, 4, 8)", S);
    for (int j = 0; j < nrx; ++j) {
        if (nsec[j] < 0 || nsec[j] > S)
            return pddc_set_error_(PDDC_EINVAL, "eq: receiver %d: %d sections (0 .. %d)", j, nsec[j], S);
        const int bad = eq_bad_section(sec + (size_t)j * (size_t)S, nsec[j]);
        if (bad >= 0)
            return eq_refuse_section(j, bad, sec[(size_t)j * (size_t)S + (size_t)bad]);
    }
    return stage_create(out, device, nrx, [&](pddc_eq &s) {
        s.S = S;
        s.table.host.resize((size_t)nrx);
        for (int j = 0; j < nrx; ++j)
            eq_fill(s.table.host[(size_t)j], nsec[j], sec + (size_t)j * (size_t)S, 0u);
        PDDC_TRY(s.table.alloc());
        return s.state.alloc((size_t)nrx * (size_t)S * 2);
    });
}

int pddc_eq_destroy(pddc_eq *s) { return stage_destroy(s); }

int pddc_eq_reset(pddc_eq *s)
{
    PDDC_TRY(stage_quiesce(s));
    s->fresh = true;
    for (EqRx &r : s->table.host)
        r.flags &= ~kEqRestart;
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_eq_set_rx(pddc_eq *s, int rx, int nsec, const pddc_eq_section *sec, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(s, "eq", rx));
    if (nsec < 0 || nsec > s->S || (nsec && !sec) || (flags & ~kEqRestart))
        return pddc_set_error_(PDDC_EINVAL, "eq: %d sections (0 .. %d) and their values, flags 0x%x", nsec, s->S, flags);
    const int bad = eq_bad_section(sec, nsec);
    if (bad >= 0)
        return eq_refuse_section(rx, bad, sec[bad]);
    EqRx &r = s->table.host[(size_t)rx];
    /* a restart asked for earlier and not yet honoured stays asked for */
    eq_fill(r, nsec, sec, r.flags | (flags & kEqRestart));
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_eq_process(pddc_eq *s, const void *d_a, size_t n, size_t a_stride, void *d_out, size_t out_stride, void *stream)
{
    if (!s)
        return null_argument();
    if (n) {
        PDDC_TRY(device_ptr_ok(d_a, 4, "d_a"));
        PDDC_TRY(device_ptr_ok(d_out, 4, "d_out"));
    }
    if (over_capacity(n, a_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "eq: %zu samples per receiver, a_stride %zu, out_stride %zu", n, a_stride,
                               out_stride);
    if (!n)
        return PDDC_OK;
    if (!(d_out == d_a && out_stride == a_stride) &&
        ranges_overlap(d_out, rows_extent(s->nrx, n, out_stride, 4), d_a, rows_extent(s->nrx, n, a_stride, 4)))
        return pddc_set_error_(PDDC_EINVAL, "eq: out overlaps a (in place is out == a with equal strides)");
    PDDC_TRY(set_device(s->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(s->table.upload(st));
    EqArgs a{};
    a.a = static_cast<const uint32_t *>(d_a);
    a.a_stride = (long long)a_stride;
    a.out = static_cast<uint32_t *>(d_out);
    a.out_stride = (long long)out_stride;
    a.n = (long long)n;
    a.rx = s->table.dev();
    a.nrx = s->nrx;
    a.S = s->S;
    a.old_state = s->state.old();
    a.new_state = s->state.next();
    a.fresh = s->fresh ? 1u : 0u;
    PDDC_HIP_TRY(launch_eq(a, st));
    /* the launch was accepted: only now does the record turn; the restart marks go, and the table on the device follows
     * with the next batch */
    s->state.turn();
    s->fresh = false;
    for (EqRx &r : s->table.host)
        if (r.flags & kEqRestart) {
            r.flags &= ~kEqRestart;
            s->table.dirty = true;
        }
    return PDDC_OK;
}

int pddc_eq_read_state(pddc_eq *s, double *host, void *stream)
{
    if (!s || !host)
        return null_argument();
    PDDC_TRY(set_device(s->device));
    const size_t count = (size_t)s->nrx * (size_t)s->S * 2;
    if (s->fresh)
        std::memset(host, 0, sizeof(double) * count);
    return read_back(host, s->fresh ? nullptr : s->state.old(), count, (hipStream_t)stream);
}

} // extern "C"
