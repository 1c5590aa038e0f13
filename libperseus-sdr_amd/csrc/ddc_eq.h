/*
 * ddc_eq.h -- internal launch interface between the equaliser's host code (ddc_eq.cpp) and its gfx950 kernel
 * (ddc_eq.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_EQ_H
#define PDDC_DDC_EQ_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kEqMaxRx = 1024;
static constexpr int kEqMaxSections = 8;                    /* S: 1, 2, 4 or 8; PDDC_EQ_MAX_SECTIONS             */
/* waves of one block: each wave walks its own receivers with its own rows, so a block of several waves is several blocks
 * of one behind the same barriers; NOTEBOOK.md has the measurement that chose 1.  (-DPDDC_EQ_WAVES=4: an A/B build) */
#ifndef PDDC_EQ_WAVES
#define PDDC_EQ_WAVES 1
#endif
static constexpr int kEqWaves = PDDC_EQ_WAVES;
static_assert(kEqWaves == 1 || kEqWaves == 2 || kEqWaves == 4, "waves per block: 1, 2 or 4");
static constexpr int kEqThreads = 64 * kEqWaves;
static constexpr int kEqTile = 256;                         /* TT: samples per tile                              */
/* receivers of one wave, at most: a receiver has L = S lanes, so 64 / L of them fit; the chain's latency bounds a step
 * whatever the number of busy lanes, so fewer receivers per wave cost a wave nothing and give more waves to spread over
 * the compute units (8: 128 waves for 1024 receivers at every S, and a tile's prefetch in 32 registers).  The same bits
 * either way; NOTEBOOK.md has the measurement that chose.  (The macro is for a same-box A/B build of another share,
 * tools/ab.sh build group16:"-DPDDC_EQ_GROUP=16") */
#ifndef PDDC_EQ_GROUP
#define PDDC_EQ_GROUP 8
#endif
static constexpr int kEqGroup = PDDC_EQ_GROUP;
static_assert(kEqGroup == 8 || kEqGroup == 16 || kEqGroup == 32, "receivers per wave at most: 8, 16 or 32");
static constexpr uint32_t kEqRestart = 1u;                  /* PDDC_EQ_RESTART                                   */

constexpr int eq_group(int sections) { return 64 / sections < kEqGroup ? 64 / sections : kEqGroup; }

/* one receiver as the kernel sees it */
struct EqRx {
    uint32_t nsec;      /* sections that run, 0 .. S; 0: the words pass                        */
    uint32_t flags;     /* kEqRestart: this launch takes the carried states as 0               */
    double c[kEqMaxSections][5];   /* b0, b1, b2, a1, a2 of section s < nsec                   */
};

struct EqArgs {
    const uint32_t *a;        /* the words of a[j * a_stride + i], i < n                                        */
    long long a_stride;
    uint32_t *out;            /* out[j * out_stride + i]; may be a itself (equal strides)                       */
    long long out_stride;
    long long n;              /* samples per receiver of this launch, > 0                                       */
    const EqRx *rx;           /* [nrx]                                                                          */
    int nrx;
    int S;                    /* the object's sections: 1, 2, 4 or 8                                            */
    const double *old_state;  /* [nrx][S][2]: s1, s2 as the batch before left them (not read when `fresh`)      */
    double *new_state;        /* the same, written by this launch                                               */
    uint32_t fresh;           /* the carried record is not read: the states are 0                               */
};

/* k_eq: grid ceil(nrx / (kEqWaves eq_group(S))) blocks of kEqWaves waves */
hipError_t launch_eq(const EqArgs &a, hipStream_t s);

} // namespace pddc
#endif
