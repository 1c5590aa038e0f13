/*
 * ddc_fax.h -- internal launch interface between the radiofax decoder's host code (ddc_fax.cpp) and its gfx950 kernel
 * (ddc_fax.hip).  Not part of the public ABI (that is include/perseus_ddc.h).  The clock's closed form, the line
 * structure and the bounds both sides share are in ddc_fax_bits.h.
 */
#ifndef PDDC_DDC_FAX_H
#define PDDC_DDC_FAX_H

#include "ddc_fax_bits.h"
#include "ddc_decoder_rx.h"

namespace pddc {

static constexpr int kFaxBack = (int)kFaxBoxMost;       /* discriminator values kept in front of a tile: B - 1 are read */
static constexpr int kFaxTilePix = kDecTile / 2;        /* pixels of a tile at the most (inc <= 2^31)              */
/* the tile's pixels in LDS lie as they will in memory, 0 .. 3 bytes behind a word's first; whole words of 4 */
static constexpr int kFaxPixBytes = (kFaxTilePix + 3 + 3) / 4 * 4 + 4;

/* LDS per receiver of the group: the input row (float2), kFaxBack + TT discriminator values (float), the tile's pixels
 * and, a byte each, the samples they were strobed at */
static constexpr size_t kFaxRowBytes = (size_t)(kFaxBack + kDecTile) * sizeof(float) + (size_t)kFaxPixBytes + (size_t)kFaxTilePix;
inline size_t fax_lds_bytes(int window) { return (size_t)kDecGroup * ((size_t)dec_in_slots(window) * sizeof(float2) + kFaxRowBytes); }
static constexpr size_t kFaxLdsCap = (size_t)kDecGroup * ((size_t)(kDecMaxWindow - 1 + kDecTile) * 8 + kFaxRowBytes);
static_assert(kFaxRowBytes % 8 == 0, "the rows behind the first stay aligned");

/* receiver flags beside kDecOn and the marks: kDecClear also means y, f, acc and the level as at create */
static constexpr uint32_t kFaxReverse = 0x2;
static constexpr uint32_t kFaxReline = kDecThird;       /* another modem: the line structure as at create, y, f, acc and the level stay */
static constexpr uint32_t kFaxMarks = kDecFresh | kDecClear | kFaxReline;

/* what a receiver carries behind its inputs; read() reports from it */
struct FaxState {
    FaxLine l;
    uint32_t acc;
    uint32_t pad;
    float2 y;                 /* the filter's last output                                                        */
    float f[kFaxBack];        /* the last discriminator values, the newest last                                  */
};

struct FaxArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    FaxLineRec *chars;        /* the lines, [nrx][char_stride]: named as the walk's launch names a decoder's records */
    long long char_stride;    /* >= the bound of pddc_fax_max_lines: the host refuses less                       */
    uint32_t *counts;         /* [nrx]                                                                           */
    uint8_t *pix;             /* [nrx][pix_stride]                                                               */
    long long pix_stride;     /* >= the bound of pddc_fax_max_pixels                                             */
    uint32_t *npix;           /* [nrx]                                                                           */
    float *disc;              /* [nrx][disc_stride] or NULL                                                      */
    long long disc_stride;    /* >= n                                                                            */
    const float *taps;        /* [nbank][dec_row(W)]                                                             */
    const FaxModem *bank;     /* [nbank]                                                                         */
    const DecRx *rx;          /* [nrx]                                                                           */
    const FaxState *state;    /* [nrx] (not read where fresh)                                                    */
    FaxState *new_state;
    const float2 *hist;       /* [nrx][W - 1]: the inputs before the batch's first (not read where fresh or cleared) */
    float2 *new_hist;
    int nrx;
    int nbank;
    int window;               /* W                                                                               */
};

/* k_fax: grid ceil(nrx / kDecGroup) */
hipError_t launch_fax(const FaxArgs &a, hipStream_t s);

} // namespace pddc
#endif
