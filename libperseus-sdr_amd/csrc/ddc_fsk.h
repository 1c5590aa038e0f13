/*
 * ddc_fsk.h -- internal launch interface between the FSK decoder's host code (ddc_fsk.cpp) and its gfx950 kernel
 * (ddc_fsk.hip).  Not part of the public ABI (that is include/perseus_ddc.h).
 */
#ifndef PDDC_DDC_FSK_H
#define PDDC_DDC_FSK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kFskMaxRx = 1024;
static constexpr int kFskMaxModems = 16;
static constexpr int kFskMaxWindow = 256;
static constexpr int kFskGroup = 4;                     /* G: receivers per block, one wave each                   */
static constexpr int kFskThreads = 64 * kFskGroup;
static constexpr int kFskOut = 4;                       /* O: outputs per lane and tile, 64 apart                  */
static constexpr int kFskTile = 64 * kFskOut;           /* TT: outputs per receiver and tile                       */
static constexpr int kFskStep = 8;                      /* taps per pass of the tap loop                           */
/* a modem's taps on the device: per tap (hm.re, hm.im, hs.re, hs.im), W taps rounded up to a whole number of passes
 * (zeros behind the W-th: the tap loop loads whole passes and runs the first W taps only) */
inline __host__ __device__ int fsk_row(int window) { return (window + kFskStep - 1) / kFskStep * kFskStep; }

/* LDS per receiver of the group: W - 1 carried inputs and a tile of them (float2), the tile's d (float), and 2 O
 * 64-bit masks, the tile's decisions and rising edges */
inline __host__ __device__ int fsk_row_slots(int window) { return window - 1 + kFskTile; }
inline size_t fsk_lds_bytes(int window)
{
    return (size_t)kFskGroup * ((size_t)fsk_row_slots(window) * sizeof(float2) + (size_t)kFskTile * sizeof(float) + 2 * kFskOut * 8);
}
static constexpr size_t kFskLdsCap =
    (size_t)kFskGroup * ((size_t)(kFskMaxWindow - 1 + kFskTile) * 8 + (size_t)kFskTile * 4 + 2 * kFskOut * 8);

/* receiver flags on the device: the header's two and the marks of the host */
static constexpr uint32_t kFskOn = 0x1, kFskReverse = 0x2;
static constexpr uint32_t kFskFresh = 0x100;            /* create / reset: nothing carried is read, all of it is zero */
static constexpr uint32_t kFskClear = 0x200;            /* RESTART, OFF -> ON: carried inputs zero, IDLE, prev = mark */
static constexpr uint32_t kFskIdle = 0x400;             /* another modem: IDLE, a character in progress is dropped  */
static constexpr uint32_t kFskMarks = kFskFresh | kFskClear | kFskIdle;

static constexpr uint32_t kFskStIdle = 0, kFskStStart = 1, kFskStData = 2, kFskStStop = 3;

struct FskRx {
    int32_t modem;
    uint32_t flags;
};

struct FskModem {
    uint32_t inc;             /* bit phase per sample, 1 .. 2^30                                                 */
    uint32_t nbits;           /* 5 .. 8                                                                          */
};

/* what the start-stop receiver carries; read() reports from it */
struct FskState {
    uint64_t start;           /* sample index of the edge of the character in progress                           */
    uint32_t state;           /* kFskSt*                                                                         */
    uint32_t acc;
    uint32_t k;
    uint32_t shift;
    float qmin;
    uint32_t prev;            /* the previous sample's `space`                                                   */
    uint32_t chars, framing, false_starts;
    float d_last;
};

/* pddc_fsk_char, 16 bytes */
struct FskChar {
    uint64_t start;
    uint16_t code;
    uint16_t flags;
    float quality;
};

struct FskArgs {
    const float2 *z;          /* z[j * z_stride + i], i < n                                                      */
    long long z_stride;
    long long n;              /* samples per receiver of this launch, > 0                                        */
    unsigned long long m0;    /* samples before this launch                                                      */
    FskChar *chars;           /* [nrx][char_stride]                                                              */
    long long char_stride;    /* >= the bound of pddc_fsk_max_chars: the host refuses less                       */
    uint32_t *counts;         /* [nrx]                                                                           */
    float *d;                 /* [nrx][d_stride] or NULL                                                         */
    long long d_stride;
    const float *taps;        /* [nmodems][fsk_row(W)][4]                                                        */
    const FskModem *modems;   /* [nmodems]                                                                       */
    const FskRx *rx;          /* [nrx]                                                                           */
    const FskState *state;    /* [nrx] (not read where fresh)                                                    */
    FskState *new_state;
    const float2 *hist;       /* [nrx][W - 1]: the inputs before the batch's first (not read where fresh or cleared) */
    float2 *new_hist;
    int nrx;
    int nmodems;
    int window;               /* W                                                                               */
};

/* k_fsk: grid ceil(nrx / kFskGroup) */
hipError_t launch_fsk(const FskArgs &a, hipStream_t s);

} // namespace pddc
#endif
