/*
 * ddc_decoder_rx.h -- what both sides of a decoder (fsk, morse, psk, sitor; fax, whose records are lines) name: the constants of the kernels' walk
 * (ddc_decoder_dev.h), the receiver record of the table and its flag bits.  No function of the device and no pragma:
 * ddc_<decoder>.h includes it for the host files (ddc_decoder.h) and the kernels alike.  Internal.
 */
#ifndef PDDC_DDC_DECODER_RX_H
#define PDDC_DDC_DECODER_RX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pddc {

static constexpr int kDecMaxRx = 1024;
static constexpr int kDecMaxBank = 16;                  /* modems or keyers                                        */
static constexpr int kDecMaxWindow = 256;
static constexpr int kDecGroup = 4;                     /* G: receivers per block, one wave each                   */
static constexpr int kDecThreads = 64 * kDecGroup;
static constexpr int kDecOut = 4;                       /* O: outputs per lane and tile, 64 apart                  */
static constexpr int kDecTile = 64 * kDecOut;           /* TT: samples per receiver and tile                       */
static constexpr int kDecStep = 8;                      /* taps per pass of the tap loop                           */
/* a bank entry's taps on the device: W taps rounded up to a whole number of passes (zeros behind the W-th: the tap
 * loop loads whole passes and runs the first W taps only) */
inline __host__ __device__ int dec_row(int window) { return (window + kDecStep - 1) / kDecStep * kDecStep; }
/* the input row of a receiver in LDS, in float2: W - 1 carried inputs and a tile of them */
inline __host__ __device__ int dec_in_slots(int window) { return window - 1 + kDecTile; }

/* receiver flags on the device: ON and the marks of the host; a decoder's own bits lie between them */
static constexpr uint32_t kDecOn = 0x1;
static constexpr uint32_t kDecFresh = 0x100;            /* create / reset: nothing carried is read, all of it is zero */
static constexpr uint32_t kDecClear = 0x200;            /* RESTART, OFF -> ON: the carried inputs read as zero     */
static constexpr uint32_t kDecThird = 0x400;            /* the decoder's own mark, if it has one                   */

struct DecRx {
    int32_t bank;             /* the receiver's modem or keyer                                                   */
    uint32_t flags;
};

} // namespace pddc
#endif
