/*
 * perseus_ddc.h -- thin C ABI over the MI355X (gfx950) I/Q ingest + decimation
 * kernels.  Plain pointers and sizes only; no C++/torch types.
 *
 * What each entry point stands in for in the reference (libperseus-sdr):
 *
 *   pddc_unpack24_f32      examples/perseustest.c:466-502  user_data_callback_c_f
 *   pddc_unpack24_i32      examples/perseustest.c:432-460  user_data_callback_c_u
 *                          (dup. examples/simple.c:33-61)
 *   pddc_pack24_f32        (none) inverse of the above: what the FPGA emits on USB endpoint
 *                          0x82 -- 24-bit packed samples at the selected rate -- so that an
 *                          unmodified client sees the wire format it expects (perseustest.c:434)
 *   pddc_nco_freg          perseus-sdr.c:584   tuning word written to the FPGA
 *   pddc_pipeline_*        the FPGA DDC itself (NCO mix + decimating FIR chain)
 *                          that perseus_set_sampling_rate() selects by bitstream
 *                          (perseus-sdr.c:776-867) and perseus_set_ddc_center_freq()
 *                          tunes (perseus-sdr.c:556-619); no software model of it
 *                          exists in the reference, so its arithmetic is defined
 *                          by oracle/perseus_oracle.c.
 *   pddc_pipeline_push_host   what perseus-in.c:206-207 hands to the client
 *                          callback, batched (see perseus-sdr.h in this directory
 *                          for the drop-in callback API built on top of this).
 *   pddc_pipeline_push_host_async / _wait_ticket / pddc_host_alloc
 *                          the ring of 8 in-flight USB transfers of perseus-in.c:39-118
 *                          (queue create / submit / resubmit), as two pinned batches in
 *                          flight: copy in, kernels and copy out of neighbouring batches overlap
 *   pddc_pipeline_seek     (none) positions a pipeline inside ONE stream so that several
 *                          GPUs can take contiguous time chunks of it
 *
 * Sample formats
 *   packed : 6 bytes / complex sample, I0 I1 I2 Q0 Q1 Q2, 24-bit two's
 *            complement little endian (examples/perseustest.c:449-455)
 *   f32    : interleaved float32 I,Q  (8 bytes / sample), range [-1.00000012, 1]
 *   i32    : interleaved int32 I,Q, MSB aligned (multiples of 256)
 *
 * All functions return PDDC_OK (0) or a negative PDDC_E* code, and set a
 * thread-local message readable through pddc_last_error().  There is NO CPU
 * fallback: without a usable HIP device every compute entry point fails with
 * PDDC_ENODEV.
 *
 * "d_" pointers are device (HBM) addresses, "h_" pointers host addresses.
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).
 */
#ifndef PERSEUS_DDC_H
#define PERSEUS_DDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libperseus_ddc.so is built with -fvisibility=hidden: what this header declares is ALL the library exports (its C++
 * internals -- kernel stubs, launchers, the pipeline classes -- stay out of the dynamic symbol table) */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define PDDC_OK          0
#define PDDC_EINVAL     -1   /* bad argument (size, alignment, NULL)          */
#define PDDC_ENODEV     -2   /* no HIP device / device index out of range      */
#define PDDC_EHIP       -3   /* a HIP runtime call failed                      */
#define PDDC_ENOMEM     -4   /* allocation failed                              */
#define PDDC_ECAPACITY  -5   /* output buffer too small                        */
#define PDDC_ESTATE     -6   /* call not valid in the pipeline's current state */
#define PDDC_ECOMM      -7   /* an RCCL call failed                             */

#define PDDC_ADC_CLK_HZ        80000000.0   /* perseus-sdr.h:44 */
#define PDDC_MAX_STAGES        4
#define PDDC_MAX_TAPS          4096         /* rational (interp > 1) stages       */
#define PDDC_MAX_TAPS_DECIM    1024         /* plain decimators                   */
#define PDDC_FAST_MAX_TAPS     256          /* fused decimate-by-8 kernel      */
#define PDDC_PACKED_BYTES      6
#define PDDC_INPUT_GRANULE     8            /* process(): nsamples % 8 == 0    */

/* pipeline flags */
#define PDDC_F_MIX         0x1u   /* NCO complex mix before stage 0            */
#define PDDC_F_TAPS_FP16   0x2u   /* binary16 taps (config 5): rounded to binary16; a /8 first stage without NCO on the
                                     matrix cores (k_fir_i8x's plain form) then holds them on the device AS binary16, 2
                                     bytes a tap, and its matrix waves quantise them themselves; the other kernels keep
                                     the rounded values in fp32, tuned tables are built on the host from them */
#define PDDC_F_NO_FAST     0x4u   /* force the generic kernels (testing)       */
#define PDDC_F_OUT_PACKED24 0x8u  /* process()/push_host() emit 24-bit packed (6 B/sample)
                                     instead of float32: "FPGA emulation"      */

typedef struct pddc_pipeline pddc_pipeline;

typedef struct {
    int          decim;    /* decimation factor D (M of a rational L/M stage), >= 1 */
    int          ntaps;    /* 1 .. PDDC_MAX_TAPS_DECIM (PDDC_MAX_TAPS if interp > 1) */
    const float *taps;     /* h[0..ntaps-1], host memory, copied               */
    int          interp;   /* 0 or 1: plain decimator.  L > 1: rational resampler
                              y[m] = sum_j h[j*L + (m*D mod L)] * x[floor(m*D/L) - j]
                              (upsample by L, filter, keep every D-th); used for the
                              reference's non-integer rates  */
} pddc_stage_desc;

/* ---- library ------------------------------------------------------------ */
int         pddc_version(void);
const char *pddc_last_error(void);
int         pddc_device_count(void);                 /* >= 0, or PDDC_E*      */

/* ---- tuning word (perseus-sdr.c:584) ------------------------------------ */
uint32_t    pddc_nco_freg(double center_freq_hz, double adc_clk_hz);

/* ---- stateless kernels on device-resident buffers ------------------------ */
/* d_packed must be 16-byte aligned; nsamples may be any value >= 0.          */
int pddc_unpack24_f32(const void *d_packed, size_t nsamples, void *d_out_f32, void *stream);
int pddc_unpack24_i32(const void *d_packed, size_t nsamples, void *d_out_i32, void *stream);
/* float32 I/Q -> 24-bit packed: code = clamp(rint(x*8388607), -2^23, 2^23-1).  */
int pddc_pack24_f32(const void *d_in_f32, size_t nsamples, void *d_out_packed, void *stream);
/* synthetic source of BASELINE.md section 3: byte k of the LCG stream
 * s=s*1664525+1013904223, byte=s>>24, starting `byte_offset` bytes in.        */
int pddc_synth_lcg(void *d_dst, size_t nbytes, uint32_t seed, uint64_t byte_offset, void *stream);

/* ---- device memory helpers for C hosts (tests/bench use torch instead) ----
 * No reference counterpart: the reference's only buffers are the eight libusb transfer buffers of a queue in host
 * memory (perseus-in.c:67-110, input_queue_create); everything here exists because the DSP moved from the FPGA
 * into HBM. */
int pddc_set_device(int device);
int pddc_malloc(void **d_ptr, size_t nbytes);
int pddc_free(void *d_ptr);
/* Device memory for a buffer that is streamed AGAINST d_partner (one read while the other is written -- the packed
 * input and the float output of a pipeline): HBM is laid out in a few classes of large extents, and such a pair runs
 * ~8 % faster (k_fir8 127 taps: 0.340 instead of 0.367 ms) when the two buffers lie in extents of different classes;
 * allocations made one after the other usually share one.  This allocates candidates 8 GiB apart (spacers, freed
 * again), times a read+write probe stream between the partner and each, stops when both speeds have been seen or after
 * max_candidates, and returns the fastest (free it with pddc_free).  *ms_best / *ms_worst: the probe's time per launch
 * for the kept and for the slowest candidate.  Buffers under 1 MiB, a partner under 64 MiB, or max_candidates <= 1: a
 * plain allocation.  A buffer between 1 MiB and 1 GiB gets a 1 GiB allocation (the probe must write past the 256 MB
 * last-level cache to see the HBM), because small write streams matter too: the fused first two stages of the /320
 * cascade write 1/48 of what they read and still run at 0.292 or 0.330 ms depending on where that small buffer lies.
 * Candidates and spacers never take more than half of the free memory; a probe that fails leaves a plain allocation.
 * pddc_pipeline_place_buffers does this for a pipeline's own inter-stage buffers (process() never searches).         */
int pddc_malloc_apart(void **d_ptr, size_t nbytes, const void *d_partner, size_t partner_bytes, int max_candidates,
                      float *ms_best, float *ms_worst);
/* Where in ONE large allocation of the caller's (tens of GiB; 288 GB of HBM make it affordable) does a pipeline's write
 * side go?  The arena is cut into slots of slot_bytes; the packed batch lies at the arena's start (fill it BEFORE the
 * call), the write side at out_offset of a slot.  The probe is the pipeline's OWN first kernel: one fused stage writes its
 * nsamples / D outputs there; a cascade's inter-stage workspace (pddc_pipeline_workspace_size bytes) is set there with
 * pddc_pipeline_set_workspace and stays at the chosen slot -- the caller puts the output behind it.  Probed: the slot
 * right behind the input ("first come"), +32 / +48 / +64 GiB, every slot only if none of those gains 3 %; 0.1-0.2 s.
 * *ms_first_come / *ms_best: the kernel's time at slot 1 and at the returned slot.  Stream state is not advanced.
 * Worth 1-8 % (which slots are fast is a property of the process's physical layout, found, not modelled); a host that
 * does not care skips it.  This is the one placement entry point for caller-owned memory: rounds 2-4 also had
 * pddc_arena_search / pddc_arena_place, which ranked the slots with a read+write MODEL stream -- on one box in a dozen it
 * ranked them opposite to the kernel it stood for, so they are gone.  (No reference counterpart.)                  */
int pddc_pipeline_arena_place(pddc_pipeline *p, void *d_arena, size_t arena_bytes, size_t slot_bytes, size_t nsamples,
                              size_t out_offset, size_t *out_slot, float *ms_first_come, float *ms_best, int *nprobes,
                              void *stream);
int pddc_memcpy_h2d(void *d_dst, const void *h_src, size_t nbytes, void *stream);
int pddc_memcpy_d2h(void *h_dst, const void *d_src, size_t nbytes, void *stream);
int pddc_stream_sync(void *stream);

/* ---- DDC pipeline: [NCO mix] -> stage 0 -> ... -> stage n-1 --------------- */
int pddc_pipeline_create(pddc_pipeline **out, int device,
                         const pddc_stage_desc *stages, int nstages, uint32_t flags);
int pddc_pipeline_destroy(pddc_pipeline *p);
/* zero FIR histories, decimation phases and the NCO sample counter            */
int pddc_pipeline_reset(pddc_pipeline *p);

/* Inter-stage buffers of a cascade from CALLER-provided device memory instead of the pipeline's own allocations, so that
 * the host decides where they lie (the buffer a stage writes should sit in another HBM extent class than the batch the
 * stage reads -- see pddc_malloc_apart; bench.py cuts input, workspace and output from one arena and keeps the fastest
 * arrangement).  d_ws: 256-byte aligned, nbytes >= pddc_pipeline_workspace_size(p, max_nsamples); batches of more than
 * max_nsamples are then refused (PDDC_ECAPACITY).  Synchronises the device; call between batches.  d_ws == NULL
 * returns to own allocations.  The memory stays the caller's; stream state (histories, phases) is not touched.
 * (No reference counterpart: libperseus-sdr's buffers are libusb transfers, perseus-in.c:67-110.)               */
size_t pddc_pipeline_workspace_size(const pddc_pipeline *p, size_t max_nsamples);
int pddc_pipeline_set_workspace(pddc_pipeline *p, void *d_ws, size_t nbytes, size_t max_nsamples);
/* The same decision for the pipeline's OWN inter-stage buffers (a host that does not manage a workspace): allocates
 * them now, for batches of up to max_nsamples samples read from d_packed, each through the candidate walk of
 * pddc_malloc_apart against the buffer its writer reads.  Probes run on `stream`; candidates and spacers take at most
 * half of the free device memory and are freed again; a failing probe leaves a plain allocation.  About a second per
 * buffer, once.  pddc_pipeline_process itself never searches: without this call (or a workspace) the buffers are plain
 * allocations made when the first batch arrives.  (No reference counterpart.)                                    */
int pddc_pipeline_place_buffers(pddc_pipeline *p, const void *d_packed, size_t max_nsamples, void *stream);
/* reset, then place the stream at absolute input sample `abs_sample` with zero history:
 * the NCO phase and every stage's decimation phase are those of a stream that started at
 * sample 0.  This is what lets ONE stream be cut into time chunks for several GPUs
 * (SURVEY.md 8e (2)): a rank seeks to (chunk start - halo), processes halo + chunk and drops
 * the first halo/decimation outputs; the NCO needs no hand-over because its phase is a pure
 * function of the absolute index (perseus-sdr.c:584).  abs_sample must lie on an output
 * boundary of every stage (a multiple of the product of the decimation factors is enough)
 * and be a multiple of PDDC_INPUT_GRANULE.                                                */
int pddc_pipeline_seek(pddc_pipeline *p, uint64_t abs_sample);
/* New tuning word from the next sample on.  The NCO is a phase accumulator, like the FPGA's:
 * phase(n) = n*freg + offset (mod 2^32), and a retune at sample n moves the offset by
 * n*(freg_old - freg_new) so that the phase is continuous there (no phase jump on retune).
 * reset()/seek() clear the offset (phase of a stream that began at sample 0 with this word). */
int pddc_pipeline_set_freg(pddc_pipeline *p, uint32_t freg);
uint32_t pddc_pipeline_get_phase_offset(const pddc_pipeline *p);
int pddc_pipeline_set_center_freq(pddc_pipeline *p, double center_freq_hz);
int pddc_pipeline_set_taps(pddc_pipeline *p, int stage, const float *taps, int ntaps);
uint32_t pddc_pipeline_get_freg(const pddc_pipeline *p);
int pddc_pipeline_total_decim(const pddc_pipeline *p);
/* upper bound of outputs a process() of nsamples_in can produce               */
size_t pddc_pipeline_max_output(const pddc_pipeline *p, size_t nsamples_in);
/* exactly what the NEXT process()/push of nsamples_in will produce (depends on the
 * decimation phases the stream is at)                                          */
size_t pddc_pipeline_next_output(const pddc_pipeline *p, size_t nsamples_in);
/* 1 if stage 0 runs the fused unpack+mix+polyphase kernel for this geometry   */
int pddc_pipeline_uses_fused(const pddc_pipeline *p);
/* nonzero if a batch of nsamples_in would run stage 0 on the int8 matrix cores (the wire bytes are the operand, the
 * taps are quantised to 2^-31 of the largest one; same history, same outputs to 1e-7 of full scale)               */
int pddc_pipeline_stage0_on_i8(const pddc_pipeline *p, size_t nsamples_in);
/* The return value says WHICH kernel: 0 none (k_fir8), 2 k_fir_i8x (1 was round 3's k_fir_i8, retired in round 5: one
 * kernel family) -- without NCO its plain form, one tap table; with it the NCO folded into the taps, y[m] = LO(n0 + 8m) sum_k (h[k] e^{+j theta k}) x_raw[8m - k]: complex taps on the raw
 * integer planes, one float rotation per output -- which every tuned (PDDC_F_MIX) decimate-by-8 first stage of 1..256
 * taps runs on, i.e. every pipeline the drop-in API builds behind perseus_set_ddc_center_freq (perseus-sdr.c:556-619);
 * with a decimate-by-8 second stage of <= 64 taps behind a first stage of <= 128 and whole 8192-sample tiles, both are one kernel
 * (pddc_pipeline_uses_fused_pair answers 2).  The one batch whose history window straddles a retune takes k_fir8.   */
/* The operands k_fir_i8x reads, as the library builds them (host arithmetic, no device needed), from
 * Hc[k] = round(h[k] cos(theta k) 2^E) and Hs[k] = round(h[k] sin(theta k) 2^E), theta k = 2 pi ((k freg) mod 2^32) / 2^32
 * (`mix` = 0: H[k] = round(h[k] 2^E), one table, pddc_fir_i8_table's).  A table is 4 digit planes x ksteps x 64 lanes x 16
 * bytes in the matrix instruction's lane order.  hist = 32, 64 or 128 with `mix`: TWO tables of paired rows -- rows 0..7 the
 * band of eight outputs for one tap set, rows 8..15 the band of the same outputs for the other: [Hc ; Hs] meets the I
 * planes, [-Hs ; Hc] the Q planes, one set of int32 accumulators takes both, rows 0..7 are uI, rows 8..15 uQ;
 * ksteps = (56 + hist + 63) / 64.  hist = 256 with `mix`: the 16-row tables of Hc and of Hs, ksteps = (120 + hist + 63) / 64
 * (as without `mix`).  ct[0], ct[1]: the byte planes' offset constants of uI = gc * xI - gs * xQ and
 * uQ = gs * xI + gc * xQ.  Returns the number of tables written (1 or 2).                                           */
int pddc_fir_i8x_tables(const float *taps, int ntaps, int hist, int mix, uint32_t freg, int8_t *tables, size_t tables_bytes,
                        float *scale, float *ct /* [2] */);
/* ... the same for the tuned decimate-by-10 first stage (the 1.6 MS/s plan's; hist = 64, columns of 8 outputs 80 samples
 * apart, 3 k-steps): tt = c - 10 (r & 7); the taps delayed by `delay` = 0 .. 7 samples, g[k] = h[k - delay] e^{+j theta k},
 * which is how a batch whose first output does not fall on a multiple of 8 samples is put on the loaders' 8-sample groups
 * (ntaps + delay <= 64).  Two tables of 4 * 3 * 1024 bytes. */
int pddc_fir_i8x_d10_tables(const float *taps, int ntaps, int delay, uint32_t freg, int8_t *tables, size_t tables_bytes,
                            float *scale, float *ct /* [2] */);
/* ... and the fused second stage's taps: out[i] = Re g2[64 - i], out[68 + i] = Im g2[64 - i], i = 0 .. 64,
 * g2[k] = h2[k] e^{+j 8 theta k} (a first-stage output is 8 input samples); 136 floats */
int pddc_fir_i8x_taps2(const float *taps2, int ntaps2, int mix, uint32_t freg, float *out, size_t out_len);
/* Kernel selection is API state, not environment: name = "no_i8", "i8x", "i8x_pair", "i8x_plain", "i8x_blocks",
 * "i8x_chunk", "i8x_layout", "i8x_pair_max_log2", "no_fuse2", "fuse3" (the PDDC_* environment variables of the same names
 * are read once, when the pipeline is created).
 * PDDC_ESTATE while overlap mode holds a tail back (fence first), PDDC_EINVAL for an unknown name.                  */
int pddc_pipeline_set_option(pddc_pipeline *p, const char *name, int value);
/* Process-wide development knobs of the launchers (tile schedule of k_fir8, block shapes, gang plumbing): "fir8_dyn_pct",
 * "fir8_chunk", "fir8_walk" (1: chunks handed round the blocks, 0: static runs + dynamic tail, -1: the launcher's default), "gen_shape_nt", "gen_shape_p", "no_firp", "firp_packed_p", "unpack_blocks", "debug", "push_three_streams",
 * "gang_copy_out", "gang_gen_inline", "gang_solo", "chan_run", "wblank_run" (samples one workgroup of the wideband
 * blanker walks), "wblank_chunk" (samples one round of its launches takes); 0: automatic.  Their PDDC_<NAME> environment variables are read once, at first use;
 * no library call on the data path looks at the environment.                                                         */
int pddc_set_tunable(const char *name, int value);
int pddc_get_tunable(const char *name, int *value);
int pddc_pipeline_get_option(const pddc_pipeline *p, const char *name, int *value);
/* The tap operand k_fir_i8x's plain form reads, as the library builds it (host arithmetic, no device needed; for tests and for
 * hosts that want to look at the quantisation): taps -> H[k] = round(h[k] * 2^E), E = 30 - ceil(log2 max|h|), as four
 * balanced base-256 digits d_j[k] in [-128, 127]; table[j][ks][lane][jj] = d_j[hist - (c - 8 r)] for r = lane & 15,
 * c = 64 ks + 16 (lane >> 4) + jj and 1 <= c - 8 r <= hist, else 0 (the banded Toeplitz matrix in the lane order of
 * v_mfma_i32_16x16x64_i8); 4 * ksteps * 1024 bytes with ksteps = (120 + hist + 63) / 64, hist = 32, 64, 128 or 256.  *scale turns the
 * integer result into the reference's float, *cterm is the constant that undoes the byte planes' -128 offset.       */
int pddc_fir_i8_table(const float *taps, int ntaps, int hist, int8_t *table, size_t table_bytes, float *scale, float *cterm);
/* With PDDC_F_TAPS_FP16 (no NCO) the device holds no such table but the taps as IEEE binary16, and the kernel's matrix waves quantise
 * them into their operand registers: out[128 + tt] = binary16(h[hist - tt]) for tt = 1 .. hist, zeros elsewhere,
 * PDDC_FIR_I8_TAPS16_LEN entries (lane (r, kq) reads the 16 values 128 + 64 ks + 16 kq - 8 r + jj of k-step ks as two
 * aligned 16-byte loads); H = llround(value * *two_e), digits as above.  Host arithmetic, no device needed. */
#define PDDC_FIR_I8_TAPS16_LEN 512
int pddc_fir_i8_taps16(const float *taps, int ntaps, int hist, uint16_t *out, size_t out_len, double *two_e);
/* 1 if stage 0 reads the packed samples itself (the fused decimate-by-8, or the generic decimator
 * with its unpack-while-staging load phase for any other first decimation): no float32
 * intermediate of the input is ever written; 6 + 8/D bytes per input sample                  */
int pddc_pipeline_stage0_reads_packed(const pddc_pipeline *p);
/* 1 if a process() of nsamples would run stages 0 AND 1 as one kernel (both
 * decimate-by-8, stage 1 <= 64 taps, nsamples a multiple of the kernel's tile):
 * the stage-0 output then never reaches HBM                                    */
int pddc_pipeline_uses_fused_pair(const pddc_pipeline *p, size_t nsamples);
/* 1 if a process() of nsamples would run stages 0, 1 AND 2 as one kernel (the fused pair followed by a plain
 * decimator whose group of tiles fits the LDS, e.g. the 8*8*5 and 8*8*10 plans of the 250 and 125 kS/s rates):
 * the whole cascade is then one streaming pass, 6 + 8/D bytes per input sample                               */
int pddc_pipeline_uses_fused_cascade(const pddc_pipeline *p, size_t nsamples);
/* Waits for `stream`, then reports whether a kernel of this pipeline has flagged a failure since the last reset (the
 * fused cascade's blocks hand each other FIR history inside the launch; their wait is bounded and a block that
 * gives up says so here: PDDC_EHIP).  PDDC_OK otherwise.  Tests and bench.py call it after their runs.          */
int pddc_pipeline_check(pddc_pipeline *p, void *stream);

/* Device-resident batch: d_packed (16-byte aligned, nsamples % 8 == 0) ->
 * d_out_f32 (16-byte aligned, capacity in complex samples; with
 * PDDC_F_OUT_PACKED24 it receives 6 bytes per sample instead of 8).  Asynchronous on
 * `stream`; *n_out (host) is written before return (it depends only on sizes).
 * Stream state (FIR history, phase, NCO counter) advances by nsamples.  The state
 * lives in device memory ordered by `stream`: use ONE stream per pipeline, and do
 * not mix process() and push_host() (which runs on the pipeline's own stream)
 * without a synchronisation in between.                                        */
int pddc_pipeline_process(pddc_pipeline *p, const void *d_packed, size_t nsamples,
                          void *d_out_f32, size_t out_capacity, size_t *n_out, void *stream);
/* Overlap mode for three-stage cascades whose first two stages run as the fused pair (pddc_pipeline_uses_fused_pair):
 * the third stage -- 1/64 of the samples, a tenth of the arithmetic, but one more kernel in the row with its launch
 * gaps, 11 % of the /320 step -- is NOT launched with its batch.  The NEXT process() makes it part of its own launch:
 * extra thread blocks behind the pair's persistent ones, on waves the pair leaves idle (the pair writes the other half
 * of a double-buffered workspace meanwhile).  One stream, no events.  The price is one batch of latency in what
 * `stream` holds: behind process() k, the outputs up to batch k-1 are complete; pddc_pipeline_fence(p, stream) launches
 * the tail that is still held back -- call it before the last output is read, and before save_state / set_taps /
 * set_overlap / set_workspace / set_option (they answer PDDC_ESTATE while a tail is held back).  The output buffer given to process() k must stay valid until the launch of k+1 (or the fence).
 * Batches that do not take the fused pair (not whole tiles) fence by themselves and run in line; push_host* fence every
 * batch (they are PCIe-bound).  Call set_overlap BEFORE pddc_pipeline_workspace_size / _set_workspace: the workspace
 * then holds stage 2's input twice.  No reference counterpart (the FPGA's stages all run at once).              */
int pddc_pipeline_set_overlap(pddc_pipeline *p, int enable);
int pddc_pipeline_fence(pddc_pipeline *p, void *stream);
/* Host batch: H2D copy, process, D2H copy, synchronous.                        */
int pddc_pipeline_push_host(pddc_pipeline *p, const void *h_packed, size_t nsamples,
                            void *h_out_f32, size_t out_capacity, size_t *n_out);
/* The same, returning at once: the batch travels H2D -> kernels -> D2H on three streams
 * through one of two staging slots, so with two batches in flight the copy in, the kernels
 * and the copy out of neighbouring batches overlap (the pinned, double-buffered host ring
 * the reference's 6 KB callback buffers need).  *n_out is known at
 * return (it depends on sizes only); h_packed and h_out must stay valid, and h_out unread,
 * until pddc_pipeline_wait_ticket(*ticket) -- at most two tickets (0, 1) are outstanding,
 * pushing a third batch reuses the older slot and waits for it on the device side.  For
 * the copies to be truly asynchronous both host buffers should come from pddc_host_alloc
 * (pinned memory); pageable memory works but the runtime stages it.                      */
int pddc_pipeline_push_host_async(pddc_pipeline *p, const void *h_packed, size_t nsamples,
                                  void *h_out_f32, size_t out_capacity, size_t *n_out, int *ticket);
/* The same with the synthetic source of BASELINE.md section 3 generated ON the device (the
 * batch is bytes [byte_offset, byte_offset + 6*nsamples) of the LCG stream of `seed`,
 * bit-identical to the host loop): no host -> device traffic, so a C host driving several
 * virtual receivers is not bound by a single-thread CPU generator.                         */
int pddc_pipeline_push_synth_async(pddc_pipeline *p, uint32_t seed, uint64_t byte_offset, size_t nsamples,
                                   void *h_out_f32, size_t out_capacity, size_t *n_out, int *ticket);
/* 1 if the batch of `ticket` has completely arrived in its h_out, 0 if not yet (non-blocking) */
int pddc_pipeline_ticket_done(pddc_pipeline *p, int ticket);
int pddc_pipeline_wait_ticket(pddc_pipeline *p, int ticket);
int pddc_pipeline_wait(pddc_pipeline *p);          /* everything pushed so far is complete */
/* ---- gang: several pipelines of ONE GPU, one launch chain --------------------------------
 * The reference serves up to eight receivers from one poll thread (perseus-sdr.c:43-47 the
 * descriptor table, 736-774 the thread); here several of them may share a GPU.  A batch of
 * 2^22 samples keeps the GPU busy for a few dozen microseconds -- about what ONE launch costs
 * in front of it -- so a launch chain per receiver leaves the GPU waiting for the host.  A gang
 * round pushes the next batch (the same nsamples) of up to PDDC_GANG_MAX pipelines through one
 * stream with ONE launch per kernel: the generator (or one H2D copy each), the first-stage
 * kernel with the receiver as the grid's second dimension -- every receiver its own tuning
 * word, phase, histories and buffers --, the decimator behind it likewise, one D2H copy
 * each and ONE event.  Results are bit-identical to pushing every pipeline by itself
 * (pddc_pipeline_push_*_async): the kernels' code and every receiver's arguments are the same.
 * Members whose plan is not "fused /8 first stage [+ /8 fused with it] [+ one plain
 * decimator]" (resampling rates, a first stage that is not /8, packed output) still go out in
 * the round, as launches of their own on the gang's stream; *n_ganged says how many shared.
 * Tickets are the pipelines' own (pddc_pipeline_wait_ticket).  A pipeline may change between
 * gang rounds and pushes of its own at any batch boundary (the change waits for what it still
 * has in flight).  One thread at a time per gang.  Everything that can refuse a round (null
 * pointers, capacities, a pipeline twice, a held-back overlap tail) is checked before anything is
 * queued: such a call leaves every stream where it was.  A failure AFTER that (a HIP error while
 * queueing) leaves the round's members in an undefined position: reset or destroy them.  A
 * member's h_out must stay the kind of memory it was when first seen (pinned or pageable): the
 * answer is remembered per staging slot.                                                     */
#define PDDC_GANG_MAX 8
typedef struct pddc_gang pddc_gang;
typedef struct {
    pddc_pipeline *pipe;
    const void    *h_packed;      /* host batch (6*nsamples bytes), or NULL: the on-device LCG source ... */
    uint32_t       seed;          /* ... of this seed ...                                                 */
    uint64_t       byte_offset;   /* ... from this byte of its stream                                     */
    void          *h_out;         /* receives the outputs (float2, or packed with PDDC_F_OUT_PACKED24)     */
    size_t         out_capacity;  /* in samples                                                            */
    size_t         n_out;         /* out: outputs of this batch                                            */
    int            ticket;        /* out                                                                   */
} pddc_gang_item;
int pddc_gang_create(pddc_gang **out, int device);
int pddc_gang_destroy(pddc_gang *g);      /* after (or before) its pipelines: waits for what is in flight */
int pddc_gang_push_async(pddc_gang *g, pddc_gang_item *items, int n, size_t nsamples, int *n_ganged);

/* ---- bank: several tuned receivers from ONE read of the same batch -------------------------
 * A gang round shares launches, but every receiver still reads its own copy of the batch.  A
 * bank is a fixed set of up to PDDC_BANK_MAX pipelines of one GPU that are fed the SAME batch
 * every round; members whose first stage is the tuned decimate-by-8 on the matrix cores (<= 64
 * taps: history 32 or 64) share its launch -- one read of the batch for up to four of them
 * (k_fir_i8x_bank) -- grouped by history length into launches of 4, 2 and 1 members (8 = 4 + 4,
 * 6 = 4 + 2, 3 = 2 + 1).  Members whose first stage is the tuned decimate-by-10 on the matrix
 * cores (the 1, 1.6 and 2 MS/s plans: history 48 or 56) share it in PAIRS: two members whose batch
 * puts its first stage-0 output on the same decimation phase (0 .. 9) take one launch, the longer
 * history first, whatever their histories; a member of a phase without a partner runs alone.
 * Everything behind the first stage runs per member as in pddc_pipeline_process, and a banked
 * member's outputs, histories, counters and save_state blob are bit for bit what
 * pddc_pipeline_process gives that pipeline alone -- with option no_fuse2 = 1 for the
 * decimate-by-8 members.  Each member keeps its own plan, word, taps, options and buffers.
 * A member is banked in a round when its batch would take k_fir_i8x alone (decimate by 8), or the
 * tuned decimate-by-10 form with at least one stage-0 output, with one tuning word in its history
 * window (no retune inside it), no overlap mode, no packed output, no stage-0 timing or failure
 * injection and default k_fir_i8x options -- and it is ALIGNED: its stage-0 history is the bank's
 * (the last samples of the previous round's batch, or zeros while every member is fresh).  A member
 * is aligned after create if it was fresh (created, reset or seek, nothing processed), and after
 * every round whose batch held at least its history length (a decimate-by-10 member that was
 * aligned stays so through a shorter one); anything done to it outside the bank (process, push,
 * reset, seek, restore_state, set_taps) makes it unaligned for one round -- and a decimate-by-10
 * member that processed a batch of its own may sit on another phase than its partner from then on.
 * Members that are not banked run pddc_pipeline_process on the same stream in the same round:
 * every member's output is correct in every round, only the sharing changes.
 * A pipeline belongs to at most one bank; destroy the bank before its members.  A member
 * destroyed first is detached: the bank refuses further rounds (PDDC_ESTATE) and can still be
 * destroyed.  Everything that can refuse a round (null pointers or capacities, a detached member,
 * a held-back overlap tail, nsamples not a multiple of 8) is checked before anything is queued:
 * such a call leaves every stream where it was.  A failure AFTER that (a HIP error while queueing,
 * or an error an unbanked member's own processing reports, e.g. an overlap-mode member whose
 * workspace cannot take its tail) leaves the members before it advanced and the rest where they
 * were: reset or destroy them.  One thread at a time per bank. */
#define PDDC_BANK_MAX 8
typedef struct pddc_bank pddc_bank;
/* members[0 .. n): distinct pipelines on `device`, none in another bank (PDDC_ENODEV without a GPU) */
int pddc_bank_create(pddc_bank **out, int device, pddc_pipeline *const *members, int n);
int pddc_bank_destroy(pddc_bank *b);
/* one batch of nsamples at d_packed through every member; member i writes d_out[i] (capacity out_capacity[i]),
 * n_out[i] = its outputs; *n_banked = members whose first stage shared a bank launch.  Stream-ordered like
 * pddc_pipeline_process. */
int pddc_bank_process(pddc_bank *b, const void *d_packed, size_t nsamples, void *const *d_out,
                      const size_t *out_capacity, size_t *n_out, int *n_banked, void *stream);
/* what the next round of nsamples would do: bit i set = member i shares a bank launch; *launches = bank launches
 * (a decimate-by-8 group of one is a launch of the solo kernel and counts; a decimate-by-10 pair is one launch) */
int pddc_bank_schedule(const pddc_bank *b, size_t nsamples, unsigned *banked_mask, int *launches);

/* ---- panorama: averaged power spectrum of the packed stream --------------------
 * Stands in for NOTHING in the reference: the FPGA has no spectrum output and the reference's
 * example clients compute none; a client that wants one works on the host from the callback
 * buffers.  Here the packed ADC-rate samples are read once, as they lie in HBM (the same d_packed
 * a pipeline or a bank reads), and no float copy of them is ever written.
 *
 * x[n] = I[n] + j Q[n], the float32 values of pddc_unpack24_f32, n counted since create / reset;
 * w[0 .. N) the caller's real window, N = nfft in {1024, 2048, 4096, 8192}, hop = N or N/2.
 * Segment s covers samples [s hop, s hop + N);  X_s[k] = sum_n w[n] x[s hop + n] exp(-2 pi i k n / N),
 * k = 0 .. N-1, DC first (a tone exp(+2 pi i k0 n / N) lands in bin k0);
 *   sum[k]  = sum over the COMPLETE segments of |X_s[k]|^2    (no normalisation: float full scale squared)
 *   peak[k] = max over the same segments                        (PDDC_SPEC_PEAK)
 * The segment grid belongs to the stream, not to the batch: the object carries the last
 * N - hop + (length mod hop) packed samples (fewer than N) across process() calls, so the set of
 * segments does not depend on how the stream is cut; a batch may be shorter than a segment.
 * Sums are accumulated without atomics in an order fixed by the batch sizes: the same batches give
 * the same bits (another cut of the same stream may differ in the last bits).
 * Stream-ordered like pddc_pipeline_process: one stream per object, one thread at a time.
 * process() queues two launches and moves the host-side counters only after both were accepted; a
 * refused call (PDDC_EINVAL: nsamples not a multiple of 8, d_packed NULL or not 16-byte aligned)
 * queues nothing.  Argument errors are answered before any device access; with good arguments and
 * no device create answers PDDC_ENODEV. */
typedef struct pddc_spectrum pddc_spectrum;
#define PDDC_SPEC_PEAK 0x1u      /* also keep peak[k] */
int pddc_spectrum_create(pddc_spectrum **out, int device, int nfft, int hop, const float *window /* [nfft], copied */,
                         uint32_t flags);
int pddc_spectrum_destroy(pddc_spectrum *s);
int pddc_spectrum_reset(pddc_spectrum *s);       /* sums, peak, tail, sample counter; synchronises the device */
int pddc_spectrum_process(pddc_spectrum *s, const void *d_packed, size_t nsamples, void *stream);
/* what is accumulated since the last clear: d_sum / d_peak float32[nfft] on the device (either may be NULL; d_peak must
 * be NULL without PDDC_SPEC_PEAK); *nsegments (host) is known from sizes alone, like process()'s *n_out; clear != 0
 * zeroes sums and peak afterwards, in stream order -- the tail and the segment grid go on */
int pddc_spectrum_read(pddc_spectrum *s, void *d_sum, void *d_peak, uint64_t *nsegments, int clear, void *stream);
/* Every batch the pipeline is PUSHED from now on (pddc_pipeline_push_host_async / _push_synth_async, a gang round) also
 * goes through `s`: the same device batch, on the stream the batch's kernels run on (the pipeline's own, or the gang's),
 * so a pddc_spectrum_read on another stream comes after pddc_pipeline_wait.  s == NULL detaches.  The pipeline does not
 * own `s`: detach or destroy the pipeline first.  pddc_pipeline_process itself is unchanged (the caller has d_packed). */
int pddc_pipeline_attach_spectrum(pddc_pipeline *p, pddc_spectrum *s);
/* segments the NEXT process() of nsamples completes */
uint64_t pddc_spectrum_next_segments(const pddc_spectrum *s, size_t nsamples);
/* the same without an object (host arithmetic, no device): segments completed by nsamples more samples of a stream
 * that already holds samples_before; 0 for unsupported sizes */
uint64_t pddc_spectrum_segments(int nfft, int hop, uint64_t samples_before, size_t nsamples);

/* ---- channelizer: M uniform channels of the packed stream as time series --------
 * Stands in for NOTHING in the reference either (the FPGA delivers one tuned channel).  All M
 * equally spaced channels of the ADC-rate stream, each filtered by the caller's real prototype
 * low-pass and decimated, as complex samples -- from ONE read of the packed batch (a polyphase
 * filter bank by weighted overlap-add: the panorama's transform behind a longer, folded window).
 *
 * x[n] = I[n] + j Q[n], the float32 values of pddc_unpack24_f32, n counted since create / reset.
 * M = nchan in {1024, 2048, 4096}; prototype w[0 .. L), real float32, L = proto_len = P M with
 * P in {1, 2, 4, 8} taps per branch and L <= 16384; hop D in {M, M/2} (critically sampled /
 * oversampled by 2).  Row s exists once sample s D + L - 1 is in the stream (zero history is NOT
 * assumed: only complete windows, like the panorama's complete segments):
 *   y[s][k] = sum_{n=0}^{L-1} w[n] x[s D + n] exp(-2 pi i k (s D + n) / M),     k = 0 .. M-1
 * The phase is counted from the stream's sample 0, so channel k is a proper base-band series: a
 * tone exp(+2 pi i k0 n / M) gives the constant sum(w) in channel k0, every row.  (With D = M/2
 * the factor exp(-2 pi i k s D / M) is the sign (-1)^(k s).)  In the terms of a tuned pipeline:
 * channel k is the decimate-by-D FIR h = [0, w[L-1], .., w[0]] behind the NCO word k 2^32 / M,
 * output s + L/D of a stream with zero history.
 * Channel range: only channels (first + i) mod M, i < count, are written; a row is `count`
 * complex float32, interleaved (re, im), rows consecutive: out[s count + i].
 * Channel list (set_channels): instead of a range, channels[0 .. n), 1 <= n <= 1024, each in
 * [0, M), pairwise distinct, in any order; a row then is n values, out[s n + i] = y[s][channels[i]],
 * and `count` is n wherever it means values per row (capacity, next_rows).  A value's bits are those
 * the range mode gives for the same (M, D, P, w, samples, channel): they do not depend on the list,
 * its order or the mode.  set_range returns to range mode; either takes effect from the next
 * process(), the rows go on without a gap.
 * Stream semantics are the panorama's: the row grid belongs to the stream, the object carries the
 * last (fewer than L) packed samples across process() calls, a batch may be shorter than L, and
 * batches cut anywhere on a multiple of 8 samples give the same rows -- here the same BITS: a
 * row's bits depend on (M, D, P, w, the samples) alone, not on the cut, the range or the launch.
 * process() knows the row count from sizes alone, checks every argument before any device access
 * and before anything is queued (PDDC_EINVAL: nsamples not a multiple of 8, d_packed NULL or not
 * 16-byte aligned, d_out NULL or not 8-byte aligned when rows are due; PDDC_ECAPACITY:
 * out_capacity_rows too small -- nothing queued, no state moved), and moves its counters only
 * after every launch was accepted.  Stream-ordered; one stream per object, one thread at a time.
 * create: argument errors are answered before any device access; good arguments and no device:
 * PDDC_ENODEV.  flags: 0 (reserved). */
typedef struct pddc_channelizer pddc_channelizer;
int pddc_channelizer_create(pddc_channelizer **out, int device, int nchan, int hop,
                            const float *proto /* [proto_len], copied */, int proto_len, int first, int count,
                            uint32_t flags);
int pddc_channelizer_destroy(pddc_channelizer *c);
int pddc_channelizer_reset(pddc_channelizer *c);      /* tail, sample and row counters; synchronises the device */
/* one batch; d_out: out_capacity_rows rows of `count` complex float32; *n_rows (host, may be NULL) = rows written */
int pddc_channelizer_process(pddc_channelizer *c, const void *d_packed, size_t nsamples, void *d_out,
                             size_t out_capacity_rows, size_t *n_rows, void *stream);
/* another channel range, from the next process() on (the rows go on without a gap) */
int pddc_channelizer_set_range(pddc_channelizer *c, int first, int count);
/* list mode from the next process() on: rows of n values, out[s n + i] = y[s][channels[i]].  The list is copied.
 * PDDC_EINVAL, nothing changed: NULL, n outside 1 .. 1024, an entry outside [0, nchan), a duplicate. */
int pddc_channelizer_set_channels(pddc_channelizer *c, const int *channels, int n);
/* rows the NEXT process() of nsamples writes */
uint64_t pddc_channelizer_next_rows(const pddc_channelizer *c, size_t nsamples);
/* the same without an object (host arithmetic, no device): rows completed by nsamples more samples of a stream that
 * already holds samples_before; 0 for unsupported sizes */
uint64_t pddc_channelizer_rows(int nchan, int hop, int proto_len, uint64_t samples_before, size_t nsamples);

/* ---- tuner: many freely tuned narrowband receivers behind the channelizer --------
 * K receivers, each with its own 32-bit NCO word, read the channelizer's rows on the device and
 * give K narrowband complex series.  The channelizer: M = nchan, D = hop, prototype w[0 .. L),
 * range first / count, b = log2 M, rows y[s][k], s counted from the stream's first row.  Receiver
 * j with word F_j (frequency F_j fs / 2^32, the sign convention of pddc_nco_freg: a tone at that
 * frequency comes out at 0 Hz):
 *   channel  k_j = ((F_j + 2^(31-b)) mod 2^32) >> (32 - b)   (nearest centre, wrapping to 0 at the top)
 *   residue  r_j = (int32)(F_j - (k_j << (32 - b))),   in [-2^(31-b), 2^(31-b))
 *   phase    theta_j[s] = (r_j (s D) + phi_j) mod 2^32, all in unsigned 32-bit arithmetic (s D taken
 *            mod 2^32); phi_j = 0 at create and reset
 *   z_j[s]   = y[s][k_j] exp(-2 pi i theta_j[s] / 2^32)
 *   out_j[m] = sum_{t<T} h[t] z_j[m R + T - 1 - t],   m = 0, 1, ..: it exists once row m R + T - 1 is
 *            in the stream (complete windows only, no zero history).  h: real float32 low-pass of
 *            T = ntaps taps, R = decim: both common to all receivers.  Output rate fs / (D R).
 * This is the receiver tuned to F_j: z_j[s] = sum_n w[n] e^{+2 pi i r_j n / 2^32} x[s D + n]
 * e^{-2 pi i (F_j (s D + n) + phi_j) / 2^32} -- the stream mixed with the accumulator F_j n + phi_j
 * and filtered by the prototype shifted by r_j towards its channel centre.
 * Retune: set_freq(j, F') takes effect at the next row the tuner is given, row s0.  The accumulator
 * is continuous (the increment changes, never the phase): phi_j' = phi_j + (F_j - F') (s0 D) mod 2^32.
 * Rows before s0 keep the z they had, so the first T - 1 outputs after a retune mix old and new
 * tuning.  A word whose channel lies outside the channel range: PDDC_EINVAL, nothing changed.
 * Channel list (set_channels, after pddc_channelizer_set_channels with the same list, between two
 * batches): rows are [nrows][n] in the list's order, receiver j reads the column at which k_j stands
 * in the list; several receivers may share a listed channel.  A list that misses a current
 * receiver's channel, and in list mode a set_freq to a word whose channel is not listed:
 * PDDC_EINVAL, nothing changed.  To retune to an unlisted channel, between two batches: set the
 * union list on both objects, set_freq, then (optionally) the shrunk list on both.  The carried z is
 * indexed by the caller's receiver index, so a list change leaves it as it is, like a range change.
 * set_range returns to range mode.
 * Stream semantics are the channelizer's: the tuner counts rows itself and must be given every row
 * since create / reset, in order, as [nrows][count] complex float32 of the CURRENT range
 * (set_range follows pddc_channelizer_set_range, between two batches); it carries what the next
 * outputs need of the last rows (fewer than T per receiver) across process() calls; a batch may
 * hold any number of rows, 0 included.  Output: out[j out_stride + m], complex float32, m counted
 * from 0 in every call.  The bits of out_j[m] depend on (M, D, F_j and its retune history, h, R, the
 * rows) alone: not on the cut into batches, K, j, the other receivers or the channel range.
 * process() knows the output count from sizes alone, checks every argument before any device
 * access and before anything is queued (PDDC_EINVAL: d_rows NULL or not 8-byte aligned when
 * nrows > 0, d_out NULL or not 8-byte aligned when outputs are due; PDDC_ECAPACITY: out_stride
 * smaller than the outputs due -- nothing queued, no state moved), and moves its counters only
 * after every launch was accepted.  Stream-ordered; one stream per object, one thread at a time.
 * Limits: 1 <= nrx <= 1024, 1 <= ntaps <= 512, 1 <= decim <= 64, flags 0.  create: argument errors
 * (a word outside the range among them) before any device access; good arguments, no device:
 * PDDC_ENODEV. */
typedef struct pddc_tuner pddc_tuner;
int pddc_tuner_create(pddc_tuner **out, int device, int nchan, int hop, int first, int count,   /* the channelizer's */
                      const uint32_t *freg /* [nrx], copied */, int nrx, const float *taps /* [ntaps], copied */,
                      int ntaps, int decim, uint32_t flags);
int pddc_tuner_destroy(pddc_tuner *t);
int pddc_tuner_reset(pddc_tuner *t);                  /* row counter, carried rows, phase offsets; synchronises the device */
int pddc_tuner_set_freq(pddc_tuner *t, int rx, uint32_t freg);
int pddc_tuner_set_range(pddc_tuner *t, int first, int count);        /* every receiver must lie inside it */
/* the channelizer's list (pddc_channelizer_set_channels), from the next process() on; every receiver's channel must be in it */
int pddc_tuner_set_channels(pddc_tuner *t, const int *channels, int n);
/* one batch of rows; *n_out (host, may be NULL) = outputs written per receiver */
int pddc_tuner_process(pddc_tuner *t, const void *d_rows, size_t nrows, void *d_out, size_t out_stride,
                       size_t *n_out, void *stream);
/* outputs per receiver the NEXT process() of nrows writes */
uint64_t pddc_tuner_next_outputs(const pddc_tuner *t, size_t nrows);
/* what process(nrows) would launch now (host arithmetic: launches nothing, moves no counter):
 * out = { receivers per block, outputs per tile, outputs per run, blocks along the outputs, rows carried afterwards }
 * -- block x of a receiver group owns the outputs [x run, (x + 1) run) of the batch, tile by tile; with no outputs
 * { group, tile, 0, 0, carried }.  For tests, which place their cases on these seams. */
int pddc_tuner_schedule(const pddc_tuner *t, size_t nrows, int out[5]);
/* the same without an object (host arithmetic, no device); 0 for unsupported sizes */
uint64_t pddc_tuner_outputs(int ntaps, int decim, uint64_t rows_before, size_t nrows);
/* channel and residue of a word (host arithmetic, no device); either pointer may be NULL */
int pddc_tuner_channel(int nchan, uint32_t freg, int *channel, int32_t *residue);
/* the distinct channels of nrx words (pddc_tuner_channel's rule), ascending, into channels[nrx]: the list for the two
 * set_channels calls (host arithmetic, no device).  -> how many, or a negative PDDC_E* (NULL, nrx <= 0, unsupported nchan) */
int pddc_tuner_channel_list(int nchan, const uint32_t *freg, int nrx, int *channels /* [nrx] */);

/* ---- demod: AM, FM and SSB audio from the tuner's receivers ---------------------
 * K receivers, each a complex float32 series z_j[m] at the tuner's output rate, give K real float32
 * series a_j[m], one output per input.  m counts since create / reset and goes on across batches;
 * z_j[-1] = 0.  All arithmetic is float32 with floating-point contraction off, the same operation
 * sequence for every caller and every cut (DESIGN.md 8 spells the sequence).
 * Detector d_j[m], by the receiver's mode:
 *   PDDC_DEMOD_AM   d = sqrtf(re re + im im)
 *   PDDC_DEMOD_FM   p = z[m] conj(z[m-1]) (four multiplies, one add, one subtract),
 *                   d = atan2f(p.im, p.re) (1/pi), in [-1, 1]: 1 is a deviation of half the output rate.
 *                   Where there is no older z (the first output after create, reset or a change of mode
 *                   or flags) d = 0.
 *   PDDC_DEMOD_SSB  theta = (bfo m + psi) mod 2^32 in unsigned 32-bit arithmetic, psi = 0 at create and
 *                   reset; d = re c - im s with c + i s = exp(-2 pi i theta / 2^32): the real part of z
 *                   times the phasor, the sign convention of pddc_nco_freg.  USB, LSB and CW are SSB with a
 *                   choice of words: tune the tuner to the middle of the wanted sideband, give its low-pass
 *                   half the sideband's width, and bfo moves the sideband back.
 * Post stage, by the receiver's flags, sequential in m:
 *   PDDC_DEMOD_DCBLOCK  y[m] = fmaf(rho, y[m-1], d[m] - d[m-1]), y[-1] = d[-1] = 0; without it y = d
 *   PDDC_DEMOD_AGC      e[m] = fmaxf(|y[m]|, lambda e[m-1]), e[-1] = 0; g = fminf(gmax, target / e[m])
 *                       (e = 0 gives gmax); a = y g; without it a = y
 * rho, lambda, target, gmax are common to all receivers: 0 <= rho, lambda < 1; target, gmax > 0, finite.
 * Carried per receiver: z[m-1], d[m-1], y[m-1], e[m-1], psi.  The bits of a_j[m] depend on the
 * receiver's series, its mode / word / flag history and the four parameters alone: not on the cut into
 * batches (0 outputs included), K, j's index, the other receivers, grid or tile sizes.
 * set_rx(j, mode, bfo, flags) between two batches takes effect from the next output m0.  The word
 * alone: phase-continuous, psi' = psi + (bfo - bfo') m0 mod 2^32 (the tuner's rule).  Another mode or
 * other flags: that receiver's carried z, d, y, e return to their create values and psi = 0; m goes on.
 * An unknown mode or flag: PDDC_EINVAL, nothing changed.
 * Non-finite samples are data like any other: what they do follows from the operations above, in the receiver's own
 * row alone.  The detector of a NaN sample is NaN (FM: of that output and the next).  Without a post stage that is
 * all.  DCBLOCK: y is NaN from there on, and so is every output, until the caller acts.  AGC without DCBLOCK: one NaN
 * output, e = fmaxf(NaN, lambda e) steps over it.  An infinite y leaves e = inf for good (lambda inf): the gain is 0
 * and every later output 0.  The caller gets the row back with set_rx to another mode or other flags (and back), or
 * reset.
 * process(): z is [nrx][z_stride] complex float32 and out [nrx][out_stride] float32, n values used per
 * row (the strides in elements: the tuner's output view has its capacity as stride).  Every argument
 * is checked before anything is queued: PDDC_EINVAL for NULL or misaligned (8 / 4 bytes) pointers with
 * n > 0, PDDC_ECAPACITY when a stride is below n; n = 0 is valid and does nothing.  State moves only
 * after the launch was accepted.  Stream-ordered; one stream per object, one thread at a time.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_DEMOD_AM       0
#define PDDC_DEMOD_FM       1
#define PDDC_DEMOD_SSB      2
#define PDDC_DEMOD_DCBLOCK  0x1u
#define PDDC_DEMOD_AGC      0x2u
typedef struct pddc_demod_rx {
    int mode;             /* PDDC_DEMOD_AM / _FM / _SSB                   */
    uint32_t bfo;         /* SSB: the BFO word (frequency bfo fs_out / 2^32) */
    uint32_t flags;       /* PDDC_DEMOD_DCBLOCK | PDDC_DEMOD_AGC          */
} pddc_demod_rx;
typedef struct pddc_demod_params {
    float rho;            /* DC block pole                                */
    float lambda;         /* AGC envelope decay per output                */
    float target;         /* AGC output level                             */
    float gmax;           /* AGC largest gain                             */
} pddc_demod_params;
typedef struct pddc_demod pddc_demod;
int pddc_demod_create(pddc_demod **out, int device, int nrx, const pddc_demod_rx *rx /* [nrx], copied */,
                      const pddc_demod_params *params);
int pddc_demod_destroy(pddc_demod *d);
int pddc_demod_reset(pddc_demod *d);                  /* m, carried values, psi; synchronises the device */
int pddc_demod_set_rx(pddc_demod *d, int rx, int mode, uint32_t bfo, uint32_t flags);
int pddc_demod_process(pddc_demod *d, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                       void *stream);
/* outputs per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_demod_tile_outputs(void);

/* ---- rxfilter: each receiver its own bandwidth from a filter bank ----------------
 * A stage between the tuner and the demodulator.  Receiver j's input is z_j[i], complex float32; i
 * counts since create / reset and goes on across batches; z_j[i] = 0 for i < 0 (zero history, as in
 * audio).  One output per input, so the demodulator's m behind it is the same m.
 * Fixed at create: nrx (1 .. 1024); a bank of B filters (1 .. 64) of T real float32 taps each
 * (1 .. 256), bank[f T + t], copied, every value finite; per receiver a filter index f_j in [0, B).
 * Value, float32 with floating-point contraction off, the same operation sequence for every caller
 * and every cut: acc = (0, 0); for t = 0 .. T-1 ascending: acc.re = fmaf(h_f[t], z_j[m - t].re, acc.re)
 * and the same for im; out_j[m] = acc, with f = f_j(m).  All T taps are always run: a shorter filter
 * is padded with zeros by the caller.  Symmetric filters of one bank share the delay (T - 1) / 2, so
 * the receivers stay aligned in time.
 * set_rx(j, f') between two batches takes effect from the next output m0: outputs m >= m0 use h_f'
 * over the same inputs, the carried ones before m0 included -- what is carried is inputs, not filter
 * state, so nothing is reset and there is no gap.  f' outside [0, B) or j outside [0, nrx):
 * PDDC_EINVAL, nothing changed.
 * Carried per receiver: its last T - 1 inputs; the object carries m, for reporting only.  The bits of
 * out_j[m] depend on the receiver's series, its filter history and the bank alone: not on the cut
 * into batches (batches of 0, 1 and fewer than T - 1 inputs included), nrx, j's index, the other
 * receivers and their filters, strides, grid or tile sizes.
 * Non-finite samples: transient.  A NaN in z_j[p] makes the T outputs p .. p + T - 1 of that receiver NaN, in the part
 * (re or im) it is in, zero-valued taps included (0 NaN is NaN); every other output, and every other receiver, has
 * the bits it has without it.  An infinity does the same with inf or, against a zero tap or an opposite infinity, NaN.
 * Nothing is left behind once the sample has left the window: the caller does nothing.
 * process(): z is [nrx][z_stride] and out [nrx][out_stride] complex float32, n values used per row
 * (the strides in elements: the tuner's output view has its capacity as stride).  Every argument is
 * checked before anything is queued: PDDC_EINVAL for NULL or not 8-byte aligned pointers with n > 0,
 * PDDC_ECAPACITY when a stride is below n, PDDC_EINVAL when the input and output byte ranges overlap
 * (tiles read their neighbours' inputs: in place is not supported); n = 0 is valid, launches nothing
 * and changes nothing.  State moves only after the launch was accepted.  Stream-ordered; one stream
 * per object, one thread at a time.  create: argument errors before any device access; good
 * arguments, no device: PDDC_ENODEV. */
typedef struct pddc_rxfilter pddc_rxfilter;
int pddc_rxfilter_create(pddc_rxfilter **out, int device, int nrx, const float *bank /* [nfilters][ntaps], copied */,
                         int nfilters, int ntaps, const int *sel /* [nrx] */);
int pddc_rxfilter_destroy(pddc_rxfilter *f);
int pddc_rxfilter_reset(pddc_rxfilter *f);            /* m and the carried inputs; synchronises the device */
int pddc_rxfilter_set_rx(pddc_rxfilter *f, int rx, int filter);
int pddc_rxfilter_process(pddc_rxfilter *f, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                          void *stream);
/* outputs per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_rxfilter_tile_outputs(void);

/* ---- carrier: synchronous AM with a tracking PLL per receiver -------------------
 * A stage between the receiver filter and the demodulator.  K receivers (1 .. 1024), each a complex
 * float32 series z_j[m], give K complex float32 series u_j[m], one output per input, whose real part
 * is the synchronous audio: the demodulator in PDDC_DEMOD_SSB with word 0 behind it takes that real
 * part bit for bit (its phasor is (1, 0)) and adds DC block and AGC.  m counts since create / reset
 * and goes on across batches.  All arithmetic is float32 with floating-point contraction off, the
 * same operation sequence for every caller and every cut (DESIGN.md 8 spells the sequence).
 * Per receiver and output, in this order:
 *   1. rotation: c + i s = exp(-2 pi i theta[m] / 2^32) from the exact 32-bit word (the phasor of
 *      pddc_nco_freg's convention); w.re = z.re c - z.im s, w.im = z.re s + z.im c (two multiplies and
 *      one subtract / add each).
 *   2. phase detector: e = atan2f(w.im, w.re) (1/pi), in [-1, 1] half-turns; atan2f(0, 0) = 0.
 *   3. loop filter (PI): v[m] = fminf(vmax, fmaxf(-vmax, fmaf(ki, e, v[m-1])));
 *      step = fmaf(kp, e, v[m]); theta[m+1] = theta[m] + (uint32_t)(int32_t)rint(step 2^31) in unsigned
 *      32-bit arithmetic (round to nearest even); theta[0] = 0, v[-1] = 0.  With kp <= 0.5 and
 *      vmax < 0.5, |step| < 1, so the conversion cannot overflow.
 *   4. lock metric: q[m] = fmaf(gamma, |e| - q[m-1], q[m-1]), q[-1] = 0.
 *   5. output by the receiver's mode; h is the caller's Hilbert filter, L taps (odd, 3 .. 255),
 *      D = (L - 1) / 2, common to all receivers, copied at create, every value finite:
 *      PDDC_CARRIER_DSB  u[m] = w[m], no delay.
 *      PDDC_CARRIER_USB / _LSB  acc = 0; for k = 0 .. L-1 ascending: acc = fmaf(h[k], w[m-k].im, acc);
 *                        u.re = w[m-D].re - acc (USB) or + acc (LSB); u.im = w[m-D].im; w[i] = 0 for
 *                        i < 0.  All L taps are always run.
 *      PDDC_CARRIER_OFF  the loop is not run: theta, v, q stay as they are, w = z bit for bit, u = z.
 * Common, fixed at create: vmax in (0, 0.5), gamma in (0, 1], lock_thr > 0 (finite), h[L].
 * Per receiver, changeable between two batches with set_rx(j, mode, kp, ki): the mode, kp in
 * (0, 0.5], ki in [0, 0.25].  Another kp / ki alone keeps everything carried: the loop goes on without
 * a gap.  Another mode returns that receiver's theta, v, q and its w history to their create values
 * (0); m goes on.  An unknown mode, a value out of range, j outside [0, nrx): PDDC_EINVAL, nothing
 * changed.
 * Carried per receiver: theta, v, q and the last L - 1 values of w.  The bits of u_j[m] and of the
 * carried values depend on the receiver's own series, its set_rx history and the common parameters
 * alone: not on the cut into batches (n = 0 included), K, j's index, the other receivers, strides,
 * grid or tile sizes.
 * Non-finite samples, in the receiver's own row alone.  A NaN in z[m] makes w[m] and e NaN.  v: fmaxf and fminf drop
 * the NaN, v[m] = -vmax, and the loop goes on from there.  theta: a NaN step adds 0 to theta (C leaves that conversion
 * undefined; this is the rule here).  q is NaN from there on, so read() gives err = NaN and locked = 0 until the caller
 * acts.  u: NaN at m (DSB), at the L outputs m .. m + L - 1 in re and at m + D in im (USB / LSB, zero-valued taps
 * included); later outputs are finite again.  OFF passes the sample as it is.  An infinite sample: with re and im both
 * infinite, or one of them infinite against a phasor component that is exactly 0 (theta = 0 among others), w is NaN
 * (inf c - inf s, inf 0) and everything is as after a NaN; with one infinite part and ordinary c and s, w is
 * (+-inf, +-inf), whose angle is a finite number: the loop takes a wrong step and q stays finite.  The caller gets err
 * and locked back with set_rx to another mode (and back), or reset.
 * process(): z is [nrx][z_stride] and u [nrx][u_stride] complex float32, n values used per row (the
 * strides in elements).  d_u may be d_z with the same stride (in place); any other overlap of the two
 * byte ranges is PDDC_EINVAL.  Every argument is checked before anything is queued: PDDC_EINVAL for
 * NULL or not 8-byte aligned pointers with n > 0, PDDC_ECAPACITY when a stride is below n; n = 0 is
 * valid and does nothing.  State moves only after the launch was accepted.  Stream-ordered; one
 * stream per object, one thread at a time.
 * read(): per receiver theta (theta[m+1] behind the last output m: the word the next output is
 * rotated by), freq (v: the carrier's offset is v rate / 2 Hz), err (q) and locked (q < lock_thr),
 * behind the batches submitted so far (it waits for them).  AFC: add freq, turned into a tuner word,
 * to the receiver's tuner word.  locked is the comparison and nothing else: a receiver
 * with its create values (just created, reset or given another mode) and an OFF receiver have q = 0
 * and read as locked with freq = 0, and q needs some 1 / gamma outputs to say anything; a caller that
 * retunes on locked waits that long after such an event.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_CARRIER_OFF  0
#define PDDC_CARRIER_DSB  1
#define PDDC_CARRIER_USB  2
#define PDDC_CARRIER_LSB  3
typedef struct pddc_carrier_params {
    float vmax;           /* bound of the loop's frequency term, half-turns per output */
    float gamma;          /* the lock metric's smoothing                  */
    float lock_thr;       /* locked: q < lock_thr                         */
} pddc_carrier_params;
typedef struct pddc_carrier_rx {
    int mode;             /* PDDC_CARRIER_OFF / _DSB / _USB / _LSB        */
    float kp;             /* proportional gain, (0, 0.5]                  */
    float ki;             /* integral gain, [0, 0.25]                     */
} pddc_carrier_rx;
typedef struct pddc_carrier_status {
    uint32_t theta;       /* the NCO word behind the last output          */
    float freq;           /* v: offset = freq rate / 2 Hz                 */
    float err;            /* q: smoothed |e|                              */
    uint32_t locked;      /* q < lock_thr                                 */
} pddc_carrier_status;
typedef struct pddc_carrier pddc_carrier;
int pddc_carrier_create(pddc_carrier **out, int device, int nrx, const pddc_carrier_params *params,
                        const pddc_carrier_rx *rx /* [nrx], copied */, const float *hilbert /* [ntaps], copied */,
                        int ntaps);
int pddc_carrier_destroy(pddc_carrier *c);
int pddc_carrier_reset(pddc_carrier *c);              /* m and everything carried; synchronises the device */
int pddc_carrier_set_rx(pddc_carrier *c, int rx, int mode, float kp, float ki);
int pddc_carrier_process(pddc_carrier *c, const void *d_z, size_t n, size_t z_stride, void *d_u, size_t u_stride,
                         void *stream);
int pddc_carrier_read(pddc_carrier *c, pddc_carrier_status *host /* [nrx] */, void *stream);
/* outputs per tile of the kernel's walk and receivers per block (for tests that place batch cuts and K on its seams) */
int pddc_carrier_tile_outputs(void);
int pddc_carrier_group(void);

/* ---- squelch: per-receiver level meter and gated audio ------------------------
 * A stage between the demodulator and audio.  Per batch it reads the receivers' complex series
 * z_j[m] (the rows the demodulator reads) and their audio a_j[m] (the demodulator's output at the
 * same m) and gives the gated audio out_j[m], per completed metering block a level and an open /
 * closed state, and on request a status per receiver.  m counts samples since create / reset and
 * goes on across batches.  All arithmetic is float32 with floating-point contraction off, the same
 * operation sequence for every caller and every cut.
 * Fixed at create, common to all receivers: nrx (1 .. 1024); B, the block length in samples
 * (1 .. 4096); attack and hang, the consecutive blocks to open and to close (1 .. 65535 each); R, the
 * ramp length in samples (1 .. 65536); up, the noise floor's rise per block (finite, >= 1).
 * invB = 1.0f / (float)B and invR = 1.0f / (float)R, one correctly rounded division each.
 * Per receiver, changeable between batches with set_rx: open_thr and close_thr, finite,
 * 0 <= close_thr <= open_thr; flags, a subset of PDDC_SQL_GATE | PDDC_SQL_RELATIVE.
 * Carried per receiver, with the values at create / reset: the partial sum s = 0, the floor
 * f = +inf, level = 0, peak = 0, open = 0, run = 0, opens = 0 (uint32 both), the ramp counter c = 0
 * with GATE, else R.  The object carries the sample count N (uint64).
 * Per sample m, in order:
 *   1. p = (re re) + (im im); s = s + p.
 *   2. the target is R if open or GATE is not set, else 0; towards R: c = min(c + 1, R), towards 0:
 *      c = max(c - 1, 0).
 *   3. c == R: out = a (g = 1.0f: a's bits pass unchanged); c == 0: out = +0.0f whatever a is;
 *      otherwise g = (float)c invR and out = a g.
 * At the end of a block, after the sample with (m + 1) mod B == 0, in order:
 *   1. L = s invB; s = 0.
 *   2. if !open: f = fminf(L, f up) -- the floor is frozen while open.
 *   3. with RELATIVE: to = f open_thr, tc = f close_thr; without: the thresholds themselves.
 *   4. if !open: run = (L >= to) ? run + 1 : 0; on run >= attack: open = 1, run = 0, ++opens.
 *   5. else: run = !(L >= tc) ? run + 1 : 0; on run >= hang: open = 0, run = 0.
 *   6. peak = fmaxf(peak, L); level = L.
 * The decision of block k governs the target from the first sample of block k + 1: no look-ahead,
 * no added delay.
 * set_rx(j, open_thr, close_thr, flags): the thresholds take effect from the next block end, the
 * flags from the next sample; nothing carried is reset.  An unknown flag, thresholds out of order or
 * not finite, j outside [0, nrx): PDDC_EINVAL, nothing changed.
 * The bits of every output and every carried value depend on the receiver's two series, its
 * threshold and flag history and the create parameters alone: not on the cut into batches (batches of
 * 0 and of fewer than B samples included), nrx, j's index, the other receivers, strides, grid or tile
 * sizes.
 * Non-finite samples, in the receiver's own row alone.  In a: out = a g wherever c > 0, so a NaN or an infinity
 * passes (inf g is inf); with c == 0 out is +0.0f whatever a is.  Nothing is carried.  In z: the block's level is NaN
 * or inf.  A NaN level: every comparison with it is false -- closed, the run towards attack restarts; open, the block
 * counts towards hang --, fminf and fmaxf drop it from f and peak, level reads NaN until the next block.  An infinite
 * level counts as a loud block; peak = inf from then on: sticky by definition, until read(clear_peak).  level and f
 * heal by themselves with the next block: the caller does nothing.
 * process(): z is [nrx][z_stride] complex float32, a [nrx][a_stride] and out [nrx][out_stride]
 * float32, n values used per row; d_level float32 and d_state uint8, [nrx][blk_stride] each or NULL,
 * get *blocks = floor((N + n) / B) - floor(N / B) values per row: entry k of a row belongs to the
 * k-th block completed in this batch, the level L and `open` after the decision.  Every argument is
 * checked before anything is queued: PDDC_EINVAL for a NULL (z, a, out) or misaligned (8 / 4 / 4 /
 * 4 / 1 bytes) pointer with work to do, PDDC_ECAPACITY when a stride is below what the row must
 * hold; d_out == d_a with equal strides is allowed (gating in place), any other overlap of out with
 * a or z is PDDC_EINVAL; n = 0 is valid and does nothing.  State moves only after the launch was
 * accepted.  Stream-ordered; one stream per object, one thread at a time.
 * read(): the status of every receiver after the batches submitted so far (it waits for them);
 * clear_peak: peak restarts at 0 for the blocks that complete after the call.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_SQL_GATE      0x1u
#define PDDC_SQL_RELATIVE  0x2u
typedef struct pddc_squelch_params {
    int block;            /* B: samples per metering block                */
    int attack;           /* consecutive blocks at or above open to open  */
    int hang;             /* consecutive blocks below close to close      */
    int ramp;             /* R: samples of the gain ramp                  */
    float up;             /* the floor's rise per block while closed      */
} pddc_squelch_params;
typedef struct pddc_squelch_rx {
    float open_thr;
    float close_thr;
    uint32_t flags;       /* PDDC_SQL_GATE | PDDC_SQL_RELATIVE            */
} pddc_squelch_rx;
typedef struct pddc_squelch_status {
    float level, floor, peak;
    uint32_t open, opens;
} pddc_squelch_status;
typedef struct pddc_squelch pddc_squelch;
int pddc_squelch_create(pddc_squelch **out, int device, int nrx, const pddc_squelch_params *params,
                        const pddc_squelch_rx *rx /* [nrx], copied */);
int pddc_squelch_destroy(pddc_squelch *s);
int pddc_squelch_reset(pddc_squelch *s);              /* N and everything carried; synchronises the device */
int pddc_squelch_set_rx(pddc_squelch *s, int rx, float open_thr, float close_thr, uint32_t flags);
int pddc_squelch_process(pddc_squelch *s, const void *d_z, const void *d_a, size_t n, size_t z_stride, size_t a_stride,
                         void *d_out, size_t out_stride, void *d_level /* float [nrx][blk_stride] or NULL */,
                         void *d_state /* uint8 [nrx][blk_stride] or NULL */, size_t blk_stride, size_t *blocks,
                         void *stream);
/* blocks per receiver the next process() of n samples completes (host arithmetic) */
int pddc_squelch_next_blocks(const pddc_squelch *s, size_t n, size_t *count);
/* the same without an object (host arithmetic, no device): floor((before + n) / B) - floor(before / B);
 * 0 for B outside 1 .. 4096 */
uint64_t pddc_squelch_blocks(int block, uint64_t samples_before, size_t n);
int pddc_squelch_read(pddc_squelch *s, pddc_squelch_status *host /* [nrx] */, int clear_peak, void *stream);
/* samples per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_squelch_tile_outputs(void);

/* ---- adapt: automatic notch and noise reduction per receiver -------------------
 * A stage between the squelch (or the demodulator) and audio: an adaptive line enhancer, a leaky
 * normalised LMS predictor over a delayed copy of the audio.  Per batch it reads the receivers' real
 * float32 series x_j[m] (the rows the demodulator and the squelch write) and gives out_j[m]: the
 * prediction (noise reduction: what is predictable stays), the prediction error (notch: a carrier
 * whistle goes) or x itself.  m counts samples since create / reset and goes on across batches;
 * x[m] = 0 for m < 0.  All arithmetic is float32 with floating-point contraction off, every division
 * the correctly rounded one, denormals kept, the same operation sequence for every caller and cut.
 * Fixed at create, common to all receivers: nrx (1 .. 1024); T taps (16, 32, 64 or 128); the delay
 * D (1 .. 256); eps (finite, > 0).
 * Per receiver, changeable between batches with set_rx: mode, PDDC_ADAPT_OFF / _NR / _NOTCH; the
 * step mu, 0 < mu < 2; the leak, 0 <= leak < 1, from which lam = 1.0f - leak, one float32
 * subtraction.  All finite.
 * Carried per receiver: the weights w_0 .. w_(T-1), 0 at create / reset, and its last D + T - 1
 * inputs.  Nothing else.
 * The tree sum of T values v_0 .. v_(T-1): for h = T/2, T/4, .. 1: v_k = v_k + v_(k+h) for k < h;
 * the sum is v_0.
 * Per sample m, with u_k = x[m - D - k], k = 0 .. T-1, in order:
 *   1. y = tree sum of (w_k u_k); P = tree sum of (u_k u_k).
 *   2. e = x[m] - y.
 *   3. g = (mu e) / (P + eps).
 *   4. unless OFF: w_k = (w_k lam) + (g u_k) for every k.
 *   5. out = y with NR, e with NOTCH; with OFF out has the bits of x[m] and the weights are not
 *      touched -- the inputs go on being carried, so a receiver switched on again resumes with the
 *      weights it held.
 * set_rx(j, mode, mu, leak, flags): from the next sample on; the weights are kept unless flags has
 * PDDC_ADAPT_RESTART, which takes that receiver's weights as 0 from the next sample on (a mark the
 * next batch with n > 0 honours; nothing on the device is cleared from the host).  A mode, step,
 * leak or flag outside the above, not finite, j outside [0, nrx): PDDC_EINVAL, nothing changed.
 * The bits of every output and every weight depend on the receiver's series, its set_rx history, T,
 * D and eps alone: not on the cut into batches (batches of 0 included), nrx, j's index, the other
 * receivers, strides, grid or tile sizes.
 * Non-finite samples, in the receiver's own row alone: sticky.  A NaN, an infinity or a value whose square overflows
 * (1e25) in x[p] makes g, and with it every weight, NaN or infinite at the latest when the sample enters the window
 * (sample p + D); weights that are not finite stay so, w lam + g u has no way back, and every NR / NOTCH output after
 * that is not finite.  OFF passes x and holds its weights.  RESTART zeroes the weights only: the sample is still in
 * the carried inputs for D + T - 1 samples and poisons them again.  So the caller feeds D + T - 1 good samples and
 * then calls set_rx with PDDC_ADAPT_RESTART -- from that sample on the row is that of a receiver restarted there on
 * the good series --, or calls reset.
 * process(): a is [nrx][a_stride] and out [nrx][out_stride] float32, n values used per row.  Every
 * argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned (4 bytes)
 * pointer with work to do, PDDC_ECAPACITY when a stride is below n; d_out == d_a with equal strides
 * is allowed (in place), any other overlap of out with a is PDDC_EINVAL; n = 0 is valid and does
 * nothing.  State moves only after the launch was accepted.  Stream-ordered; one stream per object,
 * one thread at a time.
 * read_weights(): the weights [nrx][T] as the last accepted batch left them (it waits for it): the
 * predictor's impulse response, from which a display draws the notch's frequency response.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_ADAPT_OFF     0u
#define PDDC_ADAPT_NR      1u
#define PDDC_ADAPT_NOTCH   2u
#define PDDC_ADAPT_RESTART 0x1u
typedef struct pddc_adapt_params {
    int taps;             /* T: 16, 32, 64 or 128                         */
    int delay;            /* D: 1 .. 256                                  */
    float eps;            /* added to the power before the division       */
} pddc_adapt_params;
typedef struct pddc_adapt_rx {
    uint32_t mode;        /* PDDC_ADAPT_OFF, _NR, _NOTCH                  */
    float mu;             /* step, 0 < mu < 2                             */
    float leak;           /* 0 <= leak < 1                                */
    uint32_t flags;       /* PDDC_ADAPT_RESTART (set_rx)                  */
} pddc_adapt_rx;
typedef struct pddc_adapt pddc_adapt;
int pddc_adapt_create(pddc_adapt **out, int device, int nrx, const pddc_adapt_params *params,
                      const pddc_adapt_rx *rx /* [nrx], copied */);
int pddc_adapt_destroy(pddc_adapt *s);
int pddc_adapt_reset(pddc_adapt *s);                  /* everything carried; synchronises the device */
int pddc_adapt_set_rx(pddc_adapt *s, int rx, uint32_t mode, float mu, float leak, uint32_t flags);
int pddc_adapt_process(pddc_adapt *s, const void *d_a, size_t n, size_t a_stride, void *d_out, size_t out_stride,
                       void *stream);
int pddc_adapt_read_weights(pddc_adapt *s, float *host /* [nrx][taps] */, void *stream);
/* samples per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_adapt_tile_outputs(void);

/* ---- denoise: spectral noise reduction per receiver ---------------------------
 * A stage where adapt sits: behind the demodulator, the squelch or the adaptive filter, in front of
 * audio.  Short-time transform, a noise estimate and a gain per bin, overlap-add.  Per batch it reads
 * the receivers' real float32 rows x_j[m] and writes out_j[m], n values out per n values in, delayed
 * by exactly nfft samples.  m counts samples since create / reset and goes on across batches;
 * x[m] = 0 for m < 0.
 * Fixed at create, common to all receivers: nrx (1 .. 1024); nfft (256, 512 or 1024); hop (nfft/2 or
 * nfft/4), R = nfft / hop; a window w[nfft] (the caller's, finite, copied; used for analysis and
 * synthesis); the tracker's constants: smooth a, up, down, each in (0, 1]; nmin in [0, 1]; eps,
 * finite and > 0.
 * Per receiver, changeable between batches with set_rx: mode PDDC_DENOISE_OFF or _NR; the
 * over-subtraction beta, finite and > 0; the gain floor gmin in [0, 1]; the decision-directed weight
 * alpha in [0, 1); flags: PDDC_DENOISE_RESTART, one-shot: the next completed frame is a first frame;
 * PDDC_DENOISE_HOLD, lasting until a set_rx without it: S and N are not updated (a "noise profile").
 * A set_rx governs every frame whose last sample arrives in a later batch.  A value outside the
 * above, not finite, rx outside [0, nrx): PDDC_EINVAL, nothing changed.
 * Frames: frame q >= 0 holds the inputs m = (q+1) hop - nfft .. (q+1) hop - 1 and is complete once
 * (q+1) hop samples have arrived.  B = nfft/2 + 1 bins.
 * Per completed frame and bin k, in this order; all arithmetic outside the two transforms is float32
 * with contraction off, every division the correctly rounded one, comparisons as written:
 *    1. f[i] = x[..] w[i]; X_k the forward transform of f.
 *    2. P = re re + im im.
 *    3. first frame (after create, reset or RESTART): S = P, N = P, A = 0.
 *    4. otherwise, unless HOLD: S = S + a (P - S); if S > N: r = N + up N; r2 = nmin S; if r < r2
 *       then r = r2; N = (r < S) ? r : S; else N = N + down (S - N).  (A smoothed periodogram and a
 *       minimum tracker: it falls at `down`, rises by at most the factor 1 + up per frame and is
 *       never more than nmin below S.)
 *    5. Nb = beta N + eps.
 *    6. t = P / Nb - 1.
 *    7. xi = alpha (A / Nb) + (1 - alpha) (t > 0 ? t : 0).
 *    8. g = xi / (1 + xi).
 *    9. G = (g > gmin) ? g : gmin.
 *   10. with OFF, G = 1: S and N go on being tracked, so switching on is seamless (OFF is unity gain
 *       through the transforms, not a copy).
 *   11. A = (G G) P.
 *   12. Y_k = G X_k.
 *   13. s = the inverse real transform of Y, scaled 1/nfft; the frame's term is t_q[i] = s[i] w[i].
 * Overlap-add: y[m] = sum of t_q[i] over the frames that hold m, added in ascending q starting from
 * the first term itself (at most R terms); out[m] = y[m - nfft], and 0 for m < nfft.  With this delay
 * every value a batch emits is final however the batch is cut: out[m] needs frame floor(m / hop) - 1,
 * which is complete before x[m] arrives.
 * Carried per receiver: the inputs since the start of the oldest incomplete frame, the partial
 * overlap sums, the finished y not yet emitted, S, N, A per bin, the first-frame mark.  Nothing else.
 * The bits of every output and every N depend on the receiver's series, its set_rx history (in sample
 * positions) and the create-time parameters alone: not on the cut into batches (batches of 0 and
 * batches that complete no frame included), nrx, the row's index, the other receivers, strides, grid
 * or tile sizes.  A frame's transform is a function of that frame's own nfft values alone.
 * Non-finite samples, in the receiver's own row alone (other rows keep their bits): a NaN, an
 * infinity or a value whose square overflows (1e25) in x[p] makes P NaN or infinite in every bin of
 * the R frames that hold it (where w is not 0 at its place).  Those frames' terms, and the outputs
 * they reach, are NaN or infinite (for the overflowing square finite, of the sample's size).  S, and
 * with it N, is NaN at the latest one frame later: S + a (P - S) and both branches of the tracker have
 * no way back, so N stays NaN (read_noise shows it) when good samples follow.  Every comparison with a
 * NaN is false, so from the first good frame on g > gmin fails in every bin and G = gmin: the output
 * is finite again, the input through the floor gain (through 1 with OFF), for as long as N is NaN.
 * Under HOLD S and N are not touched and A alone is lost, for one frame.  Recovery: the caller feeds
 * nfft good samples and then calls set_rx with PDDC_DENOISE_RESTART; the next completed frame q holds
 * good samples only and is a first frame, and from out index q hop + nfft on (once the overlap has
 * drained) the row is that of a receiver restarted there on the good series.  Or reset.  What
 * counts is that frame alone: a RESTART whose next completed frame still holds the bad sample makes
 * a first frame of it, S = N = P is NaN, and N is NaN again.
 * process(): x is [nrx][x_stride] and out [nrx][out_stride] float32, n values used per row.  Every
 * argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned (4 bytes)
 * pointer with work to do, PDDC_ECAPACITY when a stride is below n; in place is not offered: any
 * overlap of out with x is PDDC_EINVAL; n = 0 is valid and does nothing.  State moves only after the
 * launch was accepted.  Stream-ordered; one stream per object, one thread at a time.
 * read_noise(): N [nrx][B] as the last accepted batch left it (it waits for it); zeros before the
 * first completed frame.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_DENOISE_OFF     0u
#define PDDC_DENOISE_NR      1u
#define PDDC_DENOISE_RESTART 0x1u
#define PDDC_DENOISE_HOLD    0x2u
typedef struct pddc_denoise_params {
    int nfft;             /* 256, 512 or 1024                             */
    int hop;              /* nfft/2 or nfft/4                             */
    float smooth;         /* a: the periodogram's smoothing, (0, 1]       */
    float up;             /* the tracker's rise per frame, (0, 1]         */
    float down;           /* the tracker's fall, (0, 1]                   */
    float nmin;           /* N >= nmin S while it rises, [0, 1]           */
    float eps;            /* added to beta N before the divisions         */
} pddc_denoise_params;
typedef struct pddc_denoise_rx {
    uint32_t mode;        /* PDDC_DENOISE_OFF, _NR                        */
    float beta;           /* over-subtraction, > 0                        */
    float gmin;           /* gain floor, 0 .. 1                           */
    float alpha;          /* decision-directed weight, 0 <= alpha < 1     */
    uint32_t flags;       /* PDDC_DENOISE_HOLD; _RESTART (set_rx)         */
} pddc_denoise_rx;
typedef struct pddc_denoise pddc_denoise;
int pddc_denoise_create(pddc_denoise **out, int device, int nrx, const pddc_denoise_params *params,
                        const float *window /* [nfft], copied */, const pddc_denoise_rx *rx /* [nrx], copied */);
int pddc_denoise_destroy(pddc_denoise *s);
int pddc_denoise_reset(pddc_denoise *s);              /* everything carried; synchronises the device */
int pddc_denoise_set_rx(pddc_denoise *s, int rx, uint32_t mode, float beta, float gmin, float alpha, uint32_t flags);
int pddc_denoise_process(pddc_denoise *s, const void *d_x, size_t n, size_t x_stride, void *d_out, size_t out_stride,
                         void *stream);
int pddc_denoise_read_noise(pddc_denoise *s, float *host /* [nrx][nfft/2 + 1] */, void *stream);
/* the delay in samples: nfft (host arithmetic, no device); 0 for an nfft that is none of the three */
int pddc_denoise_delay(int nfft);
/* frames of one block pass of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_denoise_tile_frames(void);

/* ---- eq: per-receiver biquad cascades over the audio ---------------------------
 * A stage behind the demodulator, the squelch, the adaptive filter or the noise reduction and in
 * front of audio (it works behind audio, at 48 kHz, as well): per receiver a cascade of second-order
 * sections that shapes the audio itself -- de-emphasis, an audio peak filter, a manual notch, hum
 * notches, bass and treble, high and low cut.  Per batch it reads the receivers' real float32 series
 * x_j[m] and gives out_j[m], n values out per n values in, no delay.
 * All arithmetic is binary64: coefficients, states and every operation; input and output stay
 * float32.  (A float32 cascade of a 20 Hz notch of Q 30 leaves a noise floor 63 dB below the
 * output's peak; the binary64 cascade rounded once is within half a float32 ulp.)
 * Fixed at create: nrx (1 .. 1024); S, the sections a receiver can have (1, 2, 4 or 8).
 * Per receiver, changeable between batches with set_rx: nsec, 0 .. S, and nsec sections (b0, b1, b2,
 * a1, a2), a0 = 1.  Each section must be stable: all five values finite, |a2| < 1 and
 * |a1| < 1 + a2; a section that is not, nsec outside 0 .. S, an unknown flag, rx outside [0, nrx):
 * PDDC_EINVAL with a message that names the section, nothing changed.
 * Carried per receiver and section: two binary64 states s1, s2, 0 at create, reset and RESTART.
 * Nothing else.
 * Per sample m: v = (double)x[m]; for s = 0 .. nsec - 1, in this order:
 *     y  = (b0 v) + s1
 *     s1 = ((b1 v) - (a1 y)) + s2
 *     s2 = (b2 v) - (a2 y)
 *     v  = y
 * every product and sum a separately rounded IEEE operation (no contraction, denormals kept): the
 * transposed direct form II in the operation sequence of scipy.signal.sosfilt; out[m] = (float)v,
 * rounded to nearest even.
 * nsec = 0 is OFF: the output words are the input words, copied as 32-bit words without a
 * conversion (-0.0 and NaN payloads survive).
 * Sections s >= nsec are not run; a batch with n > 0 leaves their states 0, so a cascade that grows
 * later starts those sections from rest.
 * set_rx(j, nsec, sections, flags): from the next sample on, and the states are KEPT: no gap, the
 * transient is the filter's own.  With PDDC_EQ_RESTART that receiver's states are taken as 0 (a mark
 * the next batch with n > 0 honours; nothing on the device is cleared from the host).
 * The bits of every output and every state depend on the receiver's series and its set_rx history
 * alone: not on the cut into batches (batches of 0 included), nrx, j's index, the other receivers,
 * S, strides, grid or tile sizes.  The same receiver in an S = 2 and an S = 8 object gives the same
 * bits.
 * Non-finite samples, in the receiver's own row alone (other rows keep their bits): sticky.  A NaN
 * or an infinity in x[p] makes that receiver's states NaN or infinite from sample p on (an infinity
 * turns NaN in s1 = (b1 v) - (a1 y) + s2 at the latest one sample later), states that are not finite
 * stay so -- the recursion has no way back -- and every output after it is not finite.  OFF passes
 * the words and has no states.  Recovery: set_rx with PDDC_EQ_RESTART in front of the first batch of
 * good samples -- from that sample on the row is that of a receiver restarted there --, or reset.
 * process(): a is [nrx][a_stride] and out [nrx][out_stride] float32, n values used per row.  Every
 * argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned (4 bytes)
 * pointer with work to do, PDDC_ECAPACITY when a stride is below n; d_out == d_a with equal strides
 * is allowed (in place), any other overlap of out with a is PDDC_EINVAL; n = 0 is valid and does
 * nothing.  State moves only after the launch was accepted.  Stream-ordered; one stream per object,
 * one thread at a time.
 * read_state(): s1, s2 [nrx][S][2] as the last accepted batch left them (it waits for it).
 * design(): one section in double (host arithmetic, no device): the RBJ cookbook's LOWPASS, HIGHPASS,
 * BANDPASS (0 dB peak), NOTCH, PEAK (gain_db at f), LOWSHELF and HIGHSHELF (gain_db at the far end; q
 * is the shelf's Q), and the one-pole LOWPASS1 / HIGHPASS1 through the bilinear transform (b2 = a2 =
 * 0, half power at f_hz; q and gain_db are not used).  De-emphasis with the time constant tau is
 * LOWPASS1 at 1 / (2 pi tau).  f_hz outside (0, rate_hz / 2), q <= 0, anything not finite, an unknown
 * kind, or a result that fails the stability test: PDDC_EINVAL.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_EQ_MAX_SECTIONS 8
#define PDDC_EQ_RESTART      0x1u
#define PDDC_EQ_LOWPASS      0
#define PDDC_EQ_HIGHPASS     1
#define PDDC_EQ_BANDPASS     2
#define PDDC_EQ_NOTCH        3
#define PDDC_EQ_PEAK         4
#define PDDC_EQ_LOWSHELF     5
#define PDDC_EQ_HIGHSHELF    6
#define PDDC_EQ_LOWPASS1     7
#define PDDC_EQ_HIGHPASS1    8
typedef struct pddc_eq_section {
    double b0, b1, b2, a1, a2;   /* a0 = 1                               */
} pddc_eq_section;
typedef struct pddc_eq_params {
    int sections;         /* S: 1, 2, 4 or 8                              */
} pddc_eq_params;
typedef struct pddc_eq pddc_eq;
int pddc_eq_create(pddc_eq **out, int device, int nrx, const pddc_eq_params *params, const int *nsec /* [nrx] */,
                   const pddc_eq_section *sec /* [nrx][S], copied; receiver j's first nsec[j] are read */);
int pddc_eq_destroy(pddc_eq *s);
int pddc_eq_reset(pddc_eq *s);                        /* everything carried; synchronises the device */
int pddc_eq_set_rx(pddc_eq *s, int rx, int nsec, const pddc_eq_section *sec /* [nsec]; NULL with nsec 0 */,
                   uint32_t flags);
int pddc_eq_process(pddc_eq *s, const void *d_a, size_t n, size_t a_stride, void *d_out, size_t out_stride,
                    void *stream);
int pddc_eq_read_state(pddc_eq *s, double *host /* [nrx][S][2] */, void *stream);
/* samples per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_eq_tile_outputs(void);
int pddc_eq_design(int kind, double rate_hz, double f_hz, double q, double gain_db, pddc_eq_section *out);

/* ---- blanker: impulse noise blanker per receiver ------------------------------
 * A stage between the tuner and the receiver filter, the only place where an impulse is still a few
 * samples long.  Per batch it reads the receivers' complex float32 rows z_j[m] (the tuner's output
 * view, whose stride is its capacity) and gives out_j[m]: the same series delayed by D samples, with
 * the neighbourhood of every detected impulse taken to zero through a linear ramp.  m counts input
 * samples since create / reset and goes on across batches; z[m] = 0 for m < 0.  All arithmetic is
 * float32 with floating-point contraction off, the same operation sequence for every caller and cut.
 * Fixed at create, common to all receivers: nrx (1 .. 1024); B, samples per metering block
 * (1 .. 4096); W, the guard half-width (0 .. 128); R, the ramp length (0 .. 128); beta, the
 * reference's smoothing (finite, 0 < beta <= 1); cap, the reference's largest rise per block (finite,
 * >= 1).  D = W + R (0 .. 256); invB = 1.0f / (float)B and invR1 = 1.0f / (float)(R + 1), one
 * correctly rounded division each.
 * Per receiver, changeable between batches with set_rx: thr, finite and > 0, a power ratio; flags, a
 * subset of PDDC_NB_ON.
 * Carried per receiver, with the values at create / reset: the partial sum s = 0, the reference
 * ref = 0, the counters triggers = 0 and blanked = 0 (uint32, modulo 2^32), the last D inputs and the
 * trigger bits of the last 2 D inputs (all clear).  The object carries the sample count N (uint64).
 * Per input sample m, in order:
 *   1. p = (re re) + (im im); s = s + p.
 *   2. t[m] = ON && (ref > 0) && (p > ref thr): the product is one float32 multiply, ref the value
 *      after the last completed block, a comparison with a NaN is false.  On t[m]: ++triggers.
 *   3. after the sample with (m + 1) mod B == 0: L = s invB; s = 0; if ref > 0: x = fminf(L, ref cap),
 *      d = x - ref, ref = ref + (beta d); otherwise ref = L.  There are no other special cases: what a
 *      non-finite input does follows from these operations.
 * The gate, for every m (m < 0 included): dist[m] is the smallest |m - u| over all u with t[u] set and
 * |m - u| <= D; g = 0 when dist <= W; g = (float)(dist - W) invR1 when W < dist <= D; g = 1 when no
 * trigger is that near.
 * Output n, one per input, at the same index of the batch: c = n - D; with g[c] == 1 out has the bits
 * of z[c] (+0 + 0i for c < 0); with g[c] == 0 both parts are +0.0f whatever z is; otherwise
 * out.re = re g and out.im = im g, one multiply each.  ++blanked for every output with g[c] != 1.
 * A trigger at u touches outputs u .. u + 2 D only, so everything is causal.  The last D inputs of a
 * stream come out when the caller feeds D more samples: there is no flush call.
 * set_rx(j, thr, flags): from the next input sample on; nothing carried is reset -- triggers already
 * taken stay, and receivers that are off go on being metered and delayed.  An unknown flag, a thr that
 * is not finite or <= 0, j outside [0, nrx): PDDC_EINVAL, nothing changed.
 * The bits of every output, of ref and of the counters depend on the receiver's series, its set_rx
 * history and the create parameters alone: not on the cut into batches (batches of 0, of fewer than D
 * and of fewer than B samples included), nrx, j's index, the other receivers, strides, grid or tile
 * sizes.
 * Non-finite samples, in the receiver's own row alone: healing.  A NaN sample does not trigger (p > ref thr is
 * false) and comes out as it is, D samples later, unless a neighbouring trigger blanks it (+0.0f whatever z is); an
 * infinite one, or one whose square overflows, triggers (once ref > 0) and is blanked with its neighbourhood, 2 D + 1
 * finite outputs.
 * The block it lies in has L = NaN or inf: with ref > 0, x = fminf(L, ref cap) = ref cap and ref rises by its largest
 * step; in the first block (ref = 0) ref = L itself, then NaN for one block (inf - inf), then `ref > 0` is false and
 * ref starts again from the next block's L.  ref is finite again within three blocks: the caller does nothing.
 * process(): z is [nrx][z_stride] and out [nrx][out_stride] complex float32, n values used per row.
 * Every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned (8 bytes)
 * pointer with work to do, PDDC_ECAPACITY when a stride is below n; ANY overlap of out with z is
 * PDDC_EINVAL -- there is no in-place form, out[n] is made from z[n - D]; n = 0 is valid and does
 * nothing.  State moves only after the launch was accepted.  Stream-ordered; one stream per object,
 * one thread at a time.
 * read(): ref and the counters of every receiver after the batches submitted so far (it waits for
 * them).
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_NB_ON 0x1u
typedef struct pddc_blanker_params {
    int block;            /* B: samples per metering block                */
    int guard;            /* W: samples zeroed on either side of a trigger */
    int ramp;             /* R: samples of the ramp on either side        */
    float beta;           /* the reference's smoothing per block          */
    float cap;            /* the reference's largest rise per block       */
} pddc_blanker_params;
typedef struct pddc_blanker_rx {
    float thr;            /* trigger at p > ref thr                       */
    uint32_t flags;       /* PDDC_NB_ON                                   */
} pddc_blanker_rx;
typedef struct pddc_blanker_status {
    float ref;
    uint32_t triggers, blanked;
} pddc_blanker_status;
typedef struct pddc_blanker pddc_blanker;
int pddc_blanker_create(pddc_blanker **out, int device, int nrx, const pddc_blanker_params *params,
                        const pddc_blanker_rx *rx /* [nrx], copied */);
int pddc_blanker_destroy(pddc_blanker *b);
int pddc_blanker_reset(pddc_blanker *b);              /* N and everything carried; synchronises the device */
int pddc_blanker_set_rx(pddc_blanker *b, int rx, float thr, uint32_t flags);
int pddc_blanker_process(pddc_blanker *b, const void *d_z, size_t n, size_t z_stride, void *d_out, size_t out_stride,
                         void *stream);
int pddc_blanker_read(pddc_blanker *b, pddc_blanker_status *host /* [nrx] */, void *stream);
/* D = W + R: output n is input n - D */
int pddc_blanker_delay(const pddc_blanker *b);
/* samples per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_blanker_tile_outputs(void);

/* ---- wblank: impulse blanking on the packed ADC stream ------------------------
 * A stage in front of everything that reads the packed 24-bit stream (pipeline, bank, panorama,
 * channelizer): packed samples in, packed samples out, so none of them changes.  At the full ADC
 * bandwidth an impulse is 1 - 3 samples long and is cut with a few dozen samples lost; behind the
 * channelizer and the tuner it has their filters' length and is in every receiver.
 * Everything is integer arithmetic: every output bit and every counter depends on the stream, the
 * create parameters and the set() history alone, not on the cut into batches, grid, tile or run.
 * Samples: I[m], Q[m] are the 24-bit codes in [-2^23, 2^23) (pddc_unpack24_i32 >> 8, arithmetic); m
 * counts input samples since create / reset (uint64 N is carried).  p[m] = I^2 + Q^2, uint64, at
 * most 2^47.
 * Fixed at create: B, samples per metering block, a power of two 64 .. 4096, b = log2 B; H, blocks
 * of history, 1 .. 16; W, the guard half-width, 0 .. 128; r, the ramp exponent, 0 .. 7, the ramp
 * length is R = 2^r - 1; D = W + R, at most 255.
 * Changeable between batches with set(thr16, flags): thr16, the threshold as a power ratio in
 * sixteenths, 16 .. 65536; flags, a subset of PDDC_WB_ON.  A change applies from the next input
 * sample on, decisions already taken stay; a bad value is PDDC_EINVAL and changes nothing.
 * Metering: block k covers samples [k B, (k + 1) B), S_k is the sum of p over it (at most 2^59);
 * the block grid belongs to the stream.  For k >= 1: mean_k = (the least S_j, j = max(0, k - H) ..
 * k - 1) >> b; mean_0 = 0.  The minimum keeps the impulses themselves, and a signal keying on, out
 * of the reference.
 * Trigger, m in block k: t[m] = ON && mean_k > 0 && p[m] > ((mean_k thr16) >> 4); the product is at
 * most 2^63.
 * Gate, as the per-receiver blanker's: dist[m] is the least |m - u| over u with t[u] set and
 * |m - u| <= D; num = 0 when dist <= W, num = dist - W when W < dist <= D, "open" when no trigger is
 * that near.
 * Output n of the stream is made from input c = n - D, one per input, at the same index of the
 * batch: six zero bytes for c < 0; open: the six input bytes of sample c unchanged; otherwise I and
 * Q each become sign(v) ((|v| num) >> r), packed again (toward zero, no DC added, |v| num < 2^31).
 * The last D inputs of a stream come out when D more are fed: there is no flush call.
 * Carried: N, the open block's partial sum, the last H block sums, the last 2 D inputs (rounded up
 * to 8) with their trigger bits -- the bits are kept, not taken again, since the threshold may have
 * changed --, the counters.
 * read(): after the batches submitted so far (it waits for them): mean, the reference of the block
 * the next input sample falls into; triggers, the t[m] set; blanked, the outputs made from an input
 * (c >= 0) whose gate was not open; samples = N.
 * process(): d_packed holds nsamples packed samples, d_out takes exactly nsamples.  Checked before
 * anything is queued: nsamples a multiple of 8, both pointers 16-byte aligned and not NULL with
 * work to do, ANY overlap of out and in is PDDC_EINVAL -- there is no in-place form, a workgroup
 * reads D samples beyond what it writes.  nsamples = 0 is valid and does nothing; batches shorter
 * than D or B samples are valid.  The object moves only after the last launch was accepted: a batch
 * of more than 2^26 samples goes in rounds of 2^26, and no round writes what the object holds.
 * Stream-ordered, no allocation and no synchronisation; one stream per object, one thread at a time.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV.
 * The "wblank_run" knob of pddc_set_tunable sets the samples one workgroup walks (0: automatic). */
#define PDDC_WB_ON 0x1u
typedef struct pddc_wblank_params {
    int block;            /* B: samples per metering block                */
    int history;          /* H: block sums the reference is the least of  */
    int guard;            /* W: samples zeroed on either side of a trigger */
    int ramp_log2;        /* r: the ramp is 2^r - 1 samples on either side */
} pddc_wblank_params;
typedef struct pddc_wblank_status {
    uint64_t mean, triggers, blanked, samples;
} pddc_wblank_status;
typedef struct pddc_wblank pddc_wblank;
int pddc_wblank_create(pddc_wblank **out, int device, const pddc_wblank_params *params, uint32_t thr16, uint32_t flags);
int pddc_wblank_destroy(pddc_wblank *w);
int pddc_wblank_reset(pddc_wblank *w);                /* N and everything carried; synchronises the device */
int pddc_wblank_set(pddc_wblank *w, uint32_t thr16, uint32_t flags);
int pddc_wblank_process(pddc_wblank *w, const void *d_packed, size_t nsamples, void *d_out, void *stream);
int pddc_wblank_read(pddc_wblank *w, pddc_wblank_status *host, void *stream);
/* D = W + 2^r - 1: output n is input n - D */
int pddc_wblank_delay(const pddc_wblank *w);
/* samples per tile of the gate kernel's walk, and the samples one workgroup walks under the current "wblank_run" (one
 * tile when it is automatic): for tests that place batch cuts on the kernel's seams */
int pddc_wblank_tile_samples(void);
int pddc_wblank_run_samples(void);

/* ---- scope: each receiver's own spectrum and waterfall lines ------------------
 * Beside the chain, not in it: it reads any of the per-receiver complex float32 series -- the
 * tuner's, the blanker's or the receiver filter's output, in place, with their strides -- and writes
 * averaged power-spectrum lines per display slot.  It changes nothing it reads.
 * Input: z[r][i], complex float32, nsrc rows (1 .. 1024); i counts since create / reset and goes on
 * across batches; every process() supplies n new values of every row.
 * Slots: nslots display slots (1 .. 1024); slot j watches row[j], 0 <= row[j] < nsrc, or -1: off.
 * Several slots may watch one row.
 * Segments: segment s of slot j is the nfft values z[row[j]][s hop .. s hop + nfft - 1], each times
 * the caller's float32 window[nfft] (one multiply per part), transformed with an unnormalised forward
 * DFT in float32; p_s[k] = re^2 + im^2, float32, natural bin order.  The segment grid is global -- s
 * counts from sample 0 and is the same for every slot -- and a segment exists once its last sample is
 * in the stream: there is no zero padding.
 * Lines: line l is the sum of segments l A .. l A + A - 1, A = avg, added in float32 in ascending
 * segment order from the first segment's own value (the sum register starts at +0, and +0 + p has the
 * bits of p for every p = re^2 + im^2).  process() writes the lines that complete in this call to
 * lines[(j line_stride + m) nfft + k], float32, m counted from 0 in every call.  The count is the
 * same for all slots and follows from sizes alone: pddc_scope_next_lines(s, n); without an object
 * pddc_scope_lines(nfft, hop, avg, samples_before, n) (0 for sizes create refuses).  An off slot's
 * lines are written as zeros.
 * PDDC_SCOPE_CENTERED: position k holds bin (k + nfft/2) mod nfft, ascending frequency; the bits
 * are those without the flag, only the place changes.
 * Carried per slot, in two sets of device buffers used in turn: the samples from the start of the
 * first incomplete segment (fewer than nfft) and the partial sum of the line under way.  Nothing is
 * cleared from the host after create.
 * set_slot(j, row), between two batches: with the row the slot already has nothing changes; with
 * another the slot's carried samples and partial line return to their create values -- for that slot
 * the new row counts as zeros before the change -- while the grid and the line numbering go on.  A
 * slot outside [0, nslots) or a row outside [-1, nsrc): PDDC_EINVAL, nothing changed.
 * The bits of a line depend on the watched row's values, window, nfft, hop, avg and the slot's own
 * set_slot history alone: not on the cut into batches (n = 0 and n = 1 included), nslots, the slot's
 * index, the other slots, strides, grid or block sizes.  Every segment goes through the same
 * arithmetic sequence wherever it lies; one that begins in the carried samples is no exception.
 * Non-finite samples: transient.  A NaN in z[r][p] makes every bin of the segments that hold sample p NaN, and with
 * them the lines those segments go into, in the slots that watch row r; every other line and slot has the bits it has
 * without it.  Nothing is left behind once the sample has left the carried samples: the caller does nothing (set_slot
 * to another row, or reset, drops it at once).
 * Limits: nfft 256, 512, 1024, 2048 or 4096; nfft/16 <= hop <= nfft; 1 <= avg <= 4096; window
 * finite; flags 0 or PDDC_SCOPE_CENTERED.
 * process(): z is [nsrc][z_stride] complex float32 with n values used per row; *n_lines (may be NULL)
 * gets the lines written per slot.  Every argument is checked before anything is queued: PDDC_EINVAL
 * for a NULL or misaligned pointer (d_z: 8 bytes, with n > 0; d_lines: 16 bytes, and NULL only when
 * no line is due) and when the lines' bytes overlap z's; PDDC_ECAPACITY when z_stride < n, when
 * line_stride is below the lines due, or when a batch completes more lines than one launch holds
 * (nslots times lines above 2^31).  n = 0 is valid and does nothing.  State moves only after the
 * launch was accepted.  Stream-ordered; one stream per object, one thread at a time.
 * create: argument errors before any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_SCOPE_CENTERED 0x1u
typedef struct pddc_scope pddc_scope;
int pddc_scope_create(pddc_scope **out, int device, int nsrc, int nslots, const int *rows /* [nslots], copied */,
                      int nfft, int hop, int avg, const float *window /* [nfft], copied */, uint32_t flags);
int pddc_scope_destroy(pddc_scope *s);
int pddc_scope_reset(pddc_scope *s);                  /* the sample count and everything carried; the slots keep their rows; synchronises the device */
int pddc_scope_set_slot(pddc_scope *s, int slot, int row);
int pddc_scope_process(pddc_scope *s, const void *d_z, size_t n, size_t z_stride, void *d_lines, size_t line_stride,
                       size_t *n_lines, void *stream);
/* lines per slot the next process() of n samples writes */
uint64_t pddc_scope_next_lines(const pddc_scope *s, size_t n);
/* ... and of n samples after samples_before, without an object */
uint64_t pddc_scope_lines(int nfft, int hop, int avg, uint64_t samples_before, size_t n);
/* (slot, line) items one block of the kernel takes side by side (for tests that choose slot counts across that seam);
 * 0 for an nfft create refuses */
int pddc_scope_block_items(int nfft);

/* ---- audio: the receivers' audio at a standard rate, float32 or int16 PCM -----
 * nrx receivers, each a real float32 series x_j[i] such as the demodulator writes, give nrx real
 * series y_j[k] at L/M times the input rate: 9765.625 Hz -> 48 kHz is 3072/625.  i and k count since
 * create / reset and go on across batches; x_j[i] = 0 for i < 0.  Fixed at create, common to all
 * receivers: the ratio L/M (1 <= L, M <= 2^24, M <= 16 L; given reduced or not, stored reduced), P
 * phases (a power of two, 32 .. 1024), T taps per phase (1 .. 64, P T <= 8192), the real prototype
 * g[0 .. P T) (copied; g[P T] := 0) and scale (finite, > 0; 32767 maps +-1 to full-scale PCM).
 * Position of output k, in exact integers: v = k M, n_k = v div L, r_k = v mod L; u = r_k P,
 * q = u div L, alpha = float(u mod L) / float(L), one correctly rounded float32 division.
 * Value, float32 with floating-point contraction off, the same operation sequence for every caller
 * and every cut: acc = 0; for t = 0 .. T-1 ascending: g0 = g[t P + q], g1 = g[t P + q + 1],
 * w = fmaf(alpha, g1 - g0, g0), acc = fmaf(w, x[n_k - t], acc); y[k] = acc.  That is x convolved with
 * the piecewise-linear interpolation of g, sampled at n_k + r_k / L; no input after n_k is used.
 * Output k exists once input n_k is in the stream: ceil(N L / M) outputs after N inputs, so a batch's
 * count follows from sizes alone (pddc_audio_next_outputs; pddc_audio_outputs without an object).
 * PCM: p = (int16) clamp(rintf(y scale), -32768, 32767), ties to even; NaN gives 0.
 * Carried: per receiver its last T - 1 inputs; the object N and the next output's n and r, advanced
 * batch by batch, so nothing wraps at any stream length.  The bits of y_j[k] depend on the receiver's
 * series, L, M, P, T and g alone: not on the cut into batches (0 inputs and 0 outputs included), nrx,
 * j's index, the other receivers, strides, grid or tile sizes.
 * Non-finite samples: transient.  A NaN in x_j[p] makes the outputs k with n_k - T < p <= n_k NaN (PCM: 0), zero
 * weights included; every other output, and every other receiver, has the bits it has without it.  Nothing is left
 * behind once the sample has left the last T - 1 inputs: the caller does nothing.
 * process(): x is [nrx][x_stride] float32 with n values used per row (the demodulator's output view
 * has its capacity as stride); d_f32 [nrx][f32_stride] float32 and d_i16 [nrx][i16_stride] int16 get
 * *count values per row; either may be NULL, not both when there are outputs.  Every argument is
 * checked before anything is queued: PDDC_EINVAL for a NULL or misaligned (4 / 4 / 2 bytes) pointer
 * with work to do, PDDC_ECAPACITY when a stride is below what it must hold; n = 0 is valid.  State
 * moves only after the launch was accepted.  Stream-ordered; one stream per object, one thread at a
 * time.  create: argument errors (the limits above, a non-finite prototype value) before any device
 * access; good arguments, no device: PDDC_ENODEV.  Another ratio or prototype: another object. */
typedef struct pddc_audio pddc_audio;
int pddc_audio_create(pddc_audio **out, int device, int nrx, uint32_t L, uint32_t M, int phases, int taps,
                      const float *proto /* [phases * taps], copied */, float scale);
int pddc_audio_destroy(pddc_audio *a);
int pddc_audio_reset(pddc_audio *a);                  /* N, n, r, the carried inputs; synchronises the device */
/* outputs per receiver the next process() of n inputs writes (host arithmetic) */
int pddc_audio_next_outputs(const pddc_audio *a, size_t n, size_t *count);
/* the same without an object (host arithmetic, no device): ceil((before + n) L / M) - ceil(before L / M);
 * 0 for L or M outside 1 .. 2^24 */
uint64_t pddc_audio_outputs(uint32_t L, uint32_t M, uint64_t inputs_before, size_t n);
int pddc_audio_process(pddc_audio *a, const void *d_x, size_t n, size_t x_stride, void *d_f32, size_t f32_stride,
                       void *d_i16, size_t i16_stride, size_t *count, void *stream);

/* ---- mixer: receivers' audio summed into output buses, with a peak limiter -----
 * The stage behind audio (or squelch, or the adaptive filter): nrx receivers, each a real float32
 * series a_j[i], are summed into nbus output buses (1 .. 8) and leave as planar float32 and / or
 * interleaved int16 frames, what a sound device takes.  Every value is float32, fmaf is one
 * rounding, floating-point contraction is off.  i counts since create / reset across batches.
 * Gains: receiver j has a target gain to[j][q] per bus (finite, any sign; the nrx x nbus table of
 * create).  set_rx(rx, gains[nbus]) takes effect at the first sample of the next accepted batch:
 * from[q] := the gain the last sample processed was given (at create: to), to[q] := the new value,
 * the receiver's ramp counter c := 0; two calls between two batches count as one, the later wins.
 * Per sample c = min(c + 1, R) first, then g = to if c == R, else fmaf(to - from, float(c) invR, from);
 * R is the common ramp length (1 .. 65536), invR = 1.0f / R; c = R at create and reset.
 * A receiver is SILENT at a sample when there c == R and every to[q] is +-0: it is not read (a NaN
 * in it reaches no bus) and it is not in the sum.  The others are active; p numbers them in
 * ascending j.  With C = pddc_mixer_chunk(), for bus q and sample i: chunk m takes
 * p = m C .. m C + C - 1, s_m = +0, then s_m = fmaf(g_pq(i), a_p[i], s_m) in ascending p; y = s_0,
 * then y = y + s_m in ascending m; no active receiver: y = +0.  The tree depends on the active set
 * alone: not on n, the cut into batches, grid or tile.
 * Limiter (flag PDDC_MIX_LIMIT; block Lb 8 .. 4096, ceil finite > 0, 0 < rel <= 1), per bus with
 * the absolute block index k = i div Lb: P[k] = fmaxf over the block of fabsf(y) from +0 (a NaN is
 * dropped); m = fmaxf(P[k], P[k+1]); t[k] = ceil / m if m > ceil else 1;
 * E[k] = fminf(t[k], fmaf(rel, 1 - E[k-1], E[k-1])), E[-1] = 1.  Sample r of block k:
 * g = E[k] if r = Lb - 1, else fmaf(E[k] - E[k-1], float(r + 1) invLb, E[k-1]);
 * out = fminf(fmaxf(y g, -ceil), ceil), so |out| <= ceil exactly.  Block k is written once block
 * k + 1 is complete: Lb max(0, N div Lb - 1) outputs after N samples, a batch's count follows from
 * sizes alone (pddc_mixer_next_outputs; pddc_mixer_outputs without an object).  Without the flag
 * out = y and a batch of n samples writes n outputs.
 * +-Inf in y, in block k: m is Inf for the blocks k - 1 and k, so t = 0 and E = 0 there; the sample
 * itself becomes Inf * 0 = NaN, which fmaxf drops: it leaves as -ceil, as does a NaN in y (which P
 * ignores: it changes no gain).  From block k + 1 on E recovers by rel per block.  Nothing sticks.
 * In block 0 the ramp comes down from E[-1] = 1, so g > 0 at every sample but the block's last: an
 * infinity there is Inf * g = Inf and leaves clamped, as +ceil or -ceil by its sign.
 * Outputs, either or both: f32[q * f32_stride + k] planar; i16[k * nbus + q] interleaved frames,
 * p = (int16) clamp(rintf(out scale), -32768, 32767), NaN -> 0, audio's rule.
 * Status per bus (pddc_mixer_read): peak = fmaxf of |y| over the samples processed since create or
 * the last clear, gain = the latest E, min_gain = the smallest E since create or the last clear
 * (1 and 1 without the limiter or before the first E).
 * process(): a is [nrx][a_stride] float32 with n values used per row.  Every argument is checked
 * before anything is queued: PDDC_EINVAL for a NULL or misaligned (4 / 4 / 2 bytes) pointer with
 * work to do, for no output pointer when there are outputs, and for an output that overlaps a;
 * PDDC_ECAPACITY when a_stride < n, f32_stride < count or i16_cap_frames < count; n = 0 is valid and
 * changes nothing; a refused call changes nothing.  Stream-ordered; one stream per object, one
 * thread at a time.  create: argument errors (ranges, non-finite gains, ceil, rel, scale) before
 * any device access; good arguments, no device: PDDC_ENODEV. */
#define PDDC_MIX_LIMIT     0x1u
typedef struct pddc_mixer_params {
    int nbus;             /* Q, 1 .. 8                                      */
    int ramp;             /* R, 1 .. 65536 samples                          */
    uint32_t flags;       /* PDDC_MIX_LIMIT                                 */
    int block;            /* Lb, 8 .. 4096 (with PDDC_MIX_LIMIT)            */
    float ceil;           /* finite, > 0 (with PDDC_MIX_LIMIT)              */
    float rel;            /* 0 < rel <= 1 (with PDDC_MIX_LIMIT)             */
    float scale;          /* int16 = out * scale; finite, > 0               */
} pddc_mixer_params;
typedef struct pddc_mixer_status {
    float peak, gain, min_gain;
} pddc_mixer_status;
typedef struct pddc_mixer pddc_mixer;
int pddc_mixer_create(pddc_mixer **out, int device, int nrx, const pddc_mixer_params *params,
                      const float *gains /* [nrx][nbus], copied */);
int pddc_mixer_destroy(pddc_mixer *m);
int pddc_mixer_reset(pddc_mixer *m);                  /* N, the ramps (c = R), everything carried; synchronises the device */
int pddc_mixer_set_rx(pddc_mixer *m, int rx, const float *gains /* [nbus] */);
/* outputs per bus the next process() of n samples writes (host arithmetic) */
int pddc_mixer_next_outputs(const pddc_mixer *m, size_t n, size_t *count);
/* the limiter's count without an object (host arithmetic, no device):
 * Lb (max(0, (before + n) div Lb - 1) - max(0, before div Lb - 1)); 0 for an unsupported block */
uint64_t pddc_mixer_outputs(int block, uint64_t samples_before, size_t n);
int pddc_mixer_process(pddc_mixer *m, const void *d_a, size_t n, size_t a_stride, void *d_f32, size_t f32_stride,
                       void *d_i16, size_t i16_cap_frames, size_t *count, void *stream);
/* status[nbus] after the batches submitted so far (it waits for them); clear: peak and min_gain restart */
int pddc_mixer_read(pddc_mixer *m, pddc_mixer_status *host /* [nbus] */, int clear, void *stream);
/* C, the active receivers per chunk sum (for the reference) */
int pddc_mixer_chunk(void);
/* samples per tile of the kernel's walk (for tests that cut batches across that seam) */
int pddc_mixer_tile_outputs(void);

/* pinned host memory for the two calls above */
int pddc_host_alloc(void **h_ptr, size_t nbytes);
int pddc_host_free(void *h_ptr);

/* ---- fsk: start-stop FSK (RTTY) decoding per receiver ---------------------------
 * The first stage whose output is data, not samples: two-tone FSK with start-stop characters (RTTY at
 * 45.45 / 50 / 75 baud with 170 / 450 / 850 Hz shift, the asynchronous maritime and weather traffic).
 * It reads the rows the tuner, blanker, receiver filter and carrier write.  K receivers (1 .. 1024), a
 * window length W (1 .. 256), a bank of B modems (1 .. 16), copied at create.  Modem b: hm[W] and
 * hs[W], complex float32 taps (the mark and the space matched filter, every value finite); inc,
 * uint32 in 1 .. 2^30, the bit phase advanced per sample, 2^32 baud / rate; nbits, 5 .. 8.  Receiver j:
 * a modem index and flags PDDC_FSK_ON, _REVERSE, _RESTART.
 * Input per batch: z[j z_stride + i], i < n, complex float32, any row stride, n >= 0.  m counts the
 * object's samples since create / reset (every batch adds n, for every receiver); inputs before a
 * receiver's first are zero.
 * Discriminator, for every sample m of an ON receiver; every operation is one float32 operation in
 * this order, contraction off:
 *   M = sum over t = 0 .. W-1 of hm[t] z[m - t], from (0, 0) with t ascending, per tap
 *       re = fmaf(hr, zr, re); re = fmaf(-hi, zi, re); im = fmaf(hr, zi, im); im = fmaf(hi, zr, im);
 *   S the same with hs.  pm = fmaf(Mi, Mi, Mr Mr), ps likewise; with REVERSE the two are exchanged.
 *   space = (ps > pm), so a NaN reads as mark.  s = pm + ps; d = s > 0 ? (pm - ps) / s : 0, the division
 *   correctly rounded; q = |d|.  Non-finite samples are data like any other: nothing is tested or cleaned.
 *   Transient, in the receiver's own row alone: while a NaN is in the window, pm or ps and with it s is
 *   NaN, so d = +0 and the sample reads mark; an infinity does the same wherever it makes a power NaN
 *   (inf - inf, 0 inf), otherwise d is NaN and space is the plain comparison.  fminf drops a NaN q.
 *   Nothing is left behind once the sample has left the window.
 * Start-stop receiver, per ON receiver, sample by sample behind the discriminator.  Carried: state
 * (IDLE, START, DATA, STOP), prev (the previous `space`, initially false), acc (uint32), k, shift,
 * qmin, start (the uint64 sample index of the edge) and the counters.
 *   IDLE: if space && !prev: state = START, acc = 2^31, start = m; no strobe on this sample.
 *   Other states: a2 = acc + inc (mod 2^32); a strobe occurs iff a2 < acc; acc = a2.  On a strobe:
 *     START: if space, DATA with k = 0, shift = 0, qmin = q; otherwise IDLE and false_starts++.
 *     DATA:  shift |= (space ? 0 : 1) << k; qmin = fminf(qmin, q); ++k; when k == nbits, STOP.
 *     STOP:  qmin = fminf(qmin, q); a character {start, code = shift, flags = space ?
 *            PDDC_FSK_FRAMING : 0, quality = qmin} is emitted; chars++; framing += space; IDLE.
 *   prev = space at the end of every sample, in every state.
 * A stop element of 1, 1.5 or 2 bits is accepted alike; a break yields one framing-error character,
 * then nothing until mark returns.
 * Receiver control.  An OFF receiver is not read and does not advance: its count is 0, its d row, if
 * one is asked for, is written +0.  set_rx(rx, modem, flags) takes effect at the next batch's first
 * sample.  RESTART, or a change from OFF to ON, clears the receiver's carried inputs and puts the
 * start-stop receiver in IDLE with prev = mark; the counters stay.  Another modem keeps the carried
 * inputs and puts the start-stop receiver in IDLE: a character in progress is dropped.  reset() clears
 * everything and m, and synchronises the device.
 * Outputs of process(), all device memory, no host synchronisation: chars [nrx][char_stride], the
 * characters whose STOP strobe lies in this batch, in order; counts uint32 [nrx]; d float32
 * [nrx][d_stride] or NULL, the soft discriminator, one value per input (for a tuning display and for
 * host decoders of the synchronous modes).
 * Capacity: pddc_fsk_max_chars(f, n, &count) is host arithmetic, max over the bank of n div P_b + 1
 * with P_b = ceil((nbits_b + 1.5) 2^32 / inc_b): two STOP strobes are at least 1 + P_b samples apart
 * ("FSK decoder", derives it).  A char_stride below it is PDDC_ECAPACITY, and nothing is queued.
 * process(): every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned
 * pointer (z and chars 8 bytes, counts and d 4; d may be NULL; with n = 0 z and chars are not looked at
 * and counts may be NULL), PDDC_ECAPACITY for a stride below n or below the bound, PDDC_EINVAL when an
 * output's byte range meets the input's.  n = 0 is valid: counts, if given, is set to 0, nothing
 * carried moves, marks of set_rx stay for the next batch.  State moves only after the launch was
 * accepted.  Stream-ordered; one stream per object, one thread at a time.
 * read(): per receiver chars, framing, false_starts (since create / reset), the state and d_last (the
 * last d computed, 0 before the first) behind the batches submitted so far (it waits for them).
 * Every bit of chars, counts, d and the status is independent of the cut into batches (n = 0 and n = 1
 * included), nrx, j's index, the other receivers, strides, grid and tile sizes.
 * create: argument errors before any device access (non-finite taps, inc or nbits out of range, a bad
 * modem index, unknown flag bits); good arguments, no device: PDDC_ENODEV. */
#define PDDC_FSK_ON       0x1u
#define PDDC_FSK_REVERSE  0x2u   /* mark and space exchanged                    */
#define PDDC_FSK_RESTART  0x4u   /* set_rx: start this receiver afresh          */
#define PDDC_FSK_FRAMING  0x1    /* pddc_fsk_char.flags: the stop element was space */
#define PDDC_FSK_IDLE     0      /* pddc_fsk_status.state                       */
#define PDDC_FSK_START    1
#define PDDC_FSK_DATA     2
#define PDDC_FSK_STOP     3
typedef struct pddc_fsk_rx {
    int modem;            /* 0 .. nmodems - 1                             */
    uint32_t flags;       /* PDDC_FSK_ON | _REVERSE | _RESTART            */
} pddc_fsk_rx;
typedef struct pddc_fsk_char {
    uint64_t start;       /* sample index m of the start element's edge   */
    uint16_t code;        /* data bit k in bit k, mark = 1                */
    uint16_t flags;       /* PDDC_FSK_FRAMING                             */
    float quality;        /* the least |d| at the data and stop strobes   */
} pddc_fsk_char;
typedef struct pddc_fsk_status {
    uint32_t chars, framing, false_starts;
    uint32_t state;       /* PDDC_FSK_IDLE / _START / _DATA / _STOP       */
    float d_last;
} pddc_fsk_status;
typedef struct pddc_fsk pddc_fsk;
int pddc_fsk_create(pddc_fsk **out, int device, int nrx, int window, int nmodems,
                    const float *taps /* [nmodems][2][window] complex: hm, then hs; copied */,
                    const uint32_t *inc /* [nmodems] */, const int *nbits /* [nmodems] */, const pddc_fsk_rx *rx /* [nrx] */);
int pddc_fsk_destroy(pddc_fsk *f);
int pddc_fsk_reset(pddc_fsk *f);                      /* m and everything carried; synchronises the device */
int pddc_fsk_set_rx(pddc_fsk *f, int rx, int modem, uint32_t flags);
int pddc_fsk_max_chars(const pddc_fsk *f, size_t n, size_t *count);
int pddc_fsk_process(pddc_fsk *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                     void *d_counts, void *d_d, size_t d_stride, void *stream);
/* status[nrx] after the batches submitted so far (it waits for them) */
int pddc_fsk_read(pddc_fsk *f, pddc_fsk_status *host /* [nrx] */, void *stream);
/* samples per tile of the kernel's walk (for tests that place batch cuts on its seams) */
int pddc_fsk_tile_outputs(void);

/* ---- morse: CW (on-off keyed Morse) decoding per receiver -------------------------
 * Beside the chain, where fsk sits: it reads the rows the tuner, blanker, receiver filter and carrier
 * write, and gives characters, not samples.  K receivers (1 .. 1024), a window length W (1 .. 256), a
 * bank of B keyers (1 .. 16), copied at create.  Keyer b: h[W], real float32 taps of the envelope
 * filter, every value finite; two0, two_min, two_max, uint32: the length of TWO dots in samples times
 * 256, the start value and the bounds of the speed tracker, 512 <= two_min <= two0 <= two_max <= 2^28;
 * shift, 0 .. 8, the tracker's time constant.  Common to the object, float32: a_on, a_off
 * (0 < a_off <= a_on < 1), the thresholds' places between floor and peak; rel, relf in [0, 1], the
 * release of peak and floor per block; ratio >= 1, the least peak over floor that counts as a signal.
 * Receiver j: a keyer index and flags PDDC_MORSE_ON, _FIXED (no speed tracking), _RESTART.
 * Input per batch: z[j z_stride + i], i < n, complex float32, any row stride, n >= 0.  m counts the
 * object's samples since create / reset (every batch adds n, for every receiver); inputs before a
 * receiver's first are zero.  Every float operation below is one float32 operation in the stated
 * order, contraction off; all timing is in integers.
 * 1. Envelope, for every sample m of an ON receiver: y = sum over t = 0 .. W-1 of h[t] z[m - t], from
 *    (0, 0) with t ascending, per tap re = fmaf(h, zr, re); im = fmaf(h, zi, im).  p = fmaf(yi, yi, yr yr);
 *    if !(p <= FLT_MAX) then p = 0: a NaN or an infinity in the window reads as no signal, nothing
 *    non-finite reaches a tracker, and nothing is left behind once the sample has left the window.
 * 2. Key: key = p > on ? 1 : (p < off ? 0 : key_prev); on = off = +inf before the first block ends.
 * 3. Block meter, behind the sample's key and timing.  Blocks are the 64 samples with the same m >> 6,
 *    absolute in m.  Carried: hi (initially 0), lo (+inf), pk, fl, primed.  Every sample: hi =
 *    fmaxf(hi, p); lo = fminf(lo, p).  On a block's last sample (m & 63 == 63): if not primed: pk = hi,
 *    fl = lo, primed; otherwise pk = fmaxf(hi, fmaf(rel, fl - pk, pk)); fl = fminf(lo, fmaf(relf, pk - fl,
 *    fl)), the new pk in fl.  span = pk - fl.  If pk >= ratio * fl && span > 0: on = fmaf(a_on, span, fl),
 *    off = fmaf(a_off, span, fl); otherwise on = off = +inf.  Then hi = 0, lo = +inf.  So block k's levels
 *    govern block k + 1, and the elements in the first block of a transmission are lost.
 * 4. Element timing, with prev the previous sample's key.  Carried: two, nel, code (initially 1, a
 *    sentinel), start, word, first (initially 1), t_up, t_down, last (initially 0), the counters.
 *    In this order:
 *    a. if !prev && nel > 0 && m - t_up == ((two + 255) >> 8): the character {start, code, nel, flags,
 *       two} is emitted, flags = (word ? PDDC_MORSE_WORD : 0) | (nel > 15 ? PDDC_MORSE_LONG : 0); chars++;
 *       nel = 0; code = 1.
 *    b. rising edge (key && !prev): t_down = m; if nel == 0: start = m and word = first ||
 *       ((m - t_up) << 9) >= 5 two in uint64 (m - t_up taken as at most 2^40), a gap of at least five dots.
 *    c. falling edge (!key && prev): dur = min(m - t_down, 2^24); dash = (dur << 8) >= two; if nel < 15:
 *       code = code << 1 | dash; nel saturates at 255; marks++.  Unless FIXED, and only if last > 0: a =
 *       min(dur, last), b = max(dur, last); if b >= 2 a && b <= 4 a (a dot beside a dash, whose sum is two
 *       dots whatever the speed): two += (((a + b) << 7) - two) >> shift in signed 64 bits with an
 *       arithmetic shift, then clamped to [two_min, two_max].  last = dur; t_up = m; first = 0.
 *    A dash is a mark of at least two dots, a character gap a space of at least two dots.  code holds
 *    the first 15 elements, the first highest, dash = 1, under a leading 1 ("A", dot dash: binary 101).
 * Receiver control.  An OFF receiver is not read and does not advance: its count is 0, its p row, if
 * one is asked for, is written +0.  set_rx(rx, keyer, flags) takes effect at the next batch's first
 * sample.  RESTART, or a change from OFF to ON: the carried inputs are zero, the meter is unprimed with
 * hi, lo and the thresholds as at create, key = 0, the timing is as at create with two = the keyer's
 * two0; the counters stay.  Another keyer: the same, but the carried inputs stay.  reset() clears
 * everything and m, and synchronises the device.
 * Outputs of process(), all device memory, no host synchronisation: chars [nrx][char_stride], the
 * characters whose emission sample lies in this batch, in order; counts uint32 [nrx]; p float32
 * [nrx][p_stride] or NULL, the envelope power, one value per input.
 * Capacity: pddc_morse_max_chars(f, n, &count) is host arithmetic: two emissions lie at least D = 1 +
 * ((two_min + 255) >> 8) samples apart, D the least over the bank, so n samples end at most
 * (n - 1) div D + 1 characters (0 for n = 0; DESIGN.md 4, "Morse decoder", derives it).  A char_stride
 * below it is PDDC_ECAPACITY, and nothing is queued.
 * process(): every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned
 * pointer (z and chars 8 bytes, counts and p 4; p may be NULL; with n = 0 z and chars are not looked at
 * and counts may be NULL), PDDC_ECAPACITY for a stride below n or below the bound, PDDC_EINVAL when an
 * output's byte range meets the input's.  n = 0 is valid: counts, if given, is set to 0, nothing
 * carried moves, marks of set_rx stay for the next batch.  State moves only after the launch was
 * accepted.  Stream-ordered; one stream per object, one thread at a time.
 * read(): per receiver chars and marks (since create / reset), two, nel, key, and pk, fl (0 until the
 * meter is primed) behind the batches submitted so far (it waits for them).
 * Every bit of chars, counts, p and the status is independent of the cut into batches (n = 0 and n = 1
 * included), nrx, j's index, the other receivers, strides, grid and tile sizes.
 * create: argument errors before any device access (non-finite taps, a keyer or a parameter out of
 * range, a bad keyer index, unknown flag bits); good arguments, no device: PDDC_ENODEV. */
#define PDDC_MORSE_ON       0x1u
#define PDDC_MORSE_FIXED    0x2u   /* the keyer's two0 throughout: no speed tracking */
#define PDDC_MORSE_RESTART  0x4u   /* set_rx: start this receiver afresh          */
#define PDDC_MORSE_WORD     0x1    /* pddc_morse_char.flags: the first character, or one behind a gap of five dots */
#define PDDC_MORSE_LONG     0x2    /* more than 15 elements: code holds the first 15 */
typedef struct pddc_morse_keyer {
    uint32_t two0, two_min, two_max;   /* two dots in samples, times 256        */
    uint32_t shift;                    /* 0 .. 8                                */
} pddc_morse_keyer;
typedef struct pddc_morse_params {
    float a_on, a_off, rel, relf, ratio;
} pddc_morse_params;
typedef struct pddc_morse_rx {
    int keyer;            /* 0 .. nkeyers - 1                             */
    uint32_t flags;       /* PDDC_MORSE_ON | _FIXED | _RESTART            */
} pddc_morse_rx;
typedef struct pddc_morse_char {
    uint64_t start;       /* sample index m of the first element's rising edge */
    uint16_t code;        /* 1, then an element per bit, dash = 1         */
    uint8_t nel;          /* elements, saturating at 255                  */
    uint8_t flags;        /* PDDC_MORSE_WORD | _LONG                      */
    uint32_t two;         /* the tracker's two dots at the emission       */
} pddc_morse_char;
typedef struct pddc_morse_status {
    uint32_t chars, marks;
    uint32_t two, nel, key;
    float pk, fl;
} pddc_morse_status;
typedef struct pddc_morse pddc_morse;
int pddc_morse_create(pddc_morse **out, int device, int nrx, int window, int nkeyers,
                      const float *taps /* [nkeyers][window]; copied */, const pddc_morse_keyer *keyers /* [nkeyers] */,
                      const pddc_morse_params *par, const pddc_morse_rx *rx /* [nrx] */);
int pddc_morse_destroy(pddc_morse *f);
int pddc_morse_reset(pddc_morse *f);                  /* m and everything carried; synchronises the device */
int pddc_morse_set_rx(pddc_morse *f, int rx, int keyer, uint32_t flags);
int pddc_morse_max_chars(const pddc_morse *f, size_t n, size_t *count);
int pddc_morse_process(pddc_morse *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                       void *d_counts, void *d_p, size_t p_stride, void *stream);
/* status[nrx] after the batches submitted so far (it waits for them) */
int pddc_morse_read(pddc_morse *f, pddc_morse_status *host /* [nrx] */, void *stream);
/* samples per tile of the kernel's walk, aligned to m (for tests that place batch cuts on its seams) */
int pddc_morse_tile_outputs(void);

/* ---- psk: differential BPSK (PSK31 / 63 / 125) decoding per receiver ---------------
 * Beside the chain, where fsk and morse sit: it reads the rows the tuner, blanker, receiver filter and
 * carrier write, and gives Varicode characters.  Where this block is silent, fsk's rules hold.
 * K receivers (1 .. 1024), a window length W (1 .. 256), a bank of B modems (1 .. 16), copied at
 * create.  Modem b: h[W], real float32 taps of the matched filter, every value finite; inc, uint32 in
 * 1 .. 2^29: the symbol phase advanced per sample, 2^32 baud / rate, so a symbol is at least 8 samples;
 * q in 1 .. 64 with 4 q inc <= 2^32: the early and late offset in samples, about a quarter symbol;
 * step, uint32 in 0 .. inc: the clock correction per reversal, 0 is a fixed clock.  Receiver j: a modem
 * index and flags PDDC_PSK_ON, _RESTART.
 * Input per batch: z[j z_stride + i], i < n, complex float32, any row stride, n >= 0.  m counts the
 * object's samples since create / reset.  Every float operation below is one float32 operation in the
 * stated order, contraction off; the clock and the framing are integers.
 * 1. Filter, for every sample m of an ON receiver: y[m] = sum over t = 0 .. W-1 of h[t] z[m - t], from
 *    (0, 0) with t ascending, per tap re = fmaf(h, zr, re); im = fmaf(h, zi, im).  p[m] = fmaf(yi, yi,
 *    yr yr).  z, y and p at samples before the receiver's first are +0.
 * 2. Clock.  Carried: acc, uint32, 0 at the start.  Each sample: a2 = acc + inc mod 2^32; a strobe iff
 *    a2 < acc; acc = a2.
 * 3. On a strobe at sample m, with c = m - q the on-time sample, e = m - 2 q the early one and m the
 *    late one.  u = y[c], pu = p[c]; carried v, pv: the previous strobe's u and pu, zero at the start.
 *    dot = fmaf(ui, vi, ur vr); cross = fmaf(ui, vr, -(ur vi)); s = pu + pv; d = s > 0 ? (dot + dot) / s
 *    : 0; x = s > 0 ? (cross + cross) / s : 0, both divisions correctly rounded.  bit = dot > 0: no
 *    reversal is 1, and a NaN reads as 0, the idle bit.
 *    Clock correction, on a reversal (bit == 0) only -- a run of ones has a flat envelope and nothing to
 *    time: if p[m] > p[e], the peak lies later: acc = acc >= step ? acc - step : 0; otherwise, if
 *    p[e] > p[m]: acc = acc + step (no overflow: acc < inc behind a strobe).  A NaN moves nothing.
 *    Framing.  Carried: reg (uint32, 0), nb (saturates at 255), qmin, start.  If reg == 0 and bit == 0:
 *    nothing.  Otherwise: if reg == 0: start = c, nb = 0, qmin = |d|.  reg = reg << 1 | bit; ++nb; qmin =
 *    fminf(qmin, |d|).  If (reg & 3) == 0: the character {start, code = (reg >> 2) & 0xFFFF, nbits =
 *    nb - 2, flags = (nb - 2 > 16 ? PDDC_PSK_LONG : 0), quality = qmin} is emitted; chars++; reg = 0.
 *    Then v = u, pv = pu, symbols++.
 *    code is the Varicode character as sent, the first bit highest ("e" is binary 11, space is 1).
 * Receiver control.  An OFF receiver is not read and does not advance: its count and its nsym are 0.
 * set_rx(rx, modem, flags) takes effect at the next batch's first sample.  RESTART, a change from OFF
 * to ON and another modem do the same: the carried inputs and filter outputs are zero, the clock, the
 * differential pair and the framing are as at create; the counters stay.  reset() clears everything and
 * m, and synchronises the device.
 * Outputs of process(), all device memory, no host synchronisation: chars [nrx][char_stride], the
 * characters whose last strobe lies in this batch, in order; counts uint32 [nrx]; sym float2
 * [nrx][sym_stride] or NULL, one (d, x) per strobe of the batch, in order, with nsym uint32 [nrx]: the
 * hook for a phase display, for AFC on the host (the angle of (d + j x)^2 is twice the offset's phase
 * per symbol) and for host decoders of QPSK and FEC modes.
 * Capacity, host arithmetic.  Behind a strobe acc <= inc - 1 + step (a late correction only puts the next
 * strobe off), so two strobes lie at least D_b =
 * floor((2^32 - step_b) / inc_b) samples apart ("PSK decoder", derives it), D the least
 * over the bank: pddc_psk_max_syms(f, n, &count) gives (n - 1) div D + 1, 0 for n = 0.  Emissions lie
 * at least 3 strobes apart: pddc_psk_max_chars gives (max_syms - 1) div 3 + 1, 0 for n = 0.  A
 * char_stride or, with sym, a sym_stride below its bound is PDDC_ECAPACITY, and nothing is queued.
 * process(): every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned
 * pointer (z, chars and sym 8 bytes, counts and nsym 4; sym may be NULL, and nsym is then not looked at
 * beyond its alignment; with n = 0 z, chars and sym are not looked at and counts and nsym may be NULL),
 * PDDC_ECAPACITY for a stride below n or below a bound, PDDC_EINVAL when an output's byte range meets
 * the input's.  n = 0 is valid: counts and nsym, if given, are set to 0, nothing carried moves, marks
 * of set_rx stay for the next batch.  State moves only after the launch was accepted.  Stream-ordered;
 * one stream per object, one thread at a time.
 * read(): per receiver chars and symbols (since create / reset), acc, reg, and the last strobe's d and
 * x behind the batches submitted so far (it waits for them).
 * Every bit of chars, counts, sym, nsym and the status is independent of the cut into batches (n = 0
 * and n = 1 included), nrx, j's index, the other receivers, strides, grid and tile sizes.
 * create: argument errors before any device access (non-finite taps, a modem out of range, a bad modem
 * index, unknown flag bits); good arguments, no device: PDDC_ENODEV. */
#define PDDC_PSK_ON       0x1u
#define PDDC_PSK_RESTART  0x4u   /* set_rx: start this receiver afresh          */
#define PDDC_PSK_LONG     0x1    /* pddc_psk_char.flags: more than 16 bits: code holds the last 16 */
typedef struct pddc_psk_modem {
    uint32_t inc;         /* 1 .. 2^29: 2^32 baud / rate                  */
    uint32_t q;           /* 1 .. 64, 4 q inc <= 2^32                     */
    uint32_t step;        /* 0 .. inc                                     */
} pddc_psk_modem;
typedef struct pddc_psk_rx {
    int modem;            /* 0 .. nmodems - 1                             */
    uint32_t flags;       /* PDDC_PSK_ON | _RESTART                       */
} pddc_psk_rx;
typedef struct pddc_psk_char {
    uint64_t start;       /* sample index m of the first bit's on-time sample */
    uint16_t code;        /* the bits in front of the two zeros, the first highest */
    uint8_t nbits;        /* their number, saturating at 253              */
    uint8_t flags;        /* PDDC_PSK_LONG                                */
    float quality;        /* the least |d| of the character's strobes     */
} pddc_psk_char;
typedef struct pddc_psk_status {
    uint32_t chars, symbols;
    uint32_t acc, reg;
    float d_last, x_last;
} pddc_psk_status;
typedef struct pddc_psk pddc_psk;
int pddc_psk_create(pddc_psk **out, int device, int nrx, int window, int nmodems,
                    const float *taps /* [nmodems][window]; copied */, const pddc_psk_modem *modems /* [nmodems] */,
                    const pddc_psk_rx *rx /* [nrx] */);
int pddc_psk_destroy(pddc_psk *f);
int pddc_psk_reset(pddc_psk *f);                      /* m and everything carried; synchronises the device */
int pddc_psk_set_rx(pddc_psk *f, int rx, int modem, uint32_t flags);
int pddc_psk_max_syms(const pddc_psk *f, size_t n, size_t *count);
int pddc_psk_max_chars(const pddc_psk *f, size_t n, size_t *count);
int pddc_psk_process(pddc_psk *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                     void *d_counts, void *d_sym, size_t sym_stride, void *d_nsym, void *stream);
/* status[nrx] after the batches submitted so far (it waits for them) */
int pddc_psk_read(pddc_psk *f, pddc_psk_status *host /* [nrx] */, void *stream);
/* samples per tile of the kernel's walk, from the batch's first (for tests that place batch cuts on its seams) */
int pddc_psk_tile_outputs(void);

/* ---- sitor: synchronous FSK (SITOR-B / NAVTEX / AMTOR FEC) decoding per receiver ----
 * Beside the chain, where fsk, morse and psk sit: it reads the rows the tuner, blanker, receiver filter
 * and carrier write, and gives the 7-bit characters of the constant-ratio code of ITU-R M.476 (100
 * baud, 170 Hz shift, no start or stop elements).  Where this block is silent, fsk's rules hold.
 * K receivers (1 .. 1024), a window length W (1 .. 256), a bank of B modems (1 .. 16), copied at
 * create.  Modem b: hm[W] and hs[W], complex float32 taps of the mark and the space filter as for fsk,
 * every value finite; inc, uint32 in 1 .. 2^29: the bit phase advanced per sample, 2^32 baud / rate, so
 * a bit is at least 8 samples; step, uint32 in 0 .. inc: the clock correction per transition, 0 is a
 * fixed clock; lock, 0, 2, 3 or 4: the valid characters in a row that lock the framing without a
 * phasing word (0: only a phasing word locks); unlock, 1 .. 15: the invalid characters in a row that
 * unlock it.  Receiver j: a modem index and flags PDDC_SITOR_ON, _REVERSE, _RESTART.
 * Input per batch: z[j z_stride + i], i < n, complex float32, any row stride, n >= 0.  m counts the
 * object's samples since create / reset (every batch adds n, for every receiver); inputs before a
 * receiver's first are zero.
 * Discriminator, for every sample m of an ON receiver: exactly fsk's operation sequence.  M and S by
 * four spelled fmaf per tap, t ascending; pm = fmaf(M.im, M.im, M.re M.re), ps likewise (REVERSE: pm
 * and ps exchanged); space = ps > pm; s = pm + ps; d = s > 0 ? (pm - ps) / s : 0, correctly rounded;
 * q = |d|.  Non-finite samples are data: fsk's "Non-finite samples" paragraph holds word for word, in
 * the receiver's own row alone (while a NaN is in the window s is NaN, d = +0 and the sample reads
 * mark; fminf drops a NaN q; nothing is left behind once the sample has left the window -- but for the
 * bits it put into reg and the corrections it gave the clock, which the framing's own rules undo).
 * Clock and framing, per sample, behind the discriminator, all integer.  Carried per receiver: acc
 * (uint32), prev (initially mark), reg (uint32, 28 bits used), seen, nb, bad, locked, start (uint64),
 * qmin, the counters chars, symbols, errors, reframes, and d_last.
 * 1. a2 = acc + inc mod 2^32; a strobe iff a2 < acc; acc = a2.
 * 2. On a strobe, in order: symbols++; bit = space ? 0 : 1; reg = (reg >> 1) | (bit << 27); seen =
 *    min(seen + 1, 28); with soft, d is appended to the receiver's soft row.  The newest character is
 *    reg >> 21, its first-received bit lowest.
 *    a. If locked: if nb == 0: start = m, qmin = q; otherwise qmin = fminf(qmin, q).  ++nb.  When nb ==
 *       7: the record {start, code = reg >> 21, flags = (popcount(code) == 4 ? PDDC_SITOR_VALID : 0),
 *       quality = qmin} is emitted; chars++; nb = 0.  If the code was valid: bad = 0; otherwise
 *       errors++ and ++bad.  If bad >= unlock: locked = 0, seen = 0.
 *    b. Then, if reg is one of the two 28-bit phasing words -- alpha beta alpha beta and beta alpha beta
 *       alpha with alpha = 0x0F (phasing signal 1) and beta = 0x33 (phasing signal 2), 7 bits each, the
 *       newest character highest: 0x1ECC7B3 and 0x663D98F -- : unless locked and nb == 0: reframes++.
 *       Then locked = 1, nb = 0, bad = 0: a character in progress is dropped.  This rule acts in every
 *       state: four of the seven bit phases of the phasing sequence are all-valid, and rule c alone
 *       locks on one of them (DESIGN.md 8 has what that costs).
 *    c. Otherwise, if not locked, lock > 0, seen >= 7 lock and each of the newest `lock` 7-bit groups of
 *       reg has four ones: locked = 1, nb = 0, bad = 0.
 * 3. If space != prev: acc += step where acc < 2^31, else acc -= step (neither can wrap, since step <=
 *    inc <= 2^29); then prev = space.  A transition in a bit's first half brings the strobe nearer, one
 *    in its second half moves it away: the strobe settles half a bit behind the transitions.
 * Receiver control.  An OFF receiver is not read and does not advance: its count and its nsoft are 0.
 * set_rx(rx, modem, flags) takes effect at the next batch's first sample.  RESTART, or a change from
 * OFF to ON: the carried inputs are zero, acc = 0, prev = mark, reg = seen = nb = bad = locked = 0; the
 * counters stay.  Another modem: the carried inputs, acc and prev stay, reg = seen = nb = bad = locked
 * = 0.  reset() clears everything and m, and synchronises the device.
 * Outputs of process(), all device memory, no host synchronisation: chars [nrx][char_stride], the
 * characters whose seventh strobe lies in this batch, in order; counts uint32 [nrx]; soft float32
 * [nrx][soft_stride] or NULL, d at every strobe of the batch, in order, with nsoft uint32 [nrx]: the
 * hook for soft-decision combining of the two copies of a mode-B character on the host.
 * Capacity, host arithmetic.  The clock is advanced below 2^31 only, and acc enters [2^31, 2^32) below
 * 2^31 + inc, so two strobes lie at least D_b = 2^31 div inc_b samples apart ("SITOR
 * decoder", derives it), D the least over the bank: pddc_sitor_max_syms(f, n, &count) gives (n - 1)
 * div D + 1, 0 for n = 0.  Emissions lie at least 7 strobes apart: pddc_sitor_max_chars gives
 * (max_syms - 1) div 7 + 1, 0 for n = 0.  A char_stride or, with soft, a soft_stride below its bound is
 * PDDC_ECAPACITY, and nothing is queued.  The kernel never drops.
 * process(): every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned
 * pointer (z and chars 8 bytes, counts, soft and nsoft 4; soft may be NULL, and nsoft is then not
 * looked at beyond its alignment; with n = 0 z, chars and soft are not looked at and counts and nsoft
 * may be NULL), PDDC_ECAPACITY for a stride below n or below a bound, PDDC_EINVAL when an output's byte
 * range meets the input's.  n = 0 is valid: counts and nsoft, if given, are set to 0, nothing carried
 * moves, marks of set_rx stay for the next batch.  State moves only after the launch was accepted.
 * Stream-ordered; one stream per object, one thread at a time.
 * read(): per receiver chars, symbols, errors and reframes (since create / reset), locked, acc, reg,
 * and d_last (the last d computed, 0 before the first) behind the batches submitted so far (it waits
 * for them), as the next batch will find them.
 * Every bit of chars, counts, soft, nsoft and the status is independent of the cut into batches (n = 0
 * and n = 1 included), nrx, j's index, the other receivers, strides, grid and tile sizes.
 * create: argument errors before any device access (non-finite taps, a modem out of range, a bad modem
 * index, unknown flag bits); good arguments, no device: PDDC_ENODEV.
 * The text (the M.476 table, the letters and figures shifts, the pairing of a mode-B character's two
 * copies) is host work: Python's sitor_text has it. */
#define PDDC_SITOR_ON       0x1u
#define PDDC_SITOR_REVERSE  0x2u   /* mark and space exchanged                    */
#define PDDC_SITOR_RESTART  0x4u   /* set_rx: start this receiver afresh          */
#define PDDC_SITOR_VALID    0x1    /* pddc_sitor_char.flags: four of the seven bits are mark */
typedef struct pddc_sitor_modem {
    uint32_t inc;         /* 1 .. 2^29: 2^32 baud / rate                  */
    uint32_t step;        /* 0 .. inc                                     */
    uint32_t lock;        /* 0, 2, 3 or 4                                 */
    uint32_t unlock;      /* 1 .. 15                                      */
} pddc_sitor_modem;
typedef struct pddc_sitor_rx {
    int modem;            /* 0 .. nmodems - 1                             */
    uint32_t flags;       /* PDDC_SITOR_ON | _REVERSE | _RESTART          */
} pddc_sitor_rx;
typedef struct pddc_sitor_char {
    uint64_t start;       /* sample index m of the character's first strobe */
    uint16_t code;        /* the first-received bit in bit 0, mark = 1    */
    uint16_t flags;       /* PDDC_SITOR_VALID                             */
    float quality;        /* the least |d| of the character's strobes     */
} pddc_sitor_char;
typedef struct pddc_sitor_status {
    uint32_t chars, symbols, errors, reframes;
    uint32_t locked, acc, reg;
    float d_last;
} pddc_sitor_status;
typedef struct pddc_sitor pddc_sitor;
int pddc_sitor_create(pddc_sitor **out, int device, int nrx, int window, int nmodems,
                      const float *taps /* [nmodems][2][window] complex: hm, then hs; copied */,
                      const pddc_sitor_modem *modems /* [nmodems] */, const pddc_sitor_rx *rx /* [nrx] */);
int pddc_sitor_destroy(pddc_sitor *f);
int pddc_sitor_reset(pddc_sitor *f);                  /* m and everything carried; synchronises the device */
int pddc_sitor_set_rx(pddc_sitor *f, int rx, int modem, uint32_t flags);
int pddc_sitor_max_syms(const pddc_sitor *f, size_t n, size_t *count);
int pddc_sitor_max_chars(const pddc_sitor *f, size_t n, size_t *count);
int pddc_sitor_process(pddc_sitor *f, const void *d_z, size_t n, size_t z_stride, void *d_chars, size_t char_stride,
                       void *d_counts, void *d_soft, size_t soft_stride, void *d_nsoft, void *stream);
/* status[nrx] after the batches submitted so far (it waits for them) */
int pddc_sitor_read(pddc_sitor *f, pddc_sitor_status *host /* [nrx] */, void *stream);
/* samples per tile of the kernel's walk, from the batch's first (for tests that place batch cuts on its seams) */
int pddc_sitor_tile_outputs(void);

/* ---- fax: radiofax (WEFAX) image decoding per receiver ----
 * Beside the chain, where fsk, morse, psk and sitor sit: it reads the rows the tuner, blanker, receiver
 * filter and carrier write, and gives the pixels and the line structure of a frequency-modulated
 * facsimile (120 lines a minute, black 1500 Hz, white 2300 Hz of the audio).  The receiver is tuned to
 * the subcarrier's centre, 1900 Hz of the audio, so black lies 400 Hz below the tuned frequency and
 * white 400 Hz above it.  Where this block is silent, sitor's rules hold.
 * K receivers (1 .. 1024), a window length W (1 .. 256), a bank of B modems (1 .. 16), copied at
 * create.  Modem b: h[W], real float32 taps of the pre-detection low-pass, every value finite; inc,
 * uint32 in 1 .. 2^31: the pixel phase advanced per sample, 2^32 width lpm / 60 / rate, so a pixel is
 * at least 2 samples; width, 16 .. 8192 pixels per line (round(pi IOC): 1810 for IOC 576, 905 for IOC
 * 288); box, 1 .. 16: the length of the post-detection boxcar; scale and bias, finite float32: grey
 * level = scale v + bias; start_lo <= start_hi and stop_lo <= stop_hi, uint16, two ranges that share
 * no value (the start tone lies below the stop tone for IOC 576 and above it for IOC 288): the
 * crossings per line that make a line a start-tone or a stop-tone line; need, 1 .. 255: such lines in
 * a row that start or stop an image.  Receiver j: a modem index and flags PDDC_FAX_ON, _REVERSE, _RESTART.
 * Input per batch: z[j z_stride + i], i < n, complex float32, any row stride, n >= 0.  m counts the
 * object's samples since create / reset; inputs, y and f before a receiver's first sample are zero.
 * Per sample m of an ON receiver, every step with one operation sequence:
 * 1. y = sum h[t] z[m - t]: y.re = fmaf(h[t], z.re, y.re), y.im likewise, t ascending from (0, 0).
 * 2. w = y[m] conj(y[m - 1]): w.re = y.re p.re + y.im p.im, w.im = y.im p.re - y.re p.im (products
 *    rounded, then the sum; p = y[m - 1]).  q = (w.re - w.re) + (w.im - w.im): 0, or NaN where w is
 *    not finite.  d = 0 where w.re and w.im are both zero, else atan2f(w.im, w.re) (1 / pi) + q with
 *    1 / pi = 0.318309886183790672f; f = d, under REVERSE -d.  (atan2f is the platform's: f is defined
 *    to its accuracy, a few units in the last place; everything behind it is exact in f.)
 * 3. a2 = acc + inc mod 2^32; a strobe iff a2 < acc; acc = a2.
 * 4. On a strobe: v = (f[m - box + 1] + ... + f[m]), added in that order, times 1.0f / box (correctly
 *    rounded); g = fmaf(scale, v, bias); pixel = g > 0 ? (uint8) rintf(fminf(g, 255)) : 0, so a NaN
 *    reads 0; the pixel is appended to the receiver's pixel row; pixels++.
 * 5. Line structure, behind the strobe, all integer.  Carried: col, start, crossings, white, level
 *    (initially low), run, class, active.  If col == 0: start = m.  If pixel >= 192 and level is low:
 *    level = high, crossings++.  If pixel < 64: level = low.  If pixel >= 128: white++.  ++col.  When
 *    col == width the line ends: class = PDDC_FAX_START if start_lo <= crossings <= start_hi,
 *    PDDC_FAX_STOP if stop_lo <= crossings <= stop_hi, else 0; run = 0 for class 0, 1 for a class
 *    other than the previous line's, min(run + 1, 65535) for the same; if class is START and run ==
 *    need: active = 1, images++; if class is STOP and run == need: active = 0; the record {start,
 *    crossings, white, flags = class | (active ? PDDC_FAX_ACTIVE : 0), run} is emitted; lines++; col,
 *    crossings and white go to 0, the level stays.
 * Non-finite samples are data, in the receiver's own row alone.  A NaN or an infinity at sample p makes
 * y non-finite for p .. p + W - 1 wherever its tap is not zero (0 times infinity is NaN), w for one
 * sample more, and q turns every such f into NaN (without q two infinities would give a finite angle);
 * v is NaN while such an f is under the boxcar and the pixels read 0: W + box samples after p nothing
 * of it is left in f, the pixels or disc.  What the zero pixels did to crossings, white and the run of
 * the lines they fell into stays in those lines' records, as a fade would; acc and col never depend on
 * the data.  fminf never sees a NaN (g > 0 is false for one).
 * Receiver control.  An OFF receiver is not read and does not advance: its counts and npix are 0.
 * set_rx(rx, modem, flags) takes effect at the next batch's first sample.  RESTART, or a change from
 * OFF to ON: the carried inputs, y and f are zero, acc = 0, the level is low, col, the line in
 * progress, run, class and active are 0; the counters stay.  Another modem: the carried inputs, y, f,
 * acc and the level stay; col, the line in progress, run, class and active are 0.  reset() clears
 * everything and m, and synchronises the device.
 * Outputs of process(), all device memory, no host synchronisation: pix uint8 [nrx][pix_stride], the
 * pixels whose strobe lies in this batch, in order, with npix uint32 [nrx]; lines [nrx][line_stride],
 * the lines whose last pixel lies in this batch, with counts uint32 [nrx]; disc float32
 * [nrx][disc_stride] or NULL, f of every sample of the batch (an OFF receiver's row is not written):
 * a tuning display, and what a host AFC reads.
 * Capacity, host arithmetic.  n samples behind any acc hold at most ((n inc - 1) >> 32) + 1 strobes:
 * pddc_fax_max_pixels(f, n, &count) gives that for the bank's greatest inc, 0 for n = 0;
 * pddc_fax_max_lines gives (max_pixels - 1) div (the bank's least width) + 1, 0 for n = 0.  A
 * pix_stride or a line_stride below its bound is PDDC_ECAPACITY, and nothing is queued.  The kernel
 * never drops.
 * process(): every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned
 * pointer (z and lines 8 bytes, npix, counts and disc 4, pix 1; disc may be NULL; with n = 0 z, pix,
 * lines and disc are not looked at and npix and counts may be NULL), PDDC_ECAPACITY for a z_stride
 * or, with disc, a disc_stride below n or a stride below its bound, PDDC_EINVAL when an output's byte
 * range meets the input's.  n = 0 is valid: npix and counts, if given, are set to 0, nothing carried
 * moves, marks of set_rx stay for the next batch.  State moves only after the launch was accepted.
 * Stream-ordered; one stream per object, one thread at a time.
 * read(): per receiver lines, pixels and images (since create / reset), active, acc, col and f_last
 * (the last f computed, 0 before the first) behind the batches submitted so far (it waits for them),
 * as the next batch will find them.
 * Every bit of pix, npix, lines, counts, disc and the status is independent of the cut into batches
 * (n = 0 and n = 1 included), nrx, j's index, the other receivers, strides, grid and tile sizes.
 * create: argument errors before any device access (non-finite taps, a modem out of range,
 * overlapping tone ranges, a bad modem index, unknown flag bits); good arguments, no device:
 * PDDC_ENODEV.
 * The image (cutting the pixel row into lines by the records, finding the phasing pulse, rotating the
 * lines) is host work: Python's fax_image has it. */
#define PDDC_FAX_ON       0x1u
#define PDDC_FAX_REVERSE  0x2u   /* f negated: the receiver is tuned from the other side */
#define PDDC_FAX_RESTART  0x4u   /* set_rx: start this receiver afresh          */
#define PDDC_FAX_START    0x1    /* pddc_fax_line.flags: a start-tone line      */
#define PDDC_FAX_STOP     0x2    /* a stop-tone line                            */
#define PDDC_FAX_ACTIVE   0x4    /* an image is in progress behind this line    */
typedef struct pddc_fax_modem {
    uint32_t inc;         /* 1 .. 2^31: 2^32 width lpm / 60 / rate        */
    uint32_t width;       /* 16 .. 8192 pixels per line                   */
    uint32_t box;         /* 1 .. 16                                      */
    float scale, bias;    /* finite                                       */
    uint16_t start_lo, start_hi, stop_lo, stop_hi;   /* two ranges apart   */
    uint32_t need;        /* 1 .. 255                                     */
} pddc_fax_modem;
typedef struct pddc_fax_rx {
    int modem;            /* 0 .. nmodems - 1                             */
    uint32_t flags;       /* PDDC_FAX_ON | _REVERSE | _RESTART            */
} pddc_fax_rx;
typedef struct pddc_fax_line {
    uint64_t start;       /* sample index m of the strobe of the line's first pixel */
    uint16_t crossings;   /* low -> high crossings of the hysteresis      */
    uint16_t white;       /* pixels >= 128                                */
    uint16_t flags;       /* PDDC_FAX_START or _STOP, | _ACTIVE           */
    uint16_t run;         /* lines of this class in a row, this one counted */
} pddc_fax_line;
typedef struct pddc_fax_status {
    uint32_t lines, pixels, images;
    uint32_t active, acc, col;
    float f_last;
} pddc_fax_status;
typedef struct pddc_fax pddc_fax;
int pddc_fax_create(pddc_fax **out, int device, int nrx, int window, int nmodems,
                    const float *taps /* [nmodems][window] real; copied */,
                    const pddc_fax_modem *modems /* [nmodems] */, const pddc_fax_rx *rx /* [nrx] */);
int pddc_fax_destroy(pddc_fax *f);
int pddc_fax_reset(pddc_fax *f);                      /* m and everything carried; synchronises the device */
int pddc_fax_set_rx(pddc_fax *f, int rx, int modem, uint32_t flags);
int pddc_fax_max_pixels(const pddc_fax *f, size_t n, size_t *count);
int pddc_fax_max_lines(const pddc_fax *f, size_t n, size_t *count);
int pddc_fax_process(pddc_fax *f, const void *d_z, size_t n, size_t z_stride, void *d_pix, size_t pix_stride, void *d_npix,
                     void *d_lines, size_t line_stride, void *d_counts, void *d_disc, size_t disc_stride, void *stream);
/* status[nrx] after the batches submitted so far (it waits for them) */
int pddc_fax_read(pddc_fax *f, pddc_fax_status *host /* [nrx] */, void *stream);
/* samples per tile of the kernel's walk, from the batch's first (for tests that place batch cuts on its seams) */
int pddc_fax_tile_outputs(void);

/* ---- mfsk: M-tone FSK (2G ALE, MFSK16 / 8, the tone layer of Olivia and Contestia) symbols per receiver ----
 * Beside the chain, where fsk, morse, psk, sitor and fax sit: it reads the rows the tuner, blanker,
 * receiver filter and carrier write, and gives one record per symbol: the strongest tone, the second
 * strongest and how far apart they were.  What the symbols mean (2G ALE's words, an interleaver, a
 * Viterbi decoder) is host work.  Where this block is silent, psk's rules hold.
 * K receivers (1 .. 1024), a window length W (1 .. 256), a bank of B modems (1 .. 16), copied at
 * create.  Modem b: ntones, M in 2 .. 32; the matched filters h_k[W], k < M, complex float32 taps, in
 * taps[b][k][t] with PDDC_MFSK_MAX_TONES = 32 tone rows per modem whatever M is: every value of all 32
 * rows finite, the rows from M on not used; inc, uint32 in 1 .. 2^29: the symbol phase advanced per
 * sample, 2^32 baud / rate; q in 1 .. 64 with 4 q inc <= 2^32: the early and late offset in samples,
 * about a quarter symbol; step, uint32 in 0 .. inc: the clock correction per strobe, 0 is a fixed
 * clock.  Receiver j: a modem index and flags PDDC_MFSK_ON, _REVERSE, _RESTART.
 * Input per batch: z[j z_stride + i], i < n, complex float32, any row stride, n >= 0.  m counts the
 * object's samples since create / reset.  Every float operation below is one float32 operation in the
 * stated order, contraction off; the clock and the counter are integers.
 * 1. Tone powers, for every sample m of an ON receiver and k = 0 .. M-1: Y_k[m] = sum over t = 0 .. W-1
 *    of h_k[t] z[m - t], from (0, 0) with t ascending, per tap, with h = h_k[t] and z = z[m - t], fsk's
 *    four operations: re = fmaf(h.re, z.re, re); re = fmaf(-h.im, z.im, re); im = fmaf(h.re, z.im, im);
 *    im = fmaf(h.im, z.re, im).  p_k = fmaf(Y.im, Y.im, Y.re Y.re).
 * 2. Best and runner-up of the sample: from a = 0, b = +0, s = 0, r = +0, with k ascending: if p_k > b:
 *    r = b, s = a, b = p_k, a = k; otherwise, if p_k > r: r = p_k, s = k.  Ties keep the lower tone; a NaN
 *    power is never greater and is passed over.  a[m], b[m], s[m], r[m] at samples before the receiver's
 *    first are 0, +0, 0, +0.
 * 3. Clock.  Carried: acc, uint32, and skip, 0 or 1, both 0 at the start.  Each sample: a2 = acc + inc
 *    mod 2^32; a wrap iff a2 < acc; acc = a2.  A wrap with skip = 0 is a strobe; a wrap with skip = 1
 *    is none and clears skip.
 * 4. On a strobe at sample m, with c = m - q the on-time sample, e = m - 2 q the early one and m the
 *    late one: tone = a[c], second = s[c] (REVERSE: M - 1 - a[c] and M - 1 - s[c], the tones counted from
 *    the other end, for a receiver tuned from the other side); sum = b[c] + r[c]; quality = sum > 0 ?
 *    (b[c] - r[c]) / sum : 0, the division correctly rounded: 1 is one tone alone, 0 two tones alike.
 *    Clock correction, at every strobe: if b[m] > b[e], the peak lies later: if acc < step, skip = 1;
 *    acc = acc - step mod 2^32.  Otherwise, if b[e] > b[m]: acc = acc + step (no overflow: acc < inc
 *    behind a strobe).  A NaN moves nothing.  The late correction differs from psk's, which stops at
 *    acc = 0: behind a strobe acc < inc is the fraction of a sample the wrap overshot by, and a clock
 *    whose inc divides 2^32 (8 or 16 samples a symbol) has acc = 0 there for good -- it could be
 *    advanced and never delayed, and a sender 200 ppm slow walked out of its symbols.  Here a late
 *    correction larger than acc borrows from the next sample: acc goes below zero, that sample wraps
 *    it back to acc - step + inc >= 0, and skip keeps that wrap from being a strobe.  The correction is not gated on a tone change: where the tone stays, b is flat
 *    and the two sides differ by noise alone, which moves the clock either way; a transition on one side
 *    pushes away from it and the one on the other side pushes back, so on data that changes tone the
 *    strobe settles where both are as far as they can be, the symbol's middle plus q.
 *    The record {start = c, tone, second, flags = 0, quality} is emitted; symbols++.
 * Receiver control.  An OFF receiver is not read and does not advance: its count is 0 and its row of
 * best is +0.  set_rx(rx, modem, flags) takes effect at the next batch's first sample.  RESTART, a
 * change from OFF to ON and another modem do the same: the carried inputs and per-sample results are
 * zero and the clock (acc, skip) is as at create; the counter stays.  reset() clears everything and m, and
 * synchronises the device.
 * Outputs of process(), all device memory, no host synchronisation: syms [nrx][sym_stride], the records
 * of the strobes of this batch, in order (a record's start may lie up to q samples before the batch);
 * counts uint32 [nrx]; best float32 [nrx][best_stride] or NULL, b[m] of every sample of the batch, for
 * a tuning display.
 * Capacity, host arithmetic.  Behind a strobe acc <= inc - 1 + step (a late correction only puts the next
 * strobe off), so two strobes lie at least D_b =
 * floor((2^32 - step_b) / inc_b) samples apart ("MFSK decoder", derives it), D the least
 * over the bank: pddc_mfsk_max_syms(f, n, &count) gives (n - 1) div D + 1, 0 for n = 0.  A sym_stride
 * below it is PDDC_ECAPACITY, and nothing is queued.
 * process(): every argument is checked before anything is queued: PDDC_EINVAL for a NULL or misaligned
 * pointer (z and syms 8 bytes, counts and best 4; best may be NULL; with n = 0 z, syms and best are not
 * looked at beyond best's alignment and counts may be NULL), PDDC_ECAPACITY for a stride below n or
 * below the bound, PDDC_EINVAL when an output's byte range meets the input's.  n = 0 is valid: counts,
 * if given, is set to 0, nothing carried moves, marks of set_rx stay for the next batch.  State moves
 * only after the launch was accepted.  Stream-ordered; one stream per object, one thread at a time.
 * read(): per receiver symbols (since create / reset), acc and skip, and the last strobe's tone and quality
 * behind the batches submitted so far (it waits for them).
 * Every bit of syms, counts, best and the status is independent of the cut into batches (n = 0 and
 * n = 1 included), nrx, j's index, the other receivers, strides, grid and tile sizes.
 * Non-finite samples.  A NaN or an infinity in z[m0] stays in its receiver's row.  It is in the window
 * of the samples m0 .. m0 + W - 1: a tone whose taps meet it has a NaN or infinite power there (a NaN
 * is passed over by the maximum, +inf wins it), and b, r or both may be +inf or, where every tone is
 * NaN, +0 with tone 0.  Strobes at m <= m0 + W - 1 + 2 q read such samples: their quality may be NaN
 * (inf - inf, inf / inf) or 0 and their tone arbitrary; a comparison with a NaN moves nothing, one with
 * +inf moves the clock by step like any other.  From sample m0 + W + 2 q on, every value a strobe reads
 * is the one the clean series gives; what remains is the clock: acc differs by the corrections the
 * poisoned strobes made or missed, at most step each, and the loop pulls it back like any other timing
 * error.  The counter, the records' starts and the capacity bound hold whatever the samples are.
 * create: argument errors before any device access (non-finite taps, a modem out of range, a bad modem
 * index, unknown flag bits); good arguments, no device: PDDC_ENODEV. */
#define PDDC_MFSK_ON        0x1u
#define PDDC_MFSK_REVERSE   0x2u   /* tones counted from the other end              */
#define PDDC_MFSK_RESTART   0x4u   /* set_rx: start this receiver afresh            */
#define PDDC_MFSK_MAX_TONES 32     /* tone rows per modem in create's taps          */
typedef struct pddc_mfsk_modem {
    uint32_t ntones;      /* 2 .. 32                                      */
    uint32_t inc;         /* 1 .. 2^29: 2^32 baud / rate                  */
    uint32_t q;           /* 1 .. 64, 4 q inc <= 2^32                     */
    uint32_t step;        /* 0 .. inc                                     */
} pddc_mfsk_modem;
typedef struct pddc_mfsk_rx {
    int modem;            /* 0 .. nmodems - 1                             */
    uint32_t flags;       /* PDDC_MFSK_ON | _REVERSE | _RESTART           */
} pddc_mfsk_rx;
typedef struct pddc_mfsk_sym {
    uint64_t start;       /* sample index m of the symbol's on-time sample */
    uint8_t tone;         /* the strongest tone, 0 .. M - 1               */
    uint8_t second;       /* the second strongest                         */
    uint16_t flags;       /* 0 for now                                    */
    float quality;        /* (b - r) / (b + r) of the two                 */
} pddc_mfsk_sym;
typedef struct pddc_mfsk_status {
    uint32_t symbols;
    uint32_t acc, skip, tone_last;
    float q_last;
} pddc_mfsk_status;
typedef struct pddc_mfsk pddc_mfsk;
int pddc_mfsk_create(pddc_mfsk **out, int device, int nrx, int window, int nmodems,
                     const float *taps /* [nmodems][32][window] complex (re, im); copied */,
                     const pddc_mfsk_modem *modems /* [nmodems] */, const pddc_mfsk_rx *rx /* [nrx] */);
int pddc_mfsk_destroy(pddc_mfsk *f);
int pddc_mfsk_reset(pddc_mfsk *f);                    /* m and everything carried; synchronises the device */
int pddc_mfsk_set_rx(pddc_mfsk *f, int rx, int modem, uint32_t flags);
int pddc_mfsk_max_syms(const pddc_mfsk *f, size_t n, size_t *count);
int pddc_mfsk_process(pddc_mfsk *f, const void *d_z, size_t n, size_t z_stride, void *d_syms, size_t sym_stride,
                      void *d_counts, void *d_best, size_t best_stride, void *stream);
/* status[nrx] after the batches submitted so far (it waits for them) */
int pddc_mfsk_read(pddc_mfsk *f, pddc_mfsk_status *host /* [nrx] */, void *stream);
/* samples per tile of the kernel's walk, from the batch's first (for tests that place batch cuts on its seams) */
int pddc_mfsk_tile_outputs(void);

/* ---- measurement hooks (bench.py) ----------------------------------------- */
/* Times `iters` back-to-back launches of the pipeline's stage-0 kernel alone
 * with HIP events on `stream`; returns average milliseconds per launch.
 * State is not advanced (history taken as is).                                 */
int pddc_pipeline_time_stage0(pddc_pipeline *p, const void *d_packed, size_t nsamples,
                              void *d_out_f32, int iters, void *stream, float *avg_ms);

/* The same measurement INSIDE the caller's own loop: while enabled, every process() brackets its stage-0
 * (or fused-pair) kernel with a pair of HIP events on the caller's stream; pddc_pipeline_stage0_time waits for
 * them and returns the average kernel duration over the process() calls since it was enabled (or last read).
 * This is how bench.py gets the dominant kernel's duration over exactly its timed region.                  */
int pddc_pipeline_time_stage0_inline(pddc_pipeline *p, int enable);
int pddc_pipeline_stage0_time(pddc_pipeline *p, float *avg_ms, int *nlaunches);
/* The tile schedule a process() of nsamples would launch the fused stage-0 kernel with:
 * out = { inputs per tile, tiles, persistent blocks, S, K } -- block b first owns the S
 * tiles [b*S, (b+1)*S), the tiles from blocks*S on are handed out in chunks of K.  For
 * tests and bench.py, which place their comparison windows on these seams.           */
int pddc_pipeline_schedule(const pddc_pipeline *p, size_t nsamples, int out[5]);
/* Checkpoint / resume.  The stream state the reference never needed (its FPGA kept it): per stage the
 * FIR history and the decimation phase, the sample counter, the NCO word with its phase offset.  save:
 * one host blob (pddc_pipeline_state_size bytes), taken after everything pushed so far has completed.
 * restore: into a pipeline of the SAME plan and flags, on the same or another GPU -- the stream then
 * continues bit-identically (a receiver can move between GPUs, or survive a restart).             */
size_t pddc_pipeline_state_size(const pddc_pipeline *p);
int pddc_pipeline_save_state(pddc_pipeline *p, void *h_buf, size_t capacity, size_t *used);
int pddc_pipeline_restore_state(pddc_pipeline *p, const void *h_buf, size_t nbytes);
/* Test hook: the next process()/push fails with PDDC_EHIP when it reaches `stage`, after the stages
 * in front of it have been launched -- to show that a failure half way leaves the stream state
 * (histories, decimation phases, NCO counter) where it was and the batch can simply be retried.   */
int pddc_pipeline_inject_failure(pddc_pipeline *p, int stage);
/* Device-to-device streaming copy of nbytes (16 B per lane, nontemporal stores), `iters`
 * times, timed with HIP events on `stream`: the measured copy ceiling bench.py prints
 * next to the 8 TB/s spec figure (SURVEY.md 8d "Which roofline").  A copy moves
 * 2*nbytes through HBM.  Pointers and size: multiples of 16.                         */
int pddc_measure_copy(void *d_dst, const void *d_src, size_t nbytes, int iters, void *stream, float *avg_ms);

/* ---- multi-GPU: RCCL over xGMI (ddc_multi.cpp) --------------------------------
 * The reference models up to 8 receivers as 8 independent descriptors, each with
 * its own transfer queue and callback (perseus-sdr.c:43-47, perseus-in.h:87): the
 * stream shards as one receiver per GPU and the data path needs no collective.
 * What these calls carry between GPUs is the configuration (root -> all) and,
 * for BASELINE config 4, every GPU's decimated output to one root GPU.  They
 * stand where the reference has nothing (its receivers never talk to each other);
 * the hand-over point to the client stays perseus-in.c:206-207.
 *
 * One communicator rank per GPU.  pddc_comm_init_rank: one process per GPU -- rank 0
 * calls pddc_comm_get_unique_id and hands the 128 bytes to the others through
 * whatever started the processes (bench.py: the torch.distributed store).
 * pddc_comm_init_all: ONE process driving ndev GPUs (a C host holding several
 * perseus_descr); its collective calls -- one per communicator, same arguments --
 * go between pddc_comm_group_start() and pddc_comm_group_end().
 * All sizes in bytes.  Errors: PDDC_ECOMM + pddc_last_error().                  */
typedef struct pddc_comm pddc_comm;
#define PDDC_COMM_ID_BYTES 128
/* Version codes (ncclGetVersion style: major*10000 + minor*100 + patch) of the RCCL library bound at run time and of the
 * header this library was compiled against.  Every communicator constructor checks that the MAJOR versions agree and
 * fails with PDDC_ECOMM otherwise (two librccl can be on a box: /opt/rocm/lib and the one inside a torch wheel).   */
int pddc_comm_rccl_version(int *running, int *compiled);
int pddc_comm_get_unique_id(void *id128);
int pddc_comm_init_rank(pddc_comm **out, int nranks, int rank, const void *id128, int device);
int pddc_comm_init_all(pddc_comm **comms /* [ndev] */, int ndev, const int *devices /* NULL: 0..ndev-1 */);
int pddc_comm_destroy(pddc_comm *c);
int pddc_comm_rank(const pddc_comm *c);
int pddc_comm_size(const pddc_comm *c);
int pddc_comm_device(const pddc_comm *c);
int pddc_comm_group_start(void);
int pddc_comm_group_end(void);
/* root's d_buf -> everybody's d_buf (ncclBroadcast), asynchronous on `stream`     */
int pddc_comm_bcast(pddc_comm *c, void *d_buf, size_t nbytes, int root, void *stream);
/* the same for a host buffer, synchronous (one process per GPU only)              */
int pddc_comm_bcast_host(pddc_comm *c, void *h_buf, size_t nbytes, int root);
/* *h_val = max over ranks; pddc_comm_barrier = the same with nothing to say        */
int pddc_comm_allreduce_max_f64(pddc_comm *c, double *h_val);
int pddc_comm_barrier(pddc_comm *c);
/* Gather: every rank's nbytes at d_send land on the root at d_recv + rank*nbytes
 * (d_recv is read on the root only).  Grouped ncclSend/ncclRecv, peer -> root: the
 * root's xGMI links carry one peer each.  Asynchronous on `stream`.                */
int pddc_comm_gather(pddc_comm *c, const void *d_send, size_t nbytes, void *d_recv, int root, void *stream);
/* The same on the communicator's own side stream, started once everything queued on
 * `after_stream` so far (the kernels that wrote d_send) is done -- the transfer of
 * batch k then runs under the kernels of batch k+1.  Meant for TWO alternating send
 * buffers: pddc_comm_gather_fence(c, stream) makes `stream` wait for every transfer
 * but the most recent one -- call it before the kernels that overwrite the buffer
 * used two gathers ago; pddc_comm_gather_wait(c) makes the host wait for all of them
 * (before d_recv is read, or a buffer is freed).                                    */
int pddc_comm_gather_async(pddc_comm *c, const void *d_send, size_t nbytes, void *d_recv, int root,
                           void *after_stream);
int pddc_comm_gather_fence(pddc_comm *c, void *stream);
int pddc_comm_gather_wait(pddc_comm *c);

/* The configuration a broadcast carries: stage plan + taps + NCO word + flags, as one
 * flat little-endian buffer.  pack: returns the bytes used (buf == NULL: the bytes
 * needed), 0 on error.  unpack: stages[i].taps point INTO buf.                      */
size_t pddc_plan_pack(const pddc_stage_desc *stages, int nstages, uint32_t freg, uint32_t flags,
                      void *buf, size_t capacity);
int pddc_plan_unpack(const void *buf, size_t nbytes, pddc_stage_desc *stages /* [PDDC_MAX_STAGES] */,
                     int *nstages, uint32_t *freg, uint32_t *flags);
/* Root supplies the plan (others pass NULL/0); every rank gets a pipeline on its
 * communicator's GPU, created from the broadcast plan, NCO word set.                */
int pddc_comm_bcast_pipeline(pddc_comm *c, int root, const pddc_stage_desc *stages, int nstages,
                             uint32_t freg, uint32_t flags, pddc_pipeline **out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* PERSEUS_DDC_H */
