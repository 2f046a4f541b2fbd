/* lorahip.h -- C ABI of the MI355X-native LoRa demodulation hot path.
 *
 * Drop-in boundary for the part of myriadrf/LoRa-SDR that BASELINE.json's north_star
 * names: dechirp multiply -> 2^SF-point complex FFT -> |.|^2 arg-max / power / fractional
 * bin. Everything here is plain pointers and sizes; no exceptions cross the boundary,
 * every entry point returns LORAHIP_OK (0) or a negative LORAHIP_E_* code.
 * File:line citations are relative to the LoRa-SDR tree.
 *
 * Three levels, from the inner seam outwards:
 *
 *   1. lorahip_detector_*   one window, host buffers: exactly the semantics of
 *      `template<T> class LoRaDetector` (LoRaDetector.hpp:8-72) so LoRaDemod.cpp can
 *      swap `LoRaDetector<float> _detector` for a thin wrapper.
 *
 *   2. lorahip_detect_batch   many independent symbol windows per call (the data-parallel
 *      axis: channels x windows), device pointers, asynchronous on the context's stream.
 *      Per window it performs LoRaDemod.cpp:157-166 (dechirp with the chirp table and the
 *      fine-tune table, including the int<-float index recurrence) followed by
 *      LoRaDetector::detect (LoRaDetector.hpp:29-64 on kissfft.hh:77-157).
 *
 *   3. lorahip_demod_*   B channels of the `LoRaDemod` block (LoRaDemod.cpp:68-143 setters,
 *      :145-327 work()): same parameters (sf, sync, thresh, mtu), same 5-state frame
 *      machine, same int16 symbol packets; driven by a streaming kernel that walks every
 *      channel's stream on the device (SF6-12), or in lock-step from the host with one batch
 *      launch per work() round (lorahip_demod_set_mode).
 *
 * Around the path (each behind its own entry points further down): the batched modulator + AWGN channel
 * (lorahip_mod_frames, lorahip_add_awgn), the batched decoder (lorahip_decode_packets) with the packet hand-off
 * lorahip_demod_packets_to_device, and the front-end channeliser (lorahip_channelizer_*), which like the polyphase bank
 * (lorahip_pfb_*) also takes the integer samples a radio delivers (sc16, sc8: the *_run_iq entry points, LORAHIP_IQ_*). On the
 * transmit side the synthesiser (lorahip_synthesizer_*) and the polyphase synthesis bank (lorahip_psb_*) write the same integer
 * formats, quantised in the store, through their own *_run_iq entry points ("Integer IQ output" below).
 *
 * Results: symbol indices and FFT bins are bit-identical to the reference CPU path
 * compiled without FMA contraction (the kernels evaluate kissfft's radix-4/2 DIT graph
 * with kissfft's own float twiddles, op for op); power / powerAvg / fIndex agree to
 * float rounding of log10/hypot (tolerances in tests/).
 */
#ifndef LORAHIP_H
#define LORAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LORAHIP_OK             0
#define LORAHIP_E_INVALID     -1  /* bad argument (NULL, sf out of range, size mismatch)   */
#define LORAHIP_E_NODEVICE    -2  /* no HIP device / device index out of range             */
#define LORAHIP_E_HIP         -3  /* a HIP runtime call failed; see lorahip_last_error()    */
#define LORAHIP_E_NOMEM       -4  /* host or device allocation failed                       */
#define LORAHIP_E_ARCH        -5  /* device is not gfx950 (kernels are built for it only)   */

#define LORAHIP_SF_MIN  6
#define LORAHIP_SF_MAX 12
#define LORAHIP_FINE_STEPS 128     /* LoRaDemod.cpp:69 _fineSteps */

/* chirp selection per window */
#define LORAHIP_CHIRP_UP    0      /* _upChirpTable  = conj(entry)  LoRaDemod.cpp:103 (FRAMESYNC, DATASYMBOLS) */
#define LORAHIP_CHIRP_DOWN  1      /* _downChirpTable = entry       LoRaDemod.cpp:104 (DOWNCHIRP0/1)           */
#define LORAHIP_CHIRP_NONE  2      /* input is already dechirped: the LoRaDetector::feed seam (no dechirp loop:
                                      fine_idx0 / fine_err are ignored, fine_idx_out = fine_idx0)               */

const char *lorahip_strerror(int code);
const char *lorahip_last_error(void);       /* thread-local text of the last LORAHIP_E_HIP */
int lorahip_version(void);                  /* ABI version, currently 4 (1 -> 2: lorahip_work_result grew, level-3 ports and labels;
                                               2 -> 3, additions only: level-3 signals, append runs / lorahip_demod_receive, lorahip_rx_*;
                                               3 -> 4, additions only: lorahip_demod_receive_flush, _run_host_rows, _stream_wait / _stream_follow,
                                               _set_stream_lanes / _stream_lanes, _set_stream_grid, _set_variant, _set_record_capacity,
                                               lorahip_decode_packets_host, lorahip_decode_max_symbols, lorahip_decode_max_data_length, lorahip_demod_receive_signal_rows /
                                               _receive_num_signals: signals in receiver steps, pipelined ones included; async = 3: the resident receiver,
                                               lorahip_demod_resident_active, lorahip_demod_receive_steps) */
int lorahip_device_count(void);             /* number of usable gfx950 devices, 0 if none */
int lorahip_selfcheck(void);                /* host-only: the kernels' compile-time LDS layouts are consistent; no device needed */

/* -------------------------------------------------------------------------------------
 * Host-side tables, exactly the reference's expressions (no device needed):
 *   up/down : N cf32       LoRaDemod.cpp:97-107
 *   fine    : 128*N cf32   LoRaDemod.cpp:108-114
 *   twiddle : N cf32       kissfft.hh:17-22
 * Any pointer may be NULL. Buffers are interleaved (re,im) floats.
 * ------------------------------------------------------------------------------------- */
int lorahip_host_tables(int sf, float *up, float *down, float *fine, float *twiddle);

/* -------------------------------------------------------------------------------------
 * Level 2: batch context. One per (device, SF); not thread-safe (one host thread per
 * context, like one Pothos actor per block). Replaces: LoRaDemod ctor tables
 * (LoRaDemod.cpp:97-116) + LoRaDetector ctor (LoRaDetector.hpp:12-20) + kissfft ctor
 * (kissfft.hh:71-75).
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_ctx lorahip_ctx;

int lorahip_create(lorahip_ctx **ctx, int device, int sf);
void lorahip_destroy(lorahip_ctx *ctx);
int lorahip_sf(const lorahip_ctx *ctx);
/* Launch on an existing hipStream_t (e.g. torch's current stream) from now on. NULL is HIP's
 * null stream. Until this is called the context uses a private non-blocking stream. */
int lorahip_set_stream(lorahip_ctx *ctx, void *hip_stream);
int lorahip_reset_stream(lorahip_ctx *ctx);          /* back to the private stream */
int lorahip_synchronize(lorahip_ctx *ctx);

/* Kernel variant: 0 = auto (fastest validated for this SF), 1 = generic LDS kernel, 10 = the tuned kernel with every table in LDS.
 * These produce identical symbol indices and FFT bins (the reference's operation graph, no FMA).
 * LORAHIP_VARIANT_FMA (opt-in, level 2 only) is NOT one of them: the same tuned kernels with every complex multiply contracted to
 * one multiply + one FMA. Its bins differ from the CPU build's in the last place or two (far inside the 1e-4 relative tolerance
 * north_star states, symbol indices identical wherever the peak's margin exceeds that), and it is ~20 % fewer vector instructions.
 * It exists to measure what bit-exact bins cost (profiles/r04); nothing selects it by default and level 3 cannot reach it. */
#define LORAHIP_VARIANT_FMA 40
int lorahip_set_variant(lorahip_ctx *ctx, int variant);

/* How the kernels obtain _fineTuneTable[_fineTuneIndex] for windows whose index moves (LoRaDemod.cpp:159-162). Default (0): no
 * table read at all -- the index sequence in closed form, the entry as the product of two small fp64 factor tables held in LDS,
 * which the library has checked against all 128*N entries of the reference's table on this host (lorahip_fine_split_active() == 1;
 * if that check ever failed the tables are not built and the kernels read the table). 1: always read the table in HBM and walk
 * the index chain (the A/B switch; results are bit-identical either way). */
int lorahip_set_fine_gather(lorahip_ctx *ctx, int enable);
int lorahip_fine_split_active(const lorahip_ctx *ctx);
/* host-only self tests of the above (no device needed): 1 if the split reproduces every entry of the fine-tune table of `sf`;
 * the index sequence of one window as the kernels evaluate it (idx_out: N entries, *path = 1 closed form / 0 serial chain) */
int lorahip_fine_split_selftest(int sf);
int lorahip_fine_indices_host(int sf, int32_t idx0, float err, int32_t *idx_out, int32_t *idx_end, int32_t *path);

/* One batch of independent windows. All pointers are DEVICE pointers for
 * lorahip_detect_batch and HOST pointers for lorahip_detect_batch_host.
 *
 * Window w reads N = 2^sf cf32 samples starting at sample index
 *     offsets ? offsets[w] : w * window_stride
 * of `iq` (window_stride 0 means N: back-to-back windows).
 */
typedef struct lorahip_batch {
    size_t struct_size;          /* = sizeof(lorahip_batch), for ABI growth                      */
    /* inputs */
    const float *iq;             /* interleaved cf32 samples                                      */
    size_t n_windows;
    const int64_t *offsets;      /* optional per-window start sample                              */
    size_t window_stride;        /* used when offsets == NULL                                     */
    const int32_t *chirp_sel;    /* optional per-window LORAHIP_CHIRP_*; NULL -> chirp_sel_all    */
    int32_t chirp_sel_all;
    const int32_t *fine_idx0;    /* optional per-window _fineTuneIndex on entry (NULL -> 0)       */
    const float *fine_err;       /* optional per-window _finefreqError (NULL -> 0)                */
    /* outputs (sym/power/power_avg/f_index required, the rest optional) */
    uint16_t *sym;               /* detect() return value                LoRaDetector.hpp:63      */
    float *power;                /*                                      LoRaDetector.hpp:54      */
    float *power_avg;            /*                                      LoRaDetector.hpp:53      */
    float *f_index;              /*                                      LoRaDetector.hpp:56-61   */
    int32_t *fine_idx_out;       /* _fineTuneIndex after the N steps     LoRaDemod.cpp:160-162    */
    float *fft_out;              /* n_windows*N cf32, the "fft" port     LoRaDemod.cpp:154,172    */
    float *dec_out;              /* n_windows*N cf32, the "dec" port     LoRaDemod.cpp:164        */
} lorahip_batch;

int lorahip_detect_batch(lorahip_ctx *ctx, const lorahip_batch *b);       /* async, device ptrs */
/* The same with HOST pointers, synchronous: inputs are staged to the device, the call returns with the outputs filled.
 * `iq` must hold every sample a window reads, i.e. at least
 *     offsets ? max_w(offsets[w]) + N  :  (n_windows - 1) * (window_stride ? window_stride : N) + N
 * samples (that many are copied); offsets must be >= 0, fine_idx0 in [0, 128*N): LORAHIP_E_INVALID otherwise. */
int lorahip_detect_batch_host(lorahip_ctx *ctx, const lorahip_batch *b);

/* -------------------------------------------------------------------------------------
 * Mixed spreading factors in one call (BASELINE configs[3]: 16384 channels, SF = 7 + c mod 6). The reference runs one
 * LoRaDemod block per channel, each with its own SF (LoRaDemod.cpp:119); a launch here is uniform in N, so the scheduler buckets
 * the channels by SF, gives every bucket a level-2 context with its own HIP stream, issues the buckets' launches back to back
 * (they overlap on the device) and joins them on events. Results are bucket-major: the channels of the lowest SF first, each
 * bucket in ascending channel order; lorahip_mixed_rows() gives the row of every channel in the [rows][windows_per_channel]
 * arrays.
 *   create : SF of every channel (6..12)
 *   plan   : channel c's windows_per_channel back-to-back windows start at sample channel_offset[c] of the IQ buffer
 *   detect : asynchronous, device pointers, arrays of rows * windows_per_channel entries; the steady-state (up-chirp) shape
 *   synchronize : returns when every bucket's launch of the last detect has finished
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_mixed lorahip_mixed;
int lorahip_mixed_create(lorahip_mixed **m, int device, const int32_t *channel_sf, size_t n_channels);
void lorahip_mixed_destroy(lorahip_mixed *m);
size_t lorahip_mixed_num_buckets(const lorahip_mixed *m);
int lorahip_mixed_bucket(const lorahip_mixed *m, size_t i, int32_t *sf, size_t *first_row, size_t *n_channels);
/* bucket i's level-2 context, borrowed (owned by the scheduler): for lorahip_set_variant / timers / lorahip_timer_* on it */
lorahip_ctx *lorahip_mixed_context(const lorahip_mixed *m, size_t i);
int lorahip_mixed_rows(const lorahip_mixed *m, int64_t *row_of_channel);
int lorahip_mixed_plan(lorahip_mixed *m, const int64_t *channel_offset, size_t windows_per_channel);
int lorahip_mixed_detect(lorahip_mixed *m, const float *iq_dev, uint16_t *sym_dev, float *power_dev, float *power_avg_dev, float *f_index_dev);
int lorahip_mixed_synchronize(lorahip_mixed *m);

/* Several devices in one process ("one process, 8 devices, one host thread + stream per device"; the reference
 * runs one LoRaDemod block per channel, LoRaDemod.cpp:119-122, and nothing in it binds those channels to one GPU). Channels are
 * independent units, so there is no data-path collective: lorahip_mixed_create_multi splits the channels over devices[0..n_devices)
 * with lorahip_shard_plan, gives every device its own scheduler (above) and its own host thread that issues that device's launches.
 *   lorahip_shard_plan : host-only. SF buckets from the largest windows down, each cut into n_shards contiguous ranges; the
 *                        count % n_shards left-over channels of a bucket go to the shards holding the fewest bytes so far (weight
 *                        8*2^SF + 14 per window, lowest shard first among equals). The same rule as lora_sdr_amd/shard.py, which the
 *                        one-process-per-GPU form of the split (bench.py under torch.distributed) uses.
 *   create_multi       : devices may repeat (two shards on one GPU are two independent schedulers).
 *   plan               : as above, with channel_offset[c] relative to the IQ buffer of channel c's OWN device.
 *   rows               : channel c's row in the result arrays of its own device; lorahip_mixed_shard_of gives that device's index.
 *   detect_multi       : arrays of n_devices device pointers (entry s lives on devices[s]; entries of shards without channels are
 *                        ignored). Returns when every device's launches are issued; lorahip_mixed_synchronize joins all devices.
 *   lorahip_mixed_shard: shard s's single-device scheduler, borrowed (buckets, contexts, timers); NULL for a shard without channels.
 * On an object made by lorahip_mixed_create these report one shard; lorahip_mixed_detect refuses a multi-device object. */
int lorahip_shard_plan(const int32_t *channel_sf, size_t n_channels, size_t n_shards, int32_t *shard_of_channel);
int lorahip_mixed_create_multi(lorahip_mixed **m, const int *devices, size_t n_devices, const int32_t *channel_sf, size_t n_channels);
size_t lorahip_mixed_num_devices(const lorahip_mixed *m);
int lorahip_mixed_device(const lorahip_mixed *m, size_t shard, int32_t *device, size_t *n_channels);
lorahip_mixed *lorahip_mixed_shard(const lorahip_mixed *m, size_t shard);
int lorahip_mixed_shard_of(const lorahip_mixed *m, int32_t *shard_of_channel);
int lorahip_mixed_detect_multi(lorahip_mixed *m, const float *const *iq_dev, uint16_t *const *sym_dev, float *const *power_dev,
                               float *const *power_avg_dev, float *const *f_index_dev);

/* Pinned host memory for the host-pointer entry points (lorahip_detect_batch_host, lorahip_demod_run, the detector shim): buffers
 * obtained here -- or any hipHostMalloc'ed / hipHostRegister'ed memory -- are read by the DMA engine directly; ordinary memory is
 * gathered through the library's double-buffered pinned staging first (several threads, LORAHIP_UPLOAD_THREADS). NULL on failure. */
void *lorahip_host_alloc(size_t bytes);
void lorahip_host_free(void *p);

/* Time the last `n` launches made through this context between two internal HIP events
 * recorded on the launch stream (bench.py uses this for the roofline line). */
int lorahip_timer_start(lorahip_ctx *ctx);
int lorahip_timer_stop(lorahip_ctx *ctx, float *elapsed_ms);

/* -------------------------------------------------------------------------------------
 * Level 1: LoRaDetector<float> shim (LoRaDetector.hpp:8-72). N must be 2^sf with sf in
 * [LORAHIP_SF_MIN, LORAHIP_SF_MAX]. The object keeps the window (feed() writes it), the bins and
 * detect()'s results in one block of pinned host memory that the device addresses directly:
 * a detect() is one kernel launch and one wait (~19 us; no staged copies). One object is
 * used by one thread at a time, as the reference's detector is.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_detector lorahip_detector;

int lorahip_detector_create(lorahip_detector **det, int device, size_t N);   /* LoRaDetector(N)  :12 */
void lorahip_detector_destroy(lorahip_detector *det);
int lorahip_detector_feed(lorahip_detector *det, size_t i, float re, float im); /* feed()       :23 */
/* detect(): returns the arg-max bin through *index; fft_out may be NULL (:29-64) */
int lorahip_detector_detect(lorahip_detector *det, size_t *index, float *power, float *power_avg,
                            float *f_index, float *fft_out);

/* -------------------------------------------------------------------------------------
 * Level 3: B channels of the LoRaDemod block (declared here, see lorahip_demod.cpp and the lorahip_demod_*.cpp units beside it).
 *
 * What "identical to the reference block" means here: symbol values and FFT bins are bit-exact by construction; power, powerAvg and
 * fIndex equal the CPU build's to float rounding (<= 2e-5 dB / 2e-6 bins: the logarithms and the fp64 sum are evaluated in a
 * different order), and the frame machine consumes them (`snr < thresh`, `_finefreqError += fIndex`, LoRaDemod.cpp:173-174,219).
 * A value within that rounding of a decision boundary could therefore take the other branch than the CPU build; every trace the
 * tests compare is identical, but at this level the guarantee is empirical.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_demod lorahip_demod;

int lorahip_demod_create(lorahip_demod **d, int device, int sf, size_t n_channels); /* make(sf) LoRaDemod.cpp:119 */
void lorahip_demod_destroy(lorahip_demod *d);
/* One level-3 object whose channels each have their own SF, over several devices of the node: what n_channels calls of the
 * reference's make(sf) with different sf give a flow graph (LoRaDemod.cpp:119-122), as ONE handle (BASELINE configs[3]: 16384
 * channels, SF 7..12, 8 GPUs). lorahip_shard_plan assigns every channel a device (devices[] may repeat: two shards on one GPU); on
 * each device the channels of one SF form a PART -- a plain single-SF object with its own context, HIP stream and host thread, so
 * the parts of a device overlap on it and the devices run side by side; there is no data-path collective. Every lorahip_demod_*
 * setter and accessor works on the handle with GLOBAL channel numbers (packets, signals, traces, labels, consumed); the packet
 * queue lists the parts one after the other (device slot ascending, SF ascending inside one), each in its own order. Runs:
 *   lorahip_demod_run                       one host buffer per channel (any SF mix, any number of devices)
 *   lorahip_demod_run_device_segments       all channels' segments in ONE device buffer (objects on one device)
 *   lorahip_demod_run_device_segments_multi iq_dev[n_devices]: channel c's segment lies in the buffer of ITS device slot
 *                                           (lorahip_demod_part_of / lorahip_demod_part say which)
 * lorahip_demod_packets_to_device works on a handle whose parts all lie on ONE device (several slots naming it count as one): the rows
 * of all parts in the queue's order, global channel numbers in channel_dev, for ONE lorahip_decode_packets_cfgs launch whose table says
 * "configuration of channel".
 * Not offered on such a handle (LORAHIP_E_INVALID; use the part's own handle, lorahip_demod_part_handle): lorahip_demod_run_device,
 * the append runs and receiver steps, lorahip_demod_packets_to_device and lorahip_demod_set_stream when the object spans several
 * devices (the rows of one decoder launch live on one device); debug ports only for one SF and host buffers. lorahip_demod_kernel_ms / _last_launches report the maximum
 * over the parts, lorahip_demod_work_calls / _near_threshold the sums. On a plain object the part accessors report one part. */
int lorahip_demod_create_mixed(lorahip_demod **d, const int *devices, size_t n_devices, const int32_t *channel_sf, size_t n_channels);
size_t lorahip_demod_num_channels(const lorahip_demod *d);
size_t lorahip_demod_num_parts(const lorahip_demod *d);
int lorahip_demod_part(const lorahip_demod *d, size_t i, int32_t *device, int32_t *sf, size_t *n_channels, int32_t *device_slot);
int lorahip_demod_part_of(const lorahip_demod *d, int32_t *part_of_channel, int32_t *local_channel);   /* [n_channels] each, nullable */
lorahip_demod *lorahip_demod_part_handle(const lorahip_demod *d, size_t i);                             /* borrowed */
int lorahip_demod_set_sync(lorahip_demod *d, unsigned char sync);        /* setSync       :124 */
int lorahip_demod_set_threshold(lorahip_demod *d, double thresh_dB);     /* setThreshold  :129 */
int lorahip_demod_set_mtu(lorahip_demod *d, size_t mtu);                 /* setMTU        :134 */
int lorahip_demod_activate(lorahip_demod *d);                            /* activate()    :139 */
/* How work() rounds are driven: 0 = auto (1 where a streaming kernel exists for the SF, else 2),
 * 1 = on the device: one streaming kernel walks every channel's stream window after window with the frame
 *     machine (LoRaDemod.cpp:176-312) in registers; no host round trip between the windows of a channel,
 * 2 = from the host: one batch launch per lock-step round, the frame machine on the host between launches.
 * Both produce identical packets, traces and signals. */
int lorahip_demod_set_mode(lorahip_demod *d, int mode);
/* Launch on an existing hipStream_t from now on (same meaning as lorahip_set_stream): work queued on that stream before a
 * run -- a channeliser, a modulator, a copy -- is ordered before the run's kernels. A run returns with the stream drained. */
int lorahip_demod_set_stream(lorahip_demod *d, void *hip_stream);
/* Make `hip_stream` (a hipStream_t of the object's device; NULL = the null stream) wait for everything queued so far on the object's
 * launch stream: the way a consumer on a stream of its own reads rows that are "valid in stream order on the launch stream"
 * (lorahip_demod_receive with async = 1 or 2). Costs an event record and a stream wait; allowed while a pipelined step is in flight. */
int lorahip_demod_stream_wait(lorahip_demod *d, void *hip_stream);
/* The other direction: the object's launch stream waits for everything queued so far on `hip_stream` -- the producer of the samples,
 * or a consumer of rows that the next pipelined step will overwrite -- without a host wait. */
int lorahip_demod_stream_follow(lorahip_demod *d, void *hip_stream);
int lorahip_demod_reset_stream(lorahip_demod *d);    /* back to the private stream */
/* kernel variant of the host-driven mode's batch launches (lorahip_set_variant: 0, 1, 10 -- identical results); LORAHIP_VARIANT_FMA
 * is refused (LORAHIP_E_INVALID): level 3 runs the reference's operation graph only */
int lorahip_demod_set_variant(lorahip_demod *d, int variant);
/* The streaming kernels' grid (scheduling only: every result is the same). 0 = the library's choice (one workgroup per channel set;
 * at SF11 the resident number of workgroups, each walking channel after channel: lorahip_stream_wide.hip), < 0 = one workgroup per
 * channel set always, n > 0 = at most n workgroups each walking several sets -- honoured where the build holds such an instance
 * (SF11 and SF12), the default elsewhere. For measurements and tests. */
int lorahip_demod_set_stream_grid(lorahip_demod *d, int max_workgroups);
/* Lanes per channel of the streaming kernels at SF7-9 (scheduling only: every result is the same). A channel is a sequential chain of
 * work() calls; the default geometry gives a lane 16 points of the window (SF7: 8 lanes per channel), which is the cheapest per
 * window and fills the device from 16384 (SF7) / 8192 (SF8) / 4096 (SF9) channels up. A receiver with fewer channels leaves
 * wavefront slots empty, so the library then gives a channel 2x / 4x / 8x the lanes (8 or 4 points per lane: shorter calls, more
 * wavefronts). log2_lanes: 0 = chosen by the channel count (default), < 0 = 16 points per lane always, 4 / 5 / 6 = 16 / 32 / 64 lanes
 * per channel where the build holds that instance (SF7: 4, 5; SF8: 5, 6; SF9: 6), the default geometry elsewhere. For measurements
 * and tests.
 * 16 | l (l = 3, 4, 5: SF7; 4, 5: SF8; 5: SF9): a channel takes TWO groups of 2^l lanes, and the second evaluates the window the NEXT
 * work() call will read if this one consumes exactly N samples and leaves the fine-tune state where a plain call leaves it (inside a
 * packet, on a quiet or aligned FRAMESYNC call, on the first down-chirp); the frame machine makes that second call in the same pass
 * when it finds the channel exactly there, and drops the window otherwise. Chosen by the library only at SF7 with at most half as many
 * channels as the device holds wavefronts at two per SIMD (1024 on an MI355X), where it is worth 4 - 8 %.
 * The parts of a mixed object (lorahip_demod_create_mixed) run side by side on their device: where the choice is the library's, a
 * part counts the wavefronts its sibling parts bring (at 16 points per lane) as taken, and widens only into what is left. */
int lorahip_demod_set_stream_lanes(lorahip_demod *d, int log2_lanes);
/* log2 of the lanes per channel the object's streaming launches run on (the choice above resolved for its channel count and device;
 * SF11 / SF12: 7 / 8, a channel is a workgroup); LORAHIP_E_INVALID for a mixed object (per part: lorahip_demod_part_handle) */
int lorahip_demod_stream_lanes(const lorahip_demod *d);
/* A bound on the streaming kernels' per-launch record capacity (work() calls per channel per launch; 0 = none beyond the library's
 * own sizing). A channel that fills its records stops, and the run resumes it with another launch: results are the same. For tests
 * of that path (it replaces the environment hook LORAHIP_STREAM_CAP of earlier builds). */
int lorahip_demod_set_record_capacity(lorahip_demod *d, size_t max_calls_per_launch);
/* same switch as lorahip_set_fine_gather, for the demodulator's kernels */
int lorahip_demod_set_fine_gather(lorahip_demod *d, int enable);

/* Per-channel outcome of one work() round (what the block would have done on its ports). */
typedef struct lorahip_work_result {
    int64_t consumed;       /* inPort->consume(total)                          :320 */
    int32_t state_before;   /* 0 FRAMESYNC 1 DOWNCHIRP0 2 DOWNCHIRP1 3 QUARTERCHIRP 4 DATASYMBOLS */
    int32_t value;          /* detect() of window 0                            :172 */
    float power, power_avg, snr, f_index;
    int32_t worked;         /* 0 if fewer than 2N samples were available       :148 */
    int32_t packet_len;     /* >0: a packet of that many int16 symbols was posted this round :295-298 */
    int32_t signals;        /* 1 at DOWNCHIRP1: error/power/snr emitted        :267-269 */
    int32_t sig_error;
    float sig_power, sig_snr;
    /* the dechirp state of this call (LoRaDemod.cpp:157-166): what lorahip_demod_get_ports() replays the debug ports from */
    int32_t fine_idx_before;   /* _fineTuneIndex when the call began                                          */
    int32_t fine_idx_after;    /* ... after the N steps of window 0 (where the sync check's window 1 starts :191) */
    float fine_err_before;     /* _finefreqError when the call began                                          */
    int32_t reserved;
} lorahip_work_result;

/* Feed every channel's whole stream (host memory, cf32, n_samples[c] samples each) and run
 * work() rounds in lock-step until no channel has 2N samples left. Packets are appended to
 * the demod's queue. Returns the number of rounds through *rounds (may be NULL). */
int lorahip_demod_run(lorahip_demod *d, const float *const *streams, const size_t *n_samples,
                      int64_t *rounds);
/* Same, but `iq` is one DEVICE buffer holding n_channels streams of samples_per_channel each. */
int lorahip_demod_run_device(lorahip_demod *d, const float *iq_dev, size_t samples_per_channel,
                             int64_t *rounds);
/* Same for a caller that keeps its channels' samples in ONE device buffer at places of its own -- the running receiver behind a
 * channeliser: channel c's stream is the n_samples[c] samples that start at sample first_sample[c] of iq_dev (HOST arrays of
 * n_channels entries; segments may have any lengths, including 0, and need not be ordered). work() leaves fewer than 2N samples
 * of a channel unconsumed (LoRaDemod.cpp:148) and how many it consumed differs from channel to channel (lorahip_demod_consumed), so
 * a caller that appends each new chunk behind the last one advances first_sample[c] by what channel c consumed and presents the
 * remainder together with the new samples -- nothing is copied, nothing is lost at the chunk boundaries. */
int lorahip_demod_run_device_segments(lorahip_demod *d, const float *iq_dev, const int64_t *first_sample, const size_t *n_samples,
                                      int64_t *rounds);
/* HOST buffers that are the rows of ONE block of host memory: channel c's n_samples[c] samples begin at sample first_sample[c] of row c
 * (rows + 2 * c * row_stride floats), first_sample[c] + n_samples[c] <= row_stride. What a framework hands a block whose input buffer
 * manager carves every port's slabs out of one pinned allocation (lorahip_host_alloc; lora_sdr_amd/pothos/LoRaDemodBatch.cpp::
 * getInputBufferManager, the counterpart of LoRaDemod.cpp:346-357): the span of the rows that holds samples crosses PCIe as ONE strided
 * copy straight from the caller's memory -- no staging copy, no per-channel call -- and the run reads per-channel segments of the
 * device copy. Results as lorahip_demod_run on the same samples; synchronous (the rows are the caller's again on return). Ordinary
 * memory works too (the runtime stages it). An object over several parts takes its channels' buffers one by one (lorahip_demod_run). */
int lorahip_demod_run_host_rows(lorahip_demod *d, const float *rows, size_t row_stride, const int64_t *first_sample, const size_t *n_samples,
                                int64_t *rounds);
/* the same for an object that spans several devices (lorahip_demod_create_mixed): one buffer per entry of its device list */
int lorahip_demod_run_device_segments_multi(lorahip_demod *d, const float *const *iq_dev, size_t n_devices, const int64_t *first_sample,
                                            const size_t *n_samples, int64_t *rounds);

/* The RUNNING receiver: channel c's stream is row c of a (n_channels, row_stride) device array of which the first n_valid samples
 * are valid -- a capture, or the output array of a channeliser, that fills chunk by chunk. Each call is one work() of every channel
 * over what has arrived: a channel continues at ITS OWN read position (work() leaves fewer than 2N samples of it unconsumed,
 * LoRaDemod.cpp:148; the positions live on the device, nothing is uploaded per call), its frame machine, fine-tune state and any
 * open packet carry over. n_valid must not shrink from call to call; lorahip_demod_rewind() -- or any other kind of run -- starts
 * new streams at sample 0. After an append run lorahip_demod_consumed() is the channel's absolute read position in its row and the
 * packets' `round` counts the channel's work() calls since the streams began. */
int lorahip_demod_run_device_append(lorahip_demod *d, const float *iq_dev, size_t row_stride, size_t n_valid, int64_t *rounds);
int lorahip_demod_rewind(lorahip_demod *d);
/* One receiver step in ONE call: lorahip_demod_run_device_append, then the packets that completed -- those begun in earlier calls
 * included -- packed ON THE DEVICE into the batched decoder's rows (as lorahip_demod_packets_to_device, rows numbered there too:
 * no upload, no host copy of any symbol), then the queue cleared. *n_packets = packets delivered (LORAHIP_E_INVALID and the packets
 * left queued if that exceeds cap_packets), *work_calls = LoRaDemod::work() calls made by this step, summed over the channels.
 * With async = 1 the call returns without waiting for the packing kernels: the rows are valid in stream order on the object's
 * launch stream (lorahip_demod_set_stream), which is where a decoder that follows would be queued. Signals kept by
 * lorahip_demod_set_signals go to the rows registered with lorahip_demod_receive_signal_rows (below); without such rows they are dropped.
 * With async = 2 the steps are PIPELINED: this step's kernel is launched before the previous step's summary is read, so the host's
 * share of a step (launch latencies, the wait for the summary, the packing launches: ~60 us) overlaps the kernel instead of
 * following it. The price is one step of latency: *n_packets / *work_calls and the rows are those of the PREVIOUS step (0 for the
 * first), valid in stream order on the object's launch stream like with async = 1 (short steps are packed on a side stream beside
 * the running kernel; the launch stream waits for that before anything later); lorahip_demod_receive_flush() delivers the last
 * step's and leaves the pipeline. The first call after anything else touched
 * the object is an ordinary step (its packets delivered at once). While a step is in flight every other entry point that needs the
 * object's state returns LORAHIP_E_INVALID ("flush first"); no trace / ports in this mode (signals: lorahip_demod_receive_signal_rows).
 * Rows that cannot hold the packets that are due (cap_packets too small, null pointers) lose NOTHING: the call returns
 * LORAHIP_E_INVALID with *n_packets = the rows needed, the packets stay in the step's record set on the device, and the next
 * lorahip_demod_receive / _flush whose rows hold them delivers them first, together with the packets of the step launched in
 * between (*n_packets and *work_calls then cover both steps; until then no further kernel is launched -- the samples wait in the
 * caller's array, a later call covers them). As with async = 0/1 a packet longer than sym_stride keeps its true length in
 * nsyms_dev and its first sym_stride symbols (the decoder flags it): sym_stride >= the MTU never truncates.
 * With async = 3 the receiver is RESIDENT (SF7-12; the grid is at most the device's resident set of workgroups, each taking as many
 * channel sets per step as it takes to cover the channels; until the object is in place for it -- the first call of a capture -- the
 * call is an ordinary step): ONE kernel launch stays on the device across the steps. A call copies a 104-byte message into a ring in device memory (the doorbell) and
 * returns the counts of the PREVIOUS step; the kernel's wavefronts poll the ring, work through what arrived with the tables they
 * staged once, pack their own channels' packets (and signals, lorahip_demod_receive_signal_rows) themselves into the rows that came
 * WITH the step's call, and the last workgroup reports two words to pinned host memory: no launch, no helper kernel per step. So: the rows
 * passed to call k are filled by step k and are complete -- in memory, for any stream, a copy engine or, if they are pinned host
 * memory, the host -- when call k + 1 (or lorahip_demod_receive_flush) returns with their *n_packets; keep two sets of rows and
 * alternate (with a depth d > 1, `reserved` below: call k + d reports them, d + 1 sets). Rows are handed out in the order the wavefronts finish: a channel's packets of a step are consecutive and in time order,
 * channels are not sorted (channel_dev says whose a row is). The samples up to n_valid must BE in iq_dev when the call is made (the
 * kernel reads them on its own, not in the order of any stream). Rows too small for a step: the excess is dropped, counted in
 * *n_packets, and the call that reports the step returns LORAHIP_E_INVALID -- size the rows for a step (one packet per channel and
 * frame that can end in it). While the kernel is resident it holds the wavefront slots of its channels -- on a full device nothing else
 * runs until the flush, and a DEVICE-wide synchronise (hipDeviceSynchronize) waits for it --, every other entry point that needs the
 * object returns LORAHIP_E_INVALID, and every wait is bounded: a
 * wavefront that sees no message for 8 s leaves, a host call that sees no report for 5 s tells the kernel to leave and fails (the
 * object then takes ordinary steps). The launch is sized for an EMPTY device: a second object (another part of a mixed receiver, another
 * process) asking for a resident kernel while the first holds the device's slots finds its census incomplete after 2 s, ends its launch and
 * takes ordinary steps from then on -- one resident receiver per device at a time. lorahip_demod_receive_flush(d, rows, ..) reports the
 * last step, ends the kernel and leaves the
 * object as a streaming run leaves it.
 * Ordering of the rows: a step's packets are written in stream order AFTER everything that was queued on the launch stream when
 * the call began, so a consumer (decoder) of the rows handed out by the call before, queued on that stream (or on a stream the
 * launch stream was told to follow before the call, lorahip_demod_stream_follow), has read them before they are overwritten -- one
 * set of rows is enough. lorahip_demod_receive_flush also resumes a channel whose record capacity the
 * last step filled (that step's remaining packets follow the others in the rows). */
/* WHEN a packet arrived, in samples of its channel's stream (all int64 from the kernel's registers to the row; never narrowed).
 * With consumed[i] what call i of LoRaDemod::work() consumes and P(i) = consumed[0] + .. + consumed[i-1], for a packet posted by call k
 * whose frame's DOWNCHIRP1 call is j and whose first DATASYMBOLS call is m:
 *   end_pos    P(k + 1): just after the posting call -- the "RX finished" instant (Semtech's tmst)
 *   data_pos   P(m): first sample of the first data symbol            = end_pos - len * N
 *   sync_pos   P(j): start of the call that emits the frame's signals  = data_pos - (N/4 + freq_error/2) - N   (int division)
 *   freq_error the "error" that call j emits (LoRaDemod.cpp:265-267)
 * The kernels record end_pos and freq_error at the post; the identities hold because every DATASYMBOLS call consumes N, QUARTERCHIRP
 * N/4 + freqError/2, DOWNCHIRP1 N, and freqError does not change from DOWNCHIRP1 to the post. A signal's position (below) is P(j), so
 * (channel, sync_pos) == (channel, pos) joins a packet with its signal exactly.
 * Origin: that of lorahip_demod_consumed -- one-shot runs (lorahip_demod_run*, the segment runs) count from the first sample the run
 * was given for the channel (a caller of the segment runs adds its first_sample[c]; a packet begun in an earlier one-shot run has
 * data_pos / sync_pos below 0), append runs and receiver steps count absolute positions in the channel's row since the last
 * lorahip_demod_rewind. To answer an uplink: lorahip_mod_frames_sched(start = end_pos + delay). */
typedef struct lorahip_rx_info { int64_t end_pos, data_pos, sync_pos, freq_error; } lorahip_rx_info;

/* Versioned by struct_size: the size up to and including `reserved` (before info_dev existed) is accepted and means "no info_dev".
 * info_dev (nullable): [cap_packets] lorahip_rx_info per packet row, device memory, filled in the same stream order as the other rows
 * by ordinary (async 0 / 1) and pipelined (async 2) steps; rows too small lose nothing, the info arrives with the re-delivery. A
 * RESIDENT step (async 3) does not deliver it: a call whose rows carry info_dev, or whose registered signal rows carry pos, is refused
 * with LORAHIP_E_INVALID before anything is rung (lorahip_last_error() says so); the object stays usable for ordinary steps. */
typedef struct lorahip_packet_rows {
    size_t struct_size;     /* = sizeof(lorahip_packet_rows) */
    uint16_t *syms_dev; size_t sym_stride;      /* [cap_packets][sym_stride], zero padded */
    int32_t *nsyms_dev;                          /* [cap_packets] */
    int32_t *channel_dev;                        /* [cap_packets], nullable */
    size_t cap_packets;
    int32_t async;          /* 0 wait, 1 rows valid in stream order, 2 pipelined, 3 resident (see above) */
    int32_t reserved;       /* async = 3, at the call that starts the resident kernel: the DEPTH, 0 / 1 (default) .. 3 -- how many steps the
                               receiver may run ahead of the last report. Call k then reports step k - depth (the rows of call k - depth),
                               the flush everything left, and the caller cycles depth + 1 sets of rows. A step ends with its slowest
                               workgroup; with more steps in flight the fast ones work ahead instead of waiting for it. Otherwise 0. */
    lorahip_rx_info *info_dev;                   /* [cap_packets], nullable (see above); absent in the previous struct_size */
} lorahip_packet_rows;
#define LORAHIP_PACKET_ROWS_SIZE_V4 (offsetof(lorahip_packet_rows, info_dev))
int lorahip_demod_receive(lorahip_demod *d, const float *iq_dev, size_t row_stride, size_t n_valid, const lorahip_packet_rows *rows,
                          size_t *n_packets, int64_t *work_calls);
/* The block's signals in a running receiver (the reference emits "error" / "power" / "snr" once per packet at DOWNCHIRP1, LoRaDemod.cpp:
 * 267-269). With lorahip_demod_set_signals(d, 1) AND rows registered here, every lorahip_demod_receive / _receive_flush call delivers
 * the signals of the step whose packets it delivers -- ordinary steps at once, pipelined steps (async = 2) one step late, beside the
 * packets -- into rows [0, n), n = lorahip_demod_receive_num_signals(d): channel, error, power, snr per emission, channels ascending
 * and time ascending inside a channel, written in the same stream order as the packet rows. The arrays may be device memory or pinned
 * host memory (lorahip_host_alloc), which the device writes directly -- what a host consumer (a block's emitSignal) reads after the
 * stream has passed; any array may be NULL. A step emits at most one signal per packet it completes plus one per channel (a frame whose
 * packet is still open): cap >= cap_packets + n_channels always suffices. Rows that cannot hold what is due lose nothing: the call
 * returns LORAHIP_E_INVALID exactly as for packet rows that are too small (pipelined: packets and signals stay in the step's record
 * set; ordinary: they stay queued for lorahip_demod_get_packets / _get_signals). rows = NULL (or no rows registered): receiver steps
 * drop the signals, as before version 4. The registration may be changed before any call, steps in flight or not (it is two pointers
 * and a count): a caller that alternates two sets of packet rows alternates two sets of signal rows the same way. The signals a call
 * delivers go where the registration stood AT that call (ordinary and pipelined steps); a RESIDENT step's signals go, like its packets,
 * where the registration stood when the step was rung, and are complete when the next call reports them. */
typedef struct lorahip_signal_rows {
    size_t struct_size;     /* = sizeof(lorahip_signal_rows) */
    int32_t *channel;       /* [cap] */
    int32_t *error;         /* [cap]  "error": the frequency error in bins (int)      :267 */
    float *power;           /* [cap]  "power"                                         :268 */
    float *snr;             /* [cap]  "snr"                                           :269 */
    size_t cap;
    int64_t *pos;           /* [cap]  nullable: where the emitting call began (= lorahip_rx_info::sync_pos of the frame's packet); device or
                               pinned host memory like its siblings. Absent in the previous struct_size (the size up to `cap`), which is
                               still accepted. */
} lorahip_signal_rows;
#define LORAHIP_SIGNAL_ROWS_SIZE_V4 (offsetof(lorahip_signal_rows, pos))
int lorahip_demod_receive_signal_rows(lorahip_demod *d, const lorahip_signal_rows *rows /* nullable */);
size_t lorahip_demod_receive_num_signals(const lorahip_demod *d);
int lorahip_demod_receive_flush(lorahip_demod *d, const lorahip_packet_rows *rows /* nullable: the last step's packets are dropped */,
                                size_t *n_packets, int64_t *work_calls);
int lorahip_demod_resident_active(const lorahip_demod *d);      /* 1 while the resident kernel (async = 3) is on the device */
/* The resident steps the LAST receive / flush call reported, oldest first: packets[i] / signals[i] of each (the call's *n_packets is
 * their sum). A receive call reports at most one; a flush at a depth d > 1 up to d, each in the rows of its own call. Returns how many. */
size_t lorahip_demod_receive_steps(const lorahip_demod *d, size_t *packets, size_t *signals, size_t cap);

/* The block's signals "error" (int), "power" (float), "snr" (float), emitted once per packet at DOWNCHIRP1 (LoRaDemod.cpp:85-87,
 * 267-269), WITHOUT a per-call trace: with enable = 1 the following runs keep one record per emission -- the kernels evaluate
 * power / snr for that one call of a packet, nothing else changes -- queued like the packets (channels ascending, time ascending
 * inside a channel after a streaming run) and cleared with them by lorahip_demod_clear_packets. `rounds` as for packets. Off by
 * default. Values equal the traced run's sig_error / sig_power / sig_snr. */
int lorahip_demod_set_signals(lorahip_demod *d, int enable);
size_t lorahip_demod_num_signals(const lorahip_demod *d);
int lorahip_demod_get_signals(const lorahip_demod *d, int32_t *channels, int64_t *rounds, int32_t *errors, float *powers, float *snrs, size_t cap);

size_t lorahip_demod_num_packets(const lorahip_demod *d);
/* packet i: channel, round index it was posted in, and length; symbols copied if out != NULL */
int lorahip_demod_get_packet(const lorahip_demod *d, size_t i, int32_t *channel, int64_t *round,
                             size_t *len, int16_t *out, size_t cap);
/* all queued packets at once, in posting order: per packet channel / round / length, and the symbols back to back */
size_t lorahip_demod_num_packet_symbols(const lorahip_demod *d);
int lorahip_demod_get_packets(const lorahip_demod *d, int32_t *channels, int64_t *rounds, int64_t *lens, size_t cap_packets,
                              int16_t *syms, size_t cap_syms);
/* The queued packets in the batched decoder's input layout, on the device. Straight after a run of the streaming mode -- nothing
 * read back to the host yet -- the rows are packed on the device from the kernel's records (no host round trip; rows ordered by
 * channel, then time). That includes packets begun in an earlier run: the symbols of a packet a channel is inside when a run ends
 * stay on the device and the next run's records continue them (packets of at most 4096 symbols; longer ones are handed on through
 * the host queue). Otherwise the rows come from the host queue in lorahip_demod_get_packets' order. Either way: packet p's
 * symbols at syms_dev + p*sym_stride (zero padded), its length in nsyms_dev[p] -- a packet longer than sym_stride keeps its true
 * length there and lorahip_decode_packets() reports -2 for it --, its channel in channel_dev[p] (nullable). *n_packets = number of
 * queued packets (also when cap_packets is too small: LORAHIP_E_INVALID then). Does not clear the queue.
 * On a handle of lorahip_demod_create_mixed whose parts all lie on one device: the parts' rows one after the other in the queue's
 * order (device slot ascending, SF ascending inside a slot), each part's rows in the order this entry gives for that part alone (a
 * part whose records are still the only copy is packed on the device, on its own stream; the others come from their host queues);
 * channel_dev holds GLOBAL channel numbers (each part's rows are renumbered on the device from its local-to-global table);
 * *n_packets = the total over the parts; the rows are complete when the call returns. Over several devices: LORAHIP_E_INVALID. */
int lorahip_demod_packets_to_device(lorahip_demod *d, uint16_t *syms_dev, size_t sym_stride, int32_t *nsyms_dev, int32_t *channel_dev,
                                    size_t cap_packets, size_t *n_packets);
/* The same with info_dev[p] = packet p's lorahip_rx_info (device memory, [cap_packets], nullable: then exactly the entry above, which
 * forwards here with NULL). Both sources fill it: the packing on the device from the kernel's records and the upload from the host queue. On a
 * mixed handle whose parts share a device the rows come in the same order; positions are per channel and are not remapped. */
int lorahip_demod_packets_to_device_info(lorahip_demod *d, uint16_t *syms_dev, size_t sym_stride, int32_t *nsyms_dev, int32_t *channel_dev,
                                         lorahip_rx_info *info_dev, size_t cap_packets, size_t *n_packets);
/* out[i] = lorahip_rx_info of queued packet i, in lorahip_demod_get_packets' order (streaming and host-driven modes give the same values);
 * pos[i] = position of queued signal i, in lorahip_demod_get_signals' order. cap below the queue's length: LORAHIP_E_INVALID. */
int lorahip_demod_get_packets_info(const lorahip_demod *d, lorahip_rx_info *out, size_t cap);
int lorahip_demod_get_signals_pos(const lorahip_demod *d, int64_t *pos, size_t cap);
void lorahip_demod_clear_packets(lorahip_demod *d);
/* samples of `channel`'s stream the last lorahip_demod_run[_device] consumed (the sum of its consume() calls, :320): a
 * streaming caller presents the unconsumed remainder again in front of the next chunk, as the framework's port buffer does */
int64_t lorahip_demod_consumed(const lorahip_demod *d, size_t channel);
/* the same for every channel at once: out[n_channels] */
int lorahip_demod_consumed_all(const lorahip_demod *d, int64_t *out);
/* total work() calls made (sum over channels) since lorahip_demod_create */
int64_t lorahip_demod_work_calls(const lorahip_demod *d);
/* device time of the streaming kernel launches of the last lorahip_demod_run[_device] (HIP events on the launch stream; 0 in the
 * host-driven mode): what the level-3 roofline line of bench.py is computed from */
double lorahip_demod_kernel_ms(const lorahip_demod *d);
/* streaming kernel launches the last lorahip_demod_run[_device] took (0 in the host-driven mode). One is the rule; a run whose
 * per-launch record buffers filled is resumed (records drained in between, which costs more than the launch), and the capacity the
 * following runs of this object are given grows with what the run needed -- a receiver settles at one launch per run */
int lorahip_demod_last_launches(const lorahip_demod *d);
/* The runtime signal for the caveat at the top of this section: how many decisions since the last activate() sat so close to their
 * boundary that the last-place differences between this library's power / powerAvg / fIndex and a CPU build's could have flipped
 * them. Counted, never altered.
 *   near_squelch : work() calls in FRAMESYNC / DATASYMBOLS (the states that consume `snr < thresh`, LoRaDemod.cpp:174,217,291)
 *                  with |snr - thresh| <= 4e-5 dB
 *   near_step    : windows dechirped with a moving fine-tune index whose step _finefreqError * 128 (LoRaDemod.cpp:160) lies
 *                  within 6e-5 of an integer, i.e. where a last-place difference in the fIndex values accumulated in
 *                  _finefreqError (:219) would move the reference's int <- float truncation
 * Both 0 means: every branch taken has a margin far above float rounding, so the identity with the CPU block holds by margin for
 * that run, not only by observation. Either pointer may be NULL. */
int lorahip_demod_near_threshold(const lorahip_demod *d, int64_t *near_squelch, int64_t *near_step);
/* Debug ports of the block, opt-in like the trace (they triple the HBM traffic): what LoRaDemod::work() writes to its "raw", "dec"
 * and "fft" outputs (LoRaDemod.cpp:81-83,163-164,172,320-324), per channel, for the NEXT runs. Device buffers owned by the caller:
 *   fft_dev  [n_channels][fft_cap_frames][N] cf32   one frame of N bins per work() call: window 0's FFT (:172, produce(N) :324)
 *   dec_dev  [n_channels][dec_cap_samples]   cf32   `total` dechirped samples per call (:164, produce(total) :322): window 0's first
 *                                                   min(total, N), and window 1 when the call consumed 2N (the sync check, :189-206)
 *   raw_dev  [n_channels][raw_cap_samples]   cf32   the samples consumed (:163, :321)
 * Any pointer may be NULL (that port stays off); p == NULL switches all off. Bins and samples are bit-identical to the reference's.
 * What exceeds a capacity is dropped; lorahip_demod_port_counts() reports what the last run produced. Labels: see below.
 * The ports are replayed from the per-call trace, so a run with ports on keeps one internally even when lorahip_demod_set_trace was
 * never enabled: that trace lives for the run only (it is not visible through lorahip_demod_get_trace / _trace_len / _get_labels
 * and does not accumulate), and like any traced run it drains the records to the host, i.e. the device-resident packet hand-off
 * of lorahip_demod_packets_to_device takes its host-queue path. */
typedef struct lorahip_demod_ports {
    size_t struct_size;     /* = sizeof(lorahip_demod_ports) */
    float *fft_dev; size_t fft_cap_frames;
    float *dec_dev; size_t dec_cap_samples;
    float *raw_dev; size_t raw_cap_samples;
    int32_t host_buffers;   /* 1: the three pointers are HOST buffers (a framework's port buffers): the library keeps device
                               buffers of the same shape and copies what a run produced into them before the run returns */
    int32_t reserved;
} lorahip_demod_ports;
int lorahip_demod_set_ports(lorahip_demod *d, const lorahip_demod_ports *p);
int lorahip_demod_port_counts(const lorahip_demod *d, size_t channel, size_t *fft_frames, size_t *dec_samples, size_t *raw_samples);
/* The stream labels work() posts at index 0 of what each call produces on raw / dec / fft (LoRaDemod.cpp:314-319) -- "SYNC",
 * "P <fIndex>", "DC", "QC", "S<n> <fIndex>", or none ("") -- for every call in `channel`'s trace (lorahip_demod_set_trace), as
 * NUL-terminated strings back to back, formatted like the reference's (fixed, 4 decimals). Label k sits at element k*N of the fft
 * port and at element sum(consumed[0..k)) of raw / dec. *n_calls = number of strings, *bytes = bytes needed; buf may be NULL. */
int lorahip_demod_get_labels(const lorahip_demod *d, size_t channel, char *buf, size_t cap, size_t *n_calls, size_t *bytes);
/* optional trace of every work() call: enable before run, then read back */
int lorahip_demod_set_trace(lorahip_demod *d, int enable);
size_t lorahip_demod_trace_len(const lorahip_demod *d, size_t channel);
int lorahip_demod_get_trace(const lorahip_demod *d, size_t channel, lorahip_work_result *out, size_t cap);

/* -------------------------------------------------------------------------------------
 * Synthetic IQ directly in HBM (bench / tests input; ChirpGenerator.hpp:22-47 semantics in
 * closed form): window w of channel c = ampl * upchirp(sym[c*S+w]) (+ AWGN of per-component
 * sigma `noise_sigma`, counter-based RNG keyed by seed). iq_dev: B*S*N cf32.
 * The symbol is MASKED to its low sf bits (sym & (N-1)); lorahip_mod_frames below does not mask. Without noise a
 * sample is (ampl * (float)cos(phi), ampl * (float)sin(phi)) with phi the chirp's phase from 0 in double, cos and
 * sin taken in double and rounded once (tests/modulator_def.py: synth_symbols_def restates it, expression for
 * expression; the kernel gives those values).
 * ------------------------------------------------------------------------------------- */
int lorahip_synth_symbols(lorahip_ctx *ctx, float *iq_dev, const uint16_t *sym_dev,
                          size_t n_windows, float ampl, float noise_sigma, uint64_t seed);

/* -------------------------------------------------------------------------------------
 * Batched modulator + channel (the step before the path: SURVEY.md section 8f #3). n_frames packets of nsyms
 * uint16 symbols each -> the samples the LoRaMod block produces for them (LoRaMod.cpp:109-238 on
 * ChirpGenerator.hpp:22-47, ovs = 1): 10 up-chirps, the two sync-word chirps, 2 1/4 down-chirps, one chirp
 * per symbol, max(padding,1) zero symbols; one running float phase accumulator per frame. Frame f is written
 * at iq_dev + f*frame_stride samples; frame_stride >= lorahip_mod_frame_len(sf, nsyms, padding).
 * A symbol is used AS GIVEN, as the block uses it: f0 = 2 pi sym / N also for sym >= N (lorahip_synth_symbols above
 * masks instead); mask on the caller's side if that is wanted.
 * Definition (tests/modulator_def.py): the block's float recurrence -- f += 2 pi / N with one wrap at +pi,
 * phase +-= f, phase reduced mod 2 pi in double at the end of every chirp -- with the sample
 * (ampl * (float)cos((double)phase), ampl * (float)sin((double)phase)), cos and sin rounded ONCE. The kernels give
 * these values. The block itself calls the platform's cosf / sinf, which miss the correctly rounded value by one ulp
 * in a percent or two of the samples: against the block's own output a sample is within 1 float ulp when |ampl| is
 * a power of two and within 2 when it is not (a last-place step of cos is up to two of ampl * cos).
 * Refused with LORAHIP_E_INVALID, nothing written: nsyms 0 or > 0x7fffff, padding > 0x7fffff, a frame_stride shorter
 * than the frame, a null pointer with n_frames > 0. n_frames 0 is no work. lorahip_mod_frame_len is 0 outside SF 6..12.
 * ------------------------------------------------------------------------------------- */
size_t lorahip_mod_frame_len(int sf, size_t nsyms, size_t padding);
int lorahip_mod_frames(lorahip_ctx *ctx, float *iq_dev, size_t frame_stride, const uint16_t *syms_dev,
                       size_t n_frames, size_t nsyms, unsigned char sync, float ampl, size_t padding);
/* complex AWGN of per-component standard deviation sigma added in place (counter-based generator keyed by seed) */
int lorahip_add_awgn(lorahip_ctx *ctx, float *iq_dev, size_t n_samples, float sigma, uint64_t seed);

/* -------------------------------------------------------------------------------------
 * Batched decoder (the step after the path: SURVEY.md section 8f #2): what the LoRaDecoder block does with one symbol
 * message (LoRaDecoder.cpp:196-397 on LoRaCodes.hpp), for n_packets messages at once. Parameters and defaults are the
 * block's (LoRaDecoder.cpp:98-110, setters :134-191): coding rate "4/4".."4/8" = rdd 0..4.
 *   packet p: nsyms_dev[p] symbols at syms_dev + p*sym_stride (sym_stride <= lorahip_decode_max_symbols() = 16384)
 *   out_len_dev[p]: number of output elements posted at out_dev + p*out_stride -- bytes, or uint16 symbols when
 *       interleaving is off --, -1 if the block posts nothing (fewer than 8 symbols, or dropped), -2 if the row does not hold the
 *       symbols the packet's length needs (nsyms_dev[p] > sym_stride: the caller's rows are too short -- an error, see
 *       lorahip_decode_max_symbols); dropped_dev[p] = 1 where the block calls drop() (the "dropped" signal).
 *   out_stride: even, >= 2*(sym_stride + 8). ctx supplies the device and the stream only (any SF).
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_decoder_cfg {
    size_t struct_size;     /* = sizeof(lorahip_decoder_cfg) */
    int32_t sf;             /* setSpreadFactor      default 10 */
    int32_t ppm;            /* setSymbolSize        default 0 = sf */
    int32_t rdd;            /* setCodingRate        default 4 ("4/8"); LORAHIP_RDD_FROM_HEADER (-1): each packet's header names it (below) */
    int32_t crcc;           /* enableCrcc           default 0 */
    int32_t interleaving;   /* enableInterleaving   default 1 */
    int32_t error_check;    /* enableErrorCheck     default 0 */
    int32_t explicit_hdr;   /* enableExplicit       default 1 */
    int32_t hdr;            /* enableHdr            default 0 */
    int32_t data_length;    /* setDataLength        default 8 */
} lorahip_decoder_cfg;
int lorahip_decode_packets(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfg, const uint16_t *syms_dev, size_t sym_stride,
                           const int32_t *nsyms_dev, size_t n_packets, uint8_t *out_dev, size_t out_stride,
                           int32_t *out_len_dev, int32_t *dropped_dev);
/* The same with every buffer in HOST memory (staged through the context's pinned buffer; synchronous): what a host-side block calls
 * -- lora_sdr_amd/pothos/LoRaDecoderBatch.cpp collects the messages waiting on its inputs into rows and posts the bytes. The bytes of
 * an output row behind out_len (the whole row where out_len < 0) are unspecified: the rows are copied out, never in. */
int lorahip_decode_packets_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfg, const uint16_t *syms, size_t sym_stride,
                                const int32_t *nsyms, size_t n_packets, uint8_t *out, size_t out_stride, int32_t *out_len,
                                int32_t *dropped);
/* The same launch with the configuration PER PACKET (a receiver over several SFs and coding rates: lorahip_demod_create_mixed ->
 * lorahip_demod_packets_to_device -> here): packet p is decoded under cfgs[i] exactly as lorahip_decode_packets decodes it under that
 * configuration -- the same bytes, out_len and dropped, and the same bytes left untouched behind them.
 *   i = index_dev[p] with table_dev == NULL, else i = table_dev[index_dev[p]] (index_dev = the hand-off's channel_dev, table_dev[n_table]
 *       = configuration of channel). out_len_dev[p] = -3, dropped_dev[p] = 0 and nothing written to the packet's output row where
 *       index_dev[p] lies outside [0, n_table) or i outside [0, n_cfgs). -1 and -2 keep their meaning; the row rule behind -2 is each
 *       packet's own configuration's.
 *   cfgs: n_cfgs = 1..64 entries in HOST memory, read before the call returns (they travel in the kernel's arguments: nothing is
 *       allocated or uploaded). LORAHIP_E_INVALID with nothing launched: n_cfgs 0 or > 64, ANY entry that lorahip_decode_packets would
 *       refuse (whether or not a packet uses it), index_dev NULL with n_packets > 0, table_dev set with n_table 0 (or n_table >
 *       0x7fffffff), and the row and stride limits above. n_packets 0 is no work.
 *   One launch has one lane count per packet and one LDS slice per packet, those of the entry that needs most (lorahip_decode_plan below):
 *       a table that holds an implicit-header entry with a data_length of thousands of bytes runs few packets per workgroup for ALL its
 *       packets. Accepted: give such packets a launch of their own where that matters. */
int lorahip_decode_packets_cfgs(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, size_t n_table, const uint16_t *syms_dev, size_t sym_stride,
                                const int32_t *nsyms_dev, size_t n_packets, uint8_t *out_dev, size_t out_stride, int32_t *out_len_dev,
                                int32_t *dropped_dev);
/* ... with every buffer (index and table too) in HOST memory, as lorahip_decode_packets_host; synchronous */
int lorahip_decode_packets_cfgs_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, size_t n_table, const uint16_t *syms, size_t sym_stride, const int32_t *nsyms,
                                     size_t n_packets, uint8_t *out, size_t out_stride, int32_t *out_len, int32_t *dropped);
/* The CODING RATE FROM THE HEADER: rdd = LORAHIP_RDD_FROM_HEADER in a lorahip_decoder_cfg (one entry per SF is then enough for a gateway).
 * The reference de-interleaves and de-whitens a message at the rate of its SETTER and reads the header's rate field only for the Hamming
 * step (LoRaDecoder.cpp:228-255, :296): a packet sent at another rate comes out as garbage. Under an entry with rdd = -1, packet p gives
 * exactly what lorahip_decode_packets gives it under the same entry with rdd = r -- every byte of the output row, out_len (-1 and -2
 * included, by the row rule and the plan of rate r), dropped, and the bytes left untouched behind out_len -- where
 *       r = ((decodeHamming84sx(cw2) & 0xf) >> 1) & 7,
 * cw2 = codeword 2 of the first interleaver block: de-interleaved at 4/8 from the first 8 Gray-coded symbols, not whitened -- the same
 * bits at every configured rate, which is why the header block is sent that way. r > 4: out_len = -1, dropped = 1, nothing written (what
 * every setting gives such a header, :293 / :297). Fewer than 8 symbols, PPM > sf: as before. Accepted only with explicit_hdr = 1 and
 * interleaving = 1; anything else with rdd = -1, and rdd < -1, is LORAHIP_E_INVALID in every entry point below and above, nothing
 * launched. A table may hold such entries beside any others. lorahip_decode_plan: sym_cap, cw_cap and lds_slice_bytes of a header-rate
 * entry are each the largest of the same entry's at rdd = 0..4.
 * (The lane-per-packet checker -- lorahip_set_variant 1 -- keeps its own, stricter row rule: -2 for every packet longer than its row or
 * than 520 symbols, at every rate, so also for a rate field of 5..7. One corner stays the definition's and not "the uniform launch's": a
 * packet of 517..519 symbols with a field of 5..7 is -1 / dropped, where the checker's uniform launch rounds it past 520 symbols -- -2 --
 * at 4/6 (519 symbols: and at 4/7) only.) */
#define LORAHIP_RDD_FROM_HEADER (-1)
/* The HEADER REPORT of a packet: what the decoder learns from the header and the checksum and the outputs above do not show (a packet
 * forwarder's codr / size / stat). It never changes out, out_len or dropped. Written by lorahip_decode_packets_info for EVERY packet:
 *   "header not reached" -- out_len = -3, fewer than 8 symbols, PPM > sf, interleaving off, and (checker kernel only) its own -2 --:
 *       length = rdd = hdr_residue = need_syms = -1, crc = fec_error = 0.
 *   explicit header: length, rdd and hdr_residue are the decoded header's as soon as it is read (:283-291), also where the packet is then
 *       dropped by the error check (:293), for a rate field > 4 (:297) or for a row shorter than the length (:313).
 *   need_syms is set once the decode has passed :313 (the message holds the announced bytes by count) -- so for every out_len >= 0, for
 *       -2, and for packets dropped later --, else -1.
 *   crc is set where the reference computes the checksum (:367-388): with a header whenever the header's crc flag is set (crcc only
 *       decides whether a mismatch drops), without a header only with crcc = 1; a decode that ended before leaves 0.
 *   fec_error is the reference's `error` flag at the statement where this packet's decode ended: header codewords only for a packet
 *       that ended in the header stage, header + first block + the codewords of the announced bytes otherwise. */
typedef struct lorahip_packet_info {   /* 32 bytes */
    int32_t length;       /* announced payload bytes: header byte 0 (explicit), data_length (implicit); -1: the header was not reached */
    int32_t rdd;          /* the header's rate field 0..7, also where it is > 4 and the packet is dropped; the entry's rdd without a header; -1 not reached */
    int32_t crc;          /* 1 checksum carried and equal, -1 carried and different, 0 none evaluated (none carried / not enabled / decode ended before) */
    int32_t hdr_residue;  /* header byte 2 after LoRaDecoder.cpp:291 (0 = the header's checksum agrees), -1 without an explicit header or not reached */
    int32_t fec_error;    /* the reference's `error` flag where the decode of this packet ended (0 / 1) */
    int32_t need_syms;    /* symbols the announced length needs (whole interleaver blocks, the kernel's needSyms); also set when out_len = -2; -1 not known */
    int32_t reserved[2];  /* 0 */
} lorahip_packet_info;
/* lorahip_decode_packets_cfgs with the report: info_dev[n_packets], or NULL for none (then exactly lorahip_decode_packets_cfgs).
 * index_dev may be NULL only with n_cfgs == 1 and table_dev == NULL: every packet runs under entry 0 -- the uniform launch of
 * lorahip_decode_packets; with more entries a NULL index_dev is LORAHIP_E_INVALID. Everything else as lorahip_decode_packets_cfgs. The
 * other decoder entry points forward to this one. */
int lorahip_decode_packets_info(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, size_t n_table, const uint16_t *syms_dev, size_t sym_stride,
                                const int32_t *nsyms_dev, size_t n_packets, uint8_t *out_dev, size_t out_stride, int32_t *out_len_dev,
                                int32_t *dropped_dev, lorahip_packet_info *info_dev);
/* ... with every buffer in HOST memory, as lorahip_decode_packets_cfgs_host; synchronous */
int lorahip_decode_packets_info_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, size_t n_table, const uint16_t *syms, size_t sym_stride, const int32_t *nsyms,
                                     size_t n_packets, uint8_t *out, size_t out_stride, int32_t *out_len, int32_t *dropped,
                                     lorahip_packet_info *info);
/* What a launch over rows of sym_stride symbols under these configurations runs on (host only, no device touched; the launches call the
 * same function): a packet's symbols, codewords and nibbles live in an LDS slice of its lane group, sized by what the configuration can
 * need -- (sym_cap * 2 + 2 * cw_cap + 15) & ~15 bytes; lanes_per_packet is 8 / 16 / 32 / 64 for the largest sym_cap <= 48 / <= 96 / <= 200 /
 * above; packets_per_workgroup = min(256 / lanes_per_packet, 160 KiB / lds_slice_bytes). sym_cap, cw_cap and the slice are the largest
 * over the entries. With n_cfgs == 1: what lorahip_decode_packets launches. Refused like lorahip_decode_packets_cfgs (*plan zeroed). */
typedef struct lorahip_decode_tiling {
    size_t struct_size;     /* = sizeof(lorahip_decode_tiling), set by the caller */
    int32_t lanes_per_packet, sym_cap, cw_cap, lds_slice_bytes, packets_per_workgroup, reserved;
} lorahip_decode_tiling;
int lorahip_decode_plan(const lorahip_decoder_cfg *cfgs, size_t n_cfgs, size_t sym_stride, lorahip_decode_tiling *plan);   /* host only */
/* the longest row (symbols): sym_stride <= this (16384). A packet of ANY length up to its row decodes as the reference decodes it: the
 * reference de-interleaves every codeword of a message but only those the announced length needs reach the output (LoRaDecoder.cpp:
 * 315-361) -- at most 2 * 260 with an explicit header --, so the kernel's working set follows the configuration, not the packet. A packet
 * LONGER than its row (nsyms_dev[p] > sym_stride) still decodes when the symbols its length needs lie inside the row; otherwise
 * out_len = -2: the caller's rows are too short, which a caller must treat as an error (LoRaDecoderBatch.cpp throws). */
int lorahip_decode_max_symbols(void);
/* without a header: the largest data_length (4096 bytes); a larger one is refused with LORAHIP_E_INVALID */
int lorahip_decode_max_data_length(void);

/* -------------------------------------------------------------------------------------
 * Soft-decision receive: a second pass over packets the demodulator has already found. lorahip_soft_symbols turns the symbol windows of
 * each packet into one log-likelihood ratio per bit the decoder reads; lorahip_decode_packets_soft decodes rows of such values with a
 * maximum-likelihood FEC step. No other entry point, kernel or result depends on either.
 *
 * SOFT SYMBOLS. n_packets RUNS of consecutive windows at the SF of the context. Window s of run p is the window lorahip_detect_batch
 * evaluates with offsets = first_sample[p] + s*N, chirp_sel_all = LORAHIP_CHIRP_UP, fine_err = fine_err[p] and, as fine_idx0, the
 * fine_idx_out of window s - 1 (fine_idx0[p] for s = 0); its bins X[k] are that call's fft_out bit for bit (default build of the
 * kernels), sym_dev[p][s] is that call's sym. With
 *       P[k] = re*re + im*im                                                         (float, no contraction)
 *       g(k) = binaryToGray16(uint16((k + ((1 << (sf-ppm)) / 2)) >> (sf-ppm))) & ((1 << ppm) - 1)      (LoRaDecoder.cpp:218-222)
 *       llr[p][s][m] = max{P[k] : bit m of g(k) = 1} - max{P[k] : bit m of g(k) = 0},   m = 0..ppm-1
 * -- the max-log metric on |X|^2, positive = bit 1; one float subtraction of two exact maxima, so independent of any reduction order.
 * NON-FINITE BINS. Each of the two maxima starts at 0 and a bin enters it only through P[k] > max. A NaN P[k] (a NaN bin, or an
 * infinite one beside a NaN) therefore never enters; a side no bin was admitted to is +0.0, and a window with no admitted bin on either
 * side (all bins zero, all P[k] underflowed to zero, or all NaN) has the LLR +0.0. P[k] = +Inf does enter, so an LLR can be +Inf, -Inf or
 * NaN (Inf - Inf; the NaN's bit pattern is unspecified). sym is found the same way, as lorahip_detect_batch finds it: the first k in
 * ascending order whose P[k] exceeds every earlier one, from 0 -- and 0 when no bin is admitted.
 * Row p of llr_dev is sym_stride * ppm floats, window s at s * ppm; windows s >= min(nsyms[p], sym_stride) are not evaluated and their
 * entries (and sym_dev's) are left as they were; nsyms[p] < 1: nothing is read or written for the run. ppm = 0 means sf.
 * fine_idx0 / fine_err of a packet are the demodulator's _fineTuneIndex / _finefreqError when its first DATASYMBOLS call begins (both
 * constant from there to the post, LoRaDemod.cpp:299, :308): in a trace (lorahip_demod_set_trace) the fine_idx_before / fine_err_before
 * of the call that starts at lorahip_rx_info::data_pos. A fine_idx0 outside [0, 128*N) is masked into the table: an unspecified row,
 * never a fault. LORAHIP_E_INVALID, nothing launched: a null required pointer with n_packets > 0, ppm outside 0..sf, sym_stride 0 or
 * above lorahip_decode_max_symbols(), n_packets > 0x7fffffff. n_packets = 0 is no work. Asynchronous on the context's stream. */
int lorahip_soft_symbols(lorahip_ctx *ctx, const float *iq_dev,
                         const int64_t *first_sample_dev,   /* [n_packets] sample index in iq_dev of the run's first window */
                         const int32_t *nsyms_dev,          /* [n_packets] windows in the run */
                         const int32_t *fine_idx0_dev,      /* [n_packets] nullable -> 0 */
                         const float *fine_err_dev,         /* [n_packets] nullable -> 0 */
                         size_t n_packets, int ppm, float *llr_dev, size_t sym_stride,
                         uint16_t *sym_dev /* nullable, [n_packets][sym_stride] */);
/* What lorahip_soft_symbols launches for n_packets runs (host only, no device work; the launch takes its grid and block from the same
 * function). SF6-SF10: a run per lane group of a wavefront, runs_per_wavefront = 64 / lanes per window (16, 8, 4, 2, 1); four wavefronts
 * per workgroup once ceil(n_packets / (4 * runs_per_wavefront)) reaches twice the device's compute units, one below that; workgroups =
 * ceil(n_packets / (runs_per_wavefront * waves_per_workgroup)). SF11 / SF12: a run per workgroup, runs_per_wavefront = 0,
 * waves_per_workgroup = 2 / 4, workgroups = n_packets. LORAHIP_E_INVALID (*plan zeroed): a null context, n_packets > 0x7fffffff; a null
 * plan or a struct_size that is not this struct's. */
typedef struct lorahip_soft_tiling {
    size_t struct_size;     /* = sizeof(lorahip_soft_tiling), set by the caller */
    int32_t runs_per_wavefront, waves_per_workgroup, workgroups, reserved;
} lorahip_soft_tiling;
int lorahip_soft_plan(lorahip_ctx *ctx, size_t n_packets, lorahip_soft_tiling *plan);   /* no device work */
/* THE SOFT DECODER: lorahip_decode_packets_info with rows of LLRs in place of rows of symbols. Packet p under entry e reads symbol s, bit m,
 * at llr_dev[p * llr_stride + s * PPM_e + m] (PPM_e = the entry's ppm, or its sf), s < min(nsyms[p], sym_stride); every other symbol of
 * its blocks is all-zero LLRs, as the hard decoder's are zero symbols. sym_stride * PPM_e <= llr_stride <= 8 * 12 * sym_stride for every
 * entry (LORAHIP_E_INVALID otherwise). The hard bit of
 * an LLR is 1 iff llr > 0.
 *   - De-interleave and whitening move LLRs: bit k of codeword i of a block is the LLR at (symbol symOff + k, bit m), i = (m + k) % PPM; a
 *     whitening bit of 1 negates it; bits a block does not carry (k >= 4 + its rate) are 0. Header block and whitening offsets as
 *     LoRaDecoder.cpp:225-255.
 *   - Where the reference calls decodeHamming84sx / 74sx / checkParity64 / 54 or passes a 4/4 nibble through, the nibble is the x in 0..15
 *     that maximises M(x) = sum over k = 0..n-1 ascending of (bit k of enc(x) ? +L[k] : -L[k]), accumulated in float from 0.0f in that
 *     order; the smallest x wins ties; enc = the encoder's codeword at the rate that call decodes (n = 4 + rdd; the first block: n = 8).
 *     Stated as the loop it is, which also settles LLRs that are not finite: x = 0 is the incumbent, and x = 1..15 in ascending order
 *     replaces it only by M(x) > M(incumbent). A NaN M(x) (a NaN LLR, or +Inf and -Inf contributions meeting) therefore never wins, and a
 *     NaN M(0) is never replaced: the nibble is 0. The hard bit is llr > 0, so a NaN LLR reads as 0 (and, negated by a whitening bit
 *     of 1, is still NaN).
 *   - The reference's `error` flag (error_check, fec_error) is still the hard decoders' over the hard bits: the hard codeword is the hard
 *     bits of the LLRs as read, de-interleaved, XOR the whitening bits -- so drops and the report mean what they mean in the hard decoder.
 *   - Header checksum and length, the CRC and its drop, hdr, the outcomes -1 / -2 / -3 (the row rule on the caps of lorahip_decode_plan),
 *     need_syms and LORAHIP_RDD_FROM_HEADER (the rate field of the soft-decoded codeword 2) are the hard decoder's.
 * On LLRs of +1 / -1 made from an encoder's row of symbols the result is lorahip_decode_packets_info's on that row (every codeword it
 * decodes is a codeword, and a codeword beats every other candidate). interleaving = 0 in any entry is LORAHIP_E_INVALID (its output is symbols); lorahip_set_variant does not apply. The LLRs
 * are read from device memory per codeword: a packet's LDS slice is 16 + cw_cap bytes at the lane count of lorahip_decode_plan, so every
 * configuration the hard decoder accepts fits, data_length up to lorahip_decode_max_data_length() included. */
int lorahip_decode_packets_soft(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, size_t n_table, const float *llr_dev, size_t llr_stride, size_t sym_stride,
                                const int32_t *nsyms_dev, size_t n_packets, uint8_t *out_dev, size_t out_stride, int32_t *out_len_dev,
                                int32_t *dropped_dev, lorahip_packet_info *info_dev);
/* ... with every buffer in HOST memory, as lorahip_decode_packets_info_host; synchronous */
int lorahip_decode_packets_soft_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, size_t n_table, const float *llr, size_t llr_stride, size_t sym_stride,
                                     const int32_t *nsyms, size_t n_packets, uint8_t *out, size_t out_stride, int32_t *out_len,
                                     int32_t *dropped, lorahip_packet_info *info);

/* -------------------------------------------------------------------------------------
 * Batched encoder (the first block of the chain): what the LoRaEncoder block does with one message of bytes
 * (LoRaEncoder.cpp:161-233 on LoRaCodes.hpp), for n_packets messages of different lengths at once. Parameters and defaults are
 * the block's (LoRaEncoder.cpp:78-85, setters :101-133): coding rate "4/4".."4/8" = rdd 0..4.
 *   packet p: nbytes_dev[p] payload bytes at bytes_dev + p*byte_stride (byte_stride <= lorahip_encode_max_bytes() = 4096)
 *   nsyms_dev[p]: the number of symbols written at syms_dev + p*sym_stride (sym_stride <= lorahip_decode_max_symbols()), or
 *       -1 where the reference has no defined result: an empty payload without crc and without header (its symbol count
 *          `8 + (numCodewords / PPM - 1) * (4 + rdd)` wraps for numCodewords == 0), or a negative nbytes_dev[p];
 *       -2 where a row is too short: nbytes_dev[p] > byte_stride, or the packet's symbols > sym_stride.
 *   The symbols of a row behind the packet's own are written as 0 up to sym_stride (the whole row for -1 / -2), nothing behind the row.
 *   PAD NIBBLES ARE ZERO. Where 2 * bytes + header codewords is not a multiple of PPM the reference's encodeFec reads up to
 *   (PPM - 1) / 2 bytes past the end of its byte vector (LoRaEncoder.cpp:202,206), i.e. whatever the heap holds. This encoder
 *   defines the pad nibbles as 0, then FEC-encoded and whitened like any data nibble: the symbols equal the reference's wherever
 *   the reference is defined, and equal the reference's for the payload extended by zero bytes where it is not. The decoder never
 *   reads pad codewords. A payload of more than 255 bytes with an explicit header is encoded as the reference does it: all the
 *   bytes, length field & 0xff.
 *   LORAHIP_E_INVALID: struct_size mismatch, sf outside 1..12, ppm > sf (the reference throws), rdd outside 0..4, explicit header
 *   with PPM < 5 (the reference's `PPM - cOfs` wraps), byte_stride or sym_stride beyond the limits above. ctx supplies the device
 *   and the stream only (any SF).
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_encoder_cfg {
    size_t struct_size;     /* = sizeof(lorahip_encoder_cfg) */
    int32_t sf;             /* setSpreadFactor      default 10 */
    int32_t ppm;            /* setSymbolSize        default 0 = sf */
    int32_t rdd;            /* setCodingRate        default 4 ("4/8") */
    int32_t explicit_hdr;   /* enableExplicit       default 1 */
    int32_t crc;            /* enableCrc            default 1 */
    int32_t whitening;      /* enableWhitening      default 1 */
} lorahip_encoder_cfg;
/* host only: the symbols of a packet of n_bytes payload bytes; -1 for the undefined case above, for a configuration that
 * lorahip_encode_packets refuses and for n_bytes > lorahip_encode_max_bytes(). Never decreases with n_bytes. */
long lorahip_encode_num_symbols(const lorahip_encoder_cfg *cfg, size_t n_bytes);
/* the longest payload (4096 bytes, = lorahip_decode_max_data_length()): byte_stride <= this */
int lorahip_encode_max_bytes(void);
int lorahip_encode_packets(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfg, const uint8_t *bytes_dev, size_t byte_stride,
                           const int32_t *nbytes_dev, size_t n_packets, uint16_t *syms_dev, size_t sym_stride, int32_t *nsyms_dev);
/* The same with every buffer in HOST memory (staged through the context's pinned buffer; synchronous). */
int lorahip_encode_packets_host(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfg, const uint8_t *bytes, size_t byte_stride,
                                const int32_t *nbytes, size_t n_packets, uint16_t *syms, size_t sym_stride, int32_t *nsyms);

/* -------------------------------------------------------------------------------------
 * The batched modulator for frames of DIFFERENT lengths (the encoder's rows): frame f has nsyms_dev[f] symbols at
 * syms_dev + f*sym_stride (max_nsyms <= sym_stride) and is walked like a frame of lorahip_mod_frames, then continued with zero
 * chirps to the common length lorahip_mod_frame_len(sf, max_nsyms, padding) <= frame_stride: row f equals the frame
 * lorahip_mod_frames (and the LoRaMod block) produces for the same symbols with padding + max_nsyms - nsyms_dev[f]
 * (padding 0 counts as 1, as there). A frame with nsyms_dev[f] < 0 -- a packet the encoder refused -- or > max_nsyms is written as
 * all zeros. No host round trip between lorahip_encode_packets and this call: max_nsyms = lorahip_encode_num_symbols(cfg, byte_stride)
 * bounds every packet of the launch.
 * ------------------------------------------------------------------------------------- */
int lorahip_mod_frames_var(lorahip_ctx *ctx, float *iq_dev, size_t frame_stride, const uint16_t *syms_dev, size_t sym_stride,
                           const int32_t *nsyms_dev, size_t n_frames, size_t max_nsyms, unsigned char sync, float ampl, size_t padding);

/* -------------------------------------------------------------------------------------
 * The transmit side of a receiver over several SFs and coding rates (the mirror of lorahip_decode_packets_cfgs): the encoder with the
 * configuration PER PACKET, and the modulator with SF, channel row and start sample PER FRAME.
 *
 * lorahip_encode_packets_cfgs: packet p is encoded under cfgs[i] exactly as lorahip_encode_packets encodes it under that configuration --
 * the same symbols, the same nsyms (-1 and -2 included), the same zeros behind the packet up to sym_stride.
 *   i = index_dev[p] with table_dev == NULL, else i = table_dev[index_dev[p]]. nsyms_dev[p] = -3 and an all-zero row where index_dev[p]
 *       lies outside [0, n_table) or i outside [0, n_cfgs).
 *   cfgs: n_cfgs = 1..64 entries in HOST memory, read before the call returns (they travel in the kernel's arguments: nothing is
 *       allocated or uploaded). LORAHIP_E_INVALID with nothing launched: n_cfgs 0 or > 64, ANY entry that lorahip_encode_packets would
 *       refuse (whether or not a packet uses it), index_dev NULL with n_packets > 0, table_dev set with n_table 0 (or n_table >
 *       0x7fffffff), and the stride limits of lorahip_encode_packets. n_packets 0 is no work.
 *   One launch has one lane count per packet and one LDS slice per packet, those of the entry that needs most over the rows of the launch;
 *       each packet's group lays its slice out by its own entry.
 * ------------------------------------------------------------------------------------- */
int lorahip_encode_packets_cfgs(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfgs, size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, size_t n_table, const uint8_t *bytes_dev, size_t byte_stride,
                                const int32_t *nbytes_dev, size_t n_packets, uint16_t *syms_dev, size_t sym_stride, int32_t *nsyms_dev);
/* ... with every buffer (index and table too) in HOST memory, as lorahip_encode_packets_host; synchronous */
int lorahip_encode_packets_cfgs_host(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfgs, size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, size_t n_table, const uint8_t *bytes, size_t byte_stride, const int32_t *nbytes,
                                     size_t n_packets, uint16_t *syms, size_t sym_stride, int32_t *nsyms);
/* lorahip_mod_frames_sched: frame f is the BODY of the frame lorahip_mod_frames produces at SF sf_dev[f] for the first nsyms_dev[f] symbols
 * at syms_dev + f*sym_stride -- everything before the zero padding: 10 up-chirps, 2 sync chirps, 2 1/4 down-chirps, the data chirps;
 * lorahip_mod_body_len(sf, nsyms) = 14.25 N + nsyms N samples (0 outside SF 6..12) --, one float phase accumulator from 0
 * (tests/modulator_def.py), amplitude ampl_dev[f] (ampl where ampl_dev is NULL), symbols as given (a symbol >= N is not masked). It is
 * stored at samples [start_dev[f], start_dev[f] + body_len) of row row_dev[f] of iq_dev (n_rows rows of row_len complex64 samples, row_stride
 * samples apart). NOTHING ELSE IS WRITTEN: the silence between the frames is the caller's. Every written sample is bit-identical to the one
 * lorahip_mod_frames writes for the same symbols, SF, sync and amplitude. ctx supplies the device and the stream only (any SF).
 *   status_dev[f] (may be NULL), checked in this order; a frame with a status != 0 writes nothing:
 *        0  written
 *       -1  nsyms_dev[f] < 1 or > sym_stride (the encoder's -1, -2 and -3 end here)
 *       -3  sf_dev[f] outside 6..12, or row_dev[f] outside [0, n_rows)
 *       -2  the body does not lie inside [0, row_len)
 *   Frames of one launch MUST NOT OVERLAP: in an overlap every sample holds the value of one of the frames (not their sum), which one is
 *       not defined. Not detected.
 *   lanes: the lanes of a wavefront that share a frame -- 4, 16, 64, or 0 = chosen by n_frames; the samples do not
 *       depend on it. With 4 / 16 the frames of a wavefront are neighbours in the order given and it runs as long as its longest frame.
 *   LORAHIP_E_INVALID, nothing launched: a null pointer (status_dev and ampl_dev excepted) with n_frames > 0, row_len > row_stride,
 *       sym_stride 0 or > lorahip_decode_max_symbols(), lanes not one of 0, 4, 16, 64, n_rows or n_frames > 0x7fffffff. */
size_t lorahip_mod_body_len(int sf, size_t nsyms);
int lorahip_mod_frames_sched(lorahip_ctx *ctx, float *iq_dev, size_t n_rows, size_t row_stride, size_t row_len,
                             const uint16_t *syms_dev, size_t sym_stride, const int32_t *nsyms_dev, const int32_t *sf_dev,
                             const int32_t *row_dev, const int64_t *start_dev, const float *ampl_dev, size_t n_frames,
                             unsigned char sync, float ampl, int lanes, int32_t *status_dev);

/* -------------------------------------------------------------------------------------
 * Front-end channeliser (the step before the path: SURVEY.md section 8f #4). NOT a reference component: the
 * reference's topologies put Pothos' /comms/rotate and a decimating FIR in front of every LoRaDemod block; this
 * does that for K channels of one wideband stream at once and writes the [channel][time] layout
 * lorahip_demod_run_device() reads. Definition (x[n] = the wideband stream since the last reset, x[n<0] = 0,
 * w_k = lorahip_channelizer_phase_inc(freq[k]), D = decim, L = n_taps, h = taps):
 *
 *     n_m    = (m + 1) D - 1                                  (every D new samples make one output)
 *     y_k[m] = sum_{j<L} h[j] x[n_m - j] exp(-2 pi i frac(w_k (n_m - j) / 2^64))
 *
 * i.e. mix channel k's centre frequency (freq[k] cycles per input sample) down to 0, low-pass with h, keep every
 * D-th sample. Evaluated in fp32 (fused multiply-add) on taps pre-rotated in double; the phase is a 64-bit
 * counter, so there is no drift and a stream cut into arbitrary chunks gives bit-identical outputs to one call.
 * run(): consumes n_in samples, writes *n_out = lorahip_channelizer_out_count(c, n_in) samples per channel at
 * out_dev + k*out_stride (complex64, out_stride in samples >= *n_out). decim*(256 + n_taps/decim) samples must
 * fit the LDS (decim <= 64 for short filters).
 * Limits of one call (run and run_captures alike; a longer stream is fed in several calls): at most 2^30 outputs per channel
 * (8 GiB a row), and channel groups x tiles = ceil(n_channels / 8) * (outputs / 256 + 1) at most 2^31 - 1 (the launch grid). A call beyond either is refused with
 * LORAHIP_E_INVALID and consumes nothing. Rows, strides and the stream position are addressed with 64 bits.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_channelizer lorahip_channelizer;
uint64_t lorahip_channelizer_phase_inc(double freq);          /* floor(frac(freq) * 2^64) */
int lorahip_channelizer_create(lorahip_channelizer **out, lorahip_ctx *ctx, size_t n_channels, const double *freq,
                               size_t decim, const float *taps, size_t n_taps);
void lorahip_channelizer_destroy(lorahip_channelizer *c);
int lorahip_channelizer_reset(lorahip_channelizer *c);
size_t lorahip_channelizer_out_count(const lorahip_channelizer *c, size_t n_in);
int lorahip_channelizer_run(lorahip_channelizer *c, const float *wide_dev, size_t n_in, float *out_dev,
                            size_t out_stride, size_t *n_out);
/* A batch of independent captures in one launch (recordings, antennas): capture s is the n_in samples at wide_dev + s*capture_stride,
 * processed like a fresh stream (from sample 0, zero history; bit-identical to reset() + run() on it); its channel k goes to
 * out_dev + (s*n_channels + k)*out_stride, *n_out = n_in / decim samples each. The object's own stream state is not touched.
 * n_captures <= 65535. */
int lorahip_channelizer_run_captures(lorahip_channelizer *c, const float *wide_dev, size_t n_captures, size_t capture_stride,
                                     size_t n_in, float *out_dev, size_t out_stride, size_t *n_out);

/* -------------------------------------------------------------------------------------
 * Front-end synthesiser: the channeliser's mirror image on the transmit side. K channel-rate streams (the rows
 * lorahip_mod_frames / lorahip_mod_frames_var write and the demodulator reads) go onto their carriers in ONE wideband stream:
 * what a gateway's single DAC sends and what a channeliser on the other side takes apart. NOT a reference component.
 * Definition (x_k[m] = channel k's stream since the last reset, x_k[m<0] = 0, U = interp, L = n_taps, h = taps,
 * w_k = lorahip_channelizer_phase_inc(freq[k]) with freq[k] in cycles per OUTPUT sample -- the same array serves a
 * channeliser of decim = interp on the other side --, gain[k] real, gain == NULL: all 1):
 *
 *     y[n] = sum_k gain[k] exp(+2 pi i frac(w_k n / 2^64)) sum_{j<L, (n-j) mod U == 0, n-j >= 0} h[j] x_k[(n-j)/U]
 *
 * i.e. zero-stuff by U, low-pass with h, mix up to the channel's centre, scale, sum the channels. Pass
 * U * design_lowpass(U, L, ...) for unit passband gain. Output phases without a tap (L < U) are exact zeros.
 * Non-finite samples: the taps are padded with zeros to ceil(L/U) whole rounds of U and the products with the padding ARE formed
 * (0 * NaN = NaN), so a NaN or Inf in x_k[m] makes the U * ceil(L/U) outputs m U .. (m + ceil(L/U)) U - 1 non-finite (phases
 * without a tap stay zero): the L outputs of the definition when L is a multiple of U, up to U - 1 more behind them otherwise.
 * Every other output is untouched.
 * n_in samples per channel always give exactly n_in * interp outputs. Evaluated in fp32 (fused multiply-add) on taps that
 * are scaled and pre-rotated in double; every input sample is rotated once by exp(+i theta_k U m), the phase taken from a
 * 64-bit counter, and the channels are summed in ascending order: no drift, and a stream cut into arbitrary chunks gives
 * bit-identical outputs to one call.
 * run(): row k of the input is the n_in complex64 samples at in_dev + 2*k*in_stride floats (in_stride in samples >= n_in);
 * writes *n_out = lorahip_synthesizer_out_count(s, n_in) = n_in * interp samples at wide_dev. Asynchronous on the context's
 * stream. Between calls the object keeps the stream position and the ceil(L/U) - 1 trailing input samples of every channel.
 * Limits: interp 1..256, n_taps 1..65536, n_channels 1..65535*8, finite gains (a non-finite freq counts as 0, as in
 * lorahip_channelizer_phase_inc), and 8 * (256 + ceil(n_taps/interp)) samples must fit the LDS (ceil(n_taps/interp) <= 2295).
 * Limits of one call (a longer stream is fed in several calls): at most 2^30 outputs (8 GiB), and tiles x phase blocks =
 * (n_in / 256 + 2) * ceil(interp / 8) at most 2^31 - 1 (the launch grid). Anything beyond a limit is refused with
 * LORAHIP_E_INVALID and a lorahip_last_error() text, consumes nothing and leaves the stream state untouched. Rows, strides
 * and the stream position are addressed with 64 bits.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_synthesizer lorahip_synthesizer;
int lorahip_synthesizer_create(lorahip_synthesizer **out, lorahip_ctx *ctx, size_t n_channels, const double *freq,
                               const float *gain /* nullable */, size_t interp, const float *taps, size_t n_taps);
void lorahip_synthesizer_destroy(lorahip_synthesizer *s);
int lorahip_synthesizer_reset(lorahip_synthesizer *s);
size_t lorahip_synthesizer_out_count(const lorahip_synthesizer *s, size_t n_in);      /* n_in * interp; 0 for NULL */
int lorahip_synthesizer_run(lorahip_synthesizer *s, const float *in_dev, size_t in_stride, size_t n_in,
                            float *wide_dev, size_t *n_out);

/* -------------------------------------------------------------------------------------
 * Polyphase filter-bank channeliser: the front end for a UNIFORM channel plan, K channels on the grid fs / M (lorahip_pfb.hip).
 * NOT a reference component. For M = n_bins a power of two, b / M is exact in the 64-bit phase counter --
 * lorahip_channelizer_phase_inc(b / M) == (b mod M) * 2^64 / M --, and row i of this object is BY DEFINITION what the channeliser
 * above defines for freq = bins[i] / M (x[n] = the wideband stream since the last reset, x[n<0] = 0, D = decim, L = n_taps, h = taps,
 * b = bins[i]):
 *
 *     n_m    = (m + 1) D - 1
 *     y_b[m] = sum_{j<L} h[j] x[n_m - j] exp(-2 pi i b (n_m - j) / M)
 *
 * evaluated as M folded sums and one forward M-point DFT per output time, whatever the number of rows:
 *
 *     v_s[m] = sum_{j<L, (n_m - j) mod M == s} h[j] x[n_m - j]
 *     y_b[m] = sum_{s<M} v_s[m] exp(-2 pi i b s / M)
 *
 * in fp32 (fused multiply-add; the fold runs over j = r, r + M, ... in ascending order, the transform is an ordinary radix-2
 * decimation-in-frequency FFT with twiddles computed in double). The phase is the stream position modulo M: integer arithmetic, no
 * drift, and a stream cut into arbitrary chunks gives bit-identical outputs to one call. The values agree with the direct form's
 * within the tolerance both are held to (4e-6 sum|h| max|x|), not bit for bit. Each fold runs over the taps below L only (the
 * padding of the tap table to whole rounds of M is never multiplied), so a NaN or Inf at sample n reaches exactly the outputs
 * with n_m - L < n <= n_m, as in the direct form.
 * bins: n_sel entries, any int32, taken modulo M (negative bins are the lower half of the band, duplicates are allowed); NULL: the
 * bins 0 .. n_bins - 1 in order (n_sel must be n_bins then). The centre frequencies bins[i] / M are what a lorahip_synthesizer or a
 * lorahip_channelizer takes for the same plan.
 * run(): consumes n_in samples, writes *n_out = lorahip_pfb_out_count(p, n_in) samples of row i at out_dev + 2*i*out_stride floats
 * (complex64, out_stride in samples >= *n_out). Asynchronous on the context's stream. Between calls the object keeps the stream
 * position and the trailing samples the next outputs reach back to (n_taps rounded up to a multiple of n_bins, less one).
 * Limits: n_bins a power of two in 8..1024 (lorahip_pfb_check / lorahip_pfb_create) or 5 * 2^a, a = 0..6 (the _radix5 pair below);
 * decim 1..4096, n_taps 1..65536, n_sel 1..65535*8; lorahip_pfb_check answers for these four without a device (LORAHIP_OK or
 * LORAHIP_E_INVALID). Limits of one call (a longer stream is fed in several calls): at most 2^30 outputs per row, and tiles <=
 * outputs / T + 2 (T = the largest power of two with T * n_bins <= 4096, 16 at least, 256 at most; a call may start and end inside
 * a tile) at most 2^31 - 1 (the launch grid). Anything beyond a limit is refused with LORAHIP_E_INVALID and a
 * lorahip_last_error() text, consumes nothing and leaves the stream state untouched. Rows, strides and the stream position are
 * addressed with 64 bits.
 *
 * Bin counts 5 * 2^a: M = 5, 10, 20, 40, 80, 160, 320 -- the grids of the LoRaWAN plans with 125 kHz channels 200 kHz apart, where
 * decim / n_bins = 8 / 5 (fs = 1 MHz: M = 5, D = 8 ... fs = 16 MHz: M = 80, D = 128). lorahip_pfb_check_radix5 and
 * lorahip_pfb_create_radix5 take the arguments of lorahip_pfb_check and lorahip_pfb_create with the same limits, meanings, refusal
 * texts ("polyphase channeliser ...") and untouched state on refusal; they accept these seven bin counts and nothing else (powers of
 * two are refused here as 5 * 2^a is refused there: the two pairs are disjoint). The handle is a lorahip_pfb: run, reset, out_count
 * and destroy serve it unchanged. One difference in the definition: for these M, b / M is NOT exact in the direct form's 64-bit
 * phase counter (lorahip_channelizer_phase_inc(b / M) is off by less than 2^-64 cycle per sample), so the rows are defined by the
 * folded formula above, i.e. by the exact phase b (n mod M) / M:
 *
 *     y_b[m] = sum_{j<L} h[j] x[n_m - j] exp(-2 pi i b ((n_m - j) mod M) / M)
 *
 * They agree with a lorahip_channelizer for freq = bins[i] / M far inside the tolerance both are held to. The transform is one
 * radix-5 decimation-in-frequency stage (a 5-point DFT over the points M / 5 apart, constants and twiddles exp(-2 pi i r n / M) from
 * a table computed in double) followed by five radix-2 transforms of M / 5 points; everything else is as above.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_pfb lorahip_pfb;
int lorahip_pfb_check(size_t n_bins, size_t decim, size_t n_taps, size_t n_sel);       /* host only */
int lorahip_pfb_create(lorahip_pfb **out, lorahip_ctx *ctx, size_t n_bins, const int32_t *bins /* nullable */, size_t n_sel,
                       size_t decim, const float *taps, size_t n_taps);
int lorahip_pfb_check_radix5(size_t n_bins, size_t decim, size_t n_taps, size_t n_sel);   /* host only */
int lorahip_pfb_create_radix5(lorahip_pfb **out, lorahip_ctx *ctx, size_t n_bins, const int32_t *bins /* nullable */, size_t n_sel,
                              size_t decim, const float *taps, size_t n_taps);
void lorahip_pfb_destroy(lorahip_pfb *p);
int lorahip_pfb_reset(lorahip_pfb *p);
size_t lorahip_pfb_out_count(const lorahip_pfb *p, size_t n_in);
int lorahip_pfb_run(lorahip_pfb *p, const float *wide_dev, size_t n_in, float *out_dev, size_t out_stride, size_t *n_out);

/* -------------------------------------------------------------------------------------
 * Integer IQ input for the two receive front ends above. Radios and recordings hand out pairs of 16-bit or 8-bit integers; the
 * *_run_iq entry points take them as they are, so the link to the device and the wideband buffer carry 4 or 2 bytes a sample
 * instead of 8 and no conversion pass runs: the kernels convert in the load. Definition, the only one: sample n of a chunk of
 * format f is
 *
 *     x[n] = (scale * (float)I[n], scale * (float)Q[n])
 *
 * -- each component converted int -> float exactly, then multiplied by scale ONCE in fp32, an operation of its own (never fused
 * into what follows) -- and everything after that is the cf32 definition of the object, operation for operation. Hence
 * run_iq(ints, f, scale) gives, bit for bit, what run gives on the cf32 array scale * (float)ints, for every object, shape,
 * chunking and stream position. The history an object keeps between calls holds converted samples: consecutive calls on one stream
 * may change format and scale freely, and a stream fed partly as integers and partly through the plain run is bit-identical to the
 * all-cf32 stream. scale is the caller's (2^-15 and 2^-7 map full scale to +-1); any finite value, 0 and negative ones included.
 * wide_dev: n_in samples of I, Q pairs in the format's type, aligned to the sample size (4 / 2 / 8 bytes) and no more: any sample
 * offset into a ring buffer will do. For run_captures_iq, capture_stride counts samples of the format.
 * The limits, refusals, *n_out, stream-state rules and asynchrony are exactly those of lorahip_channelizer_run /
 * lorahip_channelizer_run_captures / lorahip_pfb_run (lorahip_pfb_run_iq serves handles of lorahip_pfb_create and
 * lorahip_pfb_create_radix5 alike). Refused in addition, with LORAHIP_E_INVALID and a lorahip_last_error() text ("channeliser:
 * ...", "polyphase channeliser: ..."): an unknown format, a non-finite scale, LORAHIP_IQ_CF32 with scale != 1.0f, wide_dev not
 * aligned to the sample size. A refusal consumes nothing and leaves the stream state untouched. LORAHIP_IQ_CF32 with scale 1.0f is
 * the plain run. The transmit side writes the same formats: "Integer IQ output for the two synthesisers" at the end of this file.
 * ------------------------------------------------------------------------------------- */
#define LORAHIP_IQ_CF32 0   /* float I, float Q: 8 bytes a sample; scale must be 1.0f; identical to the plain run */
#define LORAHIP_IQ_SC16 1   /* int16 I, int16 Q: 4 bytes a sample */
#define LORAHIP_IQ_SC8  2   /* int8 I, int8 Q: 2 bytes a sample */
size_t lorahip_iq_sample_bytes(int format);    /* host only: 8 / 4 / 2, 0 for anything else */
int lorahip_channelizer_run_iq(lorahip_channelizer *c, const void *wide_dev, int format, float scale, size_t n_in, float *out_dev,
                               size_t out_stride, size_t *n_out);
int lorahip_channelizer_run_captures_iq(lorahip_channelizer *c, const void *wide_dev, int format, float scale, size_t n_captures,
                                        size_t capture_stride /* samples */, size_t n_in, float *out_dev, size_t out_stride, size_t *n_out);
int lorahip_pfb_run_iq(lorahip_pfb *p, const void *wide_dev, int format, float scale, size_t n_in, float *out_dev, size_t out_stride,
                       size_t *n_out);

/* -------------------------------------------------------------------------------------
 * Polyphase synthesis filter bank: the transmit front end for a UNIFORM channel plan, K channel streams onto the grid fs / M
 * (lorahip_psb.hip). The mirror image of lorahip_pfb_*. NOT a reference component. For M = n_bins a power of two, b / M is exact in
 * the 64-bit phase counter, and the output of this object is BY DEFINITION what the synthesiser above defines for
 * freq[k] = bins[k] / M (x_k[m] = channel k's stream since the last reset, x_k[m<0] = 0, U = interp, L = n_taps, h = taps,
 * g = gain, NULL: all 1, b_k = bins[k]):
 *
 *     y[n] = sum_k g_k exp(+2 pi i b_k n / M) sum_{j<L, (n-j) mod U == 0, n-j >= 0} h[j] x_k[(n-j)/U]
 *
 * evaluated as one gather and one inverse M-point DFT per INPUT time and a fold per output, whatever the number of rows (p = n mod U):
 *
 *     X_b[m] = sum_{k : b_k mod M == b} g_k x_k[m]
 *     u_s[m] = sum_{b<M} X_b[m] exp(+2 pi i b s / M)
 *     y[n]   = sum_{i : p + iU < L} h[p + iU] u_{n mod M}[n/U - i]
 *
 * in fp32 (fused multiply-add; the rows of a bin are summed in ascending k with the gain applied there, the transform is an ordinary
 * radix-2 decimation-in-frequency FFT with twiddles computed in double, the fold runs over i in ascending order). The phase is the
 * stream position modulo M: integer arithmetic, no drift, and a stream cut into arbitrary chunks gives bit-identical outputs to one
 * call. The values agree with the direct form's within the tolerance both are held to (4e-6 of max|x| sum|g| max_p sum_i |h[p + iU]|),
 * not bit for bit. Each fold runs over the taps below L only (no product with padding is formed), so a NaN or Inf in x_k[m] makes
 * exactly the outputs m U .. m U + L - 1 non-finite, as in the definition -- not the direct synthesiser's whole rounds of U. Output
 * phases without a tap (L < U) are exact zeros. n_in samples per row always give exactly n_in * interp outputs.
 * bins: n_sel entries, any int32, taken modulo M (negative bins are the lower half of the band; rows that share a bin are summed);
 * NULL: the bins 0 .. n_bins - 1 in order (n_sel must be n_bins then). bins[k] / M is what a lorahip_synthesizer, a
 * lorahip_channelizer or a lorahip_pfb takes for the same plan.
 * run(): row k of the input is the n_in complex64 samples at in_dev + 2*k*in_stride floats (in_stride in samples >= n_in);
 * writes *n_out = lorahip_psb_out_count(p, n_in) = n_in * interp samples at wide_dev. Asynchronous on the context's stream. Between
 * calls the object keeps the stream position and the transforms u_s[m] of the last ceil(L/U) - 1 input times; a call works through
 * a device workspace of at most 32 MiB that grows on first use.
 * Limits: n_bins a power of two in 8..1024 (lorahip_psb_check / lorahip_psb_create) or 5 * 2^a, a = 0..6 (the _radix5 pair below);
 * interp 1..4096, n_taps 1..65536, n_sel 1..65535*8; lorahip_psb_check answers for these
 * four without a device (LORAHIP_OK or LORAHIP_E_INVALID); finite gains. Limit of one call (a longer stream is fed in several
 * calls): at most 2^30 outputs (8 GiB); a call is worked off in segments whose launch grids stay far below 2^31 - 1. Anything
 * beyond a limit is refused with LORAHIP_E_INVALID and a lorahip_last_error() text that begins "polyphase synthesiser", consumes
 * nothing and leaves the stream state untouched. Rows, strides and the stream position are addressed with 64 bits.
 *
 * Bin counts 5 * 2^a: M = 5, 10, 20, 40, 80, 160, 320 -- the transmit side of the LoRaWAN plans with 125 kHz channels 200 kHz apart,
 * where interp / n_bins = 8 / 5 (fs = 1 MHz: M = 5, U = 8 ... fs = 64 MHz: M = 320, U = 512). lorahip_psb_check_radix5 and
 * lorahip_psb_create_radix5 take the arguments of lorahip_psb_check and lorahip_psb_create with the same limits, meanings, refusal
 * texts ("polyphase synthesiser ...") and untouched state on refusal; they accept these seven bin counts and nothing else (powers of
 * two are refused here as 5 * 2^a is refused there: the two pairs are disjoint). The handle is a lorahip_psb: run, reset, out_count
 * and destroy serve it unchanged, with the same 2^30 outputs a call, the same workspace and carried history. One difference in the
 * definition: for these M, b / M is NOT exact in the direct form's 64-bit phase counter (lorahip_channelizer_phase_inc(b / M) is off
 * by less than 2^-64 cycle per sample), so the output is defined by the exact phase b (n mod M) / M:
 *
 *     y[n] = sum_k g_k exp(+2 pi i b_k (n mod M) / M) sum_{j<L, (n-j) mod U == 0, n-j >= 0} h[j] x_k[(n-j)/U]
 *
 * evaluated as the three formulas above (gather X_b[m], inverse M-point DFT u_s[m], fold over i ascending with the taps below L
 * only). It agrees with a lorahip_synthesizer for freq[k] = bins[k] / M far inside the tolerance both are held to. Chunked calls are
 * bit-identical to one call, phases without a tap are exact zeros, and a NaN or Inf in x_k[m] makes exactly the outputs
 * m U .. m U + L - 1 non-finite, as above. The transform is one radix-5 decimation-in-frequency stage (a 5-point DFT over the points
 * M / 5 apart, constants and twiddles exp(+2 pi i r n / M) from a table computed in double) followed by five radix-2 transforms of
 * M / 5 points: the receive bank's, with the conjugate tables.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_psb lorahip_psb;
int lorahip_psb_check(size_t n_bins, size_t interp, size_t n_taps, size_t n_sel);      /* host only */
int lorahip_psb_create(lorahip_psb **out, lorahip_ctx *ctx, size_t n_bins, const int32_t *bins /* nullable */, size_t n_sel,
                       const float *gain /* nullable */, size_t interp, const float *taps, size_t n_taps);
int lorahip_psb_check_radix5(size_t n_bins, size_t interp, size_t n_taps, size_t n_sel);   /* host only */
int lorahip_psb_create_radix5(lorahip_psb **out, lorahip_ctx *ctx, size_t n_bins, const int32_t *bins /* nullable */, size_t n_sel,
                              const float *gain /* nullable */, size_t interp, const float *taps, size_t n_taps);
void lorahip_psb_destroy(lorahip_psb *p);
int lorahip_psb_reset(lorahip_psb *p);
size_t lorahip_psb_out_count(const lorahip_psb *p, size_t n_in);                       /* n_in * interp; 0 for NULL */
int lorahip_psb_run(lorahip_psb *p, const float *in_dev, size_t in_stride, size_t n_in, float *wide_dev, size_t *n_out);

/* -------------------------------------------------------------------------------------
 * Integer IQ output for the two synthesisers above. DACs, SDR transmit ports and recordings take pairs of 16-bit or 8-bit integers;
 * the *_run_iq entry points write them as they are, so the wideband buffer and the link from the device carry 4 or 2 bytes a sample
 * instead of 8 and no conversion pass runs: the kernels quantise in the store. Definition, the only one: let y be the cf32 output
 * sample of the object's definition above, operation for operation, and [lo, hi] = [-32768, 32767] (LORAHIP_IQ_SC16) or [-128, 127]
 * (LORAHIP_IQ_SC8). For each component c of y:
 *
 *     1. t = scale * c        one fp32 multiply, an operation of its own: never fused with the sum before it or anything after it
 *     2. r = rint(t)          in fp32: to nearest, ties to even
 *     3. stored: 0 if r is NaN, lo if r < lo, hi if r > hi, (int)r otherwise (so +Inf gives hi, -Inf gives lo)
 *     4. the component is CLIPPED if r is NaN or lies outside [lo, hi]
 *
 * Hence run_iq(rows, f, scale) stores, bit for bit, the same object's run(rows) quantised like this -- in numpy terms
 * clip(nan_to_num(rint(float32(scale) * y), nan=0, posinf=hi, neginf=lo), lo, hi) as integers -- for every shape, chunking, stream
 * position and output alignment. The state an object carries between calls stays cf32 and does not depend on the output format:
 * consecutive calls on one stream may alternate between run, sc16 and sc8 with any scales, and each call's outputs are the
 * quantisation of what run would have written at that stream position. The channel-rate rows stay cf32. scale is the caller's
 * (32767 and 127 map +-1 to full scale without a clip); any finite value, 0 and negative ones included.
 * wide_dev: room for *n_out samples of I, Q pairs in the format's type, aligned to the sample size (4 / 2 / 8 bytes) and no more: any
 * sample offset into a ring buffer will do. Nothing outside the *n_out samples is written. *n_out counts samples.
 * The limits, *n_out, stream-state rules and asynchrony are exactly those of lorahip_synthesizer_run / lorahip_psb_run
 * (lorahip_psb_run_iq serves handles of lorahip_psb_create and lorahip_psb_create_radix5 alike; 2^30 outputs a call at most).
 * Refused in addition, before anything else is looked at, with LORAHIP_E_INVALID, *n_out = 0 and a lorahip_last_error() text
 * ("synthesiser: ...", "polyphase synthesiser: ..."): an unknown format, a non-finite scale, LORAHIP_IQ_CF32 with scale != 1.0f,
 * wide_dev not aligned to the sample size. A refusal consumes nothing and leaves the stream state and the clip count untouched.
 * LORAHIP_IQ_CF32 with scale 1.0f is the plain run and counts nothing.
 * *_clipped: *count = the clipped components (I and Q counted separately) that the integer runs of this object have stored since
 * create or the last *_reset. It synchronises the context's stream and does not clear the count; *_reset clears it. Every sample
 * is bit-identical across chunkings, so the count of a stream is too. A NULL handle or a NULL count is LORAHIP_E_INVALID.
 * ------------------------------------------------------------------------------------- */
int lorahip_synthesizer_run_iq(lorahip_synthesizer *s, const float *in_dev, size_t in_stride, size_t n_in, void *wide_dev, int format,
                               float scale, size_t *n_out);
int lorahip_psb_run_iq(lorahip_psb *p, const float *in_dev, size_t in_stride, size_t n_in, void *wide_dev, int format, float scale,
                       size_t *n_out);
int lorahip_synthesizer_clipped(lorahip_synthesizer *s, unsigned long long *count);
int lorahip_psb_clipped(lorahip_psb *p, unsigned long long *count);

/* -------------------------------------------------------------------------------------
 * Rational-rate resampler: K rows of complex64 at one rate -> the same rows at up / down times that rate (lorahip_resamp.hip). The
 * block between the rate a radio delivers and the rates the four front ends above take (2.4 Msps x 5/6 = 2 Msps in front of a
 * channeliser of decim 16; 61.44 Msps x 25/24 = 64 Msps in front of lorahip_pfb_create_radix5(320, 512); 1.28 Msps rows x 25/256 =
 * 125 kHz in front of the demodulator; the same objects in reverse behind the synthesisers). K = 1 is a wideband stream, K > 1 the
 * rows a channeliser writes or a synthesiser reads. NOT a reference component.
 * Definition (x_k[n] = row k of the stream since the last reset, x_k[n<0] = 0, U = up, D = down, L = n_taps, h = taps, real):
 *
 *     t_m    = (m + 1) D - 1                        (output m sits at this instant of the U-times zero-stuffed stream)
 *     y_k[m] = sum_{j<L, (t_m - j) mod U == 0, t_m - j >= 0} h[j] x_k[(t_m - j) / U]
 *
 * i.e. zero-stuff by U, low-pass with h, keep every D-th sample. After N input samples per row exactly floor(N U / D) outputs per row
 * exist: a call of n_in samples at stream position n0 writes floor((n0 + n_in) U / D) - floor(n0 U / D) outputs per row -- possibly 0,
 * the same count for every row --, which is what lorahip_resampler_out_count answers for the next call. With U = 1 this is the
 * channeliser's definition at frequency 0, with D = 1 the synthesiser's for one row at frequency 0 and gain 1 (the same values within
 * the tolerance all three are held to, not bit for bit). Pass U * design_lowpass(max(U, D), L) for unit passband gain and a cutoff
 * at the lower of the two Nyquist rates.
 * Evaluated in fp32: with p = t_m mod U, c = floor(t_m / U), T = ceil(L / U) and the taps padded with zeros to T whole rounds of U,
 * each component of y_k[m] is ONE chain of T fused multiply-adds acc = fma(h[p + i U], x_k[c - i], acc) over i = 0 .. T - 1 from
 * acc = 0. Nothing in it depends on how the stream was cut into calls: arbitrary chunks give bit-identical outputs to one call. The
 * stream position is a 64-bit counter; n0 U, t_m and the row addressing are evaluated in 64 bits.
 * Non-finite samples follow the synthesiser's rule: the products with the padding ARE formed, so a NaN or Inf in x_k[c] makes
 * non-finite exactly the outputs m of row k with floor(t_m / U) - T < c <= floor(t_m / U); every other output and every other row
 * is untouched. A phase without a tap (p >= L, possible when L < U) gives exact zeros whatever the input holds.
 * run(): row k of the input is the n_in complex64 samples at in_dev + 2*k*in_stride floats (in_stride in samples >= n_in), row k of
 * the output goes to out_dev + 2*k*out_stride floats (out_stride in samples >= the output count); *n_out = the count. Asynchronous
 * on the context's stream. Between calls the object keeps the stream position and the T - 1 trailing samples of every row (nothing
 * when L <= U).
 * run_iq(): the input rows are LORAHIP_IQ_CF32, LORAHIP_IQ_SC16 or LORAHIP_IQ_SC8 samples (in_stride counts samples of the format;
 * the definition, alignment and refusals of "Integer IQ input" above), converted in the kernel's load: bit-identical to run() on
 * scale * (float)ints, and free to alternate with run() on one stream. The output stays cf32.
 * reset(): a new stream at position 0. reset_at(position): a new stream whose samples before `position` are zeros and whose first
 * sample is number `position` (<= 2^52): a capture that stays phase-aligned with an earlier recording.
 * Limits: up and down 1..1024 each, n_taps 1..65536, n_rows 1..65535*8, stream position + n_in <= 2^52; lorahip_resampler_check
 * answers for the first four without a device (LORAHIP_OK, or LORAHIP_E_INVALID and a lorahip_last_error() text). A workgroup keeps
 * the input span of its tile in LDS: with U' = U / gcd, D' = D / gcd, one row of a tile of NS output steps x PB = min(U', 32) phases
 * spans (NS - 1) D' + T + ceil((PB - 1) D / U) + 1 samples, rounded up to a multiple of D', next to its NS PB outputs; NS is a power
 * of two, 64 .. 512 where that fits 64 KiB, 64 where it fits 160 KiB (20480 samples), and halves down to 1 where it does not, so
 * every up / down is served and the bound is on the taps alone: T = ceil(n_taps / up) <= 16384 always fits; beyond that D' decides, and what does not fit is refused by _check and
 * _create. Limits of one call (a longer stream is fed in several calls): at most 2^30 outputs per row, and tiles x phase blocks =
 * (outputs / (NS U') + 2) * ceil(U' / 32) at most 2^31 - 1 and times the up to 512 threads of a workgroup below 2^32 (the launch
 * grid; the second binds only where NS < 64, since a workgroup of 512 threads then makes fewer than 512 outputs: at NS = 1 and
 * 32 phases, 16 threads per output and calls of up to 2^28 outputs). Anything beyond a limit, a NULL pointer (in_dev with
 * n_in > 0, out_dev with outputs to write) or a stride shorter than its count is refused with LORAHIP_E_INVALID and a
 * lorahip_last_error() text that begins "resampler", consumes nothing and leaves the stream state untouched.
 * lorahip_resampler_plan(): the tiling _create would choose for (up, down, n_taps, n_rows), host only like _check and refused exactly
 * where _check refuses (*plan is then all zeros). For tests and tuning: which branch of the kernel a shape lands on is read, not guessed.
 * ------------------------------------------------------------------------------------- */
typedef struct lorahip_resampler lorahip_resampler;
typedef struct lorahip_resampler_tiling
{
    size_t ns;              /* NS: output steps of one tile per phase, a power of two 1..512 */
    size_t rg;              /* RG: rows one workgroup serves, 1, 2, 4 or 8 (selects the kernel instance) */
    size_t pb;              /* PB: output phases of one workgroup, min(U', 32) */
    size_t n_phase_blocks;  /* workgroups per tile and row group, ceil(U' / PB) */
    size_t ti;              /* TI: input samples one workgroup stages per row, (NS - 1) D' + T + ceil((PB - 1) D / U) + 1 */
    size_t qp;              /* QP: slots per D' phase of the staged span in LDS, odd, D' QP >= TI */
    size_t waves;           /* wavefronts per workgroup, 1..8 */
    size_t lds_bytes;       /* dynamic LDS of one workgroup, RG (D' QP + NS PB) 8 */
    size_t t;               /* T = ceil(n_taps / up): fused multiply-adds per output component */
    size_t up_reduced;      /* U' = up / gcd(up, down) */
    size_t down_reduced;    /* D' = down / gcd(up, down) */
} lorahip_resampler_tiling;
int lorahip_resampler_check(size_t up, size_t down, size_t n_taps, size_t n_rows);     /* host only */
int lorahip_resampler_plan(size_t up, size_t down, size_t n_taps, size_t n_rows, lorahip_resampler_tiling *plan);   /* host only */
int lorahip_resampler_create(lorahip_resampler **out, lorahip_ctx *ctx, size_t n_rows, size_t up, size_t down, const float *taps,
                             size_t n_taps);
void lorahip_resampler_destroy(lorahip_resampler *r);
int lorahip_resampler_reset(lorahip_resampler *r);
int lorahip_resampler_reset_at(lorahip_resampler *r, uint64_t position);
size_t lorahip_resampler_out_count(const lorahip_resampler *r, size_t n_in);           /* of the next call; 0 for NULL and past 2^52 */
int lorahip_resampler_run(lorahip_resampler *r, const float *in_dev, size_t in_stride, size_t n_in, float *out_dev, size_t out_stride,
                          size_t *n_out);
int lorahip_resampler_run_iq(lorahip_resampler *r, const void *in_dev, int format, float scale, size_t in_stride, size_t n_in,
                             float *out_dev, size_t out_stride, size_t *n_out);

/* Measurement aid: one read-only streaming pass over n_bytes of device memory (pattern 0: linear
 * 16 B per lane; 1: the access shape of the tuned SF7 kernel). Time it with lorahip_timer_*; the
 * result is the practical HBM ceiling the roofline fraction can be compared with. */
int lorahip_membw_probe(lorahip_ctx *ctx, const float *buf_dev, size_t n_bytes, int pattern, int blocks_per_cu);

#ifdef __cplusplus
}
#endif
#endif /* LORAHIP_H */
