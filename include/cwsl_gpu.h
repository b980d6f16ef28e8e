/*
 * cwsl_gpu.h -- C ABI of libcwslgpu.so, the MI355X (gfx950) replacement for the
 * per-Instance CPU DSP chain of CWSL_DIGI.
 *
 * The reference has no plugin/FFI layer: the seam is a handful of C++ call sites.
 * Every entry point below names the reference interface it replaces (paths are
 * relative to the reference's source/ directory).  include/cwsl_gpu_shim.hpp
 * wraps this ABI back into SSBD- and Instance-shaped C++ classes so those call
 * sites compile unchanged; INTEGRATION.md shows the binding.
 *
 * Conventions: plain pointers and sizes only; every function returns a CWSLG_*
 * status (0 = OK, <0 = error); the library never falls back to a CPU path --
 * without a usable HIP device cwslg_create() fails with CWSLG_ERR_NO_DEVICE.
 * All entry points are thread-safe with respect to one context (one internal
 * mutex; device work is serialised on the context's HIP stream), mirroring the
 * reference's {Receiver thread} || {slot-clock thread} || {consumer} concurrency.
 */
#ifndef CWSL_GPU_H
#define CWSL_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWSLG_ABI_VERSION 5

/* ---- status codes ---- */
#define CWSLG_OK                  0
#define CWSLG_ERR_RATIO          -1  /* SSBD.hpp:54-55   "Fs/B must be an even integer >= 4"      */
#define CWSLG_ERR_BAND_LOW       -2  /* SSBD.hpp:100-101 "Signal outside of band (low)"           */
#define CWSLG_ERR_BAND_HIGH      -3  /* SSBD.hpp:102-103 "Signal outside of band (high)"          */
#define CWSLG_ERR_NOMEM          -4
#define CWSLG_ERR_MODE           -5  /* CWSL_DIGI.hpp:110-112 "Unhandled mode: ..."               */
#define CWSLG_ERR_ARG            -6
#define CWSLG_ERR_NO_DEVICE      -7  /* no HIP device / wrong arch: the product never runs on CPU */
#define CWSLG_ERR_HIP            -8
#define CWSLG_ERR_NO_FRAME       -9  /* nothing to fetch (e.g. first partial slot, Instance.cpp:224-227) */
#define CWSLG_ERR_UNSUPPORTED   -10  /* sample rate other than CWSL's 48/96/192 kHz               */
#define CWSLG_ERR_BLOCK         -11  /* n_complex not a multiple of SSBD::GetInSize() (= 2*Fs/B)  */

/* ---- slot-clock groups: CWSL_DIGI_Types.hpp:83-143 (SyncPredicates vectors) ---- */
#define CWSLG_GROUP_FT8     0   /* FT8, JS8                       (ft8Preds)    */
#define CWSLG_GROUP_FT4     1   /* FT4                            (ft4Preds)    */
#define CWSLG_GROUP_Q65_30  2   /* Q65-30                         (q65_30Preds) */
#define CWSLG_GROUP_S60     3   /* JT65, FST4-60                  (s60sPreds)   */
#define CWSLG_GROUP_S120    4   /* WSPR, FST4-120, FST4W-120      (s120sPreds)  */
#define CWSLG_GROUP_S300    5   /* FST4-300, FST4W-300            (s300sPreds)  */
#define CWSLG_GROUP_S900    6   /* FST4-900, FST4W-900            (s900sPreds)  */
#define CWSLG_GROUP_S1800   7   /* FST4-1800, FST4W-1800          (s1800sPreds) */
#define CWSLG_NUM_GROUPS    8

typedef struct cwslg_ctx cwslg_ctx;

/* One sync candidate (row a13 of SURVEY.md 8a: no reference counterpart; the layout is
 * builder-defined and the ordering is deterministic: by default descending sync, ties by ascending
 * freq_bin then ascending time_step; see cwslg_set_candidate_order). */
typedef struct {
    int32_t freq_bin;     /* FT8: 3.125 Hz bins of the 3840-point symbol spectrum               */
    int32_t time_step;    /* FT8: lag in quarter-symbol steps (40 ms), -62..+62                 */
    float   sync;         /* normalised Costas sync metric                                      */
    float   freq_hz;      /* freq_bin * df                                                      */
    float   dt_s;         /* (time_step - 0.5 s offset convention of the upstream decoder)      */
} cwslg_candidate;

/* ---- context ---- */
int  cwslg_abi_version(void);
/* device_ordinal < 0: use LOCAL_RANK from the environment if set, else 0. */
int  cwslg_create(cwslg_ctx **out, int device_ordinal);
void cwslg_destroy(cwslg_ctx *ctx);
const char *cwslg_strerror(int status);
/* Text of the last failure on this context (HIP error string included).  Safe from any thread; the pointer is to a per-thread copy,
 * valid until the same thread calls this function again. */
const char *cwslg_last_error(cwslg_ctx *ctx);
/* wsjtx.ftaudioscalefactor / wsjtx.wspraudioscalefactor (CWSL_DIGI.cpp:100-101; defaults 0.90 / 0.20) */
int  cwslg_set_scale_factors(cwslg_ctx *ctx, float scale_ft, float scale_wspr);

/* Arithmetic mode of the demodulator.
 *   on = 1, the DEFAULT of a new context ("exact"): the reference's own operation order (SSBD.hpp:160-183, un-fused float32,
 *           tap blocks oldest first).  The float frame, the int16 frame and therefore every candidate list equal the reference
 *           chain's (SSBD + Instance::prepareAudio + int16 conversion compiled from the reference's headers) BIT FOR BIT.
 *   on = 0  ("fast"): the fused polyphase form of the same filter (FMA, different summation order): about 1.5x the throughput of the whole path;
 *           float audio within 1e-5 of the frame's peak (measured 4e-7 with in-band signals; up to 6.6e-6 when the band is empty next
 *           to a strong out-of-band carrier, because the rounding noise scales with the INPUT level while the bound is relative to
 *           the frame's own peak -- DESIGN.md section 2 derives the bound); int16 samples differ by at most 1 LSB, and only where
 *           x*factor + 0.5 lies within that error of an integer; candidate lists equal the reference chain's keys except within 1e-3
 *           of a threshold, sync values within 1e-3.
 * Samples already pushed keep the mode they were pushed under.  A real-time receiver needs 0.3 % of either mode's throughput. */
int  cwslg_set_exact(cwslg_ctx *ctx, int on);

/* ---- receivers: replaces Receiver::init + the SPMC ring (Receiver.hpp:115-163, ring_buffer_spmc.h) ----
 * fs, iq_len, lo_hz are SM_HDR.SampleRate / BlockInSamples / L0 (SharedMemory.h:10-21, Receiver.hpp:86-88).
 * ring_blocks = 0 selects the reference depth 3*(fs/iq_len+1) blocks (Receiver.hpp:132).  The ring lives in HBM and is shorter than 4 GiB
 * (512 M samples: CWSLG_ERR_ARG beyond). */
int cwslg_receiver_open(cwslg_ctx *ctx, uint32_t fs, uint32_t iq_len, int32_t lo_hz,
                        uint32_t ring_blocks, int *rx_id);
int cwslg_receiver_close(cwslg_ctx *ctx, int rx_id);
/* Replaces the memcpy into the ring slot + inc_write_index (Receiver.hpp:247-249) AND the N per-Instance
 * pop_no_wait()/Iterate() loops (Instance.cpp:265-276): called ONCE per block per receiver.  The host block
 * is only read during the call.  n_complex must be a multiple of 2*fs/6000 (SSBD::GetInSize).
 * One call is one H2D copy and two context-mutex acquisitions: right for the reference's topology (a few receivers, many channels each).
 * A host that feeds THOUSANDS of private streams in real time must use cwslg_push_iq_many below (measured, profiles/r4_realtime.json: 4096
 * streams through this call fall behind -- 13.1 s of wall time for 5.2 s of signal; through the batched call 0 drops at 6.3 GB/s on a
 * quarter of a host core).  A receiver has one pusher at a time (Receiver.hpp:167); a second concurrent push of the same receiver,
 * by either call, is refused with CWSLG_ERR_ARG and nothing is accounted. */
int cwslg_push_iq(cwslg_ctx *ctx, int rx_id, const float *iq_interleaved, uint32_t n_complex);
/* One block of n_complex samples for EACH of n_rx receivers in one call -- the batched form of the per-block memcpy + inc_write_index of
 * Receiver::readIQ (Receiver.hpp:242-249) for a host that serves thousands of streams (the north star's 4096 private 192 kHz streams are
 * 384 000 blocks a second: through cwslg_push_iq that is as many H2D copies and twice as many context-mutex acquisitions; through this
 * call, with one batch per block period, 94 launches and 188 acquisitions).  iq[k] is receiver rx_ids[k]'s block (interleaved re, im; read
 * only during the call); every receiver of a batch gets the same n_complex (a multiple of SSBD::GetInSize for each of them) and may appear
 * once.  The blocks are copied into one pinned, host-mapped staging buffer (sized on demand) and ONE kernel scatters them into the rings;
 * frame-overflow accounting is per receiver with its own iq_len, exactly as n_rx calls of cwslg_push_iq would do it.  Thread safety: several
 * threads may push disjoint batches concurrently; a receiver must not be pushed from two threads at once (the reference has one thread per
 * Receiver, Receiver.hpp:167) -- detected and refused with CWSLG_ERR_ARG, nothing accounted. */
int cwslg_push_iq_many(cwslg_ctx *ctx, int n_rx, const int *rx_ids, const float *const *iq_interleaved, uint32_t n_complex);
/* Same, source already in device memory (tests, device-side producers). */
int cwslg_push_iq_device(cwslg_ctx *ctx, int rx_id, const void *d_iq_interleaved, uint32_t n_complex);
/* Synthetic IQ source standing in for CW Skimmer's shared memory (SharedMemory.cpp is Win32-only):
 * appends n_complex samples generated on the device.  The generator is the portable one specified in
 * DESIGN.md (integer Irwin-Hall noise + table-lookup tones) and is bit-identical to the oracle's.
 * tones_hz are relative to the LO; block_len = the push granularity used for the frame-overflow guard. */
int cwslg_push_synth(cwslg_ctx *ctx, int rx_id, uint64_t seed, uint32_t n_complex, uint32_t block_len,
                     const double *tones_hz, int n_tones, float amp);

/* Zero-copy producer: declare that the next n_complex samples ALREADY in the ring (written by a device-side
 * producer, or left there by an earlier lap) are new input.  Host bookkeeping only; nothing is copied.
 * block_len = granularity of the frame-overflow guard (0 = the receiver's iq_len). */
int cwslg_ring_commit(cwslg_ctx *ctx, int rx_id, uint32_t n_complex, uint32_t block_len);
/* cwslg_ring_commit on every open receiver of the context (one call per tick for thousands of streams). */
int cwslg_ring_commit_all(cwslg_ctx *ctx, uint32_t n_complex, uint32_t block_len);
/* Device address and capacity (complex samples) of the ring; *write_pos = ring index of the next sample. */
int cwslg_ring_info(cwslg_ctx *ctx, int rx_id, void **d_ring, uint32_t *capacity, uint64_t *total_pushed);

/* ---- channels: replaces SSBD<float>(Fs, SSB_BW, (float)demodFreq, USB) + Instance::init
 *      (Instance.cpp:121-176,183-187).  demod_hz = calibratedSSBFreq - LO (Instance.cpp:183).
 *      mode is the decoder= line's mode string ("FT8", "FT4", "WSPR", "FST4W-120", ...). ---- */
int cwslg_channel_open(cwslg_ctx *ctx, int rx_id, int32_t demod_hz, int usb, const char *mode, int *ch_id);
int cwslg_channel_close(cwslg_ctx *ctx, int ch_id);
/* SSBD::Tune(F, isUSB) with its default reset = true (SSBD.hpp:96-123): the channel gets a new tone and phasor step, its
 * filter history is forgotten and its phasor restarts at (1, 0); samples pushed before the call keep the old tuning and
 * the frame keeps filling where it was.  The band checks fail with the same two statuses / messages as at open, and then
 * leave the old tuning in place.  Like a Tune() on Instance's live SSBD object, the retune lasts until the demodulator is next
 * re-created: after every emitted frame Instance constructs a new SSBD from its OWN demodFreq / USB (Instance.cpp:251), and so
 * does cwslg_slot_boundary -- the channel is back on the tuning it was opened with.  (A lasting change of frequency is a new
 * channel, as band rotation is a new Instance in the reference, CWSL_DIGI.cpp:1217-1226.) */
int cwslg_channel_tune(cwslg_ctx *ctx, int ch_id, int32_t demod_hz, int usb);
/* SSBD::Tune(F, isUSB, reset) with its third argument (SSBD.hpp:97, :116-121).  reset != 0 is cwslg_channel_tune.  reset == 0 is the
 * phase-continuous retune: the filter history stays as it was mixed with the old tuning, the phasor continues from its live value
 * with the new step, the block count (Iterate's position) goes on -- so the 31 outputs after the retune point blend the two
 * tunings exactly as the reference's workspace does (bit-identical in exact mode; in the default mode those outputs are computed
 * in the reference's order and the rest within the usual 1e-5).  The reference never passes reset = false itself.
 * A second reset == 0 retune before 32 more blocks have been pushed returns CWSLG_ERR_UNSUPPORTED. */
int cwslg_channel_tune_ex(cwslg_ctx *ctx, int ch_id, int32_t demod_hz, int usb, int reset);
/* SSBD getters (SSBD.hpp:140-154) for the shim */
int cwslg_channel_info(cwslg_ctx *ctx, int ch_id, uint32_t *in_size, uint32_t *out_size,
                       uint32_t *out_rate, uint32_t *delay, size_t *frame_len);

/* ---- config.ini `decoder=` lines (source/CWSL_DIGI.cpp:731-837), accepted unchanged ----
 * "<freqHz> <MODE> [smnum [freqcal [callsign]]]" split on single spaces exactly like splitStringByDelim
 * (StringUtils.hpp:48-66: consecutive spaces yield empty fields), 2..5 fields, callsign only for WSPR.
 * calibrated_hz = (uint32)(freq / (freqcal_global * freqcal)) (:834).  No context needed. */
typedef struct {
    uint32_t freq_hz;          /* dial frequency as written                                   */
    uint32_t calibrated_hz;    /* what Instance tunes to (before subtracting the LO)          */
    char     mode[16];
    int32_t  smnum;            /* shared-memory interface number, -1 if not given (use radio.sharedmem) */
    double   freqcal;          /* per-decoder calibration factor (default 1.0)                */
    char     callsign[16];     /* per-decoder callsign (WSPR only), "" if not given           */
    int32_t  group;            /* CWSLG_GROUP_* of the mode                                   */
    uint32_t frame_len;        /* 12000*(period+5)                                            */
    float    period_s;
} cwslg_decoder_spec;
int cwslg_parse_decoder_line(const char *line, double freqcal_global, cwslg_decoder_spec *out);
/* Parse + open in one step: demod_hz = calibrated_hz - lo_hz of the receiver (Instance.cpp:183), USB. */
int cwslg_channel_open_line(cwslg_ctx *ctx, int rx_id, const char *line, double freqcal_global, int *ch_id);

/* ---- processing ----
 * Demodulate everything pushed so far for every channel (enqueued on the context stream; returns
 * without waiting).  push/slot_boundary/fetch call it implicitly when they have to. */
int cwslg_process(cwslg_ctx *ctx);
/* When is a cwslg_process() call worth a launch (ABI 5)?  The reference wakes every Instance once per block (Instance.cpp:260-276); a host
 * that mirrors this calls cwslg_process() after every push.  The bit-identical kernel starts every stream of outputs 32 blocks early (the
 * workspace of SSBD::ProcessBlock needs an output's 32 blocks), so a launch over 128 pending outputs per channel fetches and multiplies several
 * times what it delivers.  min_outputs = 0 (default): every call launches, as documented above.  min_outputs > 0: a call returns at once until
 * some channel has that many 12 kHz outputs pending.  min_outputs < 0: the library's own threshold (exact mode 20480 outputs = 1.7 s: one wave
 * per channel, 32 streams of 640 outputs, 5 % warm-up; fast mode 2048).  A slot boundary, a retune, a mode switch and ring pressure
 * (Receiver.hpp:222-229, "I/Q buffer is full!") always demodulate everything pending, whatever the threshold -- no sample is ever late for
 * its frame.  stats.demod_blocks_read x D / stats.demod_samples is the redundancy actually paid; stats.process_deferred counts the calls
 * that returned without a launch. */
int cwslg_set_process_threshold(cwslg_ctx *ctx, int min_outputs);
/* Demodulate everything pending NOW, whatever the threshold says (enqueued; returns without waiting).  For a host with a slot clock: called
 * ~100 ms before a boundary it leaves the boundary only the last few blocks to demodulate, so that frames and lists are final one
 * sync stage after the boundary call instead of one demod launch + one sync stage (cwsl_gpu_realtime --flush-before: 4096 channels,
 * 9.9-10.2 instead of 13.6 ms, profiles/r6_realtime.json). */
int cwslg_flush(cwslg_ctx *ctx);
/* The launch policy of the bit-identical kernel as a pure function (no context needed; for tests and capacity planning): outputs per stream for a
 * launch over total_blocks pending blocks (one block = one 12 kHz output), max_blocks of them on the busiest channel, on a chip of cu_count CUs
 * (0 = 256).  Every stream pays a 32-block warm-up, so a launch fetches and multiplies (1 + 32 / length) x what it delivers.  latency != 0: a
 * boundary's rule (the shortest launch: total / 65536, at least 4); 0: the rule of cwslg_process / cwslg_flush / ring pressure (at least one
 * full wave per channel: max_blocks / 32).  At most 1408. */
unsigned cwslg_exact_stream_length(uint64_t total_blocks, unsigned max_blocks, unsigned cu_count, int latency);
/* Replaces SyncPredicate::store(true) for every predicate of one group (CWSL_DIGI.cpp:247-251) and the
 * per-Instance reaction to it (Instance.cpp:203-253): swap frames, stamp the new frame with epoch_s,
 * finalise (peak-normalise + int16) the finished one unless its start time is 0, restart the demodulator. */
int cwslg_slot_boundary(cwslg_ctx *ctx, int group, uint64_t epoch_s);
/* (cwslg_slot_boundary and _begin fail with CWSLG_ERR_ARG while a boundary opened by _begin has not been ended.)
 * The same boundary in two halves, for a throughput host that keeps the GPU busy across boundaries (bench.py with N > 1): _begin queues
 * the boundary's device work and returns; the host queues the next slot's demodulation; _end waits for the boundary's own kernels
 * (not for the stream) and runs the rendezvous, which thereby overlaps the next demod launch.  Without a rendezvous installed _end
 * does nothing.  Do not fetch the epoch's frames or candidates before _end has returned; one boundary may be open at a time. */
int cwslg_slot_boundary_begin(cwslg_ctx *ctx, int group, uint64_t epoch_s);
int cwslg_slot_boundary_end(cwslg_ctx *ctx);
/* Same for a single channel (one SyncPredicate). */
int cwslg_slot_boundary_channel(cwslg_ctx *ctx, int ch_id, uint64_t epoch_s);
int cwslg_synchronize(cwslg_ctx *ctx);

/* ---- multi-GPU: the slot-boundary rendezvous ----
 * Channels never exchange data (Instance.cpp:260-276 reads its receiver's IQ and nothing else), so decoders shard over
 * one process per GPU -- by receiver first, as CWSL_DIGI.cpp:115-129 creates one Receiver per band -- with no data-path
 * collective.  What the reference's shared SyncPredicates give it for free (CWSL_DIGI_Types.hpp:83-143: every Instance
 * of a period family sees the same store(true)) becomes one tiny collective here: when a rendezvous is installed,
 * cwslg_slot_boundary() -- after it has queued finalise (+ sync) for its own channels and waited for its stream --
 * calls it with the number of frames this process emitted for the epoch and receives the total over all processes, so
 * every GPU publishes the epoch together.  The callback runs on the calling thread with the context unlocked; it must
 * not call back into the same context.  Return 0 or a negative CWSLG_ERR_*; the total is kept in the stats. */
typedef int (*cwslg_rendezvous_fn)(void *user, int group, uint64_t epoch_s, uint64_t frames_local, uint64_t *frames_total);
int cwslg_set_boundary_rendezvous(cwslg_ctx *ctx, cwslg_rendezvous_fn fn, void *user);
/* Built-in rendezvous (C/C++ hosts; bench.py's default for N > 1): ONE all-gather of 32 bytes per rank on RCCL over xGMI -- (frames,
 * group, epoch, flag) -- enqueued on the context's SIDE stream (the context stream may already hold the next slot's demodulation): every
 * rank sums the frames and checks that all ranks are at the same group and epoch; a mismatch fails the boundary on every rank with
 * CWSLG_ERR_ARG.  librccl is opened on first use (a process that already carries one, e.g. torch's, shares it).
 * cwslg_rccl_unique_id fills the 128-byte ncclUniqueId on rank 0; the host program hands it to the other ranks by any
 * means (cwsl_gpu_skimmer: a file); every rank then calls cwslg_rccl_init, which installs the rendezvous. */
/* A 64-bit flag word this process contributes to every later built-in rendezvous; stats.rendezvous_flags_and is the AND over all ranks
 * at the last one.  cwsl_gpu_skimmer sets bit 0 when its inputs are exhausted and leaves its loop when every rank has: a rank whose
 * band ends early keeps making the (collective) boundary calls until then instead of leaving the others blocked.  Only the built-in
 * form carries it (a callback rendezvous sees this process's own value). */
int cwslg_set_rendezvous_flag(cwslg_ctx *ctx, uint64_t flag);
#define CWSLG_RCCL_ID_BYTES 128
int cwslg_rccl_unique_id(void *id_out);
int cwslg_rccl_init(cwslg_ctx *ctx, const void *id, int rank, int world);

/* ---- results: replaces decoderPool->push(ItemToDecode(audio_i16, ...)) (Instance.cpp:244-245) ----
 * Copies the last finalised frame of the channel: frame_len = 12000*(period+5) int16 samples with the
 * reference's zero tail; *n_valid = samples actually demodulated in the slot; *start_epoch = the frame's
 * startEpochTime.  Returns CWSLG_ERR_NO_FRAME until a frame has been finalised.
 * Lifetime: the frame stays fetchable until the channel's NEXT emitting boundary replaces it.  The copy is atomic against that boundary
 * (the reference copies the frame into the ItemToDecode it pushes, Instance.cpp:238-245, DecoderPool.hpp:174-210): a fetch that started
 * before the boundary returns the old frame whole with the old start_epoch -- the boundary waits for it -- and one that starts after it
 * returns the new frame with the new start_epoch; samples of one slot are never delivered under the epoch of another.  A consumer more
 * than one slot late therefore sees only the newest frame (the reference's pool would drop the stale item by age, DecoderPool.hpp:358-374). */
int cwslg_fetch_frame(cwslg_ctx *ctx, int ch_id, int16_t *dst, size_t cap,
                      uint64_t *start_epoch, size_t *n_valid, float *factor);
/* Fetches and boundaries (ABI 5).  Every fetch of a result -- cwslg_fetch_frame, cwslg_fetch_slot, cwslg_fill_decoder_block and the four
 * candidate-list fetches -- reads only pointers under the context mutex, takes a ticket of the channel's slot-clock GROUP and copies with the
 * mutex released, on a fetch stream behind an event recorded after the boundary's kernels.  The next boundary of THAT group is the only writer
 * of those buffers and waits for the group's tickets before it queues its kernels, holding the context mutex.  Stall bound: a boundary of group
 * g can hold the context (pushes, cwslg_process, stats) for at most the longest copy of group g still in flight -- one frame + lists, i.e.
 * 0.36 MB (FT8) ... 3 MB (120 s modes) at PCIe speed, plus, for a fetch issued while kernels were still queued, the wait for those kernels
 * (at most the previous boundary's finalise + sync, or a demod launch: <= 40 ms at 4096 slots, ~0.1 ms in real-time operation).  Fetches of
 * OTHER groups never delay it.  A consumer that fetches within its slot period (the reference's pool drops items older than that,
 * DecoderPool.hpp:358-374) never meets the wait at all. */
#define CWSLG_LIST_NONE   0
#define CWSLG_LIST_FT8    1   /* cwslg_candidate records                                            */
#define CWSLG_LIST_FT4    2   /* cwslg_candidate records (+ cwslg_ft4_sync refinements)             */
#define CWSLG_LIST_WSPR   3   /* cwslg_wspr_candidate records                                       */
#define CWSLG_LIST_FST4W  4   /* cwslg_fst4w_candidate records                                      */
typedef struct {
    uint64_t start_epoch;     /* the frame's startEpochTime (Instance.cpp:215); every list below was computed from THIS frame */
    uint64_t n_valid;         /* samples demodulated in the slot                                                            */
    float    factor;          /* prepareAudio's scale factor                                                                */
    int32_t  list_kind;       /* CWSLG_LIST_*: record type written to `list`; NONE if no list of this epoch exists           */
    int32_t  n_list;          /* records written to `list`                                                                  */
    int32_t  n_ft4_sync;      /* records written to `ft4` (FT4 channels with the coherent stage on)                          */
} cwslg_slot_result;
/* The results of ONE epoch of one channel in one call and under one ticket -- the GPU-side counterpart of the ItemToDecode that carries
 * audio + startEpochTime together (DecoderPool.hpp:174-210, Instance.cpp:238-245): the int16 frame (frame may be NULL), the scale factor,
 * the channel's candidate list in its own record type (list_bytes = capacity of `list` in bytes; 0 / NULL to skip) and, for FT4 channels, the
 * coherent refinements.  Frame and lists can never belong to different slots. */
/* The last finalised frame as the reference's .wav (WaveFile.hpp:19-35,87-135: 46-byte RIFF/WAVE/fmt(18-byte
 * WAVEFORMATEX, PCM, mono, 12 kHz, 16 bit)/data header + the whole int16 frame) -- the file jt9/wsprd are given in
 * transfermethod=wavefile mode (DecoderPool.hpp:966-1046).  For the shared-memory mode pass &dec_data->d2[0]
 * to cwslg_fetch_frame instead (DecoderPool.hpp:588). */
int cwslg_write_wav(cwslg_ctx *ctx, int ch_id, const char *path);
/* ---- host service pieces: pure functions, usable without a context -----------------------
 * Slot clock: the first boundary instant (UTC milliseconds) of a mode group strictly after `after_ms` -- what the
 * reference's waitForTime* polling threads (CWSL_DIGI.cpp:174-451) converge on within one 25 ms poll: FT8 :00/:15/
 * :30/:45; FT4 the same plus 7.4 s later (the thread sleeps to 400 ms into seconds 7/22/37/52, :427-437); Q65-30
 * :00/:30; 60 s; 120/300/900/1800 s at second 0 of minutes divisible by 2/5/15/30.  Returns 0 for a bad group.
 * The epoch to hand to cwslg_slot_boundary() is edge_ms / 1000 (Instance.cpp:214 stamps whole seconds). */
uint64_t cwslg_slot_clock_next(int group, uint64_t after_ms);
/* Decoder-pool sizing (CWSL_DIGI.cpp:857-887).  counts[8] = decoders of FT4, FT8, Q65-30, JS8, WSPR, JT65, FST4W-*,
 * FST4-* in that order. */
int cwslg_pool_sizing(const int *counts, float decoderburden, int n_decoders, int *numjt9instances, int *maxwsprdinstances);
/* findBand (CWSL_Utils.hpp:28-55): index of the first band with |f - L0| <= Fs/2, or -1. */
int cwslg_find_band(const int64_t *lo_hz, const uint32_t *fs_hz, int n_bands, int64_t f_hz);

/* ---- decoder stdout -> spot record, every mode but JS8 -----------------------------------------------
 * JT65: "HHMM snr  dt freq #  message" (OutputHandler.cpp:623-695); Q65-30: FT8's columns (:697-780);
 * FST4-*: "HHMM snr  dt freq `  message" (OutputHandler.cpp:243-312); FST4W-*: the same columns with call, locator and
 * dBm as tokens (:152-240); WSPR: wsprd's eight tokens "id snr dt MHz drift call locator dBm" (:314-402).
 * One line of jt9's stdout ("HHMMSS snr  dt freq ~  message", fixed columns: OutputHandler.cpp:505-621) -> the
 * arguments reporter->handle() would receive (message rules: OutputHandler.cpp:924-1128; call / locator checks
 * :788-922, HamUtils.hpp:26-43).  base_freq_hz = the decoder's dial frequency (ItemToDecode::baseFreq).
 * CWSLG_SPOT_OK: call (and locator if has_locator) identify the transmitting station; CWSLG_SPOT_UNHANDLED: a well
 * formed line whose message the reference logs as "Message not handled"; CWSLG_SPOT_SKIP: not a decode line. */
#define CWSLG_SPOT_OK         0
#define CWSLG_SPOT_UNHANDLED  1
#define CWSLG_SPOT_SKIP       2
typedef struct {
    int32_t  snr_db;
    float    dt_s;
    uint32_t freq_hz;          /* audio offset + base frequency, truncated like static_cast<uint32_t> */
    int32_t  has_locator;
    char     call[16];
    char     locator[8];
    char     message[64];      /* the message text, trimmed (FT8 / FT4 / FST4)                        */
    int32_t  drift;            /* WSPR: Hz per minute                                                 */
    int32_t  dbm;              /* WSPR / FST4W: reported power                                        */
} cwslg_spot;
int cwslg_parse_decode_line(const char *mode, const char *line, int64_t base_freq_hz, cwslg_spot *out);

/* ---- decoder hand-off formats -------------------------------------------------------------
 * The block a stock jt9 (js8 = 0: dec_data_t, DecoderPool.hpp:58-108, "in sync with lib/jt9com.f90") or js8
 * (js8 = 1: dec_data_js8_t, :110-171) maps as shared memory.  cwslg_fill_decoder_block() does what
 * decodeUsingShMem() does between lock and unlock (:451-590): zero the block, set params and ipc for the channel's
 * mode, copy min(frame, 30*60*12000) int16 samples into d2 -- here straight from HBM, no intermediate vector.
 * Returns CWSLG_ERR_MODE for a mode that route rejects ("Unknown mode", :566-570), CWSLG_ERR_NO_FRAME before the
 * first finalised frame.  cwslg_decoder_block_field() gives offset/size of "ipc","ss","savg","sred","d2","params"
 * or of any params member by name (e.g. "nzhsym"). */
size_t cwslg_decoder_block_bytes(int js8);
int cwslg_decoder_block_field(int js8, const char *name, size_t *offset, size_t *bytes);
int cwslg_fill_decoder_block(cwslg_ctx *ctx, int ch_id, void *block, size_t block_bytes, int js8, int decodedepth,
                             int highest_decode_hz, uint64_t *start_epoch);
/* 1 = shared memory, 0 = wave file: the route DecoderPool gives an item of this mode (:379-395; WSPR, JS8 and the
 * FST4 family always go through a file). */
int cwslg_decoder_route(const char *mode, int transfer_shmem);
/* Program name ("jt9.exe" / "wsprd.exe" / "js8.exe") and argument string, character for character as
 * DecoderPool.hpp:634-659 (shared memory; target = key) and :1007-1046 (wave file; target = file name) build them. */
int cwslg_decoder_command(const char *mode, int shmem_route, int numjt9threads, int decodedepth, int highest_decode_hz,
                          int wspr_cycles, float trperiod, const char *target, char *app, size_t app_cap, char *opts,
                          size_t opts_cap);
/* The same frame as 12 kHz float audio BEFORE prepareAudio's scaling (for the 1e-5 check). */
int cwslg_fetch_audio_f32(cwslg_ctx *ctx, int ch_id, float *dst, size_t cap, size_t *n_valid);
/* Device pointers of the last finalised frame (valid until the next boundary of that channel). */
int cwslg_frame_device_ptrs(cwslg_ctx *ctx, int ch_id, const int16_t **d_i16, const float **d_f32);
/* Sync candidates of the last finalised frame (FT8/FT4 channels with sync enabled). */
int cwslg_enable_sync(cwslg_ctx *ctx, int enable, float syncmin, int max_cand, int f_lo_hz, int f_hi_hz);
/* Final ORDER and CUT of the FT8 / FT4 candidate lists (ABI 5).  Upstream's source is not in the reference tree, so which of the two a given
 * jt9 build does cannot be verified here (PARITY UNPINNED); both are implemented -- oracle, kernels and tests/indep_sync.py -- bit-identically:
 *   CWSLG_ORDER_SYNC_DESC (default): strongest first, the first max_cand kept.  Believed to mirror sync8.f90's "Sort by sync" lines (commented
 *       out in WSJT-X 2.x, live in 1.x) and getcandidates4.f90's list by height.
 *   CWSLG_ORDER_FREQ_ASC: ascending frequency, the first max_cand IN THAT ORDER kept -- believed to mirror WSJT-X 2.x sync8.f90 ("Sort by
 *       frequency": indexx on the frequency column, copy while k <= maxcand); entries of one bin stay in their order of discovery (the builder's
 *       tie rule: upstream's indexx is not stable).  FT4: the peaks as getcandidates4 finds them scanning upwards.  (Upstream's "nfqso first"
 *       promotion has no counterpart: the skimmer has no QSO frequency.)
 * The two lists hold the same entries unless the list is cut at max_cand; FT4's hold the same entries always (its scan stops at max_cand before
 * any ordering).  Applies from the next boundary on.
 * sync8's near-duplicate rule on the time axis is evaluated in single precision exactly as
 *       tdiff = fabsf(((float)lag_i - 0.5f) * tstep - ((float)lag_j - 0.5f) * tstep) < 0.04f,   tstep = 480 / 12000.0f,
 * under which 77 of the 124 lag pairs exactly one step apart count as duplicates and 47 do not (0.04 is not a binary fraction; the table is pinned
 * in tests/test_sync_oracle.py); a double-precision evaluation would make none of them duplicates.  Also unverifiable here. */
#define CWSLG_ORDER_SYNC_DESC 0
#define CWSLG_ORDER_FREQ_ASC  1
int cwslg_set_candidate_order(cwslg_ctx *ctx, int order);
/* *start_epoch (may be NULL) = start epoch of the frame the list was computed from: compare it with cwslg_fetch_frame's, or use
 * cwslg_fetch_slot, which returns both under one ticket (ABI 5; ItemToDecode carries epochTime with its audio, DecoderPool.hpp:174-210). */
int cwslg_fetch_candidates(cwslg_ctx *ctx, int ch_id, cwslg_candidate *dst, int max, int *n, uint64_t *start_epoch);
/* FT4 channels run getcandidates4's spectral-peak search instead (freq_hz = interpolated peak - 1.5 tone spacings,
 * sync = normalised peak height, time_step/dt_s = 0); its threshold defaults to upstream's 1.2. */
/* FT4 coherent sync (row a13; PARITY UNPINNED, restated from upstream ft4_decode / ft4_downsample / sync4d): every
 * getcandidates4 candidate of an FT4 channel is band-limited to a 666.7 Hz complex baseband around its frequency and
 * correlated with the four 4x4 Costas blocks over ft4_decode's three start-time segments (coarse then fine grid in start
 * sample and frequency tweak).  One record per candidate and segment that passes (sync >= 1.2, not weaker than segment 1,
 * 10 < f1 < 4990), in candidate order then segment order.  Enabled by default whenever sync is enabled.  A boundary at
 * which the stage is off makes a list and no records: until the next boundary with the stage on cwslg_fetch_ft4_sync
 * returns CWSLG_ERR_NO_FRAME and cwslg_fetch_slot returns n_ft4_sync = 0 -- never an older slot's records under the
 * newer epoch. */
typedef struct {
    float   f0_hz;        /* the getcandidates4 candidate                                            */
    float   f1_hz;        /* f0 + best frequency tweak (Hz)                                          */
    float   dt_s;         /* ibest / 666.67 - 0.5                                                    */
    float   sync;         /* sum of the four block correlation magnitudes / 64                       */
    int32_t ibest;        /* start sample of the first Costas block at 666.7 Hz                      */
    int32_t idf;          /* frequency tweak, Hz                                                     */
    int32_t seg;          /* 1..3: ft4_decode's start-time segment                                   */
    int32_t cand;         /* index into the cwslg_fetch_candidates list                              */
} cwslg_ft4_sync;
int cwslg_enable_ft4_coherent(cwslg_ctx *ctx, int enable);
int cwslg_fetch_ft4_sync(cwslg_ctx *ctx, int ch_id, cwslg_ft4_sync *dst, int max, int *n, uint64_t *start_epoch);
/* FT8 soft bits (row a13; PARITY UNPINNED, restated from upstream ft8b's nsym = 1 pass: its s8 magnitudes, the hard-decision Costas count
 * nsync, bmeta, normalizebmet, scalefac = 2.83).  One record per entry of the FT8 candidate list of the SAME epoch (record q belongs to entry q),
 * computed on the device from the symbol-spectra plane the search has just read, ON THE PLANE'S GRID -- one step (40 ms) by one bin (3.125 Hz),
 * the way ft8_lib decodes from its waterfall; this is not ft8b's 192 000-point downsample with its fine time / frequency search.  A consumer
 * (an in-process LDPC decoder, a pre-filter ahead of jt9 -- ft8b rejects nsync <= 6 --, a quality figure per spot) gets this without pulling the
 * 1.45 MB plane of every slot back to the host.  Off by default; while it is off nothing changes (launches, buffers, row pitch, lists).
 *   Addressing: i = freq_bin, j = time_step of the candidate; S(bin, m) the plane, m the 1-based step.  Symbol n = 0..78 sits at step
 *       m = j + 12 + 4 n, tone k = 0..7 at bin i + 2 k.
 *   Magnitudes: s8[n][k] = sqrtf(S(i + 2 k, m)), correctly rounded; 0 where m < 1, m > 372 or the bin is above 1920.
 *   nsync: over the 21 Costas symbols n = base + r (base 0, 36, 72; r = 0..6) the number whose FIRST maximum over k of s8[n][k] (ties to the
 *       lowest k, Fortran maxloc) is at k = icos7[r], icos7 = 3,1,4,0,6,5,2.
 *   Bit metrics: the 58 data symbols in the order n = 7..35, 43..71; graymap = 0,1,3,2,5,6,4,7, s2[v] = s8[n][graymap[v]]; three per symbol, MSB
 *       first, exact float32 max and subtract:
 *           b[p]   = max(s2[4..7])     - max(s2[0..3])
 *           b[p+1] = max(s2[2,3,6,7])  - max(s2[0,1,4,5])
 *           b[p+2] = max(s2[1,3,5,7])  - max(s2[0,2,4,6])
 *   Normalisation (normalizebmet), every operation un-fused float32, the sums in the order a 64-lane wave evaluates them: pad b to 192 entries
 *       with +0; a[l] = (b[l] + b[l+64]) + b[l+128], l = 0..63; six halving steps a[l] = a[l] + a[l+h] for l < h, h = 32, 16, 8, 4, 2, 1;
 *       S1 = a[0]; S2 the same tree over fl(b b); mean = S1 / 174.0f, m2 = S2 / 174.0f, var = m2 - fl(mean mean);
 *       sigma = sqrtf(var > 0 ? var : m2); llr[t] = fl(fl(b[t] / sigma) 2.83f), every llr +0 if sigma == 0.  llr > 0 means bit 1.
 *   Row pitch: tone 7 of a candidate at the upper edge bin ib lies at ib + 14, so while the feature is on the plane's row pitch
 *       (cwslg_sync_debug_fetch's row_len) is ib + 15 rounded up to 32 bins instead of ib + 13 (the default f_hi = 3000: 992 either way).
 * cwslg_enable_ft8_softbits needs the sync stage enabled (CWSLG_ERR_ARG otherwise) and applies from the next boundary on.
 * cwslg_fetch_ft8_softbits hands the records out like cwslg_fetch_candidates (same ticket, same count: min(list length, max)); it returns
 * CWSLG_ERR_MODE for a channel of another mode and CWSLG_ERR_NO_FRAME unless records, list and frame belong to one epoch -- after a boundary
 * that ran with the feature off there is nothing to fetch, never an older slot's records under the newer epoch. */
typedef struct { float llr[174]; float sigma; int32_t nsync; } cwslg_ft8_soft;   /* 704 bytes */
int cwslg_enable_ft8_softbits(cwslg_ctx *ctx, int enable);
int cwslg_fetch_ft8_softbits(cwslg_ctx *ctx, int ch_id, cwslg_ft8_soft *dst, int max, int *n, uint64_t *start_epoch);
/* FT8 decode (row a13; PARITY UNPINNED): flooding sum-product decoding of the LDPC(174,91) code on the 174 metrics of every cwslg_ft8_soft record,
 * then the CRC-14 -- the first consumer of those metrics, on the device: per candidate 91 bits, "is a codeword", "CRC matches" and an iteration
 * count (20 bytes) instead of 704 bytes over the link and belief propagation on the host.  Structured like upstream bpdecode174_91.  Out of scope:
 * ordered-statistics decoding (a stage of its own: FT8 OSD below), a-priori passes (a fetch of their own: FT8 a-priori decoding below), signal subtraction (a fetch of its own: FT8 signal subtraction below; a second pass over its residual stays out), unpacking the 77 bits into text.  De-duplication (neighbouring candidates of
 * one transmission repeat one message) is not this stage's either: cwslg_fetch_decodes below hands the words of a whole group out chosen and de-duplicated.  Off by default; while it is off nothing changes (launches, buffers, upload bytes, lists, records).
 *   The code is DATA THE CALLER LOADS: the WSJT-X source is not part of this repository and its parity-check table is not reproduced here.
 *       cwslg_set_ldpc_code takes the 83 x 7 table `Nm` of the integrator's own WSJT-X tree (recalled, not checked here, as lib/ft8/ldpc_174_91_c_parity.f90), row-major: entry =
 *       1-based codeword position 1..174, a row of weight 6 ends in one 0.  Validation: every position 1..174 occurs exactly three times; row
 *       weights are 6 or 7; zeros occur only as the last entry of a row; no position occurs twice in a row -- anything else is CWSLG_ERR_ARG and
 *       the loaded code, if any, stays.  Derived: per bit n its three checks in ascending row order c(n,0) < c(n,1) < c(n,2).  May be called
 *       again at any time; the new table applies to every launch queued after the call.  The call drains the context's streams and copies
 *       synchronously: it stalls the pipeline, so load a table once, not per slot.  Nothing in the kernel depends on which table it is.
 *   Arithmetic: every operation is ONE un-fused float32 operation, `/` correctly rounded.  Row m's edges are its entries in the caller's order,
 *       e = 0..w_m - 1; v[n][k] is the message from check c(n,k) to bit n, all +0 at the start.  The metrics are expected to be finite.
 *       State ncnt = 0, nclast = 0.  For it = 0, 1, ...:
 *         1. z[n] = ((llr[n] + v[n][0]) + v[n][1]) + v[n][2]; cw[n] = z[n] > 0.
 *         2. nbad = number of rows whose cw over their entries has odd parity.
 *         3. nbad == 0: exit, iters = it.
 *         4. it == max_iter: exit, iters = max_iter.
 *         5. it > 0: nd = nbad - nclast; ncnt = nd < 0 ? 0 : ncnt + 1; if ncnt >= 5 && it >= 10 && nbad > 15: exit, iters = it.
 *         6. nclast = nbad.
 *         7. every edge (m, e), n its bit, k the slot of m in n: t[m][e] = T(-0.5f * (z[n] - v[n][k])).
 *         8. every edge: p = product of t[m][e'] over e' != e in ascending e', starting from 1.0f; v[n][k] = 2.0f * A(-p).
 *       T(x): a = |x|; a >= 4.97f: 1.0f; otherwise x2 = a a, r = (a (945 + x2 (105 + x2))) / (945 + x2 (420 + x2 15)) (the [5/4] Pade form of
 *           tanh), r = fminf(r, 1.0f); the result is copysignf(r, x).
 *       A(y): z = |y|; z <= 0.664f: z / 0.83f; z <= 0.9217f: (z - 0.4064f) / 0.322f; z <= 0.9951f: (z - 0.8378f) / 0.0524f;
 *           z <= 0.9998f: (z - 0.9914f) / 0.0012f; otherwise 7.0f; the result is copysignf(., y).
 *   CRC-14: polynomial 0x2757 (x^14 implicit), bit-serial, MSB first, initial remainder 0, over bits 0..76 followed by 5 zero bits and then 14
 *       augmenting zero bits (the remainder of M(x) x^14 for the 82-bit M); crc_ok means that remainder, MSB first, equals bits 77..90 AND
 *       nbad == 0.  A consumer who needs another convention has all 91 bits and nbad.
 *   Record: bits = codeword positions 0..90 at exit (whether or not a codeword), MSB first; nharderr = #{t < 174 : (llr[t] > 0) != cw[t]}.
 *       A candidate whose nsync < min_nsync or whose sigma == 0 is NOT ATTEMPTED: iters = nbad = nharderr = -1, zero bits, crc_ok = 0.
 * cwslg_enable_ft8_decode(ctx, 1, max_iter 1..200 (upstream 30), min_nsync 0..22 (upstream 7)) returns CWSLG_ERR_ARG unless a code is loaded,
 * the sync stage is on and FT8 soft bits are on; switching it off is always allowed.  A boundary makes decode records only when soft bits and
 * decode are both on at that boundary: one launch behind the soft-bit launch, the candidate count read on the device.  That launch is counted in
 * stats.sync_launches (two per boundary with the decode on): sync_ms / sync_launches is then HALF the per-boundary time.  cwslg_fetch_ft8_decode behaves like cwslg_fetch_ft8_softbits: same ticket, record q belongs to list entry q, *n = min(list length,
 * max), CWSLG_ERR_MODE for a channel that is not FT8, CWSLG_ERR_NO_FRAME unless decode records, soft-bit records, list and frame are of one
 * epoch -- after a boundary that ran with the feature off there is nothing to fetch, never an older slot's records under a newer epoch.
 * cwslg_ldpc_decode runs the same kernel on n >= 0 caller-supplied sets of 174 metrics (host memory) with no nsync filter, synchronously; it
 * returns CWSLG_ERR_ARG without a loaded code.  It is the in-process path for FT4 metrics that are already on the host: fetch cwslg_ft4_soft, pass the
 * sets you want; on the device the FT4 chain has a stage of its own, cwslg_enable_ft4_decode below, which needs no fetch and no round trip.
 * Upstream's rvec descrambling of the 77 message bits stays with the consumer. */
typedef struct {
    uint8_t bits[12];     /* codeword positions 0..90 at exit, MSB first: bit t = bits[t>>3] & (0x80 >> (t&7)); the last 5 bits are 0 */
    int16_t iters;        /* iterations run; 0 = the hard decision of the llr was already a codeword; -1 = not attempted            */
    int16_t nbad;         /* unsatisfied checks at exit; 0 = a codeword; -1 when not attempted                                      */
    int16_t nharderr;     /* #{t < 174 : (llr[t] > 0) != cw[t]} at exit; -1 when not attempted                                      */
    uint8_t crc_ok;       /* nbad == 0 and the CRC-14 of bits 0..76 equals bits 77..90                                              */
    uint8_t pad_;
} cwslg_ft8_msg;          /* 20 bytes */
int cwslg_set_ldpc_code(cwslg_ctx *ctx, const uint8_t *nm /* [83*7] */);
int cwslg_enable_ft8_decode(cwslg_ctx *ctx, int enable, int max_iter, int min_nsync);
int cwslg_fetch_ft8_decode(cwslg_ctx *ctx, int ch_id, cwslg_ft8_msg *dst, int max, int *n, uint64_t *start_epoch);
int cwslg_ldpc_decode(cwslg_ctx *ctx, const float *llr /* [n][174] */, int n, int max_iter, cwslg_ft8_msg *out);
/* FT8 OSD (PARITY UNPINNED): ordered-statistics decoding, order 0, 1 or 2, of the candidates the decode above attempted and did not bring to
 * crc_ok -- the last stage of the chain on the device: 24 bytes per candidate instead of a second fetch of its 704 bytes of metrics and OSD on
 * the host.  This is the repository's OWN statement of OSD on the channel metrics; it is not upstream osd174_91, which takes reliabilities summed
 * over BP iterations and applies its own thresholds.  False accepts under a 14-bit CRC grow with the order: dmin, nharderr and how are handed
 * out so that the consumer can gate on them.  Off by default; while it is off nothing changes (launches, buffers, upload bytes, records).
 *   Inputs: llr[174] (float32), the loaded code with parity check H (83 x 174) of rank 83 (K = 91), order in {0, 1, 2}.
 *     1. a[t] = |llr[t]|, hard[t] = llr[t] > 0 (the decode record's own rule for z).  If any a[t] is not finite the record is NOT ATTEMPTED.
 *     2. Reliability order: position t comes before u iff a[t] > a[u], or a[t] == a[u] and t < u.
 *     3. Most reliable basis: walk the positions in that order; a position joins iff its column of a generator of the code is linearly
 *        independent over GF(2) of the columns already taken; stop at the 91st.  p_0 .. p_90 are the taken positions in joining order, nskip the
 *        number of positions passed over.  Both depend on the code and the order alone, not on which generator the host derived.
 *     4. Reduced basis: the unique codewords g_i with g_i[p_j] = (i == j).
 *     5. Order-0 word: c0 = XOR of the g_i with hard[p_i] = 1.
 *     6. Candidates: c0 (0 flips); order >= 1: c0 ^ g_i (91 words); order == 2: c0 ^ g_i ^ g_j, i < j (4095 words).
 *     7. Distance: d(c) = (((+0 + m_0 a[0]) + m_1 a[1]) + ...) + m_173 a[173], m_t = 1 iff c[t] != hard[t]: float32 adds in ascending t, one
 *        operation each, nothing fused (skipping a term and adding +0 give the same bits).
 *     8. Winner: the smallest d; ties go to fewer flips, then the smaller i, then the smaller j.
 *   Record: bits = the winner's codeword positions 0..90, packed as cwslg_ft8_msg.bits; crc_ok by the CRC-14 rule above on the winner (always a
 *     codeword).  A record that is not attempted has zero bits, dmin = +0, nharderr = nskip = -1, crc_ok = 0, how = flip[0] = flip[1] = 0xff.
 * cwslg_set_ldpc_code also derives the rank of H and a generator of its null space; it accepts exactly what it accepted before, and a table
 * whose rank is below 83 simply cannot have OSD enabled (loading one switches OSD off).  Loading a code replaces the generator for every launch
 * queued after the call.
 * cwslg_enable_ft8_osd(ctx, 1, order 0..2, min_nsync 0..22) returns CWSLG_ERR_ARG unless a code of rank 83 is loaded and the arguments are in
 * range; switching it off is always allowed.  Like the decode it takes effect only while FT8 soft bits and the FT8 decode are both on at a
 * boundary: then one launch follows the decode launch on the same stream, the candidate count read on the device, and candidate q is attempted
 * iff its cwslg_ft8_msg was attempted (iters >= 0) and has crc_ok == 0 and its soft-bit record has nsync >= min_nsync.  That launch is counted
 * in stats.sync_launches (three per boundary with soft bits, decode and OSD on): sync_ms / sync_launches is then A THIRD of the per-boundary
 * time.  cwslg_fetch_ft8_osd behaves like cwslg_fetch_ft8_decode: same ticket, record q belongs to list entry q, *n = min(list length, max),
 * CWSLG_ERR_MODE for a channel that is not FT8, CWSLG_ERR_NO_FRAME unless OSD, decode and soft-bit records, list and frame are of one epoch.
 * cwslg_osd_decode runs the same kernel on n >= 0 caller-supplied sets of 174 metrics (host memory) with no gates, synchronously; it returns
 * CWSLG_ERR_ARG without a loaded code of rank 83 or for an order outside 0..2.  The FT4 chain has the same stage: FT4 OSD, behind the FT4 decode
 * below. */
typedef struct {
    uint8_t bits[12];     /* the winner's codeword positions 0..90, MSB first, as cwslg_ft8_msg.bits; the last 5 bits are 0           */
    float dmin;           /* the winner's distance d                                                                                 */
    int16_t nharderr;     /* #{t < 174 : winner[t] != hard[t]}; -1 when not attempted                                                */
    int16_t nskip;        /* positions passed over while the basis was chosen; -1 when not attempted                                 */
    uint8_t crc_ok;       /* the CRC-14 of bits 0..76 equals bits 77..90                                                             */
    uint8_t how;          /* flips of the winner, 0..2; 0xff = not attempted                                                         */
    uint8_t flip[2];      /* i, j (joining order of the basis); 0xff where unused                                                    */
} cwslg_osd_msg;          /* 24 bytes */
int cwslg_enable_ft8_osd(cwslg_ctx *ctx, int enable, int order, int min_nsync);
int cwslg_fetch_ft8_osd(cwslg_ctx *ctx, int ch_id, cwslg_osd_msg *dst, int max, int *n, uint64_t *start_epoch);
int cwslg_osd_decode(cwslg_ctx *ctx, const float *llr /* [n][174] */, int n, int order, cwslg_osd_msg *out);
/* FT4 soft bits (row a13; PARITY UNPINNED, restated from upstream ft4_decode's last stage before LDPC: the final ft4_downsample at the corrected
 * frequency, get_ft4_bitmetrics' three metric sets, the sync-quality counts nsync / nqual, normalizebmet, scalefac = 2.83).  One record per
 * cwslg_ft4_sync record of the SAME epoch, in the same order -- candidate order, then segment order: record q belongs to entry q of
 * cwslg_fetch_ft4_sync -- computed on the device from the frame spectrum and the records the refinement has just written.  A consumer (an
 * in-process LDPC decoder, a pre-filter ahead of jt9, a quality figure per spot) gets this without pulling the int16 frame back and redoing the
 * 72576-point spectrum, the 4032-point inverse transform at f1 and 103 symbol transforms per record on the host.  Off by default; while it is
 * off nothing changes (launches, buffers, lists, frames).  Every operation below is one un-fused float32 operation except where an fmaf is written.
 *   Baseband: cb[0..4031] is exactly what the refinement stage computes for a candidate frequency, evaluated at f1_hz instead of f0_hz:
 *       i0 = lroundf(f1 / df), the same 630 windowed bins, the same 63 x 64 inverse transform, the same unit-mean-power normalisation over 4032
 *       samples (oracle/ft4sync_oracle.c:orc_ft4_downsample states it).  Upstream divides by NSS NN = 3296 here instead of 4032: that scales
 *       sigma only; the llr are scale-free up to rounding.
 *   Symbols: cd[32 k + t] = cb[ibest + 32 k + t], k = 0..102, t = 0..31; +0 where the index falls outside 0..4031.
 *   Symbol spectra: cs[k][q], q = 0..3, a 32-term chain in ascending t from z = (+0, +0) with c = cd[32 k + t] and
 *       w = w32[(q t) mod 32] = (float cos, float sin) of the double angle 2 pi p / 32 (the four cardinal points exact, as in the csync table):
 *           zr = fmaf(c.r, w.x, zr);  zr = fmaf(c.i, w.y, zr);
 *           zi = fmaf(c.i, w.x, zi);  zi = fmaf(-c.r, w.y, zi);
 *       The magnitude of a complex z is |z| = sqrtf(fmaf(z.r, z.r, z.i * z.i)) everywhere below; complex sums add real and imaginary parts.
 *   nsync (0..16): over the 16 Costas symbols k = 33 b + s (b, s = 0..3) the number whose FIRST maximum over q of |cs[k][q]| (ties to the lowest
 *       q) is at icos4[b][s]; the blocks are 0132 1023 2310 3201.  Upstream stops at nsync < 8; here every record is delivered and the consumer
 *       decides.
 *   Metric sets: three, of 206 entries each.  graymap g = 0,1,3,2; bit ib of a group of nb bits pairs with index bit nb - 1 - ib (most
 *       significant bit first); a metric is max(s2[i] : index bit set) - max(s2[i] : index bit clear), exact float32 max and subtract.
 *       Set 0: per symbol k, s2[v] = |cs[k][g[v]]|, v = 0..3 -> bm0[2 k + ib], ib = 0, 1.
 *       Set 1: pairs ks = 0, 2, ..., 100, i = 0..15: s2[i] = |cs[ks][g[i>>2]] + cs[ks+1][g[i&3]]| -> bm1[2 ks .. 2 ks + 3];
 *           bm1[204..205] = bm0[204..205].
 *       Set 2: groups ks = 0, 4, ..., 96, i = 0..255:
 *           s2[i] = |((cs[ks][g[i>>6]] + cs[ks+1][g[(i>>4)&3]]) + cs[ks+2][g[(i>>2)&3]]) + cs[ks+3][g[i&3]]| -> bm2[2 ks .. 2 ks + 7];
 *           bm2[200..203] = bm1[200..203], bm2[204..205] = bm0[204..205].
 *       The copies are taken before normalisation.
 *   nqual (0..32): hard[t] = (bm0[t] >= 0); the number of agreements with 0,0,0,1,1,0,1,1 at t = 0..7, 0,1,0,0,1,1,1,0 at t = 66..73,
 *       1,1,1,0,0,1,0,0 at t = 132..139 and 1,0,1,1,0,0,0,1 at t = 198..205 (the gray-decoded Costas blocks).  Upstream requires at least 20.
 *   Normalisation per set (normalizebmet over all 206 entries), the sums in the order a 64-lane wave evaluates them: pad b to 256 entries with
 *       +0; a[l] = ((b[l] + b[l+64]) + b[l+128]) + b[l+192], l = 0..63; six halving steps a[l] = a[l] + a[l+h] for l < h, h = 32, 16, 8, 4, 2, 1;
 *       S1 = a[0]; S2 the same tree over fl(b b); mean = S1 / 206.0f, m2 = S2 / 206.0f, var = m2 - fl(mean mean);
 *       sigma = sqrtf(var > 0 ? var : m2).
 *   llr[set][0..57], [58..115], [116..173] come from entries 8..65, 74..131, 140..197 (the data symbols), each fl(fl(b / sigma) 2.83f); every llr
 *       of a set +0 if its sigma == 0.  llr > 0 means bit 1.  (Upstream's rvec scrambling is a matter of the 77 message bits after decoding, not
 *       of the metrics.)
 * cwslg_enable_ft4_softbits needs the sync stage enabled (CWSLG_ERR_ARG otherwise) and applies from the next boundary on; a boundary at which
 * cwslg_enable_ft4_coherent is off produces no records.  cwslg_fetch_ft4_softbits hands the records out like cwslg_fetch_ft4_sync (same ticket,
 * *n = min(record count, max)); it returns CWSLG_ERR_MODE for a channel that is not FT4 and CWSLG_ERR_NO_FRAME unless soft records, sync
 * records, candidate list and frame belong to one epoch -- after a boundary that ran with the feature off there is nothing to fetch, never an
 * older slot's records under the newer epoch. */
typedef struct { float llr[3][174]; float sigma[3]; int32_t nsync; int32_t nqual; int32_t pad_; } cwslg_ft4_soft;   /* 2112 bytes */
int cwslg_enable_ft4_softbits(cwslg_ctx *ctx, int enable);
int cwslg_fetch_ft4_softbits(cwslg_ctx *ctx, int ch_id, cwslg_ft4_soft *dst, int max, int *n, uint64_t *start_epoch);
/* FT4 decode (row a13; PARITY UNPINNED): the FT8 decode above on the three metric sets of every cwslg_ft4_soft record, on the device, behind the
 * launch that has just written them -- per record three cwslg_ft8_msg (60 bytes) instead of 2112 bytes over the link, a choice of sets on the
 * host and a blocking cwslg_ldpc_decode.  FT4 and FT8 share the LDPC(174,91) code and the CRC-14: the code is the one cwslg_set_ldpc_code
 * loaded.  Off by default; while it is off nothing changes (launches, buffers, upload bytes, lists, records, frames).
 *   Record: set[s], s = 0..2, is exactly what the contract of cwslg_ft8_msg above yields for llr[s][0..173] of the record's cwslg_ft4_soft: the
 *       same arithmetic, the same exits, the same bits / iters / nbad / nharderr / crc_ok.  Nothing is restated or changed here.
 *   Gates: a record whose nsync < min_nsync or whose nqual < min_nqual is NOT ATTEMPTED in all three sets (iters = nbad = nharderr = -1, zero
 *       bits, crc_ok = 0).  Otherwise set s is not attempted exactly when sigma[s] == 0: its llr are all +0 then, which would "decode" to the
 *       all-zero codeword.  The three sets of a record are decoded side by side, each to its own exit.
 *   Which set "wins" is not stored.  Upstream tries the sets in order and stops at the first success: the smallest s with crc_ok
 *       (cwslgpu::ft4BestSet in cwsl_gpu_shim.hpp, ft4_best_set in the Python package; -1 if none).
 *   Out of scope: the rvec descrambling of the 77 message bits (the CRC is over the scrambled bits, so crc_ok does not need it), a-priori
 *       passes, unpacking to text, de-duplication, extending cwslg_fetch_slot.  Ordered-statistics decoding is a stage of its own: FT4 OSD below.
 * cwslg_enable_ft4_decode(ctx, 1, max_iter 1..200 (upstream 30), min_nsync 0..17 (upstream 8), min_nqual 0..33 (upstream 20)) returns
 * CWSLG_ERR_ARG unless a code is loaded, the sync stage is on and FT4 soft bits are on; switching it off is always allowed.  min_nsync 17 or
 * min_nqual 33 mean "nothing is attempted", as min_nsync 22 does for FT8.  A boundary makes decode records only when the coherent stage, FT4
 * soft bits and the decode are all on at that boundary: one launch behind the soft-bit launch, the candidate and record counts read on the
 * device.  That launch is counted in stats.sync_launches, as the FT8 decode's is (a boundary with FT4 channels alone then counts two: sync_ms /
 * sync_launches is HALF the per-boundary time).  cwslg_fetch_ft4_decode behaves like cwslg_fetch_ft4_softbits: same ticket, record q belongs to
 * entry q of cwslg_fetch_ft4_sync, *n = min(record count, max), CWSLG_ERR_MODE for a channel that is not FT4, CWSLG_ERR_NO_FRAME unless decode
 * records, soft records, sync records, list and frame are of one epoch -- after a boundary that ran with the feature, the soft bits or the
 * coherent stage off there is nothing to fetch, never an older slot's records under a newer epoch. */
typedef struct { cwslg_ft8_msg set[3]; } cwslg_ft4_msg;          /* 60 bytes */
int cwslg_enable_ft4_decode(cwslg_ctx *ctx, int enable, int max_iter, int min_nsync, int min_nqual);
int cwslg_fetch_ft4_decode(cwslg_ctx *ctx, int ch_id, cwslg_ft4_msg *dst, int max, int *n, uint64_t *start_epoch);
/* FT4 OSD (PARITY UNPINNED, as FT8 OSD above): ordered-statistics decoding, order 0, 1 or 2, of the metric sets of the records the FT4 decode
 * left without a word -- the last stage of the FT4 chain on the device, where the FT8 chain ends too: 72 bytes per record instead of a second
 * fetch of its 2112 bytes of metrics, a choice of sets on the host and a blocking cwslg_osd_decode.  Off by default; while it is off nothing
 * changes (launches, buffers, upload bytes, lists, records, frames).
 *   Record: set[s], s = 0..2, is exactly what the contract of cwslg_osd_msg above yields for llr[s][0..173] of the record's cwslg_ft4_soft: the
 *       same arithmetic, the same record, the same not-attempted record (also for a metric that is not finite).  Nothing of the OSD
 *       arithmetic is restated or changed here.
 *   Gate: set s of a record is attempted iff (1) its cwslg_ft8_msg (set[s] of the record's cwslg_ft4_msg) was attempted (iters >= 0), (2) NO
 *       set of that record has BP crc_ok, and (3) the soft record has nsync >= min_nsync and nqual >= min_nqual.
 *   The gate is per RECORD, not per set, on purpose: a record that BP decodes in set 1 alone does not have its sets 0 and 2 pushed through
 *       4187 words each.  Every such search has roughly a 1 % chance of a false accept under the 14-bit CRC, and under upstream's set order
 *       (first success wins) a false word in set 0 would be preferred to the true BP word in set 1.
 *   Which word "wins" is not stored: the smallest s with BP crc_ok; if there is none, the smallest s with OSD crc_ok, marked as found by OSD
 *       (cwslgpu::ft4BestWord in cwsl_gpu_shim.hpp, ft4_best_word in the Python package; -1 if none).  ft4BestSet / ft4_best_set are unchanged.
 *   Out of scope: rvec descrambling, a-priori passes (a fetch of their own: FT4 a-priori decoding below), unpacking to text, de-duplication, extending cwslg_fetch_slot.
 * cwslg_enable_ft4_osd(ctx, 1, order 0..2, min_nsync 0..17, min_nqual 0..33) returns CWSLG_ERR_ARG unless a code of rank 83 is loaded and the
 * arguments are in range (17 and 33 mean "nothing is attempted", as for cwslg_enable_ft4_decode); switching it off is always allowed.  It takes
 * effect only at a boundary where the coherent stage, FT4 soft bits and the FT4 decode are all on: then one launch follows the decode launch on
 * the same stream, the candidate and record counts read on the device.  That launch is counted in stats.sync_launches (a boundary with FT4
 * channels alone then counts three).  cwslg_fetch_ft4_osd behaves like cwslg_fetch_ft4_decode: same ticket, the same walk over the records,
 * record q belongs to entry q of cwslg_fetch_ft4_sync, *n = min(record count, max), CWSLG_ERR_MODE for a channel that is not FT4,
 * CWSLG_ERR_NO_FRAME unless OSD, decode, soft and sync records, list and frame are of one epoch -- after a boundary that ran with OSD, the
 * decode, the soft bits or the coherent stage off there is nothing to fetch, never an older slot's records under a newer epoch. */
typedef struct { cwslg_osd_msg set[3]; } cwslg_ft4_osd;          /* 72 bytes */
int cwslg_enable_ft4_osd(cwslg_ctx *ctx, int enable, int order, int min_nsync, int min_nqual);
int cwslg_fetch_ft4_osd(cwslg_ctx *ctx, int ch_id, cwslg_ft4_osd *dst, int max, int *n, uint64_t *start_epoch);
/* The decodes of a slot: the words of a whole FT8 or FT4 slot-clock group in ONE fetch, chosen (BP before OSD; FT4: the set ft4BestWord takes)
 * and de-duplicated per channel on the device.  Without it a consumer calls cwslg_fetch_candidates, cwslg_fetch_ft8_decode and cwslg_fetch_ft8_osd
 * for every channel (three tickets and stream synchronisations each), copies 64 bytes per list entry although a handful of entries per channel
 * carry a word, and picks and de-duplicates on the host.  A FETCH, not a stage: no record kind, no stamp, no launch at a boundary; the kernel
 * (decode_harvest_kernel: count, scan, emit) runs inside the call, on the fetch stream.
 *   1. group is CWSLG_GROUP_FT8 or CWSLG_GROUP_FT4, anything else CWSLG_ERR_ARG; so is a null ctx, start_epoch, n or n_total, or dst null with
 *      max > 0.  n_channels may be null.
 *   2. A channel takes part only if it is open, belongs to the group, has that chain's sync stage (an FT8 / FT4 channel: a JS8 channel of the FT8
 *      group does not take part) and the rule that governs cwslg_fetch_ft8_decode / cwslg_fetch_ft4_decode gives it an epoch E_ch != 0 -- decode
 *      records, soft records, list and frame of one epoch.  The slot epoch is E = *start_epoch; *start_epoch == 0 means the largest E_ch among such
 *      channels.  The channels that take part are those with E_ch == E.  None: CWSLG_ERR_NO_FRAME, all counts 0, *start_epoch untouched.
 *      Otherwise *start_epoch = E.
 *   3. A taking-part channel's OSD records are used only if the rule of cwslg_fetch_ft8_osd / cwslg_fetch_ft4_osd also gives them epoch E.
 *   4. The entries are all min(count, max_cand) entries of the list; FT4: the sync records in the order cwslg_fetch_ft4_sync compacts them.
 *      The word of an entry -- FT8: the decode record's if its crc_ok is set; otherwise, if OSD is used and the OSD record's crc_ok is set, the OSD
 *      record's.  FT4: the smallest set with BP crc_ok; failing that, if OSD is used, the smallest set with OSD crc_ok.  An entry without a word
 *      contributes nothing, and neither does a word whose 91 bits are all zero (its CRC is 0, so it would otherwise pass).
 *   5. Per channel, entries with equal bits[12] are ONE decode: the entry reported is the smallest by (by_osd, nharderr, entry); ndup counts all
 *      entries that carried the word.  Words are never compared across channels.
 *   6. Order: ascending ch_id, then ascending entry.  *n_total counts every decode; *n = min(*n_total, max) and the first *n are written;
 *      *n_channels = channels that took part.  Two calls on the same epoch return the same bytes.
 *   7. The call takes one ticket of the group and runs on a fetch stream behind the group's generation event, like every fetch: the group's next
 *      boundary waits for it.  Concurrent calls on one group are serialised by the library.  It is not counted in stats.sync_launches, adds no
 *      field to cwslg_stats, and never changes records, lists or stamps.  Its device and pinned staging blocks are allocated at the group's first
 *      call (a context that never calls it holds no byte of them) and freed by cwslg_destroy.
 * Out of scope: rvec descrambling, unpacking the 77 bits into text, comparing words across channels or slots. */
typedef struct {
    int32_t  ch_id;
    int16_t  entry;      /* FT8: index into the candidate list; FT4: index of the sync record as cwslg_fetch_ft4_sync compacts them */
    uint8_t  by_osd;     /* 0: word of the decode record (BP); 1: word of the OSD record; 2 (cwslg_fetch_ft8_ap, cwslg_fetch_ft4_ap only): word of the AP record */
    uint8_t  set;        /* FT4: metric set 0..2 the word came from; FT8: 0.  by_osd 2: FT8 the pattern index p; FT4 s | p << 2 (set & 3 the metric set, set >> 2 the pattern) */
    uint8_t  bits[12];   /* as cwslg_ft8_msg.bits */
    float    freq_hz;    /* FT8: candidate freq_hz; FT4: record f1_hz */
    float    dt_s;       /* FT8: candidate dt_s; FT4: record dt_s */
    float    sync;       /* FT8: candidate sync; FT4: record sync */
    float    dmin;       /* by_osd: the OSD record's dmin; else +0 */
    int16_t  nharderr;   /* of the record the word came from */
    uint16_t ndup;       /* entries of this channel that carried this word, this one included; saturates at 65535 */
} cwslg_decode;          /* 40 bytes */
int cwslg_fetch_decodes(cwslg_ctx *ctx, int group, uint64_t *start_epoch /* in/out */, cwslg_decode *dst, int max, int *n, int *n_total,
                        int *n_channels);
/* FT8 signal reports (row a13; PARITY UNPINNED like the rest of the stage): per decode of cwslg_fetch_decodes an SNR figure and a tone check,
 * made on the device from what is already there -- the channel's symbol-spectra plane (written by the boundary that made the list), the
 * candidate's grid position and the loaded code.  A spot needs a report (cwslg_spot.snr_db); without this call a consumer of the device chain
 * pulls each channel's 1.45 MB plane back and redoes the arithmetic on the host.  Structured like upstream ft8b's xsig / xnoi report, recalled and
 * not copied, on the plane's own grid.  A FETCH like cwslg_fetch_decodes, not a stage: no record kind, no stamp, no launch at a boundary, no
 * field in cwslg_stats, stats.sync_launches untouched.  tests/decode_reports_ref.py restates everything below in numpy.  Every operation is one
 * un-fused float32 operation unless stated otherwise.
 *   Re-encoder: cwslg_set_ldpc_code reduces H taking pivots in columns 91..173.  If those 83 columns are invertible the code is SYSTEMATIC:
 *       the codeword of a 91-bit word is the word followed by the 83 parity bits H demands.  If they are not, the table is still loaded and
 *       decodes as before; cwslg_fetch_decode_reports and cwslg_ft8_tones then return CWSLG_ERR_ARG with a text that says so.
 *   Tones t[0..78] of a word: symbols 0..6, 36..42 and 72..78 are the Costas array 3,1,4,0,6,5,2; data symbol d (0..57) sits at n = d + 7
 *       (d < 29) or d + 14 and its tone is graymap[4 cw[3d] + 2 cw[3d+1] + cw[3d+2]], graymap = 0,1,3,2,5,6,4,7 -- the inverse of what the soft
 *       bits read.  cwslg_ft8_tones(ctx, bits[12], tones[79]) is this on its own, host work only, under the code in force.
 *   For a decode with candidate (i = freq_bin, j = time_step) -- the list entry cwslg_decode.entry names:
 *     Plane power: P[n][k] = S(i + 2 k, m), m = j + 12 + 4 n (n = 0..78, k = 0..7): the soft bits' addressing; +0 where m < 1, m > 372, the bin
 *       is above 1920 or the bin is beyond the row.
 *     Magnitude: s8 = sqrtf(P), correctly rounded.
 *     nsync: of the 21 Costas symbols, the number whose FIRST maximum of s8 over k = 0..7 (ties to the lowest k) is at t[n].  By construction
 *       this equals the entry's cwslg_ft8_soft.nsync.
 *     nsymerr: of the 58 data symbols, the number whose first maximum of s8 is NOT at t[n]; 0..58.
 *     xsig = sum of P[n][t[n]], xnoise = sum of P[n][(t[n] + 4) mod 7], both over n = 0..78 in the order a 64-lane wave evaluates them: lane l
 *       holds term l, plus term l + 64 where that is below 79, added in that order (a[l] = term[l] + term[l + 64] for l < 15, term[l] otherwise);
 *       then six halving steps a[l] = a[l] + a[l + h] for l < h, h = 32, 16, 8, 4, 2, 1; the result is a[0].
 *     snr_db: r = xnoise > 0 ? xsig / xnoise - 1.0f : 0.0f;  x = r > 0.1f ? r : 0.001f;  x = min(x, FLT_MAX) (an infinite ratio, which no
 *       logarithm is defined for, reports as the largest float's);  snr_db = max((float)(10.0 L((double)x) - 27.0), -24.0f), L the library's fixed
 *       double-precision log10 (oracle/sync_oracle.c: orc_log10_fixed), so the bits are the same on every machine.  Upstream's baseline-referred
 *       xsnr2 is not made.  How far this figure lies from an SNR in 2500 Hz is a measured property, not part of the contract.
 * cwslg_fetch_decode_reports is cwslg_fetch_decodes' contract, points 1 to 7 above, with these differences: group must be CWSLG_GROUP_FT8 (FT4
 * and every other group: CWSLG_ERR_ARG -- the FT4 chain keeps no symbol-aligned plane; its reports are cwslg_fetch_ft4_decode_reports below); dec receives byte-identical records to what
 * cwslg_fetch_decodes returns for that epoch and max; rep[p] is the report of dec[p]; either output pointer may be null (nothing is written
 * through it; the counts are the same).  Execution, one ticket and one serialised call of the group: the descriptors go up, the three harvest
 * launches run, ONE further launch (decode_report_kernel, one wave per record) runs over the min(n_total, max) emitted records, ONE
 * copy brings head, decodes and reports down, one synchronise.  The staging blocks are the group's, shared with cwslg_fetch_decodes and grown
 * in the same way; the encoder's 2184-byte device copy is made by the first report call after a (re)load of the code: a context that never asks
 * for reports holds no device byte of it.  It writes no record, list, stamp or statistic.
 * The report uses the code IN FORCE AT THE CALL: words decoded under an earlier table are re-encoded under the new one (their first 91 bits are
 * kept; parity, tones and therefore the figures are the new code's).
 * Out of scope: unpacking to text, xsnr2, a second search pass over the residual frame (the subtraction itself is cwslg_subtract_ft8 below;
 * FT4 reports: the next block). */
typedef struct {
    float   snr_db;      /* see above; never below -24 (FT4: -21) */
    float   xsig;        /* power at the re-encoded tones */
    float   xnoise;      /* power at the tones (t + 4) mod 7 (FT4: (t + 2) & 3) */
    int16_t nsync;       /* Costas symbols whose strongest tone is the Costas tone, 0..21 (FT4: 0..16) */
    int16_t nsymerr;     /* data symbols whose strongest tone is not the re-encoded one, 0..58 (FT4: 0..87) */
} cwslg_decode_report;   /* 16 bytes */
int cwslg_fetch_decode_reports(cwslg_ctx *ctx, int group, uint64_t *start_epoch /* in/out */, cwslg_decode *dec, cwslg_decode_report *rep, int max,
                               int *n, int *n_total, int *n_channels);
int cwslg_ft8_tones(cwslg_ctx *ctx, const uint8_t *bits /* [12] */, uint8_t *tones /* [79] */);
/* FT4 signal reports (row a13; PARITY UNPINNED like the rest of the stage): the same 16-byte cwslg_decode_report beside every decode of
 * cwslg_fetch_decodes(CWSLG_GROUP_FT4), made on the device from what is there when the fetch is made -- the channel's frame spectrum (written by
 * the boundary that made the records), the sync record's refined frequency and start, and the loaded code.  Without this call a consumer pulls
 * the channel's 290 KB frame spectrum back and redoes the downsample and 412 symbol transforms per decode on the host.  A FETCH, not a stage:
 * no record kind, no stamp, no launch at a boundary, no field in cwslg_stats, stats.sync_launches untouched.  tests/ft4_decode_reports_ref.py
 * restates everything below in numpy.  Every operation is one un-fused float32 operation unless written as fmaf.
 *   Tones t[0..102] of a word: the codeword is the FT8 report's systematic re-encoding of the 91 bits (above; the same errors for a table whose
 *       columns 91..173 are singular).  No rvec: descrambling stays with the consumer, as everywhere in the FT4 chain.  Symbols 0..3, 33..36,
 *       66..69 and 99..102 carry the Costas blocks 0132, 1023, 2310, 3201; data symbol d (0..86) sits at n = d + 4 (d < 29), d + 8 (d < 58) or
 *       d + 12 and its tone is graymap[2 cw[2d] + cw[2d+1]], graymap = 0,1,3,2 -- the inverse of what the soft bits read.
 *       cwslg_ft4_tones(ctx, bits[12], tones[103]) is this on its own, host work only, under the code in force.
 *   For a decode whose entry names the sync record (f1_hz, ibest) -- cwslg_fetch_ft4_sync's compacted order:
 *     Spectra: the baseband is the soft bits' (orc_ft4_downsample at f1_hz); cs[n][q] (n = 0..102, q = 0..3) is cwslg_ft4_soft's 32-term fmaf
 *       chain over the samples ibest + 32 n .. + 31, +0 outside 0..4031: the SAME bits as the soft-bit stage computes (one device text).
 *     Power: P[n][q] = fmaf(re, re, im * im).  Magnitude: sqrtf(P), correctly rounded.
 *     nsync: of the 16 Costas symbols, the number whose FIRST maximum of the magnitude over q = 0..3 (ties to the lowest q) is t[n]; 0..16.  By
 *       construction this equals the record's cwslg_ft4_soft.nsync.  On an all-zero baseband it is 4: tone 0 wins every tie and each Costas
 *       block contains one 0.
 *     nsymerr: of the 87 data symbols, the number whose first maximum is NOT t[n]; 0..87.
 *     xsig = sum of P[n][t[n]], xnoise = sum of P[n][(t[n] + 2) & 3] (the tone two bins away is orthogonal over the 32-sample symbol), both over
 *       n = 0..102 in the order a 64-lane wave evaluates them: a[l] = term[l] + term[l + 64] for l < 39, term[l] otherwise; then six halving
 *       steps a[l] = a[l] + a[l + h] for l < h, h = 32, 16, 8, 4, 2, 1; the result is a[0].
 *     snr_db: r = xnoise > 0 ? xsig / xnoise - 1.0f : 0.0f;  x = r > 0.1f ? r : 0.001f;  x = min(x, FLT_MAX);
 *       snr_db = max((float)(10.0 L((double)x) - 20.8), -21.0f), L the fixed log10 of the FT8 report.  20.8 is 10 log10(2500 / 20.8333), the
 *       ratio of the reference bandwidth to a tone bin's noise bandwidth; it contains no fitted term.  -21 is the floor FT4 reports
 *       conventionally have; it is reached at r = 0.955, so the 0.1 / 0.001 branch never shows in snr_db.  A NaN xsig or xnoise fails both
 *       comparisons and reports -21: the logarithm never sees NaN or infinity.  How far the figure lies from an SNR in 2500 Hz is a measured
 *       property, not part of the contract.
 * cwslg_fetch_ft4_decode_reports is cwslg_fetch_decodes' contract for CWSLG_GROUP_FT4, points 1 to 7 above, with these additions: dec receives
 * byte-identical records to what cwslg_fetch_decodes returns for that epoch and max; rep[p] is the report of dec[p] (nsync 0..16, nsymerr 0..87);
 * either output pointer may be null.  Execution, one ticket and one serialised call of the group: the descriptors go up (a second per-channel
 * descriptor with the spectrum, the sync records, nrec and the capacity rides in the same copy), the three harvest launches run, ONE further
 * launch (ft4_report_kernel, one 256-thread workgroup per record, the grid sized by max) runs over the
 * min(n_total, max) emitted records, ONE copy brings head, decodes and reports down, one synchronise.  Staging and the encoder's device copy are
 * as for the FT8 call; the code IN FORCE AT THE CALL is used.  A channel takes part only if its decode records are of the frame's epoch, which
 * implies that the last boundary ran the coherent stage on it: the spectrum read is that frame's.
 * Out of scope: unpacking to text, rvec, a baseline-referred SNR, any second pass over a residual (a-priori passes and the subtraction are
 * fetches of their own: cwslg_fetch_ft4_ap, cwslg_subtract_ft4 below; the second pass stays out there too). */
int cwslg_fetch_ft4_decode_reports(cwslg_ctx *ctx, uint64_t *start_epoch /* in/out */, cwslg_decode *dec, cwslg_decode_report *rep, int max,
                                   int *n, int *n_total, int *n_channels);
int cwslg_ft4_tones(cwslg_ctx *ctx, const uint8_t *bits /* [12] */, uint8_t *tones /* [103] */);
/* FT8 a-priori decoding (PARITY UNPINNED like the rest of the chain): the candidates that belief propagation and OSD gave up on, decoded again
 * with some of the 91 message bits TOLD to the decoder.  Nearly every transmission a skimmer wants to spot begins with a known field; telling the
 * decoder those bits buys sensitivity on exactly those messages (measured against this chain's own BP + OSD: DESIGN.md 4.12).  Everything it
 * needs is on the device after a boundary -- the alternative is 704 bytes per failed candidate over the link and BP on the host.  A FETCH with a
 * kernel inside, not a stage: no record kind, no stamp, no launch at a boundary, no field in cwslg_stats, stats.sync_launches untouched.
 * tests/ap_ref.py restates everything below in numpy.
 *   Patterns are DATA THE CALLER LOADS, as the parity-check table is: nothing here knows what "CQ" packs to.  A pattern is a mask and a value over
 *       codeword bits 0..90, both packed as cwslg_ft8_msg.bits.  cwslg_set_ft8_ap(ctx, pat, n_pat 0..8 (0 clears the patterns), max_iter 1..200,
 *       min_nsync 0..22) returns CWSLG_ERR_ARG for an argument out of range, a mask or value bit at position 91..95, or a value bit outside its
 *       mask; the patterns in force then stay.  A mask with no bit set is allowed: it is a second plain BP pass.  The call has host effect only and
 *       may be repeated at any time; every AP call takes the patterns (and the code) IN FORCE AT THE CALL up with its own upload.
 *   Arithmetic per metric set llr[174]; every operation is ONE un-fused float32 operation.
 *     1. If any llr[t] is not finite the set is NOT ATTEMPTED.
 *     2. A = 1.01f * max_t |llr[t]| (the max is exact, the product one multiply).
 *     3. For p = 0, 1, ... in the caller's order: llr_p[t] = (value_p[t] ? +A : -A) where mask_p[t] is set, llr[t] elsewhere.
 *     4. The decode contract's loop (steps 1 to 8 of cwslg_ft8_msg, the same T, A(y) and early stop) runs on llr_p with max_iter, from messages +0.
 *     5. Pattern p SUCCEEDS iff at exit nbad == 0, the CRC-14 rule holds, and cw[t] == value_p[t] on every masked t -- a word that contradicts
 *        the hypothesis it was found under is not a find.
 *     6. The first p that succeeds ends the set.
 *   Record on success: bits and iters of that run, nbad = 0, crc_ok = 1, pad_ = p; nharderr = #{t < 174 : (llr[t] > 0) != cw[t]} and dmin = OSD's
 *       distance (rule 7 of cwslg_osd_msg: the ascending-t chain from +0 over |llr[t]| of the disagreeing t), both against the ORIGINAL metrics:
 *       dmin is the gate upstream applies to AP decodes.  Without success: zero bits, iters = the SUM of all runs' iteration counts, nbad = the
 *       last run's, nharderr = -1, crc_ok = 0, pad_ = 0xff, dmin = +0.  Not attempted: the decode record's "not attempted" bytes, pad_ = 0xff,
 *       dmin = +0.
 * cwslg_ap_decode runs the kernel on n >= 0 caller-supplied sets (host memory) with no nsync gate, synchronously: the twin of cwslg_ldpc_decode
 * and cwslg_osd_decode.  CWSLG_ERR_ARG without a loaded code or with no pattern set.
 * cwslg_fetch_ft8_ap is cwslg_fetch_decodes' contract for CWSLG_GROUP_FT8, points 1 to 7 above, with these differences.  Which channels take
 * part, and whether a channel's OSD records are used, is decided exactly as there (points 2 and 3).  Entry q of a channel is ATTEMPTED iff its
 * decode record was attempted (iters >= 0) and has crc_ok == 0; the OSD records are not used, or its OSD record has crc_ok == 0; its soft record
 * has nsync >= min_nsync; and rule 1 holds.  An entry's word is its AP record's, if crc_ok; the all-zero word is dropped; equal words of one
 * channel fold into one cwslg_decode ranked by (nharderr, entry), with ndup; the order is ch_id, then entry -- the harvest kernel's existing
 * modes, run on the AP records.  Each emitted record has by_osd = 2, set = the pattern index and dmin = the AP record's.  Words that another
 * entry of the channel already decoded by BP or OSD are NOT removed here: merge on the host by bits[12] per ch_id, BP / OSD winning
 * (mergeApDecodes in cwsl_gpu_shim.hpp, merge_ap_decodes in api.py).  CWSLG_ERR_ARG with no pattern set or no code loaded.  Execution, one
 * ticket and one serialised call of the group: descriptors, pattern block and tables go up in one copy, the a-priori decode runs (ap_decode_kernel: one wave
 * per candidate, the count read on the device), the three harvest launches run on its records, ONE further launch (ap_annotate_kernel)
 * annotates the emitted records, ONE copy down, one synchronise.  Staging: per taking-part channel max_cand x (20 + 4) bytes; it belongs to the
 * group, is allocated at the first call, grows, and is freed by cwslg_destroy: a context that never calls holds no byte of it.
 * Out of scope: AP words inside cwslg_fetch_decodes itself, packing call signs into patterns, unpacking to text, a second pass over the residual frame (the subtraction: cwslg_subtract_ft8), OSD
 * on AP-modified metrics. */
typedef struct { uint8_t mask[12]; uint8_t value[12]; } cwslg_ap_pattern;   /* codeword bits 0..90, packed as cwslg_ft8_msg.bits */
typedef struct { cwslg_ft8_msg msg; float dmin; } cwslg_ap_msg;             /* 24 bytes; msg.pad_ = pattern index, 0xff: none */
int cwslg_set_ft8_ap(cwslg_ctx *ctx, const cwslg_ap_pattern *pat, int n_pat, int max_iter, int min_nsync);
int cwslg_fetch_ft8_ap(cwslg_ctx *ctx, uint64_t *start_epoch /* in/out */, cwslg_decode *dst, int max, int *n, int *n_total, int *n_channels);
int cwslg_ap_decode(cwslg_ctx *ctx, const float *llr /* [n][174] */, int n, cwslg_ap_msg *out);
/* FT4 a-priori decoding (PARITY UNPINNED like the rest of the chain): the FT4 sync records that belief propagation and OSD gave up on, decoded
 * again under known-bit patterns -- the FT8 block above on the FT4 chain's three-set records.  Everything it needs is on the device after an FT4
 * boundary; the alternative is 2112 bytes of metrics per failed record over the link and BP on the host.  A FETCH with a kernel inside, not a
 * stage: no record kind, no stamp, no launch at a boundary, no field in cwslg_stats, stats.sync_launches untouched.  tests/ft4_ap_ref.py restates
 * everything below in numpy, on tests/ap_ref.py.
 *   Setter: cwslg_set_ft4_ap(ctx, pat, n_pat 0..8 (0 clears the patterns), max_iter 1..200, min_nsync 0..17, min_nqual 0..33) -- the ranges of
 *       cwslg_enable_ft4_decode; 17 and 33 mean nothing is attempted.  The FT4 patterns are a state OF THEIR OWN beside the FT8 ones: on the air
 *       FT4's 77 message bits are rvec-scrambled, so a caller's FT4 patterns hold the SCRAMBLED values and differ from their FT8 patterns.  No rvec
 *       is applied anywhere in the library.  Validation is cwslg_set_ft8_ap's: CWSLG_ERR_ARG for an argument out of range, a bit at positions
 *       91..95 or a value bit outside its mask; the patterns in force then stay.  Host effect only.
 *   Gate, PER RECORD (for the reason the FT4 OSD gate gives: a consumer takes one word per record, and a record BP or OSD decoded in any set
 *       has it).  A record is a sync record in the slot array: slot = 3 cand + r, r < nrec[cand].  It is TAKEN iff (1) no set of its
 *       cwslg_ft4_msg has BP crc_ok; (2) if the channel's OSD records are used (point 3 of cwslg_fetch_decodes), no set of its cwslg_ft4_osd has
 *       crc_ok; (3) its soft record has nsync >= min_nsync and nqual >= min_nqual.  Set s of a taken record is ATTEMPTED iff set[s].iters >= 0 in
 *       the decode record (which covers sigma[s] == 0) and all 174 metrics llr[s][t] are finite.
 *   Arithmetic: each attempted set follows rules 1 to 6 and the record rules of cwslg_ap_msg above on llr[s][0..173], unchanged.  The three sets of
 *       a record run side by side, each to its own exit, as in the FT4 decode: no traffic between them, no early stop across them.  A set that is
 *       not attempted gets the "not attempted" record.
 *   Choice: a record's word is that of the SMALLEST s whose AP record has crc_ok.  The choice is SET-MAJOR: a find in set 0 under pattern 3 beats
 *       a find in set 1 under pattern 0.  This is the library's own order; it has not been compared with upstream's.
 * cwslg_fetch_ft4_ap is cwslg_fetch_decodes' contract for CWSLG_GROUP_FT4, points 1 to 7 above.  The harvest kernel's existing FT4 modes run
 * unchanged on the AP records: entries in the order cwslg_fetch_ft4_sync compacts them, the all-zero word dropped, equal words of a channel
 * folded by (nharderr, entry) with ndup, order ch_id then entry.  Every emitted record has by_osd = 2, set = s | p << 2 (s the metric set, p the
 * pattern index: set & 3 and set >> 2) and dmin = that AP record's.  Words that BP or OSD already found on another entry are NOT removed: merge
 * on the host as for FT8 (mergeApDecodes / merge_ap_decodes merge by (ch_id, bits) and serve unchanged).  CWSLG_ERR_ARG with no FT4 pattern set
 * or no code loaded; CWSLG_ERR_NO_FRAME as for cwslg_fetch_decodes.  The call uses the patterns and tables IN FORCE AT THE CALL and takes them up
 * in its own upload.  Execution: the FT8 call's, with one wave per (record slot, metric set) in the a-priori launch -- grid (ceil(9 max_cand / 4),
 * taking-part channels), the FT4 decode's own exits -- and staging of 3 max_cand x (60 + 12) bytes per taking-part channel in the FT4 group's
 * stage.  cwslg_ap_decode stays the flat twin under the FT8 patterns: the per-set arithmetic is the same kernel text.
 * Out of scope: AP words inside cwslg_fetch_decodes itself, packing call signs into patterns, rvec, unpacking to text, OSD on AP-modified metrics,
 * an early stop across the three sets of a record. */
int cwslg_set_ft4_ap(cwslg_ctx *ctx, const cwslg_ap_pattern *pat, int n_pat, int max_iter, int min_nsync, int min_nqual);
int cwslg_fetch_ft4_ap(cwslg_ctx *ctx, uint64_t *start_epoch /* in/out */, cwslg_decode *dst, int max, int *n, int *n_total, int *n_channels);
/* FT8 signal subtraction (PARITY UNPINNED like the rest of the chain): per decode of cwslg_fetch_decodes a refined frequency and start, fitted with
 * the KNOWN word as the sync pattern (79 known symbols instead of 21 Costas symbols), and per channel a RESIDUAL frame: the float frame minus the
 * fitted waveform of every emitted decode.  Everything it needs is on the device when the decodes are harvested -- the float frame, the
 * re-encoder of the reports, the emitted records; without it a consumer pulls 720 KB per channel to the host and synthesises and fits there.
 * Shaped like upstream's subtractft8 (reference waveform, complex amplitude low-passed, subtract), recalled and not copied, on grids of its own.
 * A FETCH, not a stage: no record kind, no stamp, no launch at a boundary, no field in cwslg_stats, stats.sync_launches untouched; it never
 * writes the frame, the plane, a list or a record.  tests/ft8_subtract_ref.py restates everything below in numpy, bit for bit.  Every float
 * operation is one un-fused float32 operation in the order written; phases are uint32 arithmetic modulo 2^32, in units of 2^-32 turns.
 *   Tables (cwsl_digi_amd/csrc/modules/ft8sub_tables.inc, written by scripts/gen_ft8sub_tables.py): CP[3][1920], CPT[3], COSQ[1025], WIN[97].
 *   Waveform of (tones t[0..78] -- the reports' re-encoder --, increment inc): GFSK, BT = 2.0, unit amplitude, 79 x 1920 samples at 12 kHz.  Sample v
 *       of symbol n has phase  base[n] + v inc + tp CP[2][v] + tc CP[1][v] + tn CP[0][v],  tp / tc / tn the tones of symbols n - 1 / n / n + 1
 *       (n - 1 and n + 1 clamped to 0..78: the first and last tone are held outside the transmission); base[0] = 0, base[n + 1] = base[n] +
 *       1920 inc + tp CPT[2] + tc CPT[1] + tn CPT[0].  CP[x][v] is the exclusive prefix of the per-sample integer increments of one tone unit
 *       (6.25 Hz) of the pulse's third x, so the phase is the prefix of the increments  inc + tp P[2][v] + tc P[1][v] + tn P[0][v].
 *       (cos, sin) = CS[(phase + 2^19) >> 20], CS[i] = (cos, sin)(2 pi i / 4096) made from the quarter-turn table by symmetry: cos is COSQ[r],
 *       -COSQ[1024 - r], -COSQ[r], COSQ[1024 - r] in the four quarters (r = i mod 1024), sin(i) = cos(i - 1024).  No sinf / cosf anywhere.
 *   Start: i0 = (int)clamp(rintf(dt_s * 12000.0f), -400000, 400000) + 6000 - 480; inc0 = (uint32)llrint((double)freq_hz * 2^32 / 12000).  The 480:
 *       a candidate's dt_s is (time_step - 0.5) 0.04 s, while the window of plane step time_step + 12, where the search finds symbol 0, starts
 *       0.04 time_step - 0.06 s after the protocol's 0.5 s: the signal's first sample lies one plane step BEFORE what dt_s names, and the time
 *       search, half a step to either side, is centred there.  The report's dt_s is the signal's own start, so it is about 0.04 s below dec's.
 *   Block sums of a start s and an increment: the signal's 151680 samples in 2528 blocks of 60 (32 per symbol); B[b] = (re, im), re = re + x c and
 *       im = im - x s over the block's samples in ascending order from +0, x the frame sample (frame * conj(wave)); a sample before sample 0 or
 *       past 179999 (or past the frame's n_valid: the zero tail) is +0, which leaves the sums as skipping it would.
 *   Symbol metric of block sums: S[n] = the symbol's 32 block sums halved (a[l] = a[l] + a[l + h] for l < h, h = 16, 8, 4, 2, 1), per component;
 *       M = sum over n = 0..78 ascending, from +0, of (S.re S.re + S.im S.im).
 *   FIT, from the ORIGINAL frame for every decode (no decode sees another's subtraction; deterministic and parallel):
 *     1. frequency, at block rate: B at (i0, inc0); for k = -52..52: B'[b] = (re cr + im sr, im cr - re sr), (cr, sr) = CS of the phase
 *        (uint32)(k 11185) * (60 b + 30); the FIRST maximum of M over ascending k wins; inc = inc0 + k 11185.  The grid is 0.0312505 Hz wide
 *        (11185 * 12000 / 2^32) and reaches +-1.62503 Hz: more than half a 3.125 Hz search bin.
 *     2. time, at sample rate and at the refined frequency: for j = 0..60: M of the block sums at (i0 - 240 + 8 j, inc); the FIRST maximum over
 *        ascending j wins; start = i0 - 240 + 8 j.  The grid is 8 samples (2/3 ms) wide and reaches +-240 samples: half a 40 ms plane step.
 *     3. frequency once more, now that the symbols are aligned: step 1 on B at (start, inc), inc = inc + k2 11185 (df_steps = k + k2).
 *        B at (start, inc); cnt[b] = samples of block b inside 0..179999.
 *     4. amplitude track: a[b] = (sum_j WIN[j] B[b - 48 + j].re / den, the same of .im), den = sum_j WIN[j] (float)cnt[b - 48 + j], j = 0..96
 *        ascending from +0, blocks outside 0..2527 contributing +0 -- a Hann window three symbols wide, normalised by the samples actually under
 *        it, so the edges of the signal and of the frame are not pulled down; den > 0 else a[b] = +0.
 *     5. figures, each summed as: thread l of 256 adds the terms of blocks l, l + 256, .. ascending from +0; then a[l] = a[l] + a[l + h] for l < h,
 *        h = 128 .. 1.  p_removed: 2 (a.re a.re + a.im a.im) cnt (the energy of the fitted waveform, A cos carrying 2 |a|^2 per sample);
 *        p_before: cnt > 0 ? 2 (B.re B.re + B.im B.im) / cnt : 0 -- the frame's energy along the signal's de-chirped track, 200 Hz wide around
 *        the tone: its time-frequency footprint; p_after: the same of B - cnt a (this decode's own fit taken out, at block rate).
 *   APPLY: residual[t] = frame[t] - sum over the channel's emitted decodes IN EMISSION ORDER of 2 y_d[t], i.e. r = r - 2.0f * y one decode after
 *       the other in a register, no atomics; y = ar c - ai s at signal sample u = t - start (0 <= u < 151680, t inside the frame), (ar, ai) the
 *       track between block centres: pp = 2 u - 59; pp < 0: a[0]; b0 = min(pp / 120, 2526), m = pp - 120 b0; m >= 120: a[2527]; otherwise
 *       a[b0] + ((float)m * (1.0f / 120.0f)) * (a[b0 + 1] - a[b0]).
 * 1. cwslg_subtract_ft8 is cwslg_fetch_decode_reports' contract for the FT8 group (points 1 to 7 of cwslg_fetch_decodes, one ticket, one
 *    serialised call, the fetch stream, the group's staging blocks, a systematic code or CWSLG_ERR_ARG; dec byte-identical to cwslg_fetch_decodes
 *    for that epoch and max; either output pointer may be null), with sub[p] the cwslg_subtract_report of dec[p].  The frame is the decoder's:
 *    the first 180000 samples (15 s) of the channel's float frame, whose device buffer is the reference's 20 s.  Per channel that took part it
 *    leaves the residual over the first min(n_total, max) records in a device block of the group, allocated by the first call, grown on demand,
 *    freed by cwslg_destroy; a channel without an emitted decode -- and every channel at max = 0 -- gets the frame's own bits.  Two calls on one
 *    epoch leave the same bytes.  Execution: descriptors up, the three harvest launches, the 16-byte head down and one synchronise (the fit
 *    records, 20736 bytes each, are sized by what was emitted), ft8_sub_fit_kernel (one workgroup per emitted decode), ft8_sub_apply_kernel (one
 *    workgroup per channel and 1024-sample tile), one copy down, one synchronise.  The kernels are in a code object of their own beside the
 *    library (cwslgpu_ft8sub.hsaco), loaded by the first call; a missing file is CWSLG_ERR_ARG with a text that names it.
 *    The call has no group argument: it is the FT8 group's.  FT4 channels never take part, and a context with FT4 channels alone answers
 *    CWSLG_ERR_NO_FRAME like any call no channel takes part in; the FT4 group has a call of its own, cwslg_subtract_ft4 below.
 *    The call holds the group's ticket for as long as it runs -- about 10 ms for 800 decodes against 0.2 ms for the report call -- and the
 *    group's next boundary waits for the ticket with the context locked: a boundary that arrives during the call delays every push on the
 *    context by the rest of it.  Call it right after the boundary, not just before the next one.
 * 2. cwslg_fetch_ft8_residual copies a channel's residual (180000 floats, the units of cwslg_fetch_audio_f32; cap below that: CWSLG_ERR_ARG) and
 *    cwslg_ft8_residual_device_ptr hands out its device address; both only while the residual's epoch is the channel's frame epoch, otherwise
 *    CWSLG_ERR_NO_FRAME: never an older slot's residual under a newer epoch.  The next cwslg_subtract_ft8 overwrites the block, and FREES it
 *    when more channels take part than it was sized for: an address handed out is dead from the next cwslg_subtract_ft8 call on.
 * 3. cwslg_ft8_subtract_flat runs the same two kernels on caller-supplied frames (n_frames x 180000 floats) and items, the cwslg_ldpc_decode
 *    pattern (synchronous, temporary device buffers, the context's stream): items in ascending frame order (else CWSLG_ERR_ARG), freq_hz in
 *    0..6000 and |dt_s| <= 30, dt_s in the candidate's convention (a transmission that starts at T has dt_s = T + 0.04); sub[i] reports items[i]; residual, [n_frames][180000], may be null.  n_items = 0 gives residual = audio.
 *    The increment is uint32 throughout: where the searches step it below 0 (freq_hz = 0 and k + k2 < 0) it wraps, and f_hz reports the wrapped
 *    increment by the formula above, a value just under 12000 (11999.75 at k + k2 = -8), not a negative frequency.
 * Out of scope: a second search or decode pass over the residual, an int16 or prepareAudio-scaled residual, joint refitting of overlapping
 * signals, unpacking to text.  (FT4: the section below.) */
typedef struct {
    float   f_hz;        /* refined frequency of tone 0: inc * 12000 / 2^32 in double, rounded to float */
    float   dt_s;        /* refined start: (float)(start - 6000) / 12000.0f */
    float   p_removed;   /* energy of the fitted waveform, in squared units of cwslg_fetch_audio_f32 */
    float   p_before;    /* the frame's energy in the signal's time-frequency footprint */
    float   p_after;     /* the same with this decode's fit taken out */
    int32_t n_inside;    /* samples of the 79 x 1920 (FT4: 103 x 576) inside the frame */
    int16_t df_steps;    /* k + k2 of the two frequency searches, each -52..52 (FT4: -26..26) */
    int16_t dt_steps;    /* j - 30 of the time grid, -30..30 (FT4: j - 27, -27..27) */
} cwslg_subtract_report;   /* 28 bytes */
typedef struct { int32_t frame; uint8_t bits[12]; float freq_hz; float dt_s; } cwslg_ft8_sub_item;   /* 24 bytes; bits as cwslg_ft8_msg.bits */
#define CWSLG_FT8_FRAME_SAMPLES 180000
int cwslg_subtract_ft8(cwslg_ctx *ctx, uint64_t *start_epoch /* in/out */, cwslg_decode *dec, cwslg_subtract_report *sub, int max, int *n, int *n_total,
                       int *n_channels);
int cwslg_fetch_ft8_residual(cwslg_ctx *ctx, int ch_id, float *dst, size_t cap, size_t *n_valid, uint64_t *start_epoch);
int cwslg_ft8_residual_device_ptr(cwslg_ctx *ctx, int ch_id, const float **d_f32, uint64_t *start_epoch);
int cwslg_ft8_subtract_flat(cwslg_ctx *ctx, const float *audio /* [n_frames][180000] */, int n_frames, const cwslg_ft8_sub_item *items, int n_items,
                            cwslg_subtract_report *sub, float *residual /* [n_frames][180000] or null */);
/* FT4 signal subtraction (PARITY UNPINNED like the rest of the chain): the FT8 block above on the FT4 chain -- per decode of
 * cwslg_fetch_decodes(CWSLG_GROUP_FT4) a refined frequency and start, fitted with the KNOWN word as the sync pattern (103 known symbols instead of
 * 16 Costas symbols), and per channel a RESIDUAL frame: the float frame minus the fitted waveform of every emitted decode.  FT4 signals are four
 * times as wide as FT8's and the mode is the busier one, so a weak signal under a strong one is the common case; without this call a consumer
 * pulls 290 KB per channel to the host and synthesises and fits there.  A FETCH, not a stage: no record kind, no stamp, no launch at a boundary,
 * no field in cwslg_stats, stats.sync_launches untouched; it never writes the frame, a plane, a list or a record.  tests/ft4_subtract_ref.py
 * restates everything below in numpy, bit for bit.  Every float operation is one un-fused float32 operation in the order written; phases are
 * uint32 arithmetic modulo 2^32, in units of 2^-32 turns.
 *   Frame: the decoder's -- the first 72576 samples (CWSLG_FT4_FRAME_SAMPLES) of the channel's float frame; samples at or past the frame's
 *       n_valid count as +0.
 *   Tables (cwsl_digi_amd/csrc/modules/ft4sub_tables.inc, written by scripts/gen_ft4sub_tables.py): CP[3][576], CPT[3], COSQ[1025], WIN[97];
 *       COSQ and WIN are the FT8 tables value for value (both modes have 32 blocks per symbol).
 *   Waveform of (tones t[0..102] -- what cwslg_ft4_tones returns: the reports' re-encoding through the FT4 mapping, no rvec --, increment inc):
 *       GFSK, BT = 1.0, tone unit 12000 / 576 Hz, unit amplitude, 103 x 576 samples at 12 kHz.  Sample v of symbol n has phase
 *       base[n] + v inc + tp CP[2][v] + tc CP[1][v] + tn CP[0][v],  tp / tc / tn the tones of symbols n - 1 / n / n + 1 (clamped to 0..102: the
 *       first and last tone are held outside the transmission; the protocol's two ramp symbols are NOT modelled, the amplitude track absorbs
 *       them); base[0] = 0, base[n + 1] = base[n] + 576 inc + tp CPT[2] + tc CPT[1] + tn CPT[0].  (cos, sin) = CS[(phase + 2^19) >> 20] from
 *       the quarter-turn table by symmetry, exactly as for FT8.  No sinf / cosf anywhere.
 *   Start: i0 = (int)clamp(rintf((dt_s + 0.5f) * 12000.0f), -400000, 400000) - F4SUB_CAND_OFFSET; inc0 = (uint32)llrint((double)f1_hz * 2^32 /
 *       12000).  F4SUB_CAND_OFFSET = 0: a record's dt_s is ibest / 666.67 - 0.5 with ibest the baseband sample (18 frame samples) at which the
 *       first Costas symbol starts, so it names the transmission's first sample itself, to within half a baseband sample.  Established on the
 *       CPU with the float64 synthesiser (tests/ft4_gfsk.py) against the oracle's FT4 search and refinement: over starts on and off the 666.67 Hz
 *       grid the record's dt_s lay -6.1 .. +3.6 samples from the truth, never a whole step to one side.  FT8's 480 has no twin.
 *   Block sums of a start s and an increment: the signal's 59328 samples in 3296 blocks of 18 (32 per symbol, block rate 666.67 Hz); B[b] = (re,
 *       im), re = re + x c and im = im - x s over the block's samples in ascending order from +0; a sample outside 0..72575 is +0.
 *   Symbol metric: S[n] = the symbol's 32 block sums halved (a[l] = a[l] + a[l + h] for l < h, h = 16, 8, 4, 2, 1), per component; M = sum over
 *       n = 0..102 ascending, from +0, of (S.re S.re + S.im S.im).
 *   FIT, from the ORIGINAL frame for every decode:
 *     1. frequency, at block rate: B at (i0, inc0); for k = -26..26: B'[b] = (re cr + im sr, im cr - re sr), (cr, sr) = CS of the phase
 *        (uint32)(k 27962) * (18 b + 9); the FIRST maximum of M over ascending k wins; inc = inc0 + k 27962.  The grid is 0.078124 Hz wide
 *        (27962 * 12000 / 2^32: 0.4 / T for the 4.94 s signal, as FT8's) and reaches +-2.03 Hz: f1_hz sits on the refinement's 1 Hz grid around
 *        a peak-interpolated f0_hz.
 *     2. time, at sample rate and at the refined frequency: for j = 0..54: M of the block sums at (i0 - 54 + 2 j, inc); the FIRST maximum over
 *        ascending j wins; start = i0 - 54 + 2 j.  The step is 2 samples (2/576 of a symbol against FT8's 8/1920); +-54 samples is three
 *        samples of the 666.67 Hz baseband in which ibest was found.
 *     3. frequency once more: step 1 on B at (start, inc), inc = inc + k2 27962 (df_steps = k + k2).  B at (start, inc); cnt[b] = samples of
 *        block b inside 0..72575.
 *     4. amplitude track: the FT8 rule with WIN[97] over blocks b - 48 .. b + 48 (three symbols), blocks outside 0..3295 contributing +0,
 *        normalised by the samples under the window; den > 0 else a[b] = +0.
 *     4a. the track's phase slope, a step FT8 does not have.  The symbol metric of steps 1 and 3 is not coherent across symbols, and over FT4's
 *        48 ms symbol it falls by only 4.6e-5 of its value per grid step: a neighbour one tone spacing away moves its maximum by a step (measured:
 *        0.09 Hz).  What the searches leave of the frequency turns the track from block to block, coherently over the whole
 *        signal: num = sum of (a[b+1].im a[b].re - a[b+1].re a[b].im), den = sum of (a[b+1].re a[b].re + a[b+1].im a[b].im) over b = 0..3294
 *        (two products and one sum or difference each; block 3295 contributes +0; summed as the figures of step 5 are); den > 0: d =
 *        (double)(num / den) * (2^32 / (6.283185307179586 * 18)) -- the small-angle tangent, radians per block to 2^-32 turns per sample --
 *        clamped to +-2 * 27962 (the searches are trusted to two grid steps; a NaN takes the lower bound), inc = inc + (int)rint(d); otherwise
 *        inc stays.  Then B at (start, inc) and step 4 once more: the track the record and the figures hold is the second one.  df_steps still
 *        counts the two searches alone.
 *     5. figures p_removed, p_before, p_after: the FT8 terms, summed as thread l of 256 adds the terms of blocks l, l + 256, .. ascending from
 *        +0 (13 rows), then a[l] = a[l] + a[l + h] for l < h, h = 128 .. 1.  The footprint is 666.67 Hz wide around the tone.
 *   APPLY: r = r - 2.0f * y one decode after the other IN EMISSION ORDER in a register, no atomics; y = ar c - ai s at signal sample u = t - start
 *       (0 <= u < 59328, t inside the frame), (ar, ai) the track between block centres (sample 18 b + 8.5): pp = 2 u - 17; pp < 0: a[0];
 *       b0 = min(pp / 36, 3294), m = pp - 36 b0; m >= 36: a[3295]; otherwise a[b0] + ((float)m * (1.0f / 36.0f)) * (a[b0 + 1] - a[b0]).
 * 1. cwslg_subtract_ft4 is cwslg_fetch_ft4_decode_reports' contract for the FT4 group with sub[p] the cwslg_subtract_report of dec[p] (the same
 *    28-byte struct; df_steps is k + k2, each -26..26, dt_steps is j - 27, -27..27; n_inside counts the 103 x 576 samples inside the frame;
 *    dt_s is (float)(start - 6000) / 12000.0f).  Everything point 1 of the FT8 section says holds: one ticket, one serialised call, the fetch
 *    stream, a systematic code or CWSLG_ERR_ARG, dec byte-identical to cwslg_fetch_decodes(CWSLG_GROUP_FT4) for that epoch and max, either
 *    output pointer nullable.  The residual block belongs to the FT4 group: allocated by the first call, grown on demand, freed by
 *    cwslg_destroy; a channel without an emitted decode -- and every channel at max = 0 -- gets the frame's own bits.  Two calls on one epoch
 *    leave the same bytes.  FT8 channels never take part; a context with FT8 channels alone answers CWSLG_ERR_NO_FRAME.  A frame shorter than
 *    72576 samples or not 16-byte aligned is CWSLG_ERR_ARG.  Execution: descriptors up, the three harvest launches, the 16-byte head down and
 *    one synchronise (the fit records, 26896 bytes each, are sized by what was emitted), ft4_sub_fit_kernel (one workgroup per emitted decode),
 *    ft4_sub_apply_kernel (one workgroup per channel and 1024-sample tile, 71 tiles), one copy down, one synchronise.  f_hz is the final
 *    inc (step 4a included) * 12000 / 2^32; an increment that the searches or step 4a took below 0 (freq_hz = 0 in the flat call) has wrapped
 *    modulo 2^32 and is reported as it stands, a value just under 12000, as for FT8.  The kernels are in a
 *    third code object beside the library (cwslgpu_ft4sub.hsaco), loaded by the first call; a missing file is CWSLG_ERR_ARG
 *    with a text that names it.  The call holds the group's ticket while it runs: call it right after the boundary.
 * 2. cwslg_fetch_ft4_residual copies a channel's residual (72576 floats; cap below that: CWSLG_ERR_ARG) and cwslg_ft4_residual_device_ptr hands
 *    out its device address; both only while the block's epoch is the channel's frame epoch, otherwise CWSLG_ERR_NO_FRAME.  An FT8 channel's id
 *    answers CWSLG_ERR_NO_FRAME.  An address handed out is dead from the next cwslg_subtract_ft4 call on.
 * 3. cwslg_ft4_subtract_flat runs the same two kernels on caller-supplied frames (n_frames x 72576 floats) and items, under the argument rules of
 *    cwslg_ft8_subtract_flat; dt_s in the record's convention (a transmission that starts at T seconds into the frame has dt_s = T - 0.5).
 * Out of scope: a second search or decode pass over the residual, an int16 or prepareAudio-scaled residual, rvec, joint refitting of overlapping
 * signals, unpacking to text. */
typedef struct { int32_t frame; uint8_t bits[12]; float freq_hz; float dt_s; } cwslg_ft4_sub_item;   /* 24 bytes; cwslg_ft8_sub_item's layout; freq_hz: the record's f1_hz */
#define CWSLG_FT4_FRAME_SAMPLES 72576
int cwslg_subtract_ft4(cwslg_ctx *ctx, uint64_t *start_epoch /* in/out */, cwslg_decode *dec, cwslg_subtract_report *sub, int max, int *n, int *n_total,
                       int *n_channels);
int cwslg_fetch_ft4_residual(cwslg_ctx *ctx, int ch_id, float *dst, size_t cap, size_t *n_valid, uint64_t *start_epoch);
int cwslg_ft4_residual_device_ptr(cwslg_ctx *ctx, int ch_id, const float **d_f32, uint64_t *start_epoch);
int cwslg_ft4_subtract_flat(cwslg_ctx *ctx, const float *audio /* [n_frames][72576] */, int n_frames, const cwslg_ft4_sub_item *items, int n_items,
                            cwslg_subtract_report *sub, float *residual /* [n_frames][72576] or null */);
int cwslg_fetch_slot(cwslg_ctx *ctx, int ch_id, int16_t *frame, size_t cap, void *list, size_t list_bytes,
                     cwslg_ft4_sync *ft4, int max_ft4, cwslg_slot_result *out);
int cwslg_set_ft4_syncmin(cwslg_ctx *ctx, float syncmin);

/* Intermediate products of the sync stage for parity tests: what = 0 symbol spectra [372][nbins] float,
 * 1 red, 2 red2 (float[1921], before normalisation), 3 jpeak, 4 jpeak2 (int32[1921]).  *n_items = items available.
 * FT4 channels: 0 = [122][1168] windowed spectra, 1 = savsm/sbase (first 1153 entries), 2 = sbase,
 * 5 = frame spectrum (complex float[36289]), 6 = unit-power baseband of candidate 0 (complex float[4032]).
 * Planes 1 and 2 of an FT4 channel belong to the frame of the last boundary on EVERY outcome of the search.  Where the search ends before its
 * local maxima -- a search range under 20 bins, fewer than 5 baseline points or a singular fit, a baseline that is not > 0 somewhere -- the list
 * is empty, plane 1 is savsm NOT divided by the baseline and plane 2 the baseline as far as it was computed: +0 before the fit, the fitted
 * values after it.  An all-zero frame ends that way: 10 log10(0) is -inf, the fit is NaN, plane 2 is NaN over the search range (a quiet NaN of
 * unspecified sign and payload) and +0 outside it, plane 1 is +0. */
int cwslg_sync_debug_fetch(cwslg_ctx *ctx, int ch_id, int what, void *dst, size_t cap_bytes, size_t *n_items, int *row_len);

/* ---- candidate search of the 120 s modes (BASELINE.json configs[4]) ----
 * PARITY UNPINNED like the FT8/FT4 stage: the reference hands WSPR frames to `wsprd -C <cycles> -o 5 -d <wav>` and FST4W-120
 * frames to `jt9 -W -p 120 ... -L 1400 -H 1600 -F 200 <wav>` (DecoderPool.hpp:1019-1033); what runs here is the candidate-finding
 * front end of those programs as restated in oracle/longsync_oracle.c.  When enabled, cwslg_slot_boundary() runs it on every
 * WSPR / FST4W-120 frame it finalises.
 *   WSPR:  wsprd.c main(): FFT-based /32 down-conversion to 375 Hz around 1500 Hz, 359 half-symbol 512-point spectra, smoothed
 *          spectrum / noise percentile / local maxima within +-110 Hz ordered by snr, then per candidate the coarse
 *          (frequency, shift, drift) search on the 162-symbol sync vector.  freq_hz is relative to 1500 Hz audio; shift is in
 *          375 Hz samples from the start of the file (wsprd prints DT = shift/375 - 2 s).
 *   FST4W: get_candidates_fst4.f90: comb-summed power spectrum over [nfa, nfb], 30th-percentile normalisation, CLEAN peak pick
 *          above minsync (at most 100), in order of discovery (strongest first). */
typedef struct {
    float   freq_hz;
    float   snr_db;
    float   drift;
    float   sync;
    int32_t shift;
} cwslg_wspr_candidate;
typedef struct {
    float   freq_hz;
    float   snr;            /* peak of the normalised comb spectrum ("rough estimate of SNR") */
    int32_t bin;            /* index on the baud/2 grid */
    int32_t pad_;
} cwslg_fst4w_candidate;
int cwslg_enable_long_sync(cwslg_ctx *ctx, int enable, int fst4w_nfa_hz, int fst4w_nfb_hz, float fst4w_minsync);
int cwslg_fetch_wspr_candidates(cwslg_ctx *ctx, int ch_id, cwslg_wspr_candidate *dst, int max, int *n, uint64_t *start_epoch);
int cwslg_fetch_fst4w_candidates(cwslg_ctx *ctx, int ch_id, cwslg_fst4w_candidate *dst, int max, int *n, uint64_t *start_epoch);
/* Intermediate results for parity tests.  WSPR channels: what = 0 the 375 Hz baseband (complex float[46080]), 1 the spectra
 * (float[359][512], time-major: wsprd's ps[j][i] is element [i][j]), 2 the normalised smoothed spectrum (float[411]).
 * FST4W channels: 3 the normalised comb spectrum s2 (float, indexed by the baud/2 bin), 4 the band of the long transform
 * (complex float, first bin = nint(ina*df2/df1) - ndh). */
int cwslg_long_sync_debug_fetch(cwslg_ctx *ctx, int ch_id, int what, void *dst, size_t cap_bytes, size_t *n_items);

/* ---- introspection for bench / tests ---- */
typedef struct {
    uint64_t demod_launches;       /* demod kernel launches                                   */
    uint64_t demod_samples;        /* complex input samples consumed, summed over channels    */
    uint64_t finalize_launches;
    uint64_t sync_launches;
    uint64_t frames_emitted;
    uint64_t frames_discarded;     /* startEpochTime == 0                                      */
    uint64_t blocks_dropped;       /* "af buffer full" events (Instance.cpp:268-271)           */
    uint64_t h2d_bytes;
    double   demod_ms;             /* HIP-event time of demod kernels on the context stream   */
    double   finalize_ms;
    double   sync_ms;
    uint64_t phasor_regrows;       /* checkpoint tables extended because a channel kept discarding frames */
    uint64_t rendezvous_calls;     /* slot boundaries that went through the multi-GPU rendezvous          */
    uint64_t rendezvous_frames;    /* frames over ALL processes at the last rendezvous                    */
    uint64_t rccl_world;           /* ranks of the built-in RCCL communicator (cwslg_rccl_init), 0 without one */
    uint64_t rendezvous_flags_and; /* AND over all ranks of cwslg_set_rendezvous_flag's value at the last built-in rendezvous */
    /* ABI 4 */
    double   demod_clock_mhz;      /* shader clock INSIDE the timed demod launches since the last reset: mean over launches of delta s_memtime /
                                    * delta s_memrealtime x 100 MHz, read by one workgroup at the start and the end of its life (exact mode: a
                                    * persistent workgroup, i.e. the whole launch; fast mode: the tile workgroup in the middle of the grid;
                                    * 0 until a timed launch has been drained).  What bench.py prices roofline.valu_pipe at.              */
    uint64_t demod_clock_launches; /* launches that contributed to it                                                                 */
    uint64_t push_calls;           /* host pushes accepted (cwslg_push_iq: one per call; cwslg_push_iq_many: one per receiver)         */
    uint64_t push_batches;         /* cwslg_push_iq_many calls                                                                        */
    double   push_host_ms;         /* wall time spent inside host pushes (staging copy + enqueue), summed over the calling threads      */
    double   sync_spectra_ms;      /* of sync_ms: the FT8 symbol-spectra kernel ...                                                     */
    double   sync_search_ms;       /* ... and the FT8 Costas search + candidate selection                                                */
    /* ABI 5 */
    uint64_t demod_blocks_read;    /* blocks (D input samples = one 12 kHz output each) the demod launches fetched and put through the arithmetic,
                                    * summed over channels: the pending blocks plus every stream's 32-block warm-up (exact) / every tile's
                                    * 31-block history (fast).  x D / demod_samples = redundancy.                                          */
    uint64_t process_deferred;     /* cwslg_process() calls that returned without a launch (cwslg_set_process_threshold)                    */
} cwslg_stats;
int cwslg_get_stats(cwslg_ctx *ctx, cwslg_stats *out);
int cwslg_reset_stats(cwslg_ctx *ctx);
/* Enable HIP-event timing of every kernel launch (bench.py's roofline leg).  Off by default. */
int cwslg_set_timing(cwslg_ctx *ctx, int enable);
/* Name (with template arguments) of the kernel the context's most recent demod launch ran -- what bench.py reports as
 * roofline.kernel; "" before the first launch.  The pointer is to a string literal. */
const char *cwslg_demod_kernel_name(cwslg_ctx *ctx);
/* Raw stream handle (hipStream_t) so callers can order their own work (torch, RCCL) against it. */
void *cwslg_stream(cwslg_ctx *ctx);
/* Host-side DSP constants exactly as uploaded (tests pin them against the oracle):
 * taps[32*D], tone[2*D] (re,im), phase_inc[2]; returns D (= Fs/12000) or <0. */
int cwslg_channel_constants(cwslg_ctx *ctx, int ch_id, float *taps, float *tone_ri, float *phase_inc_ri);
/* Phasor checkpoints as computed on the device: entry c is phase_{c*stride}, stride = cwslg_phasor_checkpoint_stride()
 * blocks (one block = one 12 kHz output sample).  Copies up to n complex values. */
int cwslg_phasor_checkpoint_stride(void);
int cwslg_channel_phasor_checkpoints(cwslg_ctx *ctx, int ch_id, float *dst_ri, size_t n, size_t *n_total);

#ifdef __cplusplus
}
#endif
#endif /* CWSL_GPU_H */
