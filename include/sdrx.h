/* sdrx -- MI355X (gfx950) engine for SDRangel's sdrbase/dsp RX hot path.
 *
 * C ABI of libsdrx.so.  Plain pointers and sizes only.  Every entry point names the reference
 * interface it replaces (paths relative to the lainy/sdrangel tree, v4.0.6).
 *
 * Conventions
 *   - a complex sample is the reference's `Sample` {int16 re; int16 im} packed in 4 bytes
 *     (sdrbase/dsp/dsptypes.h:44-65); buffers of them are "iq" (interleaved I,Q int16).
 *   - every function returns 0 on success or a negative code (SDRX_E*); nothing throws across
 *     the ABI.  sdrx_last_error() gives the text of the calling thread's last failure.
 *   - a handle is single-threaded (caller serialises, like one Decimators member per device
 *     thread in the reference); different handles are independent and may sit on different GPUs.
 *   - `*_dev` variants take device pointers and are asynchronous on the handle's HIP stream;
 *     the host-pointer variants copy in/out and return when the result is in the caller's buffer.
 *   - the library has NO CPU fallback: without a usable HIP device every create call fails with
 *     SDRX_ENODEV.
 */
#ifndef SDRX_H
#define SDRX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SDRX_OK        0
#define SDRX_EINVAL   -1   /* bad argument */
#define SDRX_ENODEV   -2   /* no HIP device / device index out of range */
#define SDRX_EHIP     -3   /* a HIP runtime call failed (text in sdrx_last_error) */
#define SDRX_ENOMEM   -4
#define SDRX_ESTATE   -5   /* call not valid in the handle's current state */

/* fcPos of the device plugins (limesdrinputthread.cpp:103-135): which decimateK_* is called */
#define SDRX_FC_INF 0      /* decimateK_inf */
#define SDRX_FC_SUP 1      /* decimateK_sup */
#define SDRX_FC_CEN 2      /* decimateK_cen */

/* DownChannelizer::FilterStage::Mode (sdrbase/dsp/downchannelizer.h:76-80) */
#define SDRX_MODE_CENTER 0
#define SDRX_MODE_LOWER  1
#define SDRX_MODE_UPPER  2

const char* sdrx_version(void);
const char* sdrx_last_error(void);
int         sdrx_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Decimators<qint32, qint16, 16, InputBits>  (sdrbase/dsp/decimators.h:279-341)
 * One handle == one `m_decimators` member used with ONE (log2, fcpos) -- the reference keeps the
 * six half-band states inside the object (decimators.h:326-340); so does the handle.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_decim sdrx_decim_t;

/* log2_decim 0..6, fcpos SDRX_FC_*, input_bits 8|12|16 (decimation_shifts<16,InputBits>,
 * decimators.h:25-185). */
int sdrx_decim_create(sdrx_decim_t** out, int device, int log2_decim, int fcpos, int input_bits);
/* DecimatorsU<qint32, quint8, 16, 8, Shift> (sdrbase/dsp/decimatorsu.h:175-216; RTL-SDR thread,
 * plugins/samplesource/rtlsdr/rtlsdrthread.h:55 uses Shift = 127): unsigned 8-bit I/Q, value = byte - shift,
 * decimation_shifts<16,8>.  Same cascades, strides and tail drop as Decimators. */
int sdrx_decim_create_u8(sdrx_decim_t** out, int device, int log2_decim, int fcpos, int shift);
int sdrx_decim_process_u8(sdrx_decim_t* h, const uint8_t* iq, int32_t n_uint8, int16_t* out_iq, int32_t* n_out_cplx);
/* d_iq must be 8-byte aligned */
int sdrx_decim_process_dev_u8(sdrx_decim_t* h, const uint8_t* d_iq, int64_t n_uint8, int16_t* d_out_iq, int64_t* n_out_cplx);
int sdrx_decim_destroy(sdrx_decim_t* h);
/* zero filter state == a freshly constructed Decimators object */
int sdrx_decim_reset(sdrx_decim_t* h);

/* Replaces  m_decimators.decimateK_{inf,sup,cen}(&it, buf, len)  (decimators.h:463-3885):
 * `iq`/`n_int16` are the reference's `buf`/`len`; whole groups only, a trailing partial group
 * is dropped and NOT carried (decimators.h:3492); state is carried across calls.
 * out_iq must hold n_int16/2 >> log2 complex samples; *n_out_cplx = how far `it` advanced. */
int sdrx_decim_process(sdrx_decim_t* h, const int16_t* iq, int32_t n_int16,
                       int16_t* out_iq, int32_t* n_out_cplx);

/* Same contract on device-resident buffers, asynchronous on the handle's stream.
 * d_iq must be 16-byte aligned. */
int sdrx_decim_process_dev(sdrx_decim_t* h, const int16_t* d_iq, int64_t n_int16,
                           int16_t* d_out_iq, int64_t* n_out_cplx);
/* MANY device streams, ONE launch.  The reference runs one Decimators object per device thread
 * (plugins/samplesource/limesdrinput/limesdrinputthread.cpp:103-135, filesource/testsource likewise); with many
 * concurrent device sets each of their blocks (32 768 samples for LimeSDR) is far too small to fill a GPU on its own.
 * handles[i] consumes n_elems[i] input elements at d_iq[i] (int16 for sdrx_decim_create handles, bytes for
 * sdrx_decim_create_u8 ones; same whole-group / tail-drop rule per stream, each stream's own carried state) into
 * d_out_iq[i]; n_out_cplx[i] (optional) receives how far that stream's `it` advanced.  All handles must have been created
 * with the same (log2, fcpos, input flavour) on the same device and must be distinct; everything is queued on
 * handles[0]'s stream, which the other handles join (as by sdrx_decim_set_stream) the first time.  More than 64
 * handles are served by consecutive launches of 64. */
int sdrx_decim_process_dev_batch(sdrx_decim_t* const* handles, int32_t n_handles, const void* const* d_iq,
                                 const int64_t* n_elems, int16_t* const* d_out_iq, int64_t* n_out_cplx);
/* Pinned, double-buffered HOST path (SURVEY 8b "Ownership": the async variant + sync).  The device thread's receive
 * buffer IS a slot of a pinned ring the handle owns, so a block travels host -> HBM by DMA while the previous blocks are
 * being decimated and their outputs travel back (limesdrinputthread.cpp:77-135: LMS_RecvStream(buf) -> decimate -> FIFO):
 *     void* in = sdrx_decim_ring_acquire(h);            next free slot (NULL + last_error when the ring is full)
 *     ... fill `in` with up to slot_elems elements ...
 *     sdrx_decim_ring_submit(h, n_elems);               returns at once; same whole-group / tail-drop rule per block
 *     sdrx_decim_ring_retire(h, &out, &n_out_cplx);     oldest submitted block: waits for it; `out` (pinned) stays valid
 *                                                        until that slot is acquired again
 * Blocks are retired in submission order.  `flush_slots` full blocks are coalesced into ONE copy + ONE launch (consecutive
 * blocks of a stream are consecutive samples, and a full slot is a whole number of groups, so the result is identical to
 * separate calls): 1 = every block at once (lowest latency), 16 = a LimeSDR-sized 32 768-sample block rate that is not
 * bound by launch latency.  slot_elems: int16 per slot (bytes for the u8 flavour), a whole number of groups, bytes % 16 == 0. */
int sdrx_decim_ring_create(sdrx_decim_t* h, int32_t slot_elems, int32_t n_slots, int32_t flush_slots);
int sdrx_decim_ring_destroy(sdrx_decim_t* h);
void* sdrx_decim_ring_acquire(sdrx_decim_t* h);
int sdrx_decim_ring_submit(sdrx_decim_t* h, int32_t n_elems);
int sdrx_decim_ring_retire(sdrx_decim_t* h, const int16_t** out_iq, int32_t* n_out_cplx);
int sdrx_decim_sync(sdrx_decim_t* h);
/* run on a caller-owned hipStream_t; NULL = the handle's own (non-blocking) stream.  The HIP default stream has the
 * handle value 0 and is therefore NOT selectable: work queued on it (PyTorch's default stream) is not ordered against the
 * handle's stream -- synchronise, or hand over a real stream object. */
int sdrx_decim_set_stream(sdrx_decim_t* h, void* hip_stream);
/* #int16 consumed per loop iteration of the matching reference function (its `pos +=`) */
int sdrx_decim_group_int16(int log2_decim, int fcpos);
/* One reference Decimators object runs every decimateK_x on the SAME six half-band filters (m_decimator2 .. m_decimator64,
 * decimators.h:326-333): a device thread that changes log2Decim or fcPos at run time continues on whatever each stage saw
 * last.  A handle here is one variant; `sdrx_decim_stages_t` is the object's shared filter set.  On a change of variant:
 *     sdrx_decim_save_stages(old_handle, stages);      stages 1..log2(old) := what old_handle's filters hold now
 *     sdrx_decim_load_stages(new_handle, stages);      new_handle continues from them (its own history is forgotten)
 * and the outputs equal the reference object's, bit for bit (include/sdrx/dsp.hpp does this inside sdrx::Decimators).
 * Cost: a few milliseconds per change (a one-lane walk over 4096 samples on the device); nothing on the steady path. */
typedef struct sdrx_decim_stages sdrx_decim_stages_t;
int sdrx_decim_stages_create(sdrx_decim_stages_t** s, int device);
int sdrx_decim_stages_destroy(sdrx_decim_stages_t* s);
int sdrx_decim_save_stages(sdrx_decim_t* h, sdrx_decim_stages_t* s);
int sdrx_decim_load_stages(sdrx_decim_t* h, const sdrx_decim_stages_t* s);

/* checkpoint of the carried state (the last `sdrx_decim_state_bytes()` bytes of consumed input;
 * the six ring buffers of the reference are a pure function of it) */
int64_t sdrx_decim_state_bytes(const sdrx_decim_t* h);
int sdrx_decim_get_state(sdrx_decim_t* h, void* host_buf);
int sdrx_decim_set_state(sdrx_decim_t* h, const void* host_buf);
/* HIP-event timing of the chain kernel itself, on the stream it is launched on: when enabled every
 * process call brackets its main kernel with two events; get_timing synchronises the stream and
 * returns the summed kernel time and launch count since the last reset. */
int sdrx_decim_set_timing(sdrx_decim_t* h, int enabled);
int sdrx_decim_get_timing(sdrx_decim_t* h, double* total_ms, int64_t* launches, int reset);
/* name + launch geometry of the kernel the last process call launched (for profiling/bench) */
int sdrx_decim_last_launch(const sdrx_decim_t* h, char* kernel_name, int name_cap,
                           int* grid, int* block, int* lds_bytes);
/* Fallback report of the most recent process call of this handle (auto path: FAST kernel + flagged EXACT recompute).  Synchronises
 * the handle's stream and reads back the per-chunk overflow flags the call's FAST launch wrote: one per 4096 consumed input
 * samples, 1 = the EXACT kernel recomputed that chunk.  flags_out (may be NULL) receives min(cap, total) bytes of 0 / 1.
 * Reports 0, 0 when that call ran no FAST launch (log2 = 0, SDRX_DECIM_PATH=exact, or only the serial hand-over after
 * sdrx_decim_load_stages).  In a batch every handle reports its own stream.  Nothing on the launch path depends on it. */
int sdrx_decim_last_fallback(sdrx_decim_t* h, int64_t* flagged_chunks, int64_t* total_chunks, uint8_t* flags_out, int64_t cap);

/* ------------------------------------------------------------------------------------------
 * DownChannelizer bank  (sdrbase/dsp/downchannelizer.{h,cpp}) -- N channels fed from ONE device
 * stream.  Replaces N x { ThreadedBasebandSampleSink::feed -> DownChannelizer::feed }
 * (threadedbasebandsamplesink.cpp:114-119, downchannelizer.cpp:50-91): the input is read once and
 * every distinct prefix of the channels' half-band chains is evaluated once.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_chan_bank sdrx_chan_bank_t;

/* Runs DownChannelizer::applyConfiguration's float bisection (downchannelizer.cpp:157-189,
 * 250-287) per channel: req_rate[c]/req_fc[c] are the DSPConfigureChannelizer arguments. */
int sdrx_chan_bank_create(sdrx_chan_bank_t** out, int device, int32_t in_rate, int32_t n_ch,
                          const int32_t* req_rate, const int32_t* req_fc);
int sdrx_chan_bank_destroy(sdrx_chan_bank_t* h);
/* per-channel result of the bisection == what MsgChannelizerNotification reports
 * (downchannelizer.cpp:184-187); modes[] gets n_stages entries (cap 32). */
int sdrx_chan_bank_info(const sdrx_chan_bank_t* h, int32_t ch, int32_t* n_stages, uint8_t* modes,
                        int32_t* out_rate, int32_t* residual_ofs);
/* the bisection alone, no device needed (host logic) */
int sdrx_chan_plan(int32_t in_rate, int32_t req_rate, int32_t req_fc,
                   uint8_t* modes, int32_t* out_rate, int32_t* residual_ofs);
/* DSPConfigureChannelizer for one channel: chain rebuilt with ZERO history
 * (downchannelizer.cpp:167-171 frees and recreates the stages). */
int sdrx_chan_bank_reconfigure(sdrx_chan_bank_t* h, int32_t ch, int32_t req_rate, int32_t req_fc);
/* A new DownChannelizer next to the running ones (a demod plugin added to the device set,
 * sdrbase/device/devicesourceapi.h:47-50 addThreadedSink): starts from zero history with the next feed; the existing
 * channels keep their histories and queued output.  *channel = its index. */
int sdrx_chan_bank_add_channel(sdrx_chan_bank_t* h, int32_t req_rate, int32_t req_fc, int32_t* channel);
/* removeThreadedSink: channel `ch` stops producing and its queued output is dropped; the index stays reserved
 * (it can be revived with sdrx_chan_bank_reconfigure). */
int sdrx_chan_bank_remove_channel(sdrx_chan_bank_t* h, int32_t ch);
/* number of independently planned stage tries the bank currently evaluates per feed (1 after create / reset; a
 * reconfigured or added channel runs in a trie of its own, and tries without a live channel are retired) */
/* checkpoint of the bank's filter state: every stream's history and sample count (the reference's per-stage rings are a
 * pure function of them); queued, unread output is not part of it.  A state fits only a bank with the same channels
 * configured in the same order; set_state checks the shape, drops what is queued and continues the saved timeline. */
int64_t sdrx_chan_bank_state_bytes(const sdrx_chan_bank_t* b);
int sdrx_chan_bank_get_state(sdrx_chan_bank_t* b, void* host_buf);
int sdrx_chan_bank_set_state(sdrx_chan_bank_t* b, const void* host_buf);
int32_t sdrx_chan_bank_group_count(const sdrx_chan_bank_t* h);
int sdrx_chan_bank_reset(sdrx_chan_bank_t* h);

/* Replaces DownChannelizer::feed(begin, end, positiveOnly) for every channel of the bank.  Any
 * n_cplx; decimation phase is carried across calls (no drop).  Outputs accumulate in per-channel
 * device queues until read. */
int sdrx_chan_bank_feed(sdrx_chan_bank_t* h, const int16_t* iq, int64_t n_cplx);
int sdrx_chan_bank_feed_dev(sdrx_chan_bank_t* h, const int16_t* d_iq, int64_t n_cplx);
/* number of complex outputs of channel ch waiting to be read */
int64_t sdrx_chan_bank_available(sdrx_chan_bank_t* h, int32_t ch);
/* == the m_sampleBuffer handed to m_sampleSink->feed (downchannelizer.cpp:87): copies up to cap
 * complex samples of channel ch to host memory and removes them; returns the count (<0: error) */
int64_t sdrx_chan_bank_read(sdrx_chan_bank_t* h, int32_t ch, int16_t* out_iq, int64_t cap);
/* readCommit-style: discard up to n queued samples of channel ch without copying (n < 0: all) */
int64_t sdrx_chan_bank_skip(sdrx_chan_bank_t* h, int32_t ch, int64_t n);
/* device-side view of what the last feed produced for channel ch (valid until the next feed) */
int sdrx_chan_bank_last_dev(sdrx_chan_bank_t* h, int32_t ch, const int16_t** d_out_iq, int64_t* n_cplx);
int sdrx_chan_bank_sync(sdrx_chan_bank_t* h);
int sdrx_chan_bank_set_stream(sdrx_chan_bank_t* h, void* hip_stream);
/* the hipStream_t the bank's kernels run on (its own stream unless set_stream gave it another) */
int sdrx_chan_bank_get_stream(sdrx_chan_bank_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's tree_kernel launches (all passes) */
int sdrx_chan_bank_set_timing(sdrx_chan_bank_t* h, int enabled);
int sdrx_chan_bank_get_timing(sdrx_chan_bank_t* h, double* total_ms, int64_t* feeds, int reset);
int sdrx_chan_bank_last_launch(const sdrx_chan_bank_t* h, char* kernel_name, int name_cap,
                               int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * Channel back-end bank: what every channelrx demod does with the DownChannelizer output before its
 * audio-rate tail (plugins/channelrx/demodnfm/nfmdemod.cpp:150-163, demodssb/ssbdemod.cpp:158-172):
 *     Complex c(re, im); c *= m_nco.nextIQ();                         NCO (sdrbase/dsp/nco.cpp:30-64)
 *     if (m_interpolator.decimate(&dist, c, &ci)) { ... dist += step } Interpolator (interpolator.h:23-36)
 *     n = filter->runSSB(ci, &sideband, usb) | runFilt(...)            fftfilt (fftfilt.cpp:261-325), g_fft
 *     demod = m_phaseDiscri.phaseDiscriminatorDelta(...)               phasediscri.h:50-78
 * One handle holds N channels; every feed produces that feed's outputs (like the demod's feed()
 * running to completion), read them before the next feed.  float32, <= 1 ulp of the strict-IEEE
 * scalar reference build (SURVEY.md finding 6).
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_backend sdrx_backend_t;
typedef struct sdrx_backend_cfg {
    int32_t in_rate;         /* channelizer output rate: m_nco.setFreq(nco_freq, in_rate) */
    int32_t nco_freq;        /* the demods pass -frequencyOffset of MsgChannelizerNotification */
    int32_t out_rate;        /* audio / demod rate; distance step = (Real) in_rate / (Real) out_rate; <= in_rate */
    float   interp_cutoff;   /* m_interpolator.create(16, in_rate, interp_cutoff, taps_per_phase) */
    float   taps_per_phase;  /* 4.5 (default, NFM) or 2.0 (SSB): (int)(taps_per_phase * 16) taps per phase, made even;
                              * 0.0625 .. 16.0 (1 .. 256 taps), anything else is refused with SDRX_EINVAL */
    int32_t filt_mode;       /* 0 none, 1 runFilt, 2 runSSB usb, 3 runSSB lsb, 4 runDSB  (getDC = true),
                              * 5 runAsym usb, 6 runAsym lsb: fftfilt(f2, 2048) + create_asym_filter(fopp = f1, fin = f2) (atvdemod.cpp:262,647),
                              * 7 runFilt at length 2048 on create_rrc_filter(fb = f1, a = f2) (chanalyzer.cpp:305): the root raised
                              * cosine written in the frequency domain */
    float   f1, f2;          /* modes 1-3: fftfilt(f1, f2, 1024); mode 4: fftfilt(f2, 2048) (DSBFilter, ssbdemod.cpp:92); normalised to the OUTPUT rate */
    int32_t discri;          /* 0 none, 1 phaseDiscriminatorDelta (NFM; bit-identical to the strict-IEEE reference),
                              * 2 phaseDiscriminator (UDPSrc): std::arg = atan2f.  The device evaluates a double atan2 rounded once
                              * to float: <= 3 ulp from glibc's atan2f (2 measured, tests/test_backend_gpu.py), i.e. outside the
                              * 1 ulp of the other float stages -- parity with a given reference binary depends on that box's libm. */
    float   fm_scaling;      /* setFMScaling */
} sdrx_backend_cfg;
int sdrx_backend_create(sdrx_backend_t** out, int device, int32_t n_ch, const sdrx_backend_cfg* cfg);
int sdrx_backend_destroy(sdrx_backend_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to m_sampleSink->feed) */
int sdrx_backend_feed(sdrx_backend_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
int sdrx_backend_feed_dev(sdrx_backend_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* cfg 4 hand-over without a host round trip: channel c takes what the bank's last feed produced for its channel c
 * (sdrx_chan_bank_last_dev), ordered on the device -- the back-end's readers wait for the bank's stream, and the bank's
 * stream waits until they have consumed the samples before anything queued on it later (its next feed) may run.
 * The distance schedule, which needs the counts only, overlaps the bank's kernels. */
int sdrx_backend_feed_bank(sdrx_backend_t* h, sdrx_chan_bank_t* bank);
/* outputs of the last feed for channel ch: complex (re,im pairs) unless a discriminator is on;
 * returns the number of FLOATS written (<0: error) */
int64_t sdrx_backend_read(sdrx_backend_t* h, int32_t ch, float* out, int64_t cap_floats);
/* device-side view of the same (valid until the next feed): pointer and number of FLOATS */
int sdrx_backend_last_dev(sdrx_backend_t* h, int32_t ch, const float** d_out, int64_t* n_floats);
/* design products, for inspection: polyphase taps [16][ntaps], filter spectrum (2048 complex slots; 1024 used
 * unless filt_mode 4), NCO increment */
int sdrx_backend_get_design(sdrx_backend_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                            float* filter_iq, int32_t* nco_inc);
int sdrx_backend_sync(sdrx_backend_t* h);

/* ------------------------------------------------------------------------------------------
 * Audio-rate tail of the NFM and SSB demodulators -- what follows the resampler / fftfilt in
 * NFMDemod::feed (plugins/channelrx/demodnfm/nfmdemod.cpp:150-300; m_deltaSquelch, m_ctcssOn, m_audioMute off) and
 * SSBDemod::feed (plugins/channelrx/demodssb/ssbdemod.cpp:181-250; mono): discriminator + power squelch + gate delay
 * line + 301-tap Bandpass for NFM, MagAGC (sdrbase/dsp/agc.cpp:96-175) + delay line + step value for SSB, down to the
 * qint16 the demod writes to both channels of m_audioBuffer.  Input per channel: the complex float stream the demod body
 * sees (sdrx_backend_* with discri = 0: resampler output for NFM, fftfilt sideband for SSB).  One output per input.
 * Serial state machines: one lane per channel, N channels per handle.  m_prevArg of the reference's PhaseDiscriminators
 * is uninitialised (phasediscri.h:139); it starts at 0 here.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_audiotail sdrx_audiotail_t;
typedef struct sdrx_audiotail_cfg {
    int32_t kind;                 /* 0 NFM, 1 SSB */
    int32_t audio_rate;           /* m_audioSampleRate (48000) */
    float   volume;               /* m_settings.m_volume (NFM) / m_volume (SSB) */
    /* NFM */
    float   fm_scaling;           /* m_phaseDiscri.setFMScaling(): (float) audioRate / (2 * fmDeviation) */
    float   squelch_level;        /* m_squelchLevel: linear power */
    int32_t squelch_gate;         /* m_squelchGate, samples */
    float   af_bandwidth;         /* m_bandpass.create(301, rate, 300.0, af_bandwidth) */
    /* SSB: MagAGC(12000, agcTarget, 1e-2) after resize(n, n / 2, agcTarget), setStepDownDelay(n) (ssbdemod.cpp:411-414) */
    int32_t agc_active;           /* settings.m_agc; off: agcVal = 10.0 */
    int32_t agc_nb_samples;       /* (audioRate / 1000) * (1 << agcTimeLog2) */
    int32_t agc_threshold_enable; /* setThresholdEnable */
    int32_t agc_gate;             /* setGate, samples */
    int32_t agc_clamping;         /* setClamping; clampMax = SDR_RX_SCALED / 100 */
    double  agc_threshold;        /* setThreshold: powerFromdB(dB) * 32768^2 */
} sdrx_audiotail_cfg;
int sdrx_audiotail_create(sdrx_audiotail_t** h, int device, int32_t n_ch, const sdrx_audiotail_cfg* cfg);
int sdrx_audiotail_destroy(sdrx_audiotail_t* h);
int sdrx_audiotail_reset(sdrx_audiotail_t* h);
/* in[c]: n[c] complex floats (re, im); audio[c]: n[c] qint16 (the value written to .l and .r) */
int sdrx_audiotail_feed(sdrx_audiotail_t* h, const float* const* in, const int64_t* n, int16_t* const* audio);
int sdrx_audiotail_feed_dev(sdrx_audiotail_t* h, const float* const* d_in, const int64_t* n, int16_t* const* d_audio);
int sdrx_audiotail_sync(sdrx_audiotail_t* h);

/* ------------------------------------------------------------------------------------------
 * The 24-bit sample build of the integer half-band path (the reference compiled with SDR_RX_SAMPLE_24BIT: dsptypes.h:24-34
 * FixReal = qint32 and an 8-byte Sample; decimators.h:326-333, downchannelizer.h:78-81 IntHalfbandFilterEO<qint64,qint64,N>;
 * decimation_shifts<24,InputBits>, decimators.h:62-185).  Samples in and out of these calls are {int32 re, int32 im}.
 *   sdrx_decim24_*      Decimators<qint32, qint16, 24, {8,12,16}>::decimate{1..64}_{cen,inf,sup}: same call contract as
 *                       sdrx_decim_process (whole groups, dropped tail, carried state); out_iq holds 2 x int32 per sample
 *   sdrx_chan24_bank_*  N DownChannelizers on a 24-bit stream: any feed length, carried phase, final `/= (1 << n)`;
 *                       sdrx_chan24_bank_read returns what the LAST feed produced for the channel
 * Exact (incl. the build's 32-bit wrap of the centre tap, inthalfbandfiltereo.h:818-827), plain 64-bit arithmetic, not tuned.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_decim24 sdrx_decim24_t;
int sdrx_decim24_create(sdrx_decim24_t** h, int device, int log2_decim, int fcpos, int input_bits);
int sdrx_decim24_destroy(sdrx_decim24_t* h);
int sdrx_decim24_reset(sdrx_decim24_t* h);
int sdrx_decim24_process(sdrx_decim24_t* h, const int16_t* iq, int32_t n_int16, int32_t* out_iq, int32_t* n_out_cplx);
/* device pointers, asynchronous on the handle's stream (sdrx_decim24_sync waits): d_iq = n_cplx int16 pairs, d_out = room for
 * (n_cplx >> log2) + 1 samples of 8 bytes; *n_out_cplx = samples this call produced (the phase carries) */
int sdrx_decim24_process_dev(sdrx_decim24_t* h, const void* d_iq, int64_t n_cplx, void* d_out, int64_t* n_out_cplx);
int sdrx_decim24_sync(sdrx_decim24_t* h);
typedef struct sdrx_chan24_bank sdrx_chan24_bank_t;
int sdrx_chan24_bank_create(sdrx_chan24_bank_t** h, int device, int32_t in_rate, int32_t n_ch, const int32_t* req_rate, const int32_t* req_fc);
int sdrx_chan24_bank_destroy(sdrx_chan24_bank_t* h);
int sdrx_chan24_bank_reset(sdrx_chan24_bank_t* h);
int sdrx_chan24_bank_info(const sdrx_chan24_bank_t* h, int32_t ch, int32_t* n_stages, uint8_t* modes, int32_t* out_rate, int32_t* residual_ofs);
int sdrx_chan24_bank_feed(sdrx_chan24_bank_t* h, const int32_t* iq, int64_t n_cplx);
int64_t sdrx_chan24_bank_read(sdrx_chan24_bank_t* h, int32_t ch, int32_t* out_iq, int64_t cap);
/* device pointers: feed n_cplx {int32,int32} from HBM, then look at each channel's output where it lies (valid until the
 * next feed); asynchronous on the bank's stream, sdrx_chan24_bank_sync waits */
int sdrx_chan24_bank_feed_dev(sdrx_chan24_bank_t* h, const void* d_iq, int64_t n_cplx);
int sdrx_chan24_bank_out_dev(sdrx_chan24_bank_t* h, int32_t ch, const void** d_out, int64_t* n_cplx);
int sdrx_chan24_bank_sync(sdrx_chan24_bank_t* h);

/* ------------------------------------------------------------------------------------------
 * IIRFilter<float, Order> (sdrbase/dsp/iirfilter.h; FilterMbe's low/high-pass pair, filtermbe.h:76-77): N recursive
 * filters, one per channel, state carried across feeds.  `a` / `b` are the constructor's arguments in the reference's
 * meaning: order 2 = the specialisation (y = b0 s + b1 x0 + b2 x1 + a1 y0 + a2 y1); other orders = the generic template,
 * including its swapped coefficient copy (iirfilter.h:78-81).  Serial along time: one lane per channel.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_iir sdrx_iir_t;
typedef struct sdrx_iir_cfg { int32_t order; float a[9]; float b[9]; } sdrx_iir_cfg;   /* order 2..8, order + 1 coefficients each */
int sdrx_iir_create(sdrx_iir_t** h, int device, int32_t n_ch, const sdrx_iir_cfg* cfg);
int sdrx_iir_destroy(sdrx_iir_t* h);
int sdrx_iir_reset(sdrx_iir_t* h);
int sdrx_iir_feed(sdrx_iir_t* h, const float* const* in, const int64_t* n, float* const* out);

/* ------------------------------------------------------------------------------------------
 * Lowpass<Real> / Bandpass<Real> (sdrbase/dsp/lowpass.h:11-105, bandpass.h:11-128): the symmetric-folded real
 * FIRs of the demods' audio tail (NFM: m_lowpass.create(301, rate, 250.0), m_bandpass.create(301, rate, 300.0, bw),
 * nfmdemod.cpp:88,428-429; filter() per audio sample :239,279), N channels per handle, state carried across feeds.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_firbank sdrx_firbank_t;
typedef struct sdrx_fir_cfg {
    int32_t kind;            /* 0: Lowpass::create(ntaps, sample_rate, f1); 1: Bandpass::create(ntaps, sample_rate, f1, f2) */
    int32_t ntaps;           /* made odd like the reference does */
    float   sample_rate, f1, f2;
} sdrx_fir_cfg;
int sdrx_firbank_create(sdrx_firbank_t** out, int device, int32_t n_ch, const sdrx_fir_cfg* cfg);
int sdrx_firbank_destroy(sdrx_firbank_t* h);
/* == filter(sample) for every sample of in[c]; out[c] gets n_per_ch[c] floats */
int sdrx_firbank_feed(sdrx_firbank_t* h, const float* const* in, const int64_t* n_per_ch, float* const* out);
/* the ntaps/2 + 1 folded taps (m_taps); returns their count */
int sdrx_firbank_get_taps(const sdrx_firbank_t* h, int32_t ch, float* taps, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * SampleSinkFifo (sdrbase/dsp/samplesinkfifo.{h,cpp}) -- host ring of `Sample`, same
 * write / readBegin / readCommit contract, minus the Qt signal (a callback instead of dataReady()).
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_fifo sdrx_fifo_t;
typedef void (*sdrx_fifo_data_ready_cb)(void* user);
int      sdrx_fifo_create(sdrx_fifo_t** out, uint32_t size_samples);          /* SampleSinkFifo(int) + setSize */
int      sdrx_fifo_destroy(sdrx_fifo_t* f);
int      sdrx_fifo_set_size(sdrx_fifo_t* f, uint32_t size_samples);           /* setSize: also empties */
uint32_t sdrx_fifo_size(sdrx_fifo_t* f);
uint32_t sdrx_fifo_fill(sdrx_fifo_t* f);
void     sdrx_fifo_on_data_ready(sdrx_fifo_t* f, sdrx_fifo_data_ready_cb cb, void* user);
/* write(const quint8* data, uint count) (samplesinkfifo.cpp:70-111): count in BYTES, returns samples written */
uint32_t sdrx_fifo_write_bytes(sdrx_fifo_t* f, const uint8_t* data, uint32_t count_bytes);
/* write(begin, end) (samplesinkfifo.cpp:113-153): count in samples */
uint32_t sdrx_fifo_write(sdrx_fifo_t* f, const int16_t* iq, uint32_t count_samples);
/* read(begin, end) (samplesinkfifo.cpp:155-191) */
uint32_t sdrx_fifo_read(sdrx_fifo_t* f, int16_t* iq, uint32_t count_samples);
/* readBegin / readCommit (samplesinkfifo.cpp:193-231): two spans as offsets into the ring */
uint32_t sdrx_fifo_read_begin(sdrx_fifo_t* f, uint32_t count, const int16_t** part1, uint32_t* n1,
                              const int16_t** part2, uint32_t* n2);
uint32_t sdrx_fifo_read_commit(sdrx_fifo_t* f, uint32_t count);
/* samples dropped by overflowing writes since creation (the reference only logs them) */
uint64_t sdrx_fifo_dropped(sdrx_fifo_t* f);

/* ------------------------------------------------------------------------------------------
 * .sdriq record files (sdrbase/dsp/filerecord.cpp:129-148; read by the FileSource plugin,
 * plugins/samplesource/filesource/filesourceinput.cpp / filesourcethread.cpp:170-229).
 * Layout: qint32 sampleRate | quint64 centerFrequency | time_t startTimeStamp | quint32 sampleSize, written
 * field by field = 24 bytes, then raw `Sample`s.  readHeader() treats any sampleSize other than 16/24 as 16.
 * Reference quirk kept visible: on end-of-file FileSourceThread::tick() rewinds to sizeof(FileRecord::Header),
 * which is 32 with struct padding, i.e. loop playback skips the first two samples of the file.
 * ------------------------------------------------------------------------------------------ */
#define SDRX_SDRIQ_HEADER_BYTES 24
#define SDRX_SDRIQ_LOOP_OFFSET  32
typedef struct sdrx_sdriq_header {
    int32_t  sample_rate;
    uint64_t center_frequency;
    int64_t  start_timestamp;
    uint32_t sample_size;       /* 16 or 24 after parsing */
} sdrx_sdriq_header;
int sdrx_sdriq_parse_header(const uint8_t* bytes, uint64_t n_bytes, sdrx_sdriq_header* out);
int sdrx_sdriq_write_header(uint8_t* bytes24, const sdrx_sdriq_header* hdr);

/* ---- float half-band decimators ----
 * DecimatorsFI (sdrbase/dsp/decimatorsfi.h:29-57: float I/Q in, int16 Sample out; the AirspyHF thread's member,
 * plugins/samplesource/airspyhf/airspyhfthread.h), DecimatorsFF (decimatorsff.h: float in, float FSample out) and
 * DecimatorsIF<qint16,InputBits> (decimatorsif.h:52-79: int16 in, float out), all over IntHalfbandFilterEOF<64>
 * (inthalfbandfiltereof.h).  One handle = one decimateK_{inf,sup,cen} method of one object: (log2_decim, fcpos).
 *   in_kind  0 float I/Q            1 int16 I/Q, scaled by decimation_scale<input_bits> (8|12|16) at the output
 *   out_kind 0 int16 Sample = (int16)(v * SDR_RX_SCALED), truncation (float input only)      1 float re, im
 * n_elems = the reference's nbIAndQ (floats or int16s); whole groups only, tail dropped; filter state carried.
 * Results are bit-identical to the reference built without -ffast-math (same operation order, no FMA).
 * The out_kind 0 conversion is what x86-64 gives: cvttss2si / cvttsd2si and the low 16 bits, so a product outside the int32
 * range, and NaN, give 0. */
typedef struct sdrx_fdecim sdrx_fdecim_t;
#define SDRX_FD_IN_F32  0
#define SDRX_FD_IN_I16  1
#define SDRX_FD_OUT_I16 0
#define SDRX_FD_OUT_F32 1
int sdrx_fdecim_create(sdrx_fdecim_t** out, int device, int log2_decim, int fcpos, int in_kind, int out_kind, int input_bits);
int sdrx_fdecim_destroy(sdrx_fdecim_t* h);
int sdrx_fdecim_reset(sdrx_fdecim_t* h);
/* host pointers; blocking.  *n_out_cplx = advance of the reference's output iterator */
int sdrx_fdecim_process(sdrx_fdecim_t* h, const void* in, int32_t n_elems, void* out, int32_t* n_out_cplx);
/* device pointers (d_in 16-byte, d_out 8-byte aligned); asynchronous on the handle's stream */
int sdrx_fdecim_process_dev(sdrx_fdecim_t* h, const void* d_in, int64_t n_elems, void* d_out, int64_t* n_out_cplx);
int sdrx_fdecim_sync(sdrx_fdecim_t* h);
int sdrx_fdecim_set_stream(sdrx_fdecim_t* h, void* hip_stream);
/* input elements per loop iteration of the reference method (its `pos +=` stride) */
int32_t sdrx_fdecim_group(int log2_decim, int fcpos);
/* checkpoint of the carried state (the cascade's filter rings) */
int64_t sdrx_fdecim_state_bytes(const sdrx_fdecim_t* h);
int sdrx_fdecim_get_state(sdrx_fdecim_t* h, void* host_buf);
int sdrx_fdecim_set_state(sdrx_fdecim_t* h, const void* host_buf);
/* the six IntHalfbandFilterEOF members that all decimateK_x of one DecimatorsFI / FF / IF object share (cascade stage s is
 * member s in every variant): same protocol as sdrx_decim_save_stages / _load_stages.  The float handles carry their filters'
 * rings explicitly, so both calls are plain device copies. */
typedef struct sdrx_fdecim_stages sdrx_fdecim_stages_t;
int sdrx_fdecim_stages_create(sdrx_fdecim_stages_t** s, int device);
int sdrx_fdecim_stages_destroy(sdrx_fdecim_stages_t* s);
int sdrx_fdecim_save_stages(sdrx_fdecim_t* h, sdrx_fdecim_stages_t* s);
int sdrx_fdecim_load_stages(sdrx_fdecim_t* h, const sdrx_fdecim_stages_t* s);
int sdrx_fdecim_set_timing(sdrx_fdecim_t* h, int enabled);
int sdrx_fdecim_get_timing(sdrx_fdecim_t* h, double* total_ms, int64_t* launches, int reset);
int sdrx_fdecim_last_launch(const sdrx_fdecim_t* h, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes);

/* ---- DC offset correction of the device stream ----
 * What DSPDeviceSourceEngine::work does to every FIFO span before the sinks see it when m_dcOffsetCorrection is set
 * (dspdevicesourceengine.cpp:339-343,375-379 -> iqCorrections(begin, end, false), :175-181,255-259):
 * re -= (int32) m_iBeta, im -= (int32) m_qBeta with MovingAverageUtil<int32_t,int64_t,1024> averages (total of the last
 * 1024 samples / 1024, truncating).  State (the last 1023 samples) is carried across calls; reset == fresh engine.
 * The I/Q imbalance branch (:183-253: float/double averages, a division and a sqrt per sample, serial) is not offered. */
typedef struct sdrx_dccorr sdrx_dccorr_t;
int sdrx_dccorr_create(sdrx_dccorr_t** out, int device);
int sdrx_dccorr_destroy(sdrx_dccorr_t* h);
int sdrx_dccorr_reset(sdrx_dccorr_t* h);
/* in place on a host span, like the reference (blocking) */
int sdrx_dccorr_process(sdrx_dccorr_t* h, int16_t* iq, int64_t n_cplx);
/* device buffers, asynchronous on the handle's stream; d_out_iq must not alias d_iq */
int sdrx_dccorr_process_dev(sdrx_dccorr_t* h, const int16_t* d_iq, int16_t* d_out_iq, int64_t n_cplx);

/* I/Q imbalance correction of the device stream: DSPDeviceSourceEngine::iqCorrections(begin, end, imbalanceCorrection = true)
 * (dspdevicesourceengine.cpp:175-181, 217-253, float flavour: IMBALANCE_INT is not defined), i.e. DC removal + phase and
 * amplitude imbalance estimated by 128-deep float/double moving averages, in the reference's statement order.  The
 * recurrence is serial per stream, so ONE handle serves `n_streams` device streams side by side (one lane each).
 * Buffers are rewritten in place like the reference rewrites the FIFO span.  State carries across calls; reset = freshly
 * constructed engine members.  The float -> qint16 conversion of both outputs is what x86-64 gives: cvttss2si and the low
 * 16 bits, so a product outside the int32 range, and NaN (the amplitude average after a negative residue), give 0. */
typedef struct sdrx_iqimb sdrx_iqimb_t;
int sdrx_iqimb_create(sdrx_iqimb_t** h, int device, int32_t n_streams);
int sdrx_iqimb_destroy(sdrx_iqimb_t* h);
int sdrx_iqimb_reset(sdrx_iqimb_t* h);
int sdrx_iqimb_process(sdrx_iqimb_t* h, int16_t* const* iq, const int64_t* n_cplx);
int sdrx_iqimb_process_dev(sdrx_iqimb_t* h, const int16_t* const* d_iq, int16_t* const* d_out_iq, const int64_t* n_cplx);
int sdrx_iqimb_sync(sdrx_iqimb_t* h);
int sdrx_iqimb_set_stream(sdrx_iqimb_t* h, void* hip_stream);
int sdrx_dccorr_sync(sdrx_dccorr_t* h);
int sdrx_dccorr_set_stream(sdrx_dccorr_t* h, void* hip_stream);

/* ---- diagnostics ----
 * SURVEY 8(d) quotes the HBM roofline twice: the datasheet's 8 TB/s and what a read-only streaming kernel
 * (sum of int32 over n_bytes, best of reps launches) reaches on this box.  Not part of the sample path. */
int sdrx_measure_hbm_read(int device, uint64_t n_bytes, int32_t reps, double* gb_per_s);

/* ------------------------------------------------------------------------------------------
 * Fan-out of one staged source stream to several GPUs by peer copies (xGMI on an 8 x MI355X node): SURVEY 8e's optional
 * staging path -- "one stream per GPU, xGMI only for fan-out, no collective on the per-sample path".  A stream uploaded (or
 * decimated) once on `src_device` is copied point-to-point into one buffer per destination GPU, each on its own stream;
 * the consumers (e.g. one channelizer bank per GPU over the same 61.44 MS/s stream) read their local copy.
 *   send      asynchronous; the copies start when what `producer_stream` (on src_device; NULL = everything queued on the
 *             legacy stream) holds so far is done
 *   buffer    destination i's device pointer (on dst_devices[i]); valid contents after wait / stream_wait
 *   wait      host waits for destination i;  stream_wait: a consumer stream on that GPU waits instead (device-ordered)
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_fanout sdrx_fanout_t;
int sdrx_fanout_create(sdrx_fanout_t** f, int src_device, int32_t n_dst, const int32_t* dst_devices, int64_t max_bytes);
int sdrx_fanout_destroy(sdrx_fanout_t* f);
int sdrx_fanout_send(sdrx_fanout_t* f, const void* d_src, int64_t bytes, void* producer_stream);
void* sdrx_fanout_buffer(sdrx_fanout_t* f, int32_t i);
int sdrx_fanout_wait(sdrx_fanout_t* f, int32_t i);
int sdrx_fanout_stream_wait(sdrx_fanout_t* f, int32_t i, void* consumer_stream);

/* ------------------------------------------------------------------------------------------
 * SpectrumVis (sdrgui/dsp/spectrumvis.{h,cpp}:70-300, v4.0.6, kissfft engine: sdrbase/dsp/kissfft.h, fftwindow.{h,cpp},
 * util/movingaverage2d.h, util/fixedaverage2d.h): the spectrum / waterfall sink a device set feeds with every raw span
 * (dspdevicesourceengine.cpp:360-363).  Each frame the reference hands to GLSpectrum::newSpectrum(powerSpectrum, N) is
 * queued on the device until read: N floats, fft-shifted (with positive_only: bin i at 2i and 2i+1), dB or linear.
 *   - frames, linear output and the averaged power are bit-identical to the reference (tests/golden/spectrum_golden.npz
 *     is recorded from the reference's own SpectrumVis); dB output is m_mult * log2f(v) + m_ofs with log2f evaluated in
 *     double and rounded once.  That log2f differs from glibc's by 1 ulp on about 1.5e-4 of inputs, and where the sum
 *     cancels (values near 0 dB) one ulp of log2f becomes several ulps of the dB value: up to 16 ulp measured
 *   - the 4096-entry buffer and its quirks are kept: with overlap, consecutive frames share no samples and the ends of
 *     the frame hold the buffer's leftovers (zeros for a fresh object, older samples after a mid-stream configure)
 *   - deliberate divergences, all rejected with SDRX_EINVAL before any device call: 2 * overlap >= fft_size (the
 *     reference loops forever at 50 % and writes past its buffer above), a fft_size that is not a power of two after the
 *     clamp to [64, 4096], a window or avg_mode outside the enums, a zero or non-finite scalef
 *   - configure that changes fft_size while frames are queued fails with SDRX_ESTATE (read or skip them first)
 *   - the queue has no cap: it grows by 4 * fft_size bytes per queued frame until the caller reads or skips the frames,
 *     so a consumer that falls behind must drain it (sdrx_spectrum_read / sdrx_spectrum_skip) after every feed or so
 * ------------------------------------------------------------------------------------------ */
/* FFTWindow::Function (fftwindow.h) */
#define SDRX_SPECTRUM_BARTLETT       0
#define SDRX_SPECTRUM_BLACKMANHARRIS 1
#define SDRX_SPECTRUM_FLATTOP        2
#define SDRX_SPECTRUM_HAMMING        3
#define SDRX_SPECTRUM_HANNING        4
#define SDRX_SPECTRUM_RECTANGLE      5
/* SpectrumVis::AveragingMode */
#define SDRX_SPECTRUM_AVG_NONE   0
#define SDRX_SPECTRUM_AVG_MOVING 1
#define SDRX_SPECTRUM_AVG_FIXED  2
typedef struct sdrx_spectrum sdrx_spectrum_t;
typedef struct sdrx_spectrum_cfg {
    int32_t  fft_size;          /* clamped to [64, 4096] like handleConfigure */
    int32_t  overlap_percent;   /* clamped to [0, 100]; overlap = fft_size * pct / 100 */
    uint32_t avg_nb;            /* averaging depth / block size; <= 1: no averaging */
    int32_t  avg_mode;          /* SDRX_SPECTRUM_AVG_* */
    int32_t  window;            /* SDRX_SPECTRUM_* window */
    int32_t  linear;            /* 0: dB, 1: v / N^2 */
    float    scalef;            /* SpectrumVis(Real scalef): 32768 for the 16-bit build */
} sdrx_spectrum_cfg;
/* SpectrumVis(scalef) + handleConfigure(cfg) */
int sdrx_spectrum_create(sdrx_spectrum_t** out, int device, const sdrx_spectrum_cfg* cfg);
int sdrx_spectrum_destroy(sdrx_spectrum_t* h);
/* a freshly constructed object with the current configuration: zero buffer and averages, empty queue */
int sdrx_spectrum_reset(sdrx_spectrum_t* h);
/* handleConfigure: keeps the 4096-entry buffer, fill = overlap, zeroes the averages */
int sdrx_spectrum_configure(sdrx_spectrum_t* h, const sdrx_spectrum_cfg* cfg);
/* feed(begin, end, positiveOnly): n_cplx `Sample`s; partial frames carry across feeds */
int sdrx_spectrum_feed(sdrx_spectrum_t* h, const int16_t* iq, int64_t n_cplx, int positive_only);
/* same on a device pointer (4-byte aligned), asynchronous on the handle's stream */
int sdrx_spectrum_feed_dev(sdrx_spectrum_t* h, const int16_t* d_iq, int64_t n_cplx, int positive_only);
/* frames queued (newSpectrum calls not yet read) */
int64_t sdrx_spectrum_available(sdrx_spectrum_t* h);
/* copies up to max_frames queued frames (fft_size floats each) in call order; returns the number copied */
int64_t sdrx_spectrum_read(sdrx_spectrum_t* h, float* out, int64_t max_frames);
/* drops up to n queued frames (n < 0: all); returns the number dropped */
int64_t sdrx_spectrum_skip(sdrx_spectrum_t* h, int64_t n);
/* FFTWindow::m_window of the current configuration; returns fft_size (copies min(cap, fft_size)) */
int sdrx_spectrum_window(const sdrx_spectrum_t* h, float* out, int32_t cap);
int sdrx_spectrum_sync(sdrx_spectrum_t* h);
int sdrx_spectrum_set_stream(sdrx_spectrum_t* h, void* hip_stream);
int sdrx_spectrum_get_stream(sdrx_spectrum_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels */
int sdrx_spectrum_set_timing(sdrx_spectrum_t* h, int enabled);
int sdrx_spectrum_get_timing(sdrx_spectrum_t* h, double* total_ms, int64_t* feeds, int reset);
int sdrx_spectrum_last_launch(const sdrx_spectrum_t* h, char* kernel_name, int name_cap,
                              int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * Wideband (broadcast) FM demodulator bank: WFMDemod::feed (plugins/channelrx/demodwfm/wfmdemod.cpp:90-183), N channels
 * per handle, each fed with int16 I/Q at the channelizer's output rate:
 *     c = Complex(re, im) * m_nco.nextIQ();                               NCO (sdrbase/dsp/nco.cpp:30-64)
 *     rf_out = m_rfFilter->runFilt(c, &rf);                                fftfilt 1024 at the CHANNEL rate (fftfilt.cpp:261-282)
 *     per rf[i]: magsq + level sums, squelch counter, phaseDiscriminatorDelta only while the squelch is open
 *                (m_prevArg survives closed stretches), m_interpolator.decimate on Complex(demod, 0),
 *                (qint16)(ci.real() * 3276.8f * volume)
 * Output: mono qint16 audio, the value the reference writes to .l and .r, bit-identical to the strict-IEEE scalar
 * reference build with m_prevArg starting at 0 (as sdrx_audiotail_*).  Any feed length is valid (0 and < 512 included:
 * a feed that completes no 512-sample block produces no audio); NCO phase, pending samples, ovlbuf, squelch counter,
 * m_prevArg, resampler window and distance, and the level accumulators carry across feeds.  m_movingAverage (GUI only)
 * is left out.  A channel is configured at creation; there is no mid-stream retune.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_wfm sdrx_wfm_t;
typedef struct sdrx_wfm_cfg {
    int32_t in_rate;        /* channelizer output rate (m_inputSampleRate) */
    int32_t nco_freq;       /* m_nco.setFreq(nco_freq, in_rate): the demod passes -frequencyOffset */
    int32_t audio_rate;     /* m_audioSampleRate; <= in_rate; distance = step = (Real) in_rate / (Real) audio_rate */
    float   rf_bandwidth;   /* m_rfBandwidth: create_filter(-(rfBW / 2.0) / in_rate, +...), fmScaling = 1.0f / (rfBW / (Real) in_rate),
                             * squelch counter cap rfBW / 10, open above rfBW / 20 */
    float   af_bandwidth;   /* m_afBandwidth: m_interpolator.create(16, in_rate, afBW) */
    float   volume;         /* m_volume */
    float   squelch_db;     /* m_squelch: m_squelchLevel = pow(10.0, squelch / 10.0) */
    int32_t audio_mute;     /* m_audioMute */
} sdrx_wfm_cfg;
int sdrx_wfm_create(sdrx_wfm_t** out, int device, int32_t n_ch, const sdrx_wfm_cfg* cfg);
int sdrx_wfm_destroy(sdrx_wfm_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_wfm_reset(sdrx_wfm_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to WFMDemod::feed) */
int sdrx_wfm_feed(sdrx_wfm_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_wfm_feed_dev(sdrx_wfm_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank: the readers
 * of the samples wait for the bank's stream, and the bank's stream waits until they have consumed the samples */
int sdrx_wfm_feed_bank(sdrx_wfm_t* h, sdrx_chan_bank_t* bank);
/* audio of the last feed for channel ch; returns the number of samples written (<0: error) */
int64_t sdrx_wfm_read(sdrx_wfm_t* h, int32_t ch, int16_t* audio, int64_t cap);
/* device-side view of the same (valid until the next feed) */
int sdrx_wfm_last_dev(sdrx_wfm_t* h, int32_t ch, const int16_t** d_audio, int64_t* n);
/* m_squelchOpen after the last feed: 1 / 0 (<0: error) */
int sdrx_wfm_squelch_open(sdrx_wfm_t* h, int32_t ch);
/* m_magsqSum / m_magsqPeak / m_magsqCount of getMagSqLevels; reset != 0 zeroes them as getMagSqLevels does.
 * peak and count are exact; sum is a parallel double reduction (relative difference <= 2 * count * 2^-53) */
int sdrx_wfm_levels(sdrx_wfm_t* h, int32_t ch, double* sum, double* peak, int64_t* count, int reset);
/* design products, for inspection: polyphase taps [16][ntaps], filter spectrum (1024 complex), NCO increment, m_squelchLevel */
int sdrx_wfm_get_design(sdrx_wfm_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* filter_iq, int32_t* nco_inc, float* squelch_level);
int sdrx_wfm_sync(sdrx_wfm_t* h);
int sdrx_wfm_set_stream(sdrx_wfm_t* h, void* hip_stream);
int sdrx_wfm_get_stream(sdrx_wfm_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels */
int sdrx_wfm_set_timing(sdrx_wfm_t* h, int enabled);
int sdrx_wfm_get_timing(sdrx_wfm_t* h, double* total_ms, int64_t* feeds, int reset);
/* the filter-block kernel of the last feed (the feed's largest launch): wfm_fft_kernel, its grid, block and LDS bytes */
int sdrx_wfm_last_launch(const sdrx_wfm_t* h, char* kernel_name, int name_cap,
                         int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * Broadcast-FM stereo demodulator bank: BFMDemod::feed (plugins/channelrx/demodbfm/bfmdemod.cpp:116-281) with m_rdsActive
 * clear, N channels per handle, each fed with int16 I/Q at the channelizer's output rate:
 *     Complex c(re / SDR_RX_SCALEF, im / SDR_RX_SCALEF); c *= m_nco.nextIQ();      NCO (sdrbase/dsp/nco.cpp:30-64)
 *     rf_out = m_rfFilter->runFilt(c, &rf);                                         fftfilt 1024 at the CHANNEL rate
 *     per rf[i]: msq = re*re + im*im (not divided by the scale) + level sums, squelch counter, phaseDiscriminator
 *                (conj(m_m1Sample) * sample, atan2f, / M_PI * m_fmScaling) only while the squelch is open: m_m1Sample is
 *                the last OPEN sample and survives closed stretches and feeds;
 *                audio_stereo: m_pilotPLL.process(demod, ...) on every sample (RDSPhaseLock, phaselock.cpp:253-367),
 *                m_interpolatorStereo.decimate on (demod * p[1], demod * p[2]) (lsb_stereo) or (demod * 1.17 * p[1], 0);
 *                m_interpolator.decimate on Complex(demod, 0); the two LowPassFilterRC on ci + / - sampleStereo (mono: X on
 *                ci alone); (qint16)(deemph * (1 << 12) * volume) into .l and .r
 * Outputs: interleaved l, r qint16 audio, and the Samples of m_sampleBuffer (what the reference hands its spectrum sink):
 * Sample(demod * SDR_RX_SCALEF, 0) per filtered sample when show_pilot is clear, Sample(m_pilotPLLSamples[1] * SDR_RX_SCALEF, 0)
 * when show_pilot and audio_stereo are set, nothing when show_pilot is set alone.  Both are bit-identical to the strict-IEEE
 * scalar reference build on a glibc >= 2.28 x86-64 host with FMA (the loop feeds back that libm's sinf / cosf, which are
 * restated bit for bit; atan2f is the fdlibm routine glibc had up to 2.40).  Any feed length is valid; NCO phase, pending
 * samples, ovlbuf, squelch counter, m_m1Sample, the pilot loop, both resampler windows and the distance, both de-emphasis
 * filters and the level accumulators carry across feeds.
 * RDS (m_rdsActive) is per channel through sdrx_bfmrds_create, below: the 57 kHz mixer, m_interpolatorRDS, RDSDemod::process and
 * RDSDecoder::frameSync run on the device; the interface ends at groups.
 * NOT reproduced: RDSParser (strings, tables), m_lowpass (created but never run by feed).  A channel is configured at creation;
 * there is no mid-stream retune.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_bfm sdrx_bfm_t;
typedef struct sdrx_bfm_cfg {
    int32_t in_rate;        /* channelizer output rate (m_inputSampleRate): the pilot loop, m_fmScaling = in_rate / 750000.0f */
    int32_t nco_freq;       /* m_nco.setFreq(nco_freq, in_rate): the demod passes -frequencyOffset */
    int32_t audio_rate;     /* m_audioSampleRate; <= in_rate; de-emphasis time constant 50.0 * audio_rate * 1.0e-6 */
    float   rf_bandwidth;   /* m_rfBandwidth: create_filter(-(rfBW / 2.0) / in_rate, +...), squelch cap rfBW / 10, open above rfBW / 20 */
    float   af_bandwidth;   /* m_afBandwidth: both Interpolators' create(16, in_rate, afBW) */
    float   volume;         /* m_volume */
    float   squelch_db;     /* m_squelch: m_squelchLevel = pow(10.0, squelch / 10.0) */
    int32_t audio_stereo;   /* m_audioStereo: 0 / 1 */
    int32_t lsb_stereo;     /* m_lsbStereo: 0 / 1 */
    int32_t show_pilot;     /* m_showPilot: 0 / 1 */
} sdrx_bfm_cfg;
/* SDRX_EINVAL with a text that names the field, before the device is touched */
int sdrx_bfm_create(sdrx_bfm_t** out, int device, int32_t n_ch, const sdrx_bfm_cfg* cfg);
int sdrx_bfm_destroy(sdrx_bfm_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_bfm_reset(sdrx_bfm_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to BFMDemod::feed) */
int sdrx_bfm_feed(sdrx_bfm_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_bfm_feed_dev(sdrx_bfm_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_wfm_feed_bank */
int sdrx_bfm_feed_bank(sdrx_bfm_t* h, sdrx_chan_bank_t* bank);
/* audio of the last feed for channel ch as l, r pairs; cap and the return value count pairs (<0: error) */
int64_t sdrx_bfm_read(sdrx_bfm_t* h, int32_t ch, int16_t* audio_lr, int64_t cap);
/* device-side view of the same (valid until the next feed); n counts pairs */
int sdrx_bfm_last_dev(sdrx_bfm_t* h, int32_t ch, const int16_t** d_audio_lr, int64_t* n);
/* the sink stream of the last feed as (re, im) Samples, im = 0; returns the number of Samples written */
int64_t sdrx_bfm_read_sink(sdrx_bfm_t* h, int32_t ch, int16_t* samples_iq, int64_t cap_samples);
int sdrx_bfm_sink_last_dev(sdrx_bfm_t* h, int32_t ch, const int16_t** d_samples_iq, int64_t* n_samples);
/* the pilot loop after the last feed: locked(), get_pilot_level(), the bits of m_freq and m_phase (any pointer may be null) */
int sdrx_bfm_pilot(sdrx_bfm_t* h, int32_t ch, int32_t* locked, float* level, uint32_t* freq_bits, uint32_t* phase_bits);
/* whether m_squelchState is above rfBW / 20 after the last feed: 1 / 0 (<0: error) */
int sdrx_bfm_squelch_open(sdrx_bfm_t* h, int32_t ch);
/* m_magsqSum / m_magsqPeak / m_magsqCount of getMagSqLevels; reset != 0 zeroes them as getMagSqLevels does.
 * peak and count are exact; sum is a parallel double reduction (relative difference <= 2 * count * 2^-53) */
int sdrx_bfm_levels(sdrx_bfm_t* h, int32_t ch, double* sum, double* peak, int64_t* count, int reset);
/* design products, for inspection: as sdrx_wfm_get_design, then the pilot loop's m_minfreq, m_maxfreq, m_phasor_b0, m_phasor_a1,
 * m_phasor_a2, m_loopfilter_b0, m_loopfilter_b1 (pll7), m_lock_delay, and LowPassFilterRC's m_b0, m_a1 (rc2) */
int sdrx_bfm_get_design(sdrx_bfm_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* filter_iq, int32_t* nco_inc, float* squelch_level, float* pll7, int32_t* lock_delay, float* rc2);
int sdrx_bfm_sync(sdrx_bfm_t* h);
int sdrx_bfm_set_stream(sdrx_bfm_t* h, void* hip_stream);
int sdrx_bfm_get_stream(sdrx_bfm_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels */
int sdrx_bfm_set_timing(sdrx_bfm_t* h, int enabled);
int sdrx_bfm_get_timing(sdrx_bfm_t* h, double* total_ms, int64_t* feeds, int reset);
/* the kernel that bounds the last feed: bfm_walk_kernel with a stereo channel in the handle (bfm_walk_rds_kernel when one of them
 * has RDS on), else bfm_fft_kernel */
int sdrx_bfm_last_launch(const sdrx_bfm_t* h, char* kernel_name, int name_cap,
                         int* grid, int* block, int* lds_bytes);

/* RDS of the same bank: BFMDemod::feed with m_rdsActive set (bfmdemod.cpp:169-187).  Per filtered sample, in front of that
 * sample's pilot step:
 *     Complex r(demod * 2.0 * std::cos(3.0 * m_pilotPLLSamples[3]), 0.0);     [3] is m_phase as the PREVIOUS sample's step found
 *                                                                             it: 0 at first, carried across feeds, never
 *                                                                             written in a mono channel (r = demod * 2.0)
 *     m_interpolatorRDS.decimate(...)        create(4, in_rate, 600.0): 4 phases of 18 taps, distance (Real) in_rate / 250000.0;
 *                                            with in_rate < 250000 the remainder goes negative, every input yields an output at
 *                                            phase 0 (doInterpolate's clamp): reproduced, not refused
 *     m_rdsDemod.process(cr.real(), bit)     rdsdemod.cpp:73-197, m_srate fixed at 250000
 *     m_rdsDecoder.frameSync(bit)            rdsdecoder.cpp:50-261; a completed group is four 16-bit blocks
 * Bits, groups, reports and the whole carried state are bit-identical to the strict-IEEE scalar reference build, with one
 * reservation that cannot be removed by restating: the mixer calls the host libm's double cos, which is not correctly rounded.
 * The device uses a cosine of its own whose error is argued to stay below 1 ulp and measured at 0.82 ulp (sdrangel_amd/csrc/rds_mix.hpp); glibc documents 1 ulp for
 * its own, so the two differ by one ulp at most.  For every sample the device also evaluates r at both ends of that enclosure and
 * counts the sample in the channel's `unsure` counter when they give another float.  A stream whose counter stays 0 has, given
 * those two bounds, mixed exactly as the reference on any libm that keeps the documented one.  The expected rate is about 2^-28 per
 * sample: a stream of hours at 250 kS/s will count a few.  Each such sample MAY (not must) differ from a given host's r by one
 * float ulp; everything downstream is then no longer known to be equal, though a one-ulp change of one input of an 18-tap FIR in
 * front of a 2.4 kHz low-pass seldom changes a bit.  Mono channels have no cosine and never count.
 * RDSDemod's numsamples is an int: fewer than 2^31 RDS samples (2 h 23 min at 250 kS/s) per handle between resets.
 * These calls work on a sdrx_bfm_t and carry the prefix sdrx_bfmrds_: the set of sdrx_bfm_* entry points is pinned.
 * rds == NULL or all zeros is sdrx_bfm_create: the same kernels are launched and the outputs are the same.  A handle may mix
 * channels with RDS on and off, mono and stereo.  The calls below return SDRX_EINVAL for a channel without RDS. */
typedef struct sdrx_bfmrds_cfg {
    int32_t rds_active;     /* m_rdsActive: 0 / 1 */
} sdrx_bfmrds_cfg;
int sdrx_bfmrds_create(sdrx_bfm_t** out, int device, int32_t n_ch, const sdrx_bfm_cfg* cfg, const sdrx_bfmrds_cfg* rds);
/* the bits RDSDemod::process returned during the last feed, one per byte; at most n_rds / 8 + 2 (<0: error) */
int64_t sdrx_bfmrds_read_bits(sdrx_bfm_t* h, int32_t ch, uint8_t* bits, int64_t cap);
int sdrx_bfmrds_bits_last_dev(sdrx_bfm_t* h, int32_t ch, const uint8_t** d_bits, int64_t* n);
/* the groups RDSDecoder::frameSync completed during the last feed, four blocks each; at most bits / 26 + 1 (<0: error) */
int64_t sdrx_bfmrds_read_groups(sdrx_bfm_t* h, int32_t ch, uint16_t* blocks4, int64_t cap_groups);
int sdrx_bfmrds_groups_last_dev(sdrx_bfm_t* h, int32_t ch, const uint16_t** d_blocks4, int64_t* n_groups);
/* m_parms.subcarr_bb[0] of every RDS sample of the last feed (the 2.4 kHz low-pass's output), for inspection */
int64_t sdrx_bfmrds_read_bb(sdrx_bfm_t* h, int32_t ch, float* subcarr_bb, int64_t cap);
/* RDSDemod::m_report (qua is NaN until an error was counted: 0.0 / 0 * 100), RDSDecoder::m_qua and synced() */
int sdrx_bfmrds_report(sdrx_bfm_t* h, int32_t ch, float* acc, float* qua, float* fclk, float* decoder_qua, int32_t* synced);
/* the carried state after the last feed; floats and doubles as their bits */
typedef struct sdrx_bfmrds_state_s {
    uint64_t subcarr_phi, clock_offset, clock_phi, prev_clock_phi, d_cphi;      /* m_parms' doubles */
    uint32_t xv[3], yv[3];                                                      /* m_xv[0], m_yv[0] */
    uint32_t prev_bb, acc, prev_acc, lo_clock, prev_lo_clock;
    int32_t  numsamples, counter, reading_frame, tot_errs[2], dbit;
    uint32_t distance_remain;                                                   /* m_interpolatorRDSDistanceRemain */
    uint32_t mix_phase;                                                         /* m_pilotPLLSamples[3] */
    int32_t  n_rds;                                                             /* RDS samples of the last feed */
    uint64_t reg, lastseen_offset_counter, bit_counter;                         /* RDSDecoder's members */
    uint32_t block_bit_counter, wrong_blocks_counter, blocks_counter, group_good_blocks_counter;
    uint32_t group[4];
    int32_t  sync, presync, lastseen_offset, block_number, group_assembly_started, good_block;
    uint32_t decoder_qua;
    int32_t  reserved;
} sdrx_bfmrds_state_t;
int sdrx_bfmrds_state(sdrx_bfm_t* h, int32_t ch, sdrx_bfmrds_state_t* out);
/* samples since creation, reset or the last call with reset != 0 whose r the enclosure does not pin (see above); <0: error */
int64_t sdrx_bfmrds_unsure(sdrx_bfm_t* h, int32_t ch, int reset);

/* ------------------------------------------------------------------------------------------
 * AM demodulator bank: AMDemod::feed and AMDemod::processOneSample (plugins/channelrx/demodam/amdemod.cpp:101-276), N channels
 * per handle, each fed with int16 I/Q at the channelizer's output rate.  In envelope mode (m_pll = false, the default;
 * synchronous AM: sdrx_am_create_ex, below):
 *     c = Complex(re, im) * m_nco.nextIQ();  m_interpolator.decimate(&dist, c, &ci)        as sdrx_backend_* (filt_mode 0)
 *     per ci: magsq = re*re + im*im (re = ci.re / 32768.0f); m_movingAverage(magsq) (MovingAverageUtil<Real, double, 16>);
 *             level sums; m_squelchDelayLine.write(magsq); squelch counter against m_magsq, cap rate / 10, open at rate / 20
 *     open and not muted: demod = sqrt(readBack(rate / 20)); m_volumeAGC.feed(demod) (SimpleAGC, rate / 10 entries of 0.003f);
 *             demod = (demod - agc) / agc; [m_bandpass.filter(demod) / 301.0f]; attack = (count - 0.05f * rate) / (0.05f * rate);
 *             (qint16)(demod * smootherstep(attack) * (rate / 24) * volume);   closed or muted: 0
 * The state of a fresh handle is the state after start(): distanceRemain = 0, so the first input already emits an output.
 * Output: mono qint16 audio, the value the reference writes to .l and .r, bit-identical to the strict-IEEE scalar reference
 * build.  Any feed length is valid (0 included); NCO phase, resampler window and distance, moving average, delay line,
 * counter, AGC history, Bandpass ring and level accumulators carry across feeds.
 *   - the delay line's contents start at 0.  DoubleBufferFIFO allocates with new T[] and does not clear, so a squelch that
 *     is above its level from the very first output opens at audio index rate / 20 - 1 and reads one slot that was never
 *     written; with 0 there the root is 0, the AGC is not fed and that sample is 0
 *   - left out: the interpolating branch (audio_rate > in_rate: SDRX_EINVAL), AudioFifo, and mid-stream retune or mode
 *     change -- a channel is configured at creation
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_am sdrx_am_t;
typedef struct sdrx_am_cfg {
    int32_t in_rate;          /* channelizer output rate (m_inputSampleRate) */
    int32_t nco_freq;         /* m_nco.setFreq(nco_freq, in_rate): the demod passes -frequencyOffset */
    int32_t audio_rate;       /* m_audioSampleRate; 1000 <= audio_rate <= in_rate; distance = (Real) in_rate / (Real) audio_rate */
    float   rf_bandwidth;     /* m_rfBandwidth: m_interpolator.create(16, in_rate, rfBW / 2.2f), m_bandpass.create(301, audio_rate, 300.0, rfBW / 2.0f) */
    float   volume;           /* m_volume */
    float   squelch_db;       /* m_squelch: m_squelchLevel = pow(10.0, squelch / 10.0) */
    int32_t audio_mute;       /* m_audioMute */
    int32_t bandpass_enable;  /* m_bandpassEnable */
} sdrx_am_cfg;
int sdrx_am_create(sdrx_am_t** out, int device, int32_t n_ch, const sdrx_am_cfg* cfg);
int sdrx_am_destroy(sdrx_am_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_am_reset(sdrx_am_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to AMDemod::feed) */
int sdrx_am_feed(sdrx_am_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_am_feed_dev(sdrx_am_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_am_feed_bank(sdrx_am_t* h, sdrx_chan_bank_t* bank);
/* audio of the last feed for channel ch; returns the number of samples written (<0: error) */
int64_t sdrx_am_read(sdrx_am_t* h, int32_t ch, int16_t* audio, int64_t cap);
/* device-side view of the same (valid until the next feed) */
int sdrx_am_last_dev(sdrx_am_t* h, int32_t ch, const int16_t** d_audio, int64_t* n);
/* m_squelchOpen after the last feed: 1 / 0 (<0: error) */
int sdrx_am_squelch_open(sdrx_am_t* h, int32_t ch);
/* magsq: m_magsq, the 16-sample moving average after the last sample; sum / peak / count: m_magsqSum / m_magsqPeak /
 * m_magsqCount of getMagSqLevels, zeroed by reset != 0 as getMagSqLevels does.  magsq, peak and count are exact; sum is a
 * parallel double reduction (relative difference <= 2 * count * 2^-53) */
int sdrx_am_levels(sdrx_am_t* h, int32_t ch, double* magsq, double* sum, double* peak, int64_t* count, int reset);
/* design products, for inspection: polyphase taps [16][ntaps], the 151 folded Bandpass taps, NCO increment, m_squelchLevel */
int sdrx_am_get_design(sdrx_am_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                       float* bandpass_taps, int32_t* nco_inc, float* squelch_level);
int sdrx_am_sync(sdrx_am_t* h);
int sdrx_am_set_stream(sdrx_am_t* h, void* hip_stream);
int sdrx_am_get_stream(sdrx_am_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_am_set_timing(sdrx_am_t* h, int enabled);
int sdrx_am_get_timing(sdrx_am_t* h, double* total_ms, int64_t* feeds, int reset);
/* the output kernel of the last feed (Bandpass, attack, conversion): am_out_kernel, its grid, block and LDS bytes */
int sdrx_am_last_launch(const sdrx_am_t* h, char* kernel_name, int name_cap,
                        int* grid, int* block, int* lds_bytes);

/* Synchronous AM (m_pll, amdemod.cpp:191-238).  The levels, the squelch counter and m_squelchOpen are as above; an open, unmuted
 * sample of a channel with pll != 0 then goes through
 *     s = m_pllFilt.filter(complex(re, im))   Lowpass<std::complex<float>>, create(101, audio_rate, 200.0)
 *     m_pll.feed(s.real(), s.imag())          PhaseLockComplex, computeCoefficients(0.05, 0.707, 1000), setSampleRate(audio_rate), order 1
 *     cs = (re * getImag() - im * getReal(), re * getReal() + im * getImag())         the UNfiltered sample, turned
 *     DSB: DSBFilter->runDSB(cs, &sb, false)  fftfilt((2.0f * rfBW) / audio_rate, 2048): blocks of 1024, DC bin zeroed
 *     USB / LSB: SSBFilter->runSSB(cs, &sb, usb, false)   fftfilt(0.0f, ssb_design_bw / ssb_design_rate, 1024): blocks of 512
 *     per output of a completed block: m_syncAMBuff[i] = z.real() + z.imag(), z = sb[i] * (float) m_syncAMAGC.feedAndGetValue(sb[i]),
 *         MagAGC(12000, 0.1, 1e-2), threshold off, resize(audio_rate / 4, audio_rate / 8, 0.1); m_syncAMBuffIndex = 0
 *     demod = m_syncAMBuff[m_syncAMBuffIndex++] * 4.0f;   then the optional Bandpass, the attack, the volume and the conversion
 * as in envelope mode; m_volumeAGC is not fed.  The whole chain advances on open, unmuted samples only and stands still
 * otherwise: the filter's ring, the loop, the block being filled, ovlbuf, the AGC history and the buffer index carry across
 * closures and across feeds, which may end anywhere, inside a block included.  Audio is bit-identical to the strict-IEEE
 * scalar reference build linked against a glibc whose sinf / cosf / atan2f are the ones pll_math.hpp and udpsrc_scan.hpp restate.
 *   - SSBFilter is designed once, in AMDemod's constructor, from m_rfBandwidth and m_audioSampleRate of that moment, and never
 *     again; only DSBFilter follows rf_bandwidth and audio_rate.  ssb_design_rate / ssb_design_bw carry those two values
 *   - m_syncAMBuff is never initialised by the reference; here it starts at 0.0f, which is what the first B - 1 open samples
 *     of a channel read (B the block length), as the never-written delay-line slots above
 *   - sync == NULL, or pll == 0 in every channel, is sdrx_am_create: such a handle launches the envelope kernels and no others.
 *     Channels of one handle may mix envelope and the three operations; an envelope channel of a mixed handle gives the audio
 *     of sdrx_am_create bit for bit */
typedef struct sdrx_am_sync_cfg {
    int32_t pll;              /* m_pll */
    int32_t sync_op;          /* m_syncAMOperation: 0 DSB, 1 USB, 2 LSB */
    int32_t ssb_design_rate;  /* m_audioSampleRate when AMDemod was constructed; 0 = 48000 */
    float   ssb_design_bw;    /* m_rfBandwidth then; 0 = 5000 (AMDemodSettings::resetToDefaults) */
} sdrx_am_sync_cfg;
int sdrx_am_create_ex(sdrx_am_t** out, int device, int32_t n_ch, const sdrx_am_cfg* cfg, const sdrx_am_sync_cfg* sync);
/* getPllLocked() and getPllFrequency() after the last feed (an envelope channel: 0 and 0.0f) */
int sdrx_am_pll(sdrx_am_t* h, int32_t ch, int32_t* locked, float* freq);
/* design products of a sync channel, for inspection: the 51 folded m_pllFilt taps, the frequency-domain filter in use
 * (filter_len complex bins as re, im pairs: 2048 for DSB, 1024 for USB / LSB; room for 2048) and m_pll's a1, a2, b0, b1, b2 */
int sdrx_am_get_sync_design(sdrx_am_t* h, int32_t ch, float* pll_filt_taps, float* filter_iq, int32_t* filter_len, float* pll_coef5);

/* ------------------------------------------------------------------------------------------
 * NFM demodulator bank: NFMDemod::feed (plugins/channelrx/demodnfm/nfmdemod.cpp:140-332), N channels per handle, each fed with
 * int16 I/Q at the channelizer's output rate.  With the power squelch (CTCSS and the AF squelch: sdrx_nfm_create_ex, below):
 *     c = Complex(re, im) * m_nco.nextIQ();  m_interpolator.decimate(&dist, c, &ci)        as sdrx_backend_* (filt_mode 0)
 *     per ci: demod = m_phaseDiscri.phaseDiscriminatorDelta(ci, magsqRaw, dev); magsq = (Real)(magsqRaw / 2^30);
 *             m_movingAverage(magsq) (MovingAverageUtil<Real, double, 32>); level sum, peak, count;
 *             below = (Real) m_movingAverage < m_squelchLevel; m_squelchDelayLine.write(below ? 0 : demod * m_discriCompensation);
 *             counter-- down to 0 when below, ++ up to 2 * m_squelchGate otherwise; open = counter > m_squelchGate
 *     muted: 0;  open: (qint16)(m_bandpass.filter(m_squelchDelayLine.readBack(m_squelchGate)) * volume);  closed: 0
 * The Bandpass (301 taps, 300 Hz .. af_bandwidth at the audio rate) advances on open, unmuted samples only.
 * Output: mono qint16 audio, the value the reference writes to .l and .r, bit-identical to the strict-IEEE scalar reference
 * build.  Any feed length is valid (0 included); NCO phase, resampler window and distance, m_prevArg, moving average, delay
 * line, counter, Bandpass ring and level accumulators carry across feeds.
 * A fresh handle is the object constructed with the audio device at audio_rate, after applySettings(settings, true) and
 * start():
 *   - m_phaseDiscri.setFMScaling((8.0f * audio_rate) / (float) fm_deviation)
 *   - m_discriCompensation = audio_rate / 48000.0f, times its own (Real) square root (nfmdemod.cpp:82-83)
 *   - m_squelchGate = (audio_rate / 100) * squelch_gate;  m_squelchLevel = (Real) pow(10.0, squelch / 100.0)
 *   - distanceRemain = 0 (the first input already emits an output), counter 0, moving average empty
 *   - m_prevArg starts at 0 (PhaseDiscriminators has no initialiser for it; as sdrx_audiotail_*)
 *   - the delay line has the constructor's 24000 entries, contents 0 (DoubleBufferFIFO allocates with new T[] and does not
 *     clear; applyAudioSampleRate's resize(rate / 2) is not on this path)
 *   - readBack clamps its delay to the line's size, and at delay == size the slot it names is the one just written: for
 *     m_squelchGate >= 24000 the Bandpass is given the current sample, not one 24000 back
 *   - left out: AudioFifo, the interpolating branch (audio_rate > in_rate: SDRX_EINVAL), mid-stream retune -- a channel is
 *     configured at creation -- and applyAudioSampleRate's low-rate AF tones and delay-line resize
 * AF squelch (m_deltaSquelch, sdrx_nfm_create_ex; sdrbase/dsp/afsquelch.cpp, all in double).  The squelch source of a sample is then
 *     if (m_afSquelch.analyze(demod * comp)) { m_afSquelchOpen = m_afSquelch.evaluate();
 *                                              if (!m_afSquelchOpen) m_squelchDelayLine.zeroBack(audio_rate / 10); }
 *     up = m_afSquelchOpen;   write(up ? demod * comp : 0), counter, open, readBack as above.
 *   The 32-sample power average still runs, for sdrx_nfm_levels.  Without delta_squelch the AF squelch is never called.
 *   - the constructor's setCoefficients(audio_rate / 2000, 600, audio_rate, 200, 0, {1000.0, 6000.0}): each tone capped at 0.4 *
 *     audio_rate, coef = 2.0 * cos((2.0 * M_PI * tone) / (double) rate); applySettings then sets m_squelchLevel = (Real)((-squelch)
 *     / 1000.0) ("negative millis"), the threshold to its double, and calls reset()
 *   - analyze is feedback on every sample; a block is N + 1 samples (the test is m_samplesProcessed < m_N before the increment).
 *     At a block end feedForward computes the powers, feeds the two MovingAverage<double> (sum += value - oldest: the difference
 *     first, then one rounded add), zeroes u and calls evaluate() itself.  For the first 600 block ends analyze returns false;
 *     from then on true, and NFMDemod's evaluate() is a second one: the counter moves twice per block
 *   - the two MovingAverage histories have 128 entries, not 600: AFSquelch's constructor makes them with m_nbAvg = 128, and
 *     setCoefficients' m_movingAverages.resize(m_nTones, MovingAverage<double>(600, 0.0)) finds the vector at that size already and
 *     leaves its elements alone.  Only the warm-up count is 600 (the recorder around the class decides this)
 *   - evaluate: maxPower == 0.0 (no sum above 0) returns the old state untouched; open condition minPower / maxPower < threshold
 *     && minIndex > maxIndex: counter++ up to 200, else-- if above 200, else 0; isOpen = counter >= 200
 *   - zeroBack zeroes ONE of the two copies the delay line keeps of each element, m_data[cur + size - i] for i < min(reach, size):
 *     a read returns 0 or the written value depending on the laps the write, the event and the read fall in.  The line is kept
 *     as the class keeps it, both copies and the write position carried across feeds
 * CTCSS (m_ctcssOn, sdrx_nfm_create_ex).  Per audio sample m_sampleCount++ comes first, muted or not.  Then, unmuted:
 *     open:   ctcss_sample = m_lowpass.filter(demod * m_discriCompensation)    the current, undelayed sample, every open sample
 *             if ((m_sampleCount & 7) == 7 && m_ctcssDetector.analyze(&ctcss_sample))        at every audio rate
 *                 m_ctcssIndex = toneDetected ? maxPowerIndex + 1 : 0
 *             m_ctcssIndexSelected && m_ctcssIndexSelected != m_ctcssIndex: 0, and the Bandpass does not advance;  else as above
 *     closed: m_ctcssIndex = 0; the detector's partial block and samplesProcessed stay
 *   a muted channel runs none of it: the detector, both FIRs and m_ctcssIndex stand still.
 *   - m_lowpass.create(301, audio_rate, 250.0); m_ctcssDetector.setCoefficients(audio_rate / 16, audio_rate / 8.0f): N =
 *     audio_rate / 16, the detector's rate is the float quotient cut to int, coef[j] = (Real)(2.0 * cos((2.0 * M_PI * (double)
 *     toneSet[j]) / (double) rate)) for the 32 EIA tones of the constructor, computed once on the host
 *   - feedback: u0 = (in + (coef * u0)) - u1;  feedForward: power = ((u0 * u0) + (u1 * u1)) - ((coef * u0) * u1), u0 = u1 = 0;
 *     evaluatePower: float sum over j = 0..31 in order, the first strict maximum above 0, toneDetected = maxPower > sum / 32 + 2.0f
 *   - u0, u1 and power start at 0 (CTCSSDetector allocates them with new Real[] and NFMDemod never calls its reset())
 *   - of m_sampleCount only the low three bits are carried
 *   The audio, m_ctcssIndex, its changes and the detector's powers are bit-identical to the strict-IEEE scalar reference build.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_nfm sdrx_nfm_t;
typedef struct sdrx_nfm_cfg {
    int32_t in_rate;          /* channelizer output rate (m_inputSampleRate) */
    int32_t nco_freq;         /* m_nco.setFreq(nco_freq, in_rate): the demod passes -frequencyOffset */
    int32_t audio_rate;       /* m_audioSampleRate; 1000 <= audio_rate <= in_rate; distance = (Real) in_rate / (Real) audio_rate */
    float   rf_bandwidth;     /* m_rfBandwidth: m_interpolator.create(16, in_rate, rfBW / 2.2f); 0 < rfBW <= 1e7 */
    float   af_bandwidth;     /* m_afBandwidth: m_bandpass.create(301, audio_rate, 300.0, afBW); 300 < afBW <= 1e7 */
    int32_t fm_deviation;     /* m_fmDeviation, Hz; > 0 */
    float   volume;           /* m_volume */
    float   squelch;          /* m_squelch, centi-Bels */
    int32_t squelch_gate;     /* m_squelchGate of the settings, in 10s of ms; 0 .. 1000 */
    int32_t audio_mute;       /* m_audioMute */
} sdrx_nfm_cfg;
int sdrx_nfm_create(sdrx_nfm_t** out, int device, int32_t n_ch, const sdrx_nfm_cfg* cfg);
typedef struct sdrx_nfm_tone_cfg {
    int32_t delta_squelch;   /* m_deltaSquelch: 1 = AF squelch; cfg.squelch is then "negative millis" */
    int32_t ctcss_on;        /* m_ctcssOn */
    int32_t ctcss_index;     /* m_ctcssIndex -> m_ctcssIndexSelected: 0 = any tone, 1..32 = that EIA tone */
    int32_t reserved;        /* 0 */
} sdrx_nfm_tone_cfg;
/* tone[c] goes with cfg[c]; NULL: all zero, which is sdrx_nfm_create.  Channels of one handle may mix every combination; one
 * with both options off gives the audio of sdrx_nfm_create bit for bit, and a handle with no option on in any channel launches
 * the kernels of sdrx_nfm_create and no others (a handle with an AF squelch channel adds nfm_af_walk_kernel, one with a CTCSS
 * channel three more).  Every other entry point works unchanged on such a handle. */
int sdrx_nfm_create_ex(sdrx_nfm_t** out, int device, int32_t n_ch, const sdrx_nfm_cfg* cfg, const sdrx_nfm_tone_cfg* tone);
int sdrx_nfm_destroy(sdrx_nfm_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_nfm_reset(sdrx_nfm_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to NFMDemod::feed) */
int sdrx_nfm_feed(sdrx_nfm_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_nfm_feed_dev(sdrx_nfm_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_nfm_feed_bank(sdrx_nfm_t* h, sdrx_chan_bank_t* bank);
/* audio of the last feed for channel ch; returns the number of samples written (<0: error) */
int64_t sdrx_nfm_read(sdrx_nfm_t* h, int32_t ch, int16_t* audio, int64_t cap);
/* device-side view of the same (valid until the next feed) */
int sdrx_nfm_last_dev(sdrx_nfm_t* h, int32_t ch, const int16_t** d_audio, int64_t* n);
/* m_squelchOpen after the last feed: 1 / 0 (<0: error) */
int sdrx_nfm_squelch_open(sdrx_nfm_t* h, int32_t ch);
/* magsq: m_movingAverage.asDouble(), the 32-sample moving average after the last sample; sum / peak / count: m_magsqSum /
 * m_magsqPeak / m_magsqCount of getMagSqLevels, zeroed by reset != 0 as getMagSqLevels does.  magsq, peak and count are exact;
 * sum is a parallel double reduction (relative difference <= 2 * count * 2^-53) */
int sdrx_nfm_levels(sdrx_nfm_t* h, int32_t ch, double* magsq, double* sum, double* peak, int64_t* count, int reset);
/* design products, for inspection: polyphase taps [16][ntaps], the 151 folded Bandpass taps, NCO increment, m_squelchLevel,
 * m_squelchGate in samples */
int sdrx_nfm_get_design(sdrx_nfm_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* bandpass_taps, int32_t* nco_inc, float* squelch_level, int32_t* squelch_gate);
/* m_ctcssIndex after the last feed (0: none), its tone in Hz (0 for none), and how many times it has changed since create / reset */
int sdrx_nfm_ctcss(sdrx_nfm_t* h, int32_t ch, int32_t* index, float* tone_hz, int64_t* n_changes);
/* the changes of m_ctcssIndex during the last feed, i.e. what MsgReportCTCSSFreq carries: audio sample position in the feed, new
 * index.  Returns how many there were (may exceed cap; <0: error) */
int64_t sdrx_nfm_ctcss_events(sdrx_nfm_t* h, int32_t ch, int64_t* at, int32_t* index, int64_t cap);
/* power[32] and toneDetected / maxPowerIndex of the last completed detector block (blocks completed since create / reset in
 * *n_blocks) */
int sdrx_nfm_ctcss_powers(sdrx_nfm_t* h, int32_t ch, float* power32, int32_t* detected, int32_t* max_index, int64_t* n_blocks);
/* m_afSquelchOpen after the last feed; AFSquelch's two moving-average sums and its m_squelchCount, bit-identical to the
 * reference's.  A channel without delta_squelch never calls its AFSquelch: 0, {0.0, 0.0}, 0 */
int sdrx_nfm_af_squelch(sdrx_nfm_t* h, int32_t ch, int32_t* open, double* sums2, int32_t* count);
/* design products: CTCSS N, detector rate, coef[32]; the 151 folded Lowpass taps; AF N, tones[2], coef[2], threshold -- AFSquelch as
 * the constructor's setCoefficients(audio_rate / 2000, 600, audio_rate, 200, 0, {1000.0, 6000.0}) leaves it: each tone capped at
 * 0.4 * audio_rate, coef = 2.0 * cos((2.0 * M_PI * tone) / (double) rate), threshold (double) m_squelchLevel with delta_squelch, 0.0
 * without.  sdrx_nfm_get_design's squelch_level is m_squelchLevel as the mode defines it */
int sdrx_nfm_get_tone_design(sdrx_nfm_t* h, int32_t ch, int32_t* ctcss_n, int32_t* ctcss_rate, float* coef32,
                             float* lowpass_taps, int32_t* af_n, double* af_tones2, double* af_coef2, double* af_threshold);
int sdrx_nfm_sync(sdrx_nfm_t* h);
int sdrx_nfm_set_stream(sdrx_nfm_t* h, void* hip_stream);
int sdrx_nfm_get_stream(sdrx_nfm_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_nfm_set_timing(sdrx_nfm_t* h, int enabled);
int sdrx_nfm_get_timing(sdrx_nfm_t* h, double* total_ms, int64_t* feeds, int reset);
/* the output kernel of the last feed (Bandpass, volume, conversion): nfm_out_kernel, its grid, block and LDS bytes */
int sdrx_nfm_last_launch(const sdrx_nfm_t* h, char* kernel_name, int name_cap,
                         int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * SSB / DSB demodulator bank: SSBDemod::feed (plugins/channelrx/demodssb/ssbdemod.cpp:147-285), N channels per handle, each
 * fed with int16 I/Q at the channelizer's output rate:
 *     c = Complex(re, im) * m_nco.nextIQ();  m_interpolator.decimate(&dist, c, &ci);  runSSB(ci, &sideband, usb) | runDSB
 *                                                        as sdrx_backend_* (filt_mode 2 USB, 3 LSB, 4 DSB; taps_per_phase 2.0)
 *     per sideband sample s: m_sum += s; when the pre-increment m_undersampleCount is a multiple of 1 << (span_log2 - 1):
 *             avg = m_sum / decim, m_magsq = |avg|^2 / 2^30, level sum, peak, count, one spectrum Sample (re and im swapped
 *             for LSB), m_sum = 0 -- the very first group holds one sample
 *         agcVal = agc ? m_agc.feedAndGetValue(s) : 10.0        MagAGC (sdrbase/dsp/agc.cpp:98-182), history hn, steps hn / 2
 *         x = m_squelchDelayLine.readBack(hn);  m_audioActive = x.re != 0;  m_squelchDelayLine.write(s * agcVal)
 *         muted: {0, 0};  else z = x * m_agc.getStepValue();
 *             mono: l = r = (qint16)((Real)((z.re + z.im) * 0.7) * m_volume)
 *             binaural: r = (qint16)(z.re * m_volume), l = (qint16)(z.im * m_volume); audio_flip swaps l and r
 * Output: qint16 l,r pairs and the spectrum Samples of the last feed, bit-identical to the strict-IEEE scalar reference
 * build.  The sideband stream arrives in blocks of 512 samples (DSB: 1024), so many feeds produce no audio.  Any feed length
 * is valid (0 included); NCO phase, resampler window and distance, the filter's overlap, the moving average, the four AGC
 * counters, the delay line, the open spectrum group and the level accumulators carry across feeds.
 * A fresh handle is the object constructed with the audio device at audio_rate, after applySettings(settings, true) and
 * start():
 *   - rf_bandwidth < 0 is LSB: band = -rf_bandwidth, low cutoff = -low_cutoff; band < 100 becomes 100 with a low cutoff of 0
 *   - m_interpolator.create(16, in_rate, band * 1.5f, 2.0f); create_filter(low / rate, band / rate), fftfilt length 1024;
 *     DSB: create_dsb_filter(2 * band / rate), length 2048
 *   - hn = (audio_rate / 1000) << agc_time_log2: MagAGC::resize(hn, hn / 2, agcTarget = 3276.8 as a Real), setStepDownDelay(hn);
 *     the history is 0 with sum 0 (resize, then fill(0)), m_stepUpCounter 0, m_stepDownCounter hn / 2, clampMax 327.68
 *   - hn == 12000 would skip resize() and leave the constructor's object (history filled with R, step length 2400); it needs
 *     audio_rate / 1000 in {375, 750, ...}, and audio_rate <= 192000 keeps it out of reach
 *   - setGate((audio_rate / 1000) * agc_threshold_gate); setThreshold(powerFromdB(agc_power_threshold) * 32768^2);
 *     setThresholdEnable(agc_power_threshold != -m_minPowerThresholdDB), which compares against +100 in the 16-bit build: every
 *     negative threshold enables it
 *   - m_volume = volume / 4.0
 *   - with agc = 0 the AGC is never fed, m_stepUpCounter stays 0 and getStepValue() is smootherstep(0) = 0: the audio is
 *     SILENCE (agcVal 10.0 goes into the delay line only).  The same holds with the threshold disabled, where
 *     feedAndGetValue returns m_u0 and moves no counter.  This is the reference's behaviour and is reproduced
 *   - the delay line has the constructor's 96000 entries, contents 0 (DoubleBufferFIFO allocates with new T[] and does not
 *     clear); readBack runs before this sample's write and clamps its delay to the line's size, where the slot it names is
 *     the last one written: x[j] = w[j - 1 - hn] for hn < 96000 and w[j - 1] from there on
 *   - zero input with the AGC on gives m_u0 = R / sqrt(0) = inf and 0 * inf = NaN in the delay line; (qint16) of a NaN is
 *     what x86-64 gives (0), as sdrx_audiotail_*
 *   - left out: AudioFifo, the interpolating branch (audio_rate > in_rate: SDRX_EINVAL), mid-stream retune or settings
 *     change -- a channel is configured at creation
 * SDRX_EINVAL also for hn < 2 or hn > 131072 and span_log2 outside 1 .. 8 (decim_mask is an unsigned char).
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_ssb sdrx_ssb_t;
typedef struct sdrx_ssb_cfg {
    int32_t in_rate;              /* channelizer output rate (m_inputSampleRate) */
    int32_t nco_freq;             /* m_nco.setFreq(nco_freq, in_rate): the demod passes -frequencyOffset */
    int32_t audio_rate;           /* m_audioSampleRate; 1000 <= audio_rate <= min(in_rate, 192000) */
    float   rf_bandwidth;         /* m_rfBandwidth; negative: LSB */
    float   low_cutoff;           /* m_lowCutoff; negative for LSB */
    float   volume;               /* m_volume of the settings */
    int32_t span_log2;            /* m_spanLog2, 1 .. 8: spectrum decimation 1 << (span_log2 - 1) */
    int32_t audio_binaural;       /* m_audioBinaural */
    int32_t audio_flip;           /* m_audioFlipChannels */
    int32_t dsb;                  /* m_dsb */
    int32_t audio_mute;           /* m_audioMute */
    int32_t agc;                  /* m_agc */
    int32_t agc_clamping;         /* m_agcClamping */
    int32_t agc_time_log2;        /* m_agcTimeLog2: hn = (audio_rate / 1000) << agc_time_log2, 2 .. 131072 */
    int32_t agc_power_threshold;  /* m_agcPowerThreshold, dB; +100 disables the threshold; -300 .. 300 */
    int32_t agc_threshold_gate;   /* m_agcThresholdGate, ms; 0 .. 10000 */
} sdrx_ssb_cfg;
int sdrx_ssb_create(sdrx_ssb_t** out, int device, int32_t n_ch, const sdrx_ssb_cfg* cfg);
int sdrx_ssb_destroy(sdrx_ssb_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_ssb_reset(sdrx_ssb_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to SSBDemod::feed) */
int sdrx_ssb_feed(sdrx_ssb_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_ssb_feed_dev(sdrx_ssb_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_ssb_feed_bank(sdrx_ssb_t* h, sdrx_chan_bank_t* bank);
/* audio of the last feed for channel ch as AudioSample {l, r} pairs; returns the number of PAIRS written (<0: error) */
int64_t sdrx_ssb_read(sdrx_ssb_t* h, int32_t ch, int16_t* audio_lr, int64_t cap_pairs);
/* device-side view of the same (valid until the next feed): pointer and number of pairs */
int sdrx_ssb_last_dev(sdrx_ssb_t* h, int32_t ch, const int16_t** d_audio_lr, int64_t* n_pairs);
/* the Samples {re, im} the last feed handed to the spectrum sink (m_sampleBuffer); returns their number (<0: error) */
int64_t sdrx_ssb_read_spectrum(sdrx_ssb_t* h, int32_t ch, int16_t* samples_iq, int64_t cap_samples);
int sdrx_ssb_spectrum_last_dev(sdrx_ssb_t* h, int32_t ch, const int16_t** d_samples_iq, int64_t* n_samples);
/* m_audioActive after the last feed: 1 / 0 (<0: error) */
int sdrx_ssb_audio_active(sdrx_ssb_t* h, int32_t ch);
/* magsq: m_magsq of the last closed spectrum group; sum / peak / count: m_magsqSum / m_magsqPeak / m_magsqCount of
 * getMagSqLevels, zeroed by reset != 0 as getMagSqLevels does.  magsq, peak and count are exact; sum is a parallel double
 * reduction (relative difference <= 2 * count * 2^-53) */
int sdrx_ssb_levels(sdrx_ssb_t* h, int32_t ch, double* magsq, double* sum, double* peak, int64_t* count, int reset);
/* design products, for inspection: polyphase taps [16][ntaps], the filter spectrum (2048 complex slots; 1024 used unless DSB),
 * NCO increment, hn, the gate in samples, the threshold (linear power) and m_volume */
int sdrx_ssb_get_design(sdrx_ssb_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, float* filter_iq,
                        int32_t* nco_inc, int32_t* agc_nb_samples, int32_t* agc_gate, double* agc_threshold, float* volume);
int sdrx_ssb_sync(sdrx_ssb_t* h);
int sdrx_ssb_set_stream(sdrx_ssb_t* h, void* hip_stream);
int sdrx_ssb_get_stream(sdrx_ssb_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_ssb_set_timing(sdrx_ssb_t* h, int enabled);
int sdrx_ssb_get_timing(sdrx_ssb_t* h, double* total_ms, int64_t* feeds, int reset);
/* the output kernel of the last feed (delay line, step value, volume, conversion): ssb_out_kernel, its grid, block and LDS bytes */
int sdrx_ssb_last_launch(const sdrx_ssb_t* h, char* kernel_name, int name_cap,
                         int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * ChannelAnalyzer bank: ChannelAnalyzer::feed (plugins/channelrx/chanalyzer/chanalyzer.cpp:92-182) with m_pll off, N channels
 * per handle, each fed with int16 I/Q at the channelizer's output rate; every feed produces the Samples the analyzer hands to
 * its scope / spectrum sink (m_sampleBuffer):
 *     c = Complex(re, im) * m_nco.nextIQ()                          NCOF (sdrbase/dsp/ncof.h): float phase, float increment
 *     down_sample: m_interpolator.decimate(&remain, c, &ci) -> processOneSample(ci); remain += in_rate / down_sample_rate
 *     else:        processOneSample(c)
 *     processOneSample: ssb: runSSB(c, &sideband, m_usb), length 1024; else rrc: runFilt on the root raised cosine, length 2048;
 *                       else runDSB, length 2048
 *     per filtered sample: m_sum += s; every (1 << span_log2)-th (the very first closes a group of one): m_sum /= decim,
 *         re = m_sum.real() / SDR_RX_SCALEF (likewise im), m_magsq = re*re + im*im, feedOneSample(m_sum), m_sum = 0
 *     feedOneSample: input_type 0: Sample(re, im) of m_sum, (im, re) for ssb with a negative bandwidth
 *                    input_type 2: a = m_corr->run(m_sum / (SDR_RX_SCALEF / 768.0f), 0), fftcorr(8192); Sample(a) with the same swap.
 *                        Call t = 1, 2, ... returns P_b[t mod 4096], b = t / 4096; P_0 = 0 and P_b = InverseComplexFFT(A .* conj(A)),
 *                        A the ComplexFFT of the b-th run of 4096 inputs padded with zeros to 8192: the first 4095 Samples are 0
 * Output: qint16 re,im pairs, bit-identical to the strict-IEEE scalar reference build; out of qint16's range the conversion is
 * what x86-64 gives (the autocorrelation's lag 0 is the block's energy and leaves the range for inputs above a few tens of LSB).
 * Any feed length is valid (0 included); everything carries across feeds.  A fresh handle is the object after the constructor,
 * applySettings(settings, true), applyChannelSettings(in_rate, -nco_freq) and start():
 *   - m_nco.setFreq(nco_freq, in_rate); m_interpolator.create(16, in_rate, in_rate / 2.2f), 4.5 taps per phase, distance 0
 *   - setFilters(rate, bandwidth, low_cutoff) with rate = down_sample ? down_sample_rate : in_rate: a negative bandwidth flips
 *     both signs and clears m_usb, a magnitude below 100 becomes 100 with a low cutoff of 0; create_filter(low / rate, band / rate),
 *     create_dsb_filter(band / rate), create_rrc_filter(band / rate, rrc_rolloff / 100.0)
 *   - with down_sample the last design of the root raised cosine is applySettings' own, create_rrc_filter(bandwidth / (float)
 *     down_sample_rate, rrc_rolloff / 100.0), on the bandwidth as the settings have it (no flip, no clamp)
 *   - frrc's cosine is the host's cosf
 *   - left out: m_channelPowerAvg (GUI only) and mid-stream changes of settings; the PLL, the FLL and the PLL input are
 *     sdrx_chanapll_create's (below)
 * SDRX_EINVAL for pll, fll, input_type 1 (or anything but 0 and 2), span_log2 outside 0 .. 8, rrc_rolloff outside 0 .. 100,
 * down_sample with down_sample_rate outside 1 .. in_rate, and |nco_freq| > in_rate (NCOF's wrap loops would not end).
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_chana sdrx_chana_t;
typedef struct sdrx_chana_cfg {
    int32_t in_rate;              /* channelizer output rate (m_inputSampleRate) */
    int32_t nco_freq;             /* m_nco.setFreq(nco_freq, in_rate): the analyzer passes -inputFrequencyOffset */
    int32_t down_sample;          /* m_downSample: the Interpolator is in use */
    int32_t down_sample_rate;     /* m_downSampleRate; 1 .. in_rate when down_sample */
    int32_t bandwidth;            /* m_bandwidth, Hz; negative: the lower side */
    int32_t low_cutoff;           /* m_lowCutoff, Hz */
    int32_t span_log2;            /* m_spanLog2, 0 .. 8 */
    int32_t ssb;                  /* m_ssb */
    int32_t rrc;                  /* m_rrc (used when ssb is 0) */
    int32_t rrc_rolloff;          /* m_rrcRolloff, hundredths, 0 .. 100 */
    int32_t input_type;           /* m_inputType: 0 signal, 2 autocorrelation; 1, the PLL, through sdrx_chanapll_create */
    int32_t pll;                  /* m_pll: must be 0 for sdrx_chana_create */
    int32_t fll;                  /* m_fll: must be 0 for sdrx_chana_create */
} sdrx_chana_cfg;
int sdrx_chana_create(sdrx_chana_t** out, int device, int32_t n_ch, const sdrx_chana_cfg* cfg);
int sdrx_chana_destroy(sdrx_chana_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_chana_reset(sdrx_chana_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to ChannelAnalyzer::feed) */
int sdrx_chana_feed(sdrx_chana_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_chana_feed_dev(sdrx_chana_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_chana_feed_bank(sdrx_chana_t* h, sdrx_chan_bank_t* bank);
/* the Samples {re, im} of the last feed for channel ch; returns their number (<0: error) */
int64_t sdrx_chana_read(sdrx_chana_t* h, int32_t ch, int16_t* samples_iq, int64_t cap_samples);
/* device-side view of the same (valid until the next feed): pointer and number of Samples */
int sdrx_chana_last_dev(sdrx_chana_t* h, int32_t ch, const int16_t** d_samples_iq, int64_t* n_samples);
/* what the analyzer passes as the sink's third argument: m_ssb, 1 / 0 (<0: error) */
int sdrx_chana_positive_only(sdrx_chana_t* h, int32_t ch);
/* m_magsq after the last feed, exact */
int sdrx_chana_magsq(sdrx_chana_t* h, int32_t ch, double* magsq);
/* design products, for inspection: polyphase taps [16][ntaps], the spectrum of the filter in use (2048 complex slots; 1024 used
 * with ssb), NCOF's phase increment */
int sdrx_chana_get_design(sdrx_chana_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, float* filter_iq,
                          float* nco_inc);
/* a fresh (or reset) channel whose filter has already put out `filtered_samples` samples of silence: m_undersampleCount and
 * fftcorr's call counter start from there (the oscillator and the filters start as on a fresh handle).  For streams whose
 * counters have passed 2^31: only the counter's low bits matter, and they carry as the mask sees them */
int sdrx_chana_seek(sdrx_chana_t* h, int32_t ch, uint64_t filtered_samples);
int sdrx_chana_sync(sdrx_chana_t* h);
int sdrx_chana_set_stream(sdrx_chana_t* h, void* hip_stream);
int sdrx_chana_get_stream(sdrx_chana_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_chana_set_timing(sdrx_chana_t* h, int enabled);
int sdrx_chana_get_timing(sdrx_chana_t* h, double* total_ms, int64_t* feeds, int reset);
/* chana_corr_kernel (grid = blocks x channels, 1024 threads, its LDS bytes) when a channel computes the autocorrelation, else
 * chana_group_kernel */
int sdrx_chana_last_launch(const sdrx_chana_t* h, char* kernel_name, int name_cap,
                           int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * ChannelAnalyzer bank with the PLL, the FLL and the PLL input: what sdrx_chana_create leaves out.  The handle is a
 * sdrx_chana_t and works with every sdrx_chana_* call above; sdrx_chana_create and its rejections stay as they are.
 *     per closed group, between m_magsq and feedOneSample (chanalyzer.cpp:160-178):
 *       pll & !fll: m_pll.feed(re, im), PhaseLockComplex::feed (sdrbase/dsp/phaselockcomplex.cpp:119-214): m_y = (cos, sin) of
 *                   m_phiHat; m_deltaPhi = arg(x * conj(m_y)), times m_pskOrder and normalizeAngle for an order above 1; the
 *                   v0 / v1 / v2 filter, both saturation branches, ExpAvg, the lock counters;  mix = m_sum * conj(m_y)
 *       pll &  fll: m_fll.feed(re, im), FreqLockComplex::feed (freqlockcomplex.cpp:64-80), whose m_phi is never wrapped;
 *                   mix = m_sum * conj(m_y) likewise
 *       feedOneSample(pll ? mix : m_sum, fll ? m_fll.getComplex() : m_pll.getComplex())
 *     input_type 1 (InputPLL): Sample(y.real() * SDR_RX_SCALEF, y.imag() * SDR_RX_SCALEF) of the second argument, swapped for ssb
 *       with a negative bandwidth; 32768 converts as x86-64 does, to -32768
 *     with fll set and pll clear, or input_type 1 with both clear, no loop runs and the oscillator is the unfed one, (1, 0)
 * Both loops feed their own output back, so only the very bits of the reference's cos, sin and arg keep a stream equal to the
 * reference's.  They are restated (sdrangel_amd/csrc/pll_math.hpp) and run on the device: cosf / sinf are glibc's from 2.28 to
 * 2.40 on x86-64 in the build a CPU with FMA is given (fused multiply-adds in double, rounded once), atan2f is the fdlibm float
 * routine that glibc had up to 2.40.  The bank equals a reference built strictly (-ffp-contract=off) on such a host.
 * A fresh handle is the object after the constructor, applySettings(settings, true), applyChannelSettings and start(), with what
 * that order of calls leaves behind: computeCoefficients(0.002f, 0.5f, 10.0f) once; without down_sample the last setSampleRate
 * is applyChannelSettings' (in_rate >> span_log2, the channel's own psk order); with down_sample it is applySettings' own at
 * chanalyzer.cpp:363, which divides by the span of the settings before (0) and runs before setPskOrder (m_lockFreq as of order 1).
 * psk_order[c] is m_pllPskOrder, 1 .. 31; NULL is 1 for every channel.  SDRX_EINVAL for what sdrx_chana_create rejects other than
 * pll, fll and input_type 1, and for a psk_order outside 1 .. 31.
 * sdrx_chana_last_launch names chana_walk_kernel (one wave per channel, four to a workgroup) when a channel runs a loop and
 * none computes the autocorrelation.
 * ------------------------------------------------------------------------------------------ */
int sdrx_chanapll_create(sdrx_chana_t** out, int device, int32_t n_ch, const sdrx_chana_cfg* cfg, const int32_t* psk_order);
/* isPllLocked, getPllFrequency, getPllDeltaPhase and getPllPhase after the last feed (each pointer may be NULL).  They are
 * m_pll's: with fll set they stay as a fresh PhaseLockComplex has them */
int sdrx_chanapll_state(sdrx_chana_t* h, int32_t ch, int32_t* locked, float* freq, float* delta_phi, float* phi_hat);

/* ------------------------------------------------------------------------------------------
 * UDPSrc bank: UDPSrc::feed (plugins/channelrx/udpsrc/udpsrc.cpp:136-321), N channels per handle, each fed with int16 I/Q at
 * the channelizer's output rate; every feed produces the samples UDPSrc hands to its UDPSink, i.e. the datagram payload:
 *     c = Complex(re, im) * m_nco.nextIQ();  m_interpolator.decimate(&dist, c, &ci)        as sdrx_backend_* (filt_mode 0)
 *     per ci: inMagSq = (double)(re*re + im*im);  m_inMovingAverage.feed(inMagSq / 2^30);  m_inMagsq = average();
 *             Sample((qint16) re, (qint16) im) to m_sampleBuffer (the spectrum);  calculateSquelch(m_inMagsq);
 *             one payload sample by format (open = m_squelchOpen after this sample's calculateSquelch):
 *       0 FormatIQ16         {int16, int16}  open: (qint16)(re * gain), (qint16)(im * gain); closed: 0, 0
 *       1 FormatIQ24         {int32, int32}  the same two qint16, each << 8
 *       2 FormatNFM          {int16, int16}  d = open ? m_phaseDiscri.phaseDiscriminator(ci) * gain : 0; both (int16)(d * 32768.0)
 *       3 FormatNFMMono      int16           (int16)(d * 32768.0)
 *       8 FormatAMMono       int16           (qint16)(Real)(open ? sqrt(inMagSq) * agcFactor * gain : 0)
 *       9 FormatAMNoDCMono   int16           open: r = sqrt(inMagSq); m_amMovingAverage.feed(r); (qint16)(Real)((r - average()) * agcFactor * gain)
 *      10 FormatAMBPFMono    int16           open: (qint16)(Real)(m_bandpass.filter(sqrt(inMagSq)) / 301.0 * agcFactor * gain);  closed: 0
 * The payload element is 4, 8, 4, 2, 2, 2, 2 bytes for formats 0, 1, 2, 3, 8, 9, 10 (sdrx_udpsrc_sample_bytes).
 * Formats 0, 1, 8, 9, 10, the spectrum Samples, m_inMagsq and the squelch state are bit-identical to the strict-IEEE scalar
 * reference build.  Formats 2 and 3 multiply std::arg = atan2f by fm_scaling * gain * 32768 / pi, up to several hundred times
 * 32768 at a small fm_deviation, where one ulp of the angle is more than a unit of the int16: an ulp bound against the host's libm
 * (the back-end's discri = 2 ruling) is no bound on the payload.  The device therefore evaluates the fdlibm float routines that
 * glibc's atan2f was up to 2.40, operation for operation: against a reference built on such a libm formats 2 and 3 are
 * bit-identical too; against a libm with another atan2f the angle is within 2 ulp, i.e. with |d| < 8 a payload int16 equals the
 * reference's or differs by 1 modulo 2^16.
 * Any feed length is valid (0 included); NCO phase, resampler window and distance, both moving averages, the squelch
 * counters, m_m1Sample, the Bandpass ring and the running sample count carry across feeds.
 * A fresh handle is the constructed object after applySettings(settings, true), applyChannelSettings(in_rate, offset, true)
 * and start():
 *   - m_sampleDistanceRemain starts at in_rate / output_sample_rate (a float quotient, also the step), NOT at 0 as in the
 *     demodulators: the first output appears after floor(step) inputs
 *   - the squelch starts closed with both counters 0; m_squelchGate = m_squelchRelease = (int)((output_sample_rate *
 *     squelch_gate) / 100) in float arithmetic; above = !squelch_enabled || m_inMagsq > pow(10.0, squelch_db / 10.0);
 *     gate 0 is stateless (open = above)
 *   - m_inMovingAverage has (int)(rate * 0.01) entries, m_amMovingAverage (int)(rate * 0.005), both filled with 1e-10 and
 *     a sum of size * 1e-10 (MovingAverage<double>::resize)
 *   - m_m1Sample starts at 0 (start() resets it); the discriminator runs on OPEN samples only, so m_m1Sample is the last
 *     open sample; m_phaseDiscri.setFMScaling(rate / (2.0f * fm_deviation))
 *   - m_amMovingAverage and m_bandpass (Bandpass<double>, 301 Real taps, 300 Hz .. rf_bandwidth / 2 at the output rate) are
 *     fed on open samples only; m_interpolator.create(16, in_rate, rf_bandwidth / 2.0)
 *   - the payload conversions are what x86-64 gives: float -> qint16 is cvttss2si and the low 16 bits, double -> int16_t
 *     cvttsd2si and the low 16 bits; outside the int32 range, and for NaN, both give 0
 *   - the SSB formats 4 .. 7 (FormatLSB, FormatUSB, FormatLSBMono, FormatUSBMono) need sdrx_udpsrc_create_ex with
 *     SDRX_UDPSRC_SSB_FORMATS; sdrx_udpsrc_create refuses them (SDRX_EINVAL).  Per resampled sample: ci *= agcFactor (the double
 *     narrowed to float once, two float products; 1.0 with agc off), then UDPFilter->runSSB(ci, &sideband, usb) (fftfilt.cpp:285-325)
 *     on the 512-point g_fft (bitrevR2, bfR4 with NDiffU = 2, two radix-8 stages): nothing until 256 samples are in, then 256
 *     sideband values = ovlbuf + the lower half of the filtered block; bin 0 times filter[0], bin 256 untouched, the other
 *     sideband's bins zeroed.  inptr and ovlbuf carry across feeds.  Rulings:
 *       . the filter never follows the settings: fftfilt(0.0, (12500 / 2.0) / 48000, 512) is built in the constructor from the default
 *         settings and applySettings never calls create_filter, so every channel of every handle runs the same low pass
 *         (sdrx_udpsrc_ssb_state returns it)
 *       . m_squelchGate = (int)(output_sample_rate * 0.05), a double product, whatever squelch_gate says; m_squelchRelease stays
 *         (int)((rate * squelch_gate) / 100) in float, so squelch_gate = 0 gives a release of 0 behind a gate that is not
 *       . m_squelchOpen is sampled when the block completes: the 256 elements of a block are written in the loop iteration of
 *         the sample that filled it, after that sample's calculateSquelch, and all of them use that one flag
 *       . format 4 also emits raw I/Q: its `if` is not chained to the ladder behind it, whose last branch therefore runs too.
 *         Per resampled sample, in order: the 256 LSB elements if the sample completes a block, then one element
 *         (qint16)(re * gain), (qint16)(im * gain) of the SCALED ci (0, 0 while closed).  Formats 5, 6, 7 emit the blocks only
 *       . elements: formats 4, 5 {int16, int16} = (int16)(double)(sideband.re * gain), likewise .im; formats 6, 7 int16 =
 *         (int16)((double)(re + im) * 0.7 * (double)gain); 0 while closed; 4, 4, 2, 2 bytes
 *       . agc != 0 feeds MagAGC for these formats too (udpsrc.cpp:155-163 excludes 0 .. 3 only); the spectrum Sample and inMagSq
 *         come from the unscaled ci.  Zero input with the AGC on: m_u0 = inf, 0 * inf = NaN, an all-NaN block and a NaN ovlbuf; the
 *         payload is 0 by the conversion ruling and so is every later block's
 *     read / last_dev / total count payload ELEMENTS for these formats (format 4's raw elements included); the spectrum stays one
 *     Sample per resampled sample
 *   - agc != 0 with formats 8 .. 10: agcFactor = m_agc.feedAndGetValue(ci) on EVERY sample, open or not, and inMagSq = getMagSq(),
 *     the same (double)(re*re + im*im).  MagAGC (sdrbase/dsp/agc.cpp:98-182) as UDPSrc sets it up: (9600, 16384.0f, 1e-6), clampMax
 *     2^30 with clamping on, m_squared false, the threshold enabled; resize((int)(rate / 5), (int)(rate / 20), 16384) leaves the
 *     history 0 with sum 0, m_stepUpCounter 0, m_stepDownCounter = the step length; setStepDownDelay((int)((rate * (squelch_gate ==
 *     0 ? 1 : squelch_gate)) / 100)); setGate((int)(rate * 0.05)); setThreshold(powerFromdB(squelch_db) * (1 << 23)) -- 2^23 in the
 *     16-bit build too, reproduced.  The factor multiplies the AM payload in double in front of the gain.  Zero input gives
 *     m_u0 = inf and a NaN amplitude, whose (qint16) is x86-64's 0, as in sdrx_ssb_*.  The history is as long as the rate makes it.
 *     Formats 0 .. 3 never feed the AGC; they accept and ignore the flag as the reference does
 *   - left out: m_outMovingAverage / m_magsq (GUI only), the audio return socket and AudioFifo, sockets of any kind (the
 *     caller cuts the stream into datagrams of 512 / element-size samples; sdrx_udpsrc_total gives the running count), the
 *     interpolating branch and mid-stream retune or settings change -- a channel is configured at creation
 * SDRX_EINVAL also for output_sample_rate outside 1000 .. min(in_rate, 1e7), rf_bandwidth outside (0, 1e7] (format 10: above
 * 600), fm_deviation <= 0, squelch_gate outside 0 .. 1000, squelch_db outside -300 .. 300, a non-finite gain.  (output_sample_rate >= 1000 keeps every window at 5 entries or more.)
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_udpsrc sdrx_udpsrc_t;
typedef struct sdrx_udpsrc_cfg {
    int32_t in_rate;              /* channelizer output rate (m_inputSampleRate) */
    int32_t nco_freq;             /* m_nco.setFreq(nco_freq, in_rate): UDPSrc passes -frequencyOffset */
    float   output_sample_rate;   /* m_outputSampleRate, a float in the reference; 1000 <= rate <= in_rate */
    int32_t sample_format;        /* UDPSrcSettings::SampleFormat, the reference's values: 0, 1, 2, 3, 8, 9, 10; 4 .. 7 with sdrx_udpsrc_create_ex */
    float   rf_bandwidth;         /* m_rfBandwidth */
    int32_t fm_deviation;         /* m_fmDeviation, Hz; > 0 */
    float   gain;                 /* m_gain */
    int32_t squelch_db;           /* m_squelchdB, power dB */
    int32_t squelch_gate;         /* m_squelchGate, 1/100 s; 0 .. 1000 */
    int32_t squelch_enabled;      /* m_squelchEnabled */
    int32_t agc;                  /* m_agc: MagAGC for formats 4 .. 10; ignored by formats 0 .. 3 */
} sdrx_udpsrc_cfg;
int sdrx_udpsrc_create(sdrx_udpsrc_t** out, int device, int32_t n_ch, const sdrx_udpsrc_cfg* cfg);
/* flags = 0: sdrx_udpsrc_create exactly, formats 4 .. 7 refused.  SDRX_UDPSRC_SSB_FORMATS: sample_format 4 .. 7 are accepted too.
 * Any other bit: SDRX_EINVAL. */
#define SDRX_UDPSRC_SSB_FORMATS 1u
int sdrx_udpsrc_create_ex(sdrx_udpsrc_t** out, int device, int32_t n_ch, const sdrx_udpsrc_cfg* cfg, uint32_t flags);
int sdrx_udpsrc_destroy(sdrx_udpsrc_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_udpsrc_reset(sdrx_udpsrc_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to UDPSrc::feed) */
int sdrx_udpsrc_feed(sdrx_udpsrc_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_udpsrc_feed_dev(sdrx_udpsrc_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_udpsrc_feed_bank(sdrx_udpsrc_t* h, sdrx_chan_bank_t* bank);
/* bytes of one payload sample of channel ch: 4, 8, 4, 2, 2, 2, 2 for formats 0, 1, 2, 3, 8, 9, 10 and 4, 4, 2, 2 for formats
 * 4, 5, 6, 7 (<0: error) */
int32_t sdrx_udpsrc_sample_bytes(sdrx_udpsrc_t* h, int32_t ch);
/* raw payload bytes of the last feed for channel ch; returns the number of SAMPLES written (<0: error) */
int64_t sdrx_udpsrc_read(sdrx_udpsrc_t* h, int32_t ch, void* payload, int64_t cap_samples);
/* device-side view of the same (valid until the next feed): pointer and number of samples */
int sdrx_udpsrc_last_dev(sdrx_udpsrc_t* h, int32_t ch, const void** d_payload, int64_t* n_samples);
/* the Samples {re, im} the last feed handed to the spectrum sink (m_sampleBuffer), one per resampled sample: one per payload
 * sample for formats 0 .. 3 and 8 .. 10, not for formats 4 .. 7 */
int64_t sdrx_udpsrc_read_spectrum(sdrx_udpsrc_t* h, int32_t ch, int16_t* samples_iq, int64_t cap_samples);
int sdrx_udpsrc_spectrum_last_dev(sdrx_udpsrc_t* h, int32_t ch, const int16_t** d_samples_iq, int64_t* n_samples);
/* m_squelchOpen after the last feed: 1 / 0 (<0: error); m_squelchOpenCount and m_squelchCloseCount */
int sdrx_udpsrc_squelch_open(sdrx_udpsrc_t* h, int32_t ch);
int sdrx_udpsrc_squelch_counts(sdrx_udpsrc_t* h, int32_t ch, int32_t* open_count, int32_t* close_count);
/* m_inMagsq after the last feed, exact (0 until the first output sample, as the constructor leaves it) */
int sdrx_udpsrc_in_magsq(sdrx_udpsrc_t* h, int32_t ch, double* in_magsq);
/* payload samples since creation or reset (<0: error): datagram k of the stream holds samples [k * M, (k + 1) * M), M = 512 / element size */
int64_t sdrx_udpsrc_total(sdrx_udpsrc_t* h, int32_t ch);
/* formats 4 .. 7 (SDRX_EINVAL for a channel of another format): fftfilt's inptr after the last feed, the blocks completed since
 * creation or reset, and the shared filter design (512 complex bins = 1024 floats, or NULL) */
int sdrx_udpsrc_ssb_state(sdrx_udpsrc_t* h, int32_t ch, int32_t* pending, int64_t* blocks, float* filter_iq);
/* design products, for inspection: polyphase taps [16][ntaps] and the 151 folded Bandpass taps (Reals, widened), NCO increment,
 * windows[3] = entries of m_inMovingAverage, m_amMovingAverage, m_outMovingAverage, gate and release in samples, m_squelch,
 * the discriminator's scaling, the distance step, agc_ints[4] = MagAGC's history length, step length, step-down delay and gate in
 * samples, and its threshold powerFromdB(squelch_db) * 2^23 */
int sdrx_udpsrc_get_design(sdrx_udpsrc_t* h, int32_t ch, int32_t* ntaps_per_phase, double* taps, int32_t taps_cap, double* bandpass_taps,
                           int32_t* nco_inc, int32_t* windows, int32_t* squelch_gate, int32_t* squelch_release, double* squelch_level,
                           float* fm_scaling, float* distance_step, int32_t* agc_ints, double* agc_threshold);
int sdrx_udpsrc_sync(sdrx_udpsrc_t* h);
int sdrx_udpsrc_set_stream(sdrx_udpsrc_t* h, void* hip_stream);
int sdrx_udpsrc_get_stream(sdrx_udpsrc_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_udpsrc_set_timing(sdrx_udpsrc_t* h, int enabled);
int sdrx_udpsrc_get_timing(sdrx_udpsrc_t* h, double* total_ms, int64_t* feeds, int reset);
/* the output kernel of the last feed (discriminator, averages, Bandpass, gain, conversion): udp_out_kernel, its grid, block and LDS bytes */
int sdrx_udpsrc_last_launch(const sdrx_udpsrc_t* h, char* kernel_name, int name_cap,
                            int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * LoRa demodulator bank: N LoRaDemod instances (plugins/channelrx/demodlora/lorademod.cpp, lorabits.h) on one device, the
 * 16-bit build.  Input: int16 I/Q at the channelizer's output rate.  Output per feed: the Samples LoRaDemod::feed puts into
 * m_sampleBuffer for its spectrum sink, one per decimator output, and the lines dumpRaw() prints.  Per input sample
 * c = (re / 32768, im / 32768) * m_nco.nextIQ(); m_interpolator.decimate(&dist, c, &ci) with create(16, in_rate, m_Bandwidth /
 * 1.9) -- the cutoff is the DOUBLE quotient of the float bandwidth and 1.9 -- and dist starting at (Real) in_rate / m_Bandwidth.
 * Per decimator output: the dechirp by m_chirp / m_angle, the two sliding FFTs (sfft of 128, bins 0 .. 126) over ci * a and
 * ci * conj(a), every 64th output detect()'s fetch with synch() and dumpRaw(), then m_bin += m_result and one Sample.
 * Samples, lines and state are bit for bit those of the strict-IEEE scalar build of the reference.
 *   - four places where the reference reads memory it never wrote are defined here, and identically in the recorder the
 *     fixtures come from (tests/golden/lora_rec.cpp):
 *       mov (new float[512]), read during the first four fetches, starts as zeros;
 *       mag[127] and rev[127], stack floats sfft::fetch does not write, are 0 (the magnitude of the bin that never moves);
 *       dumpRaw's char text[256], which interleave6 reads up to five characters past the last symbol, starts as zeros;
 *       m_count, an int, is kept in 64 bits and movpoint is (count >> 6) & 3: the reference's value while that is defined.
 *   - left out: the 24-bit build, and a mid-stream retune or bandwidth change -- a channel is configured at creation, a new
 *     configuration is a new handle.  bandwidth > in_rate (the interpolating branch) is SDRX_EINVAL.
 *   - at most one line ends per 71 fetches (4544 Samples): that bounds the text of a feed.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_lora sdrx_lora_t;
typedef struct sdrx_lora_cfg {
    int32_t in_rate;              /* channelizer output rate (m_sampleRate) */
    int32_t nco_freq;             /* m_nco.setFreq(nco_freq, in_rate): LoRaDemod passes -frequencyOffset */
    int32_t bandwidth;            /* m_Bandwidth: LoRaDemodSettings::bandwidths = 7813, 15625, 20833, 31250, 62500; any value in 1 .. in_rate is accepted */
} sdrx_lora_cfg;
typedef struct sdrx_lora_state_t {
    int32_t tune, time, result, bin;  /* m_tune, m_time, m_result, m_bin after the last feed */
    int64_t count;                /* m_count in 64 bits: decimator outputs since creation or reset */
    int64_t lines;                /* lines dumpRaw printed since creation or reset */
} sdrx_lora_state_t;
int sdrx_lora_create(sdrx_lora_t** out, int device, int32_t n_ch, const sdrx_lora_cfg* cfg);
int sdrx_lora_destroy(sdrx_lora_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_lora_reset(sdrx_lora_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to LoRaDemod::feed) */
int sdrx_lora_feed(sdrx_lora_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_lora_feed_dev(sdrx_lora_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_lora_feed_bank(sdrx_lora_t* h, sdrx_chan_bank_t* bank);
/* the m_sampleBuffer of the last feed for channel ch, {re, im} per Sample; returns the number of Samples written (<0: error) */
int64_t sdrx_lora_read(sdrx_lora_t* h, int32_t ch, int16_t* samples_iq, int64_t cap_samples);
/* device-side view of the same (valid until the next feed) */
int sdrx_lora_last_dev(sdrx_lora_t* h, int32_t ch, const int16_t** d_samples_iq, int64_t* n);
/* the lines dumpRaw printed during the last feed, '\n' after each, no terminating 0; returns the byte count, < 0 on error or
 * if cap is too small for them */
int64_t sdrx_lora_read_text(sdrx_lora_t* h, int32_t ch, char* buf, int64_t cap);
int sdrx_lora_state(sdrx_lora_t* h, int32_t ch, sdrx_lora_state_t* s);
/* design products, for inspection (any pointer may be NULL): polyphase taps [16][ntaps], NCO increment, sfft's vrot[128] as
 * (re, im) pairs and its k2, the dechirp table [256] as (re, im) pairs indexed by m_angle, the Sample table [128] as (re, im)
 * pairs indexed by m_bin */
int sdrx_lora_get_design(sdrx_lora_t* h, int32_t ch, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, int32_t* nco_inc,
                         float* vrot_iq, float* k2, float* chirp_iq, int16_t* sample_iq);
int sdrx_lora_sync(sdrx_lora_t* h);
int sdrx_lora_set_stream(sdrx_lora_t* h, void* hip_stream);
int sdrx_lora_get_stream(sdrx_lora_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_lora_set_timing(sdrx_lora_t* h, int enabled);
int sdrx_lora_get_timing(sdrx_lora_t* h, double* total_ms, int64_t* feeds, int reset);
/* the walk of the last feed: lora_walk_kernel, its grid, block and LDS bytes */
int sdrx_lora_last_launch(const sdrx_lora_t* h, char* kernel_name, int name_cap,
                          int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * ATV demodulator bank: N ATVDemod instances (plugins/channelrx/demodatv/atvdemod.cpp, atvdemod.h) on one device, the 16-bit
 * build.  Input: int16 I/Q at the channelizer's output rate.  Output per feed: the frames the screen was asked to render, the
 * screen as it stands, the scope stream and the state.  Per input sample c = (re, im) unscaled, times m_nco.nextIQ() exactly
 * when nco_freq is not 0 (the reference skips the mix at offset 0, and the oscillator at phase 0 is not (1, 0): its sine is a
 * rounded cos(pi / 2)); demod(c): FM1 / FM2 on the normalised sample and the 2 / 6 before it, FM3 phaseDiscriminatorDelta(c) +
 * 0.5, AM sqrt(magSq) / SDR_RX_SCALEF normalised by the extrema of the line before; inversion, clamp, the scope Sample, the grey
 * level, then processClassic or processHSkip (standard 5).  The screen is what TVScreen is to the demodulator
 * (sdrgui/gui/glshadertvarray.cpp:294-328): rows x cols bytes of grey and a current row.  Frames, events, screen, scope and
 * state are bit for bit those of the strict-IEEE scalar build of the reference.
 *   - pinned where the reference leaves it open or relies on x86, identically in tests/atv_oracle.cpp:
 *       m_intAvgColIndex, which the constructor does not initialise, starts at 0;
 *       the screen counts as initialised and starts as zeros; its current row is null until the first selectRow in range, so
 *         pixels before that are dropped, and a selectRow out of range makes it null again;
 *       a float that no int holds, NaN included, converts to INT_MIN: the grey level of a NaN is 0, and the scope Sample
 *         converts through int32 and keeps the low 16 bits (1.0f gives -32768, NaN gives 0).  FM1 / FM2 reach NaN on a (0, 0) sample;
 *       a NaN in the state (m_fltAmpLineAverage, m_fltBufferI / Q) is x86-64's default NaN 0xffc00000, the bits 0 / 0 gives there
 *         and SSE arithmetic hands on unchanged.
 *       m_DSBFilterBuffer makes the filtered stream lag by 1023 samples, with zeros first: demod reads slot index - 1 of a buffer
 *         refilled every 1024th call.  FM3 takes the UNFILTERED sample even with the filter on.  Both are kept.  With the filter
 *         on, FM1 / FM2 therefore see (0, 0) for the first 1023 samples and reach NaN there.
 *   - the "decimator" (decimator_enable): its step tvRate / in_rate is <= 1 and its distance starts at 0 and never reaches 1, so
 *     every input emits and the negative phase clamps to 0: a 72-tap FIR at the input rate, the phase-0 row of
 *     create(24, tvRate, rf_bw / 2.2f, 3.0), summed in doInterpolate's order.
 *   - left out: modulations USB and LSB (SimplePhaseLock and SecondOrderRecursiveFilter, the BFO), refused by create with
 *     SDRX_EINVAL and a text; m_objMagSqAverage (GUI only); a mid-stream reconfiguration (a new configuration is a new handle);
 *     EXTENDED_DIRECT_SAMPLE and the 24-bit build.  m_interpolatorDistanceRemain is not part of the state: no output depends on it.
 *   - a vsync can be re-armed by one sample above the level and fired by the next one below it, so a feed can render every
 *     second sample: the first frames_cap renders of a feed keep a snapshot, later ones are counted and listed only.
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_atv sdrx_atv_t;
typedef struct sdrx_atv_cfg {
    int32_t in_rate;              /* channelizer output rate (m_intSampleRate) */
    int32_t nco_freq;             /* m_nco.setFreq(nco_freq, in_rate): ATVDemod passes -frequencyOffset; 0: no mix */
    int32_t modulation;           /* ATVModulation: 0 FM1, 1 FM2, 2 FM3, 3 AM; 4 USB and 5 LSB are refused */
    float   rf_bw, rf_opp_bw;     /* m_fltRFBandwidth, m_fltRFOppBandwidth: read by the FFT filter and the decimator only */
    int32_t fft_filtering;        /* m_blnFFTFiltering */
    int32_t decimator_enable;     /* m_blndecimatorEnable */
    float   fm_deviation;         /* m_fmDeviation */
    float   line_duration;        /* m_fltLineDuration, seconds */
    float   top_duration;         /* m_fltTopDuration, seconds */
    float   frames_per_s;         /* m_fltFramePerS */
    int32_t standard;             /* ATVStd: 0 PAL625, 1 PAL525, 2 405, 3 ShortInterleaved, 4 Short, 5 HSkip */
    int32_t n_lines;              /* m_intNumberOfLines */
    float   level_synchro_top;    /* m_fltVoltLevelSynchroTop */
    float   level_black;          /* m_fltVoltLevelSynchroBlack, < 1 */
    int32_t hsync, vsync, invert_video;
    int32_t scope;                /* m_intVideoTabIndex == 1 with a scope sink present */
    int32_t frames_cap;           /* >= 1: renders of one feed that keep a snapshot of the screen */
} sdrx_atv_cfg;
typedef struct sdrx_atv_state_t { /* the PROCESSING block of atvdemod.h after the last feed; floats as their bits */
    int32_t image_index, synchro_points, synchro_detected, vertical_synchro_detected;
    int32_t col_index, sample_index, row_index, line_index, avg_col_index;
    int32_t screen_row;           /* the screen's current row, -1: null */
    uint32_t amp_line_average, eff_min, eff_max, amp_min, amp_max, amp_delta;
    uint32_t buffer_i[6], buffer_q[6];    /* m_fltBufferI, m_fltBufferQ */
} sdrx_atv_state_t;
typedef struct sdrx_atv_design_t { /* applySettings' and applyStandard's integers */
    int32_t samples_per_line, samples_per_top, samples_per_line_signals, samples_per_hsync;
    int32_t sync_lines, black_lines, eq_lines, interleaved;
    int32_t tv_rate;              /* m_intTVSampleRate */
    int32_t cols, rows;           /* resizeTVScreen's arguments */
    int32_t nco_inc;
} sdrx_atv_design_t;
int sdrx_atv_create(sdrx_atv_t** out, int device, int32_t n_ch, const sdrx_atv_cfg* cfg);
int sdrx_atv_destroy(sdrx_atv_t* h);
/* the state of a fresh handle with the same configuration, the screens zeroed */
int sdrx_atv_reset(sdrx_atv_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to ATVDemod::feed) */
int sdrx_atv_feed(sdrx_atv_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_atv_feed_dev(sdrx_atv_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_atv_feed_bank(sdrx_atv_t* h, sdrx_chan_bank_t* bank);
/* renderImage calls of the last feed into *n_events (may be NULL); returns how many of them kept a snapshot (<0: error) */
int64_t sdrx_atv_frames(sdrx_atv_t* h, int32_t ch, int64_t* n_events);
/* for each render of the last feed the index, within the feed, of the input sample at which it happened; returns the count written */
int64_t sdrx_atv_read_events(sdrx_atv_t* h, int32_t ch, int32_t* index, int64_t cap);
/* the screen (rows x cols bytes of grey, row after row) as it stood at render k of the last feed, k < sdrx_atv_frames();
 * returns rows * cols (<0: error, cap too small included) */
int64_t sdrx_atv_read_frame(sdrx_atv_t* h, int32_t ch, int64_t k, uint8_t* buf, int64_t cap);
/* the screen after the last feed */
int64_t sdrx_atv_read_screen(sdrx_atv_t* h, int32_t ch, uint8_t* buf, int64_t cap);
/* device-side views (valid until the next feed): the stored frames, `pitch` bytes apart, and the screen.  d_frames is the snapshot
 * arena of the last feed, NULL before the first feed, never the live screen: with n_stored 0 nothing in it is a frame */
int sdrx_atv_frames_last_dev(sdrx_atv_t* h, int32_t ch, const uint8_t** d_frames, int64_t* n_stored, int64_t* pitch);
int sdrx_atv_screen_last_dev(sdrx_atv_t* h, int32_t ch, const uint8_t** d_screen, int32_t* rows, int32_t* cols);
/* the real parts of the Samples (re, 0) of m_scopeSampleBuffer of the last feed, one per input with `scope` set, none without */
int64_t sdrx_atv_read(sdrx_atv_t* h, int32_t ch, int16_t* scope_re, int64_t cap_samples);
int sdrx_atv_last_dev(sdrx_atv_t* h, int32_t ch, const int16_t** d_scope_re, int64_t* n);
int sdrx_atv_state(sdrx_atv_t* h, int32_t ch, sdrx_atv_state_t* s);
int sdrx_atv_get_design(sdrx_atv_t* h, int32_t ch, sdrx_atv_design_t* d);
/* the rest of the design products, for inspection (any pointer may be NULL): the decimator's FIR, the phase-0 row of
 * m_interpolator.create(24, tvRate, rf_bw / 2.2f, 3.0), *ntaps of them (72; 0 without the decimator), and m_DSBFilter's filter and
 * filterOpp as 2048 (re, im) pairs each.  Returns 2048 with the FFT filter, 0 without (the arrays are then left alone), < 0 on error */
int sdrx_atv_get_filters(sdrx_atv_t* h, int32_t ch, int32_t* ntaps, float* taps, int32_t taps_cap, float* filter_iq, float* filter_opp_iq);
int sdrx_atv_sync(sdrx_atv_t* h);
int sdrx_atv_set_stream(sdrx_atv_t* h, void* hip_stream);
int sdrx_atv_get_stream(sdrx_atv_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_atv_set_timing(sdrx_atv_t* h, int enabled);
int sdrx_atv_get_timing(sdrx_atv_t* h, double* total_ms, int64_t* feeds, int reset);
/* the walk of the last feed: atv_walk_kernel, its grid, block and LDS bytes */
int sdrx_atv_last_launch(const sdrx_atv_t* h, char* kernel_name, int name_cap,
                         int* grid, int* block, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * DATV receiver bank: the sample-rate half of N DATVDemod instances (plugins/channelrx/demoddatv/datvdemod.cpp with leansdr's
 * sdr.h) on one device, the 16-bit build.  Input: int16 I/Q at the channelizer's output rate.  Per input sample
 * Complex(re, im) * m_objNCO.nextIQ() with setFreq(-centre_frequency, msps), m_objRFFilter->runFilt (fftfilt(.., 1024) with
 * create_filter(-+ rf_bandwidth / 2 / msps)), and on its 512-sample blocks cstln_receiver<f32>::run with the configured sampler,
 * a chunk of 128 samples whenever 128 + readahead are there.  Output per feed: what p_symbols (soft symbols), p_sampled (one
 * constellation point per chunk with a symbol) and p_freq / p_ss / p_mer (one measurement per meas_decimation samples) have
 * received once the scheduler has run dry, and the receiver's state.  Everything from p_symbols on (deconvolution, mpeg_sync, the
 * deinterleaver, Reed-Solomon, the derandomizer, the player) stays with the host.  Symbols, points, measurements and state are bit
 * for bit those of the strict-IEEE scalar build of the reference.
 *   - samples that do not fill a chunk, and a partial 512-block of the filter, stay in the channel: a feed of 1 sample is legal and
 *     usually returns nothing.  The output does not depend on how the stream is cut into feeds.
 *   - the tables are design, built on the host at create: trig16 (65536 (cos, sin), one copy per handle), one cstln_lut<256> per
 *     distinct (modulation, fec, hard_metric) in the handle, the RRC coefficients per channel.  Their sinf / cosf are
 *     pll_math.hpp's restatement of glibc's (also inside filtergen::root_raised_cosine, whose sqrt / sin / cos of floats are the
 *     float overloads), their atan2f is udp_atan2f (glibc 2.35's), sqrtf is IEEE: the design does not follow the machine's libm.
 *   - a measurement holds freq_tap and the three estimates as the device left them; ss = sqrtf(est_insp) and
 *     mer = est_ep ? 10 * logf(est_sp / est_ep) / logf(10) : 0 are computed inside sdrx_datv_read_meas, on the host: logf of the
 *     quotient by the calling process's libm, logf(10) as the constant the library's compiler folded it to (as the reference's is): logf
 *     is the one routine of the loop that is not correctly rounded everywhere, and it feeds nothing back.
 *   - casts.  trig16::expi(float a) is (uint16_t)(int16_t)(int32_t) a and cstln_lut::lookup casts through s8 behind its halving
 *     loop.  x86-64 converts a float that no int32 holds, NaN included, to INT_MIN, the device saturates; both agree for
 *     |a| < 2^31.  The bank converts as x86-64 does for EVERY float, so nothing hangs on the range; the loop stays inside it
 *     anyway: phase is reduced by fmodf(phase, 65536) after every chunk and moves by 128 freqw + at most 128 * 0.04 * 32768 inside
 *     one, and freqw is held within 65536 / omega / n / 2 of 0 unless allow_drift is set.  With allow_drift freqw is a sum of
 *     phase_error * freq_beta terms, |.| <= 32768 * 0.0012 each, so it takes more than 4 * 10^5 symbols of one sign to pass
 *     2^31 / 128 = 2^24, where -(phase + freqw) would leave the int32 range within a chunk; beyond that the reference's own behaviour
 *     is "undefined" (math.h) and the bank's is x86-64's.  lookup's halving loop is cut after 300 rounds, which no finite value
 *     needs; the reference spins forever on an infinity.
 *   - refused by create with SDRX_EINVAL and a text: notch_filters > 0 (auto_notch); 16APSK / 32APSK at a code rate
 *     make_dvbs2_constellation has no radii for; rolloff <= 0 with the RRC sampler (its order divides by it); an RRC with more
 *     than 4096 coefficients or more than 64 taps per symbol (ceil(ncoeffs / rrc_steps)): the walk keeps shifted_coeffs in LDS and
 *     gives a tap to a lane (the reference itself stops at 128 + readahead > 16384, BUF_BASEBAND); a meas_decimation under 64;
 *     rates that are not positive, symbol_rate > sample_rate.
 *   - left out: r_cnr (cfg.cnr is never set), m_objMagSqAverage (GUI only), the constellation screen, EXTENDED_DIRECT_SAMPLE, the
 *     24-bit build, a mid-stream reconfiguration (a new configuration is a new handle).
 * ------------------------------------------------------------------------------------------ */
typedef struct sdrx_datv sdrx_datv_t;
typedef struct sdrx_datv_cfg {
    int32_t msps;                 /* channelizer output rate (intMsps): the NCO's and the RF filter's */
    int32_t sample_rate;          /* Fs (intSampleRate; DATVDemod sets it to msps) */
    int32_t centre_frequency;     /* m_objNCO.setFreq(-centre_frequency, msps) */
    int32_t rf_bandwidth;         /* create_filter(-rf_bandwidth / 2 / msps, +rf_bandwidth / 2 / msps) */
    int32_t symbol_rate;          /* Fm */
    int32_t modulation;           /* DATVModulation: 0 BPSK, 1 QPSK, 2 8PSK, 3 16APSK, 4 32APSK, 5 64APSKe, 6 16QAM, 7 64QAM, 8 256QAM */
    int32_t fec;                  /* leansdr::code_rate: 0 1/2, 1 2/3, 2 4/6, 3 3/4, 4 5/6, 5 7/8, 6 4/5, 7 8/9, 8 9/10 */
    int32_t standard;             /* dvb_version: 0 DVB-S, 1 DVB-S2 (a warning in the reference, nothing else before p_symbols) */
    int32_t sampler;              /* dvb_sampler: 0 nearest, 1 linear, 2 RRC */
    float   rolloff;              /* fltRollOff, 0 .. 1 */
    int32_t excursion;            /* intExcursion: rrc_rej, dB */
    int32_t hard_metric;          /* cstln->harden() */
    int32_t viterbi;              /* pll_adjustment /= 6 */
    int32_t allow_drift;
    int32_t notch_filters;        /* must be 0 */
    float   finfo;                /* Finfo, Hz: meas_decimation = max(1, (int)(Fs / finfo)); 0: the reference's 5 */
} sdrx_datv_cfg;
typedef struct sdrx_datv_state_t { /* cstln_receiver's and fir_sampler's members after the last feed; floats as their bits */
    uint32_t mu, phase, freqw, agc_gain;
    uint32_t est_insp, est_sp, est_ep;
    uint32_t meas_count;
    int32_t update_freq_phase;
    uint32_t hist_p[3][2], hist_c[3][2];   /* hist[k].p and hist[k].c as (re, im) */
    int32_t held;                 /* filtered samples held back: fewer than 128 + readahead */
    int64_t chunks;               /* chunks run since creation or reset */
    int64_t n_in;                 /* filtered samples the receiver was given since creation or reset */
    int64_t n_symbols;            /* soft symbols written since creation or reset */
} sdrx_datv_state_t;
typedef struct sdrx_datv_design_t {
    float   omega, min_omega, max_omega, min_freqw, max_freqw, freq_beta;
    int32_t meas_decimation, rrc_steps, ncoeffs, readahead, nsymbols;
    int32_t nco_inc;
} sdrx_datv_design_t;
typedef struct sdrx_datv_meas_t { /* freq_out, ss_out, mer_out and the three estimates behind them */
    float freq, ss, mer;
    float est_insp, est_sp, est_ep;
} sdrx_datv_meas_t;
int sdrx_datv_create(sdrx_datv_t** out, int device, int32_t n_ch, const sdrx_datv_cfg* cfg);
int sdrx_datv_destroy(sdrx_datv_t* h);
/* the state of a fresh handle with the same configuration */
int sdrx_datv_reset(sdrx_datv_t* h);
/* iq[c] / n_per_ch[c]: channel c's new samples (what DownChannelizer handed to DATVDemod::feed) */
int sdrx_datv_feed(sdrx_datv_t* h, const int16_t* const* iq, const int64_t* n_per_ch);
/* same on device pointers (4-byte aligned), asynchronous on the handle's stream */
int sdrx_datv_feed_dev(sdrx_datv_t* h, const int16_t* const* d_iq, const int64_t* n_per_ch);
/* hand-over from a channel bank without a host round trip, ordered on the device like sdrx_backend_feed_bank */
int sdrx_datv_feed_bank(sdrx_datv_t* h, sdrx_chan_bank_t* bank);
/* the soft symbols of the last feed: softsymbol::cost and ::symbol, either array may be NULL; returns the count written (<0: error) */
int64_t sdrx_datv_read(sdrx_datv_t* h, int32_t ch, int16_t* cost, uint8_t* symbol, int64_t cap);
/* the constellation points of the last feed as (re, im) pairs: one per chunk that had a symbol; returns the count of pairs */
int64_t sdrx_datv_read_points(sdrx_datv_t* h, int32_t ch, float* iq, int64_t cap);
/* the measurements of the last feed; ss and mer are computed here, on the host */
int64_t sdrx_datv_read_meas(sdrx_datv_t* h, int32_t ch, sdrx_datv_meas_t* out, int64_t cap);
/* device-side views (valid until the next feed); any pointer may be NULL.  d_meas points at records of four floats: freq_tap,
 * est_insp, est_sp, est_ep */
int sdrx_datv_last_dev(sdrx_datv_t* h, int32_t ch, const int16_t** d_cost, const uint8_t** d_symbol, int64_t* n);
int sdrx_datv_points_last_dev(sdrx_datv_t* h, int32_t ch, const float** d_iq, int64_t* n);
int sdrx_datv_meas_last_dev(sdrx_datv_t* h, int32_t ch, const float** d_meas, int64_t* n);
int sdrx_datv_state(sdrx_datv_t* h, int32_t ch, sdrx_datv_state_t* s);
int sdrx_datv_get_design(sdrx_datv_t* h, int32_t ch, sdrx_datv_design_t* d);
/* the design's tables, for inspection (any pointer may be NULL): the RRC coefficients (returns their count, 0 without the RRC
 * sampler; at most coeffs_cap are written), trig16 as 65536 (cos, sin) pairs, the constellation table as 65536 records of 8 bytes
 * -- int16 cost, int16 phase_error, uint8 symbol, three zero bytes; record I * 256 + Q is lut[(u8) I][(u8) Q] -- and symbols[] as
 * 256 (re, im) pairs of int8, nsymbols of them set.  <0: error */
int sdrx_datv_get_tables(sdrx_datv_t* h, int32_t ch, float* coeffs, int32_t coeffs_cap, float* trig_iq, void* lut, int8_t* symbols);
int sdrx_datv_sync(sdrx_datv_t* h);
int sdrx_datv_set_stream(sdrx_datv_t* h, void* hip_stream);
int sdrx_datv_get_stream(sdrx_datv_t* h, void** hip_stream);
/* as sdrx_decim_set_timing: brackets each feed's kernels, the front's included */
int sdrx_datv_set_timing(sdrx_datv_t* h, int enabled);
int sdrx_datv_get_timing(sdrx_datv_t* h, double* total_ms, int64_t* feeds, int reset);
/* the walk of the last feed: datv_walk_kernel, its grid, block and LDS bytes */
int sdrx_datv_last_launch(const sdrx_datv_t* h, char* kernel_name, int name_cap,
                          int* grid, int* block, int* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SDRX_H */
