/*
 * ft8hip.h -- C-ABI of libft8hip.so, the MI355X (gfx950) FT8 receive path.
 *
 * Drop-in boundary for the reference's Python decoder (Rintazero/ft8_demodulator,
 * src/ft8_tools/ft8_demodulator).  The reference has no native FFI of its own: every entry point
 * below replaces one Python function on its decode path, cited as file:line relative to
 * src/ft8_tools/ft8_demodulator/.  The Python host layer (ft8_demodulator_amd/) binds these with
 * ctypes and mirrors the reference's functions, names, arguments and error behaviour.
 *
 * Conventions
 *   - All data pointers are device pointers owned by the caller (e.g. torch data_ptr()).  The
 *     library allocates scratch only inside its context and frees only what it allocated.
 *   - Every call is asynchronous on the caller's hipStream_t (passed as void*, NULL = default
 *     stream).  Results are valid after the stream is synchronised.
 *   - Return 0 (FT8_OK) on success, a negative FT8_E_* code otherwise; ft8_last_error() gives the
 *     message.  No C++ exception crosses this boundary.
 *   - One context per device per host thread/stream; a context is not re-entrant.  Its work is
 *     ordered across streams by the library: an entry point that uses the context's scratch, called
 *     on a stream other than the previous such call's, waits (device side) for that call's work, so
 *     two streams sharing one context serialise; independent streams want one context each.
 *     Every such call moves the context's order to its stream -- also one that enqueued nothing
 *     (n_slots = 0) or failed its argument checks: the next call on another stream then waits for
 *     whatever that stream holds at that point (a false dependency, never a missing one).
 */
#ifndef FT8HIP_H
#define FT8HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FT8HIP_ABI_VERSION 2

/* sample dtypes.  The waterfall dtype follows NumPy promotion against complex64 exactly as
 * scipy.signal.spectrogram does (spectrogram_analyse.py:46-56): F32/C64/I16 -> float32 waterfall,
 * F64/C128 -> float64 waterfall.  I16 samples are scaled x/32767 in float32 on the device
 * (from_wave.py:59-67 read_wave_file). */
enum ft8_dtype { FT8_F32 = 0, FT8_F64 = 1, FT8_C64 = 2, FT8_C128 = 3, FT8_I16 = 4 };

enum ft8_status {
  FT8_OK = 0,
  FT8_E_ARG = -1,         /* invalid argument (message in ft8_last_error) */
  FT8_E_HIP = -2,         /* HIP runtime error */
  FT8_E_UNSUPPORTED = -3, /* an input the path does not take (e.g. a dtype a stage does not accept) */
  FT8_E_NOMEM = -4,       /* device allocation failed */
  FT8_E_RANGE = -5        /* a size exceeds a compiled limit (see ft8_limits) */
};

/* Decoder parameters.  Mirrors decode_ft8_message's keyword arguments (ft8_decode.py:288-296);
 * the freq/time masks (ft8_decode.py:322-341) arrive as index ranges computed on the host. */
typedef struct ft8_params {
  int32_t sample_rate;      /* Hz */
  int32_t bins_per_tone;    /* freq_osr */
  int32_t steps_per_symbol; /* time_osr */
  int32_t max_candidates;   /* N of ft8_find_candidates */
  int32_t max_iterations;   /* BP iterations */
  int32_t min_score_f64;    /* 1: compare scores with min_score in float64 even for a float32
                               waterfall (the threshold was an np.float64); 0: in the waterfall
                               dtype (a Python int/float threshold, NumPy-2 rules) */
  double min_score;
  int32_t f_lo, f_hi;       /* kept STFT bins [f_lo, f_hi) after f >= 0 and the band mask */
  int32_t t_lo, t_hi;       /* kept frames [t_lo, t_hi) after the time mask */
  int32_t flags;            /* FT8_FLAG_* (0: the reference's behaviour exactly) */
  int32_t protocol;         /* FT8_PROTO_FT8 (0: everything as before the field had a meaning) or FT8_PROTO_FT4
                               ("FT4" below); anything else: FT8_E_ARG.  Honoured by ft8_stft (geometry),
                               ft8_sync_select and ft8_decode_batch; every other entry point that takes an
                               ft8_params refuses FT4 with FT8_E_UNSUPPORTED */
  double sample_rate_hz;    /* ABI 2: when > 0, the exact sample rate in Hz, integral or not (the
                               reference takes a float fs: spectrogram_analyse.py:32-34 computes
                               int(0.16 fs) and int(fs / 6.25 bpt) on it, so fs = 12006.3 gives
                               nperseg 1921); sample_rate is then ignored.  0: use sample_rate. */
} ft8_params;

/* ft8_params.flags.  All are build-defined extensions OUTSIDE reference parity (the reference
 * has none of them); with flags = 0 every result is the reference's.
 *   FT8_FLAG_TOPK      candidate selection keeps the max_candidates highest passing scores
 *                      (ties in scan order), sorted by score descending, instead of reproducing
 *                      ft8_find_candidates' heap quirk (ft8_decode.py:131-137, which keeps the
 *                      first N passing candidates in scan order).
 *   FT8_FLAG_SUBTRACT  ft8_decode_batch runs a second pass: every distinct message decoded in
 *                      pass 1 is re-modulated (ft8_encode + GFSK), fitted to the slot (time/
 *                      frequency refinement, per-symbol complex amplitude) and subtracted, and
 *                      the residual is decoded again.  New messages are appended after the
 *                      pass-1 results with pass_index bit 0 set.  F32 and I16 samples only.
 *                      ft8_set_subtract asks for up to FT8_SUBTRACT_MAX_PASSES passes and for the
 *                      FT8_FLAG_AP / FT8_FLAG_COHERENT retries inside every pass (default: 2, none).
 *   FT8_FLAG_AP        ft8_decode_batch retries every candidate BP failed on with the context's
 *                      a-priori hypotheses (ft8_set_ap; "a-priori decoding" below).  Rescued
 *                      candidates come out in candidate order among the plain decodes, with
 *                      pass_index >> 4 = hypothesis index + 1.  With FT8_FLAG_SUBTRACT only after
 *                      ft8_set_subtract(ctx, n, 1).
 *   FT8_FLAG_COHERENT  ft8_decode_batch demodulates the best-scoring candidates BP failed on again, coherently
 *                      from the samples ("coherent re-demodulation" below; ft8_set_coherent caps them per
 *                      slot), and decodes the new LLRs.  Rescued candidates come out in candidate order
 *                      among the plain decodes with pass_index bit 1 set.  F32 and I16 samples only; with
 *                      FT8_FLAG_SUBTRACT only after ft8_set_subtract(ctx, n, 1).  ft8_set_coherent_drift adds a search over linear
 *                      frequency drift to it, ft8_set_coherent_nsym joint LLRs over 2 and 3 symbols
 *                      (both off by default).
 *   FT8_FLAG_OSD       ft8_decode_batch decodes the first candidates of every slot that are still failed
 *                      after the passes above by ordered-statistics decoding of their STFT LLRs
 *                      ("ordered-statistics decoding" below; ft8_set_osd: order, cap per slot, hard-error
 *                      limit).  Rescued candidates come out in candidate order among the other decodes with
 *                      pass_index >> 4 = 15.  With FT8_FLAG_SUBTRACT only after ft8_set_subtract(ctx, n, 1).
 *   FT8_FLAG_BP_F32    every belief-propagation launch of the batch (the main pass, the a-priori, coherent and
 *                      coherent-AP retries, every subtraction pass, FT4) runs in IEEE binary32 instead of
 *                      float64 ("float32 belief propagation" below).  Decodes are then no longer bit-identical
 *                      to the reference's, but to the restatement named there; no record mark. */
#define FT8_FLAG_TOPK 1
#define FT8_FLAG_SUBTRACT 2
#define FT8_FLAG_AP 4
#define FT8_FLAG_COHERENT 8
#define FT8_FLAG_OSD 16
#define FT8_FLAG_BP_F32 32

/* One decoded (or attempted) candidate, 40 bytes, 8-byte aligned. */
typedef struct ft8_result {
  double score;            /* sync score; float32 value widened exactly on the float32 path */
  int32_t slot;            /* slot index within the batch */
  int32_t abs_time;        /* candidate time index (frame steps, may be negative) */
  int32_t abs_freq;        /* candidate frequency index (bins from f_lo) */
  uint16_t crc_extracted;  /* FT8DecodeStatus.crc_extracted */
  uint16_t crc_calculated; /* FT8DecodeStatus.crc_calculated (== FT8Message.hash when ok) */
  int16_t ldpc_errors;     /* FT8DecodeStatus.ldpc_errors (min parity errors seen by BP) */
  uint16_t cand_index;     /* position in the reference candidate order */
  uint8_t payload[10];     /* FT8Message.payload (77 bits, [9] & 0xF8) */
  uint8_t ok;              /* 1: LDPC converged and CRC matched (ft8_decode_candidate True) */
  uint8_t pass_index;      /* low nibble bit 0: 0 decoded from the slot, 1 appended by any pass >= 2 of an FT8_FLAG_SUBTRACT
                              batch, i.e. decoded from a residual (which pass: ft8_subtract_counts);
                              bit 1: decoded from the coherent LLRs (FT8_FLAG_COHERENT);
                              bit 2: ... at a drift rate other than 0 (ft8_set_coherent_drift);
                              bit 3: ... from a joint metric over 2 or 3 symbols (ft8_set_coherent_nsym);
                              high nibble 0: plain BP; h + 1 (1 .. 8): a-priori hypothesis h (FT8_FLAG_AP, ft8_ap_decode);
                              15: ordered-statistics decoding (FT8_FLAG_OSD, ft8_osd_decode) */
} ft8_result;

/* One transmitted FT8 signal for ft8_synthesize, 40 bytes. */
typedef struct ft8_tx_signal {
  double f0;               /* Hz, frequency of tone 0 (the reference's f0 + fc, modulator.py:76-90) */
  double amplitude;        /* peak amplitude of the real waveform */
  double phase;            /* radians added to the carrier phase (0: the reference's sin(phi)) */
  int64_t start;           /* first waveform sample within its slot (may be negative) */
  int32_t slot;            /* output row; the signal array must be sorted by slot ascending */
  int32_t reserved;
} ft8_tx_signal;

/* GFSK timing of ft8_synthesize */
enum ft8_tx_style {
  FT8_TX_PROTOCOL = 0,     /* symbol i occupies samples [i nsps, (i+1) nsps); ramp down at the end */
  FT8_TX_REFERENCE = 1     /* modulator.py exactly: freq_seq read without the one-symbol offset
                              (modulator.py:64-68, symbols start one symbol late) and its trailing
                              ramp (modulator.py:72-73) */
};

typedef struct ft8_ctx ft8_ctx;

/* ---- context ------------------------------------------------------------------------------ */
int ft8_create(int device, ft8_ctx** out);
int ft8_destroy(ft8_ctx* ctx);
const char* ft8_last_error(const ft8_ctx* ctx);
int ft8_abi_version(void);
/* compiled limits: max_candidates, max FFT length (real / complex) */
int ft8_limits(int32_t* max_candidates, int32_t* max_fft_real, int32_t* max_fft_complex);

/* STFT geometry of calculate_spectrogram (spectrogram_analyse.py:31-43): window length,
 * hop, FFT length and frame count for n_samples (frames = 0 when n_samples < nperseg). */
int ft8_geometry(int32_t sample_rate, int32_t bins_per_tone, int32_t steps_per_symbol,
                 int64_t n_samples, int32_t* nperseg, int32_t* hop, int32_t* nfft,
                 int32_t* n_frames);
/* The same for a sample rate given in (possibly non-integral) Hz, as ft8_params.sample_rate_hz. */
int ft8_geometry_hz(double sample_rate_hz, int32_t bins_per_tone, int32_t steps_per_symbol,
                    int64_t n_samples, int32_t* nperseg, int32_t* hop, int32_t* nfft,
                    int32_t* n_frames);

/* ---- stage 1: STFT -> dB waterfall ---------------------------------------------------------
 * Replaces calculate_spectrogram (spectrogram_analyse.py:19-66) + the f>=0 / band / time masks
 * (ft8_decode.py:322-341).  d_samples: n_slots rows of n_samples, row stride slot_stride
 * elements.  Output d_wf[n_slots][t_hi-t_lo][f_hi-f_lo] (TIME-major: the transpose of the
 * reference's mag[freq, time]), bins in natural FFT order k in [f_lo, f_hi) of [0, nfft).  For
 * real input bins above nfft/2 are the mirror image (two-sided spectrum of a real signal). */
int ft8_stft(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
             int64_t slot_stride, const ft8_params* p, void* d_wf, void* stream);

/* Which transform ft8_stft / ft8_decode_batch runs for a geometry (introspection for tests and
 * tuning): FT8_STFT_STOCKHAM (LDS mixed-radix FFT), FT8_STFT_PACKED3840 (the production 12 kHz
 * kernel), FT8_STFT_CHIRPZ (Bluestein: nfft with a prime factor above 7, or odd with real input),
 * FT8_STFT_DFT (direct DFT: what neither FFT path takes); negative FT8_E_* on a bad geometry. */
#define FT8_STFT_STOCKHAM 0
#define FT8_STFT_PACKED3840 1
#define FT8_STFT_CHIRPZ 2
#define FT8_STFT_DFT 3
int ft8_stft_method(ft8_ctx* ctx, int32_t sample_rate, int32_t bins_per_tone, int32_t steps_per_symbol,
                    int64_t n_samples, int dtype);
/* Introspection of the last ft8_stft_argmax / drift STFT on complex128 input at the 3840-point
 * geometry, which decides each frame's argmax in float32 where a rounding-error bound settles it
 * and redoes the others in float64: *frames_redone = the float64 frames of that call, *frames =
 * all its frames (0 / 0 when the last call took another path).  Synchronises the device. */
int ft8_stft_screen_stats(ft8_ctx* ctx, int64_t* frames_redone, int64_t* frames);

/* ---- stage 2: Costas sync score grid + candidate selection ---------------------------------
 * Replaces ft8_sync_score / ft8_find_candidates (ft8_decode.py:47-149).  d_wf as produced by
 * ft8_stft: [n_slots][T][F] (row stride F, slot stride T*F), float32 (wf_f64=0) or float64.
 * Outputs per slot s: d_cand[s][max_candidates][2] = (abs_time, abs_freq) in the reference's
 * final order, d_cand_score[s][max_candidates] (double), d_cand_count[s].  d_scores (nullable)
 * receives the full score grid [n_slots][NT][NF] in scan order in the waterfall dtype. */
int ft8_sync_select(ft8_ctx* ctx, const void* d_wf, int wf_f64, int32_t n_slots, int32_t T,
                    int32_t F, const ft8_params* p, int32_t* d_cand, double* d_cand_score,
                    int32_t* d_cand_count, void* d_scores, void* stream);

/* ft8_sync_score itself (ft8_decode.py:47-100) for arbitrary candidates d_cand[n][2] = (abs_time,
 * abs_freq), on or off the search grid: d_out[n] in the waterfall dtype (-inf as the reference
 * returns it), d_err[n] = 1 where the reference's get_log_power (ftx_types.py:45-47) would raise
 * IndexError (NumPy indexing: negative indices count from the end, nothing guards the frequency
 * axis).  d_wf as for ft8_sync_select. */
int ft8_sync_score(ft8_ctx* ctx, const void* d_wf, int wf_f64, int32_t T, int32_t F, int32_t steps_per_symbol,
                   int32_t bins_per_tone, const int32_t* d_cand, int32_t n, void* d_out, int32_t* d_err,
                   void* stream);

/* ---- stage 3: soft LLRs --------------------------------------------------------------------
 * Replaces ft8_extract_likelihood + ftx_normalize_logl (ft8_decode.py:151-198).  d_cand[n][3] =
 * (slot, abs_time, abs_freq).  Output d_llr[n][174] (double). */
int ft8_llr(ft8_ctx* ctx, const void* d_wf, int wf_f64, int32_t T, int32_t F,
            int32_t steps_per_symbol, int32_t bins_per_tone, const int32_t* d_cand, int32_t n,
            int normalize, double* d_llr, void* stream);

/* ftx_normalize_logl alone (ft8_decode.py:190-198): d_out[n][174] = d_in * sqrt(24 / var(d_in)),
 * with NumPy's pairwise summation order for the mean and variance. */
int ft8_normalize(ft8_ctx* ctx, const double* d_in, int32_t n, double* d_out, void* stream);

/* ---- stage 4: LDPC belief propagation + CRC ------------------------------------------------
 * Replaces bp_decode (ldpc_decoder.py:54-113) and the tail of ft8_decode_candidate
 * (ft8_decode.py:236-273, crc.py:11-54).  d_llr[n][174] double.  Outputs (each nullable):
 * d_plain[n][174] hard decisions of the last evaluated iteration, d_res[n] records (score/slot/
 * abs_* left 0). */
int ft8_bp(ft8_ctx* ctx, const double* d_llr, int32_t n, int32_t max_iterations,
           uint8_t* d_plain, ft8_result* d_res, void* stream);

/* ---- whole receive path ---------------------------------------------------------------------
 * Replaces decode_ft8_message (ft8_decode.py:288-394) for a batch of independent slots:
 * STFT -> sync/select -> LLR -> BP -> CRC, all on the device.  Writes, per slot s, the successful
 * decodes in candidate order to d_out[s][0 .. d_counts[s]) (capped at max_results_per_slot;
 * d_counts holds the uncapped count).  With FT8_FLAG_AP the a-priori pass ("a-priori decoding"
 * below) runs between BP and the compaction, on the batch's own LLRs and records: FT8_E_ARG when the
 * context holds no hypotheses, FT8_E_UNSUPPORTED together with FT8_FLAG_SUBTRACT unless
 * ft8_set_subtract(ctx, n, 1) lifted that. */
int ft8_decode_batch(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples,
                     int32_t n_slots, int64_t slot_stride, const ft8_params* p,
                     ft8_result* d_out, int32_t* d_counts, int32_t max_results_per_slot,
                     void* stream);

/* Pipelining of ft8_decode_batch (a context setting).  The batch is cut into chunks of
 * chunk_slots slots, each an independent STFT -> sync/select -> LLR -> BP -> compact chain, and
 * the chunks alternate over n_streams internal streams (forked from and joined back into the
 * caller's stream), so one chunk's BP overlaps the next chunk's STFT/score.  bp_waves_per_simd
 * (1..4) bounds the BP kernel's resident waves per SIMD (chunked or not), leaving room for work on
 * other streams.  n_streams = 0 runs the whole batch as one chain on the caller's stream.  Default
 * (0, 0, 4): one chain, the full BP grid -- on MI355X the BP kernel is FP64-VALU bound and
 * overlapping it with the next chunk's STFT/score measured no gain.  Results do not depend on the
 * setting. */
int ft8_set_pipeline(ft8_ctx* ctx, int32_t chunk_slots, int32_t n_streams, int32_t bp_waves_per_simd);

/* ---- multi-GPU exchange (slot shards, one all-gather of the decodes per batch) --
 * No reference counterpart (the reference is single-process).  Packs the decodes of one
 * ft8_decode_batch (d_records[n_slots][cap], d_counts[n_slots]) into ONE byte buffer that a
 * collective (RCCL all-gather) moves as-is, on the device and without a host sync:
 *   d_send = [int64 total][int32 counts[n_slots], padded to 8 B][capacity x ft8_result]
 * total = sum over slots of min(counts, cap) (counts are copied uncapped); records in slot order,
 * then candidate order, each with ft8_result.slot += slot_offset (global slot ids); rows of the
 * send buffer past total are zeroed.  Rows >= capacity go to d_overflow[row - capacity] when
 * d_overflow (capacity for n_slots * cap - capacity rows) is non-null, else are dropped -- the
 * receiver sees total > capacity either way.  ft8_pack_bytes gives the send-buffer size. */
int64_t ft8_pack_bytes(int32_t n_slots, int32_t capacity);
int ft8_pack_decodes(ft8_ctx* ctx, const ft8_result* d_records, const int32_t* d_counts, int32_t n_slots,
                     int32_t cap, int32_t capacity, int32_t slot_offset, void* d_send, ft8_result* d_overflow,
                     void* stream);

/* ---- message layer: 77-bit payload -> text -----------------------------------------------------
 * Build-defined, outside reference parity (the reference stops at the payload).  The FT8 message
 * types unpacked are the standard message (i3 = 1, 2), the message with one non-standard callsign
 * (i3 = 4), free text (i3 = 0, n3 = 0) and telemetry (i3 = 0, n3 = 5); field layouts in DESIGN.md.
 * One text record per ft8_result, 64 bytes. */
typedef struct ft8_text {
  char     text[28];      /* NUL-padded ASCII, at most 26 characters; hashed calls as "<...>" */
  char     learn_call[12];/* the callsign carried in full that a receiver adds to its hash table: i3=4 the c58 call;
                             i3=1/2 the second callsign without /R,/P when it is a standard callsign; else empty */
  uint32_t hash[2];       /* value of the first / second "<...>" in text, left to right */
  uint32_t learn_hash22;  /* n22 of learn_call (0 when empty) */
  int16_t  dup_of;        /* index within the slot of the first ok record with the same 77 bits, -1 if this is it */
  uint8_t  hash_bits[2];  /* 0, 12 or 22 for each entry of hash[] */
  uint8_t  i3, n3;        /* n3 is 0 unless i3 == 0 */
  uint8_t  status;        /* 0 text valid; 1 type not decoded; 2 a field out of range; 3 record not ok (not unpacked) */
  uint8_t  reserved[5];
} ft8_text;

/* Text records of a ft8_decode_batch's output (d_records[n_slots][cap], d_counts[n_slots] as that
 * call wrote them; d_counts NULL: every slot holds cap records): d_out[s * cap + r] is written for
 * every r < cap.  Records at r >= min(d_counts[s], cap) and records with ok == 0 get status 3,
 * dup_of -1 and zeros elsewhere, and never serve as a duplicate's original.  Records with status 1
 * or 2 carry i3 / n3 and zeros elsewhere.  dup_of compares the 77 payload bits ([9] & 0xF8) with
 * the slot's earlier records.  cap <= 32767.  One kernel on the caller's stream; it uses none of the
 * context's scratch and allocates nothing, so like ft8_pack_decodes it takes no part in the
 * context's cross-stream order: call it on the stream that produced d_records (or after an event
 * of it). */
int ft8_unpack77(ft8_ctx* ctx, const ft8_result* d_records, const int32_t* d_counts, int32_t n_slots,
                 int32_t cap, ft8_text* d_out, void* stream);
/* The same unpacker on the host for n payloads[n][10] in host memory: no context, no GPU.
 * dup_of = -1 throughout. */
int ft8_unpack77_host(const uint8_t* payloads, int32_t n, ft8_text* out);
/* Host: the 22-bit hash of a callsign (n12 = n22 >> 10, n10 = n22 >> 12).  FT8_E_ARG for a
 * character outside " 0-9A-Z/" or a length above 11. */
int ft8_hash_call(const char* call, uint32_t* n22);

/* ---- signal report: the SNR of every decode ------------------------------------------------------
 * Build-defined, outside reference parity (the reference stops at the payload).  The estimator
 * (DESIGN.md section 10), on a waterfall d_wf[n_slots][T][F] as ft8_stft writes it (dB, float32 or
 * float64; every value is widened to double and all arithmetic is double):
 *   P[t][f]  = 10^(wf[t][f] / 10)
 *   A[f]     = mean over t of P[t][f], added in the order t = 0 .. T-1
 *   N0       = the element of rank floor(q (F-1)) of A sorted ascending (no interpolation; NaNs last)
 *   M(dt,df) = mean over the symbols k = 0 .. 78 whose row lies in [0, T) of
 *              P[abs_time + dt + k steps_per_symbol][abs_freq + df + tone[k] bins_per_tone],
 *              tone[] the record's payload re-encoded, added in the order of k; dt, df in
 *              [-radius, radius], of which only the df with abs_freq + df >= 0 and
 *              abs_freq + df + 7 bins_per_tone <= F - 1 are considered; offsets with no row in range
 *              or a NaN mean are skipped; the first largest M wins (dt outer, df inner, ascending)
 *   S        = M - N0, raised to 1e-3 N0 (status 1) when below it
 *   snr_db   = 10 log10(S / N0) + 10 log10(enbw_hz / 2500), enbw_hz = 1.5 fs / nperseg (the
 *              equivalent noise bandwidth of the STFT's periodic Hann window): the SNR in 2500 Hz.
 * One report per ft8_result, 24 bytes. */
typedef struct ft8_snr_rec {
  double  snr_db;
  float   signal_db;      /* 10 log10 S */
  float   noise_db;       /* 10 log10 N0 */
  int8_t  dt, df;         /* the grid offset whose mean was taken */
  uint8_t n_symbols;      /* symbols of it whose row lies in [0, T) */
  uint8_t status;         /* 0 valid; 1 valid, S was raised to 1e-3 N0; 2 no admissible offset or symbol (zeros
                             elsewhere); 3 record not ok or past the slot's count (zeros elsewhere) */
  uint8_t reserved[4];
} ft8_snr_rec;

/* A and N0 of every slot: d_colmean[n_slots][F] (required) and d_floor[n_slots].  q in [0, 1].  T and
 * F >= 1; any F is taken.  Two kernels on the caller's stream (the means, reading the waterfall
 * once; the quantile, reading d_colmean); they use none of the context's scratch, so the call takes
 * no part in the context's cross-stream order. */
int ft8_noise_floor(ft8_ctx* ctx, const void* d_wf, int wf_f64, int32_t n_slots, int32_t T, int32_t F, double q,
                    double* d_floor, double* d_colmean, void* stream);
/* The reports of d_records[n_slots][cap] (d_counts as for ft8_unpack77, NULL: every slot holds cap
 * records) against d_floor[n_slots]: d_out[s * cap + r] is written for every r < cap.  p gives
 * bins_per_tone, steps_per_symbol and, with n_samples, the STFT geometry (nperseg, for enbw_hz).
 * radius 0 or 1.  One kernel on the caller's stream, no context scratch, no part in the
 * cross-stream order. */
int ft8_snr(ft8_ctx* ctx, const void* d_wf, int wf_f64, int32_t n_slots, int32_t T, int32_t F, const ft8_params* p,
            int64_t n_samples, const ft8_result* d_records, const int32_t* d_counts, int32_t cap,
            const double* d_floor, int32_t radius, ft8_snr_rec* d_out, void* stream);
/* ft8_noise_floor (q = 0.25) and ft8_snr (radius 1) on the waterfall the last ft8_decode_batch of this context left
 * in its scratch, for that call's records: n_slots and cap must equal that call's n_slots and
 * max_results_per_slot, and no other entry point that uses the context's scratch (nor ft8_llr,
 * ft8_sync_score, ft8_normalize, ft8_encode, ft8_crc14, ft8_ldpc_check) may have run on the context
 * in between -- FT8_E_ARG otherwise; ft8_unpack77 and ft8_pack_decodes may.  A pipelined (chunked)
 * batch is as good as a single chain: the chunks write one contiguous waterfall.  After an
 * FT8_FLAG_SUBTRACT batch the scratch holds the waterfall of the residual, from which the pass-1
 * signals are gone: FT8_E_UNSUPPORTED (measure those with ft8_stft + ft8_noise_floor + ft8_snr).
 * Three kernels (ft8_noise_floor's two, ft8_snr's one).  A and N0 live in the context's scratch, so the call takes part in the cross-stream order. */
int ft8_snr_last(ft8_ctx* ctx, const ft8_result* d_records, const int32_t* d_counts, int32_t n_slots, int32_t cap,
                 ft8_snr_rec* d_out, void* stream);

/* ---- a-priori decoding: retry failed candidates with known message bits ----------------------------
 * Build-defined, outside reference parity (the reference decodes every candidate once).  A candidate
 * enters a-priori (AP) decoding when plain BP left ok == 0.  With L[174] its LLRs as BP consumed them
 * (normalised doubles, positive = bit 1) and the context's hypotheses h = 0 .. H-1 (77 mask bits and
 * 77 value bits each, laid out like ft8_result.payload: MSB first, [9] & 0xF8):
 *   a        = 1.01 * max_i |L[i]| (one multiply in double); a NaN (any L[i] NaN) or a == 0 leaves the
 *              candidate as it is.  L[i] is finite or NaN.
 *   L_h[i]   = +a where i < 77 and mask bit i and value bit i are set, -a where mask bit i is set and
 *              value bit i is not, L[i] everywhere else
 *   attempt h = bp_decode(L_h, max_iterations) and the reference tail, exactly as ft8_bp runs them;
 *              it is accepted when (1) the tail says ok, (2) the decoded payload agrees with value on
 *              every masked bit, and (3) hard_h = #{ i < 174 : plain_h[i] != (L[i] > 0) } <=
 *              max_hard_errors -- counted against the UNCLAMPED L.
 * The first accepted h wins (hypotheses run one after another; a rescued candidate is not retried).
 * The winning record gets ok = 1, that attempt's payload, crc_extracted, crc_calculated and
 * ldpc_errors, and pass_index |= (h + 1) << 4; score, slot, abs_time, abs_freq and cand_index do not
 * change.  A candidate no hypothesis rescues keeps the record plain BP wrote.
 * Scratch (context-owned, grow-only) for n records: 174 * 8 n bytes of clamped LLRs, 174 n bytes of
 * hard decisions, and 68 n bytes of lists and records (n = n_slots * max_candidates in
 * ft8_decode_batch). */
typedef struct ft8_ap_hyp {
  uint8_t mask[10];
  uint8_t value[10];
} ft8_ap_hyp; /* 20 bytes */
#define FT8_AP_MAX_HYP 8

/* The context's hypotheses (a context setting, like ft8_set_pipeline): hyps[n] in HOST memory is
 * copied into the context, from where every AP launch takes its hypothesis as a kernel argument.
 * n = 0 clears them; n > FT8_AP_MAX_HYP: FT8_E_RANGE; a mask or value bit outside the 77, or
 * max_hard_errors outside [0, 174] (174: no limit): FT8_E_ARG. */
int ft8_set_ap(ft8_ctx* ctx, const ft8_ap_hyp* hyps, int32_t n, int32_t max_hard_errors);
/* The stage call, on records as ft8_bp wrote them from the same d_llr[n][174]: records with ok == 0
 * are tried against the context's hypotheses and updated in place per the contract above (the n
 * records are one list).  d_hard[n] (nullable): hard_h of an accepted AP decode, -1 otherwise.  Per
 * hypothesis three small kernels and one k_bp launch (whose work ft8_get_counters counts with the
 * plain launches').  Uses the context's scratch, so it takes part in the cross-stream order.  n = 0
 * does nothing; no hypotheses set: FT8_E_ARG. */
int ft8_ap_decode(ft8_ctx* ctx, const double* d_llr, ft8_result* d_res, int32_t n, int32_t max_iterations,
                  int16_t* d_hard, void* stream);

/* ---- coherent re-demodulation: LLRs of a candidate from the samples ----------------------------------
 * Build-defined, outside reference parity (the reference forms its LLRs once, from the dB bins of a
 * one-symbol Hann STFT).  ft8_demodulator_amd/coherent.py: coherent_restate is this contract in NumPy.
 * Geometry: nsps = nperseg, hop = nsps / steps_per_symbol, Q = the largest divisor of nsps in [8, 32],
 * D = nsps / Q, tone spacing 6.25 Hz, bin = fs / nfft.  For a candidate (abs_time, abs_freq) of a slot
 * of real float32 samples x (int16: x / 32767 in float32, as the STFT scales it):
 *   1. baseband   s0 = (t_lo + abs_time) hop, f0 = (f_lo + abs_freq) bin, fmix = f0 + 3.5 * 6.25,
 *                 Mt = ceil((hop / 2) / D), Mg = Mt + 1, nb = s0 - Mg D,
 *                 z[m] = sum_{i < D} x[nb + m D + i] exp(-2 pi i fmix (nb + m D + i) / fs), m in [0, 79 Q + 2 Mg);
 *                 samples outside [0, n_samples) count as 0.
 *   2. presence   for a start offset dt in [-Mt, Mt] symbol k's window is z[Mg + dt + k Q + q], q < Q; the
 *                 symbol is present when all of its Q D input samples lie in [0, n_samples).
 *   3. sync       on the 21 Costas symbols (3 1 4 0 6 5 2 at symbols 0-6, 36-42, 72-78, tone c_k), offsets
 *                 dt outer and df_j = (j - 2) bin / 4, j = 0 .. 4, inner, both ascending:
 *                 metric(dt, j) = sum over the present sync symbols k of
 *                                 |sum_q w_k[q] exp(-2 pi i (c_k - 3.5 + df_j / 6.25) q / Q)|^2;
 *                 the first largest metric wins; an interior j is refined by the parabola through its
 *                 two neighbours in j where their second difference is negative.  No sync symbol
 *                 present at any dt: status 2.
 *   4. LLRs       at the winning (dt, df), for each of the 58 data symbols (ft8_extract_likelihood's
 *                 order) c[t] = sum_q w_k[q] exp(-2 pi i (t - 3.5 + df / 6.25) q / Q), t = 0 .. 7,
 *                 s[t] = 10 log10(1e-12 + |c[t]|^2), three LLRs by ft8_extract_symbol's Gray map and
 *                 max-of-4 differences; a symbol that is not present gives three zeros; then
 *                 ftx_normalize_logl (x *= sqrt(24 / var) over all 174).  A variance of 0 or NaN: status 2.
 * The device accumulates z, the correlations and |c|^2 in float32 and forms s[t], the LLRs and the
 * normalisation in double; status 2 and 3 leave 174 zeros. */
typedef struct ft8_coh_fit {
  float   dt_s;           /* dt D / fs */
  float   df_hz;          /* the refined tone-0 offset */
  float   metric;         /* metric(dt, j) of the winning offsets */
  uint8_t n_sync;         /* sync symbols present at dt */
  uint8_t status;         /* 0 valid; 2 nothing to measure (no sync symbol present: zeros elsewhere; or the
                             variance test of step 4); 3 not attempted (slot index out of range; zeros elsewhere) */
  int8_t  dt_index;       /* dt, in steps of D samples */
  uint8_t df_index;       /* j */
} ft8_coh_fit; /* 16 bytes */

/* The stage call: n candidates d_cand[n][2] = (abs_time, abs_freq) of the slots d_slot_of[n] as one list
 * -> d_llr_out[n][174] (double) and d_fit_out[n], one 256-thread workgroup per candidate.  Samples and
 * params as for ft8_stft (p gives the sample rate, the oversampling factors, t_lo and f_lo).
 * FT8_E_UNSUPPORTED for a dtype other than FT8_F32 / FT8_I16 and for a geometry without Q or whose hop
 * does not divide nsps (fs = 12006.3); FT8_E_RANGE when nsps / Q twiddles do not fit the kernel's 64 KB
 * of LDS.  Caller-owned buffers, no context scratch: no part in the cross-stream order. */
int ft8_coherent_llr(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                     int64_t slot_stride, const ft8_params* p, const int32_t* d_cand, const int32_t* d_slot_of,
                     int32_t n, double* d_llr_out, ft8_coh_fit* d_fit_out, void* stream);
/* FT8_FLAG_COHERENT inside ft8_decode_batch (a context setting, like ft8_set_ap): after plain BP, per slot
 * the first max_per_slot candidates with ok == 0 in candidate order (0: every one; the selection of
 * FT8_FLAG_TOPK is sorted by score, so these are the best-scoring failures) are demodulated as above and
 * their LLRs decoded by the unchanged BP kernel and tail.  A candidate whose fit has status 0 and whose
 * attempt the tail accepts gets ok = 1, that attempt's payload, crc_extracted, crc_calculated and
 * ldpc_errors, and pass_index |= 2; score, slot, abs_time, abs_freq and cand_index do not change, and
 * every other candidate keeps the record plain BP wrote.  The pass runs before the a-priori pass, which
 * sees the STFT LLRs of the candidates still failed.  FT8_E_UNSUPPORTED as for the stage call, and
 * together with FT8_FLAG_SUBTRACT unless ft8_set_subtract(ctx, n, 1) lifted that.  Scratch (context-owned, grow-only) per listed candidate: 174 * 8
 * bytes of LLRs and 76 bytes of lists, fits and records.  max_per_slot < 0: FT8_E_ARG.  Default 0. */
int ft8_set_coherent(ft8_ctx* ctx, int32_t max_per_slot);

/* ---- coherent re-demodulation with a search over linear frequency drift ----------------------------
 * Opt-in and build-defined like the pass itself; coherent.py: coherent_restate(drift=...) restates it.
 * A signal whose frequency runs as f(t) = f_c + r (t - t_c) about its centre t_c (r in Hz/s) smears over
 * the tone filters of steps 3 and 4 above.  With n_rates = R (odd, 1 <= R <= 33) and max_rate = A
 * (0 <= A <= 4.0 Hz/s) one step is added between steps 1 and 2:
 *   1b. de-chirp  rates r_i = (i - (R - 1) / 2) * 2 A / (R - 1), i = 0 .. R - 1;
 *                 z_i[m] = z[m] exp(-i pi r_i tau_m^2), tau_m = ((m - Mg + 0.5) D - 39.5 nsps) / fs: the
 *                 centre of decimation block m relative to the centre of the nominal signal (the phase
 *                 formed in double, reduced mod 1 cycle before it is rounded to float32).
 *   3.  sync      metric(i, dt, j) is step 3's metric on z_i; i outer, then dt, then j, all ascending;
 *                 the first largest wins.  The parabola in j is applied at the winning (i, dt); the rate
 *                 is not refined.
 *   4.  LLRs      unchanged, on z_i of the winning rate, so df_hz is the offset at the signal's centre.
 * R = 1 or A = 0: off, exactly the pass above.  The device rotates z in place from one rate to the next
 * (float32, one factor per element, the same for every step) and once more to the winner. */
typedef struct ft8_coh_drift {
  float   rate_hz_per_s;  /* r_i of the winning rate */
  int32_t rate_index;     /* i */
} ft8_coh_drift; /* 8 bytes */

/* ft8_coherent_llr with the drift search: d_drift_out[n] (may be NULL) receives the winning rates, zeros
 * where no sync was made (status 3, and status 2 for want of a sync symbol).  n_rates = 1 or max_rate = 0 writes exactly the bytes of ft8_coherent_llr and zeros
 * in the drift records.  FT8_E_ARG for an even n_rates, n_rates outside [1, 33], max_rate outside [0, 4]. */
int ft8_coherent_drift_llr(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                           int64_t slot_stride, const ft8_params* p, const int32_t* d_cand,
                           const int32_t* d_slot_of, int32_t n, float max_rate_hz_per_s, int32_t n_rates,
                           double* d_llr_out, ft8_coh_fit* d_fit_out, ft8_coh_drift* d_drift_out, void* stream);
/* The drift search inside FT8_FLAG_COHERENT (a context setting like ft8_set_coherent; default off: 0, 1).
 * A record rescued at a winning rate other than 0 gets pass_index |= 4 on top of |= 2; the rate itself is
 * not carried in ft8_result (the stage call gives it).  The pass's scratch grows by 8 bytes per listed
 * candidate.  Errors as for the stage call. */
int ft8_set_coherent_drift(ft8_ctx* ctx, float max_rate_hz_per_s, int32_t n_rates);

/* ---- coherent re-demodulation with joint LLRs over 2 and 3 symbols ----------------------------------
 * Opt-in and build-defined like the pass itself; coherent.py: coherent_restate(nsym=...) restates it.
 * FT8 is continuous-phase 8-FSK: after the fit of steps 1 - 3 the phase carried from one symbol to the
 * next is known, so the correlations of adjacent symbols can be added coherently under each joint tone
 * hypothesis.  With max_nsym = S in {1, 2, 3} the pass produces S LLR vectors ("sets") per candidate; set
 * 1 is step 4's vector, unchanged (S = 1: exactly the pass above).  Step 4b, for n = 2 .. S:
 *   spectra   c_k[t], t = 0 .. 7: the complex correlations of step 4 at the winning (dt, df), of the 58
 *             data symbols k (under the drift search on z of the winning rate); c_k[t] = 0 for every t of
 *             a symbol that is not present (step 2).
 *   phase     c'_k[t] = c_k[t] exp(-2 pi i frac((df / 6.25 - 3.5) k)), k the symbol index 0 .. 78.  (The
 *             baseband is mixed to the centre of the band and 6.25 nsps / fs = 1, so a symbol of tone t
 *             advances the phase by 2 pi (t - 3.5 + df / 6.25); the integer t drops out.)
 *   groups    each half (symbols 7 .. 35 and 43 .. 71) is cut, in order, into groups of n symbols with a
 *             shorter last group: 14 pairs and 1 single for n = 2, 9 triples and 1 pair for n = 3.
 *   metric    for a group of g symbols k_1 .. k_g and each of the 8^g tone tuples (a_1 .. a_g):
 *             p = |sum_i c'_{k_i}[a_i]|^2, s = 10 log10(1e-12 + p).  Tone FT8_Gray_map[j] carries the three
 *             bits of j, MSB first (ft8_extract_symbol).  The LLR of bit b of symbol k_i is max(s over the
 *             tuples whose a_i has the bit 1) - max(s over those whose a_i has it 0).  The bits of an
 *             absent symbol come out 0.
 *   validity  each set is normalised by ftx_normalize_logl as in step 4; a set whose variance is 0 or NaN
 *             is written as zeros and is invalid.  One byte per candidate: bit n - 1 set for a valid set
 *             n; bit 0 exactly when fit.status == 0; 0 for status 2 or 3 (every set zeros).
 * The device adds the correlations and takes each maximum in float32 (the maximum is exact), and forms
 * the six logarithms per symbol, the differences and the normalisation in double. */

/* ft8_coherent_drift_llr with max_nsym sets: d_llr_out[n][max_nsym][174], d_valid_out[n] (may be NULL) the
 * validity bytes.  max_nsym = 1 writes exactly the bytes of ft8_coherent_drift_llr.  FT8_E_ARG for max_nsym
 * outside [1, 3]; other errors as for ft8_coherent_drift_llr. */
int ft8_coherent_nsym_llr(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                          int64_t slot_stride, const ft8_params* p, const int32_t* d_cand,
                          const int32_t* d_slot_of, int32_t n, float max_rate_hz_per_s, int32_t n_rates,
                          double* d_llr_out, ft8_coh_fit* d_fit_out, ft8_coh_drift* d_drift_out, int32_t max_nsym,
                          uint8_t* d_valid_out, void* stream);
/* The sets inside FT8_FLAG_COHERENT (a context setting like ft8_set_coherent_drift; default 1: off).  The
 * list and the demodulation run once per chunk; then for n = 1 .. max_nsym in order BP decodes the lists
 * from set n's LLRs and a merge follows.  Set n rewrites the record of a list position when the fit is
 * valid, set n is valid, the tail accepted the attempt and the record is not ok already: the first set
 * wins.  The record is written as by the pass above (pass_index |= 2, or |= 6 at a drift rate other than
 * 0) and gets pass_index |= 8 when n > 1; which of sets 2 and 3 won is not carried (the stage call tells).
 * Positions an earlier set rescued are decoded again by the later sets' BP launches.  Scratch per listed
 * candidate: max_nsym * 174 * 8 bytes of LLRs, max_nsym * 40 bytes of records (instead of 174 * 8 and 40)
 * and, for max_nsym > 1, 1 validity byte.  FT8_E_ARG for max_nsym outside [1, 3]. */
int ft8_set_coherent_nsym(ft8_ctx* ctx, int32_t max_nsym);

/* ---- a-priori retries on the coherent LLRs (coherent_ap) ------------------------------------------------
 * Opt-in and build-defined like both passes; coherent.py: coherent_ap_restate restates it.  The coherent
 * pass demodulates a failed candidate again but decodes it without known bits; the a-priori pass has the
 * known bits but only on the STFT LLRs.  With this setting on, a batch that carries both FT8_FLAG_COHERENT
 * and FT8_FLAG_AP runs a third stage per chunk, after the coherent pass's last merge and before the
 * a-priori pass, on the list the coherent pass built: the same M positions per slot, fits, S = max_nsym LLR
 * sets, validity bytes and drift records.  For each list position:
 *   eligible   only while the original record has ok == 0 and the position's fit has status 0.
 *   sets       n = 0 .. S - 1; with validity bytes (S > 1) only where bit n is set.  L_n is the set's 174
 *              coherent LLRs and a_n = 1.01 * max_i |L_n[i]| (one multiply in double); a_n NaN or 0: set n is
 *              skipped for every hypothesis.
 *   attempts   hypothesis h = 0 .. H - 1 outer, usable set n ascending inner: L_{h,n} is the clamp of the
 *              a-priori contract on L_n (+-a_n on the masked bits below 77, L_n[i] elsewhere), then
 *              bp_decode(L_{h,n}, max_iterations) and the reference tail, exactly as ft8_bp runs them.
 *   accepted   as in the a-priori contract: (1) the tail says ok, (2) the payload agrees with value on every
 *              masked bit, (3) #{ i < 174 : plain[i] != (L_n[i] > 0) } <= max_hard_errors, counted against
 *              the UNCLAMPED L_n.
 * The first accepted attempt in that order wins: the lowest hypothesis, and within it the first usable set.
 * Its record gets ok = 1, the attempt's payload, crc_extracted, crc_calculated and ldpc_errors, and
 * pass_index |= 2 | (h + 1) << 4, |= 4 more where the position's drift rate is not 0, |= 8 more where n > 0;
 * score, slot, abs_time, abs_freq and cand_index do not change.  A position nothing rescues keeps its record,
 * and the a-priori pass then runs unchanged on the STFT LLRs of what is still failed.  Attempts do not depend
 * on one another, so the device makes all of them and picks the first accepted afterwards: five launches per
 * chunk (a_n; the attempt lists; the clamp; one k_bp launch over every attempt, counted by ft8_get_counters
 * with the others; the merge), whatever H and S are.  Under ft8_set_subtract(ctx, n, 1) the stage runs in
 * every pass.  Scratch (context-owned, grow-only) for n_slots * M * H * S attempts: per attempt 174 * 8 bytes
 * of clamped LLRs, 174 bytes of hard decisions and 64 bytes of lists and records, and 8 S bytes per list
 * position; more than 2^31 - 1 attempts: FT8_E_RANGE.
 *
 * The setting: on = 0 or 1 (default 0); any other value: FT8_E_ARG, the setting unchanged.  It takes effect
 * only in a batch with both flags; in any other batch it is ignored and is no error, and every other check
 * and refusal of ft8_decode_batch stays as it is. */
int ft8_set_coherent_ap(ft8_ctx* ctx, int32_t on);
/* The stage call: d_llr[n][n_sets][174] as ft8_coherent_nsym_llr writes it (n_sets 1 .. 3), d_valid[n]
 * (nullable: every set usable) its validity bytes, d_res[n] records as ft8_bp left them, treated as one
 * list with every fit valid and no drift.  Records with ok == 0 are tried per the contract above with the
 * context's hypotheses and max_hard_errors and updated in place (pass_index |= 2 | (h + 1) << 4, and 8 where
 * the winning set is not the first).  d_hard[n] (nullable): the accepted attempt's hard-error count, -1
 * elsewhere.  n = 0 does nothing; no hypotheses set, or n_sets outside [1, 3]: FT8_E_ARG.  Uses the
 * context's scratch, so it takes part in the cross-stream order. */
int ft8_coherent_ap_decode(ft8_ctx* ctx, const double* d_llr, int32_t n_sets, const uint8_t* d_valid,
                           ft8_result* d_res, int32_t n, int32_t max_iterations, int16_t* d_hard, void* stream);

/* ---- ordered-statistics decoding (OSD) of failed candidates -------------------------------------------
 * Opt-in and build-defined like the a-priori and coherent passes (the reference has no counterpart);
 * osd.py restates it in NumPy: osd_restate, osd_pass_restate.  All arithmetic is in integers, the echelon
 * form is the unique reduced one and the candidates have a fixed order, so the restatement and the device
 * agree bit for bit.  For one candidate with the LLRs L[174] as BP consumed them (positive = bit 1):
 *   1. q[i] = min(floor(|L[i]| * 256), 65535) (+-inf: 65535), hard[i] = L[i] > 0.  A NaN among L, or every
 *      q[i] == 0: not attempted (status 2).
 *   2. perm: the indices sorted by q descending, equal q by index ascending.
 *   3. G = [I | P] is the 91 x 174 systematic generator (column 91 + m: parity row m of FT8_GEN_ROWS_INIT).
 *      Going through G's columns in perm order, a column is a basis column when it is independent of the
 *      basis columns before it, until there are 91.  M is the reduced row echelon form for those pivots:
 *      row k is the one row with a 1 in the k-th basis column and 0 in the other 90.
 *   4. Candidates, in this order: c0 = the XOR of the rows k whose basis column has hard = 1; c0 ^ M[k],
 *      k = 0 .. 90 (order >= 1); c0 ^ M[k1] ^ M[k2], k1 < k2 in lexicographic order (order 2):
 *      1 + 91 + 4095 candidates.
 *   5. weight(c) = the sum of q[i] over the positions where c differs from hard (int32).  The first
 *      candidate of the smallest weight wins.
 *   6. The winner, in natural bit order, goes through the reference tail as ft8_bp runs it on
 *      plain = codeword with ldpc_errors = 0.  It is accepted when the tail says ok, its hard errors
 *      n_hard = #{i : c[i] != hard[i]} <= max_hard_errors, and the 77 payload bits are not all zero.
 *   7. An accepted candidate's record gets ok = 1, the payload, crc_extracted, crc_calculated,
 *      ldpc_errors = 0 and pass_index |= 0xF0; score, slot, abs_time, abs_freq and cand_index stay, and
 *      every other record stays as it was.
 * One kernel, one 256-thread workgroup per candidate (csrc/osd.hip); no k_bp launch.
 *
 * The setting: order in [0, 2], max_per_slot >= 0 (0: every failed candidate; ft8_decode_batch only),
 * max_hard_errors in [0, 174]; anything else: FT8_E_ARG, the setting unchanged.  Defaults: 2, 0, 36. */
int ft8_set_osd(ft8_ctx* ctx, int32_t order, int32_t max_per_slot, int32_t max_hard_errors);
typedef struct ft8_osd_rec {   /* 12 bytes */
  int32_t weight;          /* the winner's weight; 0 for status 2 and 3 */
  int16_t n_hard;          /* its hard errors; -1 for status 2 and 3 */
  int16_t flip[2];         /* the rows k flipped against c0, -1 where none */
  uint8_t n_flips;         /* 0 .. 2 */
  uint8_t status;          /* 0 accepted; 1 attempted, not accepted; 2 not attempted (rule 1); 3 the record was ok */
} ft8_osd_rec;
/* The stage call, shaped like ft8_ap_decode: d_llr[n][174], d_res[n] records as ft8_bp left them, one list
 * without a per-slot cap.  Every record with ok == 0 is tried with the context's order and max_hard_errors and
 * updated in place.  d_info[n] (nullable): what the attempt found; d_codeword[n][22] (nullable): the winning
 * codeword, MSB first, zeros for status 2 and 3.  n = 0 does nothing.  Caller-owned buffers, no context
 * scratch; the call still takes part in the cross-stream order.
 *
 * FT8_FLAG_OSD inside ft8_decode_batch: last in every chunk, after the coherent passes and the a-priori
 * pass, per slot on the first max_per_slot records still ok == 0 in candidate order, from the STFT LLRs
 * (those the a-priori pass sees).  FT8_E_UNSUPPORTED together with FT8_FLAG_SUBTRACT unless
 * ft8_set_subtract(ctx, n, 1); then it runs in every pass.  ft8_replay_stage refuses after such a batch.
 * Scratch (context-owned, grow-only): 24 bytes per listed candidate (the list, and the compacted positions
 * and scores the list kernel writes) and 4 per slot. */
int ft8_osd_decode(ft8_ctx* ctx, const double* d_llr, ft8_result* d_res, int32_t n, ft8_osd_rec* d_info,
                   uint8_t* d_codeword, void* stream);

/* Per-slot flags of the last selection (copied device->device into d_out[n_slots]):
 * bit 0: an exact score tie reached a heap comparison (the reference raises TypeError there,
 *        ftx_types.py:37-47; here ties are ordered by scan index), bit 1: unused (0), bit 2
 *        (informational): the selected set held equal scores, so the heap sequence was replayed
 *        to order them, bit 3 (informational): that replay ran outside the selection kernel
 *        (beside the LLRs in ft8_decode_batch). */
int ft8_select_warnings(ft8_ctx* ctx, int32_t* d_out, int32_t n_slots, void* stream);

/* ---- float32 belief propagation (build-defined, opt-in; no reference counterpart) --------------------
 * The reference's decoder is float64 because NumPy made it so; the C library it ports is float32.  ft8_bp_f32
 * and FT8_FLAG_BP_F32 run the same algorithm in IEEE binary32 (csrc/bp32.hip, k_bp32: two candidates per
 * wave, packed float32 arithmetic).  With the flag clear nothing changes.  The contract, per candidate
 * (bp32.bp32_restate is its NumPy restatement, bit for bit):
 *   - the 174 input LLRs (double) are rounded to nearest float32 (beyond its range: +-inf; below: subnormal, 0);
 *   - every later operation is IEEE binary32, round to nearest, no FMA contraction, subnormals kept, in the
 *     reference's order (ldpc_decoder.py:54-113): messages = c + ((t0 + t1) + t2); Tnm = c + the other two
 *     tov in kFTX_LDPC_Mn order; toc = fast_tanh(-Tnm / 2) with np.clip to +-4.97 rounded to float32 (NaN
 *     passes); Tmn = the left-to-right product of the check's other toc starting from 1.0f;
 *     tov = -2 fast_atanh(Tmn);
 *   - the all-zero stop, the errors < min_errors rule, the unread update of the last iteration, the CRC-14
 *     tail and every ft8_result field are ft8_bp's.
 * NaN and +-inf LLRs behave as the restatement does.  ft8_bp_f32 has ft8_bp's signature and argument checks;
 * its persistent grid follows ft8_set_pipeline's bp_waves_per_simd (ft8_bp's does not).  In a batch the flag
 * is a property of the batch: OSD reads LLRs only and is unaffected, and ft8_replay_stage replays the kernel
 * that ran. */
int ft8_bp_f32(ft8_ctx* ctx, const double* d_llr, int32_t n, int32_t max_iterations,
               uint8_t* d_plain, ft8_result* d_res, void* stream);

/* ---- small device utilities used by the Python mirror of crc.py / ldpc_check ---------------- */
/* CRC-14 (crc.py:11-39) of d_msg[n][12] over d_nbits[n] bits -> d_crc[n]. */
int ft8_crc14(ft8_ctx* ctx, const uint8_t* d_msg, const int32_t* d_nbits, int32_t n,
              uint16_t* d_crc, void* stream);
/* parity-check error count (ldpc_decoder.py:33-52) of d_bits[n][174] (0/1) -> d_errors[n]. */
int ft8_ldpc_check(ft8_ctx* ctx, const uint8_t* d_bits, int32_t n, int32_t* d_errors,
                   void* stream);

/* ---- transmit chain (ft8_generator) and subtract-and-redecode ------------------------------ */
/* Replaces crc_generator + ldpc_generator + ft8_encode (ft8_generator/crc.py:25-47,
 * ldpc.py:104-131, encoder.py:15-73).  d_msg[n][msg_bytes]: msg_bytes = 10, a payload (77 bits;
 * [9] & 0xF8 is applied) whose a91 = crc_generator(payload); msg_bytes = 12, an a91 taken as given
 * (ldpc_generator's input).  Outputs d_a91[n][12], d_codeword[n][22], d_tones[n][79] (nullable). */
int ft8_encode(ft8_ctx* ctx, const uint8_t* d_msg, int32_t msg_bytes, int32_t n, uint8_t* d_a91,
               uint8_t* d_codeword, uint8_t* d_tones, void* stream);

/* Replaces gfsk_modulation_waveform_generator + ft8_modulation_waveform_generator + ft8_generator
 * (modulator.py:27-90) for a batch: ADDS amplitude * ramp * sin(phi + phase) of every signal to
 * d_out[slot][start .. start + 79 nsps) (clipped to [0, n_samples)), nsps = int(0.16 fs).
 * out_dtype FT8_F32 / FT8_F64 (real) or FT8_C64 / FT8_C128 (the complex baseband
 * amplitude * ramp * (sin - j cos)(phi + phase) of ft8_baseband_generator).  d_tones[n][79];
 * d_signals sorted by slot.  Signals overlapping in a slot are summed in array order. */
int ft8_synthesize(ft8_ctx* ctx, const uint8_t* d_tones, const ft8_tx_signal* d_signals, int32_t n_signals,
                   int32_t sample_rate, int32_t style, void* d_out, int out_dtype, int64_t n_samples,
                   int32_t n_slots, int64_t slot_stride, void* stream);

/* Subtraction step of FT8_FLAG_SUBTRACT (build-defined; no reference counterpart): for each slot,
 * every distinct ok message among d_res[slot][0 .. min(d_counts[slot], cap)) (the records of a
 * ft8_decode_batch with the same params) is re-modulated, its start and tone-0 frequency refined
 * around the candidate's (abs_time, abs_freq), its complex amplitude fitted per symbol, and the
 * fitted waveform subtracted: d_residual[slot][n] = x[slot][n] - sum of fitted signals (float32,
 * row stride slot_stride).  dtype FT8_F32 or FT8_I16 (x / 32767); d_residual may alias F32
 * d_samples. */
int ft8_subtract(ft8_ctx* ctx, const void* d_samples, int dtype, float* d_residual, int64_t n_samples,
                 int32_t n_slots, int64_t slot_stride, const ft8_params* p, const ft8_result* d_res,
                 const int32_t* d_counts, int32_t cap, void* stream);

/* The signals the last subtraction of this context fitted (ft8_subtract, or pass 1 of a two-pass
 * FT8_FLAG_SUBTRACT ft8_decode_batch, whose cap is max_candidates): fit of record r of slot s at
 * d_out[s * cap + r] for r < min(counts[s], cap), copied device -> device.  n_slots and cap must
 * equal that subtraction's.  After an FT8_FLAG_SUBTRACT batch of more than two passes the context
 * holds no valid fits (the scratch was used again by the later subtractions): FT8_E_ARG.  The residual is x - sum over the active fits of
 * ramp(n) Re(A(n) exp(2 pi i phase(n))), A interpolated linearly between symbol centres. */
typedef struct ft8_sub_fit {
  int32_t active;          /* 1: fitted and subtracted; 0: failed record, or a payload an earlier record carries */
  int32_t reserved;
  int64_t start;           /* refined first sample of the 79-symbol waveform (slot sample index) */
  double f0;               /* refined tone-0 frequency, Hz */
  float amp[79][2];        /* complex amplitude per symbol ([1 2 1]-smoothed), (re, im) */
  float phase0[80];        /* carrier phase in cycles (fractional part) at the start of each symbol */
  uint8_t tones[80];       /* the payload's re-encoded tone sequence (79 used) */
} ft8_sub_fit;
int ft8_subtract_fits(ft8_ctx* ctx, ft8_sub_fit* d_out, int32_t n_slots, int32_t cap, void* stream);

/* ---- FT8_FLAG_SUBTRACT with more than two passes, and with the retries in every pass ---------------
 * Opt-in and build-defined (a host-side context setting, like ft8_set_coherent; it takes effect at the
 * next ft8_decode_batch with FT8_FLAG_SUBTRACT).  n_passes in [2, FT8_SUBTRACT_MAX_PASSES], retry 0 or 1;
 * anything else is FT8_E_ARG and leaves the setting as it was.  Default (2, 0).
 *
 * An n-pass batch, per slot, with x_0 the samples and N = max_candidates:
 *   R_k    the records (compacted, capacity N) of the receive path without FT8_FLAG_SUBTRACT on x_{k-1};
 *   acc_1  = R_1;  acc_k = acc_{k-1} followed by the ok rows of R_k whose payload no row of acc_{k-1}
 *          carries (only rows present before the pass count as seen), in R_k order, pass_index |= 1;
 *   x_k    (k < n) = x_{k-1} minus the fits of the rows pass k appended (k = 1: all of R_1): the rows that
 *          are ok and the first of their payload among those rows, fitted on x_{k-1} and subtracted in
 *          record order as ft8_subtract does, in place in the context's float32 residual.
 * d_out / d_counts receive acc_n under max_results_per_slot; the count is uncapped.  n = 2, retry = 0 is the
 * two-pass batch described at FT8_FLAG_SUBTRACT.
 *
 * retry = 0: FT8_FLAG_AP or FT8_FLAG_COHERENT together with FT8_FLAG_SUBTRACT is FT8_E_UNSUPPORTED.
 * retry = 1: every pass runs the retries the flags ask for, as a batch without FT8_FLAG_SUBTRACT would on
 * that pass's input: the coherent pass reads x_{k-1} (from pass 2 on the float32 residual) with the
 * context's cap, drift search and nsym settings, the a-priori pass sees that pass's STFT LLRs.  A row
 * rescued at a drift rate other than 0 (pass_index bit 2) is fitted like any other, WITHOUT a drift term:
 * its subtraction is as good as a constant-frequency fit of it is.
 *
 * Scratch (context-owned, grow-only) per slot: (n - 1) N records (40 B) and fits (ft8_sub_fit, 1056 B) and
 * (n - 1) N + 1 list entries (4 B) for the accumulated rows, N records of the current pass, n counts, and
 * n_samples floats of residual; n = 2 is what the two-pass batch always took.  ft8_snr_last after any such
 * batch stays FT8_E_UNSUPPORTED, and slot_stride >= n_samples as before. */
#define FT8_SUBTRACT_MAX_PASSES 4
int ft8_set_subtract(ft8_ctx* ctx, int32_t n_passes, int32_t retry);

/* d_out[s * n_passes + k] (device, int32) = the uncapped row count of slot s after pass k + 1 of this
 * context's last ft8_decode_batch: rows [count_{k-1}, count_k) of the slot (count_{-1} = 0) are the ones
 * pass k + 1 appended.  The low nibble of pass_index is full, so the pass number is reported here and not
 * in the record.  FT8_E_ARG unless that batch ran FT8_FLAG_SUBTRACT (and had something to search) with
 * these n_slots and n_passes. */
int ft8_subtract_counts(ft8_ctx* ctx, int32_t* d_out, int32_t n_slots, int32_t n_passes, void* stream);

/* ---- frequency-drift correction (ft8_beacon_receiver/frequency_correction.py) -------------
 * Paths below are relative to src/ft8_tools/ft8_beacon_receiver/.  Parameters of
 * correct_frequency_drift (frequency_correction.py:118-163); fields default to the reference's
 * default_params when the Python mirror fills them. */
typedef struct ft8_drift_params {
  double sample_rate;          /* fs, Hz (integral) */
  double sym_bin;              /* symbol frequency spacing, Hz (6.25) */
  double sym_t;                /* symbol time, s (0.16) */
  double max_variance_factor;  /* max_variance = factor * freq_bins^2 */
  int32_t bins_per_tone;       /* freq_osr */
  int32_t steps_per_symbol;    /* time_osr */
  int32_t nsync_sym, ndata_sym;
  int32_t window_size_factor;  /* window_size = factor * steps_per_symbol */
  int32_t fit_middle_percent;
  int32_t poly_degree;
  int32_t precise_sync;
} ft8_drift_params;

/* how correct_frequency_drift returned (frequency_correction.py line of the return) */
enum ft8_drift_status {
  FT8_DRIFT_PENDING = 0,       /* stage 1 done, stage 2 not yet run */
  FT8_DRIFT_NO_SEGMENT = 1,    /* :236  no continuous segment: the input is returned, rate 0 */
  FT8_DRIFT_LINEAR = 2,        /* :359  precise_sync off: linear compensation only */
  FT8_DRIFT_FEW_POINTS = 3,    /* :523  < 10 sync regression points: linear compensation */
  FT8_DRIFT_DEGREE = 4,        /* :631  poly_degree not 1 or 2: linear compensation */
  FT8_DRIFT_FULL = 5,          /* :655  linear + polynomial compensation */
  FT8_DRIFT_UNDERDETERMINED = 6, /* :659 points <= poly_degree + 1: linear compensation */
  FT8_DRIFT_VALUE_ERROR = -1  /* the reference raises ValueError inside LinearRegression.fit
                                 (:337 an empty segment, :539 regression x/y lengths differ) */
};

/* Per-slot outcome, 72 bytes. */
typedef struct ft8_drift_result {
  double rate_per_sample;      /* correct_frequency_drift's second return value */
  double rate1;                /* f_shift_rate of the linear pass, Hz/s (:348) */
  double coef[3];              /* coefs_final[0..2] of the polynomial fit (coef[0] = 0) */
  double intercept;            /* intercept_final */
  int32_t status;              /* ft8_drift_status */
  int32_t n_segments;          /* continuity segments found (detect_signal_continuity) */
  int32_t seg_start, seg_end;  /* longest segment (max by end - start, first on ties) */
  int32_t sync_idx;            /* correlation_peak_time_block_index (:463) */
  int32_t n_points;            /* regression points of the polynomial fit */
} ft8_drift_result;

/* calculate_spectrogram -> kept bins -> np.argmax over frequency per frame, without writing the
 * waterfall (the argmax is fused into the STFT epilogue): d_idx[n_slots][t_hi - t_lo] = the first
 * bin index (relative to f_lo) of the largest dB value of each frame (frequency_correction.py:
 * 190-224, 364-384).  Samples and params as for ft8_stft. */
int ft8_stft_argmax(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                    int64_t slot_stride, const ft8_params* p, int32_t* d_idx, void* stream);

/* The two estimation stages on per-frame argmax indices d_idx[n_slots][T] (F = kept bins):
 * stage 1: detect_signal_continuity (:42-115) + longest segment + linear fit (:227-348) -> d_res
 *          (d_metric[n_slots][T - window + 1], nullable: the continuity metric; d_segments
 *          [n_slots][max_segments][2], nullable: the first max_segments segments);
 * stage 2: d_idx of the linearly compensated signal -> sync correlation (:386-463) + polynomial
 *          fit (:502-590) -> d_res (which must hold the stage-1 result). */
int ft8_drift_fit(ft8_ctx* ctx, int32_t stage, const int32_t* d_idx, int32_t n_slots, int32_t T, int32_t F,
                  const ft8_drift_params* p, ft8_drift_result* d_res, double* d_metric, int32_t* d_segments,
                  int32_t max_segments, void* stream);

/* Replaces correct_frequency_drift (frequency_correction.py:118-659) for a batch of independent
 * signals: STFT-argmax -> stage 1 -> linear de-rotation -> STFT-argmax -> stage 2 -> polynomial
 * de-rotation, all on the device.  d_samples: dtype F32/F64/C64/C128, row stride slot_stride
 * elements.  d_out: complex128 [n_slots][n_samples] (for FT8_DRIFT_NO_SEGMENT the input converted
 * to complex128).  d_res[n_slots].  De-rotation carriers: :352 and :598-611. */
int ft8_drift_correct(ft8_ctx* ctx, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                      int64_t slot_stride, const ft8_drift_params* p, void* d_out, ft8_drift_result* d_res,
                      void* stream);

/* ---- FT4 -------------------------------------------------------------------------------------------
 * Build-defined, outside reference parity: the reference decodes FT8 only, and no vector of another FT4
 * implementation was available to the build.  The constants are the published protocol's as the build
 * states them below; INTEROPERABILITY WITH WSJT-X IS NOT VERIFIED.  ft8_demodulator_amd/ft4.py restates
 * every stage in NumPy and the tests pin the device to it bit for bit.
 *   symbol      T = 0.048 s: nsps = fs * 6 / 125 samples, which must be an integer (12 000 Hz: 576; 44 100 Hz:
 *               FT8_E_UNSUPPORTED).  Tone spacing fs / nsps (20.8333 Hz), 4-FSK, modulation index 1.
 *   STFT        nperseg = nsps, hop = nsps / steps_per_symbol (the reference's noverlap rule), nfft =
 *               nsps * bins_per_tone, periodic Hann, the same dB formula.
 *   frame       103 symbols S4 D29 S4 D29 S4 D29 S4.  Sync group m = 0 .. 3 starts at symbol 33 m with the
 *               tones {0,1,3,2}, {1,0,2,3}, {2,3,1,0}, {3,2,0,1}.  Data symbol k (0 .. 86) sits at k + 4
 *               (k < 29), k + 8 (k < 58), else k + 12; Gray map {0,1,3,2}, two bits per symbol, MSB first.
 *   scrambling  the 77 message bits are XORed with rvec = 4a 5e 89 b4 b0 8a 79 55 be 28 (MSB first, 77 bits)
 *               before CRC-14 and LDPC(174,91); the receiver XORs the decoded 77 bits again.  CRC and parity
 *               are over the scrambled bits.
 *   waveform    105 symbols: a ramp-up symbol, the 103, a ramp-down symbol.  GFSK with the frequency pulse
 *               of ft8_synthesize at BT = 1.0 (length 3 nsps): symbol j's pulse covers the samples
 *               [(j - 1) nsps, (j + 2) nsps) relative to the start of symbol 0.  No extension pulses: the
 *               ramp symbols carry tone 0 plus their neighbours' tails.  Envelope (1 - cos(pi i / nsps)) / 2
 *               over the first symbol, its mirror over the last, 1 between.  The phase is 0 at the
 *               waveform's first sample and the real part is sin.
 *   sync score  ft8_sync_score with the layout swapped: m = 0 .. 3 outer, k = 0 .. 3 inner, block = 33 m + k,
 *               tone = Costas[m][k]; the block test is on floor(abs_time / sps) + block against
 *               num_blocks = T / sps; the terms are tone - 1 (tone > 0), tone + 1 (tone < 3), time - 1 (k > 0
 *               and block_abs > 0), time + 1 (k < 3 and block_abs + 1 < num_blocks), each added one after
 *               another in the waterfall dtype, the sum divided by the term count; -inf for no terms or a
 *               NaN or infinite sum.  Grid: abs_time in [-10 sps, (num_blocks - 83) sps), abs_freq in
 *               [0, F - 3 bpt).
 *   selection   unchanged (the heap rule, or FT8_FLAG_TOPK).
 *   LLRs        per data symbol s[j] = wf[row][abs_freq + Gray[j] bpt] in double, L[2k] = max(s2, s3) -
 *               max(s0, s1), L[2k+1] = max(s1, s3) - max(s0, s2); both 0 where the symbol's block lies
 *               outside [0, num_blocks); then ftx_normalize_logl unchanged.
 *   back end    unchanged (ft8_bp, the a-priori and OSD passes).  ft8_result.payload of a decode of
 *               ft8_decode_batch holds the DESCRAMBLED message bits; crc_* are the transmitted (scrambled)
 *               frame's.  ft8_bp's own records carry scrambled bits (ft8_ft4_unscramble).
 * ft8_params.protocol = FT8_PROTO_FT4 is honoured by ft8_stft (geometry only), ft8_sync_select and
 * ft8_decode_batch.  In an FT4 batch FT8_FLAG_TOPK and FT8_FLAG_OSD work unchanged; FT8_FLAG_AP works with the
 * context's hypotheses in MESSAGE bits (every AP launch takes a copy whose value is XORed with rvec, so the
 * clamp and the acceptance both work on scrambled bits); FT8_FLAG_COHERENT and FT8_FLAG_SUBTRACT are
 * FT8_E_UNSUPPORTED, as are ft8_stft_argmax, ft8_subtract, ft8_snr, ft8_coherent_*llr with an FT4 block and
 * ft8_snr_last after an FT4 batch (follow-ups: DESIGN.md section 15).  ft8_replay_stage after an FT4 batch is
 * FT8_E_ARG: the descramble step is an involution, not idempotent. */
#define FT8_PROTO_FT8 0
#define FT8_PROTO_FT4 1
#define FT8_FT4_SYMBOLS 103
/* ft8_geometry_hz for a protocol (host only).  FT8_E_ARG for an unknown protocol, FT8_E_UNSUPPORTED for an FT4
 * sample rate whose symbol is no whole number of samples. */
int ft8_geometry_proto(int32_t protocol, double sample_rate_hz, int32_t bins_per_tone, int32_t steps_per_symbol,
                       int64_t n_samples, int32_t* nperseg, int32_t* hop, int32_t* nfft, int32_t* n_frames);
/* ft8_llr for FT4: d_cand[n][3] = (slot, abs_time, abs_freq) -> d_llr[n][174] (double). */
int ft8_ft4_llr(ft8_ctx* ctx, const void* d_wf, int wf_f64, int32_t T, int32_t F, int32_t steps_per_symbol,
                int32_t bins_per_tone, const int32_t* d_cand, int32_t n, int normalize, double* d_llr,
                void* stream);
/* XORs rvec onto the 77 payload bits of d_res[0 .. n) in place; nothing else of a record changes and the low
 * 3 bits of payload[9] stay.  ft8_decode_batch runs it on its output; it is a stage call because ft8_bp's
 * records carry scrambled bits.  Its own inverse. */
int ft8_ft4_unscramble(ft8_ctx* ctx, ft8_result* d_res, int32_t n, void* stream);
/* ft8_encode for FT4: d_msg[n][10] payloads (77 bits; [9] & 0xF8 is applied) -> d_a91[n][12] (scrambled
 * payload | CRC-14), d_codeword[n][22], d_tones[n][103]; each output nullable. */
int ft8_ft4_encode(ft8_ctx* ctx, const uint8_t* d_msg, int32_t n, uint8_t* d_a91, uint8_t* d_codeword,
                   uint8_t* d_tones, void* stream);
/* ft8_synthesize for FT4 (its contract: ADDS into d_out in array order, the same dtypes, d_signals sorted by
 * slot): d_tones[n][103]; ft8_tx_signal.start is the first sample of symbol 0, so a signal covers
 * [start - nsps, start + 104 nsps).  FT8_E_UNSUPPORTED for a sample rate FT4 does not take. */
int ft8_ft4_synthesize(ft8_ctx* ctx, const uint8_t* d_tones, const ft8_tx_signal* d_signals, int32_t n_signals,
                       int32_t sample_rate, void* d_out, int out_dtype, int64_t n_samples, int32_t n_slots,
                       int64_t slot_stride, void* stream);

/* ---- build provenance --------------------------------------------------------------------- */
/* SHA-256 prefix of the sources, headers and Makefile the library was compiled from (the Python
 * binding recomputes it from the tree and refuses a stale library), and the effective compile
 * flags of every object.  No reference counterpart. */
const char* ft8_build_id(void);
const char* ft8_build_flags(void);

/* ---- benchmarking: re-launch one kernel of the last ft8_decode_batch -------------------------
 * Re-launches, reps times on `stream`, the kernel of `stage` (0 stft, 1 score, 2 select, 6 llr,
 * 3 bp, 4 compact) exactly as the last single-chain ft8_decode_batch of this context launched it
 * (same buffers, same arguments; every stage is idempotent on its inputs), so a kernel's duration
 * can be measured by wall clock over back-to-back launches, without events between stages.  Valid
 * while the caller's buffers of that call are alive and until any other entry point of this
 * context runs (FT8_E_ARG otherwise, and after an FT8_FLAG_SUBTRACT, FT8_FLAG_AP, FT8_FLAG_COHERENT
 * or FT8_FLAG_OSD batch, whose stages are not idempotent).  No reference counterpart. */
int ft8_replay_stage(ft8_ctx* ctx, int32_t stage, int32_t reps, void* stream);

/* ---- per-stage device timing (HIP events on the caller's stream) --------------------------- */
#define FT8_N_STAGES 12 /* 0 stft, 1 score, 2 select, 3 bp, 4 compact, 5 whole decode_batch, 6 llr,
                         7 subtraction fits (k_sub_est), 8 drift STFT-argmax, 9 drift fits,
                         10 drift de-rotation, 11 subtraction of the fitted signals (k_sub_apply) */
int ft8_set_timing(ft8_ctx* ctx, int enable);
/* which stages record events while timing is enabled (bit s = stage s; default all): timing one
 * stage at a time brackets only that kernel, so the rest of the step runs undisturbed */
int ft8_set_timing_stages(ft8_ctx* ctx, uint32_t mask);
/* accumulated milliseconds and launch counts per stage since the last reset; synchronises. */
int ft8_get_timing(ft8_ctx* ctx, double* ms, int64_t* launches, int reset);
/* BP work counters, accumulated while timing is enabled: out4 = {candidates decoded, BP
 * iterations entered, message-passing sweeps executed, candidates converged}; synchronises. */
int ft8_get_counters(ft8_ctx* ctx, int64_t* out4, int reset);
/* k_bp's own clock, accumulated over launches made while timing is enabled (each persistent wave
 * reads the shader-clock and the constant-rate wall-clock counters when it starts and when it
 * retires): out5 = {sum of wave lifetimes in shader cycles, the same in wall-clock ticks, the
 * longest wave lifetime in cycles, waves, wall-clock rate in kHz}.  Cycles per launch do not depend
 * on the box's clock; cycles / wall time is the clock k_bp ran at.  Synchronises.  (No reference
 * counterpart: measurement of ldpc_decoder.py:54-113's replacement.) */
int ft8_get_bp_clock(ft8_ctx* ctx, int64_t* out5, int reset);

#ifdef __cplusplus
}
#endif
#endif /* FT8HIP_H */
