/*
 * include/kws.h -- C ABI of the MI355X-native keyword-spotting hot path.
 *
 * The reference (david8862/tf-keras-speech-commands) has no FFI of its own: its
 * hot path is Python calling sonopy and tf.keras.  This header is the boundary
 * a maintainer would bind from that Python with ctypes;
 * every entry point names the reference interface it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no torch / C++ types; all array arguments are caller-owned
 *     DEVICE pointers (row-major, float32 unless stated); `stream` is a
 *     hipStream_t passed as void* (NULL = default stream);
 *   - every int-returning function returns KWS_OK (0) or a negative kws_status;
 *     kws_last_error() gives the message for the calling thread;
 *   - work is only enqueued on `stream`; nothing synchronises the device;
 *   - there is no CPU fallback: without a HIP device the create/launch calls
 *     fail with KWS_ERR_HIP.
 */
#ifndef KWS_H
#define KWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum kws_status {
    KWS_OK = 0,
    KWS_ERR_INVALID = -1,     /* bad argument / inconsistent params              */
    KWS_ERR_UNSUPPORTED = -2, /* valid in the reference, not built here yet      */
    KWS_ERR_HIP = -3,         /* HIP runtime error (no device, launch failure)   */
    KWS_ERR_NOMEM = -4,
    KWS_ERR_WORKSPACE = -5,   /* caller's workspace too small                    */
    KWS_ERR_COMM = -6         /* RCCL missing or a collective failed             */
} kws_status;

const char *kws_version(void);
/* "<source file>:<sha1 prefix>;..." of every file the library was built from (measurement records in profiles/ are tied to it) */
const char *kws_build_id(void);
const char *kws_last_error(void);
/* number of visible HIP devices (0 when none / no driver); never fails */
int kws_device_count(void);

/* Opt-in per-kernel timing: while enabled every kernel launched through this library is bracketed by HIP
 * events on its launch stream.  kws_prof_enable(1) clears and starts, (0) stops and clears;
 * kws_prof_report synchronises the recorded events and writes a JSON object
 * {"<kernel>": {"count": n, "total_ms": t}, ...} into buf; returns the bytes needed (incl. NUL). */
int kws_prof_enable(int on);
int64_t kws_prof_report(char *buf, size_t buflen);

/* ------------------------------------------------------------------------
 * Audio-pipeline parameters: the numeric fields of ListenerParams
 * (classifier/params.py:49-59) as read from params.json (configs/params.json).
 * ---------------------------------------------------------------------- */
typedef struct kws_params {
    double buffer_t, window_t, hop_t;
    int32_t sample_rate, sample_depth, n_fft, n_filt, n_mfcc, use_delta;
} kws_params;

/* derived properties, classifier/params.py:59-91 */
typedef struct kws_geometry {
    int32_t window_samples, hop_samples, max_samples, buffer_samples, n_features, feature_size;
} kws_geometry;

/* defaults of classifier/params.py:99-103 */
void kws_params_default(kws_params *p);
/* host-only; KWS_ERR_INVALID if the parameters are unusable */
int kws_params_derive(const kws_params *p, kws_geometry *g);

/* ------------------------------------------------------------------------
 * Featurizer: replaces common/data_utils.py:73-86 audio_to_feature (and with
 * it vectorize_raw :61-70 = sonopy.mfcc_spec, and add_deltas :50-58), batched.
 * KWS_BANK_BARK swaps in the filterbank of common/bark_feature.py:92-136
 * (bfcc_spec :156-175).
 * ---------------------------------------------------------------------- */
typedef enum kws_bank_kind { KWS_BANK_MEL = 0, KWS_BANK_BARK = 1 } kws_bank_kind;
typedef enum kws_wav_dtype {
    KWS_WAV_F32 = 0, /* float32 in [-1,1), what librosa.load returns (data_utils.py:93) */
    KWS_WAV_I16 = 1  /* raw little-endian PCM16, scaled by 1/32768 (data_utils.py:21)     */
} kws_wav_dtype;

typedef struct kws_featurizer kws_featurizer;

int kws_featurizer_create(const kws_params *p, int bank_kind, kws_featurizer **out);
void kws_featurizer_destroy(kws_featurizer *f);
/* geometry the featurizer was built for */
int kws_featurizer_geometry(const kws_featurizer *f, kws_geometry *g);
/* host copy of the dense (n_filt x (n_fft/2+1)) bank the sparse tables were built from */
int kws_featurizer_bank(const kws_featurizer *f, float *host_bank, size_t count);

/*
 * wav      : (B, stride) samples of `wav_dtype`; row b holds clip b from its first sample
 * valid_len: NULL (every clip has `stride` samples) or B DEVICE int32 clip lengths
 *            (0 <= len <= stride).  Per clip the reference's contract applies: keep
 *            the FIRST max_samples (data_utils.py:77), LEFT-pad with zeros when
 *            shorter (:79-80).
 * feat     : (B, n_features, feature_size) float32
 */
int kws_featurize(kws_featurizer *f, const void *wav, int wav_dtype, int B, int64_t stride,
                  const int32_t *valid_len, float *feat, void *stream);
/* The same for B clips GATHERED from a device-resident dataset: clip b is row index[b] (device int32) of `wav` (rows x stride) and of
 * `valid_len` (one length per ROW).  This is the minibatch draw of model.fit(shuffle=True) (train.py:81-92) without a copy of the
 * audio: the reference's fit gathers feature rows on the host; here a step's 4096 x 64 KB of samples are read in place. */
int kws_featurize_gather(kws_featurizer *f, const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride,
                         const int32_t *valid_len, float *feat, void *stream);

/*
 * vectorize_raw (common/data_utils.py:61-70): audio of exactly n_samples per clip, no length
 * clipping, no padding, no deltas.  feat: (B, n_frames, n_mfcc) with
 * n_frames = kws_featurize_raw_frames(f, n_samples) = (n_samples - window)/hop + 1 (0 if shorter).
 */
int kws_featurize_raw_frames(const kws_featurizer *f, int32_t n_samples);

int kws_featurize_raw(kws_featurizer *f, const void *wav, int wav_dtype, int B, int64_t stride, int32_t n_samples,
                      float *feat, void *stream);

/*
 * vectorize_raw of R whole recordings of ragged length in one launch: row j of recording r is vectorize_raw of its samples
 * [j hop, j hop + window), i.e. the row Listener.update_vectors (listen.py:96-114) appends once those samples have arrived.
 *   wav     : (R, stride) samples of `wav_dtype`, recording r from its first sample
 *   lengths : R DEVICE int32 sample counts (clamped to 0..stride)
 *   rows    : (R, max_frames, n_mfcc); recording r has kws_featurize_raw_frames(f, lengths[r]) rows (at most max_frames are
 *             written), the rows after them are written as zeros
 * Work is cut into (recording, tile of frames) jobs, so one long recording fills the device and no length is refused: the
 * default geometry runs the tuned kernel's own frame loop per tile (a row has the bits kws_featurize_raw gives the same samples);
 * other geometries go through the clip kernels as overlapping segments (stream-ordered scratch of about the audio's size).
 */
int kws_featurize_long(kws_featurizer *f, const void *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths,
                       int max_frames, float *rows, void *stream);

/* How much of every compute unit one launch of the tuned (default-geometry) kernel may hold.  2 (default): two persistent blocks of
 * 8 waves per CU (4 waves per SIMD, 2 x 52 KB of LDS), fastest when the featurizer has the chip to itself (inference, dataset
 * featurization); 1: ONE block of 12 waves (75 KB of LDS), so that kernels of OTHER streams still find wave slots and LDS on every
 * CU -- use it when a batch is featurized beside a running train step (kws_train_args.overlap_event).  Same arithmetic, same bits.
 * Other geometries (generic kernels) ignore it. */
int kws_featurizer_set_cu_share(kws_featurizer *f, int blocks_per_cu);

/* Diagnostics: resident blocks (= clips) per compute unit the runtime reports for the float32 featurizer kernel at this
 * featurizer's LDS size, and that LDS size in bytes.  No reference counterpart; used by tools/ and DESIGN.md. */
int kws_featurizer_occupancy(const kws_featurizer *f, int *blocks_per_cu, size_t *lds_bytes);

/* ------------------------------------------------------------------------
 * Background-noise augmentation of raw audio: the mix of tools/audio_process/add_noise.py:19-35, drawn afresh for every clip of every
 * train step on the device instead of written once as *_noised.wav copies.  Per clip (voice v of valid length Lv, clipped to max_samples
 * as the featurizer does):
 *   noised:   L = min(Lv, seg_len[k]); p_v = mean(v[0:L]^2), p_n = mean(n_k[o:o+L]^2);
 *             g = sqrt(p_v / 10^(s/10) / (p_n + FLT_EPSILON)); m[t] = v[t] + g n_k[o+t], t < L
 *   otherwise m = v[0:Lv], L = Lv
 *   time shift (no counterpart in the reference): m'[t] = m[t - d] where 0 <= t - d < L, else 0; length L
 * m' is then featurized with the keep-head / left-pad rule on length L.  Divergences from the offline tool: no int16 quantisation or
 * clipping of the mixed clip, the voice power is taken over the head the featurizer keeps, draws are fresh every step.
 * ---------------------------------------------------------------------- */
typedef struct kws_noise_bank kws_noise_bank;

/* K recordings (add_noise.py: noise_files), concatenated on the HOST: samples[sum(seg_len)] of wav_dtype (int16 is scaled by 1/32768 as
 * the featurizer does), seg_len[K] >= 1 each.  Uploads them with an fp64 prefix sum of squares (the power of any window in O(1)). */
int kws_noise_bank_create(const void *samples, int wav_dtype, const int32_t *seg_len, int K, kws_noise_bank **out);
void kws_noise_bank_destroy(kws_noise_bank *bank);
/* host: number of segments, total samples, and (seg_len may be NULL) the K segment lengths */
int kws_noise_bank_info(const kws_noise_bank *bank, int *K, int64_t *total, int32_t *seg_len);

#define KWS_AUG_MAX_SNR 16
typedef struct kws_augment_params {
    float noised_rate;                 /* add_noise.py --noised_rate: fraction of clips noised, [0, 1] */
    int32_t n_snr;                     /* 1..KWS_AUG_MAX_SNR */
    float snr_db[KWS_AUG_MAX_SNR];     /* add_noise.py --snr: choice(snr_list) */
    int32_t max_shift;                 /* time shift d uniform in [-max_shift, max_shift] samples; 0 = off */
    int32_t max_samples;               /* the head the featurizer keeps (kws_geometry.max_samples) */
    uint64_t seed;
} kws_augment_params;

/* one clip's augmentation (32 bytes, device memory) */
typedef struct kws_aug_clip {
    int32_t apply;        /* 1: noised */
    int32_t segment;      /* k: choice(noise_files) */
    int32_t offset;       /* o: start of the noise window in segment k */
    int32_t shift;        /* d */
    int32_t length;       /* L (filled by kws_augment_plan) */
    float snr_db;         /* s: choice(snr_list) */
    float gain;           /* g (filled by kws_augment_plan; 0 when not noised) */
    int32_t voice_length; /* Lv (filled by kws_augment_plan) */
} kws_aug_clip;

/* Plan B clips, one wave per clip, no host synchronisation.  Clip b is row index[b] (device int32; NULL: row b) of wav (rows x stride)
 * with valid_len[row] samples (device int32; NULL: stride).  Draws are counter-based, keyed by (params->seed, step) and indexed by the
 * clip's global position position_base + b (a data-parallel shard plans with position_base = its first position): apply = u <
 * noised_rate, k, s, o uniform in [0, seg_len[k] - L], d uniform in [-max_shift, max_shift].  explicit_plan (HOST, B records, or NULL):
 * take apply / segment / offset / shift / snr_db from the caller instead (an offset past seg_len[k] - L is clamped to it); L, gain and
 * voice_length are computed either way.  plan: B device records.
 * KWS_ERR_INVALID: an SNR outside [-200, 200] dB, in params->snr_db or in an explicit record (the message names the list entry or the
 * clip).  At +-200 dB and |v| <= 1 the gain is at most 2.9e13, finite in float32 with 25 orders of magnitude to spare, and nothing real
 * needs more; from -702 dB on a full-scale voice over silent noise gives g = inf and a mix of inf and NaN. */
int kws_augment_plan(const kws_noise_bank *bank, const kws_augment_params *params, const void *wav, int wav_dtype, const int32_t *index,
                     int B, int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, kws_aug_clip *plan,
                     const kws_aug_clip *explicit_plan, void *stream);

/* Materialise the planned clips m' (what the model trains on): out (B x out_stride float32, out_stride >= max_samples) holds m'[0:L]
 * head-aligned, zeros after, out to out_stride as every wave stage fills its rows; lengths (device int32 B, may be NULL) = L.
 * featurize(out, valid_len = lengths) equals kws_featurize_gather_augmented bit for bit. */
int kws_augment_apply(const kws_noise_bank *bank, const kws_aug_clip *plan, const void *wav, int wav_dtype, const int32_t *index, int B,
                      int64_t stride, int max_samples, float *out, int64_t out_stride, int32_t *lengths, void *stream);

/* kws_featurize_gather of the planned clips m' (lengths from the plan; the plan must have been made with this featurizer's
 * max_samples).  The default geometry mixes in the tuned kernel's sample loads; other geometries run apply + featurize. */
int kws_featurize_gather_augmented(kws_featurizer *f, const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride,
                                   const kws_noise_bank *bank, const kws_aug_clip *plan, float *feat, void *stream);

/* ------------------------------------------------------------------------
 * Room-reverberation augmentation of raw audio: the convolution of tools/audio_process/audio_reverberation.py (pyroomacoustics) and
 * gpuRIR_reverberation.py of the reference with a room impulse response (RIR), drawn afresh for every clip of every train step on the
 * device instead of written once as *_reverb.wav copies.  Clip b sits at global batch position p = position_base + b; its dry signal v
 * is row index[b] of wav (int16 scaled by 1/32768), Lv = min(valid_len[row] or stride, max_samples).  Draws: h_f = aug_hash(seed, step,
 * 2 p + f) (kws_augment.h; kws_amd passes seed_r = WaveAugment seed ^ 0x9E3779B97F4A7C15, so the noise draws are unchanged):
 *   f = 0: wet = ((h_0 >> 8) * 2^-24) < reverb_rate;  f = 1: k = aug_uniform(h_1, K)
 *   wet:  L' = min(Lv + Lh_k - 1, max_samples) (0 when Lv = 0); y[t] = sum_{j <= min(t, Lh_k - 1)} h_k[j] v[t - j], t < L' (v[u] = 0 for
 *         u >= Lv): causal, starting at the direct path; the tail lengthens a short clip up to max_samples.  rescale: y *= sqrt(E_v /
 *         (E_y + Lv FLT_EPSILON)), E = sum of squares over t < Lv (the clip keeps its level, so a later SNR draw means what it says)
 *   dry:  L' = Lv, y = v (bit for bit after the f32 conversion)
 * Reverb runs first; the noise stage (kws_augment_plan and the fused featurizer, time shift included) then runs unchanged on (out,
 * lengths) with index = NULL and the same position_base.  Divergences from the reference: the noise is mixed after the reverberation
 * (the reference places it as a second source in the same room); a single omni microphone (the reference records a 3-mic array that
 * librosa.load(mono=True) averages); no int16 quantisation of the result; fresh draws every step.
 * ---------------------------------------------------------------------- */
typedef struct kws_rir_bank kws_rir_bank;

/* K RIRs concatenated on the HOST: taps[sum(rir_len)] float32, rir_len[K] >= 1 each, finite.  Taps at index >= max_samples can never
 * reach an output sample and are clipped away (Lh = min(rir_len, max_samples)).  Every clipped RIR is transformed once (fp64 on the
 * host) into the spectrum the kernel multiplies by; the clipped taps are kept on the device as well, for the clips of at most 64
 * samples, which are convolved directly in fp64.  max_samples in [1, 16384] (KWS_ERR_UNSUPPORTED above: one 32768-point transform). */
int kws_rir_bank_create(const float *taps, const int32_t *rir_len, int K, int max_samples, kws_rir_bank **out);
void kws_rir_bank_destroy(kws_rir_bank *bank);
/* host: number of RIRs, the bank's max_samples and the real transform size (32768) */
int kws_rir_bank_info(const kws_rir_bank *bank, int *K, int *max_samples, int *fft_size);

typedef struct kws_reverb_params {
    float reverb_rate;     /* fraction of clips reverberated, [0, 1] */
    int32_t rescale;       /* 1: keep the dry clip's energy over t < Lv */
    int32_t max_samples;   /* the head the featurizer keeps, [1, 16384] */
    int32_t reserved;      /* 0 */
    uint64_t seed;         /* seed_r */
} kws_reverb_params;

/* Reverberate B clips, no host synchronisation (explicit_rir is copied from the host first).  out: B x out_stride float32
 * (out_stride >= max_samples), row b = y[0:L'] then zeros; lengths (device int32 B, required) = L'; rir_used (device int32 B, may be
 * NULL) = k, or -1 for a dry clip.  explicit_rir (HOST int32 B, values -1..K-1, or NULL): take k (-1 = dry) from the caller instead of
 * the draws.  Fixed reduction order and no atomics: two calls give the same bits. */
int kws_reverb_apply(const kws_rir_bank *bank, const kws_reverb_params *params, const void *wav, int wav_dtype, const int32_t *index,
                     int B, int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const int32_t *explicit_rir,
                     float *out, int64_t out_stride, int32_t *lengths, int32_t *rir_used, void *stream);

/* ------------------------------------------------------------------------
 * Butterworth filter augmentation of raw audio: tools/audio_process/wav_filter.py of the reference (scipy.signal.butter(order, Wn, type),
 * Wn = 2 f / sample_rate, applied with zero phase by scipy.signal.filtfilt(b, a, x)), drawn afresh for every clip of every train step on
 * the device instead of written once as filtered copies.  Clip b sits at global batch position p = position_base + b; its dry signal v
 * is row index[b] of wav (int16 scaled by 1/32768), Lv = min(valid_len[row] or stride, max_samples).  Draws: h_f = aug_hash(seed, step,
 * 2 p + f) (kws_augment.h; kws_amd passes seed_f = WaveAugment seed ^ 0xD1B54A32D192ED03, so the noise and reverb draws are unchanged):
 *   f = 0: filtered = ((h_0 >> 8) * 2^-24) < filter_rate;  f = 1: k = aug_uniform(h_1, K)
 *   filtered, Lv > padlen_k: y[0:Lv] = filtfilt of v[0:Lv] with scipy's defaults: the odd extension ext of padlen_k samples on each side
 *         (ext[i] = 2 v[0] - v[padlen - i], ext[padlen + Lv + j] = 2 v[Lv-1] - v[Lv-2-j]); the forward pass runs the cascade from
 *         zi_k * ext[0], the backward pass over the reversed forward output from zi_k * y_fwd[last]; cropped back to Lv, zeros after.
 *         rescale: y *= sqrt(E_v / (E_y + Lv FLT_EPSILON)), E = sum of squares over t < Lv (a later SNR draw means what it says)
 *   dry (not drawn, or Lv <= padlen_k, where scipy raises): y = v (bit for bit after the f32 conversion), filter_used = -1
 *   lengths = Lv either way.
 * Order of stages: reverb (kws_reverb_apply), then this filter on its (out, lengths) with index = NULL, then the noise stage (time shift
 * included), all with the same position_base.  Divergences from the reference: only the featurizer's head (max_samples) is filtered, not
 * the whole file; no int16 quantisation of the result; the noise is not filtered; fresh draws every step; short clips stay dry instead
 * of raising.
 * ---------------------------------------------------------------------- */
#define KWS_FILTER_MAX_SECTIONS 4      /* lowpass / highpass up to order 8, bandpass / bandstop up to order 4 */
#define KWS_FILTER_MAX_PADLEN 32       /* filtfilt's default 3 (n + 1) is at most 27 within the section limit */
#define KWS_FILTER_MAX_SAMPLES 16320   /* max_samples + 2 padlen fits the kernel's 64 chunks of 256 samples */
typedef struct kws_filter_bank kws_filter_bank;

/* K filters as second-order sections on the HOST, float64: sos[K][n_sections][6] = (b0, b1, b2, a0, a1, a2) per section (scipy's
 * output='sos'; a filter of fewer sections is padded with (1, 0, 0, 1, 0, 0)), n_sections in [1, KWS_FILTER_MAX_SECTIONS]
 * (KWS_ERR_UNSUPPORTED above), padlen[K] in [1, KWS_FILTER_MAX_PADLEN] (filtfilt's 3 max(len(a), len(b))).  Every section must be finite,
 * a0 != 0 and stable (both poles inside the unit circle).  The steady-state initial conditions zi (scipy's sosfilt_zi) and the powers
 * A^(2^e) of the cascade's state matrix the kernel's chunk scan needs are computed here in float64, and the device filters in float64
 * (samples stay float32 in memory). */
int kws_filter_bank_create(const double *sos, int n_sections, const int32_t *padlen, int K, kws_filter_bank **out);
void kws_filter_bank_destroy(kws_filter_bank *bank);
/* host: number of filters, sections per filter, and padlen[K] (may be NULL) */
int kws_filter_bank_info(const kws_filter_bank *bank, int *K, int *n_sections, int32_t *padlen);

typedef struct kws_filter_params {
    float filter_rate;     /* fraction of clips filtered, [0, 1] */
    int32_t rescale;       /* 1: keep the dry clip's energy over t < Lv */
    int32_t max_samples;   /* the head the featurizer keeps, [1, KWS_FILTER_MAX_SAMPLES] */
    int32_t reserved;      /* 0 */
    uint64_t seed;         /* seed_f */
} kws_filter_params;

/* Filter B clips, no host synchronisation (explicit_filter is copied from the host first).  out: B x out_stride float32 (out_stride >=
 * max_samples), row b = y[0:Lv] then zeros; lengths (device int32 B, required; may be valid_len itself when index is NULL) = Lv;
 * filter_used (device int32 B, may be NULL unless explicit_filter is given) = k, or -1 for a dry clip.  explicit_filter (HOST int32 B,
 * values -1..K-1, or NULL): take k (-1 = dry) from the caller instead of the draws.  In place (out == wav) needs float32 input, index
 * NULL and out_stride == stride.  Fixed reduction order and no atomics: two calls give the same bits. */
int kws_filter_apply(const kws_filter_bank *bank, const kws_filter_params *params, const void *wav, int wav_dtype, const int32_t *index,
                     int B, int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const int32_t *explicit_filter,
                     float *out, int64_t out_stride, int32_t *lengths, int32_t *filter_used, void *stream);

/* ------------------------------------------------------------------------
 * Speed and loudness perturbation of raw audio: tools/audio_process/audio_convert.py of the reference (audio_resample / set_frame_rate
 * changes the rate of a file; --loudness sets its level with pydub's apply_gain(target - dBFS)), drawn afresh for every clip of every
 * train step on the device instead of written once as converted copies.  Clip b sits at global batch position p = position_base + b; its
 * source v is row index[b] of wav (int16 scaled by 1/32768), Ls = valid_len[row] or stride -- NOT clipped to max_samples: a clip played
 * faster reaches past the head the featurizer would otherwise keep.  Draws: h_f = aug_hash(seed, step, 4 p + f) (kws_augment.h; kws_amd
 * passes seed_s = WaveAugment seed ^ 0xA0761D6478BD642F, so the noise, reverb and filter draws are unchanged), u_f = (h_f >> 8) * 2^-24:
 *   f = 0: resampled = u_0 < speed_rate;  f = 1: r = fmaf(u_1, speed_hi - speed_lo, speed_lo)      (float32)
 *   f = 2: levelled  = u_2 < loud_rate;   f = 3: target = fmaf(u_3, loud_hi_db - loud_lo_db, loud_lo_db) dBFS
 *   resampled: the clip is played r times faster (tempo and pitch move together) by band-limited interpolation with the table h of a
 *         kws_resampler (Z zero crossings, P phases).  L' = min(ceil((double)Ls / (double)r), max_samples) (0 when Ls = 0).  For n < L':
 *         s = min(1, 1 / r); t = n r, n0 = floor(t), phi = t - n0 (float64; n r is exact);
 *         left wing,  k = 0, 1, ... while n0 - k >= 0 and pos = ((phi + k) s) P < Z P:  i = floor(pos), eta = pos - i,
 *                     acc += (h[i] + eta (h[i + 1] - h[i])) v[n0 - k];
 *         right wing, k = 0, 1, ... while n0 + 1 + k < Ls and pos = ((1 - phi + k) s) P < Z P: the same weight times v[n0 + 1 + k];
 *         y[n] = s acc.  t, pos, i and eta are float64 (a float32 phase is off by 1e-3 of a sample at n = 16000); the weight
 *         (fmaf(eta, h[i + 1] - h[i], h[i])), the products and the sum are float32, in this order: left wing, then right wing, k ascending.
 *   not resampled: L' = min(Ls, max_samples), y = v (bit for bit after the f32 conversion), speed_used = 0
 *   levelled: m = mean(y[0:L']^2) in float64 (fixed order; 0 when L' = 0), g = sqrtf((float)(10^(target / 10) / (m + FLT_EPSILON))),
 *         y *= g: pydub's apply_gain(target - dBFS) with full scale 1.0 (the 1/32768 scaling).  A silent clip stays silent.
 *   not levelled: gain_used = 1
 * This stage runs first; reverb, filter and noise (time shift included) then run unchanged on (out, lengths) with index = NULL and the
 * same position_base.  Divergences from the reference: a Kaiser-windowed sinc table instead of audioop.ratecv / sox; the number of
 * samples changes and the rate stays (a speed change), where the tool keeps the duration and changes the rate; only max_samples
 * outputs are made; no int16 quantisation and no clipping of the levelled result; fresh draws every step.
 * ---------------------------------------------------------------------- */
typedef struct kws_resampler kws_resampler;

/* The interpolation table, a HOST object (no device is needed to create or query it; the float32 device copy is made by the first
 * kws_speed_apply): the right half of a Kaiser-windowed sinc, h[i] = rolloff sinc(rolloff i / P) kaiser_beta(i / (P Z)), i = 0 .. Z P,
 * sinc(x) = sin(pi x) / (pi x), kaiser_beta(u) = I0(beta sqrt(1 - u^2)) / I0(beta), computed in float64 and rounded to float32.
 * zero_crossings Z in [4, 32], phases P in [32, 1024], beta in [0, 20], rolloff in (0, 1] (KWS_ERR_INVALID outside), and the table's
 * (Z P + 1) floats must fit 64 KiB of LDS (KWS_ERR_UNSUPPORTED above). */
int kws_resampler_create(int zero_crossings, int phases, double beta, double rolloff, kws_resampler **out);
void kws_resampler_destroy(kws_resampler *rs);
/* host: the arguments of kws_resampler_create (each may be NULL) */
int kws_resampler_info(const kws_resampler *rs, int *zero_crossings, int *phases, double *beta, double *rolloff);
/* host: the table as the device holds it, h[0 .. Z P] float32 (n >= Z P + 1) */
int kws_resampler_table(const kws_resampler *rs, float *out, size_t n);

typedef struct kws_speed_params {
    float speed_rate;      /* fraction of clips resampled, [0, 1]; 0 switches the speed half off */
    float speed_lo, speed_hi;     /* ratio r uniform in [lo, hi], 0.5 <= lo <= hi <= 2 (checked when speed_rate > 0) */
    float loud_rate;       /* fraction of clips levelled, [0, 1]; 0 switches the loudness half off */
    float loud_lo_db, loud_hi_db; /* target dBFS uniform in [lo, hi], -80 <= lo <= hi <= 0 (checked when loud_rate > 0) */
    int32_t max_samples;   /* the head the featurizer keeps, >= 1 */
    int32_t reserved;      /* 0 */
    uint64_t seed;         /* seed_s */
} kws_speed_params;

/* Perturb B clips, no atomics and no host synchronisation (the explicit arrays are copied from the host first).  out: B x out_stride
 * float32 (out_stride >= max_samples; never wav itself), row b = y[0:L'] then zeros; lengths (device int32 B, required) = L';
 * speed_used (device float32 B, may be NULL unless explicit_speed is given: the ratios are staged there) = r, or 0 for a clip that was
 * not resampled; gain_used (device float32 B, may be NULL unless explicit_db is given) = g, or 1 for a clip that was not levelled.
 * explicit_speed (HOST float32 B, or NULL): r from the caller, 0 = not resampled, other values in [0.5, 2].  explicit_db (HOST float32
 * B, or NULL): the target from the caller in [-80, 0], NaN = not levelled.  rs may be NULL when no clip can be resampled: speed_rate == 0 and
 * explicit_speed NULL or all zeros.  Fixed summation order: two calls give the same bits. */
int kws_speed_apply(const kws_resampler *rs, const kws_speed_params *params, const void *wav, int wav_dtype, const int32_t *index, int B,
                    int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const float *explicit_speed,
                    const float *explicit_db, float *out, int64_t out_stride, int32_t *lengths, float *speed_used, float *gain_used,
                    void *stream);

/* ------------------------------------------------------------------------
 * Tempo and pitch perturbation of raw audio by a phase vocoder: tempo without pitch, pitch without tempo, or both, where the speed
 * change above moves them together.  The reference has no counterpart; this comment is the definition (tests/pitch_ref.py restates it in
 * float64 numpy).  Clip b sits at global batch position p = position_base + b; its source v is row index[b] of wav (int16 scaled by
 * 1/32768), Ls = valid_len[row] or stride, NOT clipped to max_samples, as in the speed stage.
 * Draws: h_f = aug_hash(seed, step, 4 p + f) (kws_amd passes seed_p = WaveAugment seed ^ 0x8EBC6AF09C88C6E3, so the draws of every
 * other stage are unchanged), u_f = (h_f >> 8) * 2^-24:
 *   f = 0: stretched = u_0 < tempo_rate;  f = 1: tempo = fmaf(u_1, tempo_hi - tempo_lo, tempo_lo)      (float32, 0.5 .. 2)
 *   f = 2: pitched   = u_2 < pitch_rate;  f = 3: n = fmaf(u_3, pitch_hi - pitch_lo, pitch_lo) semitones (float32, -12 .. 12)
 *   r = (float)exp2((double)n / 12), 1 for a clip that is not pitched; rho = (double)tempo / (double)r, tempo 1 when not stretched.
 *   A clip neither stretched nor pitched: L' = min(Ls, max_samples), y = v (bit for bit after the f32 conversion), tempo_used = 0,
 *   pitch_used = NaN.  Every other clip:
 * Analysis.  N = n_fft in {256, 512, 1024}, H = N / 4, w[i] = 0.5 - 0.5 cos(2 pi i / N) (periodic Hann; float32, evaluated as
 *   sinpif(i / N)^2, which keeps its relative precision at the window's ends).  The source, N / 2 zeros in front of it and zeros behind
 *   it, is cut into the frames m = 0 .. M - 1, M = 1 + floor(Ls / H): x_m[i] = w[i] v[m H + i - N / 2].  D[m][k], k = 0 .. N / 2, is the
 *   real FFT of x_m in float32 (bins 0 and N / 2 have imaginary part +0); D[m] = 0 for m >= M.
 * Vocoder.  J = ceil(M / rho) output frames.  For frame j: t_j = j rho (float64, contraction off), m0 = floor(t_j), alpha = t_j - m0;
 *   mag = (1 - alpha) |D[m0]| + alpha |D[m0 + 1]|; ang(z) = atan2f(im, re), and 0 when re == 0 and im == 0 (signed zeros decide no
 *   phase); delta_j = ang(D[m0 + 1]) - ang(D[m0]) - (pi / 2) k, wrapped into [-pi, pi] by subtracting 2 pi rint(delta / 2 pi);
 *   Phi_j = ang(D[0]) + sum_{i < j} delta_i, accumulated in frame order (float32; only exp(i Phi) is used, and the device keeps Phi
 *   itself wrapped into [-pi, pi] so that its rounding does not grow with j; (pi / 2) k is taken off as (pi / 2)(k mod 4));
 *   Y_j[k] = mag i^((j k) mod 4) exp(i Phi_j).  With H = N / 4 the nominal advance 2 pi k H / N is a quarter turn per bin index: it is
 *   applied as an exact power of i and never enters the accumulator.
 * Synthesis.  y_j = the inverse real FFT of Y_j (the imaginary parts of bins 0 and N / 2 do not count) times w, overlap-added at hop H
 *   in frame order; every sample is divided by the sum of w^2 over the frames j < J that cover it where that sum is > 1e-8; the leading
 *   N / 2 samples are dropped; the stretched signal has Lst = floor(Ls / rho + 0.5) samples.
 * Pitch.  r != 1: the stretched signal is played r times faster by exactly kws_speed_apply's interpolation (the same table, the same
 *   order of operations), L' = min(ceil(Lst / r), max_samples); r == 1: L' = min(Lst, max_samples).  Only the frames and stretched
 *   samples that the L' outputs read are computed.
 * This stage runs first: speed and loudness, reverb, filter and noise then run unchanged on (out, lengths) with index = NULL and the
 * same position_base, so the loudness levels the final signal.  Divergences from the usual tools (librosa's phase_vocoder /
 * pitch_shift, sox): the plain vocoder, with no phase locking and no transient handling, so a stretched transient smears over a
 * window; bins below the rounding floor carry arbitrary phases (an exact zero: phase 0); the Kaiser-windowed sinc table instead of a
 * polyphase resampler; only max_samples outputs are made; fresh draws every step.
 * ---------------------------------------------------------------------- */
typedef struct kws_pitch_params {
    float tempo_rate;      /* fraction of clips stretched, [0, 1]; 0 switches the tempo half off */
    float tempo_lo, tempo_hi;     /* tempo uniform in [lo, hi], 0.5 <= lo <= hi <= 2 (checked when tempo_rate > 0) */
    float pitch_rate;      /* fraction of clips pitched, [0, 1]; 0 switches the pitch half off */
    float pitch_lo, pitch_hi;     /* semitones uniform in [lo, hi], -12 <= lo <= hi <= 12 (checked when pitch_rate > 0) */
    int32_t n_fft;         /* 256, 512 or 1024 */
    int32_t max_samples;   /* the head the featurizer keeps, 1 .. 2^20 */
    int32_t reserved;      /* 0 */
    uint64_t seed;         /* seed_p */
} kws_pitch_params;

/* host only (no device needed): the bytes with which kws_pitch_apply works on at least tile_clips clips at a time: per clip the spectrum
 * of the frames and the stretched samples that max_samples outputs can need at the ends of the ranges, rho = 4 and r = 2 (2.2 MB at n_fft
 * 512 and max_samples 16000; a 1 s clip at rho = 1 touches 260 KB of it).  kws_pitch_apply walks a batch in tiles of as many clips as
 * its workspace holds at the largest rho and r of that call (its ranges' ends, or its explicit values'), which is more than tile_clips
 * for narrower ranges. */
int kws_pitch_workspace_bytes(int n_fft, int max_samples, int tile_clips, size_t *bytes);

/* The analysis alone (a spectrogram): out (device, B x frames x (n_fft / 2 + 1) complex float32, re and im interleaved) = D[m][k] of the
 * B clips wav[index[b]] (index, valid_len as above), rows m >= M of a clip zeros.  frames >= 1; 1 + floor(stride / (n_fft / 4)) holds
 * every frame of every clip.  kws_pitch_apply's analysis is this one, bit for bit. */
int kws_pitch_stft(const void *wav, int wav_dtype, const int32_t *index, int B, int64_t stride, const int32_t *valid_len, int n_fft,
                   float *out, int frames, void *stream);

/* Perturb B clips, no atomics and no host synchronisation (the explicit arrays are copied from the host first).  out: B x out_stride
 * float32 (out_stride >= max_samples; never wav itself), row b = y[0:L'] then zeros; lengths (device int32 B, required) = L';
 * tempo_used (device float32 B, may be NULL unless explicit_tempo is given: the values are staged there) = tempo, or 0 for a clip that
 * was not stretched; pitch_used (device float32 B, may be NULL unless explicit_semitones is given) = n, or NaN for a clip that was not
 * pitched.  explicit_tempo (HOST float32 B, or NULL): tempo from the caller, 0 = not stretched, other values in [0.5, 2].
 * explicit_semitones (HOST float32 B, or NULL): n from the caller in [-12, 12], NaN = not pitched.  rs may be NULL when no clip can be
 * pitched, workspace when no clip can be stretched or pitched either.  workspace (device, workspace_bytes >= the bytes of one clip:
 * KWS_ERR_WORKSPACE below) is free again when the call's work on `stream` is done.  Fixed order of every sum: two calls give the same
 * bits, whatever the tile. */
int kws_pitch_apply(const kws_resampler *rs, const kws_pitch_params *params, const void *wav, int wav_dtype, const int32_t *index, int B,
                    int64_t stride, const int32_t *valid_len, int64_t position_base, int64_t step, const float *explicit_tempo,
                    const float *explicit_semitones, float *out, int64_t out_stride, int32_t *lengths, float *tempo_used,
                    float *pitch_used, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * SpecAugment of the FEATURES (time warp, time masks, frequency masks): the one augmentation stage behind the featurizer (or behind the
 * gather of cached features) and in front of the model.  The reference has no counterpart; this comment is the definition.  Clip b sits
 * at global batch position p = position_base + b; its features are x[T][F], T = n_features frames of F = feature_size coefficients.
 * Draws: h_f = aug_hash(seed, step, 32 p + f) (kws_wave_stage.h; 32 fields per clip; kws_amd passes seed_m = FeatureMask seed ^
 * 0xE7037ED1A0B428DB, so the draws of the wave stages are unchanged under the same user seed).  In this order:
 *   apply (f = 0):  the clip is transformed iff ((h_0 >> 8) * 2^-24) < rate; any other clip is bit-identical on output.
 *   time warp (max_warp = W > 0, needs T >= 2 W + 3): c = W + 1 + aug_uniform(h_1, T - 2 W - 2), d = (int)aug_uniform(h_2, 2 W + 1) - W,
 *         so frame c moves to c + d in [1, T - 2].  Source position of output frame t, in float32 with exactly these operations:
 *           t <= c + d:  s = (float)(t c) / (float)(c + d)
 *           otherwise:   s = (float)c + (float)((t - c - d) (T - 1 - c)) / (float)(T - 1 - c - d)
 *         k = min((int)s, T - 2), fr = s - k, y[t][f] = (1 - fr) x[k][f] + fr x[k + 1][f] (float32: one subtraction, two products,
 *         one sum; fr = 0 takes x[k] and fr = 1 takes x[k + 1] as they are).  Frames 0 and T - 1 map to themselves; d = 0 is the
 *         identity.  W = 0: y = x.
 *   fill value, per clip and per coefficient: KWS_FMASK_ZERO: 0; KWS_FMASK_MEAN: (sum over t ascending of y[t][f], float32) / (float)T
 *         -- an MFCC's 0th coefficient is a large log-energy offset, for which zero is an outlier value.
 *   time masks i < n_time:  w = aug_uniform(h_{3+2i}, max_time_width + 1), t0 = aug_uniform(h_{4+2i}, T - w + 1); the frames t0 <= t <
 *         t0 + w take the fill value in every coefficient.
 *   frequency masks j < n_freq:  w = aug_uniform(h_{11+2j}, max_freq_width + 1), f0 = aug_uniform(h_{12+2j}, F - w + 1); the
 *         coefficients f0 <= f < f0 + w take the fill value in every frame.
 * Masks may overlap; width 0 is a no-op.  Validation, evaluation, prediction and quantization never see this stage.
 * ---------------------------------------------------------------------- */
#define KWS_FMASK_MAX 4                /* time masks, and frequency masks, per clip */
#define KWS_FMASK_ZERO 0
#define KWS_FMASK_MEAN 1

typedef struct kws_feature_mask_params {
    float rate;              /* fraction of clips transformed, [0, 1] */
    int32_t n_time;          /* time masks per clip, 0..KWS_FMASK_MAX */
    int32_t max_time_width;  /* widths uniform in [0, max_time_width], 0..T */
    int32_t n_freq;          /* frequency masks per clip, 0..KWS_FMASK_MAX */
    int32_t max_freq_width;  /* widths uniform in [0, max_freq_width], 0..F */
    int32_t max_warp;        /* W: 0 = no time warp, otherwise T >= 2 W + 3 */
    int32_t fill;            /* KWS_FMASK_ZERO or KWS_FMASK_MEAN */
    int32_t reserved;        /* 0 */
    uint64_t seed;           /* seed_m */
} kws_feature_mask_params;

/* one clip's plan (84 bytes) */
typedef struct kws_fmask_clip {
    int32_t apply;           /* 1: transformed */
    int32_t warp_center;     /* c; 0 = not warped */
    int32_t warp_shift;      /* d */
    int32_t n_time, n_freq;
    int32_t t0[KWS_FMASK_MAX], tw[KWS_FMASK_MAX];   /* time masks: start, width */
    int32_t f0[KWS_FMASK_MAX], fw[KWS_FMASK_MAX];   /* frequency masks: start, width */
} kws_fmask_clip;

/* HOST only (no GPU needed): the plan the kernel draws for the clip at global position `position`, made by the same __host__ __device__
 * code.  Every field is drawn whether or not the clip is applied.  KWS_ERR_INVALID: rate outside [0, 1], a count outside
 * [0, KWS_FMASK_MAX], max_time_width outside [0, T], max_freq_width outside [0, F], T < 2 W + 3 with W > 0 (or W < 0), an unknown fill. */
int kws_feature_mask_draw(const kws_feature_mask_params *params, int T, int F, int64_t position, int64_t step, kws_fmask_clip *out);

/* Transform B clips feat (B x T x F float32, contiguous) into out (the same layout; out == feat is allowed: a clip that is not applied
 * then moves no bytes), one wave per clip, no atomics and no host synchronisation.  explicit_plan (HOST, B records, or NULL): the plans
 * from the caller instead of the draws (apply in {0, 1}; counts in [0, KWS_FMASK_MAX]; every mask inside [0, T] or [0, F], whatever the
 * params' maximum widths; warp_center = warp_shift = 0, or 1 <= c <= T - 2 and 1 <= c + d <= T - 2); they are copied into plan_out,
 * which is required then.  plan_out (device, B records, or NULL): the plans that were applied.  B == 0 is KWS_OK without a launch; the
 * parameter errors of kws_feature_mask_draw apply; T * F > kws_feature_mask_max_clip() is KWS_ERR_UNSUPPORTED and launches nothing.
 * Fixed summation order: two calls give the same bits. */
int kws_feature_mask(const kws_feature_mask_params *params, const float *feat, float *out, int B, int T, int F, int64_t position_base,
                     int64_t step, const kws_fmask_clip *explicit_plan, kws_fmask_clip *plan_out, void *stream);

/* the largest T * F kws_feature_mask takes: a clip and its F fill values stay in a wave's share of the LDS (5120; the default is 600) */
int64_t kws_feature_mask_max_clip(void);

/* ------------------------------------------------------------------------
 * Model: replaces the tf.keras objects built by classifier/model.py:14-46
 * get_model() (backbones classifier/models/cnn.py, rnn.py) and the work
 * Keras does inside model.fit / model.predict (train.py:75-92).
 *
 * Weights live in two caller-owned flat float32 device buffers:
 *   params : the trainable tensors           (kws_model_param_count floats)
 *   state  : BatchNormalization moving stats (kws_model_state_count floats)
 * kws_model_tensor_info() enumerates the tensors in Keras get_weights() order
 * with their offset into params (trainable) or state (not trainable); offsets
 * are multiples of 4 floats, gaps are zero.  grads / Adam moments mirror params.
 * ---------------------------------------------------------------------- */
typedef enum kws_model_kind {
    KWS_SIMPLE_CNN = 0,      /* classifier/models/cnn.py:11-74  */
    KWS_SIMPLE_CNN_LITE = 1, /* classifier/models/cnn.py:77-141 */
    KWS_SIMPLE_GRU = 2,      /* classifier/models/rnn.py:10-43  */
    KWS_SIMPLE_LSTM = 3      /* classifier/models/rnn.py:46-79  */
} kws_model_kind;

typedef struct kws_model kws_model;

typedef struct kws_tensor_info {
    char name[64];      /* e.g. "conv2d/kernel", "batch_normalization/gamma", "score_predict/bias" */
    int32_t ndim;
    int32_t shape[4];   /* Keras shapes: conv HWIO, dense (in, out) */
    int32_t trainable;  /* 1: offset is into params, 0: into state */
    int64_t offset;     /* in floats */
    int64_t size;       /* in floats */
} kws_tensor_info;

/* host only (no GPU needed).  kind outside the enum -> KWS_ERR_INVALID "Unsupported model type"
 * (classifier/model.py:32). n_features / feature_size: classifier/params.py:66-68,86-91. */
int kws_model_create(int kind, int num_classes, int n_features, int feature_size, kws_model **out);
/* simple_gru / simple_lstm with num_layers = 1 .. 4 recurrent layers of 48 units (the reference's `num_layers` argument, rnn.py): every
 * layer but the last returns its whole sequence (B, T, 48) to the next one, the last returns its final state to Dense(C).  Tensors in
 * Keras get_weights() order: gru_unit_<l>/kernel (F_l, 144), /recurrent_kernel (48, 144), /bias (2, 144) -- lstm_unit_<l>/...: (F_l, 192),
 * (48, 192), (192) -- for l = 0 .. num_layers - 1 with F_0 = feature_size and F_l = 48 above, then score_predict/kernel, /bias.
 * num_layers outside 1 .. 4, or != 1 for a CNN kind: KWS_ERR_INVALID.  kws_model_create is num_layers = 1.  A stacked model trains and
 * infers like any other; kws_quantize_simple_rnn / kws_qmodel_create_rnn refuse it with KWS_ERR_UNSUPPORTED (one layer only). */
int kws_model_create_stacked(int kind, int num_classes, int n_features, int feature_size, int num_layers, kws_model **out);
int kws_model_num_layers(const kws_model *m);
void kws_model_destroy(kws_model *m);
int64_t kws_model_param_count(const kws_model *m);
int64_t kws_model_state_count(const kws_model *m);
int kws_model_num_tensors(const kws_model *m);
int kws_model_tensor_info(const kws_model *m, int index, kws_tensor_info *out);
/* Creates the model's per-device resources (its side stream and fork / join events) on the CURRENT device now instead of at the first
 * train step.  HIP deals streams to a small number of hardware queues in creation order; when the side stream lands on the queue of
 * the caller's stream the step's fork / join overlap is lost (measured: 0.65 -> 1.2 ms per step when an RCCL communicator, which
 * creates streams of its own, was initialised before the model's first step).  Call it before kws_comm_init. */
int kws_model_bind_device(kws_model *m);
/* bytes of 256-byte aligned device scratch the calls below need for batch B */
int64_t kws_model_workspace_bytes(const kws_model *m, int B, int training);

/* model.predict (inference mode: BN moving statistics, no dropout).
 * feat (B, n_features, feature_size) -> probs (B, C) and/or argmax (B) (either may be NULL). */
int kws_model_forward(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws,
                      size_t ws_bytes, float *probs, int32_t *argmax, void *stream);

/* Inference with FIXED weights (serving, evaluation): kws_model_prepare_inference derives everything kws_model_forward computes
 * from the weights alone -- the folded BatchNormalization coefficients, the bf16 planes of the split-precision matrix operands,
 * the fp16 weight blob of simple_cnn_lite -- once, into `ws`; every later kws_model_forward with the SAME (B, params, state, ws)
 * and precisions then skips that work (17 of 300 us per call at B = 4096 for simple_cnn).  The caller promises not to change
 * `params` / `state` in between; kws_model_invalidate_prepared (or a train step, or a different forward in the same workspace)
 * drops the prepared state; it is keyed by the model's precisions, so a forward at another precision simply does not match it.  Recurrent models have nothing to prepare (returns KWS_OK). */
int kws_model_prepare_inference(kws_model *m, int B, const float *params, const float *state, void *ws, size_t ws_bytes, void *stream);
int kws_model_invalidate_prepared(kws_model *m);

/* One training forward + backward (what Keras does per batch inside model.fit, train.py:81):
 * batch-statistics BN (moving stats in `state` are updated), dropout from `dropout_seed` (0 = off),
 * loss = classifier/loss.py SparseCategoricalCrossEntropy (class_weights NULL) or
 * WeightedSparseCategoricalCrossEntropy (class_weights: C device floats), reduced by the batch mean.
 * grads <- grad_scale * d(mean loss)/d(params)  (data parallel: grad_scale = 1/world, then sum-all-reduce). */
/* seed of recurrent layer l's input-dropout mask: dropout_seed + l * 0x9E3779B97F4A7C15 modulo 2^64 (layer 0: dropout_seed itself) */
#define KWS_LAYER_DROPOUT_SEED(seed, l) ((uint64_t)(seed) + (uint64_t)(l) * 0x9E3779B97F4A7C15ull)
struct kws_comm;
typedef struct kws_train_args {
    const float *feat;          /* (B, n_features, feature_size)                                   */
    const int32_t *labels;      /* (B) class indices                                               */
    const float *class_weights; /* NULL or (C)                                                     */
    int32_t B;
    int32_t ignore_index;       /* <= 0: none (the reference tests truthiness, loss.py:25,59); else samples
                                   with this label contribute zero loss and zero gradient            */
    const float *params;
    float *state;
    float *grads;
    void *ws;
    size_t ws_bytes;
    uint64_t dropout_seed;      /* 0 = no dropout anywhere.  Recurrent layer l of a stacked model draws its (B, F_l) input mask with
                                   KWS_LAYER_DROPOUT_SEED(dropout_seed, l) at index b * F_l + f; layer 0's seed is dropout_seed   */
    float grad_scale;
    float *probs;               /* NULL or (B, C)                                                   */
    float *stats;               /* NULL or 2 floats: {sum of per-sample losses, number of top-1 hits} */
    void *bucket_event;         /* NULL or a hipEvent_t recorded (possibly on a library-internal stream) as soon as the
                                   gradients of the LAST kws_model_grad_split() .. param_count floats are final (they are
                                   produced first by the backward pass): a stream that waits on it may all-reduce that
                                   bucket while the rest of the backward pass runs */
    void *forward_event;        /* NULL or a hipEvent_t recorded on `stream` once the forward pass and the loss are
                                   enqueued: work that should share the chip with the backward pass (the next batch's
                                   featurization) can be ordered after it                                       */
    void *overlap_event;        /* NULL or a hipEvent_t recorded on `stream` at the best point of the step to start independent
                                   vector-ALU / memory work on another stream (the next batch's featurization).  simple_cnn: behind
                                   conv3's forward kernel (round 3's sweep of eleven points at B = 4096: 0.548 ms per step there,
                                   0.579 at forward_event; kws_model.hip; kws_model_set_overlap_point moves it);
                                   simple_cnn_lite and the recurrent models record it together with forward_event.          */
    void (*overlap_callback)(void *user);   /* NULL or a host function the call invokes (same thread, once) right after it has
                                   enqueued the work overlap_event marks: enqueueing the next batch's kws_featurize from it
                                   puts that launch at the same place in HOST order, so the overlap does not depend on how far
                                   the host runs ahead of the device (under a tracing profiler it does not run ahead at all) */
    void *overlap_user;
    struct kws_comm *comm;      /* NULL, or a communicator (kws_comm_init): the step then EXCHANGES its gradients itself -- sum over the
                                   ranks, in place: the early bucket grads[kws_model_grad_split(m), P) (conv4 + BN4 + dense + head, 82 % of
                                   the bytes, final first) on the model's side stream right behind conv4's weight gradient, i.e. under the
                                   rest of the backward pass; the late bucket together with `state * comm_state_weight` (BatchNormalization
                                   moving statistics: weight = local clips / global clips gives their batch-weighted mean over the replicas)
                                   on `stream` behind the backward pass.  When the call returns, kws_adam_step can be enqueued on `stream`.
                                   Set grad_scale = local clips / global clips.  bucket_event is not needed (and still honoured).        */
    float comm_state_weight;
    const double *feat_moments; /* NULL or the KWS_FEATURE_MOMENTS doubles kws_feature_moments() wrote for `feat` (same B): simple_cnn
                                   derives the batch statistics of its first BatchNormalization and the closed forms of its first
                                   layer's gradients from them instead of computing them at the head of the step, so an input
                                   pipeline can prepare them on its own stream right behind the featurizer.  Ignored by the
                                   other model kinds and at geometries kws_feature_moments() does not cover.             */
} kws_train_args;
int kws_model_train_fwd_bwd(kws_model *m, const kws_train_args *a, void *stream);

/* Second moments of a feature batch as seen by a 3x3 'same' convolution with one input channel (the first layer of
 * classifier/models/cnn.py:27): Q[t][t'] = sum over clips and pixels of a_t a_t', a_t = the feature at tap t of the pixel's
 * 3x3 patch (zero outside the map) for t < 9 and a_9 = 1; row-major 10 x 10 doubles (Q[t][9] = tap sums, Q[9][9] = B*H*W).
 * They depend on the features only, so they can be computed where the features are produced (kws_train_args.feat_moments).
 * ws: kws_feature_moments_workspace_bytes() bytes of 256-byte aligned device scratch.  Deterministic (fixed summation order).
 * KWS_ERR_UNSUPPORTED outside the geometries of the wave-per-clip kernels (H, W even, (H+2)(W+2) <= 768, H*W/4 <= 160): pass
 * feat_moments = NULL there. */
#define KWS_FEATURE_MOMENTS 100
int64_t kws_feature_moments_workspace_bytes(int B);
int kws_feature_moments(const float *feat, int B, int n_features, int feature_size, double *moments, void *ws, size_t ws_bytes,
                        void *stream);
/* Arithmetic of the GEMM-shaped layers with 32 or more reduced channels (simple_cnn: conv3, conv4, dense).
 *   KWS_MATRIX_BF16X6 (default): every fp32 operand is carried as h + m + l in bf16 (24 bits) and a product is the six
 *                      leading partial products on the bf16 matrix cores with fp32 accumulation: fp32-level error at
 *                      ~2.7x the fp32 matrix rate
 *   KWS_MATRIX_FP32:   the fp32 MFMA everywhere (bit-identical to an fp32 fmaf chain)
 * kws_set_matrix_precision sets the library-wide DEFAULT, which a model follows until kws_model_set_precision gives it its own
 * value; read at the next forward / train call. */
enum { KWS_MATRIX_FP32 = 0, KWS_MATRIX_BF16X6 = 1 };
int kws_set_matrix_precision(int mode);
int kws_get_matrix_precision(void);
/* Precision of simple_cnn_lite INFERENCE (kws_model_forward; BASELINE configs[4] asks fp16).  Library-wide default, per model
 * through kws_model_set_precision.
 *   KWS_INFER_FP32 (default): fp32 activations and products.
 *   KWS_INFER_FP16: the activations between stages and every matrix operand are fp16, all accumulation (depthwise taps,
 *                   matrix products, bias / BatchNorm affine, softmax) fp32; the network behind the second pooling stage
 *                   runs as ONE kernel with its fp16 weights in LDS.  Needs the default geometry family (pooled maps up to
 *                   7 x 5 / 4 x 3) and at most 48 classes, otherwise kws_model_forward returns KWS_ERR_UNSUPPORTED.
 * Other model kinds ignore the switch (classifier/models/cnn.py:77-141 is the topology it applies to). */
enum { KWS_INFER_FP32 = 0, KWS_INFER_FP16 = 1 };
int kws_set_inference_precision(int mode);
int kws_get_inference_precision(void);
/* Per-model precision attributes: `matrix` in {KWS_MATRIX_FP32, KWS_MATRIX_BF16X6}, `infer` in {KWS_INFER_FP32, KWS_INFER_FP16},
 * or -1 = follow the library-wide default above.  Two models with different precisions may live in one process (one host
 * thread per model; a model's calls are not re-entrant).  kws_model_get_precision reports the EFFECTIVE values. */
int kws_model_set_precision(kws_model *m, int matrix, int infer);
int kws_model_get_precision(const kws_model *m, int *matrix, int *infer);
/* Test aid: with on != 0 every weight-gradient reduction of simple_cnn / simple_cnn_lite runs in a fixed order (one block
 * along the reduced axis, a batch-ordered head kernel) instead of per-block float atomics, so two runs of a step give
 * bit-identical gradients.  Much slower at large batches; recurrent models: KWS_ERR_UNSUPPORTED. */
int kws_model_set_deterministic(kws_model *m, int on);

/* Tuning aid: where in the simple_cnn train step kws_train_args.overlap_event is recorded / overlap_callback is called.  -1 (default):
 * the library's choice (10 = behind conv3's forward); 6 behind the last forward convolution's BatchNormalization statistics (its activation now rides in the Dense + head kernel), 0 behind the last forward convolution, 1 behind
 * the loss, 2 behind the head's backward kernel, 3 behind the dense data gradient, 4 behind BatchNorm-4's backward, 5 behind conv4's
 * data gradient, 7 behind the dense forward product, 8 behind layer 1's forward kernel, 9 behind conv2's forward, 10 behind conv3's.
 * Changes scheduling only, never results (tests/test_model_gpu.py). */
int kws_model_set_overlap_point(kws_model *m, int point);

/* offset (in floats) that splits `grads` into {late bucket [0, split), early bucket [split, param_count)} */
int64_t kws_model_grad_split(const kws_model *m);

/* ------------------------------------------------------------------------
 * int8 post-training quantization of simple_cnn: what a user of the reference does with the MNN quantizer
 * (inference/MNN/configs/quantizeConfig.json, weight_quantize_method MAX_ABS) or tools/model_converter/custom_tflite_convert.py
 * (--post_training_quantize) before shipping the model, and then measures with eval.py.  A quantized model is a frozen snapshot: it
 * does not follow later changes of the float weights.  Scope: KWS_SIMPLE_CNN at the default geometry (30 x 20 features; pooled maps
 * 15 x 10 -> 7 x 5 -> 4 x 3 -> 2 x 1) and C <= KWS_QUANT_MAX_CLASSES; everything else is KWS_ERR_UNSUPPORTED.
 *
 * Contract.  Symmetric, zero-point 0 everywhere: "same" padding pads with code 0 and every accumulator is an exact int32.
 *   Quantized tensors t0 = the features x, t1 = a1 (after pool 1), t2 = a2 (after pool 2), t3 = a3 (conv3 -> BN -> ReLU6),
 *   t4 = a4 (after pool 4), t5 = d (Dense -> ReLU6).
 *   Activation scales s_t = A_t / 127 in double.  A_0 = calibrated max|x|; for t >= 1 A_t = min(calibrated max, 6), a calibrated 0
 *   (dead layer) becoming 6; KWS_QUANT_RELU6 uses A_t = 6 for t >= 1.  A non-finite or negative A_t, or A_0 == 0, is KWS_ERR_INVALID.
 *   Weights, per output channel c, MAX_ABS in double: r_c = max|W[..., c]|, s_wc = r_c / 127 (1 when r_c == 0),
 *   q = clamp(rint(W / s_wc), -127, 127), rint rounding half to even; all four conv kernels (HWIO), Dense (256, 128), head (128, C).
 *   BatchNorm fold in double: g = gamma / sqrt(moving_var + eps), h = beta - moving_mean * g, eps = the library's float 1e-3 widened.
 *   Per-channel constants, each computed in double in the order written and rounded ONCE to fp32:
 *     conv l = 1..4: M[c] = ((s_in * s_wc) * g_c) / s_out,  Bq[c] = h_c / s_out
 *     Dense:         M[c] = (s_4 * s_wc) / s_5,             Bq[c] = bias_c / s_5
 *     head:          Mh[c] = s_5 * s_wc;   input: inv_s0 = 1 / s_0
 *   Device arithmetic (fp32, every multiply and add rounded separately -- no contraction -- and rint half to even):
 *     input:           code = clamp(rint(x * inv_s0), -127, 127)
 *     conv1-3, Dense:  code = clamp(rint((float)acc * M[c] + Bq[c]), 0, 127)          (the clamp is ReLU6)
 *     conv4:           acc = max(acc, 0) first (Conv2D(activation='relu') -> BN -> ReLU6), then as conv1-3
 *     max pooling (2 x 2, stride 2, valid) on the codes AFTER the epilogue (a negative gamma makes the epilogue decreasing)
 *     head:            logit = (float)acc * Mh[c] + bias[c], then the fp32 softmax of the float head (first maximum wins the arg-max)
 *   |acc| < 2^24 everywhere (conv4: 576 * 127^2 ~ 9.3 M), so (float)acc is exact.
 *   KWS_QUANT_KL (section "entropy calibration" below) applies the rules of KWS_QUANT_MAX to KL ranges passed in place of the maxima.
 * Divergences from MNN / TFLite: symmetric int8 instead of TFLite's asymmetric uint8; per-channel weight scales; the entropy (KL)
 * calibration is modelled on MNN's "KL" feature_quantize_method (TensorRT's 8-bit recipe), its details fixed by the contract below
 * rather than by MNN's source; fp32 epilogue multipliers instead of fixed-point ones; fp32 softmax.
 * ---------------------------------------------------------------------- */
#define KWS_QUANT_TENSORS 6
#define KWS_QUANT_MAX_CLASSES 48
enum { KWS_QUANT_MAX = 0, KWS_QUANT_RELU6 = 1, KWS_QUANT_KL = 2 };

/* Calibration: runs the fp32 inference forward (BN moving statistics, no dropout) of B clips and max-reduces into amax (6 DEVICE floats):
 * amax[0] = max |x|, amax[1..5] = max of t1..t5 (all >= 0).  The caller zeroes amax once; every call folds its batch into the running
 * maxima, so calls over the halves of a set give the call over the whole set.  One block per clip, exact fp32; does not use or touch
 * the tuned forward's kernels.  ws may be NULL (no scratch needed); B = 0 is a no-op. */
int kws_model_calibrate(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                        float *amax, void *stream);

/* The quantized network on the HOST (every array in Keras order, filled by kws_quantize_simple_cnn) */
typedef struct kws_qsimple_cnn {
    int32_t num_classes;                /* C, 2..KWS_QUANT_MAX_CLASSES */
    int32_t method;                     /* KWS_QUANT_MAX / KWS_QUANT_RELU6 / KWS_QUANT_KL */
    float inv_s0;                       /* 1 / s_0 */
    int32_t reserved;
    double amax[KWS_QUANT_TENSORS];     /* A_0..A_5 after the rules above */
    double scale[KWS_QUANT_TENSORS];    /* s_0..s_5 (reporting) */
    int8_t conv_w1[3 * 3 * 1 * 16];     /* HWIO */
    int8_t conv_w2[3 * 3 * 16 * 32];
    int8_t conv_w3[3 * 3 * 32 * 64];
    int8_t conv_w4[3 * 3 * 64 * 128];
    int8_t dense_w[256 * 128];          /* (in, out) */
    int8_t head_w[128 * KWS_QUANT_MAX_CLASSES];   /* (128, C): the first 128 C entries, row stride C */
    float M1[16], B1[16], M2[32], B2[32], M3[64], B3[64], M4[128], B4[128];
    float Md[128], Bd[128];
    float Mh[KWS_QUANT_MAX_CLASSES], head_bias[KWS_QUANT_MAX_CLASSES];
} kws_qsimple_cnn;

/* Host only (no GPU): params_host / state_host are the model's flat buffers (kws_model_param_count / state_count floats, the layout of
 * kws_model_tensor_info), amax_host the 6 calibrated maxima.  Fills *out by the contract above. */
int kws_quantize_simple_cnn(const kws_model *m, const float *params_host, const float *state_host, const float *amax_host, int method,
                            kws_qsimple_cnn *out);

/* A quantized model on the CURRENT device: uploads q's arrays and packs the weights into the fragment-major layout the kernel reads.
 * The only way to build one (a saved quantized checkpoint is loaded through it too).  m gives the model kind and geometry. */
typedef struct kws_qmodel kws_qmodel;
int kws_qmodel_create(const kws_model *m, const kws_qsimple_cnn *q, kws_qmodel **out);
void kws_qmodel_destroy(kws_qmodel *q);
/* bytes of device scratch kws_qmodel_forward needs for batch B (the single-kernel forward needs none: 0) */
int64_t kws_qmodel_workspace_bytes(const kws_qmodel *q, int B);
/* feat (B, 30, 20) float32 -> logits (B, C) float32, probs (B, C) float32, argmax (B) int32; each may be NULL.  B = 0 is a no-op, B
 * need not be a multiple of anything.  One kernel on `stream`, no host synchronisation: capturable into a hipGraph. */
int kws_qmodel_forward(const kws_qmodel *q, const float *feat, int B, void *ws, size_t ws_bytes, float *logits, float *probs,
                       int32_t *argmax, void *stream);

/* ------------------------------------------------------------------------
 * int8 post-training quantization of simple_cnn_lite (classifier/models/cnn.py:77-141, four SeparableConv2D stages): the on-device
 * model, the one a user of the reference ships through the same MNN / TFLite quantizers.  Scope: KWS_SIMPLE_CNN_LITE at the default
 * geometry (30 x 20; pooled maps 15 x 10 -> 7 x 5 -> 4 x 3 -> 2 x 1) and C <= KWS_QUANT_MAX_CLASSES; everything else is
 * KWS_ERR_UNSUPPORTED.  The rules of the simple_cnn section above hold unless stated otherwise (symmetric, zero-point 0, "same"
 * padding = code 0, exact int32 accumulators with |acc| < 2^24, rint half to even, constants in double rounded once to fp32, no
 * contraction on the device).
 *
 * Contract.
 *   Quantized tensors, in the order of amax[0..9]: t0 = x, t1 = u1, t2 = a1 (after pool 1), t3 = u2, t4 = a2 (after pool 2), t5 = u3,
 *   t6 = a3, t7 = u4, t8 = a4 (after pool 4), t9 = d (Dense -> ReLU6).  u_l is the depthwise output of stage l: signed and quantized
 *   as a tensor of its own, as TFLite does when it splits a SeparableConv2D into DEPTHWISE_CONV_2D + CONV_2D.
 *   Ranges A_t, scales s_t = A_t / 127: x: A = calibrated max|x| (0 is KWS_ERR_INVALID); u_l: A = calibrated max|u_l|, no cap, a
 *   calibrated 0 becoming 1 (the tensor is identically zero); a1..a4, d: A = min(calibrated max, 6), a calibrated 0 becoming 6.
 *   KWS_QUANT_RELU6 uses 6 for a1..a4 and d and the calibrated values for x and u_l.  Non-finite or negative: KWS_ERR_INVALID.
 *   Weights, per-channel MAX_ABS as for simple_cnn: depthwise kernels (3, 3, C, 1) per channel c over its 9 taps; pointwise kernels
 *   (1, 1, CI, CO) per output channel; Dense and head as for simple_cnn.
 *   Stage l (s_in = s_{2l-2}, s_u = s_{2l-1}, s_out = s_{2l}; s_dwc, s_pwc the weight scales; g, h the BatchNorm fold of simple_cnn):
 *     Mu[c] = (s_in * s_dwc) / s_u
 *     bq[c] = rint(bias_c / (s_u * s_pwc)) clamped to +-2^23 (int32)
 *     M[c]  = ((s_u * s_pwc) * g_c) / s_out,   Bq[c] = h_c / s_out
 *   Dense: Md[c] = (s_8 * s_wc) / s_9, Bd[c] = bias_c / s_9;  head: Mh[c] = s_9 * s_wc;  input: inv_s0 = 1 / s_0.
 *   Device arithmetic:
 *     input:      code = clamp(rint(x * inv_s0), -127, 127)
 *     depthwise:  dacc = sum over the 9 taps of code_in * qdw[tap][c];  u = clamp(rint((float)dacc * Mu[c]), -127, 127)
 *                 (stage 3: stride 2, padding 1 before and 1 after on both axes, as simple_cnn's conv3)
 *     pointwise:  acc = sum over ci of u[ci] * qpw[ci][c] + bq[c]  (|acc| <= 64 * 127^2 + 2^23 < 2^24);  stages 3 and 4 then
 *                 acc = max(acc, 0) (their activation='relu');  code = clamp(rint((float)acc * M[c] + Bq[c]), 0, 127)
 *     max pooling on the codes after the epilogue (stages 1, 2, 4); Dense, head, softmax, arg-max as in the simple_cnn contract.
 *   KWS_QUANT_KL applies the rules of KWS_QUANT_MAX to KL ranges passed in place of the maxima (section "entropy calibration" below).
 * Divergences from MNN / TFLite: symmetric int8; per-channel depthwise and pointwise scales; the entropy (KL) calibration modelled on
 * MNN's "KL" method (TensorRT's 8-bit recipe) by the contract below, not by MNN's source; fp32 epilogue multipliers; the pointwise
 * bias clamped to +-2^23 (TFLite keeps the full int32 bias).
 * ---------------------------------------------------------------------- */
#define KWS_QLITE_TENSORS 10

/* Calibration of simple_cnn_lite: as kws_model_calibrate, into 10 DEVICE floats amax[0..9] = max|x|, max|u1|, max a1, max|u2|, max a2,
 * max|u3|, max a3, max|u4|, max a4, max d (the u_l over the whole depthwise map).  Exact fp32 forward, one block per clip, in a
 * kernel of its own (not the tuned lite kernels).  Other model kinds: KWS_ERR_UNSUPPORTED. */
int kws_model_calibrate_lite(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                             float *amax, void *stream);

/* The quantized simple_cnn_lite on the HOST (Keras order, filled by kws_quantize_simple_cnn_lite) */
typedef struct kws_qsimple_cnn_lite {
    int32_t num_classes;                /* C, 2..KWS_QUANT_MAX_CLASSES */
    int32_t method;                     /* KWS_QUANT_MAX / KWS_QUANT_RELU6 / KWS_QUANT_KL */
    float inv_s0;                       /* 1 / s_0 */
    int32_t reserved;
    double amax[KWS_QLITE_TENSORS];     /* A_0..A_9 after the rules above */
    double scale[KWS_QLITE_TENSORS];    /* s_0..s_9 (reporting) */
    int8_t dw_w1[3 * 3 * 1], dw_w2[3 * 3 * 16], dw_w3[3 * 3 * 32], dw_w4[3 * 3 * 64];     /* (3, 3, C, 1) */
    int8_t pw_w1[1 * 16], pw_w2[16 * 32], pw_w3[32 * 64], pw_w4[64 * 128];              /* (1, 1, CI, CO) */
    int8_t dense_w[256 * 128];          /* (in, out) */
    int8_t head_w[128 * KWS_QUANT_MAX_CLASSES];   /* (128, C): the first 128 C entries, row stride C */
    int32_t bq1[16], bq2[32], bq3[64], bq4[128];
    float Mu1[1], Mu2[16], Mu3[32], Mu4[64];
    float M1[16], B1[16], M2[32], B2[32], M3[64], B3[64], M4[128], B4[128];
    float Md[128], Bd[128];
    float Mh[KWS_QUANT_MAX_CLASSES], head_bias[KWS_QUANT_MAX_CLASSES];
} kws_qsimple_cnn_lite;

/* Host only: as kws_quantize_simple_cnn, with the 10 calibrated maxima of kws_model_calibrate_lite */
int kws_quantize_simple_cnn_lite(const kws_model *m, const float *params_host, const float *state_host, const float *amax_host, int method,
                                 kws_qsimple_cnn_lite *out);
/* A quantized simple_cnn_lite on the CURRENT device.  kws_qmodel_forward (ONE kernel, features to probabilities, capturable),
 * kws_qmodel_workspace_bytes (0) and kws_qmodel_destroy serve it as they serve a quantized simple_cnn. */
int kws_qmodel_create_lite(const kws_model *m, const kws_qsimple_cnn_lite *q, kws_qmodel **out);

/* ------------------------------------------------------------------------
 * int8 dynamic-range ("hybrid") quantization of simple_gru and simple_lstm: what the reference's
 * tools/model_converter/custom_tflite_convert.py --post_training_quantize gives a recurrent model (Optimize.DEFAULT, no
 * representative dataset, FLOAT inference type): int8 weights, the inputs of every matrix product quantized on the fly per row,
 * int32 accumulation rescaled to fp32, gates, biases and the softmax in fp32.  No calibration.  A frozen snapshot of the weights.
 * Scope: KWS_SIMPLE_GRU and KWS_SIMPLE_LSTM (48 units, one layer), feature_size F in 1..64 (the input product is one k-step),
 * T = n_features in 1..KWS_QRNN_MAX_STEPS, 2 <= C <= KWS_QUANT_MAX_CLASSES; everything else is KWS_ERR_UNSUPPORTED.  A non-finite
 * weight or bias is KWS_ERR_INVALID.  G = 3 gates (GRU: z, r, h) or 4 (LSTM: i, f, c, o), N = 48 G gate columns.
 *
 * Contract.
 *   Weights: kernel (F, N), recurrent_kernel (48, N) and the head kernel (48, C), each per output column j, symmetric MAX_ABS in
 *   double: a_j = max_k |w_kj|, s_j = a_j / 127, q = clamp(rint(w / s_j), -127, 127) (rint half to even), stored with s_j rounded
 *   once to fp32; an all-zero column has codes 0 and s_j = 0.  Biases stay fp32: the GRU's (2, N) = b0 | b1, the LSTM's (N), the head's.
 *   Dynamic rows: for every clip, each step's input x_t (F values), each step's recurrent input h_{t-1} (48 values, h_0 = 0) and the
 *   final h_T are quantized as a row of their own: m = max|v|; m == 0: codes 0 and s = 0; otherwise, in fp32 with IEEE division,
 *   inv = 127.f / m, code = clamp(rint(v * inv), -127, 127) (ties to even), s = m / 127.f.
 *   Accumulators are exact int32 (|acc| <= 64 * 127^2 < 2^24, so (float)acc is exact).  Device arithmetic is fp32 with every
 *   multiply and add rounded separately (no contraction), left to right as written:
 *     X_j = ((float)acc_x * s_x) * sW_j,   H_j = ((float)acc_h * s_h) * sU_j
 *     GRU (reset_after=True):  mx = X + b0,  mh = H + b1;  z = sg(mx_z + mh_z),  r = sg(mx_r + mh_r),  hh = mx_h + r * mh_h,
 *                              h' = z * h + (1 - z) * hh                              (activation='linear': no tanh on hh)
 *     LSTM:                    a = (X + H) + b;  i = sg(a_i), f = sg(a_f), g = th(a_c), o = sg(a_o);  c' = f * c + i * g,
 *                              h' = o * th(c')
 *     head:                    logit_c = ((float)acc * s_hT) * s_c + bias_c, then the fp32 softmax and arg-max of the other int8 heads
 *                              (first maximum wins)
 *   h and c are fp32 registers.  sg and th are the fp32 kernels' sigmoidf_ / tanh_fast_ (csrc/kws_gru.h: hardware exp2 and reciprocal,
 *   each within a few ulp, absolute error below 1e-6): NOT bit-reproducible off the device.  A restatement that evaluates them in
 *   float64 agrees with the device to that error per gate, and exactly where they saturate to 0 or 1; a requantized code may then
 *   differ by one where v * inv lies within that error of a rounding tie.
 * Divergences from TFLite: per-column weight scales; symmetric rows (TFLite's hybrid ops may quantize inputs asymmetrically); the fp32
 * gate functions above.
 * ---------------------------------------------------------------------- */
#define KWS_QRNN_MAX_STEPS 128
#define KWS_QRNN_MAX_FEATURES 64
#define KWS_QRNN_UNITS 48
enum { KWS_QUANT_DYNAMIC = 3 };

/* The quantized simple_gru / simple_lstm on the HOST (Keras order, row-major, filled by kws_quantize_simple_rnn) */
typedef struct kws_qsimple_rnn {
    int32_t kind;                       /* KWS_SIMPLE_GRU / KWS_SIMPLE_LSTM */
    int32_t num_classes;                /* C, 2..KWS_QUANT_MAX_CLASSES */
    int32_t n_steps, feature_size;      /* T, F */
    int32_t method;                     /* KWS_QUANT_DYNAMIC */
    int32_t reserved;
    int8_t kernel[KWS_QRNN_MAX_FEATURES * 4 * KWS_QRNN_UNITS];    /* (F, N): the first F N entries, row stride N */
    int8_t recurrent_kernel[KWS_QRNN_UNITS * 4 * KWS_QRNN_UNITS]; /* (48, N): the first 48 N entries */
    int8_t head_w[KWS_QRNN_UNITS * KWS_QUANT_MAX_CLASSES];       /* (48, C): the first 48 C entries, row stride C */
    float kernel_scale[4 * KWS_QRNN_UNITS];                      /* sW_j, the first N */
    float recurrent_scale[4 * KWS_QRNN_UNITS];                   /* sU_j, the first N */
    float bias[2 * 4 * KWS_QRNN_UNITS];                          /* GRU: (2, N) = b0 | b1 (first 2N); LSTM: (N) (first N) */
    float head_scale[KWS_QUANT_MAX_CLASSES], head_bias[KWS_QUANT_MAX_CLASSES];
} kws_qsimple_rnn;

/* Host only: params_host = the model's flat parameter buffer (kws_model_param_count floats, the layout of kws_model_tensor_info).
 * Fills *q by the contract above (method = KWS_QUANT_DYNAMIC). */
int kws_quantize_simple_rnn(const kws_model *m, const float *params_host, kws_qsimple_rnn *q);
/* A quantized simple_gru / simple_lstm on the CURRENT device.  kws_qmodel_forward (ONE kernel from features (B, T, F) to logits,
 * probabilities and arg-max, capturable), kws_qmodel_workspace_bytes (0) and kws_qmodel_destroy serve it as the CNN kinds. */
int kws_qmodel_create_rnn(const kws_model *m, const kws_qsimple_rnn *q, kws_qmodel **out);

/* ------------------------------------------------------------------------
 * Entropy (KL) calibration of the int8 models: what the reference's deployment recipe asks for
 * (inference/MNN/configs/quantizeConfig.json, "feature_quantize_method": "KL").  Modelled on MNN's KL method, itself TensorRT's 8-bit
 * entropy calibration; MNN's source being outside this project, the details below are this contract's own: zeros are not counted,
 * the 128 groups split [0, i) with integer arithmetic, the candidates run up to i = 2048 inclusive and the range is i* amax / 2048.
 *
 *   1. A max pass (kws_model_calibrate / kws_model_calibrate_lite) gives the T maxima amax_t (T = 6 / 10, their order).
 *   2. A histogram pass (kws_model_calibrate_hist) over the same set, with amax copied to the host: for every tensor t with
 *      amax_t > 0, k_t = (float)(2048.0 / (double)amax_t) on the host, and for every element v the max pass reduces for t (the same
 *      fp32 values: both passes run one per-clip forward), v != 0: bin = min((int)(|v| * k_t), 2047) (one fp32 multiply, no
 *      contraction), hist[t][bin] += 1.  Zeros are not counted (after a ReLU6 they would swamp bin 0); amax_t == 0 gives no counts.
 *   3. kws_quant_kl_ranges (host) turns the counts into ranges A_t; kws_quantize_simple_cnn[_lite](..., A, KWS_QUANT_KL, ...) applies
 *      the rules of KWS_QUANT_MAX to them (post-ReLU6 ranges capped at 6; a range of 0 becoming 6, or 1 for u_l; A_0 = 0 invalid)
 *      and records method = KWS_QUANT_KL.
 *   KL search, per tensor, h its 2048 counts, N = sum h, all in double with sums in ascending index order: for i = 128 .. 2048,
 *     P[j] = h[j] for j < i, then P[i-1] += sum_{j >= i} h[j];
 *     groups g = 0..127 of [0, i): [floor(g i / 128), floor((g + 1) i / 128)), S_g = sum of h, n_g = number of nonzero h over the group;
 *     Q[j] = S_g / n_g where h[j] != 0, else 0;  p = P / sum P, q = Q / sum Q;  KL_i = sum_{p_j > 0} p_j ln(p_j / q_j),
 *     +inf if sum Q = 0 or some p_j > 0 has q_j = 0 (i = 2048 clips nothing: some KL_i is finite).
 *   i* = the SMALLEST i of least KL_i; A_t = i* amax_t / 2048 in double, rounded once to float.  N = 0 gives A_t = 0.
 * ---------------------------------------------------------------------- */
#define KWS_QUANT_HIST_BINS 2048

/* Histogram pass: dispatches on the model kind (simple_cnn: T = 6, simple_cnn_lite: T = 10; other kinds KWS_ERR_UNSUPPORTED).
 * amax_host: the T maxima of a finished max pass (HOST floats, copied into the kernel arguments: the call is capturable).  hist: a
 * DEVICE T x KWS_QUANT_HIST_BINS uint64 array of running counts; the caller zeroes it once and every call adds its batch (calls over
 * the halves of a set give the call over the whole set, exactly).  A persistent kernel: each block counts in LDS and adds its nonzero
 * bins once at its end.  ws may be NULL; B = 0 is a no-op. */
int kws_model_calibrate_hist(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                             const float *amax_host, uint64_t *hist, void *stream);
/* Host only: the KL search above over T histograms (hist_host T x KWS_QUANT_HIST_BINS, amax_host T floats) -> ranges_out[T] and, when
 * bins_out is not NULL, i* per tensor (0 for an empty histogram). */
int kws_quant_kl_ranges(const uint64_t *hist_host, const float *amax_host, int T, float *ranges_out, int32_t *bins_out);

/* ------------------------------------------------------------------------
 * Data-parallel exchange (RCCL over xGMI).  New: the reference trains in one
 * process (train.py:81-92, model.fit(..., workers=1) at :90-91); this is the
 * collective SURVEY.md section 5 / 8(e) specify around that loop.  One process
 * per GPU, one communicator per process, created on the CURRENT device.
 * RCCL is bound at run time (dlopen of librccl.so.1, sharing the instance the
 * process already holds if any), so single-GPU hosts never load it.
 *
 *   rank 0:  kws_comm_unique_id(id);  ship the 128 bytes to every rank (file, socket, MPI, torch.distributed ...)
 *   all:     kws_comm_init(rank, world, id, &comm)            -- collective
 *   step:    args.comm = comm; args.grad_scale = args.comm_state_weight = local clips / global clips;
 *            kws_model_train_fwd_bwd(m, &args, stream);       -- gradients arrive summed over the ranks
 *            kws_adam_step(...)
 * The communicator owns no stream: every collective is enqueued on a stream the step already uses (a collective on a stream of its
 * own stalled the device by ~1.1 ms per step on MI355X / ROCm 7.2: 0.65 -> 1.79 ms, tools/commbench.py).
 * ---------------------------------------------------------------------- */
typedef struct kws_comm kws_comm;
#define KWS_COMM_ID_BYTES 128
int kws_comm_unique_id(void *id /* KWS_COMM_ID_BYTES host bytes */);
int kws_comm_init(int rank, int world, const void *unique_id, kws_comm **out);
void kws_comm_destroy(kws_comm *c);
/* rccl_version: NCCL-style code of the bound library (e.g. 22707), 0 if unknown; any out pointer may be NULL */
int kws_comm_info(const kws_comm *c, int *rank, int *world, int *rccl_version);

/* The exchange as a call of its own, for steps that did not run kws_model_train_fwd_bwd with args.comm (a rank whose shard of a
 * partial last batch is empty: cleared gradients, weight 0; or a caller with its own backward pass): in-place sum over the ranks of
 * grads[split, n), then -- one RCCL group -- of grads[0, split) and of state[0, n_state) * state_weight, all on `stream`, i.e.
 * the same collectives in the same order as the train step issues, so ranks may mix the two forms.  split in {0, n}: one bucket. */
int kws_allreduce_grads(kws_comm *c, float *grads, int64_t n, int64_t split, float *state, int64_t n_state, float state_weight,
                        void *stream);

/* A plain in-place all-reduce on `stream` (loss / hit counters of a logging step, timing maxima). */
enum { KWS_DT_F32 = 0, KWS_DT_F64 = 1, KWS_DT_I32 = 2, KWS_DT_I64 = 3 };
enum { KWS_OP_SUM = 0, KWS_OP_MAX = 1, KWS_OP_AVG = 2 };
int kws_comm_allreduce(kws_comm *c, void *buf, int64_t n, int dtype, int op, void *stream);
/* In-place broadcast of nbytes device bytes from rank `root` on `stream`: what a data-parallel fit needs once per run (the initial
 * weights / moving statistics, where the reference has a single model object, classifier/model.py:14-46) and once per epoch (the
 * shuffle permutation of train.py:90, shuffle=True), so that no second communicator -- with streams of its own -- is ever built. */
int kws_comm_broadcast(kws_comm *c, void *buf, int64_t nbytes, int root, void *stream);

/* Opt-in timing of the two buckets of the most recent exchange (HIP events around each RCCL launch on the stream it was enqueued
 * on); kws_comm_last_us synchronises those events; -1 = that bucket was not issued / timing off. */
int kws_comm_timing(kws_comm *c, int on);
int kws_comm_last_us(kws_comm *c, float *early_us, float *late_us);

/* Standalone losses of classifier/loss.py: y_pred (B, C) probabilities (or logits when from_logits != 0),
 * labels (B) -> per-sample losses (B), exactly what the two classes' __call__ return. */
int kws_loss_forward(const float *y_pred, const int32_t *labels, const float *class_weights, int from_logits,
                     int ignore_index, int B, int C, float *losses, void *stream);

/* keras.optimizers.Adam update (common/model_utils.py:47) on flat buffers of n floats, step count t >= 1:
 *   lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t); m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr_t m/(sqrt(v)+eps)
 * with g = grad_scale * grads. */
int kws_adam_step(float *params, const float *grads, float *m, float *v, int64_t n, float lr, float beta1, float beta2,
                  float eps, int64_t t, float grad_scale, void *stream);

/* Evaluation (eval.py:201-256): counts[label * C + pred] += 1 for every sample of the batch (int32, caller zeroes it). */
int kws_confusion_counts(const int32_t *labels, const int32_t *pred, int B, int C, int32_t *counts, void *stream);

/* Score statistics of a batch, from which the host derives per-class ROC / DET curves, top-k accuracy and calibration
 * (kws_amd/metrics.py): one read of probs (B, C) and labels (B), integer counts only.  Every output
 * ACCUMULATES (the caller zeroes it once and calls per batch), so the result is the same bit for bit whatever the grid, the order of
 * the atomics or the split into batches.  A sample whose label is outside [0, C) is skipped in all three outputs (callers map an
 * ignored label to -1).
 *
 *   bin of a score p (fp32):  !(p > 0) -> 0 (zero, negatives, NaN);  p >= 1 -> bins - 1;  else min(bins - 1, (int)(p * (float)bins))
 *   hist[c][1][bin]   samples whose label is c, by their score for c (targets)
 *   hist[c][0][bin]   samples whose label is another valid class, by their score for c (non-targets)
 *   rank_counts[r]    samples whose true class y has rank r = #{c : p_c > p_y} + #{c < y : p_c == p_y}: the heads' arg-max takes the
 *                     first maximum (the lowest index wins a tie), so rank_counts[0] is the trace of kws_confusion_counts over the
 *                     forward's own arg-max.  A sample with a NaN score anywhere counts at rank C - 1.
 *   calib[0][bin]     samples by the bin of their largest score (the largest bin of the row: a NaN score counts as bin 0)
 *   calib[1][bin]     the correct ones among them (rank 0)
 * rank_counts (C) and calib (2, bins) may be NULL.  B == 0 is a no-op; C >= 1, bins >= 2, else KWS_ERR_INVALID.
 *
 * Two counting paths.  While the 2 * C * bins counters of hist fit KWS_SCORE_LDS_BUDGET bytes as int32, every block counts into a
 * copy in LDS (with calib and rank_counts behind it) and adds its non-zero counters to the int64 arrays once at its end; otherwise
 * the counts go to global memory with 64-bit atomics (a lane merges a run of counts for one counter into one add).  The budget is 96 KiB: the default evaluation (12 classes, 1024 bins) fits it
 * exactly, and with the calibration counters behind it (at most half as much again for C >= 2) a block stays inside the 160 KiB
 * of a compute unit.  One block of 16 waves per compute unit holds it: tiling the classes over blocks instead would make every
 * block read every row.  kws_score_hist_uses_lds (host only, no device needed) tells which path a shape takes. */
#define KWS_SCORE_LDS_BUDGET 98304
int kws_score_hist_uses_lds(int C, int bins);
int kws_score_hist(const float *probs, const int32_t *labels, int B, int C, int bins, int64_t *hist, int64_t *rank_counts,
                   int64_t *calib, void *stream);

/* keras SGD(momentum=0) and RMSprop(rho=0.9, momentum=0, epsilon=1e-7, centered=False), model_utils.py:48-51:
 *   sgd:     p -= lr * g
 *   rmsprop: a = rho a + (1-rho) g^2;  p -= lr * g / (sqrt(a) + eps)            with g = grad_scale * grads */
int kws_sgd_step(float *params, const float *grads, int64_t n, float lr, float grad_scale, void *stream);
int kws_rmsprop_step(float *params, const float *grads, float *accum, int64_t n, float lr, float rho, float eps,
                     float grad_scale, void *stream);

/* ------------------------------------------------------------------------
 * The tf.keras optimizer_v2 options the three steps above do not take: gradient clipping (clipvalue, clipnorm,
 * global_clipnorm) on all three, momentum / nesterov on SGD, momentum / centered on RMSprop, amsgrad on Adam.
 * The buffers are flat; a segment table names the variables (for a model: one segment per trainable entry of
 * kws_model_tensor_info, padded to the next one).  With g = grad_scale * grads, the gradient transformations run
 * in Keras' _transform_gradients order:
 *   clipvalue        g = clip(g, -clipvalue, clipvalue)
 *   clipnorm         per segment, tf.clip_by_norm: g = g*c / max(||g||, c); a zero norm leaves g as it is, an inf norm
 *                    makes the finite entries 0 and the inf ones NaN, a NaN norm makes the segment NaN
 *   global_clipnorm  over all segments, tf.clip_by_global_norm: g *= c*min(1/N, 1/c); a non-finite N makes every entry NaN
 * clipnorm and global_clipnorm are exclusive; a value of 0 is "off".  Then, t the 1-based step count:
 *   sgd      momentum == 0: p -= lr g  (nesterov ignored);  else a = momentum a - lr g;  p += a  or, nesterov, p += momentum a - lr g
 *   rmsprop  ms = rho ms + (1-rho) g^2;  centered: mg = rho mg + (1-rho) g, d = ms - mg^2, else d = ms;
 *            momentum == 0: p -= lr g / (sqrt(d) + eps);  else mom = momentum mom + lr g / sqrt(d + eps); p -= mom
 *            (eps inside the sqrt with momentum: ResourceApply[Centered]RMSProp)
 *   adam     as kws_adam_step; amsgrad: vhat = max(vhat, v), p -= lr_t m / (sqrt(vhat) + eps)
 * Launches: one when no norm clipping is asked for; else two -- per-block sums of squares of the value-clipped g
 * (every block lies inside one segment), then the fused update, each of whose blocks sums the partials it needs in a
 * fixed order.  No atomics, no host synchronisation: the same inputs give the same bits.
 * Elements outside every segment are not touched.
 *
 * Weight averaging (tensorflow-addons' MovingAverage, SWA and Lookahead) is folded into the update pass: with p' the new
 * parameter and avg the averaging slot,
 *   KWS_AVG_BLEND    avg = avg - (avg - p') * avg_alpha;  p' is stored unchanged   (avg_alpha == 1: avg = p')
 *   KWS_AVG_SYNC     s = avg + avg_alpha * (p' - avg);  avg = s and p = s
 *   KWS_AVG_NONE     avg is neither read nor written
 * The step keeps no schedule: the caller chooses mode and alpha per step (common/model_utils.py: average_args) and starts the
 * slot as a copy of params.  No further launch, no atomics.
 * ---------------------------------------------------------------------- */
enum { KWS_OPT_SGD = 0, KWS_OPT_RMSPROP = 1, KWS_OPT_ADAM = 2 };
enum { KWS_OPT_NESTEROV = 1, KWS_OPT_CENTERED = 2, KWS_OPT_AMSGRAD = 4 };
enum { KWS_AVG_NONE = 0, KWS_AVG_BLEND = 1, KWS_AVG_SYNC = 2 };

/* Host only.  Segment i is [offsets[i], offsets[i] + sizes[i]): sorted, not overlapping, offsets multiples of 4, sizes > 0.
 * Returns the bytes of the optimizer workspace (a block table, then one double per block), or a negative kws error code. */
int64_t kws_optimizer_workspace_bytes(const int64_t *offsets, const int64_t *sizes, int n_segments);
/* Host only: writes the workspace's block table into host_ws (ws_bytes >= kws_optimizer_workspace_bytes) and its block count
 * into *n_blocks.  Copy host_ws to the device once; the steps only read the table and use the rest as scratch. */
int kws_optimizer_plan(const int64_t *offsets, const int64_t *sizes, int n_segments, void *host_ws, int64_t ws_bytes,
                       int32_t *n_blocks);

typedef struct kws_optimizer_args {
    int32_t kind;           /* KWS_OPT_SGD / KWS_OPT_RMSPROP / KWS_OPT_ADAM */
    int32_t flags;          /* KWS_OPT_NESTEROV (sgd), KWS_OPT_CENTERED (rmsprop), KWS_OPT_AMSGRAD (adam) */
    float *params;
    const float *grads;
    float *m;               /* adam: first moment */
    float *v;               /* adam: second moment; rmsprop: ms (the accum of kws_rmsprop_step) */
    float *vhat;            /* adam with amsgrad */
    float *mg;              /* centered rmsprop */
    float *mom;             /* sgd / rmsprop with momentum > 0 */
    void *ws;               /* device copy of the planned workspace, 16-byte aligned */
    int64_t ws_bytes;
    int32_t n_blocks;       /* from kws_optimizer_plan */
    float lr;
    float beta1;            /* adam */
    float beta2;            /* adam beta_2; rmsprop rho */
    float eps;              /* adam / rmsprop */
    float momentum;         /* sgd / rmsprop, in [0, 1] */
    int64_t t;              /* 1-based step count (adam) */
    float grad_scale;
    float clipvalue;        /* 0: off */
    float clipnorm;         /* 0: off */
    float global_clipnorm;  /* 0: off */
    /* appended: a zero-filled tail is "no averaging" */
    float *avg;             /* averaging slot: same length and layout as params, 16-byte aligned; NULL when avg_mode == 0 */
    int32_t avg_mode;       /* KWS_AVG_NONE / KWS_AVG_BLEND / KWS_AVG_SYNC */
    float avg_alpha;        /* BLEND: weight of the new parameter; SYNC: slow_step_size; in [0, 1] */
} kws_optimizer_args;

/* One update on `stream` by the rules above.  The buffers the kind / flags / momentum need are non-NULL and 16-byte aligned. */
int kws_optimizer_step(const kws_optimizer_args *args, void *stream);

/* Exchanges params and avg inside the segments of the planned workspace `ws` (device copy, as kws_optimizer_args.ws); padding is
 * not touched.  Exact: two calls restore every bit. */
int kws_optimizer_swap(float *params, float *avg, const void *ws, int64_t ws_bytes, int32_t n_blocks, void *stream);

/* ------------------------------------------------------------------------
 * Streaming post-processing: replaces the per-chunk work of listen.py for S
 * concurrent audio streams that advance in lockstep (one chunk each per step):
 *   Listener.update_vectors   listen.py:96-114   sliding feature matrix
 *   ThresholdDecoder          listen.py:452-522  logit-normal cumulative table
 *   TriggerDetector.update    listen.py:525-559  activation counter
 *   the loop around them      listen.py:350-375  argmax / max / decode / update
 * New MFCC rows come from kws_featurize_raw() on the carried + new samples.
 * ------------------------------------------------------------------------ */
typedef struct kws_decoder kws_decoder;

/* ThresholdDecoder.__init__ (listen.py:467-472): mu_stds is n pairs (mu, std) on the host; the cumulative table
 * (resolution * out_range float64 entries) is built once in double precision and kept on the device. */
int kws_decoder_create(const double *mu_stds, int n, double center, int resolution, double min_z, double max_z,
                       kws_decoder **out);
void kws_decoder_destroy(kws_decoder *d);
/* min_out, out_range (= max_out - min_out) and len(cd) */
int kws_decoder_info(const kws_decoder *d, int32_t *min_out, int32_t *out_range, int64_t *table_len);
/* host copy of the table `cd` (count must equal table_len) */
int kws_decoder_table(const kws_decoder *d, double *host_cd, size_t count);
/* ThresholdDecoder.decode (listen.py:496-508) on n device values.  raw_dtype KWS_RAW_F64: Python-float semantics;
 * KWS_RAW_F32: the live loop's semantics, where the float32 network output makes numpy evaluate 1/x - 1 in float32. */
enum { KWS_RAW_F64 = 0, KWS_RAW_F32 = 1 };
int kws_decoder_decode(const kws_decoder *d, const void *raw, int raw_dtype, double *decoded, int64_t n, void *stream);
/* ThresholdDecoder.encode (listen.py:510-517), a host-side scalar helper (searchsorted on the host copy of the table) */
int kws_decoder_encode(const kws_decoder *d, double threshold, double *raw_out);

/* mfccs = concatenate(mfccs[n:], new[-n:]) with n = min(n_rows, F) for every stream (listen.py:107-109):
 * feat (S, F, D) updated in place from rows (S, n_rows, D). */
int kws_stream_push_rows(float *feat, const float *rows, int S, int F, int D, int n_rows, void *stream);

/* TriggerDetector.update (listen.py:538-559) for S streams: state (S, 2) int32 = {activation, record_index}, start it
 * at {0, -1}.  fired[s] = 1 when the prediction activates the stream. */
int kws_trigger_update(const int32_t *index, const double *score, int S, int background_index, double sensitivity,
                       int trigger_level, int chunk_size, int32_t *state, int32_t *fired, void *stream);

/* One step of the loop listen.py:361-375 for S streams, fused: probs (S, C) float32 -> index = argmax, score = max,
 * decoded through `dec` unless the class is background (dec may be NULL: no decoding), then the trigger update above. */
int kws_stream_postprocess(const kws_decoder *dec, const float *probs, int S, int C, int background_index,
                           double sensitivity, int trigger_level, int chunk_size, int32_t *state, int32_t *index,
                           double *score, int32_t *fired, void *stream);

/* ------------------------------------------------------------------------
 * Ragged streaming: the same per-chunk loop for streams that do NOT advance in lockstep.  A server has S slots, each an
 * independent Listener of the reference with, per slot,
 *   window_audio  the carry, win[slot][0 : carry) int16; with H <= W at most W - 1 samples after a push, so cap = W + chunk_size
 *                 samples per slot suffice (W = window_samples, H = hop_samples);
 *   mfccs         the (F, D) feature window, initially zero;
 *   state         {activation, record_index}, initially {0, -1};
 *   sensitivity, trigger_level   its own operating point.
 * One push delivers A chunks for A DISTINCT slots, in any order, 1 <= len <= chunk_size samples each, 0 <= A <= S.  For every
 * entry it does what listen.py:96-109 and :350-375 do for one chunk:
 *   L = carry + len;  n_new = 0 if L < W else (L - W) / H + 1;
 *   new rows = vectorize_raw of the samples [j H, j H + W) of carry + chunk, j < n_new;
 *   mfccs = concatenate(mfccs[n:], new[-n:]) with n = min(n_new, F);
 *   the carry keeps the max(L - n_new H, 0) samples from n_new H on (H > W: the carry empties, as in the lockstep form);
 *   the slot's window is predicted on, ALSO when n_new == 0 (the reference predicts on every chunk); argmax, max, decode
 *   unless background, then TriggerDetector.update with the slot's own sensitivity and trigger level.  The refractory
 *   period uses the server's nominal chunk_size, as the lockstep form does.
 * Slots a push does not name are not touched in any buffer.
 *
 * The push is described by one host-built table of A entries of KWS_RAGGED_FIELDS int32 each, copied to the device with the
 * push: the slot, the carry length BEFORE the push (the host mirrors it with the three lines above, which is also how it knows
 * max_frames = max n_new without reading anything back), the chunk's length, n_new, and a flag that restarts the slot (empty
 * carry, zero window, state {0, -1}) before the chunk is taken.  The sequence of a push, all on one stream:
 *   kws_stream_ragged_append -> kws_featurize_long(act, act_len) when max_frames > 0 -> kws_stream_ragged_push_rows ->
 *   the forward pass on feat (A, F, D) -> kws_stream_ragged_postprocess.
 * Each entry point checks its arguments on the host before any launch (KWS_ERR_INVALID), does nothing for A == 0, is
 * stream-ordered and uses neither synchronisation nor atomics.  The kernels clamp what they read from the table to the
 * buffers, so a wrong table gives wrong results and no access outside them; entries naming one slot twice race.
 * ------------------------------------------------------------------------ */
enum { KWS_RAGGED_SLOT = 0, KWS_RAGGED_CARRY = 1, KWS_RAGGED_LEN = 2, KWS_RAGGED_NEW = 3, KWS_RAGGED_RESET = 4, KWS_RAGGED_FIELDS = 8 };

/* Entry a: act[a][0 : L) = win[slot][0 : carry) ++ chunks[a][0 : len), act_len[a] = L (the input of kws_featurize_long), and
 * win[slot][0 : keep) = the samples of that row from n_new H on, in the same kernel.  win (S, win_stride), act (A, act_stride):
 * rows of at least cap samples, a multiple of 8 samples long, the arrays starting on 16 bytes; chunks (A, chunk_stride), any
 * stride and alignment (rows that start on 16 bytes and are a multiple of 8 long are read 16 bytes at a time).
 * cap >= window_samples + chunk_size, at most 32768 (KWS_ERR_UNSUPPORTED beyond). */
int kws_stream_ragged_append(int16_t *win, int64_t win_stride, int S, int cap, const int16_t *chunks, int64_t chunk_stride,
                             const int32_t *table, int A, int chunk_size, int window_samples, int hop_samples, int16_t *act,
                             int64_t act_stride, int32_t *act_len, void *stream);

/* Entry a: mfccs[slot] (of mfccs (S, F, D)) slides by n = min(n_new, F) with rows[a][n_new - n : n_new) of rows
 * (A, max_frames, D), what kws_featurize_long wrote for act; the updated window is also written to feat[a] of feat (A, F, D).
 * n_new == 0 only copies; the restart flag takes the old window as zeros.  rows may be NULL when max_frames == 0. */
int kws_stream_ragged_push_rows(float *mfccs, int S, int F, int D, const float *rows, int max_frames, const int32_t *table, int A,
                                float *feat, void *stream);

/* Entry a: kws_stream_postprocess of probs[a] (probs (A, C)) with sensitivity[slot], trigger_level[slot] (device arrays of S)
 * on state[slot] (state (S, 2); the restart flag sets {0, -1} first).  The results go to index / score / fired [a] (A) and to
 * slot_index / slot_score / slot_fired [slot] (S). */
int kws_stream_ragged_postprocess(const kws_decoder *dec, const float *probs, int A, int C, const int32_t *table, int S,
                                  int background_index, const double *sensitivity, const int32_t *trigger_level, int chunk_size,
                                  int32_t *state, int32_t *slot_index, double *slot_score, int32_t *slot_fired, int32_t *index,
                                  double *score, int32_t *fired, void *stream);

/* ------------------------------------------------------------------------
 * Sample-rate conversion in front of the detector: a stream or a recording at f_in Hz becomes one at f_out Hz, streaming (state per
 * stream, any chunking gives the same samples bit for bit) or in one shot.  The reference has no counterpart on the device
 * (common/data_utils.py load_wav converts one file on the host); this comment is the definition, tests/rate_ref.py restates it.
 *
 * Rates f_in, f_out are positive integers; g = gcd(f_in, f_out), p = f_in / g, q = f_out / g, s = min(1, q / p).  Supported pairs
 * have 1/4 <= p / q <= 4 and a bank of at most KWS_RATE_MAX_BANK_BYTES (q * 2K float32); KWS_ERR_UNSUPPORTED outside either limit.
 * Z (zero crossings, 4..32), beta and rolloff have the meaning of kws_resampler_create.
 *   kernel   h(x) = rolloff sinc(rolloff x) kaiser_beta(x / Z) for 0 <= x < Z, 0 from Z on.
 *   taps     per wing K = Z if p <= q else ceil(Z p / q) = (Z p + q - 1) / q  (tap K would have weight 0 at every phase).
 *   bank     W, q rows of 2K float32, computed in float64 from the formula and rounded once (no interpolated table):
 *              W[m][k]     = s h(s (m / q + k))        the left wing,
 *              W[m][K + k] = s h(s (1 - m / q + k))    the right wing,   k < K,
 *            the distances formed from the integers m + k q and q - m + k q.
 *   output n (n = 0, 1, ... since the stream began): n0 = (n p) div q, m = (n p) mod q in 64-bit integers; acc = 0;
 *              acc = fmaf(W[m][k],     v[n0 - k],     acc)   k = 0 .. K-1, then
 *              acc = fmaf(W[m][K + k], v[n0 + 1 + k], acc)   k = 0 .. K-1,   float32, in this order;  y[n] = acc.
 *            v[j] = int16 sample j of the stream / 32768, 0 for j < 0 (the silence in front of the stream).  The int16 sample handed
 *            on is clamp(rintf(y[n] * 32768), -32768, 32767), rounding half to even.
 *   streaming  output n is emitted by the push that delivers input sample n0 + K, its rightmost tap: after N input samples in all,
 *            M(N) = 0 if N <= K else ceil((N - K) q / p) outputs have been emitted; a push of len samples emits
 *            M(N + len) - M(N) <= ceil(len q / p), so a chunk of at most floor(chunk_size p / q) input samples emits at most
 *            chunk_size.  The latency is K input samples.  Between pushes a stream keeps its last 2K - 1 input samples and N.
 *   flush / one shot  a finished stream of N samples gives ceil(N q / p) outputs in all, the taps at j >= N taken as 0; the outputs
 *            n < M(N) are bit-identical to the streaming ones.
 *   p == q   K = 0: the samples pass through bit for bit, without latency.
 * ------------------------------------------------------------------------ */
typedef struct kws_rate_bank kws_rate_bank;
enum { KWS_RATE_MAX_BANKS = 16, KWS_RATE_MAX_BANK_BYTES = 1 << 20 };

/* The bank, a HOST object (no device is needed to create or query it; the device copy is made by the first kws_rate_convert on each
 * device).  KWS_ERR_INVALID: a rate < 1, Z outside [4, 32], beta outside [0, 20], rolloff outside (0, 1]; KWS_ERR_UNSUPPORTED: see above. */
int kws_rate_bank_create(int f_in, int f_out, int zero_crossings, double beta, double rolloff, kws_rate_bank **out);
void kws_rate_bank_destroy(kws_rate_bank *bank);
/* host: p, q and K (each may be NULL) */
int kws_rate_bank_info(const kws_rate_bank *bank, int *p, int *q, int *taps);
/* host: W as (q, 2K) float32, row-major (n >= q * 2K); the device holds the same values tap-major, (2K, q) */
int kws_rate_bank_weights(const kws_rate_bank *bank, float *out, size_t n);
/* host: emitted = M(N), total = ceil(N q / p) (each may be NULL); 0 <= N <= 2^44 */
int kws_rate_counts(const kws_rate_bank *bank, int64_t N, int64_t *emitted, int64_t *total);

/* One launch is described by a host-built table of A entries of KWS_RATE_FIELDS int32 each (device memory, copied with the call's
 * audio).  Entry a: BANK, index into banks; IN_ROW and IN_LEN, its new input samples in[IN_ROW][0 : IN_LEN) (IN_LEN may be 0); N_LO /
 * N_HI, the low and high words of N, the stream's sample count before this chunk; OUT_ROW, the row of out_i16 / out_f32 it writes, -1 for an
 * entry that emits nothing and only feeds its history;
 * FIRST_LO / FIRST_HI, the index n of its first output, and COUNT, how many it writes from column 0 on -- the host computes both with M:
 * FIRST = M(N), COUNT = M(N + IN_LEN) - M(N), or ceil((N + IN_LEN) q / p) - M(N) for an entry that flushes; HIST_IN, the row of hist
 * that holds the stream's last 2K - 1 input samples (zeros in front of a shorter stream), -1 for none (zeros); HIST_OUT, the row that
 * receives them after this chunk (a chunk shorter than 2K - 1 shifts the old ones), -1 for none -- a DIFFERENT row from HIST_IN, since
 * the blocks of an entry read one while one of them writes the other; FLAGS, KWS_RATE_RESTART takes the history as zeros,
 * KWS_RATE_FINAL marks the stream's last entry: its COUNT includes the flush and no history is written.  Taps past the chunk's end are
 * taken as 0 in every entry. */
enum { KWS_RATE_BANK = 0, KWS_RATE_IN_ROW = 1, KWS_RATE_IN_LEN = 2, KWS_RATE_N_LO = 3, KWS_RATE_N_HI = 4, KWS_RATE_OUT_ROW = 5,
       KWS_RATE_FIRST_LO = 6, KWS_RATE_FIRST_HI = 7, KWS_RATE_COUNT = 8, KWS_RATE_HIST_IN = 9, KWS_RATE_HIST_OUT = 10,
       KWS_RATE_FLAGS = 11, KWS_RATE_FIELDS = 12 };
enum { KWS_RATE_RESTART = 1, KWS_RATE_FINAL = 2 };

/* Convert A entries in one stream-ordered launch: no atomics, no synchronisation, nothing read back (the first use of a bank on a device
 * uploads it, once).  in (in_rows, in_stride) int16; hist (hist_rows, hist_stride) int16 with hist_stride >= 2K - 1 of every bank, NULL
 * with hist_rows == 0 when no entry has history; out_i16 and out_f32 (out_rows, out_stride), either may be NULL: row OUT_ROW receives
 * COUNT samples and zeros from there to out_width <= out_stride (at most 65535 * 512 columns, KWS_ERR_UNSUPPORTED beyond).  Entries
 * must name distinct OUT_ROWs and distinct HIST_OUT rows.  Arguments are checked on the host before any launch (KWS_ERR_INVALID); the
 * kernel clamps what it reads from the table to the buffers, so a wrong table gives wrong samples and no access outside them.  Fixed
 * order of every sum: two calls give the same bits. */
int kws_rate_convert(const kws_rate_bank *const *banks, int n_banks, const int16_t *in, int64_t in_stride, int in_rows,
                     const int32_t *table, int A, int16_t *hist, int64_t hist_stride, int hist_rows, int16_t *out_i16, float *out_f32,
                     int64_t out_stride, int out_rows, int out_width, void *stream);

/* ------------------------------------------------------------------------
 * Offline scan: the loop above over whole recordings that already lie in memory, parallel over time.  It returns per
 * chunk what the chunk loop returns.  With W = window_samples, H = hop_samples, c = chunk_size and N samples:
 *   chunks  T = ceil(N / c); after chunk k (1-based) n_k = min(k c, N) samples have arrived (wave.readframes delivers a short
 *           last chunk, listen.py:403-428);
 *   rows    update_vectors (listen.py:96-114) featurizes the carried + new samples and keeps the remainder from
 *           len(new) * hop on, so the carry always starts on a frame boundary: after chunk k there are
 *           r_k = 0 if n_k < W else (n_k - W) / H + 1 rows, row j = vectorize_raw of samples [j H, j H + W)
 *           (kws_featurize_long computes them all at once);
 *   window  the matrix predicted on at chunk k is rows [r_k - F, r_k), zeros for negative indices (listen.py:92); chunks
 *           before the first row see the all-zero matrix and are predicted on like any other (listen.py:350-375).
 * ------------------------------------------------------------------------ */

/* feat (R * n_chunks, F, D): window i of recording r (at r * n_chunks + i) is the matrix of its chunk k0 + i (0-based), cut
 * from rows (R, max_frames, D); lengths: R device int32 sample counts.  Chunks at or past a recording's T give zeros.
 * hop_samples <= window_samples is required (KWS_ERR_INVALID otherwise): only then do the chunk loop's frames start on
 * multiples of the hop whatever the chunk size. */
int kws_stream_gather_windows(const float *rows, int R, int max_frames, const int32_t *lengths, int chunk_size,
                              int window_samples, int hop_samples, int F, int D, int64_t k0, int n_chunks, float *feat,
                              void *stream);

/* kws_stream_postprocess for the chunks k0 .. k0 + n_chunks of R recordings at once: probs (R, n_chunks, C) float32 as the
 * forward pass gives the windows above; rec_chunks: R device int32 chunk counts T.  index / score / fired: element
 * (r, i) at r * out_stride + i (out_stride >= n_chunks: a tile may be written into a column range of a larger matrix).
 * argmax / max / decode (listen.py:361-367) run per chunk in parallel; TriggerDetector.update (listen.py:538-559) is
 * walked in chunk order per recording from state (R, 2) = {activation, record_index}, which is left as after the last
 * chunk walked: calls on consecutive tiles equal kws_stream_postprocess chunk by chunk.  Chunks at or past T leave
 * the recording's state alone and get index -1, score 0, fired 0. */
int kws_stream_scan_postprocess(const kws_decoder *dec, const float *probs, int R, int n_chunks, int C,
                                const int32_t *rec_chunks, int64_t k0, int background_index, double sensitivity,
                                int trigger_level, int chunk_size, int32_t *state, int32_t *index, double *score,
                                int32_t *fired, int64_t out_stride, void *stream);

/* Operating-point sweep: TriggerDetector.update (listen.py:538-559) walked over what a scan wrote, index / score (R, stride)
 * with rec_chunks (R) chunks per recording, once per operating point p = (sensitivity[p], trigger_level[p]), p < P, every
 * walk starting from {activation 0, record_index none}.  Argmax and decoding do not depend on the point, so a scan is
 * made once and swept; one wave walks a recording at 64 points, one per lane.  Entries at or past rec_chunks[r] are not
 * read.  counts (R, P, 5) int32 = {fires, hits, false_alarms, duplicates, latency_chunks_sum}.
 * ev_off == NULL: no labels, fires alone is counted and the other four are 0.  Otherwise ev_off (R + 1) are CSR offsets
 * into ev_class / ev_lo / ev_hi (E): recording r's events, in chunk units, sorted, ev_lo[e] <= ev_hi[e] < ev_lo[e + 1].
 * A fire at chunk k of class c (the chunk's index) belongs to the event e with ev_lo[e] <= k <= ev_hi[e] if there is one
 * and ev_class[e] == c: the first such fire is a hit and adds k - ev_lo[e] to the latency sum, later ones are duplicates.
 * Every other fire is a false alarm, a fire of another class inside an event's window included.  All arrays are device
 * memory; nothing is synchronised.  R == 0 or P == 0 does nothing. */
int kws_stream_sweep(const int32_t *index, const double *score, int R, int64_t stride, const int32_t *rec_chunks,
                     int background_index, int chunk_size, const double *sensitivity, const int32_t *trigger_level, int P,
                     const int32_t *ev_off, const int32_t *ev_class, const int32_t *ev_lo, const int32_t *ev_hi,
                     int32_t *counts, void *stream);

/* The activations of R scanned recordings at ONE operating point, each with its chunk, class and kind: what
 * Listener.on_activation (listen.py:291-308) sees, for the files a scan or a sweep has already decoded.  index / score / stride /
 * rec_chunks and the event arrays are kws_stream_sweep's, with the same preconditions; the walk is TriggerDetector.update from
 * {activation 0, record_index none} per recording, recomputed here rather than read from a scan's `fired`, so any point of a
 * sweep can be collected from the same scan.  det (R, max_det, 4) int32 = {chunk, class, kind, event} in chunk order and
 * det_score (R, max_det) the chunk's decoded score; `kind` follows the rule above (the first fire of the event's class inside its
 * window is a hit, later ones duplicates, every other fire a false alarm; KWS_DET_UNLABELLED when ev_off == NULL) and `event`
 * is the event's position within its recording, -1 when the fire belongs to none.  n_det (R) is the true count, also when
 * it exceeds max_det; only the first max_det activations are stored, and the slots past min(n_det[r], max_det) are written
 * as {-1, -1, 0, -1} with score 0.  max_det == 0 only counts (det / det_score may be NULL); R == 0 does nothing.  One wave per
 * recording; nothing is synchronised. */
enum { KWS_DET_UNLABELLED = 0, KWS_DET_HIT = 1, KWS_DET_DUPLICATE = 2, KWS_DET_FALSE_ALARM = 3 };
int kws_stream_collect(const int32_t *index, const double *score, int R, int64_t stride, const int32_t *rec_chunks,
                       int background_index, int chunk_size, double sensitivity, int trigger_level,
                       const int32_t *ev_off, const int32_t *ev_class, const int32_t *ev_lo, const int32_t *ev_hi,
                       int max_det, int32_t *n_det, int32_t *det, double *det_score, void *stream);

/* The near misses of R scanned recordings: per recording the up to K highest-scoring, well-separated non-background chunks.
 * Chunk k < rec_chunks[r] is a candidate when index != background_index, score > min_score (strict) and, with events
 * (ev_off != NULL; CSR as above, the classes are not needed), k lies in no [ev_lo[e], ev_hi[e]] of its recording, whatever the
 * event's class.  Greedy, at most K times: the candidate with the largest score, ties to the lowest chunk, whose distance to
 * every chunk already picked is >= min_gap.  peaks (R, K, 2) int32 = {chunk, class} and peak_score (R, K) in pick order,
 * n_peaks (R) <= K; unused slots are {-1, -1} with score 0.  The comparisons are on the stored doubles: the result is exact and
 * the same on every run.  1 <= K <= 64 and min_gap >= 1, anything else is KWS_ERR_INVALID.  One wave per recording, no atomics;
 * nothing is synchronised. */
int kws_stream_peaks(const int32_t *index, const double *score, int R, int64_t stride, const int32_t *rec_chunks,
                     int background_index, double min_score, int min_gap,
                     const int32_t *ev_off, const int32_t *ev_lo, const int32_t *ev_hi,
                     int K, int32_t *n_peaks, int32_t *peaks, double *peak_score, void *stream);

/* ------------------------------------------------------------------------
 * Voice-activity detection of whole recordings: where the speech is, which files are silent, and the clips.  Replaces
 *   VoiceActivityDetector.detect_speech              tools/audio_process/speech_duration_check.py:149-176
 *   ._median_filter / ._smooth_speech_detection      speech_duration_check.py:88-106
 *   .convert_windows_to_readable_labels              speech_duration_check.py:108-130
 *   speech_duration_check (the `simple` type)        speech_duration_check.py:301-330
 *   silent_check                                     tools/audio_process/silent_check.py:14-24
 * for R recordings of ragged length in one packed (R, stride) buffer, int16 or float32, with device `lengths`.
 * With N = int(rate * window_t), H = int(rate * hop_t) and L samples: window w covers [w H, w H + N) for every w with
 * w H < L - N; E_k = |X_k|^2 of its N-point DFT; full = sum_{k=1..N/2} 2 E_k (Nyquist counted twice, as the
 * reference's dict does), band = the same sum over band_lo < k rate / N < band_hi; raw = band / full > energy_threshold
 * (false when full == 0); smoothed = median of int(smooth_t / window_t) windows (made odd), first and last value
 * replicated at the ends; an interval begins at the first sample of the first smoothed-1 window and ends at the first
 * sample of the next smoothed-0 window; an interval still open at the last window is dropped.
 * ------------------------------------------------------------------------ */
typedef struct kws_vad kws_vad;

/* VoiceActivityDetector.__init__ (speech_duration_check.py:25-32 holds the defaults 0.02, 0.01, 300, 3000, 0.6, 0.5).
 * Host only: the cos/sin matrix of the band bins is built in double here and uploaded by the first kws_vad_detect on a
 * device.  Geometries other than N == 2 H, N <= 1024 and a band of at most 56 bins return KWS_ERR_UNSUPPORTED. */
int kws_vad_create(int sample_rate, double window_t, double hop_t, double band_lo, double band_hi, double energy_threshold,
                   double smooth_t, kws_vad **out);
void kws_vad_destroy(kws_vad *vad);
/* N, H, the first and last band bin (inclusive) and the median's length; any pointer may be NULL */
int kws_vad_info(const kws_vad *vad, int32_t *window_samples, int32_t *hop_samples, int32_t *bin_lo, int32_t *bin_hi,
                 int32_t *median);
/* Host only: the window count of a recording of n_samples (the loop condition of speech_duration_check.py:162), or a
 * negative kws error code. */
int64_t kws_vad_windows(const kws_vad *vad, int64_t n_samples);
/* Host only: bytes of the device workspace kws_vad_detect needs (one 8-byte sum per job), or a negative error code. */
int64_t kws_vad_workspace_bytes(const kws_vad *vad, int R, int max_windows);

/* detect_speech + convert_windows_to_readable_labels + the span of speech_duration_check.py:314-330 + the energy of
 * silent_check.py:17-18 for all recordings, in two launches on `stream` without host synchronisation.  All pointers
 * but `vad` are device memory; max_windows >= kws_vad_windows(stride).
 *   ratio (R, max_windows) float32       band / full; 0 where full <= 0 and past a recording's window count
 *   smoothed (R, max_windows) uint8      the smoothed flags; 0 past the window count
 *   segments (R, max_segments, 2) int32  {begin, end} sample indices in window order; 0 past the count
 *   n_segments (R) int32                 the true count, also when it exceeds max_segments
 *   span (R, 2) int32                    {min begin, max end}, or {0, 0} without an interval
 *   energy_per_second (R) float64        sum((x / 32768)^2) / (L / rate) (float32 input: sum(x^2)); 0 for L == 0
 * The same inputs give the same bits (fixed summation order, no float atomics); samples at or past lengths[r] are never
 * read. */
int kws_vad_detect(const kws_vad *vad, const void *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths,
                   int max_windows, int max_segments, void *workspace, int64_t workspace_bytes, float *ratio,
                   uint8_t *smoothed, int32_t *segments, int32_t *n_segments, int32_t *span, double *energy_per_second,
                   void *stream);

/* Clips for kws_featurize / raw-audio training from n device triples {recording, begin, end} (sample indices, e.g. the
 * segments above): clip i is cut from [max(0, begin - pad_before), min(L, end + pad_after)) and scaled as the featurizer
 * scales (int16 / 32768).  KWS_VAD_ALIGN_LEFT_PAD: zeros in front of a shorter cut (audio_to_feature, common/data_utils.py:77-80);
 * KWS_VAD_ALIGN_CENTER: zeros on both sides, the odd one at the end.  A longer cut keeps its head.  A recording index
 * outside [0, R) gives a clip of zeros.  clips: (n, clip_samples) float32. */
enum { KWS_VAD_ALIGN_LEFT_PAD = 0, KWS_VAD_ALIGN_CENTER = 1 };
int kws_vad_gather_clips(const void *wav, int wav_dtype, int R, int64_t stride, const int32_t *lengths, const int32_t *triples,
                         int n, int clip_samples, int pad_before, int pad_after, int align, float *clips, void *stream);

/* ------------------------------------------------------------------------
 * Labelled streaming test recordings from clips: what TensorFlow's speech_commands example does on the host with
 * generate_streaming_test_wav.py (clips laid at random gaps over a continuous background, their positions written down), on the device
 * and for R recordings at once.  Recording r has N_r samples and sits at global position p = position_base + r; every draw is
 * h(i) = aug_hash(seed, (uint32)p, i) (csrc/kws_wave_stage.h, restated in tests/aug_ref.py):
 *   bed     k = aug_uniform(h(0), K), o = aug_uniform(h(1), seg_len[k]), bed_gain = fmaf(aug_unit(h(2)), hi - lo, lo): the bed of the
 *           whole recording is segment k of the noise bank read circularly from o at ONE gain, so it stays continuous
 *   slot j  row_j = pick[aug_uniform(h(4 + 3 j), M)] (no pick table: the drawn number itself, M = rows),
 *           gap_j = gap_lo + aug_uniform(h(5 + 3 j), gap_hi - gap_lo + 1), snr_j = snr_db[aug_uniform(h(6 + 3 j), n_snr)];
 *           the index depends on j alone, so a larger max_events changes no earlier draw
 *   place   len_j = min(clamp(valid_len[row_j], 0, stride), clip_cap); start_j = lead_in + sum_{i<j} (len_i + gap_i) + gap_j;
 *           n_events = the number of leading slots with start_j + len_j <= N_r: the first slot that does not fit ends the recording
 *   gain    p_v = mean(v[0:len]^2), p_n = bed_gain^2 mean(n_k[(o + start + i) mod seg_len[k]]^2, i < len), both in fp64;
 *           gain = min(max_gain, (float)sqrt(10^(snr/10) p_n / (p_v + FLT_EPSILON))); gain = 1 when n_snr == 0 or there is no bank,
 *           0 for len == 0.  The voice is scaled against the bed under it (the noise mix above scales the noise against the voice)
 *   sample  x[t] = bed_gain n_k[(o + t) mod seg_len[k]] (0 without a bank); inside event e, u = t - start_e:
 *           w = min(1, (u + 1) inv_fade, (len_e - u) inv_fade), inv_fade = 1.0f / (fade + 1);
 *           x[t] = fmaf(gain_e w, v[row_e][u], x[t]); t in [N_r, out_stride) is 0
 * Divergences from the TensorFlow tool: the draws are counter-based and made per recording on the device (no host loop over events);
 * the gap is uniform between two bounds; the clip's level is set by an SNR against the bed under it instead of a fixed gain; a
 * linear fade at both ends of a clip; the bed is one circular segment per recording instead of a fresh cut per second; clips of
 * every class are drawn alike (the caller leaves the background's clips out of its events).
 * ---------------------------------------------------------------------- */
typedef struct kws_synth_params {
    int32_t gap_lo, gap_hi;            /* samples between two clips, 0 <= gap_lo <= gap_hi */
    int32_t lead_in;                   /* samples before the first gap, >= 0 */
    int32_t clip_cap;                  /* a clip is cut to this many samples, >= 1 */
    int32_t n_snr;                     /* 0..KWS_AUG_MAX_SNR; 0: every gain is 1 */
    float snr_db[KWS_AUG_MAX_SNR];
    float bed_gain_lo, bed_gain_hi;    /* bed_gain_lo <= bed_gain_hi */
    float max_gain;                    /* > 0 */
    int32_t fade;                      /* samples of the linear fade at both ends of a clip, 0 = off */
    int32_t reserved;
    uint64_t seed;
} kws_synth_params;

/* one recording's bed (16 bytes, device memory); without a bank {-1, 0, 0, n_events} */
typedef struct kws_synth_rec {
    int32_t segment;      /* k */
    int32_t offset;       /* o */
    float bed_gain;
    int32_t n_events;
} kws_synth_rec;

/* one slot of a recording (32 bytes, device memory); a slot at or past n_events is {-1, 0, 0, 0, 0} */
typedef struct kws_synth_event {
    int32_t row;          /* row of the clip store */
    int32_t start;        /* first sample in the recording */
    int32_t length;       /* len */
    float snr_db;         /* the drawn SNR (0 when n_snr == 0) */
    float gain;
    int32_t reserved[3];
} kws_synth_event;

#define KWS_SYNTH_MAX_EVENTS 4096

/* Plan R recordings without host synchronisation: the draws and the placement by one wave per recording (lanes stride over the slots,
 * an inclusive scan in int64 with a carry between groups of 64), then the gains by one wave per placed slot (fp32 lane partials, an
 * fp64 wave sum: a fixed order, the same bits on every run; p_n from the bank's prefix sums as whole loops of the segment plus at most
 * two pieces).  wav (rows x stride) of wav_dtype, valid_len (rows device int32, NULL: stride), pick (M device int32 row numbers, NULL:
 * every row), bank (NULL: a silent bed), lengths (R device int32, each N_r >= 0), rec (R) and events (R x max_events) device records.
 * KWS_ERR_INVALID: gap_lo < 0 or gap_hi < gap_lo, lead_in < 0, clip_cap < 1, n_snr outside 0..KWS_AUG_MAX_SNR or an SNR that is not
 * finite, bed_gain_hi < bed_gain_lo, max_gain <= 0, fade < 0, max_events outside 1..KWS_SYNTH_MAX_EVENTS, an unknown wav_dtype, a
 * negative R, stride or position_base, rows or M < 1; KWS_ERR_UNSUPPORTED: stride > INT_MAX.  All of it is reported before any device
 * work.  R == 0 does nothing. */
int kws_synth_plan(const kws_noise_bank *bank, const kws_synth_params *params, const void *wav, int wav_dtype, int rows, int64_t stride,
                   const int32_t *valid_len, const int32_t *pick, int M, const int32_t *lengths, int R, int max_events,
                   int64_t position_base, kws_synth_rec *rec, kws_synth_event *events, void *stream);

/* Render the planned recordings: out (R x out_stride) of out_dtype, KWS_WAV_F32 or KWS_WAV_I16 = rint(x * 32768) saturated to
 * [-32768, 32767].  max_len: the largest N_r (host; lengths[r] above it is cut to it), out_stride >= max_len.  The grid is (tiles of
 * a row, R); a block finds the events that meet its tile by binary search over the sorted slots and stages them in LDS; the stores are 128 bits wide when
 * out and out_stride allow it.  Precondition, NOT checked (rec and events are device memory): the first n_events slots of a
 * recording are sorted by start and do not overlap, as kws_synth_plan writes them.  A slot whose row lies outside [0, rows) is
 * skipped and its length is cut to stride, so no clip is read past its row; the bank is read inside segment k only (a segment
 * outside [0, K) gives a silent bed).  KWS_ERR_INVALID: fade < 0, max_events outside 1..KWS_SYNTH_MAX_EVENTS, an unknown dtype,
 * out_stride < max_len, a negative R, rows, stride or max_len; KWS_ERR_UNSUPPORTED: stride or max_len > INT_MAX.  R == 0 does nothing. */
int kws_synth_render(const kws_noise_bank *bank, const void *wav, int wav_dtype, int rows, int64_t stride, const kws_synth_rec *rec,
                     const kws_synth_event *events, int max_events, const int32_t *lengths, int R, int64_t max_len, int fade,
                     void *out, int out_dtype, int64_t out_stride, void *stream);

/* ------------------------------------------------------------------------
 * Transfer to a new keyword set: the activations in front of the last Dense layer ("embeddings") of a frozen backbone, and a
 * trainer for Dense(E -> C, softmax) heads on them (csrc/kws_transfer.hip).
 * ---------------------------------------------------------------------- */
/* Host only: E = 128 for simple_cnn / simple_cnn_lite (dense, after ReLU6), 48 for simple_gru / simple_lstm (the last layer's final
 * state), whatever num_layers is.  0 for a NULL model. */
int kws_model_embed_size(const kws_model *m);
/* emb (B, E) float32: what score_predict reads in inference mode (BatchNormalization moving statistics, no dropout).  Workspace of
 * kws_model_workspace_bytes(m, B, 0).  Always runs the unfused layer chain at the model's matrix precision: simple_cnn's one-kernel
 * tail and simple_cnn_lite's fp16 forward never materialise the activation, so the inference precision (KWS_INFER_FP16) is ignored.
 * Rewrites the weight-derived tables of `ws`: a state prepared there by kws_model_prepare_inference is dropped. */
int kws_model_embed(kws_model *m, const float *feat, int B, const float *params, const float *state, void *ws, size_t ws_bytes,
                    float *emb, void *stream);

/* One head to train.  Offsets are in elements of the shared arrays handed to kws_head_fit. */
typedef struct kws_head_job {
    int64_t order_offset;        /* first entry of this job's slice of `order`                                            */
    int64_t weight_offset;       /* first float of this job's kernel (E, C) row-major, followed by its bias (C): Keras Dense
                                    layout; the same offset addresses the job's optimizer slots                            */
    int64_t class_weight_offset; /* first of C floats in `class_weights`, or < 0: the plain (clipped) loss                 */
    int64_t t0;                  /* steps already taken (>= 0): step s of the launch is Adam's t = t0 + s, s = 1 ..        */
    int32_t n_order;             /* entries of the slice; steps = ceil(n_order / batch); 0: the job is left untouched      */
    int32_t batch;               /* rows per step; the last step takes the rest and averages over its own size             */
    int32_t num_classes;         /* 2 .. kws_head_fit_max_classes(E)                                                       */
    int32_t ignore_index;        /* <= 0: off                                                                              */
    int32_t optimizer;           /* KWS_OPT_ADAM or KWS_OPT_SGD                                                            */
    float lr, beta1, beta2, eps; /* Adam: keras defaults are 0.9, 0.999, 1e-7                                              */
    float momentum;              /* SGD, in [0, 1], no nesterov (the rule above kws_optimizer_step)                        */
    int32_t reserved[2];         /* 0: the struct is 80 bytes */
} kws_head_job;

/* Host only: the most classes a head on E-wide embeddings may have (0 for an E kws_head_fit does not take).  The kernel keeps a
 * job's weights, optimizer slots and gradient sums in registers, 32 elements of the kernel matrix per thread and slot, next to at
 * most 160 KiB of LDS tiles per block; the smaller of the two bounds is reported: 64 at E = 128. */
int kws_head_fit_max_classes(int E);

/* Trains J independent heads in ONE launch, one 256-thread block per job, every step of a job inside the block.
 * emb (N, E) float32 and labels (N) int32 are shared; order holds int32 row numbers into them.  Step s of job j takes the next `batch`
 * entries of its slice: logits = X W + b, softmax, the loss and dlogits of the train heads (plain: p_y clipped to [1e-7, 1 - 1e-7],
 * gradient gated by the clip; weighted: unclipped; ignored samples give zero loss and a zero row; the mean runs over every row of
 * the step), dW = X^T dlogits, db = column sums, then the update: KWS_OPT_ADAM by the formula of kws_adam_step with t = t0 + s,
 * KWS_OPT_SGD by the rule above kws_optimizer_step (momentum 0: p -= lr g).  All arithmetic is float32, every sum runs in a fixed
 * order, jobs never interact: the same inputs give the same bits on every run and for every J.
 *   weights        in: initial value, out: trained                        (addressed by weight_offset, (E + 1) C floats per job)
 *   slot_m, slot_v in/out optimizer slots in the layout of `weights`: Adam's m and v; SGD with momentum: slot_m is the momentum
 *                  buffer.  Either may be NULL: the slot then starts at zero and is not stored.
 *   stats          (J, 2) floats: the sum of the per-sample losses and the number of top-1 hits over all steps of the launch.  A job
 *                  with n_order == 0 writes nothing at all, its stats included.
 *   jobs           host array; jobs_dev: device scratch of J * sizeof(kws_head_job) bytes, 8-byte aligned, that the call fills on
 *                  `stream`.
 * Checked on the host before any HIP call: KWS_ERR_INVALID for J < 1, N < 1, E not a multiple of 4 in 4 .. 128, a NULL buffer,
 * batch < 1, num_classes < 2, n_order < 0, negative offsets or t0, a momentum outside [0, 1], a class_weight_offset >= 0 without
 * class_weights; KWS_ERR_UNSUPPORTED for another optimizer and for num_classes > kws_head_fit_max_classes(E) (the message names the
 * limit).  The device arrays `order` and `labels` are trusted, as kws_featurize_gather's index: entries of order in [0, N), labels in
 * [0, num_classes). */
int kws_head_fit(const float *emb, const int32_t *labels, int64_t N, int E, const int32_t *order, const float *class_weights,
                 const kws_head_job *jobs, void *jobs_dev, int J, float *weights, float *slot_m, float *slot_v, float *stats,
                 void *stream);

/* ------------------------------------------------------------------------
 * A bank of heads on one backbone: the serving half of the transfer block (csrc/kws_heads.hip).  The backbone
 * runs once over all rows (kws_model_embed); kws_heads_apply then gives every row the Dense(E -> C_h, softmax) head that row names,
 * out of H heads resident on the device: a keyword set per stream, or every fold's head on its own held-out rows, in one launch.
 *
 * Bank layout.  Head h is C_h = head_classes[h] classes wide, 2 <= C_h <= Cmax <= KWS_HEADS_MAX_CLASSES; its kernel matrix (E, C_h),
 * row-major, followed by its bias (C_h), lies at weights + head_offset[h]: kws_head_fit's layout, so a fitted head is copied in as it
 * is.  weights holds weights_count floats; head_offset (H) int64 and head_classes (H) int32 are DEVICE arrays, so a head is replaced
 * or emptied (head_classes[h] = 0) by stream-ordered copies between two launches.  E is a multiple of 4 in 4 .. 128, as for
 * kws_head_fit.  KWS_HEADS_MAX_CLASSES is the largest value kws_head_fit_max_classes(E) takes over those E (256, for E <= 32; it is
 * 64 at E = 128), so every head kws_head_fit can train can be banked.
 *
 * Rows.  Row r of the R output rows reads emb[rows[r]] (rows NULL: emb[r], and then R <= N), has the key key[r * key_stride], and its
 * head is the key itself (head_of_key NULL) or head_of_key[key] with key in [0, K).  A streaming push passes key = table +
 * KWS_RAGGED_SLOT, key_stride = KWS_RAGGED_FIELDS, head_of_key = the server's per-slot head array, K = S: no gather, no read-back.
 *
 * Arithmetic, all float32.  logit[c] is ONE chain: acc = b_c; acc = fma(x_e, W[e][c], acc) for e = 0, 1, .. E - 1.  m = max_c logit[c];
 * p_c = exp(logit[c] - m) / sum, the sum taken over c = 0, 1, .. C_h - 1 in that order, exp the precise expf and the division IEEE.
 * pred is the arg-max of the logits, an exact tie going to the lower class.  Columns C_h .. Cmax - 1 of logits and probs are written
 * as 0 (a padded zero cannot win an arg-max over probabilities: the largest of them is at least 1 / C_h).
 * Independence.  A row's outputs depend on its embedding row and its head alone: not on R, on its position, on the rows that share
 * its tile or on the other heads.  No atomics; the same bits on every run.  A tile whose rows all name one head reads that head from
 * LDS instead of from memory; the chains are the same, so are the bits.
 *
 * Trust and clamping, as in the ragged-streaming entry points: key (R entries at key_stride) and rows (R) are read as given; whatever
 * they lead to is checked.  A row is written as zeros with pred = -1, and nothing is read outside emb, head_of_key, head_offset,
 * head_classes or weights, when rows[r] is outside [0, N), its key is outside [0, K), its head id is outside [0, H), head_classes[h]
 * is outside 2 .. Cmax, or head_offset[h] is negative or head_offset[h] + (E + 1) C_h runs past weights_count.
 *
 * logits, probs: NULL or (R, Cmax) float32; pred: NULL or (R) int32.  One launch, stream-ordered, no synchronisation.
 * Checked on the host before any HIP call (KWS_ERR_INVALID): E not a multiple of 4 in 4 .. 128, N < 0, R < 0, H < 1, Cmax outside
 * 2 .. KWS_HEADS_MAX_CLASSES, key_stride < 1, weights_count < 0, a NULL emb / key / weights / head_offset / head_classes, an emb that
 * is not 16-byte aligned, head_of_key with K < 1, all three outputs NULL, rows == NULL with R > N.  R == 0 does nothing and returns
 * KWS_OK.
 * ---------------------------------------------------------------------- */
#define KWS_HEADS_MAX_CLASSES 256
#define KWS_HEADS_TILE_ROWS 16         /* consecutive rows one block handles; no result depends on it (the tests cut their runs around it) */
int kws_heads_apply(const float *emb, int64_t N, int E, const int32_t *rows, const int32_t *key, int64_t key_stride,
                    const int32_t *head_of_key, int64_t K, int64_t R, const float *weights, int64_t weights_count,
                    const int64_t *head_offset, const int32_t *head_classes, int H, int Cmax, float *logits, float *probs,
                    int32_t *pred, void *stream);

/* ------------------------------------------------------------------------
 * Nearest neighbours over embeddings: which rows of an (N, E) matrix look alike (csrc/kws_knn.hip).  The
 * reference's hygiene tools (tools/audio_process/wav_check.py, silent_check.py, speech_duration_check.py) look at one file at a time;
 * this looks at pairs: duplicates across a train / validation split, clips whose neighbours carry another label, k-NN as a classifier.
 *
 * Scores.  E is a multiple of 4 in 4 .. 128 (as kws_head_fit), k is in 1 .. KWS_KNN_MAX_K, N in 1 .. 2^31 - 1.
 *   KWS_KNN_DOT  score = q.r                          best = largest
 *   KWS_KNN_L2   score = max(0, (q.q + r.r) - 2 q.r)   best = smallest
 * Cosine similarity is KWS_KNN_DOT on rows that went through kws_rows_normalize; it is not a third metric.  Every dot product (q.r,
 * q.q and r.r alike) is ONE float32 chain acc = fma(a_c, b_c, acc) over the columns c in ascending order, starting from 0 -- what
 * v_mfma_f32_32x32x2_f32 computes -- so a score depends on its two rows only, not on the tile, slice or launch that computed it.
 * KWS_KNN_L2 caveat: the expansion loses the distance of near-identical rows to cancellation (two rows that differ in the last bits
 * come out at 0 or at a few ulp of q.q, in any order); a search for duplicates uses cosine.
 * Order.  Candidates are ordered by the pair (score, reference index): the better score first, at equal score the lower index; the k
 * output entries of a query are sorted in that order.  The order is total, so the result is the same bits for every `slices` and
 * every block schedule; there are no atomics.  Where fewer than k candidates exist the tail is idx = -1 with score = -inf (DOT) /
 * +inf (L2).  A NaN score ranks last among the candidates and is REPORTED as the worst score (-inf / +inf) with its index; other
 * non-finite inputs are compared as IEEE compares them.  A NaN never touches another query's row.
 * ---------------------------------------------------------------------- */
#define KWS_KNN_MAX_K 64
enum { KWS_KNN_DOT = 0, KWS_KNN_L2 = 1 };

/* out[i] = x[i] / ||x[i]|| (a zero row stays zero); norms: NULL or (N), the norms.  out may be x.  The sum of squares is taken in
 * double, so the norm is the correctly rounded one and a unit row is the float32 nearest to the exact quotient.  x and out 16-byte
 * aligned.  N == 0 does nothing.  KWS_ERR_INVALID: E, N < 0, a NULL or misaligned x / out. */
int kws_rows_normalize(const float *x, int64_t N, int E, float *out, float *norms, void *stream);

/* Host only.  Bytes of the workspace kws_knn needs with the same arguments: 0 for one slice, else `slices` x Q x k (index, score)
 * pairs rounded up to 256 bytes.  slices == 0 asks for the library's choice, which depends on Q and N only.  A negative kws_status
 * for arguments kws_knn refuses. */
int64_t kws_knn_workspace_bytes(int64_t Q, int64_t N, int E, int k, int slices);

/* For every query row, its k best reference rows.  queries (Q, E), refs (N, E), 16-byte aligned; idx (Q, k) int32, score (Q, k) float32.
 * exclude: NULL or (Q) int32, the reference row query i must skip (-1: none); a search of a set in itself passes i.
 * slices: 0 = the library chooses (a small Q gets enough blocks to fill the chip, a large Q gets 1); 1 .. 1024 = the N reference rows
 * are cut into that many runs of 32-row tiles, handled by different blocks, and merged by the total order above.  Slices past the last
 * tile are empty, which is allowed.  The Q x N scores never reach memory.
 * Checked on the host before any device work: KWS_ERR_INVALID for E, k, N, Q < 0, the metric, slices outside 0 .. 1024, a NULL or
 * misaligned queries / refs, a NULL idx / score; KWS_ERR_WORKSPACE for more than one slice with ws NULL or ws_bytes below
 * kws_knn_workspace_bytes.  Q == 0 does nothing and returns KWS_OK. */
int kws_knn(const float *queries, int64_t Q, const float *refs, int64_t N, int E, int metric, int k, const int32_t *exclude, int slices,
            int32_t *idx, float *score, void *ws, size_t ws_bytes, void *stream);

/* Votes of the neighbours kws_knn found.  labels (N) int32: the labels of the reference rows; C classes, 2 .. 1024.
 * An entry with idx = -1, or whose label lies outside [0, C), casts no vote.  weighted == 0: every vote counts 1.  weighted != 0: a vote
 * counts its score, a negative (or NaN) score counts 0 -- meaningful for KWS_KNN_DOT scores only; this function cannot see the metric,
 * kws_amd.neighbors refuses the combination with L2.
 *   pred (Q)     the class with the most votes, a tie goes to the lower class; -1 for a query whose votes sum to 0
 *   support (Q)  pred's share of the votes (0 without a vote)
 *   own          NULL or (Q): the share of own_labels[i] (own_labels NULL <=> own NULL)
 * KWS_ERR_INVALID: k, C, Q < 0, N outside 1 .. 2^31 - 1, a NULL idx / labels / pred / support, weighted without score, own without
 * own_labels or the reverse.  Q == 0 does nothing. */
int kws_knn_vote(const int32_t *idx, const float *score, int64_t Q, int k, const int32_t *labels, int64_t N, int C, int weighted,
                 const int32_t *own_labels, int32_t *pred, float *support, float *own, void *stream);

/* ------------------------------------------------------------------------
 * Query-by-example keyword search: where in a recording does something occur that sounds like these few examples?  No model, no
 * labels and no one-second framing: subsequence dynamic time warping of templates (the MFCC rows of the examples) against the rows
 * kws_featurize_long gives whole recordings (csrc/kws_dtw.hip).
 *
 * A template q has L rows, 1 <= L <= KWS_DTW_MAX_ROWS; a recording x has n rows; all rows are D wide, D a multiple of 4 in 4 .. 64
 * (pad with zero columns, which change neither metric).  Local cost of template row i against frame j:
 *   KWS_DTW_DOT  d(i, j) = 1 - q_i . x_j        (cosine distance on rows that went through kws_rows_normalize; nothing is normalised here)
 *   KWS_DTW_L2   d(i, j) = sum_k (q_ik - x_jk)^2
 * Both are ONE float32 chain acc = fma(., ., acc) over the columns in ascending order, starting from 0.  The recurrence is slope
 * constrained and every path weighs L in total:
 *   C(0, j) = d(0, j)                  S(0, j) = j                (a match may begin at any frame)
 *   C(i, j) = min( C(i-1, j-1) +   d(i, j),       candidate 1
 *                  C(i-1, j-2) +   d(i, j),       candidate 2
 *                  C(i-2, j-1) + 2 d(i, j) )      candidate 3     (a candidate with a negative index does not exist)
 *   S(i, j) = S of the winning candidate; a tie goes to the lower candidate number
 *   cost[j] = C(L-1, j) / L            start[j] = S(L-1, j)
 * in float32 throughout.  A cell without a finite candidate is +inf with start -1 (the first ceil((L-1)/2) frames of a recording);
 * frames j >= n are +inf / -1; cost and start are written for every j < max_frames.  A match that ends at frame j spans
 * ceil((L+1)/2) .. 2L - 1 frames, so every path to (L-1, j) lies in the columns >= j - 2 (L-1): a recording is cut into tiles of
 * frames that each recompute a halo of 2 (L-1) frames, and the result is the SAME BITS for every tile size.  No atomics.
 * ---------------------------------------------------------------------- */
#define KWS_DTW_MAX_ROWS 64
#define KWS_DTW_MAX_HITS 64
enum { KWS_DTW_DOT = 0, KWS_DTW_L2 = 1 };

/* Host only.  Bytes of the workspace kws_dtw needs with the same arguments, or a negative kws_status for arguments kws_dtw refuses.
 * The DP lives in registers and a tile recomputes its halo instead of taking it from its neighbour, so this is 0 today; callers
 * still ask, so that a later kernel may need one. */
int64_t kws_dtw_workspace_bytes(int R, int Q, int max_frames, int D, int tile_frames);

/* Every template against every recording.  All pointers but `ws` are device memory.
 *   templates (Q, Lmax, D), 16-byte aligned; tmpl_len (Q) int32, the rows of each (clamped to 0 .. Lmax; 0 rows match nothing)
 *   rows (R, max_frames, D), 16-byte aligned, as kws_featurize_long writes them; n_frames (R) int32 (clamped to 0 .. max_frames)
 *   cost (R, Q, max_frames) float32, start (R, Q, max_frames) int32
 *   tile_frames: 0 = the library cuts the frames so that the chip is filled (from R, Q and max_frames alone: the lengths live on the
 *   device); 32 .. 2^20 = that many frames per job.  Any value gives the same bits.
 * One launch, no host synchronisation, nothing read back.  Checked on the host before any device work: KWS_ERR_INVALID for D, R < 0,
 * Q < 0, max_frames outside 1 .. 2^30, Lmax outside 1 .. KWS_DTW_MAX_ROWS, the metric, tile_frames, a NULL or misaligned pointer;
 * KWS_ERR_WORKSPACE for a workspace below kws_dtw_workspace_bytes; KWS_ERR_UNSUPPORTED for more jobs than one launch takes.
 * R == 0 or Q == 0 does nothing and returns KWS_OK. */
int kws_dtw(const float *templates, const int32_t *tmpl_len, int Q, int Lmax, const float *rows, const int32_t *n_frames, int R, int max_frames,
            int D, int metric, int tile_frames, float *cost, int32_t *start, void *ws, size_t ws_bytes, void *stream);

/* The detections in what kws_dtw wrote.  Template q belongs to keyword group[q]; group is (Q) int32 on the DEVICE, group_host is NULL or
 * the same Q values on the host, which are then checked: non-decreasing from 0 without gaps, the last one G - 1.  (The kernel itself
 * takes a keyword's templates wherever they stand.)  Q is at most 1024 here.
 * For each (recording, keyword) the curve is the minimum over the keyword's templates of cost[r, q, :], a tie going to the lower q.
 * Greedy selection, up to K <= KWS_DTW_MAX_HITS times: the unsuppressed frame with the lowest curve value, which must be finite and
 * <= threshold, a tie going to the lower frame; it is emitted as (end frame, start of that template at that frame, cost, template),
 * and every frame f with |f - end| < min_gap is suppressed (min_gap >= 1).
 *   count (R, G) int32; end, hit_start, hit_template (R, G, K) int32, hit_cost (R, G, K) float32, in the order of selection; unused
 *   slots hold -1 / +inf.
 * KWS_ERR_INVALID: R < 0, Q outside 1 .. 1024, max_frames < 1, G outside 1 .. Q, K, min_gap < 1, a NaN threshold, a NULL pointer, a
 * group_host that is not sorted as above.  R == 0 does nothing. */
int kws_dtw_peaks(const float *cost, const int32_t *start, int R, int Q, int max_frames, const int32_t *group, const int32_t *group_host, int G,
                  float threshold, int min_gap, int K, int32_t *count, int32_t *end, int32_t *hit_start, float *hit_cost, int32_t *hit_template,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KWS_H */
