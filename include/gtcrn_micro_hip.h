/*
 * gtcrn_micro_hip.h -- C ABI of the MI355X (gfx950) GTCRN-Micro hot path.
 *
 * The reference (bglid/GTCRN-Micro) has no FFI layer: its seam is the Python
 * class surface.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference repo).  All pointers are plain
 * caller-owned pointers; "d_" = device memory (e.g. torch.Tensor.data_ptr()),
 * "h_" = host memory.  No torch types cross this boundary.
 *
 * Every function returns 0 on success or a negative gtcrn_status; the message
 * is available from gtcrn_last_error() (thread-local).  Launches are
 * asynchronous on the given HIP stream (a hipStream_t passed as void*; NULL =
 * the default stream).  A model handle is bound to one device and is not
 * meant for concurrent calls from several threads (the reference's contract:
 * single-threaded caller, one process per GPU -- train.py:461-471).
 */
#ifndef GTCRN_MICRO_HIP_H
#define GTCRN_MICRO_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTCRN_ABI_VERSION 1
#define GTCRN_NFFT 512
#define GTCRN_HOP 256
#define GTCRN_NBINS 257
#define GTCRN_NPARAM_FLOATS 44938 /* state_dict minus num_batches_tracked */

typedef enum {
    GTCRN_OK = 0,
    GTCRN_ERR_ARG = -1,     /* bad argument (shape, null pointer, T < 1 ...) */
    GTCRN_ERR_HIP = -2,     /* a HIP runtime call failed */
    GTCRN_ERR_DEVICE = -3,  /* no gfx950 device / wrong architecture */
    GTCRN_ERR_STATE = -4    /* handle used before/after its lifetime, workspace too small under capture */
} gtcrn_status;

typedef struct gtcrn_model gtcrn_model;

int gtcrn_abi_version(void);
const char *gtcrn_last_error(void);

/* ---- parameter blob -----------------------------------------------------
 * The flat fp32 blob is the reference state_dict in its own order without the
 * int64 num_batches_tracked entries (ckpt["model"], train.py:200-216;
 * models/gtcrn_micro.py:486-504).  These describe that order so a host can
 * pack by name. */
long gtcrn_param_tensors(void);             /* number of tensors (342) */
const char *gtcrn_param_name(long i);       /* e.g. "encoder.en_convs.0.conv.weight" */
long gtcrn_param_numel(long i);
long gtcrn_param_offset(long i);            /* float offset into the blob */

/* ---- model handle -------------------------------------------------------
 * Replaces: GTCRNMicro(...).to(device) + load_state_dict(ckpt["model"]) + .eval()
 * (infer.py:37-41).  BatchNorm is folded with its running statistics
 * (eval mode).  device = HIP device ordinal. */
int gtcrn_model_create(gtcrn_model **out, const float *h_params, long n_floats, int device);
/* Re-fold after the host changed the weights (load_state_dict on a live module). */
int gtcrn_model_set_params(gtcrn_model *m, const float *h_params, long n_floats);
void gtcrn_model_destroy(gtcrn_model *m);

/* Pre-size the library-owned workspace so that later calls with batch <= B and
 * frames <= T do no allocation (required before HIP-graph capture). */
int gtcrn_model_reserve(gtcrn_model *m, int B, int T);

/* ---- windows ------------------------------------------------------------
 * kind 0: torch.hann_window(512).pow(0.5) (infer.py:65, loss.py:50, tests);
 * kind 1: torch.hann_window(512) (train.py:252).  Host helper; callers may
 * pass any 512-tap window they computed themselves. */
int gtcrn_make_window(int kind, float *h_w512);
long gtcrn_num_frames(long L); /* 1 + L/256 (torch.stft center=True) */

/* ---- STFT / iSTFT (the callers' torch.stft / torch.istft) ---------------
 * Replaces torch.stft(x,512,256,512,win,return_complex=False) (infer.py:60-67,
 * train.py:247-263): d_wave (B,L) -> d_spec.  The spectrogram is addressed as
 *   spec[b,f,t,c] = d_spec[b*sb + f*sf + t*st + c]   (c = 0 re, 1 im)
 * reference layout (B,257,T,2): sb = 257*T*2, sf = T*2, st = 2. */
int gtcrn_stft(const float *d_wave, int B, long L, const float *d_win, float *d_spec,
               long sb, long sf, long st, void *stream);
/* Windowed frames only, (B,T,512): exposes the framing/indexing for the
 * bit-exactness check (reflect pad 256, frame t = xp[256t:256t+512]). */
int gtcrn_stft_frames(const float *d_wave, int B, long L, const float *d_win, float *d_frames, void *stream);
/* Replaces torch.istft(view_as_complex(y),512,256,512,win) (infer.py:73-76):
 * d_spec (strided as above) -> d_wave (B, 256*(T-1)). */
int gtcrn_istft(const float *d_spec, long sb, long sf, long st, int B, int T, const float *d_win,
                float *d_wave, void *stream);

/* ---- offline forward ----------------------------------------------------
 * Replaces GTCRNMicro.forward(spec) in eval mode (models/gtcrn_micro.py:506-532):
 * (B,257,T,2) -> (B,257,T,2), both addressed with the strides given. */
int gtcrn_forward_spec(gtcrn_model *m, const float *d_spec_in, long isb, long isf, long ist,
                       float *d_spec_out, long osb, long osf, long ost, int B, int T, void *stream);
/* Fused caller loop of infer.py:60-76 for B equal-length clips:
 * STFT -> forward -> iSTFT; d_wave (B,L) -> d_wave_out (B, 256*(L/256)). */
int gtcrn_forward_wave(gtcrn_model *m, const float *d_wave, float *d_wave_out, int B, long L,
                       const float *d_win, void *stream);
/* The same loop for B clips of DIFFERENT lengths in one launch sequence (infer.py:48-107 takes the clips of a
 * folder one by one, whatever their lengths): row b of d_wave (B,Lmax) holds d_lengths[b] samples
 * (device int32[B], 257 <= d_lengths[b] <= Lmax); row b of d_wave_out (B, 256*(Lmax/256)) receives its
 * 256*(d_lengths[b]/256) enhanced samples -- bit-identical to gtcrn_forward_wave on that clip alone; the rest
 * of the row is left untouched.  The caller guarantees the bounds (the lengths live in device memory). */
int gtcrn_forward_wave_var(gtcrn_model *m, const float *d_wave, float *d_wave_out, int B, long Lmax,
                           const int *d_lengths, const float *d_win, void *stream);

/* ---- int8-weight / fp16-activation variant (BASELINE configs[4]) ----------------------
 * Replaces the quantised deployment path of the reference: onnx2tf -oiqt -qt per-channel -rtpo PReLU
 * (scripts/onnx2tf.sh:50-64) run by tflite_infer.py:60-107.  The reference ships no quantised model, no
 * calibration data and no TensorFlow, so this variant has its OWN stated contract -- PARITY UNPINNED:
 *   weights      every conv / linear weight of the BatchNorm-folded graph -> symmetric int8 per output channel
 *                (scale = max|w| / 127), consumed as fp16(int8 * scale); biases and PReLU slopes stay fp32
 *   activations  rounded to fp16 (round to nearest even) where a layer produces them; products and sums in fp32
 *                (v_mfma_f32_16x16x16_f16: fp16 operands, fp32 accumulate)
 *   boundary     in_scale / out_scale > 0 add the tflite model's int8 input / output tensors:
 *                x_q = clip(round(x / (scale/255)), -128, 127), x = x_q * scale/255 (tflite_infer.py:79-92 with zero
 *                point 0; the calibration convention x/scale + 0.5 in [0,1] of utils/calibration_data.py:97-106 is
 *                this quantiser, scale = 19.944473 in streaming/tflite/calib_scale.txt).  0 = fp16 boundary.
 *   functions    PReLU(x) = max(x, 0) + a * min(x, 0) (a * x rounded once); magnitude = sqrt(re^2 + im^2 + 1e-12)
 *                (__builtin_amdgcn_sqrtf, 1 ulp); TRA gate sigmoid(z) = __frcp_rn(1 + __expf(-z)); mask
 *                tanh(x) = 1 - 2 * __frcp_rn(__expf(2x) + 1) -- absolute error ~1e-7, i.e. a LARGE relative error of a
 *                small mask value, which the fp16 rounding behind it then shows; each is rounded to fp16 like any
 *                other activation, as an fp32 value (never a fused multiply-add rounded straight to fp16)
 * Same shapes/strides as gtcrn_forward_spec / gtcrn_forward_wave (STFT and iSTFT stay fp32: they are the caller's
 * torch.stft / torch.istft around the tflite interpreter, tflite_infer.py:63-101).  Offline only.
 *
 * Stage taps (gtcrn_debug_tap after a _quant forward that ran with gtcrn_debug_enable(m, 1); without it every tap is
 * refused with GTCRN_ERR_STATE, as the fp32 stage taps do not read fp16 records; tests/test_gpu_quant_stages.py pins a
 * float64 checker of this contract to them, stage by stage).  Every tap comes back as float in the fp32 taps' (C,T,F) layout and holds fp16
 * numbers only:
 *   en0 .. en4   the encoder's hand-off tensors, fp16 records (same element offsets as the fp32 ones, half the bytes),
 *                widened on the host
 *   gtcn1        the first GTCN stack's output, likewise
 *   sum4         what the second stack stores: fp16(gtcn2(x) + en4), the decoder's first input.  "gtcn2" is REFUSED
 *                after a _quant forward (GTCRN_ERR_STATE): the rounded sum cannot be un-added (after an fp32 forward
 *                "gtcn2" is sum4 - en4 as before, and "sum4" the stored sum)
 *   de0 .. de2   the decoder blocks' outputs before the skip sum; de3; de4 = the tanh mask (2,T,129): fp32 copies
 *                written by the stage-tap build of the decoder, whose output is bit-identical to the plain build's
 * The taps follow the variant of the most recent forward. */
int gtcrn_forward_spec_quant(gtcrn_model *m, const float *d_spec_in, long isb, long isf, long ist,
                             float *d_spec_out, long osb, long osf, long ost, int B, int T, float in_scale,
                             float out_scale, void *stream);
int gtcrn_forward_wave_quant(gtcrn_model *m, const float *d_wave, float *d_wave_out, int B, long L,
                             const float *d_win, float in_scale, float out_scale, void *stream);
/* Host views for CPU tests: the packed buffers with quantised weights; float -> binary16 -> float (RNE). */
int gtcrn_pack_params_quant_host(const float *h_params, long n_floats, float *h_f, int *h_i);
float gtcrn_round_to_half(float x);

/* ---- streaming ----------------------------------------------------------
 * Replaces StreamGTCRNMicro.forward(spec, conv_cache, tra_cache, tcn_cache)
 * (gtcrn_micro_stream.py:541-574) for nstreams independent streams.  The
 * per-stream state lives in device memory in the library's ring layout;
 * import/export convert from/to the reference's three caches:
 *   conv_cache (2,N,16,6,33)  tra_cache (2,3,N,8,2)
 *   tcn_cache  2 x 4 tensors (N,16,2d,33), d = 1,2,4,8, passed as 8 pointers
 *   in the order [g0 d1, g0 d2, g0 d4, g0 d8, g1 d1, ...]. */
size_t gtcrn_stream_state_bytes(void); /* per stream */
int gtcrn_stream_reset(gtcrn_model *m, void *d_state, int nstreams, void *stream);
/* nframes >= 1 consecutive frames per call: d_spec_t / d_spec_out_t are
 * (N,257,nframes,2) addressed with the strides given.  nframes == 1 (the
 * reference's loop, :626-635) is ONE kernel launch -- encoder, both GTCN stacks
 * and decoder for four streams per workgroup, nothing handed over through HBM --
 * asynchronous on `stream`, no allocation once gtcrn_model_reserve(N, 1) was
 * called: capturable into a HIP graph.  (With gtcrn_debug_enable the step runs
 * as three launches whose hand-off tensors the stage taps read.)  The state holds
 * a 16-bit frame counter; only its value mod 16 matters, it wraps freely. */
int gtcrn_stream_step(gtcrn_model *m, void *d_state, const float *d_spec_t, long isb, long isf, long ist,
                      float *d_spec_out_t, long osb, long osf, long ost, int nstreams, int nframes,
                      void *stream);
int gtcrn_stream_import(gtcrn_model *m, void *d_state, int nstreams, const float *d_conv_cache,
                        const float *d_tra_cache, const float *const *d_tcn_cache8, void *stream);
int gtcrn_stream_export(gtcrn_model *m, const void *d_state, int nstreams, float *d_conv_cache,
                        float *d_tra_cache, float *const *d_tcn_cache8, void *stream);

/* ---- hop-level waveform streaming --------------------------------------------------------------------------
 * Replaces the caller loop around StreamGTCRNMicro.forward (gtcrn_micro_stream.py:596-646: torch.stft of the whole
 * file, the model frame by frame, torch.istft of the whole result) for a live caller that has 256 samples (one hop,
 * 16 ms at 16 kHz) at a time: nstreams streams, nhops >= 1 hops each per call, 256 * nhops samples in, as many out.
 *
 * Contract.  After a reset, with finite input and a window with win[0] == 0 (every periodic Hann-type window, e.g.
 * torch.hann_window(512).pow(0.5) of infer.py:65 -- pass the same 512 floats the offline call gets), the output
 * stream is gtcrn_forward_wave(x, win) delayed by exactly one hop, bit for bit:
 *     out[n] = 0                                      0 <= n < 256
 *     out[n] = gtcrn_forward_wave(x, win)[n - 256]    n >= 256
 * Call k frames hop k (frame k of torch.stft(center=True) is x[256k-256 : 256k+256]), steps the model on it and emits
 * block k-1: the second half of frame k-1 plus the first half of frame k over the window envelope.  Call 0 emits
 * zeros; its frame 0 is the start-reflected hop 0, whose one future sample x[256] meets win[0] == 0.  A clip of
 * L = 256 K + r >= 257 samples (r = 0..255) ends with ONE flush that takes the r extra samples, builds the last frame
 * end-reflected (torch.stft's reflect padding) and emits 256 samples: the K steps and the flush give 256 (K + 1)
 * samples, the last 256 K of which equal gtcrn_forward_wave.  A flush of a stream that received fewer than 257
 * samples emits zeros.  The flush ends the stream: reset both states before it is used again.
 *
 * State.  d_state is the model state of gtcrn_stream_step (gtcrn_stream_state_bytes per stream, same layout: the
 * reference's caches can be imported / exported around wave steps); d_wstate is the wave state,
 * gtcrn_wave_stream_state_bytes per stream: the last 512 input samples (the end reflection reaches back 257), the
 * overlap-add tail (256) and a hop counter.  Both 16-byte aligned; reset a sub-range of streams by offsetting the
 * pointers.  The counter is per stream: the streams of one call may sit at different hop counts.
 *
 * Calls.  A step or flush is three launches on `stream` (analysis, the model step of gtcrn_stream_step in its form
 * for nframes = nhops, synthesis), asynchronous, and does no allocation once gtcrn_model_reserve(nstreams, nhops) was
 * called: capturable into a HIP graph.  d_in / d_out: row n of stream n at d_in + n * in_stride (256 * nhops samples)
 * and d_out + n * out_stride (256 * nhops samples; the flush: d_tail + n * tail_stride, r samples -> 256 samples;
 * d_tail may be NULL when r == 0).  The _pcm16 forms take and return int16 samples: widened as s / 32768 and
 * stored as clip(rint(y * 32768)), i.e. equal to the float forms between gtcrn_pcm16_to_f32 and gtcrn_f32_to_pcm16.
 * The library cannot read device memory without a synchronisation: win[0] == 0 is the caller's precondition.
 * Null pointers, nstreams < 1, nhops < 1, r outside 0..255 and strides shorter than a row return GTCRN_ERR_ARG before
 * anything is launched. */
size_t gtcrn_wave_stream_state_bytes(void); /* per stream: input ring 512 + OLA tail 256 + hop counter, 16-B aligned */
int gtcrn_wave_stream_reset(gtcrn_model *m, void *d_state, void *d_wstate, int nstreams, void *stream);
int gtcrn_wave_stream_step(gtcrn_model *m, void *d_state, void *d_wstate, const float *d_in, long in_stride,
                           float *d_out, long out_stride, int nstreams, int nhops, const float *d_win, void *stream);
int gtcrn_wave_stream_step_pcm16(gtcrn_model *m, void *d_state, void *d_wstate, const short *d_in, long in_stride,
                                 short *d_out, long out_stride, int nstreams, int nhops, const float *d_win, void *stream);
int gtcrn_wave_stream_flush(gtcrn_model *m, void *d_state, void *d_wstate, const float *d_tail, long tail_stride, int r,
                            float *d_out, long out_stride, int nstreams, const float *d_win, void *stream);
int gtcrn_wave_stream_flush_pcm16(gtcrn_model *m, void *d_state, void *d_wstate, const short *d_tail, long tail_stride,
                                  int r, short *d_out, long out_stride, int nstreams, const float *d_win, void *stream);

/* ---- sample-rate conversion: 8 / 11.025 / 22.05 / 24 / 32 / 44.1 / 48 kHz <-> 16 kHz ---------------------------
 * Replaces `librosa.resample(noisy, orig_sr=sr, target_sr=16000)` in front of the STFT (infer.py:54-57, and the same
 * call on the reference file, infer.py:90-93) and the stateful per-stream resamplers a live caller would otherwise
 * write around gtcrn_wave_stream_step.  The model runs at 16 kHz; these calls are the only way another rate gets in
 * or out.
 *
 * Contract: the filter is this library's own, stated here to the coefficient.  It is NOT librosa's: librosa.resample
 * defaults to soxr_hq, whose filter is not documented to the coefficient, so bit parity with the reference's resampled
 * waveform is neither claimed nor tested; the tests compare with an independent float64 implementation of the
 * definition below (scipy.signal.resample_poly(x, up, down, window=h / up)).
 *   up / down = fs_out / fs_in in lowest terms, q = max(up, down), half = 32 q, 2 half + 1 taps on the fs_in * up grid
 *   h[n] ~ sinc(2 fc n) * kaiser(n; beta),  n = -half .. half,  fc = 0.9375 * 0.5 / q,  beta = 8.95926 (90 dB),
 *          scaled so that sum(h) == up; computed in double on the host, rounded once to float
 *   y[j] = sum over i of x[i] * h[j * down - i * up + half],  0 <= i < L,  0 <= index <= 2 half,
 *          j = 0 .. ceil(L * up / down) - 1; samples outside x are zero (zero padding, centred: no delay)
 * Within +0.0003 / -0.112 dB up to 0.875 of the lower Nyquist frequency, >= 96 dB down from 1.125 x it (whatever
 * aliases lands in 7 - 8 kHz-equivalent only).  Audio above 8 kHz of a wide-band input never reaches the model, and the
 * output at fs is band-limited to 8 kHz unless the caller asks for the band above it to be carried around the model: see
 * "high band" below (the hop-level rate form and the offline composition at 24 / 32 / 48 kHz).  fs_in == fs_out == 16000 is a one-tap copy.  Any other pair of rates is
 * GTCRN_ERR_ARG.  Arithmetic: fp32 fmaf, each output's products in a fixed order into four accumulators, so one signal
 * gives the same bits in a batch of any shape and in the streaming form below.  No designed tap is zero, and the zeros that
 * pad the kernels' phase tables read no sample: a NaN or Inf at x[i0] makes exactly the outputs j with
 * |j * down - i0 * up| <= half non-finite, and every other output keeps its bits.
 *
 * gtcrn_resample_taps (host only, no device): up, down and the 2 half + 1 coefficients exactly as the kernels use
 * them; returns the tap count (h_taps may be NULL to query it; cap = capacity of h_taps in floats).
 * gtcrn_resample_out_len (host only): ceil(L * up / down).
 * gtcrn_resample: B rows; row b holds d_lengths[b] <= L samples (d_lengths: int32 on the device, or NULL = all L) at
 * d_in + b * in_stride and receives ceil(d_lengths[b] * up / down) samples at d_out + b * out_stride; nothing beyond
 * that is written.  Asynchronous on `stream`.  _pcm16_in reads int16 samples (s / 32768), _pcm16_out writes them
 * (clip(rint(y * 32768))): equal to the float form between gtcrn_pcm16_to_f32 / gtcrn_f32_to_pcm16, bit for bit. */
typedef struct gtcrn_resampler gtcrn_resampler;
int gtcrn_resampler_create(gtcrn_resampler **out, int fs_in, int fs_out, int device);   /* designs the taps, uploads them */
void gtcrn_resampler_destroy(gtcrn_resampler *r);
long gtcrn_resample_taps(int fs_in, int fs_out, int *up, int *down, float *h_taps, long cap);
long gtcrn_resample_out_len(int fs_in, int fs_out, long L);
int gtcrn_resample(gtcrn_resampler *r, const float *d_in, long in_stride, const int *d_lengths, long L, float *d_out,
                   long out_stride, int B, void *stream);
int gtcrn_resample_pcm16_in(gtcrn_resampler *r, const short *d_in, long in_stride, const int *d_lengths, long L,
                            float *d_out, long out_stride, int B, void *stream);
int gtcrn_resample_pcm16_out(gtcrn_resampler *r, const float *d_in, long in_stride, const int *d_lengths, long L,
                             short *d_out, long out_stride, int B, void *stream);

/* ---- hop-level streaming at the caller's rate --------------------------------------------------------------------
 * gtcrn_wave_stream_step for a live caller whose audio is not at 16 kHz: fs in {8000, 24000, 32000, 48000} (the rates
 * at which a hop H = 256 fs / 16000 = 128 / 384 / 512 / 768 samples and the stage delay D below are whole numbers;
 * 44.1 kHz and its family have no hop form; 44.1 and 22.05 kHz are live through packets, below).  nhops hops of H samples in per stream and call, as many out.
 *
 * Contract.  `in` is a resampler fs -> 16000, `out` one 16000 -> fs on the model's device.  Each is run in its causal
 * form: the centred filter above delayed by D = 32 q / up_in samples at fs (96 / 48 / 64 / 32 samples at 48 / 24 / 32 /
 * 8 kHz: 2 ms, 4 ms at 8 kHz), with the stream's last samples kept in d_rstate.  With the one-hop delay of the wave step,
 * after a reset, for K hops of input x and u = resample(16000 -> fs) of gtcrn_forward_wave of resample(fs -> 16000) of
 * (D zeros followed by x):
 *     out[n] = 0                  0 <= n < H
 *     out[n] = u[n - H - D]       H + D <= n < H * K          bit for bit
 * (the D samples in between are the interpolator's pre-ringing).  gtcrn_rate_stream_latency = H + 2 D samples at fs:
 * 20 ms, 24 ms at 8 kHz.  There is no rate flush: a caller drains a stream by sending ceil(latency / H) hops of zeros.
 *
 * State.  d_state and d_wstate are those of gtcrn_wave_stream_step, unchanged; d_rstate holds
 * gtcrn_rate_stream_state_bytes(fs) per stream (the two filters' histories as floats).  All 16-byte aligned; reset a
 * sub-range of streams by offsetting the three pointers.  gtcrn_rate_stream_reset resets all three.
 *
 * Calls.  A step is five launches on `stream` (k_rate_in, the three of gtcrn_wave_stream_step, k_rate_out),
 * asynchronous, and allocates nothing once gtcrn_rate_stream_reserve(m, in, out, nstreams, nhops) was called (it sizes
 * the model workspace and the two 16 kHz hand-off buffers, which belong to the model handle): capturable into a HIP
 * graph.  Rows: d_in + n * in_stride and d_out + n * out_stride, H * nhops samples each.  The _pcm16 form takes and
 * returns int16 samples and equals the float form between the two PCM conversions.  Null pointers, counts < 1, short
 * strides, an unsupported rate and a resampler pair that does not match return GTCRN_ERR_ARG before any launch. */
int gtcrn_rate_stream_hop(int fs);              /* H */
int gtcrn_rate_stream_latency(int fs);          /* H + 2 D samples at fs */
size_t gtcrn_rate_stream_state_bytes(int fs);   /* per stream; 0 for an unsupported rate */
int gtcrn_rate_stream_reserve(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, int nstreams, int nhops);
int gtcrn_rate_stream_reset(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state, void *d_wstate,
                            void *d_rstate, int nstreams, void *stream);
int gtcrn_rate_stream_step(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state, void *d_wstate,
                           void *d_rstate, const float *d_in, long in_stride, float *d_out, long out_stride, int nstreams,
                           int nhops, const float *d_win, void *stream);
int gtcrn_rate_stream_step_pcm16(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state, void *d_wstate,
                                 void *d_rstate, const short *d_in, long in_stride, short *d_out, long out_stride,
                                 int nstreams, int nhops, const float *d_win, void *stream);

/* ---- packet-sized live streaming -----------------------------------------------------------------------------------
 * gtcrn_wave_stream_step / gtcrn_rate_stream_step for a live caller whose audio arrives in blocks that are not the model's
 * hop: RTP / WebRTC packets of 10 or 20 ms (160 / 320 samples at 16 kHz, 480 / 960 at 48 kHz), sound-card blocks of 441
 * samples at 44.1 kHz.  For a GROUP of streams every call takes one packet of n samples per stream at fs and returns n
 * enhanced samples per stream, at a constant latency.  The re-blocking to 256-sample hops, both FIFOs and the two
 * resampling stages run on the device (k_packet_in, k_packet_out); the model step in between is gtcrn_wave_stream_step.
 *
 * Geometry (host arithmetic).  fs in {8000, 16000, 22050, 24000, 32000, 44100, 48000} (11025: offline only, its stage
 * delays are not whole samples at 16 kHz).  n16 = n * 16000 / fs must be a whole number in 1..4096, and at fs != 16000 the
 * packet must hold each stage's filter history (ntp_in <= n, ntp_out <= n16; ntp = the taps of the filter's longest phase
 * rounded up to a multiple of 4): 10 ms packets pass at every rate but 22050 (220.5 samples), which takes 20 ms (441).
 * The group has ONE phase phi = (16 kHz samples taken so far) mod 256, kept in the host handle.  A call steps
 * h = (phi + n16) div 256 hops -- the same for every stream, possibly 0 -- then phi <- (phi + n16) mod 256.  With
 * g = gcd(n16, 256) the outbound FIFO starts with 256 - g zeros, the smallest pre-fill that never underflows (its level is
 * 256 - g - phi between calls), so the latency at 16 kHz is L16 = 512 - g samples: 256 at n16 = 256, 480 (30 ms) at 160,
 * 448 (28 ms) at 320.  At fs != 16000 the two causal stages of the rate form add d_in + d_out 16 kHz samples (32 + 32; 64 + 64
 * at 8 kHz).  gtcrn_packet_stream_latency16 returns L16 + d_in + d_out IN 16 kHz SAMPLES: at fs that is
 * latency16 * fs / 16000, a whole number except in the 44.1 kHz family (1499.4 samples for 10 ms packets at 44.1 kHz).
 * A stream that is reset while the group is at phase z joins with z zeros in front of its input (its FIFOs are zeroed and
 * the levels are the group's) and runs in lockstep with the others at the same latency.
 *
 * Contract, bit for bit.  At 16 kHz: for a stream reset at group phase z whose input since then is x, with
 * Y = gtcrn_forward_wave(zeros(z) ++ x, win):
 *     out[k] = 0                    0 <= k < L16 - z
 *     out[k] = Y[k + z - L16]       L16 - z <= k < samples emitted so far
 * (n = 256, z = 0: the calls equal gtcrn_wave_stream_step call by call, outputs and both states.)  At another rate,
 * stage by stage through the public batch calls, with R = gtcrn_resample(fs -> 16000), up / down its ratio,
 * c = ceil(d_in / up) and x the stream's input since its reset:
 *     a16 = R(zeros(c * down) ++ x)[c * up - d_in ...]   -- R(x) delayed by d_in samples; a16[k] == R(x)[k - d_in] for
 *           k >= d_in, and the d_in samples in front are the decimator's pre-ringing, NOT zeros: the stage is the causal
 *           form of k_rate_in (where d_in * fs / 16000 is whole, a16 = R(zeros(D) ++ x) as in the rate form above)
 *     b16 = the 16 kHz contract above applied to a16
 *     out = gtcrn_resample(16000 -> fs)(zeros(d_out) ++ b16), cut to n * calls
 * At 48 kHz with n = 768, z = 0 the calls equal gtcrn_rate_stream_step (960 = H + 2 D).  There is no flush: a caller
 * drains a stream with ceil(latency / packet) packets of zeros.
 *
 * State.  d_state and d_wstate are those of gtcrn_wave_stream_step; d_pstate holds gtcrn_packet_stream_state_bytes(fs, n)
 * per stream: two FIFOs of 256 floats (neither ever holds a whole hop between calls) and the two filter histories.
 * All 16-byte aligned; reset a sub-range of streams by offsetting the three pointers.
 *
 * Calls.  gtcrn_packet_stream_create checks (fs, n) and the resamplers (fs -> 16000 and 16000 -> fs on the model's device;
 * both NULL at 16 kHz), reserves the model workspace for max_streams streams and allocates the hand-off buffers: after it
 * a step allocates nothing.  The handle keeps the model and the resamplers by pointer; destroy it before them.  A step is
 * TWO launches plus those of gtcrn_wave_stream_step for h hops; with h == 0 it is the two alone, no model kernel runs.
 * Asynchronous on `stream`.  Rows: d_in + s * in_stride and d_out + s * out_stride, n samples each.  The _pcm16 form takes
 * and returns int16 samples and equals the float form between the two PCM conversions.  The launch sequence of a call
 * depends only on (n16, phi) and the step advances phi on the HOST, so phi returns to its start after 256 / g calls: a
 * caller who wants a HIP graph captures ONE WHOLE PERIOD of 256 / g steps (each with its own packet buffers) and replays
 * it; streams then join (gtcrn_packet_stream_reset) between replays.  gtcrn_packet_stream_schedule (host only) returns h
 * for a phase and the phase after it; _phase and _next_hops read the handle.  A call's cost varies with h (n16 = 160:
 * 0,1,0,1,1,0,1,1 over a period); a server evens it out with two groups created at different points of their periods.
 * Null pointers, counts < 1 or above max_streams, short strides and an unsupported (fs, n) or resampler pair return
 * GTCRN_ERR_ARG before any launch. */
typedef struct gtcrn_packet_stream gtcrn_packet_stream;
int gtcrn_packet_stream_n16(int fs, int n);             /* n * 16000 / fs, or GTCRN_ERR_ARG */
int gtcrn_packet_stream_latency16(int fs, int n);       /* 512 - g + d_in + d_out, in 16 kHz samples */
size_t gtcrn_packet_stream_state_bytes(int fs, int n);  /* per stream; 0 for an unsupported (fs, n) */
int gtcrn_packet_stream_schedule(int fs, int n, int phase, int *next_phase);   /* h of a call at `phase` */
int gtcrn_packet_stream_create(gtcrn_packet_stream **out, gtcrn_model *m, gtcrn_resampler *rs_in, gtcrn_resampler *rs_out,
                               int fs, int n, int max_streams);
void gtcrn_packet_stream_destroy(gtcrn_packet_stream *ps);
int gtcrn_packet_stream_phase(const gtcrn_packet_stream *ps);
int gtcrn_packet_stream_next_hops(const gtcrn_packet_stream *ps);
int gtcrn_packet_stream_reset(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate, int nstreams,
                              void *stream);
int gtcrn_packet_stream_step(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate, const float *d_in,
                             long in_stride, float *d_out, long out_stride, int nstreams, const float *d_win, void *stream);
int gtcrn_packet_stream_step_pcm16(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate,
                                   const short *d_in, long in_stride, short *d_out, long out_stride, int nstreams,
                                   const float *d_win, void *stream);

/* ---- attenuation limit: a per-stream dry / wet mix on every waveform path ------------------------------------------
 * The "suppression level" / "attenuation limit" / "dry-wet" control of a deployed enhancer: an operator caps the noise
 * reduction at limit_dB, a client switches the enhancer off for an A/B comparison without changing the call's latency.
 * The library holds the dry signal where the output is written, so the control costs no launch, no delay line and, in the
 * PCM16 forms, no second rounding.
 *
 * Contract.  A DRY GAIN beta in [0, 1] per stream or clip, beta = 10^(-limit_dB / 20): beta = 0 is no limit (the plain
 * call's output), beta = 1 is bypass (the input comes out at the form's latency).  The calls take beta itself: d_gain, a
 * device array of floats, one per stream / row.  d_gain == NULL means no limit and runs the plain call's kernels.  With w
 * the sample the plain call emits and x the input sample aligned with it,
 *     y = fl( fl(beta * x) + fl( fl(1 - beta) * w ) )        every fl() ONE fp32 rounding, no fused multiply-add
 * so a numpy float32 expression reproduces y bit for bit.  Hence beta = 0 gives w and beta = 1 gives x, exactly, for finite
 * inputs (as values: a zero may change its sign).  Bypass is bit for bit the input for finite wet samples only: at beta = 1
 * y = x + 0 * w, so a bypassed stream repeats a non-finite model output ("non-finite input" below) instead of the input.
 * The mix is made in float BEFORE the one rounding to int16 of the _pcm16
 * forms.  Samples a form emits as structural zeros stay zeros: the first block of a hop stream, the FIFO pre-fill of the
 * packet form, the flush of a stream that holds fewer than 257 samples.  The limit changes no state: model state and wave
 * state after a limited call equal those after the plain call, and no state layout or *_state_bytes differs.
 *
 * Alignment (it follows from the contracts above).
 *   offline   gtcrn_forward_wave_limited: x = d_wave[b][n] for n < 256 * (L / 256); with d_lengths, n < 256 * (len_b / 256)
 *             per row and nothing beyond is written, as in gtcrn_forward_wave_var.  d_lengths == NULL: all rows hold Lmax.
 *   hop form  the block emitted for hop k is block k - 1, its dry samples are input hop k - 1: the ring's newest 256
 *             samples for the first hop of a call (and for the flush's block), hop h - 1 of the call's input rows for
 *             the later hops.  The stream equals gtcrn_forward_wave_limited one hop late, bit for bit.
 *   rate and packet forms: the mix is made at 16 kHz inside the wave step they run.  Their stage-by-stage contracts hold
 *             word for word with gtcrn_forward_wave replaced by gtcrn_forward_wave_limited (on a16, the 16 kHz hand-off);
 *             the dry signal passes the same outbound stage as the wet one, band-limited and delayed identically.
 *
 * d_gain is read from device memory by the kernel at every call: a caller may rewrite it between calls, also between the
 * replays of a captured HIP graph, and the change takes effect at the next emitted block.  The library cannot read device
 * memory without a synchronisation: 0 <= beta <= 1 is the caller's precondition (as win[0] == 0 is).  A limited call makes
 * the launches of its plain form, one for one (the mixing kernels are timed as k_wave_synthesis_mix / k_istft_mix), and
 * checks its arguments as the plain form does.  gtcrn_packet_stream_set_dry_gain stores the pointer in the handle (it must
 * cover max_streams floats and stay valid; NULL switches the limit off), so the packet steps keep their signatures and a
 * captured period keeps replaying while gains change.
 * A change of beta lands as a step at a block boundary unless the caller asks for a ramp: "gain ramps" below.
 * Out of scope: the _quant entry points; the spectrogram-level calls (a caller holding spectra mixes them itself: by linearity
 * beta * X + (1 - beta) * forward_spec(X) is this control up to the rounding of an STFT -> iSTFT round trip). */
int gtcrn_forward_wave_limited(gtcrn_model *m, const float *d_wave, float *d_wave_out, int B, long Lmax,
                               const int *d_lengths, const float *d_gain, const float *d_win, void *stream);
int gtcrn_wave_stream_step_limited(gtcrn_model *m, void *d_state, void *d_wstate, const float *d_in, long in_stride,
                                   float *d_out, long out_stride, int nstreams, int nhops, const float *d_gain,
                                   const float *d_win, void *stream);
int gtcrn_wave_stream_step_limited_pcm16(gtcrn_model *m, void *d_state, void *d_wstate, const short *d_in, long in_stride,
                                         short *d_out, long out_stride, int nstreams, int nhops, const float *d_gain,
                                         const float *d_win, void *stream);
int gtcrn_wave_stream_flush_limited(gtcrn_model *m, void *d_state, void *d_wstate, const float *d_tail, long tail_stride,
                                    int r, float *d_out, long out_stride, int nstreams, const float *d_gain,
                                    const float *d_win, void *stream);
int gtcrn_wave_stream_flush_limited_pcm16(gtcrn_model *m, void *d_state, void *d_wstate, const short *d_tail,
                                          long tail_stride, int r, short *d_out, long out_stride, int nstreams,
                                          const float *d_gain, const float *d_win, void *stream);
int gtcrn_rate_stream_step_limited(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state, void *d_wstate,
                                   void *d_rstate, const float *d_in, long in_stride, float *d_out, long out_stride,
                                   int nstreams, int nhops, const float *d_gain, const float *d_win, void *stream);
int gtcrn_rate_stream_step_limited_pcm16(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state,
                                         void *d_wstate, void *d_rstate, const short *d_in, long in_stride, short *d_out,
                                         long out_stride, int nstreams, int nhops, const float *d_gain, const float *d_win,
                                         void *stream);
int gtcrn_packet_stream_set_dry_gain(gtcrn_packet_stream *ps, const float *d_gain);

/* ---- high band: the band above 8 kHz of a 24 / 32 / 48 kHz stream, carried around the model ---------------------------
 * The model runs at 16 kHz, so the plain rate form returns a stream at fs with nothing above 8 kHz (>= 96 dB down), and
 * its attenuation limit at 0 dB is a low-pass filter, not a bypass.  Deployed enhancers that run a 16 kHz model inside a
 * wide-band call split the band: the model cleans the low band, the high band goes around it, delayed to match, with a
 * gain the application controls.  The library holds the 16 kHz dry signal and the outbound stage where the output is
 * written, so the control costs no launch and no pass over the audio by the caller.
 *
 * Contract.  A HIGH-BAND GAIN gamma in [0, 1] per stream: d_hb_gain, a device array of floats, read by the kernel at
 * every call like d_gain (it may be rewritten between calls and between the replays of a captured graph; 0 <= gamma <= 1 is
 * the caller's precondition).  fs in {24000, 32000, 48000}.  The wave step is called as it is: `w` below is whatever it
 * emits, limited (d_gain) or not (d_gain == NULL), and the meters see what they saw.
 *   Live form.  For one stream after a reset, with x[n] the input at fs (PCM16: s / 32768), x[n < 0] = 0; a[k] the 16 kHz
 *   hand-off of the inbound stage, a[k < 0] = 0; w[k] what the wave step emits for it (one hop late); H and D as in the
 *   rate form and LAT = H + 2 D = gtcrn_rate_stream_latency(fs):
 *       s[k]   = fl( w[k] - fl(gamma * a[k - 256]) )        fp32, every fl() ONE rounding, no fused multiply-add
 *       v      = the causal outbound stage applied to s      (what gtcrn_rate_stream_step would emit if handed s for w)
 *       out[n] = fl( v[n] + fl(gamma * x[n - LAT]) )         then the form's one rounding to int16 (_pcm16)
 *   Both stages are linear phase with whole delays that sum to LAT, so the stage applied to -gamma a removes from
 *   gamma x[n - LAT] exactly the band the model path carries: in exact arithmetic out = R(w) + gamma highpass(x delayed by
 *   LAT), R the outbound stage.  Hence
 *     - gamma = 0 equals the plain / limited step in value (the products are +-0: a zero may change its sign), outputs and
 *       the model, wave and rate states;
 *     - with the attenuation limit at 0 dB (beta = 1: w[k] == a[k - 256] exactly) and gamma = 1: s == 0, v == 0 and
 *       out[n] == x[n - LAT] bit for bit, float and PCM16: the true bypass at the caller's rate;
 *     - the output and all four states do not depend on how the hops are cut into calls.
 *   Offline form.  With x16 = gtcrn_resample(fs -> 16000)(x), y = gtcrn_forward_wave[_limited](x16) and no delay anywhere,
 *       out[j] = fl( gtcrn_resample(16000 -> fs)( fl(y - fl(gamma * x16)) )[j] + fl(gamma * x[j]) )     j < min(Lx, outputs)
 *   and outputs at j >= Lx (a length-rounding tail, if any) get no dry term.  gtcrn_resample_hb is that last step: row b
 *   holds d_lengths[b] <= L samples of d_wet (y) and d_dry (x16), d_xlengths[b] <= Lx samples of d_x (either array NULL: all
 *   rows full) and receives ceil(d_lengths[b] * up / down) samples; `r` is a resampler 16000 -> fs.  One launch, asynchronous;
 *   null pointers, B, L or Lx < 1, short strides, another resampler and d_x rows that overlap the output rows return
 *   GTCRN_ERR_ARG before it.
 *
 * State.  d_hbstate holds gtcrn_rate_stream_hb_state_bytes(fs) = 4 * (256 + LAT) bytes per stream: the last 256 samples of
 * a and the last LAT input samples as floats (the outbound history in d_rstate then holds s).  16-byte aligned; zeroed by
 * gtcrn_rate_stream_hb_reset, a sub-range by offsetting the pointer.  It is a buffer of its own: d_rstate and
 * gtcrn_rate_stream_state_bytes, every other state and GTCRN_ABI_VERSION are what they were.
 *
 * Calls.  gtcrn_rate_stream_step_hb[_pcm16] take the arguments of the _limited calls (d_gain may be NULL: no limit) plus
 * d_hbstate and d_hb_gain.  A step is still five launches (k_rate_out_hb in the place of k_rate_out), asynchronous,
 * allocates nothing after gtcrn_rate_stream_reserve and is capturable.  The kernel reads x[n - LAT] from the call's input
 * rows while other threads write the output rows, so a call is NOT legal in place: input and output rows that overlap
 * return GTCRN_ERR_ARG, as do fs = 8000 or 16000 (no high band), the 44.1 kHz family, a NULL d_hbstate or d_hb_gain and
 * everything the plain step refuses, all before any launch.
 * Out of scope: the folder driver (the packet forms carry the high band through "high band on the packet forms" below); a gain the library derives from the mask or the meters (a caller computes one on the device from the
 * meter records without a synchronisation); ramping gamma inside a block. */
size_t gtcrn_rate_stream_hb_state_bytes(int fs);   /* per stream; 0 (and GTCRN_ERR_ARG recorded) without a high band */
int gtcrn_rate_stream_hb_reset(int fs, void *d_hbstate, int nstreams, void *stream);
int gtcrn_rate_stream_step_hb(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state, void *d_wstate,
                              void *d_rstate, const float *d_in, long in_stride, float *d_out, long out_stride, int nstreams,
                              int nhops, const float *d_gain, const float *d_win, void *d_hbstate, const float *d_hb_gain,
                              void *stream);
int gtcrn_rate_stream_step_hb_pcm16(gtcrn_model *m, gtcrn_resampler *in, gtcrn_resampler *out, void *d_state, void *d_wstate,
                                    void *d_rstate, const short *d_in, long in_stride, short *d_out, long out_stride,
                                    int nstreams, int nhops, const float *d_gain, const float *d_win, void *d_hbstate,
                                    const float *d_hb_gain, void *stream);
int gtcrn_resample_hb(gtcrn_resampler *r, const float *d_wet, long wet_stride, const float *d_dry, long dry_stride,
                      const int *d_lengths, long L, const float *d_x, long x_stride, const int *d_xlengths, long Lx,
                      const float *d_hb_gain, float *d_out, long out_stride, int B, void *stream);

/* ---- stream slots: step any subset of the resident live streams per call -----------------------------------------------
 * The contiguous live calls step every stream of a state range.  In a server some streams have no packet this tick and
 * streams join and leave all the time; the _slots calls leave every state where it is and take, per call, a device array
 * naming the slots that step and a device word saying how many:
 *   d_slots     int32[max_active] on the device: row i of the call is the stream whose model state sits at
 *               d_state + d_slots[i] * gtcrn_stream_state_bytes() and whose wave state at
 *               d_wstate + d_slots[i] * gtcrn_wave_stream_state_bytes();
 *   d_count     one int32 on the device, clamped on the device to 0 .. max_active: rows at or beyond it are neither read
 *               nor written (their slots, input and output rows alike).  NULL: max_active rows step;
 *   max_active  >= 1: the host sizes the grid, the workspace (gtcrn_model_reserve(m, max_active, 1)) and the kernel form
 *               from it alone, so ONE captured graph serves a changing active set: rewrite d_slots, d_count and the input
 *               rows between replays.
 * Sample and spectrum rows are COMPACT: row i of d_in / d_out / d_spec_t belongs to slot d_slots[i].  d_gain (may be NULL:
 * no limit) is indexed BY SLOT, d_gain[d_slots[i]]: gains belong to the stream, not to the call.
 * Contract:
 *   - per slot, the sequence of calls that name it IS the contiguous stream of the same inputs: the outputs are those of
 *     gtcrn_wave_stream_step (gtcrn_stream_step) on a state holding that one stream, bit for bit, i.e.
 *     gtcrn_forward_wave (gtcrn_forward_wave_limited with a gain) one hop late;
 *   - a slot not named in a call is not touched, byte for byte;
 *   - the ids are in range and distinct within a call: the caller's precondition, as win[0] == 0 is (the library cannot
 *     read device memory without a synchronisation).  A repeated id gives undefined results for that slot, an id out of
 *     range is a memory error.  Sorted ids are recommended for locality and are not required.
 * gtcrn_stream_reset_slots zeroes the model state and, when d_wstate is given, the wave state of the listed slots with a
 * kernel (gtcrn_stream_reset / gtcrn_wave_stream_reset use a memset on a contiguous range), so a captured graph can admit
 * a stream at any slot.  The flush emits the named streams' last 256 samples (r = 0..255 tail samples per row) and leaves
 * their states as they are: reset a slot before it is reused.
 * All calls are asynchronous on `stream`, allocate nothing once gtcrn_model_reserve(m, max_active, 1) was called, and can
 * be captured.  One hop (frame) per call: this is the live tick.  Only the single-launch forms exist indexed: after
 * gtcrn_stream_form(m, 1), or with gtcrn_debug_enable(m, 1), the step calls return GTCRN_ERR_STATE.  Argument errors
 * (null pointers, max_active < 1, short strides, misaligned states, r outside 0..255) return GTCRN_ERR_ARG before any
 * launch.  Out of scope: the rate form (its streams step whole hops at the caller's rate; for packets see "packet stream
 * slots" below), several hops per call. */
int gtcrn_stream_step_slots(gtcrn_model *m, void *d_state, const int *d_slots, const int *d_count, int max_active,
                            const float *d_spec_t, long isb, long isf, long ist, float *d_spec_out_t, long osb, long osf,
                            long ost, void *stream);   /* one frame per row: (max_active,257,1,2) by strides */
int gtcrn_stream_reset_slots(gtcrn_model *m, void *d_state, void *d_wstate /* may be NULL */, const int *d_slots,
                             const int *d_count, int max_active, void *stream);
int gtcrn_wave_stream_step_slots(gtcrn_model *m, void *d_state, void *d_wstate, const int *d_slots, const int *d_count,
                                 int max_active, const float *d_in, long in_stride, float *d_out, long out_stride,
                                 const float *d_gain /* per SLOT, may be NULL */, const float *d_win, void *stream);
int gtcrn_wave_stream_step_slots_pcm16(gtcrn_model *m, void *d_state, void *d_wstate, const int *d_slots,
                                       const int *d_count, int max_active, const short *d_in, long in_stride, short *d_out,
                                       long out_stride, const float *d_gain, const float *d_win, void *stream);
int gtcrn_wave_stream_flush_slots(gtcrn_model *m, void *d_state, void *d_wstate, const int *d_slots, const int *d_count,
                                  int max_active, const float *d_tail, long tail_stride, int r, float *d_out,
                                  long out_stride, const float *d_gain, const float *d_win, void *stream);
int gtcrn_wave_stream_flush_slots_pcm16(gtcrn_model *m, void *d_state, void *d_wstate, const int *d_slots,
                                        const int *d_count, int max_active, const short *d_tail, long tail_stride, int r,
                                        short *d_out, long out_stride, const float *d_gain, const float *d_win,
                                        void *stream);

/* ---- packet stream slots: per-stream phase, any subset of the resident packet streams per call -------------------------
 * The packet form above keeps ONE phase per group in the host handle, so every stream of the group needs a packet at every
 * call.  These calls keep the phase on the device, one word per resident slot, and take the slot table of "stream slots":
 *   d_phase     int32[resident slots], owned by the caller like the three states: slot s holds phi_s in [0, 256), a
 *               multiple of g = gcd(n16, 256).  d_state / d_wstate / d_pstate keep their layouts and sizes;
 *   d_slots, d_count, max_active   as in the _slots calls above (count clamped on the device to 0 .. max_active, rows at
 *               or beyond it neither read nor written, ids in range and distinct by the caller's precondition);
 *               max_active <= the handle's max_streams.  How many slots are resident is the caller's own affair.
 * Rows are COMPACT: row i of d_in / d_out is one packet of n samples for slot d_slots[i].  The dry gains are the pointer of
 * gtcrn_packet_stream_set_dry_gain, read BY SLOT: gain[d_slots[i]].
 * Contract:
 *   - per slot, bit for bit: take the calls that name a slot after its reset; its outputs and its model, wave and packet
 *     state are those of gtcrn_packet_stream_step(_pcm16) on a one-stream group created at phase 0 and fed the same
 *     packets.  At 16 kHz: out = zeros(L16) ++ gtcrn_forward_wave(x), L16 = 512 - g; at other rates the stage-by-stage
 *     contract of the packet form with z = 0.  The latency is the same constant for every stream, whenever it joined;
 *   - a slot not named in a call is not touched, byte for byte, in all four arrays;
 *   - gtcrn_packet_stream_reset_slots is a kernel (no memset): it zeroes the named slots' model, wave and packet state
 *     and their phase word, so a captured graph can admit a stream at any slot;
 *   - there is no flush: drain with packets of zeros, as in the packet form.
 * A call makes a FIXED launch sequence that depends on (fs, n, max_active) alone, hmax = (256 - g + n16) div 256:
 * plan (reads and advances the phases, writes per round the table of slots that still have a hop ready, in row order) ->
 * inbound -> hmax rounds of the single-launch indexed wave step, one hop each -> outbound.  So ONE captured call serves
 * every tick and every active set, and a 20 ms call runs single-launch one-frame steps.  It allocates nothing after
 * gtcrn_packet_stream_create and neither reads nor advances the handle's host phase (gtcrn_packet_stream_phase).
 * Mixing gtcrn_packet_stream_step and the _slots calls on the same states is not supported.  Only the single-launch stream
 * forms exist indexed: after gtcrn_stream_form(m, 1), or with gtcrn_debug_enable(m, 1), the calls return GTCRN_ERR_STATE.
 * Argument errors (null pointers, max_active < 1 or above the handle's max_streams, short strides, misaligned states)
 * return GTCRN_ERR_ARG before any launch.  Out of scope: _slots for gtcrn_rate_stream_* (48 kHz / 768-sample packets ARE
 * that form), the _quant paths, gtcrn_packet_stream_debug_handoff after a slot call. */
int gtcrn_packet_stream_reset_slots(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate, int *d_phase,
                                    const int *d_slots, const int *d_count, int max_active, void *stream);
int gtcrn_packet_stream_step_slots(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate, int *d_phase,
                                   const int *d_slots, const int *d_count, int max_active, const float *d_in,
                                   long in_stride, float *d_out, long out_stride, const float *d_win, void *stream);
int gtcrn_packet_stream_step_slots_pcm16(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate,
                                         int *d_phase, const int *d_slots, const int *d_count, int max_active,
                                         const short *d_in, long in_stride, short *d_out, long out_stride,
                                         const float *d_win, void *stream);

/* ---- high band on the packet forms: 24 / 32 / 48 kHz packets, group and slots ----------------------------------------------
 * "high band" above, for the caller whose audio arrives in 10 or 20 ms packets (gtcrn_packet_stream_step, the packet slots):
 * the 16 kHz samples the inbound kernel produced, the outbound FIFO, the outbound stage and the call's input rows are all on
 * the device where the output is written, so the band above 8 kHz costs no launch and no extra pass over the audio, only one
 * more per-stream state buffer.
 *
 * Contract (every fl() ONE fp32 rounding, no fused multiply-add).  Per stream, counted from the stream's own reset: x[n] the
 * input at fs (PCM16: s / 32768); A[t] the 16 kHz output of the packet form's causal inbound stage (what the inbound kernel
 * appends to the inbound FIFO); P[t] the 16 kHz sequence the outbound FIFO pops (its pre-fill, then what the wave step
 * emitted); negative indices are zero.  g = gcd(n16, 256), L16 = 512 - g, LAT16 = L16 + d_in + d_out =
 * gtcrn_packet_stream_latency16(fs, n), LAT = LAT16 * fs / 16000 = gtcrn_packet_stream_hb_latency(fs, n), and gamma the
 * stream's HIGH-BAND GAIN in [0, 1] (the caller's precondition, read from device memory at every call):
 *     s[t]   = fl( P[t] - fl(gamma * A[t - L16]) )
 *     v      = the packet form's causal outbound stage applied to s (in the place of P)
 *     out[n] = fl( v[n] + fl(gamma * x[n - LAT]) )          then the form's one rounding to int16 (_pcm16)
 * L16 holds whatever the join phase: a stream that joins a group at phase z has z zeros in front of A in the inbound FIFO and
 * 256 - g - z zeros of outbound pre-fill, and the wave step is one hop late, so P[t] pairs with
 * A[t - (256 - g - z) - 256 - z + z] = A[t - L16]; the slot form has z = 0.  Both stages are linear phase with whole delays
 * (d_in = d_out = 32 16 kHz samples at the three rates), so the low band of x arrives at the output delayed by exactly LAT and
 * the stage applied to -gamma A removes it from gamma x[n - LAT]: LAT = 1632 / 1536 / 960 samples for 480 / 960 / 768-sample
 * packets at 48 kHz, 1088 for 320 at 32 kHz, 816 / 768 for 240 / 480 at 24 kHz.  Hence, bit for bit:
 *   - with the attenuation limit at 0 dB (beta = 1: the wave step emits the dry block) and gamma = 1: s == 0, v == 0 and
 *     out[n] == x[n - LAT], float and PCM16: the true bypass at the caller's rate and packet size;
 *   - gamma = 0 equals the plain / limited packet call in value (the products are +-0), outputs and the model, wave and packet
 *     states;
 *   - at 48 kHz with n = 768 a group created at phase 0 equals gtcrn_rate_stream_step_hb call by call (L16 = 256, LAT = 960);
 *   - the limit (gtcrn_packet_stream_set_dry_gain) and the level meters compose with nothing added: the wave step is called
 *     exactly as it is and P is whatever it emitted;
 *   - per slot, the slot form equals a one-stream group created at phase 0 and fed the same packets.
 *
 * Rates and packets.  fs in {24000, 32000, 48000} and LAT16 * fs / 16000 whole: always at 32 and 48 kHz, at 24 kHz for an even
 * n16 (10 and 20 ms packets are).  8 / 16 kHz (no high band), 22.05 / 44.1 kHz (1499.4 samples) and an odd n16 at 24 kHz:
 * gtcrn_packet_stream_hb_latency returns GTCRN_ERR_ARG, gtcrn_packet_stream_hb_state_bytes 0 with the error recorded, and
 * the steps GTCRN_ERR_ARG before any launch.
 *
 * State.  d_hbstate, a buffer of its own: gtcrn_packet_stream_hb_state_bytes(fs, n) per stream = L16 floats (the last L16
 * samples of A) ++ LAT floats (the last LAT input samples), the row rounded up to a multiple of 4 floats (8 448 bytes at
 * 48 kHz / 480).  16-byte aligned, zeros after a reset; the outbound history in d_pstate then holds s.  d_pstate,
 * gtcrn_packet_stream_state_bytes, every other state and GTCRN_ABI_VERSION are what they were.  gtcrn_packet_stream_hb_reset
 * zeroes nstreams rows (a sub-range by offsetting the pointer) next to gtcrn_packet_stream_reset;
 * gtcrn_packet_stream_hb_reset_slots is a kernel, next to gtcrn_packet_stream_reset_slots, so a captured graph can admit a
 * stream.
 *
 * Calls.  The plain signatures plus d_hbstate and d_hb_gain; d_hb_gain is read by ROW in the group form and BY SLOT in the
 * slot form (like the dry gains), at every call, so it may change between calls and between graph replays.  A call makes the
 * launch sequence of its plain form one for one, k_packet_out_hb / k_packet_out_slots_hb in the place of the outbound kernel
 * (timed in that kernel's row of the launch records), the two launches of an h = 0 call included; it allocates nothing after
 * gtcrn_packet_stream_create and captures as the plain form does (one period for the group form, one call for the slot
 * form).  The kernel reads x[n - LAT] from the call's input rows while other threads write the output rows: rows that overlap
 * return GTCRN_ERR_ARG, as do a NULL or misaligned d_hbstate, a NULL d_hb_gain, an unsupported (fs, n) and everything the
 * plain call refuses, all before any launch.
 * Out of scope: G.711 (an 8 kHz payload: no high band); 44.1 / 22.05 kHz; the folder driver; a gain the library derives;
 * ramping gamma inside a packet. */
int gtcrn_packet_stream_hb_latency(int fs, int n);          /* LAT in samples at fs, or GTCRN_ERR_ARG */
size_t gtcrn_packet_stream_hb_state_bytes(int fs, int n);   /* per stream; 0 (and GTCRN_ERR_ARG recorded) without a high band */
int gtcrn_packet_stream_hb_reset(gtcrn_packet_stream *ps, void *d_hbstate, int nstreams, void *stream);
int gtcrn_packet_stream_hb_reset_slots(gtcrn_packet_stream *ps, void *d_hbstate, const int *d_slots, const int *d_count,
                                       int max_active, void *stream);
int gtcrn_packet_stream_step_hb(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate, const float *d_in,
                                long in_stride, float *d_out, long out_stride, int nstreams, const float *d_win,
                                void *d_hbstate, const float *d_hb_gain, void *stream);
int gtcrn_packet_stream_step_hb_pcm16(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate,
                                      const short *d_in, long in_stride, short *d_out, long out_stride, int nstreams,
                                      const float *d_win, void *d_hbstate, const float *d_hb_gain, void *stream);
int gtcrn_packet_stream_step_slots_hb(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate, int *d_phase,
                                      const int *d_slots, const int *d_count, int max_active, const float *d_in,
                                      long in_stride, float *d_out, long out_stride, const float *d_win, void *d_hbstate,
                                      const float *d_hb_gain, void *stream);
int gtcrn_packet_stream_step_slots_hb_pcm16(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate,
                                            int *d_phase, const int *d_slots, const int *d_count, int max_active,
                                            const short *d_in, long in_stride, short *d_out, long out_stride,
                                            const float *d_win, void *d_hbstate, const float *d_hb_gain, void *stream);

/* ---- G.711 payloads (mu-law / A-law) on the packet form, the packet slots and a pair of bulk converters ----------------
 * Most 8 kHz RTP carries G.711: payload type 0 (PCMU) and 8 (PCMA), one byte a sample, 160 bytes per 20 ms packet.  The
 * packet kernels read and write their samples through one load / store function per sample type, so the companding sits
 * exactly where the packet is read and written: no launch, no extra pass, a quarter of the float bytes over the host link,
 * and no rounding beyond the ONE the PCM16 form already makes.
 *
 * Two laws: law = 0 mu-law, law = 1 A-law.  Everything is defined on the 16-bit linear scale of the _pcm16 forms.
 *
 * Decode.  A byte c is the integer D_law[c], the sample D_law[c] / 32768 exactly (ITU-T G.711's tables):
 *   mu-law:  u = ~c & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 132) << e) - 132; -mag if u & 0x80, else +mag.
 *            Range +-32124; 255 distinct values: 0xFF and 0x7F both decode to 0.
 *   A-law:   a = c ^ 0x55, m = a & 15, s = (a >> 4) & 7, t = (m << 4) + 8 if s == 0, else ((m << 4) + 264) << (s - 1);
 *            +t if a & 0x80, else -t.  Range +-32256; 256 distinct values, no zero.
 * Encode.  A float y becomes p = clip(rint(y * 32768), -32768, 32767) -- exactly the _pcm16 rounding, half to even -- and
 * then the byte E_law(p), an integer map:
 *   mu-law (sign-magnitude):  s = 0x80 if p < 0, else 0; a = min(|p|, 32635) + 132; e = floor(log2 a) - 7 (0..7);
 *            m = (a >> (e + 3)) & 15; byte = ~(s | e << 4 | m) & 0xFF.  There is no "zero trap".
 *   A-law (ones-complement magnitude):  g = p if p >= 0, else ~p; q = g >> 3 (0..4095); s = 0 if q < 32, else
 *            floor(log2 q) - 4 (1..7); m = (q >> 1) & 15 if s < 2, else (q >> s) & 15;
 *            byte = ((p >= 0 ? 0x80 : 0) | s << 4 | m) ^ 0x55.
 * Both encoders are monotone in p, and E(D[c]) == c for every code except mu-law 0x7F (negative zero re-encodes as 0xFF).
 * The A-law encoder equals Python's audioop.lin2alaw on all 65 536 inputs.  The mu-law encoder differs from
 * audioop.lin2ulaw on 381 negative inputs: audioop floors p >> 2 BEFORE it takes the magnitude, this one is symmetric
 * (E(-p) == E(p) ^ 0x80 for p != 0).  That is by design.
 *
 * Contract, by construction and bit for bit: a _g711 call equals the _pcm16 call followed by E_law on its output, and
 * input bytes c equal the float call's input D_law[c] / 32768; the model, wave and packet states after it are the float
 * call's.  Samples a form emits as structural zeros leave as 0xFF (mu) / 0xD5 (A): the first block, the FIFO pre-fill and a limited
 * stream's zeros.  The handle's dry gains (gtcrn_packet_stream_set_dry_gain) and the model's level meters apply unchanged:
 * the mix and the meter values are taken in float at 16 kHz, before the encode.
 *
 * gtcrn_packet_stream_step_g711 / _step_slots_g711: the _pcm16 signatures with byte rows and `law`, the same law in and
 * out, strides in samples (= bytes).  They make the launches of their plain forms one for one under the same timing rows,
 * capture as they do (the contiguous form one period, the slot form one call), and make the same argument checks before any
 * launch, plus law outside {0, 1} -> GTCRN_ERR_ARG.  No state layout, no *_state_bytes and no ABI version changes.
 *
 * gtcrn_g711_to_f32 / gtcrn_f32_to_g711, for the offline and hop-form caller: device pointers, both 16-byte aligned, n a
 * multiple of 16, asynchronous on `stream`.  gtcrn_g711_decode_table (h_table[c] = D_law[c]) and gtcrn_g711_encode_pcm16
 * (returns E_law(p); p outside -32768 .. 32767 -> GTCRN_ERR_ARG) are host only and touch no device: they run the very
 * functions the kernels compile.
 *
 * Out of scope: different laws in and out; G.711 on the hop and rate forms and on the offline calls (the bulk converters
 * serve those); G.711 WAV files in the folder driver; Appendix I / II (packet-loss concealment, comfort noise); the _quant
 * paths. */
int gtcrn_packet_stream_step_g711(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate,
                                  const unsigned char *d_in, long in_stride, unsigned char *d_out, long out_stride,
                                  int nstreams, int law, const float *d_win, void *stream);
int gtcrn_packet_stream_step_slots_g711(gtcrn_packet_stream *ps, void *d_state, void *d_wstate, void *d_pstate,
                                        int *d_phase, const int *d_slots, const int *d_count, int max_active,
                                        const unsigned char *d_in, long in_stride, unsigned char *d_out, long out_stride,
                                        int law, const float *d_win, void *stream);
int gtcrn_g711_to_f32(int device, int law, const unsigned char *d_codes, float *d_wave, long n, void *stream);
int gtcrn_f32_to_g711(int device, int law, const float *d_wave, unsigned char *d_codes, long n, void *stream);
int gtcrn_g711_decode_table(int law, short *h_table /* [256] */);
int gtcrn_g711_encode_pcm16(int law, int p);

/* ---- level meters: per-stream energies, peak and block count on every live waveform path ------------------------------
 * A conferencing or telephony front end needs, per stream and per tick, how loud the stream is: the RTP audio-level header
 * extension (RFC 6464), a silence / DTX decision, a clip indicator, and "how much is the enhancer taking out" as dry against
 * wet energy.  The emitted block and the dry hop aligned with it meet in registers where the block is written, so the
 * figures cost no launch and no copy of the audio: one 16-byte record per stream.
 *
 * gtcrn_wave_stream_set_meters stores d_meters in the model (as gtcrn_packet_stream_set_dry_gain stores the gains in its
 * handle).  NULL, the default, means no metering: the plain launches, nothing else changes.  While an address is set, every
 * call that runs the wave step -- gtcrn_wave_stream_step*, _flush*, _limited*, _slots*, gtcrn_rate_stream_step*,
 * gtcrn_packet_stream_step* and gtcrn_packet_stream_step_slots* -- updates one RECORD of four floats per stepped stream.
 * The record index follows the dry gains: the contiguous calls use d_meters + 4 n for row n of the call, the slot calls
 * d_meters + 4 d_slots[i].  The array is caller-owned device memory, 16-byte aligned, and must cover every row or slot a
 * call can name; a captured graph holds the address, as it does for the gains.  A null model or a misaligned pointer is
 * GTCRN_ERR_ARG.
 *
 * The record.  All values are taken at 16 kHz, where the wave step works (also in the rate and packet forms):
 *   [0] E_dry  += sum of x^2 over the dry samples aligned with each emitted block: exactly the x of the attenuation limit
 *              (the ring's newest 256 samples for the first hop of a call and for the flush, hop h - 1 of the call's input
 *              rows after that);
 *   [1] E_out  += sum of y^2 over the emitted samples, y the float handed to the store: after the attenuation mix if there
 *              is one, BEFORE the rounding to int16 of the _pcm16 forms;
 *   [2] peak    = max(peak, max |y|): above 1.0 the PCM16 form clipped;
 *   [3] blocks += 1 per emitted 256-sample block (a float: exact to 2^24).
 * Every block the kernel writes counts.  The structural zero blocks -- the first hop of a stream, the flush of a stream that
 * holds fewer than 257 samples -- add 1 to blocks and 0 to both energies.  Rows a call does not step are neither written
 * nor read: slots not named, rows at or beyond the device count, rows of a packet-slot call that have no hop in a round.
 *
 * Accumulation order.  The wave that owns the stream reads the record once, adds hop after hop in order,
 * acc = fl(acc + e_h), and stores it once (lane 0, one 16-byte store; in the flush too).  e_h, the hop's sum, is reduced in
 * ONE fixed order: lane l (0..63) holds samples 2l, 2l + 1, 128 + 2l, 129 + 2l of the block and forms
 * p_l = fl(fl(fl(s0^2 + s1^2) + s2^2) + s3^2), every square and every add one fp32 rounding and no fused multiply-add; then
 * six butterfly steps v_l = fl(v_l + v_(l xor d)), d = 1, 2, 4, 8, 16, 32 in that order, leave e_h in every lane.  The
 * DEPTH D of this order -- the most roundings on a path from a sample to e_h -- is 1 + 3 + 6:
 *     D = 10
 * (and D <= 16 is required of any later change).  So each energy is within m u / (1 - m u), u = 2^-24, m = D + K + 1, of the
 * exact sum after K hops, and a numpy float32 emulation of the order reproduces it bit for bit.  The peak is exact.  Hence
 * metered values do not depend on how a hop sequence is cut into calls or launches: a 2-hop contiguous packet call and two
 * 1-hop rounds of the slot form give the same bits.
 *
 * The caller starts a window by zeroing records (hipMemsetAsync, also as a graph node).  There is no meter state anywhere
 * else: every *_state_bytes and gtcrn_abi_version() are what they were, and the outputs and the model, wave, rate and packet
 * states after a metered call equal the plain call's bit for bit.  A metered call makes the launches of its plain form, one
 * for one (the synthesis is timed as k_wave_synthesis_meter, with or without gains).
 *
 * gtcrn_level_dbov is a pure host function (no device is touched): RFC 6464's level of a window,
 * floor(-10 log10(energy / nsamples) + 0.5) clamped to 0..127, and 127 for energy <= 0 or nsamples <= 0.  Full scale is 1.0,
 * so a full-scale sine gives 3.  Feed it E_out and 256 * blocks.
 * Out of scope: the offline calls (gtcrn_forward_wave* leaves both arrays on the device for the caller to reduce); the
 * spectral gtcrn_stream_step*; the _quant paths; per-packet windows at the caller's rate (the meter is per 16 kHz hop, the
 * caller chooses the window by when it zeroes); a voice-activity decision. */
int gtcrn_wave_stream_set_meters(gtcrn_model *m, float *d_meters);
int gtcrn_level_dbov(double energy, double nsamples);

/* ---- gain ramps: a change of the dry gain is spread over one block ---------------------------------------------------------
 * The attenuation limit is the one control that moves DURING a call.  d_gain is read once per call, so a rewritten beta
 * lands as a step between two adjacent samples: at 0 -> 1 the output jumps from the enhanced to the dry signal, an audible
 * click.  With a ramp the change is spread linearly over the 256 samples (16 ms at 16 kHz) of the next emitted block.
 *
 * d_ramp is a caller-owned device array of one float per stream or slot: the dry gain at which that stream's last emitted
 * block ended.  gtcrn_wave_stream_set_gain_ramp stores it in the model, exactly as gtcrn_wave_stream_set_meters stores
 * d_meters; NULL, the default, switches ramps off; a null model is GTCRN_ERR_ARG and no device is touched.  d_ramp is indexed
 * where the dry gain is read: row n of a contiguous call, d_slots[i] of a slot call, the packet forms' row tables likewise.
 * It is NOT part of the wave state: every *_state_bytes and GTCRN_ABI_VERSION (1) are what they were.  With d_ramp == NULL,
 * or with d_gain == NULL, every call launches exactly the kernels it launched before and d_ramp is neither read nor written.
 *
 * Per launch.  With d_ramp and d_gain both set, a synthesis launch does the following for every stream it names, with
 * p = d_ramp[idx] and g = d_gain[idx]:
 *   - Only the block of hop h == 0 of the call ramps (the flush's block is such a block); later hops of the call use g.
 *   - A structural zero block stays zeros and does not ramp: the first block of a stream (c0 + h == 0) and a flush that has
 *     no block.
 *   - Sample i = 0..255 of the ramping block is wave_mix(beta_i, x_i, w_i), the four-rounding formula of "attenuation limit"
 *     (no fused multiply-add), with r_i = (i + 1) / 256, exact in fp32, and
 *         beta_i = g                                   if p == g or i == 255
 *                = fl( p + fl( fl(g - p) * r_i ) )     otherwise      (every fl() ONE fp32 rounding, no fused multiply-add)
 *   - At the end of the launch d_ramp[idx] = g, always: after a zero block, after a flush and after a flush without a
 *     block.  One lane writes it with a plain vector store.
 *
 * What follows.
 *   Steady state is the limited call: with p == g a ramped call equals the limited call bit for bit -- the output, the
 *     meters and every state tensor.
 *   A stream that joins snaps: after gtcrn_stream_reset_slots, gtcrn_packet_stream_reset_slots or on a fresh state its first
 *     block is a structural zero, which sets d_ramp = g; the next block starts at g with no ramp from the previous tenant of
 *     the slot.  No reset entry point changed.
 *   The cut of hops into calls does not matter: a call with nhops = 2 equals two one-hop calls, as long as the gain is not
 *     rewritten between them.  So the packet forms behave the same whether a tick steps a stream 0, 1 or 2 times (they run
 *     hmax indexed wave steps per tick); a stream with no hop in a tick is not named and keeps its d_ramp.
 *   The formula: beta_i is monotone from p to g, stays inside [min(p, g), max(p, g)] (so inside [0, 1]), ends exactly at g,
 *     and its first step from p is (g - p) / 256 -- checked in numpy float32 over 200 000 (p, g) pairs including 0 <-> 1,
 *     denormals and neighbouring floats, without a violation.  A numpy float32 expression reproduces y bit for bit.
 *   Rate and packet forms: the ramp is made at 16 kHz inside the wave step (256 samples, 16 ms) and passes the outbound stage
 *     like everything else; the stage-by-stage contracts hold word for word.
 *   G.711 forms inherit the ramp: the mix is made in float before companding.
 *   High band: R(w - gamma a) + gamma x takes the ramped w; its steady-state bypass identity is unchanged.
 *   Graph capture: the pointer is a captured kernel argument, like d_meters; a captured step follows gains that change between
 *     replays.
 *   A ramped launch is timed in the row of the form it stands in for (k_wave_synthesis_mix, or k_wave_synthesis_meter).
 *
 * gtcrn_gain_ramp_host is a pure host function: it writes beta_0..255 for one (p, g) with the function the kernel compiles.
 * Out of scope: ramping gamma, the high-band gain (the follow-up: it needs the same word next to the high band's gains);
 * gtcrn_forward_wave_limited (offline, one constant gain per clip); ramp lengths other than one block; the _quant and
 * spectrogram-level calls. */
int gtcrn_wave_stream_set_gain_ramp(gtcrn_model *m, float *d_ramp);
int gtcrn_gain_ramp_host(float p, float g, float *out256);

/* ---- level control: a speech-gated output gain, a limiter and a voice flag per stream ---------------------------------------
 * The synthesis kernel that writes an output block holds the enhanced ("wet") block w, the aligned dry block x ("attenuation
 * limit") and the block m it is about to store.  With level control it also decides, per block, whether the stream holds
 * speech (from the wet energy: the evidence a model-based voice activity decision wants), moves a per-stream gain towards a
 * target level while the stream is voiced, holds the block under a ceiling, and stores y = gain * m instead of m.  No launch,
 * no pass over the audio and no state layout is added.
 *
 * Every operation below is ONE correctly rounded fp32 operation (multiply, add, subtract, divide, square root, min, max,
 * compare); no fused multiply-add is formed and no log / exp runs on the device, so a numpy float32 statement reproduces the
 * outputs and the records bit for bit (tests/alc_checker.py).
 *
 * Parameters.  d_alc_params: caller-owned device memory, 16 floats, 16-byte aligned, ONE set for the states a call steps; read
 * at every launch as wave-uniform values; may be rewritten between calls and between replays of a captured graph.
 *     word 0  theta   absolute block-energy floor, 256 * 10^(floor_dbov / 10), clamped to >= 1e-30
 *     word 1  rho     wet / dry energy ratio, 10^(ratio_db / 10)
 *     word 2  H       hangover in blocks, ceil(hang_ms / 16), integer-valued
 *     word 3  alpha   smoothing of the speech energy, in [0, 1]
 *     word 4  T       target block energy, 256 * 10^(target_dbov / 10)
 *     word 5  a_min   lowest gain, 10^(min_gain_db / 20), clamped to (0, 1]
 *     word 6  a_max   highest gain, 10^(max_gain_db / 20), clamped to >= 1
 *     word 7  d_up    per-block rise factor, 10^(rise_db_s * 0.016 / 20) >= 1
 *     word 8  d_dn    per-block fall factor, 10^(-fall_db_s * 0.016 / 20) <= 1
 *     word 9  c       ceiling amplitude, 10^(ceiling_dbov / 20)
 *     word 10 mode    1.0: the gain is applied; 0.0: measure only (the voice flag and the counts; y = m)
 *     words 11..15    reserved, zero
 * gtcrn_alc_params_host makes the words from a gtcrn_alc_config on the host: double arithmetic, one rounding to float per
 * word, the clamps above; GTCRN_ERR_ARG for a null pointer, a non-finite field, min_gain_db > max_gain_db, a negative slew
 * rate or hang_ms, alpha outside [0, 1] or a mode other than 0 / 1.  Defaults (GTCRN_ALC_DEFAULTS): target -26 dBov, gain
 * range -6 .. +24 dB, rise 6 dB/s, fall 30 dB/s, ceiling -1 dBov, floor -45 dBov, ratio -10 dB, hangover 200 ms, alpha 1/16.
 *
 * Record.  d_alc: caller-owned device memory, 8 floats per stream or slot, 32-byte aligned, indexed as the dry gains and the
 * meters are (row n of a contiguous call, d_slots[i] of a slot call, the packet forms' row tables likewise).
 *     word 0  a       the gain at which the stream's last emitted block ended
 *     word 1  S       the smoothed speech block energy (0: no estimate yet)
 *     word 2  hang    blocks of hangover left
 *     word 3  voice   1.0 or 0.0 for the last emitted block
 *     word 4  voiced  blocks counted as voiced
 *     word 5  blocks  blocks counted
 *     words 6..7      reserved, zero
 * The record is NOT part of any state: every *_state_bytes and GTCRN_ABI_VERSION (1) are what they were.
 *
 * gtcrn_wave_stream_set_alc stores both addresses in the model, as gtcrn_wave_stream_set_meters stores d_meters; both NULL,
 * the default, gives the launches of before, and nothing of this section is read or written.  One NULL and one set, a
 * misaligned address or a null model is GTCRN_ERR_ARG; no device is touched.
 *
 * Per emitted block, in hop order.  w_i: the wet sample; x_i: the dry sample of "attenuation limit"; m_i: the sample the call
 * would store without level control -- wave_mix(beta_i, x_i, w_i) with gains (beta_i ramped as "gain ramps" says), w_i without.
 *   1. E_w = sum w_i^2 and E_x = sum x_i^2 in the meters' order (lane l holds samples 2l, 2l+1, 128+2l, 129+2l and sums
 *      ((s0^2 + s1^2) + s2^2) + s3^2; then the xor butterfly over lane distances 1, 2, 4, 8, 16, 32); pk = max |m_i|.
 *   2. Structural zero, the first block of a stream (c0 + h == 0): the record becomes {1, 0, 0, 0, 0, 0, 0, 0} and the output is
 *      zeros; steps 3..11 do not run.  So a stream that joins starts fresh and no reset entry point changed.  A flush that has
 *      no block emits zeros and leaves the record alone.
 *   3. Non-finite block -- any of E_w, E_x, pk not <= FLT_MAX: a0 = a1 = a, voice = 0, and steps 4..8 do not run: S, hang and
 *      a stay as they are (finite whatever a stream is fed; the stream recovers without a reset).
 *   4. speech = E_w >= theta && E_w >= fl(rho * E_x).
 *   5. speech: hang = H, voice = 1.  Else hang > 0: hang = hang - 1, voice = 1.  Else voice = 0.
 *   6. speech: S = (S == 0) ? E_w : fl(S + fl(alpha * fl(E_w - S))).  Hangover blocks do not move S.
 *   7. a_t = a.  If voice && S > 0:  a* = min(max(sqrt(T / S), a_min), a_max),  a_t = min(max(a*, fl(a d_dn)), fl(a d_up)).
 *      The gain moves only while the stream is voiced: pauses are not pumped.
 *   8. Limiter.  If pk > 0 && fl(pk * max(a, a_t)) > c:  L = max(a_min, c / pk),  a0 = min(a, L),  a1 = min(a_t, L); else
 *      a0 = a, a1 = a_t.  The one place a gain step may land between two samples (a0 != a); no look-ahead, no latency.  The
 *      limiter never goes below a_min: past that the int16 rounding saturates as it does without level control.
 *   9. mode == 0: a0 = a1 = 1.
 *  10. y_i = fl(gain_ramp_at(a0, a1, i) * m_i), gain_ramp_at the function of "gain ramps".  y_i goes to the store (one int16
 *      rounding in the PCM16 forms, companding in the G.711 forms) and, where meters are set, to the meters (E_dry stays the
 *      dry block's).
 *  11. a = a1, voiced += voice, blocks += 1.
 *
 * What follows.
 *   a stays in [a_min, a_max] and S stays finite, always, while the range words are not narrowed.  After a rewrite that puts
 *     a outside the new range (a_max lowered below a, or a_min raised above it) nothing snaps: a moves back into the range at
 *     the slew rate (d_dn or d_up per block) over the following voiced blocks and holds where it is while the stream is not
 *     voiced; from the block at which it is inside the range again it stays inside.
 *   With mode == 0 the outputs, every state tensor, the meters and the ramp words equal the call without level control bit
 *     for bit (1 * m is m); the record still carries voice, voiced, blocks, S and hang, and a == 1.
 *   The record does not depend on how the hops are cut into calls.  Slot and contiguous forms give the same bits.  Rows a
 *     call does not step are neither read nor written.
 *   A NaN or Inf in one stream moves no bit of another stream's output or record ("non-finite input").
 *   Rate, packet and G.711 forms: the gain is made at 16 kHz inside the wave step and passes the outbound stage like
 *     everything else.  Not together with the high band, whose formulas assume the 16 kHz hand-off at unit gain: while the
 *     model holds a level-control address every gtcrn_rate_stream_step_hb* and gtcrn_packet_stream_step*_hb* call returns
 *     GTCRN_ERR_STATE and launches nothing.
 *   Graph capture: both pointers are captured kernel arguments; a captured step follows parameter words rewritten between
 *     replays.
 *   A launch with level control is timed in the row of the form it stands in for (k_wave_synthesis, k_wave_synthesis_mix or
 *     k_wave_synthesis_meter), as a ramped launch is: the timing list is what it was.
 *
 * gtcrn_alc_block_host is a pure host function: one block (steps 1, 3..11; the caller handles step 2) through the functions the
 * kernel compiles -- params16 and the 256-sample blocks w, x, m in, y out, record8 advanced in place.
 * Out of scope: gtcrn_forward_wave* (offline), the spectrogram-level and _quant calls, one parameter set per stream, a
 * per-stream on / off other than separate states. */
typedef struct gtcrn_alc_config {
    double target_dbov;    /* the level the voiced blocks are moved to */
    double min_gain_db;    /* gain range */
    double max_gain_db;
    double rise_db_s;      /* slew rates of the gain, dB per second */
    double fall_db_s;
    double ceiling_dbov;   /* the limiter's ceiling */
    double floor_dbov;     /* a block below this wet level is not speech */
    double ratio_db;       /* ... nor one whose wet / dry energy ratio is below this */
    double hang_ms;        /* hangover */
    double alpha;          /* smoothing of the speech energy */
    int mode;              /* 1: apply the gain; 0: measure only */
} gtcrn_alc_config;
#define GTCRN_ALC_DEFAULTS {-26.0, -6.0, 24.0, 6.0, 30.0, -1.0, -45.0, -10.0, 200.0, 0.0625, 1}
int gtcrn_wave_stream_set_alc(gtcrn_model *m, float *d_alc, const float *d_alc_params);
int gtcrn_alc_params_host(const gtcrn_alc_config *config, float *out16);
int gtcrn_alc_block_host(const float *params16, float *record8, const float *w256, const float *x256, const float *m256,
                         float *y256);

/* ---- tone guard: DTMF and fax tones are detected per stream and passed dry -------------------------------------------------
 * A DTMF digit, a fax calling tone (CNG, 1100 Hz) and an answer tone (ANS, 2100 Hz) are stationary narrow-band signals: what
 * the model removes.  A gateway puts a tone detector beside its suppressor and bypasses the processing while a tone is
 * present.  The synthesis kernel holds the dry block x aligned with the block it emits ("attenuation limit"), so the detector
 * and the bypass cost no launch, no latency and no pass over the audio: one 32-byte record per stream.
 *
 * Everything is taken at 16 kHz inside the wave step, on the dry block x, whether or not gains are set.  Every operation
 * below is ONE correctly rounded fp32 operation and no fused multiply-add is formed, so a numpy float32 statement reproduces
 * the outputs and the records bit for bit (tests/tone_checker.py).
 *
 * Table.  gtcrn_tone_table_host(out) writes 10 x 256 x 2 floats, out[(f * 256 + i) * 2 + {0, 1}] = float(cos(a)), float(sin(a)),
 * a = 2 pi F_f i / 16000 computed in double and rounded once; F = 697, 770, 852, 941 (the DTMF rows), 1209, 1336, 1477, 1633
 * (the columns), 1100, 2100.  The caller uploads it once as d_tone_table (20 480 bytes, 16-byte aligned).
 *
 * Parameters.  d_tone_params: caller-owned device memory, 16 floats, 16-byte aligned, ONE set for the states a call steps; read
 * at every launch as wave-uniform values; may be rewritten between calls and between replays of a captured graph.
 *     word 0  theta    256 * 10^(min_dbov / 10), the floor on one tone's block energy              default -45 dBov
 *     word 1  tau      10^(twist_db / 10)                                                          8 dB
 *     word 2  delta    10^(-dominance_db / 10)                                                     8 dB
 *     word 3  pi2      purity of a tone pair, in (0, 1]                                            0.6
 *     word 4  pi1      purity of a single tone, in (0, 1]                                          0.8
 *     word 5  G        blocks of the same candidate before the guard acts                          1
 *     word 6  N2       blocks before a DTMF digit is reported                                      2
 *     word 7  N1       blocks before a single tone is guarded and reported                         4
 *     word 8  H        hold, in blocks                                                             1
 *     word 9  mode     1.0: guard; 0.0: detect only
 *     word 10 singles  1.0: 1100 / 2100 Hz are looked for; 0.0: DTMF only
 *     words 11..15     zero
 * Counts are integer-valued floats.  gtcrn_tone_params_host makes the words from a gtcrn_tone_config: double arithmetic, one
 * rounding to float per word; GTCRN_ERR_ARG for a null pointer, a non-finite field, a purity outside (0, 1], a negative count
 * (or one above 2^24) or a mode / singles value other than 0 / 1.
 *
 * Record.  d_tone: caller-owned device memory, 8 floats per stream or slot, 32-byte aligned, indexed as the dry gains, the
 * meters and the level-control records are.
 *     word 0  tone     the reported code of the last emitted block: 0 none, 1..16 = 1 + 4 row + col, 17 = 1100 Hz, 18 = 2100 Hz
 *     word 1  cand     the last block's candidate
 *     word 2  run      its run length
 *     word 3  hold     blocks of hold left
 *     word 4  guard    1 if the last block qualified to be passed dry (it was, when mode == 1)
 *     word 5  events   reported onsets
 *     word 6  guarded  blocks counted with guard == 1
 *     word 7  blocks   blocks counted
 * The record is NOT part of any state: every *_state_bytes and GTCRN_ABI_VERSION (1) are what they were.
 *
 * gtcrn_wave_stream_set_tone stores the three addresses in the model, as gtcrn_wave_stream_set_alc stores its two; all NULL,
 * the default, gives the launches of before, and nothing of this section is read or written.  A mixed call (some NULL, some
 * set), a misaligned address or a null model is GTCRN_ERR_ARG; no device is touched.
 *
 * Per emitted block, in hop order.  x_i: the dry sample of "attenuation limit"; w_i: the wet sample.
 *   1. E_x in the meters' order.  For each f: c_f = the sum over the block of fl(x_i cos_f,i), s_f the same with sin -- lane l
 *      holds samples 2l, 2l+1, 128+2l, 129+2l and forms ((p0 + p1) + p2) + p3, then the xor butterfly over lane distances
 *      1, 2, 4, 8, 16, 32.  P_f = fl(fl(c_f^2) + fl(s_f^2)) and e_f = P_f * 2^-7.
 *   2. Structural zero, the first block of a stream (c0 + h == 0): the record becomes eight zeros and nothing else runs.  A
 *      flush that has no block leaves the record alone.
 *   3. The candidate.  r = the first argmax of P over the rows, c = the first argmax over the columns.  The pair candidate
 *      1 + 4 r + c needs ALL of: e_r >= theta and e_c >= theta; e_c <= fl(tau e_r) and e_r <= fl(tau e_c); every other row
 *      P_j <= fl(delta P_r) and every other column P_j <= fl(delta P_c); fl(e_r + e_c) >= fl(pi2 E_x).  Otherwise, with
 *      singles, the first k of 1100 / 2100 with e_k >= theta && e_k >= fl(pi1 E_x) gives 17 or 18.  Otherwise 0.  If any of
 *      E_x, P_f is not <= FLT_MAX, the candidate is 0.
 *   4. The run.  If the candidate is not 0 and equals cand, run += 1; otherwise run = 1 if the candidate is not 0, else 0.
 *      cand = the candidate.  need_g = cand < 17 ? G : N1, need_r = cand < 17 ? N2 : N1.
 *   5. Guard and report.  If cand != 0 && run >= need_g: guard = 1, hold = H.  Else if hold > 0: hold -= 1, guard = 1.  Else
 *      guard = 0.  If cand != 0 && run >= need_r: events += 1 when tone != cand, then tone = cand.  Else if guard == 0:
 *      tone = 0.  During the hold tone stays.
 *   6. If mode == 1 && guard == 1 the block's dry gain is 1 at every sample: with gains m_i = wave_mix(1, x_i, w_i), which is
 *      x_i ("attenuation limit"); without gains m_i = x_i.  With ramp words the ramp word ends the block at 1, and the next
 *      unguarded block ramps 1 -> g by the rule of "gain ramps": entering snaps, leaving ramps.  With tones set, a block ramps
 *      from the carried p to its own target at ANY hop of a call (p is carried from block to block inside the launch).
 *      Otherwise m_i is what the call makes without the guard.
 *   7. Level control (if set) and the meters (if set) then see m exactly as in "level control" (E_w stays the wet block's).
 *      After that guarded += guard, blocks += 1.
 *
 * What follows.
 *   With mode == 0 the outputs, every state, the meters, the ramp words and the level-control records equal the call without
 *     tones bit for bit.  With mode == 1 every unguarded block whose predecessor was unguarded equals that twin too.
 *   A guarded block is the dry input one hop late, bit for bit, in the float, int16 and G.711 forms.
 *   The record does not depend on how the hops are cut into calls.  Slot and contiguous forms give the same bits.  Rows a call
 *     does not step are neither read nor written.
 *   A NaN or Inf in one stream moves no bit of another stream's output or record; its own candidate is 0 while E_x or a P_f
 *     is not finite, and the record stays finite.
 *   Graph capture: the three pointers are captured kernel arguments; a captured step follows rewritten parameter words.
 *   Rate, packet, packet-slot and G.711 forms inherit the guard through the 16 kHz hand-off.
 *   High band: the guard only changes beta, and beta = 1 with gamma = 1 is the bypass identity, so the _hb calls stay legal
 *     with tones set.  They still refuse while a level-control address is set.
 *   No look-ahead: the block in which a tone starts part-way is emitted as the model made it, and H covers the partial last
 *     block.
 *   A launch with tones is timed in the row of the form it stands in for, as a launch with level control is.
 *
 * gtcrn_tone_block_host is a pure host function: steps 1 and 3..5 of one block through the functions the kernel compiles,
 * lane layout and butterfly included -- params16, the table and the 256 dry samples in, record8 advanced in place (words 6
 * and 7 are step 7's and stay), *guard_out = (mode == 1 && guard == 1).
 * Out of scope: gtcrn_forward_wave* (offline), the spectrogram-level and _quant calls, one parameter set per stream,
 * second-harmonic checks, other signalling tones, RFC 4733 packetisation. */
typedef struct gtcrn_tone_config {
    double min_dbov;       /* floor on one tone's level */
    double twist_db;       /* most a row and a column tone may differ */
    double dominance_db;   /* least the strongest row / column stands above the others of its group */
    double pair_purity;    /* share of the block's energy the pair holds */
    double single_purity;  /* ... a single tone holds */
    int guard_blocks;      /* G */
    int digit_blocks;      /* N2 */
    int single_blocks;     /* N1 */
    int hold_blocks;       /* H */
    int mode;              /* 1: guard; 0: detect only */
    int singles;           /* 1: look for 1100 / 2100 Hz too */
} gtcrn_tone_config;
#define GTCRN_TONE_DEFAULTS {-45.0, 8.0, 8.0, 0.6, 0.8, 1, 2, 4, 1, 1, 1}
#define GTCRN_TONE_TABLE_FLOATS 5120
int gtcrn_wave_stream_set_tone(gtcrn_model *m, float *d_tone, const float *d_tone_params, const float *d_tone_table);
int gtcrn_tone_params_host(const gtcrn_tone_config *config, float *out16);
int gtcrn_tone_table_host(float *out /* [GTCRN_TONE_TABLE_FLOATS] */);
int gtcrn_tone_block_host(const float *params16, const float *table, float *record8, const float *x256, int *guard_out);

/* ---- non-finite input: what a NaN or Inf in one stream may touch ---------------------------------------------------------
 * The library seats unrelated callers side by side -- four or seven streams in a workgroup, MFMA tiles that straddle two
 * streams, time spans that run across utterance boundaries -- and a float sample is whatever the caller sent.  The contract
 * for an input that holds a NaN, an Inf, or a finite value whose square overflows, in ONE stream, utterance or row (the
 * victim), on every inference call of this header, offline and live, and on gtcrn_resample:
 *   P1 isolation   every other stream / utterance / row / slot keeps every bit: its outputs at every call and its rows of
 *                  every state (model, wave, rate, packet, high-band state, phase word, meter record).
 *   P2 causality   the victim's outputs before the call that took the value keep every bit.
 *   P3 cone        the model is a FIR in time: spectrum frame t0 reaches output frames t0 .. t0 + 84 and no other -- 85 =
 *                  1 + 2 * 12 + 2 * 30 frames, the encoder / decoder blocks' and the two GTCN stacks' histories.  A NaN in
 *                  one element of frame t0 makes every bin of exactly those frames non-finite, as the float64 reference
 *                  does: no kernel turns it into a finite value.  A sample inside hop h (not the hop's first sample) lies in
 *                  frames h and h + 1 and makes offline output blocks h - 1 .. h + 85 non-finite, 87 blocks of 256 samples,
 *                  every sample of them; the hop form emits them one hop later, the rate and packet forms at their latency
 *                  with the edges widened by the two filters' spans (one contiguous run of samples).  An Inf or an
 *                  overflowing value stays inside the same frames; which of their values are finite is unspecified.
 *   P4 recovery    from the first frame behind the cone on the victim's outputs keep every bit, and 16 frames later (the
 *                  deepest ring of the state) so does its whole state: no field accumulates.  A meter record holds what it
 *                  summed until the caller zeroes it.
 *   P5 reset       resetting the victim through its form's reset (and zeroing its meter record) at any call makes it, from
 *                  that call on, a fresh stream, bit for bit, whatever it held.
 * One legitimate difference between forms: a non-finite x[256] -- the hop form frames hop 0 without its future sample
 * x[256], which meets win[0] == 0, while the offline frame 0 (the reflected one) reads it -- so there the live stream's
 * first frames are finite where the offline call's are not.  Stores of a non-finite value to PCM16 or G.711 outputs are
 * unspecified (the integer forms cannot carry one in).  Training is outside all this: train-mode BatchNorm and the
 * batch-mean loss couple the clips of a batch by definition. */

/* ---- scores: SDR, SI-SNR and STOI of (clean, enhanced) pairs, on the device ------------------------------------------------
 * Replaces sdr_metric / sisnr_metric / stoi_metric of eval/eval_intrusive_metrics.py:22-32,74-91 and stands in for the
 * scoring lines of train.py:_validation_epoch (train.py:343-362) without a copy to the host: B clips at 16 kHz in, one
 * 32-byte record per clip out.  PESQ (ITU C code) and DNSMOS (an ONNX model) stay the caller's.
 *
 * gtcrn_score: row b of d_ref / d_inf holds d_lengths[b] <= L samples (int32 on the device, clamped to 0 .. L; NULL = all L)
 * at d_ref + b * ref_stride / d_inf + b * inf_stride; `what` is a sum of 1 (SDR), 2 (SI-SNR), 4 (STOI); d_out receives B
 * records, fields not asked for written as 0 (kept_frames and segments belong to STOI).  d_workspace: 16-byte aligned,
 * gtcrn_score_workspace_bytes(B, L) bytes (B times a function of L alone); needed only with STOI.  Asynchronous on `stream`;
 * allocates nothing, never synchronises the host, can be captured in a graph.  A null pointer, B outside 1 .. 65535, L
 * outside 1 .. 2^28, a stride shorter than L, `what` outside 1 .. 7 and a missing or misaligned workspace return
 * GTCRN_ERR_ARG before any launch.
 *
 * SDR and SI-SNR, to the letter of the reference, its quirk included (the projection divides by sum(ref^2 + 1e-8), which is
 * sum(ref^2) + n * 1e-8).  With n the clip's length, r = ref - mean(ref), y = inf - mean(inf):
 *     sdr   = 10 log10((sum r^2 + 1e-8) / (sum (y - r)^2 + 1e-8))
 *     a     = sum(y r) / (sum r^2 + n * 1e-8)
 *     sisnr = 10 log10((sum (a r)^2 + 1e-8) / (sum (y - a r)^2 + 1e-8))
 * Samples are read as fp32; every sum is a double one in a fixed order; three passes (the means; the centred sums and a;
 * the two sums of SI-SNR formed from the residual y - a r itself, never expanded from moments).  The reference computes in
 * float32; the tests hold the difference to the reference's own noise floor.  n = 0 gives NaN.
 *
 * STOI: the structure and constants of Taal et al. 2011 as the reference calls it (stoi(ref, inf, 16000, extended=False)).
 * Only the 10 kHz resampling filter is this library's own: pystoi resamples with an Octave-style resampler whose taps differ,
 * so decimal parity with pystoi is neither claimed nor tested; the tests compare with an independent float64 statement of the
 * definition below.  EPS = 2^-52.
 *   1. Both signals 16 kHz -> 10 kHz by the formula of "sample-rate conversion" above with up / down = 5 / 8: q = 8,
 *      half = 256, 513 taps, fc = 0.9375 * 0.5 / 8, the same Kaiser beta, sum(h) = 5, taps rounded once to float, zero
 *      padding, centred; ceil(len * 5 / 8) outputs, each the double sum of its exact products, rounded once to float.
 *      (gtcrn_resampler_create(16000, 10000) stays GTCRN_ERR_ARG: the taps are designed inside the scorer.)
 *   2. Analysis frames start at s = 0, 128, ... < len10 - 256 (strict): n of them.  w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257)),
 *      i = 0 .. 255.  e_j = 20 log10(||w ref_frame_j||_2 + EPS).  Frame j is kept iff e_j > max_j e - 40; the mask comes from
 *      ref alone and applies to both signals; K = the number of kept frames.
 *   3. The kept, windowed frames of each signal are overlap-added at hop 128, in order: (K - 1) * 128 + 256 samples.
 *   4. The result is framed again by the rule of 2, which gives M = K - 1 frames (0 for K = 0); each is windowed by w,
 *      zero-padded to 512, and transformed (rFFT).
 *   5. env[j, m] = sqrt(sum over k = lo_j .. hi_j - 1 of |X[k, m]|^2), 15 bands whose edges are the bins nearest to
 *      150 * 2^((2 j -/+ 1) / 6) Hz on the grid k * 10000 / 512:
 *        lo = 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174
 *        hi = 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219
 *   6. S = M - 29 segments of 30 consecutive frames if M >= 30.  Per band and segment, x of ref and y of inf:
 *      alpha = ||x|| / (||y|| + EPS); y' = min(alpha y, x (1 + 10^(15/20))); the mean over the 30 frames is removed from x
 *      and from y'; each is divided by (its norm + EPS); d = sum x y'.  stoi = the mean of d over the 15 S pairs.  Steps 3
 *      to 5 run in fp32 (the envelopes are stored as float), this step in double.
 *   7. M < 30: stoi = 1e-5 (pystoi's value for this case), segments = 0, kept_frames = K.
 * Properties that belong to the contract:
 *   batch invariance  a clip's record has the same bits whatever B, L and the row it sits in, and whatever lengths the other
 *                     rows have: every reduction is a fixed-order one over the clip's own samples, frames and segments.
 *   non-finite input  ("non-finite input" above) a NaN or Inf in one clip changes no bit of another clip's record, and moves
 *                     no index: K <= n by construction, and every store lands in the clip's own slice of the workspace.
 *                     That clip's own scores are unspecified (NaN or 1e-5).
 *   silence           an all-zero ref, inf or both keeps every score defined by the formulas above (EPS and the 1e-8 terms):
 *                     no division by zero.
 *
 * Host only, no device: gtcrn_score_taps (up = 5, down = 8 and the 513 taps as the kernel uses them; returns the count,
 * h_taps may be NULL), gtcrn_score_bands (the two tables of step 5), gtcrn_score_frames (n of step 2 for an L-sample clip).
 * gtcrn_score_debug (test hook, synchronises `stream`): copies one intermediate of row b of the most recent call with STOI
 * to d_dst as floats and returns the element count: which = 0 the 10 kHz ref (len10), 1 the frame energies in dB (n),
 * 2 the keep mask as 0 / 1 (n), 3 / 4 the ref / inf band envelopes (15 x M, band-major).  The workspace of that call must
 * still be alive.  gtcrn_score_timing(s, 1) records events around the launches of each following call (not under capture);
 * gtcrn_score_timing_read returns launch `stage`'s name and milliseconds of the most recent one, stage = 0 .. 5. */
typedef struct gtcrn_scorer gtcrn_scorer;
typedef struct { double sdr, sisnr, stoi; int kept_frames, segments; } gtcrn_score_record;   /* 32 bytes */
int gtcrn_scorer_create(gtcrn_scorer **out, int device);   /* designs taps / window / tables in double, uploads them */
void gtcrn_scorer_destroy(gtcrn_scorer *s);
size_t gtcrn_score_workspace_bytes(int B, long L);
int gtcrn_score(gtcrn_scorer *s, const float *d_ref, long ref_stride, const float *d_inf, long inf_stride,
                const int *d_lengths, long L, int B, int what, gtcrn_score_record *d_out, void *d_workspace, void *stream);
long gtcrn_score_taps(int *up, int *down, float *h_taps, long cap);
int gtcrn_score_bands(int *lo15, int *hi15);
long gtcrn_score_frames(long L);
long gtcrn_score_debug(gtcrn_scorer *s, int which, int b, float *d_dst, long cap, void *stream);
int gtcrn_score_timing(gtcrn_scorer *s, int on);
int gtcrn_score_timing_read(gtcrn_scorer *s, int stage, char *name, int name_cap, float *ms);

/* ---- scores, extended: ESTOI and segmental SNR next to the three above --------------------------------------------------
 * gtcrn_score_ext is gtcrn_score with a 64-byte record and two more bits in `what`: 8 (ESTOI) and 16 (segmental SNR), so
 * `what` is a sum out of 1, 2, 4, 8, 16 in 1 .. 31.  Same rows, strides, lengths, refusals (GTCRN_ERR_ARG before any launch)
 * and properties as gtcrn_score: asynchronous on `stream`, allocates nothing, never synchronises the host, capturable.  Fields
 * not asked for are written as 0; kept_frames and segments are written when `what` & 12; zero[] is 0.  d_workspace: 16-byte
 * aligned, gtcrn_score_ext_workspace_bytes(B, L) bytes (B times a function of L alone, not less than
 * gtcrn_score_workspace_bytes(B, L)); needed when `what` & 28.  With `what` <= 7 bytes 0 .. 31 of each record are bit for bit
 * what gtcrn_score writes and bytes 32 .. 63 are 0.  gtcrn_score itself is unchanged and keeps refusing `what` > 7.
 * EPS = 2^-52; samples are read as fp32; everything below is in double.
 *
 * ESTOI (Jensen & Taal 2016; the structure of pystoi's stoi(..., extended=True)).  Steps 1 to 5 of STOI above are shared
 * unchanged: the 10 kHz stage, the keep mask from ref, the overlap-add, the re-framing, the fp32 envelopes env[j, m] of 15
 * bands, M = K - 1.  With M >= 30 there are S = M - 29 segments; for segment s, X = env_ref[:, s .. s + 29] and
 * Y = env_inf[:, s .. s + 29] (15 x 30) each go through the same normalisation:
 *   1. rows: from every band's 30 values their mean is subtracted, then they are divided by (their 2-norm + EPS);
 *   2. columns of the result: from every frame's 15 values their mean is subtracted, then they are divided by
 *      (their 2-norm + EPS).
 * d_s = (1 / 30) sum over j, t of X~[j, t] Y~[j, t]; estoi = (1 / S) sum over s of d_s.  No clipping, no alpha.  M < 30:
 * estoi = 1e-5 and segments = 0, as STOI.  pystoi adds EPS-scaled random noise before each normalisation to avoid 0 / 0; this
 * contract has + EPS in the denominators instead.  As for STOI, decimal parity with pystoi is neither claimed nor tested.
 * (The kernel multiplies by 1 / 30, by 1 / 15 and by the reciprocal of a row's denominator, and divides a column's sum of
 * products once by the product of its two denominators: roundings of 1e-16, the same for a segment wherever it is computed.)
 *
 * Segmental SNR: this library's own stated contract (Hansen-Pellom form), no parity with any package claimed; on the 16 kHz
 * rows as given, no mean removal.  With n the clip's length: frames of 480 samples start at s = 0, 120, 240, ... with
 * s + 480 <= n, F = (n - 480) / 120 + 1 of them (integer division) for n >= 480, else 0.
 * w[i] = 0.5 (1 - cos(2 pi (i + 1) / 481)), i = 0 .. 479, designed in double on the host.  Per frame, with r of ref and y of inf:
 *     num = sum (w r)^2,  den = sum (w (r - y))^2      (r - y: the difference of the two fp32 samples, formed in double)
 *     v   = 10 log10(num / (den + EPS) + EPS), clamped to [-10, 35]
 * segsnr = (1 / F) sum of v, frames in ascending order; segsnr_frames = F.  F = 0: segsnr = NaN, as SDR for n = 0.
 *
 * The properties of "scores" hold for the whole 64-byte record: batch invariance (d_s is a function of its segment, v of its
 * frame, and each is summed by a thread's strided partial and a fixed tree that depend on S / F alone), non-finite input (a
 * NaN or Inf in one clip changes no bit of another's record and moves no index), silence (estoi = 0 exactly when either
 * signal is all zero; segsnr = -10 for a zero ref, about 0 for a zero inf, and 35 with estoi about 1 for a signal against
 * itself).
 *
 * Host only, no device: gtcrn_score_segsnr_frames (F for an n-sample clip, n in 0 .. 2^28), gtcrn_score_segsnr_window (the
 * 480 window values).  gtcrn_score_ext_stages: the launches of a call with everything asked for (9); gtcrn_score_timing(s, 1)
 * arms gtcrn_score_ext too, and gtcrn_score_ext_timing_read returns launch `stage`'s name and milliseconds of the most recent
 * gtcrn_score_ext (gtcrn_score_timing_read keeps serving gtcrn_score alone). */
typedef struct { gtcrn_score_record base;        /* bytes 0 .. 31 */
                 double estoi, segsnr;           /* 32, 40 */
                 int segsnr_frames, zero[3]; } gtcrn_score_ext_record;   /* 64 bytes */
size_t gtcrn_score_ext_workspace_bytes(int B, long L);
int gtcrn_score_ext(gtcrn_scorer *s, const float *d_ref, long ref_stride, const float *d_inf, long inf_stride,
                    const int *d_lengths, long L, int B, int what, gtcrn_score_ext_record *d_out, void *d_workspace,
                    void *stream);
long gtcrn_score_segsnr_frames(long n);
int gtcrn_score_segsnr_window(double *h_w480);
int gtcrn_score_ext_stages(void);
int gtcrn_score_ext_timing_read(gtcrn_scorer *s, int stage, char *name, int name_cap, float *ms);

/* ---- training batches from a resident corpus ---------------------------------------------------------------------------
 * Replaces DNS3Dataset.__getitem__ + DataLoader + .to(device) (dataloader.py:113-170, train.py:244-250): the training set
 * lives in device memory as int16 and a batch is cut (and, optionally, mixed) where it lies.  No handle, no host state.
 *
 * Corpus: two caller-owned device buffers.  pcm: int16, all clips back to back, no alignment or padding between them.
 * offsets: int64 [n + 1], clip c = pcm[offsets[c] .. offsets[c + 1]).  Every clip holds 1 .. 2^31 - 1 samples, n < 2^31; the
 * total is unbounded (pcm is indexed with 64 bits).  16 kHz mono is assumed, nothing here looks at a rate.
 *
 * Plan: one 32-byte gtcrn_batch_item per row of the batch, drawn by gtcrn_batch_plan or written by the caller.
 *   Philox4x32-10, key = (seed_lo, seed_hi), counter = (uint32(item0 + b), step_lo, step_hi, k): k = 0 gives r0..r3, k = 1
 *   gives q0..q3.  mulhi(r, K) = (uint64(r) * K) >> 32.
 *     sclip  = d_clips[b] if d_clips, else mulhi(r0, n_speech)          (a d_clips entry outside 0 .. n - 1 is clamped)
 *     Ks     = max(1, (len_s - L) / granule + 1) by integer division, 1 when len_s < L;  sstart = granule * mulhi(r1, Ks)
 *     nclip  = mulhi(r2, n_noise);  nstart = mulhi(r3, len_n)           (both 0 without a noise table)
 *     u(q)   = float(q >> 8) * 2^-24 (exact);  snr_db = lo + (hi - lo) * u(q0), lvl_db likewise from q1: float, every
 *              operation rounded once
 *     snr_amp = float(pow(10.0, -double(snr_db) / 20));  lvl_amp = float(pow(10.0, double(lvl_db) / 20))
 *   d_seed_step: two uint64 on the device, {seed, step}; a batch is a pure function of (seed, step, item0 + b).  item0 is
 *   the first global row of this rank (rank * B): ranks then cut one global batch, whatever the world size.  granule = 1:
 *   sample-exact starts; 16000: the reference's whole-second random_start (dataloader.py:137) on the clip's true length.
 *   advance != 0: a one-thread launch after the plan's adds 1 to step, in stream order.  gtcrn_batch_plan_host is the same
 *   function body on host pointers (it never advances).
 *
 * gtcrn_batch_pairs (the reference's loader; two corpora under ONE offsets table): noisy[b][i] =
 *   float(pcm_noisy[offsets[sclip] + sstart + i]) / 32768 where sstart + i < len, else 0; clean alike.  One launch.
 *
 * gtcrn_batch_mix (dynamic mixing), per row, s_i the speech window (0 past the clip's end), n_i = noise[(nstart + i) mod len_n]:
 *   Ss = sum s_i^2, Sn = sum n_i^2, Ssn = sum s_i n_i as 64-bit integers over the int16 values (exact, order-free).
 *   gn = 0 and flag 1 if Sn == 0; else 1 and flag 2 if Ss == 0; else float(sqrt(double(Ss) / double(Sn)) * double(snr_amp)).
 *   sf_i = float(s_i) / 32768, nf_i = float(n_i) / 32768;  m_i = sf_i + (gn * nf_i): a rounded multiply, a rounded add, NO fma.
 *   g = double(gn);  Sm = double(Ss) + g * (2.0 * double(Ssn) + g * double(Sn)), clamped at 0;  peak = max |m_i| (float).
 *   G = 1 and flag 4 if Sm == 0; else rms = sqrt(Sm / L) / 32768, G = double(lvl_amp) / rms, and if double(peak) * G > 0.99
 *   then G = 0.99 / double(peak), flag 8.  Gf = float(G);  noisy[b][i] = Gf * m_i, clean[b][i] = Gf * sf_i.
 *   d_records[b] = {Ss, Sn, Ssn, gn, Gf, peak, flags}.  Given a plan the output is defined bit for bit.
 *   Three launches over (row, chunk) grids: integer partial sums, peak, write; d_workspace (16-byte aligned,
 *   gtcrn_batch_workspace_bytes(B, L)) holds the partials.  passes = 7 is a draw; a subset (1 sums, 2 peak, 4 write) repeats
 *   single launches on a workspace a full draw has filled (tools/batch_bench.py times them).
 *   A plan entry outside its table is clamped into it (sclip, nclip, nstart; sstart < 0 counts as 0): a wrong plan gives
 *   wrong audio, never an access outside pcm.
 *
 * Output rows are float32 with noisy_stride / clean_stride >= L floats between them.  Everything is asynchronous on `stream`,
 * allocates nothing and is capturable.  B <= 0, L <= 0 or L >= 2^31, an empty corpus, a null table or buffer, granule < 1,
 * hi < lo and a stride below L return GTCRN_ERR_ARG before anything is enqueued.  Out of scope: other sample rates, float
 * corpora, streaming a corpus larger than device memory from disk.  (Room impulse responses: the next section; levels over
 * active windows instead of the plain RMS: "active levels".) */
typedef struct { int sclip, sstart, nclip, nstart; float snr_db, snr_amp, lvl_db, lvl_amp; } gtcrn_batch_item;   /* 32 bytes */
typedef struct { long long Ss, Sn, Ssn; float gn, Gf, peak; int flags; } gtcrn_batch_record;                   /* 40 bytes */
int gtcrn_batch_plan(const long long *d_speech_offsets, int n_speech, const long long *d_noise_offsets, int n_noise, int B,
                     long L, long item0, int granule, float snr_lo, float snr_hi, float lvl_lo, float lvl_hi,
                     const int *d_clips, unsigned long long *d_seed_step, int advance, gtcrn_batch_item *d_plan, void *stream);
int gtcrn_batch_plan_host(const long long *h_speech_offsets, int n_speech, const long long *h_noise_offsets, int n_noise, int B,
                          long L, long item0, int granule, float snr_lo, float snr_hi, float lvl_lo, float lvl_hi,
                          const int *h_clips, const unsigned long long *h_seed_step, gtcrn_batch_item *h_plan);
size_t gtcrn_batch_workspace_bytes(int B, long L);   /* 0 (and GTCRN_ERR_ARG recorded) for a bad shape */
int gtcrn_batch_pairs(const short *d_noisy_pcm, const short *d_clean_pcm, const long long *d_offsets, int n,
                      const gtcrn_batch_item *d_plan, int B, long L, float *d_noisy, long noisy_stride, float *d_clean,
                      long clean_stride, void *stream);
int gtcrn_batch_mix(const short *d_speech_pcm, const long long *d_speech_offsets, int n_speech, const short *d_noise_pcm,
                    const long long *d_noise_offsets, int n_noise, const gtcrn_batch_item *d_plan, int B, long L, float *d_noisy,
                    long noisy_stride, float *d_clean, long clean_stride, gtcrn_batch_record *d_records, void *d_workspace,
                    int passes, void *stream);

/* ---- reverberant speech: exact RIR convolution ----------------------------------------------------------------------------
 * The DNS noisy files the reference trains on were synthesised from REVERBERANT speech; a dynamic mix of dry speech is not
 * that data.  gtcrn_batch_reverb convolves each row's speech window with a room impulse response before the mix, in exact
 * integer arithmetic: the result is a function of its inputs, not of a summation order.  Additions only; no handle, no host
 * state, caller-owned buffers, everything asynchronous on `stream`, capturable, nothing allocated.
 *
 * RIR bank: shaped like a corpus.  taps: int16 Q15 (32768 = 1.0), all responses back to back; offsets: int64 [n + 1].  Every
 * response holds 1 .. GTCRN_REVERB_MAX_TAPS taps (1.024 s) and every tap lies in -GTCRN_REVERB_TAP_MAX .. GTCRN_REVERB_TAP_MAX
 * (+-32639 = 127 * 256 + 127: both balanced int8 digits of a tap then fit; a tap outside gives wrong audio).  Speech is NOT
 * restricted: -32768 and 32767 are exact.  A response whose offsets give another length counts as absent (its rows stay dry).
 *
 * Reverb plan: one 8-byte gtcrn_reverb_item per row, drawn by gtcrn_batch_reverb_plan or written by the caller; rir < 0: the
 * row stays dry.  The batch plan's Philox4x32-10, same key and counter, block k = 2 gives t0..t3 (k = 0, 1 are the batch
 * plan's, so no existing plan changes):  rir = mulhi(t1, n_rir) if u(t0) < p_reverb, else -1; reserved = 0.  p_reverb = 0
 * never reverberates a row, 1 always does.  The function READS d_seed_step and never advances it: launch it BEFORE
 * gtcrn_batch_plan in the stream, it then sees the step that plan is about to use.  gtcrn_batch_reverb_plan_host is the same
 * function body on host pointers.
 *
 * gtcrn_batch_reverb, per row b with c = plan[b].sclip, s0 = plan[b].sstart, response h of K taps:
 *   acc[i] = sum_{k=0}^{K-1} h[k] * x[s0 + i - k],  i = 0 .. L - 1, a 64-bit integer, exact;
 *   x[j]   = clip c's sample j for 0 <= j < len_c, else 0 (true history before the window; zeros before the clip and behind it);
 *   wet[i] = clamp((acc[i] + 16384) >> 15, -32768, 32767), an arithmetic shift;  a dry row: wet[i] = x[s0 + i].
 *   d_staged[b * staged_stride + i] = wet[i] (int16; samples L .. staged_stride - 1 of a row are not touched);
 *   d_staged_offsets[b] = b * staged_stride for b = 0 .. B (B + 1 entries): with d_staged a corpus of B clips, of which only
 *   the first L samples are read;  d_staged_plan[b] = d_plan[b] with sclip = b, sstart = 0.  gtcrn_batch_mix then runs
 *   UNCHANGED on (d_staged, d_staged_offsets, B, d_staged_plan): its clean output is the reverberant speech, the target of a
 *   model that does not dereverberate.  With every row dry the draw is bit-identical to the draw without this call.
 *   d_records[b] = {rir (as used: clamped, -1 for a dry row), ntaps, saturated = the number of clamped samples, 0}.
 *   A plan entry outside its table is clamped into it (sclip, rir > n_rir - 1; sstart < 0 counts as 0): a wrong plan gives wrong
 *   audio, never an access outside a buffer.  Given the plans the output is defined bit for bit, in both forms:
 *   form 1, plain: one thread per output sample, the sum as written above.  form 2, matrix: int16 operands as two int8 digits
 *   (tap = 256 * hi + lo, both in -127 .. 127; sample = 256 * (x >> 8) + ((x & 255) - 128) + 128, zero padding stored as the
 *   digits of 0, so the + 128 adds 128 * sum(h) per output), digit products on v_mfma_i32_16x16x64_i8 into int32 (below
 *   2^31 for 16384 + 255 terms), recombined in int64; a workgroup takes 8192 output samples of a row if B rows of such blocks
 *   make 256 workgroups, else 2048; forms 3 and 4 pin the small and the large block (the A/B switch of tests and
 *   measurements).  form 0: the library chooses (form 2).  The matrix form reads a table derived from the bank:
 *   gtcrn_batch_reverb_table_bytes(host offsets, n) bytes, 16-byte aligned, filled once per bank by
 *   gtcrn_batch_reverb_prepare (16 bytes per tap and digit, taps padded to whole 256); form 1 takes d_table = NULL.  A table of another bank
 *   gives wrong audio (rows whose entry does not lie inside table_bytes stay dry), never an access outside it.
 *   d_workspace: gtcrn_batch_reverb_workspace_bytes(B, L) bytes, 4-byte aligned (per-workgroup clamp counts; integers, so the
 *   total is order-free).  Two launches: the convolution over a (row, block) grid, then records / offsets / plan.
 * B <= 0, L <= 0 or L >= 2^31, an empty corpus or bank, a null or misaligned buffer, a stride below L, p_reverb outside 0 .. 1,
 * an unknown form and a matrix form without its table return GTCRN_ERR_ARG before anything is enqueued.  Out of scope:
 * responses longer than 16384 taps, multichannel responses.  (Early-reflection or direct-path targets: the next section.) */
#define GTCRN_REVERB_MAX_TAPS 16384
#define GTCRN_REVERB_TAP_MAX 32639
typedef struct { int rir, reserved; } gtcrn_reverb_item;                        /* 8 bytes */
typedef struct { int rir, ntaps, saturated, reserved; } gtcrn_reverb_record;    /* 16 bytes */
int gtcrn_batch_reverb_plan(int n_rir, float p_reverb, int B, long item0, const unsigned long long *d_seed_step,
                            gtcrn_reverb_item *d_rplan, void *stream);
int gtcrn_batch_reverb_plan_host(int n_rir, float p_reverb, int B, long item0, const unsigned long long *h_seed_step,
                                 gtcrn_reverb_item *h_rplan);
size_t gtcrn_batch_reverb_table_bytes(const long long *h_rir_offsets, int n_rir);   /* 0 (and GTCRN_ERR_ARG recorded) for a bad bank */
int gtcrn_batch_reverb_prepare(const short *d_taps, const long long *d_rir_offsets, int n_rir, void *d_table, size_t table_bytes,
                               void *stream);
size_t gtcrn_batch_reverb_workspace_bytes(int B, long L);                           /* 0 (and GTCRN_ERR_ARG recorded) for a bad shape */
int gtcrn_batch_reverb(const short *d_speech_pcm, const long long *d_speech_offsets, int n_speech, const short *d_taps,
                       const long long *d_rir_offsets, int n_rir, const void *d_table, size_t table_bytes,
                       const gtcrn_batch_item *d_plan, const gtcrn_reverb_item *d_rplan, int B, long L, short *d_staged,
                       long staged_stride, long long *d_staged_offsets, gtcrn_batch_item *d_staged_plan,
                       gtcrn_reverb_record *d_records, void *d_workspace, int form, void *stream);

/* ---- dereverberation targets: early or direct clean ---------------------------------------------------------------------------
 * The clean output of the section above is the full reverberant speech: a model trained from it learns to denoise.  To train
 * it to remove the late tail the target is the early part of the response, or the direct path alone.  The convolution is
 * linear, so after the first E taps its accumulators ARE that target: gtcrn_batch_reverb_split writes them out and walks on
 * into the tail -- one pass over the speech, two staged corpora, still exact integers.  gtcrn_batch_mix_target then takes its
 * clean rows from the second.  Additions only: nothing above changes.
 *
 * Split: d_split, int32 [n_rir], E_r in 1 .. K_r, the number of leading taps of response r that make the target (E_r = K_r:
 * the target is the wet row).  A value outside 1 .. K_r is clamped into it: a wrong value gives wrong audio, never an access
 * outside a buffer.
 *
 * gtcrn_batch_reverb_split, per wet row b with h, K, s0 and x[] exactly as in gtcrn_batch_reverb and E = split[rir]:
 *   early[i] = sum_{k<E} h[k] * x[s0 + i - k];   acc[i] = early[i] + sum_{k>=E} h[k] * x[s0 + i - k]     (64-bit integers, exact)
 *   d_staged_target[b * staged_stride + i] = clamp((early[i] + 16384) >> 15);   d_staged[b * staged_stride + i] =
 *   clamp((acc[i] + 16384) >> 15): the latter is gtcrn_batch_reverb's wet row, bit for bit, for any split.  A dry row copies x
 *   into both.  The two staged buffers share staged_stride, d_staged_offsets and d_staged_plan (written as above): the target
 *   is a corpus parallel to the wet one under one offsets table.
 *   d_records[b] = {rir, ntaps, saturated (as above), split = E as used (0 for a dry row), target_saturated = the clamped
 *   samples of the target row, 0, 0, 0}: 32 bytes.
 *   d_workspace: gtcrn_batch_reverb_split_workspace_bytes(B, L) bytes, 4-byte aligned: two per-workgroup clamp counts.
 *   Forms: the numbering above, and all agree on every bit.  1, plain: one thread per output sample, two accumulators, the sums
 *   as written.  2, matrix (0: the library chooses it); 3 / 4 pin the 2048 / 8192 block, the block rule is the one above.  The
 *   matrix form runs the chunks of the early taps, the epilogue into the target row with bias 128 * sum(h[:E]), does NOT reset
 *   its accumulators, runs the chunks of the rest and the epilogue into the wet row with bias 128 * sum(h).  Padding taps are
 *   stored as zero and add zero products, so every int32 accumulator holds a subset of the terms it holds in
 *   gtcrn_batch_reverb: the bound above (below 2^31 for 16384 + 255 terms) covers both epilogues.
 *   Split table (matrix form): gtcrn_batch_reverb_split_table_bytes(host offsets, host split, n) bytes, 16-byte aligned,
 *   filled once per (bank, split) by gtcrn_batch_reverb_split_prepare.  Header: 32 bytes per response {int64 byte offset,
 *   int64 sum(h[:E]), int64 sum(h), int64 E}, padded to whole 256 bytes.  Per response two contiguous segments in the tile
 *   format above: taps 0 .. E - 1 padded with zeros to 16 * ceil((E + 15) / 256) groups, then -- absent when E == K -- groups
 *   16 * floor(E / 256) .. of the response with its taps below E stored as zero (the 256-tap block that holds E is there
 *   twice, cut at E; one block more than gtcrn_batch_reverb's table, two when E mod 256 > 241).
 *   The matrix form takes E from the table's header (clamped as a split is) and checks that both segments lie inside
 *   table_bytes -- a row whose entry does not stays dry in both outputs; the plain form and the record take E from d_split.  A
 *   table prepared from another split or bank gives wrong audio, never an access outside a buffer.
 * Argument errors as for gtcrn_batch_reverb; a null d_split or d_staged_target is one too.  Refused before anything is enqueued.
 *
 * gtcrn_batch_mix_target: gtcrn_batch_mix with one more corpus, d_target_pcm, under the SPEECH offsets table (as the two
 * sides of gtcrn_batch_pairs).  Everything is as in the mix contract but the clean output: clean[b][i] = Gf * tf_i, tf_i =
 * float(t_i) / 32768, t_i = target[offsets[sclip] + sstart + i] inside the clip, else 0.  The sums, both gains, the peak, the
 * limiter, the record and noisy come from the speech side: the SNR is that of the speech the model hears.  Passes 1 and 2 are
 * gtcrn_batch_mix's launches, pass 3 a write kernel of its own.  With d_target_pcm == d_speech_pcm the call is bit-identical
 * to gtcrn_batch_mix.  After gtcrn_batch_reverb_split: speech = d_staged, target = d_staged_target, plan = d_staged_plan.  A
 * caller who owns paired (degraded, target) speech mixes noise in on the device with the same call.
 * Out of scope: targets that need a response of their own (a shortened-decay tail), responses longer than 16384 taps. */
typedef struct { int rir, ntaps, saturated, split, target_saturated, reserved[3]; } gtcrn_reverb_split_record;   /* 32 bytes */
size_t gtcrn_batch_reverb_split_table_bytes(const long long *h_rir_offsets, const int *h_split, int n_rir);   /* 0 for a bad bank */
int gtcrn_batch_reverb_split_prepare(const short *d_taps, const long long *d_rir_offsets, const int *d_split, int n_rir,
                                     void *d_table, size_t table_bytes, void *stream);
size_t gtcrn_batch_reverb_split_workspace_bytes(int B, long L);                               /* 0 for a bad shape */
int gtcrn_batch_reverb_split(const short *d_speech_pcm, const long long *d_speech_offsets, int n_speech, const short *d_taps,
                             const long long *d_rir_offsets, const int *d_split, int n_rir, const void *d_table,
                             size_t table_bytes, const gtcrn_batch_item *d_plan, const gtcrn_reverb_item *d_rplan, int B, long L,
                             short *d_staged, short *d_staged_target, long staged_stride, long long *d_staged_offsets,
                             gtcrn_batch_item *d_staged_plan, gtcrn_reverb_split_record *d_records, void *d_workspace, int form,
                             void *stream);
int gtcrn_batch_mix_target(const short *d_speech_pcm, const long long *d_speech_offsets, int n_speech, const short *d_noise_pcm,
                           const long long *d_noise_offsets, int n_noise, const short *d_target_pcm,
                           const gtcrn_batch_item *d_plan, int B, long L, float *d_noisy, long noisy_stride, float *d_clean,
                           long clean_stride, gtcrn_batch_record *d_records, void *d_workspace, int passes, void *stream);

/* ---- active levels: the mix at an SNR of the levels while each side is active ------------------------------------------------
 * gtcrn_batch_mix levels speech and noise by their plain RMS over the row.  A clip shorter than the row, pauses, and the build-up
 * and tail of a reverberant row put samples without speech into that mean: the noise is scaled too low and the SNR while
 * somebody speaks is higher than the drawn one (a 2 s utterance in a 4 s row: 3 dB).  gtcrn_batch_mix_active levels each side
 * over its ACTIVE windows.  The rule is the familiar one of DNS-style synthesizers -- fixed windows, an energy threshold, each
 * side judged by its own activity -- but the threshold is absolute, not applied after a normalisation: the contract is this
 * library's own and no parity with an outside tool is claimed.
 *
 * Inputs as gtcrn_batch_mix_target, with d_target_pcm NULLABLE (null: clean is cut from the speech side, as gtcrn_batch_mix), plus
 *   window W in samples, a multiple of 8, 8 <= W <= 2^20 (production: 1600, 100 ms), and
 *   threshold thr, an integer mean-square level in int16^2 units, 0 <= thr <= 2^30 (floor(2^30 * 10^(dB / 10)) re full scale,
 *   computed by the caller: -50 dB -> 10737).
 * Window w of a row covers row samples [w W, min((w + 1) W, L)), n_w its length (the last one may be short); windows are aligned
 * to the row, not to the clip.  Per side, E_w = the 64-bit sum of squares of the int16 samples AS MIXED (the speech window with
 * zeros past the clip's end; the wrapped noise window; the staged wet speech of a reverberant row).  Window w is active on that
 * side iff E_w > thr * n_w: an int64 comparison (both sides below 2^51), equality is inactive.
 *   As = sum E_w, Ns = sum n_w over the speech-active windows; An, Nn likewise over the noise-active windows;
 *   Ss, Sn, Ssn: the whole-row sums of gtcrn_batch_mix.
 *   Fallback: Ns == 0 -> As = Ss, Ns = L, flag 16 (SPEECH_INACTIVE);  Nn == 0 -> An = Sn, Nn = L, flag 32 (NOISE_INACTIVE).
 *   gn = 0 and flag 1 if An == 0; else 1 and flag 2 if As == 0; else
 *     r = double(As) / double(An);  if (Ns != Nn) r = r * (double(Nn) / double(Ns));  gn = float(sqrt(r) * double(snr_amp)):
 *     every conversion and operation rounds once, in double, in this order.
 * Everything after gn is gtcrn_batch_mix, unchanged: m_i, the peak, Gf from the PLAIN mixture RMS over L (what the level range
 * describes), the 0.99 limiter, noisy, clean (or the target row), flags 1, 2, 4, 8.  When every window of both sides is active
 * (Ns == Nn == L) the output and the shared record fields equal gtcrn_batch_mix's bit for bit.
 * d_records[b] = {Ss, Sn, Ssn, As, An, Ns, Nn, gn, Gf, peak, flags}; As, An, Ns, Nn as USED, i.e. after the fallback.
 * Energies and decisions are exact integers, so the output is defined bit for bit given a plan and does not depend on how a row
 * is cut over workgroups.  Three launches as gtcrn_batch_mix's, kernels of their own; a chunk is a whole number of windows.
 * d_workspace: gtcrn_batch_active_workspace_bytes(B, L, window) bytes, 16-byte aligned; `passes` as gtcrn_batch_mix.
 * Argument errors as gtcrn_batch_mix_target's, then a bad window, then a bad threshold: GTCRN_ERR_ARG before anything is
 * enqueued.  Out of scope: an active-level lvl_db, a threshold relative to the clip, hangover smoothing and P.56-style
 * envelope followers, activity labels as an output. */
typedef struct { long long Ss, Sn, Ssn, As, An; int Ns, Nn; float gn, Gf, peak; int flags; } gtcrn_batch_active_record;   /* 64 bytes */
size_t gtcrn_batch_active_workspace_bytes(int B, long L, int window);   /* 0 (and GTCRN_ERR_ARG recorded) for a bad shape */
int gtcrn_batch_mix_active(const short *d_speech_pcm, const long long *d_speech_offsets, int n_speech, const short *d_noise_pcm,
                           const long long *d_noise_offsets, int n_noise, const short *d_target_pcm,
                           const gtcrn_batch_item *d_plan, int B, long L, float *d_noisy, long noisy_stride, float *d_clean,
                           long clean_stride, int window, long long threshold, gtcrn_batch_active_record *d_records,
                           void *d_workspace, int passes, void *stream);

/* ---- telephone-channel rows: exact 8 kHz band + G.711 -------------------------------------------------------------------------
 * The live side serves 8 kHz streams and G.711 packets; a telephone stream reaches the 16 kHz model with nothing above 4 kHz and
 * with the log-PCM noise floor of a G.711 hop.  gtcrn_batch_phone gives a drawn share of the rows of a batch both properties.  It
 * is a post-pass over the float rows a draw has written, so it composes with every draw form without entering their kernels, and
 * it is integers only, so that a few lines of numpy restate it bit for bit (tests/phone_checker.py).
 *
 * Filter table: 129 integers T[0 .. 128].  h is the 16 kHz -> 8 kHz design of "sample-rate conversion" above: up / down = 1 / 2,
 * q = 2, half = 64, fc = 0.9375 * 0.5 / 2, Kaiser beta = 8.95926, scaled to sum(h) = 1, in double on the host;
 * T[n] = rint(32768 h[n]).  sum(T) = 32766, max(T) = T[64] = 15360, sum |T| = 69558, ten taps are 0, T[n] = T[128 - n]; no
 * 32768 h[n] lies within 0.003 of a rounding tie, so two double designs cannot disagree.  Within +0.002 / -0.112 dB up to
 * 3500 Hz, at least 70 dB down from 4500 Hz on (-70.3 dB at 8 kHz: the even and the odd taps sum to 16378 and 16388).
 * gtcrn_batch_phone_taps (host only) returns 129 and fills h_taps exactly as the kernel uses it.
 *
 * Per row, a source row r of L floats, J = ceil(L / 2):
 *   1. p_i = clip(rint(32768 r_i), -32768, 32767): the _pcm16 rounding, half to even.
 *   2. v_j = sat16((sum_i p_i T[2j - i + 64] + 2^14) >> 15), j < J, over 0 <= i < L with the tap index in 0 .. 128: samples
 *      outside the row are zero (centred, no delay); the shift is arithmetic, so the rounding is half up.
 *   3. w_j = v_j (codec 0, linear 8 kHz PCM), D_mu[E_mu(v_j)] (codec 1) or D_A[E_A(v_j)] (codec 2): E and D of "G.711 payloads".
 *   4. z_i = sat16((sum_j w_j T[i - 2j + 64] + 2^13) >> 14), i < L, over 0 <= j < J.
 *   5. out_i = float(z_i) / 32768 (exact).
 * sat16 clips to -32768 .. 32767.  Every sum is exact; |sum| <= 69558 * 32768 does not fit 32 bits, and the kernel does not
 * wrap: 32-bit partial sums over tap subsets whose sum |T| * 32768 < 2^31, joined in 64 bits (csrc/phone.h).
 *
 * Phone plan: one 8-byte gtcrn_phone_item {codec, reserved} per row, drawn from the batch plan's Philox4x32-10 with the same
 * key and counter, block k = 3 (0 and 1 are the batch plan, 2 the reverb plan: none of their draws move), t = its four words:
 * the row is a phone row iff unit24(t0) < p_phone, and its codec is then the mulhi(t1, popcount(codec_mask))-th set bit of
 * codec_mask counted from the low end (bit 0 linear, bit 1 mu-law, bit 2 A-law); codec = -1: a wide-band row.
 * gtcrn_batch_phone_plan runs on the device, reads d_seed_step and never advances it: it goes BEFORE gtcrn_batch_plan in the
 * stream, as the reverb plan does.  gtcrn_batch_phone_plan_host is the same function body on host pointers.  p_phone outside
 * 0 .. 1 or codec_mask outside 1 .. 7 -> GTCRN_ERR_ARG.
 *
 * gtcrn_batch_phone: for a phone row, noisy = steps 1 - 5 of the source noisy row; clean = steps 1, 2, 4, 5 of the source clean
 * row with target = 0 ("narrow": the same band, no codec -- a mask model cannot restore a band its input does not have) or the
 * source clean row, copied, with target = 1 ("wide").  A row with codec = -1 is copied to both outputs bit for bit; a plan
 * entry outside -1 .. 2 counts as -1.  d_src_clean and d_clean may both be NULL (noisy only).  d_records[b] = {codec,
 * saturated_down, saturated_up, reserved}: the counts of sat16 clips in steps 2 and 4 of the noisy row (0 for a wide-band row).
 * Asynchronous on `stream`, allocates nothing, capturable: a small launch that writes the records and one launch over (row,
 * chunk, side), a workgroup per gtcrn_batch_phone_chunk() consecutive outputs, the 128-sample halo recomputed.  GTCRN_ERR_ARG
 * before any launch: B <= 0, L <= 0 or L >= 2^31, a null row buffer, plan or records, one of the clean pair NULL and the other
 * not, a stride below L, target outside {0, 1}, a misaligned pointer, and a source range that overlaps a destination range
 * (the halo reads make in-place use a race).  A NaN or Inf in one source row leaves that row's output and record unspecified
 * and changes no bit of any other row.  No load falls outside [0, L) of a row, whatever the plan holds.
 * gtcrn_batch_phone_host: the same arguments on host pointers, no device and no stream; it runs the very functions the kernel
 * compiles (csrc/phone.h), as gtcrn_batch_plan_host does for the plan.
 *
 * Out of scope: a 300 Hz high-pass or an IRS send / receive characteristic; other codecs; packet loss and jitter; a channel in
 * front of the mix (speech through the phone, noise added after); corpora at 8 kHz; a per-row target. */
#define GTCRN_PHONE_TAPS 129
typedef struct { int codec, reserved; } gtcrn_phone_item;                                  /* 8 bytes */
typedef struct { int codec, saturated_down, saturated_up, reserved; } gtcrn_phone_record;  /* 16 bytes */
int gtcrn_batch_phone_taps(int *h_taps /* [129] */);
int gtcrn_batch_phone_chunk(void);
int gtcrn_batch_phone_plan(float p_phone, int codec_mask, int B, long item0, const unsigned long long *d_seed_step,
                           gtcrn_phone_item *d_plan, void *stream);
int gtcrn_batch_phone_plan_host(float p_phone, int codec_mask, int B, long item0, const unsigned long long *h_seed_step,
                                gtcrn_phone_item *h_plan);
int gtcrn_batch_phone(const float *d_src_noisy, long src_noisy_stride, const float *d_src_clean, long src_clean_stride,
                      const gtcrn_phone_item *d_plan, int B, long L, float *d_noisy, long noisy_stride, float *d_clean,
                      long clean_stride, int target, gtcrn_phone_record *d_records, void *stream);
int gtcrn_batch_phone_host(const float *h_src_noisy, long src_noisy_stride, const float *h_src_clean, long src_clean_stride,
                           const gtcrn_phone_item *h_plan, int B, long L, float *h_noisy, long noisy_stride, float *h_clean,
                           long clean_stride, int target, gtcrn_phone_record *h_records);

/* ---- conference rooms: mix-minus of the loudest talkers ------------------------------------------------------------------------
 * The one step of a conference bridge that crosses streams: every participant of a room receives the sum of the other talkers,
 * limited to the K who are speaking, faded over one block when the talkers change.  A post-pass over the enhanced blocks a live
 * step has just written (any rate, any packet form: rows of n samples), with no handle and in no existing kernel; a caller who
 * does not mix issues the launches they issued before.  Stated operation by operation, every fl() one correctly rounded fp32
 * operation (the files are compiled with -ffp-contract=off), so that a page of numpy restates it bit for bit
 * (tests/mixer_checker.py).
 *
 * One call: d_in holds n_in rows of n samples (1 <= n <= 1024) at in_stride, d_out n_out rows at out_stride; the two ranges may not
 * overlap.  d_room_start[R + 1]: room r holds the seats [d_room_start[r], d_room_start[r + 1]) of d_seats (n_seats of them, 16-byte
 * aligned), a seat four ints {in_row, out_row, rec, 0}: in_row = -1 the participant sent nothing this tick, out_row = -1 nothing
 * is to be written for them, rec their record.  d_nrooms (may be NULL) is a device word: rooms at or above *d_nrooms are
 * skipped, so that one captured call serves a changing set of rooms.  d_rec: n_rec records of 4 floats {g, level, picked, blocks},
 * 16-byte aligned; a zeroed record is a fresh participant.  d_params: 8 floats, 16-byte aligned, read at launch: {K (1 .. 8, an
 * integer), theta1 = 10^(floor_dbov / 10), alpha in [0, 1], kappa = 10^(incumbent_db / 10) >= 1, 0, 0, 0, 0}; gtcrn_mix_params_host
 * makes them (double arithmetic, one rounding to float per word; GTCRN_ERR_ARG for a null pointer, a non-finite field, k outside
 * 1 .. 8, alpha outside [0, 1], incumbent_db < 0).  Defaults (GTCRN_MIX_DEFAULTS): K = 3, floor -50 dBov, alpha 0.125, 3 dB.  A K
 * that gtcrn_mix_params_host did not make is clamped to 1 .. 8.  d_voice (may be NULL): float words, that of a seat at
 * d_voice[rec * voice_stride]; level control's voice flag is read in place with d_voice = d_alc + 3, voice_stride = 8.
 *
 * Per live room, the seats in table order (s the samples of a seat's in_row; in the _pcm16 form s = p / 32768, exact):
 *   1. E: lane l of 64 runs acc = +0; for j = l, l + 64, ... < n: acc = fl(acc + fl(s_j s_j)); then the xor butterfly
 *      v_l = fl(v_l + v_(l xor d)) over d = 1, 2, 4, 8, 16, 32.
 *   2. present iff in_row is valid and E <= FLT_MAX (read from the bits: a NaN fails).  A seat that is not present contributes
 *      nothing, keeps its level and counts as g_old = 0: a non-finite block never reaches another participant.
 *   3. level = E >= level ? E : fl(level + fl(alpha fl(E - level))).
 *   4. eligible iff d_voice[rec * voice_stride] != 0, or without d_voice iff E >= fl(theta1 fl(n)).
 *   5. key = eligible ? (g_old == 1 ? fl(kappa level) : level) : -1, g_old the record's g.
 *   6. up to K rounds, each taking the unpicked seat of largest key, key > 0, ties to the lowest seat position: t = 1, else 0.
 *   7. r_i = fl(fl(i + 1) / fl(n)); the gain of sample i is 1 (g_old 1, t 1), r_i (0, 1: fade in), fl(1 - r_i) (1, 0: fade out),
 *      0 (0, 0).  The contributors are the present seats with g_old + t > 0: at most 2 K while every g = 1 was written by a call
 *      with K <= 8 (of more than 16, the first 16 in seat order count).
 *   8. for every seat with a valid out_row: acc = +0; for each contributor c other than this seat, in seat order:
 *      acc = fl(acc + fl(gain_c,i s_c,i)).  Stored as acc, or in the _pcm16 form as clip(rint(32768 acc), -32768, 32767), the rule
 *      of gtcrn_f32_to_pcm16.
 *   9. g = t for a present seat, else 0; picked += t; blocks += 1 for every seat of a live room.
 * So: a room's outputs and records depend on nothing outside its seats; a lone participant hears zeros; with no change of
 * talkers the mix is the plain ordered sum; a talker who leaves the pick fades over exactly one block.
 *
 * No load or store leaves the buffers, whatever the tables hold: a row index outside [-1, n_in) / [-1, n_out) counts as -1, a
 * seat with rec outside [0, n_rec) is ignored, a room is skipped when its d_room_start pair decreases, leaves [0, n_seats] or
 * spans more than GTCRN_MIX_MAX_ROOM seats.  A rec or an out_row named twice in one call is the caller's error: the result is
 * then unspecified for those seats only.  Output rows that no seat names are not written.
 *
 * gtcrn_mix_rooms / gtcrn_mix_rooms_pcm16 take device pointers, are asynchronous on `stream`, allocate nothing and are
 * capturable: one launch, a workgroup per room.  GTCRN_ERR_ARG before any launch: a negative count, n outside 1 .. 1024, a null
 * d_room_start, d_seats, d_rec or d_params (or row buffer with rows), a stride below n, voice_stride < 1, a misaligned pointer,
 * overlapping input and output ranges.  gtcrn_mix_rooms_host / _pcm16_host: the same arguments on host pointers, no device and
 * no stream; they run the very functions the kernel compiles (csrc/mixer.h).
 *
 * Out of scope: rooms whose legs differ in rate or packet length; G.711 bytes in and out (gtcrn_g711_to_f32 / gtcrn_f32_to_g711
 * stand either side); per-talker gains or panning; more than 8 talkers; a participant in two rooms at once. */
#define GTCRN_MIX_MAX_ROOM 1024
typedef struct gtcrn_mix_config {
    int k;                 /* talkers admitted, 1 .. 8 */
    double floor_dbov;     /* a block below it is not speech (used without d_voice) */
    double alpha;          /* release smoothing of the level, 0 .. 1 */
    double incumbent_db;   /* what a challenger must exceed a talker in the mix by, >= 0 */
} gtcrn_mix_config;
#define GTCRN_MIX_DEFAULTS {3, -50.0, 0.125, 3.0}
int gtcrn_mix_params_host(const gtcrn_mix_config *config, float *out8);
int gtcrn_mix_rooms(const float *d_in, long in_stride, int n_in, float *d_out, long out_stride, int n_out, int n,
                    const int *d_room_start, const int *d_seats, int n_seats, int R, const int *d_nrooms, float *d_rec, int n_rec,
                    const float *d_params, const float *d_voice, long voice_stride, void *stream);
int gtcrn_mix_rooms_pcm16(const short *d_in, long in_stride, int n_in, short *d_out, long out_stride, int n_out, int n,
                          const int *d_room_start, const int *d_seats, int n_seats, int R, const int *d_nrooms, float *d_rec,
                          int n_rec, const float *d_params, const float *d_voice, long voice_stride, void *stream);
int gtcrn_mix_rooms_host(const float *h_in, long in_stride, int n_in, float *h_out, long out_stride, int n_out, int n,
                         const int *h_room_start, const int *h_seats, int n_seats, int R, const int *h_nrooms, float *h_rec,
                         int n_rec, const float *h_params, const float *h_voice, long voice_stride);
int gtcrn_mix_rooms_pcm16_host(const short *h_in, long in_stride, int n_in, short *h_out, long out_stride, int n_out, int n,
                               const int *h_room_start, const int *h_seats, int n_seats, int R, const int *h_nrooms, float *h_rec,
                               int n_rec, const float *h_params, const float *h_voice, long voice_stride);

/* ---- packet loss concealment -------------------------------------------------------------------------------------------------------
 * What a gateway does to a call leg when a packet does not arrive: it makes the audio up.  A pre-pass over the rows a live step is
 * about to take (any rate, any packet form: rows of n samples, float, int16 or G.711 codes), with no handle and in no existing
 * kernel; a caller who does not conceal issues the launches they issued before.  Every leg then has a packet every tick, real or
 * synthesised, and the step, the meters, level control and the mixer run on continuous time.  The arithmetic is this project's
 * own: the ideas of G.711 Appendix I (pitch-synchronous repetition of the history, a hold, a linear fade-out, a cross-fade back
 * into the real signal) without its quarter-wavelength overlap-add and with no claim of parity.  Integer arithmetic but for one
 * stated double expression and the float cross-fade (the files are compiled with -ffp-contract=off), so that a page of numpy
 * restates outputs, histories and records bit for bit (tests/plc_checker.py).
 *
 * The 8 parameter words (int32, 16-byte aligned, read at launch) are {pmin, pmax, W, D, T0, T1, F, fs}, `div` the integer quotient:
 *   pmin = fs div 200 (shortest lag), pmax = fs 15 div 1000 (longest lag), W = fs div 50 (correlation window, 20 ms),
 *   D = max(1, fs div 8000) (stride of the coarse search), T0 = hold_ms fs div 1000 (hold), T1 = fade_ms fs div 1000 (fade-out),
 *   F = max(1, recover_ms fs div 1000) (cross-fade into the real signal);  Lh = pmax + W is the history length (at most
 *   GTCRN_PLC_MAX_HISTORY, reached at 48 kHz).
 * gtcrn_plc_params_host is the one place they are made; GTCRN_ERR_ARG with a reason for a null pointer, an fs other than 8000,
 * 16000, 22050, 24000, 32000, 44100, 48000, hold_ms outside 0 .. 200, fade_ms outside 1 .. 200, recover_ms outside 0 .. 200.
 * Defaults (GTCRN_PLC_DEFAULTS(fs)): 10, 50 and 5 ms.  Words made elsewhere turn a call into a no-op unless pmin >= 1,
 * pmin <= pmax, W >= 1, D >= 1, Lh <= min(GTCRN_PLC_MAX_HISTORY, hist_stride), 0 <= T0 <= 65536, 1 <= T1 <= 65536, F >= 1.
 *
 * Per-stream state, owned by the caller at fixed addresses, S slots of each:
 *   d_hist  int16, slot s at d_hist + s hist_stride: a ring of Lh samples.  Logical sample j (0 the oldest, Lh - 1 the newest)
 *           lives at ring[(pos + j) mod Lh]; nothing beyond Lh is read or written.
 *   d_rec   four int32 {pos, lag, erased, events}, 16-byte aligned: the ring's write position, the lag of the running (or last)
 *           erasure, the samples concealed so far in the running erasure (0: none running; saturates at T0 + T1), and the
 *           counters: events & 0xFFFF erasures, (events >> 16) & 0xFFFF lost packets, each modulo 65536.
 * A zeroed history and record are a fresh stream.  A record no call wrote is read with pos outside [0, Lh) as 0, lag clamped to
 * [pmin, pmax], erased clamped to [0, T0 + T1].
 *
 * One call: d_x holds M rows of n samples (1 <= n <= 1024) at `stride`; row i belongs to slot d_slots[i] (d_slots NULL: slot i);
 * d_lost[i] != 0 says that the packet did not arrive, and the row's contents are then ignored; d_count (may be NULL) is a device
 * word: rows at or beyond *d_count are skipped.  Rows that are skipped and slots that are not named are not touched in any array;
 * a slot id outside [0, S) makes its row a no-op.  A slot named twice in one call is the caller's error: the result is then
 * unspecified for that slot only.  Per row, with h the history in logical order and `int16 of` a sample: the sample itself,
 * pcm_of(x) = clip(rint(32768 x), -32768, 32767) (the rule of gtcrn_f32_to_pcm16; a NaN gives -32768), or D_law[code] of
 * "G.711 payloads":
 *   1. received, erased = 0: the row is not written (it stays bit for bit, NaN and Inf included).  The history takes the int16 of
 *      every sample: appending n samples writes sample j to ring[(pos + j) mod Lh] for j >= max(0, n - Lh) (a row longer than
 *      the history leaves its last Lh samples) and sets pos = (pos + n) mod Lh.  Only pos of the record is written.
 *   2. lost, erased = 0 (an erasure begins): m = max |h_j|, s = max(0, bitlength(m) - 10), a_j = h_j >> s (arithmetic), so that
 *      every product is below 2^20 and every sum below 2^30.  For a lag p and a stride d, over i = 0, d, 2d, ... < W:
 *      c = sum a[Lh-1-i] a[Lh-1-i-p], e = sum a[Lh-1-i-p]^2 (int32), score = (c > 0 and e > 0) ?
 *      fl64(fl64(double(c) double(c)) / double(e)) : 0.  Coarse: p = pmin, pmin + D, ... <= pmax at stride D; the largest score
 *      wins, among equal scores the smallest lag, and only a score > 0 can win.  No winner (silence, a fresh stream): lag = pmax.
 *      Otherwise refine over max(pmin, p0 - D + 1) .. min(pmax, p0 + D - 1) at stride 1 by the same rule; no winner there: lag = p0.
 *   3. lost (after 2, or erased > 0): s_i = h[Lh - lag + (i mod lag)], t = erased + i, g(t) = 32768 for t < T0, 0 for t >= T0 + T1,
 *      else 32768 - ((t - T0) 32768) div T1; o_i = (s_i g(t) + 16384) >> 15.  The row is written as o_i (int16), fl(o_i / 32768)
 *      (float, exact) or E_law(o_i).  The history takes s, not o (it holds the unattenuated continuation, so a longer erasure
 *      needs no recursion).  erased = min(erased + n, T0 + T1); events: lost packets + 1, and erasures + 1 after step 2.
 *   4. received, erased > 0 (recovery): f = min(F, n); for i < f: r_i = ((i + 1) 32768) div f, sa_i step 3's o_i;
 *      int16: o = (x r + sa (32768 - r) + 16384) >> 15; G.711: the same on x = D_law[code], stored as E_law(o) (so the f faded
 *      samples are re-encoded; at r = 32768 o = x); float: o = fl(fl(x rf) + fl(saf fl(1 - rf))) with the exact rf = r / 32768,
 *      saf = sa / 32768.  The rest of the row is not written.  The history takes the int16 of the row as written; erased = 0.
 * So: no added latency; a stream depends on nothing outside its own row, history and record; the cut of a clip into packets
 * matters (packets are the units of loss), the grouping of rows into calls does not; a non-finite float sample stays in its own
 * stream and enters that stream's history as an int16 like any other.
 *
 * gtcrn_plc_rows / _pcm16 / _g711 take device pointers, are asynchronous on `stream`, allocate nothing and are capturable: one
 * launch, a wave per row.  gtcrn_plc_reset zeroes the histories (Lh samples) and records of the named slots (d_slots NULL: slots
 * 0 .. M - 1) below *d_count, in one launch of its own: a stream joins a captured tick through it.  GTCRN_ERR_ARG before any launch:
 * a negative count, n outside 1 .. 1024, a null d_lost, d_hist, d_rec or d_params (or row buffer with rows), a stride below n,
 * hist_stride < 1, a law other than 0 / 1, a misaligned pointer.  gtcrn_plc_rows_host / _pcm16_host / _g711_host: the same
 * arguments on host pointers, no device and no stream; they run the very functions the kernel compiles (csrc/plc.h).
 *
 * Out of scope: parity with G.711 Appendix I or any codec's own concealment; concealment on the output side; jitter buffering
 * and reordering (d_lost is their result); comfort noise in long erasures; a new pitch estimate inside an erasure; the offline
 * forward_wave calls. */
#define GTCRN_PLC_MAX_HISTORY 1680
typedef struct gtcrn_plc_config {
    int fs;                /* 8000, 16000, 22050, 24000, 32000, 44100 or 48000 */
    int hold_ms;           /* full level for this long, 0 .. 200 */
    int fade_ms;           /* then a linear fade to zero over this long, 1 .. 200 */
    int recover_ms;        /* cross-fade into the first received packet, 0 .. 200 (at least one sample) */
} gtcrn_plc_config;
#define GTCRN_PLC_DEFAULTS(fs) {(fs), 10, 50, 5}
int gtcrn_plc_params_host(const gtcrn_plc_config *config, int *out8);
int gtcrn_plc_rows(float *d_x, long stride, int M, int n, const int *d_slots, const int *d_lost, const int *d_count, short *d_hist,
                   long hist_stride, int *d_rec, int S, const int *d_params, void *stream);
int gtcrn_plc_rows_pcm16(short *d_x, long stride, int M, int n, const int *d_slots, const int *d_lost, const int *d_count,
                         short *d_hist, long hist_stride, int *d_rec, int S, const int *d_params, void *stream);
int gtcrn_plc_rows_g711(unsigned char *d_x, long stride, int M, int n, const int *d_slots, const int *d_lost, const int *d_count,
                        short *d_hist, long hist_stride, int *d_rec, int S, const int *d_params, int law, void *stream);
int gtcrn_plc_reset(short *d_hist, long hist_stride, int *d_rec, int S, const int *d_params, const int *d_slots, int M,
                    const int *d_count, void *stream);
int gtcrn_plc_rows_host(float *h_x, long stride, int M, int n, const int *h_slots, const int *h_lost, const int *h_count, short *h_hist,
                        long hist_stride, int *h_rec, int S, const int *h_params);
int gtcrn_plc_rows_pcm16_host(short *h_x, long stride, int M, int n, const int *h_slots, const int *h_lost, const int *h_count,
                              short *h_hist, long hist_stride, int *h_rec, int S, const int *h_params);
int gtcrn_plc_rows_g711_host(unsigned char *h_x, long stride, int M, int n, const int *h_slots, const int *h_lost, const int *h_count,
                             short *h_hist, long hist_stride, int *h_rec, int S, const int *h_params, int law);

/* ---- standalone streaming conv wrappers -----------------------------------
 * Replaces StreamConv2d.forward / StreamConvTranspose2d.forward
 * (streaming/conversion/convolution.py:107-119, 201-253): out = conv(cat([cache, x], time)),
 * cache_out = last (kt-1)*dt rows of the input.  x (B,Cin,T,F), cache (B,Cin,(kt-1)*dt,F),
 * y (B,Cout,T,Fout); stride 1, time padding 0 (causal), frequency padding pad_f.
 * transposed = 0: Conv2d weight (Cout, Cin/groups, kt, kf);
 * transposed = 1: ConvTranspose2d weight (Cin, Cout, kt, kf) as stored by the OFFLINE module
 * (the permute + flip of convert.py:35-48 is implied).  Returns Fout (> 0) or a negative status. */
int gtcrn_stream_conv2d(const float *d_x, const float *d_cache, const float *d_w, const float *d_bias,
                        float *d_y, float *d_cache_out, int B, int Cin, int Cout, int T, int F, int kt, int kf,
                        int dt, int df, int pad_f, int groups, int transposed, void *stream);

/* ---- host-side packer view (no device needed) ---------------------------
 * The BatchNorm-folded "slot space" buffers the kernels consume, as produced
 * from a parameter blob; lets a CPU test check the weight contract
 * (convert_to_stream's permute/flip, streaming/conversion/convert.py:35-48,
 * and the shuffle renaming) without a GPU. */
void gtcrn_pack_sizes(long *n_floats, long *n_ints);
int gtcrn_pack_params_host(const float *h_params, long n_floats, float *h_f, int *h_i);

/* ---- test hooks ---------------------------------------------------------
 * Stage boundaries of the most recent gtcrn_forward_spec call, converted to
 * the reference's (C,T,F) layout and logical channel order, for batch item b.
 * Names: en0..en4, gtcn1, gtcn2, de0..de4 (de* need gtcn_debug_enable(m,1)
 * before the forward).  Returns element count, or a negative status. */
/* on = 2 (diagnostic build): phase stamps only -- a single-frame streaming step stays the ONE-launch form (its
 * stamps land in kernel slot 0 of gtcrn_debug_stamps, one row per workgroup of four streams). */
int gtcrn_debug_enable(gtcrn_model *m, int on);
/* Variable-length batches (gtcrn_forward_wave_var) of B <= 1024 utterances that are not whole rounds of 256 run the
 * per-utterance kernels in time spans: 256-workgroup rounds share the frames that exist, so a folder of a few dozen
 * files fills the chip.  Results are bit-identical either way; on = 0 goes back to one workgroup per utterance (the A/B
 * switch of tests and measurements).  Default on. */
int gtcrn_var_spans_enable(gtcrn_model *m, int on);
/* Single-frame streaming steps (gtcrn_stream_step with nframes == 1): form 0 (default) runs the whole step as ONE
 * kernel, nothing handed over through HBM -- four streams per workgroup (k_stream_ms) while one round of workgroups
 * covers the streams, seven per workgroup (k_stream_wide: eight waves x two tiles, parameters streamed through LDS)
 * once the stream count fills the chip more than once; form 1 runs the three-launch form (encoder, both GTCN stacks,
 * decoder; hand-off tensors in HBM) that the stage taps use; forms 2 and 3 pin the one-launch step to four / seven
 * streams per workgroup whatever the count.  Bit-identical outputs and ring state in every form
 * (tests/test_gpu_stream.py); the A/B switch of the capacity measurements. */
int gtcrn_stream_form(gtcrn_model *m, int form);
/* Which one-launch form the default (form 0) runs for `nstreams` single-frame steps: the streams per workgroup, 4
 * (k_stream_ms) or 7 (k_stream_wide).  Pure host logic (no device is touched): both forms run one workgroup per CU, so a
 * step costs rounds-of-256-workgroups x the form's time per round (32.9 us against ~1.5 x that); the wide form is taken
 * once the narrow one needs more rounds than it. */
int gtcrn_stream_streams_per_workgroup(int nstreams);
long gtcrn_debug_tap(gtcrn_model *m, const char *name, int b, float *h_dst, long cap);
/* The 16 kHz hand-off of the most recent gtcrn_rate_stream_step, copied to d_dst (n floats: nstreams rows of
 * 256 * nhops) on `stream`: which = 0 what k_rate_in handed to the wave step, 1 what the wave step handed to
 * k_rate_out.  Returns n, or a negative status. */
long gtcrn_rate_stream_debug_handoff(gtcrn_model *m, int which, float *d_dst, long n, void *stream);
/* The same for the most recent gtcrn_packet_stream_step: nstreams rows of 256 h floats, h the hops that step ran (n at
 * most nstreams * 256 * h; GTCRN_ERR_STATE when the step ran no hop): which = 0 what k_packet_in handed to the wave
 * step, 1 what the wave step handed to k_packet_out. */
long gtcrn_packet_stream_debug_handoff(gtcrn_packet_stream *ps, int which, float *d_dst, long n, void *stream);
/* Diagnostic build only (libgtcrn_micro_hip_stamps.so, -DGT_STAMPS): per-workgroup sums of shader
 * cycles spent in each barrier-delimited phase of kernel 0 encoder, 1 gtcn1, 2 gtcn2, 3 decoder,
 * (B,16) values.  The product library returns zeros. */
long gtcrn_debug_stamps(gtcrn_model *m, int kernel, unsigned long long *h_dst, long cap);
/* Checks the MFMA f32 16x16x4 lane maps the kernels rely on (exact integer
 * data, asymmetric operands).  0 = as assumed. */
/* 16-bit PCM at the host boundary: the reference's callers read mono 16-bit WAV files with soundfile (infer.py:54: the
 * samples arrive as int16 / 32768) and write the enhanced waveform back as 16-bit PCM (infer.py:113, sf.write).  A caller
 * that hands the int16 SAMPLES over moves half the bytes across the host link, which is what bounds a served pipeline
 * (bench.py io.served_pcm16_*).  gtcrn_pcm16_to_f32: x = s / 32768 (exact); gtcrn_f32_to_pcm16: s = clip(rint(y * 32768),
 * -32768, 32767), round half to even.  Device pointers, 16-byte aligned; n samples, a multiple of 8; asynchronous on
 * `stream`.  The bulk offline driver (gtcrn_micro_amd/infer.py) uses both. */
int gtcrn_pcm16_to_f32(int device, const short *d_pcm, float *d_wave, long n, void *stream);
int gtcrn_f32_to_pcm16(int device, const float *d_wave, short *d_pcm, long n, void *stream);
int gtcrn_selftest_mfma(int device);
/* The same for v_mfma_i32_16x16x64_i8, the instruction of gtcrn_batch_reverb's matrix form: asymmetric full-range int8
 * operands and a non-zero C, every element of D compared with the integer product.  0 = as assumed. */
int gtcrn_selftest_mfma_i8(int device);
/* The exact three-way bf16 split the dense 3x3 runs on (kernels.hip split3 / join3 / split_mm6), on caller-chosen
 * values: h_x[n] (n a multiple of 4) -> h_planes[3][n] (hi, mid, lo as floats) and h_joined[n] (= h_x bit for bit
 * wherever all three planes are normal numbers); optionally h_A (16x32, row major) * h_B (32x16) -> h_D (16x16)
 * through the same six-product helper the kernels use, from operands split on the device.  Host pointers. */
int gtcrn_selftest_split3(int device, const float *h_x, long n, float *h_planes, float *h_joined, const float *h_A,
                          const float *h_B, float *h_D);
/* HIP-event timing of every kernel launch (events recorded on the call's stream, no
 * synchronisation inside the timed region).  gtcrn_timing_enable(m,1) clears the record;
 * gtcrn_timing_read returns, for kernel idx in [0, gtcrn_timing_kernels()) -- every timed launch records which
 * kernel it was, so offline and streaming calls keep their own rows (k_front, k_encoder_gt, k_gtcn1, k_gtcn2,
 * k_decoder, k_istft offline; k_stream_ms / k_stream_wide for single-frame streaming steps; ...) -- its name, the average device time
 * in ms over the launches recorded since and their count.  idx = -1 - k only returns the name of kernel k (m may be
 * NULL).  on = 2 + idx records events around kernel idx ONLY: every event pair costs a few microseconds of dispatch
 * gap, so the timed region of bench.py keeps just the dominant kernel's.  Used for the roofline line. */
int gtcrn_timing_enable(gtcrn_model *m, int on);
int gtcrn_timing_kernels(void);
int gtcrn_timing_read(gtcrn_model *m, int idx, char *name, int name_cap, float *ms, int *launches);

/* ---- train step (model forward/backward) ---------------------------------
 * Replaces: `enhanced = self.model(noisy_spec)` with the module in .train() mode and the model part
 * of `loss.backward()` (train.py:265, 280; models/gtcrn_micro.py:506-532).  Every nn.BatchNorm2d
 * normalises with the statistics of the batch and updates its running estimates in place
 * (momentum 0.1, unbiased variance), exactly as nn.BatchNorm2d.train() does; the transposed
 * depth convs of the decoder produce T+2 frames whose tail takes part in the statistics
 * (models/gtcrn_micro.py:238-251).  The loss, the optimiser and the scheduler stay with the caller
 * (PyTorch; train.py:267-288).
 *
 * d_params: the canonical blob (GTCRN_NPARAM_FLOATS floats, raw, NOT folded) in device memory; the
 *   forward writes the new running_mean/running_var into it.
 * d_grads:  same layout; the backward writes d loss / d parameter for the 248 trainable tensors and
 *   zeros in the slots of buffers (running statistics, ERB filterbank).
 * Spectrograms are addressed by strides like gtcrn_forward_spec.  The backward differentiates the
 * most recent forward of this trainer (same d_params, same d_spec).  One trainer per device,
 * single caller thread (train.py:461-471); no CPU fallback. */
typedef struct gtcrn_trainer gtcrn_trainer;
int gtcrn_trainer_create(gtcrn_trainer **out, int device);
void gtcrn_trainer_destroy(gtcrn_trainer *t);
long gtcrn_train_workspace_bytes(int B, int T);   /* saved activations + gradient buffers (fp32 storage) */
/* Storage of the SAVED activations (everything the backward re-reads): 0 = fp32, the reference's own precision
 * (train.py:239-288 trains in fp32); 1 = bf16 (BASELINE configs[3] asks for bf16: half the bytes of every pass of the
 * HBM-bound layer-at-a-time step; the forward then IS the bf16-activation network: its consumers read the rounded
 * values); 4 = bf16 SAVES with an exact forward chain: every forward tensor is written twice -- the fp32 value the next
 * layer reads and the bf16 copy the backward re-reads -- so the output equals mode 0's bit for bit and the gradient
 * differs from mode 0's only by the rounding of the saved tensors, at mode 1's workspace (the fp32 buffers of the chain
 * are short-lived and share the backward's scratch region); 5 = mode 1 with the gradient tensors handed from one
 * unit's backward to the next stored in bf16 as well (what bf16 autocast training keeps: the forward is mode 1's bit for
 * bit; a unit rounds the gradient it hands on where it stores it).  Arithmetic, BatchNorm statistics and reductions,
 * every PARAMETER gradient, the gradient all-reduce, Adam and the master weights stay fp32 in all modes.  Takes effect
 * at the next forward. */
int gtcrn_trainer_set_storage(gtcrn_trainer *t, int storage);
/* Workspace of a (B, T) problem in `storage` with the DEFAULT fusion mask (every pass fusion on).  A trainer whose mask
 * was changed with gtcrn_trainer_set_fusions stores more tensors (about 6 GiB more at B = 512 with mask 7):
 * gtcrn_trainer_workspace_bytes plans with the trainer's own storage mode and mask. */
long gtcrn_train_workspace_bytes2(int B, int T, int storage);
long gtcrn_trainer_workspace_bytes(gtcrn_trainer *t, int B, int T);
/* Diagnostic: which pass fusions of the train step are active (default: all).  bit 0: BatchNorm + PReLU of a unit
 * applied by the conv that consumes it (normalise-on-load; the forward is bit-identical with and without), bit 1: the
 * depthwise unit's backward in one pass, bit 2: BatchNorm reductions accumulated by the kernel that produces their
 * gradient input, bit 3 (needs bits 0 and 2): an activation whose only readers are a normalise-on-load conv and that
 * conv's fused backward is not stored -- the backward recomputes it from the conv output it reads anyway (22 of the 46
 * units: one tensor write less in the forward, one read less in the backward, 6 GiB less workspace at B = 512).
 * bit 4: the two gradients every encoder output receives (decoder skip + main path) are summed by accumulating stores
 * of the kernels that produce the second one, not by five add passes.  bit 5 (needs bit 2): the reductions of
 * point_conv1 (six blocks) and en_convs.0 ride in the adjoint conv that produces their gradient input.  bit 6: the
 * backward of the encoder's depthwise 3x3 unit (dy, weight gradient, data gradient) in one LDS-tiled pass.  bit 7: the
 * same for the decoder's dense transposed 3x3 unit (both matrix products from LDS images of dy and x).  bit 8 (needs bit
 * 0): point_conv1's BatchNorm + PReLU applied by LDS-tiled depth convs while they stage their input tile.  bit 9: the
 * backward of the two 16 -> 16 (1,5) stride-2 units (en_convs.1, de_convs.3) from LDS tiles.  bit 10: the second
 * stage of every BatchNorm reduction (forward statistics + running estimates; backward means, dgamma, dbeta, dslope) runs
 * in the LAST workgroup of the kernel that produces the per-workgroup sums (two-level last-arriver reduction, agent-scope
 * write-through hand-off, fixed summation order) instead of 92 one-workgroup finish launches per step.  bit 11 (not
 * in storage mode 4): each of the decoder's five sums x + en_outs[..] (models/gtcrn_micro.py:463-469) is written by the layer
 * that produces x (the last TCN block's normalise pass, the decoder blocks' gate/shuffle, de_convs.3's normalise pass)
 * instead of an add pass; x itself is not stored (its test tap is sum - skip); in the 16-bit modes x is rounded to
 * the storage format before the add, as the stored x was, and the backward no longer recomputes the sums.  bit 12 (needs bit 0; not in storage
 * mode 4): point_bn2 -- the one BatchNorm with no activation behind it -- is applied on load by its four readers
 * (TRALite's energy, the gate/shuffle, their two backward passes): six normalise passes per step and the tensor they
 * wrote are gone, the values are the same bit for bit.  bit 13: the 28 pointwise forward convs of a step run in a
 * dedicated kernel (flat positions, compile-time formats, two tiles per iteration with the next two requested) instead of
 * the general strided / padded conv kernel (and the two 16 -> 16 (1,5) stride-2 layers in one of their own, k_c15_fwd).  bit 14: the TCN's dilated depthwise (3,1) forward in a column form -- a
 * thread walks one residue class of frames modulo the dilation, so every input is normalised once instead of three
 * times and a chunk's loads are issued together.  Both are bit-identical to the kernels they replace (conv outputs;
 * the BatchNorm statistics to the float); bit 14 also runs that unit's fused backward in the column form (dy and the
 * recomputed activation once per element; sums in another order).  bit 15: the weight-gradient finishes of a backward
 * pass (44 small launches) are recorded and run as two batched launches at its end, partial sums in a pool (same sums,
 * same order: bit-identical gradients).  Default 65535.
 * 0 runs the layer-at-a-time passes (tests/test_gpu_train.py compares them).  Takes effect at the next forward; not
 * part of the reference's interface. */
int gtcrn_trainer_set_fusions(gtcrn_trainer *t, int mask);
int gtcrn_train_forward(gtcrn_trainer *t, float *d_params, const float *d_spec, long sb, long sf, long st,
                        float *d_out, long ob, long of, long ot, int B, int T, void *stream);
int gtcrn_train_backward(gtcrn_trainer *t, const float *d_params, const float *d_spec, long sb, long sf,
                         long st, const float *d_grad_out, long gb, long gf, long gt, float *d_grads,
                         void *stream);
/* HybridLoss (loss.py:30-71): 30 * (MSE of the 0.3-compressed real and imaginary parts) + 70 * MSE of the
 * compressed magnitudes + SI-SNR of the sqrt-Hann iSTFTs, batch mean.  d_loss receives one float; d_grad
 * (optional) the gradient w.r.t. d_pred as a contiguous (B,257,T,2) tensor.  Replaces
 * `loss = self.loss_func(enhanced, clean_spec)` and the loss part of `loss.backward()` (train.py:267, 280). */
int gtcrn_train_loss(gtcrn_trainer *t, const float *d_pred, long pb, long pf, long pt, const float *d_true, long tb,
                     long tf, long tt, int B, int T, float *d_loss, float *d_grad, void *stream);
/* The same with the gradient addressed by strides (gb, gf, gt) like the spectrograms: a caller that keeps its
 * spectrograms frame-major -- (B,257,T,2)-shaped views of (B,T,257,2) memory, which every kernel of the step then reads
 * and writes in 2 KB rows -- gets the gradient in that layout too. */
int gtcrn_train_loss_strided(gtcrn_trainer *t, const float *d_pred, long pb, long pf, long pt, const float *d_true,
                             long tb, long tf, long tt, int B, int T, float *d_loss, float *d_grad, long gb, long gf,
                             long gt, void *stream);
/* Test hook: the per-utterance SI-SNR terms -log10(|s|^2 / (|yp - s|^2 + 1e-8) + 1e-8) of the most recent loss call
 * on this trainer (B doubles, host memory; B must be that call's), whose batch mean went into the loss.  Valid until the
 * trainer's next call of any kind; `stream` must be the loss call's.  Synchronises the stream. */
int gtcrn_train_loss_terms(gtcrn_trainer *t, double *h_terms, int B, void *stream);
/* clip_grad_norm_ + Adam over flat blobs in two launches.  Replaces `torch.nn.utils.clip_grad_norm_(self.model.parameters(),
 * clip_grad_norm_value)` + `self.optimizer.step()` (train.py:282-285; Adam(lr) from train.py:90, conf/cfg_train_DNS3.yaml
 * clip 3.0) for a model whose parameters, gradients and Adam moments are views of four blobs in the canonical layout
 * (PyTorch walks the 248 views: ~300 launches per step): total 2-norm of the masked gradient (double accumulation,
 * fixed order), gradients scaled in place by min(max_norm / (norm + 1e-6), 1) (max_norm <= 0: no clipping), then
 * torch.optim.Adam's update (no amsgrad; L2 weight_decay added to the gradient; bias corrections from `step` >= 1 in
 * double) of every element with d_mask != 0.  d_norm_out (optional, 2 floats): the total norm clip_grad_norm_ returns,
 * and the clip coefficient.  d_workspace: gtcrn_clip_adam_workspace_bytes(n) bytes of device memory, zeroed ONCE by the
 * caller (it holds the norm's last-workgroup ticket, which every call leaves at zero).  The learning-rate schedule stays
 * with the caller (utils/scheduler.py is host scalar arithmetic).  Asynchronous on `stream`. */
long gtcrn_clip_adam_workspace_bytes(long n);
int gtcrn_clip_adam_step(int device, float *d_params, float *d_grads, float *d_exp_avg, float *d_exp_avg_sq,
                         const float *d_mask, long n, float max_norm, double lr, double beta1, double beta2, double eps,
                         double weight_decay, long step, float *d_norm_out, void *d_workspace, void *stream);
/* Test hook: a tensor the most recent forward stored, valid until the next backward: the stage boundaries
 * en0..en4, tcn0..tcn7 (the output of each TCN block; tcn3 / tcn7 are gtcn1 / gtcn2), de0..de4; the
 * decoder sums sum0..sum4 (the input x + skip of de_convs.0..4, as stored: in the 16-bit modes without
 * fusion bit 11 one shared buffer holds them, so only sum4 is there; none in storage mode 4); and every
 * unit's stored conv output y as "<its BatchNorm's parameter prefix>.y" (e.g. gtcn1.blocks.2.bn2.y,
 * encoder.en_convs.3.point_bn1.y) -- in the bf16 modes the centred copy bf16(y - shift) exactly, with no
 * shift added back.  Channels-last (B, T, F, C) in the reference's channel order; shape4 receives the four
 * extents; d_out may be NULL to query the shape.  With fusion bit 11 a block output stored only inside a
 * sum (gtcn2 / tcn7, de0..de3) is returned as sum - skip. */
int gtcrn_train_tap(gtcrn_trainer *t, const char *name, float *d_out, long *shape4, void *stream);

#ifdef __cplusplus
}
#endif
#endif
