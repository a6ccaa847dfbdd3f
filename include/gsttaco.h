/*
 * gsttaco.h -- C-ABI of the MI355X-native GST-Tacotron inference hot path.
 *
 * The reference (CODEJIN/GST_Tacotron, TF2/Keras) has no FFI/plugin interface: its
 * boundary is the Python class GST_Tacotron (reference Model.py:37) and
 * Hyper_Parameters.json.  This header is what a binding for that class calls instead
 * of the Keras functional model `model_Dict['Inference']` (reference Model.py:145-156):
 *
 *   gsttaco_create / gsttaco_load_weight / gsttaco_finalize_weights
 *       <- GST_Tacotron.__init__ + Model_Generate + Restore   (Model.py:38-40, 42-189, 267-276)
 *   gsttaco_inference_step
 *       <- GST_Tacotron.Inference_Step                        (Model.py:249-255)
 *   gsttaco_encode      <- Modules/Taco2.py:12-51   Encoder.call
 *   gsttaco_gst         <- Modules/GST.py:91-109    Style_Token_Layer.call
 *                          (== GST_Tacotron.Inference_GST_Step, Model.py:257-265)
 *   gsttaco_gst_ex / gsttaco_style_compose / gsttaco_inference_step_styled
 *                       <- EXTENSION (style control, DESIGN row A14): the attention weights the reference computes and drops
 *                          (GST.py:105), the layer's last stage on GIVEN weights (Layers.py:207-211), and Inference_Step on a
 *                          GIVEN style embedding
 *   gsttaco_decode      <- Modules/Taco2.py:153-228 Decoder.call loop (training=False),
 *                          Decoder_Step :96-120, Prenet :262-283,
 *                          Modules/Attention/Steps.py:107-229 (BMA / SMA)
 *   gsttaco_decode_forced / gsttaco_inference_step_forced / gsttaco_forced_durations
 *                       <- the same loop's training=True branch (Taco2.py:161,185: step t consumes mels[:, t*r]) for GTA mels and forced
 *                          alignments; the per-token frame counts are an EXTENSION
 *   gsttaco_fill_randomness / gsttaco_utterance_report
 *                       <- EXTENSION (DESIGN row A16): randomness that depends on an utterance's own seed alone, and the stop test of
 *                          Model.py:380,413 with alignment diagnostics per utterance on the device
 *   gsttaco_losses / gsttaco_feature_frontend
 *                       <- EXTENSION (DESIGN row A17): the four loss terms of Train_Step (Model.py:210-241) of a teacher-forced pass, per
 *                          utterance on the device, and the mel plus the linear spectrogram target (Audio.py:18-21) from one STFT
 *   gsttaco_mel_dtw     <- EXTENSION (DESIGN row A18): the free-run metric, mel-cepstral distortion along a dynamic-time-warping path
 *                          between synthesised and reference mels of different lengths, per utterance on the device
 *   gsttaco_resample    <- EXTENSION (DESIGN row A19): librosa.core.load's 'kaiser_best' resampling of reference audio at another rate
 *                          (Pattern_Generator.py:40-43), batched on the device ahead of gsttaco_mel_frontend
 *   gsttaco_postnet     <- Modules/Taco2.py:131-149, 230
 *   gsttaco_vocoder     <- Modules/Taco2.py:234-260 Vocoder_Taco1.call, CBHG :285-380
 *   gsttaco_mel_frontend <- Pattern_Generator.py:39-60 Mel_Generate + Audio.py:29-32,49-55,70-96 melspectrogram
 *                          + the batch layout of Feeder.py:204-225 / 229-250
 *   gsttaco_griffin_lim <- Audio.py:23-27 inv_spectrogram, :57-68 _griffin_lim, :74-75 _istft (SURVEY row N4;
 *                          called from Model.py:414-422 Export_Inference)
 *   gsttaco_mel_basis   <- Audio.py:81-83 _build_mel_basis (librosa.filters.mel); host-side getter for tests
 *
 * Conventions
 *   - every function returns 0 on success or a negative GSTTACO_E_* code; nothing throws
 *     across the ABI; gsttaco_last_error() returns a message for the last failure.
 *   - tensor arguments are DEVICE pointers (HIP) owned by the caller, dense row-major,
 *     innermost dimension contiguous, float32 unless stated; weights are HOST pointers.
 *   - all work is enqueued on the given hipStream_t (passed as void*); no implicit sync.
 *   - one ctx per device; a ctx is not thread-safe; distinct ctxs are independent.
 *   - there is NO CPU fallback: without a gfx950 device every compute call fails with
 *     GSTTACO_E_NO_DEVICE.
 */
#ifndef GSTTACO_H
#define GSTTACO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSTTACO_ABI_VERSION 14
#define GSTTACO_MAX_LAYERS 8

enum {
    GSTTACO_OK = 0,
    GSTTACO_E_INVALID = -1,     /* bad argument / unsupported configuration */
    GSTTACO_E_NO_DEVICE = -2,   /* no HIP device (the product path has no CPU fallback) */
    GSTTACO_E_HIP = -3,         /* a HIP runtime call failed */
    GSTTACO_E_WEIGHTS = -4,     /* missing / mis-shaped weight, or weights not finalized */
    GSTTACO_E_CAPACITY = -5     /* batch / tokens / frames exceed the capacity given at create */
};

/* BMA / SMA: reference Taco2.py:66-75.  LSA: EXTENSION -- step-wise restatement of LocationSensitiveAttention
 * (reference Modules/Attention/Layers.py:289-444), which the reference decoder cannot select. */
enum { GSTTACO_ATT_BMA = 0, GSTTACO_ATT_SMA = 1, GSTTACO_ATT_LSA = 2 };

/* Mirrors the hot-path keys of Hyper_Parameters.json (reference file of that name). */
typedef struct gsttaco_config {
    int32_t abi_version;        /* GSTTACO_ABI_VERSION */
    int32_t device;             /* HIP device ordinal */
    /* Sound / loop */
    int32_t mel_dim;            /* Sound.Mel_Dim */
    int32_t step_reduction;     /* Step_Reduction */
    int32_t max_step;           /* Max_Step (decoder runs Max_Step // Step_Reduction iterations, Taco2.py:213) */
    /* Tacotron2.Encoder */
    int32_t vocab;              /* len(Token_Index_Dict) */
    int32_t emb;                /* Embedding.Size */
    int32_t n_enc_conv;
    int32_t enc_filters[GSTTACO_MAX_LAYERS];
    int32_t enc_kernels[GSTTACO_MAX_LAYERS];
    int32_t enc_rnn;            /* RNN.Size (per direction) */
    /* Tacotron2.Decoder */
    int32_t n_prenet;           /* must be 2 */
    int32_t prenet[GSTTACO_MAX_LAYERS];
    float   prenet_rate;        /* Prenet.Dropout_Rate -- live at inference (Taco2.py:283) */
    int32_t n_dec_rnn;          /* must be 2 */
    int32_t dec_rnn[GSTTACO_MAX_LAYERS];
    int32_t att_type;           /* GSTTACO_ATT_* */
    int32_t att_size;           /* Attention.Size */
    float   sigmoid_noise;      /* SMA 2.0 (Steps.py:212), BMA 0.0 (Steps.py:58) */
    int32_t loc_filters;        /* LSA only: Attention.Conv.Filters      (Layers.py:314-319) */
    int32_t loc_kernel;         /* LSA only: Attention.Conv.Kernel_Size */
    int32_t lsa_cumulate;       /* LSA only: cumulate_weights (Layers.py:302, default 1) */
    int32_t lsa_smoothing;      /* LSA only: smoothing normalisation instead of softmax (Layers.py:300, 426-444) */
    int32_t n_post;             /* len(Decoder.Conv.Filters)+1 */
    int32_t post_filters[GSTTACO_MAX_LAYERS];
    int32_t post_kernels[GSTTACO_MAX_LAYERS];
    int32_t post_tanh;          /* number of leading postnet layers followed by tanh (Taco2.py:145) */
    /* GST */
    int32_t gst_use;
    int32_t n_ref_conv;
    int32_t ref_filters[GSTTACO_MAX_LAYERS];
    int32_t ref_kernels[GSTTACO_MAX_LAYERS];
    int32_t ref_strides[GSTTACO_MAX_LAYERS];
    int32_t ref_rnn;            /* Reference_Encoder.RNN.Size */
    int32_t ref_dense;          /* Reference_Encoder.Dense.Size */
    int32_t n_tokens;           /* Style_Token.Size */
    int32_t token_emb;          /* Style_Token.Embedding.Size */
    int32_t heads;              /* Style_Token.Attention.Head */
    int32_t gst_att;            /* Style_Token.Attention.Size */
    /* Vocoder_Taco1 (CBHG mel -> linear spectrogram, reference Taco2.py:234-260, 285-424); optional */
    int32_t voc_use;            /* 0: no vocoder weights / entry point */
    int32_t spec_dim;           /* Sound.Spectrogram_Dim */
    int32_t bank_count;         /* CBHG.Conv_Bank.Stack_Count (kernel sizes 1..count) */
    int32_t bank_filters;       /* CBHG.Conv_Bank.Filters */
    int32_t n_voc_proj;
    int32_t voc_proj_filters[GSTTACO_MAX_LAYERS];
    int32_t voc_proj_kernels[GSTTACO_MAX_LAYERS];
    int32_t highway_count;
    int32_t highway_size;
    int32_t voc_rnn;            /* CBHG.RNN.Size (per direction) */
    /* Sound: audio front end (wav -> mels_for_gst) and back end (spectrogram -> wav, row N4); optional */
    int32_t sample_rate;        /* Sound.Sample_Rate */
    int32_t frame_length;       /* Sound.Frame_Length (STFT window, <= n_fft = 2 * (Spectrogram_Dim - 1)) */
    int32_t frame_shift;        /* Sound.Frame_Shift (hop) */
    float   max_abs_mel;        /* Sound.Max_Abs_Mel; 0 = the [0,1] normalisation (Audio.py:92-93) */
    int32_t max_wav_samples;    /* capacity of the audio entry points per utterance; 0 = disabled */
    /* Use_Mixed_Precision (reference Model.py:31-35 selects Keras mixed_float16; here: bf16 GEMM operands, fp32 accumulation,
     * fp32 state / epilogues / outputs -- BASELINE configs[4]).  0 = everything fp32 (the parity path). */
    int32_t mixed_precision;
    /* capacity: workspace is sized once, at finalize */
    int32_t max_batch;
    int32_t max_tokens;
    int32_t max_ref_frames;     /* frames of mels_for_gst INCLUDING the prepended zero frame */
} gsttaco_config;

typedef struct gsttaco_ctx gsttaco_ctx;

int gsttaco_abi_version(void);

/* Validates cfg and creates a context.  Does not touch the GPU (so the host logic is
 * testable without one); the device is first used by gsttaco_finalize_weights. */
int gsttaco_create(const gsttaco_config* cfg, gsttaco_ctx** out);
void gsttaco_destroy(gsttaco_ctx* ctx);
const char* gsttaco_last_error(const gsttaco_ctx* ctx);   /* ctx may be NULL: last create error */

/* Weight manifest (names/shapes in the TF variable layouts). */
int gsttaco_num_weights(const gsttaco_ctx* ctx);
int gsttaco_weight_info(const gsttaco_ctx* ctx, int index, const char** name, int64_t shape[4], int* ndim);
/* Copies one tensor (HOST float32 pointer) into the context. */
int gsttaco_load_weight(gsttaco_ctx* ctx, const char* name, const float* host_data,
                        const int64_t* shape, int ndim);
/* BN folding, MFMA-fragment repack, upload to HBM, workspace allocation. */
int gsttaco_finalize_weights(gsttaco_ctx* ctx);

/* Masked mode (EXTENSION): the reference has no padding masks -- `token_lengths` is accepted by
 * Inference_Step and ignored (Model.py:249-253).  token_lengths == NULL reproduces that.  With a [B] int32
 * device array the padded positions t >= token_lengths[b] are treated as non-existent (encoder convs see zeros there,
 * the BiLSTM and the attention cover [0, length) only), so every utterance of a ragged batch equals that utterance
 * run alone; encoder rows / alignment columns beyond the length are written as 0. */

/* tokens [B,Tv] int32  ->  enc [B,Tv,2*enc_rnn] */
int gsttaco_encode(gsttaco_ctx* ctx, const int32_t* tokens, const int32_t* token_lengths, int B, int Tv, float* enc,
                   void* stream);

/* mels_for_gst [B,Tref1,mel] (frame 0 = the prepended zero frame, dropped inside as GST.py:98 does),
 * mel_lengths [B] int32 (excluding that frame)  ->  gst [B,gst_att] */
int gsttaco_gst(gsttaco_ctx* ctx, const float* mels_for_gst, const int32_t* mel_lengths,
                int B, int Tref1, float* gst, void* stream);

/* Style control (EXTENSION, ABI 14).  H = heads, N = n_tokens, A = gst_att, dh = A / H; V = tanh(tokens).Wv + bv [N,A] is
 * precomputed at finalize.  The reference's layer (Layers.py:172-214) is
 *     q        = ref.Wq + bq                                                      [B,A]   (ref = reference-encoder output)
 *     p[b,h,:] = softmax_n( q[b, h*dh:(h+1)*dh] . V[:, h*dh:(h+1)*dh]^T )          [B,H,N]
 *     gst      = LayerNorm( concat_h( p[b,h,:] . V[:, h-slice] ) + q ; gamma, beta, eps 1e-8 )
 * and throws p away (GST.py:105).
 *
 * gsttaco_gst_ex = gsttaco_gst + what it computed on the way: token_weights [B,heads,n_tokens] = p and query [B,gst_att] = q;
 * either may be NULL.  gst is bitwise what gsttaco_gst returns. */
int gsttaco_gst_ex(gsttaco_ctx* ctx, const float* mels_for_gst, const int32_t* mel_lengths, int B, int Tref1,
                   float* gst, float* token_weights, float* query, void* stream);

/* compose(weights, query) = LayerNorm( concat_h( weights[b,h,:] . V[:, h-slice] ) + query ):
 * token_weights [B,heads,n_tokens], query [B,gst_att] or NULL (= 0)  ->  gst [B,gst_att].
 *   - the weights are ANY real numbers: not normalised, not clipped (the GST paper scales and negates them; a caller who wants
 *     a softmax applies one);
 *   - compose(p, q) of a reference's exported pair is that reference's embedding up to fp32 rounding (gsttaco_gst divides the
 *     weighted sum by the softmax denominator once, compose multiplies by the already divided weights);
 *   - all-zero weights with no query give exactly beta (the LayerNorm input is 0 and 0 / sqrt(0 + 1e-8) = 0);
 *   - tokens alone (query NULL) are OUTSIDE THE TRAINING DISTRIBUTION of this architecture: the decoder only ever saw
 *     LayerNorm(attention output + q).  The function is well defined there all the same.
 * One launch on the caller's stream straight from / to the caller's pointers (like gsttaco_mel_frontend); needs finalized
 * weights, GST on, B <= max_batch. */
int gsttaco_style_compose(gsttaco_ctx* ctx, const float* token_weights, const float* query, int B, float* gst, void* stream);

/* enc [B,Tv,2*enc_rnn], gst [B,gst_att] (NULL when GST is off)
 * prenet_mask: keep-masks [steps,2,B,prenet] float32 (1 keep / 0 drop), or NULL = generated on the device from `seed`:
 *              at the reference's rate 0.5 the keep bit of (step, layer, utterance row, column) is bit (column & 31) of a
 *              32-bit COUNTER HASH of (seed, step, layer, row, column >> 5) -- three murmur3 finalisers, device_utils.h
 *              gt_keep_word; NOT Philox: the scalar unit derives a wave's 16 decisions in ~25 instructions, which is what
 *              lets the front kernel skip the weight rows that meet an exact zero -- and at any other rate
 *              Philox4x32-10 (u01 > rate).  The reference draws tf.nn.dropout's unseeded stream (Taco2.py:283): only
 *              the distribution can match, checked by tests/test_gpu_parity.py::test_hashed_keep_decisions_look_random
 * attn_noise : N(0,1) samples [steps,B,Tv], or NULL = Philox4x32-10 + Box-Muller from `seed`
 *              (gsttaco_debug_randomness reads back what a call used)
 * steps      : 0 = Max_Step // Step_Reduction, else 1..that
 * outputs    : pre_mel [B,steps*r,mel], stop [B,steps], align [B,steps,Tv] */
int gsttaco_decode(gsttaco_ctx* ctx, const float* enc, const float* gst, const int32_t* token_lengths,
                   const float* prenet_mask, const float* attn_noise, uint64_t seed,
                   int B, int Tv, int steps, float* pre_mel, float* stop, float* align, void* stream);

/* pre_mel [B,T,mel] -> mel [B,T,mel] (5 x Conv1D+BN, tanh on the first post_tanh layers, + residual) */
int gsttaco_postnet(gsttaco_ctx* ctx, const float* pre_mel, int B, int T, float* mel, void* stream);

/* mel [B,T,mel] (the post-net mel) -> spectrogram [B,T,spec_dim]: Vocoder_Taco1 = CBHG (conv bank k=1..N + BN + ReLU,
 * max-pool 2/1, two projection convs, residual, highway stack, BiLSTM) + Dense (reference Taco2.py:234-260, 285-424). */
int gsttaco_vocoder(gsttaco_ctx* ctx, const float* mel, int B, int T, float* spectrogram, void* stream);

/* wav -> mels_for_gst without leaving the GPU and without needing weights (works before finalize).
 * Needs cfg.max_wav_samples > 0.  Reference: Mel_Generate(path, top_db, range_Ignore=True) per utterance
 * (Pattern_Generator.py:39-60; top_db is 60 for one reference wav and 15 for several, Feeder.py:204-209, and 60 in
 * Get_Inference_GST_Pattern, Feeder.py:232), stacked as Feeder does: frame 0 of every utterance is zero, frames
 * 1..mel_lengths[b] hold the mel, the rest is zero padding.
 * wav          : [B, ld_wav] float32 samples in [-1,1) at Sound.Sample_Rate (librosa.load's output; gsttaco_resample below brings
 *                audio at another rate there on the device, in this layout), wav_lengths [B] valid samples
 *                (17 <= length <= max_wav_samples)
 * mels_for_gst : [B, cap_frames, mel_dim] with cap_frames >= 2 + ld_wav / frame_shift
 * mel_lengths  : [B] int32, frames EXCLUDING the prepended one; 0 when the trimmed signal is shorter than n_fft/2+1
 *                samples (librosa.stft raises there) */
int gsttaco_mel_frontend(gsttaco_ctx* ctx, const float* wav, const int32_t* wav_lengths, int B, int ld_wav, float top_db,
                         float* mels_for_gst, int32_t* mel_lengths, int cap_frames, void* stream);

/* gsttaco_mel_frontend with a second output from the same STFT (EXTENSION, DESIGN row A17): the linear spectrogram Train_Step compares
 * the vocoder's output with (Pattern_Generator.Spectrogram_Generate / Audio.spectrogram, Audio.py:18-21) of the same trimmed signal,
 *   normalise(20 log10(max(1e-5, |STFT|)) - 20),
 * with the normalisation the mel has: symmetric with Max_Abs_Mel, or [0,1] when it is 0 (Pattern_Generator.py:75-82 passes Max_Abs_Mel).
 * wav, wav_lengths, top_db, cap_frames: as gsttaco_mel_frontend.
 * mels         : [B, cap_frames, mel_dim] as gsttaco_mel_frontend writes it (bitwise), or NULL
 * spectrograms : [B, cap_frames, spec_dim] in the same batch layout -- frame 0 zero, frames 1..lengths[b], zero padding --, or NULL
 * lengths      : [B] int32, the frame count of both (excluding frame 0)
 * GSTTACO_E_INVALID when both outputs are NULL, otherwise as gsttaco_mel_frontend. */
int gsttaco_feature_frontend(gsttaco_ctx* ctx, const float* wav, const int32_t* wav_lengths, int B, int ld_wav, float top_db,
                             float* mels, float* spectrograms, int32_t* lengths, int cap_frames, void* stream);

/* EXTENSION (DESIGN row A19): the resampling of librosa.core.load(path, sr) on the device -- resampy.resample(x, sr_in, sr_out,
 * filter='kaiser_best') followed by fix_length to ceil(n * ratio) samples (Pattern_Generator.py:40-43 on a file that is not at
 * Sound.Sample_Rate) -- for a batch of rows at possibly different rates.  Needs cfg.max_wav_samples > 0, no weights.
 *   x           : [B, ld_in] float32, DEVICE; row b holds in_lengths[b] samples at sr_in[b]
 *   in_lengths, sr_in : [B] int32, HOST.  The launch geometry and the tables depend on them, and a caller has them on the host anyway
 *                 (it read them from the files' headers); they are read before the call returns.
 *   y           : [B, ld_out] float32, DEVICE.  Row b: samples [0, int(n * ratio)) are computed, [int(n * ratio), ld_out) are 0.0 --
 *                 so y with out_lengths is the padded batch gsttaco_mel_frontend takes.  Nothing else is written.
 *   out_lengths : [B] int32, HOST, filled on return (it depends on no device work): ceil(in_lengths[b] * ratio_b) in double with
 *                 ratio_b = (double)sr_out / (double)sr_in[b], at most one more than the computed samples (fix_length's zero)
 * Algorithm (resampy core.py / interpn.py, gst_tacotron_amd/audio.py resample_kaiser_best): band-limited sinc interpolation with the
 * published kaiser_best table -- 64 zero crossings, 512 entries per crossing, beta 14.769656459379492, roll-off 0.9475937167399596,
 * 32 769 float64 entries, built by the library (Kaiser window by the power series of I0), times ratio when ratio < 1 -- linearly
 * interpolated between entries; scale = min(1, ratio), table step int(scale * 512), both wings' tap counts clipped at the signal's ends.
 * The time register of output t is the float64 sum of t additions of 1 / ratio, as resampy accumulates it -- NOT t / ratio: the
 * truncated step makes the interpolation discontinuous where the register crosses an integer, and the accumulated value often lies one
 * rounding below.  One array per rate pair serves every row.  Each output is summed in double in one fixed order (left wing tap 0
 * upward, then right wing tap 0 upward) and rounded to float32 once, so a row is bitwise the same in whatever batch it runs; a row
 * with sr_in[b] == sr_out is copied through bitwise.
 * Tables: per context, keyed by (sr_in, sr_out), built on the host and uploaded on `stream` by the first call that needs the pair (the
 * register to max_wav_samples entries + 512 KiB); the cache holds eight pairs and evicts the least recently used.  One launch per 256
 * rows on `stream`; the per-row parameters travel in the kernel arguments, so calls may follow each other on a stream without
 * synchronisation.
 * GSTTACO_E_INVALID, before anything is enqueued or written: a NULL pointer; B, ld_in, ld_out or a rate < 1; an in_lengths[b] outside
 * [0, ld_in]; sr_in[b] > 16 sr_out or sr_out > 16 sr_in[b]; an out_lengths[b] above ld_out; more than eight distinct pairs
 * (sr_in[b] != sr_out) in one call.  GSTTACO_E_CAPACITY: B > max_batch, ld_out > max_wav_samples. */
int gsttaco_resample(gsttaco_ctx* ctx, const float* x, const int32_t* in_lengths, const int32_t* sr_in, int B, int ld_in, int sr_out,
                     float* y, int ld_out, int32_t* out_lengths, void* stream);

/* spectrogram -> waveform: Audio.inv_spectrogram (reference Audio.py:23-27) = symmetric de-normalisation (max_abs_mel,
 * or the [0,1] one when it is 0), + ref_level_db, dB -> amplitude, ^power, `iters` Griffin-Lim iterations
 * (Audio.py:57-68; librosa stft / istft, hann, centred), inverse pre-emphasis 0.97.  Needs cfg.max_wav_samples > 0.
 * spectrogram : [B, T, spec_dim], the layout gsttaco_vocoder / gsttaco_inference_step write (time-major; the reference
 *               transposes it before the call, Model.py:415)
 * frames      : [B] int32 frames to use per utterance (Model.py:415: max(1, stop index) * Step_Reduction) or NULL = T
 * init_phase  : [B, T, spec_dim] uniform [0,1) numbers (the reference draws np.random.rand unseeded, Audio.py:61) or
 *               NULL = Philox4x32-10 from `seed`
 * wav         : [B, ld_wav] float32, ld_wav >= frame_shift * (T - 1); samples beyond an utterance's length are zero
 * wav_lengths : [B] int32 out (may be NULL): frame_shift * (frames - 1); 0 when that is <= n_fft/2 (librosa raises) */
int gsttaco_griffin_lim(gsttaco_ctx* ctx, const float* spectrogram, const int32_t* frames, int B, int T, int iters,
                        float power, float ref_level_db, const float* init_phase, uint64_t seed,
                        float* wav, int32_t* wav_lengths, int ld_wav, void* stream);

/* CRC-32C of a host buffer continued from `crc` (0 to start): the checksum of TensorFlow checkpoint bundles, used by
 * gst_tacotron_amd/tf_checkpoint.py for the reference's tf.train.Checkpoint files (Model.py:186-189, 267-276).  Host only. */
uint32_t gsttaco_crc32c(const void* data, size_t n, uint32_t crc);

/* host_out [mel_dim, spec_dim] float32 <- the Slaney mel filterbank the front end uses (librosa.filters.mel defaults) */
int gsttaco_mel_basis(gsttaco_ctx* ctx, float* host_out);

/* The whole Inference_Step (Model.py:249-255): encoder, GST, decode loop, postnet and -- when `spectrogram` is not
 * NULL -- the CBHG vocoder, replayed from one cached hipGraph per (B,Tv,Tref1,steps) shape.
 * mels_for_gst / mel_lengths are ignored (may be NULL) when GST is off; pre_mel and spectrogram may be NULL. */
int gsttaco_inference_step(gsttaco_ctx* ctx, const int32_t* tokens, const int32_t* token_lengths,
                           const float* mels_for_gst, const int32_t* mel_lengths,
                           const float* prenet_mask, const float* attn_noise, uint64_t seed,
                           int B, int Tv, int Tref1, int steps,
                           float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream);

/* gsttaco_inference_step with the style GIVEN (EXTENSION, ABI 14): style [B,gst_att] -- from gsttaco_gst / gsttaco_gst_ex,
 * gsttaco_style_compose, or arithmetic on such rows -- replaces mels_for_gst / mel_lengths / Tref1; the reference encoder and the
 * style-token layer are not run.  Everything downstream is the same code and the same decode plan: with style = gsttaco_gst(mels)
 * the outputs are bitwise those of gsttaco_inference_step(mels).  The encoder segment's cached graph is gsttaco_encode's.
 * GSTTACO_E_INVALID ("GST is not used") when GST is off, and for a NULL style. */
int gsttaco_inference_step_styled(gsttaco_ctx* ctx, const int32_t* tokens, const int32_t* token_lengths, const float* style,
                                  const float* prenet_mask, const float* attn_noise, uint64_t seed,
                                  int B, int Tv, int steps,
                                  float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream);

/* Teacher-forced decoding (EXTENSION of the inference interface; the reference's own training=True loop branch, Taco2.py:161,183-187,
 * as Model.py:99-106 wires its Train model): step t consumes the ground-truth frame teacher[:, t*r] in place of the frame step t-1
 * emitted.  For ground-truth-aligned (GTA) mels -- vocoder training -- and forced alignments / durations.
 *   teacher : [B, Tq, mel_dim] float32 in the reference's `mels` layout (Feeder.py:125-139): frame 0 is the go frame, USED AS GIVEN (the
 *             reference feeds zeros), frames 1.. the target, any padding behind it.  Tq >= 2.
 *   steps   : none -- S = ceil((Tq - 1) / r); outputs pre_mel [B,S*r,mel], stop [B,S], align [B,S,Tv] (S*r may exceed Tq - 1)
 *   lengths : like the reference, nothing is masked by mel length: every row runs all S steps, rows past an utterance's own length are
 *             the caller's to trim.  token_lengths (masked mode), injected masks / noise and the seed mean what they mean to
 *             gsttaco_decode: the dropout and noise of step t are those a free run draws at step t under the same seed.
 *   layers  : inference mode (BatchNorm statistics, no encoder dropout) as everywhere in this library -- the usual meaning of GTA, not
 *             Train_Step's forward pass.
 * Every step's prenet-0 pre-activations come from ONE fp32 GEMM over the staged frames in front of the loop (fp32 operands under
 * Use_Mixed_Precision too); the loop runs as launches per step -- never as the persistent decode launch, which feeds its own frames
 * back -- from one cached graph per distinct S: callers whose lengths vary should bucket Tq or use capture_after = 2.  The workspace
 * (max_batch x Max_Step//r x (mel_dim + prenet[0]) floats) is allocated by the first forced call.
 * GSTTACO_E_INVALID: NULL teacher, Tq < 2; GSTTACO_E_CAPACITY: S > Max_Step // r, B / Tv beyond the capacity given at create. */
int gsttaco_decode_forced(gsttaco_ctx* ctx, const float* enc, const float* gst, const int32_t* token_lengths,
                          const float* prenet_mask, const float* attn_noise, uint64_t seed,
                          int B, int Tv, const float* teacher, int Tq, float* pre_mel, float* stop, float* align, void* stream);

/* gsttaco_inference_step / gsttaco_inference_step_styled with the decoder teacher-forced.  With GST on the style comes from EXACTLY ONE of
 * mels_for_gst (+ mel_lengths, Tref1) and style [B,gst_att] -- both or neither: GSTTACO_E_INVALID --; with GST off both are ignored.
 * The encoder segment replays the cached graph of the unforced calls; the middle segment has a graph key kind of its own. */
int gsttaco_inference_step_forced(gsttaco_ctx* ctx, const int32_t* tokens, const int32_t* token_lengths,
                                  const float* mels_for_gst, const int32_t* mel_lengths, const float* style,
                                  const float* prenet_mask, const float* attn_noise, uint64_t seed,
                                  int B, int Tv, int Tref1, const float* teacher, int Tq,
                                  float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream);

/* Durations from an alignment: align [B,S,Tv] -> durations [B,Tv] int32 (device).  For utterance b with n = token_lengths ?
 * token_lengths[b] : Tv and L = mel_lengths ? min(mel_lengths[b], S*r) : S*r, every frame f < L adds 1 to token
 * argmax_{j<n} align[b, f / r, j] (the lowest index on a tie): rows sum to L, columns >= n are 0.  One launch (one workgroup per
 * utterance) on the caller's stream straight from / to the caller's pointers; needs no weights. */
int gsttaco_forced_durations(gsttaco_ctx* ctx, const float* align, const int32_t* token_lengths, const int32_t* mel_lengths,
                             int B, int S, int Tv, int32_t* durations, void* stream);

/* Per-utterance seeds (EXTENSION, DESIGN row A16).  With one `seed` per call an utterance's dropout and noise depend on its row and on
 * the batch's Tv; this entry writes the randomness of a whole decode so that they depend on the utterance's own seed alone: row b draws
 * exactly what a batch of ONE draws at its row 0 under seed = seeds[b] --
 *   keep decisions gt_drop_keep(seeds[b], step, layer, row = 0, col, ncols, rate) (the counter hash at Prenet.Dropout_Rate 0.5, Philox
 *   otherwise), noise gt_normal of Philox(seeds[b]; position, step, 0, 0x2000) -- for any B, row order and Tv.
 *   seeds       : [B] uint64 on the DEVICE
 *   prenet_mask : [steps][2][B][prenet] float32 0/1 at the caller's (unpadded) prenet sizes, or NULL
 *   attn_noise  : [steps][B][Tv] float32, or NULL
 * These are the layouts every prenet_mask / attn_noise argument of this library takes and gsttaco_debug_randomness returns: pass the
 * buffers on to gsttaco_decode[_forced] / gsttaco_inference_step[_styled|_forced] (with token_lengths: without masking the padding of a
 * ragged batch reaches the outputs whatever the seeds).  One launch on the caller's stream; needs a created context, no weights.
 * GSTTACO_E_INVALID: NULL seeds, both outputs NULL, a prenet_mask with unequal prenet layer sizes (the stacked layout needs them equal);
 * GSTTACO_E_CAPACITY: steps > Max_Step // r, B / Tv beyond the capacity given at create. */
int gsttaco_fill_randomness(gsttaco_ctx* ctx, const uint64_t* seeds, int B, int Tv, int steps,
                            float* prenet_mask, float* attn_noise, void* stream);

/* The synthesis report (EXTENSION, DESIGN row A16): what stop [B,S] and align [B,S,Tv] (and mel [B,S*r,mel_dim], or NULL) of a decode say
 * about each utterance, computed on the device.  For utterance b: n = token_lengths ? clip(token_lengths[b], 1, Tv) : Tv;
 * s* = the first step with stop[b,s] < 0, else S (Model.py:380; a NaN is not below 0); E = min(S, max(1, s*));
 * a_s = argmax_{j<n} align[b,s,j] (the lowest index on a tie) and m_s that maximum.  report [B][8] int32:
 *   0 stop_step   s* (== S: the stop token never fired)
 *   1 frames      max(1, s*) * r (Model.py:413; the `frames` gsttaco_griffin_lim takes)
 *   2 end_gap     (n - 1) - max_{s<E} a_s (> 0: the speech ended before the text did)
 *   3 max_jump    max(0, max_{1<=s<E} (a_s - a_{s-1})) (skipped tokens)
 *   4 back_steps  number of s in [1, E) with a_s < a_{s-1}
 *   5 max_stall   longest run of equal consecutive a_s in [0, E), in steps (>= 1)
 *   6 visited     number of distinct values among a_0 .. a_{E-1}
 *   7 nonfinite   non-finite values in stop[b,:E], align[b,:E,:n] and, with mel, mel[b,:frames,:]
 * focus [B] float32 (or NULL): the mean of m_s over s < E, summed in double in a fixed order and rounded once.  With nonfinite != 0,
 * fields 2..6 and focus are unspecified.  Only the E steps an utterance used are read.  One launch (one workgroup per utterance) on the
 * caller's stream straight from / to the caller's pointers; needs no weights.  No thresholds: what counts as too long a stall depends
 * on the voice and on r.  GSTTACO_E_INVALID: NULL stop / align / report; GSTTACO_E_CAPACITY as gsttaco_forced_durations. */
int gsttaco_utterance_report(gsttaco_ctx* ctx, const float* stop, const float* align, const int32_t* token_lengths, const float* mel,
                             int B, int S, int Tv, int32_t* report, float* focus, void* stream);

/* Validation losses (EXTENSION, DESIGN row A17): the four terms of the reference's Train_Step (Model.py:210-241) of a teacher-forced pass
 * -- gsttaco_inference_step_forced's pre_mel, mel, stop and spectrogram against the teacher it consumed -- per utterance, as SUMS (the
 * means over the padded batch are the host's: gst_tacotron_amd/evaluate.py).
 *   pre_mel, mel : [B, S*r, mel_dim]     stop : [B, S]     spectrogram : [B, S*r, spec_dim] or NULL
 *   teacher      : [B, Tq, mel_dim]      spec_target : [B, Tq, spec_dim] or NULL      (frame 0 = the go frame, Feeder.py:125-143)
 *   mel_lengths, spec_lengths : [B] int32 or NULL (= T)
 * T = Tq - 1; the target of prediction frame t is teacher[b, 1 + t]; L = clip(mel_lengths[b], 0, T), Ls = clip(spec_lengths[b], 0, T);
 * S*r >= T and prediction frames t >= T are never read.  losses [B][6] DOUBLE -- the one double output of this header:
 *   0 pre_mel_l1  (sum_{t<L} sum_c |teacher - pre_mel|) / mel_dim
 *   1 mel_l1      the same with mel
 *   2 mel_l2      (sum_{t<L} sum_c (teacher - mel)^2) / mel_dim
 *   3 stop_bce    sum_{s<S} bce(x = stop[b,s], z = [s < ceil(mel_lengths[b] / r)]) over ALL S steps, unmasked as Model.py:227-234 leaves
 *                 it; bce = max(x,0) - x z + log1p(exp(-|x|)); mel_lengths NULL: z = 1 everywhere
 *   4 spec_l1     as field 1 with the spectrogram pair over t < Ls and spec_dim; 0 when either spectrogram pointer is NULL
 *   5 spec_l2     as field 2, likewise
 * Each element's difference is ONE fp32 subtraction; everything after it is double: |.|, the square, the bce, every sum and the one
 * division by the channel count.  Sums run in a fixed order (no floating-point atomics): a call is bitwise reproducible.  A non-finite
 * input propagates to the fields that read it.  One launch (one workgroup per utterance) on the caller's stream straight from / to the
 * caller's pointers; needs no weights.
 * GSTTACO_E_INVALID: a NULL required pointer, Tq < 2, S*r < Tq - 1; GSTTACO_E_CAPACITY as gsttaco_forced_durations (S, B). */
int gsttaco_losses(gsttaco_ctx* ctx, const float* pre_mel, const float* mel, const float* stop, const float* spectrogram,
                   const float* teacher, const float* spec_target, const int32_t* mel_lengths, const int32_t* spec_lengths,
                   int B, int S, int Tq, double* losses, void* stream);

/* Free-run metric (EXTENSION, DESIGN row A18): mel-cepstral distortion along a dynamic-time-warping path (MCD-DTW) between x (synthesised)
 * and y (reference), whose lengths differ, per utterance on the device.
 *   x : [B, Tx, mel_dim]    y : [B, Ty, mel_dim]    float32; x_stride / y_stride = batch stride in floats (0 = T * mel_dim), so
 *       mels_for_gst + mel_dim with y_stride = Tref1 * mel_dim skips the prepended zero frame without a copy
 *   x_len, y_len : [B] int32 or NULL (= Tx / Ty); Lx = clip(x_len[b], 0, Tx), Ly = clip(y_len[b], 0, Ty).  Frames at or beyond the length
 *       are never read.
 * Features.  Every value v is clipped to the normalisation's range as the reference's de-normalisation clips it (Audio.py:98-102):
 * [-A, A] with A = Sound.Max_Abs_Mel (held as float32), [0, 1] when A == 0 (or the context has no Sound section); then converted to
 * double.  n_ceps == 0: the feature vector is the mel_dim channels; 1 <= n_ceps < mel_dim: coefficients k = 1 .. n_ceps (c0 dropped)
 * of the orthonormal DCT-II over the M = mel_dim channels, sum_m v_m sqrt(2/M) cos(pi k (2m+1) / (2M)), summed in double in ascending
 * m; the basis is built in double on the host once per n_ceps.  Either kind is multiplied by g / sqrt(2), g = dB per unit of the
 * normalised mel = 100 / (2A) (100 when A == 0).  Derivation: the normalised mel is affine in the mel's dB value with slope 2A / 100
 * (Audio.py:92-96, min_level_db = -100), so a difference of 1 is g dB; dB = 20 log10(amplitude), so a difference ddB is
 * dc = ddB ln10 / 20 in natural-log amplitude; the usual MCD in dB of a frame pair is (10 / ln10) sqrt(2 sum_k dc_k^2)
 * = (10 / ln10) sqrt(2) (ln10 / 20) sqrt(sum_k ddB_k^2) = (g / sqrt(2)) sqrt(sum_k dv_k^2), and an orthonormal transform keeps that
 * sum.  So the Euclidean distance of two scaled feature vectors IS that frame pair's MCD in dB -- of these log-mel cepstra: comparable
 * between checkpoints of one configuration, NOT with SPTK mel-cepstrum figures from papers.
 * Recurrence, double throughout.  C(i,j) = sqrt(sum_k (f_ik - g_jk)^2); D(0,0) = C(0,0); D(i,j) = C(i,j) + min(D(i-1,j-1), D(i-1,j),
 * D(i,j-1)) over the predecessors that exist; unit weights, no band.  Ties: the diagonal, replaced by up (i-1,j) only if that is
 * strictly smaller, then by left (i,j-1) only if that is strictly smaller than the best so far.  The path is the chain of chosen
 * predecessors from (Lx-1, Ly-1).
 *   cost     : [B] DOUBLE  D(Lx-1, Ly-1)            path_len : [B] int32  cells on that path (max(Lx,Ly) .. Lx+Ly-1)
 *   path     : [B, Tx+Ty-1, 2] int32 or NULL: the cells (i, j) from (0,0) to (Lx-1, Ly-1); rows at or beyond path_len[b] are -1
 * A row with Lx == 0 or Ly == 0: cost 0, path_len 0, path all -1.  A non-finite value (NaN or +-Inf: an infinity is NOT clipped into
 * range) in a used frame makes that row's cost non-finite and its path_len / path unspecified (but within bounds); the other rows are
 * unaffected and the call finishes: every loop is bounded by the lengths.  No floating-point atomics: two calls are bitwise equal;
 * identical x and y rows give cost exactly 0 (one code path computes both sides' features).
 * Two launches (features of all used frames; one workgroup per utterance sweeping the anti-diagonals, then walking back) on the
 * caller's stream straight from / to the caller's pointers; needs a created context, no weights.  Workspace, allocated by the first
 * call and kept: max_batch * Max_Step * max(n_ceps, mel_dim) * 8 bytes for each side's features; by the first call that passes `path`:
 * max_batch * Max_Step^2 back-pointers of one byte.  The sweep keeps three anti-diagonals in LDS (36 bytes per column of Ty).
 * GSTTACO_E_INVALID: NULL x / y / cost / path_len, B < 1, Tx < 1, Ty < 1, n_ceps outside [0, mel_dim), a negative stride;
 * GSTTACO_E_CAPACITY: B > max_batch, Tx or Ty > Max_Step (frames), Ty > 4551 (the LDS of one workgroup). */
int gsttaco_mel_dtw(gsttaco_ctx* ctx, const float* x, const int32_t* x_len, int64_t x_stride,
                    const float* y, const int32_t* y_len, int64_t y_stride,
                    int B, int Tx, int Ty, int n_ceps, double* cost, int32_t* path_len, int32_t* path, void* stream);

/* F0 and aperiodicity per frame of a batch of waveforms by YIN (EXTENSION, DESIGN row A20; de Cheveigne & Kawahara, JASA 111(4), 2002,
 * steps 2-5, restated from the paper) on the frame grid of the mel front end: frame t of the F0 track is frame t of the mel of the same
 * wav.  Needs cfg.max_wav_samples > 0, no weights.
 *   wav, wav_lengths, ld_wav : as gsttaco_mel_frontend (DEVICE; samples at Sound.Sample_Rate = sr)
 *   top_db >= 0  : the row is first cut to the trim bounds gsttaco_mel_frontend computes for that top_db (its two trim launches run, no
 *                  second copy of the decision exists);  top_db < 0 : no trim, y = the row's wav_lengths[b] samples (clipped to
 *                  [0, ld_wav]) -- the case of a Griffin-Lim output.
 *   The tracker reads the raw samples y[0 .. n) of the cut signal: no pre-emphasis and no 0.99 factor (YIN is scale-invariant).
 *   frames       : [B] int32  n > n_fft/2 ? 1 + n / Frame_Shift : 0, clipped to cap_frames (cap_frames >= 1 + ld_wav / Frame_Shift never
 *                  clips).  With top_db >= 0 this is gsttaco_mel_frontend's mel_lengths[b]; for a gsttaco_griffin_lim wav of k frames, k.
 *   f0           : [B, cap_frames] float32 Hz, 0.0 = unvoiced; entries at or beyond frames[b] are written as 0
 *   aperiodicity : [B, cap_frames] float32 or NULL: d' at the chosen lag; for an unvoiced frame the minimum of d' over [tau_min, tau_max];
 *                  0 at or beyond frames[b]
 * Lags: tau_min = floor(sr / fmax), tau_max = ceil(sr / fmin) (in double, of the float arguments); W = window, 0 = round(0.025 sr).
 * Frame t, in double throughout: x_j = y[t * Frame_Shift - (W + tau_max) / 2 + j] (integer division), j in [0, W + tau_max); a sample
 * outside [0, n) reads as 0.0 (reflection is defined only for a pad below n, and this span is wider than n_fft / 2).
 *   1. d(tau) = sum_{j < W} (x_j - x_{j+tau})^2, tau = 0 .. tau_max: one accumulator per lag, ascending j
 *   2. d'(0) = 1, d'(tau) = d(tau) * tau / sum_{k=1..tau} d(k), the running total summed in ascending k; d' = 1 where that total is 0
 *   3. the first tau in [tau_min, tau_max) with d'(tau) < threshold, then tau + 1 while tau + 1 < tau_max and d'(tau+1) < d'(tau);
 *      no such tau: the frame is unvoiced
 *   4. a, b, c = d(tau-1), d(tau), d(tau+1) of the RAW d: offset = (a - c) / (2 (a - 2b + c)) where a - 2b + c > 0, else 0;
 *      f0 = sr / (tau + offset)
 *   5. rounded to float32 once.  (The paper's step 6, the best local estimate, is not built.)
 * One launch (behind the front end's two trim launches when top_db >= 0) on the caller's stream straight from / to the caller's
 * pointers: one workgroup per frame, a lane per lag.  No floating-point atomics: two calls are bitwise equal and a row is bitwise the
 * same in whatever batch it runs.  A non-finite sample makes the frames that read it unspecified; every loop stays bounded.
 * GSTTACO_E_INVALID, before anything is enqueued or written: NULL wav / wav_lengths / f0 / frames; B, ld_wav or cap_frames < 1; a NaN
 * top_db; fmin <= 0, fmax <= fmin, tau_min < 2, tau_min >= tau_max; threshold outside (0, 1]; window < 0; W + tau_max > 3072 (the
 * samples, 4 bytes each, and two doubles per lag within 64 KiB of one workgroup's LDS).
 * GSTTACO_E_CAPACITY: B > max_batch, ld_wav > max_wav_samples. */
int gsttaco_pitch(gsttaco_ctx* ctx, const float* wav, const int32_t* wav_lengths, int B, int ld_wav,
                  float top_db, float fmin, float fmax, float threshold, int window,
                  float* f0, float* aperiodicity, int32_t* frames, int cap_frames, void* stream);

/* Pitch errors of a synthesised F0 track x against a reference track y along a path (EXTENSION, DESIGN row A20): the counts behind
 * gross pitch error, voicing decision error and F0 frame error.  Voiced means f0 > 0.
 *   f0_x : [B, Tx], x_len [B] or NULL (= Tx; clipped to [0, Tx]) = Lx;   f0_y : [B, Ty], y_len likewise = Ly
 *   path : [B, path_cap, 2] int32 cells (i, j) and path_len [B] exactly as gsttaco_mel_dtw writes them (path_cap = Tx + Ty - 1 there;
 *          path_len is clipped to [0, path_cap]); NULL: the cells (i, i), i < min(Lx, Ly) -- the teacher-forced case.
 *          A cell outside [0, Lx) x [0, Ly) (the -1 rows) is skipped, never read.
 *   counts : [B][6] int32  0 pairs (cells used), 1 both_voiced, 2 gross (both voiced and |fx - fy| > gross * fy, in double, strict),
 *            3 voicing (exactly one side voiced), 4 x_voiced, 5 y_voiced
 *   sums   : [B][2] DOUBLE over the both-voiced, non-gross cells, c = 1200 log2(fx / fy):  0 sum |c|,  1 sum c^2
 * One launch, one workgroup per utterance, fixed-order reductions: bitwise reproducible.  Needs a created context only.
 * GSTTACO_E_INVALID: NULL f0_x / f0_y / counts / sums, a path without path_len, B / Tx / Ty < 1, path_cap < 1 with a path, gross < 0
 * or NaN;  GSTTACO_E_CAPACITY: B > max_batch. */
int gsttaco_pitch_errors(gsttaco_ctx* ctx, const float* f0_x, const int32_t* x_len, int Tx,
                         const float* f0_y, const int32_t* y_len, int Ty,
                         const int32_t* path, const int32_t* path_len, int path_cap,
                         int B, float gross, int32_t* counts, double* sums, void* stream);

/* The symmetric affinities of exact t-SNE over N style embeddings (EXTENSION, DESIGN row A21; van der Maaten & Hinton, JMLR 9, 2008, with
 * the perplexity search as bhtsne / Rtsne run it, restated here).  Needs a created context only, no weights.
 *   x : [N, ldx] float32 (DEVICE), the first D channels of a row are the embedding -- what gsttaco_gst writes, ldx = D = Attention.Size
 *   p : [N, N] DOUBLE   beta : [N] DOUBLE   search_iters : [N] int32 or NULL
 * Distances, in double: d_ij = sum_k (x_ik - x_jk)^2, each x converted to double first, one accumulator per pair, ascending k, the
 * square and the sum each rounded (no fused multiply-add) -- direct differences, not the Gram form: identical rows give exactly 0,
 * d_ij == d_ji bitwise, and d is the same double on any IEEE machine.
 * Row i: delta_j = d_ij - min_{j != i} d_ij for j != i (the shift changes nothing mathematically and keeps s >= 1 for embeddings of any
 * scale: no 0 / 0).  The search: beta = 1, lo = -inf, hi = +inf; a round computes w_j = exp(-beta delta_j) for j != i, s = sum_j w_j,
 * H = log(s) + beta (sum_j delta_j w_j) / s and Hd = H - log(perplexity) (the log in double of the float argument); it stops the search
 * when |Hd| < 1e-5; else if Hd > 0: lo = beta, then beta = 2 beta while hi is +inf, else (beta + hi) / 2; otherwise: hi = beta, then
 * beta = beta / 2 while lo is -inf, else (beta + lo) / 2.  At most 200 rounds.  search_iters[i] = the rounds run (1 .. 200, the
 * stopping round included), beta[i] = the beta the search ended with: the stopping round's, or the one the 200th round's update left.
 * p_{j|i} = w_j / s at THAT beta (after 200 undecided rounds w and s are evaluated once more at it); p_ij = (p_{j|i} + p_{i|j}) / (2N),
 * p_ii = 0, p_ij == p_ji bitwise, no floor on p.  Rows with duplicates, or a perplexity below a point's number of duplicates, end with
 * a large finite beta (up to 2^200) and finite p.  The sums over j have a fixed order (not ascending j), so two calls are bitwise equal.
 * Three launches on the caller's stream, everything in the caller's buffers: p holds the distances, then p_{j|i}, then p_ij; no
 * workspace.  A non-finite x makes the result unspecified; every loop stays bounded and the call finishes.
 * GSTTACO_E_INVALID, before anything is enqueued or written: NULL x / p / beta; N < 3; D < 1; ldx < D; a perplexity that is not finite
 * or lies outside the open interval (1, N - 1) -- log(N - 1) is the entropy no beta exceeds.
 * GSTTACO_E_CAPACITY: N > 8192 (a row of distances stays in the registers of one workgroup: 1024 lanes x 8). */
int gsttaco_style_affinities(gsttaco_ctx* ctx, const float* x, int N, int D, int64_t ldx, float perplexity,
                             double* p, double* beta, int32_t* search_iters, void* stream);

/* The descent of exact (theta = 0) t-SNE into two dimensions as bhtsne / Rtsne run it (EXTENSION, DESIGN row A21), double throughout;
 * the float arguments are converted to double as they are.  Needs a created context only.
 *   p : [N, N] DOUBLE as gsttaco_style_affinities writes it   y, velocity, gains : [N, 2] DOUBLE each, read AND written
 * For t = first_iter .. first_iter + iters - 1:
 *   e = exaggeration while t < stop_lying_iter, else 1;  m = momentum while t < mom_switch_iter, else final_momentum
 *   n_ij = 1 / (1 + |y_i - y_j|^2) for i != j;  Z = sum_{i != j} n_ij
 *   g_i = sum_j (e p_ij - n_ij / Z) n_ij (y_i - y_j), computed as e A_i - B_i / Z with S_i = sum_j n_ij, A_i = sum_j p_ij n_ij (y_i - y_j),
 *         B_i = sum_j n_ij^2 (y_i - y_j) and Z = sum_i S_i -- no factor 4: bhtsne's exact gradient has none and its eta = 200 assumes that
 *   per component: gains = gains + 0.2 where sign(g) != sign(velocity), else gains * 0.8, sign in {-1, 0, +1}; gains = max(gains, 0.01);
 *         velocity = m velocity - eta gains g;  y = y + velocity
 *   then the column means of y are subtracted from y.
 * kl (DOUBLE [1] or NULL), after the last step: sum over p_ij > 0 of p_ij log(p_ij / q_ij), q_ij = n_ij / Z at the final y, no exaggeration.
 * The state is (y, velocity, gains, first_iter) and nothing else: one call of 1000 steps equals two of 500 bitwise (the second with
 * first_iter = 500), and iters = 0 with kl only evaluates the divergence.  A fresh run starts at gains = 1, velocity = 0.
 * Per step two plain launches on the caller's stream (the pair terms, a wave per row with y tiled through LDS; then one workgroup that
 * sums Z, updates and recentres), four more for kl; every sum has one fixed order (not ascending j), no floating-point atomics, no
 * workgroup waits on another: two calls are bitwise equal.  Workspace: 5 * 8192 + 1 doubles, allocated by the first call and kept.
 * A non-finite input makes the result unspecified; every loop is bounded by N and iters and the call finishes.
 * GSTTACO_E_INVALID, before anything is enqueued or written: NULL p / y / velocity / gains; N < 3; iters < 0; first_iter < 0; an eta or
 * exaggeration that is not finite and positive; momentum or final_momentum outside [0, 1).
 * GSTTACO_E_CAPACITY: N > 8192 (the cap of gsttaco_style_affinities). */
int gsttaco_style_map(gsttaco_ctx* ctx, const double* p, int N, double* y, double* velocity, double* gains,
                      int first_iter, int iters, float exaggeration, int stop_lying_iter, int mom_switch_iter,
                      float momentum, float final_momentum, float eta, double* kl, void* stream);

/* The neural vocoder: the MelGAN generator, mel -> waveform (EXTENSION, DESIGN row A22; Kumar et al., NeurIPS 2019, and its public
 * implementation).  One per context, owned by it and freed by gsttaco_destroy; gsttaco_config and the model's manifest know nothing of it.
 * The network, with mult = 2^n_ratios, x [T, mel_dim] and L(.) = LeakyReLU(slope):
 *   input    reflection-pad 3 each side, Conv1D mel_dim -> mult * base, 7 taps, bias
 *   per ratio r (C the channels so far): L; ConvTranspose1D C -> C/2, kernel 2r, stride r, padding r/2, bias: the output length is exactly
 *            r * len, every output sample has two taps, and beyond its ends the input counts as absent (zero), not reflected.  Then
 *            n_res residual blocks, block j = 0 .. n_res - 1 at dilation d = 3^j:
 *              y = shortcut(x) + conv1(L(conv3_d(reflect_pad_d(L(x)))))
 *            shortcut and conv1 1-tap convs C/2 -> C/2, conv3_d a 3-tap conv at dilation d, all three with bias.
 *   output   L, reflection-pad 3, Conv1D base -> 1, 7 taps, bias, tanh
 * T frames give exactly T * prod(ratios) samples in [-1, 1].  Weight normalisation is folded on the host; the device sees plain weights.
 * Rows have lengths: row b uses frames[b] frames, and every reflection and every transposed-conv edge is taken at the row's own length
 * at that stage, frames[b] * prod(ratios so far).  A row's samples are bitwise those of the row run alone, whatever batch, T or
 * capacity it ran in: every output has one summation order (bias, taps ascending, channels ascending in groups of 16; fp32 MFMA, no
 * atomics).  A row shorter than min_frames = max(4, floor(3^(n_res-1) / ratios[0]) + 1) -- reflection needs pad < length -- gets
 * length 0; frames[b] > T counts as T.  Samples beyond a row's length, up to ld_wav, are written as zeros. */
typedef struct gsttaco_melgan_config {
    int32_t mel_dim;            /* 80 */
    int32_t base;               /* 32: channels in front of the output conv (ngf) */
    int32_t n_ratios;           /* 4 */
    int32_t ratios[GSTTACO_MAX_LAYERS];     /* 8, 8, 2, 2: even, their product is the hop */
    int32_t n_res;              /* 3 */
    float slope;                /* 0.2 */
    int32_t max_batch, max_frames;          /* capacity of a call */
} gsttaco_melgan_config;

/* Fixes the sizes and builds the vocoder's manifest.  No GPU use.  GSTTACO_E_INVALID with a message: an odd ratio (it would need
 * output_padding), mel_dim / base / n_res / a capacity < 1, n_res > 8, more than 8 ratios, a slope outside [0, 1], a stage whose
 * tile cannot fit in 160 KB of LDS, or a context whose vocoder is configured already. */
int gsttaco_melgan_configure(gsttaco_ctx* ctx, const gsttaco_melgan_config* cfg);

/* The vocoder's own manifest (gsttaco_num_weights of the model is unchanged), plain folded fp32 in the [taps * cin, cout] convention:
 *   melgan/in/kernel [7 * mel_dim, mult * base]      melgan/in/bias [mult * base]
 *   melgan/up<i>/kernel [2r, cin, cout]               melgan/up<i>/bias [cout]            (i = 0 .. n_ratios - 1; tap k, as torch's [cin, cout, k])
 *   melgan/up<i>/res<j>/conv3/kernel [3 * C, C], .../conv1/kernel [C, C], .../shortcut/kernel [C, C], each with .../bias [C]
 *   melgan/out/kernel [7 * base, 1]                   melgan/out/bias [1]
 * GSTTACO_E_WEIGHTS: an unknown name, a wrong shape, a load before configure or after finalize. */
int gsttaco_melgan_num_weights(const gsttaco_ctx* ctx);
int gsttaco_melgan_weight_info(const gsttaco_ctx* ctx, int i, const char** name, int64_t shape[4], int* ndim);
int gsttaco_melgan_load_weight(gsttaco_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);

/* Repacks the weights into the kernels' fragment order (channel counts zero-padded to multiples of 16), uploads them and allocates the
 * workspace for the capacity: 2 * max_batch * max_frames * (the widest activation, 8192 floats per frame at the defaults) floats.
 * GSTTACO_E_WEIGHTS when a tensor was not loaded. */
int gsttaco_melgan_finalize(gsttaco_ctx* ctx);

/* mel : [B, T, mel_dim] float32 (DEVICE), normalised as gsttaco_inference_step writes it   frames : [B] int32 (DEVICE) or NULL = T
 * wav : [B, ld_wav] float32 (DEVICE), ld_wav >= T * hop   wav_lengths : [B] int32 (DEVICE) or NULL, written
 * 2 + n_ratios * (1 + n_res) plain launches on the caller's stream: no allocation, no synchronisation, capturable in a graph.
 * GSTTACO_E_WEIGHTS before gsttaco_melgan_finalize; GSTTACO_E_CAPACITY: B > max_batch or T > max_frames; GSTTACO_E_INVALID: a NULL
 * mel / wav, B or T < 1, ld_wav < T * hop. */
int gsttaco_melgan(gsttaco_ctx* ctx, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths,
                   int ld_wav, void* stream);

/* Test support: what the launches of a configured vocoder are.  fields[0] = the number of launches S, fields[1] = min_frames,
 * fields[2] = hop; then per launch GSTTACO_MELGAN_PLAN_STRIDE ints: kind (0 input conv, 1 transposed conv, 2 residual block, 3 output
 * conv), output channels, the time tile (kind 1: in input positions 0 .. len inclusive; else in output samples), the kernel form
 * (N-tiles of 16 channels a wave owns per item; 0 for kind 3), samples per frame of the tile's unit, dynamic LDS bytes.
 * fields holds GSTTACO_MELGAN_PLAN_INTS ints.  Launches nothing.
 * gsttaco_melgan_debug_stage (timing support, tools/melgan_time.py): launch `stage` (0 .. S - 1) of gsttaco_melgan alone, with the
 * same arguments and checks, on whatever activations the workspace holds from an earlier whole call of the same B and T. */
int gsttaco_melgan_debug_stage(gsttaco_ctx* ctx, int stage, const float* mel, const int32_t* frames, int B, int T, float* wav, int ld_wav,
                               void* stream);
#define GSTTACO_MELGAN_PLAN_STRIDE 6
#define GSTTACO_MELGAN_PLAN_INTS (3 + 6 * 74)
int gsttaco_melgan_plan(const gsttaco_ctx* ctx, int32_t fields[]);

/* The flow vocoder: WaveGlow inference, mel -> waveform, sampled from noise under a temperature (EXTENSION, DESIGN row A23; Prenger,
 * Valle & Catanzaro, ICASSP 2019).  One per context, owned by it and freed by gsttaco_destroy; gsttaco_config, the model's manifest and the
 * MelGAN state know nothing of it.  With G = n_group, F = n_flows, EE = n_early_every, ES = n_early_size, NL = n_layers, C = n_channels:
 *   c_k   = G - ES * #{j : 0 < j <= k, j % EE == 0}, the channels of flow k (the defaults: 8 for flows 0..3, 6 for 4..7, 4 for 8..11);
 *   n_rem = c_{F-1};   L = frames * hop / G, the columns of a row of `frames` frames.
 * Inference of one row, at the row's own length, zeros beyond it:
 *   1. up: ConvTranspose1D mel_dim -> mel_dim, kernel win, stride hop, bias, cropped to the first frames * hop samples: sample
 *      q * hop + p sums taps p + j * hop of frames q - j, j = 0 .. win / hop - 1; frames below 0 are absent.  Later frames never reach an
 *      earlier sample, so the crop is exact for a padded batch.
 *   2. group: spect[l, m * G + g] = up[l * G + g, m], giving [L, mel_dim * G].
 *   3. noise: audio = sigma * z[:, 0:n_rem], giving [L, n_rem].
 *   4. for k = F-1 down to 0, h = c_k / 2, a0 = audio[:, :h], a1 = audio[:, h:]:
 *        hid = start_k of a0 (one tap, h -> C);  out = 0
 *        for layer i = 0 .. NL-1 at dilation 2^i, zero "same" padding at the row's ends:
 *          acts = in_{k,i} of hid (three taps, C -> 2C) + cond_{k,i} of spect (one tap, mel_dim * G -> 2C)
 *          g = tanh(acts[:, :C]) * sigmoid(acts[:, C:]);  rs = res_skip_{k,i} of g (one tap, C -> 2C; at the last layer C -> C)
 *          every layer but the last: hid += rs[:, :C], out += rs[:, C:];  the last: out += rs
 *        o = end_k of out (one tap, C -> 2h), b = o[:, :h], s = o[:, h:];  a1 = (a1 - b) * exp(-s)
 *        audio = [a0 | a1] @ inverse(W_k)^T
 *        if k % EE == 0 and k > 0: audio = [sigma * z[:, next ES columns] | audio]
 *   5. wav[l * G + g] = audio[l, g].  It is NOT bounded by 1; a WAV writer clips.
 * The G columns of z are each used exactly once: n_rem first, then ES per early injection in the order inference meets them.
 * inverse(W_k) is computed once at finalize, in float64 on the host.  Row b uses frames[b] frames (above T: T; below 1: length 0, all zeros);
 * its samples are bitwise those of the row run alone, whatever batch, T or capacity it ran in: one summation order per output (fp32
 * MFMA, no atomics), and z[b, l * G + g] depends on (seed, l, g) only. */
typedef struct gsttaco_waveglow_config {
    int32_t mel_dim;            /* 80 */
    int32_t hop;                /* 256 = Sound.Frame_Shift */
    int32_t win;                /* 1024: the upsampler's kernel, a multiple of hop */
    int32_t n_group;            /* 8: even, divides hop, at most 16 */
    int32_t n_flows;            /* 12, at most 32 */
    int32_t n_early_every;      /* 4 */
    int32_t n_early_size;       /* 2: even */
    int32_t n_layers;           /* 8, at most 10 */
    int32_t n_channels;         /* 256 */
    int32_t kernel;             /* 3, fixed: the WN layers' taps */
    int32_t max_batch, max_frames;          /* capacity of a call */
} gsttaco_waveglow_config;

/* Fixes the sizes and builds the flow vocoder's manifest.  No GPU use.  GSTTACO_E_INVALID with a message that names the field: win % hop,
 * hop % n_group, n_group % 2, n_early_size % 2 or any c_k % 2 nonzero; n_rem < 2; any size below 1; n_layers > 10, n_flows > 32,
 * n_group > 16; kernel other than 3; a tile that cannot fit the 160 KB of LDS; max_batch * max_frames * hop above 2^31 - 1; a context
 * whose flow vocoder is configured already. */
int gsttaco_waveglow_configure(gsttaco_ctx* ctx, const gsttaco_waveglow_config* cfg);

/* The flow vocoder's own manifest, plain folded fp32 in the [taps * cin, cout] convention:
 *   waveglow/up/kernel [win, mel_dim, mel_dim] (tap t, as torch's [cin, cout, t])       waveglow/up/bias [mel_dim]
 *   waveglow/flow<k>/W [c_k, c_k]
 *   waveglow/flow<k>/start/kernel [c_k / 2, C]      .../start/bias [C]      waveglow/flow<k>/end/kernel [C, c_k]     .../end/bias [c_k]
 *   waveglow/flow<k>/layer<i>/in/kernel [3 * C, 2 * C], .../cond/kernel [mel_dim * G, 2 * C], .../res_skip/kernel [C, 2 * C] (the last
 *   layer: [C, C]), each with .../bias
 * GSTTACO_E_WEIGHTS: an unknown name, a wrong shape, a load before configure or after finalize. */
int gsttaco_waveglow_num_weights(const gsttaco_ctx* ctx);
int gsttaco_waveglow_weight_info(const gsttaco_ctx* ctx, int i, const char** name, int64_t shape[4], int* ndim);
int gsttaco_waveglow_load_weight(gsttaco_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);

/* Inverts every W_k (float64), repacks the weights into the kernels' fragment order (channel counts zero-padded to multiples of 16),
 * uploads them and allocates the workspace for the capacity:
 *   max_batch * max_frames * (hop / G) * (S_p + 3 * C_p + 16) floats
 * -- spect, two hid, out and audio per column; S_p and C_p are mel_dim * G and C rounded up to 16; 45 568 floats per frame at the defaults.
 * GSTTACO_E_WEIGHTS when a tensor was not loaded or a W_k is singular; a failed allocation is GSTTACO_E_HIP. */
int gsttaco_waveglow_finalize(gsttaco_ctx* ctx);

/* seeds : [B] uint64 (DEVICE)   z : [B, T * hop] float32 (DEVICE), written:  z[b, l * G + g] = gt_normal of the Philox words of counter
 * (l, g, 0, 0x8000) under seeds[b] -- a sample depends on (seed, position, channel) only, not on the batch, on T or on the capacity.
 * Needs a configured context (hop and G).  GSTTACO_E_INVALID: a NULL, B or T < 1. */
int gsttaco_waveglow_noise(gsttaco_ctx* ctx, const uint64_t* seeds, int B, int T, float* z, void* stream);

/* mel : [B, T, mel_dim] float32 (DEVICE), normalised as gsttaco_inference_step writes it   frames : [B] int32 (DEVICE) or NULL = T
 * seeds : [B] uint64 (DEVICE) or z : [B, T * hop] float32 (DEVICE) -- exactly one of the two; with seeds the call is bitwise the call
 * with z = what gsttaco_waveglow_noise writes for them.   sigma >= 0: the temperature.
 * wav : [B, ld_wav] float32 (DEVICE), ld_wav >= T * hop   wav_lengths : [B] int32 (DEVICE) or NULL, written: frames[b] * hop
 * 2 + F * (NL + 1) plain launches on the caller's stream: no allocation, no synchronisation, capturable in a graph.
 * GSTTACO_E_WEIGHTS before gsttaco_waveglow_finalize; GSTTACO_E_CAPACITY: B > max_batch or T > max_frames; GSTTACO_E_INVALID: a NULL
 * mel / wav, B or T < 1, ld_wav < T * hop, both or neither of seeds / z, sigma < 0 or not finite. */
int gsttaco_waveglow(gsttaco_ctx* ctx, const float* mel, const int32_t* frames, int B, int T, float sigma,
                     const uint64_t* seeds, const float* z, float* wav, int32_t* wav_lengths, int ld_wav, void* stream);

/* Test support: what the launches of a configured flow vocoder are.  fields[0] = the number of launches S, fields[1] = hop,
 * fields[2] = G; then per launch GSTTACO_WAVEGLOW_PLAN_STRIDE ints: kind (0 upsampler, 1 WN layer, 2 flow tail), channels, the time tile
 * (kind 0: in frames; else in columns of G samples), the kernel form (N-tiles of 16 channels a wave owns per item; 0 for kind 2),
 * samples per unit of the tile (hop or G), dynamic LDS bytes.  fields holds GSTTACO_WAVEGLOW_PLAN_INTS ints.  Launches nothing.
 * gsttaco_waveglow_debug_stage (timing support, tools/waveglow_time.py): launch `stage` (0 .. S - 1) of gsttaco_waveglow alone, with
 * the same arguments and checks, on whatever the workspace holds from an earlier whole call of the same B and T. */
int gsttaco_waveglow_debug_stage(gsttaco_ctx* ctx, int stage, const float* mel, const int32_t* frames, int B, int T, float sigma,
                                 const uint64_t* seeds, const float* z, float* wav, int ld_wav, void* stream);
#define GSTTACO_WAVEGLOW_PLAN_STRIDE 6
#define GSTTACO_WAVEGLOW_PLAN_INTS (3 + 6 * 354)
int gsttaco_waveglow_plan(const gsttaco_ctx* ctx, int32_t fields[]);

/* The HiFi-GAN vocoder: the generator of Kong, Kim & Bae (NeurIPS 2020) and its public implementation, mel -> waveform (EXTENSION,
 * DESIGN row A24).  One per context, beside or without the MelGAN generator and WaveGlow, owned by the context and freed by
 * gsttaco_destroy; gsttaco_config and the model's manifest know nothing of it.
 * The network, with x [T, mel_dim] and L(.) = LeakyReLU(slope):
 *   input    Conv1D mel_dim -> initial, 7 taps, zero padding 3, bias
 *   per rate u_i (C the channels so far): L; ConvTranspose1D C -> C/2, kernel 2 u_i, stride u_i, padding u_i / 2, bias: the output
 *            length is exactly u_i * len, every output sample has two taps, and beyond its ends the input counts as absent (zero).
 *            Then the fusion  y = (1 / n_kernels) * sum_j ResBlock_j(x)  over residual blocks of kernel size k_j = kernels[j] and
 *            dilations D_j = dilations[j][0 .. n_dilations[j] - 1], the sum taken in the order j = 0, 1, ...:
 *              resblock = 1, for every d in D_j in order:  x = x + conv_{k_j, 1}(L(conv_{k_j, d}(L(x))))
 *              resblock = 2, for every d in D_j in order:  x = x + conv_{k_j, d}(L(x))
 *            every conv C/2 -> C/2 with bias and zero padding (k_j - 1) / 2 * d.
 *   output   LeakyReLU(out_slope) -- 0.01, NOT slope: the public code calls F.leaky_relu with its default there --, Conv1D C_last -> 1,
 *            7 taps, zero padding 3, bias, tanh
 * T frames give exactly T * prod(rates) samples in [-1, 1].  Weight normalisation is folded on the host; the device sees plain weights.
 * The shipped configurations: V1 initial 512, rates 8 8 2 2, resblock 1, kernels 3 7 11, dilations 1 3 5 each; V2 the same at initial
 * 128; V3 initial 256, rates 8 8 4, resblock 2, kernels 3 5 7, dilations {1 2} {2 6} {3 12}.
 * Rows have lengths: row b uses frames[b] frames, and every zero pad and every transposed-conv edge is taken at the row's own length at
 * that stage, frames[b] * prod(rates so far); workspace beyond a row's end is never read as data.  A row's samples are bitwise those
 * of the row run alone, whatever batch, T or capacity it ran in: every output has one summation order (bias, taps ascending, channels
 * ascending in groups of 16, the residual, the blocks in order; fp32 MFMA, no atomics).  min_frames is 1 (zero padding needs no
 * length): a row of 0 frames has length 0; frames[b] > T counts as T.  Samples beyond a row's length, up to ld_wav, are written as zeros. */
#define GSTTACO_HIFIGAN_MAX_DILATIONS 4
typedef struct gsttaco_hifigan_config {
    int32_t mel_dim;            /* 80 */
    int32_t initial;            /* 512 (V1): channels behind the input conv; a multiple of 2^n_rates */
    int32_t n_rates;            /* 4 */
    int32_t rates[GSTTACO_MAX_LAYERS];      /* 8, 8, 2, 2: even, their product is the hop; the transposed kernel is twice the rate */
    int32_t resblock;           /* 1 or 2 */
    int32_t n_kernels;          /* 3 */
    int32_t kernels[GSTTACO_MAX_LAYERS];    /* 3, 7, 11: odd, at most 11 */
    int32_t n_dilations[GSTTACO_MAX_LAYERS];                                /* 3, 3, 3: 1 .. 4 per kernel */
    int32_t dilations[GSTTACO_MAX_LAYERS][GSTTACO_HIFIGAN_MAX_DILATIONS];   /* 1, 3, 5 each */
    float slope;                /* 0.1 */
    float out_slope;            /* 0.01 */
    int32_t max_batch, max_frames;          /* capacity of a call */
} gsttaco_hifigan_config;

/* Fixes the sizes and builds the vocoder's manifest.  No GPU use.  GSTTACO_E_INVALID with a message that names the field: mel_dim /
 * initial / a capacity < 1, n_rates or n_kernels outside 1 .. 8, a rate that is odd or < 2, initial not a multiple of 2^n_rates,
 * resblock other than 1 or 2, a kernel that is even or above 11, n_dilations outside 1 .. 4, a dilation < 1, a slope or out_slope
 * outside [0, 1], a launch whose smallest tile cannot fit in 160 KB of LDS, or a context whose HiFi-GAN is configured already. */
int gsttaco_hifigan_configure(gsttaco_ctx* ctx, const gsttaco_hifigan_config* cfg);

/* The vocoder's own manifest (gsttaco_num_weights of the model is unchanged), plain folded fp32 in the [taps * cin, cout] convention:
 *   hifigan/in/kernel [7 * mel_dim, initial]          hifigan/in/bias [initial]
 *   hifigan/up<i>/kernel [2 u_i, cin, cout]            hifigan/up<i>/bias [cout]           (i = 0 .. n_rates - 1; tap k, as torch's [cin, cout, k])
 *   hifigan/up<i>/res<j>/unit<m>/conv1/kernel [k_j * C, C], .../conv1/bias [C]: the conv at dilation D_j[m]; and under resblock = 1
 *   hifigan/up<i>/res<j>/unit<m>/conv2/kernel [k_j * C, C], .../conv2/bias [C]: the unit's closing conv at dilation 1
 *   hifigan/out/kernel [7 * C_last, 1]                 hifigan/out/bias [1]
 * GSTTACO_E_WEIGHTS: an unknown name, a wrong shape, a load before configure or after finalize. */
int gsttaco_hifigan_num_weights(const gsttaco_ctx* ctx);
int gsttaco_hifigan_weight_info(const gsttaco_ctx* ctx, int i, const char** name, int64_t shape[4], int* ndim);
int gsttaco_hifigan_load_weight(gsttaco_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);

/* Repacks the weights into the kernels' fragment order (channel counts zero-padded to multiples of 16), uploads them and allocates the
 * workspace for the capacity: 4 * max_batch * max_frames * (the widest activation, 8192 floats per frame at V1) floats.
 * GSTTACO_E_WEIGHTS when a tensor was not loaded. */
int gsttaco_hifigan_finalize(gsttaco_ctx* ctx);

/* mel : [B, T, mel_dim] float32 (DEVICE), normalised as gsttaco_inference_step writes it   frames : [B] int32 (DEVICE) or NULL = T
 * wav : [B, ld_wav] float32 (DEVICE), ld_wav >= T * hop   wav_lengths : [B] int32 (DEVICE) or NULL, written
 * One launch per convolution (2 + n_rates + the residual convs: 78 at V1), plain launches on the caller's stream: no allocation, no
 * synchronisation, capturable in a graph.
 * GSTTACO_E_WEIGHTS before gsttaco_hifigan_finalize; GSTTACO_E_CAPACITY: B > max_batch or T > max_frames; GSTTACO_E_INVALID: a NULL
 * mel / wav, B or T < 1, ld_wav < T * hop. */
int gsttaco_hifigan(gsttaco_ctx* ctx, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths,
                    int ld_wav, void* stream);

/* Test support: what the launches of a configured HiFi-GAN are.  fields[0] = the number of launches S, fields[1] = min_frames,
 * fields[2] = hop; then per launch GSTTACO_HIFIGAN_PLAN_STRIDE ints: kind (0 input conv, 1 transposed conv, 2 residual conv, 3 output
 * conv), output channels, taps, dilation, the time tile (kind 1: in input positions 0 .. len inclusive; else in output samples), the
 * kernel form (N-tiles of 16 channels a wave owns per item; 0 for kind 3), samples per frame of the tile's unit (kind 1: the rate of
 * its input), dynamic LDS bytes.  fields holds GSTTACO_HIFIGAN_PLAN_INTS ints.  Launches nothing.
 * gsttaco_hifigan_debug_stage is timing support (tools/hifigan_time.py): launch `stage` (0 .. S - 1) of gsttaco_hifigan alone, with
 * the same arguments and checks, on whatever activations the workspace holds from an earlier whole call of the same B and T. */
int gsttaco_hifigan_debug_stage(gsttaco_ctx* ctx, int stage, const float* mel, const int32_t* frames, int B, int T, float* wav, int ld_wav,
                                void* stream);
#define GSTTACO_HIFIGAN_PLAN_STRIDE 8
#define GSTTACO_HIFIGAN_PLAN_INTS (3 + 8 * 522)
int gsttaco_hifigan_plan(const gsttaco_ctx* ctx, int32_t fields[]);

/* The operand form of the HiFi-GAN's matrix products (EXTENSION; new symbols only, no struct and no signature changes).
 * GSTTACO_HIFIGAN_F32, the default, is everything above, bit for bit, uploaded bytes included.  Under GSTTACO_HIFIGAN_BF16 /
 * GSTTACO_HIFIGAN_F16 the input conv, the transposed convs and the residual convs run on v_mfma_f32_16x16x32_bf16 / _f16: the MFMA's
 * two operands are 16-bit, nothing else is.
 *   - Activations stay fp32 in the workspace (the residual stream and the fusion sums are never rounded); the workspace, its four
 *     buffers, the launches, tiles and forms are those of the fp32 plan.  gsttaco_hifigan_plan reports the same table, the dynamic LDS
 *     bytes excepted: they are those of the 16-bit tile, never more than the fp32 tile's.
 *   - A launch's input is taken in fp32 at its bounds (zero outside the row), passed through the LeakyReLU in fp32, then rounded once,
 *     to nearest even, on its way into the staged tile; fp16 saturates to +-65504 instead of producing inf.  The input conv's mel
 *     is rounded the same way (no LeakyReLU).
 *   - A kernel weight is rounded once, to nearest even, on the host at gsttaco_hifigan_finalize.  An fp16 weight that is not finite
 *     after rounding refuses the finalize with GSTTACO_E_WEIGHTS and a message that names the tensor; nothing was uploaded, and the
 *     context may select another form, load the tensor again and finalize.
 *   - Products are exact and summed in fp32 by the MFMA; the accumulator, the bias (fp32), the residual add, the fused sum and the
 *     whole output conv (fp32 weights, VALU) are as in the fp32 form.  One summation order per output sample -- bias, taps ascending,
 *     channels ascending in blocks of 32, the residual, the blocks in order -- that depends on neither batch, T nor capacity: a row
 *     is still bitwise the row run alone, and the call is still capturable.
 * Valid between gsttaco_hifigan_configure and gsttaco_hifigan_finalize: GSTTACO_E_INVALID for another value, GSTTACO_E_WEIGHTS
 * before configure or after finalize.  gsttaco_hifigan_configure always starts a context at GSTTACO_HIFIGAN_F32.
 * Pinned to a float64 restatement with rounded operands on synthetic weights (tests/hifigan_half_cases.py); no trained checkpoint
 * has been run in any form.  MelGAN and WaveGlow have no such setting. */
#define GSTTACO_HIFIGAN_F32 0
#define GSTTACO_HIFIGAN_BF16 1
#define GSTTACO_HIFIGAN_F16 2
int gsttaco_hifigan_set_operands(gsttaco_ctx* ctx, int operands);

/* Test support: copies `floats` floats between the START of workspace buffer `buffer` (0 the fused sum, 1 the transposed conv's output,
 * 2 and 3 the two a residual block alternates between) and `device` (DEVICE memory), device to device on `stream`; write != 0 copies
 * into the workspace.  With gsttaco_hifigan_debug_stage it runs one launch on inputs the caller chose and reads its result back.
 * What a launch of a call (B, T) addresses, with R samples per frame and C_p = round16(channels) at that side of the launch: row b
 * starts at float b * T * R * C_p of the buffer, position t of the row at + t * C_p, channel c at + c; channels [C, C_p) hold zeros.
 *   kind 0 (input conv)       reads mel [B, T, mel_dim] (the call's argument, no workspace), writes buffer 0 at R = 1
 *   kind 1 (transposed conv)  reads buffer 0 at its input rate, writes buffer 1 at its output rate
 *   kind 2 (residual conv)    reads its source through the LeakyReLU, adds its residual raw, writes its destination, or -- the last
 *                             conv of a residual block -- sets (block 0) or adds to (later blocks) buffer 0, times 1 / n_kernels on
 *                             the last block.  resblock = 1: a unit's first conv reads x (buffer 1 in the block's first unit, 3 after)
 *                             and writes 2; its second reads 2, adds x and writes 3.  resblock = 2: a unit reads and adds x (buffer 1,
 *                             then 2, 3, 2, ...) and writes the other of 2 and 3 (2 first).
 *   kind 3 (output conv)      reads buffer 0, writes wav [B, ld_wav]
 * Only positions below a row's own length are read or written.  GSTTACO_E_INVALID: a buffer outside 0 .. 3, a NULL array, floats < 0
 * or beyond the buffer's size (max_batch * max_frames * the widest activation per frame); GSTTACO_E_WEIGHTS before finalize. */
int gsttaco_hifigan_debug_buffer(gsttaco_ctx* ctx, int buffer, float* device, int64_t floats, int write, void* stream);

/* hipGraph cache policy.  Every entry point replays one cached graph executable per (entry, B, Tv, Tref1, steps, flags) key.
 * The cache is LRU-bounded to `max_cached` executables (default 16 -- an Inference_Step replays two or three: encoder segment, GST + decode + postnet, vocoder; GSTTACO_GRAPH_CACHE; 0 = no graphs, everything is
 * enqueued eagerly on the caller's stream); the least recently used one is destroyed when a new shape is captured.
 * `capture_after` = n >= 1: a key is captured at its n-th use and enqueued eagerly before that (default 1;
 * GSTTACO_GRAPH_CAPTURE_AFTER).  Callers whose shapes vary from batch to batch -- the reference's Feeder pads to the
 * batch maximum (Feeder.py:175-180) -- should use 2, or bucket shapes with masked mode, so that a shape that never
 * repeats never pays a ~2 000-node capture.  Results are identical either way (a GPU test compares them bitwise). */
int gsttaco_set_graph_policy(gsttaco_ctx* ctx, int max_cached, int capture_after);
int gsttaco_graph_cache_size(const gsttaco_ctx* ctx);

/* Measurement support (bench.py): per-kernel timing of the last gsttaco_inference_step replay.
 * When enabled, HIP event-record nodes bracket the four kernels of every `every`-th decode step inside the graph. */
int gsttaco_set_profiling(gsttaco_ctx* ctx, int every);
/* After the stream has been synchronised by the caller: average duration (ms) of the bracketed
 * launches of decode-LSTM layer `layer` (0/1) and how many were bracketed. */
int gsttaco_get_profile(gsttaco_ctx* ctx, int layer, float* avg_ms, int* count);
/* Diagnostic (GSTTACO_STAMPS=1): 96 words of phase stamps (100 MHz ticks) at the middle decode step of the last replay.  Launch
 * path: the first 3 x 16 = workgroup 0 of the fused front kernel and of the two decode LSTM kernels; persistent decode launch:
 * 3 x 32 = its chain workgroup 0, projection workgroup 32 and plain workgroup 255 (tools/stamps.py, tools/stamps_persist.py).
 * Synchronises the device. */
int gsttaco_debug_stamps(gsttaco_ctx* ctx, unsigned long long* host_out96);
/* Three launches hand data between their workgroups INSIDE the kernel and therefore need those workgroups resident together: the
 * persistent BiLSTM launch (one launch for all time steps of the encoder's / vocoder's Bidirectional LSTM, reference
 * Taco2.py:39-43, 394-398; the 32 workgroups of each of its groups), the persistent decode launch (the whole decoder loop,
 * Taco2.py:153-228, in one launch of 256 workgroups) and the fused decode-LSTM launch (both LSTMCells of a decoder step,
 * Taco2.py:77-85,111, in one launch; all of its workgroups).  The library arranges that for everything it controls:
 * exactly one persistent workgroup per compute unit, and the fused launches' whole grid against occupancy x compute units, are
 * checked at finalize; the persistent launches of ALL contexts of the process are chained on the GPU, so two of them never split
 * an XCD; the fused / persistent decode launches are taken only while the process has ONE live context, and another context's
 * segments start behind those still in flight (one recorded event per device).  What the library cannot see -- another process on
 * the GPU, a CU mask -- is caught by BOUNDED waits: a wait that gives up raises a word in host-mapped memory, the whole launch
 * drains at once, and
 *   - gsttaco_synchronize(ctx, stream) synchronises the stream and returns GSTTACO_E_HIP if that happened since the last check:
 *     the outputs of the calls since then are invalid, repeat them.  It is the ONLY place that clears the condition: calls
 *     enqueued behind the one that gave up do not erase it (they notice the word when they are enqueued, keep it in a sticky
 *     per-context flag, and already run the next launch form down -- and are correct: each launch form has a give-up word of its
 *     own, so a give-up of the persistent decode launch does not make the fused LSTM launches enqueued behind it leave early);
 *   - the next compute call that notices the word switches the context to the launch-per-step / two-launch form (bitwise the
 *     same results in fp32; under Use_Mixed_Precision the per-step BiLSTM kernel sums in a different order: within the mixed
 *     tolerance), succeeds, and leaves a "warning: ..." text in gsttaco_last_error.
 * Nothing stays poisoned and nothing hangs.  gsttaco_debug_handoff_error synchronises the device and returns what is pending,
 * i.e. raised and not yet reported by gsttaco_synchronize (bit 0: fused decode-LSTM launch, bit 8: persistent BiLSTM, bit 16:
 * persistent decode launch; 0 = clear). */
int gsttaco_synchronize(gsttaco_ctx* ctx, void* stream);
int gsttaco_debug_handoff_error(gsttaco_ctx* ctx, uint32_t* host_out);
/* Test support: out[0] = persistent BiLSTM launches this context has enqueued (eagerly or into a captured graph), out[1] = 1
 * while the context uses the persistent launch, 0 once it has fallen back to one launch per time step; out[2] / out[3] the same
 * for the persistent DECODE launch (the whole decoder loop of Taco2.py:153-228 as one launch: batch <= 128 -- above 32 rows as
 * groups of 32 through one set of resident weights --, T_v <= 256, fp32, decoder sizes up to the reference's (smaller ones are
 * zero-padded to them at finalize: exact, GSTTACO_PAD_DECODER), one live context;
 * GSTTACO_PERSIST_DECODE=0, GSTTACO_PERSIST_ROWS=<max batch> or a give-up: launches per step, bitwise the same). */
int gsttaco_debug_counters(const gsttaco_ctx* ctx, uint64_t out[4]);
/* Test support (fault injection).  bits 0..6 / 7 / 8..15: raise the fused launch's / the persistent decode launch's / the persistent
 * BiLSTM's give-up word as a kernel would.  bits 16..: n > 0 makes member n - 1 of every group of the NEXT persistent launches exit at once and the next fused
 * launches expect one arrival too many, so that their waits really run into the bound. */
int gsttaco_debug_raise_handoff_error(gsttaco_ctx* ctx, uint32_t bits);
/* Test support: the prenet keep-masks [steps][mask0 B*P0 | mask1 B*P1] (0/1) and SMA noise [steps][B][Tv] the LAST
 * gsttaco_inference_step / gsttaco_decode of that shape used -- generated from the seed in throughput mode, or the
 * injected tensors -- copied to HOST buffers (either may be NULL).  Synchronises the device. */
int gsttaco_debug_randomness(gsttaco_ctx* ctx, float* host_masks, float* host_noise, int steps, int B, int Tv);
/* Which variant of the decode step a (Tv)-token batch runs on (finalized context).  plan[0]: 1 = fused per-utterance
 * front kernel (prenet + query + attention), 0 = the four-kernel front end (LSA, or a shape the fused kernel does not
 * cover); plan[1]: 1 = prenet layer 0's pre-activations ride in the previous step's projection launch (a composed
 * weight matrix: under Use_Mixed_Precision that matrix is what gets rounded to bf16, which the parity oracle must know);
 * plan[2]: 1 = lean compile-time-K kernels for the LSTM / projection launches, 0 = general skinny GEMM. */
int gsttaco_decode_plan(const gsttaco_ctx* ctx, int Tv, int32_t plan[3]);
/* Test support: the WHOLE launch plan of one decode of B utterances of Tv tokens on this (finalized) context, as the function that
 * enqueues it decides it (forced != 0: a teacher-forced decode), while this is the process's only live context and no keep masks are
 * injected (those change only whether the keep-mask tensor is read, which is not reported).  fields[GSTTACO_PLAN_*]:
 * PERSIST / PERSIST_BF16 the whole loop as one persistent launch / its bf16 kernel; FUSED the fused front launch (0: the four-kernel
 * front end and whole LSTM GEMMs, and every field below is 0); LEAN_FRONT its lean utterance path; LEAN_REC its workers' recurrent body
 * (0 general, 1 lean fp32, 2 lean bf16); Z0 prenet-0 pre-activations from the previous step's projection launch; FUSE12 both LSTM cells
 * in one launch (0 no, 1 up to 32 rows, 2 the multi-chunk form); LEAN_X0 / LEAN_X1 LSTM layer 1 / 2's input half on the lean kernel;
 * CO_TILES layer-2 recurrent tiles beside the projection; LEAN_PROJ that launch on the lean kernel; MIRROR bf16 mirrors of the blocked
 * activations; DEC_PADDED the decoder runs zero-padded to the reference's sizes; PJ_TILES 16-column tiles of the projection pack
 * [frames, stop | prenet-0 pre-activations].  Launches nothing. */
enum {
    GSTTACO_PLAN_PERSIST = 0, GSTTACO_PLAN_PERSIST_BF16 = 1, GSTTACO_PLAN_FUSED = 2, GSTTACO_PLAN_LEAN_FRONT = 3, GSTTACO_PLAN_LEAN_REC = 4,
    GSTTACO_PLAN_Z0 = 5, GSTTACO_PLAN_FUSE12 = 6, GSTTACO_PLAN_LEAN_X0 = 7, GSTTACO_PLAN_LEAN_X1 = 8, GSTTACO_PLAN_CO_TILES = 9,
    GSTTACO_PLAN_LEAN_PROJ = 10, GSTTACO_PLAN_MIRROR = 11, GSTTACO_PLAN_DEC_PADDED = 12, GSTTACO_PLAN_PJ_TILES = 13,
    GSTTACO_PLAN_COUNT = 14
};
int gsttaco_decode_plan_fields(const gsttaco_ctx* ctx, int B, int Tv, int forced, int32_t fields[GSTTACO_PLAN_COUNT]);
/* Algorithmic bytes one launch of decode-LSTM layer `layer` moves at batch B (weights + activations). */
int64_t gsttaco_lstm_launch_bytes(const gsttaco_ctx* ctx, int layer, int B);

/* Test support: the conv/GEMM dispatcher behind every tall GEMM outside the decode step (encoder convolutions, hoisted BiLSTM
 * inputs, Value projection, GST Conv2D, postnet, vocoder).  Which kernel instantiation a call runs, as decided by the same
 * function the dispatcher switches on: IG = fp32 implicit GEMM <WAVES_M, WAVES_N, RM, RN>, C2D = its 2-D (Conv2D) form,
 * WINO4 / WINO2 = Winograd F(4,5) / F(2,5) on the fp32 pipe, ..._S = the same as split-bf16 x6 (X3: the reduced three-product
 * knob), GEMM_SPLIT = the plain split-bf16 x6 GEMM, C5 = the bf16 five-tap kernel <RN>, BF16 = the bf16 implicit GEMM <RM>;
 * _XB / _OB = bf16 activations in / out. */
enum {
    GSTTACO_CONV_V_INVALID = -1,
    GSTTACO_CONV_V_IG_1411 = 0, GSTTACO_CONV_V_IG_2212 = 1, GSTTACO_CONV_V_IG_2222 = 2,
    GSTTACO_CONV_V_IG_4113 = 3, GSTTACO_CONV_V_IG_4112 = 4, GSTTACO_CONV_V_IG_4111 = 5,
    GSTTACO_CONV_V_C2D_1411 = 6, GSTTACO_CONV_V_C2D_4112 = 7, GSTTACO_CONV_V_C2D_4111 = 8,
    GSTTACO_CONV_V_WINO4 = 9, GSTTACO_CONV_V_WINO2 = 10,
    GSTTACO_CONV_V_WINO4_S = 11, GSTTACO_CONV_V_WINO2_S = 12, GSTTACO_CONV_V_WINO4_S_X3 = 13, GSTTACO_CONV_V_WINO2_S_X3 = 14,
    GSTTACO_CONV_V_GEMM_SPLIT = 15,
    GSTTACO_CONV_V_C5_RN4 = 16, GSTTACO_CONV_V_C5_RN4_XB = 17, GSTTACO_CONV_V_C5_RN4_OB = 18, GSTTACO_CONV_V_C5_RN4_XB_OB = 19,
    GSTTACO_CONV_V_C5_RN2 = 20, GSTTACO_CONV_V_C5_RN2_XB = 21, GSTTACO_CONV_V_C5_RN2_OB = 22, GSTTACO_CONV_V_C5_RN2_XB_OB = 23,
    GSTTACO_CONV_V_BF16_RM2 = 24, GSTTACO_CONV_V_BF16_RM2_XB = 25, GSTTACO_CONV_V_BF16_RM2_OB = 26, GSTTACO_CONV_V_BF16_RM2_XB_OB = 27,
    GSTTACO_CONV_V_BF16_RM1 = 28, GSTTACO_CONV_V_BF16_RM1_XB = 29, GSTTACO_CONV_V_BF16_RM1_OB = 30, GSTTACO_CONV_V_BF16_RM1_XB_OB = 31,
    GSTTACO_CONV_V_COUNT = 32
};
/* The bounded-input variants, numbered on behind the list above (no id moves): WINO4_S / WINO2_S as two fp16 planes and three
 * products (conv_wino_split.hip).  A call reaches them only with the WINO_SPLIT_H form AND a promised input bound
 * (gsttaco_conv_call::x_absmax), so they are kept as a group of their own: what a call without a bound can run is the list above. */
enum {
    GSTTACO_CONV_VH_WINO4_S = 32, GSTTACO_CONV_VH_WINO2_S = 33,
    GSTTACO_CONV_VH_END = 34
};
/* Weight forms gsttaco_debug_conv_prepare builds (bit set), as finalize builds them for a layer:
 * FP32 = w [taps*cin, ldw] with scale / shift (always built), BF16 = its transposed bf16 copy (the mixed-precision kernels),
 * WINO2 / WINO4 = the float64 Winograd transforms U / U4 rounded to fp32 (taps 5), WINO_SPLIT = the three bf16 planes of each
 * Winograd transform built, GEMM_SPLIT = the three bf16 planes of w (taps 1), WINO_SPLIT_H = each Winograd transform built as two fp16
 * planes with per-column power-of-two scaling (only a call that promises |x| <= 1 takes them: x_absmax below). */
enum {
    GSTTACO_CONV_FORM_FP32 = 1, GSTTACO_CONV_FORM_BF16 = 2, GSTTACO_CONV_FORM_WINO2 = 4, GSTTACO_CONV_FORM_WINO4 = 8,
    GSTTACO_CONV_FORM_WINO_SPLIT = 16, GSTTACO_CONV_FORM_GEMM_SPLIT = 32, GSTTACO_CONV_FORM_WINO_SPLIT_H = 64
};
typedef struct gsttaco_conv_desc {
    int32_t taps, cin, n, ldw;  /* ldw: row stride of w in floats (0 = n) */
    int32_t forms;              /* GSTTACO_CONV_FORM_* */
} gsttaco_conv_desc;
typedef struct gsttaco_conv_call {
    int32_t forms;              /* which of the prepared forms the call hands to the dispatcher (a subset of the desc's) */
    int32_t B, T, pad_before, act;     /* act: 0 none, 1 relu, 2 tanh */
    int64_t ldo;                /* output row stride (0 = n) */
    int32_t pool2, x_bf16, out_bf16, wino_x3, wino_min_wgs;
    int32_t conv2d, H, W, Wo, kw, stride, pad_h, pad_w;     /* 2-D mode: T = Ho * Wo, taps = kh * kw */
    float x_absmax;             /* the caller's promise that |x| <= x_absmax everywhere; 0 = none.  (It lies in what was the alignment
                                 * padding in front of xb: the struct's size and every other offset are what they were, and a zeroed
                                 * struct of an older caller makes no promise.) */
    int64_t xb;                 /* 2-D mode: batch stride of x in floats */
} gsttaco_conv_call;
/* Uploads the forms of one conv/GEMM weight (host w [taps*cin, ldw], scale / shift [n] or NULL) as finalize would; the context
 * owns them until destroy.  *id names them for gsttaco_debug_conv_run.  Synchronous. */
int gsttaco_debug_conv_prepare(gsttaco_ctx* ctx, const gsttaco_conv_desc* desc, const float* w_host, const float* scale_host,
                               const float* shift_host, int* id);
/* One dispatcher call with prepared weights `id` on device buffers (x, tokens, row_len, rowbias, res may be NULL; out is written):
 * enqueued on `stream` (a hipStream_t, NULL = the default stream) without allocation or synchronisation.  *variant (may be NULL)
 * receives the GSTTACO_CONV_V_* the call ran. */
int gsttaco_debug_conv_run(gsttaco_ctx* ctx, int id, const gsttaco_conv_call* call, const void* x, const int32_t* tokens,
                           const int32_t* row_len, const float* rowbias, const float* res, void* out, int* variant, void* stream);

/* Test support: the GSTTACO_CONV_V_* / GSTTACO_CONV_VH_* each postnet layer runs at (B, Tf) on this context (variants[i], i < the
 * number of postnet layers; at most 8 are written).  Built by the function that enqueues them; launches nothing. */
int gsttaco_postnet_variants(const gsttaco_ctx* ctx, int B, int Tf, int32_t variants[8]);
/* The same for the encoder's conv layers at (B, Tv).  *rows_path (may be NULL): 1 when the embedding lookup is launched as rows in
 * front of layer 0 (layer 0 then reads rows, not tokens), else 0.  The report is for the call's arguments WITHOUT its buffers and
 * without the masked mode's row lengths: it holds for a masked call only while no form the encoder passes looks at row_len (today
 * none does: FP32, BF16 and the Winograd forms; the plain split GEMM form would). */
int gsttaco_encoder_variants(const gsttaco_ctx* ctx, int B, int Tv, int32_t variants[8], int32_t* rows_path);
/* The same for the vocoder's GEMMs of one kind at (B, Tf), in the order they are enqueued.  *count receives how many layers of the
 * kind the model has (0 for a Dense it does not have); at most 32 variants are written. */
#define GSTTACO_VOC_BANK 0            /* the conv bank, kernel sizes 1 .. Stack_Count */
#define GSTTACO_VOC_PROJ 1            /* the Conv1D projections */
#define GSTTACO_VOC_PROJ_DENSE 2      /* the Dense back to Mel_Dim, where the last projection is not that wide */
#define GSTTACO_VOC_HIGHWAY_IN 3      /* the Dense to Highwaynet.Size, where that is not Mel_Dim */
#define GSTTACO_VOC_HIGHWAY 4         /* the highway layers (relu | sigmoid in one GEMM) */
#define GSTTACO_VOC_DENSE 5           /* the Dense to Spectrogram_Dim behind the BiLSTM */
int gsttaco_vocoder_variants(const gsttaco_ctx* ctx, int which, int B, int Tf, int32_t variants[32], int32_t* count);
/* Test support, host only (no context, no device): the WINO_SPLIT_H plane builder as finalize runs it.  u: a float64 Winograd-domain
 * weight [al][cin][cout]; planes: [al][2][npad][wino_cin] fp16 bits (hi, lo of u[:, n] 2^su[n]); su: [cout]; *sv (may be NULL): the
 * power of two the kernel's input transform carries. */
int gsttaco_debug_wino_h_planes(const double* u, int al, int cin, int wino_cin, int cout, int npad, uint16_t* planes, int32_t* su,
                                int32_t* sv);

#ifdef __cplusplus
}
#endif
#endif /* GSTTACO_H */
