/* seedvc_hip.h -- C ABI of libseedvc_hip.so: the MI355X (gfx950) hot path of seed-vc inference.
 *
 * Every entry point replaces one seam of the reference's Python call surface.  The
 * caller (PyTorch-ROCm, or any C host) owns all input/output buffers; pointers are DEVICE pointers to
 * contiguous fp32 unless stated otherwise; work is enqueued on the caller's stream (hipStream_t passed
 * as void*; NULL = default stream).  The sampler, estimator and length-regulator calls do not synchronise the host in
 * steady state: HOST arrays (lengths) are copied into handle-owned pinned staging slots before the call returns, so the
 * caller may reuse them at once.  A call synchronises only when it has to grow the handle's workspace (first call, or a
 * larger batch / sequence than any before), svc_ar_generate / svc_ar_generate_batch[_seeded] read tokens back every `check_every`
 * steps, and the *_create functions finish packing before they return.  The library owns only packed weights and per-model workspace.  Every function returns 0 on success and non-zero on failure with a
 * message available from svc_last_error() (the Python shim re-raises it as RuntimeError, where the
 * reference raises Python exceptions: diffusion_transformer.py:121, inference.py:137,313).
 *
 * Devices and threading: a handle belongs to the device that was current when it was created, and must be used with
 * that device current (per-device state such as the zero page and kernel attributes is created lazily, once per device,
 * under a mutex).  Calls on one handle must be serialised by the caller (the reference is single-threaded Python under
 * torch.inference_mode, flow_matching.py:30); different handles may run concurrently on different streams.
 */
#ifndef SEEDVC_HIP_H
#define SEEDVC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVC_ABI_VERSION 1

/* One entry of an already-loaded state_dict (fp32, device memory).  Checkpoint ingestion itself stays
 * in the reference (modules/commons.py:412-479 build_model + load_checkpoint; bigvgan.py:413-492;
 * inference.py:118-119): the shim hands the loaded module's state_dict() to *_create. */
typedef struct svc_tensor_desc {
    const char* name;
    const float* data;
    int ndim;
    int64_t shape[4];
} svc_tensor_desc_t;

/* ---------------------------------------------------------------- DiT estimator + CFM sampler */
/* Hyper-parameters the reference reads from configs/presets/NAME.yml (model_params.DiT / .wavenet /
 * .style_encoder) or configs/v2/vc_wrapper.yaml (cfm.estimator). */
typedef struct svc_dit_config {
    int version;            /* 1: modules/diffusion_transformer.py DiT ; 2: modules/v2/dit_wrapper.py DiT */
    int hidden_dim, num_heads, depth, in_channels, content_dim, style_dim;
    int final_layer_type;   /* 0 = mlp, 1 = wavenet */
    int time_as_token, style_as_token, uvit_skip_connection, long_skip_connection, style_condition;
    int wn_hidden_dim, wn_num_layers, wn_kernel_size, wn_dilation_rate;
} svc_dit_config_t;

typedef struct svc_dit svc_dit_t;

/* Packs a DiT from `CFM.estimator.state_dict()` (keys listed in SURVEY.md 8b).  Replaces nothing in the
 * reference's loading code; it is what `model.cfm.estimator.setup_caches(...)` (inference.py:90) plus
 * the first forward would have prepared (RoPE table, skip lists). */
int svc_dit_create(const svc_dit_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights,
                   void* stream, svc_dit_t** out);
/* svc_dit_create with the arithmetic chosen; numbering follows the vocoders' `precision`.
 *   1  fp16 GEMM and attention operands, fp32 accumulation (svc_dit_create is create_ex(..., 1, ...), bit for bit).
 *   2  fp16x3 ("full precision"): every value that precision 1 rounds to fp16 on its way into a GEMM or the attention is carried
 *      as two fp16 planes, hi = half(v) and lo = half(v - float(hi)), and every product is hi*hi + lo*hi + hi*lo with fp32
 *      accumulation (the lo*lo term is dropped).  This covers the merge linear, QKV, wo, w1/w3, w2, the UViT and long skip
 *      linears, the mlp head, conv1 / conv2, the WaveNet in_layer / res_skip convs and FinalLayer, and QK^T and PV of the
 *      attention (P is split after the exponent; softmax statistics are fp32).  What is fp32 in precision 1 stays fp32: the
 *      time / style MLPs, the AdaLN tables, the residual stream, the norms, RoPE and the ODE state.  For users whose reference
 *      runs the sampler in fp32 (inference.py --fp16 False, CPU runs, the v2 timbre-only branch).
 * Any other value is refused before anything is allocated or launched: non-zero return, the reason in svc_last_error(), *out
 * untouched.  A handle has one precision for life (svc_dit_precision).  Its weights are packed once in that form: precision 2 packs
 * the split taps' sub-blocks [w_hi | w_lo | w_hi] per tap ([N][3][K]), so its weight memory is 3x the fp16 pack, and its workspace
 * holds a lo plane beside every fp16 operand plane plus one fp32 scratch of [rows][max(3 hidden, 2 ffn, 2 wn_hidden)].
 * On a precision-2 handle the fused row-panel kernel does not exist: svc_dit_fused_available returns 0, and
 * svc_dit_set_fused_min_rows / svc_dit_set_fused_seams succeed and change nothing.  Everything else works unchanged and keeps its
 * contracts (ragged batches equal the runs alone bit for bit, micro-batching, graph replay, seeds, per-row settings):
 * svc_cfm_sample, _seeded, _rows, svc_dit_forward, svc_dit_set_microbatch, svc_dit_set_graphs. */
int svc_dit_create_ex(const svc_dit_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, int precision,
                      void* stream, svc_dit_t** out);
/* 1 or 2: the precision the handle was created with (0 for NULL) */
int svc_dit_precision(svc_dit_t* m);
void svc_dit_destroy(svc_dit_t* m);

/* Utterances processed together inside one sampler call (micro-batch whose activations stay cache
 * resident); 0 restores the default. */
int svc_dit_set_microbatch(svc_dit_t* m, int utterances);

/* Transformer layers run on the fused row-panel kernel (one launch per layer besides attention, csrc/fused.hip) when a
 * launch covers at least `rows` token rows (streams x utterances x padded frames) and the width is supported (hidden_dim
 * 384 or 512); smaller launches use the tap-GEMM kernels.  rows < 0 restores the default (10240), 0 forces the fused
 * kernel, a huge value disables it.  The two paths agree to fp16-operand rounding (not bit for bit). */
int svc_dit_set_fused_min_rows(svc_dit_t* m, long rows);
/* Sampler seams run inside the fused row-panel launches of a step: bit 0 = the x block of the merge linear, the prefix-token
 * rows and the zeroed pad rows are built by the first panel (in_channels in (64, 128]); bit 1 = the mlp output head runs
 * in the last panel (final_layer_type mlp, in_channels a multiple of 16).  Default 3; unsupported bits are ignored; 0 issues
 * the separate launches (prefix rows, merge GEMM, two head GEMMs).  The two forms agree to fp16-operand rounding. */
int svc_dit_set_fused_seams(svc_dit_t* m, int mask);
int svc_dit_fused_available(svc_dit_t* m);
/* Optional (off by default: the sampler is GPU-bound on MI355X, replay measured 3 % slower than eager launches at B = 1):
 * the Euler loop of svc_cfm_sample (all steps of a micro-batch group: estimator + state update) is captured into a hipGraph
 * the second time a (batch, length, steps, guidance streams) combination is seen and replayed afterwards (the reference's
 * counterpart: `compile_cfm`, modules/v2/vc_wrapper.py:116-123).  The guidance rates and temperatures are not part of the
 * combination: the loop reads them from the handle's settings table.  Replays are bit-identical to eager runs.  on = 0 turns
 * capture off and drops the cached graphs; the environment variable SVC_DIT_GRAPH=0|1 overrides. */
int svc_dit_set_graphs(svc_dit_t* m, int on);

typedef struct svc_cfm_args {
    int B;                      /* utterances; each is an independent B=1 run of the reference sampler */
    int T;                      /* max frames (prompt + source) */
    int P;                      /* frames in `prompt` */
    const float* mu;            /* [B][T][content_dim]   (cat_condition) */
    const float* prompt;        /* [B][in_channels][P]   (mel2) */
    const float* style;         /* [B][style_dim]        (style2) */
    const float* z;             /* [B][in_channels][T]   noise: torch.randn in flow_matching.py:50 */
    const int64_t* x_lens;      /* HOST [B] valid frames per utterance (<= T); NULL = all T */
    const int64_t* prompt_lens; /* HOST [B] prompt frames per utterance (<= P); NULL = all P */
    int n_timesteps;
    float temperature;
    float cfg_rate[2];          /* v1: cfg_rate[0] = inference_cfg_rate ; v2: [intelligibility, similarity] */
    int random_voice;           /* v2 only (modules/v2/cfm.py:77-87) */
    float* out;                 /* [B][in_channels][T] */
} svc_cfm_args_t;

/* Replaces `model.cfm.inference(mu, x_lens, prompt, style, f0, n_timesteps, temperature,
 * inference_cfg_rate)` = BASECFM.inference + solve_euler (modules/flow_matching.py:30-112) and the v2
 * CFM.inference + solve_euler (modules/v2/cfm.py:16-132; cosine-warped t_span, 1/2/3-way CFG). */
int svc_cfm_sample(svc_dit_t* m, const svc_cfm_args_t* args, void* stream);

/* ---- seeded noise (sampler z, HiFT's SineGen draws): per-utterance seeds, draws made inside the consuming kernels.
 * One rule for every draw: Philox4x32-10 with key = (seed low word, seed high word) and counter = (pos, row / 4, domain, 0);
 * output word row % 4 belongs to element (row, pos).  Domains: 0 = the AR sampler's layout (svc_ar_generate_batch_seeded),
 * 1 = sampler z (row = mel channel, pos = frame), 2 = HiFT source noise (row = harmonic 0 .. nb_harmonics, pos = sample),
 * 3 = HiFT phase0 (row = harmonic, pos = 0): one seed may go to every stage of a request without a draw being reused.
 * Uniforms u = ((word >> 8) + 1) * 2^-24 in (0, 1]; normals by Box-Muller on word pairs, words (0, 1) -> rows 4q, 4q + 1 =
 * r cos(2 pi u1), r sin(2 pi u1) with r = sqrt(-2 ln u0), words (2, 3) -> rows 4q + 2, 4q + 3 (|n| <= 5.77); phase0 =
 * (2 u - 1) pi.  A draw is a pure function of (seed, domain, row, pos): the batch row, the padded T / S, the micro-batch and
 * the neighbours never enter it, and the first n positions of a row are the same whatever length is asked for.
 *
 * svc_cfm_sample with z[b] = the draws of seeds[b]: args->z is ignored (may be NULL), everything else as svc_cfm_sample.
 * seeds: HOST [B], consumed before the call returns.  Bit for bit svc_cfm_sample fed svc_cfm_noise_draws(seeds[b], C, T).
 * seeds == NULL, B < 1 or a handle of another device: non-zero, svc_last_error(), nothing enqueued. */
int svc_cfm_sample_seeded(svc_dit_t* m, const svc_cfm_args_t* args, const uint64_t* seeds, void* stream);
/* z (device, [C][T]) = the sampler noise of `seed`: what svc_cfm_sample_seeded draws for an utterance of that seed. */
int svc_cfm_noise_draws(uint64_t seed, int C, int T, float* z, void* stream);

/* ---- per-utterance sampler settings: steps, guidance and temperature of every utterance in one call.
 * The guidance rates and the temperature enter the sampler in two places only, the start state (temperature * z) and the
 * update x += dt (c0 v - ca v_a - cb v_b); the estimator never sees them.  Both read them per utterance from a small device
 * table, so utterances with different rates and temperatures share every launch.  What cannot be shared is the time grid (a
 * function of n_timesteps) and the set of guidance streams, so the batch is partitioned into CLASSES: two rows are in one
 * class when they have the same n_timesteps and the same guidance structure, which is the branch the sampler takes --
 * v1: cfg_rate[0] > 0 or not; v2: random_voice, then (0, 0), (0, rb), (ra, 0), (ra, rb).  The temperature and the values of
 * the rates never split a class.  A class runs like one svc_cfm_sample call over its members in batch order (micro-batches
 * of the handle's size over that list); the classes run one after the other on the stream, numbered by first appearance.
 * Members of a class need not be adjacent: mu / prompt / style / z are read and out is written through a row map, nothing
 * is gathered or copied.
 *
 * Contract.  (a) Rows that all carry one setting give bit for bit the result of svc_cfm_sample[_seeded] with that setting
 * (they are the same code: the uniform entries are this one with B copies of args' setting).  (b) In general the call is bit
 * for bit the sequence of svc_cfm_sample[_seeded] runs over each class's members stacked in batch order -- so a class whose
 * members share all four settings equals the existing call on those rows.  (c) Every row is an independent B = 1 run of the
 * reference sampler with its own settings.
 * With svc_dit_set_graphs the captured loop is keyed by the class shape and reads the settings table at replay: a replay
 * with other rates or temperatures uses the new ones. */
typedef struct svc_cfm_row {          /* HOST, one per utterance */
    int32_t n_timesteps;              /* >= 1 */
    float   temperature;
    float   cfg_rate[2];              /* v1: [0] ; v2: [intelligibility, similarity] */
    int32_t random_voice;             /* v2 only */
} svc_cfm_row_t;

/* svc_cfm_sample / _seeded with the four settings taken per row (args->n_timesteps, temperature, cfg_rate, random_voice
 * are ignored).  rows: HOST [B], consumed before the call returns.  seeds: HOST [B] or NULL (then args->z).
 * Refused before anything is enqueued, with svc_last_error(): rows == NULL, n_timesteps < 1, a non-finite temperature or
 * rate, random_voice on a v1 handle, seeds and args->z both NULL, and everything svc_cfm_sample refuses. */
int svc_cfm_sample_rows(svc_dit_t* m, const svc_cfm_args_t* args, const svc_cfm_row_t* rows,
                        const uint64_t* seeds, void* stream);
/* The partition svc_cfm_sample_rows uses for a handle of `version` (1 or 2); needs no GPU.  class_of[b] (HOST [B]) = class
 * of row b, classes numbered by first appearance; n_streams[c] (HOST, room for B) = guidance streams of class c (estimator
 * evaluations per step: 1, 2 or 3).  Either may be NULL.  Returns the number of classes, < 0 on bad rows (svc_last_error()). */
int svc_cfm_rows_plan(int version, const svc_cfm_row_t* rows, int B, int32_t* class_of, int32_t* n_streams);

/* Replaces one estimator evaluation `estimator(x, prompt_x, x_lens, t, style, mu)` =
 * DiT.forward (modules/diffusion_transformer.py:486-537, modules/v2/dit_wrapper.py:114-152).
 * x, prompt_x, out: [N][in_channels][T]; style [N][style_dim]; mu [N][T][content_dim]; t scalar
 * (the sampler always passes one t for the whole batch). x_lens HOST [N] or NULL. */
int svc_dit_forward(svc_dit_t* m, int N, int T, const float* x, const float* prompt_x, const int64_t* x_lens,
                    float t, const float* style, const float* mu, float* out, void* stream);

/* ---------------------------------------------------------------- vocoders */
typedef struct svc_bigvgan_config {   /* modules/bigvgan/config.json */
    int num_mels, upsample_initial_channel, num_upsamples, num_kernels;
    int upsample_rates[8], upsample_kernel_sizes[8];
    int resblock_kernel_sizes[4], resblock_dilation_sizes[4][3];
    int use_tanh_at_final, use_bias_at_final, snake_logscale, snakebeta;
    int precision;                    /* 0 = fp32 MFMA (exact); 1 = plain fp16 operands (RMS 2.4e-4: outside the 1e-4 bound,
                                         reported only); 2 = fp16x3: hi/lo fp16 split of both operands, three MFMA products,
                                         fp32 accumulate (RMS <= 2e-6); 3 = fp16p8: as 2, but on the long stride-1 convs the
                                         two correction products run as ONE block-scaled fp8 MFMA (RMS 6e-6 at S = 430
                                         against the reference; bound 1e-4) -- the value the Python mirrors pass by default */
} svc_bigvgan_config_t;
typedef struct svc_bigvgan svc_bigvgan_t;
int svc_bigvgan_create(const svc_bigvgan_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights,
                       void* stream, svc_bigvgan_t** out);
void svc_bigvgan_destroy(svc_bigvgan_t* m);
/* Replaces `vocoder_fn(mel)` = BigVGAN.forward (modules/bigvgan/bigvgan.py:360-386).
 * mel [B][num_mels][S] -> out [B][1][S * prod(upsample_rates)]. */
int svc_bigvgan_forward(svc_bigvgan_t* m, const float* mel, int B, int S, float* out, void* stream);
/* The same for a batch of utterances of different lengths, in one call (HiFT: svc_hift_forward_ragged below).
 * mel [B][num_mels][S]; lens HOST [B], 0 <= lens[b] <= S; out [B][1][S * up], up = prod(upsample_rates).
 * out[b][0][: lens[b] * up] is the waveform of mel[b][:, :lens[b]] run alone (its convs zero-pad and its anti-aliased
 * activations replicate at the utterance's own last frame); every sample at and above lens[b] * up is written as zero, and
 * lens[b] == 0 gives an all-zero row.  Mel frames at and above lens[b] are never read as values: they may hold anything, NaN
 * included.  "Run alone" is bit for bit what svc_bigvgan_forward returns for (1, num_mels, lens[b]) when lens[b] >= 192,
 * whatever the other utterances, their order and the micro-batch size; below 192 frames a layer may take another kernel
 * form in the padded batch than alone (the resident-tile / fp8-correction convs need 192 output rows), and the two agree
 * within the precision's bound against the reference instead (waveform RMS < 1e-4).  Equal lengths (lens[b] == S for all b)
 * give svc_bigvgan_forward's result bit for bit.
 * lens is consumed before the call returns (pinned staging of the handle; no host synchronisation in steady state); B is not
 * limited.  The utterances run longest first in micro-batches (svc_bigvgan_set_microbatch), each padded to its own longest
 * member.  lens == NULL, a length outside [0, S], B < 1 or S < 1: error (svc_last_error), nothing enqueued. */
int svc_bigvgan_forward_ragged(svc_bigvgan_t* m, const float* mel, const int32_t* lens, int B, int S, float* out, void* stream);

typedef struct svc_hift_config {      /* configs/hifigan.yml */
    int in_channels, base_channels, nb_harmonics, sampling_rate;
    float nsf_alpha, nsf_sigma, nsf_voiced_threshold;
    int num_upsamples, upsample_rates[4], upsample_kernel_sizes[4];
    int istft_n_fft, istft_hop;
    int num_kernels, resblock_kernel_sizes[4], resblock_dilation_sizes[4][3];
    int source_resblock_kernel_sizes[4], source_resblock_dilation_sizes[4][3];
    float lrelu_slope, audio_limit;
    int f0_cond_channels;
    int precision;                    /* 0 fp32 / 1 fp16 / 2 fp16x3 / 3 fp16p8, as svc_bigvgan_config.precision */
} svc_hift_config_t;
typedef struct svc_hift svc_hift_t;
int svc_hift_create(const svc_hift_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights,
                    void* stream, svc_hift_t** out);
void svc_hift_destroy(svc_hift_t* m);
/* Replaces `vocoder_fn(mel)` = HiFTGenerator.forward (modules/hifigan/generator.py:400-436).
 * mel [B][80][S]; f0 [B][S] or NULL (NULL -> the model's f0_predictor, f0_predictor.py:51-55);
 * phase0 [B][nb_harmonics+1][1] = the U(-pi,pi) draw of SineGen (generator.py:208-210);
 * noise [B][nb_harmonics+1][S*up] = its randn_like draw (generator.py:222);  out [B][S*up].
 * f0_out (optional, [B][S]) receives the f0 actually used. */
int svc_hift_forward(svc_hift_t* m, const float* mel, const float* f0, const float* phase0, const float* noise,
                     int B, int S, float* out, float* f0_out, void* stream);
/* The same for a batch of utterances of different lengths, in one call (the contract of svc_bigvgan_forward_ragged).
 * lens: HOST int32 [B], 0 <= lens[b] <= S, consumed before the call returns (pinned staging inside the handle: no host
 * synchronisation in steady state).  mel [B][80][S]; f0 [B][S] or NULL; phase0 [B][nb_harmonics+1][1]; noise
 * [B][nb_harmonics+1][S*up], of which row b uses the first lens[b]*up samples of each harmonic: the draws of the run alone.
 * out[b][0 .. lens[b]*up) is the waveform of mel[b][:, :lens[b]] run alone through svc_hift_forward, bit for bit (an
 * utterance runs the kernels it would run alone: micro-batches never mix utterances whose convs choose differently);
 * out[b][lens[b]*up ..] and f0_out[b][lens[b] ..] (f0_out optional, [B][S]) are written as zero; lens[b] == 0 gives a zero
 * row.  Mel frames, f0 values and noise samples at and above an utterance's end are never read as values (they may hold
 * NaN): every conv bounds its operand load by the utterance's rows, the source stops at its last sample, and the STFT /
 * iSTFT reflect and overlap-add at its own end.  Utterances run longest first in micro-batches
 * (svc_hift_set_microbatch), each padded to its own longest member.  Errors (lens NULL or out of range, B < 1, S < 1)
 * return non-zero with nothing enqueued. */
int svc_hift_forward_ragged(svc_hift_t* m, const float* mel, const int32_t* lens, const float* f0, const float* phase0,
                            const float* noise, int B, int S, float* out, float* f0_out, void* stream);
/* svc_hift_forward (lens == NULL) / svc_hift_forward_ragged (lens HOST [B]) with phase0[b] and noise[b] = the draws of
 * seeds[b] (the rule above svc_cfm_sample_seeded), made inside the source kernel: no [B][nb_harmonics+1][S*up] tensor exists,
 * in the caller's memory or the handle's.  seeds: HOST [B], consumed before the call returns.  Bit for bit the explicit call
 * fed svc_hift_noise_draws(seeds[b], nb_harmonics + 1, S * up); with lens, out[b][0 .. lens[b]*up) is utterance b run alone
 * with its seed, bit for bit, whatever the other rows, S and the micro-batch.  seeds == NULL, B < 1, S < 1, a length outside
 * [0, S] or a handle of another device: non-zero, svc_last_error(), nothing enqueued. */
int svc_hift_forward_seeded(svc_hift_t* m, const float* mel, const int32_t* lens, const float* f0, const uint64_t* seeds, int B,
                            int S, float* out, float* f0_out, void* stream);
/* phase0 (device, [NH]) and noise (device, [NH][n]) of `seed`, NH = nb_harmonics + 1, n = samples (< 2^31): the tensors the
 * explicit calls take for one utterance. */
int svc_hift_noise_draws(uint64_t seed, int NH, long n, float* phase0, float* noise, void* stream);
/* Utterances per internal pass of the vocoders (0 = default 32); results do not depend on it. */
int svc_bigvgan_set_microbatch(svc_bigvgan_t* m, int utterances);
int svc_hift_set_microbatch(svc_hift_t* m, int utterances);

/* ---- precision plan of an fp16p8 handle (precision 3): which convs run as fp16 + fp8 corrections.
 * The fp8 correction bytes have a fixed window: activations carry no scale (bytes fp8(hi), fp8(2^11 lo), clamp +-448), weights
 * one power-of-two scale per layer.  A conv whose operands lie outside it silently falls back to plain-fp16 operand error.
 * The plan holds one veto per CANDIDATE conv; a vetoed conv runs the fp16x3 form instead (and whoever writes its operand planes
 * writes fp16 residuals): a layer property, never the batch's, so batched, ragged and micro-batched runs stay bit-identical
 * to the run alone under any plan.  The empty plan (the default) is today's fp16p8, launch for launch; the full plan gives
 * the bits of a precision-2 (fp16x3) handle.
 * Candidates: the ResBlock convs that own the fp8 weight packing (k >= 3, at least 64 padded channels in and out), in model
 * order: BigVGAN resblocks.<i> for i ascending, HiFT per stage i source_resblocks.<i> then resblocks.<i * num_kernels + j>;
 * inside a ResBlock convs1.<d>, convs2.<d> for d ascending.  svc_*_plan_name gives candidate i's state-dict prefix (e.g.
 * "resblocks.3.convs2.1"; valid while the handle lives; NULL out of range), so a plan can be stored next to a checkpoint and
 * restored with svc_*_plan_set without calibration data.
 * get / set: veto[n] bytes (0 = runs p8), n == svc_*_plan_size(m).  reset clears every veto.  All of them, and calibrate,
 * are host-side state changes of the handle: call them between forwards, not concurrently with one.
 * Refused (non-zero, svc_last_error(), plan untouched): a NULL argument, a handle of another precision, n != plan size. */
int svc_bigvgan_plan_size(svc_bigvgan_t* m);          /* -1: NULL handle or not an fp16p8 handle */
const char* svc_bigvgan_plan_name(svc_bigvgan_t* m, int i);
int svc_bigvgan_plan_get(svc_bigvgan_t* m, uint8_t* veto, int n);
int svc_bigvgan_plan_set(svc_bigvgan_t* m, const uint8_t* veto, int n);
int svc_bigvgan_plan_reset(svc_bigvgan_t* m);
/* One census record (csrc/range_census.hip): counts over the live elements of a conv's operand planes (hi fp16, lo fp16
 * residual) and the energy of each term and of what its fp8 byte loses; the bytes are those of the hardware convert the p8
 * producers use.  n: hi != 0; n_hi_clamp: |hi| > 448; n_hi_sub: 0 < |hi| < 2^-6 (e4m3 subnormal); n_lo_flush: lo != 0 whose
 * byte fp8(2^11 lo) is zero; n_lo_clamp: |2^11 lo| > 448; s_hi2 = sum hi^2, s_hi_err2 = sum (hi - dq fp8(hi))^2, s_lo2 =
 * sum lo^2, s_lo_err2 = sum (lo - 2^-11 dq fp8(2^11 lo))^2. */
typedef struct svc_census {
    int64_t n, n_hi_clamp, n_hi_sub, n_lo_flush, n_lo_clamp;
    double max_hi;
    double s_hi2, s_hi_err2, s_lo2, s_lo_err2;
} svc_census_t;
/* One report row of calibrate.  rho = s_lo_err2 / s_lo2 and eta = s_hi_err2 / s_hi2 of the conv's activation planes (0 for an
 * all-zero term); omega_hi / omega_lo: the same two ratios of its weight bytes, the largest over the output channels
 * (all-zero channels exempt); L: the conv's rows per utterance (of the longest utterance); veto: THIS call's decision (the
 * plan holds the OR of all calls since the last reset / set). */
typedef struct svc_plan_row {
    int32_t index, veto, L, reserved;
    double rho, eta, omega_hi, omega_lo;
    svc_census_t census;
} svc_plan_row_t;
/* Calibrates the plan on the caller's own material: runs ONE forward with every candidate vetoed (the fp16x3 forward, so all
 * operand planes are in the fp16 format; its waveform is discarded), takes the census of each candidate's operand planes at
 * the point the conv consumes them (rows at and above an utterance's end are never read), combines it with the weight
 * census, vetoes a conv when rho, eta or an omega exceeds tau, ORs the vetoes into the plan -- several calls on different
 * material accumulate -- and fills rows[i] for candidate i.  mel [B][num_mels][S]; lens HOST [B], 1 <= lens[b] <= S, or
 * NULL (all S).  tau in (0, 1]; the default of the Python mirrors is 2^-6 (it rests on a CPU
 * simulation of one conv).  Deterministic: counts are integers and every sum has one fixed order, so equal material gives
 * equal rows and the same plan.  Synchronises the stream.
 * Refused before any launch (non-zero, svc_last_error(), plan untouched): a handle that is not fp16p8, NULL m / mel / rows,
 * n_rows != plan size, tau outside (0, 1] or NaN, B or S < 1, B * S * up >= 2^31, a lens entry outside [1, S]. */
int svc_bigvgan_calibrate(svc_bigvgan_t* m, const float* mel, const int32_t* lens, int B, int S, float tau, svc_plan_row_t* rows,
                          int n_rows, void* stream);
/* The same for HiFT; f0 / phase0 / noise as in svc_hift_forward(_ragged) (f0 may be NULL: the model's predictor). */
int svc_hift_plan_size(svc_hift_t* m);
const char* svc_hift_plan_name(svc_hift_t* m, int i);
int svc_hift_plan_get(svc_hift_t* m, uint8_t* veto, int n);
int svc_hift_plan_set(svc_hift_t* m, const uint8_t* veto, int n);
int svc_hift_plan_reset(svc_hift_t* m);
int svc_hift_calibrate(svc_hift_t* m, const float* mel, const int32_t* lens, const float* f0, const float* phase0, const float* noise,
                       int B, int S, float tau, svc_plan_row_t* rows, int n_rows, void* stream);

/* ---------------------------------------------------------------- v2 AR model (decode step, B = 1 and batched) */
typedef struct svc_ar_config {        /* configs/v2/vc_wrapper.yaml:39-53 (modules.v2.ar.NaiveModelArgs) */
    int dim, n_head, n_local_heads, head_dim, n_layer, intermediate_size, vocab_size, max_seq_len;
    float rope_base, norm_eps;
} svc_ar_config_t;
typedef struct svc_ar svc_ar_t;
/* Packs `NaiveWrapper.state_dict()` (keys model.layers.N.*, model.norm, model.output); allocates the fp32 KV cache
 * that `setup_caches(1, max_seq_len)` would (modules/v2/ar.py:160-179). */
int svc_ar_create(const svc_ar_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream, svc_ar_t** out);
void svc_ar_destroy(svc_ar_t* m);
int svc_ar_reset(svc_ar_t* m, void* stream);      /* zero the KV cache (slot 0, the cache of the B = 1 calls) */
/* Replaces `model.forward_generate(x, input_pos, kv_pos)` (modules/v2/ar.py:239-267) for B = 1: x [S][dim] fp32,
 * input_pos / kv_pos HOST [S]; logits_out [vocab] = logits of the last token. */
int svc_ar_forward_generate(svc_ar_t* m, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos,
                            float* logits_out, void* stream);
/* The same one-token step replayed from a captured hipGraph (replaces `compiled_decode_fn`, the
 * torch.compile(mode="reduce-overhead") step of modules/v2/vc_wrapper.py:105-114).  set_pos != 0 (re)sets the device
 * positions; every call afterwards advances input_pos and kv_pos by one (ar.py:402-403).  Refused before anything is
 * launched: a call without set_pos that is not preceded by one (or that follows another B = 1 call -- svc_ar_forward_generate,
 * svc_ar_generate -- which rewrite the device positions), and a replay whose position has reached max_seq_len. */
int svc_ar_decode_step(svc_ar_t* m, const float* x, int set_pos, int64_t input_pos, int64_t kv_pos, float* logits_out,
                       void* stream);
/* Replaces the token loop of `NaiveWrapper.generate(prompt_text, prompt_target, ...)` (modules/v2/ar.py:382-422), B = 1
 * (SURVEY.md 8f row 4).  x_prefill [S][dim] = [sep, prompt_text, sep, embed(prompt_target)] as the reference builds it
 * (ar.py:390-396), input_pos / kv_pos HOST [S]; exp_noise device [max_new][vocab] = the Exp(1) draws of
 * multinomial_sample_one_no_sync, row t for token t; EOS (vocab-1) is suppressed while fewer than
 * min_tokens_before_eos (reference: 10) tokens exist; the host inspects the tokens every `check_every` steps only.
 * tokens_out device [max_new]; *n_tokens = tokens generated before EOS (<= max_new; reference cap 4001).
 * Needs `model.embeddings.weight` in the state dict given to svc_ar_create. */
int svc_ar_generate(svc_ar_t* m, const float* x_prefill, int S, const int64_t* input_pos, const int64_t* kv_pos,
                    const float* exp_noise, int max_new, int min_tokens_before_eos, float temperature, float top_p,
                    float repetition_penalty, int check_every, int32_t* tokens_out, int32_t* n_tokens, void* stream);
/* ---- batched AR: up to 64 sequences per decode step, each in its own SLOT (KV cache, input_pos, kv_pos).
 * The calls above are the B = 1 path and work on slot 0, the cache svc_ar_create allocates; they are unaffected by the
 * calls below.  One batched step reads every weight byte once for all slots (skinny MFMA GEMMs, M = B padded to 16 rows).
 * A slot's result is bit-identical whatever B is, whichever slot it is given and whatever the other slots hold: no
 * atomics, every reduction in a fixed order.  Cache rows at or above a sequence's kv_pos never reach its result as
 * values (the batched attention addresses rows 0 .. kv_pos only), so a slot needs no reset between sequences.
 *
 * svc_ar_set_max_batch: 1 <= max_batch <= 64.  Allocates (or frees) the fp32 caches of slots 1 .. max_batch - 1,
 * n_layer * 2 * n_local_heads * max_seq_len * 64 * 4 bytes each (25 MB for ar_base at 4096 positions).  Synchronises. */
int svc_ar_set_max_batch(svc_ar_t* m, int max_batch, void* stream);
/* svc_ar_forward_generate on the cache of slot `slot` (0 <= slot < max_batch). */
int svc_ar_prefill_slot(svc_ar_t* m, int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos,
                        float* logits_out, void* stream);
/* One token for each of slots 0 .. B-1 from a captured hipGraph (one per padded batch 16 / 32 / 48 / 64): x [B][dim],
 * logits_out [B][vocab].  set_pos != 0 (re)sets the device positions from input_pos / kv_pos HOST [B] (required on the
 * first step of a batch and after svc_ar_generate_batch); every call afterwards advances both by one per slot. */
int svc_ar_decode_step_batch(svc_ar_t* m, int B, const float* x, int set_pos, const int64_t* input_pos, const int64_t* kv_pos,
                             float* logits_out, void* stream);
/* B independent svc_ar_generate loops in one (sequence b in slot b).  x_prefill: the prefill rows of all sequences
 * concatenated, [sum S][dim]; S HOST [B]; input_pos / kv_pos HOST [sum S], concatenated alike; exp_noise device
 * [B][max_new][vocab]; tokens_out device [B][max_new]; n_tokens HOST [B].  A sequence that has drawn EOS, holds max_new
 * tokens or has filled its cache is masked, not compacted: its slot keeps running and records nothing more.  The host
 * reads the slots' counters every `check_every` steps and returns once every sequence is finished. */
int svc_ar_generate_batch(svc_ar_t* m, int B, const float* x_prefill, const int32_t* S, const int64_t* input_pos,
                          const int64_t* kv_pos, const float* exp_noise, int max_new, int min_tokens_before_eos, float temperature,
                          float top_p, float repetition_penalty, int check_every, int32_t* tokens_out, int32_t* n_tokens,
                          void* stream);
/* svc_ar_generate_batch with the Exp(1) draws generated inside the sampler instead of read from a tensor: seeds HOST [B],
 * one per sequence.  The draw for vocabulary entry v at token step t (0 = the first generated token) of sequence b is
 * q = -log(u), u = ((w >> 8) + 1) * 2^-24 in (0, 1], where w is output word v % 4 of Philox4x32-10 with key
 * (seeds[b] & 0xffffffff, seeds[b] >> 32) and counter (v / 4, t, 0, 0): a function of (seed, t, v) alone, so the slot
 * contract above holds unchanged, and B = 1 is the single-sequence case (slot 0).  No [B][max_new][vocab] buffer exists. */
int svc_ar_generate_batch_seeded(svc_ar_t* m, int B, const float* x_prefill, const int32_t* S, const int64_t* input_pos,
                                 const int64_t* kv_pos, const uint64_t* seeds, int max_new, int min_tokens_before_eos,
                                 float temperature, float top_p, float repetition_penalty, int check_every, int32_t* tokens_out,
                                 int32_t* n_tokens, void* stream);
/* out device [n_steps][vocab] = exactly the draws the seeded sampler uses for `seed` at steps step0 .. step0 + n_steps - 1
 * (handing them to svc_ar_generate_batch as exp_noise reproduces the seeded run bit for bit). */
int svc_ar_exp_draws(svc_ar_t* m, uint64_t seed, int step0, int n_steps, float* out, void* stream);
/* ---- ragged prefill and sessions (continuous batching).
 * svc_ar_prefill_batch: svc_ar_prefill_slot for n sequences in one pass.  Sequence i goes to the cache of slots[i]
 * (HOST [n], distinct, 0 <= slot < max_batch, not occupied by a session); x [sum S][dim], S HOST [n], input_pos / kv_pos
 * HOST [sum S] are concatenated the way svc_ar_generate_batch takes them; logits_out device [n][vocab] = the logits of
 * each sequence's last row.  Norms and linears run over all rows in one launch each (always the tap-GEMM, whatever S is),
 * RoPE / cache scatter and the causal GQA attention (fp32 MFMA, flash-style; csrc/ar_prefill_attn.h) find every row's slot
 * through per-pass tables that are uploaded once.  A pass takes at most 8192 rows (svc_ar_set_prefill_rows lowers that, to
 * max_seq_len at the least); a call with more rows runs as several passes of whole sequences.
 * Contract: a sequence's logits and the cache rows it writes are bit-identical whether it is prefilled alone or with any
 * companions, in any slot, at any place in the concatenation.  Rows above a sequence's prefix never reach its result, not
 * even as 0 x value.  Against svc_ar_prefill_slot the results agree to the logit tolerance, not bit for bit (another
 * summation order in the attention; no GEMV form for short sequences).  Arguments are checked before anything is launched. */
int svc_ar_prefill_batch(svc_ar_t* m, int n, const int32_t* slots, const float* x, const int32_t* S, const int64_t* input_pos,
                         const int64_t* kv_pos, float* logits_out, void* stream);
int svc_ar_set_prefill_rows(svc_ar_t* m, int rows);   /* rows of one pass: max_seq_len .. 8192 (default 8192) */
int svc_ar_prefill_passes(svc_ar_t* m);               /* passes the last ragged prefill ran as */
/* One request of svc_ar_admit.  Everything svc_ar_generate_batch takes per call is per request here. */
typedef struct svc_ar_request {
    int32_t slot;                 /* a free slot, 0 <= slot < max_batch */
    int32_t S;                    /* its prefill rows */
    const float* exp_noise;       /* device [max_new][vocab] Exp(1) draws, or NULL: the sampler draws them from `seed` */
    uint64_t seed;
    int32_t max_new;              /* >= 1 */
    int32_t min_tokens_before_eos;
    float temperature, top_p, repetition_penalty;
    int32_t* tokens_out;          /* device [max_new]; must outlive the request (until svc_ar_retire) */
} svc_ar_request_t;
/* svc_ar_admit: one ragged prefill for the n newcomers (rows concatenated in request order), each one's first token, then
 * ONLY these slots' loop state, positions and next-input row are written, all on the stream: slots in mid-sequence are not
 * disturbed.  A request that is finished at admission (max_new == 1, cache full) is admitted as finished.  The first admit
 * opens a SESSION; it is active until every slot is retired.  While it is active svc_ar_generate_batch[_seeded],
 * svc_ar_decode_step_batch and svc_ar_set_max_batch fail with "a session is active" (they share the slot state), and so do
 * the B = 1 calls and svc_ar_prefill_slot / _batch on an occupied slot (B = 1: slot 0).  With no session active everything
 * behaves as before.  Synchronises.
 * svc_ar_run: n_steps replays of the captured generate graph over slots 0 .. highest occupied one (free slots below it sit
 * in the batch as finished slots and record nothing), then one read of the slots' counters: n_tokens / done HOST
 * [max_batch] (a free slot reports 0 / 1).  A slot's tokens are tokens_out[0 .. n_tokens).
 * svc_ar_retire: frees a slot (finished or not; a running sequence stops recording).  Its tokens stay in tokens_out.
 * Contract: a request's tokens are a function of its own inputs alone -- bit-identical to the same request admitted alone
 * and run to completion, whatever else is in flight, whichever slot it gets, however n_steps is chosen, whenever admitted. */
int svc_ar_admit(svc_ar_t* m, int n, const svc_ar_request_t* requests, const float* x_prefill, const int64_t* input_pos,
                 const int64_t* kv_pos, void* stream);
int svc_ar_run(svc_ar_t* m, int n_steps, int32_t* n_tokens, int32_t* done, void* stream);
int svc_ar_retire(svc_ar_t* m, int slot, void* stream);
int svc_ar_session_active(svc_ar_t* m);               /* occupied slots; 0 = no session */
/* Replaces `sample(logits, previous_tokens, suppress_tokens, temperature, top_p, repetition_penalty)`
 * (modules/v2/ar.py:712-763): repetition penalty, top-p, temperature softmax, argmax(probs / q) with q = exp_noise
 * (the Exp(1) draw of multinomial_sample_one_no_sync, supplied by the caller).  suppress_token < 0 = none;
 * suppress_token >= vocab is refused.  Vocabulary <= 4096.
 * Contract, in order: the penalty (score < 0 ? score * rp : score / rp) is taken from the ORIGINAL logit of every
 * previous token (duplicates do not compound); then suppression; the descending order is torch's stable one (ties: lower
 * index first); the cumulative sum of exp(s - s0) is NORMALISED BY ITS OWN TOTAL before it is compared with top_p, so its
 * last value is exactly 1 and top_p >= 1 removes nothing (a softmax-then-cumsum may overshoot 1 by an ulp and drop tail
 * tokens at top_p = 1); an entry is removed where that value > top_p, never the first; the kept logits are divided by
 * max(temperature, 1e-5); softmax; the winner is argmax(probs / q), ties to the lower index.
 * Not specified: NaN logits, and a vector whose entries are all -inf. */
int svc_ar_sample(svc_ar_t* m, const float* logits, const int32_t* prev_tokens, int n_prev, int suppress_token,
                  float temperature, float top_p, float repetition_penalty, const float* exp_noise, int32_t* idx_out,
                  float* probs_out, void* stream);

/* ---------------------------------------------------------------- length regulator */
typedef struct svc_lr_config {        /* modules/length_regulator.py:29-88, modules/v2/length_regulator.py:28-72 */
    int channels, in_channels, out_channels;
    int is_discrete, codebook_size;   /* discrete: token ids through `embedding`; else `content_in_proj` */
    int n_convs;                      /* len(sampling_ratios): Conv1d(k3) + GroupNorm(1) + Mish blocks */
    int interpolate;                  /* len(sampling_ratios) > 0 */
    int has_final_conv;               /* v1: always; v2: only when out_channels != channels (else nn.Identity) */
    int f0_condition, n_f0_bins;
} svc_lr_config_t;
typedef struct svc_lr svc_lr_t;
/* Packs `InterpolateRegulator.state_dict()` (keys model.N.*, embedding.weight, content_in_proj.*, f0_embedding.weight,
 * f0_mask). */
int svc_lr_create(const svc_lr_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream, svc_lr_t** out);
void svc_lr_destroy(svc_lr_t* m);
/* Replaces `length_regulator(x, ylens=..., n_quantizers=..., f0=...)[0]` (modules/length_regulator.py:90-141; v2
 * modules/v2/length_regulator.py:74-105) for a batch of independent utterances.
 * x [B][tin_max][in_channels] fp32 (continuous) or tokens [B][tin_max] int64 (discrete); in_lens / ylens / f0_lens are
 * HOST arrays [B]; f0 [B][tf0_max] Hz or NULL (NULL with f0_condition -> `f0_mask`); out [B][tout_max][out_channels],
 * rows >= ylens[b] zero (the reference's `out * mask`). */
int svc_lr_forward(svc_lr_t* m, const float* x, const int64_t* tokens, const int32_t* in_lens, int B, int tin_max,
                   const int32_t* ylens, int tout_max, const float* f0, const int32_t* f0_lens, int tf0_max, float* out,
                   void* stream);

/* ---------------------------------------------------------------- ragged assembly of a v2 batch
 * Both write every element of `out`, padding included; lengths are HOST int32 [B] and are consumed before the call
 * returns (they travel as kernel arguments: no copy to wait for, no synchronisation).
 *
 * Replaces `cat_condition = torch.cat([prompt_condition, cond], dim=1)` (modules/v2/vc_wrapper.py:657-660) for B
 * utterances of different lengths: out[b] = cat(prompt_cond[b][:prompt_lens[b]], cond[b][:cond_lens[b]]), rows at and
 * above prompt_lens[b] + cond_lens[b] zero.  prompt_cond [B][Pmax][Dc], cond [B][Smax][Dc], out [B][T][Dc];
 * prompt_lens[b] + cond_lens[b] <= T. */
int svc_v2_assemble_cond(const float* prompt_cond, const int32_t* prompt_lens, const float* cond, const int32_t* cond_lens, int B,
                         int Pmax, int Smax, int Dc, int T, float* out, void* stream);
/* Replaces `vc_mel[:, :, prompt_len:original_len]` (modules/v2/vc_wrapper.py:700) for a ragged batch: mel [B][C][T],
 * out [B][C][Smax]; out[b][c][s] = mel[b][c][prompt_lens[b] + s] for s < x_lens[b] - prompt_lens[b], else pad_value.
 * x_lens[b] <= T and x_lens[b] - prompt_lens[b] <= Smax. */
int svc_mel_strip_prompt(const float* mel, const int32_t* prompt_lens, const int32_t* x_lens, int B, int C, int T, int Smax,
                         float pad_value, float* out, void* stream);

/* Replaces the reference's only native seam: anti_alias_activation_cuda.forward(inputs, up_ftr,
 * down_ftr, alpha, beta) (modules/bigvgan/alias_free_activation/cuda/anti_alias_activation.cpp:19-23,
 * anti_alias_activation_cuda.cu:43-246).  x, y: [B][C][L]; dtype 0 = fp32, 1 = fp16, 2 = bf16;
 * up12 / down12: 12 filter taps (fp32); log_alpha / log_beta: [C] log-scale SnakeBeta parameters
 * (exp is applied in the kernel, as in the reference kernel). Accumulates in fp32 for every dtype. */
int svc_anti_alias_act_fwd(const void* x, void* y, const float* up12, const float* down12,
                           const float* log_alpha, const float* log_beta, int B, int C, int L, int dtype,
                           void* stream);

/* ---------------------------------------------------------------- log-mel front-end (first half) */
typedef struct svc_mel svc_mel_t;
/* Replaces `mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)`
 * (modules/audio.py:45-82).  window [win] = torch.hann_window(win_size), mel_basis [n_mels][n_fft/2+1] =
 * librosa.filters.mel(...) as the reference caches them (device fp32); win must equal n_fft (all presets). */
int svc_mel_create(int n_fft, int hop, int win, int n_mels, const float* window, const float* mel_basis, void* stream,
                   svc_mel_t** out);
void svc_mel_destroy(svc_mel_t* m);
int svc_mel_frames(const svc_mel_t* m, int L);          /* frames for L samples: 1 + (L - hop) / hop */
/* y [B][L] fp32 in [-1, 1] -> out [B][n_mels][frames] = log(clamp(mel @ sqrt(|STFT|^2 + 1e-9), 1e-5)). */
int svc_mel_forward(svc_mel_t* m, const float* y, int B, int L, float* out, void* stream);
/* The same for a batch of clips of different lengths, in one call (the contract of the ragged vocoder calls).
 * y [B][L]; lens HOST int32 [B], consumed before the call returns (pinned staging inside the handle: no host synchronisation in
 * steady state); out [B][n_mels][svc_mel_frames(L)].  out[b][:, :svc_mel_frames(lens[b])] is the log-mel of y[b][:lens[b]] run
 * alone through svc_mel_forward (the reflect padding happens at the clip's own end, and a frame's row of the two GEMMs does not
 * depend on its neighbours); every frame at and above that count is written as pad_value.  Samples at and above lens[b] are
 * never read as values: they may hold anything, NaN included.  lens[b] == L for all b gives svc_mel_forward's result bit for bit.
 * Legal lengths: (n_fft - hop) / 2 < lens[b] <= L and lens[b] >= hop (svc_mel_min_len <= lens[b] <= L).  lens == NULL, a length outside that range or B < 1:
 * non-zero, a svc_last_error() that names lens, nothing enqueued; the checks that do not need n_fft and hop come before the
 * handle is touched.  Workspace grows with B * L (the padded signal and three [B * frames] matrices). */
int svc_mel_min_len(int n_fft, int hop);               /* the shortest legal lens[b]: max((n_fft - hop) / 2 + 1, hop); needs no handle */
int svc_mel_forward_ragged(svc_mel_t* m, const float* y, const int32_t* lens, int B, int L, float pad_value, float* out, void* stream);

/* ---------------------------------------------------------------- sample-rate conversion
 * Replaces `torchaudio.functional.resample(wave, orig, new)` (inference.py:380-406) for any filter of that polyphase form.  With
 * g = gcd(orig, new), o = orig / g, n = new / g the operator is out[i n + j] = sum_k K[j][k] xpad[i o + k], xpad = x padded by
 * `width` zeros on the left; the library takes the non-zero run of every phase: taps HOST [n][ntaps] fp32 and first HOST [n]
 * int32, the column of K where phase j's run starts (runs shorter than ntaps are padded with 0.0 at the end).  The host mirror
 * builds both from torchaudio's float64 formula (audio.py: sinc_resample_taps).  Both arrays are copied before create returns.
 * o so large that four periods of input do not fit the LDS (about 3900 with these filters) is refused. */
typedef struct svc_resampler svc_resampler_t;
int svc_resampler_create(int o, int n, int width, int ntaps, const int32_t* first, const float* taps, void* stream,
                         svc_resampler_t** out);
void svc_resampler_destroy(svc_resampler_t* r);
long svc_resample_len(int o, int n, long L);           /* ceil(n L / o) in 64-bit integers; needs no handle and no GPU */
long svc_resampler_tile(const svc_resampler_t* r);     /* outputs one workgroup owns (a multiple of n); for tests and tools */
/* x [B][L] -> out [B][Lout], 1 <= B <= 64, Lout >= svc_resample_len(o, n, max lens).  lens HOST int32 [B] (1 <= lens[b] <= L) or
 * NULL (every clip has L samples); they travel as kernel arguments: consumed before the call returns, nothing is copied or
 * synchronised.  For m < svc_resample_len(o, n, lens[b]), with j = m mod n and i = m div n,
 *     out[b][m] = sum_{k = 0}^{ntaps - 1} taps[j][k] * xx[i o + first[j] + k - width],
 * accumulated in ascending k as one fp32 FMA chain, where xx is x[b] inside [0, lens[b]) and 0.0 outside: samples outside go
 * through the same chain as zeros, so an output's bits depend on its clip's samples alone, not on its place in a tile, the
 * batch or the other clips.  Every out[b][m] at and above that count is written as 0.0.  Samples at and above lens[b] are never
 * read as values (NaN is fine there).  lens[b] == L for all b equals lens == NULL bit for bit.  All sample positions are 64-bit.
 * A length outside [1, L], B outside [1, 64], Lout too small, a null pointer, x and out overlapping: non-zero, a
 * svc_last_error() that names the argument, nothing enqueued. */
int svc_resample(svc_resampler_t* r, const float* x, const int32_t* lens, int B, long L, float* out, long Lout, void* stream);

/* ---------------------------------------------------------------- CAMPPlus style encoder + Kaldi fbank (second half) */
typedef struct svc_campplus_config {  /* modules/campplus/DTDNN.py:54-62 (CAMPPlus.__init__ defaults; the drivers use embedding_size 192) */
    int feat_dim, embedding_size, growth_rate, bn_size, init_channels, m_channels;
    int n_blocks, block_layers[4], block_kernel[4], block_dilation[4];
    int seg_len;                      /* CAMLayer.seg_pooling segment length (layers.py:119) */
} svc_campplus_config_t;
typedef struct svc_campplus svc_campplus_t;
/* Packs `CAMPPlus.state_dict()` (eval mode: BatchNorm running statistics are folded). */
int svc_campplus_create(const svc_campplus_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream,
                        svc_campplus_t** out);
void svc_campplus_destroy(svc_campplus_t* m);
/* Replaces `campplus_model(feat)` = CAMPPlus.forward(x) (modules/campplus/DTDNN.py:132-137; inference.py:430,
 * seed_vc_wrapper.py): feat [B][T][feat_dim] (mean-normalised fbank) -> out [B][embedding_size].  All clips of a batch
 * have T frames (the drivers call it with B = 1 and no x_lens). */
int svc_campplus_forward(svc_campplus_t* m, const float* feat, int B, int T, float* out, void* stream);
/* Replaces `torchaudio.compliance.kaldi.fbank(wave, num_mel_bins=feat_dim, dither=0, sample_frequency=16000)`
 * (inference.py:418-428): wave [n_samples] fp32 -> out [frames][feat_dim], frames = svc_kaldi_fbank_frames(n_samples). */
int svc_kaldi_fbank_frames(int n_samples);
int svc_kaldi_fbank(svc_campplus_t* m, const float* wave, int n_samples, float* out, void* stream);
/* Both for a batch of reference clips of different lengths, in one call each (the contract of the ragged vocoder calls): lens is
 * HOST int32 [B], consumed before the call returns (pinned staging inside the handle: no host synchronisation in steady state);
 * values at and above a clip's end are never read as values (they may hold NaN); lens == NULL, a length out of range or B < 1:
 * non-zero, a svc_last_error() that names lens, nothing enqueued, and the checks come before the handle is touched.
 *
 * svc_kaldi_fbank_ragged: wave [B][L] at 16 kHz, 400 <= lens[b] <= L samples; out [B][svc_kaldi_fbank_frames(L)][feat_dim].
 * Clip b gets its own n_b = svc_kaldi_fbank_frames(lens[b]) frames, each what svc_kaldi_fbank gives for the clip alone; rows at
 * and above n_b are written as zero.  subtract_mean != 0: the mean over the clip's own n_b frames is subtracted from them (the
 * drivers' `feat - feat.mean(dim=0, keepdim=True)`, inference.py:429, in a kernel).
 *
 * svc_campplus_forward_ragged: feat [B][T][feat_dim], 8 <= lens[b] <= T frames (the lower bound is svc_campplus_forward's);
 * out [B][embedding_size], out[b] = the embedding of feat[b][:lens[b]] run alone, whatever the other clips and their order:
 * the FCM convs see zero time steps above the clip's end, the TDNN and the dilated CAM convs zero-pad at its own last row
 * (T2_b = (lens[b] - 1) / 2 + 1 rows after the TDNN), the CAM context uses its own ceil(T2_b / seg_len) segments and its own
 * global mean, and the statistics pool over T2_b rows (unbiased, T2_b - 1).  lens[b] == T for all b gives
 * svc_campplus_forward's result bit for bit.
 * Workspace grows with B * Tmax: the three FCM planes are B * (T + 2) * feat_dim * 32 * 4 bytes each (1.6 GB each for 64 clips
 * of 25 s), the dense-block buffers B * T / 2 rows; a padded row costs what a live one does. */
int svc_kaldi_fbank_ragged(svc_campplus_t* m, const float* wave, const int32_t* lens, int B, int L, int subtract_mean, float* out,
                           void* stream);
int svc_campplus_forward_ragged(svc_campplus_t* m, const float* feat, const int32_t* lens, int B, int T, float* out, void* stream);

/* ---------------------------------------------------------------- RMVPE pitch extractor
 * Replaces `rmvpe.infer_from_audio(wave_16k, thred=0.03)` of the drivers' f0-conditioned path and their pitch step (voiced-median
 * shift + semitone shift).  Architecture of RVC's rmvpe.py, restated (the file is not on the build machine; parity with a real
 * rmvpe.pt is unpinned): log-mel (16 kHz, n_fft = win = 1024, hop 160, Hann, center=True with reflect padding, sqrt(re^2 + im^2),
 * caller's mel basis, log(max(., 1e-5))), the mel read as a one-channel (time, bin) image zero-padded in time to a multiple of
 * 32 frames, BatchNorm, en_de_layers encoder levels of n_blocks ConvBlockRes + AvgPool(2, 2), inter_layers x n_blocks
 * ConvBlockRes, decoder (stride-2 ConvTranspose2d + BatchNorm + ReLU, concatenation with the skip, n_blocks ConvBlockRes),
 * Conv2d(., 3), bidirectional GRU(3 n_mels, gru_hidden), Linear(2 gru_hidden, n_bins) + sigmoid.  fp32 throughout.
 * The state-dict keys are those of that module tree (unet.encoder.bn.*, unet.encoder.layers.L.conv.J.conv.{0,1,3,4}.*,
 * ....shortcut.{weight,bias}, unet.intermediate.layers.*, unet.decoder.layers.D.conv1.{0,1}.* / .conv2.J.*, cnn.*,
 * fc.0.gru.{weight,bias}_{ih,hh}_l0[_reverse], fc.1.*); num_batches_tracked is ignored.
 *
 * Ragged batches, as in the calls above: every lens / frame_lens array is HOST int32 [B], consumed before the call returns (kernel
 * arguments: nothing is copied or synchronised), B <= 64; clip b is computed as if it ran alone, whatever the other clips, their
 * order and the internal grouping are (bit for bit), and nothing at or above its end is read as a value (NaN is fine there).  The
 * host checks come first, name the offending argument and touch no handle.  A call synchronises only to grow its workspace. */
typedef struct svc_rmvpe_config {
    int n_mels;            /* 128; a multiple of 8 and of 2^en_de_layers */
    int en_de_layers;      /* 1 .. 5 (5); the time padding multiple is 32 whatever the depth */
    int inter_layers;      /* >= 1 (4) */
    int n_blocks;          /* >= 1 (4) */
    int en_out_channels;   /* 16, or a multiple of 32 */
    int gru_hidden;        /* 64 | 128 | 192 | 256 (256) */
    int n_bins;            /* 360 */
} svc_rmvpe_config_t;
typedef struct svc_rmvpe svc_rmvpe_t;
/* mel_basis: device fp32 [n_mels][513] (librosa.filters.mel(16000, 1024, n_mels, 30, 8000, htk=True) in the reference). */
int svc_rmvpe_create(const svc_rmvpe_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, const float* mel_basis, void* stream,
                     svc_rmvpe_t** out);
void svc_rmvpe_destroy(svc_rmvpe_t* m);
int svc_rmvpe_frames(int n_samples);                   /* frames of a clip: 1 + n_samples / 160 */
int svc_rmvpe_min_len(void);                           /* the shortest legal clip: n_fft / 2 + 1 = 513 samples (reflect padding) */
/* Workspace grows with B * Tpad: about 11 times one level-0 plane of B * (Tpad + 2) * n_mels * 32 * 4 bytes.  A call whose level-0
 * plane would exceed the budget (default 256 MiB; 0 restores it) runs its clips in consecutive groups that fit (at least one clip
 * per group); no row's bits depend on the grouping. */
int svc_rmvpe_set_plane_budget(svc_rmvpe_t* m, long long bytes);
/* Measurement aid (tools/rmvpe_bench.py): with timing on, every network pass records HIP events on its stream around its stages;
 * svc_rmvpe_last_timing waits for the last pass (the last group of the last call) and fills ms4 = {U-Net, GRU input projection,
 * GRU recurrence, output layer} in milliseconds. */
int svc_rmvpe_set_timing(svc_rmvpe_t* m, int on);
int svc_rmvpe_last_timing(svc_rmvpe_t* m, float* ms4);
/* wave [B][L] at 16 kHz, svc_rmvpe_min_len() <= lens[b] <= L -> mel_out [B][n_mels][svc_rmvpe_frames(L)]; the frames at and above
 * svc_rmvpe_frames(lens[b]) are 0. */
int svc_rmvpe_mel(svc_rmvpe_t* m, const float* wave, const int32_t* lens, int B, int L, float* mel_out, void* stream);
/* The network alone: mel [B][n_mels][T], 1 <= frame_lens[b] <= T -> out [B][T][n_bins] (salience in (0, 1)); rows at and above
 * frame_lens[b] are 0. */
int svc_rmvpe_salience(svc_rmvpe_t* m, const float* mel, const int32_t* frame_lens, int B, int T, float* out, void* stream);
/* salience [B][T][360] -> f0_out [B][T] in Hz (needs no handle).  Per frame: arg-max bin (the first maximum on ties), the
 * salience-weighted mean of cents[k] = 20 k + 1997.3794084376191 over the 9 bins around it (bins outside 0 .. 359 contribute zero),
 * f0 = 10 * 2^(cents / 1200); a frame whose maximum is <= thred, and every frame at and above frame_lens[b], is exactly 0. */
int svc_rmvpe_decode(const float* salience, const int32_t* frame_lens, int B, int T, float thred, float* f0_out, void* stream);
/* The one call: wave [B][L] -> f0_out [B][svc_rmvpe_frames(L)].  lens may be NULL (every clip has L samples). */
int svc_rmvpe_f0(svc_rmvpe_t* m, const float* wave, const int32_t* lens, int B, int L, float thred, float* f0_out, void* stream);
/* The drivers' pitch step in one launch (inference.py, `if f0_condition:` block): f0_alt [B][Talt] (source), f0_ori [B][Tori]
 * (reference), alt_lens / ori_lens HOST int32 [B] frames (0 .. Talt / Tori), semitones HOST float [B] or NULL (= 0), out [B][Talt].
 * voiced = f0 > 1; m_x = torch's median (the lower middle element) of log(f0_x + 1e-5) over the voiced frames of row b, found by a
 * 4-pass radix select on the bit pattern;
 *   out = exp(log(f0_alt + 1e-5) - m_alt + m_ori) * 2^(semitones[b] / 12)     voiced frames, auto_adjust != 0
 *   out = f0_alt' * 2^(semitones[b] / 12), f0_alt' = exp(log(f0_alt + 1e-5))   voiced frames, auto_adjust == 0
 *   out = exp(log(f0_alt + 1e-5))  (1e-5 for an exact 0, not 0, as in the reference)   unvoiced frames;  0 at and above alt_lens[b].
 * A row without a voiced frame on either side gets no median shift (the reference raises on the empty median).
 * medians: optional device [B][2] = (m_alt, m_ori) of each row (0 where there is no voiced frame); NULL = not wanted. */
int svc_f0_adjust(const float* f0_alt, const int32_t* alt_lens, const float* f0_ori, const int32_t* ori_lens, int B, int Talt, int Tori,
                  int auto_adjust, const float* semitones, float* out, float* medians, void* stream);

/* ---------------------------------------------------------------- Whisper content encoder (csrc/whisper.hip)
 * Replaces `semantic_fn(waves_16k)` of the drivers (WhisperFeatureExtractor + the encoder half of openai/whisper-small, one 30 s
 * window at a time) and their loop over the windows of a long clip.  P = max_source_positions rows per window, W = 320 P samples.
 * Log-mel: the window zero-padded to W, n_fft = win = 400, hop 160, periodic Hann, center=True with the reflect padding applied to
 * the PADDED window, re^2 + im^2, the last of the 2 P + 1 frames dropped, mel_basis [n_mels][201] (device, copied),
 * log10(max(., 1e-10)), max(x, m - 8) with m the maximum over the whole window, (x + 4) / 4.  Encoder: conv1 (k 3, pad 1) + GELU,
 * conv2 (k 3, stride 2, pad 1) + GELU, + embed_positions.weight, n_layers pre-LN blocks (LayerNorm eps 1e-5; q (bias) / 8, k (no
 * bias), v (bias); unmasked softmax attention over all P keys, heads of 64; out_proj + residual; LayerNorm; fc1 + erf-GELU; fc2 +
 * residual), final layer_norm.  Residual stream, LayerNorm statistics and softmax are fp32; attention operands are fp16.
 * precision 1: convs and linears with fp16 operands and fp32 accumulation; 0: on the fp32 tap-GEMM.
 * weights: WhisperEncoder.state_dict() (device fp32); the prefixes "encoder." and "model.encoder." are accepted, other keys are
 * ignored; a missing or mis-shaped key is named in the error.  d_model a multiple of 64 with n_heads * 64 == d_model, n_mels a
 * multiple of 8, ffn_dim a multiple of 64.  Lengths are HOST int32 arrays consumed before the call returns; arguments are checked
 * before the handle is touched; nothing synchronises in steady state (the workspace grows on the first call of a size).  Samples at
 * and above a clip's length are never read as values.  A window's rows are bit-identical whatever else shares the call, in any
 * order and with any group size. */
typedef struct svc_whisper_config {
    int n_mels, d_model, n_heads, n_layers, ffn_dim, max_source_positions, precision;
} svc_whisper_config_t;
typedef struct svc_whisper svc_whisper_t;

int svc_whisper_create(const svc_whisper_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, const float* mel_basis, void* stream,
                       svc_whisper_t** out);
void svc_whisper_destroy(svc_whisper_t* m);
/* The drivers' window plan of a clip of n_samples >= 1 samples, 0 <= overlap_rows < P (no handle; -1 on a bad argument): window j
 * starts at j (W - O), O = 320 overlap_rows, and has min(W, n_samples - start) samples; window 0 always exists, window j >= 1 exists
 * iff W + (j - 1)(W - O) < n_samples.  A window of n samples yields rows [0, min(P, n / 320 + 1)); every window but the first drops
 * its first overlap_rows.  svc_whisper_rows = the kept rows of the clip. */
int svc_whisper_n_windows(int P, int overlap_rows, long n_samples);
int svc_whisper_rows(int P, int overlap_rows, long n_samples);
/* Windows computed side by side (1 .. 64, 0 = the default of 16): bounds the workspace; results do not depend on it. */
int svc_whisper_set_window_group(svc_whisper_t* m, int windows);
/* Measurement aid (tools/whisper_bench.py): with timing on, svc_whisper_content records HIP events around its stages;
 * svc_whisper_last_timing waits for the last group of the last call and fills ms4 = {log-mel, stem, layers, assemble} in ms. */
int svc_whisper_set_timing(svc_whisper_t* m, int on);
int svc_whisper_last_timing(svc_whisper_t* m, float* ms4);
/* wave [B][L] at 16 kHz, 1 <= lens[b] <= min(L, W), B <= 64 -> feat [B][n_mels][2 P] (one window per clip). */
int svc_whisper_mel(svc_whisper_t* m, const float* wave, const int32_t* lens, int B, int L, float* feat, void* stream);
/* feat [B][n_mels][2 P] -> out [B][P][d_model]. */
int svc_whisper_encode(svc_whisper_t* m, const float* feat, int B, float* out, void* stream);
/* The one call: wave [B][L], lens HOST [B] in 1 .. L or NULL (= L), B <= 64 clips of any length -> out [B][Rmax][d_model]: rows
 * [0, svc_whisper_rows(P, overlap_rows, lens[b])) of out[b] are the kept rows of the clip's windows in order, the rows above are
 * zero.  Rmax >= the largest row count.  All windows of all clips run through the log-mel and the encoder together, in groups. */
int svc_whisper_content(svc_whisper_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, float* out, int Rmax,
                        void* stream);

/* ---------------------------------------------------------------- wav2vec 2.0 content encoder (csrc/wav2vec2.hip)
 * Replaces `semantic_fn(waves_16k)` of the drivers for the xlsr models (Wav2Vec2FeatureExtractor + the first n_layers layers of
 * facebook/wav2vec2-xls-r-300m, one 30 s window at a time) and their loop over the windows of a long clip.  HuBERT-large is the same
 * network.  Accepted: feat_extract_norm = "layer" with do_stable_layer_norm and conv_bias, one conv_dim (a multiple of 64, at most
 * 512) for all n_conv <= 8 extractor convs whose strides multiply to 320 samples per row (the window plan counts rows of 320
 * samples) and conv_kernel[0] * conv_dim <= 8192, heads of 64, erf-GELU, an even num_conv_pos_embeddings (pos_k <= 128) in groups of 64
 * channels; anything else is refused by svc_w2v_create.  n_layers layers run, then encoder.layer_norm.
 * frames(n): (n - conv_kernel[l]) / conv_stride[l] + 1 applied for every conv (0 once n < conv_kernel[l]).
 * Stages: normalisation (x - mean) / sqrt(var + 1e-7) over the clip's (in the one call: the window's) own samples, population
 * variance about the mean, fixed reduction order; the extractor (conv, LayerNorm over channels, GELU; then the feature projection's
 * LayerNorm and Linear conv_dim -> d_model); the positional conv (grouped Conv1d, padding pos_k / 2, last output dropped, GELU,
 * added to its input); n_layers pre-LN blocks (LayerNorm eps 1e-5; q / 8, k, v with biases; unmasked softmax attention over the
 * clip's own rows; out_proj + residual; LayerNorm; intermediate_dense + GELU; output_dense + residual); encoder.layer_norm.
 * Residual stream, LayerNorm statistics and softmax are fp32.  precision 1: fp16 operands with fp32 accumulation (the positional
 * conv on its own MFMA kernel); 0: the fp32 tap-GEMM everywhere (attention operands stay fp16).
 * weights: Wav2Vec2Model.state_dict() or HubertModel.state_dict() (device fp32); the prefixes "wav2vec2.", "hubert." and "model." are
 * accepted, unknown keys (masked_spec_embed, ...) are ignored; the positional conv's weight norm (parametrizations.weight.original0 /
 * original1, or weight_g / weight_v, or a plain weight) is folded at pack time.  Lengths and row counts are HOST int32 arrays consumed
 * before the call returns; arguments are checked before the handle is touched; nothing synchronises once the workspace has its size.
 * Samples / rows at and above a clip's length are never read as values.  Every clip (window) gets what it would get alone: its bits
 * do not depend on what shares the call, on the order or on the group size.
 *
 * The base family (facebook/wav2vec2-base, facebook/hubert-base-ls960 and their fine-tunes) enters through
 * svc_w2v_create_ex with a non-NULL `ext`: feat_extract_norm = "group" (feat_extract_norm_layer = 0) together with
 * do_stable_layer_norm = 0; the two flags must agree (the mixed forms exist in no released model and are refused by name), conv_bias
 * may be 0 or 1 in either family, and the positional conv's groups may be 16, 32, 48 or 64 channels wide (d_model / pos_groups).
 * Group-norm extractor: conv0, then GroupNorm(conv_dim groups of one channel, eps 1e-5, affine) = a per-channel normalisation over
 * the window's own conv0 frames, then GELU; convs 1 .. n - 1 are conv, GELU without a norm; then the feature projection as above.
 * The channel statistics are derived from the window's own samples (the means of the conv_kernel[0] tap positions and their
 * centred covariance, 64 block partials each, folded in index order in double), so they depend on nothing but the window.  In this
 * family conv_kernel[0] <= 16.  Post-LN encoder: encoder.layer_norm on h + gelu(pos_conv(h)) BEFORE the layers, each layer
 * x = layer_norm(x + attention(x)), x = final_layer_norm(x + feed_forward(x)), no norm after the last layer.
 * ext->do_normalize = 0 feeds the samples as they are (svc_w2v_normalize then copies, svc_w2v_content skips the normalisation).
 * Every other call serves both families unchanged. */
typedef struct svc_w2v_config {
    int conv_dim, n_conv, conv_kernel[8], conv_stride[8];
    int d_model, n_heads, n_layers, ffn_dim, pos_k, pos_groups;
    int feat_extract_norm_layer, do_stable_layer_norm, conv_bias;   /* svc_w2v_create: must all be 1; svc_w2v_create_ex: see above */
    int window_samples;     /* the drivers' window: 480000 (a multiple of 320) */
    int precision;
} svc_w2v_config_t;
typedef struct svc_w2v_ext {
    int do_normalize;          /* 1: per-window zero-mean / unit-variance (svc_w2v_create's behaviour); 0: samples as they are */
    int feat_proj_layer_norm;  /* must be 1 (HubertConfig.feat_proj_layer_norm; wav2vec2 always has it) */
} svc_w2v_ext_t;
typedef struct svc_w2v svc_w2v_t;

int svc_w2v_create(const svc_w2v_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream, svc_w2v_t** out);
/* svc_w2v_create is this call with ext == NULL (the strict checks above).  With ext the base family is accepted as well. */
int svc_w2v_create_ex(const svc_w2v_config_t* cfg, const svc_w2v_ext_t* ext, const svc_tensor_desc_t* weights, int n_weights,
                      void* stream, svc_w2v_t** out);
void svc_w2v_destroy(svc_w2v_t* m);
/* Host-side counts (no handle; -1 on a bad argument).  svc_w2v_frames: rows of n_samples in one piece.  The window plan is the
 * drivers' (svc_whisper_n_windows, with W = window_samples and O = 320 overlap_rows); a window of n samples yields frames(n) rows,
 * every window but the first drops its first overlap_rows, a later window with frames(n) <= overlap_rows contributes nothing.
 * A clip whose first window is shorter than the extractor's receptive field is an error. */
long svc_w2v_frames(const svc_w2v_config_t* cfg, long n_samples);
int svc_w2v_n_windows(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples);
int svc_w2v_rows(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples);
/* Windows computed side by side (1 .. 64, 0 = the default of 16): bounds the workspace; results do not depend on it. */
int svc_w2v_set_window_group(svc_w2v_t* m, int windows);
/* Measurement aid (tools/w2v_bench.py): ms4 = {normalisation + extractor, positional conv, layers, assemble} of the last group of the
 * last svc_w2v_content call, in ms. */
int svc_w2v_set_timing(svc_w2v_t* m, int on);
int svc_w2v_last_timing(svc_w2v_t* m, float* ms4);
/* wave [B][L], 1 <= lens[b] <= L, B <= 64 -> out [B][L]: samples below lens[b] normalised, the others not touched. */
int svc_w2v_normalize(svc_w2v_t* m, const float* wave, const int32_t* lens, int B, int L, float* out, void* stream);
/* normalised wave [B][L] -> out [B][Tmax][d_model]: the frames(lens[b]) projected rows of each clip; the rows above are not touched. */
int svc_w2v_features(svc_w2v_t* m, const float* wave_norm, const int32_t* lens, int B, int L, float* out, int Tmax, void* stream);
/* h [B][T][d_model], 1 <= rows[b] <= T -> out = h + gelu(pos_conv(h)) on rows below rows[b]; the rows above are not touched. */
int svc_w2v_posconv(svc_w2v_t* m, const float* h, const int32_t* rows, int B, int T, float* out, void* stream);
/* h (projected rows) -> out [B][T][d_model]: positional conv, n_layers layers, encoder.layer_norm; rows at and above rows[b] are not touched. */
int svc_w2v_encode(svc_w2v_t* m, const float* h, const int32_t* rows, int B, int T, float* out, void* stream);
/* The one call: wave [B][L], lens HOST [B] or NULL (= L), B <= 64 clips of any length -> out [B][Rmax][d_model]: rows
 * [0, svc_w2v_rows(cfg, overlap_rows, lens[b])) of out[b] are the kept rows of the clip's windows in order, the rows above are zero.
 * Each window is normalised on its own (the drivers call the feature extractor per window). */
int svc_w2v_content(svc_w2v_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, float* out, int Rmax, void* stream);

/* ---------------------------------------------------------------- ASTRAL tokenizer (csrc/astral.hip)
 * Replaces the v2 model's content tokenizers (`AstralQuantizer`: HubertModel of facebook/hubert-large-ll60k cut to ssl.n_layers
 * layers with encoder.layer_norm replaced by Identity, then ConvNeXtV2Stage and BinarySphericalQuantize) and the drivers' loop over
 * the windows of a long clip.  One SSL pass feeds n_heads heads (v2: wide, 2048 codes, and narrow, 32 codes).
 * SSL front: the wav2vec 2.0 encoder above under `ssl` (its n_layers is the SSL output layer, its precision is shared by the heads),
 * without the final LayerNorm.  A window of n samples yields min(frames(n), n / 320) rows.
 * Head on rows h [T][ssl.d_model]: x = input_projection(h) (d_model -> dim); n_blocks times x += pwconv2(GRN(gelu(pwconv1(
 * LayerNorm(dwconv(x)))))) with a depthwise conv of 7 taps whose zero padding sits at the window's own first and last row, LayerNorm
 * over channels (eps 1e-6), erf-GELU, GRN: Gx[c] = sqrt(sum over the window's own rows of y[t][c]^2), Nx = Gx / (mean_c Gx + 1e-6),
 * y = gamma (y Nx) + beta + y; then z = project_in(x) (dim -> bits) and index = sum_j [z_j > 0] 2^(bits - 1 - j).
 * Residual stream, statistics and logits are fp32; the linears follow ssl.precision as in the w2v section; project_in is always fp32.
 * weights: ssl_weights as svc_w2v_create takes them (encoder.layer_norm.* and layers at and above n_layers are ignored); per head
 * encoder.input_projection.{weight (dim, d_model[, 1]), bias}, encoder.blocks.{i}.dwconv.{weight (dim, 1, 7), bias}, .norm.{weight,
 * bias}, .pwconv1.{weight, bias}, .grn.{gamma, beta} ((1, 1, F) or (F,)), .pwconv2.{weight, bias}, quantizer.project_in.{weight,
 * bias}; other keys are ignored.  Lengths and row counts are HOST int32 arrays consumed before the call returns; arguments are
 * checked before the handle is touched where they can be; nothing synchronises once the workspace has its size.  Every window gets
 * what it would get alone: its bits do not depend on what shares the call, on the order or on the group size. */
#define SVC_ASTRAL_MAX_HEADS 2
typedef struct svc_astral_head_config {
    int dim, intermediate_dim;              /* multiples of 64, at most 2048 */
    int n_blocks;                           /* 1 .. 64 */
    int bits;                               /* 1 .. 16: log2(codebook_size) */
    int dw_kernel;                          /* must be 7 */
} svc_astral_head_config_t;
typedef struct svc_astral_config {
    svc_w2v_config_t ssl;
    int n_heads;                            /* 1 or 2 */
    svc_astral_head_config_t head[SVC_ASTRAL_MAX_HEADS];
} svc_astral_config_t;
typedef struct svc_astral svc_astral_t;

/* head_weights[k] / n_head_weights[k]: the state dict of head k.  Configurations the kernels do not cover are refused with a message. */
int svc_astral_create(const svc_astral_config_t* cfg, const svc_tensor_desc_t* ssl_weights, int n_ssl_weights,
                      const svc_tensor_desc_t* const* head_weights, const int* n_head_weights, void* stream, svc_astral_t** out);
void svc_astral_destroy(svc_astral_t* m);
/* Host-side counts (no handle; -1 on a bad argument): the drivers' window plan as svc_w2v_n_windows / svc_w2v_rows, with
 * min(frames(n), n / 320) rows per window. */
int svc_astral_n_windows(const svc_astral_config_t* cfg, int overlap_rows, long n_samples);
int svc_astral_rows(const svc_astral_config_t* cfg, int overlap_rows, long n_samples);
int svc_astral_set_window_group(svc_astral_t* m, int windows);
/* Measurement aid (tools/astral_bench.py): ms4 = {SSL front, ConvNeXt stages, BSQ heads, assemble} of the last group of the last
 * svc_astral_tokens / svc_astral_tokens_heads call, in ms. */
int svc_astral_set_timing(svc_astral_t* m, int on);
int svc_astral_last_timing(svc_astral_t* m, float* ms4);
/* Seam: wave [B][L], 1 <= lens[b] <= min(L, window_samples), one window per clip -> out [B][T][ssl.d_model]: the residual stream
 * after layer n_layers (no final LayerNorm) on each clip's rows; the rows above are not touched. */
int svc_astral_ssl(svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, float* out, int T, void* stream);
/* Seam: head `head`, h [B][T][ssl.d_model], 1 <= rows[b] <= T -> x [B][T][dim] after the last block; rows at and above rows[b] are
 * neither read as values nor written. */
int svc_astral_convnext(svc_astral_t* m, int head, const float* h, const int32_t* rows, int B, int T, float* x, void* stream);
/* Seam: head `head`, x [B][T][dim] -> z [B][T][bits] = project_in(x), fp32; rows at and above rows[b] are not touched. */
int svc_astral_logits(svc_astral_t* m, int head, const float* x, const int32_t* rows, int B, int T, float* z, void* stream);
/* z [rows][bits] -> index[rows] = sum_j [z_j > 0] 2^(bits - 1 - j) (strict: +0, -0 and NaN give bit 0). */
int svc_op_bsq_index(const float* z, int32_t* index, long rows, int bits, void* stream);
/* Duration reduction (torch.unique_consecutive per clip): tokens [B][R], 0 <= rows[b] <= R (HOST) -> out [B][R]: the first token
 * of every run in order, -1 above the count; counts [B] on the DEVICE.  tokens and out must not overlap. */
int svc_tokens_reduce(const int32_t* tokens, const int32_t* rows, int B, int R, int32_t* out, int32_t* counts, void* stream);
/* The one call: wave [B][L], lens HOST [B] or NULL (= L), B <= 64 clips of any length -> tokens [n_heads][B][Rmax]: tokens
 * [0, svc_astral_rows(cfg, overlap_rows, lens[b])) of tokens[k][b] are head k's indices of the kept rows of the clip's windows in
 * order, -1 above.  reduce_head >= 0: also reduced [B][Rmax] and counts [B] (device), svc_tokens_reduce of that head's tokens. */
int svc_astral_tokens(svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, int32_t* tokens, int Rmax,
                      int reduce_head, int32_t* reduced, int32_t* counts, void* stream);
/* svc_astral_tokens for a subset of the heads: bit k of head_mask means "head k runs"; the mask is non-zero and inside
 * (1 << n_heads) - 1.  tokens [popcount(head_mask)][B][Rmax]: the selected heads' planes in ascending head order.  reduce_head
 * stays a head index: -1 or a selected head.  svc_astral_tokens is this call with every bit set (one code path).  Contract:
 *   - a selected head's plane is bit for bit the plane svc_astral_tokens writes for that head;
 *   - an unselected head launches nothing (no ConvNeXt group, no BSQ, no assemble plane), and memory past the popcount planes
 *     is neither read nor written (the overlap check of `reduced` uses the compacted size);
 *   - every refusal -- those of svc_astral_tokens, a mask that is zero or out of range, a reduce_head that is not selected, null
 *     pointers -- happens before any launch and is reported through svc_last_error().
 * svc_astral_last_timing keeps its four stages; stages 2 and 3 cover the selected heads. */
int svc_astral_tokens_heads(svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, unsigned head_mask,
                            int32_t* tokens, int Rmax, int reduce_head, int32_t* reduced, int32_t* counts, void* stream);

/* Device-side counterpart of `crossfade(chunk1, chunk2, overlap)` (inference.py:343-350): the first n samples of
 * chunk2 become chunk2 * fade_in + chunk1_tail * fade_out in float64, stored as float32 (bit-identical to the numpy
 * arithmetic).  fade_in / fade_out: the caller's cos^2 windows (double, device). */
int svc_crossfade(float* chunk2, const float* chunk1_tail, const double* fade_in, const double* fade_out, int n,
                  void* stream);

/* ---------------------------------------------------------------- long-form conversion as a pool of chunks
 * The drivers' chunk loop (inference.py:470-527, seed_vc_wrapper.py:561-623) with the chunks of one or more utterances run
 * side by side: a chunk reads the source, the shared prompt and fresh noise, never its neighbour; only the cross-fade
 * couples neighbours, and it reads finished waveforms.  Conventions of the ragged assembly calls above: every per-chunk /
 * per-utterance array is HOST int32 and consumed before the call returns (kernel arguments, one launch per 64 chunks),
 * arguments are checked before anything is launched, every output element is written, nothing synchronises.
 *
 * Replaces `cat_condition = torch.cat([prompt_condition, cond[:, p0:p0 + s]], dim=1)` for N chunks of U utterances:
 * prompt_cond [U][Pmax][Dc], prompt_lens [U], cond [R][Dc] (the utterances' condition rows concatenated along time),
 * chunk k belongs to utterance utt[k] and takes rows row0[k] .. row0[k] + rows[k] - 1 of cond.  mu [N][T][Dc]:
 *   mu[k][t] = t < P_u ? prompt_cond[u][t] : t < P_u + rows[k] ? cond[row0[k] + t - P_u] : 0        (u = utt[k])
 * 0 <= utt[k] < U, 0 <= prompt_lens[u] <= Pmax, rows[k] >= 0, row0[k] >= 0, row0[k] + rows[k] <= R,
 * prompt_lens[u] + rows[k] <= T, Dc >= 1. */
int svc_chunks_gather_cond(const float* prompt_cond, const int32_t* prompt_lens, int U, int Pmax, const float* cond, int R,
                           const int32_t* utt, const int32_t* row0, const int32_t* rows, int N, int Dc, int T, float* mu,
                           void* stream);
/* Replaces `_stream_wave_chunks` + `crossfade` + the final concatenation (seed_vc_wrapper.py:201-285, inference.py:343-350,
 * :507-527) for N chunk waveforms: wave[k * stride + i], i < lens[k] (samples at and above lens[k] are never read);
 * first[k] / last[k] != 0 flag the first / last chunk of an utterance (an utterance's chunks are consecutive and in order);
 * fade_in / fade_out [ov]: the caller's cos^2 windows (double, device), as svc_crossfade takes them.  With
 * body[k] = lens[k] - (last[k] ? 0 : ov) and off[k] the sum of the bodies before k, for i < body[k]:
 *   out[off[k] + i] = wave[k][i]                                                               first[k] or i >= ov
 *                   = float(double(wave[k][i]) * fade_in[i] + double(wave[k-1][lens[k-1] - ov + i]) * fade_out[i])   otherwise
 * with the products and the sum rounded separately (svc_crossfade's arithmetic, bit-identical to numpy's); a last chunk
 * shorter than ov is the `len(chunk2) < overlap` branch of `crossfade`.  Each output sample is written exactly once, the
 * utterances follow each other in `out`.  0 <= lens[k] <= stride; lens[k] >= ov unless last[k]; first[0] and last[N-1]
 * set, first[k] set exactly when last[k-1] is; out_len == sum(body); ov >= 0. */
int svc_chunks_assemble(const float* wave, long long stride, const int32_t* lens, const int32_t* first, const int32_t* last, int N,
                        const double* fade_in, const double* fade_out, int ov, float* out, long long out_len, void* stream);
/* svc_chunks_assemble for an arbitrary list of N pieces of the same chunk-wave buffer (n_rows rows of `stride` floats), so
 * that a file's audio can be spliced while later chunks do not exist yet: rows in any order, any subset of them, a chunk
 * delivered in one piece or several.  Piece p, HOST arrays consumed before the call returns (one launch per 64 pieces):
 *   row[p]       the row holding the chunk, len[p] its samples;
 *   prev_row[p]  the row of the chunk before it in its file, or -1 (no seam); prev_len[p] that row's samples;
 *   begin[p] <= end[p] <= len[p]   the samples of the chunk this piece delivers;
 *   out_off[p]   (int64) where sample begin[p] lands in `out`.
 * For begin[p] <= i < end[p]:
 *   out[out_off + i - begin] = wave[row][i]                                                          prev_row < 0 or i >= ov
 *                            = float(double(wave[row][i]) * fade_in[i] + double(wave[prev_row][prev_len - ov + i]) * fade_out[i])
 * with the products and the sum rounded separately: the device function svc_chunks_assemble's kernel calls, so a file
 * emitted piece by piece is bit for bit the file assembled at once.  No sample at or above len / prev_len is read; nothing
 * outside the pieces' ranges is written (`out` is NOT otherwise initialised).  Every piece of a chunk carries
 * the chunk's prev_row: samples below ov are seam samples whichever piece delivers them, and a tail held back for a
 * successor that never came (begin = len - ov, end = len) is one more piece of its chunk.
 * pcm (int16, may be NULL): a second plane written at the same offsets, the reference streaming leg's
 * `(wave * 32768.0).astype(np.int16)`: the float scaled exactly, truncated toward zero, SATURATED to [-32768, 32767].
 * Saturation is the one deliberate deviation: numpy wraps +1.0 (where the vocoders' clamp can land) to -32768.  NaN gives 0.
 * Refused before anything is launched: row / prev_row outside the buffer, len or prev_len outside 0 .. stride, a range
 * outside its chunk, prev_row >= 0 with prev_len < ov, pieces that overlap in `out`, a piece outside 0 .. out_len. */
int svc_chunks_emit(const float* wave, long long stride, int n_rows, const int32_t* row, const int32_t* len, const int32_t* prev_row,
                    const int32_t* prev_len, const int32_t* begin, const int32_t* end, const int64_t* out_off, int N,
                    const double* fade_in, const double* fade_out, int ov, float* out, int16_t* pcm, long long out_len, void* stream);

/* ---------------------------------------------------------------- real-time sessions: the SOLA splice of one block step
 * Replaces the SOLA lines of the reference GUI's audio callback (real-time-gui.py, `audio_callback`: two conv1d, an argmax,
 * a slice at a device-resident index, the fade and the buffer update; restated from memory) for N streams in one call, with
 * the conventions of the assembly calls above: `slots` is HOST int32 [N] and is consumed before the call returns (kernel
 * arguments, one launch per 64 streams), arguments are checked before anything is launched, nothing synchronises, copies
 * or allocates on the device.
 *
 * Row k of `wave` (wave[k * stride + i]) is the vocoder output of stream slots[k]; x = wave[k] + start; b = row slots[k]
 * of sola_state [max_slots][Lb], read and written in place; fade_in / fade_out [Lb]: the caller's windows (float, device).
 *   score[o] = sum_{i<Lb} x[o+i] b[i] / sqrt(sum_{i<Lb} x[o+i]^2 + 1e-8)         o = 0 .. Ls, fp32, each sum from its own terms
 *   o*       = the lowest o with the highest score (an all-zero buffer gives 0);   offsets[k] = o*  (offsets may be NULL)
 *   y[i]     = float(float(x[o*+i] * fade_in[i]) + float(b[i] * fade_out[i]))  i < Lb;   y[i] = x[o*+i]  Lb <= i < block + Lb
 *   out[k][i] = y[i], i < block;   sola_state[slots[k]][i] = y[block + i], i < Lb   (the faded samples where block < Lb)
 * No sample at or above start + block + Lb + Ls of a row is read; rows of sola_state that no slot names are not touched.
 * N >= 0 (N == 0: success, no pointer is looked at), block >= 1, Lb >= 1, Ls >= 0, start >= 0,
 * start + block + Lb + Ls <= stride, 2 * Lb + Ls <= 16128 (the search is staged in LDS), 0 <= slots[k] < max_slots, no slot
 * twice in one call. */
int svc_sola_step(const float* wave, long long stride, int start, int N, float* sola_state, int max_slots, const int32_t* slots,
                  const float* fade_in, const float* fade_out, int block, int Lb, int Ls, float* out, int32_t* offsets,
                  void* stream);

/* svc_sola_step behind a prologue, in the same launch: output at a rate other than the model's (the GUI's
 * `resampler2` before SOLA) and the GUI's `infer_wav = zeros` while its VAD reports no speech.  svc_sola_step is this call with
 * r = NULL, speech = NULL and no `infer` row (the prologue is compiled out of that form).  Per stream k:
 *   y = what svc_resample gives for wave[k][start : start + n_in] alone (rs_dot4's ascending-k fp32 FMA chain, zeros outside the
 *       segment); the segment itself where r is NULL;  y = +0.0 everywhere where speech[k] == 0  (`speech`: HOST int32 [N],
 *       consumed before the call returns, NULL = all 1)
 *   infer[k] = y  (device out [N][block + Lb + Ls]: what SOLA saw), then svc_sola_step's arithmetic on y with start 0 and the given
 *       block, Lb, Ls, fade_in, fade_out, all at the output rate.
 * out, sola_state, offsets and infer are bit-identical to svc_resample on the slice followed by svc_sola_step on its result.
 * One workgroup per stream, one launch per 64 streams; the dynamic LDS is the larger of the two phases, at most 64 KB.
 * Refused (non-zero, nothing touched): everything svc_sola_step refuses, and block + Lb + Ls != svc_resample_len(o, n, n_in)
 * (!= n_in where r is NULL); start + n_in > stride; a resampler whose span is above the 16000 floats of svc_rt_push; infer NULL
 * or overlapping wave, sola_state, out, the windows or offsets; a speech entry other than 0 or 1. */
int svc_rt_out(const svc_resampler_t* r,       /* model rate -> output rate; NULL: equal rates */
               const float* wave, long long stride, int start, int n_in, int N,
               float* sola_state, int max_slots, const int32_t* slots,
               const int32_t* speech,          /* HOST int32[N] or NULL (= all 1), consumed before return */
               const float* fade_in, const float* fade_out, int block, int Lb, int Ls,
               float* infer,                   /* device out [N][block + Lb + Ls]: what SOLA saw */
               float* out, int32_t* offsets, void* stream);

/* svc_rt_out with the mute flags of a device-resident VAD (svc_vad_step below): speech_dev is DEVICE int32 [max_slots] or NULL.
 * Stream k is muted when its host speech[k] is 0 or speech_dev[slots[k]] == 0 (read once by the stream's workgroup, before
 * anything else).  With speech_dev == NULL this is svc_rt_out, bit for bit; svc_rt_out and svc_sola_step keep their forms.
 * Refused: everything svc_rt_out refuses, and speech_dev overlapping wave, infer, sola_state, out, the windows or offsets. */
int svc_rt_out_dev(const svc_resampler_t* r, const float* wave, long long stride, int start, int n_in, int N,
                   float* sola_state, int max_slots, const int32_t* slots, const int32_t* speech,
                   const int32_t* speech_dev,  /* DEVICE int32[max_slots] or NULL */
                   const float* fade_in, const float* fade_out, int block, int Lb, int Ls,
                   float* infer, float* out, int32_t* offsets, void* stream);

/* ---------------------------------------------------------------- FSMN voice activity detector
 * 16 kHz audio -> P(silence) per 10 ms frame -> speech segments and a mute flag per live stream: funasr's `fsmn-vad`
 * (WavFrontendOnline + FSMN + E2EVadModel), restated from memory; parity with the released checkpoint is not pinned.
 *
 * Front-end: Kaldi fbank (x 32768, DC removal, pre-emphasis 0.97, Hamming, 512-point power spectrum, 80 mel bins, log with
 * the fp32 epsilon floor), F(n) = n < 400 ? 0 : (n - 400) / 160 + 1 frames; LFR m = 5, n = 1: row i = frames i-2 .. i+2
 * (400 values), indices below 0 read frame 0 and, at a final call, indices above F - 1 read frame F - 1; then
 * (row + shift400) * scale400.  Rows R(n, final) = final ? F(n) : max(0, F(n) - 2) = svc_vad_rows.
 * Encoder: in_linear1 (400 -> 140) -> in_linear2 (140 -> 250) -> ReLU; 4 x { linear (250 -> 128, no bias) = p;
 * y[t] = (sum_{k<20} w[c][k] p[t - 19 + k], an fp32 FMA chain in ascending k) + p[t], rows before the stream's start zero;
 * affine (128 -> 250) -> ReLU }; out_linear1 (250 -> 140) -> out_linear2 (140 -> 248) -> softmax; p_sil = column 0.
 * `weights`: the state dict of the encoder, names with or without an "encoder." prefix:
 *   in_linear1.linear.{weight,bias}  in_linear2.linear.{weight,bias}  fsmn.{l}.linear.linear.weight
 *   fsmn.{l}.fsmn_block.conv_left.weight [128,1,20,1]  fsmn.{l}.affine.linear.{weight,bias}
 *   out_linear1.linear.{weight,bias}  out_linear2.linear.{weight,bias}
 * Every p_sil element's bits are a function of its row's samples and the 76 rows before it: not of the batch, the slot, N, the
 * segment split or the position of the row inside a call.
 *
 * Detector (integers only, one frame = 10 ms): frame t is speech iff p_sil[t] <= p_max in fp32 (NaN: silence).  A ring of the
 * last `win` decisions has the sum s; window state Sil: s >= on_count -> Speech; else window state Speech: s <= off_count ->
 * Sil.  Outside a segment a Sil -> Speech switch at t opens one: event (SVC_VAD_BEGIN, 10 max(prev_end, t - lookback)).
 * Inside one, sil_run counts consecutive frames whose window state is Sil; sil_run == end_silence: event (SVC_VAD_END, 10 t),
 * prev_end = t; otherwise t - begin + 1 >= max_segment: the same, and the ring and the window state are cleared.
 * flags[slot] = 1 iff the stream was inside a segment at any frame of this call (a segment that closes within it included);
 * a call that handles no frame leaves the flag alone.  events [N][8][2] = (kind, time_ms): the first 8 of the call are kept,
 * n_events counts all of them.
 *
 * `state`: svc_vad_state_floats(max_slots) floats, [max_slots][SVC_VAD_STATE_FLOATS]: the last 19 p rows of the four layers
 * (4 x 19 x 128 floats), then 32 int32 words (frames seen, ring bits, ring position, s, window state, in-segment, begin,
 * sil_run, prev_end; the rest reserved).  All zeros is a fresh stream; so is flags = 0.
 *
 * Conventions of svc_rt_push: host arrays (lens, n_rows, total, slots) are consumed before the call returns (they become
 * kernel arguments); every argument is checked before anything is launched, the handle last, and svc_last_error() names it; nothing
 * synchronises or allocates in steady state (scratch grows when a call needs more rows than any before it); rows of slots
 * that are not listed keep every bit; N and B in 1 .. 64; no slot twice; overlapping buffers are refused.
 *
 * svc_vad_scores: wave [B][L], lens[b] in 0 .. L; p_sil [B][svc_vad_rows(L, final)], row b holds svc_vad_rows(lens[b], final)
 * values, the rest is not written (p_sil may be NULL where svc_vad_rows(L, final) is 0).  A clip is cut into runs of seg_rows rows (0: the handle's default, else >= 16); a run that
 * does not start at row 0 first runs the 76 rows before it from zero caches and drops their output, which is bit-exact.
 * svc_vad_detect: p_sil [N][ld], row k has n_rows[k] <= min(ld, 6000) new frames of stream slots[k]; frame_speech (int32
 * [N][ld], may be NULL) receives the frame decisions; the thresholds are the handle's config.  Needs no weights: the op-level seam of the detector.
 * svc_vad_step: row k of x holds the stream's samples ending at x[k][end), the last n_new of them new, total[k] before them;
 * n_new a positive multiple of 160 up to 16000 and total[k] a multiple of 160; produces rows svc_vad_rows(total, 0) ..
 * svc_vad_rows(total + n_new, 0) - 1 into p_sil[k] (ld max_rows >= n_new / 160; may be NULL), runs the detector on them and
 * leaves flags[slot].  Reads svc_vad_history(total[k]) = min(total[k], 960) samples before the new ones: refused when
 * end - n_new is below that for a listed stream, or end > stride. */
typedef struct svc_vad_config {
    float p_max;                 /* 0.2 = (1 - speech_noise_thres 0.6) / 2 */
    int32_t win, on_count, off_count, lookback, end_silence, max_segment;   /* 20, 15, 15, 20, 65, 6000 */
    int32_t seg_rows;            /* default run length of svc_vad_scores; 0 = 512 */
} svc_vad_config_t;
typedef struct svc_vad svc_vad_t;
enum { SVC_VAD_BEGIN = 1, SVC_VAD_END = 2, SVC_VAD_MAX_EVENTS = 8, SVC_VAD_STATE_FLOATS = 4 * 19 * 128 + 32, SVC_VAD_MAX_ROWS = 6000 };
int svc_vad_create(const svc_vad_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, const float* shift400,
                   const float* scale400, void* stream, svc_vad_t** out);
void svc_vad_destroy(svc_vad_t* vad);
long svc_vad_rows(long n_samples, int final_);                 /* needs no GPU */
long svc_vad_history(long total);                              /* samples svc_vad_step reads before the new ones; needs no GPU */
long long svc_vad_state_floats(int max_slots);                 /* needs no GPU */
int svc_vad_scores(svc_vad_t* vad, const float* wave, const int32_t* lens /* HOST [B] */, int B, long L, int final_, int seg_rows,
                   float* p_sil, void* stream);
int svc_vad_detect(svc_vad_t* vad, const float* p_sil, long ld, const int32_t* n_rows /* HOST [N] */, int N,
                   const int32_t* slots /* HOST [N] */, int max_slots, float* state, int32_t* frame_speech, int32_t* events,
                   int32_t* n_events, int32_t* flags, void* stream);
int svc_vad_step(svc_vad_t* vad, const float* x, long long stride, long end, int n_new, const int64_t* total /* HOST [N] */, int N,
                 const int32_t* slots /* HOST [N] */, int max_slots, float* state, int32_t* flags, float* p_sil, int max_rows,
                 int32_t* events, int32_t* n_events, void* stream);

/* ---------------------------------------------------------------- real-time sessions: the audio history of one block step
 * (DESIGN.md 8l).  Replaces the `input_wav` / `input_wav_res` lines of the reference GUI's audio callback (two clone-shifts, a
 * resample of the last block with 2 zc samples of history, a slice copy; restated from memory) and the gather into the dense
 * batch a content encoder takes, for N streams in one launch.  Conventions of svc_sola_step: `slots` is HOST int32 [N],
 * consumed before the call returns; arguments are checked before anything is launched; nothing synchronises, copies or
 * allocates.
 *
 * Per listed stream, s = slots[k]:  m = Lin / zc;  x = hist[s] ‖ block[k] (2 zc + Lin samples);  y = what svc_resample gives for
 * x alone with r's taps (the same ascending-k fp32 FMA chain, zeros outside [0, len x)), y = x where r is NULL (equal rates);
 * shift = m z16, n_new = shift + z16;  with c_old the slot's context before the call,
 *     c[0 : L16 - n_new] = c_old[shift : L16 - z16]          c[L16 - n_new :] = y[z16 : z16 + n_new]
 * (the last z16 samples of a context are computed again by the next push, then with real audio to their right instead of zero
 * padding).  ctx[k] = c, the slot's context becomes c, hist[s] = x[-2 zc:].  Slots that are not listed keep every bit.
 *
 * `ring` holds svc_rt_ring_floats(max_slots, L16) = 2 max_slots (L16 + 1) floats: two planes [2][max_slots][L16], then
 * uint64 tickets[max_slots].  A push reads a slot's current plane and writes its other one, so no workgroup reads what another
 * writes; tickets[s] counts the workgroups that pushed to slot s, svc_rt_push_tiles(L16) per push, and the slot's current plane
 * is (tickets[s] / svc_rt_push_tiles(L16)) & 1.  All zeros is a valid start (empty contexts).  To clear a slot, zero both of its
 * planes and its hist row; its tickets word stays.  `ring` is 8-byte aligned; 16-byte accesses are used where shift, z16 and L16 are
 * multiples of 4 and ring and ctx are 16-byte aligned.
 *
 * Refused (non-zero, svc_last_error() names it, no state touched): Lin not a positive multiple of zc; L16 < n_new;
 * svc_resample_len(o, n, 2 zc + Lin) < z16 + n_new; zc % o != 0 or z16 % n != 0 (a block must start at resampling phase 0;
 * o = n = 1 for r == NULL); N outside 1 .. 64; a slot outside [0, max_slots) or listed twice; stride < Lin; null pointers;
 * block, hist, ring, ctx overlapping. */
int svc_rt_push_tiles(int L16);                          /* workgroups per stream and push; needs no GPU */
long long svc_rt_ring_floats(int max_slots, int L16);    /* floats to allocate for `ring`; needs no GPU */
int svc_rt_push(const svc_resampler_t* r,            /* NULL: equal rates, samples are copied */
                const float* block, long long stride, int Lin,   /* block[k][0..Lin): new samples of slots[k], stream rate */
                int N, const int32_t* slots, int max_slots,      /* HOST int32[N], consumed before return (as svc_sola_step) */
                int zc, int z16,                                  /* samples per 20 ms at the stream rate / content rate */
                float* hist,        /* [max_slots][2 zc]  state */
                float* ring,        /* state: svc_rt_ring_floats(max_slots, L16) floats, layout above */
                int L16,
                float* ctx,         /* out [N][L16]: row k = the new context of slots[k], dense, what the encoder takes */
                void* stream);

/* svc_rt_push behind the input noise gate of the reference GUI (a causal statement of the GUI's gate: its window
 * of 4 zc, hop zc, dB scale and off-switch, not its half-frame buffer offsets sample for sample).  svc_rt_push is this call with
 * the three gate arguments NULL.  Per listed stream s = slots[k], with m = Lin / zc frames of 20 ms:
 *   e_j = sum_{i<zc} block[k][j zc + i]^2 in fp32; the summation order is a function of zc alone, so a frame's energy does not
 *         depend on N, k, the slot, Lin or j;
 *   (g0, g1, g2) = gate_e[s]: the energies of the three raw frames before this block, oldest first; ..., g0, g1, g2, e_0, ...,
 *         e_{m-1} is the stream's sequence of frame energies;
 *   E_j = ((a + b) + c) + d over the four most recent frames ending at frame j, oldest first, in fp32: the energy of the last
 *         80 ms;
 *   frame j is muted when E_j < gate_pow[k] (a NaN energy never mutes); gate_mask[k][j] = 1 where it is, else 0;
 *   x' = the block with its muted frames replaced by +0.0; everything else is svc_rt_push on x', bit for bit: ctx, both ring
 *         planes, the ticket and hist (hist holds gated samples);
 *   gate_e[s] becomes the energies of the last three RAW frames of this block.  Energies are tracked while the gate is off
 *         (gate_pow NULL or 0.0f) too, so a threshold can be switched on in mid-stream; rows of gate_e of slots that are not
 *         listed keep every bit.
 * For a threshold in dB (RMS re 1.0) the host passes float(4 zc 10^(dB / 10)); at or below -60 dB it passes 0.0f, the GUI's "off".
 * Refused (nothing touched): everything svc_rt_push refuses, and gate_e NULL while gate_pow is given; a negative or NaN
 * gate_pow[k]; gate_e or gate_mask overlapping the other buffers or each other; Lin / zc above 256 while gate_e is given (the
 * frame energies of a block are held in LDS). */
int svc_rt_push_gated(const svc_resampler_t* r, const float* block, long long stride, int Lin, int N, const int32_t* slots,
                      int max_slots, int zc, int z16, float* hist, float* ring, int L16, float* ctx,
                      const float* gate_pow,   /* HOST float[N], consumed before return (as slots); NULL or 0.0f = gate off */
                      float* gate_e,           /* device state [max_slots][3]; zeros = a fresh stream                       */
                      int32_t* gate_mask,      /* device out [N][Lin / zc], 1 = frame muted; may be NULL                    */
                      void* stream);

/* ---------------------------------------------------------------- real-time sessions: pitch (csrc/rt_pitch.hip)
 * The drivers' pitch step (svc_f0_adjust: voiced-median shift in the log domain, semitone shift) for streams, which have no
 * "whole source" to take a median of: every slot keeps running voiced-pitch statistics on the device, in which each 10 ms frame
 * of the stream is counted exactly once, and the applied shift glides towards its target.  One launch for N streams;
 * conventions of svc_rt_push: `slots`, `auto_adjust` and `semitones` are HOST arrays consumed before the call returns,
 * arguments are checked before anything is launched, nothing synchronises, copies or allocates.
 *
 * `state`: svc_rt_pitch_state_words(max_slots) int32 words, [max_slots][SVC_RT_PITCH_STATE_WORDS]; per slot
 *   words 0 .. 1535  the histogram of voiced frames, 256 bins per octave over [32, 2048) Hz;
 *   word 1536        n, the number of voiced frames counted so far;
 *   word 1537        the bits of the float s, the log shift that was applied by the last call;
 *   word 1538        the median bin the last call found (0 while n == 0);  words 1539 .. 1543 are reserved and kept.
 * All zeros is a fresh stream.  Per listed stream s = slots[k], in this order:
 *   counted frames: the frames i in [Tf - lag - n_new, Tf - lag) of row k.  A block advances the context by exactly n_new frames
 *         (n_new = 2 Lin / zc at hop 160), so every frame of the stream is counted exactly once, when it is `lag` frames from the
 *         end of the context (the last frames of a context are provisional: the next push computes their samples again);
 *   voicing and binning: a counted frame is voiced iff f0 > 1.f (svc_f0_adjust's rule; NaN is unvoiced).  A voiced frame adds 1
 *         to state[s][bin], bin = clamp((float_bits(f0) >> 15) - 33792, 0, 1535): the bit pattern of f0 itself, no
 *         transcendental, so a host statement reproduces it in exact integers; values outside [32, 2048) Hz, +inf included, go
 *         to the end bins.  n grows by the number of voiced counted frames;
 *   running median: r = (n - 1) / 2, the lower-middle rank (torch's rule, as svc_f0_adjust); the median bin is the first bin
 *         whose cumulative count exceeds r, in the histogram that includes this call's frames;  m_run = logf(c + 1e-5f) with c
 *         the float of bits ((bin + 33792) << 15) | 0x4000, the bin's centre;
 *   target: d = ref_median[s] - m_run when auto_adjust[k] != 0, n >= max(warmup, 1) and ref_median[s] > 0, else d = 0.  A voiced
 *         median is the log of a float above 1, so it is positive; 0 (what svc_f0_adjust's `medians` holds for a reference
 *         without a voiced frame), a negative value or NaN stands for "no reference" and gives no shift, as svc_f0_adjust
 *         applies none when a side has no voiced frame;
 *   glide: with s_old the float of word 1537, s_new = d when |d - s_old| <= max_step or the step is off (max_step <= 0 or
 *         +inf): arrival is exact; otherwise s_new = s_old + max_step when d > s_old, else s_old - max_step.  Word 1537 becomes
 *         s_new, shift_out[k] = s_new;
 *   output, for all i < Tf, lg = logf(f0 + 1e-5f), factor = exp2f(semitones[k] * (1.f / 12.f)):
 *         out = expf(s_new == 0 ? lg : lg + s_new) * factor     voiced frames
 *         out = expf(lg)                                        unvoiced frames
 *         (the expressions of svc_f0_adjust: with auto_adjust[k] == 0 and s_old == 0 the row equals
 *         svc_f0_adjust(auto_adjust = 0) bit for bit).
 * Rows of slots that are not listed keep every bit.  A stream's state and output are a function of its own frames and settings
 * alone: not of N, k, the slot or its companions; all counting is in integers, so no result depends on an order.  The statistics
 * never forget: a stream that changes register keeps the median of its whole past until the slot's row is zeroed.
 *
 * Refused (non-zero, svc_last_error() names it, nothing touched): n_new < 1, lag < 0 or Tf - lag - n_new < 0; N outside 1 .. 64;
 * a slot outside [0, max_slots) or listed twice; stride or out_stride below Tf; warmup < 0; a NaN max_step; a semitones entry
 * that is not finite; null pointers (semitones and shift_out may be NULL); out overlapping f0 or state. */
enum { SVC_RT_PITCH_BINS = 1536, SVC_RT_PITCH_STATE_WORDS = 1536 + 8 };
long long svc_rt_pitch_state_words(int max_slots);          /* int32 words to allocate for `state`; needs no GPU */
int svc_rt_pitch(const float* f0, long long stride, int Tf,  /* f0[k][0..Tf): Hz, the RMVPE track of slots[k]'s context */
                 int n_new, int lag,                         /* frames a block renews; frames at the end that are still provisional */
                 int N, const int32_t* slots, int max_slots, /* HOST [N], consumed before return (as svc_rt_push) */
                 int32_t* state,                             /* device [max_slots][SVC_RT_PITCH_STATE_WORDS]; zeros = fresh stream */
                 const float* ref_median,                    /* device [max_slots]: log-domain median of the slot's reference */
                 const int32_t* auto_adjust,                 /* HOST [N] 0/1 */
                 const float* semitones,                     /* HOST [N] or NULL (= 0) */
                 int warmup, float max_step,                 /* voiced frames before the median is used; largest change of the
                                                                applied log shift per call (<= 0 or +inf: none) */
                 float* out, long long out_stride,           /* out[k][0..Tf): the shifted track the regulator takes */
                 float* shift_out,                           /* device [N] applied log shift, or NULL */
                 void* stream);

/* ---------------------------------------------------------------- real-time sessions: pitch on the context's tail
 * svc_rt_pitch for a stream whose RMVPE track covers only the LAST W frames of its context: every slot keeps the raw track of
 * its whole context in a cache row that moves with the stream, and (memory > 0) the bins of its last `memory` counted frames
 * in a ring, so that the statistics forget.  One launch, one workgroup per listed stream, conventions and state of svc_rt_pitch.
 *
 * `cache`: svc_rt_pitch_cache_words(max_slots, Tf) floats, [max_slots][Tf], raw Hz; zeros = a fresh stream (0 Hz is unvoiced).
 * `ring`:  svc_rt_pitch_ring_words(max_slots, memory) int32 words, [max_slots][memory + 2]; per slot
 *   words 0 .. memory - 1  the entries: the bin of a counted voiced frame, or -1 for a counted unvoiced frame;
 *   word memory            head, the index of the oldest entry;   word memory + 1   fill, the number of entries held.
 *   All zeros is a fresh stream.  memory == 0 with ring == NULL: the statistics never forget (svc_rt_pitch's).
 * Per listed stream s = slots[k], with `old` the slot's cache row before the call, in this order:
 *   cache update: new[i] = f0_win[k][i - (Tf - W)]   for i >= Tf - W + guard   (the window's frame j is context frame Tf - W + j;
 *                 new[i] = old[i + n_new]             for i <  Tf - W + guard    its first `guard` frames are not trusted)
 *         W - guard >= n_new, so i + n_new < Tf and no frame is left unwritten.  cache[s] becomes new; raw_out[k] = new.
 *   counted frames: the frames i in [Tf - lag - n_new, Tf - lag) of new, voicing and binning as svc_rt_pitch:
 *         voiced iff new[i] > 1.f, bin = clamp((float_bits(new[i]) >> 15) - 33792, 0, 1535);
 *   forgetting (memory > 0): the ring is a FIFO of `memory` entries.  The counted frames are pushed in frame order; with
 *         fill the count before the call, e = max(0, fill + n_new - memory) entries are pushed out: the oldest e, those at
 *         (head + j) % memory for j < e.  An entry pushed out that is a bin takes 1 from state[s][bin] and from n.  Counted frame
 *         j goes to (head + fill + j) % memory; then head = (head + e) % memory, fill = fill + n_new - e.  So n, the rank
 *         r = (n - 1) / 2, the median bin and the comparison with `warmup` are over what the ring holds; when n falls below
 *         max(warmup, 1) the target is 0 and the shift glides there;
 *   running median, target, glide, words 1536 .. 1538, shift_out and the Tf outputs over new: svc_rt_pitch's, by the same
 *         device code (with memory == 0 the call equals svc_rt_pitch on raw_out[k] bit for bit).
 * Rows of slots that are not listed keep every bit of cache, ring and state.  A stream's state, cache, ring and output are a
 * function of its own frames and settings alone: not of N, k, the slot or its companions.  The shift of the cache is in
 * place: a workgroup stages its whole row in LDS across a barrier before it stores a frame, so Tf is at most
 * SVC_RT_PITCH_WIN_MAX_TF = 4096 frames (16 KB of LDS; 41 s of context); any n_new is safe.
 *
 * Refused (non-zero, svc_last_error() names it, nothing touched): everything svc_rt_pitch refuses (stride is compared with W);
 * Tf above SVC_RT_PITCH_WIN_MAX_TF; W < 1 or W > Tf; guard < 0; W - guard < n_new; memory < 0, or 0 < memory < n_new; ring NULL
 * while memory > 0 or given while memory == 0; cache NULL; raw_stride below Tf while raw_out is given; out or raw_out overlapping
 * f0_win, cache, state, ring or each other; f0_win, cache, state and ring overlapping one another. */
enum { SVC_RT_PITCH_WIN_MAX_TF = 4096 };
long long svc_rt_pitch_cache_words(int max_slots, int Tf);       /* floats to allocate for `cache`; 0 for arguments out of range */
long long svc_rt_pitch_ring_words(int max_slots, int memory);    /* int32 words to allocate for `ring`; 0 for memory == 0 */
int svc_rt_pitch_win(const float* f0_win, long long stride,      /* f0_win[k][0..W): Hz, the RMVPE track of the last samples of slots[k]'s context */
                     int W, int guard, int Tf,                   /* window frames; untrusted frames at its start; frames of a context */
                     int n_new, int lag, int N, const int32_t* slots, int max_slots,     /* as svc_rt_pitch */
                     float* cache,                               /* device [max_slots][Tf]; zeros = fresh stream */
                     int32_t* ring, int memory,                  /* device [max_slots][memory + 2], or NULL with memory == 0 */
                     int32_t* state, const float* ref_median, const int32_t* auto_adjust, const float* semitones, int warmup,
                     float max_step,                             /* as svc_rt_pitch */
                     float* out, long long out_stride,           /* out[k][0..Tf): the shifted track over new */
                     float* raw_out, long long raw_stride,       /* raw_out[k][0..Tf) = new, or NULL */
                     float* shift_out, void* stream);

/* ---------------------------------------------------------------- op-level entry points (parity tests) */
/* C[M][N] (fp32) = act(A[M][K] * W[N][K]^T + bias) ; dtype 0: operands rounded to fp16, 1: fp32 MFMA.  act: a KG_ACT_* value
 * (0 none, 1 SiLU, 2 ELU, 3 leaky ReLU 0.1, 4 tanh, 5 abs, 6 clamp, 7 sigmoid, 8 GELU in the exact erf form). */
int svc_op_linear(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, int dtype,
                  int act, void* stream);
/* Channels-last Conv1d through the tap-GEMM: x [B][L][Cin], w [Cout][Cin][k] (torch layout),
 * y [B][Lout][Cout]; pad_mode 0 zero / 1 reflect / 2 replicate; explicit left pad. */
int svc_op_conv1d(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout,
                  int k, int dilation, int stride, int pad_left, int Lout, int pad_mode, int dtype, void* stream);
/* Test aid (tests/test_gpu_kconv.py; no model uses it): one stride-1, zero-padded channels-last Conv1d with everything a
 * ConvRun of the vocoders can carry, and a report of the kernel that ran.  Device pointers unless noted; NULL = absent.
 *   x [B][L][Cin] fp32, or a_hi / a_lo: ready operand planes [B][L][cin_pad] (16-bit words, cin_pad = Cin rounded up to 64) as
 *   a fused Snake wrote them;  w [Cout][Cin][k], bias [Cout].
 *   dtype 0 fp16, 2 fp16x3, 3 fp16 + fp8 corrections (lo plane as byte pairs; needs a shape the resident-tile kernel takes).
 *   seq_len: HOST [B] valid input rows per sequence (the ragged form; needs Lout == L).
 *   epilogue, in this order: + bias, act (KG_ACT_* value, act_slope), + res, * out_scale (0 = 1), + res2;
 *   y, res, res2 [B][c_rows][Cout] fp32 (c_rows 0 = Lout); the conv writes rows c_off .. c_off + Lout of y, the others are kept.
 *   res and / or res2 may be y itself: the conv then runs in place, reading the addend from the buffer it writes.
 *   post_a / post_ib [Cout]: fused Snake sv = v + post_ib sin^2(post_a v) towards plane_hi / plane_lo [B][c_rows][cout_pad]
 *   (raw 16-bit words over all cout_pad = Cout rounded up to 64 columns, written in place): hi = fp16(sv), lo = fp16(sv - hi) or,
 *   with next_p8, the byte pair (fp8(hi), fp8(2^11 (sv - hi))); y keeps v.
 *   bm: resident-tile position-tile override 64 | 128 | 256 (0 = the launch's choice; 128-channel form only).
 *   force_gemm: run on the tap-GEMM (not with byte-pair planes).
 *   took (out): 0 = tap-GEMM; else bit 0 set, bits 8..19 = BM, bits 20.. = BN of the resident-tile instantiation launched. */
typedef struct {
    const float* x; const uint16_t* a_hi; const uint16_t* a_lo;
    const float* w; const float* bias;
    int32_t B, L, Cin, Cout, k, dilation, pad_left, Lout, dtype;
    const int32_t* seq_len;
    const float* res; const float* res2;
    float out_scale; int32_t act; float act_slope;
    int32_t c_rows, c_off;
    const float* post_a; const float* post_ib; int32_t next_p8;
    int32_t bm, force_gemm;
    float* y; uint16_t* plane_hi; uint16_t* plane_lo;
    int32_t took;
} svc_conv1d_ex_t;
int svc_op_conv1d_ex(svc_conv1d_ex_t* args, void* stream);
/* Test aid: the `took` word of this thread's last successful svc_op_conv1d or svc_op_conv1d_ex call (the first has no argument
 * for it). */
int svc_op_conv1d_last_took(void);
/* Test aid (tests/test_gpu_panel.py; no model uses it): ONE launch of the fused DiT row-panel kernel (csrc/fused.hip) on
 * unpacked nn.Linear weights.  The call packs the given weights with the model's own packers into a temporary stream in the
 * model's order ([merge | wo, mlp | skip | qkv | head]), launches once and synchronises.  Device pointers; NULL = absent.
 *   D 384 | 512, I a multiple of 32, gated: the AdaLN-zero form (x += gate * ...), tm: 16-row tiles per wave 1 | 2, 0 = the
 *   launcher's choice.  Local row m < M = n_seq * Lout is buffer row (m / Lout) * seq_rows + row_off + m % Lout; every
 *   activation buffer has n_seq * seq_rows rows, row_off + Lout <= seq_rows.
 *   phases: do_post (wo, w1, w3 [I][D], w2 [D][I], ao, g_ffn, optional gates and w_f / b_f; c16 = fp16 copy of its output),
 *   do_skip (wskip [D][2 D], skip_in, bskip), do_final (g_fin, w_fin, b_fin -> n16), do_qkv (wqkv [3 D][D], g_attn, w_a, b_a,
 *   rope [>= row_off + Lout][32][2] -> qk [rows][2 D], vt[seq][d][vt_pos(position, vt_mode)] with vt_ld >= the written positions
 *   rounded up to 32).  norm vectors: A = g * (add_one + w), or g without w.
 *   seam 1 (merge, with do_qkv alone, row_off 0): x[seq][pos] = tok_time (time_first and pos 0) | tok_style[seq] for pos < npre,
 *   st_term[seq][pos] + w_merge[:, :C] x16[seq][pos - npre] for npre <= pos < npre + T, zeros beyond; w_merge [D][ldw], C <= 128,
 *   x16 [n_seq][seq_rows][128] (columns >= C are multiplied by zero weights), st_term [n_seq][seq_rows][D].
 *   seam 2 (head, with do_post and do_final, no c16): v32[row][< head_C] = head_w2 silu(head_wa n + head_b0) + head_b2 on the
 *   final-norm rows n; head_wa [D][D], head_w2 [head_C][D], head_C 16 .. 128 in steps of 16, ldv >= head_C; n16 is not
 *   written, and x is scratch (the gated form leaves x + gate_a * wo(ao) there, the ungated form leaves it alone).
 *   x is read and written in place.  Refused (nothing launched): whatever fused_panel_launch refuses, a launch without a
 *   streamed phase, and a NULL operand of an enabled phase. */
typedef struct {
    int32_t D, I, gated, tm;
    int32_t M, Lout, seq_rows, row_off, n_seq;
    float eps; int32_t add_one;
    int32_t do_post, do_skip, do_qkv, do_final, seam;
    const float* wo; const float* w1; const float* w3; const float* w2; const float* wskip; const float* wqkv;
    const float* w_merge; int32_t ldw, C;
    const float* head_wa; const float* head_w2;
    const float* gate_a; const float* gate_f;
    const float* g_ffn; const float* w_f; const float* b_f;
    const float* g_attn; const float* w_a; const float* b_a;
    const float* bskip;
    const float* g_fin; const float* w_fin; const float* b_fin;
    const float* head_b0; const float* head_b2;
    const float* tok_time; const float* tok_style;
    const uint16_t* ao; const uint16_t* skip_in; const uint16_t* x16;
    float* x; const float* st_term;
    uint16_t* c16; uint16_t* n16; uint16_t* qk;
    uint16_t* vt; int64_t vt_seq_stride, vt_ld; int32_t vt_mode;
    float* v32; int32_t ldv, head_C;
    const float* rope; float q_scale;
    int32_t npre, time_first, T;
} svc_dit_panel_t;
int svc_op_dit_panel(const svc_dit_panel_t* args, void* stream);
/* ConvTranspose1d (k = 2*stride, padding = stride/2): x [B][L][Cin], w [Cin][Cout][k], y [B][L*stride][Cout]. */
int svc_op_conv_transpose1d(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin,
                            int Cout, int k, int stride, int dtype, void* stream);
/* softmax(q k^T / 8 + key-padding mask) v ; q,k,v,out [N][T][H][64] fp32 (computed in fp16 MFMA). */
int svc_op_attention(const float* q, const float* k, const float* v, float* out, int N, int T, int H,
                     const int64_t* kv_lens_host, void* stream);
/* Test aid (tests/test_gpu_attention.py; no model uses it): ONE attention launch on buffers that are ALREADY in the kernels' layout.
 * Nothing is packed, permuted or padded, so the caller owns every byte the kernels read.  Device pointers, fp16:
 *   q, k [n_seq * seq_rows][ld_qk] with head h at column 64 h (separate buffers, or two column blocks of one), q pre-scaled by
 *   log2(e) / 8; vt [n_seq][H * 64][vt_ld] with key p of a sequence at column vt_pos(p, vt_perm) (0 natural, 1 and 2 the orders of
 *   the 16x16x32 and the 32x32x16 kernels, which vt_perm thereby selects); out (fp16) or out32 (fp32) [n_seq * seq_rows][ld_out],
 *   exactly one of them.  Queries [q_start, Tq) of every sequence are computed, over keys [0, kv_len[seq]) (HOST array) or
 *   [0, kv_len_const) when kv_len is NULL; rows outside are not written; kv_len 0 gives zero rows.  qt_form: 0 = by the grid size,
 *   1 = 64-query workgroups, 2 = 128-query workgroups.  K rows at and past kv_len may hold anything; V^T columns
 *   [kv_len, round_up(kv_len, 64)) must hold finite values (they meet P = 0 in the MFMA); nothing past that is read.
 *   Refused, before anything is allocated or launched: a NULL q, k or vt; both or neither of out and out32; vt_perm or qt_form
 *   outside 0 .. 2; n_seq or H < 1; Tq < 1 or > seq_rows; q_start < 0 or >= Tq; a kv_len < 0, > seq_rows or with
 *   round_up(kv_len, 64) > vt_ld; vt_seq_stride < H * 64 * vt_ld; ld_qk or ld_out < H * 64; vt_ld not a multiple of 64, ld_qk or
 *   vt_seq_stride not of 8, ld_out not of 4; q, k, vt, out32 not 16-byte or out not 8-byte aligned. */
typedef struct {
    const uint16_t* q; const uint16_t* k; const uint16_t* vt;
    uint16_t* out; float* out32;
    int64_t ld_qk, vt_seq_stride, vt_ld, ld_out;
    int32_t n_seq, H, seq_rows, Tq, q_start;
    const int64_t* kv_len;
    int32_t kv_len_const, vt_perm, qt_form;
} svc_attention_t;
int svc_op_attention_ex(const svc_attention_t* args, void* stream);
/* Test aid (tests/test_gpu_vocoder_pointwise.py; no model uses it): ONE call of the vocoders' channels-last activation launch
 * (csrc/aa_act.hip, act_cl_launch) with every argument taken as given.  Device pointers unless noted.
 *   x fp32 [B][L][ldx]; y_hi and y_lo planes [B][L][ldy]: fp32 (out_f16 0, no y_lo) or 16-bit words (out_f16 1; y_lo may be NULL);
 *   lo_fmt 0: y_lo = fp16(v - hi), 1: the byte pair (fp8(hi), fp8(2^11 (v - hi))); taps: the 12 filter taps, by value;
 *   a, inv_b [C]; mode 0 anti-aliased Snake, 1 Snake v + inv_b sin^2(a v), 2 leaky ReLU with `slope`;
 *   lens: HOST [B] valid rows per sequence (mode 0 only) or NULL.
 *   Refused (nothing launched): NULL x or y_hi; B, C or L < 1; ldx or ldy < C; mode outside 0 .. 2; a Snake mode without a and
 *   inv_b; lo_fmt outside 0 .. 1, or 1 without y_lo; y_lo or lo_fmt with the fp32 output; lens with mode 1 or 2, or outside
 *   [0, L]; x not 8-byte or a plane not 4-byte aligned. */
typedef struct {
    const float* x; void* y_hi; void* y_lo;
    int64_t ldx, ldy;
    int32_t out_f16, lo_fmt;
    float taps[12];
    const float* a; const float* inv_b;
    int32_t B, C, L, mode;
    float slope;
    const int32_t* lens;
} svc_act_cl_t;
int svc_op_act_cl(const svc_act_cl_t* args, void* stream);
/* Test aid (tests/test_gpu_vocoder_pointwise.py; no model uses it): ONE signal stage of HiFT (csrc/vocoder.hip) on explicit
 * buffers, through the launcher the model calls.  Device pointers unless noted; NULL = absent.  Rows: B micro-batch rows; row j
 * is utterance src[j] (HOST [B]; NULL: j) of the caller's n_utt-utterance tensors and holds len[j] (HOST [B]; NULL: S) frames.
 *   stage 1  phase prefix + source, loaded noise: in = f0 [B][S], phase0 [n_utt][NH], noise [n_utt][NH][S_in * up], lin_w [NH],
 *            lin_b [1] -> out fp32 [B][S * up]; scalars NH, up, sr, sine_amp, noise_std, voiced_thr
 *   stage 2  STFT: in = s [B][Lw] -> out fp32 [B][F][ld] (9 real | 9 imaginary | zeros); lw, nf HOST [B] or NULL (Lw, F)
 *   stage 3  frames: in = [B * F][ld] (9 log-magnitudes | 9 phase pre-activations) -> out fp32 [B * F][16]
 *   stage 4  overlap-add: in = frames [B][F][16] -> out fp32 [n_utt][Lw], row src[j]; lw, nf as in stage 2; limit
 *   stage 5  mel_to_cl: in = mel [n_utt][C][S_in] -> out (and out_lo) [B][S][ld]; vd 0 fp16, 1 fp32, 2 | 3 fp16 hi + lo
 *   stage 6  ew_cl: in = [B * S][ld] -> out (and out_lo) [B * S][ld]; vd as above; mode 2 leaky ReLU with `slope`, 3 cast
 *   Refused (nothing launched): a stage outside 1 .. 6; NULL in or out; B or n_utt < 1; src outside [0, n_utt) (without src: B >
 *   n_utt); stages 1, 5: S < 1, S_in < S, len outside [0, S]; stages 2, 4: F or Lw < 1, one of lw and nf alone, lw outside
 *   [0, Lw], nf outside [0, F]; stage 2: ld < 18, a row with frames and lw < 9 or nf > lw / 4 + 1; stage 3: ld < 18;
 *   stages 5, 6: vd outside 0 .. 3, C < 1, ld < C, a split mode without out_lo; stage 6: a mode other than 2 or 3. */
typedef struct {
    int32_t stage;
    const float* in; const float* phase0; const float* noise; const float* lin_w; const float* lin_b;
    void* out; void* out_lo;
    int32_t B, n_utt, NH, up;
    float sr, sine_amp, noise_std, voiced_thr, limit;
    int32_t S, S_in, F;
    int64_t Lw;
    int32_t ld, C, vd, mode;
    float slope;
    const int32_t* src; const int32_t* len; const int32_t* lw; const int32_t* nf;
} svc_hift_signal_t;
int svc_op_hift_signal(const svc_hift_signal_t* args, void* stream);
/* Test aid (tests/test_gpu_voc_plan.py; no model uses it): ONE range census (csrc/range_census.hip, census_launch) of explicit
 * operand planes, through the launcher svc_*_calibrate calls.  hi, lo: DEVICE fp16 planes [B][L][ld] (lo = the fp16 residual),
 * C live channels; lens: HOST [B] valid rows per sequence or NULL (rows at and above lens[b] are never read: they may hold
 * NaN); out: HOST, one record.
 *   Refused (nothing launched): NULL args, hi, lo or out; B, L or C < 1; B * L >= 2^31; ld < C or ld % 4 != 0; a plane not
 *   8-byte aligned; lens outside [0, L]. */
typedef struct {
    const void* hi; const void* lo;
    int32_t B, L, C, ld;
    const int32_t* lens;
    svc_census_t* out;
} svc_range_census_t;
int svc_op_range_census(const svc_range_census_t* args, void* stream);
/* Test aid: the pack-time weight census of one Conv1d.  w DEVICE fp32 [Cout][Cin][k] is packed as an fp16p8 model packs it
 * (fp16x3 rows and [w_hi | fp8 byte pairs] rows with one power-of-two scale s = 2^w8_exp from max|w|); out HOST
 * [Cout][4] doubles per output channel: sum w_hi^2, sum (w_hi - dq fp8(s w_hi) / s)^2, sum w_lo^2, sum (w_lo - dq fp8(2^11 s
 * w_lo) / (2^11 s))^2; w8_exp_out (HOST, optional) receives log2 s.
 *   Refused: NULL w or out; Cout or Cin < 1; k outside 3 .. 16 (a conv with fewer taps gets no fp8 packing). */
int svc_op_weight_census(const float* w, int Cout, int Cin, int k, double* out, int* w8_exp_out, void* stream);
/* Test aids (tests/test_host_voc_plan.py; they need no device).  svc_op_plan_fake: a BigVGAN handle of `precision` that holds
 * nothing but a precision plan of n_candidates (<= 96) candidates named resblocks.<i>.convs{1,2}.<d>; it supports the
 * svc_bigvgan_plan_* calls, the refusals of svc_bigvgan_calibrate, svc_op_plan_apply and svc_bigvgan_destroy, nothing else.
 * svc_op_plan_apply: the decision step of calibrate alone on the caller's rows -- rows[i].veto = rho, eta, omega_hi or
 * omega_lo above tau, ORed into the plan. */
int svc_op_plan_fake(int precision, int n_candidates, svc_bigvgan_t** out);
int svc_op_plan_apply(svc_bigvgan_t* m, svc_plan_row_t* rows, int n_rows, float tau);
/* Test aid (tests/test_gpu_ar_sampler.py; no model uses it, and it needs no svc_ar_t): ONE call of the AR sampler's launch
 * (csrc/ar_sampler.h) on explicit inputs.  It allocates the rank -> sample buffers, the slot state, the slot count and the
 * device positions itself, launches once, synchronises, copies the state back and frees its buffers.  Device pointers
 * unless noted; NULL = absent.  The contract of the sampler is that of svc_ar_sample.
 *   form 0  explicit: ar_sampler_launch without loop state.  logits [V], prev [n_prev], suppress (negative: none), rep_pen,
 *           temperature, top_p; draws exp_noise [V], or NULL: those of (seed, step), as the generate loops draw them
 *           -> idx_out [1], probs_out [V] (optional).
 *   form 1  one sequence's loop state (GenState): logits [V], toks [max_new] (read: toks[0]; written: toks[cnt]), noise
 *           [max_new][V] or NULL (seeded), emb [V][D] -> next_x [D], probs_out [V] (optional).  The per-slot HOST arrays
 *           below hold one entry; s_done, s_max_new and s_has_noise are not read.  pos HOST [2] (input, kv), in and out.
 *   form 2  B slots (GenSlot) of Bp = B rounded up to 16 rows, *nb = B: ar_sampler_batch_launch.  logits [Bp][V], toks
 *           [B][max_new], noise [B][max_new][V] (rows of slots with s_has_noise; may be NULL when none has), emb [V][D]
 *           -> next_x [Bp][D].  pos HOST [2][B], in and out.  max_new is the row stride; a slot's own limit is s_max_new[b].
 *   HOST per-slot arrays [B]: s_cnt (in and out), s_done (in and out), s_max_new, s_min_before_eos, s_eos, s_temperature,
 *   s_top_p, s_rep_pen, s_seed, s_has_noise.
 *   Token values inside prev and toks live on the device and are NOT checked: the caller keeps them in [0, V).
 *   Refused (nothing allocated or launched): form outside 0 .. 2; V outside 1 .. 4096; NULL logits; form 0: NULL idx_out,
 *   n_prev < 0 or tokens without prev, suppress >= V, a NaN or negative rep_pen, step < 0; forms 1, 2: max_new or D < 1,
 *   missing emb, next_x, toks, pos or per-slot arrays, a slot's max_new outside [1, max_new], cnt < 1, cnt >= max_new (form
 *   2: cnt > max_new, or cnt == max_new in a slot that is not done -- token cnt is written at toks[cnt]), eos outside [0, V),
 *   a NaN or negative rep_pen; form 2: B outside 1 .. 64, Lmax < 1, a position outside [0, Lmax), a slot with noise and no
 *   noise buffer. */
typedef struct {
    int32_t form, V, D, B, max_new, Lmax;
    const float* logits;
    const int32_t* prev;
    int32_t n_prev, suppress;
    float rep_pen, temperature, top_p;
    const float* exp_noise;
    uint64_t seed;
    int32_t step;
    int32_t* idx_out; float* probs_out;
    int32_t* toks; const float* noise; const float* emb; float* next_x;
    int32_t* s_cnt; int32_t* s_done;
    const int32_t* s_max_new; const int32_t* s_min_before_eos; const int32_t* s_eos;
    const float* s_temperature; const float* s_top_p; const float* s_rep_pen;
    const uint64_t* s_seed;
    const int32_t* s_has_noise;
    int32_t* pos;
} svc_ar_sampler_t;
int svc_op_ar_sampler(const svc_ar_sampler_t* args, void* stream);
/* Test aid (tests/test_gpu_ar_step.py; no model uses it, and it needs no svc_ar_t): ONE call of the launch function of an AR
 * kernel that reads or writes the KV cache (csrc/ar_prefill.h, ar_decode1.h, ar_batch.h, ar_prefill_attn.h), on explicit
 * buffers.  It builds the device tables the launch needs (cache bases per slot, positions, live-slot count, PrefillTabs),
 * launches once, synchronises and frees them.  Device pointers unless noted.  D = 64 H, kvd = 64 Hkv.
 *   kc, vc  the caches of n_slots slots, [n_slots][Hkv][Lmax][64] fp32;  rope [Lmax][32][2] fp32 (cos, sin), taken as given
 *   slots   HOST: the slot of the call (kinds 0, 1, 4: one entry), of every row (kind 2: [n]) or of every sequence (kinds 3, 5: [n])
 *   pos     HOST [2][R]: input_pos of the R rows, then kv_pos (kind 1: R = 1; kinds 0, 4: R = n; kind 2: R = n; kinds 3, 5: the
 *           rows of the n sequences one after another, R = sum of seq_S)
 *   kind 0  ar_attn_launch: x = q [n][D] -> y16 [n][D]; reads rows 0 .. kv_pos of the slot's cache and nothing above
 *   kind 1  dec_attn2_launch: x = qkv_raw [D + 2 kvd], hres [D], eps, rope, wo fp16 [D][D] -> part [H][D] and cache row kv_pos.
 *           Rows above kv_pos MAY be read (by position, clamped to the cache) and must be finite; row kv_pos is never used
 *   kind 2  battn_launch: x = q [Bp][D], Bp = n rounded up to 16, *nb = n -> y16 [Bp][D] (rows >= n untouched).  The cache table
 *           holds slots[b] for b < n and NULL above.  Reads rows 0 .. kv_pos[b] only
 *   kind 3  ar_prefill_attn_launch: x = q [R][D], tiles of 16 rows per sequence as the ragged prefill builds them -> y16 [R][D].
 *           Reads rows 0 .. the tile's largest kv_pos only
 *   kind 4  ar_rope_cache_launch: x = qkv [n][ldq] -> q_out [n][D], cache rows kv_pos of the slot
 *   kind 5  ar_rope_cache_ragged_launch: x = qkv [R][ldq] -> q_out [R][D], cache rows kv_pos of each row's slot
 *   Refused (nothing allocated or launched): NULL args; kind outside 0 .. 5; H or Hkv < 1, H > 64, H % Hkv != 0; Lmax outside
 *   8 .. 8192; n_slots outside 1 .. 64; NULL x, kc, vc, slots or pos; n < 1 (kinds 0, 4: n > 8192; kinds 2, 3, 5: n > 64); a
 *   slot outside [0, n_slots); a slot named twice (kinds 2, 3, 5); kinds 3, 5: NULL seq_S, seq_S[i] < 1, R > 8192; a position
 *   outside [0, Lmax); kinds 0, 2, 3: NULL y16; kinds 1, 4, 5: NULL rope; kinds 4, 5: NULL q_out, ldq < D + 2 kvd; kind 1:
 *   NULL hres, wo or part, D > 1024 (the shapes for which svc_ar_create keeps the decode step). */
typedef struct {
    int32_t kind, H, Hkv, Lmax, n_slots, n;
    const float* x;
    int64_t ldq;
    float* kc; float* vc;
    const float* rope;
    const int32_t* slots; const int32_t* seq_S; const int32_t* pos;
    void* y16; float* q_out;
    const float* hres; float eps; const void* wo; float* part;
} svc_ar_attn_t;
int svc_op_ar_attn(const svc_ar_attn_t* args, void* stream);
/* Test aid (tests/test_gpu_ar_step.py; no model uses it, and it needs no svc_ar_t): ONE call of the launch function of a skinny
 * AR linear on explicit buffers, with the template instance the model selects for (D, I, H) and the row count.  W is fp16, packed
 * as svc_ar_create packs it: row-major [N rounded up to 128][K] (rows >= N are read by the batched path and must be finite).
 * Nqkv = D + 2 * 64 Hkv.  role: 0 qkv, 1 wo, 2 w13, 3 w2, 4 head.
 *   path 0  gemv_pair_launch, rows = S in 1 .. 8:
 *           qkv  x fp32 [S][D], gamma, eps, W [Nqkv][D] -> q_out [S][D], cache rows (kc, vc, rope, slots[0], pos HOST [2][S])
 *           wo   x fp16 [S][D], W [D][D], res [S][D] -> out32 [S][D]       w2    x fp16 [S][I], W [D][I], res -> out32 [S][D]
 *           w13  x fp32 [S][D], gamma, eps, W [2 I][D] ((w1_j, w3_j) rows interleaved) -> out16 [S][I]
 *           head x fp32 [S][D], gamma, eps, W [V][D] -> out32 [S][V]
 *   path 1  bgemm_launch, rows = B in 1 .. 64, Bp = B rounded up to 16 rows in x, res and the outputs; the same five roles (qkv:
 *           slots HOST [B], pos HOST [2][B], *nb = B, the cache table NULL above B; q_out rows >= B untouched)
 *   path 2  the B = 1 decode step's launches, rows ignored:
 *           qkv  dec_qkvraw: x fp32 [D], W [Nqkv][D] -> out32 [Nqkv]
 *           wo   dec_w2qkv:  x fp16 ff [I], res = h_mid [D], W2 = w2 [D][I], W = wc [Nqkv][I + D] -> out32 = h_out [D], out2 = qkv_raw [Nqkv]
 *           w13  dec_ffn13:  x fp32 h_in [D], part [H][D], gamma, eps, W [2 I][D] -> out2 = h_out [D], out16 = ff [I]
 *           w2   dec_w2:     x fp16 [I], W [D][I], res [D] -> out32 [D]     head  dec_head: x fp32 [D], gamma, eps, W [V][D] -> out32 [V]
 *   res may be the same buffer as out32 (the model runs wo and w2 in place).
 *   Refused (nothing allocated or launched): NULL args; path outside 0 .. 2; role outside 0 .. 4; D != 64 H; H < 1, Hkv < 1,
 *   H % Hkv != 0; D or I not a positive multiple of 64, or above 8192; V outside 1 .. 4096; path 0: rows outside 1 .. 8; path 1:
 *   rows outside 1 .. 64; path 2: D > 1024 or I > 2560 (svc_ar_create clears the decode step there); NULL x or W; a role's
 *   missing buffer (gamma, res, part, W2, out32, out16, out2); qkv on paths 0, 1: NULL q_out, kc, vc, rope, slots or pos, Lmax
 *   outside 8 .. 8192, n_slots outside 1 .. 64, a slot outside [0, n_slots) or named twice, a position outside [0, Lmax). */
typedef struct {
    int32_t path, role, D, I, H, Hkv, V, Lmax, rows, n_slots;
    const void* x;
    const float* gamma; float eps;
    const void* W; const void* W2;
    const float* res; const float* part;
    float* out32; void* out16; float* out2;
    float* q_out; float* kc; float* vc; const float* rope;
    const int32_t* slots; const int32_t* pos;
} svc_ar_linear_t;
int svc_op_ar_linear(const svc_ar_linear_t* args, void* stream);
/* y = rmsnorm(x) * gamma * (add_one + w) + b ; x [rows][D]. */
int svc_op_rmsnorm(const float* x, const float* gamma, const float* w, const float* b, int add_one, float* y,
                   int rows, int D, void* stream);
/* y = LayerNorm(x) * gamma + beta ; x, y [rows][D], D a multiple of 64 (at most 2048); mean, then the variance about it, in fp32. */
int svc_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream);

/* y = gelu(LayerNorm(x) * gamma + beta), erf form: the wav2vec 2.0 extractor's row kernel (one wave per row, two-pass statistics). */
int svc_op_layernorm_gelu(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream);

/* Tuning / measurement aid (tools/gemm_bench.py, tools/gemm_small_bench.py; no model uses it): times `iters` launches of the
 * tap-GEMM on synthetic operands of shape M x N x K; dtype 0 fp16 / 1 fp32, epi = epilogue kind, debug = tile-form override
 * bits; *out_ms = average launch time. */
int svc_op_gemm_bench(int M, int N, int K, int dtype, int epi, int iters, int debug, float* out_ms, void* stream);
/* Test aid: one fp16 tap-GEMM (epi: 0 store + bias + residual, 1 SwiGLU, 2 tanh-sigmoid, 3 QKV + RoPE + V^T) computed under
 * two tile-form overrides on the same pseudo-random operands; *n_diff = 32-bit output words that differ (every tile form keeps
 * the k order of each output element, so 0 is the contract). */
int svc_op_gemm_forms_diff(int M, int N, int K, int epi, int debug_a, int debug_b, long long* n_diff, void* stream);
/* Test aid (tests/test_gpu_kgemm.py; no model uses it): ONE kgemm_launch (csrc/kgemm.hip) on caller-supplied operands.  The call
 * checks every row the launch can address, packs A and W to the dtype (0 fp16, 1 fp32), launches once and synchronises; nothing
 * else runs between packing and readback.  Device pointers unless noted; NULL = absent.
 *   a_src[i]  fp32 [a_rows[i]][a_K[i]], i < n_src <= 4: the source buffers; packed to [a_rows][a_K rounded up to the k-tile] (zeros)
 *   taps      tap t < n_taps <= 48 reads source tap_src[t] at row shift tap_shift[t]; tap_K[t] must equal the source's K
 *   w         fp32 [w_rows][sum of tap_K]: w_rows = N rounded up to 256, the caller fills the rows at and above N (finite);
 *             packed tap by tap, each tap's K padded with zeros to the k-tile
 *   row map   m = s Lout + pos < M reads source row (a_seq_map ? a_seq_map[s] : s) a_seq_rows + a_off + pad(pos a_stride + shift)
 *             with pad over [0, seq_len ? seq_len[s] : a_len) by pad_mode / reflect_min as KGemmParams states; seq_len and
 *             a_seq_map are HOST arrays of ceil(M / Lout) entries.  Output row s c_seq_rows + c_off + pos.
 *   outputs   c32 fp32, c16 and c16_lo 16-bit words, res and res2 fp32: all [c_rows][ldc]; res / res2 may equal c32.
 *             vt [ceil(M / Lout)][rope_D][vt_ld] 16-bit words; rope fp32 [rope_rows][32][2].
 *   vectors   bias [N], rowvec / gate [nseq][ld] (ld 0: one row), post_a / post_ib [post_n]: sizes are the caller's to keep
 *   epi       KG_EPI_* 0 store, 1 SwiGLU, 2 tanh-sigmoid, 3 QKV + RoPE; form: launch_wide's tile-form bits (0 = its own choice)
 * Refused (nothing allocated or launched): NULL args, w or an output the epilogue needs; dtype outside 0 .. 1; n_src outside
 * 1 .. 4, n_taps outside 1 .. 48, a tap's source outside [0, n_src) or K other than its source's; M, N, Lout < 1, a_stride < 1,
 * pad_mode outside 0 .. 2; a sequence length < 0, or 0 under KG_PAD_CLAMP; an a_seq_map entry < 0; ANY (m, tap) whose source row
 * lies outside [0, a_rows) of its buffer; c_off < 0, c_off + Lout > c_seq_rows, nseq c_seq_rows > c_rows, ldc below the written
 * width; QKV: rope_rows < Lout, vt_ld < Lout rounded up to 32 or not a multiple of 4, vt_mode outside 0 .. 2; vec_ok or a
 * paired / QKV epilogue with N, ldc (a multiple of 8) or a pointer that breaks 16-byte access; form bits outside 0xF0; and
 * whatever kgemm_launch refuses.  check_only != 0: return 0 once every check has passed, before the first allocation (no device
 * is touched and no pointer is dereferenced, so the host tests can show an argument set to be acceptable without a GPU). */
typedef struct {
    int32_t dtype, epi, form;
    int32_t n_src;
    const float* a_src[4]; int64_t a_rows[4]; int32_t a_K[4];
    int32_t n_taps;
    int32_t tap_src[48]; int32_t tap_shift[48]; int32_t tap_K[48];
    const float* w; int64_t w_rows;
    int32_t M, N, Lout, a_seq_rows, a_off, a_stride, a_len, pad_mode, reflect_min;
    const int32_t* seq_len; const int32_t* a_seq_map;
    int32_t c_seq_rows, c_off;
    int64_t c_rows, ldc;
    float* c32; uint16_t* c16; uint16_t* c16_lo;
    const float* bias;
    const float* rowvec; int64_t ld_rowvec;
    const float* gate; int64_t ld_gate;
    const float* res; const float* res2;
    const float* post_a; const float* post_ib; int32_t post_n;
    float out_scale; int32_t act; float act_slope; int32_t post_relu, vec_ok;
    const float* rope; int32_t rope_rows, rope_D; float q_scale;
    uint16_t* vt; int64_t vt_ld; int32_t vt_mode;
    int32_t check_only;
} svc_kgemm_t;
int svc_op_kgemm(const svc_kgemm_t* args, void* stream);
/* Test aid (tests/test_gpu_kgemm.py; no model uses it): attention_permute_vt (csrc/attention.hip) on a caller's buffer: the in-place
 * column permutation of a natural-order V^T buffer [rows][vt_ld] (16-bit words, device) into order `mode` (vt_pos), as
 * svc_op_attention applies it; synchronises.  Refused: NULL vt, rows < 1, vt_ld < 32 or not a multiple of 32, mode outside 0 .. 2. */
int svc_op_permute_vt(uint16_t* vt, int64_t rows, int64_t vt_ld, int mode, void* stream);
/* Op-level seam of the split-precision (fp16x3) attention of the DiT's precision 2 (csrc/attention.hip, attn_x3): q, k, v, out are
 * DEVICE fp32 [n_seq][seq_rows][H][64], RoPE already applied to q and k; out = softmax(q k^T / 8 over keys < kv_len) v for the
 * query rows [q_start, Tq) of every sequence, other rows of out are not written.  kv_lens: HOST [n_seq], each in [0, seq_rows]
 * (0 writes zero rows).  The call scales q by log2(e) / 8 in fp32, splits q, k and v into hi / lo fp16 planes (V transposed, natural
 * column order) with the model's own kernels and issues ONE launch; synchronises.  Contracts: keys are walked in a fixed order
 * without atomics; a sequence's rows do not depend on the other sequences of the call (bit for bit); k and v rows at and above
 * kv_len are never used as values and may hold NaN.  Refused before anything is allocated: NULL pointers, n_seq, H or seq_rows < 1,
 * Tq outside [1, seq_rows], q_start outside [0, Tq), a length outside [0, seq_rows]. */
int svc_op_attention_x3(const float* q, const float* k, const float* v, float* out, int n_seq, int seq_rows, int H, int Tq,
                        int q_start, const int64_t* kv_lens, void* stream);
/* Test aid (tests/test_gpu_lr_ops.py; no model uses it): ONE launch of one of the length regulator's four kernels (csrc/lr.hip)
 * through the launch function svc_lr_forward calls, with the model's grid and block, on caller buffers; synchronises.  Device
 * pointers unless noted; NULL = absent.  Activations are channels-last rows of ld floats, utterance b at row b tout_max.
 *   stage 0 gather     x [B][tout_max][ld] (written whole) = row src of feat [B][tin_max][ld_feat] or of emb [.][C] at tokens
 *                      [B][tin_max] (int64; their values are device data and the caller's to keep inside the table), src =
 *                      interpolate ? min(floor(t (float)in_lens[b] / (float)ylens[b]), in_lens[b] - 1) : t; with f0_emb
 *                      [n_bins][C]: + f0_emb[bin(f0[b][nearest index over f0_lens[b]])] (f0 [B][tf0_max]), or + f0_mask [C]
 *                      when f0 is NULL; rows t >= ylens[b] and columns [C, ld) are zeros
 *   stage 1 gn_stats   stats [B][32][2] doubles: workgroup i's (sum, sum of squares) over rows [i rpb, min((i + 1) rpb, ylens[b]))
 *                      x C of x, rpb = ceil(ylens[b] / 32); zeros where it has no row
 *   stage 2 gn_mish    x = Mish(GroupNorm(x; the 32 partials of stats folded in index order, gamma [C], beta [C], eps)) in place;
 *                      rows t >= ylens[b] and columns [C, ld) become zeros
 *   stage 3 mask_copy  out [B][tout_max][ld_out] columns [0, N) = x [B][tout_max][ld] for t < ylens[b], else zeros
 * ylens, in_lens and f0_lens are HOST arrays of B entries.  Refused (nothing allocated or launched): NULL args, ylens or x; stage
 * outside 0 .. 3; B outside 1 .. 65535; tout_max < 1; ylens[b] outside [0, tout_max]; stages 0 .. 2: C < 1 or ld < C; stage 0: feat
 * and tokens both or neither, ld_feat < C, tokens without emb, tin_max < 1, NULL in_lens, in_lens[b] outside [1, tin_max],
 * ylens[b] > in_lens[b] without interpolate, f0 without f0_emb, n_bins < 2, f0_emb with neither f0 nor f0_mask, f0 with tf0_max < 1,
 * NULL f0_lens or f0_lens[b] outside [1, tf0_max]; stages 1 and 2: NULL stats; stage 2: NULL gamma or beta, eps <= 0; stage 3: NULL
 * out, N < 1, ld < N or ld_out < N.  check_only != 0: return 0 once every check has passed, before the first allocation. */
typedef struct {
    int32_t stage;
    int32_t B, tout_max, C, ld;
    const int32_t* ylens;
    float* x;
    const float* feat; int64_t ld_feat; int32_t tin_max;
    const int64_t* tokens; const float* emb;
    const int32_t* in_lens; int32_t interpolate;
    const float* f0; int32_t tf0_max; const int32_t* f0_lens;
    const float* f0_emb; const float* f0_mask; int32_t n_bins;
    double* stats;
    const float* gamma; const float* beta; float eps;
    float* out; int32_t ld_out, N;
    int32_t check_only;
} svc_lr_op_t;
int svc_op_lr(const svc_lr_op_t* args, void* stream);

/* Optional launch timing: HIP events around every tap-GEMM / attention launch on its stream.
 * svc_prof_collect fills out[cls*4 + {0..3}] = {launches, total ms, algorithmic flops, algorithmic bytes}
 * for the n_cls <= 4 classes 0 = fp16 tap-GEMM + resident-tile conv, 1 = fp32 tap-GEMM, 2 = attention, 3 = fused DiT
 * row-panel kernel, and clears the records. */
int svc_prof_enable(int on);
int svc_prof_collect(double* out, int n_cls);

const char* svc_last_error(void);
int svc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
