/* ta355.h -- C ABI of libta355.so: the MI355X-native (gfx950) projector-training hot path of
 * alexkroman/tiny-audio.  Plain pointers + sizes + a hipStream_t; no torch types; every function
 * returns an int status (0 = ok, 1 = bad argument, 2 = launch failure) and never allocates device
 * memory: callers pass workspaces sized by the matching *_workspace_bytes() query.  All pointers are
 * DEVICE pointers unless a comment says "host".  `long` is 64-bit (LP64).  bf16 buffers are passed as
 * `void*` (raw bfloat16 bits).
 *
 * The reference has no FFI of its own (it is 100 % Python on top of torch/transformers); the seams this
 * library sits behind are the reference's nn.Module boundaries.  Each entry point
 * names the reference interface it replaces; INTEGRATION.md shows the ctypes stubs a maintainer adds.
 */
#ifndef TA355_H
#define TA355_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define TA_OK 0
#define TA_ERR_ARG 1
#define TA_ERR_LAUNCH 2

int ta_version(void); /* ABI version, currently 4 (round 6: the residual-stream storage mode left process-wide state -- ta_set_stream_modes /
                          ta_get_stream_modes are gone, ta_encoder_weights.res_f32 and ta_lm_weights.res_f32 / dx_f32 carry it per handle; ta_rmsnorm_bwd_dyb is new;
                          ta_attention_fwd_qkv / ta_attention_bwd_qkv accept V = NULL.
                          Version 3 was round 5's: the opt-in paths that measured slower left the library -- ta_enc_layer lost its
                          wqk_il / *_ln image fields, ta_gemm_opts its swiglu_* / lnf_* fields, ta_layernorm_stats / ta_attention_bwd_gqa /
                          ta_attention_bwd_qkv_o went.  Version 2 was round 3's: ta_gemm_opts.rope_cols, ta_enc_layer.wqkv_fa / bqkv_fa,
                          ta_attention_enc_fwd, ta_logmel_f32's scratch contract) */

/* ---- storage dtype of the residual streams (the numerics contract of DESIGN.md section 6): a field of the weights handle
 * each call receives (ta_encoder_weights.res_f32; ta_lm_weights.res_f32 / dx_f32), so two models of different model_dtype -- or a
 * decoding thread beside a training step (tiny_audio/asr_modeling.py:733-734) -- share the library without sharing a mode.
 * The reference runs its frozen models either as bf16 MODULES (ASRConfig default model_dtype="bfloat16",
 * tiny_audio/asr_config.py:41: every residual add / norm input is bf16) or -- the training recipe of BASELINE configs[1] -- as
 * fp32 modules under bf16 autocast (configs/config.yaml:14-18 + configs/training/production.yaml:49; loaders
 * tiny_audio/asr_modeling.py:203-254: residual stream, norm in/out and embeddings stay fp32, only Linear / attention run in bf16).
 * 0 = bf16 storage (the first regime), 1 = fp32 storage (the second).
 * MFMA operand (bf16) and accumulator (fp32) types are the same in both; norms / softmax / CE arithmetic is fp32 in both.
 * A forward's tape must be read back by a backward whose handle carries the same res_f32 / dx_f32.  Workspace / tape sizes do not
 * depend on the mode (the fp32 size is always reserved). */

/* ============================================================================================
 * Composite ops (what a binding would call)
 * ============================================================================================ */

/* ---- log-mel features: replaces WhisperFeatureExtractor.__call__ as used at
 *      scripts/train.py:327-333 and tiny_audio/asr_processing.py:74-80
 *      (TF:models/whisper/feature_extraction_whisper.py:135-168,330-339).
 * wav [B, Ls] f32 zero-padded to the longest clip, lens [B] true sample counts.
 * dft [400, 402] / window [400] / melfb [201, n_mels] are host-built constant tables uploaded once (of dft the kernel reads row
 *      n = 1, the twiddles W400^j of its 16 x 25 mixed-radix FFT).
 * feats [B, n_mels, T] f32, mask [B, T] int32, T = Ls / 160.
 * scratch: float[ta_logmel_scratch_floats(B, Ls, n_mels)] -- every persistent workgroup records the maximum of its tiles per clip
 *      there (plain stores; no initial contents required, no atomics) and the second launch reduces them into the (max - 8) floor.
 *      (ABI 2: int[2 * B] behind an init launch, one device-scope atomicMax per workgroup.)
 * mel_ranges: int[2 * n_mels] {first, end} frequency bin of every mel filter, from ta_logmel_mel_ranges -- a function of the
 *      filter bank alone, computed once when the tables are uploaded. */
long ta_logmel_scratch_floats(int B, int Ls, int n_mels);
int ta_logmel_mel_ranges(const float* melfb, int n_mels, int* mel_ranges, hipStream_t st);
int ta_logmel_f32(const float* wav, const long* lens, int B, int Ls, const float* dft, const float* window,
                  const float* melfb, int n_mels, float* feats, int* mask, float* scratch, const int* mel_ranges, hipStream_t st);

/* ---- frozen GLM-ASR encoder: replaces model.audio_tower(input_features=...).last_hidden_state
 *      (tiny_audio/asr_modeling.py:448-450; TF:models/glmasr/modeling_glmasr.py:313-327). */
typedef struct {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b; /* [H] */
  const void* wqkv;   /* bf16 [3H, H] rows = q | k | v */
  const float* bqkv;  /* [3H] (k part zero: k_proj has no bias) */
  const void* wo;     /* bf16 [H, H] */
  const float* bo;
  const void* w1;     /* bf16 [F, H] */
  const float* b1;
  const void* w2;     /* bf16 [H, F] */
  const float* b2;
  /* Optional (both NULL = the three-kernel path: q|k|v GEMM + ta_enc_qkv_post + ta_attention_fwd): the image of the
   * ta_attention_enc_fwd path.
   *   wqkv_fa bf16 [3H, H]: the q rows and k rows with every head's rows reordered for ta_gemm_opts.rope_tab (row 2i = head dim i,
   *           row 2i+1 = head dim i+16 for i < 16, rows 32..63 unchanged), the q rows MULTIPLIED by head_dim^-0.5 * log2(e) (the
   *           softmax then runs in base 2 with no per-score multiply), then the v rows as they are;
   *   bqkv_fa [3H] likewise (q part scaled, k part zero, v part = v_proj.bias).
   * q | k | v then come out of ONE GEMM (rope on the first 2H columns: ta_gemm_opts.rope_cols) as a token-major [M, 3H]
   * buffer that the attention kernel reads in place -- no V^T image, no M % 8 restriction. */
  const void* wqkv_fa;
  const float* bqkv_fa;
} ta_enc_layer;

typedef struct {
  int hidden, ffn, n_layers, heads, n_mels, max_pos;
  float ln_eps;
  const void* conv1_w;  /* bf16 [H, 3*n_mels], column = tap*n_mels + cin */
  const float* conv1_b;
  const void* conv2_w;  /* bf16 [H, 3*H], column = tap*H + cin */
  const float* conv2_b;
  const float *norm_w, *norm_b;
  const float *rope_cos, *rope_sin; /* [max_pos, 16] (partial rotary: 32 of 64 dims) */
  const ta_enc_layer* layers;       /* host array [n_layers] */
  const float* rope_il;             /* [max_pos, 16, 2] (cos, sin) interleaved, or NULL (see ta_enc_layer.wqkv_fa) */
  int res_f32;                      /* storage of the residual stream: 0 = bf16, 1 = fp32 (see the top of this file) */
} ta_encoder_weights;

long ta_encoder_workspace_bytes(const ta_encoder_weights* w, int B, int T);
/* feats [B, n_mels, T] f32 -> out_bf16 [B*S, H] (and/or out_f32), S = (T-1)/2+1.
 * frame_keep [B*S] f32 or NULL: the train-time whole-frame dropout mask of
 * ASRModel._maybe_drop_audio_tokens (tiny_audio/asr_modeling.py:458-479), fused into the final LayerNorm. */
int ta_encoder_forward(const ta_encoder_weights* w, const float* feats, int B, int T, const float* frame_keep,
                       void* out_bf16, float* out_f32, void* ws, long ws_bytes, hipStream_t st);

/* ---- the same tower with every clip encoded at its OWN length (the "ragged encoder"; opt-in, GLM-ASR only): replaces
 *      model.audio_tower(input_features=feats[b:b+1, :, :T_b]).last_hidden_state for every clip b of the batch -- what the reference
 *      computes at inference, where the feature extractor's padding is off and a clip is encoded alone
 *      (tiny_audio/asr_modeling.py:198-200) -- instead of the training-time call on the padded batch (:448-450), whose encoder has
 *      no attention mask (TF:models/glmasr/modeling_glmasr.py:187-217), so that a short clip's frames depend on its neighbours' lengths.
 * mel_len_host: HOST int [B], the clips' mel lengths T_b (audio_attention_mask.sum(-1)), 1 <= T_b <= T; they set the launch geometry.
 * cu_rows_dev:   DEVICE int [B + 1], cu[0] = 0, cu[b + 1] = cu[b] + S_b with S_b = (T_b - 1) / 2 + 1, built by the caller from the
 *               same lengths.  The host cannot read it, so a table that disagrees with mel_len_host is not detected: the copy kernels
 *               (compaction, rotary table, expansion) skip the rows it places outside the workspace, but the attention kernel
 *               TRUSTS it and reads and writes rows cu[b] .. cu[b + 1] unchecked.
 * Output rows [b, 0:S_b) = the encoder applied to feats[b, :, :T_b] alone (the stem's zero padding at the clip's own end, rotary
 * positions 0 .. S_b - 1, attention over the clip's own frames); rows [b, S_b:S) and the frames with frame_keep == 0 are exact
 * zeros; out_bf16 / out_f32 keep ta_encoder_forward's padded [B*S, H] layout.  feats[b, :, T_b:] is never read.
 * Internally the layer loop runs on rows = sum of S_b compact rows.  Needs ta_enc_layer.wqkv_fa / bqkv_fa and rope_il (TA_ERR_ARG
 * without them: the three-kernel path is not extended).  Kernel launches on st only: no allocation, copy or synchronisation. */
long ta_encoder_ragged_workspace_bytes(const ta_encoder_weights* w, int B, int T, long rows);
int ta_encoder_forward_ragged(const ta_encoder_weights* w, const float* feats, int B, int T, const int* mel_len_host,
                              const int* cu_rows_dev, const float* frame_keep, void* out_bf16, float* out_f32, void* ws,
                              long ws_bytes, hipStream_t st);

/* ---- frozen Whisper encoder (any openai/whisper-* checkpoint; the reference's other audio_tower, tiny_audio/asr_modeling.py:203-237):
 *      replaces WhisperEncoder.forward(input_features).last_hidden_state (TF:models/whisper/modeling_whisper.py:592-650).
 * The stem, the layer arithmetic (TF:models/whisper/modeling_whisper.py:379-407: pre-LN, q/v/out bias, k without, exact GELU,
 * scale head_dim^-0.5, no mask) and the final LayerNorm are the GLM-ASR tower's, so ta_enc_layer is reused unchanged with
 *   ln1_* = self_attn_layer_norm, ln2_* = final_layer_norm, wo/bo = self_attn.out_proj, w1/b1 = fc1, w2/b2 = fc2, and
 *   wqkv_fa / bqkv_fa (REQUIRED here) = q | k | v rows in their natural order -- no rotary row interleave -- with the q rows and
 *   the q bias multiplied by head_dim^-0.5 * log2(e), the k part of the bias zero.  wqkv / bqkv are not read.
 * What differs: no rotary embedding anywhere; instead pos_emb (embed_positions.weight) is added once to the stem's output
 * (TF:models/whisper/modeling_whisper.py:622-624), and the input must span exactly 2 * max_pos frames (:612-616). */
typedef struct {
  int hidden, ffn, n_layers, heads, n_mels, max_pos;   /* head_dim = hidden / heads must be 64; hidden, ffn multiples of 128; n_mels of 8 */
  float ln_eps;
  const void* conv1_w;  /* bf16 [H, K1], K1 = 3*n_mels rounded up to a multiple of 64 (256 at 80 bins); column = tap*n_mels + cin,
                           columns 3*n_mels..K1-1 ZERO (the rows of the time-major input overlap: those columns meet the next frame) */
  const float* conv1_b;
  const void* conv2_w;  /* bf16 [H, 3*H], column = tap*H + cin */
  const float* conv2_b;
  const float* pos_emb; /* f32 [max_pos, H] = embed_positions.weight */
  const float *norm_w, *norm_b;     /* layer_norm */
  const ta_enc_layer* layers;       /* host array [n_layers] */
  int res_f32;                      /* storage of the residual stream: 0 = bf16, 1 = fp32 (see the top of this file) */
} ta_whisper_encoder_weights;

long ta_whisper_encoder_workspace_bytes(const ta_whisper_encoder_weights* w, int B, int T);
/* feats [B, n_mels, T] f32, T == 2 * max_pos (else TA_ERR_ARG) -> out_bf16 [B*S, H] (and/or out_f32), S = max_pos.
 * frame_keep [B*S] f32 or NULL: as ta_encoder_forward (fused into the final LayerNorm). */
int ta_whisper_encoder_forward(const ta_whisper_encoder_weights* w, const float* feats, int B, int T, const float* frame_keep,
                               void* out_bf16, float* out_f32, void* ws, long ws_bytes, hipStream_t st);

/* ---- MLP projector: replaces MLPAudioProjector.forward + its autograd backward
 *      (tiny_audio/projectors.py:57-71,79-87). x bf16 [B, S, E] -> y f32 [B*N, D], N = (S-k)/k+1. */
typedef struct {
  int enc_dim, k, hidden, llm_dim;
  float eps;
  const void* w1;   /* bf16 [Hd, k*E]   (cast of linear_1.weight) */
  const void* w2;   /* bf16 [D, Hd]     (cast of linear_2.weight) */
  const void* w2_t; /* bf16 [Hd, D]     (transposed cast, for dA = dH2 W2) */
  const float* g1;  /* norm.weight   [Hd] */
  const float* g2;  /* norm_2.weight [D]  */
} ta_mlp_weights;

long ta_mlp_tape_bytes(const ta_mlp_weights* w, int B, int S);
long ta_mlp_bwd_workspace_bytes(const ta_mlp_weights* w, int B, int S);
int ta_mlp_projector_forward(const ta_mlp_weights* w, const void* x_bf16, int B, int S, float* y, void* tape,
                             hipStream_t st);
/* dy f32 [B*N, D] -> dW1 [Hd,kE], dg1 [Hd], dW2 [D,Hd], dg2 [D] (f32, overwritten). */
int ta_mlp_projector_backward(const ta_mlp_weights* w, const void* x_bf16, int B, int S, const float* dy,
                              const void* tape, float* dW1, float* dg1, float* dW2, float* dg2, void* ws,
                              long ws_bytes, hipStream_t st);

/* ---- shared + sparse MoE projector: replaces MoEAudioProjector.forward/_forward_sparse + autograd backward
 *      (tiny_audio/projectors.py:185-351): frame-stack -> RMSNorm(kE) -> shared SimpleAdapter + top-2-of-E routed
 *      SimpleAdapters (fc1+bias -> erf-GELU -> fc2+bias), fp32 softmax router with optional multiplicative jitter,
 *      balance + z auxiliary loss.  Arrays w1.. hold E+1 device pointers (HOST arrays): routed experts 0..E-1, then
 *      the shared expert at index E. */
typedef struct {
  int enc_dim, k, hidden, llm_dim, num_experts;
  float eps, aux_coef, z_coef;
  const float* norm_w;       /* [k*E_enc] */
  const float* router_w;     /* f32 [E, k*E_enc] */
  const void* const* w1;     /* bf16 [Hd, kE] */
  const void* const* w1_t;   /* bf16 [kE, Hd] */
  const float* const* b1;    /* [Hd] */
  const void* const* w2;     /* bf16 [D, Hd] */
  const void* const* w2_t;   /* bf16 [Hd, D] */
  const float* const* b2;    /* [D] */
} ta_moe_weights;

/* bf16 images of all n = E + 1 adapters (routed experts, then the shared one) in two launches: f32 masters w1[i] [H, In], w2[i] [D, H],
 * b1[i] [H], b2[i] [D] (host arrays of device pointers) -> stacked W1a [n, H, In], W1ta [n, In, H], W2a [n, D, H], W2ta [n, H, D]
 * (bf16) and B1a [n, H], B2a [n, D] (f32): what ta_moe_weights points into (tiny_audio/projectors.py:257-283 keeps one nn.Linear
 * pair per expert). */
int ta_moe_pack_images(const float* const* w1, const float* const* b1, const float* const* w2, const float* const* b2, int n, int H, int In,
                       int D, void* W1a, void* W1ta, void* W2a, void* W2ta, float* B1a, float* B2a, hipStream_t st);
long ta_moe_tape_bytes(const ta_moe_weights* w, int B, int S);
long ta_moe_bwd_workspace_bytes(const ta_moe_weights* w, int B, int S);
/* noise: [T, E] jitter factors (train mode; the reference draws U(1-0.01, 1+0.01)) or NULL; aux: device scalar out. */
int ta_moe_projector_forward(const ta_moe_weights* w, const void* x_bf16, int B, int S, const float* noise, int training,
                             float* y, float* aux, void* tape, hipStream_t st);
/* gradients of sum(dy * y) + d_aux * aux; dW1/db1/dW2/db2 are HOST arrays of E+1 device pointers (overwritten). */
int ta_moe_projector_backward(const ta_moe_weights* w, const void* x_bf16, int B, int S, const float* dy, float d_aux,
                              const float* noise, int training, const void* tape, float* d_norm_w, float* d_router_w,
                              float* const* dW1, float* const* db1, float* const* dW2, float* const* db2, void* ws,
                              long ws_bytes, hipStream_t st);
/* The same with the upstream gradient of the auxiliary loss read from DEVICE memory (d_aux_dev: one f32): the autograd
 * engine hands it over as a device scalar, and reading it on the host would stall the launch queue once per step. */
int ta_moe_projector_backward_dev(const ta_moe_weights* w, const void* x_bf16, int B, int S, const float* dy,
                                  const float* d_aux_dev, const float* noise, int training, const void* tape,
                                  float* d_norm_w, float* d_router_w, float* const* dW1, float* const* db1,
                                  float* const* dW2, float* const* db2, void* ws, long ws_bytes, hipStream_t st);

/* round 4: the share of d(norm.weight) [k * enc_dim] and d(router.weight) [E, k * enc_dim] that comes from the auxiliary losses alone
 * (d_aux * d aux / d .; overwritten).  Same tape / workspace as the backward.  The trainer keeps it in a shadow of its flat gradient
 * buffer so that the auxiliary term keeps its full weight under the optimizer's division by the global label-token count without a
 * second collective (tiny_audio_amd/trainer.py). */
int ta_moe_router_aux_grads(const ta_moe_weights* w, const void* x_bf16, int B, int S, const float* d_aux_dev, const float* noise,
                            int training, const void* tape, float* d_norm_w_aux, float* d_router_w_aux, void* ws, long ws_bytes,
                            hipStream_t st);

/* ---- frozen causal LM (Qwen3; SmolLM3 / Llama with head_dim 128) + shifted CE: replaces model.language_model(inputs_embeds=, attention_mask=, labels=)
 *      together with the embed/masked_scatter glue of ASRModel.forward
 *      (tiny_audio/asr_modeling.py:497-526; TF:models/qwen3/modeling_qwen3.py:367-508; TF:loss/loss_utils.py:33-71)
 *      and its activation-gradient backward (encoder + LM frozen: dX only). */
typedef struct {
  const float* ln_in_w;             /* [D] */
  const void *wqkv, *wqkv_t;        /* bf16 [NQKV, D], [D, NQKV]; rows = q | k | v */
  const float *qn_w, *kn_w;         /* [head_dim] q_norm / k_norm (Qwen3), or BOTH NULL: a decoder without q/k-norm (SmolLM3, Llama:
                                       TF:models/smollm3/modeling_smollm3.py:174-250) -- q and k go to RoPE unscaled.  One set, one not: TA_ERR_ARG */
  const void *wo, *wo_t;            /* bf16 [D, Hq*hd], [Hq*hd, D] */
  const float* ln_post_w;           /* [D] */
  const void *wgu, *wgu_t;          /* bf16 [2F, D] rows = gate | up, [D, 2F] */
  const void *wd, *wd_t;            /* bf16 [D, F], [F, D] */
  /* LoRA adapters (stage 2, tiny_audio/asr_modeling.py:289-301; all NULL when disabled): fp32 MASTERS, the peft
   * tensors of the linears that share an input stacked on rows, group g in {qkv, o, gate|up, down}:
   *   la_g [members*r, in_g] = concat of lora_A_j [r, in];   lb_g [N_g, r] = concat of lora_B_j [out_j, r]. */
  const float *la_qkv, *lb_qkv, *la_o, *lb_o, *la_gu, *lb_gu, *la_d, *lb_d;
} ta_lm_layer;

/* gradients of the LoRA masters of one layer (same layouts; written, not accumulated) */
typedef struct {
  float *dla_qkv, *dlb_qkv, *dla_o, *dlb_o, *dla_gu, *dlb_gu, *dla_d, *dlb_d;
} ta_lm_lora_grads;

typedef struct {
  int vocab, vocab_pad, hidden, ffn, n_layers, heads, kv_heads, head_dim, max_pos;
  float eps;
  const float* embed_f32;   /* [vocab, D]   input embedding (fp32 master, as the reference looks it up) */
  const void* embed_bf16;   /* [vocab_pad, D] tied lm_head, rows >= vocab zero */
  const void* embed_t_bf16; /* [D, vocab_pad] */
  const float* norm_w;
  const float *rope_cos, *rope_sin; /* [max_pos, head_dim/2] */
  const ta_lm_layer* layers;        /* host array */
  int lora_rank;                    /* 0 = no adapters; else r with 3 r <= 64 (the reference default 8; 4 and 16 are tested) */
  float lora_scale;                 /* alpha / r */
  int train_base;                   /* 1 = full decoder fine-tuning (freeze_language_model=False, tiny_audio/asr_config.py:77,
                                       configs/experiments/embedded.yaml:23): the tape also keeps what ta_lm_wgrads needs */
  int lora_groups;                  /* lora_target_modules subsets (tiny_audio/asr_config.py:72-75): bit g set = group g of
                                       {1 q|k|v, 2 o, 4 gate|up, 8 down} carries an adapter; 0 = all four.  A group without
                                       a bit costs nothing (no rank-space GEMM, no K extension, gradients left at zero); inside
                                       a group, members that are not targeted keep A = B = 0 in the masters and so get exactly
                                       zero gradients (dA = s (dy B)^T x, dB = dy^T (x A^T)). */
  int res_f32;                      /* storage of the forward residual stream and of its rows in the tape: 0 = bf16, 1 = fp32 */
  int dx_f32;                       /* storage of the backward d(x) stream: 0 = follows res_f32, 1 = fp32 even over a bf16 forward
                                       stream (rounds 1-3) */
  unsigned long long nope_layers;   /* bit l set = decoder layer l applies NO rotary embedding ("NoPE": SmolLM3's no_rope_layers[l] == 0,
                                       TF:models/smollm3/configuration_smollm3.py; use_rope at TF:models/smollm3/modeling_smollm3.py:174-250):
                                       q and k skip the rotation and its table loads in training, prefill and both decode steps, and the
                                       K rows of the cache are the unrotated ones.  0 = every layer rotates (Qwen3, Llama).  A set bit
                                       needs n_layers <= 64.  Appended in ABI 4: handles are ZERO-INITIALISED by the caller (ctypes
                                       structures and `= {}` are), so a caller that never names the field runs Qwen3's arithmetic. */
} ta_lm_weights;

/* Gradients of the LM's own weights (full decoder fine-tuning).  All f32, ACCUMULATED (+=) into the caller's buffers, which
 * the caller zeroes at the start of an optimizer step (gradient accumulation over micro-batches then needs nothing else).
 * dembed [vocab, D] receives both shares of the tied matrix: lm_head (dlogits^T h) and the input lookup (scatter-add of
 * d inputs_embeds at the text positions; <audio> rows were overwritten by the projector output and get none). */
typedef struct {
  float *dwqkv;  /* [NQKV, D] rows = q | k | v */
  float *dwo;    /* [D, heads*head_dim] */
  float *dwgu;   /* [2F, D] rows = gate | up */
  float *dwd;    /* [D, F] */
  float *dln_in, *dln_post;   /* [D] */
  float *dqn, *dkn;           /* [head_dim] */
} ta_lm_layer_wgrads;
typedef struct {
  const ta_lm_layer_wgrads* layers;   /* host array [n_layers] */
  float* dnorm;                       /* [D] */
  float* dembed;                      /* [vocab, D] */
} ta_lm_wgrads;

long ta_lm_tape_bytes(const ta_lm_weights* w, int B, int L, int n_label_rows);
long ta_lm_workspace_bytes(const ta_lm_weights* w, int B, int L, int n_label_rows);
/* ids [B,L] i64; src_row [B*L] from ta_audio_index (or NULL = text only); audio f32 [*, D] projector output;
 * kmask [B,L] int32 attention mask (NULL = all ones); pos [B*L] int32 (NULL = arange(L));
 * label_rows/label_targets: the n_label_rows positions whose shifted label != -100 (ta_label_rows);
 * loss_scale = 1 / num_items_in_batch.  loss: device scalar, ACCUMULATED into (zero it first).
 * logits_out: optional [B*L, vocab_pad] bf16 full logits (the reference's outputs.logits), else NULL. */
int ta_lm_forward_loss(const ta_lm_weights* w, const long* ids, const int* src_row, const float* audio,
                       const int* kmask, const int* pos, int B, int L, const int* label_rows,
                       const long* label_targets, int n_label_rows, float loss_scale, float* loss,
                       float* nll_rows, void* logits_out, void* tape, void* ws, long ws_bytes, hipStream_t st);
/* ---- primitives of the trainable transformer-style projectors (QFormer / MOSA, SURVEY.md section 8(f) rank 4;
 * tiny_audio/projectors.py:88-182,359-475 over TF:models/blip_2/modeling_blip_2.py Blip2QFormer*).  The linears are
 * ta_gemm_bf16_nt; these are the pieces around them. */
int ta_gelu_fwd(const void* h_bf16, void* a_bf16, long n, hipStream_t st);                     /* nn.GELU (erf) */
int ta_gelu_bwd(const void* da_bf16, const void* h_bf16, void* dh_bf16, long n, hipStream_t st);
int ta_colsum(const void* x, int is_f32, int R, int C, float* out, hipStream_t st);           /* out[c] = sum_r x[r,c]: bias grads */
int ta_relu_fwd(const void* h_bf16, void* a_bf16, long n, hipStream_t st);                     /* MOSA router (projectors.py:136-140) */
int ta_relu_bwd(const void* da_bf16, const void* h_bf16, void* dh_bf16, long n, hipStream_t st);
/* MOSA dense mixture (projectors.py:158-166): rw = softmax(logits [M,E]); out = sum_e rw[:,e] * o[e] with o f32 [E, M, D].
 * Backward: do_bf16 [E, M, D] = dout * rw[:,e]; dlogits [M,E] = softmax backward of drw[e] = <dout, o[e]>. */
int ta_mix_fwd(const float* logits, const float* o, float* rw, float* out, int M, int D, int E, hipStream_t st);
int ta_mix_bwd(const float* dout, const float* o, const float* rw, void* do_bf16, float* dlogits, int M, int D, int E,
               hipStream_t st);
/* y = LayerNorm(z * keep + res[row % res_rows]) (keep: dropout mask already divided by 1-p, or NULL; res optional);
 * saves xhat [M,H] and rstd [M] for ta_layernorm_bwd.  Blip2QFormerSelfOutput / Output: dense -> dropout -> +res -> LN. */
int ta_layernorm_res_fwd(const float* z, const float* keep, const float* res, long res_rows, const float* gamma,
                         const float* beta, float eps, float* xhat, float* rstd, float* y_f32, void* y_bf16, int M, int H,
                         hipStream_t st);
/* du (f32, gradient of the LN input = residual branch) and dz = du * keep (bf16, dense branch) are optional;
 * dgamma / dbeta are ACCUMULATED. */
int ta_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* keep, float* du,
                     void* dz_bf16, float* dgamma, float* dbeta, int M, int H, hipStream_t st);
/* Windowed multi-head attention (Blip2QFormerMultiHeadAttention, eager): EB windows, Q bf16 [EB*Lq, heads*hd],
 * K / V bf16 [EB*Lk, heads*hd]; P f32 [EB, heads, Lq, Lk] = softmax probabilities (saved); keep = attention-probs
 * dropout mask / (1-p) or NULL; O bf16 [EB*Lq, heads*hd]. */
int ta_attn_small_fwd(const void* Q, const void* K, const void* V, int EB, int heads, int hd, int Lq, int Lk, float scale,
                      const float* keep, float* P, void* O, hipStream_t st);
int ta_attn_small_bwd(const void* dO, const void* Q, const void* K, const void* V, const float* P, const float* keep,
                      float scale, void* dQ, void* dK, void* dV, int EB, int heads, int hd, int Lq, int Lk, hipStream_t st);

/* ---- greedy decoding: ASRModel.generate, tiny_audio/asr_modeling.py:562-646, which
 * drives HF GenerationMixin greedy search (num_beams 1, do_sample False: tiny_audio/asr_config.py:103-111) with a KV cache.
 * kcache / vcache: bf16 [n_layers, B, kv_heads, Lmax, head_dim], owned by the caller.  lora_img: scratch of
 * ta_lm_lora_image_bytes() bytes holding the bf16 adapter images between the prompt pass and the decode steps (NULL
 * without adapters).
 * ta_lm_prefill: the prompt pass over [B, L] rows (same inputs as ta_lm_forward_loss); fills cache slots [0, L) and
 * returns logits f32 [B, vocab_pad] of row last_rows[b] (= b*L + index of clip b's last prompt token). */
long ta_lm_prefill_workspace_bytes(const ta_lm_weights* w, int B, int L);
long ta_lm_lora_image_bytes(const ta_lm_weights* w);
int ta_lm_prefill(const ta_lm_weights* w, const long* ids, const int* src_row, const float* audio, const int* kmask,
                  const int* pos, int B, int L, void* kcache, void* vcache, int Lmax, const int* last_rows, float* logits,
                  void* lora_img, void* ws, long ws_bytes, hipStream_t st);
/* One decode step: ids [B] = the tokens emitted last, at RoPE position pos[b]; their K/V go to cache slot *slot_dev;
 * kmask [B, Lmax] marks the valid slots (including *slot_dev); logits f32 [B, vocab_pad] of the next token.  Every
 * per-step quantity is read from device memory, so the launch sequence is step-invariant (hipGraph-capturable). */
long ta_lm_decode_workspace_bytes(const ta_lm_weights* w, int B);
int ta_lm_decode_step(const ta_lm_weights* w, const long* ids, const int* pos, const int* kmask, const int* slot_dev, int B,
                      void* kcache, void* vcache, int Lmax, float* logits, const void* lora_img, void* ws, long ws_bytes,
                      hipStream_t st);
/* out[r] = argmax over the first n columns of row r (lowest index on ties) */
int ta_argmax_f32(const float* x, long ld, int n, int rows, long* out, hipStream_t st);
/* HF greedy bookkeeping for step t = *step_dev (TF:generation/utils.py _sample): finished clips emit pad_id, a clip
 * finishes on any eos id; writes out_seq[b, t], next_ids[b]; advances pos / *slot_dev / kmask for the next decode step
 * (not on t == 0, whose token comes from the prompt pass); *step_dev += 1; *n_unfinished = clips still running. */
/* The reference's non-default greedy settings (tiny_audio/asr_config.py:84-86,155-160; TF:generation/logits_process.py
 * RepetitionPenaltyLogitsProcessor + NoRepeatNGramLogitsProcessor) on the step's logits [B, ld] f32 (V valid columns) BEFORE
 * ta_argmax_f32.  The processors see prompt_ids [B, L] i64 followed by the first *step_dev tokens of out_seq [B, max_new]
 * (the reference passes input_ids to generate for exactly this: tiny_audio/asr_modeling.py:625-633).  repetition_penalty 1.0 and
 * no_repeat_ngram_size 0 make it a no-op; L + max_new <= 8192. */
int ta_logits_process(float* logits, long ld, int V, const long* prompt_ids, int L, const long* out_seq, int max_new,
                      const int* step_dev, int B, float repetition_penalty, int no_repeat_ngram_size, hipStream_t st);
/* Sampling (generation_config.do_sample / temperature / top_k / top_p: tiny_audio/asr_config.py:78-81, forwarded to HF at
 * tiny_audio/asr_modeling.py:631-637).  ta_logits_warp applies HF's warpers in HF's order, in place on logits f32 [B, ld] (columns
 * < V): TemperatureLogitsWarper (scores / T), TopKLogitsWarper (below the k-th largest -> -inf; 0 = off), TopPLogitsWarper (ascending
 * cumulative probability <= 1 - top_p -> -inf, the largest always kept; 1 = off).  ta_sample_f32 draws out[b] ~ softmax(logits[b, :V])
 * with a Philox4x32-10 uniform keyed by (seed, *step_dev, b): reproducible per seed, independent of launch geometry.  Call both
 * between the logits processors and ta_greedy_advance (ta_sample_f32 takes the place of ta_argmax_f32). */
int ta_logits_warp(float* logits, long ld, int V, int B, float temperature, int top_k, float top_p, hipStream_t st);
int ta_sample_f32(const float* logits, long ld, int V, int B, unsigned long long seed, const int* step_dev, long* out, hipStream_t st);
/* HF MinNewTokensLengthLogitsProcessor (generation_config.min_new_tokens: tiny_audio/asr_config.py:83, forwarded to
 * language_model.generate at tiny_audio/asr_modeling.py:631-637): while *step_dev (tokens generated so far, device memory) is below
 * min_new, logits[b, ids[e]] = -inf for every eos id.  Call between ta_logits_process and ta_argmax_f32. */
int ta_logits_suppress_until(float* logits, long ld, int V, const long* ids, int n_ids, int min_new, const int* step_dev, int B,
                             hipStream_t st);
/* ---- Decoding options: HF's remaining single-hypothesis logits processors (TF:generation/logits_process.py; the reference forwards
 * **generate_kwargs to language_model.generate, tiny_audio/asr_modeling.py:625-637, :723-729).  All three work in place on the step's
 * logits f32 [B, ld] (V valid columns; columns >= V are never read or written), read the step from *step_dev (tokens generated so far)
 * and take tables that live in device memory, so their launch arguments are step-invariant (hipGraph-capturable).  HF's order
 * (TF:generation/utils.py _get_logits_processor): ta_logits_sequence_bias (sequence_bias) -> ta_logits_process ->
 * ta_logits_sequence_bias (bad_words_ids) -> ta_logits_suppress_until -> ta_logits_step_rules -> ta_logits_warp -> ta_logits_warp_ext.
 *
 * ta_logits_sequence_bias: SequenceBiasLogitsProcessor; NoBadWordsLogitsProcessor is the same with every bias -inf.  The context of row
 * b is prompt_ids[b, :L] followed by the first *step_dev tokens of out_seq[b] (L = 0: the generated tokens only).  A length-1 sequence
 * always adds its bias to its token; a longer one adds it to its last token iff it is not longer than the context and its first len-1
 * tokens equal the last len-1 tokens of the context.  The table: seq_tokens i64 [n_tokens] (the sequences, flattened), seq_offsets i32
 * [n_seq + 1], seq_bias f32 [n_seq], SORTED by last token with group_starts i32 [n_groups + 1] delimiting the runs of equal last token
 * (distinct between groups).  One lane owns a group and adds its matching biases in table order to 0, then the sum to the score: no
 * float atomics, HF's f32 result bit for bit when a group lists its length-1 entry first and then HF's order (ops.build_sequence_table).
 * n_seq <= TA_SEQ_BIAS_MAX_SEQS, every sequence <= TA_SEQ_BIAS_MAX_LEN tokens (n_tokens <= n_seq * TA_SEQ_BIAS_MAX_LEN), else TA_ERR_ARG. */
#define TA_SEQ_BIAS_MAX_SEQS 4096
#define TA_SEQ_BIAS_MAX_LEN 32
int ta_logits_sequence_bias(float* logits, long ld, int V, const long* prompt_ids, int L, const long* out_seq, int max_new,
                            const int* step_dev, int B, const long* seq_tokens, const int* seq_offsets, const float* seq_bias,
                            const int* group_starts, int n_seq, int n_groups, int n_tokens, hipStream_t st);
/* ta_logits_step_rules: the four processors that depend on t = *step_dev only, in HF's order, one launch; any subset may be absent
 * (count 0 / NULL):
 *   ForcedEOSTokenLogitsProcessor          at t == max_new - 1 the row becomes -inf and forced_eos_ids [n_forced] become 0;
 *   ExponentialDecayLengthPenalty          for t > decay_start: score[e] += |score[e]| * decay_mult[t] for every id e of eos_ids [n_eos]
 *                                          (decay_mult f32 [max_new] = f32(factor ** (t - decay_start) - 1), computed on the host exactly
 *                                          as HF's Python does; NULL = off; one rounded multiply, one rounded add, no pow on the device);
 *   SuppressTokensLogitsProcessor          suppress_ids [n_suppress] -> -inf at every step;
 *   SuppressTokensAtBeginLogitsProcessor   begin_suppress_ids [n_begin] -> -inf at t == 0.
 * The prompt length cancels out of all four HF conditions. */
int ta_logits_step_rules(float* logits, long ld, int V, int B, const int* step_dev, int max_new, const long* forced_eos_ids,
                         int n_forced, const long* eos_ids, int n_eos, int decay_start, const float* decay_mult,
                         const long* suppress_ids, int n_suppress, const long* begin_suppress_ids, int n_begin, hipStream_t st);
/* ta_logits_warp_ext: the warpers ta_logits_warp lacks, after it, in HF's order, each on the row its predecessor left
 * (min_tokens_to_keep = 1):
 *   MinPLogitsWarper (min_p in [0, 1], 0 = off)          remove p < min_p * max p;
 *   TypicalLogitsWarper (typical_p in (0, 1], 1 = off)   s_i = |-log p_i - H|; keep s_i <= s_cut, the shifted score at which the
 *                                                        cumulative probability in ascending s first reaches typical_p (ties with s_cut
 *                                                        all survive; like HF this can remove the row maximum);
 *   EpsilonLogitsWarper (epsilon_cutoff in [0, 1), 0 = off)   remove p < eps, never the row maximum;
 *   EtaLogitsWarper (eta_cutoff in [0, 1), 0 = off)           remove p < min(eps, sqrt(eps) exp(-H)), never the row maximum.
 * Removed entries become -inf, survivors keep their value.  One 1024-lane workgroup per row; s_cut by bisection, no sort. */
int ta_logits_warp_ext(float* logits, long ld, int V, int B, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff,
                       hipStream_t st);
int ta_greedy_advance(const long* amax, const long* eos_ids, int n_eos, long pad_id, int* finished, long* next_ids,
                      long* out_seq, int max_new, int* step_dev, int* slot_dev, int* pos, int* kmask, int Lmax, int B,
                      int* n_unfinished, hipStream_t st);
/* Decoding scores of one step, from the PROCESSED logits [B, ld] f32 (V valid columns; columns >= V are never read; valid columns may
 * be -inf) -- what HF's compute_transition_scores(..., normalize_logits=True) gives on its `scores` (TF:generation/utils.py), without
 * ever keeping the [B, V] rows.  Writes column t = *step_dev (device memory, so the launch arguments are step-invariant; NULL = column 0;
 * t >= max_new writes nothing) of the row-major buffers logprob / entropy f32 [B, max_new] and, with top_k > 0, top_ids i64 /
 * top_logprobs f32 [B, max_new, top_k] (both may be NULL with top_k == 0; 0 <= top_k <= 8, else TA_ERR_ARG):
 *   logprob[b, t]  = x[chosen[b]] - logsumexp(x[:V])      (a chosen -inf gives -inf)
 *   entropy[b, t]  = -sum p log p over the entries with p > 0
 *   top_ids[b, t]  = the top_k largest entries, descending, lowest index first on ties (slot 0 = ta_argmax_f32's choice),
 *   top_logprobs   = their log-probabilities; slots beyond the number of finite entries are (-1, -inf).
 * Rows with finished[b] != 0 (finished BEFORE this step: they emit pad; NULL = none) get 0 / 0 / -1 / -inf.  Call between the
 * selection (ta_argmax_f32 / ta_sample_f32, whose output is `chosen`) and ta_greedy_advance, which advances *step_dev and finished.
 * One workgroup per row; B <= 64 rows of V >= 16384 columns are split over 8 workgroups per row plus a combine launch, through a
 * scratch the library owns (TA355_SCORES_SPLIT=0: never).  Calls are ordered by their stream; calls of the split form on two streams
 * at the same time would share that scratch and must be serialised by the caller. */
int ta_token_scores_f32(const float* logits, long ld, int V, int B, const long* chosen, const int* finished, const int* step_dev,
                        int max_new, int top_k, float* logprob, float* entropy, long* top_ids, float* top_logprobs, hipStream_t st);

/* ---- candidate scoring (csrc/attention_extend.hip, api.hip): log-probability of GIVEN texts under the model, the clips' prompt cache
 * shared by their candidates.  For clip b with prompt P_b and candidate c = (c_0 .. c_{n-1}), n >= 1:
 *     lp_t = log_softmax(z(P_b, c_<t))[c_t] over the V true columns, in f32;   score = sum_t lp_t in the order t = 0 .. n-1
 * i.e. minus HF's summed cross-entropy over those label positions (the `labels` path of tiny_audio/asr_modeling.py:481-533 ->
 * TF:loss/loss_utils.py ForCausalLMLoss), which re-encodes the prompt per text and returns one batch mean; and what closed-set
 * evaluation otherwise approximates by generating free text and string-matching the choices (scripts/eval/evaluators/mcq.py:89-132).
 *
 * ta_attention_extend: causal GQA attention (head_dim 128) of R rows x T given positions appended to a cache -- the pass between the
 * prompt pass ("q rows = k rows, no cache") and the decode step ("one q row against the cache"); it takes the place of the attention of
 * TF:models/qwen3/modeling_qwen3.py:185-208 when past_key_values holds the prompt and T new tokens arrive at once.  Query t of row r
 * sees (1) the prompt slots s < Lp of clip clip_of[r] with pmask[clip_of[r], s] != 0 (pmask int [B, Lp]), read in place from ONE
 * layer of the cache Kc / Vc bf16 [B, Hkv, Lmax, 128] -- never copied per row -- and (2) the row's own slots j <= t, j < len[r], of
 * Kn / Vn bf16 [R, Hkv, T, 128].  Q bf16 [R, Hq, T, 128]: Q / Kn / Vn are what ta_lm_qkv_post_fwd writes for B = R, L = T.  O bf16
 * [R*T, Hq*128] token-major like ta_attention_fwd's; LSE f32 [R, Hq, T] or NULL.  Query rows t >= len[r], and queries without any
 * visible key, get O exactly 0 (LSE 1e30).  Masked slots must hold finite values and contribute exactly nothing.  No workspace.
 * TA_ERR_ARG before any launch unless 1 <= T <= TA_EXTEND_MAX_T, 1 <= R <= TA_EXTEND_MAX_R, Hq / Hkv in {1, 2, 4}, 1 <= Lp <= Lmax,
 * B >= 1 and every pointer but LSE non-NULL. */
#define TA_EXTEND_MAX_T 256
#define TA_EXTEND_MAX_R 1024
int ta_attention_extend(const void* Q, const void* Kn, const void* Vn, const void* Kc, const void* Vc, const int* pmask,
                        const int* clip_of, const int* len, void* O, float* LSE, int B, int R, int Hq, int Hkv, int T, int Lp,
                        int Lmax, float scale, hipStream_t st);
/* ta_lm_score: the scores of R candidates of B clips after ONE ta_lm_prefill of those clips made with Lmax = L = Lp, whose kcache /
 * vcache [n_layers, B, kv_heads, Lp, 128], kmask (here pmask [B, Lp]), logits [B, vocab_pad] and lora_img it takes unchanged.
 * ids i64 [R, T] (entries behind a row's end are ignored), len int [R] on the device and the same values in len_host (host memory:
 * the number of label rows sizes the launches), clip_of int [R], pos0 int [B] = RoPE position of a clip's first new token (its number
 * of valid prompt tokens; token t sits at pos0 + t, where the decode step would place it).  The decoder layers run over the R*T rows
 * as in the prompt pass, with ta_attention_extend for the attention; token 0 is read off the prefill's logits (log-sum-exp once per
 * clip), tokens 1 .. n-1 go through the final norm, the head (f32 logits) and ta_cross_entropy in chunks of TA_SCORE_CE_ROWS label
 * rows.  Raw logits: no processor, no temperature.  token_logprobs f32 [R, T] (exact 0 at t >= len[r]); score f32 [R] = the row's sum
 * in index order (no atomics: the same bits on every run).  TA_ERR_ARG before any HIP call: a NULL among the above (lora_img only
 * with adapters), R / T beyond ta_attention_extend's limits, R*T > TA_SCORE_MAX_ROWS, B < 1, Lp < 1, Lp + T > max_pos, a len_host
 * entry outside [1, T], a model outside ta_lm_prefill's envelope, or ws_bytes < ta_lm_score_workspace_bytes(w, B, R, T). */
#define TA_SCORE_MAX_ROWS 65536
#define TA_SCORE_CE_ROWS 256
long ta_lm_score_workspace_bytes(const ta_lm_weights* w, int B, int R, int T);
int ta_lm_score(const ta_lm_weights* w, const long* ids, const int* len, const int* len_host, const int* clip_of, const int* pos0,
                int B, int R, int T, const void* kcache, const void* vcache, int Lp, const int* pmask, const float* logits,
                const void* lora_img, float* token_logprobs, float* score, void* ws, long ws_bytes, hipStream_t st);

/* ---- beam search (csrc/beam.hip): HF GenerationMixin._beam_search (TF:generation/utils.py) for do_sample=False, around the unchanged
 * ta_lm_prefill / ta_lm_decode_step.  Beams are rows: R = B * K rows, row = b * K + k; 1 <= K <= 8 beams, n_eos <= 3 eos ids,
 * M = max(2, 1 + n_eos) * K <= 32 candidates per clip and step (anything else: TA_ERR_ARG, nothing launched).  A step is
 * ta_lm_decode_step on R rows -> ta_beam_logprobs_f32 -> the ta_logits_* processors on R rows (context: the replicated prompt ids
 * followed by run_seq) -> ta_beam_topk_f32 -> ta_beam_advance -> ta_kv_beam_reorder; every argument is step-invariant (the step, the
 * slot and all flags are device memory), so the step is hipGraph-capturable like the greedy one.  All state-machine arithmetic is the
 * f32 add / compare / IEEE divide / select HF performs, in HF's order.
 *
 * ta_beam_logprobs_f32: `log_probs = nn.functional.log_softmax(logits, dim=-1)` of _beam_search, in place on rows [R, ld] f32 over
 * the first V columns (columns >= V untouched): (x - m) - log(sum e^(x - m)), -inf stays -inf, a row without a finite entry is left
 * alone.  R <= 64 rows of V >= 16384 columns are split over 8 workgroups per row through a scratch the library owns (its own, not
 * ta_token_scores_f32's); as there, such calls on two streams at once must be serialised by the caller. */
int ta_beam_logprobs_f32(float* logits, long ld, int V, int R, hipStream_t st);
/* ta_beam_topk_f32: _get_top_k_continuations (torch.topk of `log_probs + running_beam_scores[:, :, None]` reshaped [B, K * V]).
 * cand_score f32 [B, M] = the M largest of fl32(rows[b * K + k][v] + score[b * K + k]), descending; cand_flat i32 [B, M] = their
 * flat indices k * V + v (parent beam = flat / V, token = flat % V).  Ties: lowest flat index first (-inf entries included: a clip
 * with fewer than M finite values is completed by its lowest -inf indices).  ws: ta_beam_topk_workspace_bytes(B, K, V, M) bytes. */
long ta_beam_topk_workspace_bytes(int B, int K, int V, int M);
int ta_beam_topk_f32(const float* rows, long ld, int V, const float* score, int B, int K, int M, float* cand_score, int* cand_flat,
                     void* ws, long ws_bytes, hipStream_t st);
/* ta_beam_advance: the rest of one _beam_search iteration for step t = *step_dev, one workgroup per clip:
 *   stopping criteria                       hit[c] = token[c] is an eos id, or t + 1 == max_new
 *   _get_running_beams_for_next_iteration   the K best of cand_score + hit * -1e9 -> run_score f32 [R], parent i32 [R] (the beam each
 *                                           new row continues), next_ids i64 [R], run_seq i64 [R, max_new] (permuted through LDS:
 *                                           K * max_new <= 12288) with the new token at column t
 *   _update_finished_beams                  only the first K candidates may finish; cand_score / len_div[t] (len_div f32 [max_new],
 *                                           len_div[n - 1] = float32(float(n) ** length_penalty) from the host), then + -1e9 for "pool
 *                                           full and early_stopping is True", for "heuristic satisfied", for "did not just finish", in
 *                                           that order; merged behind the pool, the K best kept: pool_seq i64 [B, K, max_new] (padded
 *                                           with pad_id), pool_score f32 [B, K], pool_len i32 [B, K], pool_fin i32 [B, K] (is_sent_finished)
 *   _check_early_stop_heuristic             heur i32 [B] (is_early_stop_heuristic_unsatisfied); heur_max_len != 0 when early_stopping
 *                                           is "never" and length_penalty > 0 (the divisor is then len_div[max_new - 1], else len_div[t])
 *   _beam_search_has_unfinished_sequences   clip_done i32 [B], sticky; *n_unfinished = clips not done.  HF stops the whole batch on
 *                                           batch-wide any / all; a done clip keeps stepping here and its pool no longer changes.
 * early_stopping: 0 False, 1 True, 2 "never".  Initial state: run_score = 0, -1e9, ... per clip, pool_score = -1e9, pool_fin = 0,
 * heur = 1, clip_done = 0.  Also advances *step_dev, *slot_dev, pos [R] and kmask [R, Lmax] as ta_greedy_advance does.  The five tr_*
 * pointers (all or none) receive at index t of [max_new, ...] buffers: the candidates [B, M], run_seq / run_score as they stood
 * BEFORE the step ([R, max_new] / [R]) and parent [R]. */
int ta_beam_advance(const float* cand_score, const int* cand_flat, int B, int K, int M, int V, const long* eos_ids, int n_eos,
                    long pad_id, int max_new, const float* len_div, int early_stopping, int heur_max_len, long* run_seq,
                    float* run_score, int* parent, long* next_ids, long* pool_seq, float* pool_score, int* pool_len,
                    int* pool_fin, int* heur, int* clip_done, int* step_dev, int* slot_dev, int* pos, int* kmask, int Lmax,
                    int* n_unfinished, float* tr_cand_score, int* tr_cand_flat, long* tr_run_seq, float* tr_run_score,
                    int* tr_parent, hipStream_t st);
/* The cache of a beam run, bf16 [layers, R, kv_heads, Lmax, head_dim] (head_dim a multiple of 8), moved in 16-byte pieces.
 * ta_kv_beam_expand (_expand_inputs_for_generation): slots [0, L) of clip b of the B-row prefill caches [layers, B, kv_heads, Lsrc,
 * head_dim] -> rows b * K .. b * K + K - 1.  ta_kv_beam_reorder (the `reorder_cache(beam_idx)` of _beam_search): the generated slots
 * [L, *slot_dev) of the K rows of every clip permuted in place by parent [R] (row j takes row parent[j]'s), both caches, every layer;
 * a lane loads its piece of all K rows before it stores any, so no scratch copy is needed.  Prompt slots are never touched; clips
 * whose parent is the identity, and K == 1, move nothing.  Lmax >= L + max_new; the grid covers max_new slots. */
int ta_kv_beam_expand(const void* ksrc, const void* vsrc, void* kdst, void* vdst, int layers, int B, int K, int kv_heads, int L,
                      int Lsrc, int Lmax, int head_dim, hipStream_t st);
int ta_kv_beam_reorder(void* kcache, void* vcache, int layers, int B, int K, int kv_heads, int L, int Lmax, int head_dim, int max_new,
                       const int* parent, const int* slot_dev, hipStream_t st);

/* loss.backward() through the LM (replaces autograd over Qwen3ForCausalLM, tiny_audio/asr_modeling.py:517-533).
 * d_audio f32 [n_audio_rows, D] (zeroed, then rows referenced by src_row written; NULL = not wanted, e.g. frozen
 * projector); d_embeds optional [B*L, D]; lora_grads: host array [n_layers] (required iff w->lora_rank > 0, zeroed and
 * written); wgrads: NULL for a frozen LM, else the weight-gradient buffers of ta_lm_wgrads (w->train_base must be 1; they
 * are ACCUMULATED into) together with ids [B, L] i64, the token ids of the forward (input-lookup share of the embedding). */
int ta_lm_backward(const ta_lm_weights* w, const int* src_row, const int* kmask, const int* pos, int B, int L,
                   const int* label_rows, int n_label_rows, float* d_audio, long n_audio_rows, float* d_embeds,
                   const ta_lm_lora_grads* lora_grads, const ta_lm_wgrads* wgrads, const long* ids, const void* tape, void* ws,
                   long ws_bytes, hipStream_t st);

/* ---- LoRA dropout (peft LoraLayer with lora_dropout = p > 0; tiny_audio/asr_modeling.py:289-301 forwards config.lora_dropout
 * to LoraConfig).  In TRAINING mode every adapted linear j has its own nn.Dropout(p) on the adapter's input:
 *     y_j = W_j x + s B_j A_j (x (.) K_j / (1 - p)),    s = alpha / r,  K_j ~ Bernoulli(1 - p) per element of x,
 * so the members of the q|k|v and gate|up groups see the same x under three / two independent masks.  The backward uses the
 * forward's masks: dB_j = dy_j^T xa_j (xa already holds the dropped product), dA_j = s (dy_j B_j)^T (x (.) K_j / (1 - p)) and
 * d(x) += sum_j (s (dy_j B_j) A_j) (.) K_j / (1 - p).  Evaluation and decoding never apply dropout (no descriptor there).
 *
 * Masks are never stored: the keep decision of element (m, c) of linear j (peft order q, k, v, o, gate, up, down = 0..6) in
 * decoder layer l, m the row of the [B*L] row space, is a pure function of (seed, offset, l, j, m, c) -- Philox4x32-10 with
 *     counter = ((8 l + j) << 20 | c >> 3,  m,  lo32(offset),  hi32(offset)),   key = (lo32(seed), hi32(seed)),
 * 16-bit half (c & 1) (low half first) of output word (c & 7) >> 1 = u16;  keep <=> u16 >= round(p * 65536).
 * One call decides 8 consecutive columns; the DROP probability is p rounded to a multiple of 2^-16 (the kept values are scaled by
 * 1 / (1 - p) with p as given).  Valid for in_features < 2^23 and n_layers < 512.  The backward regenerates what its forward drew,
 * so it must get the SAME descriptor; ta_lm_tape_bytes does not depend on it.  tiny_audio_amd/lora_dropout.py is a numpy twin. */
typedef struct ta_lora_dropout {
  float p;                          /* 0 <= p < 1; 0 = off */
  unsigned long long seed;          /* Philox key */
  unsigned long long offset;        /* Philox counter words 2-3: a fresh value per training forward (and per rank) */
} ta_lora_dropout;
/* ta_lm_forward_loss / ta_lm_backward with LoRA dropout: drop NULL or drop->p == 0 is exactly the plain call (the plain entry
 * points are these with NULL).  drop->p > 0 needs w->lora_rank > 0. */
int ta_lm_forward_loss_ex(const ta_lm_weights* w, const long* ids, const int* src_row, const float* audio,
                          const int* kmask, const int* pos, int B, int L, const int* label_rows,
                          const long* label_targets, int n_label_rows, float loss_scale, float* loss,
                          float* nll_rows, void* logits_out, void* tape, void* ws, long ws_bytes,
                          const ta_lora_dropout* drop, hipStream_t st);
int ta_lm_backward_ex(const ta_lm_weights* w, const int* src_row, const int* kmask, const int* pos, int B, int L,
                      const int* label_rows, int n_label_rows, float* d_audio, long n_audio_rows, float* d_embeds,
                      const ta_lm_lora_grads* lora_grads, const ta_lm_wgrads* wgrads, const long* ids, const void* tape, void* ws,
                      long ws_bytes, const ta_lora_dropout* drop, hipStream_t st);
/* ---- Sequence packing: several clips per LM row, block-diagonal causal attention.  A packed row holds S >= 1 segments back to back
 * (one segment = one clip's whole chat sequence) and right padding; segment_ids int32 [R, L] is 0 on padding and 1..S, non-decreasing
 * and gap-free, on the tokens.  The query at (r, q) sees the key at (r, k) iff both carry the same non-zero id and k <= q.
 * ta_segment_table: seg int32 [2, R*L] -- plane 0 the index of the first token of q's segment (q + 1 on padding), plane 1 one past
 * the last token of k's segment (k on padding) -- and, unless NULL, pos int32 [R*L], the RoPE positions restarting at 0 in every
 * segment.  The attention kernels test  seg[q] <= k <= q  next to the key mask and skip the KV / query tiles outside those bounds.
 * ta_audio_index_seg: ta_audio_index for packed rows.  counts i64 [C] and the projector output [C, N, D] are per CLIP, clip c being the
 * c-th segment row-major over (row, segment); the j-th <audio> token of that segment takes row c*N + j while j < counts[c] and j < N,
 * -2 (a zero row) beyond, exactly as ta_audio_index treats surplus placeholders; every other token -1.
 * ta_lm_forward_loss_seg / ta_lm_backward_seg: the _ex calls with the table next to kmask / pos (the backward needs the forward's
 * table: it is not on the tape, and ta_lm_tape_bytes / ta_lm_workspace_bytes do not change).  seg NULL is exactly the _ex call.  The
 * caller masks the label at the first token of every segment, so that the last token of one clip never predicts the next clip. */
int ta_segment_table(const int* segment_ids, int* seg, int* pos, int R, int L, hipStream_t st);
int ta_audio_index_seg(const long* ids, const int* segment_ids, const long* counts, int* src_row, int R, int L, int C, int N,
                       long audio_id, hipStream_t st);
int ta_lm_forward_loss_seg(const ta_lm_weights* w, const long* ids, const int* src_row, const float* audio,
                           const int* kmask, const int* pos, const int* seg, int B, int L, const int* label_rows,
                           const long* label_targets, int n_label_rows, float loss_scale, float* loss,
                           float* nll_rows, void* logits_out, void* tape, void* ws, long ws_bytes,
                           const ta_lora_dropout* drop, hipStream_t st);
int ta_lm_backward_seg(const ta_lm_weights* w, const int* src_row, const int* kmask, const int* pos, const int* seg, int B, int L,
                       const int* label_rows, int n_label_rows, float* d_audio, long n_audio_rows, float* d_embeds,
                       const ta_lm_lora_grads* lora_grads, const ta_lm_wgrads* wgrads, const long* ids, const void* tape, void* ws,
                       long ws_bytes, const ta_lora_dropout* drop, hipStream_t st);
/* The LM forward with loss options (ta_ce_options, below at ta_cross_entropy_opt; replaces TF:trainer_pt_utils.py LabelSmoother over
 * TF:loss/loss_utils.py fixed_cross_entropy): ta_lm_forward_loss_seg plus `ce`.  One entry point serves the three call shapes: seg NULL
 * and drop NULL is the plain forward, seg NULL the _ex one.  `loss` accumulates loss_scale * sum of the objective (summed in row order
 * from ce->obj [n_label_rows]), nll_rows stays the plain NLL, and the tape's dlogits are the objective's: every ta_lm_backward* entry
 * point consumes them unchanged.  ce NULL is exactly ta_lm_forward_loss_seg.  eps > 0 or zc > 0 with ce->obj NULL is TA_ERR_ARG: the
 * training step's loss is never summed with float atomics. */
struct ta_ce_options;
int ta_lm_forward_loss_opt(const ta_lm_weights* w, const long* ids, const int* src_row, const float* audio,
                           const int* kmask, const int* pos, const int* seg, int B, int L, const int* label_rows,
                           const long* label_targets, int n_label_rows, float loss_scale, float* loss,
                           float* nll_rows, void* logits_out, void* tape, void* ws, long ws_bytes,
                           const ta_lora_dropout* drop, const struct ta_ce_options* ce, hipStream_t st);
/* The attention entry points of the LM over packed rows (causal, head_dim 128; seg NULL = the plain call). */
int ta_attention_fwd_seg(const void* Q, const void* K, const void* VT, void* O, float* LSE, const int* kmask, const int* seg,
                         int B, int Hq, int Hkv, int L, int Lp, float scale, hipStream_t st);
int ta_attention_fwd_qkv_seg(const void* qkv0, const float* qn_w, const float* kn_w, const float* cosT, const float* sinT,
                             const int* pos, void* Q, void* K, void* V, float* rq, float* rk, void* O, float* LSE,
                             const int* kmask, const int* seg, int B, int Hq, int Hkv, int L, float scale, float eps,
                             hipStream_t st);
int ta_attention_bwd_seg(const void* Q, const void* K, const void* V, const void* dO, long dO_stride, const float* LSE,
                         const float* Delta, const int* kmask, const int* seg, void* dQ, void* dK, void* dV, int B, int Hq,
                         int Hkv, int L, int Lp, float scale, hipStream_t st);
int ta_attention_bwd_qkv_seg(const void* Q, const void* K, const void* V, const void* dO, long dO_stride, const float* LSE,
                             const float* Delta, const int* kmask, const int* seg, const void* qkv0, const float* rq,
                             const float* rk, const float* qn_w, const float* kn_w, const float* cosT, const float* sinT,
                             const int* pos, void* dqkv, int B, int Hq, int Hkv, int L, int Lp, float scale, hipStream_t st);
/* The keep mask of linear `linear` (0..6, peft order) in layer `layer` over M rows x in columns: out u8 [M, in] (1 = kept). */
int ta_lora_dropout_keep(const ta_lora_dropout* drop, int layer, int linear, int M, int in, unsigned char* out, hipStream_t st);

/* ============================================================================================
 * Primitive kernels (exported for the parity tests; also what the composites are built from)
 * ============================================================================================ */

/* GLM-ASR encoder self-attention straight from the q|k|v GEMM output (TF:models/glmasr/modeling_glmasr.py:187-217: non-causal,
 * no mask, head_dim 64).  qkv bf16 [B*S, 3*heads*64] token-major, thirds q | k | v, head h at columns h*64 of each third; the
 * q values must already carry head_dim^-0.5 * log2(e) (ta_enc_layer.wqkv_fa): out = softmax_base2(q k^T) v, bf16 [B*S, heads*64]. */
int ta_attention_enc_fwd(const void* qkv, void* out, int B, int heads, int S, hipStream_t st);
/* The same over clips of different lengths, for ta_encoder_forward_ragged (replaces one GlmAsrAttention.forward per clip,
 * TF:models/glmasr/modeling_glmasr.py:187-217, on that clip's frames alone): clip b owns rows cu_rows[b] .. cu_rows[b + 1] of
 * qkv [rows, 3*heads*64] and out [rows, heads*64]; cu_rows DEVICE int [B + 1], non-decreasing from 0; max_rows = the longest clip's
 * row count (sizes the grid).  Clip b's rows are bit-identical to ta_attention_enc_fwd on those rows with B = 1, S = its length. */
int ta_attention_enc_fwd_varlen(const void* qkv, void* out, const int* cu_rows, int B, int heads, int max_rows, hipStream_t st);

/* C = epilogue(A[M,K] x W[N,K]^T).  A/C rows are mapped  row -> (row / rpb) * bs + (row % rpb) * ld
 * (rpb <= 0 means "no batching").  act: 0 none, 1 erf-GELU.  residual: f32, C's row map.
 * splits > 1: split-K through splitk_ws (f32 [splits, M, N]); then no bias/act, plain C layout. */
int ta_gemm_bf16_nt(const void* A, const void* W, void* C, int M, int N, int K, long lda, int a_rpb, long a_bs,
                    long ldc, int c_rpb, long c_bs, long c_off, const float* bias, const float* residual, int act,
                    int out_bf16, int splits, float* splitk_ws, hipStream_t st);
/* Grouped / routed form (MoE experts): a_idx (gather list for A rows), seg {row base, row count} and krange
 * {first, end} 64-wide K tile are DEVICE int arrays read by the kernel, so routing counts never visit the host.
 * M is then only the upper bound used to size the grid. */
int ta_gemm_bf16_nt_ex(const void* A, const void* W, void* C, int M, int N, int K, long lda, int a_rpb, long a_bs,
                       long ldc, int c_rpb, long c_bs, long c_off, const float* bias, const float* residual, int act,
                       int out_bf16, int splits, float* splitk_ws, const int* a_idx, const int* seg,
                       const int* krange, hipStream_t st);
/* Optional extras of one GEMM call (all pointers NULL = plain GEMM).  Passed by value semantics: read during the call,
 * no state is kept (the composites run on any host thread / stream concurrently).
 *   a2/w2/k2/lda2   K extension (LoRA): C = epilogue(A W^T + A2 W2^T), A2 [M, k2] (row stride lda2), W2 [N, k2],
 *                   k2 % 64 == 0, in the same accumulator pass (no split-K, no krange)
 *   residual_bf16   bf16 residual with C's row map (may alias C); the call's f32 `residual` must then be NULL.  The
 *                   frozen models' residual adds in the model dtype (TF:models/glmasr/modeling_glmasr.py:249-270,
 *                   TF:models/qwen3/modeling_qwen3.py:283-324 on bf16 models)
 *   rope_tab/rows   act == 2: GLM-ASR partial rotary embedding (TF:models/glmasr/modeling_glmasr.py:153-168) applied to the
 *                   bf16 result after the bias.  Heads are 64 columns (N % 64 == 0); W's rows must be ordered so that the
 *                   first 32 columns of each head hold the 16 rotation pairs interleaved -- column 2i = head dim i,
 *                   column 2i+1 = head dim i+16 -- and columns 32..63 = head dims 32..63 (q and k permuted alike leave
 *                   q.k unchanged).  rope_tab f32 [rope_rows][16][2] = (cos, sin) of pair i at position p; row m of the
 *                   GEMM is position m % rope_rows. */
typedef struct {
  const void* a2; const void* w2; int k2; long lda2;
  const void* residual_bf16;
  const float* rope_tab; int rope_rows;
  int w_blocked;   /* W is given as [N/64][K/64][64][64] blocks (N % 64 == 0): each 64-row x 64-column K tile 8 KB contiguous */
  int rope_cols;   /* act == 2: the rotary embedding applies to columns [0, rope_cols) only (0 = all N columns); % 64 == 0 */
} ta_gemm_opts;
int ta_gemm_bf16_nt_opt(const void* A, const void* W, void* C, int M, int N, int K, long lda, int a_rpb, long a_bs,
                        long ldc, int c_rpb, long c_bs, long c_off, const float* bias, const float* residual, int act,
                        int out_bf16, int splits, float* splitk_ws, const int* a_idx, const int* seg,
                        const int* krange, const ta_gemm_opts* opts, hipStream_t st);
long ta_gemm_splitk_ws_bytes(int M, int N, int splits);
/* Grouped GEMMs: every expert of the MoE projector in ONE launch (tiny_audio/projectors.py:327-345 loops over the experts
 * in Python).  n_groups <= 8; exactly one of seg / krange is given (DEVICE int arrays, read by the kernel):
 *   rows form     seg = int[2 * n_groups] {row base, row count} over a common row space (the expert-sorted token slots).
 *                 Group e: C[rows of e, :] = act(A[rows of e (through a_idx, if given), :] (W + e * w_stride)^T + bias[e * N ...]).
 *                 M = upper bound of the TOTAL row count (grid sizing); the tile -> (expert, row tile) map is resolved on the
 *                 device, so routing counts never visit the host.
 *   K-slice form  krange = int[2 * n_groups] {first, end} 64-wide K tile.  Group e: (C + e * c_stride)[M, N] = A[:, slice e]
 *                 W[:, slice e]^T, f32, no bias / activation (per-expert weight gradients: the contraction runs over the slot
 *                 axis, which the counting-sort plan keeps contiguous and 64-aligned per expert). */
int ta_gemm_bf16_nt_grouped(const void* A, const void* W, void* C, int M, int N, int K, const float* bias, int act, int out_bf16,
                            const int* a_idx, const int* seg, const int* krange, int n_groups, long w_stride, long c_stride,
                            hipStream_t st);
/* "TN" product (contraction over the ROWS of both row-major operands): out f32 [Ny, Nx] (+)= Y[M, Ny]^T X[M, Nx] -- the
 * weight gradient dW = dY^T X of a linear layer (full decoder fine-tuning) without transposing dY and X first.
 * Ny, Nx multiples of 8; ws: ta_gemm_bf16_tn_ws_bytes(M, Ny, Nx) bytes of scratch (row-chunk partial sums). */
long ta_gemm_bf16_tn_ws_bytes(int M, int Ny, int Nx);
int ta_gemm_bf16_tn(const void* Y, const void* X, float* out, int M, int Ny, int Nx, int accumulate, void* ws, long ws_bytes,
                    hipStream_t st);
/* in-situ GEMM timing for bench.py's roofline leg: HIP events on the launch stream around every GEMM kernel.
 * collect(): host pointers; sums + clears the records (total kernel ms, total 2*M*N*K flops, launches). */
int ta_profile_gemm(int enable);   /* 0 off, 1 time every launch (collect below), 2 log every launch's shape (ta_profile_gemm_log) */
int ta_profile_gemm_collect(double* total_ms, double* total_flops, long* launches);
/* round 4: the launches since ta_profile_gemm(2) as rows of 24 longs {M, N, K, lda, a_rpb, a_bs, ldc, c_rpb, c_bs, c_off, act,
 * out_bf16, has_residual, residual_bf16, has_bias, splits, rope_cols, rope_rows, flags, K2, tile variant, groups, lnf mode,
 * persistent} (flags: 1 gather, 2 segments, 4 K range, 8 K extension, 16 blocked W, 32 grouped, 64 LayerNorm fold, 128 SwiGLU
 * backward, 256 / 512 identity A / C row map).  Host memory; returns the row count (out may be NULL).  The step-shape parity test
 * (tests/test_gpu_round4.py) runs one real B = 32 step under it and replays every distinct launch against an fp32 matmul. */
long ta_profile_gemm_log(long* out, long max_rows);
/* round 4: the library reads its environment knobs (TA355_GEMM_VARIANT, TA355_GELU_LUT, TA355_DECODE_FUSED) ONCE, at first use;
 * this re-reads them (tests and A/B scripts that switch a knob between launches). */
int ta_gemm_reload_knobs(void);

int ta_layernorm_f32(const float* x, const float* w, const float* b, void* y_bf16, float* y_f32,
                     const float* rowscale, int M, int H, float eps, hipStream_t st);
int ta_layernorm_bf16(const void* x_bf16, const float* w, const float* b, void* y_bf16, float* y_f32, const float* rowscale,
                      int M, int H, float eps, hipStream_t st);            /* same, the row is read as bf16 */
int ta_rmsnorm_fwd(const float* x, const float* w, void* y_bf16, float* y_f32, float* rstd, int M, int H,
                   float eps, int act_gelu, hipStream_t st);
int ta_rmsnorm_bwd(const float* dy, const float* x, const float* rstd, const float* w, const float* dres,
                   float* dx_f32, void* dx_bf16, float* dw_accum, int M, int H, int act_gelu, hipStream_t st);
/* the same with x read as bf16 (frozen weights: no dw, no GELU): the LM's residual stream in the model dtype */
int ta_rmsnorm_fwd_bf16(const void* x_bf16, const float* w, void* y_bf16, float* y_f32, float* rstd, int M, int H, float eps,
                        hipStream_t st);
int ta_rmsnorm_bwd_bf16(const void* dy, int dy_is_bf16, const void* x_bf16, const float* rstd, const float* w,
                        const float* dres, float* dx_f32, void* dx_bf16, int M, int H, hipStream_t st);
/* round 4: the same with the residual gradient ALSO bf16 -- the LM's d(x) stream in the reference's dtype (its bf16 model back-
 * propagates bf16 activations' gradients); dres_bf16 may alias dx_bf16 (updated in place), dx_f32 is optional (NULL except where an
 * f32 consumer follows: the embedding / audio-row gather at the bottom of the stack) */
int ta_rmsnorm_bwd_bf16s(const void* dy, int dy_is_bf16, const void* x_bf16, const float* rstd, const float* w,
                         const void* dres_bf16, float* dx_f32, void* dx_bf16, int M, int H, hipStream_t st);
/* the fp32-stream counterpart (round 6): x, dres, dx_f32 fp32, the incoming gradient bf16 (under the recipe's bf16 autocast the
 * gradient of a Linear's bf16 input IS a bf16 tensor), a bf16 image of dx beside it (either output may be NULL) */
int ta_rmsnorm_bwd_dyb(const void* dy_bf16, const float* x, const float* rstd, const float* w, const float* dres, float* dx_f32,
                       void* dx_bf16, int M, int H, hipStream_t st);

/* d loss / d weight of an RMSNorm (y = w * x * rstd): dw_accum[h] += sum_m dy[m,h] * x[m,h] * rstd[m]; dy and x are f32 or bf16 */
int ta_rmsnorm_dw(const void* dy, int dy_is_bf16, const void* x, int x_is_bf16, const float* rstd, float* dw_accum, int M,
                  int H, hipStream_t st);

int ta_attention_fwd(const void* Q, const void* K, const void* VT, void* O, float* LSE, const int* kmask, int B,
                     int Hq, int Hkv, int L, int Lp, int head_dim, int causal, float scale, hipStream_t st);
/* The same over caller-described operand layouts (element strides; NULL = the head-major defaults above):
 *   Q(b,h,row,d)  = Q  + b*q_bs + h*q_hs + row*q_rs + d        K likewise with k_*
 *   VT(b,h,d,col) = VT + b*v_bs + h*v_hs + d*v_rs + col
 * so the encoder reads q | k straight from the token-major GEMM output [B*L, 2*H*64] and V^T from the [H*64, B*L]
 * result of V^T = Wv xn^T (v_bs = L, v_rs = B*L: key columns beyond L belong to the next clip -- they are masked,
 * but must be readable and finite: keep 64 elements of slack behind the image).  Column offsets that are not
 * multiples of 8 elements are read with narrower loads. */
typedef struct { long q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs; } ta_attn_layout;
int ta_attention_fwd_ex(const void* Q, const void* K, const void* VT, void* O, float* LSE, const int* kmask, int B,
                        int Hq, int Hkv, int L, int Lp, int head_dim, int causal, float scale, const ta_attn_layout* lay,
                        hipStream_t st);
/* ta_lm_qkv_post_fwd + ta_attention_fwd in ONE launch for short causal sequences (head_dim 128, L <= 192, (Hq / Hkv) * ceil(L / 32)
 * <= 12; otherwise TA_ERR_ARG and nothing is launched): qkv0 is the pre-norm q | k | v GEMM output [B*L, (Hq + 2 Hkv) * 128]; writes
 * O [B*L, Hq*128], LSE and the backward's operands Q / K (normalised, rotated) and V head-major [B, heads, L, 128], rq / rk (1 / rms per
 * (token, head)).  V may be NULL (round 6): V is neither normalised nor rotated, so ta_attention_bwd_qkv can read it in place from
 * qkv0 and the head-major copy is only needed by callers that use it themselves (the KV cache of ta_lm_prefill, ta_attention_bwd).
 * tiny_audio path: TF:models/qwen3/modeling_qwen3.py:211-280 forward. */
/* qn_w == kn_w == NULL: no q/k-norm (rq / rk are then neither written nor needed: they may be NULL); cosT == sinT == NULL: no rotary
 * embedding (a NoPE layer).  The two switches are independent; each combination is its own kernel instantiation.  The same convention
 * holds for ta_attention_bwd_qkv, ta_lm_qkv_post_fwd and ta_lm_qkv_post_bwd; one pointer of a pair NULL and the other not is TA_ERR_ARG. */
int ta_attention_fwd_qkv(const void* qkv0, const float* qn_w, const float* kn_w, const float* cosT, const float* sinT,
                         const int* pos, void* Q, void* K, void* V, float* rq, float* rk, void* O, float* LSE,
                         const int* kmask, int B, int Hq, int Hkv, int L, float scale, float eps, hipStream_t st);
/* backward of the causal GQA attention (head_dim 128).  QT / KT / dOT are IGNORED since round 2 (pass NULL): the kernels read the
 * transposed fragments out of their row tiles with ds_read_b64_tr_b16, so no transposed image has to be produced or staged. */
int ta_attention_bwd(const void* Q, const void* QT, const void* K, const void* KT, const void* V, const void* dO,
                     long dO_stride, const void* dOT, const float* LSE, const float* Delta, const int* kmask,
                     void* dQ, void* dK, void* dV, int B, int Hq, int Hkv, int L, int Lp, int head_dim, int causal,
                     float scale, hipStream_t st);
/* the same with ta_lm_qkv_post_bwd fused into its epilogue (frozen q_norm / k_norm): d(qkv0) token-major [B*L, (Hq + 2 Hkv) * 128] is
 * written directly from the f32 accumulators; no head-major dQ / dK / dV (tiny_audio path: TF:models/qwen3/modeling_qwen3.py:211-280 backward).
 * V == NULL: the V rows are read in place from qkv0 (columns (Hq + Hkv) * 128 ...), see ta_attention_fwd_qkv. */
int ta_attention_bwd_qkv(const void* Q, const void* K, const void* V, const void* dO, long dO_stride, const float* LSE,
                         const float* Delta, const int* kmask, const void* qkv0, const float* rq, const float* rk,
                         const float* qn_w, const float* kn_w, const float* cosT, const float* sinT, const int* pos,
                         void* dqkv, int B, int Hq, int Hkv, int L, int Lp, int head_dim, int causal, float scale,
                         hipStream_t st);
int ta_enc_qkv_post(const void* qkv, const float* cosT, const float* sinT, void* Q, void* K, void* VT, int B, int H,
                    int S, int Sp, hipStream_t st);
/* QT / KT / VT: transposed images [B, heads, 128, Lp]; any of them may be NULL (not written).  The forward attention needs VT only. */
int ta_lm_qkv_post_fwd(const void* qkv0, const float* qn_w, const float* kn_w, const float* cosT, const float* sinT,
                       const int* pos, void* Q, void* K, void* V, void* QT, void* KT, void* VT, float* rq, float* rk,
                       int B, int Hq, int Hkv, int L, int Lp, float eps, hipStream_t st);
int ta_lm_qkv_post_bwd(const void* dQ, const void* dK, const void* dV, const void* qkv0, const float* rq,
                       const float* rk, const float* qn_w, const float* kn_w, const float* cosT, const float* sinT,
                       const int* pos, void* dqkv, float* dqn_accum, float* dkn_accum, int B, int Hq, int Hkv, int L, hipStream_t st);   /* dqn/dkn_accum [128] or NULL: += the q_norm / k_norm weight gradients */
/* Delta = rowsum(dO o O); dOT (optional, may be NULL): the transposed dO image, no longer read by ta_attention_bwd */
int ta_attn_bwd_prep(const void* dO, const void* O, float* Delta, void* dOT, int B, int Hq, int L, int Lp,
                     hipStream_t st);

int ta_swiglu_fwd(const void* gu, void* act, long M, int F, hipStream_t st);
int ta_swiglu_bwd(const void* dact, const void* gu, void* dgu, long M, int F, hipStream_t st);
int ta_cast_f32_bf16(const float* x, void* y, long n, hipStream_t st);
int ta_transpose_to_bf16(const void* in, int in_is_f32, long ld_in, long in_bs, int in_rpb, void* out, long ld_out,
                         int R, int C, hipStream_t st);
int ta_feats_to_time_major(const float* feats, void* out, int B, int C, int T, hipStream_t st);
int ta_zero_pad_rows(void* buf, int B, int T, int C, hipStream_t st);
/* Whisper's position table: x [B*S, H] (f32 if x_f32 else bf16) += pos f32 [S, H], row m taking table row m % S
 * (hidden_states = inputs_embeds + embed_positions.weight, TF:models/whisper/modeling_whisper.py:622-624).  H % 8 == 0. */
int ta_pos_add(void* x, int x_f32, const float* pos, int B, int S, int H, hipStream_t st);

/* <audio> placeholder bookkeeping: _gather_audio_embeds + masked_scatter
 * (tiny_audio/asr_modeling.py:27-44,511-515). */
int ta_audio_index(const long* ids, const long* counts, int* src_row, int B, int L, int N, long audio_id,
                   hipStream_t st);
int ta_embed_scatter(const long* ids, const int* src_row, const float* emb, const float* audio, float* x0,
                     void* x0_bf16, int n_rows, int D, long vocab, hipStream_t st);
int ta_audio_grad_gather(const int* src_row, const float* dx0, float* d_audio, int n_rows, int D, hipStream_t st);
/* input-lookup share of the embedding gradient: dembed[ids[m], :] += dx0[m, :] for every text row (src_row[m] == -1 or src_row NULL) */
int ta_embed_grad_scatter(const long* ids, const int* src_row, const float* dx0, float* dembed, int n_rows, int D, long vocab,
                          hipStream_t st);
int ta_gather_rows_bf16(const void* in, const int* idx, void* out, int n, int D, hipStream_t st);
int ta_scatter_rows_f32(const float* in, const int* idx, float* out, int n, int D, hipStream_t st);
int ta_bernoulli_keep(float* keep, long n, float keep_prob, unsigned long long seed, hipStream_t st);
/* Instrumentation (not on the hot path): `workgroups` x 256 threads stay resident for `micros` microseconds streaming buf [bytes]
 * (read + write back) -- the footprint of a ring all-reduce's channel workgroups next to the step's kernels.  scripts/allreduce_footprint.py
 * uses it to choose the N > 1 default (overlapped vs synchronous all-reduce) on a one-GPU box. */
int ta_debug_occupy(int workgroups, double micros, void* buf, long bytes, hipStream_t st);

/* TA_ERR_ARG unless ldl % 4 == 0 and V <= ldl, and, with dlogits, ldd % 4 == 0 and ldd >= V. */
int ta_cross_entropy(const void* logits, int logits_bf16, long ldl, const int* rows, const long* targets, int n, int V,
                     float scale, float* nll, float* loss_accum, void* dlogits_bf16, long ldd, hipStream_t st);
int ta_label_rows(const long* labels, int B, int L, int* rows, long* targets, int* n_out, hipStream_t st);
/* ---- LM loss options, fused into the cross-entropy pass (TF:trainer_pt_utils.py LabelSmoother, i.e. TrainingArguments.
 * label_smoothing_factor, and torch.nn.functional.cross_entropy(label_smoothing=) inside TF:loss/loss_utils.py fixed_cross_entropy;
 * z-loss: coef * logsumexp^2 per target row, PaLM).  Per row r with a valid target t, over the V true columns:
 *     nll_r = lse_r - z_rt                                                        (what `nll` keeps holding)
 *     obj_r = (1 - eps) nll_r + eps (lse_r - mean_v z_rv) + zc lse_r^2            (what the loss sums, times scale)
 *     dlogits_rv = scale (p_rv (1 + 2 zc lse_r) - (1 - eps) [v == t] - eps / V),  p_rv = exp(z_rv - lse_r)
 * Rows with an invalid target keep nll = obj = 0 and a zero dlogits row, columns >= V exact zeros.  The mean is accumulated as
 * sum_v (z_rv - z_r0), so it is as invariant to a shift of the row as lse - z_t.  0 <= eps < 1 and zc >= 0, else TA_ERR_ARG. */
typedef struct ta_ce_options {
  float eps;                        /* label smoothing; 0 = off */
  float zc;                         /* z-loss coefficient; 0 = off */
  float* obj;                       /* [n] per-row objective, or NULL.  With it the loss is summed from it in row order (the same
                                     * bits on every run); without it every row adds itself to loss_accum atomically. */
} ta_ce_options;
/* ta_cross_entropy with options (replaces TF:trainer_pt_utils.py LabelSmoother over TF:loss/loss_utils.py fixed_cross_entropy).
 * opt NULL, or eps == zc == 0 with obj NULL, is exactly ta_cross_entropy (the plain entry point is this with NULL). */
int ta_cross_entropy_opt(const void* logits, int logits_bf16, long ldl, const int* rows, const long* targets, int n, int V,
                         float scale, float* nll, float* loss_accum, void* dlogits_bf16, long ldd, const ta_ce_options* opt,
                         hipStream_t st);

/* optimizer: clip_grad_norm_(max_norm) + AdamW on fp32 masters (configs/training/production.yaml:5-9) */
/* accum[0] += sum(g^2), DETERMINISTICALLY (two launches: per-block partials into scratch, then one block adds them in index order):
 * data-parallel ranks that hold the same all-reduced gradient must compute bit-identical clip coefficients, or their replicas
 * drift apart.  scratch: float[TA_SQNORM_SCRATCH_FLOATS], no initial contents required. */
#define TA_SQNORM_SCRATCH_FLOATS 1024
int ta_grad_sqnorm(const float* g, long n, float* accum, float* scratch, hipStream_t st);
int ta_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, const float* sqnorm, float max_norm, float grad_scale,
                  const float* denom, hipStream_t st);
/* the same update for a flat buffer of nseg parameter tensors in ONE launch (scripts/train.py:406-432: per-group learning rate and
 * weight decay): segment s ends at element seg_end[s] (device long[nseg], multiples of 4, seg_end[nseg-1] == n), has learning
 * rate seg_lr[s] * lr_mult and weight decay seg_wd[s] (device float[nseg]).  Bit-identical to ta_adamw_step per segment. */
int ta_adamw_step_multi(float* p, const float* g, float* m, float* v, long n, const long* seg_end, const float* seg_lr,
                        const float* seg_wd, int nseg, float lr_mult, float beta1, float beta2, float eps, int step,
                        const float* sqnorm, float max_norm, float grad_scale, const float* denom, hipStream_t st);

/* ---- device-side waveform augmentation, between the upload of wav [B, Ls] and ta_logmel_f32 (tiny_audio_amd/csrc/augment.hip).
 * Replaces the numeric stages that the reference's production recipe (configs/training/production.yaml:67-140) runs in CPU
 * dataloader workers through audiomentations (tiny_audio/augmentation.py:71-223, wired at scripts/train.py:530-587), in the
 * reference's order: ApplyImpulseResponse, AddBackgroundNoise, AddGaussianSNR, ClippingDistortion.  Semantics: DESIGN.md section 3
 * "Device-side augmentation", defined by tests/augment_ref.py.  Every stage acts on clip b over [0, lens[b]); the padding stays
 * zero; a stage that is off for a clip leaves that clip bit-identical.  All per-clip descriptors are DEVICE arrays of B entries.
 *
 * RIR convolution (replaces RIRAugmentation.__call__, tiny_audio/augmentation.py:71-93): uniformly partitioned overlap-save in f32,
 * hop TA_WAVE_CONV_HOP, complex FFT of 2 * TA_WAVE_CONV_HOP points in LDS.
 *   ta_wave_fft_twiddles: tw float[2 * TA_WAVE_CONV_HOP] = exp(-2 pi i k / N) as (re, im), k < N / 2, rounded once from float64.
 *   ta_wave_ir_spectra: the pool's partition spectra, computed ONCE per pool.  ir: the impulse responses back to back; response r
 *      is ir[ir_off[r] .. ir_off[r + 1]) (device long[n_ir + 1]) and owns partitions part_off[r] .. part_off[r + 1] (device
 *      int[n_ir + 1]; ceil(taps / hop) each); max_parts = the largest partition count; spectra: float[part_off[n_ir] * 2 *
 *      (TA_WAVE_CONV_HOP + 1)].
 *   ta_wave_conv_f32: out[b] = the convolution of clip b with response ir_idx[b] (>= 0), kept on [0, lens[b]) and scaled by
 *      rir_peak / max|full convolution| (rir_peak <= 0: no scaling) -- or the copy of wav[b] when ir_idx[b] < 0 (or ir_idx is
 *      NULL: every clip copied, no workspace needed).  max_taps = the longest response of the pool; ws: ta_wave_conv_ws_bytes
 *      bytes, no initial contents required; out must not alias wav.  Where the clip or the response has at most
 *      TA_WAVE_CONV_DIRECT samples the convolution is formed directly from ir (the same array ta_wave_ir_spectra read), each
 *      sample as a sum of <= TA_WAVE_CONV_DIRECT products in double, rounded once: cheaper than the transforms there, and exact
 *      to the last bit where a transform is not. */
#define TA_WAVE_CONV_HOP 2048
#define TA_WAVE_CONV_DIRECT 32
int ta_wave_fft_twiddles(float* tw, hipStream_t st);
int ta_wave_ir_spectra(const float* ir, const long* ir_off, const int* part_off, int n_ir, int max_parts, const float* tw,
                       float* spectra, hipStream_t st);
long ta_wave_conv_ws_bytes(int B, int Ls, int max_taps);
int ta_wave_conv_f32(const float* wav, const long* lens, int B, int Ls, const int* ir_idx, const float* ir, const long* ir_off,
                     const int* part_off, int n_ir, int max_taps, const float* tw, const float* spectra, float rir_peak,
                     float* out, void* ws, long ws_bytes, hipStream_t st);
/* Background noise at an SNR, then the Gaussian floor at an SNR, in place (replaces AddBackgroundNoise and AddGaussianSNR inside
 * NoiseAugmentation.__call__, tiny_audio/augmentation.py:154-185,218-223).  Clip b with noise_idx[b] = j >= 0 gets
 * x + (rms_x * noise_amp[b] / rms_v) v,  v[t] = noise_j[(noise_start[b] + t) mod len_j],  noise_amp = 10^(-snr_dB / 20), the rms
 * over [0, lens[b]); skipped when rms_v < 1e-9.  noise: the pool back to back, clip j = noise[noise_off[j] .. noise_off[j + 1]).
 * Then, where gauss_amp[b] > 0:  + rms * gauss_amp[b] * z[b, t]  with rms taken after the background stage and z the Philox4x32-10
 * Box-Muller normals of (seed, offset, b, t) documented in csrc/philox.h.  noise_idx / gauss_amp may be NULL (stage off everywhere).
 * scratch: float[ta_wave_mix_scratch_floats(B, Ls)], no initial contents required. */
long ta_wave_mix_scratch_floats(int B, int Ls);
int ta_wave_mix_f32(float* wav, const long* lens, int B, int Ls, const int* noise_idx, const long* noise_start,
                    const float* noise_amp, const float* noise, const long* noise_off, int n_noise, const float* gauss_amp,
                    unsigned long long seed, unsigned long long offset, float* scratch, hipStream_t st);
/* Percentile clipping in place (replaces ClippingDistortion inside NoiseAugmentation.__call__, tiny_audio/augmentation.py:190-195):
 * where pct[b] > 0, q = pct[b] / 2 (integer),  lo, hi = numpy.percentile(x[0:n], [q, 100 - q]) (linear interpolation),
 * x = clip(x, lo, hi).  The order statistics are found exactly by bisection on the ordered-integer image of the floats. */
int ta_wave_clip_f32(float* wav, const long* lens, int B, int Ls, const int* pct, hipStream_t st);
/* Short noises in place (replaces AddShortNoises inside NoiseAugmentation.__call__, tiny_audio/augmentation.py:172-177; it sits
 * between the background noise and the Gaussian floor).  Clip b has ev_count[b] <= min(ev_stride, TA_WAVE_MAX_EVENTS) events; the
 * descriptor arrays are [B, ev_stride].  Event e = the window [ev_off, ev_off + ev_len) of pool clip ev_pool (pool_off as noise_off
 * above; no tiling: the window lies inside the clip), laid at ev_t0 >= 0:
 *   y[t0 + i] += g a_in[i] a_out[i] v[i],  i < ev_len, t0 + i < lens[b];   g = R ev_amp / r,  ev_amp = 10^(-snr_dB / 20),
 *   R = rms of the stage's input over [0, lens[b]) taken once before any event, r = rms of the whole window before the fades (an
 *   event with r < 1e-9 is skipped);  a_in[i] = 10^(-(D / 20)(1 - (i + 1) / fade_in)) for i < fade_in, a_out[i] =
 *   10^(-(D / 20)(1 - (ev_len - i) / fade_out)) for i >= ev_len - fade_out, else 1;  D = fade_floor_db.
 * Overlapping events add in list order: no atomics, the result does not depend on launch order.  An event longer than
 * max_event_len (which sizes the scratch) or not inside its pool clip is skipped.
 * scratch: float[ta_wave_events_scratch_floats(B, Ls, ev_stride, max_event_len)], no initial contents required. */
#define TA_WAVE_MAX_EVENTS 64
long ta_wave_events_scratch_floats(int B, int Ls, int ev_stride, long max_event_len);
int ta_wave_events_f32(float* wav, const long* lens, int B, int Ls, const int* ev_count, int ev_stride, const int* ev_pool,
                       const long* ev_off, const long* ev_len, const long* ev_t0, const int* ev_fade_in, const int* ev_fade_out,
                       const float* ev_amp, const float* pool, const long* pool_off, int n_pool, long max_event_len,
                       float fade_floor_db, float* scratch, hipStream_t st);
/* A cascade of second-order sections in place (replaces SevenBandParametricEQ and OneOf{LowPassFilter, BandPassFilter} inside
 * NoiseAugmentation.__call__, tiny_audio/augmentation.py:186-215).  Clip b is filtered over [0, lens[b]) by its n_sec[b] <=
 * TA_WAVE_IIR_MAX_SECTIONS sections sos[b][k] = (b0, b1, b2, a1, a2), a0 = 1 (device double[B][TA_WAVE_IIR_MAX_SECTIONS][5]); a
 * first-order section has b2 = a2 = 0; n_sec[b] = 0 leaves the clip untouched.  The result is scipy.signal.sosfilt's in float64
 * from a zero state, rounded to f32 once per sample: the recurrence is carried in f64 and evaluated EXACTLY in parallel over time
 * (per chunk of `chunk` samples: the final state from zero; per clip: the chunk map of the 2 S states and the entry state of every
 * chunk; per chunk again: the run from its entry state).  chunk: 0 = TA_WAVE_IIR_CHUNK, else a multiple of 32; chunk >= Ls is the
 * sequential one-thread-per-clip form (for measurements).  The caller guarantees stable sections.
 * ws: ta_wave_sos_ws_bytes(B, Ls, chunk) bytes, no initial contents required. */
#define TA_WAVE_IIR_MAX_SECTIONS 8
#define TA_WAVE_IIR_CHUNK 256
long ta_wave_sos_ws_bytes(int B, int Ls, int chunk);
int ta_wave_sos_f32(float* wav, const long* lens, int B, int Ls, const int* n_sec, const double* sos, int chunk, void* ws,
                    long ws_bytes, hipStream_t st);

/* ---- forced alignment of CTC emissions against a token sequence, for word timestamps (tiny_audio_amd/csrc/align.hip).  Replaces
 * ForcedAligner._get_trellis and ._backtrack (tiny_audio/alignment.py:47-152), which the reference's pipeline calls per clip from
 * ForcedAligner.align (tiny_audio/alignment.py:213-286; seam at tiny_audio/asr_pipeline.py:117-131).  Contract: DESIGN.md section 3,
 * "Forced alignment", defined by tests/align_ref.py.  N clips in one launch, ragged:
 *   emission: f32 log-probabilities, clip n owns rows cu_frames[n] .. cu_frames[n + 1] (T_n of them) of [sum T_n, C], row stride ld;
 *   tokens:   int32 ids in [0, C), clip n owns tokens[cu_tokens[n] .. cu_tokens[n + 1]) (J_n of them); cu_* are int32[N + 1].
 * trellis[0, 0] = 0, every other entry -inf, then
 *   trellis[t + 1, j] = max(trellis[t, j] + emission[t, blank_id], trellis[t, j - 1] + emission[t, tokens[j - 1]])   (j = 0: first term)
 * with one f32 add per candidate.  Outputs per clip:
 *   score[n]  = trellis[T_n, J_n];
 *   status[n] = 0 aligned, 1 failed (score == -inf; the caller falls back to uniform spans), 2 refused: T_n > max_T, J_n > max_J,
 *               a negative length, or a token id outside [0, C) (nothing else of the clip is written);
 *   frames[cu_tokens[n] + i] = the frame of token i on the best path (ties between staying and moving go to moving, as the
 *               reference's `move >= stay`), strictly increasing in i; written ONLY for status 0, so token i spans (f, f + 1).
 * J_n = 0 gives status 0 and no frames; T_n = 0 < J_n gives status 1.
 * trellis_out (may be NULL): clip n's full [T_n + 1, J_n + 1] trellis is written at trellis_out + trellis_off[n] (device long[N]).
 * ws: ta_ctc_align_workspace_bytes(N, max_T, max_J) bytes holding the decision bits, no initial contents required; max_T / max_J
 * bound every clip's T_n / J_n.  Limits (TA_ERR_ARG beyond them): N <= TA_ALIGN_MAX_CLIPS, max_T <= TA_ALIGN_MAX_FRAMES,
 * max_J <= TA_ALIGN_MAX_TOKENS, C <= TA_ALIGN_MAX_CLASSES; also 0 <= blank_id < C <= ld. */
#define TA_ALIGN_MAX_TOKENS 2048
#define TA_ALIGN_MAX_FRAMES 32768
#define TA_ALIGN_MAX_CLASSES 65536
#define TA_ALIGN_MAX_CLIPS 4096
#define TA_ALIGN_THREADS 256      /* one workgroup per clip; a thread owns every 256th trellis column */
#define TA_ALIGN_FRAME_BLOCK 64   /* frames whose emissions are staged in LDS at a time ... */
#define TA_ALIGN_STAGE_FLOATS 8192 /* ... or fewer: min(TA_ALIGN_FRAME_BLOCK, TA_ALIGN_STAGE_FLOATS / (J_n + 1)), at least 3 */
long ta_ctc_align_workspace_bytes(int N, int max_T, int max_J);
int ta_ctc_align_f32(const float* emission, long ld, int C, const int* cu_frames, const int* tokens, const int* cu_tokens, int N,
                     int max_T, int max_J, int blank_id, int* frames, float* score, int* status, void* ws, long ws_bytes,
                     float* trellis_out, const long* trellis_off, hipStream_t st);

/* ---- forced alignment, long form: the same alignment for transcripts beyond TA_ALIGN_MAX_TOKENS and recordings beyond
 * TA_ALIGN_MAX_FRAMES (tiny_audio_amd/csrc/align_long.hip) -- the whole-recording call ForcedAligner.align(whole_audio, whole_text) of
 * the reference's pipeline (tiny_audio/asr_pipeline.py:117-131; trellis and walk tiny_audio/alignment.py:47-152).  Contract: that of
 * ta_ctc_align_f32 in every respect (tests/align_ref.py; DESIGN.md section 3, "Forced alignment", "Long form"): the same ragged
 * layout, the same f32 recurrence with one f32 add per candidate, ties to moving, the same status 0 / 1 / 2, frames strictly
 * increasing and written for status 0 only, score = trellis[T_n, J_n], J_n = 0 legal, trellis_out / trellis_off as there.  The
 * results are the reference's bytes, and on any clip inside the old envelope the bytes ta_ctc_align_f32 gives.
 * A clip's trellis is cut into tiles of col_block columns by frame_block frames (0 = the defaults below; col_block a multiple of 64
 * up to TA_ALIGN_LONG_MAX_COL_BLOCK, frame_block >= 1, else TA_ERR_ARG; the results do not depend on either).  Launch k runs every
 * tile (cb, fb) with cb + fb == k of every clip, one workgroup per tile; a tile's entering row and the column to its left reach it
 * through the workspace from the launch before, so ceil((max_J + 1) / col_block) + ceil(max_T / frame_block) - 1 tile launches on
 * `st`, one launch before them (the per-clip checks) and one after (the walk, one wave per clip) make the call.  No kernel waits
 * for another workgroup.
 * ws: ta_ctc_align_long_workspace_bytes(N, max_T, max_J, col_block, frame_block) bytes (-1 for a tiling that would be refused),
 * no initial contents required: the decision bits, max_T * ceil((max_J + 1) / 64) * 8 bytes per clip (1.35 GB for max_T = 180 000,
 * max_J = 60 000; 34 GB at the limits), and the two carries, (col_block + max_T) * ceil((max_J + 1) / col_block) floats per clip.
 * Limits (TA_ERR_ARG beyond them): N <= TA_ALIGN_LONG_MAX_CLIPS, max_T <= TA_ALIGN_LONG_MAX_FRAMES (5.8 h of 20 ms frames),
 * max_J <= TA_ALIGN_LONG_MAX_TOKENS, C <= TA_ALIGN_LONG_MAX_CLASSES; also 0 <= blank_id < C <= ld.
 * The trellis is f32, as the reference's is: at one hour |trellis| is around 2e5, where one ulp is about 0.016, so late decisions
 * between candidates closer than that are decided by rounding -- identically here and in the reference; nothing is renormalised. */
#define TA_ALIGN_LONG_MAX_TOKENS 262144
#define TA_ALIGN_LONG_MAX_FRAMES 1048576
#define TA_ALIGN_LONG_MAX_CLASSES 65536
#define TA_ALIGN_LONG_MAX_CLIPS 64
#define TA_ALIGN_LONG_MAX_COL_BLOCK 2048   /* a tile's two rows, column ids and staged emissions fit one workgroup's LDS */
#define TA_ALIGN_LONG_COL_BLOCK 256        /* the default tile: the best of those measured (profiles/forced_alignment.md) */
#define TA_ALIGN_LONG_FRAME_BLOCK 64
long ta_ctc_align_long_workspace_bytes(int N, int max_T, int max_J, int col_block, int frame_block);
int ta_ctc_align_long_f32(const float* emission, long ld, int C, const int* cu_frames, const int* tokens, const int* cu_tokens, int N,
                          int max_T, int max_J, int blank_id, int col_block, int frame_block, int* frames, float* score, int* status,
                          void* ws, long ws_bytes, float* trellis_out, const long* trellis_off, hipStream_t st);

/* ---- text alignment on the device: word / character error counts (WER, CER) and the LCS word matching of the reference's timestamp
 * evaluator (tiny_audio_amd/csrc/text_align.hip).  Replaces the O(n m) host loops behind jiwer.wer in the reference's evaluator
 * (scripts/eval/evaluators/base.py:114,150) and align_words_to_reference (scripts/eval/evaluators/alignment.py:12-79).  Contract:
 * DESIGN.md section 3, "Text alignment", defined by tests/text_align_ref.py.  N pairs in one call, ragged:
 *   ref: int32 symbol ids, pair p owns ref[cu_ref[p] .. cu_ref[p + 1]) (n_p of them); hyp / cu_hyp the same (m_p); cu_* are
 *   int32[N + 1].  Only equality of ids is used; any int32 value is legal.
 * mode TA_TEXT_ALIGN_EDIT: D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (r_i != h_j), D[i-1][j] + 1, D[i][j-1] + 1); the
 *   path from (n, m) steps diagonally if i, j > 0 and D[i][j] == D[i-1][j-1] + (r_i != h_j) (a hit if the symbols are equal, else a
 *   substitution), else up if i > 0 and D[i][j] == D[i-1][j] + 1 (a deletion), else left (an insertion).
 * mode TA_TEXT_ALIGN_LCS: L[i][j] = L[i-1][j-1] + 1 if r_i == h_j else max(L[i-1][j], L[i][j-1]); the path from (n, m), while
 *   i, j > 0, records a pair and steps diagonally if r_i == h_j, else steps up if L[i-1][j] > L[i][j-1], else left.
 * Outputs per pair (all int32; cells are int32):
 *   status[p] = 0 ok, 2 refused: n_p or m_p negative or beyond max_n / max_m, or (want_path) decision bits that do not fit ws;
 *               a refused pair gets dist -1 and nothing else of it is written;
 *   dist[p]   = D[n][m], or L[n][m];
 *   counts[p][4] = hits, substitutions, deletions, insertions (lcs: pairs, 0, n - pairs, m - pairs)            -- want_path only
 *   map[cu_ref[p] + i] = the hypothesis index of reference position i's diagonal step, -1 if deleted / unmatched -- want_path only
 * want_path = 0 writes status and dist only, needs no decision bits, and counts / map may be NULL.
 * Tiling: a tile is col_block hypothesis columns (64, 128, 256 or 512) by row_block reference rows (a multiple of 64), one wave per
 * tile.  col_block = row_block = 0 chooses: the short kernel (one workgroup per pair: fill and walk in one launch) when
 * max_m <= TA_TEXT_ALIGN_SHORT_MAX_M, else the long kernel with the default tile.  Any non-zero value asks for the long kernel (the
 * other one, if 0, takes its default): launch k runs every tile (cb, rb) with cb + rb == k of every pair, a tile's entering row and
 * the column to its left reach it through the workspace from the launch before, so ceil(max_m / col_block) +
 * ceil(max_n / row_block) - 1 tile launches on `st`, one before them (the per-pair checks) and, with want_path, one after (the walk,
 * one wave per pair).  No kernel waits for another workgroup.  Neither the kernel nor the tile changes an output byte.
 * ws: ta_text_align_workspace_bytes(cu_ref_host, cu_hyp_host, N, max_n, max_m, want_path, col_block, row_block) bytes (-1 for a
 * tiling that would be refused), no initial contents required.  The two cu_* arrays are HOST copies: the decision bits are sized
 * from the batch's actual pairs, sum over p of m_p * ceil(n_p / 64) * 16 bytes (two bits a cell; 268 MB for 32 768 x 32 768),
 * after a fixed part of 12 bytes a pair and, for the long kernel, the carries: max_m + max_n + ceil(max_n / row_block) ints a pair.
 * With want_path = 0 (or NULL cu_*) the fixed part is all.
 * Limits (TA_ERR_ARG beyond them): N <= TA_TEXT_ALIGN_MAX_PAIRS, max_n and max_m <= TA_TEXT_ALIGN_MAX_LEN (the transcript size
 * ta_ctc_align_long_f32 takes); mode and want_path 0 or 1. */
#define TA_TEXT_ALIGN_EDIT 0
#define TA_TEXT_ALIGN_LCS 1
#define TA_TEXT_ALIGN_MAX_LEN 262144
#define TA_TEXT_ALIGN_MAX_PAIRS 65536
#define TA_TEXT_ALIGN_MAX_COL_BLOCK 512    /* 64 lanes x 8 columns in registers */
#define TA_TEXT_ALIGN_SHORT_MAX_M 512      /* the short kernel: the hypothesis side fits one tile */
#define TA_TEXT_ALIGN_COL_BLOCK 256        /* the default tile of the long kernel (profiles/text_align.md) */
#define TA_TEXT_ALIGN_ROW_BLOCK 256
long ta_text_align_workspace_bytes(const int* cu_ref_host, const int* cu_hyp_host, int N, int max_n, int max_m, int want_path,
                                   int col_block, int row_block);
int ta_text_align_i32(const int* ref, const int* cu_ref, const int* hyp, const int* cu_hyp, int N, int max_n, int max_m, int mode,
                      int want_path, int col_block, int row_block, int* dist, int* counts, int* map, int* status, void* ws,
                      long ws_bytes, hipStream_t st);

/* ---- frozen wav2vec2-base CTC acoustic model: the front half of forced alignment (tiny_audio_amd/csrc/wav2vec2.hip).  Replaces the
 * torchaudio WAV2VEC2_ASR_BASE_960H forward + log_softmax the reference runs through PyTorch in ForcedAligner.align
 * (tiny_audio/alignment.py:206-211).  Arithmetic of Wav2Vec2ForCTC.forward (TF:models/wav2vec2/modeling_wav2vec2.py:1667-1700; feature encoder :382-419, projection :422-434,
 * encoder :657-727, layer :575-608) with
 * feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False, no attention mask, no input normalisation; inference only.
 * Every clip is processed as if alone (the reference aligns one unpadded clip at a time).  Contract: DESIGN.md section 3, "wav2vec2
 * acoustic model", defined by tests/wav2vec2_ref.py.
 * ta_enc_layer is reused with ln1_* = layer_norm (behind the attention residual), ln2_* = final_layer_norm, wo/bo = attention.out_proj,
 * w1/b1 = feed_forward.intermediate_dense, w2/b2 = feed_forward.output_dense, and wqkv_fa / bqkv_fa (REQUIRED) = q | k | v rows in
 * their natural order with the q rows and q bias multiplied by head_dim^-0.5 * log2(e); k keeps its bias.  wqkv / bqkv are not read. */
#define TA_W2V_HEAD_PAD 64   /* rows of the zero-padded lm_head image; n_classes <= 64 */
typedef struct {
  int hidden, ffn, n_layers, heads, conv_dim, n_classes;   /* hidden = 64 * heads, hidden and ffn multiples of 128, hidden / 16 a
                                                              multiple of 8 up to 64, conv_dim a multiple of 64 */
  float ln_eps;
  const float* conv0_w;        /* f32 [C, 10]: feature_extractor.conv_layers.0.conv.weight */
  const float *gn_w, *gn_b;    /* [C]: conv_layers.0.layer_norm (GroupNorm, C groups) */
  const void* conv_w[6];       /* conv_layers.1 .. 6: bf16 [C, k*C], column = tap*C + cin; k = 3,3,3,3,2,2, stride 2 */
  const float *fp_ln_w, *fp_ln_b;   /* [C]: feature_projection.layer_norm */
  const void* fp_w;            /* bf16 [H, C]: feature_projection.projection */
  const float* fp_b;
  const void* pos_w;           /* bf16 [16][NB*16][128*cg], cg = H/16, NB = ceil(cg/16): group g, output channel co (rows >= cg ZERO),
                                  column = tap*cg + cin -- pos_conv_embed.conv's weight with its weight norm folded */
  const float* pos_b;          /* [H] */
  const float *enc_ln_w, *enc_ln_b; /* encoder.layer_norm */
  const ta_enc_layer* layers;  /* host array [n_layers] */
  const void* head_w;          /* bf16 [TA_W2V_HEAD_PAD, H]: lm_head.weight, rows >= n_classes ZERO */
  const float* head_b;         /* [n_classes] */
  int res_f32;                 /* storage of the residual stream: 0 = bf16, 1 = fp32 (see the top of this file) */
} ta_wav2vec2_weights;

/* wav f32 [B, Ls] (clip b = its first lens[b] samples, 400 <= lens[b] <= Ls; the rest is never read) -> emissions f32
 * [rows, n_classes] log-probabilities, rows = sum of T_b with T_b = (lens[b] - 400) / 320 + 1 ((T - k) / s + 1 per conv layer), clip
 * b at rows cu_frames[b] .. cu_frames[b + 1]: the layout ta_ctc_align_f32 takes.  Rows past `rows` are not written.
 * lens_host: HOST int [B] (sets the launch geometry); lens_dev: the same on the DEVICE; cu_frames_dev: DEVICE int [B + 1] built by
 * the caller from the same lengths (the host cannot read it: a table that disagrees is not detected, as for
 * ta_encoder_forward_ragged).  ws: ta_wav2vec2_workspace_bytes(w, B, Ls, rows) bytes, no initial contents required; on return its
 * last rows * TA_W2V_HEAD_PAD floats (rounded up to 256 bytes) hold the lm_head GEMM's f32 output [rows, TA_W2V_HEAD_PAD], bias not added.
 * Kernel launches on st only: no allocation, copy or synchronisation. */
long ta_wav2vec2_workspace_bytes(const ta_wav2vec2_weights* w, int B, int Ls, long rows);
int ta_wav2vec2_forward(const ta_wav2vec2_weights* w, const float* wav, const int* lens_host, const int* lens_dev,
                        const int* cu_frames_dev, int B, int Ls, float* emissions, void* ws, long ws_bytes, hipStream_t st);

/* Its new kernels, exported for the tests.
 * Conv layer 0 (k 10, stride 5, no bias) + GroupNorm(C groups: per-channel statistics over the clip's own T0 = (len - 10) / 5 + 1
 * frames, biased variance, eps) + exact GELU: replaces Wav2Vec2GroupNormConvLayer.forward
 * (TF:models/wav2vec2/modeling_wav2vec2.py:302-323).  w f32 [C, 10]; out bf16 time-major, clip b's frame t at row b * out_rpb + t
 * (out_rpb >= (Ls - 10) / 5 + 1); rows t >= T0_b are not written.  The statistics are per-256-frame-chunk (mean, sum of squared
 * deviations from it) merged pairwise in f64; the conv is recomputed for the apply pass.  ws: ta_w2v_conv0_ws_bytes(B, Ls, C). */
long ta_w2v_conv0_ws_bytes(int B, int Ls, int C);
int ta_w2v_conv0_gn_gelu(const float* wav, const int* lens_dev, int B, int Ls, const float* w, const float* gn_w,
                         const float* gn_b, int C, float eps, void* out_bf16, long out_rpb, void* ws, long ws_bytes,
                         hipStream_t st);
/* y = x + gelu(pos_conv(x) + bias) with Conv1d(H, H, k = 128, padding = 64, groups = 16) and its last output frame dropped:
 * replaces Wav2Vec2PositionalConvEmbedding.forward and the add behind it (TF:models/wav2vec2/modeling_wav2vec2.py:326-379, :689-690).
 * x, y: [rows, H] in the stream's dtype (x_f32: 0 = bf16, 1 = f32), y != x; clip b owns rows cu_rows[b] .. cu_rows[b + 1] and meets
 * zeros outside them; max_rows = the longest clip (sizes the grid).  wp / bias: ta_wav2vec2_weights.pos_w / pos_b.  H / 16 must be
 * a multiple of 8 up to 64 (TA_ERR_ARG otherwise).  bf16 MFMA operands, f32 accumulation. */
int ta_w2v_pos_conv(const void* x, int x_f32, const void* wp, const float* bias, void* y, const int* cu_rows, int B,
                    int max_rows, int H, hipStream_t st);
/* out [rows, n_classes] = log_softmax(logits[:, :n_classes] + bias) in f32, logits f32 [rows, ld] (the lm_head GEMM at its padded
 * width; columns >= n_classes never enter): replaces lm_head's bias add and torch.log_softmax (tiny_audio/alignment.py:206-211,
 * TF:models/wav2vec2/modeling_wav2vec2.py:1700).  1 <= n_classes <= TA_W2V_HEAD_PAD, ld >= n_classes. */
int ta_w2v_head_logsoftmax(const float* logits, long ld, const float* bias, int n_classes, float* out, int rows,
                           hipStream_t st);

/* ---- the "layer-norm / stable" wav2vec2 family (wav2vec2-large-960h-lv60(-self), XLSR-53 and XLS-R 300M fine-tunes, MMS 300M /
 * torchaudio's MMS_FA): Wav2Vec2ForCTC.forward with feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, eager
 * attention, no attention mask, optional input normalisation; inference only, every clip as if alone.  Against the base model:
 * every conv layer is conv + bias -> LayerNorm over the CHANNELS of a frame (affine, nn.LayerNorm's default eps 1e-5, NOT ln_eps) ->
 * exact GELU (Wav2Vec2LayerNormConvLayer); the encoder adds the positional conv with no LayerNorm behind it, runs pre-LN layers
 * x += out_proj(attn(layer_norm(x))), x += ffn(final_layer_norm(x)) (Wav2Vec2EncoderLayerStableLayerNorm) and applies
 * encoder.layer_norm behind the last one (Wav2Vec2EncoderStableLayerNorm).  Contract: DESIGN.md section 3, "wav2vec2 acoustic model:
 * the layer-norm / stable family", defined by tests/wav2vec2_sln_ref.py.  ta_enc_layer as for ta_wav2vec2_weights (ln1_* =
 * layer_norm, now IN FRONT of the attention; ln2_* = final_layer_norm, in front of the feed-forward).
 * Not built, refused with TA_ERR_ARG: conv_dim other than 64 / 128 / 256 / 512, head_dim != 64 (XLS-R 1B / 2B), more than
 * TA_W2V_HEAD_PAD classes; adapter layers (MMS adapter_attn_dim) and the two mixed configurations have no field here at all. */
typedef struct {
  int hidden, ffn, n_layers, heads, conv_dim, n_classes;   /* as ta_wav2vec2_weights; conv_dim in {64, 128, 256, 512} */
  float ln_eps;                /* feature_projection.layer_norm, the layers' norms and encoder.layer_norm */
  float input_norm_eps;        /* > 0: each clip's samples become (x - mean) / sqrt(var + eps), biased variance over the clip's own
                                  samples (1e-7: Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm; 1e-5: torchaudio's
                                  layer_norm(waveform, waveform.shape)); 0: the raw waveform goes in */
  const float* conv0_w;        /* f32 [C, 10]: conv_layers.0.conv.weight */
  const float* conv_b[7];      /* [C]: conv_layers.l.conv.bias */
  const float *conv_ln_w[7], *conv_ln_b[7];   /* [C]: conv_layers.l.layer_norm */
  const void* conv_w[6];       /* conv_layers.1 .. 6: bf16 [C, k*C], column = tap*C + cin */
  const float *fp_ln_w, *fp_ln_b;
  const void* fp_w;            /* bf16 [H, C] */
  const float* fp_b;
  const void* pos_w;           /* the packed image of ta_wav2vec2_weights.pos_w */
  const float* pos_b;
  const float *enc_ln_w, *enc_ln_b; /* encoder.layer_norm (behind the LAST layer) */
  const ta_enc_layer* layers;  /* host array [n_layers] */
  const void* head_w;          /* bf16 [TA_W2V_HEAD_PAD, H], rows >= n_classes ZERO */
  const float* head_b;         /* [n_classes] */
  int res_f32;
} ta_wav2vec2_sln_weights;

/* Same arguments, layouts and workspace tail (the lm_head GEMM's f32 output) as ta_wav2vec2_forward.  Replaces
 * TF:models/wav2vec2/modeling_wav2vec2.py Wav2Vec2LayerNormConvLayer.forward, Wav2Vec2EncoderStableLayerNorm.forward,
 * Wav2Vec2EncoderLayerStableLayerNorm.forward and lm_head; with input_norm_eps > 0 also
 * feature_extraction_wav2vec2.py zero_mean_unit_var_norm on each unpadded clip. */
long ta_wav2vec2_sln_workspace_bytes(const ta_wav2vec2_sln_weights* w, int B, int Ls, long rows);
int ta_wav2vec2_sln_forward(const ta_wav2vec2_sln_weights* w, const float* wav, const int* lens_host, const int* lens_dev,
                            const int* cu_frames_dev, int B, int Ls, float* emissions, void* ws, long ws_bytes, hipStream_t st);
/* For the per-stage tests: byte offsets inside that workspace of (feat) the feature extractor's output on the compact rows, bf16
 * [rows, conv_dim], and (stream) the residual stream behind the last layer, [rows, hidden] in the stream's dtype -- behind the
 * positional-conv add when n_layers = 0.  HOST pointers; no launch. */
int ta_wav2vec2_sln_ws_offsets(const ta_wav2vec2_sln_weights* w, int B, int Ls, long rows, long* feat_off, long* stream_off);

/* Its new kernels, exported for the tests.
 * Input normalisation: out[b, i] = (wav[b, i] - mean_b) / sqrt(var_b + eps) for i < lens[b] (clipped to Ls), statistics over the
 * clip's own samples with the biased variance; samples behind a clip's end are neither read nor written; out may be wav.  Per
 * 4096-sample chunk (mean, sum of squared deviations from it) in f32, merged pairwise in f64 -- never E[x^2] - E[x]^2.  A silent
 * clip gives zeros.  wav, out f32 [B, Ls]; ws: ta_w2v_input_norm_ws_bytes(B, Ls) bytes; eps > 0. */
long ta_w2v_input_norm_ws_bytes(int B, int Ls);
int ta_w2v_input_norm(const float* wav, const int* lens_dev, int B, int Ls, float eps, float* out, void* ws, long ws_bytes,
                      hipStream_t st);
/* Conv layer 0 (k 10, stride 5) + bias + LayerNorm over the C channels of each frame (biased variance, eps) + exact GELU in ONE
 * kernel: replaces Wav2Vec2LayerNormConvLayer.forward for layer 0.  Same output contract as ta_w2v_conv0_gn_gelu: out bf16
 * time-major, clip b's frame t at row b * out_rpb + t (out_rpb >= (Ls - 10) / 5 + 1), rows t >= T0_b not written.  One wave per
 * frame, a lane owning C / 64 contiguous channels; mean first, then squared deviations from it; no workspace.
 * C in {64, 128, 256, 512} (TA_ERR_ARG otherwise). */
int ta_w2v_conv0_ln_gelu(const float* wav, const int* lens_dev, int B, int Ls, const float* w, const float* bias, const float* ln_w,
                         const float* ln_b, int C, float eps, void* out_bf16, long out_rpb, hipStream_t st);
/* y = gelu(LayerNorm(x)) row by row, bf16 [M, H] -> bf16 [M, H], y != x: ta_layernorm_bf16's kernels with exact-erf GELU as their
 * output activation -- the LayerNorm + GELU behind conv layers 1 .. 6 (Wav2Vec2LayerNormConvLayer.forward) as one pass over the rows.
 * A row of NaN stays in its row.  H as ta_layernorm_bf16 takes it. */
int ta_layernorm_gelu_bf16(const void* x_bf16, const float* w, const float* b, void* y_bf16, int M, int H, float eps,
                           hipStream_t st);

/* ---- frozen ECAPA-TDNN speaker-embedding model: the hot path of speaker diarization (tiny_audio_amd/csrc/ecapa.hip).  Replaces the
 * loop of the reference's LocalSpeakerDiarizer._extract_embeddings, which reflect-pads every 0.75 s window and pushes it through
 * SpeechBrain's spkrec-ecapa-voxceleb encode_batch ONE WINDOW PER CALL (tiny_audio/diarization.py:457-517; the call itself :490-502).
 * Arithmetic: the published ECAPA-TDNN at that checkpoint's hyper-parameters behind SpeechBrain's Fbank (n_fft 400, hop 160, Hamming,
 * 80 mel, top_db 80) and sentence-mean normalisation; eval-mode BatchNorm folded to (scale, shift) BEHIND each ReLU.  Every window is
 * processed as if alone.  Contract: DESIGN.md section 3, "Speaker diarization", defined by tests/ecapa_ref.py. */
#define TA_ECAPA_N_MELS 80
#define TA_ECAPA_FEAT_STRIDE 128   /* channel stride of the bf16 feature slab (80 mel + 48 zeros): block0's K = 5 * 128 = 640 */
#define TA_ECAPA_SCALE 8           /* Res2Net sub-bands */
#define TA_ECAPA_MIN_T 5           /* frames per window, T = window_samples / 160 + 1: the reflect padding of 4 needs 5 */
#define TA_ECAPA_MAX_T 512
#define TA_ECAPA_MAX_DILATION 4
#define TA_ECAPA_MAX_CHANNELS 1024 /* C: a multiple of 128 (sub-band width C / 8 a multiple of 16 up to 128) */
#define TA_ECAPA_MAX_SE 256
#define TA_ECAPA_MAX_ATTN 256      /* attention channels: a multiple of 64 */
#define TA_ECAPA_MAX_EMB 1024      /* embedding width: a multiple of 4 */
typedef struct {
  const void* w1;              /* bf16 [C, C]: tdnn1.conv */
  const float *b1, *bn1_s, *bn1_t;      /* [C]: its bias, and tdnn1.norm folded: scale = g / sqrt(var + eps), shift = b - mean * scale */
  const void* res_w;           /* bf16 [7][C/8][Kp], Kp = 3 C/8 rounded up to 32: res2net conv m, output channel co, column = tap * C/8 + cin,
                                  columns >= 3 C/8 ZERO */
  const float *res_b, *res_s, *res_t;   /* [7 * C/8]: bias, folded norm of res2net conv m at m * C/8 */
  const void* w2;              /* bf16 [C, C]: tdnn2.conv */
  const float *b2, *bn2_s, *bn2_t;
  const float *se_w1t, *se_b1; /* f32 [C, se] (se_block.conv1 weight TRANSPOSED), [se] */
  const float *se_w2t, *se_b2; /* f32 [se, C] (se_block.conv2 weight TRANSPOSED), [C] */
  int dilation;                /* 1 .. TA_ECAPA_MAX_DILATION */
} ta_ecapa_block;
typedef struct {
  int channels, se_channels, attn_channels, emb_dim;
  const float* fb_window;      /* f32 [400] periodic Hamming */
  const float* fb_twiddle;     /* f32 [400][2] = cos(2 pi j / 400), -sin(2 pi j / 400) */
  const float* fb_mel;         /* f32 [201, 80] triangular filters, bin-major */
  const int* fb_mel_range;     /* int [80][2]: first / end bin of every filter's non-zero taps */
  const void* w0;              /* bf16 [C, 5 * TA_ECAPA_FEAT_STRIDE]: blocks.0.conv, column = tap * stride + mel, columns of mel >= 80 ZERO */
  const float *b0, *bn0_s, *bn0_t;
  ta_ecapa_block blocks[3];
  const void* mfa_w;           /* bf16 [3C, 3C] */
  const float *mfa_b, *mfa_s, *mfa_t;
  const void* att_wh;          /* bf16 [A, 3C]: asp.tdnn.conv columns 0 .. 3C (the frames' share) */
  const void* att_wms;         /* bf16 [A, 6C]: its columns 3C .. 9C (the window mean and std's share) */
  const float *att_b, *att_s, *att_t;   /* [A] */
  const void* att_conv_w;      /* bf16 [3C, A]: asp.conv */
  const float* att_conv_b;     /* [3C] */
  const float *aspbn_s, *aspbn_t;       /* [6C]: asp_bn folded */
  const void* fc_w;            /* bf16 [D, 6C] */
  const float* fc_b;           /* [D] */
} ta_ecapa_weights;

/* audio f32 [n_audio] (one shared buffer, uploaded once); window i = samples starts[i] .. starts[i] + lens[i], extended on the right
 * to window_samples by reflection while it is read (sample len + j = sample len - 2 - j: numpy's mode="reflect",
 * tiny_audio/diarization.py:484-488) -> emb f32 [N, emb_dim].  starts_host / lens_host: HOST int [N] (checked: 1 <= len <=
 * window_samples, window_samples - len <= len - 1 as np.pad demands, start + len <= n_audio; else TA_ERR_ARG); starts_dev / lens_dev:
 * the same on the DEVICE.  T = window_samples / 160 + 1 frames, TA_ECAPA_MIN_T <= T <= TA_ECAPA_MAX_T.  The windows go through in
 * chunks of chunk_windows; ws: ta_ecapa_workspace_bytes(w, min(N, chunk_windows), T) bytes, no initial contents required.  Window i's
 * embedding does not depend on the other windows or on the chunking.  Kernel launches on st only. */
long ta_ecapa_workspace_bytes(const ta_ecapa_weights* w, int n_windows, int T);
int ta_ecapa_forward(const ta_ecapa_weights* w, const float* audio, long n_audio, const int* starts_host, const int* lens_host,
                     const int* starts_dev, const int* lens_dev, int N, int window_samples, int chunk_windows, float* emb,
                     void* ws, long ws_bytes, hipStream_t st);

/* Its new kernels, exported for the tests.
 * Filter bank + sentence-mean normalisation (replaces the compute_features / mean_var_norm front of encode_batch,
 * tiny_audio/diarization.py:490-502): feat f32 [N, T, 80] = 10 log10(max(mel power, 1e-10)) floored at the window's own maximum
 * - 80 dB, minus each mel bin's mean over the T frames; slab bf16 [N, T + 4, TA_ECAPA_FEAT_STRIDE]: the same values rounded, frames at
 * rows 2 .. T + 1, rows 1, 0 = frames 1, 2 and rows T + 2, T + 3 = frames T - 2, T - 3 (block0's reflect padding), channels >= 80
 * zero.  The starts / lens are trusted (ta_ecapa_forward checks its host copies); a sample outside the audio buffer reads as 0. */
int ta_ecapa_fbank(const float* audio, long n_audio, const int* starts_dev, const int* lens_dev, int N, int window_samples,
                   const float* fb_window, const float* fb_twiddle, const float* fb_mel, const int* fb_mel_range,
                   float* feat, void* slab_bf16, hipStream_t st);
/* The Res2Net chain of one SERes2NetBlock on MFMA (replaces Res2NetBlock.forward inside encode_batch, tiny_audio/diarization.py:490-502).
 * z1 bf16: tdnn1's PRE-activation rows, window n's frame t at row n * z_rpw + t, ldz elements apart; y bf16 likewise (y_rpw, ldy):
 * y[:, 0:w] = x_0, y[:, i w:(i+1) w] = TDNN_{i-1}(x_i + y_{i-1}) with x_i = relu(z1_i) * bn1_s + bn1_t and the operand x_i + y_{i-1}
 * rounded to bf16 once.  Rows t >= T of a window and columns >= 8 w are neither read nor written.  w a multiple of 16 up to 128,
 * dilation 1 .. TA_ECAPA_MAX_DILATION, T > dilation; ldz, ldy multiples of 8; z1, y 16-byte aligned. */
int ta_ecapa_res2net(const void* z1, long ldz, long z_rpw, const float* bn1_s, const float* bn1_t, const void* res_w,
                     const float* res_b, const float* res_s, const float* res_t, void* y, long ldy, long y_rpw, int N, int T,
                     int w, int dilation, hipStream_t st);
/* out bf16 [N T, Cw] = relu(z) * scale + shift from a GEMM's pre-activation bf16 output (the ReLU and BatchNorm of a TDNNBlock,
 * tiny_audio/diarization.py:490-502).  With stats_f32 and / or stats_bf16 (else NULL): [N, 2 Cw] = each window's mean over time and
 * sqrt(max(biased variance, 1e-12)) of the rounded output, two passes (the global statistics of attentive pooling). */
int ta_ecapa_relu_bn(const void* z, const float* scale, const float* shift, void* out, float* stats_f32, void* stats_bf16,
                     int N, int T, int Cw, hipStream_t st);
/* out[:, 0:Cw] (rows ldout apart) = (relu(z2) * bn2_s + bn2_t) * gate + residual (rows ldres apart), gate = sigmoid(W2 relu(W1 m + b1)
 * + b2) with m the window's mean over time of relu(z2) * bn2_s + bn2_t: the SEBlock and the residual add of SERes2NetBlock.forward.
 * ws: f32 [ta_ecapa_se_ws_floats(N, Cw)]; on return its first N Cw floats hold m, the next N Cw the gate. */
long ta_ecapa_se_ws_floats(int N, int Cw);
int ta_ecapa_se_residual(const void* z2, const float* bn2_s, const float* bn2_t, const float* se_w1t, const float* se_b1,
                         const float* se_w2t, const float* se_b2, const void* residual, long ldres, void* out, long ldout,
                         int N, int T, int Cw, int se, float* ws, hipStream_t st);
/* out bf16 [N T, A] = tanh(relu(g + per_window[window]) * scale + shift): asp.tdnn's activation with the window-constant share of its
 * convolution added (AttentiveStatisticsPooling.forward).  g f32 [N T, A], per_window f32 [N, A]. */
int ta_ecapa_attn_act(const float* g, const float* per_window, const float* scale, const float* shift, void* out, int N, int T,
                      int A, hipStream_t st);
/* Attentive statistics pooling: a = softmax over the window's T frames of logits f32 [N T, Cw] per channel; out bf16 [N, 2 Cw] =
 * ([sum a h | sqrt(max(sum a (h - mean)^2, 1e-12))]) * aspbn_s + aspbn_t, h bf16 [N T, Cw].  attn_w f32 [N T, Cw] / pooled_f32
 * [N, 2 Cw] (before asp_bn): optional outputs, or NULL. */
int ta_ecapa_asp_pool(const float* logits, const void* h, const float* aspbn_s, const float* aspbn_t, void* out, float* attn_w,
                      float* pooled_f32, int N, int T, int Cw, hipStream_t st);

/* ---- speaker clustering: the spectral embedding behind the window embeddings (tiny_audio_amd/csrc/cluster.hip).  Replaces the dense
 * float64 host chain of the reference's SpectralCluster -- cosine_similarity, argpartition pruning, symmetrisation, the Laplacian and
 * scipy.linalg.eigh of the whole [N, N] matrix (tiny_audio/diarization.py:49-106) -- by f32 kernels and a block Lanczos iteration that
 * tiny_audio_amd/spectral.py drives over them.  Everything is f32 in and out, row-major with explicit leading dimensions (in elements);
 * no floating-point atomics: equal inputs give equal bits.  Contract: DESIGN.md section 3, "Spectral clustering", defined by
 * tests/cluster_ref.py. */
#define TA_SPK_MIN_N 6        /* fewer rows are one speaker on the host (SpeakerClusterer) */
#define TA_SPK_MAX_N 32768    /* a row of the affinity has to fit in LDS: 82 minutes of pure speech at STEP_SIZE 0.15 */
#define TA_SPK_MAX_D 256      /* embedding width (the checkpoint's is 192) */
#define TA_SPK_MAX_P 32       /* columns of a block the Laplacian is applied to, of a panel that is updated or combined */
#define TA_SPK_MAX_COLS 1024  /* columns of the Krylov basis */
/* E [N, D] -> W [N, N] (leading dimension ldw >= N) and deg [N]: get_sim_mat, p_pruning, 0.5 (P + P^T), fill_diagonal(0) and the row
 * sums of the Laplacian (tiny_audio/diarization.py:49-86).  phases is a mask, 7 = all of it in order:
 *   1  rows of E normalised (a zero row stays zero), S = E^ E^T with f32 accumulation; S[i, j] and S[j, i] are bitwise equal
 *   2  every row of W keeps its `keep` largest entries (1 <= keep <= N; the diagonal counts), the others become 0; entries equal to the
 *      keep-th largest are kept lowest column first until exactly `keep` survive.  kept_count int [N] (or NULL): the survivors per row
 *   4  W = 0.5 (W + W^T), diagonal 0, deg[i] = sum_j W[i, j] in a fixed order
 * ws: f32 [ta_spk_affinity_ws_floats(N, D)], 16-byte aligned, needed by phase 1 only.  Columns N .. ldw of W are never touched. */
long ta_spk_affinity_ws_floats(int N, int D);
int ta_spk_affinity_f32(const float* E, int N, int D, int keep, float* W, long ldw, float* deg, int* kept_count, float* ws, int phases,
                        hipStream_t st);
/* Y [N, p] = diag(deg) X - W X, the unnormalised Laplacian (tiny_audio/diarization.py:87-89) applied to a block X [N, p],
 * 1 <= p <= TA_SPK_MAX_P, without forming it: one pass over W.  ws: f32 [ta_spk_lapmul_ws_floats(N, p)].  X != Y.  W is read 16 bytes
 * per lane when ldw is a multiple of 4 and W is 16-byte aligned, 4 bytes otherwise. */
long ta_spk_lapmul_ws_floats(int N, int p);
int ta_spk_laplacian_matmul_f32(const float* W, long ldw, const float* deg, const float* X, long ldx, float* Y, long ldy, int N, int p,
                                float* ws, hipStream_t st);
/* Panel algebra of the Krylov basis that replaces scipy.linalg.eigh (tiny_audio/diarization.py:91-106).  C [a, b] = A^T B for
 * A [N, a], B [N, b], a, b <= TA_SPK_MAX_COLS; ws: f32 [ta_spk_gram_ws_floats(N, a, b)]. */
long ta_spk_gram_ws_floats(int N, int a, int b);
int ta_spk_panel_gram_f32(const float* A, long lda, int a, const float* B, long ldb, int b, int N, float* C, long ldc, float* ws,
                          hipStream_t st);
/* B [N, b] -= A [N, a] C [a, b], b <= TA_SPK_MAX_P, summed in increasing k (one Gram-Schmidt sweep against the basis). */
int ta_spk_panel_update_f32(float* B, long ldb, int b, const float* A, long lda, int a, const float* C, long ldc, int N, hipStream_t st);
/* Y [N, m] = V [N, c] Z [c, m], m <= TA_SPK_MAX_P (Ritz vectors; a block times the inverse of its Cholesky factor).  Y != V. */
int ta_spk_panel_combine_f32(const float* V, long ldv, int c, const float* Z, long ldz, int m, float* Y, long ldy, int N, hipStream_t st);

/* ---- long-form segmentation: where to cut a whole recording into encoder windows, at pauses and never beyond the window, and the cut
 * itself (tiny_audio_amd/csrc/segment.hip; driven by tiny_audio_amd/longform.py).  The reference has no counterpart: its
 * ASRPipeline.postprocess keeps the first chunk only (tiny_audio/asr_pipeline.py:243-245).  Contract: DESIGN.md section 3, "Long-form
 * transcription", defined by tests/segment_ref.py.  R recordings in one flat f32 buffer `wav`, recording r at samples
 * offsets[r] .. offsets[r + 1] (device long[R + 1]); n = its length, T = ceil(n / TA_CUT_HOP); its grid has the positions p = 0 .. T,
 * p standing for sample TA_CUT_HOP p and T for sample n.  max_n bounds every n (it sizes the workspaces and the rows: ld >= max_T + 1
 * with max_T = ceil(max_n / TA_CUT_HOP)); a recording with n < 1 or n > max_n is refused: its rows are not written and its n_seg is -1.
 * Limits (TA_ERR_ARG beyond them): R <= TA_CUT_MAX_RECORDINGS, max_T <= TA_CUT_MAX_POSITIONS (2.9 h), 0 <= h <= TA_CUT_MAX_SMOOTH,
 * 1 <= min_len, 2 min_len <= max_len <= TA_CUT_MAX_LEN, max_T / min_len <= TA_CUT_MAX_BLOCKS, cut_penalty finite and >= 0.
 *
 * ta_wave_cut_cost_f32: cost [R, ld] f32, for p = 0 .. T of every recording
 *   pw[p]   = (1 / 400) sum_{i = -200}^{199} x[160 p + i]^2                 samples outside [0, n) count as 0
 *   s[p]    = (1 / (2 h + 1)) sum_{q = p - h}^{p + h} pw[q]                 positions outside [0, T] count as 0; the divisor is fixed
 *   cost[p] = s[p] + cut_penalty * (1 / n) sum x^2
 * in f32, every term non-negative, in the fixed order written beside the kernels: no atomics, no workgroup waits for another, two runs
 * give the same bits, zeros cost exactly 0.  |cost - exact| <= gamma_K cost with K = TA_CUT_COST_K(h), gamma_K = K u / (1 - K u),
 * u = 2^-24: K is the longest chain of additions + 3, which is 2 h + 25 through s[p] and 65 through the mean power at the cap
 * (a blocked reduction: 128 positions per workgroup, then one workgroup per recording).
 * ws: ta_wave_cut_cost_workspace_bytes(R, max_n) bytes, no initial contents required (0 for arguments that would be refused).
 *
 * ta_cut_plan_f32: the cheapest set of cuts with every window between min_len and max_len positions, one workgroup per recording:
 *   dp[0] = 0;  dp[p] = (p < T ? cost[p] : 0) + min{dp[s] : max(0, p - max_len) <= s <= p - min_len}    for p = 1 .. T, one f32 add
 *   back[p] = the LOWEST s that attains the minimum; dp[p] = +inf and back[p] = -1 where the range is empty (back[0] = -1)
 * back int32 [R, ld] is written for p = 0 .. T.  cuts int32 [R, ldc] receives cuts[0] = 0 < ... < cuts[n_seg] = T, the walk of back[]
 * from T; n_seg int32 [R]; dp_T f32 [R] = dp[T].  ldc >= max_T / min_len + 2.  T < min_len: the single window {0, T}, n_seg = 1,
 * dp_T = 0 (back[] still holds the recurrence's -1).  With 2 min_len <= max_len a plan exists for every T >= min_len; n_seg = -1 is
 * left only where the walk breaks (non-finite costs).  The workgroup runs ceil(T / min_len) blocks of min_len positions one after the
 * other, two barriers each (13 ns per position at min_len = 1000; a small min_len makes a long recording one long kernel, hence
 * TA_CUT_MAX_BLOCKS: at the cap of positions min_len must be at least 8).
 *
 * ta_wave_windows_f32: out f32 [W, Ls] row w = wav[start[w] .. start[w] + len[w]) then zeros, lens long [W] = len[w] clamped to
 * [0, Ls]: the input contract of ta_logmel_f32.  start long [W] indexes the flat buffer of `total` samples, len int32 [W]; samples
 * outside [0, total) are never read (they come out as 0).  16-byte stores when Ls is a multiple of 4 and out is 16-byte aligned;
 * 16-byte loads where a source quad is aligned, 4-byte loads otherwise.  W <= TA_WAVE_WINDOWS_MAX. */
#define TA_CUT_HOP 160
#define TA_CUT_POWER_WINDOW 400
#define TA_CUT_MAX_POSITIONS 1048576
#define TA_CUT_MAX_LEN 3000
#define TA_CUT_MAX_SMOOTH 64
#define TA_CUT_MAX_RECORDINGS 64
#define TA_CUT_MAX_BLOCKS 131072
#define TA_CUT_COST_K(h) (2 * (h) + 25 > 65 ? 2 * (h) + 25 : 65)
#define TA_WAVE_WINDOWS_MAX 65535
long ta_wave_cut_cost_workspace_bytes(int R, long max_n);
int ta_wave_cut_cost_f32(const float* wav, const long* offsets, int R, long max_n, int h, float cut_penalty, float* cost, long ld,
                         void* ws, long ws_bytes, hipStream_t st);
int ta_cut_plan_f32(const float* cost, long ld, const long* offsets, int R, long max_n, int min_len, int max_len, int* back, int* cuts,
                    long ldc, int* n_seg, float* dp_T, hipStream_t st);
int ta_wave_windows_f32(const float* wav, long total, const long* start, const int* len, int W, int Ls, float* out, long* lens,
                        hipStream_t st);

/* ---- voice activity detection: per-frame speech decisions of whole recordings, model-free (tiny_audio_amd/csrc/vad.hip; driven by
 * tiny_audio_amd/vad.py).  The reference takes its decisions from TEN-VAD, a compiled third-party library
 * (tiny_audio/diarization.py:370-387); this is a statistical detector of its own, not a restatement of that model.  Contract: DESIGN.md
 * section 3, "Voice activity detection", defined by tests/vad_ref.py.  The ragged layout of the segmentation block: R recordings in one
 * flat f32 buffer `wav`, recording r at samples offsets[r] .. offsets[r + 1] (device long[R + 1]), starting at any sample; x[k] = 0
 * outside [0, n) of a recording, whatever lies beside it.  The grid is the diarizer's: frame i for every i >= 0 with
 * TA_VAD_HOP i < n - TA_VAD_HOP, F = ta_vad_frames(n) = (n - 1) / TA_VAD_HOP of them, 0 for n <= TA_VAD_HOP (which is legal).
 * With h = smooth, W = noise_window, beta = noise_bias, theta = threshold, e0 = floor:
 *   y[m]    = w[m] x[256 i - 72 + m], m = 0 .. 399          w the periodic Hann window of 400: the window is centred on the frame
 *   P[i][f] = |DFT400(y)[f]|^2 / 400^2                       f = 2 .. 97
 *   E[i][b] = sum_{f = 2 + 6 b}^{7 + 6 b} P[i][f]            b = 0 .. 15: 16 bands of 240 Hz, 80 Hz .. 3.92 kHz
 *   S[i][b] = mean of E[j][b] over max(0, i - h) <= j <= min(F - 1, i + h)        the divisor counts the frames inside the grid
 *   N[i][b] = min of S[j][b] over max(0, i - W) <= j <= min(F - 1, i + W)
 *   g = (S + e0) / (beta N + e0),  t = g - 1 - ln g where g > 1, else 0,  L[i] = (1 / 16) sum_b t[i][b],  flag[i] = L[i] > theta
 * in f32 and in a fixed order: the 6 bins of a band ascending (scaled by 1 / 400^2 after the sum), the at most 2 h + 1 frames of S
 * ascending, (g - 1) - ln g, the 16 bands ascending.  No atomics, no workgroup waits for another; two runs give the same bits and a
 * recording gives the same bits alone as inside a batch.  Zeros give L = 0 exactly.  A non-finite sample makes L NaN (flag 0) on every
 * frame within W + h frames of one whose window holds it (or of the frame 2 j / 2 j + 1 that shares its transform): a NaN wins the
 * minimum.
 * Outputs: stat f32 [R, ld] = L, flags unsigned char [R, ld], ld >= ta_vad_frames(max_n); positions >= F of a row are not written.
 * n_frames int [R] = F; a recording with n < 0 or n > max_n is refused: n_frames -1 and its rows are not written.
 * Limits (TA_ERR_ARG beyond them): R <= TA_CUT_MAX_RECORDINGS, 1 <= max_n <= TA_CUT_HOP * TA_CUT_MAX_POSITIONS (2.9 h),
 * 0 <= smooth <= TA_VAD_MAX_SMOOTH, 1 <= noise_window <= TA_VAD_MAX_NOISE_WINDOW, noise_bias >= 1, threshold > 0, floor > 0, all finite.
 * ws: ta_vad_workspace_bytes(R, max_n) bytes (E, 64 bytes per frame), no initial contents required; 0 for arguments that would be
 * refused, and for max_n <= TA_VAD_HOP, where ws, stat and flags may be NULL.  Two launches: the band energies (TA_VAD_ENERGY_FRAMES
 * frames per workgroup, two real frames per complex transform) and the fused statistic (TA_VAD_TILE frames per workgroup plus a halo of
 * W + h frames per side). */
#define TA_VAD_HOP 256
#define TA_VAD_LEAD 72
#define TA_VAD_BANDS 16
#define TA_VAD_BAND_BINS 6
#define TA_VAD_FIRST_BIN 2
#define TA_VAD_MAX_SMOOTH 8
#define TA_VAD_MAX_NOISE_WINDOW 1024
#define TA_VAD_ENERGY_FRAMES 32
#define TA_VAD_TILE 256
typedef struct { int smooth; int noise_window; float noise_bias; float threshold; float floor; } ta_vad_options;
long ta_vad_frames(long n);
long ta_vad_workspace_bytes(int R, long max_n);
int ta_vad_f32(const float* wav, const long* offsets, int R, long max_n, const ta_vad_options* opt, float* stat, unsigned char* flags,
               long ld, int* n_frames, void* ws, long ws_bytes, hipStream_t st);

/* ---- speaker turns: window labels -> frame votes -> runs -> merged turns, and words -> turns, for R recordings per call
 * (tiny_audio_amd/csrc/speaker_post.hip; driven by tiny_audio_amd/diarization.py).  The reference does this stage in Python loops on the
 * host: one loop over the 10 ms voting grid, one over the runs, one over words x segments.  Contract: DESIGN.md section 3, "Speaker
 * turns"; the definition is the host functions of tiny_audio_amd/diarization.py (pinned on tests/golden/diarization.json), restated in
 * integer frames by tests/speaker_post_ref.py.  Every time of the reference's output is f * voting_rate for an integer frame f, so runs
 * and turns are (speaker, f0, f1) in int32 and the caller forms f * voting_rate; the votes are exact integers; the VAD index and the merge
 * rules are float64 evaluated as Python evaluates them (a * r - b * r with two roundings, an IEEE divide, truncation toward zero):
 * the source is compiled without contraction and without fast-math, and takes no integer shortcut.
 * Ragged layout: item k of recording r lies at cu[r] + k of the flat arrays, cu int32 [R + 1] on the device.
 *
 * ta_spk_vote_i32 (tiny_audio/diarization.py:520-537 _resample_vad, tiny_audio/diarization.py:539-614 _postprocess_segments): windows
 *   first / last / label int32 [sum_windows] (cu_win; label in [0, S) after the caller's rank mapping) vote on the frames
 *   [first, min(last, n_frames[r])) of recording r when first < last; any order, overlapping, empty or beyond the grid.  The owner of
 *   frame f is -1 when its largest count is 0 or flags[clip((long)((f * voting_rate) / vad_frame_s), 0, n_vad[r] - 1)] is 0 (vad
 *   unsigned char [R, ld_vad] as ta_vad_f32 writes it; n_vad[r] <= 0 silences the recording), else the lowest speaker among the largest
 *   counts.  A run is a maximal stretch of one owner != -1, f1 the first frame of the next owner or n_frames[r].  Runs in ascending time
 *   at run_spk / run_f0 / run_f1 [cu_cap[r] ..), n_runs[r] of them; positions beyond n_runs[r] are not written.  status[r]: 0, or 1 when
 *   the runs do not fit cu_cap[r + 1] - cu_cap[r] (the first that fit are written, nothing beyond), or 2 for n_frames[r] outside
 *   [0, max_frames] (no runs) or a window with first < 0 or a label outside [0, S) (that window does not vote; the reference's slice would
 *   wrap a negative start around: a documented divergence, refused by the Python layer).  2 sum_windows + VAD transitions + 2 runs always fit.
 *   One memset and three launches (integer atomics on a difference array per speaker, whose order cannot change the result; a scan
 *   fused with the arg-max, the VAD read and the boundary flags, TA_SPK_FRAME_TILE frames per workgroup; a compaction).
 * ta_spk_merge_i32 (tiny_audio/diarization.py:616-643 _merge_short_segments): for every run in order, start = f0 * voting_rate,
 *   end = f1 * voting_rate, short = (end - start) < min_segment_s, near = short ? short_gap_s : same_gap_s; a run of the last kept turn's
 *   speaker with start - that turn's end < near extends it, any other run that is not short is appended, a short one is dropped.  Turns at
 *   seg_* [cu_run[r] ..) (at most as many as runs), n_seg[r]; the runs need not come from ta_spk_vote_i32.  Recording r has
 *   cu_run[r + 1] - cu_run[r] runs, or with n_run (int32 [R], may be NULL) the first n_run[r] of that range: ta_spk_vote_i32's n_runs
 *   and cu_cap go in as they are, without a visit to the host in between.  One workgroup per recording, runs staged through LDS, one
 *   lane walks them.
 * ta_spk_words_f64 (tiny_audio/diarization.py:645-682 assign_speakers_to_words): mid = (word_start + word_end) / 2; out[w] = the lowest
 *   segment index g of the recording (counted from cu_seg[r]) with seg_start[g] <= mid <= seg_end[g], else the lowest g that minimises
 *   fabs(mid - (seg_start[g] + seg_end[g]) / 2), else -1 (no segments).  Segments in any order, overlapping allowed.  Brute force:
 *   16 lanes per word, segments staged through LDS TA_SPK_SEG_TILE at a time.  max_words bounds every recording's word count.
 * Limits (TA_ERR_ARG beyond them): R <= TA_SPK_MAX_RECORDINGS, 1 <= S <= TA_SPK_MAX_SPEAKERS, max_frames <= TA_SPK_MAX_FRAMES (the voting
 * grid of 2.9 h), sum_windows and max_words <= TA_SPK_MAX_ITEMS, every option finite and > 0.  Values that live on the device (labels,
 * first, word and segment times) are checked by the Python layer before they are uploaded.
 * ws: ta_spk_post_workspace_bytes(R, S, max_frames, sum_windows) bytes, no initial contents required; -1 for sizes that are refused. */
#define TA_SPK_MAX_RECORDINGS 64
#define TA_SPK_MAX_SPEAKERS 16
#define TA_SPK_MAX_FRAMES 1048577
#define TA_SPK_MAX_ITEMS 1048576
#define TA_SPK_FRAME_TILE 1024
#define TA_SPK_SEG_TILE 1024
typedef struct { double voting_rate, vad_frame_s, min_segment_s, short_gap_s, same_gap_s; } ta_spk_post_options;
long ta_spk_post_workspace_bytes(int R, int S, long max_frames, long sum_windows);
int ta_spk_vote_i32(const int* first, const int* last, const int* label, const int* cu_win, long sum_windows, int R, int S,
                    const int* n_frames, long max_frames, const unsigned char* vad, long ld_vad, const int* n_vad,
                    const ta_spk_post_options* opt, const int* cu_cap, int* run_spk, int* run_f0, int* run_f1, int* n_runs, int* status,
                    void* ws, long ws_bytes, hipStream_t st);
int ta_spk_merge_i32(const int* run_spk, const int* run_f0, const int* run_f1, const int* cu_run, const int* n_run, int R,
                     const ta_spk_post_options* opt, int* seg_spk, int* seg_f0, int* seg_f1, int* n_seg, hipStream_t st);
int ta_spk_words_f64(const double* word_start, const double* word_end, const int* cu_word, const double* seg_start, const double* seg_end,
                     const int* cu_seg, int R, long max_words, int* out, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif /* TA355_H */
