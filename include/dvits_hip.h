/*
 * dvits_hip.h — C ABI of libdvits_hip.so, the MI355X (gfx950) engine under the
 * diff-vits diffusion-sampling path.
 *
 * The reference (adelacvg/diff-vits) has no FFI layer: its boundary for this path is
 * the Python surface
 *     unet1d/unet_1d_condition.py:743-1037   UNet1DConditionModel.forward
 *     sampler/dpm_solver.py:1047-1245         DPM_Solver.sample  (multistep, dpmsolver++)
 *     sampler/uni_pc.py:590-672               UniPC.sample       (multistep, bh1/bh2)
 * The Python mirror classes in diff-vits_amd/{unet1d,sampler}/ keep that surface and
 * bind the entry points below through ctypes (diff-vits_amd/_lib.py); INTEGRATION.md
 * shows the stub.  Plain pointers and sizes only: no torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, a negative dv_status otherwise;
 *     dv_last_error() returns a thread-local message for the last failure.
 *   - all tensor pointers are DEVICE pointers to contiguous float32 unless noted.
 *     The caller owns inputs/outputs; the library owns packed weights and workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Work is
 *     enqueued asynchronously on it; nothing here synchronises the device except
 *     dv_unet_prepare / dv_penc_prepare / dv_*_destroy, the single-operator dv_op_* entry points (they
 *     return results) and the first dv_sampler_run of a plan (it captures the loop into a hipGraph).
 *   - handles are not thread-safe; distinct handles are independent.
 */
#ifndef DVITS_HIP_H
#define DVITS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DV_OK = 0,
  DV_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
  DV_ERR_HIP = -2,          /* a HIP runtime call failed */
  DV_ERR_STATE = -3,        /* call order violated (e.g. forward before prepare) */
  DV_ERR_MISSING_WEIGHT = -4
} dv_status;

/* Contraction precision (SURVEY.md §7 "Accuracy vs bf16"):
 *   DV_PREC_BF16X3: split-bf16, 3 MFMA products per tile, fp32 accumulate — the parity mode
 *   DV_PREC_BF16  : single bf16 product — fast mode, ~7e-3 rel. error, reported separately */
typedef enum { DV_PREC_BF16X3 = 0, DV_PREC_BF16 = 1 } dv_precision;

/* Constructor keywords of UNet1DConditionModel that shape the network
 * (reference unet_1d_condition.py:151-203; diffusion values model3.py:887-896). */
typedef struct {
  int32_t in_channels;            /* C + cond channels, e.g. 208 */
  int32_t out_channels;           /* C, e.g. 80 */
  int32_t n_levels;               /* len(block_out_channels), 2..6 */
  int32_t block_out_channels[6];
  int32_t layers_per_block;       /* 2 */
  int32_t num_heads;              /* `attention_head_dim` keyword (= head count) */
  int32_t cross_attention_dim;    /* encoder_hidden_states feature dim */
  int32_t norm_num_groups;        /* 8 */
  int32_t add_embed_heads;        /* addition_embed_type_num_heads, 64 */
  float   norm_eps;               /* 1e-5 */
} dv_unet_cfg;

/* PromptEncoder constructor arguments (reference model3.py:382-406 as built by Diffusion_Encoder, model3.py:898:
 * PromptEncoder(100, hidden, hidden, 4, 0.2); every layer is OPERATIONS_ENCODER[8] = EncSALayer(c, 8 heads,
 * kernel_size 9, 'SAME'), operations.py:961-964). */
typedef struct {
  int32_t in_channels;            /* mel channels of the prompt, 100 */
  int32_t hidden_channels;        /* 128 (config.json diffusion_encoder.hidden_channels) */
  int32_t out_channels;           /* = hidden_channels at the reference call site */
  int32_t n_layers;               /* 4 */
  int32_t num_heads;              /* 8 */
  int32_t ffn_kernel;             /* 9 */
} dv_penc_cfg;

/* TextEncoder constructor arguments (reference model3.py:322-358 over attentions.Encoder, attentions.py:37-68): the product
 * is 256 hidden channels, 2 heads (head dim 128), 6 post-norm layers, k = 3 feed-forward convolutions, relative-position
 * window 4, speaker vector added before layer 2. */
typedef struct {
  int32_t n_vocab, n_tones, n_languages;  /* rows of emb / tone_emb / language_emb */
  int32_t hidden_channels;        /* H, a multiple of 32; H / n_heads must be 32, 64 or 128 */
  int32_t filter_channels;        /* feed-forward width, a multiple of 32 */
  int32_t out_channels;           /* C: proj writes 2C statistics channels (m | logs) */
  int32_t n_heads;
  int32_t n_layers;
  int32_t kernel_size;            /* of conv_1 / conv_2, odd ('same' padding) */
  int32_t window_size;            /* relative-position window w: emb_rel_k / emb_rel_v are [1, 2w+1, H / n_heads]; <= 16 */
  int32_t gin_channels;           /* speaker vector width, 0 = no spk_emb_linear */
  int32_t cond_layer_idx;         /* the layer in front of which the speaker vector is added */
} dv_tenc_cfg;

/* PosteriorEncoder constructor arguments (reference model3.py:526-548 over modules.WN): the product is 100 mel channels -> 256
 * hidden channels, 16 layers of 5-tap gated convolutions with dilation 1, 128 output channels, a 256-wide speaker vector. */
typedef struct {
  int32_t in_channels;            /* mel channels (any; the input planes are padded to a multiple of 64) */
  int32_t out_channels;           /* C: proj writes 2C statistics channels (m | logs); a multiple of 16 */
  int32_t hidden_channels;        /* H: k_wn_layer is instantiated for 256 */
  int32_t kernel_size;            /* 5 */
  int32_t dilation_rate;          /* 1 */
  int32_t n_layers;
  int32_t gin_channels;           /* speaker vector width, 0 = no cond_layer */
} dv_qenc_cfg;

/* Log-mel front-end (mel.py MelSpectrogram as tts_infer.py:57-66 builds it).  Built: n_fft 1024, hop_length 256, centred frames
 * with reflect padding, one-sided spectrum, n_mels <= 128; everything else is refused at create. */
typedef struct {
  int32_t n_fft;                  /* 1024 */
  int32_t hop_length;             /* 256 */
  int32_t n_mels;                 /* 1..128 (100) */
  int32_t center;                 /* 1 */
  float   log_clip;               /* floor under the logarithm of DV_MEL_LOG, > 0 (1e-7) */
} dv_mel_cfg;

/* Vocos vocoder (charactr/vocos-mel-24khz: ConvNeXt-1D backbone + ISTFT head).  The product is 100 mel channels -> dim 512,
 * intermediate 1536, 8 layers, n_fft 1024, hop 256. */
typedef struct {
  int32_t n_mels;                 /* input channels (any; the input planes are padded to a multiple of 64) */
  int32_t dim;                    /* C: a multiple of 64 up to 512 (k_dw7_ln) */
  int32_t intermediate;           /* I: a multiple of 32 */
  int32_t n_layers;
  int32_t n_fft;                  /* 1024 */
  int32_t hop;                    /* 256 */
} dv_voc_cfg;

typedef struct dv_unet dv_unet;
typedef struct dv_plan dv_plan;
typedef struct dv_penc dv_penc;
typedef struct dv_tenc dv_tenc;
typedef struct dv_qenc dv_qenc;
typedef struct dv_voice dv_voice;
typedef struct dv_mel dv_mel;
typedef struct dv_resample dv_resample;
typedef struct dv_voc dv_voc;

const char* dv_last_error(void);
/* Library/version probe: returns e.g. "dvits_hip 0.1 gfx950". */
const char* dv_version(void);
/* Development: bytes of plan memory filled so far in this process because DVITS_POISON was "nan" (byte 0xFF) or "big" (byte 0x4B)
 * at a prepare or a single-operator call (development knobs).  The fill covers memory whose contents the plan leaves
 * undefined: the denoiser's and the prompt encoder's activation slab, and every buffer the row engines and the dv_op_* entry points
 * allocate without zeroing.  A running total that never goes back; it stays where it is while the variable is unset. */
int64_t dv_poisoned_bytes(void);
/* Development: bytes of plan memory REQUESTED so far without defined contents - the same allocations, counted at the same place,
 * whether DVITS_POISON is set or not.  Its growth over one prepare (or one dv_op_* call, or the first dv_sampler_run of a plan) is
 * that plan's unzeroed byte count: under `nan` / `big`, dv_poisoned_bytes() must grow by exactly as much. */
int64_t dv_unwritten_bytes(void);

/* ---- denoiser: UNet1DConditionModel ------------------------------------------------ */

/* Replaces UNet1DConditionModel.__init__ (unet_1d_condition.py:151-607). */
int dv_unet_create(const dv_unet_cfg* cfg, dv_unet** out);
void dv_unet_destroy(dv_unet* u);

/* Hand over one state-dict tensor under its reference name, e.g.
 * "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k.weight"
 * (replaces load_state_dict, tts_infer.py:75-81).  `dev_ptr` is float32, contiguous,
 * shape[ndim]; the data is copied (the caller keeps ownership). */
int dv_unet_set_weight(dv_unet* u, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim);

/* Pack weights for `precision`, build the kernel schedule for (B, T, L) and allocate the
 * workspace arena (T is arbitrary: levels whose frame count is no multiple of 32 are laid out in a padded row space
 * inside the engine).  Must be called after all weights are set and again whenever B/T/L,
 * the precision or the weights change.  `force_upsample_size` = the reference's
 * forward_upsample_size flag (unet_1d_condition.py:789-797), computed by the caller from
 * the shape of `sample`. */
int dv_unet_prepare(dv_unet* u, int32_t B, int32_t T, int32_t L, int32_t precision, int32_t force_upsample_size);

/* Step-invariant conditioning (hoisted out of the sampler loop): pooled-text embedding
 * add_embedding(enc) (unet_1d_condition.py:869-870), the 16 cross-attention K/V
 * projections (attention_processor.py:1016-1017) and the additive mask bias (:816-818).
 * enc: [B, L, cross_attention_dim]; mask_bias: [B, L] additive (0 / -10000) or NULL. */
int dv_unet_set_cond(dv_unet* u, const float* enc, const float* mask_bias, void* stream);

/* One denoiser evaluation = UNet1DConditionModel.forward (unet_1d_condition.py:743-1037).
 *   x    : [B, cx, T]            first cx input channels (channels-first, as the reference)
 *   cond : [B, in_channels-cx, T] remaining input channels, or NULL when cx == in_channels
 *   t    : [B] float32 timesteps (fractional allowed)
 *   y    : [B, out_channels, T]  output
 * Passing x and cond separately avoids materialising torch.cat([x, cond]) (model3.py:908). */
int dv_unet_forward(dv_unet* u, const float* x, int32_t cx, const float* cond, const float* t, float* y,
                    void* stream);

/* Number of kernel launches one forward enqueues, and algorithmic FLOPs (2*MAC of all
 * contractions) of one forward at the prepared shape — for the roofline report. */
int dv_unet_stats(dv_unet* u, int64_t* n_launch, double* flops);
/* Number of schedule OPERATIONS of one forward (the index range of dv_unet_op_info / dv_unet_forward_timed).  An
 * operation is one kernel launch, except a split-K GEMM pair (k-slice pass + epilogue pass), which is one operation
 * of two launches. */
int dv_unet_op_count(dv_unet* u, int32_t* n_ops);

/* Measurement aid for bench.py: one forward with a HIP event pair around every launch of the
 * schedule (eager, not graph-replayed); ms_per_op[i] = elapsed ms of operation i (capacity >= dv_unet_op_count).
 * dv_unet_op_info gives operation i's kernel family ("gemm", "attn", "gn_partial", "gn_finalize",
 * "ln_stats", "misc"), its algorithmic FLOPs (0 for non-contractions) and a shape description. */
int dv_unet_forward_timed(dv_unet* u, const float* x, int32_t cx, const float* cond, const float* t, float* y,
                          void* stream, float* ms_per_op, int32_t capacity);
int dv_unet_op_info(dv_unet* u, int32_t index, char* kind16, double* flops, char* desc128);
/* Re-launches only the schedule's launches of one kernel family (e.g. "gemm"), in schedule order with their own
 * arguments, `reps` times back to back between ONE HIP event pair on `stream` (after one untimed pass);
 * *ms_total / *launches = that family's average launch duration without per-launch event overhead.  Needs a completed
 * dv_unet_forward (the buffers then hold valid data; outputs are overwritten with the same values). */
int dv_unet_time_family(dv_unet* u, const char* kind, int32_t reps, void* stream, float* ms_total, int32_t* launches);

/* Persistent per-XCD schedule (environment DVITS_PERSIST=1 at prepare time; csrc/persist.hip): *n_ops = number of
 * schedule operations that run inside the one persistent launch (0 = off / not applicable to this shape);
 * *error_flag = 0 ok, 1 = an in-launch barrier timed out, 2 = the workgroups were not spread evenly over the XCDs
 * (synchronises the device). */
int dv_unet_persist_status(dv_unet* u, int32_t* n_ops, int32_t* error_flag);
/* In-launch hand-overs (default; environment DVITS_GNX=0 at prepare time restores the separate k_gn_apply launches and the
 * two-GEMM feed-forward).  GroupNorm finished inside the producer GEMM: the workgroups of such a GEMM exchange their tile
 * statistics inside the launch and wait for one another (bounded).  Feed-forward block of the C = 256 / 384 / 512 transformer
 * blocks as one launch (round 5, csrc/kernels_ffsplit.hip; reference unet1d/attention.py:189-203, 206-255; DVITS_FF_SPLIT=0
 * restores the two GEMMs): the 4 / 8 workgroups of a row block hand their partial sums over the same way.  *n_ops = schedule
 * operations that wait inside their launch; *timed_out = 1 if any of them ever gave up waiting - the
 * results of that launch are invalid and every later dv_unet_forward / dv_sampler_run on this handle fails with
 * DV_ERR_HIP.  Does not synchronise: meaningful once the stream has drained. */
int dv_unet_handover_status(dv_unet* u, int32_t* n_ops, int32_t* timed_out);
/* Recovery from such a time-out (a foreign kernel kept some workgroups off the CUs past the bounded wait): synchronises the
 * device and clears the flag, so that the handle works again.  The caller then re-plans it with dv_unet_set_exclusive(u, 0) -
 * GroupNorm as separate launches, no in-launch waits - and repeats the lost run; diff_vits_amd/engine.py does exactly that
 * (UNetEngine.recover_handover; WHEN it checks - lazily since round 5, UNetEngine.wait() being the explicit point - is
 * described in INTEGRATION.md section 4) and reports the downgrade once. */
int dv_unet_handover_reset(dv_unet* u);
/* The in-launch waits above assume that the launch has the device to itself (every workgroup resident at once): true
 * for one stream, or for several streams that never run kernels of such handles side by side.  A host that drives
 * several handles CONCURRENTLY on different streams of one device must call this with exclusive = 0 before
 * dv_unet_prepare (GroupNorm then runs as separate launches on that handle); two such GEMMs sharing the CUs could wait
 * for each other's queued workgroups - the bounded wait turns that into DV_ERR_HIP, not a hang, but the run is lost. */
int dv_unet_set_exclusive(dv_unet* u, int32_t exclusive);
/* Profiling aid: s_memtime stamps taken by one workgroup of XCD 0 after every operation of the last persistent launch;
 * returns the number of stamps written (operations + 1) or a negative error; *first_op = schedule index of the first
 * operation inside the launch (pairs with dv_unet_op_info). */
int dv_unet_persist_ticks(dv_unet* u, int32_t* first_op, uint64_t* ticks, int32_t capacity);

/* Debug/parity probe: copy a named intermediate activation (channels-last [B, T, C]) of the
 * last forward to the host.  Available only when dv_unet_prepare ran with the environment
 * variable DVITS_KEEP_INTERMEDIATES=1 (buffers are then never reused) or =tap.  dims[3] = {B, T, C};
 * host_out may be NULL to query dims.  Names follow the reference module paths, e.g.
 * "conv_in", "emb", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0",
 * "mid_block.resnets.1", "up_blocks.1.upsamplers.0".
 * =1 plans a schedule of its own that keeps every intermediate (the feed-forward as two GEMMs, no buffer reuse, every fp32 copy
 * kept).  =tap plans what an unset variable plans and adds one copy operation per probe (kind "probe" in dv_unet_op_info, counted
 * by dv_unet_stats) behind its producer, into a side buffer freed with the schedule; a tensor without an fp32 copy is read from
 * its split planes.  Names the production plan does not hold - "...transformer_blocks.0.ff", and a "...conv1" whose output exists
 * only normalised - are not registered then: DV_ERR_INVALID, as for any unknown name. */
int dv_unet_probe(dv_unet* u, const char* name, float* host_out, int64_t capacity, int64_t* dims);

/* ---- enrolled voices: the conditioning of one speaker prompt, kept and bound to batch rows --------------------------------
 * Everything dv_unet_set_cond computes depends on the prompt alone.  At prepare time the engine records which persistent
 * buffers the conditioning schedule writes and the step schedule reads (the K / V^T fragments of the 16 transformer blocks,
 * the key-bias rows, the pooled-text row; the fp32 K | V and the mask bias where a block's attention still reads them) - the
 * conditioning segment table, every buffer utterance-major.  A voice record is one row of all of them, laid end to end in
 * 16-byte chunks (a segment whose bytes per utterance are no multiple of 16 is padded in the record, never in the buffer).
 * No arithmetic: binding a record writes, byte for byte, what dv_unet_set_cond wrote into the row it was taken from.
 *
 * Layout signature: a hash over the engine configuration, the precision, L and every segment's kind and size - not over B
 * or T.  A record binds to any schedule with its signature (another batch size, another frame count, a re-planned or
 * another handle of the same network); it does NOT know the weights - the caller keeps records apart per weight set. */
/* 0 before dv_unet_prepare. */
uint64_t dv_unet_cond_signature(const dv_unet* u);
/* After a dv_unet_set_cond (or binds) on the prepared schedule: copies rows[0..n) of the conditioning (repeats allowed) into n
 * new records, out[0..n).  A record owns its device memory: it outlives dv_unet_prepare and dv_unet_destroy.  Waits for the
 * device before and after its one gather launch (k_voice_gather): the records are complete on return.  DV_ERR_INVALID for a
 * row outside the batch, DV_ERR_STATE for a row that has not been conditioned since prepare; nothing is returned then. */
int dv_voice_capture(dv_unet* u, const int32_t* rows, int32_t n, dv_voice** out);
/* Writes voices[i] into row rows[i] of the CURRENT schedule's persistent buffers: one scatter launch (k_voice_scatter) on
 * `stream` for up to 192 rows (one more per further 192; the pairs travel in the launch's 3 KiB argument block), no allocation,
 * no wait - capturable.  The buffers' addresses do
 * not change, so a sampler graph captured on this schedule replays with the new voices as it is.  Rows not named keep their
 * conditioning.  dv_unet_forward / dv_sampler_run need every row conditioned since prepare, by dv_unet_set_cond or by binds
 * (DV_ERR_STATE otherwise).  DV_ERR_INVALID, before anything is launched and with nothing changed, for a row outside the
 * batch, a row named twice, or a record whose signature is not dv_unet_cond_signature.  The records must stay alive until
 * the launch has run (dv_voice_destroy waits for the device). */
int dv_unet_bind_voices(dv_unet* u, const int32_t* rows, dv_voice* const* voices, int32_t n, void* stream);
/* Which rows have been conditioned since prepare: flags[0..n), n = the schedule's batch (DV_ERR_INVALID otherwise).  set = 0
 * reads them; set != 0 overwrites them - a caller that used the schedule's rows as scratch for a conditioning pass of its own
 * (re-deriving records) hands back the truth, and a forward is refused again while a row is unconditioned.  Host only. */
int dv_unet_cond_rows(dv_unet* u, uint8_t* flags, int32_t n, int32_t set);
uint64_t dv_voice_signature(const dv_voice* v);
/* Device bytes of the record: every segment's bytes per utterance, i.e. it grows with L and not with B or T.  The production
 * denoiser at L = 256 keeps 10 226 688 bytes (9.75 MiB) per voice, nearly all of it the K / V^T fragment planes of the 16 blocks:
 * a service that enrols many voices budgets device memory for them. */
int64_t dv_voice_bytes(const dv_voice* v);
void dv_voice_destroy(dv_voice* v);

/* ---- sampler: DPM-Solver++ / UniPC multistep loops --------------------------------- */

/* DV_SOLVER_UNIPC_VARY: variant='vary_coeff' (multistep_uni_pc_vary_update, uni_pc.py:368-469).  DPM-Solver++ takes
 * orders 1-3 (the reference's three closed forms); the UniPC variants any order 1..8 (the reference solves the
 * order x order systems numerically, uni_pc.py:545-560 / :410-420). */
/* DV_SOLVER_DPM: algorithm_type='dpmsolver' - the multistep updates on the NOISE prediction (dpm_solver.py:581-592, 841-847,
 * 895-904); the network still predicts x0: every evaluation is followed by eps = (x - alpha_t x0) / sigma_t on its history
 * slot (model_wrapper's 'x_start' branch, dpm_solver.py:290-292).
 * DV_SOLVER_*_TAYLOR: solver_type='taylor' - the second-order update's Taylor form (dpm_solver.py:825-829, 848-851); orders 1
 * and 3 are the same as without it.
 * DV_SOLVER_UNIPC_*_NOISE: UniPC(algorithm_type='noise_prediction') - the same three variants on the noise prediction
 * (uni_pc.py:448-468, 569-587), with the in-place x0 -> noise conversion of DV_SOLVER_DPM. */
typedef enum { DV_SOLVER_DPMPP = 0, DV_SOLVER_UNIPC_BH1 = 1, DV_SOLVER_UNIPC_BH2 = 2, DV_SOLVER_UNIPC_VARY = 3, DV_SOLVER_DPM = 4,
               DV_SOLVER_DPMPP_TAYLOR = 5, DV_SOLVER_DPM_TAYLOR = 6, DV_SOLVER_UNIPC_BH1_NOISE = 7, DV_SOLVER_UNIPC_BH2_NOISE = 8,
               DV_SOLVER_UNIPC_VARY_NOISE = 9 } dv_solver;
typedef enum { DV_SKIP_TIME_UNIFORM = 0, DV_SKIP_TIME_QUADRATIC = 1, DV_SKIP_LOGSNR = 2 } dv_skip;
/* NoiseScheduleVP(schedule=...): 'discrete' (betas; dpm_solver.py:98-107, uni_pc.py:59-66), or the continuous-time VP
 * schedules 'linear' (beta_0, beta_1; dpm_solver.py:108-111,133-134,160-163) and 'cosine' (uni_pc.py:73-100; UniPC only -
 * dpm_solver.py:94 knows 'discrete' and 'linear').  Continuous schedules: total_N = 1000, T = 1 (0.9946 for 'cosine'), and
 * the network is called with t itself instead of (t - 1/N) * N (dpm_solver.py:271-280). */
typedef enum { DV_SCHEDULE_DISCRETE = 0, DV_SCHEDULE_LINEAR = 1, DV_SCHEDULE_COSINE = 2 } dv_schedule;

/* Host fp64 precompute of every schedule scalar of the loop
 * (NoiseScheduleVP + get_time_steps + the multistep coefficient algebra:
 * dpm_solver.py:6-167, 453-480, 547-592, 796-904; uni_pc.py:471-588).
 * betas: HOST float32[n_betas] (the reference's `self.betas`, model3.py:990). */
int dv_sampler_plan(int32_t solver, const float* betas, int32_t n_betas, int32_t steps, int32_t order,
                    int32_t skip_type, int32_t lower_order_final, dv_plan** out);
/* The same with the remaining multistep options of DPM_Solver.sample / UniPC.sample (dpm_solver.py:1047-1050,
 * uni_pc.py:590-591): integrate from t_start (<= 0: T = 1) down to t_end (<= 0: 1/N); denoise_to_zero appends the
 * data prediction at t_end as one more model evaluation (dpm_solver.py:1234-1240). */
int dv_sampler_plan_ex(int32_t solver, const float* betas, int32_t n_betas, int32_t steps, int32_t order,
                       int32_t skip_type, int32_t lower_order_final, double t_start, double t_end,
                       int32_t denoise_to_zero, dv_plan** out);
/* ... for any schedule kind: betas / n_betas are read for DV_SCHEDULE_DISCRETE only, beta_0 / beta_1 for DV_SCHEDULE_LINEAR
 * only (the reference's defaults: 0.1, 20). */
int dv_sampler_plan_sched(int32_t solver, int32_t schedule, const float* betas, int32_t n_betas, double beta_0, double beta_1,
                          int32_t steps, int32_t order, int32_t skip_type, int32_t lower_order_final, double t_start,
                          double t_end, int32_t denoise_to_zero, dv_plan** out);
/* ... and for the singlestep methods of DPM_Solver.sample ("DPM-Solver-fast", dpm_solver.py:482-539, 594-794, 1214-1232):
 * `steps` model evaluations shared out over outer steps of order <= `order`; DV_METHOD_SINGLESTEP_FIXED: steps / order outer
 * steps of exactly `order`.  DPM-Solver(++) solvers only. */
typedef enum { DV_METHOD_MULTISTEP = 0, DV_METHOD_SINGLESTEP = 1, DV_METHOD_SINGLESTEP_FIXED = 2 } dv_method;
int dv_sampler_plan_method(int32_t solver, int32_t schedule, const float* betas, int32_t n_betas, double beta_0, double beta_1,
                           int32_t method, int32_t steps, int32_t order, int32_t skip_type, int32_t lower_order_final,
                           double t_start, double t_end, int32_t denoise_to_zero, dv_plan** out);
void dv_plan_destroy(dv_plan* p);

/* Introspection for tests: number of model evaluations, and the plan's tables.
 * t_input[nfe] = timestep fed to the network at each evaluation;
 * timesteps[steps+1] = continuous-time grid. */
int dv_plan_info(const dv_plan* p, int32_t* nfe, double* t_input, double* timesteps);
/* n_timesteps = entries of `timesteps` (steps + 1 for the multistep loops, outer steps + 1 for the singlestep methods);
 * eval_times[nfe] = continuous time of each evaluation. */
int dv_plan_times(const dv_plan* p, int32_t* n_timesteps, double* eval_times);

/* The compiled loop, for host-side execution with an arbitrary Python callable and for tests:
 * coefficient rows (8 floats each: c0 for x, c1..c4 for the history terms) and events
 * (9 int32 each: type 0=EVAL/1=COMB, src 0=x/1=x_pred (EVAL: the network input; COMB: the
 * tensor the c0 term multiplies - sums of more than four history terms are chained through
 * x_pred), eval_idx (EVAL; -1 for COMB), dst (EVAL: history slot; COMB: 0=x/1=x_pred), coef row,
 * slot0..slot3 (-1 = unused)).  *n_slots = number of history buffers the loop needs. */
int dv_plan_coefs(const dv_plan* p, int32_t* n_rows, float* rows8);
int dv_plan_events(const dv_plan* p, int32_t* n_events, int32_t* ev9, int32_t* n_slots);

/* Run the whole loop: x_inout [B, C, T] is x_T on entry and x_0 on exit; cond
 * [B, in_channels-C, T] is the channel-concat condition.  dv_unet_set_cond must have been
 * called.  The first call for a given (plan, unet shape) captures the loop into a
 * hipGraph; later calls replay it.  x_inout must be 16-byte aligned (the update kernel moves it as float4):
 * DV_ERR_INVALID otherwise, before anything is launched. */
int dv_sampler_run(dv_plan* p, dv_unet* u, float* x_inout, const float* cond, void* stream);

/* Same loop with a caller-supplied model instead of the UNet, for sampler known-answer
 * tests: model(user, x_dev, t_input_host, out_dev) must enqueue out = f(x, t) on `stream`.  x_inout [numel], any
 * numel >= 1, 16-byte aligned like dv_sampler_run's (DV_ERR_INVALID otherwise, before anything is launched). */
typedef int (*dv_model_fn)(void* user, const float* x, double t_input, float* out, void* stream);
int dv_sampler_run_custom(dv_plan* p, dv_model_fn fn, void* user, float* x_inout, int64_t numel, void* stream);

/* correcting_x0_fn='dynamic_thresholding' of DPM_Solver / UniPC (dpm_solver.py:409-425, 433-445; uni_pc.py:256-277, 292-293) as
 * part of the compiled loop: after every evaluation e with eval_mask[e] != 0 (HOST uint8[nfe]; NULL: all of them) the data
 * prediction is replaced, per utterance, by clamp(x0, -s, s) / s with s = max(quantile(|x0|, ratio), max_val) - before
 * anything reads it (in the noise forms the x0 -> noise conversion sees the thresholded x0).  Which evaluations the
 * reference thresholds is the caller's rule (all of them for 'dpmsolver++' / 'data_prediction'; only the final
 * denoise_to_zero evaluation otherwise).  ratio < 0 switches it off again; ratio > 1, or max_val <= 0 or not finite:
 * DV_ERR_INVALID.  Any change drops the captured graph.  dv_sampler_run thresholds per row of its batch; a plan with
 * thresholding is refused by dv_sampler_run_custom (DV_ERR_INVALID), which does not know the rows: */
int dv_plan_set_thresholding(dv_plan* p, double ratio, double max_val, const uint8_t* eval_mask);
/* dv_sampler_run_custom with x_inout as [rows, numel / rows] (rows in 1..2048, numel % rows == 0), for plans with and
 * without thresholding. */
int dv_sampler_run_custom_rows(dv_plan* p, dv_model_fn fn, void* user, float* x_inout, int32_t rows, int64_t numel, void* stream);

/* model_wrapper(guidance_type='classifier-free', condition=, unconditional_condition=, guidance_scale=) (dpm_solver.py:322-330,
 * uni_pc.py:221-229) as part of the compiled loop.  on != 0: every evaluation of dv_sampler_run runs the network on [x | x]
 * - the unet must be prepared at an EVEN batch 2B and conditioned (dv_unet_set_cond) with [unconditional | conditional]
 * encoder states and mask biases, the unconditional half first; x_inout [B, C, T] and cond [B, in_channels-C, T] hold B rows
 * (an odd unet batch: DV_ERR_INVALID before anything is launched) - and the history slot receives
 * x0_u + scale * (x0_c - x0_u): d = x0_c - x0_u in float32, then fmaf(scale, d, x0_u).  (The reference combines the noise
 * predictions; they are linear in x0, so this is the same guided prediction without the x0 -> noise -> x0 round trip.)
 * Thresholding (dv_plan_set_thresholding), where the plan has it, sees the guided prediction, per row of x_inout.  The plan
 * owns three 2B-row staging buffers (network input, network output, cond - the latter filled once per run); the cost per
 * evaluation is two elementwise launches.  scale must be finite (DV_ERR_INVALID); on = 0 switches guidance off again (scale
 * is ignored).  Any change drops the captured graph.  dv_sampler_run_custom / _rows refuse a guided plan (DV_ERR_INVALID):
 * the callback has no pair of conditions. */
int dv_plan_set_guidance(dv_plan* p, double scale, int32_t on);
/* *n_nodes = nodes of the hipGraph the last dv_sampler_run of this plan captured (kernel launches of the complete loop:
 * the head-of-loop chains, every evaluation, every update); 0 while the plan holds no graph (never run, dropped by a
 * change, DVITS_NO_GRAPH=1).  For measurements and tests: what a captured loop really holds. */
int dv_plan_graph_nodes(const dv_plan* p, int64_t* n_nodes);

/* Known-frame correction (mel infilling: keep a set of frames on the forward process of a known signal while the rest is
 * generated) as part of the compiled loop - the closed form of a correcting_xt_fn (dpm_solver.py:384-394; uni_pc.py:256-261):
 *     x[b, :, f] <- alpha_t * known[b, :, f] + sigma_t * eps[b, :, f]   where keep[b, f] != 0,   unchanged elsewhere,
 * at exactly the points where the reference calls correcting_xt_fn (dpm_solver.py:1180-1238, uni_pc.py:615-666).  Multistep
 * methods: the start point once the first evaluation is complete (an x0 -> noise conversion of that evaluation still reads the
 * uncorrected x), then x after every update that lands in x (UniPC: after the corrector), the denoise_to_zero result
 * included.  Singlestep methods: after every outer step; the start point is not corrected.  t is the grid point the step
 * lands on; (alpha, sigma) come from the plan's own schedule in fp64 and are applied as floats - fadd(fmul(alpha, known),
 * fmul(sigma, eps)), the three float32 roundings of the torch expression.
 * known / eps [rows, channels, frames] float32 and keep [rows, frames] uint8 are DEVICE pointers that stay valid and keep
 * their addresses across runs (their contents may change between runs: a captured graph reads them on replay).
 * known == NULL switches the correction off.  Any change of a pointer or of the shape drops the captured graph; setting the
 * same values again is free.  dv_sampler_run refuses (DV_ERR_INVALID, before anything is launched) a plan whose rows /
 * channels / frames are not those of x_inout - under guidance x_inout holds B rows and the correction sees those B rows;
 * dv_sampler_run_custom_rows takes rows from its argument and needs rows * channels * frames == numel; dv_sampler_run_custom
 * has no row count and refuses such a plan.  Cost: one elementwise launch per correction point. */
int dv_plan_set_known_frames(dv_plan* p, const float* known, const float* eps, const uint8_t* keep,
                             int32_t rows, int32_t channels, int32_t frames);
/* The correction points of the plan, with or without dv_plan_set_known_frames: *n_rows of them, rows2 [n_rows][2] =
 * (alpha, sigma) as the floats the loop applies, in the order of the launches.  Either output may be NULL. */
int dv_plan_known_coefs(const dv_plan* p, int32_t* n_rows, float* rows2);

/* ---- prompt encoder: PromptEncoder.forward, reference model3.py:408-433 ------------------
 * The reference recomputes it inside every denoiser call (Diffusion_Encoder.forward, model3.py:902-906) although it
 * does not depend on the step; the host mirror calls this once per sampler run and feeds the result to
 * dv_unet_set_cond. */
int dv_penc_create(const dv_penc_cfg* cfg, dv_penc** out);
void dv_penc_destroy(dv_penc* p);
/* State-dict tensors under their reference names relative to the PromptEncoder ("pre.layer_norm.weight",
 * "layers.0.op.self_attn.in_proj_weight" [3H,H], "layers.0.op.ffn.ffn_1.3.weight" [4H,H], "out_proj.conv.bias",
 * "layer_norm.weight", ...), float32, copied.  The two ConvTBC weights (model.py:145-146, stored [1, C_in, C_out])
 * are handed over as [C_out, C_in]: "pre.conv.weight", "out_proj.conv.weight". */
int dv_penc_set_weight(dv_penc* p, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim);
int dv_penc_prepare(dv_penc* p, int32_t B, int32_t L, int32_t precision);
/* prompt: [B, in_channels, L] float32 (the reference's src_tokens); keep: [B, L] float32, 1 = frame < length,
 * 0 = padding (commons.sequence_mask, model3.py:416); out: [B, L, out_channels] float32 = the reference's return
 * value transposed (model3.py:912 feeds prompt.transpose(1,2) to the UNet), padding frames zero. */
int dv_penc_forward(dv_penc* p, const float* prompt, const float* keep, float* out, void* stream);
int dv_penc_stats(dv_penc* p, int64_t* n_launch, double* flops);
/* Debug/parity probe, the contract of dv_unet_probe: a named intermediate (channels-last [B, L, C]) of the last
 * dv_penc_forward, copied to the host; only after a dv_penc_prepare with DVITS_KEEP_INTERMEDIATES=1.  Names: "pre",
 * "layerN.attn" (after the attention out-projection + residual + mask), "layerN.ffn1" (the ReLU'd 4H-wide product,
 * joined from its split planes and scaled by ffn_kernel^-1/2 as the reference has it; padding frames are NOT masked
 * there, in the reference neither), "layerN" (the layer's output), "out_proj" (before the last LayerNorm). */
int dv_penc_probe(dv_penc* p, const char* name, float* host_out, int64_t capacity, int64_t* dims);

/* ---- text encoder enc_p: TextEncoder.forward, reference model3.py:360-381 (phoneme ids -> prior statistics) -------
 * The contracts of the dv_penc_* functions.  Weights under their reference names relative to "enc_p.": "emb.weight",
 * "tone_emb.weight", "language_emb.weight", "encoder.attn_layers.N.conv_{q,k,v,o}.{weight,bias}",
 * "encoder.attn_layers.N.emb_rel_{k,v}", "encoder.norm_layers_{1,2}.N.{gamma,beta}", "encoder.ffn_layers.N.conv_{1,2}.{weight,bias}",
 * "encoder.spk_emb_linear.{weight,bias}", "proj.{weight,bias}"; float32, in the reference's shapes, copied. */
int dv_tenc_create(const dv_tenc_cfg* cfg, dv_tenc** out);
void dv_tenc_destroy(dv_tenc* t);
int dv_tenc_set_weight(dv_tenc* t, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim);
/* Packs the weights (once per weight set) and plans the launches for B utterances of T tokens (T <= 512, the largest length
 * k_rel_attention is tested at: DV_ERR_INVALID beyond).  precision: DV_PREC_BF16X3; DV_PREC_BF16 is unsupported (DV_ERR_INVALID
 * with a message). */
int dv_tenc_prepare(dv_tenc* t, int32_t B, int32_t T, int32_t precision);
/* ids, tone, language: DEVICE int64 [B, T] (indices outside their table are clamped into it, never read out of bounds: the caller
 * validates); lengths: DEVICE int64 [B], valid tokens per utterance (values outside 0..T are clamped); g: [B, gin_channels] float32
 * or NULL (no speaker conditioning in this call).  Outputs, channels-first as the reference returns them, padding frames
 * exactly zero: x [B, H, T], m [B, C, T], logs [B, C, T].  Allocates nothing and never waits for the device: capturable into a
 * graph. */
int dv_tenc_forward(dv_tenc* t, const int64_t* ids, const int64_t* tone, const int64_t* language, const int64_t* lengths,
                    const float* g, float* x, float* m, float* logs, void* stream);
/* Launches one forward enqueues (the two speaker-conditioning launches included) and the FLOPs of its contractions. */
int dv_tenc_stats(dv_tenc* t, int64_t* n_launch, double* flops);
/* Probe, the contract of dv_penc_probe (channels-last [B, T, C], after a prepare with DVITS_KEEP_INTERMEDIATES=1).  Names: "emb",
 * "layerN.attn" (after conv_o + residual, before LayerNorm 1), "layerN.ln1", "layerN.ffn1" (ReLU'd, masked conv_1 output, joined
 * from its split planes), "layerN" (the layer's output), "proj" (2C statistics channels).  Padding rows hold zeros. */
int dv_tenc_probe(dv_tenc* t, const char* name, float* host_out, int64_t capacity, int64_t* dims);

/* ---- posterior encoder enc_q: PosteriorEncoder.forward, reference model3.py:550-572 (mel frames -> posterior draw) -------
 * The contracts of the dv_tenc_* functions.  Weights under their reference names relative to "enc_q.": "pre.{weight,bias}",
 * "enc.in_layers.N.{weight_g,weight_v,bias}", "enc.res_skip_layers.N.{weight_g,weight_v,bias}", "enc.cond_layer.{weight_g,weight_v,bias}",
 * "proj.{weight,bias}"; float32, in the reference's shapes, copied.  Weight norm (w = weight_g * weight_v / ||weight_v||, the norm
 * per output channel) is folded when the weights are packed. */
int dv_qenc_create(const dv_qenc_cfg* cfg, dv_qenc** out);
void dv_qenc_destroy(dv_qenc* q);
int dv_qenc_set_weight(dv_qenc* q, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim);
/* Packs the weights (once per weight set) and plans the launches for B utterances of T frames.  DV_ERR_INVALID with a message,
 * before anything is launched, for what k_wn_layer (csrc/kernels_wn.hip) does not cover: kernel_size != 5, dilation_rate != 1,
 * hidden_channels != 256, DV_PREC_BF16, T > 16384 (the aligner's limit), B > 65535, B * T > 2^22. */
int dv_qenc_prepare(dv_qenc* q, int32_t B, int32_t T, int32_t precision);
/* y: DEVICE float32 [B, in_channels, T]; lengths: DEVICE int64 [B], valid frames per utterance (values outside 0..T are clamped;
 * a zero-length utterance yields zeros and leaves the others alone); g: [B, gin_channels] float32 or NULL (no speaker
 * conditioning in this call); noise: [B, C, T] float32, the posterior draw.  Outputs channels-first [B, C, T], padding frames
 * exactly zero: z = (m + noise * exp(logs)) * mask, m, logs.  n_layers + 4 launches.  Allocates nothing and never waits for the
 * device: capturable into a graph. */
int dv_qenc_forward(dv_qenc* q, const float* y, const int64_t* lengths, const float* g, const float* noise, float* z, float* m,
                    float* logs, void* stream);
/* Launches one forward enqueues (n_layers + 4, in either mode) and the FLOPs of its contractions. */
int dv_qenc_stats(dv_qenc* q, int64_t* n_launch, double* flops);
/* Measurement aid (tools/qenc_bench.py): replays the n_layers k_wn_layer launches of the last dv_qenc_forward (its buffers and
 * arguments; DV_ERR_STATE without one) `reps` times between two events on `stream`, waits, and returns microseconds per pass of
 * n_layers launches.  lengths (and g) of that forward must still be alive.  The schedule's activations are overwritten with the values the same layers would write again. */
int dv_qenc_time_layers(dv_qenc* q, int32_t reps, void* stream, float* us_per_pass);
/* Probe, the contract of dv_tenc_probe (channels-last [B, T, C], after a prepare with DVITS_KEEP_INTERMEDIATES=1).  Names: "pre",
 * "layerN.acts" (the gated activations tanh * sigmoid, which only this mode writes to memory), "layerN.x" (the residual stream
 * after layer N; not for the last layer, which has no residual half), "layerN.skip" (the running skip sum), "proj" (2C statistics
 * channels).  Padding rows hold zeros. */
int dv_qenc_probe(dv_qenc* q, const char* name, float* host_out, int64_t capacity, int64_t* dims);

/* ---- log-mel front-end: a ragged batch of recordings -> mels in one launch (csrc/kernels_mel.hip) ---- */

/* window: HOST float32 [n_fft], fb: HOST float32 [n_fft / 2 + 1, n_mels] (row = bin) - the buffers mel.MelSpectrogram registers, so
 * both of its backends share the constants bit for bit.  They are copied to device tables together with the FFT twiddles (computed
 * in double on the host, rounded once) and each band's bin range (first and last non-zero row of its fb column; the dense weights
 * inside the range are used, so any filterbank is handled).  A configuration outside dv_mel_cfg's scope, a non-finite table entry:
 * DV_ERR_INVALID with the reason in dv_last_error. */
int dv_mel_create(const dv_mel_cfg* cfg, const float* window, const float* fb, dv_mel** out);
typedef enum { DV_MEL_LOG = 1, DV_MEL_POWER2 = 2 } dv_mel_flags;
/* k_log_mel: wave float32 [B, n_max], n_samples DEVICE int64 [B] -> out float32 [B, n_mels, L_max], frames DEVICE int64 [B].
 * L_max must be 1 + n_max / hop_length; frames[b] = L_b = 1 + n_samples[b] / hop_length.  Frame f of row b is the windowed samples
 * f * hop - n_fft / 2 + j, j < n_fft, reflected about the ROW's own ends (i < 0 -> -i, i >= n_b -> 2 (n_b - 1) - i; no sample at an
 * index >= n_b is read), a 1024-point real DFT in float32, the 513 magnitudes (sqrtf; squared with DV_MEL_POWER2), per mel band the
 * sum of fb[k, m] * mag[k] over the band's bin range in ascending k, and with DV_MEL_LOG logf(fmaxf(v, log_clip)).  Every element at
 * or past L_b is exactly 0.  A row whose n_samples[b] is outside [n_fft / 2 + 1, n_max] is all zeros with frames[b] = 0: a value for
 * the caller to check, not a fault.  Null pointers, B outside 1..65535, n_max outside n_fft / 2 + 1 .. 2^30, a wrong L_max, unknown
 * flag bits, misaligned pointers: DV_ERR_INVALID before anything is launched.  One launch, no allocation, no wait: capturable. */
int dv_mel_forward(dv_mel* h, const float* wave, const int64_t* n_samples, int32_t B, int32_t n_max, float* out, int64_t* frames,
                   int32_t L_max, int32_t flags, void* stream);
void dv_mel_destroy(dv_mel* h);

/* ---- sample-rate conversion: a ragged batch of recordings, each with its own rate pair, in one launch (csrc/kernels_resample.hip) ---- */

/* orig / new_: HOST int32 [n_pairs], the rate pairs a call's rows choose from (Hz or any common unit; reduced by their gcd to o : n).
 * Per pair the filter table of torchaudio.transforms.Resample's documented defaults (sinc_interp_hann, lowpass_filter_width 6,
 * rolloff 0.99): base = min(o, n) * 0.99, width = ceil(6 o / base), K = 2 width + o, for phase p < n and tap j < K
 *   t = clamp((-p / n + (j - width) / o) * base, -6, 6),  h[p][j] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / 12)^2 * base / o,
 * computed in double on the host and rounded once to float32; orig == new: the delta h[0][width] = 1 (the identity, bit for bit).
 * The device table keeps each phase's first non-zero tap, the count up to its last one and the taps between them (any table is
 * handled).  n_pairs outside 1..64, a rate < 1, o or n above 1024 after reduction (the table is staged in LDS): DV_ERR_INVALID with
 * the reason in dv_last_error. */
int dv_resample_create(const int32_t* orig, const int32_t* new_, int32_t n_pairs, dv_resample** out);
/* k_resample: wave float32 [B, n_max], n_samples DEVICE int64 [B], pair DEVICE int32 [B] (index into the handle's pairs; null: every
 * row uses pair 0) -> out float32 [B, n_out_max], n_out DEVICE int64 [B].  n_out_max must be the largest ceil(n * n_max / o) over the
 * handle's pairs (the host computes it; nothing is read back from the device); n_out[b] = ceil(n * n_samples[b] / o) of the row's own
 * pair, written on the device so that it can be passed on as n_samples of dv_mel_forward without a host read.  Row b:
 *   out[b][q n + p] = sum_j h[p][j] x[q o - width + j] over the phase's tap range in ascending j (float32, fmaf),
 * x = 0 outside [0, n_samples[b]) - no sample at an index >= n_samples[b] is read.  Every element at or past n_out[b] is exactly 0.
 * A row whose n_samples[b] is outside [0, n_max] or whose pair[b] is outside [0, n_pairs) is all zeros with n_out[b] = 0: a value for
 * the caller to check, not a fault.  Null pointers (pair excepted), B outside 1..65535, n_max outside 1..2^30, a wrong n_out_max (or
 * one beyond 2^32), misaligned pointers (4 bytes for wave / out / pair, 8 for n_samples / n_out): DV_ERR_INVALID before anything is
 * launched.  One launch, no atomics, no allocation, no wait: capturable; two calls agree bit for bit. */
int dv_resample_forward(dv_resample* h, const float* wave, const int64_t* n_samples, const int32_t* pair, int32_t B, int64_t n_max,
                        float* out, int64_t n_out_max, int64_t* n_out, void* stream);
void dv_resample_destroy(dv_resample* h);

/* ---- single-operator entry points (parity tests of each kernel through the C ABI) ---- */

/* k_rel_attention alone: q, k, v, o float32 [B, T, H*d] (heads interleaved on the last axis), emb_k / emb_v [2*window+1, d] shared
 * by the heads, lengths DEVICE int64 [B].  o_i = softmax_j over the utterance's valid keys of (q_i.k_j + [|j-i| <= window]
 * q_i.emb_k[j-i+window]) / sqrt(d), times v_j, plus the in-range band probabilities times emb_v; rows >= lengths[b] are zeros.
 * d = 32, 64 or 128; T <= 512; window <= 16; 16-byte aligned pointers.  DV_ERR_INVALID otherwise, before anything is launched. */
int dv_op_rel_attention(const float* q, const float* k, const float* v, const float* emb_k, const float* emb_v,
                        const int64_t* lengths, float* o, int32_t B, int32_t H, int32_t T, int32_t d, int32_t window, void* stream);

/* Length regulator of the prior at inference (reference model3.py:840-856), first half (k_dur_scan): logw float32 [B, Tx] (the
 * duration predictor's output), x_lengths DEVICE int64 [B] (clamped to 0..Tx).  w = expf(logw) * [j < x_lengths[b]] * length_scale
 * in float32, cum [B, Tx] int32 = inclusive prefix sums of ceil(w), y_len [B] int64 = max(cum[b, x_lengths[b] - 1], 1).  An utterance
 * with a w that is NaN, infinite, negative or above 2^24, or whose total leaves int32, gets y_len[b] = -1 (its cum row is then
 * unspecified; the other rows are unaffected): a value for the caller to check, not a fault.  length_scale must be finite and
 * >= 0.  Null pointers or B, Tx < 1: DV_ERR_INVALID before anything is launched.  One launch, no allocation, no wait: capturable. */
int dv_op_regulate_lengths(const float* logw, const int64_t* x_lengths, int32_t B, int32_t Tx, double length_scale, int32_t* cum,
                           int64_t* y_len, void* stream);
/* Second half (k_regulate_sample): m_p, logs_p float32 [B, C, Tx], cum as written above, noise float32 [B, C, Tp] ->
 * z_p [B, C, Tp] = m_p[b, c, tok] + (noise[b, c, t] * expf(logs_p[b, c, tok])) * noise_scale, each product and the sum rounded to
 * float32 in that order, tok = the first j < x_lengths[b] with cum[b, j] > t.  A frame without such a token (the padding behind an
 * utterance's frames up to Tp, the single frame of an utterance of zero durations) takes m = logs = 0 as the reference's all-zero
 * alignment row gives them: z_p = noise * noise_scale there.  m_p_exp / logs_p_exp [B, C, Tp] (or NULL) receive the gathered
 * statistics.  Tp is the caller's (max(y_len) in the product).  Null pointers (other than the two optional outputs), B, C, Tx or
 * Tp < 1, B > 65535: DV_ERR_INVALID before anything is launched.  One launch, no allocation, no wait: capturable. */
int dv_op_regulate_sample(const float* m_p, const float* logs_p, const int32_t* cum, const int64_t* x_lengths, const float* noise,
                          double noise_scale, int32_t B, int32_t C, int32_t Tx, int32_t Tp, float* z_p, float* m_p_exp,
                          float* logs_p_exp, void* stream);

/* Forced alignment (csrc/kernels_align.hip; reference model3.py:767-794 and monotonic_align/core.py), scores (k_mas_scores):
 * z float32 [B, C, Ty] (the posterior sample), m_p, logs_p float32 [B, C, Tx] (the prior's statistics), y_lengths / x_lengths DEVICE
 * int64 [B] (clamped to 0..Ty / 0..Tx) -> neg_cent float32 [B, Ty, Tx], with s = exp(-2 logs_p):
 *   sum_c(-0.5 log 2 pi - logs_p) + sum_c(-0.5 z^2 s) + sum_c(z m_p s) + sum_c(-0.5 m_p^2 s)
 * in plain float32, the roundings in the order the kernel's header comment lists: within (C + 6) * 2^-23 * (the sum of the
 * summands' magnitudes) of the exact value.  Cells outside an utterance's y_lengths[b] x x_lengths[b] are written as zeros.
 * Null pointers, a dimension < 1, B > 65535: DV_ERR_INVALID before anything is launched.  One launch, no allocation, no wait. */
int dv_op_mas_scores(const float* z, const float* m_p, const float* logs_p, const int64_t* y_lengths, const int64_t* x_lengths,
                     int32_t B, int32_t C, int32_t Ty, int32_t Tx, float* neg_cent, void* stream);
/* Bytes of device scratch dv_op_mas_path needs at these sizes: 0 while the decision bits fit in LDS (Ty * ceil(Tx / 8) <= 65536:
 * every Ty <= 1024), B * Ty * 64 beyond; -1 for sizes the search refuses (a dimension < 1, Tx > 512, Ty > 16384). */
int64_t dv_op_mas_scratch_bytes(int32_t B, int32_t Ty, int32_t Tx);
/* The monotonic alignment search (k_mas_path, one wave per utterance): neg_cent float32 [B, Ty, Tx] (READ ONLY - the reference
 * accumulates in place), the two DEVICE int64 length arrays -> durations int32 [B, Tx] (frames per token, zeros behind x_lengths[b])
 * and frame_token int32 [B, Ty] (the token of every frame, -1 behind y_lengths[b]).  The integers are exactly those of the
 * reference's routine: one float32 addition per cell, ties stay on the token.  An utterance with x_lengths[b] < 1, y_lengths[b] < 1,
 * x_lengths[b] > y_lengths[b] or a length beyond Tx / Ty is not searched: both its rows are all -1 and the other utterances are
 * unaffected - a value for the caller to check, not a fault.  Scores that are not finite: unspecified path.  scratch: 16-byte aligned
 * device memory of at least dv_op_mas_scratch_bytes(B, Ty, Tx) bytes (may be NULL when that is 0).  Null pointers, a dimension < 1,
 * Tx > 512, Ty > 16384, too little scratch: DV_ERR_INVALID before anything is launched.  One launch, no allocation, no wait. */
int dv_op_mas_path(const float* neg_cent, const int64_t* y_lengths, const int64_t* x_lengths, int32_t B, int32_t Ty, int32_t Tx,
                   int32_t* durations, int32_t* frame_token, void* scratch, int64_t scratch_bytes, void* stream);
/* The same search with two clock stamps per wave (a measuring instantiation; the one above executes none): ticks DEVICE int64 [B, 2]
 * = (the row loop, the whole wave) in ticks of the 100 MHz constant clock; zeros for an utterance that is not searched. */
int dv_op_mas_path_timed(const float* neg_cent, const int64_t* y_lengths, const int64_t* x_lengths, int32_t B, int32_t Ty, int32_t Tx,
                         int32_t* durations, int32_t* frame_token, void* scratch, int64_t scratch_bytes, int64_t* ticks, void* stream);

/* y[B,Cout,T_out] = conv1d(act(x)) on channels-first tensors, through the implicit-GEMM
 * kernel: k = 1 or 3, stride 1/2, padding (k-1)/2, optional nearest upsample to `up_T`
 * frames first (0 = none).  w: [Cout, Cin, k] float32, bias [Cout] or NULL. */
int dv_op_conv1d(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t Cin, int32_t T,
                 int32_t Cout, int32_t k, int32_t stride, int32_t up_T, int32_t precision, void* stream);
/* y[M,N] = x[M,K] @ w[N,K]^T + bias */
int dv_op_linear(const float* x, const float* w, const float* bias, float* y, int32_t M, int32_t K, int32_t N,
                 int32_t precision, void* stream);
/* The same contraction with the result leaving the GEMM epilogue as split bf16 planes (hi = bf16(y), lo = bf16(y - hi);
 * uint16 bit patterns, [M, ldo] each; y_lo ignored in bf16 mode) - the form every contraction of the denoiser hands to the
 * next one - and optionally as fp32 y [M, ldo] as well (NULL: planes only).  Any N and any pitch ldo >= N are legal (the
 * 16-byte plane stores of the epilogue are taken only when N and ldo are multiples of 8: tests/test_gpu_ops.py drives the
 * other paths).  geglu = 1: w = [value rows | gate rows] (N = 2 x N_out, N % 64 == 0; reference unet1d/attention.py GEGLU),
 * the planes receive N_out columns of value * gelu(gate), y must be NULL. */
int dv_op_linear_planes(const float* x, const float* w, const float* bias, float* y, uint16_t* y_hi, uint16_t* y_lo, int32_t M,
                        int32_t K, int32_t N, int32_t ldo, int32_t geglu, int32_t precision, void* stream);
/* The general form of dv_op_linear*: y[M, ldo] = epi(x[M, K] @ w[N, K]^T + bias) on a chosen entry of k_gemm's tile menu.
 *   tile     DV_GT_AUTO (the shape heuristic of the forward) or a DV_GT_* tile, optionally | DV_GT_BK64 (64-deep k-tiles on two
 *            k-groups; the 128x128 tiles are 32 deep only) - what the prepare-time tuner sets
 *   epi      DV_GEMM_STORE; DV_GEMM_RESIDUAL: + res[M, ldres >= N]; DV_GEMM_GEGLU: w = [value rows | gate rows], N % 64 == 0, N / 2
 *            output columns of value * gelu(gate), only on the tiles with a 64-column block per wave (T0, T0S, T1, T2G, T4G)
 *   relu     1: max(., 0) after bias / residual;  rowmask[M] (or NULL): multiplies every row after it.  Not with GEGLU.
 *   K0       0, or 0 < K0 < K: the first K0 columns of x become source 0 and the rest source 1 of one k-segment (the channel
 *            concatenation of the up path).  Every source width is a multiple of 32, of 64 with DV_GT_BK64.
 *   splitk   0; 2 or 3: that many k-slices dumped by one launch and summed by an epilogue-only second; 2 | DV_GEMM_SPLITK_FUSED:
 *            both halves and the epilogue in one launch.  Store and residual epilogues only, K / 64 >= slices.
 *   outputs  fp32 y and / or split bf16 planes y_hi, y_lo (uint16 bit patterns; y_lo is ignored in bf16 mode), all [M, ldo];
 *            x, res and the outputs 16-byte aligned.
 * Every argument is checked before anything is launched (DV_ERR_INVALID with a message: a combination the kernel cannot run is
 * never launched); returns after the stream has drained. */
enum { DV_GT_AUTO = 0, DV_GT_T0 = 1, DV_GT_T1 = 2, DV_GT_T2 = 3, DV_GT_T2S = 4, DV_GT_T2G = 5, DV_GT_T3 = 6, DV_GT_T4 = 7, DV_GT_T4G = 8,
       DV_GT_T0S = 9, DV_GT_BK64 = 0x100 };
enum { DV_GEMM_STORE = 0, DV_GEMM_RESIDUAL = 1, DV_GEMM_GEGLU = 2 };
enum { DV_GEMM_SPLITK_FUSED = 0x100 };
int dv_op_gemm(const float* x, const float* w, const float* bias, const float* res, const float* rowmask, float* y, uint16_t* y_hi,
               uint16_t* y_lo, int32_t M, int32_t K, int32_t N, int32_t K0, int32_t ldo, int32_t ldres, int32_t epi, int32_t relu,
               int32_t tile, int32_t splitk, int32_t precision, void* stream);
/* Which instantiation dv_op_gemm would launch for these arguments (host only, the same checks): variant = BM | BN << 8 | BK << 16 |
 * k-groups << 24, tile_kind = its DV_GT_* menu entry (the heuristic's choice resolved), nsplit = 3 (split bf16: three products per
 * k-step) or 1 (single bf16). */
int dv_op_gemm_variant(int32_t M, int32_t K, int32_t N, int32_t K0, int32_t epi, int32_t tile, int32_t splitk, int32_t precision,
                       int32_t* variant, int32_t* tile_kind, int32_t* nsplit);
/* k_gemm as the implicit-GEMM convolution of the forward (Downsample2D, the size-forced Upsample2D, every convolution the
 * resident-operand kernels refuse), on CHANNELS-LAST tensors in a padded row space: T frames of each of the B utterances exist,
 * Tp_in >= T is the row pitch of the sources, Tp_out >= the output frames that of the result (any value).
 *   sources  x0 [B, Tp_in, c0] and, with c1 > 0, x1 [B, Tp_in, c1]: the channel concatenation [x0 | x1]; rows [T, Tp_in) may hold
 *            anything finite and reach no output.  w [Cout, c0 + c1, taps], taps 1 or 3, padding (taps - 1) / 2; bias [Cout] or NULL.
 *   c_sc > 0 + the 1x1 convolution w_sc [Cout, c_sc, 1] of x_sc [B, Tp_in, c_sc] as a second k-segment; stride 1, DV_UP_NONE only.
 *   mode     stride 1 or 2; up_mode DV_UP_NONE, DV_UP_X2 (nearest to 2 T frames) or DV_UP_SIZE (nearest to up_T frames: source frame
 *            min(floor((float)t * ((float)T / (float)up_T)), T - 1), ATen's rule); upsampling with stride 1 only, up_T = 0 otherwise.
 *            Output frames Tv_out = (T_virt + 2 padding - taps) / stride + 1, T_virt = T, 2 T or up_T.
 *   outputs  fp32 y and / or split bf16 planes y_hi, y_lo (as dv_op_gemm), [B, Tp_out, Cout]: rows [Tv_out, Tp_out) of every utterance
 *            are written as zeros.  stats16 (or NULL): [B * Tp_out / 32, Cout / 16, 2] (sum, squared deviations from the block's own
 *            mean) over the rows that exist of every 32 x 16 block; needs Cout % 16 == 0 and Tp_out = Tv_out rounded up to 32.
 *   tile     as dv_op_gemm; every source width (c0, c1, c_sc) a multiple of 32, of 64 with DV_GT_BK64.  B * Tp_out <= 32768.
 * The operand planes the kernel reads are followed by 32 rows of NaN.  No fragment-major weights are made: the launch always runs on
 * k_gemm.  Every argument is checked before anything is launched (DV_ERR_INVALID with a message); returns after the stream has drained. */
enum { DV_UP_NONE = 0, DV_UP_X2 = 1, DV_UP_SIZE = 2 };
int dv_op_conv_rows(const float* x0, const float* x1, const float* w, const float* bias, const float* x_sc, const float* w_sc, float* y,
                    uint16_t* y_hi, uint16_t* y_lo, float* stats16, int32_t B, int32_t T, int32_t Tp_in, int32_t c0, int32_t c1,
                    int32_t c_sc, int32_t Cout, int32_t taps, int32_t stride, int32_t up_mode, int32_t up_T, int32_t Tp_out, int32_t tile,
                    int32_t precision, void* stream);
/* Which instantiation dv_op_conv_rows would launch (host only, the same shape checks; as dv_op_gemm_variant), and the forced tiles the
 * prepare-time tuner would try on this launch: candidates[0 .. cap) receives them, DV_GT_AUTO (0) behind the last (cap 0: none). */
int dv_op_conv_rows_variant(int32_t B, int32_t T, int32_t Tp_in, int32_t c0, int32_t c1, int32_t c_sc, int32_t Cout, int32_t taps,
                            int32_t stride, int32_t up_mode, int32_t up_T, int32_t Tp_out, int32_t tile, int32_t precision,
                            int32_t* variant, int32_t* tile_kind, int32_t* nsplit, int32_t* candidates, int32_t cap);
/* GroupNorm statistics over a channels-last tensor x[B*T, C]: mean/rstd [B, groups]. */
int dv_op_group_stats(const float* x, float* mean, float* rstd, int32_t B, int32_t T, int32_t C, int32_t groups,
                      float eps, void* stream);
/* softmax(q k^T * d^-0.5 + bias) v on [B, T, H*d] tensors (heads interleaved on the last
 * axis as the reference's .view(B,-1,H,d)); bias [B, Tk] additive or NULL. */
int dv_op_attention(const float* q, const float* k, const float* v, const float* bias, float* o, int32_t B,
                    int32_t H, int32_t Tq, int32_t Tk, int32_t d, void* stream);
/* dv_op_attention with the precision mode as an argument: DV_PREC_BF16X3 is dv_op_attention itself (split-bf16 operands, P as one
 * fp16 plane); DV_PREC_BF16 launches k_attention<., ., 1> as the bf16 fast mode of the forward does - q (pre-scaled), k, v and P each
 * ONE bf16 plane, fp32 accumulation.  Any other precision: DV_ERR_INVALID. */
int dv_op_attention_prec(const float* q, const float* k, const float* v, const float* bias, float* o, int32_t B,
                         int32_t H, int32_t Tq, int32_t Tk, int32_t d, int32_t precision, void* stream);
/* The same operation on the kernel the forward runs (k_attention_frag): k | v become split-bf16 MFMA fragments of 32-key tiles
 * in the layout of the hoisted cross-attention keys / values, bias [B, Tk] (or NULL) becomes log2-domain rows of whole tiles,
 * and the launcher picks its instantiation (waves per workgroup, key split) from the shape as it does in the forward.  d must
 * be a multiple of 16, <= 64. */
int dv_op_attention_frag(const float* q, const float* k, const float* v, const float* bias, float* o, int32_t B,
                         int32_t H, int32_t Tq, int32_t Tk, int32_t d, void* stream);
/* The k = 3, padding 1 convolution of ResnetBlock2D / Upsample2D on the kernels the forward runs it on (k_conv3: Cin <= 512;
 * k_conv3s: wider, or with the folded 1x1 shortcut; k_conv3u: up2), on CHANNELS-LAST tensors in a padded row space:
 *   x [B, Tp, Cin], w [Cout, Cin, 3], bias [Cout] or NULL;  T frames of every utterance exist, Tp >= T is the row pitch (a
 *   multiple of 32, T > Tp - 32); rows [T, Tp) of x may hold anything finite and reach no output frame.
 *   Csc > 0: + the 1x1 convolution w_sc [Cout, Csc, 1] of x_sc [B, Tp, Csc] as a second K segment (bias = the sum of both).
 *   up2 = 0: y [B, Tp, Cout].  up2 = 1: nearest x2 upsampling first, y [B, Tpo, Cout] with 2 T frames, Tpo = 2 T rounded up to 32.
 * Cin a multiple of 128 (128 .. 1024; up2: 128 .. 512), Cout a multiple of 64.  A shape that would run on the general GEMM
 * kernel is an error (-1), never a silent fall-back. */
int dv_op_conv3(const float* x, const float* w, const float* bias, const float* x_sc, const float* w_sc, float* y, int32_t B,
                int32_t Cin, int32_t T, int32_t Tp, int32_t Cout, int32_t Csc, int32_t up2, void* stream);
/* Dynamic thresholding on the kernels the sampler loop runs (k_thr_*): in place on x0_inout [rows, row_numel] (rows in 1..2048,
 * row_numel < 2^31, any 4-byte aligned address), per row s = max(quantile(|x0|, ratio), max_val) - torch.quantile's linear
 * interpolation on float32, the two order statistics found exactly by radix select - and x0 <- clamp(x0, -s, s) / s.  A row
 * with a NaN becomes NaN.  s_out [rows] (device, or NULL) receives s.  ratio outside [0, 1], max_val <= 0 or not finite:
 * DV_ERR_INVALID before anything is launched. */
int dv_op_dynamic_threshold(float* x0_inout, int32_t rows, int64_t row_numel, double ratio, double max_val, float* s_out,
                            void* stream);
/* The guidance combination on the kernel the sampler loop runs (k_cfg_combine): x0_pair [2 rows, row_numel] holds the
 * unconditional predictions in rows 0 .. rows-1 and the conditional ones behind them; out [rows, row_numel] (no overlap with
 * x0_pair) receives fmaf(scale, c - u, u) with the difference rounded to float32 first.  rows in 1..2048, row_numel < 2^31, any
 * 4-byte aligned addresses; a non-finite scale or a bad size: DV_ERR_INVALID before anything is launched. */
int dv_op_cfg_combine(const float* x0_pair, float* out, int32_t rows, int64_t row_numel, double scale, void* stream);
/* The other guidance kernel (k_cfg_pair_in): out[0 .. numel) = out[numel .. 2 numel) = in[0 .. numel), no overlap, any
 * 4-byte aligned addresses, 1 <= numel <= 2^40; DV_ERR_INVALID before anything is launched otherwise. */
int dv_op_cfg_pair_in(const float* in, float* out, int64_t numel, void* stream);
/* The known-frame correction on the kernel the sampler loop runs (k_known_frames): x_inout / known / eps [rows, channels,
 * frames] float32, keep [rows, frames] uint8 (device);  x <- float(alpha) * known + float(sigma) * eps in the kept frames (three
 * float32 roundings), the others are not written.  rows * channels * frames < 2^31, 4-byte aligned float pointers (16-byte
 * aligned ones and frames % 4 == 0 take the vector route); DV_ERR_INVALID before anything is launched otherwise. */
int dv_op_known_frames(float* x_inout, const float* known, const float* eps, const uint8_t* keep,
                       int32_t rows, int32_t channels, int32_t frames, double alpha, double sigma, void* stream);

/* ---- normalisation on the kernels the forward runs (tests/test_gpu_norm_ops.py).  All pointers are device pointers; every
 * argument is checked before anything is launched (DV_ERR_INVALID), the call returns after the stream has drained. ---- */
/* LayerNorm over the last axis of x [M, C] float32 (biased variance, two passes on register-resident rows), C a multiple of 4 up
 * to 2048 (anything else is an error, there is no other kernel), x / gamma / beta / outputs 16-byte aligned.  route:
 *   DV_LN_STATS   k_ln_rows<false>: mean [M], rstd [M] only; every other pointer NULL.
 *   DV_LN_ROWS    k_ln_rows<true>: y [M, C] = (x - mean) * rstd * gamma + beta; gamma, beta, y only.
 *   DV_LN_APPLY   k_ln_apply: y_hi / y_lo [M, C] = split planes of (x - mean) * rstd, no affine (y_lo may be NULL); gamma = beta = NULL.
 *   DV_LN_AFFINE  k_ln_affine: (fma((x - mean) * rstd, gamma, beta)) * rowmask[row] (rowmask [M] or NULL) -> y and / or planes. */
enum { DV_LN_STATS = 0, DV_LN_ROWS = 1, DV_LN_APPLY = 2, DV_LN_AFFINE = 3 };
int dv_op_layer_norm(const float* x, const float* gamma, const float* beta, const float* rowmask, float* y, uint16_t* y_hi,
                     uint16_t* y_lo, float* mean, float* rstd, int32_t M, int32_t C, float eps, int32_t route, void* stream);
/* k_ln_rows<true> with the row re-mapping of the pooled-text sequence: x holds M / rows_per_batch utterances of rows_per_batch
 * rows; row r of utterance b goes to row b * out_rows_per_batch + out_row_off + r of y [M / rows_per_batch * out_rows_per_batch,
 * C].  The other rows of y are not written.  0 <= out_row_off <= out_rows_per_batch - rows_per_batch, M % rows_per_batch == 0. */
int dv_op_layer_norm_into(const float* x, const float* gamma, const float* beta, float* y, int32_t M, int32_t C, float eps,
                          int32_t rows_per_batch, int32_t out_rows_per_batch, int32_t out_row_off, void* stream);
/* The prompt encoder's input stage (k_prompt_pre): prompt [B, C, L] channels-first, keep [B, L] (0 = padding frame: its channels
 * are read as zeros), LayerNorm(C) with affine -> split planes hi / lo [B * L, cpad] (lo may be NULL), columns [C, cpad) zero,
 * key_bias [B, L] = keep ? 0 : -1e30.  A padding frame is a constant row: its planes hold beta.  1 <= C <= cpad <= 512. */
int dv_op_prompt_pre(const float* prompt, const float* keep, const float* gamma, const float* beta, uint16_t* hi, uint16_t* lo,
                     float* key_bias, int32_t B, int32_t C, int32_t L, int32_t cpad, float eps, void* stream);
/* LayerNorm fused across two contractions, as the transformer blocks run it (eps 1e-5):
 *   producer  y1 [M, C] = x [M, K] w1 [C, K]^T + b1 (+ res [M, C]); b1, res may be NULL
 *   consumer  y2 [M, N] = LayerNorm(y1; gamma, beta) w2 [N, C]^T + b2 (b2 may be NULL)
 * fused = 1: the producer's epilogue also writes the raw split planes of y1 and rowstat [M, C / 32, 2] - per 32-column block of a
 * row (sum, squared deviations from the block's own mean) -; the consumer multiplies the raw planes by the gamma-folded weights
 * and finishes rstd * (acc - mean * u) + b' from the partials in its epilogue.  fused = 0: k_ln_apply normalises y1 into planes
 * between the two launches (the DVITS_FUSE_LN=0 schedule); rowstat is not written and may be NULL.  Both routes use the weights
 * as the engine packs them: gamma folded into w2's planes, u[n] = sum_c gamma[c] w2[n, c], beta folded into the bias.
 * K a multiple of 32; C a multiple of 32 up to 512 (the consumer holds at most 16 partials per row). */
int dv_op_linear_ln(const float* x, const float* w1, const float* b1, const float* res, const float* gamma, const float* beta,
                    const float* w2, const float* b2, int32_t M, int32_t K, int32_t C, int32_t N, int32_t fused, float* y1,
                    float* rowstat, float* y2, void* stream);
/* GroupNorm behind a k = 1 contraction in the padded row space of dv_op_conv3 (T frames of B utterances, row pitch Tp a multiple
 * of 32, T > Tp - 32): y [B * Tp, C] = x [B * Tp, K] w [C, K]^T + b (b may be NULL; rows [T, Tp) of x may hold anything finite,
 * the same rows of y are written as zeros), then k_gn_apply (no time scale / shift, no SiLU) -> split planes y_norm_hi / _lo
 * [B * Tp, C] of (y - mean) * rstd * gamma + beta over G groups of channels and the T frames of an utterance (padding rows: beta -
 * mean * rstd * gamma, of no meaning).  route says who writes the statistics k_gn_apply reduces:
 *   DV_GN_STAT16   the GEMM epilogue: per (32-row, 16-column) block (sum, squared deviations from the block's own mean over the
 *                  rows that exist), stats [B * Tp / 32, C / 16, 2].  C / G a multiple of 16.
 *   DV_GN_SLAB     the GEMM epilogue: per 32-row block and column (sum, squared deviations from the column's own mean in the
 *                  block), stats [B * Tp / 32, C, 2].  C / G a multiple of 4; T == Tp (the slab has no padded-row form).
 *   DV_GN_KSTAT16  no statistics in the epilogue; the standalone k_stat16 computes DV_GN_STAT16's words from y.  T == Tp.
 * stats (NULL: not wanted) receives those words.  K a multiple of 32; G <= 64; C / G <= 512. */
enum { DV_GN_STAT16 = 0, DV_GN_SLAB = 1, DV_GN_KSTAT16 = 2 };
int dv_op_linear_gn(const float* x, const float* w, const float* b, const float* gamma, const float* beta, int32_t B, int32_t T,
                    int32_t Tp, int32_t K, int32_t C, int32_t G, float eps, int32_t route, float* y, float* stats,
                    uint16_t* y_norm_hi, uint16_t* y_norm_lo, void* stream);

/* ---- the conditioning path's fp32 kernels in isolation (csrc/kernels_misc.hip), each through the launcher the cond and step
 * schedules call.  Device pointers; every argument is checked before anything is launched (DV_ERR_INVALID), the call returns
 * after the stream has drained. ---- */
/* k_timestep_sincos: t [B] -> out [B, dim] = [cos(t f_j) | sin(t f_j)], f_j = exp(-ln(10000) j / (dim / 2)); dim even. */
int dv_op_timestep_embedding(const float* t, float* out, int32_t B, int32_t dim, void* stream);
/* out [M, N] (row pitch ldo) = act_out(act_in(in [M, K], row pitch ldin) w^T + bias [N]) + add [., N] (row pitch ldo); act = SiLU
 * where silu_in / silu_out is 1; bias and add may be NULL.
 *   route 0  k_small_linear, w [N, K]: one wave per output column; M * K floats must fit 64 KiB of LDS.
 *   route 1  k_small_linear_t, w [K, N] (already transposed): lane per output column, eight k-eighths; K <= 512.  M <= 8 and
 *            9 <= M <= 16 run one chunk of 8 / 16 rows, M > 16 chunks of 8 rows.  add_rows > 0: row r adds add[r % add_rows].
 * A size a launcher refuses is DV_ERR_INVALID with nothing launched. */
int dv_op_small_linear(const float* in, int32_t ldin, const float* w, const float* bias, const float* add, float* out, int32_t ldo,
                       int32_t M, int32_t K, int32_t N, int32_t silu_in, int32_t silu_out, int32_t route, int32_t add_rows,
                       void* stream);
/* The attention pooling of the text states, S = L + 1 rows per utterance.
 *   stage 0  k_mean_token, in place on seq [B, L + 1, D]: row 0 = mean of rows 1..L + pos [D]; seq and pos only.
 *   stage 1  k_pool_attn: q [B, D], kv [B (L + 1), 2 D] (keys | values) -> out [B, D], `heads` heads of D / heads <= 8 channels,
 *            q and k each scaled by (D / heads)^-1/4; q, kv and out only. */
int dv_op_pool_attention(float* seq, const float* pos, const float* q, const float* kv, float* out, int32_t B, int32_t L, int32_t D,
                         int32_t heads, int32_t stage, void* stream);

/* ---- vocoder: Vocos backbone + ISTFT head (csrc/voc.hip, csrc/kernels_voc.hip) --------
 * mel [B, n_mels, T] (the denormalised log-mel) -> wave [B, (T - 1) * hop] float32 and samples [B] int64.  Ragged batches: with
 * lengths [B] (int64, device) every row is its own utterance of L_b frames - filter taps read zeros at t < 0 and t >= L_b, the
 * overlap-add and its envelope use L_b frames, row b holds n_b = (L_b - 1) * hop samples followed by exact zeros, samples[b] = n_b.
 * A row with L_b < 2 or L_b > T is all zeros with samples[b] = 0.  lengths null: every row has T frames.
 * State-dict names as the vocos package publishes them (backbone.*, head.out.*, head.istft.window). */
int dv_voc_create(const dv_voc_cfg* cfg, dv_voc** out);     /* n_fft != 1024, hop != 256, dim / intermediate outside the kernels' range: DV_ERR_INVALID */
void dv_voc_destroy(dv_voc* v);
int dv_voc_set_weight(dv_voc* v, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim);
/* Packs the weights (once per weight set; gamma is folded into pwconv2) and plans the launches for B utterances of T frames.
 * precision: DV_PREC_BF16X3 or DV_PREC_BF16 (the GEMMs; the depthwise convolution, the LayerNorms and the head are fp32 either way). */
int dv_voc_prepare(dv_voc* v, int32_t B, int32_t T, int32_t precision);
/* Enqueues the forward on `stream`: no allocation, no wait, capturable in a hipGraph. */
int dv_voc_forward(dv_voc* v, const float* mel, const int64_t* lengths, float* wave, int64_t* samples, void* stream);
int dv_voc_stats(dv_voc* v, int64_t* n_launch, double* flops);
/* Kept intermediates [B, T, C] (prepare with DVITS_KEEP_INTERMEDIATES=1): embed, norm, l<i>.dwln, l<i>.act, l<i>.out, final, head. */
int dv_voc_probe(dv_voc* v, const char* name, float* host_out, int64_t capacity, int64_t* dims);
/* The vocoder's two kernels in isolation; both return after the stream has drained.
 * dv_op_dwconv_ln: rows x [B * T, C] channels-last, w [C, 7], b / gamma / beta [C] -> LayerNorm(dwconv7(x)) as fp32 y and / or
 * split planes y_hi / y_lo (any may be null, not all); C a multiple of 64 up to 512; 16-byte aligned pointers.
 * dv_op_istft_head: logits [B * T, 1026] (513 log-magnitudes | 513 phases), window [1024] -> wave [B, (T - 1) * 256], samples [B]. */
int dv_op_dwconv_ln(const float* x, const float* w, const float* b, const float* gamma, const float* beta, const int64_t* lengths,
                    int32_t B, int32_t T, int32_t C, float eps, float* y, uint16_t* y_hi, uint16_t* y_lo, void* stream);
int dv_op_istft_head(const float* logits, const float* window, const int64_t* lengths, int32_t B, int32_t T, float* wave,
                     int64_t* samples, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVITS_HIP_H */
