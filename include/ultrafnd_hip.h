/* ultrafnd_hip.h -- C ABI of libultrafnd_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the text+vision fusion train-step hot path of
 * Nuralamsiddik16/Ultrafnd_git.  The reference has no FFI of its
 * own (it is pure Python on torch CPU/MPS); each entry point below names the reference
 * Python interface it replaces (file:line under the reference root).  INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says host;
 *   - row-major, fp32 unless a name says bf16 (bf16 = raw uint16 storage);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     allocates, frees or synchronises (safe inside hipGraph capture);
 *   - return 0 on success, a UFND_ERR_* code otherwise; ufnd_last_error() gives the text;
 *   - buffers are caller-owned; nothing is retained across calls.
 */
#ifndef ULTRAFND_HIP_H
#define ULTRAFND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UFND_OK 0
#define UFND_ERR_INVALID 1 /* bad argument: shape, alignment, null pointer */
#define UFND_ERR_LAUNCH 2  /* HIP launch error */

#define UFND_ABI_VERSION 6

const char* ufnd_last_error(void);
int ufnd_abi_version(void);

/* ------------------------------------------------------------------------------------
 * Device-resident step state (graph-replay safe: hyper-parameters and counters are read
 * from memory, never baked into launches).  Host initialises it with hipMemcpy.
 * ---------------------------------------------------------------------------------- */
typedef struct ufnd_step_state {
  uint64_t step;       /* optimizer steps taken so far (AdamW's t-1); ++ by ufnd_step_advance / ufnd_clip_adamw_step */
  uint64_t seed;       /* dropout key: every mask is drawn from (seed, step + ((uint64_t)micro << 40), layer tag, element) */
  float lr;            /* current learning rate (StepLR writes it between epochs) */
  float weight_decay;
  float beta1, beta2, eps;
  float max_norm;      /* clip_grad_norm_ max_norm; <= 0 disables clipping */
  float grad_scale;    /* multiplied into every gradient before use (1/world for summed DP grads) */
  float loss;          /* out: mean CE loss of the last ufnd_softmax_ce */
  float grad_norm;     /* out: global L2 norm (after grad_scale, before clipping) */
  float clip_coef;     /* out: min(1, max_norm / (grad_norm + 1e-6)) */
  float bc1, bc2_sqrt; /* out: 1-beta1^t, sqrt(1-beta2^t) for the step being applied */
  uint32_t micro;      /* micro-batches already folded into the gradient accumulator since the last optimizer step: ++ by
                        * ufnd_grad_accumulate (given the state), 0 again by whatever advances `step`.  Forward and backward of
                        * micro-batch j of a group both run at micro == j, so its masks differ from every other micro-batch's
                        * and from every other step's; 0 (always, without accumulation) leaves the key at `step` */
  float reserved[2];
} ufnd_step_state;

/* ------------------------------------------------------------------------------------
 * Tier A geometry (configs/model_configs/fusion.yaml:2-7, classifier.yaml:2-17)
 * ---------------------------------------------------------------------------------- */
typedef struct ufnd_dims {
  int hidden;       /* 512; must be a multiple of 256 */
  int text_dim;     /* 768 */
  int audio_dim;    /* 128 */
  int visual_dim;   /* 512 */
  int temporal_dim; /* 256 */
  int gnn_dim;      /* 128 */
  int aux_dim;      /* 2 (0 = classifier without aux) */
  int trees;        /* 6 */
  int depth;        /* 4 (<= 6) */
  int classes;      /* 2 (only 2 is supported) */
  float fusion_dropout; /* 0.1 */
  float clf_dropout;    /* 0.1 */
  float node_dropout;   /* 0.3 */
} ufnd_dims;

/* Parameter (or gradient) pointer table.  The same struct type carries the gradients.
 * Names follow the reference's state_dict.  Three groups must be
 * CONTIGUOUS in memory because the kernels treat them as one stacked matrix:
 *   qkv_w : rows [attn_tv.q, attn_ta.q, attn_tv.k, attn_tv.v, attn_vu.q,
 *                 attn_ta.k, attn_ta.v, attn_vu.k, attn_vu.v] each (hidden x hidden)
 *   qkv_b : the nine biases in the same order
 *   gates : node.trees.{t}.gates.{k} for t-major, k-minor, each (hidden)
 *   thresh: node.trees.{t}.thresh.{k}, same order, one float each
 *   leaf  : node.trees.{t}.leaf_logits, t-major, each (2^depth x classes)
 *   tau   : node.trees.{t}.tau, one float each
 */
typedef struct ufnd_fusion_params {
  float *text_w, *text_b;         /* text_proj      (hidden x text_dim)   cross_modal_transformer.py:96 */
  float *audio_w, *audio_b;       /* audio_proj                                                    :97 */
  float *visual_w, *visual_b;     /* visual_proj                                                   :98 */
  float *temporal_w, *temporal_b; /* temporal_proj                                                 :99 */
  float *gnn_w, *gnn_b;           /* gnn_proj                                                      :102 */
  float *qkv_w, *qkv_b;           /* stacked co-attention projections                              :31-33 */
  float *ev0_w[3], *ev0_b[3];     /* attn_{tv,ta,vu}.evidence_proj.0 (hidden x 3), (hidden)        :34-38 */
  float *ev2_w[3], *ev2_b[3];     /* attn_{tv,ta,vu}.evidence_proj.2 (1 x hidden), (1)                    */
  float *fuse0_w, *fuse0_b;       /* fuse_mlp.0 (2*hidden x 16*hidden)                             :122 */
  float *fuse3_w, *fuse3_b;       /* fuse_mlp.3 (hidden x 2*hidden)                                :125 */
  float *cls_w, *cls_b;           /* classifier (2 x hidden) -- aux head, no grad under the trainer :130 */
} ufnd_fusion_params;

typedef struct ufnd_clf_params {
  float *pre0_w, *pre0_b;     /* pre.0 (hidden x (hidden+aux_dim))   deep_truth_classifier.py:122 */
  float *pre3_w, *pre3_b;     /* pre.3 (hidden x hidden)                                     :125 */
  float *gates, *thresh;      /* NODE gates / thresholds                                     :44-45 */
  float *leaf, *tau;          /* leaf logits, temperature tau per tree                       :41,49 */
  float *bypass_w, *bypass_b; /* bypass (classes x hidden)                                   :137 */
  float *temperature;         /* scalar                                                      :115 */
} ufnd_clf_params;

/* ------------------------------------------------------------------------------------
 * Workspaces.  Sizes depend on the batch size only; the caller allocates `floats`
 * fp32 elements (256-byte aligned) and passes the base pointer to every call of the
 * same batch size.  Forward leaves its saved activations there for backward.
 * ---------------------------------------------------------------------------------- */
size_t ufnd_fusion_workspace_floats(const ufnd_dims* d, int B);
size_t ufnd_clf_workspace_floats(const ufnd_dims* d, int B);

/* ------------------------------------------------------------------------------------
 * CrossModalTransformer.forward                 src/models/fusion/cross_modal_transformer.py:134-210
 *   in : text (B,text_dim) audio (B,audio_dim) visual (B,visual_dim) temporal (B,temporal_dim)
 *        gnn (B,gnn_dim); contiguous rows.  gnn must be given (the reference's fuse_mlp is
 *        built for the 16*hidden concat and rejects a missing gnn_feat, :184-195).
 *   out: fused (B,hidden) with row stride ld_fused (multiple of 4), logits (B,2) or NULL to
 *        skip the aux head, forensic (3,B) = emotion_intensity, semantic_conflict, temporal_delay.
 *   train != 0 applies dropout with the mask keyed by state->{seed,step}.
 * ---------------------------------------------------------------------------------- */
int ufnd_fusion_forward(const ufnd_dims* d, const ufnd_fusion_params* p, const float* text, const float* audio,
                        const float* visual, const float* temporal, const float* gnn, int B, int train,
                        float* workspace, float* fused, int ld_fused, float* logits, float* forensic,
                        const ufnd_step_state* state, void* stream);

/* The two backward entry points take an optional `side_stream` (NULL = everything on `stream`): the
 * dX chain -- the critical path -- stays on `stream`, every dW / parameter-gradient kernel goes to
 * `side_stream`, forked with events as soon as its inputs exist.  `join` != 0 makes `stream` wait for
 * the side work before the call returns control of the stream (pass 0 to keep the overlap going into
 * the next call and join there).  Event record/wait pairs are capturable into a hipGraph.
 *
 * autograd backward of the above (what loss.backward() runs, forensic_trainer.py:291).
 *   d_fused (B,hidden) stride ld_dfused; d_logits (B,2) or NULL.  Writes EVERY gradient in
 *   `g` that can receive one (cls_w/cls_b only when d_logits != NULL; overwritten, not
 *   accumulated).  Inputs get no gradient (they are data). */
int ufnd_fusion_backward(const ufnd_dims* d, const ufnd_fusion_params* p, const ufnd_fusion_params* g,
                         const float* text, const float* audio, const float* visual, const float* temporal,
                         const float* gnn, int B, int train, float* workspace, const float* d_fused,
                         int ld_dfused, const float* d_logits, const ufnd_step_state* state, void* stream,
                         void* side_stream, int join);

/* The same backward in two phases, for a gradient exchange that overlaps backward (data parallel; the reference
 * step is single-process, forensic_trainer.py:285-298).  The flat gradient arena is laid out in gradient-ready
 * order [classifier | fuse_mlp | co-attention | projections]:
 *   UFND_BWD_FUSE_MLP  d_fused -> fuse_mlp.3 -> fuse_mlp.0: their dW / db (incl. the 33.5 MB fuse_mlp.0.weight
 *                      gradient, 2/3 of all gradient bytes) are complete when this call's work has run -- the
 *                      caller starts all-reducing [classifier | fuse_mlp] while
 *   UFND_BWD_REST      computes everything else (co-attention, stacked q/k/v, projections).
 * FUSE_MLP followed by REST writes bit-identical gradients to UFND_BWD_ALL (= ufnd_fusion_backward). */
#define UFND_BWD_ALL 0
#define UFND_BWD_FUSE_MLP 1
#define UFND_BWD_REST 2
/* OR-ed into `phase` (and the `flags` of ufnd_classifier_backward_ex): run the backward WITHOUT the Linear layers' dW / db
 * products -- every other gradient and the whole dX chain as usual.  The caller forms those products from gathered
 * factors (ufnd_head_linear_grads_from_factors below); until then the Linear entries of `g` hold stale values. */
#define UFND_BWD_NO_LINEAR_GRADS 16
int ufnd_fusion_backward_phase(const ufnd_dims* d, const ufnd_fusion_params* p, const ufnd_fusion_params* g,
                               const float* text, const float* audio, const float* visual, const float* temporal,
                               const float* gnn, int B, int train, float* workspace, const float* d_fused,
                               int ld_dfused, const float* d_logits, const ufnd_step_state* state, void* stream,
                               void* side_stream, int join, int phase);

/* ------------------------------------------------------------------------------------
 * DeepTruthClassifier.forward                   src/models/fusion/deep_truth_classifier.py:148-171
 *   fused (B,hidden) stride ld_fused; aux (B,aux_dim) or NULL when aux_dim == 0.
 *   out: logits (B,2), probs (B,2) = softmax(logits / clamp(temperature,0.5,5)).
 *   If `fused` already points at the workspace's input panel (ufnd_clf_input_panel) the
 *   copy is skipped -- the fused train step lets the fusion write there directly.
 * ---------------------------------------------------------------------------------- */
float* ufnd_clf_input_panel(const ufnd_dims* d, float* clf_workspace, int B, int* ld);
int ufnd_classifier_forward(const ufnd_dims* d, const ufnd_clf_params* p, const float* fused, int ld_fused,
                            const float* aux, int B, int train, float* workspace, float* logits, float* probs,
                            const ufnd_step_state* state, void* stream);
/* backward for a gradient arriving at `logits` (the trainer's CE-on-logits loss; temperature
 * and tau get no gradient, deep_truth_classifier.py:41,164-170).  d_fused (B,hidden) stride
 * ld_dfused is written. */
int ufnd_classifier_backward(const ufnd_dims* d, const ufnd_clf_params* p, const ufnd_clf_params* g, int B,
                             int train, float* workspace, const float* d_logits, float* d_fused, int ld_dfused,
                             const ufnd_step_state* state, void* stream, void* side_stream, int join);

int ufnd_classifier_backward_ex(const ufnd_dims* d, const ufnd_clf_params* p, const ufnd_clf_params* g, int B,
                                int train, float* workspace, const float* d_logits, float* d_fused, int ld_dfused,
                                const ufnd_step_state* state, void* stream, void* side_stream, int join, int flags);

/* ------------------------------------------------------------------------------------
 * Factor form of the head's Linear gradients, for a data-parallel gradient exchange that moves FACTORS instead of
 * gradients (the reference step is single-process: forensic_trainer.py:285-298; loss.backward() at :291 is what is
 * being distributed).  All 13 Linear layers of the head (fuse_mlp.0/.3, the nine stacked q/k/v, the five input
 * projections, pre.0/.3: 50.9 of the 51.0 MB of gradient) have dW = dY^T X and db = column sums of dY over the batch
 * rows, so the sum over ranks is the same product over ALL ranks' rows:
 *   1. backward with UFND_BWD_NO_LINEAR_GRADS (both modules);
 *   2. ufnd_head_pack_factors: the rank's dY / X panels out of the two workspaces and the step's inputs into ONE
 *      contiguous pack of ufnd_head_factor_floats(d, B) floats (one launch; 2.5 MB at B = 32, hidden 512);
 *   3. all-gather the packs (rank r's pack at packs + r * rank_stride);
 *   4. ufnd_head_linear_grads_from_factors: the SUMMED dW / db of every Linear over ranks * B rows, written into the
 *      gradient tables in one grouped launch -- two from 128 gathered rows on when (hidden + aux_dim) % 4 != 0 -- (fp32 MFMA; rows in rank order, so every rank computes the same bits).
 * The remaining gradients (gates, thresholds, leaves, bypass, evidence_proj: 21 k floats) are summed by an ordinary
 * all-reduce.  ranks == 1 reproduces the plain backward's dW / db bit for bit.
 * ---------------------------------------------------------------------------------- */
size_t ufnd_head_factor_floats(const ufnd_dims* d, int B);
int ufnd_head_pack_factors(const ufnd_dims* d, const float* text, const float* audio, const float* visual, const float* temporal,
                           const float* gnn, int B, float* fusion_workspace, float* clf_workspace, float* pack, void* stream);
int ufnd_head_linear_grads_from_factors(const ufnd_dims* d, const ufnd_fusion_params* fusion_grads, const ufnd_clf_params* clf_grads,
                                        const float* packs, size_t rank_stride, int ranks, int B, void* stream);

/* ------------------------------------------------------------------------------------
 * The head's train step over BOTH modules in two calls (round 4): forensic_trainer.py:285-291's
 *   logits, _ = model(...); loss = F.cross_entropy(logits, y); loss.backward()
 * with the same kernels and arithmetic as ufnd_fusion_forward -> ufnd_classifier_forward -> ufnd_softmax_ce ->
 * ufnd_classifier_backward -> ufnd_fusion_backward_phase, minus the launches that exist only because those are five calls
 * (classifier input preparation, the CE kernel, the activation backward between the modules, one of the two parameter-gradient
 * launches, the classifier's own weight-gradient launch): 26 -> 21 launches per step at B = 32.  Logits, probabilities, forensic scalars, state->loss, d_logits and every
 * gradient are bit-identical to the five-call sequence.  The fusion writes `fused` straight into the classifier's input panel;
 * the aux head (fusion logits) is not evaluated.  Plain mean CE only (the weighted / label-smoothed criterion keeps the
 * five-call sequence).  `phase` as in ufnd_fusion_backward_phase (UFND_BWD_FUSE_MLP includes the classifier's backward).
 * ---------------------------------------------------------------------------------- */
typedef struct ufnd_head_io {
  const float *text, *audio, *visual, *temporal, *gnn, *aux;   /* the step's inputs (gnn NULL iff dims.gnn_dim == 0, aux NULL iff aux_dim == 0) */
  const int64_t* labels;                                        /* (B) */
  float *fusion_workspace, *clf_workspace;                      /* ufnd_fusion_workspace_floats / ufnd_clf_workspace_floats */
  float *logits, *probs, *forensic;                             /* (B,2), (B,2), (3,B) */
  float* d_logits;                                              /* (B,2): written by the forward, read by the backward */
} ufnd_head_io;
int ufnd_head_forward_loss(const ufnd_dims* d, const ufnd_fusion_params* fusion, const ufnd_clf_params* clf, const ufnd_head_io* io, int B,
                           int train, ufnd_step_state* state, void* stream);
int ufnd_head_backward(const ufnd_dims* d, const ufnd_fusion_params* fusion, const ufnd_fusion_params* fusion_grads, const ufnd_clf_params* clf,
                       const ufnd_clf_params* clf_grads, const ufnd_head_io* io, int B, int train, ufnd_step_state* state, void* stream,
                       void* side_stream, int join, int phase);

/* F.cross_entropy(logits, y), mean reduction, + its gradient (forensic_trainer.py:287).
 * labels int64 (B, 8-B aligned).  loss_rows (B) or NULL: each row's own loss, NOT divided by B; d_logits (B,2) = (softmax - onehot)/B
 * or NULL.  state->loss receives the mean (summed in a fixed order: bit-reproducible).  The row's -log p_c is logf(S) - (l_c - max)
 * with S = sum exp(l_c - max): nothing is rounded at the logits' common magnitude (a shift of both logits changes no output bit as
 * long as the shifted logits are exact). */
int ufnd_softmax_ce(const float* logits, const int64_t* labels, int B, float* loss_rows, float* d_logits,
                    ufnd_step_state* state, void* stream);

/* nn.CrossEntropyLoss(weight=(w0, w1), label_smoothing=eps), mean reduction (normalised by the sum of the
 * target-class weights), + its gradient: the criterion of the integrated trainer variant
 * (src/training/forensic_trainer_integrated.py:154-166).  eps = 0, w = (1, 1) is ufnd_softmax_ce in state->loss and d_logits;
 * loss_rows here are each row's term DIVIDED by the weight sum (they add up to state->loss), B times smaller than ufnd_softmax_ce's. */
int ufnd_softmax_ce_weighted(const float* logits, const int64_t* labels, int B, float w0, float w1, float label_smoothing,
                             float* loss_rows, float* d_logits, ufnd_step_state* state, void* stream);

/* FocalLoss(alpha, gamma), mean reduction, optionally under mixup_criterion, + its gradient: the criterion of the raw-data trainer
 * (src/training/run_train_eval.py:717,1245-1281).  Per row and label y, pt = p_y, q = the other class's softmax probability (taken
 * directly from the row's softmax, not as 1 - pt) and ce = -log pt, by the expressions of ufnd_softmax_ce:
 *   fl(z, y) = alpha q^gamma ce,    d fl / d z_c = alpha (q^gamma + gamma q^(gamma-1) pt ce) (p_c - [c == y]).
 * labels_b NULL (then mix NULL): state->loss = sum_r fl(z_r, ya_r) / B.  Otherwise mix points at two device floats
 * (fl32(lam), fl32(1 - lam)) and every row is mix[0] fl(z_r, ya_r) + mix[1] fl(z_r, yb_r): state->loss is their sum / B.  lam is read
 * on the device: a captured launch serves every draw.  loss_rows (B) or NULL: each row's term, not divided by B; d_logits (B,2) or NULL:
 * the gradient of state->loss.  alpha finite and > 0; gamma == 0 (no power is evaluated: with alpha = 1 and labels_b NULL every output
 * has ufnd_softmax_ce's bits) or 1 <= gamma <= 5.  One workgroup, fixed summation order, no atomics. */
int ufnd_softmax_focal(const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* mix, int B, float alpha, float gamma,
                       float* loss_rows, float* d_logits, ufnd_step_state* state, void* stream);

/* ------------------------------------------------------------------------------------
 * clip_grad_norm_ + AdamW.step over a flat fp32 arena    forensic_trainer.py:292-298,176
 *   grad/param/exp_avg/exp_avg_sq: n floats each (n % 4 == 0, 16-byte aligned).
 *   ufnd_grad_norm : state->grad_norm = ||grad * grad_scale||_2, clip_coef, bias corrections
 *                    for step t = state->step + 1.  partials: >= 1024 floats scratch.
 *   ufnd_adamw_step: p *= 1 - lr*wd; m,v update with g = grad*grad_scale*clip_coef; p -= ...
 *   ufnd_step_advance: state->step += 1, state->micro = 0 (once per optimizer step, after every arena is done).
 * ---------------------------------------------------------------------------------- */
int ufnd_grad_norm(const float* grad, size_t n, float* partials, ufnd_step_state* state, void* stream);
int ufnd_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                    const ufnd_step_state* state, void* stream);
int ufnd_step_advance(ufnd_step_state* state, void* stream);
/* The three calls above (four launches) as ONE call of two launches, for a single arena: the sum of squares (its first
 * block also advances state->step), then AdamW, in which every block re-derives the norm, the clip coefficient and the
 * bias corrections from the partials.  Same arithmetic in the same order: parameters, moments and the published scalars
 * are bit-identical to the three-call form. */
int ufnd_clip_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float* partials,
                         ufnd_step_state* state, void* stream);
/* Gradient accumulation over micro-batches: dst[i] = overwrite ? src[i] : dst[i] + src[i] over n floats (n % 4 == 0, both
 * 16-byte aligned, not overlapping), one streaming launch.  With a state (may be NULL) the launch also does
 * state->micro += 1: one more micro-batch is in the accumulator, and the next one draws other dropout masks.  Enqueue it
 * behind everything that reads the masks of the micro-batch just finished (every side stream joined). */
int ufnd_grad_accumulate(float* dst, const float* src, size_t n, int overwrite, ufnd_step_state* state /* may be NULL */,
                         void* stream);

/* ====================================================================================
 * Tier B -- the frozen, forward-only encoders that produce `text` and `visual`
 * (SURVEY.md 8 rows a10/a11).  bf16 operands on v_mfma_f32_16x16x32_bf16, fp32
 * accumulate, fp32 residual stream, fp32 LayerNorm/softmax statistics.
 * The arithmetic these replace is third-party: transformers' BertModel (called at
 * src/core_blocks/text_blocks.py:79) and CLIPVisionModel (geometry pointer
 * configs/model_configs/semantic.yaml:2); the pooling is the reference's own
 * (text_blocks.py:82-101,126-128).
 * ================================================================================== */
#define UFND_ACT_NONE 0
#define UFND_ACT_GELU 1       /* exact erf GELU (BERT intermediate) */
#define UFND_ACT_QUICK_GELU 2 /* x * sigmoid(1.702 x) (CLIP MLP) */
#define UFND_ACT_GELU_BWD 3       /* ufnd_gemm_bf16_dgrad only: out = acc * GELU'(aux) */
#define UFND_ACT_QUICK_GELU_BWD 4 /* ufnd_gemm_bf16_dgrad only: out = acc * quick_GELU'(aux) */

/* fp32 -> bf16 (round to nearest even); used once per weight tensor. */
int ufnd_cast_bf16(const float* src, void* dst_bf16, size_t n, void* stream);

/* out = act(A W^T + bias) + residual -- every nn.Linear of both encoders.
 *   A (M,K) bf16 row stride lda; W (N,K) bf16 row stride ldw (nn.Linear layout);
 *   bias fp32 (N) or NULL; residual fp32 (M,N) row stride ldr or NULL (added after act);
 *   out_bf16 (M,N) row stride ldo and/or out_f32 (M,N) row stride ldf (either may be NULL).
 *   K % 64 == 0, N % 64 == 0, strides multiples of 8, pointers 16-byte aligned. */
int ufnd_gemm_bf16(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                   float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                   void* stream);

/* Same, with an explicit tile configuration (the encoders pick tiles per compute-unit partition): tile_cfg < 0 =
 * automatic; otherwise the id of a tile built into this library (ufnd_gemm_bf16_tile_info; table in
 * csrc/gemm_bf16_kernel.hpp: block tile, wave grid, LDS ring slots of the A and W operands).  N must be a multiple
 * of the tile width; any other id is rejected with UFND_ERR_INVALID.
 * UFND_GEMM_TILE_PERSISTENT (round 4) names the persistent, software-pipelined form (csrc/gemm_bf16_pp.hpp): one workgroup per
 * compute unit walks 256 x 128 tiles with two accumulator sets -- the epilogue of a tile rides through the K loop of the
 * next one, the LDS-DMA operand stream never drains -- for K = 768, M a multiple of 256, N a multiple of 128, bf16 output
 * only (ufnd_gemm_bf16_ln: folded LayerNorm [+ activation], or the bf16 residual stream with out_stats; no fp32 residual /
 * output); any other call that names it is refused.  Same bits as the table's tiles (tests/test_gpu_gemm_pp.py).  The
 * automatic choice takes it for folded-LayerNorm calls with an activation once a workgroup gets two tiles (the FFN1 Linears
 * of both encoders at encoder lookahead >= 2), and for every supported call with at least three tiles per workgroup whose
 * last round of tiles is at least 93 % full (the configs[3] geometry, 65,536+ rows per launch).  The form addresses A, W,
 * out_bf16, residual_bf16 and out_stats with 32-bit byte offsets: a call that names it with an operand reaching 2^31 bytes
 * ((rows - 1) x stride + width, in bytes) is refused, and the automatic choice does not take such a call. */
#define UFND_GEMM_TILE_PERSISTENT 64
int ufnd_gemm_bf16_ex(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                      float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                      int tile_cfg, void* stream);

/* LayerNorm-aware form: the LayerNorms around a Linear are folded into the GEMM epilogues, so that no
 * LayerNorm kernel (and no normalised copy of the activations) sits between two Linears.
 *   producer side  out_stats (M, N/32, 2): the partial {sum, sum of squares} of every aligned group of 32
 *                  columns of the fp32 output row (N/32 = ufnd_gemm_bf16_stat_parts(M,N,K), <= 24).
 *   consumer side  a_stats (M, a_parts, 2) + colsum (N): A is the bf16 rounding of the UN-normalised rows;
 *                  with W' = W * gamma (rows scaled, rounded to bf16), colsum[n] = sum_k W'[n,k] and
 *                  bias' = b + W beta:  LayerNorm(x) W^T + b = rstd (x W'^T - mean colsum) + bias'.
 *   residual side  r_stats (M, r_parts, 2) + r_gamma, r_beta (N): the residual added is
 *                  LayerNorm(residual) * r_gamma + r_beta (BERT's post-LN stream), computed on the fly.
 * a_stats and r_stats are mutually exclusive per call; partial counts are even, 2..24; statistics are
 * over `width` elements; partial layout and summation order are canonical (independent of the tile the
 * shape selects, no atomics): results are run-to-run identical and a row's outputs do not depend on the
 * batch it is computed in.
 * Accuracy of the folded form.  The consumer multiplies the bf16 rounding of the UN-normalised row, so a common-mode
 * offset of the row is rounded before it is subtracted: relative to the normalised output the error is about
 * (1 + |mean| / std) * 2^-9 (measured: tests/test_gpu_tier_b.py::test_gemm_ln_fold_error_grows_with_the_row_offset).
 * Rows of trained BERT / CLIP streams have |mean| / std well below 1; ufnd_ln_fold_guard (below) reports the largest
 * ratio in a statistics buffer so that a caller can fall back to a materialised LayerNorm (ufnd_layernorm +
 * ufnd_gemm_bf16) when it is not; the folding GEMM itself reports the same ratio through ufnd_gemm_ln.guard (below: the reduction
 * in its prologue, ONE atomicMax per workgroup at the kernel's very end -- an atomic in the prologue sits in front of the K loop's
 * counted vmcnt waits and cost 10 us per launch).  A non-finite statistic reports +inf.
 * Replaces nn.LayerNorm + nn.Linear pairs of the third-party encoders (transformers modeling_bert.py
 * BertSelfOutput / BertOutput, modeling_clip.py CLIPEncoderLayer) behind text_blocks.py:79. */
typedef struct ufnd_gemm_ln {
  const float* a_stats;
  const float* colsum;
  const float* r_stats;
  const float* r_gamma;
  const float* r_beta;
  float* out_stats;
  int a_parts, r_parts;
  float a_eps, r_eps;
  int width;
  int tile_cfg; /* < 0: automatic; otherwise a LayerNorm-aware tile id (ufnd_gemm_bf16_tile_info) or UFND_GEMM_TILE_PERSISTENT */
  /* bf16 residual stream (ABI v3): the residual operand as (M, ldrb) bf16 rows -- the rounding the producing GEMM already
   * wrote for its consumer -- instead of the fp32 `residual` argument (exclusive).  With it and out_f32 = NULL a residual
   * GEMM moves 2 + 2 B per element of the stream instead of 4 + 4 + 2; the stream then carries 8 significant bits per
   * layer (statistics are still taken from the fp32 sums before rounding). */
  const void* residual_bf16;
  int ldrb;
  /* fold guard inside the GEMM (ABI v4; optional, used with a_stats): UFND_FOLD_GUARD_SLOTS floats.  Every workgroup of the
   * launch leaves max(slot, largest |mean| * rstd among the rows it folds) in slot (workgroup id % UFND_FOLD_GUARD_SLOTS) -- the
   * statistics are in its registers at that point anyway, so the guard costs one atomicMax per workgroup at its very end instead
   * of a kernel that re-reads every statistics buffer of the pass (55-75 MB per pass).  The largest
   * ratio any folded row has had since the slots were last zeroed = the maximum over the slots (the caller reduces 4 KB). */
  float* guard;
} ufnd_gemm_ln;
#define UFND_FOLD_GUARD_SLOTS 1024
int ufnd_gemm_bf16_ln(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16,
                      float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                      const ufnd_gemm_ln* ln, void* stream);
/* Number of {sum, sumsq} partials per row that an automatic (tile_cfg < 0) ufnd_gemm_bf16_ln call of this shape writes to
 * out_stats, whichever kernel the dispatch picks for it -- the persistent form included (0 = no statistics epilogue). */
int ufnd_gemm_bf16_stat_parts(int M, int N, int K);

/* *guard = max(*guard, max over rows of |mean| * rstd) for the M rows of a statistics buffer (M, parts, 2) as
 * ufnd_gemm_bf16_ln writes and reads them (partial {sum, sumsq}; statistics over `width` elements). */
int ufnd_ln_fold_guard(const float* stats, int M, int parts, int width, float eps, float* guard, void* stream);

/* The tile table of this library: ids 0 .. ufnd_gemm_bf16_tile_count()-1; ufnd_gemm_bf16_tile_info returns 1 and the
 * block tile (rows x columns) of a tile that is built into the library (ln_aware: usable by ufnd_gemm_bf16_ln), 0 for
 * an id that exists only in the diagnostics library.  Timing ablations, in-kernel stamps and experimental tiles are
 * NOT reachable through this ABI (they live in libultrafnd_hip_diag.so, csrc/diag/). */
int ufnd_gemm_bf16_tile_count(void);
int ufnd_gemm_bf16_tile_info(int tile_cfg, int* bm, int* bn, int* ln_aware);

/* y = LayerNorm(x) * gamma + beta over the last dim (H % 256 == 0, H <= 1024).
 *   x fp32 rows with stride ldx; outputs (M,H) contiguous: bf16 (next GEMM's operand) and/or
 *   fp32 (the residual stream). */
int ufnd_layernorm(const float* x, int ldx, const float* gamma, const float* beta, void* out_bf16, float* out_f32,
                   int M, int H, float eps, void* stream);

/* softmax(Q K^T / sqrt(d) + mask) V for every (batch, head); d = 64.
 *   qkv (B*L, 3*heads*64) bf16 = [Q | K | V] per token (the fused QKV projection's output);
 *   key_mask (B,L) int32, 1 = attend, 0 = masked (HF's additive finfo.min), or NULL;
 *   ctx (B*L, heads*64) bf16. */
int ufnd_attention_bf16(const void* qkv, const int32_t* key_mask, void* ctx, int B, int L, int heads,
                        void* stream);

/* BertSelfAttention of one layer in ONE launch, for 128-token samples: the fused Q/K/V projection of X (B*128, H) bf16
 * with the stacked weight Wqkv (3H, H) / bias (3H) -- optionally of LayerNorm(X) folded exactly as ufnd_gemm_bf16_ln
 * does (ln != NULL with a_stats / colsum / a_parts / a_eps / width; the other fields are ignored) -- followed by
 * ufnd_attention_bf16 on the result, without the (tokens, 3H) round trip through HBM: one workgroup computes one
 * sample's Q | K | V for two heads (a 128 x 384 x H tile), rounds them to bf16 into LDS and runs their attention.
 * Same operations in the same order as the two-launch form: ctx (B*128, H) bf16 is bit-identical to it.
 * L must be 128, heads even; other shapes use the two-launch form.
 * Replaces modeling_bert.py BertSelfAttention (query / key / value Linears + eager attention) behind text_blocks.py:79. */
int ufnd_qkv_attention_bf16(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask, void* ctx, int B, int L,
                            int heads, int ldx, int ldw, const ufnd_gemm_ln* ln, void* stream);

/* Packed rows with the row count on the device (no host synchronisation, fixed launch geometry: hipGraph-capturable; a replay
 * follows whatever mask the captured buffers hold).  HF BertModel computes the padded positions too (text_blocks.py:71-79 pads every
 * string to max_length) and the pooling then ignores them (:82-86).  Sample b of a (B, L) batch keeps its positions 0 .. n_b - 1, n_b = 1 + its last
 * kept position (0 for an all-masked sample): only TRAILING padding is dropped, holes stay as rows and stay masked as keys, so every
 * kept token's value is bit-identical to the padded computation for every mask.  The buffers keep their padded capacity B L; the
 * live row count T = cu_seqlens[B] is read by every kernel at entry, and rows T .. capacity are never read into a live row.
 *   ufnd_text_pack                 (B, L) int32 mask -> cu_seqlens (B + 1) and row_src (capacity): row_src[cu[b] + l] = b L + l
 *   ufnd_bert_embed_live           ufnd_bert_embed of the first *m_live of `capacity` rows: row r is token row_src[r] of ids (B, L), at
 *                                  position row_src[r] % L
 *   ufnd_gemm_bf16_live / _ln_live ufnd_gemm_bf16_ex / ufnd_gemm_bf16_ln over the first *m_live of M rows: M (the capacity) picks
 *                                  the tile and bounds the grid, workgroups past the live tiles exit at entry, the live tiles are
 *                                  spread over every XCD; per-row arithmetic is that of the M-row call (bit-identical rows)
 *   ufnd_text_pack_bins            ufnd_text_pack (L <= 128) + slot bins: sample b takes ceil(n_b / 32) contiguous 32-row slots of a
 *                                  4-slot bin, full bins first; bins (B, 8): slot j of bin i is {cu[b] + 32 s, (b << 10) | (s << 8) | n_b}
 *                                  ({0, -1}: empty), *nbins = the bin count
 *   ufnd_qkv_attention_bf16_packed ufnd_qkv_attention_bf16 with sample b's rows at cu_seqlens[b] .. cu_seqlens[b+1] (key_mask (B, 128))
 *   ufnd_qkv_attention_bf16_bins   ..._packed with one workgroup per bin of ufnd_text_pack_bins (up to four samples) and head pair;
 *                                  the grid keeps B x heads / 2, workgroups of bins past *nbins exit at entry; bit-identical ctx
 *   ufnd_text_pack_tiles           ufnd_text_pack (L <= 128, B <= UFND_TEXT_TILE_MAX_B) + sample tiles: whole samples placed back to back in
 *                                  256-row tiles by first-fit-decreasing on n_b (ties: ascending b; at most UFND_TEXT_TILE_SAMPLES samples per
 *                                  tile, which can only bind where samples of fewer than 16 rows meet), a function of the n_b alone;
 *                                  samples with n_b = 0 take no rows.  tiles ((B + 1) / 2, UFND_TEXT_TILE_INTS), tile t:
 *                                  [0] samples, [1] live rows, [2] units, [3] 0; [4 + 2 j], [5 + 2 j]: sample j's {cu[b], (b << 16) | (r0 << 8)
 *                                  | n_b}, r0 = the tile row of its row 0 (samples in placement order, r0 ascending, n_b descending);
 *                                  [UFND_TEXT_TILE_UNIT0 + u]: attention unit u = j | (q << 8), queries 32 q .. of sample j, sample-major;
 *                                  [UFND_TEXT_TILE_ROWMAP + r]: the global row of tile row r (rows past the live ones: the tile's first
 *                                  row); [UFND_TEXT_TILE_KBIAS + r]: the float key bias of tile row r, 0 where mask keeps the token,
 *                                  -3e38 otherwise (holes, rows past the live ones); *ntiles = the tile count.  bins, nbins (both or
 *                                  neither): ufnd_text_pack_bins' table as well, from the same launch
 *   ufnd_qkv_attention_bf16_tiles  ufnd_qkv_attention_bf16_packed with one workgroup per tile of ufnd_text_pack_tiles and HEAD (a
 *                                  256 x 192 x H tile [q_h | k_h | v_h], any head count); the grid is cap_tiles x heads, workgroups of
 *                                  tiles past *ntiles exit at entry; the key mask is the table's; bit-identical ctx
 *   ufnd_attention_bf16_varlen_masked  ufnd_attention_bf16 per sample over the packed fused-QKV rows: sample b's rows are
 *                                  cu_seqlens[b] .. cu_seqlens[b+1] (at most max_len of them), key_mask (B, max_len) indexed by position
 *                                  (NULL: every key valid); ctx rows are packed like qkv's
 *   ufnd_layernorm_live            ufnd_layernorm over the first *m_live of `capacity` rows
 *   ufnd_masked_meanpool_l2_live   ufnd_masked_meanpool_l2 over the packed rows: the same groups and summation order
 *   ufnd_ln_masked_meanpool_l2_live  ufnd_layernorm_live (fp32 rows) + ufnd_masked_meanpool_l2_live without the rows in between: one
 *                                  workgroup per sample normalises y's rows cu_seqlens[b] .. cu_seqlens[b+1] in registers and adds the
 *                                  ones mask (B, L) keeps, in ufnd_masked_meanpool_l2_live's order; out (B, H) is bit-identical to
 *                                  the two entries', and no row past cu_seqlens[B] is read */
int ufnd_text_pack(const int32_t* mask, int B, int L, int32_t* cu_seqlens, int32_t* row_src, void* stream);
int ufnd_text_pack_bins(const int32_t* mask, int B, int L, int32_t* cu_seqlens, int32_t* row_src, int32_t* bins, int32_t* nbins,
                        void* stream);
int ufnd_bert_embed_live(const int64_t* ids, const int32_t* row_src, const int* m_live, const float* word, const float* pos,
                         const float* type0, const float* gamma, const float* beta, void* x_bf16, float* x_f32, int capacity, int L,
                         int H, int vocab, float eps, void* stream);
int ufnd_gemm_bf16_live(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16, float* out_f32,
                        int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act, int tile_cfg, const int* m_live,
                        void* stream);
int ufnd_gemm_bf16_ln_live(const void* A, const void* W, const float* bias, const float* residual, void* out_bf16, float* out_f32,
                           int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act, const ufnd_gemm_ln* ln,
                           const int* m_live, void* stream);
int ufnd_qkv_attention_bf16_packed(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask, const int32_t* cu_seqlens,
                                   void* ctx, int B, int L, int heads, int ldx, int ldw, const ufnd_gemm_ln* ln, void* stream);
int ufnd_qkv_attention_bf16_bins(const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask, const int32_t* cu_seqlens,
                                 const int32_t* bins, const int32_t* nbins, void* ctx, int B, int L, int heads, int ldx, int ldw,
                                 const ufnd_gemm_ln* ln, void* stream);
int ufnd_attention_bf16_varlen_masked(const void* qkv, const int32_t* cu_seqlens, const int32_t* key_mask, void* ctx, int B, int max_len,
                                      int heads, void* stream);
#define UFND_TEXT_TILE_MAX_B 512
#define UFND_TEXT_TILE_SAMPLES 16
#define UFND_TEXT_TILE_UNITS 24
#define UFND_TEXT_TILE_UNIT0 36
#define UFND_TEXT_TILE_ROWMAP 64
#define UFND_TEXT_TILE_KBIAS 320
#define UFND_TEXT_TILE_INTS 576
int ufnd_text_pack_tiles(const int32_t* mask, int B, int L, int32_t* cu_seqlens, int32_t* row_src, int32_t* tiles, int32_t* ntiles,
                         int32_t* bins, int32_t* nbins, void* stream);
int ufnd_qkv_attention_bf16_tiles(const void* X, const void* Wqkv, const float* bqkv, const int32_t* tiles, const int32_t* ntiles, void* ctx,
                                  int cap_tiles, int heads, int ldx, int ldw, const ufnd_gemm_ln* ln, void* stream);

/* CLIPAttention of one layer in ONE launch, for samples of T <= 64 rows (ViT-B/32 at 224^2: T = 50): ufnd_qkv_attention_bf16's fusion
 * with one workgroup per (256 / T whole samples, head) -- a 256 x 192 x H tile [q_h | k_h | v_h] whose row tiles start every
 * (256 / T) T rows -- and no key mask.  X (N*T, H) bf16, Wqkv (3H, H) / bqkv (3H), ln as ufnd_qkv_attention_bf16 (NULL: plain
 * projection); ctx (N*T, H) bf16 is bit-identical to ufnd_gemm_bf16[_ln] + ufnd_attention_bf16 and the only output.  Nothing past
 * row N*T of X is read.  T outside 1 .. 64 is refused: use the two-launch form.
 * Replaces modeling_clip.py CLIPAttention (q / k / v Linears + eager attention) of the frozen visual encoder. */
int ufnd_qkv_attention_bf16_vit(const void* X, const void* Wqkv, const float* bqkv, void* ctx, int N, int T, int heads, int ldx, int ldw,
                                const ufnd_gemm_ln* ln, void* stream);
int ufnd_layernorm_live(const float* x, int ldx, const float* gamma, const float* beta, void* out_bf16, float* out_f32, int capacity,
                        int H, float eps, const int* m_live, void* stream);
int ufnd_masked_meanpool_l2_live(const float* hidden, const int32_t* mask, const int32_t* cu_seqlens, float* out, int B, int L, int H,
                                 void* stream);
int ufnd_ln_masked_meanpool_l2_live(const float* y, const float* gamma, const float* beta, float eps, const int32_t* mask,
                                    const int32_t* cu_seqlens, float* out, int B, int L, int H, void* stream);

/* BertEmbeddings: LayerNorm(word[ids] + position[0..L) + token_type[0]).  Tables fp32.
 *   ids (B,L) int64 in [0,vocab).  Outputs (B*L,H): bf16 and fp32. */
int ufnd_bert_embed(const int64_t* ids, const float* word, const float* pos, const float* type0, const float* gamma,
                    const float* beta, void* x_bf16, float* x_f32, int B, int L, int H, int vocab, float eps,
                    void* stream);

/* BERTContextEncoder.encode pooling (text_blocks.py:82-86,100): masked mean over tokens
 * (denominator clamp_min 1e-6) then v / (||v|| + 1e-9).  hidden (B,L,H) fp32, mask (B,L) int32. */
int ufnd_masked_meanpool_l2(const float* hidden, const int32_t* mask, float* out, int B, int L, int H,
                            void* stream);

/* BERTContextEncoder.encode_fields (text_blocks.py:108-128): parts (N, M, D) fp32 are the encoded
 * title / OCR / comment vectors of N records, valid (N, M) int32 marks the parts that exist
 * (empty strings are skipped by the reference); out (N, D) = mean of the valid parts, then
 * v / (||v|| + 1e-9); zero vector when a record has no part. */
int ufnd_field_mean_l2(const float* parts, const int32_t* valid, float* out, int N, int M, int D, void* stream);

/* CLIP patch embedding as an im2col-free GEMM operand: frames (N,3,S,S) fp32 ->
 * patches (N*(S/P)^2, 3*P*P) bf16 in the conv weight's (c,ky,kx) order. */
int ufnd_vit_patchify(const float* frames, void* patches_bf16, int N, int image, int patch, void* stream);

/* tokens = pre_layrnorm([class_embedding ; patch_emb] + position_embedding) -> x_f32 (N, P+1, H) and / or its
 * bf16 rounding x_bf16 (at least one of the two; with the bf16 residual stream only x_bf16), and optionally the rows' {sum, sumsq} as two partials per row
 * (stats (N*(P+1), 2, 2): the a_stats operand of ufnd_gemm_bf16_ln for the first layer). */
int ufnd_vit_assemble(const float* patch_emb, const float* cls, const float* pos, const float* gamma,
                      const float* beta, float* x_f32, void* x_bf16, float* stats, int N, int P, int H, float eps,
                      void* stream);

/* per-frame e / (||e|| + 1e-9); then, for F > 1, mean over the F frames of a sample and
 * L2-normalise again (text_blocks.py:126-128 idiom).  e (B*F, D) fp32 -> out (B, D). */
int ufnd_l2norm_frames(const float* e, float* out, int B, int F, int D, void* stream);

/* ------------------------------------------------------------------------------------
 * Batch assembly from the device-resident cache: CachedTensorDataset.__getitem__ +
 * default collate, src/training/forensic_trainer.py:60-83,232-234, and the gnn_Z[global_idx] gather of
 * _forward_batch :240-252.  For every item, dst row r = src row idx[r] (r < B); rows are row_bytes long
 * (a multiple of 8, both sides 8-B aligned and densely packed).  One launch for up to 8 tensors.
 * Indices come from the loader's permutation; an index outside [0, src_rows) is clamped into it.
 * ---------------------------------------------------------------------------------- */
#define UFND_GATHER_MAX_ITEMS 8
typedef struct ufnd_gather_item {
  const void* src;
  void* dst;
  int row_bytes;
  int64_t src_rows;
} ufnd_gather_item;
int ufnd_gather_rows(const int64_t* idx, int B, const ufnd_gather_item* items, int n_items, void* stream);

/* The same launch with mixup_data (src/training/run_train_eval.py:1245-1257) folded in.  perm: n_groups x B int64 (values outside
 * [0, B) are clamped), mix: n_groups x 2 floats (fl32(lam), fl32(1 - lam)), both in device memory; item i belongs to draw
 * g = items[i].group.
 *   kind 0, fp32 rows: dst[r] = fl32(mix[g][0] x[idx[r]]) + fl32(mix[g][1] x[idx[perm[g][r]]]) -- two rounded products and one
 *           rounded sum, what torch computes for lam * x + (1 - lam) * x[index, :]; dst_b is ignored.  16-byte accesses when
 *           row_bytes % 16 == 0 and src, dst are 16-B aligned, 8-byte ones otherwise.
 *   kind 1, labels: dst[r] = src[idx[r]], dst_b[r] = src[idx[perm[g][r]]].
 * Rows as in ufnd_gather_rows (a multiple of 8 bytes, 8-B aligned, dense; source indices clamped into [0, src_rows)).  No
 * destination may overlap a source. */
typedef struct ufnd_mix_item {
  const void* src;
  void* dst;
  void* dst_b;
  int64_t row_bytes;
  int64_t src_rows;
  int kind;
  int group;
} ufnd_mix_item;
int ufnd_gather_mix_rows(const int64_t* idx, const int64_t* perm, const float* mix, int B, const ufnd_mix_item* items, int n_items, int n_groups,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * TemporalSyncNet.align, batched          src/core_blocks/temporal_blocks.py:102-140 (+ _cosine :10-13)
 *   text (B,D), visual (B,Dv) fp32 -> out (B,out_dim): W3 GELU(W0 [t, v^, t-v^, t*v^, cos] + b0) + b3
 *   with v^ = visual zero-padded / truncated to D.  w0 is (hidden, 4D+1) stored with row stride
 *   ufnd_temporal_weight_ld(D) (4D+1 rounded up to a multiple of 4, pad zero); w3 (out_dim, hidden).
 *   workspace: ufnd_temporal_workspace_floats(B, D, hidden) floats.
 *   dropout_p > 0 = the module's train mode: nn.Dropout(p) after the GELU, mask keyed by state->{seed, step} (the
 *   reference's align() is under torch.inference_mode, which does not switch dropout off, and its cache builder never
 *   calls .eval()); dropout_p = 0 (state may be NULL) = eval mode.
 * ---------------------------------------------------------------------------------- */
int ufnd_temporal_weight_ld(int in_dim);
size_t ufnd_temporal_workspace_floats(int B, int in_dim, int hidden);
int ufnd_temporal_align(const float* text, const float* visual, const float* w0, const float* b0, const float* w3,
                        const float* b3, float* workspace, float* out, int B, int in_dim, int vis_dim, int hidden,
                        int out_dim, float dropout_p, const ufnd_step_state* state, void* stream);

/* ------------------------------------------------------------------------------------
 * TemporalSyncNet.forward, the sequence path   src/core_blocks/temporal_blocks.py:141-157, _TinyTCN :16-43
 *   text_seq (B,T,text_dim), vis_seq (B,T,vis_dim) fp32, channel-last; in_ch = text_dim + vis_dim.
 *   Per block i: Conv1d(ch -> hid, kernel, padding 'same', dilation 2^i) -> BatchNorm1d -> GELU -> dropout, added to
 *   its input when the widths match; then out (B,out_dim) = head([mean_t h, max_t h]).
 *   layer.w is the Conv1d weight (hid, ch, kernel) re-packed tap-major: w[h][j*ch + c] = weight[h][c][j], row stride
 *   ufnd_tcn_weight_ld(ch, kernel) (ch*kernel rounded up to a multiple of 4, pad zero).  head_w (out_dim, 2*hid).
 *   train != 0: batch statistics (and the running_mean / running_var update, `momentum`), dropout keyed by `state`;
 *   train == 0: running statistics, no dropout.  Forward only (nothing in the reference trains this module).
 *   workspace: ufnd_tcn_workspace_floats(B, T, in_ch, hid, kernel) floats.
 * ---------------------------------------------------------------------------------- */
typedef struct ufnd_tcn_layer {
  const float *w, *b;                 /* packed conv weight, bias (hid) */
  const float *gamma, *beta;          /* BatchNorm1d weight, bias (hid) */
  float *running_mean, *running_var;  /* (hid); written when train != 0 */
} ufnd_tcn_layer;
int ufnd_tcn_weight_ld(int in_ch, int kernel);
size_t ufnd_tcn_workspace_floats(int B, int T, int in_ch, int hid, int kernel);
int ufnd_tcn_forward(const float* text_seq, int text_dim, const float* vis_seq, int vis_dim, int B, int T,
                     const ufnd_tcn_layer* layers, int n_layers, int kernel, int hid, const float* head_w,
                     const float* head_b, int out_dim, int train, float dropout_p, float momentum, float eps,
                     const ufnd_step_state* state, float* workspace, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Graph side of the trainer's construction: src/training/forensic_trainer.py
 *   build_adj_from_ocr :114-132, SimpleGCN :25-53, ForensicTrainer._pretrain_gnn :214-224.
 * Init-time work in the reference (an O(N^2) Python loop and dense (N,N) products on the CPU).
 * ---------------------------------------------------------------------------------- */

/* adj (N, N) row stride ld: 1 where i == j or Jaccard(set_i, set_j) >= thresh, else 0 (both sets empty ->
 * Jaccard 0).  Phrase sets as CSR: offsets (N+1) int32, tokens = every set's phrase ids, sorted ascending and
 * duplicate-free (any injective phrase -> id map; Jaccard only tests equality).  The comparison is
 * inter / (union + 1e-9) >= thresh in double, as the reference's Python floats do. */
int ufnd_ocr_adjacency(const int32_t* offsets, const int32_t* tokens, int N, double thresh, float* adj, int ld, void* stream);

typedef struct ufnd_gcn_params {
  const float* w1; /* lin1.weight (hid, in_dim) */
  const float* b1; /* lin1.bias   (hid)         */
  const float* w2; /* lin2.weight (out, hid)    */
  const float* b2; /* lin2.bias   (out)         */
} ufnd_gcn_params;

size_t ufnd_gcn_workspace_floats(int N, int in_dim, int hid, int out_dim, int train);

/* SimpleGCN.forward: z = lin2(A_norm @ dropout(gelu(lin1(A_norm @ x)))), A_norm = D^-1/2 (adj + I) D^-1/2 with
 * D = rowsum(adj + I) + 1e-9.  x (N, in_dim), adj (N, N) row stride ld_adj, z (N, out_dim).  dropout_p > 0 =
 * train mode (counter-based mask keyed by state->seed / state->step); in_dim % 4 == 0, hid and out_dim % 32 == 0.
 * adj need not be symmetric (a directed or asymmetrically weighted graph is fine): the backward passes of
 * ufnd_gcn_pretrain_step and ufnd_gnn_backward multiply by A_norm^T, as autograd does. */
int ufnd_gcn_forward(const float* x, const float* adj, int ld_adj, const ufnd_gcn_params* p, float* z, float* workspace, int N,
                     int in_dim, int hid, int out_dim, float dropout_p, const ufnd_step_state* state, void* stream);

/* One step of _pretrain_gnn: forward (train-mode dropout), loss = mse(sigmoid(z head_w^T + head_b), rowsum(adj) /
 * max(1, N)) written to *loss, backward through the GCN, torch.optim.Adam(lr, weight_decay as L2 on the gradient,
 * betas (0.9, 0.999), eps 1e-8) on the GCN parameters only (the head is not in that optimizer).  The four
 * parameter tensors must be ONE flat buffer [w1 | b1 | w2 | b2]; exp_avg / exp_avg_sq have that layout; `step`
 * is 1-based; z receives the forward output of this step. */
int ufnd_gcn_pretrain_step(const float* x, const float* adj, int ld_adj, const ufnd_gcn_params* p, float* exp_avg,
                           float* exp_avg_sq, const float* head_w, const float* head_b, float* z, float* workspace, int N,
                           int in_dim, int hid, int out_dim, float dropout_p, float lr, float weight_decay, int step,
                           const ufnd_step_state* state, float* loss, void* stream);

/* ------------------------------------------------------------------------------------
 * The reference's post graph: src/models/gnn/graph_builder.py
 *   cosine_knn :4-28, add_ocr_overlap_weights :30-45, add_temporal_inconsistency :47-59, build_dense_adj :61-68.
 * ---------------------------------------------------------------------------------- */

/* Floats of the workspace of ufnd_cosine_knn (the normalised, column-padded copy of X); 0 for sizes it refuses. */
size_t ufnd_cosine_knn_workspace_floats(int N, int D, int k);

/* idx (N, k) int32, contiguous: row i's k nearest rows of X (N, D) row stride ldx by cosine similarity, i itself excluded,
 * ordered by (similarity descending, index ascending), so ties go to the lower index.  Every row is divided by
 * (its L2 norm + 1e-9) in fp32; S = Xn Xn^T runs on the exact-fp32 MFMA and is never stored: a workgroup keeps the running
 * lists of its 32 query rows on chip while the columns stream past.  No atomics: two calls give the same bits.
 * 1 <= k <= 64 and k < N; D >= 1, ldx >= D; workspace 16-B aligned. */
int ufnd_cosine_knn(const float* X, int ldx, int N, int D, int k, int32_t* idx, float* workspace, void* stream);

#define UFND_ADJ_KNN 1
#define UFND_ADJ_OCR 2
#define UFND_ADJ_TEMPORAL 4
/* adj (N, N) row stride ld in ONE pass, `flags` = any non-empty subset of the three above, applied in the reference's order:
 *   KNN       adj is overwritten: 1 where j is in idx[i], i is in idx[j] or i == j, else 0 (idx (N, k) from ufnd_cosine_knn).
 *             Without it the entry updates the adj it is given in place.
 *   OCR       i != j with ov = |set_i ^ set_j| > 0: a = (float)((double)a + alpha * log1p((double)ov)).  Sets as CSR, exactly
 *             as for ufnd_ocr_adjacency.
 *   TEMPORAL  i != j: a = fl(a * fl(1 + fl(fl(beta) * fl(|delay_i - delay_j|)))), every operation rounded to fp32
 *             (delay (N) fp32).
 * The diagonal is never weighted.  Pointers of parts not asked for may be NULL. */
int ufnd_dense_adj(const int32_t* idx, int k, const int32_t* offsets, const int32_t* tokens, const float* delay, double alpha,
                   double beta, int N, float* adj, int ld, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * The integrated trainer variant's in-graph GNN: src/training/forensic_trainer_integrated.py
 *   build_adj_from_ocr_sets :77-98 (weighted Jaccard adjacency of the mini-batch), _pack_batch / _forward :203-224,
 *   src/models/gnn/gnn_model.py GNNModel :7-41 (lin1 -> A_norm -> ReLU -> dropout -> A_norm -> lin2), trained WITH the head.
 *   (The reference's `torch.stack([T, A, V, U]).mean(0)` at :205 stacks tensors of widths 768/128/512/256 and raises; the
 *   node feature built here is the 416-wide one that line's own comment and `gnn_in_dim = 416` describe, i.e. the main
 *   trainer's compact slice concat, forensic_trainer.py:193-195.)
 * ---------------------------------------------------------------------------------- */

/* adj (N, N) row stride ld: Jaccard(set_i, set_j) where it is >= thresh, i != j and both sets are non-empty, else 0
 * (zero diagonal).  Sets as for ufnd_ocr_adjacency. */
int ufnd_ocr_adjacency_weighted(const int32_t* offsets, const int32_t* tokens, int N, double thresh, float* adj, int ld, void* stream);

/* out (B, n_text + n_audio + n_visual + n_temporal) = [text[:, :n_text] | audio[:, :n_audio] | visual[:, :n_visual] |
 * temporal[:, :n_temporal]] with every row divided by (its L2 norm + 1e-9)     forensic_trainer.py:193-195 */
int ufnd_node_features(const float* text, int ld_text, const float* audio, int ld_audio, const float* visual, int ld_visual,
                       const float* temporal, int ld_temporal, int n_text, int n_audio, int n_visual, int n_temporal, int B,
                       float* out, void* stream);

size_t ufnd_gnn_workspace_floats(int N, int in_dim, int hid, int out_dim);
/* GNNModel.forward: z (N, out_dim).  dropout_p > 0 = train mode (mask keyed by state->{seed, step}).  The workspace keeps
 * what ufnd_gnn_backward needs. */
int ufnd_gnn_forward(const float* x, const float* adj, int ld_adj, const ufnd_gcn_params* p, float* z, float* workspace, int N,
                     int in_dim, int hid, int out_dim, float dropout_p, const ufnd_step_state* state, void* stream);
/* its autograd backward for a gradient d_z (N, out_dim) at z: the four parameter gradients (overwritten).  Correct for any
 * adj, symmetric or not (the forward leaves A_norm^T in the workspace). */
int ufnd_gnn_backward(const float* x, const ufnd_gcn_params* p, float* g_w1, float* g_b1, float* g_w2, float* g_b2, const float* d_z,
                      float* workspace, int N, int in_dim, int hid, int out_dim, float dropout_p, const ufnd_step_state* state,
                      void* stream);
/* d loss / d text_features (B, text_dim) and d loss / d visual_features (B, visual_dim) out of the workspace a fusion backward
 * has just filled (either pointer may be NULL).  The reference's trainer treats both as cached data
 * (src/training/forensic_trainer.py:60-83); with trainable encoders they are where the encoders' backward starts. */
int ufnd_fusion_feature_grads(const ufnd_dims* d, const ufnd_fusion_params* p, float* workspace, int B, float* d_text, float* d_visual,
                              const ufnd_step_state* state, void* stream);

/* d loss / d gnn_feat (B, gnn_dim) after ufnd_fusion_backward[_phase] has run on `workspace`. */
int ufnd_fusion_gnn_input_grad(const ufnd_dims* d, const ufnd_fusion_params* p, float* workspace, int B, float* d_gnn,
                               const ufnd_step_state* state, void* stream);

/* The gradients at ALL five fusion inputs out of the workspace a fusion backward has just filled, any subset non-NULL
 * (contiguous rows, 16-byte aligned; d_gnn must be NULL when dims.gnn_dim == 0), as ONE grouped launch.  The two entries above
 * are this call with their own subset: the same kernel, the same bits. */
int ufnd_fusion_input_grads(const ufnd_dims* d, const ufnd_fusion_params* p, float* workspace, int B, float* d_text, float* d_audio,
                            float* d_visual, float* d_temporal, float* d_gnn, const ufnd_step_state* state, void* stream);

/* ------------------------------------------------------------------------------------
 * Explanations: gradients with respect to the classifier's INPUTS         src/models/fusion/deep_truth_classifier.py:189-272
 * (feature_importance: gradient x input at the logits; explain_shap's smooth-grad branch: mean |gradient| of probs[:, 1] over
 * a 16-point random walk).  None of these entries takes a gradient table: parameters and the gradient arena are untouched.
 *
 * ufnd_classifier_input_grad: ufnd_classifier_forward (same arguments, same logits / probs), then the gradient of
 *     UFND_TARGET_LOGIT  sum_b logits[b, class_idx]
 *     UFND_TARGET_PROB   sum_b probs[b, class_idx]     (through softmax(logits / clamp(temperature, 0.5, 5)))
 *   with respect to the WHOLE input row [fused | aux]: d_x (B, hidden + aux_dim), row stride ld_dx >= hidden + aux_dim.
 *   The backward is the training backward's dX chain (node_bwd, pre.3, pre.0 over all hidden + aux_dim weight columns)
 *   without a single parameter-gradient launch; train != 0 regenerates the forward's dropout masks from `state`.
 *   If `fused` points at the workspace's input panel (ufnd_clf_input_panel) the panel is used as it stands -- fused AND
 *   aux columns, `aux` is not read -- which is how the walk below feeds it.
 * ---------------------------------------------------------------------------------- */
#define UFND_TARGET_LOGIT 0
#define UFND_TARGET_PROB 1
int ufnd_classifier_input_grad(const ufnd_dims* d, const ufnd_clf_params* p, const float* fused, int ld_fused, const float* aux,
                               int B, int train, int target, int class_idx, float* workspace, float* d_x, int ld_dx,
                               float* logits, float* probs, const ufnd_step_state* state, void* stream);

/* The smooth-grad evaluation points (deep_truth_classifier.py:258-270): a random WALK X_i = X_{i-1} + noise_{i-1} * sigma
 * (that order of operations, no fused multiply-add), X_0 = x0; the N-th draw is never used.  Rows of steps
 * [step0, step0 + steps) are written step-major (row (i - step0) * B + b) straight into the input panel
 * [fused | aux | zero pad] (row stride hidden + 4) of `workspace`, a classifier workspace of steps * B rows, so that
 * ufnd_classifier_input_grad on that panel skips its input copy.
 *   x0 (B, W) stride ld_x0; sigma (W rounded up to 4); noise (N, B, W) with row stride ld_noise, step stride B * ld_noise;
 *   W = hidden + aux_dim; ld_x0 and ld_noise multiples of 4, all pointers 16-byte aligned (16-byte loads and stores). */
int ufnd_smoothgrad_points(const ufnd_dims* d, const float* x0, int ld_x0, const float* sigma, const float* noise, int ld_noise,
                           int B, int N, int step0, int steps, float* workspace, void* stream);

/* Attribution reductions over a gradient panel G (row stride ldg), W columns.  No atomics: a rerun gives the same bits.
 *   UFND_ATTR_SMOOTHGRAD    out[b, j] = (acc + sum_{i < steps} |G[i * B + b, j]|) / divisor, added in step order;
 *                           acc = 0, or out's previous content when `accumulate` != 0 (a walk evaluated in several chunks of
 *                           whole steps); divisor <= 0: no division yet (every chunk but the last).  X, agg, partials unused.
 *   UFND_ATTR_GRAD_X_INPUT  out[b, j] = |G[b, j] * X[b, j]| (steps == 1) and, when agg != NULL, agg[j] = mean_b out[b, j]
 *                           as a fixed-order column reduction: slices of 32 rows -> partials -> one finishing pass in
 *                           ascending slice order.  partials: ((B + 31) / 32) * W floats.
 *   UFND_ATTR_PATH_MEAN     out[b, j] = (acc + sum_{i < steps} G[i * B + b, j]) / divisor: UFND_ATTR_SMOOTHGRAD without the absolute
 *                           value (the SIGNED mean gradient along an integration path), the same accumulate / divisor protocol.
 * Rows of 16-byte aligned panels whose strides are multiples of 4 move as 16-byte words; any other layout by element. */
#define UFND_ATTR_SMOOTHGRAD 0
#define UFND_ATTR_GRAD_X_INPUT 1
#define UFND_ATTR_PATH_MEAN 3 /* (2 is not a mode: it stays refused) */
int ufnd_attribution_reduce(int mode, const float* G, int ldg, const float* X, int ldx, int B, int W, int steps, int accumulate,
                            int divisor, float* out, int ldo, float* agg, float* partials, void* stream);

/* ------------------------------------------------------------------------------------
 * Compute-unit partitions.  The reference runs its step in program order on one queue
 * (src/training/forensic_trainer.py:285-298); here the text encoder, the visual encoder and the
 * head -> exchange -> optimizer chain are concurrent chains on their own HIP streams, each confined to
 * its share of the 256 CUs so that whole-CU GEMM workgroups of different chains do not displace each other.
 *   ufnd_stream_create_cu_mask: *stream_out = a hipStream_t restricted to the CUs whose bits are set in
 *     mask_words (n_words x 32 bits; bit b = logical CU b in the driver's numbering).
 *   ufnd_device_cu_count: CUs of the current device (256 on MI355X), negative on error.
 * ---------------------------------------------------------------------------------- */
int ufnd_stream_create_cu_mask(const uint32_t* mask_words, int n_words, void** stream_out);
int ufnd_stream_destroy(void* stream);
int ufnd_device_cu_count(void);

/* ====================================================================================
 * Tier-B backward (ABI v3; SURVEY.md 8b's *_bwd list).  The reference never trains its encoders
 * (src/core_blocks/text_blocks.py:52 `.eval()`, :63 `inference_mode`), so no reference interface is replaced here: these
 * are the backward forms of the forward entry points above, for TrainConfig.train_encoders.  Parity: torch autograd over
 * oracle/encoders_ref.py, itself checked against the installed third-party classes ("parity unpinned by the reference").
 * bf16 operands, fp32 accumulation; parameter gradients are written in fp32; nothing uses atomics (results are
 * run-to-run identical).
 * ================================================================================== */

/* out (M, N) = dY (M, K) x Wt (N, K)^T [x act'(aux)] [+ residual]: the data gradient of y = x W^T through the TRANSPOSED
 * weight copy Wt = W^T (N = in_features rows of K = out_features).  act = UFND_ACT_GELU_BWD / UFND_ACT_QUICK_GELU_BWD
 * multiplies by the activation's derivative at the pre-activations aux (M, ldaux) bf16 (fused dgrad through FFN1's
 * activation); residual (M, ldr) fp32 adds the gradient arriving over the residual branch.  aux and residual are exclusive. */
int ufnd_gemm_bf16_dgrad(const void* dY, const void* Wt, const float* residual, const void* aux, void* out_bf16, float* out_f32,
                         int M, int N, int K, int lda, int ldw, int ldr, int ldaux, int ldo, int ldf, int act, void* stream);

/* dW (n_out, k_in) fp32 [+]= dYt (n_out, tokens) x Xt (k_in, tokens)^T: the weight gradient of y = x W^T from the transposed
 * activations (ufnd_transpose_bf16; `tokens` padded to a multiple of 64 with zero columns).  The token range is cut into
 * slices (grid = tiles x slices, fp32 partial slabs in `workspace`), a reduce pass adds the slabs in slice order.
 * The workspace query sizes every shape either entry accepts (any n_out >= 1, ufnd_linear_wgrad's 8 <= N < 64 included); it returns 0
 * only for k_in or tokens that are not positive multiples of 64. */
size_t ufnd_gemm_bf16_wgrad_workspace_floats(int n_out, int k_in, int tokens);
int ufnd_gemm_bf16_wgrad(const void* dYt, const void* Xt, float* dW, int n_out, int k_in, int tokens, int lda, int ldb, int ldw,
                         float* workspace, int accumulate, void* stream);

/* A LayerNorm's deferred parameter-gradient finish (ufnd_layernorm_bwd with accumulate = UFND_PARTIALS_DEFER leaves the block
 * partials part[blk][2][H] in its workspace): out0 (H) = dgamma, out1 (H) = dbeta, the nblk blocks added in ascending order. */
typedef struct ufnd_partials_job {
  const float* part;
  int nblk, H;
  float *out0, *out1;
} ufnd_partials_job;
#define UFND_PARTIALS_DEFER 2

/* One Linear's weight and bias gradient from the row-major activations, in THREE launches (round 4; the five-launch sequence
 * ufnd_transpose_bf16 x 2 + column-sum finish + ufnd_gemm_bf16_wgrad + slab reduce stays available):
 *   dW (N, K) fp32 = dY (M, N)^T x X (M, K), db (N) = column sums of dY (NULL: skipped); both OVERWRITTEN.
 *   1. both operand transposes (dYt (N, ldt), Xt (K, ldt), ldt >= M rounded up to 64; zero-padded) + dY's column-sum partials;
 *   2. the NT kernel over the token dimension in slices (slab_workspace: ufnd_gemm_bf16_wgrad_workspace_floats(N, K, Mpad));
 *   3. ONE finish launch: slab reduce of dW, column-sum finish of db (colsum_workspace: ufnd_transpose_colsum_workspace_floats)
 *      and, if `extra` != NULL, a deferred LayerNorm dgamma / dbeta finish.
 * Same arithmetic in the same order as the five-launch sequence: bit-identical gradients.
 * `part`: UFND_WGRAD_ALL, or the two halves for a caller that runs the product beside its data-gradient chain on a second
 * stream: UFND_WGRAD_TRANSPOSE (launch 1: dY and X are free to be overwritten once it has run), then UFND_WGRAD_PRODUCT
 * (launches 2 and 3, same arguments). */
#define UFND_WGRAD_ALL 0
#define UFND_WGRAD_TRANSPOSE 1
#define UFND_WGRAD_PRODUCT 2
int ufnd_linear_wgrad(const void* dY, int lddy, const void* X, int ldx, int M, int N, int K, float* dW, float* db, void* dYt, void* Xt, int ldt,
                      float* slab_workspace, float* colsum_workspace, const ufnd_partials_job* extra, int part, void* stream);

/* bf16 W (rows, ld_w) and W^T (cols, ld_wt) of MANY Linears from their fp32 masters (rows, ld_master) in ONE launch (after an
 * optimizer step).  rows and cols multiples of 64, every pointer 16-B aligned, ld_master % 4 == 0, ld_w % 8 == 0, ld_wt % 8 == 0;
 * tile0 = the item's first 64 x 64 tile in the launch (items sorted by it: tile0 of item i + (rows/64)(cols/64) = tile0 of item i+1);
 * `items_device` is a DEVICE-resident table (it is read by the kernel), total_tiles the sum over the items. */
typedef struct ufnd_refresh_item {
  const void* master;
  void* w;
  void* wt;
  int rows, cols, ld_master, ld_w, ld_wt, tile0;
} ufnd_refresh_item;
int ufnd_refresh_operands(const ufnd_refresh_item* items_device, int n_items, int total_tiles, void* stream);

/* dst (cols, ldd) bf16 = src (rows, lds)^T, columns rows..rows_pad-1 zero; src bf16, or fp32 (src_is_f32: cast on the way --
 * weight masters to transposed operand copies).  colsum != NULL (bf16 sources): colsum (cols) [+]= the column sums of src
 * (bias gradients: db = sum over tokens of dy), two-stage through colsum_ws (ufnd_transpose_colsum_workspace_floats). */
size_t ufnd_transpose_colsum_workspace_floats(int rows_pad, int cols);
int ufnd_transpose_bf16(const void* src, int src_is_f32, int rows, int cols, int lds, void* dst, int ldd, int rows_pad, float* colsum,
                        float* colsum_ws, int colsum_accumulate, void* stream);

/* ufnd_attention_bf16 that also keeps lse (B L, heads) fp32: each query's log-sum-exp of its scaled, masked scores in the
 * log2 domain -- what ufnd_attention_bf16_bwd recomputes P from. */
int ufnd_attention_bf16_lse(const void* qkv, const int32_t* key_mask, void* ctx, float* lse, int B, int L, int heads, void* stream);
/* dqkv (B L, 3H) bf16 = the gradients of the fused q | k | v rows, from dctx (B L, H) bf16, the forward's qkv, ctx and lse.
 * workspace: ufnd_attention_bwd_workspace_floats floats (delta = rowsum(dO o O)).  Three launches (delta; dQ; dK and dV).
 * A masked key of a sample that has a live key gets dK = dV = 0 exactly.  A sample WITHOUT a live key is the forward's uniform
 * average (P = 1 / L over all L keys, lse = the mask constant -3e38, which is how its rows are recognised: lse > -1e30 fails) and
 * is differentiated as such: dV_j = (1 / L) sum_i dO_i for every key, dS = (dP - delta) / (8 L). */
size_t ufnd_attention_bwd_workspace_floats(int B, int L, int heads);
int ufnd_attention_bf16_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, const int32_t* key_mask, void* dqkv,
                            float* workspace, int B, int L, int heads, void* stream);

/* LayerNorm backward: dx = rstd (g - mean(g) - xh mean(g xh)) [+ add], g = dy gamma, xh = (x - mean) rstd, from the LayerNorm's
 * INPUT x (M rows of stride ldx); dx as fp32 and / or bf16 (stride lddx).  dgamma / dbeta (H) [+]= their row sums (two-stage,
 * through `workspace`: ufnd_layernorm_bwd_workspace_floats); both may be NULL (then workspace may be too).
 * accumulate = UFND_PARTIALS_DEFER: only the block partials are written (ufnd_layernorm_bwd_blocks(M) blocks); the caller hands
 * them to ufnd_linear_wgrad (`extra`) or ufnd_row_partials_finish before the workspace is reused -- dgamma / dbeta are not touched. */
size_t ufnd_layernorm_bwd_workspace_floats(int M, int H);
int ufnd_layernorm_bwd_blocks(int M);
int ufnd_row_partials_finish(const ufnd_partials_job* job, int accumulate, void* stream);
int ufnd_layernorm_bwd(const float* x, int ldx, const float* gamma, const float* dy, int lddy, const float* add, int ldadd, float* dx_f32,
                       void* dx_bf16, int lddx, float* dgamma, float* dbeta, float* workspace, int accumulate, int M, int H, float eps,
                       void* stream);

/* out = act(x) over n bf16 elements (act = UFND_ACT_GELU / UFND_ACT_QUICK_GELU; n a multiple of 8): the training forward keeps
 * FFN1's pre-activations (for the fused activation backward of ufnd_gemm_bf16_dgrad) next to their activation. */
int ufnd_act_bf16(const void* x, void* out, size_t n, int act, void* stream);

/* ufnd_masked_meanpool_l2 backward: dhidden (B L, H) from dfeat (B, H) and the forward's inputs. */
int ufnd_masked_meanpool_l2_bwd(const float* hidden, const int32_t* mask, const float* dfeat, float* dhidden, int B, int L, int H, void* stream);
/* ufnd_l2norm_frames backward: de (B F, D) from dfeat (B, D) and the forward's input e. */
int ufnd_l2norm_frames_bwd(const float* e, const float* dfeat, float* de, int B, int F, int D, void* stream);
/* BERT embeddings backward from ds (B L, H) = the gradient of the summed embeddings (ufnd_bert_embed with gamma = beta = NULL
 * returns those sums; their LayerNorm is ufnd_layernorm / ufnd_layernorm_bwd): dword (vocab, H), dpos (max_pos, H),
 * dtype (type_vocab, H) are overwritten. */
int ufnd_bert_embed_bwd(const int64_t* ids, const float* ds, float* dword, float* dpos, float* dtype, int B, int L, int H, int vocab,
                        int max_pos, int type_vocab, void* stream);
/* ViT token assembly backward from ds (N (P + 1), H): dcls (H), dpos (P + 1, H) overwritten; dpe (N P, H) bf16 = the patch rows
 * (the `patch_embed_bwd` of SURVEY 8b is ufnd_gemm_bf16_wgrad on dpe and the patch matrix).  dcls = dpos = NULL: the patch rows
 * only (a data-gradient pass: one launch). */
int ufnd_vit_assemble_bwd(const float* ds, float* dcls, float* dpos, void* dpe_bf16, int N, int P, int H, void* stream);

/* ------------------------------------------------------------------------------------
 * Train-mode dropout of the trainable encoders (HF BertModel / CLIPVisionModel in .train()).
 * No mask is stored: each multiplier is regenerated from Philox4x32-10 keyed by state->seed, with counter
 * (element / 4, tag, state->step) -- a pure function of (seed, step, tag, element).  Element numbering:
 *   attention probabilities  ((b heads + h) L + q) Lp + k,  Lp = L rounded up to a multiple of 4
 *   hidden states (M, H)     row H + col
 * The host descriptor is read at enqueue time; state is a device pointer read by the kernels (graph-replay safe).
 * Every _dropout entry requires 0 < p < 1 (p = 0 is the entry without the suffix).
 * ---------------------------------------------------------------------------------- */
typedef struct ufnd_dropout {
  const ufnd_step_state* state; /* device: seed, step and micro (the key's step word is step + (micro << 40)) */
  float p;                      /* drop probability, 0 < p < 1 */
  uint32_t tag;                 /* the site's stream tag (ranges: csrc/common.hpp) */
} ufnd_dropout;

#define UFND_LN_BWD_DROP_DXB 1  /* the bf16 output (the dense layer's input gradient) is multiplied by the mask; the fp32 one is not */
#define UFND_LN_BWD_DROP_DY 2   /* the incoming dy is multiplied by the mask (LayerNorm followed by dropout) */

/* ufnd_attention_bf16_lse with dropout on the softmax probabilities: ctx = (m o P) V.  lse stays that of the undropped P. */
int ufnd_attention_bf16_lse_dropout(const void* qkv, const int32_t* key_mask, void* ctx, float* lse, int B, int L, int heads,
                                    const ufnd_dropout* drop, void* stream);
/* ufnd_attention_bf16_bwd of the dropped forward (same mask): dV = (m o P)^T dO, dS = P o (m o dO V^T - delta). */
int ufnd_attention_bf16_bwd_dropout(const void* qkv, const void* ctx, const void* dctx, const float* lse, const int32_t* key_mask,
                                    void* dqkv, float* workspace, int B, int L, int heads, const ufnd_dropout* drop, void* stream);
/* Post-LN residual site with dropout on the dense output: y = x + m o d (d = the dense layer's output incl. bias, without its
 * residual); y (M, H) fp32 is stored (the LayerNorm backward's input), then LayerNorm(y) -> out_bf16 and / or out_f32 (stride H). */
int ufnd_dropout_residual_layernorm(const float* x, int ldx, const float* d, int ldd, const float* gamma, const float* beta, float* y,
                                    void* out_bf16, float* out_f32, int M, int H, float eps, const ufnd_dropout* drop, void* stream);
/* LayerNorm followed by dropout: out = m o LayerNorm(x) (BertEmbeddings). */
int ufnd_layernorm_dropout(const float* x, int ldx, const float* gamma, const float* beta, void* out_bf16, float* out_f32, int M, int H,
                           float eps, const ufnd_dropout* drop, void* stream);
/* ufnd_layernorm_bwd with a dropout mask (element row H + col) at `where`: UFND_LN_BWD_DROP_DXB or UFND_LN_BWD_DROP_DY. */
int ufnd_layernorm_bwd_dropout(const float* x, int ldx, const float* gamma, const float* dy, int lddy, const float* add, int ldadd,
                               float* dx_f32, void* dx_bf16, int lddx, float* dgamma, float* dbeta, float* workspace, int accumulate,
                               int M, int H, float eps, const ufnd_dropout* drop, int where, void* stream);

/* ------------------------------------------------------------------------------------
 * Attributions at the encoders' INPUTS (explain.input_attribution): which tokens, which image patches.  The gradient reaches
 * them through the data-gradient chain of the entries above (ufnd_gemm_bf16_dgrad, ufnd_attention_bf16_bwd, ufnd_layernorm_bwd
 * with dgamma = dbeta = NULL, ufnd_vit_assemble_bwd with dcls = dpos = NULL): no parameter gradient is formed anywhere.
 * No atomics: every sum below runs in a fixed order.
 * ---------------------------------------------------------------------------------- */

/* Points of a straight path: out[k, r, :] = base[r, :] + alphas[k] (x[r, :] - base[r, :]), k < n_points (out: n_points panels of
 * rows x width, point-major).  alphas is a HOST array, read at enqueue time; base = NULL is the zero baseline.  width a multiple of 4,
 * dense 16-byte aligned panels.  Serves the text encoder's embedding sums (B L x H) and the frames (B F x 3 S S). */
#define UFND_PATH_MAX_POINTS 64
int ufnd_path_points(const float* x, const float* base, const float* alphas, int n_points, size_t rows, int width, float* out,
                     void* stream);

/* Per token row r < R: score[r] = sum_h g[r, h] (s[r, h] - base[r, h]) and grad_norm[r] = ||g[r, :]||_2, one wave per row.
 * mask (R) int32 or NULL: rows with mask 0 are written as exactly 0.  H and the strides multiples of 4, 16-byte aligned panels. */
int ufnd_token_attribution(const float* g, int ldg, const float* s, int lds, const float* base, int ldb, const int32_t* mask, int R, int H,
                           float* score, float* grad_norm, void* stream);

/* The inverse of ufnd_vit_patchify's layout for a gradient panel dpatches (N (S/P)^2, 3 P P) fp32, columns in (c, ky, kx) order:
 *   grad (N, 3, S, S)        the gradient at the pixels,
 *   pixels (N, 3, S, S)      grad * (x - base)  (base = NULL: zero baseline),
 *   patch_sums (N, (S/P)^2)  each patch's sum of `pixels`,
 * any subset (NULL = not written); pixels and patch_sums need x (N, 3, S, S).  patch a multiple of 4. */
int ufnd_vit_unpatchify_attribution(const float* dpatches, const float* x, const float* base, float* grad, float* pixels, float* patch_sums,
                                    int N, int image, int patch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Audio encoder (wav2vec2-base geometry; csrc/audio.hip, ultrafnd_git_amd/audio.py).  Frames are rows, channel-last, in
 * per-clip slabs: after conv0 clip b owns rows b S1 .. b S1 + T1_b - 1 of a (B S1, 512) bf16 buffer (S1 a multiple of 64), every
 * stride-2 layer halves the slab.  A valid output row reads valid input rows only; slab-tail rows hold garbage nothing valid reads.
 * Every reduction below runs a fixed tree that depends on the clip's own length only: a clip's results do not depend on its batch.
 * ------------------------------------------------------------------------------------------- */
#define UFND_AUDIO_MIN_SAMPLES 400      /* one output frame of the seven-layer feature extractor */
#define UFND_WAVE_CHUNK 4096            /* samples per partial of ufnd_wave_normalize */
#define UFND_CONV0_CHUNK 256            /* frames per partial of ufnd_w2v2_conv0 */

/* Wav2Vec2FeatureExtractor(do_normalize): out[b, i] = (wave[b, i] - mean_b) / sqrt(var_b + 1e-7) for i < lengths[b] (population
 * variance over the clip's own samples; samples past lengths[b] are neither read nor written).  wave, out (B, n_max) fp32;
 * lengths (B) int32 on the device, each in [UFND_AUDIO_MIN_SAMPLES, n_max]; ws: 3 B ceil(n_max / UFND_WAVE_CHUNK) floats.
 * Partials per chunk are {centre, sum, sum of squares about the centre} in fp32, the centre being the chunk's own fp32 mean (formed
 * inside the workgroup first), combined in float64 (Chan): the accuracy does not depend on where in a chunk an outlier sits. */
int ufnd_wave_normalize(const float* wave, const int32_t* lengths, float* out, float* ws, int B, int n_max, void* stream);

/* Layer 0 of the feature extractor: Conv1d(1 -> 512, k = 10, s = 5, no bias) + GroupNorm(512, 512) (per clip and channel over
 * the clip's T1_b = (lengths[b] - 10) / 5 + 1 frames, biased variance, affine) + GELU.  Two passes that both recompute the conv
 * from the wave: the fp32 conv output is never stored.  Statistics as in ufnd_wave_normalize, per chunk of UFND_CONV0_CHUNK frames
 * about the conv of the chunk's mean window (the conv is linear: that is each channel's mean over the chunk).  wave (B, n_max) fp32 (normalised); w (512, 10); out_bf16 rows b S1 + t;
 * out_f32 (optional, tests): the same rows before the bf16 rounding.  ws: 3 B 512 ceil(S1 / UFND_CONV0_CHUNK) + 2 B 512 floats. */
int ufnd_w2v2_conv0(const float* wave, const int32_t* lengths, const float* w, const float* gamma, const float* beta, void* out_bf16,
                    float* out_f32, float* ws, int B, int n_max, int S1, float eps, void* stream);

/* A strided Conv1d over frames-as-rows as ONE bf16 GEMM with an overlapping-row A operand (no unfold buffer): output row r is
 * act(W . A[r lda .. r lda + K) + bias), i.e. ufnd_gemm_bf16 with lda < K allowed (lda = stride C, K = k C, W tap-major (N, k C)).
 * The caller owns the rows past M the last rows read: A must hold (M - 1) lda + K elements.  lda % 8 == 0, K % 64 == 0,
 * N % 64 == 0; same kernel and tile choice as ufnd_gemm_bf16 (whose entries keep requiring lda >= K). */
int ufnd_conv1d_rows_bf16(const void* A, const void* W, const float* bias, void* out_bf16, float* out_f32, int M, int N, int K, int lda,
                          int ldw, int ldo, int ldf, int act, void* stream);

/* Positional conv, step 1: x (B S, 768) bf16 -> 16 group-major, edge-padded panels packed[g] (Mp, 48) bf16, Mp = B Sp + 128,
 * Sp = S + 128: row b Sp + 64 + t of panel g = x[b S + t, 48 g .. 48 g + 47] for t < frames[b], zero for every other row of the
 * clip's Sp rows (the conv's zero padding sits at the CLIP's edges) and for the 128 spare rows behind the last clip, which the
 * last rows of the GEMM below read: every row of every panel is written, nothing depends on what `packed` held.  Conv1d(768, 768, k = 128, pad = 64, groups = 16) is then 16
 * ufnd_conv1d_rows_bf16 calls with lda = 48, K = 6144, N = 64 (48 padded). */
int ufnd_w2v2_pos_pack(const void* x_bf16, const int32_t* frames, void* packed, int B, int S, void* stream);
/* Step 2: y[b S + t, 48 g + o] = x[b S + t, 48 g + o] + conv[g][b Sp + t][o] for t < frames[b] (conv (16, B Sp, 64) fp32 holds
 * GELU(conv + bias)), zero for the slab's other rows (so that nothing downstream of here reads garbage). */
int ufnd_w2v2_pos_add(const float* x, const float* conv, const int32_t* frames, float* y, int B, int S, void* stream);

/* frames[b] = the feature extractor's output length for lengths[b] samples; key_mask (B, S) = 1 for t < frames[b]. */
int ufnd_w2v2_frames(const int32_t* lengths, int32_t* frames, int32_t* key_mask, int B, int S, void* stream);

/* out.mean(dim=1) over a clip's valid frames: ufnd_masked_meanpool_l2's first phase (same grouping, same order), no L2. */
int ufnd_masked_meanpool(const float* hidden, const int32_t* mask, float* out, int B, int L, int H, void* stream);

/* Y (M, N) = X (M, K) W^T + bias in exact fp32 (the skinny-GEMM family of the head; N % 32 == 0, 16-B aligned rows). */
int ufnd_linear_f32(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, void* stream);

/* -------------------------------------------------------------------------------------
 * CLIP text tower (CLIPTextModelWithProjection, ViT-B/32 geometry: hidden 512, 8 heads x 64, 12 pre-LN quick-GELU layers, 77
 * positions) and the text-image semantic analyzer (src/models/semantic_forgery.py).  Frozen, forward only.  The layers are the
 * entries above (ufnd_gemm_bf16[_live], ufnd_layernorm[_live]) around the causal attention; csrc/clip_text.hip holds the rest.
 *
 * Causal attention: ufnd_attention_bf16 / ufnd_attention_bf16_varlen_masked with key k visible to query q iff k <= q and
 * key_mask (NULL: all ones; (B, L) resp. (B, max_len) int32) keeps it.  Precondition: key 0 of every sample is kept, so that
 * every query sees a key; a row whose every visible key is masked is unspecified.  A workgroup never reads a key block past its
 * last query.
 *
 * The live-row pass.  Under the causal mask no row after a sample's pooled position e(b) can influence row e(b), so the tower
 * runs over rows 0 .. e(b) of each sample only:
 *   ufnd_clip_text_pack   ids (B, L) int64 -> e (B): the pooled position by HF's rule -- eos_token_id == 2: the first position of
 *                         the largest id (argmax), otherwise the first position equal to eos_token_id (0 if there is none);
 *                         cu_seqlens (B + 1) with cu[b+1] - cu[b] = e[b] + 1, cu[B] = the live row count (the m_live of the
 *                         *_live entries); row_src[cu[b] + l] = b L + l.  One workgroup, a wave per sample, a fixed-order scan.
 *   ufnd_clip_text_embed[_live]  x = token_embedding[id] + position_embedding[l] -> x_f32 and its bf16 rounding x_bf16 (both
 *                         required); ids outside [0, vocab) are clamped; L <= max_position.  _live: over the first *m_live of
 *                         `capacity` packed rows (row r is token row_src[r]).
 *   ufnd_clip_text_pool   final_layer_norm of row e(b) of each sample -> out_bf16 (B, H), the A operand of the text_projection
 *                         GEMM.  cu_seqlens NULL: x is the padded (B L, H) stream, row b L + e[b]; otherwise the packed one, row
 *                         cu_seqlens[b+1] - 1.
 * H in {256, 512, 768, 1024}; B <= 16384 for the pack. */
int ufnd_attention_bf16_causal(const void* qkv, const int32_t* key_mask, void* ctx, int B, int L, int heads, void* stream);
int ufnd_attention_bf16_causal_varlen(const void* qkv, const int32_t* cu_seqlens, const int32_t* key_mask, void* ctx, int B, int max_len,
                                      int heads, void* stream);
int ufnd_clip_text_pack(const int64_t* ids, int B, int L, int eos_token_id, int32_t* e, int32_t* cu_seqlens, int32_t* row_src, void* stream);
int ufnd_clip_text_embed(const int64_t* ids, const float* token_embedding, const float* position_embedding, void* x_bf16, float* x_f32, int B,
                         int L, int H, int vocab, int max_position, void* stream);
int ufnd_clip_text_embed_live(const int64_t* ids, const int32_t* row_src, const int* m_live, const float* token_embedding,
                              const float* position_embedding, void* x_bf16, float* x_f32, int capacity, int L, int H, int vocab,
                              int max_position, void* stream);
int ufnd_clip_text_pool(const float* x, const int32_t* e, const int32_t* cu_seqlens, const float* gamma, const float* beta, void* out_bf16, int B,
                        int L, int H, float eps, void* stream);

/* SemanticForgeryAnalyzer's head, eval-mode arithmetic, all fp32: t = GELU(text Wt^T + bt), i = GELU(image Wi^T + bi) (exact erf),
 * out_text = l2n(t), out_image = l2n(i), out_gap = l2n(t - i) with l2n(x) = x / (||x|| + 1e-9).  text / image (B, K), Wt / Wi
 * (D, K), outputs (B, D); D % 32 == 0, K % 4 == 0, 16-B aligned rows; workspace: 2 B D floats (the pre-activations).  The two
 * products are one launch of the exact-fp32 skinny GEMM (ufnd_linear_f32's kernels). */
int ufnd_semantic_head(const float* text, const float* image, const float* wt, const float* bt, const float* wi, const float* bi,
                       float* workspace, float* out_text, float* out_image, float* out_gap, int B, int D, int K, void* stream);

/* similarity[b] = <t_b, i_b> / ((||t_b|| + 1e-9) (||i_b|| + 1e-9)), clamped to [-1, 1]: the diagonal of CLIPModel's logits_per_text without
 * logit_scale; conflict[b] = 1 - (similarity[b] + 1) / 2 in [0, 1].  text / image (B, D) fp32, D % 4 == 0. */
int ufnd_clip_similarity(const float* text, const float* image, float* similarity, float* conflict, int B, int D, void* stream);

/* -------------------------------------------------------------------------------------
 * The RoBERTa emotion classifier (RobertaForSequenceClassification: post-LN BERT layers, learned positions offset by the pad id,
 * a tanh head on the <s> row) and AffectiveForensics (src/models/affective_forensics.py).  Frozen, forward only.  The layers are
 * the text pass's entries above; csrc/affective.hip holds the rest.
 *
 *   ufnd_roberta_pack     ids (B, L) int64, mask (B, L) int32 -> pos_ids (B L) int32 by HF's create_position_ids_from_input_ids:
 *                         cumsum(ids != pad) * (ids != pad) + pad, taken over the ids, not the mask; valid (B, optional): 1 where the
 *                         mask keeps a token; and, when cu_seqlens / row_src are given (both or neither), exactly what
 *                         ufnd_text_pack writes.  One workgroup, a wave per sample: a fixed-order wave prefix scan across 64-token
 *                         chunks, no atomics.  Without cu_seqlens it is the position-id launch that goes with ufnd_text_pack_bins /
 *                         ufnd_text_pack_tiles (L == 128) and with the padded pass.  B <= 16384.
 *   ufnd_roberta_embed[_live]  LayerNorm(word[id] + position[pos_ids] + token_type[0]) -> x_bf16 and / or x_f32.  Ids are clamped
 *                         into [0, vocab), position ids into [0, max_position); L <= max_position - pad_token_id - 1 is required
 *                         (what the rule can produce then fits the table).  _live: over the first *m_live of `capacity` packed
 *                         rows (row r is token row_src[r]).  H in {256, 512, 768, 1024}.
 *   ufnd_gather_class_rows  the class (<s>) row of each sample -- stream row cu_seqlens[b], or b L when cu_seqlens is NULL -- of up to
 *                         four row-indexed buffers into compact B-row ones: ctx and res_bf16 (bf16, H columns), res_f32 (fp32, H
 *                         columns), stats (fp32, stat_floats per row: a folded LayerNorm's partials).  A source and its destination
 *                         go together; absent pairs are NULL.  A sample without rows (cu[b] == cu[b+1]) gets zeros.  `capacity`:
 *                         the sources' row count (a row index outside it is treated as "no rows").  This is what the last layer of
 *                         a sequence classifier runs over past its attention.
 *   ufnd_emotion_head     all fp32: z = x Wd^T + bd on the exact skinny GEMM (ufnd_linear_f32's kernels; workspace: B H floats), then
 *                         one launch, one workgroup per sample, fixed-order reductions: logits = tanh(z) Wo^T + bo (B, C), class_probs
 *                         = softmax(logits), the group sums f, a, j by `group` (C int32: -1 none, 0 fear, 1 anger, 2 joy, 4 + m for a
 *                         label in several groups, m = bit 0 fear | bit 1 anger | bit 2 joy), probs (B, 3) = [f, a, j] / (f + a + j +
 *                         1e-9), text_intensity = sigmoid(2.5 (f + a - 0.5 j)), intensity = clip(0.6 text_intensity + 0.4 arousal, 0,
 *                         1) (arousal NULL: 0.5), valence = clip(0.5 + 0.5 (j - 0.5 (f + a)), 0, 1).  text_valid (B int32, optional): 0
 *                         marks a sample without text -- its features count as zero (z = bd) and its probs are 0.  probs,
 *                         text_intensity, intensity, valence: all four (with group) or none.  x (B, H), Wd (H, H), Wo (C, H);
 *                         H % 32 == 0, H <= 1024, C <= 32, B <= 65535.
 *   ufnd_audio_arousal    waves (B, T) fp32, lengths (B int32, NULL: T; clamped to [0, T]) -> clip(sigmoid(5 mean(x^2)), 0, 1): the
 *                         reference's RMS-energy branch.  One workgroup per clip, a fixed-order tree, a clip is computed as if
 *                         alone; length 0 gives sigmoid(0). */
int ufnd_roberta_pack(const int64_t* ids, const int32_t* mask, int B, int L, int pad_token_id, int32_t* cu_seqlens, int32_t* row_src,
                      int32_t* pos_ids, int32_t* valid, void* stream);
int ufnd_roberta_embed(const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos, const float* type0, const float* gamma,
                       const float* beta, void* x_bf16, float* x_f32, int B, int L, int H, int vocab, int max_position, int pad_token_id, float eps,
                       void* stream);
int ufnd_roberta_embed_live(const int64_t* ids, const int32_t* pos_ids, const int32_t* row_src, const int* m_live, const float* word, const float* pos,
                            const float* type0, const float* gamma, const float* beta, void* x_bf16, float* x_f32, int capacity, int L, int H,
                            int vocab, int max_position, int pad_token_id, float eps, void* stream);
int ufnd_gather_class_rows(const int32_t* cu_seqlens, const void* ctx, void* ctx_out, const void* res_bf16, void* res_bf16_out, const float* res_f32,
                           float* res_f32_out, const float* stats, float* stats_out, int B, int L, int H, int stat_floats, int capacity, void* stream);
int ufnd_emotion_head(const float* x, const float* wd, const float* bd, const float* wo, const float* bo, const int32_t* group,
                      const int32_t* text_valid, const float* arousal, float* workspace, float* logits, float* class_probs, float* probs,
                      float* text_intensity, float* intensity, float* valence, int B, int H, int C, void* stream);
int ufnd_audio_arousal(const float* waves, const int32_t* lengths, float* arousal, int B, int T, void* stream);

/* -------------------------------------------------------------------------------------
 * Video motion forensics: OpticalFlow3DCNN.extract (src/core_blocks/visual_blocks.py:129-258) and ChronosGuard
 * (src/models/chronos_guard.py), batched, on the branches the reference takes without OpenCV (csrc/motion.hip).  A clip is T uint8 RGB
 * frames of H x W; every frame becomes a 256 x 256 uint8 luma plane (nearest neighbour: source pixel ((y H) >> 8, (x W) >> 8); luma
 * (0.2989 r + 0.587 g + 0.114 b) in double, operation by operation, truncated).  Pair t is frames (t, t + 1); d = g[t+1] - g[t].
 * `lengths` (B int32, NULL: T; clamped to [0, T]): clip b uses frames 0 .. lengths[b] - 1 and its results are the bits of that clip alone.
 * Nothing allocates or synchronises; no global atomics, fixed reduction orders; every entry can be captured into a hipGraph.
 *
 *   ufnd_motion_workspace_bytes   bytes of the workspace all four stages share for (B, T) (0 for a refused shape).  It starts with the
 *                         gray planes, (B, T, 256, 256) uint8; the rest is per-slab histogram counts and per-tile partials.
 *                         Alignment: 256 bytes.
 *   ufnd_motion_gray      frames: device pointer to uint8; element (b, t, c, y, x) lies at frames + b stride_b + t stride_t +
 *                         c stride_c + y stride_h + x stride_w (64-bit offsets: any layout, no copy; 3 channels).  Writes the gray
 *                         planes and each frame's 32-bin counts (value v in bin min(31, 32 v / 255): np.histogram(bins=32, range=(0,
 *                         255))).  Only the sampled source pixels are read; frames past a clip's length are not touched.
 *   ufnd_motion_pairs     over the gray planes: pair_sums != 0 -> per pair the integer sum of |d| over the plane (ChronosGuard's flow
 *                         magnitude); levels == 3 -> per pixel and chunk of the 1-2-4 temporal pyramid (chunk p of a level with
 *                         `parts` parts is pairs [p seg, (p + 1) seg), seg = max(1, pairs / parts), the last one runs to the end)
 *                         m = fl32(sum |d| / n) and a = fl32(0.25 (2n + sum sign d) / n), correctly rounded, and per chunk the sum and
 *                         centred second moment of m in double, max m and the counts of a in 8 bins (min(7, floor(8 a))).  levels 0:
 *                         no pyramid.
 *   ufnd_motion_chronos_finish   cut_scores, flow_mags (B, T - 1) fp32 (entries past a clip's last pair: 0; T == 1: may be NULL):
 *                         cut = sum_k |c0_k / w / N - c1_k / w / N| in double over the 32 bins (w = 7.96875, N = 65536), flow = sum |d|
 *                         / 65536 (exact); stats (B, 7) = mean, std, max of the cut scores, of the flow magnitudes, and their
 *                         correlation (0 up to 3 pairs; NaN when a series has no variance), evaluated in double; features (B,
 *                         feat_dim) = the seven tiled to feat_dim and divided by (norm + 1e-9); tamper_score (B) = clip(0.6
 *                         norm01(mean cut, 0.05, 0.5) + 0.4 norm01(|std flow - mean flow|, 0, 0.5), 0, 1).  Fewer than 2 frames:
 *                         zeros.  Needs ufnd_motion_gray and ufnd_motion_pairs (pair_sums) before it.
 *   ufnd_motion_flow_finish   pooled (B, 77, optional) = per chunk [mean m, std m, max m, 8 counts], in double from the partials;
 *                         features (B, dim) = pooled tiled (or cut) to dim and divided by (norm + 1e-9).  Fewer than 2 frames: zeros;
 *                         2 to 4 frames: a pyramid chunk is empty, its mean, std and max are NaN and so is every feature, as in the
 *                         reference.  levels must be 3.  Needs ufnd_motion_gray and ufnd_motion_pairs (levels 3) before it.
 * B >= 1, T >= 1, B T <= 2^24, 1 <= H, W <= 2^20. */
size_t ufnd_motion_workspace_bytes(int B, int T);
int ufnd_motion_gray(const void* frames, long long stride_b, long long stride_t, long long stride_c, long long stride_h, long long stride_w,
                     const int32_t* lengths, void* workspace, int B, int T, int H, int W, void* stream);
int ufnd_motion_pairs(const int32_t* lengths, void* workspace, int B, int T, int pair_sums, int levels, void* stream);
int ufnd_motion_chronos_finish(const int32_t* lengths, const void* workspace, float* cut_scores, float* flow_mags, float* stats, float* features,
                               float* tamper_score, int B, int T, int feat_dim, void* stream);
int ufnd_motion_flow_finish(const int32_t* lengths, const void* workspace, float* pooled, float* features, int B, int T, int dim, int levels,
                            void* stream);

/* -------------------------------------------------------------------------------------
 * STFT audio forensics: the branches of src/core_blocks/audio_blocks.py that the reference takes without librosa and without a
 * wav2vec2 checkpoint (csrc/spectral.hip): SpectralForensics._torch_stft_fallback, MelSpectrogramGenerator.generate's torch branch,
 * VoiceCloneDetector.score's energy proxy.  Geometry: torch.stft(n_fft=400, hop_length=160, window=None, center=True,
 * pad_mode="reflect"), one-sided: 201 bins.  waves (B, n_max) fp32; lengths (B int32 on the device, NULL: n_max; clamped to
 * [0, n_max]).  Clip b of len_b samples has T_b = 1 + len_b / 160 frames, frame t being samples 160 t .. 160 t + 399 of the clip
 * reflect-padded by 200 on both sides (x_pad[i] = x[200 - i], ..., x[2 (len_b - 1) - (i - 200)]); the padding is index arithmetic,
 * nothing at or past waves[b][len_b] is read.  A clip of fewer than 201 samples (torch.stft refuses it) has T_b = 0: all its outputs
 * are zeros.  T_max = 1 + n_max / 160.  Nothing allocates or synchronises; no atomics, fixed reduction orders; a clip's outputs are
 * the same bits alone, in any batch and with any set of outputs; every entry can be captured into a hipGraph.
 *
 *   ufnd_spectral_workspace_bytes   bytes of the per-tile statistics partials for (B, n_max) (0 for a refused shape): 32 per tile of
 *                         UFND_STFT_FRAME_TILE frames.  Alignment: 8 bytes.
 *   ufnd_stft_forensics   basis: (402, 400) fp32, row k < 201 = cos(2 pi k n / 400), row 201 + k = -sin(2 pi k n / 400), each the
 *                         float64 value rounded once; 16-B aligned.  re and im of a (frame, bin) are each one chain of 400 fmaf from
 *                         zero on the exact-fp32 MFMA, taps in the order 8u + e, 8u + 4 + e (u = 0 .. 49, e = 0 .. 3);
 *                         |S| = sqrtf(fmaf(re, re, im im)).  Outputs, each optional (NULL), at least one:
 *                           magnitude (B, 201, T_max)  |S|, zeros from frame T_b on
 *                           mel_like  (B, 64, T_max)   ((|S|[3m] + |S|[3m+1]) + |S|[3m+2]) / 3 in fp32 (bins 192 .. 200 dropped), zeros
 *                                                      from frame T_b on
 *                           stats     (B, 4)           mean, population std, max, min of the clip's 201 T_b magnitudes: sum and centred
 *                                                      second moment in double (per tile, then the tiles in order by Chan's update),
 *                                                      rounded to fp32 once
 *                           features  (B, dim)         stats tiled to dim, divided by (norm + 1e-9) in fp32 (the norm in double,
 *                                                      rounded once); an all-zero clip gives exactly 0
 *                         stats or features need the workspace; neither writes the spectrogram anywhere.
 *   ufnd_wave_energy      energy (B, optional) = e = mean(x^2) over the clip's len_b samples in fp32 (thread t of 256 chains samples
 *                         t, t + 256, ... by fmaf, then a fixed tree; len_b = 0 gives 0); score (B, optional) = clip(e / (e + 1), 0, 1)
 *                         divided in double and rounded once.  Any len_b >= 0.
 * 1 <= B <= 65535, 1 <= n_max <= 2^30; offsets are 64-bit. */
#define UFND_STFT_FRAME_TILE 64         /* frames of a workgroup's tile, counted from the clip's first frame */
#define UFND_STFT_MIN_SAMPLES 201       /* shorter clips have no frames */
size_t ufnd_spectral_workspace_bytes(int B, int n_max);
int ufnd_stft_forensics(const float* waves, const int32_t* lengths, const float* basis, void* workspace, float* magnitude, float* mel_like,
                        float* stats, float* features, int B, int n_max, int dim, void* stream);
int ufnd_wave_energy(const float* waves, const int32_t* lengths, float* energy, float* score, int B, int n_max, void* stream);

/* -------------------------------------------------------------------------------------
 * The librosa branches of src/core_blocks/audio_blocks.py (csrc/spectral_desc.hip): SpectralForensics._librosa_spectral (:141-176)
 * and VoiceCloneDetector.score's descriptor mix (:244-254), batched over 16 kHz clips.  The arithmetic below is RESTATED from
 * librosa's documented algorithms (0.10 defaults) and is not verified against librosa itself.  waves, lengths as for
 * ufnd_stft_forensics.  A clip of len_b >= 1 samples has T_A = 1 + len_b / 160 and T_B = 1 + len_b / 512 frames; len_b = 0 has none
 * and all its outputs are zeros.  TA_max = 1 + n_max / 160, TB_max = 1 + n_max / 512.
 *
 *   STFT A   n_fft 400, hop 160, periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / 400), center=True with ZERO padding of 200
 *            (pad_mode="constant", librosa >= 0.10; "reflect" is not built), 201 bins 40 Hz apart, S = |.|.
 *            basis_a (402, 400) fp32: row k < 201 = w[n] cos(2 pi k n / 400), row 201 + k = -w[n] sin(2 pi k n / 400), each the
 *            float64 product rounded once.  re, im: one chain of 400 fmaf each, in the tap order of ufnd_stft_forensics.
 *   stats    mean, population std, max, min of the clip's 201 T_A magnitudes (double per tile, tiles in order by Chan's update).
 *   contrast (7, T_A): spectral_contrast(S, sr=16000), n_bands 6, fmin 200, quantile 0.02.  Band k uses the bin rows
 *            0..4, 4..9, 9..19, 19..39, 39..79, 79..159, 159..200; valley = the smallest row value of the frame, peak = the
 *            largest (band 5: the mean of the two smallest / two largest, (a + b) 0.5 in fp32).  dB(v) = 10 log10(max(1e-10, v)) in
 *            double; each of the two (7, T_A) dB arrays is clipped from below at its own maximum - 80; contrast = dB(peak) -
 *            dB(valley).  Descriptors: its mean and population std (double, two passes).
 *   flatness (T_A): P = max(1e-10, S^2); exp(mean_bins log P) / mean_bins P over the 201 bins in ascending order, in double.
 *            Descriptors: its mean and population std.
 *   STFT B   n_fft 2048, hop 512, the same window rule, ZERO padding of 1024, 1025 bins 7.8125 Hz apart.  basis_b (2050, 2048) as
 *            basis_a.  re, im: one chain of 2048 fmaf each, taps 8u + e, 8u + 4 + e (u = 0 .. 255, e = 0 .. 3).
 *   centroid   (T_B): 7.8125 sum_k k S_k / sum_k S_k, 0 where sum S < FLT_MIN.  rolloff (T_B): 7.8125 times the first bin whose
 *            running sum of S over ascending bins is >= 0.85 sum S (bin 0 for a silent frame).  flatness_y (T_B): as flatness, over
 *            the 1025 bins.  All in double: a lane of the frame's wave owns 17 consecutive bins in ascending order and the 64 lane
 *            sums are added in lane order; the running sum of a lane starts from the sum of the lanes below it.
 *   zcr      (T_B): frame t = samples 512 t - 1024 .. 512 t + 1023 of the clip EDGE-padded; a sample with |x| <= 1e-10f counts as
 *            +0; crossings = number of i in 1 .. 2047 whose sign bit differs from sample i - 1's; value = crossings / 2048 (exact).
 *   descriptors (B, 11) = stats (4), contrast mean, std, flatness mean, std, mean centroid, mean rolloff, mean zcr, each a double
 *            rounded to fp32 once.  features (B, dim) = descriptors tiled to dim, divided by (norm + 1e-9) in fp32 (the norm in
 *            double, rounded once).  clone_score (B) = clip(0.4 mean(flatness_y) + 0.3 mean(zcr) + 0.3 tanh(mean(centroid) / 3000),
 *            0, 1) from the fp32 means, in double, rounded once.
 *
 *   ufnd_spectral_desc_workspace_bytes   bytes of the workspace for (B, n_max) (0 for a refused shape): the per-frame values above
 *            and the frame-major magnitudes of STFT B, 4224 bytes per frame of 32-frame tiles.  Alignment: 16 bytes.
 *   ufnd_spectral_descriptors   every member of `out` is optional (NULL), at least one is needed; only what the asked outputs need
 *            is launched, and an output's bits do not depend on which others are asked for.  Per-frame outputs hold zeros from the
 *            clip's own frame count on: contrast (B, 7, TA_max), flatness (B, TA_max), magnitude (B, 201, TA_max), centroid /
 *            rolloff / flatness_y / zcr (B, TB_max), magnitude_y (B, 1025, TB_max).
 * Nothing allocates or synchronises; no atomics, no scratch, fixed reduction orders: a clip's outputs are the same bits alone, in
 * any batch and from run to run; hipGraph-capturable.  1 <= B <= 65535, 1 <= n_max <= 2^30; offsets are 64-bit.
 * Not built: pyin, pad_mode="reflect", an FFT form of STFT B, other n_fft / hop, the HTK mel scale, the str hash proxies. */
#define UFND_DESC_FRAME_TILE_A 64       /* frames of a workgroup's tile in STFT A */
#define UFND_DESC_FRAME_TILE_B 32       /* ... in STFT B */
typedef struct ufnd_spectral_desc_out {
  float *features, *descriptors, *contrast, *flatness, *centroid, *rolloff, *flatness_y, *zcr, *clone_score, *magnitude, *magnitude_y;
} ufnd_spectral_desc_out;
size_t ufnd_spectral_desc_workspace_bytes(int B, int n_max);
int ufnd_spectral_descriptors(const float* waves, const int32_t* lengths, const float* basis_a, const float* basis_b, void* workspace,
                              const ufnd_spectral_desc_out* out, int B, int n_max, int dim, void* stream);

/* -------------------------------------------------------------------------------------
 * The mel spectrogram in dB of the librosa branch (csrc/mel_db.hip): MelSpectrogramGenerator.generate of
 * src/core_blocks/audio_blocks.py (:71-78) on a host with librosa,
 *     S_db = power_to_db(melspectrogram(y, sr=16000, n_fft=400, hop_length=160, n_mels=64, power=2.0), ref=np.max)
 * batched over 16 kHz clips.  Like the descriptors above, the arithmetic is RESTATED from librosa's documented algorithms (0.10
 * defaults) and is not verified against librosa itself; the filterbank alone has an independent check (tests/test_mel_ref.py:
 * transformers.audio_utils.mel_filter_bank).  Fixed geometry: sr 16000, n_fft 400, hop 160, 64 mels, fmin 0, fmax 8000, the Slaney
 * scale (htk=False), norm="slaney".  waves, lengths as for ufnd_stft_forensics.
 *
 *   frames     T = 1 + len_b / 160 for len_b >= 1, none for len_b = 0; center=True with ZERO padding of 200 (pad_mode="constant");
 *              T_max = 1 + n_max / 160.  basis_a: the (402, 400) window-folded basis of STFT A above.
 *   magnitude  S[k, t]: STFT A, the same bits as ufnd_spectral_descriptors' `magnitude` (one value, one arithmetic: the tap order
 *              8u + e, 8u + 4 + e and sqrtf(fmaf(re, re, im im))).
 *   power      P = S S, one fp32 multiply (librosa's np.abs(D) ** 2).
 *   filterbank W (64, 201), evaluated in float64 on the host and rounded to fp32 once: mel(f) = 3 f / 200 below 1000 Hz and
 *              15 + 27 ln(f / 1000) / ln 6.4 from 1000 Hz on; 66 points equally spaced in mel over [mel(0), mel(8000)], mapped back
 *              to Hz as m[0 .. 65] (m[1] = 46.4057851 Hz; m[22] is the first at or above 1000 Hz); bin k is at 40 k Hz;
 *              W[i, k] = max(0, min((40 k - m[i]) / (m[i+1] - m[i]), (m[i+2] - 40 k) / (m[i+2] - m[i+1]))) 2 / (m[i+2] - m[i]).
 *              Every row's support is contiguous: 2 to 18 bins, 388 nonzeros in all; bins 0 and 200 carry no weight; row 0 covers
 *              bins 1..2, row 63 bins 182..199.  The device gets fb_weights (388: the nonzeros, row after row), fb_first (64) and
 *              fb_count (64); whatever those arrays hold, a support is clamped to the 201 bins and to the 388 weights.
 *   mel power  M[i, t] = one chain from zero over the row's support in ascending bins, M = fmaf(W[i, k], P[k, t], M).  Nothing
 *              outside the support is touched (an exact zero weight times a stray Inf would be NaN).
 *   dB         power_to_db(M, ref=np.max) is  L = 10 log10(max(1e-10, M)) - 10 log10(max(1e-10, Mmax)),  Mmax the maximum of the
 *              clip's own 64 T values, then  max(L, max(L) - top_db)  with top_db = 80.  log10 and max are monotone, so the largest
 *              L belongs to the entry that IS Mmax and is exactly 0: the floor is the constant -80,  D = max(L, -80).  Evaluated in
 *              double and rounded to fp32 once (as the contrast dB above).  An all-zero clip has D = 0 on all its frames.
 *
 *   mel_db (B, 64, T_max), mel_power (B, 64, T_max), mel_max (B): each optional (NULL), at least one is needed; which of them are
 *              asked for changes no bit of any.  Per-frame outputs hold zeros from the clip's own T on -- 0 is ALSO a legitimate dB
 *              value (the clip's loudest entry), so read a clip's frames by its own T.  A clip of length 0 gives zeros everywhere.
 *   ufnd_mel_workspace_bytes   bytes of the workspace for (B, n_max), 0 for a refused shape: the mel powers (B 64 T_max floats) and
 *              one maximum per 64-frame tile, each rounded up to 16 bytes.  Alignment: 16 bytes.
 * Two launches (tile kernel: STFT tile + filterbank + tile maximum; dB kernel: every workgroup folds its clip's tile maxima, then
 * converts its own tile).  Nothing allocates or synchronises; no atomics, no scratch: a clip's outputs are the same bits alone, in
 * any batch and from run to run; hipGraph-capturable.  1 <= B <= 65535, 1 <= n_max <= 2^30; offsets are 64-bit.
 * Not built: pad_mode="reflect", other geometries (sr, n_fft, hop, n_mels, fmin, fmax), the HTK scale, norm other than "slaney". */
#define UFND_MEL_FRAME_TILE 64          /* frames of a workgroup's tile */
#define UFND_MEL_FILTERS 64             /* mel filters */
#define UFND_MEL_NNZ 388                /* nonzero weights of the (64, 201) filterbank */
size_t ufnd_mel_workspace_bytes(int B, int n_max);
int ufnd_mel_spectrogram(const float* waves, const int32_t* lengths, const float* basis_a, const float* fb_weights, const int32_t* fb_first,
                         const int32_t* fb_count, void* workspace, float* mel_db, float* mel_power, float* mel_max, int B, int n_max,
                         void* stream);

/* -------------------------------------------------------------------------------------
 * Sample-rate conversion (csrc/resample.hip): the device form of the reference's _ensure_mono_16k
 * (src/core_blocks/audio_blocks.py:34-45: channel mean, then librosa.resample, one clip at a time on the host).  Band-limited
 * windowed-sinc interpolation in polyphase form.  With g = gcd(orig_sr, new_sr), o = orig_sr / g, n = new_sr / g and a quality
 * (lpw, rolloff, window):  base = min(o, n) rolloff,  width = ceil(lpw o / base),  K = 2 width + o,  and for phase p < n, tap k < K
 *     t = ((k - width) n - p o) / (o n) base;   h[p][k] = (base / o) sinc(pi t) w(t) for |t| < lpw, else 0
 * (hann: w = cos^2(pi t / (2 lpw)); kaiser: w = I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)), evaluated in float64 on the host and
 * rounded once.  Output:  y[q n + p] = sum_k h[p][k] xz[q o + k - width],  xz the clip, zero outside [0, len_b);  clip b has
 * m_b = ceil(n len_b / o) outputs (64-bit arithmetic), m_max = ceil(n n_max / o).  o = n = 1 with the table h = [[1]] (width 0) copies.
 *
 *   waves     element (b, c, s) at waves + b stride_b + c stride_c + s stride_s ELEMENTS (64-bit offsets: channel-first, channel-last
 *             or mono, no copy); dtype UFND_RESAMPLE_F32 or UFND_RESAMPLE_I16.  The mix happens while staging: float(v) per channel,
 *             summed in channel order in fp32, divided once by C, multiplied once by `scale` (NumPy's
 *             astype(float32).mean(axis=0) bit for bit; 1 / 32768 for PCM).  lengths: (B) int32 on the device, NULL: n_max; clamped
 *             to [0, n_max].  Nothing at or past sample len_b of a clip is read.
 *   the table is built by the host for a super-stride of G strides (o' = G o, n' = G n; phase g n + p of the super-stride is phase
 *             p with its taps shifted by g o), in GROUPS of 4 neighbouring phases:
 *               groups (ngroups, 3) int32 = first tap, tap count, row offset into `taps`; ngroups = ceil(n' / 4); first and count
 *                      are multiples of 8 and cover the bands of the group's phases
 *               taps   (tap_rows, 4) fp32, 16-B aligned: row (offset + k - first) = the taps k of phases 4 g .. 4 g + 3, zero where a
 *                      phase has none (and for the phases past n')
 *             A group whose entry is inconsistent (negative, not a multiple of 8, past tap_rows) computes zeros; the device never
 *             reads outside the two tables.
 *   a workgroup owns qt (<= UFND_RESAMPLE_OUT_TILE) super-strides of one clip, that is qt G n consecutive outputs counted from the
 *             clip's first, and walks the filter in nchunks chunks of kc taps (kc a multiple of 8, nchunks kc >= the largest
 *             first + count, (qt - 1) G o + kc <= UFND_RESAMPLE_LDS_FLOATS; a filter that fits has nchunks = 1).
 *   out (B, m_max) fp32, zeros from m_b on;  out_lengths (B) int32 = m_b, written on the device.
 * One value, one arithmetic: output (q, p) is ONE chain acc = fmaf(h[p][k], xz[q o + k - width], acc) from +0 over the stored band
 * of phase p in ASCENDING k, whatever G, the group, the tile, the chunking, the batch and the row; the zero taps the group table
 * adds leave it unchanged for finite samples (a non-finite sample inside a clip also poisons the outputs whose group band covers it,
 * a few taps beyond its true support).  Nothing allocates or synchronises; no atomics, no scratch; hipGraph-capturable.
 * 1 <= B <= 65535, 1 <= C <= 64, 1 <= n_max <= 2^30, 1 <= o, n <= UFND_RESAMPLE_MAX_RATIO_TERM, m_max <= 2^31 - 1. */
#define UFND_RESAMPLE_OUT_TILE 64          /* super-strides (rows of G n outputs) of a workgroup's tile: one per lane */
#define UFND_RESAMPLE_LDS_FLOATS 40000     /* staged samples of a workgroup */
#define UFND_RESAMPLE_MAX_RATIO_TERM 1024  /* the reduced o and n */
#define UFND_RESAMPLE_F32 0
#define UFND_RESAMPLE_I16 1
int ufnd_resample(const void* waves, int dtype, long long stride_b, long long stride_c, long long stride_s, const int32_t* lengths,
                  const float* taps, const int32_t* groups, float* out, int32_t* out_lengths, int B, int C, int n_max, int o, int n, int G,
                  int width, int ngroups, int tap_rows, int qt, int kc, int nchunks, float scale, void* stream);

/* -------------------------------------------------------------------------------------
 * Image-forgery evidence: DeepForgeryDetector.ela_lbp and FaceWarpAnalyzer.score (src/core_blocks/visual_blocks.py:265-406), batched
 * (csrc/forgery.hip).  Frames as for ufnd_motion_gray: uint8, (b, t, c, y, x) at frames + b stride_b + t stride_t + c stride_c +
 * y stride_h + x stride_w, 3 channels; a batch of single images is T = 1.  `lengths` (B int32 on the device, NULL: T; clamped to
 * [0, T]).  Clip b contributes ONE frame, index len_b / 2 (the reference's frames[len(frames) // 2]), resized to 256 x 256 by the
 * nearest-neighbour rule (source pixel ((y H) >> 8, (x W) >> 8)).  A clip of length 0 has no frame: nothing of it is read, its stats,
 * histogram, vector and gradient are zeros and its score is 0.0 (the reference's `img is None` result); its planes and maps are not
 * written.  The error level (ELA) map is |rgb - rec| with rec the image after a JPEG round trip, which is integer arithmetic from end to
 * end (baseline libjpeg, 4:2:0, the "islow" DCTs, fancy upsampling; entropy coding is lossless and left out): rec equals what
 * libjpeg decodes in every byte.  Nothing allocates or synchronises; no global atomics, fixed reduction orders: a clip's results are the
 * same bits alone, in any batch and from run to run; every entry can be captured into a hipGraph.
 *
 *   ufnd_forgery_workspace_bytes   bytes of the workspace all stages share for B clips (0 for a refused B).  It starts with rgb
 *                         (B, 256, 256, 3) uint8, then rec slot 0 and rec slot 1 of the same shape; the rest is the decoded Y / Cb /
 *                         Cr planes and per-slab partials.  Alignment: 256 bytes.
 *   ufnd_forgery_resize   writes rgb.  Only the sampled pixels of the one frame per clip are read.
 *   ufnd_forgery_roundtrip   rgb -> rec[slot].  jpeg_mode 1: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G +
 *                         32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16; chroma
 *                         2 x 2 downsampled, (sum + bias) >> 2 with bias 1 on even and 2 on odd output columns; per 8 x 8 block of
 *                         sample - 128 jfdctint (rows, then columns; the result is scaled by 8), |c| -> (|c| + (8 q >> 1)) / (8 q) with
 *                         the sign restored, times q, jidctint (columns DESCALE 11, rows DESCALE 18), + 128, clamped; fancy h2v2
 *                         upsampling (3/4 nearer + 1/4 farther row, then column, edges replicated, rounding 8 / 7 on even / odd
 *                         columns); R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16), G = Y + ((-22554 Cb' +
 *                         32768 - 46802 Cr') >> 16) with C' = C - 128, clamped.  qtables: HOST pointer to 128 quantisers (1 .. 255),
 *                         luma then chroma, natural order; they travel as kernel arguments.  jpeg_mode 0: rec[slot] = rgb, the
 *                         reference's branch on a host without OpenCV (qtables may be NULL).  Needs ufnd_forgery_resize before it.
 *   ufnd_forgery_maps     over rgb and rec[slot]: ela = uint8(trunc(clip(fl32(|rgb - rec|) ela_scale, 0, 255))), the product in fp32;
 *                         per 16-row slab the integer sum, sum of squares, max and min over the three channels.  want_lbp: the luma of
 *                         the ELA map (the float64 luma of ufnd_motion_gray) and, for the centres (y, x), y and x in 1, 3, ..., 253,
 *                         the number of the 8 neighbours strictly greater than the centre: counts per code 0 .. 8.  want_grad: of the
 *                         luma g of rgb (not of the map) gx = g(y, x) - g(y, x - 1), gy = g(y, x) - g(y - 1, x), zero in column 0 /
 *                         row 0; the sum of sqrt(gx^2 + gy^2) in double and of gx^2 + gy^2 as an integer (slot 0 only: the gradient does
 *                         not depend on rec).  ela_map (B, 256, 256, 3) and ela_gray (B, 256, 256) uint8, each optional (NULL), 4-B aligned.
 *   ufnd_forgery_finish   every output optional (NULL), at least one.  From slot 0's partials: stats (B, 4) = mean (the exact integer
 *                         sum divided once in double), population std (sqrt((N Q - S^2) / N^2) from the exact integer numerator),
 *                         max, min over the N = 196608 values; lbp (B, 10) = count / 1.0 / 16129 in double, as np.histogram(bins=10,
 *                         range=(0, 10), density=True): code k in bin k, the tenth bin is always 0; features (B, dim) = the 14 values
 *                         tiled (or cut) to dim and divided by (norm + 1e-9), the finish of ufnd_motion_flow_finish.  Needs maps on
 *                         slot 0 with want_lbp.  grad (B, 2) = mean and population std of sqrt(gx^2 + gy^2) over the 65536 pixels in
 *                         double; score (B) = clip(0.5 tanh(g_std / (g_mean + 1e-6)) + 0.5 mean_ela / 255, 0, 1) in double, rounded
 *                         once, mean_ela being the map mean of rec[score_slot] (the reference scores with a quality-85, scale-1
 *                         map whatever the detector's own settings are: callers put that map in a slot).  Needs maps on slot 0 with
 *                         want_grad, and maps on score_slot.
 * 1 <= B <= 65536, T >= 1, 1 <= H, W <= 2^20. */
size_t ufnd_forgery_workspace_bytes(int B);
int ufnd_forgery_resize(const void* frames, long long stride_b, long long stride_t, long long stride_c, long long stride_h, long long stride_w,
                        const int32_t* lengths, void* workspace, int B, int T, int H, int W, void* stream);
int ufnd_forgery_roundtrip(const int32_t* lengths, void* workspace, const unsigned char* qtables, int B, int T, int jpeg_mode, int slot, void* stream);
int ufnd_forgery_maps(const int32_t* lengths, void* workspace, float ela_scale, void* ela_map, void* ela_gray, int B, int T, int slot, int want_lbp,
                      int want_grad, void* stream);
int ufnd_forgery_finish(const int32_t* lengths, const void* workspace, float* stats, float* lbp, float* features, float* grad, float* score, int B, int T,
                        int dim, int score_slot, void* stream);

/* -------------------------------------------------------------------------------------
 * A/V lag estimation (csrc/av_lag.hip): the reference's estimate_av_lag (TemporalSyncNet, src/core_blocks/temporal_blocks.py:176-223,
 * and ChronosGuard, src/models/chronos_guard.py:175-196), batched on the device as a DIRECT windowed cross-correlation (the
 * reference reads the same window out of three zero-padded FFTs).  Pair b is a = a[b, :len_a[b]] and m = m[b, :len_m[b]]:
 *
 *   n          min(len_a, len_m) (each clamped to [0, row width] on the device; NULL: the row width).  n < 4: lag 0, peak 0, the
 *              xcorr row -inf, the a_std / m_std rows zero (the reference returns 0.0 before it standardises).
 *   statistics sum of x and, with the mean in double, sum of (x - mean)^2, both in double: thread t of 1024 adds x[t], x[t + 1024],
 *              ... in ascending order, the 1024 partials fold by halves (red[t] += red[t + o], o = 512 .. 1); mean = sum / n and
 *              std = sqrt(sumsq / n) (population, ddof 0) in double, each rounded to fp32 once.
 *   xhat       (x - mean) / (std + 1e-9f), three fp32 operations (the reference's float32 NumPy expression; its mean and std are
 *              NumPy's pairwise fp32 sums, so the two differ within rounding).  A constant row whose mean is exact gives zeros.
 *   window     K = max_lag (the host's int(max_lag_s * sr)), Kc = min(K, n - 1):  c[k] = sum_i ahat[i + k] mhat[i] over the i with
 *              0 <= i < n and 0 <= i + k < n, k = -Kc .. Kc; a[i + s] = m[i] gives lag +s.  (The reference's lo / hi / center
 *              arithmetic on its 2 n - 1 lags is this window, for K < n - 1 and for K >= n - 1.)
 *   c[k]       segments of UFND_AVLAG_SEGMENT = 2048 samples i: P[s][k] = ONE chain acc = fmaf(ahat[i + k], mhat[i], acc) from +0
 *              over the i of segment s in ASCENDING i (terms with i + k outside the pair multiply a zero: the value is that of the
 *              chain over the valid i);  c[k] = ((P[0][k] + P[1][k]) + ...) + P[S - 1][k] + 0.0f, S = ceil(n / 2048), fp32 additions
 *              in ascending s; the closing + 0.0f makes every zero +0.  The order depends on (n, k) alone.
 *   lag        argmax_k c[k], ties to the LOWEST k (np.argmax's first index): an all-zero a gives -Kc, as in the reference.
 *              lag_seconds = lag_samples / sr is left to the caller (an IEEE double division equals the reference's float).
 *
 *   a, m       fp32, row b at a + b a_row_stride, m + b m_row_stride ELEMENTS (64-bit, >= 0), unit inner stride, na_max / nm_max wide.
 *   lag_samples (B) int32;  peak_corr (B) fp32 = c[lag] / n, one fp32 division (an addition to the reference: a correlation
 *              coefficient);  xcorr (B, 2 K + 1) fp32, column j is lag j - K, -inf outside the pair's window;  a_std, m_std
 *              (B, min(na_max, nm_max)) fp32, zero from n on.  Each optional (NULL), at least one; what is asked for changes no bit.
 *   ufnd_av_lag_workspace_bytes(B, n_max, max_lag)   n_max = min(na_max, nm_max).  The two standardised rows (each B rows of n_max
 *              rounded up to 8 floats) and the partials (B ceil(n_max / 2048) (2 max_lag + 1) floats), each rounded up to 16 bytes.
 *              0 for a refused shape: B outside 1 .. UFND_AVLAG_MAX_B, n_max outside 1 .. UFND_AVLAG_MAX_N, max_lag < 0 or above
 *              UFND_AVLAG_MAX_LAG, or more partials than UFND_AVLAG_MAX_PARTIAL_FLOATS.  Alignment: 16 bytes.
 * Three launches (standardise; correlate: a workgroup per (UFND_AVLAG_LAG_BLOCK lags, segment, pair), a lane per 8 consecutive lags
 * sliding a register window over LDS; finish).  Nothing allocates or synchronises; no atomics, no scratch; lengths are never read on
 * the host; nothing at or past a row's length is read; a pair's outputs are the same bits alone, in any batch and from run to run;
 * hipGraph-capturable.  Not built: an FFT form, producers of the two envelopes, non-finite samples (outside the contract). */
#define UFND_AVLAG_SEGMENT 2048                        /* samples of one partial chain */
#define UFND_AVLAG_LAG_BLOCK 1024                      /* lags of a workgroup */
#define UFND_AVLAG_MAX_B 65535
#define UFND_AVLAG_MAX_N (1 << 26)
#define UFND_AVLAG_MAX_LAG (1 << 26)
#define UFND_AVLAG_MAX_PARTIAL_FLOATS 2147483648LL     /* 8 GiB of partials */
size_t ufnd_av_lag_workspace_bytes(int B, int n_max, int max_lag);
int ufnd_av_lag(const float* a, int64_t a_row_stride, const float* m, int64_t m_row_stride, const int32_t* len_a, const int32_t* len_m,
                void* workspace, int32_t* lag_samples, float* peak_corr, float* xcorr, float* a_std, float* m_std, int B, int na_max, int nm_max,
                int max_lag, void* stream);

/* -------------------------------------------------------------------------------------
 * CLIP image preprocessing (csrc/clip_preprocess.hip): what the checkpoint's CLIPImageProcessor does on its Pillow backend (the one
 * the reference instantiates, src/models/semantic_forgery.py:54-61) -- shortest-edge bicubic resize, centre crop, rescale,
 * normalise -- on decoded uint8 frames, batched and ragged on the device, equal to Pillow and the processor in every byte and bit.
 * Frames as for ufnd_motion_gray: uint8, (b, t, c, y, x) at frames + b stride_b + t stride_t + c stride_c + y stride_h + x stride_w
 * (elements, 64-bit, >= 0), 3 channels; a batch of single images is T = 1.  `lengths` (B int32 on the device, NULL: T; clamped to
 * [0, T]).  With S the output edge (the encoder's `image`):
 *
 *   size       short, long = the source's shorter and longer edge; the resized image has short edge S and long edge
 *              int(S * long / short) (truncated); W <= H makes the width the short edge.
 *   one pass   in -> out samples along an axis: scale = in / out, fs = max(scale, 1), support = 2 fs.  Output xx: c = (xx + 0.5) scale,
 *              xmin = max(int(c - support + 0.5), 0), xmax = min(int(c + support + 0.5), in), n = xmax - xmin taps
 *              w[x] = bicubic((x + xmin - c + 0.5) (1 / fs)), a = -0.5: ((a + 2)|t| - (a + 3)) t^2 + 1 for |t| < 1,
 *              (((|t| - 5)|t| + 8)|t| - 4) a for |t| < 2, else 0; summed in index order in double, each divided by a non-zero sum;
 *              k = (int)(w 2^22 + 0.5) for w >= 0, (int)(w 2^22 - 0.5) for w < 0 (the cast truncates);
 *              pixel = clip((2^21 + sum_x k[x] p[xmin + x]) >> 22, 0, 255), an arithmetic shift of a signed 32-bit sum.
 *   order      horizontal, then vertical; the image between them is uint8 (rounded and clipped as above).  A pass with in == out is
 *              skipped: its table is the identity, one tap of 2^22.
 *   crop       S x S at top = (h' - S) / 2, left = (w' - S) / 2 (floor) of the resized h' x w' image; only the crop's rows and columns
 *              are computed, and of the source only the rows and columns their taps reach.
 *   value map  channel c, byte v:  r = fl32(double(v) 0.00392156862745098);  (r - fl32(mean[c])) / fl32(std[c]), both in fp32, the
 *              division correctly rounded: 768 values, evaluated on the host and passed as value_map (3, 256) fp32 on the device.
 *
 *   tables     int32 on the device, built on the host in double by the formulas above (video.clip_resize_tables) for the S crop
 *              columns and the S crop rows:  hfirst[S], hcount[S], vfirst[S], vcount[S], hk[S][taps_h], vk[S][taps_v]  in this
 *              order; taps_h / taps_v = the largest count of the pass; |k| < 2^23 (a normalised weight stays below 2: the kernel's
 *              products are 24-bit multiplies).  x_lo, x_span: the source columns the horizontal taps reach,
 *              [x_lo, x_lo + x_span).  tile_rows: output rows of a workgroup; lds_rows: the most intermediate rows one tile's taps
 *              reach.  The kernel clamps every table entry into the source and into its tile, so a wrong table gives wrong pixels,
 *              never an access outside the frames or the tile.
 *   outputs    pixel_values (B, T, 3, S, S) fp32 and rgb (B, T, S, S, 3) uint8 (the cropped resized image), contiguous, each optional
 *              (NULL), at least one.  Frame t >= len_b holds the bits of frame len_b - 1 (the reference's padding,
 *              src/training/run_train_eval.py:329-333); a clip of length 0 holds the image of an all-zero frame (:325).  Source
 *              frames at or past a clip's length are never read.
 * One launch: a workgroup per (frame, tile of tile_rows output rows).  It runs the horizontal pass over the intermediate rows its
 * tile needs, source rows staged through LDS in 16-byte reads when the pixels are dense (stride_c = 1 and stride_w = 3, or
 * stride_w = 1; any other view is gathered byte by byte), keeps the uint8 intermediate in LDS, and runs the vertical pass from
 * there: the intermediate never travels through memory.  Intermediates up to UFND_CLIP_PRE_INTER_BYTES run in a 64 KiB workgroup
 * (two per CU), larger ones up to UFND_CLIP_PRE_INTER_BYTES_LARGE in a 156 KiB one.  Each output depends on its source frame and
 * (H, W, S) alone: the same bits alone, in any batch, for any tile_rows, from run to run.  Nothing allocates or synchronises; no
 * atomics, no scratch, no workspace; hipGraph-capturable.
 * Refused by name: B, T, H, W < 1; H, W > UFND_CLIP_PRE_MAX_EDGE; B T > UFND_CLIP_PRE_MAX_FRAMES or more than 2^31 - 1
 * workgroups; S outside UFND_CLIP_PRE_MIN_SIZE .. UFND_CLIP_PRE_MAX_SIZE; taps_h, taps_v outside 1 .. UFND_CLIP_PRE_MAX_TAPS (41 taps
 * resize 2160 x 3840 to 224); x_span outside 1 .. UFND_CLIP_PRE_MAX_SPAN or a span outside the row; tile_rows outside
 * 1 .. UFND_CLIP_PRE_MAX_TILE_ROWS; lds_rows < 1, > H or more than UFND_CLIP_PRE_INTER_BYTES_LARGE of intermediate (rows of
 * 3 S bytes rounded up to 4). */
#define UFND_CLIP_PRE_MIN_SIZE 16
#define UFND_CLIP_PRE_MAX_SIZE 448
#define UFND_CLIP_PRE_MAX_TAPS 64
#define UFND_CLIP_PRE_MAX_SPAN 7000                  /* source columns a row's horizontal taps reach */
#define UFND_CLIP_PRE_MAX_TILE_ROWS 16
#define UFND_CLIP_PRE_INTER_BYTES 40960              /* the intermediate of a tile in the 64 KiB workgroup */
#define UFND_CLIP_PRE_INTER_BYTES_LARGE 135168       /* ... and in the 156 KiB one */
#define UFND_CLIP_PRE_STAGE_BYTES 21376              /* staged source rows of a workgroup */
#define UFND_CLIP_PRE_MAX_EDGE 65536
#define UFND_CLIP_PRE_MAX_FRAMES (1 << 24)
int ufnd_clip_preprocess(const void* frames, long long stride_b, long long stride_t, long long stride_c, long long stride_h, long long stride_w,
                         const int32_t* lengths, const int32_t* tables, const float* value_map, float* pixel_values, void* rgb, int B, int T, int H,
                         int W, int S, int taps_h, int taps_v, int x_lo, int x_span, int tile_rows, int lds_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRAFND_HIP_H */
