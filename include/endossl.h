/* endossl C-ABI: the MI355X (gfx950) kernels behind the FixMatch / CoMatch SSL training step.
 *
 * libendossl_hip.so exports exactly these functions.  Conventions:
 *  - every pointer is a caller-owned DEVICE pointer; no function allocates or synchronises;
 *  - every call takes the HIP stream it is enqueued on (last argument) and returns an int
 *    status: 0 = OK, -1 = bad shape, -2 = bad argument (null / inconsistent), -3 = HIP error;
 *  - no C++ exception crosses this boundary; functions are stateless and re-entrant;
 *  - bf16 tensors are passed as void* (raw 16-bit bfloat16 storage), fp32 as float*;
 *  - token-major activations are row-major [tokens, features]; buffers read by the GEMMs are
 *    padded to a multiple of 256 rows whose pad rows are zero (DESIGN.md "HBM layout").
 *
 * The reference has no FFI (pure Python / PyTorch); each entry point cites the
 * reference computation it replaces.  The Python host side (endossl/_lib.py) binds them with
 * ctypes exactly as INTEGRATION.md shows.
 */
#ifndef ENDOSSL_H
#define ENDOSSL_H
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- identity ---------------------------------------------------------------------------- */
int es_abi_version(void);

/* ---- GEMMs (code/models/conformer.py:13-23,35-50 nn.Linear; timm PatchEmbed Conv2d) ------- */
/* C[M,N] = A[M,K] . B[N,K]^T with a fused epilogue:
 *   epi 0: C bf16 = acc (+bias)                      (qkv, dgrad to a bf16 operand)
 *   epi 1: C bf16 = acc+bias, C2 bf16 = GELU(acc+bias) (Mlp.fc1 + act, conformer.py:19-20)
 *   epi 2: C f32 = acc (+bias) + aux f32              (Attention.proj / Mlp.fc2 + residual, :70-71)
 *   epi 3: C bf16 = acc * GELU'(aux bf16)             (fc2 dgrad through the activation)
 *   epi 4: C f32 = acc (+bias)                        (dgrad into LayerNorm backward)
 *   epi 5: C f32 at token row img*(np+1)+1+p = acc + bias + aux[1+p]   (patch embed + pos_embed)
 *   epi 6: C bf16 = GELU(acc+bias) only                (fc1 + act in inference forwards)
 *   epi 7: C bf16 = GELU'(acc+bias), C2 bf16 = GELU(acc+bias)   (train fc1: keeps the derivative, not the
 *          pre-activation, so the backward needs no erf; activation bits identical to epi 1)
 *   epi 8: C bf16 = acc * aux bf16                     (fc2 dgrad times the stored GELU')
 * N % 128 == 0, K % 64 == 0; A readable for round_up(M,256) rows.  The epilogue reads aux in 16-byte pieces at
 * (m * ldaux + n): -1 (ES_BAD_SHAPE) unless ldaux >= N and ldaux % 4 == 0 for the fp32 aux of epi 2 and 5,
 * ldaux % 8 == 0 for the bf16 aux of epi 3 and 8 (ldaux is ignored by the other epilogues). */
int es_gemm_nt(int epi, const void* A, int lda, const void* B, int ldb, const float* bias, void* C, int ldc,
               void* C2, const void* aux, int ldaux, int M, int N, int K, int np, hipStream_t stream);
/* x = A B^T + bias + aux, h = LayerNorm(x; gamma, beta, eps) with per-row mean / rstd, in one launch, for
 * N == K == 384 (ViT-S's attention projection followed by norm2): the bits of es_gemm_nt(epi 2) followed by
 * es_layernorm_fwd.  x fp32 [M, ldc], aux fp32 [M, ldaux] (16-B aligned rows), h bf16 [M, ldh]; bias nullable.
 * Replaces code/models/conformer.py:65-66 (x + attn(...), then norm2).  ES_BAD_SHAPE for other N / K;
 * ES_BAD_ARG for a null or misaligned operand (A, B, aux, gamma, beta, bias 16-B; C 8-B; h 4-B). */
int es_gemm_nt_resid_ln(const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc,
                        const float* aux, int ldaux, const float* gamma, const float* beta, void* h, int ldh,
                        float* mean, float* rstd, int M, int N, int K, float eps, hipStream_t stream);
/* The MLP's fc2, its residual add and the next block's LayerNorm 1 in one launch (N = 384, K a multiple of 64):
 * x = A B^T + bias + aux (fp32, into C), h = LayerNorm(x; gamma, beta) (bf16) with the per-row mean / rstd the
 * LayerNorm backward reads -- bit-identical to es_gemm_nt(epi 2) followed by es_layernorm_fwd.  A bf16 [M, lda],
 * B bf16 [384, ldb], x fp32 [M, ldc], aux fp32 [M, ldaux], h bf16 [M, ldh]; bias nullable.  Replaces
 * code/models/conformer.py:70-71 (x + mlp(norm2(x))) and the next block's norm1 (:65).  ES_BAD_SHAPE for other N,
 * K % 64 != 0, M <= 0, a row stride below its width or misaligned (lda, ldb % 8; ldc, ldaux, ldh % 2);
 * ES_BAD_ARG for a null or misaligned operand (A, B, gamma, beta, bias 16-B; C, aux 8-B; h, mean, rstd 4-B). */
int es_gemm_nt_ln(const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc,
                  const float* aux, int ldaux, const float* gamma, const float* beta, void* h, int ldh, float* mean,
                  float* rstd, int M, int N, int K, float eps, hipStream_t stream);
/* tuning knob: NT kernel family (-1 = per-shape default; 0, 1, 2, 5, 6, 10, 11 = fixed tilings, see gemm.hip);
 * returns the old one, or -2 (state unchanged) for a family that does not exist */
int es_set_gemm_variant(int variant);
/* 1 (default): the 64 x 128 NT tile rules (N <= 384 outputs of small token shards, M < 32768, and the residual
 * proj forward); 0: without them.  Returns the old value. */
int es_set_gemm_small_tile(int v);
/* weight gradient: out[N1,N2] (+)= sum_m A1[m,N1]^T A2[m,N2], token axis split `splits` ways into
 * fp32 slabs (workspace = es_gemm_tn_workspace floats) and reduced; bias_out (nullable) (+)=
 * sum_m A1[m,:] computed from the same tiles.  splits <= 0: sized by the library for the kernel it
 * picks (es_gemm_tn_workspace(N1, N2, 0) bounds the workspace).  N1,N2 % 128 == 0, or N1 % 384 == 0
 * and N2 % 192 == 0; rows in [M, round_up(M,64)) of A1 must be zero. */
/* tuning knob for es_gemm_tn: -1 = default (384x192 tile for M >= 65536 where it tiles, else
 * 128x128), 0 = the 128x128 tile (32-token steps, two stages), 7 = the 384x192 tile (64-token steps,
 * two stages); a pin >= 0 also overrides the variant es_gemm_tn_ex callers pass.  Returns the previous
 * value, or -2 (state unchanged) for any other value */
int es_set_tn_variant(int variant);
size_t es_gemm_tn_workspace(int N1, int N2, int splits);
int es_gemm_tn(const void* A1, int ld1, const void* A2, int ld2, int M, int N1, int N2, int splits,
               float* workspace, float* out, int accumulate, float* bias_out, hipStream_t stream);
/* es_gemm_tn with an explicit kernel choice (0 or 7, the es_set_tn_variant numbering; -1 = the
 * library's per-shape choice; anything else -2): the engine passes the 384x192 tile for its
 * CU-share-sized launches this way instead of toggling the global knob around each call */
int es_gemm_tn_ex(const void* A1, int ld1, const void* A2, int ld2, int M, int N1, int N2, int splits,
                  float* workspace, float* out, int accumulate, float* bias_out, int variant, hipStream_t stream);
int es_splitk_reduce(const float* P, float* out, int S, int n, int accumulate, hipStream_t stream);
/* Grouped weight gradients: many independent es_gemm_tn problems in ONE launch, each 128x128 tile
 * over its problem's whole token axis (no split-K slabs, no reduction launches) -- the small-shard
 * backward (strong scaling: M = 12,608 tokens per rank at N = 8), where split-K slabs and per-GEMM
 * reductions cost more than the products.  N1, N2 % 128 == 0; rows [M, round_up(M, 32)) of dy zero;
 * out / bias_out overwritten.  es_gemm_tn_grouped_prepare fills mchunk / tile0 of a HOST table and
 * returns the total tile count; the caller copies the table to the device and launches. */
typedef struct {
  const void* dy;     /* A1 [M, N1] bf16, row stride ld1 */
  const void* x;      /* A2 [M, N2] bf16, row stride ld2 */
  float* out;         /* [N1, N2] fp32 */
  float* bias_out;    /* [N1] fp32 column sums of dy, nullable */
  int M, N1, N2, ld1, ld2;
  int mchunk, tile0, pad;  /* filled by es_gemm_tn_grouped_prepare */
} es_tn_problem;
size_t es_tn_problem_size(void);
int es_gemm_tn_grouped_prepare(void* host_table, int count);
int es_gemm_tn_grouped(const void* device_table, int count, int total_tiles, hipStream_t stream);
/* A Linear layer's weight gradients as ONE split-K launch on the 384x192 tile (the long-token-axis
 * backward: fc1 + fc2 + qkv + proj of a ViT block in one grid), then ONE reduce launch over every
 * problem's fp32 slabs and bias partials.  Input: `count` es_tn_problem entries (dy, x, out, bias_out,
 * M, N1, N2, ld1, ld2; mchunk / tile0 / pad ignored), N1 % 384 == 0, N2 % 192 == 0, rows
 * [M, round_up(M, 64)) of dy zero; out / bias_out overwritten.  Every problem gets
 * max(1, target_wgs / its-and-the-others' 384x192 tiles) splits (at most one per 64 tokens), so the
 * slabs are S x the layer's outputs with S a few, not 16-32 per GEMM (one split: written in place).
 * count <= 8.  _prepare writes the table (es_gemm_tn_big_grouped_table_bytes(count) bytes of HOST memory;
 * es_gemm_tn_big_grouped passes it by value in the kernel arguments) and dims[3] = {workgroups, reduce
 * blocks, reduce entries}; workspace >= es_gemm_tn_big_grouped_workspace floats.  Replaces the per-Linear es_gemm_tn launches of code/models/conformer.py:13-23,35-50's
 * backward (autograd's addmm weight gradients). */
size_t es_gemm_tn_big_grouped_table_bytes(int count);
size_t es_gemm_tn_big_grouped_workspace(const void* problems, int count, int target_wgs);
int es_gemm_tn_big_grouped_prepare(const void* problems, int count, int target_wgs, float* workspace,
                                   size_t workspace_floats, void* table, int* dims);
int es_gemm_tn_big_grouped(const void* table, int count, const int* dims, hipStream_t stream);
/* the same launch with timing: `start` is stamped at the grouped kernel's own start, `stop` at the end of its
   reduce launch (hipExtLaunchKernelGGL events: the kernels' execution, as a rocprofv3 kernel trace sees it, not
   the stream position of a hipEventRecord).  Events from es_event_create. */
int es_gemm_tn_big_grouped_timed(const void* table, int count, const int* dims, void* start, void* stop,
                                 hipStream_t stream);
/* timing events for the *_timed launches (hipEvent_t handles): create, elapsed ms (waits for `stop`), destroy */
int es_event_create(void** ev);
int es_event_elapsed(void* start, void* stop, float* ms);
int es_event_destroy(void* ev);
/* bias gradient: out[n] (+)= sum_m Y[m][n]  (workspace >= blocks*N floats) */
int es_colsum(const void* Y, int ld, int M, int N, float* workspace, int blocks, float* out, int accumulate,
              hipStream_t stream);
/* out[n] (+)= sum_g P[g][n]  (per-workgroup partials -> parameter gradient) */
int es_reduce_partials(const float* P, float* out, int G, int N, int accumulate, hipStream_t stream);

/* tuning knob: forward attention kernel -- 7 (default) = seven waves per workgroup at 13 key tiles (193 <= T <= 208: ViT/16 at 224^2),
   else as 2; 2 = four waves, register budget of two workgroups per CU; 3 = four waves, three per CU;
   returns previous */
int es_set_attn_variant(int occ);
/* attention backward loops: 4 (default) = the single-pass kernel for 13-tile heads (192 < T <= 208), else
   as 3; 3 = two query / key tiles per wave item (dq2 / dkv2), 2 = pipelined dQ + dkv2, 1 = software-pipelined,
   0 = plain (all bit-identical); returns the previous value, or -2 (state unchanged) for any other value */
int es_set_attn_bwd_variant(int v);
/* tuning knob: the single-pass attention backward's workgroups (-1, the default: max(CUs, heads / 4);
   0: one persistent workgroup per CU); returns the previous value */
int es_set_attn_bwd_grid(int workgroups);
/* 1 (default): the backward variant above also for T > 256 (the 37-tile kernels); 0: plain loops there. */
int es_set_attn_bwd_long(int v);
/* ---- attention (code/models/conformer.py:40-50), head dim 64, tokens T <= 592 (384^2 / 16) ------ */
int es_attn_fwd(const void* qkv, int ldqkv, void* o, int ldo, float* lse, int nimg, int T, int H, float scale,
                hipStream_t stream);
/* delta: fp32 workspace [nimg*H*T] (rowsum(dO*O), produced by the dQ pass for the dK/dV pass; the single-pass
   kernel that 13-tile heads (192 < T <= 208) use by default keeps it on chip and leaves the workspace untouched) */
int es_attn_bwd(const void* qkv, int ldqkv, const void* o, int ldo, const float* lse, float* delta, const void* dout,
                int lddo, void* dqkv, int lddqkv, int nimg, int T, int H, float scale, hipStream_t stream);
/* CLS-query attention for a block whose non-CLS outputs are unused (the last block: only the CLS
 * token reaches timm's head, VisionTransformer.forward_features x[:, 0]).  o / dout are compact
 * [nimg, ld] CLS rows, lse [nimg*H]; the backward writes dqkv for every token (q part zero off the
 * CLS rows), as es_attn_bwd would for a dout that is zero off the CLS rows. */
int es_attn_cls_fwd(const void* qkv, int ldqkv, void* o, int ldo, float* lse, int nimg, int T, int H, float scale,
                    hipStream_t stream);
int es_attn_cls_bwd(const void* qkv, int ldqkv, const void* o, int ldo, const float* lse, const void* dout, int lddo,
                    void* dqkv, int lddqkv, int nimg, int T, int H, float scale, hipStream_t stream);

/* ---- LayerNorm(eps) (code/models/conformer.py:58,60,65) -------------------------------------- */
/* tuning knob: 0 = the one-shot forward (a workgroup per 8 rows), > 0 = the grid-stride forward on this many
   workgroups (bit-identical); returns the previous value */
int es_set_ln_fwd_grid(int workgroups);
int es_layernorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, float* mean,
                     float* rstd, int M, int D, float eps, hipStream_t stream);
int es_layernorm_bwd(const float* dy, int lddy, const float* x, int ldx, const float* mean, const float* rstd,
                     const float* gamma, const float* dres, int ldres, float* dx, int lddx, void* dxb, int lddxb,
                     float* dgamma, float* dbeta, float* workspace, int blocks, int M, int D, int accumulate,
                     hipStream_t stream);
// es_layernorm_bwd with dy = d(LN output) in bf16 (what the ViT engine's dgrad GEMMs write: the
// GEMM operands downstream are bf16 already; half the bytes of the fp32 form on both sides)
int es_layernorm_bwd_b16(const void* dy, int lddy, const float* x, int ldx, const float* mean, const float* rstd,
                         const float* gamma, const float* dres, int ldres, float* dx, int lddx, void* dxb, int lddxb,
                         float* dgamma, float* dbeta, float* workspace, int blocks, int M, int D, int accumulate,
                         hipStream_t stream);
// Both backwards with dgamma == dbeta == NULL leave their per-workgroup partials in `workspace`
// (es_layernorm_bwd_grid(blocks, M) rows of D floats for dgamma, then as many for dbeta);
// es_ln_param_grads_multi then reduces up to 32 such workspaces in ONE launch (the ViT engine defers its
// LayerNorms' parameter gradients off the data-gradient chain).  Table entries (host memory, passed by value):
// {const float* workspace; float* dgamma; float* dbeta; int grid; int D; int accumulate; int pad}, all with the
// same (grid >= 64 && D <= 2048) class.  Same sums, bit for bit, as the undeferred backward.
int es_layernorm_bwd_grid(int blocks, int M);
int es_ln_param_grads_entry_size(void);
int es_ln_param_grads_multi(const void* table, int n, hipStream_t stream);

/* ---- standalone GELU (nn.GELU, exact erf) ---------------------------------------------------- */
int es_gelu_fwd(const void* x, void* y, long n, hipStream_t stream);
int es_gelu_bwd(const void* x, const void* dy, void* dx, long n, hipStream_t stream);

/* ---- device input path: TransformFixMatch on the GPU (csrc/device_aug.hip) --------------------------
 * code/dataset.py:24-56 (Resize -> [CenterCrop] = the weak view; -> RandomHorizontalFlip -> RandomCrop(S,
 * pad int(0.125 S), reflect) -> RandAugmentMC(2, 10) = the strong view) and code/randaugment.py:147-222, from
 * decoded RGB HWC frames of ragged sizes in one device byte arena to planar uint8 [n][3][S][S] batches (the
 * input of the uint8 patch gather above).  Every random draw and every double-precision parameter is resolved
 * on the host into one EsAugEntry per image plus Pillow's 22-bit bilinear tables (include/endossl_aug_plan.h;
 * written by libendossl_host.so, include/endossl_host.h); the kernels are integer / fp32 ports of that
 * library's pixel loops and their output is byte-identical to its batch builder's for the same (seed, index).
 * Nothing here allocates or synchronises.
 *
 * The fixmatch call: frames = the arena (frames_bytes long), entries = n EsAugEntry (8-byte aligned), coeffs =
 * coeff_count int32 of tables, max_h = the tallest frame of the batch (sizes the horizontal pass's temporary),
 * weak / strong = the outputs; strong may be NULL (the evaluation transform, code/dataset.py:217-231).  The
 * strong call runs the strong chain alone from S x S planar views (weak) under the entries' flip / crop / op /
 * Cutout fields.  workspace: the byte count the matching query returns (0 for shapes the calls refuse).
 * ES_BAD_SHAPE: n <= 0 or above 65535, S < 2 or above 4096, a reflect pad int(0.125 S) >= S, max_h <= 0;
 * ES_BAD_ARG: a null or misaligned pointer, a workspace smaller than the query's.  An entry that points outside
 * the arena, the tables or the temporary is skipped by the kernels (its outputs are not written). */
size_t es_aug_entry_size(void);
size_t es_aug_strong_workspace(int n, int S);
size_t es_aug_fixmatch_workspace(int n, int S, int is_crop, int max_w, int max_h);
int es_aug_fixmatch_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                       size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* weak, uint8_t* strong,
                       void* workspace, size_t workspace_bytes, hipStream_t stream);
int es_aug_strong_u8(const uint8_t* weak, const void* entries, int n, int S, uint8_t* strong, void* workspace,
                     size_t workspace_bytes, hipStream_t stream);

/* TransformCoMatch (code/dataset.py:58-110) and the labeled train transform (:185-196) the same way: entries = n
 * EsAugCoEntry / EsAugLabEntry (esh_comatch_device_plan / esh_labeled_device_plan), every other argument, the
 * refusals and the skipping of bad entries as in the fixmatch call; no output may be NULL.
 *   comatch (4 launches): both resize passes once, the vertical one writing the unflipped base and the weak view
 *     with its flip; strong_0 = the strong chain of the base (crop window = the image); strong_1 = the jitter chain.
 *   labeled (3 launches): the vertical pass keeps the whole R x R image; one gather makes the S x S CenterCrop
 *     window of the flipped, rotated image (Pillow's 16.16 walk, black outside); then the jitter chain.
 * The jitter chain (up to four ColorJitter ops in the plan's order, RandomGrayscale, the flip) includes
 * ColorJitter's hue: Pillow's HSV round trip per pixel, in the host's float / double types with IEEE division,
 * fmod, floor and round.  es_aug_jitter_u8 runs that chain alone from S x S planar views x under n EsAugJitter
 * plans (4-byte aligned) into out (not x itself); it needs no workspace. */
size_t es_aug_comatch_entry_size(void);
size_t es_aug_labeled_entry_size(void);
size_t es_aug_comatch_workspace(int n, int S, int is_crop, int max_w, int max_h);
size_t es_aug_labeled_workspace(int n, int S, int is_crop, int max_w, int max_h);
int es_aug_comatch_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                      size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* weak, uint8_t* strong0,
                      uint8_t* strong1, void* workspace, size_t workspace_bytes, hipStream_t stream);
int es_aug_labeled_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                      size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* out, void* workspace,
                      size_t workspace_bytes, hipStream_t stream);
int es_aug_jitter_u8(const uint8_t* x, const void* plans, int n, int S, uint8_t* out, hipStream_t stream);


/* ---- ViT ends: patches, CLS/pos rows, embedding backward, final LN + head on CLS ------------- */
int es_patch_im2col(const float* img, void* patches, int n, int S, int P, hipStream_t stream);

// es_patch_im2col from uint8 pixels [n, 3, S, S]: ToTensor (x / 255) then Normalize ((x - mean[c]) /
// std[c]) in fp32, IEEE divisions (code/dataset.py:21-22,49-51 -- torchvision's transforms on the
// host), then the same bf16 patch permutation.  img 8-byte aligned.
int es_patch_im2col_u8(const void* img, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                       void* patches, int n, int S, int P, hipStream_t stream);
int es_cls_init(float* x, int ldx, const float* cls, const float* pos, int n, int T, int D, hipStream_t stream);
int es_embed_bwd(const float* dx, int lddx, void* dpatch, int ldp, float* dpos, float* dcls, int n, int T, int D,
                 int accumulate, hipStream_t stream);
int es_cls_head_fwd(const float* x, int ldx, int T, const float* gamma, const float* beta, const float* W,
                    const float* b, float* logits, int ldl, float* xhat, float* rstd, int n, int D, int C, float eps,
                    hipStream_t stream);
int es_cls_head_bwd(const float* dl, int lddl, const float* W, const float* gamma, const float* beta,
                    const float* xhat, const float* rstd, float* dyn, float* dx, int lddx, int T, float* dW, float* db,
                    float* dgamma, float* dbeta, int n, int D, int C, hipStream_t stream);
/* the same with dW / db / dgamma / dbeta written (accumulate = 0) instead of added to (1): the first writer of
 * those gradient entries in a step, so the flat gradient buffer needs no zero fill before the backward */
int es_cls_head_bwd_ex(const float* dl, int lddl, const float* W, const float* gamma, const float* beta,
                       const float* xhat, const float* rstd, float* dyn, float* dx, int lddx, int T, float* dW,
                       float* db, float* dgamma, float* dbeta, int n, int D, int C, int accumulate, hipStream_t stream);

/* CoMatch features: fts [n, D] = LN(x_cls) (ModelwEmb's `fts` over the ViT trunk,
 * code/models/custom_model.py:207-209) and its backward into the CLS rows of dx; dgamma / dbeta
 * accumulated (+=), the images summed in a fixed order (no atomics: repeated launches give the same bits). */
int es_cls_ln_fwd(const float* x, int ldx, int T, const float* gamma, const float* beta, float* fts, int ldf,
                  float* xhat, float* rstd, int n, int D, float eps, hipStream_t stream);
int es_cls_ln_bwd(const float* dfts, int lddf, const float* gamma, const float* xhat, const float* rstd, float* dx,
                  int lddx, int T, float* dgamma, float* dbeta, int n, int D, hipStream_t stream);

/* ---- CoMatch heads (fp32; code/models/custom_model.py:107-145,201-205) ------------------------- */
/* Every leading dimension of a used operand must be at least its width (else ES_BAD_SHAPE, before any launch); the
 * same holds for es_comatch_focal_fwd_bwd, es_fm_consistency_fwd_bwd, es_poly_ce_fwd_bwd and es_ce_weighted_*. */
/* Y = act(X W^T + b) (* keep * keep_scale, the replayed Dropout keep-mask, uint8 [n, N]);
 * act 0 = none, 1 = ReLU, 2 = LeakyReLU(slope) */
int es_dense_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, int n, int K, int N,
                 int act, float slope, const void* keep, float keep_scale, hipStream_t stream);
size_t es_dense_bwd_workspace(int n, int N);
/* backward of es_dense_fwd given its output Yact: dW, db overwritten; dX (+)= when dX != NULL */
int es_dense_bwd(const float* dY, int lddy, const float* Yact, int ldya, int act, float slope, const void* keep,
                 float keep_scale, const float* X, int ldx, const float* W, float* dX, int lddx, int accumulate_dx,
                 float* dW, float* db, int n, int K, int N, float* workspace, hipStream_t stream);
/* The same two layers as tiled fp32 GEMMs on the exact f32-input MFMA (csrc/dense_wide.hip), for the heads over a wide
 * trunk (ResNet-50: D = 2048): arguments and semantics of es_dense_fwd / es_dense_bwd, K and N up to 4096 and n up to
 * 65535 * 32 rows (the row tiles are one grid dimension; more is ES_BAD_SHAPE, a workspace of 0 floats), results
 * bit-identical from run to run (split reductions go through the workspace and are added in a fixed order; no
 * atomics).  The workspace holds dpre [n, N] and the split partials of dW and, with want_dx, of dX.
 * es_dense_wide_tile(0 / 1 / 2 / 3): the kernels' row tile, column tile, reduction step and the workgroup count the
 * backward splits its reductions towards (what the tile-edge tests derive their shapes from). */
int es_dense_wide_tile(int which);
int es_dense_wide_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int ldy, int n, int K, int N,
                      int act, float slope, const void* keep, float keep_scale, hipStream_t stream);
size_t es_dense_wide_bwd_workspace(int n, int K, int N, int want_dx);
int es_dense_wide_bwd(const float* dY, int lddy, const float* Yact, int ldya, int act, float slope, const void* keep,
                      float keep_scale, const float* X, int ldx, const float* W, float* dX, int lddx,
                      int accumulate_dx, float* dW, float* db, int n, int K, int N, float* workspace,
                      hipStream_t stream);
/* BatchNorm1d (nn.BatchNorm1d semantics): train = batch statistics + running-buffer update
 * (momentum, unbiased variance, num_batches_tracked int64 += 1), eval = running statistics */
int es_bn1d_fwd(const float* U, int ldu, const float* gamma, const float* beta, float* running_mean, float* running_var,
                void* num_batches_tracked, float momentum, float eps, int train, float* Y, int ldy, float* xhat,
                float* rstd, int n, int F, hipStream_t stream);
int es_bn1d_bwd(const float* dY, int lddy, const float* xhat, const float* rstd, const float* gamma, float* dU,
                int lddu, float* dgamma, float* dbeta, int n, int F, hipStream_t stream);
/* SyncBatchNorm1d pieces for the data-parallel CoMatch head (statistics over the global batch of N
 * rows, the caller all-reducing the per-feature sums between launches; code/models/custom_model.py:
 * 110-116 BatchNorm1d as one process computes it on the concatenated batch):
 *   es_bn1d_sums: out[f] = sum_i U[i][f] (S1 NULL) or sum_i (U[i][f] - S1[f]/N)^2;
 *   es_bn1d_fwd_global: y / xhat / rstd from the global S1, S2, running-buffer update (unbiased var);
 *   es_bn1d_bwd_sums: out[f] = sum dY, out[F+f] = sum dY xhat over this rank's rows;
 *   es_bn1d_bwd_global: dU from the all-reduced sums, dgamma / dbeta = this rank's sums. */
int es_bn1d_sums(const float* U, int ldu, int n, int F, const float* S1, float N, float* out, hipStream_t stream);
int es_bn1d_fwd_global(const float* U, int ldu, const float* gamma, const float* beta, const float* S1,
                       const float* S2, float N, float* running_mean, float* running_var, void* num_batches_tracked,
                       float momentum, float eps, float* Y, int ldy, float* xhat, float* rstd, int n, int F,
                       hipStream_t stream);
int es_bn1d_bwd_sums(const float* dY, int lddy, const float* xhat, int n, int F, float* out, hipStream_t stream);
int es_bn1d_bwd_global(const float* dY, int lddy, const float* xhat, const float* rstd, const float* gamma,
                       const float* sums_global, const float* sums_local, float N, float* dU, int lddu,
                       float* dgamma, float* dbeta, int n, int F, hipStream_t stream);
/* Dropout(p) keep-mask (uint8 0/1), counter-based hash of (seed, offset + i) */
int es_dropout_keep(void* keep, long n, float p, unsigned long long seed, unsigned long long offset,
                    hipStream_t stream);
/* Normalize(2) (code/models/custom_model.py:136-145) */
int es_l2norm_fwd(const float* V, int ldv, float* Z, int ldz, float* norm, int n, int L, hipStream_t stream);
int es_l2norm_bwd(const float* dZ, int lddz, const float* Z, int ldz, const float* norm, float* dV, int lddv, int n,
                  int L, hipStream_t stream);

/* ---- CoMatch step (code/comatch.py:162-220) ---------------------------------------------------- */
size_t es_comatch_pseudo_workspace(int nu, int C, int Q);
/* softmax(weak) -> distribution alignment (batch mean appended at hist[hist_pos] of a hist_cap
 * ring, mean of the hist_len newest) -> memory smoothing against the Q-row bank -> argmax / mask.
 * C <= 32, L <= 64. */
int es_comatch_pseudo(const float* logits_w, int ldl, int nu, int C, float* hist, int hist_cap, int hist_len,
                      int hist_pos, const float* z_w, int ldz, int L, const float* bank_feats, const float* bank_probs,
                      int Q, float temperature, float alpha, float thres, float* probs, float* probs_orig, int* pl,
                      float* mask, float* workspace, hipStream_t stream);
/* as es_comatch_pseudo; hist_given = 1: hist[hist_pos] already holds the step's batch mean (the
 * data-parallel path writes the all-ranks mean there: es_softmax_colmean + all-reduce) */
int es_comatch_pseudo_ex(const float* logits_w, int ldl, int nu, int C, float* hist, int hist_cap, int hist_len,
                         int hist_pos, int hist_given, const float* z_w, int ldz, int L, const float* bank_feats,
                         const float* bank_probs, int Q, float temperature, float alpha, float thres, float* probs,
                         float* probs_orig, int* pl, float* mask, float* workspace, hipStream_t stream);
/* out[c] = mean over rows of softmax(logits)[c], C <= 32 (the DA batch mean) */
int es_softmax_colmean(const float* logits, int ldl, int n, int C, float* out, hipStream_t stream);
/* ring write of [z_w; z_x] and [probs_orig; onehot(y)] at bank row ptr (code/comatch.py:187-196) */
int es_comatch_bank_write(const float* z_w, int ldzw, int nu, const float* z_x, int ldzx, int bt, int L,
                          const float* probs_orig, const void* y_int64, int C, float* bank_feats, float* bank_probs,
                          int ptr, int Q, hipStream_t stream);
size_t es_comatch_contrastive_workspace(int nu);
/* loss_out[0] = L_c = mean_i L_i; dz0 / dz1 = grad_scale * d(sum_i L_i)/dz -- pass lambda_c / nu for the
 * gradient of lambda_c * L_c (code/comatch.py:199-213) */
int es_comatch_contrastive_fwd_bwd(const float* z0, int ldz0, const float* z1, int ldz1, const float* probs, int nu,
                                   int L, int C, float temperature, float contrast_th, float grad_scale,
                                   float* loss_out, float* dz0, int lddz0, float* dz1, int lddz1, float* workspace,
                                   hipStream_t stream);
/* the data-parallel form: nr local anchor rows (global rows row_off..) against the nc global columns
 * (all-gathered z1 / probs); loss_out[0] = local row-loss sum / loss_div; dz1_all [nc, L] is this
 * rank's share of d/dz1 for every column (sum it over ranks, keep the own rows) */
size_t es_comatch_contrastive_ex_workspace(int nr, int nc);
int es_comatch_contrastive_fwd_bwd_ex(const float* z0, int ldz0, const float* z1_all, int ldz1,
                                      const float* probs_rows, const float* probs_all, int nr, int nc, int row_off,
                                      int L, int C, float temperature, float contrast_th, float grad_scale,
                                      float loss_div, float* loss_out, float* dz0, int lddz0, float* dz1_all,
                                      int lddz1, float* workspace, hipStream_t stream);
/* loss_out[0] = L_u = mean_i L_i; dls = grad_scale * d(sum_i L_i)/dlogits -- pass lambda_u / nu
 * (code/comatch.py:215-220); workspace nu floats */
int es_comatch_focal_fwd_bwd(const float* ls, int ldl, const float* probs, const float* mask, int nu, int C,
                             float gamma, float grad_scale, float* loss_out, float* dls, int lddl, float* workspace,
                             hipStream_t stream);

/* ---- FixMatch losses, forward + gradient fused ------------------------------------------------ */
/* code/loss.py:126-164 consistency_loss(name='ce', use_hard_labels=True); out[0]=loss, out[1]=mask mean */
int es_fm_consistency_fwd_bwd(const float* logits_w, int ldw, const float* logits_s, int lds, int n, int C,
                              float tau, float grad_scale, int* pseudo_label, uint8_t* mask, float* row_loss,
                              float* dlogits_s, int lddls, float* out, hipStream_t stream);
/* code/loss.py:103-114,308-364 ce_loss(type_loss='poly') = PolyLoss(epsilon=2); out[0]=loss.  A target outside
 * [0, C) as a 64-bit value (2^32 + 3 is not class 3): NaN loss, zero gradient in that row, no out-of-range read;
 * es_ce_weighted_* and es_ce_weight_sum check their targets the same way. */
int es_poly_ce_fwd_bwd(const float* logits, int ldl, const int64_t* targets, const float* weights, int n, int C,
                       float epsilon, float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream);

/* ---- supervised triplet mode (code/supervised.py:84-108,238-268) ------------------------------- */
/* code/loss.py:170-190 TripletLoss on z [3 bs, L] fp32, rows [0,bs) anchors, [bs,2bs) positives, [2bs,3bs)
 * negatives: h_i = |z_a - z_p| - |z_a - z_n| + alpha; out[0] = mean max(h_i, 0), out[1] = mean d_p,
 * out[2] = mean d_n, out[3] = fraction of h_i > 0.  dz = grad_scale * d(sum_i max(h_i, 0))/dz -- pass
 * lambda_c / bs; every row is written (zeros where h_i <= 0; a unit direction is 0 at distance 0).
 * 1 <= L <= 2048; no atomics: repeated launches give the same bits */
int es_triplet_fwd_bwd(const float* z, int ldz, int bs, int L, float alpha, float grad_scale, float* dz, int lddz,
                       float* out, hipStream_t stream);
/* per row of logits [n, C <= 64]: pred = argmax (first index on ties), conf = max softmax probability,
 * label = conf > thres ? pred : 0 (code/supervised.py:258-266); each output nullable, not all three */
int es_softmax_predict(const float* logits, int ldl, int n, int C, float thres, int* pred, float* conf, int* label,
                       hipStream_t stream);

/* ---- supervised angular-margin mode (code/supervised.py:117-119) ------------------------------- */
/* code/loss.py:228-266 AngularPenaltySMLoss.forward and its autograd in one call.  x [n, F] fp32 (row stride
 * ldx), W [C, F] row-major (nn.Linear's weight, NOT normalised: the reference's normalisation of it rebinds a
 * local), bias [C] nullable, int64 targets, class weights w [C] and per-row mask [n] nullable (1 when absent):
 *   x^_i = x_i / max(|x_i|, 1e-12);  z = x^ W^T (+ bias);  t_i = z[i][y_i];  tc = clamp(t, -1 + eps, 1 - eps)
 *   kind 0 cosface     num_i = s (t - m)
 *        1 arcface     num_i = s cos(acos(tc) + m)
 *        2 sphereface  num_i = s cos(m acos(tc))
 *        3 acloss      num_i = s g_theta(acos(tc) + m), g_theta of code/loss.py:262-266 (k = 0.3)
 *   L_i = w[y_i] mask_i (num_i - log(exp(num_i) + sum_{j != y_i} exp(s z_ij)));  out[0] = -grad_scale sum_i L_i
 * (pass 1/n: a plain mean, not weight-normalised).  The log-sum-exp subtracts its maximum, so the value stays
 * finite where the reference's literal exp overflows (s z > 88).  The clamp passes no gradient outside its range:
 * such a row's target logit gets none (kinds 1-3), and its loss uses the clamped cosine.
 * Writes every entry of dx [n, F] (row stride lddx; through the normalisation), dW [C, F] and db [C] (nullable)
 * -- the gradients of out[0] -- and of row_loss [n] (nullable; -L_i, not scaled).  An out-of-range target
 * gives a NaN loss and a zero gradient row.  workspace: es_margin_softmax_workspace(n, C) floats (0 for an
 * unsupported n / C).  No atomics, fixed summation order: repeated launches give the same bits.
 * 1 <= C <= 64, F % 4 == 0, 4 <= F <= 2048, n >= 1, ldx / lddx >= F and % 4 == 0, x / W / dx / dW 16-byte
 * aligned, kind in 0..3, 0 < eps < 1, x / W / targets / dx / dW / out / workspace non-null: anything else returns -2 (bad
 * argument) before any launch, and nothing is written. */
size_t es_margin_softmax_workspace(int n, int C);
int es_margin_softmax_fwd_bwd(const float* x, int ldx, const float* W, const float* bias, const int64_t* targets,
                              const float* class_weights, const float* mask, int n, int F, int C, int kind, float s,
                              float m, float eps, float grad_scale, float* dx, int lddx, float* dW, float* db,
                              float* out, float* row_loss, float* workspace, hipStream_t stream);

/* ---- EZBM stage 2 (code/ezbm.py:133-182; csrc/ezbm.hip) ------------------------------------------
 * fp32, no atomics (repeated launches give the same bits), every output entry written.  A bad shape returns -1,
 * a null required pointer -2, before any launch. */
/* EmbFeatEZBM.__getitem__ (code/dataset.py:135-175) for n rows in one launch, and the mix of code/ezbm.py:162.
 * mem [N, D] (row stride ldm) is the feature bank, mem_y [N] its int64 targets; cls_off [C+1] / cls_idx [N]
 * (int32) list the bank rows by class (CSR, ascending within a class); cdf [C] is the dual draw's class CDF;
 * lam_table [C*C] holds lam for (t, td).  Row i draws from the splitmix64 counter hash of es_dropout_keep at
 * counters offset + 4i + k: k = 0 the row's class, ((z >> 40) * C) >> 24; k = 1 its member among the class's m
 * rows, ((z >> 40) * m) >> 24; k = 2 the dual's class, the first c with (z >> 40) * 2^-24 < cdf[c] (the last
 * class if none); k = 3 the dual's member.  With idx_in / dual_in (int32 [n], both or neither) nothing is drawn:
 * those rows are used, and cls_off / cls_idx / cdf may be NULL.
 * Out: X [2n, D] (row stride ldx): X[i] = mem[idx_i], X[n+i] = lam_i * mem[idx_i] + (1 - lam_i) * mem[dual_i]
 * in torch's fp32 rounding (two rounded products, one rounded sum; 1 - lam_i rounded once); t / td [n] int64 =
 * mem_y[idx] / mem_y[dual]; lam [n] = lam_table[t * C + td]; idx / dual [n] int32 the rows used.  A row index
 * outside [0, N) (a bad replay index, an empty class) reads nothing: NaN rows, targets -1; a stored target
 * outside [0, C) gives lam = NaN.  1 <= D <= 2048, 1 <= C <= 64, 1 <= N < 2^24, ldm / ldx >= D. */
int es_ezbm_sample_mix(const float* mem, int ldm, const int64_t* mem_y, int N, int D, int C, const int* cls_off,
                       const int* cls_idx, const float* cdf, const float* lam_table, unsigned long long seed,
                       unsigned long long offset, const int* idx_in, const int* dual_in, int n, float* X, int ldx,
                       int64_t* t, int64_t* td, float* lam, int* idx, int* dual, hipStream_t stream);
/* BatchNorm1d in train mode over G consecutive groups of n rows (U [G*n, F]): each group normalised with its own
 * batch mean / biased variance; the running buffers updated G times in group order (momentum, unbiased
 * variance), num_batches_tracked (nullable) += G; xhat [G*n, F] and rstd [G, F] saved.  The backward gives each
 * group's dU from that group's own sums; dgamma / dbeta = the groups' sums added in group order (overwritten).
 * G = 1 is es_bn1d_fwd / es_bn1d_bwd bit for bit.  n >= 2, G >= 1, row strides >= F. */
int es_bn1d_groups_fwd(const float* U, int ldu, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, void* num_batches_tracked, float momentum, float eps, float* Y, int ldy,
                       float* xhat, float* rstd, int n, int G, int F, hipStream_t stream);
int es_bn1d_groups_bwd(const float* dY, int lddy, const float* xhat, const float* rstd, const float* gamma, float* dU,
                       int lddu, float* dgamma, float* dbeta, int n, int G, int F, hipStream_t stream);
/* code/ezbm.py:163-167 on logits [2n, C], rows [0, n) = outputs_o, [n, 2n) = outputs_s, int64 t / td [n]:
 *   l_o = mean_i CE(o_i, t_i);  l_s = 0.5 mean_i CE(s_i, t_i) + 0.5 mean_i CE(s_i, td_i)   (plain means)
 *   out = {l_o + lambda_c l_s, l_o, l_s}
 *   dlogits[i]   = grad_scale (softmax(o_i) - e_t) / n
 *   dlogits[n+i] = grad_scale lambda_c (softmax(s_i) - 0.5 e_t - 0.5 e_td) / n
 * A t_i or td_i outside [0, C) gives a NaN loss and zero gradient rows i and n+i.  C >= 1, ldl / lddl >= C. */
int es_ezbm_ce_fwd_bwd(const float* logits, int ldl, const int64_t* t, const int64_t* td, int n, int C, float lambda_c,
                       float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream);

/* ---- Conformer CNN branch (SemiFormer backbone, code/models/conformer.py:75-445) ---------------
 * fp32 NHWC maps with element strides; Conv2d groups = 1, weights in the reference layout
 * [Cout][Cin][kh][kw].  Replaces the reference's aten conv2d / batch_norm / max_pool2d /
 * avg_pool2d / upsample_nearest2d calls in ConvBlock, FCUDown, FCUUp and the stem. */
/* 1 (default): the 3 -> 64 channel 7x7 / stride-2 / pad-3 stem (Conformer.conv1, resnet18.conv1) on NHWC fp32
 * images runs on its own forward (bit-identical to the generic kernel) and weight-gradient kernels inside
 * es_conv2d_fwd / es_conv2d_bwd_weight; 0: the generic kernels.  Returns the previous value. */
int es_set_stem_kernels(int v);
int es_conv2d_fwd(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                  const float* w, const float* bias, int Cout, int kh, int kw, int stride, int pad, float* y, long syn,
                  long syh, long syw, int accumulate, hipStream_t stream);
int es_conv2d_bwd_data(const float* dy, long syn, long syh, long syw, const float* w, int N, int H, int W, int Cin,
                       int Cout, int kh, int kw, int stride, int pad, float* dx, long sxn, long sxh, long sxw, long sxc,
                       int accumulate, hipStream_t stream);
// workgroup tiles (Cout x Cin kh kw) one pixel split of es_conv2d_bwd_weight launches: callers size
// `splits` so that tiles x splits fills the chip
int es_conv2d_dw_tiles(int Cout, int Cin, int kh, int kw);
size_t es_conv2d_bwd_weight_workspace(int Cout, int Cin, int kh, int kw, int splits);
int es_conv2d_bwd_weight(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                         const float* dy, long syn, long syh, long syw, int Cout, int kh, int kw, int stride, int pad,
                         int splits, float* workspace, float* dw, int accumulate, hipStream_t stream);
/* bf16-operand forms of the three convs above (csrc/conv_bf16.hip): the same fp32 maps and
 * geometry arguments, operands rounded to bf16 as they are staged, fp32 accumulation on
 * v_mfma_f32_16x16x32_bf16.  Taken for eligible convs (Cin, Cout multiples of 32) when
 * the maps have channel stride 1 with 16-byte aligned pixel rows.  Weights go through
 * es_conv2d_pack_bf16 first: wp [Cout][kh kw][Cin] (forward), wt [Cin][kh kw][Cout] (data grad),
 * Cout Cin kh kw bf16 each, either pointer may be null. */
int es_conv2d_bf16_eligible(int Cin, int Cout, int kh, int kw);
/* tuning knob: the workgroup count the bf16 weight gradient's automatic pixel split aims at (default 512;
   each split writes an fp32 slab of the gradient that a reduce kernel sums); returns the previous value */
int es_set_conv_dw_target(int v);
/* tuning knob: the bf16-map data-gradient convs and the forwards that do not widen the channels on the LDS-DMA
 * ring kernel with 3 or 4 stages (default 3), or 0 = the register-staged gather (bit-identical); returns the
 * previous value, or -2 (unchanged) otherwise */
int es_set_conv_ring(int stages);
/* tuning knob: 1 (default) = the register-staged bf16 conv kernels (weight gradient; forward / data gradient off the
 * ring) with branch-free (range-checked buffer) loads and pixel walk where they apply, 0 = the branchy loads
 * (bit-identical); returns the previous value, or -2 otherwise */
int es_set_conv_dw_buf(int v);
/* tuning knob: a bf16 conv forward / data gradient whose 128-channel tiling would launch fewer than `wgs`
 * workgroups (default 128; 0 = never) runs on the 64-channel tile: twice the workgroups on small maps, the same
 * per-element reduction order (bit-identical); returns the previous value, or -2 (unchanged) for wgs < 0 */
int es_set_conv_small(int wgs);
int es_conv2d_pack_bf16(const float* w, int Cout, int Cin, int kh, int kw, void* wp, void* wt, hipStream_t stream);
/* es_conv2d_pack_bf16 for n weights in ONE launch (a model's conv weights after each optimizer step):
 * table = n device-resident entries of es_conv_pack_entry_size() bytes
 * {const float* w; void* wp; void* wt; int Cout; int Cin; int kh_x_kw; int pad}, max_elems = the largest
 * Cout * Cin * kh * kw (sizes the grid).  Same images, bit for bit. */
int es_conv_pack_entry_size(void);
int es_conv2d_pack_bf16_multi(const void* table, int n, long max_elems, hipStream_t stream);
int es_conv2d_fwd_bf16(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                       const void* wp, const float* bias, int Cout, int kh, int kw, int stride, int pad, float* y,
                       long syn, long syh, long syw, int accumulate, hipStream_t stream);
int es_conv2d_bwd_data_bf16(const float* dy, long syn, long syh, long syw, const void* wt, int N, int H, int W,
                            int Cin, int Cout, int kh, int kw, int stride, int pad, float* dx, long sxn, long sxh,
                            long sxw, long sxc, int accumulate, hipStream_t stream);
/* es_conv2d_fwd_bf16 (overwrite) that also writes y's BatchNorm statistics per 128-pixel block:
 * partials[b][0][c] = block sum, partials[b][1][c] = block-centred sum of squares
 * (es_conv2d_bnstats_size floats) -- es_bn2d_fwd_partials needs no statistics pass over y. */
size_t es_conv2d_bnstats_size(int M, int Cout);
int es_conv2d_fwd_bf16_bnstats(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                               const void* wp, const float* bias, int Cout, int kh, int kw, int stride, int pad,
                               float* y, long syn, long syh, long syw, float* partials, hipStream_t stream);
/* workspace floats for M = N Ho Wo output pixels; splits <= 0 sizes the pixel split automatically */
size_t es_conv2d_bwd_weight_bf16_workspace(int M, int Cout, int Cin, int kh, int kw, int splits);
int es_conv2d_bwd_weight_bf16(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                              const float* dy, long syn, long syh, long syw, int Cout, int kh, int kw, int stride,
                              int pad, int splits, float* workspace, float* dw, int accumulate, hipStream_t stream);
size_t es_chan_workspace(int rows, int C);
/* out[c] (+)= sum_r v[(r / HW) * sn + (r % HW) * sp + c]  (bias gradients) */
int es_chan_sum(const float* v, int rows, int C, long sn, long sp, int HW, float* workspace, float* out,
                int accumulate, hipStream_t stream);
/* BatchNorm2d (train: batch stats, running update, num_batches_tracked += 1; eval: running stats),
 * y = bn(x) (+ res) then ReLU if relu.  workspace: es_chan_workspace(rows, C) floats. */
int es_bn2d_fwd(const float* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                float* running_var, void* num_batches_tracked, float momentum, float eps, int train, const float* res,
                int relu, float* y, float* mean, float* rstd, float* workspace, hipStream_t stream);
int es_bn2d_bwd(const float* x, const float* y, const float* dy, int rows, int C, int relu, const float* gamma,
                const float* mean, const float* rstd, int train, const float* running_var, float eps, float* dx,
                float* gout, float* dgamma, float* dbeta, int accumulate, float* workspace, hipStream_t stream);
/* Train-mode BatchNorm2d with the batch statistics from es_conv2d_fwd_bf16_bnstats' partials of x
 * (128-row blocks, combined as Chan et al. in two levels of 64 blocks; the first level overwrites
 * partials in place): running stats, num_batches_tracked, mean / rstd and y = bn(x) (+ res) (relu)
 * as es_bn2d_fwd. */
int es_bn2d_fwd_partials(const float* x, int rows, int C, float* partials, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, void* num_batches_tracked,
                         float momentum, float eps, const float* res, int relu, float* y, float* mean, float* rstd,
                         hipStream_t stream);
/* SyncBatchNorm2d: the Conformer's BatchNorm2d over the global batch at N > 1 (SURVEY.md §8(e):
 * exact parity with the single-process step needs the statistics of every rank's rows).  Flow per
 *  BatchNorm: es_bn2d_sums [mode 0] -> all-reduce -> es_bn2d_sums [mode 1: centred on the global mean]
 * -> all-reduce -> es_bn2d_fwd_global; backward: es_bn2d_bwd_sums -> all-reduce of a copy ->
 * es_bn2d_bwd_global [dx from the global sums, dgamma / dbeta from the local ones].  rows_g = the
 * rows of every rank together; workspace = es_chan_workspace(rows, C) floats. */
int es_bn2d_sums(const float* x, int rows, int C, int mode, const float* sum_g, int rows_g, float* out,
                 float* workspace, hipStream_t stream);
int es_bn2d_fwd_global(const float* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, void* num_batches_tracked, float momentum, float eps, const float* sum_g,
                       const float* sq_g, int rows_g, const float* res, int relu, float* y, float* mean, float* rstd,
                       hipStream_t stream);
int es_bn2d_bwd_sums(const float* x, const float* y, const float* dy, int rows, int C, int relu, const float* mean,
                     const float* rstd, float* out, float* workspace, hipStream_t stream);
int es_bn2d_bwd_global(const float* x, const float* y, const float* dy, int rows, int C, int relu, const float* gamma,
                       const float* mean, const float* rstd, const float* sums_local, const float* sums_g, int rows_g,
                       float* dx, float* gout, float* dgamma, float* dbeta, int accumulate, hipStream_t stream);
int es_maxpool2d_fwd(const float* x, int N, int H, int W, int C, int k, int s, int p, float* y, void* arg,
                     hipStream_t stream);
int es_maxpool2d_bwd(const float* dy, const void* arg, int N, int H, int W, int C, int k, int s, int p, float* dx,
                     hipStream_t stream);
int es_avgpool2d_fwd(const float* x, int N, int H, int W, int C, int k, float* y, hipStream_t stream);
int es_avgpool2d_bwd(const float* dy, int N, int H, int W, int C, int k, float* dx, int accumulate,
                     hipStream_t stream);
int es_upsample_add_fwd(const float* base, const float* src, int N, int H, int W, int C, int s, float* out,
                        hipStream_t stream);
int es_upsample_bwd(const float* dout, int N, int H, int W, int C, int s, float* dsrc, hipStream_t stream);

/* ---- bf16 activation / gradient maps (the Conformer CNN branch when every conv of the branch takes the
 * bf16 kernels: conformer.NativeConformer.map_bf16).  Same arguments as the fp32 entry points above plus
 * `flags`: conv fwd / data grad, pools: bit 0 = the input map is bf16, bit 1 = the output map is bf16;
 * conv weight grad: bit 0 = x bf16, bit 1 = dy bf16; BatchNorm / chan_sum / upsampling: bit 0 = every map
 * argument bf16.  Arithmetic in fp32, each output rounded once (an accumulating store adds in fp32).
 * These replace the same reference ops as their fp32 forms (code/models/conformer.py:75-200 ConvBlock /
 * FCUDown / FCUUp, torch autocast's bf16 conv outputs). */
int es_conv2d_fwd_bf16_ex(const void* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                          const void* wp, const float* bias, int Cout, int kh, int kw, int stride, int pad, void* y,
                          long syn, long syh, long syw, int accumulate, float* bn_partials, int flags,
                          hipStream_t stream);
int es_conv2d_bwd_data_bf16_ex(const void* dy, long syn, long syh, long syw, const void* wt, int N, int H, int W,
                               int Cin, int Cout, int kh, int kw, int stride, int pad, void* dx, long sxn, long sxh,
                               long sxw, long sxc, int accumulate, int flags, hipStream_t stream);
int es_conv2d_bwd_weight_bf16_ex(const void* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                                 const void* dy, long syn, long syh, long syw, int Cout, int kh, int kw, int stride,
                                 int pad, int splits, float* workspace, float* dw, int accumulate, int flags,
                                 hipStream_t stream);
/* The same forward / weight-gradient convs when x is the INPUT of a train-mode BatchNorm2d + ReLU whose output
 * feeds this conv alone (ConvBlock bn1 -> conv2, bn2 -> conv3, code/models/conformer.py:118-134): the gathers
 * apply relu((x - mean) rstd gamma + beta), rounded to x's map type exactly as es_bn2d_fwd*_ex stores it,
 * so the normalised map is never written (es_bn2d_fwd_partials_ex with y = NULL gives mean / rstd; the
 * backward is es_bn2d_bwd_recompute_ex).  Per-channel arrays 16-byte aligned. */
int es_conv2d_fwd_bf16_bnin_ex(const void* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                               const void* wp, const float* bias, int Cout, int kh, int kw, int stride, int pad,
                               void* y, long syn, long syh, long syw, int accumulate, float* bn_partials, int flags,
                               const float* in_mean, const float* in_rstd, const float* in_gamma,
                               const float* in_beta, hipStream_t stream);
int es_conv2d_bwd_weight_bf16_bnin_ex(const void* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw,
                                      long sxc, const void* dy, long syn, long syh, long syw, int Cout, int kh, int kw,
                                      int stride, int pad, int splits, float* workspace, float* dw, int accumulate,
                                      int flags, const float* in_mean, const float* in_rstd, const float* in_gamma,
                                      const float* in_beta, hipStream_t stream);
/* Direct 1 x 1 convolution (timm Bottleneck conv1 / conv3 / downsample.0 at stride 1: nn.Conv2d(k=1)).  A 1 x 1
 * stride-1 unpadded conv over a dense NHWC bf16 map of M = N H W pixels is the NT GEMM y[M, Cout] = x[M, Cin] .
 * wp[Cout, Cin]^T: these read the rows with plain row-major 16-byte loads instead of the implicit-GEMM gather.
 * Same packed weights, same flags (bit 0, the input map is bf16, must be set), same outputs and the same
 * bn_partials as es_conv2d_fwd_bf16_ex / _bnin_ex / es_conv2d_bwd_data_bf16_ex, bit for bit.  Maps and weights
 * under 2 GiB each. */
int es_conv1x1_fwd_bf16_ex(const void* x, int M, int Cin, const void* wp, const float* bias, int Cout, void* y,
                           int accumulate, float* bn_partials, int flags, hipStream_t stream);
int es_conv1x1_fwd_bf16_bnin_ex(const void* x, int M, int Cin, const void* wp, const float* bias, int Cout, void* y,
                                int accumulate, float* bn_partials, int flags, const float* in_mean,
                                const float* in_rstd, const float* in_gamma, const float* in_beta,
                                hipStream_t stream);
int es_conv1x1_bwd_data_bf16_ex(const void* dy, int M, int Cout, const void* wt, int Cin, void* dx, int accumulate,
                                int flags, hipStream_t stream);
/* tuning knob: the direct 1 x 1 kernels for 0 = no conv, 1 (default) = the shape class where they measured faster
 * than the implicit kernels (a reduction 512 deep or more: forward Cin, data gradient Cout), 2 = every
 * conv they can take; returns the previous value, or -2
 * (unchanged) otherwise.  es_conv1x1_bf16_select: 1 when such a conv (kind 0 = forward, 1 = forward with the
 * input BatchNorm, 2 = data gradient) goes to the direct kernel under the knob.  Callers ask only for models that
 * opt in (resnet.NativeResNet bottleneck configs): every other model keeps the implicit kernels. */
int es_set_conv_1x1(int v);
int es_conv1x1_bf16_select(int kind, int M, int Cin, int Cout);
int es_chan_sum_ex(const void* v, int rows, int C, long sn, long sp, int HW, float* workspace, float* out,
                   int accumulate, int flags, hipStream_t stream);
/* tuning knob: 1 (default) = the channel-stationary BatchNorm apply kernels (forward apply and the backward's dx
 * pass), 0 = the per-iteration forms (bit-identical); returns the previous value, or -2 (unchanged) otherwise */
int es_set_bn_cs(int v);
/* test knob: 1 = the BatchNorm channel sums over 8-channel groups (a different fp32 summation order of the same
 * sums), 0 (default) = 4-channel groups; returns the previous value, or -2 (unchanged) otherwise */
int es_set_bn_sum8(int v);
int es_bn2d_fwd_ex(const void* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, void* num_batches_tracked, float momentum, float eps, int train, const void* res,
                   int relu, void* y, float* mean, float* rstd, float* workspace, int flags, hipStream_t stream);
int es_bn2d_bwd_ex(const void* x, const void* y, const void* dy, int rows, int C, int relu, const float* gamma,
                   const float* mean, const float* rstd, int train, const float* running_var, float eps, void* dx,
                   void* gout, float* dgamma, float* dbeta, int accumulate, float* workspace, int flags,
                   hipStream_t stream);
/* es_bn2d_bwd_ex for a train-mode ReLU BatchNorm without residual whose output y was not kept: the ReLU mask
   is rebuilt from x with the forward's affine map and rounding, so the backward reads x and dy only */
int es_bn2d_bwd_recompute_ex(const void* x, const void* dy, int rows, int C, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta, int accumulate,
                             float* workspace, int flags, hipStream_t stream);
/* es_bn2d_fwd_partials(_ex) with y = NULL (and no residual): statistics, running buffers, mean / rstd only */
int es_bn2d_fwd_partials_ex(const void* x, int rows, int C, float* partials, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, void* num_batches_tracked, float momentum,
                            float eps, const void* res, int relu, void* y, float* mean, float* rstd, int flags,
                            hipStream_t stream);
int es_bn2d_sums_ex(const void* x, int rows, int C, int mode, const float* sum_g, int rows_g, float* out,
                    float* workspace, int flags, hipStream_t stream);
int es_bn2d_fwd_global_ex(const void* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, void* num_batches_tracked, float momentum, float eps, const float* sum_g,
                          const float* sq_g, int rows_g, const void* res, int relu, void* y, float* mean, float* rstd,
                          int flags, hipStream_t stream);
int es_bn2d_bwd_sums_ex(const void* x, const void* y, const void* dy, int rows, int C, int relu, const float* mean,
                        const float* rstd, float* out, float* workspace, int flags, hipStream_t stream);
int es_bn2d_bwd_global_ex(const void* x, const void* y, const void* dy, int rows, int C, int relu, const float* gamma,
                          const float* mean, const float* rstd, const float* sums_local, const float* sums_g, int rows_g,
                          void* dx, void* gout, float* dgamma, float* dbeta, int accumulate, int flags,
                          hipStream_t stream);
int es_maxpool2d_fwd_ex(const float* x, int N, int H, int W, int C, int k, int s, int p, void* y, void* arg, int flags,
                        hipStream_t stream);
int es_maxpool2d_bwd_ex(const void* dy, const void* arg, int N, int H, int W, int C, int k, int s, int p, float* dx,
                        int flags, hipStream_t stream);
int es_avgpool2d_fwd_ex(const void* x, int N, int H, int W, int C, int k, void* y, int flags, hipStream_t stream);
int es_avgpool2d_bwd_ex(const void* dy, int N, int H, int W, int C, int k, void* dx, int accumulate, int flags,
                        hipStream_t stream);
int es_upsample_add_fwd_ex(const void* base, const void* src, int N, int H, int W, int C, int s, void* out, int flags,
                           hipStream_t stream);
int es_upsample_bwd_ex(const void* dout, int N, int H, int W, int C, int s, void* dsrc, int flags, hipStream_t stream);
/* FCUDown LayerNorm + GELU + cat(cls) fused with ConvTransBlock's x_st + x_t */
int es_fcu_down_tokens_fwd(const float* pooled, const float* xt, const float* ln_w, const float* ln_b, float* out,
                           float* mean, float* rstd, int N, int np, int D, float eps, hipStream_t stream);
size_t es_fcu_down_workspace(int N, int np, int D);
int es_fcu_down_tokens_bwd(const float* dout, const float* pooled, const float* ln_w, const float* ln_b,
                           const float* mean, const float* rstd, float* dxt, float* dpooled, float* dln_w,
                           float* dln_b, int accumulate, int N, int np, int D, float* workspace, hipStream_t stream);
/* es_fcu_down_tokens_bwd with dxt (+)= when dxt_accumulate (the second consumer of a gradient sink) */
int es_fcu_down_tokens_bwd_ex(const float* dout, const float* pooled, const float* ln_w, const float* ln_b,
                              const float* mean, const float* rstd, float* dxt, float* dpooled, float* dln_w,
                              float* dln_b, int accumulate, int N, int np, int D, float* workspace, int dxt_accumulate,
                              hipStream_t stream);
int es_tokens_cls_set(float* xt, int N, int T, int D, const float* cls, hipStream_t stream);
/* F.cross_entropy(weight=w, reduction='mean') (code/loss.py:118): out[0] = sum w_y l / sum w_y;
 * dlogits = grad_scale * d(out[0]) / d logits */
int es_ce_weighted_fwd_bwd(const float* logits, int ldl, const int64_t* targets, const float* weights, int n, int C,
                           float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream);
/* out[0] = sum_i w[y_i] over this rank's rows (weights nullable -> n) */
int es_ce_weight_sum(const int64_t* targets, const float* weights, int n, int C, float* out, hipStream_t stream);
/* the data-parallel weighted mean (code/loss.py:118 over the GLOBAL batch): *wsum_global = the weight sum over every
 * rank's rows; out[0] = sum_{own rows} w_y l / W_global; dlogits = grad_scale * d(out[0]) / d logits */
int es_ce_weighted_fwd_bwd_global(const float* logits, int ldl, const int64_t* targets, const float* weights,
                                  const float* wsum_global, int n, int C, float grad_scale, float* dlogits, int lddl,
                                  float* out, hipStream_t stream);

/* ---- squeeze-excite bottleneck tail (code/models/se.py:32-58; csrc/se.hip) -------------------- */
/* The tail of an SE-ResNet Bottleneck after conv3, with bn3's output o = gamma (y - mean) rstd + beta never
 * written: a = pool(o) = gamma (pool(y) - mean) rstd + beta, h = relu(a W_down^T), s = sigmoid(h W_up^T),
 * out = relu(s o + res).  y / res / out / dout / dy / gres are NHWC maps [N, HW, C], fp32 (flags 0) or bf16
 * (flags bit 0); ybar, a, s, da, p1, p2 are fp32 [N, C]; h is fp32 [N, R]; w_down [R, C], w_up [C, R] fp32.
 * Supported: C % 16 == 0, 16 <= C <= 2048, 1 <= R <= 128, N, HW >= 1 (else ES_BAD_SHAPE); maps and per-channel
 * arrays 16-byte aligned, no null required pointer (else ES_BAD_ARG); both before any launch.  Every sum is taken
 * in a fixed order (no atomics) and every output element is written. */
/* mean / rstd for the tail where conv3's epilogue partials are not available.  train: from sum = es_bn2d_sums_ex
 * mode 0 and sq = mode 1 over `rows` rows (biased variance; running buffers with the unbiased one,
 * num_batches_tracked += 1 when non-null); eval (train 0): mean = running_mean, rstd = 1 / sqrt(running_var +
 * eps), sum / sq unused */
int es_se_bn_stats(const float* sum, const float* sq, int rows, int C, float eps, float momentum, int train,
                   float* mean, float* rstd, float* running_mean, float* running_var, void* num_batches_tracked,
                   hipStream_t stream);
/* workspace sizes in floats (0 for an unsupported shape) */
size_t es_se_squeeze_workspace(int N, int HW, int C, int flags);
size_t es_se_bn_bwd_sums_workspace(int N, int HW, int C, int flags);
size_t es_se_gate_bwd_workspace(int N, int C, int R);
/* ybar[n][c] = mean_hw y (fp32 accumulation), a = gamma (ybar - mean) rstd + beta: one read of y */
int es_se_squeeze_ex(const void* y, int N, int HW, int C, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, float* ybar, float* a, float* workspace, int flags, hipStream_t stream);
int es_se_gate_fwd(const float* a, const float* w_down, const float* w_up, int N, int C, int R, float* h, float* s,
                   hipStream_t stream);
/* out = relu(s o + res) in es_bn2d_fwd_ex's affine form and rounding: with s == 1 bit-identical to
 * es_bn2d_fwd_ex(res, relu = 1) on the same mean / rstd */
int es_se_bn_apply_ex(const void* y, const void* res, const float* s, int N, int HW, int C, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, void* out, int flags,
                      hipStream_t stream);
/* g = dout [out > 0]; p1[n][c] = sum_hw g, p2[n][c] = sum_hw g xhat, xhat = (y - mean) rstd */
int es_se_bn_bwd_sums_ex(const void* y, const void* out, const void* dout, int N, int HW, int C, const float* mean,
                         const float* rstd, float* p1, float* p2, float* workspace, int flags, hipStream_t stream);
/* dt = (gamma p2 + beta p1) s (1 - s); dw_up = dt^T h; dh = (dt W_up) [h > 0]; dw_down = dh^T a; da = dh W_down;
 * dbeta = sum_n (s p1 + da); dgamma = sum_n (s p2 + da (ybar - mean) rstd): all overwritten */
int es_se_gate_bwd(const float* p1, const float* p2, const float* ybar, const float* a, const float* h,
                   const float* s, const float* w_down, const float* w_up, const float* gamma, const float* beta,
                   const float* mean, const float* rstd, int N, int C, int R, float* dw_down, float* dw_up, float* da,
                   float* dgamma, float* dbeta, float* workspace, hipStream_t stream);
/* d_o = g s + da / HW; train: dy = gamma rstd (d_o - dbeta / M - xhat dgamma / M), M = N HW; eval (train 0):
 * dy = gamma rstd d_o (dgamma / dbeta unused); gres (+)= g, the shortcut's gradient (accumulate: the second
 * consumer of a gradient sink) */
int es_se_bn_bwd_dx_ex(const void* y, const void* out, const void* dout, const float* s, const float* da, int N,
                       int HW, int C, const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                       const float* dbeta, int train, void* dy, void* gres, int accumulate, int flags,
                       hipStream_t stream);

/* ---- DenseNet: dense blocks in place over one NHWC buffer (csrc/densenet.hip) ---------------------------------
 * timm / torchvision `densenet161` (code/build.py:196-197,218-220; _DenseLayer: norm1 -> relu -> conv1 1x1 -> norm2
 * -> relu -> conv2 3x3, the output concatenated after the input; _Transition: norm -> relu -> conv 1x1 ->
 * AvgPool2d(2, 2)).  A block is one buffer [rows, ld]: layer i reads the channel prefix [0, C_i) and writes its
 * growth slice through the convs' strides, so torch.cat and every later BatchNorm's statistics pass over the same
 * channels disappear.  These replace aten cat / batch_norm / avg_pool2d around the convs above.
 *
 * Padded weight images: fp32 w [Cout][Cin][kh][kw] -> wp [Cout_p][kh kw][Cin_p], wt [Cin_p][kh kw][Cout_p] (bf16,
 * either nullable), es_conv2d_pack_bf16's mapping and rounding with zeros in the padding; Cout_p, Cin_p % 8 == 0.
 * _multi: n device-resident entries of es_conv_pack_pad_entry_size() bytes {const float* w; void* wp; void* wt;
 * int Cout, Cin, kh_x_kw, Cout_p, Cin_p, 0}, max_elems = the largest Cout_p Cin_p kh kw. */
int es_conv2d_pack_bf16_pad(const float* w, int Cout, int Cin, int kh, int kw, int Cout_p, int Cin_p, void* wp, void* wt,
                            hipStream_t stream);
int es_conv_pack_pad_entry_size(void);
int es_conv2d_pack_bf16_pad_multi(const void* table, int n, long max_elems, hipStream_t stream);
/* Padded weight gradients -> the true tensors: n device-resident entries of es_dw_unpad_entry_size() bytes
 * {const float* src; float* dst; int Cout_p, Cin_p, Cout, Cin, kh_x_kw, 0}; dst [Cout][Cin][kh kw] (overwritten) = the
 * true rows / columns of src [Cout_p][Cin_p][kh kw]; max_elems = the largest Cout Cin kh kw.  The entries are not
 * validated (the caller checks them); rows are copied 16 bytes at a time where src and dst are 16-byte aligned and
 * Cin kh kw % 4 == 0, element by element otherwise.  The _pad_multi pack likewise trusts its entries: wp / wt
 * 16-byte aligned, Cout_p, Cin_p % 8 == 0, as es_conv2d_pack_bf16_pad checks for one weight. */
int es_dw_unpad_entry_size(void);
int es_dw_unpad_multi(const void* table, int n, long max_elems, hipStream_t stream);
/* Batch statistics of the row-strided view x[r * ld + c] (r < rows, c < C <= ld): mean, rstd = 1 / sqrt(biased var +
 * eps), m2 = the centred square sum.  es_bn2d_fwd_ex's statistics passes: the same bits on a contiguous copy.
 * workspace: es_chan_workspace(rows, C) floats.  flags bit 0: x is bf16. */
int es_bn2d_stats_ld_ex(const void* x, int rows, int C, long ld, float eps, float* mean, float* rstd, float* m2,
                        float* workspace, int flags, hipStream_t stream);
/* The same arrays from a bf16 conv's bn_partials (es_conv2d_bnstats_size(rows, PC) floats; PC = the conv's output
 * channels, the first C taken): es_bn2d_fwd_partials_ex's combination bit for bit, no running-buffer update.  The
 * partials are overwritten. */
int es_bn2d_stats_from_partials(float* partials, int rows, int C, int PC, float eps, float* mean, float* rstd, float* m2,
                                hipStream_t stream);
/* Train-mode running-buffer update of n BatchNorms over one statistics array: n device-resident entries of
 * es_bn_running_entry_size() bytes {float* running_mean; float* running_var; int64* num_batches_tracked; int C;
 * int offset}, entry j reading mean / m2 [offset, offset + C).  Blend with momentum and the unbiased variance
 * m2 / (rows - 1), num_batches_tracked += 1: es_bn2d_fwd_ex's update.  max_c = the largest C. */
int es_bn_running_entry_size(void);
int es_bn2d_running_multi(const void* table, int n, int max_c, const float* mean, const float* m2, int rows,
                          float momentum, hipStream_t stream);
/* Eval mode: mean[c] = running_mean[c], rstd[c] = 1 / sqrt(running_var[c] + eps) for c < C, zeros over [C, Cp) */
int es_bn2d_eval_stats(const float* running_mean, const float* running_var, int C, int Cp, float eps, float* mean,
                       float* rstd, hipStream_t stream);
/* y[r * ldy + c] = bn(x[r * ldx + c]) (ReLU if relu) with the given mean / rstd: es_bn2d_fwd_ex's affine map and
 * rounding.  flags bit 0: x is bf16, bit 1: y is bf16. */
int es_bn2d_apply_ld_ex(const void* x, long ldx, int rows, int C, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int relu, void* y, long ldy, int flags,
                        hipStream_t stream);
/* es_bn2d_bwd_recompute_ex between row-strided views x[r * ldx + c], dy[r * ldy + c], dx[r * lddx + c], c < C (columns
 * beyond C untouched).  flags bit 0: x and dy are bf16; bit 1: dx is fp32 whatever the maps are; bit 2: dx
 * accumulates (in fp32).  The dense kernel's reduction order: on contiguous views the same dx / dgamma / dbeta bits.
 * workspace: es_chan_workspace(rows, C) floats. */
int es_bn2d_bwd_recompute_ld_ex(const void* x, long ldx, const void* dy, long ldy, int rows, int C, const float* gamma,
                                const float* beta, const float* mean, const float* rstd, void* dx, long lddx,
                                float* dgamma, float* dbeta, int accumulate, float* workspace, int flags,
                                hipStream_t stream);
/* AvgPool2d(2, 2) of the dense map x [N, H, W, C] into the row-strided view y[((n Ho + ho) Wo + wo) * ldy + c], and
 * its backward from a row-strided dy into the dense dx (overwritten).  es_avgpool2d_*_ex's values.  flags bit 0: the
 * input (x / dy) is bf16, bit 1: the output (y / dx) is bf16. */
int es_avgpool2_ld_fwd_ex(const void* x, int N, int H, int W, int C, void* y, long ldy, int flags, hipStream_t stream);
int es_avgpool2_ld_bwd_ex(const void* dy, long lddy, int N, int H, int W, int C, void* dx, int flags,
                          hipStream_t stream);

/* ---- optimizer / EMA (code/optimizer.py:50-51, code/ema.py:51-62) ----------------------------- */
int es_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2,
                     float eps, float neg_step, float bc2_sqrt, float decay, float one_minus_decay,
                     float grad_scale, hipStream_t stream);
/* AdamW and SGD (momentum, Nesterov) sweeps with per-param-group lr / weight decay (code/optimizer.py:43-49),
 * fused with the same EMA blend (ema nullable).  `cls` is the class map: one byte per 64 consecutive floats of
 * the flat buffer (n / 64 bytes; every parameter starts at a multiple of 64 floats), 0 = not trained (frozen
 * parameter or alignment padding: p, g and the moments are neither updated nor written, only the EMA blend
 * runs), 1 = param group 0, 2 = param group 1.  n % 64 == 0 and n < 2^38 (else ES_BAD_SHAPE); p, g, cls and the
 * moments non-null, every float buffer 16-byte aligned and cls 4-byte aligned (else ES_BAD_ARG).
 * AdamW: p *= decay_mul_c [= (float)(1 - lr_c wd_c)], then the Adam update with neg_step_c = -lr_c / (1 - beta1^t);
 * one_minus_beta{1,2} = (float)(1 - beta) rounded from double, as torch passes them (within 1e-6 of the fp32
 * 1 - beta, else ES_BAD_ARG).
 * SGD: d = g grad_scale + wd_c p; buf = buf momentum + d; p += neg_lr_c (nesterov ? d + momentum buf : buf). */
int es_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, const uint8_t* cls, long n,
                      float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                      float bc2_sqrt, float neg_step0, float neg_step1, float decay_mul0, float decay_mul1,
                      float decay, float one_minus_decay, float grad_scale, hipStream_t stream);
int es_sgd_ema_step(float* p, const float* g, float* buf, float* ema, const uint8_t* cls, long n, float momentum,
                    float neg_lr0, float neg_lr1, float wd0, float wd1, int nesterov, float decay,
                    float one_minus_decay, float grad_scale, hipStream_t stream);
int es_ema_entry_size(void);
int es_ema_update_multi(const void* entries, const void* chunks, int nchunks, float decay, float one_minus_decay,
                        hipStream_t stream);
int es_pack_entry_size(void);
int es_pack_weights(const float* flat, const void* entries, int nmat, hipStream_t stream);
int es_cast_f32_bf16(const float* x, void* y, long n, hipStream_t stream);

// y += x over n fp32 values (n % 4 == 0, 16-byte aligned).  Sums the second lane's flat gradient into the
// first (two-lane backward, endossl/vit.py Engine.backward); no reference counterpart (autograd accumulates).
int es_add_f32(float* y, const float* x, long n, hipStream_t stream);

/* ---- fp32 parity mode (csrc/parity.hip) --------------------------------------------------------
 * The same arguments as the bf16 entry points above, with fp32 storage wherever those read or write
 * bf16 (GEMM operands and epilogue outputs, qkv / attention output, LN output, patches, the packed
 * weight images).  endossl/vit.py's Engine(precision="fp32") runs its one forward / backward sequence
 * over these, so the 12-layer step is pinned to the fp32 oracle at 1e-3.  Same reference ops as the
 * bf16 forms (code/models/conformer.py:13-72, timm PatchEmbed); GEMMs on fp32 MFMA, no shape
 * restrictions beyond head dim 64 and T <= 1024 for attention, D % 64 == 0 for LayerNorm. */
int es_gemm_nt_f32(int epi, const void* A, int lda, const void* B, int ldb, const float* bias, void* C, int ldc,
                   void* C2, const void* aux, int ldaux, int M, int N, int K, int np, hipStream_t stream);
size_t es_gemm_tn_f32_workspace(int N1, int N2, int splits);
int es_gemm_tn_f32(const void* A1, int ld1, const void* A2, int ld2, int M, int N1, int N2, int splits,
                   float* workspace, float* out, int accumulate, float* bias_out, hipStream_t stream);
int es_attn_fwd_f32(const void* qkv, int ldqkv, void* o, int ldo, float* lse, int nimg, int T, int H, float scale,
                    hipStream_t stream);
int es_attn_bwd_f32(const void* qkv, int ldqkv, const void* o, int ldo, const float* lse, float* delta,
                    const void* dout, int lddo, void* dqkv, int lddqkv, int nimg, int T, int H, float scale,
                    hipStream_t stream);
int es_attn_cls_fwd_f32(const void* qkv, int ldqkv, void* o, int ldo, float* lse, int nimg, int T, int H, float scale,
                        hipStream_t stream);
int es_attn_cls_bwd_f32(const void* qkv, int ldqkv, const void* o, int ldo, const float* lse, const void* dout,
                        int lddo, void* dqkv, int lddqkv, int nimg, int T, int H, float scale, hipStream_t stream);
int es_layernorm_fwd_f32(const float* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, float* mean,
                         float* rstd, int M, int D, float eps, hipStream_t stream);
int es_layernorm_bwd_f32(const float* dy, int lddy, const float* x, int ldx, const float* mean, const float* rstd,
                         const float* gamma, const float* dres, int ldres, float* dx, int lddx, void* dxb, int lddxb,
                         float* dgamma, float* dbeta, float* workspace, int blocks, int M, int D, int accumulate,
                         hipStream_t stream);
int es_patch_im2col_f32(const float* img, void* patches, int n, int S, int P, hipStream_t stream);
int es_patch_im2col_u8_f32(const void* img, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                           void* patches, int n, int S, int P, hipStream_t stream);
int es_embed_bwd_f32(const float* dx, int lddx, void* dpatch, int ldp, float* dpos, float* dcls, int n, int T, int D,
                     int accumulate, hipStream_t stream);
int es_pack_weights_f32(const float* flat, const void* entries, int nmat, hipStream_t stream);
/* y = x, n fp32 values (the parity form of es_cast_f32_bf16) */
int es_copy_f32(const float* x, void* y, long n, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ENDOSSL_H */
