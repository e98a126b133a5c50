/* libhamer_hip: C ABI of the MI355X (gfx950) hand-mesh hot path.
 *
 * The reference (2646207530/hamer-yolo) has no FFI: its boundary is a set of Python call
 * signatures.  Each entry point below replaces the PyTorch/cv2/smplx
 * arithmetic behind one of those calls; the Python host layer (hamer_yolo_amd/) keeps the
 * reference's names and argument meaning and binds these symbols with ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - every pointer is DEVICE memory owned by the caller unless the name ends in _host;
 *    the library allocates nothing persistent and keeps no reference after return;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*), no internal sync;
 *  - return value: 0 on success, negative library code otherwise (HM_ERR_*); the message is
 *    available from hm_last_error_string() (thread-local); nothing throws across the ABI;
 *  - matrices are row-major; "ld*" are leading dimensions in ELEMENTS;
 *  - dtype selects the 16-bit GEMM operand type (bf16 or fp16, same MFMA rate).
 */
#ifndef HAMER_HIP_H
#define HAMER_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_VERSION 402   /* 402 also carries the additive SAR mesh-head entry points (hm_sar_saigb, hm_sar_graph_mix, hm_sar_linear, hm_sar_softargmax, hm_sar_postprocess) and the additive mesh overlay entry points (hm_mesh_overlay, hm_mesh_overlay_workspace_bytes: lib.load() checks them by export name, and the fp32 route's tests pin 402) and the additive fp32 RootNet / SAR entry points (hm_conv2d_f32_relu, hm_nchw3_to_nhwc8_f32, hm_gap_linear_f32, hm_sar_saigb_f32, hm_sar_graph_mix_f32, hm_sar_linear_f32) and the additive fp32 HaMeR entry points (hm_gemm_f32, hm_vit_attention_f32; hm_hamer_forward, hm_patch_im2col and hm_cross_attention take HM_DTYPE_F32) and the additive ConvNeXt SAR entry points (hm_dwconv7_ln, hm_ln_patchify2, hm_stem4_im2col, hm_sar_saigb_ch) and the additive attention test hook (hm_attention_grid, HM_OPT_ATT_GRID) and the additive hand-metric entry point (hm_pose_eval) and the additive depth-fit entry points (hm_depth_fit_workspace_bytes, hm_depth_fit: the existing tests pin 402) and the additive motion entry points (hm_track_smooth, hm_track_jitter: checked by export name) and the additive fp8 route query (hm_gemm_fp8_persistent: checked by export name); 402: HM_DTYPE_F32 (the fp32 YOLOv7 route: conv, maxpool, upsample, letterbox, hm_yolo_run); 401: hm_conv2d_stem_pair, HM_OP_CONV_PAIR, HM_OPT_CONV_STEM_PAIR; 400 = round 4: hm_option_count, hm_gemm_px_grid (302 = round 3: hm_set_option, hm_hamer_weights.tome_r) -- lib.load() checks it */

enum { HM_DTYPE_BF16 = 0, HM_DTYPE_F16 = 1,
       HM_DTYPE_F32 = 2 /* same value as HM_OUT_F32.  The fp32 YOLOv7 route (its section below) and the precise HaMeR route
                           (hm_hamer_forward, hm_gemm_f32, hm_patch_im2col, hm_cross_attention); every other entry point rejects it */ };

/* GEMM epilogues */
enum {
  HM_EPI_STORE = 0,     /* C(16-bit) = acc + bias                                  */
  HM_EPI_GELU = 1,      /* C(16-bit) = gelu_erf(acc + bias)        vit.py:82-87    */
  HM_EPI_RESID_F32 = 2, /* C(f32)    = acc + bias + resid[m % resid_mod][n]        */
  HM_EPI_F32 = 3,       /* C(f32)    = acc + bias                                  */
  HM_EPI_SILU = 4,      /* C(16-bit) = silu(acc + bias)      yolov7 common.py:114  */
  /* deferred LayerNorm (Block.forward vit.py:148-151: x += f(LN(x))): the GEMM that writes the residual
   * stream also emits the next LayerNorm's statistics and x*gamma, the GEMM that follows applies them:
   * LN(x).W^T + b = rstd * ((x*gamma).W^T - mean * colsum) + (b + W.beta), colsum[n] = sum_k W[n][k]*gamma[k] */
  HM_EPI_RESID_LN = 5,  /* RESID_F32, plus ln_xg = C*ln_gamma (16-bit) and ln_stats     */
  HM_EPI_LN_STORE = 6,  /* C(16-bit) = rstd*(acc - mean*ln_colsum) + bias               */
  HM_EPI_LN_GELU = 7,   /* C(16-bit) = gelu_erf(rstd*(acc - mean*ln_colsum) + bias)     */
  HM_EPI_GELU_MX8 = 8,  /* hm_gemm_fp8 only: C = MXFP8(gelu_erf(acc + bias)): e4m3 bytes + E8M0 scale per 32 columns */
  HM_EPI_RELU = 9,      /* hm_conv2d_nhwc only: C(16-bit) = relu(acc + bias)                 torchvision BasicBlock     */
  HM_EPI_ADD_RELU = 10  /* hm_conv2d_nhwc only: C(16-bit) = relu(acc + bias + resid16[m][n]) (out += identity; relu)    */
};

typedef struct hm_gemm_args {
  const void* X;      /* [M][ldx] 16-bit activations                                  */
  const void* W;      /* [N][ldw] 16-bit weights (nn.Linear layout)                   */
  void* C;            /* [M][ldc] 16-bit or f32 by epilogue                           */
  const float* bias;  /* [N] or NULL                                                  */
  const float* resid; /* [resid_mod or M][ldr] f32, HM_EPI_RESID_F32 only (may alias C) */
  int M, N, K;
  int ldx, ldw, ldc, ldr;
  int resid_mod;      /* >0: residual row = m % resid_mod (positional embedding)      */
  int epilogue;
  int dtype;
  /* deferred LayerNorm, NULL / 0 for the other epilogues */
  const float* ln_gamma;  /* RESID_LN: [N] gamma of the LayerNorm that reads C                            */
  void* ln_xg;            /* RESID_LN: out [M][N] 16-bit, C * gamma (the consuming GEMM's X)              */
  float* ln_stats;        /* RESID_LN: out [N/64][M][2] = (sum, sum of squares) of C per 64 columns;
                             LN_*: in [M][2] = (mean, rstd) per row, made from those by hm_ln_finalize     */
  const float* ln_colsum; /* LN_*: [N] sum_k W[n][k] * gamma[k] over the 16-bit W; bias = b + W.beta      */
  /* split-K (HM_EPI_F32, bias == NULL): K is cut into k_split ranges computed by separate workgroups; range s
   * writes its partial product to C + s*M*ldc.  For small M (few output tiles, long K); the consumer adds the
   * slabs in order (hm_layernorm_accum), so the result is deterministic.  0 or 1: off. */
  int k_split;
  /* HM_EPI_GELU only: C = gelu_erf(acc + bias) * out_scale, a power of two chosen at load so that the 16-bit activation stays
   * finite (the consumer's weights carry 1 / out_scale; HamerEngine prescale).  0 or 1: off. */
  float out_scale;
} hm_gemm_args;

/* nn.Linear forward on MFMA: C = epilogue(X . W^T).  Replaces the aten::addmm calls behind
 * Attention.qkv/.proj (vit.py:114,:124), Mlp.fc1/.fc2 (vit.py:83,:85), PatchEmbed.proj
 * (vit.py:172, after hm_patch_im2col) and CrossAttention.to_kv (pose_transformer.py:114). */
int hm_gemm(const hm_gemm_args* args, void* stream);
/* HM_EPI_RESID_LN partials [D/64][M][2] -> row_stats [M][2] = (mean, 1/sqrt(var + eps)) for HM_EPI_LN_*. */
int hm_ln_finalize(const float* partials, float* row_stats, int M, int D, float eps, void* stream);
/* Tuning hook: pin the GEMM tile configuration (see launch_gemm in gemm.hip: 0 = 128x128, 10 = 256x256 two-stage,
 * 24 = 256x256 with X two K-steps ahead, 26 = persistent; any other id is refused); -1 restores the default
 * (also settable through the HM_GEMM_VARIANT environment variable).  Results do not depend on it
 * beyond fp32 summation order. */
int hm_gemm_set_variant(int variant);
/* Tuning hook: M-tiles per group in the XCD-aware tile walk (default 8). */
int hm_gemm_set_group_m(int group_m);
/* Process-wide test / tuning switches.  Launch paths read these, never the environment (HM_GEMM_VARIANT and HM_PX_GRID are
 * read ONCE, on first use, as start-up defaults for tuning runs).  Returns 0, or HM_ERR_ARG for an unknown key / bad value. */
enum {
  HM_OPT_PX_GRID = 0,               /* workgroups of the persistent 16-bit GEMM (0 = one per CU)                        */
  HM_OPT_FP8P_GRID = 1,             /* workgroups of the persistent fp8 GEMM (0 = one per CU; tests: few, many tiles each) */
  HM_OPT_FP8_ONE_TILE = 2,          /* 1: hm_gemm_fp8 always takes the one-tile kernel (tests compare the two)           */
  HM_OPT_FP8P_RESID = 3,            /* 1: persistent fp32-residual fp8 epilogue (bit-identical, measured not faster)     */
  HM_OPT_TOME_NO_SPLITK = 4,        /* 1: token-merging forward never splits proj / fc2 over K (tests compare the routes) */
  HM_OPT_TOME_SCALAR_ATTENTION = 5, /* 1: hm_tome_attention takes the fp32 lane-per-key kernel                           */
  HM_OPT_RESID_IN_EPILOGUE = 6,     /* 1: the fp32-residual GEMM fetches its residual rows in the epilogue (round-2 form) */
  HM_OPT_CONV_TILE = 7,             /* tuning: force convolution tile (1..9 = 128x128, 128x64, 128x32, 256x128, 256x256, 256x64, then the deep-ring 128x32, 128x64, 128x128; 10..15 = the two-K-group tiles; 16 = the persistent 256x256 GEMM kernel for the 1x1 layers it applies to); 0 = per-layer choice */
  HM_OPT_CONV_SPLITK = 8,           /* tuning: 1 = never split a convolution over K, n > 1 = ask for n ranges where splitting applies; 0 = automatic */
  HM_OPT_PX_LDS_EPILOGUE = 9,       /* persistent GEMM epilogue: 0 = per epilogue (GELU: lane swaps, store: through LDS), 1 = always LDS, 2 = always lane swaps */
  HM_OPT_CONV_DIRECT = 10,          /* direct kernels (3x3: 3(8) -> 32 stem, 64 -> 64 stride 1, 32 -> 64 stride 2; 1x1 with K, Cout in {128, 256}): 0 = all, each from its own tile count up, 1 = none (implicit GEMM everywhere), 2 = stem only, 3 = all at any size */
  HM_OPT_GEMM_TILE_RULE = 11,       /* tuning: 1 = round 2's GEMM tile rule (256 x 256 only from 85 % full rounds), 0 = the rate model */
  HM_OPT_CONV_KGROUPS = 12,         /* tuning: 1 = no K groups inside a convolution workgroup (small maps), 0 = automatic */
  HM_OPT_CONV_GENERAL_LOADER = 13,  /* tuning / tests: 1 = the implicit-GEMM convolution takes its general loader (per-lane tap arithmetic every K-step) even where the lean one applies (Cin % 64 == 0); 0 = automatic.  Same bytes either way */
  HM_OPT_CONV_STEM_PAIR = 14,       /* tuning / tests: 1 = hm_conv2d_stem_pair (and HM_OP_CONV_PAIR of hm_yolo_run) always runs its two convolutions as two launches; 0 = one launch where the fused kernel applies.  Same bytes either way */
  HM_OPT_ATT_GRID = 15,             /* tests: the number of compute units the persistent attention launches (hm_vit_attention, hm_vit_attention_mx8, the MFMA path of hm_tome_attention) plan for; 0 = the device's count.  Any value >= 1 (a grid that is no multiple of the 8 XCDs is wanted here): few units make every workgroup walk several (crop, head) items.  Same bytes at every value */
  HM_OPT_GEMM_STAGGER = 16,         /* 256x256 GEMM K loops (persistent 16-bit store kernel, in-loop fp32-residual kernel): 0 = each kernel's default, 1 = lockstep (all eight waves in one phase), 2 = staggered wherever the shape allows (waves 4-7 one sub-step behind waves 0-3); tuning: 3 = persistent kernel only, 4 = residual kernel only; hm_set_option refuses any other value.  Same bytes at every value */
  HM_OPT_COUNT = 17
};
int hm_set_option(int key, int value);
int hm_get_option(int key);
/* HM_OPT_COUNT of the library as built: a binding checks its own key table against it (hamer_yolo_amd/lib.py load()). */
int hm_option_count(void);
/* Host-side query, no device work: the workgroup count the persistent 16-bit GEMM takes for `tiles` whole 256 x 256 tiles on a
 * chip of `cus` compute units (0: 256) under the current HM_OPT_PX_GRID -- tests check that the option is not sticky. */
int hm_gemm_px_grid(int tiles, int cus);
/* Host-side query, no device work: the workgroup count the persistent attention kernel takes for `items` (crop, head) pairs
 * under the current HM_OPT_ATT_GRID; `cus` compute units (0: 256) apply when the option is 0.  Every workgroup then walks at most
 * ceil(items / grid) items.  The launches call the same function, so a test that asserts its geometry cannot disagree with them. */
int hm_attention_grid(int items, int cus);

/* The fp8 flavour of hm_gemm for BASELINE configs[4] ("fp8 ViT-H weights on CDNA4 fp8 MFMA"): C = epilogue(X . W^T) on
 * v_mfma_scale_f32_16x16x128_f8f6f4 (2x the bf16 MFMA rate, half the operand bytes).
 *   X : MXFP8 -- e4m3 (OCP) bytes [M][ldx] plus one E8M0 scale per row and 32 K-elements, stored [K/32][M]
 *       (written by hm_layernorm_mx8 and by the HM_EPI_GELU_MX8 epilogue);
 *   W : e4m3 bytes [N][ldw] with one f32 scale per output channel (w_scale[n] = max|W[n]| / 448);
 *   epilogues HM_EPI_STORE (16-bit C, out_dtype), HM_EPI_RESID_F32, HM_EPI_GELU_MX8 (C bytes [M][ldc], out_scales [N/32][M]).
 * M % 16 == 0, N % 64 == 0, K % 128 == 0. */
typedef struct hm_gemm_fp8_args {
  const void* X8; const void* x_scales;
  const void* W8; const float* w_scale;
  void* C; const float* bias; const float* resid; void* out_scales;
  int M, N, K, ldx, ldw, ldc, ldr;
  int epilogue;
  int out_dtype;      /* HM_EPI_STORE: HM_DTYPE_BF16 or HM_DTYPE_F16 */
} hm_gemm_fp8_args;
int hm_gemm_fp8(const hm_gemm_fp8_args* args, void* stream);
/* Host-side query, no device work: 1 when hm_gemm_fp8 runs `args` on the persistent kernel (whole 256 x 256 tiles, at least 8,
 * K >= 256, a bias, the leading dimensions it needs, under the current HM_OPT_FP8_ONE_TILE / HM_OPT_FP8P_RESID), 0 when on the
 * one-tile kernel, -1 when hm_gemm_fp8 would refuse them (hm_last_error_string says why).  hm_gemm_fp8 dispatches on the same
 * function, so a test that asserts the route cannot disagree with the launch. */
int hm_gemm_fp8_persistent(const hm_gemm_fp8_args* args);
/* nn.LayerNorm with MXFP8 output (the X operand of hm_gemm_fp8): out8 [M][D] e4m3, out_scales [D/32][M] E8M0.  D % 32 == 0. */
int hm_layernorm_mx8(const float* x, const float* gamma, const float* beta, void* out8, void* out_scales, int M, int D,
                     float eps, void* stream);

/* nn.LayerNorm over the last dim (vit.py:136,:144,:252 eps 1e-6; t_cond_mlp.py:51-52 eps 1e-5).
 * x [M][D] f32 -> out [M][D]; out_dtype: HM_DTYPE_BF16 / HM_DTYPE_F16 / HM_OUT_F32. */
#define HM_OUT_F32 2
int hm_layernorm(const float* x, const float* gamma, const float* beta, void* out, int out_dtype,
                 int M, int D, float eps, void* stream);
/* The residual add in front of a LayerNorm (Block.forward vit.py:148-151) for a split-K producer:
 * x[m] += bias + sum_s partials[s][m] (s ascending; partials [n_partials][M][D] f32 from hm_gemm k_split), then
 * out = LayerNorm(x) as hm_layernorm.  x is updated in place. */
int hm_layernorm_accum(float* x, const float* partials, int n_partials, const float* bias, const float* gamma,
                       const float* beta, void* out, int out_dtype, int M, int D, float eps, void* stream);
/* max |x[m][col0 + c]| over m < M, c < ncols of a 16-bit matrix with row pitch ld, folded into *slot (device, >= 0 on entry)
 * with an atomic max: the range probe of hm_hamer_weights.range_stats. */
int hm_absmax16(const void* x, int ld, int M, int col0, int ncols, int dtype, float* slot, void* stream);

/* Attention.forward core (vit.py:115-123): softmax(scale q k^T) v for `tokens`=192 keys.
 * qkv [B*tokens][3*heads*head_dim] 16-bit, column = which*H*d + head*d + i (reshape at
 * vit.py:112); out [B*tokens][heads*head_dim] 16-bit (head-major, vit.py:123).
 * One persistent kernel: hm_attention_grid(B*heads, CUs) workgroups walk the (crop, head) items; a (crop, head)'s bytes do not
 * depend on the grid (HM_OPT_ATT_GRID, a test hook, makes a workgroup walk several items at any B). */
int hm_vit_attention(const void* qkv, void* out, int B, int tokens, int heads, int head_dim, float scale,
                     int dtype, void* stream);

/* Token merging (selective_vit_adapter.py).  hm_tome_attention: ToMeAttention.forward core (:166-195) for any
 * tokens <= 192 -- softmax(scale q k^T + log(size)) v, `size` [B*tokens] f32 or NULL (no merge yet).
 * hm_tome_merge: the matching metric (head-averaged keys, :198), bipartite_soft_matching (:17-66: alternate tokens form
 * the sets A / B, every A token proposes its most similar B token, the r best proposals merge) and merge_wavg (:98-113)
 * in one call: x [B*tokens][D] f32 -> x_out [B*(tokens-r)][D], size_out [B*(tokens-r)] ([unmerged A tokens in proposal
 * order | B tokens]).  metric_ws: B*tokens*80 floats, index_ws: hm_tome_index_bytes(B). */
size_t hm_tome_index_bytes(int B);
int hm_tome_attention(const void* qkv, const float* size, void* out, int B, int tokens, int heads, int head_dim, float scale,
                      int dtype, void* stream);
int hm_tome_merge(const void* qkv, const float* x, const float* size, float* x_out, float* size_out, float* metric_ws,
                  int* index_ws, int B, int tokens, int r, int heads, int head_dim, int D, int dtype, void* stream);
/* hm_tome_merge with a caller-supplied fp32 metric: metric[(b*tokens + t) * ld_metric + d] (+ the same at column lo_off + d when
 * lo_off > 0: a hi / lo pair), d < 80. */
int hm_tome_merge_metric(const float* metric, int ld_metric, int lo_off, const float* x, const float* size, float* x_out,
                         float* size_out, int* index_ws, int B, int tokens, int r, int D, void* stream);

/* Same attention with MXFP8 output for an fp8 proj GEMM (bf16 qkv in).  Heads are widened from 80 to 96 columns so that
 * scale blocks of 32 never straddle two heads: out8 [B*tokens][heads*96] e4m3 bytes (columns 80..95 of every head zero),
 * out_scales [heads*3][B*tokens] E8M0.  The proj weight must use the same K order (hm_vit_block.proj_w8). */
int hm_vit_attention_mx8(const void* qkv, void* out8, void* out_scales, int B, int tokens, int heads, int head_dim, float scale,
                         void* stream);

/* PatchEmbed.proj im2col (vit.py:168-176, called on x[:, :, :, 32:-32] at hamer.py:119):
 * img [B][3][img_h][img_w_full] f32, window columns [x0, x0+win_w), conv k=patch, s=patch,
 * zero pad `pad` -> patches [B*gh*gw][3*patch*patch] 16-bit, K order (c, ky, kx). */
int hm_patch_im2col(const float* img, void* patches, int B, int img_h, int img_w_full, int x0, int win_w,
                    int patch, int pad, int dtype, void* stream);   /* HM_DTYPE_F32: fp32 patches (32-byte aligned) */

/* Small f32 nn.Linear on f32-input MFMA: out[M][N] = act(x[M][K] . W[N][K]^T + bias) (+ resid).
 * act: 0 none, 1 gelu_erf.  Decoder layers (pose_transformer.py:40-124) and the read-out
 * heads (mano_head.py:93-95).  K % 16 == 0. */
int hm_linear_f32(const float* x, int ldx, const float* W, int ldw, const float* bias, const float* resid, int ldr,
                  float* out, int ldo, int M, int N, int K, int act, void* stream);


/* out[b][:] = vec[:] for b < B (the zero-token embedding, pose_transformer.py:350-354). */
int hm_broadcast_rows(const float* vec, float* out, int B, int D, void* stream);

/* CrossAttention core for one query token (pose_transformer.py:117-123):
 * q [B][heads*dim_head] f32; k,v rows b*tokens+t of kv (16-bit, ld = ldkv), k at column
 * k_off + h*dim_head, v at v_off + h*dim_head; out [B][heads*dim_head] f32.  dim_head == 64. */
int hm_cross_attention(const float* q, const void* kv, int ldkv, int k_off, int v_off, float* out, int B, int tokens,
                       int heads, int dim_head, float scale, int dtype, void* stream);
/* HM_DTYPE_F32: kv holds fp32 (32-byte aligned) and the softmax takes the accurate expf: the precise route. */

/* MANO-shaped model parameters (smplx.MANOLayer buffers; mano_wrapper.py:12-30). */
typedef struct hm_mano_model {
  const float* v_template;  /* [V][3]                */
  const float* shapedirs;   /* [V][3][10]            */
  const float* posedirs;    /* [135][3V]             */
  const float* J_regressor; /* [16][V]               */
  const float* lbs_weights; /* [V][16]               */
  int n_verts;              /* V = 778               */
} hm_mano_model;

/* rot6d_to_rotmat (geometry.py:47-70) + MANO.forward (mano_wrapper.py:32-44 -> smplx lbs) +
 * cam_t and perspective_projection (hamer.py:131-154), one workgroup per hand.
 * pose6d [B][96], betas [B][10], cam [B][3] ->
 * rotmats [B][16][3][3], verts [B][V][3], joints [B][21][3], cam_t [B][3], kp2d [B][21][2]. */
int hm_mano_forward(const hm_mano_model* model, const float* pose6d, const float* betas, const float* cam,
                    float* rotmats, float* verts, float* joints, float* cam_t, float* kp2d, int B,
                    float focal_length, float image_size, void* stream);

/* Batched affine bilinear crop (prepare_batch_bbox, infer.py:154-259; generate_image_patch_cv2,
 * datasets/utils.py:318-376).  The per-box map is cv2.warpAffine's inverted matrix in its
 * fixed-point form (source x = (x0 + rint(m0 * dst_x * 1024)) / 1024, 1/32-px bilinear). */
typedef struct hm_crop_box {
  double m0, m4;    /* d src_x / d dst_x, d src_y / d dst_y                         */
  int32_t x0, y0;   /* rint(offset * 1024) + 16                                      */
  int32_t flip;     /* 1: left hand, patch mirrored after the crop (infer.py:229-230) */
  int32_t reserved;
} hm_crop_box;

/* HOST helper (no GPU work): box centre (cx, cy) and square side `size` in frame pixels ->
 * hm_crop_box for a P x P patch (gen_trans_from_patch_cv, datasets/utils.py:82-129, rot 0). */
int hm_crop_box_from_bbox(double cx, double cy, double size, int flip, int P, hm_crop_box* out);

/* frame [H][W][3] u8 BGR (device); boxes [B] (device); out [B][3][P][P] f32 RGB,
 * (x - mean_c) / std_c with mean/std in 0..255 units (infer.py:145-146,:235-238). */
int hm_crop_batch(const uint8_t* frame, int H, int W, const hm_crop_box* boxes, float* out, int B, int P,
                  const float* mean3_host, const float* std3_host, void* stream);

/* The same crop with the anti-alias prefilter of prepare_item (infer.py:263-352): with df = (size / P) / 2 > 1.1 the frame
 * is blurred by skimage.filters.gaussian(sigma = (df - 1) / 2, preserve_range) before it is sampled.  Per axis the blur is
 * radius = int(4 sigma + 0.5) normalised taps exp(-k^2 / (2 sigma^2)) over replicated frame edges; the float image is then
 * sampled at the SAME 1/32-px coordinates as the 8-bit crop with the weights (32-fx)(32-fy)/1024 ..., a tap outside the
 * frame counting 0, and nothing is rounded to 8 bits.  df <= 1.1: the 8-bit rule of hm_crop_batch, same bytes. */
#define HM_CROP_AA_MAX_SIGMA 12.0       /* a box inside a 3840 x 2160 frame at P = 256: size 12800 */
#define HM_CROP_AA_MAX_RADIUS 48        /* int(4 * 12 + 0.5) */
#define HM_CROP_AA_TAPS (HM_CROP_AA_MAX_RADIUS + 1)
typedef struct hm_crop_aa_box {
  double m0, m4;    /* the hm_crop_box fields, same arithmetic                       */
  int32_t x0, y0;
  int32_t flip;
  int32_t reserved;
  float sigma;      /* 0: df <= 1.1, the 8-bit rule (radius is 0 then)               */
  int32_t radius;   /* 0 .. HM_CROP_AA_MAX_RADIUS; 0 with sigma > 0: float rule, no blur */
  int32_t pad[2];
} hm_crop_aa_box;

/* HOST helper (no GPU work): hm_crop_box_from_bbox plus sigma, radius and the one-sided taps g[0 .. radius] (computed in
 * double, stored as float; taps_out[radius + 1 .. 48] = 0; all 0 but g[0] = 1 on the 8-bit rule).  A size whose sigma
 * exceeds HM_CROP_AA_MAX_SIGMA (so every radius above HM_CROP_AA_MAX_RADIUS) is HM_ERR_ARG, the message naming the size --
 * it is not clamped. */
int hm_crop_aa_box_from_bbox(double cx, double cy, double size, int flip, int P, hm_crop_aa_box* out, float* taps_out);

/* hm_crop_batch over hm_crop_aa_box records: boxes [B] and taps [B][HM_CROP_AA_TAPS] on the device, as the helper wrote
 * them.  One launch for all hands of the frame; no blurred frame and no per-hand copy exists in memory: every workgroup
 * filters the source rows and columns of its own output row.  fp32 arithmetic; a hand's bytes do not depend on B or on its
 * position.  A record whose radius is outside 0 .. HM_CROP_AA_MAX_RADIUS (not one the helper wrote) gets NaN pixels. */
int hm_crop_batch_aa(const uint8_t* frame, int H, int W, const hm_crop_aa_box* boxes, const float* taps, float* out, int B,
                     int P, const float* mean3_host, const float* std3_host, void* stream);

/* Whole HAMER.forward_step (hamer.py:99-156) as one enqueue: see hm_hamer_forward below. */
typedef struct hm_vit_block {
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w;       /* 16-bit [N][K]                 */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  /* optional (all four, in every block, or none): deferred-LayerNorm operands, see HM_EPI_RESID_LN.
   * *_colsum[n] = sum_k W[n][k]*ln_g[k] over the 16-bit weights, *_bias_ln = b + W.ln_b.  When present
   * hm_hamer_forward runs no LayerNorm kernel inside the blocks. */
  const float *qkv_colsum, *qkv_bias_ln, *fc1_colsum, *fc1_bias_ln;
  /* optional (all six, in every block, or none; dtype must be HM_DTYPE_BF16): the fp8 path of BASELINE configs[4].
   * e4m3 bytes [N][K] and one f32 scale per output channel for qkv / fc1 / fc2; hm_hamer_forward then runs those three
   * GEMMs through hm_gemm_fp8 with MXFP8 activations (hm_layernorm_mx8, HM_EPI_GELU_MX8); proj stays 16-bit. */
  const void *qkv_w8, *fc1_w8, *fc2_w8;
  const float *qkv_ws, *fc1_ws, *fc2_ws;
  /* optional on top of those: proj in fp8 as well.  proj_w8 is [D][heads*96] e4m3, column h*96 + d = proj.weight[:, h*80 + d]
   * for d < 80 and zero for d >= 80 (the K order of hm_vit_attention_mx8), proj_ws its per-output-channel scale. */
  const void* proj_w8;
  const float* proj_ws;
  /* optional, token merging only (round 3): the matching metric k.mean(heads) = LN1(x) . Wbar^T + bbar with
   * Wbar = mean over heads of the key rows of qkv.weight (the metric is linear in the keys, selective_vit_adapter.py:198), so
   * hm_hamer_forward forms it entirely in fp32 -- an fp32 LayerNorm output and hm_linear_f32 -- instead of averaging 16-bit
   * keys: merge decisions then follow the fp32 reference up to what the residual stream itself differs by.
   * kmean_w: f32 [80][embed_dim]; kmean_b: f32 [80]. */
  const float* kmean_w;
  const float* kmean_b;
  /* range prescale (round 4; 0 = 1): powers of two folded into the weights at load so that every 16-bit activation of the
   * block stays inside fp16 on checkpoints whose activations overflow it.  attn_scale_mul multiplies the softmax scale (q and k
   * rows were scaled down by 2^-aq, 2^-ak: attn_scale_mul = 2^(aq+ak)); gelu_out_scale is hm_gemm's out_scale for fc1
   * (fc2.weight carries its inverse).  Everything else (LayerNorm gamma / beta against the next weight's columns, v rows
   * against proj) is weight folding only. */
  float attn_scale_mul, gelu_out_scale;
} hm_vit_block;

typedef struct hm_dec_layer {
  const float *ln0_g, *ln0_b, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const float* sa_v_w;    /* rows [2*inner, 3*inner) of to_qkv.weight: [inner][dim]  */
  const float* sa_w;      /* optional: to_out.weight . sa_v_w, [dim][dim] -- self-attention over one token is linear
                             (softmax == 1), so the two projections fold into one                                    */
  const float *sa_out_w, *sa_out_b;
  const float* ca_q_w;
  const float *ca_out_w, *ca_out_b;
  const float *ff1_w, *ff1_b, *ff2_w, *ff2_b;
  float ca_scale_mul;     /* range prescale (0 = 1): this layer's key rows of kv_w were scaled by 2^-a, the cross-attention scale takes 2^a */
} hm_dec_layer;

typedef struct hm_hamer_weights {
  /* ViT (backbones/vit.py) */
  int img_h, img_w_full, win_x0, win_w, patch, pad, embed_dim, depth, heads, mlp_dim;
  float vit_eps;
  const void* patch_w;       /* 16-bit [D][3*p*p]                                    */
  const float* patch_b;
  const float* pos;          /* f32 [tokens][D] = pos_embed[1:] + pos_embed[0]       */
  const hm_vit_block* blocks; /* host array of `depth` entries                        */
  const float *last_g, *last_b;
  /* decoder (components/pose_transformer.py, heads/mano_head.py) */
  int dec_dim, dec_depth, dec_heads, dec_dim_head, dec_mlp;
  float dec_eps;
  const float* token0;       /* f32 [dec_dim] = to_token_embedding.bias + pos_embedding */
  const void* kv_w;          /* 16-bit [dec_depth*2*inner][embed_dim], layers stacked  */
  const hm_dec_layer* layers; /* host array of `dec_depth` entries                     */
  const float* head_w;       /* f32 [112][dec_dim]: decpose(96) | decshape(10) | deccam(3) | 3 zero rows */
  const float* head_b;       /* f32 [112]: bias + init_{hand_pose,betas,cam}            */
  hm_mano_model mano;
  float focal_length, image_size;
  int dtype;
  /* token merging (HAMER_INFER(token_merge=True), hamer.py:481-483): host array of `depth` ints, the tokens to merge away
   * after the attention of each block (parse_r of selective_vit_adapter.py:132-157), or NULL for the dense backbone */
  const int* tome_r;
  /* calibration (load time only): device array of 6 * depth + 1 + 2 * dec_depth floats, zeroed by the caller, or NULL.  When
   * set (dense 16-bit path only), the forward also records the largest magnitude of every 16-bit activation class:
   * per block [LN1 out, q, k, v, LN2 out, GELU out], then last_norm out, then per decoder layer [k, v] of the to_kv output. */
  float* range_stats;
} hm_hamer_weights;

typedef struct hm_hamer_outputs {
  float* pose6d;   /* [B][96]  */
  float* betas;    /* [B][10]  */
  float* cam;      /* [B][3]   */
  float* rotmats;  /* [B][16][3][3]: [:,0] = global_orient, [:,1:] = hand_pose */
  float* verts;    /* [B][V][3]  */
  float* joints;   /* [B][21][3] */
  float* cam_t;    /* [B][3]     */
  float* kp2d;     /* [B][21][2] */
  void* tokens;    /* optional [B*tokens][D] 16-bit copy of the backbone output (fp32 with HM_DTYPE_F32), or NULL */
} hm_hamer_outputs;

/* Bytes of workspace hm_hamer_forward needs for a batch of B crops. */
size_t hm_hamer_workspace_bytes(const hm_hamer_weights* w, int B);

/* img [B][3][img_h][img_w_full] f32 normalised crops -> outputs.  Enqueues ~300 kernels.
 *
 * hm_hamer_weights.dtype == HM_DTYPE_F32 is the precise route (HAMER(..., dtype=torch.float32); the reference's fp32 CPU
 * arithmetic, hamer.py:99-156 with an fp32 model): every `const void*` weight is fp32, hm_hamer_outputs.tokens (when asked
 * for) is fp32, the workspace holds fp32 activations (hm_hamer_workspace_bytes sizes it).  tome_r, range_stats, the fp8
 * pointers, *_colsum / *_bias_ln, kmean_* must be NULL and the prescale factors 0 or 1, else HM_ERR_ARG.  The backbone runs
 * hm_layernorm (fp32 out), hm_gemm_f32 and hm_vit_attention_f32; every output is bias + one sum over K in a fixed order with
 * the residual added behind it, at every B -- a hand's outputs are the same bytes alone, in any batch, at any position. */
int hm_hamer_forward(const hm_hamer_weights* w, const float* img, int B, const hm_hamer_outputs* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- YOLOv7 detector path
 * Activations are NHWC 16-bit tensors addressed as (base pointer, pixel stride in elements): a
 * producer can write straight into a channel slice of a concat buffer (Concat, common.py:60-66,
 * costs nothing), a consumer can read a slice the same way.
 *
 * HM_DTYPE_F32 (round 5): the reference's CPU branch (detector.py:110-112 with half = False) -- activations, the image and the
 * weights in fp32.  Taken by hm_conv2d_nhwc (act 0 or 1, no resid), hm_maxpool_nhwc, hm_upsample2x_nhwc, hm_letterbox,
 * hm_letterbox_batch (x8 in fp32: 8 channels, 3 real, u / 255 correctly rounded as torch divides) and the conv / maxpool /
 * upsample ops of hm_yolo_run; the strides (ldx, ldy, ldr) stay in elements.  Every other entry point, hm_conv2d_stem_pair
 * (HM_OP_CONV_PAIR) among them, rejects it with HM_ERR_ARG.  The convolution (conv_f32.hip) runs on the fp32-input MFMA: each
 * output is bias + a sum over K in one order fixed by k*k*Cin alone -- no split-K (hm_conv_splitk_bytes returns 0, splitk_ws is
 * ignored), no K groups, none of the HM_OPT_CONV_* tuning options -- so results are deterministic and batch-invariant, and a
 * convolution is within ~1e-6 * sum|x * w| of exact (the fp32 MFMA is a k-ordered fmaf chain); pooling, upsampling and the
 * letterbox are exact. */
typedef struct hm_conv_args {
  const void* X;      /* [N][H][W_in][ldx] 16-bit (fp32 with HM_DTYPE_F32), pointer already offset to the first input channel */
  const void* W;      /* [Cout][Kpad] 16-bit (fp32 with HM_DTYPE_F32), K order (ky, kx, ci), zero padded to Kpad (% 64 == 0) */
  void* Y;            /* [N][Hout][Wout][ldy] 16-bit (or f32 when out_f32 or HM_DTYPE_F32), offset to the channel slice */
  const float* bias;  /* [Cout]                                                                        */
  const void* zeros;  /* >= 16 zero bytes on the device: source of padding taps                        */
  int N, H, W_in, Cin, Cout, ksize, stride, ldx, ldy, Kpad;
  int act;            /* 1: SiLU (Conv.fuseforward, common.py:114); 2: ReLU (ResNet-34 of the RootNet backbone) */
  int out_f32;        /* 1: f32 output, no activation (detect head, yolo.py:151)                       */
  int dtype;
  const void* resid;  /* optional with act == 2: [N][Hout][Wout][ldr] 16-bit added before the ReLU (BasicBlock identity) */
  int ldr;
  /* round 3, optional: scratch for split-K (few output tiles, long K: the 12x20 / 24x40 maps of the YOLOv7 neck).  When given
   * (16-byte aligned, at least hm_conv_splitk_bytes(args) bytes), the library cuts K into 2 or 4 ranges by a rule that looks at
   * ONE image's output only (so a frame's result does not depend on the batch it rides in), writes fp32 partial slabs
   * [ranges][N*Hout*Wout][Cout] here and adds them, in order, in a second small kernel. */
  void* splitk_ws;
  size_t splitk_ws_bytes;
} hm_conv_args;

/* Conv2d(k in {1,3,5,7}, stride in {1,2}, pad k/2) + bias (+ SiLU / ReLU / residual add + ReLU) as an implicit GEMM on MFMA.
 * Cin must be a power of two >= 8 (the 3-channel image is stored with 8 channels).
 * HM_DTYPE_F32: act 0 or 1, no resid; X / W 16-byte aligned, ldx % 4 == 0; zeros and splitk_ws are not used; the HM_OPT_CONV_*
 * options do not apply (one kernel, its tile chosen by Cout and the tile count, with no effect on the result). */
int hm_conv2d_nhwc(const hm_conv_args* args, void* stream);
/* bytes of splitk_ws this convolution would use (0: it is never split -- always for HM_DTYPE_F32) */
size_t hm_conv_splitk_bytes(const hm_conv_args* args);
/* Two consecutive convolutions of which the second is the ONLY reader of the first's output: Conv 0 and Conv 1 of yolov7.yaml
 * (yolo.py Model.forward_once walks them one after the other; 3 -> 32, k3 s1, then 32 -> 64, k3 s2, both SiLU).  Where the fused
 * kernel applies (first: Cin 8 (3 real), ldx 8, Cout 32, k3 s1, SiLU; second: X == first.Y, ldx == first.ldy == 32, Cout 64, k3 s2,
 * SiLU, ldy % 8 == 0, Y 16-byte aligned; one dtype) both run as ONE launch and first->Y is NOT written (the intermediate stays in
 * LDS; the result is bit-identical to the two launches); anywhere else, or with HM_OPT_CONV_STEM_PAIR = 1, this is
 * hm_conv2d_nhwc(first) followed by hm_conv2d_nhwc(second). */
int hm_conv2d_stem_pair(const hm_conv_args* first, const hm_conv_args* second, void* stream);

/* nn.MaxPool2d(k, stride, pad) on NHWC 16-bit (MP common.py:34-40: k=2,s=2; SPPCSPC common.py:275:
 * k=5/9/13, s=1, pad k/2 -- the 9 and 13 windows are cascades of the 5 window). C % 8 == 0. */
int hm_maxpool_nhwc(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int k, int stride, int pad,
                    int dtype, void* stream);

/* (B,3,H,W) f32 planes -> NHWC 16-bit with 8 channels (3 real, 5 zero): the convolution input layout, for crops that
 * hm_crop_batch produced in HaMeR's layout (RootNet patch, rootnet/Model_RGB.py:596-610). */
int hm_nchw3_to_nhwc8(const float* x, void* y, int B, int H, int W, int dtype, void* stream);
/* ResRootNet.forward_coord (rootnet/Model_RGB.py:282-292): global average pool of feat [B][HW][C] (16-bit), 1x1 conv to
 * one channel (w [C], bias), times k_value[b] -> depth [B] f32. */
int hm_gap_linear(const void* feat, int HW, int C, const float* w, float bias, const float* k_value, float* depth, int B,
                  int dtype, void* stream);

/* nn.Upsample(scale_factor=2, mode='nearest') on NHWC 16-bit (yolov7.yaml:78,:92). C % 8 == 0. */
int hm_upsample2x_nhwc(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int dtype, void* stream);

/* letterbox (utils/datasets.py:999-1029, auto=True) + LoadImage.process_img (:137-141) + /255
 * (detector.py:121-125).  The plan is host-side scalar work; the resize follows cv2's 8-bit
 * INTER_LINEAR fixed-point algorithm (11-bit coefficients). */
typedef struct hm_letterbox_plan {
  int src_h, src_w;     /* frame size                                  */
  int new_w, new_h;     /* resized (unpadded) size                      */
  int top, left;        /* padding before the resized image             */
  int out_h, out_w;     /* network input size (multiples of the stride) */
  float gain, pad_x, pad_y; /* scale_coords inputs (general.py:323-331) */
} hm_letterbox_plan;
int hm_letterbox_plan_make(int H, int W, int new_shape, int stride, hm_letterbox_plan* plan);      /* host */
/* host: tab[0:new_w]=x0, [new_w:2new_w]=ax0, [2new_w:3new_w]=ax1, then y0, ay0, ay1 (3*new_h)     */
int hm_letterbox_tables(const hm_letterbox_plan* plan, int32_t* tab_host);
/* frame [H][W][3] u8 BGR -> x8 [out_h][out_w][8] 16-bit RGB/255 (+5 zero channels), and optionally
 * u8_chw [3][out_h][out_w] RGB (the reference's uint8 network input, for parity checks). */
int hm_letterbox(const uint8_t* frame, const hm_letterbox_plan* plan, const int32_t* tab_dev, void* x8, int dtype,
                 uint8_t* u8_chw, void* stream);
/* `nb` equally sized frames, frame i at frames + i * frame_stride_bytes, into x8 [nb][out_h][out_w][8] in one launch (round 3:
 * the folder drivers upload a chunk's frames as one tensor). */
int hm_letterbox_batch(const uint8_t* frames, size_t frame_stride_bytes, int nb, const hm_letterbox_plan* plan,
                       const int32_t* tab_dev, void* x8, int dtype, void* stream);

/* Detect decode (IDetect.fuseforward, yolo.py:148-184): raw [ny*nx][3*(5+nc)] f32 of one level ->
 * rows [row0 + a*ny*nx + y*nx + x][5+nc] of pred: sigmoid, xy = (2s-0.5+grid)*stride, wh = (2s)^2*anchor. */
int hm_yolo_decode(const float* raw, int ldraw, float* pred, int row0, int ny, int nx, int nc, float stride,
                   const float* anchors6_host, void* stream);
/* The same for `nb` images of one batched pass in one launch: image i's raw map starts ny*nx*ldraw floats after image i-1's,
 * its rows of pred `pred_rows_per_image` rows after (round 3: 3 launches per pass instead of 3 per frame). */
int hm_yolo_decode_batch(const float* raw, int ldraw, float* pred, int row0, int ny, int nx, int nc, float stride,
                         const float* anchors, int nb, size_t pred_rows_per_image, void* stream);

/* Test-time augmentation (csrc/tta.hip): Model.forward(x, augment=True), yolo.py:589-605.  For a letterboxed network input
 * x of h x w, in [0,1] and RGB, the reference runs forward_once on scale_img(x, s) for s = 1, 0.83, 0.67 -- the 0.83 pass on
 * x.flip(3), the left-right mirror -- divides each prediction's xywh by s, sets x = w - x on the mirrored pass, and
 * concatenates the three predictions per image in that order for ONE non_max_suppression.  scale_img (utils/torch_utils.py:
 * 247-257) with gs = the largest stride:
 *   resized size   (sh, sw) = (int(h * s), int(w * s))                    in doubles, as Python
 *   padded size    (hp, wp) = (ceil(h * s / gs) * gs, ceil(w * s / gs) * gs)
 *   resize         F.interpolate(mode='bilinear', align_corners=False): along each axis, for output d < out,
 *                  src = max(0, (in / out) * (d + 0.5) - 0.5) in fp32 -- in / out and d + 0.5 rounded, the multiply and
 *                  subtract as one fused multiply-add, which is how torch's kernels evaluate it; tap0 = (int)src,
 *                  tap1 = tap0 + (tap0 < in - 1), weight1 = src - tap0, weight0 = 1 - weight1
 *   pad            right and bottom with 0.447 (F.pad) up to (hp, wp)
 * 384 x 640 gives 384x640, 320x544 (resized 318x531) and 288x448 (257x428): 15120 + 10710 + 7938 = 33768 rows per image.
 *
 * hm_tta_sizes (host): sizes4 = {sh, sw, hp, wp}.
 * hm_tta_tables (host): the taps of one plan, 4 * wp + 4 * hp int32 -- columns first:
 *   tap0[wp] | tap1[wp] | weight0[wp] | weight1[wp] (fp32 bits), then the same four for the hp rows.
 *   Outputs past the resized size are padding: taps -1, weights 0.  flip_lr folds the mirror into the column taps
 *   (tap -> w - 1 - tap), so the mirrored image is never written.
 * hm_tta_scale: x [nb][h][w][8] -> y [nb][hp][wp][8] in `dtype` (HM_DTYPE_F16, HM_DTYPE_BF16 or HM_DTYPE_F32), tab_dev the
 *   table of hm_tta_tables for the same (h, w, ratio, gs) on the device.  Channels 0-2 are interpolated in fp32 from the
 *   four taps (columns first, then rows) and rounded once to `dtype`; padding pixels get 0.447 rounded to `dtype`; channels
 *   3-7 are 0.  x and y must not overlap.
 * All three: HM_ERR_ARG, before any device work, for a null pointer, h, w or gs outside 1..16384, a ratio outside (0, 1] (or
 *   NaN), a resized side of 0 pixels; hm_tta_scale also for nb outside 1..65535, an unknown dtype, x or y not aligned to one
 *   pixel (16 bytes, 32 with HM_DTYPE_F32) or a table not aligned to 4 bytes. */
int hm_tta_sizes(int h, int w, double ratio, int gs, int* sizes4);                                      /* host */
int hm_tta_tables(int h, int w, double ratio, int gs, int flip_lr, int32_t* tab_host);                  /* host */
int hm_tta_scale(const void* x, void* y, const int32_t* tab_dev, int nb, int h, int w, double ratio, int gs, int dtype,
                 void* stream);
/* hm_yolo_decode_batch for one scale of a TTA pass: the same decode (the same bits), then xywh = xywh / scale as an fp32
 * IEEE division (torch divides; not a reciprocal multiply), then x = full_w - x when flip_lr (yolo.py:599-603).  The
 * confidence and class columns are those of hm_yolo_decode_batch.  HM_ERR_ARG as hm_yolo_decode_batch, and for a scale outside
 * (0, 1] or a flipped pass without a positive full_w. */
int hm_yolo_decode_batch_tta(const float* raw, int ldraw, float* pred, int row0, int ny, int nx, int nc, float stride,
                             const float* anchors, int nb, size_t pred_rows_per_image, float scale, int flip_lr, float full_w,
                             void* stream);

/* non_max_suppression (utils/general.py:611-703, best-class branch) + scale_coords/clip/round
 * (general.py:323-344, detector.py:142).  pred [n][5+nc] f32.  class_mask: bit c set = class c kept.
 * Workspace: hm_nms_workspace_bytes(n).  dets [max_det][6] f32 = x1,y1,x2,y2,conf,cls (score order),
 * count[0] = number of rows.  When plan != NULL boxes are mapped to frame pixels and rounded. */
size_t hm_nms_workspace_bytes(int n);
int hm_yolo_nms(const float* pred, int n, int nc, float conf_thres, float iou_thres, unsigned class_mask, int agnostic,
                int max_det, const hm_letterbox_plan* plan, float* dets, int* count, void* workspace,
                size_t workspace_bytes, void* stream);

/* The same function for the nb images of a pass in ONE call (csrc/nms_batch.hip): one memset of the counters, one filter
 * launch over nb * n rows, one suppression launch of nb workgroups -- the number of launches does not depend on nb.  Image i
 * reads pred + i * pred_image_stride (floats, [n][5+nc] f32), writes dets + i * dets_image_stride * 6 (stride in ROWS,
 * >= max_det) and count[i]; rows past count[i] are not written.  Both branches of general.py:611-703 (labels=(), no merge):
 *   multi_label == 0  best class per row (:665-667): the bytes hm_yolo_nms gives for that image alone;
 *   multi_label == 1  every class c with obj * cls_c > conf_thres is a candidate (:662-664), in (row, class) order; nc == 1
 *                     turns it off (:628).
 * Per image: rows with obj > conf_thres; score s_c = cls_c * obj (one fp32 multiply; obj itself when nc == 1); class_mask;
 * box = x -+ w/2, y -+ h/2; descending score, EQUAL SCORES BY ASCENDING row * nc + c (the reference leaves that to its sort);
 * the best 30000 enter the suppression (:681-682; the reference's argsort there is not stable, this one is); greedy NMS on
 * box + cls * 4096 (0 when agnostic; the sum rounded to fp32), IoU = inter / (area_i + area_j - inter), each product and sum
 * rounded on its own, suppressed when IoU > iou_thres (a NaN does not suppress); the first max_det kept, in score order, as
 * x1, y1, x2, y2, conf, cls without the class offset; plan != NULL: subtract pad, divide by gain, clamp, rintf as hm_yolo_nms.
 * Workspace, with C = n * (multi_label && nc > 1 ? nc : 1), pow2(x) the least power of two >= x:
 *   int counter[nb] rounded up to 256 bytes, then per image  u64 key[pow2(C)] | float4 box[n] | float4 sorted[min(C, 30000)]
 *   hm_nms_batch_workspace_bytes = roundup(nb * 4, 256) + nb * (pow2(C) * 8 + n * 16 + min(C, 30000) * 16), 0 for a refused shape.
 * A key is (sortable(score) << 32) | ~(row * nc + c); score and class are read back out of it.
 * HM_ERR_ARG before any device work: a null pred / dets / count / workspace, nb outside 1..4096, nc outside 1..32, max_det
 * outside 1..1024, n <= 0 or C > 1048576, conf_thres < 0 or NaN, dets_image_stride < max_det, a workspace smaller than the
 * above or not 16-byte aligned. */
size_t hm_nms_batch_workspace_bytes(int nb, int n, int nc, int multi_label);
int hm_yolo_nms_batch(const float* pred, size_t pred_image_stride, int nb, int n, int nc, float conf_thres, float iou_thres,
                      unsigned class_mask, int agnostic, int multi_label, int max_det, const hm_letterbox_plan* plan,
                      float* dets, size_t dets_image_stride, int* count, void* workspace, size_t workspace_bytes, void* stream);

/* One enqueue for a whole planned graph (Model.forward_once, yolo.py:609-639): the host planner
 * (hamer_yolo_amd/yolo/engine.py) turns the layer list into this op array once per input size. */
enum { HM_OP_CONV = 0, HM_OP_MAXPOOL = 1, HM_OP_UPSAMPLE2X = 2,
       HM_OP_CONV_PAIR = 3 /* this op's conv and the NEXT op's (kind HM_OP_CONV) through hm_conv2d_stem_pair; the next op is consumed */ };
typedef struct hm_yolo_op {
  int kind;
  int pool_pad;       /* HM_OP_MAXPOOL: padding; ksize/stride/N/H/W_in/Cin(=C)/X/Y/ldx/ldy/dtype come from conv */
  hm_conv_args conv;
} hm_yolo_op;
int hm_yolo_run(const hm_yolo_op* ops_host, int n_ops, void* stream);

/* Mesh overlay (hamer/reconstruct.py project_and_draw, :50-86): every face of every mesh filled into its
 * frame, then blended with it.  The drawing rule, bit-exact (tests/render_rule.py restates it in numpy):
 *  - geometry: a mesh is camera-frame vertices (fp64; the OBJ of reconstruct_and_save_obj_with_wrapper: MANO vertices,
 *    x := -x for left hands, + cam_t) and triangles of one frame.  A corner's z == 0 becomes 1e-5, then in fp64, without
 *    contraction and in this order, w = K20*x + K21*y + K22*z, u = (K00*x + K01*y + K02*z) / w, v = (K10*x + K11*y + K12*z) / w,
 *    each truncated toward zero to int32 (astype(np.int32)).  Deviation: a face is skipped if a corner has z <= 0, if
 *    |u| or |v| >= 2^24 (or is not a number), or if a corner index lies outside [0, nv) (the reference draws something
 *    undefined in the first two cases);
 *  - coverage: integer pixel (x, y) of the frame lies in the CLOSED triangle of the three integer corners (int64 edge
 *    functions, winding-independent); a face of area 0 covers the integer points of its three segments.  cv2's own
 *    scanline edge rule is not reproduced: the bytes are exact to this rule, unpinned against cv2.fillConvexPoly;
 *  - visibility: a pixel takes the covering face of smallest key (fp32(((z0 + z1) + z2) / 3 in fp64), global face id), the
 *    reference's painter's order (nearest drawn last), ties to the lower id.  The global face id is the face's row in
 *    `faces`, so the result depends neither on the order of the mesh table nor on scheduling;
 *  - HM_STYLE_FLAT (reconstruct.py): colour per mesh (BGR); a covered pixel becomes rint_half_even(a*c + b*i) per channel in
 *    fp32 (product, product, sum), a = (float)alpha, b = (float)(1.0 - alpha) (cv2.addWeighted(overlay, 0.6, image, 0.4, 0));
 *  - HM_STYLE_SHADED (an approximation of MeshRenderer + image_fusion, not pyrender's lighting): base colour (1.0, 1.0, 0.9)
 *    RGB times I = 0.3 + 0.7*|n.z| (n the fp64 unit face normal, 0 for a face of area 0 in space), each channel
 *    rint_half_even(255 * base * I) in fp64, replacing the pixel opaquely; the mesh colour is not used;
 *  - every pixel no face covers is byte-identical to the input. */
enum { HM_STYLE_FLAT = 0, HM_STYLE_SHADED = 1 };
typedef struct hm_mesh {
  int32_t frame;          /* frame of the batch the mesh is drawn into                                       */
  int32_t v0, nv;         /* its vertices: rows v0 .. v0 + nv - 1 of verts                                   */
  int32_t f0, nf;         /* its faces: rows f0 .. f0 + nf - 1 of faces, corner indices relative to v0 (0 .. nv-1);
                             two meshes never share a face row                                                 */
  uint8_t color_bgr[3];   /* HM_STYLE_FLAT colour                                                              */
  uint8_t reserved;
} hm_mesh;
/* Workspace of one call; the first N*H*W*8 bytes are the per-pixel key buffer, which must hold 0xFF bytes on entry.  Fill
 * the workspace with 0xFF once when it is allocated: every call resets the keys it wrote, so it stays reusable. */
size_t hm_mesh_overlay_workspace_bytes(int N, int H, int W, int n_meshes, int n_faces);
/* frames [N][H][W][3] u8 BGR (device), K [N][3][3] fp64 per frame (device), verts [n_verts][3] fp64 (device), faces
 * [n_faces][3] int32 (device), meshes_host [n_meshes] (HOST, read before return), out [N][H][W][3] u8 (device, never
 * overlapping frames).  0 <= alpha <= 1.  Three launches (setup, raster, compose) and one memset of the workspace's
 * counters; no host synchronisation.  n_meshes == 0 copies the frames. */
int hm_mesh_overlay(const uint8_t* frames, int N, int H, int W, const double* K, const double* verts, int n_verts,
                    const int32_t* faces, int n_faces, const hm_mesh* meshes_host, int n_meshes, int style, double alpha,
                    uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* Z-buffered mesh renderer (hamer/utils/mesh_renderer.py MeshRenderer.__call__, :243-320: `color, rend_depth =
 * renderer.render(...)`): per view an RGBA image, a depth map and a mesh-label map, resolved per
 * pixel.  The rule, stated once (tests/zrender_rule.py restates it in numpy).  Every fp64 expression is evaluated left to
 * right as written, without contraction:
 *  - geometry: vertices are camera-frame fp64, x right, y down, z forward.  K is given per view on the HOST and its last row
 *    must be exactly (0, 0, 1).  u = ((K00*x + K01*y) + K02*z) / z, v = ((K10*x + K11*y) + K12*z) / z; fixed point
 *    X = rint_half_even(256*u), Y = rint_half_even(256*v) (int64).  A face is skipped if a corner has z < znear (or z not a
 *    number), if |u| or |v| >= 2^16 (or not a number), if a corner index lies outside [0, nv), or if twice its signed area
 *    A = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0) is 0.  There is no near-plane clipping (a deviation from pyrender);
 *  - coverage: pixel (px, py) is sampled at its centre (256*px + 128, 256*py + 128).  If A < 0, corners 1 and 2 are swapped
 *    with everything they carry, and A := -A.  E_i is the edge function (bx-ax)*(py-ay) - (by-ay)*(px-ax) of the edge opposite
 *    corner i (1->2, 2->0, 0->1) at the sample.  The pixel is covered if every E_i is > 0, or == 0 on an edge that owns its
 *    boundary: edge a->b owns it when dy < 0, or dy == 0 and dx > 0 (the top-left rule), so faces that share an edge cover
 *    each sample on it exactly once;
 *  - depth: lambda_i = (double)E_i / (double)A, r_i = 1.0 / z_i, q = (lambda0*r0 + lambda1*r1) + lambda2*r2,
 *    d = (float)(1.0 / q).  A pixel takes the covering face of smallest key (bits(d) << 32) | global face id: the nearest,
 *    ties to the lower face row; the result depends neither on the order of the mesh table nor on scheduling;
 *  - shading: the vertex normal n_v is the sum, from zero and in ascending face row, over the mesh's faces with three valid
 *    corner indices that name v (once per face), of (p1-p0) x (p2-p0) in the face's own corner order, components
 *    ay*cz - az*cy, az*cx - ax*cz, ax*cy - ay*cx.  At a pixel a_i = lambda_i*r_i, m_c = (a0*n0c + a1*n1c) + a2*n2c,
 *    t = |m_z| / sqrt((m_x*m_x + m_y*m_y) + m_z*m_z) (0 when the length is not > 0), I = 0.3 + 0.7*t, and each channel is
 *    rint_half_even(255*base_c*I) clamped to 0..255 (not-a-number gives 0).  Smooth, per pixel and two-sided: a left hand
 *    needs no flipped faces.  It is the SHADED style's ambient + headlight term, not pyrender's BRDF;
 *  - outputs, each optional (NULL), at least one: rgba u8 [N][H][W][4] in R G B A order (uncovered: bg_rgba; covered: the
 *    colour, alpha 255); depth f32 [N][H][W] (uncovered 0.0f, covered d); mesh_id i32 [N][H][W] (uncovered -1, covered the
 *    mesh's row in meshes_host); frames + out u8 BGR [N][H][W][3], both or neither, never overlapping (uncovered: the
 *    frame's bytes; covered: the colour, opaque).
 * hm_mesh.frame is the view; color_bgr is not used; two meshes share neither face rows nor vertex rows.  base_rgb: HOST
 * double[3] in [0, 1], NULL = (1.0, 1.0, 0.9); bg_rgba: HOST u8[4], NULL = all 0; znear > 0 (pyrender's default is 0.05).
 * The workspace's first N*H*W*8 bytes are the key buffer with hm_mesh_overlay's contract (0xFF on entry, 0xFF on return), so
 * one 0xFF-filled workspace serves both entry points.  Launches: one memset, normals + setup per 48 meshes, raster, resolve;
 * no host synchronisation; argument errors return HM_ERR_ARG before any device work.  Alignment: workspace and verts 8 bytes,
 * faces, rgba, depth and mesh_id 4 bytes; with W % 4 == 0, workspace, rgba, depth and mesh_id 16-byte and frames, out 4-byte
 * aligned, resolve moves four pixels per lane. */
size_t hm_mesh_render_workspace_bytes(int N, int H, int W, int n_verts, int n_meshes, int n_faces);
int hm_mesh_render(int N, int H, int W, const double* K_host, const double* verts, int n_verts, const int32_t* faces,
                   int n_faces, const hm_mesh* meshes_host, int n_meshes, const double* base_rgb, const uint8_t* bg_rgba,
                   double znear, const uint8_t* frames, uint8_t* out, uint8_t* rgba, float* depth, int32_t* mesh_id,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Hand skeletons (rootnet/vis_tool.py draw_2d_skeleton, :602-640; hamer/utils/draw_2d_skeleton.py; hamer/utils/render_openpose.py
 * render_keypoints, :56-91): the 20 bones and 21 joint discs of every hand drawn opaquely onto its image.
 * The drawing rule, bit-exact (tests/skeleton_rule.py restates it in numpy as a sequential painter); it generalises
 * rootnet/Model_RGB.py draw_2d_skeleton, which it equals at line_radius 0, joint_radius 2:
 *  - joints: joint j of a hand is the point p_j = (trunc(u), trunc(v)), truncated toward zero to int32.  A joint is ABSENT if u
 *    or v is not finite, if |u| or |v| >= 32768, or, with kp_stride 3, if `conf > threshold` is false (render_openpose.py:76,85).
 *    An absent joint draws no disc, and no bone that touches it is drawn (a deviation: the host rule is undefined for
 *    non-finite and out-of-range inputs);
 *  - bone j (j = 1..20) runs a -> b with a = p_parent(j), b = p_j, parent(j) = 0 if j % 4 == 1 else j - 1.  dx = bx - ax,
 *    dy = by - ay, m = max(|dx|, |dy|).  Its samples are s_i = (rint(ax + t_i*dx), rint(ay + t_i*dy)), i = 0..m, with
 *    t_i = i * (1.0 / m) for i < m and t_m = 1.0 (m = 0: the one sample a), all in fp64 without contraction, rint half-to-even
 *    (numpy's linspace(0, 1, m + 1), then np.rint).  The bone covers pixel (x, y) iff some sample has
 *    (x - sx)^2 + (y - sy)^2 <= line_radius^2;
 *  - disc j covers (x, y) iff (x - px)^2 + (y - py)^2 <= joint_radius^2.  Radii are integers in 0..32;
 *  - order, per hand: HM_SKEL_INTERLEAVED: for j = 0..20 bone j (j > 0), then disc j; HM_SKEL_BONES_FIRST
 *    (render_keypoints:74-91): bones 1..20, then discs 0..20.  Bone j and disc j have colour palette[j].  Hands are drawn in
 *    table order, a later hand over an earlier one: a pixel gets the colour of the covering primitive with the largest
 *    (hand index, draw index), opaque, its three bytes to channels 0, 1, 2 as the image stores them; uncovered pixels keep
 *    their bytes.  The result does not depend on scheduling.
 * cv2.line / cv2.circle pixels and the reference's LINE_AA are not reproduced: the bytes are exact to this rule, unpinned
 * against cv2. */
enum { HM_SKEL_INTERLEAVED = 0, HM_SKEL_BONES_FIRST = 1 };
typedef struct hm_skeleton {
  int32_t image;                      /* image of the batch the hand is drawn into; its keypoints are row i of kp    */
  int32_t line_radius, joint_radius;  /* 0..32                                                                       */
  float threshold;                    /* kp_stride 3: a joint is drawn if conf > threshold                           */
} hm_skeleton;
/* 0 when n_hands <= 0 (no workspace is needed then) or the sizes are invalid. */
size_t hm_skeleton_overlay_workspace_bytes(int N, int H, int W, int n_hands);
/* images [N][H][W][3] u8 (device), kp [n_hands][21][kp_stride] f32 (device, never read back; kp_stride 2: u v, 3: u v conf),
 * hands_host [n_hands] and palette_host [21][3] u8 (HOST, read before return), out [N][H][W][3] u8 (device): out == images is
 * the in-place form, which touches only 16 x 16 tiles inside some hand's box; otherwise out must not overlap images and gets
 * one device-to-device copy first.  One memset of the workspace's counters, a setup launch per 128 hands and one raster launch;
 * no host synchronisation.  n_hands == 0 is valid (the copy alone; kp, the tables and the workspace may be NULL).  HM_ERR_ARG
 * before any device work: N, H or W <= 0, H or W > 16384, kp_stride not 2 or 3, an unknown order, a radius outside 0..32, an
 * image outside 0..N-1, a null pointer with n_hands > 0 (images and out always), out partly overlapping images, a workspace
 * smaller than hm_skeleton_overlay_workspace_bytes.  Alignment: kp 4 bytes, workspace 8 bytes. */
int hm_skeleton_overlay(const uint8_t* images, int N, int H, int W, const float* kp, int kp_stride,
                        const hm_skeleton* hands_host, int n_hands, const uint8_t* palette_host, int order, uint8_t* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- SAR hand-mesh head of the RootNet checkpoint (rootnet/Model_RGB.py:76-177 SoftHeatmap / GraphConv / SAIGB / GBBMR,
 * :198-222 SARhead, :428-480 post_processing, :500-570 EstimateRGB.run).  f16 operands, fp32 accumulation; activations are
 * node-major across the batch, [778][B][C].  No split-K and no batch-dependent reduction order: a hand's numbers are the
 * same alone and inside any batch.  All pointers are device pointers unless marked HOST. */

/* SAIGB (:119-136): feat [B][8][8][512] f16 (NHWC backbone output), w [6224][512] f16 (the 1x1 conv), bias [6224] f32,
 * tmpl [778][3] f32 (head.saigb.template) -> g [778][B][544] f16: node v, hand b holds LeakyReLU_0.1(conv + bias) of
 * channels 8v .. 8v+7 x the 64 positions (the .view(-1, 778, 512) of NCHW), then the 3 template values, then 29 zeros. */
int hm_sar_saigb(const void* feat, const void* w, const float* bias, const float* tmpl, void* g, int B, void* stream);
/* hm_sar_saigb for a backbone of `channels` feature channels: 512 (the ResNet-34, the same bytes as hm_sar_saigb) or 1024
 * (ConvNeXt-base): feat [B][8][8][channels] f16, w [6224][channels] f16; g as above (SAIGB's output channels do not depend on
 * its input channels).  feat / w 16-byte aligned. */
int hm_sar_saigb_ch(const void* feat, const void* w, const float* bias, const float* tmpl, void* g, int B, int channels,
                    void* stream);
/* The L . x of GraphConv.forward (:110-115) for all hands at once: y [778][N] f16 = lap [778][ldl] f16 . x [778][N] f16,
 * lap = adj / (rowsum(adj) + 1e-5) with columns 778 .. ldl-1 zero; ldl % 32 == 0, N % 8 == 0 (N = B * C). */
int hm_sar_graph_mix(const void* lap, int ldl, const void* x, int N, void* y, void* stream);
/* GraphConv.fc (:115) over M = 778 * B rows: y [M][N] = x [M][K] f16 . w [N][K]^T f16 + bias [N] f32; out_f32 == 0:
 * LeakyReLU(0.1) (:148-149) and f16 out, out_f32 == 1: no activation, f32 out (the second layer's logits).  K % 32 == 0
 * (zero-padded columns in both operands). */
int hm_sar_linear(const void* x, int M, int K, const void* w, const float* bias, void* y, int N, int out_f32, void* stream);
/* GBBMR.forward's tail (:163-176): logits_xy / logits_z are [799][B][1024] f32 whose rows 0 .. 777 hold the two branches'
 * second-layer logits; rows 778 .. 798 are WRITTEN here by mesh2pose_hm / mesh2pose_dm (w [21][778], b [21]).  Then
 * SoftHeatmap (:76-99): beta [799] (beta.weight), softmax over the 1024 cells, x = sum p * wx, y = sum p * wy (the
 * checkpoint's [32][32] wx / wy buffers), z = sum p * heatmap_z, xy / 16 - 1 -> coords [B][799][3] f32.  Two launches. */
int hm_sar_softargmax(float* logits_xy, float* logits_z, const float* m2p_w_xy, const float* m2p_b_xy, const float* m2p_w_z,
                      const float* m2p_b_z, const float* beta, const float* wx, const float* wy, float* coords, int B,
                      void* stream);
/* One hand of hm_sar_postprocess. */
typedef struct hm_sar_hand {
  float bb2img[6];        /* 2x3 patch -> frame map (generate_patch_image's inv_trans), f32                          */
  float depth_box;        /* cfg.depth_box (0.3)                                                                      */
  int32_t flip;           /* 1: left hand, x -> img_w - x - 1 after the map (:445-446)                                */
  int32_t img_w, img_h;   /* frame size                                                                               */
  int32_t depth_w, depth_h; /* size of this hand's depth map                                                          */
  int64_t depth_offset;   /* >= 0: root depth = grid_sample of depth + depth_offset (f32 metres) at row 778, else root */
  double fx, fy, fu, fv;  /* camera K                                                                                 */
} hm_sar_hand;
/* post_processing (:428-480) with run's root depth (:533-551): coords [B][799][3] f32 (hm_sar_softargmax), hands [B]
 * (device), root [B] f32 metres or NULL (0), depth: the depth maps hands[].depth_offset points into, or NULL.
 * z = z * depth_box + root; uv = (uv + 0.5) * P; bb2img; flip; uvd2xyz (preprocessing.py:11-17) -> uvd, xyz [B][799][3]
 * f32 (rows 778 .. are the joints).  With a depth map the root is the bilinear (zeros, align_corners=False) sample at
 * convert2origin_pixel(row 778) / (W // 2, H // 2) - 1, which for a left hand is NOT un-flipped: the reference's rule. */
int hm_sar_postprocess(const float* coords, const hm_sar_hand* hands, const float* root, const float* depth, float* uvd,
                       float* xyz, int B, int P, void* stream);


/* ---- The precise (fp32) route of the RootNet backbone, the depth head and the SAR head (EstimateRGB(cfg, precise=True)):
 * the reference runs that network in fp32 (rootnet/Model_RGB.py:318-340).  Every product runs on the fp32-input MFMA and every
 * output is bias + ONE sum over K in a fixed order: no split-K, no K groups, no batch-dependent reduction, so the route is
 * deterministic and batch-invariant (a hand's numbers are the same bits alone and inside any batch).  These are additive
 * entry points: hm_conv2d_nhwc keeps rejecting fp32 with ReLU or a residual, and hm_nchw3_to_nhwc8 / hm_gap_linear keep
 * rejecting HM_DTYPE_F32.  hm_maxpool_nhwc (HM_DTYPE_F32), hm_sar_softargmax and hm_sar_postprocess (already fp32) serve both
 * routes. */

/* The ResNet-34 convolution in fp32 (conv_f32.hip's kernel with a ReLU / residual epilogue): dtype must be HM_DTYPE_F32, act 0
 * or 2 (ReLU), out_f32 0; X, W, Y, bias fp32 with the layouts of hm_conv_args; optional resid [N][Hout][Wout][ldr] fp32 added
 * before the ReLU (BasicBlock identity; ldr >= Cout).  Cin a power of two >= 8, X / W 16-byte aligned, ldx % 4 == 0; zeros and
 * splitk_ws are not used.  Within ~1e-6 * sum|x * w| of exact. */
int hm_conv2d_f32_relu(const hm_conv_args* args, void* stream);
/* (B,3,H,W) f32 planes -> NHWC f32 with 8 channels (3 real, 5 zero); y 16-byte aligned. */
int hm_nchw3_to_nhwc8_f32(const float* x, float* y, int B, int H, int W, void* stream);
/* ResRootNet.forward_coord on fp32 features [B][HW][C]: per channel the HW positions summed in order, / HW, dot with w [C]
 * in a fixed order, + bias, * k_value[b] -> depth [B] f32.  The order depends on HW and C only. */
int hm_gap_linear_f32(const float* feat, int HW, int C, const float* w, float bias, const float* k_value, float* depth, int B,
                      void* stream);
/* hm_sar_saigb in fp32: feat [B][8][8][512], w [6224][512] (16-byte aligned), bias [6224], tmpl [778][3] -> g [778][B][544]. */
int hm_sar_saigb_f32(const float* feat, const float* w, const float* bias, const float* tmpl, float* g, int B, void* stream);
/* hm_sar_graph_mix in fp32: y [778][N] = lap [778][ldl] . x [778][N]; ldl >= 778, ldl % 4 == 0, columns 778 .. ldl-1 of lap
 * zero; N % 4 == 0; lap / x 16-byte aligned.  Rows of x are never read past 778. */
int hm_sar_graph_mix_f32(const float* lap, int ldl, const float* x, int N, float* y, void* stream);
/* hm_sar_linear in fp32: y [M][N] = x [M][K] . w [N][K]^T + bias [N]; logits == 0: LeakyReLU(0.1), logits == 1: no
 * activation (the second layer's logits, rows 0 .. 777 of hm_sar_softargmax's [799][B][1024] buffers).  K % 32 == 0
 * (zero-padded columns in both operands); x / w 16-byte aligned. */
int hm_sar_linear_f32(const float* x, int M, int K, const float* w, const float* bias, float* y, int N, int logits, void* stream);

/* ---- The precise (fp32) route of HaMeR (HAMER(..., dtype=torch.float32), load_hamer(path, precise=True)).
 * nn.Linear in fp32 on v_mfma_f32_32x32x2_f32: C [M][ldc] f32 = epilogue(X [M][ldx] f32 . W [N][ldw]^T f32).  Replaces the
 * fp32 aten::addmm behind Attention.qkv / .proj (vit.py:114,:124), Mlp.fc1 / .fc2 (vit.py:83,:85), PatchEmbed.proj (vit.py:172,
 * after hm_patch_im2col) and CrossAttention.to_kv (pose_transformer.py:114).  args->dtype must be HM_DTYPE_F32; epilogues
 * HM_EPI_F32 (acc + bias), HM_EPI_GELU (gelu_erf(acc + bias)), HM_EPI_RESID_F32 ((acc + bias) + resid[m % resid_mod][n], resid
 * may alias C); C is fp32 in all three; bias may be NULL.  k_split, ln_*, out_scale must be unset.  Any M >= 1, any N >= 1,
 * K % 32 == 0, ldx / ldw multiples of 4, X / W 16-byte aligned.  Every output's sum over K is ONE fmaf chain from zero in an
 * order fixed by K alone (no split-K, no tile- or grid-dependent reduction): a row's result does not depend on M or on its
 * position, and is within ~4.5e-7 * (1 + sum|x w|) of exact up to K = 5120. */
int hm_gemm_f32(const hm_gemm_args* args, void* stream);
/* Attention.forward core (vit.py:115-123) in fp32: qkv [B*192][3*heads*80] f32 (column = which*H*d + head*d + i) -> out
 * [B*192][heads*80] f32, head-major.  q * scale first (vit.py:116-117), q k^T and P V on v_mfma_f32_16x16x4_f32, softmax with
 * the row maximum subtracted, expf, a row sum in one fixed order and IEEE division.  tokens == 192 and head_dim == 80 only.
 * A hand's result does not depend on B. */
int hm_vit_attention_f32(const float* qkv, float* out, int B, int tokens, int heads, int head_dim, float scale, void* stream);

/* ---- The ConvNeXt-base SAR backbone (rootnet/convnext.py; EstimateRGB with backbone = 'convnext'): the kernels around its
 * GEMMs.  The residual stream is fp32 NHWC [B][H][W][C]; the 16-bit outputs are the X operands of hm_gemm.  fp32 arithmetic,
 * one rounding at the store; a pixel's bytes depend on C alone, not on B or on its position in the batch.  dtype:
 * HM_DTYPE_BF16 or HM_DTYPE_F16.  fp32 pointers 16-byte aligned, 16-bit outputs 8-byte aligned; C % 4 == 0, C <= 1024. */

/* Block.dwconv + Block.norm (convnext.py:28-29, :39-41): out [B*H*W][C] 16-bit = LayerNorm_C(depthwise 7 x 7 conv of x, zero
 * padding 3, + bias) * gamma + beta.  w [49][C] fp32, tap-major (ky * 7 + kx): nn.Conv2d's [C][1][7][7] weight transposed. */
int hm_dwconv7_ln(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, void* out, int B, int H,
                  int W, int C, float eps, int dtype, void* stream);
/* downsample_layers[1..3] up to their GEMM (convnext.py:79-82): LayerNorm over C of every pixel of x, written into the row of its
 * 2 x 2 patch: out [B*(H/2)*(W/2)][4C] 16-bit, column (ky * 2 + kx) * C + c (the Conv2d weight permuted to [2C][ky][kx][c]).
 * H and W even. */
int hm_ln_patchify2(const float* x, const float* gamma, const float* beta, void* out, int B, int H, int W, int C, float eps,
                    int dtype, void* stream);
/* The im2col of the stem (Conv2d(3, 128, 4, stride 4), convnext.py:74): img [B][3][H][W] fp32 planes (hm_crop_batch's output)
 * -> patches [B*(H/4)*(W/4)][64] 16-bit: 48 values in the weight's (c, ky, kx) order, then 16 zeros (hm_gemm: K % 64 == 0).
 * H % 4 == 0, W % 4 == 0. */
int hm_stem4_im2col(const float* img, void* patches, int B, int H, int W, int dtype, void* stream);

/* ---- Hand metrics (hamer/utils/pose_utils.py): MPJPE and Procrustes-aligned MPJPE of a batch in one launch.
 * Restates compute_similarity_transform (pose_utils.py:9-58: centroids, var1, K = X1 X2^T, R = V Z U^T with
 * Z = diag(1, 1, sign det(U V^T)), scale = trace(R K) / var1, t = mu2 - scale R mu1, S1_hat = scale R S1 + t),
 * reconstruction_error (:60-71), the two means of eval_pose (:83, :86; metres here, eval_pose multiplies by 1000) and the root
 * subtraction and keypoint selection of Evaluator.__call__ (:163-168).  fp32 in, every sum over points and the 3 x 3 solve in
 * fp64, one rounding to fp32 at the store.  One wave per hand; a hand's bytes do not depend on B or on its place in the batch.
 * var1 == 0 (one selected point, coincident predictions): pa_err, aligned and transform of that hand are NaN, err is not.
 * Coincident gt points (K = 0, var1 > 0) are finite as in the reference: R = I, scale = 0, S1_hat = mu2.  A non-finite input
 * makes every output of that hand that depends on it non-finite, and no other hand's. */
typedef struct hm_pose_eval_args {
  const float* pred;      /* [B][P][3] f32 */
  const float* gt;        /* [B][P][gt_stride] f32, the first 3 of each point are read; gt_stride 3 or 4
                             (batch['keypoints_3d'] is (B, 21, 4)) */
  int B, P, gt_stride;    /* P in 1..1024 */
  int root;               /* index into P or -1: pred[b][root] / gt[b][root] are subtracted from every point of hand b first
                             (Evaluator's pelvis_ind, :163-165), before the selection */
  uint64_t sel[16];       /* bit p set = point p takes part (Evaluator's keypoint_list); all zero = all P points */
  float* err;             /* [B] mean over the selected points of |pred - gt|, metres (MPJPE)              or NULL */
  float* pa_err;          /* [B] the same after the similarity alignment of pred onto gt (PA-MPJPE)        or NULL */
  float* aligned;         /* [B][n_sel][3] S1_hat, the selected points in ascending index order            or NULL */
  float* transform;       /* [B][13]: scale, R row-major (9), t (3), with S1_hat = scale * R * x + t, x a point of pred
                             after the root subtraction                                                    or NULL */
} hm_pose_eval_args;
/* All checks run on the host before the launch (HM_ERR_ARG): null args / pred / gt, B <= 0, P outside 1..1024, gt_stride not 3
 * or 4, root outside -1..P-1, a bit of sel at or past P, all four outputs NULL, pred or gt not 4-byte aligned. */
int hm_pose_eval(const hm_pose_eval_args* args, void* stream);

/* ---- Mesh F-scores and the area under the PCK curve: csrc/mesh_eval.hip.  The caller owns every buffer, the calls are
 * asynchronous on `stream`, nothing synchronises or allocates, argument errors return HM_ERR_ARG before any device work.  All
 * fp64 arithmetic is plain IEEE in the order written (no FMA contraction, no fast-math).
 *
 * hm_mesh_score: nearest-neighbour distances between two point sets per hand, both ways, and what the hand-mesh tables make of
 * them, in one launch (one 1024-thread workgroup per hand, both sets staged once in LDS as fp64).  Per hand: pred[b][root] and
 * gt[b][root] are subtracted from every point in fp64 (root >= 0), each participating pred point x becomes scale * R * x + t
 * in fp64 when `transform` is given (exactly the [13] hm_pose_eval writes), then for every participating point of one set
 *   d = sqrt(min over the participating points of the other set of (dx dx + dy dy) + dz dz),
 * a NaN candidate making the minimum NaN (numpy.min); precision[j] = #(d_pred < thr[j]) / pred_n, recall[j] =
 * #(d_gt < thr[j]) / gt_n (strict, in fp64 on the unrounded distances, NaN compares false), fscore = 2 p r / (p + r), 0 when
 * p + r == 0.  This is the F-score of the FreiHAND evaluation (its script names the two shares the other way round; F is
 * symmetric); it is UNPINNED against FreiHAND's script and open3d -- the rule above is the definition.  Every output is
 * rounded to fp32 once, at the store.  A hand's bytes do not depend on B or on its place in the batch; a non-finite input
 * reaches the outputs of its own hand only.
 * Measured on an MI355X (tools/bench_mesh_eval.py, profiles/mesh_eval_bench.log; per call, host submission included): 64 hands
 * of 778 x 778 points 0.163 ms, 1024 hands 0.648 ms (the same computation in torch ops: 1.17 / 16.9 ms). */
typedef struct hm_mesh_score_args {
  const float* pred;        /* [B][P][3] f32 */
  const float* gt;          /* [B][Q][gt_stride] f32, gt_stride 3 or 4; the fourth component is never read */
  const float* transform;   /* [B][13]: scale, R row-major, t (hm_pose_eval's layout), applied to pred       or NULL */
  int B, P, Q, gt_stride;   /* P and Q in 1..1024, independent of one another */
  int root;                 /* -1, or an index into both sets */
  int pred_lo, pred_n;      /* the participating pred points: pred_lo .. pred_lo + pred_n - 1 (pred_n >= 1) */
  int gt_lo, gt_n;          /* the participating gt points */
  int n_thr;                /* 0..8 */
  double thresholds[8];     /* metres */
  float* d_pred;            /* [B][pred_n] distance of every participating pred point to its nearest gt point  or NULL */
  float* d_gt;              /* [B][gt_n]   the other direction                                               or NULL */
  float* precision;         /* [B][n_thr]                                                                    or NULL */
  float* recall;            /* [B][n_thr]                                                                    or NULL */
  float* fscore;            /* [B][n_thr]                                                                    or NULL */
  float* point_err;         /* [B][pred_n] |pred_i - gt_i| of corresponding participating points (after the same root
                               subtraction and transform): the per-point error of the PCK curve; pred_n == gt_n   or NULL */
} hm_mesh_score_args;
/* HM_ERR_ARG: null args / pred / gt, B <= 0, P or Q outside 1..1024, gt_stride not 3 or 4, root outside -1..min(P, Q) - 1,
 * a range that leaves its set or is empty, n_thr outside 0..8 (0 with precision, recall or fscore wanted), point_err with
 * pred_n != gt_n, all six outputs NULL, pred / gt / transform not 4-byte aligned. */
int hm_mesh_score(const hm_mesh_score_args* args, void* stream);

/* hm_pck_auc: get_measures / _get_pck of rootnet/KeypointFusion/util/eval_utils.py (:38-75) for any number of keypoints K
 * (the reference is hard-wired to 21).  thresholds = np.linspace(val_min, val_max, steps) bit for bit, formed in the kernel
 * (i * step + start, step = (val_max - val_min) / (steps - 1), the last one set to val_max);
 *   pck[k][i] = #(err[n][k] <= thr[i]) / N   (the reference's <=; a NaN error is a miss; one division),
 *   auc[k] = trapz(pck[k], thr) / trapz(1, thr),  mean_auc = their mean,  curve[i] = mean over k of pck[k][i] (ascending k).
 * The counts are integer histograms (LDS atomics, then 64-bit integer atomics into `workspace`, which the call zeroes on the
 * stream first): the result does not depend on chunk_rows, the number of samples a workgroup takes (0: the default).  N is
 * bounded by memory only.  Three operations on the stream: the zeroing, the histogram, one finishing workgroup.
 * Measured on an MI355X (profiles/mesh_eval_bench.log; per call, 100 steps): N = 10000, K = 799 0.149 ms (torch ops 4.60 ms);
 * N = 64, K = 799 0.102 ms (torch ops 0.093 ms); N = 64, K = 21 0.033 ms (0.093 ms).
 * HM_ERR_ARG: a null args / err / pck / auc / workspace, N <= 0 (the reference returns None there and then fails), K < 1,
 * ld < K, steps outside 2..256, val_min >= val_max or either not finite, chunk_rows < 0, workspace_bytes below the query. */
typedef struct hm_pck_auc_args {
  const float* err;         /* [N][ld] f32 on the device, the first K of each row are read */
  long long N, ld, chunk_rows;
  double val_min, val_max;
  int K, steps;             /* steps in 2..256 */
  double* pck;              /* [K][steps] f64 */
  double* auc;              /* [K] f64 */
  double* mean_auc;         /* [1] f64                                                                       or NULL */
  double* curve;            /* [steps] f64                                                                   or NULL */
  double* thresholds;       /* [steps] f64, the thresholds as the kernel formed them                          or NULL */
  void* workspace; size_t workspace_bytes;
} hm_pck_auc_args;
size_t hm_pck_auc_workspace_bytes(int K, int steps);   /* 0 for an illegal K or steps */
int hm_pck_auc(const hm_pck_auc_args* args, void* stream);

/* ---- Mask scores: region similarity J and contour accuracy F of a predicted silhouette against a label mask, the pair of
 * segmentation measures of the DAVIS benchmark, written from its definition: csrc/mask_eval.hip.  The rule below is the
 * definition; it is UNPINNED against DAVIS's own script (and skimage), neither of which this project can run.
 *
 * For one query, pred and gt are binary images of H x W pixels.
 *   Boundary map  b(s)[y][x] = s[y][x] != s[y][x1] || s[y][x] != s[y1][x] || s[y][x] != s[y1][x1],
 *                 x1 = min(x + 1, W - 1), y1 = min(y + 1, H - 1): the east, south and south-east neighbours with the last row
 *                 and column replicated.  A full or an empty image has no boundary pixel; the bottom-right pixel never is one.
 *   Match         a boundary pixel of pred is matched when some boundary pixel of gt lies at an integer offset (dx, dy) with
 *                 dx dx + dy dy <= r r, and the same the other way round: dilation by a disk of radius r, in integers only.
 *   Radius        bound_radius(H, W, bound_th = 0.008) = bound_th if bound_th >= 1, else ceil(bound_th * sqrt(H H + W W)):
 *                 18 for 1080 x 1920, 12 for 720 x 1280 (hamer/utils/mask_eval.py).  The kernel takes r in 0..64.
 *   counts[q][8]  0 inter = sum(pred & gt), 1 pred_area, 2 gt_area, 3 pred_boundary, 4 gt_boundary, 5 pred_matched,
 *                 6 gt_matched, 7 pixels = H W: exact integers.
 *   From counts, in float64: J = 1 if pred_area + gt_area == 0, else inter / (pred_area + gt_area - inter);
 *                 P = pred_matched / pred_boundary, R = gt_matched / gt_boundary; neither boundary exists: P = R = 1; only gt
 *                 has one: P = 1, R = 0; only pred has one: P = 0, R = 1; F = 0 if P + R == 0, else 2 P R / (P + R).
 *
 * pred_id [N][H][W] int32 is what hm_mesh_render writes (a mesh index or -1); mask [N][H][W] uint8 is a label image.  Query q
 * looks at frame `frame`; a pixel is pred when id_lo <= pred_id < id_hi (an empty range is an empty pred) and gt when
 * mask == label, or mask != 0 when label == -1.  Several queries may name one frame.  A query whose frame is outside 0..N-1 is
 * not read: its counts are all zero, pixels included.  All 8 counts of every query are written on every call (callers do not
 * clear them).  A query's counts depend on its own images and the radius alone: not on Q, the order of the queries, the rest of
 * the batch or the grid (the sums are integer atomics).  Asynchronous on `stream`: three kernels, no host synchronisation, no
 * allocation.  Q == 0 succeeds and launches nothing (queries, counts and workspace may then be NULL).
 * HM_ERR_ARG before any device work: a null pointer, N, H or W < 1, N H W >= 2^31, radius outside 0..64, Q < 0, workspace_bytes
 * below the query, counts or workspace not 8-byte aligned (pred_id and queries: 4-byte).
 * Measured on an MI355X (tools/bench_mask_eval.py, profiles/mask_eval_bench.log; per call, host submission included, 1080 x 1920,
 * r = 18): 16 frames with one query each 0.148 ms, with four 0.377 ms; 64 frames 0.456 / 1.418 ms (the same counts from torch ops
 * on the device 12.4 / 49.3 / 48.9 / 197 ms; the hm_mesh_render call of the same frames 0.96 / 3.24 ms). */
typedef struct hm_mask_query { int32_t frame, id_lo, id_hi, label; } hm_mask_query;
size_t hm_mask_score_workspace_bytes(int Q, int H, int W, int radius);   /* 0 for illegal sizes; positive otherwise */
int hm_mask_score(const int32_t* pred_id, const uint8_t* mask, int N, int H, int W, const hm_mask_query* queries /* device */,
                  int Q, int radius, int64_t* counts /* device [Q][8] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Mask boxes: the tight bounding box and the pixel count of a label in a label mask, for many (frame, label) queries in
 * one call: csrc/mask_boxes.hip.  It is what get_bbox_from_npy (infer.py:1040-1072) takes from `np.where(mask == label)`, and
 * what feeds the batched mask-driven folder driver its hand boxes (hamer_yolo_amd/mask_boxes.py).
 *
 * mask [N][H][W] uint8 is a batch of label images.  A pixel belongs to query q when mask == label, or mask != 0 when
 * label == -1 (hm_mask_query's convention; any other label outside 0..255 is in no byte).  boxes[q] = x1, y1, x2, y2, count:
 * the least / greatest column, the least / greatest row and the number of such pixels of frame `frame`.  No such pixel, or a
 * frame outside 0..N-1 (which is not read), gives -1, -1, -1, -1, 0.  All five values of every query are written on every
 * call (callers do not clear them).  Several queries may name one frame.  A query's row depends on its own frame alone: not on
 * Q, the order of the queries, the rest of the batch or the grid (integer min / max / add atomics behind an initialisation
 * that is part of the call).  The frame is read as H * W consecutive bytes in 16-byte vectors from the first aligned address,
 * with up to 15 single bytes before and after: W, H * W and the mask's address need not be multiples of anything.
 * Asynchronous on `stream`: two kernels, no host synchronisation, no allocation.  Q == 0 succeeds and launches nothing
 * (queries and boxes may then be NULL).  HM_ERR_ARG before any device work: a null pointer, N, H or W < 1, N H W >= 2^31,
 * Q < 0, queries or boxes not 4-byte aligned.
 * Measured on an MI355X: tools/bench_mask_driver.py, profiles/mask_boxes_bench.log ("The mask-driven folder driver"). */
typedef struct hm_box_query { int32_t frame, label; } hm_box_query;
int hm_mask_boxes(const uint8_t* mask /* [N][H][W] */, int N, int H, int W, const hm_box_query* queries /* device */, int Q,
                  int32_t* boxes /* device [Q][5]: x1, y1, x2, y2, count */, void* stream);

/* ---- Depth residuals: the predicted hands' z-buffer against a sensor depth map: csrc/depth_eval.hip.  Per query a histogram of
 * `sensor - predicted` over the pixels its meshes cover, six pixel counts and four statistics; from the median follows the
 * shift of a hand along its viewing ray (hamer/utils/depth_eval.py refine_cam_t).
 *
 * pred_depth [N][H][W] f32 (metres, 0 where uncovered) and pred_id [N][H][W] i32 (mesh row or -1) are what hm_mesh_render
 * writes; sensor [N][H][W] u16 holds raw sensor units, 0 = no measurement; mask [N][H][W] u8 is a label image or NULL;
 * labels [Q] i32 or NULL gives per query -2 (no mask test), -1 (mask != 0) or 0..255 (mask == label; any other value: no pixel
 * passes); a NULL mask or NULL labels means no mask test.  mesh_query [n_meshes] i32 names the query a mesh's pixels count for,
 * or -1 for none; several meshes may share a query (a frame's union of hands).  unit: metres per raw unit; a raw value outside
 * raw_lo..raw_hi counts as no measurement; bin_m: the bin width in metres; bins: even, 2..4096.
 *
 * Rule per pixel p, all arithmetic fp64 and exactly as written: the unit is compiled with contraction off
 * (#pragma clang fp contract(off)), so no product is fused into a sum.
 *   1  id = pred_id[p]; the pixel is skipped unless 0 <= id < n_meshes and q = mesh_query[id] is in 0..Q-1
 *   2  counts[q][0] (covered) += 1
 *   3  a mask test applies and the pixel fails it: counts[q][1] (off mask) += 1, stop
 *   4  raw == 0, raw < raw_lo or raw > raw_hi: counts[q][2] (no measurement) += 1, stop
 *   5  r = (double)raw * unit - (double)pred_depth[p]
 *   6  k = (long long)floor(r / bin_m) + bins / 2
 *   7  k < 0: counts[q][3] (below: something nearer than the hand) += 1; k >= bins: counts[q][4] (above) += 1; otherwise
 *      hist[q][k] += 1 and counts[q][5] (in range) += 1.  (floor(...) below -2^40 is below, at or past 2^40 or NaN is above.)
 * hist u32 [Q][bins], counts i64 [Q][8] (entries 6 and 7 are written 0) and stats f64 [Q][4] are all written on every call
 * (callers do not clear them).  stats, from hist and counts alone, with centre(k) = ((double)(k - bins / 2) + 0.5) * bin_m:
 *   0  the LOWER median: n = below + in_range + above, rank m = (n + 1) / 2 counted from 1, the below pixels first and the above
 *      pixels last; centre(k) of the bin that holds rank m; NaN when n == 0 or the rank falls in below or above
 *   1  mean = S1 / in_range, 2 mean absolute = S2 / in_range, 3 rms = sqrt(S3 / in_range), where over the occupied bins in
 *      ascending k, from 0: S1 += (double)hist[k] * centre(k); S2 += (double)hist[k] * fabs(centre(k));
 *      S3 += (double)hist[k] * (centre(k) * centre(k)); all three NaN when in_range == 0.
 * A query's numbers depend on its own pixels and the scalars alone: not on Q, N, the order of the meshes or the grid (the sums
 * are integer atomics; a workgroup adds its pixels up in LDS first and the pixels it has no room for straight to memory -- the
 * same integers either way).  Asynchronous on `stream`: three kernels, ONE pass over the pixels for all queries, no host
 * synchronisation, no allocation; the workspace keeps each query's range of occupied bins.  Q == 0 succeeds and launches
 * nothing (mesh_query and the outputs may then be NULL).  HM_ERR_ARG before any device work: a null pointer, N, H or W < 1,
 * N H W >= 2^31, Q or n_meshes < 0, bins odd or outside 2..4096, unit or bin_m not finite and > 0, raw_lo > raw_hi,
 * workspace_bytes below the query, counts or stats not 8-byte aligned, hist, workspace or a 32-bit input not 4-byte aligned.
 * Measured on an MI355X (tools/bench_depth_eval.py, profiles/depth_eval_bench.log; per call, host submission included, 1080 x 1920,
 * four meshes per frame, every hand pixel in one bin): 16 frames with one query per frame 0.546 ms, with one per mesh 0.401 ms;
 * 64 frames 0.901 / 0.678 ms (the same histograms from torch ops on the device 3.96 / 14.6 / 15.3 / 58.5 ms); bound by its
 * atomics, not by memory (0.24-0.78 TB/s of pred_id; hm_mask_boxes reads masks at 2.1-4.5 TB/s): DESIGN.md section 10.3. */
size_t hm_depth_residuals_workspace_bytes(int Q, int bins);   /* 0 for an illegal Q or bins; positive otherwise */
int hm_depth_residuals(const float* pred_depth, const int32_t* pred_id, const uint16_t* sensor, const uint8_t* mask /* or NULL */,
                       const int32_t* labels /* device [Q] or NULL */, int N, int H, int W, const int32_t* mesh_query /* device */,
                       int n_meshes, int Q, double unit, int raw_lo, int raw_hi, double bin_m, int bins,
                       uint32_t* hist /* device [Q][bins] */, int64_t* counts /* device [Q][8] */, double* stats /* device [Q][4] */,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- Depth fit: the rigid motion that brings the predicted hands' z-buffer onto a sensor depth map: csrc/depth_fit.hip.  Per
 * query the 6 x 6 normal equations of a point-to-plane fit over the pixels its meshes cover, seven pixel counts, and their
 * damped Cholesky solution (hamer/utils/depth_eval.py depth_fit and fit_rigid).
 *
 * pred_depth, pred_id, sensor, mask, labels, mesh_query, n_meshes, Q, unit, raw_lo and raw_hi are hm_depth_residuals' and mean
 * the same.  cameras [N][4] f64 on the device: fx, fy, cx, cy of every frame; pivot [Q][3] f64 on the device: the point each
 * query's rotation turns about, in the camera frame.  gate_m in (0, 0.25], edge_m > 0, reach_m in (0, 1], damping >= 0,
 * lever_m > 0 (all finite), min_pixels >= 1.
 *
 * Rule per pixel e = (n H + v) W + u, all arithmetic fp64 and exactly as written, sums left to right: the unit is compiled with
 * contraction off (#pragma clang fp contract(off)), so no product is fused into a sum.
 *   1  id = pred_id[e]; the pixel is skipped unless 0 <= id < n_meshes and q = mesh_query[id] is in 0..Q-1; counts[q][0]
 *      (covered) += 1
 *   2  a mask test applies and the pixel fails it: counts[q][1] (off mask) += 1, stop
 *   3  raw == 0, raw < raw_lo or raw > raw_hi: counts[q][2] (no measurement) += 1, stop
 *   4  d = (double)pred_depth[e]; rz = (double)raw * unit - d; fabs(rz) <= gate_m is false (so for a NaN too): counts[q][3]
 *      (gated) += 1, stop
 *   5  the four neighbours (u-1, v), (u+1, v), (u, v-1), (u, v+1), depths dl, dr, du, dd: one lies outside the image (u < 1,
 *      u + 1 >= W, v < 1 or v + 1 >= H: a neighbour never comes from the next row or frame), or its pred_id != id, or
 *      fabs(dn - d) <= edge_m is false: counts[q][4] (no normal) += 1, stop
 *   6  rx = ((double)u - cx) / fx, rxl and rxr the same of (double)(u - 1) and (double)(u + 1); ry = ((double)v - cy) / fy,
 *      ryu and ryd the same of v - 1 and v + 1;
 *      a = (dr * rxr - dl * rxl, dr * ry - dl * ry, dr - dl);  b = (dd * rx - du * rx, dd * ryd - du * ryu, dd - du);
 *      n = a x b = (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx);  l2 = nx * nx + ny * ny + nz * nz;
 *      m = (d * rx - pivot[q][0], d * ry - pivot[q][1], d - pivot[q][2]);  mm = mx * mx + my * my + mz * mz;
 *      J = (my * nz - mz * ny, mz * nx - mx * nz, mx * ny - my * nx, nx, ny, nz);  rho = (nx * rx + ny * ry + nz) * rz;
 *      l2 > 0 && l2 <= DBL_MAX is false, or mm > reach_m * reach_m, or rho * rho > l2: counts[q][5] (rejected) += 1, stop
 *   7  counts[q][6] (used) += 1 and sums[q] += 28 integers: llrint((J_i * J_j) / l2 * 2^30) for the 21 pairs i <= j row by row
 *      ((0,0), (0,1) .. (0,5), (1,1) ..), llrint((J_i * rho) / l2 * 2^30) for i = 0..5, llrint((rho * rho) / l2 * 2^30).
 * The normal is never normalised (the weight 1 / l2 does it) and there is no square root: one correctly rounded division per
 * term, so the integers are the same wherever the rule is evaluated; |m| <= 1 and rho^2 <= l2 keep every term within 2^30, so
 * an int64 sum cannot overflow below 2^31 pixels.  A query's sums and counts depend on its own pixels and the scalars alone: not
 * on Q, N, the order of the meshes or the grid.
 * The solve, per query from its integers: used = counts[q][6]; M symmetric with M_ij = (double)sums[k] * 2^-30 for the 21
 * pairs, then M_ii = M_ii + (damping * (double)used) * (lever_m * lever_m) for i < 3 and M_ii + damping * (double)used for the
 * rest; g_i = (double)sums[21 + i] * 2^-30.  Cholesky M = L L^T column by column, j = 0..5: s = M_jj, s = s - L_jk * L_jk for
 * k = 0..j-1, L_jj = sqrt(s); then for i = j+1..5: s = M_ij, s = s - L_ik * L_jk for k = 0..j-1, L_ij = s / L_jj.  Forward
 * y_i = (g_i - L_i0 y_0 - .. - L_i,i-1 y_i-1) / L_ii for i = 0..5; backward x_i = (y_i - L_i+1,i x_i+1 - .. - L_5i x_5) / L_ii
 * for i = 5..0.  solution [Q][8] = omega (x_0..2), t (x_3..5), rms = sqrt(((double)sums[27] * 2^-30) / (double)used) (NaN when
 * used == 0) and 1.0 for solved; a query with used < min_pixels or an s of a diagonal that is not > 0 is not solved: omega =
 * t = 0 and the flag 0.  The fitted motion is p -> p + omega x (p - pivot) + t: it minimises, linearised, the squared distances
 * of the moved surface points to the sensor's points on the same rays, measured along the surface normals.
 * sums i64 [Q][28], counts i64 [Q][8] (entry 7 is written 0) and solution are all written on every call (callers do not clear
 * them).  Asynchronous on `stream`: three kernels, ONE pass over the pixels for all queries, no host synchronisation, no
 * allocation; the workspace (36 int64 per query) is where the sums are added up.  Q == 0 succeeds and launches nothing
 * (mesh_query, cameras, pivot and the outputs may then be NULL).  HM_ERR_ARG before any device work: a null pointer, N, H or
 * W < 1, N H W >= 2^31, Q or n_meshes < 0, unit not finite and > 0, raw_lo > raw_hi, a scalar outside its range above,
 * workspace_bytes below the query, a 64-bit buffer not 8-byte aligned, a 32-bit input not 4-byte aligned. */
size_t hm_depth_fit_workspace_bytes(int Q);   /* 0 for Q < 0; positive otherwise */
int hm_depth_fit(const float* pred_depth, const int32_t* pred_id, const uint16_t* sensor, const uint8_t* mask /* or NULL */,
                 const int32_t* labels /* device [Q] or NULL */, int N, int H, int W, const int32_t* mesh_query /* device */,
                 int n_meshes, int Q, const double* cameras /* device [N][4] */, const double* pivot /* device [Q][3] */,
                 double unit, int raw_lo, int raw_hi, double gate_m, double edge_m, double reach_m, double damping, double lever_m,
                 int min_pixels, int64_t* sums /* device [Q][28] */, int64_t* counts /* device [Q][8] */,
                 double* solution /* device [Q][8] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Mask fit: the 2-D similarity that brings a predicted silhouette's contour onto a label mask's: csrc/mask_fit.hip.  Per
 * query the 4 x 4 normal equations of a contour alignment, 2 x 6 pixel counts and their damped Cholesky solution: image-plane
 * shift, scale and rotation about the viewing axis (hamer/utils/mask_eval.py mask_fit and fit_contour).
 *
 * pred_id, mask, N, H, W, queries and Q are hm_mask_score's and mean the same (pred: id_lo <= pred_id < id_hi; gt: mask == label,
 * or mask != 0 when label == -1).  centre [Q][2] i32 on the device: the integer pixel (x, y) each query's similarity is taken
 * about.  radius in 0..64, reach_px in 1..4096, directions 1 (pred -> mask), 2 (mask -> pred) or 3 (both), damping >= 0 and
 * lever_px > 0 (both finite), min_pixels >= 1.
 *
 * All per-pixel work is in integers.
 *   Boundary map  b(s) exactly as under "Mask scores": the east, south and south-east neighbours, the last row and column
 *                 replicated.
 *   Match         for a boundary pixel p of map A, the boundary pixel of map B at an integer offset (dx, dy) with d2 = dx dx +
 *                 dy dy <= radius radius that has the least d2; ties go to the least dy, then to the least dx.  None: the pixel is
 *                 `unmatched`.
 *   Direction 1   A = b(pred), B = b(gt); the moved point is u = p - centre and the displacement d = (dx, dy).
 *   Direction 2   A = b(gt), B = b(pred); the moved point is the matched pred pixel, u = p + (dx, dy) - centre, and d = (-dx, -dy).
 *   Reach         a matched pixel with ux ux + uy uy > reach_px reach_px is `out_of_reach` and adds nothing (evaluated without
 *                 overflow for any centre: |ux| or |uy| > reach_px is out of reach).
 * Unknowns x = (alpha, beta, tx, ty) of the motion q -> centre + (1 + alpha) (q - centre) + beta J (q - centre) + t with
 * J (x, y) = (-y, x): scale hypot(1 + alpha, beta), angle atan2(beta, 1 + alpha) (positive: x turns towards y).
 *   d2 > 0        a point-to-line term whose line normal is the direction to the nearest pixel: row Jr = (d.u, d.Ju, dx, dy) =
 *                 (dx ux + dy uy, dy ux - dx uy, dx, dy) of the displacement d, residual rho = d2, weight 1 / d2.  sums[q] += the
 *                 ten integers llrint((double)(Jr_i Jr_j) / (double)d2 * 2^20) for the pairs i <= j row by row ((0,0), (0,1) ..
 *                 (0,3), (1,1) ..) into sums[0..9], the four integers Jr_i (= Jr_i rho / d2, exact) into sums[10..13], and d2
 *                 (= rho rho / d2) into sums[14].  The products are exact int64 and exact doubles (below 2^38); one correctly
 *                 rounded division per term, so the integers are the same wherever the rule is evaluated.
 *   d2 == 0       the pixel already lies on the other contour: a point-to-point anchor with right-hand side 0.  sums[15] += ux,
 *                 sums[16] += uy, sums[17] += ux ux + uy uy; with their number these are the entries of A^T A for
 *                 A = [[ux, -uy, 1, 0], [uy, ux, 0, 1]].
 * Every divided term is at most max(|u|^2, 1) <= 2^25 times 2^20, so an int64 sum cannot overflow below 2^18 used pixels per
 * query (a 1080 x 1920 frame whose every pixel is a boundary pixel has 2^21; a hand's contour has some 2^11).
 * counts i64 [Q][2][6], per direction: 0 boundary, 1 matched with d2 > 0, 2 anchored, 3 unmatched, 4 out of reach, 5 zero;
 * boundary = the sum of 1..4; the entries of a direction that is switched off are 0.  sums i64 [Q][18].
 * The solve, per query from its integers: used = the matched and the anchored of both directions, na = the anchored of both.
 * M symmetric with M_ij = (double)sums[k] * 2^-20 for the ten pairs; then M_00 += (double)sums[17], M_11 += (double)sums[17],
 * M_02 += (double)sums[15], M_03 += (double)sums[16], M_12 -= (double)sums[16], M_13 += (double)sums[15], M_22 += (double)na,
 * M_33 += (double)na; then M_ii = M_ii + (damping * (double)used) * (lever_px * lever_px) for i < 2 and M_ii + damping *
 * (double)used for the rest; g_i = (double)sums[10 + i].  Cholesky M = L L^T column by column, the forward and the backward
 * substitution exactly as under "Depth fit" with 4 in the place of 6, every inner sum from k = 0 upwards; fp64, compiled with
 * contraction off.  solution f64 [Q][8] = alpha, beta, tx, ty, rms = sqrt((double)sums[14] / (double)used) (0 when used == 0),
 * 1.0 for solved, 0, 0; a query with used < min_pixels or an s of a diagonal that is not > 0 is not solved: zeros, the flag 0,
 * and never a NaN.  A query whose frame is outside 0..N-1 is not read: its sums, counts and solution are all zero.
 * sums, counts and solution are all written on every call (callers do not clear them).  A query's numbers depend on its own
 * images and the scalars alone: not on Q, the order of the queries, the rest of the batch or the grid (the sums are integer
 * atomics).  Asynchronous on `stream`: four kernels (init, pack, match, solve), no host synchronisation, no allocation; the
 * workspace holds the two boundary maps of every query, one bit per pixel, and 32 int64 per query where the sums are added up.
 * Q == 0 succeeds and launches nothing (queries, centre, the outputs and workspace may then be NULL).
 * HM_ERR_ARG before any device work: a null pointer, N, H or W < 1, N H W >= 2^31, radius outside 0..64, reach_px outside
 * 1..4096, directions outside 1..3, damping negative or not finite, lever_px not finite and > 0, min_pixels < 1, Q < 0,
 * workspace_bytes below the query, sums, counts, solution or workspace not 8-byte aligned (pred_id, queries and centre: 4-byte). */
size_t hm_mask_fit_workspace_bytes(int Q, int H, int W, int radius);   /* 0 for illegal sizes; positive otherwise */
int hm_mask_fit(const int32_t* pred_id, const uint8_t* mask, int N, int H, int W, const hm_mask_query* queries /* device */, int Q,
                const int32_t* centre /* device [Q][2]: x, y */, int radius, int reach_px, int directions, double damping,
                double lever_px, int min_pixels, int64_t* sums /* device [Q][18] */, int64_t* counts /* device [Q][2][6] */,
                double* solution /* device [Q][8] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Visibility: which parts of a hand the camera sees: csrc/visibility.hip.  hm_point_visibility gives one code per 3-D
 * point (a joint, a vertex), hm_mesh_coverage pixel counts and boxes per mesh; both read the depth and mesh_id maps that
 * hm_mesh_render wrote for the same meshes, and optionally a sensor depth map and a label mask (hamer/utils/visibility.py,
 * DESIGN.md section 10.6).  The unit is compiled with contraction off (#pragma clang fp contract(off)); every fp64 expression
 * is evaluated left to right as written.
 *
 * Common inputs.  depth [N][H][W] f32 and mesh_id [N][H][W] i32 as hm_mesh_render writes them (a pixel is COVERED when
 * mesh_id >= 0); K_host [N][3][3] fp64 on the HOST, last row exactly (0, 0, 1); znear as hm_mesh_render's.  sensor [N][H][W] u16
 * or NULL: raw units of `unit` metres; a reading is VALID when raw != 0 && raw_lo <= raw <= raw_hi; unit, raw_lo, raw_hi and
 * scene_tol_m are read (and checked) only with a sensor.  mask [N][H][W] u8 or NULL, tested with a label as hm_depth_residuals
 * does: -2 no test, -1 mask != 0, 0..255 mask == label, any other value: no pixel passes.
 *
 * hm_point_visibility.  points [P][3] fp64, camera frame, on the device.  groups [G] on the device: group g owns the points
 * p0 .. p0 + np - 1, lies in view `view`, belongs to mesh row `mesh` of the render, and is tested with its own tol_m (metres)
 * and label.  The groups' point ranges do not overlap.  A group whose range leaves 0..P-1 (or with np < 0) is treated as
 * empty: no point of it is read or written and its entry 7 is 0.  window in 0..2: the half-width of the pixel window.
 * Rule per point (x, y, z) of a group:
 *   1  `z >= znear` is false (NaN included): BEHIND (1)
 *   2  projection, exactly hm_mesh_render's: u = ((K00*x + K01*y) + K02*z) / z, v = ((K10*x + K11*y) + K12*z) / z with the K of
 *      the group's view; `|u| < 65536 && |v| < 65536` is false: OUTSIDE (2).  X = rint_half_even(256*u), px = X >> 8 (an
 *      arithmetic shift: the floor; a negative X is outside), py likewise from v.  (px, py) outside the image, or the group's
 *      view outside 0..N-1 (such a group reads no map): OUTSIDE (2)
 *   3  hand test over the window pixels (px + dx, py + dy), |dx|, |dy| <= window, that lie inside the image: a covered pixel
 *      passes when (double)depth >= z - tol_m; an uncovered pixel passes only when it is the centre pixel (an uncovered
 *      neighbour is neutral).  No pixel passes: SELF (3) when the centre's mesh_id == group.mesh, else OTHER (4)
 *   4  with a sensor, over the same window: a valid reading passes when (double)raw * unit >= z - scene_tol_m.  At least one
 *      valid reading and none passing: SCENE (5).  No valid reading leaves the point where it was
 *   5  with a mask and label != -2: the centre pixel fails the mask test: OFF_MASK (6)
 *   6  otherwise VISIBLE (0)
 * codes u8 [P]: every point of every group is written, points in no group are not touched.  counts i32 [G][8]: entry c is the
 * number of the group's points with code c for c = 0..6, entry 7 is np; all entries are written on every call.  The counts are
 * integer sums (ballot popcounts added up in LDS, then integer atomics behind an init kernel that is part of the call), so a
 * group's row depends on its own points and maps alone, not on G, P, the order of the groups or the grid.
 * Launches: the init kernel, then one point kernel per 64 views (the cameras travel as kernel arguments); no workspace.
 *
 * hm_mesh_coverage.  The mesh table, verts, faces, K_host and znear of hm_mesh_render, with its geometry and coverage rule word
 * for word: the same faces are skipped, samples are pixel centres, the top-left rule applies.  labels i32 [n_meshes] on the
 * device or NULL (no mask test; also without a mask).  Pixel p of mesh m's view is COVERED BY m when some non-skipped face of m
 * covers its centre; a pixel counts once however many faces of m cover it, and other meshes play no part.
 * counts i64 [n_meshes][8]:
 *   0 amodal            covered by m
 *   1 modal             covered by m and mesh_id == m
 *   2 behind_other      covered by m and mesh_id names another mesh (>= 0, != m)
 *   7 uncovered_in_map  covered by m and mesh_id < 0
 * and the modal pixels split, in this order, into
 *   4 scene             a valid reading with (double)raw * unit < (double)depth - scene_tol_m
 *   6 off_mask          else: a mask and labels given, labels[m] != -2, and the pixel fails the mask test
 *   3 clear             else
 * Entry 5, unmeasured, counts the modal pixels with a sensor given and no valid reading; it is informational and not exclusive
 * of entries 3 and 6.  Identities: amodal == modal + behind_other + uncovered_in_map, modal == clear + scene + off_mask.
 * boxes i32 [n_meshes][8]: x1, y1, x2, y2 (inclusive) of the amodal pixels, then of the modal pixels; -1, -1, -1, -1 when there
 * are none.  Pixels outside the frame count nowhere.  Both arrays are written whole on every call.
 * Work items are (mesh, 16 x 16 tile) as in the renderers: setup per 48 meshes projects the corners to the rule's fixed point and
 * lists the tiles of each mesh's clipped box; one kernel walks the list, one lane per pixel against the faces culled into LDS,
 * and the workgroup adds ballot popcounts and sends integer atomics (64-bit add, 32-bit min and max).  No key buffer, no
 * per-pixel output; three memsets (work counter, counts, boxes).  The sums are integers: a mesh's row depends on its own
 * faces and maps alone.  H, W <= 32767.
 *
 * Both calls: asynchronous on `stream`, no host synchronisation, no allocation.  G == 0 / n_meshes == 0 succeeds and launches
 * nothing.  HM_ERR_ARG, with a message naming the entry point, before any device work: a null required pointer, N, H or W < 1,
 * N H W >= 2^31, window outside 0..2, znear (and with a sensor unit or scene_tol_m) not finite and > 0, raw_lo > raw_hi, a last
 * row of K other than (0, 0, 1), a buffer not aligned (8 bytes: points, groups, verts, i64 counts, workspace; 4 bytes: depth,
 * mesh_id, faces, labels, boxes, i32 counts; 2 bytes: sensor), a bad mesh table, a workspace that is too small.
 * Measured on an MI355X (tools/bench_visibility.py, profiles/visibility_bench.log; per call, host submission included, 1080 x 1920,
 * four meshes of 780 vertices and 1500 faces per frame, every vertex and 21 more points per mesh): 16 frames hm_point_visibility
 * 0.042 ms and hm_mesh_coverage 0.300 ms next to 0.688 ms for the hm_mesh_render call of the same scene; 64 frames 0.321 ms and
 * 1.050 ms next to 2.349 ms; a sensor and a mask change neither: DESIGN.md section 10.6. */
enum { HM_VIS_VISIBLE = 0, HM_VIS_BEHIND = 1, HM_VIS_OUTSIDE = 2, HM_VIS_SELF = 3, HM_VIS_OTHER = 4, HM_VIS_SCENE = 5,
       HM_VIS_OFF_MASK = 6 };
typedef struct hm_vis_group { double tol_m; int32_t view, mesh, p0, np, label, reserved; } hm_vis_group;
int hm_point_visibility(const float* depth, const int32_t* mesh_id, int N, int H, int W, const double* K_host, double znear,
                        const double* points /* device [P][3] */, int P, const hm_vis_group* groups /* device [G] */, int G,
                        int window, const uint16_t* sensor /* or NULL */, double unit, int raw_lo, int raw_hi, double scene_tol_m,
                        const uint8_t* mask /* or NULL */, uint8_t* codes /* device [P] */, int32_t* counts /* device [G][8] */,
                        void* stream);
size_t hm_mesh_coverage_workspace_bytes(int N, int H, int W, int n_verts, int n_meshes, int n_faces);   /* 0 for illegal sizes */
int hm_mesh_coverage(int N, int H, int W, const double* K_host, const double* verts, int n_verts, const int32_t* faces,
                     int n_faces, const hm_mesh* meshes_host, int n_meshes, double znear, const float* depth,
                     const int32_t* mesh_id, const uint16_t* sensor /* or NULL */, double unit, int raw_lo, int raw_hi,
                     double scene_tol_m, const uint8_t* mask /* or NULL */, const int32_t* labels /* device [n_meshes] or NULL */,
                     int64_t* counts /* device [n_meshes][8] */, int32_t* boxes /* device [n_meshes][8] */, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- Penetration: do two hand meshes pass through each other: csrc/penetration.hip (hamer/utils/penetration.py, DESIGN.md
 * section 10.7; tests/penetration_rule.py restates the rule in numpy).  A QUERY is an ordered pair (a, b) of rows of the mesh
 * table: every vertex of a gets its signed distance to the surface of b.  verts, faces and the hm_mesh rows are those of
 * hm_mesh_render (frame is not read but must be >= 0; two meshes share neither vertex rows nor face rows); a query may name
 * any two rows, also of different frames.  b should be a closed surface (hamer/utils/penetration.py close_boundaries closes the
 * MANO wrist).  The rule uses integers and fp64 only; the unit is compiled with contraction off and every rounded fp64
 * expression is evaluated left to right as written, so the outputs equal the numpy rule bit for bit.
 *
 * Fixed point.  X = rint_half_even(x * 65536) per coordinate (a quantum of 2^-16 m, about 15 um).  A vertex is VALID when
 * |x|, |y|, |z| < 16384 (not-a-number and infinities fail), so |X| <= 2^30.  A face is VALID when its three corners lie in
 * 0..nv-1 and name valid vertices; other faces are never read further.  A mesh's BOX is the integer bounding box of its valid
 * vertices (empty without one).  T = ceil(contact_tol_m * 65536), 0 <= contact_tol_m <= 1, so T <= 2^16.
 * Status of a query, in this order:
 *   HM_PEN_TOO_LARGE (2)  a side (hi - lo) of a's or b's box is >= 2^17 (2 m): every vertex of a gets INVALID, NaN, -1, every
 *                         count and sum is 0, nothing else is computed
 *   HM_PEN_DISJOINT (1)   a's box and b's box inflated by T on every side do not overlap (also when either is empty): every
 *                         valid vertex of a is FAR, `invalid` is counted, every other count and sum is 0; no face is read
 *   HM_PEN_OK (0)         otherwise.  A valid vertex of a outside b's inflated box is FAR without any face test; the others are
 *                         TESTED
 * Exactness.  A tested vertex P lies in b's inflated box and every corner V of a valid face in b's box, so per axis
 * |P - V| < 2^17 + 2^16 < 2^18 and |V - V'| < 2^17.  The edge functions are two products below 2^35; the six dot products of the
 * distance are three products below 2^35, sums below 2^37; the components of n = (V1 - V0) x (V2 - V0) are two products below 2^34,
 * so |n_k| < 2^35: all are integers below 2^53, which fp64 products and sums give exactly.  n . (V0 - P) is three products below
 * 2^35 * 2^18 = 2^53, a sum below 2^55 (< 2^57): it is taken in int64.  Nothing else in the rule needs to be exact.
 * Face order.  A = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0) is twice the face's projected area; when A < 0 corners 1 and 2 are swapped
 * and A := -A, and everything below uses this order (so n_z = A >= 0).
 * Inside test.  P is inside b when the ray from P in +z crosses an odd number of b's valid faces.  A face with A != 0 is crossed
 * when (a) (X, Y) of P lies in its projection by hm_mesh_render's coverage rule: E_i the edge function of the edge opposite
 * corner i (1->2, 2->0, 0->1) at (X, Y), every E_i > 0, or == 0 on an edge that owns its boundary (dy < 0, or dy == 0 and
 * dx > 0), and (b) s = n . (V0 - P) > 0: the face's plane at (X, Y) is strictly above P.  With the half-open ownership a ray
 * through a shared edge or vertex crosses each sheet of the surface once; a vertex exactly on the surface gets what the rule
 * gives.
 * Distance.  For a tested vertex, over b's valid faces with n != 0 (a face of area 0 in space is skipped), delta = closest
 * point of the face minus P, in quanta, by the region method with a = V0, b = V1, c = V2, ab = b-a, ac = c-a, bc = c-b, ap = P-a,
 * bp = P-b, cp = P-c (integers), dot(u, w) = (ux*wx + uy*wy) + uz*wz, d1 = dot(ab,ap), d2 = dot(ac,ap), d3 = dot(ab,bp),
 * d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp), the first case that holds:
 *   1  d1 <= 0 && d2 <= 0: delta = -ap                          2  d3 >= 0 && d4 <= d3: delta = -bp
 *   3  vc = d1*d4 - d3*d2; vc <= 0 && d1 >= 0 && d3 <= 0: v = d1 / (d1 - d3), delta_k = v*ab_k - ap_k
 *   4  d6 >= 0 && d5 <= d6: delta = -cp
 *   5  vb = d5*d2 - d1*d6; vb <= 0 && d2 >= 0 && d6 <= 0: w = d2 / (d2 - d6), delta_k = w*ac_k - ap_k
 *   6  va = d3*d6 - d5*d4; va <= 0 && d4-d3 >= 0 && d5-d6 >= 0: w = (d4-d3) / ((d4-d3) + (d5-d6)), delta_k = w*bc_k - bp_k
 *   7  nn = (nx*nx + ny*ny) + nz*nz, s = (nx*-apx + ny*-apy) + nz*-apz, t = s / nn, delta_k = n_k*t
 * (d1 - d3 = |ab|^2, d2 - d6 = |ac|^2, (d4-d3) + (d5-d6) = |bc|^2 and nn are >= 1 for a face with n != 0: no division by 0.)
 * D2 = (dx*dx + dy*dy) + dz*dz; the nearest face is the one of smallest D2, ties to the lower face row; d = sqrt(D2) * 2^-16 in
 * metres.  A face of the product region 7 that the rounded va, vb, vc misjudge lies within rounding of an edge, where both
 * formulas agree to rounding.
 * Per vertex of a (row = the sum of the a-meshes' nv over the earlier queries, plus the vertex's index): code u8 -- HM_PEN_FAR
 * 0 (not tested, or outside with d > contact_tol_m), HM_PEN_NEAR 1 (outside, d <= contact_tol_m), HM_PEN_INSIDE 2,
 * HM_PEN_INVALID 3 (not a valid vertex); signed_distance f32: (float)d for NEAR, (float)-d for INSIDE, +inf for FAR, NaN for
 * INVALID; nearest_face i32: the face's index inside mesh b for NEAR and INSIDE, else -1.
 * Per query sums i64 [10]: 0 tested, 1 near, 2 inside, 3 invalid, 4 status, 5 the bits of the largest d over the inside
 * vertices as an fp64 (0 without one; non-negative doubles order like their bit patterns), 6 the sum of llrint(d * 2^32) over
 * the inside vertices, 7..9 the sums of llrint(delta_k * 65536) (= (c - p)_k in metres * 2^32), k = x, y, z, over the inside
 * vertices: the push that takes a out of b.  All integer sums (ballot popcounts, wave sums, one 64-bit atomic per term behind
 * a memset that is part of the call): a query's outputs depend on its two meshes and contact_tol_m alone, not on the batch, its
 * place in it, or scheduling.
 * meshes_host and queries_host are read on the HOST before return.  n_rows: the capacity of code, signed_distance and
 * nearest_face in rows, >= the sum of the a-meshes' nv.  Launches: one memset, setup per 128 meshes, the query table per 192
 * queries, one kernel over (query, 64 vertices of a) items: four waves share b's faces, staged 512 at a time in LDS.
 * Asynchronous on `stream`, no host synchronisation, no allocation; n_queries == 0 succeeds and launches nothing.  HM_ERR_ARG,
 * with a message naming the entry point, before any device work: a negative count, contact_tol_m outside 0..1, a null required
 * pointer, a buffer not aligned (16 bytes: workspace; 8: verts, sums; 4: faces, signed_distance, nearest_face), a bad mesh
 * table, a query naming a mesh outside it, 2^31 or more rows or work items, n_rows or the workspace too small.
 * Measured on an MI355X (tools/bench_penetration.py, profiles/penetration_bench.log; per call through the Python wrapper, host
 * submission included, queries of 778 vertices against 1552 faces; in brackets the device time of the call's memset and launches):
 * overlapping 16 queries 0.318 ms (0.309), 64 queries 0.548 ms (0.525), 256 queries 1.610 ms (1.311); disjoint (the early out) 0.143 ms
 * (0.025), 0.428 ms (0.027), 1.545 ms (0.049): the wrapper's per-mesh packing, not the kernel; hm_mesh_score on the same point
 * counts 0.163 / 0.167 / 0.182 ms: DESIGN.md section 10.7. */
enum { HM_PEN_FAR = 0, HM_PEN_NEAR = 1, HM_PEN_INSIDE = 2, HM_PEN_INVALID = 3 };
enum { HM_PEN_OK = 0, HM_PEN_DISJOINT = 1, HM_PEN_TOO_LARGE = 2 };
typedef struct hm_pen_query { int32_t a, b; } hm_pen_query;            /* rows of the mesh table */
size_t hm_mesh_penetration_workspace_bytes(int n_verts, int n_meshes, int n_queries);   /* 0 for illegal sizes */
int hm_mesh_penetration(const double* verts, int n_verts, const int32_t* faces, int n_faces, const hm_mesh* meshes_host,
                        int n_meshes, const hm_pen_query* queries_host, int n_queries, double contact_tol_m,
                        uint8_t* code /* device [n_rows] */, float* signed_distance /* device [n_rows] */,
                        int32_t* nearest_face /* device [n_rows] */, long long n_rows, int64_t* sums /* device [n_queries][10] */,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- Motion: csrc/motion.hip.  The first entry points that look across frames.  A sequence is N
 * frames by S tracks (the drivers: S = 2, right and left); nothing associates hands, a track is one column.  Everything is fp64
 * without contraction in the order written; tests/motion_rule.py restates it in numpy and the kernels equal it byte for byte.
 *
 * hm_track_smooth: a zero-phase filter of rotations as rotations.
 *   rot [N][S][J][9] f64 (3 x 3, row-major), lin [N][S][C] f64, present [N][S] u8 (non-zero: present);
 *   weights_host [R + 1] f64, 0 <= R <= HM_MOTION_MAX_RADIUS, read on the HOST before return and passed to the kernel as
 *   arguments (the callers make them as w[0] = 1, w[k] = exp(-0.5 (k / sigma)^2): the kernel calls no exp and no trigonometry).
 * The symmetric-pair window of frame t of a track, for every element A of the rotations and channels alike:
 *   acc = w[0] * A[t], W = w[0] when t is present, else acc = 0, W = 0;
 *   for k = 1 .. R, only when t - k >= 0, t + k < N and both are present (a PAIR):
 *     acc = acc + w[k] * (A[t-k] + A[t+k]);  W = W + 2.0 * w[k].
 * Offsets count only as pairs, so a track of constant velocity (a fixed axis and rate; channels linear in t) comes back
 * unchanged for any presence pattern and at both ends, and a missing frame is interpolated by the same sum.
 * pairs [N][S] i32: the pairs used; nearest_pair: the smallest k used, 0 without one.  Without a pair the outputs are the
 * input's bytes (present: HM_TRACK_KEPT) or NaN (absent: HM_TRACK_ABSENT).  With one:
 *   linear channels: acc / W.
 *   rotations: M = acc / W element by element.  With the cofactor matrix
 *     c00 = m11 m22 - m12 m21   c01 = m12 m20 - m10 m22   c02 = m10 m21 - m11 m20
 *     c10 = m02 m21 - m01 m22   c11 = m00 m22 - m02 m20   c12 = m01 m20 - m00 m21
 *     c20 = m01 m12 - m02 m11   c21 = m02 m10 - m00 m12   c22 = m00 m11 - m01 m10
 *   and det = (m00 c00 + m01 c01) + m02 c02, the rotation is degenerate unless det M >= 1/64 (a NaN is degenerate); else
 *   X = M and exactly 12 times X <- (X + cof(X) / det X) * 0.5, element by element: Newton's iteration for the polar factor,
 *   the rotation nearest M (on the CPU every window with det >= 1/64 had converged to fp64 after 9 steps).
 * status [N][S] i32: HM_TRACK_SMOOTHED (present) or HM_TRACK_FILLED (absent) when there is a pair and none of the J rotations is
 * degenerate; HM_TRACK_DEGENERATE when one is: every output of the hand, channels included, is then the input's bytes
 * (present) or NaN (absent), so a hand never mixes filtered and raw joints.  pairs and nearest_pair are what was counted either way.
 * moved [N][S][J] f64: for HM_TRACK_SMOOTHED ((((0 + d0 d0) + d1 d1) + ...) + d8 d8), d = output - input over the 9 elements
 * in row-major order -- the squared Frobenius distance, 8 sin^2(angle / 2) between rotations -- and NaN for every other status.
 * rot_out and lin_out never alias rot and lin.  Launch: one kernel; a workgroup is (32 frames, track), its 256 threads 32
 * frames x 8 units (a rotation, or 9 channels), the units in passes of 8 with the tile and a halo of R frames on each side in
 * LDS (at most 54 KiB); one flag per frame in LDS carries the degenerate decision across the passes.  A (frame, track)'s bytes
 * depend on its own window only: not on N, S or the tile.  N == 0 or S == 0 succeeds without a launch.  HM_ERR_ARG before any
 * device work: a negative count, R outside 0..32, a weight outside 0..1 or NaN, a null pointer where its count is positive,
 * a misaligned array, in-place outputs, 2^31 or more frames x tracks.
 *
 * hm_track_jitter: the acceleration of point tracks.  points [N][S][P][3] f64, 1 <= P <= HM_MOTION_MAX_POINTS; accel [N][S] f64:
 * where t - 1, t and t + 1 lie in the sequence and are present, the mean over the P points of |x[t-1] - 2 x[t] + x[t+1]|, NaN
 * elsewhere.  Per point d = (x[t-1] - 2.0 * x[t]) + x[t+1] per coordinate, n = sqrt((dx dx + dy dy) + dz dz); a wave per
 * (frame, track): lane l adds the n of points l, l + 64, ... in this order to 0.0, the lanes meet as v[l] = v[l] + v[l + o]
 * for o = 32, 16, 8, 4, 2, 1, and accel = v[0] / (double)P.  The same conventions and errors; P > 1024 is HM_ERR_ARG.
 * Measured on an MI355X (tools/bench_motion.py, profiles/motion_bench.log; S = 2, J = 16, C = 13, per call through the Python
 * wrapper, in brackets the device time of the launch): hm_track_smooth, R = 4, N = 64 / 1024 / 16384: 0.049 (0.034) / 0.051
 * (0.034) / 0.127 (0.096) ms; R = 32: 0.075 (0.065) / 0.084 (0.072) / 0.206 (0.182) ms; hm_track_jitter, N = 16384, P = 21 / 778:
 * 0.023 (0.015) / 0.154 (0.147) ms: DESIGN.md section 10.8. */
#define HM_MOTION_MAX_RADIUS 32
#define HM_MOTION_MAX_POINTS 1024
enum { HM_TRACK_KEPT = 0, HM_TRACK_SMOOTHED = 1, HM_TRACK_FILLED = 2, HM_TRACK_ABSENT = 3, HM_TRACK_DEGENERATE = 4 };
int hm_track_smooth(const double* rot, const double* lin, const uint8_t* present, int N, int S, int J, int C,
                    const double* weights_host, int R, double* rot_out, double* lin_out, int32_t* status, int32_t* pairs,
                    int32_t* nearest_pair, double* moved, void* stream);
int hm_track_jitter(const double* points, const uint8_t* present, int N, int S, int P, double* accel, void* stream);

/* ---- Detector evaluation (yolo/yolov7/test.py and utils/metrics.py): csrc/det_eval.hip.  The caller owns every buffer, the
 * calls are asynchronous on `stream`, nothing synchronises or allocates, argument errors return HM_ERR_ARG before any device
 * work.  All fp32 / fp64 arithmetic is plain IEEE in the order written (no FMA contraction, no fast-math).
 *
 * hm_det_match: test.py:178-209 for N images in one launch (one wave per image), IoU as box_iou of general.py:447-469 in fp32:
 * inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0), iou = inter / (area1 + area2 - inter).
 *   pred [N][stride][6] f32 (xyxy, conf, cls: the layout of hm_yolo_nms's dets), pred_count [N] i32,
 *   labels [N][lmax][5] f32 (cls, xyxy, the predictions' units), label_count [N] i32, iouv [niou] f32 (test.py:78);
 *   correct [N][stride][niou] u8, best_iou [N][stride] f32, matched [N][stride] i32 (the target's index in its image or -1).
 * Per image: the label classes in ascending order and, within a class, its predictions in stored order (:191-202); a
 * prediction takes its best-IoU target of that class, the lowest index on a tie (:198); a NaN IoU in its row leaves it
 * unmatched with best_iou NaN (torch.max hands a NaN on); it is assigned only when iou > iouv[0], strictly, and that target
 * is still free, and then correct = iou > iouv (:202-207); a prediction whose best target is taken does NOT fall back to its
 * second best; the walk stops once every label of the image is taken (:208).  best_iou is the row maximum whether or not the
 * prediction was assigned, 0 when no label has its class.  Rows at or past pred_count[i] are written 0 / 0 / -1 and rows of
 * labels at or past label_count[i] are never read into a result.  Counts are clamped to [0, stride] and [0, lmax] in the
 * kernel.  An image's output bytes depend on that image alone, not on N or its place.
 * HM_ERR_ARG: a null pointer, N < 1, stride outside 1..4096, lmax outside 1..1024, niou outside 1..16. */
int hm_det_match(const float* pred, const int* pred_count, const float* labels, const int* label_count, const float* iouv,
                 int N, int stride, int lmax, int niou, uint8_t* correct, float* best_iou, int* matched, void* stream);

/* hm_det_ap: ap_per_class (metrics.py:18-78) with compute_ap (:81-110) for every (class, threshold) pair, one workgroup each.
 *   tp [P][niou] u8, conf [P] f32, pred_cls [P] f32: the predictions ALREADY sorted by descending confidence (:33-34);
 *   classes [nc] f32: the sorted unique target classes (:37), n_labels [nc] i32 (:45);
 *   x101 [101] f64 and px [1000] f64: the abscissae of :104 and :41, passed in so that they are np.linspace's bits;
 *   ap [nc][niou], p [nc][1000], r [nc][1000] f64 (p and r from threshold 0, :57-60).
 * A class with no prediction or no label leaves zeros (:48-49).  Cumulative counts are integers; recall = tpc / (n_l + 1e-16),
 * precision = tpc / (tpc + fpc) in fp64; the envelope is a reverse running maximum (:99); the sentinels are :93-96
 * (mrec ends at recall[-1] + 0.01, or 1.0 with v5_metric); the area is np.trapz over x101 (:105).  Interpolation is np.interp:
 * for x the right-most knot j with xp[j] <= x gives fp[j] + (x - xp[j]) * ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])),
 * x >= xp[-1] gives fp[-1], x < xp[0] gives `left` (0 for r, 1 for p).  tp counts of a class are expected not to exceed its
 * n_labels (with v5_metric a recall above 1 would make mrec decrease, which np.interp leaves undefined too).
 * 0 <= P <= 2^30 (1073741824: counts and indices are int32 with a bit to spare); 1 <= nc <= 65535; 1 <= niou <= 16.  The
 * kernel keeps no curve, so hm_det_ap_workspace_bytes is 0 for every legal size today and workspace may be NULL; callers
 * that size and pass it stay correct if that changes.  HM_ERR_ARG: P < 0 or > 2^30, nc or niou outside their ranges, a null
 * pointer (tp, conf and pred_cls may be NULL when P == 0). */
size_t hm_det_ap_workspace_bytes(int P, int nc, int niou);
int hm_det_ap(const uint8_t* tp, const float* conf, const float* pred_cls, int P, const float* classes, const int* n_labels,
              int nc, int niou, const double* x101, const double* px, int v5_metric, double* ap, double* p, double* r,
              void* workspace, size_t workspace_bytes, void* stream);

/* hm_det_ap_curve: compute_ap (metrics.py:81-110) of one given curve, recall [n] (non-decreasing) and precision [n] f64,
 * 1 <= n <= 2^30: ap [1], mpre [n + 2], mrec [n + 2] f64.  The interpolation and the trapezoid are the device code of
 * hm_det_ap.  HM_ERR_ARG: a null pointer, n outside its range. */
int hm_det_ap_curve(const double* recall, const double* precision, int n, const double* x101, int v5_metric, double* ap,
                    double* mpre, double* mrec, void* stream);

/* Optional per-launch timing (HIP events on the launch stream); kinds below. */
enum { HM_K_GEMM = 0, HM_K_LAYERNORM = 1, HM_K_ATTENTION = 2, HM_K_IM2COL = 3, HM_K_LINEAR_F32 = 4,
       HM_K_CROSS_ATTN = 5, HM_K_MANO = 6, HM_K_CROP = 7, HM_K_CONV = 8, HM_K_OTHER = 9 };
typedef struct hm_prof_record { int kind, epilogue, M, N, K; float ms; } hm_prof_record;
int hm_prof_begin(int capacity);                        /* allocate 2*capacity events, start logging */
int hm_prof_collect(hm_prof_record* out_host, int cap); /* sync, copy records, clear; returns count   */
int hm_prof_end(void);                                  /* stop logging, destroy the events           */

int hm_version(void);
const char* hm_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif /* HAMER_HIP_H */
