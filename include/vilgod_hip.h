/* libvilgod_hip.so -- C ABI of the MI355X (gfx950) pseudo-label hot path.
 *
 * Drop-in boundary for the per-frame hot path of chreisinger/ViLGOD's tools/preprocess_data.py
 * (SURVEY.md §8b).  The reference has no operator/plugin ABI of its own for this path: its seam is
 * Python (stage methods of ZeroShotDetector) plus one pybind11 module (pypatchworkpp).  Every entry
 * point below therefore cites the reference *call site* it replaces; INTEGRATION.md shows the
 * ctypes stub a ViLGOD maintainer would add at that call site.
 *
 * Conventions
 *   - all `d_*` pointers are DEVICE pointers (HBM); `h_*` are host pointers; no torch types.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     on that stream unless stated otherwise.
 *   - return value: 0 = VG_OK, 1 = bad argument, 2 = HIP runtime error (message on stderr),
 *     3 = a capacity given at handle creation was exceeded.
 *   - paths are relative to the reference checkout root.
 */
#ifndef VILGOD_HIP_H
#define VILGOD_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int vg_abi_version(void);    /* 2: vg_cluster_boxes reports hulls beyond its capacity (d_aux3, below) instead of a partial fit */

/* ---- renderer (rows D1-D6) ------------------------------------------------------------------
 * Replaces the per-cluster loop src/vilgod/zero_shot_detector.py:389-409 and the CLIP
 * preprocessing third_party/CLIP/clip/clip.py:79-86 for ALL clusters x views of a frame. */

/* ego[i] = float32( T * [points[index[i]], 1] )   (src/utils/pointcloud_utils.py:21-46,
 * called at zero_shot_detector.py:392).  d_index may be NULL (identity).  T: 4x4 row-major f64. */
int vg_gather_ego(const float* d_points, int stride, const int32_t* d_index, int n, const double* d_T4x4,
                  float* d_ego, void* stream);

/* per-cluster np.median over xyz (float32) and the view-direction rotation derived from it
 * (pointcloud_utils.py:396-398).  d_seg_off: [n_clusters+1] offsets into the packed point array.
 * d_median: [n_clusters,3] f32.  d_rot: [n_clusters,6] f64 = {m00,m01,m10,m11,m22, angle}: the matrix
 * scipy's Rotation.from_euler('z', -angle) yields and the float32 angle = atan2(med_y, med_x) itself
 * (correctly rounded; numpy's float32 arctan2 is a <=1 ulp SIMD routine). */
int vg_cluster_median(const float* d_ego, const int32_t* d_seg_off, int n_clusters, float* d_median,
                      double* d_rot, void* stream);

/* d_rot rows for caller-supplied float32 view angles (same layout as vg_cluster_median writes).  The reference takes
 * `np.arctan2(center_pos[1], center_pos[0])` of the float32 medians (pointcloud_utils.py:396-397): numpy's float32 arctan2
 * is host dependent (SVML on AVX-512 hosts, libm elsewhere), so a caller that must reproduce the reference ON ITS HOST reads
 * d_median back, evaluates np.arctan2 there and passes the angles in (device.angle_mode=reference). */
int vg_cluster_rot(const float* d_angle, int n_clusters, double* d_rot, void* stream);

/* transform_cluster_points_to_origin (pointcloud_utils.py:399-412) in float64, rounded to float32
 * (the `.float()` of zero_shot_detector.py:394).  d_point_cluster: [n] cluster id of each packed point.
 * d_Timg3x3: Rx(pi) @ Rz(pi/2) as scipy builds it (row-major f64). */
int vg_to_origin(const float* d_ego, const int32_t* d_point_cluster, int n, const float* d_median,
                 const double* d_rot, const double* d_Timg3x3, float* d_origin, void* stream);

/* RealisticProjection.get_img (src/utils/mv_utils.py:173-187: point_transform, points2grid,
 * GridToImage) + F.interpolate/permute/uint8 (zero_shot_detector.py:405-409) + CLIP Normalize.
 * d_view_rot: [n_views,9] f32 (points @ rot).  d_lut: [3*256+3] f32 = CLIP-normalised value of
 * every uint8 level per channel, then the 3 distinct taps (corner, edge, centre) of the 3x3 Gaussian.
 * out_kind 0: uint8 [n,224,224,3] (the arrays given to PIL)   1: f32 [n,3,224,224]   2: f16 same
 *          3: f32 [n,110,110], one channel of get_img()'s output before the resize (parity tests)
 *          4: f16 [n*196,768] patch rows (= im2col of kind 2 for 16x16 patches), the A operand of the ViT-B/16
 *             patch-embedding GEMM; vg_vit_encode input_kind 2 consumes it directly.
 *          5: f16 [n*196,256] SINGLE-CHANNEL patch rows: value = uint8 level / 256 (exact), column = i*16 + j.  The three channels of
 *             a crop are one image (src/utils/mv_utils.py:36) and the per-channel normalisation (third_party/CLIP/clip/clip.py:79-86)
 *             is affine, so vg_vit_encode input_kind 3 folds both into a K = 256 patch-embedding weight: a third of kind 4's bytes
 *             (d_lut's normalisation entries are not read for this kind). */
int vg_render_crops(const float* d_origin, const int32_t* d_seg_off, int n_clusters, const float* d_view_rot,
                    int n_views, const float* d_lut, void* d_out, int out_kind, void* stream);

/* vg_render_crops at any `lidar_image_projection` setting (tools/configs/preprocessor/waymo.yaml:75-80; src/utils/mv_utils.py:91-127
 * points2grid takes the four numbers from the config, :158-161).  vg_render_crops is the shipped setting (112, 8, 0.8, 0.2) with the
 * numbers compiled in; this entry point runs a second kernel that takes them as arguments and computes the same chain:
 *   resolution    16 .. 128: grid side; the image is (resolution - 2)^2, resized to 224 with scale float(resolution - 3) / 223
 *   depth         3 .. 32: depth slices; values are clipped to 1 .. depth - 2, the slice is the unclipped ceil (mv_utils.py:114-118)
 *   obj_ratio     (0, 1], depth_bias [0, 1]: float32, as torch rounds the Python scalars
 *   one_plus_bias float32( 1.0 + (double)depth_bias_as_configured ): torch forms `1 + depth_bias` (mv_utils.py:110) in double before
 *                 it meets the float32 tensor, so the caller does too (1 <= one_plus_bias <= 2)
 * out_kind as above, kind 3 is [n, resolution - 2, resolution - 2]; the output side stays 224.  VG_ERR_ARG (nothing launched) for a
 * null `params` or any value outside these ranges, also when there is nothing to render. */
#define VG_RENDER_MIN_RESOLUTION 16
#define VG_RENDER_MAX_RESOLUTION 128
#define VG_RENDER_MIN_DEPTH 3
#define VG_RENDER_MAX_DEPTH 32
typedef struct vg_render_params {
    int resolution, depth;
    float obj_ratio, depth_bias, one_plus_bias;
} vg_render_params;
int vg_render_crops_ex(const float* d_origin, const int32_t* d_seg_off, int n_clusters, const float* d_view_rot, int n_views,
                       const float* d_lut, const vg_render_params* params, void* d_out, int out_kind, void* stream);

/* The crops at a `classification.image_size` other than 224 (tools/configs/preprocessing.yaml:91).  The reference interpolates
 * get_img()'s image to image_size^2 (bilinear, align_corners=True), permutes, truncates to uint8 and builds a PIL image
 * (src/vilgod/zero_shot_detector.py:405-410); CLIP's preprocess then opens with Resize(224, BICUBIC) (third_party/CLIP/clip/clip.py:79-86),
 * Pillow's antialiased 8-bit resample (src/libImaging/Resample.c: horizontal, then vertical pass, clip8((2^21 + sum pixel * k) >> 22)).
 * At 224 that resize is the identity and vg_render_crops[_ex] write the crops themselves; this entry point computes the chain for
 * 65 <= image_size <= 448, bit for bit (below 65 torch's CPU interpolate sums in another order: DESIGN.md section 4).
 *   in_kind 0: d_in = float [n, in_side, in_side], vg_render_crops[_ex] out_kind 3 (in_side = resolution - 2: 14 .. 126): the whole chain
 *   in_kind 1: d_in = uint8 [n, image_size, image_size], single-channel images at image_size already: the resample alone (in_side unused)
 *   d_bounds [224,2] = (first input pixel, tap count) and d_coef [224,ksize] = the taps in 2^-22 units per output pixel: Pillow's
 *   precompute_coeffs + normalize_coeffs_8bpc for image_size -> 224 (vilgod_amd/pil_resample.py; one table serves both passes).
 *   ksize >= ceil(2 * max(image_size / 224, 1)) * 2 + 1, the taps Pillow reserves (5 .. 9).
 *   d_lut as vg_render_crops; out_kind 0, 1, 2, 4, 5 with the layouts and value mappings documented there (d_out sized for n crops).
 * One workgroup per crop; no allocation, no synchronisation.  n <= 0: VG_OK.  VG_ERR_ARG (nothing launched, outputs untouched) for an
 * image_size outside 65 .. 448, null pointers, other kinds, an in_side outside 14 .. 126 for in_kind 0, a ksize below the bound above. */
#define VG_PREPROCESS_MIN_IMAGE_SIZE 65
#define VG_PREPROCESS_MAX_IMAGE_SIZE 448
int vg_clip_preprocess(const void* d_in, int in_kind, int n, int in_side, int image_size,
                       const int32_t* d_bounds /*[224,2]*/, const int32_t* d_coef /*[224,ksize]*/, int ksize,
                       const float* d_lut, void* d_out, int out_kind, void* stream);

/* ---- CLIP ViT image tower + zero-shot scores (rows D7, D9) --------------------------------------
 * Replaces ClipWrapper.predict_clip_labels' GPU part, src/utils/clip_utils.py:37-44:
 *   model.encode_image (third_party/CLIP/clip/model.py:340-341 -> VisionTransformer.forward :223-240,
 *   ResidualAttentionBlock :171-192, LayerNorm-in-fp32 :157-163, QuickGELU :166-168),
 *   feature normalisation, 100 * f @ text.T, softmax.  */
typedef struct vg_vit vg_vit;

/* dtype 0: float32 everywhere (parity mode vs the fp32 CPU reference)
 * dtype 1: fp16 GEMM operands/activations with fp32 accumulate, fp32 LayerNorm statistics and fp32 residual stream
 *          (what model.py:375-396 `convert_weights` gives the reference on a GPU, or better).  With width % 256 == 0 the
 *          blocks' ln_1 / ln_2 are folded into the GEMMs around them (gamma-scaled fp16 weights built once per handle at the
 *          first encode, which therefore allocates and synchronises and must not run inside a stream capture);
 *          VG_VIT_LN_FOLD=0 at create time keeps separate LayerNorm kernels.
 * Constraints: width % 128 == 0, width <= 1024, heads * 64 == width, tokens T = (resolution / patch)^2 + 1 <= 1024 for dtype 1
 * (T <= 224: k_attention_f16; above: k_attention_f16_long) and T <= 282 for dtype 0 (k_attention_f32's LDS bound).  Any patch size:
 * the patch-embedding K = 3 * patch^2 is padded to a multiple of 64 (ViT-L/14: 588 -> 640) in conv1.weight and the im2col rows. */
int vg_vit_create(vg_vit** out, int width, int layers, int heads, int patch, int resolution, int out_dim, int dtype);
void vg_vit_destroy(vg_vit* v);
/* one tensor by its reference state_dict name without the 'visual.' prefix (model.py:206-221,171-183);
 * h_data: HOST float32.  Synchronous (hipMalloc + copy); not on the per-frame path. */
int vg_vit_set_weight(vg_vit* v, const char* name, const float* h_data, int64_t numel);
/* The per-channel input normalisation (x / 255 - mean_c) / std_c that input_kind 3 folds into the patch embedding; HOST float[3] each.
 * Default: CLIP's preprocess constants (third_party/CLIP/clip/clip.py:85). */
int vg_vit_set_input_norm(vg_vit* v, const float* h_mean3, const float* h_std3);
/* bytes of device workspace for n_crops; the caller zero-fills it once. */
int64_t vg_vit_workspace_bytes(const vg_vit* v, int n_crops);
/* d_crops: [n,3,res,res] CHW, input_kind 0 = float32, 1 = float16 (what vg_render_crops out_kind 1/2
 * writes); input_kind 2 = f16 patch rows [n*(res/patch)^2, 3*patch^2] (vg_render_crops out_kind 4, fp16 mode and 3*patch^2 % 64 == 0 only;
 * row count must be padded by the caller to a multiple of 256 rows of readable memory); input_kind 3 = f16 single-channel patch rows
 * [n*(res/patch)^2, patch^2] holding level / 256 (vg_render_crops out_kind 5, fp16 mode, patch^2 % 128 == 0): the patch embedding
 * (model.py:223-226 after clip.py:79-86's Normalize) runs as a K = patch^2 GEMM on W1[n,p] = 256/255 sum_c conv1[n,c,p] / std_c with
 * the constant - sum_c mean_c / std_c sum_p conv1[n,c,p] added through the positional table; built once per handle at the first such
 * encode (allocates and synchronises: not inside a stream capture).  d_feat: [n,out_dim] float32 = encode_image output (before normalisation). */
int vg_vit_encode(vg_vit* v, const void* d_crops, int input_kind, int n_crops, void* d_workspace, float* d_feat,
                  void* stream);
/* Measurement hooks (bench.py `roofline`): HIP event pairs around every projection-GEMM launch of
 * vg_vit_encode, on the stream the kernels are launched on.  vg_vit_profile(v,1) arms and clears,
 * vg_vit_profile_read synchronises and returns launches, summed ms and algorithmic FLOPs (2*M*N*K each). */
int vg_vit_profile(vg_vit* v, int on);
int vg_vit_profile_read(vg_vit* v, int32_t* h_launches, double* h_ms, double* h_flops);
/* the same, restricted to one kernel: kind 1 = the 256 x 256 projection GEMM (k_gemm_f16_w4, or k_gemm_f16_pp64 with VG_GEMM_W4=0: every ViT-B/16
 * shape), 0 = k_gemm_f16 / k_gemm_f32, -1 = all projection GEMMs; 2 = the fp16 attention launches over all query rows, 3 = the
 * class-row-only attention of the last block (flops: 4 * rows * T * 64 per (crop, head)) */
int vg_vit_profile_read_kind(vg_vit* v, int kind, int32_t* h_launches, double* h_ms, double* h_flops);

/* One projection GEMM of the tower, C = X @ Wt^T with the fused epilogue the block uses
 * (model.py:175-191: in_proj, out_proj + residual, c_fc + QuickGELU, c_proj + residual), exposed so the
 * GEMM can be unit-tested and timed alone.  dtype 1: f16 operands (M%256, N%128, K%32 == 0); 0: f32
 * (M%64, N%64, K%16).  epi 0: +bias -> C   1: +bias, QuickGELU -> C   2: d_resid(f32) += X@Wt^T + bias
 * 3: C float32, no bias (patch embedding, model.py:224).
 * 4 (dtype 1, N%256 == 0, K%64 == 0, K >= 128): d_resid points to an fp16 [M,N] residual stream updated in place,
 *   resid = f16(resid + f16(X@Wt^T + bias)) -- what the reference's fp16 run computes; the f16 tower takes it only with the
 *   environment variable VG_VIT_RESID16=1 (width%256 == 0); the default keeps the fp32 stream of epi 2. */
int vg_gemm(int dtype, int epi, const void* d_X, const void* d_Wt, const float* d_bias, void* d_C, float* d_resid,
            int M, int N, int K, void* stream);
/* The kernel vg_gemm would launch for these arguments under the current environment switches (VG_GEMM_W4, VG_GEMM_F32_MFMA, read
 * per call as vg_gemm reads them): 0 k_gemm_f16, 1 k_gemm_f16_pp64, 2 k_gemm_f16_w4, 3 k_gemm_f32, 4 k_gemm_f32_mfma; negative where
 * vg_gemm returns VG_ERR_ARG.  It is the function vg_gemm's own dispatch asks; it launches nothing and touches no device.  (The
 * split-K tail of vg_gemm_resid_splitk is planned from the CU count and is not part of the answer.) */
int vg_gemm_family(int dtype, int epi, int M, int N, int K);

/* The folded-LayerNorm epilogues of the fp16 projection GEMM (model.py:190-191: ln_1 / ln_2 ride in in_proj / c_fc), alone, for
 * unit tests.  Handle-less like vg_gemm: the kernel family is chosen by VG_GEMM_W4, read per call.  d_X, d_Wt f16; M % 256 == 0,
 * N % 256 == 0, K % 64 == 0, K >= 256 under k_gemm_f16_w4.  d_stats: LnPartial[M][N_or_K / P] of float pairs (mean, m2 = sum of
 * squared deviations from that mean) over P consecutive columns, P = vg_gemm_ln_partial_cols().
 * kind 0: consumer, C = f16(rstd (X@Wt^T - mean c1) + d_bias) with (mean, rstd) merged from the row's K / P partials of d_stats,
 *         rstd = rsqrt((sum m2 + P sum (mean_i - mean)^2) / K + 1e-5); d_bias is c2.  d_C f16 with row stride ldc >= N (ldc % 8 == 0).
 *         K % 128 == 0 (w4) or K % 256 == 0 (pp64), K <= 1024.
 * kind 1: the same, then QuickGELU.
 * kind 2: producer on the fp32 stream, ldc == N: d_resid f32 [M,N] += X@Wt^T + d_bias; d_x16 = f16 copy of the new d_resid; d_stats
 *         written from it.
 * kind 3: producer on the fp16 pair (k_gemm_f16_w4 only: VG_ERR_ARG with VG_GEMM_W4=0), ldc == N: t = (X@Wt^T + d_bias) + (hi + lo)
 *         with hi = d_x16, lo = d_resid (both f16 [M,N], read and written): hi = f16(t), lo = f16(t - hi); d_stats of hi + lo. */
int vg_gemm_ln(int kind, const void* d_X, const void* d_Wt, const float* d_bias, const float* d_c1, void* d_stats, void* d_C, int ldc,
               void* d_resid, void* d_x16, int M, int N, int K, void* stream);
/* P of vg_gemm_ln's partial statistics for the current VG_GEMM_W4: 128 (k_gemm_f16_w4) or 256 (k_gemm_f16_pp64) */
int vg_gemm_ln_partial_cols(void);

/* vg_gemm(dtype 1, epi 2) the way the tower launches its residual GEMMs (out_proj / c_proj, model.py:190-191): with scratch for a
 * split-K tail.  A 256 x 256 tile owns a CU, so a launch runs in rounds of n_cu tiles; the row tiles that do not fill complete rounds
 * (when they are at most half a round) are computed by several workgroups per tile, each over a slice of K, their fp32 partial tiles
 * summed in fixed order before the residual epilogue -- deterministic, within fp32 rounding of the unsplit result.  d_scratch: device
 * memory, 256 KB per (tail tile, part).  OPT-IN through the environment, read per launch: VG_GEMM_SPLITK=n allows up to n parts per tile
 * (8 is the measured optimum); unset, 0, K < 1536 or too little scratch = the unsplit launch.  One encode at a time gains 2.8 % at
 * 333-338 crops; with two encodes in flight (the throughput pipeline) the other encode already fills the last round: off by default. */
int vg_gemm_resid_splitk(const void* d_X, const void* d_Wt, const float* d_bias, float* d_resid, int M, int N, int K,
                         void* d_scratch, int64_t scratch_bytes, void* stream);

/* The fp16 attention kernel of the tower alone (model.py:175-187 via nn.MultiheadAttention): d_qkv fp16 [n_crops*T, ld] with
 * q | k | v at column offsets 0 | W | 2W (what in_proj writes), d_out fp16 [n_crops*T, W] = softmax(q k^T / 8) v per (crop, head).
 * 1 <= T <= 1024: k_attention_f16 for T <= 224, the flash-style k_attention_f16_long above (ViT-L/14's 257 tokens).
 * Exposed so that the kernels can be unit-tested against a plain fp32 attention. */
int vg_attention(const void* d_qkv, void* d_out, int n_crops, int T, int W, int heads, int ld, void* stream);

/* Every attention path of the tower alone (model.py:175-187 via nn.MultiheadAttention), for unit tests against a float64
 * softmax(q k^T / 8) v; vg_attention's layout of d_qkv / d_out.  Handle-less: VG_ATT_TR / VG_ATT_STAGGER are read per call.
 * dtype 1: the fp16 kernels as vg_vit_encode launches them, with the caller's q_tiles: only the first q_tiles 32-row query tiles of
 *   every crop are computed and written (1 <= q_tiles <= ceil(T / 32); the tower passes 1 in its last block, whose class-token row
 *   alone is used, model.py:235), the other rows of d_out are left as they were.  ld >= 3 W, ld % 8 == 0.
 * dtype 0: k_attention_f32 (the fp32 parity mode) on float32 d_qkv / d_out.  That kernel hard-codes ld = 3 W and computes every row:
 *   ld != 3 W or q_tiles != ceil(T / 32) is VG_ERR_ARG, and so is a T whose K, V and probability rows exceed its 160 KiB of LDS
 *   (T * 145 * 4 bytes: T <= 282, the limit of vg_vit_create).
 * Anything else (T outside 1 .. 1024, heads * 64 != W, null pointers) is VG_ERR_ARG and nothing is launched. */
int vg_attention_rows(int dtype, const void* d_qkv, void* d_out, int n_crops, int T, int W, int heads, int ld, int q_tiles, void* stream);

/* The causal attention of the text tower alone (third_party/CLIP/clip/model.py:320-326 build_attention_mask, applied at :186): row q of
 * an item sees keys 0 .. q.  vg_attention_rows' layouts, handle-less, every query row computed.
 * dtype 1: k_attention_f16 with its CAUSAL parameter (key blocks above a wave's query tile skipped, the diagonal block masked), T <= 224,
 *   ld >= 3 W, ld % 8 == 0.   dtype 0: k_attention_f32<CAUSAL>, ld == 3 W, T <= 282 (its LDS bound).
 * Row i equals, bit for bit, row i of vg_attention_rows on the item's first i + 1 tokens.
 * Anything else (a longer T, heads * 64 != W, null pointers) is VG_ERR_ARG and nothing is launched. */
int vg_attention_causal_rows(int dtype, const void* d_qkv, void* d_out, int n_items_crops, int T, int W, int heads, int ld, void* stream);

/* ---- CLIP text tower: replaces model.encode_text (third_party/CLIP/clip/model.py:343-356) as ClipWrapper.__init__ calls it for the
 * class prompts (src/utils/clip_utils.py:22-26).  The image tower's blocks (VitRun) with causal attention, a token-table front end
 * and a head that reads one row per prompt.  dtype as vg_vit_create; the stream stays fp32 (no class-row last block). */
typedef struct vg_text vg_text;
/* Constraints: width % 128 == 0, width <= 1024, heads * 64 == width (vg_vit_create's), 1 <= ctx <= 224, vocab >= 1 (model.py:288-300). */
int vg_text_create(vg_text** out, int width, int layers, int heads, int ctx, int vocab, int out_dim, int dtype);
void vg_text_destroy(vg_text* t);
/* one tensor by its reference state_dict name (model.py:288-300: token_embedding.weight [vocab, width], positional_embedding
 * [ctx, width], transformer.resblocks.N.* (model.py:171-183), ln_final.weight / .bias, text_projection [width, out_dim]); h_data: HOST
 * float32.  A table whose size does not match the handle's is VG_ERR_ARG.  Synchronous. */
int vg_text_set_weight(vg_text* t, const char* name, const float* h_data, int64_t numel);
/* bytes of device workspace for n_prompts; the caller zero-fills it once. */
int64_t vg_text_workspace_bytes(const vg_text* t, int n_prompts);
/* d_tokens: int32 [n, ctx] (clip.py:197-237 tokenize); d_eot: int32 [n], the position whose row the head reads -- the first maximum of
 * the prompt's ids (model.py:354 argmax), computed by the caller; d_feat: float32 [n, out_dim] = ln_final(x[p, eot[p]]) @
 * text_projection, NOT normalised (model.py:352-354).  A token id outside [0, vocab) or an eot outside [0, ctx) is clamped on the
 * device: a wrong row, never a read outside the tables.  The first encode of a handle allocates (folded LayerNorms) like vg_vit_encode's. */
int vg_text_encode(vg_text* t, const int32_t* d_tokens, const int32_t* d_eot, int n_prompts, void* d_workspace, float* d_feat, void* stream);

/* ---- captured classification: the hipGraph loop of BASELINE config 5 ------------------------------------------------
 * vg_vit_encode + vg_clip_scores of one frame (the reference's per-chunk model.encode_image + softmax, clip_utils.py:37-61) as ONE
 * hipGraph per distinct crop count: captured on the first frame that has that many crops, replayed for every later one
 * (~150 kernel launches become one graph launch).  A cache belongs to ONE worker: one stream and one set of persistent buffers
 * (every pointer is part of the key).  The data-dependent stages of a frame (ground, clustering, rendering: their launch
 * dimensions change with every frame, and the hierarchy is built on the host) stay plain stream launches around the graph.
 * `stream` must be a created stream (not NULL).  While vg_vit_profile is on, the call falls back to plain launches.  A handle's first
 * call of every launch form (stream form of the plan, class-row last block, input kind, up to / above 64 classes) runs as plain
 * launches and counts in no statistic: it sets the kernels' launch attributes, which a capture must not. */
typedef struct vg_graph_cache vg_graph_cache;
int vg_graph_cache_create(vg_graph_cache** out);
void vg_graph_cache_destroy(vg_graph_cache* c);
int vg_graph_cache_stats(const vg_graph_cache* c, int64_t* h_captured, int64_t* h_replayed);
/* at most `max_graphs` graphExecs are kept (default 32); the least recently used one is destroyed when a new crop count arrives */
int vg_graph_cache_limit(vg_graph_cache* c, int max_graphs);
int vg_graph_cache_stats2(const vg_graph_cache* c, int64_t* h_captured, int64_t* h_replayed, int64_t* h_evicted, int64_t* h_live);
int vg_vit_classify_graph(vg_vit* v, vg_graph_cache* c, const void* d_crops, int input_kind, int n_crops, void* d_workspace, float* d_feat,
                          const float* d_text, int dim, int n_classes, float* d_probs, int32_t* d_top1, float* d_top1_score, void* stream);

/* clip_utils.py:42-61: probs = softmax(100 * normalise(feat) @ text.T) (d_text rows already unit
 * norm, clip_utils.py:26), top-1 class id and probability per crop.  One wave per crop, one lane per class: n_classes <= 64
 * (more is VG_ERR_ARG; vg_clip_scores_wide takes any number). */
int vg_clip_scores(const float* d_feat, int n, int dim, const float* d_text, int n_classes, float* d_probs,
                   int32_t* d_top1, float* d_top1_score, void* stream);
/* The same function for a class list of any length (clip_utils.py:22-26 builds one text row per entry of clip.class_list, :43 takes
 * the softmax over all of them; :49-61 the top-1): d_feat [n, dim], d_text [n_classes, dim], d_probs [n, n_classes], d_top1 /
 * d_top1_score [n]; the lowest index wins a tie.  Any n_classes >= 1 and any dim; n * n_classes is indexed in 64 bits.  One
 * 256-thread workgroup per crop; d_probs also holds the crop's logits between the kernel's passes.  A class's logit, probability and
 * rank do not depend on how many other classes there are, and for n_classes <= 64 the results equal vg_clip_scores' bit for bit.
 * n <= 0: VG_OK, nothing is launched.  Null pointers or n_classes <= 0: VG_ERR_ARG, nothing is launched.
 * vg_vit_classify_graph uses vg_clip_scores up to 64 classes and this entry point above. */
int vg_clip_scores_wide(const float* d_feat, int n, int dim, const float* d_text, int n_classes, float* d_probs,
                        int32_t* d_top1, float* d_top1_score, void* stream);
/* The top_k classes of every crop (clip_utils.py:49-61: np.argpartition(img_score, -top_k)[-top_k:] ordered by np.argsort(-scores)),
 * selected on the device from the table either kernel above wrote.  d_probs [n, n_classes]; row i of d_idx / d_score [n, top_k]
 * holds the top_k classes of crop i under the strict total order (probability descending, class index ascending), entry 0 the best,
 * d_score each class's own float32 bits from the table.  A NaN probability orders behind every number (NaNs among themselves by
 * index) and is written as it stands; -0.0 and +0.0 are equal, the index decides.  Column 0 therefore equals d_top1 / d_top1_score
 * of vg_clip_scores[_wide] bit for bit, and a row whose top_k + 1 largest probabilities are distinct equals the reference's.
 * vg_clip_topk: device pointers, ONE launch on `stream` (csrc/clip_topk.hip: one wave per crop, top_k shuffle rounds), its grid sized
 * from n alone: no atomics, no read-back, no allocation, no scratch -- the same bits on every run, and it can be captured.
 * vg_clip_topk_host: the same arguments over host arrays under the same comparator (csrc/clip_topk_key.inc); the two agree bit for
 * bit.  No GPU needed.
 * VG_ERR_ARG (nothing launched, outputs untouched): top_k < 1, top_k > VG_CLIP_MAX_TOPK, top_k > n_classes, n_classes < 1, null
 * pointers with n > 0.  n <= 0 (with valid top_k / n_classes): VG_OK, nothing launched, nothing written. */
#define VG_CLIP_MAX_TOPK 32
int vg_clip_topk(const float* d_probs, int n, int n_classes, int top_k, int32_t* d_idx, float* d_score, void* stream);
int vg_clip_topk_host(const float* h_probs, int n, int n_classes, int top_k, int32_t* h_idx, float* h_score);

/* ---- ground segmentation (rows A1-A5) -----------------------------------------------------------
 * Replaces the pybind11 module `pypatchworkpp` (third_party/patchwork-plusplus/python_wrapper/pybinding.cpp:9-55)
 * as used by ZeroShotDetector.mask_ground_points (src/vilgod/zero_shot_detector.py:129-151) through
 * pointcloud_utils.mask_ground_points_patchwork_pp (src/utils/pointcloud_utils.py:49-56).
 * One handle per sequence and stream: like the reference object it carries the adaptive state
 * (elevation / flatness stores and thresholds, sensor height) from frame to frame
 * (patchworkpp.cpp:315-316, 339-376) and is not thread-safe. */
typedef struct vg_ground vg_ground;

/* field-for-field patchwork::Params (patchworkpp/include/patchworkpp.h:38-108; `verbose`,
 * `intensity_thr` dropped: unused by the algorithm) */
typedef struct vg_ground_params {
    int enable_RNR, enable_RVPF, enable_TGR;
    int num_iter, num_lpr, num_min_pts, num_zones, num_rings_of_interest;
    double RNR_ver_angle_thr, RNR_intensity_thr;
    double sensor_height, th_seeds, th_dist, th_seeds_v, th_dist_v, max_range, min_range;
    double uprightness_thr, adaptive_seed_selection_margin;
    int num_sectors_each_zone[4];
    int num_rings_each_zone[4];
    int max_flatness_storage, max_elevation_storage;
    double elevation_thr[4], flatness_thr[4];
} vg_ground_params;

void vg_ground_default_params(vg_ground_params* p);          /* patchworkpp.h:75-107 */
int vg_ground_create(vg_ground** out, const vg_ground_params* p, int max_points);   /* patchworkpp.h:116-146 */
void vg_ground_destroy(vg_ground* h);
/* fresh adaptive state (the reference builds a new object per sequence, zero_shot_detector.py:137-140);
 * p may be NULL to keep the parameters.  Parameters that vg_ground_create refuses are refused here too (VG_ERR_ARG):
 * the handle then keeps its parameters and its state. */
int vg_ground_reset(vg_ground* h, const vg_ground_params* p);
/* estimateGround + getGround (patchworkpp.cpp:152-337; pybinding.cpp:49,53).  d_points: [n,stride] f32,
 * columns x, y, z, intensity; z_offset is subtracted in float64 and rounded to float32 exactly as
 * pointcloud_utils.py:50-51 + the Eigen::MatrixXf conversion do.  d_ground_mask: [n] uint8, 1 = ground
 * (the index set the reference returns; lidar_frame.py:82-87 turns it into this mask anyway). */
int vg_ground_estimate(vg_ground* h, const float* d_points, int n, int stride, double z_offset,
                       uint8_t* d_ground_mask, void* stream);
/* synchronous diagnostics: {sensor_height (getHeight, pybinding.cpp:47), elevation_thr[4], flatness_thr[4],
 * stored elevation counts[4], stored flatness counts[4]} */
int vg_ground_get_state(vg_ground* h, double* h_out17, void* stream);
/* the COMPLETE frame-to-frame state (patchworkpp.cpp:315-316, 339-376: sensor height, elevation / flatness thresholds and the
 * per-ring stores they are recomputed from, patchworkpp.h:171-189 members) as an opaque host blob of vg_ground_state_bytes()
 * bytes.  export after frame f on one handle + set on another handle (other stream / GPU / rank) = the sequence continues
 * there bit for bit: the hand-off that frame-sharding a sequence needs (SURVEY 8b "Native surface", 8e exception 1).
 * Synchronous.  set_state validates the blob's cursors and returns VG_ERR_ARG for a foreign layout. */
int64_t vg_ground_state_bytes(void);
int vg_ground_export_state(vg_ground* h, void* h_blob, void* stream);
int vg_ground_set_state(vg_ground* h, const void* h_blob, void* stream);
int vg_ground_num_patches(const vg_ground* h);
/* synchronous: [n_patches,12] = n, n_ground, normal[3] (getNormals), mean[3] (getCenters), singular values[3],
 * decision (0 non-ground, 1 ground) */
int vg_ground_get_patch_info(vg_ground* h, float* h_out, void* stream);

/* ---- spatial clustering (row B2) -------------------------------------------------------------------
 * Replaces `cluster_model.fit(X)` (src/vilgod/zero_shot_detector.py:248; model built by
 * src/utils/cluster_utils.py:11-12 from tools/configs/preprocessor/waymo.yaml:10-15:
 * hdbscan.HDBSCAN(min_cluster_size=15, cluster_selection_epsilon=0.15, metric='euclidean')) and reads
 * back `labels_` / `probabilities_` (consumed at src/vilgod/lidar_frame.py:163-167).
 * The library itself is an un-vendored, unpinned dependency of the reference (README.md:74-75). */

/* Hierarchy stage on the HOST from the MST of the mutual-reachability graph, edges sorted ascending by
 * (w2, lo, hi): single linkage -> condense(min_cluster_size) -> stability -> EOM ->
 * cluster_selection_epsilon -> labels (-1 = noise) and probabilities.  h_w2: SQUARED weights, ascending;
 * runs of equal weight are re-ordered by (lo, hi) internally.
 * Host pointers only; no GPU involved (runs in the CPU test-suite too). */
int vg_hdbscan_tree_host(const int32_t* h_lo, const int32_t* h_hi, const double* h_w2, int n,
                         int min_cluster_size, double eps, int32_t* h_labels, double* h_probs,
                         int32_t* h_n_clusters);

/* vg_hdbscan_tree_host with the library's three cluster-selection options (the semantics of its scikit-learn port,
 * sklearn/cluster/_hdbscan/_tree.pyx:708-784 selection, :578-641 epsilon, :433-512 labels):
 *   selection             0 = excess of mass, 1 = leaf (the leaves of the cluster tree; a tree without a split selects nothing)
 *   allow_single_cluster  0 / 1: the root takes part in excess of mass (birth 0, size = the sum of its child clusters' sizes), the
 *                         epsilon climb may end at the root, and a selected root holds the points whose own lambda reaches 1 / eps
 *                         (eps != 0) or the largest lambda among the root's own rows (eps == 0).  A tree of 2 .. min_cluster_size
 *                         points is all root then (without the option: all noise).
 *   max_cluster_size      0 = unlimited; excess of mass only: a larger cluster loses to its children whatever the stabilities
 * Values outside these ranges: VG_ERR_ARG.  (0, 0, 0) is vg_hdbscan_tree_host. */
int vg_hdbscan_tree_host_ex(const int32_t* h_lo, const int32_t* h_hi, const double* h_w2, int n, int min_cluster_size, double eps,
                            int selection, int allow_single_cluster, int max_cluster_size, int32_t* h_labels, double* h_probs,
                            int32_t* h_n_clusters);

/* The same hierarchy stage ON THE DEVICE (csrc/hdbscan_device.hip): d_lo / d_hi / d_w2 = the tree as vg_cluster_mst_nd leaves it
 * (sorted by weight, ties in any order), d_labels [n] / d_probs [n] / d_n_clusters [1] device outputs equal, bit for bit, to what
 * vg_hdbscan_tree_host returns for the same tree.  No host work between the tree and the labels: the stage is a sequence of kernels on
 * `stream`.  A handle holds the stage's buffers for trees of up to max_points (<= 2^20) points; min_cluster_size in [2, 32]
 * (VG_ERR_ARG beyond: the host stage has no such bound), n > max_points: VG_ERR_CAPACITY.  One call at a time per handle. */
typedef struct vg_hier vg_hier;
int vg_hier_create(vg_hier** out, int max_points);
int vg_hier_destroy(vg_hier* h);
int vg_hdbscan_tree_device(vg_hier* h, const int32_t* d_lo, const int32_t* d_hi, const double* d_w2, int n, int min_cluster_size,
                           double eps, int32_t* d_labels, double* d_probs, int32_t* d_n_clusters, void* stream);
/* ... with selection / allow_single_cluster / max_cluster_size as vg_hdbscan_tree_host_ex takes them (VG_ERR_ARG outside their ranges):
 * bit for bit what vg_hdbscan_tree_host_ex returns, by the same sequence of kernels (the root's chain statistics are computed only
 * with allow_single_cluster).  (0, 0, 0) is vg_hdbscan_tree_device. */
int vg_hdbscan_tree_device_ex(vg_hier* h, const int32_t* d_lo, const int32_t* d_hi, const double* d_w2, int n, int min_cluster_size,
                              double eps, int selection, int allow_single_cluster, int max_cluster_size, int32_t* d_labels,
                              double* d_probs, int32_t* d_n_clusters, void* stream);

/* LidarFrame.generate_detections' grouping (src/vilgod/lidar_frame.py:163-167, 230-237; Detection objects :42-58 of
 * src/dataclass/objects.py) on the host: points whose membership probability is < threshold become noise (h_probs may be NULL),
 * clusters in ascending label order, each cluster's point indices ascending.  h_ids [capacity n]: the labels that own a point;
 * h_index [capacity n]: packed point indices; h_seg [capacity n + 1]: cluster offsets into h_index; *h_n_clusters: clusters written. */
int vg_pack_clusters_host(const int32_t* h_labels, const double* h_probs, int n, double threshold, int64_t* h_ids,
                          int32_t* h_index, int32_t* h_seg, int32_t* h_n_clusters);

/* The same grouping ON THE DEVICE (csrc/pack.hip), for labels that are born there (vg_hdbscan_tree_device) and lists that are only read
 * there (vg_cluster_filter[_ex], vg_plane_ransac, vg_render_crops, vg_cluster_boxes / _lshape / _medians): lidar_frame.py:163-167 (low
 * probability -> noise) and :230-237 (one Detection per remaining label, np.where's ascending indices) without leaving HBM.
 * A point is dropped iff label < 0 or (d_probs given and prob < threshold: strict, float64, so a NaN probability keeps the point like
 * numpy's `labels[probs < threshold] = -1`).  label_bound: exclusive upper bound of the labels, 0 .. 2^24 (a hierarchy of n points with
 * min_cluster_size m selects at most n / m clusters); only the bits it needs are sorted.  n <= 2^24.
 * Device outputs with vg_pack_clusters_host's meaning -- d_ids [capacity n] int64 labels that own a point, ascending; d_index
 * [capacity n] kept point indices, cluster after cluster, ascending inside a cluster; d_seg [capacity n + 1] offsets -- and
 * d_counts [3] = {C, P = d_seg[C], overflow}.  Only d_ids[0 .. C), d_index[0 .. P), d_seg[0 .. C] are written.  overflow != 0: some label
 * was >= label_bound; those points were left out (nothing is written out of bounds) and the lists must not be used -- pack such a frame
 * with a larger bound or with vg_pack_clusters_host.
 * A fixed sequence of 3 * passes + 3 kernels and one 16-byte memset on `stream` (passes = 1, 2, 3 for label_bound <= 2^8, 2^16, 2^24):
 * no host work, no synchronisation, no allocation.  A stable radix sort whose positions come from ranks, never from an atomic cursor:
 * the same bits on every run.  d_work: vg_pack_clusters_work_bytes(n) bytes of device scratch (-1 for an n out of range), contents
 * irrelevant before and after; one call at a time per work buffer.  VG_ERR_ARG (nothing launched, outputs untouched) for null pointers,
 * n or label_bound out of range, work_bytes too small.  n == 0 / no kept point: C = P = 0, d_seg[0] = 0. */
int64_t vg_pack_clusters_work_bytes(int n);
int vg_pack_clusters(const int32_t* d_labels, const double* d_probs, int n, double threshold, int label_bound, void* d_work,
                     int64_t work_bytes, int64_t* d_ids, int32_t* d_index, int32_t* d_seg, int32_t* d_counts, void* stream);

/* The packed sub-lists of the clusters that passed the filters (classification and boxes are `valid_only`,
 * src/vilgod/zero_shot_detector.py:389-390, :444-448): the segments c of (d_index, d_seg [n_clusters + 1]) with d_valid[c] != 0 --
 * the bytes vg_cluster_filter / vg_cluster_filter_ex write, taken as they are -- concatenated in order.  n_index: entries of d_index
 * the caller vouches for (P, or an upper bound of it: min(n_index, d_seg[n_clusters]) points are looked at).
 * d_out_index [capacity n_index], d_out_seg [capacity n_clusters + 1], d_counts [2] = {kept clusters K, kept points Q}; only
 * d_out_index[0 .. Q) and d_out_seg[0 .. K] are written.  Two kernels on `stream` (one scan of the cluster sizes, one copy that finds
 * each point's cluster by bisection), deterministic.  d_work: vg_pack_select_work_bytes(n_clusters) bytes of device scratch. */
int64_t vg_pack_select_work_bytes(int n_clusters);
int vg_pack_select(const int32_t* d_index, const int32_t* d_seg, int n_clusters, int n_index, const uint8_t* d_valid, void* d_work,
                   int64_t work_bytes, int32_t* d_out_index, int32_t* d_out_seg, int32_t* d_counts, void* stream);

/* GPU half of the clustering: exact k-NN core distances and THE minimum spanning tree of the mutual
 * reachability graph under the strict edge order (w2, pair d2, min id, max id) (unique -> identical to the CPU oracle's). */
typedef struct vg_cluster vg_cluster;
#define VG_CLUSTER_MAX_K 64 /* largest min_samples of vg_cluster_mst[_nd] */
int vg_cluster_create(vg_cluster** out, int max_points);
void vg_cluster_destroy(vg_cluster* h);
/* HOST ONLY (no HIP call): bytes of device memory a handle for max_points points holds in its listed buffers (csrc/cluster.hip
 * CL_BUFFERS) -- all of it but the sort / scan scratch, a few MB.  0 for max_points <= 0. */
size_t vg_cluster_bytes(int max_points);
/* d_points [n,stride] f32 (x,y,z first; `points_ref_wo_ground[..., :3]`, zero_shot_detector.py:246).
 * k = min_samples (= min_cluster_size in the reference's configuration), 1 <= k <= VG_CLUSTER_MAX_K (VG_ERR_ARG outside):
 * core distance = distance to the k-th nearest OTHER point, +inf for a point with fewer than k others.  k <= 15 keeps each
 * query's neighbour list in registers; 16 <= k <= 64 keeps it in LDS (per-lane heaps) and, for the queries whose neighbourhood
 * is wider than their node's shell, in one sorted list across the 64 lanes of a wave -- hence the limit.  Same results
 * either way: exact, float64.  Outputs (device): d_core2 [n] f64 squared core distances in input order (may be NULL);
 * d_mst_lo/hi [n-1] int32 input indices (lo < hi); d_mst_w2 [n-1] f64 SQUARED weights, ascending.
 * Termination is decided on the device (every kernel of a round returns at once when the tree was complete before the round);
 * the host queues the first six rounds without reading anything back and synchronises `stream` once per batch (one 4-byte
 * counter per round): typically one or two synchronisations per call.  h_rounds (host, may be NULL): rounds needed. */
int vg_cluster_mst(vg_cluster* h, const float* d_points, int n, int stride, int k, double* d_core2, int32_t* d_mst_lo,
                   int32_t* d_mst_hi, double* d_mst_w2, int32_t* h_rounds, void* stream);
/* The same over the first `dim` (3, 4 or 5) columns: dim = 5 is the two-frame clustering input
 * [x, y, z, entropy score, 0.1 * relative frame] of zero_shot_detector.py:232-239 (preprocessing.yaml:68 n_frames: 2).
 * float64 distances summed left to right over the coordinates; the cell grid and all pruning use x,y,z only. */
int vg_cluster_mst_nd(vg_cluster* h, const float* d_points, int n, int stride, int dim, int k, double* d_core2,
                      int32_t* d_mst_lo, int32_t* d_mst_hi, double* d_mst_w2, int32_t* h_rounds, void* stream);

/* ---- fixed-radius neighbour queries (entropy scores, two-frame clustering) -------------------
 * vg_cluster_grid builds the handle's 0.4 m cell grid over a TARGET set; it stays valid until the next
 * vg_cluster_grid / vg_cluster_mst[_nd] call on the handle.  Queued on `stream`: nothing is read back and nothing is copied from
 * the host, so the call can be captured into a graph (the number of targets is the handle's host state: a replay serves the n of
 * the captured call). */
int vg_cluster_grid(vg_cluster* h, const float* d_points, int n, int stride, void* stream);
/* d_counts[i] = min(cap, #{target t : d2(query_i, t) < r2}) with float32 d2 = fma(dz,dz,fma(dy,dy,dx*dx)):
 * what pointcloud_utils.py:74-107 derives from pcdet's ball_query (r2 = float32(radius)^2; count_neighbors: radius
 * 0.3, cap 1000, per neighbouring frame; count_neighbors_inter_frame: radius 0.2, cap 100), and the `dists < 0.1`
 * test on pytorch3d's squared k-NN distances (zero_shot_detector.py:226-227: r2 = 0.1f).  A query that is itself a
 * target counts (the reference subtracts 1 for the seek frame on the host side, pointcloud_utils.py:90-91). */
int vg_cluster_ball_count(vg_cluster* h, const float* d_query, int nq, int qstride, float r2, int cap, int32_t* d_counts,
                          void* stream);
/* Nearest target with float32 d2 <= max_d2 -> d_idx (row in the array given to vg_cluster_grid; lowest row among
 * equidistant targets; -1 if none) and d_d2 (+inf if none): knn_labels (pointcloud_utils.py:505-513; K=1 and the
 * 0.2 gate on pytorch3d's SQUARED distance). */
int vg_cluster_nearest(vg_cluster* h, const float* d_query, int nq, int qstride, float max_d2, int32_t* d_idx, float* d_d2,
                       void* stream);

/* ---- K nearest neighbours, no radius limit (csrc/cluster_knn.inc) -------------------------------------------
 * pytorch3d's `knn_points` as the reference calls it: pointcloud_utils.py:476-493 (chamfer_distance), :496-503 (knn), :505-513
 * (knn_labels), zero_shot_detector.py:221 (K = 4 among the moving points) and :237 (the label transfer).
 * The K nearest TARGETS (the set given to the last vg_cluster_grid, or vg_cluster_mst[_nd], on h) of every query row:
 *   pair distance  float32 d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) on float32 differences -- ONE function (cl_d2_f32), called by the
 *                  kernel and by vg_knn_host, the one vg_cluster_nearest / vg_cluster_ball_count use
 *   gate           a target qualifies when d2 <= max_d2; INFINITY: no gate; NaN or <= 0: VG_ERR_ARG (as vg_cluster_nearest)
 *   order          strict and total: (d2, row in the array given to vg_cluster_grid), ascending.  Row i of d_idx / d_d2 [nq, K] holds
 *                  the qualifying targets with the K smallest keys in that order.  Equidistant targets compete on the row, whichever
 *                  cells they lie in and also where K cuts through a group of ties.
 *   missing        -1 / +inf: fewer than K qualifying targets, an empty grid, and -- in all K places -- a query row with a coordinate
 *                  that is not finite (decided before any cell arithmetic).  Targets are finite by contract, as for vg_cluster_grid.
 *   refusals       VG_ERR_ARG for K < 1, K > VG_KNN_MAX_K, qstride < 3, null pointers with nq > 0; nq == 0 is VG_OK.
 * One launch on `stream`: one lane per query walks the target set's octree depth-first with its K best so far; no atomics, nothing
 * read back, nothing allocated, capturable.  The order in which nodes are visited decides speed only, never the result.
 * Where the K best live (the kernel's instantiations; the tests straddle each limit):
 *   K <= VG_KNN_K_REG1, <= VG_KNN_K_REG4, <= VG_KNN_K_REG8: 1, 4 or 8 register pairs per lane;
 *   K <= VG_KNN_K_LDS16, <= VG_KNN_MAX_K: a per-lane heap of 16 or 32 entries in LDS. */
#define VG_KNN_MAX_K 32
#define VG_KNN_K_REG1 1
#define VG_KNN_K_REG4 4
#define VG_KNN_K_REG8 8
#define VG_KNN_K_LDS16 16
int vg_cluster_knn(vg_cluster* h, const float* d_query, int nq, int qstride, int K, float max_d2, int32_t* d_idx, float* d_d2,
                   void* stream);
/* HOST ONLY, no GPU: the same pair function and the same order over ALL query x target pairs -- no grid, no pruning.
 * h_target [nt, tstride] (nt = 0: every entry missing); the other arguments and the refusals as above (tstride < 3: VG_ERR_ARG). */
int vg_knn_host(const float* h_query, int nq, int qstride, const float* h_target, int nt, int tstride, int K, float max_d2,
                int32_t* h_idx, float* h_d2);
/* HOST ONLY: the value the kernel compares with a query's K-th best d2 before it skips a node whose box distance
 * (vg_cluster_geom_probe h_box_d2) is box_d2: a lower bound of the FLOAT32 d2 to every target of the node.  The walk skips the node
 * only when this value is strictly greater. */
double vg_knn_prune_bound_host(double box_d2);

/* ---- ball query, the index form of vg_cluster_ball_count (csrc/cluster_ball_query.inc) ------------------------
 * pcdet's `pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils.ball_query` (ball_query_kernel_stack plus its Python wrapper) as the
 * reference calls it: pointcloud_utils.py:83 (count_neighbors) and :99 (count_neighbors_inter_frame).
 *   targets        the point set last given to vg_cluster_grid on h (or to vg_cluster_mst[_nd] / vg_cluster_dbscan); a target's row is
 *                  its index in that array
 *   hits           H(q) = the target rows t with cl_d2_f32(q, t) < r2, STRICTLY; cl_d2_f32 is the float32
 *                  fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of vg_cluster_ball_count / _nearest / _knn (ONE function, called by the kernel
 *                  and by vg_ball_query_host).  A query that is itself a target is a hit.
 *   outputs        cnt(q) = min(|H(q)|, nsample); d_idx[q, 0 .. cnt) = the cnt SMALLEST rows of H(q), ascending (pcdet walks the
 *                  targets in row order and keeps the first nsample hits); d_idx[q, cnt .. nsample) = d_idx[q, 0], pcdet's padding
 *                  with the first hit; an empty ball: cnt = 0 and a row of zeros (what pcdet's wrapper leaves after
 *                  idx[empty_ball_mask] = 0).  d_idx int32 [nq, nsample]; d_cnt int32 [nq], may be NULL.
 *   not finite     a query row with a coordinate that is not finite has an empty ball (decided before any cell is indexed); a target
 *                  with such a coordinate is never a hit.  Both are what pcdet's arithmetic gives.
 *   consequence    cnt equals vg_cluster_ball_count(..., cap = nsample) for every query.
 *   refusals       VG_ERR_ARG, nothing launched, outputs untouched: r2 NaN or <= 0; ceil(sqrt(r2) / 0.4) > 8 (the grid's reach limit,
 *                  3.2 m, as vg_cluster_ball_count); nsample < 1 or > VG_BALL_QUERY_MAX_NSAMPLE (the reference uses 1000 and 100);
 *                  qstride < 3; null h, d_query or d_idx with nq > 0.  nq == 0 is VG_OK.  An empty grid gives zeros and cnt = 0.
 * One launch on `stream`, its grid sized from nq alone: nothing read back, nothing allocated, no global-memory atomics, capturable;
 * the same bits on every run.  One wave per query collects the hits' rows in an LDS buffer of VG_BALL_QUERY_CAND entries; before the
 * buffer could overflow it is sorted, the nsample smallest rows stay and only hits below the largest of them are taken from then on.
 * All scratch is LDS: the handle holds no buffer for this call. */
#define VG_BALL_QUERY_MAX_NSAMPLE 1024
#define VG_BALL_QUERY_CAND 2048
int vg_cluster_ball_query(vg_cluster* h, const float* d_query, int nq, int qstride, float r2, int nsample, int32_t* d_idx,
                          int32_t* d_cnt, void* stream);
/* HOST ONLY, no GPU: pcdet's loop as written -- the targets [n, tstride] in row order, the first nsample hits, the same pair function,
 * the same outputs (cnt may be NULL).  No reach limit; the other refusals as above (tstride < 3: VG_ERR_ARG). */
int vg_ball_query_host(const float* targets, int n, int tstride, const float* query, int nq, int qstride, float r2, int nsample,
                       int32_t* idx, int32_t* cnt);

/* DBSCAN: sklearn.cluster.DBSCAN, the second clustering model the reference's cluster_utils.py imports (src/utils/cluster_utils.py:4-5),
 * on the handle's 0.4 m grid (csrc/cluster_dbscan.inc).  The definition -- what sklearn's dbscan_inner computes, stated without its
 * traversal (it grows clusters to completion one seed at a time in row order; a border row is claimed by the first cluster that
 * reaches it):
 *   input     d_points [n, stride] float32; the first dim = 3, 4 or 5 columns are the clustering space, x, y, z first (5 = the
 *             two-frame points_seq).  Finite by contract, as for vg_cluster_grid: nothing is read back to check it.
 *   pair      both rows widened exactly to double; d2 = ((dx*dx + dy*dy) + dz*dz [+ d4*d4 [+ d5*d5]]), left to right, no fused
 *             multiply-add (csrc/dbscan_pair.inc, one __host__ __device__ text for the kernels and the host twin); neighbours iff
 *             d2 <= eps2, INCLUSIVE, eps2 = eps * eps formed in double.  A row is its own neighbour.
 *   core      row i is a core sample iff it has at least min_samples neighbours, itself and duplicates counted
 *   clusters  the connected components of the graph on the core rows whose edges are neighbour pairs; labels 0, 1, ... in ascending
 *             order of each component's LOWEST CORE ROW (index in the caller's array)
 *   border    a non-core row with at least one core neighbour takes the smallest label among its core neighbours; every other
 *             non-core row gets -1
 *   outputs   on the device, in the caller's row order: d_labels int32 [n]; d_core uint8 [n] (1 = core sample); d_n_clusters int32 [1];
 *             d_probs float64 [n] or NULL: 1.0 for a labelled row, 0.0 for noise.  sklearn's DBSCAN has no probabilities_; the
 *             reference reads cluster_info.probabilities_ after fit, so this is this project's own convention.
 * vg_cluster_dbscan builds the grid over d_points itself (the handle's grid is replaced, as by vg_cluster_mst_nd, and afterwards
 * serves vg_cluster_ball_count / _nearest / _knn over these points) and queues the rest on `stream`: no read-back, no synchronisation,
 * no allocation (the working arrays are the handle's), every launch sized from n -- the call can be captured into a graph -- and only
 * integer atomics whose result is a set property or a minimum: the same bits on every run.  Every pointer walk of the union-find is
 * bounded by n; should one overrun (it cannot: parent[p] <= p throughout), d_n_clusters holds -1 and the labels are undefined.
 * One call at a time per handle.
 * vg_dbscan_host: HOST ONLY, no GPU: all pairs, no grid, a sequential union-find, the same pair function.  The two agree exactly.
 * VG_ERR_ARG (nothing launched): eps NaN, <= 0 or with ceil(eps / 0.4) > 8 (the grid's reach limit, 3.2 m, as
 * vg_cluster_ball_count); min_samples < 1; dim outside 3..5; stride < dim; n < 0; n > the handle's max_points; null pointers (d_probs /
 * h_probs may be NULL).  n == 0: VG_OK, n_clusters 0. */
int vg_cluster_dbscan(vg_cluster* h, const float* d_points, int n, int stride, int dim, double eps, int min_samples, int32_t* d_labels,
                      uint8_t* d_core, double* d_probs, int32_t* d_n_clusters, void* stream);
int vg_dbscan_host(const float* h_points, int n, int stride, int dim, double eps, int min_samples, int32_t* h_labels, uint8_t* h_core,
                   double* h_probs, int32_t* h_n_clusters);

/* HOST ONLY, no GPU (like vg_hdbscan_tree_host): the geometry vg_cluster_mst[_nd] prunes with, evaluated on the CPU by the very
 * functions its kernels call, so that the bounds can be checked without a device.  Pair i = (point i, query i), finite float32.
 *   h_origin_in [3] f64 or NULL: the grid's origin; NULL: the origin the kernels derive from the float32 extremes h_bbox_lo/hi [3]
 *   h_points [n,3] or NULL: NULL reads point i's cell from h_cell [n,3] instead of assigning it (cells outside the grid: VG_ERR_ARG)
 *   h_queries [n,3] or NULL (then h_box_d2 / h_radius2 are not written)
 * Outputs (each may be NULL): h_origin [3]; h_cell [n,3] cell of point i (512 x 512 x 64 cells of 0.4 m, points beyond the grid
 * clamped into border cells); h_code [n] its Morton code; h_box_d2 [n,7] the walk's squared box distance from query i to the
 * level-l node (2^l cells per axis) that holds point i, l = 0..6 -- a LOWER BOUND of the float64 (dx*dx + dy*dy) + dz*dz of the
 * pair; h_radius2 [n,7] squared distance from query i to the nearest face of the 3 x 3 x 3 level-l nodes around its own (+inf
 * where the grid ends first): no point outside those 27 nodes is nearer; h_lvl_off [8] offsets of the level tables 1..7 ([0] = 0). */
int vg_cluster_geom_probe(const double* h_origin_in, const float* h_bbox_lo, const float* h_bbox_hi, const float* h_points,
                          const float* h_queries, int n, double* h_origin, int32_t* h_cell, uint32_t* h_code, double* h_box_d2,
                          double* h_radius2, int64_t* h_lvl_off);

/* PP / ephemerality score from the per-neighbour-frame counts (pointcloud_utils.py:110-117 compute_ephe_score):
 * d_counts [n_frames][nq] int32 (row f = counts against neighbour frame f); seek_row >= 0: that row is the query frame
 * itself, 1 is subtracted (pointcloud_utils.py:90-91).  P = c / (sum c + 1e-8), H = sum(-P log(P + 1e-8)) / log(n_frames),
 * float64, sums in numpy's pairwise order.  d_H [nq] f64. */
int vg_entropy_scores(const int32_t* d_counts, int n_frames, int nq, int seek_row, double* d_H, void* stream);

/* Counter-based replacement for `np.random.choice(n, n / n_frames, replace=False)` (zero_shot_detector.py:228):
 * d_keys[i] = splitmix64(seed * 0x100000001B3 + (tag << 32) + i) >> 1; the caller keeps the n / n_frames smallest keys
 * (stable order).  tag = absolute frame number. */
int vg_subsample_keys(uint64_t seed, uint64_t tag, int n, int64_t* d_keys, void* stream);

/* ---- frame transform, validity filters, boxes (rows B1, B4, C1, C2, E1) --------------------------------
 * dst[i] = float32(T * [src[i],1]), other columns copied: LidarFrame.points_ref
 * (src/vilgod/lidar_frame.py:66-69 -> src/utils/pointcloud_utils.py:21-46). */
int vg_ref_transform(const float* d_src, int n, int stride, const double* d_T4x4, float* d_dst, void* stream);

/* Ground plane by RANSAC: LidarFrame.ground_plane_model_ref (lidar_frame.py:96-109) -> fit_plane
 * (pointcloud_utils.py:375-387) -> pyransac3d.Plane.fit (un-vendored).  Same algorithm (3-point hypotheses,
 * |distance| <= thresh inlier count, first strictly best of `iters`), sample indices from a counter-based hash of
 * (seed, iteration) instead of python's global `random`.  Call twice (all ground points, then the inliers) like
 * fit_plane does.  d_index: optional index list (NULL = first n rows).  d_work: iters*36+64 bytes scratch. */
int vg_plane_ransac(const float* d_points, int stride, const int32_t* d_index, int n, double thresh, int iters,
                    uint64_t seed, void* d_work, double* d_plane4, uint8_t* d_flags, int32_t* d_count, void* stream);

/* Detection.filter with the three active filters of tools/configs/preprocessor/waymo.yaml:16-49
 * (src/dataclass/objects.py:158-181; src/utils/cluster_utils.py:14-15 number_points, :48-49 height,
 * :51-60 plane_distance; all `and` + `required`).  Clusters = segments of d_index (packed point indices into
 * d_points).  d_stats6[c] = {n, zmin, zmax, dmin, dmax, height}; d_valid[c] = 0/1.  Thresholds are inclusive on both sides.
 * Plane distance = (((a x + b y) + c z) + d) / sqrt((a^2 + b^2) + c^2) in float64 (the plane need not be unit length), its extremes
 * rounded to float32 in d_stats6.  An empty segment keeps the reductions' identities (zmin = dmin = +inf, zmax = dmax = -inf,
 * height = -inf, n = 0) and is not valid; vg_cluster_filter_ex does the same. */
int vg_cluster_filter(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                      const double* d_plane4, int min_points, int max_points, double max_min_height, double min_max_height,
                      double min_height, double max_height, float* d_stats6, uint8_t* d_valid, void* stream);

/* Detection.filter with ANY of the filters of src/utils/cluster_utils.py and the and / or / required combination of
 * src/dataclass/objects.py:158-181 (cluster_utils.py:66-89 validate_cluster is the same formula):
 *   valid = (all(and) or any(or)) and all(and + required),   all([]) = True, any([]) = False.
 * Filters, in the order of d_verdict's columns:
 *   number_points  cluster_utils.py:14-15      height          :48-49 (float32 height, objects.py:112-114)
 *   aspect_ratio   :17-23 (float32 extents and division; x/0 = inf, 0/0 = nan compare false; `size < 1.0` exemption)
 *   volume         :25-35   area  :37-46: convex hull of xy with exact float64 orientation tests, shoelace area in float64
 *                  (the reference: qhull + a float32 shoelace, pointcloud_utils.py:123-126), volume = area * float32 height;
 *                  fewer than 3 points -> false; a degenerate hull (collinear / identical points: the reference dies with
 *                  QhullError) -> area 0, verdict `0 >= min_area`, VG_FILTER_FLAG_DEGENERATE; more than 1024 hull vertices ->
 *                  verdicts 0 and VG_FILTER_FLAG_HULL_OVERFLOW: the caller must compute that cluster's area itself
 *   plane_distance :51-60   ephemeral_score :62-64: np.percentile(scores, percentile) (linear method: the two order statistics
 *                  at floor(t(n-1)) and the next by an exact radix select, combined in float64), verdict `not (q > min score)`
 * number_points, height and plane_distance use the arithmetic of vg_cluster_filter: the same bits through either entry.
 * d_scores: float32 per ROW of d_points (indexed like d_points by d_index); may be NULL unless ephemeral_score is active.
 * d_stats[c][VG_FILTER_NSTATS] (float64) = {n, zmin, zmax, dmin, dmax, height, size_x, size_y, aspect ratio, area, volume,
 *   hull vertices, flags, percentile value, sum(|x_i y_j| + |x_j y_i|) over the hull edges, 0}
 * d_verdict[c][VG_FILTER_COUNT]: every ACTIVE filter's own verdict (Detection.filter_dict), 0 for inactive ones;
 * d_valid[c]: the combination. */
#define VG_FILTER_NUMBER_POINTS 0
#define VG_FILTER_HEIGHT 1
#define VG_FILTER_ASPECT_RATIO 2
#define VG_FILTER_VOLUME 3
#define VG_FILTER_AREA 4
#define VG_FILTER_PLANE_DISTANCE 5
#define VG_FILTER_EPHEMERAL_SCORE 6
#define VG_FILTER_COUNT 7
#define VG_FILTER_NSTATS 16
#define VG_FILTER_AND_REQUIRED 0   /* logic: and, required: True */
#define VG_FILTER_AND 1            /* logic: and */
#define VG_FILTER_OR 2             /* logic: or */
#define VG_FILTER_FLAG_DEGENERATE 1
#define VG_FILTER_FLAG_HULL_OVERFLOW 2
typedef struct vg_filter_params {
    int active[VG_FILTER_COUNT];
    int logic[VG_FILTER_COUNT];
    int min_points, max_points;
    int has_max_volume, has_max_area;      /* cluster_utils.py:33,44: optional kwargs */
    double min_height, max_height;
    double min_aspect_ratio, max_aspect_ratio;
    double min_volume, max_volume;
    double min_area, max_area;
    double max_min_height, min_max_height;
    double percentile, min_percentile_pp_score;
} vg_filter_params;
void vg_filter_default_params(vg_filter_params* p);    /* nothing active, every threshold open */
int vg_cluster_filter_ex(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                         const double* d_plane4, const float* d_scores, const vg_filter_params* p, double* d_stats,
                         uint8_t* d_verdict, uint8_t* d_valid, void* stream);

/* fit_bounding_boxes_simple, static branch (src/vilgod/zero_shot_detector.py:444-462) with
 * method minimum_bounding_rectangle (pointcloud_utils.py:309-372): d_box7[c] = {cx,cy,cz,l,w,h+0.3,rz} float64 in
 * the frame of d_points.  All hull edges are tried (the reference omits the closing edge of qhull's vertex cycle, :329-330; see
 * DESIGN.md).  d_aux3[c] = {hull vertices, rectangle area, flag}:
 *   hull vertices  the strict vertices of the exact convex hull of the xy points (collinear points and duplicates are none): 1 for
 *                  identical points, 2 for collinear ones (ABI 1 wrote 0 for both), at most VG_BOX_MAX_HULL
 *   flag 0                          the rectangle of smallest area over the edges of the whole hull
 *   VG_BOX_FLAG_DEGENERATE (1)      fewer than 3 hull vertices (the reference: qhull raises, :320-326): the 0.1 m square at the float64
 *                                   mean of the points, rz = 0, area 0
 *   VG_BOX_FLAG_HULL_OVERFLOW (2)   more than VG_BOX_MAX_HULL hull vertices (a dense ring).  The wrapping stops there, with the part
 *                                   of the outline that lies counter-clockwise from the lowest point, and NO rectangle is fitted:
 *                                   cx, cy, l, w, rz = NaN, area 0, hull vertices = VG_BOX_MAX_HULL; cz and h are valid.  The caller
 *                                   must fit that cluster itself (vilgod_amd/boxes.py all_edges_box; ABI 1 returned the
 *                                   rectangle of the partial outline, flag 0). */
#define VG_BOX_MAX_HULL 512
#define VG_BOX_FLAG_DEGENERATE 1
#define VG_BOX_FLAG_HULL_OVERFLOW 2
int vg_cluster_boxes(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                     double* d_box7, float* d_aux3, void* stream);

/* fit_bounding_boxes_simple, static branch (src/vilgod/zero_shot_detector.py:451, :477, :672) with method closeness_rectangle
 * (criterion 0, src/utils/pointcloud_utils.py:170-229) or variance_rectangle (criterion 1, :231-288): the L-shape search over
 * the angles of d_angle_table, the first angle of the largest criterion, the rectangle there and the box of zero_shot_detector.py:452-461.
 * d_angle_table: [n_angles][VG_LSHAPE_TABLE_STRIDE] float64 rows {cos a, sin a, cos(a + pi/2), sin(a + pi/2), a, a + pi/2,
 * a + pi/2 + pi/2, (a + pi/2) + pi/2} with a = np.arange(0, 90 + delta, delta)[k] / 180 * np.pi; cos / sin rounded to float32 for
 * closeness (the reference's components dtype).  delta_zero: closeness only (> 0).  d_work: [n_clusters, n_angles] float64, the
 * criterion of every (cluster, angle).  d_box7[c] = {cx,cy,cz,l,w,h+0.3,rz}; d_aux[c] = {chosen angle index, its criterion, rz
 * before the l/w swap}.  VG_ERR_ARG before any device work for a bad criterion, n_angles outside [1, VG_LSHAPE_MAX_ANGLES]
 * (delta >= 0.01 degrees), delta_zero <= 0 with closeness, or null pointers with n_clusters > 0; n_clusters == 0 is a no-op. */
#define VG_LSHAPE_CLOSENESS 0
#define VG_LSHAPE_VARIANCE 1
#define VG_LSHAPE_TABLE_STRIDE 8
#define VG_LSHAPE_MAX_ANGLES 9001
int vg_cluster_lshape(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                      int criterion, const double* d_angle_table, int n_angles, double delta_zero, double* d_work,
                      double* d_box7, double* d_aux, void* stream);

/* Rotated-box IoU: pcdet's boxes_iou3d_gpu / boxes_iou_bev, which the reference calls in src/utils/tracking_utils.py:9-20,
 * src/vilgod/zero_shot_detector.py:737-739 and src/datasets/waymo_dataset.py:300.  Boxes are rows of 7 values
 * {x, y, z, dx, dy, dz, heading}, float32 (dtype VG_IOU_F32, widened exactly) or float64 (VG_IOU_F64); all arithmetic is float64.
 * Grouped: one call covers n_groups independent matrices.  Group g pairs the a rows [a_off[g], a_off[g+1]) with the b rows
 * [b_off[g], b_off[g+1]) and writes its row-major [na_g, nb_g] matrix at d_out + out_off[g].  a_off / b_off: n_groups + 1 entries,
 * non-decreasing; out_off: n_groups entries, >= 0, each group's range behind the one before (gaps allowed).  Elements of d_out that
 * belong to no group are never written.  The plain N x M call is n_groups = 1.
 *   mode VG_IOU_3D        BEV intersection area x z overlap / (vol_a + vol_b - intersection); 0 where the union is not positive
 *        VG_IOU_BEV       BEV intersection area / (area_a + area_b - intersection); z and dz are not read
 *        VG_IOU_BEV_AREA  the BEV intersection area
 * Exactly 0.0 for an extent <= 0 (dx, dy; dz too in mode VG_IOU_3D), for no z overlap (VG_IOU_3D) and for centres farther apart than
 * the half-diagonals allow.  |heading| < 1.6e6 (beyond: NaN).  The geometry is formed relative to b's centre, so the value does not
 * depend on where the pair stands.
 * vg_boxes_iou3d: device pointers; reads the three offset tables back first (one stream synchronisation; not capturable into a
 * graph), then one launch with one lane per output element.  vg_boxes_iou3d_host: the same per-pair code (csrc/iou_pair.inc)
 * over host arrays, no GPU needed; the two agree bit for bit.
 * VG_ERR_ARG: dtype or mode unknown, n_groups < 0, offsets that break the rules above, null pointers with non-empty work.
 * n_groups == 0 or only empty groups: VG_OK, nothing launched (d_a / d_b / d_out may then be NULL). */
#define VG_IOU_F32 0
#define VG_IOU_F64 1
#define VG_IOU_3D 0
#define VG_IOU_BEV 1
#define VG_IOU_BEV_AREA 2
int vg_boxes_iou3d(int dtype, const void* d_a, const int32_t* d_a_off, const void* d_b, const int32_t* d_b_off,
                   int n_groups, const int64_t* d_out_off, int mode, double* d_out, void* stream);
int vg_boxes_iou3d_host(int dtype, const void* h_a, const int32_t* h_a_off, const void* h_b, const int32_t* h_b_off,
                        int n_groups, const int64_t* h_out_off, int mode, double* h_out);

/* Rotated-box NMS: pcdet's iou3d_nms_utils.nms_gpu / nms_normal_gpu, the two functions of the module the reference imports
 * (src/utils/tracking_utils.py:6, src/vilgod/zero_shot_detector.py:17, src/datasets/waymo_dataset.py:3) next to the IoU above.
 * Grouped: one call runs n_groups independent NMS passes; group g is the rows [off[g], off[g+1]) of d_boxes / d_scores (off:
 * n_groups + 1 entries, non-decreasing, inside [0, n_rows]).  Boxes are rows of 7 values {x, y, z, dx, dy, dz, heading}, float32
 * (VG_NMS_F32, widened exactly) or float64 (VG_NMS_F64); z and dz are not read.  Scores: float32 or float64.  Per group:
 *   order      rows are ranked by the strict total order (score descending, row index ascending); +0.0 and -0.0 are one score; a NaN
 *              score ranks behind every number
 *   padding    a row whose score is NaN, or one of whose x, y, dx, dy, heading is not finite, is never kept and suppresses nothing
 *              (it keeps its rank).  The rule is this project's own, in both modes
 *   pre_max    > 0: only the first pre_max ranked rows of each group take part (pcdet's pre_maxsize), the others are not kept;
 *              <= 0: all take part
 *   greedy     walking the ranked rows, a row q is kept iff no earlier-KEPT row p has v(q, p) > thresh: strict, and a NaN value
 *              compares false (|heading| >= 1.6e6 gives one).  v(q, p) is the mode's value with a = row q (the later one) and
 *              b = row p (the kept one): the geometry is formed in b's frame and is not bit-symmetric, so the operand order is
 *              part of the contract
 *   mode VG_NMS_ROTATED   v = the VG_IOU_BEV value of vg_boxes_iou3d (csrc/iou_pair.inc), as in nms_gpu
 *        VG_NMS_NORMAL    v = the axis-aligned BEV IoU with the headings ignored, as in nms_normal_gpu (csrc/nms_pair.inc): float64,
 *                         relative to b's centre, d = centre_a - centre_b, ix = min(d.x + ahx, bhx) - max(d.x - ahx, -bhx), iy alike;
 *                         exactly 0.0 for an extent <= 0, an overlap <= 0 on either axis or a union <= 0, else inter / (Sa + Sb - inter)
 * Outputs: d_keep int32, one slot per input row: the kept rows of group g as GLOBAL row indices, best first, at
 * off[g] .. off[g] + count[g] - 1, the rest of the group's slots -1; slots that belong to no group are never written.
 * d_count int32 [n_groups].
 * vg_boxes_nms: device pointers, three launches on `stream` (csrc/nms.hip: counting rank, ballot mask over the upper triangle, one
 * wave per group for the greedy pass), sized from n_groups, n_rows and max_group alone: no read-back, no synchronisation, no
 * allocation, no atomics -- it can be captured into a graph and gives the same bits on every run.  max_group is the caller's upper
 * bound on any group's size, at most VG_NMS_MAX_GROUP.  A group the table describes wrongly (larger than max_group, reaching outside
 * [0, n_rows], negative size) does not fault: its count is -1 and those of its rows that exist get -1, written by the kernels.
 * d_work: vg_boxes_nms_work_bytes(n_rows, max_group, n_groups) bytes (the ranks and the mask: n_rows * (4 + 8 * ceil(max_group / 64))
 * rounded up to 8), contents irrelevant before and after; one call at a time per work buffer.
 * vg_boxes_nms_host: the same arguments over host arrays, no work buffer, the same per-pair and per-row code; the two agree bit
 * for bit (identical keep lists and counts).  No GPU needed.
 * VG_ERR_ARG (nothing launched): dtype or mode unknown, a negative n_groups / n_rows / max_group, max_group > VG_NMS_MAX_GROUP, null
 * pointers with non-empty work.  n_groups == 0 or n_rows == 0: VG_OK, nothing launched, nothing written. */
#define VG_NMS_F32 0
#define VG_NMS_F64 1
#define VG_NMS_ROTATED 0
#define VG_NMS_NORMAL 1
#define VG_NMS_MAX_GROUP 4096
int vg_boxes_nms(int box_dtype, const void* d_boxes, int score_dtype, const void* d_scores, const int32_t* d_off, int n_groups,
                 int n_rows, int max_group, int mode, double thresh, int pre_max, void* d_work, int32_t* d_keep, int32_t* d_count,
                 void* stream);
size_t vg_boxes_nms_work_bytes(int n_rows, int max_group, int n_groups);
int vg_boxes_nms_host(int box_dtype, const void* h_boxes, int score_dtype, const void* h_scores, const int32_t* h_off, int n_groups,
                      int n_rows, int max_group, int mode, double thresh, int pre_max, int32_t* h_keep, int32_t* h_count);

/* Linear assignment: scipy.optimize.linear_sum_assignment, which the reference reaches in src/datasets/waymo_eval.py:111 (the
 * matcher inside the detection metric) and calls in src/utils/tracking_utils.py:23-51.  Grouped: one call solves n_groups independent
 * problems.  Group g has n_g = row_off[g+1] - row_off[g] rows and m_g = col_off[g+1] - col_off[g] columns, and its row-major float64
 * cost matrix [n_g, m_g] starts at d_cost + cost_off[g]: the offset tables of vg_boxes_iou3d (a_off, b_off, out_off), so that kernel's
 * output can be this one's input.  cost_len: the elements of d_cost.
 *   problem     minimise the summed cost over injective partial assignments of rows to columns; a row may stay unassigned at the
 *               price unassigned_cost (one double per call; NaN or -inf: VG_ERR_ARG).  +INFINITY: every row takes a column, the
 *               classic problem, which needs n_g <= m_g.  An entry of +INFINITY forbids that pair.  Entries and prices whose sums
 *               overflow float64 are outside the contract.
 *   order       d_order (may be NULL: row order): int32, the entries row_off[g] .. row_off[g] + n_g - 1 are a permutation of
 *               0 .. n_g - 1, the order in which group g's rows enter; n_rows: the entries of d_order (not read without it)
 *   snapshots   after the k-th row has entered, the state is an optimal assignment of the first k rows.  d_prefix lists, per group,
 *               strictly ascending prefix lengths in 1 .. n_g: group g's are d_prefix[prefix_off[g] .. prefix_off[g+1]) (prefix_off:
 *               n_groups + 1 entries inside [0, n_snaps]).  Snapshot s (an index into d_prefix) is the group's col4row after
 *               d_prefix[s] rows, n_g int32 at d_match + match_off[s]: the row's column, -1 for a row unassigned or not yet entered.
 *               d_prefix == NULL (then prefix_off == NULL and n_snaps == n_groups): one snapshot per group after its last row, at
 *               match_off[g].  match_len: the elements of d_match; what belongs to no snapshot is never written.
 *   status      d_status int32 [n_groups]: 0 solved; 1 infeasible (a row with no finite choice left); 2 an entry is NaN or -INFINITY;
 *               -1 the tables describe the group wrongly (n_g or m_g negative or above max_rows / max_cols, a matrix outside
 *               [0, cost_len), order entries outside [0, n_rows), out of range or repeated, a prefix range outside [0, n_snaps], a
 *               prefix length outside 1 .. n_g or not ascending, a snapshot outside [0, match_len)).  For any status but 0 every
 *               snapshot of the group that lies inside d_match is filled with -1 (min(n_g, max_rows) entries).  Both forms check what
 *               they read: nothing is read or written out of range.
 *   algorithm   shortest augmenting paths with dual variables (the algorithm scipy uses), float64 throughout.  The next column is the
 *               one of smallest path cost; among equal costs a free column wins, then the lowest column index, "stay unassigned"
 *               counting as a free column behind all real ones (row i's is column m_g + i).  This tie rule is the project's own:
 *               scipy's order among ties depends on its internal permutation and cannot be restated in parallel.  Where the optimum
 *               is unique the assignments are scipy's; among ties the total is.
 * vg_lap_groups: device pointers; ONE launch on `stream` (csrc/lap.hip: one wave per group), sized from n_groups, max_rows and max_cols
 * alone: no read-back, no synchronisation, no allocation, no atomics -- it can be captured into a graph and gives the same bits on
 * every run.  max_rows / max_cols: the caller's upper bounds on any group's size, at most VG_LAP_MAX each.
 * vg_lap_groups_host: the same arguments over host arrays, the same per-column steps (csrc/lap_step.inc) run one after the other; the
 * two agree bit for bit in every snapshot and status, ties included.  No GPU needed.
 * VG_ERR_ARG (nothing launched): a negative count or length, max_rows / max_cols above VG_LAP_MAX, unassigned_cost NaN or -INFINITY,
 * d_prefix without prefix_off or the reverse, d_prefix == NULL with n_snaps != n_groups, null pointers with non-empty work.
 * n_groups == 0: VG_OK, nothing launched. */
#define VG_LAP_MAX 1024
int vg_lap_groups(const double* d_cost, int64_t cost_len, const int64_t* d_cost_off, const int32_t* d_row_off,
                  const int32_t* d_col_off, int n_groups, int n_rows, int max_rows, int max_cols, double unassigned_cost,
                  const int32_t* d_order, const int32_t* d_prefix, const int32_t* d_prefix_off, int n_snaps,
                  const int64_t* d_match_off, int64_t match_len, int32_t* d_match, int32_t* d_status, void* stream);
int vg_lap_groups_host(const double* h_cost, int64_t cost_len, const int64_t* h_cost_off, const int32_t* h_row_off,
                       const int32_t* h_col_off, int n_groups, int n_rows, int max_rows, int max_cols, double unassigned_cost,
                       const int32_t* h_order, const int32_t* h_prefix, const int32_t* h_prefix_off, int n_snaps,
                       const int64_t* h_match_off, int64_t match_len, int32_t* h_match, int32_t* h_status);

/* Points in boxes: pcdet's roiaware_pool3d_utils.points_in_boxes_gpu, which the reference calls in src/utils/pointcloud_utils.py:144-158
 * (get_box_heights) and :516-522 (points_in_boxes; src/vilgod/lidar_frame.py:154-161 turns box proposals into detections with it).
 * Per point the LOWEST index of a box that contains it, -1 when none does.  A box is a row of 7 values {cx, cy, cz, dx, dy, dz, rz},
 * float32 (box_dtype VG_PIB_F32, widened exactly) or float64 (VG_PIB_F64); a point is the first three floats of a row of
 * point_stride floats.  The point (x, y, z) is inside iff
 *     fabs(z - cz) <= dz / 2                                        (the z faces belong to the box)
 *     fabs(lx) < dx / 2 + 1e-5  and  fabs(ly) < dy / 2 + 1e-5      (strict, beyond a margin of 1e-5)
 *     lx = sx cos(rz) + sy sin(rz), ly = -sx sin(rz) + sy cos(rz), (sx, sy) = (x - cx, y - cy)
 * with all arithmetic in float64 (pcdet: float32) and the sine / cosine of csrc/iou_pair.inc.  The rule is positive: a NaN anywhere in
 * the point or the box, an extent that is not >= 0 and |rz| >= 1.6e6 all mean "outside".
 * Batched: element b reads the points [b * n_points, (b + 1) * n_points), the boxes [b * n_boxes, (b + 1) * n_boxes) and writes
 * d_box_idx [b * n_points ..], indices counted inside the element.
 * vg_points_in_boxes: device pointers; ONE launch on `stream` (csrc/points_in_boxes.hip: one lane per point, the boxes through LDS in
 * chunks of VG_PIB_CHUNK), no read-back, no allocation, no synchronisation, no atomics -- it can be captured into a graph and gives the
 * same bits on every run.  vg_points_in_boxes_host: the same per-pair code (csrc/points_in_boxes_pair.inc) over host arrays, no GPU
 * needed; the two agree bit for bit.
 * n_boxes == 0: every index is -1 (d_boxes may be NULL).  n_points == 0 or batch == 0: VG_OK, nothing launched, nothing read.
 * VG_ERR_ARG (nothing launched): box_dtype unknown, a negative count, point_stride < 3, null pointers with non-empty work.
 * VG_ERR_CAPACITY: batch > 65535 (device form). */
#define VG_PIB_F32 0
#define VG_PIB_F64 1
#define VG_PIB_CHUNK 256
int vg_points_in_boxes(int box_dtype, const float* d_points, int point_stride, int n_points, const void* d_boxes, int n_boxes,
                       int batch, int32_t* d_box_idx, void* stream);
int vg_points_in_boxes_host(int box_dtype, const float* h_points, int point_stride, int n_points, const void* h_boxes, int n_boxes,
                            int batch, int32_t* h_box_idx);

/* Detection.cluster_mass_center (src/dataclass/objects.py:121-123: np.median(cluster_points, axis=0)) of every packed cluster over the
 * first n_cols columns of the point rows (the tracker reads all five: src/vilgod/tracker.py:52-59, objects.py:238-306).  Exact
 * order statistics; an even count gives the float32 mean of the two middle values like np.median.  d_median: [n_clusters, n_cols] f32. */
int vg_cluster_medians(const float* d_points, int stride, int n_cols, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                       float* d_median, void* stream);

/* Oriented extents: the per-point part of the motion-aligned boxes of moving tracks (the reference's fit_bounding_boxes_simple,
 * src/vilgod/zero_shot_detector.py:576-603: `np.dot(pts[:, :3] - center, rot)`, its min / max per column, min / max of z).
 * A PAIR is (cluster, direction).  Pair p reads cluster c = d_pair_cluster[p] (NULL: c = p, and then n_pairs == n_clusters), whose
 * points are d_index[d_seg_off[c] .. d_seg_off[c + 1]), rows of `stride` floats as in vg_cluster_medians; the same cluster may sit in
 * several pairs.  d_center3[p]: float32 {cx, cy, cz}, the cluster's median.  d_rot4[p] = {r00, r01, r10, r11}, float64: the upper-left
 * 2 x 2 of the direction's rotation matrix exactly as the host built it (scipy's goes through a quaternion: not cos / sin).  Per point
 *     float  dx = x - cx,  dy = y - cy;                      (float32, rounded once)
 *     double px = fma((double)dy, r10, (double)dx * r00);    double py = fma((double)dy, r11, (double)dx * r01);
 * which is what np.dot gives for float32 points and centre and a float64 matrix whose third row and column are (0, 0, 1).
 * d_ext6[p] = {min px, max px, min py, max py, min z, max z}, float64, z the point's own float32 z widened; a zero is written as +0.
 * Six NaN for: a cluster without points, a pair index outside [0, n_clusters) (no point is read), and a pair with anything
 * non-finite in it -- a point's x, y or z, the centre, or a projection (numpy would poison only the affected columns).
 * vg_cluster_oriented_extents: device pointers; ONE launch on `stream` (csrc/oriented_extent.hip: one workgroup of VG_OEXT_BLOCK
 * threads per pair), no read-back, no allocation, no synchronisation, no atomics -- it can be captured into a graph; min / max do not
 * depend on the order of reduction, so every run gives the same bits.  vg_cluster_oriented_extents_host: the same per-point code
 * (csrc/oriented_extent_point.inc) over host arrays, no GPU needed; the two agree bit for bit.
 * VG_ERR_ARG before any device work: a negative count, stride < 3, and with n_pairs > 0: d_pair_cluster == NULL with
 * n_pairs != n_clusters, null pointers with non-empty work.  n_pairs == 0 (valid counts and stride): VG_OK, nothing launched. */
#define VG_OEXT_BLOCK 1024
int vg_cluster_oriented_extents(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                                const int32_t* d_pair_cluster, int n_pairs, const float* d_center3, const double* d_rot4,
                                double* d_ext6, void* stream);
int vg_cluster_oriented_extents_host(const float* h_points, int stride, const int32_t* h_index, const int32_t* h_seg_off, int n_clusters,
                                     const int32_t* h_pair_cluster, int n_pairs, const float* h_center3, const double* h_rot4,
                                     double* h_ext6);

/* ---- execution resources (no reference counterpart: the reference has one implicit CUDA stream) -------------
 * A HIP stream whose kernels may only be dispatched to the compute units set in h_cu_mask (hipExtStreamCreateWithCUMask):
 * n_words 32-bit words, bit i of the mask = CU slot i.  On gfx950 in SPX mode the driver deals the mask bits round-robin over the
 * 8 XCDs and, inside an XCD, over its shader engines (bit i -> XCD i % 8), so the low 8 r bits are r CUs of every XCD.
 * Used to keep the small latency-bound kernels of a frame's front stage (ground, clustering, render) off the CUs the projection
 * GEMMs of other frames' ViT passes need whole; numerics cannot depend on it.
 * vg_device_cu_count: compute units of the current device. */
int vg_stream_create_cu_mask(void** out_stream, const uint32_t* h_cu_mask, int n_words);
int vg_stream_destroy(void* stream);
int vg_device_cu_count(int32_t* h_count);

#ifdef __cplusplus
}
#endif
#endif
