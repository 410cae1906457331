// CLIP ViT image tower + zero-shot scoring for gfx950.
//
// Replaces third_party/CLIP/clip/model.py:206-240 (VisionTransformer.forward), :171-192
// (ResidualAttentionBlock), :157-168 (LayerNorm in fp32, QuickGELU) as called from
// src/utils/clip_utils.py:39-44 (encode_image -> normalise -> 100*cos -> softmax).
//
// Two precisions, one code path:
//   dtype 1 (f16): GEMM operands and activations fp16, fp32 accumulate, fp32 LayerNorm -- what the
//                  reference runs on a GPU (model.py:375-396 convert_weights) -- except that the
//                  residual stream is kept in fp32 (strictly more accurate than the reference's fp16
//                  stream).  Projection GEMMs: k_gemm_f16_pp64 (v_mfma_f32_16x16x32_f16, 256 x 256 x 64 tiles, 8 waves as two
//                  groups one barrier apart, LDS-DMA rings, LayerNorm folded into the epilogues); shapes with N % 256 != 0:
//                  k_gemm_f16 (256 x 128 x 32).  Attention: persistent workgroups, item = (crop, head), K and V row-major in
//                  LDS, S^T = K Q^T and O^T = V^T P^T both on MFMA with the softmax row living on one lane.
//   dtype 0 (f32): parity mode against the fp32 CPU reference (tolerance 1e-3 on probabilities): the same tower in fp32 --
//                  k_gemm_f32_mfma (v_mfma_f32_32x32x2_f32, 128 x 128 tiles; bit-identical to the vector-ALU k_gemm_f32 that
//                  serves the other shapes), k_attention_f32, k_layernorm -- same epilogues.
//
// Layout (all row-major, K contiguous):
//   tokens M = n_crops * T (T = 1 + (res/patch)^2), rows padded to a multiple of 256 (the padding rows of the
//   residual stream are re-zeroed by k_embed_lnpre on every call; the other buffers' padding rows are written by
//   the GEMMs from them and stay finite).
//   x    [Mp, W]   f32   residual stream
//   h    [Mp, W]   f16|f32   LayerNorm output / attention output
//   qkv  [Mp, 3W]  f16|f32
//   mlp  [Mp, 4W]  f16|f32
//
// One translation unit, split by stage (the includes are compiled in place, in this order; vit.hip is the only source the build names):
//   vit.hip                  this file: the switches (VitSwitches::from_env: the one reader of the environment; vit_resolve_switches), GemmCfg,
//                            GemmProfile, the handle vg_vit, then
//     vit_gemm_kernels.inc   the EPI enum, k_gemm_f16, k_gemm_f32, k_gemm_f32_mfma, k_gemm_f16_pp64, k_gemm_f16_w4 (K loop: gemm_w4_loop.inc,
//                            written by gen_gemm_w4.py), k_splitk_resid
//     vit_gemm_launch.inc    tile order, splitk_plan, gemm_family (which kernel), launch_gemm_pp64 / _w4 / _resid_tail, launch_gemm (the launch path)
//     vit_attention.inc      k_attention_f16 (plain and causal), k_attention_f16_long, k_attention_f32 (plain and causal), launch_attention[_causal / _f32]
//     vit_stage_kernels.inc  k_im2col, k_embed_lnpre, k_layernorm, k_head, k_ln_fold, k_conv1_fold, class-row gather / scatter
//     vit_scores.inc         k_clip_scores, k_clip_scores_wide, vg_clip_scores, vg_clip_scores_wide
//                            weights by role (vit_weights), the folds (vit_fold_ln, vit_fold_conv1), vg_vit_create / _destroy / _set_weight,
//                            the encode plan (vit_plan), one encode (VitRun, vg_vit_encode), the kernel-level test entry points
//                            (vg_attention*, vg_gemm*), vg_vit_profile*
//     vit_text.inc           the CLIP text tower on VitRun: k_text_embed, vg_text_create / _destroy / _set_weight / _workspace_bytes / _encode
//     vit_graph.inc          the graph cache, vg_vit_classify_graph
//   dev/*.inc                development build only (-DVG_DEV): superseded kernels, ablations, trace entry points, behind one-line hooks
#include "common.h"
#include <hip/hip_fp16.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <map>
#include <atomic>
#include <mutex>
#include <memory>
#include <type_traits>
#include <assert.h>
#include <utility>

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// Environment switches (VG_*).  VitSwitches::from_env is the one reader of the product text: vg_vit_create calls it ONCE per handle --
// never per launch: getenv is not safe against a concurrent setenv, the worker threads launch concurrently, and a captured graph must
// replay what the plain launches of the same handle run -- and the handle-less entry points (vg_gemm, vg_gemm_family,
// vg_gemm_ln, vg_gemm_ln_partial_cols, vg_gemm_resid_splitk, vg_attention, vg_attention_rows) call it per call, on the caller's thread
// (the tests set the environment between such calls).  env_on: any value that parses to 0 is "off"; unset = `dflt`.
static int env_int(const char* name, int dflt) { const char* s = getenv(name); return s ? atoi(s) : dflt; }
static bool env_on(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

// the fp16 attention's A/B switches: row-major V + transposing LDS reads (VG_ATT_TR), SIMD partners apart in phase (VG_ATT_STAGGER, k_attention_f16 STAG)
struct AttOptions { bool tr = true, stagger = true; };

struct VitSwitches {                 // the environment as it is, plain data; what a tower makes of it: vit_resolve_switches
    int gemm_w4;                     // VG_GEMM_W4 (1): projection GEMMs by k_gemm_f16_w4 (round 6: persistent, 4 waves, assembly K loop); 0: k_gemm_f16_pp64
                                     // (a tower uses one family: their LayerNorm partials differ in granularity)
    bool f32_mfma;                   // VG_GEMM_F32_MFMA (on): fp32 tower on the matrix cores
    int splitk_max;                  // VG_GEMM_SPLITK (0): opt-in split-K tail of the residual GEMMs (splitk_plan)
    bool cls_last;                   // VG_VIT_CLS_LAST (on): last block on the class-token rows only (see vit_plan)
    bool resid16;                    // VG_VIT_RESID16 (unset; ANY value sets it): fp16 residual stream
    bool ln_fold;                    // VG_VIT_LN_FOLD (on): LayerNorm folded into the GEMMs around it
    bool resid_hl;                   // VG_VIT_RESID_HL (on): the residual stream as an fp16 pair
    AttOptions att;                  // VG_ATT_TR (on), VG_ATT_STAGGER (on)
    static VitSwitches from_env() {
        return {env_int("VG_GEMM_W4", 1), env_on("VG_GEMM_F32_MFMA", true), env_int("VG_GEMM_SPLITK", 0), env_on("VG_VIT_CLS_LAST", true),
                getenv("VG_VIT_RESID16") != nullptr, env_on("VG_VIT_LN_FOLD", true), env_on("VG_VIT_RESID_HL", true),
                {env_on("VG_ATT_TR", true), env_on("VG_ATT_STAGGER", true)}};
    }
};

// what launch_gemm needs to know to pick and launch a projection GEMM (vit_gemm_launch.inc)
struct GemmCfg {
    int dtype, gemm_w4, splitk_max;
    bool f32_mfma;
#ifdef VG_DEV
    bool gemm_x2 = false;            // projection GEMMs by k_gemm_f16_x2 (dev_vit_create: VG_GEMM_X2)
#endif
};
static GemmCfg gemm_cfg(const VitSwitches& s, int dtype) { return {dtype, s.gemm_w4, s.splitk_max, s.f32_mfma}; }

// The switches as one tower runs with them (vg_vit's first members).
struct VitTower {
    GemmCfg gemm;                    // (gemm.dtype = the handle's dtype)
    AttOptions att;
    bool cls_last;
    bool resid_h;                    // opt-in (VG_VIT_RESID16=1, dtype 1, width % 256 == 0): fp16 residual stream like upstream's fp16 run.
                                     // +2.7 % frames/s, 3x the feature error (1.1e-3 vs 3.4e-4 rel. L2): default keeps the fp32 stream
    bool ln_fold;                    // LayerNorm folded into the GEMMs around it (k_gemm_f16_pp64 / k_gemm_f16_w4 LN = 1 / 2): fp16 tower with the fp32
                                     // residual stream and width % 256 == 0, unless VG_VIT_LN_FOLD=0
    bool resid_hl;                   // the residual stream kept as an fp16 PAIR (EPI_BIAS_RESID_HL; round 6, default for the k_gemm_f16_w4 tower with the folded
                                     // LayerNorm and the last block on the class rows; VG_VIT_RESID_HL=0: the fp32 stream): 22 bits of the stream, a third less
                                     // written by out_proj / c_proj -- features 1.8e-4 from the fp32-stream tower's, the same distance to the fp32 tower
};
static VitTower vit_resolve_switches(const VitSwitches& s, int dtype, int width) {
    VitTower t;
    t.gemm = gemm_cfg(s, dtype); t.att = s.att; t.cls_last = s.cls_last;
    t.resid_h = dtype == 1 && width % 256 == 0 && s.resid16;
    t.ln_fold = dtype == 1 && width % 256 == 0 && !t.resid_h && s.ln_fold;
    t.resid_hl = t.ln_fold && s.gemm_w4 && s.cls_last && width <= 1024 && s.resid_hl;
    return t;
}

// Compute units of the current device, queried once per device (one slot per device, like VgPerDeviceOnce in common.h: racing threads
// store the same value, so no lock).  A device that reports fewer than 8 counts as 256 (MI355X).  The persistent kernels launch one
// workgroup per CU, rounded up to a multiple of 8: slot s of XCD x = block 8 s + x (vg_persistent_grid).
static int vg_cu_count() {
    static std::atomic<int> count[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<int>& slot = count[dev & 63];
    int n = slot.load(std::memory_order_relaxed);
    if (!n) {
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        if (n < 8) n = 256;
        slot.store(n, std::memory_order_relaxed);
    }
    return n;
}
static int vg_persistent_grid(int tiles, int cap) { return ((tiles < cap ? tiles : cap) + 7) / 8 * 8; }

// Optional per-launch timing of a handle's projection GEMMs and fp16 attention launches (vg_vit_profile*, bench.py roofline): event
// pairs on the launch stream.  begin() opens a sample if there is room for one; end() closes the sample begin() opened.
#define VG_PROF_MAX 4096
struct GemmProfile {
    int on = 0, n = 0;
    bool init = false;
    hipEvent_t ev[2 * VG_PROF_MAX];
    double flops[VG_PROF_MAX];
    int kind[VG_PROF_MAX];           // 0 = k_gemm_f16 / k_gemm_f32, 1 = the 256 x 256 kernels (k_gemm_f16_w4 / k_gemm_f16_pp64), 2 / 3 = fp16 attention (all rows / class rows)
    bool begin(hipStream_t st) {
        if (!on || n >= VG_PROF_MAX) return false;
        (void)hipEventRecord(ev[2 * n], st);
        return true;
    }
    void end(hipStream_t st, int k, double fl) {
        (void)hipEventRecord(ev[2 * n + 1], st);
        kind[n] = k;
        flops[n++] = fl;
    }
};

struct VitWeights;
struct vg_vit : VitTower {
    int width, layers, heads, patch, res, out_dim, dtype, T;
    bool text = false;                     // a CLIP text tower (vg_text, vit_text.inc): T = the context length, causal attention, token-table front end
    GemmProfile prof;
    std::map<std::string, void*> w;        // device pointers (f32 or f16 depending on role)
    std::map<std::string, size_t> numel;
    // The fp32 originals of in_proj / c_fc stay on the device (w32) so that the folded LayerNorm's pre-scaled fp16 weights are rounded
    // once, from g[k] * W[n,k]; the derived tensors live in `w` under "<name>#ln" (weights), "#c1", "#c2" and are rebuilt when any of
    // their inputs is set again.
    std::atomic<bool> fold_ready{false};
    // vg_vit_classify_graph: one bit per launch form (classify_warm_slot, vit_graph.inc) that has run once as plain launches on this handle
    std::atomic<uint64_t> warmed[2] = {{0}, {0}};
    // single-channel patch rows (vg_vit_encode input_kind 3): per-channel input normalisation the fold assumes (clip.py:79-86; set by
    // vg_vit_set_input_norm) and the readiness of "conv1.weight#1ch" / "positional_embedding#1ch" (vit_fold_conv1)
    float in_mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, in_std[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    std::atomic<bool> conv1_ready{false};
    // bumped whenever a device tensor the kernels read is replaced (vg_vit_set_weight, vit_fold_ln): part of the captured graphs'
    // key, so a graph that holds pointers to freed weights is never replayed
    std::atomic<uint64_t> weights_gen{0};
    std::mutex mtx;
    std::map<std::string, void*> w32;
    // the tensors of `w` by role (vit_weights): resolved from the maps once per generation, shared by the encodes in flight
    std::shared_ptr<const VitWeights> resolved;
    uint64_t resolved_gen = 0;
};

static bool is_gemm_weight(const std::string& n) {
    return n == "conv1.weight" || n.find("in_proj_weight") != std::string::npos ||
           n.find("out_proj.weight") != std::string::npos || n.find("c_fc.weight") != std::string::npos ||
           n.find("c_proj.weight") != std::string::npos;
}

// K of the patch-embedding GEMM: 3 * patch^2 rounded up to a multiple of 64 (ViT-L/14: 588 -> 640; patch 16 / 32: unpadded).  The
// im2col rows and conv1.weight's rows carry zero columns up to it.
static int vit_kpad(const vg_vit* v) { return (3 * v->patch * v->patch + 63) / 64 * 64; }

#include "vit_gemm_kernels.inc"
#include "vit_gemm_launch.inc"
#include "vit_attention.inc"
#include "vit_stage_kernels.inc"
#include "vit_scores.inc"

static void* vit_w(const vg_vit* v, const std::string& n) {
    auto it = v->w.find(n);
    return it == v->w.end() ? nullptr : it->second;
}

// ---- the tower's tensors by role.  One table of a block's state_dict names serves the resolver and vit_fold_ln.
enum { LN1_W, LN1_B, IN_W, IN_B, OUT_W, OUT_B, LN2_W, LN2_B, FC_W, FC_B, PROJ_W, PROJ_B, N_BLOCK_TENSORS };
static const char* const kBlockTensor[N_BLOCK_TENSORS] = {"ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias",
                                                          "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
                                                          "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"};
static std::string block_prefix(int l) { return "transformer.resblocks." + std::to_string(l) + "."; }

struct FoldedLn { const void* w; const float *c1, *c2; };      // "<weight>#ln", "#c1", "#c2": a LayerNorm folded into the GEMM behind it (vit_fold_ln)
struct BlockWeights {
    const void* t[N_BLOCK_TENSORS];
    FoldedLn in_proj, c_fc;                                    // (null unless vg_vit::ln_fold)
    const float* f(int i) const { return (const float*)t[i]; }
};
struct TopWeights {
    const void *conv1, *conv1_1ch;                             // (#1ch: vit_fold_conv1, null until an input_kind 3 encode)
    const float *cls, *pos, *pos_1ch, *ln_pre_w, *ln_pre_b, *ln_post_w, *ln_post_b, *proj;
    const float* tok;                                          // text tower: token_embedding.weight (ln_post_* = ln_final.*, proj = text_projection)
};
struct VitWeights { TopWeights top; std::vector<BlockWeights> blocks; };

// fills `out` from the handle's maps (caller holds v->mtx); a tensor that was never set is reported by name
static int vit_resolve(const vg_vit* v, VitWeights* out) {
    bool ok = true, told = false;
    auto get = [&](const std::string& n, auto& slot, bool required) {
        slot = static_cast<std::remove_reference_t<decltype(slot)>>(vit_w(v, n));
        if (slot || !required) return;
        if (!told && n.find('#') == std::string::npos) { fprintf(stderr, "[vilgod_hip] vg_vit_encode: weight %s not set\n", n.c_str()); told = true; }
        ok = false;
    };
    TopWeights& t = out->top;
    t = TopWeights();
    get("positional_embedding", t.pos, true);
    if (v->text) {                            // model.py:288-300
        get("token_embedding.weight", t.tok, true);
        get("ln_final.weight", t.ln_post_w, true); get("ln_final.bias", t.ln_post_b, true); get("text_projection", t.proj, true);
    } else {
        get("conv1.weight", t.conv1, true);       get("class_embedding", t.cls, true);
        get("ln_pre.weight", t.ln_pre_w, true);   get("ln_pre.bias", t.ln_pre_b, true);
        get("ln_post.weight", t.ln_post_w, true); get("ln_post.bias", t.ln_post_b, true);  get("proj", t.proj, true);
        get("conv1.weight#1ch", t.conv1_1ch, false);
        get("positional_embedding#1ch", t.pos_1ch, false);
    }
    out->blocks.resize((size_t)v->layers);
    for (int l = 0; l < v->layers; ++l) {
        BlockWeights& b = out->blocks[l];
        const std::string p = block_prefix(l);
        for (int i = 0; i < N_BLOCK_TENSORS; ++i) get(p + kBlockTensor[i], b.t[i], true);
        for (FoldedLn* f : {&b.in_proj, &b.c_fc}) {
            const std::string wn = p + kBlockTensor[f == &b.in_proj ? IN_W : FC_W];
            get(wn + "#ln", f->w, v->ln_fold); get(wn + "#c1", f->c1, v->ln_fold); get(wn + "#c2", f->c2, v->ln_fold);
        }
    }
    return ok ? VG_OK : VG_ERR_ARG;
}

// the handle's tensors by role, resolved again only after one of them was replaced (weights_gen moved)
static int vit_weights(vg_vit* v, std::shared_ptr<const VitWeights>* out) {
    std::lock_guard<std::mutex> lock(v->mtx);
    const uint64_t gen = v->weights_gen.load();
    if (!v->resolved || v->resolved_gen != gen) {
        auto w = std::make_shared<VitWeights>();
        const int rc = vit_resolve(v, w.get());
        if (rc) return rc;
        v->resolved = w;
        v->resolved_gen = gen;
    }
    *out = v->resolved;
    return VG_OK;
}

/* Builds the derived tensors of the folded LayerNorms once per handle (and again after a weight was replaced).  Called at the top
 * of vg_vit_encode; allocates and synchronises, so the first encode of a handle must not run inside a stream capture
 * (vg_vit_classify_graph runs it as plain launches). */
static int vit_fold_ln(vg_vit* v, hipStream_t st) {
    if (!v->ln_fold || v->fold_ready.load()) return VG_OK;
    std::lock_guard<std::mutex> lock(v->mtx);
    if (v->fold_ready.load()) return VG_OK;
    const int W = v->width;
    for (int l = 0; l < v->layers; ++l) {
        const std::string p = block_prefix(l);
        const int sets[2][4] = {{LN1_W, LN1_B, IN_W, IN_B}, {LN2_W, LN2_B, FC_W, FC_B}};      // LayerNorm gain, shift; the GEMM's weight, bias
        for (int k = 0; k < 2; ++k) {
            const std::string wn = p + kBlockTensor[sets[k][2]];
            auto it32 = v->w32.find(wn);
            const float* g = (const float*)vit_w(v, p + kBlockTensor[sets[k][0]]);
            const float* be = (const float*)vit_w(v, p + kBlockTensor[sets[k][1]]);
            const float* b = (const float*)vit_w(v, p + kBlockTensor[sets[k][3]]);
            if (it32 == v->w32.end() || !g || !be || !b) continue;      // vg_vit_encode reports the missing weight by name
            const int N = (int)(v->numel[wn] / (size_t)W);
            for (const char* suffix : {"#ln", "#c1", "#c2"}) {
                auto old = v->w.find(wn + suffix);
                if (old != v->w.end()) { (void)hipFree(old->second); v->w.erase(old); }
            }
            void *wf = nullptr, *c1 = nullptr, *c2 = nullptr;
            VG_CHECK(hipMalloc(&wf, (size_t)N * W * 2));
            VG_CHECK(hipMalloc(&c1, (size_t)N * 4));
            VG_CHECK(hipMalloc(&c2, (size_t)N * 4));
            hipLaunchKernelGGL(k_ln_fold, dim3(N), dim3(256), 0, st, (const float*)it32->second, g, be, b, (f16*)wf, (float*)c1, (float*)c2, W);
            VG_LAUNCH_CHECK();
            v->w[wn + "#ln"] = wf; v->w[wn + "#c1"] = c1; v->w[wn + "#c2"] = c2;
        }
    }
    VG_CHECK(hipStreamSynchronize(st));          // other threads' streams may use the tensors as soon as the flag is up
    v->weights_gen.fetch_add(1);
    v->fold_ready.store(true);
    return VG_OK;
}

/* Derived tensors of the single-channel patch embedding, once per handle (again after conv1.weight / positional_embedding /
 * the input normalisation changed).  Allocates and synchronises like vit_fold_ln: not inside a stream capture. */
static int vit_fold_conv1(vg_vit* v, hipStream_t st) {
    if (v->conv1_ready.load()) return VG_OK;
    std::lock_guard<std::mutex> lock(v->mtx);
    if (v->conv1_ready.load()) return VG_OK;
    auto it32 = v->w32.find("conv1.weight");
    const float* pos = (const float*)vit_w(v, "positional_embedding");
    if (v->dtype != 1 || it32 == v->w32.end() || !pos) return VG_ERR_ARG;
    const int W = v->width, pp = v->patch * v->patch;
    for (const char* nm : {"conv1.weight#1ch", "positional_embedding#1ch"}) {
        auto old = v->w.find(nm);
        if (old != v->w.end()) { (void)hipFree(old->second); v->w.erase(old); }
    }
    void *w1 = nullptr, *p1 = nullptr;
    VG_CHECK(hipMalloc(&w1, (size_t)W * pp * 2));
    VG_CHECK(hipMalloc(&p1, (size_t)v->T * W * 4));
    hipLaunchKernelGGL(k_conv1_fold, dim3(W), dim3(256), 0, st, (const float*)it32->second, pos, (f16*)w1, (float*)p1, W, v->T, pp,
                       v->in_mean[0], v->in_mean[1], v->in_mean[2], v->in_std[0], v->in_std[1], v->in_std[2]);
    VG_LAUNCH_CHECK();
    v->w["conv1.weight#1ch"] = w1;
    v->w["positional_embedding#1ch"] = p1;
    VG_CHECK(hipStreamSynchronize(st));
    v->weights_gen.fetch_add(1);
    v->conv1_ready.store(true);
    return VG_OK;
}

// the handle's events and device tensors (vg_vit_destroy, vg_text_destroy)
static void vit_release(vg_vit* v) {
    if (v->prof.init) for (int i = 0; i < 2 * VG_PROF_MAX; ++i) (void)hipEventDestroy(v->prof.ev[i]);
    for (auto& kv : v->w) (void)hipFree(kv.second);
    for (auto& kv : v->w32) (void)hipFree(kv.second);
}

#ifdef VG_DEV      // dev_vit_create and the development aids of tools/dev/vilgod_hip_dev.h: ablations, cycle-stamp traces
#include "dev/vit_dev_entry.inc"
#endif

extern "C" {

/* per-channel input normalisation (x / 255 - mean_c) / std_c that the single-channel patch rows (input_kind 3) fold into the patch
 * embedding; default: CLIP's constants (clip.py:79-86). */
int vg_vit_set_input_norm(vg_vit* v, const float* h_mean3, const float* h_std3) {
    if (!v || !h_mean3 || !h_std3) return VG_ERR_ARG;
    for (int c = 0; c < 3; ++c) {
        if (!(h_std3[c] > 0.f)) return VG_ERR_ARG;
        v->in_mean[c] = h_mean3[c]; v->in_std[c] = h_std3[c];
    }
    v->conv1_ready.store(false);
    return VG_OK;
}

int vg_vit_create(vg_vit** out, int width, int layers, int heads, int patch, int resolution, int out_dim, int dtype) {
    if (!out || width % 128 || width > 1024 || heads * 64 != width || resolution % patch || dtype < 0 || dtype > 1)
        return VG_ERR_ARG;
    int T = (resolution / patch) * (resolution / patch) + 1;
    // f16: k_attention_f16 up to AT_MAXT tokens, k_attention_f16_long up to AL_MAXT; f32: k_attention_f32 keeps an item's K, V and
    // four rows of probabilities per wave in LDS, (T * 65 + T * 64 + 16 * T) * 4 bytes within the 160 KiB it requests (T <= 282)
    if (dtype == 1 ? T > AL_MAXT : (size_t)T * (65 + 64 + 16) * 4 > 160 * 1024) return VG_ERR_ARG;
    vg_vit* v = new vg_vit();
    v->width = width; v->layers = layers; v->heads = heads; v->patch = patch; v->res = resolution;
    v->out_dim = out_dim; v->dtype = dtype; v->T = T;
    VitTower& tower = *v;
    tower = vit_resolve_switches(VitSwitches::from_env(), dtype, width);      // the handle's one reading of the environment
#ifdef VG_DEV
    dev_vit_create(v);
#endif
    *out = v;
    return VG_OK;
}

void vg_vit_destroy(vg_vit* v) {
    if (!v) return;
    vit_release(v);
    delete v;
}

/* upload one tensor by its reference state_dict name (prefix 'visual.' dropped); h_data is host float32.
 * GEMM weights are stored in the compute dtype, everything else stays float32. */
int vg_vit_set_weight(vg_vit* v, const char* name, const float* h_data, int64_t numel) {
    if (!v || !name || !h_data || numel <= 0) return VG_ERR_ARG;
    std::string n(name);
    std::lock_guard<std::mutex> lock(v->mtx);
    auto it = v->w.find(n);
    if (it != v->w.end()) {
        (void)hipFree(it->second);
        v->w.erase(it);
        v->weights_gen.fetch_add(1);             // (no resolved pointer to the freed tensor survives an early return below)
    }
    if (v->dtype == 1 && (n == "conv1.weight" || n == "positional_embedding")) {
        v->conv1_ready.store(false);             // the single-channel patch embedding's derived tensors are rebuilt at the next encode
        if (n == "conv1.weight") {
            auto o = v->w32.find(n);
            if (o != v->w32.end()) { (void)hipFree(o->second); v->w32.erase(o); }
            void* d32 = nullptr;
            VG_CHECK(hipMalloc(&d32, (size_t)numel * 4));
            VG_CHECK(hipMemcpy(d32, h_data, (size_t)numel * 4, hipMemcpyHostToDevice));
            v->w32[n] = d32;
        }
    }
    if (v->ln_fold && n.find("transformer.resblocks.") == 0) {
        v->fold_ready.store(false);              // a block's tensor changed: the folded LayerNorm tensors are rebuilt at the next encode
        if (n.find("in_proj_weight") != std::string::npos || n.find("c_fc.weight") != std::string::npos) {
            auto o = v->w32.find(n);
            if (o != v->w32.end()) { (void)hipFree(o->second); v->w32.erase(o); }
            void* d32 = nullptr;
            VG_CHECK(hipMalloc(&d32, (size_t)numel * 4));
            VG_CHECK(hipMemcpy(d32, h_data, (size_t)numel * 4, hipMemcpyHostToDevice));
            v->w32[n] = d32;
        }
    }
    std::vector<float> padded;
    if (n == "conv1.weight" && vit_kpad(v) != 3 * v->patch * v->patch) {     // [W, 3 p^2] -> [W, Kpad] with zero columns
        const int K = 3 * v->patch * v->patch, Kp = vit_kpad(v);
        if (numel != (int64_t)v->width * K) return VG_ERR_ARG;
        padded.assign((size_t)v->width * Kp, 0.f);
        for (int r = 0; r < v->width; ++r) memcpy(padded.data() + (size_t)r * Kp, h_data + (size_t)r * K, (size_t)K * 4);
        h_data = padded.data();
        numel = (int64_t)padded.size();
    }
    void* d = nullptr;
    if (v->dtype == 1 && is_gemm_weight(n)) {
        std::vector<f16> tmp((size_t)numel);
        for (int64_t i = 0; i < numel; ++i) tmp[i] = (f16)h_data[i];
        VG_CHECK(hipMalloc(&d, (size_t)numel * 2));
        VG_CHECK(hipMemcpy(d, tmp.data(), (size_t)numel * 2, hipMemcpyHostToDevice));
    } else {
        VG_CHECK(hipMalloc(&d, (size_t)numel * 4));
        VG_CHECK(hipMemcpy(d, h_data, (size_t)numel * 4, hipMemcpyHostToDevice));
    }
    v->w[n] = d;
    v->numel[n] = (size_t)numel;
    v->weights_gen.fetch_add(1);
    return VG_OK;
}

static int64_t pad128(int64_t m) { return (m + 255) / 256 * 256; }   // GEMM row tile (256)

}  // extern "C"

// ---- the plan of one encode: every size, the form of the residual stream and the byte offset of every workspace region, computed once
// per call from (handle, n_crops, input_kind).  vg_vit_workspace_bytes reports plan.total; vg_vit_encode takes its pointers from the
// same offsets.
enum class Stream {
    F32,         // fp32 in region x; separate LayerNorm launches write h
    F32_FOLD,    // fp32 in region x; the LayerNorms ride in the GEMMs around them: out_proj / c_proj also write the fp16 copy x16 and the rows' partial statistics
    PAIR,        // an fp16 pair (EPI_BIAS_RESID_HL): hi = x16 (what in_proj / c_fc read anyway), lo in region x; LayerNorms folded; 22 bits of the stream
    F16          // fp16 in region x (VG_VIT_RESID16), separate LayerNorm launches
};
struct Carve {                                  // consecutive regions of a buffer
    int64_t at = 0;
    int64_t take(int64_t bytes) { const int64_t o = at; at += bytes; return o; }
};
// The last block's compact class-token rows (Mc = n_crops padded to the row tile).  Both layouts borrow a region that is dead at the time:
struct ClsTail { int64_t xc, hc, x16c, mlpc, stats, size; };        // inside qkv, after the attention: fp32 stream rows, attention rows, fp16 copy, hidden activations, row statistics
struct ClsQuery { int64_t x16, q, stats, size; };                   // inside mlp, before the attention: fp16 stream rows, their projected queries, row statistics
struct VitPlan {
    int64_t M, Mp, P, Pp, Kp, Mc;               // tokens, patches (p: padded to the row tile), K of the patch embedding (padded to 64), class rows
    int embed_k;                                // K the patch-embedding GEMM runs with (input_kind 3: patch^2, the folded single-channel weight)
    int qkv_ld;                                 // row stride of the qkv buffer in elements
    int nst;                                    // partial statistics per row the folded LayerNorm's producers write
    Stream stream;
    bool ln1_in_embed;                          // k_embed_lnpre also writes ln_1 of block 0 into h
    bool cls_only_last;                         // the last block runs its tail on the class-token rows only
    int64_t x, h, qkv, mlp, patches, pe, x16, lnst, total;      // byte offsets of the regions; the workspace's size
    int64_t pe_bytes;                           // (pe is dead once the embedding kernel has run: scratch of the residual GEMMs' split-K tails)
    ClsTail tail;
    ClsQuery query;
};

static int vit_plan(const vg_vit* v, int n_crops, int input_kind, VitPlan* out) {
    if (!v || n_crops <= 0 || input_kind < 0 || input_kind > 3) return VG_ERR_ARG;
    if (input_kind >= 2 && v->dtype != 1) return VG_ERR_ARG;
    if (input_kind == 3 && (v->patch * v->patch) % 128) return VG_ERR_ARG;       // K of the folded patch embedding: two 64-wide K-tiles at least
    if (input_kind == 2 && vit_kpad(v) != 3 * v->patch * v->patch) return VG_ERR_ARG; // renderer patch rows carry no K padding
    VitPlan p;
    const int64_t W = v->width, es = v->dtype == 1 ? 2 : 4;
    p.M = (int64_t)n_crops * v->T;        p.Mp = pad128(p.M);
    p.P = (int64_t)n_crops * (v->T - 1);  p.Pp = pad128(p.P);
    p.Kp = vit_kpad(v);                   p.Mc = pad128(n_crops);
    p.embed_k = input_kind == 3 ? v->patch * v->patch : (int)p.Kp;
    // fp16: qkv rows padded by 64 halves.  The padding dates from k_gemm_f16, where 4608-byte rows aliased on the memory channels
    // (+20 %); with k_gemm_f16_pp64 the GEMM time no longer depends on it (13.50-13.58 ms per frame for 0 / 32 / 64 / 128 / 256),
    // but whole frames run 2.5 % faster with 0-128 than with 256 halves (57.0 vs 55.3 frames/s): less to write and to stride over.
    // (The region keeps room for 256.)
    p.qkv_ld = v->dtype == 1 ? 3 * (int)W + 64 : 3 * (int)W;
    p.nst = v->gemm.gemm_w4 ? (int)W >> 7 : (int)W >> 8;           // per 128 columns (k_gemm_f16_w4) or per 256 (k_gemm_f16_pp64)
    const bool fold = v->ln_fold;                             // (vg_vit_create: fp16 tower, width % 256 == 0, not the fp16 stream)
    const int64_t stats_row = (W / 64) * (int64_t)sizeof(LnPartial);     // room for W / 64 partials per row (k_gemm_f16_x2's count)
    Carve ws;
    p.x = ws.take(p.Mp * W * 4);
    p.h = ws.take(p.Mp * W * es);
    const int64_t qkv_bytes = p.Mp * (3 * W + 256) * es, mlp_bytes = p.Mp * 4 * W * es;
    p.qkv = ws.take(qkv_bytes);
    p.mlp = ws.take(mlp_bytes);
    p.patches = ws.take(p.Pp * p.Kp * es);
    p.pe_bytes = p.Pp * W * 4;
    p.pe = ws.take(p.pe_bytes);
    p.x16 = ws.take(fold ? p.Mp * W * 2 : 0);
    p.lnst = ws.take(fold ? p.Mp * stats_row : 0);
    p.total = ws.at + 1024;
    Carve t, q;
    p.tail.xc = t.take(p.Mc * W * 4);     p.tail.hc = t.take(p.Mc * W * 2);   p.tail.x16c = t.take(p.Mc * W * 2);
    p.tail.mlpc = t.take(p.Mc * 4 * W * 2);
    p.tail.stats = t.take(p.Mc * stats_row);
    p.tail.size = t.at;
    p.query.x16 = q.take(p.Mc * W * 2);   p.query.q = q.take(p.Mc * W * 2);   p.query.stats = q.take(p.Mc * stats_row);
    p.query.size = q.at;
    // The last block runs on the compact class-token rows only if their buffers fit in the regions they borrow.  With ViT-B/16 that holds
    // from 3 crops, ViT-B/32 from 11, ViT-L/14 from 2 (tests/test_vit.py pins the boundary).
    const bool cls_fits = p.tail.size <= qkv_bytes && p.query.size <= mlp_bytes;
    p.cls_only_last = v->cls_last && fold && v->layers > 1 && cls_fits;
    // every full-row residual GEMM of the pair stream is a folded-LayerNorm producer and no kernel reads the pair as the tower's output, so
    // it needs the last block on the compact fp32 class rows (vg_vit_create: resid_hl implies cls_last); otherwise the fp32 stream stays
    const bool pair = v->resid_hl && fold && p.cls_only_last;
    p.stream = v->resid_h ? Stream::F16 : pair ? Stream::PAIR : fold ? Stream::F32_FOLD : Stream::F32;
    p.ln1_in_embed = !v->resid_h && v->dtype == 1 && v->layers > 0;
    assert(p.stream != Stream::PAIR || p.cls_only_last);
    *out = p;
    return VG_OK;
}

// ---- one encode: the handle, its plan and resolved tensors, the stream, and the workspace regions as pointers
struct VitRun {
    vg_vit* v; const VitPlan& p; const TopWeights& top; hipStream_t st; int n_crops; char* ws;
    int W() const { return v->width; }
    float* x() const { return (float*)(ws + p.x); }                 // F16: fp16 rows; PAIR: the lo halves
    f16* x_h() const { return (f16*)(ws + p.x); }
    void* h() const { return ws + p.h; }
    void* qkv() const { return ws + p.qkv; }
    void* mlp() const { return ws + p.mlp; }
    float* pe() const { return (float*)(ws + p.pe); }
    f16* x16() const { return (f16*)(ws + p.x16); }
    LnPartial* lnst() const { return (LnPartial*)(ws + p.lnst); }
    bool folded() const { return p.stream == Stream::F32_FOLD || p.stream == Stream::PAIR; }

    // patches (im2col unless the renderer already wrote patch rows) -> patch embedding -> class token, positions, ln_pre [, ln_1 of block 0]
    int embed(const void* d_crops, int input_kind, const BlockWeights* b0) const {
        const void* patches = d_crops;
        if (input_kind < 2) {
            void* out = ws + p.patches;
            patches = out;
            int blocks = (int)((p.P * p.Kp + 255) / 256);
            if (blocks > 65535 * 8) blocks = 65535 * 8;
            const int res = v->res, ps = v->patch, Kp = (int)p.Kp;
            if (v->dtype == 1) {
                if (input_kind == 0) hipLaunchKernelGGL((k_im2col<float, f16>), dim3(blocks), dim3(256), 0, st, (const float*)d_crops, (f16*)out, n_crops, res, ps, Kp);
                else hipLaunchKernelGGL((k_im2col<f16, f16>), dim3(blocks), dim3(256), 0, st, (const f16*)d_crops, (f16*)out, n_crops, res, ps, Kp);
            } else {
                if (input_kind == 0) hipLaunchKernelGGL((k_im2col<float, float>), dim3(blocks), dim3(256), 0, st, (const float*)d_crops, (float*)out, n_crops, res, ps, Kp);
                else hipLaunchKernelGGL((k_im2col<f16, float>), dim3(blocks), dim3(256), 0, st, (const f16*)d_crops, (float*)out, n_crops, res, ps, Kp);
            }
            VG_LAUNCH_CHECK();
        }
        // input_kind 3: single-channel patch rows [P, patch^2] times the folded K = patch^2 weight; its constant rides in the positional table
        const bool one_ch = input_kind == 3;
        const int rc = launch_gemm<EPI_NONE_F32>(v->gemm, &v->prof, patches, one_ch ? top.conv1_1ch : top.conv1, nullptr, pe(), nullptr, (int)p.Pp, W(), p.embed_k, st);
        if (rc) return rc;
        const float* pos = one_ch ? top.pos_1ch : top.pos;
        const dim3 grid((unsigned)((p.Mp + 3) / 4));
        if (p.stream == Stream::F16)
            hipLaunchKernelGGL((k_embed_lnpre<f16>), grid, dim3(256), 0, st, pe(), top.cls, pos, top.ln_pre_w, top.ln_pre_b, x_h(), (int)p.M, v->T, W(), (int)p.Mp);
        else {
            // fp16 tower: ln_1 of block 0 is computed by the same kernel (writes h next to x); PAIR: it writes the pair instead of fp32 rows
            const bool ln1 = p.ln1_in_embed, pair = p.stream == Stream::PAIR;
            hipLaunchKernelGGL((k_embed_lnpre<float>), grid, dim3(256), 0, st, pe(), top.cls, pos, top.ln_pre_w, top.ln_pre_b, x(), (int)p.M, v->T, W(),
                               (int)p.Mp, ln1 ? b0->f(LN1_W) : (const float*)nullptr, ln1 ? b0->f(LN1_B) : (const float*)nullptr,
                               ln1 ? (f16*)h() : (f16*)nullptr, pair ? x16() : (f16*)nullptr, pair ? x_h() : (f16*)nullptr);
        }
        VG_LAUNCH_CHECK();
        return VG_OK;
    }

    // h = LayerNorm(stream); nothing to launch where the LayerNorm rides in the GEMM behind it
    int layernorm(const float* lw, const float* lb) const {
        const dim3 grid((unsigned)((p.M + 3) / 4));
        if (folded()) return VG_OK;
        if (p.stream == Stream::F16) hipLaunchKernelGGL((k_layernorm<f16, f16>), grid, dim3(256), 0, st, (const f16*)x_h(), lw, lb, (f16*)h(), (int)p.M, W(), 1);
        else if (v->dtype == 1) hipLaunchKernelGGL((k_layernorm<f16>), grid, dim3(256), 0, st, (const float*)x(), lw, lb, (f16*)h(), (int)p.M, W(), 1);
        else hipLaunchKernelGGL((k_layernorm<float>), grid, dim3(256), 0, st, (const float*)x(), lw, lb, (float*)h(), (int)p.M, W(), 1);
        VG_LAUNCH_CHECK();
        return VG_OK;
    }

    // stream += X @ Wt^T + bias over all rows (out_proj, c_proj).  `producer`: a folded LayerNorm reads the result, so the epilogue also
    // writes the fp16 copy and the rows' partial statistics (the last block's c_proj has no such consumer: ln_post reads fp32 rows in k_head)
    int resid_gemm(const void* X, const void* Wt, const float* bias, int K, bool producer) const {
        const int Mp = (int)p.Mp;
        if (p.stream == Stream::F16) return launch_gemm<EPI_BIAS_RESID_H>(v->gemm, &v->prof, X, Wt, bias, nullptr, x(), Mp, W(), K, st);
        if (p.stream == Stream::PAIR && producer) return launch_gemm<EPI_BIAS_RESID_HL, 2>(v->gemm, &v->prof, X, Wt, bias, nullptr, x(), Mp, W(), K, st, 0, nullptr, lnst(), x16());
        if (folded() && producer) return launch_gemm<EPI_BIAS_RESID, 2>(v->gemm, &v->prof, X, Wt, bias, nullptr, x(), Mp, W(), K, st, 0, nullptr, lnst(), x16(), pe(), (size_t)p.pe_bytes);
        return launch_gemm<EPI_BIAS_RESID>(v->gemm, &v->prof, X, Wt, bias, nullptr, x(), Mp, W(), K, st, 0, nullptr, nullptr, nullptr, pe(), (size_t)p.pe_bytes);
    }

    // qkv = ln_1(stream) @ in_proj^T + bias.  ln_done: h already holds ln_1 (block 0 after k_embed_lnpre, or layernorm() on an unfolded stream)
    int in_proj(const BlockWeights& b, bool ln_done) const {
        const int Mp = (int)p.Mp;
        if (ln_done) return launch_gemm<EPI_BIAS>(v->gemm, &v->prof, h(), b.t[IN_W], b.f(IN_B), qkv(), nullptr, Mp, 3 * W(), W(), st, p.qkv_ld);
        // ln_1 rides in in_proj: raw fp16 residual (x16) and row statistics (lnst) from the previous block's c_proj epilogue
        return launch_gemm<EPI_BIAS, 1>(v->gemm, &v->prof, x16(), b.in_proj.w, b.in_proj.c2, qkv(), nullptr, Mp, 3 * W(), W(), st, p.qkv_ld, b.in_proj.c1, lnst());
    }

    // The last block on the class rows needs K and V for every row but Q for the class-token rows only (round 5: a third of the launch,
    // 270 -> ~190 us per frame): in_proj's K / V rows (weight rows [W, 3W)) over all tokens, its Q rows over the compacted class-token
    // rows (the MLP buffer is free here), the queries scattered back to where the attention reads them.  The other tokens' Q columns keep
    // block L - 2's values: the attention's first query tile computes rows from them that nobody reads (a query row never meets another
    // query row).  Same kernel, same K loop per row: the same bits.
    int in_proj_cls(const BlockWeights& b) const {
        const int w = W(), Mc = (int)p.Mc;
        const FoldedLn& f = b.in_proj;
        char* cb = (char*)mlp();
        f16 *x16q = (f16*)(cb + p.query.x16), *qc = (f16*)(cb + p.query.q);
        LnPartial* lnq = (LnPartial*)(cb + p.query.stats);
        int rc = launch_gemm<EPI_BIAS, 1>(v->gemm, &v->prof, x16(), (const f16*)f.w + (size_t)w * w, f.c2 + w, (f16*)qkv() + w, nullptr, (int)p.Mp, 2 * w, w, st, p.qkv_ld, f.c1 + w, lnst());
        if (rc) return rc;
        hipLaunchKernelGGL(k_gather_cls_ln, dim3((unsigned)Mc), dim3(256), 0, st, (const f16*)x16(), (const LnPartial*)lnst(), x16q, lnq, n_crops, v->T, w, p.nst);
        VG_LAUNCH_CHECK();
        rc = launch_gemm<EPI_BIAS, 1>(v->gemm, &v->prof, x16q, f.w, f.c2, qc, nullptr, Mc, w, w, st, 0, f.c1, lnq);
        if (rc) return rc;
        hipLaunchKernelGGL(k_scatter_cls_q, dim3((unsigned)n_crops), dim3(256), 0, st, (const f16*)qc, (f16*)qkv(), v->T, w, p.qkv_ld);
        VG_LAUNCH_CHECK();
        return VG_OK;
    }

    // h = attention(qkv); cls: the class token's query row only (the first query tile)
    int attention(bool cls) const {
        const int T = v->T, H = v->heads;
        if (v->dtype != 1) return launch_attention_f32(v->text, (const float*)qkv(), (float*)h(), T, W(), H, n_crops * H, st);
        if (v->text) return launch_attention_causal((const f16*)qkv(), (f16*)h(), T, W(), H, p.qkv_ld, n_crops * H, st);
        // measurement hook (vg_vit_profile_read_kind 2 / 3): an event pair around each attention launch
        const bool aprof = v->prof.begin(st);
        const int rc = launch_attention<false>((const f16*)qkv(), (f16*)h(), T, W(), H, p.qkv_ld, n_crops * H, nullptr, st, cls ? 1 : (T + 31) / 32, v->att);
        if (rc) return rc;
        if (aprof) v->prof.end(st, cls ? 3 : 2, 4.0 * (cls ? 1.0 : (double)T) * (double)T * 64.0 * (double)(n_crops * H));
        return VG_OK;
    }

    // the rest of a block over all rows: out_proj, ln_2, c_fc + QuickGELU, c_proj
    int tail_full(const BlockWeights& b, bool last) const {
        int rc = resid_gemm(h(), b.t[OUT_W], b.f(OUT_B), W(), true);
        if (rc) return rc;
        if ((rc = layernorm(b.f(LN2_W), b.f(LN2_B)))) return rc;
        rc = folded() ? launch_gemm<EPI_BIAS_GELU, 1>(v->gemm, &v->prof, x16(), b.c_fc.w, b.c_fc.c2, mlp(), nullptr, (int)p.Mp, 4 * W(), W(), st, 0, b.c_fc.c1, lnst())
                      : launch_gemm<EPI_BIAS_GELU>(v->gemm, &v->prof, h(), b.t[FC_W], b.f(FC_B), mlp(), nullptr, (int)p.Mp, 4 * W(), W(), st);
        if (rc) return rc;
        return resid_gemm(mlp(), b.t[PROJ_W], b.f(PROJ_B), 4 * W(), !last);
    }

    // The LAST block: only the class token's row of its output is ever read (ln_post(x[:, 0, :]) @ proj, model.py:235-238), and
    // after the attention every row is processed on its own (out_proj, ln_2, c_fc, QuickGELU, c_proj and the two residual adds).
    // So the block computes all keys and values, the class token's attention row, and then runs its three remaining GEMMs on
    // the n_crops class-token rows alone (compacted, padded to the row tile) instead of on n_crops x T rows: the same value
    // per element -- a row's dot products do not depend on which rows share its tile -- for 1 / T of the work.  Ends with the head.
    int tail_cls(const BlockWeights& b, float* d_feat) const {
        const int w = W(), Mc = (int)p.Mc;
        const bool pair = p.stream == Stream::PAIR;
        char* cb = (char*)qkv();                 // (dead once the attention has run)
        float* xc = (float*)(cb + p.tail.xc);
        f16 *hc = (f16*)(cb + p.tail.hc), *x16c = (f16*)(cb + p.tail.x16c), *mlpc = (f16*)(cb + p.tail.mlpc);
        LnPartial* lnc = (LnPartial*)(cb + p.tail.stats);
        hipLaunchKernelGGL(k_gather_cls, dim3((unsigned)Mc), dim3(256), 0, st, (const f16*)h(), (const float*)x(), hc, xc, n_crops, v->T, w,
                           pair ? (const f16*)x16() : (const f16*)nullptr, pair ? (const f16*)x_h() : (const f16*)nullptr);
        VG_LAUNCH_CHECK();
        int rc = launch_gemm<EPI_BIAS_RESID, 2>(v->gemm, &v->prof, hc, b.t[OUT_W], b.f(OUT_B), nullptr, xc, Mc, w, w, st, 0, nullptr, lnc, x16c);
        if (rc) return rc;
        rc = launch_gemm<EPI_BIAS_GELU, 1>(v->gemm, &v->prof, x16c, b.c_fc.w, b.c_fc.c2, mlpc, nullptr, Mc, 4 * w, w, st, 0, b.c_fc.c1, lnc);
        if (rc) return rc;
        rc = launch_gemm<EPI_BIAS_RESID>(v->gemm, &v->prof, mlpc, b.t[PROJ_W], b.f(PROJ_B), nullptr, xc, Mc, w, 4 * w, st);
        if (rc) return rc;
        return head(xc, 1, d_feat);
    }

    // features = ln_post(class-token rows) @ proj; rows_per_crop: distance between two crops' class rows; row_idx (text tower): the row of
    // each item that is read instead of its first, ln_final(x[p, eot[p]]) @ text_projection
    template <typename TI>
    int head(const TI* rows, int rows_per_crop, float* d_feat, const int32_t* row_idx = nullptr) const {
        hipLaunchKernelGGL((k_head<TI>), dim3(n_crops), dim3(256), W() * sizeof(float), st, rows, top.ln_post_w, top.ln_post_b, top.proj, d_feat,
                           rows_per_crop, W(), v->out_dim, row_idx);
        VG_LAUNCH_CHECK();
        return VG_OK;
    }

    // every block after the front end, then the head (the class-row last block ends with its own)
    int blocks_and_head(const VitWeights& w, float* d_feat, const int32_t* row_idx = nullptr) const {
        const int L = v->layers;
        int rc;
        for (int l = 0; l < L; ++l) {
            const BlockWeights& b = w.blocks[l];
            const bool last = l == L - 1, cls = last && p.cls_only_last, ln1_done = l == 0 && p.ln1_in_embed;
            assert(!(last && p.stream == Stream::PAIR) || cls);        // the pair stream has no full-row last block (vit_plan)
            if (!ln1_done && (rc = layernorm(b.f(LN1_W), b.f(LN1_B)))) return rc;
            if ((rc = cls ? in_proj_cls(b) : in_proj(b, ln1_done || !folded()))) return rc;
            if ((rc = attention(cls))) return rc;
            if (cls) return tail_cls(b, d_feat);
            if ((rc = tail_full(b, last))) return rc;
        }
        return p.stream == Stream::F16 ? head(x_h(), v->T, d_feat, row_idx) : head(x(), v->T, d_feat, row_idx);
    }
};

extern "C" {

/* bytes of zero-initialised device workspace vg_vit_encode needs for n_crops */
int64_t vg_vit_workspace_bytes(const vg_vit* v, int n_crops) {
    VitPlan p;
    return vit_plan(v, n_crops, 0, &p) == VG_OK ? p.total : 0;
}

/* input_kind 0: f32 CHW crops [n,3,res,res]; 1: f16 CHW crops; 2: patch rows; 3: single-channel patch rows; d_feat: [n,out_dim] f32 */
int vg_vit_encode(vg_vit* v, const void* d_crops, int input_kind, int n_crops, void* d_workspace, float* d_feat,
                  void* stream) {
    if (!d_crops || !d_workspace || !d_feat) return VG_ERR_ARG;
    VitPlan p;
    int rc = vit_plan(v, n_crops, input_kind, &p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = vit_fold_ln(v, st))) return rc;
    if (input_kind == 3 && (rc = vit_fold_conv1(v, st))) return rc;
    std::shared_ptr<const VitWeights> w;
    if ((rc = vit_weights(v, &w))) return rc;
    if (input_kind == 3 && (!w->top.conv1_1ch || !w->top.pos_1ch)) return VG_ERR_ARG;
    const VitRun r{v, p, w->top, st, n_crops, (char*)d_workspace};
    if ((rc = r.embed(d_crops, input_kind, v->layers ? &w->blocks[0] : nullptr))) return rc;
    return r.blocks_and_head(*w, d_feat);
}

/* k_attention_f16 alone: softmax(q k^T / 8) v per (crop, head) on the padded qkv rows in_proj writes (model.py:175-187 via
 * nn.MultiheadAttention); exposed so that the kernel can be unit-tested against a plain fp32 attention. */
int vg_attention(const void* d_qkv, void* d_out, int n_crops, int T, int W, int heads, int ld, void* stream) {
    if (!d_qkv || !d_out || n_crops <= 0 || T < 1 || T > AL_MAXT || heads * 64 != W) return VG_ERR_ARG;
    // (handle-less test entry point: the switches are read per call, on the caller's thread)
    return launch_attention<false>((const f16*)d_qkv, (f16*)d_out, T, W, heads, ld, n_crops * heads, nullptr, (hipStream_t)stream, (T + 31) / 32,
                                   VitSwitches::from_env().att);
}

/* Every attention path of the tower, alone (test entry point; header: vilgod_hip.h).  dtype 1: launch_attention with the caller's q_tiles
 * (the class-row-only launch of the last block passes 1); dtype 0: k_attention_f32 as vg_vit_encode launches it. */
int vg_attention_rows(int dtype, const void* d_qkv, void* d_out, int n_crops, int T, int W, int heads, int ld, int q_tiles, void* stream) {
    if (!d_qkv || !d_out || n_crops <= 0 || T < 1 || T > AL_MAXT || heads <= 0 || heads * 64 != W || ld < 3 * W) return VG_ERR_ARG;
    if (q_tiles < 1 || q_tiles > (T + 31) / 32) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 1) {
        if (ld % 8) return VG_ERR_ARG;                  // (16-byte loads of the rows)
        return launch_attention<false>((const f16*)d_qkv, (f16*)d_out, T, W, heads, ld, n_crops * heads, nullptr, st, q_tiles,
                                       VitSwitches::from_env().att);  // (read per call, as vg_attention does)
    }
    if (dtype != 0) return VG_ERR_ARG;
    // k_attention_f32 hard-codes ld = 3 W and computes every row; its K, V and probability rows must fit the LDS it requests (vg_vit_create)
    if (ld != 3 * W || q_tiles != (T + 31) / 32) return VG_ERR_ARG;
    return launch_attention_f32(false, (const float*)d_qkv, (float*)d_out, T, W, heads, n_crops * heads, st);
}

/* The causal attention of the text tower, alone (test entry point; header: vilgod_hip.h): row q sees keys 0 .. q (model.py:320-326).
 * dtype 1: k_attention_f16<CAUSAL>, every query tile; dtype 0: k_attention_f32<CAUSAL>. */
int vg_attention_causal_rows(int dtype, const void* d_qkv, void* d_out, int n_items_crops, int T, int W, int heads, int ld, void* stream) {
    if (!d_qkv || !d_out || n_items_crops <= 0 || T < 1 || heads <= 0 || heads * 64 != W || ld < 3 * W) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 1) {
        if (T > AT_MAXT || ld % 8) return VG_ERR_ARG;
        return launch_attention_causal((const f16*)d_qkv, (f16*)d_out, T, W, heads, ld, n_items_crops * heads, st);
    }
    if (dtype != 0 || ld != 3 * W) return VG_ERR_ARG;
    return launch_attention_f32(true, (const float*)d_qkv, (float*)d_out, T, W, heads, n_items_crops * heads, st);     // (T <= 282: its LDS bound)
}

/* C = X @ Wt^T (+ epilogue), exposed for unit tests / micro-benchmarks of the GEMM itself.
 * dtype 1: X,Wt f16, M%256==0, N%128==0, K%32==0; dtype 0: f32, M%64, N%64, K%16.
 * epi 0: +bias -> C (compute dtype)   1: +bias, QuickGELU -> C   2: resid(f32) += acc + bias   3: C f32, no bias
 * epi 4 (dtype 1, N % 256 == 0, K % 64 == 0, K >= 128): d_resid holds fp16 [M,N]: resid = f16(resid + f16(acc + bias)) */
int vg_gemm(int dtype, int epi, const void* d_X, const void* d_Wt, const float* d_bias, void* d_C, float* d_resid,
            int M, int N, int K, void* stream) {
    const GemmCfg g = gemm_cfg(VitSwitches::from_env(), dtype);       // (handle-less: the switches are read per call, on the caller's thread)
    hipStream_t st = (hipStream_t)stream;
    switch (epi) {
        case 0: return launch_gemm<EPI_BIAS>(g, nullptr, d_X, d_Wt, d_bias, d_C, d_resid, M, N, K, st);
        case 1: return launch_gemm<EPI_BIAS_GELU>(g, nullptr, d_X, d_Wt, d_bias, d_C, d_resid, M, N, K, st);
        case 2: return launch_gemm<EPI_BIAS_RESID>(g, nullptr, d_X, d_Wt, d_bias, d_C, d_resid, M, N, K, st);
        case 3: return launch_gemm<EPI_NONE_F32>(g, nullptr, d_X, d_Wt, d_bias, d_C, d_resid, M, N, K, st);
        case 4: return dtype == 1 ? launch_gemm<EPI_BIAS_RESID_H>(g, nullptr, d_X, d_Wt, d_bias, d_C, d_resid, M, N, K, st) : VG_ERR_ARG;
    }
    return VG_ERR_ARG;
}

/* The kernel vg_gemm would launch for these arguments under the current VG_GEMM_W4 / VG_GEMM_F32_MFMA (read per call, as vg_gemm
 * does): gemm_family's answer.  0 k_gemm_f16, 1 k_gemm_f16_pp64, 2 k_gemm_f16_w4, 3 k_gemm_f32, 4 k_gemm_f32_mfma, negative: refused.
 * No launch, no device. */
int vg_gemm_family(int dtype, int epi, int M, int N, int K) {
    if (epi < 0 || epi > 4 || (epi == 4 && dtype != 1)) return GF_REFUSED;
    const VitSwitches s = VitSwitches::from_env();
    return gemm_family(dtype, epi, M, N, K, s.gemm_w4, s.f32_mfma, gemm_tile256(dtype, N, K));
}

/* The folded-LayerNorm epilogues of the projection GEMM, alone (test entry point; header: vilgod_hip.h).  Reuses the tower's own
 * instantiations: kind 0 / 1 = the consumer (in_proj / c_fc), 2 = the producer on the fp32 stream, 3 = the producer on the fp16 pair. */
int vg_gemm_ln(int kind, const void* d_X, const void* d_Wt, const float* d_bias, const float* d_c1, void* d_stats, void* d_C, int ldc,
               void* d_resid, void* d_x16, int M, int N, int K, void* stream) {
    if (!d_X || !d_Wt || !d_bias || !d_stats || ldc < N || ldc % 8) return VG_ERR_ARG;
    const GemmCfg g = gemm_cfg(VitSwitches::from_env(), 1);
    if (g.gemm_w4 && K < 256) return VG_ERR_ARG;       // (launch_gemm would take k_gemm_f16_pp64 there: 256-column partials)
    hipStream_t st = (hipStream_t)stream;
    LnPartial* stats = (LnPartial*)d_stats;
    switch (kind) {
        case 0:
        case 1:
            if (!d_c1 || !d_C) return VG_ERR_ARG;
            return kind == 0 ? launch_gemm<EPI_BIAS, 1>(g, nullptr, d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, st, ldc, d_c1, stats)
                             : launch_gemm<EPI_BIAS_GELU, 1>(g, nullptr, d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, st, ldc, d_c1, stats);
        case 2:
            if (!d_resid || !d_x16) return VG_ERR_ARG;
            return launch_gemm<EPI_BIAS_RESID, 2>(g, nullptr, d_X, d_Wt, d_bias, nullptr, (float*)d_resid, M, N, K, st, ldc, nullptr, stats, (f16*)d_x16);
        case 3:
            if (!d_resid || !d_x16) return VG_ERR_ARG;
            return launch_gemm<EPI_BIAS_RESID_HL, 2>(g, nullptr, d_X, d_Wt, d_bias, nullptr, (float*)d_resid, M, N, K, st, ldc, nullptr, stats, (f16*)d_x16);
    }
    return VG_ERR_ARG;
}

/* columns per (mean, m2) partial of the family vg_gemm_ln uses now (VG_GEMM_W4, read per call) */
int vg_gemm_ln_partial_cols(void) {
    return VitSwitches::from_env().gemm_w4 ? 128 : 256;
}

/* vg_gemm epi 2 (dtype 1) with scratch for the split-K tail (launch_gemm / splitk_plan): what the tower's residual GEMMs run.  Row tiles
 * beyond the last complete round of n_cu tiles are computed K-split through d_scratch (>= 2 MB per tail tile; without enough the
 * launch is not split).  Opt-in: VG_GEMM_SPLITK=n (at most n parts per tile; 8) in the environment, read per call. */
int vg_gemm_resid_splitk(const void* d_X, const void* d_Wt, const float* d_bias, float* d_resid, int M, int N, int K,
                         void* d_scratch, int64_t scratch_bytes, void* stream) {
    if (!d_X || !d_Wt || !d_bias || !d_resid || scratch_bytes < 0) return VG_ERR_ARG;
    const GemmCfg g = gemm_cfg(VitSwitches::from_env(), 1);
    return launch_gemm<EPI_BIAS_RESID>(g, nullptr, d_X, d_Wt, d_bias, nullptr, d_resid, M, N, K, (hipStream_t)stream, 0, nullptr, nullptr, nullptr,
                                       (float*)d_scratch, (size_t)scratch_bytes);
}

/* on != 0: record a HIP event pair around every projection-GEMM launch of vg_vit_encode (on the launch stream);
 * resets the collected samples. */
int vg_vit_profile(vg_vit* v, int on) {
    if (!v) return VG_ERR_ARG;
    GemmProfile& p = v->prof;
    if (on && !p.init) {
        for (int i = 0; i < 2 * VG_PROF_MAX; ++i) VG_CHECK(hipEventCreate(&p.ev[i]));
        p.init = true;
    }
    p.on = on;
    p.n = 0;
    return VG_OK;
}

/* synchronises, then returns the number of GEMM launches sampled, their summed duration (ms) and algorithmic FLOPs;
 * kind -1: every projection GEMM, 0: k_gemm_f16 / k_gemm_f32, 1: the 256 x 256 kernels (k_gemm_f16_w4 / k_gemm_f16_pp64) */
int vg_vit_profile_read_kind(vg_vit* v, int kind, int32_t* h_launches, double* h_ms, double* h_flops) {
    if (!v || !h_launches || !h_ms || !h_flops) return VG_ERR_ARG;
    *h_launches = 0; *h_ms = 0; *h_flops = 0;
    const GemmProfile& p = v->prof;
    for (int i = 0; i < p.n; ++i) {
        if (kind >= 0 ? p.kind[i] != kind : p.kind[i] >= 2) continue;     // (-1: the projection GEMMs)
        VG_CHECK(hipEventSynchronize(p.ev[2 * i + 1]));
        float ms = 0.f;
        VG_CHECK(hipEventElapsedTime(&ms, p.ev[2 * i], p.ev[2 * i + 1]));
        *h_ms += ms;
        *h_flops += p.flops[i];
        ++*h_launches;
    }
    return VG_OK;
}

int vg_vit_profile_read(vg_vit* v, int32_t* h_launches, double* h_ms, double* h_flops) {
    return vg_vit_profile_read_kind(v, -1, h_launches, h_ms, h_flops);
}

}  // extern "C"

#include "vit_text.inc"
#include "vit_graph.inc"
