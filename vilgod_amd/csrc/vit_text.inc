// Part of vit.hip (included in place): the CLIP text tower (model.py:343-356 CLIP.encode_text) on the image tower's blocks.  A vg_text is
// a vg_vit whose T is the context length, with `text` set: VitRun::attention launches the causal kernels (model.py:320-326), the resolver
// takes the text tower's names (model.py:288-300), the front end is k_text_embed and the head reads one row per prompt (the eot token's).
// The plan has no class-row last block (the wanted row sits elsewhere in every prompt), so the stream is fp32: folded LayerNorms for
// the fp16 tower at width % 256 == 0, separate LayerNorm launches otherwise -- projection-GEMM instantiations the image tower already has.

// x[p][t] = token_embedding[tok[p][t]] + positional_embedding[t]  (model.py:344-346; no ln_pre).  One wave per row.  Like k_embed_lnpre:
// rows n_rows .. n_rows_padded - 1 of the stream are re-zeroed on every call, and with h1 the row's ln_1 of block 0 (k_layernorm's
// formula) is written next to it.  A token id outside [0, vocab) is clamped: a wrong row of the table, never a read outside it.
__global__ __launch_bounds__(256) void k_text_embed(const int32_t* __restrict__ tokens, const float* __restrict__ tok_emb,
                                                    const float* __restrict__ pos, float* __restrict__ x, int n_rows, int ctx, int W,
                                                    int vocab, int n_rows_padded, const float* __restrict__ lw1,
                                                    const float* __restrict__ lb1, f16* __restrict__ h1) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows_padded) return;
    if (row >= n_rows) {
        for (int c = lane; c < W; c += 64) x[(size_t)row * W + c] = 0.f;
        return;
    }
    const int t = row % ctx;
    int id = tokens[row];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;
    const float* src = tok_emb + (size_t)id * W;
    float v[16];
    const int per = W / 64;   // W multiple of 64, <= 1024
    float s = 0.f;
    for (int i = 0; i < per; ++i) {
        const int c = lane + 64 * i;
        v[i] = src[c] + pos[(size_t)t * W + c];
        x[(size_t)row * W + c] = v[i];
        s += v[i];
    }
    if (h1) {
        const float mean = vg_wave_sum(s) / (float)W;
        float q = 0.f;
        for (int i = 0; i < per; ++i) {
            const float d = v[i] - mean;
            q += d * d;
        }
        const float rstd = rsqrtf(vg_wave_sum(q) / (float)W + 1e-5f);
        for (int i = 0; i < per; ++i) {
            const int c = lane + 64 * i;
            h1[(size_t)row * W + c] = (f16)((v[i] - mean) * rstd * lw1[c] + lb1[c]);
        }
    }
}

struct vg_text {
    vg_vit vit;                      // width, layers, heads, out_dim, dtype as given; T = ctx; patch = res = 0 (no patch rows)
    int ctx, vocab;
};

// the front end of one text encode: the stream's rows [, ln_1 of block 0 into h]
static int text_embed(const VitRun& r, const int32_t* d_tokens, int vocab, const BlockWeights* b0) {
    const bool ln1 = r.p.ln1_in_embed;
    hipLaunchKernelGGL(k_text_embed, dim3((unsigned)((r.p.Mp + 3) / 4)), dim3(256), 0, r.st, d_tokens, r.top.tok, r.top.pos, r.x(), (int)r.p.M,
                       r.v->T, r.W(), vocab, (int)r.p.Mp, ln1 ? b0->f(LN1_W) : (const float*)nullptr, ln1 ? b0->f(LN1_B) : (const float*)nullptr,
                       ln1 ? (f16*)r.h() : (f16*)nullptr);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

extern "C" {

int vg_text_create(vg_text** out, int width, int layers, int heads, int ctx, int vocab, int out_dim, int dtype) {
    if (!out || width <= 0 || width % 128 || width > 1024 || heads * 64 != width || layers < 0 || ctx < 1 || ctx > AT_MAXT || vocab < 1 ||
        out_dim < 1 || dtype < 0 || dtype > 1)
        return VG_ERR_ARG;
    vg_text* t = new vg_text();
    t->ctx = ctx; t->vocab = vocab;
    vg_vit* v = &t->vit;
    v->width = width; v->layers = layers; v->heads = heads; v->patch = 0; v->res = 0;
    v->out_dim = out_dim; v->dtype = dtype; v->T = ctx;
    v->text = true;
    VitSwitches s = VitSwitches::from_env();      // the handle's one reading of the environment
    s.cls_last = false;                           // no class row: every prompt's wanted row is its own (-> the fp32 stream, vit_plan)
    s.resid16 = false;                            // k_text_embed writes the fp32 stream only
    VitTower& tower = *v;
    tower = vit_resolve_switches(s, dtype, width);
    *out = t;
    return VG_OK;
}

void vg_text_destroy(vg_text* t) {
    if (!t) return;
    vit_release(&t->vit);
    delete t;
}

/* one tensor by its reference state_dict name (model.py:288-300); the tables' sizes are checked against the handle's, so that no
 * kernel indexes past one */
int vg_text_set_weight(vg_text* t, const char* name, const float* h_data, int64_t numel) {
    if (!t || !name) return VG_ERR_ARG;
    const std::string n(name);
    const int64_t W = t->vit.width;
    if ((n == "token_embedding.weight" && numel != (int64_t)t->vocab * W) || (n == "positional_embedding" && numel != (int64_t)t->ctx * W) ||
        (n == "text_projection" && numel != W * t->vit.out_dim) || ((n == "ln_final.weight" || n == "ln_final.bias") && numel != W))
        return VG_ERR_ARG;
    return vg_vit_set_weight(&t->vit, name, h_data, numel);
}

/* bytes of zero-initialised device workspace vg_text_encode needs for n_prompts */
int64_t vg_text_workspace_bytes(const vg_text* t, int n_prompts) {
    VitPlan p;
    return t && vit_plan(&t->vit, n_prompts, 0, &p) == VG_OK ? p.total : 0;
}

/* d_tokens [n, ctx] int32, d_eot [n] int32 (the row of each prompt the head reads), d_feat [n, out_dim] f32, not normalised */
int vg_text_encode(vg_text* t, const int32_t* d_tokens, const int32_t* d_eot, int n_prompts, void* d_workspace, float* d_feat, void* stream) {
    if (!t || !d_tokens || !d_eot || !d_workspace || !d_feat) return VG_ERR_ARG;
    vg_vit* v = &t->vit;
    VitPlan p;
    int rc = vit_plan(v, n_prompts, 0, &p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = vit_fold_ln(v, st))) return rc;
    std::shared_ptr<const VitWeights> w;
    if ((rc = vit_weights(v, &w))) return rc;
    const VitRun r{v, p, w->top, st, n_prompts, (char*)d_workspace};
    if ((rc = text_embed(r, d_tokens, t->vocab, v->layers ? &w->blocks[0] : nullptr))) return rc;
    return r.blocks_and_head(*w, d_feat, d_eot);
}

}  // extern "C"
