// Part of vit.hip (included in place): vg_vit_encode + scores as one captured hipGraph per crop count.

extern "C" {

// the scores head of vg_vit_classify_graph: the one-wave kernel up to its 64 classes (the shipped 24-class graphs keep their node),
// the workgroup kernel above
static int classify_scores(const float* d_feat, int n, int dim, const float* d_text, int n_classes, float* d_probs, int32_t* d_top1,
                           float* d_top1_score, void* stream) {
    return n_classes <= 64 ? vg_clip_scores(d_feat, n, dim, d_text, n_classes, d_probs, d_top1, d_top1_score, stream)
                           : vg_clip_scores_wide(d_feat, n, dim, d_text, n_classes, d_probs, d_top1, d_top1_score, stream);
}

// The launch form of one classification: everything that selects kernel INSTANTIATIONS in vg_vit_encode + classify_scores beyond what is
// fixed per handle (type, width, token count, switches) -- the stream form (fp32 / folded fp32 / fp16 pair / fp16: the GEMM epilogues), the
// last block on the class rows (gather / scatter kernels, the class-row attention), the input kind (im2col instantiation or none, the
// K of the patch embedding and with it its GEMM family), the narrow or wide scores kernel -- as bit `*bit` of word `*slot` of
// vg_vit::warmed.  Slot 1: a crop count at which a residual GEMM of the k_gemm_f16_pp64 family runs a split-K tail (VG_GEMM_SPLITK,
// opt-in), which launches two more kernels.
static int classify_warm_slot(const vg_vit* v, int n_crops, int input_kind, int n_classes, int* slot, uint64_t* bit) {
    VitPlan p;
    const int rc = vit_plan(v, n_crops, input_kind, &p);
    if (rc) return rc;
    bool split = false;
    if (v->dtype == 1 && v->width % 256 == 0 && (p.stream == Stream::F32 || p.stream == Stream::F32_FOLD))
        for (const int K : {v->width, 4 * v->width})
            if (!(v->gemm.gemm_w4 && K / 64 >= 4))
                split = split || splitk_plan((int)(p.Mp / 256), v->width / 256, K / 64, (size_t)p.pe_bytes, v->gemm.splitk_max, vg_cu_count()).parts != 0;
    *slot = split ? 1 : 0;
    *bit = 1ull << ((int)p.stream | (p.cls_only_last ? 4 : 0) | (input_kind << 3) | (n_classes > 64 ? 32 : 0));
    return VG_OK;
}

/* ---- captured classification (SURVEY 7 step 7 / BASELINE config 5: hipGraph-captured loop) -----------------------------------
 * The launch-heavy, shape-stable part of a frame -- the ~150 kernels of vg_vit_encode + vg_clip_scores -- as ONE hipGraph per
 * distinct crop count, captured on first use and replayed afterwards.  The cache belongs to one worker (one stream, one set of
 * persistent buffers: patches, workspace, features, scores): the key is the crop count plus every pointer baked into the nodes. */
struct vg_graph_key {
    int n_crops, input_kind, dim, n_classes;
    const void *crops, *ws, *feat, *text, *probs, *top1, *score;
    const void* tower;            // the handle and the generation of its device tensors (weights are baked into the kernel nodes)
    uint64_t weights_gen;
    bool operator<(const vg_graph_key& o) const { return memcmp(this, &o, sizeof(*this)) < 0; }
};
struct vg_graph_entry { hipGraphExec_t exec; long last_use; };
struct vg_graph_cache {
    std::map<vg_graph_key, vg_graph_entry> graphs;
    long captured = 0, replayed = 0, evicted = 0, clock = 0;
    int limit = 32;               // graphs kept (least recently used one is destroyed beyond that): a real sequence has a new crop
                                  // count almost every frame, an unbounded cache would grow to hundreds of graphExecs per worker
};

int vg_graph_cache_create(vg_graph_cache** out) {
    if (!out) return VG_ERR_ARG;
    *out = new vg_graph_cache();
    return VG_OK;
}

void vg_graph_cache_destroy(vg_graph_cache* c) {
    if (!c) return;
    for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second.exec);
    delete c;
}

int vg_graph_cache_limit(vg_graph_cache* c, int max_graphs) {
    if (!c || max_graphs < 1) return VG_ERR_ARG;
    c->limit = max_graphs;
    return VG_OK;
}

int vg_graph_cache_stats2(const vg_graph_cache* c, int64_t* h_captured, int64_t* h_replayed, int64_t* h_evicted, int64_t* h_live) {
    if (!c) return VG_ERR_ARG;
    if (h_captured) *h_captured = c->captured;
    if (h_replayed) *h_replayed = c->replayed;
    if (h_evicted) *h_evicted = c->evicted;
    if (h_live) *h_live = (int64_t)c->graphs.size();
    return VG_OK;
}

int vg_graph_cache_stats(const vg_graph_cache* c, int64_t* h_captured, int64_t* h_replayed) {
    return vg_graph_cache_stats2(c, h_captured, h_replayed, nullptr, nullptr);
}

int vg_vit_classify_graph(vg_vit* v, vg_graph_cache* c, const void* d_crops, int input_kind, int n_crops, void* d_workspace, float* d_feat,
                          const float* d_text, int dim, int n_classes, float* d_probs, int32_t* d_top1, float* d_top1_score, void* stream) {
    if (!v || !c || n_crops <= 0 || !stream) return VG_ERR_ARG;          // capture needs a real (non-default) stream
    // Nothing may call hipFuncSetAttribute inside a capture, and the kernels' dynamic-LDS attributes are set lazily, once per kernel
    // INSTANTIATION, at its first launch (VG_MAX_DYNAMIC_LDS).  Which instantiations a classification launches is decided by its launch
    // form (classify_warm_slot): a handle's first call of every form runs as plain launches, so a capture only ever launches kernels
    // that a plain launch of the same handle has launched before.  Guaranteed: no attribute is set inside a capture.  (One plain call
    // per form and handle, not per crop count: the production buckets of 8 crops and more all share one form.)
    // The plain call also builds the handle's derived tensors (vit_fold_ln / vit_fold_conv1: they allocate and synchronise); the other
    // threads wait for it.
    int slot = 0;
    uint64_t bit = 0;
    { const int rc = classify_warm_slot(v, n_crops, input_kind, n_classes, &slot, &bit); if (rc) return rc; }
    const auto cold = [&]() { return !(v->warmed[slot].load() & bit) || (v->ln_fold && !v->fold_ready.load()) || (input_kind == 3 && !v->conv1_ready.load()); };
    if (cold()) {
        static std::mutex warm_mtx;
        std::lock_guard<std::mutex> lock(warm_mtx);
        if (cold()) {
            int rc = vg_vit_encode(v, d_crops, input_kind, n_crops, d_workspace, d_feat, stream);
            if (!rc) rc = classify_scores(d_feat, n_crops, dim, d_text, n_classes, d_probs, d_top1, d_top1_score, stream);
            if (!rc) VG_CHECK(hipStreamSynchronize((hipStream_t)stream));
            if (!rc) v->warmed[slot].fetch_or(bit);
            return rc;
        }
    }
    if (v->prof.on) {                                                   // event pairs cannot live in a graph: plain launches while profiling
        const int rc = vg_vit_encode(v, d_crops, input_kind, n_crops, d_workspace, d_feat, stream);
        return rc ? rc : classify_scores(d_feat, n_crops, dim, d_text, n_classes, d_probs, d_top1, d_top1_score, stream);
    }
    hipStream_t st = (hipStream_t)stream;
    vg_graph_key key;
    memset(&key, 0, sizeof(key));
    key.n_crops = n_crops; key.input_kind = input_kind; key.dim = dim; key.n_classes = n_classes;
    key.crops = d_crops; key.ws = d_workspace; key.feat = d_feat; key.text = d_text; key.probs = d_probs; key.top1 = d_top1; key.score = d_top1_score;
    key.tower = v; key.weights_gen = v->weights_gen.load();
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
        // thread-local capture mode: the other workers keep launching on their streams meanwhile
        hipGraph_t graph = nullptr;
        VG_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        int rc = vg_vit_encode(v, d_crops, input_kind, n_crops, d_workspace, d_feat, stream);
        if (!rc) rc = classify_scores(d_feat, n_crops, dim, d_text, n_classes, d_probs, d_top1, d_top1_score, stream);
        hipError_t e = hipStreamEndCapture(st, &graph);
        if (rc || e != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            fprintf(stderr, "[vilgod_hip] vg_vit_classify_graph: capture failed (rc %d, %s)\n", rc, hipGetErrorString(e));
            return rc ? rc : VG_ERR_HIP;
        }
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        VG_CHECK(e);
        while ((int)c->graphs.size() >= c->limit) {                    // least recently used out (its launches are stream-ordered
            auto lru = c->graphs.begin();                               // before this point; hipGraphExecDestroy defers the release)
            for (auto j = c->graphs.begin(); j != c->graphs.end(); ++j)
                if (j->second.last_use < lru->second.last_use) lru = j;
            VG_CHECK(hipStreamSynchronize(st));
            (void)hipGraphExecDestroy(lru->second.exec);
            c->graphs.erase(lru);
            c->evicted++;
        }
        it = c->graphs.emplace(key, vg_graph_entry{exec, 0}).first;
        c->captured++;
    }
    it->second.last_use = ++c->clock;
    VG_CHECK(hipGraphLaunch(it->second.exec, st));
    c->replayed++;
    return VG_OK;
}

}  // extern "C"
