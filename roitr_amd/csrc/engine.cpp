// Whole-pair RoITr inference engine: host-side orchestration of the HIP kernels of this library.
//
// Reference path restated (file:line into /root/reference):
//   RIGA_v2.forward                      model/RIGA_v2.py:58-175
//   RIPointTransformer.forward           model/model.py:187-237
//   TransitionDown / Block / TransitionUp model/model.py:47-142
//   LocalPPFTransformer                  model/transformer/ppftransformer.py:202-253
//   GeometricTransformer                 model/transformer/geotransformer.py:94-133
//
// Execution model: B independent pairs per call, every kernel batched over the 2B clouds laid out
// [src_0..src_{B-1}, tgt_0..tgt_{B-1}] with cumulative offsets per hierarchy level (the reference's
// own `offset` convention, one level deeper: it batches clouds through pointops but runs one pair per
// forward).  No host synchronisation inside the forward: level sizes follow from the input sizes
// (model/model.py:59-62), data-dependent counts stay on the device.  All scratch comes from one
// arena sized from the input sizes; derived (folded / concatenated) weights are built once in finalize.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "prof.h"
#include "roitr_encode.h"
#include "roitr_engine.h"
#include "roitr_pointops.h"

#define CHK(x)                    \
    do {                          \
        int s__ = (x);            \
        if (s__ != 0) return s__; \
    } while (0)

namespace {

constexpr int HEADS = 4;
constexpr int GRID_MIN_POINTS = 768;  // clouds at or below this are scanned brute force

struct Lin {
    const float* w = nullptr; const float* b = nullptr; int out = 0, in = 0;
    const unsigned short* wb = nullptr;   // the weight stored in bf16 (operand_dtype = 1 only)
};

// How the forward runs one local transformer (roitr_local_form, include/roitr_engine.h; the table in DESIGN.md)
enum LocalForm { FIRST = ROITR_LOCAL_FIRST, FUSED_BLOCK = ROITR_LOCAL_FUSED_BLOCK, FUSED_TD = ROITR_LOCAL_FUSED_TD, TD_FOLD = ROITR_LOCAL_TD_FOLD,
                 SEQUENCE = ROITR_LOCAL_SEQUENCE };

struct LocalT {  // LocalPPFTransformer (+ derived weights)
    Lin emb, in_proj, q, k, v, p, vp, lin, out_proj;
    const float* norm_w = nullptr; const float* norm_b = nullptr;
    int in_dim = 0, H = 0, out_dim = 0;
    int K = 0;          // neighbours per node
    float scale = 0.f;  // 1 / sqrt(channels per head)
    bool td = false;    // the transformer of a TransitionDown (rows sampled by node_idx, no bn2 residual); false: of a block
    // set by fold_local():
    LocalForm form = SEQUENCE;
    bool from_x = false;   // in_proj is folded into the q | k | v projections (wqkv_x): they read the layer input, not f = in_proj(x)
    float* wqkv = nullptr;  // rows: [Wq (H) ; Wk (H) ; Wv (H)] x H
    unsigned short* wqkv_b = nullptr;   // the same, stored bf16 (operand_dtype = 1)
    float* bqkv = nullptr;
    // TransitionDown transformers (in_dim != H): [q|k|v] straight from the layer input, W' = Wqkv Win (R x in_dim),
    // b' = Wqkv b_in + bqkv -- in_proj and the q/k/v projections are two linear maps with nothing in between
    float* wqkv_x = nullptr; float* bqkv_x = nullptr; unsigned short* wqkv_x_b = nullptr;
    float* wkT_x = nullptr;                        // (in_dim, H): transpose of the k rows of wqkv_x (TD_FOLD, FUSED_TD)
    // FUSED_TD: q AND q~ from one on-chip GEMM over the gathered input rows --
    // rows 0 .. H-1 = Wq' (q = Wq' x + bq), rows H + h in_dim + i = (Wk'_h^T Wq'_h)[i, :] (q~_h = Wk'_h^T q_h); ((H + 4 in_dim), in_dim)
    float* wqqt_x = nullptr; float* bqqt_x = nullptr;
    // linear(att) + in_proj(x) as ONE GEMM over the K-concatenated operand [att | x]: cat.w = [Wlin | Win] (H x (H + in_dim)),
    // cat.b = b_lin + b_in; f = in_proj(x) is then never materialised
    Lin cat;
    unsigned short* wcat_b = nullptr;   // cat.w stored bf16 (bf16 operand mode, fused block)
    // the PPF coefficient rows of the query, qp[h] = [Wpe_h^T q_h, q_h . bpe_h], are computed inside the attention kernel from
    // wpe (H,4) / bpe (H): [q|k|v] is 3 H wide = whole 64-column GEMM tiles (as 5 extra GEMM columns per head it was 212 wide: one
    // 64-column tile in four was 31 % full)
    const float* wpe = nullptr; const float* bpe = nullptr;
    float* wvpe = nullptr;  // (H,4)
    float* bvpe = nullptr;  // (H)
    const float* bn2_w = nullptr; const float* bn2_b = nullptr;  // block only
};

struct Up {  // TransitionUp
    Lin l1, l2; const float* l1n_w = nullptr; const float* l1n_b = nullptr; const float* l2n_w = nullptr; const float* l2n_b = nullptr;
};

struct Ffn {
    Lin expand, squeeze; const float* n_w = nullptr; const float* n_b = nullptr;
};

struct GeoLayer {
    bool cross = false;
    Lin q, k, v, p, vp, lin, pos_lin;
    const float *n_w = nullptr, *n_b = nullptr, *pn_w = nullptr, *pn_b = nullptr;
    Ffn out, pos;
    float* wqkv = nullptr; float* bqkv = nullptr;  // self: [Wq;Wk;Wv]
    float* wpT = nullptr;                          // self: transpose(Wp)
    unsigned short* wqkv_b = nullptr; unsigned short* wpT_b = nullptr;   // stored bf16 (operand_dtype = 1)
};

struct Arena {
    char* base = nullptr; size_t cap = 0, off = 0, peak = 0;   // peak: the largest `off` since it was last zeroed
    bool fail = false;
    template <typename T> T* get(size_t count)
    {
        const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        if (off + bytes > cap) { fail = true; return (T*)base; }
        T* p = base ? (T*)(base + off) : nullptr;   // no base: a counting arena, only `off` advances
        off += bytes;
        if (off > peak) peak = off;
        return p;
    }
};

// 256-wide fp32 Linear + LayerNorm as one launch (ln256_fuses): the default row threshold, the longest K it covers, "never"
constexpr int LN256_MIN_ROWS = 39936;   // level-4 rows of 512 pairs of 5 000 points: the smallest measured size at which one launch won
constexpr int LN256_MAX_K = 512;
constexpr int LN256_NEVER = 0x7fffffff;

struct Engine {
    RoitrEngineConfig cfg;
    std::map<std::string, std::pair<const float*, long>> params;
    std::map<std::string, void*> taps;
    std::map<std::string, const void*> injects;
    bool finalized = false;
    int planes[4];
    int nblocks[4] = {2, 3, 3, 3};
    int nsample[4] = {8, 16, 16, 16};
    LocalT enc[4][3];
    LocalT dec[4];
    Up up[4];
    Lin geo_in, geo_out, proj_d, proj_a, coarse_proj, fine_proj;
    const float* geo_div = nullptr;
    float* geo_div_own = nullptr;
    // function-table form of the embedding (geo_table.hip): built at finalize unless ROITR_GEO_TABLE=0
    float* geo_tab = nullptr; float geo_tab_h = 0.f; int geo_tab_nd = 0, geo_tab_na = 0; double geo_tab_fit[6] = {0, 0, 0, 0, 0, 0};
    std::vector<GeoLayer> geo;
    const float* ot_alpha = nullptr;
    // rank-1 form of the first local transformer (in_planes = 1): constants of csrc/local_block.hip local_first_kernel
    float* first_consts = nullptr;   // head_consts (64) | G (64 x 32) | zero bias (64)
    Arena warena;  // derived weights
    Arena arena;   // per-forward scratch
    // scratch of the branch (the global transformer and the coarse front of the matching phase, queued beside the decoder): a region
    // of its own, carved once per call with no release inside the call -- the decoder reuses main-arena addresses while the branch runs
    Arena barena;
    // sampling-ahead mode (RoitrForwardIO::inputs_ready): descriptors, FPS scratch, pick indices and the coarser levels' coordinates /
    // normals of forward s+1 are written on the geometry stream while forward s still runs on the main one, so they cannot live in
    // the (stream-ordered, single) scratch arena: two small arenas used alternately
    Arena garena[2];
    int gpar = 0;
    int cur_par = -1;                // parity arena the running forward uses (-1: none)
    hipEvent_t gend[2] = {nullptr, nullptr};   // recorded on the main stream where the forward that used the arena ends
    bool gend_rec[2] = {false, false};
    bool ahead_off = false;          // the alternating arenas could not be allocated: every call is ordered on the main stream
    bool garena_short = false;       // an alternating arena ran out INSIDE a call: the wrapper repeats the call on the main-stream path
    static constexpr int RING = 4;   // descriptor staging slots: the host may run RING forwards ahead
    char* pinned[RING] = {nullptr, nullptr, nullptr, nullptr}; size_t pinned_cap[RING] = {0, 0, 0, 0};
    hipEvent_t pinned_ev[RING] = {nullptr, nullptr, nullptr, nullptr};
    int ring_pos = 0;
    hipStream_t side = nullptr;      // the geometry chain (FPS, grids, kNN + PPF of levels 2-4, 3-NN, embedding E, partition, GT outputs)
    // what each event orders ("main" / "geometry": the stream that records it)
    enum Ev {
        EV_MAIN_BEGIN,           // main: where this call begins -- inputs + descriptors in place, the shared scratch is free from here
        EV_LEVEL2_GEOM_DONE,     // geometry: "level l geometry done", levels 2 - 4 -- picks, coordinates, self and TransitionDown
        EV_LEVEL3_GEOM_DONE,     //           groups + PPF of the level are written (ev_level_done)
        EV_LEVEL4_GEOM_DONE,
        EV_LEVEL1_WS_FREE,       // main: the level-1 workspace (grid + retry list) is free for the TransitionDown query
        EV_EMBED_DONE,           // geometry: E and its index arrays
        EV_NN3_DONE,             // geometry: the decoder's 3-NN
        EV_TAIL_DONE,            // geometry: node coordinates, partition and ground-truth outputs (the last join)
        EV_ERROR_JOIN,           // geometry: the error-path join of roitr_engine_forward
        EV_DESC_COPIED,          // geometry: descriptors copied (ahead mode)
        EV_LEVEL1_GROUPS_READY,  // geometry: level-1 groups and PPFs (ahead mode)
        EV_ENCODER_DONE,         // main: the encoder's outputs are written (where the branch forks)
        EV_BRANCH_DONE,          // branch: global features, coarse correspondences and patch arrays (joined in front of the score product)
        EV_BRANCH_ERROR_JOIN,    // branch: the error-path join of roitr_engine_forward
        NEV
    };
    static Ev ev_level_done(int l) { return (Ev)(EV_LEVEL2_GEOM_DONE + l - 1); }   // l = 1 .. 3: the 0-based index of levels 2 - 4
    hipEvent_t ev[NEV] = {};
    bool side_forked = false;        // the current forward has issued work on `side` that `st` has not joined yet
    hipStream_t branch = nullptr;    // the global transformer and the coarse front, beside the decoder on the main stream
    int phase_overlap = 1;           // roitr_engine_set_phase_overlap: 0 = the branch's launches are queued on the main stream, in front of the decoder;
                                     // 1 = on the branch stream for calls of at least BRANCH_MIN_NODES superpoints; 2 = on the branch stream always
    int ln256_min_rows = LN256_MIN_ROWS;   // roitr_engine_set_ln256_min_rows: rows from which a 256-wide fp32 Linear + LayerNorm runs as one launch
    bool branch_forked = false;      // the current forward has issued work on `branch` that `st` has not joined yet
    bool on_branch = false;          // the last forward queued its branch on the branch stream (roitr_engine_scratch_info)
    std::string err;
    hipStream_t fin_stream = nullptr;   // stream of the running finalize (weight conversions are queued on it)
    // ---- captured forwards (roitr_engine_forward_graph): one hipGraphExec per (sizes, io pointers) key
    struct GraphEntry {
        std::vector<long> key;
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        char* pin = nullptr; size_t pin_cap = 0;   // the descriptor staging buffer the graph's H2D node reads
        long epoch = -1;                            // arena generation the graph's addresses belong to
        bool warmed = false, failed = false;
        unsigned long stamp = 0;
    };
    std::vector<GraphEntry> graphs;
    long arena_epoch = 0;            // bumped whenever the scratch arena is reallocated (invalidates captured addresses)
    unsigned long graph_clock = 0;
    char* capture_pin = nullptr;     // != nullptr: the forward is being captured and stages its descriptors here
    // operand_dtype = 2: the three bf16 pieces (csrc/gemm_x3.hip) of every weight block a K >= 256 GEMM has multiplied with, made on first
    // use (a warm-up call is never captured), dropped at finalize.  Key: (first element, elements) of the contiguous [N x K] block.
    std::map<std::pair<const float*, long>, unsigned short*> x3;
    // weights with a fragment-ordered copy for the fused local kernels (roitr_local_weights_prepare): made at finalize, released at
    // the next finalize (a parameter may have moved or changed) and at destroy
    std::vector<const float*> frag_weights;
};

// the engine whose forward / finalize is running on this thread (the GEMM helpers below are free functions)
thread_local Engine* g_engine = nullptr;

// operand_dtype = 2: route a plain fp32 GEMM with K >= 256 through the three-way bf16 split (same contract, fp32-accurate products on the
// bf16 matrix cores; rows bitwise independent of the row count, so the choice may not depend on M -- it depends on (K, layout) only)
int use_x3(RoitrGemm& g, hipStream_t st)
{
    Engine* E = g_engine;
    if (!E || E->cfg.operand_dtype != 2 || !E->finalized || g.bf16 || g.K < 256 || g.ldw != g.K || g.batch != 1 || g.ln_gamma) return 0;
    RoitrGemm t = g;
    t.bf16 = ROITR_BF16_X3; t.w_piece = (long)g.N * g.K;
    const long numel = (long)g.N * g.K;
    const auto key = std::make_pair(g.W, numel);
    auto it = E->x3.find(key);
    unsigned short* w3 = nullptr;
    if (it != E->x3.end()) w3 = it->second;
    else {
        if (E->capture_pin) return 0;   // no allocation inside a capture: this launch stays on the fp32 kernel (cannot happen after a warm-up)
        if (hipMalloc((void**)&w3, sizeof(unsigned short) * 3 * (size_t)numel) != hipSuccess) { (void)hipGetLastError(); return 0; }
        if (roitr_split_bf16x3(numel, g.W, w3, numel, st) != ROITR_OK) { (void)hipFree(w3); return 0; }
        E->x3[key] = w3;
    }
    t.W = reinterpret_cast<const float*>(w3);
    if (!roitr_gemm_x3_supported(&t)) return 0;
    g = t;
    return 0;
}

const float* P(Engine& E, const std::string& name, long expect)
{
    auto it = E.params.find(name);
    if (it == E.params.end()) { if (E.err.empty()) E.err = "missing parameter " + name; return nullptr; }
    if (expect > 0 && it->second.second != expect) {
        if (E.err.empty()) E.err = "parameter " + name + " has " + std::to_string(it->second.second) + " elements, expected " + std::to_string(expect);
        return nullptr;
    }
    return it->second.first;
}

Lin lin(Engine& E, const std::string& prefix, int out, int in)
{
    Lin l;
    l.w = P(E, prefix + ".weight", (long)out * in);
    l.b = P(E, prefix + ".bias", out);
    l.out = out; l.in = in;
    if (E.cfg.operand_dtype == 1 && l.w) {   // bf16 operand storage: converted once, here
        unsigned short* wb = E.warena.get<unsigned short>((size_t)out * in);
        if (!E.warena.fail && roitr_f32_to_bf16((long)out * in, l.w, wb, E.fin_stream) == 0) l.wb = wb;
    }
    return l;
}

// bf16 operand mode: `Wb` = the same weight stored bf16 (nullptr: fp32 layer).  The bf16 kernel is used whenever it takes the
// shape (K % 64 == 0, 16-byte rows); `bf` = ROITR_BF16_A / ROITR_BF16_C says A is / C shall be STORED in bf16 -- only legal
// when the bf16 kernel runs (callers check bf16_layer()), an fp32 fallback with such a request is an error.
bool bf16_layer(const unsigned short* Wb, int K) { return Wb != nullptr && K % 64 == 0; }
int use_bf16(RoitrGemm& g, const float* W, const unsigned short* Wb, int bf)
{
    if (Wb) {
        g.W = reinterpret_cast<const float*>(Wb);
        g.bf16 = ROITR_BF16_W | bf;
        if (roitr_gemm_bf16_supported(&g)) return 0;
        g.W = W; g.bf16 = 0;
    }
    if (bf) { roitr_set_error("engine: bf16-stored activation routed to an fp32 layer", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    return 0;
}

// nn.Linear followed by (+ residual) LayerNorm (+ post-add) (ReLU): one launch when the layer is 64 wide (the LayerNorm
// runs in the GEMM epilogue, the (M, 64) intermediate never reaches HBM), the two-launch sequence otherwise.
// `tmp` (M x N) is only touched by the two-launch form.
// The fused form is bitwise the two-launch result, so the choice may depend on the row count without breaking batch invariance.
// 64 / 128 columns: always fused.  256 columns (fp32 operand mode only; bf16 and the three-way split keep their paths): fused on the
// 32 x 256 tile of gemm_ln256.hip from LN256_MIN_ROWS rows, see ln256_fuses() for what was measured.
bool ln_fuses(const RoitrGemm& g)
{
    return (g.N == 64 || g.N == 128) && g.K % 32 == 0 && g.lda % 4 == 0 && g.ldw % 4 == 0;
}
// The 256-wide layers (levels 3 - 4, the global transformer, dec4 / dec3).  Measured per shape, events, the forms alternated
// (scripts/bench_gemm_ln.py, profiles/ln256_shapes.txt), fused 32 x 256 launch against GEMM + add_layernorm, K = 256 / 384 / 512, five
// epilogues: 319 488 rows 0.75 - 0.94 of the two launches, 79 872 rows 0.77 - 0.95, 39 936 rows 0.82 - 0.96; 19 968 rows 0.98 - 1.25,
// 9 984 rows 0.99 - 1.17, 624 rows 1.7 - 2.3 (a one-pair call: the two accumulator chains of a handful of blocks are the critical
// path, the plain GEMM has its 32 x 32 tiles there).  The break-even lies between 19 968 and 39 936 rows for every K; the rule is the
// smallest measured size that won.  The 64 x 256 instantiation of the general kernel loses to both at 39 936 rows and below and to the
// 32 x 256 tile everywhere (it reaches 0.83 - 0.98 of two launches at 319 488 / 79 872 rows).  Per 512-pair step: 78.63 -> 77.55 ms.
// K above LN256_MAX_K was not measured (no such layer).
bool ln256_fuses(const RoitrGemm& g, bool bf16_asked)
{
    const Engine* E = g_engine;
    if (!E || E->cfg.operand_dtype != 0 || bf16_asked) return false;
    return g.N == 256 && g.K % 32 == 0 && g.K <= LN256_MAX_K && g.lda % 4 == 0 && g.ldw % 4 == 0 && g.M >= E->ln256_min_rows;
}

// One GEMM of the engine: the launch arguments (RoitrGemm) with every optional part named, the operand-mode choice in run(), and
// the Linear + LayerNorm rule above in run_ln().  This is the only place a RoitrGemm is zeroed.
struct Gemm : RoitrGemm {
    const unsigned short* wb = nullptr;   // the weight stored bf16 (operand_dtype = 1); run() takes the bf16 kernel where it fits
    int bf = 0;                           // ROITR_BF16_A / ROITR_BF16_C: A is / C shall be stored bf16 (an error on an fp32 kernel)
    bool w_is_weight = true;              // false: W is an activation -- never a cached three-way split (operand_dtype = 2)
    struct {                              // LayerNorm epilogue of run_ln(): out = [relu](LN(C + res[res_idx]) * gamma + beta + post) (+ interp)
        const float *gamma, *beta, *res; const int* res_idx; const float* post; bool relu;
        const float* ip_feat; const int* ip_idx; const float* ip_dist2;
    } e = {};

    Gemm(int M_, int N_, int K_, const float* A_, int lda_, const float* W_, int ldw_, const float* bias_, float* C_, int ldc_)
    {
        memset(static_cast<RoitrGemm*>(this), 0, sizeof(RoitrGemm));
        M = M_; N = N_; K = K_; A = A_; lda = lda_; W = W_; ldw = ldw_; bias = bias_; C = C_; ldc = ldc_; alpha = 1.0f; batch = 1;
    }
    Gemm(int M_, const float* A_, const Lin& l, float* C_) : Gemm(M_, l.out, l.in, A_, l.in, l.w, l.in, l.b, C_, l.out) { wb = l.wb; }

    Gemm& with_relu() { relu = 1; return *this; }
    Gemm& gather(const int* idx) { a_idx = idx; return *this; }                   // row r of the operand is A[idx[r]]
    Gemm& plus(const float* A2_) { A2 = A2_; return *this; }                      // the operand is A + A2
    // the operand is [A | A_cat]: A dense (M, k_cat), A_cat of leading dimension lda_cat, rows optionally gathered by a_cat_idx (fp32 only)
    Gemm& cat(const float* Ac, int ldac, int kc, const int* idx = nullptr) { A_cat = Ac; lda_cat = ldac; k_cat = kc; a_cat_idx = idx; lda = kc; return *this; }
    Gemm& heads(int batch_, long sA_, long sW_, long sC_, long sBias_ = 0) { batch = batch_; sA = sA_; sW = sW_; sC = sC_; sBias = sBias_; return *this; }
    Gemm& bf16_weight(const unsigned short* wb_) { wb = wb_; return *this; }
    Gemm& stored(int bf_) { bf = bf_; return *this; }
    Gemm& activations() { w_is_weight = false; return *this; }
    Gemm& ln(const float* gamma, const float* beta, bool relu_ = false) { e.gamma = gamma; e.beta = beta; e.relu = relu_; return *this; }
    Gemm& residual(const float* res, const int* res_idx = nullptr) { e.res = res; e.res_idx = res_idx; return *this; }
    Gemm& post(const float* p) { e.post = p; return *this; }
    // TransitionUp's interpolation addend (RoitrGemm::ip_*): rows of `feat` (N floats) mixed by the 3-NN of every output row
    Gemm& interp3(const float* feat, const int* idx, const float* dist2) { e.ip_feat = feat; e.ip_idx = idx; e.ip_dist2 = dist2; return *this; }

    // The kernel choice of every launch: bf16 where a bf16 copy is given and fits (a K-concatenated operand is fp32-only: with A_cat
    // a copy is never looked at, and a bf16 request stays the error it is on an fp32 kernel), then the three-way split of
    // operand_dtype = 2 -- which itself refuses a bf16 launch, a batched one and one with a LayerNorm epilogue.
    int run(hipStream_t st)
    {
        CHK(use_bf16(*this, W, A_cat ? nullptr : wb, bf));
        if (w_is_weight) CHK(use_x3(*this, st));
        return roitr_gemm(this, st);
    }
    // Linear + LayerNorm into C; `tmp` (M x N) holds the GEMM's output where the two run as two launches
    int run_ln(hipStream_t st, float* tmp)
    {
        // measured per 128-pair forward: fusing the 64-wide layers -1.55 ms, + the 128-wide ones -0.4 ms
        // res gathered by res_idx from the buffer the launch writes: another block may have stored the row already (no such call site)
        const bool gather_in_place = e.res_idx && e.res == C;
        if (ln_fuses(*this) || (ln256_fuses(*this, wb || bf) && !gather_in_place)) {
            ln_gamma = e.gamma; ln_beta = e.beta; ln_res = e.res; ln_res_idx = e.res_idx; ln_post = e.post; ln_relu = e.relu ? 1 : 0; ln_eps = 1e-5f;
            ip_feat = e.ip_feat; ip_idx = e.ip_idx; ip_dist2 = e.ip_dist2;
            return run(st);
        }
        if (bf & ROITR_BF16_C) { roitr_set_error("engine: bf16 LayerNorm output needs the fused epilogue", __FILE__, __LINE__); return ROITR_ERR_ARG; }
        if (e.ip_feat && e.post) { roitr_set_error("engine: interpolation addend and post-add together", __FILE__, __LINE__); return ROITR_ERR_ARG; }
        float* out = C;
        C = tmp;
        CHK(run(st));
        if (e.ip_feat)
            return roitr_add_layernorm_interp(M, N, tmp, e.res, e.res_idx, e.gamma, e.beta, e.relu ? 1 : 0, 1e-5f, e.ip_feat, e.ip_idx, e.ip_dist2, out, st);
        return roitr_add_layernorm(M, N, tmp, e.res, e.res_idx, e.gamma, e.beta, e.post, e.relu ? 1 : 0, 1e-5f, out, st);
    }
};

int d2d(hipStream_t st, void* dst, const void* src, size_t bytes)
{
    ROITR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

int tap(Engine& E, hipStream_t st, const std::string& name, void* data, size_t bytes)
{
    auto ij = E.injects.find(name);
    if (ij != E.injects.end() && ij->second) CHK(d2d(st, data, ij->second, bytes));
    auto it = E.taps.find(name);
    if (it != E.taps.end() && it->second) CHK(d2d(st, it->second, data, bytes));
    return 0;
}

// ---------------------------------------------------------------- weight resolution + folding
int resolve_local(Engine& E, LocalT& L, const std::string& pre, int in_dim, int H, int out_dim, int K, bool td)
{
    L.in_dim = in_dim; L.H = H; L.out_dim = out_dim; L.K = K; L.td = td;
    L.scale = 1.0f / sqrtf((float)(H / HEADS));
    L.emb = lin(E, pre + ".embedding.proj", H, 4);
    L.in_proj = lin(E, pre + ".in_proj", H, in_dim);
    const std::string at = pre + ".transformer.attention";
    L.q = lin(E, at + ".proj_q", H, H); L.k = lin(E, at + ".proj_k", H, H); L.v = lin(E, at + ".proj_v", H, H);
    L.p = lin(E, at + ".proj_p", H, H); L.vp = lin(E, at + ".proj_vp", H, H);
    L.lin = lin(E, pre + ".transformer.linear", H, H);
    L.norm_w = P(E, pre + ".transformer.norm.weight", H); L.norm_b = P(E, pre + ".transformer.norm.bias", H);
    L.out_proj = lin(E, pre + ".out_proj", out_dim, H);
    return E.err.empty() ? 0 : ROITR_ERR_ARG;
}

int prepare_fragments(Engine& E, const float* W, int rows, int k, hipStream_t st)
{
    CHK(roitr_local_weights_prepare(W, rows, k, k, st));
    E.frag_weights.push_back(W);
    return 0;
}
void release_fragments(Engine& E)
{
    for (const float* W : E.frag_weights) (void)roitr_local_weights_release(W);
    E.frag_weights.clear();
}

// bf16 operand mode: a derived weight, folded in fp32, stored once in bf16
int bf16_copy(Engine& E, long n, const float* w, unsigned short*& wb, hipStream_t st)
{
    wb = E.warena.get<unsigned short>((size_t)n);
    return E.warena.fail ? ROITR_ERR_ARG : roitr_f32_to_bf16(n, w, wb, st);
}

int fold_local(Engine& E, LocalT& L, hipStream_t st)
{
    const int H = L.H;
    Arena& A = E.warena;
    float* weT = A.get<float>(4 * (size_t)H);
    float* wpeT = A.get<float>(4 * (size_t)H);
    float* wpe = A.get<float>(4 * (size_t)H);
    float* bpe = A.get<float>(H);
    float* wvpeT = A.get<float>(4 * (size_t)H);
    L.wvpe = A.get<float>(4 * (size_t)H);
    L.bvpe = A.get<float>(H);
    const int R = 3 * H;
    L.wqkv = A.get<float>((size_t)R * H);
    L.bqkv = A.get<float>(R);
    if (A.fail) return ROITR_ERR_ARG;
    // Wpe^T (4,H) = We^T (4,H) @ Wp^T ; bpe = Wp be + bp        (see csrc/local_attn.hip)
    CHK(roitr_transpose(H, 4, L.emb.w, 4, weT, H, st));
    CHK(Gemm(4, H, H, weT, H, L.p.w, H, nullptr, wpeT, H).run(st));
    CHK(roitr_transpose(4, H, wpeT, H, wpe, 4, st));
    CHK(Gemm(1, H, H, L.emb.b, H, L.p.w, H, L.p.b, bpe, H).run(st));
    L.wpe = wpe; L.bpe = bpe;
    CHK(Gemm(4, H, H, weT, H, L.vp.w, H, nullptr, wvpeT, H).run(st));
    CHK(roitr_transpose(4, H, wvpeT, H, L.wvpe, 4, st));
    CHK(Gemm(1, H, H, L.emb.b, H, L.vp.w, H, L.vp.b, L.bvpe, H).run(st));
    const Lin* qkv[3] = {&L.q, &L.k, &L.v};
    for (int j = 0; j < 3; ++j) {
        CHK(d2d(st, L.wqkv + (size_t)j * H * H, qkv[j]->w, sizeof(float) * (size_t)H * H));
        CHK(d2d(st, L.bqkv + j * H, qkv[j]->b, sizeof(float) * H));
    }
    const int I = L.in_dim;
    const bool bf16 = E.cfg.operand_dtype == 1;
    if (bf16) CHK(bf16_copy(E, (long)R * H, L.wqkv, L.wqkv_b, st));
    // ---- the form the forward runs this layer in, and exactly the derived weights that form reads
    L.form = (LocalForm)roitr_local_form(I, H, L.out_dim, L.K, L.td ? 1 : 0, E.cfg.operand_dtype);
    L.from_x = I % 32 == 0 && (!bf16 || L.form == FUSED_BLOCK || (L.td && I != H));
    const bool cat = L.form == FUSED_BLOCK || L.form == FUSED_TD || L.form == TD_FOLD || (L.form == SEQUENCE && L.from_x && !L.td);
    if (cat) {   // [Wlin | Win], b_lin + b_in
        float* wcat = A.get<float>((size_t)H * (H + I));
        float* bcat = A.get<float>(H);
        if (A.fail) return ROITR_ERR_ARG;
        ROITR_HIP(hipMemcpy2DAsync(wcat, sizeof(float) * (H + I), L.lin.w, sizeof(float) * H, sizeof(float) * H, H, hipMemcpyDeviceToDevice, st));
        ROITR_HIP(hipMemcpy2DAsync(wcat + H, sizeof(float) * (H + I), L.in_proj.w, sizeof(float) * I, sizeof(float) * I, H, hipMemcpyDeviceToDevice, st));
        CHK(roitr_add_vectors(H, L.lin.b, L.in_proj.b, bcat, st));
        L.cat.w = wcat; L.cat.b = bcat; L.cat.out = H; L.cat.in = H + I;   // (no Lin::wb: a K-concatenated GEMM is fp32-only)
        if (bf16) CHK(bf16_copy(E, (long)H * (H + I), wcat, L.wcat_b, st));   // the fused block's on-chip `linear`
    }
    if (L.from_x) {
        float* winT = A.get<float>((size_t)I * H);
        L.wqkv_x = A.get<float>((size_t)R * I);
        L.bqkv_x = A.get<float>(R);
        if (A.fail) return ROITR_ERR_ARG;
        CHK(roitr_transpose(H, I, L.in_proj.w, I, winT, H, st));                       // (in, H)
        CHK(Gemm(R, I, H, L.wqkv, H, winT, H, nullptr, L.wqkv_x, I).run(st));           // (R, in) = Wqkv Win
        CHK(Gemm(1, R, H, L.in_proj.b, H, L.wqkv, H, L.bqkv, L.bqkv_x, R).run(st));     // Wqkv b_in + bqkv
        if (bf16) CHK(bf16_copy(E, (long)R * I, L.wqkv_x, L.wqkv_x_b, st));
    }
    if (L.form == TD_FOLD || L.form == FUSED_TD) {
        // q~_h = Wk'_h^T q_h needs the k rows transposed: (I, H), head h = columns h c .. (csrc/local_attn.hip, fold form)
        L.wkT_x = A.get<float>((size_t)I * H);
        if (A.fail) return ROITR_ERR_ARG;
        CHK(roitr_transpose(H, I, L.wqkv_x + (size_t)H * I, I, L.wkT_x, H, st));
    }
    if (L.form == FUSED_TD) {
        // q~_h = Wk'_h^T (Wq'_h x + bq_h): one (H + 4 I) x I weight instead of the q GEMM followed by the batched q~ GEMM --
        // at I = 64 those were 1.42 + 1.19 ms per 512-pair step for 2 GB of q / q~ rows (two launches of K = 64 / K = 32);
        // wider inputs keep the two-step form (the folded weight has (H + 4 I) I entries against H I + H I / 4: more FLOPs
        // than the launch saves from I = 128 on)
        const int c = H / HEADS, R2 = H + HEADS * I;
        float* wqT = A.get<float>((size_t)I * H);
        L.wqqt_x = A.get<float>((size_t)R2 * I);
        L.bqqt_x = A.get<float>(R2);
        if (A.fail) return ROITR_ERR_ARG;
        CHK(roitr_transpose(H, I, L.wqkv_x, I, wqT, H, st));                                  // (I, H): q rows transposed
        CHK(d2d(st, L.wqqt_x, L.wqkv_x, sizeof(float) * (size_t)H * I));
        CHK(d2d(st, L.bqqt_x, L.bqkv_x, sizeof(float) * H));
        for (int h = 0; h < HEADS; ++h) {
            // (Wk'_h^T Wq'_h)[i', i] = sum_c wkT[i', h c + c] wqT[i, h c + c]
            CHK(Gemm(I, I, c, L.wkT_x + (size_t)h * c, H, wqT + (size_t)h * c, H, nullptr, L.wqqt_x + (size_t)(H + h * I) * I, I).run(st));
            // (Wk'_h^T bq_h)[i'] = sum_c bq[h c + c] wkT[i', h c + c]
            CHK(Gemm(1, I, c, L.bqkv_x + (size_t)h * c, c, L.wkT_x + (size_t)h * c, H, nullptr, L.bqqt_x + H + (size_t)h * I, I).run(st));
        }
    }
    // the fused fp32 kernels of csrc/local_block.hip read fragment-ordered copies of their weights, under exactly the views
    // block_args() / td_args() hand over (roitr_local_first's: build_local_first)
    if (L.form == FUSED_BLOCK && !bf16) {
        CHK(prepare_fragments(E, L.wqkv_x, H, H, st));
        CHK(prepare_fragments(E, L.cat.w, H, 2 * H, st));
        CHK(prepare_fragments(E, L.out_proj.w, H, H, st));
    }
    if (L.form == FUSED_TD) {
        CHK(prepare_fragments(E, L.wqqt_x, H + HEADS * I, I, st));
        CHK(prepare_fragments(E, L.wqkv_x + (size_t)(2 * H) * I, H, I, st));
        CHK(prepare_fragments(E, L.cat.w, H, H + I, st));
        CHK(prepare_fragments(E, L.out_proj.w, H, H, st));
    }
    return 0;
}

Ffn ffn(Engine& E, const std::string& pre, int C)
{
    Ffn f;
    f.expand = lin(E, pre + ".expand", 2 * C, C);
    f.squeeze = lin(E, pre + ".squeeze", C, 2 * C);
    f.n_w = P(E, pre + ".norm.weight", C); f.n_b = P(E, pre + ".norm.bias", C);
    return f;
}

// ---------------------------------------------------------------- per-forward geometry
struct Levels {
    std::vector<int> n[4];             // per cloud sizes per level (0-based level index = enc level - 1)
    std::vector<int> off[4];           // cumulative
    int T[4] = {0, 0, 0, 0};
    int nmax[4] = {0, 0, 0, 0};
};

// The descriptor block of one forward, staged on the host and copied to the device in one piece:
// off[4][NC] | cloud_of_node[T4] | partner[NC] | pad | eoff[NC] (long, 16-byte aligned) | a match only: slot_cloud[NC]
struct Desc {
    int* off[4]; int* cloud_of_node; int* partner; long* eoff;
    int* slot_cloud;   // roitr_engine_match: the cached cloud in every cloud slot of the call (behind the block of a forward)
    static size_t eoff_at(size_t NC, size_t T4) { return ((4 * NC + T4 + NC + 8) * sizeof(int) + 15) & ~(size_t)15; }
    static size_t bytes(size_t NC, size_t T4) { return eoff_at(NC, T4) + NC * sizeof(long); }
    static size_t bytes_with_slots(size_t NC, size_t T4) { return bytes(NC, T4) + NC * sizeof(int); }
    static Desc at(char* base, size_t NC, size_t T4)   // the fields of a block at `base` (host or device)
    {
        Desc D;
        for (int l = 0; l < 4; ++l) D.off[l] = (int*)base + (size_t)l * NC;
        D.cloud_of_node = (int*)base + 4 * NC;
        D.partner = D.cloud_of_node + T4;
        D.eoff = (long*)(base + eoff_at(NC, T4));
        D.slot_cloud = (int*)(base + bytes(NC, T4));
        return D;
    }
};

// ---------------------------------------------------------------- the local transformer: one function per form (LocalT::form)
// LocalPPFTransformer.forward (ppftransformer.py:227-253) on N_in input rows x -> M node rows.  node_idx (M) = the input row of every
// node of a TransitionDown that samples (nullptr: node r is row r).  The transformer of a block (!LocalT::td) is followed by the block's
// tail, out = relu(bn2(out_proj(..)) + x) (RIPointTransformerBlock.forward, model/model.py:131-142).
struct LocalIn { int N_in; const float* x; int M; const int* node_idx; const int* group; const float* ppf; const void* order; };

int form_error(const char* form)
{
    roitr_set_error((std::string("engine: local transformer finalized for another form than ") + form).c_str(), __FILE__, __LINE__);
    return ROITR_ERR_ARG;
}

RoitrLocalFirst first_args(const Engine& E, const LocalT& L, const LocalIn& in, float* out)
{
    RoitrLocalFirst lf;
    memset(&lf, 0, sizeof(lf));
    lf.M = in.M; lf.K = L.K; lf.x = in.x; lf.group_idx = in.group; lf.ppf = in.ppf; lf.node_order = in.order;
    lf.head_consts = E.first_consts; lf.G = E.first_consts + 64; lf.zero_bias = E.first_consts + 64 + 64 * 32;
    lf.norm_w = L.norm_w; lf.norm_b = L.norm_b; lf.wout = L.out_proj.w; lf.bout = L.out_proj.b;
    lf.scale = L.scale; lf.eps = 1e-5f; lf.out = out;
    return lf;
}
RoitrLocalBlock block_args(const LocalT& L, const LocalIn& in, const float* kv, float* out)
{
    RoitrLocalBlock b;
    memset(&b, 0, sizeof(b));
    b.M = in.M; b.K = L.K; b.H = L.H; b.x = in.x; b.kv = kv; b.group_idx = in.group; b.ppf = in.ppf; b.node_order = in.order;
    b.wq = L.wqkv_x; b.bq = L.bqkv_x; b.wpe = L.wpe; b.bpe = L.bpe; b.wvpe = L.wvpe; b.bvpe = L.bvpe;
    b.wcat = L.cat.w; b.bcat = L.cat.b; b.norm_w = L.norm_w; b.norm_b = L.norm_b; b.wout = L.out_proj.w; b.bout = L.out_proj.b;
    b.bn2_w = L.bn2_w; b.bn2_b = L.bn2_b; b.scale = L.scale; b.eps = 1e-5f; b.out = out;
    return b;
}
RoitrLocalTd td_args(const LocalT& L, const LocalIn& in, float* out)
{
    RoitrLocalTd t;
    memset(&t, 0, sizeof(t));
    t.M = in.M; t.in_dim = L.in_dim; t.H = L.H; t.x = in.x; t.node_idx = in.node_idx; t.group_idx = in.group; t.ppf = in.ppf; t.node_order = in.order;
    t.wqqt = L.wqqt_x; t.bqqt = L.bqqt_x; t.wv = L.wqkv_x + (size_t)(2 * L.H) * L.in_dim; t.bv = L.bqkv_x + 2 * L.H;
    t.wpe = L.wpe; t.wvpe = L.wvpe; t.bvpe = L.bvpe; t.wcat = L.cat.w; t.bcat = L.cat.b; t.norm_w = L.norm_w; t.norm_b = L.norm_b;
    t.wout = L.out_proj.w; t.bout = L.out_proj.b; t.scale = L.scale; t.eps = 1e-5f; t.out = out;
    return t;
}

// FIRST -- the first transformer of the network: scalar input feature -> rank-1 q | k | v, one launch (csrc/local_block.hip)
int local_first(Engine& E, hipStream_t st, const LocalT& L, const LocalIn& in, float* out)
{
    if (!E.first_consts || in.node_idx) return form_error("FIRST");
    const RoitrLocalFirst lf = first_args(E, L, in, out);
    return roitr_local_first(&lf, st);
}

// FUSED_BLOCK -- the 64- / 128-wide block transformers (levels 1-2, where the separate launches are HBM-shaped): one fused launch
// behind a plain k | v GEMM over all points (csrc/local_block.hip).  f = in_proj(x) is never formed: q|k|v come from x, the residual
// of the LayerNorm rides in `linear` as the second K-half of [att | x].  bf16 operand mode: the k | v rows are stored bf16 and the
// kernel's three on-chip GEMMs take bf16 matrix operands.
int local_fused_block(Engine& E, hipStream_t st, const LocalT& L, const LocalIn& in, float* out)
{
    if (!L.wqkv_x || !L.cat.w || in.node_idx || in.M != in.N_in) return form_error("FUSED_BLOCK");
    Arena& A = E.arena;
    const size_t mark = A.off;
    const int H = L.H, I = L.in_dim;
    float* kv = A.get<float>((size_t)in.N_in * 2 * H);
    if (A.fail) return ROITR_ERR_ARG;
    const unsigned short* wkv_b = bf16_layer(L.wqkv_x_b, I) ? L.wqkv_x_b + (size_t)H * I : nullptr;
    CHK(Gemm(in.N_in, 2 * H, I, in.x, I, L.wqkv_x + (size_t)H * I, I, L.bqkv_x + H, kv, 2 * H)
            .bf16_weight(wkv_b).stored(wkv_b ? ROITR_BF16_C : 0).run(st));
    RoitrLocalBlock b = block_args(L, in, kv, out);
    b.kv_bf16 = wkv_b ? 1 : 0;
    if (wkv_b && L.wcat_b && L.out_proj.wb) { b.wq_h = L.wqkv_x_b; b.wcat_h = L.wcat_b; b.wout_h = L.out_proj.wb; }
    CHK(roitr_local_block(&b, st));
    A.off = mark;
    return 0;
}

// FUSED_TD -- the whole TransitionDown transformer of the 64 -> 128 wide level in one launch (csrc/local_block.hip local_td_kernel)
int local_fused_td(Engine&, hipStream_t st, const LocalT& L, const LocalIn& in, float* out)
{
    if (!L.wqqt_x || !L.wqkv_x || !L.cat.w || !in.node_idx) return form_error("FUSED_TD");
    const RoitrLocalTd t = td_args(L, in, out);
    return roitr_local_td(&t, st);
}

// TD_FOLD -- TransitionDown in fp32 with the k | v projections folded into the query side (csrc/local_attn.hip local_attn_fold_kernel):
// q~ = Wk'^T q per head in front, Wv' applied to the attention-weighted INPUT rows behind; the (N_in, 2H) tensor is never formed.
// f = in_proj(x[node_idx]) -- only ever the LayerNorm residual -- rides in the K-concatenated `linear` as its second K part.
int local_td_fold(Engine& E, hipStream_t st, const LocalT& L, const LocalIn& in, float* out)
{
    if (!L.wkT_x || !L.wqkv_x || !L.cat.w || !in.node_idx) return form_error("TD_FOLD");
    Arena& A = E.arena;
    const size_t mark = A.off;
    const int M = in.M, H = L.H, I = L.in_dim, c = H / HEADS;
    float* qe = A.get<float>((size_t)M * H);
    float* qt = A.get<float>((size_t)M * HEADS * I);
    float* xbar = A.get<float>((size_t)M * HEADS * I);
    float* vpart = A.get<float>((size_t)M * H);
    float* val = A.get<float>((size_t)M * H);
    float* hid = A.get<float>((size_t)M * H);
    float* y = A.get<float>((size_t)M * H);
    if (A.fail) { roitr_set_error("arena exhausted (TransitionDown fold)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    CHK(Gemm(M, H, I, in.x, I, L.wqkv_x, I, L.bqkv_x, qe, H).gather(in.node_idx).run(st));
    // qt[(row, h), :] = Wk'_h^T q_h   (batched over heads; no bias: q_h . bk'_h is constant over the neighbours)
    CHK(Gemm(M, I, c, qe, H, L.wkT_x, H, nullptr, qt, HEADS * I).heads(HEADS, c, c, I).run(st));
    RoitrLocalAttnFold a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.in_dim = I; a.H = H; a.x = in.x; a.ldx = I; a.q = qe; a.ldq = H; a.qt = qt; a.group_idx = in.group; a.ppf = in.ppf;
    a.wpe = L.wpe; a.wvpe = L.wvpe; a.bvpe = L.bvpe; a.scale = L.scale; a.xbar = xbar; a.vpart = vpart; a.node_order = in.order;
    CHK(roitr_local_attention_fold(&a, st));
    // val[:, h-slice] = Wv'_h xbar_h + bv'_h
    CHK(Gemm(M, c, I, xbar, HEADS * I, L.wqkv_x + (size_t)(2 * H) * I, I, L.bqkv_x + 2 * H, val, H).heads(HEADS, I, (long)c * I, c, c).run(st));
    // LN([vpart + val | x[node_idx]] [Wlin | Win]^T + b_lin + b_in): att = vpart + val is formed while the operand is staged
    CHK(Gemm(M, vpart, L.cat, y).plus(val).cat(in.x, I, H, in.node_idx).ln(L.norm_w, L.norm_b).run_ln(st, hid));
    CHK(Gemm(M, y, L.out_proj, out).run(st));
    A.off = mark;
    return 0;
}

// SEQUENCE -- one launch per step: (in_proj,) q | k | v, attention, linear + LayerNorm, out_proj (+ the block's tail)
// (measured and dropped: folding in_proj into the projections of the first transformer of the network, K = 1 -- an outer-product kernel
//  writing the (T, 212) q|k|v rows is no faster than the K = 64 MFMA GEMM it replaces: 59.9 vs 59.2 ms of GEMM per 512-pair step)
int local_sequence(Engine& E, hipStream_t st, const LocalT& L, const LocalIn& in, float* out)
{
    Arena& A = E.arena;
    const size_t mark = A.off;
    const int M = in.M, N_in = in.N_in, H = L.H, R = 3 * H;
    // the three flavours, fixed at finalize:
    const bool from_x = L.from_x;            // q | k | v straight from x (in_proj folded into them), else from f = in_proj(x)
    const bool cat_res = from_x && !L.td;    // the LayerNorm residual f rides in `linear` as the second K-half of [att | x]: f is never formed
    // bf16 operand mode: the q | k | v tensor (operands of the attention products) and the attention output (operand of
    // `linear`) are stored bf16 by their producers -- half the bytes of the gather-bound attention kernel
    const bool hb = (from_x ? bf16_layer(L.wqkv_x_b, L.in_dim) : bf16_layer(L.wqkv_b, H)) && bf16_layer(L.lin.wb, H);
    if (from_x ? !L.wqkv_x : !L.wqkv) return form_error("SEQUENCE");
    if (cat_res && !L.cat.w) return form_error("SEQUENCE");
    const int cq = hb ? ROITR_BF16_C : 0;
    const size_t esz = hb ? 2 : 4;
    // f: the residual and, unless from_x, the operand of the projections -- of the M sampled rows only where only the residual reads it
    float* f = nullptr;
    if (!cat_res) {
        f = A.get<float>((size_t)(from_x ? M : N_in) * H);
        if (from_x) CHK(Gemm(M, in.x, L.in_proj, f).gather(in.node_idx).run(st));
        else CHK(Gemm(N_in, in.x, L.in_proj, f).run(st));
    }
    const float* src = from_x ? in.x : f;
    const int Kp = from_x ? L.in_dim : H;
    const float* w = from_x ? L.wqkv_x : L.wqkv; const float* b = from_x ? L.bqkv_x : L.bqkv;
    const unsigned short* wb = from_x ? L.wqkv_x_b : L.wqkv_b;
    const float *q, *k, *v; int ldq, ldkv;
    if (!in.node_idx) {   // every row is a node: q | k | v in one GEMM
        float* qkv = A.get<float>((size_t)N_in * R);
        if (A.fail) return ROITR_ERR_ARG;
        CHK(Gemm(N_in, R, Kp, src, Kp, w, Kp, b, qkv, R).bf16_weight(wb).stored(cq).run(st));
        const char* b0 = (const char*)qkv;
        q = qkv; k = (const float*)(b0 + (size_t)H * esz); v = (const float*)(b0 + (size_t)(2 * H) * esz); ldq = R; ldkv = R;
    } else {              // q of the M sampled rows, k | v of all N_in
        float* qe = A.get<float>((size_t)M * H);
        float* kv = A.get<float>((size_t)N_in * 2 * H);
        if (A.fail) return ROITR_ERR_ARG;
        CHK(Gemm(M, H, Kp, src, Kp, w, Kp, b, qe, H).gather(in.node_idx).bf16_weight(wb).stored(cq).run(st));
        CHK(Gemm(N_in, 2 * H, Kp, src, Kp, w + (size_t)H * Kp, Kp, b + H, kv, 2 * H).bf16_weight(wb ? wb + (size_t)H * Kp : nullptr).stored(cq).run(st));
        q = qe; k = kv; v = (const float*)((const char*)kv + (size_t)H * esz); ldq = H; ldkv = 2 * H;
    }
    float* att = A.get<float>((size_t)M * H);
    float* hid = A.get<float>((size_t)M * H);
    float* y = A.get<float>((size_t)M * H);
    if (A.fail) return ROITR_ERR_ARG;
    RoitrLocalAttn a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.K = L.K; a.H = H; a.heads = HEADS; a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldkv; a.v = v; a.ldv = ldkv;
    a.group_idx = in.group; a.ppf = in.ppf; a.wvpe = L.wvpe; a.bvpe = L.bvpe; a.scale = L.scale;
    a.out = att; a.ldo = H; a.node_order = in.order; a.bf16 = hb ? 3 : 0;
    a.wpe = L.wpe; a.bpe = L.bpe;   // qp computed in the kernel
    CHK(roitr_local_attention(&a, st));
    // bf16 operand mode: `y` only feeds out_proj -> the LayerNorm epilogue stores it in bf16 (half the round trip)
    Gemm lin_ln(M, att, L.lin, y);
    const bool y_h = ln_fuses(lin_ln) && bf16_layer(L.lin.wb, H) && bf16_layer(L.out_proj.wb, H);   // independent of M: batch-invariant storage
    if (cat_res) CHK(Gemm(M, att, L.cat, y).cat(in.x, L.in_dim, H).ln(L.norm_w, L.norm_b).run_ln(st, hid));
    else
    CHK(lin_ln.stored((y_h ? ROITR_BF16_C : 0) | (hb ? ROITR_BF16_A : 0)).ln(L.norm_w, L.norm_b).residual(f, from_x ? nullptr : in.node_idx).run_ln(st, hid));
    if (L.td) CHK(Gemm(M, y, L.out_proj, out).stored(y_h ? ROITR_BF16_A : 0).run(st));
    else {
        float* t = A.get<float>((size_t)M * L.out_dim);
        if (A.fail) return ROITR_ERR_ARG;
        CHK(Gemm(M, y, L.out_proj, out).stored(y_h ? ROITR_BF16_A : 0).ln(L.bn2_w, L.bn2_b, true).post(in.x).run_ln(st, t));
    }
    A.off = mark;
    return 0;
}

int local_transformer(Engine& E, hipStream_t st, const LocalT& L, const LocalIn& in, float* out)
{
    switch (L.form) {
    case FIRST: return local_first(E, st, L, in, out);
    case FUSED_BLOCK: return local_fused_block(E, st, L, in, out);
    case FUSED_TD: return local_fused_td(E, st, L, in, out);
    case TD_FOLD: return local_td_fold(E, st, L, in, out);
    case SEQUENCE: return local_sequence(E, st, L, in, out);
    }
    return form_error("any");
}

// scratch from `A` (the arena of the stream the launches are queued on), released on return
int ffn_apply(Arena& A, hipStream_t st, const Ffn& F, int M, int C, const float* x, float* out)
{
    const size_t mark = A.off;
    float* e = A.get<float>((size_t)M * 2 * C);
    float* s = A.get<float>((size_t)M * C);
    if (A.fail) { roitr_set_error("arena exhausted (ffn)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    // bf16 operand mode: the (M, 2C) hidden activation lives in bf16 between the two GEMMs
    const bool e_h = bf16_layer(F.expand.wb, C) && bf16_layer(F.squeeze.wb, 2 * C);
    CHK(Gemm(M, x, F.expand, e).with_relu().stored(e_h ? ROITR_BF16_C : 0).run(st));
    CHK(Gemm(M, e, F.squeeze, out).stored(e_h ? ROITR_BF16_A : 0).ln(F.n_w, F.n_b).residual(x).run_ln(st, s));
    A.off = mark;
    return 0;
}


// Constants of the first local transformer's rank-1 form (include/roitr_engine.h RoitrLocalFirst), in float64 from the layer's
// weights: q = x qa + qb etc. with qa = Wq w_in, qb = Wq b_in + bq (ppftransformer.py:244, attention.py:166-168).
int build_local_first(Engine& E, const LocalT& L, hipStream_t st)
{
    const int H = L.H, c = H / HEADS;
    if (L.form != FIRST) return 0;
    ROITR_HIP(hipStreamSynchronize(st));
    auto get = [&](const float* dev, size_t n, std::vector<double>& out) -> int {
        std::vector<float> h(n);
        ROITR_HIP(hipMemcpy(h.data(), dev, sizeof(float) * n, hipMemcpyDeviceToHost));
        out.assign(h.begin(), h.end());
        return 0;
    };
    std::vector<double> win, bin, wq, bq, wk, bk, wv, bv, wpe, bpe, wvpe, bvpe, wl, bl;
    CHK(get(L.in_proj.w, H, win)); CHK(get(L.in_proj.b, H, bin));
    CHK(get(L.q.w, (size_t)H * H, wq)); CHK(get(L.q.b, H, bq)); CHK(get(L.k.w, (size_t)H * H, wk)); CHK(get(L.k.b, H, bk));
    CHK(get(L.v.w, (size_t)H * H, wv)); CHK(get(L.v.b, H, bv));
    CHK(get(L.wpe, (size_t)H * 4, wpe)); CHK(get(L.bpe, H, bpe)); CHK(get(L.wvpe, (size_t)H * 4, wvpe)); CHK(get(L.bvpe, H, bvpe));
    CHK(get(L.lin.w, (size_t)H * H, wl)); CHK(get(L.lin.b, H, bl));
    auto matvec = [&](const std::vector<double>& W, const std::vector<double>& x, const std::vector<double>* b) {
        std::vector<double> y(H, 0.0);
        for (int o = 0; o < H; ++o) { double s = b ? (*b)[o] : 0.0; for (int i = 0; i < H; ++i) s += W[(size_t)o * H + i] * x[i]; y[o] = s; }
        return y;
    };
    const std::vector<double> qa = matvec(wq, win, nullptr), qb = matvec(wq, bin, &bq), ka = matvec(wk, win, nullptr), kb = matvec(wk, bin, &bk);
    const std::vector<double> va = matvec(wv, win, nullptr), vb = matvec(wv, bin, &bv);
    std::vector<float> hc(64, 0.f), G((size_t)H * 32, 0.f), zb(H, 0.f);
    for (int h = 0; h < HEADS; ++h) {
        double c1 = 0, c2 = 0, c3 = 0, c4 = 0, d1 = 0, d0 = 0, P1[4] = {0, 0, 0, 0}, P0[4] = {0, 0, 0, 0};
        for (int ch = h * c; ch < (h + 1) * c; ++ch) {
            c1 += qa[ch] * ka[ch]; c2 += qa[ch] * kb[ch]; c3 += qb[ch] * ka[ch]; c4 += qb[ch] * kb[ch];
            d1 += qa[ch] * bpe[ch]; d0 += qb[ch] * bpe[ch];
            for (int t = 0; t < 4; ++t) { P1[t] += wpe[(size_t)ch * 4 + t] * qa[ch]; P0[t] += wpe[(size_t)ch * 4 + t] * qb[ch]; }
        }
        float* o = hc.data() + h * 16;
        o[0] = (float)c1; o[1] = (float)c2; o[2] = (float)c3; o[3] = (float)c4;
        for (int t = 0; t < 4; ++t) { o[4 + t] = (float)P1[t]; o[8 + t] = (float)P0[t]; }
        o[12] = (float)d1; o[13] = (float)d0;
    }
    for (int o = 0; o < H; ++o) {
        double cst = bl[o] + bin[o];
        for (int h = 0; h < HEADS; ++h) {
            double sv = 0, sp[4] = {0, 0, 0, 0};
            for (int ch = h * c; ch < (h + 1) * c; ++ch) {
                const double w = wl[(size_t)o * H + ch];
                sv += w * va[ch];
                for (int t = 0; t < 4; ++t) sp[t] += w * wvpe[(size_t)ch * 4 + t];
                cst += w * (vb[ch] + bvpe[ch]);
            }
            G[(size_t)o * 32 + h] = (float)sv;
            for (int t = 0; t < 4; ++t) G[(size_t)o * 32 + 4 + 4 * h + t] = (float)sp[t];
        }
        G[(size_t)o * 32 + 20] = (float)win[o];
        G[(size_t)o * 32 + 21] = (float)cst;
    }
    E.first_consts = E.warena.get<float>(64 + (size_t)H * 32 + H);
    if (E.warena.fail) return ROITR_ERR_ARG;
    ROITR_HIP(hipMemcpy(E.first_consts, hc.data(), sizeof(float) * 64, hipMemcpyHostToDevice));
    ROITR_HIP(hipMemcpy(E.first_consts + 64, G.data(), sizeof(float) * G.size(), hipMemcpyHostToDevice));
    ROITR_HIP(hipMemcpy(E.first_consts + 64 + (size_t)H * 32, zb.data(), sizeof(float) * H, hipMemcpyHostToDevice));
    CHK(prepare_fragments(E, L.out_proj.w, H, H, st));   // roitr_local_first's out_proj
    return 0;
}
}  // namespace

extern "C" int roitr_local_form(int in_dim, int H, int out_dim, int K, int transition_down, int operand_dtype)
{
    const bool fp32 = operand_dtype != 1;   // the fused TransitionDown forms are fp32 arithmetic; the three-way split chooses like fp32
    if (transition_down) {
        if (fp32 && in_dim == 1 && H == 64 && out_dim == H && (K == 8 || K == 16)) return FIRST;
        if (fp32 && roitr_local_attention_fold_supported(in_dim, H, K))
            return out_dim == H && roitr_local_td_supported(in_dim, H, K) ? FUSED_TD : TD_FOLD;
        return SEQUENCE;
    }
    // bf16 too: behind a bf16 k | v GEMM, with bf16 matrix operands inside the kernel
    return in_dim == H && out_dim == H && roitr_local_block_supported(H, K) ? FUSED_BLOCK : SEQUENCE;
}

extern "C" void roitr_level_sizes(int n, int* out4)
{
    out4[0] = n; out4[1] = n / 4; out4[2] = out4[1] / 4; out4[3] = out4[2] / 4;
}

extern "C" void* roitr_engine_create(const RoitrEngineConfig* cfg)
{
    Engine* E = new Engine();
    E->cfg = *cfg;
    const int f = cfg->factor;
    E->planes[0] = 64 * f; E->planes[1] = 128 * f; E->planes[2] = 256 * f; E->planes[3] = 256 * f;
    return E;
}

extern "C" void roitr_engine_destroy(void* h)
{
    Engine* E = (Engine*)h;
    if (!E) return;
    if (g_engine == E) g_engine = nullptr;
    if (E->warena.base) (void)hipFree(E->warena.base);
    if (E->arena.base) (void)hipFree(E->arena.base);
    if (E->branch) (void)hipStreamSynchronize(E->branch);
    if (E->barena.base) (void)hipFree(E->barena.base);
    for (int i = 0; i < 2; ++i) if (E->garena[i].base) (void)hipFree(E->garena[i].base);
    for (int i = 0; i < 2; ++i) if (E->gend[i]) (void)hipEventDestroy(E->gend[i]);
    for (auto& g : E->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
        if (g.pin) (void)hipHostFree(g.pin);
    }
    for (auto& kv : E->x3) (void)hipFree(kv.second);
    release_fragments(*E);
    if (E->side) (void)hipStreamDestroy(E->side);
    if (E->branch) (void)hipStreamDestroy(E->branch);
    for (int i = 0; i < Engine::NEV; ++i) if (E->ev[i]) (void)hipEventDestroy(E->ev[i]);
    for (int i = 0; i < Engine::RING; ++i) {
        if (E->pinned[i]) (void)hipHostFree(E->pinned[i]);
        if (E->pinned_ev[i]) (void)hipEventDestroy(E->pinned_ev[i]);
    }
    delete E;
}

extern "C" int roitr_engine_set_param(void* h, const char* name, const float* ptr, long numel)
{
    Engine* E = (Engine*)h;
    E->params[name] = std::make_pair(ptr, numel);
    E->finalized = false;
    return 0;
}

extern "C" int roitr_engine_set_tap(void* h, const char* name, void* ptr)
{
    ((Engine*)h)->taps[name] = ptr;
    return 0;
}

extern "C" int roitr_engine_set_inject(void* h, const char* name, const void* ptr)
{
    ((Engine*)h)->injects[name] = ptr;
    return 0;
}

extern "C" int roitr_engine_finalize(void* h, hipStream_t st)
{
    Engine& E = *(Engine*)h;
    E.err.clear();
    g_engine = &E;
    E.finalized = false;   // (also: the folds below multiply WEIGHTS with weights in plain fp32 -- use_x3 only serves a finalized engine)
    // captured forwards replay kernels that read the parameter / derived-weight pointers of the previous finalize
    for (auto& g : E.graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
        if (g.pin) (void)hipHostFree(g.pin);
    }
    E.graphs.clear();
    if (E.branch) ROITR_HIP(hipStreamSynchronize(E.branch));   // a forward's branch may still read the weights this call replaces
    if (!E.x3.empty()) {   // split copies of the previous weights: a forward may still read them
        ROITR_HIP(hipStreamSynchronize(st));
        if (E.side) ROITR_HIP(hipStreamSynchronize(E.side));
        for (auto& kv : E.x3) (void)hipFree(kv.second);
        E.x3.clear();
    }
    release_fragments(E);   // of the previous weights (the release waits for forwards that still read them)
    const int f = E.cfg.factor;
    const int C4 = 256 * f;
    if (E.cfg.operand_dtype < 0 || E.cfg.operand_dtype > 2) { roitr_set_error("operand_dtype must be 0 (fp32), 1 (bf16) or 2 (fp32 by three-way bf16 split)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    // ---- derived-weight arena (folded / concatenated weights, bf16 copies); the bf16 copies are made while the names resolve
    {
        const size_t want = ((size_t)96 << 20) * (f > 1 ? 2 : 1) + (E.cfg.operand_dtype == 1 ? ((size_t)48 << 20) * f * f : 0);
        if (E.warena.cap < want) {
            if (E.warena.base) { ROITR_HIP(hipStreamSynchronize(st)); ROITR_HIP(hipFree(E.warena.base)); E.warena.base = nullptr; }
            E.warena.cap = want;
            ROITR_HIP(hipMalloc((void**)&E.warena.base, E.warena.cap));
        }
        E.warena.off = 0; E.warena.fail = false;
        E.fin_stream = st;
    }
    // ---- resolve names (model/model.py:146-184 module tree)
    int in_planes = 1;
    for (int l = 0; l < 4; ++l) {
        const std::string e = "backbone.enc" + std::to_string(l + 1);
        const int pl = E.planes[l];
        const int hid = pl < 256 * f ? pl : 256 * f;
        resolve_local(E, E.enc[l][0], e + ".0.transformer", in_planes, hid, pl, E.nsample[l], true);
        for (int b = 1; b < E.nblocks[l]; ++b) {
            const std::string bp = e + "." + std::to_string(b);
            resolve_local(E, E.enc[l][b], bp + ".transformer.transformer", pl, hid, pl, E.nsample[l], false);
            E.enc[l][b].bn2_w = P(E, bp + ".bn2.weight", pl); E.enc[l][b].bn2_b = P(E, bp + ".bn2.bias", pl);
        }
        in_planes = pl;
    }
    for (int l = 3; l >= 0; --l) {
        const std::string d = "backbone.dec" + std::to_string(l + 1);
        const int pl = E.planes[l];
        const int hid = pl < 256 * f ? pl : 256 * f;
        Up& U = E.up[l];
        if (l == 3) {
            U.l1 = lin(E, d + ".0.linear1.0", pl, 2 * pl);
            U.l2 = lin(E, d + ".0.linear2.0", pl, pl);
            U.l1n_w = P(E, d + ".0.linear1.1.weight", pl); U.l1n_b = P(E, d + ".0.linear1.1.bias", pl);
        } else {
            U.l1 = lin(E, d + ".0.linear1.0", pl, pl);
            U.l2 = lin(E, d + ".0.linear2.0", pl, E.planes[l + 1]);
            U.l1n_w = P(E, d + ".0.linear1.1.weight", pl); U.l1n_b = P(E, d + ".0.linear1.1.bias", pl);
            U.l2n_w = P(E, d + ".0.linear2.1.weight", pl); U.l2n_b = P(E, d + ".0.linear2.1.bias", pl);
        }
        resolve_local(E, E.dec[l], d + ".1.transformer.transformer", pl, hid, pl, E.nsample[l], false);
        E.dec[l].bn2_w = P(E, d + ".1.bn2.weight", pl); E.dec[l].bn2_b = P(E, d + ".1.bn2.bias", pl);
    }
    const std::string g = "backbone.global_transformer";
    E.proj_d = lin(E, g + ".embedding.proj_d", C4, C4);
    E.proj_a = lin(E, g + ".embedding.proj_a", C4, C4);
    E.geo_in = lin(E, g + ".in_proj", C4, C4);
    E.geo_out = lin(E, g + ".out_proj", C4, C4);
    E.geo.clear();
    for (int i = 0; i < E.cfg.n_geo_layers; ++i) {
        GeoLayer L;
        L.cross = E.cfg.geo_is_cross[i] != 0;
        const std::string lp = g + ".transformer.layers." + std::to_string(i);
        const std::string at = lp + ".attention.attention";
        L.q = lin(E, at + ".proj_q", C4, C4); L.k = lin(E, at + ".proj_k", C4, C4); L.v = lin(E, at + ".proj_v", C4, C4);
        L.lin = lin(E, lp + ".attention.linear", C4, C4);
        L.n_w = P(E, lp + ".attention.norm.weight", C4); L.n_b = P(E, lp + ".attention.norm.bias", C4);
        L.out = ffn(E, lp + ".output", C4);
        if (!L.cross) {
            L.p = lin(E, at + ".proj_p", C4, C4); L.vp = lin(E, at + ".proj_vp", C4, C4);
            L.pos_lin = lin(E, lp + ".attention.pos_linear", C4, C4);
            L.pn_w = P(E, lp + ".attention.pos_norm.weight", C4); L.pn_b = P(E, lp + ".attention.pos_norm.bias", C4);
            L.pos = ffn(E, lp + ".pos_proj", C4);
        }
        E.geo.push_back(L);
    }
    E.coarse_proj = lin(E, "coarse_proj", C4, C4);
    E.fine_proj = lin(E, "fine_proj", C4, 64 * f);
    E.ot_alpha = P(E, "optimal_transport.alpha", 1);
    if (!E.err.empty()) { roitr_set_error(E.err.c_str(), __FILE__, __LINE__); return ROITR_ERR_ARG; }

    // ---- derived weights
    for (int l = 0; l < 4; ++l) {
        for (int b = 0; b < E.nblocks[l]; ++b) CHK(fold_local(E, E.enc[l][b], st));
        CHK(fold_local(E, E.dec[l], st));
    }
    E.first_consts = nullptr;
    CHK(build_local_first(E, E.enc[0][0], st));
    for (auto& L : E.geo) {
        if (L.cross) continue;
        L.wqkv = E.warena.get<float>((size_t)3 * C4 * C4);
        L.bqkv = E.warena.get<float>((size_t)3 * C4);
        L.wpT = E.warena.get<float>((size_t)C4 * C4);
        if (E.warena.fail) break;
        const Lin* qs[3] = {&L.q, &L.k, &L.v};
        for (int j = 0; j < 3; ++j) {
            CHK(d2d(st, L.wqkv + (size_t)j * C4 * C4, qs[j]->w, sizeof(float) * (size_t)C4 * C4));
            CHK(d2d(st, L.bqkv + (size_t)j * C4, qs[j]->b, sizeof(float) * C4));
        }
        CHK(roitr_transpose(C4, C4, L.p.w, C4, L.wpT, C4, st));
        if (E.cfg.operand_dtype == 1) {
            L.wqkv_b = E.warena.get<unsigned short>((size_t)3 * C4 * C4);
            L.wpT_b = E.warena.get<unsigned short>((size_t)C4 * C4);
            if (E.warena.fail) break;
            CHK(roitr_f32_to_bf16((long)3 * C4 * C4, L.wqkv, L.wqkv_b, st));
            CHK(roitr_f32_to_bf16((long)C4 * C4, L.wpT, L.wpT_b, st));
        }
    }
    // SinusoidalPositionalEmbedding.div_term (positional_encoding.py:43-45): a buffer in the state_dict;
    // regenerate it in fp32 when the caller did not register it
    {
        auto it = E.params.find(g + ".embedding.embedding.div_term");
        if (it != E.params.end()) E.geo_div = it->second.first;
        else {
            E.geo_div_own = E.warena.get<float>(C4 / 2);
            std::vector<float> dv(C4 / 2);
            const float c = (float)(-log(10000.0) / (double)C4);
            for (int i = 0; i < C4 / 2; ++i) dv[i] = expf((float)(2 * i) * c);
            ROITR_HIP(hipMemcpyAsync(E.geo_div_own, dv.data(), sizeof(float) * dv.size(), hipMemcpyHostToDevice, st));
            ROITR_HIP(hipStreamSynchronize(st));
            E.geo_div = E.geo_div_own;
        }
    }
    E.geo_tab = nullptr;
    {   // GeometricStructureEmbedding as a function table: proj_x(sinusoid(v)) is univariate per channel.  The widest interval
        // whose MEASURED fit error (float64, between the interpolation nodes) is below 2^-25 of the function's amplitude is
        // taken; distances up to the table range (default 48 = 9.6 m at sigma_d = 0.2) are tabulated, larger ones are
        // evaluated directly by the kernel.  Angles: atan2 in [0, pi] scaled by 180 / (sigma_a pi).
        // ROITR_GEO_TABLE (the one switch of this library that selects a code path; tests/test_stages_gpu.py covers each form):
        // "0" = the GEMM form; otherwise options "range=<units>" (where the distance table ends) and "h=<interval>" (start the
        // interval search there instead of at 2), comma-separated
        const char* ev = getenv("ROITR_GEO_TABLE");
        double opt_range = 0.0, opt_h = 0.0;
        bool gemm_form = false;
        if (ev) {   // strict: comma-separated tokens "0" | "range=<units>" | "h=<interval>"; anything else is reported, not guessed at
            std::string all(ev);
            size_t pos = 0;
            while (pos <= all.size()) {
                size_t end = all.find(',', pos);
                if (end == std::string::npos) end = all.size();
                const std::string tok = all.substr(pos, end - pos);
                char* tail = nullptr;
                if (tok == "0") gemm_form = true;
                else if (tok.rfind("range=", 0) == 0 && (opt_range = strtod(tok.c_str() + 6, &tail), tail && *tail == 0 && opt_range > 0)) {}
                else if (tok.rfind("h=", 0) == 0 && (opt_h = strtod(tok.c_str() + 2, &tail), tail && *tail == 0 && opt_h > 0)) {}
                else if (!tok.empty()) {
                    fprintf(stderr, "roitr: ROITR_GEO_TABLE: unknown option '%s' (known: 0, range=<units>, h=<interval>)\n", tok.c_str());
                    roitr_set_error("ROITR_GEO_TABLE: unknown option", __FILE__, __LINE__);
                    return ROITR_ERR_ARG;
                }
                pos = end + 1;
            }
        }
        for (const char* gone : {"ROITR_GEO_TABLE_RANGE", "ROITR_GEO_TABLE_H"})   // round-4 names, folded into ROITR_GEO_TABLE in round 5
            if (getenv(gone)) fprintf(stderr, "roitr: %s is no longer read: use ROITR_GEO_TABLE=\"range=<units>,h=<interval>\"\n", gone);
        if (!gemm_form && C4 % 64 == 0) {
            const double d_range = opt_range > 0 ? opt_range : 48.0, a_range = 180.0 / 15.0;
            std::vector<float> hd((size_t)C4 * C4), ha((size_t)C4 * C4), hbd(C4), hba(C4), hdiv(C4 / 2);
            ROITR_HIP(hipStreamSynchronize(st));
            ROITR_HIP(hipMemcpy(hd.data(), E.proj_d.w, sizeof(float) * hd.size(), hipMemcpyDeviceToHost));
            ROITR_HIP(hipMemcpy(ha.data(), E.proj_a.w, sizeof(float) * ha.size(), hipMemcpyDeviceToHost));
            ROITR_HIP(hipMemcpy(hbd.data(), E.proj_d.b, sizeof(float) * C4, hipMemcpyDeviceToHost));
            ROITR_HIP(hipMemcpy(hba.data(), E.proj_a.b, sizeof(float) * C4, hipMemcpyDeviceToHost));
            ROITR_HIP(hipMemcpy(hdiv.data(), E.geo_div, sizeof(float) * (C4 / 2), hipMemcpyDeviceToHost));
            const float h_first = opt_h > 0 ? (float)opt_h : 2.0f;
            for (float h : {2.0f, 1.0f, 0.5f}) {
                if (h > h_first) continue;
                const int nd = (int)ceil(d_range / h), na = (int)floor(a_range / h) + 1;
                const size_t nf = roitr_geo_table_floats(C4, nd, na);
                if ((size_t)(nd + na) * 8 * 64 * sizeof(float) > 160 * 1024) break;
                std::vector<float> tab(nf);
                double fit[6];
                CHK(roitr_geo_table_build(C4, hdiv.data(), hd.data(), hbd.data(), ha.data(), hba.data(), h, nd, na, tab.data(), fit));
                // accepted when EVERY channel's measured error (64 probe points per interval) is below 2^-25 of that channel's
                // amplitude: trained weights that load the top frequencies fail h = 2 (degree 7 on sin(x): 2^-22) and get h = 1
                // (2^-30); near-cancelling coefficients can fail every interval -> the GEMM form
                const double tol = 1.0 / (double)(1 << 25);
                if (fit[4] <= tol && fit[5] <= tol) {
                    float* dev = E.warena.get<float>(nf);
                    if (E.warena.fail) break;
                    ROITR_HIP(hipMemcpy(dev, tab.data(), sizeof(float) * nf, hipMemcpyHostToDevice));
                    E.geo_tab = dev; E.geo_tab_h = h; E.geo_tab_nd = nd; E.geo_tab_na = na;
                    for (int q = 0; q < 6; ++q) E.geo_tab_fit[q] = fit[q];
                    break;
                }
            }
        }
    }
    if (E.warena.fail) { roitr_set_error("derived-weight arena exhausted", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    E.finalized = true;
    return 0;
}

/* The function table of the geometric embedding chosen at finalize: info[0..8] = {interval, n_int_d, n_int_a, fit error of the
 * distance projection, its amplitude, fit error of the angle projection, its amplitude, largest per-channel relative error of
 * the two}; returns 0 when no table is in use. */
extern "C" int roitr_engine_geo_table_info(void* h, double* info)
{
    Engine& E = *(Engine*)h;
    if (!E.geo_tab) return 0;
    info[0] = E.geo_tab_h; info[1] = E.geo_tab_nd; info[2] = E.geo_tab_na;
    for (int q = 0; q < 6; ++q) info[3 + q] = E.geo_tab_fit[q];
    return 1;
}

// mean points per grid cell (every level): the sphere of one cell size then holds ~2.5 (k + 2) points at level 1 (k = 8), what the
// prefilter kNN kernel's radius rule needs.  Round 5 re-measured 8 / 9.4 / 11 points per cell at levels 1 - 2 (per-call times of
// scripts/bench_knn_shapes.py: 5.6 -> 6.0 - 6.6 ms for the calls of a 512-pair forward): 6 stays.
static constexpr float GRID_OCC = 6.0f;

// Calls with fewer superpoints (rows of the global transformer) keep the branch's launches on the main stream, in the single-stream order
// (global transformer, decoder, coarse front).  Measured (profiles/phase_overlap_ab.txt): with the third stream one 5 000-point pair per call
// (156 rows), two calls in flight, was slower, 1.84 -> 1.91 ms per pair; calls of 9 984 (64 pairs), 16 000 (config 4) and 79 872 rows (config 2)
// were faster.  Nothing was measured between 156 and 9 984 rows: 8192 is a choice inside that gap, not a measured break-even.  The cause at
// one pair was not traced (expected: the geometry stream runs the NEXT call's whole chain beside this call, and a third stream competes with it).
// Every kernel's rows are independent of the row count, so the choice changes no result.
static constexpr int BRANCH_MIN_NODES = 8192;

// calls of up to this many pairs run their whole geometry chain ahead of the previous call (RoitrForwardIO::inputs_ready, reserve_arenas)
static constexpr int AHEAD_MAX_PAIRS = 128;

static int forward_body(Engine& E, const RoitrForwardIO* io, hipStream_t st);

// forward_body with the side stream joined on the error path
static int join_on_error(Engine& E, int rc, hipStream_t st);
static int forward_joined(Engine& E, const RoitrForwardIO* io, hipStream_t st)
{
    E.side_forked = false; E.branch_forked = false; E.cur_par = -1; E.garena_short = false;
    return join_on_error(E, forward_body(E, io, st), st);
}

// what a failed call (a forward, an encode) has left on the engine's other streams is joined into `st`
static int join_on_error(Engine& E, int rc, hipStream_t st)
{
    // (the branch first: it may itself wait for events of the geometry stream)
    if (rc != ROITR_OK && E.branch_forked && E.branch && E.ev[Engine::EV_BRANCH_ERROR_JOIN]) {
        if (hipEventRecord(E.ev[Engine::EV_BRANCH_ERROR_JOIN], E.branch) == hipSuccess) (void)hipStreamWaitEvent(st, E.ev[Engine::EV_BRANCH_ERROR_JOIN], 0);
        else (void)hipStreamSynchronize(E.branch);
    }
    if (rc != ROITR_OK && E.side_forked && E.side && E.ev[Engine::EV_ERROR_JOIN]) {
        if (hipEventRecord(E.ev[Engine::EV_ERROR_JOIN], E.side) == hipSuccess) (void)hipStreamWaitEvent(st, E.ev[Engine::EV_ERROR_JOIN], 0);
        else (void)hipStreamSynchronize(E.side);
    }
    return rc;
}

/* One engine = one main stream at a time: the side stream and its events are per engine, so two forwards of the same engine must
 * be ordered on the caller's stream (the Python side guarantees it: launch_batch uses torch's current stream).  An early return
 * between a fork and the last join (arena exhausted, unsupported shape, a HIP error) would leave side- or branch-stream work un-joined --
 * racing with the next forward's arena reuse, or ending a graph capture with an unjoined stream: forward_joined joins both. */
extern "C" int roitr_engine_forward(void* h, const RoitrForwardIO* io, hipStream_t st)
{
    Engine& E = *(Engine*)h;
    g_engine = &E;
    int rc = forward_joined(E, io, st);
    if (rc != ROITR_OK && E.garena_short) {
        // a buffer did not fit the alternating arena: no hard failure -- drain what the attempt queued and run the call once
        // more with everything ordered on the main stream; the engine stays on that path (the arena is sized by counting the carve
        // itself and the tests assert that the size holds: test_graph_gpu.py, so this is a safety net, not a mode)
        fprintf(stderr, "roitr: alternating geometry arena too small for this call (%s): falling back to main-stream order\n", roitr_last_error());
        (void)hipStreamSynchronize(st);
        if (E.side) (void)hipStreamSynchronize(E.side);
        if (E.branch) (void)hipStreamSynchronize(E.branch);
        E.ahead_off = true;
        rc = forward_joined(E, io, st);
    }
    E.side_forked = false; E.branch_forked = false;
    if (E.cur_par >= 0 && E.gend[E.cur_par]) {   // the alternating arena is free again where this call ends on the main stream
        if (hipEventRecord(E.gend[E.cur_par], st) == hipSuccess) E.gend_rec[E.cur_par] = true;
        else { (void)hipStreamSynchronize(st); E.gend_rec[E.cur_par] = false; }
    }
    E.cur_par = -1;
    return rc;
}

namespace {

// ---------------------------------------------------------------- one forward: its plan, its geometry buffers, its stages
// The host-side plan: sizes, limits, the ordering mode and the stream pair.  plan_sizes and reserve_arenas fill it; every later
// stage only reads it.
struct Plan {
    Levels V;
    int B = 0, NC = 0;                        // pairs, clouds (a forward and a match: 2 B cloud slots; an encode: NC clouds, B = 0)
    int T1 = 0, T4 = 0;                       // rows of the finest / the coarsest level (V.T[0], V.T[3])
    int C4 = 0, LIM = 0, P_ = 0;              // width of the coarsest level, points per patch, patches per pair
    size_t NPs = 0; bool compact = false;     // patch slots of the call; compact: the selected patches of all pairs back to back
    std::vector<long> eoff; long etot = 0;    // per cloud: where its n4 x n4 block of the embedding E starts; entries in all
    bool ahead = false, knn0_ahead = false, full_ahead = false;   // how much of the geometry chain runs beside the previous call (reserve_arenas)
    bool e_h = false;                         // E is stored bf16
    bool gt = false, gt_corr = false;         // ground-truth side outputs (RIGA_v2.py:91-116), only when rot / trans are given; node correspondences
    int Tp = 0, Tsp = 0, Ttp = 0;             // their padded rows: all, source, target
    hipStream_t st = nullptr, sd = nullptr;   // main stream, geometry stream
    hipStream_t sb = nullptr;                 // the stream of the branch: the engine's third stream, or `st` with the phase overlap off
    // roitr_engine_match: the cloud table the call's slots point into and the cloud of every slot (host).  Such a call has no geometry
    // stream (sd == nullptr): nothing of it waits for the chain's events
    const RoitrCloudTable* cache = nullptr; const int* slot_cloud = nullptr;
};

// Everything the geometry chain reads and writes.  carve_geometry takes every buffer; issue_geometry_chain fills them on the
// geometry stream (level 1's groups: on the stream the mode picks); the feature path reads them behind the chain's events.
struct GeoBufs {
    char* desc = nullptr; Desc D;                          // the descriptor block on the device and its fields
    const float* pts_out = nullptr;                        // coordinates the outputs are made of (io->points_out, or the geometry's own)
    const float* p[4]; const float* nrm[4];                // coordinates / normals per level ([0]: the inputs)
    int* down[4] = {nullptr, nullptr, nullptr, nullptr};   // FPS indices into level l-1 (global rows)
    int* g_self[4]; float* ppf_self[4];                    // self kNN groups (blocks + decoder)
    int* g_td[4]; float* ppf_td[4];                        // TransitionDown groups (level l nodes over level l-1 points)
    int* i3[3]; float* d3[3];                              // decoder: 3 nearest level-(l+1) points of every level-l point
    void* knn_ws[4];
    bool grid[4];
    const void* order[4] = {nullptr, nullptr, nullptr, nullptr};  // cell-order visiting order of each level's points
    float* d_idx = nullptr; float* a_idx = nullptr; float* Emb = nullptr;   // the global transformer's embedding and its index arrays
    float* node_xyz = nullptr; int* node_masks = nullptr; int* kidx = nullptr; int* kmask = nullptr;   // node outputs (the caller's, or scratch)
    float* fps_tmp = nullptr; int* fps_tie[4] = {nullptr, nullptr, nullptr, nullptr};   // FPS scratch; per cloud: first pick with a shared arg-max
    int* c3 = nullptr; int* c4 = nullptr; int* p2n = nullptr; float* p2nd = nullptr;    // partition scratch
    // ground-truth scratch: padded clouds, their offsets, nearest distances, the two kNN workspaces; node correspondences
    float* gt_pad = nullptr; int* gt_poff = nullptr; float* gt_d2p = nullptr; void* gt_ws_s = nullptr; void* gt_ws_t = nullptr;
    float* gt_om = nullptr; float* gt_nt = nullptr; float* gt_nr = nullptr;
};

// what the feature path hands from stage to stage (main arena): encoder output per level, global transformer output, decoder output per level
struct Feats { float* xe[4]; float* gfeat; float* xd[4]; };

// Everything the branch (global_transformer, then coarse_front) writes: all of it in the branch arena, taken once per call by
// carve_branch -- what the matching tail reads behind the join (correspondences, patch rows / masks / points) therefore lives as
// long as the call.  The caller's own output buffers are used where given.
struct BranchBufs {
    float *gfeat, *fcur, *pos, *qkv, *qt, *ebar, *hid, *t1, *t2;   // global transformer
    float *node_feats, *cp, *cscratch, *cxy; long cstride, xystride;   // coarse head and matching
    int *tgt_corr, *src_corr, *n_corr, *pair_off; float* cscore;
    int *trows, *srows, *tmask, *smask; float *tpts, *spts;            // patch arrays
};

// Run against a counting arena this is also what sizes the branch arena (its `peak`), so the two cannot differ.
void carve_branch(const RoitrForwardIO* io, const Plan& P, Arena& A, BranchBufs& R)
{
    const size_t T4 = P.T4, C4 = P.C4, B = P.B, LIM = P.LIM, P_ = P.P_, NP = P.NPs, n4 = P.V.nmax[3];
    R.gfeat = A.get<float>(T4 * C4);
    R.fcur = A.get<float>(T4 * C4);
    R.pos = A.get<float>(T4 * C4);
    R.qkv = A.get<float>(T4 * 3 * C4);
    R.qt = A.get<float>(T4 * HEADS * C4);
    R.ebar = A.get<float>(T4 * HEADS * C4);
    R.hid = A.get<float>(T4 * C4);
    R.t1 = A.get<float>(T4 * C4);
    R.t2 = A.get<float>(T4 * C4);
    R.node_feats = io->node_feats ? io->node_feats : A.get<float>(T4 * C4);
    R.cp = A.get<float>(T4 * C4);
    R.tgt_corr = io->tgt_corr ? io->tgt_corr : A.get<int>(B * P_);
    R.src_corr = io->src_corr ? io->src_corr : A.get<int>(B * P_);
    R.cscore = io->corr_scores ? io->corr_scores : A.get<float>(B * P_);
    R.n_corr = io->n_corr ? io->n_corr : A.get<int>(B);
    R.pair_off = P.compact ? (io->patch_offsets ? io->patch_offsets : A.get<int>(B + 1)) : nullptr;
    R.trows = A.get<int>(NP * LIM); R.srows = A.get<int>(NP * LIM);
    R.tmask = io->tgt_knn_masks ? io->tgt_knn_masks : A.get<int>(NP * LIM);
    R.smask = io->src_knn_masks ? io->src_knn_masks : A.get<int>(NP * LIM);
    R.tpts = io->tgt_knn_pts ? io->tgt_knn_pts : A.get<float>(NP * LIM * 3);
    R.spts = io->src_knn_pts ? io->src_knn_pts : A.get<float>(NP * LIM * 3);
    R.cstride = (long)roitr_coarse_scratch_floats((int)n4, (int)n4);
    R.cscratch = A.get<float>(B * (size_t)R.cstride);
    R.xystride = (long)(n4 * n4);
    R.cxy = A.get<float>(B * (size_t)R.xystride);
    // the hidden pair of ffn_apply over all T4 rows: the only scratch the branch takes and releases inside the call
    const size_t mark = A.off;
    (void)A.get<float>(T4 * 2 * C4); (void)A.get<float>(T4 * C4);
    A.off = mark;
}

// ---- stage 1: level sizes (host), patch slots, limits
// the cloud half: level sizes and offsets of NC clouds, where each cloud's block of E starts (back to back)
int plan_clouds(const Engine& E, const int* n_points, int NC, Plan& P)
{
    const int f = E.cfg.factor;
    P.NC = NC; P.C4 = 256 * f; P.LIM = E.cfg.point_limit; P.P_ = E.cfg.num_corr;
    Levels& V = P.V;
    for (int l = 0; l < 4; ++l) { V.n[l].resize(NC); V.off[l].resize(NC); }
    for (int c = 0; c < NC; ++c) {
        int s[4];
        roitr_level_sizes(n_points[c], s);
        for (int l = 0; l < 4; ++l) V.n[l][c] = s[l];
        if (s[3] < 4) { roitr_set_error("cloud too small: needs >= 256 points (4 nodes)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    }
    for (int l = 0; l < 4; ++l) {
        int acc = 0;
        for (int c = 0; c < NC; ++c) { acc += V.n[l][c]; V.off[l][c] = acc; V.nmax[l] = V.n[l][c] > V.nmax[l] ? V.n[l][c] : V.nmax[l]; }
        V.T[l] = acc;
    }
    P.T1 = V.T[0]; P.T4 = V.T[3];
    if (V.nmax[3] > 1024) { roitr_set_error("more than 1024 superpoints per cloud", __FILE__, __LINE__); return ROITR_ERR_UNSUPPORTED; }
    P.eoff.resize(NC);
    P.etot = 0;
    for (int c = 0; c < NC; ++c) { P.eoff[c] = P.etot; P.etot += (long)V.n[3][c] * V.n[3][c]; }
    // bf16 operand mode: E (an operand of the q~ . E and a' . E contractions of every self layer) is stored bf16 when the
    // attention kernel for this width reads it (C = 256 / 512, 4 heads, <= 512 superpoints)
    P.e_h = E.cfg.operand_dtype == 1 && E.proj_d.wb && E.proj_a.wb && (P.C4 == 256 || P.C4 == 512) && V.nmax[3] <= 512;
    return 0;
}

// the pair half: ground-truth rows, patch slots and their limits for the B pairs over the 2 B planned clouds
int plan_pairs(const Engine& E, const RoitrForwardIO* io, Plan& P)
{
    const int B = io->pairs, NC = P.NC; const Levels& V = P.V;
    P.B = B;
    P.gt = io->rot && io->trans && (io->gt_node_occ || io->gt_corr_idx);
    P.gt_corr = P.gt && io->gt_corr_idx && io->gt_corr_overlaps && io->gt_corr_count;
    P.Tp = P.T1 + NC; P.Tsp = V.off[0][B - 1] + B; P.Ttp = P.Tp - P.Tsp;
    if (E.cfg.adaptive_coarse) P.P_ = V.nmax[3] * V.nmax[3];  // every node pair may be selected (modules.py:111-112)
    // Patch slots of the call.  3DMatch: exactly B * num_corr, strided.  Adaptive matching: the SELECTED patches of all pairs back to back
    // (roitr_patch_offsets) in as many slots as the caller's per-patch outputs hold (RoitrForwardIO::patch_slots; 0 = the bound B * n^2)
    P.compact = E.cfg.adaptive_coarse != 0;
    P.NPs = (size_t)B * P.P_;
    if (P.compact && io->patch_slots > 0 && (size_t)io->patch_slots < P.NPs) P.NPs = (size_t)io->patch_slots;
    const int LIM = P.LIM;
    if (P.NPs * (size_t)(LIM * LIM) > 0x7fffffffffLL || P.NPs > 0x7ffffff0u / (size_t)LIM) { roitr_set_error("too many patch slots for one call", __FILE__, __LINE__); return ROITR_ERR_UNSUPPORTED; }
    return 0;
}

int plan_sizes(const Engine& E, const RoitrForwardIO* io, Plan& P)
{
    CHK(plan_clouds(E, io->n_points, 2 * io->pairs, P));
    return plan_pairs(E, io, P);
}

// ---- stage 4 (and the size of the alternating arena in stage 2): EVERY buffer the geometry chain writes, before the encoder's mark /
// release scopes.  G: what is written before the call begins on the main stream (the alternating arena in the ahead mode); GF: everything
// else the geometry stream writes.  Run against counting arenas this is also what sizes the alternating arena, so the two cannot differ.
void carve_geometry(const Engine& E, const RoitrForwardIO* io, const Plan& P, Arena& G, Arena& GF, GeoBufs& S)
{
    const Levels& V = P.V; const int NC = P.NC, T1 = P.T1, T4 = P.T4, LIM = P.LIM;
    S.desc = G.get<char>(Desc::bytes(NC, T4));
    S.pts_out = io->points_out ? io->points_out : io->points_geom;
    S.node_xyz = io->node_xyz ? io->node_xyz : GF.get<float>((size_t)T4 * 3);
    S.node_masks = io->node_masks ? io->node_masks : GF.get<int>(T4);
    S.kidx = io->node_knn_idx ? io->node_knn_idx : GF.get<int>((size_t)T4 * LIM);
    S.kmask = io->node_knn_mask ? io->node_knn_mask : GF.get<int>((size_t)T4 * LIM);
    S.fps_tmp = G.get<float>(T1);
    S.fps_tie[1] = G.get<int>(NC); S.fps_tie[2] = G.get<int>(NC);
    S.p[0] = io->points_geom; S.nrm[0] = io->normals;
    for (int l = 1; l < 4; ++l) {
        S.down[l] = G.get<int>(V.T[l]);
        S.p[l] = G.get<float>((size_t)V.T[l] * 3);
        S.nrm[l] = G.get<float>((size_t)V.T[l] * 3);
    }
    for (int l = 0; l < 4; ++l) {
        const int K = E.nsample[l];
        const int mcap = l == 0 ? T1 : V.T[l - 1];
        Arena& GA = (l == 0 && P.knn0_ahead) ? G : GF;
        S.knn_ws[l] = GA.get<char>(roitr_knn_workspace_bytes(NC, V.T[l], mcap));
        S.grid[l] = V.T[l] > GRID_MIN_POINTS * NC;
        S.g_self[l] = GA.get<int>((size_t)V.T[l] * K);
        S.ppf_self[l] = GA.get<float>((size_t)V.T[l] * K * 4);
        if (l > 0) {
            S.g_td[l] = GF.get<int>((size_t)V.T[l] * K);
            S.ppf_td[l] = GF.get<float>((size_t)V.T[l] * K * 4);
        } else {
            S.g_td[0] = S.g_self[0]; S.ppf_td[0] = S.ppf_self[0];  // stride 1: the same kNN (model/model.py:75 vs :31)
        }
        if (l < 3) { S.i3[l] = GF.get<int>((size_t)V.T[l] * 3); S.d3[l] = GF.get<float>((size_t)V.T[l] * 3); }
    }
    S.d_idx = GF.get<float>(P.etot);
    S.a_idx = GF.get<float>((size_t)P.etot * 3);
    if (!S.Emb) S.Emb = GF.get<float>((size_t)P.etot * P.C4);   // (an encode presets it: E is written into the caller's cache)
    S.c3 = GF.get<int>(V.T[2]);
    S.c4 = GF.get<int>(T4);
    S.p2n = GF.get<int>(T1);
    S.p2nd = GF.get<float>(T1);
    if (P.gt) {
        S.gt_pad = GF.get<float>((size_t)P.Tp * 3);
        S.gt_poff = GF.get<int>((size_t)3 * P.B + 4);
        S.gt_d2p = GF.get<float>(P.Tp);
        S.gt_ws_s = GF.get<char>(roitr_knn_workspace_bytes(P.B, P.Tsp, P.Ttp));
        S.gt_ws_t = GF.get<char>(roitr_knn_workspace_bytes(P.B, P.Ttp, P.Tsp));
    }
    if (P.gt_corr) {
        S.gt_om = GF.get<float>((size_t)P.B * V.nmax[3] * V.nmax[3]);
        S.gt_nt = GF.get<float>((size_t)T4 * 3);
        S.gt_nr = GF.get<float>(T4);
    }
}

int carve_geometry_buffers(Engine& E, const RoitrForwardIO* io, const Plan& P, GeoBufs& S)
{
    Arena& G = P.ahead ? E.garena[E.cur_par] : E.arena;
    Arena& GF = P.full_ahead ? G : E.arena;
    carve_geometry(E, io, P, G, GF, S);
    if (G.fail || GF.fail) {
        if (P.ahead) E.garena_short = true;   // roitr_engine_forward repeats the call on the main-stream path
        roitr_set_error("arena exhausted (geometry)", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    return 0;
}

// ---- stage 2: the scratch arena (upper bound from the sizes), the geometry stream and its events, the ordering mode and its arena
int reserve_arenas(Engine& E, const RoitrForwardIO* io, Plan& P)
{
    const Levels& V = P.V; hipStream_t st = P.st;
    const int B = P.B, NC = P.NC, T1 = P.T1, T4 = P.T4, C4 = P.C4, LIM = P.LIM, f = E.cfg.factor;
    {
        size_t need = (size_t)T1 * 4 * (64 * f * 14 + 256 * f * 2 + 600) + (size_t)P.etot * (C4 * 4 + 64) /* E once + its index arrays */ + (size_t)T4 * C4 * 4 * 18 +
                      P.NPs * (LIM * LIM * 3 + (LIM + 1) * (LIM + 1) + LIM * 6) * 4 + ((size_t)64 << 20);
        // (the global transformer's 20 (T4, C4) tensors, the coarse head's two, the coarse scratch, the correspondence and the patch row / mask /
        // point arrays are not in this bound: they live in the branch arena, sized below by counting)
        if (E.cfg.operand_dtype == 1) need += (size_t)T1 * C4 * 2 + 1024;   // bf16 copy of the point descriptors (patch scores)
        for (int l = 0; l < 4; ++l) need += roitr_knn_workspace_bytes(NC, V.T[l], T1) + 1024;
        need += 2 * roitr_knn_workspace_bytes(B, T1 + NC, T1 + NC) + (size_t)(T1 + NC) * 16 + 4096;
        if (need > E.arena.cap) {
            ROITR_HIP(hipStreamSynchronize(st));
            if (E.arena.base) ROITR_HIP(hipFree(E.arena.base));
            E.arena.base = nullptr; E.arena.cap = 0;
            ROITR_HIP(hipMalloc((void**)&E.arena.base, need));
            E.arena.cap = need; E.arena.peak = 0;
            E.arena_epoch++;
        }
        E.arena.off = 0; E.arena.fail = false;
    }
    if (!E.side) {
        // (a lower or higher queue priority for this stream changes nothing measurable: 97.3 / 98.2 / 98.2 ms per 512-pair step)
        // (round 5: the same stream confined to 32 / 64 / 96 / 128 / 192 CUs by hipExtStreamCreateWithCUMask, spread evenly over the XCDs,
        // with the main stream off the null stream so that the masked -- "blocking" -- stream does not serialise with it: 3 927 /
        // 5 768 / 6 004 / 5 969 / 5 949 pairs/s against 5 905 - 6 005 unmasked.  Confinement buys nothing: DESIGN.md section 4.)
        ROITR_HIP(hipStreamCreateWithFlags(&E.side, hipStreamNonBlocking));
        ROITR_HIP(hipStreamCreateWithFlags(&E.branch, hipStreamNonBlocking));
        for (int i = 0; i < Engine::NEV; ++i) ROITR_HIP(hipEventCreateWithFlags(&E.ev[i], hipEventDisableTiming));
    }
    hipStream_t sd = P.sd = E.side;
    P.sb = (E.phase_overlap == 2 || (E.phase_overlap == 1 && T4 >= BRANCH_MIN_NODES)) ? E.branch : st;
    if (P.B > 0) {   // the branch arena: exactly what carve_branch takes (counted the same way as the alternating arenas below); an encode has no branch
        Arena cnt; cnt.cap = ~(size_t)0;
        BranchBufs unused;
        carve_branch(io, P, cnt, unused);
        if (cnt.peak > E.barena.cap) {
            ROITR_HIP(hipStreamSynchronize(st));
            ROITR_HIP(hipStreamSynchronize(E.branch));
            if (E.barena.base) ROITR_HIP(hipFree(E.barena.base));
            E.barena.base = nullptr; E.barena.cap = 0;
            ROITR_HIP(hipMalloc((void**)&E.barena.base, cnt.peak));
            E.barena.cap = cnt.peak;
            E.arena_epoch++;
        }
        E.barena.off = 0; E.barena.peak = 0; E.barena.fail = false;
    }

    // ---------------- sampling ahead of the previous forward's tail (io->inputs_ready, include/roitr_engine.h).  `st` is in order,
    // so everything queued on it for this forward starts after the previous forward has left it -- but the first sampling level
    // (one serial chain per cloud: 0.9 ms for a 5000-point pair, 1/3 of a one-pair forward) needs the input coordinates only.
    // With the inputs ordered by an event instead of by `st`, the geometry stream copies the descriptors and runs that level
    // at once, beside the previous forward; the rest of the geometry chain writes scratch of the shared arena and waits, as
    // before, for the point of `st` where this forward begins.
    P.ahead = io->inputs_ready != nullptr && E.capture_pin == nullptr && !E.ahead_off;
    // ... and so does the level-1 grid + self kNN (+ PPF) the first transformer starts from: in the ahead mode it runs in front of the
    // sampling level on the geometry stream, its workspace and its group / PPF arrays in the alternating arena too (the previous call's
    // decoder still reads ITS level-1 groups) -- 3 ms per 512-pair step off the main stream's chain
    // up to 128 pairs per call: a small batch is bound by the main stream's chain (one pair per call 2.01 -> 1.87 ms, 64 pairs 12.25 -> 12.04 ms);
    // at 512 pairs the step is bound by the chip's total work and the move only shifts contention onto the GEMMs (5 843 / 5 886 vs 5 906 / 5 862
    // pairs/s, gemm_kernel 37.7 -> 38.9 ms per step)
    P.knn0_ahead = P.ahead && B <= AHEAD_MAX_PAIRS;
    // ... and with it the WHOLE geometry chain: for calls of up to 128 pairs every buffer the geometry stream writes lives in
    // the alternating arena, so the chain of call s + 1 needs nothing from the main stream: it runs beside call s from the first kernel to
    // the last and only waits for the call before that one (same arena) to have ended
    P.full_ahead = P.knn0_ahead;
    if (P.ahead) {
        Arena& G = E.garena[E.gpar];
        Arena cnt, rest;   // the size of the alternating arena: what carve_geometry takes from it (no base: only `off` advances)
        cnt.cap = rest.cap = ~(size_t)0;
        GeoBufs unused;
        carve_geometry(E, io, P, cnt, P.full_ahead ? cnt : rest, unused);
        const size_t need = cnt.off;
        if (need > G.cap) {
            ROITR_HIP(hipStreamSynchronize(st));
            ROITR_HIP(hipStreamSynchronize(sd));
            if (G.base) ROITR_HIP(hipFree(G.base));
            G.base = nullptr; G.cap = 0;
            const size_t cap = need + need / 8 + ((size_t)1 << 20);   // a margin, not a multiple: 2.4 GB at 128 pairs, twice (two arenas)
            if (hipMalloc((void**)&G.base, cap) == hipSuccess) G.cap = cap;
            else {   // no memory for the alternating arenas: this engine orders every call on the main stream from now on
                (void)hipGetLastError();
                G.base = nullptr;
                E.ahead_off = true;
                P.ahead = P.knn0_ahead = P.full_ahead = false;
            }
        }
    }
    if (io->inputs_ready && !P.ahead && E.capture_pin == nullptr) ROITR_HIP(hipStreamWaitEvent(st, (hipEvent_t)io->inputs_ready, 0));   // inputs ordered by the event all the same
    if (P.ahead) {
        Arena& G = E.garena[E.gpar];
        G.off = 0; G.fail = false;
        E.cur_par = E.gpar;
        if (!E.gend[E.gpar]) ROITR_HIP(hipEventCreateWithFlags(&E.gend[E.gpar], hipEventDisableTiming));
        // the call that used this arena before (two calls back) must have left the main stream: implied by `sd` waiting for
        // EV_MAIN_BEGIN in the partial mode, the only ordering left in the full one
        if (E.gend_rec[E.gpar]) ROITR_HIP(hipStreamWaitEvent(sd, E.gend[E.gpar], 0));
        E.gpar ^= 1;
        ROITR_HIP(hipStreamWaitEvent(sd, (hipEvent_t)io->inputs_ready, 0));
        E.side_forked = true;
    }
    return 0;
}

// ---- stage 3: the descriptor block, filled in a pinned staging buffer and copied on the stream the mode picks
int stage_descriptors(Engine& E, const Plan& P, GeoBufs& S)
{
    const Levels& V = P.V; const int B = P.B, NC = P.NC; hipStream_t st = P.st, sd = P.sd;
    const size_t desc_bytes = P.slot_cloud ? Desc::bytes_with_slots(NC, P.T4) : Desc::bytes(NC, P.T4);
    hipStream_t st_desc = P.ahead ? sd : st;   // the stream that stages the descriptors
    const int slot = E.ring_pos;
    char* pin = E.capture_pin;   // a captured forward owns its staging buffer (the graph re-reads it at every launch)
    if (!pin) {
        E.ring_pos = (E.ring_pos + 1) % Engine::RING;
        if (!E.pinned_ev[slot]) ROITR_HIP(hipEventCreateWithFlags(&E.pinned_ev[slot], hipEventDisableTiming));
        else ROITR_HIP(hipEventSynchronize(E.pinned_ev[slot]));  // the copy that last used this slot has finished
        if (desc_bytes > E.pinned_cap[slot]) {
            if (E.pinned[slot]) ROITR_HIP(hipHostFree(E.pinned[slot]));
            E.pinned_cap[slot] = desc_bytes * 2;
            ROITR_HIP(hipHostMalloc((void**)&E.pinned[slot], E.pinned_cap[slot], hipHostMallocDefault));
        }
        pin = E.pinned[slot];
    }
    const Desc H = Desc::at(pin, NC, P.T4);
    for (int l = 0; l < 4; ++l) memcpy(H.off[l], V.off[l].data(), sizeof(int) * NC);
    for (int c = 0, r = 0; c < NC; ++c) for (int i = 0; i < V.n[3][c]; ++i) H.cloud_of_node[r++] = c;
    for (int c = 0; c < NC; ++c) H.partner[c] = c < B ? c + B : c - B;
    memcpy(H.eoff, P.eoff.data(), sizeof(long) * NC);
    if (P.slot_cloud) memcpy(H.slot_cloud, P.slot_cloud, sizeof(int) * NC);
    ROITR_HIP(hipMemcpyAsync(S.desc, pin, desc_bytes, hipMemcpyHostToDevice, st_desc));
    if (!E.capture_pin) ROITR_HIP(hipEventRecord(E.pinned_ev[slot], st_desc));
    if (P.ahead) {   // `st` reads the descriptors (and the inputs) from here on
        ROITR_HIP(hipEventRecord(E.ev[Engine::EV_DESC_COPIED], sd));
        ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_DESC_COPIED], 0));
    }
    S.D = Desc::at(S.desc, NC, P.T4);
    return 0;
}

// ---- stage 5: the geometry chain
// level l's picks and their coordinates / normals: the part of the geometry chain that touches none of the shared scratch
int sample_level(const Plan& P, const GeoBufs& S, int l)
{
    const Levels& V = P.V; hipStream_t sd = P.sd;
    // tmp = 1e10 (functions/pointops.py:22)
    ROITR_HIP(hipMemsetD32Async((hipDeviceptr_t)S.fps_tmp, 0x501502F9 /* bits of 1e10f */, V.T[l - 1], sd));
    roitr_prof_next_bytes(ROITR_PROF_FPS, 12.0 * V.T[l - 1] + 4.0 * V.T[l] + 8.0 * V.T[l - 1]);
    // levels 2 and 3 sample the previous level's picks in pick order: answered with the prefix while no arg-max was
    // shared (pointops_fps.hip), the serial chain of 312 + 78 dependent iterations otherwise
    CHK(roitr_furthestsampling_ex(P.NC, V.nmax[l - 1], S.p[l - 1], S.D.off[l - 1], S.D.off[l], S.fps_tmp, S.down[l], l > 1 ? S.fps_tie[l - 1] : nullptr,
                                  l < 3 ? S.fps_tie[l] : nullptr, 4, sd));
    CHK(roitr_gather_rows(V.T[l], 3, S.p[l - 1], S.down[l], 0, (float*)S.p[l], sd));
    CHK(roitr_gather_rows(V.T[l], 3, S.nrm[l - 1], S.down[l], 0, (float*)S.nrm[l], sd));
    return ROITR_OK;
}

// the embedding of the global transformer (positional_encoding.py:139-154): needs the level-4 coordinates only
int issue_embedding(Engine& E, const Plan& P, const GeoBufs& S)
{
    const Desc& D = S.D; const int C4 = P.C4; const long etot = P.etot; hipStream_t sd = P.sd;
    CHK(roitr_geo_indices(P.T4, S.p[3], D.off[3], D.cloud_of_node, D.eoff, 0.2f, 15.0f, 3, P.V.nmax[3], S.d_idx, S.a_idx, sd));
    if (E.geo_tab && roitr_geo_embed_table(etot, C4, 3, S.d_idx, S.a_idx, E.geo_tab, E.geo_tab_h, E.geo_tab_nd, E.geo_tab_na, E.geo_div,
                                           E.proj_d.w, E.proj_d.b, E.proj_a.w, E.proj_a.b, S.Emb, P.e_h ? 1 : 0, sd) != ROITR_OK)
        E.geo_tab = nullptr;   // e.g. a device that does not grant the table's LDS: this engine serves the GEMM form from now on
    if (!E.geo_tab) {
        if (P.e_h)
            CHK(roitr_geo_embed_bf16_out(etot, C4, 3, S.d_idx, S.a_idx, E.geo_div, E.proj_d.wb, E.proj_d.b, E.proj_a.wb, E.proj_a.b,
                                         reinterpret_cast<unsigned short*>(S.Emb), sd));
        else if (E.cfg.operand_dtype == 1 && E.proj_d.wb && E.proj_a.wb)
            CHK(roitr_geo_embed_bf16(etot, C4, 3, S.d_idx, S.a_idx, E.geo_div, E.proj_d.wb, E.proj_d.b, E.proj_a.wb, E.proj_a.b, S.Emb, sd));
        else
            CHK(roitr_geo_embed(etot, C4, 3, S.d_idx, S.a_idx, E.geo_div, E.proj_d.w, E.proj_d.b, E.proj_a.w, E.proj_a.b, S.Emb, sd));
    }
    ROITR_HIP(hipEventRecord(E.ev[Engine::EV_EMBED_DONE], sd));
    return ROITR_OK;
}

// the chain's tail: the decoder's 3-NN, node coordinates, partition, ground-truth outputs
int issue_tail(Engine& E, const RoitrForwardIO* io, const Plan& P, const GeoBufs& S)
{
    const Levels& V = P.V; const Desc& D = S.D; hipStream_t sd = P.sd;
    const int B = P.B, NC = P.NC, T1 = P.T1, T4 = P.T4, LIM = P.LIM;
    // the decoder's 3-NN (pointops.py:168-182 `interpolation`): level-l points among the level-(l+1) points
    for (int l = 2; l >= 0; --l)
        CHK(roitr_knnquery_ex(NC, V.T[l + 1], V.T[l], 3, S.p[l + 1], S.p[l], D.off[l + 1], D.off[l], S.i3[l], S.d3[l], nullptr, nullptr, nullptr,
                              nullptr, S.grid[l + 1] ? 1 : 0, V.T[l], S.knn_ws[l + 1], sd));
    ROITR_HIP(hipEventRecord(E.ev[Engine::EV_NN3_DONE], sd));
    // From here on the chain writes the CALLER's output buffers (node_xyz, node_masks, node_knn_*, gt_*).  In the whole-chain-ahead
    // mode nothing so far has ordered this stream against the previous call on `st` -- but that call's matching phase may still
    // read ITS outputs through the same pointers (a C caller that reuses one set of buffers; torch's caching allocator handing a
    // freed block out again): wait for the point where this call begins on `st` (EV_MAIN_BEGIN, recorded behind everything the
    // previous call queued there).  The kernels below then run beside this call's encoder instead of the previous call's
    // tail; the matching phase, which needs them, is 1 - 2 ms further down the main stream.
    if (P.full_ahead) ROITR_HIP(hipStreamWaitEvent(sd, E.ev[Engine::EV_MAIN_BEGIN], 0));
    // node coordinates (model/model.py:233-235), point-to-node partition (lib/utils.py:428-471) and the ground-truth side
    // outputs: coordinates, the FPS picks and the given transform only
    CHK(roitr_compose_idx(V.T[2], S.down[1], S.down[2], S.c3, sd));  // level-3 nodes as level-1 rows
    CHK(roitr_compose_idx(T4, S.c3, S.down[3], S.c4, sd));
    CHK(roitr_gather_rows(T4, 3, S.pts_out, S.c4, 0, S.node_xyz, sd));
    CHK(roitr_point_to_node_partition(NC, T1, T4, S.pts_out, D.off[0], S.node_xyz, D.off[3], D.cloud_of_node, LIM, S.p2n, S.p2nd, S.node_masks,
                                      S.kidx, S.kmask, sd));
    // ---------------- ground-truth side outputs (RIGA_v2.py:91-116), only when rot / trans are given
    if (P.gt) {
        const int Tsp = P.Tsp, Ttp = P.Ttp;
        CHK(roitr_build_padded_clouds(B, T1, S.pts_out, D.off[0], io->rot, io->trans, S.gt_pad, S.gt_poff, sd));
        const float* src_p = S.gt_pad; const float* tgt_p = S.gt_pad + (size_t)Tsp * 3;
        const int* off_s = S.gt_poff; const int* off_t = S.gt_poff + 2 * B;
        const int use_grid = (Tsp > GRID_MIN_POINTS * B) ? 1 : 0;
        if (io->gt_node_occ) {
            // kNN(1) of every padded target point among the transformed padded source points, and back (l.509-510)
            float* d2p = S.gt_d2p;
            if (use_grid) CHK(roitr_knn_build_grid(B, Tsp, Ttp, src_p, off_s, S.gt_ws_s, sd));
            const float occ_cap2 = E.cfg.occlusion_radius * E.cfg.occlusion_radius * 1.01f;   // only `distance < radius` is read
            CHK(roitr_knn_within(B, Tsp, Ttp, src_p, tgt_p, off_s, off_t, occ_cap2, d2p + Tsp, use_grid, Ttp, S.gt_ws_s, sd));
            if (use_grid) CHK(roitr_knn_build_grid(B, Ttp, Tsp, tgt_p, off_t, S.gt_ws_t, sd));
            CHK(roitr_knn_within(B, Ttp, Tsp, tgt_p, src_p, off_t, off_s, occ_cap2, d2p, use_grid, Tsp, S.gt_ws_t, sd));
            CHK(roitr_node_occlusion_score(T4, LIM, D.cloud_of_node, D.off[0], S.kidx, S.kmask, S.node_masks, d2p, E.cfg.occlusion_radius,
                                           io->gt_node_occ, sd));
        }
        if (P.gt_corr) {
            const long ms = (long)V.nmax[3] * V.nmax[3];
            RoitrNodeCorr nc; memset(&nc, 0, sizeof(nc));
            nc.pairs = B; nc.limit = LIM; nc.max_nodes = V.nmax[3]; nc.pos_radius = E.cfg.matching_radius;
            nc.nodes = S.node_xyz; nc.node_offset = D.off[3]; nc.node_masks = S.node_masks; nc.points = S.pts_out; nc.pt_offset = D.off[0];
            nc.knn_idx = S.kidx; nc.knn_mask = S.kmask; nc.rot = io->rot; nc.trans = io->trans; nc.overlap = S.gt_om; nc.mat_stride = ms;
            nc.out_idx = io->gt_corr_idx; nc.out_overlap = io->gt_corr_overlaps; nc.out_count = io->gt_corr_count;
            nc.n_nodes = T4; nc.nodes_t = S.gt_nt; nc.radius = S.gt_nr;
            CHK(roitr_node_correspondences(&nc, sd));
        }
    }
    ROITR_HIP(hipEventRecord(E.ev[Engine::EV_TAIL_DONE], sd));
    return ROITR_OK;
}

// hierarchy: the GEOMETRY CHAIN on a side stream, the feature path on the main one
// (model/model.py:56-80, 30-42, 195-205).  Everything here depends on the input coordinates only: the FPS chain, the
// grids, self / TransitionDown kNN groups + PPF of levels 2-4, the decoder's 3-NN, the distance / angle indices and the
// embedding E of the global transformer.  These kernels are issue- / latency- / LDS-bound (FPS: one long serial workgroup
// per cloud; kNN: VALU issue; geo_table: LDS), the feature path beside them is MFMA- and HBM-bound, so they share the chip
// instead of queueing in front of each level (round 3; the FPS chain alone since round 1).  Level 1's grid and self kNN stay on
// the main stream (the first transformer needs them at once).  Level l's feature work waits for "level l geometry done" only.
int issue_geometry_chain(Engine& E, const RoitrForwardIO* io, const Plan& P, GeoBufs& S)
{
    const Levels& V = P.V; const Desc& D = S.D; const int NC = P.NC, T1 = P.T1; hipStream_t st = P.st, sd = P.sd;
    // ---- level-1 grid + self kNN (+ PPF): on the main stream (the first transformer needs them at once), or -- ahead mode -- in
    // front of everything else on the geometry stream, beside the previous call
    hipStream_t s0 = P.knn0_ahead ? sd : st;
    if (S.grid[0]) {
        // 6 points per cell on average: at level 1 (k = 8) the sphere of one cell size then holds ~2.5 (k + 2) points, what
        // the prefilter kNN kernel's radius rule needs
        CHK(roitr_knn_build_grid_ex(NC, V.T[0], T1, S.p[0], D.off[0], S.knn_ws[0], GRID_OCC, s0));
        S.order[0] = roitr_knn_sorted_points(NC, V.T[0], T1, S.knn_ws[0]);
    }
    if (!P.knn0_ahead) ROITR_HIP(hipEventRecord(E.ev[Engine::EV_MAIN_BEGIN], st));  // inputs + descriptors are in place
    CHK(roitr_knnquery_ex(NC, V.T[0], V.T[0], E.nsample[0] + 1, S.p[0], S.p[0], D.off[0], D.off[0], nullptr, nullptr, S.g_self[0], S.ppf_self[0],
                          S.nrm[0], S.nrm[0], S.grid[0] ? 1 : 0, T1, S.knn_ws[0], s0));
    if (P.knn0_ahead) {
        ROITR_HIP(hipEventRecord(E.ev[Engine::EV_LEVEL1_GROUPS_READY], sd));   // the level-1 groups and PPFs are in place
        ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_LEVEL1_GROUPS_READY], 0));
        ROITR_HIP(hipEventRecord(E.ev[Engine::EV_MAIN_BEGIN], st));            // where this call begins on the main stream: the shared scratch is free from here
    } else
        ROITR_HIP(hipEventRecord(E.ev[Engine::EV_LEVEL1_WS_FREE], st));  // the level-1 workspace (grid + retry list) is free for the TransitionDown query
    if (P.ahead) CHK(sample_level(P, S, 1));

    // ---- side stream
    if (!P.full_ahead) ROITR_HIP(hipStreamWaitEvent(sd, E.ev[Engine::EV_MAIN_BEGIN], 0));   // (full mode: nothing below touches the shared arena)
    E.side_forked = true;
    for (int l = 1; l < 4; ++l) {
        const int K = E.nsample[l];
        if (!(P.ahead && l == 1)) CHK(sample_level(P, S, l));
        // grid over this level's points (refs for: own self-kNN, next level's TD query, finer level's 3-NN)
        if (S.grid[l]) {
            CHK(roitr_knn_build_grid_ex(NC, V.T[l], V.T[l - 1], S.p[l], D.off[l], S.knn_ws[l], GRID_OCC, sd));
            S.order[l] = roitr_knn_sorted_points(NC, V.T[l], V.T[l - 1], S.knn_ws[l]);
        }
        CHK(roitr_knnquery_ex(NC, V.T[l], V.T[l], K + 1, S.p[l], S.p[l], D.off[l], D.off[l], nullptr, nullptr, S.g_self[l], S.ppf_self[l], S.nrm[l],
                              S.nrm[l], S.grid[l] ? 1 : 0, V.T[l - 1], S.knn_ws[l], sd));
        if (l == 1 && !P.knn0_ahead) ROITR_HIP(hipStreamWaitEvent(sd, E.ev[Engine::EV_LEVEL1_WS_FREE], 0));   // (ahead mode: that query ran on this stream)
        const int mcap_prev = l - 1 == 0 ? T1 : V.T[l - 2];
        CHK(roitr_knnquery_ex(NC, V.T[l - 1], V.T[l], K + 1, S.p[l - 1], S.p[l], D.off[l - 1], D.off[l], nullptr, nullptr, S.g_td[l],
                              S.ppf_td[l], S.nrm[l - 1], S.nrm[l], S.grid[l - 1] ? 1 : 0, mcap_prev, S.knn_ws[l - 1], sd));
        ROITR_HIP(hipEventRecord(E.ev[Engine::ev_level_done(l)], sd));
    }
    // The embedding E and the chain's tail (3-NN, partition, ground-truth outputs).  (Round 4 measured both units queued behind
    // encoder level 1, 2 or 3 instead of here: no effect on the step)
    CHK(issue_embedding(E, P, S));
    return issue_tail(E, io, P, S);
}

// ---- stage 6: the encoder (model/model.py:195-205), level l behind "level l geometry done"
int encoder(Engine& E, const RoitrForwardIO* io, const Plan& P, const GeoBufs& S, Feats& F)
{
    const Levels& V = P.V; const int T1 = P.T1; hipStream_t st = P.st; Arena& A = E.arena;
    const float* xin = io->feats;
    for (int l = 0; l < 4; ++l) {
        const int K = E.nsample[l], pl = E.planes[l];
        if (l > 0) {
            ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::ev_level_done(l)], 0));
            CHK(tap(E, st, "fps." + std::to_string(l + 1), S.down[l], sizeof(int) * V.T[l]));
        }
        CHK(tap(E, st, "group.self." + std::to_string(l + 1), S.g_self[l], sizeof(int) * (size_t)V.T[l] * K));
        CHK(tap(E, st, "ppf.self." + std::to_string(l + 1), S.ppf_self[l], sizeof(float) * (size_t)V.T[l] * K * 4));
        if (l > 0) {
            CHK(tap(E, st, "group.td." + std::to_string(l + 1), S.g_td[l], sizeof(int) * (size_t)V.T[l] * K));
            CHK(tap(E, st, "ppf.td." + std::to_string(l + 1), S.ppf_td[l], sizeof(float) * (size_t)V.T[l] * K * 4));
        }
        // ---- encoder level l
        float* a = A.get<float>((size_t)V.T[l] * pl);
        float* b = A.get<float>((size_t)V.T[l] * pl);
        if (A.fail) break;
        const int n_in = l == 0 ? T1 : V.T[l - 1];
        CHK(local_transformer(E, st, E.enc[l][0], {n_in, xin, V.T[l], l == 0 ? nullptr : S.down[l], S.g_td[l], S.ppf_td[l], S.order[l]}, a));
        CHK(tap(E, st, "enc" + std::to_string(l + 1) + ".0", a, sizeof(float) * (size_t)V.T[l] * pl));
        float* cur = a; float* nxt = b;
        for (int bi = 1; bi < E.nblocks[l]; ++bi) {
            CHK(local_transformer(E, st, E.enc[l][bi], {V.T[l], cur, V.T[l], nullptr, S.g_self[l], S.ppf_self[l], S.order[l]}, nxt));
            CHK(tap(E, st, "enc" + std::to_string(l + 1) + "." + std::to_string(bi), nxt, sizeof(float) * (size_t)V.T[l] * pl));
            float* t = cur; cur = nxt; nxt = t;
        }
        F.xe[l] = cur; xin = cur;
    }
    if (A.fail) { roitr_set_error("arena exhausted (encoder)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    return 0;
}

// ---- stage 7: the global geometric transformer (geotransformer.py:94-133), all pairs batched
// Queued on the branch's stream (P.sb), in the branch's buffers: it reads the encoder's last level and E, and only the coarse head reads
// its output, so it runs beside the decoder.
// the input projection of the global transformer: per cloud (roitr_engine_encode writes these rows into the cache)
int geo_in_proj(Engine& E, hipStream_t st, int T4, const float* xe4, float* out)
{
    CHK(Gemm(T4, xe4, E.geo_in, out).run(st));
    return tap(E, st, "geo.in_proj", out, sizeof(float) * (size_t)T4 * E.geo_in.out);
}

int global_layers(Engine& E, const Plan& P, const GeoBufs& S, Feats& F, const BranchBufs& R);

int global_transformer(Engine& E, const Plan& P, const GeoBufs& S, Feats& F, const BranchBufs& R)
{
    hipStream_t st = P.sb; const int T4 = P.T4, C4 = P.C4; const long etot = P.etot; const bool e_h = P.e_h;
    ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_EMBED_DONE], 0));   // E and its index arrays were written on the side stream
    CHK(tap(E, st, "geo.d_idx", S.d_idx, sizeof(float) * etot));
    CHK(tap(E, st, "geo.a_idx", S.a_idx, sizeof(float) * etot * 3));
    CHK(tap(E, st, "geo.emb", S.Emb, (e_h ? sizeof(unsigned short) : sizeof(float)) * (size_t)etot * C4));   // bf16 mode: the tap holds bf16
    CHK(geo_in_proj(E, st, T4, F.xe[3], R.fcur));
    return global_layers(E, P, S, F, R);
}

// the layers of the global transformer and its output projection over the rows of R.fcur (what roitr_engine_match starts from: its
// fcur rows are the cached geo_in rows of the call's cloud slots, its E the cache's, addressed per slot through D.eoff)
int global_layers(Engine& E, const Plan& P, const GeoBufs& S, Feats& F, const BranchBufs& R)
{
    const Levels& V = P.V; const Desc& D = S.D; hipStream_t st = P.sb; Arena& A = E.barena;
    const int B = P.B, T4 = P.T4, C4 = P.C4; const long etot = P.etot; const bool e_h = P.e_h;
    float* gfeat = F.gfeat = R.gfeat;
    float *fcur = R.fcur, *pos = R.pos, *qkv = R.qkv, *qt = R.qt, *ebar = R.ebar, *hid = R.hid, *t1 = R.t1, *t2 = R.t2;
    const int cpe = C4 / HEADS;
    const float scale = 1.0f / sqrtf((float)cpe);
    const int Ts = V.off[3][B - 1];  // source-cloud rows come first
    for (size_t li = 0; li < E.geo.size(); ++li) {
        const GeoLayer& L = E.geo[li];
        if (!L.cross) {
            CHK(Gemm(T4, 3 * C4, C4, fcur, C4, L.wqkv, C4, L.bqkv, qkv, 3 * C4).bf16_weight(L.wqkv_b).run(st));
            // qt[(row,h), :] = Wp_h^T q_h   (batched over heads)
            CHK(Gemm(T4, C4, cpe, qkv, 3 * C4, L.wpT, C4, nullptr, qt, HEADS * C4).heads(HEADS, cpe, cpe, C4).bf16_weight(L.wpT_b).run(st));
            RoitrMha m; memset(&m, 0, sizeof(m));
            m.q_row0 = 0; m.q_rows = T4; m.C = C4; m.heads = HEADS; m.q = qkv; m.ldq = 3 * C4; m.k = qkv + C4; m.ldk = 3 * C4;
            m.v = qkv + 2 * C4; m.ldv = 3 * C4; m.offset = D.off[3]; m.cloud_of_row = D.cloud_of_node; m.partner = nullptr;
            m.E = S.Emb; m.eoff = D.eoff; m.qt = qt; m.bp = L.p.b; m.scale = scale; m.nk_max = V.nmax[3]; m.out = hid; m.ldo = C4; m.ebar = ebar;
            m.e_bf16 = e_h ? 1 : 0;
            // algorithmic bytes of the launch: E read once, q | k | v, the folded queries q~, out and ebar written once
            roitr_prof_next_bytes(ROITR_PROF_MHA, (double)etot * C4 * (e_h ? 2.0 : 4.0) + (double)T4 * C4 * 4.0 * (3 + HEADS + 1 + HEADS));
            CHK(roitr_mha(&m, st));
            // pos_raw[:, h-slice] = Wvp_h ebar_h + bvp_h
            CHK(Gemm(T4, cpe, C4, ebar, HEADS * C4, L.vp.w, C4, L.vp.b, t2, C4).heads(HEADS, C4, (long)cpe * C4, cpe, cpe).bf16_weight(L.vp.wb).run(st));
            // RPEAttentionLayer tail (geoattention.py:236-244) + AttentionOutput x2 (l.278-280)
            // (in place is safe for the fused form: a block reads and writes only its own 64 rows)
            CHK(Gemm(T4, hid, L.lin, hid).ln(L.n_w, L.n_b).residual(fcur).run_ln(st, t1));
            CHK(ffn_apply(A, st, L.out, T4, C4, hid, fcur));
            CHK(Gemm(T4, t2, L.pos_lin, t2).ln(L.pn_w, L.pn_b).run_ln(st, t1));
            CHK(ffn_apply(A, st, L.pos, T4, C4, t2, pos));
            CHK(tap(E, st, "geo.layer" + std::to_string(li) + ".pos", pos, sizeof(float) * (size_t)T4 * C4));
        } else {
            // geotransformer.py:45-46: feats0 (src) attends feats1 (tgt), then feats1 attends the UPDATED feats0
            for (int half = 0; half < 2; ++half) {
                const int q0 = half == 0 ? 0 : Ts, qn = half == 0 ? Ts : T4 - Ts;
                const int k0 = half == 0 ? Ts : 0, kn = half == 0 ? T4 - Ts : Ts;
                float* qb_ = qkv;                          // (T4, C4) region reused: q rows at their own row index
                float* kb_ = qkv + (size_t)T4 * C4;
                float* vb_ = qkv + (size_t)2 * T4 * C4;
                CHK(Gemm(qn, fcur + (size_t)q0 * C4, L.q, qb_ + (size_t)q0 * C4).plus(pos + (size_t)q0 * C4).run(st));
                CHK(Gemm(kn, fcur + (size_t)k0 * C4, L.k, kb_ + (size_t)k0 * C4).plus(pos + (size_t)k0 * C4).run(st));
                CHK(Gemm(kn, fcur + (size_t)k0 * C4, L.v, vb_ + (size_t)k0 * C4).run(st));
                RoitrMha m; memset(&m, 0, sizeof(m));
                m.q_row0 = q0; m.q_rows = qn; m.C = C4; m.heads = HEADS; m.q = qb_; m.ldq = C4; m.k = kb_; m.ldk = C4; m.v = vb_; m.ldv = C4;
                m.offset = D.off[3]; m.cloud_of_row = D.cloud_of_node; m.partner = D.partner; m.scale = scale; m.nk_max = V.nmax[3];
                m.out = hid; m.ldo = C4;
                roitr_prof_next_bytes(ROITR_PROF_MHA, ((double)qn * 2 + (double)kn * 2) * C4 * 4.0);
                CHK(roitr_mha(&m, st));
                CHK(Gemm(qn, hid + (size_t)q0 * C4, L.lin, t2 + (size_t)q0 * C4).ln(L.n_w, L.n_b).residual(fcur + (size_t)q0 * C4).run_ln(st, t1 + (size_t)q0 * C4));
                CHK(ffn_apply(A, st, L.out, qn, C4, t2 + (size_t)q0 * C4, fcur + (size_t)q0 * C4));
            }
        }
        CHK(tap(E, st, "geo.layer" + std::to_string(li), fcur, sizeof(float) * (size_t)T4 * C4));
    }
    CHK(Gemm(T4, fcur, E.geo_out, gfeat).run(st));
    CHK(tap(E, st, "geo.out", gfeat, sizeof(float) * (size_t)T4 * C4));
    return 0;
}

// ---- stage 8: the decoder (model/model.py:223-231)
int decoder(Engine& E, const Plan& P, const GeoBufs& S, Feats& F)
{
    const Levels& V = P.V; const Desc& D = S.D; const int NC = P.NC, T4 = P.T4; hipStream_t st = P.st; Arena& A = E.arena;
    float** xe = F.xe; float** xd = F.xd;
    {
        // dec4 head: cat(x, linear2(mean).repeat) -> linear1 -> LN -> ReLU   (model/model.py:99-111)
        const int pl = E.planes[3];
        const Up& U = E.up[3];
        float* mean = A.get<float>((size_t)NC * pl);
        float* tm = A.get<float>((size_t)NC * pl);
        float* um = A.get<float>((size_t)NC * pl);
        float* y = A.get<float>((size_t)T4 * pl);
        float* x0 = A.get<float>((size_t)T4 * pl);
        xd[3] = A.get<float>((size_t)T4 * pl);
        if (A.fail) { roitr_set_error("arena exhausted (decoder)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
        CHK(roitr_segment_mean(NC, pl, xe[3], D.off[3], mean, st));
        CHK(Gemm(NC, mean, U.l2, tm).with_relu().run(st));
        CHK(Gemm(NC, pl, pl, tm, pl, U.l1.w + pl, 2 * pl, U.l1.b, um, pl).bf16_weight(U.l1.wb ? U.l1.wb + pl : nullptr).run(st));
        CHK(Gemm(T4, pl, pl, xe[3], pl, U.l1.w, 2 * pl, nullptr, y, pl).bf16_weight(U.l1.wb).run(st));
        CHK(roitr_add_layernorm(T4, pl, y, um, D.cloud_of_node, U.l1n_w, U.l1n_b, nullptr, 1, 1e-5f, x0, st));
        CHK(tap(E, st, "dec4.0", x0, sizeof(float) * (size_t)T4 * pl));
        CHK(local_transformer(E, st, E.dec[3], {T4, x0, T4, nullptr, S.g_self[3], S.ppf_self[3], S.order[3]}, xd[3]));
        CHK(tap(E, st, "dec4.1", xd[3], sizeof(float) * (size_t)T4 * pl));
    }
    ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_NN3_DONE], 0));   // the 3-NN of the three TransitionUp layers (side stream)
    for (int l = 2; l >= 0; --l) {
        // TransitionUp (model/model.py:112-116): linear1(x1) + interpolation(p2, p1, linear2(x2))
        const int pl = E.planes[l];
        const Up& U = E.up[l];
        const int Tl = V.T[l], Tc = V.T[l + 1];
        float* a0 = A.get<float>((size_t)Tl * pl);
        float* a1 = A.get<float>((size_t)Tl * pl);
        float* b0 = A.get<float>((size_t)Tc * pl);
        float* b1 = A.get<float>((size_t)Tc * pl);
        float* x0 = A.get<float>((size_t)Tl * pl);
        xd[l] = A.get<float>((size_t)Tl * pl);
        if (A.fail) { roitr_set_error("arena exhausted (decoder)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
        CHK(Gemm(Tc, xd[l + 1], U.l2, b1).ln(U.l2n_w, U.l2n_b, true).run_ln(st, b0));
        if (E.cfg.operand_dtype != 1) {
            // fp32: `linear1(x1) + interpolation(p2, p1, linear2(x2))` in the launch that computes linear1 -- the interpolation rides in
            // the LayerNorm epilogue (after the ReLU), the (Tl, pl) intermediate a1 is never written
            CHK(Gemm(Tl, xe[l], U.l1, x0).ln(U.l1n_w, U.l1n_b, true).interp3(b1, S.i3[l], S.d3[l]).run_ln(st, a0));
        } else {
            CHK(Gemm(Tl, xe[l], U.l1, a1).ln(U.l1n_w, U.l1n_b, true).run_ln(st, a0));
            CHK(roitr_interp3_add(Tl, pl, b1, S.i3[l], S.d3[l], a1, x0, st));
        }
        CHK(tap(E, st, "dec" + std::to_string(l + 1) + ".0", x0, sizeof(float) * (size_t)Tl * pl));
        CHK(local_transformer(E, st, E.dec[l], {Tl, x0, Tl, nullptr, S.g_self[l], S.ppf_self[l], S.order[l]}, xd[l]));
        CHK(tap(E, st, "dec" + std::to_string(l + 1) + ".1", xd[l], sizeof(float) * (size_t)Tl * pl));
    }
    return 0;
}

// ---- stage 9a: the coarse front of the matching phase (RIGA_v2.py:64-66, 118-125): coarse head, coarse matching, patch slots and patch
// arrays.  It needs the global features and the geometry chain's tail only, so it follows the global transformer on the branch's stream.
int coarse_front(Engine& E, const Plan& P, const GeoBufs& S, const Feats& F, const BranchBufs& R)
{
    const Levels& V = P.V; const Desc& D = S.D; hipStream_t st = P.sb;
    const int B = P.B, T4 = P.T4, C4 = P.C4, LIM = P.LIM, P_ = P.P_; const bool compact = P.compact;
    const size_t NP = P.NPs;
    if (P.sd) ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_TAIL_DONE], 0));   // node masks, partition and ground-truth side outputs (side stream)
    CHK(Gemm(T4, F.gfeat, E.coarse_proj, R.cp).run(st));
    CHK(roitr_l2_normalize(T4, C4, R.cp, R.node_feats, st));
    {   // all tgt_b x src_b feature dot products in one ragged-batched GEMM (rows: tgt cloud B+b, cols: src cloud b)
        Gemm g(V.nmax[3], V.nmax[3], C4, R.node_feats, C4, R.node_feats, C4, nullptr, R.cxy, V.nmax[3]);
        g.heads(B, 0, 0, R.xystride).activations();
        g.seg_off = D.off[3]; g.seg_a0 = B; g.seg_w0 = 0;
        CHK(g.run(st));
    }
    {
        RoitrCoarse c; memset(&c, 0, sizeof(c));
        c.pairs = B; c.C = C4; c.num_corr = P_; c.dual_norm = 1; c.max_ref = V.nmax[3]; c.max_src = V.nmax[3];
        c.feats = R.node_feats; c.node_offset = D.off[3]; c.node_masks = S.node_masks; c.scratch = R.cscratch; c.scratch_stride = R.cstride;
        c.tgt_corr = R.tgt_corr; c.src_corr = R.src_corr; c.corr_scores = R.cscore; c.n_corr = R.n_corr;
        c.xy = R.cxy; c.xy_stride = R.xystride; c.xy_ld = V.nmax[3];
        if (E.cfg.adaptive_coarse) CHK(roitr_adaptive_matching(&c, E.cfg.num_corr, 0.75f, st));
        else CHK(roitr_coarse_matching(&c, st));
    }
    // the tail runs on the selected patches only (RIGA_v2.py:126-152): their slots, pair after pair
    if (compact) CHK(roitr_patch_offsets(B, R.n_corr, (int)NP, R.pair_off, st));
    if (P.cache) {   // a match: node and point segments of both sides from the cloud table, rows of the cache's point arrays
        RoitrCachePatch cg; memset(&cg, 0, sizeof(cg));
        cg.pairs = B; cg.num_corr = P_; cg.limit = LIM; cg.n_corr = R.n_corr; cg.tgt_corr = R.tgt_corr; cg.src_corr = R.src_corr;
        cg.seg = P.cache->seg_dev; cg.slot_cloud = D.slot_cloud;
        cg.knn_idx = P.cache->node_knn_idx; cg.knn_mask = P.cache->node_knn_mask; cg.points = P.cache->points;
        cg.tgt_rows = R.trows; cg.src_rows = R.srows; cg.tgt_masks = R.tmask; cg.src_masks = R.smask; cg.tgt_pts = R.tpts; cg.src_pts = R.spts;
        CHK(roitr_cache_patch_gather(&cg, st));
    } else {
        RoitrPatch pg; memset(&pg, 0, sizeof(pg));
        pg.pairs = B; pg.num_corr = P_; pg.limit = LIM; pg.n_corr = R.n_corr; pg.tgt_corr = R.tgt_corr; pg.src_corr = R.src_corr;
        pg.node_offset = D.off[3]; pg.pt_offset = D.off[0]; pg.knn_idx = S.kidx; pg.knn_mask = S.kmask; pg.points = S.pts_out;
        pg.tgt_rows = R.trows; pg.src_rows = R.srows; pg.tgt_masks = R.tmask; pg.src_masks = R.smask; pg.tgt_pts = R.tpts; pg.src_pts = R.spts;
        pg.pair_off = R.pair_off; pg.slots = compact ? (int)NP : 0;
        CHK(roitr_patch_gather(&pg, st));
    }
    return 0;
}

// ---- stage 9b: the fine head (RIGA_v2.py:67-68) behind the decoder, then -- behind the branch -- patch scores, optimal transport, fine matching
int matching_tail(Engine& E, const RoitrForwardIO* io, const Plan& P, const BranchBufs& R, const float* point_feats, int feat_rows);

int heads_and_matching(Engine& E, const RoitrForwardIO* io, const Plan& P, const Feats& F, const BranchBufs& R)
{
    hipStream_t st = P.st; Arena& A = E.arena;
    const int T1 = P.T1, C4 = P.C4;
    float* point_feats = io->point_feats ? io->point_feats : A.get<float>((size_t)T1 * C4);
    if (A.fail) { roitr_set_error("arena exhausted (heads)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    CHK(Gemm(T1, F.xd[0], E.fine_proj, point_feats).run(st));
    // the last join: the branch, and the geometry chain's tail (the branch waited for it; the main stream waits for it as well, so
    // that a capture sees every stream joined by the stream it began on)
    if (P.sb != st) {
        ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_BRANCH_DONE], 0));
        ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_TAIL_DONE], 0));
    }
    // everything the other two streams were given is ordered before `st` from here (on one stream coarse_front, queued just in front of this
    // function, took the EV_TAIL_DONE wait on `st`)
    E.side_forked = false; E.branch_forked = false;
    return matching_tail(E, io, P, R, point_feats, T1);
}

// patch scores, optimal transport, fine matching over the patch arrays of coarse_front.  point_feats (feat_rows, C4): the rows the patch
// rows index -- the call's own fine-head output, or (roitr_engine_match) the cached descriptors of every cloud of the table
int matching_tail(Engine& E, const RoitrForwardIO* io, const Plan& P, const BranchBufs& R, const float* point_feats, int feat_rows)
{
    hipStream_t st = P.st; Arena& A = E.arena;
    const int B = P.B, T1 = feat_rows, C4 = P.C4, LIM = P.LIM, P_ = P.P_; const bool compact = P.compact;
    const int* n_corr = R.n_corr; const int* pair_off = R.pair_off; const float* cscore = R.cscore;
    const int *trows = R.trows, *srows = R.srows, *tmask = R.tmask, *smask = R.smask; const float *tpts = R.tpts, *spts = R.spts;
    const size_t NP = P.NPs;
    float* mscore = A.get<float>(NP * LIM * LIM);
    float* ot = io->matching_scores ? io->matching_scores : A.get<float>(NP * (LIM + 1) * (LIM + 1));
    unsigned char* flags = A.get<unsigned char>(NP * LIM * LIM);
    int* counts = A.get<int>(NP);
    int* offsets = io->fine_offsets ? io->fine_offsets : A.get<int>(NP);
    int* n_out = io->n_out ? io->n_out : A.get<int>(1);
    const size_t cap = NP * LIM * (size_t)E.cfg.fine_topk * (E.cfg.fine_mutual ? 1 : 2);   // row top-k OR column top-k when not mutual
    float* o_t = io->out_tgt_pts ? io->out_tgt_pts : A.get<float>(cap * 3);
    float* o_s = io->out_src_pts ? io->out_src_pts : A.get<float>(cap * 3);
    float* o_sc = io->out_scores ? io->out_scores : A.get<float>(cap);
    if (A.fail) { roitr_set_error("arena exhausted (matching)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    const int* live_patches = compact ? pair_off + B : nullptr;
    {   // matching_scores = einsum('bnd,bmd->bnm', tgt, src) / sqrt(C)   (RIGA_v2.py:150-152)
        Gemm g(LIM, LIM, C4, point_feats, C4, point_feats, C4, nullptr, mscore, LIM);
        g.gather(trows).heads((int)NP, 0, 0, (long)LIM * LIM).activations();
        g.a_limit = T1; g.w_idx = srows; g.w_limit = T1; g.alpha = 1.0f / sqrtf((float)C4); g.sAidx = LIM; g.sWidx = LIM;
        g.batch_live = live_patches;   // compacted list: the products of the live patches only
        if (E.cfg.operand_dtype == 1) {
            // bf16 operand mode: both operands of this contraction are the point descriptors -- one bf16 copy of them, products on
            // the bf16 matrix cores, fp32 accumulate; the scores (and the optimal transport behind them) stay fp32
            unsigned short* pf_h = A.get<unsigned short>((size_t)T1 * C4);
            if (A.fail) { roitr_set_error("arena exhausted (matching)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
            Gemm gh = g;
            gh.A = reinterpret_cast<const float*>(pf_h); gh.W = reinterpret_cast<const float*>(pf_h); gh.bf16 = ROITR_BF16_W | ROITR_BF16_A;
            if (roitr_gemm_bf16_supported(&gh)) {
                CHK(roitr_f32_to_bf16((long)T1 * C4, point_feats, pf_h, st));
                g = gh;
            }
        }
        CHK(g.run(st));
    }
    {   // optimal transport and fine matching: the transport wave of a patch also sets the patch's flags (roitr_matching_tail)
        RoitrOT o; memset(&o, 0, sizeof(o));
        o.pairs = B; o.num_corr = P_; o.limit = LIM; o.num_iter = 100; o.n_corr = n_corr; o.scores = mscore; o.row_masks = tmask;
        o.col_masks = smask; o.alpha = E.ot_alpha; o.out = ot;
        o.pair_off = pair_off; o.slots = compact ? (int)NP : 0;
        RoitrFine fm; memset(&fm, 0, sizeof(fm));
        fm.pairs = B; fm.num_corr = P_; fm.limit = LIM; fm.k = E.cfg.fine_topk; fm.mutual = E.cfg.fine_mutual; fm.conf = E.cfg.fine_conf;
        fm.n_corr = n_corr; fm.ot = ot; fm.row_masks = tmask; fm.col_masks = smask; fm.row_pts = tpts; fm.col_pts = spts;
        fm.global_scores = E.cfg.fine_use_global_score ? cscore : nullptr;
        fm.flags = flags; fm.counts = counts; fm.offsets = offsets; fm.n_out = n_out;
        fm.out_row_pts = o_t; fm.out_col_pts = o_s; fm.out_scores = o_sc; fm.out_patch = io->out_patch; fm.out_cap = (long)cap;
        fm.pair_off = pair_off; fm.slots = compact ? (int)NP : 0; fm.pair_starts = io->pair_starts;
        CHK(roitr_matching_tail(&o, &fm, st));
    }
    return 0;
}
}  // namespace

// One forward = this list of stages, no host synchronisation.  The geometry chain is queued whole before the feature path, which joins
// it stage by stage: encoder level l behind "level l geometry done", the global transformer behind the embedding, the decoder's
// TransitionUp layers behind the 3-NN, the coarse front behind the chain's tail.  Behind the encoder the feature path forks once more:
// the global transformer and the coarse front (the branch, on the engine's third stream) run beside the decoder and the fine head, and
// the main stream joins the branch in front of the patch score product.  The host queues the branch first (the other order measures the
// same at 512 pairs per call: DESIGN.md section 4, "Global transformer beside the decoder").
static int forward_body(Engine& E, const RoitrForwardIO* io, hipStream_t st)
{
    if (!E.finalized) { roitr_set_error("engine not finalized", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    if (io->pairs <= 0) return 0;
    Plan P; GeoBufs S; Feats F; BranchBufs R;
    P.st = st;
    CHK(plan_sizes(E, io, P));
    CHK(reserve_arenas(E, io, P));
    CHK(carve_geometry_buffers(E, io, P, S));   // (host work only; in front of the staging because the descriptor block is one of the buffers)
    carve_branch(io, P, E.barena, R);
    if (E.barena.fail) { roitr_set_error("arena exhausted (branch)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    CHK(stage_descriptors(E, P, S));
    hipStream_t sb = P.sb;
    roitr_prof_begin(ROITR_PROF_PH_FORWARD, 0.0, st);
    CHK(issue_geometry_chain(E, io, P, S));
    roitr_prof_begin(ROITR_PROF_PH_ENC, 0.0, st);   CHK(encoder(E, io, P, S, F));             roitr_prof_end(ROITR_PROF_PH_ENC, st);
    if (sb != st) {   // fork: the branch starts where the encoder's outputs are written
        ROITR_HIP(hipEventRecord(E.ev[Engine::EV_ENCODER_DONE], st));
        ROITR_HIP(hipStreamWaitEvent(sb, E.ev[Engine::EV_ENCODER_DONE], 0));
        E.branch_forked = true;
    }
    const bool forked = sb != st;
    E.on_branch = forked;
    roitr_prof_begin(ROITR_PROF_PH_GEO, 0.0, sb);
    CHK(global_transformer(E, P, S, F, R));
    if (forked) CHK(coarse_front(E, P, S, F, R));
    roitr_prof_end(ROITR_PROF_PH_GEO, sb);
    if (forked) ROITR_HIP(hipEventRecord(E.ev[Engine::EV_BRANCH_DONE], sb));
    roitr_prof_begin(ROITR_PROF_PH_DEC, 0.0, st);   CHK(decoder(E, P, S, F));                 roitr_prof_end(ROITR_PROF_PH_DEC, st);
    roitr_prof_begin(ROITR_PROF_PH_MATCH, 0.0, st);
    // one stream: the single-stream order of before -- global transformer, decoder, coarse front (inside the matching phase, behind the
    // decoder, so that the main stream meets the wait for the geometry chain's tail as late as it used to)
    if (!forked) CHK(coarse_front(E, P, S, F, R));
    CHK(heads_and_matching(E, io, P, F, R));
    roitr_prof_end(ROITR_PROF_PH_MATCH, st);
    roitr_prof_end(ROITR_PROF_PH_FORWARD, st);
    return 0;
}

// ---------------------------------------------------------------- encode once, match many (include/roitr_encode.h)
// The forward cut where its per-cloud half ends.  Both halves queue the stage functions above; the forward itself is unchanged.
static int cache_scope(const Engine& E, const char* who)
{
    const std::string w(who);
    if (!E.finalized) { roitr_set_error((w + ": engine not finalized").c_str(), __FILE__, __LINE__); return ROITR_ERR_ARG; }
    if (E.cfg.operand_dtype == 1) {
        roitr_set_error((w + ": operand_dtype 1 (bf16 operand storage) is not supported: the cache holds no bf16 E and no bf16 point descriptors").c_str(), __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    if (E.cfg.adaptive_coarse) {
        roitr_set_error((w + ": adaptive_coarse (4DMatch, the compacted patch layout) is not supported").c_str(), __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    return ROITR_OK;
}

// no graph capture: both calls stage descriptors through the pinned ring and may reallocate scratch, which a replay would not repeat
static int refuse_capture(hipStream_t st, const char* who)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return ROITR_OK; }
    if (cs != hipStreamCaptureStatusNone) {
        roitr_set_error((std::string(who) + ": the stream is capturing a graph: not supported").c_str(), __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    return ROITR_OK;
}

// The per-cloud stages exactly as the forward queues them -- the geometry chain (without its ground-truth part) on the geometry stream,
// encoder, geo_in, decoder, fine_proj on `st` -- for NC unpaired clouds, with the node outputs, E, the geo_in rows and the point
// descriptors written into the caller's cache arrays.
static int encode_body(Engine& E, const RoitrEncodeIO* eio, hipStream_t st)
{
    RoitrForwardIO io; memset(&io, 0, sizeof(io));
    io.n_points = eio->n_points; io.points_geom = eio->points_geom; io.normals = eio->normals; io.feats = eio->feats; io.points_out = eio->points_out;
    io.node_xyz = eio->node_xyz; io.node_masks = eio->node_masks; io.node_knn_idx = eio->node_knn_idx; io.node_knn_mask = eio->node_knn_mask;
    Plan P; GeoBufs S; Feats F;
    P.st = st;
    CHK(plan_clouds(E, eio->n_points, eio->clouds, P));
    CHK(reserve_arenas(E, &io, P));
    P.sb = st;   // no branch: the pair half is another call
    S.Emb = eio->embedding;
    CHK(carve_geometry_buffers(E, &io, P, S));
    CHK(stage_descriptors(E, P, S));
    CHK(issue_geometry_chain(E, &io, P, S));
    CHK(encoder(E, &io, P, S, F));
    CHK(geo_in_proj(E, st, P.T4, F.xe[3], eio->node_geo));
    CHK(decoder(E, P, S, F));
    CHK(Gemm(P.T1, F.xd[0], E.fine_proj, eio->point_feats).run(st));
    if (eio->points != S.pts_out) CHK(d2d(st, eio->points, S.pts_out, sizeof(float) * 3 * (size_t)P.T1));
    // the join: E and the chain's tail (node coordinates, partition) were written on the geometry stream
    ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_EMBED_DONE], 0));
    ROITR_HIP(hipStreamWaitEvent(st, E.ev[Engine::EV_TAIL_DONE], 0));
    E.side_forked = false;
    return ROITR_OK;
}

extern "C" int roitr_engine_encode(void* h, const RoitrEncodeIO* eio, hipStream_t st)
{
    Engine& E = *(Engine*)h;
    g_engine = &E;
    CHK(cache_scope(E, "roitr_engine_encode"));
    CHK(refuse_capture(st, "roitr_engine_encode"));
    if (eio->clouds < 1 || !eio->n_points) { roitr_set_error("roitr_engine_encode: needs at least one cloud", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    if (!eio->points_geom || !eio->normals || !eio->feats || !eio->points || !eio->point_feats || !eio->node_xyz || !eio->node_masks ||
        !eio->node_knn_idx || !eio->node_knn_mask || !eio->node_geo || !eio->embedding) {
        roitr_set_error("roitr_engine_encode: an input or a cache array is NULL", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    for (int c = 0; c < eio->clouds; ++c)   // (before anything is reserved or queued)
        if (eio->n_points[c] < 256) { roitr_set_error("roitr_engine_encode: cloud too small: needs >= 256 points (4 nodes)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    E.side_forked = false; E.branch_forked = false; E.cur_par = -1; E.garena_short = false;
    const int rc = join_on_error(E, encode_body(E, eio, st), st);
    E.side_forked = false;
    return rc;
}

// The pair half over cached clouds, on `st` alone: the cached geo_in rows and node masks of the call's 2 B cloud slots gathered into the
// call layout, the global transformer from its first layer on with E read in the cache (per-slot offsets in D.eoff), the coarse front
// with the cached patch gather, the matching tail on the cached point descriptors.
static int match_body(Engine& E, const RoitrCloudTable* tab, const RoitrMatchIO* mio, hipStream_t st)
{
    const int B = mio->pairs, NC = 2 * B;
    std::vector<int> slot_cloud(NC), n_pts(NC);
    for (int b = 0; b < B; ++b) { slot_cloud[b] = mio->src_cloud[b]; slot_cloud[B + b] = mio->tgt_cloud[b]; }
    for (int c = 0; c < NC; ++c) n_pts[c] = tab->seg[slot_cloud[c]].n_points;
    long feat_rows = 0;
    for (int c = 0; c < tab->n_clouds; ++c) {
        const long end = (long)tab->seg[c].pt_row0 + tab->seg[c].n_points;
        feat_rows = end > feat_rows ? end : feat_rows;
    }
    RoitrForwardIO io; memset(&io, 0, sizeof(io));
    io.pairs = B; io.n_points = n_pts.data();
    io.node_xyz = mio->node_xyz; io.node_feats = mio->node_feats;
    io.tgt_corr = mio->tgt_corr; io.src_corr = mio->src_corr; io.corr_scores = mio->corr_scores; io.n_corr = mio->n_corr;
    io.tgt_knn_pts = mio->tgt_knn_pts; io.src_knn_pts = mio->src_knn_pts; io.tgt_knn_masks = mio->tgt_knn_masks; io.src_knn_masks = mio->src_knn_masks;
    io.matching_scores = mio->matching_scores; io.out_tgt_pts = mio->out_tgt_pts; io.out_src_pts = mio->out_src_pts; io.out_scores = mio->out_scores;
    io.out_patch = mio->out_patch; io.fine_offsets = mio->fine_offsets; io.n_out = mio->n_out; io.pair_starts = mio->pair_starts;
    Plan P; GeoBufs S; Feats F; BranchBufs R;
    P.st = st; P.sb = st; P.sd = nullptr; P.cache = tab; P.slot_cloud = slot_cloud.data();
    CHK(plan_clouds(E, n_pts.data(), NC, P));
    for (int c = 0; c < NC; ++c) {
        const RoitrCloudSeg& sg = tab->seg[slot_cloud[c]];
        if (sg.n_nodes != P.V.n[3][c] || sg.pt_row0 < 0 || sg.node_row0 < 0 || sg.emb0 < 0) {
            roitr_set_error("roitr_engine_match: a table entry's node count is not the level-4 size of its point count (or a negative row)", __FILE__, __LINE__);
            return ROITR_ERR_ARG;
        }
        P.eoff[c] = sg.emb0;   // E is read in the cache: the slot's block is the cloud's
    }
    CHK(plan_pairs(E, &io, P));
    const size_t T4 = P.T4, C4 = P.C4, LIM = P.LIM;
    {   // the main arena: what matching_tail takes (the patch term of the forward's bound)
        const size_t need = P.NPs * (LIM * LIM * 3 + (LIM + 1) * (LIM + 1) + LIM * 6) * 4 + ((size_t)64 << 20);
        if (need > E.arena.cap) {
            ROITR_HIP(hipStreamSynchronize(st));
            if (E.side) ROITR_HIP(hipStreamSynchronize(E.side));
            if (E.arena.base) ROITR_HIP(hipFree(E.arena.base));
            E.arena.base = nullptr; E.arena.cap = 0;
            ROITR_HIP(hipMalloc((void**)&E.arena.base, need));
            E.arena.cap = need; E.arena.peak = 0;
            E.arena_epoch++;
        }
        E.arena.off = 0; E.arena.fail = false;
    }
    // the branch arena: what carve_branch takes, the descriptor block and the gathered node arrays of the call layout -- counted, then carved
    // (carve_branch last: it ends with the scratch it only reserves, which ffn_apply takes again from the same offset)
    auto carve = [&](Arena& A, BranchBufs& r, GeoBufs& s) {
        s.desc = A.get<char>(Desc::bytes_with_slots(NC, T4));
        s.node_masks = A.get<int>(T4);
        s.node_xyz = io.node_xyz;   // copied only when the caller asks for it
        carve_branch(&io, P, A, r);
    };
    {
        Arena cnt; cnt.cap = ~(size_t)0;
        BranchBufs r0; GeoBufs s0;
        carve(cnt, r0, s0);
        if (cnt.peak > E.barena.cap) {
            ROITR_HIP(hipStreamSynchronize(st));
            if (E.branch) ROITR_HIP(hipStreamSynchronize(E.branch));
            if (E.barena.base) ROITR_HIP(hipFree(E.barena.base));
            E.barena.base = nullptr; E.barena.cap = 0;
            ROITR_HIP(hipMalloc((void**)&E.barena.base, cnt.peak));
            E.barena.cap = cnt.peak;
            E.arena_epoch++;
        }
        E.barena.off = 0; E.barena.peak = 0; E.barena.fail = false;
    }
    carve(E.barena, R, S);
    if (E.barena.fail) { roitr_set_error("arena exhausted (match)", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    S.Emb = const_cast<float*>(tab->embedding);
    CHK(stage_descriptors(E, P, S));
    E.on_branch = false;
    {
        RoitrCacheGather g; memset(&g, 0, sizeof(g));
        g.slots = NC; g.C = (int)C4; g.n_max = P.V.nmax[3]; g.seg = tab->seg_dev; g.slot_cloud = S.D.slot_cloud; g.node_offset = S.D.off[3];
        g.node_geo = tab->node_geo; g.node_masks = tab->node_masks; g.node_xyz = tab->node_xyz;
        g.out_geo = R.fcur; g.out_masks = S.node_masks; g.out_xyz = S.node_xyz;
        CHK(roitr_cache_gather_nodes(&g, st));
    }
    CHK(global_layers(E, P, S, F, R));
    CHK(coarse_front(E, P, S, F, R));
    return matching_tail(E, &io, P, R, tab->point_feats, (int)feat_rows);
}

extern "C" int roitr_engine_match(void* h, const RoitrCloudTable* tab, const RoitrMatchIO* mio, hipStream_t st)
{
    Engine& E = *(Engine*)h;
    g_engine = &E;
    CHK(cache_scope(E, "roitr_engine_match"));
    CHK(refuse_capture(st, "roitr_engine_match"));
    if (!tab || !tab->seg || !tab->seg_dev || tab->n_clouds < 1 || !tab->points || !tab->point_feats || !tab->node_xyz || !tab->node_masks ||
        !tab->node_knn_idx || !tab->node_knn_mask || !tab->node_geo || !tab->embedding) {
        roitr_set_error("roitr_engine_match: the cloud table is empty or an array of it is NULL", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    if (tab->channels != 256 * E.cfg.factor || tab->limit != E.cfg.point_limit) {
        roitr_set_error("roitr_engine_match: the cache was encoded with other channels / point_limit than this engine's", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    if ((uintptr_t)tab->node_geo & 15) {   // the segment gather moves these rows as float4 (channels is a multiple of 256)
        roitr_set_error("roitr_engine_match: the cache's node_geo array is not 16-byte aligned", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    for (int c = 0; c < tab->n_clouds; ++c) {   // patch rows are int32 rows of the cache's point arrays
        const RoitrCloudSeg& sg = tab->seg[c];
        if (sg.pt_row0 < 0 || sg.n_points < 0 || (long)sg.pt_row0 + sg.n_points > 0x7fffffffL ||
            sg.node_row0 < 0 || sg.n_nodes < 0 || (long)sg.node_row0 + sg.n_nodes > 0x7fffffffL || sg.emb0 < 0) {
            roitr_set_error("roitr_engine_match: a table entry has a negative row, or rows past 2^31", __FILE__, __LINE__);
            return ROITR_ERR_ARG;
        }
    }
    const long max_pairs = (long)(0x7ffffff0u / (size_t)E.cfg.point_limit) / E.cfg.num_corr;   // the forward's bound on patch slots per call
    if (mio->pairs < 1 || mio->pairs > max_pairs || !mio->src_cloud || !mio->tgt_cloud) {
        roitr_set_error("roitr_engine_match: pairs outside the range of one call (1 .. what the forward takes)", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    for (int b = 0; b < mio->pairs; ++b)
        if (mio->src_cloud[b] < 0 || mio->src_cloud[b] >= tab->n_clouds || mio->tgt_cloud[b] < 0 || mio->tgt_cloud[b] >= tab->n_clouds) {
            roitr_set_error("roitr_engine_match: cloud index outside the table", __FILE__, __LINE__);
            return ROITR_ERR_ARG;
        }
    return match_body(E, tab, mio, st);
}

/* The global transformer and the coarse front beside the decoder on the branch stream (2: always; 1, the default: for calls of at least
 * BRANCH_MIN_NODES superpoints) or on the main stream in the single-stream order (0, and small calls in mode 1): the same launches on the same
 * buffers either way, so the results are the same bytes -- which is what modes 0 and 2 are for (tests).  Captured forwards hold the order they
 * were captured with: a change re-captures them. */
/* {main arena capacity, its largest fill since it was allocated, branch arena capacity, its fill in the last call, 1 if the last forward queued its
 * branch on the branch stream} -- diagnostics (tests, the footprint figures of DESIGN.md) */
extern "C" int roitr_engine_scratch_info(void* h, long* out5)
{
    Engine& E = *(Engine*)h;
    out5[0] = (long)E.arena.cap; out5[1] = (long)E.arena.peak; out5[2] = (long)E.barena.cap; out5[3] = (long)E.barena.peak;
    out5[4] = E.on_branch ? 1 : 0;
    return ROITR_OK;
}

extern "C" int roitr_engine_set_ln256_min_rows(void* h, int rows)
{
    Engine& E = *(Engine*)h;
    const int r = rows < 0 ? LN256_MIN_ROWS : rows == 0 ? LN256_NEVER : rows;
    if (E.ln256_min_rows != r) { E.ln256_min_rows = r; E.arena_epoch++; }   // another launch sequence: captured forwards are stale
    return ROITR_OK;
}

extern "C" int roitr_engine_set_phase_overlap(void* h, int on)
{
    Engine& E = *(Engine*)h;
    const int mode = on == 0 ? 0 : on == 2 ? 2 : 1;
    if (E.phase_overlap != mode) { E.phase_overlap = mode; E.arena_epoch++; }
    return ROITR_OK;
}


// ---------------------------------------------------------------- the forward as a HIP graph
// One engine forward is ~800 launches; at one pair per call the device finishes each kernel long before the host has
// issued the next (6.4 ms per forward against ~2 ms of kernel time).  For a repeated (sizes, buffers) combination the
// whole forward -- both streams, the descriptor upload, every memset and kernel -- is captured once and replayed with a
// single hipGraphLaunch.  First call with a key: plain forward (sizes the arena, creates streams / events, runs the
// one-time attribute setup); second call: capture + instantiate; from then on: replay.  A captured graph is tied to the
// addresses of its io buffers (the key) and of the scratch arena (its epoch): a reallocated arena re-captures.
// Profiling events, taps and injects are not capturable -> those calls take the plain path.
// Measured (scripts/bench_graph.py, N = 5000): replay == plain launches to within 1 % at 1, 2, 8 and 32 pairs per call
// (4.75 ms per one-pair forward either way): the forward is bound by the device-side dispatch of ~800 DEPENDENT kernels
// (~6 us each), which a graph does not shorten on this runtime, not by host launch cost.  Kept as an opt-in.
extern "C" int roitr_engine_forward_graph(void* h, const RoitrForwardIO* io, hipStream_t st)
{
    Engine& E = *(Engine*)h;
    if (!E.finalized) { roitr_set_error("engine not finalized", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    if (!st || roitr_prof_is_enabled() || !E.taps.empty() || !E.injects.empty() || io->pairs <= 0) return roitr_engine_forward(h, io, st);
    std::vector<long> key;
    key.push_back(io->pairs);
    long t4 = 0;
    for (int c = 0; c < 2 * io->pairs; ++c) { key.push_back(io->n_points[c]); int s4[4]; roitr_level_sizes(io->n_points[c], s4); t4 += s4[3]; }
    {   // every pointer field of the io block (they follow `n_points` in the struct)
        const void* const* pp = reinterpret_cast<const void* const*>(&io->points_geom);
        const size_t n_ptr = (reinterpret_cast<const char*>(&io->patch_slots) - reinterpret_cast<const char*>(&io->points_geom)) / sizeof(void*);
        for (size_t i = 0; i < n_ptr; ++i) key.push_back((long)(uintptr_t)pp[i]);
        key.push_back(io->patch_slots);
    }
    Engine::GraphEntry* ge = nullptr;
    for (auto& g : E.graphs) if (g.key == key) { ge = &g; break; }
    if (!ge) {
        if (E.graphs.size() >= 16) {   // evict the least recently used entry
            size_t lru = 0;
            for (size_t i = 1; i < E.graphs.size(); ++i) if (E.graphs[i].stamp < E.graphs[lru].stamp) lru = i;
            auto& g = E.graphs[lru];
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            if (g.graph) (void)hipGraphDestroy(g.graph);
            if (g.pin) (void)hipHostFree(g.pin);
            E.graphs.erase(E.graphs.begin() + lru);
        }
        E.graphs.emplace_back();
        ge = &E.graphs.back();
        ge->key = key;
    }
    ge->stamp = ++E.graph_clock;
    if (ge->failed) return roitr_engine_forward(h, io, st);
    if (!ge->warmed || ge->epoch != E.arena_epoch) {
        if (ge->exec) { (void)hipGraphExecDestroy(ge->exec); ge->exec = nullptr; }
        if (ge->graph) { (void)hipGraphDestroy(ge->graph); ge->graph = nullptr; }
        const int rc = roitr_engine_forward(h, io, st);   // warm-up: everything that may not happen inside a capture
        ge->warmed = rc == ROITR_OK;
        ge->epoch = E.arena_epoch;
        return rc;
    }
    if (!ge->exec) {
        const size_t need = Desc::bytes(2 * (size_t)io->pairs, (size_t)t4) + 64;
        if (need > ge->pin_cap) {
            if (ge->pin) (void)hipHostFree(ge->pin);
            ge->pin = nullptr; ge->pin_cap = 0;
            ROITR_HIP(hipHostMalloc((void**)&ge->pin, need, hipHostMallocDefault));
            ge->pin_cap = need;
        }
        E.capture_pin = ge->pin;
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
        int rc = ROITR_OK;
        hipGraph_t g = nullptr;
        if (e == hipSuccess) {
            rc = roitr_engine_forward(h, io, st);
            e = hipStreamEndCapture(st, &g);
        }
        E.capture_pin = nullptr;
        if (e == hipSuccess && rc == ROITR_OK && g) e = hipGraphInstantiate(&ge->exec, g, nullptr, nullptr, 0);
        if (e != hipSuccess || rc != ROITR_OK || !g || !ge->exec) {
            (void)hipGetLastError();
            if (g) (void)hipGraphDestroy(g);
            ge->exec = nullptr; ge->failed = true;   // this key stays on the plain path
            return roitr_engine_forward(h, io, st);
        }
        ge->graph = g;
    }
    ROITR_HIP(hipGraphLaunch(ge->exec, st));
    return ROITR_OK;
}

/* number of forwards currently held as instantiated graphs (tests / diagnostics) */
extern "C" int roitr_engine_graph_count(void* h)
{
    Engine& E = *(Engine*)h;
    int n = 0;
    for (auto& g : E.graphs) n += g.exec ? 1 : 0;
    return n;
}
