/*
 * roitr_engine.h -- C ABI of libroitr_hip.so, part 2: the fused stage operators of the RoITr
 * inference path and the whole-pair engine (boundary B2 of SURVEY.md 8(b), restated as C entry
 * points so a host in any language can drive the path; the roitr_amd Python package is one).
 *
 * Conventions: device pointers to contiguous fp32 / int32; caller owns all memory; every call is
 * asynchronous on `stream` and returns 0 or an error code (text via roitr_last_error()).
 * Citations are into /root/reference.
 */
#ifndef ROITR_ENGINE_H
#define ROITR_ENGINE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef ROITR_POINTOPS_H
typedef struct ihipStream_t* roitr_stream_t;
#endif

/* ------------------------------------------------------------------ dense layers (nn.Linear) */
/* C[b] = act(alpha * (A[b] (+A2[b])) @ W[b]^T + bias[b]);  A (M,K) lda, W (N,K) ldw, C (M,N) ldc.
 * a_idx / w_idx: optional int32 row gathers; an index < 0 or >= *_limit (when *_limit > 0) reads
 * a zero row (the reference's zero-padded patch rows, model/RIGA_v2.py:129-142). */
typedef struct RoitrGemm {
    int M, N, K;
    const float* A; const float* A2; int lda; const int* a_idx; int a_limit;
    const float* W; int ldw; const int* w_idx; int w_limit;
    const float* bias; float alpha; int relu;
    float* C; int ldc;
    int batch; long sA, sW, sC, sBias, sAidx, sWidx;
    /* optional ragged batching: batch b multiplies row segment (seg_a0 + b) of A with row segment (seg_w0 + b) of W,
     * segments given by the cumulative int32 `seg_off`; M / N then only bound the grid. */
    const int* seg_off; int seg_a0, seg_w0;
    /* optional fused LayerNorm epilogue (ln_gamma != NULL; requires N == 64 = one tile per row, batch == 1):
     *   C[r,:] = [relu]( LayerNorm(acc[r,:] + bias + ln_res[ln_res_idx ? ln_res_idx[r] : r, :]) * gamma + beta + ln_post[r,:] )
     * i.e. the GEMM followed by roitr_add_layernorm in one launch (ln_res / ln_post rows are 64 floats, dense). */
    const float* ln_gamma; const float* ln_beta; const float* ln_res; const int* ln_res_idx; const float* ln_post;
    int ln_relu; float ln_eps;
    /* bf16 operand mode (0 = the fp32 kernel above): a mask of ROITR_BF16_*.  The products run on the bf16 matrix cores with
     * fp32 accumulation; W MUST be stored bf16 (ROITR_BF16_W: `W` then points to uint16 data, ldw / sW in elements), A is
     * fp32 and rounded while it is staged unless ROITR_BF16_A says it is stored bf16 (`A` -> uint16, A2 unsupported), C is
     * written bf16 (uint16, ldc / sC in elements) with ROITR_BF16_C.  bias / ln_* stay fp32.  Needs K % 64 == 0 and
     * 16-byte aligned rows (roitr_gemm_bf16_supported). */
    int bf16;
    /* optional K-concatenated A operand (fp32 kernel only): columns k >= k_cat of the product come from A_cat (same row
     * index / gather as A, leading dimension lda_cat), i.e. C = [A | A_cat] @ W^T with W (N, K), K = k_cat + width(A_cat);
     * k_cat % 32 == 0.  Lets `linear(att) + in_proj(x)` of a local transformer run as ONE GEMM. */
    const float* A_cat; int lda_cat; int k_cat;
    /* optional, fused LayerNorm epilogue of the fp32 kernel only: the three-nearest-neighbour interpolation of TransitionUp
     * (pointops.py:168-182 behind model/model.py:112-116) added AFTER the activation,
     *   C[r,:] += sum_k w_k ip_feat[ip_idx[3 r + k], :],   w_k = (1 / (sqrt(ip_dist2[3 r + k]) + 1e-8)) / sum of the three,
     * ip_feat rows N floats, dense: `linear1(x1) + interpolation(...)` in the launch that computes linear1. */
    const float* ip_feat; const int* ip_idx; const float* ip_dist2;
    /* optional with A_cat: its own row gather (A_cat row of output row r = a_cat_idx[r]; A keeps a_idx / the identity) -- the
     * `linear(att) + in_proj(x[node_idx])` of a TransitionDown transformer as one GEMM (model/model.py:59-62 samples the rows).
     * With A_cat an addend A2 applies to the A part only (columns k < k_cat). */
    const int* a_cat_idx;
    /* optional (ABI 3): device int; batches (tiles of batch index) >= *batch_live leave at once -- a batch list whose live length is
     * only known on the device (the compacted patch list of the adaptive matching, RIGA_v2.py:126-152) without a host round trip. */
    const int* batch_live;
    /* ROITR_BF16_X3 (ABI 3; alone in `bf16`): fp32 arithmetic on the bf16 matrix cores by a three-way operand split (csrc/gemm_x3.hip).
     * `W` points to THREE bf16 images of the fp32 weight (roitr_split_bf16x3): piece p of element (n, k) at W[p * w_piece + n * ldw + k]
     * (uint16, ldw / w_piece in elements); A (A2, A_cat) stay fp32 and are split while they are staged; C fp32.  Six bf16 products per
     * multiply (error ~ one fp32 rounding per product; rows bitwise independent of the row count).  Needs K % 32 == 0, batch == 1. */
    long w_piece;
} RoitrGemm;
#define ROITR_BF16_W 1
#define ROITR_BF16_A 2
#define ROITR_BF16_C 4
#define ROITR_BF16_X3 8
int roitr_gemm(const RoitrGemm* g, roitr_stream_t stream);
/* The kernel form roitr_gemm gives this struct (the rule roitr_gemm itself dispatches through; host code, no pointer is followed, no
 * device is needed), or, for a struct roitr_gemm refuses, MINUS the status it returns (-ROITR_ERR_ARG, -ROITR_ERR_UNSUPPORTED).
 * "Fast path": K % 32 == 0, K <= 2048, lda / ldw % 4 == 0, 16-byte aligned A, A2 and W with sA / sW % 4 == 0; "tiles": 64 x 64 tiles
 * of C times batch.  The results of SMALL, TILE and TILE_IL are the same bytes; so are those of the LayerNorm forms of one width. */
#define ROITR_GEMM_NOTHING 0        /* M, N or batch <= 0: returns ROITR_OK, launches nothing */
#define ROITR_GEMM_SMALL 1          /* fast path, no LayerNorm, tiles < 512: 32 x 32 tiles of 16x16x4 MFMAs */
#define ROITR_GEMM_TILE 2           /* fast path, no LayerNorm, 512 <= tiles < 1024: 64 x 64 tiles, staging loads in one burst */
#define ROITR_GEMM_TILE_IL 3        /* fast path, no LayerNorm, tiles >= 1024: 64 x 64 tiles, staging loads between the MFMAs */
#define ROITR_GEMM_GENERIC 4        /* off the fast path: 64 x 64 tiles with bounds-checked scalar tails */
#define ROITR_GEMM_LN_GENERIC 5     /* LayerNorm epilogue off the fast path (N == 64 only) */
#define ROITR_GEMM_LN_TILE64 6      /* LayerNorm epilogue, fast path, N == 64: 64 x 64 tiles */
#define ROITR_GEMM_LN_TILE128 7     /* LayerNorm epilogue, fast path, N == 128: 64 x 128 tiles */
#define ROITR_GEMM_LN_TILE256 8     /* LayerNorm epilogue, fast path, N == 256, what LN256 declines (row gathers): 64 x 256 tiles */
#define ROITR_GEMM_LN256 9          /* LayerNorm epilogue, fast path, N == 256, dense rows: 32 x 256 tiles (csrc/gemm_ln256.hip) */
#define ROITR_GEMM_BF16 10          /* RoitrGemm::bf16 with ROITR_BF16_W (csrc/gemm_bf16.hip) */
#define ROITR_GEMM_X3 11            /* RoitrGemm::bf16 == ROITR_BF16_X3 (csrc/gemm_x3.hip) */
int roitr_gemm_form(const RoitrGemm* g);
int roitr_gemm_bf16_supported(const RoitrGemm* g);
/* Diagnostics: block-tile rows of the fp32 LayerNorm launches with N == 256 -- 32 (csrc/gemm_ln256.hip, the default) or 64 (the
 * 64 x 256 instantiation of the general kernel).  Process-wide; the results are the same bytes. */
int roitr_gemm_set_ln256_tile(int rows);
/* fp32 -> bf16 (round to nearest even), n elements; dst 4-byte aligned */
int roitr_f32_to_bf16(long n, const float* src, unsigned short* dst, roitr_stream_t stream);
/* shapes / layouts the split kernel takes (RoitrGemm::bf16 == ROITR_BF16_X3) */
int roitr_gemm_x3_supported(const RoitrGemm* g);
/* src (n fp32) -> its three bf16 pieces at dst, dst + piece, dst + 2 * piece (piece >= n, even): src[i] == h[i] + m[i] + l[i] exactly */
int roitr_split_bf16x3(long n, const float* src, unsigned short* dst, long piece, roitr_stream_t stream);

/* ------------------------------------------------------------------ row-wise layers */
/* out = act( LayerNorm(x + res[res_idx]) * gamma + beta (+ post_add) ); res, res_idx, post_add optional.
 * attention.py:319, model/model.py:138-140 (bn2, += identity, relu), geoattention.py:50,161,241. */
int roitr_add_layernorm(int M, int C, const float* x, const float* res, const int* res_idx, const float* gamma,
                        const float* beta, const float* post_add, int relu, float eps, float* out, roitr_stream_t stream);
/* the same followed by the three-nearest-neighbour interpolation of TransitionUp, added after the activation (see RoitrGemm::ip_*):
 * out[r,:] = act( LayerNorm(x[r,:] + res) * gamma + beta ) + sum_k w_k ip_feat[ip_idx[3 r + k], :] */
int roitr_add_layernorm_interp(int M, int C, const float* x, const float* res, const int* res_idx, const float* gamma,
                               const float* beta, int relu, float eps, const float* ip_feat, const int* ip_idx, const float* ip_dist2,
                               float* out, roitr_stream_t stream);
/* F.normalize(p=2, dim=1), model/RIGA_v2.py:64-65 */
int roitr_l2_normalize(int M, int C, const float* x, float* out, roitr_stream_t stream);
int roitr_transpose(int rows, int cols, const float* in, int ld_in, float* out, int ld_out, roitr_stream_t stream);
/* out = a + b over n floats (bias of a folded layer) */
int roitr_add_vectors(int n, const float* a, const float* b, float* out, roitr_stream_t stream);
/* out = base + 3-NN inverse-distance interpolation of feat (functions/pointops.py:168-182 + model/model.py:116);
 * dist2 = SQUARED distances as produced by the kNN call. */
int roitr_interp3_add(int n, int C, const float* feat, const int* idx, const float* dist2, const float* base, float* out,
                      roitr_stream_t stream);
/* per-cloud feature mean (model/model.py:101-109); offset (b) cumulative cloud ends, no cloud empty; compensated fp32 sum over the rows */
int roitr_segment_mean(int b, int C, const float* x, const int* offset, float* out, roitr_stream_t stream);
/* SinusoidalPositionalEmbedding (positional_encoding.py:38-62): out (rows, C) */
int roitr_sinusoid(long rows, int C, const float* vals, const float* div_term, float* out, roitr_stream_t stream);
/* Fused positional_encoding.py:139-154: out[r,:] = proj_d(sinusoid(d_idx[r])) + max_k proj_a(sinusoid(a_idx[r,k])) */
int roitr_geo_embed(long rows, int C, int angle_k, const float* d_idx, const float* a_idx, const float* div_term,
                    const float* Wd, const float* bd, const float* Wa, const float* ba, float* out, roitr_stream_t stream);
/* OPT-IN: the same embedding on the bf16 matrix cores with three-way split operands (x = hi + mid + lo, six partial
 * products kept: error of the order of fp32 rounding).  W*3: 3 * C * C uint16 made by roitr_split3_bf16. */
int roitr_split3_bf16(long n, const float* src, unsigned short* dst, roitr_stream_t stream);
int roitr_geo_embed_split(long rows, int C, int angle_k, const float* d_idx, const float* a_idx, const float* div_term,
                          const unsigned short* Wd3, const float* bd, const unsigned short* Wa3, const float* ba, float* out,
                          roitr_stream_t stream);
/* bf16 operand form (engine operand_dtype = 1): Wd / Wa = the (C, C) weights stored bf16, sinusoid rounded to bf16, fp32 accumulate */
int roitr_geo_embed_bf16(long rows, int C, int angle_k, const float* d_idx, const float* a_idx, const float* div_term,
                         const unsigned short* Wd, const float* bd, const unsigned short* Wa, const float* ba, float* out,
                         roitr_stream_t stream);
/* the same with the embedding itself STORED in bf16 (out: rows x C uint16) -- half the bytes of the tensor every self
 * layer of the global transformer streams (read back by roitr_mha with e_bf16 = 1) */
int roitr_geo_embed_bf16_out(long rows, int C, int angle_k, const float* d_idx, const float* a_idx, const float* div_term,
                             const unsigned short* Wd, const float* bd, const unsigned short* Wa, const float* ba,
                             unsigned short* out, roitr_stream_t stream);
/* Function-table form of the same embedding (csrc/geo_table.hip): proj_x(sinusoid(v)) is a univariate band-limited function of
 * the scalar v per output channel (positional_encoding.py:38-62 feeds ONE value per row into the sinusoid), so it is fitted once
 * per weight set by a degree-7 polynomial per channel on intervals of width `interval` (float64 Chebyshev interpolation on the
 * HOST) and evaluated from LDS.  roitr_geo_table_build: all pointers are HOST memory; table holds roitr_geo_table_floats()
 * floats; fit[0..5] = {max |poly - g_d| over a dense probe (64 points per interval), max |g_d|, the same for the angle projection,
 * the largest per-channel relative error of the distance / of the angle projection}.
 * roitr_geo_embed_table: device pointers; values outside [0, n_int * interval) are evaluated directly from div_term / W / b, so
 * any input is served; angle_k must be 3, C a multiple of 64; out is fp32 (rows, C), or bf16 when out_bf16. */
size_t roitr_geo_table_floats(int C, int n_int_d, int n_int_a);
int roitr_geo_table_build(int C, const float* div_term, const float* Wd, const float* bd, const float* Wa, const float* ba,
                          float interval, int n_int_d, int n_int_a, float* table, double* fit);
int roitr_geo_embed_table(long rows, int C, int angle_k, const float* d_idx, const float* a_idx, const float* table, float interval,
                          int n_int_d, int n_int_a, const float* div_term, const float* Wd, const float* bd, const float* Wa,
                          const float* ba, void* out, int out_bf16, roitr_stream_t stream);
/* E = P_d + max_k P_a[:, k, :] (positional_encoding.py:146-152) */
int roitr_geo_combine(long rows, int C, int k, const float* pd, const float* pa, float* out, roitr_stream_t stream);
int roitr_gather_rows(long rows, int C, const float* in, const int* idx, int limit, float* out, roitr_stream_t stream);
int roitr_compose_idx(int n, const int* outer, const int* inner, int* out, roitr_stream_t stream);
/* lib/utils.py:358-389 with the gather fused: out (m,k,4) */
int roitr_calc_ppf(int m, int k, const float* centre_xyz, const float* centre_normals, const float* ref_xyz,
                   const float* ref_normals, const int* group_idx, float* out, roitr_stream_t stream);

/* ------------------------------------------------------------------ local PPF attention */
/* attention.py:152-200 with the positional branch folded (see csrc/local_attn.hip).
 * q: (M, >= H + 5*heads) rows = [q | per head: Wpe_h^T q_h (4), q_h.bpe_h (1)] (or (M, >= H) rows with wpe / bpe given); k, v: rows of the input
 * cloud (ld given); group_idx (M,K) int32; ppf (M,K,4); wvpe (H,4), bvpe (H); out (M,H).
 * scale = 1/sqrt(H/heads). */
typedef struct RoitrLocalAttn {
    int M, K, H, heads;
    const float* q; int ldq;
    const float* k; int ldk;
    const float* v; int ldv;
    const int* group_idx; const float* ppf;
    const float* wvpe; const float* bvpe;
    float scale;
    float* out; int ldo;
    const void* node_order;   /* optional float4[M] (x,y,z,index-as-bits): visiting order, e.g. roitr_knn_sorted_points() */
    int bf16;                 /* 0: fp32 rows; 3: q / k / v rows AND the output row are stored in bf16 (uint16; ld* in elements) --
                                 the engine's bf16 operand mode, where the q|k|v tensor is written bf16 by its GEMM */
    const float* wpe; const float* bpe;   /* optional (both or none): Wpe (H,4) and bpe (H) of the folded positional branch; the
                                 kernel then forms qp[h] = [Wpe_h^T q_h, q_h . bpe_h] itself and q rows are only H wide */
} RoitrLocalAttn;
int roitr_local_attention(const RoitrLocalAttn* a, roitr_stream_t stream);
int roitr_build_pfold(int H, int heads, const float* wpe, const float* bpe, float* pfold, roitr_stream_t stream);

/* TransitionDown form of the local PPF attention with the key / value projections folded into the query side
 * (csrc/local_attn.hip local_attn_fold_kernel; attention.py:152-200 behind ppftransformer.py:227-253).  M query nodes, 16 neighbours
 * each among the rows of x (N_in, in_dim):
 *     score(h, j) = scale * ( qt[node][h] . x_j + (Wpe_h^T q_h) . ppf_j )       (terms constant over j are dropped: softmax)
 *     xbar[node][h] = sum_j a_hj x_j            (M, 4, in_dim)  -> the caller applies Wv'_h and bv'_h (one batched GEMM)
 *     vpart[node]   = Wvpe_h pbar_h + bvpe_h    (M, H)          -> the positional value term; attention output = vpart + Wv' xbar + bv'
 * with qt[node][h] = Wk'_h^T q_h (M, 4, in_dim) supplied by the caller.  fp32, 4 heads, K = 16,
 * (in_dim, H) in {(64, 128), (128, 256), (256, 256)}; everything 16-byte aligned. */
typedef struct RoitrLocalAttnFold {
    int M, in_dim, H;
    const float* x; int ldx;
    const float* q; int ldq;      /* (M, H) query rows (for the PPF coefficients) */
    const float* qt;              /* (M, 4 * in_dim) */
    const int* group_idx; const float* ppf;   /* (M, 16), (M, 16, 4) */
    const float* wpe;             /* (H, 4) */
    const float* wvpe; const float* bvpe;     /* (H, 4), (H) */
    float scale;
    float* xbar;                  /* (M, 4 * in_dim) */
    float* vpart;                 /* (M, H) */
    const void* node_order;       /* optional float4[M]: visiting order */
    int ldqt;                     /* row stride of qt in floats; 0 = dense (4 * in_dim).  Lets q and q~ be the two column blocks of ONE
                                   * GEMM's output (engine, round 5: q~_h = (Wk'_h^T Wq'_h) x + Wk'_h^T bq_h straight from the input row) */
} RoitrLocalAttnFold;
int roitr_local_attention_fold(const RoitrLocalAttnFold* a, roitr_stream_t stream);
int roitr_local_attention_fold_supported(int in_dim, int H, int K);

/* The block form of the local PPF transformer in ONE launch (csrc/local_block.hip), for the 64- / 128-wide levels:
 *   out = relu( bn2( out_proj( LN( linear(att) + in_proj(x) ) ) ) + x )     model/model.py:131-142, ppftransformer.py:227-253
 * with att = local PPF attention of q = x Wq^T + bq over the neighbours' k | v rows.  The caller supplies kv (M, 2H) = the k | v
 * projections of EVERY point (one plain GEMM) and the folded weights: wq / bq = proj_q o in_proj, wcat (H, 2H) = [W_linear | W_in],
 * bcat = b_linear + b_in, wpe / bpe / wvpe / bvpe = the folded positional branch (see RoitrLocalAttn).  fp32, heads = 4,
 * H in {64, 128}, K in {8, 16}; everything 16-byte aligned. */
typedef struct RoitrLocalBlock {
    int M, K, H;
    const float* x; const float* kv; const int* group_idx; const float* ppf;
    const void* node_order;   /* optional float4[M] (x,y,z,index-as-bits): visiting order */
    const float* wq; const float* bq;
    const float* wpe; const float* bpe; const float* wvpe; const float* bvpe;
    const float* wcat; const float* bcat; const float* norm_w; const float* norm_b;
    const float* wout; const float* bout; const float* bn2_w; const float* bn2_b;
    float scale, eps;
    float* out;
    int kv_bf16;   /* ABI 3: 1 = the k | v rows are STORED in bf16 (`kv` -> uint16, 2 H elements per row); everything else stays fp32 */
    /* ABI 4 (optional, all three or none, with kv_bf16 = 1): bf16 copies of wq (H x H), wcat (H x 2H), wout (H x H).  Given: the three
     * on-chip GEMMs take bf16 matrix operands (v_mfma_f32_32x32x16_bf16, fp32 accumulate; the activations are rounded on their way into
     * the operand registers, like the A operand of a ROITR_BF16_W GEMM) -- the fused block of the engine's bf16 operand mode */
    const unsigned short* wq_h; const unsigned short* wcat_h; const unsigned short* wout_h;
} RoitrLocalBlock;
int roitr_local_block(const RoitrLocalBlock* a, roitr_stream_t stream);
int roitr_local_block_supported(int H, int K);

/* The TransitionDown transformer of the 64 -> 128 wide level in ONE launch (csrc/local_block.hip local_td_kernel, round 5):
 *   out = out_proj( LN( linear(att) + in_proj(x_n) ) ),  x_n = x[node_idx[node]],                      ppftransformer.py:227-253
 * att = the folded-attention form of RoitrLocalAttnFold (scores from q~_h = Wk'_h^T q_h against the 16 gathered INPUT rows, value
 * = Wv'_h (sum_j a_hj x_j) + bv'_h + the positional value term).  A workgroup keeps a tile of 32 nodes on chip from x_n to out: q | q~
 * (one on-chip GEMM with the folded weight wqqt), the attention, the per-head value projection, the K-concatenated linear with its
 * LayerNorm, out_proj.  fp32, 4 heads, in_dim = 64, H = 128, K = 16; weights as the engine folds them (csrc/engine.cpp fold_local):
 * wqqt ((H + 4 in_dim), in_dim) / bqqt, wv (H, in_dim) / bv = the folded value projection, wcat (H, H + in_dim) = [W_linear | W_in] /
 * bcat, wpe / wvpe (H, 4) / bvpe the folded positional branch.  Everything 16-byte aligned. */
typedef struct RoitrLocalTd {
    int M, in_dim, H;
    const float* x; const int* node_idx;      /* (N_in, in_dim) input rows; (M) row of x of every node */
    const int* group_idx; const float* ppf;   /* (M, 16) rows of x, (M, 16, 4) */
    const void* node_order;                   /* optional float4[M]: visiting order */
    const float* wqqt; const float* bqqt;
    const float* wv; const float* bv;
    const float* wpe; const float* wvpe; const float* bvpe;
    const float* wcat; const float* bcat; const float* norm_w; const float* norm_b;
    const float* wout; const float* bout;
    float scale, eps;
    float* out;                               /* (M, H) */
} RoitrLocalTd;
int roitr_local_td(const RoitrLocalTd* a, roitr_stream_t stream);
int roitr_local_td_supported(int in_dim, int H, int K);

/* The first local transformer of the network (in_planes = 1, model/model.py:152): its q | k | v are rank-1 affine in the scalar
 * input feature, so the whole TransitionDown transformer collapses to per-node scalars + two small on-chip GEMMs
 * (csrc/local_block.hip local_first_kernel).  x (M,) the scalar feature; H = 64.  Constants (built from the layer's weights, see
 * csrc/engine.cpp build_local_first): head_consts (4 heads x 16 floats: c1 c2 c3 c4 | P1[4] | P0[4] | d1 d0 | 0 0),
 * G (64, 32) = the affine map of g = [S(4) | pbar(16) | x | 1 | 0...] to linear(att) + in_proj(x), zero_bias (64 zeros). */
typedef struct RoitrLocalFirst {
    int M, K;
    const float* x; const int* group_idx; const float* ppf; const void* node_order;
    const float* head_consts; const float* G; const float* zero_bias;
    const float* norm_w; const float* norm_b; const float* wout; const float* bout;
    float scale, eps;
    float* out;
} RoitrLocalFirst;
int roitr_local_first(const RoitrLocalFirst* a, roitr_stream_t stream);

/* The form the engine runs one local transformer in (csrc/engine.cpp; the table in DESIGN.md): decided once, at finalize, from the
 * layer's shapes (in_dim -> H -> out_dim), its neighbour count K, its role (transition_down != 0: the transformer of a TransitionDown,
 * rows sampled by node_idx; 0: of a block, with the bn2 residual) and the engine's operand_dtype, through the *_supported predicates
 * above.  Pure host code: no engine, no device.  fp32 (0) and the three-way split (2) choose alike. */
#define ROITR_LOCAL_FIRST 0        /* roitr_local_first */
#define ROITR_LOCAL_FUSED_BLOCK 1  /* k | v GEMM + roitr_local_block */
#define ROITR_LOCAL_FUSED_TD 2     /* roitr_local_td */
#define ROITR_LOCAL_TD_FOLD 3      /* roitr_local_attention_fold between its GEMMs */
#define ROITR_LOCAL_SEQUENCE 4     /* one launch per step around roitr_local_attention */
int roitr_local_form(int in_dim, int H, int out_dim, int K, int transition_down, int operand_dtype);

/* Fragment-ordered copies of the fp32 weights that the on-chip GEMMs of the three launches above read (csrc/local_block.hip
 * gemm_phase).  Weights stay the same from call to call in real use, so the copy is made once: for every 32-row region and every
 * 32-k slab of W one 4 KB block of four groups of 64 float4 in the order a wave consumes them, (c, n) = (0,0), (0,1), (1,0), (1,1);
 * entry 16 g + i of a group holds W[32 region + 16 n + i][32 slab + 16 c + 4 g .. + 3].  A wave's fragment load is then one
 * contiguous 1 KB read instead of 64 bytes of each of 16 rows.
 *   prepare: makes (or, for a view prepared before, rewrites) the device copy of the (rows, k) view at W with leading dimension ldw,
 *            on `stream`, and records it in a library-internal table under (W, rows, k, ldw).  rows and k multiples of 32, ldw >= k.
 *   release: frees every copy recorded under W (none: a no-op).  Call it before W is freed or its contents change for good; after a
 *            change in place, prepare again.
 * A launch takes the fragment path when ALL of its weights are in the table, under exactly these views, and the row-major path
 * otherwise -- the same bits either way:
 *   roitr_local_block (fp32 form): (wq, H, H, H), (wcat, H, 2H, 2H), (wout, H, H, H)
 *   roitr_local_td:    (wqqt, H + 4 in_dim, in_dim, in_dim), (wv, H, in_dim, in_dim), (wcat, H, H + in_dim, H + in_dim), (wout, H, H, H)
 *   roitr_local_first: (wout, 64, 64, 64)
 * count: the number of copies the table holds.
 * reorder_host: the same permutation over host buffers (dst: rows * k floats). */
int roitr_local_weights_prepare(const float* W, int rows, int k, int ldw, roitr_stream_t stream);
int roitr_local_weights_release(const float* W);
int roitr_local_weights_count(void);
int roitr_local_weights_reorder_host(const float* src, int rows, int k, int ldw, float* dst);

/* ------------------------------------------------------------------ global geometric transformer */
/* positional_encoding.py:110-137 get_embedding_indices for a batch of clouds.  pts (rows,3) = all nodes,
 * offset (b) cumulative, cloud_of_row (rows), eoff (b) = element offset of cloud c's (n_c, n_c) block.
 * d_idx: concatenated (n_c, n_c); a_idx: concatenated (n_c, n_c, angle_k). */
int roitr_geo_indices(int rows, const float* pts, const int* offset, const int* cloud_of_row, const long* eoff,
                      float sigma_d, float sigma_a, int angle_k, int n_max, float* d_idx, float* a_idx, roitr_stream_t stream);

/* Multi-head attention, query rows [q_row0, q_row0 + q_rows) of the concatenated node array.
 * Keys/values of query row r are the rows of cloud partner[cloud_of_row[r]] (partner == NULL: own cloud).
 * Without E: geoattention.py:26-66 (cross attention; q/k already hold the +pos inputs).
 * With E (n_c,n_c,C per cloud at eoff): geoattention.py:87-136 with the RPE branch folded --
 *   qt (rows, heads, C) = Wp_h^T q_h,  bp (C) = proj_p.bias,  ebar (rows, heads, C) = sum_j a'_ij E_ij
 *   where a' is the diagonal-masked softmax; the caller finishes pos_states = Wvp_h ebar_h + bvp_h. */
typedef struct RoitrMha {
    int q_row0, q_rows, C, heads;
    const float* q; int ldq;
    const float* k; int ldk;
    const float* v; int ldv;
    const int* offset; const int* cloud_of_row; const int* partner;
    const float* E; const long* eoff; const float* qt; const float* bp;
    float scale; int nk_max;
    float* out; int ldo;
    float* ebar;
    int e_bf16;   /* E is stored in bf16 (uint16, same element offsets): engine operand_dtype = bf16; needs C = 256 or 512, 4 heads */
} RoitrMha;
/* Launches ONE kernel form (below) for the struct, or refuses it with ROITR_ERR_UNSUPPORTED and a message that names the limit:
 * heads outside 1..8, C % heads, (C / heads) % 4, ldk % 4, bf16 E outside C = 256 / 512 with 4 heads and nk_max <= 512, and for the
 * generic kernel a heads x nk_max score table over its 150 KB of LDS. */
int roitr_mha(const RoitrMha* a, roitr_stream_t stream);
/* The kernel form roitr_mha gives this struct (the rule roitr_mha itself dispatches through; host arithmetic on the fields, E and
 * partner only tested for NULL, no device is needed), or, for a struct roitr_mha refuses, MINUS the status it returns.
 * "Quad layout": 4 heads, ldq % 4 == 0 (and ldk % 4 == 0, which every form needs).  "Self with E": E != NULL, partner == NULL.
 * The forms with a key bound are tried in this order: GEO_WIDE2*, GEO_WIDE_H, (bf16 refusal), PLAIN_WIDE2, GEO*, PLAIN*. */
#define ROITR_MHA_NOTHING 0         /* q_rows <= 0: returns ROITR_OK, launches nothing */
#define ROITR_MHA_GEO20 1           /* self with E, quad layout, C = 256, fp32 E, nk_max <= 80: E rows in registers, 20 per wave */
#define ROITR_MHA_GEO32 2           /* the same, 80 < nk_max <= 128: 32 rows per wave */
#define ROITR_MHA_GEO_STREAM 3      /* the same, 128 < nk_max <= 1024: E streamed twice */
#define ROITR_MHA_GEO_WIDE_H 4      /* self with E, quad layout, C = 256, bf16 E, nk_max <= 512: E streamed twice */
#define ROITR_MHA_GEO_WIDE2 5       /* self with E, quad layout, C = 512, fp32 E, nk_max <= 512: E streamed twice */
#define ROITR_MHA_GEO_WIDE2_H 6     /* the same with bf16 E */
#define ROITR_MHA_PLAIN128 7        /* no E, quad layout, C = 256, nk_max <= 128: four query rows per block */
#define ROITR_MHA_PLAIN1024 8       /* the same, 128 < nk_max <= 1024 */
#define ROITR_MHA_PLAIN_WIDE2 9     /* no E, quad layout, C = 512, nk_max <= 512: one query row per block */
#define ROITR_MHA_GENERIC 10        /* everything else (other widths or head counts, ldq % 4 != 0, partner with E, more keys): one key row per lane */
int roitr_mha_form(const RoitrMha* a);

/* ------------------------------------------------------------------ coarse-to-fine matching tail */
/* Cloud layout for every batched call below: [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}], B = pairs. */

/* lib/utils.py:428-471.  p2n (n_points) node index local to the cloud; knn_idx (n_nodes, limit) point index
 * local to the cloud, padded with the cloud's point count; masks are int32 0/1. */
int roitr_point_to_node_partition(int b, int n_points, int n_nodes, const float* pts, const int* pt_offset,
                                  const float* nodes, const int* node_offset, const int* cloud_of_node, int limit,
                                  int* p2n, float* p2n_dist, int* node_masks, int* knn_idx, int* knn_mask, roitr_stream_t stream);

/* model/modules.py:141-178 CoarseMatching (ref = tgt, src = src as called at RIGA_v2.py:121).
 * feats (n_nodes, C) L2-normalised; outputs (pairs, num_corr): node indices local to their cloud (-1 beyond
 * n_corr[pair]), scores.  scratch: pairs * scratch_stride floats, stride >= roitr_coarse_scratch_floats().
 * xy: optional precomputed feature dot products, pair b at xy + b*xy_stride, row-major (n_tgt, ld = xy_ld). */
typedef struct RoitrCoarse {
    int pairs, C, num_corr, dual_norm, max_ref, max_src;
    const float* feats; const int* node_offset; const int* node_masks;
    float* scratch; long scratch_stride;
    int* tgt_corr; int* src_corr; float* corr_scores; int* n_corr;
    const float* xy; long xy_stride; int xy_ld;
    int lds_cap;   /* filled in by the launcher (LDS keys per sort chunk); callers leave it 0 */
} RoitrCoarse;
size_t roitr_coarse_scratch_floats(int n_ref, int n_src);
int roitr_coarse_matching(const RoitrCoarse* a, roitr_stream_t stream);
/* model/modules.py:75-124 AdaptiveSuperPointMatching (4DMatch); needs a->xy; a->num_corr = output capacity per pair */
int roitr_adaptive_matching(const RoitrCoarse* a, int min_num, float threshold, roitr_stream_t stream);

/* Patch layouts of the four operators below (ABI 3).  STRIDED (pair_off == NULL): per-patch arrays have pairs * num_corr slots,
 * patch p of pair b at slot b * num_corr + p, live while p < n_corr[b] (dead slots are zero-filled / skipped).  COMPACTED
 * (pair_off != NULL, pairs + 1 cumulative int32 from roitr_patch_offsets): the live patches of all pairs back to back in `slots`
 * slots, pair b owns [pair_off[b], pair_off[b + 1]); slots past pair_off[pairs] are never read or written.  That is how the
 * reference runs the tail -- on the SELECTED node pairs only (model/RIGA_v2.py:126-152, modules.py:102-111): the adaptive 4DMatch
 * matching selects between 128 and n_t * n_s = 15 625 pairs per cloud pair, typically ~1 000.  The coarse lists tgt_corr /
 * src_corr / corr_scores stay (pairs, num_corr) in both layouts. */
/* pair_off[0] = 0, pair_off[b + 1] = min(slots, n_corr[0] + .. + n_corr[b]); the caller detects a cut from n_corr */
int roitr_patch_offsets(int pairs, const int* n_corr, int slots, int* pair_off, roitr_stream_t stream);

/* model/RIGA_v2.py:125-147: per patch correspondence the `limit` point rows / points / masks of both sides.
 * rows index the concatenated point arrays (-1 = the zero pad row). */
typedef struct RoitrPatch {
    int pairs, num_corr, limit;
    const int* n_corr; const int* tgt_corr; const int* src_corr;
    const int* node_offset; const int* pt_offset; const int* knn_idx; const int* knn_mask; const float* points;
    int* tgt_rows; int* src_rows; int* tgt_masks; int* src_masks; float* tgt_pts; float* src_pts;
    const int* pair_off; int slots;   /* compacted layout (see above); NULL / 0 = strided */
} RoitrPatch;
int roitr_patch_gather(const RoitrPatch* a, roitr_stream_t stream);

/* model/modules.py:10-72 LearnableLogOptimalTransport: scores (patches, limit, limit) -> out (patches, limit+1, limit+1) */
typedef struct RoitrOT {
    int pairs, num_corr, limit, num_iter;
    const int* n_corr; const float* scores; const int* row_masks; const int* col_masks; const float* alpha;
    float* out;
    const int* pair_off; int slots;   /* compacted layout; NULL / 0 = strided */
} RoitrOT;
int roitr_optimal_transport(const RoitrOT* a, roitr_stream_t stream);
/* Diagnostics of the data-dependent work of that stage (synchronous): reads out[0] = live patches, out[1] = Sinkhorn iterations skipped by
 * the exact fixed-point exit, out[2] = patches served by the log-domain kernel, all since the last enable; then enable = 1 (re)starts
 * counting from zero, 0 stops it, -1 leaves it.  out may be NULL. */
int roitr_ot_stats(int enable, unsigned long long* out);

/* model/modules.py:216-324 FineMatching (use_dustbin = False).  ot = the OT output; rows = tgt, cols = src.
 * Emits correspondences in (patch, row, col) order; offsets[patch] = first output slot of the patch. */
typedef struct RoitrFine {
    int pairs, num_corr, limit, k, mutual;
    float conf;
    const int* n_corr; const float* ot; const int* row_masks; const int* col_masks;
    const float* row_pts; const float* col_pts; const float* global_scores;
    unsigned char* flags; int* counts; int* offsets; int* n_out;
    float* out_row_pts; float* out_col_pts; float* out_scores; int* out_patch;
    long out_cap;   /* rows the out_* arrays hold (0 = caller guarantees pairs*num_corr*limit*limit): the emitter never writes past
                       it and *n_out is clamped to it.  Worst case per patch: limit*k rows when mutual, 2*limit*k otherwise
                       (row top-k OR column top-k, modules.py:259-266). */
    const int* pair_off; int slots;   /* compacted layout; NULL / 0 = strided.  out_patch then holds slot numbers */
    int* pair_starts;                 /* optional (pairs + 1): first output row of every pair, then the total */
} RoitrFine;
int roitr_fine_matching(const RoitrFine* a, roitr_stream_t stream);
/* roitr_optimal_transport(o) followed by roitr_fine_matching(f), bit for bit, with the flag stage done by the transport kernels (the
 * transport output is not read back, one launch less; the selection is the one roitr_fine_matching runs, for every k).  o and f must describe the same patch list (pairs, num_corr, limit, n_corr,
 * row / column masks, pair_off, slots) and f->ot must be o->out: ROITR_ERR_ARG otherwise. */
int roitr_matching_tail(const RoitrOT* o, const RoitrFine* f, roitr_stream_t stream);

/* ------------------------------------------------------------------ ground-truth side outputs (need rot/trans) */
/* Padded clouds for lib/utils.py:506-510: out_pts has n_points + 2*pairs rows -- every cloud followed by its pad row
 * (the zero row of RIGA_v2.py:86-87), source clouds (and their pad rows) transformed by rot/trans;
 * out_offset (3*pairs): cumulative padded sizes of the 2*pairs clouds, then the pairs target offsets relative to
 * the first target row. */
int roitr_build_padded_clouds(int pairs, int n_points, const float* pts, const int* pt_offset, const float* rot,
                              const float* trans, float* out_pts, int* out_offset, roitr_stream_t stream);
/* lib/utils.py:511-527.  d2_padded: squared distance of every padded point to its nearest neighbour in the
 * partner cloud (kNN(1) over the padded clouds). */
int roitr_node_occlusion_score(int n_nodes, int limit, const int* cloud_of_node, const int* pt_offset, const int* knn_idx,
                               const int* knn_mask, const int* node_masks, const float* d2_padded, float overlap_thres,
                               float* out, roitr_stream_t stream);
/* lib/utils.py:530-614 (ref = tgt, src = src).  overlap: scratch (pairs, mat_stride >= max_nodes^2);
 * out_idx (pairs, mat_stride, 2) [ref, src] local node indices in torch.nonzero order, out_overlap, out_count (pairs).
 * During the call out_idx / out_count[0] also carry the work list of node pairs that survive the enclosing-sphere prune (they are
 * rewritten by the final compaction); pairs * max_nodes^2 must stay below 2^31. */
typedef struct RoitrNodeCorr {
    int pairs, limit, max_nodes;
    float pos_radius;
    const float* nodes; const int* node_offset; const int* node_masks;
    const float* points; const int* pt_offset; const int* knn_idx; const int* knn_mask;
    const float* rot; const float* trans;
    float* overlap; long mat_stride;
    int* out_idx; float* out_overlap; int* out_count;
    int n_nodes; float* nodes_t; float* radius;   /* scratch: (n_nodes,3) and (n_nodes) */
} RoitrNodeCorr;
int roitr_node_correspondences(const RoitrNodeCorr* a, roitr_stream_t stream);

/* ------------------------------------------------------------------ the whole-pair engine */
/* One engine = one set of weights + its workspace on the current device.  Drives the complete test-mode
 * forward of model/RIGA_v2.py:58-175 for a batch of B independent pairs with HIP kernels only.
 *
 * Parameters are registered by their reference state_dict key (e.g.
 * "backbone.enc2.0.transformer.transformer.attention.proj_p.weight", lib/trainer.py:94-130 layout) as
 * device pointers that must stay valid while the engine lives. */
typedef struct RoitrEngineConfig {
    int factor;            /* 1 = 3DMatch, 2 = 4DMatch (model/RIGA_v2.py:24,28) */
    int num_corr;          /* num_est_coarse_corr */
    int point_limit;       /* point_per_patch (64) */
    int fine_topk, fine_mutual, fine_use_global_score;
    float fine_conf;       /* fine_matching_confidence_threshold */
    int n_geo_layers;      /* len(transformer_architecture) */
    int geo_is_cross[16];  /* 0 = 'self', 1 = 'cross' */
    float matching_radius; /* coarse_matching.matching_radius (GT helpers) */
    int adaptive_coarse;   /* 1 = AdaptiveSuperPointMatching (4DMatch): num_corr is then its min_num_correspondences and
                              the per-pair patch capacity becomes n_tgt_nodes_max * n_src_nodes_max */
    float occlusion_radius;/* lib/utils.py:485 overlap_thres */
    int operand_dtype;     /* 0 = fp32 everywhere (the reference's arithmetic); 1 = bf16 operand storage for the dense layers
                              (BASELINE config 4): weights stored bf16 once at finalize, activations rounded to bf16 as MFMA
                              operands, GEMM-to-GEMM intermediates, the q|k|v tensors, the attention outputs and the geometric
                              embedding E stored bf16, the patch score contraction (RIGA_v2.py:150) on a bf16 copy of the point
                              descriptors; fp32 accumulation / bias / LayerNorm / softmax everywhere; FPS, kNN, PPF, partition,
                              coarse scores, optimal transport and fine matching stay fp32;
                              2 = fp32 everywhere like 0, but the plain linear layers with K >= 256 (levels 3 - 4, the global transformer,
                              the decoder's coarse half) multiply on the bf16 matrix cores by the three-way operand split of
                              csrc/gemm_x3.hip: fp32-accurate products (error against float64 not above the fp32 MFMA kernel's), rows
                              bitwise independent of the batch; results differ from mode 0 in the last bits only (round 6) */
} RoitrEngineConfig;

typedef struct RoitrForwardIO {
    int pairs;                 /* B */
    const int* n_points;       /* host array, 2B entries: src_0..src_{B-1}, tgt_0..tgt_{B-1} */
    /* inputs, device, clouds concatenated in that order */
    const float* points_geom;  /* (T,3): src_raw_pcd / tgt_pcd (model/RIGA_v2.py:62) */
    const float* normals;      /* (T,3) */
    const float* feats;        /* (T,1) */
    const float* points_out;   /* (T,3): src_pcd / tgt_pcd; NULL = points_geom */
    const float* rot;          /* (B,3,3) or NULL: skips the ground-truth side outputs */
    const float* trans;        /* (B,3) */
    /* outputs, device, caller-allocated; any may be NULL.  T4 = total nodes, P = num_corr, L = point_limit.  The per-patch outputs
     * -- *_knn_pts, *_knn_masks, matching_scores, fine_offsets -- have B * P slots, patch p of pair b at slot b * P + p, EXCEPT with
     * adaptive_coarse (4DMatch): there P = nmax4^2 only bounds the coarse lists tgt_corr / src_corr / corr_scores, and the per-patch
     * outputs hold the SELECTED patches of all pairs back to back in `patch_slots` slots (pair b at patch_offsets[b] ..
     * patch_offsets[b + 1]); see patch_slots below. */
    float* node_xyz;           /* (T4,3) */
    float* node_feats;         /* (T4, 256f) */
    float* point_feats;        /* (T, 256f) */
    int* node_masks;           /* (T4) */
    int* node_knn_idx;         /* (T4, L) local point indices, pad = cloud size */
    int* node_knn_mask;        /* (T4, L) */
    int* tgt_corr; int* src_corr; float* corr_scores; int* n_corr;   /* (B,P) x3, (B) */
    float* tgt_knn_pts; float* src_knn_pts;    /* (B,P,L,3) */
    int* tgt_knn_masks; int* src_knn_masks;    /* (B,P,L) */
    float* matching_scores;    /* (B,P,L+1,L+1) */
    float* out_tgt_pts; float* out_src_pts; float* out_scores; int* out_patch;  /* capacity B*P*L*fine_topk rows (x2 when fine_mutual == 0) */
    int* fine_offsets;         /* (B*P) first output row of every patch */
    int* n_out;                /* (1) total correspondences */
    float* gt_node_occ;        /* (T4) node occlusion scores, src clouds then tgt clouds; needs rot/trans */
    int* gt_corr_idx;          /* (B, nmax4^2, 2) [tgt node, src node]; needs rot/trans */
    float* gt_corr_overlaps;   /* (B, nmax4^2) */
    int* gt_corr_count;        /* (B) */
    /* Optional hipEvent_t.  NULL: the inputs above are ordered on `stream` (whatever produced them was queued there before the call).
     * Non-NULL: the inputs are complete once this event has fired and `stream` carries no dependency on them -- the engine then
     * stages the descriptors and runs the first sampling level (the longest serial chain of a small-batch forward) on its geometry
     * stream as soon as the event fires, BESIDE the previous forward still occupying `stream`, instead of behind it (calls of up to 128
     * pairs: the whole geometry chain, in scratch the engine alternates between calls); everything that touches the engine's shared
     * scratch -- and every kernel that writes one of the OUTPUT buffers above -- still starts where this forward begins on `stream`:
     * output buffers may be reused from call to call, nothing but `stream` order is required of the caller.  Results are identical.
     * Ignored by roitr_engine_forward_graph. */
    void* inputs_ready;
    /* ABI 3.  patch_slots: with adaptive_coarse, the number of patch slots the per-patch outputs above (and the engine's own patch
     * scratch) hold for the WHOLE call; 0 = the bound B * nmax4^2.  Patches beyond it are cut from the END of the call's list: the
     * true counts are in n_corr, the kept ones in patch_offsets -- a caller that sees sum(n_corr) > patch_slots repeats the call with
     * that sum (roitr_amd/riga.py does).  Ignored without adaptive_coarse (the slots are exactly B * num_corr there).
     * patch_offsets (B + 1): first patch slot of every pair, then the live total.  pair_starts (B + 1): first row of every pair in
     * out_scores / out_*_pts, then the total (== *n_out).  Both optional. */
    int* patch_offsets;
    int* pair_starts;
    int patch_slots;
} RoitrForwardIO;

void* roitr_engine_create(const RoitrEngineConfig* cfg);
void roitr_engine_destroy(void* engine);
int roitr_engine_set_param(void* engine, const char* name, const float* device_ptr, long numel);
int roitr_engine_finalize(void* engine, roitr_stream_t stream);
/* The function table of the geometric embedding chosen by finalize (see roitr_geo_table_build): info[0..8] = {interval, n_int_d,
 * n_int_a, fit error d, amplitude d, fit error a, amplitude a, largest per-channel relative error d, a}; returns 1 when a table is
 * in use, 0 when the GEMM form is.  finalize accepts the widest interval of {2, 1, 0.5} whose per-channel relative errors are both
 * below 2^-25, the GEMM form (geo_embed_kernel) otherwise. */
int roitr_engine_geo_table_info(void* engine, double* info);
int roitr_engine_forward(void* engine, const RoitrForwardIO* io, roitr_stream_t stream);
/* Same forward, replayed as ONE hipGraphLaunch once the same (sizes, io buffers) combination has been seen twice
 * (1st call: plain forward; 2nd: capture + instantiate; then replay).  `stream` must be a real (non-NULL) stream.
 * The caller keeps the io buffers at fixed addresses and re-fills them between calls. */
int roitr_engine_forward_graph(void* engine, const RoitrForwardIO* io, roitr_stream_t stream);
int roitr_engine_graph_count(void* engine);
/* Behind the encoder the global transformer and the coarse front of the matching phase (coarse head, coarse matching, patch arrays)
 * depend on nothing the decoder writes, and the decoder on nothing of theirs.  on == 1 (the default): for calls with enough superpoints
 * for it to pay they run on a stream of the engine's own beside the decoder, joined in front of the patch score product; smaller calls
 * keep them on the caller's stream.  on == 2: on the engine's stream for every call.  on == 0: never -- the same launches, on the same
 * buffers, queued on the caller's stream in front of the decoder.  The results are the same bytes in every mode. */
int roitr_engine_set_phase_overlap(void* engine, int on);
/* The 256-wide fp32 Linear + LayerNorm layers (levels 3 - 4, global transformer, dec4 / dec3) run as ONE launch (csrc/gemm_ln256.hip) from
 * `rows` rows per launch on, as GEMM + roitr_add_layernorm below.  rows == 0: never; rows < 0: the built-in default.  The two forms give
 * the same bytes; fp32 operand mode only (the bf16 and split modes keep their launches). */
int roitr_engine_set_ln256_min_rows(void* engine, int rows);
/* Diagnostics: out5 = {capacity of the main scratch arena in bytes, its largest fill since it was allocated, capacity of the branch arena,
 * its fill in the last call, 1 if the last forward queued its branch on the engine's own stream (0: on the caller's)}. */
int roitr_engine_scratch_info(void* engine, long* out5);
/* Test taps: after stage `name` its output tensor is copied to `device_ptr` (NULL removes the tap);
 * inject: the stage output is REPLACED by the tensor at device_ptr before the forward continues. */
int roitr_engine_set_tap(void* engine, const char* name, void* device_ptr);
int roitr_engine_set_inject(void* engine, const char* name, const void* device_ptr);
/* level sizes the engine will use for a cloud of n points: out[0..3] (model/model.py:59-62 floor rule) */
void roitr_level_sizes(int n, int* out4);


/* ------------------------------------------------------------------ evaluators, batched over pairs
 * lib/loss.py:195-206 Evaluator.evaluate_fine == registration/benchmark_utils.py:69-77: pair b owns correspondences
 * [starts[b], starts[b+1]) of src_pts / tgt_pts; inliers[b] = #{ ||rot_b s + trans_b - t|| < radius }. */
int roitr_inlier_counts(int pairs, const int* starts, const float* src_pts, const float* tgt_pts, const float* rot,
                        const float* trans, float radius, int* inliers, roitr_stream_t stream);
/* lib/loss.py:170-193 Evaluator.evaluate_coarse: hits[b] = #{ i < n_corr[b] : (tgt_corr[b,i], src_corr[b,i]) is one of
 * the gt_count[b] ground-truth node pairs gt_idx[b,:,(tgt,src)] whose overlap exceeds acceptance_overlap }. */
int roitr_coarse_hits(int pairs, int num_corr, const int* n_corr, const int* tgt_corr, const int* src_corr, int gt_cap,
                      const int* gt_idx, const float* gt_overlaps, const int* gt_count, float acceptance_overlap, int* hits,
                      roitr_stream_t stream);


/* ------------------------------------------------------------------ registration, batched over pairs
 * registration/evaluate_registration_c2f.py:78-85 + registration/benchmark_utils.py:169-215 (Open3D correspondence RANSAC) and
 * lib/utils.py:159-212 (weighted_procrustes).  Pair b owns rows [starts[b], starts[b+1]) of src_pts / tgt_pts / scores
 * (fp32 (N,3), (N,3), (N); scores may be NULL = all 1), the layout RoitrForwardIO::pair_starts / out_*_pts / out_scores has.
 * total_rows >= starts[pairs] (rows past it are never read).
 *
 * Random stream (registration_math.h): splitmix64 s(x); hypothesis draw d of iteration i of the pair with key k:
 *   u = hi32(s(seed ^ s(k << 32 | i << 4 | d))), index = (u * n) >> 32; draws 0..15 in order, an index already taken is skipped,
 *   the first three distinct ones are the triple (none after draw 15: the iteration is invalid).
 * Selection (sample_mode): 0 all rows; 1 the n_points largest scores (ties: lower index); 2 n_points rows without replacement with
 *   probability proportional to the score (Efraimidis-Spirakis: the n_points largest log(v_j) / w_j, ties: lower index,
 *   v_j = (hi32(s(seed ^ 0xA0761D6478BD642F ^ s(k << 32 | j))) + 0.5) / 2^32, j the row's index in the pair).  Rows with a score
 *   <= 0 (or not finite) are never drawn in mode 2; with fewer than n_points of them all are taken (numpy's choice would raise).
 * Hypothesis of iteration i: the triple; edge checker: reject if |s_i - s_j| < sim |t_i - t_j| or |t_i - t_j| < sim |s_i - s_j|;
 *   degenerate triangles rejected (|a x b|^2 <= 1e-12 |a|^2 |b|^2 in source or target); float64 Kabsch (proper rotation);
 *   distance checker: every sample with ||R s + t - g||^2 <= thr^2 (fp32).  Valid hypotheses are scored over all selected rows:
 *   inliers = #{ ||R s + t - g||^2 < thr^2 } (fp32), ties broken by the smaller sum of inlier d^2, then the lower iteration.
 * refine_iters rounds of Procrustes on the current inlier set (unweighted, or weighted by the score with refine_weighted).
 * Outputs per pair: transforms (B,4,4) row-major, inliers (count under the final transform), best_iteration (-1: none),
 * valid_hypotheses (passed both checkers), n_used (selected rows), selected (optional, int32 (total_rows)): the selected rows'
 * local indices at [starts[b], starts[b] + n_used[b]) in increasing order.  No valid hypothesis (or fewer than 3 rows): identity,
 * inliers 0, valid_hypotheses 0.
 * chunks: hypothesis workgroups per pair (0: automatic); results do not depend on it.  The workspace (device, caller-owned) holds at
 * least roitr_registration_workspace_bytes(pairs, total_rows, iterations, chunks) bytes.
 * Refusals: ransac_n != 3 -> ROITR_ERR_UNSUPPORTED; iterations outside [1, 2^28], thresholds not finite and positive,
 * edge_similarity outside (0, 1], null pointers, a short workspace -> ROITR_ERR_ARG. */
size_t roitr_registration_workspace_bytes(int pairs, int total_rows, int iterations, int chunks);
int roitr_ransac_correspondences(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                                 const float* scores, const unsigned int* pair_keys, int sample_mode, int n_points, int ransac_n,
                                 float distance_threshold, float edge_similarity, int iterations, int refine_iters, int refine_weighted,
                                 unsigned long long seed, int chunks, void* workspace, size_t workspace_bytes, float* transforms,
                                 int* inliers, int* best_iteration, int* valid_hypotheses, int* n_used, int* selected,
                                 roitr_stream_t stream);
/* The triples of iterations [it0, it0 + count) for each pair (n[b] rows, key pair_keys[b]): out (pairs, count, 3) int32, -1 for an
 * invalid iteration or n[b] < 3.  Device pointers; the stream above bit for bit. */
int roitr_ransac_samples(int pairs, const int* n, const unsigned int* pair_keys, unsigned long long seed, int it0, int count, int* out,
                         roitr_stream_t stream);
/* lib/utils.py:159-212 weighted_procrustes on dense (batch, n, 3) src / tgt and (batch, n) weights (NULL = all 1): weights below
 * weight_thresh count 0, centroids sum(w p) / (sum w + eps), H = sum w (s - cs)(t - ct)^T, the rotation with the sign(det) fix,
 * t = ct - R cs; transforms (batch, 4, 4). */
int roitr_weighted_procrustes(int batch, int n, const float* src_pts, const float* tgt_pts, const float* weights, float weight_thresh,
                              float eps, float* transforms, roitr_stream_t stream);


/* ------------------------------------------------------------------ RANSAC-free registration
 * GeoTransformer's local-to-global registration (LGR) on the patches of the coarse-to-fine matcher: one pose hypothesis per patch,
 * verification over all correspondences, iterative reweighted refits.  No random stream.  Pair b owns rows [starts[b], starts[b+1])
 * of src_pts / tgt_pts (fp32 (N,3)), scores (fp32 (N); NULL = all 1) and row_patch (int32 (N)), the layout
 * RoitrForwardIO::pair_starts / out_src_pts / out_tgt_pts / out_scores / out_patch has in the strided and in the compacted patch
 * layout alike: only equality of neighbouring row_patch entries is read.  total_rows >= starts[pairs]; starts are clamped into
 * [0, total_rows] before anything is read through them.
 * Parameters: radius (acceptance radius, finite, > 0), min_rows (rows a patch needs to form a hypothesis, >= 3: GeoTransformer's
 *   correspondence_threshold), steps (number of global solves, >= 1: GeoTransformer's num_refinement_steps, 5 there).
 * Runs: row r of pair b starts a run when r == starts[b] or row_patch[r] != row_patch[r-1].  A run of at least min_rows rows is a
 *   hypothesis; hypotheses are numbered in row order.
 * Solve(rows, w): roitr_weighted_procrustes with weight_thresh 0 and eps 1e-5: centroids cs, ct = sum w p / (sum w + eps),
 *   H = sum w (s - cs)(t - ct)^T, all sums in float64 on the fp32 inputs, the rotation from rg_solve_rigid (registration_math.h),
 *   T rounded to fp32.  Residual: rg_dist2 (fp32, fixed FMA order); a row is an inlier when d^2 < radius^2, strictly.
 * Local stage: T_h = Solve(the rows of run h, their scores).  Verification: count_h = the rows of the pair that are inliers under
 *   T_h; the winner has the largest count, ties go to the lower hypothesis number.
 * Global stage: w0 = score x [inlier under T_winner], T1 = Solve(all rows, w0); for k = 1 .. steps - 1: wk = score x [inlier under
 *   Tk], T(k+1) = Solve(all rows, wk).  A pair without a hypothesis starts from T0 = Solve(all rows, score) instead of T_winner
 *   (GeoTransformer's degenerate branch) and goes on in the same way.  A solve whose weights sum to 0 keeps the previous transform,
 *   sets ROITR_LGR_EMPTY_REFIT and ends the loop.
 * Outputs per pair: transforms (B,4,4) row-major; inliers (count under the final transform); best_hypothesis (-1: none);
 *   best_first_row (first row of the winning run, local to the pair; -1: none); hypotheses (their number); local_inliers
 *   (count_winner; the count under T0 in the degenerate branch); status (bits below; a pair without rows: identity, NO_ROWS alone).
 * Optional outputs (NULL allowed), each of capacity total_rows / min_rows hypotheses: hyp_first_row, hyp_transforms (12 floats
 *   each: [R | t] row-major 3x4) and hyp_counts; hyp_starts (pairs + 1): pair b's hypotheses are entries [hyp_starts[b],
 *   hyp_starts[b] + hypotheses[b]) with hyp_starts[b] = starts[b] / min_rows (a pair of n rows has at most n / min_rows hypotheses,
 *   so the ranges of different pairs never meet and are found without a scan over the pairs; entries between them are not written).
 * Determinism: a pair's results are bitwise independent of the batch it travels in, of where its rows sit in the arrays, of the
 *   absolute values in row_patch and of a repeat of the call: every float64 sum is a strided per-lane sum over the row index local
 *   to the run (16 lanes) or to the pair (256 lanes) followed by a fixed butterfly; the only atomics add integer counts.
 * The workspace (device, caller-owned) holds at least roitr_lgr_workspace_bytes(pairs, total_rows) bytes (host-only, monotone).
 * Refusals (ROITR_ERR_ARG, nothing is launched or written): null pointers, a radius not finite and positive, min_rows < 3,
 *   steps < 1, total_rows < 0, more than 65535 pairs, a short workspace. */
#define ROITR_LGR_NO_ROWS 1
#define ROITR_LGR_NO_LOCAL 2
#define ROITR_LGR_EMPTY_REFIT 4
size_t roitr_lgr_workspace_bytes(int pairs, int total_rows);
int roitr_lgr_batch(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts, const float* scores,
                    const int* row_patch, float radius, int min_rows, int steps, void* workspace, size_t workspace_bytes,
                    float* transforms, int* inliers, int* best_hypothesis, int* best_first_row, int* hypotheses, int* local_inliers,
                    int* status, int* hyp_starts, int* hyp_first_row, float* hyp_transforms, int* hyp_counts, roitr_stream_t stream);


/* ------------------------------------------------------------------ spatial-compatibility registration
 * Pose hypotheses from the second-order spatial compatibility of the correspondences themselves, the idea of SC2-PCR (Chen et al.,
 * CVPR 2022), for sets without patch structure: no random stream, no row_patch.  PARITY WITH SC2-PCR IS NOT CLAIMED: the operator is
 * defined here.  Simplifications against the paper: seeds by degree instead of a leading eigenvector plus non-maximum suppression;
 * one consensus stage instead of two; hard (0 / 1) compatibility only.
 * Inputs as roitr_lgr_batch without row_patch: pair b owns rows [starts[b], starts[b+1]) (clamped into [0, total_rows]) of src_pts /
 * tgt_pts (fp32 (N,3)) and scores (fp32 (N); NULL = all 1).  Inputs must be finite; they are not checked.
 * Parameters: compat_dist (finite, > 0), radius (finite, > 0), max_rows (3 ... 8192), max_seeds (1 ... 1024), k (consensus size,
 *   3 ... 64), steps (>= 1).
 * 1. Selection.  A pair of n rows has m = min(n, max_rows) selected rows.  n <= max_rows: all rows in row order.  Otherwise: the
 *   max_rows rows of largest (score, -row) -- the key is float_image(score) of csrc/common.h, a lower row wins among equal scores;
 *   with NULL scores the first max_rows rows -- listed in ascending row order, and status bit TRUNCATED is set.  Selected row
 *   a in [0, m) is row sel[a] of the pair; p_a, q_a are its source and target point.
 * 2. Graph.  For a != b: d_ab = | rg_len(p_a, p_b) - rg_len(q_a, q_b) |, rg_len in float64 on the fp32 inputs (registration_math.h);
 *   C_ab = d_ab < (double)compat_dist, strictly; C_aa = 0; deg_a = sum_b C_ab.
 * 3. Seeds.  S = min(max_seeds, m) seeds: the S selected rows of largest (deg, -a).  A seed's rank is its position in that order.
 * 4. Consensus set of seed s.  c_b = C_sb * sum_x C_sx C_bx (the common compatible neighbours).  Members: the seed plus the at most
 *   k - 1 indices b with c_b > 0 of largest (c_b, -b).  Fewer than 3 members: the hypothesis is invalid, its count is -1.  Weights:
 *   w_b = (float)c_b and w_s = (float)max_b c_b, integers <= 8190; scores take no part.  T_rank = Solve(members in ascending a, w),
 *   the Solve of roitr_lgr_batch above: float64 moments, eps 1e-5, rg_solve_rigid, T rounded to fp32.
 * 5. Verification and global stage: those of roitr_lgr_batch, over ALL n rows of the pair (not only the selected ones).  Residual
 *   rg_dist2, inlier when d^2 < radius^2 strictly; the winner is the valid hypothesis with the largest count, ties go to the lower
 *   rank; then `steps` reweighted solves with score x [inlier].  A pair without a valid hypothesis starts from Solve(all rows, score)
 *   and sets NO_HYPOTHESIS; a solve whose weights sum to 0 keeps the transform, sets EMPTY_REFIT and ends the loop; a pair without
 *   rows gets the identity and NO_ROWS alone.
 * Outputs per pair: transforms (B,4,4); inliers; best_rank (-1: none); best_seed_row (row local to the pair, -1: none); seeds (S);
 *   hypotheses (the valid ones); local_inliers (the winner's count; the count under the first solve without a hypothesis); status.
 * Optional outputs (NULL allowed): degree (total_rows) int32, deg of the selected rows of every pair and -1 for its unselected rows
 *   (rows outside every pair are not written); seed_rows (pairs x max_seeds) local rows in rank order, -1 padded; seed_members
 *   (pairs x max_seeds x k) local rows ascending, -1 padded (an invalid hypothesis lists the one or two rows it has); hyp_transforms (pairs x
 *   max_seeds x 12), zeros for an invalid hypothesis and for ranks >= S; hyp_counts (pairs x max_seeds), -1 for those.
 * Slots: pair b's begin at b x max_seeds; there is no scan over the pairs and no host read.
 * Determinism: as roitr_lgr_batch.  Every decision of stages 1 - 4 is an integer or an exact float64 comparison, every float64 sum
 *   runs in an order fixed by the pair's own local indices, the only atomics add integers: a pair's results are bitwise independent
 *   of its batch, its slot, its row offset, of max_rows / max_seeds capacity that changes no decision, and of repeats.
 * The workspace (device, caller-owned) holds at least roitr_compat_workspace_bytes() bytes (host-only, monotone; 0 for arguments the
 *   batch call refuses).  It holds C bit-packed: pairs x max_rows x ceil(max_rows / 64) 64-bit words.
 * Refusals (ROITR_ERR_ARG, nothing is launched or written): null pointers, parameters out of the ranges above, total_rows < 0,
 *   more than 65535 pairs, a short workspace. */
#define ROITR_COMPAT_NO_ROWS 1
#define ROITR_COMPAT_NO_HYPOTHESIS 2
#define ROITR_COMPAT_EMPTY_REFIT 4
#define ROITR_COMPAT_TRUNCATED 8
size_t roitr_compat_workspace_bytes(int pairs, int total_rows, int max_rows, int max_seeds, int k);
int roitr_compat_batch(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts, const float* scores,
                       float compat_dist, float radius, int max_rows, int max_seeds, int k, int steps, void* workspace,
                       size_t workspace_bytes, float* transforms, int* inliers, int* best_rank, int* best_seed_row, int* seeds,
                       int* hypotheses, int* local_inliers, int* status, int* degree, int* seed_rows, int* seed_members,
                       float* hyp_transforms, int* hyp_counts, roitr_stream_t stream);


/* ------------------------------------------------------------------ fast global registration
 * A pose from ONE robust objective over all correspondences of a pair, no hypotheses: the Geman-McClure cost of Fast Global
 * Registration (Zhou, Park and Koltun, ECCV 2016; Open3D's FastGlobalRegistration), minimised by Gauss-Newton steps on a 6-vector
 * while the scale mu is lowered (graduated non-convexity).  PARITY WITH OPEN3D IS NOT CLAIMED: the operator is defined here.  Open3D
 * normalises both clouds by a global scale, draws its tuples from rand() and compares `par` with the unsquared distance; this
 * operator works in metres, draws from the project's counter-based stream and compares squared with squared.
 * Inputs as roitr_compat_batch: pair b owns rows [starts[b], starts[b+1]) (clamped into [0, total_rows]) of src_pts / tgt_pts (fp32
 * (N,3)) and scores (fp32 (N); NULL = all 1); pair_keys (uint32 per pair) and seed feed the triple stream and are read only when
 * tuples > 0 (pair_keys may be NULL otherwise).  Inputs must be finite; they are not checked.
 * Parameters: max_dist (the final scale in metres, finite, > 0), division_factor (double, > 1, finite; Open3D: 1.4), iterations
 *   (1 ... 1024 Gauss-Newton steps), mu_every (>= 1 iterations between two decreases of mu; Open3D: 4), tuples (0 ... 2^28 triples
 *   DRAWN per pair, 0: no tuple test; the bound is the stream's iteration field), tuple_scale (float in (0, 1); Open3D: 0.95), radius
 *   (finite, > 0; only for the reported inlier count).
 * Per pair of n rows, p_c / q_c the source / target point of local row c:
 * 1. Multiplicity.  m_c = 1 for every row when tuples == 0 or n < 3.  Otherwise, for it in [0, tuples): the triple is what
 *   roitr_ransac_samples reports for (n, pair_keys[b], seed, it); an invalid iteration is skipped.  It is accepted when each of its
 *   three edges (a, b), with ls = rg_len(p_a, p_b), lt = rg_len(q_a, q_b) (float64 on the fp32 inputs, registration_math.h) and
 *   s = (double)tuple_scale, has ls * s < lt && lt * s < ls, strictly.  An accepted triple adds 1 to m of each of its rows (Open3D
 *   appends an accepted tuple's correspondences with repeats).  No triple accepted: every m_c = 1 and status NO_TUPLES.
 * 2. Weights.  w_c = (double)score_c * m_c.  Rows with w_c > 0 are USED.  Fewer than 3 used rows: the identity, status TOO_FEW, no
 *   loop (mu and objective 0).  No rows at all: the identity and NO_ROWS alone.
 * 3. Centring and start scale, float64.  cs, ct = the plain means of the used rows' source and target points; p~ = p - cs,
 *   q~ = q - ct; D2 = the largest of |p~|^2, |q~|^2 over the used rows; md2 = (double)max_dist^2; mu_0 = max(D2, md2).  The state
 *   (R, t), float64, starts at (I, 0) in the centred frame: at the translation that aligns the centroids.
 * 4. Iteration k = 0 ... iterations - 1 over the used rows: y = R p~ + t, r = y - q~, e = r . r, l = mu / (e + mu), omega = w l^2,
 *   J = [-[y]x | I] (3 x 6, rotation part first); A = sum omega J^T J, g = sum omega J^T r, objective_k = sum w mu e / (e + mu),
 *   sum_omega_k = sum omega; x = ldl_solve6(A, -g) (csrc/gauss_newton6.h).  A non-positive or non-finite pivot sets SINGULAR, keeps the
 *   state and ends the loop.  Otherwise (R, t) <- dT(x) (R, t) in float64, dT = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5] (compose_step_d,
 *   Open3D's TransformVector6dToMatrix4d), and then, if (k + 1) % mu_every == 0 and mu > md2: mu = max(mu / division_factor, md2).
 *   Every product and sum is rounded on its own (no contraction).
 * 5. Outputs per pair: transforms (B,4,4) fp32 = [R | ct + t - R cs], rounded once at the end; inliers: rows of the WHOLE pair with
 *   rg_dist2 < radius^2 (fp32, strictly) under that fp32 transform, as roitr_lgr_batch verifies; n_used; tuples_accepted; steps (the
 *   updates applied); mu and objective (double: the last scale, the objective of the last evaluated iteration); status (bits below).
 *   Optional (NULL allowed): multiplicity (total_rows) int32, m_c as it was used (1 under the fallback; rows outside every pair are
 *   not written); trace (pairs x iterations x 16) double, row k = the 12 values of the centred state [R | t] (rows of 4) BEFORE step
 *   k, mu_k, objective_k, sum_omega_k, 1.0; rows that were not run are zero.
 * 6. Determinism: as roitr_compat_batch.  Every float64 sum is a strided per-lane sum over the pair's local row index (256 lanes)
 *   followed by a fixed butterfly; the maximum D2 does not depend on an order; the only atomics add integers.  A pair's results are
 *   bitwise independent of its batch, its slot, its row offset and of repeats, and depend on pair_keys[b] and seed only through the
 *   triples.
 * Two kernel launches and two memsets for a whole batch, whatever `iterations` is; no host read.
 * The workspace (device, caller-owned) holds at least roitr_fgr_workspace_bytes() bytes (host-only, monotone; 0 for arguments the
 *   batch call refuses).
 * Refusals (ROITR_ERR_ARG, nothing is launched or written): null pointers, pair_keys NULL with tuples > 0, parameters out of the
 *   ranges above, total_rows < 0, more than 65535 pairs, a short workspace.
 * roitr_fgr_batch_staged is the same call with the number of rows a pair may have to be staged in LDS (0 ... 1536; roitr_fgr_batch
 *   passes 1536): longer pairs are swept from global memory in the same order, so the results are bitwise the same for every value.
 *   It exists so that a test can hold the two paths against each other on the same rows. */
#define ROITR_FGR_NO_ROWS 1
#define ROITR_FGR_TOO_FEW 2
#define ROITR_FGR_SINGULAR 4
#define ROITR_FGR_NO_TUPLES 8
size_t roitr_fgr_workspace_bytes(int pairs, int total_rows);
int roitr_fgr_batch(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts, const float* scores,
                    const unsigned int* pair_keys, unsigned long long seed, float max_dist, double division_factor, int iterations,
                    int mu_every, int tuples, float tuple_scale, float radius, void* workspace, size_t workspace_bytes,
                    float* transforms, int* inliers, int* n_used, int* tuples_accepted, int* steps, double* mu, double* objective,
                    int* status, int* multiplicity, double* trace, roitr_stream_t stream);
int roitr_fgr_batch_staged(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts, const float* scores,
                           const unsigned int* pair_keys, unsigned long long seed, float max_dist, double division_factor,
                           int iterations, int mu_every, int tuples, float tuple_scale, float radius, int lds_rows, void* workspace,
                           size_t workspace_bytes, float* transforms, int* inliers, int* n_used, int* tuples_accepted, int* steps,
                           double* mu, double* objective, int* status, int* multiplicity, double* trace, roitr_stream_t stream);


/* ------------------------------------------------------------------ multiway registration
 * One pose per fragment of a scene in a common frame from the scene's pairwise poses, with wrong loop closures switched off by a
 * line process: the pose-graph optimisation of Choi, Zhou and Koltun (CVPR 2015), which Open3D exposes as global_optimization with
 * GlobalOptimizationLevenbergMarquardt.  PARITY WITH OPEN3D IS NOT CLAIMED: the operator is defined here.  Six-vectors are in the
 * project's order, rotation first: (a, b, g, tx, ty, tz).  Every product and sum is rounded on its own (no contraction).
 *
 * roitr_edge_information: the weight of an edge from the correspondences that produced its pose.  Inputs as roitr_lgr_batch: pair b
 * owns rows [starts[b], starts[b+1]) (clamped into [0, total_rows]) of src_pts / tgt_pts; transforms (pairs,4,4) fp32, source to
 * target; radius (finite, > 0).  A row is an inlier when rg_dist2(T p, q) < radius^2, in fp32 and strictly, as roitr_lgr_batch
 * verifies: n_inlier[b] equals its inliers[b] when its own transform is passed.  info (pairs,6,6) double = the sum over the inliers
 * of G^T G with G = [ -[p]x | I3 ], p the SOURCE point in its own frame as the double of the fp32 input: the rotation block is
 * sum (|p|^2 I - p p^T), the off-diagonal blocks hold +- sum p, info[3][3] = info[4][4] = info[5][5] = n_inlier.  Nine sums are
 * carried (the six of the rotation block and sum x, y, z): the other entries are zero, the count, or an exact negation.  Each is a
 * strided per-lane sum over the local row index (256 lanes) followed by the fixed butterfly of roitr_fgr_batch, so a pair's result is
 * bitwise independent of its batch, its slot, its row offset and of repeats.  One launch, one workgroup per pair; a pair without
 * rows gives zeros.  Refusals (ROITR_ERR_ARG, nothing launched): null pointers, a radius not finite and positive, total_rows < 0,
 * more than 65535 pairs.
 *
 * roitr_pose_graph_batch: `scenes` ragged scenes.  Scene s owns the nodes [node_starts[s], node_starts[s+1]) of init_poses / poses and
 * the edges [edge_starts[s], edge_starts[s+1]).  Edge e has edge_i, edge_j (int32, node indices LOCAL to the scene), edge_T (4,4 fp32,
 * mapping points of cloud i into cloud j's frame; only its first three rows are read), edge_info (6,6 double, the matrix Lambda,
 * rotation first; it must be symmetric, the solver reads the upper triangle of the system) and edge_uncertain (int32; 0: an
 * odometry edge, anything else: a loop closure under the line process).  init_poses (nodes,4,4) fp32 map a cloud's frame into the
 * scene's.  Node 0 of every scene is the gauge: it keeps its initial pose and has no unknowns; node k >= 1 owns the unknowns
 * [6 (k-1), 6 k) of the scene's u = 6 (n - 1).  node_starts_host / edge_starts_host are HOST copies of the two start arrays (scenes + 1
 * entries): the limits are checked and the workspace is laid out from them, nothing is read back from the device.
 * Parameters (double): mu (the line-process scale, finite, > 0; see roitr_amd.posegraph.line_process_weight), tau (finite, > 0),
 * step_tol (finite, >= 0), prune_threshold (0 ... 1); iterations 0 ... 1024.
 * The state X (one [R | t] per node) is double throughout, X = (double)init_poses at the start.
 * 1. Residual of edge e = (i, j): D = T_e^-1 X_j^-1 X_i, both inverses in closed form ([R^T | -R^T t]);
 *    xi = ((D21 - D12) / 2, (D02 - D20) / 2, (D10 - D01) / 2, D03, D13, D23), Drc the entry of row r, column c; e_e = xi^T (Lambda xi).
 * 2. Line process: l_e = 1 for a certain edge, (mu / (mu + e_e))^2 for an uncertain one.  The objective is
 *    F = sum_e [ l_e e_e + (uncertain ? mu (sqrt(l_e) - 1)^2 : 0) ], a strided per-lane sum over the scene's local edge index (256 lanes)
 *    and the fixed butterfly.
 * 3. Linearisation.  The update is X_k <- dT(delta_k) X_k, dT of compose_step_d (csrc/gauss_newton6.h).  Column k of J_e (6 x 6) is
 *    the six-vector (as in 1) of T_e^-1 X_j^-1 G_k X_i with the six generators G_k; the j side is exactly -J_e.
 *    M_e = l_e J^T (Lambda J), g_e = l_e J^T (Lambda xi).  H_ii += M, H_jj += M, H_ij -= M, H_ji -= M, b_i += g, b_j -= g (the gauge's
 *    rows and columns do not exist).  Every block of H and every segment of b is the sum of its edges' terms in ASCENDING EDGE INDEX,
 *    gathered through an adjacency list that is built once per scene; no floating-point atomics.
 * 4. Solve.  lambda_0 = tau * max diag(H) of the first assembly.  Every iteration solves (H + lambda I) delta = -b by a dense
 *    L D L^T in the workspace: for column j, t_k = V[k][j] / d_k (k < j); V[j][i] = A[i][j] - sum_{k<j} V[k][i] t_k for i >= j, one
 *    thread's sequential sum in ascending k, with d_j = V[j][j]; the right-hand side is carried as one more row i = u of the same
 *    recurrence (w_j = -b_j - sum_{k<j} w_k t_k).  Back substitution: delta_i = (w_i - sum_{k>i} V[i][k] delta_k) / d_i, the sum taken
 *    in DESCENDING k.  No entry depends on the thread mapping.  A pivot d_j that is not positive or not finite sets SINGULAR, keeps the
 *    state and ends the scene.
 * 5. Stop and gain.  max |delta| < step_tol, tested before delta is applied, sets CONVERGED and ends the scene.  Otherwise
 *    X'_k = dT(delta_k) X_k, F' = F(X') with its own line weights, rho = (F - F') / sum_q delta_q (lambda delta_q - b_q).
 *    rho > 0: X <- X', steps += 1, lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2.  Otherwise (a NaN included): X stays,
 *    lambda *= nu, nu *= 2 (nu starts at 2).  The loop ends after `iterations` solves; iterations = 0 returns the initial poses.
 * Outputs: poses (nodes,4,4) fp32, rounded once at the end (a node that never moved -- the gauge, every node of a scene without an
 *   accepted step -- gets the 16 floats of its initial pose); line_weight (edges) double, l_e at the final state; pruned (edges) int32,
 *   uncertain && l_e < prune_threshold; per scene steps (accepted), solves (run), objective (F at the final state), lambda_out (the
 *   last lambda) and status (bits below).  Optional (NULL allowed), rows that were not run are zero: trace_scalars (scenes x iterations
 *   x 8): F, lambda, rho, max |delta|, accepted (0 / 1), F', the denominator of rho, 1.0, per solve; trace_poses (nodes x iterations x
 *   12): the state [R | t] of every node BEFORE that solve; trace_delta (nodes x iterations x 6): the solve's delta (the gauge's row 0).
 * Status scenes get their initial poses, l = 1, pruned = 0 and zeros, and touch nothing else in the batch: ONE_NODE (fewer than two
 *   nodes; set alone, whatever edges the scene lists), else NO_EDGES, else BAD_EDGE (an index outside [0, n) or i == j; found by the
 *   status pass on the device); and BAD_COUNTS (the device
 *   start arrays disagree with the host copies: more than ROITR_POSEGRAPH_MAX_NODES nodes or a workspace slice outside the workspace).
 * Two launches for a whole batch: the status pass and the whole loop, one workgroup per scene; no workgroup waits for another and
 *   every loop is bounded by `iterations`.  H lives in the workspace, (6 (n - 1))^2 doubles per scene.
 * Determinism: a scene's results are bitwise independent of its batch, its slot, its node and edge offsets and of repeats.
 * The workspace (device, caller-owned) holds at least roitr_pose_graph_workspace_bytes() bytes (host-only; 0 for counts the batch
 *   call refuses).
 * Refusals (ROITR_ERR_ARG, nothing is launched or written): null pointers, host start arrays that do not begin at 0 or decrease, a
 *   scene of more than ROITR_POSEGRAPH_MAX_NODES nodes, more than 65535 scenes, parameters out of the ranges above, a short workspace. */
#define ROITR_POSEGRAPH_MAX_NODES 256
#define ROITR_POSEGRAPH_ONE_NODE 1
#define ROITR_POSEGRAPH_NO_EDGES 2
#define ROITR_POSEGRAPH_BAD_EDGE 4
#define ROITR_POSEGRAPH_SINGULAR 8
#define ROITR_POSEGRAPH_CONVERGED 16
#define ROITR_POSEGRAPH_BAD_COUNTS 32
int roitr_edge_information(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                           const float* transforms, float radius, double* info, int* n_inlier, roitr_stream_t stream);
size_t roitr_pose_graph_workspace_bytes(int scenes, const int* node_starts_host, const int* edge_starts_host);
int roitr_pose_graph_batch(int scenes, const int* node_starts, const int* edge_starts, const int* node_starts_host,
                           const int* edge_starts_host, const int* edge_i, const int* edge_j, const float* edge_T,
                           const double* edge_info, const int* edge_uncertain, const float* init_poses, double mu, double tau,
                           double step_tol, double prune_threshold, int iterations, void* workspace, size_t workspace_bytes,
                           float* poses, double* line_weight, int* pruned, int* steps, int* solves, double* objective,
                           double* lambda_out, int* status, double* trace_scalars, double* trace_poses, double* trace_delta,
                           roitr_stream_t stream);


/* ------------------------------------------------------------------ 4DMatch non-rigid evaluation
 * registration/evaluate_fdmatch.py:50-115: NFMR (non-rigid feature matching recall) of every pair of a batch.  Pair b owns points
 * [src_offsets[b], src_offsets[b+1]) of src_raw (the undeformed source) and src_deformed (what the model was fed), both (total_src,
 * 3); correspondences [corr_starts[b], corr_starts[b+1]) of src_corr / tgt_corr (total_corr, 3), the layout
 * RoitrForwardIO::pair_starts / out_src_pts / out_tgt_pts has; metric points [metric_starts[b], metric_starts[b+1]) of
 * metric_index (total_metric), indices into the pair's own cloud; rot (pairs, 3, 3), trans (pairs, 3).  All device pointers.
 *   anchors: idx_c = the nearest point of the pair's DEFORMED cloud to src_corr[c] (fp32 fmaf(dz,dz, fmaf(dy,dy, dx*dx)), the lowest
 *     index at equal distance), anchor_c = src_raw[idx_c], motion_c = tgt_corr[c] - anchor_c;
 *   blend: p = src_raw[metric_index[m]]; its 3 nearest anchors (same distance form, the lowest index at equal distance -- the
 *     reference's np.argpartition leaves that choice open); d < 1e-10 -> 1e-10, d > search_radius -> 1e10, weights (1 / d) / sum,
 *     flow = sum of weight x motion.  Three anchors beyond the radius weigh 1/3 each and the point still counts, as in the reference;
 *   err[m] = | p + flow - (rot_b src_deformed[metric_index[m]] + trans_b) |, hits[b] = #{ err < recall_thr }.  NFMR = hits / points.
 * status[b] (bits below): a pair with fewer than 3 anchors (or an empty cloud) or without metric points gets 0 hits and its bit
 * (the reference raises there); a metric index outside the pair's cloud is skipped, never dereferenced, and sets BAD_INDEX;
 * offsets that decrease or leave [0, total] set BAD_OFFSETS and are clamped before use.  err of a skipped point is +inf.
 * anchor_idx (total_corr, local to the pair) and err (total_metric) may be NULL.  block: lanes per workgroup, 0 (automatic), 64, 128
 * or 256; results do not depend on it, nor on the batch a pair travels in.  The workspace (device, caller-owned) holds at least
 * roitr_nfmr_workspace_bytes() bytes.  Refusals (ROITR_ERR_ARG): negative counts, null pointers, thresholds not finite and
 * positive, another block size, a short workspace. */
#define ROITR_NFMR_FEW_ANCHORS 1
#define ROITR_NFMR_NO_METRIC 2
#define ROITR_NFMR_BAD_INDEX 4
#define ROITR_NFMR_BAD_OFFSETS 8
size_t roitr_nfmr_workspace_bytes(int pairs, int total_corr, int total_metric);
int roitr_nfmr_batch(int pairs, int total_src, const int* src_offsets, const float* src_raw, const float* src_deformed, int total_corr,
                     const int* corr_starts, const float* src_corr, const float* tgt_corr, int total_metric, const int* metric_starts,
                     const int* metric_index, const float* rot, const float* trans, float search_radius, float recall_thr, int block,
                     int* anchor_idx, float* err, int* hits, int* status, void* workspace, size_t workspace_bytes,
                     roitr_stream_t stream);
/* blend_anchor_motion (evaluate_fdmatch.py:50-71, knn = 3) alone, batched: queries [query_starts[b], query_starts[b+1]) of
 * query_loc against references [ref_starts[b], ref_starts[b+1]) of ref_loc / ref_flow -> blended_flow (total_query, 3) and
 * mask (total_query; 1 where fewer than 3 of the 3 neighbours lie beyond the radius).  Fewer than 3 references: flow 0, mask 0 and
 * ROITR_NFMR_FEW_ANCHORS in status[b]. */
int roitr_blend_anchor_motion(int pairs, int total_ref, const int* ref_starts, const float* ref_loc, const float* ref_flow,
                              int total_query, const int* query_starts, const float* query_loc, float search_radius, int block,
                              float* blended_flow, int* mask, int* status, roitr_stream_t stream);


/* ------------------------------------------------------------------ descriptor matching
 * lib/utils.py:99-156 (matching_descriptors, square_distance) and registration/benchmark_utils.py:42-161 (mutual_selection,
 * get_inlier_ratio, ransac_pose_estimation): the best target of every source descriptor and the best source of every target
 * descriptor of every pair of a batch, from ONE fp32 MFMA product per pair whose (N, M) score matrix never reaches memory.
 * Pair b owns rows [src_offsets[b], src_offsets[b+1]) of src_desc (total_src, dim) and rows [tgt_offsets[b], tgt_offsets[b+1]) of
 * tgt_desc (total_tgt, dim); both may point into one buffer (the engine's point_feats holds the clouds of a call back to back).
 * The row ranges of different pairs must not overlap on either side.  All device pointers, 16-byte aligned.
 *   metric 0: score = s . t, the LARGEST wins;  metric 1: score = max((-2 s.t + |s|^2) + |t|^2, 1e-12) (square_distance with
 *   normalized = False, in its order), the SMALLEST wins.  fp32 operands, fp32 accumulation, a fixed k order: a score does not
 *   depend on the batch, on the tile it falls into or on the launch geometry.
 *   THE LOWEST INDEX WINS among equal scores, in both directions (np.argmax / np.argmin / torch.max).
 * row_idx / row_val (total_src): the best target of every source row, local to the pair, and its score; col_idx / col_val
 * (total_tgt) likewise.  A row whose pair has nothing on the other side, and every row outside all pairs, gets index -1 and value 0.
 * Offsets are clamped to [0, total] (and made non-decreasing) before use.  Descriptors are assumed finite; with non-finite input
 * every index still is -1 or inside its pair and nothing is read out of bounds.  Every output is bitwise independent of the batch
 * a pair travels in, of the order blocks finish in and of a repeat of the call.
 * Refusals: dim not a multiple of 4 in [4, 1024] -> ROITR_ERR_UNSUPPORTED; negative counts, null or misaligned pointers, a
 * workspace below roitr_desc_match_workspace_bytes(), an unknown metric -> ROITR_ERR_ARG. */
size_t roitr_desc_match_workspace_bytes(int pairs, int total_src, int total_tgt);
int roitr_desc_match_batch(int pairs, int dim, const int* src_offsets, int total_src, const float* src_desc, const int* tgt_offsets,
                           int total_tgt, const float* tgt_desc, int metric, int* row_idx, float* row_val, int* col_idx, float* col_val,
                           void* workspace, size_t workspace_bytes, roitr_stream_t stream);
/* Ordered compaction of the matches into corr (capacity, 2), local indices (source, target), pair b's at [corr_starts[b],
 * corr_starts[b+1]):  mode 0 (row-major): (i, row_idx[i]) for every source row i;  mode 1 (col-major): (col_idx[j], j) for every
 * target row j;  mode 2 (mutual): (i, row_idx[i]) where col_idx[row_idx[i]] == i, in increasing i (the order np.nonzero gives: a
 * row holds at most one mutual entry).  Entries whose index is -1 or outside the pair are left out.  The offsets are the ones
 * roitr_desc_match_batch was given (this call has no totals to clamp against).  *n_out: the count NEEDED; rows beyond capacity
 * are not written.  Refusals (ROITR_ERR_ARG): negative counts, null pointers, an unknown mode. */
int roitr_desc_match_select(int pairs, const int* src_offsets, const int* tgt_offsets, const int* row_idx, const int* col_idx, int mode,
                            int* corr_starts, int* corr, int capacity, int* n_out, roitr_stream_t stream);


/* ------------------------------------------------------------------ validation losses
 * lib/loss.py:8-166: the forward values of FineMatchingLoss and CoarseMatchingLoss (weighted_circle_loss) for every pair of a batch,
 * read from the buffers RoitrForwardIO describes, in place.  All device pointers; no host round trip; no float atomics: every output
 * is bitwise independent of the batch a pair travels in, of the slots its patches sit in and of a repeat of the call.
 * status[b] is WRITTEN by each call (bits below); the two calls take separate status arrays.
 *
 * Fine loss.  Pair b owns patch slots [first_slot[b], first_slot[b] + patch_count[b]) of the per-patch arrays (`slots` slots:
 * tgt_knn_pts / src_knn_pts (slots, L, 3), tgt_knn_masks / src_knn_masks (slots, L), matching_scores (slots, L+1, L+1)); the ranges
 * must lie in [0, slots) in increasing order without overlap -- b * num_corr and n_corr[b] in the strided layout, patch_offsets[b] and
 * the difference to the next entry in the compacted one.  Per patch: src' = src rot_b^T + trans_b (fp32 FMA chain),
 * gt[i][j] = (d2 < positive_radius^2) & tgt_mask[i] & src_mask[j] with d2 = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) of tgt_i - src'_j (NOT the
 * reference's |a|^2 + |b|^2 - 2ab: a label can differ where |d2 - r^2| lies inside that form's fp32 error), label (i, L) where a valid
 * tgt row has no gt, label (L, j) where a valid src column has none.  f_sum[b] = sum of the labelled matching_scores (fp32, summed in
 * float64 over the pair's patches in slot order), f_count[b] = number of labels, f_loss[b] = -f_sum / f_count; no labels (or no
 * patches): NaN and ROITR_LOSS_FINE_EMPTY.  A range outside [0, slots): ROITR_LOSS_BAD_OFFSETS, the pair counts as empty, nothing is
 * read through it; a range that starts before its predecessor's end (the slot-to-pair search needs increasing order): the same for
 * EVERY pair of the call.  L outside [1, 64] -> ROITR_ERR_UNSUPPORTED; negative counts, null pointers, a radius
 * not finite and positive, a workspace below roitr_fine_loss_workspace_bytes() -> ROITR_ERR_ARG.
 *
 * Coarse loss.  Pair b owns rows [tgt_first[b], tgt_first[b] + tgt_count[b]) of tgt_feats (total_tgt, D) and likewise of src_feats
 * (both may point into one buffer: the engine's node_feats holds the clouds of a call back to back); at most max_t / max_s rows.
 * feat_dists = sqrt(max((-2 t.s + |t|^2) + |s|^2, 1e-12)) (square_distance's order, fp32 FMA in k order); overlaps[i][j] from the
 * pair's gt_count[b] entries of gt_idx (pairs, gt_cap, 2) [tgt, src] / gt_overlaps (pairs, gt_cap), the last entry of a repeated node
 * pair winning, 0 elsewhere; pos = overlap > pos_overlap, neg = overlap == 0; weighted_circle_loss with pos_scales = sqrt(overlap):
 * the masked means over rows and columns of softplus(logsumexp_pos + logsumexp_neg) / log_scale, halved.  c_loss[b] is NaN with
 * ROITR_LOSS_COARSE_EMPTY when no row or no column has both a positive and a negative.  A ground-truth index outside the pair is
 * skipped, never dereferenced, and sets ROITR_LOSS_BAD_INDEX; a row range outside [0, total] or longer than max_t / max_s empties the
 * pair and sets ROITR_LOSS_BAD_OFFSETS.  D not a positive multiple of 4, more than 65535 pairs -> ROITR_ERR_UNSUPPORTED; negative
 * counts, null or misaligned (16 bytes) pointers, log_scale not finite and positive, a short workspace -> ROITR_ERR_ARG. */
#define ROITR_LOSS_FINE_EMPTY 1
#define ROITR_LOSS_COARSE_EMPTY 2
#define ROITR_LOSS_BAD_OFFSETS 4
#define ROITR_LOSS_BAD_INDEX 8
size_t roitr_fine_loss_workspace_bytes(int slots);
int roitr_fine_loss_batch(int pairs, int slots, const int* first_slot, const int* patch_count, int L, const float* tgt_knn_pts,
                          const float* src_knn_pts, const int* tgt_knn_masks, const int* src_knn_masks, const float* matching_scores,
                          const float* rot, const float* trans, float positive_radius, float* f_sum, int* f_count, float* f_loss,
                          int* status, void* workspace, size_t workspace_bytes, roitr_stream_t stream);
size_t roitr_coarse_loss_workspace_bytes(int pairs, int max_t, int max_s);
int roitr_coarse_loss_batch(int pairs, int D, const float* tgt_feats, int total_tgt, const int* tgt_first, const int* tgt_count,
                            const float* src_feats, int total_src, const int* src_first, const int* src_count, int max_t, int max_s,
                            int gt_cap, const int* gt_idx, const float* gt_overlaps, const int* gt_count, float pos_margin,
                            float neg_margin, float pos_optimal, float neg_optimal, float log_scale, float pos_overlap, float* c_loss,
                            int* status, void* workspace, size_t workspace_bytes, roitr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROITR_ENGINE_H */
