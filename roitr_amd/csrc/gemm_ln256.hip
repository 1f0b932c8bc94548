// nn.Linear + (residual) LayerNorm for the 256-wide fp32 layers in one launch: a 32 x 256 block tile.
//
// gemm_kernel<true, 4, true> (gemm.hip) spans a 256-wide row with a 64 x 256 tile: four accumulators per wave, half as many blocks as
// the coarse levels have slots for, and an epilogue that fetches residual rows two at a time.  This kernel gives a block 32 rows:
// every wave owns all 32 rows and two 32 x 32 accumulators (columns 64 w .. 64 w + 63), so a launch has twice the tiles and a wave half
// the MFMA stream per K-slab, at about the arithmetic intensity of the 64 x 64 tile the plain GEMMs run on.
//
// Bitwise the two-launch result (roitr_gemm + roitr_add_layernorm / roitr_add_layernorm_interp), for the same reasons as the fused
// epilogue of gemm_kernel: the LDS image is its [kh][row][kk] image with the same global-k -> slot map, the products are
// v_mfma_f32_32x32x2_f32 in ascending slot order, `acc * alpha + bias` is the same expression, and the rows are normalised with
// add_layernorm_kernel<4>'s arithmetic and summation order (lane owns columns lane + 64 i).
//
// Takes the fast fp32 LayerNorm launches with N == 256 and no row gather on A or W, no batching (roitr_gemm_ln256_takes); the options
// are ln_res, ln_res_idx, ln_post, ln_relu, ip_*, A2, A_cat, a_cat_idx, k_cat, alpha, bias.  A block reads all of its A rows (K loop)
// and all of its residual / post rows (requested right behind the K loop) before it stores an output row, so out == A and
// out == ln_res (without ln_res_idx) are legal.
#include "common.h"
#include "gemm_host.h"
#include "gemm_tile.h"

namespace {

constexpr int BK = 32, LDR = 20;   // K-slab; row pitch (floats) of the [kh][row][kk] LDS image: gemm.hip's
constexpr int LM = 32, LC = 256;   // block tile
constexpr int LN256_IL_MIN_TILES = 1024;   // tiles from which the staging loads are issued between the MFMAs (gemm.hip: GEMM_IL_MIN_TILES)
constexpr int LN256_ZERO_LEN = 2048;       // longest K of the fast path (gemm.hip: ZERO_ROW_LEN)
__device__ __attribute__((aligned(16))) float g_ln256_zero_row[LN256_ZERO_LEN];

// HA2: the launch has an elementwise addend on A; IL: staging loads spread over the MFMA stream (both as in gemm_kernel)
template <bool HA2, bool IL>
__global__ __launch_bounds__(256) void gemm_ln256_kernel(RoitrGemm g, int T)
{
    constexpr int STAGE = 2 * LM * LDR + 2 * LC * LDR, TP = LC + 1;
    static_assert(LM * TP <= STAGE, "the parked tile must fit the staging LDS");
    __shared__ __attribute__((aligned(16))) float smem[STAGE];
    float* As = smem;
    float* Bs = smem + 2 * LM * LDR;
    const int tile = xcd_block_id_live(T);
    if (tile < 0) return;
    const int m0 = tile * LM;
    const float* bias = g.bias;
    float* C = g.C;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // W: gemm_kernel's stager (thread = row r + 64 v, k quarter tid & 3: floats 4 j.. and 16 + 4 j.. -> slots 8 j .. 8 j + 7)
    const int r = tid >> 2, kq = (tid & 3) * 8, kf = (tid & 3) * 4;
    // A: 32 rows x 8 pieces of four k; piece (j, h) = floats 4 j + 16 h .. -> slots 8 j + 4 h .. 8 j + 4 h + 3 (the same map)
    const int ra = tid >> 3, ja = tid & 3, ha = (tid >> 2) & 1, ka = 4 * ja + 16 * ha;

    const float* arow = g_ln256_zero_row; const float* arow2 = g_ln256_zero_row; const float* arowc = g_ln256_zero_row;
    {
        const int am = m0 + ra;
        if (am < g.M) {
            arow = g.A + (size_t)am * g.lda;
            if (HA2) arow2 = g.A2 + (size_t)am * g.lda;
            if (g.A_cat) arowc = g.A_cat + (size_t)(g.a_cat_idx ? g.a_cat_idx[am] : am) * g.lda_cat;
        }
    }
    const float* wrow[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) wrow[v] = g.W + (size_t)(r + 64 * v) * g.ldw + kf;

    f32x16 acc[2];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[v][i] = 0.f;

    float4 av, a2v = make_float4(0.f, 0.f, 0.f, 0.f);
    float wv[4][8];
    auto asrc = [&](int k) { return ((g.A_cat && k >= g.k_cat) ? arowc + (k - g.k_cat) : arow + k) + ka; };   // slab-uniform: k_cat % 32 == 0
    auto a2src = [&](int k) { return ((g.A_cat && k >= g.k_cat) ? g_ln256_zero_row : arow2 + k) + ka; };      // the addend covers the A part only
    {
        av = *reinterpret_cast<const float4*>(asrc(0));
        if (HA2) a2v = *reinterpret_cast<const float4*>(a2src(0));
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float4 x = *reinterpret_cast<const float4*>(wrow[v]), y = *reinterpret_cast<const float4*>(wrow[v] + 16);
            wv[v][0] = x.x; wv[v][1] = x.y; wv[v][2] = x.z; wv[v][3] = x.w; wv[v][4] = y.x; wv[v][5] = y.y; wv[v][6] = y.z; wv[v][7] = y.w;
        }
    }
    const int kh = lane >> 5, ml = lane & 31;
    const float4* ar = reinterpret_cast<const float4*>(As + (kh * LM + ml) * LDR);
    const float4* br = reinterpret_cast<const float4*>(Bs + (kh * LC + wave * 64 + ml) * LDR);
    float2* aw0 = reinterpret_cast<float2*>(As + (0 * LM + ra) * LDR + 4 * ja + 2 * ha);
    float2* aw1 = reinterpret_cast<float2*>(As + (1 * LM + ra) * LDR + 4 * ja + 2 * ha);
    float4* bw0 = reinterpret_cast<float4*>(Bs + (0 * LC + r) * LDR + (kq >> 1));
    float4* bw1 = reinterpret_cast<float4*>(Bs + (1 * LC + r) * LDR + (kq >> 1));
    for (int k0 = 0; k0 < g.K; k0 += BK) {
        __syncthreads();
        if (HA2) { av.x += a2v.x; av.y += a2v.y; av.z += a2v.z; av.w += a2v.w; }
        *aw0 = make_float2(av.x, av.z); *aw1 = make_float2(av.y, av.w);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            bw0[v * 64 * LDR / 4] = make_float4(wv[v][0], wv[v][2], wv[v][4], wv[v][6]);
            bw1[v * 64 * LDR / 4] = make_float4(wv[v][1], wv[v][3], wv[v][5], wv[v][7]);
        }
        __syncthreads();
        // every fragment of the slab in registers before its MFMAs
        float4 af[4], bf[2][4];
        if (!IL) {   // burst: the next slab's loads behind the barrier, in flight across the MFMA block
            if (k0 + BK < g.K) {
                const int kn = k0 + BK;
                av = *reinterpret_cast<const float4*>(asrc(kn));
                if (HA2) a2v = *reinterpret_cast<const float4*>(a2src(kn));
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float4 x = *reinterpret_cast<const float4*>(wrow[v] + kn), y = *reinterpret_cast<const float4*>(wrow[v] + kn + 16);
                    wv[v][0] = x.x; wv[v][1] = x.y; wv[v][2] = x.z; wv[v][3] = x.w; wv[v][4] = y.x; wv[v][5] = y.y; wv[v][6] = y.z; wv[v][7] = y.w;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            af[q] = ar[q];
#pragma unroll
            for (int v = 0; v < 2; ++v) bf[v][q] = br[v * 32 * LDR / 4 + q];
        }
        __builtin_amdgcn_sched_barrier(0);
        const int kn = k0 + BK < g.K ? k0 + BK : k0;   // IL: the last slab re-fetches itself (no branch in the stream)
        const float* an = asrc(kn);
        const float* a2n = a2src(kn);
        constexpr int NS = 1 + (HA2 ? 1 : 0) + 8, TOT = 32;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const float a = c == 0 ? af[q].x : c == 1 ? af[q].y : c == 2 ? af[q].z : af[q].w;
                    const float b = c == 0 ? bf[v][q].x : c == 1 ? bf[v][q].y : c == 2 ? bf[v][q].z : bf[v][q].w;
                    acc[v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[v], 0, 0, 0);
                    if (IL) {
                        const int n = (q * 4 + c) * 2 + v;
#pragma unroll
                        for (int i = 0; i < NS; ++i)
                            if (n == (i * TOT + TOT / 2) / NS) {
                                __builtin_amdgcn_sched_barrier(0);
                                if (i == 0) av = *reinterpret_cast<const float4*>(an);
                                else if (HA2 && i == 1) a2v = *reinterpret_cast<const float4*>(a2n);
                                else {
                                    const int j = i - 1 - (HA2 ? 1 : 0), h = j & 1, wr = j >> 1;   // half h of staging row wr
                                    const float4 x = *reinterpret_cast<const float4*>(wrow[wr] + kn + 16 * h);
                                    wv[wr][4 * h] = x.x; wv[wr][4 * h + 1] = x.y; wv[wr][4 * h + 2] = x.z; wv[wr][4 * h + 3] = x.w;
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                    }
                }
        __builtin_amdgcn_sched_barrier(0);  // consumers of the prefetched registers stay below the MFMAs
    }

    // ---- epilogue: wave w normalises rows w, w + 4, .., w + 28 of the tile
    float gam[4], bet[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { gam[i] = g.ln_gamma[lane + 64 * i]; bet[i] = g.ln_beta[lane + 64 * i]; }
    // residual / post rows of ALL eight rows requested here, in front of the parking and its barriers: one HBM round trip under the
    // parking instead of one per row behind two wave reductions (the staging and fragment registers are free by now)
    float resv[8][4], postv[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int row_ = m0 + wave + 4 * u;
#pragma unroll
        for (int i = 0; i < 4; ++i) { resv[u][i] = 0.f; postv[u][i] = 0.f; }
        if (row_ < g.M) {
            if (g.ln_res) {
                const float* rr = g.ln_res + (size_t)(g.ln_res_idx ? g.ln_res_idx[row_] : row_) * LC;
#pragma unroll
                for (int i = 0; i < 4; ++i) resv[u][i] = rr[lane + 64 * i];
            }
            if (g.ln_post) {
#pragma unroll
                for (int i = 0; i < 4; ++i) postv[u][i] = g.ln_post[(size_t)row_ * LC + lane + 64 * i];
            }
        }
    }
    float* tile_ = smem;   // [LM][TP]
    __syncthreads();   // every wave is done with the operand images
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int col = wave * 64 + v * 32 + (lane & 31);
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int rl = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            tile_[rl * TP + col] = acc[v][i] * g.alpha + bv;
        }
    }
    __syncthreads();
    // TransitionUp addend: lane t holds the descriptors of the wave's t-th row (indices, normalised weights: interp3_add_kernel's
    // expressions), the rows' feature values are fetched one row AHEAD of their use
    int pi0 = 0, pi1 = 0, pi2 = 0; float pw0 = 0.f, pw1 = 0.f, pw2 = 0.f;
    float fn0[4], fn1[4], fn2[4];
    if (g.ip_feat) {
        const int rowl = m0 + wave + 4 * lane;
        if (lane < LM / 4 && rowl < g.M) {
            const int* ii = g.ip_idx + (size_t)rowl * 3;
            const float* dd = g.ip_dist2 + (size_t)rowl * 3;
            pi0 = ii[0]; pi1 = ii[1]; pi2 = ii[2];
            pw0 = 1.0f / (sqrtf(dd[0]) + 1e-8f); pw1 = 1.0f / (sqrtf(dd[1]) + 1e-8f); pw2 = 1.0f / (sqrtf(dd[2]) + 1e-8f);
            const float ws = (pw0 + pw1) + pw2;
            pw0 /= ws; pw1 /= ws; pw2 /= ws;
        }
        const float* a0 = g.ip_feat + (size_t)__builtin_amdgcn_readlane(pi0, 0) * LC;
        const float* a1 = g.ip_feat + (size_t)__builtin_amdgcn_readlane(pi1, 0) * LC;
        const float* a2 = g.ip_feat + (size_t)__builtin_amdgcn_readlane(pi2, 0) * LC;
#pragma unroll
        for (int i = 0; i < 4; ++i) { fn0[i] = a0[lane + 64 * i]; fn1[i] = a1[lane + 64 * i]; fn2[i] = a2[lane + 64 * i]; }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int rl = wave + 4 * u;
        const int row = m0 + rl;
        if (row >= g.M) break;   // wave-uniform
        float fc0[4], fc1[4], fc2[4];
        float w0 = 0.f, w1 = 0.f, w2 = 0.f;
        if (g.ip_feat) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { fc0[i] = fn0[i]; fc1[i] = fn1[i]; fc2[i] = fn2[i]; }
            w0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pw0), u));
            w1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pw1), u));
            w2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pw2), u));
            if (u + 1 < 8 && row + 4 < g.M) {        // the next row's feature rows: in flight across this row's LayerNorm
                const float* a0 = g.ip_feat + (size_t)__builtin_amdgcn_readlane(pi0, (u + 1) & 7) * LC;
                const float* a1 = g.ip_feat + (size_t)__builtin_amdgcn_readlane(pi1, (u + 1) & 7) * LC;
                const float* a2 = g.ip_feat + (size_t)__builtin_amdgcn_readlane(pi2, (u + 1) & 7) * LC;
#pragma unroll
                for (int i = 0; i < 4; ++i) { fn0[i] = a0[lane + 64 * i]; fn1[i] = a1[lane + 64 * i]; fn2[i] = a2[lane + 64 * i]; }
            }
        }
        float t[4];
        float s_ = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            t[i] = tile_[rl * TP + lane + 64 * i];
            if (g.ln_res) t[i] += resv[u][i];
            s_ += t[i];
        }
        const float mean = wave_sum(s_) / (float)LC;
        float q_ = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float d = t[i] - mean; q_ += d * d; }
        const float rstd = 1.0f / sqrtf(wave_sum(q_) / (float)LC + g.ln_eps);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float y = (t[i] - mean) * rstd * gam[i] + bet[i];
            if (g.ln_post) y += postv[u][i];
            if (g.ln_relu) y = fmaxf(y, 0.f);
            if (g.ip_feat) {   // TransitionUp: + three-nearest-neighbour interpolation, after the activation
                float acc_ = 0.f;
                acc_ += fc0[i] * w0; acc_ += fc1[i] * w1; acc_ += fc2[i] * w2;
                y = y + acc_;
            }
            C[(size_t)row * g.ldc + lane + 64 * i] = y;
        }
    }
}

int g_ln256_tile_rows = LM;   // roitr_gemm_set_ln256_tile

}  // namespace

// Diagnostics (scripts/bench_gemm_ln.py): rows of the block tile the fast 256-wide LayerNorm launches of roitr_gemm get -- 32 (this
// kernel, the default) or 64 (gemm_kernel<true, 4, true>).  Process-wide; the results are the same bytes either way.
extern "C" int roitr_gemm_set_ln256_tile(int rows)
{
    g_ln256_tile_rows = rows == 64 ? 64 : LM;
    return ROITR_OK;
}

// Whether the launch is one of this kernel's.  The caller (roitr_gemm) has established the fast path (K % 32 == 0, K <= 2048, 16-byte
// rows of A, A2 and W), the LayerNorm shape rules (gemm_ln_shape_ok) and the A_cat / ip_* rules.
bool roitr_gemm_ln256_takes(const RoitrGemm* g)
{
    return g_ln256_tile_rows == LM && g->ln_gamma && g->N == LC && !g->bf16 && !g->a_idx && !g->w_idx && g->a_limit <= 0 && g->w_limit <= 0 &&
           g->batch == 1 && !g->seg_off && !g->batch_live && g->K <= LN256_ZERO_LEN && div_up(g->M, LM) <= 0x7ffffff0 / 8;
}

void roitr_gemm_ln256_launch(const RoitrGemm* g, hipStream_t stream)
{
    const int T = div_up(g->M, LM);
    const unsigned grid = (unsigned)xcd_grid(T);
    const bool a2 = g->A2 != nullptr, il = T >= LN256_IL_MIN_TILES;
    if (a2 && il) gemm_ln256_kernel<true, true><<<grid, 256, 0, stream>>>(*g, T);
    else if (a2) gemm_ln256_kernel<true, false><<<grid, 256, 0, stream>>>(*g, T);
    else if (il) gemm_ln256_kernel<false, true><<<grid, 256, 0, stream>>>(*g, T);
    else gemm_ln256_kernel<false, false><<<grid, 256, 0, stream>>>(*g, T);
}
