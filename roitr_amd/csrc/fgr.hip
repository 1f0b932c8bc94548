// Fast global registration: one Geman-McClure objective over all correspondences of a pair,
// minimised by 6x6 Gauss-Newton steps while the scale mu is lowered.  The rules are stated in include/roitr_engine.h above
// roitr_fgr_batch.  Two launches on the caller's stream, whatever the iteration count:
//   fgr_tuple_kernel   (chunks x pairs) blocks of 256, one triple of the RANSAC stream (rg_triple) per lane: the edge-length test in
//                      float64, an accepted triple adds 1 to the multiplicity of its three rows and to the pair's count (integer
//                      atomics on words a memset zeroed).  It leaves at once when no triples are asked for;
//   fgr_solve_kernel   one block of 256 per pair, the whole loop of the pair: the rows staged once in LDS as (point, score) and (point,
//                      multiplicity) -- a pair longer than the capacity is swept from global memory in the same order --, the centroids
//                      and the start scale, then per iteration the strided per-lane float64 sums, block_sum_d, the solve and the
//                      composition by wave 0, and the state and mu through LDS to all waves; at the end the fp32 transform and the
//                      inlier count.
// A thread carries 17 sums, not the 29 of A (21), g (6), objective and sum_omega: with J = [-[y]x | I] six entries of A are zero for
// every row, its three translation diagonals all equal sum_omega and the six entries of its rotation-translation block are
// +- sum omega y_i (a negation is exact), so carrying them would add the same bits again.
#include "common.h"
#include "procrustes_block.h"
#include "registration_math.h"
#include "roitr_engine.h"
#include "workspace.h"

#pragma clang fp contract(off)
#include "gauss_newton6.h"

namespace {

constexpr int FG_THREADS = LG_THREADS;
constexpr int FG_LDS_ROWS = 1536;        // rows of a pair that are staged: 2 x 16 bytes each, 48 KB
constexpr int FG_MAX_ITERATIONS = 1024;
constexpr int FG_MAX_TUPLES = 1 << 28;   // the iteration field of the stream's counter (registration_math.h rg_draw)
constexpr int FG_NS = 17;               // sums per thread, see above

struct FgWorkspace {
    int* mult;       // (total_rows) accepted triples per row
    int* accepted;   // (pairs) accepted triples
    size_t bytes;
};

FgWorkspace carve(void* ws, int pairs, int total_rows)
{
    Carve c(ws);
    FgWorkspace w;
    w.mult = c.take<int>((size_t)total_rows);
    w.accepted = c.take<int>((size_t)pairs);
    w.bytes = c.bytes;
    return w;
}

// ------------------------------------------------------------------------------------------------------------------ tuple test
__global__ __launch_bounds__(FG_THREADS) void fgr_tuple_kernel(const int* __restrict__ starts, int total_rows,
                                                               const float* __restrict__ src, const float* __restrict__ tgt,
                                                               const unsigned* __restrict__ pair_keys, unsigned long long seed,
                                                               int tuples, double scale, FgWorkspace ws)
{
    if (tuples == 0) return;
    const int b = blockIdx.y;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    const long it = (long)blockIdx.x * FG_THREADS + threadIdx.x;
    if (n < 3) return;
    bool ok = it < tuples;
    int i0 = 0, i1 = 0, i2 = 0;
    if (ok) ok = rg_triple(seed, pair_keys[b], (uint32_t)it, n, i0, i1, i2);
    if (ok) {
        const size_t r0 = (size_t)(s + i0), r1 = (size_t)(s + i1), r2 = (size_t)(s + i2);
        const double p0[3] = {src[3 * r0], src[3 * r0 + 1], src[3 * r0 + 2]}, q0[3] = {tgt[3 * r0], tgt[3 * r0 + 1], tgt[3 * r0 + 2]};
        const double p1[3] = {src[3 * r1], src[3 * r1 + 1], src[3 * r1 + 2]}, q1[3] = {tgt[3 * r1], tgt[3 * r1 + 1], tgt[3 * r1 + 2]};
        const double p2[3] = {src[3 * r2], src[3 * r2 + 1], src[3 * r2 + 2]}, q2[3] = {tgt[3 * r2], tgt[3 * r2 + 1], tgt[3 * r2 + 2]};
        auto edge = [&](const double (&pa)[3], const double (&pb)[3], const double (&qa)[3], const double (&qb)[3]) {
            const double ls = rg_len(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]), lt = rg_len(qa[0], qa[1], qa[2], qb[0], qb[1], qb[2]);
            return ls * scale < lt && lt * scale < ls;
        };
        ok = edge(p0, p1, q0, q1) && edge(p0, p2, q0, q2) && edge(p1, p2, q1, q2);
        if (ok) {
            atomicAdd(ws.mult + r0, 1);
            atomicAdd(ws.mult + r1, 1);
            atomicAdd(ws.mult + r2, 1);
        }
    }
    const int cnt = __popcll(__ballot(ok));   // one atomic per wave
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(ws.accepted + b, cnt);
}

// ------------------------------------------------------------------------------------------------------------------ solve
struct FgParams {
    double md2, division_factor;
    int iterations, mu_every, tuples;
    float thr2;
};

struct FgOut {
    float* T; int* inliers; int* n_used; int* accepted; int* steps; double* mu; double* objective; int* status; int* multiplicity;
    double* trace;
};

// The pair of rows [s, s + n) by its whole block.  STAGED: the rows sit in sa / sb (n <= the capacity); otherwise they are read from
// global memory.  row(j) yields the same values either way and every sum runs over j = tid, tid + 256, ..., so both give the same bits.
template <bool STAGED>
__device__ __forceinline__ void fgr_pair(int b, int s, int n, const float* __restrict__ src, const float* __restrict__ tgt,
                                         const float* __restrict__ scores, const int* __restrict__ mult, bool use_mult, int accepted,
                                         const FgParams& P, const FgOut& o, float4* sa, float4* sb, double* red, int* red4,
                                         double* sh_state, int* sh_stop)
{
    const int tid = threadIdx.x;
    // row j of the pair: source, target, weight (float64) and multiplicity
    auto row = [&](int j, double (&p)[3], double (&q)[3], double& w, int& m) {
        float sc;
        if (STAGED) {
            const float4 u = sa[j], v = sb[j];
            p[0] = u.x; p[1] = u.y; p[2] = u.z; sc = u.w;
            q[0] = v.x; q[1] = v.y; q[2] = v.z; m = __float_as_int(v.w);
        } else {
            const size_t r = (size_t)(s + j);
            p[0] = src[3 * r]; p[1] = src[3 * r + 1]; p[2] = src[3 * r + 2];
            q[0] = tgt[3 * r]; q[1] = tgt[3 * r + 1]; q[2] = tgt[3 * r + 2];
            sc = scores ? scores[r] : 1.0f;
            m = use_mult ? mult[r] : 1;
        }
        w = (double)sc * (double)m;
    };
    if (STAGED) {
        for (int j = tid; j < n; j += FG_THREADS) {
            const size_t r = (size_t)(s + j);
            const int m = use_mult ? mult[r] : 1;
            sa[j] = make_float4(src[3 * r], src[3 * r + 1], src[3 * r + 2], scores ? scores[r] : 1.0f);
            sb[j] = make_float4(tgt[3 * r], tgt[3 * r + 1], tgt[3 * r + 2], __int_as_float(m));
        }
        __syncthreads();
    }
    // used rows, their means, the multiplicity as it is used
    double csum[6] = {0, 0, 0, 0, 0, 0};
    int used = 0;
    for (int j = tid; j < n; j += FG_THREADS) {
        double p[3], q[3], w;
        int m;
        row(j, p, q, w, m);
        if (o.multiplicity) o.multiplicity[s + j] = m;
        if (w > 0.0) {
            ++used;
#pragma unroll
            for (int k = 0; k < 3; ++k) { csum[k] += p[k]; csum[3 + k] += q[k]; }
        }
    }
    used = block_sum_i(used, red4);
    block_sum_d<6>(csum, red);
    int st = (use_mult || P.tuples == 0 || n < 3) ? 0 : ROITR_FGR_NO_TUPLES;
    double S[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double cs[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
    double mu = 0.0, objective = 0.0;
    int steps = 0, ran = 0;
    if (n == 0) st = ROITR_FGR_NO_ROWS;
    else if (used < 3) st |= ROITR_FGR_TOO_FEW;
    else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { cs[k] = csum[k] / (double)used; ct[k] = csum[3 + k] / (double)used; }
        double d2 = 0.0;
        for (int j = tid; j < n; j += FG_THREADS) {
            double p[3], q[3], w;
            int m;
            row(j, p, q, w, m);
            if (w > 0.0) {
                const double px = p[0] - cs[0], py = p[1] - cs[1], pz = p[2] - cs[2];
                const double qx = q[0] - ct[0], qy = q[1] - ct[1], qz = q[2] - ct[2];
                d2 = fmax(d2, fmax(px * px + py * py + pz * pz, qx * qx + qy * qy + qz * qz));
            }
        }
        d2 = block_max_d(d2, red);
        mu = fmax(d2, P.md2);
        double* trace = o.trace ? o.trace + (size_t)b * P.iterations * 16 : nullptr;
        for (int k = 0; k < P.iterations; ++k) {
            double a[FG_NS];
#pragma unroll
            for (int i = 0; i < FG_NS; ++i) a[i] = 0.0;
            for (int j = tid; j < n; j += FG_THREADS) {
                double p[3], q[3], w;
                int m;
                row(j, p, q, w, m);
                if (!(w > 0.0)) continue;
                const double px = p[0] - cs[0], py = p[1] - cs[1], pz = p[2] - cs[2];
                const double y0 = S[0] * px + S[1] * py + S[2] * pz + S[3];
                const double y1 = S[4] * px + S[5] * py + S[6] * pz + S[7];
                const double y2 = S[8] * px + S[9] * py + S[10] * pz + S[11];
                const double r0 = y0 - (q[0] - ct[0]), r1 = y1 - (q[1] - ct[1]), r2 = y2 - (q[2] - ct[2]);
                const double e = r0 * r0 + r1 * r1 + r2 * r2;
                const double l = mu / (e + mu);
                const double om = w * l * l;
                // A = sum om J^T J, upper triangle, J = [K | I], K = -[y]x: the rotation block K^T K, then K^T
                a[0] += om * (y1 * y1 + y2 * y2);
                a[1] -= om * (y0 * y1);
                a[2] -= om * (y0 * y2);
                a[3] += om * (y0 * y0 + y2 * y2);
                a[4] -= om * (y1 * y2);
                a[5] += om * (y0 * y0 + y1 * y1);
                a[6] += om * y0;     // A(1,5) = -a[6], A(2,4) = +a[6]
                a[7] += om * y1;     // A(0,5) = +a[7], A(2,3) = -a[7]
                a[8] += om * y2;     // A(0,4) = -a[8], A(1,3) = +a[8]
                // g = sum om J^T r
                a[9] += om * (y1 * r2 - y2 * r1);
                a[10] += om * (y2 * r0 - y0 * r2);
                a[11] += om * (y0 * r1 - y1 * r0);
                a[12] += om * r0;
                a[13] += om * r1;
                a[14] += om * r2;
                a[15] += w * mu * e / (e + mu);
                a[16] += om;
            }
            block_sum_d<FG_NS>(a, red);
            objective = a[15];
            ++ran;
            if (tid < 64) {   // every lane holds the same sums and takes the same decisions; lane 0 writes
                if (trace && tid == 0) {
                    double* tr = trace + (size_t)k * 16;
#pragma unroll
                    for (int i = 0; i < 12; ++i) tr[i] = S[i];
                    tr[12] = mu; tr[13] = a[15]; tr[14] = a[16]; tr[15] = 1.0;
                }
                const double A21[21] = {a[0], a[1], a[2], 0.0, -a[8], a[7],
                                        a[3], a[4], a[8], 0.0, -a[6],
                                        a[5], -a[7], a[6], 0.0,
                                        a[16], 0.0, 0.0,
                                        a[16], 0.0,
                                        a[16]};
                const double rhs[6] = {-a[9], -a[10], -a[11], -a[12], -a[13], -a[14]};
                double x[6], Sn[12];
                const bool ok = ldl_solve6(A21, rhs, x);
                if (ok) compose_step_d(x, S, Sn);
                if (tid == 0) {
                    *sh_stop = ok ? 0 : 1;
                    if (ok)
#pragma unroll
                        for (int i = 0; i < 12; ++i) sh_state[i] = Sn[i];
                }
            }
            __syncthreads();
            if (*sh_stop) { st |= ROITR_FGR_SINGULAR; break; }
#pragma unroll
            for (int i = 0; i < 12; ++i) S[i] = sh_state[i];
            ++steps;
            if ((k + 1) % P.mu_every == 0 && mu > P.md2) mu = fmax(mu / P.division_factor, P.md2);
        }
        if (trace)
            for (int i = ran * 16 + tid; i < P.iterations * 16; i += FG_THREADS) trace[i] = 0.0;
    }
    if (o.trace && (n == 0 || used < 3))
        for (int i = tid; i < P.iterations * 16; i += FG_THREADS) o.trace[(size_t)b * P.iterations * 16 + i] = 0.0;
    // [R | ct + t - R cs], rounded once
    float T[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double tr = ct[r] + S[4 * r + 3] - (S[4 * r] * cs[0] + S[4 * r + 1] * cs[1] + S[4 * r + 2] * cs[2]);
        T[4 * r] = (float)S[4 * r]; T[4 * r + 1] = (float)S[4 * r + 1]; T[4 * r + 2] = (float)S[4 * r + 2]; T[4 * r + 3] = (float)tr;
    }
    int cnt = 0;
    for (int j = tid; j < n; j += FG_THREADS) {
        double p[3], q[3], w;
        int m;
        row(j, p, q, w, m);
        cnt += rg_dist2(T, (float)p[0], (float)p[1], (float)p[2], (float)q[0], (float)q[1], (float)q[2]) < P.thr2;
    }
    cnt = block_sum_i(cnt, red4);
    write_T44(o.T + 16 * (size_t)b, T);
    if (tid == 0) {
        o.inliers[b] = cnt;
        o.n_used[b] = used;
        o.accepted[b] = accepted;
        o.steps[b] = steps;
        o.mu[b] = mu;
        o.objective[b] = objective;
        o.status[b] = st;
    }
}

__global__ __launch_bounds__(FG_THREADS) void fgr_solve_kernel(const int* __restrict__ starts, int total_rows,
                                                               const float* __restrict__ src, const float* __restrict__ tgt,
                                                               const float* __restrict__ scores, int lds_rows, FgWorkspace ws, FgParams P,
                                                               FgOut o)
{
    __shared__ float4 sa[FG_LDS_ROWS], sb[FG_LDS_ROWS];
    __shared__ double red[4 * FG_NS];
    __shared__ double sh_state[12];
    __shared__ int red4[4];
    __shared__ int sh_stop;
    const int b = blockIdx.x;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    const int accepted = (P.tuples > 0 && n >= 3) ? ws.accepted[b] : 0;
    const bool use_mult = accepted > 0;
    if (n <= lds_rows)
        fgr_pair<true>(b, s, n, src, tgt, scores, ws.mult, use_mult, accepted, P, o, sa, sb, red, red4, sh_state, &sh_stop);
    else
        fgr_pair<false>(b, s, n, src, tgt, scores, ws.mult, use_mult, accepted, P, o, sa, sb, red, red4, sh_state, &sh_stop);
}

bool finite_positive(float v) { return v > 0.f && v <= 3.402823466e38f; }

}  // namespace

extern "C" size_t roitr_fgr_workspace_bytes(int pairs, int total_rows)
{
    if (pairs <= 0 || pairs > 65535 || total_rows < 0) return 0;
    return carve(nullptr, pairs, total_rows).bytes;
}

extern "C" int roitr_fgr_batch_staged(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                                      const float* scores, const unsigned int* pair_keys, unsigned long long seed, float max_dist,
                                      double division_factor, int iterations, int mu_every, int tuples, float tuple_scale, float radius,
                                      int lds_rows, void* workspace, size_t workspace_bytes_given, float* transforms, int* inliers,
                                      int* n_used, int* tuples_accepted, int* steps, double* mu, double* objective, int* status,
                                      int* multiplicity, double* trace, hipStream_t stream)
{
    if (!finite_positive(max_dist)) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: max_dist must be finite and positive");
    if (!finite_positive(radius)) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: radius must be finite and positive");
    if (!(division_factor > 1.0) || !(division_factor <= 1.7976931348623157e308))
        return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: division_factor must be finite and above 1");
    if (iterations < 1 || iterations > FG_MAX_ITERATIONS) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: iterations outside 1 ... 1024");
    if (mu_every < 1) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: mu_every < 1");
    if (tuples < 0 || tuples > FG_MAX_TUPLES) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: tuples outside 0 ... 2^28");
    if (!(tuple_scale > 0.f) || !(tuple_scale < 1.f)) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: tuple_scale outside (0, 1)");
    if (lds_rows < 0 || lds_rows > FG_LDS_ROWS) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch_staged: lds_rows outside 0 ... 1536");
    if (pairs <= 0) return ROITR_OK;
    if (total_rows < 0 || pairs > 65535) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: total_rows < 0 or pairs > 65535");
    if (!starts || !transforms || !inliers || !n_used || !tuples_accepted || !steps || !mu || !objective || !status ||
        (total_rows > 0 && (!src_pts || !tgt_pts)))
        return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: null pointer");
    if (tuples > 0 && !pair_keys) return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: pair_keys is null with tuples > 0");
    const FgWorkspace ws = carve(workspace, pairs, total_rows);
    if (workspace_bytes_given < ws.bytes || !workspace)
        return refuse(ROITR_ERR_ARG, "roitr_fgr_batch: workspace smaller than roitr_fgr_workspace_bytes()");
    if (total_rows > 0) ROITR_HIP(hipMemsetAsync(ws.mult, 0, (size_t)total_rows * sizeof(int), stream));
    ROITR_HIP(hipMemsetAsync(ws.accepted, 0, (size_t)pairs * sizeof(int), stream));
    fgr_tuple_kernel<<<dim3(tuples > 0 ? div_up(tuples, FG_THREADS) : 1, pairs), FG_THREADS, 0, stream>>>(
        starts, total_rows, src_pts, tgt_pts, pair_keys, seed, tuples, (double)tuple_scale, ws);
    ROITR_LAUNCH_CHECK();
    FgParams P;
    P.md2 = (double)max_dist * (double)max_dist;
    P.division_factor = division_factor;
    P.iterations = iterations; P.mu_every = mu_every; P.tuples = tuples;
    P.thr2 = radius * radius;
    const FgOut o = {transforms, inliers, n_used, tuples_accepted, steps, mu, objective, status, multiplicity, trace};
    fgr_solve_kernel<<<pairs, FG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, scores, lds_rows, ws, P, o);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_fgr_batch(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                               const float* scores, const unsigned int* pair_keys, unsigned long long seed, float max_dist,
                               double division_factor, int iterations, int mu_every, int tuples, float tuple_scale, float radius,
                               void* workspace, size_t workspace_bytes_given, float* transforms, int* inliers, int* n_used,
                               int* tuples_accepted, int* steps, double* mu, double* objective, int* status, int* multiplicity,
                               double* trace, hipStream_t stream)
{
    return roitr_fgr_batch_staged(pairs, starts, total_rows, src_pts, tgt_pts, scores, pair_keys, seed, max_dist, division_factor,
                                  iterations, mu_every, tuples, tuple_scale, radius, FG_LDS_ROWS, workspace, workspace_bytes_given,
                                  transforms, inliers, n_used, tuples_accepted, steps, mu, objective, status, multiplicity, trace, stream);
}
