// Multiway registration: the information matrix of an edge from its correspondences and the
// pose-graph optimisation of a scene with a line process over its loop closures (Choi, Zhou and Koltun, CVPR 2015).  The rules are
// stated in include/roitr_engine.h above roitr_edge_information.  Launches on the caller's stream:
//   edge_information_kernel  one block of 256 per pair: the fp32 inlier test of the verification, nine float64 sums as strided per-lane
//                            sums with block_sum_d, the 36 entries from them;
//   pg_status_kernel         one block per scene: the scene's workspace offset (an integer sum over the scenes before it), the count
//                            checks and the scan of its edge indices; writes status[s] and the offset;
//   pg_solve_kernel          one block per scene, the whole Levenberg-Marquardt loop: the adjacency list once, then per iteration the
//                            edge terms (thread per edge, per column, per entry, handed on through the scene's workspace slice), the
//                            gather of H and b in ascending edge index, the dense L D L^T with the right-hand side as one more row,
//                            the back substitution, the trial state and its objective, the gain.
// The factor V is kept in the UPPER triangle of H (V[k][i], k <= i), so the lanes of a wave read neighbouring addresses in the inner
// product loop; the pivots d and the column's multipliers t live in LDS.  A scene's H stays in L2 at the 3DMatch scene sizes.
#include "common.h"
#include "procrustes_block.h"
#include "registration_math.h"
#include "roitr_engine.h"
#include "workspace.h"

#pragma clang fp contract(off)
#include "gauss_newton6.h"

namespace {

constexpr int PG_THREADS = LG_THREADS;
constexpr int PG_MAX_NODES = ROITR_POSEGRAPH_MAX_NODES;
constexpr int PG_MAX_U = 6 * (PG_MAX_NODES - 1);                           // 1530 unknowns
constexpr int PG_ROWS = (PG_MAX_U + 1 + PG_THREADS - 1) / PG_THREADS;    // rows of the factor (and the right-hand side) per thread: 6
constexpr int PG_MAX_ITERATIONS = 1024;
// per-edge doubles in the workspace: A = T_e^-1 X_j^-1 (12), xi (6), Lambda xi (6), J (36), Lambda J (36), M (36), g (6), l (1)
constexpr int PG_A = 0, PG_XI = 12, PG_LXI = 18, PG_J = 24, PG_LJ = 60, PG_M = 96, PG_G = 132, PG_L = 138, PG_EDGE = 139;

// ------------------------------------------------------------------------------------------------------------------ edge information
__global__ __launch_bounds__(PG_THREADS) void edge_information_kernel(const int* __restrict__ starts, int total_rows,
                                                                      const float* __restrict__ src, const float* __restrict__ tgt,
                                                                      const float* __restrict__ transforms, float thr2,
                                                                      double* __restrict__ info, int* __restrict__ n_inlier)
{
    __shared__ double red[4 * 9];
    __shared__ int red4[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = transforms[16 * (size_t)b + k];
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cnt = 0;
    for (int j = tid; j < n; j += PG_THREADS) {
        const size_t r = (size_t)(s + j);
        const float px = src[3 * r], py = src[3 * r + 1], pz = src[3 * r + 2];
        if (!(rg_dist2(T, px, py, pz, tgt[3 * r], tgt[3 * r + 1], tgt[3 * r + 2]) < thr2)) continue;
        const double x = px, y = py, z = pz;
        ++cnt;
        a[0] += y * y + z * z;
        a[1] += x * y;
        a[2] += x * z;
        a[3] += x * x + z * z;
        a[4] += y * z;
        a[5] += x * x + y * y;
        a[6] += x;
        a[7] += y;
        a[8] += z;
    }
    block_sum_d<9>(a, red);
    cnt = block_sum_i(cnt, red4);
    if (tid == 0) {
        const double c = (double)cnt, o = 0.0;
        // G^T G of G = [-[p]x | I]: the rotation block |p|^2 I - p p^T, then [p]x (upper right) and its transpose
        const double I[36] = {a[0], o - a[1], o - a[2], o, o - a[8], a[7],
                              o - a[1], a[3], o - a[4], a[8], o, o - a[6],
                              o - a[2], o - a[4], a[5], o - a[7], a[6], o,
                              o, a[8], o - a[7], c, o, o,
                              o - a[8], o, a[6], o, c, o,
                              a[7], o - a[6], o, o, o, c};
        for (int k = 0; k < 36; ++k) info[36 * (size_t)b + k] = I[k];
        n_inlier[b] = cnt;
    }
}

// ------------------------------------------------------------------------------------------------------------------ pose graph
// A scene's slice of the workspace, in doubles from its start; every part begins at a multiple of 32 doubles (256 bytes).
struct PgLayout { size_t H, b, w, delta, X, Xn, edge, adj_start, adj, end; };

__host__ __device__ __forceinline__ size_t pg_round(size_t doubles) { return (doubles + 31) & ~(size_t)31; }

__host__ __device__ __forceinline__ PgLayout pg_layout(int n, int m)
{
    const size_t nn = n > 0 ? (size_t)n : 0, mm = m > 0 ? (size_t)m : 0, u = nn > 1 ? 6 * (nn - 1) : 0;
    PgLayout L;
    size_t at = 0;
    L.H = at; at += pg_round(u * u);
    L.b = at; at += pg_round(u);
    L.w = at; at += pg_round(u);
    L.delta = at; at += pg_round(u);
    L.X = at; at += pg_round(12 * nn);
    L.Xn = at; at += pg_round(12 * nn);
    L.edge = at; at += pg_round((size_t)PG_EDGE * mm);
    L.adj_start = at; at += pg_round((nn + 2) / 2);   // n + 1 ints
    L.adj = at; at += pg_round(mm);                   // 2 m ints
    L.end = at;
    return L;
}

struct PgWorkspace {
    unsigned long long* offset;   // (scenes) first double of the scene's slice
    double* slices;
    size_t slice_doubles;         // what the host laid out: a slice that would leave it is refused on the device (BAD_COUNTS)
    size_t bytes;
};

PgWorkspace carve(void* ws, int scenes, const int* node_starts_host, const int* edge_starts_host)
{
    size_t doubles = 0;
    for (int s = 0; s < scenes; ++s)
        doubles += pg_layout(node_starts_host[s + 1] - node_starts_host[s], edge_starts_host[s + 1] - edge_starts_host[s]).end;
    Carve c(ws);
    PgWorkspace w;
    w.offset = c.take<unsigned long long>((size_t)scenes);
    w.slices = c.take<double>(doubles);
    w.slice_doubles = doubles;
    w.bytes = c.bytes;
    return w;
}

struct PgIn {
    const int *node_starts, *edge_starts, *edge_i, *edge_j, *edge_uncertain;
    const float* edge_T;
    const double* edge_info;
    const float* init_poses;
    int total_nodes, total_edges;
};

struct PgParams { double mu, tau, step_tol, prune_threshold; int iterations; };

struct PgOut {
    float* poses; double* line_weight; int* pruned; int* steps; int* solves; double* objective; double* lambda; int* status;
    double *trace_scalars, *trace_poses, *trace_delta;
};

__global__ __launch_bounds__(PG_THREADS) void pg_status_kernel(PgIn in, PgWorkspace ws, int* __restrict__ status)
{
    __shared__ unsigned long long redu[4];
    __shared__ int red4[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    // the slices of the scenes before this one: an integer sum, so its order does not matter
    unsigned long long off = 0;
    for (int q = tid; q < s; q += PG_THREADS) {
        const int2 nr = starts_range(in.node_starts, q, in.total_nodes), er = starts_range(in.edge_starts, q, in.total_edges);
        off += pg_layout(nr.y - nr.x, er.y - er.x).end;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    if ((tid & 63) == 0) redu[tid >> 6] = off;
    __syncthreads();
    off = redu[0] + redu[1] + redu[2] + redu[3];
    const int2 nr = starts_range(in.node_starts, s, in.total_nodes), er = starts_range(in.edge_starts, s, in.total_edges);
    const int n = nr.y - nr.x, m = er.y - er.x;
    int bad = 0;
    for (int e = tid; e < m; e += PG_THREADS) {
        const int i = in.edge_i[er.x + e], j = in.edge_j[er.x + e];
        bad += (i < 0 || i >= n || j < 0 || j >= n || i == j);
    }
    bad = block_sum_i(bad, red4);
    if (tid == 0) {
        int st = 0;
        if (starts_bad(in.node_starts, s, in.total_nodes) || starts_bad(in.edge_starts, s, in.total_edges) || n > PG_MAX_NODES ||
            off + pg_layout(n, m).end > ws.slice_doubles)
            st |= ROITR_POSEGRAPH_BAD_COUNTS;
        if (n < 2) st |= ROITR_POSEGRAPH_ONE_NODE;   // alone: such a scene cannot have a valid edge
        else if (m == 0) st |= ROITR_POSEGRAPH_NO_EDGES;
        else if (bad) st |= ROITR_POSEGRAPH_BAD_EDGE;
        status[s] = st;
        ws.offset[s] = off;
    }
}

// [R^T | -R^T t] of S = [R | t] (rows of 4)
__device__ __forceinline__ void pg_inverse(const double (&S)[12], double (&I)[12])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) I[4 * r + c] = S[4 * c + r];
        I[4 * r + 3] = 0.0 - ((S[r] * S[3] + S[4 + r] * S[7]) + S[8 + r] * S[11]);
    }
}

// C = A B of two [R | t]
__device__ __forceinline__ void pg_mul(const double (&A)[12], const double (&B)[12], double (&C)[12])
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
            C[4 * r + c] = c == 3 ? v + A[4 * r + 3] : v;
        }
}

__device__ __forceinline__ void pg_six(const double (&D)[12], double (&xi)[6])
{
    xi[0] = (D[9] - D[6]) / 2.0;
    xi[1] = (D[2] - D[8]) / 2.0;
    xi[2] = (D[4] - D[1]) / 2.0;
    xi[3] = D[3]; xi[4] = D[7]; xi[5] = D[11];
}

__device__ __forceinline__ void pg_load12(const double* p, double (&S)[12])
{
#pragma unroll
    for (int k = 0; k < 12; ++k) S[k] = p[k];
}

// Edge e of the scene under the state Xs: A = T_e^-1 X_j^-1, xi, Lambda xi and e = xi . (Lambda xi)
__device__ __forceinline__ double pg_residual(const PgIn& in, int e0, int e, const double* Xs, double (&A)[12], double (&xi)[6],
                                              double (&Lxi)[6])
{
    const size_t g = (size_t)(e0 + e);
    const int i = in.edge_i[g], j = in.edge_j[g];
    double Te[12], Xi[12], Xj[12], Ti[12], Xji[12], D[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Te[k] = (double)in.edge_T[16 * g + k];
    pg_load12(Xs + 12 * (size_t)i, Xi);
    pg_load12(Xs + 12 * (size_t)j, Xj);
    pg_inverse(Te, Ti);
    pg_inverse(Xj, Xji);
    pg_mul(Ti, Xji, A);
    pg_mul(A, Xi, D);
    pg_six(D, xi);
    const double* Lm = in.edge_info + 36 * g;
    double en = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double v = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) v += Lm[6 * a + b] * xi[b];
        Lxi[a] = v;
        en += xi[a] * v;
    }
    return en;
}

// l_e and the edge's term of the objective
__device__ __forceinline__ double pg_line(bool uncertain, double en, double mu, double& term)
{
    if (!uncertain) { term = en; return 1.0; }
    const double r = mu / (mu + en), l = r * r, d = sqrt(l) - 1.0;
    term = l * en + mu * (d * d);
    return l;
}

// F of the state Xs (block sum, every thread gets it); line_weight / pruned: where to leave l_e and the pruning flag, or null
__device__ __forceinline__ double pg_objective(const PgIn& in, const PgParams& P, int e0, int m, const double* Xs, double* red,
                                               double* line_weight, int* pruned)
{
    double f[1] = {0.0};
    for (int e = threadIdx.x; e < m; e += PG_THREADS) {
        double A[12], xi[6], Lxi[6], term;
        const double en = pg_residual(in, e0, e, Xs, A, xi, Lxi);
        const bool unc = in.edge_uncertain[e0 + e] != 0;
        const double l = pg_line(unc, en, P.mu, term);
        f[0] += term;
        if (line_weight) line_weight[e0 + e] = l;
        if (pruned) pruned[e0 + e] = unc && l < P.prune_threshold;
    }
    block_sum_d<1>(f, red);
    return f[0];
}

__global__ __launch_bounds__(PG_THREADS) void pg_solve_kernel(PgIn in, PgParams P, PgWorkspace ws, PgOut o)
{
    __shared__ double sh_t[PG_MAX_U], sh_d[PG_MAX_U];
    __shared__ double red[4];
    __shared__ int sh_bad;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int2 nr = starts_range(in.node_starts, s, in.total_nodes), er = starts_range(in.edge_starts, s, in.total_edges);
    const int n0 = nr.x, n = nr.y - nr.x, e0 = er.x, m = er.y - er.x;
    const int iters = P.iterations;
    int st = o.status[s];
    double lambda = 0.0, nu = 2.0, F = 0.0;
    int steps = 0, solves = 0;
    double* X = nullptr;

    if (st == 0) {
        const PgLayout L = pg_layout(n, m);
        double* base = ws.slices + ws.offset[s];
        double *H = base + L.H, *bv = base + L.b, *wv = base + L.w, *dl = base + L.delta, *Xn = base + L.Xn, *E = base + L.edge;
        int *adj_start = reinterpret_cast<int*>(base + L.adj_start), *adj = reinterpret_cast<int*>(base + L.adj);
        X = base + L.X;
        const int u = 6 * (n - 1);
        const int* ei = in.edge_i + e0;
        const int* ej = in.edge_j + e0;
        for (int q = tid; q < 12 * n; q += PG_THREADS) X[q] = (double)in.init_poses[16 * (size_t)(n0 + q / 12) + q % 12];
        // adjacency: the edges of node k in ascending edge index, adj[adj_start[k] ... adj_start[k + 1])
        for (int k = tid; k < n; k += PG_THREADS) {
            int c = 0;
            for (int e = 0; e < m; ++e) c += (ei[e] == k) | (ej[e] == k);
            adj_start[k + 1] = c;
        }
        __syncthreads();
        if (tid == 0) {
            adj_start[0] = 0;
            for (int k = 0; k < n; ++k) adj_start[k + 1] += adj_start[k];
        }
        __syncthreads();
        for (int k = tid; k < n; k += PG_THREADS) {
            int at = adj_start[k];
            for (int e = 0; e < m; ++e)
                if ((ei[e] == k) | (ej[e] == k)) adj[at++] = e;
        }
        __syncthreads();

        bool first = true;
        for (int it = 0; it < iters; ++it) {
            // ---- edge terms at X.  Phase 1, thread per edge: A, xi, Lambda xi, l and the objective
            double f[1] = {0.0};
            for (int e = tid; e < m; e += PG_THREADS) {
                double A[12], xi[6], Lxi[6], term;
                const double en = pg_residual(in, e0, e, X, A, xi, Lxi);
                const double l = pg_line(in.edge_uncertain[e0 + e] != 0, en, P.mu, term);
                f[0] += term;
                double* Ee = E + (size_t)PG_EDGE * e;
#pragma unroll
                for (int k = 0; k < 12; ++k) Ee[PG_A + k] = A[k];
#pragma unroll
                for (int k = 0; k < 6; ++k) { Ee[PG_XI + k] = xi[k]; Ee[PG_LXI + k] = Lxi[k]; }
                Ee[PG_L] = l;
            }
            block_sum_d<1>(f, red);   // (its barriers also publish phase 1)
            F = f[0];
            // phase 2, thread per (edge, k): column k of J = the six-vector of A G_k X_i
            for (int q = tid; q < 6 * m; q += PG_THREADS) {
                const int e = q / 6, k = q % 6;
                double* Ee = E + (size_t)PG_EDGE * e;
                double A[12], Xi[12], B[12], C[12], col[6];
                pg_load12(Ee + PG_A, A);
                pg_load12(X + 12 * (size_t)ei[e], Xi);
#pragma unroll
                for (int c = 0; c < 12; ++c) B[c] = 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {   // [e_k]x applied to the rows of X_i
                    if (k == 0) { B[4 + c] = 0.0 - Xi[8 + c]; B[8 + c] = Xi[4 + c]; }
                    if (k == 1) { B[c] = Xi[8 + c]; B[8 + c] = 0.0 - Xi[c]; }
                    if (k == 2) { B[c] = 0.0 - Xi[4 + c]; B[4 + c] = Xi[c]; }
                }
                if (k >= 3) B[4 * (k - 3) + 3] = 1.0;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
                pg_six(C, col);
#pragma unroll
                for (int a = 0; a < 6; ++a) Ee[PG_J + 6 * a + k] = col[a];
            }
            __syncthreads();
            // phase 3, thread per (edge, a, c): Lambda J
            for (int q = tid; q < 36 * m; q += PG_THREADS) {
                const int e = q / 36, a = (q % 36) / 6, c = q % 6;
                double* Ee = E + (size_t)PG_EDGE * e;
                const double* Lm = in.edge_info + 36 * (size_t)(e0 + e);
                double v = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) v += Lm[6 * a + b] * Ee[PG_J + 6 * b + c];
                Ee[PG_LJ + 6 * a + c] = v;
            }
            __syncthreads();
            // phase 4, thread per (edge, r, c): M = l J^T (Lambda J); the first six of an edge also g = l J^T (Lambda xi)
            for (int q = tid; q < 36 * m; q += PG_THREADS) {
                const int e = q / 36, r = (q % 36) / 6, c = q % 6;
                double* Ee = E + (size_t)PG_EDGE * e;
                const double l = Ee[PG_L];
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 6; ++a) v += Ee[PG_J + 6 * a + r] * Ee[PG_LJ + 6 * a + c];
                Ee[PG_M + 6 * r + c] = l * v;
                if (r == 0) {
                    double g = 0.0;
#pragma unroll
                    for (int a = 0; a < 6; ++a) g += Ee[PG_J + 6 * a + c] * Ee[PG_LXI + a];
                    Ee[PG_G + c] = l * g;
                }
            }
            for (int q = tid; q < u * u; q += PG_THREADS) H[q] = 0.0;
            __syncthreads();
            // ---- assembly, every sum in ascending edge index.  Diagonal blocks and b: thread per (node, entry)
            for (int q = tid; q < 36 * (n - 1); q += PG_THREADS) {
                const int k = 1 + q / 36, r = (q % 36) / 6, c = q % 6;
                double v = 0.0, g = 0.0;
                for (int at = adj_start[k]; at < adj_start[k + 1]; ++at) {
                    const int e = adj[at];
                    const double* Ee = E + (size_t)PG_EDGE * e;
                    v += Ee[PG_M + 6 * r + c];
                    if (r == 0) g = ei[e] == k ? g + Ee[PG_G + c] : g - Ee[PG_G + c];
                }
                H[(size_t)(6 * (k - 1) + r) * u + 6 * (k - 1) + c] = v;
                if (r == 0) bv[6 * (k - 1) + c] = g;
            }
            // off-diagonal blocks: thread per (edge, entry); the first edge of a node pair gathers the pair's edges
            for (int q = tid; q < 36 * m; q += PG_THREADS) {
                const int e = q / 36, r = (q % 36) / 6, c = q % 6;
                const int hi = max(ei[e], ej[e]), lo = min(ei[e], ej[e]);
                if (lo == 0) continue;   // the gauge has no unknowns
                double v = 0.0;
                bool owner = true, seen = false;
                for (int at = adj_start[hi]; at < adj_start[hi + 1]; ++at) {
                    const int e2 = adj[at];
                    if (min(ei[e2], ej[e2]) != lo) continue;
                    if (!seen) { owner = e2 == e; seen = true; }
                    if (!owner) break;
                    v -= E[(size_t)PG_EDGE * e2 + PG_M + 6 * r + c];
                }
                if (!owner) continue;
                H[(size_t)(6 * (hi - 1) + r) * u + 6 * (lo - 1) + c] = v;
                H[(size_t)(6 * (lo - 1) + r) * u + 6 * (hi - 1) + c] = v;
            }
            __syncthreads();
            if (first) {
                double dmax = 0.0;
                for (int q = tid; q < u; q += PG_THREADS) dmax = fmax(dmax, H[(size_t)q * u + q]);
                lambda = P.tau * block_max_d(dmax, red);
                first = false;
            }
            // ---- L D L^T of H + lambda I with the right-hand side -b as row u; V[k][i] = H[k * u + i] (i < u) or wv[k] (i == u)
            if (tid == 0) sh_bad = 0;
            for (int j = 0; j < u; ++j) {
                for (int k = tid; k < j; k += PG_THREADS) sh_t[k] = H[(size_t)k * u + j] / sh_d[k];
                __syncthreads();
                for (int i = j + tid; i <= u; i += PG_THREADS) {
                    const double* col = i < u ? H + i : wv;
                    const size_t stride = i < u ? (size_t)u : 1;
                    double v = i < u ? H[(size_t)j * u + i] : 0.0 - bv[j];
                    if (i == j) v += lambda;
#pragma unroll 4
                    for (int k = 0; k < j; ++k) v -= col[k * stride] * sh_t[k];
                    if (i < u) H[(size_t)j * u + i] = v; else wv[j] = v;
                    if (i == j) {
                        sh_d[j] = v;
                        if (!(v > 0.0) || !isfinite(v)) sh_bad = 1;
                    }
                }
                __syncthreads();
                if (sh_bad) break;   // read between this barrier and the next: thread 0 writes it only behind the next one
            }
            __syncthreads();
            ++solves;
            const bool singular = sh_bad != 0;
            double maxd = 0.0, rho = 0.0, Fn = 0.0, den = 0.0;
            bool accepted = false, converged = false;
            if (!singular) {
                // back substitution, k descending: thread tid owns rows tid + 256 r
                double acc[PG_ROWS];
#pragma unroll
                for (int r = 0; r < PG_ROWS; ++r) acc[r] = tid + PG_THREADS * r < u ? wv[tid + PG_THREADS * r] : 0.0;
                for (int k = u - 1; k >= 0; --k) {
#pragma unroll
                    for (int r = 0; r < PG_ROWS; ++r)
                        if (tid + PG_THREADS * r == k) sh_t[k] = acc[r] / sh_d[k];
                    __syncthreads();
                    const double x = sh_t[k];
#pragma unroll
                    for (int r = 0; r < PG_ROWS; ++r) {
                        const int i = tid + PG_THREADS * r;
                        if (i < k) acc[r] -= H[(size_t)i * u + k] * x;
                    }
                }
                __syncthreads();
                double dd[1] = {0.0};
                for (int q = tid; q < u; q += PG_THREADS) {
                    const double x = sh_t[q];
                    dl[q] = x;
                    maxd = fmax(maxd, fabs(x));
                    dd[0] += x * (lambda * x - bv[q]);
                }
                maxd = block_max_d(maxd, red);
                block_sum_d<1>(dd, red);
                den = dd[0];
                converged = maxd < P.step_tol;
                if (!converged) {
                    for (int k = tid; k < n; k += PG_THREADS) {
                        double S[12], Sn[12];
                        pg_load12(X + 12 * (size_t)k, S);
                        if (k == 0) {
#pragma unroll
                            for (int c = 0; c < 12; ++c) Sn[c] = S[c];
                        } else {
                            const double* d6 = dl + 6 * (size_t)(k - 1);
                            const double x6[6] = {d6[0], d6[1], d6[2], d6[3], d6[4], d6[5]};
                            compose_step_d(x6, S, Sn);
                        }
#pragma unroll
                        for (int c = 0; c < 12; ++c) Xn[12 * (size_t)k + c] = Sn[c];
                    }
                    __syncthreads();
                    Fn = pg_objective(in, P, e0, m, Xn, red, nullptr, nullptr);
                    rho = (F - Fn) / den;
                    accepted = rho > 0.0;
                }
            }
            // the trace of this solve: the state before it, its delta, its scalars
            if (o.trace_poses)
                for (int q = tid; q < 12 * n; q += PG_THREADS)
                    o.trace_poses[((size_t)(n0 + q / 12) * iters + it) * 12 + q % 12] = X[q];
            if (o.trace_delta)
                for (int q = tid; q < 6 * n; q += PG_THREADS)
                    o.trace_delta[((size_t)(n0 + q / 6) * iters + it) * 6 + q % 6] = (q < 6 || singular) ? 0.0 : dl[q - 6];
            if (o.trace_scalars && tid == 0) {
                double* tr = o.trace_scalars + ((size_t)s * iters + it) * 8;
                tr[0] = F; tr[1] = lambda; tr[2] = rho; tr[3] = maxd; tr[4] = accepted ? 1.0 : 0.0; tr[5] = Fn; tr[6] = den; tr[7] = 1.0;
            }
            if (singular) { st |= ROITR_POSEGRAPH_SINGULAR; break; }
            if (converged) { st |= ROITR_POSEGRAPH_CONVERGED; break; }
            __syncthreads();   // the trace has read X
            if (accepted) {
                for (int q = tid; q < 12 * n; q += PG_THREADS) X[q] = Xn[q];
                ++steps;
                const double c = 2.0 * rho - 1.0;
                lambda *= fmax(1.0 / 3.0, 1.0 - c * c * c);
                nu = 2.0;
            } else {
                lambda *= nu;
                nu *= 2.0;
            }
            __syncthreads();
        }
        __syncthreads();
        F = pg_objective(in, P, e0, m, X, red, o.line_weight, o.pruned);
    } else {
        for (int e = tid; e < m; e += PG_THREADS) { o.line_weight[e0 + e] = 1.0; o.pruned[e0 + e] = 0; }
    }
    // the traces of what was not run
    for (int it = solves; it < iters; ++it) {
        if (o.trace_poses)
            for (int q = tid; q < 12 * n; q += PG_THREADS) o.trace_poses[((size_t)(n0 + q / 12) * iters + it) * 12 + q % 12] = 0.0;
        if (o.trace_delta)
            for (int q = tid; q < 6 * n; q += PG_THREADS) o.trace_delta[((size_t)(n0 + q / 6) * iters + it) * 6 + q % 6] = 0.0;
        if (o.trace_scalars && tid < 8) o.trace_scalars[((size_t)s * iters + it) * 8 + tid] = 0.0;
    }
    // poses: a node that never moved keeps the 16 floats it came with
    for (int q = tid; q < 16 * n; q += PG_THREADS) {
        const int k = q / 16, c = q % 16;
        const size_t at = 16 * (size_t)(n0 + k) + c;
        float v = in.init_poses[at];
        if (steps > 0 && k > 0) v = c < 12 ? (float)X[12 * (size_t)k + c] : (c == 15 ? 1.f : 0.f);
        o.poses[at] = v;
    }
    if (tid == 0) {
        o.steps[s] = steps;
        o.solves[s] = solves;
        o.objective[s] = F;
        o.lambda[s] = lambda;
        o.status[s] = st;
    }
}

bool finite_positive_d(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// the host copies: scenes + 1 entries from 0, never decreasing, no scene above the node limit
bool host_counts_ok(int scenes, const int* node_starts_host, const int* edge_starts_host)
{
    if (node_starts_host[0] != 0 || edge_starts_host[0] != 0) return false;
    for (int s = 0; s < scenes; ++s) {
        const long n = (long)node_starts_host[s + 1] - node_starts_host[s], m = (long)edge_starts_host[s + 1] - edge_starts_host[s];
        if (n < 0 || m < 0 || n > PG_MAX_NODES) return false;
    }
    return true;
}

}  // namespace

extern "C" int roitr_edge_information(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                                      const float* transforms, float radius, double* info, int* n_inlier, hipStream_t stream)
{
    if (!(radius > 0.f) || !(radius <= 3.402823466e38f))
        return refuse(ROITR_ERR_ARG, "roitr_edge_information: radius must be finite and positive");
    if (pairs <= 0) return ROITR_OK;
    if (total_rows < 0 || pairs > 65535) return refuse(ROITR_ERR_ARG, "roitr_edge_information: total_rows < 0 or pairs > 65535");
    if (!starts || !transforms || !info || !n_inlier || (total_rows > 0 && (!src_pts || !tgt_pts)))
        return refuse(ROITR_ERR_ARG, "roitr_edge_information: null pointer");
    edge_information_kernel<<<pairs, PG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, transforms, radius * radius, info,
                                                              n_inlier);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" size_t roitr_pose_graph_workspace_bytes(int scenes, const int* node_starts_host, const int* edge_starts_host)
{
    if (scenes <= 0 || scenes > 65535 || !node_starts_host || !edge_starts_host) return 0;
    if (!host_counts_ok(scenes, node_starts_host, edge_starts_host)) return 0;
    return carve(nullptr, scenes, node_starts_host, edge_starts_host).bytes;
}

extern "C" int roitr_pose_graph_batch(int scenes, const int* node_starts, const int* edge_starts, const int* node_starts_host,
                                      const int* edge_starts_host, const int* edge_i, const int* edge_j, const float* edge_T,
                                      const double* edge_info, const int* edge_uncertain, const float* init_poses, double mu, double tau,
                                      double step_tol, double prune_threshold, int iterations, void* workspace,
                                      size_t workspace_bytes_given, float* poses, double* line_weight, int* pruned, int* steps,
                                      int* solves, double* objective, double* lambda_out, int* status, double* trace_scalars,
                                      double* trace_poses, double* trace_delta, hipStream_t stream)
{
    if (!finite_positive_d(mu)) return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: mu must be finite and positive");
    if (!finite_positive_d(tau)) return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: tau must be finite and positive");
    if (!(step_tol >= 0.0) || !(step_tol <= 1.7976931348623157e308))
        return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: step_tol must be finite and not negative");
    if (!(prune_threshold >= 0.0) || !(prune_threshold <= 1.0))
        return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: prune_threshold outside 0 ... 1");
    if (iterations < 0 || iterations > PG_MAX_ITERATIONS) return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: iterations outside 0 ... 1024");
    if (scenes <= 0) return ROITR_OK;
    if (scenes > 65535) return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: more than 65535 scenes");
    if (!node_starts || !edge_starts || !node_starts_host || !edge_starts_host || !poses || !steps || !solves || !objective || !lambda_out ||
        !status)
        return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: null pointer");
    if (!host_counts_ok(scenes, node_starts_host, edge_starts_host))
        return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: host starts do not begin at 0, decrease, or a scene has more than 256 nodes");
    const int total_nodes = node_starts_host[scenes], total_edges = edge_starts_host[scenes];
    if ((total_nodes > 0 && !init_poses) ||
        (total_edges > 0 && (!edge_i || !edge_j || !edge_T || !edge_info || !edge_uncertain || !line_weight || !pruned)))
        return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: null pointer");
    const PgWorkspace ws = carve(workspace, scenes, node_starts_host, edge_starts_host);
    if (workspace_bytes_given < ws.bytes || !workspace)
        return refuse(ROITR_ERR_ARG, "roitr_pose_graph_batch: workspace smaller than roitr_pose_graph_workspace_bytes()");
    const PgIn in = {node_starts, edge_starts, edge_i, edge_j, edge_uncertain, edge_T, edge_info, init_poses, total_nodes, total_edges};
    const PgParams P = {mu, tau, step_tol, prune_threshold, iterations};
    const PgOut o = {poses, line_weight, pruned, steps, solves, objective, lambda_out, status, trace_scalars, trace_poses, trace_delta};
    pg_status_kernel<<<scenes, PG_THREADS, 0, stream>>>(in, ws, status);
    ROITR_LAUNCH_CHECK();
    pg_solve_kernel<<<scenes, PG_THREADS, 0, stream>>>(in, P, ws, o);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
