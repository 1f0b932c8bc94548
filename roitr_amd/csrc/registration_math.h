// Scalar pieces of the correspondence RANSAC (registration.hip), host and device alike: the counter-based random stream, the
// triple draw, Open3D's two correspondence checkers as the reference calls them, the degenerate-triangle test, the rigid
// solve (Horn's quaternion form of Kabsch / Umeyama, float64) and the fp32 residual.  Kept free of kernel code so that one
// definition serves the hypothesis kernel, the reduce / refit kernel and the sample dump.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define RG_HD __host__ __device__ __forceinline__

// ------------------------------------------------------------------ random stream
// splitmix64 finaliser (Steele, Lea, Flood 2014).
RG_HD uint64_t rg_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Hypothesis draws: counter c = key << 32 | iteration << 4 | draw (iteration < 2^28, draw < 16),
// u = high 32 bits of splitmix64(seed ^ splitmix64(c)), index = (u * n) >> 32.
RG_HD int rg_draw(uint64_t seed, uint32_t key, uint32_t it, uint32_t d, int n)
{
    const uint64_t c = ((uint64_t)key << 32) | ((uint64_t)it << 4) | (uint64_t)d;
    const uint32_t u = (uint32_t)(rg_splitmix64(seed ^ rg_splitmix64(c)) >> 32);
    return (int)(((uint64_t)u * (uint64_t)(uint32_t)n) >> 32);
}

// Selection keys (weighted mode): their own domain of the same generator.  Row j (local index in the pair):
// u = high 32 bits of splitmix64(seed ^ RG_SEL_DOMAIN ^ splitmix64(key << 32 | j)), v = (u + 0.5) / 2^32 in (0, 1).
#define RG_SEL_DOMAIN 0xA0761D6478BD642Full
RG_HD double rg_select_uniform(uint64_t seed, uint32_t key, uint32_t j)
{
    const uint64_t c = ((uint64_t)key << 32) | (uint64_t)j;
    const uint32_t u = (uint32_t)(rg_splitmix64(seed ^ RG_SEL_DOMAIN ^ rg_splitmix64(c)) >> 32);
    return ((double)u + 0.5) * (1.0 / 4294967296.0);
}

// The triple of iteration `it`: draws d = 0, 1, ..., 15 in order; a draw equal to an index already taken is skipped; the first
// three distinct indices form the triple.  Returns false (iteration invalid) when draw 15 passes without three.
RG_HD bool rg_triple(uint64_t seed, uint32_t key, uint32_t it, int n, int& i0, int& i1, int& i2)
{
    int a = -1, b = -1, c = -1;   // scalars and selects only: an indexed "slot[got] = x" would live in scratch
#pragma unroll
    for (uint32_t d = 0; d < 16; ++d) {
        const int x = rg_draw(seed, key, it, d, n);
        const bool ta = a < 0, tb = !ta && b < 0 && x != a, tc = !ta && b >= 0 && c < 0 && x != a && x != b;
        a = ta ? x : a;
        b = tb ? x : b;
        c = tc ? x : c;
    }
    i0 = a; i1 = b; i2 = c;
    return c >= 0;
}

// ------------------------------------------------------------------ checkers (float64 on fp32 inputs)
RG_HD double rg_len(double ax, double ay, double az, double bx, double by, double bz)
{
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// Open3D CorrespondenceCheckerBasedOnEdgeLength(sim) as the reference calls it: reject when, for a sample pair i, j,
// |s_i - s_j| < sim |t_i - t_j| or |t_i - t_j| < sim |s_i - s_j|.
RG_HD bool rg_edge_ok(const double (&s)[9], const double (&t)[9], double sim)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i + 1; j < 3; ++j) {
            const double ds = rg_len(s[3 * i], s[3 * i + 1], s[3 * i + 2], s[3 * j], s[3 * j + 1], s[3 * j + 2]);
            const double dt = rg_len(t[3 * i], t[3 * i + 1], t[3 * i + 2], t[3 * j], t[3 * j + 1], t[3 * j + 2]);
            ok = ok && !(ds < dt * sim) && !(dt < ds * sim);
        }
    }
    return ok;
}

// Degenerate triangle: |a x b|^2 <= 1e-12 |a|^2 |b|^2 with a = p1 - p0, b = p2 - p0 (sine of the angle at p0 at most 1e-6, which
// covers duplicate points: a or b = 0), in the source or in the target triangle.
#define RG_DEGENERATE_SIN2 1e-12
RG_HD bool rg_triangle_ok(const double (&p)[9])
{
    const double ax = p[3] - p[0], ay = p[4] - p[1], az = p[5] - p[2];
    const double bx = p[6] - p[0], by = p[7] - p[1], bz = p[8] - p[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double c2 = cx * cx + cy * cy + cz * cz;
    const double a2 = ax * ax + ay * ay + az * az, b2 = bx * bx + by * by + bz * bz;
    return c2 > RG_DEGENERATE_SIN2 * a2 * b2;
}

// ------------------------------------------------------------------ rigid solve
// R maximising sum w (t_c . R s_c) for the cross-covariance H[a][b] = sum w s_c[a] t_c[b], restricted to rotations: the unit
// quaternion of the largest eigenvalue of Horn's 4x4 matrix (cyclic Jacobi in float64).  This is the Kabsch / Umeyama rotation
// V diag(1, 1, sign det(V U^T)) U^T of H = U S V^T wherever that one is unique.  Then t = ct - R cs; T = [R | t] row-major 3x4.
RG_HD void rg_jacobi_rot(double (&A)[4][4], double (&V)[4][4], int p, int q)
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // A <- A J
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // A <- J^T A
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // V <- V J
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

RG_HD void rg_solve_rigid(const double (&H)[9], const double (&cs)[3], const double (&ct)[3], float (&T)[12])
{
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
        const double dia = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]) + fabs(A[3][3]);
        if (!(off > 1e-300) || off <= 1e-17 * dia) break;
        rg_jacobi_rot(A, V, 0, 1); rg_jacobi_rot(A, V, 0, 2); rg_jacobi_rot(A, V, 0, 3);
        rg_jacobi_rot(A, V, 1, 2); rg_jacobi_rot(A, V, 1, 3); rg_jacobi_rot(A, V, 2, 3);
    }
    // largest eigenvalue, first one on ties; its column as a 0 / 1 blend (a select of columns becomes a runtime-indexed load)
    const bool g1 = A[1][1] > A[0][0];
    const double b01 = g1 ? A[1][1] : A[0][0];
    const bool g2 = A[2][2] > b01;
    const double b012 = g2 ? A[2][2] : b01;
    const bool g3 = A[3][3] > b012;
    const double m3 = g3 ? 1.0 : 0.0, m2 = (!g3 && g2) ? 1.0 : 0.0, m1 = (!g3 && !g2 && g1) ? 1.0 : 0.0;
    const double m0 = 1.0 - m1 - m2 - m3;
    double w = m0 * V[0][0] + m1 * V[0][1] + m2 * V[0][2] + m3 * V[0][3];
    double x = m0 * V[1][0] + m1 * V[1][1] + m2 * V[1][2] + m3 * V[1][3];
    double y = m0 * V[2][0] + m1 * V[2][1] + m2 * V[2][2] + m3 * V[2][3];
    double z = m0 * V[3][0] + m1 * V[3][1] + m2 * V[3][2] + m3 * V[3][3];
    const double nq = sqrt(w * w + x * x + y * y + z * z);
    w /= nq; x /= nq; y /= nq; z /= nq;
    const double R[9] = {w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double tr = ct[r] - (R[3 * r] * cs[0] + R[3 * r + 1] * cs[1] + R[3 * r + 2] * cs[2]);
        T[4 * r] = (float)R[3 * r]; T[4 * r + 1] = (float)R[3 * r + 1]; T[4 * r + 2] = (float)R[3 * r + 2]; T[4 * r + 3] = (float)tr;
    }
}

// Unweighted three-point solve (the hypothesis of a triple).
RG_HD void rg_solve3(const double (&s)[9], const double (&t)[9], float (&T)[12])
{
    double cs[3], ct[3], H[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cs[a] = (s[a] + s[3 + a] + s[6 + a]) / 3.0;
        ct[a] = (t[a] + t[3 + a] + t[6 + a]) / 3.0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            H[3 * a + b] = (s[a] - cs[a]) * (t[b] - ct[b]) + (s[3 + a] - cs[a]) * (t[3 + b] - ct[b]) + (s[6 + a] - cs[a]) * (t[6 + b] - ct[b]);
    rg_solve_rigid(H, cs, ct, T);
}

// ------------------------------------------------------------------ fp32 residual
// d^2 = || R s + t - g ||^2 in fp32, one fixed FMA order (the counting, the distance checker and the refit all use it).
RG_HD float rg_dist2(const float (&T)[12], float sx, float sy, float sz, float gx, float gy, float gz)
{
    const float px = fmaf(T[2], sz, fmaf(T[1], sy, fmaf(T[0], sx, T[3])));
    const float py = fmaf(T[6], sz, fmaf(T[5], sy, fmaf(T[4], sx, T[7])));
    const float pz = fmaf(T[10], sz, fmaf(T[9], sy, fmaf(T[8], sx, T[11])));
    const float dx = px - gx, dy = py - gy, dz = pz - gz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// The hypothesis of iteration `it` on the n selected rows (s4 / t4: x, y, z, weight): triple, edge checker (sim), degenerate
// test, solve, distance checker (every sample within thr: d^2 <= thr^2).  Returns whether it passed; T is set when it did.
RG_HD bool rg_hypothesis(uint64_t seed, uint32_t key, uint32_t it, int n, const float4* s4, const float4* t4, float thr2, double sim,
                         float (&T)[12])
{
    int i0, i1, i2;
    if (!rg_triple(seed, key, it, n, i0, i1, i2)) return false;
    const float4 a0 = s4[i0], a1 = s4[i1], a2 = s4[i2], b0 = t4[i0], b1 = t4[i1], b2 = t4[i2];
    const double s[9] = {a0.x, a0.y, a0.z, a1.x, a1.y, a1.z, a2.x, a2.y, a2.z};
    const double t[9] = {b0.x, b0.y, b0.z, b1.x, b1.y, b1.z, b2.x, b2.y, b2.z};
    if (!rg_edge_ok(s, t, sim) || !rg_triangle_ok(s) || !rg_triangle_ok(t)) return false;
    rg_solve3(s, t, T);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        ok = ok && rg_dist2(T, (float)s[3 * k], (float)s[3 * k + 1], (float)s[3 * k + 2], (float)t[3 * k], (float)t[3 * k + 1],
                            (float)t[3 * k + 2]) <= thr2;
    return ok;
}
