// The two pieces of a 6-parameter Gauss-Newton step that the ICP family (icp_common.h) and fast global registration (fgr.hip) share:
// the 6x6 L D L^T solve and the composition of a step with a state.  Moved out of icp_common.h unchanged, so that a source that needs
// only them does not get the ICP kernels along.  Like icp_common.h, include it AFTER `#pragma clang fp contract(off)`: every product
// and sum is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace {

// x of (L D L^T) x = b for the symmetric 6x6 A (upper triangle, row-major, 21 values); false on a non-positive or non-finite pivot
__device__ __forceinline__ bool ldl_solve6(const double* A21, const double (&rhs)[6], double (&x)[6])
{
    double A[6][6], L[6][6], d[6];
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { A[i][j] = A21[at]; A[j][i] = A21[at]; ++at; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= L[j][k] * L[j][k] * d[k];
        ok = ok && v > 0.0 && isfinite(v);
        d[j] = v;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) w -= L[i][k] * L[j][k] * d[k];
            L[i][j] = w / v;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v;
    }
    return ok;
}

// T_next = fp32(dT T) with dT = [Rz(g) Ry(b) Rx(a) | t] of x = (a, b, g, tx, ty, tz): Open3D's TransformVector6dToMatrix4d
__device__ __forceinline__ void compose_step(const double (&x)[6], const float (&T)[12], float (&Tn)[12])
{
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                         -sb, cb * sa, cb * ca};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = R[3 * r] * (double)T[c] + R[3 * r + 1] * (double)T[4 + c] + R[3 * r + 2] * (double)T[8 + c];
            Tn[4 * r + c] = (float)(c == 3 ? v + x[3 + r] : v);
        }
}

// The same dT applied to a float64 state S = [R | t] (rows of 4), without the rounding to fp32: fgr.hip keeps its state in float64
__device__ __forceinline__ void compose_step_d(const double (&x)[6], const double (&S)[12], double (&Sn)[12])
{
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                         -sb, cb * sa, cb * ca};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = R[3 * r] * S[c] + R[3 * r + 1] * S[4 + c] + R[3 * r + 2] * S[8 + c];
            Sn[4 * r + c] = c == 3 ? v + x[3 + r] : v;
        }
}

}  // namespace
