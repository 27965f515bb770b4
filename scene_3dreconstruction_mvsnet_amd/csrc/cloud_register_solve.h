// cloud_register_solve.h -- the small dense algebra of mvs_cloud_register's step (include/ext/mvs_register_abi.h): the
// LDL^T solve of the point-to-plane system, Horn's quaternion for the point-to-point rotation, the 6-vector to matrix and
// the 4 x 4 product.  Plain C++, __host__ __device__: cloud_register.hip runs it in a one-thread kernel, and
// tests/register_solve_host.cpp runs the very same code on the host.
//
// Nothing here keeps an array of its own that it indexes with a variable: every array is the caller's (the kernel hands
// over shared memory), so the device code needs no scratch.  One operation at a time; the users compile with
// -ffp-contract=off.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MVS_SOLVE_HD __host__ __device__
#else
#define MVS_SOLVE_HD
#endif

namespace mvs {

constexpr int kRegisterJacobiSweeps = 10;      // MVS_REGISTER_JACOBI_SWEEPS

MVS_SOLVE_HD inline bool solve_finite(double v) { return std::fabs(v) < INFINITY; }      // false for NaN

// A x = -b for the symmetric 6 x 6 A, whose upper triangle is read from a[36] (row-major).  LDL^T without pivoting, in
// place: afterwards a[j][j] = d[j] and a[i][j] = L[i][j] for i > j.
//     d[j]    = A[j][j] - sum_{m<j} (L[j][m] * L[j][m]) * d[m]                 m ascending
//     L[i][j] = (A[j][i] - sum_{m<j} (L[i][m] * L[j][m]) * d[m]) / d[j]        i > j
//     y[i] = -b[i] - sum_{m<i} L[i][m] * y[m];   z[i] = y[i] / d[i];   x[i] = z[i] - sum_{m>i} L[m][i] * x[m], i descending
// false, with x untouched, as soon as a pivot d[j] is not > 0 or not finite.
MVS_SOLVE_HD inline bool register_ldlt6(double* a, const double* b, double* x) {
    for (int j = 0; j < 6; ++j) {
        double d = a[j * 6 + j];
        for (int m = 0; m < j; ++m) d = d - (a[j * 6 + m] * a[j * 6 + m]) * a[m * 6 + m];
        if (!(d > 0.0) || !solve_finite(d)) return false;
        a[j * 6 + j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double l = a[j * 6 + i];
            for (int m = 0; m < j; ++m) l = l - (a[i * 6 + m] * a[j * 6 + m]) * a[m * 6 + m];
            a[i * 6 + j] = l / d;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double y = -b[i];
        for (int m = 0; m < i; ++m) y = y - a[i * 6 + m] * x[m];
        x[i] = y;
    }
    for (int i = 0; i < 6; ++i) x[i] = x[i] / a[i * 6 + i];
    for (int i = 5; i >= 0; --i) {
        double z = x[i];
        for (int m = i + 1; m < 6; ++m) z = z - a[m * 6 + i] * x[m];
        x[i] = z;
    }
    return true;
}

// Open3D's TransformVector6dToMatrix4d: x = (alpha, beta, gamma, tx, ty, tz) -> T[16], row-major, with the rotation
// Rz(gamma) * Ry(beta) * Rx(alpha) written out
MVS_SOLVE_HD inline void register_vector6_to_matrix(const double* x, double* T) {
    const double ca = std::cos(x[0]), sa = std::sin(x[0]), cb = std::cos(x[1]), sb = std::sin(x[1]);
    const double cg = std::cos(x[2]), sg = std::sin(x[2]);
    T[0] = cg * cb;
    T[1] = (cg * sb) * sa - sg * ca;
    T[2] = (cg * sb) * ca + sg * sa;
    T[4] = sg * cb;
    T[5] = (sg * sb) * sa + cg * ca;
    T[6] = (sg * sb) * ca - cg * sa;
    T[8] = -sb;
    T[9] = cb * sa;
    T[10] = cb * ca;
    T[3] = x[3];
    T[7] = x[4];
    T[11] = x[5];
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// C = A * B for two rigid 4 x 4 matrices (last rows 0 0 0 1, which is what C's is set to); C aliases neither
MVS_SOLVE_HD inline void register_compose(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            C[i * 4 + j] = ((A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j]) + A[i * 4 + 2] * B[8 + j]) + A[i * 4 + 3] * B[12 + j];
    C[12] = C[13] = C[14] = 0.0;
    C[15] = 1.0;
}

// The rotation R[9] (row-major) that brings the source onto the target in the least-squares sense, from the
// cross-covariance S[9], S[3a + b] = sum of source[a] * target[b] (any positive multiple of it): Horn's closed form.
//     N = [ Sxx+Syy+Szz   Syz-Szy        Szx-Sxz        Sxy-Syx
//           .             Sxx-Syy-Szz    Sxy+Syx        Szx+Sxz
//           .             .             -Sxx+Syy-Szz    Syz+Szy
//           .             .              .             -Sxx-Syy+Szz ]     each entry summed left to right
// kRegisterJacobiSweeps cyclic Jacobi sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) in that order; a pair whose
// off-diagonal entry is exactly 0 is skipped; else theta = (n_qq - n_pp) / (2 * n_pq), t = sign(theta) / (|theta| +
// sqrt(theta * theta + 1)), c = 1 / sqrt(t * t + 1), s = t * c, and rows / columns p, q of N and columns p, q of V (from
// the identity) are rotated.  The quaternion (w, x, y, z) is the column of V under the largest diagonal entry (the first
// of equals), divided by its norm; R is the matrix of that unit quaternion.  n[16] and v[16] are the caller's.
// false if N has an entry that is not finite or the column's norm is not a positive finite number.
MVS_SOLVE_HD inline bool register_horn(const double* S, double* n, double* v, double* R) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    n[0] = (Sxx + Syy) + Szz;
    n[1] = n[4] = Syz - Szy;
    n[2] = n[8] = Szx - Sxz;
    n[3] = n[12] = Sxy - Syx;
    n[5] = (Sxx - Syy) - Szz;
    n[6] = n[9] = Sxy + Syx;
    n[7] = n[13] = Szx + Sxz;
    n[10] = (-Sxx + Syy) - Szz;
    n[11] = n[14] = Syz + Szy;
    n[15] = (-Sxx - Syy) + Szz;
    for (int i = 0; i < 16; ++i) {
        if (!solve_finite(n[i])) return false;
        v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < kRegisterJacobiSweeps; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = n[p * 4 + q];
                if (apq == 0.0) continue;
                const double theta = (n[q * 4 + q] - n[p * 4 + p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {      // columns p, q: N <- N J
                    const double kp = n[k * 4 + p], kq = n[k * 4 + q];
                    n[k * 4 + p] = c * kp - s * kq;
                    n[k * 4 + q] = s * kp + c * kq;
                }
                for (int k = 0; k < 4; ++k) {      // rows p, q: N <- J^T N
                    const double pk = n[p * 4 + k], qk = n[q * 4 + k];
                    n[p * 4 + k] = c * pk - s * qk;
                    n[q * 4 + k] = s * pk + c * qk;
                }
                for (int k = 0; k < 4; ++k) {      // V <- V J
                    const double kp = v[k * 4 + p], kq = v[k * 4 + q];
                    v[k * 4 + p] = c * kp - s * kq;
                    v[k * 4 + q] = s * kp + c * kq;
                }
            }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (n[i * 4 + i] > n[best * 4 + best]) best = i;
    double w = v[best], x = v[4 + best], y = v[8 + best], z = v[12 + best];
    const double norm = std::sqrt(((w * w + x * x) + y * y) + z * z);
    if (!(norm > 0.0) || !solve_finite(norm)) return false;
    w = w / norm;
    x = x / norm;
    y = y / norm;
    z = z / norm;
    R[0] = ((w * w + x * x) - y * y) - z * z;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = ((w * w - x * x) + y * y) - z * z;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = ((w * w - x * x) - y * y) + z * z;
    return true;
}

// the point-to-point step: sums[] are the reduced terms of the header (3..5 the source sums, 6..8 the target sums,
// 9..17 the products, all about the origin o), n = n_inliers >= 1 -> dT[16].  work[50]: S (9), N (16), V (16), R (9)
MVS_SOLVE_HD inline bool register_point_step(const double* sums, double n, const double* o, double* work, double* dT) {
    double* S = work;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) S[3 * a + b] = sums[9 + 3 * a + b] - (sums[3 + a] * sums[6 + b]) / n;
    double* R = work + 41;
    if (!register_horn(S, work + 9, work + 25, R)) return false;
    for (int a = 0; a < 3; ++a) {
        // t = (mq + o) - R (ms + o)
        const double c0 = sums[3] / n + o[0], c1 = sums[4] / n + o[1], c2 = sums[5] / n + o[2];
        const double rc = (R[3 * a] * c0 + R[3 * a + 1] * c1) + R[3 * a + 2] * c2;
        dT[4 * a] = R[3 * a];
        dT[4 * a + 1] = R[3 * a + 1];
        dT[4 * a + 2] = R[3 * a + 2];
        dT[4 * a + 3] = (sums[6 + a] / n + o[a]) - rc;
    }
    dT[12] = dT[13] = dT[14] = 0.0;
    dT[15] = 1.0;
    return true;
}

// the point-to-plane step: A from terms 3..23, b = terms 24..29 -> dT[16].  work[42]: A (36), x (6)
MVS_SOLVE_HD inline bool register_plane_step(const double* sums, double* work, double* dT) {
    double* A = work;
    int t = 3;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) A[a * 6 + b] = A[b * 6 + a] = sums[t++];
    double* x = work + 36;
    if (!register_ldlt6(A, sums + 24, x)) return false;
    register_vector6_to_matrix(x, dT);
    return true;
}

constexpr int kRegisterSolveWork = 50;      // doubles of `work` above, the larger of the two

}  // namespace mvs
