// cloud_planes_fit.h -- the least-squares plane of mvs_cloud_planes (include/ext/mvs_planes_abi.h) from the nine sums over
// a candidate's inliers: mean, covariance, the eigenvector of the smallest eigenvalue by cyclic Jacobi sweeps (the
// rotation, the order and the count of cloud_normals.hip, restated here because that file's copy lives inside a kernel),
// the sign, and the candidate's own plane where the fit is not finite.  Plain C++, __host__ __device__:
// cloud_planes.hip runs it in a one-thread kernel, and tests/planes_fit_host.cpp runs the very same code on the host.
// One operation at a time; the users compile with -ffp-contract=off.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MVS_FIT_HD __host__ __device__
#else
#define MVS_FIT_HD
#endif

namespace mvs {

constexpr int kPlanesJacobiSweeps = 8;      // MVS_PLANES_JACOBI_SWEEPS
constexpr int kPlanesSums = 9;              // q0 q1 q2, q0q0 q0q1 q0q2 q1q1 q1q2 q2q2
constexpr int kPlanesCand = 8;              // doubles of a candidate: n0 n1 n2 d0 thr q^0_0 q^0_1 q^0_2

MVS_FIT_HD inline bool fit_finite(double v) { return std::fabs(v) < INFINITY; }      // false for NaN

// one Jacobi rotation that zeroes A[p][q] of the symmetric A (its third index is r), accumulated into the columns of V
MVS_FIT_HD inline void fit_rotate(double A[3][3], double V[3][3], int p, int q, int r) {
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
    A[p][p] = A[p][p] - t * apq;
    A[q][q] = A[q][q] + t * apq;
    A[p][q] = A[q][p] = 0.0;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

// the header's Sign, and d: n is a unit normal, c a point of the plane; plane = (n, d).  false if d is not finite
MVS_FIT_HD inline bool fit_orient(const double n[3], const double c[3], const double* toward, double plane[4]) {
    const double a0 = std::fabs(n[0]), a1 = std::fabs(n[1]), a2 = std::fabs(n[2]);
    const double big = a0 >= a1 && a0 >= a2 ? n[0] : a1 >= a2 ? n[1] : n[2];
    const bool flip = big < 0.0;
    for (int a = 0; a < 3; ++a) plane[a] = flip ? -n[a] : n[a];
    plane[3] = -((plane[0] * c[0] + plane[1] * c[1]) + plane[2] * c[2]);
    if (toward && ((plane[0] * toward[0] + plane[1] * toward[1]) + plane[2] * toward[2]) + plane[3] < 0.0)
        for (int a = 0; a < 4; ++a) plane[a] = -plane[a];
    return fit_finite(plane[3]);
}

// the least-squares plane of the sums over m inliers about the origin o -> plane[4]; false where the header falls back
MVS_FIT_HD inline bool fit_least_squares(const double* sums, double m, const double* o, const double* toward,
                                         double plane[4]) {
    double mean[3], A[3][3];
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
        mean[a] = sums[a] / m;
        ok = ok && fit_finite(mean[a]);
    }
    int k = 3;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            A[a][b] = A[b][a] = sums[k++] / m - mean[a] * mean[b];
            ok = ok && fit_finite(A[a][b]);
        }
    if (!ok) return false;
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kPlanesJacobiSweeps; ++sweep) {
        fit_rotate(A, V, 0, 1, 2);
        fit_rotate(A, V, 0, 2, 1);
        fit_rotate(A, V, 1, 2, 0);
    }
    const bool use1 = A[1][1] < A[0][0];
    const double l01 = use1 ? A[1][1] : A[0][0];
    const bool use2 = A[2][2] < l01;
    double v[3];
    for (int a = 0; a < 3; ++a) v[a] = use2 ? V[a][2] : use1 ? V[a][1] : V[a][0];
    const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(len > 0.0) || !fit_finite(len)) return false;
    double n[3], c[3];
    for (int a = 0; a < 3; ++a) {
        n[a] = v[a] / len;
        c[a] = mean[a] + o[a];
    }
    return fit_orient(n, c, toward, plane);
}

// the plane of round r: the least-squares fit, else the candidate's own plane (cand: n0 n1 n2 d0 thr q^0).
// -> 1: the fit, 0: the candidate's
MVS_FIT_HD inline int planes_fit(const double* sums, double m, const double* o, const double* toward, const double* cand,
                                 double plane[4]) {
    if (fit_least_squares(sums, m, o, toward, plane)) return 1;
    const double nn = (cand[0] * cand[0] + cand[1] * cand[1]) + cand[2] * cand[2];
    const double len = std::sqrt(nn);
    double n[3], c[3];
    for (int a = 0; a < 3; ++a) {
        n[a] = cand[a] / len;
        c[a] = cand[5 + a] + o[a];
    }
    fit_orient(n, c, toward, plane);
    return 0;
}

}  // namespace mvs
