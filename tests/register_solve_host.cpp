// register_solve_host.cpp -- csrc/cloud_register_solve.h as host C++: the very code mvs_cloud_register's one-thread
// kernel runs, built with the address and undefined-behaviour sanitizers by tests/test_cloud_register_host.py.  No GPU,
// nothing loaded into Python.
//
// It makes its own seeded cases and prints every input and every result as hexadecimal doubles, one case per line:
//     ldlt    A (36) b (6)        -> ok x (6)            seeded J^T J systems, near-singular ones, singular ones
//     horn    S (9)               -> ok R (9)            covariances of point sets under rotations up to 179 degrees,
//                                                        of mirrored sets (Kabsch needs its determinant fix there), of
//                                                        planar and collinear sets
//     vec6    x (6)               -> T (16)
//     compose A (16) B (16)       -> C (16)
//     point   sums (31) o (3)     -> ok dT (16)
//     plane   sums (31)           -> ok dT (16)
// The host test checks each line against numpy within the bounds of tests/register_ref.py.
#include "cloud_register_solve.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

struct Rng {      // SplitMix64: the same stream everywhere
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uniform(double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 11) * 0x1p-53); }
};

void put(const char* tag, const double* v, int n) {
    std::printf("%s", tag);
    for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
}

void ldlt_case(Rng& rng, int rows, double squeeze) {
    // A = J^T J over `rows` rows of J; `squeeze` scales the last column towards a copy of the first
    double A[36] = {0}, b[6] = {0}, x[6] = {0}, keep[36];
    for (int r = 0; r < rows; ++r) {
        double J[6];
        for (int a = 0; a < 6; ++a) J[a] = rng.uniform(-1.0, 1.0);
        J[5] = J[0] + squeeze * J[5];
        const double res = rng.uniform(-0.1, 0.1);
        for (int a = 0; a < 6; ++a) {
            for (int c = 0; c < 6; ++c) A[a * 6 + c] += J[a] * J[c];
            b[a] += J[a] * res;
        }
    }
    for (int i = 0; i < 36; ++i) keep[i] = A[i];
    const bool ok = mvs::register_ldlt6(A, b, x);
    put("ldlt", keep, 36);
    put("", b, 6);
    std::printf(" -> %d", ok ? 1 : 0);
    put("", x, 6);
    std::printf("\n");
}

void rotation(double ax, double ay, double az, double angle, double* R) {
    const double n = std::sqrt(ax * ax + ay * ay + az * az);
    const double x = ax / n, y = ay / n, z = az / n, c = std::cos(angle), s = std::sin(angle), t = 1.0 - c;
    const double M[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c,
                         t * y * z - s * x, t * x * z - s * y, t * y * z + s * x, t * z * z + c};
    for (int i = 0; i < 9; ++i) R[i] = M[i];
}

// kind 0: a cloud in space; 1: mirrored in x before the rotation; 2: planar (z = 0); 3: collinear
void horn_case(Rng& rng, double degrees, int kind, double noise) {
    double Rt[9], S[9] = {0}, ms[3] = {0}, mq[3] = {0};
    rotation(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1) + 1.5, degrees * 3.14159265358979323846 / 180.0, Rt);
    const int n = 200;
    std::vector<double> s(3 * n), q(3 * n);
    for (int i = 0; i < n; ++i) {
        double p[3] = {rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(-1, 1)};
        if (kind == 2) p[2] = 0.0;
        if (kind == 3) p[1] = p[2] = 0.0;
        for (int a = 0; a < 3; ++a) s[3 * i + a] = p[a];
        if (kind == 1) p[0] = -p[0];
        for (int a = 0; a < 3; ++a)
            q[3 * i + a] = Rt[3 * a] * p[0] + Rt[3 * a + 1] * p[1] + Rt[3 * a + 2] * p[2] + rng.uniform(-noise, noise);
        for (int a = 0; a < 3; ++a) {
            ms[a] += s[3 * i + a] / n;
            mq[a] += q[3 * i + a] / n;
        }
    }
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) S[3 * a + c] += (s[3 * i + a] - ms[a]) * (q[3 * i + c] - mq[c]);
    double N[16], V[16], R[9] = {0};
    const bool ok = mvs::register_horn(S, N, V, R);
    put("horn", S, 9);
    std::printf(" -> %d", ok ? 1 : 0);
    put("", R, 9);
    std::printf("\n");
}

// the reduced sums of a cloud of n correspondences under a small motion, as the kernel would hand them over
void step_case(Rng& rng, bool plane, int n, double far) {
    double sums[31] = {0}, o[3] = {far, -far, 0.5 * far}, Rt[9], work[mvs::kRegisterSolveWork], dT[16] = {0};
    rotation(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1) + 1.5, 0.05, Rt);
    sums[0] = sums[1] = n;
    for (int i = 0; i < n; ++i) {
        const double u = rng.uniform(-3, 3), v = rng.uniform(-2, 2);
        const double q[3] = {u + o[0], v + o[1], 0.3 * std::sin(u) * std::cos(v) + o[2]};
        double nrm[3] = {-0.3 * std::cos(u) * std::cos(v), 0.3 * std::sin(u) * std::sin(v), 1.0};
        const double len = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        double s[3];
        for (int a = 0; a < 3; ++a) {
            nrm[a] /= len;
            s[a] = Rt[3 * a] * (q[0] - o[0]) + Rt[3 * a + 1] * (q[1] - o[1]) + Rt[3 * a + 2] * (q[2] - o[2]) + o[a] + 0.01 * (a + 1);
        }
        const double e[3] = {s[0] - q[0], s[1] - q[1], s[2] - q[2]};
        sums[2] += e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
        if (plane) {
            const double r = e[0] * nrm[0] + e[1] * nrm[1] + e[2] * nrm[2];
            const double J[6] = {s[1] * nrm[2] - s[2] * nrm[1], s[2] * nrm[0] - s[0] * nrm[2], s[0] * nrm[1] - s[1] * nrm[0],
                                 nrm[0], nrm[1], nrm[2]};
            int t = 3;
            for (int a = 0; a < 6; ++a)
                for (int c = a; c < 6; ++c) sums[t++] += J[a] * J[c];
            for (int a = 0; a < 6; ++a) sums[24 + a] += J[a] * r;
            sums[30] += r * r;
        } else {
            for (int a = 0; a < 3; ++a) {
                sums[3 + a] += s[a] - o[a];
                sums[6 + a] += q[a] - o[a];
                for (int c = 0; c < 3; ++c) sums[9 + 3 * a + c] += (s[a] - o[a]) * (q[c] - o[c]);
            }
        }
    }
    const bool ok = plane ? mvs::register_plane_step(sums, work, dT) : mvs::register_point_step(sums, sums[1], o, work, dT);
    put(plane ? "plane" : "point", sums, 31);
    if (!plane) put("", o, 3);
    std::printf(" -> %d", ok ? 1 : 0);
    put("", dT, 16);
    std::printf("\n");
}

}  // namespace

int main() {
    Rng rng{2024};
    for (int i = 0; i < 8; ++i) ldlt_case(rng, 50 + 10 * i, 1.0);
    for (double squeeze : {1e-2, 1e-4, 1e-6}) ldlt_case(rng, 80, squeeze);       // condition numbers up to about 1e12
    ldlt_case(rng, 80, 0.0);                                                      // singular: the last pivot is not > 0
    ldlt_case(rng, 3, 1.0);                                                       // rank 3
    for (double deg : {0.0, 1e-6, 5.0, 45.0, 90.0, 135.0, 170.0, 179.0})
        for (int kind : {0, 1}) horn_case(rng, deg, kind, 0.01);
    for (double deg : {5.0, 120.0, 179.0}) horn_case(rng, deg, 2, 0.0);           // planar
    horn_case(rng, 30.0, 3, 0.0);                                                 // collinear: the rotation about the line is free
    for (int i = 0; i < 6; ++i) {
        double x[6], T[16], B[16], C[16];
        for (int a = 0; a < 6; ++a) x[a] = rng.uniform(-3.2, 3.2);
        if (i == 0)
            for (int a = 0; a < 6; ++a) x[a] = 0.0;
        mvs::register_vector6_to_matrix(x, T);
        put("vec6", x, 6);
        std::printf(" ->");
        put("", T, 16);
        std::printf("\n");
        for (int a = 0; a < 6; ++a) x[a] = rng.uniform(-1.0, 1.0);
        mvs::register_vector6_to_matrix(x, B);
        mvs::register_compose(T, B, C);
        put("compose", T, 16);
        put("", B, 16);
        std::printf(" ->");
        put("", C, 16);
        std::printf("\n");
    }
    for (double far : {0.0, 300.0}) {
        step_case(rng, true, 500, far);
        step_case(rng, false, 500, far);
    }
    step_case(rng, true, 5, 0.0);       // five rows: rank 5, the sixth pivot is rounding noise or not > 0
    std::printf("done\n");
    return 0;
}
