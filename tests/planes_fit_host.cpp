// planes_fit_host.cpp -- csrc/cloud_planes_fit.h on the host: the plane fit of mvs_cloud_planes on stated point sets, built
// by tests/test_cloud_planes_host.py with the address and undefined-behaviour sanitizers and run directly.  Every line is
//     fit <9 sums> <m> <o: 3> <has_toward> <toward: 3> <candidate: 8> -> <1: the fit, 0: the candidate's plane> <plane: 4>
// in hexadecimal floats, which the test reads back exactly; the last line is "done".
#include "cloud_planes_fit.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace mvs;

struct Pt {
    double x, y, z;
};

static void emit(const double* sums, double m, const double* o, const double* toward, const double* cand) {
    double plane[4] = {0.0, 0.0, 0.0, 0.0};
    const int fitted = planes_fit(sums, m, o, toward, cand, plane);
    std::printf("fit");
    for (int a = 0; a < kPlanesSums; ++a) std::printf(" %a", sums[a]);
    std::printf(" %a", m);
    for (int a = 0; a < 3; ++a) std::printf(" %a", o[a]);
    std::printf(" %a", toward ? 1.0 : 0.0);
    for (int a = 0; a < 3; ++a) std::printf(" %a", toward ? toward[a] : 0.0);
    for (int a = 0; a < kPlanesCand; ++a) std::printf(" %a", cand[a]);
    std::printf(" -> %a", (double)fitted);
    for (int a = 0; a < 4; ++a) std::printf(" %a", plane[a]);
    std::printf("\n");
}

// the sums of the points about o, added in order (the fit does not care how they were added), and the candidate through
// the first three points
static void run(const std::vector<Pt>& pts, const double* o, const double* toward) {
    double sums[kPlanesSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    std::vector<Pt> q;
    for (const Pt& p : pts) q.push_back({p.x - o[0], p.y - o[1], p.z - o[2]});
    for (const Pt& v : q) {
        const double c[3] = {v.x, v.y, v.z};
        int k = 3;
        for (int a = 0; a < 3; ++a) {
            sums[a] += c[a];
            for (int b = a; b < 3; ++b) sums[k++] += c[a] * c[b];
        }
    }
    const double a[3] = {q[1].x - q[0].x, q[1].y - q[0].y, q[1].z - q[0].z};
    const double b[3] = {q[2].x - q[0].x, q[2].y - q[0].y, q[2].z - q[0].z};
    double cand[kPlanesCand] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0], 0.0, 0.0,
                                q[0].x, q[0].y, q[0].z};
    cand[3] = (cand[0] * q[0].x + cand[1] * q[0].y) + cand[2] * q[0].z;
    cand[4] = 0.25 * ((cand[0] * cand[0] + cand[1] * cand[1]) + cand[2] * cand[2]);
    emit(sums, (double)pts.size(), o, toward, cand);
}

int main() {
    const double o[3] = {1.0, -2.0, 600.0}, zero[3] = {0.0, 0.0, 0.0};
    const double above[3] = {0.0, 0.0, 1000.0}, below[3] = {0.0, 0.0, -1000.0};
    // a plane: z = 0.1 x - 0.2 y + 603 on a 7 x 5 grid, with a ripple of 0.01
    std::vector<Pt> plane;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 5; ++j)
            plane.push_back({10.0 * i - 30.0, 7.0 * j - 14.0, 0.1 * (10.0 * i - 30.0) - 0.2 * (7.0 * j - 14.0) + 603.0 + 0.01 * ((i * 5 + j) % 3 - 1)});
    run(plane, o, nullptr);
    run(plane, o, above);
    run(plane, o, below);
    run(plane, zero, nullptr);
    // an axis-aligned wall: x = -285 exactly; the eigenvalue is zero
    std::vector<Pt> wall;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 4; ++j) wall.push_back({-285.0, 20.0 * i, 600.0 + 30.0 * j + i});
    run(wall, o, nullptr);
    run(wall, o, above);
    // collinear points: two eigenvalues vanish; any normal across the line is a least-squares plane
    std::vector<Pt> line;
    for (int i = 0; i < 9; ++i) line.push_back({1.0 + i, 2.0 + 2.0 * i, 600.0 - i});
    line[1] = {1.5, 2.0, 600.0};      // the candidate's three points are not collinear, the rest are
    run(line, o, nullptr);
    // coincident points: the covariance is zero, the lowest axis is taken
    std::vector<Pt> same(5, Pt{3.0, 4.0, 605.0});
    same[1] = {4.0, 4.0, 605.0};
    same[2] = {3.0, 5.0, 605.0};
    {
        double sums[kPlanesSums];
        const double v[3] = {2.0, 6.0, 5.0};
        int k = 3;
        for (int a = 0; a < 3; ++a) {
            sums[a] = 5.0 * v[a];
            for (int b = a; b < 3; ++b) sums[k++] = 5.0 * (v[a] * v[b]);
        }
        const double cand[kPlanesCand] = {0.0, 0.0, 1.0, 5.0, 0.25, 2.0, 6.0, 5.0};
        emit(sums, 5.0, o, nullptr, cand);
        emit(sums, 5.0, o, below, cand);
    }
    run(same, o, nullptr);
    // sums that are not finite: the candidate's own plane, signed by the same rules
    {
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        const double cand[kPlanesCand] = {0.0, -3.0, 4.0, 12.0, 6.25, 1.0, 0.0, 3.0};
        double sums[kPlanesSums] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0};
        sums[4] = nan;
        emit(sums, 4.0, o, nullptr, cand);
        sums[4] = 5.0;
        sums[0] = inf;
        emit(sums, 4.0, o, above, cand);
        sums[0] = 1e308;
        sums[3] = 1e308;      // mean * mean overflows
        emit(sums, 1.0, o, below, cand);
    }
    std::printf("done\n");
    return 0;
}
