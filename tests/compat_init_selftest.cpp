// compat_init_selftest.cpp -- orbg_compat::ref::Initializer (compat/orbg_reference.hpp) the
// way Tracking::MonocularInitialization uses the reference's class (Tracking.cc:588-676), on
// stand-ins of Frame and cv::Point3f and two synthetic views it builds itself:
//
//   a general scene (300 points at depths 3-8, a rotation of 0.05 rad about y, a baseline of
//   (0.4, 0.05, 0.02), a tenth of the matches wrong): Initialize() returns true, R21 / t21 are
//   the planted motion, nine tenths of the right matches are triangulated in front of both
//   cameras and reproject within 2 px;
//   the same points seen again after a pure rotation: Initialize() returns false and leaves
//   vP3D / vbTriangulated as they were.
//
// Compiles with g++ -std=c++17 -Wall -Werror against both compat headers and the test-only cv::
// stub; running it needs liborbg.so and a GPU.  Exit status 0 and "compat_init_selftest ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <opencv2/core/core.hpp>

#include "orbg_compat.hpp"
#include "orbg_reference.hpp"

struct Point3f {  // cv::Point3f
    float x = 0.f, y = 0.f, z = 0.f;
    Point3f() {}
    Point3f(float a, float b, float c) : x(a), y(b), z(c) {}
};

struct Frame {  // include/Frame.h: what Initializer touches
    cv::Mat mK;
    std::vector<cv::KeyPoint> mvKeysUn;
};

static uint32_t lcg_state = 12345u;
static double uniform(double lo, double hi)
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lo + (hi - lo) * ((lcg_state >> 8) / 16777216.0);
}

#define REQUIRE(c)                                                      \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main()
{
    const double fx = 517.3, fy = 516.5, cx = 318.6, cy = 255.3, ang = 0.05;
    const double R[9] = {cos(ang), 0, sin(ang), 0, 1, 0, -sin(ang), 0, cos(ang)};
    const int n = 300;
    using Init = orbg_compat::ref::Initializer<Frame, cv::Mat, Point3f>;
    for (int pass = 0; pass < 2; pass++) {
        const double C[3] = {pass ? 0.0 : 0.4, pass ? 0.0 : 0.05, pass ? 0.0 : 0.02};
        double t[3];
        for (int r = 0; r < 3; r++) t[r] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
        Frame F1, F2;
        F1.mK = cv::Mat::eye(3, 3, CV_32F);
        F1.mK.at<float>(0, 0) = (float)fx, F1.mK.at<float>(1, 1) = (float)fy;
        F1.mK.at<float>(0, 2) = (float)cx, F1.mK.at<float>(1, 2) = (float)cy;
        F2.mK = F1.mK;
        std::vector<int> vMatches12;
        std::vector<bool> wrong;
        while ((int)F1.mvKeysUn.size() < n) {
            const double u = uniform(20, 620), v = uniform(20, 460), z = uniform(3, 8);
            const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
            double Y[3];
            for (int r = 0; r < 3; r++) Y[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
            double u2 = fx * Y[0] / Y[2] + cx, v2 = fy * Y[1] / Y[2] + cy;
            if (u2 < 5 || u2 > 635 || v2 < 5 || v2 > 475) continue;
            const bool bad = uniform(0, 1) < 0.1;
            if (bad) u2 = uniform(5, 635), v2 = uniform(5, 475);
            F1.mvKeysUn.push_back(cv::KeyPoint((float)(u + uniform(-0.3, 0.3)), (float)(v + uniform(-0.3, 0.3)), 31.f));
            F2.mvKeysUn.push_back(cv::KeyPoint((float)(u2 + uniform(-0.3, 0.3)), (float)(v2 + uniform(-0.3, 0.3)), 31.f));
            vMatches12.push_back((int)F2.mvKeysUn.size() - 1);
            wrong.push_back(bad);
        }
        for (int k = 0; k < 40; k++) {  // keypoints without a match: Normalize sees them
            F1.mvKeysUn.push_back(cv::KeyPoint((float)uniform(5, 635), (float)uniform(5, 475), 31.f));
            F2.mvKeysUn.push_back(cv::KeyPoint((float)uniform(5, 635), (float)uniform(5, 475), 31.f));
            vMatches12.push_back(-1);
        }
        srand(0);  // DUtils::Random::SeedRandOnce(0)
        Init init(orbg_compat::ref::default_ctx(), F1, 1.0f, 200);
        cv::Mat R21, t21;
        std::vector<Point3f> vP3D(3, Point3f(7.f, 7.f, 7.f));
        std::vector<bool> vbTriangulated(3, true);
        const bool ok = init.Initialize(F2, vMatches12, R21, t21, vP3D, vbTriangulated);
        REQUIRE(init.result.n == n);
        if (pass == 1) {
            REQUIRE(!ok);
            REQUIRE(vP3D.size() == 3 && vP3D[0].x == 7.f && vbTriangulated.size() == 3);
            continue;
        }
        REQUIRE(ok && init.result.model == 2);
        REQUIRE(R21.rows == 3 && R21.cols == 3 && t21.rows == 3 && t21.cols == 1);
        double eR = 0, dot = 0, nt = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) eR = fmax(eR, fabs(R21.at<float>(r, c) - R[3 * r + c]));
            dot += t21.at<float>(r) * t[r] / nt;
        }
        REQUIRE(eR < 1e-2 && dot > 0.99);  // as tests/test_initializer_ref.py holds the reference
        REQUIRE((int)vP3D.size() == n + 40 && (int)vbTriangulated.size() == n + 40);
        int right = 0, tri = 0;
        for (int i = 0; i < n + 40; i++) {
            if (i < n && !wrong[i]) right++;
            if (!vbTriangulated[i]) continue;
            REQUIRE(i < n);
            tri++;
            const Point3f &X = vP3D[i];
            REQUIRE(X.z > 0);
            const double du = fx * X.x / X.z + cx - F1.mvKeysUn[i].pt.x, dv = fy * X.y / X.z + cy - F1.mvKeysUn[i].pt.y;
            REQUIRE(du * du + dv * dv <= 4.0 + 1e-3);
        }
        REQUIRE(tri == init.result.ntriangulated && tri >= 0.9 * right);
    }
    printf("compat_init_selftest ok\n");
    return 0;
}
