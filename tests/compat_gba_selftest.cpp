// compat_gba_selftest.cpp -- orbg_compat::ref::GlobalBundleAdjustemnt / BundleAdjustment
// (compat/orbg_reference.hpp) on stand-ins of the reference's KeyFrame / MapPoint / Map, built
// from a map that tests/test_compat_gba.py writes to files (a scene of tests/ref_gba.py with a
// bad key frame, a bad map point and a point seen from the bad key frame alone):
//
//   compat_gba_selftest DIR nIterations nLoopKF bRobust
//
//   DIR/kfs.bin  per key frame: int32 mnId, int32 bad, float Tcw[12] (3x4), float fx, fy, cx,
//                cy, mbf
//   DIR/mps.bin  per map point: int32 mnId, int32 bad, float pos[3]
//   DIR/obs.bin  per observation, grouped by map point, key frames ascending: int32 map point,
//                int32 key frame, float u, v, uright (< 0: mono), int32 octave
//   DIR/sig.bin  float mvInvLevelSigma2[8]
// and writes what the call left in every object:
//   DIR/out_kf.bin  per key frame: int32 nSetPose, int32 mnBAGlobalForKF, int32 mTcwGBA is 4x4,
//                   int32 0, float GetPose()[12], float mTcwGBA[12] (zeros if empty)
//   DIR/out_mp.bin  per map point: int32 nSetWorldPos, int32 nUpdateNormalAndDepth, int32
//                   mnBAGlobalForKF, int32 mPosGBA is 3x1, float GetWorldPos()[3], float mPosGBA[3]
//   DIR/out_rep.bin the orbg_gba_report
// The Python test holds them to GlobalBundleAdjustment() on arrays it builds from the same
// files itself.  Compiles with g++ -std=c++17 -Wall -Werror against both compat headers and the
// test-only cv:: stub; running it needs liborbg.so and a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "orbg_compat.hpp"
#include "orbg_reference.hpp"

struct KeyFrame;

struct MapPoint {  // include/MapPoint.h: what BundleAdjustment touches
    long unsigned int mnId = 0, mnBAGlobalForKF = 0;
    cv::Mat pos, mPosGBA;
    bool bad = false;
    int nSetWorldPos = 0, nUpdateNormalAndDepth = 0;
    std::map<KeyFrame *, size_t> obs;
    bool isBad() const { return bad; }
    cv::Mat GetWorldPos() const { return pos.clone(); }
    std::map<KeyFrame *, size_t> GetObservations() const { return obs; }
    void SetWorldPos(const cv::Mat &X)
    {
        pos = X.clone();
        nSetWorldPos++;
    }
    void UpdateNormalAndDepth() { nUpdateNormalAndDepth++; }
};

struct KeyFrame {  // include/KeyFrame.h
    long unsigned int mnId = 0, mnBAGlobalForKF = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    cv::Mat Tcw, mTcwGBA;
    bool bad = false;
    int nSetPose = 0;
    bool isBad() const { return bad; }
    cv::Mat GetPose() const { return Tcw.clone(); }
    void SetPose(const cv::Mat &T)
    {
        Tcw = T.clone();
        nSetPose++;
    }
};

struct Map {  // include/Map.h
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> mps;
    std::vector<KeyFrame *> GetAllKeyFrames() const { return kfs; }
    std::vector<MapPoint *> GetAllMapPoints() const { return mps; }
};

#pragma pack(push, 1)
struct KfRec {
    int32_t mnId, bad;
    float Tcw[12], fx, fy, cx, cy, mbf;
};
struct MpRec {
    int32_t mnId, bad;
    float pos[3];
};
struct ObsRec {
    int32_t mp, kf;
    float u, v, uright;
    int32_t octave;
};
struct KfOut {
    int32_t nSetPose, mnBAGlobalForKF, hasGBA, pad;
    float Tcw[12], TcwGBA[12];
};
struct MpOut {
    int32_t nSetWorldPos, nUpdateNormalAndDepth, mnBAGlobalForKF, hasGBA;
    float pos[3], posGBA[3];
};
#pragma pack(pop)

template <class T>
static bool read_all(const std::string &path, std::vector<T> &v)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    const bool ok = std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    std::fclose(f);
    return ok && (size_t)n == v.size() * sizeof(T);
}

template <class T>
static bool write_all(const std::string &path, const T *p, size_t n)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, sizeof(T), n, f) == n;
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 5) {
        std::printf("usage: %s DIR nIterations nLoopKF bRobust\n", argv[0]);
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int nIterations = std::atoi(argv[2]);
    const unsigned long nLoopKF = std::strtoul(argv[3], nullptr, 10);
    const bool bRobust = std::atoi(argv[4]) != 0;
    std::vector<KfRec> kr;
    std::vector<MpRec> mr;
    std::vector<ObsRec> orr;
    std::vector<float> sig;
    if (!read_all(dir + "kfs.bin", kr) || !read_all(dir + "mps.bin", mr) ||
        !read_all(dir + "obs.bin", orr) || !read_all(dir + "sig.bin", sig)) {
        std::printf("cannot read the map in %s\n", dir.c_str());
        return 2;
    }
    std::vector<KeyFrame> K(kr.size());  // one allocation: pointer order = index order
    std::vector<MapPoint> P(mr.size());
    Map m;
    for (size_t i = 0; i < kr.size(); i++) {
        K[i].mnId = kr[i].mnId;
        K[i].bad = kr[i].bad != 0;
        K[i].Tcw = cv::Mat::eye(4, 4, CV_32F);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) K[i].Tcw.at<float>(r, c) = kr[i].Tcw[4 * r + c];
        K[i].fx = kr[i].fx;
        K[i].fy = kr[i].fy;
        K[i].cx = kr[i].cx;
        K[i].cy = kr[i].cy;
        K[i].mbf = kr[i].mbf;
        K[i].mvInvLevelSigma2 = sig;
        m.kfs.push_back(&K[i]);
    }
    for (size_t j = 0; j < mr.size(); j++) {
        P[j].mnId = mr[j].mnId;
        P[j].bad = mr[j].bad != 0;
        P[j].pos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) P[j].pos.at<float>(c) = mr[j].pos[c];
        m.mps.push_back(&P[j]);
    }
    for (const ObsRec &o : orr) {
        KeyFrame &kf = K[o.kf];
        P[o.mp].obs[&kf] = kf.mvKeysUn.size();
        kf.mvKeysUn.push_back(cv::KeyPoint(o.u, o.v, 31.f, -1.f, 0.f, o.octave));
        kf.mvuRight.push_back(o.uright);
    }
    bool stop = false;
    orbg_gba_report rep;
    orbg_compat::ref::GlobalBundleAdjustemnt(orbg_compat::ref::default_ctx(), &m, nIterations, &stop,
                                             nLoopKF, bRobust, &rep);
    std::vector<KfOut> ko(K.size());
    std::vector<MpOut> mo(P.size());
    std::memset(ko.data(), 0, ko.size() * sizeof(KfOut));
    std::memset(mo.data(), 0, mo.size() * sizeof(MpOut));
    for (size_t i = 0; i < K.size(); i++) {
        ko[i].nSetPose = K[i].nSetPose;
        ko[i].mnBAGlobalForKF = (int32_t)K[i].mnBAGlobalForKF;
        ko[i].hasGBA = K[i].mTcwGBA.rows == 4 && K[i].mTcwGBA.cols == 4;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) {
                ko[i].Tcw[4 * r + c] = K[i].Tcw.at<float>(r, c);
                if (ko[i].hasGBA) ko[i].TcwGBA[4 * r + c] = K[i].mTcwGBA.at<float>(r, c);
            }
    }
    for (size_t j = 0; j < P.size(); j++) {
        mo[j].nSetWorldPos = P[j].nSetWorldPos;
        mo[j].nUpdateNormalAndDepth = P[j].nUpdateNormalAndDepth;
        mo[j].mnBAGlobalForKF = (int32_t)P[j].mnBAGlobalForKF;
        mo[j].hasGBA = P[j].mPosGBA.rows == 3 && P[j].mPosGBA.cols == 1;
        for (int c = 0; c < 3; c++) {
            mo[j].pos[c] = P[j].pos.at<float>(c);
            if (mo[j].hasGBA) mo[j].posGBA[c] = P[j].mPosGBA.at<float>(c);
        }
    }
    if (!write_all(dir + "out_kf.bin", ko.data(), ko.size()) ||
        !write_all(dir + "out_mp.bin", mo.data(), mo.size()) ||
        !write_all(dir + "out_rep.bin", &rep, 1)) {
        std::printf("cannot write the results to %s\n", dir.c_str());
        return 2;
    }
    std::printf("nLoopKF %lu robust %d: %d iterations, %d trials, chi2 %.6g -> %.6g, %d blocks of L\n",
                nLoopKF, (int)bRobust, rep.lm.iterations, rep.lm.trials, rep.lm.initial_chi2,
                rep.lm.final_chi2, rep.plan.l_blocks);
    std::printf("compat_gba_selftest OK\n");
    return 0;
}
