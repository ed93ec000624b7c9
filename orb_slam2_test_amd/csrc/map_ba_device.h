// map_ba_device.h -- what the two bundle adjustments on the Map share (map_lba_kernels.hip,
// map_gba_kernels.hip): the test of a vertex keyframe, Converter::toSE3Quat and
// Converter::toCvMat(SE3Quat) as the reference's Eigen code orders them, the edge record of one
// observation, and the float cv::Mat product of two poses.  Included after map_device.h, in files
// compiled with fp contraction off.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/orbg.h"
#include "map_args.h"
#include "map_device.h"

namespace orbg {

__device__ __forceinline__ bool lba_kf_good(const MapDev &M, int s)
{
    return (M.kf_flags[s] & (MAP_KF_LIVE | ORBG_MAP_KF_BAD)) == MAP_KF_LIVE;
}

// Eigen's Quaterniond(Matrix3d) when the trace is not positive: I the largest diagonal entry
template <int I>
__device__ __forceinline__ void lba_quat_diag(const double (&R)[3][3], double (&q)[4])
{
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double s = sqrt(R[I][I] - R[J][J] - R[K][K] + 1.0);
    q[I] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (R[K][J] - R[J][K]) * s;
    q[J] = (R[J][I] + R[I][J]) * s;
    q[K] = (R[K][I] + R[I][K]) * s;
}

// Converter::toSE3Quat of a float 3x4 pose: Eigen's branch, w >= 0, one normalisation
__device__ __forceinline__ void lba_se3quat(const float *T, int fixed, orbg_pose *o)
{
    double R[3][3], q[4];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j];
    const double tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0) {
        double s = sqrt(tr + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[2][1] - R[1][2]) * s;
        q[1] = (R[0][2] - R[2][0]) * s;
        q[2] = (R[1][0] - R[0][1]) * s;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (i == 0 ? R[2][2] > R[0][0] : R[2][2] > R[1][1]) i = 2;
        if (i == 0)
            lba_quat_diag<0>(R, q);
        else if (i == 1)
            lba_quat_diag<1>(R, q);
        else
            lba_quat_diag<2>(R, q);
    }
    if (q[3] < 0) {
        q[0] = -q[0];
        q[1] = -q[1];
        q[2] = -q[2];
        q[3] = -q[3];
    }
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    o->q[0] = q[0] / nq;
    o->q[1] = q[1] / nq;
    o->q[2] = q[2] / nq;
    o->q[3] = q[3] / nq;
    o->t[0] = (double)T[3];
    o->t[1] = (double)T[7];
    o->t[2] = (double)T[11];
    o->fixed = fixed;
    o->pad = 0;
}

// Converter::toCvMat(SE3Quat): Eigen's toRotationMatrix, every element cast to float
__device__ __forceinline__ void lba_tcw(const orbg_pose &p, float *T)
{
    const double *q = p.q;
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    T[0] = (float)(1 - (tyy + tzz));
    T[1] = (float)(txy - twz);
    T[2] = (float)(txz + twy);
    T[3] = (float)p.t[0];
    T[4] = (float)(txy + twz);
    T[5] = (float)(1 - (txx + tzz));
    T[6] = (float)(tyz - twx);
    T[7] = (float)p.t[1];
    T[8] = (float)(txz - twy);
    T[9] = (float)(tyz + twx);
    T[10] = (float)(1 - (txx + tyy));
    T[11] = (float)p.t[2];
}

// The edge of feature j of slot u (vertex `pose`) on window point i: stereo = mvuRight[j] >= 0
// (none attached: mono), obs from mvKeysUn[j] / mvuRight[j], mvInvLevelSigma2[octave], the
// attached camera's intrinsics, C's Huber deltas, active = 1.  false: j is past the attached
// count (obs and inv_sigma2 stay 0).
__device__ __forceinline__ bool lba_fill_edge(const MapAttach &A, const MapLbaConst &C, int u, int j,
                                              int i, int pose, int robust, orbg_edge *out)
{
    orbg_edge E;
    bool ok = true;
    E.point = i;
    E.pose = pose;
    E.stereo = 0;
    E.robust = robust;
    E.active = 1;
    E.pad = 0;
    E.obs[0] = E.obs[1] = E.obs[2] = 0.0;
    E.inv_sigma2 = 0.0;
    if (j < min(A.kfs.counts[u], A.cap)) {
        const orbg_keypoint kp = A.kfs.kps[(size_t)u * A.cap + j];
        const float ur = A.kfs.uright ? A.kfs.uright[(size_t)u * A.cap + j] : -1.0f;
        E.stereo = ur < 0 ? 0 : 1;
        E.obs[0] = (double)kp.x;
        E.obs[1] = (double)kp.y;
        E.obs[2] = E.stereo ? (double)ur : 0.0;
        E.inv_sigma2 = (double)C.inv_sigma2[min(max(kp.octave, 0), 15)];
    } else {
        ok = false;
    }
    const orbg_frustum_camera *cam = A.cams + u;
    E.fx = (double)cam->fx;
    E.fy = (double)cam->fy;
    E.cx = (double)cam->cx;
    E.cy = (double)cam->cy;
    E.bf = (double)cam->bf;
    E.huber_delta = E.stereo ? C.huber_stereo : C.huber_mono;
    *out = E;
    return ok;
}

// The float 4x4 cv::Mat product A * B of two poses stored 3x4 (the fourth rows are 0 0 0 1):
// each entry's four terms summed in double over k in order, rounded once.  B is read as
// [Rb | tb] (trans false) or as the inverse pose [Rb^T | Ob] with the stored centre Ob.
__device__ __forceinline__ void pose_mul(const float *A, const float *B, bool trans, const float *Ob,
                                         float *out)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            double a = 0.0;
            for (int k = 0; k < 3; k++) {
                const float b = trans ? (c < 3 ? B[c * 4 + k] : Ob[k]) : B[k * 4 + c];
                a += (double)A[r * 4 + k] * (double)b;
            }
            a += (double)A[r * 4 + 3] * (c < 3 ? 0.0 : 1.0);
            out[r * 4 + c] = (float)a;
        }
}

}  // namespace orbg
