// jacobi.h -- the fixed-sweep Jacobi eigen / singular value solves the solvers restate, once:
// the rotation, the two-sided cyclic solve of a small symmetric matrix, the one-sided cyclic
// solve (b <- b V) and the lane-parallel round-robin solve, with the small helpers around
// them.  Used by Sim3Solver (sim3_args.h), PnPsolver (pnp_device.h) and Initializer
// (init_device.h); tri_nullvec (triangulate_kernels.hip) and init_triangulate's 4x4 loop take
// the rotation alone.
//
// Everything is __host__ __device__ with a fixed operation order (no FMA contraction), so a
// host program runs the very same statements as a kernel.  The small solves take T[N][N] with
// compile-time N and sweep counts and are unrolled: every index is a constant and the
// matrices stay in registers.  The sweep counts belong to the callers: each is that solver's
// documented departure from the reference.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

namespace orbg {

// separates the phases of a (lane, nl) routine; every lane of the workgroup reaches it
#ifdef __HIP_DEVICE_COMPILE__
#define ORBG_GROUP_SYNC() __syncthreads()
#else
#define ORBG_GROUP_SYNC() ((void)0)
#endif

// (c, s) of the rotation that annihilates a_pq, from theta = (a_qq - a_pp) / (2 a_pq): the
// smaller root t of t^2 + 2 theta t - 1 = 0
template <typename T>
__host__ __device__ __forceinline__ void jacobi_rot(T theta, T *c, T *s)
{
    const T at = std::fabs(theta) + std::sqrt(theta * theta + T(1));
    const T t = (theta < T(0) ? T(-1) : T(1)) / at;
    *c = T(1) / std::sqrt(t * t + T(1));
    *s = t * *c;
}

// columns p and q of m <- (c p - s q, s p + c q)
template <int N, typename T>
__host__ __device__ __forceinline__ void jacobi_rot_cols(T m[N][N], int p, int q, T c, T s)
{
#pragma unroll
    for (int k = 0; k < N; k++) {
        const T mkp = m[k][p], mkq = m[k][q];
        m[k][p] = c * mkp - s * mkq;
        m[k][q] = s * mkp + c * mkq;
    }
}

template <int N, typename T>
__host__ __device__ __forceinline__ void jacobi_identity(T v[N][N])
{
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) v[i][j] = i == j ? T(1) : T(0);
}

// Two-sided cyclic Jacobi on the symmetric a: eigenvalues left on the diagonal, eigenvectors
// in the columns of v.  A <- A J, A <- J^T A, the rotated entry set to zero, V <- V J; a plane
// whose entry is zero already is skipped.
template <int N, int SWEEPS, typename T>
__host__ __device__ static inline void jacobi_eig_sym(T a[N][N], T v[N][N])
{
    jacobi_identity<N>(v);
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const T apq = a[p][q];
                if (apq == T(0)) continue;
                T c, s;
                jacobi_rot((a[q][q] - a[p][p]) / (T(2) * apq), &c, &s);
                jacobi_rot_cols<N>(a, p, q, c, s);
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const T apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                a[p][q] = a[q][p] = T(0);
                jacobi_rot_cols<N>(v, p, q, c, s);
            }
    }
}

// columns p and q of b: ((x0 y0 + x1 y1) + x2 y2) + ... in index order
template <int N, typename T>
__host__ __device__ __forceinline__ T jacobi_coldot(const T b[N][N], int p, int q)
{
    T s = b[0][p] * b[0][q] + b[1][p] * b[1][q];
#pragma unroll
    for (int k = 2; k < N; k++) s = s + b[k][p] * b[k][q];
    return s;
}

// One-sided cyclic Jacobi: the columns of b are rotated until they are orthogonal, b <- b V
// (b = U S V^T leaves U S).  A pair of columns that is orthogonal already is skipped.
template <int N, int SWEEPS, typename T>
__host__ __device__ static inline void jacobi_onesided(T b[N][N], T v[N][N])
{
    jacobi_identity<N>(v);
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const T al = jacobi_coldot<N>(b, p, p);
                const T be = jacobi_coldot<N>(b, q, q);
                const T ga = jacobi_coldot<N>(b, p, q);
                if (ga == T(0)) continue;
                T c, s;
                jacobi_rot((be - al) / (T(2) * ga), &c, &s);
                jacobi_rot_cols<N>(b, p, q, c, s);
                jacobi_rot_cols<N>(v, p, q, c, s);
            }
    }
}

// The round-robin (circle) ordering of N indices over NP = N rounded up to even players:
// NP - 1 rounds of N / 2 planes.  Round r pairs player NP - 1 with r and (r + t) with (r - t)
// mod NP - 1 for t = 1 .. NP / 2 - 1.  For odd N player NP - 1 is the bye and its pairing is
// dropped.  Every index is in at most one plane of a round.
template <int N>
__host__ __device__ __forceinline__ void jacobi_round_pair(int round, int t, int *p, int *q)
{
    constexpr int NP = N + (N & 1);
    int a, b;
    if ((N & 1) == 0 && t == 0) {
        a = NP - 1, b = round;
    } else {
        t += N & 1;
        a = (round + t) % (NP - 1);
        b = (round + (NP - 1) - t) % (NP - 1);
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// Cyclic Jacobi in the round-robin ordering on M symmetric N x N matrices at once, by a group
// of nl lanes: A and V are M row-major matrices each (eigenvalues left on A's diagonals,
// eigenvectors in V's columns), cs holds a round's (c, s) pairs, M x N / 2 of them.  A round
// has three phases with a barrier after each: the (c, s) of its planes from A; A <- A J and
// V <- V J, a task per (plane, row), which writes entries (k, p) and (k, q) alone; A <- J^T A
// with the rotated entry set to zero, a task per (plane, column), which writes (p, k) and
// (q, k) alone.  The planes of a round share no index, so within a phase no task reads what
// another writes, and no entry is written twice: the result depends neither on nl nor on
// which task a plane is, and one lane running the tasks in turn gives the same bits.  A plane
// whose entry is zero rotates by (1, 0).  Every trip count is fixed, so every lane of the
// workgroup reaches every barrier.
template <int M, int N, int SWEEPS, typename T>
__host__ __device__ static inline void jacobi_eig_lanes(T *A, T *V, T *cs, int lane, int nl)
{
    constexpr int R = N / 2, NN = N * N;
    for (int e = lane; e < M * NN; e += nl) {
        const int k = e % NN;
        V[e] = (k / N == k % N) ? T(1) : T(0);
    }
    ORBG_GROUP_SYNC();
    for (int sweep = 0; sweep < SWEEPS; sweep++)
        for (int round = 0; round < N + (N & 1) - 1; round++) {
            for (int e = lane; e < M * R; e += nl) {
                const int m = M == 1 ? 0 : e / R, t = e - R * m;
                const T *a = A + NN * m;
                int p, q;
                jacobi_round_pair<N>(round, t, &p, &q);
                const T apq = a[N * p + q];
                T c = T(1), s = T(0);
                if (apq != T(0)) jacobi_rot((a[(N + 1) * q] - a[(N + 1) * p]) / (T(2) * apq), &c, &s);
                cs[2 * e] = c;
                cs[2 * e + 1] = s;
            }
            ORBG_GROUP_SYNC();
            for (int e = lane; e < M * R * N; e += nl) {  // A <- A J, V <- V J
                const int m = M == 1 ? 0 : e / (R * N), r = e - R * N * m, t = r / N, k = r - N * t;
                T *a = A + NN * m, *v = V + NN * m;
                int p, q;
                jacobi_round_pair<N>(round, t, &p, &q);
                const T c = cs[2 * (R * m + t)], s = cs[2 * (R * m + t) + 1];
                const T akp = a[N * k + p], akq = a[N * k + q];
                a[N * k + p] = c * akp - s * akq;
                a[N * k + q] = s * akp + c * akq;
                const T vkp = v[N * k + p], vkq = v[N * k + q];
                v[N * k + p] = c * vkp - s * vkq;
                v[N * k + q] = s * vkp + c * vkq;
            }
            ORBG_GROUP_SYNC();
            for (int e = lane; e < M * R * N; e += nl) {  // A <- J^T A, the rotated entry set to zero
                const int m = M == 1 ? 0 : e / (R * N), r = e - R * N * m, t = r / N, k = r - N * t;
                T *a = A + NN * m;
                int p, q;
                jacobi_round_pair<N>(round, t, &p, &q);
                const T c = cs[2 * (R * m + t)], s = cs[2 * (R * m + t) + 1];
                const T apk = a[N * p + k], aqk = a[N * q + k];
                a[N * p + k] = k == q ? T(0) : c * apk - s * aqk;
                a[N * q + k] = k == p ? T(0) : s * apk + c * aqk;
            }
            ORBG_GROUP_SYNC();
        }
}

// (row, column), row <= column, of the e-th unique entry of a symmetric N x N
template <int N>
__host__ __device__ __forceinline__ void sym_index(int e, int *r, int *c)
{
    int row = 0;
    while (e >= N - row) {
        e -= N - row;
        row++;
    }
    *r = row;
    *c = row + e;
}

template <typename T>
__host__ __device__ __forceinline__ void swap_cols3(T m[3][3], int i, int j)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const T x = m[k][i];
        m[k][i] = m[k][j], m[k][j] = x;
    }
}

// key into descending order, the columns of every matrix given along with it: the
// comparisons (0,1) (1,2) (0,1), strict, so equal keys keep their order
template <typename T, typename... Ms>
__host__ __device__ __forceinline__ void sort3_desc(T key[3], Ms... ms)
{
#pragma unroll
    for (int n = 0; n < 3; n++) {
        const int i = n & 1, j = i + 1;
        if (key[j] > key[i]) {
            const T x = key[i];
            key[i] = key[j], key[j] = x;
            (swap_cols3(ms, i, j), ...);
        }
    }
}

// -1 where column j's component of largest magnitude (the first of equals) is negative, else 1:
// the sign convention for an eigenvector or singular vector
template <typename T>
__host__ __device__ __forceinline__ T largest_sign3(const T m[3][3], int j)
{
    T big = m[0][j];
    if (std::fabs(m[1][j]) > std::fabs(big)) big = m[1][j];
    if (std::fabs(m[2][j]) > std::fabs(big)) big = m[2][j];
    return big < T(0) ? T(-1) : T(1);
}

}  // namespace orbg
