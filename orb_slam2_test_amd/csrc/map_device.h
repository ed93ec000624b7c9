// map_device.h -- what the Map's kernel files share (map_kernels.hip, map_cull_kernels.hip,
// map_edit_kernels.hip, map_loop_kernels.hip, map_lba_kernels.hip, map_gba_kernels.hip,
// map_create_kernels.hip): the workgroup size, the sort-key layout, the workgroup scan, the LDS
// bitonic sort, the store of an ordered list and the test of an entry of a stale observation
// index.  Every kernel file that includes it has its own map_smem.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "map_args.h"

namespace orbg {

#define MAP_T 256
#define MAP_SLOT_MASK 0x1FFFu
#define MAP_BADBIT 0x40000000u
#define MAP_MARKBIT 0x80000000u
#define MAP_VOTES 0x3FFFFFFFu
#define MAP_PRE 12            // staged per initial local keyframe: 10 neighbours, first child, parent
#define MAP_SCAN_TILE 2048

extern __shared__ __attribute__((aligned(16))) char map_smem[];

// LDS of the workgroup kernels: a [K] u32, b [bn] u32, pre [81 * 12] i32, scr [16] i32
static __host__ __device__ inline size_t map_off_b(int K) { return ((size_t)K * 4 + 15) & ~(size_t)15; }
static __host__ __device__ inline size_t map_off_pre(int K, int bn) { return map_off_b(K) + (size_t)bn * 4; }
static __host__ __device__ inline size_t map_off_scr(int K, int bn)
{
    return map_off_pre(K, bn) + (size_t)(ORBG_MAP_MAX_LOCAL + 1) * MAP_PRE * 4;
}
static inline size_t map_lds(int K, int bn) { return map_off_scr(K, bn) + 16 * 4; }
static inline int map_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// exclusive prefix of one value per thread over the workgroup (all threads call it); scr: 4 ints
__device__ __forceinline__ int block_scan(int v, int *scr, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();
    if (lane == 63) scr[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < MAP_T / 64; i++) {
        const int s = scr[i];
        if (i < w) base += s;
        tot += s;
    }
    *total = tot;
    return base + incl - v;
}

// bitonic sort, descending, of a[0 .. n2) in LDS (n2 a power of two)
__device__ __forceinline__ void lds_sort_desc(uint32_t *a, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n2; i += MAP_T) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t x = a[i], y = a[l];
                    if ((i & k) == 0 ? x < y : x > y) {
                        a[i] = y;
                        a[l] = x;
                    }
                }
            }
        }
    __syncthreads();
}

// The ordered list of slot s from keys[t] (weight << 13 | t, 0 = not in the list) in LDS:
// compacted in slot order into srt, sorted descending, stored with nord and neigh.
static __device__ void map_store_order(const MapDev &M, int s, const uint32_t *keys, uint32_t *srt,
                                int *scr)
{
    const int C = (M.K + MAP_T - 1) / MAP_T;
    const int t0 = min((int)threadIdx.x * C, M.K), t1 = min(t0 + C, M.K);
    int c = 0;
    for (int t = t0; t < t1; t++) c += keys[t] != 0;
    int total;
    int pos = block_scan(c, scr, &total);
    for (int t = t0; t < t1; t++)
        if (keys[t]) srt[pos++] = keys[t];
    int n2 = 1;
    while (n2 < total) n2 <<= 1;
    for (int i = total + threadIdx.x; i < n2; i += MAP_T) srt[i] = 0;
    lds_sort_desc(srt, n2);
    uint16_t *os = M.ord_slot + (size_t)s * M.K, *ow = M.ord_w + (size_t)s * M.K;
    for (int i = threadIdx.x; i < total; i += MAP_T) {
        os[i] = (uint16_t)(srt[i] & MAP_SLOT_MASK);
        ow[i] = (uint16_t)(srt[i] >> 13);
    }
    if (threadIdx.x < ORBG_MAP_NEIGH)
        M.neigh[s * ORBG_MAP_NEIGH + threadIdx.x] =
            (int)threadIdx.x < total ? (int32_t)(srt[threadIdx.x] & MAP_SLOT_MASK) : -1;
    if (threadIdx.x == 0) M.nord[s] = total;
}

__device__ __forceinline__ bool map_point_ok(const MapDev &M, int p)
{
    return p >= 0 && p < M.P && (M.mp[p].flags & ORBG_MP_VALID);
}

// entry ob of point p's (possibly stale) index segment still stands; its slot and feature
__device__ __forceinline__ bool cull_obs(const MapDev &M, uint32_t ob, int p, int *u, int *j)
{
    *u = (int)(ob >> 16);
    *j = (int)(ob & 0xFFFFu);
    return (M.kf_flags[*u] & MAP_KF_LIVE) && M.kf_points[(size_t)*u * M.cap + *j] == p;
}

__device__ __forceinline__ int cull_weight(const MapDev &M, int u, int j)
{
    return (M.kf_feat[(size_t)u * M.cap + j] & ORBG_MAP_FEAT_STEREO) ? 2 : 1;
}

// MapPoint::SetBadFlag: bad, and out of every row that holds it
__device__ __forceinline__ void cull_point_bad(const MapDev &M, int p)
{
    M.mp[p].flags &= ~ORBG_MP_VALID;
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) {
        int u, j;
        if (cull_obs(M, M.obs[e], p, &u, &j)) M.kf_points[(size_t)u * M.cap + j] = -1;
    }
}

__device__ __forceinline__ int cull_nobs(const MapDev &M, int p)
{
    int nobs = 0;
    const int e1 = M.obs_off[p + 1];
    for (int e = M.obs_off[p]; e < e1; e++) {
        int u, j;
        if (cull_obs(M, M.obs[e], p, &u, &j)) nobs += cull_weight(M, u, j);
    }
    return nobs;
}

// Ow = -Rwc * tcw of a 3x4 float pose: the product in double, one rounding
__device__ __forceinline__ void loop_centre(const float *T, float *O)
{
    for (int i = 0; i < 3; i++) {
        double a = (double)T[i] * (double)T[3];
        a += (double)T[4 + i] * (double)T[7];
        a += (double)T[8 + i] * (double)T[11];
        O[i] = (float)(-a);
    }
}

static inline int last_rc() { return hipGetLastError() == hipSuccess ? ORBG_OK : ORBG_EIO; }

static inline int map_attr(const void *fn, size_t lds)
{
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess
               ? ORBG_OK
               : ORBG_EIO;
}

}  // namespace orbg
