// place_args.h -- device layout and launch arguments of place recognition (place_kernels.hip:
// DBoW2 L1 score, KeyFrameDatabase), shared with the host entry points (api_place.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbg.h"

namespace orbg {

#define ORBG_KFDB_MAX_KEYFRAMES 8192   // a slot is 13 bits of k_place_query's sort key
#define ORBG_KFDB_MAX_CAP 8192         // as orbg_bow_transform_batch_device
#define ORBG_KFDB_NEIGH 10             // GetBestCovisibilityKeyFrames(10)

// An orbg_kfdb's device state.  Slot s (the caller's KeyFrame handle) owns row s of words /
// weights; live[s] says whether it is in the database, seq[s] is its add-sequence number
// (its position in every inverted list), reloc[s] its mRelocScore.  The inverted file is a
// CSR over the words: inv_off[w] .. inv_off[w + 1] index `post` (slots, in no particular
// order), rebuilt from the live rows when stale; rank[s] = live slots added before s.
struct PlaceDb {
    int32_t K, cap, nwords;
    int32_t *words;             // [K][cap] ascending word ids
    double *weights;            // [K][cap]
    int32_t *nbow;              // [K]
    int32_t *live;              // [K]
    int64_t *seq;               // [K]
    float *reloc;               // [K]
    int64_t *counter;           // [1] next add-sequence number
    int32_t *nlive;             // [1]
    int32_t *rank;              // [K]
    int32_t *inv_off;           // [nwords + 1]
    int32_t *inv_cur;           // [nwords] histogram, then the fill cursors
    int32_t *part;              // [ceil(nwords / 4096)] the scan's tile sums
    uint16_t *post;             // [K * cap]
    unsigned long long *pending;  // [K] (query + 1) << 32 | float bits: this call's mRelocScore
};

struct PlaceQuery {
    orbg_bow_vectors q;
    int32_t qcap, nq;
    const int32_t *qindex;      // [nq] (NULL: query i is vector i)
    const int32_t *neigh;       // [K][10]
    const int32_t *conn;        // loop: [nq][conn_cap]
    const int32_t *nconn;       // loop: [nq]
    const float *min_score;     // loop: [nq]
    int32_t conn_cap, loop;
    int32_t *cand;              // [nq][cand_cap]
    int32_t cand_cap;
    int32_t *ncand, *max_common, *nscored;
};

size_t place_query_lds(int K, int qcap);
struct Prof;  // the context's profiler (orbg_ctx.h)
int launch_place_score(hipStream_t st, const orbg_bow_vectors &a, const orbg_bow_vectors &b, int cap,
                       const int32_t *a_index, const int32_t *b_index, int npairs, double *score,
                       Prof *prof);
int launch_place_add(hipStream_t st, const PlaceDb &D, const int32_t *slots,
                     const orbg_bow_vectors &v, int vcap, const int32_t *index, int n, Prof *prof);
int launch_place_erase(hipStream_t st, const PlaceDb &D, int slot);
int launch_place_rebuild(hipStream_t st, const PlaceDb &D, Prof *prof);
int launch_place_count(hipStream_t st, const PlaceDb &D);
int launch_place_query(hipStream_t st, const PlaceDb &D, const PlaceQuery &Q, Prof *prof);

}  // namespace orbg
