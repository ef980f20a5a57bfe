// The running top-k lists of the fused searches (search.hip over the embedding index,
// maxsim_search.hip over the token store): (score, id) pairs in LDS, kept in the order
// of the results by one whole wave.
#pragma once

#include "device_common.h"

namespace emb {

// (score, id) order of the results: higher score first, equal scores by ascending
// id.  Empty slots are (-inf, -1): the unsigned compare puts id -1 behind every row.
__device__ __forceinline__ bool better(float as, int32_t ai, float bs, int32_t bi)
{
    return as > bs || (as == bs && (uint32_t)ai < (uint32_t)bi);
}

struct Hit { float s; int32_t id; };

// Inserts (cs, ci) into the descending list of k <= 128 entries, by one whole wave
// (lane l holds entries l and l + 64).  Entries the candidate beats move down by
// one, the last one drops out; a candidate that beats none changes nothing.  The
// reads of every lane precede the writes (one wave, LDS operations in order).
__device__ __forceinline__ void list_insert(Hit *list, int k, float cs, int32_t ci, int lane)
{
    const int j0 = lane, j1 = lane + 64;
    Hit e0{0.f, 0}, e1{0.f, 0};
    if (j0 < k) e0 = list[j0];
    if (j1 < k) e1 = list[j1];
    const bool b0 = j0 < k && better(e0.s, e0.id, cs, ci);
    const bool b1 = j1 < k && better(e1.s, e1.id, cs, ci);
    const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));
    if (pos >= k) return;
    if (j0 < k && !b0 && j0 + 1 < k) list[j0 + 1] = e0;
    if (j1 < k && !b1 && j1 + 1 < k) list[j1 + 1] = e1;
    if (lane == (pos & 63)) list[pos] = Hit{cs, ci};
}

// Offers this lane's (s, id) (when `valid`) to the list: candidates that beat the
// current k-th entry are inserted one by one, lowest lane first.  The final list is
// the k best of everything offered whatever the order of the offers, because
// `better` is a total order.
__device__ __forceinline__ void list_offer(Hit *list, int k, float s, int32_t id, bool valid, int lane)
{
    const Hit th = list[k - 1];
    unsigned long long mask = __ballot(valid && better(s, id, th.s, th.id));
    while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        list_insert(list, k, __shfl(s, l, 64), __shfl(id, l, 64), lane);
    }
}

}  // namespace emb
