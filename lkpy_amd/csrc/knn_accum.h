// knn_accum.h -- the reference's `ScoreAccumulator` (src/accel/knn/accum.rs:16-239) restated for
// ONE lane, shared by the kNN scoring kernels (iknn_score.hip, uknn_recommend.hip).
#pragma once

#include "common.h"

namespace lk {

// `Full(BinaryHeap<AccEntry>)` with the REVERSED ordering of accum.rs:170-184: a min-heap on
// the weight.  std's BinaryHeap::push = sift_up(0, old_len); pop = swap the last element into
// the root, sift_down_to_bottom(0), sift_up.  Followed step for step so that WHICH of several
// equal weights is evicted, and the array order the sums run over, are the reference's.
// Element i of the arrays is w[i * STRIDE], v[i * STRIDE] (LDS, or a slab in global memory;
// STRIDE = 64: the accumulators of a wave's lanes interleaved, lane l's at w + l).
template <int STRIDE = 1>
struct KfHeap {
    float *w, *v;
    int len;
    __device__ __forceinline__ void sift_up(int pos, float ew, float ev)
    {
        while (pos > 0) {
            const int parent = (pos - 1) >> 1;
            if (ew >= w[parent * STRIDE]) break;  // hole.element() <= hole.get(parent) in reversed order
            w[pos * STRIDE] = w[parent * STRIDE];
            v[pos * STRIDE] = v[parent * STRIDE];
            pos = parent;
        }
        w[pos * STRIDE] = ew;
        v[pos * STRIDE] = ev;
    }
    __device__ __forceinline__ void push(float ew, float ev) { sift_up(len++, ew, ev); }
    __device__ __forceinline__ void pop()
    {
        const float ew = w[(len - 1) * STRIDE], ev = v[(len - 1) * STRIDE];
        --len;
        if (len == 0) return;
        const int end = len;
        int pos = 0, child = 1;
        const int limit = end >= 2 ? end - 2 : 0;
        while (child <= limit && end >= 2) {
            if (w[child * STRIDE] >= w[(child + 1) * STRIDE]) child += 1;  // hole.get(child) <= hole.get(child + 1)
            w[pos * STRIDE] = w[child * STRIDE];
            v[pos * STRIDE] = v[child * STRIDE];
            pos = child;
            child = 2 * pos + 1;
        }
        if (child == end - 1) {
            w[pos * STRIDE] = w[child * STRIDE];
            v[pos * STRIDE] = v[child * STRIDE];
            pos = child;
        }
        sift_up(pos, ew, ev);
    }
};

// `ScoreAccumulator::add_value` (accum.rs:99-117) on one accumulator of max_nbrs + 1 slots
// (a push precedes the pop): `c` entries held, `heap` = it has turned Full.  Both are updated.
template <int STRIDE = 1>
__device__ __forceinline__ void kf_offer(float *ss, float *sv, int &c, bool &heap, int max_nbrs,
                                         float s, float rv)
{
    if (!heap && c < max_nbrs) {  // Partial(vec): push (accum.rs:103-104)
        ss[c * STRIDE] = s;
        sv[c * STRIDE] = rv;
        c = c + 1;
        return;
    }
    // Full(heap): the reference's BinaryHeap, step for step
    KfHeap<STRIDE> h{ss, sv, c};
    if (!heap) {
        // Partial -> Full (heap_mut, accum.rs:76-83): the vector is popped from the
        // back and every element pushed onto an empty heap = reverse it in place,
        // then sift element k up into the heap formed by the k before it
        for (int i = 0, j = c - 1; i < j; ++i, --j) {
            const float a = ss[i * STRIDE], b = sv[i * STRIDE];
            ss[i * STRIDE] = ss[j * STRIDE];
            sv[i * STRIDE] = sv[j * STRIDE];
            ss[j * STRIDE] = a;
            sv[j * STRIDE] = b;
        }
        for (int kk = 1; kk < c; ++kk) h.sift_up(kk, ss[kk * STRIDE], sv[kk * STRIDE]);
        heap = true;
    }
    if (s > ss[0]) {  // accum.rs:108: strictly greater than the minimum
        h.push(s, rv);
        while (h.len > max_nbrs) h.pop();
        c = h.len;
    }
}

}  // namespace lk
