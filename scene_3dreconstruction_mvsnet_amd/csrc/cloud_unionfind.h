// cloud_unionfind.h -- the lock-free union-find of cloud_cluster.hip (mvs_cloud_cluster, include/mvs_cluster_abi.h): one
// 32-bit parent word per point, uf_find with path halving, uf_union by compare-and-swap on a root, the larger root always
// hung under the smaller.  It compiles as HIP device code (the __hip_atomic_* builtins at agent scope, as cloud_knn.h uses
// them) and as plain host C++ (the compiler's __atomic builtins): tests/cluster_unionfind_host.cpp runs the very same two
// functions from 16 threads under the host sanitizers.
//
// The invariant, argued in the header of the ABI: every value ever stored in parent[i] is <= i.  There are two stores,
// both compare-and-swaps that replace a value by a smaller one: the halving step of uf_find (p -> g = parent[p] <= p) and
// the hang of uf_union (a root r -> a smaller root).  So a find path strictly decreases and ends within i steps whatever
// other threads do; a failed swap means a word has decreased, which bounds the retries; and at quiescence the root of a
// set is its smallest index.  All accesses are relaxed: only the coherence of each single word is used.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define MVS_UF_FN __device__ __forceinline__
#else
#define MVS_UF_FN inline
#endif

namespace mvs {

MVS_UF_FN unsigned uf_load(const unsigned* w) {
#if defined(__HIP__) || defined(__HIPCC__)
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(w, __ATOMIC_RELAXED);
#endif
}

// *w: expect -> want, if it still holds `expect`; true when this call stored
MVS_UF_FN bool uf_swap(unsigned* w, unsigned expect, unsigned want) {
#if defined(__HIP__) || defined(__HIPCC__)
    return __hip_atomic_compare_exchange_strong(w, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_compare_exchange_n(w, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
}

// The root of x's set at some moment of the call.  Each step goes from x to a value read from a parent word of the path,
// which is below x unless x is a root; `p >= x` ends the walk at a root -- and at anything the invariant excludes, so the
// loop ends within x steps and stays inside [0, x] whatever the words hold.  Halving: x's word moves from its parent p to
// its grandparent g (only if it still holds p: the word never grows), and the walk goes on from g < p < x.
MVS_UF_FN unsigned uf_find(unsigned* parent, unsigned x) {
    for (;;) {
        const unsigned p = uf_load(&parent[x]);
        if (p >= x) return x;
        const unsigned g = uf_load(&parent[p]);
        if (g >= p) return p;
        uf_swap(&parent[x], p, g);
        x = g;
    }
}

// the same walk without a store, for a launch in which nobody unites
MVS_UF_FN unsigned uf_root(const unsigned* parent, unsigned x) {
    for (;;) {
        const unsigned p = uf_load(&parent[x]);
        if (p >= x) return x;
        x = p;
    }
}

// Unites the sets of a and b.  A round finds both roots; equal roots end it; else the larger root, if it still is one, is
// hung under the smaller.  A failed swap means the larger root has been hung elsewhere meanwhile (its word decreased):
// the next round starts from the two roots just found, which are still in the sets of a and b.
MVS_UF_FN void uf_union(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        if (uf_swap(&parent[hi], hi, lo)) return;
    }
}

}  // namespace mvs
