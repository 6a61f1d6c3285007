// oa_unionfind.hpp -- a lock-free union-find on parent[n] (uint32, parent[x] = x at the start), for many threads that never wait
// for each other (oa_cluster.hpp's link pass).  Written over an atomic-operations policy A so that the same text
// compiles for the device (agent-scope atomics) and for the host (tests/host/unionfind_check.cpp: 16 threads under
// -fsanitize=thread):
//     A::load(p)            a relaxed atomic load
//     A::cas(p, want, v)    compare-and-swap, returns what was there
//     A::fetch_min(p, v)    atomic minimum
//
// Invariants, kept by every operation whichever order they land in:
//   (1) parent[x] <= x, and parent[x] only ever falls.  A root is an x with parent[x] == x; once x is no root it never is again.
//   (2) x and parent[x] belong to the same component of the edges linked so far; trees merge and never split.
// uf_link hooks the HIGHER root under the lower with cas(parent[hi], hi, lo): the cas succeeds only on a word that still says
// "root", so a stale view of parent (an L2 of another XCD, a value read a moment ago) costs a retry and decides nothing.  A stale
// value of parent[x] is an older ancestor of x -- by (2) still in x's component, by (1) not below the true root -- so a find over
// stale values ends at a vertex of the right component; if it is no root any more the cas fails and returns the newer parent, from
// which the link continues: every retry strictly lowers the index in hand.  uf_find_compress moves parent[x] down to the root it
// found with fetch_min, never with a store: the minimum of two ancestors is an ancestor, so (1) and (2) hold.
// When every edge of a component has been linked its tree has one root, and by (1) that is the component's LOWEST index: the
// partition and the roots are the same bits whichever order the threads ran in.
//
// `budget` bounds the steps of one caller (each step of a find and each retry of a link takes one): at 0 the functions return
// where they stand and the caller reports it; nothing spins.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OA_UF_FN __host__ __device__ __forceinline__
#else
#define OA_UF_FN inline
#endif

namespace oa {

// the root of x as far as the loads show it
template <class A>
OA_UF_FN uint32_t uf_find(uint32_t *parent, uint32_t x, int &budget)
{
    for (;;) {
        const uint32_t p = A::load(parent + x);
        if (p == x || budget <= 0) return x;
        x = p;
        --budget;
    }
}

// ... and parent[x] lowered to it when the walk was longer than one step
template <class A>
OA_UF_FN uint32_t uf_find_compress(uint32_t *parent, uint32_t x, int &budget)
{
    const uint32_t first = A::load(parent + x);
    if (first == x) return x;
    const uint32_t r = uf_find<A>(parent, first, budget);
    if (r != first) A::fetch_min(parent + x, r);
    return r;
}

// join the components of a and b
template <class A>
OA_UF_FN void uf_link(uint32_t *parent, uint32_t a, uint32_t b, int &budget)
{
    for (;;) {
        a = uf_find<A>(parent, a, budget);
        b = uf_find<A>(parent, b, budget);
        if (a == b || budget <= 0) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = A::cas(parent + hi, hi, lo);
        if (old == hi) return;                                       // hooked
        a = old;                                                     // (old < hi: somebody hooked hi first)
        b = lo;
        --budget;
    }
}

}  // namespace oa
