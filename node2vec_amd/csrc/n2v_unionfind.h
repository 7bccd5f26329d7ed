// n2v_unionfind.h -- a lock-free union-find over int32 parent[], the connected components of n2v_dbscan.hip's union
// scan.  The same text runs on the device (many threads at once) and, single-threaded, on a host
// (tests/test_dbscan_host.py compiles it into a stand-alone program).  The includer defines before this file:
//   N2V_UF_FN            the qualifiers of the functions (`__device__ inline`; `static inline` on a host)
//   N2V_UF_LOAD(p)       a relaxed atomic load of *p (agent scope on the device: the XCDs' L2s are not coherent)
//   N2V_UF_CAS(p, e, v)  atomic compare-and-swap: *p becomes v if it was e; the value it held
//   N2V_UF_MIN(p, v)     atomic minimum: *p becomes min(*p, v)
//
// The rules that keep a union from being lost and a thread from spinning:
//   1. parent[v] <= v always, and parent[v] only ever DECREASES, to a vertex of v's own component.  It starts as v.
//      So every find strictly descends and ends at a root (parent[r] == r), whatever happens around it; a value read
//      late is an older ancestor, still of the same component.
//   2. unite(a, b) is a loop: find both roots; equal: done; else atomicCAS(&parent[hi], hi, lo) with hi the larger
//      root and lo the smaller.  A CAS that succeeds hooks a vertex that WAS a root at that moment under a smaller
//      vertex of b's component: the two components are one from then on.  A CAS that fails means another thread
//      lowered parent[hi] first: loop again.  parent[hi] can be lowered only finitely often (rule 1).
//   3. No thread ever waits for another thread: there is no lock, no flag and no spin on a value someone else owes.
//   4. Every read of parent[] during the scan is N2V_UF_LOAD.
//   5. Path compression goes through N2V_UF_MIN only (find halves the path: parent[x] is lowered to the grandparent
//      it just read).  A plain store parent[x] = parent[parent[x]] could overwrite the hook a concurrent unite just
//      put on the root x and lose that union; a minimum cannot raise what the hook lowered.
// The root of a component is therefore its smallest vertex.
#pragma once

#include <stdint.h>

N2V_UF_FN int32_t uf_find(int32_t *parent, int32_t x) {
  for (;;) {
    const int32_t p = N2V_UF_LOAD(&parent[x]);
    if (p == x) return x;
    const int32_t g = N2V_UF_LOAD(&parent[p]);  // g <= p < x
    if (g != p) N2V_UF_MIN(&parent[x], g);
    x = g;
  }
}

N2V_UF_FN void uf_unite(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    if (N2V_UF_CAS(&parent[hi], hi, lo) == hi) return;
  }
}
