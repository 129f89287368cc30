// The lock-free union-find of the mesh stages (mesh_parts.hip: face components; mesh_manifold.hip: the corner union and the
// double cover): an int32 parent array, one thread per link, no host round trip and no launch per round.  find halves the
// path as it goes; the root with the LARGER index is hooked under the root with the smaller one by
// atomicCAS(parent[hi], hi, lo).  A flatten pass follows.  The representative of a class is therefore its smallest member,
// whatever order the atomics took.
//
// Why the union terminates.  Every value a parent slot ever holds obeys parent[x] <= x: it starts as x, a hook writes lo < hi
// into parent[hi], and path halving writes an ancestor of x, which is <= x by induction.  (1) find follows x = parent[x] and
// stops at parent[x] == x; every step strictly lowers x >= 0, so it ends, whatever mixture of old and new values it reads:
// an old value of parent[x] is still an ancestor of x, because a slot that stopped being a root never becomes one again (a
// hook needs parent[hi] == hi, halving only writes where it read parent[x] != x).  (2) A link holds two indices (a, b).
// Each round replaces them by what find returns (not larger), and then either they are equal (done), or the CAS succeeds
// (done), or the CAS fails and RETURNS the value that beat it, old < hi, which replaces hi.  So every unsuccessful round
// strictly lowers a + b, which cannot go below 0: at most a + b + 1 rounds, none of which waits for another thread -- a
// failed CAS means another thread's hook went through.  Progress does not depend on how fresh a load is: the loads and the
// halving stores are relaxed agent-scope atomics (the per-XCD L2s are not coherent for plain loads inside one kernel), but
// even a stale root is corrected by the value the failed CAS brings back from memory.
#pragma once
#include "sg_common.h"

namespace sg {
namespace {

// ---- union-find ------------------------------------------------------------------------------------------------------
__device__ inline int32_t load_parent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree as far as this thread can see; every step halves the path behind it
__device__ inline int32_t find_root(int32_t* __restrict__ parent, int32_t x) {
  int32_t p = load_parent(parent + x);
  while (p != x) {
    const int32_t g = load_parent(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// see the head comment for why this ends
__device__ inline void unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;                       // hi was hooked meanwhile: go on from where it was hooked (old < hi)
    b = lo;
  }
}

__global__ void iota32(int32_t* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int32_t)i;
}

// after the union kernel has finished: every slot points at its root (plain accesses: whatever a thread reads is an
// ancestor, and the roots no longer change)
__global__ void flatten(int32_t* __restrict__ parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t x = (int32_t)i;
  for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
  parent[i] = x;
}

}  // namespace
}  // namespace sg
