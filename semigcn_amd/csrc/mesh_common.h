// What the mesh stages (mesh_prep, mesh_smooth, mesh_fill, mesh_parts, mesh_manifold, mesh_remesh, mesh_dist, mesh_isect, mesh_fair, mesh_sample, mesh_denoise, mesh_ray, mesh_align) share on the host
// side: typed device buffers that own their memory, the launch geometry, the bit count behind the radix-sort ranges, the
// exclusive scan, and the kernels and the one device helper that were literal copies.  The rule that goes with it: device
// memory of a plan or of a call is a typed member or local that frees itself -- never a raw pointer on a hand-kept free list.
// No floating-point code belongs here: mesh_isect.hip, mesh_remesh.hip, mesh_manifold.hip, mesh_fair.hip, mesh_sample.hip,
// mesh_denoise.hip, mesh_ray.hip and mesh_align.hip are built with -ffp-contract=off, the others not.
#pragma once
#include <hipcub/hipcub.hpp>

#include <utility>

#include "sg_common.h"

namespace sg {

constexpr int kThreads = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The runs of the deterministic reductions (sg_distance_stats, sg_normal_agreement, sg_align_accumulate): at most
// SG_REDUCE_BLOCKS blocks, block b sums the rows [b * chunk, (b + 1) * chunk), chunk a multiple of kThreads
inline int blocks_of(int64_t N) { return N == 0 ? 1 : (int)(blocks_for(N) < (unsigned)SG_REDUCE_BLOCKS ? blocks_for(N) : SG_REDUCE_BLOCKS); }

inline int64_t chunk_for(int64_t N, int nb) {
  const int64_t c = (N + nb - 1) / nb;
  return (c + kThreads - 1) / kThreads * kThreads;
}

// bits needed for a value below n (at least 1, at most cap): the end bit of a radix sort over such values
inline int bits_for(uint64_t n, int cap) {
  int b = 1;
  while (b < cap && (n >> b) != 0) ++b;
  return b;
}

// n elements of device memory (at least one).  An empty buffer makes no HIP call, neither here nor when it is destroyed:
// a plan that never touched a device is destroyed without one.
template <class T>
struct DeviceBuf {
  T* p = nullptr;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { reset(); }
  hipError_t alloc(size_t n) {
    reset();
    return hipMalloc(&p, (n > 0 ? n : 1) * sizeof(T));
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
};

// a device buffer that only grows, by half of what it holds at least; cap counts elements
template <class T>
struct GrowBuf : DeviceBuf<T> {
  size_t cap = 0;
  // room for n elements; `keep` carries the old contents over
  int reserve(size_t n, bool keep, hipStream_t stream) {
    if (n <= cap) return SG_OK;
    SG_HIP_TRY(hipStreamSynchronize(stream));          // nothing in flight reads what is freed below
    size_t bytes = cap * sizeof(T) + cap * sizeof(T) / 2;   // the policy counts bytes, whatever T is
    if (bytes < n * sizeof(T)) bytes = n * sizeof(T);
    if (bytes < 256) bytes = 256;
    const size_t want = (bytes + sizeof(T) - 1) / sizeof(T);
    DeviceBuf<T> q;
    SG_HIP_TRY(q.alloc(want));
    if (keep && this->p && cap) {
      SG_HIP_TRY(hipMemcpyAsync(q.p, this->p, cap * sizeof(T), hipMemcpyDeviceToDevice, stream));
      SG_HIP_TRY(hipStreamSynchronize(stream));
    }
    std::swap(this->p, q.p);                           // q frees the old block on return
    cap = want;
    return SG_OK;
  }
};

// Stream-ordered temporaries: no host synchronisation to free them.
template <class T>
struct AsyncBuf {
  T* p = nullptr;
  hipStream_t s = nullptr;
  explicit AsyncBuf(hipStream_t st) : s(st) {}
  AsyncBuf(const AsyncBuf&) = delete;
  AsyncBuf& operator=(const AsyncBuf&) = delete;
  hipError_t alloc(size_t n) { return hipMallocAsync(&p, n ? n * sizeof(T) : 16, s); }
  ~AsyncBuf() { if (p) (void)hipFreeAsync(p, s); }
};

template <class T>
int exclusive_sum(const T* in, T* out, int64_t n, hipStream_t stream) {
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, stream));
  DeviceBuf<char> temp;
  SG_HIP_TRY(temp.alloc(tb ? tb : 16));
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp.p, tb, in, out, (int)n, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));     // the temporary is freed on return
  return SG_OK;
}

// corner k + 1 of a triangle
__device__ inline int next3(int k) { return k == 2 ? 0 : k + 1; }

namespace {

// the int32 ids a plan keeps, as the int64 the callers take (a template: only the files that launch it carry the kernel)
template <class T>
__global__ void widen32(const int32_t* __restrict__ in, int64_t n, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}

// The neighbour lists of mesh_smooth.hip and mesh_fair.hip start here (templates for the same reason); row_starts also bounds
// the vertex -> face lists of mesh_denoise.hip.  Face-edge
// h = 3 f + i joins a = faces[f][i] and b = faces[f][(i+1)%3]; it puts b on a's list and a on b's: keys (a << 32 | b) and
// (b << 32 | a).  flags[0]: vertex id out of range; flags[1]: degenerate face (repeated vertex).
template <class Key>
__global__ void directed_keys(const int64_t* __restrict__ faces, int64_t n_half, int64_t V, Key* __restrict__ keys,
                              int* __restrict__ flags) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_half) return;
  const int64_t f = h / 3;
  const int i = (int)(h - 3 * f);
  const int64_t a = faces[3 * f + i], b = faces[3 * f + next3(i)];
  Key k0 = ~(Key)0, k1 = ~(Key)0;
  if (a < 0 || a >= V || b < 0 || b >= V) {
    flags[0] = 1;
  } else {
    if (a == b) flags[1] = 1;
    k0 = ((Key)a << 32) | (Key)b;
    k1 = ((Key)b << 32) | (Key)a;
  }
  keys[2 * h] = k0;
  keys[2 * h + 1] = k1;
}

// rowptr[v] = first run whose source vertex is >= v (the runs are sorted by (source, neighbour))
template <class Key>
__global__ void row_starts(const Key* __restrict__ ukeys, int64_t n, int64_t V, int32_t* __restrict__ rowptr) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > V) return;
  const Key key = (Key)v << 32;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ukeys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  rowptr[v] = (int32_t)lo;
}

}  // namespace
}  // namespace sg
