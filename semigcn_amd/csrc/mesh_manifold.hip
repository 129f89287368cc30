// A raw triangle list made manifold on the device: weld coincident vertices, drop degenerate and duplicate faces, cut what is
// not manifold, orient the faces, turn closed components outward.  The part of MeshFix.repair() in the reference's
// preprocess/prepare.py:28-33 that comes before anything is selected, filled or repaired.  The specification is
// semigcn_amd/manifold.py; in short, in the order the steps run (SG_MANIFOLD_* in include/semigcn.h selects them):
//
//   weld       a vertex's key is the bits of its three float32 coordinates with -0.0 replaced by +0.0.  Three stable 32-bit
//              radix-sort passes over (key, index) -- z, then y, then x -- put equal keys next to each other in ascending
//              index; a position whose key differs from its predecessor's heads a run, an inclusive max-scan of the head
//              positions gives every position its head, and the head's index (the lowest of the class) is the vertex_map.
//   clean      after the weld a face with a repeated vertex is degenerate; the others are keyed by their sorted vertex triple,
//              the same three passes over (key, face) follow, and every face whose triple equals its predecessor's is a
//              duplicate (the sort is stable: the lowest face of a set stays).  One exclusive scan compacts the faces.
//   cut        the union-find of mesh_union.h over the 3 F' corners.  Half-edge h = 3 f + i is keyed lo * V + hi and sorted
//              (the first half-edge sort); a run of exactly two half-edges is a link and unites the two faces' corners at lo
//              and their corners at hi; a run of one or of three and more unites nothing.  Without the cut every corner of
//              a vertex is one class.  A stable 32-bit sort of the corners by vertex then puts the class representatives
//              (the smallest corner of each class) in ascending (vertex, corner) order, and an exclusive scan numbers them.
//   orient     the second half-edge sort, over the cut faces.  The double cover has the nodes 2 f + s; a pair of faces that
//              run along their edge in opposite directions unites (f, 0) ~ (g, 0) and (f, 1) ~ (g, 1), a pair that runs the
//              same way (f, 0) ~ (g, 1) and (f, 1) ~ (g, 0).  r0 = root(2 f), r1 = root(2 f + 1): r0 == r1 is a
//              non-orientable component (left alone), otherwise the face is flipped when r1 < r0, and min(r0, r1) >> 1 is
//              the component's smallest face, which therefore keeps its orientation.  No parity lives on a tree edge, so
//              the termination argument of mesh_union.h holds as it stands.
//   outward    vol6 = sum of det[a, b, c] over the faces of an orientable component that has exactly two faces on every edge,
//              each term float64 from the float32 coordinates by plain multiplies and adds (this file is built with
//              -ffp-contract=off); vol6 < 0 flips the component.  The sum is an atomicAdd per face, so only its sign away
//              from zero is defined.
//
// Everything else is integer work, and every count is an integer atomicAdd: nothing depends on the order of the atomics.
#include <memory>
#include <new>

#include "mesh_common.h"
#include "mesh_union.h"

struct sg_manifold {
  int64_t V = 0, F = 0, Vn = 0, Fn = 0;
  int flags = 0;
  int64_t counts[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // kWelded .. kClosed
  sg::DeviceBuf<int32_t> vmap;      // [V] old vertex -> its weld representative; empty: the identity
  sg::DeviceBuf<int32_t> vid;       // [Vn] new vertex -> input vertex; empty: the identity (no SG_MANIFOLD_DROP)
  sg::DeviceBuf<int32_t> tri;       // [Fn][3] the faces that go out
  sg::DeviceBuf<int32_t> fid;       // [Fn] new face -> old face
  sg::DeviceBuf<uint8_t> flipped;   // [Fn]
  sg::DeviceBuf<uint8_t> nonor;     // [Fn]
};

namespace sg {
namespace {

enum { kWelded = 0, kDegenerate, kDuplicate, kNonManifold, kDistinct, kFlipped, kNonOrientable, kComponents, kClosed, kStats };
constexpr uint32_t kNoKey = 0xffffffffu;       // above every vertex id (V < 2^31)

// one atomicAdd per wavefront: call from converged code, with the condition folded into c
__device__ inline void count_if(bool c, unsigned long long* counter) {
  const unsigned long long m = __ballot(c);
  if (c && __ffsll((long long)m) - 1 == (int)__lane_id()) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// ---- the three-pass sort -----------------------------------------------------------------------------------------------
__global__ void gather_key(const uint32_t* __restrict__ src, const int32_t* __restrict__ idx, int64_t n, int k,
                           uint32_t* __restrict__ key) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) key[p] = src[3 * (int64_t)idx[p] + k];
}

__device__ inline bool same3(const uint32_t* __restrict__ src, int64_t a, int64_t b) {
  return src[3 * a] == src[3 * b] && src[3 * a + 1] == src[3 * b + 1] && src[3 * a + 2] == src[3 * b + 2];
}

// ---- weld --------------------------------------------------------------------------------------------------------------
__global__ void vertex_keys(const float* __restrict__ vs, int64_t n3, uint32_t* __restrict__ src) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const uint32_t b = __float_as_uint(vs[i]);
  src[i] = b == 0x80000000u ? 0u : b;
}

// head[p] = p where sorted position p starts a run of equal keys, 0 elsewhere: the inclusive max-scan is every position's head
__global__ void run_heads(const uint32_t* __restrict__ src, const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ head) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  head[p] = (p > 0 && !same3(src, idx[p], idx[p - 1])) ? (int32_t)p : 0;
}

__global__ void weld_map(const int32_t* __restrict__ idx, const int32_t* __restrict__ headpos, int64_t n, int32_t* __restrict__ vmap,
                         unsigned long long* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool welded = false;
  if (p < n) {
    const int64_t h = headpos[p];
    welded = h != p;
    vmap[idx[p]] = (h >= 0 && h < n) ? idx[h] : idx[p];
  }
  count_if(welded, stats + kWelded);
}

// ---- faces -------------------------------------------------------------------------------------------------------------
// tri = the faces as int32; bad[0]: a vertex id out of range (the face is stored as zeros)
__global__ void load_faces(const int64_t* __restrict__ faces, int64_t F, int64_t V, int32_t* __restrict__ tri, int* __restrict__ bad) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
    bad[0] = 1;
    a = b = c = 0;
  }
  tri[3 * f] = (int32_t)a;
  tri[3 * f + 1] = (int32_t)b;
  tri[3 * f + 2] = (int32_t)c;
}

__global__ void remap_corners(int32_t* __restrict__ tri, int64_t n, const int32_t* __restrict__ vmap) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) tri[c] = vmap[tri[c]];
}

// degen[f] = 1 for a face with a repeated vertex; src = the sorted vertex triple of the others (kNoKey for a degenerate face)
__global__ void classify_faces(const int32_t* __restrict__ tri, int64_t F, uint8_t* __restrict__ degen, uint32_t* __restrict__ src,
                               unsigned long long* __restrict__ stats) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool d = false;
  if (f < F) {
    int32_t a = tri[3 * f], b = tri[3 * f + 1], c = tri[3 * f + 2];
    d = a == b || b == c || c == a;
    degen[f] = d ? 1 : 0;
    if (src) {
      int32_t t;
      if (a > b) { t = a; a = b; b = t; }
      if (b > c) { t = b; b = c; c = t; }
      if (a > b) { t = a; a = b; b = t; }
      src[3 * f] = d ? kNoKey : (uint32_t)a;
      src[3 * f + 1] = d ? kNoKey : (uint32_t)b;
      src[3 * f + 2] = d ? kNoKey : (uint32_t)c;
    }
  }
  count_if(d, stats + kDegenerate);
}

// dup was zeroed
__global__ void mark_duplicates(const uint32_t* __restrict__ src, const int32_t* __restrict__ idx, int64_t n, uint8_t* __restrict__ dup,
                                unsigned long long* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool d = false;
  if (p > 0 && p < n) {
    const int64_t f = idx[p];
    d = src[3 * f] != kNoKey && same3(src, f, idx[p - 1]);
    if (d) dup[f] = 1;
  }
  count_if(d, stats + kDuplicate);
}

// keep[f] for f < F, keep[F] = 0: the exclusive scan ends on the total
__global__ void keep_flags(const uint8_t* __restrict__ degen, const uint8_t* __restrict__ dup, int64_t F, int drop, int32_t* __restrict__ keep) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > F) return;
  keep[f] = (f < F && !(drop && degen[f]) && !dup[f]) ? 1 : 0;
}

__global__ void compact_faces(const int32_t* __restrict__ tri, const uint8_t* __restrict__ degen, const int32_t* __restrict__ keep,
                              const int32_t* __restrict__ fnew, int64_t F, int64_t Fn, int32_t* __restrict__ ftri,
                              int32_t* __restrict__ fid, uint8_t* __restrict__ live) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F || !keep[f]) return;
  const int64_t n = fnew[f];
  if (n < 0 || n >= Fn) return;
  ftri[3 * n] = tri[3 * f];
  ftri[3 * n + 1] = tri[3 * f + 1];
  ftri[3 * n + 2] = tri[3 * f + 2];
  fid[n] = (int32_t)f;
  live[n] = degen[f] ? 0 : 1;
}

// ---- half-edges --------------------------------------------------------------------------------------------------------
// half-edge h = 3 f + i keyed by its undirected edge lo * W + hi, ~0 for a face that is not live (sorts last, links nothing)
__global__ void edge_keys(const int32_t* __restrict__ tri, const uint8_t* __restrict__ live, int64_t n_half, int64_t W,
                          uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_half) return;
  const int64_t f = h / 3;
  const int i = (int)(h - 3 * f);
  uint64_t key = ~0ull;
  if (live[f]) {
    const int64_t a = tri[3 * f + i], b = tri[3 * f + next3(i)];
    key = (uint64_t)(a < b ? a : b) * (uint64_t)W + (uint64_t)(a < b ? b : a);
  }
  keys[h] = key;
  vals[h] = (int32_t)h;
}

// sorted position p starts a run of exactly two half-edges
__device__ inline bool starts_pair(const uint64_t* __restrict__ keys, int64_t p, int64_t n, uint64_t k) {
  return (p == 0 || keys[p - 1] != k) && p + 1 < n && keys[p + 1] == k && !(p + 2 < n && keys[p + 2] == k);
}

// the corner of half-edge h at its lower (which = 0) or higher vertex
__device__ inline int32_t corner_at(const int32_t* __restrict__ tri, int32_t h, int which) {
  const int32_t f = h / 3;
  const int i = h - 3 * f, j = next3(i);
  const bool from_is_lo = tri[3 * f + i] < tri[3 * f + j];
  return 3 * f + ((which == 0) == from_is_lo ? i : j);
}

// the corner union: a link unites the two faces' corners at each end of the edge; stats: edges with three and more faces
__global__ void link_corners(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                             const int32_t* __restrict__ tri, int32_t* __restrict__ parent, unsigned long long* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool many = false;
  if (p < n) {
    const uint64_t k = keys[p];
    if (k != ~0ull) {
      many = (p == 0 || keys[p - 1] != k) && p + 2 < n && keys[p + 2] == k;
      if (starts_pair(keys, p, n, k)) {
        const int32_t h0 = vals[p], h1 = vals[p + 1];
        if (h0 >= 0 && h0 < n && h1 >= 0 && h1 < n) {
          unite(parent, corner_at(tri, h0, 0), corner_at(tri, h1, 0));
          unite(parent, corner_at(tri, h0, 1), corner_at(tri, h1, 1));
        }
      }
    }
  }
  count_if(many, stats + kNonManifold);
}

// the double cover: nodes 2 f + s
__global__ void link_cover(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                           const int32_t* __restrict__ tri, int32_t* __restrict__ parent) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint64_t k = keys[p];
  if (k == ~0ull || !starts_pair(keys, p, n, k)) return;
  const int32_t h0 = vals[p], h1 = vals[p + 1];
  if (h0 < 0 || h0 >= n || h1 < 0 || h1 >= n) return;
  const int32_t f = h0 / 3, g = h1 / 3;
  const int i = h0 - 3 * f, j = h1 - 3 * g;
  const bool up0 = tri[3 * f + i] < tri[3 * f + next3(i)], up1 = tri[3 * g + j] < tri[3 * g + next3(j)];
  const int s = up0 != up1 ? 0 : 1;            // opposite directions: consistent
  unite(parent, 2 * f, 2 * g + s);
  unite(parent, 2 * f + 1, 2 * g + 1 - s);
}

// after flatten: the flip, the non-orientable flag and the component (its smallest face; -1 for a face that is not live)
__global__ void face_parity(const int32_t* __restrict__ parent, const uint8_t* __restrict__ live, int64_t Fn, uint8_t* __restrict__ flip,
                            uint8_t* __restrict__ nonor, int32_t* __restrict__ comp) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= Fn) return;
  if (!live[f]) {
    flip[f] = nonor[f] = 0;
    comp[f] = -1;
    return;
  }
  const int32_t r0 = parent[2 * f], r1 = parent[2 * f + 1];
  nonor[f] = r0 == r1 ? 1 : 0;
  flip[f] = r1 < r0 ? 1 : 0;
  comp[f] = (r0 < r1 ? r0 : r1) >> 1;
}

// open[c] = 1 for a component with a half-edge whose edge does not have exactly two faces (open was zeroed; every writer
// writes the same 1)
__global__ void mark_open(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int64_t Fn,
                          const int32_t* __restrict__ comp, int32_t* __restrict__ open) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint64_t k = keys[p];
  if (k == ~0ull) return;
  const bool first = starts_pair(keys, p, n, k);
  const bool second = p > 0 && keys[p - 1] == k && starts_pair(keys, p - 1, n, k);
  if (first || second) return;
  const int32_t h = vals[p];
  if (h < 0 || h >= n) return;
  const int32_t c = comp[h / 3];
  if (c >= 0 && c < Fn) open[c] = 1;
}

// vol[c] += det[a, b, c] of every face of an orientable component without an open edge, as step 4 left it
__global__ void volume_terms(const float* __restrict__ vs, const int32_t* __restrict__ vid, const int32_t* __restrict__ tri,
                             const uint8_t* __restrict__ flip, const uint8_t* __restrict__ nonor, const int32_t* __restrict__ comp,
                             const int32_t* __restrict__ open, int64_t Fn, double* __restrict__ vol) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= Fn) return;
  const int32_t c = comp[f];
  if (c < 0 || c >= Fn || nonor[f] || open[c]) return;
  const int sw = flip[f];
  int64_t ia = tri[3 * f], ib = tri[3 * f + 1 + sw], ic = tri[3 * f + 2 - sw];
  if (vid) {
    ia = vid[ia];
    ib = vid[ib];
    ic = vid[ic];
  }
  const double ax = vs[3 * ia], ay = vs[3 * ia + 1], az = vs[3 * ia + 2];
  const double bx = vs[3 * ib], by = vs[3 * ib + 1], bz = vs[3 * ib + 2];
  const double cx = vs[3 * ic], cy = vs[3 * ic + 1], cz = vs[3 * ic + 2];
  const double t = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  atomicAdd(&vol[c], t);
}

// the faces that go out, their flags and the counts; vol: null without the outward step
__global__ void finish_faces(const int32_t* __restrict__ tri, const uint8_t* __restrict__ flip, const uint8_t* __restrict__ nonor,
                             const int32_t* __restrict__ comp, const int32_t* __restrict__ open, const double* __restrict__ vol,
                             int64_t Fn, int32_t* __restrict__ out_tri, uint8_t* __restrict__ flipped,
                             unsigned long long* __restrict__ stats) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool fl = false, rep = false, closed = false, no = false;
  if (f < Fn) {
    const int32_t c = comp[f];
    fl = flip[f] != 0;
    if (c >= 0 && c < Fn) {
      if (vol && !nonor[f] && !open[c] && vol[c] < 0.0) fl = !fl;
      rep = c == (int32_t)f;
      closed = rep && !open[c];
      no = rep && nonor[f];
    }
    flipped[f] = fl ? 1 : 0;
    out_tri[3 * f] = tri[3 * f];
    out_tri[3 * f + 1] = tri[3 * f + (fl ? 2 : 1)];
    out_tri[3 * f + 2] = tri[3 * f + (fl ? 1 : 2)];
  }
  count_if(fl, stats + kFlipped);
  count_if(rep, stats + kComponents);
  count_if(closed, stats + kClosed);
  count_if(no, stats + kNonOrientable);
}

// ---- the corner classes and their numbers --------------------------------------------------------------------------------
__global__ void corner_keys(const int32_t* __restrict__ tri, int64_t n, uint32_t* __restrict__ key, int32_t* __restrict__ val) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  key[c] = (uint32_t)tri[c];
  val[c] = (int32_t)c;
}

// over the corners sorted by (vertex, corner): is_rep[p] = 1 where the corner represents its class -- with the cut, where it
// is its own root; without it, where its vertex begins.  is_rep[n] = 0.  stats: the distinct vertices in use.
__global__ void mark_representatives(const uint32_t* __restrict__ key, const int32_t* __restrict__ val, int64_t n,
                                     const int32_t* __restrict__ parent, int32_t* __restrict__ is_rep,
                                     unsigned long long* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool head = false;
  if (p <= n) {
    int32_t r = 0;
    if (p < n) {
      head = p == 0 || key[p - 1] != key[p];
      r = parent ? (parent[val[p]] == val[p] ? 1 : 0) : (head ? 1 : 0);
    }
    is_rep[p] = r;
  }
  count_if(head, stats + kDistinct);
}

// cid[corner] = the new vertex of a representative corner (without the cut: of every corner); vid[new vertex] = its input vertex
__global__ void number_representatives(const uint32_t* __restrict__ key, const int32_t* __restrict__ val,
                                       const int32_t* __restrict__ is_rep, const int32_t* __restrict__ rank, int64_t n, int64_t Vn,
                                       int cut, int32_t* __restrict__ cid, int32_t* __restrict__ vid) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int r = is_rep[p];
  if (cut && !r) return;
  const int64_t id = (int64_t)rank[p] + r - 1;
  if (id < 0 || id >= Vn) return;
  cid[val[p]] = (int32_t)id;
  if (r) vid[id] = (int32_t)key[p];
}

__global__ void renumber_corners(const int32_t* __restrict__ parent, const int32_t* __restrict__ cid, int64_t n,
                                 int32_t* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  out[c] = cid[parent ? parent[c] : c];
}

// ---- export ------------------------------------------------------------------------------------------------------------
__global__ void gather_rows(const float* __restrict__ vs, const int32_t* __restrict__ vid, int64_t Vn, float* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Vn) return;
  const int64_t v = vid ? vid[n] : n;
  out[3 * n] = vs[3 * v];
  out[3 * n + 1] = vs[3 * v + 1];
  out[3 * n + 2] = vs[3 * v + 2];
}

__global__ void iota64(int64_t* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// ---- host helpers ------------------------------------------------------------------------------------------------------
// n (key, index) pairs sorted by the three uint32 of src[index], last component first: stable, so equal triples stay in
// ascending index.  The result is idx_a.
struct Sort3 {
  DeviceBuf<uint32_t> key_a, key_b;
  DeviceBuf<int32_t> idx_a, idx_b;
  DeviceBuf<char> temp;
  int run(const uint32_t* src, int64_t n, hipStream_t stream) {
    SG_HIP_TRY(key_a.alloc(n));
    SG_HIP_TRY(key_b.alloc(n));
    SG_HIP_TRY(idx_a.alloc(n));
    SG_HIP_TRY(idx_b.alloc(n));
    size_t tb = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key_a.p, key_b.p, idx_a.p, idx_b.p, (int)n, 0, 32, stream));
    SG_HIP_TRY(temp.alloc(tb ? tb : 16));
    iota32<<<blocks_for(n), kThreads, 0, stream>>>(idx_a.p, n);
    for (int k = 2; k >= 0; --k) {
      gather_key<<<blocks_for(n), kThreads, 0, stream>>>(src, idx_a.p, n, k, key_a.p);
      SG_HIP_TRY(hipGetLastError());
      SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp.p, tb, key_a.p, key_b.p, idx_a.p, idx_b.p, (int)n, 0, 32, stream));
      std::swap(idx_a.p, idx_b.p);
    }
    return SG_OK;
  }
};

// the half-edges of tri sorted by their undirected edge: (keys_b, vals_b)
struct HalfEdgeSort {
  DeviceBuf<uint64_t> keys_a, keys_b;
  DeviceBuf<int32_t> vals_a, vals_b;
  DeviceBuf<char> temp;
  size_t temp_bytes = 0;
  int alloc(int64_t n_half) {
    SG_HIP_TRY(keys_a.alloc(n_half));
    SG_HIP_TRY(keys_b.alloc(n_half));
    SG_HIP_TRY(vals_a.alloc(n_half));
    SG_HIP_TRY(vals_b.alloc(n_half));
    return SG_OK;
  }
  int run(const int32_t* tri, const uint8_t* live, int64_t n_half, int64_t W, hipStream_t stream) {
    edge_keys<<<blocks_for(n_half), kThreads, 0, stream>>>(tri, live, n_half, W, keys_a.p, vals_a.p);
    SG_HIP_TRY(hipGetLastError());
    const int bits = bits_for((uint64_t)W * (uint64_t)W, 62);   // the keys are below W * W < 2^62; ~0 has every sorted bit set
    size_t tb = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)n_half, 0, bits, stream));
    if (!temp.p || tb > temp_bytes) {
      SG_HIP_TRY(hipStreamSynchronize(stream));              // the first sort's temporary may still be read
      SG_HIP_TRY(temp.alloc(tb ? tb : 16));
      temp_bytes = tb;
    }
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp.p, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)n_half, 0, bits, stream));
    return SG_OK;
  }
};

int inclusive_max(const int32_t* in, int32_t* out, int64_t n, hipStream_t stream) {
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, tb, in, out, hipcub::Max(), (int)n, stream));
  DeviceBuf<char> temp;
  SG_HIP_TRY(temp.alloc(tb ? tb : 16));
  SG_HIP_TRY(hipcub::DeviceScan::InclusiveScan(temp.p, tb, in, out, hipcub::Max(), (int)n, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));     // the temporary is freed on return
  return SG_OK;
}

}  // namespace

void destroy_manifold(sg_manifold* s) { delete s; }

int manifold_create(const float* vs, int64_t V, const int64_t* faces, int64_t F, int flags, hipStream_t stream, sg_manifold** out) {
  const bool weld = flags & SG_MANIFOLD_WELD, dedup = flags & SG_MANIFOLD_DEDUP, cut = flags & SG_MANIFOLD_CUT;
  const bool orient = flags & SG_MANIFOLD_ORIENT, outward = flags & SG_MANIFOLD_OUTWARD, drop = flags & SG_MANIFOLD_DROP;
  SG_REQUIRE(V < ((int64_t)1 << 31) && 3 * F < ((int64_t)1 << 31), "sg_manifold_create: sizes must fit int32");
  std::unique_ptr<sg_manifold> s(new (std::nothrow) sg_manifold);
  SG_REQUIRE(s != nullptr, "sg_manifold_create: out of host memory");
  s->V = V;
  s->F = F;
  s->flags = flags;
  s->Vn = drop ? 0 : V;
  if (F == 0) {                                  // nothing uses a vertex: no device is asked for
    *out = s.release();
    return SG_OK;
  }

  DeviceBuf<int> bad;
  DeviceBuf<unsigned long long> stats;
  DeviceBuf<int32_t> tri;
  int h_bad[1] = {0};
  unsigned long long h_stats[kStats] = {0};
  SG_HIP_TRY(bad.alloc(1));
  SG_HIP_TRY(stats.alloc(kStats));
  SG_HIP_TRY(tri.alloc(3 * F));
  SG_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(h_bad), stream));
  SG_HIP_TRY(hipMemsetAsync(stats.p, 0, sizeof(h_stats), stream));
  load_faces<<<blocks_for(F), kThreads, 0, stream>>>(faces, F, V, tri.p, bad.p);
  SG_HIP_TRY(hipGetLastError());
  // everything below indexes by vertex: nothing runs on ids that were not checked
  SG_HIP_TRY(hipMemcpyAsync(h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(!h_bad[0], "sg_manifold_create: face refers to a vertex outside [0, %lld)", (long long)V);

  // ---- 1. weld (V > 0: a face passed the range check)
  Sort3 vsort, fsort;
  DeviceBuf<uint32_t> vsrc, fsrc;
  DeviceBuf<int32_t> head, headpos;
  if (weld) {
    SG_HIP_TRY(vsrc.alloc(3 * V));
    SG_HIP_TRY(head.alloc(V));
    SG_HIP_TRY(headpos.alloc(V));
    SG_HIP_TRY(s->vmap.alloc(V));
    vertex_keys<<<blocks_for(3 * V), kThreads, 0, stream>>>(vs, 3 * V, vsrc.p);
    SG_HIP_TRY(hipGetLastError());
    if (int rc = vsort.run(vsrc.p, V, stream)) return rc;
    run_heads<<<blocks_for(V), kThreads, 0, stream>>>(vsrc.p, vsort.idx_a.p, V, head.p);
    SG_HIP_TRY(hipGetLastError());
    if (int rc = inclusive_max(head.p, headpos.p, V, stream)) return rc;
    weld_map<<<blocks_for(V), kThreads, 0, stream>>>(vsort.idx_a.p, headpos.p, V, s->vmap.p, stats.p);
    remap_corners<<<blocks_for(3 * F), kThreads, 0, stream>>>(tri.p, 3 * F, s->vmap.p);
    SG_HIP_TRY(hipGetLastError());
  }

  // ---- 2. clean faces
  DeviceBuf<uint8_t> degen, dup, live;
  DeviceBuf<int32_t> keep, fnew, ftri;
  SG_HIP_TRY(degen.alloc(F));
  SG_HIP_TRY(dup.alloc(F));
  SG_HIP_TRY(keep.alloc(F + 1));
  SG_HIP_TRY(fnew.alloc(F + 1));
  if (dedup) SG_HIP_TRY(fsrc.alloc(3 * F));
  SG_HIP_TRY(hipMemsetAsync(dup.p, 0, (size_t)F, stream));
  classify_faces<<<blocks_for(F), kThreads, 0, stream>>>(tri.p, F, degen.p, fsrc.p, stats.p);
  SG_HIP_TRY(hipGetLastError());
  if (dedup) {
    if (int rc = fsort.run(fsrc.p, F, stream)) return rc;
    mark_duplicates<<<blocks_for(F), kThreads, 0, stream>>>(fsrc.p, fsort.idx_a.p, F, dup.p, stats.p);
    SG_HIP_TRY(hipGetLastError());
  }
  keep_flags<<<blocks_for(F + 1), kThreads, 0, stream>>>(degen.p, dup.p, F, drop ? 1 : 0, keep.p);
  SG_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_sum(keep.p, fnew.p, F + 1, stream)) return rc;
  int32_t Fn32 = 0;
  SG_HIP_TRY(hipMemcpyAsync(&Fn32, fnew.p + F, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  const int64_t Fn = Fn32, n_half = 3 * Fn;
  SG_REQUIRE(Fn >= 0 && Fn <= F, "sg_manifold_create: face count %lld out of range", (long long)Fn);
  SG_HIP_TRY(ftri.alloc(n_half));
  SG_HIP_TRY(live.alloc(Fn));
  SG_HIP_TRY(s->fid.alloc(Fn));
  SG_HIP_TRY(s->tri.alloc(n_half));
  SG_HIP_TRY(s->flipped.alloc(Fn));
  SG_HIP_TRY(s->nonor.alloc(Fn));
  compact_faces<<<blocks_for(F), kThreads, 0, stream>>>(tri.p, degen.p, keep.p, fnew.p, F, Fn, ftri.p, s->fid.p, live.p);
  SG_HIP_TRY(hipGetLastError());

  // ---- 3. the corner classes and the new vertices (with SG_MANIFOLD_DROP every face left is live)
  HalfEdgeSort hsort;
  DeviceBuf<int32_t> parent, is_rep, rank, cid, ckey_val_a, ckey_val_b, newtri;
  DeviceBuf<uint32_t> ckey_a, ckey_b;
  DeviceBuf<char> ctemp;
  int64_t Vn = drop ? 0 : V;
  const int32_t* cur = ftri.p;                   // the faces as they stand
  if (Fn > 0 && (cut || orient)) {
    if (int rc = hsort.alloc(n_half)) return rc;
  }
  if (Fn > 0 && drop) {
    if (cut) {
      SG_HIP_TRY(parent.alloc(n_half));
      iota32<<<blocks_for(n_half), kThreads, 0, stream>>>(parent.p, n_half);
      if (int rc = hsort.run(ftri.p, live.p, n_half, V, stream)) return rc;
      link_corners<<<blocks_for(n_half), kThreads, 0, stream>>>(hsort.keys_b.p, hsort.vals_b.p, n_half, ftri.p, parent.p, stats.p);
      flatten<<<blocks_for(n_half), kThreads, 0, stream>>>(parent.p, n_half);
      SG_HIP_TRY(hipGetLastError());
    }
    SG_HIP_TRY(ckey_a.alloc(n_half));
    SG_HIP_TRY(ckey_b.alloc(n_half));
    SG_HIP_TRY(ckey_val_a.alloc(n_half));
    SG_HIP_TRY(ckey_val_b.alloc(n_half));
    SG_HIP_TRY(is_rep.alloc(n_half + 1));
    SG_HIP_TRY(rank.alloc(n_half + 1));
    SG_HIP_TRY(cid.alloc(n_half));
    SG_HIP_TRY(newtri.alloc(n_half));
    corner_keys<<<blocks_for(n_half), kThreads, 0, stream>>>(ftri.p, n_half, ckey_a.p, ckey_val_a.p);
    SG_HIP_TRY(hipGetLastError());
    const int bits = bits_for((uint64_t)V, 32);
    size_t tb = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ckey_a.p, ckey_b.p, ckey_val_a.p, ckey_val_b.p, (int)n_half, 0, bits,
                                                  stream));
    SG_HIP_TRY(ctemp.alloc(tb ? tb : 16));
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(ctemp.p, tb, ckey_a.p, ckey_b.p, ckey_val_a.p, ckey_val_b.p, (int)n_half, 0, bits,
                                                  stream));
    mark_representatives<<<blocks_for(n_half + 1), kThreads, 0, stream>>>(ckey_b.p, ckey_val_b.p, n_half, cut ? parent.p : nullptr,
                                                                           is_rep.p, stats.p);
    SG_HIP_TRY(hipGetLastError());
    if (int rc = exclusive_sum(is_rep.p, rank.p, n_half + 1, stream)) return rc;
    int32_t Vn32 = 0;
    SG_HIP_TRY(hipMemcpyAsync(&Vn32, rank.p + n_half, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    SG_HIP_TRY(hipStreamSynchronize(stream));
    Vn = Vn32;
    SG_REQUIRE(Vn > 0 && Vn <= n_half, "sg_manifold_create: vertex count %lld out of range", (long long)Vn);
    SG_HIP_TRY(s->vid.alloc(Vn));
    number_representatives<<<blocks_for(n_half), kThreads, 0, stream>>>(ckey_b.p, ckey_val_b.p, is_rep.p, rank.p, n_half, Vn,
                                                                         cut ? 1 : 0, cid.p, s->vid.p);
    renumber_corners<<<blocks_for(n_half), kThreads, 0, stream>>>(cut ? parent.p : nullptr, cid.p, n_half, newtri.p);
    SG_HIP_TRY(hipGetLastError());
    cur = newtri.p;
  }

  // ---- 4. orient, 5. outward
  DeviceBuf<int32_t> cover, comp, open;
  DeviceBuf<uint8_t> flip;
  DeviceBuf<double> vol;
  if (Fn > 0 && orient) {
    SG_HIP_TRY(cover.alloc(2 * Fn));
    SG_HIP_TRY(comp.alloc(Fn));
    SG_HIP_TRY(open.alloc(Fn));
    SG_HIP_TRY(flip.alloc(Fn));
    SG_HIP_TRY(hipMemsetAsync(open.p, 0, (size_t)Fn * sizeof(int32_t), stream));
    iota32<<<blocks_for(2 * Fn), kThreads, 0, stream>>>(cover.p, 2 * Fn);
    if (int rc = hsort.run(cur, live.p, n_half, Vn, stream)) return rc;
    link_cover<<<blocks_for(n_half), kThreads, 0, stream>>>(hsort.keys_b.p, hsort.vals_b.p, n_half, cur, cover.p);
    flatten<<<blocks_for(2 * Fn), kThreads, 0, stream>>>(cover.p, 2 * Fn);
    face_parity<<<blocks_for(Fn), kThreads, 0, stream>>>(cover.p, live.p, Fn, flip.p, s->nonor.p, comp.p);
    mark_open<<<blocks_for(n_half), kThreads, 0, stream>>>(hsort.keys_b.p, hsort.vals_b.p, n_half, Fn, comp.p, open.p);
    SG_HIP_TRY(hipGetLastError());
    if (outward) {
      SG_HIP_TRY(vol.alloc(Fn));
      SG_HIP_TRY(hipMemsetAsync(vol.p, 0, (size_t)Fn * sizeof(double), stream));
      volume_terms<<<blocks_for(Fn), kThreads, 0, stream>>>(vs, s->vid.p, cur, flip.p, s->nonor.p, comp.p, open.p, Fn, vol.p);
    }
    finish_faces<<<blocks_for(Fn), kThreads, 0, stream>>>(cur, flip.p, s->nonor.p, comp.p, open.p, outward ? vol.p : nullptr, Fn,
                                                           s->tri.p, s->flipped.p, stats.p);
    SG_HIP_TRY(hipGetLastError());
  } else if (Fn > 0) {
    SG_HIP_TRY(hipMemcpyAsync(s->tri.p, cur, (size_t)n_half * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    SG_HIP_TRY(hipMemsetAsync(s->flipped.p, 0, (size_t)Fn, stream));
    SG_HIP_TRY(hipMemsetAsync(s->nonor.p, 0, (size_t)Fn, stream));
  }
  SG_HIP_TRY(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));                // the temporaries are freed on return
  s->Fn = Fn;
  s->Vn = Vn;
  for (int i = 0; i < kStats; ++i) s->counts[i] = (int64_t)h_stats[i];
  *out = s.release();
  return SG_OK;
}

void manifold_query(const sg_manifold* s, int64_t* info) {
  const int64_t* c = s->counts;
  const bool numbered = (s->flags & SG_MANIFOLD_DROP) && s->Fn > 0;
  info[0] = s->V;
  info[1] = s->F;
  info[2] = s->Vn;
  info[3] = s->Fn;
  info[4] = s->flags;
  info[5] = c[kWelded];
  info[6] = c[kDegenerate];
  info[7] = c[kDuplicate];
  info[8] = c[kNonManifold];
  info[9] = numbered ? s->Vn - c[kDistinct] : 0;
  info[10] = c[kFlipped];
  info[11] = c[kNonOrientable];
  info[12] = c[kComponents];
  info[13] = c[kClosed];
  info[14] = info[15] = 0;
}

int manifold_export(const sg_manifold* s, const float* vs, float* new_vs, int64_t* new_faces, int64_t* vertex_map,
                    int64_t* vertex_ids, int64_t* face_ids, uint8_t* flipped, uint8_t* nonorientable, hipStream_t stream) {
  const int64_t Vn = s->Vn, Fn = s->Fn;
  SG_REQUIRE(Fn == 0 || (new_faces && face_ids && flipped && nonorientable), "sg_manifold_export: null pointer");
  SG_REQUIRE(!new_vs || Vn == 0 || vs, "sg_manifold_export: null pointer");
  if (s->F == 0) return SG_OK;                   // no device was asked for: Vn = V or 0 and the maps are the caller's
  if (new_vs && Vn > 0) gather_rows<<<blocks_for(Vn), kThreads, 0, stream>>>(vs, s->vid.p, Vn, new_vs);
  if (vertex_ids && Vn > 0) {
    if (s->vid.p) widen32<<<blocks_for(Vn), kThreads, 0, stream>>>(s->vid.p, Vn, vertex_ids);
    else iota64<<<blocks_for(Vn), kThreads, 0, stream>>>(vertex_ids, Vn);
  }
  if (vertex_map && s->V > 0) {
    if (s->vmap.p) widen32<<<blocks_for(s->V), kThreads, 0, stream>>>(s->vmap.p, s->V, vertex_map);
    else iota64<<<blocks_for(s->V), kThreads, 0, stream>>>(vertex_map, s->V);
  }
  if (Fn > 0) {
    widen32<<<blocks_for(3 * Fn), kThreads, 0, stream>>>(s->tri.p, 3 * Fn, new_faces);
    widen32<<<blocks_for(Fn), kThreads, 0, stream>>>(s->fid.p, Fn, face_ids);
    SG_HIP_TRY(hipMemcpyAsync(flipped, s->flipped.p, (size_t)Fn, hipMemcpyDeviceToDevice, stream));
    SG_HIP_TRY(hipMemcpyAsync(nonorientable, s->nonor.p, (size_t)Fn, hipMemcpyDeviceToDevice, stream));
  }
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
