// Which faces of a surface cross which: the pair query behind the third part of MeshFix.repair() in the reference's
// preprocess/prepare.py:28-33 (removal of self-intersecting triangles).  The predicate -- what "cross" means, branch by
// branch -- is specified in semigcn_amd/repair.py; tests/intersect_oracle.py restates it in numpy.
//
// The query is a self-overlap traversal of an existing sg_surface (mesh_dist.hip builds it; nothing of the build changes).
// One lane per face, the faces taken in the tree's leaf (Morton) order, so that a wavefront walks one region of the tree.
// A lane tests its face's own box against the two child boxes of a node with CLOSED comparisons (touching counts), descends
// depth first and keeps the pending sibling on a stack in LDS, as surface_query does.  At a leaf the up to kLeaf faces are
// filtered by id (only partners j > i are tested: a pair is found once, by its lower face), by their own box, and then
// tested with the predicate.  The predicate reads the ORIGINAL vs / faces rows, as refit does -- never tri[], whose b - a
// and c - a are rounded -- and evaluates every determinant in float64 without fused multiply-adds (the Makefile builds this
// file with -ffp-contract=off), so on integer coordinates of magnitude <= 2^10 every determinant is exact.
//
// The output has a data-dependent size, so the same kernel runs twice with no host walk in between:
//   count   n_upper[i] = partners j > i (a plain store by the lane of i); n_any[i] = partners j != i, by integer atomicAdd
//           on both faces of every pair found (n_any is zeroed first; integer sums do not depend on the order);
//           stats[0] = degenerate faces and stats[1] = subtrees dropped on a full stack (always 0, see the kernel; the
//           caller refuses a result that says otherwise), by integer atomicAdd.
//   offsets an exclusive scan of n_upper, done by the caller.
//   emit    the same traversal again; the lane of i writes i << 32 | j at offsets[i] + (its running count).  A lane's
//           traversal order depends on the tree only, and the tree is deterministic (sorted keys, exact min / max boxes).
//   order   one radix sort of the keys over the 32 + bits(F) bits they use, then a split into (i, j) rows: i < j, sorted
//           lexicographically, whatever order the lanes ran in.  Two runs give identical bytes.
//
// Bound: the latency of the dependent node loads, as in surface_query; the float64 arithmetic only runs on candidates whose
// boxes overlap the face's.  Per candidate: 4 bytes of tri[] (the id), 24 bytes of faces, 36 bytes of vs.
#include "mesh_bvh.h"   // struct sg_surface, kLeaf, kStack, the child codes; mesh_common.h

namespace sg {
namespace {

constexpr int kSelfThreads = 64;   // one wavefront per workgroup: its stack is 64 x 64 int32 = 16 KiB of LDS

struct D3 {
  double x, y, z;
};
struct D2 {
  double u, v;
};
struct Face {
  int ia, ib, ic;
  D3 a, b, c;
};

__device__ __forceinline__ int sgn(double v) { return (v > 0.0) - (v < 0.0); }
__device__ __forceinline__ D3 sub(const D3& a, const D3& b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// det of the rows u, v, w -- this order of operations is part of the specification
__device__ __forceinline__ double det3(const D3& u, const D3& v, const D3& w) {
  return u.x * (v.y * w.z - v.z * w.y) + u.y * (v.z * w.x - v.x * w.z) + u.z * (v.x * w.y - v.y * w.x);
}
__device__ __forceinline__ int orient3d(const D3& a, const D3& b, const D3& c, const D3& d) {
  return sgn(det3(sub(a, d), sub(b, d), sub(c, d)));
}
__device__ __forceinline__ D3 normal_of(const Face& t) {
  const D3 e1 = sub(t.b, t.a), e2 = sub(t.c, t.a);
  return D3{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
}
// the axis in which |n| is largest, the lowest one among equals; -1 for a zero normal
__device__ __forceinline__ int drop_axis(const D3& n) {
  const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
  if (ax == 0.0 && ay == 0.0 && az == 0.0) return -1;
  int axis = 0;
  double m = ax;
  if (ay > m) { axis = 1; m = ay; }
  if (az > m) axis = 2;
  return axis;
}
// the two remaining coordinates, in ascending axis order (selects: no indexing into registers)
__device__ __forceinline__ D2 proj(const D3& p, int axis) { return D2{axis == 0 ? p.y : p.x, axis == 2 ? p.y : p.z}; }
__device__ __forceinline__ int orient2d(const D2& a, const D2& b, const D2& c) {
  return sgn((a.u - c.u) * (b.v - c.v) - (a.v - c.v) * (b.u - c.u));
}
// p_k, component by component (a select between the structs themselves would be a select between their addresses)
__device__ __forceinline__ D3 pick(const D3& p0, const D3& p1, const D3& p2, int k) {
  return D3{k == 0 ? p0.x : (k == 1 ? p1.x : p2.x), k == 0 ? p0.y : (k == 1 ? p1.y : p2.y), k == 0 ? p0.z : (k == 1 ? p1.z : p2.z)};
}

// closed segment pq against closed segment cd in the plane, collinear overlap included
__device__ __forceinline__ bool seg_seg(const D2& p, const D2& q, const D2& c, const D2& d) {
  const int s1 = orient2d(p, q, c), s2 = orient2d(p, q, d), s3 = orient2d(c, d, p), s4 = orient2d(c, d, q);
  if (s1 == 0 && s2 == 0 && s3 == 0 && s4 == 0)
    return fmax(fmin(p.u, q.u), fmin(c.u, d.u)) <= fmin(fmax(p.u, q.u), fmax(c.u, d.u)) &&
           fmax(fmin(p.v, q.v), fmin(c.v, d.v)) <= fmin(fmax(p.v, q.v), fmax(c.v, d.v));
  return s1 * s2 <= 0 && s3 * s4 <= 0;
}
__device__ __forceinline__ bool in_tri(const D2& p, const D2& a, const D2& b, const D2& c) {
  const int s1 = orient2d(a, b, p), s2 = orient2d(b, c, p), s3 = orient2d(c, a, p);
  return (s1 >= 0 && s2 >= 0 && s3 >= 0) || (s1 <= 0 && s2 <= 0 && s3 <= 0);
}

// closed segment pq against the closed triangle t; sp, sq: the signs of orient3d(t, p) and orient3d(t, q); axis: t's
__device__ __forceinline__ bool seg_tri(const D3& p, const D3& q, int sp, int sq, const Face& t, int axis) {
  if (sp != 0 || sq != 0) {
    if (sp * sq > 0) return false;
    const int s1 = orient3d(p, q, t.a, t.b), s2 = orient3d(p, q, t.b, t.c), s3 = orient3d(p, q, t.c, t.a);
    return (s1 >= 0 && s2 >= 0 && s3 >= 0) || (s1 <= 0 && s2 <= 0 && s3 <= 0);
  }
  const D2 P = proj(p, axis), Q = proj(q, axis), A = proj(t.a, axis), B = proj(t.b, axis), C = proj(t.c, axis);
  if (in_tri(P, A, B, C) || in_tri(Q, A, B, C)) return true;
  return seg_seg(P, Q, A, B) || seg_seg(P, Q, B, C) || seg_seg(P, Q, C, A);
}

// `count` edges of the triangle e, the first one (e[first], e[first + 1]), in cyclic order, against the triangle t.
// The loop is kept rolled (the vertices rotate through registers): one copy of seg_tri per call site.
__device__ __forceinline__ bool edges_hit(const Face& e, int first, int count, const Face& t, int axis) {
  D3 p = pick(e.a, e.b, e.c, first), q = pick(e.b, e.c, e.a, first), r = pick(e.c, e.a, e.b, first);
  int sp = orient3d(t.a, t.b, t.c, p), sq = orient3d(t.a, t.b, t.c, q);
#pragma unroll 1
  for (int k = 0; k < count; ++k) {
    if (seg_tri(p, q, sp, sq, t, axis)) return true;
    if (k + 1 < count) {
      const D3 n = r;
      r = p;
      p = q;
      q = n;
      sp = sq;
      sq = orient3d(t.a, t.b, t.c, q);
    }
  }
  return false;
}

// position of vertex id v in the face t, -1 when it has none
__device__ __forceinline__ int slot_of(int v, const Face& t) { return v == t.ia ? 0 : (v == t.ib ? 1 : (v == t.ic ? 2 : -1)); }

// The predicate of semigcn_amd/repair.py for two non-degenerate faces, lo the one with the lower id.
__device__ __forceinline__ bool faces_cross(const Face& lo, int axis_lo, const Face& hi, int axis_hi) {
  const int m0 = slot_of(lo.ia, hi), m1 = slot_of(lo.ib, hi), m2 = slot_of(lo.ic, hi);
  const int shared = (m0 >= 0) + (m1 >= 0) + (m2 >= 0);
  if (shared == 3) return true;                             // a duplicate
  if (shared == 2) {                                        // a fold-over: coplanar, both apexes on one side of the edge
    const int k = m0 < 0 ? 0 : (m1 < 0 ? 1 : 2);            // lo's apex
    const D3 a = pick(lo.a, lo.b, lo.c, k), u = pick(lo.b, lo.c, lo.a, k), v = pick(lo.c, lo.a, lo.b, k);
    const int used = (m0 >= 0 ? 1 << m0 : 0) | (m1 >= 0 ? 1 << m1 : 0) | (m2 >= 0 ? 1 << m2 : 0);
    const int kb = (used & 1) == 0 ? 0 : ((used & 2) == 0 ? 1 : 2);      // hi's apex: the slot no vertex of lo matched
    const D3 b = pick(hi.a, hi.b, hi.c, kb);
    if (orient3d(u, v, a, b) != 0) return false;
    const D2 U = proj(u, axis_lo), V = proj(v, axis_lo);
    return orient2d(U, V, proj(a, axis_lo)) * orient2d(U, V, proj(b, axis_lo)) > 0;
  }
  if (shared == 1) {                                        // the two edges opposite the shared vertex
    const int k = m0 >= 0 ? 0 : (m1 >= 0 ? 1 : 2);
    const int kh = m0 >= 0 ? m0 : (m1 >= 0 ? m1 : m2);
    return edges_hit(lo, k == 2 ? 0 : k + 1, 1, hi, axis_hi) || edges_hit(hi, kh == 2 ? 0 : kh + 1, 1, lo, axis_lo);
  }
  return edges_hit(lo, 0, 3, hi, axis_hi) || edges_hit(hi, 0, 3, lo, axis_lo);
}

// Face f from the caller's rows; false when an id is outside [0, V) (the surface was built from other faces: the face then
// takes part in nothing, and nothing is read through the id)
__device__ __forceinline__ bool load_face(const float* __restrict__ vs, const int64_t* __restrict__ faces, int64_t V, int f,
                                          Face& t, float (&box)[6]) {
  const int64_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return false;
  t.ia = (int)ia;
  t.ib = (int)ib;
  t.ic = (int)ic;
  const float* a = vs + 3 * ia;
  const float* b = vs + 3 * ib;
  const float* c = vs + 3 * ic;
  const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
  box[0] = fminf(ax, fminf(bx, cx));
  box[1] = fminf(ay, fminf(by, cy));
  box[2] = fminf(az, fminf(bz, cz));
  box[3] = fmaxf(ax, fmaxf(bx, cx));
  box[4] = fmaxf(ay, fmaxf(by, cy));
  box[5] = fmaxf(az, fmaxf(bz, cz));
  t.a = D3{(double)ax, (double)ay, (double)az};
  t.b = D3{(double)bx, (double)by, (double)bz};
  t.c = D3{(double)cx, (double)cy, (double)cz};
  return true;
}

// -1 for a face that takes part in no pair (a repeated id, a zero float64 normal), else its drop axis
__device__ __forceinline__ int face_axis(const Face& t) {
  if (t.ia == t.ib || t.ib == t.ic || t.ic == t.ia) return -1;
  return drop_axis(normal_of(t));
}

__device__ __forceinline__ bool box_meets(const float (&b)[6], const float4& lo, const float4& hi) {
  return b[0] <= hi.x && lo.x <= b[3] && b[1] <= hi.y && lo.y <= b[4] && b[2] <= hi.z && lo.z <= b[5];
}

// kEmit = false: the count pass; true: the emit pass (see the head comment)
template <bool kEmit>
__global__ __launch_bounds__(kSelfThreads) void self_overlap(const float4* __restrict__ nodes, const float4* __restrict__ tri,
                                                             int64_t F, int64_t V, const float* __restrict__ vs,
                                                             const int64_t* __restrict__ faces, int32_t* __restrict__ n_any,
                                                             int32_t* __restrict__ n_upper,
                                                             unsigned long long* __restrict__ stats,
                                                             const int64_t* __restrict__ offsets, int64_t n_pairs,
                                                             uint64_t* __restrict__ keys) {
  __shared__ int stack[kStack][kSelfThreads];
  const int lane = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * kSelfThreads + lane;
  if (t >= F) return;
  const int f = __float_as_int(tri[3 * t].w);
  if (f < 0 || f >= F) return;
  Face A;
  float box[6];
  const int axis_a = load_face(vs, faces, V, f, A, box) ? face_axis(A) : -1;
  if (axis_a < 0) {
    if (!kEmit) {
      n_upper[f] = 0;
      atomicAdd(stats, 1ull);
    }
    return;
  }
  int64_t out = 0, room = 0;
  if (kEmit) {
    out = offsets[f];
    room = offsets[f + 1] - out;
    if (room <= 0) return;                                  // no partner above f: nothing to write, nothing to walk
    if (out < 0 || room > n_pairs - out) return;            // offsets that do not belong to n_pairs: write nothing
  }
  int found = 0;
  int cur = 0, sp = 0;
  while (true) {
    const float4* nd = nodes + 4 * (int64_t)cur;
    int next0 = -1, next1 = -1;                             // scalars, not an array: the rolled loop must not index registers
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const float4 lo = nd[2 * side], hi = nd[2 * side + 1];
      const int c = __float_as_int(lo.w);
      const bool meets = box_meets(box, lo, hi);
      if (meets && c >= 0) {
        if (side == 0) next0 = c; else next1 = c;
      }
      if (!meets || c >= 0) continue;
      const int64_t k0 = (int64_t)(~c) * kLeaf;
      const int64_t k1 = k0 + kLeaf < F ? k0 + kLeaf : F;
      for (int64_t k = k0; k < k1; ++k) {
        const int g = __float_as_int(tri[3 * k].w);
        if (g <= f || g >= F) continue;                     // a pair is found once, from its lower face
        Face B;
        float bb[6];
        if (!load_face(vs, faces, V, g, B, bb)) continue;
        if (!(box[0] <= bb[3] && bb[0] <= box[3] && box[1] <= bb[4] && bb[1] <= box[4] && box[2] <= bb[5] && bb[2] <= box[5]))
          continue;
        const int axis_b = face_axis(B);
        if (axis_b < 0 || !faces_cross(A, axis_a, B, axis_b)) continue;
        if (kEmit) {
          if (found < room) keys[out + found] = (uint64_t)(uint32_t)f << 32 | (uint64_t)(uint32_t)g;
        } else {
          atomicAdd(n_any + g, 1);
        }
        ++found;
      }
    }
    // depth first: at most one pending sibling per level, and the tree is at most kStack levels deep, so kStack entries
    // still suffice although BOTH children are followed whenever both overlap (surface_query prunes by distance instead)
    if (next0 >= 0 && next1 >= 0) {
      if (sp < kStack) stack[sp++][lane] = next1;
      else if (!kEmit) atomicAdd(stats + 1, 1ull);          // cannot happen (above); if it did, a subtree is lost: say so
      cur = next0;
    } else if (next0 >= 0) {
      cur = next0;
    } else if (next1 >= 0) {
      cur = next1;
    } else if (sp > 0) {
      cur = stack[--sp][lane];
    } else {
      break;
    }
  }
  if (!kEmit) {
    n_upper[f] = found;
    if (found) atomicAdd(n_any + f, found);
  }
}

__global__ void split_keys(const uint64_t* __restrict__ keys, int64_t n, int64_t* __restrict__ pairs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint64_t k = keys[p];
  pairs[2 * p] = (int64_t)(k >> 32);
  pairs[2 * p + 1] = (int64_t)(k & 0xffffffffull);
}

// what both entry points check before anything touches the device; *empty: nothing to do
int check_common(const char* who, const sg_surface* s, const float* vs, const int64_t* faces, int64_t F, bool* empty) {
  *empty = false;
  SG_REQUIRE(F >= 0, "%s: negative F", who);
  SG_REQUIRE(F < ((int64_t)1 << 31) - kLeaf, "%s: F = %lld does not fit the int32 face ids", who, (long long)F);
  if (F == 0) {
    *empty = true;
    return SG_OK;
  }
  SG_REQUIRE(vs && faces, "%s: null pointer", who);
  SG_REQUIRE(s != nullptr, "%s: null surface", who);
  SG_REQUIRE(s->F == F, "%s: the surface was built from %lld faces, not %lld", who, (long long)s->F, (long long)F);
  return SG_OK;
}

}  // namespace
}  // namespace sg

using namespace sg;

SG_API int sg_surface_self_count(const sg_surface* s, const float* vs, const int64_t* faces, int64_t F, int32_t* n_any,
                                 int32_t* n_upper, int64_t* stats_dev, void* stream_) {
  bool empty = false;
  if (int rc = check_common("sg_surface_self_count", s, vs, faces, F, &empty)) return rc;
  if (empty) return SG_OK;
  SG_REQUIRE(n_any && n_upper && stats_dev, "sg_surface_self_count: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  SG_HIP_TRY(hipMemsetAsync(n_any, 0, (size_t)F * sizeof(int32_t), stream));
  SG_HIP_TRY(hipMemsetAsync(stats_dev, 0, 2 * sizeof(int64_t), stream));
  const int64_t nb = (F + kSelfThreads - 1) / kSelfThreads;
  self_overlap<false><<<(unsigned)nb, kSelfThreads, 0, stream>>>(s->nodes.p, s->tri.p, F, s->V, vs, faces, n_any, n_upper,
                                                                (unsigned long long*)stats_dev, nullptr, 0, nullptr);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

SG_API int sg_surface_self_pairs(const sg_surface* s, const float* vs, const int64_t* faces, int64_t F, const int64_t* offsets,
                                 int64_t n_pairs, int64_t* pairs, void* stream_) {
  SG_REQUIRE(n_pairs >= 0, "sg_surface_self_pairs: negative n_pairs");
  SG_REQUIRE(n_pairs < ((int64_t)1 << 31), "sg_surface_self_pairs: n_pairs = %lld does not fit the int32 sort", (long long)n_pairs);
  bool empty = false;
  if (int rc = check_common("sg_surface_self_pairs", s, vs, faces, F, &empty)) return rc;
  if (empty || n_pairs == 0) return SG_OK;
  SG_REQUIRE(offsets && pairs, "sg_surface_self_pairs: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  AsyncBuf<uint64_t> keys_a(stream), keys_b(stream);
  AsyncBuf<char> temp(stream);
  SG_HIP_TRY(keys_a.alloc(n_pairs));
  SG_HIP_TRY(keys_b.alloc(n_pairs));
  SG_HIP_TRY(hipMemsetAsync(keys_a.p, 0, (size_t)n_pairs * sizeof(uint64_t), stream));   // offsets that leave a gap: (0, 0) rows
  const int64_t nb = (F + kSelfThreads - 1) / kSelfThreads;
  self_overlap<true><<<(unsigned)nb, kSelfThreads, 0, stream>>>(s->nodes.p, s->tri.p, F, s->V, vs, faces, nullptr, nullptr,
                                                               nullptr, offsets, n_pairs, keys_a.p);
  SG_HIP_TRY(hipGetLastError());
  const int end_bit = 32 + bits_for((uint64_t)F, 63);
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys_a.p, keys_b.p, (int)n_pairs, 0, end_bit, stream));
  SG_HIP_TRY(temp.alloc(tb));
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, tb, keys_a.p, keys_b.p, (int)n_pairs, 0, end_bit, stream));
  split_keys<<<blocks_for(n_pairs), kThreads, 0, stream>>>(keys_b.p, n_pairs, pairs);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}
