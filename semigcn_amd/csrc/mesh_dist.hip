// Point-to-surface distance on the device: the query behind the reference's scoring step
// (check/dist_check.py:13-67, pymeshlab's distance_from_reference_mesh).
//
// Build (sg_surface_create): 64-bit keys (Morton code of the face centroid, face index) are
// radix-sorted (hipCUB); runs of kLeaf consecutive sorted faces form the leaves; the internal nodes
// come from Karras 2012 ("Maximizing parallelism in the construction of BVHs, octrees, and k-d
// trees") over the leaves' first keys, and the boxes are refitted bottom-up (one thread per leaf,
// the second arrival at a node carries on).  The only host synchronisation is the face-index check,
// before any kernel dereferences a vertex index.
//
// Query (sg_surface_query): the points are sorted by Morton code so that a wavefront walks one
// region of the tree; each lane descends nearest child first, keeps the farther one on a stack in
// LDS, and prunes on the distance to each box.  No atomics: a point's result depends on the point
// and the tree only.  Bound: latency of the dependent node / triangle loads, not HBM bandwidth.
//
// Point-triangle arithmetic runs in the triangle's local frame (p - a, b - a, c - a): the rounding
// error then scales with the distance and the triangle size, not with the coordinates.  What rests
// on the normal is float64 (tri_offset), so the error does not grow with the triangle's thinness.
#include <memory>
#include <new>

#include "mesh_bvh.h"   // struct sg_surface, kLeaf, kStack, the child codes; mesh_common.h

namespace sg {
namespace {

constexpr int kQueryThreads = 64; // one wavefront per workgroup: its stack is 64 x 64 int32 = 16 KiB of LDS
constexpr int kRedBlocks = 1024;  // fixed grid of the metric reduction: a fixed summation order

__device__ __forceinline__ uint64_t spread3(uint64_t x) {   // 21 bits -> every third bit of 63
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

__device__ __forceinline__ uint64_t morton(float x, float y, float z, const float* b, int bits) {
  const float scale = (float)(1u << bits);
  const uint32_t top = (1u << bits) - 1;
  uint64_t c[3];
  const float v[3] = {x, y, z};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ext = b[3 + k] - b[k];
    float t = ext > 0.f ? (v[k] - b[k]) / ext : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f) * scale;            // query points outside the box clamp to its faces (NaN -> 0)
    c[k] = spread3(min((uint32_t)t, top));
  }
  return c[0] << 2 | c[1] << 1 | c[2];
}

__global__ void check_faces(const int64_t* __restrict__ faces, int64_t n, int64_t V, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = faces[i];
  if (v < 0 || v >= V) *bad = 1;
}

// Per-block min / max of n points (rows of 3 floats; centroids of faces when faces != nullptr) -> part[block][6].
__global__ void bounds_partial(const float* __restrict__ vs, const int64_t* __restrict__ faces, int64_t n,
                               float* __restrict__ part) {
  __shared__ float s[6][kThreads];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float x;
      if (faces)
        x = (vs[3 * faces[3 * i] + k] + vs[3 * faces[3 * i + 1] + k] + vs[3 * faces[3 * i + 2] + k]) * (1.f / 3.f);
      else
        x = vs[3 * i + k];
      lo[k] = fminf(lo[k], x);
      hi[k] = fmaxf(hi[k], x);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s[k][threadIdx.x] = lo[k];
    s[3 + k][threadIdx.x] = hi[k];
  }
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s[k][threadIdx.x] = fminf(s[k][threadIdx.x], s[k][threadIdx.x + w]);
        s[3 + k][threadIdx.x] = fmaxf(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + w]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 6) part[6 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

__global__ void bounds_finish(const float* __restrict__ part, int nb, float* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= 6) return;
  float v = k < 3 ? INFINITY : -INFINITY;
  for (int b = 0; b < nb; ++b) v = k < 3 ? fminf(v, part[6 * b + k]) : fmaxf(v, part[6 * b + k]);
  out[k] = v;
}

__global__ void face_keys(const float* __restrict__ vs, const int64_t* __restrict__ faces, int64_t F,
                          const float* __restrict__ bounds, int mbits, int idx_bits, uint64_t* __restrict__ keys) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = (vs[3 * faces[3 * f] + k] + vs[3 * faces[3 * f + 1] + k] + vs[3 * faces[3 * f + 2] + k]) * (1.f / 3.f);
  keys[f] = morton(c[0], c[1], c[2], bounds, mbits) << idx_bits | (uint64_t)f;
}

// Triangles in leaf order, local frame at vertex a.
__global__ void gather_tris(const float* __restrict__ vs, const int64_t* __restrict__ faces, int64_t F,
                            const uint64_t* __restrict__ keys, uint64_t idx_mask, float4* __restrict__ tri) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= F) return;
  const int64_t f = (int64_t)(keys[k] & idx_mask);
  const float* a = vs + 3 * faces[3 * f];
  const float* b = vs + 3 * faces[3 * f + 1];
  const float* c = vs + 3 * faces[3 * f + 2];
  tri[3 * k] = make_float4(a[0], a[1], a[2], __int_as_float((int)f));
  tri[3 * k + 1] = make_float4(b[0] - a[0], b[1] - a[1], b[2] - a[2], 0.f);
  tri[3 * k + 2] = make_float4(c[0] - a[0], c[1] - a[1], c[2] - a[2], 0.f);
}

__device__ __forceinline__ int delta(const uint64_t* __restrict__ keys, int64_t L, int64_t i, int64_t j) {
  if (j < 0 || j >= L) return -1;
  return __clzll((long long)(keys[i * kLeaf] ^ keys[j * kLeaf]));   // the first key of every leaf; all distinct
}

// Karras 2012, Figure 4: internal node i of the L - 1; parent codes are (parent << 1 | slot).
__global__ void karras_nodes(const uint64_t* __restrict__ keys, int64_t L, float4* __restrict__ nodes,
                             int64_t* __restrict__ parent_leaf, int64_t* __restrict__ parent_node) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (L == 1) {                         // a lone leaf: node 0 holds it as child 0 and an empty box as child 1
    if (i != 0) return;
    nodes[0].w = code_bits(~0);
    nodes[2] = make_float4(INFINITY, INFINITY, INFINITY, code_bits(~0));
    nodes[3] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    parent_leaf[0] = 0;
    parent_node[0] = -1;
    return;
  }
  if (i >= L - 1) return;
  const int d = delta(keys, L, i, i + 1) - delta(keys, L, i, i - 1) > 0 ? 1 : -1;
  const int dmin = delta(keys, L, i, i - d);
  int64_t lmax = 2;
  while (delta(keys, L, i, i + lmax * d) > dmin) lmax <<= 1;
  int64_t l = 0;
  for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(keys, L, i, i + (l + t) * d) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = delta(keys, L, i, j);
  int64_t s = 0;
  for (int64_t div = 2;; div <<= 1) {
    const int64_t t = (l + div - 1) / div;
    if (delta(keys, L, i, i + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int64_t g = i + s * d + (d < 0 ? -1 : 0);
  const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
  const int c0 = lo == g ? ~(int)g : (int)g;
  const int c1 = hi == g + 1 ? ~(int)(g + 1) : (int)(g + 1);
  nodes[4 * i].w = code_bits(c0);
  nodes[4 * i + 2].w = code_bits(c1);
  if (c0 < 0) parent_leaf[g] = 2 * i; else parent_node[g] = 2 * i;
  if (c1 < 0) parent_leaf[g + 1] = 2 * i + 1; else parent_node[g + 1] = 2 * i + 1;
  if (i == 0) parent_node[0] = -1;
}

__device__ __forceinline__ void store_box(float4* __restrict__ nodes, int64_t code, const float (&b)[6]) {
  float* lo = (float*)&nodes[4 * (code >> 1) + 2 * (code & 1)];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __hip_atomic_store((unsigned*)(lo + k), __float_as_uint(b[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((unsigned*)(lo + 4 + k), __float_as_uint(b[3 + k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Bottom-up refit.  The boxes handed from one thread to another are stored and loaded with agent-scope atomics (no L1
// copy can be stale) and ordered by the acquire-release add on the node's arrival counter; the first arrival stops, the
// second one unites both children and climbs.  Min / max are exact, so the boxes do not depend on the arrival order.
// Leaf boxes come from the vertices themselves (not a + (b - a), which rounds): they hold the triangles exactly.
__global__ void refit(const float* __restrict__ vs, const int64_t* __restrict__ faces, const float4* __restrict__ tri,
                      int64_t F, int64_t L, const int64_t* __restrict__ parent_leaf,
                      const int64_t* __restrict__ parent_node, float4* __restrict__ nodes, int* __restrict__ arrivals) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const int64_t k1 = (l + 1) * kLeaf < F ? (l + 1) * kLeaf : F;
  for (int64_t k = l * kLeaf; k < k1; ++k) {
    const int64_t f = __float_as_int(tri[3 * k].w);
    for (int c = 0; c < 3; ++c) {
      const float* v = vs + 3 * faces[3 * f + c];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        b[x] = fminf(b[x], v[x]);
        b[3 + x] = fmaxf(b[3 + x], v[x]);
      }
    }
  }
  int64_t code = parent_leaf[l];
  while (code >= 0) {
    store_box(nodes, code, b);
    const int64_t p = code >> 1;
    if (__hip_atomic_fetch_add(arrivals + p, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const float* sib = (const float*)&nodes[4 * p + 2 * (1 - (code & 1))];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      b[x] = fminf(b[x], __uint_as_float(__hip_atomic_load((unsigned*)(sib + x), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT)));
      b[3 + x] = fmaxf(b[3 + x], __uint_as_float(__hip_atomic_load((unsigned*)(sib + 4 + x), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT)));
    }
    code = parent_node[p];
  }
}

__global__ void point_keys(const float* __restrict__ pts, int64_t N, const float* __restrict__ bounds,
                           uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  keys[i] = morton(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], bounds, 10) << 32 | (uint64_t)i;
}

__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// q - (closest point of the segment s0 + t d, t in [0, 1]); a zero-length segment is its point.
__device__ __forceinline__ float3 seg_offset(float3 q, float3 s0, float3 d) {
  const float3 w = sub3(q, s0);
  const float dd = dot3(d, d);
  float t = dd > 0.f ? dot3(w, d) / dd : 0.f;
  t = fminf(fmaxf(t, 0.f), 1.f);
  return make_float3(w.x - t * d.x, w.y - t * d.y, w.z - t * d.z);
}

// Offset r = p - closest point of the triangle (0, e1, e2), p in the local frame; *below = dot(e1 x e2, r) < 0.
// Inside the triangle's prism the closest point is p's projection onto the plane; elsewhere (and for a zero-area
// triangle: collinear or repeated vertices) it lies on one of the three edges.
//
// The normal and everything derived from it (the barycentrics, the plane offset, the side) are float64 on the float32
// p, e1, e2.  A product of two float32 is exact in float64, so n = e1 x e2 keeps a relative error of 2^-52 / sin(angle
// of e1, e2); in float32 it is 2^-23 / sin, and the plane distance of a point over the far end of a needle of length l
// was off by 1e-7 l / sin: beyond 1e-5 l from sin = 1e-3 down.  The edge offsets do not involve n and stay float32.
__device__ __forceinline__ float3 tri_offset(float3 p, float3 e1, float3 e2, bool* below) {
  const double px = p.x, py = p.y, pz = p.z, ax = e1.x, ay = e1.y, az = e1.z, bx = e2.x, by = e2.y, bz = e2.z;
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double nn = nx * nx + ny * ny + nz * nz;
  const float3 zero = make_float3(0.f, 0.f, 0.f);
  float3 r = seg_offset(p, zero, e1);
  float best = dot3(r, r);
  const float3 r2 = seg_offset(p, zero, e2);
  const float d2 = dot3(r2, r2);
  if (d2 < best) { r = r2; best = d2; }
  const float3 r3 = seg_offset(p, e1, sub3(e2, e1));
  const float d3 = dot3(r3, r3);
  if (d3 < best) { r = r3; best = d3; }
  // a sliver whose normal is below rounding (sin of its angle < 1e-5) counts as degenerate: its edges are then within
  // 5e-6 of its size of every point of it
  if (nn > 1e-10 * (ax * ax + ay * ay + az * az) * (bx * bx + by * by + bz * bz)) {
    // the barycentrics times nn: dot(p x e2, n) and dot(e1 x p, n)
    const double b1 = (py * bz - pz * by) * nx + (pz * bx - px * bz) * ny + (px * by - py * bx) * nz;
    const double b2 = (ay * pz - az * py) * nx + (az * px - ax * pz) * ny + (ax * py - ay * px) * nz;
    if (b1 >= 0.0 && b2 >= 0.0 && b1 + b2 <= nn) {
      const double h = (px * nx + py * ny + pz * nz) / nn;
      const float3 rp = make_float3((float)(h * nx), (float)(h * ny), (float)(h * nz));
      if (dot3(rp, rp) <= best) r = rp;
    }
  }
  *below = nx * r.x + ny * r.y + nz * r.z < 0.0;
  return r;
}

__device__ __forceinline__ float box_dist(float4 lo, float4 hi, float3 p) {
  const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.f);
  const float dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.f);
  const float dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.f);
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

struct Best {
  float d = INFINITY;
  int face = 0x7fffffff;
  bool below = false;   // the point is on the negative side of the face's normal
  float3 c = make_float3(0.f, 0.f, 0.f);
};

__device__ __forceinline__ void test_leaf(const float4* __restrict__ tri, int64_t F, int leaf, float3 p, Best& best) {
  const int64_t k0 = (int64_t)leaf * kLeaf;
  const int64_t k1 = k0 + kLeaf < F ? k0 + kLeaf : F;
  for (int64_t k = k0; k < k1; ++k) {
    const float4 a = tri[3 * k], e1 = tri[3 * k + 1], e2 = tri[3 * k + 2];
    const float3 q = make_float3(p.x - a.x, p.y - a.y, p.z - a.z);
    bool below;
    const float3 r = tri_offset(q, make_float3(e1.x, e1.y, e1.z), make_float3(e2.x, e2.y, e2.z), &below);
    const float d = sqrtf(dot3(r, r));
    const int f = __float_as_int(a.w);
    if (d < best.d || (d == best.d && f < best.face)) {     // ties: the lowest face index
      best.d = d;
      best.face = f;
      best.below = below;
      best.c = make_float3(p.x - r.x, p.y - r.y, p.z - r.z);
    }
  }
}

__global__ __launch_bounds__(kQueryThreads) void surface_query(const float4* __restrict__ nodes,
                                                              const float4* __restrict__ tri, int64_t F,
                                                              const uint64_t* __restrict__ order, int64_t N,
                                                              const float* __restrict__ pts, int signed_dist,
                                                              float* __restrict__ dist, int32_t* __restrict__ face,
                                                              float* __restrict__ closest) {
  __shared__ int stack[kStack][kQueryThreads];
  const int lane = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * kQueryThreads + lane;
  if (t >= N) return;
  const int64_t i = (int64_t)(order[t] & 0xffffffffull);
  const float3 p = make_float3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) {   // no distance to compare: (inf, no face, nan), and no walk
    dist[i] = INFINITY;
    face[i] = 0x7fffffff;
    if (closest) closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = __int_as_float(0x7fc00000);
    return;
  }
  Best best;
  int cur = 0, sp = 0;
  while (true) {
    const float4* nd = nodes + 4 * (int64_t)cur;
    const float4 lo0 = nd[0], hi0 = nd[1], lo1 = nd[2], hi1 = nd[3];
    const int c0 = __float_as_int(lo0.w), c1 = __float_as_int(lo1.w);
    const float d0 = box_dist(lo0, hi0, p), d1 = box_dist(lo1, hi1, p);
    if (c0 < 0 && d0 <= best.d) test_leaf(tri, F, ~c0, p, best);
    if (c1 < 0 && d1 <= best.d) test_leaf(tri, F, ~c1, p, best);
    const bool go0 = c0 >= 0 && d0 <= best.d, go1 = c1 >= 0 && d1 <= best.d;
    if (go0 && go1) {
      const bool first0 = d0 <= d1;
      if (sp < kStack) stack[sp++][lane] = first0 ? c1 : c0;   // never full: the tree is at most kStack levels deep
      cur = first0 ? c0 : c1;
    } else if (go0) {
      cur = c0;
    } else if (go1) {
      cur = c1;
    } else if (sp > 0) {
      cur = stack[--sp][lane];
    } else {
      break;
    }
  }
  float d = best.d;
  if (signed_dist && best.below && d > 0.f) d = -d;     // sign of dot(n, p - closest); a zero distance is +0
  dist[i] = d;
  face[i] = best.face;
  if (closest) {
    closest[3 * i] = best.c.x;
    closest[3 * i + 1] = best.c.y;
    closest[3 * i + 2] = best.c.z;
  }
}

// Metric partials, one fused pass over the N vertices of gt: sum |q|, sum |q| over the hole, the hole count, and
// the vertices' box.  hole[i] = hole_in[i] when given, else q_org[i] > eps.
__global__ void metric_partial(const float* __restrict__ q, const float* __restrict__ q_org, float eps,
                               const uint8_t* __restrict__ hole_in, const float* __restrict__ vs, int64_t N,
                               uint8_t* __restrict__ hole_out, double* __restrict__ part) {
  __shared__ double s[9][kThreads];
  double v[9] = {0.0, 0.0, 0.0, INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const bool h = hole_in ? hole_in[i] != 0 : q_org[i] > eps;
    if (hole_out) hole_out[i] = h ? 1 : 0;
    const double a = fabs((double)q[i]);
    v[0] += a;
    if (h) {
      v[1] += a;
      v[2] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[3 + k] = fmin(v[3 + k], (double)vs[3 * i + k]);
      v[6 + k] = fmax(v[6 + k], (double)vs[3 * i + k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + w];
#pragma unroll
      for (int k = 3; k < 6; ++k) s[k][threadIdx.x] = fmin(s[k][threadIdx.x], s[k][threadIdx.x + w]);
#pragma unroll
      for (int k = 6; k < 9; ++k) s[k][threadIdx.x] = fmax(s[k][threadIdx.x], s[k][threadIdx.x + w]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 9) part[9 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

// Fixed-order finish: out = (sum |q|, sum |q[hole]|, n_hole, diag).
__global__ void metric_finish(const double* __restrict__ part, int nb, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double v[9] = {0.0, 0.0, 0.0, INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int b = 0; b < nb; ++b) {
    for (int k = 0; k < 3; ++k) v[k] += part[9 * b + k];
    for (int k = 3; k < 6; ++k) v[k] = fmin(v[k], part[9 * b + k]);
    for (int k = 6; k < 9; ++k) v[k] = fmax(v[k], part[9 * b + k]);
  }
  const double dx = v[6] - v[3], dy = v[7] - v[4], dz = v[8] - v[5];
  out[0] = v[0];
  out[1] = v[1];
  out[2] = v[2];
  out[3] = sqrt(dx * dx + dy * dy + dz * dz);
}

}  // namespace

void destroy_surface(sg_surface* s) { delete s; }

int surface_create(const float* vs, int64_t V, const int64_t* faces, int64_t F, hipStream_t stream, sg_surface** out) {
  SG_REQUIRE(F < ((int64_t)1 << 31) - kLeaf && V < ((int64_t)1 << 31), "sg_surface_create: sizes must fit int32");
  {   // the face-index check comes first: nothing below reads a vertex through an index before it has passed
    AsyncBuf<int> bad(stream);
    SG_HIP_TRY(bad.alloc(1));
    SG_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), stream));
    check_faces<<<blocks_for(3 * F), kThreads, 0, stream>>>(faces, 3 * F, V, bad.p);
    SG_HIP_TRY(hipGetLastError());
    int h_bad = 0;
    SG_HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    SG_HIP_TRY(hipStreamSynchronize(stream));
    SG_REQUIRE(!h_bad, "sg_surface_create: face refers to a vertex outside [0, %lld)", (long long)V);
  }
  std::unique_ptr<sg_surface> s(new (std::nothrow) sg_surface);
  SG_REQUIRE(s != nullptr, "sg_surface_create: out of host memory");
  const int64_t L = (F + kLeaf - 1) / kLeaf, n_nodes = L > 1 ? L - 1 : 1;
  s->V = V;
  s->F = F;
  s->L = L;
  SG_HIP_TRY(s->tri.alloc(3 * F));
  SG_HIP_TRY(s->nodes.alloc(4 * n_nodes));
  SG_HIP_TRY(s->bounds.alloc(6));

  const int nb = blocks_for(F) < kRedBlocks ? blocks_for(F) : kRedBlocks;
  AsyncBuf<float> part(stream);
  AsyncBuf<uint64_t> keys_a(stream), keys_b(stream);
  AsyncBuf<char> temp(stream);
  AsyncBuf<int64_t> pleaf(stream), pnode(stream);
  AsyncBuf<int> arrivals(stream);
  SG_HIP_TRY(part.alloc((size_t)nb * 6));
  bounds_partial<<<nb, kThreads, 0, stream>>>(vs, faces, F, part.p);
  bounds_finish<<<1, 64, 0, stream>>>(part.p, nb, s->bounds.p);
  SG_HIP_TRY(hipGetLastError());

  const int idx_bits = bits_for((uint64_t)F, 63);
  int mbits = (64 - idx_bits) / 3;
  if (mbits > 21) mbits = 21;
  SG_HIP_TRY(keys_a.alloc(F));
  SG_HIP_TRY(keys_b.alloc(F));
  face_keys<<<blocks_for(F), kThreads, 0, stream>>>(vs, faces, F, s->bounds.p, mbits, idx_bits, keys_a.p);
  SG_HIP_TRY(hipGetLastError());
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys_a.p, keys_b.p, (int)F, 0, 3 * mbits + idx_bits, stream));
  SG_HIP_TRY(temp.alloc(tb));
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, tb, keys_a.p, keys_b.p, (int)F, 0, 3 * mbits + idx_bits, stream));
  const uint64_t* keys = keys_b.p;
  gather_tris<<<blocks_for(F), kThreads, 0, stream>>>(vs, faces, F, keys, ((uint64_t)1 << idx_bits) - 1, s->tri.p);
  SG_HIP_TRY(hipGetLastError());

  SG_HIP_TRY(pleaf.alloc(L));
  SG_HIP_TRY(pnode.alloc(n_nodes));
  SG_HIP_TRY(arrivals.alloc(n_nodes));
  SG_HIP_TRY(hipMemsetAsync(arrivals.p, 0, (size_t)n_nodes * sizeof(int), stream));
  karras_nodes<<<blocks_for(n_nodes), kThreads, 0, stream>>>(keys, L, s->nodes.p, pleaf.p, pnode.p);
  refit<<<blocks_for(L), kThreads, 0, stream>>>(vs, faces, s->tri.p, F, L, pleaf.p, pnode.p, s->nodes.p, arrivals.p);
  SG_HIP_TRY(hipGetLastError());
  *out = s.release();
  return SG_OK;
}

int surface_query(const sg_surface* s, const float* pts, int64_t N, int signed_dist, float* dist, int32_t* face,
                  float* closest, hipStream_t stream) {
  SG_REQUIRE(N < ((int64_t)1 << 31), "sg_surface_query: N must fit int32");
  if (N == 0) return SG_OK;
  AsyncBuf<uint64_t> keys_a(stream), keys_b(stream);
  AsyncBuf<char> temp(stream);
  SG_HIP_TRY(keys_a.alloc(N));
  SG_HIP_TRY(keys_b.alloc(N));
  point_keys<<<blocks_for(N), kThreads, 0, stream>>>(pts, N, s->bounds.p, keys_a.p);
  SG_HIP_TRY(hipGetLastError());
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys_a.p, keys_b.p, (int)N, 0, 62, stream));
  SG_HIP_TRY(temp.alloc(tb));
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, tb, keys_a.p, keys_b.p, (int)N, 0, 62, stream));
  const int64_t nb = (N + kQueryThreads - 1) / kQueryThreads;
  surface_query<<<(unsigned)nb, kQueryThreads, 0, stream>>>(s->nodes.p, s->tri.p, s->F, keys_b.p, N, pts, signed_dist, dist,
                                                            face, closest);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

int mesh_distance_reduce(const float* q, const float* q_org, float eps, const uint8_t* hole_in, const float* gt_vs,
                         int64_t N, uint8_t* hole_out, double* out, hipStream_t stream) {
  const int nb = N == 0 ? 1 : (blocks_for(N) < kRedBlocks ? blocks_for(N) : kRedBlocks);
  AsyncBuf<double> part(stream);
  SG_HIP_TRY(part.alloc((size_t)nb * 9));
  metric_partial<<<nb, kThreads, 0, stream>>>(q, q_org, eps, hole_in, gt_vs, N, hole_out, part.p);
  metric_finish<<<1, 64, 0, stream>>>(part.p, nb, out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
