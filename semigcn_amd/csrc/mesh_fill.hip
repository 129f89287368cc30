// Hole filling on the device: boundary loops of a triangle list, and a ring patch for every loop.
//
// Replaces the hole-closing part of MeshFix.repair() in the reference's preprocess/prepare.py:28-33 (not its other repairs:
// self-intersections, component selection).  The construction is specified in semigcn_amd/holes.py; in short:
//
//   boundary  a directed half-edge (a, b) of a face without its opposite (b, a).  The 3 F half-edges are radix-sorted by
//             (lo, hi, direction), so both directions of an edge are neighbours; a repeated directed half-edge, or a vertex
//             with two outgoing boundary half-edges, makes the boundary unorderable and is counted, not walked.
//   loops     with one outgoing boundary half-edge per boundary vertex, next[b] = a is a permutation of the nb boundary
//             vertices.  ceil(log2 nb) rounds of pointer jumping carry (smallest vertex of the window, steps to it): after
//             them every vertex knows its loop's smallest vertex and its own rank from it.  No serial walk.
//   sizes     R(n) = max(1, (113 n + 355) / 710) rings, ring r of max(3, (2 n (R - r) + R) / (2 R)) vertices, the last ring
//             one vertex: integers only.  Exclusive scans over the loops give every loop its vertex, face and ring offsets.
//   vertices  one thread per new vertex: B(s) + (r / R) (c - B(s)), B the loop's polyline by float64 arc length.
//   faces     one thread per new face: strips between rings advance by floor((t + 1) m / (m + k)) > floor(t m / (m + k)).
//
// All of it is integer work and gathers bound by HBM traffic; the only sort of full size is the one over the half-edges.
#include <memory>
#include <new>

#include "mesh_common.h"

struct sg_fill {
  int64_t V = 0, F = 0, nb = 0, L = 0;
  int64_t n_dup = 0, n_bow = 0, bad_vertex = -1;
  sg::DeviceBuf<int64_t> loop_ptr;     // [L + 1]
  sg::DeviceBuf<int64_t> loop_verts;   // [nb]
  // sizes of the patches (fill_plan)
  bool planned = false;
  int64_t Vn = 0, Fn = 0, NR = 0;
  sg::DeviceBuf<uint8_t> filled;       // [L]
  sg::DeviceBuf<int64_t> counts;       // [3][L + 1]: new vertices, new faces, ring-table entries of every loop
  sg::DeviceBuf<int64_t> base;         // [3][L + 1]: their exclusive scans
  sg::DeviceBuf<int64_t> ring_v;       // [NR] per loop R + 1 entries: new vertices in rings 1 .. r
  sg::DeviceBuf<int64_t> ring_f;       // [NR] per loop R + 1 entries: new faces in strips 0 .. r - 1
  sg::DeviceBuf<double> cum;           // [nb] arc length from the loop's first vertex to vertex i
  sg::DeviceBuf<double> geo;           // [L][4] perimeter, centre x y z
};

namespace sg {
namespace {

// ---- the construction's integers -------------------------------------------------------------------------------------
__device__ inline int64_t ring_count(int64_t n) {
  const int64_t R = (113 * n + 355) / 710;       // round(n / (2 pi)): 113 / 710 = 1 / (2 * 355 / 113)
  return R < 1 ? 1 : R;
}

// ring 0 is the loop, ring R the centre vertex
__device__ inline int64_t ring_size(int64_t n, int64_t R, int64_t r) {
  if (r <= 0) return n;
  if (r >= R) return 1;
  const int64_t m = (2 * n * (R - r) + R) / (2 * R);
  return m < 3 ? 3 : m;
}

// largest q in [0, n) with a[q] <= x (a ascending, a[0] <= x)
__device__ inline int64_t last_not_above(const int64_t* __restrict__ a, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- boundary half-edges ---------------------------------------------------------------------------------------------
// Half-edge h = 3 f + i goes from a = faces[f][i] to b = faces[f][(i+1)%3]; key = lo << 33 | hi << 1 | (a > b).
// flags[0]: vertex id out of range; flags[1]: degenerate face (repeated vertex).
__global__ void fill_keys(const int64_t* __restrict__ faces, int64_t n_half, int64_t V, uint64_t* __restrict__ keys,
                          int* __restrict__ flags) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_half) return;
  const int64_t f = h / 3;
  const int i = (int)(h - 3 * f);
  const int64_t a = faces[3 * f + i], b = faces[3 * f + next3(i)];
  uint64_t key = ~0ull;
  if (a < 0 || a >= V || b < 0 || b >= V) {
    flags[0] = 1;
  } else {
    if (a == b) flags[1] = 1;
    const uint64_t lo = (uint64_t)(a < b ? a : b), hi = (uint64_t)(a < b ? b : a);
    key = (lo << 33) | (hi << 1) | (a > b ? 1ull : 0ull);
  }
  keys[h] = key;
}

__device__ inline uint64_t key_source(uint64_t k) { return (k & 1) ? ((k >> 1) & 0xffffffffull) : (k >> 33); }
__device__ inline uint64_t key_target(uint64_t k) { return (k & 1) ? (k >> 33) : ((k >> 1) & 0xffffffffull); }

// In the sorted keys the two directions of an edge are neighbours.  stats[0]: repeated directed half-edges;
// stats[2]: the smallest vertex that makes the boundary unorderable.
__global__ void mark_boundary(const uint64_t* __restrict__ keys, int64_t n, uint8_t* __restrict__ is_boundary,
                              unsigned long long* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint64_t k = keys[p];
  uint8_t out = 0;
  if (k != ~0ull) {
    if (p > 0 && keys[p - 1] == k) {
      atomicAdd(&stats[0], 1ull);
      atomicMin(&stats[2], (unsigned long long)key_source(k));
    } else {
      const uint64_t und = k >> 1;
      const bool before = p > 0 && keys[p - 1] != k && (keys[p - 1] >> 1) == und;
      const bool after = p + 1 < n && keys[p + 1] != k && (keys[p + 1] >> 1) == und;
      out = (before || after) ? 0 : 1;
    }
  }
  is_boundary[p] = out;
}

__global__ void directed_from_keys(const uint64_t* __restrict__ keys, int64_t n, uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (key_source(keys[i]) << 32) | key_target(keys[i]);
}

// bk: the boundary half-edges as a << 32 | b, ascending.  stats[1]: vertices with more than one outgoing boundary
// half-edge.  fwd = the position of the half-edge that leaves b; the loop runs against the mesh: next[fwd] = i.
// stats[3]: a boundary half-edge whose end has no outgoing one (cannot happen once stats[0] and stats[1] are zero).
__global__ void link_boundary(const uint64_t* __restrict__ bk, int64_t nb, int32_t* __restrict__ next,
                              unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const uint64_t a = bk[i] >> 32, b = bk[i] & 0xffffffffull;
  if (i > 0 && (bk[i - 1] >> 32) == a) {
    if (i < 2 || (bk[i - 2] >> 32) != a) atomicAdd(&stats[1], 1ull);
    atomicMin(&stats[2], (unsigned long long)a);
    return;
  }
  int64_t lo = 0, hi = nb;
  const uint64_t want = b << 32;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (bk[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= nb || (bk[lo] >> 32) != b) {
    atomicAdd(&stats[3], 1ull);
    return;
  }
  next[lo] = (int32_t)i;
}

// next must be a permutation before anything follows it: every entry in range (it was preset to -1)
__global__ void check_links(const int32_t* __restrict__ next, int64_t nb, unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  if (next[i] < 0 || next[i] >= nb) atomicAdd(&stats[3], 1ull);
}

// ---- loops: pointer jumping ------------------------------------------------------------------------------------------
// state[i] = (smallest position in the window of 2^k successors that starts at i) << 32 | steps from i to it.  Positions
// ascend with the vertex id, so the smallest position is the smallest vertex.
__global__ void jump_init(const int32_t* __restrict__ next, int64_t nb, uint64_t* __restrict__ state, int32_t* __restrict__ jump) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  state[i] = (uint64_t)i << 32;
  jump[i] = next[i];
}

__global__ void jump_round(const uint64_t* __restrict__ state, const int32_t* __restrict__ jump, int64_t nb, uint64_t span,
                           uint64_t* __restrict__ state_out, int32_t* __restrict__ jump_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const int32_t j = jump[i];
  const uint64_t mine = state[i], far = state[j] + span;     // steps < 2^31 + 2^31: stays in the low word
  state_out[i] = far < mine ? far : mine;
  jump_out[i] = jump[j];
}

__global__ void loop_heads(const uint64_t* __restrict__ state, int64_t nb, int64_t* __restrict__ is_head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  is_head[i] = (int64_t)(state[i] >> 32) == i ? 1 : 0;
}

// the vertex after the head is n - 1 steps away from it
__global__ void loop_sizes(const uint64_t* __restrict__ state, const int32_t* __restrict__ next, const int64_t* __restrict__ loop_of,
                           int64_t nb, int64_t L, int64_t* __restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb || (int64_t)(state[i] >> 32) != i) return;
  const int64_t l = loop_of[i];
  if (l >= 0 && l < L) sizes[l] = (int64_t)(state[next[i]] & 0xffffffffull) + 1;
}

__global__ void loop_scatter(const uint64_t* __restrict__ state, const int32_t* __restrict__ next, const int64_t* __restrict__ loop_of,
                             const uint64_t* __restrict__ bk, const int64_t* __restrict__ loop_ptr, int64_t nb, int64_t L,
                             int64_t* __restrict__ loop_verts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const int64_t head = (int64_t)(state[i] >> 32), d = (int64_t)(state[i] & 0xffffffffull);
  const int64_t l = loop_of[head];
  if (l < 0 || l >= L) return;
  const int64_t b0 = loop_ptr[l], n = loop_ptr[l + 1] - b0;
  const int64_t rank = d == 0 ? 0 : n - d;
  if (rank >= 0 && rank < n) loop_verts[b0 + rank] = (int64_t)(bk[i] >> 32);
}

// ---- patch sizes -----------------------------------------------------------------------------------------------------
// counts: [3][L + 1] new vertices, new faces, ring-table entries; entry L of each row is 0 (the scans end on the totals)
__global__ void patch_counts(const int64_t* __restrict__ loop_ptr, int64_t L, int64_t max_edges, uint8_t* __restrict__ filled,
                             int64_t* __restrict__ counts) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l > L) return;
  int64_t nv = 0, nf = 0, nr = 0;
  if (l < L) {
    const int64_t n = loop_ptr[l + 1] - loop_ptr[l];
    const bool fill = n >= 3 && (max_edges < 0 || n <= max_edges);
    filled[l] = fill ? 1 : 0;
    if (fill && n == 3) {
      nf = 1;
    } else if (fill) {
      const int64_t R = ring_count(n);
      nr = R + 1;
      int64_t m = n;
      for (int64_t r = 1; r <= R; ++r) {
        const int64_t k = ring_size(n, R, r);
        nv += k;
        nf += k == 1 ? m : m + k;
        m = k;
      }
    }
  }
  counts[l] = nv;
  counts[(L + 1) + l] = nf;
  counts[2 * (L + 1) + l] = nr;
}

__global__ void ring_tables(const int64_t* __restrict__ loop_ptr, int64_t L, const uint8_t* __restrict__ filled,
                            const int64_t* __restrict__ ring_base, int64_t NR, int64_t* __restrict__ ring_v,
                            int64_t* __restrict__ ring_f) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const int64_t n = loop_ptr[l + 1] - loop_ptr[l];
  if (!filled[l] || n <= 3) return;
  const int64_t R = ring_count(n), t0 = ring_base[l];
  if (t0 < 0 || t0 + R + 1 > NR) return;
  int64_t nv = 0, nf = 0, m = n;
  ring_v[t0] = 0;
  ring_f[t0] = 0;
  for (int64_t r = 1; r <= R; ++r) {
    const int64_t k = ring_size(n, R, r);
    nv += k;
    nf += k == 1 ? m : m + k;
    m = k;
    ring_v[t0 + r] = nv;
    ring_f[t0 + r] = nf;
  }
}

// ---- geometry --------------------------------------------------------------------------------------------------------
// One workgroup per loop: float64 arc length from the loop's first vertex to each of its vertices (chunks of kThreads
// edges, scanned in the block, carried from chunk to chunk: a fixed order), the perimeter and the mean of the vertices.
__global__ __launch_bounds__(kThreads) void loop_geometry(const float* __restrict__ vs, const int64_t* __restrict__ loop_ptr,
                                                          const int64_t* __restrict__ loop_verts, const uint8_t* __restrict__ filled,
                                                          double* __restrict__ cum, double* __restrict__ geo) {
  using Scan = hipcub::BlockScan<double, kThreads>;
  using Reduce = hipcub::BlockReduce<double, kThreads>;
  __shared__ typename Scan::TempStorage s_scan;
  __shared__ typename Reduce::TempStorage s_red;
  const int64_t l = blockIdx.x;
  const int64_t b0 = loop_ptr[l], n = loop_ptr[l + 1] - b0;
  if (!filled[l] || n <= 3) return;            // the same for every thread of the block
  double carry = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t c0 = 0; c0 < n; c0 += kThreads) {
    const int64_t i = c0 + threadIdx.x;
    double seg = 0.0;
    if (i < n) {
      const int64_t v0 = loop_verts[b0 + i], v1 = loop_verts[b0 + (i + 1 == n ? 0 : i + 1)];
      const double x0 = vs[3 * v0], y0 = vs[3 * v0 + 1], z0 = vs[3 * v0 + 2];
      const double dx = (double)vs[3 * v1] - x0, dy = (double)vs[3 * v1 + 1] - y0, dz = (double)vs[3 * v1 + 2] - z0;
      seg = sqrt(dx * dx + dy * dy + dz * dz);
      sx += x0;
      sy += y0;
      sz += z0;
    }
    double before, total;
    Scan(s_scan).ExclusiveSum(seg, before, total);
    if (i < n) cum[b0 + i] = carry + before;
    carry += total;
    __syncthreads();
  }
  sx = Reduce(s_red).Sum(sx);
  __syncthreads();
  sy = Reduce(s_red).Sum(sy);
  __syncthreads();
  sz = Reduce(s_red).Sum(sz);
  if (threadIdx.x == 0) {
    geo[4 * l] = carry;
    geo[4 * l + 1] = sx / (double)n;
    geo[4 * l + 2] = sy / (double)n;
    geo[4 * l + 3] = sz / (double)n;
  }
}

// One thread per new vertex g: loop by the vertex offsets, ring by the loop's ring table, index j inside the ring.
__global__ __launch_bounds__(kThreads) void emit_vertices(const float* __restrict__ vs, const int64_t* __restrict__ loop_ptr,
                                                          const int64_t* __restrict__ loop_verts, int64_t L,
                                                          const int64_t* __restrict__ vbase, const int64_t* __restrict__ rbase,
                                                          const int64_t* __restrict__ ring_v, const double* __restrict__ cum,
                                                          const double* __restrict__ geo, int64_t Vn, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= Vn) return;
  const int64_t l = last_not_above(vbase, L, g);
  const int64_t b0 = loop_ptr[l], n = loop_ptr[l + 1] - b0;
  const int64_t R = ring_count(n);
  const int64_t* rv = ring_v + rbase[l];
  const int64_t local = g - vbase[l];
  const int64_t q = last_not_above(rv, R, local);
  const int64_t r = q + 1, j = local - rv[q];
  const double cx = geo[4 * l + 1], cy = geo[4 * l + 2], cz = geo[4 * l + 3];
  double x = cx, y = cy, z = cz;
  if (r < R) {
    const int64_t m = ring_size(n, R, r);
    const double perim = geo[4 * l];
    const double s = (double)j / (double)m * perim;
    // the segment i with cum[i] <= s < cum[i + 1]
    const double* c = cum + b0;
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (c[mid] <= s) lo = mid;
      else hi = mid;
    }
    const int64_t i0 = lo, i1 = lo + 1 == n ? 0 : lo + 1;
    const double seg = (i1 == 0 ? perim : c[i1]) - c[i0];
    const double t = seg > 0.0 ? (s - c[i0]) / seg : 0.0;
    const int64_t v0 = loop_verts[b0 + i0], v1 = loop_verts[b0 + i1];
    const double bx = (double)vs[3 * v0] * (1.0 - t) + (double)vs[3 * v1] * t;
    const double by = (double)vs[3 * v0 + 1] * (1.0 - t) + (double)vs[3 * v1 + 1] * t;
    const double bz = (double)vs[3 * v0 + 2] * (1.0 - t) + (double)vs[3 * v1 + 2] * t;
    const double w = (double)r / (double)R;
    x = bx + w * (cx - bx);
    y = by + w * (cy - by);
    z = bz + w * (cz - bz);
  }
  out[3 * g] = (float)x;
  out[3 * g + 1] = (float)y;
  out[3 * g + 2] = (float)z;
}

// One thread per new face g: loop by the face offsets, strip by the loop's ring table, step t inside the strip.
__global__ __launch_bounds__(kThreads) void emit_faces(const int64_t* __restrict__ loop_ptr, const int64_t* __restrict__ loop_verts,
                                                       int64_t L, int64_t V, const int64_t* __restrict__ vbase,
                                                       const int64_t* __restrict__ fbase, const int64_t* __restrict__ rbase,
                                                       const int64_t* __restrict__ ring_v, const int64_t* __restrict__ ring_f,
                                                       int64_t Fn, int64_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= Fn) return;
  const int64_t l = last_not_above(fbase, L, g);
  const int64_t b0 = loop_ptr[l], n = loop_ptr[l + 1] - b0;
  const int64_t* lv = loop_verts + b0;
  int64_t f0, f1, f2;
  if (n == 3) {
    f0 = lv[0], f1 = lv[1], f2 = lv[2];
  } else {
    const int64_t R = ring_count(n);
    const int64_t* rv = ring_v + rbase[l];
    const int64_t* rf = ring_f + rbase[l];
    const int64_t local = g - fbase[l];
    const int64_t r = last_not_above(rf, R, local);          // the strip between rings r and r + 1
    const int64_t t = local - rf[r];
    const int64_t m = ring_size(n, R, r), k = ring_size(n, R, r + 1);
    const int64_t first_new = V + vbase[l];
    const int64_t inner0 = first_new + rv[r];                // ring r + 1 starts after rings 1 .. r
    const int64_t outer0 = r == 0 ? 0 : first_new + rv[r - 1];
    auto outer = [&](int64_t a) { return r == 0 ? lv[a] : outer0 + a; };
    if (k == 1) {
      f0 = outer(t), f1 = outer(t + 1 == m ? 0 : t + 1), f2 = inner0;
    } else {
      const int64_t N = m + k;
      const int64_t A = (t * m) / N, A1 = ((t + 1) * m) / N, B = t - A;
      if (A1 > A) f0 = outer(A % m), f1 = outer((A + 1) % m), f2 = inner0 + B % k;
      else f0 = outer(A % m), f1 = inner0 + (B + 1) % k, f2 = inner0 + B % k;
    }
  }
  out[3 * g] = f0;
  out[3 * g + 1] = f1;
  out[3 * g + 2] = f2;
}

void free_sizes(sg_fill* s) {
  s->filled.reset();
  s->counts.reset();
  s->base.reset();
  s->ring_v.reset();
  s->ring_f.reset();
  s->cum.reset();
  s->geo.reset();
  s->planned = false;
  s->Vn = s->Fn = s->NR = 0;
}

// the sizes of fill_plan for L > 0 loops; on an error the caller drops what was allocated
int size_patches(sg_fill* s, int64_t max_hole_edges, hipStream_t stream) {
  const int64_t L = s->L, W = L + 1;
  SG_HIP_TRY(s->filled.alloc(L));
  SG_HIP_TRY(s->counts.alloc(3 * W));
  SG_HIP_TRY(s->base.alloc(3 * W));
  SG_HIP_TRY(s->cum.alloc(s->nb));
  SG_HIP_TRY(s->geo.alloc(4 * L));
  patch_counts<<<blocks_for(W), kThreads, 0, stream>>>(s->loop_ptr.p, L, max_hole_edges, s->filled.p, s->counts.p);
  SG_HIP_TRY(hipGetLastError());
  int64_t totals[3] = {0, 0, 0};
  for (int q = 0; q < 3; ++q) {
    if (int rc = exclusive_sum(s->counts.p + q * W, s->base.p + q * W, W, stream)) return rc;
    SG_HIP_TRY(hipMemcpyAsync(&totals[q], s->base.p + q * W + L, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  }
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(totals[0] >= 0 && totals[1] >= 0 && totals[2] >= 0, "sg_fill_plan: negative totals");
  SG_REQUIRE(s->V + totals[0] < ((int64_t)1 << 31) && 3 * (s->F + totals[1]) < ((int64_t)1 << 31),
             "sg_fill_plan: the filled mesh must fit int32");
  s->Vn = totals[0];
  s->Fn = totals[1];
  s->NR = totals[2];
  if (s->NR > 0) {
    SG_HIP_TRY(s->ring_v.alloc(s->NR));
    SG_HIP_TRY(s->ring_f.alloc(s->NR));
    ring_tables<<<blocks_for(L), kThreads, 0, stream>>>(s->loop_ptr.p, L, s->filled.p, s->base.p + 2 * W, s->NR, s->ring_v.p,
                                                       s->ring_f.p);
    SG_HIP_TRY(hipGetLastError());
  }
  return SG_OK;
}

}  // namespace

void destroy_fill(sg_fill* s) { delete s; }

int fill_create(const int64_t* faces, int64_t F, int64_t V, hipStream_t stream, sg_fill** out) {
  const int64_t n_half = 3 * F;
  SG_REQUIRE(V < ((int64_t)1 << 31) && n_half < ((int64_t)1 << 31), "sg_fill_create: sizes must fit int32");
  std::unique_ptr<sg_fill> s(new (std::nothrow) sg_fill);
  SG_REQUIRE(s != nullptr, "sg_fill_create: out of host memory");
  s->V = V;
  s->F = F;
  SG_HIP_TRY(s->loop_ptr.alloc(1));
  SG_HIP_TRY(hipMemsetAsync(s->loop_ptr.p, 0, sizeof(int64_t), stream));
  if (F == 0) {
    SG_HIP_TRY(hipStreamSynchronize(stream));
    *out = s.release();
    return SG_OK;
  }

  DeviceBuf<uint64_t> keys_a, keys_b, picked;
  DeviceBuf<uint8_t> marks;
  DeviceBuf<int> count, flags;
  DeviceBuf<unsigned long long> stats;
  DeviceBuf<char> temp;
  int h_flags[2] = {0, 0}, h_count = 0;
  unsigned long long h_stats[4] = {0, 0, ~0ull, 0};
  SG_HIP_TRY(keys_a.alloc(n_half));
  SG_HIP_TRY(keys_b.alloc(n_half));
  SG_HIP_TRY(marks.alloc(n_half));
  SG_HIP_TRY(picked.alloc(n_half));
  SG_HIP_TRY(count.alloc(1));
  SG_HIP_TRY(flags.alloc(2));
  SG_HIP_TRY(stats.alloc(4));
  SG_HIP_TRY(hipMemsetAsync(flags.p, 0, sizeof(h_flags), stream));
  SG_HIP_TRY(hipMemcpyAsync(stats.p, h_stats, sizeof(h_stats), hipMemcpyHostToDevice, stream));
  fill_keys<<<blocks_for(n_half), kThreads, 0, stream>>>(faces, n_half, V, keys_a.p, flags.p);
  SG_HIP_TRY(hipGetLastError());
  const int hi_bits = bits_for((uint64_t)V, 31);
  const uint64_t* sorted = keys_b.p;        // hipCUB's iterator arguments keep the const they had
  const uint8_t* is_boundary = marks.p;
  size_t t1 = 0, t2 = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, t1, keys_a.p, keys_b.p, (int)n_half, 0, 33 + hi_bits, stream));
  SG_HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, t2, sorted, is_boundary, picked.p, count.p, (int)n_half, stream));
  const size_t tb = t1 > t2 ? t1 : t2;
  SG_HIP_TRY(temp.alloc(tb ? tb : 16));
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, t1, keys_a.p, keys_b.p, (int)n_half, 0, 33 + hi_bits, stream));
  mark_boundary<<<blocks_for(n_half), kThreads, 0, stream>>>(keys_b.p, n_half, marks.p, stats.p);
  SG_HIP_TRY(hipGetLastError());
  SG_HIP_TRY(hipcub::DeviceSelect::Flagged(temp.p, t2, sorted, is_boundary, picked.p, count.p, (int)n_half, stream));
  SG_HIP_TRY(hipMemcpyAsync(&h_count, count.p, sizeof(int), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(!h_flags[0], "sg_fill_create: face refers to a vertex outside [0, %lld)", (long long)V);
  SG_REQUIRE(!h_flags[1], "sg_fill_create: degenerate face (repeated vertex)");
  SG_REQUIRE(h_count >= 0 && h_count <= n_half, "sg_fill_create: boundary count %d out of range", h_count);
  const int64_t nb = h_count;

  // the boundary half-edges as a << 32 | b, ascending: the sources are then the boundary vertices in ascending order
  DeviceBuf<uint64_t> bk;
  DeviceBuf<int32_t> next;
  if (nb > 0) {
    SG_HIP_TRY(bk.alloc(nb));
    SG_HIP_TRY(next.alloc(nb));
    uint64_t* unsorted = keys_a.p;                      // the full-size buffers are free again
    directed_from_keys<<<blocks_for(nb), kThreads, 0, stream>>>(picked.p, nb, unsorted);
    SG_HIP_TRY(hipGetLastError());
    size_t t3 = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, t3, unsorted, bk.p, (int)nb, 0, 64, stream));
    DeviceBuf<char> temp3;
    SG_HIP_TRY(temp3.alloc(t3 ? t3 : 16));
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp3.p, t3, unsorted, bk.p, (int)nb, 0, 64, stream));
    SG_HIP_TRY(hipMemsetAsync(next.p, 0xff, (size_t)nb * sizeof(int32_t), stream));
    link_boundary<<<blocks_for(nb), kThreads, 0, stream>>>(bk.p, nb, next.p, stats.p);
    check_links<<<blocks_for(nb), kThreads, 0, stream>>>(next.p, nb, stats.p);
    SG_HIP_TRY(hipGetLastError());
    SG_HIP_TRY(hipStreamSynchronize(stream));           // temp3 is freed here
  }
  SG_HIP_TRY(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  s->n_dup = (int64_t)h_stats[0];
  s->n_bow = (int64_t)h_stats[1];
  if (s->n_dup || s->n_bow) {                           // unorderable: reported by sg_fill_query, nothing is walked
    s->bad_vertex = (int64_t)h_stats[2];
    *out = s.release();
    return SG_OK;
  }
  SG_REQUIRE(h_stats[3] == 0, "sg_fill_create: the boundary half-edges do not form a permutation (%llu broken links)",
             h_stats[3]);
  if (nb == 0) {
    *out = s.release();
    return SG_OK;
  }

  // pointer jumping: after `rounds` rounds the window of every vertex is at least as long as the longest loop can be
  DeviceBuf<uint64_t> st_a, st_b;
  DeviceBuf<int32_t> jp_a, jp_b;
  DeviceBuf<int64_t> heads, loop_of, sizes;
  SG_HIP_TRY(st_a.alloc(nb));
  SG_HIP_TRY(st_b.alloc(nb));
  SG_HIP_TRY(jp_a.alloc(nb));
  SG_HIP_TRY(jp_b.alloc(nb));
  SG_HIP_TRY(heads.alloc(nb + 1));
  SG_HIP_TRY(loop_of.alloc(nb + 1));
  uint64_t* st = st_a.p;
  uint64_t* st_o = st_b.p;
  int32_t* jp = jp_a.p;
  int32_t* jp_o = jp_b.p;
  jump_init<<<blocks_for(nb), kThreads, 0, stream>>>(next.p, nb, st, jp);
  for (uint64_t span = 1; span < (uint64_t)nb; span <<= 1) {
    jump_round<<<blocks_for(nb), kThreads, 0, stream>>>(st, jp, nb, span, st_o, jp_o);
    uint64_t* ts = st; st = st_o; st_o = ts;
    int32_t* tj = jp; jp = jp_o; jp_o = tj;
  }
  SG_HIP_TRY(hipGetLastError());
  SG_HIP_TRY(hipMemsetAsync(heads.p + nb, 0, sizeof(int64_t), stream));
  loop_heads<<<blocks_for(nb), kThreads, 0, stream>>>(st, nb, heads.p);
  SG_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_sum(heads.p, loop_of.p, nb + 1, stream)) return rc;
  int64_t L = 0;
  SG_HIP_TRY(hipMemcpyAsync(&L, loop_of.p + nb, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(L >= 1 && L <= nb, "sg_fill_create: loop count %lld out of range", (long long)L);

  SG_HIP_TRY(sizes.alloc(L + 1));
  SG_HIP_TRY(hipMemsetAsync(sizes.p, 0, (size_t)(L + 1) * sizeof(int64_t), stream));
  loop_sizes<<<blocks_for(nb), kThreads, 0, stream>>>(st, next.p, loop_of.p, nb, L, sizes.p);
  SG_HIP_TRY(hipGetLastError());
  SG_HIP_TRY(s->loop_ptr.alloc(L + 1));                 // releases the one-entry table of above
  SG_HIP_TRY(s->loop_verts.alloc(nb));
  if (int rc = exclusive_sum(sizes.p, s->loop_ptr.p, L + 1, stream)) return rc;
  int64_t total = 0;
  SG_HIP_TRY(hipMemcpyAsync(&total, s->loop_ptr.p + L, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(total == nb, "sg_fill_create: the loops hold %lld vertices, the boundary %lld", (long long)total, (long long)nb);
  SG_HIP_TRY(hipMemsetAsync(s->loop_verts.p, 0xff, (size_t)nb * sizeof(int64_t), stream));
  loop_scatter<<<blocks_for(nb), kThreads, 0, stream>>>(st, next.p, loop_of.p, bk.p, s->loop_ptr.p, nb, L, s->loop_verts.p);
  SG_HIP_TRY(hipGetLastError());
  SG_HIP_TRY(hipStreamSynchronize(stream));             // the temporaries are freed on return
  s->nb = nb;
  s->L = L;
  *out = s.release();
  return SG_OK;
}

int fill_plan(sg_fill* s, int64_t max_hole_edges, hipStream_t stream, int64_t* n_new_vertices, int64_t* n_new_faces) {
  SG_REQUIRE(!s->n_dup && !s->n_bow, "sg_fill_plan: the boundary is unorderable (see sg_fill_query)");
  free_sizes(s);
  *n_new_vertices = *n_new_faces = 0;
  if (s->L > 0) {
    if (int rc = size_patches(s, max_hole_edges, stream)) {
      free_sizes(s);
      return rc;
    }
  }
  s->planned = true;
  *n_new_vertices = s->Vn;
  *n_new_faces = s->Fn;
  return SG_OK;
}

int fill_emit(sg_fill* s, const float* vs, float* new_vs, int64_t* new_faces, uint8_t* filled_out, hipStream_t stream) {
  SG_REQUIRE(s->planned, "sg_fill_emit: call sg_fill_plan first");
  const int64_t L = s->L, W = L + 1;
  if (L == 0) return SG_OK;
  SG_REQUIRE(filled_out != nullptr && vs != nullptr, "sg_fill_emit: null pointer");
  SG_REQUIRE((s->Vn == 0 || new_vs) && (s->Fn == 0 || new_faces), "sg_fill_emit: null pointer");
  SG_HIP_TRY(hipMemcpyAsync(filled_out, s->filled.p, (size_t)L, hipMemcpyDeviceToDevice, stream));
  if (s->Vn > 0) {
    loop_geometry<<<(unsigned)L, kThreads, 0, stream>>>(vs, s->loop_ptr.p, s->loop_verts.p, s->filled.p, s->cum.p, s->geo.p);
    emit_vertices<<<blocks_for(s->Vn), kThreads, 0, stream>>>(vs, s->loop_ptr.p, s->loop_verts.p, L, s->base.p, s->base.p + 2 * W,
                                                             s->ring_v.p, s->cum.p, s->geo.p, s->Vn, new_vs);
  }
  if (s->Fn > 0)
    emit_faces<<<blocks_for(s->Fn), kThreads, 0, stream>>>(s->loop_ptr.p, s->loop_verts.p, L, s->V, s->base.p, s->base.p + W,
                                                          s->base.p + 2 * W, s->ring_v.p, s->ring_f.p, s->Fn, new_faces);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

void fill_query(const sg_fill* s, int64_t* info) {
  info[0] = s->L;
  info[1] = s->nb;
  info[2] = s->n_dup;
  info[3] = s->n_bow;
  info[4] = s->bad_vertex;
  info[5] = s->planned ? s->Vn : -1;
  info[6] = s->planned ? s->Fn : -1;
  info[7] = s->V;
}

int fill_loops(const sg_fill* s, int64_t* loop_ptr_out, int64_t* loop_verts_out, hipStream_t stream) {
  SG_REQUIRE(!s->n_dup && !s->n_bow, "sg_fill_loops: the boundary is unorderable (see sg_fill_query)");
  SG_HIP_TRY(hipMemcpyAsync(loop_ptr_out, s->loop_ptr.p, (size_t)(s->L + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  if (s->nb > 0)
    SG_HIP_TRY(hipMemcpyAsync(loop_verts_out, s->loop_verts.p, (size_t)s->nb * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  return SG_OK;
}

}  // namespace sg
