// Refining a triangle mesh to a target edge length on the device: split long edges, collapse short ones, flip edges towards
// regular valence.
//
// Replaces the splitting, collapsing and flipping of the isotropic remesh the reference runs between MeshFix and the scaling
// (preprocess/prepare.py:35-42); the relaxation / re-projection is plumbing over mesh_smooth.hip and mesh_dist.hip.  The specification is semigcn_amd/remesh.py; in short:
//
//   analysis   every round starts from the same analysis of the mesh it finds: half-edge h = 3 f + k is keyed lo * V + hi
//              (undirected) with h as the value; one radix sort over the 3 F pairs, restricted to the bits V * V needs, puts
//              the faces of an edge side by side (the sort is stable: a run lists its half-edges in ascending h).  Run
//              heads, an inclusive scan of the heads (the edge rank r in ascending (lo, hi) order), the rank of every
//              half-edge, border vertices, and -- only ever non-zero for the caller's input -- the counts of edges with
//              three or more faces, of pairs that run an edge in the same direction, and the smallest such edge.
//   split      face pass: the long edge of highest priority (len2 bits << 32 | hash(r)) of every face.  Edge pass: a long
//              edge is selected when it is that edge in each of its faces, and marks its faces.  Two exclusive scans number
//              the selected edges (new vertex V + s) and the split faces (new face F + t); ONE host synchronisation reads
//              both totals, grows the buffers when needed, and the emit writes midpoints, parents and faces in place.
//   flip       valence by integer atomicAdd per edge end; candidates with their gain and guard, keyed gain << 32 | hash(r),
//              a 64-bit atomicMax of the key into the slot of each of the four vertices; a check pass (a candidate wins when
//              all four slots hold its key); ONE host synchronisation reads the number of winners and the deviation; the
//              apply pass rewrites the two faces of every winner.  Winners are vertex-disjoint, hence face-disjoint.
//   collapse   the analysis also records the twin of every half-edge.  Candidate pass: one lane per interior short edge walks
//              the fan of the removed vertex r through twin and next half-edges -- a counted loop of val[r] steps -- looks
//              every {k, w} up in the sorted keys, evaluates the guards and bids (0xFFFFFFFF - len2 bits) << 32 | hash(r) by
//              64-bit atomicMax into the slot of every vertex of its footprint {r} + ring(r); the check pass walks the same
//              fan (a candidate wins when every slot holds its key); ONE host synchronisation reads the winners and the
//              short edges; the apply pass marks the two faces of the edge and r dead and writes k over r in the other faces
//              at r; two exclusive scans over the keep flags; the compaction writes vs / par / tri / border into second
//              buffers (stable), which are then swapped in, and composes the vertex maps of the call.  A collapse reads and
//              writes only inside its footprint, so footprint-disjoint winners are independent.
//   creases    with sg_remesh_set_feature on, one more pass per analysis: one lane per interior edge compares the two face
//              normals with the feature angle (float64 products, no root, no epsilon), flags the edge at the head of its run
//              and counts it at both ends (integer atomicAdd / atomicMin / atomicMax).  A flagged edge is no flip candidate;
//              the collapse keeps the end the creases choose, never removes a corner, and removes a crease-line vertex only
//              along its crease and only forwards.  Off, no launch is added and the kernels see null pointers.
//   simplify   (semigcn_amd/simplify.py) quadric edge collapse to a vertex budget on the same plan.  Once per call: one stable
//              sort of the 3 F corners by vertex and one lane per vertex sum the face quadrics p p^T / (n . n) in ascending
//              face index (float64, ten divisions per face, no root).  A round: the collapse analysis; a price pass, one lane
//              per interior edge, walks the fans of r and of k, evaluates link, valence floors and the fold-over guard at the
//              position k will have, and keys the edge (0xFFFFFFFF - bits(float32(cost))) << 32 | hash(rank); one radix sort
//              of the keys and a one-lane kernel leave the cut of the min(need, candidates) highest in device memory; the bid
//              pass (64-bit atomicMax over {k, r} + ring(k) + ring(r)) and the check pass read it there; ONE host
//              synchronisation reads candidates, admitted and winners; the apply and compaction are the collapse's, after k
//              has moved to the midpoint, and the quadrics are compacted with the vertices.
//
// hash is the 32-bit mixer x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16: a bijection, so two
// edges never tie and the order in which the atomics arrive cannot matter.  There are no float atomics; integer max and
// integer sums do not depend on order: every output is deterministic.  The float arithmetic is the squared length, the
// midpoint and the float64 guard, each a fixed sequence of multiplies and adds: this file is built with -ffp-contract=off.
#include <initializer_list>
#include <memory>
#include <new>

#include "mesh_common.h"

namespace sg {
namespace {

// slots of the counter block
enum {
  kOutOfRange = 0, kDegenerate, kBadFace, kNonFinite, kBadVertex, kNonManifold, kMisoriented, kBadKey, kBorderEdges, kEdges,
  kLong, kWinners, kDeviation, kTotalA, kTotalF, kShort, kCounters = 16
};

}  // namespace
}  // namespace sg

struct sg_remesh {
  int64_t V = 0, F = 0, V0 = 0, F0 = 0;
  unsigned long long h_ctr[sg::kCounters] = {};     // the counters of the creating analysis (validation)
  int64_t bad_key_V = 0;                            // the V that the smallest offending key was formed with
  bool valid = false;
  sg::GrowBuf<float> vs;                            // the mesh: [V][3]
  sg::GrowBuf<int32_t> par, tri;                    // [V][2], [F][3]
  sg::GrowBuf<uint8_t> border;                      // [V]
  sg::GrowBuf<uint64_t> keys_a, keys_b;
  sg::GrowBuf<int32_t> vals_a, vals_b, head, incl, he_rank, best, fpos, flag_a, scan_a, flag_f, scan_f, val;
  sg::GrowBuf<unsigned long long> cand, slot, ctr;
  sg::GrowBuf<uint8_t> win;
  sg::GrowBuf<char> temp;
  // collapse: the twin of every half-edge, keep flags and their scans over the vertices, where a removed vertex went, the
  // second buffers the compaction writes, and the maps of the last collapse call (ids: new -> before, into: before -> new)
  sg::GrowBuf<int32_t> twin, flag_v, scan_v, dest, par2, tri2, ids, ids2, into;
  sg::GrowBuf<float> vs2;
  sg::GrowBuf<uint8_t> border2;
  sg::GrowBuf<double> quad, quad2;                  // simplify: the vertex quadrics [V][10], and where the compaction writes them
  bool quad_fresh = false;                          // quad holds the quadrics of the mesh as it stands (sg_remesh_quadrics just ran)
  int64_t map_before = -1, map_after = -1;          // sizes of the maps; -1: no collapse call yet, both are the identity
  // creases (sg_remesh_set_feature): with `feat` every analysis flags the crease edges at the heads of their runs and, per
  // vertex, counts them (nc) and keeps the smallest and the largest crease neighbour (clo, chi)
  bool feat = false;
  double cos_t = 0.0;
  sg::GrowBuf<uint8_t> crease;                      // [3 F]
  sg::GrowBuf<int32_t> nc, clo, chi;                // [V]
  int64_t feat_C = -1;                              // crease edges of the last sg_remesh_features; -1: the analysis moved on
};

namespace sg {
namespace {

constexpr float kHalf = 0.5f;

__device__ inline uint32_t hash32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// len2 of the edge {a, b}: d = vs[hi] - vs[lo], dx * dx + dy * dy + dz * dz, left to right, float32
__device__ inline float edge_len2(const float* __restrict__ vs, int32_t a, int32_t b) {
  const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
  const float dx = vs[3 * (int64_t)hi] - vs[3 * (int64_t)lo];
  const float dy = vs[3 * (int64_t)hi + 1] - vs[3 * (int64_t)lo + 1];
  const float dz = vs[3 * (int64_t)hi + 2] - vs[3 * (int64_t)lo + 2];
  return dx * dx + dy * dy + dz * dz;
}

// ---- the caller's input -------------------------------------------------------------------------------------------------
__global__ void reset_counters(unsigned long long* __restrict__ ctr) {
  const int i = threadIdx.x;
  if (i < kCounters) ctr[i] = (i == kBadFace || i == kBadVertex || i == kBadKey) ? ~0ull : 0ull;
}

// tri = the faces as int32 (zeros where an id is out of range); counts repeated vertices
__global__ void classify_faces(const int64_t* __restrict__ faces, int64_t F, int64_t V, int32_t* __restrict__ tri,
                               unsigned long long* __restrict__ ctr) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
    ctr[kOutOfRange] = 1;
    a = b = c = 0;
  } else if (a == b || b == c || c == a) {
    atomicAdd(&ctr[kDegenerate], 1ull);
    atomicMin(&ctr[kBadFace], (unsigned long long)f);
  }
  tri[3 * f] = (int32_t)a;
  tri[3 * f + 1] = (int32_t)b;
  tri[3 * f + 2] = (int32_t)c;
}

__global__ void check_vertices(const float* __restrict__ vs, int64_t V, int32_t* __restrict__ par,
                               unsigned long long* __restrict__ ctr) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  if (!(isfinite(vs[3 * v]) && isfinite(vs[3 * v + 1]) && isfinite(vs[3 * v + 2]))) {
    atomicAdd(&ctr[kNonFinite], 1ull);
    atomicMin(&ctr[kBadVertex], (unsigned long long)v);
  }
  par[2 * v] = par[2 * v + 1] = (int32_t)v;
}

// ---- analysis -------------------------------------------------------------------------------------------------------------
__global__ void half_edge_keys(const int32_t* __restrict__ tri, int64_t n_half, int64_t V, uint64_t* __restrict__ keys,
                               int32_t* __restrict__ vals) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_half) return;
  const int64_t f = h / 3;
  const int k = (int)(h - 3 * f);
  const int64_t a = tri[h], b = tri[3 * f + next3(k)];
  keys[h] = (uint64_t)(a < b ? a : b) * (uint64_t)V + (uint64_t)(a < b ? b : a);
  vals[h] = (int32_t)h;
}

__global__ void mark_heads(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ head) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  head[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
}

// faces of the run that starts at the head p (3 stands for "three or more")
__device__ inline int run_length(const int32_t* __restrict__ head, int64_t p, int64_t n) {
  if (p + 1 >= n || head[p + 1]) return 1;
  if (p + 2 >= n || head[p + 2]) return 2;
  return 3;
}

// he_rank[h] = rank of h's edge; per edge: the validation counts, border vertices, (val != null) the valences and
// (twin != null) the other half-edge of the run, -1 on a border edge
__global__ void edge_pass(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, const int32_t* __restrict__ head,
                          const int32_t* __restrict__ incl, int64_t n, int64_t F, int64_t V, const int32_t* __restrict__ tri,
                          int32_t* __restrict__ he_rank, uint8_t* __restrict__ border, int32_t* __restrict__ val,
                          int32_t* __restrict__ twin, unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int32_t h = vals[p];
  if (h < 0 || h >= n) return;
  he_rank[h] = incl[p] - 1;
  if (!head[p]) return;
  const int64_t f = h / 3;
  const int k = (int)(h - 3 * f);
  const int32_t a = tri[h], b = tri[3 * f + next3(k)];
  if (a < 0 || a >= V || b < 0 || b >= V) return;
  atomicAdd(&ctr[kEdges], 1ull);
  if (val) {
    atomicAdd(val + a, 1);
    atomicAdd(val + b, 1);
  }
  const int len = run_length(head, p, n);
  if (len == 1) {
    atomicAdd(&ctr[kBorderEdges], 1ull);
    border[a] = 1;                                   // every writer stores the same 1
    border[b] = 1;
    if (twin) twin[h] = -1;
  } else if (len == 2) {
    const int32_t h1 = vals[p + 1];
    if (twin && h1 >= 0 && h1 < n) {
      twin[h] = h1;
      twin[h1] = h;
    }
    if (h1 >= 0 && h1 < n && tri[h1] == a) {         // both faces run the edge from a: not opposite
      atomicAdd(&ctr[kMisoriented], 1ull);
      atomicMin(&ctr[kBadKey], (unsigned long long)keys[p]);
    }
  } else {
    atomicAdd(&ctr[kNonManifold], 1ull);
    atomicMin(&ctr[kBadKey], (unsigned long long)keys[p]);
  }
}

// ---- split ----------------------------------------------------------------------------------------------------------------
// best[f] = the rank of f's long edge of highest priority, -1 when f has no long edge
__global__ void face_best_edge(const int32_t* __restrict__ tri, const int32_t* __restrict__ he_rank, const float* __restrict__ vs,
                               int64_t F, float thr2, int32_t* __restrict__ best) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int32_t v[3] = {tri[3 * f], tri[3 * f + 1], tri[3 * f + 2]};
  int32_t b = -1;
  uint64_t bp = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float l2 = edge_len2(vs, v[k], v[next3(k)]);
    if (!(l2 > thr2)) continue;
    const int32_t r = he_rank[3 * f + k];
    const uint64_t pr = ((uint64_t)__float_as_uint(l2) << 32) | hash32((uint32_t)r);
    if (b < 0 || pr > bp) {
      b = r;
      bp = pr;
    }
  }
  best[f] = b;
}

// flag_a[p] = 1 at the head of a selected edge (entry n is 0); its faces get flag_f = 1 and fpos = p
__global__ void select_split(const int32_t* __restrict__ vals, const int32_t* __restrict__ head, const int32_t* __restrict__ incl,
                             int64_t n, int64_t F, const int32_t* __restrict__ tri, const float* __restrict__ vs, float thr2,
                             const int32_t* __restrict__ best, int32_t* __restrict__ flag_a, int32_t* __restrict__ flag_f,
                             int32_t* __restrict__ fpos, unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  int32_t sel = 0;
  if (p < n && head[p]) {
    const int32_t h = vals[p];
    const int64_t f = h / 3;
    const int k = (int)(h - 3 * f);
    if (edge_len2(vs, tri[h], tri[3 * f + next3(k)]) > thr2) {
      atomicAdd(&ctr[kLong], 1ull);
      const int32_t r = incl[p] - 1;
      const int len = run_length(head, p, n);        // 1 or 2: the mesh was validated
      const int64_t f1 = len == 2 ? vals[p + 1] / 3 : f;
      if (best[f] == r && best[f1] == r && f1 < F) {
        sel = 1;
        flag_f[f] = 1;
        fpos[f] = (int32_t)p;
        flag_f[f1] = 1;
        fpos[f1] = (int32_t)p;
      }
    }
  }
  flag_a[p] = sel;
}

__global__ void store_totals(const int32_t* __restrict__ scan_a, int64_t n, const int32_t* __restrict__ scan_f, int64_t F,
                             unsigned long long* __restrict__ ctr) {
  ctr[kTotalA] = (unsigned long long)scan_a[n];
  ctr[kTotalF] = (unsigned long long)scan_f[F];
}

// vertex V + s of the s-th selected edge: the midpoint, its two ends, and whether it lies on the border
__global__ void emit_split_vertices(const int32_t* __restrict__ vals, const int32_t* __restrict__ head,
                                    const int32_t* __restrict__ flag_a, const int32_t* __restrict__ scan_a, int64_t n, int64_t V,
                                    int64_t S, const int32_t* __restrict__ tri, float* __restrict__ vs, int32_t* __restrict__ par,
                                    uint8_t* __restrict__ border) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !flag_a[p]) return;
  const int64_t s = scan_a[p];
  if (s < 0 || s >= S) return;
  const int32_t h = vals[p];
  const int64_t f = h / 3;
  const int k = (int)(h - 3 * f);
  const int32_t a = tri[h], b = tri[3 * f + next3(k)];
  const int64_t lo = a < b ? a : b, hi = a < b ? b : a, m = V + s;
#pragma unroll
  for (int i = 0; i < 3; ++i) vs[3 * m + i] = (vs[3 * lo + i] + vs[3 * hi + i]) * kHalf;
  par[2 * m] = (int32_t)lo;
  par[2 * m + 1] = (int32_t)hi;
  border[m] = run_length(head, p, n) == 1 ? 1 : 0;
}

// (a, b, c) with the selected edge from a to b: (a, m, c) stays in slot f, (m, b, c) goes to slot F + t
__global__ void emit_split_faces(const int32_t* __restrict__ flag_f, const int32_t* __restrict__ scan_f,
                                 const int32_t* __restrict__ fpos, const int32_t* __restrict__ scan_a,
                                 const int32_t* __restrict__ he_rank, const int32_t* __restrict__ best, int64_t F, int64_t V,
                                 int64_t S, int64_t T, int64_t n, int32_t* __restrict__ tri) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F || !flag_f[f]) return;
  const int64_t t = scan_f[f], p = fpos[f];
  if (t < 0 || t >= T || p < 0 || p >= n) return;
  const int64_t s = scan_a[p];
  if (s < 0 || s >= S) return;
  const int32_t r = best[f];
  const int k = he_rank[3 * f] == r ? 0 : (he_rank[3 * f + 1] == r ? 1 : 2);
  const int32_t a = tri[3 * f + k], b = tri[3 * f + next3(k)], c = tri[3 * f + next3(next3(k))], m = (int32_t)(V + s);
  tri[3 * f] = a;
  tri[3 * f + 1] = m;
  tri[3 * f + 2] = c;
  const int64_t g = F + t;
  tri[3 * g] = m;
  tri[3 * g + 1] = b;
  tri[3 * g + 2] = c;
}

// ---- flip -----------------------------------------------------------------------------------------------------------------
__device__ inline int target_valence(const uint8_t* __restrict__ border, int32_t v) { return border[v] ? 4 : 6; }

__device__ inline int iabs(int x) { return x < 0 ? -x : x; }

// sum over the vertices with an edge of |valence - target|
__global__ void valence_deviation(const int32_t* __restrict__ val, const uint8_t* __restrict__ border, int64_t V,
                                  unsigned long long* __restrict__ ctr) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int d = 0;
  if (v < V && val[v] > 0) d = iabs(val[v] - target_valence(border, (int32_t)v));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off, 64);
  if ((threadIdx.x & 63) == 0 && d > 0) atomicAdd(&ctr[kDeviation], (unsigned long long)d);
}

struct D3 {
  double x, y, z;
};
__device__ inline D3 sub3(const float* __restrict__ vs, int32_t p, int32_t q) {      // vs[p] - vs[q] in float64
  return {(double)vs[3 * (int64_t)p] - (double)vs[3 * (int64_t)q], (double)vs[3 * (int64_t)p + 1] - (double)vs[3 * (int64_t)q + 1],
          (double)vs[3 * (int64_t)p + 2] - (double)vs[3 * (int64_t)q + 2]};
}
__device__ inline D3 cross3(const D3& u, const D3& v) {
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ inline double dot3(const D3& u, const D3& v) { return u.x * v.x + u.y * v.y + u.z * v.z; }

// the four vertices of the interior edge whose run starts at p: (a, b, c) is the face of the lower half-edge, (b, a, d) the other
__device__ inline void flip_quad(const int32_t* __restrict__ vals, const int32_t* __restrict__ tri, int64_t p, int32_t q[4]) {
  const int32_t h0 = vals[p], h1 = vals[p + 1];
  const int64_t f0 = h0 / 3, f1 = h1 / 3;
  const int k0 = (int)(h0 - 3 * f0), k1 = (int)(h1 - 3 * f1);
  q[0] = tri[h0];
  q[1] = tri[3 * f0 + next3(k0)];
  q[2] = tri[3 * f0 + next3(next3(k0))];
  q[3] = tri[3 * f1 + next3(next3(k1))];
}

// ---- creases --------------------------------------------------------------------------------------------------------------
// crease[p] = 1 at the head of an edge with two faces whose normals n1 = n(a, b, c), n2 = n(b, a, d) turn by more than the
// feature angle: dd = n1 . n2, q = (n1 . n1) (n2 . n2), c2 = cos_t^2; dd < 0 || dd dd < c2 q for cos_t >= 0, dd < 0 && dd dd > c2 q
// otherwise.  Per end: nc counts the crease edges, clo / chi keep the smallest / largest crease neighbour (integer atomics).
__global__ void crease_pass(const int32_t* __restrict__ vals, const int32_t* __restrict__ head, int64_t n,
                            const int32_t* __restrict__ tri, const float* __restrict__ vs, double cos_t,
                            uint8_t* __restrict__ crease, int32_t* __restrict__ nc, int32_t* __restrict__ clo,
                            int32_t* __restrict__ chi) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  bool flag = false;
  if (head[p] && run_length(head, p, n) == 2) {
    int32_t q4[4];
    flip_quad(vals, tri, p, q4);
    const int32_t a = q4[0], b = q4[1], c = q4[2], d = q4[3];
    const D3 n1 = cross3(sub3(vs, b, a), sub3(vs, c, a)), n2 = cross3(sub3(vs, a, b), sub3(vs, d, b));
    const double dd = dot3(n1, n2), q = dot3(n1, n1) * dot3(n2, n2), c2 = cos_t * cos_t;
    flag = cos_t >= 0.0 ? (dd < 0.0 || dd * dd < c2 * q) : (dd < 0.0 && dd * dd > c2 * q);
    if (flag) {
      atomicAdd(nc + a, 1);
      atomicAdd(nc + b, 1);
      atomicMin(clo + a, b);
      atomicMax(chi + a, b);
      atomicMin(clo + b, a);
      atomicMax(chi + b, a);
    }
  }
  crease[p] = flag ? 1 : 0;
}

// flag_a[p] = crease[p] (entry n is 0): what the scan of sg_remesh_features numbers
__global__ void crease_flags(const uint8_t* __restrict__ crease, int64_t n, int32_t* __restrict__ flag_a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n) flag_a[p] = p < n ? (int32_t)crease[p] : 0;
}

__global__ void store_crease_total(const int32_t* __restrict__ scan_a, int64_t n, unsigned long long* __restrict__ ctr) {
  ctr[kTotalA] = (unsigned long long)scan_a[n];
}

// vclass: 0 smooth, 1 crease-line, 2 corner, 3 border; nbr = (lo, hi) of a crease-line vertex, (-1, -1) otherwise.  nc == null:
// the feature setting is off and every vertex is smooth or border.
__global__ void vertex_classes(const uint8_t* __restrict__ border, const int32_t* __restrict__ nc, const int32_t* __restrict__ clo,
                               const int32_t* __restrict__ chi, int64_t V, uint8_t* __restrict__ vclass, int64_t* __restrict__ nbr) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int c = nc ? nc[v] : 0;
  const uint8_t cls = border[v] ? 3 : (c == 0 ? 0 : (c == 2 ? 1 : 2));
  vclass[v] = cls;
  nbr[2 * v] = cls == 1 ? (int64_t)clo[v] : -1;
  nbr[2 * v + 1] = cls == 1 ? (int64_t)chi[v] : -1;
}

// the s-th crease edge in ascending (lo, hi): the key of its run
__global__ void emit_crease_edges(const uint8_t* __restrict__ crease, const int32_t* __restrict__ scan_a,
                                  const uint64_t* __restrict__ keys, int64_t n, int64_t V, int64_t C, int64_t* __restrict__ edges) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !crease[p]) return;
  const int64_t s = scan_a[p];
  if (s < 0 || s >= C) return;
  edges[2 * s] = (int64_t)(keys[p] / (uint64_t)V);
  edges[2 * s + 1] = (int64_t)(keys[p] % (uint64_t)V);
}

// One Jacobi step along the creases: a vertex with nbr = (lo, hi) becomes (in[v] + in[lo] + in[hi]) / 3 per component, float32,
// summed in that order -- mesh_smooth.hip's step for a border vertex with two border edges; every other vertex is copied.
__global__ void crease_step_kernel(const float* __restrict__ in, const int64_t* __restrict__ nbr, int64_t V, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int64_t lo = nbr[2 * v], hi = nbr[2 * v + 1];
  const bool move = lo >= 0 && lo < V && hi >= 0 && hi < V;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float x = in[3 * v + i];
    if (move) {
      x += in[3 * lo + i];
      x += in[3 * hi + i];
      x = __fdiv_rn(x, 3.f);
    }
    out[3 * v + i] = x;
  }
}

// cand[p] = gain << 32 | hash(rank) for a candidate, 0 otherwise; every candidate bids for its four vertices.  crease (null:
// the feature setting is off): a crease edge is no candidate.
__global__ void flip_candidates(const uint8_t* __restrict__ crease,const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, const int32_t* __restrict__ head,
                                const int32_t* __restrict__ incl, int64_t n, int64_t V, const int32_t* __restrict__ tri,
                                const float* __restrict__ vs, const int32_t* __restrict__ val, const uint8_t* __restrict__ border,
                                unsigned long long* __restrict__ cand, unsigned long long* __restrict__ slot) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  unsigned long long key = 0;
  if (head[p] && run_length(head, p, n) == 2 && !(crease && crease[p])) {
    int32_t q[4];
    flip_quad(vals, tri, p, q);
    const int32_t a = q[0], b = q[1], c = q[2], d = q[3];
    bool ok = c != d;
    if (ok) {                                        // {c, d} must not be an edge yet: lower bound in the sorted keys
      const uint64_t want = (uint64_t)(c < d ? c : d) * (uint64_t)V + (uint64_t)(c < d ? d : c);
      int64_t lo = 0, hi = n;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      ok = !(lo < n && keys[lo] == want);
    }
    int gain = 0;
    if (ok) {
      const int va = val[a], vb = val[b], vc = val[c], vd = val[d];
      const int ta = target_valence(border, a), tb = target_valence(border, b), tc = target_valence(border, c),
                td = target_valence(border, d);
      ok = va - 1 >= (border[a] ? 2 : 3) && vb - 1 >= (border[b] ? 2 : 3);
      gain = (iabs(va - ta) + iabs(vb - tb) + iabs(vc - tc) + iabs(vd - td)) -
             (iabs(va - 1 - ta) + iabs(vb - 1 - tb) + iabs(vc + 1 - tc) + iabs(vd + 1 - td));
      ok = ok && gain > 0;
    }
    if (ok) {                                        // the guard: both new normals on the side of both old ones
      const D3 o1 = cross3(sub3(vs, b, a), sub3(vs, c, a)), o2 = cross3(sub3(vs, a, b), sub3(vs, d, b));
      const D3 n1 = cross3(sub3(vs, d, a), sub3(vs, c, a)), n2 = cross3(sub3(vs, b, d), sub3(vs, c, d));
      ok = dot3(n1, o1) > 0.0 && dot3(n1, o2) > 0.0 && dot3(n2, o1) > 0.0 && dot3(n2, o2) > 0.0;
    }
    if (ok) {
      key = ((unsigned long long)gain << 32) | hash32((uint32_t)(incl[p] - 1));
      atomicMax(slot + a, key);
      atomicMax(slot + b, key);
      atomicMax(slot + c, key);
      atomicMax(slot + d, key);
    }
  }
  cand[p] = key;
}

__global__ void flip_check(const unsigned long long* __restrict__ cand, const int32_t* __restrict__ vals,
                           const int32_t* __restrict__ tri, const unsigned long long* __restrict__ slot, int64_t n,
                           uint8_t* __restrict__ win, unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned long long key = cand[p];
  uint8_t w = 0;
  if (key) {
    int32_t q[4];
    flip_quad(vals, tri, p, q);
    w = (slot[q[0]] == key && slot[q[1]] == key && slot[q[2]] == key && slot[q[3]] == key) ? 1 : 0;
    if (w) atomicAdd(&ctr[kWinners], 1ull);
  }
  win[p] = w;
}

// (a, d, c) into the slot of (a, b, c), (d, b, c) into the slot of (b, a, d)
__global__ void flip_apply(const uint8_t* __restrict__ win, const int32_t* __restrict__ vals, int64_t n, int32_t* __restrict__ tri) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !win[p]) return;
  int32_t q[4];
  flip_quad(vals, tri, p, q);
  const int64_t f0 = vals[p] / 3, f1 = vals[p + 1] / 3;
  tri[3 * f0] = q[0];
  tri[3 * f0 + 1] = q[3];
  tri[3 * f0 + 2] = q[2];
  tri[3 * f1] = q[3];
  tri[3 * f1 + 1] = q[1];
  tri[3 * f1 + 2] = q[2];
}

// ---- collapse -------------------------------------------------------------------------------------------------------------
// is {a, b} an edge of the round's mesh: lower bound in the sorted keys
__device__ inline bool has_edge(const uint64_t* __restrict__ keys, int64_t n, int64_t V, int32_t a, int32_t b) {
  const uint64_t want = (uint64_t)(a < b ? a : b) * (uint64_t)V + (uint64_t)(a < b ? b : a);
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && keys[lo] == want;
}

// the interior edge whose run starts at p: the kept vertex k, the removed vertex r and the half-edge from r to k; false when
// both ends are border vertices.  nc (null: the feature setting is off) are the crease counts: without a border end the end
// with a crease is kept when exactly one has one, else the corner end (nc not 2) when exactly one is a corner.
__device__ inline bool collapse_ends(const int32_t* __restrict__ vals, const int32_t* __restrict__ tri,
                                     const uint8_t* __restrict__ border, const int32_t* __restrict__ nc, int64_t p, int32_t& k,
                                     int32_t& r, int32_t& hs) {
  const int32_t h0 = vals[p], h1 = vals[p + 1];
  const int64_t f0 = h0 / 3;
  const int32_t a = tri[h0], b = tri[3 * f0 + next3((int)(h0 - 3 * f0))];
  const bool ba = border[a] != 0, bb = border[b] != 0;
  if (ba && bb) return false;
  k = ba ? a : (bb ? b : (a < b ? a : b));
  if (nc && !ba && !bb) {
    const int na = nc[a], nb = nc[b];
    if ((na > 0) != (nb > 0)) k = na > 0 ? a : b;
    else if (na > 0 && (na != 2) != (nb != 2)) k = na != 2 ? a : b;
  }
  r = k == a ? b : a;
  hs = r == a ? h0 : h1;                              // h0 runs from a to b, h1 from b to a: the mesh was validated
  return true;
}

// One step of the walk round r: h runs from r to w in the face (r, w, y); the next half-edge from r is the twin of the one
// from y to r.  -1 when there is none (never for an interior r of a valid mesh): the caller ends its walk.
__device__ inline int32_t fan_step(const int32_t* __restrict__ tri, const int32_t* __restrict__ twin, int64_t n, int32_t h,
                                   int32_t& w, int32_t& y) {
  const int64_t f = h / 3;
  const int j = (int)(h - 3 * f);
  const int jp = next3(next3(j));
  w = tri[3 * f + next3(j)];
  y = tri[3 * f + jp];
  const int32_t t = twin[3 * f + jp];
  return (t >= 0 && t < n) ? t : -1;
}

__device__ inline int valence_floor(const uint8_t* __restrict__ border, int32_t v) { return border[v] ? 2 : 3; }

// cand[p] = (0xFFFFFFFF - len2 bits) << 32 | hash(rank) for a candidate, 0 otherwise; counts the short edges; every candidate
// bids for the vertices of its footprint.  Both walks are counted loops of val[r] steps.
__global__ void collapse_candidates(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                    const int32_t* __restrict__ head, const int32_t* __restrict__ incl,
                                    const int32_t* __restrict__ twin, int64_t n, int64_t V, const int32_t* __restrict__ tri,
                                    const float* __restrict__ vs, const int32_t* __restrict__ val,
                                    const uint8_t* __restrict__ border, const uint8_t* __restrict__ crease,
                                    const int32_t* __restrict__ nc, const int32_t* __restrict__ clo,
                                    const int32_t* __restrict__ chi, float lo2, float thr2,
                                    unsigned long long* __restrict__ cand, unsigned long long* __restrict__ slot,
                                    unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  unsigned long long key = 0;
  if (head[p]) {
    const int32_t h0 = vals[p];
    const int64_t f0 = h0 / 3;
    const int k0 = (int)(h0 - 3 * f0);
    const float l2 = edge_len2(vs, tri[h0], tri[3 * f0 + next3(k0)]);
    int32_t k = 0, r = 0, hs = 0;
    if (l2 < lo2) {
      atomicAdd(&ctr[kShort], 1ull);
      bool ok = run_length(head, p, n) == 2 && collapse_ends(vals, tri, border, nc, p, k, r, hs);
      int vr = 0;
      if (ok && nc && nc[r] != 0) {                    // a corner stays; a crease-line vertex leaves along its crease, forwards
        ok = nc[r] == 2 && crease[p];
        if (ok) {
          const int32_t w2 = clo[r] == k ? chi[r] : clo[r];
          ok = dot3(sub3(vs, r, k), sub3(vs, w2, r)) > 0.0;
        }
      }
      if (ok) {
        const int32_t h1 = vals[p + 1];
        const int64_t f1 = h1 / 3;
        const int32_t c = tri[3 * f0 + next3(next3(k0))], d = tri[3 * f1 + next3(next3((int)(h1 - 3 * f1)))];
        vr = val[r];
        ok = c != d && val[c] - 1 >= valence_floor(border, c) && val[d] - 1 >= valence_floor(border, d) &&
             val[k] + vr - 4 >= valence_floor(border, k);
      }
      if (ok) {
        int links = 0;
        int32_t h = hs;
        for (int i = 0; i < vr && ok; ++i) {
          int32_t w, y;
          const int32_t t = fan_step(tri, twin, n, h, w, y);
          if (w != k) {
            if (has_edge(keys, n, V, k, w)) ++links;
            if (edge_len2(vs, k, w) > thr2) ok = false;                    // the split stage would split {k, w}
            if (y != k) {                                                  // the face (r, w, y) becomes (k, w, y)
              const D3 nr = cross3(sub3(vs, w, r), sub3(vs, y, r)), nk = cross3(sub3(vs, w, k), sub3(vs, y, k));
              if (!(dot3(nr, nk) > 0.0)) ok = false;
            }
          }
          if (t < 0 || (t == hs) != (i + 1 == vr)) ok = false;             // the fan is one closed cycle of val[r] faces
          h = t < 0 ? hs : t;
        }
        ok = ok && links == 2;
      }
      if (ok) {
        key = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(l2)) << 32) | hash32((uint32_t)(incl[p] - 1));
        atomicMax(slot + r, key);
        int32_t h = hs;
        for (int i = 0; i < vr; ++i) {
          int32_t w, y;
          const int32_t t = fan_step(tri, twin, n, h, w, y);
          atomicMax(slot + w, key);
          if (t < 0) break;
          h = t;
        }
      }
    }
  }
  cand[p] = key;
}

__global__ void collapse_check(const unsigned long long* __restrict__ cand, const int32_t* __restrict__ vals,
                               const int32_t* __restrict__ twin, const int32_t* __restrict__ tri, const int32_t* __restrict__ val,
                               const uint8_t* __restrict__ border, const int32_t* __restrict__ nc,
                               const unsigned long long* __restrict__ slot, int64_t n, uint8_t* __restrict__ win,
                               unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned long long key = cand[p];
  uint8_t w8 = 0;
  int32_t k, r, hs;
  if (key && collapse_ends(vals, tri, border, nc, p, k, r, hs)) {
    bool all = slot[r] == key;
    const int vr = val[r];
    int32_t h = hs;
    for (int i = 0; i < vr && all; ++i) {
      int32_t w, y;
      const int32_t t = fan_step(tri, twin, n, h, w, y);
      all = slot[w] == key && t >= 0;
      h = t < 0 ? hs : t;
    }
    w8 = all ? 1 : 0;
    if (w8) atomicAdd(&ctr[kWinners], 1ull);
  }
  win[p] = w8;
}

__global__ void fill_ones(int32_t* __restrict__ flag, int64_t n) {       // flag[0 .. n) = 1, flag[n] = 0
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) flag[i] = i < n ? 1 : 0;
}

// per winner: its two faces and r are dropped, dest[r] = k, and k goes into r's slot of the other faces at r
__global__ void collapse_apply(const uint8_t* __restrict__ win, const int32_t* __restrict__ vals, const int32_t* __restrict__ twin,
                               const int32_t* __restrict__ val, const uint8_t* __restrict__ border,
                               const int32_t* __restrict__ nc, int64_t n, int64_t F, int32_t* __restrict__ tri,
                               int32_t* __restrict__ flag_f, int32_t* __restrict__ flag_v, int32_t* __restrict__ dest) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !win[p]) return;
  int32_t k, r, hs;
  if (!collapse_ends(vals, tri, border, nc, p, k, r, hs)) return;
  flag_v[r] = 0;
  dest[r] = k;
  const int vr = val[r];
  int32_t h = hs;
  for (int i = 0; i < vr; ++i) {
    int32_t w, y;
    const int32_t t = fan_step(tri, twin, n, h, w, y);
    if (w == k || y == k) flag_f[h / 3] = 0;
    else tri[h] = k;                                   // h starts at r
    if (t < 0) break;
    h = t;
  }
}

__device__ inline int32_t new_vertex(const int32_t* __restrict__ flag_v, const int32_t* __restrict__ scan_v,
                                     const int32_t* __restrict__ dest, int32_t v) {
  return flag_v[v] ? scan_v[v] : scan_v[dest[v]];      // the kept end of a winner survives its round
}

__global__ void compact_vertices(const int32_t* __restrict__ flag_v, const int32_t* __restrict__ scan_v,
                                 const int32_t* __restrict__ dest, int64_t V, int64_t V2, const float* __restrict__ vs,
                                 const int32_t* __restrict__ par, const uint8_t* __restrict__ border, const int32_t* __restrict__ ids,
                                 float* __restrict__ vs2, int32_t* __restrict__ par2, uint8_t* __restrict__ border2,
                                 int32_t* __restrict__ ids2) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V || !flag_v[v]) return;
  const int64_t m = scan_v[v];
  if (m < 0 || m >= V2) return;
#pragma unroll
  for (int i = 0; i < 3; ++i) vs2[3 * m + i] = vs[3 * v + i];
  par2[2 * m] = new_vertex(flag_v, scan_v, dest, par[2 * v]);
  par2[2 * m + 1] = new_vertex(flag_v, scan_v, dest, par[2 * v + 1]);
  border2[m] = border[v];
  ids2[m] = ids[v];
}

__global__ void compact_faces(const int32_t* __restrict__ flag_f, const int32_t* __restrict__ scan_f,
                              const int32_t* __restrict__ scan_v, int64_t F, int64_t F2, const int32_t* __restrict__ tri,
                              int32_t* __restrict__ tri2) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F || !flag_f[f]) return;
  const int64_t g = scan_f[f];
  if (g < 0 || g >= F2) return;
#pragma unroll
  for (int i = 0; i < 3; ++i) tri2[3 * g + i] = scan_v[tri[3 * f + i]];   // every vertex of a kept face is kept
}

__global__ void compose_into(const int32_t* __restrict__ flag_v, const int32_t* __restrict__ scan_v,
                             const int32_t* __restrict__ dest, int64_t n_before, int32_t* __restrict__ into) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_before) into[i] = new_vertex(flag_v, scan_v, dest, into[i]);
}

template <class T>
__global__ void iota(T* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (T)i;
}

// ---- simplify -------------------------------------------------------------------------------------------------------------
// The specification is semigcn_amd/simplify.py.  The counters of a simplify round live in slots the collapse analysis leaves
// alone: legal candidates, refused edges, the admitted count and the cut.
enum { kCand = kLong, kRefused = kShort, kAdmitted = kTotalA, kCut = kTotalF };

__global__ void corner_keys(const int32_t* __restrict__ tri, int64_t n, uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n) return;
  keys[h] = (uint64_t)(uint32_t)tri[h];
  vals[h] = (int32_t)h;
}

// quad[v] = the sum of K = p p^T / (n . n) over the faces at v in ascending face index (the corners were sorted by vertex, stably):
// ten entries (xx, xy, xz, xw, yy, yz, yw, zz, zw, ww), ten float64 divisions per face, no root
__global__ void vertex_quadrics(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int64_t V,
                                const int32_t* __restrict__ tri, const float* __restrict__ vs, double* __restrict__ quad) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < (uint64_t)v) lo = mid + 1;
    else hi = mid;
  }
  double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t p = lo; p < n && keys[p] == (uint64_t)v; ++p) {
    const int32_t h = vals[p];
    if (h < 0 || h >= n) break;
    const int64_t f = h / 3;
    const int32_t a = tri[3 * f], b = tri[3 * f + 1], c = tri[3 * f + 2];
    const D3 nrm = cross3(sub3(vs, b, a), sub3(vs, c, a));
    const double nn = dot3(nrm, nrm);
    if (nn == 0.0) continue;
    const double ax = (double)vs[3 * (int64_t)a], ay = (double)vs[3 * (int64_t)a + 1], az = (double)vs[3 * (int64_t)a + 2];
    const double pl[4] = {nrm.x, nrm.y, nrm.z, -(nrm.x * ax + nrm.y * ay + nrm.z * az)};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j, ++e) q[e] = q[e] + (pl[i] * pl[j]) / nn;
  }
#pragma unroll
  for (int e = 0; e < 10; ++e) quad[10 * v + e] = q[e];
}

// The faces at v, from the half-edge hs that starts at v: face(x, y) for every face, rotated to read (v, x, y), and vert(u) for
// every vertex of ring(v), each once -- forwards through twin and next half-edges until the fan closes or ends at a border,
// then backwards from hs.  At most `limit` faces are visited.  Returns the number of ring vertices seen: val[v] exactly when
// the faces at v are one fan (closed round an interior vertex, open at a border vertex); -1 when the walk ran out.
template <class Face, class Vert>
__device__ inline int walk_ring(const int32_t* __restrict__ tri, const int32_t* __restrict__ twin, int64_t n, int32_t hs, int limit,
                                Face&& face, Vert&& vert) {
  int seen = 0, faces = 0;
  bool closed = false, ended = false;
  int32_t h = hs;
  while (faces < limit) {
    int32_t w, y;
    const int32_t t = fan_step(tri, twin, n, h, w, y);
    face(w, y);
    vert(w);
    ++faces;
    ++seen;
    if (t < 0) {
      vert(y);
      ++seen;
      ended = true;
      break;
    }
    if (t == hs) {
      closed = true;
      break;
    }
    h = t;
  }
  if (closed) return seen;
  if (!ended) return -1;
  h = hs;
  while (faces < limit) {
    const int32_t t = twin[h];
    if (t < 0 || t >= n) break;
    const int64_t f = t / 3;
    const int j = (int)(t - 3 * f);
    h = (int32_t)(3 * f + next3(j));                    // t runs from w to v in the face (w, v, z): h runs from v to z
    const int32_t z = tri[3 * f + next3(next3(j))];
    face(z, tri[t]);
    vert(z);
    ++faces;
    ++seen;
  }
  return seen;
}

__device__ inline D3 sub3p(const float* __restrict__ vs, int32_t p, const float q[3]) {          // vs[p] - q in float64
  return {(double)vs[3 * (int64_t)p] - (double)q[0], (double)vs[3 * (int64_t)p + 1] - (double)q[1],
          (double)vs[3 * (int64_t)p + 2] - (double)q[2]};
}

// the ends of the candidate at p as collapse_ends names them, and the half-edge from k to r
__device__ inline bool simplify_ends(const int32_t* __restrict__ vals, const int32_t* __restrict__ tri,
                                     const uint8_t* __restrict__ border, int64_t p, int32_t& k, int32_t& r, int32_t& hs,
                                     int32_t& hk) {
  if (!collapse_ends(vals, tri, border, nullptr, p, k, r, hs)) return false;
  hk = hs == vals[p] ? vals[p + 1] : vals[p];
  return true;
}

// cand[p] = (0xFFFFFFFF - bits(float32(cost))) << 32 | hash(rank) for a legal candidate, 0 otherwise; counts the legal and the
// refused ones.  Nobody bids here: the cut is not known yet.
__global__ void simplify_price(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, const int32_t* __restrict__ head,
                               const int32_t* __restrict__ incl, const int32_t* __restrict__ twin, int64_t n, int64_t V,
                               const int32_t* __restrict__ tri, const float* __restrict__ vs, const int32_t* __restrict__ val,
                               const uint8_t* __restrict__ border, const double* __restrict__ quad,
                               unsigned long long* __restrict__ cand, unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  unsigned long long key = 0;
  int32_t k = 0, r = 0, hs = 0, hk = 0;
  if (head[p] && run_length(head, p, n) == 2 && simplify_ends(vals, tri, border, p, k, r, hs, hk)) {
    const int32_t h0 = vals[p], h1 = vals[p + 1];
    const int64_t f0 = h0 / 3, f1 = h1 / 3;
    const int32_t c = tri[3 * f0 + next3(next3((int)(h0 - 3 * f0)))], d = tri[3 * f1 + next3(next3((int)(h1 - 3 * f1)))];
    const int vr = val[r], vk = val[k], vn = vk + vr - 4;
    const bool moves = border[k] == 0;
    float P[3];                                        // where k will be
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int64_t lo = k < r ? k : r, hi = k < r ? r : k;
      P[i] = moves ? (vs[3 * lo + i] + vs[3 * hi + i]) * kHalf : vs[3 * (int64_t)k + i];
    }
    bool ok = c != d && val[c] - 1 >= valence_floor(border, c) && val[d] - 1 >= valence_floor(border, d) &&
              vn >= valence_floor(border, k);
    if (ok) {                                          // the fan of r: one closed cycle, the link, the guard
      int links = 0;
      const int seen = walk_ring(
          tri, twin, n, hs, vr,
          [&](int32_t x, int32_t y) {
            if (x == k || y == k) return;
            const D3 no = cross3(sub3(vs, x, r), sub3(vs, y, r)), nw = cross3(sub3p(vs, x, P), sub3p(vs, y, P));
            if (!(dot3(no, nw) > 0.0)) ok = false;
          },
          [&](int32_t u) {
            if (u != k && has_edge(keys, n, V, k, u)) ++links;
          });
      ok = ok && seen == vr && links == 2;
    }
    if (ok) {                                          // the fan of k: one fan, and the guard when k moves
      const int seen = walk_ring(
          tri, twin, n, hk, vk,
          [&](int32_t x, int32_t y) {
            if (!moves || x == r || y == r) return;
            const D3 no = cross3(sub3(vs, x, k), sub3(vs, y, k)), nw = cross3(sub3p(vs, x, P), sub3p(vs, y, P));
            if (!(dot3(no, nw) > 0.0)) ok = false;
          },
          [](int32_t) {});
      ok = ok && seen == vk;
    }
    if (ok) {
      const double* __restrict__ qk = quad + 10 * (int64_t)k;
      const double* __restrict__ qr = quad + 10 * (int64_t)r;
      double q[10];
#pragma unroll
      for (int e = 0; e < 10; ++e) q[e] = qk[e] + qr[e];
      const double x = (double)P[0], y = (double)P[1], z = (double)P[2];
      const double s0 = q[0] * x + q[1] * y + q[2] * z + q[3];
      const double s1 = q[1] * x + q[4] * y + q[5] * z + q[6];
      const double s2 = q[2] * x + q[5] * y + q[7] * z + q[8];
      const double s3 = q[3] * x + q[6] * y + q[8] * z + q[9];
      const double err = x * s0 + y * s1 + z * s2 + s3;
      double pen = (double)(iabs(vn - 6) + 1);
      if (vn == 3) pen = pen * 100000.0;
      double cost = err * pen;
      ok = isfinite(cost);
      if (ok) {
        cost = cost > 0.0 ? cost : 0.0;
        const float c32 = cost > 3.4028234663852886e38 ? 3.4028234663852886e38f : (float)cost;
        key = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(c32)) << 32) | hash32((uint32_t)(incl[p] - 1));
      }
    }
    atomicAdd(&ctr[ok ? kCand : kRefused], 1ull);
  }
  cand[p] = key;
}

// sorted = the n keys of the round in ascending order (zeros first).  With C legal candidates the min(need, C) highest bid:
// the cut is the lowest key among them.
__global__ void simplify_cut(const unsigned long long* __restrict__ sorted, int64_t n, int64_t need,
                             unsigned long long* __restrict__ ctr) {
  const int64_t C = (int64_t)ctr[kCand];
  int64_t m = need < C ? need : C;
  if (m < 0 || m > n) m = 0;
  ctr[kAdmitted] = (unsigned long long)m;
  ctr[kCut] = m > 0 ? sorted[n - m] : ~0ull;
}

template <class Fn>
__device__ inline void simplify_footprint(const int32_t* __restrict__ vals, const int32_t* __restrict__ twin,
                                          const int32_t* __restrict__ tri, const int32_t* __restrict__ val,
                                          const uint8_t* __restrict__ border, int64_t n, int64_t p, Fn&& fn) {
  int32_t k, r, hs, hk;
  if (!simplify_ends(vals, tri, border, p, k, r, hs, hk)) return;
  fn(k);
  fn(r);
  walk_ring(tri, twin, n, hs, val[r], [](int32_t, int32_t) {}, fn);
  walk_ring(tri, twin, n, hk, val[k], [](int32_t, int32_t) {}, fn);
}

// every admitted candidate bids for the vertices of its footprint {k, r} + ring(k) + ring(r)
__global__ void simplify_bid(const unsigned long long* __restrict__ cand, const int32_t* __restrict__ vals,
                             const int32_t* __restrict__ twin, const int32_t* __restrict__ tri, const int32_t* __restrict__ val,
                             const uint8_t* __restrict__ border, const unsigned long long* __restrict__ ctr, int64_t n,
                             unsigned long long* __restrict__ slot) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned long long key = cand[p];
  if (!key || ctr[kAdmitted] == 0 || key < ctr[kCut]) return;
  simplify_footprint(vals, twin, tri, val, border, n, p, [&](int32_t u) { atomicMax(slot + u, key); });
}

__global__ void simplify_check(const unsigned long long* __restrict__ cand, const int32_t* __restrict__ vals,
                               const int32_t* __restrict__ twin, const int32_t* __restrict__ tri, const int32_t* __restrict__ val,
                               const uint8_t* __restrict__ border, const unsigned long long* __restrict__ slot, int64_t n,
                               uint8_t* __restrict__ win, unsigned long long* __restrict__ ctr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned long long key = cand[p];
  uint8_t w8 = 0;
  if (key && ctr[kAdmitted] != 0 && key >= ctr[kCut]) {
    bool all = true;
    simplify_footprint(vals, twin, tri, val, border, n, p, [&](int32_t u) {
      if (slot[u] != key) all = false;
    });
    w8 = all ? 1 : 0;
    if (w8) atomicAdd(&ctr[kWinners], 1ull);
  }
  win[p] = w8;
}

// per winner, before the faces are rewritten: k goes to the midpoint unless it is a border vertex; sum: Q[k] = Q[k] + Q[r]
__global__ void simplify_move(const uint8_t* __restrict__ win, const int32_t* __restrict__ vals, const int32_t* __restrict__ tri,
                              const uint8_t* __restrict__ border, int64_t n, int sum, float* __restrict__ vs,
                              double* __restrict__ quad) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !win[p]) return;
  int32_t k, r, hs;
  if (!collapse_ends(vals, tri, border, nullptr, p, k, r, hs)) return;
  if (!border[k]) {
    const int64_t lo = k < r ? k : r, hi = k < r ? r : k;
#pragma unroll
    for (int i = 0; i < 3; ++i) vs[3 * (int64_t)k + i] = (vs[3 * lo + i] + vs[3 * hi + i]) * kHalf;
  }
  if (sum) {
#pragma unroll
    for (int e = 0; e < 10; ++e) quad[10 * (int64_t)k + e] = quad[10 * (int64_t)k + e] + quad[10 * (int64_t)r + e];
  }
}

__global__ void compact_quadrics(const int32_t* __restrict__ flag_v, const int32_t* __restrict__ scan_v, int64_t V, int64_t V2,
                                 const double* __restrict__ quad, double* __restrict__ quad2) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V || !flag_v[v]) return;
  const int64_t m = scan_v[v];
  if (m < 0 || m >= V2) return;
#pragma unroll
  for (int e = 0; e < 10; ++e) quad2[10 * m + e] = quad[10 * v + e];
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// keys, sort, heads, ranks, edge pass on the mesh as it stands; resets the counters first.  No host synchronisation unless a
// scratch buffer has to grow.
int analyse(sg_remesh* s, bool with_valence, hipStream_t stream, bool with_twin = false) {
  const int64_t V = s->V, F = s->F, n = 3 * F;
  for (auto* b : {&s->keys_a, &s->keys_b})
    if (int rc = b->reserve(n, false, stream)) return rc;
  if (int rc = s->cand.reserve(n, false, stream)) return rc;
  for (auto* b : {&s->vals_a, &s->vals_b, &s->head, &s->incl, &s->he_rank})
    if (int rc = b->reserve(n, false, stream)) return rc;
  for (auto* b : {&s->flag_a, &s->scan_a})
    if (int rc = b->reserve(n + 1, false, stream)) return rc;
  for (auto* b : {&s->flag_f, &s->scan_f, &s->best, &s->fpos})
    if (int rc = b->reserve(F + 1, false, stream)) return rc;
  if (int rc = s->win.reserve(n, false, stream)) return rc;
  if (int rc = s->slot.reserve(V, false, stream)) return rc;
  if (int rc = s->val.reserve(V, false, stream)) return rc;
  if (with_twin)
    if (int rc = s->twin.reserve(n, false, stream)) return rc;
  s->feat_C = -1;
  s->quad_fresh = false;                             // whoever analyses is about to change the mesh, or has
  if (s->feat) {
    if (int rc = s->crease.reserve(n, false, stream)) return rc;
    for (auto* b : {&s->nc, &s->clo, &s->chi})
      if (int rc = b->reserve(V, false, stream)) return rc;
  }
  const int bits = bits_for((uint64_t)V * (uint64_t)V, 62);    // the keys are below V * V < 2^62
  const int32_t *head = s->head.p, *flag_a = s->flag_a.p, *flag_f = s->flag_f.p;   // hipCUB's iterator arguments keep their const
  size_t tb_sort = 0, tb_incl = 0, tb_a = 0, tb_f = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, (int)n, 0,
                                                bits, stream));
  SG_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb_incl, head, s->incl.p, (int)n, stream));
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_a, flag_a, s->scan_a.p, (int)(n + 1), stream));
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_f, flag_f, s->scan_f.p, (int)(F + 1), stream));
  size_t tb = tb_sort;
  for (size_t t : {tb_incl, tb_a, tb_f}) tb = t > tb ? t : tb;
  if (int rc = s->temp.reserve(tb ? tb : 16, false, stream)) return rc;

  reset_counters<<<1, 64, 0, stream>>>(s->ctr.p);
  SG_HIP_TRY(hipMemsetAsync(s->border.p, 0, (size_t)V, stream));
  if (with_valence) SG_HIP_TRY(hipMemsetAsync(s->val.p, 0, (size_t)V * sizeof(int32_t), stream));
  half_edge_keys<<<blocks_for(n), kThreads, 0, stream>>>(s->tri.p, n, V, s->keys_a.p, s->vals_a.p);
  SG_HIP_TRY(hipGetLastError());
  size_t tb_use = s->temp.cap;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(s->temp.p, tb_use, s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, (int)n, 0,
                                                bits, stream));
  mark_heads<<<blocks_for(n), kThreads, 0, stream>>>(s->keys_b.p, n, s->head.p);
  SG_HIP_TRY(hipGetLastError());
  tb_use = s->temp.cap;
  SG_HIP_TRY(hipcub::DeviceScan::InclusiveSum(s->temp.p, tb_use, head, s->incl.p, (int)n, stream));
  edge_pass<<<blocks_for(n), kThreads, 0, stream>>>(s->keys_b.p, s->vals_b.p, s->head.p, s->incl.p, n, F, V, s->tri.p,
                                                   s->he_rank.p, s->border.p, with_valence ? s->val.p : nullptr,
                                                   with_twin ? s->twin.p : nullptr, s->ctr.p);
  SG_HIP_TRY(hipGetLastError());
  if (s->feat) {                                     // the creases of the positions the round starts with
    SG_HIP_TRY(hipMemsetAsync(s->nc.p, 0, (size_t)V * sizeof(int32_t), stream));
    SG_HIP_TRY(hipMemsetAsync(s->clo.p, 0x7f, (size_t)V * sizeof(int32_t), stream));   // above every vertex id
    SG_HIP_TRY(hipMemsetAsync(s->chi.p, 0xff, (size_t)V * sizeof(int32_t), stream));   // -1
    crease_pass<<<blocks_for(n), kThreads, 0, stream>>>(s->vals_b.p, s->head.p, n, s->tri.p, s->vs.p, s->cos_t, s->crease.p,
                                                       s->nc.p, s->clo.p, s->chi.p);
    SG_HIP_TRY(hipGetLastError());
  }
  return SG_OK;
}

int read_counters(sg_remesh* s, unsigned long long* h, hipStream_t stream) {
  SG_HIP_TRY(hipMemcpyAsync(h, s->ctr.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  return SG_OK;
}

}  // namespace

void destroy_remesh(sg_remesh* s) { delete s; }

int remesh_create(const float* vs, int64_t V, const int64_t* faces, int64_t F, hipStream_t stream, sg_remesh** out) {
  SG_REQUIRE(V < ((int64_t)1 << 31) && 3 * F < ((int64_t)1 << 31), "sg_remesh_create: sizes must fit int32");
  std::unique_ptr<sg_remesh> s(new (std::nothrow) sg_remesh);
  SG_REQUIRE(s != nullptr, "sg_remesh_create: out of host memory");
  s->V = s->V0 = V;
  s->F = s->F0 = F;
  s->h_ctr[kBadFace] = s->h_ctr[kBadVertex] = s->h_ctr[kBadKey] = ~0ull;
  s->bad_key_V = V;
  if (V == 0) {
    SG_REQUIRE(F == 0, "sg_remesh_create: face refers to a vertex outside [0, 0)");
    s->valid = true;
    *out = s.release();
    return SG_OK;
  }
  if (int rc = s->ctr.reserve(kCounters, false, stream)) return rc;
  if (int rc = s->vs.reserve(3 * V, false, stream)) return rc;
  if (int rc = s->par.reserve(2 * V, false, stream)) return rc;
  if (int rc = s->border.reserve(V, false, stream)) return rc;
  if (int rc = s->tri.reserve(3 * F, false, stream)) return rc;
  SG_HIP_TRY(hipMemcpyAsync(s->vs.p, vs, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
  SG_HIP_TRY(hipMemsetAsync(s->border.p, 0, (size_t)V, stream));
  reset_counters<<<1, 64, 0, stream>>>(s->ctr.p);
  if (F > 0) classify_faces<<<blocks_for(F), kThreads, 0, stream>>>(faces, F, V, s->tri.p, s->ctr.p);
  check_vertices<<<blocks_for(V), kThreads, 0, stream>>>(s->vs.p, V, s->par.p, s->ctr.p);
  SG_HIP_TRY(hipGetLastError());
  unsigned long long first[kCounters];
  if (int rc = read_counters(s.get(), first, stream)) return rc;
  SG_REQUIRE(!first[kOutOfRange], "sg_remesh_create: face refers to a vertex outside [0, %lld)", (long long)V);
  if (F > 0) {
    if (int rc = analyse(s.get(), false, stream)) return rc;   // resets the counters: the face and vertex counts are kept in `first`
    if (int rc = read_counters(s.get(), s->h_ctr, stream)) return rc;
  }
  for (int i : {(int)kDegenerate, (int)kBadFace, (int)kNonFinite, (int)kBadVertex}) s->h_ctr[i] = first[i];
  s->valid = !s->h_ctr[kDegenerate] && !s->h_ctr[kNonFinite] && !s->h_ctr[kNonManifold] && !s->h_ctr[kMisoriented];
  *out = s.release();
  return SG_OK;
}

void remesh_query(const sg_remesh* s, int64_t* info) {
  const unsigned long long* c = s->h_ctr;
  const bool bad_edge = c[kBadKey] != ~0ull && s->bad_key_V > 0;
  info[0] = s->V;
  info[1] = s->F;
  info[2] = (int64_t)c[kEdges];
  info[3] = (int64_t)c[kBorderEdges];
  info[4] = (int64_t)c[kNonManifold];
  info[5] = (int64_t)c[kMisoriented];
  info[6] = (int64_t)c[kDegenerate];
  info[7] = (int64_t)c[kNonFinite];
  info[8] = bad_edge ? (int64_t)(c[kBadKey] / (unsigned long long)s->bad_key_V) : -1;
  info[9] = bad_edge ? (int64_t)(c[kBadKey] % (unsigned long long)s->bad_key_V) : -1;
  info[10] = c[kBadFace] != ~0ull ? (int64_t)c[kBadFace] : -1;
  info[11] = c[kBadVertex] != ~0ull ? (int64_t)c[kBadVertex] : -1;
  info[12] = s->V0;
  info[13] = s->F0;
  info[14] = s->valid ? 1 : 0;
  info[15] = 0;
}

int remesh_split(sg_remesh* s, float thr2, int64_t max_rounds, hipStream_t stream, int64_t* counts, int64_t* n_rounds,
                 int64_t* n_long) {
  *n_rounds = 0;
  *n_long = 0;
  SG_REQUIRE(s->valid, "sg_remesh_split: the mesh did not pass validation (sg_remesh_query)");
  if (s->F == 0) return SG_OK;
  for (int64_t round = 0;; ++round) {
    const int64_t V = s->V, F = s->F, n = 3 * F;
    if (int rc = analyse(s, false, stream)) return rc;
    face_best_edge<<<blocks_for(F), kThreads, 0, stream>>>(s->tri.p, s->he_rank.p, s->vs.p, F, thr2, s->best.p);
    SG_HIP_TRY(hipMemsetAsync(s->flag_f.p, 0, (size_t)(F + 1) * sizeof(int32_t), stream));
    select_split<<<blocks_for(n + 1), kThreads, 0, stream>>>(s->vals_b.p, s->head.p, s->incl.p, n, F, s->tri.p, s->vs.p, thr2,
                                                            s->best.p, s->flag_a.p, s->flag_f.p, s->fpos.p, s->ctr.p);
    SG_HIP_TRY(hipGetLastError());
    const int32_t *flag_a = s->flag_a.p, *flag_f = s->flag_f.p;   // hipCUB's iterator arguments keep their const
    size_t tb = s->temp.cap;
    SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s->temp.p, tb, flag_a, s->scan_a.p, (int)(n + 1), stream));
    tb = s->temp.cap;
    SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s->temp.p, tb, flag_f, s->scan_f.p, (int)(F + 1), stream));
    store_totals<<<1, 1, 0, stream>>>(s->scan_a.p, n, s->scan_f.p, F, s->ctr.p);
    SG_HIP_TRY(hipGetLastError());
    unsigned long long c[kCounters];
    if (int rc = read_counters(s, c, stream)) return rc;       // the round's one synchronisation: count -> emit
    const int64_t S = (int64_t)c[kTotalA], T = (int64_t)c[kTotalF];
    *n_long = (int64_t)c[kLong];
    SG_REQUIRE(S >= 0 && S <= n && T >= S && T <= 2 * S && T <= F, "sg_remesh_split: totals out of range (%lld edges, %lld faces)",
               (long long)S, (long long)T);
    if (S == 0 || round >= max_rounds) break;
    SG_REQUIRE(V + S < ((int64_t)1 << 31) && 3 * (F + T) < ((int64_t)1 << 31), "sg_remesh_split: sizes must fit int32");
    if (int rc = s->vs.reserve(3 * (V + S), true, stream)) return rc;
    if (int rc = s->par.reserve(2 * (V + S), true, stream)) return rc;
    if (int rc = s->border.reserve(V + S, true, stream)) return rc;
    if (int rc = s->tri.reserve(3 * (F + T), true, stream)) return rc;
    emit_split_vertices<<<blocks_for(n), kThreads, 0, stream>>>(s->vals_b.p, s->head.p, s->flag_a.p, s->scan_a.p, n, V, S,
                                                               s->tri.p, s->vs.p, s->par.p, s->border.p);
    emit_split_faces<<<blocks_for(F), kThreads, 0, stream>>>(s->flag_f.p, s->scan_f.p, s->fpos.p, s->scan_a.p, s->he_rank.p,
                                                            s->best.p, F, V, S, T, n, s->tri.p);
    SG_HIP_TRY(hipGetLastError());
    s->V = V + S;
    s->F = F + T;
    counts[round] = S;
    *n_rounds = round + 1;
  }
  return SG_OK;
}

int remesh_flip(sg_remesh* s, int64_t max_rounds, hipStream_t stream, int64_t* counts, int64_t* n_rounds, int64_t* deviation) {
  *n_rounds = 0;
  deviation[0] = deviation[1] = 0;
  SG_REQUIRE(s->valid, "sg_remesh_flip: the mesh did not pass validation (sg_remesh_query)");
  if (s->F == 0) return SG_OK;
  const int64_t V = s->V, F = s->F, n = 3 * F;
  for (int64_t round = 0;; ++round) {
    if (int rc = analyse(s, true, stream)) return rc;
    SG_HIP_TRY(hipMemsetAsync(s->slot.p, 0, (size_t)V * sizeof(uint64_t), stream));
    valence_deviation<<<blocks_for(V), kThreads, 0, stream>>>(s->val.p, s->border.p, V, s->ctr.p);
    flip_candidates<<<blocks_for(n), kThreads, 0, stream>>>(s->feat ? s->crease.p : nullptr, s->keys_b.p,s->vals_b.p, s->head.p, s->incl.p, n, V, s->tri.p,
                                                           s->vs.p, s->val.p, s->border.p, s->cand.p, s->slot.p);
    flip_check<<<blocks_for(n), kThreads, 0, stream>>>(s->cand.p, s->vals_b.p, s->tri.p, s->slot.p, n, s->win.p, s->ctr.p);
    SG_HIP_TRY(hipGetLastError());
    unsigned long long c[kCounters];
    if (int rc = read_counters(s, c, stream)) return rc;       // the round's one synchronisation: count -> apply
    const int64_t W = (int64_t)c[kWinners];
    if (round == 0) deviation[0] = (int64_t)c[kDeviation];
    deviation[1] = (int64_t)c[kDeviation];
    SG_REQUIRE(W >= 0 && W <= n, "sg_remesh_flip: winner count %lld out of range", (long long)W);
    if (W == 0 || round >= max_rounds) break;
    flip_apply<<<blocks_for(n), kThreads, 0, stream>>>(s->win.p, s->vals_b.p, n, s->tri.p);
    SG_HIP_TRY(hipGetLastError());
    counts[round] = W;
    *n_rounds = round + 1;
  }
  return SG_OK;
}

namespace {
template <class T>
void swap_bufs(GrowBuf<T>& a, GrowBuf<T>& b) {
  std::swap(a.p, b.p);
  std::swap(a.cap, b.cap);
}

}  // namespace

namespace {
// The second half of a collapse round, shared by sg_remesh_collapse and sg_remesh_simplify: the W winners in win[] are applied
// to the mesh of the round's analysis, vertices and faces are compacted (stable) and the maps of the call are composed.
// quad_mode < 0: no quadrics; 0 / 1 (simplify, "own" / "sum"): the kept vertex of a winner moves first, and the quadrics are
// compacted with the vertices.
int apply_and_compact(sg_remesh* s, int64_t W, int64_t V_before, const int32_t* nc, int quad_mode, hipStream_t stream) {
  const int64_t V = s->V, F = s->F, n = 3 * F;
  const int64_t V2 = V - W, F2 = F - 2 * W;
  for (auto* b : {&s->flag_v, &s->scan_v})
    if (int rc = b->reserve(V + 1, false, stream)) return rc;
  if (int rc = s->dest.reserve(V, false, stream)) return rc;
  if (int rc = s->vs2.reserve(3 * V2, false, stream)) return rc;
  if (int rc = s->par2.reserve(2 * V2, false, stream)) return rc;
  if (int rc = s->border2.reserve(V2, false, stream)) return rc;
  if (int rc = s->ids2.reserve(V2, false, stream)) return rc;
  if (int rc = s->tri2.reserve(3 * F2, false, stream)) return rc;
  const int32_t *flag_v = s->flag_v.p, *flag_f = s->flag_f.p;   // hipCUB's iterator arguments keep their const
  size_t tb_v = 0;
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_v, flag_v, s->scan_v.p, (int)(V + 1), stream));
  if (int rc = s->temp.reserve(tb_v ? tb_v : 16, false, stream)) return rc;
  fill_ones<<<blocks_for(V + 1), kThreads, 0, stream>>>(s->flag_v.p, V);
  fill_ones<<<blocks_for(F + 1), kThreads, 0, stream>>>(s->flag_f.p, F);
  if (quad_mode >= 0) {
    if (int rc = s->quad2.reserve(10 * V2, false, stream)) return rc;
    simplify_move<<<blocks_for(n), kThreads, 0, stream>>>(s->win.p, s->vals_b.p, s->tri.p, s->border.p, n, quad_mode, s->vs.p,
                                                         s->quad.p);
  }
  collapse_apply<<<blocks_for(n), kThreads, 0, stream>>>(s->win.p, s->vals_b.p, s->twin.p, s->val.p, s->border.p, nc, n, F,
                                                        s->tri.p, s->flag_f.p, s->flag_v.p, s->dest.p);
  SG_HIP_TRY(hipGetLastError());
  size_t tb = s->temp.cap;
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s->temp.p, tb, flag_v, s->scan_v.p, (int)(V + 1), stream));
  tb = s->temp.cap;
  SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s->temp.p, tb, flag_f, s->scan_f.p, (int)(F + 1), stream));
  compact_vertices<<<blocks_for(V), kThreads, 0, stream>>>(s->flag_v.p, s->scan_v.p, s->dest.p, V, V2, s->vs.p, s->par.p,
                                                          s->border.p, s->ids.p, s->vs2.p, s->par2.p, s->border2.p, s->ids2.p);
  if (F2 > 0)
    compact_faces<<<blocks_for(F), kThreads, 0, stream>>>(s->flag_f.p, s->scan_f.p, s->scan_v.p, F, F2, s->tri.p, s->tri2.p);
  if (quad_mode >= 0)
    compact_quadrics<<<blocks_for(V), kThreads, 0, stream>>>(s->flag_v.p, s->scan_v.p, V, V2, s->quad.p, s->quad2.p);
  compose_into<<<blocks_for(V_before), kThreads, 0, stream>>>(s->flag_v.p, s->scan_v.p, s->dest.p, V_before, s->into.p);
  SG_HIP_TRY(hipGetLastError());
  swap_bufs(s->vs, s->vs2);
  swap_bufs(s->par, s->par2);
  swap_bufs(s->border, s->border2);
  swap_bufs(s->ids, s->ids2);
  swap_bufs(s->tri, s->tri2);
  if (quad_mode >= 0) swap_bufs(s->quad, s->quad2);
  s->V = s->map_after = V2;
  s->F = F2;
  return SG_OK;
}

}  // namespace

int remesh_collapse(sg_remesh* s, float lo2, float thr2, int64_t max_rounds, hipStream_t stream, int64_t* counts,
                    int64_t* n_rounds, int64_t* n_short) {
  *n_rounds = 0;
  *n_short = 0;
  SG_REQUIRE(s->valid, "sg_remesh_collapse: the mesh did not pass validation (sg_remesh_query)");
  s->map_before = s->map_after = s->V;
  if (s->V == 0) return SG_OK;
  const int64_t V_before = s->V;
  if (int rc = s->ids.reserve(V_before, false, stream)) return rc;
  if (int rc = s->into.reserve(V_before, false, stream)) return rc;
  iota<<<blocks_for(V_before), kThreads, 0, stream>>>(s->ids.p, V_before);
  iota<<<blocks_for(V_before), kThreads, 0, stream>>>(s->into.p, V_before);
  SG_HIP_TRY(hipGetLastError());
  if (s->F == 0) return SG_OK;
  for (int64_t round = 0;; ++round) {
    const int64_t V = s->V, F = s->F, n = 3 * F;
    if (F == 0) {                                     // every face went: nothing left to analyse
      *n_short = 0;
      break;
    }
    if (int rc = analyse(s, true, stream, true)) return rc;
    const int32_t* nc = s->feat ? s->nc.p : nullptr;  // the analysis may have grown the buffer
    SG_HIP_TRY(hipMemsetAsync(s->slot.p, 0, (size_t)V * sizeof(uint64_t), stream));
    collapse_candidates<<<blocks_for(n), kThreads, 0, stream>>>(s->keys_b.p, s->vals_b.p, s->head.p, s->incl.p, s->twin.p, n, V,
                                                               s->tri.p, s->vs.p, s->val.p, s->border.p, s->crease.p, nc, s->clo.p,
                                                               s->chi.p, lo2, thr2, s->cand.p, s->slot.p, s->ctr.p);
    collapse_check<<<blocks_for(n), kThreads, 0, stream>>>(s->cand.p, s->vals_b.p, s->twin.p, s->tri.p, s->val.p, s->border.p,
                                                          nc, s->slot.p, n, s->win.p, s->ctr.p);
    SG_HIP_TRY(hipGetLastError());
    unsigned long long c[kCounters];
    if (int rc = read_counters(s, c, stream)) return rc;       // the round's one synchronisation: count -> apply
    const int64_t W = (int64_t)c[kWinners];
    *n_short = (int64_t)c[kShort];
    SG_REQUIRE(W >= 0 && W < V && 2 * W <= F, "sg_remesh_collapse: winner count %lld out of range", (long long)W);
    if (W == 0 || round >= max_rounds) break;
    if (int rc = apply_and_compact(s, W, V_before, nc, -1, stream)) return rc;
    counts[round] = W;
    *n_rounds = round + 1;
  }
  return SG_OK;
}

int remesh_collapse_maps(const sg_remesh* s, int64_t* vertex_ids, int64_t* merged_into, hipStream_t stream) {
  const bool called = s->map_before >= 0;
  const int64_t n_after = called ? s->map_after : s->V, n_before = called ? s->map_before : s->V;
  SG_REQUIRE((n_after == 0 || vertex_ids) && (n_before == 0 || merged_into), "sg_remesh_collapse_maps: null pointer");
  if (n_before == 0) return SG_OK;                  // nothing to write, no device to ask
  if (called) {
    if (n_after > 0) widen32<<<blocks_for(n_after), kThreads, 0, stream>>>(s->ids.p, n_after, vertex_ids);
    widen32<<<blocks_for(n_before), kThreads, 0, stream>>>(s->into.p, n_before, merged_into);
  } else {
    iota<<<blocks_for(n_after), kThreads, 0, stream>>>(vertex_ids, n_after);
    iota<<<blocks_for(n_before), kThreads, 0, stream>>>(merged_into, n_before);
  }
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

namespace {
// quad = the vertex quadrics of the mesh as it stands: one stable sort of the 3 F corners by vertex, one lane per vertex
int compute_quadrics(sg_remesh* s, hipStream_t stream) {
  const int64_t V = s->V, n = 3 * s->F;
  s->feat_C = -1;                                   // the sorted keys of the analysis are overwritten
  if (int rc = s->quad.reserve(10 * V, false, stream)) return rc;
  if (n == 0) {
    SG_HIP_TRY(hipMemsetAsync(s->quad.p, 0, (size_t)V * 10 * sizeof(double), stream));
    return SG_OK;
  }
  for (auto* b : {&s->keys_a, &s->keys_b})
    if (int rc = b->reserve(n, false, stream)) return rc;
  for (auto* b : {&s->vals_a, &s->vals_b})
    if (int rc = b->reserve(n, false, stream)) return rc;
  const int bits = bits_for((uint64_t)V, 32);
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, (int)n, 0, bits,
                                                stream));
  if (int rc = s->temp.reserve(tb ? tb : 16, false, stream)) return rc;
  corner_keys<<<blocks_for(n), kThreads, 0, stream>>>(s->tri.p, n, s->keys_a.p, s->vals_a.p);
  SG_HIP_TRY(hipGetLastError());
  tb = s->temp.cap;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(s->temp.p, tb, s->keys_a.p, s->keys_b.p, s->vals_a.p, s->vals_b.p, (int)n, 0, bits,
                                                stream));
  vertex_quadrics<<<blocks_for(V), kThreads, 0, stream>>>(s->keys_b.p, s->vals_b.p, n, V, s->tri.p, s->vs.p, s->quad.p);
  SG_HIP_TRY(hipGetLastError());
  s->quad_fresh = true;
  return SG_OK;
}
}  // namespace

int remesh_quadrics(sg_remesh* s, double* out, hipStream_t stream) {
  SG_REQUIRE(s->valid, "sg_remesh_quadrics: the mesh did not pass validation (sg_remesh_query)");
  if (s->V == 0) return SG_OK;                      // nothing to write, no device to ask
  SG_REQUIRE(out != nullptr, "sg_remesh_quadrics: null pointer");
  if (int rc = compute_quadrics(s, stream)) return rc;
  SG_HIP_TRY(hipMemcpyAsync(out, s->quad.p, (size_t)s->V * 10 * sizeof(double), hipMemcpyDeviceToDevice, stream));
  return SG_OK;
}

int remesh_simplify(sg_remesh* s, int64_t target_v, int quadrics_mode, int64_t max_rounds, hipStream_t stream, int64_t* counts,
                    int64_t* n_rounds, int64_t* n_refused) {
  SG_REQUIRE(s->valid, "sg_remesh_simplify: the mesh did not pass validation (sg_remesh_query)");
  SG_REQUIRE(!s->feat, "sg_remesh_simplify: the crease rules are on (sg_remesh_set_feature); crease-aware simplification is "
                       "not implemented");
  *n_rounds = 0;
  *n_refused = 0;
  s->map_before = s->map_after = s->V;
  if (s->V == 0) return SG_OK;
  const int64_t V_before = s->V;
  if (int rc = s->ids.reserve(V_before, false, stream)) return rc;
  if (int rc = s->into.reserve(V_before, false, stream)) return rc;
  iota<<<blocks_for(V_before), kThreads, 0, stream>>>(s->ids.p, V_before);
  iota<<<blocks_for(V_before), kThreads, 0, stream>>>(s->into.p, V_before);
  SG_HIP_TRY(hipGetLastError());
  if (s->F == 0 || s->V <= target_v) return SG_OK;
  if (!s->quad_fresh)                                          // once, on the mesh the call starts with; a caller that has just
    if (int rc = compute_quadrics(s, stream)) return rc;       // asked for them (sg_remesh_quadrics) does not pay twice
  s->quad_fresh = false;
  for (int64_t round = 0; s->V > target_v && s->F > 0; ++round) {
    const int64_t V = s->V, F = s->F, n = 3 * F, need = V - target_v;
    if (int rc = analyse(s, true, stream, true)) return rc;
    unsigned long long* sorted = reinterpret_cast<unsigned long long*>(s->keys_a.p);   // free once the analysis has sorted
    const unsigned long long* cand = s->cand.p;
    size_t tb_keys = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb_keys, cand, sorted, (int)n, 0, 64, stream));
    if (int rc = s->temp.reserve(tb_keys ? tb_keys : 16, false, stream)) return rc;
    SG_HIP_TRY(hipMemsetAsync(s->slot.p, 0, (size_t)V * sizeof(uint64_t), stream));
    simplify_price<<<blocks_for(n), kThreads, 0, stream>>>(s->keys_b.p, s->vals_b.p, s->head.p, s->incl.p, s->twin.p, n, V,
                                                          s->tri.p, s->vs.p, s->val.p, s->border.p, s->quad.p, s->cand.p,
                                                          s->ctr.p);
    SG_HIP_TRY(hipGetLastError());
    size_t tb = s->temp.cap;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(s->temp.p, tb, cand, sorted, (int)n, 0, 64, stream));
    simplify_cut<<<1, 1, 0, stream>>>(sorted, n, need, s->ctr.p);
    simplify_bid<<<blocks_for(n), kThreads, 0, stream>>>(s->cand.p, s->vals_b.p, s->twin.p, s->tri.p, s->val.p, s->border.p,
                                                        s->ctr.p, n, s->slot.p);
    simplify_check<<<blocks_for(n), kThreads, 0, stream>>>(s->cand.p, s->vals_b.p, s->twin.p, s->tri.p, s->val.p, s->border.p,
                                                          s->slot.p, n, s->win.p, s->ctr.p);
    SG_HIP_TRY(hipGetLastError());
    unsigned long long c[kCounters];
    if (int rc = read_counters(s, c, stream)) return rc;       // the round's one synchronisation: count -> apply
    const int64_t C = (int64_t)c[kCand], A = (int64_t)c[kAdmitted], W = (int64_t)c[kWinners];
    *n_refused = (int64_t)c[kRefused];
    SG_REQUIRE(C >= 0 && C <= n && A >= 0 && A <= need && A <= C && W >= 0 && W <= A && W < V && 2 * W <= F,
               "sg_remesh_simplify: counts out of range (%lld candidates, %lld admitted, %lld winners)", (long long)C,
               (long long)A, (long long)W);
    if (W == 0 || round >= max_rounds) break;
    if (int rc = apply_and_compact(s, W, V_before, nullptr, quadrics_mode, stream)) return rc;
    counts[3 * round] = C;
    counts[3 * round + 1] = A;
    counts[3 * round + 2] = W;
    *n_rounds = round + 1;
  }
  return SG_OK;
}

int remesh_export(const sg_remesh* s, float* vs, int64_t* faces, int64_t* parents, uint8_t* border, hipStream_t stream) {
  const int64_t V = s->V, F = s->F;
  SG_REQUIRE((V == 0 || (vs && parents)) && (F == 0 || faces), "sg_remesh_export: null pointer");
  if (V == 0 && F == 0) return SG_OK;               // nothing to write, no device to ask
  if (V > 0) {
    SG_HIP_TRY(hipMemcpyAsync(vs, s->vs.p, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    widen32<<<blocks_for(2 * V), kThreads, 0, stream>>>(s->par.p, 2 * V, parents);
    if (border) SG_HIP_TRY(hipMemcpyAsync(border, s->border.p, (size_t)V, hipMemcpyDeviceToDevice, stream));
  }
  if (F > 0) widen32<<<blocks_for(3 * F), kThreads, 0, stream>>>(s->tri.p, 3 * F, faces);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

void remesh_set_feature(sg_remesh* s, bool enabled, double cos_t) {
  s->feat = enabled;
  s->cos_t = enabled ? cos_t : 0.0;
  s->feat_C = -1;
}

int remesh_features(sg_remesh* s, hipStream_t stream, uint8_t* vclass, int64_t* crease_nbr, int64_t* n_crease) {
  *n_crease = 0;
  s->feat_C = -1;
  SG_REQUIRE(s->valid, "sg_remesh_features: the mesh did not pass validation (sg_remesh_query)");
  const int64_t V = s->V, F = s->F, n = 3 * F;
  if (V == 0) {                                     // nothing to write, no device to ask
    s->feat_C = 0;
    return SG_OK;
  }
  SG_REQUIRE(vclass && crease_nbr, "sg_remesh_features: null pointer");
  int64_t C = 0;
  if (F == 0) {
    SG_HIP_TRY(hipMemsetAsync(s->border.p, 0, (size_t)V, stream));
    vertex_classes<<<blocks_for(V), kThreads, 0, stream>>>(s->border.p, nullptr, nullptr, nullptr, V, vclass, crease_nbr);
    SG_HIP_TRY(hipGetLastError());
  } else {
    if (int rc = analyse(s, false, stream)) return rc;
    if (s->feat) {
      crease_flags<<<blocks_for(n + 1), kThreads, 0, stream>>>(s->crease.p, n, s->flag_a.p);
      SG_HIP_TRY(hipGetLastError());
      const int32_t* flag_a = s->flag_a.p;           // hipCUB's iterator arguments keep their const
      size_t tb = s->temp.cap;
      SG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s->temp.p, tb, flag_a, s->scan_a.p, (int)(n + 1), stream));
      store_crease_total<<<1, 1, 0, stream>>>(s->scan_a.p, n, s->ctr.p);
    }
    vertex_classes<<<blocks_for(V), kThreads, 0, stream>>>(s->border.p, s->feat ? s->nc.p : nullptr, s->clo.p, s->chi.p, V, vclass,
                                                          crease_nbr);
    SG_HIP_TRY(hipGetLastError());
    if (s->feat) {
      unsigned long long c[kCounters];
      if (int rc = read_counters(s, c, stream)) return rc;     // the one synchronisation: the caller sizes the edge list
      C = (int64_t)c[kTotalA];
      SG_REQUIRE(C >= 0 && C <= n, "sg_remesh_features: crease count %lld out of range", (long long)C);
    }
  }
  s->feat_C = *n_crease = C;
  return SG_OK;
}

int remesh_crease_edges(const sg_remesh* s, int64_t* edges, hipStream_t stream) {
  SG_REQUIRE(s->feat_C >= 0, "sg_remesh_crease_edges: call sg_remesh_features first (no operation in between)");
  if (s->feat_C == 0) return SG_OK;
  SG_REQUIRE(edges != nullptr, "sg_remesh_crease_edges: null pointer");
  const int64_t n = 3 * s->F;
  emit_crease_edges<<<blocks_for(n), kThreads, 0, stream>>>(s->crease.p, s->scan_a.p, s->keys_b.p, n, s->V, s->feat_C, edges);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

int crease_step(const float* in, float* out, const int64_t* crease_nbr, int64_t V, hipStream_t stream) {
  if (V == 0) return SG_OK;
  crease_step_kernel<<<blocks_for(V), kThreads, 0, stream>>>(in, crease_nbr, V, out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
