// Connected components of a triangle list on the device, selection by component and a stable compaction of what is kept.
//
// Replaces the first step of MeshFix.repair() in the reference's preprocess/prepare.py:28-33: everything but the scan's
// main component goes before the holes are closed (mesh_fill.hip).  The specification is semigcn_amd/components.py; in short:
//
//   degenerate a face with a repeated vertex: label -1, links to nothing, never kept, counted.
//   links      edge (0): every half-edge of a non-degenerate face is keyed lo * V + hi (undirected) with its face as the
//              value; one radix sort over the 3 F pairs, restricted to the bits V * V needs, makes the faces of an edge
//              neighbours, and every position whose key equals its predecessor's links the two faces (a run of n faces on a
//              non-manifold edge is a chain of n - 1 links).  vertex (1): the union runs over the VERTICES with the links
//              (f0, f1) and (f1, f2) of every non-degenerate face, no sort; a face then takes the root of its f0, and an
//              atomicMin of face indices into a slot per root vertex turns that root into the component's smallest face.
//   union      lock-free union-find on an int32 parent array, one thread per link, no host round trip and no launch per
//              round.  find halves the path as it goes; the root with the LARGER index is hooked under the root with the
//              smaller one by atomicCAS(parent[hi], hi, lo).  A flatten pass follows.  The representative of a component is
//              therefore its smallest member, whatever order the atomics took: the labels are deterministic.
//   labels     components are numbered 0 .. K - 1 by ascending smallest face: mark the representatives, ExclusiveSum,
//              gather.  face_count by integer atomicAdd (order-independent); the largest component by one atomicMax of
//              count << 32 | ~id, so that ties go to the lower id.
//   select     a face is kept when its component is, a vertex when a kept face uses it; two flag arrays, two exclusive
//              scans.  emit copies the kept rows in their old order (a stable compaction) and renumbers the faces.
//
// The union-find itself and the proof that it terminates are in mesh_union.h (mesh_manifold.hip uses the same one).
//
// All of it is integer work bound by the sort and by scattered 4-byte accesses.
#include <memory>
#include <new>

#include "mesh_common.h"
#include "mesh_union.h"

struct sg_parts {
  int64_t V = 0, F = 0, K = 0, n_degenerate = 0, largest = -1, largest_count = 0;
  sg::DeviceBuf<int32_t> tri;      // [F][3] the faces as int32: select and emit run on the plan's own copy
  sg::DeviceBuf<int32_t> label;    // [F] component of every face, -1 = degenerate
  sg::DeviceBuf<unsigned long long> count;   // [K] faces per component (the callers' int64, as atomicAdd takes it)
  bool selected = false;
  int64_t Vk = 0, Fk = 0;
  sg::DeviceBuf<int32_t> flags;    // [F + 1] face kept, then [V + 1] vertex kept (the last entry of each is 0)
  sg::DeviceBuf<int32_t> new_id;   // their exclusive scans, same layout: the new ids, and the totals in the last entries
};
static_assert(sizeof(unsigned long long) == sizeof(int64_t), "sg_parts::count is cleared and copied out as int64");

namespace sg {
namespace {

// ---- faces -----------------------------------------------------------------------------------------------------------
// tri = the faces as int32; degen[f] = 1 for a face with a repeated vertex; flags[0]: a vertex id out of range (the face is
// stored as zeros); stats[0]: degenerate faces
__global__ void classify_faces(const int64_t* __restrict__ faces, int64_t F, int64_t V, int32_t* __restrict__ tri,
                               uint8_t* __restrict__ degen, int* __restrict__ flags, unsigned long long* __restrict__ stats) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  uint8_t d = 0;
  if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
    flags[0] = 1;
    d = 1;
    a = b = c = 0;
  } else if (a == b || b == c || c == a) {
    d = 1;
    atomicAdd(&stats[0], 1ull);
  }
  degen[f] = d;
  tri[3 * f] = (int32_t)a;
  tri[3 * f + 1] = (int32_t)b;
  tri[3 * f + 2] = (int32_t)c;
}

// edge links: half-edge h = 3 f + i keyed by its undirected edge, ~0 for a degenerate face (sorts last, links nothing)
__global__ void edge_keys(const int32_t* __restrict__ tri, const uint8_t* __restrict__ degen, int64_t n_half, int64_t V,
                          uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n_half) return;
  const int64_t f = h / 3;
  const int i = (int)(h - 3 * f);
  uint64_t key = ~0ull;
  if (!degen[f]) {
    const int64_t a = tri[3 * f + i], b = tri[3 * f + next3(i)];
    key = (uint64_t)(a < b ? a : b) * (uint64_t)V + (uint64_t)(a < b ? b : a);
  }
  keys[h] = key;
  vals[h] = (int32_t)f;
}

__global__ void union_sorted_edges(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int64_t F,
                                   int32_t* __restrict__ parent) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < 1 || p >= n) return;
  const uint64_t k = keys[p];
  if (k == ~0ull || keys[p - 1] != k) return;
  const int32_t a = vals[p], b = vals[p - 1];
  if (a < 0 || a >= F || b < 0 || b >= F) return;
  unite(parent, a, b);
}

// vertex links: thread t < 2 F is link (f_i, f_{i+1}), i = t & 1, of face t >> 1
__global__ void union_face_vertices(const int32_t* __restrict__ tri, const uint8_t* __restrict__ degen, int64_t F,
                                    int32_t* __restrict__ parent) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * F) return;
  const int64_t f = t >> 1;
  if (degen[f]) return;
  const int i = (int)(t & 1);
  unite(parent, tri[3 * f + i], tri[3 * f + i + 1]);
}

// vertex mode: slot[root vertex] = the smallest face of the component (slot preset to 0x7f7f7f7f, above any face index)
__global__ void min_face_of_root(const int32_t* __restrict__ tri, const uint8_t* __restrict__ degen, int64_t F,
                                 const int32_t* __restrict__ vroot, int32_t* __restrict__ slot) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F || degen[f]) return;
  atomicMin(slot + vroot[tri[3 * f]], (int32_t)f);
}

// rep[f] = smallest face of f's component, -1 for a degenerate face; is_rep[f] = 1 where rep[f] == f
__global__ void representatives(const int32_t* __restrict__ tri, const uint8_t* __restrict__ degen, int64_t F,
                                const int32_t* __restrict__ face_root, const int32_t* __restrict__ vroot,
                                const int32_t* __restrict__ slot, int32_t* __restrict__ rep, int32_t* __restrict__ is_rep) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > F) return;
  int32_t r = -1;
  if (f < F && !degen[f]) r = face_root ? face_root[f] : slot[vroot[tri[3 * f]]];
  if (f < F) rep[f] = r;
  is_rep[f] = (f < F && r == (int32_t)f) ? 1 : 0;          // entry F is 0: the scan ends on the total
}

__global__ void gather_labels(const int32_t* __restrict__ rep, const int32_t* __restrict__ rank, int64_t F, int64_t K,
                              int32_t* __restrict__ label, unsigned long long* __restrict__ count) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int32_t r = rep[f];
  int32_t l = -1;
  if (r >= 0 && r < F) {
    l = rank[r];
    if (l >= 0 && l < K) atomicAdd(&count[l], 1ull);
    else l = -1;
  }
  label[f] = l;
}

// best = max over the components of count << 32 | (0xffffffff - id): the most faces, ties to the lower id
__global__ void largest_component(const unsigned long long* __restrict__ count, int64_t K, unsigned long long* __restrict__ best) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  atomicMax(best, (count[k] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k));
}

// ---- select and emit ---------------------------------------------------------------------------------------------------
// vflag was zeroed; every thread that marks a vertex writes the same 1
__global__ void mark_kept(const int32_t* __restrict__ tri, const int32_t* __restrict__ label, const uint8_t* __restrict__ keep,
                          int64_t F, int64_t V, int64_t K, int32_t* __restrict__ fflag, int32_t* __restrict__ vflag) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > F) return;
  int32_t k = 0;
  if (f < F) {
    const int32_t l = label[f];
    k = (l >= 0 && l < K && keep[l]) ? 1 : 0;
    if (k) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int64_t v = tri[3 * f + i];
        if (v >= 0 && v < V) vflag[v] = 1;
      }
    }
  }
  fflag[f] = k;
}

__global__ void emit_kept_vertices(const float* __restrict__ vs, const int32_t* __restrict__ vflag, const int32_t* __restrict__ vnew,
                                   int64_t V, int64_t Vk, float* __restrict__ new_vs, int64_t* __restrict__ vertex_ids) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V || !vflag[v]) return;
  const int64_t n = vnew[v];
  if (n < 0 || n >= Vk) return;
  new_vs[3 * n] = vs[3 * v];
  new_vs[3 * n + 1] = vs[3 * v + 1];
  new_vs[3 * n + 2] = vs[3 * v + 2];
  vertex_ids[n] = v;
}

__global__ void emit_kept_faces(const int32_t* __restrict__ tri, const int32_t* __restrict__ fflag, const int32_t* __restrict__ fnew,
                                const int32_t* __restrict__ vnew, int64_t F, int64_t Fk, int64_t* __restrict__ new_faces,
                                int64_t* __restrict__ face_ids) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F || !fflag[f]) return;
  const int64_t n = fnew[f];
  if (n < 0 || n >= Fk) return;
  new_faces[3 * n] = vnew[tri[3 * f]];
  new_faces[3 * n + 1] = vnew[tri[3 * f + 1]];
  new_faces[3 * n + 2] = vnew[tri[3 * f + 2]];
  face_ids[n] = f;
}

}  // namespace

void destroy_parts(sg_parts* s) { delete s; }

int parts_create(const int64_t* faces, int64_t F, int64_t V, int connectivity, hipStream_t stream, sg_parts** out) {
  const int64_t n_half = 3 * F;
  SG_REQUIRE(V < ((int64_t)1 << 31) && n_half < ((int64_t)1 << 31), "sg_parts_create: sizes must fit int32");
  std::unique_ptr<sg_parts> s(new (std::nothrow) sg_parts);
  SG_REQUIRE(s != nullptr, "sg_parts_create: out of host memory");
  s->V = V;
  s->F = F;
  if (F == 0) {
    *out = s.release();
    return SG_OK;
  }

  DeviceBuf<uint8_t> degen;
  DeviceBuf<int> flags;
  DeviceBuf<unsigned long long> stats;
  DeviceBuf<int32_t> parent, slot, rep, is_rep, rank;
  int h_flags[1] = {0};
  unsigned long long h_stats[2] = {0, 0};                  // degenerate faces; the largest component, packed
  const int64_t n_nodes = connectivity == 0 ? F : V;
  SG_HIP_TRY(degen.alloc(F));
  SG_HIP_TRY(flags.alloc(1));
  SG_HIP_TRY(stats.alloc(2));
  SG_HIP_TRY(parent.alloc(n_nodes));
  SG_HIP_TRY(rep.alloc(F));
  SG_HIP_TRY(is_rep.alloc(F + 1));
  SG_HIP_TRY(rank.alloc(F + 1));
  SG_HIP_TRY(s->label.alloc(F));
  SG_HIP_TRY(s->tri.alloc(n_half));
  SG_HIP_TRY(hipMemsetAsync(flags.p, 0, sizeof(h_flags), stream));
  SG_HIP_TRY(hipMemsetAsync(stats.p, 0, sizeof(h_stats), stream));
  classify_faces<<<blocks_for(F), kThreads, 0, stream>>>(faces, F, V, s->tri.p, degen.p, flags.p, stats.p);
  SG_HIP_TRY(hipGetLastError());
  // the unions below index by vertex: nothing runs on ids that were not checked
  SG_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(!h_flags[0], "sg_parts_create: face refers to a vertex outside [0, %lld)", (long long)V);

  if (n_nodes > 0) iota32<<<blocks_for(n_nodes), kThreads, 0, stream>>>(parent.p, n_nodes);
  SG_HIP_TRY(hipGetLastError());
  if (connectivity == 0) {
    DeviceBuf<uint64_t> keys_a, keys_b;
    DeviceBuf<int32_t> vals_a, vals_b;
    DeviceBuf<char> temp;
    SG_HIP_TRY(keys_a.alloc(n_half));
    SG_HIP_TRY(keys_b.alloc(n_half));
    SG_HIP_TRY(vals_a.alloc(n_half));
    SG_HIP_TRY(vals_b.alloc(n_half));
    edge_keys<<<blocks_for(n_half), kThreads, 0, stream>>>(s->tri.p, degen.p, n_half, V, keys_a.p, vals_a.p);
    SG_HIP_TRY(hipGetLastError());
    const int bits = bits_for((uint64_t)V * (uint64_t)V, 62);   // the keys are below V * V < 2^62; ~0 has every sorted bit set
    size_t tb = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)n_half, 0, bits,
                                                  stream));
    SG_HIP_TRY(temp.alloc(tb ? tb : 16));
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp.p, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (int)n_half, 0, bits,
                                                  stream));
    union_sorted_edges<<<blocks_for(n_half), kThreads, 0, stream>>>(keys_b.p, vals_b.p, n_half, F, parent.p);
    SG_HIP_TRY(hipGetLastError());
    flatten<<<blocks_for(F), kThreads, 0, stream>>>(parent.p, F);
    representatives<<<blocks_for(F + 1), kThreads, 0, stream>>>(s->tri.p, degen.p, F, parent.p, nullptr, nullptr, rep.p, is_rep.p);
    SG_HIP_TRY(hipGetLastError());
    SG_HIP_TRY(hipStreamSynchronize(stream));              // the sort's buffers are freed here
  } else {
    SG_HIP_TRY(slot.alloc(V));
    SG_HIP_TRY(hipMemsetAsync(slot.p, 0x7f, (size_t)(V > 0 ? V : 1) * sizeof(int32_t), stream));   // 0x7f7f7f7f > any face
    union_face_vertices<<<blocks_for(2 * F), kThreads, 0, stream>>>(s->tri.p, degen.p, F, parent.p);
    SG_HIP_TRY(hipGetLastError());
    if (V > 0) flatten<<<blocks_for(V), kThreads, 0, stream>>>(parent.p, V);
    min_face_of_root<<<blocks_for(F), kThreads, 0, stream>>>(s->tri.p, degen.p, F, parent.p, slot.p);
    representatives<<<blocks_for(F + 1), kThreads, 0, stream>>>(s->tri.p, degen.p, F, nullptr, parent.p, slot.p, rep.p, is_rep.p);
    SG_HIP_TRY(hipGetLastError());
  }
  if (int rc = exclusive_sum(is_rep.p, rank.p, F + 1, stream)) return rc;
  int32_t K32 = 0;
  SG_HIP_TRY(hipMemcpyAsync(&K32, rank.p + F, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  const int64_t K = K32;
  SG_REQUIRE(K >= 0 && K <= F, "sg_parts_create: component count %lld out of range", (long long)K);
  SG_HIP_TRY(s->count.alloc(K));
  SG_HIP_TRY(hipMemsetAsync(s->count.p, 0, (size_t)(K > 0 ? K : 1) * sizeof(int64_t), stream));
  gather_labels<<<blocks_for(F), kThreads, 0, stream>>>(rep.p, rank.p, F, K, s->label.p, s->count.p);
  if (K > 0) largest_component<<<blocks_for(K), kThreads, 0, stream>>>(s->count.p, K, stats.p + 1);
  SG_HIP_TRY(hipGetLastError());
  SG_HIP_TRY(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));                // the temporaries are freed on return
  s->K = K;
  s->n_degenerate = (int64_t)h_stats[0];
  if (K > 0) {
    s->largest = (int64_t)(0xffffffffu - (uint32_t)(h_stats[1] & 0xffffffffull));
    s->largest_count = (int64_t)(h_stats[1] >> 32);
    SG_REQUIRE(s->largest >= 0 && s->largest < K, "sg_parts_create: largest component %lld out of range", (long long)s->largest);
  }
  *out = s.release();
  return SG_OK;
}

void parts_query(const sg_parts* s, int64_t* info) {
  info[0] = s->K;
  info[1] = s->F;
  info[2] = s->V;
  info[3] = s->n_degenerate;
  info[4] = s->largest;
  info[5] = s->largest_count;
  info[6] = s->selected ? s->Vk : -1;
  info[7] = s->selected ? s->Fk : -1;
}

int parts_labels(const sg_parts* s, int64_t* face_label, int64_t* face_count, hipStream_t stream) {
  SG_REQUIRE((s->F == 0 || face_label) && (s->K == 0 || face_count), "sg_parts_labels: null pointer");
  if (s->F > 0) widen32<<<blocks_for(s->F), kThreads, 0, stream>>>(s->label.p, s->F, face_label);
  SG_HIP_TRY(hipGetLastError());
  if (s->K > 0) SG_HIP_TRY(hipMemcpyAsync(face_count, s->count.p, (size_t)s->K * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  return SG_OK;
}

int parts_select(sg_parts* s, const uint8_t* keep, hipStream_t stream, int64_t* n_vertices,
                 int64_t* n_faces) {
  const int64_t F = s->F, V = s->V, n = (F + 1) + (V + 1);
  s->selected = false;
  *n_vertices = *n_faces = 0;
  if (!s->flags.p) {
    SG_HIP_TRY(s->flags.alloc(n));
    SG_HIP_TRY(s->new_id.alloc(n));
  }
  int32_t* fflag = s->flags.p;
  int32_t* vflag = s->flags.p + (F + 1);
  SG_HIP_TRY(hipMemsetAsync(vflag, 0, (size_t)(V + 1) * sizeof(int32_t), stream));
  mark_kept<<<blocks_for(F + 1), kThreads, 0, stream>>>(s->tri.p, s->label.p, keep, F, V, s->K, fflag, vflag);
  SG_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_sum(fflag, s->new_id.p, F + 1, stream)) return rc;
  if (int rc = exclusive_sum(vflag, s->new_id.p + (F + 1), V + 1, stream)) return rc;
  int32_t totals[2] = {0, 0};
  SG_HIP_TRY(hipMemcpyAsync(&totals[0], s->new_id.p + F, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipMemcpyAsync(&totals[1], s->new_id.p + (F + 1) + V, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(totals[0] >= 0 && totals[0] <= F && totals[1] >= 0 && totals[1] <= V, "sg_parts_select: totals out of range");
  s->Fk = totals[0];
  s->Vk = totals[1];
  s->selected = true;
  *n_vertices = s->Vk;
  *n_faces = s->Fk;
  return SG_OK;
}

int parts_emit(sg_parts* s, const float* vs, float* new_vs, int64_t* new_faces, int64_t* vertex_ids,
               int64_t* face_ids, hipStream_t stream) {
  SG_REQUIRE(s->selected, "sg_parts_emit: call sg_parts_select first");
  SG_REQUIRE((s->Vk == 0 || (vs && new_vs && vertex_ids)) && (s->Fk == 0 || (new_faces && face_ids)), "sg_parts_emit: null pointer");
  const int64_t F = s->F, V = s->V;
  const int32_t* vnew = s->new_id.p + (F + 1);
  if (s->Vk > 0)
    emit_kept_vertices<<<blocks_for(V), kThreads, 0, stream>>>(vs, s->flags.p + (F + 1), vnew, V, s->Vk, new_vs, vertex_ids);
  if (s->Fk > 0)
    emit_kept_faces<<<blocks_for(F), kThreads, 0, stream>>>(s->tri.p, s->flags.p, s->new_id.p, vnew, F, s->Fk, new_faces, face_ids);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
