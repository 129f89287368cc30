// Vertex updating: the second half of the two-stage mesh denoiser (filter the face normals, then fit the vertices), on the
// device.  Replaces the reference's Models.vertex_updating (util/models.py:239-252), a Python loop over every vertex and
// every step.  The first half is csrc/mesh_bnf.hip.
//
// The rule (the specification; semigcn_amd/denoise.py states it in full).  One step, for all vertices at once from the
// positions p of the step before, float32, nothing fused (this file is built with -ffp-contract=off):
//   c_f  = ((p_a + p_b) + p_c) / 3.0f per component, a, b, c = faces[f]
//   s    = 0; for the faces f_1 < ... < f_k that name vertex i, in that order:
//            d = c_f - p_i;  t = (n_x d_x + n_y d_y) + n_z d_z;  s = s + t n_f
//   p_i' = p_i + s / float(k);  k == 0 or movable[i] == 0: p_i' is p_i bit for bit (such a vertex still feeds the centroids)
// The normals are used as given: not normalised, non-finite values propagate.
//
// Gather form, two launches per step: a centroid pass (one lane per face, three 16-byte gathers, one 16-byte store) and a
// vertex pass (one lane per vertex sums its own face list in ascending face order) -- no atomics, bit-reproducible.
// Positions live in two float4 buffers owned by the plan, (x, y, z, k) with k = the divisor as a float (0 = the vertex
// stays); the normals are packed once per run into float4 records as well, so that one incident face is two 16-byte loads.
// Bytes per step at valence d: vertex pass 36 d (centroid, normal, face id) + 16 (own) + 16 (store) + 8 (row bounds);
// centroid pass per face 12 (ids) + 48 (gathers) + 16 (store).  d = 6 and F = 2 V: 256 + 152 = 408 B per vertex.
#include <memory>
#include <new>

#include "mesh_common.h"

struct sg_vupdate {
  int64_t V = 0, F = 0, max_valence = 0, n_unused = 0;
  sg::DeviceBuf<int32_t> faces;    // [3 F] the triangle list in 32 bits
  sg::DeviceBuf<int32_t> rowptr;   // [V + 1]
  sg::DeviceBuf<int32_t> vf;       // [3 F] incident faces, ascending inside a row
  sg::DeviceBuf<float4> buf[2];    // [V] each: the ping-pong positions of sg_vupdate_run
  sg::DeviceBuf<float4> cent;      // [F] the centroids of the step
  sg::DeviceBuf<float4> nrm;       // [F] the normals of the run
};

namespace sg {
namespace {

// ---- plan ------------------------------------------------------------------------------------------------------------
// Corner h = 3 f + i puts face f on the list of vertex faces[f][i]: key (vertex << 32 | f).  flags[0]: vertex id out of
// range; flags[1]: degenerate face (repeated vertex).  Also keeps the triangle list in 32 bits (0 where it is out of range:
// the plan is refused then).
__global__ void corner_keys(const int64_t* __restrict__ faces, int64_t F, int64_t V, uint64_t* __restrict__ keys,
                            int32_t* __restrict__ faces32, int* __restrict__ flags) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const bool ok = a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
  if (!ok) flags[0] = 1;
  else if (a == b || b == c || c == a) flags[1] = 1;
  const int64_t v[3] = {a, b, c};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    keys[3 * f + i] = ok ? (((uint64_t)v[i] << 32) | (uint64_t)f) : ~(uint64_t)0;
    faces32[3 * f + i] = ok ? (int32_t)v[i] : 0;
  }
}

// vf[j] = the face of sorted key j; stats[0] = the largest valence, stats[1] = the number of vertices without a face
// (integer atomics, at plan creation only)
__global__ void face_lists(const uint64_t* __restrict__ sorted, int64_t n, const int32_t* __restrict__ rowptr, int64_t V,
                           int32_t* __restrict__ vf, int* __restrict__ stats) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) vf[j] = (int32_t)(sorted[j] & 0xffffffffull);
  if (j < V) {
    const int k = rowptr[j + 1] - rowptr[j];
    if (k == 0) atomicAdd(&stats[1], 1);
    else atomicMax(&stats[0], k);
  }
}

// ---- run -------------------------------------------------------------------------------------------------------------
// one launch over max(V, F) lanes: the positions with their divisor, and the normals as 16-byte records
__global__ __launch_bounds__(kThreads) void vupdate_pack(const float* __restrict__ pos, const int32_t* __restrict__ rowptr,
                                                         const uint8_t* __restrict__ movable, int64_t V,
                                                         const float* __restrict__ normals, int64_t F,
                                                         float4* __restrict__ buf, float4* __restrict__ nrm) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < V) {
    const int k = rowptr[i + 1] - rowptr[i];
    const float w = (movable && !movable[i]) ? 0.f : (float)k;
    buf[i] = make_float4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], w);
  }
  if (i < F) nrm[i] = make_float4(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], 0.f);
}

__global__ __launch_bounds__(kThreads) void vupdate_centroids(const int32_t* __restrict__ faces32, const float4* __restrict__ in,
                                                              int64_t F, float4* __restrict__ cent) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const float4 a = in[faces32[3 * f]], b = in[faces32[3 * f + 1]], c = in[faces32[3 * f + 2]];
  cent[f] = make_float4(__fdiv_rn((a.x + b.x) + c.x, 3.0f), __fdiv_rn((a.y + b.y) + c.y, 3.0f),
                        __fdiv_rn((a.z + b.z) + c.z, 3.0f), 0.f);
}

// One step of the vertices.  LAST: the result goes to the caller's [V, 3] array instead of the other buffer.
template <bool LAST>
__global__ __launch_bounds__(kThreads) void vupdate_step(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ vf,
                                                         const float4* __restrict__ cent, const float4* __restrict__ nrm,
                                                         const float4* __restrict__ in, int64_t V, float4* __restrict__ out4,
                                                         float* __restrict__ out3) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= V) return;
  const float4 me = in[i];
  float x = me.x, y = me.y, z = me.z;
  if (me.w != 0.f) {
    const int e1 = rowptr[i + 1];
    int e = rowptr[i];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    // four faces in flight at a time (the ids, then the two gathers each, are independent loads); the sum keeps list order
    for (; e + 4 <= e1; e += 4) {
      float4 c[4], n[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = vf[e + j];
        c[j] = cent[f];
        n[j] = nrm[f];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dx = c[j].x - me.x, dy = c[j].y - me.y, dz = c[j].z - me.z;
        const float t = (n[j].x * dx + n[j].y * dy) + n[j].z * dz;
        sx = sx + t * n[j].x;
        sy = sy + t * n[j].y;
        sz = sz + t * n[j].z;
      }
    }
    for (; e < e1; ++e) {
      const int f = vf[e];
      const float4 c = cent[f], n = nrm[f];
      const float dx = c.x - me.x, dy = c.y - me.y, dz = c.z - me.z;
      const float t = (n.x * dx + n.y * dy) + n.z * dz;
      sx = sx + t * n.x;
      sy = sy + t * n.y;
      sz = sz + t * n.z;
    }
    x = me.x + __fdiv_rn(sx, me.w);
    y = me.y + __fdiv_rn(sy, me.w);
    z = me.z + __fdiv_rn(sz, me.w);
  }
  if (LAST) {
    out3[3 * i] = x;
    out3[3 * i + 1] = y;
    out3[3 * i + 2] = z;
  } else {
    out4[i] = make_float4(x, y, z, me.w);
  }
}

}  // namespace

void destroy_vupdate(sg_vupdate* s) { delete s; }

void vupdate_query(const sg_vupdate* s, int64_t* info) {
  info[0] = s->V;
  info[1] = s->F;
  info[2] = s->max_valence;
  info[3] = s->n_unused;
}

int vupdate_create(const int64_t* faces, int64_t F, int64_t V, hipStream_t stream, sg_vupdate** out) {
  const int64_t n = 3 * F;
  SG_REQUIRE(V < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), "sg_vupdate_create: sizes must fit int32");
  SG_REQUIRE(F == 0 || V > 0, "sg_vupdate_create: face refers to a vertex outside [0, 0)");   // known without reading one
  std::unique_ptr<sg_vupdate> s(new (std::nothrow) sg_vupdate);
  SG_REQUIRE(s != nullptr, "sg_vupdate_create: out of host memory");
  s->V = V;
  s->F = F;
  s->n_unused = V;
  if (F == 0) {            // nothing to build: every vertex stays, and no device is touched
    *out = s.release();
    return SG_OK;
  }
  SG_HIP_TRY(s->faces.alloc(n));
  SG_HIP_TRY(s->rowptr.alloc(V + 1));
  SG_HIP_TRY(s->vf.alloc(n));
  SG_HIP_TRY(s->buf[0].alloc(V));
  SG_HIP_TRY(s->buf[1].alloc(V));
  SG_HIP_TRY(s->cent.alloc(F));
  SG_HIP_TRY(s->nrm.alloc(F));

  DeviceBuf<uint64_t> keys_a, keys_b;
  DeviceBuf<int> flags;     // [0], [1]: corner_keys; [2], [3]: the stats of face_lists
  DeviceBuf<char> temp;
  int h_flags[4] = {0, 0, 0, 0};
  SG_HIP_TRY(flags.alloc(4));
  SG_HIP_TRY(hipMemsetAsync(flags.p, 0, 4 * sizeof(int), stream));
  SG_HIP_TRY(keys_a.alloc(n));
  SG_HIP_TRY(keys_b.alloc(n));
  corner_keys<<<blocks_for(F), kThreads, 0, stream>>>(faces, F, V, keys_a.p, s->faces.p, flags.p);
  SG_HIP_TRY(hipGetLastError());
  const int end_bit = 32 + bits_for((uint64_t)V, 32);
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys_a.p, keys_b.p, (int)n, 0, end_bit, stream));
  SG_HIP_TRY(temp.alloc(tb ? tb : 16));
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, tb, keys_a.p, keys_b.p, (int)n, 0, end_bit, stream));
  SG_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));
  SG_REQUIRE(!h_flags[0], "sg_vupdate_create: face refers to a vertex outside [0, %lld)", (long long)V);
  SG_REQUIRE(!h_flags[1], "sg_vupdate_create: degenerate face (repeated vertex)");
  row_starts<<<blocks_for(V + 1), kThreads, 0, stream>>>(keys_b.p, n, V, s->rowptr.p);
  SG_HIP_TRY(hipGetLastError());
  face_lists<<<blocks_for(n > V ? n : V), kThreads, 0, stream>>>(keys_b.p, n, s->rowptr.p, V, s->vf.p, flags.p + 2);
  SG_HIP_TRY(hipGetLastError());
  SG_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));   // the temporaries are freed on return
  SG_REQUIRE(h_flags[2] >= 1 && h_flags[2] <= F && h_flags[3] >= 0 && h_flags[3] < V, "sg_vupdate_create: counts out of range");
  s->max_valence = h_flags[2];
  s->n_unused = h_flags[3];
  *out = s.release();
  return SG_OK;
}

int vupdate_run(sg_vupdate* s, const float* pos, const float* normals, const uint8_t* movable, int steps, float* out,
                hipStream_t stream) {
  const int64_t V = s->V, F = s->F;
  const float *pe = pos + 3 * V, *oe = out + 3 * V;
  SG_REQUIRE(V == 0 || oe <= pos || pe <= out, "sg_vupdate_run: out overlaps pos");
  if (V == 0) return SG_OK;
  if (steps == 0 || F == 0) {
    SG_HIP_TRY(hipMemcpyAsync(out, pos, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return SG_OK;
  }
  const unsigned grid_v = blocks_for(V), grid_f = blocks_for(F);
  vupdate_pack<<<grid_v > grid_f ? grid_v : grid_f, kThreads, 0, stream>>>(pos, s->rowptr.p, movable, V, normals, F, s->buf[0].p,
                                                                           s->nrm.p);
  SG_HIP_TRY(hipGetLastError());
  float4 *a = s->buf[0].p, *b = s->buf[1].p;
  for (int r = 0; r < steps; ++r) {
    vupdate_centroids<<<grid_f, kThreads, 0, stream>>>(s->faces.p, a, F, s->cent.p);
    if (r + 1 < steps) {
      vupdate_step<false><<<grid_v, kThreads, 0, stream>>>(s->rowptr.p, s->vf.p, s->cent.p, s->nrm.p, a, V, b, nullptr);
      float4* t = a; a = b; b = t;
    } else {
      vupdate_step<true><<<grid_v, kThreads, 0, stream>>>(s->rowptr.p, s->vf.p, s->cent.p, s->nrm.p, a, V, nullptr, out);
    }
  }
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
