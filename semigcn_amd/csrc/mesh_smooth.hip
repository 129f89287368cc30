// Network inputs from a remeshed scan: mean edge length and uniform-weight Laplacian smoothing, on the device.
//
// Replaces the tail of the reference's preprocess/prepare.py:
//   edge_based_scaling   :48-52    sum ||vs[a] - vs[b]|| / E over the unique edges (numpy over a Mesh object)
//   smooth               :110-114  pymeshlab's laplacian_smooth, stepsmoothnum=30, cotangentweight=False
//
// The smoothing operator (the specification; MeshLab's own code is not available here, parity with it is unverified):
//   k_ij = number of faces that use the undirected edge {i, j}; an edge with k = 1 is a border edge; a vertex is a border
//   vertex if any of its edges is a border edge.  Weights: interior vertex w_ij = k_ij; border vertex w_ij = 1 on its border
//   edges and 0 on all its other edges.  One step is Jacobi:  p_i <- (p_i + sum_j w_ij p_j) / (1 + sum_j w_ij).
//   A vertex without edges, or with movable[i] == 0, keeps its position.
//
// Gather form: one thread per vertex sums its own neighbour list (ascending neighbour id) -- no atomics, bit-reproducible.
// Positions live in two float4 buffers owned by the plan, (x, y, z, den) with den = 1 + sum_j w_ij (0 = the vertex stays),
// so that one neighbour is one 16-byte load and the divisor rides along with the vertex's own position.
// Bytes per step and vertex at valence d: 16 d (gathers) + 16 (own) + 16 (store) + 4 d (ids) + d (weights) + 8 (row bounds);
// d = 6: 166 B, of which the 32 MB of positions of a 1 M mesh stay in the last-level cache from step to step.
#include <memory>
#include <new>

#include "mesh_common.h"

struct sg_smooth {
  int64_t V = 0, nnz = 0;
  sg::DeviceBuf<int32_t> rowptr;   // [V + 1]
  sg::DeviceBuf<int32_t> idx;      // [nnz] neighbour ids, ascending inside a row
  sg::DeviceBuf<uint8_t> w;        // [nnz] w_ij (0: an interior edge of a border vertex)
  sg::DeviceBuf<float> den;        // [V] 1 + sum_j w_ij, 0 for a vertex without weighted edges
  sg::DeviceBuf<float4> buf[2];    // [V] each: the ping-pong positions of sg_smooth_run
};

namespace sg {
namespace {

constexpr int kRedBlocks = 1024;

// ---- mean edge length ------------------------------------------------------------------------------------------------
// float32 lengths, float64 sums: per thread over a grid-stride walk, then over the block, in a fixed order.  An edge that
// names a vertex outside [0, V) contributes NaN instead of being read.
__global__ __launch_bounds__(kThreads) void edge_length_partial(const float* __restrict__ vs, int64_t V,
                                                                const int64_t* __restrict__ edges, int64_t E,
                                                                double* __restrict__ part) {
  __shared__ double s_w[kThreads / 64];
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < E; e += (int64_t)gridDim.x * kThreads) {
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || a >= V || b < 0 || b >= V) {
      acc += __builtin_nan("");
    } else {
      const float dx = vs[3 * a] - vs[3 * b], dy = vs[3 * a + 1] - vs[3 * b + 1], dz = vs[3 * a + 2] - vs[3 * b + 2];
      acc += (double)sqrtf(dx * dx + dy * dy + dz * dz);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// one workgroup: out = (sum of the partials) / E; E == 0 gives 0 / 0 = NaN as the reference's division does
__global__ __launch_bounds__(kThreads) void edge_length_finish(const double* __restrict__ part, int64_t nb, int64_t E,
                                                               double* __restrict__ out) {
  __shared__ double s_w[kThreads / 64];
  double a = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kThreads) a += part[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3])) / (double)E;
}

// ---- plan ------------------------------------------------------------------------------------------------------------
// directed_keys and row_starts (mesh_common.h) give the sorted (source, neighbour) runs and the row bounds.
// A run's length is k_ij.  flags[2]: an edge with more than 255 faces (the weight is kept in 8 bits).
__global__ void row_weights(const uint64_t* __restrict__ ukeys, const int32_t* __restrict__ counts,
                            const int32_t* __restrict__ rowptr, int64_t V, int32_t* __restrict__ idx, uint8_t* __restrict__ w,
                            float* __restrict__ den, int* __restrict__ flags) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int b = rowptr[v], e = rowptr[v + 1];
  bool border = false;
  for (int j = b; j < e; ++j) border |= counts[j] == 1;
  int64_t sum = 0;
  for (int j = b; j < e; ++j) {
    const int c = counts[j];
    if (c > 255) flags[2] = 1;
    const int wt = border ? (c == 1 ? 1 : 0) : (c > 255 ? 255 : c);
    idx[j] = (int32_t)(ukeys[j] & 0xffffffffull);
    w[j] = (uint8_t)wt;
    sum += wt;
  }
  den[v] = sum > 0 ? (float)(1 + sum) : 0.f;
}

// ---- run -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void smooth_pack(const float* __restrict__ in, const float* __restrict__ den,
                                                        const uint8_t* __restrict__ movable, int64_t V,
                                                        float4* __restrict__ buf) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= V) return;
  const float d = (movable && !movable[i]) ? 0.f : den[i];
  buf[i] = make_float4(in[3 * i], in[3 * i + 1], in[3 * i + 2], d);
}

// One Jacobi step.  LAST: the result goes to the caller's [V, 3] array instead of the other buffer.
template <bool LAST>
__global__ __launch_bounds__(kThreads) void smooth_step(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ idx,
                                                        const uint8_t* __restrict__ w, const float4* __restrict__ in, int64_t V,
                                                        float4* __restrict__ out4, float* __restrict__ out3) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= V) return;
  const float4 me = in[i];
  float x = me.x, y = me.y, z = me.z;
  if (me.w != 0.f) {
    const int e1 = rowptr[i + 1];
    int e = rowptr[i];
    // four neighbours in flight at a time (the ids, then the gathers, are independent loads); the sums keep list order
    for (; e + 4 <= e1; e += 4) {
      float4 p[4];
      float wt[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wt[j] = (float)w[e + j];
        p[j] = in[idx[e + j]];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (wt[j] != 0.f) {     // a zero weight drops the term itself, whatever the neighbour holds
          x += wt[j] * p[j].x;
          y += wt[j] * p[j].y;
          z += wt[j] * p[j].z;
        }
      }
    }
    for (; e < e1; ++e) {
      const float wt = (float)w[e];
      if (wt != 0.f) {
        const float4 p = in[idx[e]];
        x += wt * p.x;
        y += wt * p.y;
        z += wt * p.z;
      }
    }
    x = __fdiv_rn(x, me.w);
    y = __fdiv_rn(y, me.w);
    z = __fdiv_rn(z, me.w);
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

int64_t edge_length_blocks(int64_t E) {
  const int64_t nb = (E + kThreads - 1) / kThreads;
  return nb < 1 ? 1 : (nb > kRedBlocks ? kRedBlocks : nb);
}

int launch_mean_edge_length(const float* vs, int64_t V, const int64_t* edges, int64_t E, double* partial, double* out,
                            hipStream_t stream) {
  const int64_t nb = edge_length_blocks(E);
  edge_length_partial<<<(unsigned)nb, kThreads, 0, stream>>>(vs, V, edges, E, partial);
  edge_length_finish<<<1, kThreads, 0, stream>>>(partial, nb, E, out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

void destroy_smooth(sg_smooth* s) { delete s; }

int smooth_create(const int64_t* faces, int64_t F, int64_t V, hipStream_t stream, sg_smooth** out) {
  const int64_t n_half = 3 * F, n_dir = 6 * F;
  SG_REQUIRE(V < ((int64_t)1 << 31) && n_dir < ((int64_t)1 << 31), "sg_smooth_create: sizes must fit int32");
  std::unique_ptr<sg_smooth> s(new (std::nothrow) sg_smooth);
  SG_REQUIRE(s != nullptr, "sg_smooth_create: out of host memory");
  s->V = V;
  SG_HIP_TRY(s->rowptr.alloc(V + 1));
  SG_HIP_TRY(s->den.alloc(V));
  SG_HIP_TRY(s->buf[0].alloc(V));
  SG_HIP_TRY(s->buf[1].alloc(V));

  DeviceBuf<uint64_t> keys_a, keys_b, ukeys;
  DeviceBuf<int32_t> counts;
  DeviceBuf<int> n_runs, flags;
  DeviceBuf<char> temp;
  int h_runs = 0, h_flags[3] = {0, 0, 0};
  SG_HIP_TRY(flags.alloc(3));
  SG_HIP_TRY(hipMemsetAsync(flags.p, 0, 3 * sizeof(int), stream));
  if (F > 0) {
    SG_HIP_TRY(keys_a.alloc(n_dir));
    SG_HIP_TRY(keys_b.alloc(n_dir));
    SG_HIP_TRY(ukeys.alloc(n_dir));
    SG_HIP_TRY(counts.alloc(n_dir));
    SG_HIP_TRY(n_runs.alloc(1));
    directed_keys<<<blocks_for(n_half), kThreads, 0, stream>>>(faces, n_half, V, keys_a.p, flags.p);
    SG_HIP_TRY(hipGetLastError());
    const int hi_bits = bits_for((uint64_t)V, 32);
    const uint64_t* sorted = keys_b.p;      // hipCUB's iterator argument keeps the const it had
    size_t t1 = 0, t2 = 0;
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, t1, keys_a.p, keys_b.p, (int)n_dir, 0, 32 + hi_bits, stream));
    SG_HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, t2, sorted, ukeys.p, counts.p, n_runs.p, (int)n_dir, stream));
    const size_t tb = t1 > t2 ? t1 : t2;
    SG_HIP_TRY(temp.alloc(tb ? tb : 16));
    SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, t1, keys_a.p, keys_b.p, (int)n_dir, 0, 32 + hi_bits, stream));
    SG_HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(temp.p, t2, sorted, ukeys.p, counts.p, n_runs.p, (int)n_dir, stream));
    SG_HIP_TRY(hipMemcpyAsync(&h_runs, n_runs.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    SG_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, stream));
    SG_HIP_TRY(hipStreamSynchronize(stream));
    SG_REQUIRE(!h_flags[0], "sg_smooth_create: face refers to a vertex outside [0, %lld)", (long long)V);
    SG_REQUIRE(!h_flags[1], "sg_smooth_create: degenerate face (repeated vertex)");
    SG_REQUIRE(h_runs >= 0 && h_runs <= n_dir, "sg_smooth_create: run count %d out of range", h_runs);
  }
  s->nnz = h_runs;
  SG_HIP_TRY(s->idx.alloc(h_runs));
  SG_HIP_TRY(s->w.alloc(h_runs));
  row_starts<<<blocks_for(V + 1), kThreads, 0, stream>>>(ukeys.p, h_runs, V, s->rowptr.p);
  SG_HIP_TRY(hipGetLastError());
  if (V > 0) {
    row_weights<<<blocks_for(V), kThreads, 0, stream>>>(ukeys.p, counts.p, s->rowptr.p, V, s->idx.p, s->w.p, s->den.p, flags.p);
    SG_HIP_TRY(hipGetLastError());
  }
  SG_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, stream));
  SG_HIP_TRY(hipStreamSynchronize(stream));   // the temporaries are freed on return
  SG_REQUIRE(!h_flags[2], "sg_smooth_create: an edge with more than 255 faces");
  *out = s.release();
  return SG_OK;
}

int smooth_run(sg_smooth* s, const float* in, float* out, const uint8_t* movable, int steps, hipStream_t stream) {
  const int64_t V = s->V;
  if (V == 0) return SG_OK;
  if (steps == 0) {
    if (in != out) SG_HIP_TRY(hipMemcpyAsync(out, in, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return SG_OK;
  }
  const unsigned grid = blocks_for(V);
  smooth_pack<<<grid, kThreads, 0, stream>>>(in, s->den.p, movable, V, s->buf[0].p);
  SG_HIP_TRY(hipGetLastError());
  float4 *a = s->buf[0].p, *b = s->buf[1].p;
  for (int r = 0; r + 1 < steps; ++r) {
    smooth_step<false><<<grid, kThreads, 0, stream>>>(s->rowptr.p, s->idx.p, s->w.p, a, V, b, nullptr);
    float4* t = a; a = b; b = t;
  }
  smooth_step<true><<<grid, kThreads, 0, stream>>>(s->rowptr.p, s->idx.p, s->w.p, a, V, nullptr, out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
