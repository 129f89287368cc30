// Bilateral face-normal filter and the -CAD loss term built on it.
//
// Replaces, for the position tensor the network just produced:
//   Models.bnf                 util/models.py:209-237   `loop` rounds of bilateral filtering of the face normals
//   Loss.fn_bnf_detach_loss    util/loss.py:197-253     ltype 'l1mae': sum_f |n_filtered - fn|_1 / F, filter detached
// called by every training script under -CAD (sgcn.py:133-135, mgcn.py:146-148, mgcn_wo_gt.py:116-118).  A dozen small
// ATen kernels per round and their [F,3,3] gathers become 3 + loop launches over 16-byte per-face records; every
// reduction has a fixed order (block partials, then one workgroup adding them in double), no atomics anywhere.
//
// Scratch (sg_bnf_scratch_bytes, 16-byte aligned), five [F] arrays of 16-byte records and the reduction cells:
//   rec  float4 (fc.xyz, fa)        face centre and area, so that a neighbour costs one 16-byte load
//   ring int4   (g0, g1, g2, has)   the face ring in 32 bits with the reference's wrap applied (-1 reads face F-1);
//                                   bit j of `has` = slot j holds a neighbour
//   w    float4 (w0, w1, w2, -)     d_c per slot after the static pass; the first round turns it in place into
//                                   wc * fa[g] * has, which does not change between rounds
//   na, nb float4                   the normals of a round and of the next one (ping-pong)
//   part float[nb], sig float[4]    block partials of sqrt(d_c + 1e-12); sig = (sigma_c, 2 sigma_c^2)
#include "sg_common.h"

namespace sg {
namespace {

constexpr int kBlock = 256;

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 ld3(const float* p, int64_t i) { return F3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ F3 sub(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 cross(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float l1(F3 a, F3 b) { return fabsf(a.x - b.x) + fabsf(a.y - b.y) + fabsf(a.z - b.z); }

__device__ __forceinline__ float block_sum(float v, float* s_buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0) for (int w = 0; w < kBlock / 64; ++w) t += s_buf[w];
  __syncthreads();
  return t;
}

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// pass 1: fn (compute_fn: no epsilon), rec = (fc, fa), na = the normals the filter starts from (`start`, or fn).
// With loop == 0 there is no round: nf_out = the start normals and lpart = block partials of |start - fn|_1.
__global__ __launch_bounds__(kBlock) void bnf_geometry(const float* __restrict__ pos, const int64_t* __restrict__ faces,
                                                       const float* __restrict__ start, int64_t V, int64_t F,
                                                       float* __restrict__ fn, float4* __restrict__ rec, float4* __restrict__ na,
                                                       float* __restrict__ nf_out, float* __restrict__ lpart) {
  __shared__ float s_buf[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float diff = 0.f;
  if (i < F) {
    const F3 a = ld3(pos, clampi(faces[3 * i], V)), b = ld3(pos, clampi(faces[3 * i + 1], V)),
             c = ld3(pos, clampi(faces[3 * i + 2], V));
    const F3 cr = cross(sub(b, a), sub(c, a));
    const float sq = dot(cr, cr);
    const float len = sqrtf(sq);
    const F3 n = F3{cr.x / len, cr.y / len, cr.z / len};
    fn[3 * i] = n.x; fn[3 * i + 1] = n.y; fn[3 * i + 2] = n.z;
    rec[i] = make_float4(((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f,
                         0.5f * sqrtf(sq + 1.0e-12f));
    const F3 s = start ? ld3(start, i) : n;
    na[i] = make_float4(s.x, s.y, s.z, 0.f);
    if (nf_out) {
      nf_out[3 * i] = s.x; nf_out[3 * i + 1] = s.y; nf_out[3 * i + 2] = s.z;
      diff = l1(s, n);
    }
  }
  if (lpart) {      // uniform over the grid
    const float t = block_sum(diff, s_buf);
    if (threadIdx.x == 0) lpart[blockIdx.x] = t;
  }
}

// pass 2: the ring in 32 bits, d_c per slot, block partials of sqrt(d_c + 1e-12) over ALL three slots (a padded slot
// counts with the centre of the face it wraps to, as in the reference)
__global__ __launch_bounds__(kBlock) void bnf_static(const int64_t* __restrict__ f2f, const float4* __restrict__ rec, int64_t F,
                                                     int4* __restrict__ ring, float4* __restrict__ w, float* __restrict__ part) {
  __shared__ float s_buf[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float s = 0.f;
  if (i < F) {
    const float4 me = rec[i];
    int g[3];
    float d[3];
    int has = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t raw = f2f[3 * i + j];
      has |= (raw != -1) << j;
      g[j] = (int)clampi(raw < 0 ? raw + F : raw, F);
      const float4 o = rec[g[j]];
      const float dx = o.x - me.x, dy = o.y - me.y, dz = o.z - me.z;
      d[j] = dx * dx + dy * dy + dz * dz;
    }
    ring[i] = make_int4(g[0], g[1], g[2], has);
    w[i] = make_float4(d[0], d[1], d[2], 0.f);
    s = (sqrtf(d[0] + 1.0e-12f) + sqrtf(d[1] + 1.0e-12f)) + sqrtf(d[2] + 1.0e-12f);
  }
  const float t = block_sum(s, s_buf);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one workgroup: sig = (sigma_c, 2 sigma_c^2) from the partials, added in double in a fixed order
__global__ __launch_bounds__(256) void bnf_sigma(const float* __restrict__ part, int64_t nb, float count, float* __restrict__ sig) {
  __shared__ double s_w[4];
  double a = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += 256) a += part[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float sum = (float)((s_w[0] + s_w[1]) + (s_w[2] + s_w[3]));
    const float sigma = __fdiv_rn(sum, count);
    sig[0] = sigma;
    sig[1] = __fmul_rn(2.0f, __fmul_rn(sigma, sigma));
  }
}

// one round: n'[f] = normalise(sum_j wc ws fa[g] has n[g]).  FIRST: w still holds d_c; the static weight is formed from
// sigma_c and the neighbours' areas and stored for the later rounds.  LAST: the result goes to the caller's [F,3] array
// and the block partials of |n' - fn|_1 are written.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void bnf_round(const int4* __restrict__ ring, float4* __restrict__ w,
                                                    const float4* __restrict__ rec, const float* __restrict__ sig,
                                                    float two_sigma_s2, const float4* __restrict__ nin, int64_t F,
                                                    float4* __restrict__ nout, const float* __restrict__ fn,
                                                    float* __restrict__ nf_out, float* __restrict__ lpart) {
  __shared__ float s_buf[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float diff = 0.f;
  if (i < F) {
    const int4 r = ring[i];
    float4 ww = w[i];
    const float4 me = nin[i];
    const float4 n0 = nin[r.x], n1 = nin[r.y], n2 = nin[r.z];
    if (FIRST) {
      const float den = sig[1];
      ww.x = expf(-ww.x / den) * ((r.w & 1) ? rec[r.x].w : 0.f);
      ww.y = expf(-ww.y / den) * ((r.w & 2) ? rec[r.y].w : 0.f);
      ww.z = expf(-ww.z / den) * ((r.w & 4) ? rec[r.z].w : 0.f);
      if (!LAST) w[i] = ww;
    }
    float dx = n0.x - me.x, dy = n0.y - me.y, dz = n0.z - me.z;
    const float w0 = expf(-(dx * dx + dy * dy + dz * dz) / two_sigma_s2) * ww.x;
    dx = n1.x - me.x; dy = n1.y - me.y; dz = n1.z - me.z;
    const float w1 = expf(-(dx * dx + dy * dy + dz * dz) / two_sigma_s2) * ww.y;
    dx = n2.x - me.x; dy = n2.y - me.y; dz = n2.z - me.z;
    const float w2 = expf(-(dx * dx + dy * dy + dz * dz) / two_sigma_s2) * ww.z;
    F3 s = F3{(w0 * n0.x + w1 * n1.x) + w2 * n2.x, (w0 * n0.y + w1 * n1.y) + w2 * n2.y, (w0 * n0.z + w1 * n1.z) + w2 * n2.z};
    const float len = sqrtf(dot(s, s) + 1.0e-12f) + 1.0e-12f;
    s = F3{s.x / len, s.y / len, s.z / len};
    if (LAST) {
      nf_out[3 * i] = s.x; nf_out[3 * i + 1] = s.y; nf_out[3 * i + 2] = s.z;
      if (lpart) diff = l1(s, ld3(fn, i));
    } else {
      nout[i] = make_float4(s.x, s.y, s.z, 0.f);
    }
  }
  if (LAST && lpart) {      // uniform over the grid
    const float t = block_sum(diff, s_buf);
    if (threadIdx.x == 0) lpart[blockIdx.x] = t;
  }
}

// loss = [w_pos sqrt(S_p / n_v + 1e-6) + k1 S_n / n_f] + k2 S_b / F from the block partials of mesh_loss_fwd (may be absent:
// the bilateral term alone) and of the filter's last round; out = (loss, dloss/dS_p, dloss/dS_n, dloss/dS_b).
__global__ __launch_bounds__(256) void mesh_loss_cad_finalize(const float* __restrict__ partial, int64_t nb, float n_v, float n_f,
                                                              float w_pos, float k1, const float* __restrict__ bpart, int64_t nbb,
                                                              float n_faces, float k2, float* __restrict__ out) {
  __shared__ double s_w[3][4];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (partial)
    for (int64_t b = threadIdx.x; b < nb; b += 256) {
      a0 += partial[b * 2];
      a1 += partial[b * 2 + 1];
    }
  for (int64_t b = threadIdx.x; b < nbb; b += 256) a2 += bpart[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_down(a0, off, 64);
    a1 += __shfl_down(a1, off, 64);
    a2 += __shfl_down(a2, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_w[0][threadIdx.x >> 6] = a0;
    s_w[1][threadIdx.x >> 6] = a1;
    s_w[2][threadIdx.x >> 6] = a2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the mean in double, rounded once
    const float cad = __fmul_rn(k2, (float)(((s_w[2][0] + s_w[2][1]) + (s_w[2][2] + s_w[2][3])) / (double)n_faces));
    if (partial) {     // the same arithmetic as mesh_loss_finalize, then the -CAD term on top
      const float sp = (float)((s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]));
      const float sn = (float)((s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3]));
      const float root = sqrtf(__fadd_rn(__fdiv_rn(sp, n_v), 1.0e-6f));
      const float normal = n_f > 0.f ? __fmul_rn(k1, __fdiv_rn(sn, n_f)) : 0.f;
      out[0] = __fadd_rn(__fadd_rn(__fmul_rn(w_pos, root), normal), cad);
      out[1] = w_pos * 0.5f / (root * n_v);
      out[2] = n_f > 0.f ? k1 / n_f : 0.f;
    } else {
      out[0] = cad;
      out[1] = 0.f;
      out[2] = 0.f;
    }
    out[3] = k2 / n_faces;
  }
}

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// mesh_loss_bwd_corners with both normal terms in one pass: dL/dn = g[1] keep sgn(n - n_t) + g[2] sgn(n - n_filtered)
// (`tfn` may be null: the bilateral term alone), projected through the normalisation once.  n is READ from the forward's
// `fn`, not recomputed: the signs are then those of the very differences the loss value summed.
__global__ __launch_bounds__(kBlock) void mesh_loss_cad_bwd_corners(const float* __restrict__ pos, const int64_t* __restrict__ faces,
                                                                    const float* __restrict__ tfn, const float* __restrict__ fkeep,
                                                                    const float* __restrict__ fn, const float* __restrict__ nf,
                                                                    const float* __restrict__ g, int64_t F,
                                                                    float* __restrict__ corner) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= F) return;
  const float k = tfn ? g[1] * fkeep[i] : 0.f;
  const float kb = g[2];
  const F3 a = ld3(pos, faces[3 * i]), b = ld3(pos, faces[3 * i + 1]), c = ld3(pos, faces[3 * i + 2]);
  const F3 e1 = sub(b, a), e2 = sub(c, a);
  const F3 cr = cross(e1, e2);
  const float inv = 1.0f / sqrtf(dot(cr, cr));
  const F3 n = ld3(fn, i);
  const F3 t = ld3(nf, i);
  F3 s = F3{kb * sgn(n.x - t.x), kb * sgn(n.y - t.y), kb * sgn(n.z - t.z)};
  if (k != 0.f) {
    const F3 u = ld3(tfn, i);
    s = F3{s.x + k * sgn(n.x - u.x), s.y + k * sgn(n.y - u.y), s.z + k * sgn(n.z - u.z)};
  }
  const float ns = dot(n, s);
  const F3 gc = F3{(s.x - n.x * ns) * inv, (s.y - n.y * ns) * inv, (s.z - n.z * ns) * inv};
  const F3 g1 = cross(e2, gc);
  const F3 g2 = cross(gc, e1);
  float* o = corner + 9 * i;
  o[0] = -(g1.x + g2.x); o[1] = -(g1.y + g2.y); o[2] = -(g1.z + g2.z);
  o[3] = g1.x; o[4] = g1.y; o[5] = g1.z;
  o[6] = g2.x; o[7] = g2.y; o[8] = g2.z;
}

inline int64_t align4(int64_t n) { return (n + 3) & ~(int64_t)3; }

}  // namespace

int64_t bnf_blocks(int64_t F) { return F > 0 ? (F + kBlock - 1) / kBlock : 1; }

int64_t bnf_scratch_bytes(int64_t F) { return (20 * F + align4(bnf_blocks(F)) + 4) * (int64_t)sizeof(float); }

int launch_bnf_filter(const float* pos, const int64_t* faces, const int64_t* f2f, int64_t V, int64_t F, int loop, float sigma_s,
                      const float* start, float* fn, float* nf, float* lpart, void* scratch, hipStream_t stream) {
  const int grid = (int)bnf_blocks(F);
  if (F == 0) {
    if (lpart) SG_HIP_TRY(hipMemsetAsync(lpart, 0, sizeof(float), stream));
    return SG_OK;
  }
  float4* rec = (float4*)scratch;
  int4* ring = (int4*)(rec + F);
  float4* w = (float4*)(ring + F);
  float4* na = w + F;
  float4* nb = na + F;
  float* part = (float*)(nb + F);
  float* sig = part + align4(grid);
  bnf_geometry<<<grid, kBlock, 0, stream>>>(pos, faces, start, V, F, fn, rec, na, loop == 0 ? nf : nullptr,
                                            loop == 0 ? lpart : nullptr);
  SG_HIP_TRY(hipGetLastError());
  if (loop == 0) return SG_OK;
  bnf_static<<<grid, kBlock, 0, stream>>>(f2f, rec, F, ring, w, part);
  SG_HIP_TRY(hipGetLastError());
  bnf_sigma<<<1, 256, 0, stream>>>(part, grid, (float)(3 * F), sig);
  SG_HIP_TRY(hipGetLastError());
  const float den = (float)(2.0 * (double)sigma_s * (double)sigma_s);
  for (int r = 0; r < loop; ++r) {
    const bool first = r == 0, last = r == loop - 1;
    if (first && last) bnf_round<true, true><<<grid, kBlock, 0, stream>>>(ring, w, rec, sig, den, na, F, nb, fn, nf, lpart);
    else if (first) bnf_round<true, false><<<grid, kBlock, 0, stream>>>(ring, w, rec, sig, den, na, F, nb, fn, nf, lpart);
    else if (last) bnf_round<false, true><<<grid, kBlock, 0, stream>>>(ring, w, rec, sig, den, na, F, nb, fn, nf, lpart);
    else bnf_round<false, false><<<grid, kBlock, 0, stream>>>(ring, w, rec, sig, den, na, F, nb, fn, nf, lpart);
    SG_HIP_TRY(hipGetLastError());
    float4* t = na; na = nb; nb = t;
  }
  return SG_OK;
}

int launch_mesh_loss_cad_finalize(const float* partial, int64_t nb, float n_v, float n_f, float w_pos, float k1, const float* bpart,
                                  int64_t nbb, float n_faces, float k2, float* out, hipStream_t stream) {
  mesh_loss_cad_finalize<<<1, 256, 0, stream>>>(partial, nb, n_v, n_f, w_pos, k1, bpart, nbb, n_faces, k2, out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

int launch_mesh_loss_cad_bwd_corners(const float* pos, const int64_t* faces, const float* tfn, const float* fkeep, const float* fn,
                                     const float* nf, const float* g, int64_t F, float* corner, hipStream_t stream) {
  if (F > 0) {
    mesh_loss_cad_bwd_corners<<<(int)((F + kBlock - 1) / kBlock), kBlock, 0, stream>>>(pos, faces, tfn, fkeep, fn, nf, g, F, corner);
    SG_HIP_TRY(hipGetLastError());
  }
  return SG_OK;
}

}  // namespace sg
