// Point-to-plane registration of a point set onto a surface (semigcn_amd/align.py, "The rule": the specification;
// tests/align_oracle.py: its numpy restatement).  Two kernels; the iteration itself is driven by the host, which reads 40
// doubles per iteration and solves a 6 x 6 or 7 x 7 system.
//
// Transform (sg_align_transform): one lane per point, x = M p + t in float64, rounded to float32 once; equal to the oracle
// bit for bit.  A lane reads its own row before it writes it, so the output may be the input.
//
// Normal equations (sg_align_accumulate): one lane per row computes x again (not rounded), the unit normal of the face
// the closest point lies on, the residual r and the seven entries of J, and adds the 28 + 7 + 2 sums and the 3 counts into
// 40 float64 accumulators of its own (hipcc keeps them, the row's temporaries and the tree in 256 VGPRs: no scratch, two
// waves per SIMD).  The runs of the blocks are those of sg_distance_stats (mesh_common.h: chunk_for, blocks_of), so up to
// 2^18 rows a lane sees one row and what a block costs is its tree, not its arithmetic.  The tree:
// each of the 40 values goes down a shuffle tree inside its wave (offsets 32 .. 1; 240 float64 shuffles a wave, no LDS
// array and no barrier), lane 0 of each of the four waves writes its 40 values to 1280 bytes of LDS, and after the block's
// one barrier lane k < 40 adds the four in wave order and writes the block's partial.  sg_distance_stats' own tree
// (s[K][256] in LDS, eight barriers) would take 80 KiB of LDS at K = 40.  A second launch of 40 lanes adds the block partials, lane
// k its column in block order.  No floating-point atomics: two runs give the same bits.
//
// Built with -ffp-contract=off: x, the cross product of the normal, nn, r, J and every term J_j J_k, J_j r, r r, d d are
// DEFINED as plain float64 multiplies and adds in the written order.
#include <cmath>

#include "mesh_common.h"

namespace sg {
namespace {

constexpr int kNoFace = 0x7fffffff;
constexpr int kAcc = 40;          // A upper triangle 28, g 7, sum r^2, sum d^2, rows used / rejected as far / skipped
constexpr int kWaves = kThreads / 64;

struct Pose {
  double m[9], t[3];
};

__device__ __forceinline__ void transform(const Pose& P, const float* __restrict__ p, double (&x)[3]) {
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) x[r] = ((P.m[3 * r] * px + P.m[3 * r + 1] * py) + P.m[3 * r + 2] * pz) + P.t[r];
}

__global__ void transform_rows(const float* pts, int64_t N, Pose P, float* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double x[3];
  transform(P, pts + 3 * i, x);
  out[3 * i] = (float)x[0];
  out[3 * i + 1] = (float)x[1];
  out[3 * i + 2] = (float)x[2];
}

__global__ void __launch_bounds__(kThreads)
align_partial(const float* __restrict__ vs, const int64_t* __restrict__ faces, const float* __restrict__ pts, int64_t N,
              int64_t chunk, Pose P, const float* __restrict__ closest, const int32_t* __restrict__ face,
              const float* __restrict__ dist, double max_dist, int with_scale, double* __restrict__ part) {
  double v[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) v[k] = 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = i0 + chunk < N ? i0 + chunk : N;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
    const int f = face[i];
    double x[3];
    transform(P, pts + 3 * i, x);
    if (f < 0 || f == kNoFace || !(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) {
      v[39] += 1.0;
      continue;
    }
    const float* a = vs + 3 * faces[3 * (int64_t)f];
    const float* b = vs + 3 * faces[3 * (int64_t)f + 1];
    const float* c = vs + 3 * faces[3 * (int64_t)f + 2];
    const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
    const double wx = (double)c[0] - (double)a[0], wy = (double)c[1] - (double)a[1], wz = (double)c[2] - (double)a[2];
    const double Nx = uy * wz - uz * wy, Ny = uz * wx - ux * wz, Nz = ux * wy - uy * wx;
    const double nn = (Nx * Nx + Ny * Ny) + Nz * Nz;
    if (nn == 0.0) {
      v[39] += 1.0;
      continue;
    }
    const double d = (double)dist[i];
    if (d > max_dist) {
      v[38] += 1.0;
      continue;
    }
    v[37] += 1.0;
    const double len = sqrt(nn);
    const double nx = Nx / len, ny = Ny / len, nz = Nz / len;
    const double ex = x[0] - (double)closest[3 * i], ey = x[1] - (double)closest[3 * i + 1], ez = x[2] - (double)closest[3 * i + 2];
    const double r = (nx * ex + ny * ey) + nz * ez;
    double J[7];
    J[0] = x[1] * nz - x[2] * ny;
    J[1] = x[2] * nx - x[0] * nz;
    J[2] = x[0] * ny - x[1] * nx;
    J[3] = nx;
    J[4] = ny;
    J[5] = nz;
    J[6] = with_scale ? (nx * x[0] + ny * x[1]) + nz * x[2] : 0.0;
    int q = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
      for (int k = j; k < 7; ++k) v[q++] += J[j] * J[k];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[28 + j] += J[j] * r;
    v[35] += r * r;
    v[36] += d * d;
  }
  __shared__ double s[kWaves][kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) {
    double t = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    v[k] = t;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) s[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < kAcc) {
    double t = s[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) t += s[w][threadIdx.x];
    part[kAcc * (int64_t)blockIdx.x + threadIdx.x] = t;
  }
}

// lane k adds column k of the block partials in block order
__global__ void align_finish(const double* __restrict__ part, int nb, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (blockIdx.x != 0 || k >= kAcc) return;
  double t = 0.0;
#pragma unroll 8
  for (int b = 0; b < nb; ++b) t += part[kAcc * b + k];
  out[k] = t;
}

Pose pose_of(const double* pose) {
  Pose P;
  for (int k = 0; k < 9; ++k) P.m[k] = pose[k];
  for (int k = 0; k < 3; ++k) P.t[k] = pose[9 + k];
  return P;
}

}  // namespace

int align_transform(const float* pts, int64_t N, const double* pose, float* out, hipStream_t stream) {
  transform_rows<<<blocks_for(N), kThreads, 0, stream>>>(pts, N, pose_of(pose), out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

int align_accumulate(const float* vs, const int64_t* faces, const float* pts, int64_t N, const double* pose, const float* closest,
                     const int32_t* face, const float* dist, double max_dist, int with_scale, double* partial, double* out,
                     hipStream_t stream) {
  const int nb = blocks_of(N);
  align_partial<<<nb, kThreads, 0, stream>>>(vs, faces, pts, N, chunk_for(N, nb), pose_of(pose), closest, face, dist, max_dist,
                                             with_scale, partial);
  align_finish<<<1, 64, 0, stream>>>(partial, nb, out);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

}  // namespace sg
