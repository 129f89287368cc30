// First hit of a ray on a surface: the third basic query of the surface hierarchy, after the closest point (mesh_dist.hip)
// and the self-overlap (mesh_isect.hip), and the small renderer that rests on it (what the reference shows through
// util/render.py:19-45 and the coloured mask mesh of util/datamaker.py:161-171).  The predicate -- when a face is hit, at
// which t, which hit wins -- is specified in semigcn_amd/render.py ("The rule"); tests/ray_oracle.py restates it in numpy.
//
// The walk is a first-hit traversal of an existing sg_surface (mesh_dist.hip builds it; nothing of the build changes).  One
// lane per ray, one wavefront per workgroup.  A lane computes the slab interval [tn, tf] of its ray in the two child boxes of
// a node -- the SAME function of (lo, hi) that clause 4 of the rule applies to a face's own box, so the interval of a node
// contains the interval of every face below it and the walk needs no margin of its own -- drops a child iff tn > tf,
// tf < t_min or tn > min(t_max, best t) (closed: ties survive), descends the child with the smaller tn first and keeps the
// other on a stack in LDS, as surface_query does.  At a leaf the up to kLeaf faces are tested with the predicate, which reads
// the ORIGINAL vs / faces rows -- never tri[], whose b - a and c - a are rounded -- and evaluates everything in float64
// without fused multiply-adds (the Makefile builds this file with -ffp-contract=off).  A ray's row depends on the ray and
// the set of faces only: the best hit is the smallest float64 t, the lowest face id among equals, whatever order the faces
// came in.  Two runs give identical bytes; the only atomics are the two integer counters of stats.
//
//   sg_surface_raycast  arbitrary rays, sorted first by (direction octant, 10-bit Morton code of the origin in the surface's
//                       bounds, ray index) so that a wavefront walks one region of the tree; the rows do not depend on it.
//   sg_surface_render   primary rays of a camera, generated in the kernel: one lane per pixel, an 8 x 8 pixel tile per
//                       wavefront, no ray array.
//   sg_shade_hits       face / bary (+ the ray directions or the camera) -> uint8 RGB: two-sided flat head-light shading
//                       of a constant, a per-face or an interpolated per-vertex scalar colour.
//
// Bound: the latency of the dependent node loads, like the other two walks; no rate has been measured against a model.
// Per node: 64 bytes (two child boxes and codes, four float4).  Per candidate face: 4 bytes of tri[] (the id), 24 bytes of
// faces, 36 bytes of vs; the float64 arithmetic (three 3 x 3 determinants, one division, the slab of the face's own box)
// runs on the faces of the leaves the ray's interval reaches.  The 16 KiB stack of a one-wavefront workgroup caps a compute
// unit at 10 wavefronts (160 KiB of LDS) where the registers would allow more; for a walk that waits on dependent loads the
// number of wavefronts in flight is what hides the wait, so this cap is the first thing to look at.  Its cost was not
// measured, and a smaller stack was not tried.
#include "mesh_bvh.h"   // struct sg_surface, kLeaf, kStack, the child codes; mesh_common.h

namespace sg {
namespace {

constexpr int kRayThreads = 64;    // one wavefront per workgroup: its stack is 64 x 64 int32 = 16 KiB of LDS
constexpr int kTile = 8;           // the render kernel's wavefront covers kTile x kTile pixels
constexpr int kNoFace = 0x7fffffff;

struct D3 {
  double x, y, z;
};
struct Camera {                    // sg_surface_render's cam: eye, right, up, forward, tan half-angles (or half extents)
  D3 e, r, u, w;
  double tx, ty;
  int ortho;
};
struct Ray {
  D3 o, d, inv;                    // inv_k = 1.0 / d_k where d_k != 0
  bool ok;                         // finite, d != 0
};
struct Best {
  double t = INFINITY;
  int face = kNoFace;
  float b1 = 0.f, b2 = 0.f;
};

__device__ __forceinline__ D3 sub(const D3& a, const D3& b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// det of the rows u, v, w -- this order of operations is part of the specification (mesh_isect.hip's det3)
__device__ __forceinline__ double det3(const D3& u, const D3& v, const D3& w) {
  return u.x * (v.y * w.z - v.z * w.y) + u.y * (v.z * w.x - v.x * w.z) + u.z * (v.x * w.y - v.y * w.x);
}
__device__ __forceinline__ double dot3(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross_edges(const D3& a, const D3& b, const D3& c) {   // normal_of: (b - a) x (c - a)
  const D3 e1 = sub(b, a), e2 = sub(c, a);
  return D3{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
}

__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
  Ray r;
  r.o = D3{(double)ox, (double)oy, (double)oz};
  r.d = D3{(double)dx, (double)dy, (double)dz};
  r.inv = D3{dx != 0.f ? 1.0 / r.d.x : 0.0, dy != 0.f ? 1.0 / r.d.y : 0.0, dz != 0.f ? 1.0 / r.d.z : 0.0};
  r.ok = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) &&
         (dx != 0.f || dy != 0.f || dz != 0.f);
  return r;
}

// one axis of clause 4; false: d_k == 0 and the origin is outside [lo, hi] (0 * inf is never formed)
__device__ __forceinline__ bool slab_axis(float lo, float hi, double o, double d, double inv, double& tn, double& tf) {
  if (d == 0.0) return (double)lo <= o && o <= (double)hi;
  const double t1 = ((double)lo - o) * inv, t2 = ((double)hi - o) * inv;
  tn = fmax(tn, fmin(t1, t2));
  tf = fmin(tf, fmax(t1, t2));
  return true;
}

// Clause 4 of the rule on the box [lo, hi]: the widened slab interval.  Every step is monotone in lo / hi under rounding.
__device__ __forceinline__ bool slab(float lx, float ly, float lz, float hx, float hy, float hz, const Ray& r, double& tn,
                                     double& tf) {
  tn = -INFINITY;
  tf = INFINITY;
  if (!slab_axis(lx, hx, r.o.x, r.d.x, r.inv.x, tn, tf)) return false;
  if (!slab_axis(ly, hy, r.o.y, r.d.y, r.inv.y, tn, tf)) return false;
  if (!slab_axis(lz, hz, r.o.z, r.d.z, r.inv.z, tn, tf)) return false;
  tn *= tn > 0.0 ? 1.0 - 0x1p-30 : 1.0 + 0x1p-30;
  tf *= tf > 0.0 ? 1.0 + 0x1p-30 : 1.0 - 0x1p-30;
  return true;
}

// The predicate of semigcn_amd/render.py for face f, clause by clause; a face with an id outside [0, V) (the surface was
// built from other faces) is hit by nothing, and nothing is read through the id.
__device__ __forceinline__ void test_face(const float* __restrict__ vs, const int64_t* __restrict__ faces, int64_t V, int f,
                                          const Ray& r, double t_min, double t_max, Best& best) {
  const int64_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return;
  if (ia == ib || ib == ic || ic == ia) return;                                  // 1
  const float* pa = vs + 3 * ia;
  const float* pb = vs + 3 * ib;
  const float* pc = vs + 3 * ic;
  const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
  const D3 A{(double)ax, (double)ay, (double)az}, B{(double)bx, (double)by, (double)bz}, C{(double)cx, (double)cy, (double)cz};
  const D3 n = cross_edges(A, B, C);
  if (n.x == 0.0 && n.y == 0.0 && n.z == 0.0) return;
  const D3 a = sub(A, r.o), b = sub(B, r.o), c = sub(C, r.o);                    // 2
  const double U = det3(r.d, b, c), Vv = det3(r.d, c, a), W = det3(r.d, a, b);
  const double Sb = (U + Vv) + W;
  if (Sb == 0.0) return;
  if (!((U >= 0.0 && Vv >= 0.0 && W >= 0.0) || (U <= 0.0 && Vv <= 0.0 && W <= 0.0))) return;
  const double den = dot3(r.d, n);                                               // 3
  if (den == 0.0) return;
  const double t = dot3(a, n) / den;
  double tn, tf;                                                                 // 4
  if (!slab(fminf(ax, fminf(bx, cx)), fminf(ay, fminf(by, cy)), fminf(az, fminf(bz, cz)), fmaxf(ax, fmaxf(bx, cx)),
            fmaxf(ay, fmaxf(by, cy)), fmaxf(az, fmaxf(bz, cz)), r, tn, tf))
    return;
  if (!(tn <= t && t <= tf)) return;
  if (!(t_min <= t && t <= t_max)) return;                                       // 5
  if (t < best.t || (t == best.t && f < best.face)) {     // the smallest t, the lowest id among equals: no order matters
    best.t = t;
    best.face = f;
    best.b1 = (float)(Vv / Sb);
    best.b2 = (float)(W / Sb);
  }
}

// may the subtree in the box (lo, hi) hold a hit that beats or ties `best`?  *tn: where the ray enters the box
__device__ __forceinline__ bool box_reached(const float4& lo, const float4& hi, const Ray& r, double t_min, double t_max,
                                            const Best& best, double* tn_out) {
  if (lo.x > hi.x) return false;     // the empty second child of a lone leaf: inverted infinite, a slab test would pass it
  double tn, tf;
  if (!slab(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, r, tn, tf)) return false;
  *tn_out = tn;
  return !(tn > tf || tf < t_min || tn > fmin(t_max, best.t));
}

// The walk of one lane.  Returns the leaves visited; *dropped counts subtrees lost to a full stack (cannot happen: depth
// first, at most one pending sibling per level, and the tree is at most kStack levels deep).
__device__ __forceinline__ int walk(const float4* __restrict__ nodes, const float4* __restrict__ tri, int64_t F, int64_t V,
                                    const float* __restrict__ vs, const int64_t* __restrict__ faces, const Ray& r, double t_min,
                                    double t_max, int (*stack)[kRayThreads], int lane, Best& best, int* dropped) {
  int visits = 0;
  int cur = 0, sp = 0;
  while (true) {
    const float4* nd = nodes + 4 * (int64_t)cur;
    const float4 lo0 = nd[0], hi0 = nd[1], lo1 = nd[2], hi1 = nd[3];
    const int c0 = __float_as_int(lo0.w), c1 = __float_as_int(lo1.w);
    double tn0 = 0.0, tn1 = 0.0;
    bool go0 = box_reached(lo0, hi0, r, t_min, t_max, best, &tn0);
    bool go1 = box_reached(lo1, hi1, r, t_min, t_max, best, &tn1);
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {                 // leaves: tested on the spot, the later one against the new best
      const int c = side == 0 ? c0 : c1;
      const bool go = side == 0 ? go0 : go1;
      const double tn = side == 0 ? tn0 : tn1;
      if (c >= 0 || !go || tn > fmin(t_max, best.t)) continue;
      ++visits;
      const int64_t k0 = (int64_t)(~c) * kLeaf;
      const int64_t k1 = k0 + kLeaf < F ? k0 + kLeaf : F;  // the last leaf holds fewer than kLeaf faces
      for (int64_t k = k0; k < k1; ++k) {
        const int g = __float_as_int(tri[3 * k].w);
        if (g < 0 || g >= F) continue;
        test_face(vs, faces, V, g, r, t_min, t_max, best);
      }
    }
    go0 = go0 && c0 >= 0 && !(tn0 > fmin(t_max, best.t));
    go1 = go1 && c1 >= 0 && !(tn1 > fmin(t_max, best.t));
    if (go0 && go1) {
      const bool first0 = tn0 <= tn1;                      // nearer child first
      if (sp < kStack) stack[sp++][lane] = first0 ? c1 : c0;
      else ++*dropped;
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
  return visits;
}

// a ray's row; a miss, a non-finite ray and d = 0 give (inf, no face, nan): the "no face" convention of sg_surface_query
__device__ __forceinline__ void store_row(int64_t i, const Best& best, float* __restrict__ t, int32_t* __restrict__ face,
                                          float* __restrict__ bary) {
  const bool hit = best.face != kNoFace;
  t[i] = hit ? (float)best.t : INFINITY;
  face[i] = best.face;
  if (bary) {
    bary[2 * i] = hit ? best.b1 : __int_as_float(0x7fc00000);
    bary[2 * i + 1] = hit ? best.b2 : __int_as_float(0x7fc00000);
  }
}

// stats[0] += dropped subtrees, stats[1] += leaf visits: one integer atomic per wavefront (all 64 lanes are here)
__device__ __forceinline__ void add_stats(int dropped, int visits, unsigned long long* __restrict__ stats) {
  unsigned long long v = (unsigned long long)visits, d = (unsigned long long)dropped;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v += __shfl_down(v, off, 64);
    d += __shfl_down(d, off, 64);
  }
  if (threadIdx.x == 0) {
    if (v) atomicAdd(stats + 1, v);
    if (d) atomicAdd(stats, d);
  }
}

__device__ __forceinline__ uint32_t spread10(uint32_t x) {   // 10 bits -> every third bit of 30
  x &= 0x3ffu;
  x = (x | x << 16) & 0x030000ffu;
  x = (x | x << 8) & 0x0300f00fu;
  x = (x | x << 4) & 0x030c30c3u;
  x = (x | x << 2) & 0x09249249u;
  return x;
}

// (direction octant, Morton code of the origin in the surface's bounds, ray index): 3 + 30 + 31 bits
__global__ void ray_keys(const float* __restrict__ origins, const float* __restrict__ dirs, int64_t N,
                         const float* __restrict__ bounds, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  uint64_t key = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ext = bounds[3 + k] - bounds[k];
    float t = ext > 0.f ? (origins[3 * i + k] - bounds[k]) / ext : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f) * 1024.f;               // origins outside the box clamp to its faces (NaN -> 0)
    key |= (uint64_t)spread10(min((uint32_t)t, 1023u)) << (2 - k);
    key |= (uint64_t)(dirs[3 * i + k] < 0.f ? 1 : 0) << (30 + k);
  }
  keys[i] = key << 31 | (uint64_t)i;
}

__global__ __launch_bounds__(kRayThreads) void ray_cast(const float4* __restrict__ nodes, const float4* __restrict__ tri,
                                                        int64_t F, int64_t V, const float* __restrict__ vs,
                                                        const int64_t* __restrict__ faces, const uint64_t* __restrict__ order,
                                                        int64_t N, const float* __restrict__ origins,
                                                        const float* __restrict__ dirs, double t_min, double t_max,
                                                        float* __restrict__ t_out, int32_t* __restrict__ face_out,
                                                        float* __restrict__ bary_out, unsigned long long* __restrict__ stats) {
  __shared__ int stack[kStack][kRayThreads];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kRayThreads + lane;
  int visits = 0, dropped = 0;
  if (p < N) {
    const int64_t i = (int64_t)(order[p] & 0x7fffffffull);
    const Ray r = make_ray(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    Best best;
    if (r.ok) visits = walk(nodes, tri, F, V, vs, faces, r, t_min, t_max, stack, lane, best, &dropped);
    store_row(i, best, t_out, face_out, bary_out);
  }
  add_stats(dropped, visits, stats);
}

// The primary ray of pixel (x, y), component by component in the written order (semigcn_amd/render.py, "Camera rays").
__device__ __forceinline__ Ray pixel_ray(const Camera& cam, int x, int y, int width, int height) {
  const double sx = ((2.0 * ((double)x + 0.5)) / (double)width - 1.0) * cam.tx;
  const double sy = (1.0 - (2.0 * ((double)y + 0.5)) / (double)height) * cam.ty;
  if (cam.ortho)
    return make_ray((float)((cam.e.x + sx * cam.r.x) + sy * cam.u.x), (float)((cam.e.y + sx * cam.r.y) + sy * cam.u.y),
                    (float)((cam.e.z + sx * cam.r.z) + sy * cam.u.z), (float)cam.w.x, (float)cam.w.y, (float)cam.w.z);
  return make_ray((float)cam.e.x, (float)cam.e.y, (float)cam.e.z, (float)((cam.w.x + sx * cam.r.x) + sy * cam.u.x),
                  (float)((cam.w.y + sx * cam.r.y) + sy * cam.u.y), (float)((cam.w.z + sx * cam.r.z) + sy * cam.u.z));
}

__global__ __launch_bounds__(kRayThreads) void ray_render(const float4* __restrict__ nodes, const float4* __restrict__ tri,
                                                          int64_t F, int64_t V, const float* __restrict__ vs,
                                                          const int64_t* __restrict__ faces, Camera cam, int width, int height,
                                                          int tiles_x, double t_min, double t_max, float* __restrict__ t_out,
                                                          int32_t* __restrict__ face_out, float* __restrict__ bary_out,
                                                          unsigned long long* __restrict__ stats) {
  __shared__ int stack[kStack][kRayThreads];
  const int lane = threadIdx.x;
  const int x = (int)(blockIdx.x % (unsigned)tiles_x) * kTile + (lane & (kTile - 1));
  const int y = (int)(blockIdx.x / (unsigned)tiles_x) * kTile + lane / kTile;
  int visits = 0, dropped = 0;
  if (x < width && y < height) {
    const Ray r = pixel_ray(cam, x, y, width, height);
    Best best;
    if (r.ok) visits = walk(nodes, tri, F, V, vs, faces, r, t_min, t_max, stack, lane, best, &dropped);
    store_row((int64_t)y * width + x, best, t_out, face_out, bary_out);
  }
  add_stats(dropped, visits, stats);
}

struct ShadeArgs {
  int mode;                        // SG_SHADE_*
  uint32_t color, background;      // 0xRRGGBB
  const uint8_t* face_colors;      // [F, 3], mode SG_SHADE_FACE
  const float* scalars;            // [V], mode SG_SHADE_SCALAR
  double vmin, vmax, ambient;
};

// colour level in [0, 255] of channel ch for x in [0, 1]: the five stops blue, cyan, green, yellow, red at 0, 1/4 .. 1
__device__ __forceinline__ double ramp(double x, int ch) {
  const double u = x * 4.0;
  int k = (int)u;
  if (k > 3) k = 3;
  const double f = u - (double)k;
  // channel values at the stops k and k + 1: r = 0 0 0 1 1, g = 0 1 1 1 0, b = 1 1 0 0 0
  const int lo = ch == 0 ? (k >= 3) : (ch == 1 ? (k >= 1) : (k <= 1));
  const int hi = ch == 0 ? (k >= 2) : (ch == 1 ? (k <= 2) : (k <= 0));
  return 255.0 * ((double)lo + f * (double)(hi - lo));
}

__global__ void shade(const float* __restrict__ vs, const int64_t* __restrict__ faces, int64_t F, int64_t V,
                      const int32_t* __restrict__ face, const float* __restrict__ bary, const float* __restrict__ dirs, Camera cam,
                      int width, int height, int64_t n, ShadeArgs a, uint8_t* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double level[3] = {(double)(a.background >> 16 & 255u), (double)(a.background >> 8 & 255u), (double)(a.background & 255u)};
  const int f = face[i];
  int64_t ia = -1, ib = -1, ic = -1;
  if (f >= 0 && f < F) {
    ia = faces[3 * (int64_t)f];
    ib = faces[3 * (int64_t)f + 1];
    ic = faces[3 * (int64_t)f + 2];
  }
  if (ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V) {
    D3 d;
    if (dirs) {
      d = D3{(double)dirs[3 * i], (double)dirs[3 * i + 1], (double)dirs[3 * i + 2]};
    } else {
      const Ray r = pixel_ray(cam, (int)(i % width), (int)(i / width), width, height);
      d = r.d;
    }
    const D3 A{(double)vs[3 * ia], (double)vs[3 * ia + 1], (double)vs[3 * ia + 2]};
    const D3 B{(double)vs[3 * ib], (double)vs[3 * ib + 1], (double)vs[3 * ib + 2]};
    const D3 C{(double)vs[3 * ic], (double)vs[3 * ic + 1], (double)vs[3 * ic + 2]};
    const D3 nrm = cross_edges(A, B, C);
    const double len2 = dot3(d, d) * dot3(nrm, nrm);
    double intensity = a.ambient;
    if (len2 > 0.0) intensity = a.ambient + ((1.0 - a.ambient) * fabs(dot3(d, nrm))) / sqrt(len2);
    if (a.mode == SG_SHADE_FACE) {
      for (int ch = 0; ch < 3; ++ch) level[ch] = (double)a.face_colors[3 * (int64_t)f + ch];
    } else if (a.mode == SG_SHADE_SCALAR) {
      const double b1 = (double)bary[2 * i], b2 = (double)bary[2 * i + 1];
      const double s = (((1.0 - b1) - b2) * (double)a.scalars[ia] + b1 * (double)a.scalars[ib]) + b2 * (double)a.scalars[ic];
      double x = a.vmax > a.vmin ? (s - a.vmin) / (a.vmax - a.vmin) : 0.0;
      x = !(x > 0.0) ? 0.0 : (x > 1.0 ? 1.0 : x);          // a NaN scalar takes the first stop
      for (int ch = 0; ch < 3; ++ch) level[ch] = ramp(x, ch);
    } else {
      level[0] = (double)(a.color >> 16 & 255u);
      level[1] = (double)(a.color >> 8 & 255u);
      level[2] = (double)(a.color & 255u);
    }
    for (int ch = 0; ch < 3; ++ch) level[ch] = floor(level[ch] * intensity + 0.5);
  }
  for (int ch = 0; ch < 3; ++ch) rgb[3 * i + ch] = (uint8_t)(level[ch] < 0.0 ? 0.0 : (level[ch] > 255.0 ? 255.0 : level[ch]));
}

Camera camera_of(const double* cam, int ortho) {
  Camera c;
  c.e = D3{cam[0], cam[1], cam[2]};
  c.r = D3{cam[3], cam[4], cam[5]};
  c.u = D3{cam[6], cam[7], cam[8]};
  c.w = D3{cam[9], cam[10], cam[11]};
  c.tx = cam[12];
  c.ty = cam[13];
  c.ortho = ortho != 0;
  return c;
}

// what the two walks check before anything touches the device, sizes first: as sg_surface_self_pairs checks n_pairs
int check_walk(const char* who, const sg_surface* s, const float* vs, const int64_t* faces, int64_t F, double t_min,
               double t_max) {
  SG_REQUIRE(F >= 0, "%s: negative F", who);
  SG_REQUIRE(t_min <= t_max, "%s: t_min = %g > t_max = %g (or a NaN)", who, t_min, t_max);
  SG_REQUIRE(vs && faces, "%s: null pointer", who);
  SG_REQUIRE(s != nullptr, "%s: null surface", who);
  SG_REQUIRE(s->F == F, "%s: the surface was built from %lld faces, not %lld", who, (long long)s->F, (long long)F);
  return SG_OK;
}

}  // namespace
}  // namespace sg

using namespace sg;

SG_API int sg_surface_raycast(const sg_surface* s, const float* vs, const int64_t* faces, int64_t F, const float* origins,
                              const float* dirs, int64_t N, double t_min, double t_max, float* t, int32_t* face, float* bary,
                              int64_t* stats_dev, void* stream_) {
  SG_REQUIRE(N >= 0, "sg_surface_raycast: negative N");
  SG_REQUIRE(N < ((int64_t)1 << 31), "sg_surface_raycast: N = %lld does not fit int32", (long long)N);
  if (int rc = check_walk("sg_surface_raycast", s, vs, faces, F, t_min, t_max)) return rc;
  if (N == 0) return SG_OK;
  SG_REQUIRE(origins && dirs && t && face && stats_dev, "sg_surface_raycast: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  AsyncBuf<uint64_t> keys_a(stream), keys_b(stream);
  AsyncBuf<char> temp(stream);
  SG_HIP_TRY(hipMemsetAsync(stats_dev, 0, 2 * sizeof(int64_t), stream));
  SG_HIP_TRY(keys_a.alloc(N));
  SG_HIP_TRY(keys_b.alloc(N));
  ray_keys<<<blocks_for(N), kThreads, 0, stream>>>(origins, dirs, N, s->bounds.p, keys_a.p);
  SG_HIP_TRY(hipGetLastError());
  size_t tb = 0;
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys_a.p, keys_b.p, (int)N, 0, 64, stream));
  SG_HIP_TRY(temp.alloc(tb));
  SG_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(temp.p, tb, keys_a.p, keys_b.p, (int)N, 0, 64, stream));
  const int64_t nb = (N + kRayThreads - 1) / kRayThreads;
  ray_cast<<<(unsigned)nb, kRayThreads, 0, stream>>>(s->nodes.p, s->tri.p, s->F, s->V, vs, faces, keys_b.p, N, origins, dirs,
                                                     t_min, t_max, t, face, bary, (unsigned long long*)stats_dev);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

SG_API int sg_surface_render(const sg_surface* s, const float* vs, const int64_t* faces, int64_t F, const double* cam, int ortho,
                             int64_t width, int64_t height, double t_min, double t_max, int32_t* face, float* t, float* bary,
                             int64_t* stats_dev, void* stream_) {
  SG_REQUIRE(width >= 0 && height >= 0, "sg_surface_render: negative width or height");
  SG_REQUIRE(width < ((int64_t)1 << 24) && height < ((int64_t)1 << 24) && width * height < ((int64_t)1 << 31),
             "sg_surface_render: %lld x %lld pixels do not fit int32", (long long)width, (long long)height);
  if (int rc = check_walk("sg_surface_render", s, vs, faces, F, t_min, t_max)) return rc;
  if (width == 0 || height == 0) return SG_OK;
  SG_REQUIRE(cam && face && t && bary && stats_dev, "sg_surface_render: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
  SG_HIP_TRY(hipMemsetAsync(stats_dev, 0, 2 * sizeof(int64_t), stream));
  ray_render<<<(unsigned)(tiles_x * tiles_y), kRayThreads, 0, stream>>>(s->nodes.p, s->tri.p, s->F, s->V, vs, faces,
                                                                        camera_of(cam, ortho), (int)width, (int)height,
                                                                        (int)tiles_x, t_min, t_max, t, face, bary,
                                                                        (unsigned long long*)stats_dev);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}

SG_API int sg_shade_hits(const float* vs, int64_t V, const int64_t* faces, int64_t F, const int32_t* face, const float* bary,
                         const float* dirs, const double* cam, int ortho, int64_t width, int64_t height, int64_t n, int mode,
                         uint32_t color, const uint8_t* face_colors, const float* scalars, double vmin, double vmax,
                         uint32_t background, double ambient, uint8_t* rgb, void* stream) {
  SG_REQUIRE(V >= 0 && F >= 0 && n >= 0, "sg_shade_hits: negative size");
  SG_REQUIRE(n < ((int64_t)1 << 31) && F < ((int64_t)1 << 31), "sg_shade_hits: n and F must fit int32");
  SG_REQUIRE(mode == SG_SHADE_CONSTANT || mode == SG_SHADE_FACE || mode == SG_SHADE_SCALAR, "sg_shade_hits: unknown mode %d",
             mode);
  SG_REQUIRE(ambient >= 0.0 && ambient <= 1.0, "sg_shade_hits: ambient = %g is outside [0, 1]", ambient);
  if (!dirs) {
    SG_REQUIRE(cam != nullptr, "sg_shade_hits: neither directions nor a camera");
    SG_REQUIRE(width >= 0 && height >= 0 && width < ((int64_t)1 << 24) && height < ((int64_t)1 << 24) && width * height == n,
               "sg_shade_hits: %lld x %lld pixels are not the %lld rows", (long long)width, (long long)height, (long long)n);
  }
  if (n == 0) return SG_OK;
  SG_REQUIRE(vs && faces && face && rgb, "sg_shade_hits: null pointer");
  SG_REQUIRE(mode != SG_SHADE_FACE || face_colors, "sg_shade_hits: null face_colors");
  SG_REQUIRE(mode != SG_SHADE_SCALAR || (scalars && bary), "sg_shade_hits: null scalars or bary");
  Camera c{};
  if (!dirs) c = camera_of(cam, ortho);
  ShadeArgs a{mode, color, background, face_colors, scalars, vmin, vmax, ambient};
  shade<<<blocks_for(n), kThreads, 0, (hipStream_t)stream>>>(vs, faces, F, V, face, bary, dirs, c, (int)width, (int)height, n, a,
                                                             rgb);
  SG_HIP_TRY(hipGetLastError());
  return SG_OK;
}
