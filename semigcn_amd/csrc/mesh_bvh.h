// The surface hierarchy as its traversals see it: what mesh_dist.hip (build, closest-point query), mesh_isect.hip
// (self-overlap query) and mesh_ray.hip (first-hit query) need to know about an sg_surface and the layout of its nodes.  Nothing else is shared.
#pragma once
#include "mesh_common.h"

struct sg_surface {
  int64_t V = 0, F = 0, L = 0;   // vertices, faces, leaves
  sg::DeviceBuf<float4> tri;     // [3F] in leaf order: (a, face id bits), (b - a, 0), (c - a, 0)
  sg::DeviceBuf<float4> nodes;   // [max(L - 1, 1)][4]: child 0 lo (w: child code), hi, child 1 lo (w: code), hi
  sg::DeviceBuf<float> bounds;   // [6] box of the face centroids (the query points' Morton frame)
};

namespace sg {
namespace {

constexpr int kLeaf = 4;          // faces per leaf
constexpr int kStack = 64;        // a Karras tree over 64-bit keys is at most 64 internal levels deep

// Child codes: >= 0 internal node, < 0 leaf ~code.
__device__ __forceinline__ float code_bits(int c) { return __int_as_float(c); }

}  // namespace
}  // namespace sg
