// What flow2d_node_strain_2d (node_strain.hip) and flow2d_node_strain_robust_2d (node_strain_robust.hip) share: the geometry of
// the strain window's tile, the reasons a node has no strain, the accumulator behind their record, the nine quantities from the
// four gradients and the exponents of the basis.  The definitions they restate are those of flow2d_c_abi.h.
//
// Everything lies in an unnamed namespace, as it did in node_strain.hip: the kernels of either file are internal to it, and
// node_strain.hip's keep the names and the device code they had (profiles/robust_strain/README.md).
#pragma once

#include <cmath>

#include "node_grid.hpp"
#include "plane_sample.hpp"
#include "strain_sums.hpp"

namespace {

constexpr int kMaxWindow = FLOW2D_NODE_STRAIN_MAX_WINDOW;
constexpr int kTileW = flow2d::kPixelBlockX + 2 * kMaxWindow;  // 78
constexpr int kTileH = flow2d::kPixelBlockY + 2 * kMaxWindow;  // 18
constexpr int kThreads = flow2d::kPixelBlockX * flow2d::kPixelBlockY;
constexpr int kReasons = 3;     // centre, sparse, degenerate: reserved[0 .. 2] of the record

enum Reason { kValid = -1, kCentre = 0, kSparse = 1, kDegenerate = 2 };

// StrainSums with the counts of the three reasons a node has no strain.
struct NodeStrainSums : StrainSums {
    unsigned long long reasons[kReasons];
    unsigned long long pad;

    __device__ __forceinline__ void clear()
    {
        StrainSums::clear();
        pad = 0;
#pragma unroll
        for (int k = 0; k < kReasons; ++k) reasons[k] = 0;
    }
    __device__ __forceinline__ void combine(const NodeStrainSums& q)
    {
        StrainSums::combine(q);
#pragma unroll
        for (int k = 0; k < kReasons; ++k) reasons[k] += q.reasons[k];
    }
    __device__ __forceinline__ void across_lanes()
    {
        StrainSums::across_lanes();
#pragma unroll
        for (int k = 0; k < kReasons; ++k) reasons[k] = wave_sum(reasons[k]);
    }
    __device__ __forceinline__ void fill(flow2d_deformation_stats& rec) const
    {
        StrainSums::fill(rec);
        for (int k = 0; k < kReasons; ++k) rec.reserved[k] = reasons[k];
    }
};
static_assert(sizeof(NodeStrainSums) == 192, "flow2d_node_strain_workspace_bytes counts slabs of 192 bytes");

// The nine quantities of the header from the gradients, each cast to float once.
__device__ __forceinline__ void quantities(double a, double b, double c, double d, int measure, float (&q)[9])
{
    double exx = a, eyy = d, exy = 0.5 * (b + c);
    if (measure == FLOW2D_STRAIN_GREEN_LAGRANGE) {
        exx = a + 0.5 * (a * a + c * c);
        eyy = d + 0.5 * (b * b + d * d);
        exy = 0.5 * ((b + c) + (a * b + c * d));
    }
    const double mean = 0.5 * (exx + eyy), half = 0.5 * (exx - eyy);
    const double shear = sqrt(half * half + exy * exy);
    q[0] = static_cast<float>(a + d);
    q[1] = static_cast<float>(c - b);
    q[2] = static_cast<float>((a + d) + (a * d - b * c));
    q[3] = static_cast<float>(exx);
    q[4] = static_cast<float>(eyy);
    q[5] = static_cast<float>(exy);
    q[6] = static_cast<float>(mean + shear);
    q[7] = static_cast<float>(mean - shear);
    q[8] = static_cast<float>(shear);
}

// phi_a over the offset (di, dj) as the exponents of di and dj: 1, di, dj, di*di, di*dj, dj*dj
constexpr int exp_i(int a) { return a == 1 || a == 4 ? 1 : a == 3 ? 2 : 0; }
constexpr int exp_j(int a) { return a == 2 || a == 4 ? 1 : a == 5 ? 2 : 0; }

// The workgroups of an nw x nh grid: one slab of partial sums each.
inline size_t partial_blocks(size_t nw, size_t nh)
{
    return static_cast<size_t>(flow2d::div_up(nw, flow2d::kPixelBlockX)) * flow2d::div_up(nh, flow2d::kPixelBlockY);
}

}  // namespace
