// The statistics of flow2d_deformation_2d and flow2d_node_strain_2d: the accumulator behind a flow2d_deformation_stats record
// and the kernel that adds the workgroups' slabs (the two-launch ordered reduction of ordered_reduce.hpp).
//
// What is NOT here is the step that adds one pixel or node to the accumulator (sum += t; sum_sq += t * t; min; max; valid):
// it stays written out in deformation_kernel and node_strain_kernel.  As a member called from both, the statistics
// instantiations compiled to 2 - 22 % more instructions on the same registers (profiles/node_grid_headers/README.md).
#pragma once

#include <cmath>

#include "common.hpp"
#include "ordered_reduce.hpp"

constexpr int kStrainQuantities = 6;  // divergence, vorticity, dilatation, e1, e2, max_shear: the order of the record
constexpr int kStrainFinalThreads = 256;

struct StrainSums {
    double sum[kStrainQuantities], sum_sq[kStrainQuantities];
    float min[kStrainQuantities], max[kStrainQuantities];
    unsigned long long valid, invalid;

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < kStrainQuantities; ++k) {
            sum[k] = sum_sq[k] = 0.0;
            min[k] = INFINITY;
            max[k] = -INFINITY;
        }
        valid = invalid = 0;
    }
    __device__ __forceinline__ void combine(const StrainSums& q)
    {
#pragma unroll
        for (int k = 0; k < kStrainQuantities; ++k) {
            sum[k] += q.sum[k];
            sum_sq[k] += q.sum_sq[k];
            min[k] = q.min[k] < min[k] ? q.min[k] : min[k];
            max[k] = q.max[k] > max[k] ? q.max[k] : max[k];
        }
        valid += q.valid;
        invalid += q.invalid;
    }
    __device__ __forceinline__ void across_lanes()
    {
#pragma unroll
        for (int k = 0; k < kStrainQuantities; ++k) {
            sum[k] = wave_sum(sum[k]);
            sum_sq[k] = wave_sum(sum_sq[k]);
            // (no NaN ever enters min / max: x < min and x > max are false for one)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float a = __shfl_xor(min[k], o, 64), b = __shfl_xor(max[k], o, 64);
                min[k] = a < min[k] ? a : min[k];
                max[k] = b > max[k] ? b : max[k];
            }
        }
        valid = wave_sum(valid);
        invalid = wave_sum(invalid);
    }
    // The counts and the six moments of the record; min and max of nothing are 0.
    __device__ __forceinline__ void fill(flow2d_deformation_stats& rec) const
    {
        rec.valid = valid;
        rec.invalid = invalid;
        flow2d_deformation_moments* m[kStrainQuantities] = {&rec.divergence, &rec.vorticity, &rec.dilatation,
                                                            &rec.e1,         &rec.e2,        &rec.max_shear};
        for (int k = 0; k < kStrainQuantities; ++k) {
            m[k]->sum = sum[k];
            m[k]->sum_sq = sum_sq[k];
            m[k]->min = valid ? min[k] : 0.f;
            m[k]->max = valid ? max[k] : 0.f;
        }
    }
};
// (the workspace sizes of the two entries are multiples of these: 160 here, 192 with the reasons of node_strain.hip)
static_assert(sizeof(StrainSums) == 160, "flow2d_deformation_workspace_bytes counts slabs of 160 bytes");

// One workgroup per instance: thread t sums slabs t, t + 256, ... in order, then the reduction of ordered_reduce.hpp.
// Sums: StrainSums, or a type derived from it whose members of the same names take its further fields along.
template <typename Sums>
__global__ __launch_bounds__(kStrainFinalThreads) void strain_final_kernel(const Sums* __restrict__ partials, unsigned blocks,
                                                                           flow2d_deformation_stats* __restrict__ stats)
{
    const Sums* slab = partials + static_cast<size_t>(blockIdx.x) * blocks;
    Sums t;
    t.clear();
    for (unsigned j = threadIdx.x; j < blocks; j += kStrainFinalThreads) t.combine(slab[j]);
    if (!workgroup_reduce<kStrainFinalThreads / 64>(t, threadIdx.x % 64, threadIdx.x / 64)) return;
    flow2d_deformation_stats rec = {};
    t.fill(rec);
    stats[blockIdx.x] = rec;
}
