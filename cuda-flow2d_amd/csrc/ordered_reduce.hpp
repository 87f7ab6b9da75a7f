// The deterministic reduction of flow_error.hip: no atomics, every addition in an order that depends only on the grid.  Two
// launches: every workgroup of the partials kernel reduces its lanes' accumulators into one slab of the workspace
// (workgroup_reduce), and one workgroup per instance sums the slabs -- thread t takes slabs t, t + 256, ... in order with the
// accumulator's combine() -- and reduces those sums the same way.
//
// An accumulator type supplies two members, each field named once in each:
//   combine(q)      adds (or fmaxf's) every field of q into this one, field by field;
//   across_lanes()  replaces every field by its wave_sum / wave_max.
//
// global_motion.hip uses wave_sum from here but keeps its own spelled-out form of the same steps in motion_partials_kernel
// and motion_final_kernel: with workgroup_reduce the two compiled to a different instruction stream (the waves' read-back
// from LDS) and, timed against the parent at 4096 x 4096, missed "no slower than the parent by more than the parent's own
// spread" in three of seven forms (profiles/shared_headers/README.md).  Their local form compiles to the parent's stream.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

// Lane butterfly, offsets 32, 16, ..., 1: every lane ends with the same bits (IEEE addition and fmaxf commute).
template <typename T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ float wave_max(float x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}

// Reduces the accumulators of a workgroup of `Waves` waves: across the lanes of each wave by the butterfly, then across the
// waves through LDS in wave order 1, 2, ...  True for the one thread (lane 0 of wave 0) whose `acc` then holds the total.
// Every thread of the workgroup must reach the call (it holds a barrier), and a kernel calls it once: a second call would
// need a barrier of its own before the LDS array is written again.
template <int Waves, typename Acc>
__device__ __forceinline__ bool workgroup_reduce(Acc& acc, unsigned lane, unsigned wave)
{
    static_assert(std::is_trivially_copyable<Acc>::value && std::is_trivially_default_constructible<Acc>::value,
                  "the accumulator is copied through LDS as plain bytes");
    __shared__ Acc waves[Waves];
    acc.across_lanes();
    if (lane == 0) waves[wave] = acc;
    __syncthreads();
    if (lane != 0 || wave != 0) return false;
    acc = waves[0];
    for (int wv = 1; wv < Waves; ++wv) acc.combine(waves[wv]);
    return true;
}
