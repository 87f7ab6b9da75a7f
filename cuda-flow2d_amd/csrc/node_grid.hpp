// What the kernels on the node grid of a window correlation share (correlate.hip, correlate_offset.hip, subset_refine.hip,
// predict_nodes.hip, node_strain.hip; deformation.hip takes the NaN and the plane check): the small device helpers every one of
// them had a copy of, and the host-side checks of their entries.  The definitions they restate are those of flow2d_c_abi.h.
#pragma once

#include <cmath>
#include <initializer_list>

#include "common.hpp"
#include "ordered_reduce.hpp"

constexpr int kCountRecordWords = 8;  // the 64-byte count records; flow2d_correlation_record alone has 4 words

__device__ __forceinline__ bool finite(float x) { return fabsf(x) < INFINITY; }

// The NaN every entry writes where a node or pixel has no value.
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// Node (i, j) of the instance that starts `inst` floats into a node plane of `npitch` floats per row: addressed in 64 bits.
__device__ __forceinline__ size_t node_at(size_t inst, int i, int j, int npitch)
{
    return inst + static_cast<size_t>(j) * static_cast<size_t>(npitch) + static_cast<size_t>(i);
}

// Neighbour n (0 .. 7) of the ring: the 3 x 3 block without its centre, row by row.
__device__ __forceinline__ void ring_neighbour(int n, int& dx, int& dy)
{
    const int m = n < 4 ? n : n + 1;
    dx = m % 3 - 1;
    dy = m / 3 - 1;
}

// Adds the counts to the first N words of `instance`'s record of `Words` words, by 64-bit integer atomics (their order does not
// change a sum of integers).  The entry has zeroed the record on the stream; a count of 0 costs no atomic.
template <int Words, int N>
__device__ __forceinline__ void add_counts(unsigned long long* record, unsigned instance, const unsigned (&counts)[N])
{
    static_assert(N <= Words, "the counts lie inside the record");
    unsigned long long* rec = record + Words * static_cast<size_t>(instance);
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (counts[k]) atomicAdd(rec + k, static_cast<unsigned long long>(counts[k]));
}

// The same for per-thread counts: summed over the wave first, one set of atomics per wave.  Every lane of the wave calls it.
template <int Words, int N>
__device__ __forceinline__ void add_wave_counts(unsigned long long* record, unsigned instance, unsigned lane, unsigned (&counts)[N])
{
#pragma unroll
    for (int k = 0; k < N; ++k) counts[k] = wave_sum(counts[k]);
    if (lane == 0) add_counts<Words>(record, instance, counts);
}

namespace flow2d {

// The grid of flow2d_correlation_grid: whether it exists, and its nodes along an axis of `extent` pixels.
inline bool correlation_grid_ok(size_t width, size_t height, int radius, int spacing)
{
    return radius >= 1 && radius <= FLOW2D_CORRELATION_MAX_RADIUS && spacing >= 1 && spacing <= FLOW2D_CORRELATION_MAX_SPACING &&
           width >= static_cast<size_t>(2 * radius + 1) && height >= static_cast<size_t>(2 * radius + 1);
}
inline size_t correlation_nodes(size_t extent, int radius, int spacing) { return (extent - 2 * radius - 1) / spacing + 1; }

// The kernels number the nodes of a grid in 32 bits: a larger grid is FLOW2D_ERR_UNSUPPORTED.
inline bool node_count_ok(size_t nw, size_t nh) { return nw * nh < (size_t(1) << 31); }

// A count record: checked for alignment among the checks that hold without a device (null, an absent record, passes), and
// zeroed on the stream for every instance of the batch before the kernel adds to it.
template <typename Record>
bool record_aligned(const Record* record)
{
    return reinterpret_cast<uintptr_t>(record) % alignof(Record) == 0;
}
template <typename Record>
hipError_t clear_records(const flow2d_context* ctx, Record* record)
{
    return record ? hipMemsetAsync(record, 0, ctx->batch_count * sizeof(Record), ctx->stream) : hipSuccess;
}

// What the subset refinement's entries (subset_refine.hip, subset_refine2.hip, subset_refine_masked.hip; all through
// flow2d::subset_refine_enter of subset_node.hpp) check alike, in their order: the subset's radius from `min_radius`, the iterations, the bounds (finite and positive; the epsilon may be 0), the grid
// inside the frame as flow2d_correlation_grid lays it -- it may be smaller than the full one --, the record's alignment and
// the node count.  FLOW2D_ERR_UNSUPPORTED is the last of them: an entry hands on FLOW2D_ERR_INVALID_ARGUMENT at once and
// anything else behind the plane checks of its own, which all come before the node count.
inline int subset_refine_args_status(size_t width, size_t height, size_t nw, size_t nh, int grid_radius, int spacing, int min_radius,
                                     int subset_radius, int max_iterations, float epsilon, std::initializer_list<float> bounds,
                                     const flow2d_subset_record* record)
{
    if (subset_radius < min_radius || subset_radius > FLOW2D_SUBSET_MAX_RADIUS || max_iterations < 1 ||
        max_iterations > FLOW2D_SUBSET_MAX_ITERATIONS || !(std::isfinite(epsilon) && epsilon >= 0.f))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    for (const float bound : bounds)
        if (!(std::isfinite(bound) && bound > 0.f)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!correlation_grid_ok(width, height, grid_radius, spacing) || nw > correlation_nodes(width, grid_radius, spacing) ||
        nh > correlation_nodes(height, grid_radius, spacing) || !record_aligned(record))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    return node_count_ok(nw, nh) ? FLOW2D_OK : FLOW2D_ERR_UNSUPPORTED;
}

// plane_args_ok for every plane of one shape: the required ones, and the optional ones that are there.
inline bool planes_ok(std::initializer_list<const void*> required, std::initializer_list<const void*> optional, size_t w, size_t h,
                      size_t pitch_bytes)
{
    for (const void* p : required)
        if (!plane_args_ok(p, w, h, pitch_bytes)) return false;
    for (const void* p : optional)
        if (p && !plane_args_ok(p, w, h, pitch_bytes)) return false;
    return true;
}

}  // namespace flow2d
