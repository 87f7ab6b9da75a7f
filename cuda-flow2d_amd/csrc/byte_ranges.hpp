// The alias rule of the C-ABI entries, host only (no HIP include: tests/c/byte_ranges_check.cpp builds it with the host compiler).
//
// Every kernel marks its planes __restrict__ and reads neighbours that other threads write, so an entry refuses a written
// byte range that meets a read one or another written one -- whole ranges, not base pointers, and over every instance of a
// lock-step batch.  A plane of an entry stands for the set of ranges
//     { [p + b * stride, p + b * stride + bytes) : b < count }
// and two planes meet when any range of the one shares a byte with any range of the other.  Exact per instance, not a test
// of the hulls: A0 B0 A1 B1 (stride = two planes) shares no byte and passes.
#pragma once

#include <cstddef>
#include <cstdint>

namespace flow2d {

struct ByteRange {
    const void* p;  // null: an optional argument that is absent, skipped
    size_t bytes;   // 0: holds no byte, meets nothing
};

// The instances of a launch: flow2d_context_set_batch's count and stride in bytes.  {1, 0}: no batch.
struct Instances {
    size_t count = 1;
    size_t stride_bytes = 0;
};

inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

// Whether instance i of a meets instance j of b for some i, j < count.  With k = j - i (every |k| < count occurs) and a the
// higher base, D = a - b: the ranges meet when D - b_bytes < k * stride < D + a_bytes.  k = 0 does when D < b_bytes; otherwise
// the smallest k * stride above D - b_bytes decides, as every larger one is further from the lower bound.  No loop, no allocation.
inline bool strided_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes, Instances n)
{
    if (!a || !b || a_bytes == 0 || b_bytes == 0 || n.count == 0) return false;
    uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    if (pa < pb) {  // (symmetric: k becomes -k)
        const uintptr_t p = pa;
        pa = pb, pb = p;
        const size_t s = a_bytes;
        a_bytes = b_bytes, b_bytes = s;
    }
    const uintptr_t distance = pa - pb;
    if (distance < b_bytes) return true;  // the same instance of both
    if (n.count == 1 || n.stride_bytes == 0) return false;
    const uintptr_t below = distance - b_bytes;
    if (below / n.stride_bytes + 1 > n.count - 1) return false;   // the instance of b that far up does not exist
    const uintptr_t past = n.stride_bytes - below % n.stride_bytes;  // k * stride - below, in (0, stride]
    return past < a_bytes + b_bytes;
}

// Whether two instances of one plane meet each other: a stride shorter than the plane.
inline bool self_overlap(size_t bytes, Instances n) { return n.count > 1 && n.stride_bytes < bytes; }

// Whether any written range meets a read one, another written one or another instance of itself.  Without `n`: the planes
// of one instance, which need no context field (the analysis entries check so before FLOW2D_ENTER).
inline bool any_overlap(const ByteRange* written, size_t n_written, const ByteRange* read, size_t n_read, Instances n = Instances{})
{
    for (size_t i = 0; i < n_written; ++i) {
        if (!written[i].p) continue;
        if (self_overlap(written[i].bytes, n)) return true;
        for (size_t j = 0; j < n_read; ++j)
            if (strided_overlap(written[i].p, written[i].bytes, read[j].p, read[j].bytes, n)) return true;
        for (size_t j = i + 1; j < n_written; ++j)
            if (strided_overlap(written[i].p, written[i].bytes, written[j].p, written[j].bytes, n)) return true;
    }
    return false;
}
template <size_t W, size_t R>
bool any_overlap(const ByteRange (&written)[W], const ByteRange (&read)[R], Instances n = Instances{})
{
    return any_overlap(written, W, read, R, n);
}

// An entry that works in place names the plane among its written ones and again among its read ones where another argument
// may be the same plane (operand_1 of the additions): exact identity -- the same base, hence the same instances -- is the one
// legal way for the two to meet.
inline bool overlap_unless_identical(const void* written, const void* read, size_t bytes, Instances n)
{
    return written != read && strided_overlap(written, bytes, read, bytes, n);
}

}  // namespace flow2d
