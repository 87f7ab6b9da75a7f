// The alias predicate of csrc/byte_ranges.hpp against a brute-force intersection of byte sets.  Host only: built with the host
// compiler (and its address and undefined-behaviour sanitizers) by tests/test_byte_ranges_cpu.py, run as a program of its own.
//
// Every range lives in an arena of kArena bytes; a set of ranges { [p + b * stride, p + b * stride + bytes) : b < count } is a
// bitmap of the arena, and two sets meet when the bitmaps share a bit.  All bases, extents, strides and counts below are
// enumerated, absent (null) and empty ranges included, together with the layouts the entries meet in the pipeline.
#include <bitset>
#include <cstdio>
#include <cstdlib>

#include "byte_ranges.hpp"

namespace {

constexpr size_t kArena = 192;
using Bytes = std::bitset<kArena>;

unsigned char arena[kArena];
long checked = 0, failed = 0;

const void* at(long offset) { return offset < 0 ? nullptr : arena + offset; }  // -1: an absent range

Bytes set_of(long offset, size_t bytes, flow2d::Instances n)
{
    Bytes s;
    if (offset < 0) return s;
    for (size_t b = 0; b < n.count; ++b)
        for (size_t i = 0; i < bytes; ++i) {
            const size_t byte = static_cast<size_t>(offset) + b * n.stride_bytes + i;
            if (byte >= kArena) {
                std::fprintf(stderr, "the enumeration left the arena\n");
                std::exit(2);
            }
            s.set(byte);
        }
    return s;
}

// whether two instances of one set share a byte
bool meets_itself(long offset, size_t bytes, flow2d::Instances n)
{
    Bytes seen;
    for (size_t b = 0; offset >= 0 && b < n.count; ++b) {
        const Bytes one = set_of(offset + static_cast<long>(b * n.stride_bytes), bytes, flow2d::Instances{});
        if ((seen & one).any()) return true;
        seen |= one;
    }
    return false;
}

void expect(bool got, bool want, const char* what, long a, size_t a_bytes, long b, size_t b_bytes, flow2d::Instances n)
{
    ++checked;
    if (got == want) return;
    if (++failed <= 20)
        std::fprintf(stderr, "%s: a = %ld + %zu, b = %ld + %zu, count %zu, stride %zu: got %d, want %d\n", what, a, a_bytes, b, b_bytes,
                     n.count, n.stride_bytes, got, want);
}

void pairs()
{
    const size_t extents[] = {0, 1, 3, 8, 16, 21};
    for (size_t count = 1; count <= 4; ++count)
        for (size_t stride = 0; stride <= 40; stride += (stride < 8 ? 1 : 4)) {
            const flow2d::Instances n{count, stride};
            const long room = static_cast<long>(kArena - (count - 1) * stride - 21);
            for (long a = -1; a < 56 && a < room; ++a)
                for (long b = -1; b < 56 && b < room; b += (b < 30 ? 1 : 5))
                    for (size_t a_bytes : extents)
                        for (size_t b_bytes : extents) {
                            const bool want = (set_of(a, a_bytes, n) & set_of(b, b_bytes, n)).any();
                            expect(flow2d::strided_overlap(at(a), a_bytes, at(b), b_bytes, n), want, "strided_overlap", a, a_bytes, b, b_bytes, n);
                            expect(flow2d::strided_overlap(at(b), b_bytes, at(a), a_bytes, n), want, "strided_overlap, swapped", a, a_bytes, b,
                                   b_bytes, n);
                            if (count == 1) {
                                const bool plain = a >= 0 && b >= 0 && a_bytes && b_bytes && flow2d::ranges_overlap(at(a), a_bytes, at(b), b_bytes);
                                expect(plain, want, "ranges_overlap", a, a_bytes, b, b_bytes, n);
                            }
                            // what an entry asks: one written range against one read one, and against itself across the instances
                            const flow2d::ByteRange written[] = {{at(a), a_bytes}}, read[] = {{at(b), b_bytes}};
                            const bool any_want = want || (a_bytes && meets_itself(a, a_bytes, n));
                            expect(flow2d::any_overlap(written, read, n), any_want, "any_overlap", a, a_bytes, b, b_bytes, n);
                            const flow2d::ByteRange both[] = {{at(a), a_bytes}, {at(b), b_bytes}}, none[] = {{nullptr, 0}};
                            const bool both_want = any_want || (b_bytes && meets_itself(b, b_bytes, n));
                            expect(flow2d::any_overlap(both, none, n), both_want, "any_overlap, two written", a, a_bytes, b, b_bytes, n);
                            if (a >= 0) {
                                const bool same = a == b;
                                expect(flow2d::overlap_unless_identical(at(a), at(b), a_bytes, n),
                                       !same && (set_of(a, a_bytes, n) & set_of(b, a_bytes, n)).any(), "overlap_unless_identical", a, a_bytes, b,
                                       a_bytes, n);
                            }
                        }
        }
}

// The layouts of DESIGN.md, with a plane of 16 bytes: each named case must come out as stated there.
void layouts()
{
    const size_t plane = 16;
    struct Case {
        const char* what;
        long a, b;
        flow2d::Instances n;
        bool meet;
    } cases[] = {
        {"separate planes, one instance", 0, 16, {1, 0}, false},
        {"one row into the other", 0, 4, {1, 0}, true},
        {"tall containers one behind the other: A0 A1 A2 B0 B1 B2", 0, 48, {3, 16}, false},
        {"tall containers with padding between the instances", 0, 72, {3, 24}, false},
        {"interleaved A0 B0 A1 B1 A2 B2", 0, 16, {3, 32}, false},
        {"b starts one instance into a", 0, 16, {3, 16}, true},
        {"b starts two instances into a", 0, 32, {3, 16}, true},
        {"b starts one instance before a", 16, 0, {3, 16}, true},
        {"b starts sixteen bytes into a's padding, strides of 24", 0, 40, {3, 24}, true},
        {"b exactly count * stride behind a", 0, 72, {3, 24}, false},
    };
    for (const Case& c : cases) {
        const bool brute = (set_of(c.a, plane, c.n) & set_of(c.b, plane, c.n)).any();
        expect(brute, c.meet, c.what, c.a, plane, c.b, plane, c.n);  // (the case is what its name says)
        expect(flow2d::strided_overlap(at(c.a), plane, at(c.b), plane, c.n), c.meet, c.what, c.a, plane, c.b, plane, c.n);
    }
}

}  // namespace

int main()
{
    pairs();
    layouts();
    std::printf("byte_ranges_check: %ld comparisons, %ld wrong\n", checked, failed);
    return failed ? 1 : 0;
}
