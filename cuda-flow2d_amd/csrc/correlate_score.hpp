// The scoring code of the window correlation, shared by flow2d_correlate_2d (correlate.hip: patches staged per tile of nodes) and
// flow2d_correlate_offset_2d (correlate_offset.hip: patches staged per node, around the node's predictor offset): the
// quantisation, the exact integer sums and the score of one displacement on byte patches in LDS, the order of the peak, and the
// tail of a node -- the peak among the lanes, its four neighbours, the parabola, rejection.  The normative text is the one of
// flow2d_correlate_2d in flow2d_c_abi.h.  Both files are built -ffp-contract=off.
#pragma once

#include <cmath>

#include "ordered_reduce.hpp"

namespace {

__device__ __forceinline__ unsigned quantise(float sample, float lo, float scale)
{
    const float t = (sample - lo) * scale;
    if (!(t > 0.f)) return 0u;
    if (t >= 255.f) return 255u;
    return static_cast<unsigned>(static_cast<int>(t + 0.5f));
}

// whether (c1, dx1, dy1) comes before (c2, dx2, dy2) in the order of the peak
__device__ __forceinline__ bool comes_first(double c1, int dx1, int dy1, double c2, int dx2, int dy2)
{
    if (c1 != c2) return c1 > c2;
    const int n1 = dx1 * dx1 + dy1 * dy1, n2 = dx2 * dx2 + dy2 * dy2;
    if (n1 != n2) return n1 < n2;
    if (dy1 != dy2) return dy1 < dy2;
    return dx1 < dx2;
}

// One node's view of the staged patches: q0 at its window's first pixel, q1 at the pixel displacement (0, 0) puts there.
struct CorrNode {
    const unsigned char *q0, *q1;
    int p0w, p1w;      // row lengths of the patches
    int left, top;     // the first pixel in the frame of the window displacement (0, 0) gives
    int w, h, side;    // the frame; side = 2r + 1
    long long n, s0, v0;
};

// The four bytes at p, which may have any alignment: the two aligned dwords around them (one ds_read2_b32) and a byte funnel
// shift.  (One dword load at a byte address is legal in LDS and gives the same bytes; measured, the whole kernel is 5.6 times
// slower with it: 13.3 against 2.4 ms on the PIV grid at 4096^2.)  A patch therefore starts 4-byte aligned and has 8 bytes of
// slack behind it.
__device__ __forceinline__ unsigned four_pixels(const unsigned char* p)
{
    const unsigned shift = static_cast<unsigned>(reinterpret_cast<uintptr_t>(p)) & 3u;
    const unsigned* q = reinterpret_cast<const unsigned*>(p - shift);
    return __builtin_amdgcn_alignbyte(q[1], q[0], shift);
}

// The score of displacement (dx, dy); false when it is no candidate.
__device__ __forceinline__ bool score_at(const CorrNode& nd, int dx, int dy, double& c)
{
    const int lx = nd.left + dx, ly = nd.top + dy;
    if (lx < 0 || ly < 0 || lx + nd.side > nd.w || ly + nd.side > nd.h) return false;
    const unsigned char* p0 = nd.q0;
    const unsigned char* p1 = nd.q1 + dy * nd.p1w + dx;
    unsigned s1 = 0, s11 = 0, s01 = 0;  // at most 961 * 255^2 < 2^26
    // four pixels of a row at a time: four bytes of each patch (four_pixels) and three packed byte dot products.  A row has an odd
    // number of pixels: its last one or three come from four bytes of which the others -- the next pixels of the patch, or the
    // arrays' padding -- are masked off.
    const int quads = nd.side >> 2;
    const unsigned tail = (1u << (8 * (nd.side & 3))) - 1u;
    for (int wy = 0; wy < nd.side; ++wy) {
        for (int q = 0; q < quads; ++q) {
            const unsigned a = four_pixels(p0 + 4 * q), b = four_pixels(p1 + 4 * q);
            s1 = __builtin_amdgcn_udot4(b, 0x01010101u, s1, false);
            s11 = __builtin_amdgcn_udot4(b, b, s11, false);
            s01 = __builtin_amdgcn_udot4(a, b, s01, false);
        }
        const unsigned a = four_pixels(p0 + 4 * quads) & tail, b = four_pixels(p1 + 4 * quads) & tail;
        s1 = __builtin_amdgcn_udot4(b, 0x01010101u, s1, false);
        s11 = __builtin_amdgcn_udot4(b, b, s11, false);
        s01 = __builtin_amdgcn_udot4(a, b, s01, false);
        p0 += nd.p0w;
        p1 += nd.p1w;
    }
    const long long l1 = s1;
    const long long v1 = nd.n * static_cast<long long>(s11) - l1 * l1;
    if (v1 <= 0) return false;
    const long long cov = nd.n * static_cast<long long>(s01) - nd.s0 * l1;
    c = static_cast<double>(cov) / sqrt(static_cast<double>(nd.v0) * static_cast<double>(v1));
    return true;
}

// S0 and S00 of the node's window into nd.s0 and nd.v0: the lanes share the window's pixels, one butterfly.  (correlate_kernel keeps
// its own spelled-out form of this and of wave_peak: through these two calls the same steps compile to another instruction
// stream there, and that kernel's compiled code is held fixed.  finish_node compiles to its former stream.)
__device__ __forceinline__ void window_moments(CorrNode& nd, int lane)
{
    const int pixels = nd.side * nd.side;
    unsigned s0 = 0, s00 = 0;
    for (int k = lane; k < pixels; k += 64) {
        const int wy = k / nd.side, wx = k - wy * nd.side;
        const unsigned q = nd.q0[wy * nd.p0w + wx];
        s0 += q;
        s00 += q * q;
    }
    s0 = wave_sum(s0);
    s00 = wave_sum(s00);
    nd.s0 = s0;
    nd.v0 = nd.n * static_cast<long long>(s00) - nd.s0 * nd.s0;
}

// The lanes' best candidates to the wave's: a total order, so every lane ends with the same peak.
__device__ __forceinline__ void wave_peak(double& best, int& bx, int& by)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(best, o, 64);
        const int ox = __shfl_xor(bx, o, 64), oy = __shfl_xor(by, o, 64);
        if (comes_first(oc, ox, oy, best, bx, by)) {
            best = oc;
            bx = ox;
            by = oy;
        }
    }
}

// What a node delivers, the same in every lane of its wave.
struct CorrResult {
    float u, v, score;
    bool found, rejected, refined;
};

// The tail of a node whose peak (best, bx, by) every lane holds, best = -inf without a candidate: lanes 0 .. 3 score the peak's
// four neighbours once more (the same integers, so the same doubles), the parabola per axis, the minimum score.  (ox, oy): the
// node's offset, added to the integer peak before the sub-pixel part.
__device__ __forceinline__ CorrResult finish_node(const CorrNode& nd, int d, int lane, double best, int bx, int by, int ox, int oy,
                                                  float min_score)
{
    CorrResult res;
    const float nan = __uint_as_float(0x7FC00000u);
    const bool found = best > -INFINITY;  // (a score is finite: V0 > 0 and V1 > 0)

    // the four neighbours of the peak, by lanes 0 .. 3: (-1, 0), (+1, 0), (0, -1), (0, +1)
    const bool inner = found && abs(bx) < d && abs(by) < d;
    double cn = 0.0;
    bool has = false;
    if (inner && lane < 4) has = score_at(nd, bx + (lane == 0 ? -1 : lane == 1 ? 1 : 0), by + (lane == 2 ? -1 : lane == 3 ? 1 : 0), cn);
    const bool refined = inner && (__ballot(has) & 0xFull) == 0xFull;
    const double cxm = __shfl(cn, 0, 64), cxp = __shfl(cn, 1, 64), cym = __shfl(cn, 2, 64), cyp = __shfl(cn, 3, 64);

    // (this order of the declarations, and v before u below, is the one that leaves correlate_kernel's compiled code as it was)
    float score = 0.f, u = nan, v = nan;
    bool rejected = false;
    if (found) {
        double delta_x = 0.0, delta_y = 0.0;
        if (refined) {
            const double den_x = (cxm - 2.0 * best) + cxp, den_y = (cym - 2.0 * best) + cyp;
            delta_x = den_x < 0.0 ? (cxm - cxp) / (2.0 * den_x) : 0.0;
            delta_y = den_y < 0.0 ? (cym - cyp) / (2.0 * den_y) : 0.0;
        }
        score = static_cast<float>(best);
        rejected = score < min_score;
        if (!rejected) {
            v = static_cast<float>(static_cast<double>(oy + by) + delta_y);
            u = static_cast<float>(static_cast<double>(ox + bx) + delta_x);
        }
    }
    res.u = u;
    res.v = v;
    res.score = score;
    res.found = found;
    res.rejected = rejected;
    res.refined = refined;
    return res;
}

}  // namespace
