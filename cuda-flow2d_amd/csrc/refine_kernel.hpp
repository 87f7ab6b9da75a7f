// The kernel of flow2d_refine_flow_2d (refine.hip holds the entry and the description) and its launcher for one radius.  One
// translation unit per radius -- refine_instance.hip compiled seven times, side by side under make -j -- because the window loops
// are unrolled: the sixteen instantiations of r = 7 alone take minutes to compile.
#pragma once

#include <cmath>

#include "node_grid.hpp"
#include "plane_sample.hpp"

struct RefineArgs {
    const float *u, *v, *guide, *mask;  // guide / mask: null = absent
    float *u_out, *v_out;
    unsigned long long* record;  // four counts per instance, or null
    int w, h, pitch;
    float sg2, ss2;  // sigma_guide^2, sigma_space^2
    bool space;      // sigma_space > 0: the spatial weight is on
};

// flow2d_refine_launch_r<R>: the launch for radius R (refine_instance.hip); wide: 64-bit per-lane offsets (launch_by_span)
using RefineLaunch = void (*)(flow2d_context* ctx, const RefineArgs& a, bool wide, size_t width, size_t height);

namespace {

constexpr int kRefineRows = 4;                                  // consecutive rows per thread
constexpr int kTileCols = flow2d::kPixelBlockX;                 // 64
constexpr int kTileRows = flow2d::kPixelBlockY * kRefineRows;   // 16
constexpr int kThreads = flow2d::kPixelBlockX * flow2d::kPixelBlockY;

// unsigned keys in the order of the floats (-0 just below +0; NaNs at the ends, never selected: their weight is 0)
__device__ __forceinline__ unsigned key_of(float x)
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned bits_of(unsigned key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

template <typename Offset, int R, bool HasGuide, bool HasMask, bool HasSpace>
__global__ __launch_bounds__(kThreads) void refine_kernel(RefineArgs a, BatchArg batch)
{
    constexpr int D = 2 * R + 1, N = D * D, TW = kTileCols + 2 * R, TH = kTileRows + 2 * R;
    __shared__ unsigned s_ku[TH * TW], s_kv[TH * TW];
    __shared__ float s_w[TH * TW];
    __shared__ float s_g[HasGuide ? TH * TW : 1];

    const size_t inst = batch_offset(batch);
    const float* __restrict__ pu = a.u + inst;
    const float* __restrict__ pv = a.v + inst;
    const float* __restrict__ pg = HasGuide ? a.guide + inst : nullptr;
    const float* __restrict__ pm = HasMask ? a.mask + inst : nullptr;
    const int w = a.w, h = a.h, pitch = a.pitch;
    const int tid = threadIdx.y * kTileCols + threadIdx.x;
    const int x0 = blockIdx.x * kTileCols - R, y0 = blockIdx.y * kTileRows - R;

    // every index is clamped into the frame before it is loaded: what lies outside takes no part (weight 0)
    for (int i = tid; i < TH * TW; i += kThreads) {
        const int ty = i / TW, tx = i - ty * TW;
        const int x = x0 + tx, y = y0 + ty;
        const int xc = min(max(x, 0), w - 1), yc = min(max(y, 0), h - 1);
        const Offset o = pixel_offset<Offset>(xc, yc, pitch);
        const float fu = load_at(pu, o), fv = load_at(pv, o);
        float base = 1.f;
        if (HasMask) {
            float m = load_at(pm, o);
            if (!(m <= 1.f)) m = 1.f;
            if (!(m >= 0.f)) m = 0.f;
            base = 1.f - m;
        }
        const bool part = x == xc && y == yc && fabsf(fu) <= 1e9f && fabsf(fv) <= 1e9f;
        s_ku[i] = key_of(fu);
        s_kv[i] = key_of(fv);
        s_w[i] = part ? base : 0.f;
        if (HasGuide) s_g[i] = load_at(pg, o);
    }
    __syncthreads();

    const int gx = blockIdx.x * kTileCols + threadIdx.x;
    unsigned n_pixels = 0, n_unfilled = 0, n_filled = 0, n_changed = 0;
#pragma unroll 1
    for (int i = 0; i < kRefineRows; ++i) {
        const int ly = threadIdx.y * kRefineRows + i;
        const int gy = blockIdx.y * kTileRows + ly;
        if (gx >= w || gy >= h) continue;
        const int c = (ly + R) * TW + threadIdx.x + R;
        const float gc = HasGuide ? s_g[c] : 0.f;

        // 1. the window's integer weights, two to a register, their sum and the key range of the samples that count
        unsigned qq[(N + 1) / 2];
        unsigned total = 0, lo_u = ~0u, hi_u = 0u, lo_v = ~0u, hi_v = 0u;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int j = (dy + R) * D + dx + R, at = c + dy * TW + dx;
                float wt = s_w[at];
                if (HasGuide) {
                    const float d = s_g[at] - gc;
                    wt = wt * a.sg2 / (a.sg2 + d * d);
                }
                if (HasSpace) wt = wt * a.ss2 / (a.ss2 + static_cast<float>(dx * dx + dy * dy));
                const float scaled = floorf(4096.f * wt);
                const unsigned q = static_cast<unsigned>(static_cast<int>(fabsf(wt) < INFINITY ? scaled : 0.f));
                if (j & 1)
                    qq[j / 2] |= q << 16;
                else
                    qq[j / 2] = q;
                total += q;
                const unsigned ku = s_ku[at], kv = s_kv[at];
                lo_u = q ? min(lo_u, ku) : lo_u;
                hi_u = q ? max(hi_u, ku) : hi_u;
                lo_v = q ? min(lo_v, kv) : lo_v;
                hi_v = q ? max(hi_v, kv) : hi_v;
                // (one sample at a time: left alone, the scheduler issues the LDS loads of the whole window first and holds
                // their results and the divisions' temporaries -- 512 registers and a kilobyte of scratch at r = 6)
                asm volatile("" ::: "memory");
            }
        }

        // 2. the smallest key k with 2 * (weight of the keys <= k) >= total: it holds at hi and fails below lo throughout.
        // (total = 0: lo > hi, no step.)  A lane whose range is closed keeps it while the wave's widest one is open.
        while (lo_u < hi_u || lo_v < hi_v) {
            // (the keys are read from LDS again in every step: without this the compiler keeps the window's up to 450 keys in
            // registers across the steps -- 256 registers, one wave per SIMD and spills from r = 5 on)
            asm volatile("" ::: "memory");
            const unsigned mid_u = lo_u + ((hi_u - lo_u) >> 1), mid_v = lo_v + ((hi_v - lo_v) >> 1);
            unsigned below_u = 0, below_v = 0;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const int j = (dy + R) * D + dx + R, at = c + dy * TW + dx;
                    // (the weights stay packed across the steps: without this the compiler unpacks them once, before the
                    // loop, into a register each -- 225 at r = 7)
                    if ((j & 1) == 0) asm volatile("" : "+v"(qq[j / 2]));
                    const unsigned q = (j & 1) ? qq[j / 2] >> 16 : qq[j / 2] & 0xffffu;
                    below_u += s_ku[at] <= mid_u ? q : 0u;
                    below_v += s_kv[at] <= mid_v ? q : 0u;
                }
                asm volatile("" ::: "memory");  // (row by row, as above)
            }
            if (lo_u < hi_u) {
                if (2 * below_u >= total)
                    hi_u = mid_u;
                else
                    lo_u = mid_u + 1;
            }
            if (lo_v < hi_v) {
                if (2 * below_v >= total)
                    hi_v = mid_v;
                else
                    lo_v = mid_v + 1;
            }
        }

        // nothing usable in the window: the input's bits; a -0 result is written as +0
        const unsigned in_u = bits_of(s_ku[c]), in_v = bits_of(s_kv[c]);
        unsigned out_u = in_u, out_v = in_v;
        if (total) {
            out_u = bits_of(lo_u);
            out_v = bits_of(lo_v);
            out_u = out_u == 0x80000000u ? 0u : out_u;
            out_v = out_v == 0x80000000u ? 0u : out_v;
        }
        const Offset o = pixel_offset<Offset>(gx, gy, pitch);
        store_at(a.u_out + inst, o, __uint_as_float(out_u));
        store_at(a.v_out + inst, o, __uint_as_float(out_v));
        if (a.record) {
            n_pixels += 1;
            n_unfilled += total == 0;
            n_changed += out_u != in_u || out_v != in_v;
            if (HasMask) {
                // (1 - m of the staged weight cannot tell m >= 0.5 from just below it: the pixel's own value once more)
                const float m = load_at(pm, o);
                n_filled += total != 0 && !(m < 0.5f);
            }
        }
    }
    if (a.record) {
        // (every lane arrives here: the rows' loop has no early exit)
        const unsigned counts[4] = {wave_sum(n_pixels), wave_sum(n_unfilled), wave_sum(n_filled), wave_sum(n_changed)};
        if (threadIdx.x == 0) add_counts<4>(a.record, blockIdx.z, counts);
    }
}

template <typename Offset, int R, bool HasGuide, bool HasMask>
void launch_space(flow2d_context* ctx, const RefineArgs& a, size_t width, size_t height)
{
    const dim3 grid = flow2d::pixel_grid(ctx, width, height, kRefineRows), block = flow2d::pixel_block();
    if (a.space)
        refine_kernel<Offset, R, HasGuide, HasMask, true><<<grid, block, 0, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    else
        refine_kernel<Offset, R, HasGuide, HasMask, false><<<grid, block, 0, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
}

template <typename Offset, int R>
void launch_radius(flow2d_context* ctx, const RefineArgs& a, size_t width, size_t height)
{
    if (a.guide && a.mask)
        launch_space<Offset, R, true, true>(ctx, a, width, height);
    else if (a.guide)
        launch_space<Offset, R, true, false>(ctx, a, width, height);
    else if (a.mask)
        launch_space<Offset, R, false, true>(ctx, a, width, height);
    else
        launch_space<Offset, R, false, false>(ctx, a, width, height);
}

}  // namespace
