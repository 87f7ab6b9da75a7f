// Window correlation for gfx950: the displacement of a (2r + 1)^2 window of frame 0 found by an exhaustive search of frame 1 for
// the largest zero-normalised cross-correlation, and the expansion of the node field to the frame's grid.  The body of the
// reference's Methods::Correlation, which it declares (data_structs.h) and never shipped.
//
// The normative definition is the one of flow2d_correlate_2d / flow2d_expand_nodes_2d in flow2d_c_abi.h.  Built
// -ffp-contract=off.  The frames are quantised to 8 bits while they are staged, so S0, S00, S1, S11 and S01 are exact integers in
// any order of summation; the score is three double operations on them.
//
// flow2d_correlate_2d.  A workgroup of four waves owns a tile of T x T nodes, T = corr_tile_nodes(spacing) = 32 / spacing held to
// 2 .. 8, and stages in LDS, one byte per pixel, the part of frame 0 its nodes' windows cover (at most 95 x 95) and the part of
// frame 1 their searches can reach (at most 159 x 159; what lies outside frame 1 is staged as 0 and never scored: a candidate's
// window lies inside the frame).  34.3 KB of LDS at the limits: four workgroups per CU.  Each wave then takes nodes of the tile in
// turn, alone -- no barrier after the staging:
//   1. S0 and S00: the lanes share the window's pixels, one butterfly;
//   2. the lanes share the (2d + 1)^2 displacements; a lane sums S1, S11 and S01 of its displacement over the window, four
//      pixels of a row at a time -- per patch the two aligned dwords around them (ds_read2_b32) and a byte funnel shift, then
//      three v_dot4_u32_u8; lanes of neighbouring dx read the same or neighbouring dwords and the frame-0 pair is a broadcast
//      --, scores it and keeps its best under the order of the header
//      (a total order: every lane of the butterfly that follows ends with the same peak);
//   3. lanes 0 .. 3 score the peak's four neighbours once more (the same integers, so the same doubles) instead of a table of up
//      to 4225 scores per node in LDS; lane 0 interpolates, writes the node and counts.
// The counts go to the record by 64-bit integer atomics, one set per wave; the entry zeroes the record on the stream first.
// This is the direct form: N multiply-adds per candidate and node.  It is the right body for sparse grids (spacing >= radius),
// where the windows of neighbouring nodes barely overlap; a dense grid would gain from sliding sums of the product image
// (DESIGN.md 3.13 says what that would take and why it is not here yet).
//
// flow2d_expand_nodes_2d: per pixel, the 64 x 4 geometry of plane_sample.hpp, four gathers from each node plane.
#include <cmath>

#include "correlate_score.hpp"
#include "node_grid.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kCorrThreads = 256, kCorrWaves = 4;
constexpr int kCorrTileSpan = 32;                  // T = kCorrTileSpan / spacing ...
constexpr int kCorrTileMin = 2, kCorrTileMax = 8;  // ... held to kCorrTileMin .. kCorrTileMax nodes per axis
// the farthest two nodes of a tile are (T - 1) * spacing pixels apart: 64 at most (T = 2, spacing 64)
constexpr int kCorrPatch0 = FLOW2D_CORRELATION_MAX_SPACING + 2 * FLOW2D_CORRELATION_MAX_RADIUS + 1;  // 95
constexpr int kCorrPatch1 = kCorrPatch0 + 2 * FLOW2D_CORRELATION_MAX_RANGE;                          // 159
constexpr int kExpandRows = 4;

inline int corr_tile_nodes(int spacing)
{
    const int t = kCorrTileSpan / spacing;
    return t < kCorrTileMin ? kCorrTileMin : t > kCorrTileMax ? kCorrTileMax : t;
}

struct CorrArgs {
    const float *f0, *f1;
    float *nu, *nv, *ns;         // ns: null = absent
    unsigned long long* record;  // four counts per instance, or null
    int w, h, pitch;             // the frames; pitch in floats
    int nw, nh, npitch;          // the node planes
    int r, d, s, tile;           // tile: nodes per tile axis
    unsigned tiles_x;
    float lo, scale, min_score;
};

template <typename Offset>
__global__ __launch_bounds__(kCorrThreads) void correlate_kernel(CorrArgs a, BatchArg batch)
{
    // (+ 8: the aligned dword pair of the last row's masked bytes may reach seven bytes past the patch)
    __shared__ __attribute__((aligned(16))) unsigned char s_q0[kCorrPatch0 * kCorrPatch0 + 8];
    __shared__ __attribute__((aligned(16))) unsigned char s_q1[kCorrPatch1 * kCorrPatch1 + 8];

    const size_t inst = batch_offset(batch);
    const float* __restrict__ f0 = a.f0 + inst;
    const float* __restrict__ f1 = a.f1 + inst;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int i_first = tile_x * a.tile, j_first = tile_y * a.tile;
    const int ni = min(a.tile, a.nw - i_first), nj = min(a.tile, a.nh - j_first);
    const int side = 2 * a.r + 1, d = a.d, s = a.s;
    const int p0w = (ni - 1) * s + side, p0h = (nj - 1) * s + side;  // <= kCorrPatch0
    const int p1w = p0w + 2 * d, p1h = p0h + 2 * d;                  // <= kCorrPatch1
    const int x0 = i_first * s, y0 = j_first * s;                    // the first pixel of the first node's window

    // frame 0: the windows of existing nodes lie inside the frame
    for (int i = tid; i < p0w * p0h; i += kCorrThreads) {
        const int y = i / p0w, x = i - y * p0w;
        s_q0[i] = static_cast<unsigned char>(quantise(load_at(f0, pixel_offset<Offset>(x0 + x, y0 + y, a.pitch)), a.lo, a.scale));
    }
    // frame 1: what lies outside the frame is not loaded, and never scored
    for (int i = tid; i < p1w * p1h; i += kCorrThreads) {
        const int y = i / p1w, x = i - y * p1w;
        const int gx = x0 - d + x, gy = y0 - d + y;
        unsigned q = 0;
        if (gx >= 0 && gy >= 0 && gx < a.w && gy < a.h) q = quantise(load_at(f1, pixel_offset<Offset>(gx, gy, a.pitch)), a.lo, a.scale);
        s_q1[i] = static_cast<unsigned char>(q);
    }
    __syncthreads();

    const int reach = 2 * d + 1, candidates = reach * reach, pixels = side * side;
    unsigned n_nodes = 0, n_invalid = 0, n_rejected = 0, n_unrefined = 0;  // the same in every lane of a wave
    for (int node = wave; node < ni * nj; node += kCorrWaves) {
        const int jn = node / ni, in = node - jn * ni;
        CorrNode nd;
        nd.q0 = s_q0 + jn * s * p0w + in * s;
        nd.q1 = s_q1 + (jn * s + d) * p1w + in * s + d;
        nd.p0w = p0w;
        nd.p1w = p1w;
        nd.left = x0 + in * s;
        nd.top = y0 + jn * s;
        nd.w = a.w;
        nd.h = a.h;
        nd.side = side;
        nd.n = pixels;

        unsigned s0 = 0, s00 = 0;
        for (int k = lane; k < pixels; k += 64) {
            const int wy = k / side, wx = k - wy * side;
            const unsigned q = nd.q0[wy * p0w + wx];
            s0 += q;
            s00 += q * q;
        }
        s0 = wave_sum(s0);
        s00 = wave_sum(s00);
        nd.s0 = s0;
        nd.v0 = nd.n * static_cast<long long>(s00) - nd.s0 * nd.s0;

        double best = -INFINITY;  // no candidate yet
        int bx = 0, by = 0;
        if (nd.v0 > 0) {
            for (int k = lane; k < candidates; k += 64) {
                const int ky = k / reach, dx = k - ky * reach - d, dy = ky - d;
                double c;
                if (score_at(nd, dx, dy, c) && comes_first(c, dx, dy, best, bx, by)) {
                    best = c;
                    bx = dx;
                    by = dy;
                }
            }
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
        const CorrResult res = finish_node(nd, d, lane, best, bx, by, 0, 0, a.min_score);
        n_nodes += 1;
        n_invalid += !res.found;
        n_rejected += res.rejected;
        n_unrefined += res.found && !res.rejected && !res.refined;
        if (lane == 0) {
            const size_t at = node_at(inst, i_first + in, j_first + jn, a.npitch);
            a.nu[at] = res.u;
            a.nv[at] = res.v;
            if (a.ns) a.ns[at] = res.score;
        }
    }
    if (a.record && lane == 0) {
        const unsigned counts[4] = {n_nodes, n_invalid, n_rejected, n_unrefined};
        add_counts<4>(a.record, blockIdx.z, counts);
    }
}

struct ExpandArgs {
    const float *nu, *nv;
    float *u_out, *v_out;
    int nw, nh, npitch;
    int w, h, pitch;
    float r, s;
};

template <typename Offset>
__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void expand_kernel(ExpandArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const float* __restrict__ nu = a.nu + inst;
    const float* __restrict__ nv = a.nv + inst;
    const int x = pixel_column();
    if (x >= a.w) return;
    float fx = (static_cast<float>(x) - a.r) / a.s;
    fx = fminf(fmaxf(fx, 0.f), static_cast<float>(a.nw - 1));
    const int i0 = static_cast<int>(floorf(fx)), i1 = min(i0 + 1, a.nw - 1);
    const float ax = fx - static_cast<float>(i0);
#pragma unroll
    for (int i = 0; i < kExpandRows; ++i) {
        const int y = pixel_row(kExpandRows, i);
        if (y >= a.h) continue;
        float fy = (static_cast<float>(y) - a.r) / a.s;
        fy = fminf(fmaxf(fy, 0.f), static_cast<float>(a.nh - 1));
        const int j0 = static_cast<int>(floorf(fy)), j1 = min(j0 + 1, a.nh - 1);
        const float ay = fy - static_cast<float>(j0);
        const float wt[4] = {(1.f - ax) * (1.f - ay), ax * (1.f - ay), (1.f - ax) * ay, ax * ay};
        const Offset at[4] = {pixel_offset<Offset>(i0, j0, a.npitch), pixel_offset<Offset>(i1, j0, a.npitch),
                              pixel_offset<Offset>(i0, j1, a.npitch), pixel_offset<Offset>(i1, j1, a.npitch)};
        float sw = 0.f, su = 0.f, sv = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float u = load_at(nu, at[k]), v = load_at(nv, at[k]);
            if (finite(u) && finite(v)) {
                sw += wt[k];
                su += wt[k] * u;
                sv += wt[k] * v;
            }
        }
        const Offset o = pixel_offset<Offset>(x, y, a.pitch);
        store_at(a.u_out + inst, o, sw > 0.f ? su / sw : quiet_nan());
        store_at(a.v_out + inst, o, sw > 0.f ? sv / sw : quiet_nan());
    }
}

}  // namespace

extern "C" {

int flow2d_correlation_grid(size_t width, size_t height, int radius, int spacing, size_t* nw, size_t* nh)
{
    if (!nw || !nh || !flow2d::correlation_grid_ok(width, height, radius, spacing)) return FLOW2D_ERR_INVALID_ARGUMENT;
    *nw = flow2d::correlation_nodes(width, radius, spacing);
    *nh = flow2d::correlation_nodes(height, radius, spacing);
    return FLOW2D_OK;
}

int flow2d_correlate_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                        size_t pitch_bytes, float lo, float scale, int radius, int range, int spacing, float min_score, float* node_u,
                        float* node_v, float* node_score, size_t node_pitch_bytes, flow2d_correlation_record* record)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!flow2d::planes_ok({frame_0, frame_1}, {}, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::correlation_grid_ok(width, height, radius, spacing) || range < 1 || range > FLOW2D_CORRELATION_MAX_RANGE)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(std::isfinite(scale) && scale > 0.f) || !std::isfinite(lo) || std::isnan(min_score)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const size_t nw = flow2d::correlation_nodes(width, radius, spacing), nh = flow2d::correlation_nodes(height, radius, spacing);
    if (!flow2d::planes_ok({node_u, node_v}, {node_score}, nw, nh, node_pitch_bytes) || !flow2d::record_aligned(record))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks the frames __restrict__: no written byte range may meet a frame or another written one
    auto aliased = [&](size_t frame_span, size_t node_span, size_t instances) {
        const flow2d::ByteRange written[] = {{node_u, node_span}, {node_v, node_span}, {node_score, node_span},
                                             {record, instances * sizeof(flow2d_correlation_record)}};
        const flow2d::ByteRange read[] = {{frame_0, frame_span}, {frame_1, frame_span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), flow2d::batch_span(ctx, nh * node_pitch_bytes), instances))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    const int tile = corr_tile_nodes(spacing);
    const unsigned tiles_x = flow2d::div_up(nw, tile), tiles_y = flow2d::div_up(nh, tile);
    const CorrArgs a = {frame_0, frame_1, node_u, node_v, node_score, reinterpret_cast<unsigned long long*>(record),
                        static_cast<int>(width), static_cast<int>(height), static_cast<int>(pitch_bytes / 4),
                        static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                        radius, range, spacing, tile, tiles_x, lo, scale, min_score};
    // (the largest offset a lane forms into a frame is below height * pitch_bytes; the node planes are addressed in 64 bits)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        correlate_kernel<decltype(offset)>
            <<<dim3(tiles_x * tiles_y, 1, flow2d::batch_z(ctx, 1)), dim3(kCorrThreads), 0, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

int flow2d_expand_nodes_2d(flow2d_context* ctx, const float* node_u, const float* node_v, size_t nw, size_t nh, size_t node_pitch_bytes,
                           int radius, int spacing, float* out_u, float* out_v, size_t width, size_t height, size_t pitch_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::planes_ok({node_u, node_v}, {}, nw, nh, node_pitch_bytes) || !flow2d::planes_ok({out_u, out_v}, {}, width, height, pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (radius < 0 || radius > FLOW2D_CORRELATION_MAX_RADIUS || spacing < 1 || spacing > FLOW2D_CORRELATION_MAX_SPACING)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    auto aliased = [&](size_t span, size_t node_span) {
        const flow2d::ByteRange written[] = {{out_u, span}, {out_v, span}};
        const flow2d::ByteRange read[] = {{node_u, node_span}, {node_v, node_span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, nh * node_pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), flow2d::batch_span(ctx, nh * node_pitch_bytes)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const ExpandArgs a = {node_u, node_v, out_u, out_v, static_cast<int>(nw), static_cast<int>(nh),
                          static_cast<int>(node_pitch_bytes / 4), static_cast<int>(width), static_cast<int>(height),
                          static_cast<int>(pitch_bytes / 4), static_cast<float>(radius), static_cast<float>(spacing)};
    const size_t span = height * pitch_bytes > nh * node_pitch_bytes ? height * pitch_bytes : nh * node_pitch_bytes;
    flow2d::launch_by_span(span, [&](auto offset) {
        expand_kernel<decltype(offset)><<<flow2d::pixel_grid(ctx, width, height, kExpandRows), flow2d::pixel_block(), 0, ctx->stream>>>(
            a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
