// Strain on the node grid of a DIC field for gfx950: the nine quantities of flow2d_deformation_2d from the gradients a subset
// refinement delivered (window 0) or from a least-squares polynomial fitted to the usable nodes of a strain window around each
// node (Pan et al., Opt. Eng. 2009), with ordered statistics.  No reference counterpart.
//
// The normative definition is the one of flow2d_node_strain_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// One thread per node on the 64 x 4 geometry of plane_sample.hpp (one row per thread); the node planes are addressed in 64 bits.
// Window fit: the workgroup stages the (64 + 2m) x (4 + 2m) tile of u, v and the usable flag in LDS once -- every index is
// tested against the grid before it is loaded, what lies outside is staged as not usable -- and each thread walks its
// (2m + 1)^2 window from the tile in raster order.  A tap that is not usable is skipped by a branch, never multiplied by 0:
// no NaN reaches a sum.  The normal matrix is a sum of integer monomials di^p dj^q (p + q <= 2 * order); they are added in
// 32-bit integers, which is exact here (at most 225 taps of at most 7^4) and therefore the header's 64-bit sum.  The k x k
// Cholesky factorisation and the two solves run per thread in registers: every loop over k is unrolled, no array is indexed
// by a run-time value.  The factor is not shared between the nodes of a whole window: every node factors its own matrix.
// Direct form (window 0): seven loads per node, no tile.
//
// Statistics are the two-launch ordered reduction of ordered_reduce.hpp: one slab per workgroup, then one workgroup per
// instance adds the slabs in block order.
#include <cfloat>
#include <cmath>

#include "node_strain_common.hpp"
#include "small_cholesky.hpp"

namespace {

struct StrainArgs {
    const float *u, *v, *state;  // state: null = absent
    const float* grad[4];        // ux, uy, vx, vy: read when window == 0
    float* out[9];               // the planes of flow2d_deformation_planes, null = not requested
    int nw, nh, npitch;
    int s, window, min_nodes, measure;
    float min_state;
};

// Order: 0 = direct (window 0), 1 / 2 = window fit of that order.
template <int Order, bool Stats>
__global__ __launch_bounds__(kThreads) void node_strain_kernel(StrainArgs in, NodeStrainSums* __restrict__ partials, BatchArg batch)
{
    constexpr int K = Order == 2 ? 6 : 3;
    constexpr int kTile = Order == 0 ? 1 : kTileW * kTileH;
    __shared__ float tile_u[kTile], tile_v[kTile];
    __shared__ unsigned char tile_ok[kTile];

    const size_t inst = batch_offset(batch);
    const int i = pixel_column();
    const int j = static_cast<int>(pixel_row(1, 0));
    const bool active = i < in.nw && j < in.nh;
    const size_t at = node_at(inst, active ? i : 0, active ? j : 0, in.npitch);

    int reason = kCentre;
    double ga = 0.0, gb = 0.0, gc = 0.0, gd = 0.0;
    if (Order == 0) {
        if (active) {
            const float u = in.u[at], v = in.v[at];
            const float ux = in.grad[0][at], uy = in.grad[1][at], vx = in.grad[2][at], vy = in.grad[3][at];
            const bool state_ok = in.state ? in.state[at] >= in.min_state : true;
            if (state_ok && finite(u) && finite(v) && finite(ux) && finite(uy) && finite(vx) && finite(vy)) {
                reason = kValid;
                ga = static_cast<double>(ux);
                gb = static_cast<double>(uy);
                gc = static_cast<double>(vx);
                gd = static_cast<double>(vy);
            }
        }
    } else {
        const int m = in.window;
        const int tw = flow2d::kPixelBlockX + 2 * m, th = flow2d::kPixelBlockY + 2 * m;
        const int x0 = static_cast<int>(blockIdx.x) * flow2d::kPixelBlockX - m;
        const int y0 = static_cast<int>(blockIdx.y) * flow2d::kPixelBlockY - m;
        const int tid = threadIdx.y * flow2d::kPixelBlockX + threadIdx.x;
        for (int t = tid; t < tw * th; t += kThreads) {
            const int ty = t / tw, tx = t - ty * tw;
            const int x = x0 + tx, y = y0 + ty;
            float u = 0.f, v = 0.f;
            bool ok = false;
            if (x >= 0 && y >= 0 && x < in.nw && y < in.nh) {
                const size_t q = node_at(inst, x, y, in.npitch);
                u = in.u[q];
                v = in.v[q];
                ok = (in.state ? in.state[q] >= in.min_state : true) && finite(u) && finite(v);
            }
            tile_u[t] = u;
            tile_v[t] = v;
            tile_ok[t] = ok ? 1 : 0;
        }
        __syncthreads();
        const int centre = (static_cast<int>(threadIdx.y) + m) * tw + static_cast<int>(threadIdx.x) + m;
        if (active && tile_ok[centre]) {
            const double uc = static_cast<double>(tile_u[centre]), vc = static_cast<double>(tile_v[centre]);
            // the monomial sums S[p][q] = sum of di^p dj^q, p + q <= 2 * Order, and the right-hand sides
            int S[5][5];
#pragma unroll
            for (int p = 0; p < 5; ++p)
#pragma unroll
                for (int q = 0; q < 5; ++q) S[p][q] = 0;
            double bu[K], bv[K];
#pragma unroll
            for (int a = 0; a < K; ++a) bu[a] = bv[a] = 0.0;
            for (int dj = -m; dj <= m; ++dj) {
                const int row = centre + dj * tw;
                for (int di = -m; di <= m; ++di) {
                    if (!tile_ok[row + di]) continue;
                    const double wu = static_cast<double>(tile_u[row + di]) - uc;
                    const double wv = static_cast<double>(tile_v[row + di]) - vc;
                    int pi[5], pj[5];
                    pi[0] = pj[0] = 1;
#pragma unroll
                    for (int p = 1; p < 5; ++p) {
                        pi[p] = pi[p - 1] * di;
                        pj[p] = pj[p - 1] * dj;
                    }
#pragma unroll
                    for (int p = 0; p <= 2 * Order; ++p)
#pragma unroll
                        for (int q = 0; p + q <= 2 * Order; ++q) S[p][q] += pi[p] * pj[q];
#pragma unroll
                    for (int a = 0; a < K; ++a) {
                        const double phi = static_cast<double>(pi[exp_i(a)] * pj[exp_j(a)]);
                        bu[a] += phi * wu;
                        bv[a] += phi * wv;
                    }
                }
            }
            const int n = S[0][0];
            if (!(n >= in.min_nodes)) {
                reason = kSparse;
            } else {
                double L[K][K];
#pragma unroll
                for (int a = 0; a < K; ++a)
#pragma unroll
                    for (int b = 0; b < K; ++b)
                        L[a][b] = static_cast<double>(static_cast<long long>(S[exp_i(a) + exp_i(b)][exp_j(a) + exp_j(b)]));
                if (!factor<K>(L)) {
                    reason = kDegenerate;
                } else {
                    double cu[K], cv[K];
                    solve<K>(L, bu, cu);
                    solve<K>(L, bv, cv);
                    const double s = static_cast<double>(in.s);
                    reason = kValid;
                    ga = cu[1] / s;
                    gb = cu[2] / s;
                    gc = cv[1] / s;
                    gd = cv[2] / s;
                }
            }
        }
    }

    NodeStrainSums acc;
    if (Stats) acc.clear();
    if (active) {
        const bool valid = reason == kValid;
        float q[9];
        quantities(ga, gb, gc, gd, in.measure, q);
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (in.out[k]) in.out[k][at] = valid ? q[k] : quiet_nan();
        if (Stats) {
            const float x[kStrainQuantities] = {q[0], q[1], q[2], q[6], q[7], q[8]};
#pragma unroll
            for (int k = 0; k < kStrainQuantities; ++k) {
                const double t = valid ? static_cast<double>(x[k]) : 0.0;
                acc.sum[k] += t;
                acc.sum_sq[k] += t * t;
                acc.min[k] = (valid && x[k] < acc.min[k]) ? x[k] : acc.min[k];
                acc.max[k] = (valid && x[k] > acc.max[k]) ? x[k] : acc.max[k];
            }
            acc.valid += valid;
            acc.invalid += !valid;
#pragma unroll
            for (int k = 0; k < kReasons; ++k) acc.reasons[k] += reason == k;
        }
    }
    if (Stats) {
        // (every thread of the workgroup arrives here: the reduction holds a barrier)
        if (workgroup_reduce<flow2d::kPixelBlockY>(acc, threadIdx.x, threadIdx.y))
            partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}

template <int Order>
void launch_order(flow2d_context* ctx, const StrainArgs& a, NodeStrainSums* partials, size_t nw, size_t nh)
{
    const dim3 grid = flow2d::pixel_grid(ctx, nw, nh, 1), block = flow2d::pixel_block();
    if (partials)
        node_strain_kernel<Order, true><<<grid, block, 0, ctx->stream>>>(a, partials, flow2d::batch_arg(ctx, 1));
    else
        node_strain_kernel<Order, false><<<grid, block, 0, ctx->stream>>>(a, nullptr, flow2d::batch_arg(ctx, 1));
}

}  // namespace

extern "C" {

size_t flow2d_node_strain_workspace_bytes(size_t nw, size_t nh, size_t instances)
{
    if (nw == 0 || nh == 0 || instances == 0) return 0;
    return partial_blocks(nw, nh) * instances * sizeof(NodeStrainSums);
}

int flow2d_node_strain_2d(flow2d_context* ctx, const float* node_u, const float* node_v, const float* node_state, const float* node_ux,
                          const float* node_uy, const float* node_vx, const float* node_vy, size_t nw, size_t nh,
                          size_t node_pitch_bytes, int spacing, int window, int order, int min_nodes, int min_state, int measure,
                          const flow2d_deformation_planes* out, flow2d_deformation_stats* stats, void* workspace,
                          size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const flow2d_deformation_planes p = out ? *out : flow2d_deformation_planes{};
    float* const planes[9] = {p.divergence, p.vorticity, p.dilatation, p.exx, p.eyy, p.exy, p.e1, p.e2, p.max_shear};
    if (!flow2d::planes_ok({node_u, node_v},
                           {node_state, node_ux, node_uy, node_vx, node_vy, planes[0], planes[1], planes[2], planes[3], planes[4],
                            planes[5], planes[6], planes[7], planes[8]},
                           nw, nh, node_pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const float* const grads[4] = {node_ux, node_uy, node_vx, node_vy};
    int given = 0;
    for (const float* g : grads) given += g != nullptr;
    if (given != 0 && given != 4) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (spacing < 1 || spacing > FLOW2D_CORRELATION_MAX_SPACING || window < 0 || window > FLOW2D_NODE_STRAIN_MAX_WINDOW ||
        min_state < 0 || min_state > 1 || (measure != FLOW2D_STRAIN_SMALL && measure != FLOW2D_STRAIN_GREEN_LAGRANGE))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (window == 0) {
        if (given != 4) return FLOW2D_ERR_INVALID_ARGUMENT;
    } else {
        if (order != 1 && order != 2) return FLOW2D_ERR_INVALID_ARGUMENT;
        const int k = order == 2 ? 6 : 3, side = 2 * window + 1;
        if (min_nodes < k || min_nodes > side * side) return FLOW2D_ERR_INVALID_ARGUMENT;
    }
    bool any = stats != nullptr;
    for (float* q : planes) any = any || q != nullptr;
    if (!any) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(stats) || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    if (stats && (!workspace || workspace_bytes < flow2d_node_strain_workspace_bytes(nw, nh, 1))) return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel reads its neighbours' inputs while their threads write: no written byte range may meet a read one or another
    // written one.  Without statistics the workspace is not touched and takes no part.
    auto aliased = [&](size_t span, size_t instances) {
        flow2d::ByteRange written[11];
        for (int k = 0; k < 9; ++k) written[k] = {planes[k], span};
        written[9] = {stats, instances * sizeof(flow2d_deformation_stats)};
        written[10] = {stats ? workspace : nullptr, workspace_bytes};
        const flow2d::ByteRange read[] = {{node_u, span},  {node_v, span},  {node_state, span}, {node_ux, span},
                                          {node_uy, span}, {node_vx, span}, {node_vy, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (stats && workspace_bytes < flow2d_node_strain_workspace_bytes(nw, nh, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    StrainArgs a;
    a.u = node_u;
    a.v = node_v;
    a.state = node_state;
    for (int k = 0; k < 4; ++k) a.grad[k] = grads[k];
    for (int k = 0; k < 9; ++k) a.out[k] = planes[k];
    a.nw = static_cast<int>(nw);
    a.nh = static_cast<int>(nh);
    a.npitch = static_cast<int>(node_pitch_bytes / 4);
    a.s = spacing;
    a.window = window;
    a.min_nodes = min_nodes;
    a.measure = measure;
    a.min_state = static_cast<float>(min_state);
    NodeStrainSums* partials = stats ? static_cast<NodeStrainSums*>(workspace) : nullptr;
    if (window == 0)
        launch_order<0>(ctx, a, partials, nw, nh);
    else if (order == 1)
        launch_order<1>(ctx, a, partials, nw, nh);
    else
        launch_order<2>(ctx, a, partials, nw, nh);
    FLOW2D_CHECK_LAUNCH();
    if (stats) {
        strain_final_kernel<<<dim3(static_cast<unsigned>(instances)), dim3(kStrainFinalThreads), 0, ctx->stream>>>(
            partials, static_cast<unsigned>(partial_blocks(nw, nh)), stats);
        FLOW2D_CHECK_LAUNCH();
    }
    return FLOW2D_OK;
}

}  // extern "C"
