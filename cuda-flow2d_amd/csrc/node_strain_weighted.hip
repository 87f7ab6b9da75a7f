// Weighted strain windows on the node grid of a DIC field for gfx950: the window fit of flow2d_node_strain_2d as a Gauss-Markov
// fit with the inverse variances of flow2d_subset_uncertainty_2d as weights (Aitken, Proc. R. Soc. Edinburgh 55 (1935)), the
// standard deviations of the strain from the inverse of the matrices it factors anyway, and the Cauchy reweighting of
// flow2d_node_strain_robust_2d with a scale in sigmas.  No reference counterpart.
//
// The normative definition is the one of flow2d_node_strain_weighted_2d in flow2d_c_abi.h, in IEEE double.  Built
// -ffp-contract=off.
//
// The geometry is node_strain_robust.hip's: one thread per node on the 64 x 4 block, the (64 + 2m) x (4 + 2m) tile staged in LDS
// once -- u, v, the two inverse variances as doubles (the divisions are done once per node of the tile, not once per tap and
// walk) and a flag byte.  u and v have matrices of their own, so every pass walks the window twice and keeps ONE set of moment
// sums and ONE right-hand side live; the u coefficients of a pass wait in LDS (6 doubles per thread) while the v walk still
// weights its taps by the previous pass's.  2 (K + 1) walks for the fits and one for the residuals of the last, which is left
// out where nothing asks for it (T = 0 and no diagnostic plane: every tap is kept).  Factorisation and solves are
// small_cholesky.hpp's; the arrays live in registers (no scratch; profiles/weighted_strain/README.md has the register counts).
//
// Statistics are the two-launch ordered reduction of ordered_reduce.hpp with slabs of WeightedStrainSums.
#include <cfloat>
#include <cmath>

#include "node_strain_common.hpp"
#include "small_cholesky.hpp"

namespace {

// nodes with a rejected tap, rejected taps, suspect nodes (over the finished nodes) and the usable nodes that are not weighable
// (over the grid): reserved[3 .. 6] of the record
constexpr int kWeightedCounts = 4;
constexpr int kSigmaPlanes = 9;
constexpr unsigned char kUsable = 1, kWeighable = 2;

// NodeStrainSums with the four counts of the weighted fit.
struct WeightedStrainSums : NodeStrainSums {
    unsigned long long weighted[kWeightedCounts];

    __device__ __forceinline__ void clear()
    {
        NodeStrainSums::clear();
#pragma unroll
        for (int k = 0; k < kWeightedCounts; ++k) weighted[k] = 0;
    }
    __device__ __forceinline__ void combine(const WeightedStrainSums& q)
    {
        NodeStrainSums::combine(q);
#pragma unroll
        for (int k = 0; k < kWeightedCounts; ++k) weighted[k] += q.weighted[k];
    }
    __device__ __forceinline__ void across_lanes()
    {
        NodeStrainSums::across_lanes();
#pragma unroll
        for (int k = 0; k < kWeightedCounts; ++k) weighted[k] = wave_sum(weighted[k]);
    }
    __device__ __forceinline__ void fill(flow2d_deformation_stats& rec) const
    {
        NodeStrainSums::fill(rec);
        for (int k = 0; k < kWeightedCounts; ++k) rec.reserved[kReasons + k] = weighted[k];
    }
};
static_assert(sizeof(WeightedStrainSums) == 224, "flow2d_node_strain_weighted_workspace_bytes counts slabs of 224 bytes");

struct WeightedArgs {
    const float *u, *v, *state;  // state: null = absent
    const float *su, *sv;        // the nodes' sigma_u and sigma_v
    float* out[9];               // the planes of flow2d_deformation_planes, null = not requested
    float* diag[3];              // residual, rejected, centre, null = not requested
    float* sig[kSigmaPlanes];    // the planes of flow2d_strain_sigma_planes, null = not requested
    int nw, nh, npitch;
    int s, window, min_nodes, measure, passes;  // passes = K
    int residuals;                              // the walk for the residuals of pass K is needed: T > 0 or a diagnostic plane
    float min_state;
    double f2, t2;  // floor * floor, T * T
};

// The nine standard deviations of the header from the gradients and the six covariances, each cast to float once.
__device__ __forceinline__ void sigmas(double a, double b, double c, double d, double Vaa, double Vab, double Vbb, double Vcc,
                                       double Vcd, double Vdd, int measure, float (&q)[kSigmaPlanes])
{
    double Vexx = Vaa, Veyy = Vdd, Vexy = 0.25 * (Vbb + Vcc);
    if (measure == FLOW2D_STRAIN_GREEN_LAGRANGE) {
        const double ja = 1.0 + a, jd = 1.0 + d;
        Vexx = (ja * ja) * Vaa + (c * c) * Vcc;
        Veyy = (b * b) * Vbb + (jd * jd) * Vdd;
        const double Qu = ((b * b) * Vaa + (2.0 * (b * ja)) * Vab) + (ja * ja) * Vbb;
        const double Qv = ((jd * jd) * Vcc + (2.0 * (jd * c)) * Vcd) + (c * c) * Vdd;
        Vexy = 0.25 * (Qu + Qv);
    }
    q[0] = static_cast<float>(sqrt(Vaa));
    q[1] = static_cast<float>(sqrt(Vbb));
    q[2] = static_cast<float>(sqrt(Vcc));
    q[3] = static_cast<float>(sqrt(Vdd));
    q[4] = static_cast<float>(sqrt(Vaa + Vdd));
    q[5] = static_cast<float>(sqrt(Vbb + Vcc));
    q[6] = static_cast<float>(sqrt(Vexx));
    q[7] = static_cast<float>(sqrt(Veyy));
    q[8] = static_cast<float>(sqrt(Vexy));
}

template <int Order, bool Stats>
__global__ __launch_bounds__(kThreads) void node_strain_weighted_kernel(WeightedArgs in, WeightedStrainSums* __restrict__ partials,
                                                                       BatchArg batch)
{
    constexpr int K = Order == 2 ? 6 : 3;
    constexpr int kTile = kTileW * kTileH;
    __shared__ double tile_pu[kTile], tile_pv[kTile];
    __shared__ float tile_u[kTile], tile_v[kTile];
    __shared__ unsigned char tile_ok[kTile];
    __shared__ double park[K][kThreads];  // the u coefficients of a pass, while its v walk runs

    const size_t inst = batch_offset(batch);
    const int i = pixel_column();
    const int j = static_cast<int>(pixel_row(1, 0));
    const bool active = i < in.nw && j < in.nh;
    const size_t at = node_at(inst, active ? i : 0, active ? j : 0, in.npitch);

    const int m = in.window;
    const int tw = flow2d::kPixelBlockX + 2 * m, th = flow2d::kPixelBlockY + 2 * m;
    const int x0 = static_cast<int>(blockIdx.x) * flow2d::kPixelBlockX - m;
    const int y0 = static_cast<int>(blockIdx.y) * flow2d::kPixelBlockY - m;
    const int tid = threadIdx.y * flow2d::kPixelBlockX + threadIdx.x;
    // (tw * th <= kTile: the entry refuses a window beyond kMaxWindow)
    for (int t = tid; t < tw * th; t += kThreads) {
        const int ty = t / tw, tx = t - ty * tw;
        const int x = x0 + tx, y = y0 + ty;
        float u = 0.f, v = 0.f;
        double pu = 0.0, pv = 0.0;
        unsigned char flag = 0;
        if (x >= 0 && y >= 0 && x < in.nw && y < in.nh) {
            const size_t q = node_at(inst, x, y, in.npitch);
            u = in.u[q];
            v = in.v[q];
            if ((in.state ? in.state[q] >= in.min_state : true) && finite(u) && finite(v)) {
                const double su = static_cast<double>(in.su[q]), sv = static_cast<double>(in.sv[q]);
                const double vu = su * su + in.f2, vv = sv * sv + in.f2;
                flag = kUsable;
                if (vu > 0.0 && vv > 0.0 && vu < static_cast<double>(INFINITY) && vv < static_cast<double>(INFINITY)) {
                    flag = kUsable | kWeighable;
                    pu = 1.0 / vu;
                    pv = 1.0 / vv;
                }
            }
        }
        tile_u[t] = u;
        tile_v[t] = v;
        tile_pu[t] = pu;
        tile_pv[t] = pv;
        tile_ok[t] = flag;
    }
    __syncthreads();

    int reason = kCentre;
    double ga = 0.0, gb = 0.0, gc = 0.0, gd = 0.0;
    double Vaa = 0.0, Vab = 0.0, Vbb = 0.0, Vcc = 0.0, Vcd = 0.0, Vdd = 0.0;
    int n = 0, kept = 0;
    bool finished = false;  // the passes ran to the end: the node is valid, or sparse by what it kept
    double kept_r2 = 0.0, centre_r2 = 0.0;
    const int centre = (static_cast<int>(threadIdx.y) + m) * tw + static_cast<int>(threadIdx.x) + m;
    const unsigned char own = active ? tile_ok[centre] : 0;
    if (own & kWeighable) {
        const double uc = static_cast<double>(tile_u[centre]), vc = static_cast<double>(tile_v[centre]);
        const double t2 = in.t2;
        double cu[K], cv[K];
#pragma unroll
        for (int a = 0; a < K; ++a) cu[a] = cv[a] = 0.0;
        reason = kValid;
        // walk 2t + comp is the fit of u (comp 0) or v (comp 1) of pass t, weighted by the residuals of pass t - 1
        for (int walk = 0; walk < 2 * (in.passes + 1) && reason == kValid; ++walk) {
            const int t = walk >> 1;
            const bool second = (walk & 1) != 0;
            const float* tile_w = second ? tile_v : tile_u;
            const double* tile_p = second ? tile_pv : tile_pu;
            const double wc = second ? vc : uc;
            // the weighted monomial sums S[p][q] = sum of w * di^p dj^q, p + q <= 2 * Order, and the right-hand side
            double S[5][5];
#pragma unroll
            for (int p = 0; p < 5; ++p)
#pragma unroll
                for (int q = 0; q < 5; ++q) S[p][q] = 0.0;
            double rhs[K];
#pragma unroll
            for (int a = 0; a < K; ++a) rhs[a] = 0.0;
            int taps = 0;
            for (int dj = -m; dj <= m; ++dj) {
                const int row = centre + dj * tw;
                for (int di = -m; di <= m; ++di) {
                    if (!(tile_ok[row + di] & kWeighable)) continue;
                    int pi[5], pj[5];
                    pi[0] = pj[0] = 1;
#pragma unroll
                    for (int p = 1; p < 5; ++p) {
                        pi[p] = pi[p - 1] * di;
                        pj[p] = pj[p - 1] * dj;
                    }
                    double phi[K];
#pragma unroll
                    for (int a = 0; a < K; ++a) phi[a] = static_cast<double>(pi[exp_i(a)] * pj[exp_j(a)]);
                    double w = tile_p[row + di];
                    if (t > 0) {
                        const double wu = static_cast<double>(tile_u[row + di]) - uc;
                        const double wv = static_cast<double>(tile_v[row + di]) - vc;
                        double fu = 0.0, fv = 0.0;
#pragma unroll
                        for (int a = 0; a < K; ++a) {
                            fu += cu[a] * phi[a];
                            fv += cv[a] * phi[a];
                        }
                        const double ru = wu - fu, rv = wv - fv;
                        const double r2 = (ru * ru) * tile_pu[row + di] + (rv * rv) * tile_pv[row + di];
                        w = (t2 / (t2 + r2)) * w;
                    }
                    const double wx = static_cast<double>(tile_w[row + di]) - wc;
                    ++taps;
#pragma unroll
                    for (int p = 0; p <= 2 * Order; ++p)
#pragma unroll
                        for (int q = 0; p + q <= 2 * Order; ++q) S[p][q] += w * static_cast<double>(pi[p] * pj[q]);
#pragma unroll
                    for (int a = 0; a < K; ++a) rhs[a] += (w * phi[a]) * wx;
                }
            }
            if (walk == 0) {
                n = taps;
                if (!(n >= in.min_nodes)) {
                    reason = kSparse;
                    break;
                }
            }
            double L[K][K];
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int b = 0; b < K; ++b) L[a][b] = S[exp_i(a) + exp_i(b)][exp_j(a) + exp_j(b)];
            if (!factor<K>(L)) {
                reason = kDegenerate;
                break;
            }
            double cn[K];
            solve<K>(L, rhs, cn);
            if (t == in.passes) {
                // the columns 1 and 2 of the inverse: the covariance of the two slopes, in node units
                double e[K], x1[K], x2[K];
#pragma unroll
                for (int a = 0; a < K; ++a) e[a] = a == 1 ? 1.0 : 0.0;
                solve<K>(L, e, x1);
#pragma unroll
                for (int a = 0; a < K; ++a) e[a] = a == 2 ? 1.0 : 0.0;
                solve<K>(L, e, x2);
                const double ss = static_cast<double>(in.s) * static_cast<double>(in.s);
                if (!second) {
                    Vaa = x1[1] / ss;
                    Vab = x1[2] / ss;
                    Vbb = x2[2] / ss;
                } else {
                    Vcc = x1[1] / ss;
                    Vcd = x1[2] / ss;
                    Vdd = x2[2] / ss;
                }
            }
            if (!second) {
                // (a thread reads only what it wrote itself: no barrier)
#pragma unroll
                for (int a = 0; a < K; ++a) park[a][tid] = cn[a];
            } else {
#pragma unroll
                for (int a = 0; a < K; ++a) {
                    cu[a] = park[a][tid];
                    cv[a] = cn[a];
                }
            }
        }
        if (reason == kValid) {
            kept = n;
            if (in.residuals) {
                kept = 0;
                for (int dj = -m; dj <= m; ++dj) {
                    const int row = centre + dj * tw;
                    for (int di = -m; di <= m; ++di) {
                        if (!(tile_ok[row + di] & kWeighable)) continue;
                        int pi[3], pj[3];
                        pi[0] = pj[0] = 1;
#pragma unroll
                        for (int p = 1; p < 3; ++p) {
                            pi[p] = pi[p - 1] * di;
                            pj[p] = pj[p - 1] * dj;
                        }
                        const double wu = static_cast<double>(tile_u[row + di]) - uc;
                        const double wv = static_cast<double>(tile_v[row + di]) - vc;
                        double fu = 0.0, fv = 0.0;
#pragma unroll
                        for (int a = 0; a < K; ++a) {
                            const double phi = static_cast<double>(pi[exp_i(a)] * pj[exp_j(a)]);
                            fu += cu[a] * phi;
                            fv += cv[a] * phi;
                        }
                        const double ru = wu - fu, rv = wv - fv;
                        const double r2 = (ru * ru) * tile_pu[row + di] + (rv * rv) * tile_pv[row + di];
                        if (t2 > 0.0 ? r2 <= t2 : true) {
                            ++kept;
                            kept_r2 += r2;
                        }
                        if (di == 0 && dj == 0) centre_r2 = r2;
                    }
                }
            }
            finished = true;
            if (!(kept >= in.min_nodes)) {
                reason = kSparse;
            } else {
                const double s = static_cast<double>(in.s);
                ga = cu[1] / s;
                gb = cu[2] / s;
                gc = cv[1] / s;
                gd = cv[2] / s;
            }
        }
    }

    WeightedStrainSums acc;
    if (Stats) acc.clear();
    if (active) {
        const bool valid = reason == kValid;
        float q[9];
        quantities(ga, gb, gc, gd, in.measure, q);
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (in.out[k]) in.out[k][at] = valid ? q[k] : quiet_nan();
        const int rejected = n - kept;
        const bool suspect = in.t2 > 0.0 && !(centre_r2 <= in.t2);
        if (in.diag[0]) in.diag[0][at] = valid ? static_cast<float>(sqrt(kept_r2 / static_cast<double>(kept))) : quiet_nan();
        if (in.diag[1]) in.diag[1][at] = valid ? static_cast<float>(rejected) : quiet_nan();
        if (in.diag[2]) in.diag[2][at] = valid ? static_cast<float>(sqrt(centre_r2)) : quiet_nan();
        bool any_sigma = false;
#pragma unroll
        for (int k = 0; k < kSigmaPlanes; ++k) any_sigma = any_sigma || in.sig[k] != nullptr;
        if (any_sigma) {
            float sg[kSigmaPlanes];
            sigmas(ga, gb, gc, gd, Vaa, Vab, Vbb, Vcc, Vcd, Vdd, in.measure, sg);
#pragma unroll
            for (int k = 0; k < kSigmaPlanes; ++k)
                if (in.sig[k]) in.sig[k][at] = valid ? sg[k] : quiet_nan();
        }
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
            // (over the finished nodes, as in node_strain_robust.hip; the last over every node of the grid)
            acc.weighted[0] += finished && rejected > 0;
            acc.weighted[1] += finished ? static_cast<unsigned long long>(rejected) : 0ull;
            acc.weighted[2] += finished && suspect;
            acc.weighted[3] += own == kUsable;
        }
    }
    if (Stats) {
        // (every thread of the workgroup arrives here: the reduction holds a barrier)
        if (workgroup_reduce<flow2d::kPixelBlockY>(acc, threadIdx.x, threadIdx.y))
            partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}

template <int Order>
void launch_order(flow2d_context* ctx, const WeightedArgs& a, WeightedStrainSums* partials, size_t nw, size_t nh)
{
    const dim3 grid = flow2d::pixel_grid(ctx, nw, nh, 1), block = flow2d::pixel_block();
    if (partials)
        node_strain_weighted_kernel<Order, true><<<grid, block, 0, ctx->stream>>>(a, partials, flow2d::batch_arg(ctx, 1));
    else
        node_strain_weighted_kernel<Order, false><<<grid, block, 0, ctx->stream>>>(a, nullptr, flow2d::batch_arg(ctx, 1));
}

}  // namespace

extern "C" {

size_t flow2d_node_strain_weighted_workspace_bytes(size_t nw, size_t nh, size_t instances)
{
    if (nw == 0 || nh == 0 || instances == 0) return 0;
    return partial_blocks(nw, nh) * instances * sizeof(WeightedStrainSums);
}

int flow2d_node_strain_weighted_2d(flow2d_context* ctx, const float* node_u, const float* node_v, const float* node_state,
                                   const float* node_sigma_u, const float* node_sigma_v, size_t nw, size_t nh, size_t node_pitch_bytes,
                                   int spacing, int window, int order, int min_nodes, int min_state, int measure, float sigma_floor,
                                   float threshold, int iterations, const flow2d_deformation_planes* out,
                                   const flow2d_node_strain_diagnostics* diagnostics, const flow2d_strain_sigma_planes* sigmas,
                                   flow2d_deformation_stats* stats, void* workspace, size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const flow2d_deformation_planes p = out ? *out : flow2d_deformation_planes{};
    const flow2d_node_strain_diagnostics g = diagnostics ? *diagnostics : flow2d_node_strain_diagnostics{};
    const flow2d_strain_sigma_planes e = sigmas ? *sigmas : flow2d_strain_sigma_planes{};
    constexpr int kOut = 12 + kSigmaPlanes;
    float* const planes[kOut] = {p.divergence, p.vorticity,        p.dilatation,      p.exx,       p.eyy,       p.exy,      p.e1,
                                 p.e2,         p.max_shear,        g.residual,        g.rejected,  g.centre,    e.sigma_ux, e.sigma_uy,
                                 e.sigma_vx,   e.sigma_vy,         e.sigma_divergence, e.sigma_vorticity, e.sigma_exx, e.sigma_eyy,
                                 e.sigma_exy};
    if (!flow2d::planes_ok({node_u, node_v, node_sigma_u, node_sigma_v}, {node_state}, nw, nh, node_pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    for (float* q : planes)
        if (q && !flow2d::plane_args_ok(q, nw, nh, node_pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (spacing < 1 || spacing > FLOW2D_CORRELATION_MAX_SPACING || window < 1 || window > FLOW2D_NODE_STRAIN_MAX_WINDOW ||
        min_state < 0 || min_state > 1 || (measure != FLOW2D_STRAIN_SMALL && measure != FLOW2D_STRAIN_GREEN_LAGRANGE))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (order != 1 && order != 2) return FLOW2D_ERR_INVALID_ARGUMENT;
    const int k = order == 2 ? 6 : 3, side = 2 * window + 1;
    if (min_nodes < k || min_nodes > side * side) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(std::isfinite(sigma_floor) && sigma_floor >= 0.f) || !(std::isfinite(threshold) && threshold >= 0.f) || iterations < 0 ||
        iterations > FLOW2D_NODE_STRAIN_MAX_ITERATIONS || (iterations > 0 && !(threshold > 0.f)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    bool any = stats != nullptr;
    for (float* q : planes) any = any || q != nullptr;
    if (!any) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(stats) || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    if (stats && (!workspace || workspace_bytes < flow2d_node_strain_weighted_workspace_bytes(nw, nh, 1)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel reads its neighbours' inputs while their threads write: no written byte range may meet a read one or another
    // written one.  Without statistics the workspace is not touched and takes no part.
    auto aliased = [&](size_t span, size_t instances) {
        flow2d::ByteRange written[kOut + 2];
        for (int q = 0; q < kOut; ++q) written[q] = {planes[q], span};
        written[kOut] = {stats, instances * sizeof(flow2d_deformation_stats)};
        written[kOut + 1] = {stats ? workspace : nullptr, workspace_bytes};
        const flow2d::ByteRange read[] = {{node_u, span}, {node_v, span}, {node_state, span}, {node_sigma_u, span}, {node_sigma_v, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (stats && workspace_bytes < flow2d_node_strain_weighted_workspace_bytes(nw, nh, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    WeightedArgs a;
    a.u = node_u;
    a.v = node_v;
    a.state = node_state;
    a.su = node_sigma_u;
    a.sv = node_sigma_v;
    for (int q = 0; q < 9; ++q) a.out[q] = planes[q];
    for (int q = 0; q < 3; ++q) a.diag[q] = planes[9 + q];
    for (int q = 0; q < kSigmaPlanes; ++q) a.sig[q] = planes[12 + q];
    a.nw = static_cast<int>(nw);
    a.nh = static_cast<int>(nh);
    a.npitch = static_cast<int>(node_pitch_bytes / 4);
    a.s = spacing;
    a.window = window;
    a.min_nodes = min_nodes;
    a.measure = measure;
    a.passes = iterations;
    a.residuals = (threshold > 0.f || g.residual || g.rejected || g.centre) ? 1 : 0;
    a.min_state = static_cast<float>(min_state);
    a.f2 = static_cast<double>(sigma_floor) * static_cast<double>(sigma_floor);
    a.t2 = static_cast<double>(threshold) * static_cast<double>(threshold);
    WeightedStrainSums* partials = stats ? static_cast<WeightedStrainSums*>(workspace) : nullptr;
    if (order == 1)
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
