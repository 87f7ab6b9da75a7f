// The uncertainty of a first-order subset refinement's nodes for gfx950: flow2d_subset_uncertainty_2d, the covariance s2 * H^-1 of
// the Gauss-Newton least squares at the node's p, one node per wave.
//
// The normative definition is the one of flow2d_subset_uncertainty_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// The shape is subset_refine_masked.hip's: a wave owns a node and shares nothing with the other waves of its workgroup (no
// barrier), the frame-0 quantities live in the wave's slice of dynamic LDS, with a mask compacted to the list of usable pixels
// (the compaction is that file's, restated here because that file stays as it is), and every *sum over the subset* is the lane's
// partial in ascending m, from 0, then wave_sum's butterfly.  What differs: there is one evaluation and no iteration, so the
// wave keeps THREE pixel arrays and not four -- fx and fy are dead once H is summed (no b is formed), and the samples g take fx's
// place.  A wave's bytes are 3 * 8 * slice and, with a mask or without, the index list behind them: 5 880 at R = 7, 25 016 at
// R = 15.  The workgroup is sized so that the slices fit the 64 KB every launch may ask for without an attribute call: four
// waves up to R = 12 (65 120 bytes there), three at R = 13, two from R = 14.  The eight kernels compile to 143 .. 148 VGPRs and no
// scratch (profiles/subset_uncertainty/README.md): three waves per SIMD, twelve per CU, by registers -- which the 160 KB of a CU's
// LDS hold up to R = 10 (11 496 bytes a wave); beyond that the LDS is the limit, six waves per CU at R = 15.
// Every branch on a node's fate is uniform over the wave: the centre's mask value and the node's seven inputs are loaded by all
// lanes, Nv comes from ballots, the sums from the butterfly.  The six solves with the unit vectors run side by side, lane a on
// e_a, as one solve's instructions.
// The sample of the deformed frame and whether there is a mask are template parameters.  The node, the frame-0 fill, the window
// test and the plane checks are subset_node.hpp's and node_grid.hpp's, the samplers subset_sample.hpp's, the factorisation and the
// solve small_cholesky.hpp's.
#include <cmath>

#include "small_cholesky.hpp"
#include "subset_node.hpp"

namespace {

constexpr int kUncertaintyCounts = 7;  // nodes, evaluated, skipped, masked, outside, flat, thin
enum Fate { kFateEvaluated = 0, kFateSkipped, kFateMasked, kFateOutside, kFateFlat, kFateThin };

struct UncertaintyArgs {
    const float *f0, *f1, *mask;
    const float* p[6];  // u, ux, uy, v, vx, vy
    const float* state;
    float* out[8];               // sigma_u, sigma_v, rho, sigma_ux, sigma_uy, sigma_vx, sigma_vy, noise; null = absent
    unsigned long long* record;  // eight words per instance, or null
    int w, h, pitch;             // the frames and the mask; pitch in floats
    int nw, nh, npitch;          // the node planes
    int r, s, R;
    int min_state, min_pixels;
    unsigned slice;       // doubles of one of a wave's three LDS arrays: N rounded up to a multiple of 2
    unsigned wave_bytes;  // the three arrays and the index list, a multiple of 8
};

struct UncertaintyNode : SubsetNode {  // (g shares fx's array; with a mask the arrays are compacted: element m is pixel index[m])
    const float* mask;
    unsigned short* index;  // the usable pixels' k in ascending order
    int nv;                 // the usable pixels
};

// *Excluded* of flow2d_subset_refine_masked_2d: 1 means "do not use", and a NaN is excluded.
template <typename Offset>
__device__ __forceinline__ bool excluded_at(const float* mask, int x, int y, int pitch)
{
    return !(load_at(mask, pixel_offset<Offset>(x, y, pitch)) < 0.5f);
}

template <bool kMasked>
__device__ __forceinline__ int pixel_of(const UncertaintyNode& nd, int m)
{
    if constexpr (kMasked)
        return nd.index[m];
    else
        return m;
}

// The list of usable pixels into nd.index, in ascending k, and their f (into fd), fx and fy into the same slots; returns Nv, the
// same in every lane.  subset_refine_masked.hip's compaction: the mask's five loads and frame 0's five go out together, a slot is
// filled by another lane than the one that reads it afterwards, and the wave barrier keeps those reads below these writes.
template <typename Offset>
__device__ __forceinline__ int compact_usable(const UncertaintyNode& nd)
{
    const int left = nd.cx - nd.R, top = nd.cy - nd.R;
    int nv = 0;
    for (int base = 0; base < nd.n; base += 64) {
        const int k = base + nd.lane;
        bool usable = false;
        double f = 0.0, fx = 0.0, fy = 0.0;
        if (k < nd.n) {
            const int ky = k / nd.side, kx = k - ky * nd.side;
            const int x = left + kx, y = top + ky;
            const int xp = min(x + 1, nd.w - 1), xm = max(x - 1, 0), yp = min(y + 1, nd.h - 1), ym = max(y - 1, 0);
            const bool e0 = excluded_at<Offset>(nd.mask, x, y, nd.pitch), e1 = excluded_at<Offset>(nd.mask, xp, y, nd.pitch),
                       e2 = excluded_at<Offset>(nd.mask, xm, y, nd.pitch), e3 = excluded_at<Offset>(nd.mask, x, yp, nd.pitch),
                       e4 = excluded_at<Offset>(nd.mask, x, ym, nd.pitch);
            usable = !(e0 | e1 | e2 | e3 | e4);
            f = sample_at<Offset>(nd.f0, x, y, nd.pitch);
            fx = (sample_at<Offset>(nd.f0, xp, y, nd.pitch) - sample_at<Offset>(nd.f0, xm, y, nd.pitch)) * 0.5;
            fy = (sample_at<Offset>(nd.f0, x, yp, nd.pitch) - sample_at<Offset>(nd.f0, x, ym, nd.pitch)) * 0.5;
        }
        const unsigned long long bits = __ballot(usable);
        if (usable) {
            const int slot = nv + __popcll(bits & ((1ull << nd.lane) - 1ull));  // (slot <= k < N)
            nd.index[slot] = static_cast<unsigned short>(k);
            nd.fd[slot] = f;
            nd.fx[slot] = fx;
            nd.fy[slot] = fy;
        }
        nv += __popcll(bits);
    }
    __builtin_amdgcn_wave_barrier();
    return nv;
}

// What the node's covariance is made of: s2 and the entries of H^-1 the outputs read.
struct Covariance {
    double s2;
    double diagonal[6];  // x_a[a]
    double x03;          // x_0[3]
};

// The node from the frame-0 quantities in LDS on, over the nd.nv usable pixels, steps 6 .. 10 of the header.  p holds the six
// inputs.  Every lane of the wave returns the same values.
template <typename Offset, typename Sampler, bool kMasked>
__device__ __forceinline__ Fate evaluate_node(const UncertaintyNode& nd, const double (&p)[6], Covariance& c)
{
    const double count = static_cast<double>(nd.nv);
    const int left = nd.cx - nd.R, top = nd.cy - nd.R;

    double sum_f = 0.0;
    for (int m = nd.lane; m < nd.nv; m += 64) sum_f += nd.fd[m];
    const double fm = wave_sum(sum_f) / count;

    double df2 = 0.0;
    double hs[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) hs[i] = 0.0;
    for (int m = nd.lane; m < nd.nv; m += 64) {
        const double fd = nd.fd[m] - fm;
        nd.fd[m] = fd;
        df2 += fd * fd;
        const int k = pixel_of<kMasked>(nd, m);
        const int ky = k / nd.side, kx = k - ky * nd.side;
        const double xi = static_cast<double>(kx - nd.R), eta = static_cast<double>(ky - nd.R);
        const double fx = nd.fx[m], fy = nd.fy[m];
        const double J[6] = {fx, fx * xi, fx * eta, fy, fy * xi, fy * eta};
        int at = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) hs[at++] += J[i] * J[j];
    }
    df2 = wave_sum(df2);
    if (!(df2 > 0.0)) return kFateFlat;
    const double df = sqrt(df2);
    double L[6][6];
    {
        int at = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) L[i][j] = wave_sum(hs[at++]);
    }
    if (!factor<6>(L)) return kFateFlat;

    // 7, 8: positions and samples (into fx's array: H is summed, fx and fy are not read again)
    const double xmax = static_cast<double>(nd.w - 1), ymax = static_cast<double>(nd.h - 1);
    unsigned outside = 0;
    double sum_g = 0.0;
    for (int m = nd.lane; m < nd.nv; m += 64) {
        const int k = pixel_of<kMasked>(nd, m);
        const int ky = k / nd.side, kx = k - ky * nd.side;
        const double xi = static_cast<double>(kx - nd.R), eta = static_cast<double>(ky - nd.R);
        const double X = static_cast<double>(left + kx) + ((p[0] + p[1] * xi) + p[2] * eta);
        const double Y = static_cast<double>(top + ky) + ((p[3] + p[4] * xi) + p[5] * eta);
        double g = 0.0;
        if (X >= 0.0 && X <= xmax && Y >= 0.0 && Y <= ymax)
            g = Sampler::template sample<Offset>(nd, X, Y);
        else
            outside = 1;
        nd.g[m] = g;
        sum_g += g;
    }
    if (wave_sum(outside) != 0) return kFateOutside;
    const double gm = wave_sum(sum_g) / count;
    double dg2 = 0.0;
    for (int m = nd.lane; m < nd.nv; m += 64) {
        const double gd = nd.g[m] - gm;
        nd.g[m] = gd;
        dg2 += gd * gd;
    }
    dg2 = wave_sum(dg2);
    if (!(dg2 > 0.0)) return kFateFlat;
    const double q = df / sqrt(dg2);
    // 9: the residual's sum of squares over N - 8 degrees of freedom
    double ss = 0.0;
    for (int m = nd.lane; m < nd.nv; m += 64) {
        const double res = nd.fd[m] - q * nd.g[m];
        ss += res * res;
    }
    c.s2 = wave_sum(ss) / static_cast<double>(nd.nv - 8);
    // 10: the columns of H^-1, one solve for all six: lane a (and every lane a + 6 n) solves for e_a -- the operations of
    // Solve(e_a) one by one, so the bits are those of six solves in turn at a sixth of the instructions --, and lanes 0 .. 5
    // hand their x_a[a] to everybody
    const int a = nd.lane % 6;
    double e[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = i == a ? 1.0 : 0.0;
    solve<6>(L, e, x);
    double own = x[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) own = a == i ? x[i] : own;
#pragma unroll
    for (int k = 0; k < 6; ++k) c.diagonal[k] = __shfl(own, k, 64);
    c.x03 = __shfl(x[3], 0, 64);
    return kFateEvaluated;
}

// A wave's node from its inputs to its outputs.
template <typename Offset, typename Sampler, bool kMasked>
__global__ __launch_bounds__(64 * kSubsetMaxWaves) void subset_uncertainty_kernel(UncertaintyArgs a, BatchArg batch)
{
    extern __shared__ __attribute__((aligned(16))) double s_uncertainty[];

    const size_t inst = batch_offset(batch);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node = blockIdx.x * (blockDim.x >> 6) + wave;
    if (node >= a.nw * a.nh) return;  // (no barrier anywhere: the last workgroup's surplus waves leave)
    const int jn = node / a.nw, in = node - jn * a.nw;

    UncertaintyNode nd;
    nd.f0 = a.f0 + inst;
    nd.f1 = a.f1 + inst;
    nd.mask = kMasked ? a.mask + inst : nullptr;
    nd.fd = s_uncertainty + static_cast<size_t>(wave) * (a.wave_bytes / sizeof(double));
    nd.fx = nd.fd + a.slice;
    nd.fy = nd.fx + a.slice;
    nd.g = nd.fx;
    nd.index = reinterpret_cast<unsigned short*>(nd.fy + a.slice);
    nd.w = a.w;
    nd.h = a.h;
    nd.pitch = a.pitch;
    nd.cx = a.r + in * a.s;
    nd.cy = a.r + jn * a.s;
    nd.R = a.R;
    nd.side = 2 * a.R + 1;
    nd.n = nd.side * nd.side;
    nd.nv = 0;
    nd.lane = lane;

    const size_t at = node_at(inst, in, jn, a.npitch);
    float in_p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) in_p[i] = a.p[i][at];
    const float state = a.state[at];
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = static_cast<double>(in_p[i]);
    Covariance c = {};
    Fate fate;
    // (the centre lies inside the frame: the grid does; every lane loads the same words, so the branches are the wave's)
    if (kMasked && excluded_at<Offset>(nd.mask, nd.cx, nd.cy, nd.pitch))
        fate = kFateMasked;
    else if (!(state >= static_cast<float>(a.min_state)) ||
             !(finite(in_p[0]) && finite(in_p[1]) && finite(in_p[2]) && finite(in_p[3]) && finite(in_p[4]) && finite(in_p[5])))
        fate = kFateSkipped;
    else if (!subset_inside_frame(nd.cx, nd.cy, nd.R, a.w, a.h))
        fate = kFateOutside;
    else {
        if constexpr (kMasked) {
            nd.nv = compact_usable<Offset>(nd);
        } else {
            fill_frame_0<Offset>(nd);
            nd.nv = nd.n;
        }
        if (kMasked && !(nd.nv >= a.min_pixels))
            fate = kFateMasked;
        else if (!(nd.nv >= 9))
            fate = kFateThin;
        else
            fate = evaluate_node<Offset, Sampler, kMasked>(nd, p, c);
    }
    if (lane != 0) return;

    float out[8];
    if (fate == kFateEvaluated) {
        out[0] = static_cast<float>(sqrt(c.s2 * c.diagonal[0]));
        out[1] = static_cast<float>(sqrt(c.s2 * c.diagonal[3]));
        out[2] = static_cast<float>(c.x03 / sqrt(c.diagonal[0] * c.diagonal[3]));
        out[3] = static_cast<float>(sqrt(c.s2 * c.diagonal[1]));
        out[4] = static_cast<float>(sqrt(c.s2 * c.diagonal[2]));
        out[5] = static_cast<float>(sqrt(c.s2 * c.diagonal[4]));
        out[6] = static_cast<float>(sqrt(c.s2 * c.diagonal[5]));
        out[7] = static_cast<float>(sqrt(c.s2));
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = quiet_nan();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (a.out[i]) a.out[i][at] = out[i];
    if (a.record) {
        const unsigned counts[kUncertaintyCounts] = {1u, fate == kFateEvaluated, fate == kFateSkipped, fate == kFateMasked,
                                                     fate == kFateOutside, fate == kFateFlat, fate == kFateThin};
        add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
    }
}

template <typename Offset, typename Sampler>
void launch(const flow2d_context* ctx, const UncertaintyArgs& a, unsigned waves)
{
    const dim3 grid(flow2d::div_up(static_cast<size_t>(a.nw) * a.nh, waves), 1, flow2d::batch_z(ctx, 1)), block(64 * waves);
    if (a.mask != nullptr)
        subset_uncertainty_kernel<Offset, Sampler, true><<<grid, block, waves * a.wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    else
        subset_uncertainty_kernel<Offset, Sampler, false><<<grid, block, waves * a.wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
}

}  // namespace

extern "C" {

int flow2d_subset_uncertainty_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, int interpolation, size_t width,
                                 size_t height, size_t pitch_bytes, const float* node_u, const float* node_v, const float* node_ux,
                                 const float* node_uy, const float* node_vx, const float* node_vy, const float* node_state, size_t nw,
                                 size_t nh, size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int min_state,
                                 const float* mask, int min_pixels, float* out_sigma_u, float* out_sigma_v, float* out_rho,
                                 float* out_sigma_ux, float* out_sigma_uy, float* out_sigma_vx, float* out_sigma_vy, float* out_noise,
                                 flow2d_uncertainty_record* record)
{
    using namespace flow2d;
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!planes_ok({frame_0, frame_1}, {mask}, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if ((interpolation != 0 && interpolation != 1) || (min_state != 0 && min_state != 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const int shared = subset_refine_args_status(width, height, nw, nh, grid_radius, spacing, 1, subset_radius, 1, 0.f, {}, nullptr);
    if (shared == FLOW2D_ERR_INVALID_ARGUMENT || !record_aligned(record)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const long long pixels = (2LL * subset_radius + 1) * (2LL * subset_radius + 1);
    if (mask != nullptr && (min_pixels < FLOW2D_SUBSET_MIN_PIXELS || min_pixels > pixels)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const int gradient_sigmas = (out_sigma_ux != nullptr) + (out_sigma_uy != nullptr) + (out_sigma_vx != nullptr) + (out_sigma_vy != nullptr);
    if (gradient_sigmas != 0 && gradient_sigmas != 4) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!planes_ok({node_u, node_v, node_ux, node_uy, node_vx, node_vy, node_state, out_sigma_u, out_sigma_v},
                   {out_rho, out_sigma_ux, out_sigma_uy, out_sigma_vx, out_sigma_vy, out_noise}, nw, nh, node_pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (shared != FLOW2D_OK) return shared;  // (the node count)
    float* const outs[8] = {out_sigma_u, out_sigma_v, out_rho, out_sigma_ux, out_sigma_uy, out_sigma_vx, out_sigma_vy, out_noise};
    const float* const nodes[7] = {node_u, node_ux, node_uy, node_v, node_vx, node_vy, node_state};
    // the kernel reads frames, mask and nodes while other waves write: no written byte range may meet a read one or another written one
    auto aliased = [&](size_t frame_span, size_t node_span, size_t instances) {
        ByteRange written[9], read[10];
        for (int i = 0; i < 8; ++i) written[i] = {outs[i], node_span};
        written[8] = {record, instances * sizeof(flow2d_uncertainty_record)};
        for (int i = 0; i < 7; ++i) read[i] = {nodes[i], node_span};
        read[7] = {frame_0, frame_span};
        read[8] = {frame_1, frame_span};
        read[9] = {mask, frame_span};
        return any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(batch_span(ctx, height * pitch_bytes), batch_span(ctx, nh * node_pitch_bytes), ctx->batch_count))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(clear_records(ctx, record));

    UncertaintyArgs a = {};
    a.f0 = frame_0;
    a.f1 = frame_1;
    a.mask = mask;
    for (int i = 0; i < 6; ++i) a.p[i] = nodes[i];
    a.state = node_state;
    for (int i = 0; i < 8; ++i) a.out[i] = outs[i];
    a.record = reinterpret_cast<unsigned long long*>(record);
    a.w = static_cast<int>(width);
    a.h = static_cast<int>(height);
    a.pitch = static_cast<int>(pitch_bytes / 4);
    a.nw = static_cast<int>(nw);
    a.nh = static_cast<int>(nh);
    a.npitch = static_cast<int>(node_pitch_bytes / 4);
    a.r = grid_radius;
    a.s = spacing;
    a.R = subset_radius;
    a.min_state = min_state;
    a.min_pixels = min_pixels;
    a.slice = (static_cast<unsigned>(pixels) + 1u) & ~1u;                                                   // at most 962
    a.wave_bytes = 3u * a.slice * sizeof(double) + ((2u * static_cast<unsigned>(pixels + 1) + 7u) & ~7u);  // at most 25 016
    const unsigned waves = std::min<unsigned>(kSubsetMaxWaves, kSubsetLdsBytes / a.wave_bytes);
    // (the largest offset a lane forms into a frame or the mask is below height * pitch_bytes; the node planes are addressed in 64 bits)
    launch_by_span(height * pitch_bytes, [&](auto offset) {
        if (interpolation == 1)
            launch<decltype(offset), BSpline>(ctx, a, waves);
        else
            launch<decltype(offset), CatmullRom>(ctx, a, waves);
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
