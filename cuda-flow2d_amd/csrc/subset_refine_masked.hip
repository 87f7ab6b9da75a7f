// Masked subset refinement of correlation nodes for gfx950: flow2d_subset_refine_from_2d on the pixels of a region of interest,
// one node per wave.
//
// The normative definition is the one of flow2d_subset_refine_masked_2d in flow2d_c_abi.h, in IEEE double.  Built
// -ffp-contract=off.
//
// The shape is subset_refine.hip's: a wave owns a node and shares nothing with the other waves of its workgroup (no barrier), and
// what is constant over the iterations -- fd, fx, fy -- and the samples g of the current iteration live in the wave's slice of
// dynamic LDS.  What is new is a compaction at the start of the node: per chunk of 64 pixels every lane evaluates *usable* for
// pixel k = chunk + lane from its five mask loads, __ballot gives the chunk's bits, the lane's slot is the running base plus the
// count of the lower lanes' bits, and k goes as 16 bits into an index list behind the four double arrays (two more bytes of LDS
// per pixel), f, fx and fy of the pixel into the same slot of theirs.  Every later loop runs m = lane, lane + 64, ... < Nv over
// the compacted arrays, each element then read and written by its own lane only, so a *sum over the subset* is the lane's partial
// in ascending m, from 0, then wave_sum's butterfly -- with nothing excluded the list is k itself and every bit is
// flow2d_subset_refine_from_2d's; a node at the specimen's edge runs fewer pixels than an interior one.  The compaction is the one
// place where a lane writes what another lane reads: the LDS serves a wave's accesses in order, and
// __builtin_amdgcn_wave_barrier keeps the compiler from moving the reads above the writes.
// Every branch on a node's state is uniform over the wave: the centre's mask value is loaded by all lanes, Nv comes from ballots.
// The workgroup is sized so that the slices fit the 64 KB every launch may ask for without an attribute call: four waves up to
// R = 10 (15 032 bytes per wave there), three at R = 11 and 12, two from R = 13 (32 712 bytes at R = 15).
// The sample of the deformed frame and whether there is a mask are template parameters: <CatmullRom, true> is
// flow2d_subset_refine_masked_2d; <BSpline, true> and <BSpline, false> are flow2d_subset_refine_spline_2d on frame 1's coefficients
// (subset_sample.hpp), with and without a mask.  Without one the compaction is compiled out -- no mask loads, no ballots, no index
// list read: the list is k itself, element m is pixel m, and the sums are those of a mask that excludes nothing, bit for bit.
// <CatmullRom, false> is not instantiated: it gives subset_refine.hip's bytes, but that file's kernel is the faster one at R = 15
// (profiles/subset_unified/README.md).  The node, the frame-0 fill, the window test and the host body are subset_node.hpp's, the
// samplers subset_sample.hpp's, the factorisation and the solve small_cholesky.hpp's.
#include <cmath>
#include <type_traits>

#include "small_cholesky.hpp"
#include "subset_node.hpp"

namespace {

constexpr int kMaskedCounts = kSubsetCounts + 1;  // the seven counts of flow2d_subset_record and the masked nodes

struct MaskedArgs {
    const float *f0, *f1, *mask;
    const float *u0, *v0;
    const float *ux0, *uy0, *vx0, *vy0;  // the start's gradients: all or none
    float *u, *v, *ux, *uy, *vx, *vy;    // the gradient planes: all or none
    float *score, *state;                // null = absent
    unsigned long long* record;          // eight words per instance, or null
    int w, h, pitch;                     // the frames and the mask; pitch in floats
    int nw, nh, npitch;                  // the node planes
    int r, s, R, K;
    int min_pixels;
    unsigned slice;       // doubles of one of a wave's four LDS arrays: N rounded up to a multiple of 2
    unsigned wave_bytes;  // the four arrays and the index list, a multiple of 8
    double epsilon, max_shift, max_gradient;
};

struct MaskedNode : SubsetNode {  // (the LDS arrays compacted: element m belongs to pixel index[m])
    const float* mask;
    unsigned short* index;  // the usable pixels' k in ascending order
    int nv;                 // the usable pixels
};

// *Excluded* of the header: 1 means "do not use", and a NaN is excluded.
template <typename Offset>
__device__ __forceinline__ bool excluded_at(const float* mask, int x, int y, int pitch)
{
    return !(load_at(mask, pixel_offset<Offset>(x, y, pitch)) < 0.5f);
}

// Pixel k of element m of the list.
template <bool kMasked>
__device__ __forceinline__ int pixel_of(const MaskedNode& nd, int m)
{
    if constexpr (kMasked)
        return nd.index[m];
    else
        return m;
}

// J of the header for element m of the list, pixel k.
__device__ __forceinline__ void jacobian(const MaskedNode& nd, int m, int k, double (&J)[6])
{
    const int ky = k / nd.side, kx = k - ky * nd.side;
    const double xi = static_cast<double>(kx - nd.R), eta = static_cast<double>(ky - nd.R);
    const double fx = nd.fx[m], fy = nd.fy[m];
    J[0] = fx;
    J[1] = fx * xi;
    J[2] = fx * eta;
    J[3] = fy;
    J[4] = fy * xi;
    J[5] = fy * eta;
}

// The list of usable pixels into nd.index, in ascending k, and their frame-0 quantities f (into fd), fx and fy into the same slots;
// returns Nv, the same in every lane.  The subset lies inside the frame (the frame-0 window test has passed), so the pixel itself
// needs no clamp and its stencil the header's.  The mask's five loads and frame 0's five go out together, for every pixel of the
// subset, and only the usable ones are kept: one trip to memory per chunk, where the mask first and frame 0 afterwards would be
// two (at R = 15, one wave per SIMD, nothing hides a trip: profiles/subset_mask/README.md).  A slot belongs to another lane than the one
// that fills it here; every later loop reads and writes a lane's own slots.
template <typename Offset>
__device__ __forceinline__ int compact_usable(const MaskedNode& nd)
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
            // (| and not ||: all five loads are issued, none waits for the one before it)
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
    __builtin_amdgcn_wave_barrier();  // the reads of the slots below stay below these writes
    return nv;
}

// The node from the frame-0 quantities compact_usable left in LDS on, over the nd.nv usable pixels: the state, with p, the last c
// and the iterations begun.  p = (u, ux, uy, v, vx, vy) holds the start on entry.  Every lane of the wave returns the same values.
template <typename Offset, typename Sampler, bool kMasked>
__device__ __forceinline__ int refine_node(const MaskedNode& nd, const MaskedArgs& a, double (&p)[6], double& score, unsigned& iterations)
{
    const double u0 = p[0], v0 = p[3];
    const double count = static_cast<double>(nd.nv);
    const int left = nd.cx - nd.R, top = nd.cy - nd.R;

    // frame 0: the mean of f, a lane's partial over its own slots in ascending m
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
        double J[6];
        jacobian(nd, m, pixel_of<kMasked>(nd, m), J);
        int at = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) hs[at++] += J[i] * J[j];
    }
    df2 = wave_sum(df2);
    if (!(df2 > 0.0)) return kStateFlat;
    const double df = sqrt(df2);
    double L[6][6];  // H's lower triangle, replaced column by column by the factor's
    {
        int at = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) L[i][j] = wave_sum(hs[at++]);
    }
    if (!factor<6>(L)) return kStateFlat;

    const double xmax = static_cast<double>(nd.w - 1), ymax = static_cast<double>(nd.h - 1);
    const double radius = static_cast<double>(nd.R);
    for (int n = 1; n <= a.K; ++n) {
        iterations = static_cast<unsigned>(n);
        // 1, 2: positions and samples, of the usable pixels only
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
        if (wave_sum(outside) != 0) return kStateStrayed;
        // 3: the residual and the step
        const double gm = wave_sum(sum_g) / count;
        double dg2 = 0.0, sfg = 0.0;
        for (int m = nd.lane; m < nd.nv; m += 64) {
            const double gd = nd.g[m] - gm;
            nd.g[m] = gd;
            dg2 += gd * gd;
            sfg += nd.fd[m] * gd;
        }
        dg2 = wave_sum(dg2);
        sfg = wave_sum(sfg);
        if (!(dg2 > 0.0)) return kStateFlat;
        const double dg = sqrt(dg2);
        score = sfg / (df * dg);
        const double q = df / dg;
        double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int m = nd.lane; m < nd.nv; m += 64) {
            const double res = nd.fd[m] - q * nd.g[m];
            double J[6];
            jacobian(nd, m, pixel_of<kMasked>(nd, m), J);
#pragma unroll
            for (int i = 0; i < 6; ++i) b[i] += J[i] * res;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) b[i] = wave_sum(b[i]);
        double x[6];
        solve<6>(L, b, x);
        const double du = -x[0], dux = -x[1], duy = -x[2], dv = -x[3], dvx = -x[4], dvy = -x[5];
        // 4: p <- W(p) o W(dp)^-1
        const double ma = 1.0 + dux, mb = duy, mc = dvx, md = 1.0 + dvy;
        const double det = ma * md - mb * mc;
        if (!(fabs(det) > 1e-12)) return kStateStrayed;
        const double ia = md / det, ib = (-mb) / det, ic = (-mc) / det, id = ma / det;
        const double tx = -(ia * du + ib * dv), ty = -(ic * du + id * dv);
        const double p11 = 1.0 + p[1], p12 = p[2], p21 = p[4], p22 = 1.0 + p[5];
        p[0] = (p11 * tx + p12 * ty) + p[0];
        p[3] = (p21 * tx + p22 * ty) + p[3];
        p[1] = (p11 * ia + p12 * ic) - 1.0;
        p[2] = p11 * ib + p12 * id;
        p[4] = p21 * ia + p22 * ic;
        p[5] = (p21 * ib + p22 * id) - 1.0;
        // 5: the bounds, then convergence
        if (!(fabs(p[0] - u0) <= a.max_shift && fabs(p[3] - v0) <= a.max_shift && fabs(p[1]) <= a.max_gradient &&
              fabs(p[2]) <= a.max_gradient && fabs(p[4]) <= a.max_gradient && fabs(p[5]) <= a.max_gradient))
            return kStateStrayed;
        const double step = sqrt(((((du * du + (radius * dux) * (radius * dux)) + (radius * duy) * (radius * duy)) + dv * dv) +
                                  (radius * dvx) * (radius * dvx)) + (radius * dvy) * (radius * dvy));
        if (step < a.epsilon) return n;
    }
    return 0;
}

// A wave's node from its inputs to its outputs.
template <typename Offset, typename Sampler, bool kMasked>
__global__ __launch_bounds__(64 * kSubsetMaxWaves) void subset_refine_masked_kernel(MaskedArgs a, BatchArg batch)
{
    extern __shared__ __attribute__((aligned(16))) double s_masked[];

    const size_t inst = batch_offset(batch);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node = blockIdx.x * (blockDim.x >> 6) + wave;
    if (node >= a.nw * a.nh) return;  // (no barrier anywhere: the last workgroup's surplus waves leave)
    const int jn = node / a.nw, in = node - jn * a.nw;

    MaskedNode nd;
    nd.f0 = a.f0 + inst;
    nd.f1 = a.f1 + inst;
    nd.mask = kMasked ? a.mask + inst : nullptr;
    nd.fd = s_masked + static_cast<size_t>(wave) * (a.wave_bytes / sizeof(double));
    nd.fx = nd.fd + a.slice;
    nd.fy = nd.fx + a.slice;
    nd.g = nd.fy + a.slice;
    nd.index = reinterpret_cast<unsigned short*>(nd.g + a.slice);
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
    const float u0 = a.u0[at], v0 = a.v0[at];
    float g0[4] = {0.f, 0.f, 0.f, 0.f};  // ux0, uy0, vx0, vy0; absent: 0, the start of flow2d_subset_refine_2d
    if (a.ux0) {
        g0[0] = a.ux0[at];
        g0[1] = a.uy0[at];
        g0[2] = a.vx0[at];
        g0[3] = a.vy0[at];
    }
    double p[6] = {static_cast<double>(u0), static_cast<double>(g0[0]), static_cast<double>(g0[1]),
                   static_cast<double>(v0), static_cast<double>(g0[2]), static_cast<double>(g0[3])};
    double score = 0.0;
    unsigned iterations = 0;
    int state;
    // (the centre lies inside the frame: the grid does; every lane loads the same word, so the branch is the wave's)
    if (kMasked && excluded_at<Offset>(nd.mask, nd.cx, nd.cy, nd.pitch))
        state = kStateMasked;
    else if (!(finite(u0) && finite(v0) && finite(g0[0]) && finite(g0[1]) && finite(g0[2]) && finite(g0[3])))
        state = kStateNoInput;
    else if (!subset_inside_frame(nd.cx, nd.cy, nd.R, a.w, a.h))
        state = kStateStrayed;
    else {
        if constexpr (kMasked) {
            nd.nv = compact_usable<Offset>(nd);
        } else {  // every pixel is usable and slot k is pixel k's, filled by the lane that reads it afterwards
            fill_frame_0<Offset>(nd);
            nd.nv = nd.n;
        }
        if (kMasked && !(nd.nv >= a.min_pixels))
            state = kStateMasked;
        else
            state = refine_node<Offset, Sampler, kMasked>(nd, a, p, score, iterations);
    }
    if (lane != 0) return;

    float out[6], out_score = 0.f;
    if (state >= 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = static_cast<float>(p[i]);
        out_score = static_cast<float>(score);
    } else if (state == kStateNoInput || state == kStateMasked) {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = quiet_nan();
    } else {  // flat and strayed hand the whole start back
        out[0] = u0;
        out[1] = g0[0];
        out[2] = g0[1];
        out[3] = v0;
        out[4] = g0[2];
        out[5] = g0[3];
    }
    a.u[at] = out[0];
    a.v[at] = out[3];
    if (a.ux) {
        a.ux[at] = out[1];
        a.uy[at] = out[2];
        a.vx[at] = out[4];
        a.vy[at] = out[5];
    }
    if (a.score) a.score[at] = out_score;
    if (a.state) a.state[at] = static_cast<float>(state);
    if (a.record) {
        const unsigned counts[kMaskedCounts] = {1u, state >= 1, state == 0, state == kStateStrayed, state == kStateFlat,
                                                state == kStateNoInput, iterations, state == kStateMasked};
        add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
    }
}

// The body of both entries; frame_1 is the frame for CatmullRom and its coefficients for BSpline.  mask may be null (the spline
// entry's; flow2d_subset_refine_masked_2d forwards such a call before it gets here): min_pixels is then not looked at.
template <typename Sampler>
int subset_refine_masked(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                         size_t pitch_bytes, const float* node_u0, const float* node_v0, const float* node_ux0, const float* node_uy0,
                         const float* node_vx0, const float* node_vy0, size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius,
                         int spacing, int subset_radius, int max_iterations, float epsilon, float max_shift, float max_gradient,
                         const float* mask, int min_pixels, float* out_u, float* out_v, float* out_ux, float* out_uy, float* out_vx,
                         float* out_vy, float* out_score, float* out_state, flow2d_subset_record* record)
{
    const long long pixels = (2LL * subset_radius + 1) * (2LL * subset_radius + 1);
    if (mask != nullptr && (min_pixels < FLOW2D_SUBSET_MIN_PIXELS || min_pixels > pixels)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float* const starts[6] = {node_u0, node_ux0, node_uy0, node_v0, node_vx0, node_vy0};
    float* const outs[6] = {out_u, out_ux, out_uy, out_v, out_vx, out_vy};
    flow2d::SubsetWaves lds;  // (behind the four arrays the index list, two bytes per pixel: at most 1 928)
    const int status = flow2d::subset_refine_enter(ctx, frame_0, frame_1, mask, width, height, pitch_bytes, starts, outs, 6, out_score,
                                                   out_state, record, nw, nh, node_pitch_bytes, grid_radius, spacing, 1, subset_radius,
                                                   max_iterations, epsilon, {max_shift, max_gradient},
                                                   (2u * static_cast<unsigned>(pixels + 1) + 7u) & ~7u, lds);
    if (status != FLOW2D_OK) return status;
    const unsigned slice = lds.slice, wave_bytes = lds.wave_bytes, waves = lds.waves;
    const MaskedArgs a = {frame_0, frame_1, mask, node_u0, node_v0, node_ux0, node_uy0, node_vx0, node_vy0,
                          out_u, out_v, out_ux, out_uy, out_vx, out_vy, out_score, out_state,
                          reinterpret_cast<unsigned long long*>(record),
                          static_cast<int>(width), static_cast<int>(height), static_cast<int>(pitch_bytes / 4),
                          static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                          grid_radius, spacing, subset_radius, max_iterations, min_pixels, slice, wave_bytes,
                          static_cast<double>(epsilon), static_cast<double>(max_shift), static_cast<double>(max_gradient)};
    // (the largest offset a lane forms into a frame or the mask is below height * pitch_bytes; the node planes are addressed in 64 bits)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        const dim3 grid(flow2d::div_up(nw * nh, waves), 1, flow2d::batch_z(ctx, 1)), block(64 * waves);
        if (mask != nullptr)
            subset_refine_masked_kernel<decltype(offset), Sampler, true><<<grid, block, waves * wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
        else if constexpr (std::is_same_v<Sampler, BSpline>)  // (the Catmull-Rom entry forwards a call without a mask: no such kernel)
            subset_refine_masked_kernel<decltype(offset), Sampler, false><<<grid, block, waves * wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // namespace

extern "C" {

int flow2d_subset_refine_masked_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                                   size_t pitch_bytes, const float* node_u0, const float* node_v0, const float* node_ux0,
                                   const float* node_uy0, const float* node_vx0, const float* node_vy0, size_t nw, size_t nh,
                                   size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations,
                                   float epsilon, float max_shift, float max_gradient, const float* mask, int min_pixels, float* out_u,
                                   float* out_v, float* out_ux, float* out_uy, float* out_vx, float* out_vy, float* out_score,
                                   float* out_state, flow2d_subset_record* record)
{
    if (mask == nullptr)  // (min_pixels is not looked at) every byte and the record of flow2d_subset_refine_from_2d: its kernel
        return flow2d_subset_refine_from_2d(ctx, frame_0, frame_1, width, height, pitch_bytes, node_u0, node_v0, node_ux0, node_uy0,
                                            node_vx0, node_vy0, nw, nh, node_pitch_bytes, grid_radius, spacing, subset_radius,
                                            max_iterations, epsilon, max_shift, max_gradient, out_u, out_v, out_ux, out_uy, out_vx, out_vy,
                                            out_score, out_state, record);
    return subset_refine_masked<CatmullRom>(ctx, frame_0, frame_1, width, height, pitch_bytes, node_u0, node_v0, node_ux0, node_uy0,
                                            node_vx0, node_vy0, nw, nh, node_pitch_bytes, grid_radius, spacing, subset_radius,
                                            max_iterations, epsilon, max_shift, max_gradient, mask, min_pixels, out_u, out_v, out_ux,
                                            out_uy, out_vx, out_vy, out_score, out_state, record);
}

int flow2d_subset_refine_spline_2d(flow2d_context* ctx, const float* frame_0, const float* coeff_1, size_t width, size_t height,
                                   size_t pitch_bytes, const float* node_u0, const float* node_v0, const float* node_ux0,
                                   const float* node_uy0, const float* node_vx0, const float* node_vy0, size_t nw, size_t nh,
                                   size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations,
                                   float epsilon, float max_shift, float max_gradient, const float* mask, int min_pixels, float* out_u,
                                   float* out_v, float* out_ux, float* out_uy, float* out_vx, float* out_vy, float* out_score,
                                   float* out_state, flow2d_subset_record* record)
{
    return subset_refine_masked<BSpline>(ctx, frame_0, coeff_1, width, height, pitch_bytes, node_u0, node_v0, node_ux0, node_uy0,
                                         node_vx0, node_vy0, nw, nh, node_pitch_bytes, grid_radius, spacing, subset_radius,
                                         max_iterations, epsilon, max_shift, max_gradient, mask, min_pixels, out_u, out_v, out_ux,
                                         out_uy, out_vx, out_vy, out_score, out_state, record);
}

}  // extern "C"
