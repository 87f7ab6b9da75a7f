// Subset refinement of correlation nodes for gfx950: the inverse-compositional Gauss-Newton iteration with an affine shape
// function on the zero-mean normalised sum of squared differences, one node per wave.
//
// The normative definition is the one of flow2d_subset_refine_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// The kernel here serves flow2d_subset_refine_2d and flow2d_subset_refine_from_2d; subset_refine_masked.hip states the same iteration
// over a list of pixels, and its instantiation without a mask gives these entries' bytes, but timed 0.7 to 1.6 % behind this kernel
// at R = 15 (profiles/subset_unified/README.md), so this one stays.  Both take their node, the frame-0 fill, the window test and
// the host body from subset_node.hpp and the samplers from subset_sample.hpp.
// As in correlate_offset_kernel a wave owns a node and shares nothing with the other waves of its workgroup (no barrier at all
// here).  A lane owns the subset's pixels lane, lane + 64, ... (at most 16 at R = 15; with N < 64 lanes idle).  What is constant
// over the iterations -- fd, fx, fy of a lane's pixels -- and the samples g of the current iteration live in the wave's slice
// of dynamic LDS, four doubles per pixel, each element read and written by its own lane only: 7.2 KB per wave at R = 7, 30.8 KB
// at R = 15.  The entry sizes the workgroup so that the slices fit the 64 KB every launch may ask for without an attribute
// call: four waves up to R = 10, three at R = 11 and 12 (16 960 bytes per wave at R = 11), two from R = 13.
// A *sum over the subset* is the lane's partial over its pixels in ascending order, from 0, then wave_sum's butterfly: every
// lane ends with the same bits, so H, its Cholesky factor, b and p are the same in every lane -- the 6 x 6 algebra runs
// redundantly in all lanes, nothing is broadcast, and every branch on a node's state is uniform over the wave.
// Frame 1 is gathered from global memory, 16 taps per pixel and iteration, clamped to the frame; nothing of it is staged (a patch
// per node in LDS was built and measured no faster: DESIGN.md 3.17).
#include <cmath>

#include "small_cholesky.hpp"
#include "subset_node.hpp"

namespace {

struct SubsetArgs {
    const float *f0, *f1;
    const float *u0, *v0;
    float *u, *v, *ux, *uy, *vx, *vy;  // the gradient planes: all or none
    float *score, *state;              // null = absent
    unsigned long long* record;        // eight words per instance, or null
    int w, h, pitch;                   // the frames; pitch in floats
    int nw, nh, npitch;                // the node planes
    int r, s, R, K;
    unsigned slice;  // doubles of one of a wave's four LDS arrays: N rounded up to a multiple of 2
    double epsilon, max_shift, max_gradient;
};

// J of the header for pixel k.
__device__ __forceinline__ void jacobian(const SubsetNode& nd, int k, double (&J)[6])
{
    const int ky = k / nd.side, kx = k - ky * nd.side;
    const double xi = static_cast<double>(kx - nd.R), eta = static_cast<double>(ky - nd.R);
    const double fx = nd.fx[k], fy = nd.fy[k];
    J[0] = fx;
    J[1] = fx * xi;
    J[2] = fx * eta;
    J[3] = fy;
    J[4] = fy * xi;
    J[5] = fy * eta;
}

// The node from the frame-0 quantities on: the state, with p, the last c and the iterations begun.  p = (u, ux, uy, v, vx, vy)
// holds the start on entry: (u0, 0, 0, v0, 0, 0), or (u0, ux0, uy0, v0, vx0, vy0) of flow2d_subset_refine_from_2d.  Every lane of
// the wave returns the same values.
template <typename Offset>
__device__ __forceinline__ int refine_node(const SubsetNode& nd, const SubsetArgs& a, double (&p)[6], double& score, unsigned& iterations)
{
    const double u0 = p[0], v0 = p[3];
    const double count = static_cast<double>(nd.n);
    const int left = nd.cx - nd.R, top = nd.cy - nd.R;

    // frame 0: f into the fd array first, its gradients, the mean
    const double fm = wave_sum(fill_frame_0<Offset>(nd)) / count;

    double df2 = 0.0;
    double hs[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) hs[i] = 0.0;
    for (int k = nd.lane; k < nd.n; k += 64) {
        const double fd = nd.fd[k] - fm;
        nd.fd[k] = fd;
        df2 += fd * fd;
        double J[6];
        jacobian(nd, k, J);
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
    // factor<6> of small_cholesky.hpp, kept written out: through the header the kernel timed 1.2 % slower at R = 15 (see there)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double hkk = L[k][k];
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < k; ++m) sum += L[k][m] * L[k][m];
        const double d = hkk - sum;
        if (!(d > 1e-10 * hkk)) return kStateFlat;
        L[k][k] = sqrt(d);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double inner = 0.0;
#pragma unroll
            for (int m = 0; m < k; ++m) inner += L[i][m] * L[k][m];
            L[i][k] = (L[i][k] - inner) / L[k][k];
        }
    }

    const double xmax = static_cast<double>(nd.w - 1), ymax = static_cast<double>(nd.h - 1);
    const double radius = static_cast<double>(nd.R);
    for (int n = 1; n <= a.K; ++n) {
        iterations = static_cast<unsigned>(n);
        // 1, 2: positions and samples
        unsigned outside = 0;
        double sum_g = 0.0;
        for (int k = nd.lane; k < nd.n; k += 64) {
            const int ky = k / nd.side, kx = k - ky * nd.side;
            const double xi = static_cast<double>(kx - nd.R), eta = static_cast<double>(ky - nd.R);
            const double X = static_cast<double>(left + kx) + ((p[0] + p[1] * xi) + p[2] * eta);
            const double Y = static_cast<double>(top + ky) + ((p[3] + p[4] * xi) + p[5] * eta);
            double g = 0.0;
            if (X >= 0.0 && X <= xmax && Y >= 0.0 && Y <= ymax)
                g = cubic_sample<Offset>(nd, X, Y);
            else
                outside = 1;
            nd.g[k] = g;
            sum_g += g;
        }
        if (wave_sum(outside) != 0) return kStateStrayed;
        // 3: the residual and the step
        const double gm = wave_sum(sum_g) / count;
        double dg2 = 0.0, sfg = 0.0;
        for (int k = nd.lane; k < nd.n; k += 64) {
            const double gd = nd.g[k] - gm;
            nd.g[k] = gd;
            dg2 += gd * gd;
            sfg += nd.fd[k] * gd;
        }
        dg2 = wave_sum(dg2);
        sfg = wave_sum(sfg);
        if (!(dg2 > 0.0)) return kStateFlat;
        const double dg = sqrt(dg2);
        score = sfg / (df * dg);
        const double q = df / dg;
        double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = nd.lane; k < nd.n; k += 64) {
            const double res = nd.fd[k] - q * nd.g[k];
            double J[6];
            jacobian(nd, k, J);
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

// The four start gradients of flow2d_subset_refine_from_2d.
struct SubsetStart {
    const float *ux0, *uy0, *vx0, *vy0;
};

// Whether the start's gradients are finite; without a start there are none to look at.
template <bool kFrom>
__device__ __forceinline__ bool gradients_finite(const float (&g0)[4])
{
    if constexpr (kFrom)
        return finite(g0[0]) && finite(g0[1]) && finite(g0[2]) && finite(g0[3]);
    else
        return true;
}

// A wave's node from its inputs to its outputs.  Start: nothing -- flow2d_subset_refine_2d, whose instantiation is the kernel it
// was before the pack, argument for argument and instruction for instruction -- or one SubsetStart, the start's gradients of
// flow2d_subset_refine_from_2d.  (The body stays in the kernel itself: moved into a function that two kernels call, it compiled
// to another instruction stream for the plain one; profiles/subset_sequence/README.md.)
template <typename Offset, typename... Start>
__global__ __launch_bounds__(64 * kSubsetMaxWaves) void subset_refine_kernel(SubsetArgs a, BatchArg batch, Start... start)
{
    static_assert(sizeof...(Start) <= 1, "nothing or one SubsetStart");
    constexpr bool kFrom = sizeof...(Start) != 0;
    extern __shared__ __attribute__((aligned(16))) double s_subset[];

    const size_t inst = batch_offset(batch);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node = blockIdx.x * (blockDim.x >> 6) + wave;
    if (node >= a.nw * a.nh) return;  // (no barrier anywhere: the last workgroup's surplus waves leave)
    const int jn = node / a.nw, in = node - jn * a.nw;

    SubsetNode nd;
    nd.f0 = a.f0 + inst;
    nd.f1 = a.f1 + inst;
    nd.fd = s_subset + static_cast<size_t>(wave) * 4u * a.slice;
    nd.fx = nd.fd + a.slice;
    nd.fy = nd.fx + a.slice;
    nd.g = nd.fy + a.slice;
    nd.w = a.w;
    nd.h = a.h;
    nd.pitch = a.pitch;
    nd.cx = a.r + in * a.s;
    nd.cy = a.r + jn * a.s;
    nd.R = a.R;
    nd.side = 2 * a.R + 1;
    nd.n = nd.side * nd.side;
    nd.lane = lane;

    const size_t at = node_at(inst, in, jn, a.npitch);
    const float u0 = a.u0[at], v0 = a.v0[at];
    float g0[4] = {0.f, 0.f, 0.f, 0.f};  // ux0, uy0, vx0, vy0
    if constexpr (kFrom) {
        const SubsetStart st = (start, ...);
        g0[0] = st.ux0[at];
        g0[1] = st.uy0[at];
        g0[2] = st.vx0[at];
        g0[3] = st.vy0[at];
    }
    double p[6] = {static_cast<double>(u0), static_cast<double>(g0[0]), static_cast<double>(g0[1]),
                   static_cast<double>(v0), static_cast<double>(g0[2]), static_cast<double>(g0[3])};
    double score = 0.0;
    unsigned iterations = 0;
    int state;
    if (!(finite(u0) && finite(v0)) || !gradients_finite<kFrom>(g0))
        state = kStateNoInput;
    else if (!subset_inside_frame(nd.cx, nd.cy, nd.R, a.w, a.h))
        state = kStateStrayed;
    else
        state = refine_node<Offset>(nd, a, p, score, iterations);
    if (lane != 0) return;

    float out[6], out_score = 0.f;
    if (state >= 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = static_cast<float>(p[i]);
        out_score = static_cast<float>(score);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = state == kStateNoInput ? quiet_nan() : 0.f;
        if (state != kStateNoInput) {
            out[0] = u0;
            out[3] = v0;
            if constexpr (kFrom) {  // flat and strayed hand the whole start back: the field stays the next step's input
                out[1] = g0[0];
                out[2] = g0[1];
                out[4] = g0[2];
                out[5] = g0[3];
            }
        }
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
        const unsigned counts[kSubsetCounts] = {1u, state >= 1, state == 0, state == kStateStrayed, state == kStateFlat,
                                                state == kStateNoInput, iterations};
        add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
    }
}

// Both entries: flow2d_subset_refine_2d is `start` absent.
int subset_refine_entry(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height, size_t pitch_bytes,
                        const float* node_u0, const float* node_v0, const float* const (&start)[4], size_t nw, size_t nh,
                        size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations, float epsilon,
                        float max_shift, float max_gradient, float* out_u, float* out_v, float* out_ux, float* out_uy, float* out_vx,
                        float* out_vy, float* out_score, float* out_state, flow2d_subset_record* record)
{
    const float* const starts[6] = {node_u0, start[0], start[1], node_v0, start[2], start[3]};
    float* const outs[6] = {out_u, out_ux, out_uy, out_v, out_vx, out_vy};
    flow2d::SubsetWaves lds;
    const int status = flow2d::subset_refine_enter(ctx, frame_0, frame_1, nullptr, width, height, pitch_bytes, starts, outs, 6, out_score,
                                                   out_state, record, nw, nh, node_pitch_bytes, grid_radius, spacing, 1, subset_radius,
                                                   max_iterations, epsilon, {max_shift, max_gradient}, 0, lds);
    if (status != FLOW2D_OK) return status;
    const bool started = start[0] != nullptr;
    const unsigned slice = lds.slice, wave_bytes = lds.wave_bytes, waves = lds.waves;
    const SubsetArgs a = {frame_0, frame_1, node_u0, node_v0, out_u, out_v, out_ux, out_uy, out_vx, out_vy, out_score, out_state,
                          reinterpret_cast<unsigned long long*>(record),
                          static_cast<int>(width), static_cast<int>(height), static_cast<int>(pitch_bytes / 4),
                          static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                          grid_radius, spacing, subset_radius, max_iterations, slice,
                          static_cast<double>(epsilon), static_cast<double>(max_shift), static_cast<double>(max_gradient)};
    const SubsetStart st = {start[0], start[1], start[2], start[3]};
    // (the largest offset a lane forms into a frame is below height * pitch_bytes; the node planes are addressed in 64 bits)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        const dim3 grid(flow2d::div_up(nw * nh, waves), 1, flow2d::batch_z(ctx, 1)), block(64 * waves);
        if (started)
            subset_refine_kernel<decltype(offset), SubsetStart><<<grid, block, waves * wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1), st);
        else  // (no start planes: the kernel, and so every byte, of flow2d_subset_refine_2d)
            subset_refine_kernel<decltype(offset)><<<grid, block, waves * wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // namespace

extern "C" {

int flow2d_subset_refine_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                            size_t pitch_bytes, const float* node_u0, const float* node_v0, size_t nw, size_t nh,
                            size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations, float epsilon,
                            float max_shift, float max_gradient, float* out_u, float* out_v, float* out_ux, float* out_uy,
                            float* out_vx, float* out_vy, float* out_score, float* out_state, flow2d_subset_record* record)
{
    const float* const none[4] = {nullptr, nullptr, nullptr, nullptr};
    return subset_refine_entry(ctx, frame_0, frame_1, width, height, pitch_bytes, node_u0, node_v0, none, nw, nh, node_pitch_bytes,
                               grid_radius, spacing, subset_radius, max_iterations, epsilon, max_shift, max_gradient, out_u, out_v, out_ux,
                               out_uy, out_vx, out_vy, out_score, out_state, record);
}

int flow2d_subset_refine_from_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                                 size_t pitch_bytes, const float* node_u0, const float* node_v0, const float* node_ux0,
                                 const float* node_uy0, const float* node_vx0, const float* node_vy0, size_t nw, size_t nh,
                                 size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations,
                                 float epsilon, float max_shift, float max_gradient, float* out_u, float* out_v, float* out_ux,
                                 float* out_uy, float* out_vx, float* out_vy, float* out_score, float* out_state,
                                 flow2d_subset_record* record)
{
    const float* const start[4] = {node_ux0, node_uy0, node_vx0, node_vy0};
    return subset_refine_entry(ctx, frame_0, frame_1, width, height, pitch_bytes, node_u0, node_v0, start, nw, nh, node_pitch_bytes,
                               grid_radius, spacing, subset_radius, max_iterations, epsilon, max_shift, max_gradient, out_u, out_v, out_ux,
                               out_uy, out_vx, out_vy, out_score, out_state, record);
}

}  // extern "C"
