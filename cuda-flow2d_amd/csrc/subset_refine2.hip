// Subset refinement with a second-order shape function for gfx950: the twelve-parameter inverse-compositional Gauss-Newton
// iteration on the zero-mean normalised sum of squared differences, one node per wave.
//
// The normative definition is the one of flow2d_subset_refine2_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// The shape is subset_refine.hip's: a wave owns a node and shares nothing with the other waves of its workgroup (no barrier), a
// lane owns the subset's pixels lane, lane + 64, ..., and fd, fx, fy of a lane's pixels and the samples g of the current
// iteration live in the wave's slice of dynamic LDS, each element read and written by its own lane only.  A *sum over the subset*
// is the lane's partial over its pixels in ascending order, from 0, then wave_sum's butterfly: every lane ends with the same bits,
// the 12 x 12 and 5 x 5 algebra runs redundantly in all lanes and every branch on a node's state is uniform over the wave.
// What is new is where the registers go:
//   the Hessian's 3 x 21 sums are accumulated in three passes over the subset, 21 accumulators each (wxx, wxy, wyy in turn);
//   H and then its Cholesky factor, 78 doubles, live in the wave's slice of LDS too, behind the four pixel arrays (624 bytes;
//   at R = 15 two waves' slices still fit the 64 KB).  Lane 0 writes an element, every lane reads it back as a broadcast: the
//   LDS serves a wave's accesses in order, and __builtin_amdgcn_wave_barrier keeps the compiler from moving one across another.
// Frame 1 is gathered from global memory, 16 taps per pixel and iteration, clamped to the frame.
// The sample of the deformed frame is a template parameter (subset_sample.hpp): CatmullRom is flow2d_subset_refine2_2d, BSpline on
// frame 1's coefficients flow2d_subset_refine2_spline_2d, whose taps are reflected.  Both entries share one host body.
#include <cmath>

#include "subset_node.hpp"

namespace {

constexpr unsigned kFactorDoubles = 78;  // the lower triangle of a 12 x 12 matrix

struct Subset2Args {
    const float *f0, *f1;
    const float* start[12];  // u0, ux0, uy0, uxx0, uxy0, uyy0, v0, vx0, ...: the order of p; null = absent, 0
    float* out[12];          // the same order; u and v are there, the gradients and the curvatures all or none
    float *score, *state;    // null = absent
    unsigned long long* record;  // eight words per instance, or null
    int w, h, pitch;             // the frames; pitch in floats
    int nw, nh, npitch;          // the node planes
    int r, s, R, K;
    unsigned slice;  // doubles of one of a wave's four pixel arrays: N rounded up to a multiple of 2
    double epsilon, max_shift, max_gradient, max_curvature;
};

struct Subset2Node : SubsetNode {
    double* L;  // H's lower triangle, then the factor's, behind the pixel arrays: element (i, j) at i*(i + 1)/2 + j
};

// phi of the header for pixel k.
__device__ __forceinline__ void shape(const Subset2Node& nd, int k, double (&phi)[6])
{
    const int ky = k / nd.side, kx = k - ky * nd.side;
    const double xi = static_cast<double>(kx - nd.R), eta = static_cast<double>(ky - nd.R);
    phi[0] = 1.0;
    phi[1] = xi;
    phi[2] = eta;
    phi[3] = 0.5 * xi * xi;
    phi[4] = xi * eta;
    phi[5] = 0.5 * eta * eta;
}

constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// One 6 x 6 block of H: the 21 sums of weight * (phi[a] * phi[b]), b <= a, into the triangle in LDS.  kWeight: 0 fx*fx, rows
// and columns 0 .. 5; 2 fy*fy, rows and columns 6 .. 11; 1 fx*fy, the block between them, whose rows 6 .. 11 lie below its columns
// 0 .. 5, so that both (a, b) and (b, a) are filled from the same sum.
template <int kWeight>
__device__ __forceinline__ void hessian_block(const Subset2Node& nd)
{
    double hs[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) hs[i] = 0.0;
    for (int k = nd.lane; k < nd.n; k += 64) {
        const double fx = nd.fx[k], fy = nd.fy[k];
        const double weight = kWeight == 0 ? fx * fx : kWeight == 1 ? fx * fy : fy * fy;
        double phi[6];
        shape(nd, k, phi);
        int at = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) hs[at++] += weight * (phi[a] * phi[b]);
    }
    int at = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            const double sum = wave_sum(hs[at++]);
            if (nd.lane == 0) {
                if (kWeight == 0) nd.L[tri(a, b)] = sum;
                if (kWeight == 2) nd.L[tri(6 + a, 6 + b)] = sum;
                if (kWeight == 1) {
                    nd.L[tri(6 + a, b)] = sum;
                    nd.L[tri(6 + b, a)] = sum;
                }
            }
        }
}

// The Cholesky factorisation of the header in place in LDS; false where a pivot fails its test.
__device__ __forceinline__ bool factor_in_lds(const Subset2Node& nd)
{
    double* L = nd.L;
#pragma unroll 1
    for (int k = 0; k < 12; ++k) {
        const double hkk = L[tri(k, k)];
        double sum = 0.0;
        for (int m = 0; m < k; ++m) sum += L[tri(k, m)] * L[tri(k, m)];
        const double d = hkk - sum;
        if (!(d > 1e-10 * hkk)) return false;
        const double lkk = sqrt(d);
        __builtin_amdgcn_wave_barrier();
        if (nd.lane == 0) L[tri(k, k)] = lkk;
#pragma unroll 1
        for (int i = k + 1; i < 12; ++i) {
            double inner = 0.0;
            for (int m = 0; m < k; ++m) inner += L[tri(i, m)] * L[tri(k, m)];
            const double lik = (L[tri(i, k)] - inner) / lkk;
            __builtin_amdgcn_wave_barrier();
            if (nd.lane == 0) L[tri(i, k)] = lik;
        }
        __builtin_amdgcn_wave_barrier();
    }
    return true;
}

// Solve of the header with the factor in LDS.
__device__ __forceinline__ void solve_from_lds(const double* L, const double (&b)[12], double (&x)[12])
{
    double y[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < i; ++m) sum += L[tri(i, m)] * y[m];
        y[i] = (b[i] - sum) / L[tri(i, i)];
        __builtin_amdgcn_sched_barrier(0);  // a row's loads at a time: hoisted together, the 78 elements are 156 registers
    }
#pragma unroll
    for (int i = 11; i >= 0; --i) {
        double sum = 0.0;
#pragma unroll
        for (int m = i + 1; m < 12; ++m) sum += L[tri(m, i)] * x[m];
        x[i] = (y[i] - sum) / L[tri(i, i)];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// A(q) or B(q) of the header: the row of a warp's matrix that gives xi' (kV false) or eta' (kV true).
template <bool kV>
__device__ __forceinline__ void warp_row(const double* q, double (&row)[6])
{
    row[0] = 0.5 * q[3];
    row[1] = q[4];
    row[2] = 0.5 * q[5];
    row[3] = kV ? q[1] : 1.0 + q[1];
    row[4] = kV ? 1.0 + q[2] : q[2];
    row[5] = q[0];
}

// Step 4 of the header: p <- W(p) o W(dp)^-1; false where a pivot fails its test.
__device__ __forceinline__ bool compose(double (&p)[12], const double (&dp)[12])
{
    double a[6], b[6];
    warp_row<false>(dp, a);
    warp_row<true>(dp + 6, b);
    double W[5][6];
    W[0][0] = a[3] * a[3] + 2.0 * (a[0] * a[5]);
    W[0][1] = 2.0 * (a[3] * a[4]) + 2.0 * (a[1] * a[5]);
    W[0][2] = a[4] * a[4] + 2.0 * (a[2] * a[5]);
    W[0][3] = 2.0 * (a[3] * a[5]);
    W[0][4] = 2.0 * (a[4] * a[5]);
    W[0][5] = a[5] * a[5];
    W[1][0] = (a[3] * b[3] + a[0] * b[5]) + a[5] * b[0];
    W[1][1] = ((a[3] * b[4] + a[4] * b[3]) + a[1] * b[5]) + a[5] * b[1];
    W[1][2] = (a[4] * b[4] + a[2] * b[5]) + a[5] * b[2];
    W[1][3] = a[3] * b[5] + a[5] * b[3];
    W[1][4] = a[4] * b[5] + a[5] * b[4];
    W[1][5] = a[5] * b[5];
    W[2][0] = b[3] * b[3] + 2.0 * (b[0] * b[5]);
    W[2][1] = 2.0 * (b[3] * b[4]) + 2.0 * (b[1] * b[5]);
    W[2][2] = b[4] * b[4] + 2.0 * (b[2] * b[5]);
    W[2][3] = 2.0 * (b[3] * b[5]);
    W[2][4] = 2.0 * (b[4] * b[5]);
    W[2][5] = b[5] * b[5];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        W[3][j] = a[j];
        W[4][j] = b[j];
    }
    double M[5][5], ra[6], rb[6];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int i = 0; i < 5; ++i) M[j][i] = W[i][j];
    warp_row<false>(p, ra);
    warp_row<true>(p + 6, rb);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (!(fabs(M[k][k]) > 1e-6)) return false;
#pragma unroll
        for (int j = k + 1; j < 5; ++j) {
            const double f = M[j][k] / M[k][k];
#pragma unroll
            for (int i = k + 1; i < 5; ++i) M[j][i] = M[j][i] - f * M[k][i];
            ra[j] = ra[j] - f * ra[k];
            rb[j] = rb[j] - f * rb[k];
        }
    }
    double za[6], zb[6];
#pragma unroll
    for (int i = 4; i >= 0; --i) {
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int m = i + 1; m < 5; ++m) {
            sa += M[i][m] * za[m];
            sb += M[i][m] * zb[m];
        }
        za[i] = (ra[i] - sa) / M[i][i];
        zb[i] = (rb[i] - sb) / M[i][i];
    }
    za[5] = ra[5] - ((((za[0] * W[0][5] + za[1] * W[1][5]) + za[2] * W[2][5]) + za[3] * W[3][5]) + za[4] * W[4][5]);
    zb[5] = rb[5] - ((((zb[0] * W[0][5] + zb[1] * W[1][5]) + zb[2] * W[2][5]) + zb[3] * W[3][5]) + zb[4] * W[4][5]);
    p[0] = za[5];
    p[1] = za[3] - 1.0;
    p[2] = za[4];
    p[3] = 2.0 * za[0];
    p[4] = za[1];
    p[5] = 2.0 * za[2];
    p[6] = zb[5];
    p[7] = zb[3];
    p[8] = zb[4] - 1.0;
    p[9] = 2.0 * zb[0];
    p[10] = zb[1];
    p[11] = 2.0 * zb[2];
    return true;
}

// The node from the frame-0 quantities on: the state, with p, the last c and the iterations begun.  p holds the start on entry.
// Every lane of the wave returns the same values.
template <typename Offset, typename Sampler>
__device__ __forceinline__ int refine_node(const Subset2Node& nd, const Subset2Args& a, double (&p)[12], double& score, unsigned& iterations)
{
    const double u0 = p[0], v0 = p[6];
    const double count = static_cast<double>(nd.n);
    const int left = nd.cx - nd.R, top = nd.cy - nd.R;

    // frame 0: f into the fd array first, its gradients, the mean
    const double fm = wave_sum(fill_frame_0<Offset>(nd)) / count;
    double df2 = 0.0;
    for (int k = nd.lane; k < nd.n; k += 64) {
        const double fd = nd.fd[k] - fm;
        nd.fd[k] = fd;
        df2 += fd * fd;
    }
    df2 = wave_sum(df2);
    if (!(df2 > 0.0)) return kStateFlat;
    const double df = sqrt(df2);
    hessian_block<0>(nd);
    hessian_block<1>(nd);
    hessian_block<2>(nd);
    __builtin_amdgcn_wave_barrier();
    if (!factor_in_lds(nd)) return kStateFlat;

    const double xmax = static_cast<double>(nd.w - 1), ymax = static_cast<double>(nd.h - 1);
    const double radius = static_cast<double>(nd.R), r2 = static_cast<double>(nd.R * nd.R), hr2 = 0.5 * r2;
    for (int n = 1; n <= a.K; ++n) {
        iterations = static_cast<unsigned>(n);
        // 1, 2: positions and samples
        unsigned outside = 0;
        double sum_g = 0.0;
        for (int k = nd.lane; k < nd.n; k += 64) {
            const int ky = k / nd.side, kx = k - ky * nd.side;
            double phi[6];
            shape(nd, k, phi);
            const double X = static_cast<double>(left + kx) + (((((p[0] + p[1] * phi[1]) + p[2] * phi[2]) + p[3] * phi[3]) + p[4] * phi[4]) + p[5] * phi[5]);
            const double Y = static_cast<double>(top + ky) + (((((p[6] + p[7] * phi[1]) + p[8] * phi[2]) + p[9] * phi[3]) + p[10] * phi[4]) + p[11] * phi[5]);
            double g = 0.0;
            if (X >= 0.0 && X <= xmax && Y >= 0.0 && Y <= ymax)
                g = Sampler::template sample<Offset>(nd, X, Y);
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
        double b[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) b[i] = 0.0;
        for (int k = nd.lane; k < nd.n; k += 64) {
            const double res = nd.fd[k] - q * nd.g[k];
            const double fx = nd.fx[k], fy = nd.fy[k];
            double phi[6];
            shape(nd, k, phi);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                b[i] += (fx * phi[i]) * res;
                b[6 + i] += (fy * phi[i]) * res;
            }
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) b[i] = wave_sum(b[i]);
        double dp[12];
        solve_from_lds(nd.L, b, dp);
#pragma unroll
        for (int i = 0; i < 12; ++i) dp[i] = -dp[i];
        // (the step's norm of 5 first: dp is dead once W(dp) is built)
        const double scale[6] = {1.0, radius, radius, hr2, r2, hr2};
        double step2 = dp[0] * dp[0];
#pragma unroll
        for (int i = 1; i < 12; ++i) {
            const double t = i == 6 ? dp[6] : scale[i % 6] * dp[i];
            step2 += t * t;
        }
        // 4: p <- W(p) o W(dp)^-1
        if (!compose(p, dp)) return kStateStrayed;
        // 5: the bounds, then convergence
        if (!(fabs(p[0] - u0) <= a.max_shift && fabs(p[6] - v0) <= a.max_shift && fabs(p[1]) <= a.max_gradient &&
              fabs(p[2]) <= a.max_gradient && fabs(p[7]) <= a.max_gradient && fabs(p[8]) <= a.max_gradient &&
              fabs(p[3]) <= a.max_curvature && fabs(p[4]) <= a.max_curvature && fabs(p[5]) <= a.max_curvature &&
              fabs(p[9]) <= a.max_curvature && fabs(p[10]) <= a.max_curvature && fabs(p[11]) <= a.max_curvature))
            return kStateStrayed;
        if (sqrt(step2) < a.epsilon) return n;
    }
    return 0;
}

// Compiled for three waves per SIMD, the occupancy of subset_refine_kernel: 164 / 166 VGPRs and no scratch.  Left to itself the
// compiler takes 256 (one wave); asked for four it spills (profiles/subset2/resource_usage.txt).
template <typename Offset, typename Sampler>
__global__ __launch_bounds__(64 * kSubsetMaxWaves) __attribute__((amdgpu_waves_per_eu(3, 3))) void subset_refine2_kernel(Subset2Args a, BatchArg batch)
{
    extern __shared__ __attribute__((aligned(16))) double s_subset2[];

    const size_t inst = batch_offset(batch);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node = blockIdx.x * (blockDim.x >> 6) + wave;
    if (node >= a.nw * a.nh) return;  // (no barrier anywhere: the last workgroup's surplus waves leave)
    const int jn = node / a.nw, in = node - jn * a.nw;

    Subset2Node nd;
    // (set-up and record stay written out here as in subset_refine_kernel: through a shared helper this kernel's registers moved)
    nd.f0 = a.f0 + inst;
    nd.f1 = a.f1 + inst;
    nd.fd = s_subset2 + static_cast<size_t>(wave) * (4u * a.slice + kFactorDoubles);
    nd.fx = nd.fd + a.slice;
    nd.fy = nd.fx + a.slice;
    nd.g = nd.fy + a.slice;
    nd.L = nd.g + a.slice;
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
    float start[12];
    bool is_finite = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        start[i] = a.start[i] ? a.start[i][at] : 0.f;
        is_finite = is_finite && finite(start[i]);
    }
    double p[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = static_cast<double>(start[i]);
    double score = 0.0;
    unsigned iterations = 0;
    int state;
    if (!is_finite)
        state = kStateNoInput;
    else if (!subset_inside_frame(nd.cx, nd.cy, nd.R, a.w, a.h))
        state = kStateStrayed;
    else
        state = refine_node<Offset, Sampler>(nd, a, p, score, iterations);
    if (lane != 0) return;

    const float out_score = state >= 0 ? static_cast<float>(score) : 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i)
        if (a.out[i]) a.out[i][at] = state >= 0 ? static_cast<float>(p[i]) : state == kStateNoInput ? quiet_nan() : start[i];
    if (a.score) a.score[at] = out_score;
    if (a.state) a.state[at] = static_cast<float>(state);
    if (a.record) {
        const unsigned counts[kSubsetCounts] = {1u, state >= 1, state == 0, state == kStateStrayed, state == kStateFlat,
                                                state == kStateNoInput, iterations};
        add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
    }
}

// The body of both entries; frame_1 is the frame for CatmullRom and its coefficients for BSpline.
template <typename Sampler>
int subset_refine2(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height, size_t pitch_bytes,
                   const float* node_u0, const float* node_v0, const float* const* start_gradients,
                   const float* const* start_curvatures, size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius, int spacing,
                   int subset_radius, int max_iterations, float epsilon, float max_shift, float max_gradient, float max_curvature,
                   float* out_u, float* out_v, float* const* out_gradients, float* const* out_curvatures, float* out_score,
                   float* out_state, flow2d_subset_record* record)
{
    // the planes in the order of p; a group that is absent, or a place in it, stays null
    Subset2Args a = {};
    a.start[0] = node_u0;
    a.start[6] = node_v0;
    a.out[0] = out_u;
    a.out[6] = out_v;
    for (int half = 0; half < 2; ++half) {
        for (int i = 0; i < 2; ++i) {
            if (start_gradients) a.start[6 * half + 1 + i] = start_gradients[2 * half + i];
            if (out_gradients) a.out[6 * half + 1 + i] = out_gradients[2 * half + i];
        }
        for (int i = 0; i < 3; ++i) {
            if (start_curvatures) a.start[6 * half + 3 + i] = start_curvatures[3 * half + i];
            if (out_curvatures) a.out[6 * half + 3 + i] = out_curvatures[3 * half + i];
        }
    }
    flow2d::SubsetWaves lds;  // (a wave's bytes: at most 31 408)
    const int status = flow2d::subset_refine_enter(ctx, frame_0, frame_1, nullptr, width, height, pitch_bytes, a.start, a.out, 12, out_score,
                                                   out_state, record, nw, nh, node_pitch_bytes, grid_radius, spacing,
                                                   FLOW2D_SUBSET2_MIN_RADIUS, subset_radius, max_iterations, epsilon,
                                                   {max_shift, max_gradient, max_curvature}, kFactorDoubles * sizeof(double), lds);
    if (status != FLOW2D_OK) return status;
    const unsigned slice = lds.slice, wave_bytes = lds.wave_bytes, waves = lds.waves;
    a.f0 = frame_0;
    a.f1 = frame_1;
    a.score = out_score;
    a.state = out_state;
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
    a.K = max_iterations;
    a.slice = slice;
    a.epsilon = static_cast<double>(epsilon);
    a.max_shift = static_cast<double>(max_shift);
    a.max_gradient = static_cast<double>(max_gradient);
    a.max_curvature = static_cast<double>(max_curvature);
    // (the largest offset a lane forms into a frame is below height * pitch_bytes; the node planes are addressed in 64 bits)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        const dim3 grid(flow2d::div_up(nw * nh, waves), 1, flow2d::batch_z(ctx, 1)), block(64 * waves);
        subset_refine2_kernel<decltype(offset), Sampler><<<grid, block, waves * wave_bytes, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // namespace

extern "C" {

int flow2d_subset_refine2_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                             size_t pitch_bytes, const float* node_u0, const float* node_v0, const float* const* start_gradients,
                             const float* const* start_curvatures, size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius,
                             int spacing, int subset_radius, int max_iterations, float epsilon, float max_shift, float max_gradient,
                             float max_curvature, float* out_u, float* out_v, float* const* out_gradients,
                             float* const* out_curvatures, float* out_score, float* out_state, flow2d_subset_record* record)
{
    return subset_refine2<CatmullRom>(ctx, frame_0, frame_1, width, height, pitch_bytes, node_u0, node_v0, start_gradients,
                                      start_curvatures, nw, nh, node_pitch_bytes, grid_radius, spacing, subset_radius, max_iterations,
                                      epsilon, max_shift, max_gradient, max_curvature, out_u, out_v, out_gradients, out_curvatures,
                                      out_score, out_state, record);
}

int flow2d_subset_refine2_spline_2d(flow2d_context* ctx, const float* frame_0, const float* coeff_1, size_t width, size_t height,
                                    size_t pitch_bytes, const float* node_u0, const float* node_v0,
                                    const float* const* start_gradients, const float* const* start_curvatures, size_t nw, size_t nh,
                                    size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations,
                                    float epsilon, float max_shift, float max_gradient, float max_curvature, float* out_u,
                                    float* out_v, float* const* out_gradients, float* const* out_curvatures, float* out_score,
                                    float* out_state, flow2d_subset_record* record)
{
    return subset_refine2<BSpline>(ctx, frame_0, coeff_1, width, height, pitch_bytes, node_u0, node_v0, start_gradients,
                                   start_curvatures, nw, nh, node_pitch_bytes, grid_radius, spacing, subset_radius, max_iterations,
                                   epsilon, max_shift, max_gradient, max_curvature, out_u, out_v, out_gradients, out_curvatures,
                                   out_score, out_state, record);
}

}  // extern "C"
