// The composition of two node fields of a DIC sequence whose reference frame has moved, for gfx950: the base (frame 0 -> frame r
// at the nodes of frame 0) with the increment (frame r -> frame k on the same grid laid in frame r), sampled where the base
// carries each node, into frame 0 -> frame k at the nodes of frame 0.
//
// The normative definition is the one of flow2d_compose_nodes_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// One thread per node on the 64 x 4 geometry of plane_sample.hpp (one row per thread); the node planes are addressed in 64 bits.
// A node costs the base's seven loads, then the four corners of its cell in the increment in turn, unrolled -- seven loads each (eight
// with a score), blended into seven running sums that live in registers -- and six to eight stores.  Nothing is indexed by a
// run-time value.
#include "node_grid.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kComposeCounts = 5;  // nodes, composed, no_base, outside, no_increment

struct ComposeArgs {
    const float* base[6];  // u, v, ux, uy, vx, vy of frame 0 -> frame r
    const float* base_state;
    const float* inc[6];  // the same of frame r -> frame k
    const float* inc_state;
    const float* inc_score;  // null = absent (and then out_score too)
    float* out[6];
    float* out_state;            // null = absent
    float* out_score;            // null = absent
    unsigned long long* record;  // eight words per instance, or null
    int nw, nh, npitch;
    int r, s;
    float min_state;
};

// Whether the node at `at` of a field is usable: its state at least min_state and its six values finite.
__device__ __forceinline__ bool usable_at(const float* const (&planes)[6], const float* state, float min_state, size_t at)
{
    bool ok = state[at] >= min_state;
#pragma unroll
    for (int q = 0; q < 6; ++q) ok = ok && finite(planes[q][at]);
    return ok;
}

// The float a double result is stored as: a NaN as the NaN of the header.
__device__ __forceinline__ float stored(double x) { return x == x ? static_cast<float>(x) : quiet_nan(); }

// floor(a) clamped to [0, n - 2] and the fraction a - that, clamped to [0, 1]; a lies in [-0.5, n - 0.5].
__device__ __forceinline__ void cell_of(double a, int n, int& i0, double& t)
{
    const double f = floor(a), last = static_cast<double>(n - 2);
    const double c = f < 0.0 ? 0.0 : (f > last ? last : f);
    i0 = static_cast<int>(c);
    const double d = a - c;
    t = d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d);
}

__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void compose_nodes_kernel(ComposeArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const int i = pixel_column();
    const int j = static_cast<int>(pixel_row(1, 0));
    const bool active = i < a.nw && j < a.nh;
    unsigned counts[kComposeCounts] = {0u, 0u, 0u, 0u, 0u};
    if (active) {
        const size_t at = node_at(inst, i, j, a.npitch);
        counts[0] = 1;
        bool composed = false;
        float result[6], score = quiet_nan();
#pragma unroll
        for (int q = 0; q < 6; ++q) result[q] = quiet_nan();
        if (!usable_at(a.base, a.base_state, a.min_state, at)) {
            counts[2] = 1;
        } else {
            double fa[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) fa[q] = static_cast<double>(a.base[q][at]);
            const double r = static_cast<double>(a.r), s = static_cast<double>(a.s);
            // where the base carries the node, in pixels of frame r and in nodes of the grid laid there
            const double X = (r + static_cast<double>(i) * s) + fa[0], Y = (r + static_cast<double>(j) * s) + fa[1];
            const double ga = (X - r) / s, gb = (Y - r) / s;
            const bool inside = ga >= -0.5 && ga <= static_cast<double>(a.nw) - 0.5 && gb >= -0.5 && gb <= static_cast<double>(a.nh) - 0.5;
            if (!inside) {
                counts[3] = 1;
            } else {
                int i0, j0;
                double tx, ty;
                cell_of(ga, a.nw, i0, tx);
                cell_of(gb, a.nh, j0, ty);
                double W = 0.0, sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sum_score = 0.0;
                // the corners in the header's order (0,0), (1,0), (0,1), (1,1): the usable ones add their terms, from 0
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int di = n & 1, dj = n >> 1;
                    const size_t c = node_at(inst, i0 + di, j0 + dj, a.npitch);
                    if (usable_at(a.inc, a.inc_state, a.min_state, c)) {
                        const double w = (di ? tx : 1.0 - tx) * (dj ? ty : 1.0 - ty);
                        const double dx = X - (r + static_cast<double>(i0 + di) * s), dy = Y - (r + static_cast<double>(j0 + dj) * s);
                        double fb[6];
#pragma unroll
                        for (int q = 0; q < 6; ++q) fb[q] = static_cast<double>(a.inc[q][c]);
                        W = W + w;
                        sum[0] = sum[0] + w * ((fb[0] + fb[2] * dx) + fb[3] * dy);
                        sum[1] = sum[1] + w * ((fb[1] + fb[4] * dx) + fb[5] * dy);
#pragma unroll
                        for (int q = 2; q < 6; ++q) sum[q] = sum[q] + w * fb[q];
                        if (a.inc_score) sum_score = sum_score + w * static_cast<double>(a.inc_score[c]);
                    }
                }
                if (!(W > 0.0)) {
                    counts[4] = 1;
                } else {
                    counts[1] = 1;
                    composed = true;
                    const double uB = sum[0] / W, vB = sum[1] / W, uxB = sum[2] / W, uyB = sum[3] / W, vxB = sum[4] / W, vyB = sum[5] / W;
                    const double uxA = fa[2], uyA = fa[3], vxA = fa[4], vyA = fa[5];
                    // F = F_B * F_A
                    result[0] = stored(fa[0] + uB);
                    result[1] = stored(fa[1] + vB);
                    result[2] = stored(((1.0 + uxB) * (1.0 + uxA) + uyB * vxA) - 1.0);
                    result[3] = stored((1.0 + uxB) * uyA + uyB * (1.0 + vyA));
                    result[4] = stored(vxB * (1.0 + uxA) + (1.0 + vyB) * vxA);
                    result[5] = stored((vxB * uyA + (1.0 + vyB) * (1.0 + vyA)) - 1.0);
                    score = stored(sum_score / W);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) a.out[q][at] = result[q];
        if (a.out_state) a.out_state[at] = composed ? static_cast<float>(FLOW2D_SUBSET_STATE_COMPOSED) : -1.f;
        if (a.out_score) a.out_score[at] = score;
    }
    // The record: the counts of the workgroup's four waves (one per row of the block) meet in LDS, and one thread adds them -- the
    // atomics of a whole grid land on one 64-byte line, and it is their number that the launch waits for.
    if (a.record) {
        __shared__ unsigned of_wave[flow2d::kPixelBlockY][kComposeCounts];
#pragma unroll
        for (int k = 0; k < kComposeCounts; ++k) counts[k] = wave_sum(counts[k]);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < kComposeCounts; ++k) of_wave[threadIdx.y][k] = counts[k];
        }
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
#pragma unroll
            for (int k = 0; k < kComposeCounts; ++k) {
                counts[k] = 0;
#pragma unroll
                for (int w = 0; w < flow2d::kPixelBlockY; ++w) counts[k] += of_wave[w][k];
            }
            add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
        }
    }
}

}  // namespace

extern "C" {

int flow2d_compose_nodes_2d(flow2d_context* ctx, const float* const* base, const float* const* increment,
                            const float* increment_score, size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius, int spacing,
                            int min_state, float* const* out, float* out_state, float* out_score, flow2d_compose_record* record)
{
    if (ctx == nullptr || base == nullptr || increment == nullptr || out == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::planes_ok({base[0], base[1], base[2], base[3], base[4], base[5], base[6], increment[0], increment[1], increment[2],
                            increment[3], increment[4], increment[5], increment[6], out[0], out[1], out[2], out[3], out[4], out[5]},
                           {increment_score, out_state, out_score}, nw, nh, node_pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (nw < 2 || nh < 2 || (increment_score == nullptr) != (out_score == nullptr)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (grid_radius < 1 || grid_radius > FLOW2D_CORRELATION_MAX_RADIUS || spacing < 1 || spacing > FLOW2D_CORRELATION_MAX_SPACING ||
        min_state < 0 || min_state > 1)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(record)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    // out of place: a thread reads the increment at other nodes while their threads write
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{out[0], span}, {out[1], span},   {out[2], span},   {out[3], span},
                                             {out[4], span}, {out[5], span},   {out_state, span}, {out_score, span},
                                             {record, instances * sizeof(flow2d_compose_record)}};
        flow2d::ByteRange read[15];
        for (int q = 0; q < 7; ++q) {
            read[q] = {base[q], span};
            read[7 + q] = {increment[q], span};
        }
        read[14] = {increment_score, span};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    ComposeArgs a;
    for (int q = 0; q < 6; ++q) {
        a.base[q] = base[q];
        a.inc[q] = increment[q];
        a.out[q] = out[q];
    }
    a.base_state = base[6];
    a.inc_state = increment[6];
    a.inc_score = increment_score;
    a.out_state = out_state;
    a.out_score = out_score;
    a.record = reinterpret_cast<unsigned long long*>(record);
    a.nw = static_cast<int>(nw);
    a.nh = static_cast<int>(nh);
    a.npitch = static_cast<int>(node_pitch_bytes / 4);
    a.r = grid_radius;
    a.s = spacing;
    a.min_state = static_cast<float>(min_state);
    compose_nodes_kernel<<<flow2d::pixel_grid(ctx, nw, nh, 1), flow2d::pixel_block(), 0, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
