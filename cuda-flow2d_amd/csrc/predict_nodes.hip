// The start of the next step of a DIC sequence from a step's result, for gfx950: usable nodes are kept, the others predicted
// from their usable neighbours' first-order extrapolations by a median.
//
// The normative definition is the one of flow2d_predict_nodes_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// One thread per node on the 64 x 4 geometry of plane_sample.hpp (one row per thread); the node planes are addressed in 64 bits.
// A kept node costs seven loads and seven stores.  A node to be predicted first finds which of its eight neighbours are usable
// (seven loads each), then takes the six outputs in turn: the up to eight candidates of one output live in registers, and the
// median is found by rank -- candidate i comes after candidate j when c[j] < c[i], or when neither is below the other and
// j < i -- so that nothing is sorted and no array is indexed by a run-time value.
#include "node_grid.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kPredictCounts = 4;  // nodes, kept, predicted, empty

struct PredictArgs {
    const float* in[6];  // u, v, ux, uy, vx, vy
    const float* state;
    float* out[6];
    float* out_state;            // null = absent
    unsigned long long* record;  // eight words per instance, or null
    int nw, nh, npitch;
    int s, min_neighbours;
    float min_state;
};

// Whether the node at `at` is usable: its state at least min_state and its six values finite.
__device__ __forceinline__ bool usable_at(const PredictArgs& a, size_t at)
{
    bool ok = a.state[at] >= a.min_state;
#pragma unroll
    for (int q = 0; q < 6; ++q) ok = ok && finite(a.in[q][at]);
    return ok;
}

// The median of the header over the candidates whose bit of `mask` is set; m = popcount(mask) >= 1.
__device__ __forceinline__ float median_by_rank(const double (&c)[8], unsigned mask, int m)
{
    const int hi = m >> 1, lo = (m & 1) ? hi : hi - 1;
    double at_lo = 0.0, at_hi = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j == i) continue;
            const bool before = c[j] < c[i] || (j < i && !(c[i] < c[j]));
            rank += ((mask >> j) & 1u) && before ? 1 : 0;
        }
        const bool live = (mask >> i) & 1u;
        at_lo = live && rank == lo ? c[i] : at_lo;
        at_hi = live && rank == hi ? c[i] : at_hi;
    }
    return static_cast<float>((m & 1) ? at_hi : (at_lo + at_hi) * 0.5);
}

__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void predict_nodes_kernel(PredictArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const int i = pixel_column();
    const int j = static_cast<int>(pixel_row(1, 0));
    const bool active = i < a.nw && j < a.nh;
    unsigned counts[kPredictCounts] = {0u, 0u, 0u, 0u};
    if (active) {
        const size_t at = node_at(inst, i, j, a.npitch);
        counts[0] = 1;
        if (usable_at(a, at)) {
            counts[1] = 1;
#pragma unroll
            for (int q = 0; q < 6; ++q) a.out[q][at] = a.in[q][at];
            if (a.out_state) a.out_state[at] = a.state[at];
        } else {
            // the ring in the header's order: the 3 x 3 block without its centre, row by row
            unsigned mask = 0;
            size_t where[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                int di, dj;
                ring_neighbour(n, di, dj);
                const int x = i + di, y = j + dj;
                where[n] = at;
                if (x >= 0 && y >= 0 && x < a.nw && y < a.nh) {
                    where[n] = node_at(inst, x, y, a.npitch);
                    mask |= usable_at(a, where[n]) ? 1u << n : 0u;
                }
            }
            const int m = __popc(mask);
            if (m >= a.min_neighbours) {
                counts[2] = 1;
                double c[8];
                // u and v: the neighbour's plane through this node, (value + gx*dx) + gy*dy with dx = -di*s, dy = -dj*s
#pragma unroll
                for (int q = 0; q < 2; ++q) {
#pragma unroll
                    for (int n = 0; n < 8; ++n) {
                        int di, dj;
                        ring_neighbour(n, di, dj);
                        const double dx = static_cast<double>(-di * a.s), dy = static_cast<double>(-dj * a.s);
                        c[n] = 0.0;
                        if ((mask >> n) & 1u)
                            c[n] = (static_cast<double>(a.in[q][where[n]]) + static_cast<double>(a.in[2 + 2 * q][where[n]]) * dx) +
                                   static_cast<double>(a.in[3 + 2 * q][where[n]]) * dy;
                    }
                    a.out[q][at] = median_by_rank(c, mask, m);
                }
#pragma unroll
                for (int q = 2; q < 6; ++q) {
#pragma unroll
                    for (int n = 0; n < 8; ++n) c[n] = (mask >> n) & 1u ? static_cast<double>(a.in[q][where[n]]) : 0.0;
                    a.out[q][at] = median_by_rank(c, mask, m);
                }
                if (a.out_state) a.out_state[at] = static_cast<float>(FLOW2D_SUBSET_STATE_PREDICTED);
            } else {
                counts[3] = 1;
#pragma unroll
                for (int q = 0; q < 6; ++q) a.out[q][at] = quiet_nan();
                if (a.out_state) a.out_state[at] = -1.f;
            }
        }
    }
    if (a.record) add_wave_counts<kCountRecordWords>(a.record, blockIdx.z, threadIdx.x & 63, counts);
}

}  // namespace

extern "C" {

int flow2d_predict_nodes_2d(flow2d_context* ctx, const float* node_u, const float* node_v, const float* node_ux, const float* node_uy,
                            const float* node_vx, const float* node_vy, const float* node_state, size_t nw, size_t nh,
                            size_t node_pitch_bytes, int spacing, int min_state, int min_neighbours, float* out_u, float* out_v,
                            float* out_ux, float* out_uy, float* out_vx, float* out_vy, float* out_state, flow2d_predict_record* record)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float* const in[] = {node_u, node_v, node_ux, node_uy, node_vx, node_vy};
    float* const out[] = {out_u, out_v, out_ux, out_uy, out_vx, out_vy};
    if (!flow2d::planes_ok({node_u, node_v, node_ux, node_uy, node_vx, node_vy, node_state, out_u, out_v, out_ux, out_uy, out_vx, out_vy},
                           {out_state}, nw, nh, node_pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (spacing < 1 || spacing > FLOW2D_CORRELATION_MAX_SPACING || min_state < 0 || min_state > 1 || min_neighbours < 1 ||
        min_neighbours > 8)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(record)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    // out of place: a thread reads its neighbours' inputs while their threads write
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{out_u, span},  {out_v, span},  {out_ux, span},    {out_uy, span},
                                             {out_vx, span}, {out_vy, span}, {out_state, span}, {record, instances * sizeof(flow2d_predict_record)}};
        const flow2d::ByteRange read[] = {{node_u, span},  {node_v, span},  {node_ux, span},   {node_uy, span},
                                          {node_vx, span}, {node_vy, span}, {node_state, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    PredictArgs a;
    for (int q = 0; q < 6; ++q) {
        a.in[q] = in[q];
        a.out[q] = out[q];
    }
    a.state = node_state;
    a.out_state = out_state;
    a.record = reinterpret_cast<unsigned long long*>(record);
    a.nw = static_cast<int>(nw);
    a.nh = static_cast<int>(nh);
    a.npitch = static_cast<int>(node_pitch_bytes / 4);
    a.s = spacing;
    a.min_neighbours = min_neighbours;
    a.min_state = static_cast<float>(min_state);
    predict_nodes_kernel<<<flow2d::pixel_grid(ctx, nw, nh, 1), flow2d::pixel_block(), 0, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
