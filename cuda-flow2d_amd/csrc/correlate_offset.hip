// Multi-pass window correlation for gfx950: the window search around a per-node predictor offset (discrete window offset) and the
// normalised median test of a node field against its neighbours, with replacement.
//
// The normative definitions are those of flow2d_correlate_offset_2d / flow2d_validate_nodes_2d in flow2d_c_abi.h.  Built
// -ffp-contract=off.  The scoring code is correlate_score.hpp, the one flow2d_correlate_2d runs.
//
// flow2d_correlate_offset_2d.  The offset differs from node to node, so the nodes of a tile no longer share one search area of
// frame 1: a wave stages its own node -- the window of frame 0 (at most 31 x 31 bytes) and the search area of frame 1 around the
// offset (at most 95 x 95; what lies outside frame 1 is staged as 0 and never scored: a candidate's window lies inside the frame)
// -- in its own slice of dynamic LDS, each patch 16-byte aligned with 8 bytes of slack behind it (four_pixels reads the aligned
// dword pair around any byte).  The slices are sized by the call's radius and range: 1.2 KB per wave on the PIV grid (7, 8),
// 9.8 KB at the limits (15, 32).  A workgroup is four waves, one node each; they meet at one barrier between staging and scoring
// and share nothing else.  Then, as in correlate_kernel: S0 and S00 by a butterfly, the lanes share the (2d + 1)^2
// displacements, the wave's peak, the four neighbours by lanes 0 .. 3, lane 0 writes.  The six counts go to the record by 64-bit
// integer atomics, one set per wave, after the entry has zeroed the record on the stream.
// Overlapping windows of neighbouring nodes are read from memory once per node here and once per tile there: on a grid whose
// nodes all have the same offset this kernel does more loads for the same arithmetic (DESIGN.md 3.16 has the measurement).
//
// flow2d_validate_nodes_2d.  One thread per node: the up to eight finite neighbours of the 3 x 3 ring as order-preserving integer
// keys in registers, an odd-even transposition network of 8 (absent ones sort last as INT_MAX), the two middle elements picked by
// selects -- no indexed register array, no scratch.  Out of place, so no order of the nodes matters.
#include <climits>
#include <cmath>

#include "correlate_score.hpp"
#include "node_grid.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kOffsetThreads = 256, kOffsetWaves = 4;
constexpr int kValidateThreads = 256;
constexpr int kPassCounts = 6;      // the counts of flow2d_correlation_pass_record that are written
constexpr int kValidateCounts = 6;  // ... of flow2d_validation_record

inline unsigned patch_bytes(int side) { return (static_cast<unsigned>(side * side) + 8u + 15u) & ~15u; }

struct OffsetArgs {
    const float *f0, *f1;
    const float *pu, *pv;        // the predictor, both or neither
    float *nu, *nv, *ns;         // ns: null = absent
    unsigned long long* record;  // eight words per instance, or null
    int w, h, pitch;             // the frames and the predictor; pitch in floats
    int nw, nh, npitch;          // the node planes
    int r, d, s;
    unsigned patch0, wave_bytes;  // bytes of a wave's frame-0 patch and of its whole slice
    float lo, scale, min_score;
};

// The offset of the header from one predictor component, which is finite.
__device__ __forceinline__ int node_offset(float p) { return static_cast<int>(floorf(fminf(fmaxf(p, -32768.f), 32768.f) + 0.5f)); }

template <typename Offset>
__global__ __launch_bounds__(kOffsetThreads) void correlate_offset_kernel(OffsetArgs a, BatchArg batch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_patches[];

    const size_t inst = batch_offset(batch);
    const float* __restrict__ f0 = a.f0 + inst;
    const float* __restrict__ f1 = a.f1 + inst;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node = blockIdx.x * kOffsetWaves + wave;
    const bool active = node < a.nw * a.nh;  // (the last workgroup's surplus waves only keep the barrier)
    const int jn = active ? node / a.nw : 0, in = active ? node - jn * a.nw : 0;
    const int side = 2 * a.r + 1, d = a.d;
    const int p1w = side + 2 * d;
    const int left = in * a.s, top = jn * a.s;  // the first pixel of the node's window
    unsigned char* q0 = s_patches + static_cast<size_t>(wave) * a.wave_bytes;
    unsigned char* q1 = q0 + a.patch0;

    int ox = 0, oy = 0;
    bool unpredicted = false;
    if (active && a.pu) {
        const Offset at = pixel_offset<Offset>(left + a.r, top + a.r, a.pitch);
        const float pu = load_at(a.pu + inst, at), pv = load_at(a.pv + inst, at);
        if (finite(pu) && finite(pv)) {
            ox = node_offset(pu);
            oy = node_offset(pv);
        } else {
            unpredicted = true;
        }
    }
    if (active) {
        // frame 0: the window of an existing node lies inside the frame
        for (int i = lane; i < side * side; i += 64) {
            const int y = i / side, x = i - y * side;
            q0[i] = static_cast<unsigned char>(quantise(load_at(f0, pixel_offset<Offset>(left + x, top + y, a.pitch)), a.lo, a.scale));
        }
        // frame 1 around the offset: what lies outside the frame is not loaded, and never scored
        const int x1 = left + ox - d, y1 = top + oy - d;
        for (int i = lane; i < p1w * p1w; i += 64) {
            const int y = i / p1w, x = i - y * p1w;
            const int gx = x1 + x, gy = y1 + y;
            unsigned q = 0;
            if (gx >= 0 && gy >= 0 && gx < a.w && gy < a.h) q = quantise(load_at(f1, pixel_offset<Offset>(gx, gy, a.pitch)), a.lo, a.scale);
            q1[i] = static_cast<unsigned char>(q);
        }
    }
    __syncthreads();
    if (!active) return;

    CorrNode nd;
    nd.q0 = q0;
    nd.q1 = q1 + d * p1w + d;
    nd.p0w = side;
    nd.p1w = p1w;
    nd.left = left + ox;
    nd.top = top + oy;
    nd.w = a.w;
    nd.h = a.h;
    nd.side = side;
    nd.n = side * side;
    window_moments(nd, lane);

    const int reach = 2 * d + 1, candidates = reach * reach;
    double best = -INFINITY;  // no candidate yet
    int bx = 0, by = 0;
    unsigned scored = 0;
    if (nd.v0 > 0) {
        for (int k = lane; k < candidates; k += 64) {
            const int ky = k / reach, dx = k - ky * reach - d, dy = ky - d;
            double c;
            if (score_at(nd, dx, dy, c)) {
                scored += 1;
                if (comes_first(c, dx, dy, best, bx, by)) {
                    best = c;
                    bx = dx;
                    by = dy;
                }
            }
        }
        wave_peak(best, bx, by);
        scored = wave_sum(scored);
    }
    const CorrResult res = finish_node(nd, d, lane, best, bx, by, ox, oy, a.min_score);
    if (lane != 0) return;
    const size_t at = node_at(inst, in, jn, a.npitch);
    a.nu[at] = res.u;
    a.nv[at] = res.v;
    if (a.ns) a.ns[at] = res.score;
    if (a.record) {
        const unsigned counts[kPassCounts] = {1u, !res.found, res.rejected, res.found && !res.rejected && !res.refined, unpredicted, scored};
        add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
    }
}

// ---- validation ---------------------------------------------------------------------------------------------------------------------
// The order-preserving integer key of a float (-0 < +0) and back.
__device__ __forceinline__ int float_key(float x)
{
    const int b = __float_as_int(x);
    return b ^ ((b >> 31) & 0x7FFFFFFF);
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7FFFFFFF)); }

// Sorts the eight keys (absent ones are INT_MAX and end up last).
__device__ __forceinline__ void sort8(int (&a)[8])
{
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
#pragma unroll
        for (int i = pass & 1; i + 1 < 8; i += 2) {
            const int lo = min(a[i], a[i + 1]), hi = max(a[i], a[i + 1]);
            a[i] = lo;
            a[i + 1] = hi;
        }
    }
}

// The median of the header of the first k (1 .. 8) of the sorted keys.
__device__ __forceinline__ float median_sorted(const int (&a)[8], int k)
{
    const int i0 = (k - 1) >> 1, i1 = k >> 1;
    int m0 = a[0], m1 = a[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        m0 = i == i0 ? a[i] : m0;
        m1 = i == i1 ? a[i] : m1;
    }
    return (key_float(m0) + key_float(m1)) * 0.5f;
}

struct ValidateArgs {
    const float *nu, *nv;
    float *ou, *ov, *flag;       // flag: null = absent
    unsigned long long* record;  // eight words per instance, or null
    int nw, nh, npitch;
    float threshold, epsilon;
    int min_neighbours, replace;
};

__global__ __launch_bounds__(kValidateThreads) void validate_kernel(ValidateArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const float* __restrict__ nu = a.nu + inst;
    const float* __restrict__ nv = a.nv + inst;
    const int lane = threadIdx.x & 63;
    const unsigned node = blockIdx.x * kValidateThreads + threadIdx.x;
    const bool active = node < static_cast<unsigned>(a.nw) * static_cast<unsigned>(a.nh);
    unsigned counts[kValidateCounts] = {0u, 0u, 0u, 0u, 0u, 0u};  // nodes, judged, outliers, filled, unjudged, remaining_invalid
    if (active) {
        const int j = node / a.nw, i = node - j * a.nw;
        int ku[8], kv[8];
        int k = 0;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            int dx, dy;
            ring_neighbour(n, dx, dy);
            const int x = i + dx, y = j + dy;
            ku[n] = INT_MAX;
            kv[n] = INT_MAX;
            if (x >= 0 && y >= 0 && x < a.nw && y < a.nh) {
                const size_t at = node_at(0, x, y, a.npitch);
                const float u = nu[at], v = nv[at];
                if (finite(u) && finite(v)) {
                    ku[n] = float_key(u);
                    kv[n] = float_key(v);
                    k += 1;
                }
            }
        }
        const size_t at = node_at(0, i, j, a.npitch);
        const float u = nu[at], v = nv[at];
        const bool valid = finite(u) && finite(v);
        float out_u = u, out_v = v, flag = 0.f;
        counts[0] = 1;
        if (k < a.min_neighbours) {
            counts[4] = 1;
        } else {
            sort8(ku);
            sort8(kv);
            const float mu = median_sorted(ku, k), mv = median_sorted(kv, k);
            if (valid) {
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    ku[n] = n < k ? float_key(fabsf(key_float(ku[n]) - mu)) : INT_MAX;
                    kv[n] = n < k ? float_key(fabsf(key_float(kv[n]) - mv)) : INT_MAX;
                }
                sort8(ku);
                sort8(kv);
                const float ru = median_sorted(ku, k), rv = median_sorted(kv, k);
                const float tu = fabsf(u - mu) / (ru + a.epsilon), tv = fabsf(v - mv) / (rv + a.epsilon);
                counts[1] = 1;
                if (tu > a.threshold || tv > a.threshold) {
                    counts[2] = 1;
                    flag = 1.f;
                    out_u = a.replace ? mu : quiet_nan();
                    out_v = a.replace ? mv : quiet_nan();
                }
            } else if (a.replace) {
                counts[3] = 1;
                flag = 2.f;
                out_u = mu;
                out_v = mv;
            }
        }
        counts[5] = !(finite(out_u) && finite(out_v));
        a.ou[inst + at] = out_u;
        a.ov[inst + at] = out_v;
        if (a.flag) a.flag[inst + at] = flag;
    }
    if (a.record) add_wave_counts<kCountRecordWords>(a.record, blockIdx.z, lane, counts);
}

}  // namespace

extern "C" {

int flow2d_correlate_offset_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* predictor_u,
                               const float* predictor_v, size_t width, size_t height, size_t pitch_bytes, float lo, float scale,
                               int radius, int range, int spacing, float min_score, float* node_u, float* node_v, float* node_score,
                               size_t node_pitch_bytes, flow2d_correlation_pass_record* record)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if ((predictor_u == nullptr) != (predictor_v == nullptr)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::planes_ok({frame_0, frame_1}, {predictor_u, predictor_v}, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::correlation_grid_ok(width, height, radius, spacing) || range < 1 || range > FLOW2D_CORRELATION_MAX_RANGE)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(std::isfinite(scale) && scale > 0.f) || !std::isfinite(lo) || std::isnan(min_score)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const size_t nw = flow2d::correlation_nodes(width, radius, spacing), nh = flow2d::correlation_nodes(height, radius, spacing);
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    if (!flow2d::planes_ok({node_u, node_v}, {node_score}, nw, nh, node_pitch_bytes) || !flow2d::record_aligned(record))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks the frames __restrict__: no written byte range may meet a plane that is read or another written one
    auto aliased = [&](size_t frame_span, size_t node_span, size_t instances) {
        const flow2d::ByteRange written[] = {{node_u, node_span}, {node_v, node_span}, {node_score, node_span},
                                             {record, instances * sizeof(flow2d_correlation_pass_record)}};
        const flow2d::ByteRange read[] = {{frame_0, frame_span}, {frame_1, frame_span}, {predictor_u, frame_span}, {predictor_v, frame_span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), flow2d::batch_span(ctx, nh * node_pitch_bytes), instances))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    const int side = 2 * radius + 1;
    const unsigned patch0 = patch_bytes(side), wave_bytes = patch0 + patch_bytes(side + 2 * range);  // at most 976 + 9040
    const OffsetArgs a = {frame_0, frame_1, predictor_u, predictor_v, node_u, node_v, node_score,
                          reinterpret_cast<unsigned long long*>(record),
                          static_cast<int>(width), static_cast<int>(height), static_cast<int>(pitch_bytes / 4),
                          static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                          radius, range, spacing, patch0, wave_bytes, lo, scale, min_score};
    // (the largest offset a lane forms into a frame is below height * pitch_bytes; the node planes are addressed in 64 bits)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        correlate_offset_kernel<decltype(offset)><<<dim3(flow2d::div_up(nw * nh, kOffsetWaves), 1, flow2d::batch_z(ctx, 1)),
                                                    dim3(kOffsetThreads), kOffsetWaves * wave_bytes, ctx->stream>>>(
            a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

int flow2d_validate_nodes_2d(flow2d_context* ctx, const float* node_u, const float* node_v, size_t nw, size_t nh,
                             size_t node_pitch_bytes, float threshold, float epsilon, int min_neighbours, int mode, float* out_u,
                             float* out_v, float* out_flag, flow2d_validation_record* record)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::planes_ok({node_u, node_v, out_u, out_v}, {out_flag}, nw, nh, node_pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (min_neighbours < 1 || min_neighbours > 8 || !(std::isfinite(threshold) && threshold > 0.f) ||
        !(std::isfinite(epsilon) && epsilon > 0.f) || (mode != FLOW2D_VALIDATE_FLAG && mode != FLOW2D_VALIDATE_REPLACE))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(record)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{out_u, span}, {out_v, span}, {out_flag, span},
                                             {record, instances * sizeof(flow2d_validation_record)}};
        const flow2d::ByteRange read[] = {{node_u, span}, {node_v, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    const ValidateArgs a = {node_u, node_v, out_u, out_v, out_flag, reinterpret_cast<unsigned long long*>(record),
                            static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                            threshold, epsilon, min_neighbours, mode == FLOW2D_VALIDATE_REPLACE ? 1 : 0};
    validate_kernel<<<dim3(flow2d::div_up(nw * nh, kValidateThreads), 1, flow2d::batch_z(ctx, 1)), dim3(kValidateThreads), 0, ctx->stream>>>(
        a, flow2d::batch_arg(ctx, 1));
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
