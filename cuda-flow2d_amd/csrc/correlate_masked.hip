// The window search and the normalised median test on a region of interest for gfx950: flow2d_correlate_offset_2d and
// flow2d_validate_nodes_2d with a pixel mask in frame 0's coordinates.
//
// The normative definitions are those of flow2d_correlate_masked_2d / flow2d_validate_nodes_masked_2d in flow2d_c_abi.h.  Built
// -ffp-contract=off.  The quantisation, the window's moments, the order of the peak and the wave's peak are correlate_score.hpp's;
// the score of a displacement and the tail of a node are restated here with the mask (masked_score_at, finish_masked_node):
// score_at and finish_node stay as they are, so what correlate.hip and correlate_offset.hip compile to does not change.
//
// flow2d_correlate_masked_2d.  correlate_offset_kernel's shape: a wave per node, four waves per workgroup, the patches as bytes in
// the wave's own slice of dynamic LDS, one barrier between staging and scoring.  A third patch holds the window's mask, staged in
// the same trip as frame 0's window: 0xFF where the pixel counts, 0 where it is excluded, and frame 0's byte is staged as 0 there.
// Nv is the wave's sum of the lanes' counts.  Then the state -- centre excluded or !(Nv >= min_pixels) -- is known before the
// predictor is read, uniform over the wave: a masked node stages no search area, scores nothing and only keeps the barrier.
// Per four pixels the score reads one more dword pair (the mask's) and spends one v_and: with bm = b & m,
//   S01 += dot4(a', b),  S1 += dot4(bm, 1),  S11 += dot4(bm, bm)
// -- three packed byte dot products as in score_at.  S0 and S00 over a' are window_moments' with n = Nv.  A mask that excludes
// nothing gives a' = a, bm = b and Nv = N: the integers, and so the doubles, of correlate_offset_kernel.
//
// flow2d_validate_nodes_masked_2d.  validate_kernel with the nine mask words at the centres of the node and its ring: one thread
// per node, the neighbours as integer keys in registers, no scratch.
#include <climits>
#include <cmath>

#include "correlate_score.hpp"
#include "node_grid.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kMaskedThreads = 256, kMaskedWaves = 4;
constexpr int kValidateThreads = 256;
constexpr int kMaskedPassCounts = 7;      // the six counts of flow2d_correlation_pass_record and reserved[0], the masked nodes
constexpr int kMaskedValidateCounts = 7;  // ... of flow2d_validation_record

inline unsigned patch_bytes(int side) { return (static_cast<unsigned>(side * side) + 8u + 15u) & ~15u; }

// Excluded as the header has it: !(m < 0.5) on the float, so a NaN is excluded.
__device__ __forceinline__ bool excluded(float m) { return !(m < 0.5f); }

struct MaskedArgs {
    const float *f0, *f1, *mask;
    const float *pu, *pv;        // the predictor, both or neither
    float *nu, *nv, *ns;         // ns: null = absent
    unsigned long long* record;  // eight words per instance, or null
    int w, h, pitch;             // the frames, the mask and the predictor; pitch in floats
    int nw, nh, npitch;          // the node planes
    int r, d, s, min_pixels;
    unsigned patch0, wave_bytes;  // bytes of a wave's frame-0 patch (and of its mask patch) and of its whole slice
    float lo, scale, min_score;
};

// The offset of the header from one predictor component, which is finite.
__device__ __forceinline__ int node_offset(float p) { return static_cast<int>(floorf(fminf(fmaxf(p, -32768.f), 32768.f) + 0.5f)); }

// score_at over the window's pixels that are not excluded: nd.q0 holds 0 where the mask excludes, qm 0xFF where it does not, nd.n
// is Nv.  False when the displacement is no candidate.
__device__ __forceinline__ bool masked_score_at(const CorrNode& nd, const unsigned char* qm, int dx, int dy, double& c)
{
    const int lx = nd.left + dx, ly = nd.top + dy;
    if (lx < 0 || ly < 0 || lx + nd.side > nd.w || ly + nd.side > nd.h) return false;
    const unsigned char* p0 = nd.q0;
    const unsigned char* pm = qm;
    const unsigned char* p1 = nd.q1 + dy * nd.p1w + dx;
    unsigned s1 = 0, s11 = 0, s01 = 0;  // at most 961 * 255^2 < 2^26
    const int quads = nd.side >> 2;
    const unsigned tail = (1u << (8 * (nd.side & 3))) - 1u;
    for (int wy = 0; wy < nd.side; ++wy) {
        for (int q = 0; q < quads; ++q) {
            const unsigned a = four_pixels(p0 + 4 * q), b = four_pixels(p1 + 4 * q), bm = b & four_pixels(pm + 4 * q);
            s1 = __builtin_amdgcn_udot4(bm, 0x01010101u, s1, false);
            s11 = __builtin_amdgcn_udot4(bm, bm, s11, false);
            s01 = __builtin_amdgcn_udot4(a, b, s01, false);
        }
        // (the row's last one or three pixels: the other bytes are masked off in a and in the mask, which covers b)
        const unsigned a = four_pixels(p0 + 4 * quads) & tail, b = four_pixels(p1 + 4 * quads);
        const unsigned bm = b & (four_pixels(pm + 4 * quads) & tail);
        s1 = __builtin_amdgcn_udot4(bm, 0x01010101u, s1, false);
        s11 = __builtin_amdgcn_udot4(bm, bm, s11, false);
        s01 = __builtin_amdgcn_udot4(a, b, s01, false);
        p0 += nd.p0w;
        pm += nd.p0w;
        p1 += nd.p1w;
    }
    const long long l1 = s1;
    const long long v1 = nd.n * static_cast<long long>(s11) - l1 * l1;
    if (v1 <= 0) return false;
    const long long cov = nd.n * static_cast<long long>(s01) - nd.s0 * l1;
    c = static_cast<double>(cov) / sqrt(static_cast<double>(nd.v0) * static_cast<double>(v1));
    return true;
}

// finish_node with the masked score for the peak's four neighbours.
__device__ __forceinline__ CorrResult finish_masked_node(const CorrNode& nd, const unsigned char* qm, int d, int lane, double best, int bx,
                                                         int by, int ox, int oy, float min_score)
{
    CorrResult res;
    const bool found = best > -INFINITY;  // (a score is finite: V0 > 0 and V1 > 0)

    // the four neighbours of the peak, by lanes 0 .. 3: (-1, 0), (+1, 0), (0, -1), (0, +1)
    const bool inner = found && abs(bx) < d && abs(by) < d;
    double cn = 0.0;
    bool has = false;
    if (inner && lane < 4)
        has = masked_score_at(nd, qm, bx + (lane == 0 ? -1 : lane == 1 ? 1 : 0), by + (lane == 2 ? -1 : lane == 3 ? 1 : 0), cn);
    const bool refined = inner && (__ballot(has) & 0xFull) == 0xFull;
    const double cxm = __shfl(cn, 0, 64), cxp = __shfl(cn, 1, 64), cym = __shfl(cn, 2, 64), cyp = __shfl(cn, 3, 64);

    float score = 0.f, u = quiet_nan(), v = quiet_nan();
    bool rejected = false;
    if (found) {
        double delta_x = 0.0, delta_y = 0.0;
        if (refined) {
            const double den_x = (cxm - 2.0 * best) + cxp, den_y = (cym - 2.0 * best) + cyp;
            delta_x = den_x < 0.0 ? (cxm - cxp) / (2.0 * den_x) : 0.0;
            delta_y = den_y < 0.0 ? (cym - cyp) / (2.0 * den_y) : 0.0;
        }
        score = static_cast<float>(best);
        rejected = score < min_score;
        if (!rejected) {
            u = static_cast<float>(static_cast<double>(ox + bx) + delta_x);
            v = static_cast<float>(static_cast<double>(oy + by) + delta_y);
        }
    }
    res.u = u;
    res.v = v;
    res.score = score;
    res.found = found;
    res.rejected = rejected;
    res.refined = refined;
    return res;
}

template <typename Offset>
__global__ __launch_bounds__(kMaskedThreads) void correlate_masked_kernel(MaskedArgs a, BatchArg batch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_patches[];

    const size_t inst = batch_offset(batch);
    const float* __restrict__ f0 = a.f0 + inst;
    const float* __restrict__ f1 = a.f1 + inst;
    const float* __restrict__ mask = a.mask + inst;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int node = blockIdx.x * kMaskedWaves + wave;
    const bool active = node < a.nw * a.nh;  // (the last workgroup's surplus waves only keep the barrier)
    const int jn = active ? node / a.nw : 0, in = active ? node - jn * a.nw : 0;
    const int side = 2 * a.r + 1, d = a.d;
    const int p1w = side + 2 * d;
    const int left = in * a.s, top = jn * a.s;  // the first pixel of the node's window
    unsigned char* q0 = s_patches + static_cast<size_t>(wave) * a.wave_bytes;
    unsigned char* qm = q0 + a.patch0;
    unsigned char* q1 = qm + a.patch0;

    // frame 0 and the mask in one trip: the window of an existing node lies inside the frame
    bool masked = false;  // uniform over the wave
    int nv = 0;           // Nv
    if (active) {
        unsigned counted = 0;
        for (int i = lane; i < side * side; i += 64) {
            const int y = i / side, x = i - y * side;
            const Offset at = pixel_offset<Offset>(left + x, top + y, a.pitch);
            const bool out = excluded(load_at(mask, at));
            const unsigned q = quantise(load_at(f0, at), a.lo, a.scale);
            q0[i] = static_cast<unsigned char>(out ? 0u : q);
            qm[i] = static_cast<unsigned char>(out ? 0u : 0xFFu);
            counted += out ? 0u : 1u;
        }
        nv = static_cast<int>(wave_sum(counted));
        masked = excluded(load_at(mask, pixel_offset<Offset>(left + a.r, top + a.r, a.pitch))) || !(nv >= a.min_pixels);
    }
    const bool searching = active && !masked;

    int ox = 0, oy = 0;
    bool unpredicted = false;
    if (searching && a.pu) {
        const Offset at = pixel_offset<Offset>(left + a.r, top + a.r, a.pitch);
        const float pu = load_at(a.pu + inst, at), pv = load_at(a.pv + inst, at);
        if (finite(pu) && finite(pv)) {
            ox = node_offset(pu);
            oy = node_offset(pv);
        } else {
            unpredicted = true;
        }
    }
    if (searching) {
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

    const size_t at = node_at(inst, in, jn, a.npitch);
    if (masked) {
        if (lane != 0) return;
        a.nu[at] = quiet_nan();
        a.nv[at] = quiet_nan();
        if (a.ns) a.ns[at] = 0.f;
        if (a.record) {
            const unsigned counts[kMaskedPassCounts] = {1u, 0u, 0u, 0u, 0u, 0u, 1u};
            add_counts<kCountRecordWords>(a.record, blockIdx.z, counts);
        }
        return;
    }

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
    nd.n = nv;
    window_moments(nd, lane);

    const int reach = 2 * d + 1, candidates = reach * reach;
    double best = -INFINITY;  // no candidate yet
    int bx = 0, by = 0;
    unsigned scored = 0;
    if (nd.v0 > 0) {
        for (int k = lane; k < candidates; k += 64) {
            const int ky = k / reach, dx = k - ky * reach - d, dy = ky - d;
            double c;
            if (masked_score_at(nd, qm, dx, dy, c)) {
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
    const CorrResult res = finish_masked_node(nd, qm, d, lane, best, bx, by, ox, oy, a.min_score);
    if (lane != 0) return;
    a.nu[at] = res.u;
    a.nv[at] = res.v;
    if (a.ns) a.ns[at] = res.score;
    if (a.record) {
        const unsigned counts[kMaskedPassCounts] = {1u, !res.found, res.rejected, res.found && !res.rejected && !res.refined, unpredicted,
                                                    scored, 0u};
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

struct MaskedValidateArgs {
    const float *nu, *nv, *mask;
    float *ou, *ov, *flag;       // flag: null = absent
    unsigned long long* record;  // eight words per instance, or null
    int nw, nh, npitch;
    int pitch, r, s;  // the mask's pitch in floats and the grid's geometry: node (i, j) is centred on pixel (r + i*s, r + j*s)
    float threshold, epsilon;
    int min_neighbours, replace;
};

__global__ __launch_bounds__(kValidateThreads) void validate_masked_kernel(MaskedValidateArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const float* __restrict__ nu = a.nu + inst;
    const float* __restrict__ nv = a.nv + inst;
    const float* __restrict__ mask = a.mask + inst;
    const int lane = threadIdx.x & 63;
    const unsigned node = blockIdx.x * kValidateThreads + threadIdx.x;
    const bool active = node < static_cast<unsigned>(a.nw) * static_cast<unsigned>(a.nh);
    // nodes, judged, outliers, filled, unjudged, remaining_invalid, masked
    unsigned counts[kMaskedValidateCounts] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    // whether node (x, y), which lies inside the grid, is off the specimen (the mask is addressed in 64 bits)
    auto off = [&](int x, int y) {
        return excluded(mask[static_cast<size_t>(a.r + y * a.s) * static_cast<size_t>(a.pitch) + static_cast<size_t>(a.r + x * a.s)]);
    };
    if (active) {
        const int j = node / a.nw, i = node - j * a.nw;
        const size_t at = node_at(0, i, j, a.npitch);
        counts[0] = 1;
        if (off(i, j)) {
            counts[6] = 1;
            a.ou[inst + at] = quiet_nan();
            a.ov[inst + at] = quiet_nan();
            if (a.flag) a.flag[inst + at] = 3.f;
        } else {
            int ku[8], kv[8];
            int k = 0;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                int dx, dy;
                ring_neighbour(n, dx, dy);
                const int x = i + dx, y = j + dy;
                ku[n] = INT_MAX;
                kv[n] = INT_MAX;
                if (x >= 0 && y >= 0 && x < a.nw && y < a.nh && !off(x, y)) {
                    const size_t nat = node_at(0, x, y, a.npitch);
                    const float u = nu[nat], v = nv[nat];
                    if (finite(u) && finite(v)) {
                        ku[n] = float_key(u);
                        kv[n] = float_key(v);
                        k += 1;
                    }
                }
            }
            const float u = nu[at], v = nv[at];
            const bool valid = finite(u) && finite(v);
            float out_u = u, out_v = v, flag = 0.f;
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
    }
    if (a.record) add_wave_counts<kCountRecordWords>(a.record, blockIdx.z, lane, counts);
}

}  // namespace

extern "C" {

int flow2d_correlate_masked_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* predictor_u,
                               const float* predictor_v, size_t width, size_t height, size_t pitch_bytes, float lo, float scale,
                               int radius, int range, int spacing, float min_score, const float* mask, int min_pixels, float* node_u,
                               float* node_v, float* node_score, size_t node_pitch_bytes, flow2d_correlation_pass_record* record)
{
    if (mask == nullptr)
        return flow2d_correlate_offset_2d(ctx, frame_0, frame_1, predictor_u, predictor_v, width, height, pitch_bytes, lo, scale, radius,
                                          range, spacing, min_score, node_u, node_v, node_score, node_pitch_bytes, record);
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if ((predictor_u == nullptr) != (predictor_v == nullptr)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::planes_ok({frame_0, frame_1, mask}, {predictor_u, predictor_v}, width, height, pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::correlation_grid_ok(width, height, radius, spacing) || range < 1 || range > FLOW2D_CORRELATION_MAX_RANGE)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const int side = 2 * radius + 1;
    if (min_pixels < 1 || min_pixels > side * side) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(std::isfinite(scale) && scale > 0.f) || !std::isfinite(lo) || std::isnan(min_score)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const size_t nw = flow2d::correlation_nodes(width, radius, spacing), nh = flow2d::correlation_nodes(height, radius, spacing);
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    if (!flow2d::planes_ok({node_u, node_v}, {node_score}, nw, nh, node_pitch_bytes) || !flow2d::record_aligned(record))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks the frames and the mask __restrict__: no written byte range may meet a plane that is read or another written one
    auto aliased = [&](size_t frame_span, size_t node_span, size_t instances) {
        const flow2d::ByteRange written[] = {{node_u, node_span}, {node_v, node_span}, {node_score, node_span},
                                             {record, instances * sizeof(flow2d_correlation_pass_record)}};
        const flow2d::ByteRange read[] = {{frame_0, frame_span}, {frame_1, frame_span}, {predictor_u, frame_span},
                                          {predictor_v, frame_span}, {mask, frame_span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), flow2d::batch_span(ctx, nh * node_pitch_bytes), instances))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    // a wave's slice: frame 0's window, its mask, the search area -- at most 976 + 976 + 9040 bytes, four of them in 64 KB
    const unsigned patch0 = patch_bytes(side), wave_bytes = 2 * patch0 + patch_bytes(side + 2 * range);
    const MaskedArgs a = {frame_0, frame_1, mask, predictor_u, predictor_v, node_u, node_v, node_score,
                          reinterpret_cast<unsigned long long*>(record),
                          static_cast<int>(width), static_cast<int>(height), static_cast<int>(pitch_bytes / 4),
                          static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                          radius, range, spacing, min_pixels, patch0, wave_bytes, lo, scale, min_score};
    // (the largest offset a lane forms into a frame is below height * pitch_bytes; the node planes are addressed in 64 bits)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        correlate_masked_kernel<decltype(offset)><<<dim3(flow2d::div_up(nw * nh, kMaskedWaves), 1, flow2d::batch_z(ctx, 1)),
                                                    dim3(kMaskedThreads), kMaskedWaves * wave_bytes, ctx->stream>>>(
            a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

int flow2d_validate_nodes_masked_2d(flow2d_context* ctx, const float* node_u, const float* node_v, size_t nw, size_t nh,
                                    size_t node_pitch_bytes, float threshold, float epsilon, int min_neighbours, int mode,
                                    const float* mask, size_t width, size_t height, size_t pitch_bytes, int radius, int spacing,
                                    float* out_u, float* out_v, float* out_flag, flow2d_validation_record* record)
{
    if (mask == nullptr)
        return flow2d_validate_nodes_2d(ctx, node_u, node_v, nw, nh, node_pitch_bytes, threshold, epsilon, min_neighbours, mode, out_u,
                                        out_v, out_flag, record);
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::planes_ok({node_u, node_v, out_u, out_v}, {out_flag}, nw, nh, node_pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (min_neighbours < 1 || min_neighbours > 8 || !(std::isfinite(threshold) && threshold > 0.f) ||
        !(std::isfinite(epsilon) && epsilon > 0.f) || (mode != FLOW2D_VALIDATE_FLAG && mode != FLOW2D_VALIDATE_REPLACE))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(record)) return FLOW2D_ERR_INVALID_ARGUMENT;
    // the mask is a plane of the frames, and the grid is the one flow2d_correlation_grid gives for it
    if (!flow2d::planes_ok({mask}, {}, width, height, pitch_bytes) || !flow2d::correlation_grid_ok(width, height, radius, spacing) ||
        nw != flow2d::correlation_nodes(width, radius, spacing) || nh != flow2d::correlation_nodes(height, radius, spacing))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    auto aliased = [&](size_t span, size_t mask_span, size_t instances) {
        const flow2d::ByteRange written[] = {{out_u, span}, {out_v, span}, {out_flag, span},
                                             {record, instances * sizeof(flow2d_validation_record)}};
        const flow2d::ByteRange read[] = {{node_u, span}, {node_v, span}, {mask, mask_span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), flow2d::batch_span(ctx, height * pitch_bytes), instances))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(flow2d::clear_records(ctx, record));
    const MaskedValidateArgs a = {node_u, node_v, mask, out_u, out_v, out_flag, reinterpret_cast<unsigned long long*>(record),
                                  static_cast<int>(nw), static_cast<int>(nh), static_cast<int>(node_pitch_bytes / 4),
                                  static_cast<int>(pitch_bytes / 4), radius, spacing,
                                  threshold, epsilon, min_neighbours, mode == FLOW2D_VALIDATE_REPLACE ? 1 : 0};
    validate_masked_kernel<<<dim3(flow2d::div_up(nw * nh, kValidateThreads), 1, flow2d::batch_z(ctx, 1)), dim3(kValidateThreads), 0,
                             ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
