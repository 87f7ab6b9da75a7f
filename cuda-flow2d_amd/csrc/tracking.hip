// Dense point trajectories (Sundaram, Brox & Keutzer, ECCV 2010) for gfx950: no reference counterpart.
//
// flow2d_track_points_2d advances a table of tracks by one flow step; flow2d_seed_points_2d appends tracks in uncovered,
// textured cells.  The normative definitions are those in flow2d_c_abi.h; the bilinear sample is the operation order of
// flow2d_consistency_2d.  Built -ffp-contract=off: positions and seeds follow those definitions bit for bit.
//
// Track step: one lane per slot, a gather of two flow pairs at the track's sub-pixel position (and five taps per plane for
// the motion-boundary test) plus 16 bytes of table per slot.  Slot indices are 64-bit (size_t) and the grid strides over
// the table, so any capacity below 2^40 is indexed.
//
// Seeding: five launches, no atomics, no host synchronisation.  clear -> mark (every live track flags its cell) ->
// decide (per cell: uncovered and lambda_min >= threshold; a per-block count) -> scan (one workgroup, the block counts in
// block order) -> write (per block: its offset plus the rank of the cell among the block's seeds).  The slot a cell gets
// depends only on the cell order, so repeated calls and graph replays write identical bytes.
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kThreads = 256;               // track / mark / decide / write: one workgroup of four waves
constexpr int kScanThreads = 1024;          // scan: one workgroup
constexpr unsigned kMaxBlocks = 1u << 20;   // grid-stride launches over the table use at most this many workgroups
constexpr size_t kMaxCapacity = size_t(1) << 40;
constexpr size_t kMaxCells = size_t(1) << 32;
constexpr float kNaN = __builtin_nanf("");

// Workspace of flow2d_seed_points_2d: a header, the per-block offsets, the per-block counts, one byte per cell
struct SeedHeader {
    unsigned long long base;   // *count before the call
    unsigned long long avail;  // free slots: capacity - base (0 when the table is full)
    unsigned long long pad[2];
};
static_assert(sizeof(SeedHeader) == 32, "header keeps the arrays 16-byte aligned");

__host__ __device__ __forceinline__ size_t min_size(size_t a, size_t b) { return a < b ? a : b; }

inline size_t round16(size_t b) { return (b + 15) & ~size_t(15); }

struct SeedLayout {
    size_t cells_x, cells_y, cells, blocks;
    size_t offsets, counts, flags, flags_bytes, total;
};

SeedLayout seed_layout(size_t width, size_t height, size_t spacing)
{
    SeedLayout l{};
    l.cells_x = (width + spacing - 1) / spacing;
    l.cells_y = (height + spacing - 1) / spacing;
    l.cells = l.cells_x * l.cells_y;
    l.blocks = (l.cells + kThreads - 1) / kThreads;
    l.offsets = sizeof(SeedHeader);
    l.counts = l.offsets + round16(l.blocks * sizeof(unsigned long long));
    l.flags = l.counts + round16(l.blocks * sizeof(unsigned));
    l.flags_bytes = round16(l.cells);
    l.total = l.flags + l.flags_bytes;
    return l;
}

// The four taps and weights of the bilinear sample S of flow2d_consistency_2d at a position inside the frame
struct Bilinear {
    size_t o00, o01, o10, o11;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ Bilinear bilinear(float px, float py, int w, int h, size_t pitch)
{
    const int x = static_cast<int>(floorf(px));
    const int y = static_cast<int>(floorf(py));
    const float dx = px - static_cast<float>(x);
    const float dy = py - static_cast<float>(y);
    const int x1 = min(w - 1, x + 1);
    const int y1 = min(h - 1, y + 1);
    Bilinear b;
    b.o00 = static_cast<size_t>(y) * pitch + static_cast<size_t>(x);
    b.o01 = static_cast<size_t>(y) * pitch + static_cast<size_t>(x1);
    b.o10 = static_cast<size_t>(y1) * pitch + static_cast<size_t>(x);
    b.o11 = static_cast<size_t>(y1) * pitch + static_cast<size_t>(x1);
    b.w00 = (1.f - dx) * (1.f - dy);
    b.w01 = (dx) * (1.f - dy);
    b.w10 = (1.f - dx) * (dy);
    b.w11 = (dx) * (dy);
    return b;
}

__device__ __forceinline__ float sample(const float* __restrict__ p, const Bilinear& b)
{
    return b.w00 * p[b.o00] + b.w01 * p[b.o01] + b.w10 * p[b.o10] + b.w11 * p[b.o11];
}

__device__ __forceinline__ float at(const float* __restrict__ p, size_t pitch, int x, int y)
{
    return p[static_cast<size_t>(y) * pitch + static_cast<size_t>(x)];
}

__device__ __forceinline__ bool inside(float x, float y, float x_max, float y_max)
{
    return x >= 0.f && x <= x_max && y >= 0.f && y <= y_max;  // false for a NaN
}

struct TrackArgs {
    const float* flow_u;
    const float* flow_v;
    const float* back_u;  // null: no forward-backward check
    const float* back_v;
    int w, h;
    size_t pitch;  // floats
    float alpha1, alpha2, beta1, beta2;
    int check_boundaries;
};

// The reason of flow2d_track_points_2d for one slot; (qx, qy) is the new position when the reason is 0
__device__ __forceinline__ unsigned track_one(const TrackArgs& a, float px, float py, float& qx, float& qy)
{
    const float x_max = static_cast<float>(a.w - 1), y_max = static_cast<float>(a.h - 1);
    if (!inside(px, py, x_max, y_max)) return 3;
    const Bilinear s = bilinear(px, py, a.w, a.h, a.pitch);
    const float u0 = sample(a.flow_u, s), v0 = sample(a.flow_v, s);
    const float m0 = u0 * u0 + v0 * v0;
    if (a.check_boundaries) {
        const int ix = static_cast<int>(floorf(px + 0.5f)), iy = static_cast<int>(floorf(py + 0.5f));
        const int xl = max(ix - 1, 0), xr = min(ix + 1, a.w - 1), yu = max(iy - 1, 0), yd = min(iy + 1, a.h - 1);
        const float ux = 0.5f * (at(a.flow_u, a.pitch, xr, iy) - at(a.flow_u, a.pitch, xl, iy));
        const float uy = 0.5f * (at(a.flow_u, a.pitch, ix, yd) - at(a.flow_u, a.pitch, ix, yu));
        const float vx = 0.5f * (at(a.flow_v, a.pitch, xr, iy) - at(a.flow_v, a.pitch, xl, iy));
        const float vy = 0.5f * (at(a.flow_v, a.pitch, ix, yd) - at(a.flow_v, a.pitch, ix, yu));
        const float g = (ux * ux + uy * uy) + (vx * vx + vy * vy);
        if (!(g <= a.beta1 * m0 + a.beta2)) return 2;  // a NaN lands here
    }
    qx = px + u0;
    qy = py + v0;
    if (!isfinite(qx) || !isfinite(qy)) return 4;
    if (!inside(qx, qy, x_max, y_max)) return 3;
    if (a.back_u) {
        const Bilinear t = bilinear(qx, qy, a.w, a.h, a.pitch);
        const float bu = sample(a.back_u, t), bv = sample(a.back_v, t);
        const float eu = u0 + bu, ev = v0 + bv;
        if (!(eu * eu + ev * ev <= a.alpha1 * (m0 + (bu * bu + bv * bv)) + a.alpha2)) return 4;
    }
    return 0;
}

__global__ __launch_bounds__(kThreads) void track_kernel(TrackArgs a, const float* __restrict__ xs, const float* __restrict__ ys,
                                                         const unsigned long long* __restrict__ count, size_t capacity,
                                                         float* __restrict__ out_x, float* __restrict__ out_y,
                                                         unsigned char* __restrict__ reason)
{
    const unsigned long long n = *count;
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < capacity; i += stride) {
        unsigned r = 1;
        float qx = kNaN, qy = kNaN;
        if (i < n) {
            const float px = xs[i], py = ys[i];
            if (isfinite(px) && isfinite(py)) r = track_one(a, px, py, qx, qy);
        }
        out_x[i] = r == 0 ? qx : kNaN;
        out_y[i] = r == 0 ? qy : kNaN;
        if (reason) reason[i] = static_cast<unsigned char>(r);
    }
}

__global__ __launch_bounds__(kThreads) void seed_clear_kernel(uint4* __restrict__ flags, size_t chunks)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < chunks; i += stride)
        flags[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Every slot below *count with a finite position inside the frame flags its cell (racing lanes all write 1)
__global__ __launch_bounds__(kThreads) void seed_mark_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                             const unsigned long long* __restrict__ count, size_t capacity,
                                                             int w, int h, int spacing, size_t cells_x,
                                                             unsigned char* __restrict__ flags)
{
    const unsigned long long c = *count;
    const size_t n = c < capacity ? static_cast<size_t>(c) : capacity;
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (size_t k = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; k < n; k += stride) {
        const float x = xs[k], y = ys[k];
        if (!isfinite(x) || !isfinite(y) || !inside(x, y, x_max, y_max)) continue;
        const size_t cx = static_cast<size_t>(static_cast<int>(floorf(x)) / spacing);
        const size_t cy = static_cast<size_t>(static_cast<int>(floorf(y)) / spacing);
        flags[cy * cells_x + cx] = 1;
    }
}

__device__ __forceinline__ float gradient_x(const float* __restrict__ f, size_t pitch, int w, int x, int y)
{
    return 0.5f * (at(f, pitch, min(x + 1, w - 1), y) - at(f, pitch, max(x - 1, 0), y));
}

__device__ __forceinline__ float gradient_y(const float* __restrict__ f, size_t pitch, int h, int x, int y)
{
    return 0.5f * (at(f, pitch, x, min(y + 1, h - 1)) - at(f, pitch, x, max(y - 1, 0)));
}

// lambda_min of the 5x5 structure tensor at (x, y): gradients with clamped neighbours, window with edge-replicated
// coordinates, sums in row-major order
__device__ __forceinline__ float min_eigenvalue_at(const float* __restrict__ f, size_t pitch, int w, int h, int x, int y)
{
    float a = 0.f, b = 0.f, c = 0.f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = min(max(y + dy, 0), h - 1);
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = min(max(x + dx, 0), w - 1);
            const float gx = gradient_x(f, pitch, w, xx, yy), gy = gradient_y(f, pitch, h, xx, yy);
            a = a + gx * gx;
            b = b + gx * gy;
            c = c + gy * gy;
        }
    }
    return 0.5f * (a + c) - sqrtf(0.25f * (a - c) * (a - c) + b * b);
}

__device__ __forceinline__ void seed_pixel(size_t cell, size_t cells_x, int spacing, int w, int h, int& sx, int& sy)
{
    const size_t i = cell % cells_x, j = cell / cells_x;
    const size_t s = static_cast<size_t>(spacing), half = static_cast<size_t>(spacing / 2);
    sx = static_cast<int>(min_size(i * s + half, static_cast<size_t>(w - 1)));
    sy = static_cast<int>(min_size(j * s + half, static_cast<size_t>(h - 1)));
}

// Rank of this lane's flag among the flags of its workgroup below it, and the workgroup's total (wave ballots, then the
// four waves in order)
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned& total)
{
    __shared__ unsigned wave_counts[kThreads / 64];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(flag);
    const unsigned below = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_counts[wave] = __popcll(ballot);
    __syncthreads();
    unsigned before = 0;
    total = 0;
    for (unsigned k = 0; k < kThreads / 64; ++k) {
        before += k < wave ? wave_counts[k] : 0u;
        total += wave_counts[k];
    }
    return before + below;
}

// Per cell: a seed when uncovered and textured (the decision replaces the coverage flag); per workgroup: the seeds' count
__global__ __launch_bounds__(kThreads) void seed_decide_kernel(const float* __restrict__ frame, size_t pitch, int w, int h,
                                                               int spacing, size_t cells_x, size_t cells, float min_eigenvalue,
                                                               unsigned char* __restrict__ flags, unsigned* __restrict__ counts)
{
    const size_t cell = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
    bool seed = false;
    if (cell < cells) {
        seed = flags[cell] == 0;
        if (seed && min_eigenvalue != 0.f) {
            int sx, sy;
            seed_pixel(cell, cells_x, spacing, w, h, sx, sy);
            seed = min_eigenvalue_at(frame, pitch, w, h, sx, sy) >= min_eigenvalue;
        }
        flags[cell] = seed ? 1 : 0;
    }
    unsigned total = 0;
    block_rank(seed, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// One workgroup: exclusive offsets of the per-block counts in block order, the header, the new count and the drops
__global__ __launch_bounds__(kScanThreads) void seed_scan_kernel(const unsigned* __restrict__ counts, size_t blocks,
                                                                 unsigned long long* __restrict__ offsets,
                                                                 SeedHeader* __restrict__ header,
                                                                 unsigned long long* __restrict__ count, size_t capacity,
                                                                 unsigned long long* __restrict__ dropped)
{
    __shared__ unsigned long long sums[kScanThreads];
    const size_t chunk = (blocks + kScanThreads - 1) / kScanThreads;
    const size_t begin = min_size(static_cast<size_t>(threadIdx.x) * chunk, blocks), end = min_size(begin + chunk, blocks);
    unsigned long long s = 0;
    for (size_t b = begin; b < end; ++b) s += counts[b];
    sums[threadIdx.x] = s;
    __syncthreads();
    // inclusive scan of the thread sums (Hillis-Steele; integers, so the order of the additions does not matter)
    for (unsigned d = 1; d < kScanThreads; d <<= 1) {
        const unsigned long long add = threadIdx.x >= d ? sums[threadIdx.x - d] : 0ull;
        __syncthreads();
        sums[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = sums[threadIdx.x] - s;
    for (size_t b = begin; b < end; ++b) {
        offsets[b] = run;
        run += counts[b];
    }
    if (threadIdx.x == 0) {  // one lane writes the header and the counters (plain vector stores)
        const unsigned long long total = sums[kScanThreads - 1];
        const unsigned long long old = *count;
        const unsigned long long avail = old < capacity ? static_cast<unsigned long long>(capacity) - old : 0ull;
        const unsigned long long written = total < avail ? total : avail;
        header->base = old;
        header->avail = avail;
        *count = old + written;
        if (dropped) *dropped = total - written;
    }
}

__global__ __launch_bounds__(kThreads) void seed_write_kernel(const unsigned char* __restrict__ flags, size_t cells,
                                                              size_t cells_x, int spacing, int w, int h,
                                                              const unsigned long long* __restrict__ offsets,
                                                              const SeedHeader* __restrict__ header, float* __restrict__ xs,
                                                              float* __restrict__ ys)
{
    const size_t cell = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
    const bool seed = cell < cells && flags[cell] != 0;
    unsigned total = 0;
    const unsigned long long rank = offsets[blockIdx.x] + block_rank(seed, total);
    if (!seed || rank >= header->avail) return;
    int sx, sy;
    seed_pixel(cell, cells_x, spacing, w, h, sx, sy);
    const size_t slot = static_cast<size_t>(header->base + rank);
    xs[slot] = static_cast<float>(sx);
    ys[slot] = static_cast<float>(sy);
}

inline bool aligned(const void* p, size_t alignment) { return (reinterpret_cast<uintptr_t>(p) % alignment) == 0; }

inline bool finite_non_negative(float f) { return std::isfinite(f) && f >= 0.f; }

inline unsigned table_blocks(size_t n)
{
    const size_t b = (n + kThreads - 1) / kThreads;
    return static_cast<unsigned>(b < kMaxBlocks ? (b == 0 ? 1 : b) : kMaxBlocks);
}

}  // namespace

extern "C" {

int flow2d_track_points_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* back_u,
                           const float* back_v, size_t width, size_t height, size_t pitch_bytes, const float* x, const float* y,
                           const unsigned long long* count, size_t capacity, float alpha1, float alpha2, int check_boundaries,
                           float beta1, float beta2, float* out_x, float* out_y, unsigned char* reason)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no device comes first)
    if (!flow2d::plane_args_ok(flow_u, width, height, pitch_bytes) || !flow2d::plane_args_ok(flow_v, width, height, pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if ((back_u == nullptr) != (back_v == nullptr)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (back_u && (!flow2d::plane_args_ok(back_u, width, height, pitch_bytes) ||
                   !flow2d::plane_args_ok(back_v, width, height, pitch_bytes)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!x || !y || !count || !out_x || !out_y || capacity == 0 || !aligned(x, 4) || !aligned(y, 4) || !aligned(count, 8) ||
        !aligned(out_x, 4) || !aligned(out_y, 4))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!finite_non_negative(alpha1) || !finite_non_negative(alpha2) || !finite_non_negative(beta1) ||
        !finite_non_negative(beta2))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (capacity >= kMaxCapacity) return FLOW2D_ERR_UNSUPPORTED;
    // the kernel marks every pointer __restrict__: no written byte may meet a read one or another written one
    const size_t plane = height * pitch_bytes, table = capacity * sizeof(float);
    const flow2d::ByteRange read[] = {{flow_u, plane}, {flow_v, plane}, {back_u, plane}, {back_v, plane}, {x, table}, {y, table},
                                      {count, sizeof(unsigned long long)}};
    const flow2d::ByteRange written[] = {{out_x, table}, {out_y, table}, {reason, capacity}};
    if (flow2d::any_overlap(written, read)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (ctx->batch_count > 1) return FLOW2D_ERR_UNSUPPORTED;  // lock-step batches are not supported
    FLOW2D_ENTER(ctx);
    TrackArgs a;
    a.flow_u = flow_u;
    a.flow_v = flow_v;
    a.back_u = back_u;
    a.back_v = back_v;
    a.w = static_cast<int>(width);
    a.h = static_cast<int>(height);
    a.pitch = pitch_bytes / sizeof(float);
    a.alpha1 = alpha1;
    a.alpha2 = alpha2;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.check_boundaries = check_boundaries != 0;
    track_kernel<<<dim3(table_blocks(capacity)), dim3(kThreads), 0, ctx->stream>>>(a, x, y, count, capacity, out_x, out_y,
                                                                                   reason);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

size_t flow2d_seed_points_workspace_bytes(size_t width, size_t height, size_t spacing)
{
    if (width == 0 || height == 0 || spacing == 0) return 0;
    return seed_layout(width, height, spacing).total;
}

int flow2d_seed_points_2d(flow2d_context* ctx, const float* frame, size_t width, size_t height, size_t pitch_bytes,
                          size_t spacing, float min_eigenvalue, float* x, float* y, unsigned long long* count, size_t capacity,
                          unsigned long long* dropped, void* workspace, size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no device comes first)
    if (!flow2d::plane_args_ok(frame, width, height, pitch_bytes) || spacing == 0 || !finite_non_negative(min_eigenvalue))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!x || !y || !count || capacity == 0 || !aligned(x, 4) || !aligned(y, 4) || !aligned(count, 8) ||
        (dropped && !aligned(dropped, 8)) || !workspace || !aligned(workspace, 16))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < flow2d_seed_points_workspace_bytes(width, height, spacing)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const size_t plane = height * pitch_bytes, table = capacity * sizeof(float);
    // the frame is read, everything else is written: no two of the six ranges may meet
    const flow2d::ByteRange read[] = {{frame, plane}};
    const flow2d::ByteRange written[] = {{x, table}, {y, table}, {count, sizeof(unsigned long long)},
                                         {dropped, sizeof(unsigned long long)}, {workspace, workspace_bytes}};
    // (a larger capacity is refused below; its byte size may not even be representable)
    if (capacity < kMaxCapacity && flow2d::any_overlap(written, read)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const SeedLayout l = seed_layout(width, height, spacing);
    if (capacity >= kMaxCapacity || l.cells >= kMaxCells || spacing >= (size_t(1) << 30)) return FLOW2D_ERR_UNSUPPORTED;
    if (ctx->batch_count > 1) return FLOW2D_ERR_UNSUPPORTED;  // lock-step batches are not supported
    FLOW2D_ENTER(ctx);
    char* ws = static_cast<char*>(workspace);
    SeedHeader* header = reinterpret_cast<SeedHeader*>(ws);
    unsigned long long* offsets = reinterpret_cast<unsigned long long*>(ws + l.offsets);
    unsigned* counts = reinterpret_cast<unsigned*>(ws + l.counts);
    unsigned char* flags = reinterpret_cast<unsigned char*>(ws + l.flags);
    const int w = static_cast<int>(width), h = static_cast<int>(height), s = static_cast<int>(spacing);
    const size_t pitch = pitch_bytes / sizeof(float);
    const dim3 block(kThreads);
    seed_clear_kernel<<<dim3(table_blocks(l.flags_bytes / 16)), block, 0, ctx->stream>>>(reinterpret_cast<uint4*>(flags),
                                                                                         l.flags_bytes / 16);
    FLOW2D_CHECK_LAUNCH();
    seed_mark_kernel<<<dim3(table_blocks(capacity)), block, 0, ctx->stream>>>(x, y, count, capacity, w, h, s, l.cells_x, flags);
    FLOW2D_CHECK_LAUNCH();
    seed_decide_kernel<<<dim3(static_cast<unsigned>(l.blocks)), block, 0, ctx->stream>>>(frame, pitch, w, h, s, l.cells_x, l.cells,
                                                                                       min_eigenvalue, flags, counts);
    FLOW2D_CHECK_LAUNCH();
    seed_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, ctx->stream>>>(counts, l.blocks, offsets, header, count, capacity,
                                                                      dropped);
    FLOW2D_CHECK_LAUNCH();
    seed_write_kernel<<<dim3(static_cast<unsigned>(l.blocks)), block, 0, ctx->stream>>>(flags, l.cells, l.cells_x, s, w, h,
                                                                                      offsets, header, x, y);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
