// Motion segmentation for gfx950: no reference counterpart.
//
// flow2d_segment_motion_2d: the connected components of the foreground of a residual flow, numbered in raster order of their
// smallest linear index, with one record per region and a summary.  The normative definition is that of the entry in
// flow2d_c_abi.h; every output is an integer, and the only arithmetic on the planes is fp32 built -ffp-contract=off.
//
// Union-find with equivalence by smallest index, in seven launches whatever the planes hold:
//   (a) tile_label     one workgroup per 64 x 16 tile labels it in LDS: parent[p] = linear index of the tile-local root (the
//                      smallest index of the tile-local component), -1 for background; area[root] = its pixel count, 0 elsewhere
//   (b) border_union   one thread per pixel pair across a tile edge unites the two tile roots with atomicMin on `parent`
//   (c) flatten        one thread per tile root (area > 0): parent[root] = the final root, area[final root] += area[root]
//   (d) band_count     one workgroup per band of 2048 consecutive linear indices -- block order is raster order -- counts the final
//                      roots with area >= min_area, the foreground pixels and the dropped ones into one slab, and replaces
//                      parent[final root] by -2 - (its rank within the band), or by -1 where the region is dropped
//   (e) band_scan      one workgroup per instance: the first label of every band (slabs scanned in block order), the summary
//   (f) region_init    one thread per kept root writes its whole record -- area, first, y0 are known there, x0 / x1 / y1 start at
//                      the root's own pixel, the sums at 0 --, and the records nobody owns are zeroed
//   (g) label          one workgroup per tile: labels[p] through at most three reads of `parent`, the sums and the box gathered per
//                      tile-local component in LDS, then one set of global atomics per component and tile
// Only non-root pixels of a tile never change: parent[p] of such a pixel is its tile root from (a) to (g).
//
// Integer atomics only (min, max, add on 32- and 64-bit integers): they commute and associate, so no byte depends on the order
// of arrival.  No workgroup waits for another: every data-dependent loop follows `parent` links, and a link always points to a
// strictly smaller index.  Between launches visibility is the kernel boundary's; inside (b) and (c), where other workgroups
// write the words a chase reads, every access to them is an agent-scope atomic (a plain load may be served stale from the XCD's
// own L2; a stale parent is still an ancestor, and the atomicMin retry form below stays correct with it).
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"
#include "ordered_reduce.hpp"

namespace {

constexpr int kTileW = 64;   // a wave covers one row of a tile
constexpr int kTileH = 16;
constexpr int kTileWaves = 4;
constexpr int kTileRows = kTileH / kTileWaves;  // rows per thread
constexpr int kTilePixels = kTileW * kTileH;
constexpr int kBandThreads = 256;
constexpr int kBandPerThread = 8;  // consecutive indices per thread: the ranks of a band are in raster order
constexpr int kBand = kBandThreads * kBandPerThread;
constexpr int kLinearThreads = 256;

struct Band {
    unsigned kept;  // final roots of the band with area >= min_area
    unsigned base;  // kept roots of all earlier bands (band_scan)
    unsigned long long foreground;
    unsigned long long dropped;
    unsigned long long reserved;
};
static_assert(sizeof(Band) == 32, "slabs stay 16-byte aligned");

// One instance's slice of the workspace: parent (int per pixel, unpitched), area (unsigned per pixel), the band slabs.
struct Geometry {
    int w, h, pitch;  // pitch in floats
    int tiles_x;
    unsigned tiles, bands;
    unsigned long long n;
    unsigned long long plane_bytes, slice_bytes;
};

inline Geometry geometry(size_t width, size_t height, size_t pitch_bytes)
{
    Geometry g;
    g.w = static_cast<int>(width);
    g.h = static_cast<int>(height);
    g.pitch = static_cast<int>(pitch_bytes / 4);
    g.tiles_x = static_cast<int>(flow2d::div_up(width, kTileW));
    g.tiles = static_cast<unsigned>(g.tiles_x) * flow2d::div_up(height, kTileH);
    g.n = static_cast<unsigned long long>(width) * height;
    g.bands = static_cast<unsigned>((g.n + kBand - 1) / kBand);
    g.plane_bytes = (g.n * 4 + 15) / 16 * 16;
    g.slice_bytes = 2 * g.plane_bytes + static_cast<unsigned long long>(g.bands) * sizeof(Band);
    return g;
}

__device__ __forceinline__ int* slice_parent(char* ws, const Geometry& g) { return reinterpret_cast<int*>(ws + blockIdx.z * g.slice_bytes); }
__device__ __forceinline__ unsigned* slice_area(char* ws, const Geometry& g)
{
    return reinterpret_cast<unsigned*>(ws + blockIdx.z * g.slice_bytes + g.plane_bytes);
}
__device__ __forceinline__ Band* slice_bands(char* ws, const Geometry& g)
{
    return reinterpret_cast<Band*>(ws + blockIdx.z * g.slice_bytes + 2 * g.plane_bytes);
}

__device__ __forceinline__ float clamp_mask(float m)
{
    if (!(m <= 1.f)) m = 1.f;  // NaN: left out
    if (!(m >= 0.f)) m = 0.f;
    return m;
}

__device__ __forceinline__ bool joined(float ua, float va, float ub, float vb, float join2)
{
    const float du = ua - ub, dv = va - vb;
    return du * du + dv * dv <= join2;  // a NaN difference (inf - inf) is no edge
}

// ---- union-find on one address space (LDS within a tile, the workspace across tiles) -----------------------------------------
template <int Scope>
__device__ __forceinline__ int find_root(int* parent, int i)
{
    // Invariant: a link always points to a strictly smaller index, so the chase from i ends within i steps whatever other
    // threads do meanwhile.  (Anything else -- an equal, larger or negative word -- ends it at once: i is then the root.)
    for (;;) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, Scope);
        if (p >= i || p < 0) return i;
        i = p;
    }
}

template <int Scope>
__device__ __forceinline__ void unite(int* parent, int a, int b)
{
    a = find_root<Scope>(parent, a);
    b = find_root<Scope>(parent, b);
    // Every turn either links the larger root under the smaller one and ends, or learns that `a` had stopped being a root and
    // goes on with what it pointed to: `old` < a, so (a, b) decreases and the loop ends.  A stale `a` costs a turn, no more.
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, Scope);
        if (old == a) break;
        a = find_root<Scope>(parent, old);
        b = find_root<Scope>(parent, b);
    }
}

constexpr int kWorkgroup = __HIP_MEMORY_SCOPE_WORKGROUP;
constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT;

__device__ __forceinline__ int wave_min(int x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ int wave_max_int(int x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    return x;
}

// Whether every active lane of the wave holds the same key; `leader` is then the one lane that speaks for them.
__device__ __forceinline__ bool wave_uniform(bool active, int key, unsigned long long& lanes, bool& leader)
{
    lanes = __ballot(active);
    if (lanes == 0) {
        leader = false;
        return true;
    }
    const int first = __ffsll(static_cast<long long>(lanes)) - 1;
    const int key0 = __shfl(key, first, 64);
    leader = static_cast<int>(threadIdx.x) == first;
    return __ballot(active && key != key0) == 0;
}

// (a) ------------------------------------------------------------------------------------------------------------------------------
template <bool HasMask>
__global__ __launch_bounds__(256) void tile_label_kernel(const float* __restrict__ ru, const float* __restrict__ rv,
                                                         const float* __restrict__ mask, Geometry g, float threshold2,
                                                         float join2, char* __restrict__ ws, BatchArg batch)
{
    const size_t inst = static_cast<size_t>(blockIdx.z) * static_cast<size_t>(batch.stride);
    int* parent = slice_parent(ws, g);
    unsigned* area = slice_area(ws, g);
    const int tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const int lx = threadIdx.x, gx = tx * kTileW + lx;
    __shared__ int lp[kTilePixels];
    __shared__ float lu[kTilePixels], lv[kTilePixels];
    __shared__ unsigned count[kTilePixels];
    __shared__ unsigned char lf[kTilePixels];
    bool fg[kTileRows];
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int ly = threadIdx.y + kTileWaves * i, l = ly * kTileW + lx, gy = ty * kTileH + ly;
        float u = 0.f, v = 0.f;
        fg[i] = false;
        if (gx < g.w && gy < g.h) {
            const size_t at = inst + static_cast<size_t>(gy) * g.pitch + gx;
            u = ru[at];
            v = rv[at];
            const float m = HasMask ? clamp_mask(mask[at]) : 0.f;
            fg[i] = (u * u + v * v > threshold2) && (m < 0.5f);
        }
        lu[l] = u;
        lv[l] = v;
        lf[l] = fg[i];
        lp[l] = fg[i] ? l : -1;
        count[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int ly = threadIdx.y + kTileWaves * i, l = ly * kTileW + lx;
        if (!fg[i]) continue;
        if (lx > 0 && lf[l - 1] && joined(lu[l], lv[l], lu[l - 1], lv[l - 1], join2)) unite<kWorkgroup>(lp, l, l - 1);
        if (ly > 0 && lf[l - kTileW] && joined(lu[l], lv[l], lu[l - kTileW], lv[l - kTileW], join2))
            unite<kWorkgroup>(lp, l, l - kTileW);
    }
    __syncthreads();
    int root[kTileRows];
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int l = (threadIdx.y + kTileWaves * i) * kTileW + lx;
        root[i] = fg[i] ? find_root<kWorkgroup>(lp, l) : -1;
        // the pixels of a row that share a root are counted with one LDS atomic where the whole wave agrees
        unsigned long long lanes;
        bool leader;
        if (wave_uniform(fg[i], root[i], lanes, leader)) {
            if (leader) atomicAdd(&count[root[i]], static_cast<unsigned>(__popcll(lanes)));
        } else if (fg[i]) {
            atomicAdd(&count[root[i]], 1u);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int ly = threadIdx.y + kTileWaves * i, l = ly * kTileW + lx, gy = ty * kTileH + ly;
        if (gx >= g.w || gy >= g.h) continue;
        const int at = gy * g.w + gx;  // below 2^31: the entry refuses larger planes
        int p = -1;
        if (fg[i]) p = (ty * kTileH + root[i] / kTileW) * g.w + tx * kTileW + root[i] % kTileW;
        parent[at] = p;
        area[at] = (fg[i] && root[i] == l) ? count[l] : 0u;
    }
}

// (b) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLinearThreads) void border_union_kernel(const float* __restrict__ ru, const float* __restrict__ rv,
                                                                      Geometry g, float join2, unsigned long long vertical,
                                                                      unsigned long long horizontal, char* ws, BatchArg batch)
{
    const size_t inst = static_cast<size_t>(blockIdx.z) * static_cast<size_t>(batch.stride);
    int* parent = slice_parent(ws, g);
    unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * kLinearThreads + threadIdx.x;
    int xp, yp, xq, yq;
    if (t < vertical) {  // the pair left and right of a tile edge
        xq = (static_cast<int>(t / g.h) + 1) * kTileW;
        yq = static_cast<int>(t % g.h);
        xp = xq - 1;
        yp = yq;
    } else {
        t -= vertical;
        if (t >= horizontal) return;
        yq = (static_cast<int>(t / g.w) + 1) * kTileH;
        xq = static_cast<int>(t % g.w);
        xp = xq;
        yp = yq - 1;
    }
    const int p = yp * g.w + xp, q = yq * g.w + xq;
    // (foreground: the sign of `parent`, which no union changes)
    if (__hip_atomic_load(parent + p, __ATOMIC_RELAXED, kAgent) < 0 || __hip_atomic_load(parent + q, __ATOMIC_RELAXED, kAgent) < 0)
        return;
    const size_t ap = inst + static_cast<size_t>(yp) * g.pitch + xp, aq = inst + static_cast<size_t>(yq) * g.pitch + xq;
    if (!joined(ru[ap], rv[ap], ru[aq], rv[aq], join2)) return;
    unite<kAgent>(parent, p, q);
}

// (c) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLinearThreads) void flatten_kernel(Geometry g, char* ws)
{
    int* parent = slice_parent(ws, g);
    unsigned* area = slice_area(ws, g);
    const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * kLinearThreads + threadIdx.x;
    if (t >= g.n) return;
    const int i = static_cast<int>(t);
    // a tile root, and only a tile root, has an area.  Other threads add to the area of a FINAL root meanwhile: it stays > 0,
    // and the value read is used only where i is no final root, which nobody adds to.
    const unsigned mine = __hip_atomic_load(area + i, __ATOMIC_RELAXED, kAgent);
    if (mine == 0) return;
    const int r = find_root<kAgent>(parent, i);
    if (r == i) return;
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, kAgent);  // (still an ancestor for whoever chases through i)
    atomicAdd(area + r, mine);
}

// Exclusive prefix sum of one value per thread over a workgroup of 256 threads (in thread order); `total` for every thread.
template <typename T>
__device__ __forceinline__ T workgroup_exclusive_scan(T mine, T& total)
{
    __shared__ T wave_totals[kBandThreads / 64];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    T inclusive = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(inclusive, o, 64);
        if (lane >= o) inclusive += up;
    }
    if (lane == 63) wave_totals[wave] = inclusive;
    __syncthreads();
    T before = 0;
    total = 0;
    for (int wv = 0; wv < kBandThreads / 64; ++wv) {
        if (wv < wave) before += wave_totals[wv];
        total += wave_totals[wv];
    }
    return before + inclusive - mine;
}

// (d) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBandThreads) void band_count_kernel(Geometry g, unsigned min_area, char* ws)
{
    int* parent = slice_parent(ws, g);
    const unsigned* area = slice_area(ws, g);
    const unsigned long long first = static_cast<unsigned long long>(blockIdx.x) * kBand + threadIdx.x * kBandPerThread;
    unsigned keep = 0, drop = 0, kept = 0;
    unsigned long long foreground = 0, dropped = 0;
#pragma unroll
    for (int j = 0; j < kBandPerThread; ++j) {
        const unsigned long long i = first + j;
        if (i >= g.n) break;
        const int p = parent[i];
        if (p < 0) continue;
        ++foreground;
        if (p != static_cast<int>(i)) continue;
        const unsigned a = area[i];
        if (a >= min_area) {
            keep |= 1u << j;
            ++kept;
        } else {
            drop |= 1u << j;
            dropped += a;
        }
    }
    unsigned total;
    unsigned rank = workgroup_exclusive_scan(kept, total);
#pragma unroll
    for (int j = 0; j < kBandPerThread; ++j) {
        if (keep >> j & 1u) parent[first + j] = -2 - static_cast<int>(rank++);
        if (drop >> j & 1u) parent[first + j] = -1;
    }
    foreground = wave_sum(foreground);
    dropped = wave_sum(dropped);
    __shared__ unsigned long long sums[kBandThreads / 64][2];
    if (threadIdx.x % 64 == 0) {
        sums[threadIdx.x / 64][0] = foreground;
        sums[threadIdx.x / 64][1] = dropped;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    Band out = {total, 0u, 0ull, 0ull, 0ull};
    for (int wv = 0; wv < kBandThreads / 64; ++wv) {
        out.foreground += sums[wv][0];
        out.dropped += sums[wv][1];
    }
    slice_bands(ws, g)[blockIdx.x] = out;
}

// (e) one workgroup per instance (blockIdx.z): thread t owns a run of consecutive bands ---------------------------------------------
__global__ __launch_bounds__(kBandThreads) void band_scan_kernel(Geometry g, unsigned long long max_regions, char* ws,
                                                                 flow2d_segment_summary* __restrict__ summary)
{
    Band* bands = slice_bands(ws, g);
    const unsigned run = (g.bands + kBandThreads - 1) / kBandThreads;
    const unsigned long long begin = static_cast<unsigned long long>(threadIdx.x) * run;
    const unsigned long long end = min(begin + run, static_cast<unsigned long long>(g.bands));
    unsigned kept = 0;  // (all kept roots together stay below 2^31)
    unsigned long long foreground = 0, dropped = 0;
    for (unsigned long long j = begin; j < end; ++j) {
        kept += bands[j].kept;
        foreground += bands[j].foreground;
        dropped += bands[j].dropped;
    }
    unsigned total;
    unsigned base = workgroup_exclusive_scan(kept, total);
    for (unsigned long long j = begin; j < end; ++j) {
        bands[j].base = base;
        base += bands[j].kept;
    }
    foreground = wave_sum(foreground);
    dropped = wave_sum(dropped);
    __shared__ unsigned long long sums[kBandThreads / 64][2];
    if (threadIdx.x % 64 == 0) {
        sums[threadIdx.x / 64][0] = foreground;
        sums[threadIdx.x / 64][1] = dropped;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    flow2d_segment_summary out = {total, 0ull, 0ull, 0u, 0u};
    for (int wv = 0; wv < kBandThreads / 64; ++wv) {
        out.foreground += sums[wv][0];
        out.dropped += sums[wv][1];
    }
    out.recorded = static_cast<unsigned>(min(static_cast<unsigned long long>(total), max_regions));
    summary[blockIdx.z] = out;
}

// The label behind a word of `parent` that codes a kept root of the band of index `at`.
__device__ __forceinline__ unsigned coded_label(const Band* __restrict__ bands, unsigned long long at, int code)
{
    return bands[at / kBand].base + static_cast<unsigned>(-2 - code) + 1u;
}

// (f) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBandThreads) void region_init_kernel(Geometry g, unsigned long long max_regions, char* ws,
                                                                   const flow2d_segment_summary* __restrict__ summary,
                                                                   flow2d_motion_region* __restrict__ regions)
{
    const int* parent = slice_parent(ws, g);
    const unsigned* area = slice_area(ws, g);
    const Band* bands = slice_bands(ws, g);
    regions += blockIdx.z * max_regions;
    const unsigned long long first = static_cast<unsigned long long>(blockIdx.x) * kBand + threadIdx.x * kBandPerThread;
#pragma unroll
    for (int j = 0; j < kBandPerThread; ++j) {
        const unsigned long long i = first + j;
        if (i >= g.n) break;
        const int p = parent[i];
        if (p > -2) continue;
        const unsigned label = coded_label(bands, i, p);
        if (label > max_regions) continue;
        const int x = static_cast<int>(i % g.w), y = static_cast<int>(i / g.w);
        regions[label - 1] = flow2d_motion_region{area[i], 0ull, 0ull, 0ll, 0ll, x, y, x, y, i};
    }
    // the records no region owns
    const unsigned long long recorded = summary[blockIdx.z].recorded;
    uint4* words = reinterpret_cast<uint4*>(regions + recorded);
    const unsigned long long count = (max_regions - recorded) * (sizeof(flow2d_motion_region) / sizeof(uint4));
    for (unsigned long long k = static_cast<unsigned long long>(blockIdx.x) * kBandThreads + threadIdx.x; k < count;
         k += static_cast<unsigned long long>(gridDim.x) * kBandThreads)
        words[k] = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ long long q16(float r)
{
    return __double2ll_rn(static_cast<double>(fminf(fmaxf(r, -32768.f), 32768.f)) * 65536.0);
}

// (g) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void label_kernel(const float* __restrict__ ru, const float* __restrict__ rv, Geometry g,
                                                    unsigned long long max_regions, const char* __restrict__ ws_in,
                                                    int* __restrict__ labels, flow2d_motion_region* __restrict__ regions,
                                                    BatchArg batch)
{
    const size_t inst = static_cast<size_t>(blockIdx.z) * static_cast<size_t>(batch.stride);
    char* ws = const_cast<char*>(ws_in);
    const int* parent = slice_parent(ws, g);
    const Band* bands = slice_bands(ws, g);
    regions += blockIdx.z * max_regions;
    const int tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const int lx = threadIdx.x, gx = tx * kTileW + lx;
    // one slot per pixel of the tile; a tile-local component gathers in the slot of one of its pixels, in tile coordinates
    __shared__ unsigned s_count[kTilePixels], s_x[kTilePixels], s_y[kTilePixels];
    __shared__ int s_x0[kTilePixels], s_x1[kTilePixels], s_y1[kTilePixels];
    __shared__ unsigned long long s_u[kTilePixels], s_v[kTilePixels];
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int l = (threadIdx.y + kTileWaves * i) * kTileW + lx;
        s_count[l] = s_x[l] = s_y[l] = 0u;
        s_x0[l] = INT_MAX;
        s_x1[l] = s_y1[l] = -1;
        s_u[l] = s_v[l] = 0ull;
    }
    __syncthreads();
    unsigned label[kTileRows];
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int ly = threadIdx.y + kTileWaves * i, l = ly * kTileW + lx, gy = ty * kTileH + ly;
        const bool inside = gx < g.w && gy < g.h;
        label[i] = 0u;
        int slot = l;
        size_t at = 0;
        if (inside) {
            at = inst + static_cast<size_t>(gy) * g.pitch + gx;
            const int me = gy * g.w + gx;
            const int a = parent[me];
            if (a <= -2) {
                label[i] = coded_label(bands, me, a);
            } else if (a >= 0) {
                // a: this pixel's tile root, or -- for a tile root that is no final root -- the final root, in any tile
                const int ax = a % g.w - tx * kTileW, ay = a / g.w - ty * kTileH;
                if (ax >= 0 && ax < kTileW && ay >= 0 && ay < kTileH) slot = ay * kTileW + ax;
                const int b = parent[a];
                if (b <= -2) {
                    label[i] = coded_label(bands, a, b);
                } else if (b >= 0) {
                    const int c = parent[b];
                    if (c <= -2) label[i] = coded_label(bands, b, c);
                }
            }
            labels[at] = static_cast<int>(label[i]);
        }
        const bool active = label[i] != 0u && label[i] <= max_regions;
        long long qu = 0, qv = 0;
        if (active) {
            qu = q16(ru[at]);
            qv = q16(rv[at]);
        }
        unsigned long long lanes;
        bool leader;
        if (wave_uniform(active, slot, lanes, leader)) {
            if (lanes == 0) continue;
            // one row, one slot: through the lanes first, then one set of LDS atomics
            const unsigned n = static_cast<unsigned>(__popcll(lanes));
            const unsigned sx = wave_sum(active ? static_cast<unsigned>(lx) : 0u);
            const unsigned long long su = wave_sum(static_cast<unsigned long long>(qu));
            const unsigned long long sv = wave_sum(static_cast<unsigned long long>(qv));
            const int x0 = wave_min(active ? lx : INT_MAX), x1 = wave_max_int(active ? lx : -1);
            if (leader) {
                atomicAdd(&s_count[slot], n);
                atomicAdd(&s_x[slot], sx);
                atomicAdd(&s_y[slot], n * static_cast<unsigned>(ly));
                atomicAdd(&s_u[slot], su);
                atomicAdd(&s_v[slot], sv);
                atomicMin(&s_x0[slot], x0);
                atomicMax(&s_x1[slot], x1);
                atomicMax(&s_y1[slot], ly);
            }
        } else if (active) {
            atomicAdd(&s_count[slot], 1u);
            atomicAdd(&s_x[slot], static_cast<unsigned>(lx));
            atomicAdd(&s_y[slot], static_cast<unsigned>(ly));
            atomicAdd(&s_u[slot], static_cast<unsigned long long>(qu));
            atomicAdd(&s_v[slot], static_cast<unsigned long long>(qv));
            atomicMin(&s_x0[slot], lx);
            atomicMax(&s_x1[slot], lx);
            atomicMax(&s_y1[slot], ly);
        }
    }
    __syncthreads();
    // the pixel a slot belongs to carries the label of everything gathered there: one set of global atomics per slot in use.
    // (area, first and y0 were written by region_init; x0 / x1 / y1 start at the root's own pixel.)
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int l = (threadIdx.y + kTileWaves * i) * kTileW + lx;
        const unsigned n = s_count[l];
        if (n == 0 || label[i] == 0u || label[i] > max_regions) continue;
        flow2d_motion_region* rec = regions + (label[i] - 1u);
        const unsigned long long ox = static_cast<unsigned long long>(tx) * kTileW, oy = static_cast<unsigned long long>(ty) * kTileH;
        atomicAdd(&rec->sum_x, s_x[l] + n * ox);
        atomicAdd(&rec->sum_y, s_y[l] + n * oy);
        atomicAdd(reinterpret_cast<unsigned long long*>(&rec->sum_u_q16), s_u[l]);
        atomicAdd(reinterpret_cast<unsigned long long*>(&rec->sum_v_q16), s_v[l]);
        atomicMin(&rec->x0, static_cast<int>(ox) + s_x0[l]);
        atomicMax(&rec->x1, static_cast<int>(ox) + s_x1[l]);
        atomicMax(&rec->y1, static_cast<int>(oy) + s_y1[l]);
    }
}

}  // namespace

extern "C" {

size_t flow2d_segment_motion_workspace_bytes(size_t width, size_t height, size_t instances)
{
    if (width == 0 || height == 0 || instances == 0) return 0;
    return static_cast<size_t>(geometry(width, height, 0).slice_bytes) * instances;
}

int flow2d_segment_motion_2d(flow2d_context* ctx, const float* residual_u, const float* residual_v, const float* mask, size_t width,
                             size_t height, size_t pitch_bytes, float threshold, float join, unsigned min_area, int* labels,
                             flow2d_motion_region* regions, size_t max_regions, flow2d_segment_summary* summary, void* workspace,
                             size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!flow2d::plane_args_ok(residual_u, width, height, pitch_bytes) || !flow2d::plane_args_ok(residual_v, width, height, pitch_bytes) ||
        (mask && !flow2d::plane_args_ok(mask, width, height, pitch_bytes)) || !flow2d::plane_args_ok(labels, width, height, pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (static_cast<unsigned long long>(width) * height >= (1ull << 31)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(threshold >= 0.f) || !(join >= 0.f) || min_area == 0) return FLOW2D_ERR_INVALID_ARGUMENT;  // a NaN fails
    if ((regions == nullptr && max_regions > 0) || (reinterpret_cast<uintptr_t>(regions) % 8) != 0 || !summary ||
        (reinterpret_cast<uintptr_t>(summary) % 8) != 0 || !workspace || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0 ||
        workspace_bytes < flow2d_segment_motion_workspace_bytes(width, height, 1))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{labels, span},
                                             {regions, instances * max_regions * sizeof(flow2d_motion_region)},
                                             {summary, instances * sizeof(flow2d_segment_summary)},
                                             {workspace, workspace_bytes}};
        const flow2d::ByteRange read[] = {{residual_u, span}, {residual_v, span}, {mask, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (workspace_bytes < flow2d_segment_motion_workspace_bytes(width, height, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;

    const Geometry g = geometry(width, height, pitch_bytes);
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    const unsigned z = flow2d::batch_z(ctx, 1);
    char* ws = static_cast<char*>(workspace);
    const float threshold2 = threshold * threshold, join2 = join * join;
    const dim3 tile_grid(g.tiles, 1, z), tile_block(kTileW, kTileWaves);
    const dim3 band_grid(g.bands, 1, z);
    const unsigned long long vertical = static_cast<unsigned long long>(g.tiles_x - 1) * height;
    const unsigned long long horizontal = static_cast<unsigned long long>(flow2d::div_up(height, kTileH) - 1) * width;
    const unsigned border_blocks = static_cast<unsigned>(std::max<unsigned long long>((vertical + horizontal + kLinearThreads - 1) / kLinearThreads, 1));
    const unsigned long long max_r = max_regions;

    if (mask)
        tile_label_kernel<true><<<tile_grid, tile_block, 0, ctx->stream>>>(residual_u, residual_v, mask, g, threshold2, join2, ws, batch);
    else
        tile_label_kernel<false><<<tile_grid, tile_block, 0, ctx->stream>>>(residual_u, residual_v, mask, g, threshold2, join2, ws, batch);
    FLOW2D_CHECK_LAUNCH();
    border_union_kernel<<<dim3(border_blocks, 1, z), dim3(kLinearThreads), 0, ctx->stream>>>(residual_u, residual_v, g, join2, vertical,
                                                                                              horizontal, ws, batch);
    FLOW2D_CHECK_LAUNCH();
    flatten_kernel<<<dim3(static_cast<unsigned>((g.n + kLinearThreads - 1) / kLinearThreads), 1, z), dim3(kLinearThreads), 0,
                     ctx->stream>>>(g, ws);
    FLOW2D_CHECK_LAUNCH();
    band_count_kernel<<<band_grid, dim3(kBandThreads), 0, ctx->stream>>>(g, min_area, ws);
    FLOW2D_CHECK_LAUNCH();
    band_scan_kernel<<<dim3(1, 1, z), dim3(kBandThreads), 0, ctx->stream>>>(g, max_r, ws, summary);
    FLOW2D_CHECK_LAUNCH();
    region_init_kernel<<<band_grid, dim3(kBandThreads), 0, ctx->stream>>>(g, max_r, ws, summary, regions);
    FLOW2D_CHECK_LAUNCH();
    label_kernel<<<tile_grid, tile_block, 0, ctx->stream>>>(residual_u, residual_v, g, max_r, ws, labels, regions, batch);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"
