// The cubic B-spline coefficients of a plane for gfx950: both passes of the separable prefilter in one launch.
//
// The normative definition is the one of flow2d_bspline_prefilter_2d in flow2d_c_abi.h, in IEEE double.  Built -ffp-contract=off.
//
// The recursive filter of the textbooks is a scan; the header states its symmetric impulse response instead, truncated at 16, so
// an output depends on 33 x 33 inputs and a workgroup owns a tile.  A workgroup of four waves makes a 64 x 32 tile:
//   stage   the tile and a halo of 16 on every side, 96 x 64 floats, into LDS; the source index of a staged column or row is
//           reflect() of the header, worked out once per column and row (the general form: a plane may be narrower than the halo);
//   rows    the row pass for the tile's 32 rows and the 32 halo rows, 64 x 64 doubles into a second LDS array.  A lane owns a row
//           and sixteen consecutive outputs of it: the 48 inputs are read once and converted once, where a lane per column would
//           read 33 for every output.  The float array's pitch is odd (97) and the double array's too (65), so that 64 lanes one
//           row apart meet 64 different banks in both;
//   columns the column pass from there, a lane per column and eight consecutive rows (40 reads for 8 outputs), cast to float and
//           stored where the tile lies inside the plane.
// The doubles between the passes never touch memory and the entry allocates nothing.  58 752 bytes of static LDS, below the 64 KB
// a launch may ask for; two workgroups per CU.  No atomics: the bytes depend on nothing but the input.
#include <cmath>

#include "node_grid.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kHorizon = FLOW2D_BSPLINE_HORIZON;
constexpr int kTileX = 64, kTileY = 32;
constexpr int kStageW = kTileX + 2 * kHorizon, kStageH = kTileY + 2 * kHorizon;  // 96 x 64
constexpr int kStagePitch = kStageW + 1, kMidPitch = kTileX + 1;                  // both odd
constexpr int kThreads = 256;
constexpr int kRowRun = 16, kColumnRun = 8;  // consecutive outputs of a lane in the two passes
static_assert(kStageH == 64 && kTileX == 64, "a lane per staged row, then a lane per column");
static_assert((kTileX / kRowRun) * 64 == kThreads && (kTileY / kColumnRun) * 64 == kThreads, "every thread has a run in both passes");

struct PrefilterTaps {
    double z[kHorizon + 1];  // z[j] of the header
    double g;                // G
};

// reflect(i, n) of the header.
__device__ __forceinline__ int reflect_any(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m <= n - 1 ? m : p - m;
}

// d[centre] of the header from the line's values around it: s[centre - 16 .. centre + 16].
template <int N>
__device__ __forceinline__ double filter_at(const double (&s)[N], int centre, const PrefilterTaps& taps)
{
    double acc = 0.0;
#pragma unroll
    for (int j = kHorizon; j >= 1; --j) acc = acc + taps.z[j] * (s[centre - j] + s[centre + j]);
    acc = acc + s[centre];
    return taps.g * acc;
}

template <typename Offset>
__global__ __launch_bounds__(kThreads) void bspline_prefilter_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h,
                                                                     int pitch, PrefilterTaps taps, BatchArg batch)
{
    __shared__ float s_stage[kStageH * kStagePitch];
    __shared__ double s_mid[kStageH * kMidPitch];
    __shared__ int s_column[kStageW], s_row[kStageH];

    const size_t inst = batch_offset(batch);
    src += inst;
    dst += inst;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;

    if (tid < kStageW) s_column[tid] = reflect_any(x0 - kHorizon + tid, w);
    if (tid >= kThreads - kStageH) s_row[tid - (kThreads - kStageH)] = reflect_any(y0 - kHorizon + (tid - (kThreads - kStageH)), h);
    __syncthreads();
    for (int i = tid; i < kStageW * kStageH; i += kThreads) {
        const int sy = i / kStageW, sx = i - sy * kStageW;
        s_stage[sy * kStagePitch + sx] = load_at(src, pixel_offset<Offset>(s_column[sx], s_row[sy], pitch));
    }
    __syncthreads();

    {  // rows: staged row `lane`, outputs wave * 16 .. wave * 16 + 15 of the tile's columns
        double s[kRowRun + 2 * kHorizon];
        const float* row = s_stage + lane * kStagePitch + wave * kRowRun;
#pragma unroll
        for (int i = 0; i < kRowRun + 2 * kHorizon; ++i) s[i] = static_cast<double>(row[i]);
        double* out = s_mid + lane * kMidPitch + wave * kRowRun;
#pragma unroll
        for (int k = 0; k < kRowRun; ++k) out[k] = filter_at(s, kHorizon + k, taps);
    }
    __syncthreads();

    {  // columns: column `lane` of the tile, rows wave * 8 .. wave * 8 + 7
        double s[kColumnRun + 2 * kHorizon];
        const double* column = s_mid + (wave * kColumnRun) * kMidPitch + lane;
#pragma unroll
        for (int i = 0; i < kColumnRun + 2 * kHorizon; ++i) s[i] = column[i * kMidPitch];
        const int x = x0 + lane;
#pragma unroll
        for (int k = 0; k < kColumnRun; ++k) {
            const int y = y0 + wave * kColumnRun + k;
            const float value = static_cast<float>(filter_at(s, kHorizon + k, taps));
            if (x < w && y < h) store_at(dst, pixel_offset<Offset>(x, y, pitch), value);
        }
    }
}

}  // namespace

extern "C" int flow2d_bspline_prefilter_2d(flow2d_context* ctx, const float* src, float* dst, size_t width, size_t height,
                                           size_t pitch_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!flow2d::planes_ok({src, dst}, {}, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (flow2d::ranges_overlap(dst, height * pitch_bytes, src, height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t span = flow2d::batch_span(ctx, height * pitch_bytes);
    if (flow2d::ranges_overlap(dst, span, src, span)) return FLOW2D_ERR_INVALID_ARGUMENT;
    PrefilterTaps taps;
    const double root = std::sqrt(3.0), Z = root - 2.0;
    taps.z[0] = 1.0;
    for (int j = 1; j <= kHorizon; ++j) taps.z[j] = taps.z[j - 1] * Z;
    taps.g = root / 6.0;
    // (the largest offset a lane forms into a plane is below height * pitch_bytes)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        const dim3 grid(flow2d::div_up(width, kTileX), flow2d::div_up(height, kTileY), flow2d::batch_z(ctx, 1));
        bspline_prefilter_kernel<decltype(offset)><<<grid, kThreads, 0, ctx->stream>>>(
            src, dst, static_cast<int>(width), static_cast<int>(height), static_cast<int>(pitch_bytes / 4), taps, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}
