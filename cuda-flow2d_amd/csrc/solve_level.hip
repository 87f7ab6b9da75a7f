// The solver's fixed-point loop of one pyramid level and its launch timing.
// Replaces the launch loop of CudaOperationSolve2D::Execute
// (src/cuda_operations/2d/cuda_operation_solve_2d.cpp:229-300) without its per-sweep host
// synchronisation (:291): everything is queued on the context's stream.
#include <algorithm>
#include <cstdlib>

#include "solver.hpp"

namespace {
// mode-2 timing: one more event on the stream, appended to the slot's start/stop list
hipError_t take_event(flow2d_context* ctx, hipEvent_t* ev)
{
    if (!ctx->event_pool.empty()) {
        *ev = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return hipSuccess;
    }
    return hipEventCreate(ev);
}

hipError_t mark(flow2d_context* ctx, flow2d_timing_slot* slot)
{
    hipEvent_t ev;
    hipError_t e = take_event(ctx, &ev);
    if (e != hipSuccess) return e;
    slot->kernel_events.push_back(ev);
    return hipEventRecord(ev, ctx->stream);
}

// An event before and one behind a launch of the level's dominant kernel; nothing but the launch when `slot` is null (mode 2 is
// off, or the level is below the launch filter).
struct LaunchMarks {
    flow2d_context* ctx;
    flow2d_timing_slot* slot;
    template <class Launch>
    int around(Launch launch) const
    {
        if (slot) FLOW2D_HIP_TRY(mark(ctx, slot));
        const int status = launch();
        if (status != FLOW2D_OK) return status;
        if (slot) FLOW2D_HIP_TRY(mark(ctx, slot));
        return FLOW2D_OK;
    }
};

using flow2d::ConstPair;
using flow2d::Pair;
using flow2d::SolveLevel;

// The caller's planes as pairs: 0 (flow_du, flow_dv), 1 (temp_du, temp_dv), 2 (phi, ksi).  What a run_* function reports:
struct LevelRun {
    int result_pair = 0;  // 0 or 1: the pair that holds the level's increment
    int launches = 0;     // kernel launches queued (per instance of a group where the kernel is not batched: once)
};

// The reference's loop: phi / ksi, then `inner` Jacobi sweeps that ping-pong between the two pairs, or red-black iterations in place.
int run_per_sweep(const flow2d_context* ctx, const SolveLevel& level, const Pair* pairs, size_t outer, size_t inner,
                  const LaunchMarks& marks, LevelRun& run)
{
    int at = 0;  // the pair holding du, dv
    for (size_t i = 0; i < outer; ++i) {
        int st = flow2d::launch_phi_ksi(ctx, level, pairs[at], pairs[2]);
        if (st != FLOW2D_OK) return st;
        for (size_t j = 0; j < inner; ++j) {
            if (level.sor_omega != 0.f) {  // opt-in: in place, no ping-pong
                st = flow2d::launch_sor_iteration(ctx, level, pairs[at], pairs[2]);
                if (st != FLOW2D_OK) return st;
                run.launches += 2;
            } else {
                st = marks.around([&] { return flow2d::launch_sweep(ctx, level, pairs[at], pairs[2], pairs[1 - at]); });
                if (st != FLOW2D_OK) return st;
                at = 1 - at;
                ++run.launches;
            }
        }
    }
    run.result_pair = at;
    return FLOW2D_OK;
}

// launches per outer iteration of the strips: five sweeps at most in one (red-black iterations: two half-sweep stages each, at
// most two iterations per launch)
size_t fused_chunks(size_t inner, bool sor)
{
    const size_t per_launch_max = sor ? 2 : 5;
    return std::max<size_t>(1, (inner + per_launch_max - 1) / per_launch_max);
}

// Fused path: one launch per outer iteration does phi/ksi and up to 5 sweeps (solve_fused_kernel.hpp); phi and ksi
// are not materialised, so their planes serve as a third (du, dv) pair.  More than 5 sweeps per outer
// iteration are split into equal chunks: every chunk rebuilds the coefficients from the outer iteration's
// starting pair (same arithmetic, same values) and continues the sweeps from the previous chunk's result.
int run_fused(const flow2d_context* ctx, const SolveLevel& level, const Pair* pairs, size_t outer, size_t inner,
              const LaunchMarks& marks, LevelRun& run)
{
#ifdef FLOW2D_DEV_BUILD  // uniform strips of that many rows instead of the planner's choice
    static const int rows_env = std::getenv("FLOW2D_FUSED_ROWS") ? std::atoi(std::getenv("FLOW2D_FUSED_ROWS")) : 0;
    const int rows = rows_env > 0 ? rows_env : 0;
#else
    const int rows = 0;  // the launcher plans the strip heights (solve_fused.hip, FusedPlan)
#endif
    const bool sor = level.sor_omega != 0.f;
    const size_t chunks = fused_chunks(inner, sor);
    int source = 0;  // pair holding du, dv at the start of the outer iteration
    for (size_t i = 0; i < outer; ++i) {
        int in = source;
        for (size_t c = 0; c < chunks; ++c) {
            const size_t sweeps = inner / chunks + (c < inner % chunks ? 1 : 0);
            int out = 0;
            while (out == source || out == in) ++out;
            const int st = marks.around([&] {
                return flow2d::launch_fused_outer(ctx, level, pairs[source], pairs[out], sor ? 2 * sweeps : sweeps, i == 0,
                                                  c == 0 ? ConstPair{nullptr, nullptr} : ConstPair(pairs[in]), rows);
            });
            if (st != FLOW2D_OK) return st;
            in = out;
            ++run.launches;
        }
        source = in;
    }
    if (source == 2) {  // the caller only knows two pairs: hand the result over
        for (unsigned b = 0; b < ctx->batch_count; ++b) {
            const Pair from = shifted(pairs[2], b * ctx->batch_stride_floats), to = shifted(pairs[0], b * ctx->batch_stride_floats);
            FLOW2D_HIP_TRY(hipMemcpy2DAsync(to.du, level.pitch_bytes, from.du, level.pitch_bytes, level.w * sizeof(float), level.h,
                                            hipMemcpyDeviceToDevice, ctx->stream));
            FLOW2D_HIP_TRY(hipMemcpy2DAsync(to.dv, level.pitch_bytes, from.dv, level.pitch_bytes, level.w * sizeof(float), level.h,
                                            hipMemcpyDeviceToDevice, ctx->stream));
        }
        source = 0;
    }
    run.result_pair = source;
    return FLOW2D_OK;
}

// Tiled path: one launch per outer iteration, ping-pong between the caller's two pairs.  (Round 5 tried TWO outer
// iterations per launch of the 8 x 8 and 16 x 16 tiles over a halo of 2 (inner + 1) pixels -- half the launches of the
// launch-bound levels: the regions of 32 x 32 / 40 x 40 pixels recompute 16x / 6x the tile and a lone 1024^2 pair took 0.76
// instead of 0.71 ms, a lone 4096^2 pair 4.24 instead of 4.08-4.17, the pipelined rates 1 % less:
// profiles/r05_experiments/tile_two_outer_ab.txt.  Not kept.)
int run_tiled(const flow2d_context* ctx, const SolveLevel& level, const Pair* pairs, size_t outer, size_t inner,
              const LaunchMarks& marks, LevelRun& run)
{
    const size_t stages = level.sor_omega != 0.f ? 2 * inner : inner;
    int source = 0;
    for (size_t i = 0; i < outer; ++i) {
        const int st = marks.around(
            [&] { return flow2d::launch_tiled_outer(ctx, level, pairs[source], pairs[1 - source], stages, i == 0); });
        if (st != FLOW2D_OK) return st;
        source = 1 - source;
        ++run.launches;
    }
    run.result_pair = source;
    return FLOW2D_OK;
}

// The whole level in one launch (per instance), written to the caller's first pair.
int run_single_workgroup(const flow2d_context* ctx, const SolveLevel& level, const Pair* pairs, size_t outer, size_t inner,
                         const LaunchMarks& marks, LevelRun& run)
{
    run.launches = 1;
    return marks.around([&] { return flow2d::launch_small_level(ctx, level, outer, inner, pairs[0]); });
}
}  // namespace

// largest level (pixels) AUTO gives to the tiled kernel (developer builds, -DFLOW2D_DEV_BUILD: the environment variable
// FLOW2D_TILED_MAX_PIXELS overrides; the product library reads no environment variable here).  Measured
// against the strips as they are at the end of round 3 (tools/time_levels.py; level solve 10 x 5, tiles / strips, ms):
// Grey 384^2 0.111 / 0.115, 512^2 0.119 / 0.165, 640^2 0.193 / 0.170, 768^2 0.253 / 0.181, 1024^2 0.340 / 0.260;
// Gradient 512^2 0.127 / 0.183, 640^2 0.207 / 0.182, 1024^2 0.366 / 0.280, 1920 x 1080 0.679 / 0.393.
static size_t tiled_max_pixels(int data_constancy)
{
#ifdef FLOW2D_DEV_BUILD
    static const long long forced = std::getenv("FLOW2D_TILED_MAX_PIXELS") ? std::atoll(std::getenv("FLOW2D_TILED_MAX_PIXELS")) : -1;
    if (forced >= 0) return static_cast<size_t>(forced);
#endif
    (void)data_constancy;  // the same crossover for the brightness and the gradient terms
    return static_cast<size_t>(600) * 600;
}

// `instances`: pairs of a lock-step group that share every launch (flow2d_context_set_batch; 1 for a single pair)
static int solver_algorithm_for(int requested, size_t width, size_t height, size_t pitch_bytes, size_t outer, size_t inner,
                                int data_constancy, size_t instances)
{
    if (requested < FLOW2D_SOLVER_AUTO || requested > FLOW2D_SOLVER_TILED) return -1;
    if (requested == FLOW2D_SOLVER_AUTO) {
        // Up to tiled_max_pixels (600^2) the outer iteration runs on small LDS tiles (solve_tile.hip): a strip wave
        // needs (rows + halo) x ~1 us whatever the level size, tiles spread a small level over the whole chip
        // (level solve 10 x 5 at 256^2: 0.07 against 0.11 ms, at 512^2 0.12 against 0.17, at 640^2 0.19 against 0.17).
        // That includes the coarsest levels: ten launches of a few
        // 8 x 8 tiles take 0.05 ms at 16 x 16 ... 64 x 32, the single-workgroup kernel 0.06 ... 0.11 ms.
        // A lock-step group moves the crossover down with the square of its size: its instances share the strips' launch
        // (longer strips, the planner sees all of them) and, in a pipeline of several lanes, a few strip waves find room
        // beside another lane's kernels where 1024-thread tile workgroups with their LDS wait (config 2, groups of four:
        // 3 416-3 439 pairs/s with the tiles up to 600^2 per instance, 3 524-3 567 up to 64^2 ... 128^2; config 4, groups
        // of eight: 2 168-2 197 -> 2 224-2 239; groups of two at 4096^2: no difference).
        if (inner >= 2 && width * height * instances * instances <= tiled_max_pixels(data_constancy) &&
            flow2d::tiled_supports(data_constancy, inner))
            return FLOW2D_SOLVER_TILED;
        // Where the tiled kernel does not apply (solve_2d_log, a single sweep per outer iteration), levels up to 64 x 32
        // run whole in one launch on one CU (solve_small.hip; 0.06-0.10 ms against 0.16-0.19 ms for 60 per-sweep launches;
        // at 64 x 64 four pixels per thread spill and lose).
        if (flow2d::small_level_supports(width, height) && height <= 32) return FLOW2D_SOLVER_SINGLE_WORKGROUP;
        // Everything else goes through the fused strip kernel (above 512^2 it wins over per-sweep launches by 1.7-2.9x).
        // A single sweep per outer iteration leaves nothing to fuse, and a plane of 4 GiB or more is beyond the fused
        // kernel's 32-bit byte offsets: both take the per-sweep kernels.
        return (inner >= 2 && flow2d::fused_addressable(height, pitch_bytes)) ? FLOW2D_SOLVER_FUSED : FLOW2D_SOLVER_PER_SWEEP;
    }
    if (requested == FLOW2D_SOLVER_TILED && !flow2d::tiled_supports(data_constancy, inner)) return -1;
    if (requested == FLOW2D_SOLVER_SINGLE_WORKGROUP && !flow2d::small_level_supports(width, height)) return -1;
    if (requested == FLOW2D_SOLVER_FUSED) {
        if (inner == 0 && outer != 0) return -1;  // nothing to fuse: an outer iteration without sweeps leaves du, dv as they are
        if (!flow2d::fused_addressable(height, pitch_bytes)) return -1;
    }
    return requested;
}

// The algorithm flow2d_solve_level runs for these parameters (never AUTO), or the status it returns instead: everything it checks but
// the planes, for flow2d_solve_level and flow2d_solve_level_takes_half_base alike.  Pure host logic: the
// same answer for an eager run and while a graph is recorded.
static int resolve_level_algorithm(const flow2d_solve_params* p, size_t instances, int& algorithm)
{
    if (p->width < 2 || p->height < 2 || p->container_height < p->height || !(p->hx > 0.f) || !(p->hy > 0.f))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (p->data_constancy != FLOW2D_CONSTANCY_GREY && p->data_constancy != FLOW2D_CONSTANCY_GRADIENT &&
        p->data_constancy != FLOW2D_CONSTANCY_GRADIENT_UNTILED && p->data_constancy != FLOW2D_CONSTANCY_LOG_DERIVATIVES)
        return FLOW2D_ERR_UNSUPPORTED;
    if (p->algorithm < FLOW2D_SOLVER_AUTO || p->algorithm > FLOW2D_SOLVER_TILED)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const bool sor = p->sor_omega != 0.f;
    if (sor && (!(p->sor_omega > 0.f) || !(p->sor_omega < 2.f))) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (sor && p->data_constancy == FLOW2D_CONSTANCY_LOG_DERIVATIVES) return FLOW2D_ERR_UNSUPPORTED;
    algorithm = solver_algorithm_for(p->algorithm, p->width, p->height, p->pitch_bytes, p->outer_iterations_count,
                                     p->inner_iterations_count, p->data_constancy, instances);
    // Red-black SOR (opt-in): temporally blocked in the strip kernel and in the LDS tiles with half-sweeps for stages (round 5: one
    // launch per two iterations instead of a phi / ksi launch and two half-sweep launches per iteration).  AUTO picks tiles or
    // strips by the level's size like for Jacobi (the tiles up to two iterations per outer iteration; the single-workgroup kernel
    // has no such stages); only what the strips cannot address, or an explicit request, takes the half-sweep launches.
    if (sor) {
        // stages of a launch = half-sweeps: the tiles hold up to four (two iterations), the strips chain launches of four
        const size_t stages = 2 * p->inner_iterations_count;
        const bool can_fuse = p->inner_iterations_count >= 1 && flow2d::fused_addressable(p->height, p->pitch_bytes);
        const bool can_tile = p->inner_iterations_count >= 1 && stages <= 4 && flow2d::tiled_supports(p->data_constancy, stages);
        const bool auto_tiles = can_tile && solver_algorithm_for(FLOW2D_SOLVER_AUTO, p->width, p->height, p->pitch_bytes,
                                                                 p->outer_iterations_count, stages, p->data_constancy,
                                                                 instances) == FLOW2D_SOLVER_TILED;
        if (p->algorithm == FLOW2D_SOLVER_FUSED && !can_fuse) return FLOW2D_ERR_UNSUPPORTED;
        if (p->algorithm == FLOW2D_SOLVER_TILED && !can_tile) return FLOW2D_ERR_UNSUPPORTED;
        if (p->algorithm == FLOW2D_SOLVER_SINGLE_WORKGROUP) return FLOW2D_ERR_UNSUPPORTED;
        if (p->algorithm == FLOW2D_SOLVER_AUTO)
            algorithm = auto_tiles ? FLOW2D_SOLVER_TILED : (can_fuse ? FLOW2D_SOLVER_FUSED : FLOW2D_SOLVER_PER_SWEEP);
        else
            algorithm = p->algorithm;
    }
    if (algorithm < 0) return FLOW2D_ERR_UNSUPPORTED;
    // the strips multiply with half the neighbour weight alpha / h^2, which must be exactly representable (solve_fused.hip)
    if (algorithm == FLOW2D_SOLVER_FUSED && !flow2d::fused_weights_ok(p->hx, p->hy, p->equation_alpha)) {
        if (p->algorithm == FLOW2D_SOLVER_FUSED) return FLOW2D_ERR_UNSUPPORTED;
        algorithm = FLOW2D_SOLVER_PER_SWEEP;
    }

    return FLOW2D_OK;
}

extern "C" {

// The algorithm flow2d_solve_level runs for a request (never AUTO) on a single pair, or -1 when the requested one cannot
// run the level.  Pure host logic, no device needed.  (In a lock-step group AUTO gives fewer levels to the tiles: above.)
int flow2d_solver_algorithm_for(int requested, size_t width, size_t height, size_t pitch_bytes, size_t outer, size_t inner,
                                int data_constancy)
{
    return solver_algorithm_for(requested, width, height, pitch_bytes, outer, inner, data_constancy, 1);
}

int flow2d_solve_level(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* flow_u,
                       const float* flow_v, float* flow_du, float* flow_dv, float* phi, float* ksi, float* temp_du,
                       float* temp_dv, const flow2d_solve_params* p, int* result_in_temp)
{
    FLOW2D_ENTER(ctx);
    if (!p || !result_in_temp) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float* planes[] = {frame_0, frame_1, flow_u, flow_v, flow_du, flow_dv, phi, ksi, temp_du, temp_dv};
    for (int i = 0; i < 10; ++i) {
        // (flow_u and flow_v hold fewer rows and columns with base_flow_shift = 1; what is checked here does not depend on that)
        if (!flow2d::plane_args_ok(planes[i], p->width, p->height, p->pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    }
    const bool sor = p->sor_omega != 0.f;
    int algorithm = -1;
    {
        const int status = resolve_level_algorithm(p, ctx->batch_count, algorithm);
        if (status != FLOW2D_OK) return status;
    }
    // a half-size base flow is read by the strips only
    if (p->base_flow_shift != 0 && (p->base_flow_shift != 1 || algorithm != FLOW2D_SOLVER_FUSED)) return FLOW2D_ERR_UNSUPPORTED;
    // du = dv = 0 over level width x container height (cuda_operation_solve_2d.cpp:229-232).  The fused path
    // starts its first outer iteration from zero increments without reading the planes, so it needs no memset.
    const bool one_per_outer = algorithm == FLOW2D_SOLVER_FUSED || algorithm == FLOW2D_SOLVER_TILED;
    const bool zero_increments = algorithm == FLOW2D_SOLVER_PER_SWEEP || (one_per_outer && p->outer_iterations_count == 0);
    {   // The six written planes may meet nothing, over every instance of a lock-step group: whichever algorithm runs, it gets its
        // planes from here.  (flow_du / flow_dv count with the rows of the memset where there is one; a half-size base flow with its own.)
        const size_t bytes = p->height * p->pitch_bytes, base_bytes = (p->base_flow_shift ? (p->height + 1) / 2 : p->height) * p->pitch_bytes;
        const size_t zeroed = (zero_increments ? p->container_height : p->height) * p->pitch_bytes;
        const flow2d::ByteRange written[] = {{flow_du, zeroed}, {flow_dv, zeroed}, {phi, bytes}, {ksi, bytes}, {temp_du, bytes}, {temp_dv, bytes}};
        const flow2d::ByteRange read[] = {{frame_0, bytes}, {frame_1, bytes}, {flow_u, base_bytes}, {flow_v, base_bytes}};
        if (flow2d::any_overlap(written, read, flow2d::batch_instances(ctx))) return FLOW2D_ERR_INVALID_ARGUMENT;
    }

    flow2d_timing_slot* slot = nullptr;
    if (ctx->timing) {
        flow2d_timing_slot s{};
        FLOW2D_HIP_TRY(take_event(ctx, &s.start));
        FLOW2D_HIP_TRY(take_event(ctx, &s.stop));
        ctx->timings.push_back(s);
        slot = &ctx->timings.back();
        FLOW2D_HIP_TRY(hipEventRecord(slot->start, ctx->stream));
    }

    if (zero_increments) {
        for (unsigned b = 0; b < ctx->batch_count; ++b) {
            FLOW2D_HIP_TRY(hipMemset2DAsync(flow_du + b * ctx->batch_stride_floats, p->pitch_bytes, 0,
                                            p->width * sizeof(float), p->container_height, ctx->stream));
            FLOW2D_HIP_TRY(hipMemset2DAsync(flow_dv + b * ctx->batch_stride_floats, p->pitch_bytes, 0,
                                            p->width * sizeof(float), p->container_height, ctx->stream));
        }
    }

    const bool per_launch = slot && ctx->timing >= 2 && p->width >= ctx->timing_min_w && p->height >= ctx->timing_min_h;
    const LaunchMarks marks{ctx, per_launch ? slot : nullptr};
    const SolveLevel level{p->data_constancy, frame_0, frame_1, flow_u, flow_v, p->width, p->height, p->pitch_bytes,
                           p->hx, p->hy, p->equation_alpha, p->equation_smoothness, p->equation_data,
                           sor ? p->sor_omega : 0.f, p->base_flow_shift};
    const Pair pairs[3] = {{flow_du, flow_dv}, {temp_du, temp_dv}, {phi, ksi}};
    const auto run_algorithm = algorithm == FLOW2D_SOLVER_FUSED   ? run_fused
                               : algorithm == FLOW2D_SOLVER_TILED ? run_tiled
                               : algorithm == FLOW2D_SOLVER_SINGLE_WORKGROUP ? run_single_workgroup
                                                                             : run_per_sweep;
    LevelRun run;
    {
        const int status = run_algorithm(ctx, level, pairs, p->outer_iterations_count, p->inner_iterations_count, marks, run);
        if (status != FLOW2D_OK) return status;
    }
    *result_in_temp = run.result_pair;

    if (slot) {
        FLOW2D_HIP_TRY(hipEventRecord(slot->stop, ctx->stream));
        slot->rec.width = p->width;
        slot->rec.height = p->height;
        slot->rec.outer = p->outer_iterations_count;
        slot->rec.inner = p->inner_iterations_count;
        slot->rec.data_constancy = p->data_constancy;
        slot->rec.algorithm = algorithm;
        slot->rec.kernel_launches = run.launches;
        slot->rec.elapsed_ms = -1.f;
        slot->rec.kernel_ms = -1.f;
        double per_px = 40.0;  // one Jacobi sweep
        if (algorithm == FLOW2D_SOLVER_FUSED)  // an outer iteration's bytes, spread over its launches
            per_px = (32.0 + 40.0 * p->inner_iterations_count) / static_cast<double>(fused_chunks(p->inner_iterations_count, sor));
        if (algorithm == FLOW2D_SOLVER_TILED) per_px = 32.0 + 40.0 * p->inner_iterations_count;
        if (algorithm == FLOW2D_SOLVER_SINGLE_WORKGROUP)
            per_px = p->outer_iterations_count * (32.0 + 40.0 * p->inner_iterations_count);
        slot->rec.algorithmic_bytes_per_launch = per_px * static_cast<double>(p->width) * static_cast<double>(p->height);
    }
    return FLOW2D_OK;
}

// Whether flow2d_solve_level would run these parameters with base_flow_shift = 1 (the field itself is not looked at): the level
// resolves to the strips on this context -- its lock-step group counts -- and its planes are within their 32-bit offsets.
int flow2d_solve_level_takes_half_base(flow2d_context* ctx, const flow2d_solve_params* p)
{
    if (!ctx || !p || p->outer_iterations_count == 0) return 0;  // (no outer iteration: no strip launch at all)
    int algorithm = -1;
    if (resolve_level_algorithm(p, ctx->batch_count, algorithm) != FLOW2D_OK) return 0;
    return algorithm == FLOW2D_SOLVER_FUSED && flow2d::fused_addressable(p->height, p->pitch_bytes) ? 1 : 0;
}

int flow2d_timing_enable(flow2d_context* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return FLOW2D_ERR_INVALID_ARGUMENT;
    ctx->timing = mode;
    return FLOW2D_OK;
}

int flow2d_timing_launch_filter(flow2d_context* ctx, size_t min_width, size_t min_height)
{
    if (!ctx) return FLOW2D_ERR_INVALID_ARGUMENT;
    ctx->timing_min_w = min_width;
    ctx->timing_min_h = min_height;
    return FLOW2D_OK;
}

int flow2d_timing_count(flow2d_context* ctx, size_t* count)
{
    if (!ctx || !count) return FLOW2D_ERR_INVALID_ARGUMENT;
    *count = ctx->timings.size();
    return FLOW2D_OK;
}

int flow2d_timing_get(flow2d_context* ctx, size_t index, flow2d_timing_record* out)
{
    FLOW2D_ENTER(ctx);
    if (!out || index >= ctx->timings.size()) return FLOW2D_ERR_INVALID_ARGUMENT;
    flow2d_timing_slot& s = ctx->timings[index];
    if (s.rec.elapsed_ms < 0.f) {
        FLOW2D_HIP_TRY(hipEventSynchronize(s.stop));
        FLOW2D_HIP_TRY(hipEventElapsedTime(&s.rec.elapsed_ms, s.start, s.stop));
        if (!s.kernel_events.empty()) {
            float total = 0.f;
            for (size_t k = 0; k + 1 < s.kernel_events.size(); k += 2) {
                float ms = 0.f;
                FLOW2D_HIP_TRY(hipEventElapsedTime(&ms, s.kernel_events[k], s.kernel_events[k + 1]));
                total += ms;
            }
            s.rec.kernel_ms = total;
        }
    }
    *out = s.rec;
    return FLOW2D_OK;
}

int flow2d_timing_reset(flow2d_context* ctx)
{
    FLOW2D_ENTER(ctx);
    for (auto& s : ctx->timings) {  // events go back to the pool (destroyed with the context)
        ctx->event_pool.push_back(s.start);
        ctx->event_pool.push_back(s.stop);
        for (hipEvent_t ev : s.kernel_events) ctx->event_pool.push_back(ev);
    }
    ctx->timings.clear();
    return FLOW2D_OK;
}

}  // extern "C"
