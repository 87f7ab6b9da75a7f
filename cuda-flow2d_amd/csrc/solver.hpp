// The solver's internal interface: what the level loop (solve_level.hip) and the C-ABI entries call in the kernel files
// (solve.hip, solve_fused.hip, solve_tile.hip, solve_small.hip).  Every solver translation unit includes this header, so a
// definition that does not match its declaration here does not compile.
#pragma once

#include <cmath>

#include "common.hpp"

namespace flow2d {

// What every launch of a level shares.
struct SolveLevel {
    int constancy;  // flow2d_constancy
    const float* f0;
    const float* f1;
    const float* u;
    const float* v;
    size_t w, h, pitch_bytes;
    float hx, hy, alpha, e_smooth, e_data;
    float sor_omega;      // 0: Jacobi sweeps; in (0, 2): red-black SOR (opt-in)
    int base_flow_shift;  // 1: u and v at half the size in both directions (the strips only)
};

// Two planes that travel together: an increment (du, dv), or the coefficients (phi, ksi) in the same two seats.
struct ConstPair {
    const float* du;
    const float* dv;
};
struct Pair {
    float* du;
    float* dv;
    operator ConstPair() const { return ConstPair{du, dv}; }
};

// instance b of a lock-step group: every plane `floats` further
inline SolveLevel shifted(SolveLevel l, size_t floats)
{
    l.f0 += floats, l.f1 += floats, l.u += floats, l.v += floats;
    return l;
}
inline ConstPair shifted(ConstPair p, size_t floats) { return ConstPair{p.du + floats, p.dv + floats}; }
inline Pair shifted(Pair p, size_t floats) { return Pair{p.du + floats, p.dv + floats}; }

// The kernels without a batched form: launch(ctx, level, pairs...) once per instance of the context's group, on that instance's planes.
template <class Launch, class... Pairs>
int for_each_instance(const flow2d_context* ctx, const SolveLevel& level, Launch launch, Pairs... pairs)
{
    for (unsigned b = 0; b < ctx->batch_count; ++b) {
        const size_t off = b * ctx->batch_stride_floats;
        const int status = launch(ctx, shifted(level, off), shifted(pairs, off)...);
        if (status != FLOW2D_OK) return status;
    }
    return FLOW2D_OK;
}

// true when x is a normal power of two whose reciprocal (and 1/(2x), 1/(4x)) is exactly representable
inline bool is_power_of_two(float x)
{
    int e = 0;
    return x > 0.f && std::frexp(x, &e) == 0.5f && e > -100 && e < 100;
}

// ---- solve.hip: one launch per reference kernel launch (per instance of a group) ----
int launch_phi_ksi(const flow2d_context* ctx, const SolveLevel& level, ConstPair d, Pair coeff);
int launch_sweep(const flow2d_context* ctx, const SolveLevel& level, ConstPair d, ConstPair coeff, Pair out);
// one red-black iteration (two half-sweeps) with level.sor_omega, in place on d
int launch_sor_iteration(const flow2d_context* ctx, const SolveLevel& level, Pair d, ConstPair coeff);

// ---- solve_small.hip: all outer x inner iterations in one workgroup ----
bool small_level_supports(size_t w, size_t h);
int launch_small_level(const flow2d_context* ctx, const SolveLevel& level, size_t outer, size_t inner, Pair out);

// ---- solve_tile.hip: one outer iteration on LDS tiles.  `stages`: Jacobi sweeps, or half-sweeps with level.sor_omega ----
bool tiled_supports(int constancy, size_t stages);
int launch_tiled_outer(const flow2d_context* ctx, const SolveLevel& level, ConstPair in, Pair out, size_t stages,
                       bool zero_increment);

// ---- solve_fused.hip: one outer iteration (or a chunk of its sweeps) on strips ----
bool fused_supports(size_t stages);
bool fused_addressable(size_t h, size_t pitch_bytes);
bool fused_weights_ok(float hx, float hy, float alpha);
// start: {nullptr, nullptr}, or the previous chunk's result, whose sweeps this launch continues
// rows_per_strip > 0: uniform strips of that height (developer override); 0: the planner's choice
int launch_fused_outer(const flow2d_context* ctx, const SolveLevel& level, ConstPair in, Pair out, size_t stages,
                       bool zero_increment, ConstPair start, int rows_per_strip);

// The instance objects of the strip kernel (solve_fused_instance.hip, one per data term g and spacing kind p): each launches
// fused_outer_kernel<inner, GRAD, POW2, CONT> (CONT from a.continue_sweeps) and returns non-zero when it holds no such
// instantiation (inner outside 1..5, or a developer build's reduced set).
struct FusedArgs;
using FusedLaunch = int(int inner, dim3 grid, hipStream_t stream, const FusedArgs& a);
FusedLaunch fused_launch_g0_p0, fused_launch_g0_p1, fused_launch_g1_p0, fused_launch_g1_p1, fused_launch_g2_p0, fused_launch_g2_p1,
    fused_launch_g3_p0, fused_launch_g3_p1;
// the packed build of the same kernels (not of the log-derivative term, whose one build is packed already)
FusedLaunch fused_launch_g0_p0_k, fused_launch_g0_p1_k, fused_launch_g1_p0_k, fused_launch_g1_p1_k, fused_launch_g2_p0_k,
    fused_launch_g2_p1_k;

}  // namespace flow2d
