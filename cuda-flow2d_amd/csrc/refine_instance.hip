// One radius of the refinement kernel: compiled once per FLOW2D_REFINE_RADIUS = 1 .. 7 (Makefile), refine_kernel.hpp.
#include "refine_kernel.hpp"

#ifndef FLOW2D_REFINE_RADIUS
#error "compile with -DFLOW2D_REFINE_RADIUS=1 .. 7"
#endif
#define FLOW2D_REFINE_NAME2(r) flow2d_refine_launch_r##r
#define FLOW2D_REFINE_NAME(r) FLOW2D_REFINE_NAME2(r)

void FLOW2D_REFINE_NAME(FLOW2D_REFINE_RADIUS)(flow2d_context* ctx, const RefineArgs& a, bool wide, size_t width, size_t height)
{
    if (wide)
        launch_radius<size_t, FLOW2D_REFINE_RADIUS>(ctx, a, width, height);
    else
        launch_radius<unsigned, FLOW2D_REFINE_RADIUS>(ctx, a, width, height);
}
