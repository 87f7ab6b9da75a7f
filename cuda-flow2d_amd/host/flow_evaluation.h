// Error of a flow estimate against ground truth on the device (flow2d_flow_error_2d), for host images: no reference counterpart.
// EvaluateFlow uploads the planes into containers of its own, owns the kernel's workspace, runs the two launches on the
// process-wide context (InitDeviceContext / AdoptDeviceContext) and waits for the record.  FlowErrorJson formats a record as
// the metrics the CLI prints after --ground-truth.
#pragma once

#include <string>

#include "data2d.h"
#include "flow2d_c_abi.h"

// u, v: the estimate; gt_u, gt_v: ground truth; occlusion (optional): non-zero or NaN = occluded; epe / ae (optional): the
// per-pixel errors (resized to the inputs' size).  All inputs of one size.  False (and a message) when the sizes differ, there
// is no context, or a device call fails; `out` is then untouched.
bool EvaluateFlow(Data2D& u, Data2D& v, Data2D& gt_u, Data2D& gt_v, Data2D* occlusion, flow2d_flow_error_stats& out,
                  Data2D* epe = nullptr, Data2D* ae = nullptr);

// {"all": {...}, "noc": {...}, "occ": {...}, "invalid_ground_truth": n, "nonfinite_estimate": n} with, per class, "count",
// "epe" (mean), "rmse" (sqrt of the mean squared EPE), "ae" (mean, degrees), "r0.5", "r1", "r2", "r3" and "fl" (fractions of
// the class) and "max_epe".  Means and fractions are null for an empty class; doubles are printed with 17 significant digits
// (round trip), non-finite ones as Infinity / NaN (what Python's json module reads).
std::string FlowErrorJson(const flow2d_flow_error_stats& stats);
