"""Python plumbing for the MI355X-native flow2d hot path (ctypes over the C-ABI).

The product is the HIP library (csrc/ -> libflow2d_hip.so, include/flow2d_c_abi.h) and the C++ host
layer (host/ -> libflow2d_host.so, `flow2d` CLI) that mirrors the reference's OpticalFlow2D /
CudaOperation* interface.  This module only loads those libraries for tests/ and bench.py; it holds
no algorithm and has NO CPU fallback: a missing library or a failing call raises.

The directory name carries a hyphen, so import it with
    importlib.import_module("cuda-flow2d_amd")
"""
import collections
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
# FLOW2D_HIP_LIB: an experimental build of the HIP library (ab/*.so, tools/ab_time.sh) instead of the in-tree one
HIP_LIB_PATH = os.environ.get("FLOW2D_HIP_LIB") or os.path.join(_HERE, "csrc", "libflow2d_hip.so")
HOST_LIB_PATH = os.path.join(_HERE, "host", "libflow2d_host.so")
CLI_PATH = os.path.join(_HERE, "host", "flow2d")

# flow2d_constancy; 2 = true-neighbour gradient term (not in the reference), 3 = the reference's LogDerivatives
GREY, GRADIENT, GRADIENT_UNTILED, LOG_DERIVATIVES = 0, 1, 2, 3
_HOST_CONSTANCY = {GREY: 0, GRADIENT: 1, GRADIENT_UNTILED: 3, LOG_DERIVATIVES: 2}  # enum class DataConstancy
SOLVER_AUTO, SOLVER_PER_SWEEP, SOLVER_FUSED, SOLVER_SINGLE_WORKGROUP, SOLVER_TILED = 0, 1, 2, 3, 4
# flow2d_track_reason; DEFAULT_MIN_EIGENVALUE: the seeding threshold of OpticalFlow.track_points and the CLI's --track
TRACK_ALIVE, TRACK_INACTIVE, TRACK_MOTION_BOUNDARY, TRACK_LEFT_FRAME, TRACK_OCCLUDED = 0, 1, 2, 3, 4
DEFAULT_MIN_EIGENVALUE = 1.0
# flow2d_motion_model; MOTION_MODELS: the names the CLI's --global-motion takes
MOTION_TRANSLATION, MOTION_SIMILARITY, MOTION_AFFINE = 0, 1, 2
MOTION_MODELS = {"translation": MOTION_TRANSLATION, "similarity": MOTION_SIMILARITY, "affine": MOTION_AFFINE}

STATUS = {0: "ok", 1: "invalid argument", 2: "no usable HIP device", 3: "HIP runtime error",
          4: "out of device memory", 5: "unsupported parameter"}


class Flow2DError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__("%s failed: status %d (%s)%s" % (where, status, STATUS.get(status, "?"),
                                                          (": " + detail) if detail else ""))


def build(jobs=8):
    """Compile every native piece in-tree: HIP kernels + C-ABI (hipcc, gfx950) and the C++ host layer."""
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", os.path.join(_HERE, "csrc")])
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", os.path.join(_HERE, "host")])


class SolveParams(C.Structure):
    _fields_ = [
        ("width", C.c_size_t), ("height", C.c_size_t), ("pitch_bytes", C.c_size_t),
        ("container_height", C.c_size_t), ("hx", C.c_float), ("hy", C.c_float),
        ("equation_alpha", C.c_float), ("equation_smoothness", C.c_float), ("equation_data", C.c_float),
        ("outer_iterations_count", C.c_size_t), ("inner_iterations_count", C.c_size_t),
        ("data_constancy", C.c_int), ("algorithm", C.c_int), ("sor_omega", C.c_float),
        ("base_flow_shift", C.c_int),
    ]


class TimingRecord(C.Structure):
    _fields_ = [
        ("width", C.c_size_t), ("height", C.c_size_t), ("outer", C.c_size_t), ("inner", C.c_size_t),
        ("data_constancy", C.c_int), ("algorithm", C.c_int), ("kernel_launches", C.c_int),
        ("elapsed_ms", C.c_float), ("kernel_ms", C.c_float), ("algorithmic_bytes_per_launch", C.c_double),
    ]


class FlowErrorClass(C.Structure):
    """flow2d_flow_error_class of include/flow2d_c_abi.h: one class (all / noc / occ) of a flow2d_flow_error_2d record."""
    _fields_ = [
        ("count", C.c_ulonglong), ("above", C.c_ulonglong * 4), ("fl", C.c_ulonglong),
        ("sum_epe", C.c_double), ("sum_epe_sq", C.c_double), ("sum_ae", C.c_double), ("max_epe", C.c_double),
    ]


class FlowErrorStats(C.Structure):
    """flow2d_flow_error_stats: the record flow2d_flow_error_2d writes per instance."""
    _fields_ = [
        ("all", FlowErrorClass), ("noc", FlowErrorClass), ("occ", FlowErrorClass),
        ("invalid_ground_truth", C.c_ulonglong), ("nonfinite_estimate", C.c_ulonglong),
    ]


FLOW_ERROR_STATS_BYTES = 256  # FLOW2D_FLOW_ERROR_STATS_BYTES, checked by a static_assert in the header
assert C.sizeof(FlowErrorStats) == FLOW_ERROR_STATS_BYTES
FLOW_ERROR_CLASSES = ("all", "noc", "occ")


def _stats_dict(rec):
    """A FlowErrorStats as plain Python: {"all" / "noc" / "occ": {count, above (list of 4), fl, sum_epe, sum_epe_sq, sum_ae,
    max_epe}, "invalid_ground_truth", "nonfinite_estimate"}."""
    out = {}
    for name in FLOW_ERROR_CLASSES:
        c = getattr(rec, name)
        out[name] = {"count": c.count, "above": list(c.above), "fl": c.fl, "sum_epe": c.sum_epe, "sum_epe_sq": c.sum_epe_sq,
                     "sum_ae": c.sum_ae, "max_epe": c.max_epe}
    out["invalid_ground_truth"] = rec.invalid_ground_truth
    out["nonfinite_estimate"] = rec.nonfinite_estimate
    return out


def flow_error_metrics(record):
    """The metrics of a flow_error / evaluate_flow record, as the CLI prints them after --ground-truth (FlowErrorJson): per
    class count, epe (mean), rmse, ae (mean, degrees), r0.5 / r1 / r2 / r3 / fl (fractions) and max_epe; None for the means
    and fractions of an empty class.  Same double operations as the C++ side."""
    out = {}
    for name in FLOW_ERROR_CLASSES:
        c = record[name]
        n = float(c["count"])
        empty = c["count"] == 0
        m = {"count": c["count"]}
        m["epe"] = None if empty else c["sum_epe"] / n
        m["rmse"] = None if empty else float(np.sqrt(c["sum_epe_sq"] / n))
        m["ae"] = None if empty else c["sum_ae"] / n
        for key, k in (("r0.5", 0), ("r1", 1), ("r2", 2), ("r3", 3)):
            m[key] = None if empty else c["above"][k] / n
        m["fl"] = None if empty else c["fl"] / n
        m["max_epe"] = c["max_epe"]
        out[name] = m
    out["invalid_ground_truth"] = record["invalid_ground_truth"]
    out["nonfinite_estimate"] = record["nonfinite_estimate"]
    return out


class GlobalMotion(C.Structure):
    """flow2d_global_motion of include/flow2d_c_abi.h: the record flow2d_global_motion_2d writes per instance.  In centred
    coordinates xc = x - (width - 1) / 2, yc = y - (height - 1) / 2:  u = (p0 + p1*xc) + p2*yc,  v = (p3 + p4*xc) + p5*yc."""
    _fields_ = [
        ("p", C.c_double * 6), ("weight_sum", C.c_double), ("support", C.c_ulonglong), ("model_used", C.c_int),
        ("reserved", C.c_int * 3),
    ]

    @classmethod
    def from_parameters(cls, p, model_used=MOTION_AFFINE):
        """A record holding the six parameters `p` (to upload: Context.upload_motion)."""
        return cls((C.c_double * 6)(*[float(q) for q in p]), 0.0, 0, int(model_used))

    @property
    def parameters(self):
        return np.array(self.p[:], np.float64)


GLOBAL_MOTION_BYTES = 80  # FLOW2D_GLOBAL_MOTION_BYTES, checked by a static_assert in the header
assert C.sizeof(GlobalMotion) == GLOBAL_MOTION_BYTES



class MotionRegion(C.Structure):
    """flow2d_motion_region of include/flow2d_c_abi.h: the record flow2d_segment_motion_2d writes per region."""
    _fields_ = [
        ("area", C.c_ulonglong), ("sum_x", C.c_ulonglong), ("sum_y", C.c_ulonglong), ("sum_u_q16", C.c_longlong),
        ("sum_v_q16", C.c_longlong), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("first", C.c_ulonglong),
    ]

    @property
    def bbox(self):
        return (self.x0, self.y0, self.x1, self.y1)

    @property
    def centroid(self):
        return (self.sum_x / self.area, self.sum_y / self.area)

    @property
    def mean_motion(self):
        """The mean residual motion of the region in pixels (the Q16 sums divided out)."""
        return (self.sum_u_q16 / 65536.0 / self.area, self.sum_v_q16 / 65536.0 / self.area)


class SegmentSummary(C.Structure):
    """flow2d_segment_summary: what flow2d_segment_motion_2d writes per instance."""
    _fields_ = [
        ("region_count", C.c_ulonglong), ("foreground", C.c_ulonglong), ("dropped", C.c_ulonglong), ("recorded", C.c_uint),
        ("reserved", C.c_uint),
    ]


MOTION_REGION_BYTES, SEGMENT_SUMMARY_BYTES = 64, 32  # FLOW2D_MOTION_REGION_BYTES, FLOW2D_SEGMENT_SUMMARY_BYTES
assert C.sizeof(MotionRegion) == MOTION_REGION_BYTES and C.sizeof(SegmentSummary) == SEGMENT_SUMMARY_BYTES
DEFAULT_MAX_REGIONS = 4096


STRAIN_SMALL, STRAIN_GREEN_LAGRANGE = 0, 1  # flow2d_strain_measure
# the planes of flow2d_deformation_2d in the order of flow2d_deformation_planes, and the quantities of its record in theirs
DEFORMATION_PLANES = ("divergence", "vorticity", "dilatation", "exx", "eyy", "exy", "e1", "e2", "max_shear")
DEFORMATION_STATS = ("divergence", "vorticity", "dilatation", "e1", "e2", "max_shear")


class DeformationPlanes(C.Structure):
    """flow2d_deformation_planes: a host struct of nine device pointers, NULL = not requested."""
    _fields_ = [(name, C.c_void_p) for name in DEFORMATION_PLANES]


class DeformationMoments(C.Structure):
    """flow2d_deformation_moments: sum, sum of squares, min and max of one quantity over the valid pixels."""
    _fields_ = [("sum", C.c_double), ("sum_sq", C.c_double), ("min", C.c_float), ("max", C.c_float)]


class DeformationStats(C.Structure):
    """flow2d_deformation_stats of include/flow2d_c_abi.h: what flow2d_deformation_2d writes per instance."""
    _fields_ = ([("valid", C.c_ulonglong), ("invalid", C.c_ulonglong)] + [(name, DeformationMoments) for name in DEFORMATION_STATS] +
                [("reserved", C.c_ulonglong * 12)])

    def summary(self):
        """{quantity: {"mean", "rms", "min", "max"}} over the valid pixels (None for an empty set), with "valid" and "invalid"."""
        out = {"valid": self.valid, "invalid": self.invalid}
        for name in DEFORMATION_STATS:
            m = getattr(self, name)
            out[name] = None if self.valid == 0 else {"mean": m.sum / self.valid, "rms": math.sqrt(m.sum_sq / self.valid),
                                                      "min": m.min, "max": m.max}
        return out


DEFORMATION_STATS_BYTES = 256  # FLOW2D_DEFORMATION_STATS_BYTES, checked by a static_assert in the header
assert C.sizeof(DeformationStats) == DEFORMATION_STATS_BYTES

# the diagnostic planes of flow2d_node_strain_robust_2d in the order of flow2d_node_strain_diagnostics
NODE_STRAIN_DIAGNOSTICS = ("residual", "rejected", "centre")
NODE_STRAIN_MAX_ITERATIONS = 16  # FLOW2D_NODE_STRAIN_MAX_ITERATIONS


class NodeStrainDiagnostics(C.Structure):
    """flow2d_node_strain_diagnostics: a host struct of three device pointers, NULL = not requested."""
    _fields_ = [(name, C.c_void_p) for name in NODE_STRAIN_DIAGNOSTICS]


def node_strain_robust_counts(stats):
    """The three words a robust node strain adds to its DeformationStats record, over the nodes whose passes ran to the end
    (valid, or sparse by what they kept): {"touched": nodes that rejected a tap, "rejected": the taps they rejected, "suspect":
    nodes whose own tap was not kept}."""
    return {"touched": int(stats.reserved[3]), "rejected": int(stats.reserved[4]), "suspect": int(stats.reserved[5])}


# the planes of flow2d_node_strain_weighted_2d's standard deviations in the order of flow2d_strain_sigma_planes
STRAIN_SIGMA_PLANES = ("sigma_ux", "sigma_uy", "sigma_vx", "sigma_vy", "sigma_divergence", "sigma_vorticity", "sigma_exx", "sigma_eyy",
                       "sigma_exy")


class StrainSigmaPlanes(C.Structure):
    """flow2d_strain_sigma_planes: a host struct of nine device pointers, NULL = not requested."""
    _fields_ = [(name, C.c_void_p) for name in STRAIN_SIGMA_PLANES]


def node_strain_weighted_counts(stats):
    """The four words a weighted node strain adds to its DeformationStats record: those of node_strain_robust_counts and
    "unweighable", the nodes of the grid that are usable but have no variance to weight them by."""
    return dict(node_strain_robust_counts(stats), unweighable=int(stats.reserved[6]))


REFINE_MAX_RADIUS = 7  # FLOW2D_REFINE_MAX_RADIUS


class RefineRecord(C.Structure):
    """flow2d_refine_record of include/flow2d_c_abi.h: the four counts flow2d_refine_flow_2d writes per instance."""
    _fields_ = [("pixels", C.c_ulonglong), ("unfilled", C.c_ulonglong), ("filled", C.c_ulonglong), ("changed", C.c_ulonglong)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


REFINE_RECORD_BYTES = 32  # FLOW2D_REFINE_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(RefineRecord) == REFINE_RECORD_BYTES


CORRELATION_MAX_RADIUS, CORRELATION_MAX_RANGE, CORRELATION_MAX_SPACING = 15, 32, 64  # FLOW2D_CORRELATION_MAX_*


class CorrelationRecord(C.Structure):
    """flow2d_correlation_record of include/flow2d_c_abi.h: the four counts flow2d_correlate_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("invalid", C.c_ulonglong), ("rejected", C.c_ulonglong), ("unrefined", C.c_ulonglong)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


CORRELATION_RECORD_BYTES = 32  # FLOW2D_CORRELATION_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(CorrelationRecord) == CORRELATION_RECORD_BYTES


class CorrelationPassRecord(C.Structure):
    """flow2d_correlation_pass_record of include/flow2d_c_abi.h: the six counts flow2d_correlate_offset_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("invalid", C.c_ulonglong), ("rejected", C.c_ulonglong), ("unrefined", C.c_ulonglong),
                ("unpredicted", C.c_ulonglong), ("candidates", C.c_ulonglong), ("reserved", C.c_ulonglong * 2)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_[:6]}

    @property
    def masked(self):
        """The masked nodes: what flow2d_correlate_masked_2d writes into the word the other entries leave 0.  Read-only."""
        return self.reserved[0]


class ValidationRecord(C.Structure):
    """flow2d_validation_record of include/flow2d_c_abi.h: the six counts flow2d_validate_nodes_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("judged", C.c_ulonglong), ("outliers", C.c_ulonglong), ("filled", C.c_ulonglong),
                ("unjudged", C.c_ulonglong), ("remaining_invalid", C.c_ulonglong), ("reserved", C.c_ulonglong * 2)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_[:6]}

    @property
    def masked(self):
        """The off-specimen nodes (flag VALIDATE_FLAG_MASKED): what flow2d_validate_nodes_masked_2d writes into the word the other
        entries leave 0.  Read-only."""
        return self.reserved[0]


CORRELATION_PASS_RECORD_BYTES = VALIDATION_RECORD_BYTES = 64  # FLOW2D_*_RECORD_BYTES, checked by static_asserts in the header
assert C.sizeof(CorrelationPassRecord) == CORRELATION_PASS_RECORD_BYTES and C.sizeof(ValidationRecord) == VALIDATION_RECORD_BYTES
CORRELATION_MAX_PASSES = 6  # FLOW2D_CORRELATION_MAX_PASSES


class SubsetRecord(C.Structure):
    """flow2d_subset_record of include/flow2d_c_abi.h: the seven counts flow2d_subset_refine_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("converged", C.c_ulonglong), ("unconverged", C.c_ulonglong), ("strayed", C.c_ulonglong),
                ("flat", C.c_ulonglong), ("no_input", C.c_ulonglong), ("iterations", C.c_ulonglong), ("reserved", C.c_ulonglong)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_[:7]}

    @property
    def masked(self):
        """The masked nodes (state SUBSET_MASKED): what flow2d_subset_refine_masked_2d writes into the word the other entries
        leave 0.  Read-only."""
        return self.reserved


SUBSET_RECORD_BYTES = 64  # FLOW2D_SUBSET_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(SubsetRecord) == SUBSET_RECORD_BYTES
SUBSET_MAX_RADIUS, SUBSET_MAX_ITERATIONS = 15, 64  # FLOW2D_SUBSET_MAX_*
BSPLINE_HORIZON = 16  # FLOW2D_BSPLINE_HORIZON
SUBSET_NO_INPUT, SUBSET_FLAT, SUBSET_STRAYED = -1, -2, -3  # the negative states of flow2d_subset_refine_2d
SUBSET_CATMULL_ROM, SUBSET_BSPLINE = 0, 1  # OpticalFlow2D::SubsetOptions::Interpolation
SUBSET_INTERPOLATIONS = {"catmull-rom": SUBSET_CATMULL_ROM, "bspline": SUBSET_BSPLINE}
SUBSET_MASKED = -4  # FLOW2D_SUBSET_STATE_MASKED: flow2d_subset_refine_masked_2d's, a node off the region of interest
SUBSET_MIN_PIXELS = 6  # FLOW2D_SUBSET_MIN_PIXELS


def subset_min_pixels(subset_radius):
    """The default min_pixels of a masked refinement (OpticalFlow2D::SubsetOptions::min_pixels = 0): a quarter of the subset,
    rounded up, and six at least."""
    side = 2 * int(subset_radius) + 1
    return max(SUBSET_MIN_PIXELS, (side * side + 3) // 4)
SUBSET_STATE_PREDICTED = 65  # FLOW2D_SUBSET_STATE_PREDICTED: the state flow2d_predict_nodes_2d gives a node it predicted


class PredictRecord(C.Structure):
    """flow2d_predict_record of include/flow2d_c_abi.h: the four counts flow2d_predict_nodes_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("kept", C.c_ulonglong), ("predicted", C.c_ulonglong), ("empty", C.c_ulonglong),
                ("reserved", C.c_ulonglong * 4)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_[:4]}


PREDICT_RECORD_BYTES = 64  # FLOW2D_PREDICT_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(PredictRecord) == PREDICT_RECORD_BYTES
SEQUENCE_MAX_FILL = 4  # OpticalFlow2D::kSequenceMaxFill
SUBSET_STATE_COMPOSED = 66  # FLOW2D_SUBSET_STATE_COMPOSED: the state flow2d_compose_nodes_2d gives a node it composed


class ComposeRecord(C.Structure):
    """flow2d_compose_record of include/flow2d_c_abi.h: the five counts flow2d_compose_nodes_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("composed", C.c_ulonglong), ("no_base", C.c_ulonglong), ("outside", C.c_ulonglong),
                ("no_increment", C.c_ulonglong), ("reserved", C.c_ulonglong * 3)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_[:5]}


COMPOSE_RECORD_BYTES = 64  # FLOW2D_COMPOSE_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(ComposeRecord) == COMPOSE_RECORD_BYTES


class UncertaintyRecord(C.Structure):
    """flow2d_uncertainty_record of include/flow2d_c_abi.h: the seven counts flow2d_subset_uncertainty_2d writes per instance."""
    _fields_ = [("nodes", C.c_ulonglong), ("evaluated", C.c_ulonglong), ("skipped", C.c_ulonglong), ("masked", C.c_ulonglong),
                ("outside", C.c_ulonglong), ("flat", C.c_ulonglong), ("thin", C.c_ulonglong), ("reserved", C.c_ulonglong)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_[:7]}


UNCERTAINTY_RECORD_BYTES = 64  # FLOW2D_UNCERTAINTY_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(UncertaintyRecord) == UNCERTAINTY_RECORD_BYTES
# the planes of flow2d_subset_uncertainty_2d in the order of its arguments; sigma_u and sigma_v are required, the four gradient
# sigmas go all or none
SUBSET_UNCERTAINTY_PLANES = ("sigma_u", "sigma_v", "rho", "sigma_ux", "sigma_uy", "sigma_vx", "sigma_vy", "noise")


class SequenceStepReport(C.Structure):
    """OpticalFlow2D::SequenceStepReport: one step of correlate_subset_sequence -- the refinement's record and the records of the
    prediction passes that ran before it (zero in step 1 and beyond `fill`)."""
    _fields_ = [("subset", SubsetRecord), ("prediction", PredictRecord * SEQUENCE_MAX_FILL)]

    def summary(self, fill=SEQUENCE_MAX_FILL):
        return {"subset": self.subset.summary(), "prediction": [self.prediction[k].summary() for k in range(fill)]}


class SubsetOptions(C.Structure):
    """flow2d_host_subset_options of host/host_c_api.cpp: OpticalFlow2D::SubsetOptions as every host entry that refines takes it.
    mask: a device plane for a *_device entry, a host image otherwise, None for none."""
    _fields_ = [("radius", C.c_int), ("iterations", C.c_int), ("epsilon", C.c_float), ("max_shift", C.c_float),
                ("max_gradient", C.c_float), ("order", C.c_int), ("max_curvature", C.c_float), ("min_pixels", C.c_int),
                ("mask", C.c_void_p)]


class CorrelationPassReport(C.Structure):
    """OpticalFlow2D::CorrelationPassReport: one pass of correlate_multipass -- its grid, the correlation's record and the
    validation's (zero where the pass was not validated)."""
    _fields_ = [("nw", C.c_size_t), ("nh", C.c_size_t), ("correlation", CorrelationPassRecord), ("validation", ValidationRecord)]

    def summary(self):
        return {"nw": self.nw, "nh": self.nh, "correlation": self.correlation.summary(), "validation": self.validation.summary()}
VALIDATE_FLAG, VALIDATE_REPLACE = 0, 1  # FLOW2D_VALIDATE_*
VALIDATE_FLAG_MASKED = 3  # FLOW2D_VALIDATE_FLAG_MASKED: the flag flow2d_validate_nodes_masked_2d gives a node off the specimen


def correlation_min_pixels(radius):
    """The default min_pixels of a masked window search (OpticalFlow2D::ValidationOptions::min_pixels = 0): a quarter of the
    window, rounded up, and six at least."""
    side = 2 * int(radius) + 1
    return max(6, (side * side + 3) // 4)


class PriorReport(C.Structure):
    """OpticalFlow2D::PriorReport: what a pyramid started from a prior flow reports -- the level it started at, the levels it ran
    and the count of prior pixels that were not finite (they entered as zero)."""
    _fields_ = [("start_level", C.c_size_t), ("levels_run", C.c_size_t), ("not_finite", C.c_ulonglong)]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


PROPAGATE_MAX_FILL = 64  # FLOW2D_PROPAGATE_MAX_FILL


class PropagateRecord(C.Structure):
    """flow2d_propagate_record of include/flow2d_c_abi.h: the counts flow2d_propagate_flow_2d writes per instance."""
    _fields_ = [(name, C.c_ulonglong) for name in ("pixels", "unusable", "left", "landed", "holes", "filled", "unfilled", "reserved")]

    def summary(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


PROPAGATE_RECORD_BYTES = 64  # FLOW2D_PROPAGATE_RECORD_BYTES, checked by a static_assert in the header
assert C.sizeof(PropagateRecord) == PROPAGATE_RECORD_BYTES


class WarmOptions(C.Structure):
    """OpticalFlow2D::WarmOptions: the fill passes and the photometric scale of the propagation, and the tail of the adaptive rule
    (< 0: no adaptation)."""
    _fields_ = [("fill_passes", C.c_int), ("photo_scale", C.c_float), ("tail", C.c_float)]


WARM_MODES = ("unseeded", "seeded", "redone")


class WarmReport(C.Structure):
    """OpticalFlow2D::WarmReport: how a pair of a warm-started sequence ran -- mode (0 unseeded, 1 seeded, 2 redone: seeded, then
    computed again unseeded because the prediction did not hold), the reach it was seeded with (adaptive mode; 0 unseeded), the
    PriorReport fields of the seeded run, the propagation's record, and the shares of pixels where the final flow differs from the
    prediction by more than 1, 2, 3 px (adaptive mode; -1: not measured)."""
    _fields_ = [("mode", C.c_int), ("reach", C.c_int), ("start_level", C.c_size_t), ("levels_run", C.c_size_t),
                ("not_finite", C.c_ulonglong), ("propagation", PropagateRecord), ("share", C.c_double * 3)]

    def summary(self):
        return {"mode": WARM_MODES[self.mode], "reach": self.reach, "start_level": self.start_level, "levels_run": self.levels_run,
                "not_finite": self.not_finite, "propagation": self.propagation.summary(), "share": list(self.share)}


def warm_options(fill_passes=4, photo_scale=1.0, tail=None):
    """WarmOptions; tail None: no adaptation.  ValueError for what OpticalFlow2D::WarmOptionsOk refuses.  Needs no device."""
    options = WarmOptions(int(fill_passes), float(photo_scale), -1.0 if tail is None else float(tail))
    if (tail is not None and not 0.0 <= float(tail) < 1.0) or not host_lib().flow2d_host_warm_options_ok(C.byref(options)):
        raise ValueError("warm start: fill_passes %r (0 .. %d), photo_scale %r (finite, >= 0), tail %r (None or in [0, 1))" %
                         (fill_passes, PROPAGATE_MAX_FILL, photo_scale, tail))
    return options


def warm_next_reach(count, above, tail, reach_used):
    """OpticalFlow2D::WarmNextReach, the adaptive rule of a warm sequence: from `count` compared pixels of which above[t - 1] lie
    further than t px (t = 1, 2, 3) from the prediction, returns (redo, next_reach) -- whether a pair seeded with reach_used (0:
    it ran unseeded) is to be computed again unseeded, and the reach of the next pair (0: unseeded).  ValueError for refused
    arguments.  Needs no device."""
    redo, nxt = C.c_int(), C.c_int()
    a = (C.c_ulonglong * 3)(*[int(x) for x in above])
    if host_lib().flow2d_host_warm_next_reach(int(count), a, float(tail), int(reach_used), C.byref(redo), C.byref(nxt)):
        raise ValueError("warm_next_reach(%r, %r, %r, %r)" % (count, list(above), tail, reach_used))
    return bool(redo.value), nxt.value


def prior_start_level(width, height, levels, scale, reach=2.0, level=None):
    """The level at which a pyramid of `levels` levels with scale factor `scale` over a width x height frame starts from a prior
    flow (OpticalFlow2D::PriorStartLevel): the smallest l with reach * scale^l <= 1 in the float arithmetic of the level geometry,
    at most the top level of the unseeded run; `level` (>= 0) replaces the rule and is clamped alike.  ValueError for a reach that
    is not finite and > 0, a negative level, or parameters with which no level runs.  Needs no device."""
    start = C.c_size_t()
    if level is not None and int(level) < 0:
        raise ValueError("prior level %d (>= 0)" % int(level))
    if host_lib().flow2d_host_prior_start_level(width, height, levels, scale, float(reach), -1 if level is None else int(level),
                                                C.byref(start)):
        raise ValueError("no start level for reach %g, level %s, %d levels at scale %g" % (reach, level, levels, scale))
    return start.value


def correlation_grid(width, height, radius, spacing):
    """(nw, nh): the node grid of flow2d_correlate_2d (flow2d_correlation_grid).  Needs no device."""
    nw, nh = C.c_size_t(), C.c_size_t()
    _check(hip_lib().flow2d_correlation_grid(width, height, int(radius), int(spacing), C.byref(nw), C.byref(nh)),
           "flow2d_correlation_grid")
    return nw.value, nh.value


_hip = None


def hip_lib():
    """The C-ABI library.  Raises if it has not been built -- there is no fallback."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP extension is mandatory, there is no CPU path)" % HIP_LIB_PATH)
        L = C.CDLL(HIP_LIB_PATH, mode=C.RTLD_GLOBAL)
        vp, sz, f, i = C.c_void_p, C.c_size_t, C.c_float, C.c_int
        L.flow2d_abi_version.restype = i
        L.flow2d_status_string.restype = C.c_char_p
        L.flow2d_status_string.argtypes = [i]
        L.flow2d_last_error.restype = C.c_char_p
        L.flow2d_device_count.argtypes = [C.POINTER(i)]
        L.flow2d_hw_queues.restype = i
        L.flow2d_request_hw_queues.argtypes = [i]
        # the lanes of the batched path want a hardware queue each; a refusal (HIP already running, e.g. under torch: bench.py
        # exports the variable itself) is reported by flow2d_last_error() and OpticalFlowBatch2D's warning, not here
        L.flow2d_request_hw_queues(8)
        L.flow2d_context_create.argtypes = [i, C.POINTER(vp)]
        L.flow2d_context_create_on_stream.argtypes = [i, vp, C.POINTER(vp)]
        L.flow2d_context_destroy.argtypes = [vp]
        L.flow2d_context_device.argtypes = [vp, C.POINTER(i)]
        L.flow2d_context_stream.argtypes = [vp, C.POINTER(vp)]
        L.flow2d_synchronize.argtypes = [vp]
        L.flow2d_context_set_batch.argtypes = [vp, sz, sz]
        L.flow2d_mem_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
        L.flow2d_device_name.argtypes = [vp, C.c_char_p, sz]
        L.flow2d_plane_pitch_bytes.restype = sz
        L.flow2d_plane_pitch_bytes.argtypes = [sz]
        L.flow2d_plane_alloc.argtypes = [vp, sz, sz, C.POINTER(vp), C.POINTER(sz)]
        L.flow2d_plane_free.argtypes = [vp, vp]
        L.flow2d_memset_2d.argtypes = [vp, vp, sz, i, sz, sz]
        L.flow2d_copy_h2d_2d.argtypes = [vp, vp, sz, vp, sz, sz, sz]
        L.flow2d_copy_d2h_2d.argtypes = [vp, vp, sz, vp, sz, sz, sz]
        L.flow2d_copy_d2d.argtypes = [vp, vp, vp, sz]
        L.flow2d_copy_planes.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(vp), sz, sz, sz]
        L.flow2d_event_create.argtypes = [vp, C.POINTER(vp)]
        L.flow2d_event_record.argtypes = [vp, vp]
        L.flow2d_event_synchronize.argtypes = [vp, vp]
        L.flow2d_event_elapsed_ms.argtypes = [vp, vp, vp, C.POINTER(f)]
        L.flow2d_event_destroy.argtypes = [vp, vp]
        L.flow2d_stream_wait_event.argtypes = [vp, vp]
        L.flow2d_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
        L.flow2d_host_free.argtypes = [vp, vp]
        L.flow2d_add_2d.argtypes = [vp, vp, vp, sz, sz, sz]
        L.flow2d_gaussian_kernel.argtypes = [f, C.POINTER(f), C.POINTER(i)]
        L.flow2d_convolution_rows.argtypes = [vp, vp, vp, sz, sz, sz, C.POINTER(f), i]
        L.flow2d_convolution_columns.argtypes = [vp, vp, vp, sz, sz, sz, C.POINTER(f), i]
        L.flow2d_gaussian_blur.argtypes = [vp, vp, vp, sz, sz, sz, C.POINTER(f), i]
        L.flow2d_median_2d.argtypes = [vp, vp, sz, sz, sz, sz, vp]
        L.flow2d_registration_2d.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, f, f, vp]
        L.flow2d_upsample_registration_2d.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, sz, sz, f, f, vp]
        L.flow2d_resample_x.argtypes = [vp, vp, vp, sz, sz, sz, sz]
        L.flow2d_resample_y.argtypes = [vp, vp, vp, sz, sz, sz, sz]
        L.flow2d_add_2d_pair.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz]
        L.flow2d_median_2d_pair.argtypes = [vp, vp, vp, sz, sz, sz, sz, vp, vp]
        L.flow2d_add_median_2d_pair.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, vp, vp]
        L.flow2d_add_median_2d_pair_half.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, vp, vp]
        L.flow2d_upsample_registration_half_2d.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, sz, sz, f, f, vp]
        L.flow2d_solve_level_takes_half_base.argtypes = [vp, C.POINTER(SolveParams)]
        L.flow2d_half_base_flow_launches.argtypes = []
        L.flow2d_half_base_flow_launches.restype = C.c_ulonglong
        L.flow2d_fused_packed_launches.argtypes = []
        L.flow2d_fused_packed_launches.restype = C.c_ulonglong
        L.flow2d_resample_x_pair.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz]
        L.flow2d_resample_y_pair.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz]
        L.flow2d_resample_xy_pair.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, sz]
        L.flow2d_resample_x_levels.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]
        L.flow2d_compute_phi_ksi.argtypes = [vp] * 7 + [sz, sz, sz, f, f, f, f, vp, vp]
        L.flow2d_solve_2d.argtypes = [vp] * 9 + [sz, sz, sz, f, f, f, vp, vp]
        L.flow2d_solve_2d_grad.argtypes = [vp] * 9 + [sz, sz, sz, f, f, f, vp, vp]
        L.flow2d_solve_2d_grad_untiled.argtypes = [vp] * 9 + [sz, sz, sz, f, f, f, vp, vp]
        L.flow2d_solve_2d_log.argtypes = [vp] * 9 + [sz, sz, sz, f, f, f, vp, vp]
        L.flow2d_log_frame_2d.argtypes = [vp, vp, vp, sz, sz, sz]
        L.flow2d_solver_algorithm_for.argtypes = [i, sz, sz, sz, sz, sz, i]
        L.flow2d_solve_2d_sor.argtypes = [vp] * 9 + [sz, sz, sz, f, f, f, f, i]
        L.flow2d_solve_level.argtypes = [vp] * 11 + [C.POINTER(SolveParams), C.POINTER(i)]
        L.flow2d_timing_enable.argtypes = [vp, i]
        L.flow2d_fused_fallbacks.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.flow2d_context_set_lone.argtypes = [vp, i]
        if hasattr(L, "flow2d_context_set_planning_cus"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_context_set_planning_cus.argtypes = [vp, i]
            L.flow2d_context_planning_cus.argtypes = [vp, C.POINTER(i)]
            L.flow2d_fused_block_order_for_cus.argtypes = [i, sz, sz, sz, sz, C.POINTER(i), sz, C.POINTER(sz)]
            L.flow2d_fused_plan_for_cus.argtypes = [i, sz, sz, sz, sz, C.POINTER(i), C.POINTER(i)]
            L.flow2d_stream_rows_for_cus.argtypes = [i, i, sz, sz, i, sz]
        L.flow2d_resample_y_levels.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
        L.flow2d_resample_xy_levels.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
        L.flow2d_resample_xy_levels_launches.argtypes = []
        L.flow2d_resample_xy_levels_launches.restype = C.c_ulonglong
        L.flow2d_clock_probe_start.argtypes = [vp, C.c_double]
        L.flow2d_clock_probe_read.argtypes = [vp, C.POINTER(C.c_double)]
        L.flow2d_fused_block_order.argtypes = [vp, sz, sz, sz, sz, C.POINTER(i), sz, C.POINTER(sz)]
        if hasattr(L, "flow2d_fused_plain_waves"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_fused_plain_waves.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.flow2d_timing_launch_filter.argtypes = [vp, sz, sz]
        if hasattr(L, "flow2d_consistency_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_consistency_2d.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, f, f, vp]
        if hasattr(L, "flow2d_interpolate_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_interpolate_2d.argtypes = [vp] * 9 + [sz, sz, sz, f, i, f, vp]
        if hasattr(L, "flow2d_track_points_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_track_points_2d.argtypes = [vp] * 5 + [sz, sz, sz, vp, vp, vp, sz, f, f, i, f, f, vp, vp, vp]
            L.flow2d_seed_points_workspace_bytes.restype = sz
            L.flow2d_seed_points_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_seed_points_2d.argtypes = [vp, vp, sz, sz, sz, sz, f, vp, vp, vp, sz, vp, vp, sz]
        if hasattr(L, "flow2d_denoise_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_denoise_2d.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), sz, sz, sz, f,
                                            vp, vp]
            L.flow2d_compose_flow_2d.argtypes = [vp] * 7 + [sz, sz, sz, vp, vp, vp]
        if hasattr(L, "flow2d_global_motion_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            d = C.c_double
            L.flow2d_global_motion_workspace_bytes.restype = sz
            L.flow2d_global_motion_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_global_motion_2d.argtypes = [vp, vp, vp, vp, sz, sz, sz, i, d, i, vp, vp, sz]
            L.flow2d_global_flow_2d.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, d, vp, vp, vp, vp, vp]
            L.flow2d_warp_global_2d.argtypes = [vp, vp, vp, sz, sz, sz, f, vp, vp]
        if hasattr(L, "flow2d_deformation_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_deformation_workspace_bytes.restype = sz
            L.flow2d_deformation_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_deformation_2d.argtypes = [vp, vp, vp, vp, sz, sz, sz, i, C.POINTER(DeformationPlanes), vp, vp, sz]
        if hasattr(L, "flow2d_refine_flow_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_refine_flow_2d.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, i, f, f, vp, vp, vp]
        if hasattr(L, "flow2d_correlate_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_correlation_grid.argtypes = [sz, sz, i, i, C.POINTER(sz), C.POINTER(sz)]
            L.flow2d_correlate_2d.argtypes = [vp, vp, vp, sz, sz, sz, f, f, i, i, i, f, vp, vp, vp, sz, vp]
            L.flow2d_expand_nodes_2d.argtypes = [vp, vp, vp, sz, sz, sz, i, i, vp, vp, sz, sz, sz]
        if hasattr(L, "flow2d_correlate_offset_2d"):
            L.flow2d_correlate_offset_2d.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, f, f, i, i, i, f, vp, vp, vp, sz, vp]
            L.flow2d_validate_nodes_2d.argtypes = [vp, vp, vp, sz, sz, sz, f, f, i, i, vp, vp, vp, vp]
        if hasattr(L, "flow2d_correlate_masked_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_correlate_masked_2d.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, f, f, i, i, i, f, vp, i, vp, vp, vp, sz, vp]
            L.flow2d_validate_nodes_masked_2d.argtypes = [vp, vp, vp, sz, sz, sz, f, f, i, i, vp, sz, sz, sz, i, i, vp, vp, vp, vp]
        if hasattr(L, "flow2d_subset_refine_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_subset_refine_2d.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, sz, sz, sz, i, i, i, i, f, f, f] + [vp] * 9
        if hasattr(L, "flow2d_subset_refine2_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_subset_refine2_2d.argtypes = [vp, vp, vp, sz, sz, sz] + [vp] * 4 + [sz, sz, sz, i, i, i, i, f, f, f, f] + [vp] * 7
        if hasattr(L, "flow2d_subset_refine_from_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_subset_refine_from_2d.argtypes = [vp, vp, vp, sz, sz, sz] + [vp] * 6 + [sz, sz, sz, i, i, i, i, f, f, f] + [vp] * 9
            L.flow2d_predict_nodes_2d.argtypes = [vp] + [vp] * 7 + [sz, sz, sz, i, i, i] + [vp] * 8
        if hasattr(L, "flow2d_subset_refine_masked_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_subset_refine_masked_2d.argtypes = [vp, vp, vp, sz, sz, sz] + [vp] * 6 + [sz, sz, sz, i, i, i, i, f, f, f, vp, i] + [vp] * 9
        if hasattr(L, "flow2d_bspline_prefilter_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_bspline_prefilter_2d.argtypes = [vp, vp, vp, sz, sz, sz]
            L.flow2d_subset_refine_spline_2d.argtypes = L.flow2d_subset_refine_masked_2d.argtypes
            L.flow2d_subset_refine2_spline_2d.argtypes = L.flow2d_subset_refine2_2d.argtypes
        if hasattr(L, "flow2d_node_strain_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_node_strain_workspace_bytes.restype = sz
            L.flow2d_node_strain_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_node_strain_2d.argtypes = [vp] + [vp] * 7 + [sz, sz, sz, i, i, i, i, i, i, C.POINTER(DeformationPlanes), vp, vp, sz]
        if hasattr(L, "flow2d_node_strain_robust_2d"):
            L.flow2d_node_strain_robust_workspace_bytes.restype = sz
            L.flow2d_node_strain_robust_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_node_strain_robust_2d.argtypes = [vp] + [vp] * 3 + [sz, sz, sz, i, i, i, i, i, i, C.c_float, i,
                                                                        C.POINTER(DeformationPlanes), C.POINTER(NodeStrainDiagnostics), vp, vp, sz]
        if hasattr(L, "flow2d_node_strain_weighted_2d"):
            L.flow2d_node_strain_weighted_workspace_bytes.restype = sz
            L.flow2d_node_strain_weighted_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_node_strain_weighted_2d.argtypes = [vp] + [vp] * 5 + [sz, sz, sz, i, i, i, i, i, i, C.c_float, C.c_float, i,
                                                                          C.POINTER(DeformationPlanes), C.POINTER(NodeStrainDiagnostics),
                                                                          C.POINTER(StrainSigmaPlanes), vp, vp, sz]
        if hasattr(L, "flow2d_subset_uncertainty_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_subset_uncertainty_2d.argtypes = [vp, vp, vp, i, sz, sz, sz] + [vp] * 7 + [sz, sz, sz, i, i, i, i, vp, i] + [vp] * 9
        if hasattr(L, "flow2d_compose_nodes_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_compose_nodes_2d.argtypes = [vp, vp, vp, vp, sz, sz, sz, i, i, i, vp, vp, vp, vp]
        if hasattr(L, "flow2d_prior_registration_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_prior_registration_2d.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, sz, sz, f, f, vp, vp]
        if hasattr(L, "flow2d_propagate_flow_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_propagate_flow_workspace_bytes.restype = sz
            L.flow2d_propagate_flow_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_propagate_flow_2d.argtypes = [vp] * 6 + [sz, sz, sz, f, f, i, vp, vp, vp, vp]
        if hasattr(L, "flow2d_segment_motion_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_segment_motion_workspace_bytes.restype = sz
            L.flow2d_segment_motion_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_segment_motion_2d.argtypes = [vp, vp, vp, vp, sz, sz, sz, f, f, C.c_uint, vp, vp, sz, vp, vp, sz]
        if hasattr(L, "flow2d_flow_error_2d"):  # (absent from libraries of earlier rounds loaded for an A/B)
            L.flow2d_flow_error_workspace_bytes.restype = sz
            L.flow2d_flow_error_workspace_bytes.argtypes = [sz, sz, sz]
            L.flow2d_flow_error_2d.argtypes = [vp] * 6 + [sz, sz, sz, vp, vp, vp, vp, sz]
        L.flow2d_timing_count.argtypes = [vp, C.POINTER(sz)]
        L.flow2d_timing_get.argtypes = [vp, sz, C.POINTER(TimingRecord)]
        L.flow2d_timing_reset.argtypes = [vp]
        _hip = L
    return _hip


def _check(status, where):
    if status != 0:
        raise Flow2DError(status, where, hip_lib().flow2d_last_error().decode(errors="replace"))


def half_base_flow_launches():
    """launches of the half-size up-sample + warp queued by this process so far (flow2d_half_base_flow_launches)"""
    return int(hip_lib().flow2d_half_base_flow_launches())


def fused_packed_launches():
    """strip launches of this process so far that the packed build of the strip kernel served (flow2d_fused_packed_launches)"""
    return int(hip_lib().flow2d_fused_packed_launches())


STREAM_GAUSSIAN, STREAM_MEDIAN = 0, 1


def fused_block_order_for_cus(cus, width, height, inner, instances=1):
    """Context.fused_block_order for a device of `cus` compute units; needs neither a context nor a device
    (flow2d_fused_block_order_for_cus)."""
    grid = C.c_size_t(0)
    cap = 1 << 17
    buf = (C.c_int * (4 * cap))()
    _check(hip_lib().flow2d_fused_block_order_for_cus(cus, width, height, inner, instances, buf, cap, C.byref(grid)),
           "flow2d_fused_block_order_for_cus")
    return np.frombuffer(buf, np.int32, 4 * grid.value).reshape(-1, 4).copy()


class FusedPlan(collections.namedtuple("FusedPlan", "rows_interior rows_edge strips_interior blocks_x blocks side_blocks")):
    """The strip plan of a level (flow2d_fused_plan_for_cus).  side_blocks: the first and last block column's blocks when the
    launch order deals them over the eight runs, 0 when it does not (or the plan is uniform)."""

    @property
    def uniform(self):
        return self.rows_interior == self.rows_edge


def fused_plan_for_cus(cus, width, height, inner, instances=1):
    """The strip plan a device of `cus` compute units gives a level; needs neither a context nor a device."""
    plan, side = (C.c_int * 5)(), C.c_int(0)
    _check(hip_lib().flow2d_fused_plan_for_cus(cus, width, height, inner, instances, plan, C.byref(side)), "flow2d_fused_plan_for_cus")
    return FusedPlan(*plan, side.value)


def stream_rows_for_cus(cus, kind, width, height, radius, instances=1):
    """Rows per strip of a streaming Gaussian (STREAM_GAUSSIAN, radius 1 ... 6) or median (STREAM_MEDIAN, radius 1 ... 3) launch
    on a device of `cus` compute units (flow2d_stream_rows_for_cus); needs neither a context nor a device."""
    rows = hip_lib().flow2d_stream_rows_for_cus(cus, kind, width, height, radius, instances)
    if rows < 0:
        raise ValueError("flow2d_stream_rows_for_cus(%r, %r, %r, %r, %r, %r)" % (cus, kind, width, height, radius, instances))
    return rows


def resample_xy_levels_launches():
    """launches of the one-launch frame pyramid queued by this process so far (flow2d_resample_xy_levels_launches)"""
    return int(hip_lib().flow2d_resample_xy_levels_launches())


def device_count():
    n = C.c_int(0)
    st = hip_lib().flow2d_device_count(C.byref(n))
    return n.value if st == 0 else 0


def gaussian_kernel(sigma):
    taps = (C.c_float * 51)()
    r = C.c_int(0)
    _check(hip_lib().flow2d_gaussian_kernel(sigma, taps, C.byref(r)), "flow2d_gaussian_kernel")
    return np.array(taps[: 2 * r.value + 1], np.float32), r.value


class Plane:
    """A pitched fp32 container in HBM (reference: one of the 12 cuMemAllocPitch planes)."""

    def __init__(self, ctx, width, height):
        self.ctx = ctx
        self.width, self.height = width, height
        ptr, pitch = C.c_void_p(), C.c_size_t()
        _check(hip_lib().flow2d_plane_alloc(ctx.handle, width, height, C.byref(ptr), C.byref(pitch)),
               "flow2d_plane_alloc")
        self.ptr, self.pitch = ptr.value, pitch.value

    def upload(self, array):
        a = np.ascontiguousarray(array, np.float32)
        h, w = a.shape
        assert w <= self.width and h <= self.height
        _check(hip_lib().flow2d_copy_h2d_2d(self.ctx.handle, self.ptr, self.pitch, a.ctypes.data, w * 4, w * 4, h),
               "flow2d_copy_h2d_2d")
        self.ctx.synchronize()
        return self

    def download(self, width=None, height=None):
        w = self.width if width is None else width
        h = self.height if height is None else height
        out = np.empty((h, w), np.float32)
        _check(hip_lib().flow2d_copy_d2h_2d(self.ctx.handle, out.ctypes.data, w * 4, self.ptr, self.pitch, w * 4, h),
               "flow2d_copy_d2h_2d")
        self.ctx.synchronize()
        return out

    def fill_bytes(self, value=0):
        _check(hip_lib().flow2d_memset_2d(self.ctx.handle, self.ptr, self.pitch, value, self.width * 4, self.height),
               "flow2d_memset_2d")
        return self

    def free(self):
        if self.ptr:
            hip_lib().flow2d_plane_free(self.ctx.handle, self.ptr)
            self.ptr = None


class _BatchScope:
    """What Context.set_batch returns: leaving the `with` block switches the lock-step batch off again."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        _check(hip_lib().flow2d_context_set_batch(self.ctx.handle, 1, 0), "flow2d_context_set_batch")


class Context:
    """One device + stream (reference: the CUcontext of main.cpp:51 plus the NULL stream)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        if stream is None:
            _check(hip_lib().flow2d_context_create(device, C.byref(h)), "flow2d_context_create")
        else:
            _check(hip_lib().flow2d_context_create_on_stream(device, stream, C.byref(h)),
                   "flow2d_context_create_on_stream")
        self.handle = h
        self._planes = []

    # -- memory ---------------------------------------------------------------------------------
    def plane(self, width, height, data=None):
        p = Plane(self, width, height)
        self._planes.append(p)
        if data is not None:
            p.fill_bytes(0)
            p.upload(data)
        return p

    def _record_plane(self, bytes_per_record, instances, least=0):
        """A Plane of `instances` records of `bytes_per_record` bytes, `least` floats wide at least."""
        return self.plane(max(instances * bytes_per_record // 4, least), 1)

    def _read_records(self, record, instances, kind):
        """The first `instances` records of a record Plane as a list of `kind` (synchronises)."""
        raw = record.download(instances * C.sizeof(kind) // 4, 1)
        return list((kind * instances).from_buffer_copy(raw.tobytes()))

    def copy_planes(self, srcs, dsts, width, height):
        """flow2d_copy_planes: the planes srcs[i] -> dsts[i] (same pitch) with one launch."""
        n = len(srcs)
        a, b = (C.c_void_p * n)(*[p.ptr for p in srcs]), (C.c_void_p * n)(*[p.ptr for p in dsts])
        _check(hip_lib().flow2d_copy_planes(self.handle, n, a, b, srcs[0].pitch, width, height), "flow2d_copy_planes")

    def synchronize(self):
        _check(hip_lib().flow2d_synchronize(self.handle), "flow2d_synchronize")

    def mem_info(self):
        a, b = C.c_size_t(), C.c_size_t()
        _check(hip_lib().flow2d_mem_info(self.handle, C.byref(a), C.byref(b)), "flow2d_mem_info")
        return a.value, b.value

    def fused_fallbacks(self):
        """Waves of the fused kernel that repeated their strip with the plain division (synchronises)."""
        n = C.c_ulonglong()
        _check(hip_lib().flow2d_fused_fallbacks(self.handle, C.byref(n)), "flow2d_fused_fallbacks")
        return n.value

    def set_lone(self, lone):
        """flow2d_context_set_lone: this context's launches run alone on the device (packed strip build for under-filled launches)"""
        _check(hip_lib().flow2d_context_set_lone(self.handle, int(bool(lone))), "flow2d_context_set_lone")

    def set_planning_cus(self, cus):
        """flow2d_context_set_planning_cus: the launch planners of this context plan for `cus` compute units from now on (0: the
        device's own count again).  A hint: the same bytes whatever the value, only the launch geometry changes."""
        _check(hip_lib().flow2d_context_set_planning_cus(self.handle, int(cus)), "flow2d_context_set_planning_cus")

    def planning_cus(self):
        """The compute units this context's launch planners plan for (flow2d_context_planning_cus)."""
        n = C.c_int(0)
        _check(hip_lib().flow2d_context_planning_cus(self.handle, C.byref(n)), "flow2d_context_planning_cus")
        return n.value

    def set_batch(self, count, stride_bytes=0):
        """flow2d_context_set_batch: from now on every batch-aware launcher of this context acts on `count` instances of its
        planes, `stride_bytes` apart (count = 1: off).  The switch is made at once; the value returned is a context manager
        that goes back to count = 1 on exit:  `with ctx.set_batch(3, stride): ...`."""
        _check(hip_lib().flow2d_context_set_batch(self.handle, count, stride_bytes), "flow2d_context_set_batch")
        return _BatchScope(self)

    def resample_y_levels(self, packed_a, out_a, in_height, widths, heights, columns, rows, packed_b=None, out_b=None):
        """the y passes of several pyramid levels in one launch (flow2d_resample_y_levels)"""
        n = len(widths)
        arr = lambda v: (C.c_size_t * n)(*v)
        _check(hip_lib().flow2d_resample_y_levels(self.handle, packed_a.ptr, out_a.ptr, packed_b.ptr if packed_b else None,
                                                  out_b.ptr if out_b else None, in_height, packed_a.pitch, n, arr(widths), arr(heights),
                                                  arr(columns), arr(rows)), "flow2d_resample_y_levels")

    def resample_xy_levels(self, src_a, out_a, in_width, in_height, widths, heights, rows, columns=None, src_b=None, out_b=None,
                           pitch=None):
        """the x and y passes of all levels of a halving pyramid in one launch (flow2d_resample_xy_levels).  Planes, or raw device
        addresses together with `pitch` (bytes)."""
        n = len(widths)
        arr = lambda v: (C.c_size_t * n)(*v)
        ptr = lambda p: None if p is None else (p if isinstance(p, int) else p.ptr)
        _check(hip_lib().flow2d_resample_xy_levels(self.handle, ptr(src_a), ptr(out_a), ptr(src_b), ptr(out_b), in_width, in_height,
                                                   src_a.pitch if pitch is None else pitch, n, arr(widths), arr(heights), arr(rows),
                                                   arr(columns) if columns is not None else None), "flow2d_resample_xy_levels")

    def clock_probe_start(self, duration_us):
        """queues one sleeping wave per XCD on this context's stream that brackets duration_us with the 100 MHz and the shader clock"""
        _check(hip_lib().flow2d_clock_probe_start(self.handle, float(duration_us)), "flow2d_clock_probe_start")

    def clock_probe_read(self):
        """waits for the probe; the shader clock held per XCD in GHz (0: no wave landed there)"""
        ghz = (C.c_double * 8)()
        _check(hip_lib().flow2d_clock_probe_read(self.handle, ghz), "flow2d_clock_probe_read")
        return list(ghz)

    def fused_block_order(self, width, height, inner, instances=1):
        """(grid, 4) int array: block column, strip, first row, end row of every launch block of a strip launch (-1: empty id)."""
        grid = C.c_size_t(0)
        cap = 1 << 16
        buf = (C.c_int * (4 * cap))()
        _check(hip_lib().flow2d_fused_block_order(self.handle, width, height, inner, instances, buf, cap, C.byref(grid)),
               "flow2d_fused_block_order")
        return np.frombuffer(buf, np.int32, 4 * grid.value).reshape(-1, 4).copy()

    def fused_plain_waves(self):
        """Waves of fused launches that ran the plain expressions throughout (grid spacing outside the proven range)."""
        n = C.c_ulonglong()
        _check(hip_lib().flow2d_fused_plain_waves(self.handle, C.byref(n)), "flow2d_fused_plain_waves")
        return n.value

    def device_name(self):
        buf = C.create_string_buffer(256)
        _check(hip_lib().flow2d_device_name(self.handle, buf, 256), "flow2d_device_name")
        return buf.value.decode()

    def close(self):
        if self.handle:
            for p in self._planes:
                p.free()
            self._planes = []
            hip_lib().flow2d_context_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- events ---------------------------------------------------------------------------------
    def event(self):
        e = C.c_void_p()
        _check(hip_lib().flow2d_event_create(self.handle, C.byref(e)), "flow2d_event_create")
        return e

    def record(self, ev):
        _check(hip_lib().flow2d_event_record(self.handle, ev), "flow2d_event_record")

    def wait_event(self, ev):
        """Host wait until everything recorded before `ev` on this context's stream has finished."""
        _check(hip_lib().flow2d_event_synchronize(self.handle, ev), "flow2d_event_synchronize")

    def elapsed_ms(self, start, stop):
        _check(hip_lib().flow2d_event_synchronize(self.handle, stop), "flow2d_event_synchronize")
        ms = C.c_float()
        _check(hip_lib().flow2d_event_elapsed_ms(self.handle, start, stop, C.byref(ms)), "flow2d_event_elapsed_ms")
        return ms.value

    # -- kernels (thin 1:1 wrappers of the C-ABI launchers) --------------------------------------
    def add(self, op0, op1, w, h):
        _check(hip_lib().flow2d_add_2d(self.handle, op0.ptr, op1.ptr, w, h, op0.pitch), "flow2d_add_2d")

    def convolution_rows(self, dst, src, w, h, taps, radius):
        t = np.ascontiguousarray(taps, np.float32)
        _check(hip_lib().flow2d_convolution_rows(self.handle, dst.ptr, src.ptr, w, h, src.pitch,
                                                 t.ctypes.data_as(C.POINTER(C.c_float)), radius),
               "flow2d_convolution_rows")

    def convolution_columns(self, dst, src, w, h, taps, radius):
        t = np.ascontiguousarray(taps, np.float32)
        _check(hip_lib().flow2d_convolution_columns(self.handle, dst.ptr, src.ptr, w, h, src.pitch,
                                                    t.ctypes.data_as(C.POINTER(C.c_float)), radius),
               "flow2d_convolution_columns")

    def gaussian_blur(self, dst, src, w, h, taps, radius):
        t = np.ascontiguousarray(taps, np.float32)
        _check(hip_lib().flow2d_gaussian_blur(self.handle, dst.ptr, src.ptr, w, h, src.pitch,
                                              t.ctypes.data_as(C.POINTER(C.c_float)), radius), "flow2d_gaussian_blur")

    def median(self, src, w, h, window, dst):
        _check(hip_lib().flow2d_median_2d(self.handle, src.ptr, w, h, src.pitch, window, dst.ptr), "flow2d_median_2d")

    def registration(self, f0, f1, u, v, w, h, hx, hy, out):
        _check(hip_lib().flow2d_registration_2d(self.handle, f0.ptr, f1.ptr, u.ptr, v.ptr, w, h, f0.pitch, hx, hy,
                                                out.ptr), "flow2d_registration_2d")

    def consistency(self, u, v, bu, bv, w, h, out, alpha1=0.01, alpha2=0.5):
        """Forward-backward consistency mask of the flow (u, v) against the backward flow (bu, bv) into `out`: 1.0 where the
        pair is inconsistent (occluded, leaving the frame, NaN), 0.0 elsewhere (flow2d_consistency_2d)."""
        _check(hip_lib().flow2d_consistency_2d(self.handle, u.ptr, v.ptr, bu.ptr, bv.ptr, w, h, u.pitch, alpha1, alpha2,
                                               out.ptr), "flow2d_consistency_2d")

    def interpolate(self, f0, f1, u, v, bu, bv, w, h, t, out, occ_0=None, occ_1=None, iterations=2, max_residual=0.5):
        """The frame at time t (0 <= t <= 1) between f0 and f1 into `out`, from the flow (u, v) of f0 -> f1, the flow (bu, bv) of
        f1 -> f0 and, when given, the occlusion masks occ_0 / occ_1 of the two frames (flow2d_interpolate_2d)."""
        _check(hip_lib().flow2d_interpolate_2d(self.handle, f0.ptr, f1.ptr, u.ptr, v.ptr, bu.ptr, bv.ptr,
                                               occ_0.ptr if occ_0 else None, occ_1.ptr if occ_1 else None, w, h, u.pitch, t,
                                               iterations, max_residual, out.ptr), "flow2d_interpolate_2d")

    def denoise(self, centre, frames, us, vs, w, h, out, occs=None, range_sigma=0.0, weight_sum=None):
        """`centre` fused with the neighbour frames `frames` into `out` (flow2d_denoise_2d): (us[n], vs[n]) is the flow from the
        centre to frames[n] on the centre's grid, occs[n] (the list, or any entry, may be None) its occlusion mask; range_sigma
        (grey levels, 0 = off) the scale of the photometric weight; `weight_sum` an optional Plane for the sum of weights."""
        n = len(frames)
        arr = lambda q: (C.c_void_p * max(n, 1))(*[p.ptr if p is not None else None for p in q])  # noqa: E731
        _check(hip_lib().flow2d_denoise_2d(self.handle, centre.ptr, n, arr(frames), arr(us), arr(vs),
                                           None if occs is None else arr(occs), w, h, centre.pitch, range_sigma, out.ptr,
                                           weight_sum.ptr if weight_sum else None), "flow2d_denoise_2d")

    def compose_flow(self, ab_u, ab_v, bc_u, bc_v, w, h, out_u, out_v, mask_ab=None, mask_bc=None, out_mask=None):
        """The flow a -> c on a's grid into (out_u, out_v) from the flows a -> b and b -> c (flow2d_compose_flow_2d): NaN where
        a -> b leaves the frame.  With out_mask, the union of mask_ab, mask_bc carried along a -> b and the pixels that leave."""
        _check(hip_lib().flow2d_compose_flow_2d(self.handle, ab_u.ptr, ab_v.ptr, bc_u.ptr, bc_v.ptr,
                                                mask_ab.ptr if mask_ab else None, mask_bc.ptr if mask_bc else None, w, h,
                                                ab_u.pitch, out_u.ptr, out_v.ptr, out_mask.ptr if out_mask else None),
               "flow2d_compose_flow_2d")

    def track_points(self, u, v, bu, bv, w, h, x, y, count, capacity, out_x, out_y, reason=None, alpha1=0.01, alpha2=0.5,
                     boundaries=True, beta1=0.01, beta2=0.002):
        """One step of the track table (x, y) along the flow (u, v) into (out_x, out_y) (flow2d_track_points_2d).  Tables are
        Planes of height 1 and width >= capacity; `count` is a device counter (see counter()); (bu, bv) the backward flow, or
        both None for no forward-backward check; `reason` an optional Plane whose first `capacity` bytes get the reason codes
        (TRACK_ALIVE ... TRACK_OCCLUDED)."""
        _check(hip_lib().flow2d_track_points_2d(self.handle, u.ptr, v.ptr, bu.ptr if bu else None, bv.ptr if bv else None, w, h,
                                                u.pitch, x.ptr, y.ptr, count.ptr, capacity, alpha1, alpha2, int(bool(boundaries)),
                                                beta1, beta2, out_x.ptr, out_y.ptr, reason.ptr if reason else None),
               "flow2d_track_points_2d")

    def seed_points(self, frame, w, h, spacing, x, y, count, capacity, min_eigenvalue=0.0, dropped=None):
        """Append tracks in the uncovered, textured cells of `frame` to the table (x, y) (flow2d_seed_points_2d): `count` (a
        device counter) grows by the seeds written, `dropped` (a counter, optional) gets the cells that did not fit.  The
        workspace is the context's own (kept between calls)."""
        L = hip_lib()
        need = L.flow2d_seed_points_workspace_bytes(w, h, spacing)
        cached = getattr(self, "_seed_workspace", None)
        if cached is None or cached[0] < need:
            if cached is not None:
                cached[1].free()
                self._planes.remove(cached[1])
            self._seed_workspace = cached = (need, self.plane(max((need + 3) // 4, 4), 1))
        _check(L.flow2d_seed_points_2d(self.handle, frame.ptr, w, h, frame.pitch, spacing, min_eigenvalue, x.ptr, y.ptr,
                                       count.ptr, capacity, dropped.ptr if dropped else None, cached[1].ptr, cached[0]),
               "flow2d_seed_points_2d")

    def counter(self, value=0):
        """A device counter (one unsigned 64-bit integer, in a Plane) holding `value`: the `count` / `dropped` of the tracking
        entries."""
        p = self.plane(4, 1)
        p.upload(np.frombuffer(np.array([value, 0], np.uint64).tobytes(), np.float32).reshape(1, 4))
        return p

    def read_count(self, counter):
        """The value of a device counter (synchronises)."""
        return int(counter.download(4, 1).view(np.uint64)[0, 0])

    def flow_error(self, u, v, gt_u, gt_v, w, h, occlusion=None, epe=None, ae=None, instances=1):
        """Error of the flow (u, v) against ground truth (gt_u, gt_v), all planes of one pitch (flow2d_flow_error_2d): returns
        one record per lock-step instance (`instances` = the count of flow2d_context_set_batch) as dicts (see _stats_dict);
        `occlusion` (non-zero or NaN = occluded) splits noc / occ; `epe` / `ae` planes get the per-pixel errors.  The device
        planes stay where they are: only the records are downloaded (synchronises)."""
        L = hip_lib()
        need = L.flow2d_flow_error_workspace_bytes(w, h, instances)
        cached = getattr(self, "_flow_error_buffers", None)
        if cached is None or cached[0] < need or cached[1] < instances:
            if cached is not None:
                for q in cached[2:]:
                    q.free()
                    self._planes.remove(q)
            self._flow_error_buffers = cached = (need, instances, self.plane(max(need // 4, 4), 1),
                                                 self.plane(instances * FLOW_ERROR_STATS_BYTES // 4, 1))
        ws, stats = cached[2], cached[3]
        _check(L.flow2d_flow_error_2d(self.handle, u.ptr, v.ptr, gt_u.ptr, gt_v.ptr, occlusion.ptr if occlusion else None, w, h,
                                      u.pitch, epe.ptr if epe else None, ae.ptr if ae else None, stats.ptr, ws.ptr, cached[0]),
               "flow2d_flow_error_2d")
        raw = stats.download(instances * FLOW_ERROR_STATS_BYTES // 4, 1)
        recs = (FlowErrorStats * instances).from_buffer_copy(raw.tobytes())
        return [_stats_dict(r) for r in recs]

    def motion_records(self, instances=1):
        """A Plane for `instances` flow2d_global_motion records (device memory; read_motion / upload_motion move them)."""
        return self._record_plane(GLOBAL_MOTION_BYTES, instances)

    def read_motion(self, motion, instances=1):
        """The records of a motion_records Plane as GlobalMotion structures (synchronises)."""
        return self._read_records(motion, instances, GlobalMotion)

    def upload_motion(self, records, motion=None):
        """GlobalMotion structures into a motion_records Plane (a new one unless given), byte for byte."""
        records = list(records)
        motion = motion or self.motion_records(len(records))
        raw = b"".join(bytes(r) for r in records)
        return motion.upload(np.frombuffer(raw, np.float32).reshape(1, -1))

    def global_motion(self, u, v, w, h, model=MOTION_AFFINE, sigma=0.0, iterations=0, mask=None, instances=1, motion=None):
        """The global motion of the flow (u, v) (flow2d_global_motion_2d): `model` fitted by least squares and, with sigma > 0
        (pixels), `iterations` reweighted passes; `mask` (1 = leave out) optional; `instances` = the count of
        flow2d_context_set_batch.  With `motion` (a motion_records Plane) the records stay on the device and nothing is
        returned or synchronised; without, the context's own records are downloaded and returned as GlobalMotion structures.
        The workspace is the context's own (kept between calls)."""
        L = hip_lib()
        need = L.flow2d_global_motion_workspace_bytes(w, h, instances)
        cached = getattr(self, "_global_motion_buffers", None)
        if cached is None or cached[0] < need or cached[1] < instances:
            if cached is not None:
                for q in cached[2:]:
                    q.free()
                    self._planes.remove(q)
            self._global_motion_buffers = cached = (need, instances, self.plane(max(need // 4, 4), 1),
                                                    self.motion_records(instances))
        records = motion or cached[3]
        _check(L.flow2d_global_motion_2d(self.handle, u.ptr, v.ptr, mask.ptr if mask else None, w, h, u.pitch, int(model),
                                         float(sigma), int(iterations), records.ptr, cached[2].ptr, cached[0]),
               "flow2d_global_motion_2d")
        return None if motion else self.read_motion(records, instances)

    def global_flow(self, motion, w, h, u=None, v=None, mask=None, sigma=0.0, model_u=None, model_v=None, residual_u=None,
                    residual_v=None, weight=None):
        """The model of the records `motion` (a motion_records Plane) as planes (model_u, model_v), the flow (u, v) without it
        (residual_u, residual_v; NaN where the flow is not valid) and the inlier map of a reweighted pass with `sigma` and
        `mask` (weight): every output optional, one at least (flow2d_global_flow_2d)."""
        ptr = lambda q: q.ptr if q else None  # noqa: E731
        pitch = next(q.pitch for q in (u, model_u, residual_u, weight) if q)
        _check(hip_lib().flow2d_global_flow_2d(self.handle, motion.ptr, ptr(u), ptr(v), ptr(mask), w, h, pitch, float(sigma),
                                               ptr(model_u), ptr(model_v), ptr(residual_u), ptr(residual_v), ptr(weight)),
               "flow2d_global_flow_2d")

    def warp_global(self, motion, frame, w, h, out, valid=None, fill=0.0):
        """`frame` resampled along the global motion of the records `motion` into `out`: out(x) = frame(x + model(x)), `fill`
        where that leaves the frame; `valid` (optional) gets 1 / 0 (flow2d_warp_global_2d)."""
        _check(hip_lib().flow2d_warp_global_2d(self.handle, motion.ptr, frame.ptr, w, h, frame.pitch, fill, out.ptr,
                                               valid.ptr if valid else None), "flow2d_warp_global_2d")

    def region_records(self, max_regions=DEFAULT_MAX_REGIONS, instances=1):
        """A Plane for `instances` tables of `max_regions` flow2d_motion_region records (device memory)."""
        return self._record_plane(MOTION_REGION_BYTES, max(instances * max_regions, 1))

    def segment_summaries(self, instances=1):
        """A Plane for `instances` flow2d_segment_summary records (device memory)."""
        return self._record_plane(SEGMENT_SUMMARY_BYTES, instances)

    def read_regions(self, regions, count, max_regions=None, instance=0):
        """The first `count` records of instance `instance` of a region_records Plane whose tables hold `max_regions` records
        each, as MotionRegion structures (synchronises)."""
        if count == 0:
            return []
        stride = (count if max_regions is None else max_regions) * MOTION_REGION_BYTES // 4
        raw = regions.download((instance + 1) * stride, 1)[0, instance * stride:]
        return list((MotionRegion * count).from_buffer_copy(raw[:count * MOTION_REGION_BYTES // 4].tobytes()))

    def read_segment_summary(self, summary, instances=1):
        """The records of a segment_summaries Plane as SegmentSummary structures (synchronises)."""
        return self._read_records(summary, instances, SegmentSummary)

    def segment_motion(self, ru, rv, w, h, threshold, join=float("inf"), min_area=1, mask=None, max_regions=DEFAULT_MAX_REGIONS,
                       instances=1, labels=None, regions=None, summary=None):
        """The independently moving regions of the residual flow (ru, rv) (flow2d_segment_motion_2d): the pixels with
        |r| > threshold (and mask < 0.5) form the foreground, 4-neighbours whose residuals differ by at most `join` are joined,
        components below `min_area` pixels are dropped and the rest numbered from 1 in raster order of their first pixel.
        `labels` (a Plane, read as int32), `regions` (region_records) and `summary` (segment_summaries) stay on the device; the
        ones not given are the context's own.  With none of the three given the call downloads and returns
        (labels [h, w] int32 of instance 0, [MotionRegion] of instance 0, [SegmentSummary per instance]); otherwise nothing is
        returned or synchronised.  The workspace is the context's own (kept between calls)."""
        L = hip_lib()
        need = L.flow2d_segment_motion_workspace_bytes(w, h, instances)
        cached = getattr(self, "_segment_buffers", None)
        if cached is None or cached[0] < need:
            if cached is not None:
                cached[1].free()
                self._planes.remove(cached[1])
            self._segment_buffers = cached = (need, self.plane(max(need // 4, 4), 1))
        own = labels is None and regions is None and summary is None
        if own and instances != 1:
            raise ValueError("a lock-step batch takes the caller's labels, regions and summary")
        labels = labels or self.plane(ru.width, ru.height)
        if regions is None and max_regions > 0:
            regions = self.region_records(max_regions, instances)
        summary = summary or self.segment_summaries(instances)
        _check(L.flow2d_segment_motion_2d(self.handle, ru.ptr, rv.ptr, mask.ptr if mask else None, w, h, ru.pitch, float(threshold),
                                          float(join), int(min_area), labels.ptr, regions.ptr if max_regions > 0 else None,
                                          int(max_regions), summary.ptr, cached[1].ptr, cached[0]), "flow2d_segment_motion_2d")
        if not own:
            return None
        s = self.read_segment_summary(summary, 1)
        out = labels.download(w, h).view(np.int32), self.read_regions(regions, s[0].recorded, max_regions) if regions else [], s
        for q in (labels, regions, summary):
            if q:
                q.free()
                self._planes.remove(q)
        return out

    def deformation_records(self, instances=1):
        """A Plane for `instances` flow2d_deformation_stats records (device memory)."""
        return self._record_plane(DEFORMATION_STATS_BYTES, instances)

    def read_deformation_stats(self, stats, instances=1):
        """The records of a deformation_records Plane as DeformationStats structures (synchronises)."""
        return self._read_records(stats, instances, DeformationStats)

    def deformation(self, pu, pv, w, h, measure=STRAIN_SMALL, mask=None, planes=DEFORMATION_PLANES, stats=True, instances=1):
        """How the flow (pu, pv) deforms the material (flow2d_deformation_2d): divergence, vorticity, dilatation, the strain
        tensor of `measure` (STRAIN_SMALL or STRAIN_GREEN_LAGRANGE) and its principal values from differences that never reach
        across a pixel with mask >= 0.5 or a non-finite vector; NaN where a pixel has no derivative.
        planes: names from DEFORMATION_PLANES -- the call allocates those planes, downloads them and returns {name: [h, w]
        array} --, or a {name: Plane} dict of the caller's device planes, which are written and stay on the device.
        stats: True -- the record is read back (synchronises) --, a deformation_records Plane of the caller's, which is written
        and stays on the device, or False / None.  Returns (planes dict, DeformationStats or None); with the caller's planes and
        record nothing is downloaded or synchronised.  The workspace is the context's own (kept between calls)."""
        L = hip_lib()
        own_planes = not isinstance(planes, dict)
        held = {name: self.plane(pu.width, pu.height) for name in planes} if own_planes else dict(planes)
        unknown = [name for name in held if name not in DEFORMATION_PLANES]
        if unknown:
            raise ValueError("deformation planes are %s, not %s" % (", ".join(DEFORMATION_PLANES), unknown))
        out = DeformationPlanes(**{name: q.ptr for name, q in held.items()})
        own_stats = stats is True
        if own_stats and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        record = self.deformation_records(instances) if own_stats else (stats or None)
        workspace, need = None, 0
        if record is not None:
            need = L.flow2d_deformation_workspace_bytes(w, h, instances)
            cached = getattr(self, "_deformation_workspace", None)
            if cached is None or cached[0] < need:
                if cached is not None:
                    cached[1].free()
                    self._planes.remove(cached[1])
                self._deformation_workspace = cached = (need, self.plane(max(need // 4, 4), 1))
            workspace = cached[1]
        try:
            _check(L.flow2d_deformation_2d(self.handle, pu.ptr, pv.ptr, mask.ptr if mask else None, w, h, pu.pitch, int(measure),
                                           C.byref(out), record.ptr if record is not None else None,
                                           workspace.ptr if workspace else None, need), "flow2d_deformation_2d")
            result = {name: q.download(w, h) for name, q in held.items()} if own_planes else held
            return result, (self.read_deformation_stats(record, 1)[0] if own_stats else None)
        finally:
            for q in (list(held.values()) if own_planes else []) + ([record] if own_stats else []):
                q.free()
                self._planes.remove(q)

    def refine_records(self, instances=1):
        """A Plane for `instances` flow2d_refine_record records (device memory)."""
        return self._record_plane(REFINE_RECORD_BYTES, instances, 4)

    def read_refine_record(self, record, instances=1):
        """The records of a refine_records Plane as RefineRecord structures (synchronises)."""
        return self._read_records(record, instances, RefineRecord)

    def refine_flow(self, pu, pv, w, h, radius, guide=None, mask=None, sigma_guide=0.0, sigma_space=0.0, out_u=None, out_v=None,
                    record=True, instances=1):
        """The edge-aware weighted median of the flow (pu, pv) over a (2 radius + 1)^2 window (flow2d_refine_flow_2d): a sample
        weighs 1 - mask (mask: 1 where the vector is unreliable), times sigma_guide^2 / (sigma_guide^2 + d^2) for the
        difference d of the `guide` plane when there is one and sigma_guide > 0, times sigma_space^2 / (sigma_space^2 +
        distance^2) when sigma_space > 0; a pixel with nothing usable in its window keeps its vector.
        out_u, out_v: the caller's Planes, which are written and stay on the device; without them the call allocates both,
        downloads them and returns arrays.  record: True -- the counts are read back (synchronises) --, a refine_records Plane
        of the caller's, or False / None.  Returns (u, v, RefineRecord or None)."""
        own_planes = out_u is None and out_v is None
        if not own_planes and (out_u is None or out_v is None):
            raise ValueError("refine_flow takes both output planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        held = [self.plane(pu.width, pu.height), self.plane(pu.width, pu.height)] if own_planes else [out_u, out_v]
        rec = self.refine_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_refine_flow_2d(self.handle, pu.ptr, pv.ptr, guide.ptr if guide else None,
                                                   mask.ptr if mask else None, w, h, pu.pitch, int(radius), float(sigma_guide),
                                                   float(sigma_space), held[0].ptr, held[1].ptr,
                                                   rec.ptr if rec is not None else None), "flow2d_refine_flow_2d")
            u, v = (q.download(w, h) for q in held) if own_planes else held
            return u, v, (self.read_refine_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def correlation_records(self, instances=1):
        """A Plane for `instances` flow2d_correlation_record records (device memory)."""
        return self._record_plane(CORRELATION_RECORD_BYTES, instances, 4)

    def read_correlation_record(self, record, instances=1):
        """The records of a correlation_records Plane as CorrelationRecord structures (synchronises)."""
        return self._read_records(record, instances, CorrelationRecord)

    def correlate(self, f0, f1, w, h, lo, scale, radius, search, spacing, min_score=-1.0, node_u=None, node_v=None,
                  node_score=None, record=True, instances=1):
        """Window correlation of the frames f0 -> f1 (flow2d_correlate_2d): both are quantised to 8 bits by (I - lo) * scale, and
        every node of the grid correlation_grid(w, h, radius, spacing) gets the displacement, |dx|, |dy| <= `search` (the
        header's `range`), at which its (2 radius + 1)^2 window of f0 correlates best with f1, refined to sub-pixel by a parabola
        through the peak's neighbours; NaN where a node has no texture or no candidate, or scores below min_score.
        node_u, node_v (and optionally node_score): the caller's Planes, at least nw x nh, which are written and stay on the
        device; without them the call allocates all three, downloads them and returns arrays.  record: True -- the counts are read
        back (synchronises) --, a correlation_records Plane of the caller's, or False / None.
        Returns (u, v, score or None, CorrelationRecord or None)."""
        own_planes = node_u is None and node_v is None
        if not own_planes and (node_u is None or node_v is None):
            raise ValueError("correlate takes both node planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        nw, nh = correlation_grid(w, h, radius, spacing)
        held = [self.plane(nw, nh) for _ in range(3)] if own_planes else [node_u, node_v, node_score]
        rec = self.correlation_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_correlate_2d(self.handle, f0.ptr, f1.ptr, w, h, f0.pitch, float(lo), float(scale), int(radius),
                                                 int(search), int(spacing), float(min_score), held[0].ptr, held[1].ptr,
                                                 held[2].ptr if held[2] is not None else None, held[0].pitch,
                                                 rec.ptr if rec is not None else None), "flow2d_correlate_2d")
            u, v, score = (q.download(nw, nh) for q in held) if own_planes else held
            return u, v, score, (self.read_correlation_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def expand_nodes(self, node_u, node_v, nw, nh, radius, spacing, out_u, out_v, w, h):
        """A node field brought onto the w x h grid of the frame (flow2d_expand_nodes_2d): bilinear between the surrounding valid
        nodes, constant beyond the outermost ones, NaN where none of the four is valid."""
        _check(hip_lib().flow2d_expand_nodes_2d(self.handle, node_u.ptr, node_v.ptr, nw, nh, node_u.pitch, int(radius), int(spacing),
                                                out_u.ptr, out_v.ptr, w, h, out_u.pitch), "flow2d_expand_nodes_2d")

    def pass_records(self, instances=1):
        """A Plane for `instances` 64-byte records (flow2d_correlation_pass_record or flow2d_validation_record; device memory)."""
        return self._record_plane(CORRELATION_PASS_RECORD_BYTES, instances)

    def read_correlation_pass_record(self, record, instances=1):
        """The records of a pass_records Plane as CorrelationPassRecord structures (synchronises)."""
        return self._read_records(record, instances, CorrelationPassRecord)

    def read_validation_record(self, record, instances=1):
        """The records of a pass_records Plane as ValidationRecord structures (synchronises)."""
        return self._read_records(record, instances, ValidationRecord)

    def correlate_offset(self, f0, f1, w, h, lo, scale, radius, search, spacing, min_score=-1.0, predictor=None, node_u=None,
                         node_v=None, node_score=None, record=True, instances=1):
        """One pass of a multi-pass window correlation (flow2d_correlate_offset_2d): Context.correlate with the search of every node
        centred on the offset its pixel of the dense `predictor` -- a (u, v) pair of Planes of the frames' size, or None: no
        offset -- rounds to.  Node planes and record as for correlate; the record is a pass_records Plane or True.
        Returns (u, v, score or None, CorrelationPassRecord or None)."""
        own_planes = node_u is None and node_v is None
        if not own_planes and (node_u is None or node_v is None):
            raise ValueError("correlate_offset takes both node planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        pu, pv = predictor if predictor is not None else (None, None)
        nw, nh = correlation_grid(w, h, radius, spacing)
        held = [self.plane(nw, nh) for _ in range(3)] if own_planes else [node_u, node_v, node_score]
        rec = self.pass_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_correlate_offset_2d(self.handle, f0.ptr, f1.ptr, pu.ptr if pu is not None else None,
                                                        pv.ptr if pv is not None else None, w, h, f0.pitch, float(lo), float(scale),
                                                        int(radius), int(search), int(spacing), float(min_score), held[0].ptr,
                                                        held[1].ptr, held[2].ptr if held[2] is not None else None, held[0].pitch,
                                                        rec.ptr if rec is not None else None), "flow2d_correlate_offset_2d")
            u, v, score = (q.download(nw, nh) for q in held) if own_planes else held
            return u, v, score, (self.read_correlation_pass_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def validate_nodes(self, node_u, node_v, nw, nh, threshold=2.0, epsilon=0.1, min_neighbours=3, mode=VALIDATE_REPLACE, out_u=None,
                       out_v=None, out_flag=None, record=True, instances=1):
        """The normalised median test of a node field (flow2d_validate_nodes_2d), out of place: a node whose u or v lies more than
        `threshold` normalised residuals from the median of its finite neighbours is an outlier -- NaN with VALIDATE_FLAG, the
        neighbours' median with VALIDATE_REPLACE, which also fills invalid nodes; nodes with fewer than min_neighbours finite
        neighbours are copied.  out_u, out_v (and optionally out_flag): the caller's Planes, which stay on the device; without
        them the call allocates all three, downloads them and returns arrays.  record as for correlate_offset.
        Returns (u, v, flag or None, ValidationRecord or None)."""
        own_planes = out_u is None and out_v is None
        if not own_planes and (out_u is None or out_v is None):
            raise ValueError("validate_nodes takes both output planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        held = [self.plane(node_u.pitch // 4, nh) for _ in range(3)] if own_planes else [out_u, out_v, out_flag]
        rec = self.pass_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_validate_nodes_2d(self.handle, node_u.ptr, node_v.ptr, nw, nh, node_u.pitch, float(threshold),
                                                      float(epsilon), int(min_neighbours), int(mode), held[0].ptr, held[1].ptr,
                                                      held[2].ptr if held[2] is not None else None,
                                                      rec.ptr if rec is not None else None), "flow2d_validate_nodes_2d")
            u, v, flag = (q.download(nw, nh) for q in held) if own_planes else held
            return u, v, flag, (self.read_validation_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def correlate_masked(self, f0, f1, w, h, lo, scale, radius, search, spacing, mask, min_pixels=None, min_score=-1.0, predictor=None,
                         node_u=None, node_v=None, node_score=None, record=True, instances=1):
        """correlate_offset on a region of interest (flow2d_correlate_masked_2d): `mask` is a Plane of the frames' size in frame
        0's coordinates whose pixels with !(m < 0.5) are not the specimen -- or None, which forwards to correlate_offset.  The sums
        of a window run over its pixels that are not excluded; a node whose centre is excluded or whose window keeps fewer than
        min_pixels (None: correlation_min_pixels(radius)) is masked: NaN, score 0, counted in the record's `masked`.
        Returns (u, v, score or None, CorrelationPassRecord or None)."""
        own_planes = node_u is None and node_v is None
        if not own_planes and (node_u is None or node_v is None):
            raise ValueError("correlate_masked takes both node planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        pu, pv = predictor if predictor is not None else (None, None)
        nw, nh = correlation_grid(w, h, radius, spacing)
        held = [self.plane(nw, nh) for _ in range(3)] if own_planes else [node_u, node_v, node_score]
        rec = self.pass_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_correlate_masked_2d(self.handle, f0.ptr, f1.ptr, pu.ptr if pu is not None else None,
                                                        pv.ptr if pv is not None else None, w, h, f0.pitch, float(lo), float(scale),
                                                        int(radius), int(search), int(spacing), float(min_score),
                                                        mask.ptr if mask is not None else None,
                                                        correlation_min_pixels(radius) if min_pixels is None else int(min_pixels),
                                                        held[0].ptr, held[1].ptr, held[2].ptr if held[2] is not None else None,
                                                        held[0].pitch, rec.ptr if rec is not None else None),
                   "flow2d_correlate_masked_2d")
            u, v, score = (q.download(nw, nh) for q in held) if own_planes else held
            return u, v, score, (self.read_correlation_pass_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def validate_nodes_masked(self, node_u, node_v, nw, nh, mask, w, h, radius, spacing, threshold=2.0, epsilon=0.1, min_neighbours=3,
                              mode=VALIDATE_REPLACE, out_u=None, out_v=None, out_flag=None, record=True, instances=1):
        """validate_nodes on a region of interest (flow2d_validate_nodes_masked_2d): `mask` is the w x h Plane of correlate_masked
        and (radius, spacing) the grid the nw x nh nodes lie on.  A node whose centre pixel is excluded is off the specimen: never
        a neighbour, NaN with flag VALIDATE_FLAG_MASKED, counted in the record's `masked` only.  mask None forwards to
        validate_nodes.  Returns (u, v, flag or None, ValidationRecord or None)."""
        own_planes = out_u is None and out_v is None
        if not own_planes and (out_u is None or out_v is None):
            raise ValueError("validate_nodes_masked takes both output planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        held = [self.plane(node_u.pitch // 4, nh) for _ in range(3)] if own_planes else [out_u, out_v, out_flag]
        rec = self.pass_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_validate_nodes_masked_2d(self.handle, node_u.ptr, node_v.ptr, nw, nh, node_u.pitch, float(threshold),
                                                             float(epsilon), int(min_neighbours), int(mode),
                                                             mask.ptr if mask is not None else None, w, h,
                                                             mask.pitch if mask is not None else 0, int(radius), int(spacing),
                                                             held[0].ptr, held[1].ptr, held[2].ptr if held[2] is not None else None,
                                                             rec.ptr if rec is not None else None), "flow2d_validate_nodes_masked_2d")
            u, v, flag = (q.download(nw, nh) for q in held) if own_planes else held
            return u, v, flag, (self.read_validation_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def subset_records(self, instances=1):
        """A Plane for `instances` flow2d_subset_record records (device memory)."""
        return self._record_plane(SUBSET_RECORD_BYTES, instances)

    def read_subset_record(self, record, instances=1):
        """The records of a subset_records Plane as SubsetRecord structures (synchronises)."""
        return self._read_records(record, instances, SubsetRecord)

    def subset_refine(self, f0, f1, w, h, node_u0, node_v0, nw, nh, grid_radius, spacing, subset_radius, max_iterations=20,
                      epsilon=1e-3, max_shift=2.0, max_gradient=0.5, out_u=None, out_v=None, out_gradients=None, out_score=None,
                      out_state=None, record=True, instances=1):
        """Subset refinement of a node field (flow2d_subset_refine_2d): every node (i, j) of the Planes node_u0, node_v0 -- centred
        on pixel (grid_radius + i * spacing, grid_radius + j * spacing), as correlate, correlate_offset and validate_nodes deliver
        them -- is refined on the fp32 frames by the inverse-compositional Gauss-Newton iteration with an affine shape function
        over its (2 subset_radius + 1)^2 subset: the displacement to a few hundredths of a pixel and its four gradients.  A node
        stops when its step falls below `epsilon` (state: the iteration), after max_iterations (state 0), or as SUBSET_NO_INPUT,
        SUBSET_FLAT or SUBSET_STRAYED (more than max_shift from its start, a gradient beyond max_gradient, or out of the frame).
        out_u, out_v (and optionally out_gradients = (ux, uy, vx, vy), out_score, out_state): the caller's Planes, which are
        written and stay on the device; without them the call allocates all eight, downloads them and returns arrays.  record:
        True -- the counts are read back (synchronises) --, a subset_records Plane of the caller's, or False / None.
        Returns (u, v, (ux, uy, vx, vy) or None, score or None, state or None, SubsetRecord or None)."""
        def issue(held, rec):
            _check(hip_lib().flow2d_subset_refine_2d(self.handle, f0.ptr, f1.ptr, w, h, f0.pitch, node_u0.ptr, node_v0.ptr, nw, nh,
                                                     node_u0.pitch, int(grid_radius), int(spacing), int(subset_radius),
                                                     int(max_iterations), float(epsilon), float(max_shift), float(max_gradient),
                                                     *held, rec), "flow2d_subset_refine_2d")

        return self._subset_refine_call("subset_refine", issue, node_u0, nw, nh, out_u, out_v, [(out_gradients, 4)], out_score,
                                        out_state, record, instances)

    def _subset_refine_call(self, name, issue, node_u0, nw, nh, out_u, out_v, out_groups, out_score, out_state, record, instances):
        """What subset_refine, subset_refine_from, subset_refine_masked and subset_refine2 do around their entry: the planes --
        the caller's out_u, out_v, groups (each a (planes or None, count) pair: the gradients, at order 2 the curvatures too),
        out_score and out_state, or as many of the call's own --, the record, issue(held, rec) with their addresses (None: absent)
        in that order, the download of the call's own planes, and the result: (u, v, a tuple or None per group, score, state,
        SubsetRecord or None)."""
        own_planes = out_u is None and out_v is None
        if not own_planes and (out_u is None or out_v is None):
            raise ValueError("%s takes both output planes or neither" % name)
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        if own_planes:
            held = [self.plane(node_u0.pitch // 4, nh) for _ in range(4 + sum(n for _, n in out_groups))]
        else:
            held = [out_u, out_v]
            for planes, n in out_groups:
                held += list(planes if planes is not None else (None,) * n)
            held += [out_score, out_state]
        rec = self.subset_records(instances) if own_record else (record or None)
        try:
            issue([q.ptr if q is not None else None for q in held], rec.ptr if rec is not None else None)
            got = [q.download(nw, nh) for q in held] if own_planes else held
            groups, at = [], 2
            for _, n in out_groups:
                groups.append(tuple(got[at:at + n]) if got[at] is not None else None)
                at += n
            return (got[0], got[1], *groups, got[at], got[at + 1], self.read_subset_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def subset_refine_from(self, f0, f1, w, h, node_u0, node_v0, start_gradients, nw, nh, grid_radius, spacing, subset_radius,
                           max_iterations=20, epsilon=1e-3, max_shift=4.0, max_gradient=0.5, out_u=None, out_v=None, out_gradients=None,
                           out_score=None, out_state=None, record=True, instances=1):
        """Subset refinement started from a whole deformation (flow2d_subset_refine_from_2d): subset_refine with the start's four
        gradients, start_gradients = (ux0, uy0, vx0, vy0) Planes like node_u0 -- the previous step of a sequence against one
        reference frame, through predict_nodes --, or None: then every byte is subset_refine's.  A node whose start holds a value
        that is not finite is SUBSET_NO_INPUT; flat and strayed nodes hand back their whole start.  Outputs, record and the
        return value as for subset_refine."""
        def issue(held, rec):
            start = list(start_gradients) if start_gradients is not None else [None] * 4
            if len(start) != 4:
                raise ValueError("subset_refine_from takes the four start gradients (ux0, uy0, vx0, vy0) or None")
            _check(hip_lib().flow2d_subset_refine_from_2d(self.handle, f0.ptr, f1.ptr, w, h, f0.pitch, node_u0.ptr, node_v0.ptr,
                                                          *[q.ptr if q is not None else None for q in start], nw, nh, node_u0.pitch,
                                                          int(grid_radius), int(spacing), int(subset_radius), int(max_iterations),
                                                          float(epsilon), float(max_shift), float(max_gradient), *held, rec),
                   "flow2d_subset_refine_from_2d")

        return self._subset_refine_call("subset_refine_from", issue, node_u0, nw, nh, out_u, out_v, [(out_gradients, 4)], out_score,
                                        out_state, record, instances)

    def subset_refine_masked(self, f0, f1, w, h, node_u0, node_v0, start_gradients, nw, nh, grid_radius, spacing, subset_radius, mask,
                             min_pixels=None, max_iterations=20, epsilon=1e-3, max_shift=4.0, max_gradient=0.5, out_u=None, out_v=None,
                             out_gradients=None, out_score=None, out_state=None, record=True, instances=1):
        """Masked subset refinement, DIC on a region of interest (flow2d_subset_refine_masked_2d): subset_refine_from with `mask`, a
        Plane of the frames' size and pitch in frame 0's coordinates whose values of 0.5 and more (and NaN) mean "not the
        specimen".  A subset is refined on its usable pixels -- those whose own value and whose four gradient-stencil neighbours
        are not excluded --; a node whose centre is excluded or that has fewer than min_pixels usable pixels (None:
        subset_min_pixels(subset_radius)) is SUBSET_MASKED, NaN in all six planes, and counted in the record's `masked`.  mask =
        None: every byte is subset_refine_from's.  Outputs, record and the return value as for subset_refine."""
        return self._subset_refine_masked_entry("subset_refine_masked", "flow2d_subset_refine_masked_2d", f0, f1, w, h, node_u0, node_v0,
                                                start_gradients, nw, nh, grid_radius, spacing, subset_radius, mask, min_pixels,
                                                max_iterations, epsilon, max_shift, max_gradient, out_u, out_v, out_gradients, out_score,
                                                out_state, record, instances)

    def _subset_refine_masked_entry(self, name, entry, f0, f1, w, h, node_u0, node_v0, start_gradients, nw, nh, grid_radius, spacing,
                                    subset_radius, mask, min_pixels, max_iterations, epsilon, max_shift, max_gradient, out_u, out_v,
                                    out_gradients, out_score, out_state, record, instances):
        """subset_refine_masked and subset_refine_spline: one signature, `entry` of the library; f1 is frame 1 or its coefficients."""
        def issue(held, rec):
            start = list(start_gradients) if start_gradients is not None else [None] * 4
            if len(start) != 4:
                raise ValueError("%s takes the four start gradients (ux0, uy0, vx0, vy0) or None" % name)
            pixels = subset_min_pixels(subset_radius) if min_pixels is None else min_pixels
            _check(getattr(hip_lib(), entry)(self.handle, f0.ptr, f1.ptr, w, h, f0.pitch, node_u0.ptr, node_v0.ptr,
                                             *[q.ptr if q is not None else None for q in start], nw, nh, node_u0.pitch,
                                             int(grid_radius), int(spacing), int(subset_radius), int(max_iterations), float(epsilon),
                                             float(max_shift), float(max_gradient), mask.ptr if mask is not None else None, int(pixels),
                                             *held, rec), entry)

        return self._subset_refine_call(name, issue, node_u0, nw, nh, out_u, out_v, [(out_gradients, 4)], out_score, out_state, record,
                                        instances)

    def bspline_prefilter(self, src, w, h, out=None):
        """The cubic B-spline coefficients of the Plane `src` (flow2d_bspline_prefilter_2d), times 36: what subset_refine_spline and
        subset_refine2_spline sample in the place of frame 1.  The recursive prefilter's symmetric impulse response truncated at
        BSPLINE_HORIZON, rows then columns in double, whole-sample mirroring at the borders; one launch, which honours set_batch.
        out: a Plane of src's pitch that is written and returned, or None: the call allocates one (the caller frees it)."""
        dst = out if out is not None else self.plane(src.width, src.height)
        _check(hip_lib().flow2d_bspline_prefilter_2d(self.handle, src.ptr, dst.ptr, w, h, src.pitch), "flow2d_bspline_prefilter_2d")
        return dst

    def subset_refine_spline(self, f0, coeff_1, w, h, node_u0, node_v0, start_gradients, nw, nh, grid_radius, spacing, subset_radius,
                             mask=None, min_pixels=None, max_iterations=20, epsilon=1e-3, max_shift=4.0, max_gradient=0.5, out_u=None,
                             out_v=None, out_gradients=None, out_score=None, out_state=None, record=True, instances=1):
        """subset_refine_masked with the cubic B-spline sample of frame 1 in the place of the Catmull-Rom one
        (flow2d_subset_refine_spline_2d): coeff_1 is the Plane bspline_prefilter made from frame 1.  A tenth of the interpolation
        bias in the displacement for the same sixteen taps.  mask = None: the bytes of a mask that excludes nothing.  Everything
        else, outputs, record and the return value as for subset_refine_masked."""
        return self._subset_refine_masked_entry("subset_refine_spline", "flow2d_subset_refine_spline_2d", f0, coeff_1, w, h, node_u0,
                                                node_v0, start_gradients, nw, nh, grid_radius, spacing, subset_radius, mask, min_pixels,
                                                max_iterations, epsilon, max_shift, max_gradient, out_u, out_v, out_gradients, out_score,
                                                out_state, record, instances)

    def subset_refine2(self, f0, f1, w, h, node_u0, node_v0, nw, nh, grid_radius, spacing, subset_radius, max_iterations=20,
                       epsilon=1e-3, max_shift=2.0, max_gradient=0.5, max_curvature=0.05, start_gradients=None, start_curvatures=None,
                       out_u=None, out_v=None, out_gradients=None, out_curvatures=None, out_score=None, out_state=None, record=True,
                       instances=1, _entry="flow2d_subset_refine2_2d"):
        """Subset refinement with a second-order shape function (flow2d_subset_refine2_2d): subset_refine_from with twelve
        parameters per node -- the displacement, its four gradients and the six curvatures (uxx, uxy, uyy, vxx, vxy, vyy) -- for
        subsets that bend; subset_radius from 2.  start_gradients = (ux0, uy0, vx0, vy0) and start_curvatures = (uxx0, uxy0, uyy0,
        vxx0, vxy0, vyy0): Planes like node_u0, or None (0); the curvatures only with the gradients.  A curvature beyond
        max_curvature (per pixel) strays.  out_u, out_v (and optionally out_gradients, out_curvatures, out_score, out_state): the
        caller's Planes; without them the call allocates all fourteen, downloads them and returns arrays.  record as for
        subset_refine.  Returns (u, v, (ux, uy, vx, vy) or None, (uxx, uxy, uyy, vxx, vxy, vyy) or None, score or None, state or
        None, SubsetRecord or None)."""
        def start(planes, n, what):
            if planes is None:
                return None
            planes = list(planes)
            if len(planes) != n:
                raise ValueError("subset_refine2 takes %d %s or None" % (n, what))
            return (C.c_void_p * n)(*[q.ptr if q is not None else None for q in planes])

        def issue(held, rec):
            if len(held) != 14:
                raise ValueError("subset_refine2 takes four gradient planes and six curvature planes")
            _check(getattr(hip_lib(), _entry)(self.handle, f0.ptr, f1.ptr, w, h, f0.pitch, node_u0.ptr, node_v0.ptr,
                                              start(start_gradients, 4, "start gradients"),
                                              start(start_curvatures, 6, "start curvatures"), nw, nh, node_u0.pitch,
                                              int(grid_radius), int(spacing), int(subset_radius), int(max_iterations),
                                              float(epsilon), float(max_shift), float(max_gradient), float(max_curvature),
                                              held[0], held[1], (C.c_void_p * 4)(*held[2:6]), (C.c_void_p * 6)(*held[6:12]),
                                              held[12], held[13], rec), _entry)

        return self._subset_refine_call("subset_refine2", issue, node_u0, nw, nh, out_u, out_v, [(out_gradients, 4), (out_curvatures, 6)],
                                        out_score, out_state, record, instances)

    def subset_refine2_spline(self, f0, coeff_1, w, h, node_u0, node_v0, nw, nh, grid_radius, spacing, subset_radius, **options):
        """subset_refine2 with the cubic B-spline sample of frame 1 (flow2d_subset_refine2_spline_2d): coeff_1 is the Plane
        bspline_prefilter made from frame 1.  Options, outputs and the return value as for subset_refine2."""
        if "_entry" in options:
            raise TypeError("subset_refine2_spline() got an unexpected keyword argument '_entry'")
        return self.subset_refine2(f0, coeff_1, w, h, node_u0, node_v0, nw, nh, grid_radius, spacing, subset_radius,
                                   _entry="flow2d_subset_refine2_spline_2d", **options)

    def uncertainty_records(self, instances=1):
        """A Plane for `instances` flow2d_uncertainty_record records (device memory)."""
        return self._record_plane(UNCERTAINTY_RECORD_BYTES, instances)

    def read_uncertainty_record(self, record, instances=1):
        """The records of an uncertainty_records Plane as UncertaintyRecord structures (synchronises)."""
        return self._read_records(record, instances, UncertaintyRecord)

    def subset_uncertainty(self, f0, f1, w, h, nodes, state, nw, nh, grid_radius, spacing, subset_radius, min_state=1,
                           interpolation=SUBSET_CATMULL_ROM, mask=None, min_pixels=None, out=None, record=True, instances=1):
        """The uncertainty of a first-order refinement's nodes (flow2d_subset_uncertainty_2d): per node the covariance s2 * H^-1 of
        p at nodes = (u, v, ux, uy, vx, vy) Planes with their `state` Plane, as subset_refine and its siblings wrote them -- s2 the
        residual variance of the ZNSSD there over N - 8 degrees of freedom, H the refinement's Hessian.  f1 is frame 1, or with
        interpolation = SUBSET_BSPLINE the Plane bspline_prefilter made from it; mask and min_pixels (None:
        subset_min_pixels(subset_radius)) as for subset_refine_masked.  A node with a state below min_state or a value that is not
        finite, off the mask, out of the frame, flat or with fewer than nine usable pixels gets NaN in every plane and is counted
        in the record.  The sigmas estimate the random error that the frames' noise puts into p, in pixels (gradients: per
        pixel); `noise` is sqrt(s2) in grey values, `rho` the correlation of u and v.  They say nothing about interpolation bias.
        out: eight Planes of the caller's in the order of SUBSET_UNCERTAINTY_PLANES, None where a plane is not wanted (sigma_u and
        sigma_v are required, the four gradient sigmas go all or none), which are written and stay on the device; without `out`
        the call allocates all eight, downloads them and returns arrays.  record: True -- the counts are read back
        (synchronises) --, an uncertainty_records Plane of the caller's, or False / None.
        Returns (a tuple of the eight planes, UncertaintyRecord or None)."""
        if len(nodes) != 6:
            raise ValueError("subset_uncertainty takes the six planes (u, v, ux, uy, vx, vy)")
        own_planes = out is None
        if not own_planes and len(out) != len(SUBSET_UNCERTAINTY_PLANES):
            raise ValueError("subset_uncertainty takes eight output planes (None: absent) or none")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        held = [self.plane(nodes[0].pitch // 4, nh) for _ in SUBSET_UNCERTAINTY_PLANES] if own_planes else list(out)
        rec = self.uncertainty_records(instances) if own_record else (record or None)
        pixels = subset_min_pixels(subset_radius) if min_pixels is None else min_pixels
        try:
            _check(hip_lib().flow2d_subset_uncertainty_2d(self.handle, f0.ptr, f1.ptr, int(interpolation), w, h, f0.pitch,
                                                          *[q.ptr for q in nodes], state.ptr, nw, nh, nodes[0].pitch, int(grid_radius),
                                                          int(spacing), int(subset_radius), int(min_state),
                                                          mask.ptr if mask is not None else None, int(pixels),
                                                          *[q.ptr if q is not None else None for q in held],
                                                          rec.ptr if rec is not None else None), "flow2d_subset_uncertainty_2d")
            got = [q.download(nw, nh) for q in held] if own_planes else held
            return tuple(got), (self.read_uncertainty_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def predict_records(self, instances=1):
        """A Plane for `instances` flow2d_predict_record records (device memory)."""
        return self._record_plane(PREDICT_RECORD_BYTES, instances)

    def read_predict_record(self, record, instances=1):
        """The records of a predict_records Plane as PredictRecord structures (synchronises)."""
        return self._read_records(record, instances, PredictRecord)

    def predict_nodes(self, nodes, state, nw, nh, spacing, min_state=1, min_neighbours=1, out=None, out_state=None, record=True,
                      instances=1):
        """The start of a sequence's next step from a step's result (flow2d_predict_nodes_2d), out of place: nodes = (u, v, ux, uy,
        vx, vy) Planes and their `state` Plane, as subset_refine / subset_refine_from wrote them.  A node with state >= min_state
        and six finite values is kept; any other takes, per value, the median of what its usable neighbours -- min_neighbours of
        the eight at least -- extrapolate to it (u and v along the neighbour's gradients, `spacing` pixels per node), with the
        state SUBSET_STATE_PREDICTED, or NaN and SUBSET_NO_INPUT where too few are usable: a second pass fills further.
        out = six Planes of the caller's (and optionally out_state), which stay on the device; without them the call allocates
        all seven, downloads them and returns arrays.  record: True, a predict_records Plane, or False / None.
        Returns ((u, v, ux, uy, vx, vy), state or None, PredictRecord or None)."""
        if len(nodes) != 6:
            raise ValueError("predict_nodes takes the six planes (u, v, ux, uy, vx, vy)")
        own_planes = out is None
        if not own_planes and len(out) != 6:
            raise ValueError("predict_nodes takes six output planes or none")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        held = [self.plane(nodes[0].pitch // 4, nh) for _ in range(7)] if own_planes else list(out) + [out_state]
        rec = self.predict_records(instances) if own_record else (record or None)
        try:
            _check(hip_lib().flow2d_predict_nodes_2d(self.handle, *[q.ptr for q in nodes], state.ptr, nw, nh, nodes[0].pitch, int(spacing),
                                                     int(min_state), int(min_neighbours),
                                                     *[q.ptr if q is not None else None for q in held],
                                                     rec.ptr if rec is not None else None), "flow2d_predict_nodes_2d")
            got = [q.download(nw, nh) for q in held] if own_planes else held
            return tuple(got[:6]), got[6], (self.read_predict_record(rec, 1)[0] if own_record else None)
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    def compose_records(self, instances=1):
        """A Plane for `instances` flow2d_compose_record records (device memory)."""
        return self._record_plane(COMPOSE_RECORD_BYTES, instances)

    def read_compose_record(self, record, instances=1):
        """The records of a compose_records Plane as ComposeRecord structures (synchronises)."""
        return self._read_records(record, instances, ComposeRecord)

    def compose_nodes(self, base, increment, nw, nh, grid_radius, spacing, min_state=1, score=None, out=None, out_state=None,
                      out_score=None, record=True, instances=1):
        """The composition of two node fields across a moved reference frame (flow2d_compose_nodes_2d), out of place: base =
        (u, v, ux, uy, vx, vy, state) Planes of frame 0 -> frame r at the nodes of frame 0, increment = the same seven of
        frame r -> frame k on the same grid (grid_radius, spacing) laid in frame r, `score` the increment's score Plane or None.
        The increment is sampled where the base carries each node -- over the usable corners of its cell, each extrapolated along
        its gradients -- and the deformation gradients are multiplied; a composed node gets the state SUBSET_STATE_COMPOSED, a
        node without a usable base, carried more than half a cell off the grid or without a usable corner NaN and SUBSET_NO_INPUT.
        out = six Planes of the caller's (and optionally out_state, and out_score with `score`), which stay on the device;
        without them the call allocates them all, downloads them and returns arrays.  record: True, a compose_records Plane, or
        False / None.
        Returns ((u, v, ux, uy, vx, vy), state or None, score or None, ComposeRecord or None)."""
        if len(base) != 7 or len(increment) != 7:
            raise ValueError("compose_nodes takes the seven planes (u, v, ux, uy, vx, vy, state) of the base and of the increment")
        own_planes = out is None
        if not own_planes and len(out) != 6:
            raise ValueError("compose_nodes takes six output planes or none")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        if own_planes:
            held = [self.plane(base[0].pitch // 4, nh) for _ in range(7 if score is None else 8)] + ([None] if score is None else [])
        else:
            held = list(out) + [out_state, out_score]
        rec = self.compose_records(instances) if own_record else (record or None)
        ptr = lambda q: q.ptr if q is not None else None  # noqa: E731
        try:
            _check(hip_lib().flow2d_compose_nodes_2d(self.handle, (C.c_void_p * 7)(*[q.ptr for q in base]),
                                                     (C.c_void_p * 7)(*[q.ptr for q in increment]), ptr(score), nw, nh, base[0].pitch,
                                                     int(grid_radius), int(spacing), int(min_state),
                                                     (C.c_void_p * 6)(*[q.ptr for q in held[:6]]), ptr(held[6]), ptr(held[7]), ptr(rec)),
                   "flow2d_compose_nodes_2d")
            got = [q.download(nw, nh) if q is not None else None for q in held] if own_planes else held
            return tuple(got[:6]), got[6], got[7], (self.read_compose_record(rec, 1)[0] if own_record else None)
        finally:
            for q in ([q for q in held if q is not None] if own_planes else []) + ([rec] if own_record else []):
                q.free()
                self._planes.remove(q)

    @staticmethod
    def node_strain_workspace_bytes(nw, nh, instances=1):
        """flow2d_node_strain_workspace_bytes: what node_strain needs beside a record (host logic, no device)."""
        return hip_lib().flow2d_node_strain_workspace_bytes(nw, nh, instances)

    def node_strain(self, node_u, node_v, nw, nh, spacing, window=2, order=1, min_nodes=0, min_state=1, measure=STRAIN_SMALL,
                    state=None, gradients=None, planes=DEFORMATION_PLANES, stats=True, instances=1):
        """Strain on the node grid (flow2d_node_strain_2d): the nine quantities of `deformation` at every node of the nw x nh
        planes node_u, node_v, from the least-squares fit of a polynomial of `order` (1 or 2) to the usable nodes within
        `window` nodes around each node, or, with window = 0, from `gradients` = the (ux, uy, vx, vy) Planes of a subset
        refinement.  state: the refinement's state Plane -- a node below min_state is left out -- or None: every finite node
        is usable.  min_nodes: the fewest usable nodes a window may hold, 0 = one more than the fit has coefficients.
        planes / stats / the return value: as `deformation`, on the node grid; the record's reserved[0 .. 2] count the nodes
        lost for their centre, for too few nodes and for a degenerate window."""
        L = hip_lib()
        if gradients is not None and len(gradients) != 4:
            raise ValueError("node_strain takes the four gradient planes (ux, uy, vx, vy) or none")
        if window > 0 and min_nodes == 0:
            min_nodes = (6 if order == 2 else 3) + 1
        own_planes = not isinstance(planes, dict)
        held = {name: self.plane(node_u.width, node_u.height) for name in planes} if own_planes else dict(planes)
        unknown = [name for name in held if name not in DEFORMATION_PLANES]
        if unknown:
            raise ValueError("deformation planes are %s, not %s" % (", ".join(DEFORMATION_PLANES), unknown))
        out = DeformationPlanes(**{name: q.ptr for name, q in held.items()})
        own_stats = stats is True
        if own_stats and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        record = self.deformation_records(instances) if own_stats else (stats or None)
        workspace, need = None, 0
        if record is not None:
            need = L.flow2d_node_strain_workspace_bytes(nw, nh, instances)
            cached = getattr(self, "_node_strain_workspace", None)
            if cached is None or cached[0] < need:
                if cached is not None:
                    cached[1].free()
                    self._planes.remove(cached[1])
                self._node_strain_workspace = cached = (need, self.plane(max(need // 4, 4), 1))
            workspace = cached[1]
        try:
            _check(L.flow2d_node_strain_2d(self.handle, node_u.ptr, node_v.ptr, state.ptr if state is not None else None,
                                           *([q.ptr for q in gradients] if gradients else [None] * 4), nw, nh, node_u.pitch, int(spacing),
                                           int(window), int(order), int(min_nodes), int(min_state), int(measure), C.byref(out),
                                           record.ptr if record is not None else None, workspace.ptr if workspace else None, need),
                   "flow2d_node_strain_2d")
            result = {name: q.download(nw, nh) for name, q in held.items()} if own_planes else held
            return result, (self.read_deformation_stats(record, 1)[0] if own_stats else None)
        finally:
            for q in (list(held.values()) if own_planes else []) + ([record] if own_stats else []):
                q.free()
                self._planes.remove(q)

    @staticmethod
    def node_strain_robust_workspace_bytes(nw, nh, instances=1):
        """flow2d_node_strain_robust_workspace_bytes: what node_strain_robust needs beside a record (host logic, no device)."""
        return hip_lib().flow2d_node_strain_robust_workspace_bytes(nw, nh, instances)

    def node_strain_robust(self, node_u, node_v, nw, nh, spacing, window=2, order=1, min_nodes=0, min_state=1, measure=STRAIN_SMALL,
                           sigma=0.05, iterations=8, state=None, planes=DEFORMATION_PLANES, diagnostics=NODE_STRAIN_DIAGNOSTICS,
                           stats=True, instances=1):
        """Robust strain windows (flow2d_node_strain_robust_2d): `node_strain` with window >= 1 as `iterations` passes of
        reweighted least squares with a Cauchy weight of scale `sigma` pixels; a tap further than sigma from the last fit is
        not kept, a window that keeps fewer than min_nodes is sparse.  diagnostics: names of NODE_STRAIN_DIAGNOSTICS (downloaded
        into the returned dict beside the planes) or a dict of the caller's Planes by those names.  The record's
        reserved[3 .. 5] are read by node_strain_robust_counts.  Otherwise as `node_strain`."""
        L = hip_lib()
        if min_nodes == 0:
            min_nodes = (6 if order == 2 else 3) + 1
        own_planes = not isinstance(planes, dict)
        own_diagnostics = not isinstance(diagnostics, dict)
        held = {name: self.plane(node_u.width, node_u.height) for name in planes} if own_planes else dict(planes)
        held_diag = {name: self.plane(node_u.width, node_u.height) for name in diagnostics} if own_diagnostics else dict(diagnostics)
        unknown = [name for name in held if name not in DEFORMATION_PLANES] + [name for name in held_diag if name not in NODE_STRAIN_DIAGNOSTICS]
        if unknown:
            raise ValueError("deformation planes are %s and diagnostics %s, not %s" %
                             (", ".join(DEFORMATION_PLANES), ", ".join(NODE_STRAIN_DIAGNOSTICS), unknown))
        out = DeformationPlanes(**{name: q.ptr for name, q in held.items()})
        diag = NodeStrainDiagnostics(**{name: q.ptr for name, q in held_diag.items()})
        own_stats = stats is True
        if own_stats and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        record = self.deformation_records(instances) if own_stats else (stats or None)
        workspace, need = None, 0
        if record is not None:
            need = L.flow2d_node_strain_robust_workspace_bytes(nw, nh, instances)
            cached = getattr(self, "_node_strain_robust_workspace", None)
            if cached is None or cached[0] < need:
                if cached is not None:
                    cached[1].free()
                    self._planes.remove(cached[1])
                self._node_strain_robust_workspace = cached = (need, self.plane(max(need // 4, 4), 1))
            workspace = cached[1]
        own = (list(held.values()) if own_planes else []) + (list(held_diag.values()) if own_diagnostics else [])
        try:
            _check(L.flow2d_node_strain_robust_2d(self.handle, node_u.ptr, node_v.ptr, state.ptr if state is not None else None, nw, nh,
                                                  node_u.pitch, int(spacing), int(window), int(order), int(min_nodes), int(min_state),
                                                  int(measure), float(sigma), int(iterations), C.byref(out), C.byref(diag),
                                                  record.ptr if record is not None else None, workspace.ptr if workspace else None, need),
                   "flow2d_node_strain_robust_2d")
            result = {name: q.download(nw, nh) for name, q in held.items()} if own_planes else dict(held)
            result.update({name: q.download(nw, nh) for name, q in held_diag.items()} if own_diagnostics else held_diag)
            return result, (self.read_deformation_stats(record, 1)[0] if own_stats else None)
        finally:
            for q in own + ([record] if own_stats else []):
                q.free()
                self._planes.remove(q)

    @staticmethod
    def node_strain_weighted_workspace_bytes(nw, nh, instances=1):
        """flow2d_node_strain_weighted_workspace_bytes: what node_strain_weighted needs beside a record (host logic, no device)."""
        return hip_lib().flow2d_node_strain_weighted_workspace_bytes(nw, nh, instances)

    def node_strain_weighted(self, node_u, node_v, sigma_u, sigma_v, nw, nh, spacing, window=2, order=1, min_nodes=0, min_state=1,
                             measure=STRAIN_SMALL, sigma_floor=0.0, threshold=0.0, iterations=0, state=None, planes=DEFORMATION_PLANES,
                             diagnostics=(), sigmas=STRAIN_SIGMA_PLANES, stats=True, instances=1):
        """Weighted strain windows (flow2d_node_strain_weighted_2d): `node_strain` with window >= 1 as a Gauss-Markov fit whose
        weights are 1 / (sigma^2 + sigma_floor^2) from the Planes sigma_u, sigma_v of `subset_uncertainty`, with the standard
        deviations of the strain.  threshold > 0: `iterations` reweighted passes as in `node_strain_robust`, the scale in sigmas.
        sigmas: names of STRAIN_SIGMA_PLANES (downloaded into the returned dict) or a dict of the caller's Planes by those names;
        diagnostics likewise.  The record's reserved[3 .. 6] are read by node_strain_weighted_counts.  Otherwise as `node_strain`."""
        L = hip_lib()
        if min_nodes == 0:
            min_nodes = (6 if order == 2 else 3) + 1
        groups = []
        for given, names in ((planes, DEFORMATION_PLANES), (diagnostics, NODE_STRAIN_DIAGNOSTICS), (sigmas, STRAIN_SIGMA_PLANES)):
            own = not isinstance(given, dict)
            held = {name: self.plane(node_u.width, node_u.height) for name in given} if own else dict(given)
            groups.append((own, held, names))
        unknown = [name for _, held, names in groups for name in held if name not in names]
        if unknown:
            for own, held, _ in groups:
                for q in (held.values() if own else ()):
                    q.free()
                    self._planes.remove(q)
            raise ValueError("deformation planes are %s, diagnostics %s and sigmas %s, not %s" %
                             (", ".join(DEFORMATION_PLANES), ", ".join(NODE_STRAIN_DIAGNOSTICS), ", ".join(STRAIN_SIGMA_PLANES), unknown))
        out = DeformationPlanes(**{name: q.ptr for name, q in groups[0][1].items()})
        diag = NodeStrainDiagnostics(**{name: q.ptr for name, q in groups[1][1].items()})
        sig = StrainSigmaPlanes(**{name: q.ptr for name, q in groups[2][1].items()})
        own_stats = stats is True
        if own_stats and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        record = self.deformation_records(instances) if own_stats else (stats or None)
        workspace, need = None, 0
        if record is not None:
            need = L.flow2d_node_strain_weighted_workspace_bytes(nw, nh, instances)
            cached = getattr(self, "_node_strain_weighted_workspace", None)
            if cached is None or cached[0] < need:
                if cached is not None:
                    cached[1].free()
                    self._planes.remove(cached[1])
                self._node_strain_weighted_workspace = cached = (need, self.plane(max(need // 4, 4), 1))
            workspace = cached[1]
        try:
            _check(L.flow2d_node_strain_weighted_2d(self.handle, node_u.ptr, node_v.ptr, state.ptr if state is not None else None,
                                                    sigma_u.ptr, sigma_v.ptr, nw, nh, node_u.pitch, int(spacing), int(window), int(order),
                                                    int(min_nodes), int(min_state), int(measure), float(sigma_floor), float(threshold),
                                                    int(iterations), C.byref(out), C.byref(diag), C.byref(sig),
                                                    record.ptr if record is not None else None, workspace.ptr if workspace else None, need),
                   "flow2d_node_strain_weighted_2d")
            result = {}
            for own, held, _ in groups:
                result.update({name: q.download(nw, nh) for name, q in held.items()} if own else held)
            return result, (self.read_deformation_stats(record, 1)[0] if own_stats else None)
        finally:
            for q in [q for own, held, _ in groups if own for q in held.values()] + ([record] if own_stats else []):
                q.free()
                self._planes.remove(q)

    def resample_x(self, src, dst, out_w, out_h, in_w):
        _check(hip_lib().flow2d_resample_x(self.handle, src.ptr, dst.ptr, out_w, out_h, in_w, src.pitch),
               "flow2d_resample_x")

    def resample_y(self, src, dst, out_w, out_h, in_h):
        _check(hip_lib().flow2d_resample_y(self.handle, src.ptr, dst.ptr, out_w, out_h, in_h, src.pitch),
               "flow2d_resample_y")

    def resample_xy(self, src, dst, in_w, in_h, out_w, out_h, src_b=None, dst_b=None):
        """Both resample passes in one launch (no temp plane); optional second plane."""
        _check(hip_lib().flow2d_resample_xy_pair(self.handle, src.ptr, dst.ptr, src_b.ptr if src_b else None,
                                                 dst_b.ptr if dst_b else None, in_w, in_h, out_w, out_h, src.pitch),
               "flow2d_resample_xy_pair")

    def upsample_registration(self, u, v, in_w, in_h, out_u, out_v, f0, f1, w, h, hx, hy, out):
        """(u, v) of the previous level resampled to w x h into out_u / out_v and f1 warped by them into `out`: one launch.
        u = v = None with in_w = in_h = 0 (the coarsest level): out_u = out_v = 0 and the warp by that."""
        _check(hip_lib().flow2d_upsample_registration_2d(self.handle, u.ptr if u else None, v.ptr if v else None, in_w, in_h, out_u.ptr,
                                                         out_v.ptr, f0.ptr, f1.ptr,
                                                         w, h, f0.pitch, hx, hy, out.ptr), "flow2d_upsample_registration_2d")

    def upsample_registration_half(self, u, v, in_w, in_h, out_u, out_v, f0, f1, w, h, hx, hy, out):
        """upsample_registration at an exactly doubled level with out_u / out_v kept at in_w x in_h (read as [y >> 1][x >> 1])."""
        _check(hip_lib().flow2d_upsample_registration_half_2d(self.handle, u.ptr, v.ptr, in_w, in_h, out_u.ptr, out_v.ptr, f0.ptr, f1.ptr,
                                                              w, h, f0.pitch, hx, hy, out.ptr), "flow2d_upsample_registration_half_2d")

    def prior_records(self, instances=1):
        """A Plane for the `instances` counts (one unsigned 64-bit integer each) of prior_registration, device memory."""
        return self._record_plane(8, instances, 4)

    def read_prior_records(self, record, instances=1):
        """The counts of a prior_records Plane as a list of ints (synchronises)."""
        return self._read_records(record, instances, C.c_uint64)

    def prior_registration(self, prior_u, prior_v, in_w, in_h, out_u, out_v, f0, f1, w, h, hx, hy, out, record=True):
        """The first level of a pyramid started from a prior flow (flow2d_prior_registration_2d): the in_w x in_h prior (prior_u,
        prior_v), in full-resolution pixels, made finite -- a pixel where either component is not finite counts as (0, 0) --,
        resampled to w x h into out_u / out_v, and f1 warped by that into `out`: one launch.  record: True -- the count of prior
        pixels that were not finite is read back and returned (synchronises) --, or a prior_records Plane of the caller's (a
        lock-step batch takes one count per instance), which stays on the device."""
        own = record is True
        rec = self.prior_records(1) if own else record
        try:
            _check(hip_lib().flow2d_prior_registration_2d(self.handle, prior_u.ptr, prior_v.ptr, in_w, in_h, out_u.ptr, out_v.ptr, f0.ptr,
                                                          f1.ptr, w, h, f0.pitch, hx, hy, out.ptr, rec.ptr if rec is not None else None),
                   "flow2d_prior_registration_2d")
            return self.read_prior_records(rec, 1)[0] if own else None
        finally:
            if own:
                rec.free()
                self._planes.remove(rec)

    def propagate_records(self, instances=1):
        """A Plane for `instances` flow2d_propagate_record records (device memory)."""
        return self._record_plane(PROPAGATE_RECORD_BYTES, instances, 4)

    def read_propagate_record(self, record, instances=1):
        """The records of a propagate_records Plane as PropagateRecord structures (synchronises)."""
        return self._read_records(record, instances, PropagateRecord)

    def propagate_workspace(self, w, h, instances=1):
        """A Plane of flow2d_propagate_flow_workspace_bytes(w, h, instances) bytes (device memory)."""
        return self.plane(max(hip_lib().flow2d_propagate_flow_workspace_bytes(w, h, instances) // 4, 4), 1)

    def propagate_flow(self, pu, pv, w, h, mask=None, frame_from=None, frame_to=None, step=1.0, photo_scale=1.0, fill_passes=4,
                       out_u=None, out_v=None, record=True, workspace=None, instances=1):
        """The flow (pu, pv) carried `step` times along itself onto the grid of the frame it leads to (flow2d_propagate_flow_2d): a
        deterministic forward splat -- where several vectors land on one pixel the one whose source matches best photometrically
        (frame_from at the source against frame_to at the landing point, times photo_scale; both frames or neither) wins, then the one
        that lands nearest to the pixel's centre, then the lowest source index --, a pixel no vector reaches is NaN, and fill_passes
        passes fill such holes with the mean of their finite neighbours.  mask: 1 where a vector is not to be carried.
        out_u, out_v: the caller's Planes, which are written and stay on the device; without them the call allocates both, downloads
        them and returns arrays.  record: True -- the counts are read back (synchronises) --, a propagate_records Plane of the
        caller's, or False / None.  workspace: a propagate_workspace Plane of the caller's (a captured launch needs one that
        outlives the call).  Returns (u, v, PropagateRecord or None)."""
        own_planes = out_u is None and out_v is None
        if not own_planes and (out_u is None or out_v is None):
            raise ValueError("propagate_flow takes both output planes or neither")
        own_record = record is True
        if own_record and instances != 1:
            raise ValueError("a lock-step batch takes the caller's records")
        held = [self.plane(pu.width, pu.height), self.plane(pu.width, pu.height)] if own_planes else [out_u, out_v]
        rec = self.propagate_records(instances) if own_record else (record or None)
        own_workspace = workspace is None
        work = self.propagate_workspace(w, h, instances) if own_workspace else workspace
        try:
            _check(hip_lib().flow2d_propagate_flow_2d(self.handle, pu.ptr, pv.ptr, mask.ptr if mask else None,
                                                      frame_from.ptr if frame_from else None, frame_to.ptr if frame_to else None, w, h,
                                                      pu.pitch, float(step), float(photo_scale), int(fill_passes), held[0].ptr,
                                                      held[1].ptr, rec.ptr if rec is not None else None, work.ptr),
                   "flow2d_propagate_flow_2d")
            u, v = (q.download(w, h) for q in held) if own_planes else held
            result = u, v, (self.read_propagate_record(rec, 1)[0] if own_record else None)
            if own_workspace and not (own_planes or own_record):
                self.synchronize()  # the workspace is freed below: the queued launches must have used it
            return result
        finally:
            for q in (held if own_planes else []) + ([rec] if own_record else []) + ([work] if own_workspace else []):
                q.free()
                self._planes.remove(q)

    def resample_x_levels(self, src, packed, in_w, h, widths, columns, src_b=None, packed_b=None):
        """x pass for several output widths in one trip over `src`; level l lands in columns[l] .. of `packed`."""
        n = len(widths)
        ws = (C.c_size_t * n)(*widths)
        cs = (C.c_size_t * n)(*columns)
        _check(hip_lib().flow2d_resample_x_levels(self.handle, src.ptr, packed.ptr, src_b.ptr if src_b else None,
                                                  packed_b.ptr if packed_b else None, in_w, h, src.pitch, n, ws, cs),
               "flow2d_resample_x_levels")

    # two planes of the same geometry per launch
    def add_pair(self, op0_a, op1_a, op0_b, op1_b, w, h):
        _check(hip_lib().flow2d_add_2d_pair(self.handle, op0_a.ptr, op1_a.ptr, op0_b.ptr, op1_b.ptr, w, h, op0_a.pitch),
               "flow2d_add_2d_pair")

    def median_pair(self, src_a, src_b, w, h, window, dst_a, dst_b):
        _check(hip_lib().flow2d_median_2d_pair(self.handle, src_a.ptr, src_b.ptr, w, h, src_a.pitch, window, dst_a.ptr,
                                               dst_b.ptr), "flow2d_median_2d_pair")

    def add_median(self, src_a, add_a, w, h, window, dst_a, src_b=None, add_b=None, dst_b=None):
        """Median of (src + add), the sum formed on the fly; optional second plane set."""
        _check(hip_lib().flow2d_add_median_2d_pair(self.handle, src_a.ptr, add_a.ptr, src_b.ptr if src_b else None,
                                                   add_b.ptr if add_b else None, w, h, src_a.pitch, window, dst_a.ptr,
                                                   dst_b.ptr if dst_b else None), "flow2d_add_median_2d_pair")

    def add_median_half(self, src_a, add_a, w, h, window, dst_a, src_b=None, add_b=None, dst_b=None):
        """add_median with the src planes at half the size in both directions (read as [y >> 1][x >> 1])."""
        _check(hip_lib().flow2d_add_median_2d_pair_half(self.handle, src_a.ptr, add_a.ptr, src_b.ptr if src_b else None,
                                                        add_b.ptr if add_b else None, w, h, add_a.pitch, window, dst_a.ptr,
                                                        dst_b.ptr if dst_b else None), "flow2d_add_median_2d_pair_half")

    def resample_x_pair(self, src_a, dst_a, src_b, dst_b, out_w, out_h, in_w):
        _check(hip_lib().flow2d_resample_x_pair(self.handle, src_a.ptr, dst_a.ptr, src_b.ptr, dst_b.ptr, out_w, out_h,
                                                in_w, src_a.pitch), "flow2d_resample_x_pair")

    def resample_y_pair(self, src_a, dst_a, src_b, dst_b, out_w, out_h, in_h):
        _check(hip_lib().flow2d_resample_y_pair(self.handle, src_a.ptr, dst_a.ptr, src_b.ptr, dst_b.ptr, out_w, out_h,
                                                in_h, src_a.pitch), "flow2d_resample_y_pair")

    def compute_phi_ksi(self, f0, f1, u, v, du, dv, w, h, hx, hy, e_smooth, e_data, phi, ksi):
        _check(hip_lib().flow2d_compute_phi_ksi(self.handle, f0.ptr, f1.ptr, u.ptr, v.ptr, du.ptr, dv.ptr, w, h,
                                                f0.pitch, hx, hy, e_smooth, e_data, phi.ptr, ksi.ptr),
               "flow2d_compute_phi_ksi")

    def solve_sweep(self, f0, f1, u, v, du, dv, phi, ksi, w, h, hx, hy, alpha, tdu, tdv, constancy=GREY):
        fn = {GREY: hip_lib().flow2d_solve_2d, GRADIENT: hip_lib().flow2d_solve_2d_grad,
              GRADIENT_UNTILED: hip_lib().flow2d_solve_2d_grad_untiled,
              LOG_DERIVATIVES: hip_lib().flow2d_solve_2d_log}[constancy]
        _check(fn(self.handle, f0.ptr, f1.ptr, u.ptr, v.ptr, du.ptr, dv.ptr, phi.ptr, ksi.ptr, w, h, f0.pitch, hx, hy,
                  alpha, tdu.ptr, tdv.ptr), "flow2d_solve_2d*")

    def log_frame(self, src, dst, w, h):
        """dst = log(src + 1) over w x h as the log-derivative kernels form it (flow2d_log_frame_2d): for checkers"""
        _check(hip_lib().flow2d_log_frame_2d(self.handle, src.ptr, dst.ptr, w, h, src.pitch), "flow2d_log_frame_2d")

    def sor_iteration(self, f0, f1, u, v, du, dv, phi, ksi, w, h, hx, hy, alpha, omega, constancy=GREY):
        _check(hip_lib().flow2d_solve_2d_sor(self.handle, f0.ptr, f1.ptr, u.ptr, v.ptr, du.ptr, dv.ptr, phi.ptr, ksi.ptr,
                                             w, h, f0.pitch, hx, hy, alpha, omega, constancy), "flow2d_solve_2d_sor")

    def solve_level(self, f0, f1, u, v, du, dv, phi, ksi, tdu, tdv, w, h, hx, hy, alpha, e_smooth, e_data, outer,
                    inner, constancy=GREY, algorithm=SOLVER_AUTO, container_height=None, sor_omega=0.0, base_flow_shift=0):
        """Returns (du_plane, dv_plane) holding the result (the library owns the ping-pong)."""
        p = SolveParams(w, h, f0.pitch, container_height or f0.height, hx, hy, alpha, e_smooth, e_data, outer, inner,
                        constancy, algorithm, sor_omega, base_flow_shift)
        flag = C.c_int(0)
        _check(hip_lib().flow2d_solve_level(self.handle, f0.ptr, f1.ptr, u.ptr, v.ptr, du.ptr, dv.ptr, phi.ptr,
                                            ksi.ptr, tdu.ptr, tdv.ptr, C.byref(p), C.byref(flag)),
               "flow2d_solve_level")
        return (tdu, tdv) if flag.value else (du, dv)

    # -- timing -----------------------------------------------------------------------------------
    def timing_enable(self, mode=1):
        _check(hip_lib().flow2d_timing_enable(self.handle, int(mode)), "flow2d_timing_enable")

    def timing_records(self):
        n = C.c_size_t()
        _check(hip_lib().flow2d_timing_count(self.handle, C.byref(n)), "flow2d_timing_count")
        out = []
        for k in range(n.value):
            r = TimingRecord()
            _check(hip_lib().flow2d_timing_get(self.handle, k, C.byref(r)), "flow2d_timing_get")
            out.append(r)
        return out

    def timing_reset(self):
        _check(hip_lib().flow2d_timing_reset(self.handle), "flow2d_timing_reset")


# ---- C++ host layer (OpticalFlow2D & friends) through its C facade ---------------------------------

class HostParams(C.Structure):
    _fields_ = [
        ("warp_levels_count", C.c_size_t), ("warp_scale_factor", C.c_float),
        ("outer_iterations_count", C.c_size_t), ("inner_iterations_count", C.c_size_t),
        ("equation_alpha", C.c_float), ("equation_smoothness", C.c_float), ("equation_data", C.c_float),
        ("median_radius", C.c_size_t), ("gaussian_sigma", C.c_float), ("solver_algorithm", C.c_int),
        ("sor_omega", C.c_float),
    ]


class HostSettings(C.Structure):
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int), ("medianRadius", C.c_int), ("iterInner", C.c_int),
        ("iterOuter", C.c_int), ("levels", C.c_int), ("press_key", C.c_int),
        ("sigma", C.c_float), ("alpha", C.c_float), ("e_smooth", C.c_float), ("e_data", C.c_float),
        ("warpScale", C.c_float),
        ("inputPath", C.c_char * 512), ("outputPath", C.c_char * 512), ("fileName1", C.c_char * 256),
        ("fileName2", C.c_char * 256), ("imageType", C.c_char * 32), ("dataConstancy", C.c_char * 32),
    ]


_host = None


def host_lib():
    """The C++ host layer.  Raises if it has not been built."""
    global _host
    if _host is None:
        hip_lib()
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError("%s is missing: run __graft_entry__.build()" % HOST_LIB_PATH)
        L = C.CDLL(HOST_LIB_PATH)
        vp, sz, f, i = C.c_void_p, C.c_size_t, C.c_float, C.c_int
        fp = C.POINTER(C.c_float)
        L.flow2d_host_init_device.argtypes = [i]
        L.flow2d_host_adopt_context.argtypes = [vp]
        L.flow2d_host_context.restype = vp
        L.flow2d_host_flow_create.restype = vp
        L.flow2d_host_flow_create.argtypes = [sz, sz, i, i, i]
        L.flow2d_host_flow_destroy.argtypes = [vp]
        L.flow2d_host_flow_pitch.restype = sz
        L.flow2d_host_flow_pitch.argtypes = [vp]
        L.flow2d_host_max_warp_level.restype = sz
        L.flow2d_host_max_warp_level.argtypes = [vp, sz, sz, f]
        L.flow2d_host_compute_flow.argtypes = [vp, fp, fp, fp, fp, C.POINTER(HostParams), fp]
        L.flow2d_host_compute_flow_device.argtypes = [vp, vp, vp, vp, vp, C.POINTER(HostParams), i]
        L.flow2d_host_compute_flow_sequence_device.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(vp),
                                                               C.POINTER(HostParams)]
        L.flow2d_host_compute_flow_bidirectional.argtypes = [vp, fp, fp, fp, fp, fp, fp, fp, fp, C.POINTER(HostParams), f, f,
                                                             fp]
        L.flow2d_host_compute_flow_bidirectional_device.argtypes = [vp, C.POINTER(vp), sz] + [C.POINTER(vp)] * 6 + [
            C.POINTER(HostParams), f, f]
        L.flow2d_host_interpolate_frames.argtypes = [vp, fp, fp, fp, sz, fp, C.POINTER(HostParams), i, f, i, fp]
        L.flow2d_host_interpolate_frames_device.argtypes = [vp, C.POINTER(vp), sz, fp, sz, C.POINTER(vp), C.POINTER(HostParams),
                                                            i, f, i]
        if hasattr(L, "flow2d_host_track_points"):
            ull = C.POINTER(C.c_ulonglong)
            L.flow2d_host_track_points.argtypes = [vp, fp, sz, sz, f, i, f, f, fp, fp, sz, ull, C.POINTER(HostParams), f, f, fp]
            L.flow2d_host_track_points_device.argtypes = [vp, C.POINTER(vp), sz, sz, f, i, f, f, C.POINTER(vp), C.POINTER(vp), sz,
                                                          ull, C.POINTER(HostParams), f, f]
        if hasattr(L, "flow2d_host_denoise_sequence"):
            L.flow2d_host_denoise_args_ok.argtypes = [sz, sz, f]
            L.flow2d_host_denoise_sequence.argtypes = [vp, fp, sz, sz, f, i, fp, fp, C.POINTER(HostParams), fp]
            L.flow2d_host_denoise_sequence_device.argtypes = [vp, C.POINTER(vp), sz, sz, f, i, C.POINTER(vp), C.POINTER(vp),
                                                              C.POINTER(HostParams)]
        if hasattr(L, "flow2d_host_stabilise_sequence"):
            d, gm = C.c_double, C.POINTER(GlobalMotion)
            L.flow2d_host_global_motion_args_ok.argtypes = [i, d, i]
            L.flow2d_host_compose_global_motion.argtypes = [gm, gm, gm]
            L.flow2d_host_estimate_global_motion.argtypes = [vp, fp, fp, i, d, i, i, gm, C.POINTER(HostParams), fp, fp, fp, fp, fp]
            L.flow2d_host_estimate_global_motion_device.argtypes = [vp, vp, vp, i, d, i, i, gm, C.POINTER(HostParams), vp, vp, vp,
                                                                    vp]
            L.flow2d_host_stabilise_sequence.argtypes = [vp, fp, sz, sz, i, d, i, i, f, fp, gm, C.POINTER(HostParams), fp]
            L.flow2d_host_stabilise_sequence_device.argtypes = [vp, C.POINTER(vp), sz, sz, i, d, i, i, f, C.POINTER(vp), gm,
                                                                C.POINTER(HostParams)]
        if hasattr(L, "flow2d_host_analyse_deformation"):
            L.flow2d_host_deformation_args_ok.argtypes = [i, f]
            L.flow2d_host_analyse_deformation.argtypes = [vp, fp, fp, i, f, i, C.POINTER(fp), C.POINTER(DeformationStats),
                                                          C.POINTER(HostParams), fp, fp, fp]
            L.flow2d_host_analyse_deformation_device.argtypes = [vp, vp, vp, i, f, i, C.POINTER(vp), C.POINTER(DeformationStats),
                                                                 C.POINTER(HostParams), vp, vp, vp]
        if hasattr(L, "flow2d_host_refine_flow"):
            rr = C.POINTER(RefineRecord)
            L.flow2d_host_refine_args_ok.argtypes = [i, f, f, i]
            L.flow2d_host_refine_flow.argtypes = [vp, fp, fp, i, f, f, i, i, fp, fp, rr, C.POINTER(HostParams), fp, fp, fp]
            L.flow2d_host_refine_flow_device.argtypes = [vp, vp, vp, i, f, f, i, i, vp, vp, rr, C.POINTER(HostParams), vp, vp, vp, i]
        if hasattr(L, "flow2d_host_correlate_multipass_device"):
            ip, rp = C.POINTER(C.c_int), C.POINTER(CorrelationPassReport)
            L.flow2d_host_correlation_passes_ok.argtypes = [sz, sz, f, f, ip, i, f, f, f, i]
            L.flow2d_host_correlate_multipass_device.argtypes = [vp, vp, vp, f, f, ip, i, f, f, f, i, i, i, vp, vp, vp, vp, vp, rp, vp, vp]
            L.flow2d_host_correlate_multipass.argtypes = [vp, fp, fp, ip, i, f, f, f, i, i, i, fp, fp, fp, fp, fp, rp, fp, fp, fp]
        if hasattr(L, "flow2d_host_correlate_subset_device"):
            rp, sr, st, so = C.POINTER(CorrelationPassReport), C.POINTER(SubsetRecord), C.POINTER(SequenceStepReport), C.POINTER(SubsetOptions)
            pvp, fpp = C.POINTER(vp), C.POINTER(fp)
            passes = [C.POINTER(C.c_int), i, f, f, f, i]  # the schedule, min_score, threshold, epsilon, min_neighbours
            sequence = [i, i, i, f]  # fill, min_state, predict_neighbours, sequence_max_shift
            L.flow2d_host_subset_options_ok.argtypes = [so]
            L.flow2d_host_subset_min_pixels.argtypes = [i]
            L.flow2d_host_subset_interpolation_ok.argtypes = [i]
            L.flow2d_host_set_subset_interpolation.argtypes = [vp, i]
        if hasattr(L, "flow2d_host_correlate_multipass_masked_device"):  # (absent from libraries of earlier rounds loaded for an A/B)
            ip, rp = C.POINTER(C.c_int), C.POINTER(CorrelationPassReport)
            L.flow2d_host_correlation_passes_masked_ok.argtypes = [sz, sz, f, f, ip, i, f, f, f, i, i]
            L.flow2d_host_correlate_multipass_masked_device.argtypes = [vp, vp, vp, f, f, ip, i, f, f, f, i, i, i, vp, i, vp, vp, vp, vp, vp, rp,
                                                                        vp, vp]
            L.flow2d_host_correlate_multipass_masked.argtypes = [vp, fp, fp, ip, i, f, f, f, i, i, i, fp, i, fp, fp, fp, fp, fp, rp, fp, fp, fp]
            L.flow2d_host_set_subset_mask_search.argtypes = [vp, i]
            L.flow2d_host_subset_mask_search_ok.argtypes = [C.POINTER(SubsetOptions)]
            L.flow2d_host_sequence_options_ok.argtypes = sequence
            L.flow2d_host_refine_nodes_device.argtypes = [vp, vp, vp, vp, vp, i, i, so, pvp, sr]
            L.flow2d_host_refine_nodes_from_device.argtypes = [vp, vp, vp, pvp, i, i, so, pvp, sr]
            L.flow2d_host_correlate_subset_device.argtypes = [vp, vp, vp, f, f] + passes + [so, vp, vp, pvp, rp, sr, vp, vp]
            L.flow2d_host_correlate_subset.argtypes = [vp, fp, fp] + passes + [so, fp, fp, fpp, rp, sr, fp, fp, fp]
            L.flow2d_host_correlate_subset_sequence_device.argtypes = [vp, pvp, i, f, f] + passes + [so] + sequence + [pvp, rp, st, pvp]
            L.flow2d_host_correlate_subset_sequence.argtypes = [vp, fpp, i] + passes + [so] + sequence + [fpp, rp, st, fpp, fp]
        if hasattr(L, "flow2d_host_compose_nodes_device"):
            cp = C.POINTER(ComposeRecord)
            L.flow2d_host_set_reference_every.argtypes = [vp, i]
            L.flow2d_host_compose_records.argtypes = [vp, cp, i]
            L.flow2d_host_compose_nodes_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, i, C.POINTER(vp), cp]
            L.flow2d_host_compose_nodes.argtypes = [vp, C.POINTER(fp), C.POINTER(fp), i, i, i, C.POINTER(fp), cp]
        if hasattr(L, "flow2d_host_node_uncertainty_device"):
            ur = C.POINTER(UncertaintyRecord)
            L.flow2d_host_uncertainty_options_ok.argtypes = [so, i]
            L.flow2d_host_node_uncertainty_device.argtypes = [vp, vp, vp, C.POINTER(vp), i, i, so, i, C.POINTER(vp), ur]
            L.flow2d_host_node_uncertainty.argtypes = [vp, fp, fp, C.POINTER(fp), i, i, so, i, C.POINTER(fp), ur]
        if hasattr(L, "flow2d_host_node_strain_device"):
            ds = C.POINTER(DeformationStats)
            L.flow2d_host_strain_options_ok.argtypes = [i, i, i, i, i]
            L.flow2d_host_node_strain_device.argtypes = [vp, C.POINTER(vp), i, sz, sz, i, i, i, i, i, i, C.POINTER(vp), ds]
            L.flow2d_host_node_strain.argtypes = [vp, C.POINTER(fp), i, sz, sz, i, i, i, i, i, i, C.POINTER(fp), ds]
        if hasattr(L, "flow2d_host_set_strain_robust"):
            L.flow2d_host_strain_robust_options_ok.argtypes = [i, i, i, i, i, C.c_float, i]
            L.flow2d_host_set_strain_robust.argtypes = [vp, C.c_float, i]
            L.flow2d_host_set_strain_diagnostics.argtypes = [vp, C.POINTER(vp), i]
        if hasattr(L, "flow2d_host_set_strain_weighting"):
            L.flow2d_host_strain_weighted_options_ok.argtypes = [i, i, i, i, i, C.c_float, C.c_float, C.c_float, i]
            L.flow2d_host_set_strain_weighting.argtypes = [vp, i, C.c_float, C.c_float, i]
            L.flow2d_host_node_strain_weighted_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, sz, sz, i, i, i, i, i, i,
                                                                  C.POINTER(vp), C.POINTER(vp), ds]
            L.flow2d_host_node_strain_weighted.argtypes = [vp, C.POINTER(fp), C.POINTER(fp), i, sz, sz, i, i, i, i, i, i, C.POINTER(fp),
                                                           C.POINTER(fp), ds]
        if hasattr(L, "flow2d_host_correlate"):
            cr = C.POINTER(CorrelationRecord)
            L.flow2d_host_correlation_args_ok.argtypes = [sz, sz, f, f, i, i, i, f]
            L.flow2d_host_correlate.argtypes = [vp, fp, fp, i, i, i, f, fp, fp, fp, cr, fp, fp, fp]
            L.flow2d_host_correlate_device.argtypes = [vp, vp, vp, f, f, i, i, i, f, vp, vp, vp, cr, vp, vp]
        if hasattr(L, "flow2d_host_compute_flow_from_prior"):
            cr, pr, hp = C.POINTER(CorrelationRecord), C.POINTER(PriorReport), C.POINTER(HostParams)
            L.flow2d_host_prior_start_level.argtypes = [sz, sz, sz, f, f, i, C.POINTER(sz)]
            L.flow2d_host_compute_flow_from_prior_device.argtypes = [vp] * 7 + [hp, f, i, pr]
            L.flow2d_host_compute_flow_from_prior.argtypes = [vp, fp, fp, fp, fp, fp, fp, hp, f, i, pr, fp]
            L.flow2d_host_compute_flow_correlation_seeded_device.argtypes = [vp, vp, vp, f, f, i, i, i, f, vp, vp, hp, f, i, vp, vp, vp, cr,
                                                                             pr, vp, vp]
            L.flow2d_host_compute_flow_correlation_seeded.argtypes = [vp, fp, fp, i, i, i, f, fp, fp, hp, f, i, fp, fp, fp, cr, pr, fp, fp,
                                                                      fp, fp]
            L.flow2d_host_bidirectional_refuses_prior.argtypes = [vp, hp]
            L.flow2d_host_flow_create_group.restype = vp
            L.flow2d_host_flow_create_group.argtypes = [sz, sz, i, sz]
        if hasattr(L, "flow2d_host_compute_flow_sequence_warm"):
            hp, wo, wr = C.POINTER(HostParams), C.POINTER(WarmOptions), C.POINTER(WarmReport)
            L.flow2d_host_warm_next_reach.argtypes = [C.c_ulonglong, C.POINTER(C.c_ulonglong), f, i, C.POINTER(i), C.POINTER(i)]
            L.flow2d_host_warm_options_ok.argtypes = [wo]
            L.flow2d_host_propagate_flow_device.argtypes = [vp] * 6 + [f, wo, vp, vp, C.POINTER(PropagateRecord)]
            L.flow2d_host_compute_flow_from_previous_device.argtypes = [vp] * 9 + [hp, f, i, wo, wr]
            L.flow2d_host_compute_flow_from_previous.argtypes = [vp] + [fp] * 8 + [hp, f, i, wo, wr, fp]
            L.flow2d_host_compute_flow_sequence_warm_device.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(vp), C.POINTER(vp), hp, f, i, wo,
                                                                        wr]
            L.flow2d_host_compute_flow_sequence_warm.argtypes = [vp, fp, sz, fp, fp, hp, f, i, wo, wr, fp]
        if hasattr(L, "flow2d_host_segment_motion"):
            d, u32 = C.c_double, C.c_uint
            head = [i, d, i, i, f, f, u32, C.POINTER(GlobalMotion), C.POINTER(SegmentSummary), C.POINTER(MotionRegion),
                    C.POINTER(HostParams)]
            L.flow2d_host_segment_motion_args_ok.argtypes = [f, f, u32]
            L.flow2d_host_segment_max_regions.restype = sz
            L.flow2d_host_segment_motion.argtypes = [vp, fp, fp] + head + [C.POINTER(C.c_int), fp, fp]
            L.flow2d_host_segment_motion_device.argtypes = [vp, vp, vp] + head + [vp, vp, vp]
        L.flow2d_host_read_flo.argtypes = [C.c_char_p, C.POINTER(sz), C.POINTER(sz), fp, fp, sz]
        L.flow2d_host_write_flo.argtypes = [fp, fp, sz, sz, C.c_char_p]
        L.flow2d_host_flow_error.argtypes = [fp] * 5 + [sz, sz, fp, fp, C.POINTER(FlowErrorStats)]
        L.flow2d_host_level_timings.restype = sz
        L.flow2d_host_level_timings.argtypes = [vp, fp, sz]
        L.flow2d_host_reset_timings.argtypes = [vp]
        L.flow2d_host_use_graph.argtypes = [vp, i]
        L.flow2d_host_missing_key_leaves_outputs.argtypes = [vp, C.c_char_p]
        L.flow2d_host_read_raw.argtypes = [C.c_char_p, sz, sz, i, fp]
        L.flow2d_host_write_outputs.argtypes = [fp, fp, sz, sz, C.c_char_p, C.c_char_p, f]
        L.flow2d_host_write_raw.argtypes = [fp, sz, sz, i, C.c_char_p]
        L.flow2d_host_max_warp_level_static.restype = sz
        L.flow2d_host_max_warp_level_static.argtypes = [sz, sz, f]
        L.flow2d_host_convert_to_rgb.argtypes = [f, f, C.POINTER(i)]
        L.flow2d_host_load_settings.argtypes = [C.c_char_p, C.POINTER(HostSettings)]
        L.flow2d_host_operator_create.restype = vp
        L.flow2d_host_operator_create.argtypes = [C.c_char_p, sz, sz, sz, i, i]
        L.flow2d_host_operator_name.restype = C.c_char_p
        L.flow2d_host_operator_name.argtypes = [vp]
        L.flow2d_host_operator_execute.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(vp), sz]
        L.flow2d_host_operator_destroy.argtypes = [vp]
        L.flow2d_host_batch_create.restype = vp
        L.flow2d_host_batch_create.argtypes = [sz, sz, i, sz, i, sz]
        L.flow2d_host_batch_group_stride.restype = sz
        L.flow2d_host_batch_group_stride.argtypes = [vp]
        L.flow2d_host_batch_destroy.argtypes = [vp]
        L.flow2d_host_batch_pitch.restype = sz
        L.flow2d_host_batch_pitch.argtypes = [vp]
        L.flow2d_host_batch_lanes.restype = sz
        L.flow2d_host_batch_lanes.argtypes = [vp]
        L.flow2d_host_batch_lane_context.restype = vp
        L.flow2d_host_batch_lane_context.argtypes = [vp, sz]
        L.flow2d_host_batch_use_graph.argtypes = [vp, i]
        L.flow2d_host_batch_compute.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                C.POINTER(HostParams), sz]
        L.flow2d_host_batch_synchronize.argtypes = [vp]
        L.flow2d_host_batch_compute_grouped.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                        C.POINTER(HostParams), sz]
        L.flow2d_host_data2d_create.restype = vp
        L.flow2d_host_data2d_create.argtypes = [sz, sz, i]
        L.flow2d_host_data2d_destroy.argtypes = [vp]
        L.flow2d_host_use_pinned_memory.argtypes = [i]
        L.flow2d_host_data2d_ptr.restype = vp
        L.flow2d_host_data2d_ptr.argtypes = [vp]
        L.flow2d_host_data2d_is_pinned.argtypes = [vp]
        L.flow2d_host_batch_compute_host.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                     C.POINTER(HostParams), sz]
        _host = L
    return _host


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _opt_fptr(a):
    """_fptr of an optional array: None (a null pointer) for None."""
    return None if a is None else _fptr(a)


def _ptr_array(q):
    """A list of device addresses as a void* array: None (a null pointer) for None."""
    return None if q is None else (C.c_void_p * max(len(q), 1))(*q)


class OpticalFlow:
    """OpticalFlow2D of the host layer (Initialize / ComputeFlow / ComputeFlowDevice / Destroy)."""

    def __init__(self, width, height, constancy=GREY, device=0, ctx=None, silent=True, lone=True, group_size=1):
        """group_size > 1: an object initialised for lock-step groups (OpticalFlow2D::group_size; every device plane it is handed is
        then group_size containers tall)."""
        L = host_lib()
        self._adopted = ctx is not None
        if ctx is not None:
            L.flow2d_host_adopt_context(ctx.handle)
        elif L.flow2d_host_init_device(device) != 0:
            raise Flow2DError(2, "InitDeviceContext")
        self.width, self.height = width, height
        if group_size > 1:
            self.handle = L.flow2d_host_flow_create_group(width, height, _HOST_CONSTANCY[constancy], int(group_size))
        else:
            self.handle = L.flow2d_host_flow_create(width, height, _HOST_CONSTANCY[constancy], int(silent), int(bool(lone)))
        if not self.handle:
            if self._adopted:
                L.flow2d_host_adopt_context(None)
            raise Flow2DError(1, "OpticalFlow2D::Initialize")
        self.pitch = L.flow2d_host_flow_pitch(self.handle)

    @staticmethod
    def params(levels, scale, outer, inner, alpha, e_smooth, e_data, median_radius, sigma, algorithm=SOLVER_AUTO,
               sor_omega=0.0):
        return HostParams(levels, scale, outer, inner, alpha, e_smooth, e_data, median_radius, sigma, algorithm,
                          sor_omega)

    def _pair(self, frame_0, frame_1):
        """Both frames as contiguous float32 arrays; ValueError unless each is [height, width]."""
        f0, f1 = (np.ascontiguousarray(a, np.float32) for a in (frame_0, frame_1))
        if f0.shape != (self.height, self.width) or f1.shape != f0.shape:
            raise ValueError("frames: [%d, %d]" % (self.height, self.width))
        return f0, f1

    def _stack(self, frames):
        """A sequence as one contiguous float32 array; ValueError unless it is [frame_count, height, width]."""
        fr = np.ascontiguousarray(frames, np.float32)
        if fr.ndim != 3 or fr.shape[1:] != (self.height, self.width):
            raise ValueError("frames: [frame_count, %d, %d]" % (self.height, self.width))
        return fr

    def max_warp_level(self, width, height, scale):
        return host_lib().flow2d_host_max_warp_level(self.handle, width, height, scale)

    def compute_flow(self, frame_0, frame_1, params):
        """Host images in, host flow out (upload + pyramid + download).  Returns (u, v, device_ms)."""
        f0 = np.ascontiguousarray(frame_0, np.float32)
        f1 = np.ascontiguousarray(frame_1, np.float32)
        assert f0.shape == (self.height, self.width) and f1.shape == f0.shape
        u = np.empty_like(f0)
        v = np.empty_like(f0)
        ms = C.c_float()
        rc = host_lib().flow2d_host_compute_flow(self.handle, _fptr(f0), _fptr(f1), _fptr(u), _fptr(v),
                                                 C.byref(params), C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlow")
        return u, v, ms.value

    def compute_flow_device(self, dev_f0, dev_f1, dev_u, dev_v, params, timing_mode=0):
        """Device-resident pair (raw device addresses of pitched containers); queued, not synchronised.
        timing_mode: 0 off, 1 events around each level's solve, 2 also around each solver-kernel launch."""
        rc = host_lib().flow2d_host_compute_flow_device(self.handle, dev_f0, dev_f1, dev_u, dev_v, C.byref(params),
                                                        int(timing_mode))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowDevice")

    def compute_flow_sequence_device(self, dev_frames, dev_us, dev_vs, params):
        """Flows of an image sequence: flow k goes from dev_frames[k] to dev_frames[k + 1] into (dev_us[k], dev_vs[k]).
        Every frame's blurred plane and pyramid levels are computed once.  Queued, not synchronised."""
        n = len(dev_frames)
        if n < 2 or len(dev_us) != n - 1 or len(dev_vs) != n - 1:
            raise ValueError("a sequence of n frames takes n - 1 flow plane pairs")
        rc = host_lib().flow2d_host_compute_flow_sequence_device(self.handle, _ptr_array(dev_frames), n, _ptr_array(dev_us),
                                                                 _ptr_array(dev_vs), C.byref(params))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowSequenceDevice")

    def compute_flow_bidirectional(self, frame_0, frame_1, params, alpha1=0.01, alpha2=0.5):
        """OpticalFlow2D::ComputeFlowBidirectional: host images in; the forward flow (that of compute_flow), the backward flow
        frame_1 -> frame_0 and the occlusion masks of frame_0 and frame_1 (1.0 = inconsistent) out.
        Returns (u, v, back_u, back_v, occ_0, occ_1, device_ms)."""
        f0 = np.ascontiguousarray(frame_0, np.float32)
        f1 = np.ascontiguousarray(frame_1, np.float32)
        assert f0.shape == (self.height, self.width) and f1.shape == f0.shape
        out = [np.empty_like(f0) for _ in range(6)]
        ms = C.c_float()
        rc = host_lib().flow2d_host_compute_flow_bidirectional(self.handle, _fptr(f0), _fptr(f1), *[_fptr(a) for a in out],
                                                               C.byref(params), alpha1, alpha2, C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowBidirectional")
        return tuple(out) + (ms.value,)

    def compute_flow_bidirectional_device(self, dev_frames, dev_us, dev_vs, dev_back_us, dev_back_vs, params, dev_occ_fwd=None,
                                          dev_occ_bwd=None, alpha1=0.01, alpha2=0.5):
        """Forward flow k (dev_frames[k] -> dev_frames[k + 1]) into (dev_us[k], dev_vs[k]), backward flow k (dev_frames[k + 1] ->
        dev_frames[k]) into (dev_back_us[k], dev_back_vs[k]) and, when given, the occlusion masks of frame k (dev_occ_fwd[k])
        and frame k + 1 (dev_occ_bwd[k]).  Every frame's pyramid is built once.  Queued, not synchronised."""
        n = len(dev_frames)
        lists = [dev_us, dev_vs, dev_back_us, dev_back_vs] + [q for q in (dev_occ_fwd, dev_occ_bwd) if q is not None]
        if n < 2 or any(len(q) != n - 1 for q in lists):
            raise ValueError("a sequence of n frames takes n - 1 planes in every output list")
        planes = [_ptr_array(q) for q in (dev_us, dev_vs, dev_back_us, dev_back_vs, dev_occ_fwd, dev_occ_bwd)]
        rc = host_lib().flow2d_host_compute_flow_bidirectional_device(self.handle, _ptr_array(dev_frames), n, *planes,
                                                                      C.byref(params), alpha1, alpha2)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowBidirectionalDevice")

    def interpolate_frames(self, frame_0, frame_1, params, times, iterations=2, max_residual=0.5, masks=True):
        """OpticalFlow2D::InterpolateFrames: host images in; the frames at `times` (each 0 <= t <= 1) between them out, from both
        flows of compute_flow_bidirectional and, with masks, both occlusion masks (flow2d_interpolate_2d).
        Returns (frames, device_ms): frames[j] is the frame at times[j]."""
        f0 = np.ascontiguousarray(frame_0, np.float32)
        f1 = np.ascontiguousarray(frame_1, np.float32)
        assert f0.shape == (self.height, self.width) and f1.shape == f0.shape
        ts = np.ascontiguousarray(np.atleast_1d(times), np.float32)
        out = np.empty((len(ts),) + f0.shape, np.float32)
        ms = C.c_float()
        rc = host_lib().flow2d_host_interpolate_frames(self.handle, _fptr(f0), _fptr(f1), _fptr(ts), len(ts), _fptr(out),
                                                       C.byref(params), int(iterations), max_residual, int(bool(masks)),
                                                       C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::InterpolateFrames")
        return out, ms.value

    def interpolate_frames_device(self, dev_frames, times, dev_outputs, params, iterations=2, max_residual=0.5, masks=True):
        """The frames at `times` between every consecutive pair of dev_frames: dev_outputs[k * len(times) + j] gets the frame at
        times[j] between dev_frames[k] and dev_frames[k + 1].  Queued, not synchronised."""
        n = len(dev_frames)
        ts = np.ascontiguousarray(np.atleast_1d(times), np.float32)
        if n < 2 or len(ts) < 1 or len(dev_outputs) != (n - 1) * len(ts):
            raise ValueError("n frames and m times take (n - 1) * m output planes")
        rc = host_lib().flow2d_host_interpolate_frames_device(self.handle, _ptr_array(dev_frames), n, _fptr(ts), len(ts),
                                                              _ptr_array(dev_outputs), C.byref(params), int(iterations),
                                                              max_residual, int(bool(masks)))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::InterpolateFramesDevice")

    def track_points(self, frames, params, spacing=4, min_eigenvalue=DEFAULT_MIN_EIGENVALUE, boundaries=True, capacity=None,
                     alpha1=0.01, alpha2=0.5, beta1=0.01, beta2=0.002):
        """OpticalFlow2D::TrackPoints: dense point trajectories through the host frames `frames` ([frame_count, h, w]).  Frame
        0 is seeded on a grid of `spacing`, every track is carried by the forward flow and ends at an occlusion
        (forward-backward check at its sub-pixel position, alpha1 / alpha2), at a motion boundary (boundaries, beta1 / beta2)
        or where it leaves the frame, and uncovered cells of every later frame get new tracks.  min_eigenvalue is the seeding
        threshold on the smaller eigenvalue of the 5x5 structure tensor: unnormalised sums of grey-level gradients, so it is
        scale-dependent (the default keeps the analytic scenes' textures; 0 seeds every uncovered cell).  capacity: the table
        size (default: every cell of every frame).  Returns (xs, ys): float32 [frame_count, N], N the final track count; NaN
        where a track has not started or has ended."""
        fr = np.ascontiguousarray(frames, np.float32)
        assert fr.ndim == 3 and fr.shape[1:] == (self.height, self.width) and fr.shape[0] >= 2
        n = fr.shape[0]
        if capacity is None:
            capacity = n * (-(-self.width // spacing)) * (-(-self.height // spacing))
        xs = np.empty((n, capacity), np.float32)
        ys = np.empty((n, capacity), np.float32)
        counts = (C.c_ulonglong * n)()
        ms = C.c_float()
        rc = host_lib().flow2d_host_track_points(self.handle, _fptr(fr), n, spacing, min_eigenvalue, int(bool(boundaries)), beta1,
                                                 beta2, _fptr(xs), _fptr(ys), capacity, counts, C.byref(params), alpha1, alpha2,
                                                 C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::TrackPoints")
        last = int(counts[n - 1])
        return xs[:, :last].copy(), ys[:, :last].copy()

    def track_points_device(self, dev_frames, dev_xs, dev_ys, capacity, params, spacing=4,
                            min_eigenvalue=DEFAULT_MIN_EIGENVALUE, boundaries=True, alpha1=0.01, alpha2=0.5, beta1=0.01,
                            beta2=0.002):
        """OpticalFlow2D::TrackPointsDevice: device frames in, the track table of frame k into (dev_xs[k], dev_ys[k]) (device
        addresses of `capacity` floats each).  Returns the track count after each frame's seeding (synchronises once)."""
        n = len(dev_frames)
        if n < 2 or len(dev_xs) != n or len(dev_ys) != n:
            raise ValueError("n frames take n x and n y tables")
        counts = (C.c_ulonglong * n)()
        rc = host_lib().flow2d_host_track_points_device(self.handle, _ptr_array(dev_frames), n, spacing, min_eigenvalue,
                                                        int(bool(boundaries)), beta1, beta2, _ptr_array(dev_xs),
                                                        _ptr_array(dev_ys), capacity, counts, C.byref(params), alpha1, alpha2)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::TrackPointsDevice")
        return [int(c) for c in counts]

    def denoise_sequence(self, frames, params, radius=1, range_sigma=0.0, masks=True, weight_sums=False):
        """OpticalFlow2D::DenoiseSequence: motion-compensated temporal denoising of the host frames `frames` ([frame_count, h,
        w]).  Frame k is averaged with the frames k - radius .. k + radius that exist, each sampled along the flow from frame k
        (compute_flow_bidirectional on consecutive pairs, chained for distances of 2 and more), without what the occlusion masks
        mark (masks) and, with range_sigma > 0 (grey levels), weighted by sigma^2 / (sigma^2 + difference^2)
        (flow2d_denoise_2d).  Returns the fused frames [frame_count, h, w]; with weight_sums, (frames, sums of weights)."""
        fr = self._stack(frames)
        out = np.empty_like(fr)
        sums = np.empty_like(fr) if weight_sums else None
        ms = C.c_float()
        rc = host_lib().flow2d_host_denoise_sequence(self.handle, _fptr(fr), fr.shape[0], int(radius), range_sigma,
                                                     int(bool(masks)), _fptr(out), _opt_fptr(sums),
                                                     C.byref(params), C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::DenoiseSequence")
        return (out, sums) if weight_sums else out

    def denoise_sequence_device(self, dev_frames, dev_outputs, params, radius=1, range_sigma=0.0, masks=True,
                                dev_weight_sums=None):
        """OpticalFlow2D::DenoiseSequenceDevice: device frames in, frame k fused with its neighbours into dev_outputs[k] (and the
        sum of weights into dev_weight_sums[k], when given).  Queued, not synchronised."""
        n = len(dev_frames)
        if len(dev_outputs) != n or (dev_weight_sums is not None and len(dev_weight_sums) != n):
            raise ValueError("n frames take n output planes")
        rc = host_lib().flow2d_host_denoise_sequence_device(self.handle, _ptr_array(dev_frames), n, int(radius), range_sigma,
                                                            int(bool(masks)), _ptr_array(dev_outputs), _ptr_array(dev_weight_sums),
                                                            C.byref(params))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::DenoiseSequenceDevice")

    def estimate_global_motion(self, frame_0, frame_1, params, model=MOTION_AFFINE, sigma=0.5, iterations=5, masks=False,
                               flow=False, residual=False):
        """OpticalFlow2D::EstimateGlobalMotion: the global motion of the host pair -- the flow frame_0 -> frame_1 (with masks:
        through the bidirectional flow, the forward occlusion mask leaving its vectors out), `model` fitted by
        flow2d_global_motion_2d.  Returns the GlobalMotion record; with flow / residual, (record, (u, v) and / or (ru, rv))."""
        f0, f1 = self._pair(frame_0, frame_1)
        rec, ms = GlobalMotion(), C.c_float()
        fl = [np.empty_like(f0) for _ in range(2)] if flow else [None, None]
        rs = [np.empty_like(f0) for _ in range(2)] if residual else [None, None]
        rc = host_lib().flow2d_host_estimate_global_motion(self.handle, _fptr(f0), _fptr(f1), int(model), float(sigma),
                                                           int(iterations), int(bool(masks)), C.byref(rec), C.byref(params),
                                                           *[_opt_fptr(a) for a in fl + rs], C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::EstimateGlobalMotion")
        extra = ([tuple(fl)] if flow else []) + ([tuple(rs)] if residual else [])
        return (rec, *extra) if extra else rec

    def estimate_global_motion_device(self, dev_frame_0, dev_frame_1, params, model=MOTION_AFFINE, sigma=0.5, iterations=5,
                                      masks=False, dev_flow=None, dev_residual=None):
        """OpticalFlow2D::EstimateGlobalMotionDevice: two device frames in, the GlobalMotion record out (synchronises);
        dev_flow / dev_residual: optional (u, v) pairs of device planes for the flow and the residual flow."""
        rec = GlobalMotion()
        fl, rs = dev_flow or (None, None), dev_residual or (None, None)
        rc = host_lib().flow2d_host_estimate_global_motion_device(self.handle, dev_frame_0, dev_frame_1, int(model), float(sigma),
                                                                  int(iterations), int(bool(masks)), C.byref(rec),
                                                                  C.byref(params), fl[0], fl[1], rs[0], rs[1])
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::EstimateGlobalMotionDevice")
        return rec

    def segment_motion(self, frame_0, frame_1, params, model=MOTION_AFFINE, sigma=0.5, iterations=5, threshold=0.5,
                       join=float("inf"), min_area=16, masks=False, residual=False):
        """OpticalFlow2D::SegmentMotion: the independently moving regions of the host pair -- the flow frame_0 -> frame_1
        (bidirectional with masks, the forward occlusion mask leaving its pixels out), the global motion `model`, the residual
        flow and flow2d_segment_motion_2d on it.  Returns (GlobalMotion, SegmentSummary, [MotionRegion] -- the recorded ones --,
        labels [h, w] int32); with residual, also (ru, rv)."""
        f0, f1 = self._pair(frame_0, frame_1)
        H = host_lib()
        rec, summary = GlobalMotion(), SegmentSummary()
        regions = (MotionRegion * H.flow2d_host_segment_max_regions())()
        labels = np.empty(f0.shape, np.int32)
        rs = [np.empty_like(f0) for _ in range(2)] if residual else [None, None]
        rc = H.flow2d_host_segment_motion(self.handle, _fptr(f0), _fptr(f1), int(model), float(sigma), int(iterations),
                                          int(bool(masks)), float(threshold), float(join), int(min_area), C.byref(rec),
                                          C.byref(summary), regions, C.byref(params), labels.ctypes.data_as(C.POINTER(C.c_int)),
                                          _opt_fptr(rs[0]), _opt_fptr(rs[1]))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::SegmentMotion")
        out = (rec, summary, list(regions)[:summary.recorded], labels)
        return out + (tuple(rs),) if residual else out

    def segment_motion_device(self, dev_frame_0, dev_frame_1, params, model=MOTION_AFFINE, sigma=0.5, iterations=5, threshold=0.5,
                              join=float("inf"), min_area=16, masks=False, dev_labels=None, dev_residual=None):
        """OpticalFlow2D::SegmentMotionDevice: two device frames in; (GlobalMotion, SegmentSummary, [MotionRegion]) out
        (synchronises); dev_labels / dev_residual (a (u, v) pair): optional device planes for the labels and the residual flow."""
        H = host_lib()
        rec, summary = GlobalMotion(), SegmentSummary()
        regions = (MotionRegion * H.flow2d_host_segment_max_regions())()
        rs = dev_residual or (None, None)
        rc = H.flow2d_host_segment_motion_device(self.handle, dev_frame_0, dev_frame_1, int(model), float(sigma), int(iterations),
                                                 int(bool(masks)), float(threshold), float(join), int(min_area), C.byref(rec),
                                                 C.byref(summary), regions, C.byref(params), dev_labels, rs[0], rs[1])
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::SegmentMotionDevice")
        return rec, summary, list(regions)[:summary.recorded]

    def analyse_deformation(self, frame_0, frame_1, params, measure=STRAIN_SMALL, smoothing_sigma=0.0, masks=False,
                            planes=DEFORMATION_PLANES, flow=False):
        """OpticalFlow2D::AnalyseDeformation: how the material deforms between the host pair -- the flow frame_0 -> frame_1
        (bidirectional with masks, the forward occlusion mask then keeping differences from reaching across an occlusion
        boundary), a Gaussian of smoothing_sigma pixels over both flow planes when > 0, and flow2d_deformation_2d.  Returns
        ({name: [h, w] array} for the names of `planes`, DeformationStats); with flow, also the (u, v) that was analysed."""
        f0, f1 = self._pair(frame_0, frame_1)
        out = {name: np.empty_like(f0) for name in planes}
        fp = C.POINTER(C.c_float)
        table = (fp * 9)(*[_fptr(out[name]) if name in out else fp() for name in DEFORMATION_PLANES])
        uv = [np.empty_like(f0) for _ in range(2)] if flow else [None, None]
        stats = DeformationStats()
        rc = host_lib().flow2d_host_analyse_deformation(self.handle, _fptr(f0), _fptr(f1), int(measure), float(smoothing_sigma),
                                                        int(bool(masks)), table, C.byref(stats), C.byref(params),
                                                        _opt_fptr(uv[0]), _opt_fptr(uv[1]), None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::AnalyseDeformation")
        return (out, stats, tuple(uv)) if flow else (out, stats)

    def analyse_deformation_device(self, dev_frame_0, dev_frame_1, params, measure=STRAIN_SMALL, smoothing_sigma=0.0, masks=False,
                                   dev_planes=None, stats=True, dev_flow=None, dev_mask=None):
        """OpticalFlow2D::AnalyseDeformationDevice: two device frames in; dev_planes = {name: device address} of the planes
        wanted (names from DEFORMATION_PLANES), dev_flow (a (u, v) pair) and dev_mask: optional device planes for the flow that
        was analysed and the occlusion mask.  Returns the DeformationStats (None without stats); synchronises."""
        dev_planes = dev_planes or {}
        unknown = [name for name in dev_planes if name not in DEFORMATION_PLANES]
        if unknown:
            raise ValueError("deformation planes are %s, not %s" % (", ".join(DEFORMATION_PLANES), unknown))
        table = (C.c_void_p * 9)(*[dev_planes.get(name) for name in DEFORMATION_PLANES])
        record = DeformationStats() if stats else None
        fl = dev_flow or (None, None)
        rc = host_lib().flow2d_host_analyse_deformation_device(self.handle, dev_frame_0, dev_frame_1, int(measure),
                                                               float(smoothing_sigma), int(bool(masks)), table,
                                                               C.byref(record) if stats else None, C.byref(params), fl[0], fl[1],
                                                               dev_mask)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::AnalyseDeformationDevice")
        return record

    def refine_flow(self, frame_0, frame_1, params, radius=5, sigma_guide=25.0, sigma_space=0.0, iterations=1, masks=True,
                    flow=False):
        """OpticalFlow2D::RefineFlow: the flow frame_0 -> frame_1 of the host pair (bidirectional with masks) refined by
        `iterations` passes of flow2d_refine_flow_2d -- the weighted median over a (2 radius + 1)^2 window with frame_0 as the
        guide and, with masks, the forward occlusion mask taking unreliable vectors out.  Returns (u, v, RefineRecord of the last
        pass); with flow, also the (u, v) before the refinement."""
        f0, f1 = self._pair(frame_0, frame_1)
        u, v = np.empty_like(f0), np.empty_like(f0)
        uv = [np.empty_like(f0) for _ in range(2)] if flow else [None, None]
        record = RefineRecord()
        rc = host_lib().flow2d_host_refine_flow(self.handle, _fptr(f0), _fptr(f1), int(radius), float(sigma_guide), float(sigma_space),
                                                int(iterations), int(bool(masks)), _fptr(u), _fptr(v), C.byref(record),
                                                C.byref(params), _opt_fptr(uv[0]), _opt_fptr(uv[1]), None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::RefineFlow")
        return (u, v, record, tuple(uv)) if flow else (u, v, record)

    def refine_flow_device(self, dev_frame_0, dev_frame_1, dev_refined, params, radius=5, sigma_guide=25.0, sigma_space=0.0,
                           iterations=1, masks=True, dev_flow=None, dev_mask=None, flow_given=False, record=True):
        """OpticalFlow2D::RefineFlowDevice: device frames in, dev_refined (a (u, v) pair of device planes) out.  dev_flow (a
        (u, v) pair) and dev_mask: optional device planes that get the flow before the refinement and the occlusion mask -- or,
        with flow_given, that hold the flow to refine and (optionally) its mask, computed elsewhere (dev_frame_1 may then be
        None).  Returns the RefineRecord of the last pass (None without record); synchronises."""
        rec = RefineRecord() if record else None
        fl = dev_flow or (None, None)
        rc = host_lib().flow2d_host_refine_flow_device(self.handle, dev_frame_0, dev_frame_1, int(radius), float(sigma_guide),
                                                       float(sigma_space), int(iterations), int(bool(masks)), dev_refined[0],
                                                       dev_refined[1], C.byref(rec) if record else None, C.byref(params), fl[0], fl[1],
                                                       dev_mask, int(bool(flow_given)))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::RefineFlowDevice")
        return rec

    def correlate(self, frame_0, frame_1, radius=7, search=8, spacing=8, min_score=-1.0, flow=False):
        """OpticalFlow2D::Correlate: window correlation of the host pair (flow2d_correlate_2d; no part of the variational flow).  The
        frames are quantised to 8 bits over their common finite range -- as they are when that lies in [0, 255].  Returns (node_u,
        node_v, node_score, CorrelationRecord, (lo, scale)) on the grid correlation_grid(width, height, radius, spacing); with flow,
        also the (u, v) of the field expanded to the frame's grid."""
        f0, f1 = self._pair(frame_0, frame_1)
        nw, nh = correlation_grid(self.width, self.height, radius, spacing)
        nodes = [np.empty((nh, nw), np.float32) for _ in range(3)]
        uv = [np.empty_like(f0) for _ in range(2)] if flow else [None, None]
        record = CorrelationRecord()
        lo_scale = (C.c_float * 2)()
        rc = host_lib().flow2d_host_correlate(self.handle, _fptr(f0), _fptr(f1), int(radius), int(search), int(spacing), float(min_score),
                                              _fptr(nodes[0]), _fptr(nodes[1]), _fptr(nodes[2]), C.byref(record), _opt_fptr(uv[0]),
                                              _opt_fptr(uv[1]), lo_scale)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::Correlate")
        out = (nodes[0], nodes[1], nodes[2], record, (lo_scale[0], lo_scale[1]))
        return out + (tuple(uv),) if flow else out

    def correlate_device(self, dev_frame_0, dev_frame_1, lo, scale, radius=7, search=8, spacing=8, min_score=-1.0, dev_nodes=None,
                         dev_score=None, dev_flow=None, record=True):
        """OpticalFlow2D::CorrelateDevice: device frames in.  dev_nodes (a (u, v) pair) and dev_score: optional device planes of the
        container's size whose first nw x nh floats get the node field; dev_flow (a (u, v) pair, optional) gets the field expanded
        to the frame's grid.  Returns the CorrelationRecord (None without record); synchronises."""
        rec = CorrelationRecord() if record else None
        nd, fl = dev_nodes or (None, None), dev_flow or (None, None)
        rc = host_lib().flow2d_host_correlate_device(self.handle, dev_frame_0, dev_frame_1, float(lo), float(scale), int(radius),
                                                     int(search), int(spacing), float(min_score), nd[0], nd[1], dev_score,
                                                     C.byref(rec) if record else None, fl[0], fl[1])
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateDevice")
        return rec

    @staticmethod
    def _passes(passes):
        flat = [int(x) for p in passes for x in p]
        if len(flat) != 3 * len(passes):
            raise ValueError("a pass is (radius, range, spacing)")
        return (C.c_int * max(len(flat), 1))(*flat), len(passes)

    @staticmethod
    def correlation_passes_ok(width, height, lo, scale, passes, min_score=-1.0, threshold=2.0, epsilon=0.1, min_neighbours=3, min_pixels=0):
        """OpticalFlow2D::CorrelationPassesOk: whether correlate_multipass* accepts the schedule -- and, for a masked search, the
        min_pixels, which must fit every pass's window (0: the default per pass).  Needs no device."""
        arr, n = OpticalFlow._passes(passes)
        if min_pixels:
            return bool(host_lib().flow2d_host_correlation_passes_masked_ok(width, height, float(lo), float(scale), arr, n, float(min_score),
                                                                            float(threshold), float(epsilon), int(min_neighbours),
                                                                            int(min_pixels)))
        return bool(host_lib().flow2d_host_correlation_passes_ok(width, height, float(lo), float(scale), arr, n, float(min_score),
                                                                 float(threshold), float(epsilon), int(min_neighbours)))

    def correlate_multipass(self, frame_0, frame_1, passes, min_score=-1.0, threshold=2.0, epsilon=0.1, min_neighbours=3, replace=True,
                            validate_last=True, predictor=None, flow=False, mask=None, min_pixels=0):
        """OpticalFlow2D::CorrelateMultiPass: the host pair through `passes` -- 1 .. CORRELATION_MAX_PASSES triples (radius, range,
        spacing), coarse to fine --, every pass searching around the validated, expanded field of the one before (the first around
        `predictor`, a (u, v) pair of images, or around nothing).  Returns (node_u, node_v, node_score, [CorrelationPassReport],
        (lo, scale)) on the last pass's grid; with flow, also the (u, v) of the field expanded to the frame's grid.
        mask (an image of the frames' size in frame 0's coordinates, uploaded once; values of 0.5 and more, and NaN, mean "not the
        specimen") / min_pixels (0: correlation_min_pixels of each pass's radius): the region of interest -- every pass then runs
        flow2d_correlate_masked_2d and flow2d_validate_nodes_masked_2d, and the reports' records count the masked nodes in
        `masked`.  Without a mask the method is the call it always was."""
        if mask is None and min_pixels:
            raise ValueError("min_pixels goes with a mask")
        f0, f1 = self._pair(frame_0, frame_1)
        arr, n = self._passes(passes)
        if not 1 <= n <= CORRELATION_MAX_PASSES:
            raise Flow2DError(1, "OpticalFlow2D::CorrelateMultiPass")
        nw, nh = correlation_grid(self.width, self.height, passes[-1][0], passes[-1][2])
        nodes = [np.empty((nh, nw), np.float32) for _ in range(3)]
        uv = [np.empty_like(f0) for _ in range(2)] if flow else [None, None]
        pred = [np.ascontiguousarray(q, np.float32) for q in predictor] if predictor is not None else [None, None]
        reports = (CorrelationPassReport * n)()
        lo_scale = (C.c_float * 2)()
        if mask is not None:
            region = self._mask_image(mask)
            rc = host_lib().flow2d_host_correlate_multipass_masked(self.handle, _fptr(f0), _fptr(f1), arr, n, float(min_score),
                                                                   float(threshold), float(epsilon), int(min_neighbours), int(bool(replace)),
                                                                   int(bool(validate_last)), _fptr(region), int(min_pixels),
                                                                   _opt_fptr(pred[0]), _opt_fptr(pred[1]), _fptr(nodes[0]), _fptr(nodes[1]),
                                                                   _fptr(nodes[2]), reports, _opt_fptr(uv[0]), _opt_fptr(uv[1]), lo_scale)
        else:
            rc = host_lib().flow2d_host_correlate_multipass(self.handle, _fptr(f0), _fptr(f1), arr, n, float(min_score), float(threshold),
                                                            float(epsilon), int(min_neighbours), int(bool(replace)), int(bool(validate_last)),
                                                            _opt_fptr(pred[0]), _opt_fptr(pred[1]), _fptr(nodes[0]), _fptr(nodes[1]),
                                                            _fptr(nodes[2]), reports, _opt_fptr(uv[0]), _opt_fptr(uv[1]), lo_scale)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateMultiPass")
        out = (nodes[0], nodes[1], nodes[2], list(reports), (lo_scale[0], lo_scale[1]))
        return out + (tuple(uv),) if flow else out

    def correlate_multipass_device(self, dev_frame_0, dev_frame_1, lo, scale, passes, min_score=-1.0, threshold=2.0, epsilon=0.1,
                                   min_neighbours=3, replace=True, validate_last=True, dev_predictor=None, dev_nodes=None, dev_score=None,
                                   dev_flow=None, mask=None, min_pixels=0):
        """OpticalFlow2D::CorrelateMultiPassDevice: device frames in.  dev_predictor (a (u, v) pair of planes of the container's
        size, optional): the first pass's predictor; dev_nodes, dev_score, dev_flow as for correlate_device, from the last pass.
        Returns one CorrelationPassReport per pass; synchronises.  mask (a device plane of the container's size) / min_pixels: the
        region of interest, as for correlate_multipass."""
        arr, n = self._passes(passes)
        reports = (CorrelationPassReport * max(n, 1))()
        pr, nd, fl = dev_predictor or (None, None), dev_nodes or (None, None), dev_flow or (None, None)
        if mask is None and min_pixels:
            raise ValueError("min_pixels goes with a mask")
        if mask is not None:
            rc = host_lib().flow2d_host_correlate_multipass_masked_device(self.handle, dev_frame_0, dev_frame_1, float(lo), float(scale), arr,
                                                                          n, float(min_score), float(threshold), float(epsilon),
                                                                          int(min_neighbours), int(bool(replace)), int(bool(validate_last)),
                                                                          mask, int(min_pixels), pr[0], pr[1], nd[0], nd[1], dev_score,
                                                                          reports, fl[0], fl[1])
        else:
            rc = host_lib().flow2d_host_correlate_multipass_device(self.handle, dev_frame_0, dev_frame_1, float(lo), float(scale), arr, n,
                                                                   float(min_score), float(threshold), float(epsilon), int(min_neighbours),
                                                                   int(bool(replace)), int(bool(validate_last)), pr[0], pr[1], nd[0], nd[1],
                                                                   dev_score, reports, fl[0], fl[1])
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateMultiPassDevice")
        return list(reports)[:n]

    SUBSET_PLANES = ("u", "v", "ux", "uy", "vx", "vy", "score", "state")

    # ... and with order=2 (the second-order refinement, flow2d_subset_refine2_2d) the six curvatures behind them
    SUBSET2_PLANES = SUBSET_PLANES + ("uxx", "uxy", "uyy", "vxx", "vxy", "vyy")

    @staticmethod
    def subset_options_ok(radius, iterations=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5, order=1, max_curvature=0.05, mask=False,
                          min_pixels=0):
        """OpticalFlow2D::SubsetOptionsOk: whether refine_nodes_device / correlate_subset* accept the options; mask=True: together
        with a mask and min_pixels (a mask with order 2 is refused).  Needs no device."""
        options = SubsetOptions(int(radius), int(iterations), float(epsilon), float(max_shift), float(max_gradient), int(order),
                                float(max_curvature), int(min_pixels), 1 if mask else None)
        return bool(host_lib().flow2d_host_subset_options_ok(C.byref(options)))

    @staticmethod
    def _takes_mask(mask, min_pixels, order, where):
        """Whether a call that refines has a mask (OpticalFlow2D::SubsetOptions::mask and min_pixels): mask -- the
        region of interest in frame 0's coordinates, values of 0.5 and more (and NaN) meaning "not the specimen"; a device plane of
        the container's size for a *_device method, else an image of the frames' size --, min_pixels -- the fewest usable pixels a
        node may have, 0 = subset_min_pixels(radius).  A masked node has the state SUBSET_MASKED and NaN in its six planes, and the
        SubsetRecord counts it in `masked`.  Order 1 only.  Without a mask the method is the call it always was."""
        if mask is None:
            if min_pixels:
                raise ValueError("min_pixels goes with a mask")
            return False
        if order != 1:
            raise Flow2DError(1, where, "a subset mask goes with order 1 only")
        return True

    def _mask_image(self, mask):
        image = np.ascontiguousarray(mask, np.float32)
        if image.shape != (self.height, self.width):
            raise ValueError("the subset mask is an image of the object's size")
        return image

    def _subset_options(self, where, radius, iterations, epsilon, max_shift, max_gradient, order, max_curvature, mask, min_pixels,
                        image=False, interpolation="catmull-rom", mask_search=False):
        """The SubsetOptions record of a call that refines, by the rules of _takes_mask.  image: the mask is an image and not a
        device plane; the record then holds the float32 array it points into, which lives as long as the record.
        interpolation -- "catmull-rom" or "bspline", OpticalFlow2D::SubsetOptions::interpolation: how frame 1 is sampled.  With
        "bspline" the call prefilters its frame 1 (a sequence: every step its frame k) into a plane of the object's own and runs the
        spline entry of its order; mask and order go with both.  It travels beside the record (which keeps its 40 bytes): every call
        sets it in the object, so the default restores Catmull-Rom.
        mask_search -- OpticalFlow2D::SubsetOptions::mask_search, on the methods that run the passes of a pair (correlate_subset*):
        with a mask, the passes in front of the refinement run the masked search and the masked validation with it
        (flow2d_correlate_masked_2d, flow2d_validate_nodes_masked_2d), so that an edge node starts from the specimen's motion.
        False is the call it always was; True without a mask is refused.  It travels beside the record like the interpolation."""
        if mask_search and mask is None:
            raise Flow2DError(1, where, "mask_search needs a mask")
        if interpolation not in SUBSET_INTERPOLATIONS:
            raise ValueError("interpolation is one of %s" % ", ".join(sorted(SUBSET_INTERPOLATIONS)))
        held = None
        if self._takes_mask(mask, min_pixels, order, where) and image:
            held = self._mask_image(mask)
            mask = held.ctypes.data
        options = SubsetOptions(int(radius), int(iterations), float(epsilon), float(max_shift), float(max_gradient), int(order),
                                float(max_curvature), int(min_pixels), mask)
        options.held = held
        if host_lib().flow2d_host_set_subset_interpolation(self.handle, SUBSET_INTERPOLATIONS[interpolation]):
            raise Flow2DError(1, where, "the subset interpolation was refused")
        if host_lib().flow2d_host_set_subset_mask_search(self.handle, int(bool(mask_search))):
            raise Flow2DError(1, where, "the subset mask search was refused")
        return options

    @staticmethod
    def _subset_planes(dev_out, order=1):
        """The fourteen device planes of SUBSET2_PLANES from a dict name -> address (absent or None: not wanted) by the names of
        SUBSET_PLANES or, with order=2, of SUBSET2_PLANES."""
        dev_out = dev_out or {}
        names = OpticalFlow.SUBSET_PLANES if order == 1 else OpticalFlow.SUBSET2_PLANES
        unknown = set(dev_out) - set(names)
        if unknown:
            raise ValueError("unknown subset planes %s (of %s)" % (sorted(unknown), ", ".join(names)))
        return (C.c_void_p * 14)(*[dev_out.get(name) for name in OpticalFlow.SUBSET2_PLANES])

    @staticmethod
    def _node_arrays(nodes, per):
        """The fourteen array slots per step of a host-image call from its `per` arrays per step (the other slots: not wanted)."""
        slots = (C.POINTER(C.c_float) * (14 * (len(nodes) // per)))()
        for k, q in enumerate(nodes):
            slots[14 * (k // per) + k % per] = _fptr(q)
        return slots

    def refine_nodes_device(self, dev_frame_0, dev_frame_1, dev_node_u0, dev_node_v0, grid_radius, spacing, radius, iterations=20,
                            epsilon=1e-3, max_shift=2.0, max_gradient=0.5, dev_out=None, record=True, order=1, max_curvature=0.05, mask=None,
                            min_pixels=0, interpolation="catmull-rom"):
        """OpticalFlow2D::RefineNodesDevice: the node field (dev_node_u0, dev_node_v0) of the grid (grid_radius, spacing) -- planes of
        the container's size -- refined by subsets of `radius` (flow2d_subset_refine_2d).  dev_out: a dict of device planes by the
        names of SUBSET_PLANES (u and v both or neither, the four gradients all or none).  Returns the SubsetRecord (the call then
        synchronises) or, without record, None (it only queues).  order=2: the second-order refinement (flow2d_subset_refine2_2d),
        radius from 2, a curvature beyond max_curvature strays; dev_out by the names of SUBSET2_PLANES, the six curvatures all or
        none.  order=1 is the call it always was.  mask (a device plane) / min_pixels: see _takes_mask.  interpolation ("catmull-rom", the
        call it always was, or "bspline": frame 1 prefiltered and sampled as a cubic B-spline), here and on every method below that
        refines: see _subset_options."""
        rec = SubsetRecord()
        options = self._subset_options("OpticalFlow2D::RefineNodesDevice", radius, iterations, epsilon, max_shift, max_gradient, order,
                                       max_curvature, mask, min_pixels, interpolation=interpolation)
        rc = host_lib().flow2d_host_refine_nodes_device(self.handle, dev_frame_0, dev_frame_1, dev_node_u0, dev_node_v0, int(grid_radius),
                                                        int(spacing), C.byref(options), self._subset_planes(dev_out, order),
                                                        C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::RefineNodesDevice")
        return rec if record else None

    def correlate_subset(self, frame_0, frame_1, passes, radius, iterations=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5,
                         min_score=-1.0, threshold=2.0, validate_epsilon=0.1, min_neighbours=3, predictor=None, flow=False, order=1,
                         max_curvature=0.05, mask=None, min_pixels=0, interpolation="catmull-rom", mask_search=False):
        """OpticalFlow2D::CorrelateSubset: the host pair through `passes` as in correlate_multipass -- the last pass validated with
        replacement, so that every node has a start --, then every node of the last pass's grid refined by subsets of `radius` on
        the unquantised frames.  Returns (nodes, [CorrelationPassReport], SubsetRecord, (lo, scale)), nodes a dict of [nh, nw]
        arrays by the names of SUBSET_PLANES; with flow, also the (u, v) of the refined field expanded to the frame's grid.
        order=2: the second-order refinement (radius from 2, a curvature beyond max_curvature strays), nodes by the names of
        SUBSET2_PLANES; order=1 is the call it always was.  mask (an image, uploaded once) / min_pixels: see _takes_mask; mask_search: see _subset_options."""
        f0, f1 = self._pair(frame_0, frame_1)
        arr, n = self._passes(passes)
        if not 1 <= n <= CORRELATION_MAX_PASSES:
            raise Flow2DError(1, "OpticalFlow2D::CorrelateSubset")
        nw, nh = correlation_grid(self.width, self.height, passes[-1][0], passes[-1][2])
        names = self.SUBSET_PLANES if order == 1 else self.SUBSET2_PLANES
        nodes = [np.empty((nh, nw), np.float32) for _ in names]
        uv = [np.empty_like(f0) for _ in range(2)] if flow else [None, None]
        pred = [np.ascontiguousarray(q, np.float32) for q in predictor] if predictor is not None else [None, None]
        reports, rec, lo_scale = (CorrelationPassReport * n)(), SubsetRecord(), (C.c_float * 2)()
        options = self._subset_options("OpticalFlow2D::CorrelateSubset", radius, iterations, epsilon, max_shift, max_gradient, order,
                                       max_curvature, mask, min_pixels, image=True, interpolation=interpolation, mask_search=mask_search)
        rc = host_lib().flow2d_host_correlate_subset(self.handle, _fptr(f0), _fptr(f1), arr, n, float(min_score), float(threshold),
                                                     float(validate_epsilon), int(min_neighbours), C.byref(options), _opt_fptr(pred[0]),
                                                     _opt_fptr(pred[1]), self._node_arrays(nodes, len(names)), reports, C.byref(rec),
                                                     _opt_fptr(uv[0]), _opt_fptr(uv[1]), lo_scale)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateSubset")
        out = (dict(zip(names, nodes)), list(reports), rec, (lo_scale[0], lo_scale[1]))
        return out + (tuple(uv),) if flow else out

    def correlate_subset_device(self, dev_frame_0, dev_frame_1, lo, scale, passes, radius, iterations=20, epsilon=1e-3, max_shift=2.0,
                                max_gradient=0.5, min_score=-1.0, threshold=2.0, validate_epsilon=0.1, min_neighbours=3, dev_predictor=None,
                                dev_out=None, dev_flow=None, order=1, max_curvature=0.05, mask=None, min_pixels=0,
                                interpolation="catmull-rom", mask_search=False):
        """OpticalFlow2D::CorrelateSubsetDevice: device frames in; dev_predictor and dev_flow as for correlate_multipass_device (the
        flow is the refined field's), dev_out, order and max_curvature as for refine_nodes_device.  Returns
        ([CorrelationPassReport], SubsetRecord); synchronises once.  mask (a device plane) / min_pixels: see _takes_mask; mask_search: see _subset_options."""
        arr, n = self._passes(passes)
        reports, rec = (CorrelationPassReport * max(n, 1))(), SubsetRecord()
        pr, fl = dev_predictor or (None, None), dev_flow or (None, None)
        options = self._subset_options("OpticalFlow2D::CorrelateSubsetDevice", radius, iterations, epsilon, max_shift, max_gradient, order,
                                       max_curvature, mask, min_pixels, interpolation=interpolation, mask_search=mask_search)
        rc = host_lib().flow2d_host_correlate_subset_device(self.handle, dev_frame_0, dev_frame_1, float(lo), float(scale), arr, n,
                                                            float(min_score), float(threshold), float(validate_epsilon), int(min_neighbours),
                                                            C.byref(options), pr[0], pr[1], self._subset_planes(dev_out, order), reports,
                                                            C.byref(rec), fl[0], fl[1])
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateSubsetDevice")
        return list(reports)[:n], rec

    @staticmethod
    def sequence_options_ok(fill=2, min_state=1, predict_neighbours=1, sequence_max_shift=4.0):
        """OpticalFlow2D::SequenceOptionsOk: whether correlate_subset_sequence* accept the options.  Needs no device."""
        return bool(host_lib().flow2d_host_sequence_options_ok(int(fill), int(min_state), int(predict_neighbours), float(sequence_max_shift)))

    def refine_nodes_from_device(self, dev_frame_0, dev_frame_1, dev_start, grid_radius, spacing, radius, iterations=20, epsilon=1e-3,
                                 max_shift=4.0, max_gradient=0.5, dev_out=None, record=True, order=1, max_curvature=0.05, mask=None,
                                 min_pixels=0, interpolation="catmull-rom"):
        """OpticalFlow2D::RefineNodesFromDevice: refine_nodes_device started from a whole deformation (flow2d_subset_refine_from_2d):
        dev_start is a dict of the six device planes u, v, ux, uy, vx, vy (by the names of SUBSET_PLANES), all needed.  Returns the
        SubsetRecord (the call then synchronises) or, without record, None (it only queues).  order and max_curvature as for
        refine_nodes_device; at order 2 the start's curvatures are 0.  mask (a device plane) / min_pixels: see _takes_mask."""
        names = self.SUBSET_PLANES[:6]
        if set(dev_start) != set(names) or not all(dev_start[n] for n in names):
            raise ValueError("refine_nodes_from_device takes the six start planes %s" % ", ".join(names))
        rec = SubsetRecord()
        options = self._subset_options("OpticalFlow2D::RefineNodesFromDevice", radius, iterations, epsilon, max_shift, max_gradient, order,
                                       max_curvature, mask, min_pixels, interpolation=interpolation)
        rc = host_lib().flow2d_host_refine_nodes_from_device(self.handle, dev_frame_0, dev_frame_1, (C.c_void_p * 6)(*[dev_start[n] for n in names]),
                                                             int(grid_radius), int(spacing), C.byref(options),
                                                             self._subset_planes(dev_out, order), C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::RefineNodesFromDevice")
        return rec if record else None

    def correlate_subset_sequence(self, frames, passes, radius, iterations=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5, min_score=-1.0,
                                  threshold=2.0, validate_epsilon=0.1, min_neighbours=3, fill=2, min_state=1, predict_neighbours=1,
                                  sequence_max_shift=4.0, flow=False, order=1, max_curvature=0.05, mask=None, min_pixels=0,
                                  interpolation="catmull-rom", reference_every=0, mask_search=False):
        """OpticalFlow2D::CorrelateSubsetSequence: digital image correlation over a loading sequence.  (order=2: every step refines
        at second order, the steps after the first from the prediction's first-order planes with zero curvatures; the nodes then
        go by the names of SUBSET2_PLANES.)  frames[0] is the reference and
        every later frame is correlated against it: step 1 is correlate_subset's chain; step k >= 2 takes the previous step's
        deformation, gradients included, as its start -- `fill` passes of flow2d_predict_nodes_2d keep the nodes with a state of
        min_state at least and refill the others from predict_neighbours usable neighbours, then flow2d_subset_refine_from_2d
        with sequence_max_shift in place of max_shift -- and no window search runs.  Returns ([nodes per step], [CorrelationPassReport]
        of step 1, [SequenceStepReport], (lo, scale)), nodes a dict of [nh, nw] arrays by the names of SUBSET_PLANES; with flow,
        also [(u, v) per step], the refined field expanded to the frame's grid.  mask (an image, uploaded once and used by every
        step) / min_pixels: see _takes_mask; mask_search: see _subset_options.  reference_every: see _moving_reference; the composition's records are left in
        self.compose_records."""
        images = [np.ascontiguousarray(q, np.float32) for q in frames]
        if len(images) < 2 or any(q.shape != (self.height, self.width) for q in images):
            raise ValueError("correlate_subset_sequence takes two or more frames of the object's size")
        arr, n = self._passes(passes)
        if not 1 <= n <= CORRELATION_MAX_PASSES:
            raise Flow2DError(1, "OpticalFlow2D::CorrelateSubsetSequence")
        steps = len(images) - 1
        nw, nh = correlation_grid(self.width, self.height, passes[-1][0], passes[-1][2])
        names = self.SUBSET_PLANES if order == 1 else self.SUBSET2_PLANES
        per = len(names)
        nodes = [np.empty((nh, nw), np.float32) for _ in range(per * steps)]
        uv = [np.empty_like(images[0]) for _ in range(2 * steps)] if flow else None
        fpp = C.POINTER(C.c_float)
        reports, reps, lo_scale = (CorrelationPassReport * n)(), (SequenceStepReport * steps)(), (C.c_float * 2)()
        options = self._subset_options("OpticalFlow2D::CorrelateSubsetSequence", radius, iterations, epsilon, max_shift, max_gradient, order,
                                       max_curvature, mask, min_pixels, image=True, interpolation=interpolation, mask_search=mask_search)
        self._moving_reference("OpticalFlow2D::CorrelateSubsetSequence", reference_every)
        rc = host_lib().flow2d_host_correlate_subset_sequence(self.handle, (fpp * len(images))(*[_fptr(q) for q in images]), len(images), arr, n,
                                                              float(min_score), float(threshold), float(validate_epsilon), int(min_neighbours),
                                                              C.byref(options), int(fill), int(min_state), int(predict_neighbours),
                                                              float(sequence_max_shift), self._node_arrays(nodes, per), reports, reps,
                                                              (fpp * (2 * steps))(*[_fptr(q) for q in uv]) if flow else None, lo_scale)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateSubsetSequence")
        self.compose_records = self._read_compose_records(steps)
        per_step = [dict(zip(names, nodes[per * k:per * k + per])) for k in range(steps)]
        out = (per_step, list(reports), list(reps), (lo_scale[0], lo_scale[1]))
        return out + ([(uv[2 * k], uv[2 * k + 1]) for k in range(steps)],) if flow else out

    def correlate_subset_sequence_device(self, dev_frames, lo, scale, passes, radius, dev_out, iterations=20, epsilon=1e-3, max_shift=2.0,
                                         max_gradient=0.5, min_score=-1.0, threshold=2.0, validate_epsilon=0.1, min_neighbours=3, fill=2,
                                         min_state=1, predict_neighbours=1, sequence_max_shift=4.0, dev_flows=None, order=1,
                                         max_curvature=0.05, mask=None, min_pixels=0, interpolation="catmull-rom", reference_every=0, mask_search=False):
        """OpticalFlow2D::CorrelateSubsetSequenceDevice: device frames in (the first is the reference); dev_out: per step a dict of
        device planes by the names of SUBSET_PLANES, of which only the score may be missing; dev_flows: per step a (u, v) pair or
        None.  Returns ([CorrelationPassReport] of step 1, [SequenceStepReport]); synchronises once.  order=2: every step refines
        at second order -- the steps after the first from the prediction's six first-order planes with zero curvatures --, dev_out
        by the names of SUBSET2_PLANES, the six curvatures all or none per step.  mask (a device plane, used by every step) /
        min_pixels: see _takes_mask; mask_search: see _subset_options.  reference_every: see _moving_reference; the composition's records are left in
        self.compose_records."""
        arr, n = self._passes(passes)
        steps = len(dev_frames) - 1
        if steps < 1 or len(dev_out) != steps or (dev_flows is not None and len(dev_flows) != steps):
            raise ValueError("correlate_subset_sequence_device takes two or more frames and one set of planes per step")
        planes = []
        for step in dev_out:
            planes += list(self._subset_planes(step, order))
        flows = None
        if dev_flows is not None:
            flat = []
            for pair in dev_flows:
                flat += list(pair) if pair is not None else [None, None]
            flows = (C.c_void_p * (2 * steps))(*flat)
        reports, reps = (CorrelationPassReport * max(n, 1))(), (SequenceStepReport * steps)()
        options = self._subset_options("OpticalFlow2D::CorrelateSubsetSequenceDevice", radius, iterations, epsilon, max_shift, max_gradient,
                                       order, max_curvature, mask, min_pixels, interpolation=interpolation, mask_search=mask_search)
        self._moving_reference("OpticalFlow2D::CorrelateSubsetSequenceDevice", reference_every)
        rc = host_lib().flow2d_host_correlate_subset_sequence_device(self.handle, (C.c_void_p * len(dev_frames))(*dev_frames), len(dev_frames),
                                                                     float(lo), float(scale), arr, n, float(min_score), float(threshold),
                                                                     float(validate_epsilon), int(min_neighbours), C.byref(options), int(fill),
                                                                     int(min_state), int(predict_neighbours), float(sequence_max_shift),
                                                                     (C.c_void_p * (14 * steps))(*planes), reports, reps, flows)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::CorrelateSubsetSequenceDevice")
        self.compose_records = self._read_compose_records(steps)
        return list(reports)[:n], list(reps)

    def _moving_reference(self, where, reference_every):
        """SequenceOptions::reference_every of the sequence call that follows: 0 -- every step against frame 0, what it always was --
        or N >= 1: step k is measured against frame N * floor((k - 1) / N) and composed with the field up to that frame
        (flow2d_compose_nodes_2d), so that every delivered field is still frame 0 -> frame k at the nodes of frame 0, with the
        state SUBSET_STATE_COMPOSED or SUBSET_NO_INPUT.  Refused with a mask and with curvature planes.  The value is the object's
        (flow2d_host_set_reference_every) and is set before every sequence call, so that a call without the keyword is never
        moved by an earlier one."""
        if host_lib().flow2d_host_set_reference_every(self.handle, int(reference_every)):
            raise Flow2DError(1, where)

    def _read_compose_records(self, steps):
        """The composition records of the sequence call just made: one ComposeRecord per step, zero where the step was measured
        against frame 0."""
        records = (ComposeRecord * steps)()
        host_lib().flow2d_host_compose_records(self.handle, records, steps)
        return list(records)

    COMPOSE_BASE = ("u", "v", "ux", "uy", "vx", "vy", "state")  # what compose_nodes* read of the base's SUBSET_PLANES

    def compose_nodes(self, base, increment, grid_radius, spacing, min_state=1, record=True):
        """OpticalFlow2D::ComposeNodes: the composition of two node fields across a moved reference (flow2d_compose_nodes_2d).  base --
        frame 0 -> frame r at the nodes of frame 0 -- and increment -- frame r -> frame k on the same grid laid in frame r -- are
        dicts of [nh, nw] arrays by the names of SUBSET_PLANES, as correlate_subset* return them; u, v, the gradients and the state
        are needed, the increment's score is blended when it is there.  Returns ({name: [nh, nw] array} by the names of
        SUBSET_PLANES -- without "score" when the increment has none --, ComposeRecord or None)."""
        nw, nh = correlation_grid(self.width, self.height, grid_radius, spacing)
        need = self.COMPOSE_BASE
        if any(n not in base for n in need) or any(n not in increment for n in need):
            raise ValueError("compose_nodes takes %s of base and increment" % ", ".join(need))
        a = [np.ascontiguousarray(base[n], np.float32) for n in need]
        names = [n for n in self.SUBSET_PLANES if n != "score" or increment.get("score") is not None]
        b = {n: np.ascontiguousarray(increment[n], np.float32) for n in names}
        if any(q.shape != (nh, nw) for q in a + list(b.values())):
            raise ValueError("compose_nodes takes node fields of the %d x %d grid" % (nw, nh))
        out = {n: np.empty((nh, nw), np.float32) for n in names}
        fp = C.POINTER(C.c_float)
        rec = ComposeRecord()
        rc = host_lib().flow2d_host_compose_nodes(self.handle, (fp * 7)(*[_fptr(q) for q in a]),
                                                  (fp * 8)(*[_opt_fptr(b.get(n)) for n in self.SUBSET_PLANES]), int(grid_radius), int(spacing),
                                                  int(min_state), (fp * 8)(*[_opt_fptr(out.get(n)) for n in self.SUBSET_PLANES]),
                                                  C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComposeNodes")
        return out, (rec if record else None)

    def compose_nodes_device(self, dev_base, dev_increment, grid_radius, spacing, dev_out, min_state=1, record=True):
        """OpticalFlow2D::ComposeNodesDevice: dicts of device planes by the names of SUBSET_PLANES -- of the base u, v, the gradients
        and the state, of the increment those and optionally the score, of dev_out u, v and the gradients and optionally state and
        score (a score only with the increment's).  Returns the ComposeRecord (the call then synchronises) or, without record,
        None (it only queues)."""
        rec = ComposeRecord()
        vp = C.c_void_p
        rc = host_lib().flow2d_host_compose_nodes_device(self.handle, (vp * 7)(*[dev_base.get(n) for n in self.COMPOSE_BASE]),
                                                         (vp * 8)(*[dev_increment.get(n) for n in self.SUBSET_PLANES]), int(grid_radius),
                                                         int(spacing), int(min_state), (vp * 8)(*[dev_out.get(n) for n in self.SUBSET_PLANES]),
                                                         C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComposeNodesDevice")
        return rec if record else None

    UNCERTAINTY_PLANES = SUBSET_UNCERTAINTY_PLANES  # what node_uncertainty* write: sigma_u and sigma_v needed, the gradient sigmas all or none

    def node_uncertainty(self, frame_0, frame_1, nodes, grid_radius, spacing, radius, min_state=1, mask=None, min_pixels=0,
                         interpolation="catmull-rom", record=True):
        """OpticalFlow2D::NodeUncertainty: the uncertainty of a first-order refinement's nodes (flow2d_subset_uncertainty_2d).  nodes
        -- a dict of [nh, nw] arrays by the names of SUBSET_PLANES, as correlate_subset* return them (u, v, the gradients and the
        state are needed) -- is the refinement of (frame_0, frame_1) on the grid (grid_radius, spacing); `radius`, mask (an image) /
        min_pixels and interpolation are the refinement's.  Per node the covariance s2 * H^-1 of the Gauss-Newton least squares at
        the node's p: sigma_u, sigma_v and the four gradient sigmas estimate the random error the frames' noise puts into p (not
        the sample's interpolation bias), rho is the correlation of u and v, noise is sqrt(s2) in grey values.  A node below
        min_state, off the mask, out of the frame or flat is NaN.  Returns ({name: [nh, nw] array} by the names of
        UNCERTAINTY_PLANES, UncertaintyRecord or None)."""
        f0, f1 = self._pair(frame_0, frame_1)
        nw, nh = correlation_grid(self.width, self.height, grid_radius, spacing)
        need = self.COMPOSE_BASE
        if any(n not in nodes for n in need):
            raise ValueError("node_uncertainty takes %s of the refinement" % ", ".join(need))
        a = [np.ascontiguousarray(nodes[n], np.float32) for n in need]
        if any(q.shape != (nh, nw) for q in a):
            raise ValueError("node_uncertainty takes a node field of the %d x %d grid" % (nw, nh))
        out = {n: np.empty((nh, nw), np.float32) for n in self.UNCERTAINTY_PLANES}
        options = self._subset_options("OpticalFlow2D::NodeUncertainty", radius, 20, 1e-3, 2.0, 0.5, 1, 0.05, mask, min_pixels, image=True,
                                       interpolation=interpolation)
        fp = C.POINTER(C.c_float)
        rec = UncertaintyRecord()
        rc = host_lib().flow2d_host_node_uncertainty(self.handle, _fptr(f0), _fptr(f1), (fp * 7)(*[_fptr(q) for q in a]), int(grid_radius),
                                                     int(spacing), C.byref(options), int(min_state),
                                                     (fp * 8)(*[_fptr(out[n]) for n in self.UNCERTAINTY_PLANES]),
                                                     C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::NodeUncertainty")
        return out, (rec if record else None)

    def node_uncertainty_device(self, dev_frame_0, dev_frame_1, dev_nodes, grid_radius, spacing, radius, dev_out, min_state=1, mask=None,
                                min_pixels=0, interpolation="catmull-rom", record=True, order=1):
        """OpticalFlow2D::NodeUncertaintyDevice: dev_nodes -- a dict of device planes by the names of SUBSET_PLANES, of which u, v,
        the gradients and the state are needed --, dev_out -- a dict of device planes by the names of UNCERTAINTY_PLANES (sigma_u
        and sigma_v needed, the four gradient sigmas all or none) --, planes of the container's size.  mask: a device plane.
        order=2 is refused: twelve parameters need a 12 x 12 covariance.  Returns the UncertaintyRecord (the call then
        synchronises) or, without record, None (it only queues)."""
        unknown = set(dev_out) - set(self.UNCERTAINTY_PLANES)
        if unknown:
            raise ValueError("unknown uncertainty planes %s (of %s)" % (sorted(unknown), ", ".join(self.UNCERTAINTY_PLANES)))
        if order != 1:  # (before the mask's rule: the reason printed is the uncertainty's own)
            options = SubsetOptions(int(radius), 20, 1e-3, 2.0, 0.5, int(order), 0.05, 0, None)
            if not host_lib().flow2d_host_uncertainty_options_ok(C.byref(options), int(min_state)):
                raise Flow2DError(1, "OpticalFlow2D::NodeUncertaintyDevice", "the node uncertainty goes with order 1 only")
        options = self._subset_options("OpticalFlow2D::NodeUncertaintyDevice", radius, 20, 1e-3, 2.0, 0.5, order, 0.05, mask, min_pixels,
                                       interpolation=interpolation)
        rec = UncertaintyRecord()
        vp = C.c_void_p
        rc = host_lib().flow2d_host_node_uncertainty_device(self.handle, dev_frame_0, dev_frame_1,
                                                            (vp * 7)(*[dev_nodes.get(n) for n in self.COMPOSE_BASE]), int(grid_radius),
                                                            int(spacing), C.byref(options), int(min_state),
                                                            (vp * 8)(*[dev_out.get(n) for n in self.UNCERTAINTY_PLANES]),
                                                            C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::NodeUncertaintyDevice")
        return rec if record else None


    NODE_PLANES = ("u", "v", "ux", "uy", "vx", "vy", "state")  # what node_strain* read of a step's SUBSET_PLANES

    @staticmethod
    def strain_options_ok(window=2, order=1, min_nodes=0, min_state=1, measure=STRAIN_SMALL, sigma=0.0, iterations=8, weighted=False,
                          sigma_floor=0.0, threshold=0.0):
        """OpticalFlow2D::StrainOptionsOk: whether node_strain* accept the options.  Needs no device.  weighted: the options of a
        call with uncertainty= (a robust sigma beside it is refused: one scale is in pixels, the other in sigmas)."""
        if weighted:
            return bool(host_lib().flow2d_host_strain_weighted_options_ok(int(window), int(order), int(min_nodes), int(min_state),
                                                                          int(measure), float(sigma), float(sigma_floor), float(threshold),
                                                                          int(iterations)))
        if sigma == 0.0:
            return bool(host_lib().flow2d_host_strain_options_ok(int(window), int(order), int(min_nodes), int(min_state), int(measure)))
        return bool(host_lib().flow2d_host_strain_robust_options_ok(int(window), int(order), int(min_nodes), int(min_state), int(measure),
                                                                    float(sigma), int(iterations)))

    def _set_strain_robust(self, sigma, iterations, diagnostics, steps):
        """The robust scale and passes of the node-strain call that follows, and its diagnostic planes (3 * steps pointers or None)."""
        L = host_lib()
        if L.flow2d_host_set_strain_robust(self.handle, float(sigma), int(iterations)):
            raise ValueError("node_strain: sigma is finite and >= 0 (0 = off), iterations 0 .. %d" % NODE_STRAIN_MAX_ITERATIONS)
        if diagnostics is not None and sigma == 0.0:
            raise ValueError("node_strain: the diagnostic planes go with sigma > 0")
        L.flow2d_host_set_strain_diagnostics(self.handle, (C.c_void_p * len(diagnostics))(*diagnostics) if diagnostics else None,
                                             steps if diagnostics else 0)

    def _set_strain_weighting(self, sigma, sigma_floor, threshold, iterations, diagnostics, steps):
        """The weighting of the weighted node-strain call that follows and its diagnostic planes; afterwards the object is as it
        was, so that a later plain or robust call is not weighted."""
        L = host_lib()
        if L.flow2d_host_set_strain_robust(self.handle, float(sigma), int(iterations)) or \
                L.flow2d_host_set_strain_weighting(self.handle, 1, float(sigma_floor), float(threshold), int(iterations) if threshold > 0 else 0):
            raise ValueError("node_strain: sigma_floor and threshold are finite and >= 0, iterations 0 .. %d" % NODE_STRAIN_MAX_ITERATIONS)
        L.flow2d_host_set_strain_diagnostics(self.handle, (C.c_void_p * len(diagnostics))(*diagnostics) if diagnostics else None,
                                             steps if diagnostics else 0)

    def _clear_strain_weighting(self):
        host_lib().flow2d_host_set_strain_weighting(self.handle, 0, 0.0, 0.0, 0)

    def node_strain(self, nodes, spacing, window=2, order=1, min_nodes=0, min_state=1, measure=STRAIN_SMALL, planes=DEFORMATION_PLANES,
                    stats=True, sigma=0.0, iterations=8, diagnostics=(), uncertainty=None, sigma_floor=0.0, threshold=0.0,
                    strain_sigmas=()):
        """OpticalFlow2D::NodeStrain: strain on the node grid (flow2d_node_strain_2d) of one result -- the dict of [nh, nw] arrays
        by the names of SUBSET_PLANES that correlate_subset returns; u and v are needed, the gradients only with window 0, without a
        state every finite node is usable -- or of the list of steps that correlate_subset_sequence returns.  `window` nodes around
        each node are fitted by a polynomial of `order` (0: the node's own gradients); min_nodes 0 = one more than the fit has
        coefficients.  sigma > 0: the robust fit (flow2d_node_strain_robust_2d) with `iterations` reweighted passes; diagnostics --
        names of NODE_STRAIN_DIAGNOSTICS -- then come back in the dict beside the planes, and node_strain_robust_counts reads the
        record's further words.  Returns ({name: [nh, nw] array} for `planes`, DeformationStats or None), or the list of those per
        step.
        uncertainty -- the dict node_uncertainty returned (sigma_u and sigma_v are read), or a list of them, one per step: the
        weighted fit (flow2d_node_strain_weighted_2d) with sigma_floor in pixels and `threshold` in sigmas (0: no robust part;
        above 0: `iterations` reweighted passes); strain_sigmas -- names of STRAIN_SIGMA_PLANES -- come back in the dict, and
        node_strain_weighted_counts reads the record's further words.  Not together with sigma > 0."""
        single = isinstance(nodes, dict)
        steps = [nodes] if single else list(nodes)
        if not steps or any("u" not in q or "v" not in q for q in steps):
            raise ValueError("node_strain takes a node field with u and v, or a list of them")
        unknown = [name for name in planes if name not in DEFORMATION_PLANES]
        if unknown:
            raise ValueError("deformation planes are %s, not %s" % (", ".join(DEFORMATION_PLANES), unknown))
        nh, nw = np.shape(steps[0]["u"])
        if uncertainty is None and (strain_sigmas or sigma_floor or threshold):
            raise ValueError("node_strain: sigma_floor, threshold and strain_sigmas go with uncertainty=")
        if uncertainty is not None:
            sig_steps = [uncertainty] if isinstance(uncertainty, dict) else list(uncertainty)
            if len(sig_steps) != len(steps) or any("sigma_u" not in q or "sigma_v" not in q for q in sig_steps):
                raise ValueError("node_strain takes one uncertainty with sigma_u and sigma_v per step")
            unknown = [n for n in diagnostics if n not in NODE_STRAIN_DIAGNOSTICS] + [n for n in strain_sigmas if n not in STRAIN_SIGMA_PLANES]
            if unknown:
                raise ValueError("node strain diagnostics are %s and strain sigmas %s, not %s" %
                                 (", ".join(NODE_STRAIN_DIAGNOSTICS), ", ".join(STRAIN_SIGMA_PLANES), unknown))

            def images(fields, names):
                held = []
                for q in fields:
                    for name in names:
                        a = q.get(name)
                        if a is not None:
                            a = np.ascontiguousarray(a, np.float32)
                            if a.shape != (nh, nw):
                                raise ValueError("node_strain: the node images are not %d x %d" % (nw, nh))
                        held.append(a)
                return held

            def wanted(names, every):
                return [np.empty((nh, nw), np.float32) if name in names else None for _ in steps for name in every]

            given, sig_in = images(steps, self.NODE_PLANES), images(sig_steps, ("sigma_u", "sigma_v"))
            out, diag, sig_out = wanted(planes, DEFORMATION_PLANES), wanted(diagnostics, NODE_STRAIN_DIAGNOSTICS), wanted(strain_sigmas, STRAIN_SIGMA_PLANES)
            fpp = C.POINTER(C.c_float)
            array = lambda held: (fpp * len(held))(*[_opt_fptr(a) for a in held])  # noqa: E731
            recs = (DeformationStats * len(steps))()
            self._set_strain_weighting(sigma, sigma_floor, threshold, iterations,
                                       [a.ctypes.data if a is not None else None for a in diag] if diagnostics else None, len(steps))
            try:
                rc = host_lib().flow2d_host_node_strain_weighted(self.handle, array(given), array(sig_in), len(steps), nw, nh, int(spacing),
                                                                 int(window), int(order), int(min_nodes), int(min_state), int(measure),
                                                                 array(out) if planes else None, array(sig_out) if strain_sigmas else None,
                                                                 recs if stats else None)
            finally:
                self._clear_strain_weighting()
            if rc:
                raise Flow2DError(rc, "OpticalFlow2D::NodeStrain (weighted)")
            per_step = []
            for k in range(len(steps)):
                got = {name: out[9 * k + c] for c, name in enumerate(DEFORMATION_PLANES) if name in planes}
                got.update({name: diag[3 * k + c] for c, name in enumerate(NODE_STRAIN_DIAGNOSTICS) if name in diagnostics})
                got.update({name: sig_out[9 * k + c] for c, name in enumerate(STRAIN_SIGMA_PLANES) if name in strain_sigmas})
                per_step.append((got, recs[k] if stats else None))
            return per_step[0] if single else per_step
        given = []
        for q in steps:
            for name in self.NODE_PLANES:
                a = q.get(name)
                if a is not None:
                    a = np.ascontiguousarray(a, np.float32)
                    if a.shape != (nh, nw):
                        raise ValueError("node_strain: the node images are not %d x %d" % (nw, nh))
                given.append(a)
        out = [np.empty((nh, nw), np.float32) if name in planes else None for _ in steps for name in DEFORMATION_PLANES]
        unknown = [name for name in diagnostics if name not in NODE_STRAIN_DIAGNOSTICS]
        if unknown:
            raise ValueError("node strain diagnostics are %s, not %s" % (", ".join(NODE_STRAIN_DIAGNOSTICS), unknown))
        diag = [np.empty((nh, nw), np.float32) if name in diagnostics else None for _ in steps for name in NODE_STRAIN_DIAGNOSTICS]
        self._set_strain_robust(sigma, iterations, [a.ctypes.data if a is not None else None for a in diag] if diagnostics else None,
                                len(steps))
        fpp = C.POINTER(C.c_float)
        recs = (DeformationStats * len(steps))()
        rc = host_lib().flow2d_host_node_strain(self.handle, (fpp * len(given))(*[_opt_fptr(a) for a in given]), len(steps), nw, nh,
                                                int(spacing), int(window), int(order), int(min_nodes), int(min_state), int(measure),
                                                (fpp * len(out))(*[_opt_fptr(a) for a in out]) if planes else None,
                                                recs if stats else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::NodeStrain")
        per_step = [({name: out[9 * k + c] for c, name in enumerate(DEFORMATION_PLANES) if name in planes}, recs[k] if stats else None)
                    for k in range(len(steps))]
        for k, (got, _) in enumerate(per_step):
            got.update({name: diag[3 * k + c] for c, name in enumerate(NODE_STRAIN_DIAGNOSTICS) if name in diagnostics})
        return per_step[0] if single else per_step

    def node_strain_device(self, dev_nodes, nw, nh, spacing, window=2, order=1, min_nodes=0, min_state=1, measure=STRAIN_SMALL,
                           dev_planes=None, stats=True, sigma=0.0, iterations=8, diagnostics=None, uncertainty=None, sigma_floor=0.0,
                           threshold=0.0, strain_sigmas=None):
        """OpticalFlow2D::NodeStrainDevice: dev_nodes -- a dict of device planes of the container's size by the names of
        SUBSET_PLANES (as refine_nodes_device / correlate_subset*_device wrote them), or a list of them, one per step; dev_planes --
        a dict of device planes by the names of DEFORMATION_PLANES (or a list, one per step), which stay on the device.  Returns the
        DeformationStats (a list for a list) -- the call then synchronises once -- or, without stats, None (it only queues).
        sigma > 0: the robust fit; diagnostics -- a dict of device planes by the names of NODE_STRAIN_DIAGNOSTICS (or a list, one
        per step), which stay on the device.
        uncertainty -- a dict of device planes with sigma_u and sigma_v as node_uncertainty_device wrote them (or a list, one per
        step): the weighted fit, with sigma_floor, threshold and iterations as in node_strain; strain_sigmas -- a dict of device
        planes by the names of STRAIN_SIGMA_PLANES (or a list, one per step), which stay on the device."""
        single = isinstance(dev_nodes, dict)
        steps = [dev_nodes] if single else list(dev_nodes)
        if uncertainty is None and (strain_sigmas is not None or sigma_floor or threshold):
            raise ValueError("node_strain_device: sigma_floor, threshold and strain_sigmas go with uncertainty=")
        outs = [dev_planes] if single or dev_planes is None else list(dev_planes)
        if dev_planes is not None and len(outs) != len(steps):
            raise ValueError("node_strain_device takes one set of planes per step")
        unknown = [name for q in outs if q for name in q if name not in DEFORMATION_PLANES]
        if unknown:
            raise ValueError("deformation planes are %s, not %s" % (", ".join(DEFORMATION_PLANES), unknown))
        flat = [q.get(name) for q in steps for name in self.NODE_PLANES]
        wanted = [q.get(name) for q in outs for name in DEFORMATION_PLANES] if dev_planes is not None else None
        diags = None if diagnostics is None else ([diagnostics] if single else list(diagnostics))
        if diags is not None and len(diags) != len(steps):
            raise ValueError("node_strain_device takes one set of diagnostic planes per step")
        unknown = [name for q in diags or () for name in q if name not in NODE_STRAIN_DIAGNOSTICS]
        if unknown:
            raise ValueError("node strain diagnostics are %s, not %s" % (", ".join(NODE_STRAIN_DIAGNOSTICS), unknown))
        if uncertainty is not None:
            per = lambda given, what: [given] if single else list(given)  # noqa: E731
            sig_steps = per(uncertainty, "uncertainty")
            sig_outs = None if strain_sigmas is None else per(strain_sigmas, "strain sigmas")
            if len(sig_steps) != len(steps) or (sig_outs is not None and len(sig_outs) != len(steps)) or \
                    any(not q.get("sigma_u") or not q.get("sigma_v") for q in sig_steps):
                raise ValueError("node_strain_device takes one uncertainty with sigma_u and sigma_v, and one set of strain sigmas, per step")
            unknown = [name for q in sig_outs or () for name in q if name not in STRAIN_SIGMA_PLANES]
            if unknown:
                raise ValueError("strain sigmas are %s, not %s" % (", ".join(STRAIN_SIGMA_PLANES), unknown))
            vps = lambda held: (C.c_void_p * len(held))(*held)  # noqa: E731
            sig_in = [q.get(name) for q in sig_steps for name in ("sigma_u", "sigma_v")]
            sig_wanted = None if sig_outs is None else [q.get(name) for q in sig_outs for name in STRAIN_SIGMA_PLANES]
            recs = (DeformationStats * len(steps))()
            self._set_strain_weighting(sigma, sigma_floor, threshold, iterations,
                                       [q.get(name) for q in diags for name in NODE_STRAIN_DIAGNOSTICS] if diags else None, len(steps))
            try:
                rc = host_lib().flow2d_host_node_strain_weighted_device(self.handle, vps(flat), vps(sig_in), len(steps), nw, nh, int(spacing),
                                                                        int(window), int(order), int(min_nodes), int(min_state),
                                                                        int(measure), vps(wanted) if wanted is not None else None,
                                                                        vps(sig_wanted) if sig_wanted is not None else None,
                                                                        recs if stats else None)
            finally:
                self._clear_strain_weighting()
            if rc:
                raise Flow2DError(rc, "OpticalFlow2D::NodeStrainDevice (weighted)")
            if not stats:
                return None
            return recs[0] if single else list(recs)
        self._set_strain_robust(sigma, iterations, [q.get(name) for q in diags for name in NODE_STRAIN_DIAGNOSTICS] if diags else None,
                                len(steps))
        recs = (DeformationStats * len(steps))()
        rc = host_lib().flow2d_host_node_strain_device(self.handle, (C.c_void_p * len(flat))(*flat), len(steps), nw, nh, int(spacing),
                                                       int(window), int(order), int(min_nodes), int(min_state), int(measure),
                                                       (C.c_void_p * len(wanted))(*wanted) if wanted is not None else None,
                                                       recs if stats else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::NodeStrainDevice")
        if not stats:
            return None
        return recs[0] if single else list(recs)

    @staticmethod
    def _prior_level(level):
        if level is not None and int(level) < 0:
            raise ValueError("prior level %d (>= 0)" % int(level))
        return -1 if level is None else int(level)

    def compute_flow_from_prior(self, frame_0, frame_1, prior_u, prior_v, params, reach=2.0, level=None):
        """OpticalFlow2D::ComputeFlowFromPrior: the flow of the host pair from a pyramid that starts from the prior flow (prior_u,
        prior_v) -- full-resolution pixels, [height, width]; pixels that are not finite enter as zero -- at the level
        prior_start_level(..., reach, level).  Returns (u, v, PriorReport, device_ms)."""
        f0, f1 = self._pair(frame_0, frame_1)
        pu, pv = self._pair(prior_u, prior_v)
        u, v = np.empty_like(f0), np.empty_like(f0)
        report, ms = PriorReport(), C.c_float()
        rc = host_lib().flow2d_host_compute_flow_from_prior(self.handle, _fptr(f0), _fptr(f1), _fptr(pu), _fptr(pv), _fptr(u), _fptr(v),
                                                            C.byref(params), float(reach), self._prior_level(level), C.byref(report),
                                                            C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowFromPrior")
        return u, v, report, ms.value

    def compute_flow_from_prior_device(self, dev_f0, dev_f1, dev_prior_u, dev_prior_v, dev_u, dev_v, params, reach=2.0, level=None,
                                       report=True):
        """OpticalFlow2D::ComputeFlowFromPriorDevice: raw device addresses of pitched containers.  With report the count of
        non-finite prior pixels is read back and the PriorReport returned (synchronises); without, the call only queues."""
        rep = PriorReport() if report else None
        rc = host_lib().flow2d_host_compute_flow_from_prior_device(self.handle, dev_f0, dev_f1, dev_prior_u, dev_prior_v, dev_u, dev_v,
                                                                   C.byref(params), float(reach), self._prior_level(level),
                                                                   C.byref(rep) if report else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowFromPriorDevice")
        return rep

    def compute_flow_correlation_seeded(self, frame_0, frame_1, params, radius=7, search=8, spacing=8, min_score=-1.0, reach=2.0,
                                        level=None):
        """OpticalFlow2D::ComputeFlowCorrelationSeeded: window correlation of the host pair (as correlate), its node field expanded
        to the frame's grid, and the flow from a pyramid that starts from that field (as compute_flow_from_prior; pixels the
        expansion leaves NaN enter as zero and are counted).  Returns a dict: u, v, report (PriorReport), nodes (u, v, score),
        record (CorrelationRecord), prior (u, v: the expanded field), lo_scale, ms."""
        f0, f1 = self._pair(frame_0, frame_1)
        nw, nh = correlation_grid(self.width, self.height, radius, spacing)
        nodes = [np.empty((nh, nw), np.float32) for _ in range(3)]
        u, v, pu, pv = (np.empty_like(f0) for _ in range(4))
        record, report, lo_scale, ms = CorrelationRecord(), PriorReport(), (C.c_float * 2)(), C.c_float()
        rc = host_lib().flow2d_host_compute_flow_correlation_seeded(
            self.handle, _fptr(f0), _fptr(f1), int(radius), int(search), int(spacing), float(min_score), _fptr(u), _fptr(v),
            C.byref(params), float(reach), self._prior_level(level), _fptr(nodes[0]), _fptr(nodes[1]), _fptr(nodes[2]), C.byref(record),
            C.byref(report), _fptr(pu), _fptr(pv), lo_scale, C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowCorrelationSeeded")
        return {"u": u, "v": v, "report": report, "nodes": tuple(nodes), "record": record, "prior": (pu, pv),
                "lo_scale": (lo_scale[0], lo_scale[1]), "ms": ms.value}

    def compute_flow_correlation_seeded_device(self, dev_f0, dev_f1, dev_u, dev_v, params, lo, scale, radius=7, search=8, spacing=8,
                                               min_score=-1.0, reach=2.0, level=None, dev_nodes=None, dev_score=None, dev_prior=None):
        """OpticalFlow2D::ComputeFlowCorrelationSeededDevice: device frames in, the flow into (dev_u, dev_v).  dev_nodes (a (u, v)
        pair), dev_score and dev_prior (a (u, v) pair for the expanded field) are optional device planes of the container's size.
        Returns (PriorReport, CorrelationRecord); synchronises."""
        report, record = PriorReport(), CorrelationRecord()
        nd, pr = dev_nodes or (None, None), dev_prior or (None, None)
        rc = host_lib().flow2d_host_compute_flow_correlation_seeded_device(
            self.handle, dev_f0, dev_f1, float(lo), float(scale), int(radius), int(search), int(spacing), float(min_score), dev_u, dev_v,
            C.byref(params), float(reach), self._prior_level(level), nd[0], nd[1], dev_score, C.byref(record), C.byref(report), pr[0],
            pr[1])
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowCorrelationSeededDevice")
        return report, record

    def propagate_flow_device(self, dev_u, dev_v, dev_out_u, dev_out_v, dev_mask=None, dev_frame_from=None, dev_frame_to=None, step=1.0,
                              photo_scale=1.0, fill_passes=4, record=True):
        """OpticalFlow2D::PropagateFlowDevice: raw device addresses of pitched containers; workspace and record are the object's
        own.  With record the PropagateRecord is read back and returned (synchronises); without, the call only queues."""
        options = warm_options(fill_passes, photo_scale)
        rec = PropagateRecord() if record else None
        rc = host_lib().flow2d_host_propagate_flow_device(self.handle, dev_u, dev_v, dev_mask, dev_frame_from, dev_frame_to, float(step),
                                                          C.byref(options), dev_out_u, dev_out_v, C.byref(rec) if record else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::PropagateFlowDevice")
        return rec

    def compute_flow_from_previous(self, frame_0, frame_1, prev_u, prev_v, params, prev_mask=None, prev_frame=None, reach=2.0,
                                   level=None, fill_passes=4, photo_scale=1.0):
        """OpticalFlow2D::ComputeFlowFromPrevious: the flow of the host pair, warm-started from the previous pair's flow (prev_u,
        prev_v) -- the flow into frame_0 from the frame before it --, which is propagated onto frame_0's grid and then seeds the
        pyramid as in compute_flow_from_prior.  prev_frame: that earlier frame, which switches the photometric term on.
        Returns (u, v, WarmReport, device_ms)."""
        f0, f1 = self._pair(frame_0, frame_1)
        pu, pv = self._pair(prev_u, prev_v)
        mask = None if prev_mask is None else self._pair(prev_mask, prev_mask)[0]
        frame = None if prev_frame is None else self._pair(prev_frame, prev_frame)[0]
        options = warm_options(fill_passes, photo_scale)
        u, v = np.empty_like(f0), np.empty_like(f0)
        report, ms = WarmReport(), C.c_float()
        rc = host_lib().flow2d_host_compute_flow_from_previous(self.handle, _fptr(f0), _fptr(f1), _fptr(pu), _fptr(pv), _opt_fptr(mask),
                                                               _opt_fptr(frame), _fptr(u), _fptr(v), C.byref(params), float(reach),
                                                               self._prior_level(level), C.byref(options), C.byref(report), C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowFromPrevious")
        return u, v, report, ms.value

    def compute_flow_from_previous_device(self, dev_f0, dev_f1, dev_prev_u, dev_prev_v, dev_u, dev_v, params, dev_prev_mask=None,
                                          dev_prev_frame=None, reach=2.0, level=None, fill_passes=4, photo_scale=1.0, report=True):
        """OpticalFlow2D::ComputeFlowFromPreviousDevice: raw device addresses of pitched containers.  With report the WarmReport is
        returned (synchronises); without, the call only queues."""
        options = warm_options(fill_passes, photo_scale)
        rep = WarmReport() if report else None
        rc = host_lib().flow2d_host_compute_flow_from_previous_device(self.handle, dev_f0, dev_f1, dev_prev_u, dev_prev_v, dev_prev_mask,
                                                                      dev_prev_frame, dev_u, dev_v, C.byref(params), float(reach),
                                                                      self._prior_level(level), C.byref(options),
                                                                      C.byref(rep) if report else None)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowFromPreviousDevice")
        return rep

    def compute_flow_sequence_warm(self, frames, params, reach=2.0, level=None, fill_passes=4, photo_scale=1.0, tail=None):
        """OpticalFlow2D::ComputeFlowSequenceWarm: the flows of the host sequence [frame_count, height, width], pair 0 from zero
        and every later pair from its predecessor's flow propagated onto its grid.  tail: None -- every later pair is seeded with
        reach / level --, or the share in [0, 1) of the adaptive rule (warm_next_reach), which picks every pair's reach from how
        well the last prediction held and computes a pair again unseeded when its prior did not hold (reach <= 3, no level).
        The default is None: no table of measured sequences supports a particular tail yet.
        Returns (us, vs, [WarmReport], device_ms)."""
        fr = self._stack(frames)
        n = fr.shape[0]
        if n < 2:
            raise ValueError("a sequence has at least two frames")
        options = warm_options(fill_passes, photo_scale, tail)
        us, vs = np.empty((n - 1,) + fr.shape[1:], np.float32), np.empty((n - 1,) + fr.shape[1:], np.float32)
        reports, ms = (WarmReport * (n - 1))(), C.c_float()
        rc = host_lib().flow2d_host_compute_flow_sequence_warm(self.handle, _fptr(fr), n, _fptr(us), _fptr(vs), C.byref(params),
                                                               float(reach), self._prior_level(level), C.byref(options), reports,
                                                               C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowSequenceWarm")
        return us, vs, list(reports), ms.value

    def compute_flow_sequence_warm_device(self, dev_frames, dev_us, dev_vs, params, reach=2.0, level=None, fill_passes=4, photo_scale=1.0,
                                          tail=None, reports=False):
        """OpticalFlow2D::ComputeFlowSequenceWarmDevice: raw device addresses; flow k goes from dev_frames[k] to dev_frames[k + 1]
        into (dev_us[k], dev_vs[k]).  Without adaptation and without reports the call only queues.  Returns the list of WarmReport
        with reports, else None."""
        n = len(dev_frames)
        if n < 2 or len(dev_us) != n - 1 or len(dev_vs) != n - 1:
            raise ValueError("a sequence of n frames takes n - 1 flow plane pairs")
        options = warm_options(fill_passes, photo_scale, tail)
        reps = (WarmReport * (n - 1))() if reports else None
        rc = host_lib().flow2d_host_compute_flow_sequence_warm_device(self.handle, _ptr_array(dev_frames), n, _ptr_array(dev_us),
                                                                      _ptr_array(dev_vs), C.byref(params), float(reach),
                                                                      self._prior_level(level), C.byref(options), reps)
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::ComputeFlowSequenceWarmDevice")
        return list(reps) if reports else None

    def bidirectional_refuses_prior(self, params):
        """Whether ComputeFlowBidirectional refuses a bag that carries the keys of a prior flow (it has no backward prior)."""
        return host_lib().flow2d_host_bidirectional_refuses_prior(self.handle, C.byref(params)) == 1

    def stabilise_sequence(self, frames, params, reference_index=0, model=MOTION_AFFINE, sigma=0.5, iterations=5, masks=False,
                           fill=0.0):
        """OpticalFlow2D::StabiliseSequence: every host frame of `frames` ([frame_count, h, w]) brought onto the grid of
        frames[reference_index] along the composed global motions of consecutive pairs (flow2d_global_motion_2d,
        flow2d_warp_global_2d); `fill` where a frame has nothing to show.  Returns (frames [frame_count, h, w], the GlobalMotion
        records M(reference -> k))."""
        fr = self._stack(frames)
        out = np.empty_like(fr)
        motions = (GlobalMotion * max(fr.shape[0], 1))()
        ms = C.c_float()
        rc = host_lib().flow2d_host_stabilise_sequence(self.handle, _fptr(fr), fr.shape[0], int(reference_index), int(model),
                                                       float(sigma), int(iterations), int(bool(masks)), fill, _fptr(out), motions,
                                                       C.byref(params), C.byref(ms))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::StabiliseSequence")
        return out, list(motions)[:fr.shape[0]]

    def stabilise_sequence_device(self, dev_frames, dev_outputs, params, reference_index=0, model=MOTION_AFFINE, sigma=0.5,
                                  iterations=5, masks=False, fill=0.0):
        """OpticalFlow2D::StabiliseSequenceDevice: device frames in, frame k on the reference's grid into dev_outputs[k].
        Returns the GlobalMotion records M(reference -> k) (synchronises)."""
        n = len(dev_frames)
        if len(dev_outputs) != n:
            raise ValueError("n frames take n output planes")
        motions = (GlobalMotion * max(n, 1))()
        rc = host_lib().flow2d_host_stabilise_sequence_device(self.handle, _ptr_array(dev_frames), n, int(reference_index),
                                                              int(model), float(sigma), int(iterations), int(bool(masks)), fill,
                                                              _ptr_array(dev_outputs), motions, C.byref(params))
        if rc:
            raise Flow2DError(rc, "OpticalFlow2D::StabiliseSequenceDevice")
        return list(motions)[:n]

    def level_timings(self):
        """[(width, height, solve_ms, kernel_ms, kernel_launches, algorithmic_bytes_per_launch, algorithm)] per level;
        algorithm = the flow2d_solver_algorithm the level actually ran (never AUTO)."""
        cap = 8192
        buf = np.zeros(7 * cap, np.float32)
        n = host_lib().flow2d_host_level_timings(self.handle, _fptr(buf), cap)
        return [(int(buf[7 * i]), int(buf[7 * i + 1]), float(buf[7 * i + 2]), float(buf[7 * i + 3]),
                 int(buf[7 * i + 4]), float(buf[7 * i + 5]), int(buf[7 * i + 6])) for i in range(min(n, cap))]

    def use_graph(self, on=True):
        """Record the pyramid of a (buffers, parameters) combination once and replay it (HIP graph)."""
        host_lib().flow2d_host_use_graph(self.handle, int(on))

    def reset_timings(self):
        host_lib().flow2d_host_reset_timings(self.handle)

    def missing_key_leaves_outputs(self, key):
        return host_lib().flow2d_host_missing_key_leaves_outputs(self.handle, key.encode())

    def close(self):
        if self.handle:
            host_lib().flow2d_host_flow_destroy(self.handle)
            self.handle = None
            if self._adopted:  # the caller owns (and may now destroy) the adopted context
                host_lib().flow2d_host_adopt_context(None)


class OpticalFlowBatch:
    """OpticalFlowBatch2D of the host layer: independent pairs spread over `lanes` (stream + OpticalFlow2D + plane
    pool each) on one GPU; pair k of a call runs on lane (first_lane + k) mod lanes.  The scheduling is C++; this
    class only marshals device addresses."""

    def __init__(self, width, height, constancy=GREY, lanes=4, device=0, group_size=1):
        L = host_lib()
        self.width, self.height, self.group_size = width, height, group_size
        self.handle = L.flow2d_host_batch_create(width, height, _HOST_CONSTANCY[constancy], lanes, device, group_size)
        if not self.handle:
            raise Flow2DError(1, "OpticalFlowBatch2D::Initialize")
        self.pitch = L.flow2d_host_batch_pitch(self.handle)
        self.lanes = L.flow2d_host_batch_lanes(self.handle)
        # group_size > 1: every plane handed to compute_flow_batch_device is a tall container, pair g of the group
        # group_stride bytes * g behind its address (= pitch * height: the pairs' containers one below the other)
        self.group_stride = L.flow2d_host_batch_group_stride(self.handle)

    params = staticmethod(OpticalFlow.params)

    def use_graph(self, on=True):
        host_lib().flow2d_host_batch_use_graph(self.handle, int(on))

    def compute_flow_batch_device(self, dev_f0s, dev_f1s, dev_us, dev_vs, params, first_lane=0):
        """Raw device addresses of pitched containers, one entry per pair; queued, not synchronised."""
        n = len(dev_f0s)
        if not (len(dev_f1s) == len(dev_us) == len(dev_vs) == n):
            raise ValueError("one frame 0, frame 1, u and v plane per pair")
        arrays = [(C.c_void_p * n)(*a) for a in (dev_f0s, dev_f1s, dev_us, dev_vs)]
        rc = host_lib().flow2d_host_batch_compute(self.handle, n, *arrays, C.byref(params), first_lane)
        if rc:
            raise Flow2DError(rc, "OpticalFlowBatch2D::ComputeFlowBatchDevice")

    def compute_flow_batch_device_grouped(self, dev_f0s, dev_f1s, dev_us, dev_vs, params, first_lane=0):
        """Independent pairs (one container per plane); the object forms the lock-step groups (gather, group, hand back)."""
        n = len(dev_f0s)
        if not (len(dev_f1s) == len(dev_us) == len(dev_vs) == n):
            raise ValueError("one frame 0, frame 1, u and v plane per pair")
        arrays = [(C.c_void_p * n)(*a) for a in (dev_f0s, dev_f1s, dev_us, dev_vs)]
        rc = host_lib().flow2d_host_batch_compute_grouped(self.handle, n, *arrays, C.byref(params), first_lane)
        if rc:
            raise Flow2DError(rc, "OpticalFlowBatch2D::ComputeFlowBatchDeviceGrouped")

    def compute_flow_batch(self, frames_0, frames_1, flows_u, flows_v, params, first_lane=0):
        """OpticalFlowBatch2D::ComputeFlowBatch: HostImage objects in and out, uploads / downloads pipelined against the
        lanes' pyramids.  Queued: read the flows after synchronize()."""
        n = len(frames_0)
        if not (len(frames_1) == len(flows_u) == len(flows_v) == n):
            raise ValueError("one frame 0, frame 1, u and v image per pair")
        arrays = [(C.c_void_p * n)(*[q.handle for q in a]) for a in (frames_0, frames_1, flows_u, flows_v)]
        rc = host_lib().flow2d_host_batch_compute_host(self.handle, n, *arrays, C.byref(params), first_lane)
        if rc:
            raise Flow2DError(rc, "OpticalFlowBatch2D::ComputeFlowBatch")

    def synchronize(self):
        if host_lib().flow2d_host_batch_synchronize(self.handle) != 0:
            raise Flow2DError(2, "OpticalFlowBatch2D::Synchronize")

    def close(self):
        if self.handle:
            host_lib().flow2d_host_batch_destroy(self.handle)
            self.handle = None


class HostImage:
    """A Data2D of the host layer (tight row-major float32), in page-locked memory when pinned=True
    (HostMemory::Pinned).  `array` is a numpy view of its pixels, valid until close()."""

    def __init__(self, width, height, pinned=True, data=None):
        L = host_lib()
        self.handle = L.flow2d_host_data2d_create(width, height, int(pinned))
        if not self.handle:
            raise MemoryError("Data2D(%d, %d)" % (width, height))
        self.width, self.height = width, height
        self.pinned = bool(L.flow2d_host_data2d_is_pinned(self.handle))
        buf = (C.c_float * (width * height)).from_address(L.flow2d_host_data2d_ptr(self.handle))
        self.array = np.frombuffer(buf, np.float32).reshape(height, width)
        if data is not None:
            self.array[...] = data

    def close(self):
        if self.handle:
            self.array = None
            host_lib().flow2d_host_data2d_destroy(self.handle)
            self.handle = None


def read_raw(path, width, height, u8):
    out = np.empty((height, width), np.float32)
    rc = host_lib().flow2d_host_read_raw(path.encode(), width, height, int(u8), _fptr(out))
    return out if rc == 0 else None


def write_raw(image, path, u8):
    a = np.ascontiguousarray(image, np.float32)
    return host_lib().flow2d_host_write_raw(_fptr(a), a.shape[1], a.shape[0], int(u8), path.encode()) == 0


def read_flo(path):
    """A Middlebury .flo file (IOUtils::ReadFlowFLO) -> (u, v) float32 arrays.  ValueError when the file is refused."""
    L = host_lib()
    w, h = C.c_size_t(), C.c_size_t()
    if L.flow2d_host_read_flo(os.fsencode(path), C.byref(w), C.byref(h), None, None, 0):
        raise ValueError("%s: not a readable .flo file (bad magic, size or truncated)" % path)
    u = np.empty((h.value, w.value), np.float32)
    v = np.empty_like(u)
    if L.flow2d_host_read_flo(os.fsencode(path), C.byref(w), C.byref(h), _fptr(u), _fptr(v), u.size):
        raise ValueError("%s: changed while being read" % path)
    return u, v


def write_flo(path, u, v):
    """(u, v) as a Middlebury .flo file (IOUtils::WriteFlowFLO).  OSError when it cannot be written."""
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    if host_lib().flow2d_host_write_flo(_fptr(u), _fptr(v), u.shape[1], u.shape[0], os.fsencode(path)):
        raise OSError("cannot write %s" % path)


def evaluate_flow(u, v, gt_u, gt_v, occlusion=None, planes=False, device=0):
    """EvaluateFlow of the host layer on host arrays: uploads them, runs flow2d_flow_error_2d on the process-wide context
    (created on `device` when there is none) and returns the record as a dict (see Context.flow_error); planes=True also
    returns the per-pixel (epe, ae) arrays: (record, epe, ae)."""
    L = host_lib()
    arrays = [np.ascontiguousarray(a, np.float32) for a in (u, v, gt_u, gt_v)]
    occ = None if occlusion is None else np.ascontiguousarray(occlusion, np.float32)
    if arrays[0].ndim != 2 or any(a.shape != arrays[0].shape for a in arrays + ([occ] if occ is not None else [])):
        raise ValueError("every plane must be a 2-D array of one shape")
    if not L.flow2d_host_context() and L.flow2d_host_init_device(device) != 0:
        raise Flow2DError(2, "InitDeviceContext")
    h, w = arrays[0].shape
    epe = np.empty((h, w), np.float32) if planes else None
    ae = np.empty((h, w), np.float32) if planes else None
    rec = FlowErrorStats()
    rc = L.flow2d_host_flow_error(*[_fptr(a) for a in arrays], None if occ is None else _fptr(occ), w, h,
                                  None if epe is None else _fptr(epe), None if ae is None else _fptr(ae), C.byref(rec))
    if rc:
        raise Flow2DError(1 if rc == 1 else 3, "EvaluateFlow")
    return (_stats_dict(rec), epe, ae) if planes else _stats_dict(rec)


def compose_global_motion(first, second):
    """OpticalFlow2D::ComposeGlobalMotion: the GlobalMotion record of `second` after `first` (centred coordinates, double)."""
    out = GlobalMotion()
    rc = host_lib().flow2d_host_compose_global_motion(C.byref(first), C.byref(second), C.byref(out))
    if rc:
        raise Flow2DError(rc, "OpticalFlow2D::ComposeGlobalMotion")
    return out


def max_warp_level(width, height, scale):
    """OpticalFlowBase2D::GetMaxWarpLevel of the host layer (no device needed)."""
    return host_lib().flow2d_host_max_warp_level_static(width, height, scale)


def write_outputs(u, v, ppm_path, amp_path, flow_max_scale=10.0):
    u = np.ascontiguousarray(u, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    host_lib().flow2d_host_write_outputs(_fptr(u), _fptr(v), u.shape[1], u.shape[0], ppm_path.encode(),
                                         amp_path.encode(), flow_max_scale)


def convert_to_rgb(x, y):
    rgb = (C.c_int * 3)()
    host_lib().flow2d_host_convert_to_rgb(x, y, rgb)
    return tuple(rgb)


def load_settings(path):
    s = HostSettings()
    rc = host_lib().flow2d_host_load_settings(path.encode(), C.byref(s))
    return s if rc == 0 else None


class Operator:
    """One of the reference's six operator classes (CudaOperation*2D) behind its Initialize/Execute bag API.

    execute(**bag): every value is a ctypes object (c_ulonglong device pointer, c_size_t, c_float, DataSize3...)
    whose address is pushed under its keyword, exactly like OperationParameters::PushValuePtr."""

    def __init__(self, kind, container_width, container_height, pitch_bytes, constancy=GREY, ctx=None,
                 omit_container_size=False):
        L = host_lib()
        if ctx is not None:
            L.flow2d_host_adopt_context(ctx.handle)
        self.handle = L.flow2d_host_operator_create(kind.encode(), container_width, container_height, pitch_bytes,
                                                    constancy, int(omit_container_size))
        if not self.handle:
            raise Flow2DError(1, "CudaOperation%s2D::Initialize" % kind.capitalize())

    @property
    def name(self):
        return host_lib().flow2d_host_operator_name(self.handle).decode()

    def execute(self, **bag):
        keys = (C.c_char_p * len(bag))(*[k.encode() for k in bag])
        vals = (C.c_void_p * len(bag))(*[C.cast(C.pointer(v), C.c_void_p) for v in bag.values()])
        host_lib().flow2d_host_operator_execute(self.handle, keys, vals, len(bag))

    def close(self):
        if self.handle:
            host_lib().flow2d_host_operator_destroy(self.handle)
            self.handle = None


class DataSize3(C.Structure):
    _fields_ = [("width", C.c_size_t), ("height", C.c_size_t), ("pitch", C.c_size_t)]
