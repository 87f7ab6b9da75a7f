// flow2d: command-line front end of the MI355X optical-flow path.
// Keeps the argv forms, defaults, exit codes and output files of the reference's src/main.cpp:46-229:
//   flow2d                                   -> ./settings.xml
//   flow2d <settings.xml>
//   flow2d <file1> <file2> <width> <height> <prefix> <outdir/> [<alpha> <sigma>]     (argc 7 / 9)
//   flow2d <file1> <file2> <width> <height> <outdir/>                                (argc 6)
// exit codes: 1 no device, 2 frame load failed, 3 settings error, 4 the flow computation failed, 5 bad option value (refused
// before the device is opened), 255 cannot write PPM/amp, 0 otherwise.
// Documented supersets: imageType="8-bit" selects the u8 reader; inputPath is tried as
// a prefix before the bare file name; argc == 6 no longer dereferences argv[6]; no blocking getchar();
// options --u8, --gradient, --log-derivatives, --device N, --verbose, --sor OMEGA (opt-in red-black SOR, no reference parity),
// --backward (also the backward flow and forward-backward occlusion masks, see below) may precede the positional arguments.
// --backward writes, besides the unchanged forward files, <prefix>flow-u-backward-W-H.raw, <prefix>flow-v-backward-W-H.raw
// (the flow frame 2 -> frame 1), <prefix>occlusion-W-H.raw (frame 1's grid) and <prefix>occlusion-backward-W-H.raw (frame 2's
// grid) as F32 0 / 1 (1 = occluded or leaving the frame), and <prefix>occlusion.pgm (P5, 255 where frame 1 is occluded).
// --flo also writes the flow as Middlebury .flo: <prefix>flow.flo, and <prefix>flow-backward.flo with --backward.
// --ground-truth FILE.flo loads the true flow of frame 1 -> frame 2 before computing (exit code 2 when it is missing, malformed
// or not of the frames' size) and after the run prints one line "Flow error: {json}": the flow2d_flow_error_2d metrics of the
// forward flow (FlowErrorJson, flow_evaluation.h) over all pixels and split into noc / occ by the forward occlusion mask of
// --backward (without it every pixel is noc).  Neither option changes any other file or output.
// --interpolate N (an integer >= 2) also writes the N - 1 frames between frame 1 and frame 2 at t = k / N, k = 1 .. N - 1, as
// F32 <prefix>interp-<k>-of-<N>-W-H.raw: OpticalFlow2D::InterpolateFrames (flow2d_interpolate_2d) with both flows, both
// occlusion masks, 2 fixed-point iterations and a residual bound of 0.5 px.  The forward files do not change; the backward
// files are written only with --backward.
// --track S (an integer >= 1) also seeds frame 1 on a grid of spacing S and tracks the points into frame 2
// (OpticalFlow2D::TrackPoints: flow2d_seed_points_2d with the default texture threshold, flow2d_track_points_2d with the paper's
// thresholds), writes <prefix>tracks.txt -- one line per track, "x1 y1 x2 y2", nan where the track has no position -- and prints
// the alive, ended and seeded counts.  The other files do not change.
// --denoise SIGMA (a finite number >= 0, grey levels; 0 = no photometric weight) also fuses each of the two frames with the other
// along the flow between them (OpticalFlow2D::DenoiseSequence: radius 1, occlusion masks on, flow2d_denoise_2d) and writes
// <prefix>denoised-1-W-H.raw and <prefix>denoised-2-W-H.raw in the input's raw type (u8 or F32).  The other files do not change.
// It is a run of its own after the files above are written: the pair's flows are computed a second time, in both directions.
// --global-motion MODEL (translation, similarity or affine) [--global-sigma S, a finite number >= 0 in pixels, default 0.5; 0:
// plain least squares] [--global-iterations K, 0 .. 16, default 5] also fits the global motion of the pair
// (OpticalFlow2D::EstimateGlobalMotion: flow2d_global_motion_2d on the forward flow; with --backward the forward occlusion
// mask leaves its vectors out) and prints one line "Global motion: {json}" -- "model", "model_used", the six parameters "p" of
// u = (p0 + p1*xc) + p2*yc, v = (p3 + p4*xc) + p5*yc in centred coordinates with 17 significant digits, "weight_sum" and
// "support" --, writes the flow without the global motion as <prefix>residual-u-W-H.raw and <prefix>residual-v-W-H.raw (F32, NaN
// where the flow is not finite) and, with --flo, <prefix>residual.flo.  The other files do not change; a run of its own, too.
// --segment-motion THRESHOLD (pixels, >= 0; needs --global-motion) [--segment-join J, >= 0 or inf, default inf] [--segment-min-area
// A, >= 1, default 16] also labels the independently moving regions of the pair (OpticalFlow2D::SegmentMotion:
// flow2d_segment_motion_2d on the residual flow; with --backward the forward occlusion mask is left out) and prints one line
// "Motion segmentation: {json}" -- "regions", "foreground", "dropped", "recorded" -- and one line "Region k: {json}" per recorded
// region -- "area", "bbox" [x0, y0, x1, y1], "centroid" and "motion" (the mean residual motion in pixels) with 17 significant
// digits --, and writes the labels as <prefix>labels-W-H.raw (32-bit integers).  The other files do not change; a run of its own.
// --deformation [--strain small|green, default small] [--deformation-sigma S, a number in [0, 8.66] in pixels, default 0: no
// smoothing] also analyses how the material deforms between the two frames (OpticalFlow2D::AnalyseDeformation: the forward flow,
// smoothed by a Gaussian of S pixels when S > 0, through flow2d_deformation_2d; with --backward the forward occlusion mask keeps
// differences from reaching across an occlusion boundary), writes the nine planes as <prefix>divergence-W-H.raw, vorticity,
// dilatation, exx, eyy, exy, e1, e2 and max-shear likewise (F32, NaN where a pixel has no derivative) and prints one line
// "Deformation: {json}" -- "measure", "sigma", "valid", "invalid" and per quantity "mean", "rms", "min", "max" with 17 significant
// digits.  The other files do not change; a run of its own.
// --refine R (a radius of 1 .. 7) [--refine-sigma S, grey levels, finite and >= 0, default 25; 0: no guide weight] [--refine-space P,
// pixels, finite and >= 0, default 0: no spatial weight] [--refine-iterations K, 1 .. 16, default 1] refines the forward flow
// before it is written (OpticalFlow2D::RefineFlow: K passes of flow2d_refine_flow_2d, the weighted median over a (2R + 1)^2
// window guided by frame 1; with --backward the forward occlusion mask takes unreliable vectors out and they are filled in from
// their surroundings): the forward files -- flow-u, flow-v, res.pgm, amp, flow.flo -- then hold the refined flow, and one line
// "Refinement: {json}" -- "radius", "sigma", "space", "iterations" and the last pass's "pixels", "unfilled", "filled", "changed" --
// is printed.  With --ground-truth the line "Flow error: {json}" scores the refined flow and a second line "Flow error before
// refinement: {json}" the flow as computed.  The other files do not change; a run of its own.  Without --refine nothing changes.
// --correlation R (a window radius of 1 .. 15) [--correlation-range D, 1 .. 32, default 8] [--correlation-spacing S, 1 .. 64,
// default 8] [--correlation-min-score C, a number, default -1: off] selects Methods::Correlation instead of the variational flow
// (OpticalFlow2D::Correlate: flow2d_correlate_2d on the frames quantised to 8 bits over their common range, as they are when that
// lies in [0, 255]): the forward files -- flow-u, flow-v, res.pgm, amp, flow.flo -- hold the node field expanded to the frame's
// grid (NaN where no surrounding node is valid), node-u, node-v and node-score (F32, nw x nh, the sizes in the names) the nodes,
// and one line "Correlation: {json}" -- "radius", "range", "spacing", "min_score", "lo", "scale", "nw", "nh" and the record's
// "nodes", "invalid", "rejected", "unrefined" -- is printed.  With --ground-truth the line "Flow error: {json}" scores the expanded
// field.  It does not combine with the options that run the variational flow (--backward, --interpolate, --track, --denoise,
// --global-motion, --segment-motion, --deformation, --refine).  Without --correlation nothing changes.
// --correlation-passes R:D:S[,R:D:S...] (1 .. 6 passes, coarse to fine) [--validate-threshold T, default 2] [--validate-epsilon E,
// default 0.1] [--validate-min-neighbours K, 1 .. 8, default 3] [--validate-flag-only] [--correlation-min-score C] runs the multi-pass
// window correlation (OpticalFlow2D::CorrelateMultiPass: every pass searches around the validated, expanded field of the one
// before; --initial-flow FILE.flo, accepted with it, is the first pass's predictor) instead of the variational flow.  The files are
// those of --correlation, from the last pass (whose outliers --validate-flag-only leaves as NaN instead of replacing them), and
// one line "CorrelationPasses: {json}" -- the options and, per pass, the grid and both records -- is printed.  It excludes
// --correlation and everything that runs or seeds the variational flow.  Without it nothing changes.
// --subset-refine R (a subset radius of 1 .. 15) [--subset-iterations K, 1 .. 64, default 20] [--subset-epsilon E, >= 0, default
// 1e-3] [--subset-max-shift M, > 0, default 2] [--subset-max-gradient G, > 0, default 0.5], valid only together with --correlation or
// --correlation-passes, refines the nodes of the (last) pass by subsets (OpticalFlow2D::CorrelateSubset: the pass is validated with
// replacement so that every node has a start, then flow2d_subset_refine_2d -- the affine Gauss-Newton iteration of digital image
// correlation on the unquantised frames): node-u, node-v and the forward files then hold the refined field, node-score the
// subsets' scores, and node-ux, node-uy, node-vx, node-vy (the displacement gradients) and node-state are written beside them.
// With --subset-order 2 [--subset-max-curvature C, > 0, default 0.05] the refinement is the second-order one
// (flow2d_subset_refine2_2d, R from 2): node-uxx, node-uxy, node-uyy, node-vxx, node-vxy and node-vyy are written beside the node files
// and one more line, "SubsetOrder: {json}", is printed; --subset-order 1 is the run without the option.
// One line "Subset: {json}" -- the options, the grid, "lo", "scale" and the record's "nodes", "converged", "unconverged", "strayed",
// "flat", "no_input", "iterations_run" -- is printed in place of the "Correlation:" / "CorrelationPasses:" line.  Without the option
// nothing changes.
// --subset-strain M (a strain window of 0 .. 7 nodes) [--strain-order 1|2, default 1] [--strain-min-nodes N, default 0: one more
// than the fit has coefficients] takes the strain of the node field (OpticalFlow2D::NodeStrain, flow2d_node_strain_2d): with
// --subset-refine, on the pair chain and on --subset-previous, of the refined nodes with their states (M = 0: the subsets' own
// gradients; M >= 1: a polynomial of the order fitted by least squares to the usable nodes within M nodes); with --correlation or
// --correlation-passes alone and M >= 1, of the search's nodes, every finite one usable.  --strain small|green selects the measure.
// node-divergence, node-vorticity, node-dilatation, node-exx, node-eyy, node-exy, node-e1, node-e2 and node-max-shear are written
// beside the node files, and the record is printed as "NodeStrain: {...}".
// --strain-sigma S (pixels, finite and > 0) [--strain-iterations K, 0 .. 16, default 8], with --subset-strain M and M >= 1, makes the
// window fit the robust one (flow2d_node_strain_robust_2d): K reweighted passes with a Cauchy weight of scale S, so that a node
// which converged to a wrong place does not bend the windows that hold it.  node-strain-residual, node-strain-rejected and
// node-strain-centre are written beside the nine files and one more line, "NodeStrainRobust: {json}" -- "sigma", "iterations" and
// the record's "touched" (nodes that rejected a tap), "rejected" (taps) and "suspect" (nodes whose own tap was not kept) -- is
// printed behind "NodeStrain:", which keeps its format.  Without the option nothing changes.
// --strain-weighted [--strain-sigma-floor F, pixels, default 0] [--strain-threshold T, sigmas, default 0: no robust part]
// [--strain-iterations K, with T > 0, default 8], with --subset-uncertainty and --subset-strain M, M >= 1, weights every tap of the
// window fit by 1 / (sigma^2 + F^2) of its node (flow2d_node_strain_weighted_2d), taken from the uncertainty that is computed first.
// The three diagnostic files (residual and centre in sigmas) and node-sigma-exx, -eyy, -exy, -divergence, -vorticity and
// node-sigma-strain-ux, -uy, -vx, -vy (the fitted gradients' sigmas; node-sigma-ux ... are the subsets' own) are written beside the
// nine files, and one more line, "WeightedStrain: {json}" with the record's four counts.  Not together with --strain-sigma.
// --subset-previous PREFIX [--subset-fill F, 1 .. 4, default 2] [--subset-min-state 0|1, default 1] [--subset-predict-neighbours N,
// 1 .. 8, default 1], valid only together with --subset-refine, is the next step of a loading sequence: FILE_0 is the sequence's
// reference frame, FILE_1 its current frame, and PREFIXnode-u-NW-NH.raw, -v, -ux, -uy, -vx, -vy and -state are what a --subset-refine
// run of the previous frame wrote under PREFIX (a missing file or another grid is refused like the other bad inputs).  In place of
// the search, F passes of flow2d_predict_nodes_2d build the start from them and flow2d_subset_refine_from_2d refines it
// (OpticalFlow2D::ContinueSubsetSequence), with --subset-max-shift defaulting to 4; the (last) pass of --correlation... gives the grid
// only.  One line "Prediction: {json}" -- the options and per pass "nodes", "kept", "predicted", "empty" -- is printed before the
// "Subset:" line, whose "passes" is then 0.  Without the option nothing changes.
// --subset-base PREFIX, valid only together with --subset-refine (with or without --subset-previous), is a step of a sequence whose
// reference frame has moved: FILE_0 is the current reference frame r, not frame 0, and PREFIXnode-u-NW-NH.raw, -v, -ux, -uy, -vx, -vy
// and -state are the field frame 0 -> frame r on this grid (what an earlier run delivered for frame r; refill its holes first if it
// is to serve many steps).  The refined field, frame r -> FILE_1, is the *increment*: its files are written with "increment-" in front
// of their names (increment-node-u-NW-NH.raw, ...), so that the next run's --subset-previous can start from them, and the node files
// themselves are the composition of base and increment (OpticalFlow2D::ComposeNodes, flow2d_compose_nodes_2d, with the least state
// of --subset-previous's --subset-min-state, 1 without it): frame 0 -> FILE_1 at the nodes of frame 0, state 66 or -1, the score blended.  --subset-strain works on the
// composed field; the dense flow files stay the increment's.  One more line, "Compose: {json}" -- "nodes", "composed", "no_base",
// "outside", "no_increment" -- is printed.  With --subset-order 2 the curvatures are the increment's alone.  Without the option
// nothing changes.
// --subset-mask FILE [--subset-mask-invert] [--subset-min-pixels N, 6 .. (2R + 1)^2, default a quarter of the subset], valid only
// together with --subset-refine (order 1), is digital image correlation on a region of interest (flow2d_subset_refine_masked_2d): FILE
// is a raw image of the frames' size and format, read like them, in FILE_0's coordinates, whose values of 0.5 and more mean "not the
// specimen"; with --subset-mask-invert it is a region image, non-zero meaning "inside".  A subset is refined on its usable pixels; a
// node off the specimen, or with fewer than N usable pixels, is masked: state -4 and NaN in the node files.  One more line,
// "SubsetMask: {json}" -- "masked", the masked nodes, and "min_pixels" -- is printed.  Without the option no byte of any output changes.
// --correlation-mask FILE [--correlation-mask-invert] [--correlation-min-pixels N, 1 .. (2r + 1)^2 of every pass, default a quarter
// of each pass's window], valid only together with --correlation-passes and without --subset-refine, is the window search on a
// region of interest (OpticalFlow2D::ValidationOptions::mask: flow2d_correlate_masked_2d and flow2d_validate_nodes_masked_2d in every
// pass): FILE as for --subset-mask.  A window is correlated on its specimen pixels alone; a node whose centre is off the specimen, or
// whose window keeps fewer than N pixels, is masked: NaN in the node files, no vote in the median test.  One more line,
// "CorrelationMask: {json}" -- "min_pixels" as given (0: the default) and per pass "min_pixels", "masked" (the search's masked nodes)
// and "validation_masked" (the nodes off the specimen) -- is printed behind the "CorrelationPasses:" line.
// --subset-mask-search, valid only together with --subset-mask and not with --subset-previous (which runs no passes), hands the
// subset mask to the passes in front of the refinement (OpticalFlow2D::SubsetOptions::mask_search), so that an edge node starts from
// the specimen's motion; the "CorrelationMask:" line is printed before the "SubsetMask:" line.  Without these options no byte of any
// output changes.
// --subset-uncertainty, valid only together with --subset-refine at order 1 and not with --subset-base (a composed field's covariance
// would need both fields'), on the pair chain and on --subset-previous: the covariance s2 * H^-1 of every refined node
// (flow2d_subset_uncertainty_2d, with the refinement's radius, mask and interpolation).  node-sigma-u, node-sigma-v, node-rho,
// node-sigma-ux, -uy, -vx, -vy and node-noise are written beside the node files, and one more line, "SubsetUncertainty: {json}" with
// the counts, is printed last.  The sigmas estimate the random error from the frames' noise, not the interpolation bias.  Without
// the option no byte of any output changes.
// --subset-interpolation catmull-rom|bspline, valid only together with --subset-refine, says how frame 1 is sampled
// (OpticalFlow2D::SubsetOptions::interpolation): with bspline the run prefilters FILE_1 into its cubic B-spline coefficients
// (flow2d_bspline_prefilter_2d) and refines with flow2d_subset_refine_spline_2d or, with --subset-order 2,
// flow2d_subset_refine2_spline_2d; it goes with --subset-mask and --subset-previous.  One more line, "SubsetInterpolation: {json}" --
// "interpolation" and, for bspline, "horizon" -- is printed.  Without the option no byte of any output changes.
// --initial-flow FILE.flo | --correlation-prior R  [--prior-reach P, pixels, finite and > 0, default 2] [--prior-level L, >= 0]
// start the variational pyramid from a prior flow instead of from zero at its coarsest level (OpticalFlow2D::ComputeFlowFromPrior /
// ComputeFlowCorrelationSeeded): the prior is a Middlebury file of the frames' size, or the window correlation of the pair with
// radius R (and --correlation-range / --correlation-spacing / --correlation-min-score as for --correlation) expanded to the frame's
// grid.  The pyramid starts at the smallest level l with P * scale^l <= 1 (or at L), prior pixels that are not finite enter as zero.
// The forward files are the usual ones, and one line "Prior: {json}" -- "source", "reach", "start_level", "levels_run",
// "not_finite" and, for the correlation, "radius", "range", "spacing", "min_score", "lo", "scale", "nw", "nh" and the record's
// "nodes", "invalid", "rejected", "unrefined" -- is printed.  The two sources exclude each other, and both exclude --correlation
// and every option that runs flows of its own (--backward, --interpolate, --track, --denoise, --global-motion, --segment-motion,
// --deformation, --refine): there is no prior for a backward flow.  Without these options nothing changes.
// --previous-flow FILE.flo [--previous-frame FILE] [--propagate-fill N, 0 .. 64, default 4] [--prior-reach P] [--prior-level L] is the
// warm start of a pair inside a sequence (OpticalFlow2D::ComputeFlowFromPrevious): FILE.flo is the flow of the PREVIOUS pair -- from
// the frame before frame 1 into frame 1 --, which is carried along itself onto frame 1's grid (flow2d_propagate_flow_2d, N fill
// passes) and then seeds the pyramid like --initial-flow.  --previous-frame names that earlier frame (a raw file like the frames):
// where two vectors land on one pixel, the one whose source matches frame 1 better wins.  Two lines are printed: "Propagation:
// {json}" -- "fill", "photometric" and the record's "pixels", "unusable", "left", "landed", "holes", "filled", "unfilled" -- and
// "Prior: {json}" with the source "previous-flow".  It excludes --initial-flow, --correlation-prior, --correlation and every option
// that runs flows of its own, as --initial-flow does.  Without these options nothing changes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "device_utils.h"
#include "flow_evaluation.h"
#include "io_utils.h"
#include "optical_flow_2d.h"
#include "settings.h"

using namespace OpticFlow;

static bool LoadFrame(Data2D& frame, const std::string& input_path, const std::string& name, bool u8, size_t w,
                      size_t h)
{
    std::vector<std::string> candidates;
    if (!input_path.empty()) candidates.push_back(input_path + name);
    candidates.push_back(name);
    for (const std::string& path : candidates) {
        std::FILE* probe = std::fopen(path.c_str(), "rb");
        if (!probe) continue;
        std::fclose(probe);
        return u8 ? frame.ReadRAWFromFileU8(path.c_str(), w, h) : frame.ReadRAWFromFileF32(path.c_str(), w, h);
    }
    std::printf("Cannot open file '%s'.\n", name.c_str());
    return false;
}

// The line a masked chain of passes adds, "CorrelationMask: {json}": min_pixels as given (0: the default per pass) and, per pass, the
// min_pixels it ran with and the masked counts of the search and of the validation (the records' seventh words).
static void print_correlation_mask(const std::vector<OpticalFlow2D::CorrelationPass>& passes,
                                   const std::vector<OpticalFlow2D::CorrelationPassReport>& reports,
                                   const OpticalFlow2D::ValidationOptions& validation)
{
    std::printf("CorrelationMask: {\"min_pixels\": %d, \"passes\": [", validation.min_pixels);
    for (size_t k = 0; k < reports.size(); ++k)
        std::printf("%s{\"min_pixels\": %d, \"masked\": %llu, \"validation_masked\": %llu}", k ? ", " : "",
                    OpticalFlow2D::CorrelationMinPixels(validation, passes[k].radius), reports[k].correlation.reserved[0],
                    reports[k].validation.reserved[0]);
    std::printf("]}\n");
}

int main(int argc, char** argv)
{
    // optional flags first (supersets), then the reference's positional forms
    bool force_u8 = false, verbose = false, backward = false, write_flo = false;
    int interpolate = 0;  // --interpolate N: N - 1 frames between the two (0: off)
    long track_spacing = 0;  // --track S: seed frame 1 at spacing S and track into frame 2 (0: off)
    bool denoise = false;  // --denoise SIGMA: each frame fused with the other
    float denoise_sigma = 0.f;
    int global_model = -1;  // --global-motion MODEL (-1: off)
    double global_sigma = 0.5;
    int global_iterations = 5;
    bool segment = false;  // --segment-motion THRESHOLD
    float segment_threshold = 0.f, segment_join = INFINITY;
    unsigned segment_min_area = 16;
    bool deformation = false;  // --deformation
    int strain_measure = FLOW2D_STRAIN_SMALL;
    float deformation_sigma = 0.f;
    int refine_radius = 0;  // --refine R (0: off)
    float refine_sigma = 25.f, refine_space = 0.f;
    int refine_iterations = 1;
    Methods method = Methods::OpticalFlow;  // --correlation R: Methods::Correlation
    int correlation_radius = 0, correlation_range = 8, correlation_spacing = 8;
    float correlation_min_score = -1.f;
    std::vector<OpticalFlow2D::CorrelationPass> correlation_passes;  // --correlation-passes R:D:S[,R:D:S...]
    OpticalFlow2D::SubsetOptions subset;  // --subset-refine R and the --subset-* options
    bool subset_refine = false, subset_option = false;
    bool subset_uncertainty = false;  // --subset-uncertainty
    bool subset_interpolation_given = false;  // --subset-interpolation catmull-rom|bspline
    OpticalFlow2D::SequenceOptions sequence;  // --subset-previous PREFIX and its options
    std::string subset_previous;
    std::string subset_base;  // --subset-base PREFIX: the field up to the reference frame, composed with the refined one
    bool sequence_option = false, subset_max_shift_given = false, subset_curvature_given = false;
    std::string subset_mask_file;  // --subset-mask FILE, --subset-mask-invert, --subset-min-pixels N
    bool subset_mask_invert = false, subset_mask_option = false;
    std::string correlation_mask_file;  // --correlation-mask FILE, --correlation-mask-invert, --correlation-min-pixels N
    bool correlation_mask_invert = false, correlation_mask_option = false;
    int correlation_min_pixels = 0;
    OpticalFlow2D::StrainOptions node_strain;  // --subset-strain M and --strain-order, --strain-min-nodes, --strain-sigma, --strain-iterations
    bool strain_iterations_given = false;
    bool strain_floor_given = false, strain_threshold_given = false;  // --strain-sigma-floor, --strain-threshold (with --strain-weighted)
    bool subset_strain = false, strain_option = false;
    OpticalFlow2D::ValidationOptions validation;                     // --validate-threshold / -epsilon / -min-neighbours / -flag-only
    bool validate_option = false;
    std::string initial_flow_file;  // --initial-flow FILE.flo
    int prior_radius = 0;           // --correlation-prior R (0: off)
    float prior_reach = 2.f;
    int prior_level = -1;
    bool prior_option = false;  // --prior-reach or --prior-level was given
    std::string previous_flow_file, previous_frame_file;  // --previous-flow FILE.flo, --previous-frame FILE
    int propagate_fill = 4;
    bool previous_option = false;  // --previous-frame or --propagate-fill was given
    std::string ground_truth_file;
    int device = 0;
    float sor_omega = 0.f;
    DataConstancy data_constancy = DataConstancy::Grey;
    std::vector<char*> args = {argv[0]};
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--u8")) force_u8 = true;
        else if (!std::strcmp(argv[i], "--gradient")) data_constancy = DataConstancy::Gradient;
        else if (!std::strcmp(argv[i], "--gradient-untiled")) data_constancy = DataConstancy::GradientUntiled;
        else if (!std::strcmp(argv[i], "--log-derivatives")) data_constancy = DataConstancy::LogDerivatives;
        else if (!std::strcmp(argv[i], "--verbose")) verbose = true;
        else if (!std::strcmp(argv[i], "--backward")) backward = true;
        else if (!std::strcmp(argv[i], "--flo")) write_flo = true;
        else if (!std::strcmp(argv[i], "--ground-truth") && i + 1 < argc) ground_truth_file = argv[++i];
        else if (!std::strcmp(argv[i], "--interpolate")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 2 || n > 1000000) {
                std::printf("--interpolate takes an integer N >= 2 (the frames at t = k / N, k = 1 .. N - 1).\n");
                return 5;
            }
            interpolate = static_cast<int>(n);
            ++i;
        }
        else if (!std::strcmp(argv[i], "--track")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 || n > 1000000) {
                std::printf("--track takes an integer spacing S >= 1 (the seeding grid of frame 1).\n");
                return 5;
            }
            track_spacing = n;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--denoise")) {
            char* end = nullptr;
            const float sigma = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(sigma) || sigma < 0.f) {
                std::printf("--denoise takes a finite SIGMA >= 0 (grey levels; 0: no photometric weight).\n");
                return 5;
            }
            denoise = true;
            denoise_sigma = sigma;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--global-motion")) {
            static const char* const names[3] = {"translation", "similarity", "affine"};
            for (int m = 0; m < 3 && i + 1 < argc; ++m)
                if (!std::strcmp(argv[i + 1], names[m])) global_model = m;
            if (global_model < 0) {
                std::printf("--global-motion takes a MODEL: translation, similarity or affine.\n");
                return 5;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--global-sigma")) {
            char* end = nullptr;
            const double sigma = (i + 1 < argc) ? std::strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(sigma) || sigma < 0.0) {
                std::printf("--global-sigma takes a finite S >= 0 (pixels; 0: plain least squares).\n");
                return 5;
            }
            global_sigma = sigma;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--global-iterations")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 0 || n > FLOW2D_GLOBAL_MOTION_MAX_ITERATIONS) {
                std::printf("--global-iterations takes an integer K, 0 .. %d (reweighted passes).\n", FLOW2D_GLOBAL_MOTION_MAX_ITERATIONS);
                return 5;
            }
            global_iterations = static_cast<int>(n);
            ++i;
        }
        else if (!std::strcmp(argv[i], "--segment-motion") || !std::strcmp(argv[i], "--segment-join")) {
            const bool is_join = !std::strcmp(argv[i], "--segment-join");
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(value >= 0.f) || (!is_join && !std::isfinite(value))) {
                std::printf(is_join ? "--segment-join takes a J >= 0 (pixels; inf: plain labelling).\n"
                                    : "--segment-motion takes a finite THRESHOLD >= 0 (pixels).\n");
                return 5;
            }
            if (is_join) segment_join = value;
            else {
                segment = true;
                segment_threshold = value;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--segment-min-area")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 || n > 2147483647L) {
                std::printf("--segment-min-area takes an integer A >= 1 (pixels).\n");
                return 5;
            }
            segment_min_area = static_cast<unsigned>(n);
            ++i;
        }
        else if (!std::strcmp(argv[i], "--deformation")) deformation = true;
        else if (!std::strcmp(argv[i], "--strain")) {
            if (i + 1 < argc && !std::strcmp(argv[i + 1], "small")) strain_measure = FLOW2D_STRAIN_SMALL;
            else if (i + 1 < argc && !std::strcmp(argv[i + 1], "green")) strain_measure = FLOW2D_STRAIN_GREEN_LAGRANGE;
            else {
                std::printf("--strain takes small or green (the small-strain tensor or the Green-Lagrange one).\n");
                return 5;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--deformation-sigma")) {
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(value >= 0.f) || !(value < 26.f / 3.f)) {
                std::printf("--deformation-sigma takes an S in [0, 8.66] (pixels; 0: no smoothing).\n");
                return 5;
            }
            deformation_sigma = value;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--refine") || !std::strcmp(argv[i], "--refine-iterations")) {
            const bool radius = !std::strcmp(argv[i], "--refine");
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 ||
                n > (radius ? FLOW2D_REFINE_MAX_RADIUS : OpticalFlow2D::kRefineMaxIterations)) {
                if (radius) std::printf("--refine takes a window radius R of 1 .. %d.\n", FLOW2D_REFINE_MAX_RADIUS);
                else std::printf("--refine-iterations takes an integer K of 1 .. %d.\n", OpticalFlow2D::kRefineMaxIterations);
                return 5;
            }
            (radius ? refine_radius : refine_iterations) = static_cast<int>(n);
            ++i;
        }
        else if (!std::strcmp(argv[i], "--refine-sigma") || !std::strcmp(argv[i], "--refine-space")) {
            const bool guide = !std::strcmp(argv[i], "--refine-sigma");
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(value) || value < 0.f) {
                std::printf("%s takes a finite number >= 0 (%s; 0: that weight is off).\n", argv[i], guide ? "grey levels" : "pixels");
                return 5;
            }
            (guide ? refine_sigma : refine_space) = value;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--initial-flow") && i + 1 < argc) initial_flow_file = argv[++i];
        else if (!std::strcmp(argv[i], "--previous-flow") && i + 1 < argc) previous_flow_file = argv[++i];
        else if (!std::strcmp(argv[i], "--previous-frame") && i + 1 < argc) {
            previous_frame_file = argv[++i];
            previous_option = true;
        }
        else if (!std::strcmp(argv[i], "--propagate-fill")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 0 || n > FLOW2D_PROPAGATE_MAX_FILL) {
                std::printf("--propagate-fill takes an integer of 0 .. %d (passes that fill the holes of the propagated flow).\n",
                            FLOW2D_PROPAGATE_MAX_FILL);
                return 5;
            }
            propagate_fill = static_cast<int>(n);
            previous_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--prior-reach")) {
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(value) || !(value > 0.f)) {
                std::printf("--prior-reach takes a finite number > 0 (pixels the solver is trusted to correct the prior by).\n");
                return 5;
            }
            prior_reach = value;
            prior_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--prior-level") || !std::strcmp(argv[i], "--correlation-prior")) {
            const bool level = !std::strcmp(argv[i], "--prior-level");
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < (level ? 0 : 1) || n > (level ? 1000 : FLOW2D_CORRELATION_MAX_RADIUS)) {
                if (level) std::printf("--prior-level takes an integer L >= 0 (the pyramid level the prior enters at).\n");
                else std::printf("--correlation-prior takes a window radius of 1 .. %d.\n", FLOW2D_CORRELATION_MAX_RADIUS);
                return 5;
            }
            (level ? prior_level : prior_radius) = static_cast<int>(n);
            if (level) prior_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--correlation") || !std::strcmp(argv[i], "--correlation-range") ||
                 !std::strcmp(argv[i], "--correlation-spacing")) {
            const int which = !std::strcmp(argv[i], "--correlation") ? 0 : !std::strcmp(argv[i], "--correlation-range") ? 1 : 2;
            const int limit[3] = {FLOW2D_CORRELATION_MAX_RADIUS, FLOW2D_CORRELATION_MAX_RANGE, FLOW2D_CORRELATION_MAX_SPACING};
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 || n > limit[which]) {
                std::printf("%s takes an integer of 1 .. %d.\n", argv[i], limit[which]);
                return 5;
            }
            (which == 0 ? correlation_radius : which == 1 ? correlation_range : correlation_spacing) = static_cast<int>(n);
            if (which == 0) method = Methods::Correlation;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--correlation-passes")) {
            const char* p = (i + 1 < argc) ? argv[i + 1] : "";
            bool ok = *p != '\0';
            while (ok && *p) {
                int value[3] = {0, 0, 0};
                for (int k = 0; ok && k < 3; ++k) {
                    char* end = nullptr;
                    const long n = std::strtol(p, &end, 10);
                    ok = end != p && n >= 1 && n <= 64 && *end == (k < 2 ? ':' : (*end == ',' ? ',' : '\0'));
                    value[k] = static_cast<int>(n);
                    p = ok && *end ? end + 1 : end;
                }
                ok = ok && (*p || p[-1] != ',');
                if (ok) correlation_passes.push_back({value[0], value[1], value[2]});
            }
            if (!ok || correlation_passes.size() > FLOW2D_CORRELATION_MAX_PASSES) {
                std::printf("--correlation-passes takes 1 .. %d passes RADIUS:RANGE:SPACING separated by commas, coarse to fine.\n",
                            FLOW2D_CORRELATION_MAX_PASSES);
                return 5;
            }
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-refine") || !std::strcmp(argv[i], "--subset-iterations")) {
            const bool radius = !std::strcmp(argv[i], "--subset-refine");
            const int limit = radius ? FLOW2D_SUBSET_MAX_RADIUS : FLOW2D_SUBSET_MAX_ITERATIONS;
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 || n > limit) {
                std::printf("%s takes an integer of 1 .. %d.\n", argv[i], limit);
                return 5;
            }
            (radius ? subset.radius : subset.iterations) = static_cast<int>(n);
            (radius ? subset_refine : subset_option) = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-epsilon") || !std::strcmp(argv[i], "--subset-max-shift") ||
                 !std::strcmp(argv[i], "--subset-max-gradient")) {
            const bool epsilon = !std::strcmp(argv[i], "--subset-epsilon");
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(value) || !(epsilon ? value >= 0.f : value > 0.f)) {
                std::printf("%s takes a finite number %s 0.\n", argv[i], epsilon ? ">=" : ">");
                return 5;
            }
            (epsilon ? subset.epsilon : !std::strcmp(argv[i], "--subset-max-shift") ? subset.max_shift : subset.max_gradient) = value;
            subset_max_shift_given = subset_max_shift_given || !std::strcmp(argv[i], "--subset-max-shift");
            subset_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-order")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || (n != 1 && n != 2)) {
                std::printf("--subset-order takes 1 or 2.\n");
                return 5;
            }
            subset.order = static_cast<int>(n);
            subset_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-interpolation")) {
            const char* kind = (i + 1 < argc) ? argv[i + 1] : "";
            if (!std::strcmp(kind, "catmull-rom"))
                subset.interpolation = OpticalFlow2D::SubsetOptions::CatmullRom;
            else if (!std::strcmp(kind, "bspline"))
                subset.interpolation = OpticalFlow2D::SubsetOptions::BSpline;
            else {
                std::printf("--subset-interpolation takes catmull-rom or bspline.\n");
                return 5;
            }
            subset_option = subset_interpolation_given = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-max-curvature")) {
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(value) || !(value > 0.f)) {
                std::printf("--subset-max-curvature takes a finite number > 0.\n");
                return 5;
            }
            subset.max_curvature = value;
            subset_option = subset_curvature_given = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-mask")) {
            if (i + 1 >= argc || !argv[i + 1][0]) {
                std::printf("--subset-mask takes the file of the mask image.\n");
                return 5;
            }
            subset_mask_file = argv[++i];
        }
        else if (!std::strcmp(argv[i], "--subset-mask-invert")) subset_mask_invert = subset_mask_option = true;
        else if (!std::strcmp(argv[i], "--subset-mask-search")) subset.mask_search = subset_mask_option = true;
        else if (!std::strcmp(argv[i], "--subset-uncertainty")) subset_uncertainty = subset_option = true;
        else if (!std::strcmp(argv[i], "--correlation-mask")) {
            if (i + 1 >= argc || !argv[i + 1][0]) {
                std::printf("--correlation-mask takes the file of the mask image.\n");
                return 5;
            }
            correlation_mask_file = argv[++i];
        }
        else if (!std::strcmp(argv[i], "--correlation-mask-invert")) correlation_mask_invert = correlation_mask_option = true;
        else if (!std::strcmp(argv[i], "--correlation-min-pixels")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            const long largest = (2 * FLOW2D_CORRELATION_MAX_RADIUS + 1) * (2 * FLOW2D_CORRELATION_MAX_RADIUS + 1);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 || n > largest) {
                std::printf("--correlation-min-pixels takes a whole number of 1 .. %ld.\n", largest);
                return 5;
            }
            correlation_min_pixels = static_cast<int>(n);
            correlation_mask_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-min-pixels")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            const long largest = (2 * FLOW2D_SUBSET_MAX_RADIUS + 1) * (2 * FLOW2D_SUBSET_MAX_RADIUS + 1);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < FLOW2D_SUBSET_MIN_PIXELS || n > largest) {
                std::printf("--subset-min-pixels takes a whole number of %d .. %ld.\n", FLOW2D_SUBSET_MIN_PIXELS, largest);
                return 5;
            }
            subset.min_pixels = static_cast<int>(n);
            subset_mask_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-previous")) {
            if (i + 1 >= argc || !argv[i + 1][0]) {
                std::printf("--subset-previous takes the prefix of the previous step's node files.\n");
                return 5;
            }
            subset_previous = argv[++i];
        }
        else if (!std::strcmp(argv[i], "--subset-base")) {
            if (i + 1 >= argc || !argv[i + 1][0]) {
                std::printf("--subset-base takes the prefix of the node files of the field up to the reference frame.\n");
                return 5;
            }
            subset_base = argv[++i];
        }
        else if (!std::strcmp(argv[i], "--subset-strain") || !std::strcmp(argv[i], "--strain-order") ||
                 !std::strcmp(argv[i], "--strain-min-nodes")) {
            const bool window = !std::strcmp(argv[i], "--subset-strain"), order = !std::strcmp(argv[i], "--strain-order");
            const long low = order ? 1 : 0, high = window ? FLOW2D_NODE_STRAIN_MAX_WINDOW : order ? 2 : 225;
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : -1;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < low || n > high) {
                std::printf("%s takes an integer of %ld .. %ld.\n", argv[i], low, high);
                return 5;
            }
            (window ? node_strain.window : order ? node_strain.order : node_strain.min_nodes) = static_cast<int>(n);
            (window ? subset_strain : strain_option) = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--strain-sigma")) {
            char* end = nullptr;
            const float sigma = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(std::isfinite(sigma) && sigma > 0.f)) {
                std::printf("--strain-sigma takes the scale of the robust weight in pixels: finite and above 0.\n");
                return 5;
            }
            node_strain.robust_sigma = sigma;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--strain-weighted")) node_strain.weighted = true;
        else if (!std::strcmp(argv[i], "--strain-sigma-floor") || !std::strcmp(argv[i], "--strain-threshold")) {
            const bool floor = !std::strcmp(argv[i], "--strain-sigma-floor");
            char* end = nullptr;
            const float x = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : -1.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(std::isfinite(x) && x >= 0.f)) {
                std::printf("%s\n", floor ? "--strain-sigma-floor takes a standard deviation in pixels that every node has beside its own: "
                                            "finite and not negative."
                                          : "--strain-threshold takes the scale of the robust weight in sigmas: finite and not negative "
                                            "(0: no robust part).");
                return 5;
            }
            (floor ? node_strain.sigma_floor : node_strain.weight_threshold) = x;
            (floor ? strain_floor_given : strain_threshold_given) = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--strain-iterations")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : -1;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 0 || n > FLOW2D_NODE_STRAIN_MAX_ITERATIONS) {
                std::printf("--strain-iterations takes an integer of 0 .. %d.\n", FLOW2D_NODE_STRAIN_MAX_ITERATIONS);
                return 5;
            }
            node_strain.robust_iterations = static_cast<int>(n);
            strain_iterations_given = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--subset-fill") || !std::strcmp(argv[i], "--subset-min-state") ||
                 !std::strcmp(argv[i], "--subset-predict-neighbours")) {
            const bool fill = !std::strcmp(argv[i], "--subset-fill"), state = !std::strcmp(argv[i], "--subset-min-state");
            const long low = state ? 0 : 1, high = fill ? OpticalFlow2D::kSequenceMaxFill : state ? 1 : 8;
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : -1;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < low || n > high) {
                std::printf("%s takes an integer of %ld .. %ld.\n", argv[i], low, high);
                return 5;
            }
            (fill ? sequence.fill : state ? sequence.min_state : sequence.min_neighbours) = static_cast<int>(n);
            sequence_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--validate-threshold") || !std::strcmp(argv[i], "--validate-epsilon")) {
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(std::isfinite(value) && value > 0.f)) {
                std::printf("%s takes a finite number > 0.\n", argv[i]);
                return 5;
            }
            (!std::strcmp(argv[i], "--validate-threshold") ? validation.threshold : validation.epsilon) = value;
            validate_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--validate-min-neighbours")) {
            char* end = nullptr;
            const long n = (i + 1 < argc) ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || n < 1 || n > 8) {
                std::printf("--validate-min-neighbours takes an integer of 1 .. 8.\n");
                return 5;
            }
            validation.min_neighbours = static_cast<int>(n);
            validate_option = true;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--validate-flag-only")) {
            validation.replace = false;
            validate_option = true;
        }
        else if (!std::strcmp(argv[i], "--correlation-min-score")) {
            char* end = nullptr;
            const float value = (i + 1 < argc) ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || std::isnan(value)) {
                std::printf("--correlation-min-score takes a number (a score is -1 .. 1; -1: nothing is rejected).\n");
                return 5;
            }
            correlation_min_score = value;
            ++i;
        }
        else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--sor") && i + 1 < argc) sor_omega = static_cast<float>(std::atof(argv[++i]));
        else args.push_back(argv[i]);
    }
    const int nargs = static_cast<int>(args.size());
    if (segment && global_model < 0) {
        std::printf("--segment-motion needs --global-motion MODEL (the regions are those of the residual flow).\n");
        return 5;
    }

    if (method == Methods::Correlation &&
        (backward || interpolate || track_spacing || denoise || global_model >= 0 || segment || deformation || refine_radius)) {
        std::printf("--correlation replaces the variational flow and does not combine with the options that run it.\n");
        return 5;
    }

    const bool multipass = !correlation_passes.empty();
    if (validate_option && !multipass) {
        std::printf("The --validate-* options belong to --correlation-passes.\n");
        return 5;
    }
    if (multipass && (method == Methods::Correlation || backward || interpolate || track_spacing || denoise || global_model >= 0 || segment ||
                      deformation || refine_radius || prior_radius != 0 || !previous_flow_file.empty() || prior_option)) {
        std::printf("--correlation-passes replaces the variational flow: it does not combine with --correlation or with the options that "
                    "run or seed the flow (--initial-flow FILE.flo is its first pass's predictor).\n");
        return 5;
    }

    if ((subset_refine || subset_option) && !(subset_refine && (multipass || method == Methods::Correlation))) {
        std::printf("--subset-refine R refines the nodes of --correlation or --correlation-passes, and the --subset-* options belong to it.\n");
        return 5;
    }

    if (subset_refine && ((subset.order == 2 && subset.radius < FLOW2D_SUBSET2_MIN_RADIUS) || (subset_curvature_given && subset.order != 2))) {
        std::printf("--subset-order 2 takes a subset radius of %d at least, and --subset-max-curvature belongs to it.\n",
                    FLOW2D_SUBSET2_MIN_RADIUS);
        return 5;
    }
    if ((!subset_mask_file.empty() || subset_mask_option) && !(subset_refine && !subset_mask_file.empty())) {
        std::printf("--subset-mask FILE gives --subset-refine a region of interest, and --subset-mask-invert, --subset-min-pixels and "
                    "--subset-mask-search belong to it.\n");
        return 5;
    }
    if (subset.mask_search && !subset_previous.empty()) {
        std::printf("--subset-mask-search masks the passes in front of the refinement: --subset-previous runs none.\n");
        return 5;
    }
    if ((!correlation_mask_file.empty() || correlation_mask_option) && !(multipass && !correlation_mask_file.empty())) {
        std::printf("--correlation-mask FILE gives --correlation-passes a region of interest, and --correlation-mask-invert and "
                    "--correlation-min-pixels belong to it.\n");
        return 5;
    }
    validation.min_pixels = correlation_min_pixels;
    if (!correlation_mask_file.empty() && subset_refine) {
        std::printf("--correlation-mask goes with --correlation-passes alone: with --subset-refine the region of interest is --subset-mask, "
                    "and --subset-mask-search hands it to the passes.\n");
        return 5;
    }
    if (!subset_mask_file.empty() && subset.order == 2) {
        std::printf("--subset-mask goes with the first-order refinement only: --subset-order 2 takes no mask.\n");
        return 5;
    }
    if ((!subset_previous.empty() || sequence_option) && !(subset_refine && !subset_previous.empty())) {
        std::printf("--subset-previous PREFIX continues a sequence of --subset-refine runs, and --subset-fill, --subset-min-state and "
                    "--subset-predict-neighbours belong to it.\n");
        return 5;
    }
    sequence.max_shift = subset_max_shift_given || subset_previous.empty() ? subset.max_shift : 4.f;
    if (!subset_base.empty() && !subset_refine) {
        std::printf("--subset-base PREFIX composes the field of --subset-refine with the one up to its reference frame.\n");
        return 5;
    }
    if (subset_uncertainty && (subset.order != 1 || !subset_base.empty())) {
        std::printf("--subset-uncertainty gives the covariance of the first-order refinement (--subset-order 2 would need a 12 x 12 one), "
                    "and not of a field composed by --subset-base, which would need both fields'.\n");
        return 5;
    }

    if (strain_option && !subset_strain) {
        std::printf("--strain-order and --strain-min-nodes belong to --subset-strain M.\n");
        return 5;
    }
    if ((strain_floor_given || strain_threshold_given) && !node_strain.weighted) {
        std::printf("--strain-sigma-floor and --strain-threshold belong to --strain-weighted.\n");
        return 5;
    }
    if (node_strain.weighted && (!subset_uncertainty || !subset_strain || node_strain.window == 0)) {
        std::printf("--strain-weighted weights a strain window by the nodes' variances: it goes with --subset-uncertainty and "
                    "--subset-strain M, M >= 1.\n");
        return 5;
    }
    if (node_strain.weighted && node_strain.robust_sigma != 0.f) {
        std::printf("--strain-weighted takes its scale in sigmas (--strain-threshold T); --strain-sigma S is in pixels: give one of them.\n");
        return 5;
    }
    if (strain_iterations_given && node_strain.weighted && node_strain.weight_threshold == 0.f) {
        std::printf("--strain-iterations with --strain-weighted belongs to --strain-threshold T, T > 0.\n");
        return 5;
    }
    if (strain_iterations_given && node_strain.robust_sigma == 0.f && !node_strain.weighted) {
        std::printf("--strain-iterations belongs to --strain-sigma S.\n");
        return 5;
    }
    if (node_strain.robust_sigma != 0.f && (!subset_strain || node_strain.window == 0)) {
        std::printf("--strain-sigma S reweights a strain window: it goes with --subset-strain M, M >= 1.\n");
        return 5;
    }
    if (subset_strain && !(subset_refine || multipass || method == Methods::Correlation)) {
        std::printf("--subset-strain M takes the strain of a node field: it goes with --subset-refine, or with --correlation or "
                    "--correlation-passes alone.\n");
        return 5;
    }
    if (subset_strain && !subset_refine && node_strain.window == 0) {
        std::printf("--subset-strain 0 takes the gradients of --subset-refine; a search alone delivers none (M >= 1 fits them).\n");
        return 5;
    }
    if (subset_strain) {
        node_strain.measure = strain_measure;
        node_strain.min_state = sequence.min_state;
        if (node_strain.window == 0 && strain_option) {
            std::printf("--strain-order and --strain-min-nodes describe a window fit: --subset-strain 0 has none.\n");
            return 5;
        }
        if (!OpticalFlow2D::StrainOptionsOk(node_strain)) return 5;
    }

    // (with --correlation-passes the initial flow is the first pass's predictor, not the prior of a pyramid)
    const bool from_prior = (!initial_flow_file.empty() && !multipass) || prior_radius != 0 || !previous_flow_file.empty();
    if (!initial_flow_file.empty() && prior_radius != 0) {
        std::printf("--initial-flow and --correlation-prior are two sources of one prior: give one of them.\n");
        return 5;
    }
    if (!previous_flow_file.empty() && (!initial_flow_file.empty() || prior_radius != 0)) {
        std::printf("--previous-flow, --initial-flow and --correlation-prior are sources of one prior: give one of them.\n");
        return 5;
    }
    if (previous_option && previous_flow_file.empty()) {
        std::printf("--previous-frame and --propagate-fill need --previous-flow FILE.flo.\n");
        return 5;
    }
    if (from_prior && (method == Methods::Correlation || backward || interpolate || track_spacing || denoise || global_model >= 0 || segment ||
                       deformation || refine_radius)) {
        std::printf("A prior flow seeds the forward flow of the pair: it does not combine with --correlation or with the options that run "
                    "flows of their own (there is no prior for a backward flow).\n");
        return 5;
    }
    if (prior_option && !from_prior) {
        std::printf("--prior-reach and --prior-level need a prior: --initial-flow FILE.flo, --previous-flow FILE.flo or --correlation-prior R.\n");
        return 5;
    }

    if (!InitDeviceContext(device)) return 1;
    // the reference's ALLOCATE_PINNED_MEMORY option (data2d.cpp:34), on: frames and flows live in page-locked memory
    // and move by DMA (a failed pinned allocation falls back to pageable memory, same results)
    Data2D::UsePinnedMemory(true);

    std::printf("//----------------------------------------------------------------------//\n");
    std::printf("//       2D optical flow, MI355X (gfx950) HIP path. flow2d 0.1          //\n");
    std::printf("//----------------------------------------------------------------------//\n");

    // defaults of main.cpp:65-86
    size_t width = 584, height = 388;
    size_t warp_levels_count = 50;
    float warp_scale_factor = 0.9f;
    size_t outer_iterations_count = 40;
    size_t inner_iterations_count = 5;
    float equation_alpha = 35.0f;
    float equation_smoothness = 0.001f;
    float equation_data = 0.001f;
    size_t median_radius = 5;
    float gaussian_sigma = 1.5f;
    std::string file_name1 = "rub1.raw", file_name2 = "rub2.raw";
    std::string input_path = "./data/", output_path = "./data/output/", counter;
    bool u8 = force_u8;

    if (nargs == 6 || nargs == 7 || nargs == 9) {
        file_name1 = args[1];
        file_name2 = args[2];
        width = std::atoi(args[3]);
        height = std::atoi(args[4]);
        output_path = (nargs == 6) ? args[5] : args[6];
        if (nargs == 7) counter = args[5];
        if (nargs == 9) {
            equation_alpha = std::atof(args[7]);
            gaussian_sigma = std::atof(args[8]);
            counter = "alpha" + std::string(args[7]) + "_sigma" + std::string(args[8]) + "_";
        }
        input_path.clear();
    } else if (nargs < 3) {
        const std::string settings_file = (nargs == 1) ? "settings.xml" : std::string(args[1]);
        std::cout << "Reading settings: " << settings_file << std::endl;
        Settings settings;
        if (settings.LoadSettings(settings_file)) {
            std::cout << "TERMINATING. Error reading settings: " << settings_file << std::endl;
            return 3;
        }
        std::cout << "OK" << std::endl << std::endl;
        width = settings.width;
        height = settings.height;
        input_path = settings.inputPath;
        output_path = settings.outputPath;
        file_name1 = settings.fileName1;
        file_name2 = settings.fileName2;
        warp_levels_count = settings.levels;
        warp_scale_factor = settings.warpScale;
        outer_iterations_count = settings.iterOuter;
        inner_iterations_count = settings.iterInner;
        equation_alpha = settings.alpha;
        equation_data = settings.e_data;
        equation_smoothness = settings.e_smooth;
        median_radius = settings.medianRadius;
        gaussian_sigma = settings.sigma;
        if (settings.imageType == "8-bit") u8 = true;
        if (settings.dataConstancy == "gradient") data_constancy = DataConstancy::Gradient;
        if (settings.dataConstancy == "gradient-untiled") data_constancy = DataConstancy::GradientUntiled;
        if (settings.dataConstancy == "log-derivatives") data_constancy = DataConstancy::LogDerivatives;
    } else {
        std::cout << "Usage: " << args[0] << " <settings file>. Otherwise settings.xml in the current directory is used"
                  << std::endl;
        return 0;
    }

    DataSize3 data_size = {width, height, 1};
    Data2D frame_0, frame_1;
    if (!LoadFrame(frame_0, input_path, file_name1, u8, width, height) ||
        !LoadFrame(frame_1, input_path, file_name2, u8, width, height)) {
        return 2;
    }
    Data2D gt_u, gt_v;
    if (!ground_truth_file.empty()) {
        if (!IOUtils::ReadFlowFLO(ground_truth_file, gt_u, gt_v)) {
            std::printf("Cannot read ground truth '%s' (a Middlebury .flo file).\n", ground_truth_file.c_str());
            return 2;
        }
        if (gt_u.Width() != width || gt_u.Height() != height) {
            std::printf("Ground truth '%s' is %zu x %zu, the frames %zu x %zu.\n", ground_truth_file.c_str(), gt_u.Width(),
                        gt_u.Height(), width, height);
            return 2;
        }
    }

    Data2D subset_mask;  // --subset-mask: 1 = not the specimen
    if (!subset_mask_file.empty()) {
        if (!LoadFrame(subset_mask, input_path, subset_mask_file, u8, width, height)) return 2;
        if (subset_mask_invert)  // a region image: non-zero means inside
            for (size_t k = 0; k < width * height; ++k) subset_mask.DataPtr()[k] = subset_mask.DataPtr()[k] != 0.f ? 0.f : 1.f;
    }
    Data2D* const subset_mask_image = subset_mask_file.empty() ? nullptr : &subset_mask;
    Data2D correlation_mask;  // --correlation-mask: 1 = not the specimen
    if (!correlation_mask_file.empty()) {
        if (!LoadFrame(correlation_mask, input_path, correlation_mask_file, u8, width, height)) return 2;
        if (correlation_mask_invert)  // a region image: non-zero means inside
            for (size_t k = 0; k < width * height; ++k) correlation_mask.DataPtr()[k] = correlation_mask.DataPtr()[k] != 0.f ? 0.f : 1.f;
    }
    Data2D* const correlation_mask_image = correlation_mask_file.empty() ? nullptr : &correlation_mask;

    Data2D prior_u, prior_v;
    if (!initial_flow_file.empty()) {
        if (!IOUtils::ReadFlowFLO(initial_flow_file, prior_u, prior_v)) {
            std::printf("Cannot read the initial flow '%s' (a Middlebury .flo file).\n", initial_flow_file.c_str());
            return 2;
        }
        if (prior_u.Width() != width || prior_u.Height() != height) {
            std::printf("The initial flow '%s' is %zu x %zu, the frames %zu x %zu.\n", initial_flow_file.c_str(), prior_u.Width(),
                        prior_u.Height(), width, height);
            return 2;
        }
    }

    Data2D previous_frame;
    if (!previous_flow_file.empty()) {
        if (!IOUtils::ReadFlowFLO(previous_flow_file, prior_u, prior_v)) {
            std::printf("Cannot read the previous flow '%s' (a Middlebury .flo file).\n", previous_flow_file.c_str());
            return 2;
        }
        if (prior_u.Width() != width || prior_u.Height() != height) {
            std::printf("The previous flow '%s' is %zu x %zu, the frames %zu x %zu.\n", previous_flow_file.c_str(), prior_u.Width(),
                        prior_u.Height(), width, height);
            return 2;
        }
        if (!previous_frame_file.empty() && !LoadFrame(previous_frame, input_path, previous_frame_file, u8, width, height)) return 2;
    }

    OpticalFlow2D optical_flow;
    optical_flow.silent = !verbose;
    if (optical_flow.Initialize(data_size, data_constancy)) {
        Data2D flow_u(width, height), flow_v(width, height);
        OperationParameters params;
        params.PushValuePtr("warp_levels_count", &warp_levels_count);
        params.PushValuePtr("warp_scale_factor", &warp_scale_factor);
        params.PushValuePtr("outer_iterations_count", &outer_iterations_count);
        params.PushValuePtr("inner_iterations_count", &inner_iterations_count);
        params.PushValuePtr("equation_alpha", &equation_alpha);
        params.PushValuePtr("equation_smoothness", &equation_smoothness);
        params.PushValuePtr("equation_data", &equation_data);
        params.PushValuePtr("median_radius", &median_radius);
        params.PushValuePtr("gaussian_sigma", &gaussian_sigma);
        if (sor_omega != 0.f) params.PushValuePtr("solver_sor_omega", &sor_omega);
        if (from_prior) {
            params.PushValuePtr("prior_reach", &prior_reach);
            if (prior_level >= 0) params.PushValuePtr("prior_level", &prior_level);
        }
        Data2D back_u, back_v, occlusion_0, occlusion_1;
        std::vector<Data2D> between;
        std::vector<float> times;
        if (interpolate) {
            for (int k = 1; k < interpolate; ++k) {
                between.emplace_back(width, height);
                times.push_back(static_cast<float>(k) / static_cast<float>(interpolate));
            }
        }
        if (backward || interpolate) {
            back_u = Data2D(width, height);
            back_v = Data2D(width, height);
            occlusion_0 = Data2D(width, height);
            occlusion_1 = Data2D(width, height);
        }
        Data2D node_u, node_v, node_score;
        // --subset-strain: the nine planes of the node field fields[0 .. 6] (u, v, ux, uy, vx, vy, state; null = absent), written
        // beside the node files, and the record
        // With --strain-weighted: `uncertainty` holds the nodes' sigma_u and sigma_v, the nine sigma planes are written too.
        auto write_node_strain = [&](Data2D* const* fields, size_t nw, size_t nh, int spacing, Data2D* const* uncertainty = nullptr) {
            const char* names[9] = {"node-divergence", "node-vorticity", "node-dilatation", "node-exx", "node-eyy", "node-exy", "node-e1",
                                    "node-e2", "node-max-shear"};
            std::vector<Data2D> images;
            for (int k = 0; k < 9; ++k) images.emplace_back(nw, nh);
            const bool weighted = node_strain.weighted && uncertainty;
            const bool robust = node_strain.robust_sigma != 0.f || weighted;
            const char* diagnostic_names[3] = {"node-strain-residual", "node-strain-rejected", "node-strain-centre"};
            const char* sigma_names[9] = {"node-sigma-strain-ux", "node-sigma-strain-uy", "node-sigma-strain-vx", "node-sigma-strain-vy",
                                          "node-sigma-divergence", "node-sigma-vorticity", "node-sigma-exx",      "node-sigma-eyy",
                                          "node-sigma-exy"};
            for (int k = 0; robust && k < 3; ++k) images.emplace_back(nw, nh);
            for (int k = 0; weighted && k < 9; ++k) images.emplace_back(nw, nh);
            Data2D* planes[9];
            Data2D* diagnostics[3];
            Data2D* strain_sigmas[9];
            for (int k = 0; k < 9; ++k) planes[k] = &images[k];
            for (int k = 0; robust && k < 3; ++k) diagnostics[k] = &images[9 + k];
            for (int k = 0; weighted && k < 9; ++k) strain_sigmas[k] = &images[12 + k];
            flow2d_deformation_stats stats = {};
            if (weighted)
                optical_flow.NodeStrain(fields, 1, spacing, node_strain, uncertainty, planes, &stats, diagnostics, strain_sigmas);
            else
                optical_flow.NodeStrain(fields, 1, spacing, node_strain, planes, &stats, robust ? diagnostics : nullptr);
            if (!optical_flow.LastRunSucceeded()) return;
            const std::string size = "-" + std::to_string(nw) + "-" + std::to_string(nh) + ".raw";
            for (int k = 0; k < 9; ++k) images[k].WriteRAWToFileF32((output_path + counter + names[k] + size).c_str());
            for (int k = 0; robust && k < 3; ++k)
                images[9 + k].WriteRAWToFileF32((output_path + counter + diagnostic_names[k] + size).c_str());
            std::printf("NodeStrain: {\"window\": %d, \"order\": %d, \"min_nodes\": %d, \"min_state\": %d, \"measure\": \"%s\", "
                        "\"spacing\": %d, \"nw\": %zu, \"nh\": %zu, \"valid\": %llu, \"invalid\": %llu, \"centre\": %llu, "
                        "\"sparse\": %llu, \"degenerate\": %llu",
                        node_strain.window, node_strain.order, node_strain.min_nodes, node_strain.min_state,
                        node_strain.measure == FLOW2D_STRAIN_SMALL ? "small" : "green", spacing, nw, nh, stats.valid, stats.invalid,
                        stats.reserved[0], stats.reserved[1], stats.reserved[2]);
            const flow2d_deformation_moments* moments[6] = {&stats.divergence, &stats.vorticity, &stats.dilatation,
                                                            &stats.e1,         &stats.e2,        &stats.max_shear};
            const char* quantity[6] = {"divergence", "vorticity", "dilatation", "e1", "e2", "max_shear"};
            for (int k = 0; k < 6; ++k)
                std::printf(", \"%s\": {\"sum\": %.17g, \"sum_sq\": %.17g, \"min\": %.9g, \"max\": %.9g}", quantity[k], moments[k]->sum,
                            moments[k]->sum_sq, moments[k]->min, moments[k]->max);
            std::printf("}\n");
            for (int k = 0; weighted && k < 9; ++k) images[12 + k].WriteRAWToFileF32((output_path + counter + sigma_names[k] + size).c_str());
            if (weighted)
                std::printf("WeightedStrain: {\"sigma_floor\": %.9g, \"threshold\": %.9g, \"iterations\": %d, \"touched\": %llu, "
                            "\"rejected\": %llu, \"suspect\": %llu, \"unweighable\": %llu}\n",
                            static_cast<double>(node_strain.sigma_floor), static_cast<double>(node_strain.weight_threshold),
                            node_strain.weight_threshold > 0.f ? node_strain.robust_iterations : 0, stats.reserved[3], stats.reserved[4],
                            stats.reserved[5], stats.reserved[6]);
            else if (robust)
                std::printf("NodeStrainRobust: {\"sigma\": %.9g, \"iterations\": %d, \"touched\": %llu, \"rejected\": %llu, "
                            "\"suspect\": %llu}\n",
                            static_cast<double>(node_strain.robust_sigma), node_strain.robust_iterations, stats.reserved[3],
                            stats.reserved[4], stats.reserved[5]);
        };
        if (subset_refine) {
            std::vector<OpticalFlow2D::CorrelationPass> schedule = correlation_passes;
            if (!multipass) schedule.push_back({correlation_radius, correlation_range, correlation_spacing});
            const OpticalFlow2D::CorrelationPass& fine = schedule.back();
            float lo = 0.f, scale = 1.f;
            OpticalFlow2D::CorrelationRange(frame_0, frame_1, lo, scale);
            size_t nw = 0, nh = 0;
            if (!OpticalFlow2D::CorrelationPassesOk(width, height, lo, scale, schedule.data(), schedule.size(), correlation_min_score,
                                                    validation) ||
                flow2d_correlation_grid(width, height, fine.radius, fine.spacing, &nw, &nh) != FLOW2D_OK) {
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            const char* names[14] = {"node-u",     "node-v",   "node-ux",  "node-uy",  "node-vx",  "node-vy",  "node-score",
                                     "node-state", "node-uxx", "node-uxy", "node-uyy", "node-vxx", "node-vxy", "node-vyy"};
            const int node_images = subset.order == 2 ? 14 : 8;  // --subset-order 2: the six curvatures beside the eight
            std::vector<Data2D> images;
            for (int k = 0; k < node_images; ++k) images.emplace_back(nw, nh);
            Data2D* nodes[14] = {};
            for (int k = 0; k < node_images; ++k) nodes[k] = &images[k];
            flow2d_subset_record record = {};
            const std::string size = "-" + std::to_string(nw) + "-" + std::to_string(nh) + ".raw";
            if (!subset_previous.empty()) {
                // the previous step's files, of this grid: u, v, the gradients and the state
                const int from[7] = {0, 1, 2, 3, 4, 5, 7};
                std::vector<Data2D> before(7);
                Data2D* previous[7];
                for (int k = 0; k < 7; ++k) {
                    const std::string path = subset_previous + names[from[k]] + size;
                    if (!before[k].ReadRAWFromFileF32(path.c_str(), nw, nh)) {
                        std::printf("Cannot read '%s' (%zu x %zu float32: the previous step's nodes on this grid).\n", path.c_str(), nw, nh);
                        optical_flow.Destroy();
                        DestroyDeviceContext();
                        return 2;
                    }
                    previous[k] = &before[k];
                }
                OpticalFlow2D::SequenceStepReport report = {};
                optical_flow.ContinueSubsetSequence(frame_0, frame_1, previous, fine.radius, fine.spacing, subset, sequence, nodes, &report,
                                                    &flow_u, &flow_v, subset_mask_image);
                record = report.subset;
                subset.max_shift = sequence.max_shift;
                if (optical_flow.LastRunSucceeded()) {
                    std::printf("Prediction: {\"fill\": %d, \"min_state\": %d, \"min_neighbours\": %d, \"passes\": [", sequence.fill,
                                sequence.min_state, sequence.min_neighbours);
                    for (int k = 0; k < sequence.fill; ++k)
                        std::printf("%s{\"nodes\": %llu, \"kept\": %llu, \"predicted\": %llu, \"empty\": %llu}", k ? ", " : "",
                                    report.prediction[k].nodes, report.prediction[k].kept, report.prediction[k].predicted,
                                    report.prediction[k].empty);
                    std::printf("]}\n");
                }
            } else {
                const bool predicted = multipass && !initial_flow_file.empty();
                std::vector<OpticalFlow2D::CorrelationPassReport> searched(subset.mask_search ? schedule.size() : 0);
                optical_flow.CorrelateSubset(frame_0, frame_1, schedule.data(), schedule.size(), correlation_min_score, validation, subset,
                                             nodes, subset.mask_search ? searched.data() : nullptr, &record, &flow_u, &flow_v,
                                             predicted ? &prior_u : nullptr, predicted ? &prior_v : nullptr, subset_mask_image);
                if (subset.mask_search && optical_flow.LastRunSucceeded()) print_correlation_mask(schedule, searched, validation);
            }
            flow2d_compose_record composition = {};
            std::vector<Data2D> composed;
            if (optical_flow.LastRunSucceeded() && !subset_base.empty()) {
                // the refined field is an increment from the reference frame: written under its own names, then composed with the
                // field up to the reference into the eight node images
                for (int k = 0; k < node_images; ++k)
                    images[k].WriteRAWToFileF32((output_path + counter + "increment-" + names[k] + size).c_str());
                const int from[7] = {0, 1, 2, 3, 4, 5, 7};
                std::vector<Data2D> before(7);
                Data2D *base[7], *out[8];
                for (int k = 0; k < 7; ++k) {
                    const std::string path = subset_base + names[from[k]] + size;
                    if (!before[k].ReadRAWFromFileF32(path.c_str(), nw, nh)) {
                        std::printf("Cannot read '%s' (%zu x %zu float32: the field up to the reference frame on this grid).\n", path.c_str(), nw,
                                    nh);
                        optical_flow.Destroy();
                        DestroyDeviceContext();
                        return 2;
                    }
                    base[k] = &before[k];
                }
                for (int k = 0; k < 8; ++k) composed.emplace_back(nw, nh);
                for (int k = 0; k < 8; ++k) out[k] = &composed[k];
                optical_flow.ComposeNodes(base, nodes, fine.radius, fine.spacing, sequence.min_state, out, &composition);
                for (int k = 0; k < 8; ++k) nodes[k] = out[k];  // what is written and strained below
            }
            if (optical_flow.LastRunSucceeded()) {
                if (subset_mask_image)
                    std::printf("SubsetMask: {\"masked\": %llu, \"min_pixels\": %d}\n", record.reserved, OpticalFlow2D::SubsetMinPixels(subset));
                if (!subset_base.empty())
                    std::printf("Compose: {\"min_state\": %d, \"nodes\": %llu, \"composed\": %llu, \"no_base\": %llu, \"outside\": %llu, "
                                "\"no_increment\": %llu}\n",
                                sequence.min_state, composition.nodes, composition.composed, composition.no_base, composition.outside,
                                composition.no_increment);
                // (with --subset-base and order 2 the curvature files would be the increment's: they are written with it alone)
                for (int k = 0; k < (subset_base.empty() ? node_images : 8); ++k)
                    nodes[k]->WriteRAWToFileF32((output_path + counter + names[k] + size).c_str());
                if (subset_interpolation_given) {
                    if (subset.interpolation == OpticalFlow2D::SubsetOptions::BSpline)
                        std::printf("SubsetInterpolation: {\"interpolation\": \"bspline\", \"horizon\": %d}\n", FLOW2D_BSPLINE_HORIZON);
                    else
                        std::printf("SubsetInterpolation: {\"interpolation\": \"catmull-rom\"}\n");
                }
                if (subset.order == 2) std::printf("SubsetOrder: {\"order\": 2, \"max_curvature\": %.9g}\n", subset.max_curvature);
                std::printf("Subset: {\"radius\": %d, \"iterations\": %d, \"epsilon\": %.9g, \"max_shift\": %.9g, \"max_gradient\": %.9g, "
                            "\"passes\": %zu, \"grid_radius\": %d, \"spacing\": %d, \"nw\": %zu, \"nh\": %zu, \"lo\": %.9g, \"scale\": %.9g, "
                            "\"nodes\": %llu, \"converged\": %llu, \"unconverged\": %llu, \"strayed\": %llu, \"flat\": %llu, "
                            "\"no_input\": %llu, \"iterations_run\": %llu}\n",
                            subset.radius, subset.iterations, subset.epsilon, subset.max_shift, subset.max_gradient,
                            subset_previous.empty() ? schedule.size() : size_t(0),
                            fine.radius, fine.spacing, nw, nh, lo, scale, record.nodes, record.converged, record.unconverged,
                            record.strayed, record.flat, record.no_input, record.iterations);
                if (subset_strain && !node_strain.weighted) {
                    Data2D* fields[7] = {nodes[0], nodes[1], nodes[2], nodes[3], nodes[4], nodes[5], nodes[7]};
                    write_node_strain(fields, nw, nh, fine.spacing);
                }
                if (subset_uncertainty && optical_flow.LastRunSucceeded()) {
                    const char* sigma_names[8] = {"node-sigma-u",  "node-sigma-v",  "node-rho",      "node-sigma-ux",
                                                  "node-sigma-uy", "node-sigma-vx", "node-sigma-vy", "node-noise"};
                    std::vector<Data2D> sigmas;
                    for (int k = 0; k < 8; ++k) sigmas.emplace_back(nw, nh);
                    Data2D* wanted[8];
                    for (int k = 0; k < 8; ++k) wanted[k] = &sigmas[k];
                    flow2d_uncertainty_record counts = {};
                    // (on --subset-previous the nodes below --subset-min-state were not a start either; the pair chain keeps 1)
                    optical_flow.NodeUncertainty(frame_0, frame_1, nodes, fine.radius, fine.spacing, subset, sequence.min_state, wanted, &counts,
                                                 subset_mask_image);
                    if (optical_flow.LastRunSucceeded()) {
                        for (int k = 0; k < 8; ++k) sigmas[k].WriteRAWToFileF32((output_path + counter + sigma_names[k] + size).c_str());
                        std::printf("SubsetUncertainty: {\"radius\": %d, \"min_state\": %d, \"nodes\": %llu, \"evaluated\": %llu, "
                                    "\"skipped\": %llu, \"masked\": %llu, \"outside\": %llu, \"flat\": %llu, \"thin\": %llu}\n",
                                    subset.radius, sequence.min_state, counts.nodes, counts.evaluated, counts.skipped, counts.masked,
                                    counts.outside, counts.flat, counts.thin);
                        // (--strain-weighted: the strain comes behind the uncertainty it is weighted by)
                        if (subset_strain && node_strain.weighted) {
                            Data2D* fields[7] = {nodes[0], nodes[1], nodes[2], nodes[3], nodes[4], nodes[5], nodes[7]};
                            write_node_strain(fields, nw, nh, fine.spacing, wanted);
                        }
                    }
                }
            }
        } else if (multipass) {
            const OpticalFlow2D::CorrelationPass& fine = correlation_passes.back();
            float lo = 0.f, scale = 1.f;
            OpticalFlow2D::CorrelationRange(frame_0, frame_1, lo, scale);
            size_t nw = 0, nh = 0;
            if (!OpticalFlow2D::CorrelationPassesOk(width, height, lo, scale, correlation_passes.data(), correlation_passes.size(),
                                                    correlation_min_score, validation) ||
                flow2d_correlation_grid(width, height, fine.radius, fine.spacing, &nw, &nh) != FLOW2D_OK) {
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            node_u = Data2D(nw, nh);
            node_v = Data2D(nw, nh);
            node_score = Data2D(nw, nh);
            std::vector<OpticalFlow2D::CorrelationPassReport> reports(correlation_passes.size());
            const bool predicted = !initial_flow_file.empty();
            optical_flow.CorrelateMultiPass(frame_0, frame_1, correlation_passes.data(), correlation_passes.size(), correlation_min_score,
                                            validation, node_u, node_v, &node_score, reports.data(), &flow_u, &flow_v,
                                            predicted ? &prior_u : nullptr, predicted ? &prior_v : nullptr, correlation_mask_image);
            if (optical_flow.LastRunSucceeded()) {
                const std::string nodes = "-" + std::to_string(nw) + "-" + std::to_string(nh) + ".raw";
                node_u.WriteRAWToFileF32((output_path + counter + "node-u" + nodes).c_str());
                node_v.WriteRAWToFileF32((output_path + counter + "node-v" + nodes).c_str());
                node_score.WriteRAWToFileF32((output_path + counter + "node-score" + nodes).c_str());
                std::printf("CorrelationPasses: {\"min_score\": %.9g, \"lo\": %.9g, \"scale\": %.9g, \"threshold\": %.9g, \"epsilon\": %.9g, "
                            "\"min_neighbours\": %d, \"replace\": %s, \"predictor\": %s, \"passes\": [",
                            correlation_min_score, lo, scale, validation.threshold, validation.epsilon, validation.min_neighbours,
                            validation.replace ? "true" : "false", predicted ? "true" : "false");
                for (size_t k = 0; k < reports.size(); ++k) {
                    const flow2d_correlation_pass_record& c = reports[k].correlation;
                    const flow2d_validation_record& v = reports[k].validation;
                    std::printf("%s{\"radius\": %d, \"range\": %d, \"spacing\": %d, \"nw\": %zu, \"nh\": %zu, \"correlation\": {\"nodes\": %llu, "
                                "\"invalid\": %llu, \"rejected\": %llu, \"unrefined\": %llu, \"unpredicted\": %llu, \"candidates\": %llu}, "
                                "\"validation\": {\"nodes\": %llu, \"judged\": %llu, \"outliers\": %llu, \"filled\": %llu, \"unjudged\": %llu, "
                                "\"remaining_invalid\": %llu}}",
                                k ? ", " : "", correlation_passes[k].radius, correlation_passes[k].range, correlation_passes[k].spacing,
                                reports[k].nw, reports[k].nh, c.nodes, c.invalid, c.rejected, c.unrefined, c.unpredicted, c.candidates,
                                v.nodes, v.judged, v.outliers, v.filled, v.unjudged, v.remaining_invalid);
                }
                std::printf("]}\n");
                if (correlation_mask_image) print_correlation_mask(correlation_passes, reports, validation);
                if (subset_strain) {
                    Data2D* fields[7] = {&node_u, &node_v, nullptr, nullptr, nullptr, nullptr, nullptr};
                    write_node_strain(fields, nw, nh, fine.spacing);
                }
            }
        } else if (method == Methods::Correlation) {
            size_t nw = 0, nh = 0;
            if (flow2d_correlation_grid(width, height, correlation_radius, correlation_spacing, &nw, &nh) != FLOW2D_OK) {
                std::printf("Error: a %zu x %zu frame is smaller than one correlation window of radius %d.\n", width, height,
                            correlation_radius);
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            node_u = Data2D(nw, nh);
            node_v = Data2D(nw, nh);
            node_score = Data2D(nw, nh);
            flow2d_correlation_record record = {0, 0, 0, 0};
            float lo = 0.f, scale = 1.f;
            OpticalFlow2D::CorrelationRange(frame_0, frame_1, lo, scale);
            optical_flow.Correlate(frame_0, frame_1, correlation_radius, correlation_range, correlation_spacing, correlation_min_score,
                                   node_u, node_v, &node_score, &record, &flow_u, &flow_v);
            if (optical_flow.LastRunSucceeded()) {
                const std::string nodes = "-" + std::to_string(nw) + "-" + std::to_string(nh) + ".raw";
                node_u.WriteRAWToFileF32((output_path + counter + "node-u" + nodes).c_str());
                node_v.WriteRAWToFileF32((output_path + counter + "node-v" + nodes).c_str());
                node_score.WriteRAWToFileF32((output_path + counter + "node-score" + nodes).c_str());
                std::printf("Correlation: {\"radius\": %d, \"range\": %d, \"spacing\": %d, \"min_score\": %.9g, \"lo\": %.9g, "
                            "\"scale\": %.9g, \"nw\": %zu, \"nh\": %zu, \"nodes\": %llu, \"invalid\": %llu, \"rejected\": %llu, "
                            "\"unrefined\": %llu}\n",
                            correlation_radius, correlation_range, correlation_spacing, correlation_min_score, lo, scale, nw, nh,
                            record.nodes, record.invalid, record.rejected, record.unrefined);
                if (subset_strain) {
                    Data2D* fields[7] = {&node_u, &node_v, nullptr, nullptr, nullptr, nullptr, nullptr};
                    write_node_strain(fields, nw, nh, correlation_spacing);
                }
            }
        } else if (!initial_flow_file.empty()) {
            OpticalFlow2D::PriorReport report;
            optical_flow.ComputeFlowFromPrior(frame_0, frame_1, prior_u, prior_v, flow_u, flow_v, params, &report);
            if (optical_flow.LastRunSucceeded())
                std::printf("Prior: {\"source\": \"initial-flow\", \"reach\": %.9g, \"start_level\": %zu, \"levels_run\": %zu, "
                            "\"not_finite\": %llu}\n",
                            prior_reach, report.start_level, report.levels_run, report.not_finite);
        } else if (!previous_flow_file.empty()) {
            OpticalFlow2D::WarmOptions options;
            options.fill_passes = propagate_fill;
            OpticalFlow2D::WarmReport report;
            const bool photometric = !previous_frame_file.empty();
            optical_flow.ComputeFlowFromPrevious(frame_0, frame_1, prior_u, prior_v, nullptr, photometric ? &previous_frame : nullptr, flow_u,
                                                 flow_v, params, options, &report);
            if (optical_flow.LastRunSucceeded()) {
                const flow2d_propagate_record& r = report.propagation;
                std::printf("Propagation: {\"fill\": %d, \"photometric\": %s, \"pixels\": %llu, \"unusable\": %llu, \"left\": %llu, "
                            "\"landed\": %llu, \"holes\": %llu, \"filled\": %llu, \"unfilled\": %llu}\n",
                            propagate_fill, photometric ? "true" : "false", r.pixels, r.unusable, r.left, r.landed, r.holes, r.filled,
                            r.unfilled);
                std::printf("Prior: {\"source\": \"previous-flow\", \"reach\": %.9g, \"start_level\": %zu, \"levels_run\": %zu, "
                            "\"not_finite\": %llu}\n",
                            prior_reach, report.prior.start_level, report.prior.levels_run, report.prior.not_finite);
            }
        } else if (prior_radius) {
            size_t nw = 0, nh = 0;
            if (flow2d_correlation_grid(width, height, prior_radius, correlation_spacing, &nw, &nh) != FLOW2D_OK) {
                std::printf("Error: a %zu x %zu frame is smaller than one correlation window of radius %d.\n", width, height, prior_radius);
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            OpticalFlow2D::PriorReport report;
            flow2d_correlation_record record = {0, 0, 0, 0};
            float lo = 0.f, scale = 1.f;
            OpticalFlow2D::CorrelationRange(frame_0, frame_1, lo, scale);
            optical_flow.ComputeFlowCorrelationSeeded(frame_0, frame_1, prior_radius, correlation_range, correlation_spacing,
                                                      correlation_min_score, flow_u, flow_v, params, nullptr, nullptr, nullptr, &record,
                                                      &report);
            if (optical_flow.LastRunSucceeded())
                std::printf("Prior: {\"source\": \"correlation\", \"reach\": %.9g, \"start_level\": %zu, \"levels_run\": %zu, "
                            "\"not_finite\": %llu, \"radius\": %d, \"range\": %d, \"spacing\": %d, \"min_score\": %.9g, \"lo\": %.9g, "
                            "\"scale\": %.9g, \"nw\": %zu, \"nh\": %zu, \"nodes\": %llu, \"invalid\": %llu, \"rejected\": %llu, "
                            "\"unrefined\": %llu}\n",
                            prior_reach, report.start_level, report.levels_run, report.not_finite, prior_radius, correlation_range,
                            correlation_spacing, correlation_min_score, lo, scale, nw, nh, record.nodes, record.invalid, record.rejected,
                            record.unrefined);
        } else if (interpolate) {
            optical_flow.InterpolateFrames(frame_0, frame_1, times.data(), times.size(), between.data(), 2, 0.5f, true, params,
                                           &flow_u, &flow_v, &back_u, &back_v, &occlusion_0, &occlusion_1);
        } else if (backward) {
            optical_flow.ComputeFlowBidirectional(frame_0, frame_1, flow_u, flow_v, back_u, back_v, occlusion_0, occlusion_1,
                                                  params);
        } else {
            optical_flow.ComputeFlow(frame_0, frame_1, flow_u, flow_v, params);
        }
        if (!optical_flow.LastRunSucceeded()) {
            // the reference writes whatever its buffers hold after a failed run; no output files here instead
            std::cout << "Error: the flow computation failed, no output written." << std::endl;
            optical_flow.Destroy();
            DestroyDeviceContext();
            return 4;  // superset of the reference's exit codes (0, 1, 2, 3, 255)
        }

        // --refine: the forward files hold the refined flow; flow_u / flow_v keep the flow as computed
        Data2D refined_u, refined_v;
        if (refine_radius) {
            refined_u = Data2D(width, height);
            refined_v = Data2D(width, height);
            flow2d_refine_record record;
            optical_flow.RefineFlow(frame_0, frame_1, refine_radius, refine_sigma, refine_space, refine_iterations, backward, refined_u,
                                    refined_v, &record, params);
            if (!optical_flow.LastRunSucceeded()) {
                std::cout << "Error: the flow refinement failed, no output written." << std::endl;
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            std::printf("Refinement: {\"radius\": %d, \"sigma\": %.9g, \"space\": %.9g, \"iterations\": %d, \"pixels\": %llu, "
                        "\"unfilled\": %llu, \"filled\": %llu, \"changed\": %llu}\n",
                        refine_radius, refine_sigma, refine_space, refine_iterations, record.pixels, record.unfilled, record.filled,
                        record.changed);
        }
        Data2D& computed_u = flow_u;
        Data2D& computed_v = flow_v;
        Data2D& written_u = refine_radius ? refined_u : flow_u;
        Data2D& written_v = refine_radius ? refined_v : flow_v;
        const std::string suffix = "-" + std::to_string(width) + "-" + std::to_string(height) + ".raw";
        written_u.WriteRAWToFileF32((output_path + counter + "flow-u" + suffix).c_str());
        written_v.WriteRAWToFileF32((output_path + counter + "flow-v" + suffix).c_str());
        IOUtils::WriteFlowToImageRGB(written_u, written_v, 10, output_path + counter + "res.pgm");
        IOUtils::WriteMagnitudeToFileF32(written_u, written_v, output_path + counter + "amp" + suffix);
        if (backward) {
            back_u.WriteRAWToFileF32((output_path + counter + "flow-u-backward" + suffix).c_str());
            back_v.WriteRAWToFileF32((output_path + counter + "flow-v-backward" + suffix).c_str());
            occlusion_0.WriteRAWToFileF32((output_path + counter + "occlusion" + suffix).c_str());
            occlusion_1.WriteRAWToFileF32((output_path + counter + "occlusion-backward" + suffix).c_str());
            IOUtils::WriteMaskToImagePGM(occlusion_0, output_path + counter + "occlusion.pgm");
        }
        for (int k = 1; k < interpolate; ++k)
            between[k - 1].WriteRAWToFileF32((output_path + counter + "interp-" + std::to_string(k) + "-of-" +
                                              std::to_string(interpolate) + suffix).c_str());
        if (write_flo) {
            bool ok = IOUtils::WriteFlowFLO(written_u, written_v, output_path + counter + "flow.flo");
            if (backward) ok = ok && IOUtils::WriteFlowFLO(back_u, back_v, output_path + counter + "flow-backward.flo");
            if (!ok) {
                std::cerr << "Error: cannot save file " << std::endl;
                std::exit(255);
            }
        }
        if (track_spacing) {
            const size_t s = static_cast<size_t>(track_spacing);
            const size_t capacity = 2 * ((width + s - 1) / s) * ((height + s - 1) / s);  // seeds of both frames at most
            std::vector<float> xs(2 * capacity), ys(2 * capacity);
            unsigned long long counts[2] = {0, 0};
            Data2D* frames[2] = {&frame_0, &frame_1};
            optical_flow.TrackPoints(frames, 2, s, OpticalFlow2D::kDefaultTrackMinEigenvalue, true, 0.01f, 0.002f, xs.data(),
                                     ys.data(), capacity, counts, params);
            if (!optical_flow.LastRunSucceeded()) {
                std::cout << "Error: point tracking failed." << std::endl;
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            std::FILE* out = std::fopen((output_path + counter + "tracks.txt").c_str(), "w");
            if (!out) {
                std::cerr << "Error: cannot save file " << std::endl;
                std::exit(255);
            }
            size_t alive = 0;
            auto put = [out](float v, const char* sep) {
                if (std::isnan(v)) std::fprintf(out, "nan%s", sep);
                else std::fprintf(out, "%.9g%s", v, sep);
            };
            for (size_t i = 0; i < counts[1]; ++i) {
                put(xs[i], " ");
                put(ys[i], " ");
                put(xs[capacity + i], " ");
                put(ys[capacity + i], "\n");
                if (i < counts[0] && !std::isnan(xs[capacity + i])) ++alive;
            }
            std::fclose(out);
            std::printf("Tracks: %zu alive, %zu ended, %llu seeded in frame 2\n", alive, static_cast<size_t>(counts[0]) - alive,
                        counts[1] - counts[0]);
        }
        if (denoise) {
            Data2D* frames[2] = {&frame_0, &frame_1};
            std::vector<Data2D> denoised;
            denoised.emplace_back(width, height);
            denoised.emplace_back(width, height);
            optical_flow.DenoiseSequence(frames, 2, 1, denoise_sigma, true, denoised.data(), nullptr, params);
            if (!optical_flow.LastRunSucceeded()) {
                std::cout << "Error: denoising failed." << std::endl;
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            for (int k = 0; k < 2; ++k) {
                const std::string name = output_path + counter + "denoised-" + std::to_string(k + 1) + suffix;
                if (!(u8 ? denoised[k].WriteRAWToFileU8(name.c_str()) : denoised[k].WriteRAWToFileF32(name.c_str()))) {
                    std::cerr << "Error: cannot save file " << std::endl;
                    std::exit(255);
                }
            }
        }
        if (global_model >= 0) {
            flow2d_global_motion motion;
            Data2D residual_u(width, height), residual_v(width, height);
            optical_flow.EstimateGlobalMotion(frame_0, frame_1, global_model, global_sigma, global_iterations, backward, &motion, params,
                                              nullptr, nullptr, &residual_u, &residual_v);
            if (!optical_flow.LastRunSucceeded()) {
                std::cout << "Error: the global motion estimation failed." << std::endl;
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            std::printf("Global motion: {\"model\": %d, \"model_used\": %d, \"p\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], "
                        "\"weight_sum\": %.17g, \"support\": %llu}\n",
                        global_model, motion.model_used, motion.p[0], motion.p[1], motion.p[2], motion.p[3], motion.p[4], motion.p[5],
                        motion.weight_sum, motion.support);
            bool ok = residual_u.WriteRAWToFileF32((output_path + counter + "residual-u" + suffix).c_str()) &&
                      residual_v.WriteRAWToFileF32((output_path + counter + "residual-v" + suffix).c_str());
            if (write_flo) ok = ok && IOUtils::WriteFlowFLO(residual_u, residual_v, output_path + counter + "residual.flo");
            if (!ok) {
                std::cerr << "Error: cannot save file " << std::endl;
                std::exit(255);
            }
        }
        if (segment) {
            flow2d_global_motion motion;
            flow2d_segment_summary summary;
            std::vector<flow2d_motion_region> regions(OpticalFlow2D::kSegmentMaxRegions);
            Data2D labels(width, height);
            optical_flow.SegmentMotion(frame_0, frame_1, global_model, global_sigma, global_iterations, backward, segment_threshold,
                                       segment_join, segment_min_area, &motion, &summary, regions.data(), params, &labels);
            if (!optical_flow.LastRunSucceeded()) {
                std::cout << "Error: the motion segmentation failed." << std::endl;
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            std::printf("Motion segmentation: {\"regions\": %llu, \"foreground\": %llu, \"dropped\": %llu, \"recorded\": %u}\n",
                        summary.region_count, summary.foreground, summary.dropped, summary.recorded);
            for (unsigned k = 0; k < summary.recorded; ++k) {
                const flow2d_motion_region& r = regions[k];
                const double a = static_cast<double>(r.area);
                std::printf("Region %u: {\"area\": %llu, \"bbox\": [%d, %d, %d, %d], \"centroid\": [%.17g, %.17g], "
                            "\"motion\": [%.17g, %.17g]}\n",
                            k + 1, r.area, r.x0, r.y0, r.x1, r.y1, static_cast<double>(r.sum_x) / a, static_cast<double>(r.sum_y) / a,
                            static_cast<double>(r.sum_u_q16) / 65536.0 / a, static_cast<double>(r.sum_v_q16) / 65536.0 / a);
            }
            if (!labels.WriteRAWToFileF32((output_path + counter + "labels" + suffix).c_str())) {
                std::cerr << "Error: cannot save file " << std::endl;
                std::exit(255);
            }
        }
        if (deformation) {
            static const char* const kNames[9] = {"divergence", "vorticity", "dilatation", "exx", "eyy", "exy", "e1", "e2", "max-shear"};
            std::vector<Data2D> planes;
            for (int k = 0; k < 9; ++k) planes.emplace_back(width, height);
            Data2D* wanted[9];
            for (int k = 0; k < 9; ++k) wanted[k] = &planes[k];
            flow2d_deformation_stats stats;
            optical_flow.AnalyseDeformation(frame_0, frame_1, strain_measure, deformation_sigma, backward, wanted, &stats, params);
            if (!optical_flow.LastRunSucceeded()) {
                std::cout << "Error: the deformation analysis failed." << std::endl;
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            std::printf("Deformation: {\"measure\": \"%s\", \"sigma\": %.9g, \"valid\": %llu, \"invalid\": %llu",
                        strain_measure == FLOW2D_STRAIN_SMALL ? "small" : "green", deformation_sigma, stats.valid, stats.invalid);
            const flow2d_deformation_moments* moments[6] = {&stats.divergence, &stats.vorticity, &stats.dilatation,
                                                            &stats.e1,         &stats.e2,        &stats.max_shear};
            static const char* const kStatNames[6] = {"divergence", "vorticity", "dilatation", "e1", "e2", "max_shear"};
            const double n = stats.valid ? static_cast<double>(stats.valid) : 1.0;
            for (int k = 0; k < 6; ++k)
                std::printf(", \"%s\": {\"mean\": %.17g, \"rms\": %.17g, \"min\": %.9g, \"max\": %.9g}", kStatNames[k],
                            moments[k]->sum / n, std::sqrt(moments[k]->sum_sq / n), moments[k]->min, moments[k]->max);
            std::printf("}\n");
            for (int k = 0; k < 9; ++k)
                if (!planes[k].WriteRAWToFileF32((output_path + counter + kNames[k] + suffix).c_str())) {
                    std::cerr << "Error: cannot save file " << std::endl;
                    std::exit(255);
                }
        }
        if (!ground_truth_file.empty()) {
            flow2d_flow_error_stats stats;
            if (!EvaluateFlow(written_u, written_v, gt_u, gt_v, backward ? &occlusion_0 : nullptr, stats)) {
                optical_flow.Destroy();
                DestroyDeviceContext();
                return 4;
            }
            std::printf("Flow error: %s\n", FlowErrorJson(stats).c_str());
            if (refine_radius) {
                if (!EvaluateFlow(computed_u, computed_v, gt_u, gt_v, backward ? &occlusion_0 : nullptr, stats)) {
                    optical_flow.Destroy();
                    DestroyDeviceContext();
                    return 4;
                }
                std::printf("Flow error before refinement: %s\n", FlowErrorJson(stats).c_str());
            }
        }
        optical_flow.Destroy();
    }
    DestroyDeviceContext();
    return 0;
}
