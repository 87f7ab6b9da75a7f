// Coarse-to-fine orchestrator of the flow2d hot path.
// Public interface of the reference's OpticalFlowBase2D / OpticalFlow2D
// (src/optical_flow/optical_flow_base_2d.h:29-52, src/optical_flow/optical_flow_2d.h:43-71):
//   bool Initialize(const DataSize3&, DataConstancy = Grey);
//   void ComputeFlow(Data2D& frame_0, Data2D& frame_1, Data2D& flow_u, Data2D& flow_v, OperationParameters&);
//   void Destroy();   bool silent;
// ComputeFlow bag keys and pointee types (optical_flow_2d.cpp:160-168): warp_levels_count size_t,
// warp_scale_factor float, outer_iterations_count size_t, inner_iterations_count size_t,
// equation_alpha float, equation_smoothness float, equation_data float, median_radius size_t,
// gaussian_sigma float.  Optional superset keys: solver_algorithm int (flow2d_solver_algorithm),
// solver_sor_omega float (opt-in red-black SOR; the default 0 keeps the reference's Jacobi sweeps);
// ComputeFlowBidirectional*: consistency_alpha1, consistency_alpha2 float (occlusion thresholds, default 0.01 / 0.5).
//
// MI355X-first differences (results unchanged): every launch of a pair is queued on one HIP stream
// with no host synchronisation until the flow is copied back (the reference blocks after every
// sweep, cuda_operation_solve_2d.cpp:291); frames may already live in HBM (ComputeFlowDevice).
#pragma once

#include <cstddef>
#include <functional>
#include <map>
#include <vector>

#include "cuda_operations_2d.h"
#include "data2d.h"
#include "data_structs.h"
#include "operation_parameters.h"

class OpticalFlowBase2D {
public:
    const char* GetName() const { return name_; }

    virtual bool Initialize(const DataSize3& data_size, DataConstancy data_constancy = DataConstancy::Grey) = 0;
    virtual void ComputeFlow(Data2D& frame_0, Data2D& frame_1, Data2D& flow_u, Data2D& flow_v,
                             OperationParameters& params);
    virtual void Destroy();
    virtual ~OpticalFlowBase2D();

    // Number of usable pyramid levels (src/optical_flow/optical_flow_base_2d.cpp:36-59); public here so
    // callers and tests can size a run.
    size_t GetMaxWarpLevel(size_t width, size_t height, float scale_factor) const;

protected:
    explicit OpticalFlowBase2D(const char* name) : name_(name) {}
    bool IsInitialized() const;

    bool initialized_ = false;
    DataConstancy data_constancy_ = DataConstancy::Grey;

private:
    const char* name_ = nullptr;
};

struct FlowLevelTiming {
    size_t width, height;
    float solve_ms;   // device time of the level's whole solve call (reference timer, cuda_operation_solve_2d.cpp:220,302)
    float kernel_ms;  // timing_mode 2: summed launch durations of the level's dominant solver kernel, else -1
    int kernel_launches;
    int algorithm;
    double bytes_per_launch;  // algorithmic bytes one launch of that kernel accounts for
};

class OpticalFlow2D : public OpticalFlowBase2D {
public:
    OpticalFlow2D();
    ~OpticalFlow2D() override;

    bool Initialize(const DataSize3& data_size, DataConstancy data_constancy = DataConstancy::Grey) override;
    void ComputeFlow(Data2D& frame_0, Data2D& frame_1, Data2D& flow_u, Data2D& flow_v,
                     OperationParameters& params) override;
    void Destroy() override;

    // Same computation for frames that already sit in pitched device containers of the initialised
    // size (pitch = ContainerSize().pitch).  dev_frame_* are read, dev_flow_* are written.  Nothing is
    // synchronised: the work is queued on the context's stream.  Returns false on a bad argument.
    bool ComputeFlowDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                           OperationParameters& params);

    // Flows of an image sequence: flow k is the flow from frames[k] to frames[k + 1] (frame_count - 1 flows), each
    // bit-identical to ComputeFlowDevice on that pair.  Every frame's pre-blurred plane and pyramid levels are
    // computed once and serve first as the second, then as the first frame of consecutive pairs.
    // Frames are only read; queued on the context's stream, launched eagerly (no graph).
    bool ComputeFlowSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                   const DevicePtr* dev_flows_v, OperationParameters& params);

    // Flows of a sequence in both directions (no reference counterpart; frame_count = 2 is a pair): for every k,
    // (us[k], vs[k]) = the flow frames[k] -> frames[k + 1], bit-identical to ComputeFlowDevice(frames[k], frames[k + 1]), and
    // (back_us[k], back_vs[k]) = the flow frames[k + 1] -> frames[k], bit-identical to ComputeFlowDevice(frames[k + 1], frames[k]).
    // The backward run swaps the two roles of the sequence cache: every frame's pyramid is built once and serves every flow that
    // touches the frame.  With non-null occ_fwd / occ_bwd, occ_fwd[k] (frame k's grid: the forward flow checked against the
    // backward one) and occ_bwd[k] (frame k+1's grid: roles swapped) get the forward-backward consistency masks of
    // flow2d_consistency_2d: 1 = occluded / leaves the frame / NaN, 0 = consistent.  Optional bag keys consistency_alpha1 and
    // consistency_alpha2 (float; 0.01 / 0.5, the paper's values).  Frames are only read; outputs must be distinct from each other
    // and from the frames.  Queued on the context's stream, launched eagerly (no graph).  Not for lock-step groups.
    bool ComputeFlowBidirectionalDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                        const DevicePtr* dev_flows_v, const DevicePtr* dev_back_us, const DevicePtr* dev_back_vs,
                                        const DevicePtr* dev_occ_fwd, const DevicePtr* dev_occ_bwd, OperationParameters& params);
    // The host-image form (the CLI's --backward): upload both frames, ComputeFlowBidirectionalDevice with masks, download all six
    // outputs.  flow_u / flow_v are those of ComputeFlow; LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void ComputeFlowBidirectional(Data2D& frame_0, Data2D& frame_1, Data2D& flow_u, Data2D& flow_v, Data2D& back_u,
                                  Data2D& back_v, Data2D& occlusion_0, Data2D& occlusion_1, OperationParameters& params);

    // Frames between the frames of a sequence (no reference counterpart): for every consecutive pair k it runs
    // ComputeFlowBidirectionalDevice (with the occlusion masks when use_masks) into planes of its own, then one
    // flow2d_interpolate_2d per time: dev_outputs[k * time_count + j] gets the frame at times[j] (0 <= t <= 1) between
    // frames[k] and frames[k + 1], (frame_count - 1) * time_count outputs.  iterations (1 .. 16) and max_residual (finite,
    // >= 0) are those of flow2d_interpolate_2d; use_masks = false interpolates without occlusion masks.  The flows are those of
    // ComputeFlowBidirectionalDevice, bit for bit.  Frames are only read; outputs must be distinct from each other and from the
    // frames.  Queued on the context's stream, launched eagerly (no graph).  Not for lock-step groups.
    bool InterpolateFramesDevice(const DevicePtr* dev_frames, size_t frame_count, const float* times, size_t time_count,
                                 const DevicePtr* dev_outputs, int iterations, float max_residual, bool use_masks,
                                 OperationParameters& params);
    // The host-image form (the CLI's --interpolate): upload both frames, compute both flows (and the masks when use_masks) and
    // the time_count frames of `times` into outputs[0 .. time_count - 1], download.  Non-null flow_u .. occlusion_1 also get
    // the flows and masks of ComputeFlowBidirectional (the masks only with use_masks).  LastRunSucceeded and LastTotalMs as for
    // ComputeFlow.
    void InterpolateFrames(Data2D& frame_0, Data2D& frame_1, const float* times, size_t time_count, Data2D* outputs,
                           int iterations, float max_residual, bool use_masks, OperationParameters& params,
                           Data2D* flow_u = nullptr, Data2D* flow_v = nullptr, Data2D* back_u = nullptr,
                           Data2D* back_v = nullptr, Data2D* occlusion_0 = nullptr, Data2D* occlusion_1 = nullptr);

    // Dense point trajectories through a sequence (Sundaram, Brox & Keutzer, ECCV 2010; no reference counterpart).
    // dev_xs[k] / dev_ys[k] (k < frame_count) are the track table of frame k: `capacity` floats each, slot i = track i's
    // position in frame k, NaN where the track has not started or has ended (a track never restarts).  Frame 0 is seeded
    // (flow2d_seed_points_2d, grid `spacing`, threshold min_eigenvalue); then for every pair k both flows are computed --
    // bit-identical to ComputeFlowBidirectionalDevice on the sequence --, flow2d_track_points_2d carries table k into table
    // k + 1 (forward-backward thresholds: the bag keys consistency_alpha1 / consistency_alpha2, 0.01 / 0.5; motion boundaries
    // with beta1 / beta2 when check_boundaries) and frame k + 1 is seeded.  counts_out[k] (host, frame_count entries) gets the
    // track count after frame k's seeding, read back once at the end (the call synchronises).  Flows are computed in windows
    // of kTrackWindow pairs (pyramids shared inside a window) in planes allocated once: the device memory beyond the caller's
    // tables does not grow with frame_count.  The tables must be distinct and not frames.  Eager; not for lock-step groups.
    static constexpr size_t kTrackWindow = 4;
    // The CLI's seeding threshold (lambda_min of unnormalised 5x5 sums of grey-level gradients; scale-dependent): it keeps
    // the analytic scenes' textures (profiles/tracking/) and drops flat areas.
    static constexpr float kDefaultTrackMinEigenvalue = 1.0f;
    bool TrackPointsDevice(const DevicePtr* dev_frames, size_t frame_count, size_t spacing, float min_eigenvalue,
                           bool check_boundaries, float beta1, float beta2, const DevicePtr* dev_xs, const DevicePtr* dev_ys,
                           size_t capacity, unsigned long long* counts_out, OperationParameters& params);
    // The host-image form (the CLI's --track): upload the frames (frames[k] -> frame k), TrackPointsDevice, download the tables into xs / ys (frame_count * capacity
    // floats each, table k at k * capacity).  LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void TrackPoints(Data2D* const* frames, size_t frame_count, size_t spacing, float min_eigenvalue, bool check_boundaries,
                     float beta1, float beta2, float* xs, float* ys, size_t capacity, unsigned long long* counts_out,
                     OperationParameters& params);

    // Motion-compensated temporal denoising of a sequence (no reference counterpart): dev_outputs[k] (k < frame_count) gets frame k
    // fused by flow2d_denoise_2d with the frames k - radius .. k + radius that exist (fewer at the ends of the sequence), passed
    // in ascending frame order; dev_weight_sums (optional, frame_count planes) get the sums of weights.  The flows and masks are
    // those of ComputeFlowBidirectionalDevice on consecutive pairs, bit for bit: frame k's forward flow and occ_fwd[k] serve
    // neighbour k + 1, the backward flow and occ_bwd[k - 1] of pair k - 1 serve neighbour k - 1; distances of 2 and more are
    // chained outwards from the centre by flow2d_compose_flow_2d (with the masks when use_masks), a broken chain (NaN) dropping
    // out.  range_sigma (grey levels, finite, >= 0; 0 = off) is the scale of the photometric weight; use_masks = false fuses
    // without occlusion masks.  Pairs are computed kDenoiseWindow at a time (pyramids shared inside a window) into a ring of
    // 2 * radius + kDenoiseWindow pairs' planes allocated once: the device memory beyond the caller's planes depends on radius
    // and use_masks, not on frame_count.  frame_count >= 2, radius 1 .. kDenoiseMaxRadius.  Frames are only read; outputs must be
    // distinct from each other and from the frames.  Queued on the context's stream, launched eagerly (no graph).  Not for
    // lock-step groups.
    // (Two pairs per window: a window's last frame is the next window's first, and its pyramid -- a blur and the resampled levels,
    // a few per cent of a pair's flow -- is built again there: one pyramid in three is redundant.  A longer window would share more
    // and cost six planes of ring per pair; not measured.)
    static constexpr size_t kDenoiseWindow = 2;
    static constexpr size_t kDenoiseMaxRadius = 4;
    // frame_count, radius and range_sigma as above (prints what is wrong); needs no device
    static bool DenoiseArgsOk(size_t frame_count, size_t radius, float range_sigma);
    bool DenoiseSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, size_t radius, float range_sigma, bool use_masks,
                               const DevicePtr* dev_outputs, const DevicePtr* dev_weight_sums, OperationParameters& params);
    // The host-image form (the CLI's --denoise): upload the frames (frames[k] -> frame k), DenoiseSequenceDevice, download into
    // outputs[0 .. frame_count - 1] (and weight_sums[...] when not null).  LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void DenoiseSequence(Data2D* const* frames, size_t frame_count, size_t radius, float range_sigma, bool use_masks,
                         Data2D* outputs, Data2D* weight_sums, OperationParameters& params);

    // Global motion of a pair and reference-locked stabilisation of a sequence (no reference counterpart).
    // model: flow2d_motion_model; sigma (pixels, finite, >= 0; 0 = plain least squares) and iterations (0 .. 16) are those of
    // flow2d_global_motion_2d.  GlobalMotionArgsOk prints what is wrong; needs no device.
    static bool GlobalMotionArgsOk(int model, double sigma, int iterations);
    // The composition `second` after `first` of two records, in centred coordinates and in double, in exactly this order:
    //   A = [[1 + p1, p2], [p4, 1 + p5]], t = (p0, p3) of each record;
    //   a11 = A2_11*A1_11 + A2_12*A1_21, a12 = A2_11*A1_12 + A2_12*A1_22, a21 = A2_21*A1_11 + A2_22*A1_21, a22 = A2_21*A1_12 + A2_22*A1_22,
    //   tx = (A2_11*t1x + A2_12*t1y) + t2x,  ty = (A2_21*t1x + A2_22*t1y) + t2y;   p = (tx, a11 - 1, a12, ty, a21, a22 - 1)
    // Translations stay translations and similarities similarities, bit for bit (p1 == p5, p2 == -p4).  weight_sum and support
    // are those of `second` (the newest fit), model_used the larger of the two.
    static flow2d_global_motion ComposeGlobalMotion(const flow2d_global_motion& first, const flow2d_global_motion& second);
    // One pair: the flow frame_0 -> frame_1 (ComputeFlowDevice's bits; with use_masks through ComputeFlowBidirectionalDevice, the
    // forward occlusion mask leaving its vectors out of the fit), flow2d_global_motion_2d, and the record returned to the host
    // (the call synchronises).  Optional planes: dev_flow_u / dev_flow_v get the flow, dev_residual_u / dev_residual_v the flow
    // without the global motion (flow2d_global_flow_2d).
    bool EstimateGlobalMotionDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int model, double sigma, int iterations,
                                    bool use_masks, flow2d_global_motion* motion_out, OperationParameters& params,
                                    DevicePtr dev_flow_u = 0, DevicePtr dev_flow_v = 0, DevicePtr dev_residual_u = 0,
                                    DevicePtr dev_residual_v = 0);
    // The host-image form (the CLI's --global-motion).  LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void EstimateGlobalMotion(Data2D& frame_0, Data2D& frame_1, int model, double sigma, int iterations, bool use_masks,
                              flow2d_global_motion* motion_out, OperationParameters& params, Data2D* flow_u = nullptr,
                              Data2D* flow_v = nullptr, Data2D* residual_u = nullptr, Data2D* residual_v = nullptr);
    // Every frame of a sequence brought onto the grid of frames[reference_index]: for every consecutive pair the flow towards
    // the far side of the reference is fitted -- frame k -> k + 1 for k >= reference_index, frame k + 1 -> k below it; only
    // those directions are computed, both with use_masks (the consistency check needs them) --, each record is downloaded, the
    // records are composed on the host outwards from the reference, M(ref -> k) = M(k - 1 -> k) o M(ref -> k - 1) above it and
    // M(ref -> k) = M(k + 1 -> k) o M(ref -> k + 1) below it (ComposeGlobalMotion), and dev_outputs[k] = frame k resampled by
    // flow2d_warp_global_2d along M(ref -> k), `fill` where that leaves frame k.  The reference frame is copied bit for bit.
    // motions_out (optional, frame_count records) gets M(ref -> k); the reference's is the identity.  The flows are those of
    // ComputeFlowDevice on each ordered pair, bit for bit, computed kStabiliseWindow pairs at a time into planes allocated
    // once: the device memory beyond the caller's planes does not depend on frame_count.  frame_count >= 2.  Frames are only
    // read; outputs must be distinct from each other and from the frames.  The call synchronises.  Not for lock-step groups.
    static constexpr size_t kStabiliseWindow = 2;
    bool StabiliseSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, size_t reference_index, int model, double sigma,
                                 int iterations, bool use_masks, float fill, const DevicePtr* dev_outputs,
                                 flow2d_global_motion* motions_out, OperationParameters& params);
    // The host-image form: upload the frames, StabiliseSequenceDevice, download into outputs[0 .. frame_count - 1].
    void StabiliseSequence(Data2D* const* frames, size_t frame_count, size_t reference_index, int model, double sigma,
                           int iterations, bool use_masks, float fill, Data2D* outputs, flow2d_global_motion* motions_out,
                           OperationParameters& params);

    // Motion segmentation of a pair (no reference counterpart): the flow frame_0 -> frame_1 (bidirectional with use_masks, as in
    // EstimateGlobalMotion), flow2d_global_motion_2d, flow2d_global_flow_2d (the residual planes) and flow2d_segment_motion_2d on
    // them -- with use_masks the forward occlusion mask also keeps its pixels out of the foreground.  threshold (>= 0), join (>= 0,
    // +infinity allowed) and min_area (>= 1) are those of flow2d_segment_motion_2d; SegmentMotionArgsOk prints what is wrong and
    // needs no device.  Returns the global-motion record, the summary and the first min(region_count, kSegmentMaxRegions) records
    // (regions_out: kSegmentMaxRegions records, zero beyond the recorded ones).  The label plane (int labels in a container of
    // the flow's pitch) and the residual planes stay on the device in dev_labels / dev_residual_u / dev_residual_v when given.
    // The object's own planes, table and workspace are allocated at the first call and kept.  The call synchronises.  Not for
    // lock-step groups.
    static constexpr size_t kSegmentMaxRegions = 4096;
    static bool SegmentMotionArgsOk(float threshold, float join, unsigned min_area);
    bool SegmentMotionDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int model, double sigma, int iterations, bool use_masks,
                             float threshold, float join, unsigned min_area, flow2d_global_motion* motion_out,
                             flow2d_segment_summary* summary_out, flow2d_motion_region* regions_out, OperationParameters& params,
                             DevicePtr dev_labels = 0, DevicePtr dev_residual_u = 0, DevicePtr dev_residual_v = 0);
    // The host-image form (the CLI's --segment-motion): `labels` gets the int labels in its float storage, bit for bit.
    void SegmentMotion(Data2D& frame_0, Data2D& frame_1, int model, double sigma, int iterations, bool use_masks, float threshold,
                       float join, unsigned min_area, flow2d_global_motion* motion_out, flow2d_segment_summary* summary_out,
                       flow2d_motion_region* regions_out, OperationParameters& params, Data2D* labels = nullptr,
                       Data2D* residual_u = nullptr, Data2D* residual_v = nullptr);

    // Deformation analysis of a pair (no reference counterpart): the flow frame_0 -> frame_1 (ComputeFlowDevice's bits; with
    // use_masks through ComputeFlowBidirectionalDevice, the forward occlusion mask then being the `mask` of the analysis),
    // optionally flow2d_gaussian_blur of both flow planes with smoothing_sigma > 0 into planes of the object's own (a computed
    // flow is noisy at the pixel scale and strain differentiates that noise: the sigma is the caller's resolution choice; 0 =
    // off), and flow2d_deformation_2d.  measure: flow2d_strain_measure.  dev_planes: nine device planes in the order of
    // flow2d_deformation_planes, 0 = not wanted (the array itself may be null); stats_out (host, optional) gets the record.
    // dev_flow_u / dev_flow_v (optional) get the flow that was analysed -- the smoothed one when there is a sigma --, dev_mask
    // (optional, use_masks only) the occlusion mask.  DeformationArgsOk prints what is wrong and needs no device.  The object's own
    // planes, record and workspace are allocated at the first call and kept.  The call synchronises.  Not for lock-step groups.
    static bool DeformationArgsOk(int measure, float smoothing_sigma);
    bool AnalyseDeformationDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int measure, float smoothing_sigma, bool use_masks,
                                  const DevicePtr* dev_planes, flow2d_deformation_stats* stats_out, OperationParameters& params,
                                  DevicePtr dev_flow_u = 0, DevicePtr dev_flow_v = 0, DevicePtr dev_mask = 0);
    // The host-image form (the CLI's --deformation): planes = nine images in the order of flow2d_deformation_planes, null = not
    // wanted.  LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void AnalyseDeformation(Data2D& frame_0, Data2D& frame_1, int measure, float smoothing_sigma, bool use_masks,
                            Data2D* const* planes, flow2d_deformation_stats* stats_out, OperationParameters& params,
                            Data2D* flow_u = nullptr, Data2D* flow_v = nullptr, Data2D* mask = nullptr);

    // Edge-aware refinement of a pair's flow (no reference counterpart): the flow frame_0 -> frame_1 (ComputeFlowDevice's bits;
    // with use_masks through ComputeFlowBidirectionalDevice, the forward occlusion mask then being the `mask` of the filter), then
    // `iterations` passes of flow2d_refine_flow_2d with frame 0 as the guide, the mask applied in every pass, ping-ponging between
    // planes of the object's own; the last pass writes dev_refined_u / dev_refined_v.  record_out (host, optional) gets the record
    // of the last pass.  dev_flow_u / dev_flow_v (optional) get the flow before the refinement and dev_mask (optional, use_masks
    // only) the occlusion mask -- or, with flow_given, they ARE the flow to refine, computed elsewhere by the caller, and (optional)
    // its mask: no flow is computed then and dev_frame_1 is not used.  RefineArgsOk prints what is wrong and needs no device.  The
    // object's own planes and record are allocated at the first call and kept.  The call synchronises.  Not for lock-step groups.
    static constexpr int kRefineMaxIterations = 16;
    static bool RefineArgsOk(int radius, float sigma_guide, float sigma_space, int iterations);
    bool RefineFlowDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int radius, float sigma_guide, float sigma_space,
                          int iterations, bool use_masks, DevicePtr dev_refined_u, DevicePtr dev_refined_v,
                          flow2d_refine_record* record_out, OperationParameters& params, DevicePtr dev_flow_u = 0,
                          DevicePtr dev_flow_v = 0, DevicePtr dev_mask = 0, bool flow_given = false);
    // The host-image form (the CLI's --refine).  LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void RefineFlow(Data2D& frame_0, Data2D& frame_1, int radius, float sigma_guide, float sigma_space, int iterations,
                    bool use_masks, Data2D& refined_u, Data2D& refined_v, flow2d_refine_record* record_out,
                    OperationParameters& params, Data2D* flow_u = nullptr, Data2D* flow_v = nullptr, Data2D* mask = nullptr);

    // Window correlation (the reference's Methods::Correlation, which it declares and never shipped): flow2d_correlate_2d on the
    // pair -- both frames quantised to 8 bits by (I - lo) * scale; every node of the grid of flow2d_correlation_grid gets the
    // displacement, within `range`, at which its (2 radius + 1)^2 window of frame 0 correlates best with frame 1 --, no part of the
    // variational pyramid.  dev_node_u / dev_node_v / dev_node_score (each optional) are planes of the CONTAINER's size and pitch
    // whose first nw x nh floats get the node field; without them planes of the object's own are used.  record_out (host,
    // optional) gets the counts.  dev_flow_u / dev_flow_v (optional, both or neither) get the field on the frame's grid
    // (flow2d_expand_nodes_2d), ready for every consumer of a dense flow.  CorrelationArgsOk prints what is wrong and needs no
    // device.  The object's own planes and record are allocated at the first call and kept.  The call synchronises.  Not for
    // lock-step groups.
    static bool CorrelationArgsOk(size_t width, size_t height, float lo, float scale, int radius, int range, int spacing,
                                  float min_score);
    bool CorrelateDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, int radius, int range, int spacing,
                         float min_score, DevicePtr dev_node_u, DevicePtr dev_node_v, DevicePtr dev_node_score,
                         flow2d_correlation_record* record_out, DevicePtr dev_flow_u = 0, DevicePtr dev_flow_v = 0);
    // lo and scale as Correlate chooses them, from the finite minimum and maximum of the two images: 0 and 1 when they lie in
    // [0, 255] already (8-bit data is taken as it is), else the range onto 0 .. 255.  Needs no device.
    static void CorrelationRange(Data2D& frame_0, Data2D& frame_1, float& lo, float& scale);
    // The host-image form (the CLI's --correlation): node_u / node_v (and node_score, optional) are nw x nh images.
    // LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void Correlate(Data2D& frame_0, Data2D& frame_1, int radius, int range, int spacing, float min_score, Data2D& node_u,
                   Data2D& node_v, Data2D* node_score, flow2d_correlation_record* record_out, Data2D* flow_u = nullptr,
                   Data2D* flow_v = nullptr);

    // Multi-pass window correlation (multi-grid interrogation with a discrete window offset; the normalised median test between
    // passes): 1 .. FLOW2D_CORRELATION_MAX_PASSES passes, each flow2d_correlate_offset_2d around the current predictor -- NULL in
    // pass 1 unless dev_predictor_u / dev_predictor_v (optional, both or neither: a dense flow in planes of the container's size,
    // only read) are given --, then flow2d_validate_nodes_2d in REPLACE mode and flow2d_expand_nodes_2d into planes of the
    // object's own, which are the next pass's predictor.  After the last pass the test runs in the caller's mode
    // (validation.replace; not at all without validation.validate_last); node planes (optional, as for CorrelateDevice) and score
    // come from that pass, dev_flow_u / dev_flow_v (optional, both or neither) get its field on the frame's grid.  reports_out
    // (host, optional, one per pass): the grid and both records; the validation record of a last pass that was not validated is
    // zero.  CorrelationPassesOk prints what is wrong and needs no device.  Planes and records are allocated at the first call
    // and kept.  The call synchronises once, at the end.  Not for lock-step groups.
    struct CorrelationPass {
        int radius, range, spacing;
    };
    struct ValidationOptions {
        float threshold = 2.f, epsilon = 0.1f;
        int min_neighbours = 3;
        bool replace = true, validate_last = true;
        // A region of interest through the passes (flow2d_correlate_masked_2d, flow2d_validate_nodes_masked_2d in place of the two
        // entries above, in every pass; the expansion is unchanged): mask, a device plane of the frames' size and pitch in frame
        // 0's coordinates, 0 = none -- the calls there always were --, whose values of 0.5 and more (and NaN) mean "not the
        // specimen".  A node whose centre is excluded or whose window keeps fewer than min_pixels pixels is masked (NaN); 0 = per
        // pass max(6, ((2 radius + 1)^2 + 3) / 4), an explicit value must fit every pass's window.  The masked counts are the
        // seventh words of the reports' records (reserved[0]).
        DevicePtr mask = 0;
        int min_pixels = 0;
    };
    // min_pixels as a pass of `radius` gets it: the default where it is 0
    static int CorrelationMinPixels(const ValidationOptions& validation, int radius);
    struct CorrelationPassReport {
        size_t nw, nh;
        flow2d_correlation_pass_record correlation;
        flow2d_validation_record validation;
    };
    static bool CorrelationPassesOk(size_t width, size_t height, float lo, float scale, const CorrelationPass* passes, size_t count,
                                    float min_score, const ValidationOptions& validation);
    bool CorrelateMultiPassDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, const CorrelationPass* passes,
                                  size_t count, float min_score, const ValidationOptions& validation, DevicePtr dev_predictor_u,
                                  DevicePtr dev_predictor_v, DevicePtr dev_node_u, DevicePtr dev_node_v, DevicePtr dev_node_score,
                                  CorrelationPassReport* reports_out, DevicePtr dev_flow_u = 0, DevicePtr dev_flow_v = 0);
    // The host-image form (the CLI's --correlation-passes): lo and scale from CorrelationRange; node_u / node_v (and node_score,
    // optional) are images of the LAST pass's grid; predictor_u / predictor_v (optional, both or neither): the initial predictor;
    // mask (optional): an image of the frames' size in place of validation.mask, which this form does not look at; the object
    // uploads it once per call.
    void CorrelateMultiPass(Data2D& frame_0, Data2D& frame_1, const CorrelationPass* passes, size_t count, float min_score,
                            const ValidationOptions& validation, Data2D& node_u, Data2D& node_v, Data2D* node_score,
                            CorrelationPassReport* reports_out, Data2D* flow_u = nullptr, Data2D* flow_v = nullptr,
                            Data2D* predictor_u = nullptr, Data2D* predictor_v = nullptr, Data2D* mask = nullptr);

    // Subset refinement of correlation nodes (flow2d_subset_refine_2d: the inverse-compositional Gauss-Newton iteration with an
    // affine shape function, on the fp32 frames): the second half of a digital image correlation.  All planes are planes of the
    // CONTAINER's size and pitch whose first nw x nh floats hold a node field.
    struct SubsetOptions {
        int radius = 7, iterations = 20;
        float epsilon = 1e-3f, max_shift = 2.f, max_gradient = 0.5f;
        // order 2: the twelve-parameter refinement (flow2d_subset_refine2_2d) in every call that refines, radius from 2; a
        // curvature beyond max_curvature (per pixel; a bound, not a tuned value) strays.  Order 1 takes the calls it always took.
        int order = 1;
        float max_curvature = 0.05f;
        // A region of interest (flow2d_subset_refine_masked_2d): mask, a device plane of the frames' size and pitch in frame 0's
        // coordinates, 0 = none, whose values of 0.5 and more (and NaN) mean "not the specimen"; a node with fewer than min_pixels
        // usable pixels is masked (state -4, NaN), 0 = max(6, ((2 radius + 1)^2 + 3) / 4).  Every call that refines passes them
        // on.  In a sequence every step uses the same mask, frame 0's: a masked node comes out of flow2d_predict_nodes_2d
        // predicted from its neighbours and goes back to masked in the refinement, so it never serves a later step as a start of
        // its own.  Order 1 only: SubsetOptionsOk refuses a mask with order 2.
        DevicePtr mask = 0;
        int min_pixels = 0;
        // The region of interest through the whole chain: with a mask, the calls that run the passes of a pair -- CorrelateSubset*,
        // step 1 of CorrelateSubsetSequence* and every later step that runs the pair chain -- hand it to their passes
        // (ValidationOptions::mask; the search's min_pixels stays validation.min_pixels), so that an edge node starts from the
        // specimen's motion and not the background's.  False keeps the calls there always were, byte for byte: that is why it is a
        // flag and not implied by the mask.  SubsetOptionsOk refuses it without a mask.
        bool mask_search = false;
        // How frame 1 is sampled.  BSpline: every call that refines prefilters its frame 1 -- in a sequence every step its frame k
        // -- into a plane of the object's own (flow2d_bspline_prefilter_2d) and calls the spline entry of its order
        // (flow2d_subset_refine_spline_2d, flow2d_subset_refine2_spline_2d); mask and start gradients go through.  A tenth of the
        // Catmull-Rom sample's interpolation bias for the same sixteen taps and one more launch per frame.
        enum Interpolation { CatmullRom = 0, BSpline = 1 };
        int interpolation = CatmullRom;
    };
    // min_pixels as the refinement gets it: the default where it is 0
    static int SubsetMinPixels(const SubsetOptions& subset);
    struct SubsetPlanes {
        DevicePtr u = 0, v = 0;                    // both or neither: without them planes of the object's own are written
        DevicePtr ux = 0, uy = 0, vx = 0, vy = 0;  // the four gradients: all or none
        DevicePtr score = 0, state = 0;            // each optional
        DevicePtr uxx = 0, uxy = 0, uyy = 0, vxx = 0, vxy = 0, vyy = 0;  // the six curvatures, order 2 only: all or none
    };
    // prints what is wrong; needs no device
    static bool SubsetOptionsOk(const SubsetOptions& subset);
    // The nodes (dev_node_u0, dev_node_v0) of the grid (grid_radius, spacing) refined into `out`.  record_out (host, optional): the
    // counts, read back -- the call then synchronises, otherwise it only queues.  Its planes and record are allocated at the first
    // use and kept.  Not for lock-step groups.
    bool RefineNodesDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_node_u0, DevicePtr dev_node_v0, int grid_radius,
                           int spacing, const SubsetOptions& subset, const SubsetPlanes& out, flow2d_subset_record* record_out = nullptr);
    // The whole chain: the passes of CorrelateMultiPassDevice (one pass without a predictor is CorrelateDevice's search) with the
    // last pass validated in REPLACE mode whatever `validation` says of it, so that every node has a start; then the refinement on
    // the last pass's grid into `out`; dev_flow_u / dev_flow_v (optional, both or neither) get the refined (u, v) on the frame's
    // grid (flow2d_expand_nodes_2d).  reports_out (optional, one per pass) and record_out (optional) as there and above.  The call
    // synchronises once, at the end.  Not for lock-step groups.
    bool CorrelateSubsetDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, const CorrelationPass* passes,
                               size_t count, float min_score, const ValidationOptions& validation, const SubsetOptions& subset,
                               DevicePtr dev_predictor_u, DevicePtr dev_predictor_v, const SubsetPlanes& out,
                               CorrelationPassReport* reports_out, flow2d_subset_record* record_out, DevicePtr dev_flow_u = 0,
                               DevicePtr dev_flow_v = 0);
    // The host-image form (the CLI's --subset-refine): lo and scale from CorrelationRange; nodes[8] -- u, v, ux, uy, vx, vy, score,
    // state; u and v are needed, the gradients come all or none -- are images of the LAST pass's grid.  With subset.order == 2 this
    // and the two other host-image forms below take nodes[14] per step: those eight, then uxx, uxy, uyy, vxx, vxy, vyy, all or none.
    void CorrelateSubset(Data2D& frame_0, Data2D& frame_1, const CorrelationPass* passes, size_t count, float min_score,
                         const ValidationOptions& validation, const SubsetOptions& subset, Data2D* const* nodes,
                         CorrelationPassReport* reports_out, flow2d_subset_record* record_out, Data2D* flow_u = nullptr,
                         Data2D* flow_v = nullptr, Data2D* predictor_u = nullptr, Data2D* predictor_v = nullptr, Data2D* mask = nullptr);
    // (mask, here and in the two other host-image forms below: an image of the frames' size in place of subset.mask, which these
    // forms do not look at; the object uploads it once per call)

    // DIC over a loading sequence: every frame is correlated against the same reference frame, and from the second step on the
    // start of a step is the previous step's deformation, gradients included (flow2d_predict_nodes_2d, then
    // flow2d_subset_refine_from_2d), so that no window search runs and a subset that has rotated or stretched beyond a rigid
    // window's reach is still followed.  At order 2 the steps after the first start from the prediction's six first-order planes
    // with zero curvatures (flow2d_predict_nodes_2d knows no curvature; the refinement finds it again in about one iteration more).
    // RefineNodesDevice started from a whole deformation: `start` gives u, v and the four gradients (score and state are not looked
    // at); the rest as there.
    bool RefineNodesFromDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, const SubsetPlanes& start, int grid_radius, int spacing,
                               const SubsetOptions& subset, const SubsetPlanes& out, flow2d_subset_record* record_out = nullptr);
    static constexpr int kSequenceMaxFill = 4;
    struct SequenceOptions {
        int fill = 2;            // prediction passes per step, 1 .. kSequenceMaxFill: each refills the lost nodes one ring further
        int min_state = 1;       // 1: converged nodes are kept; 0: also those that ran out of iterations
        int min_neighbours = 1;  // usable neighbours a lost node needs to be predicted, 1 .. 8
        float max_shift = 4.f;   // of the steps after the first, in place of subset.max_shift: the motion of one step
        // Incremental correlation: 0 = never (every step against frame 0); N >= 1: step k is measured against frame
        // ref(k) = N * floor((k - 1) / N), on the same grid laid in that frame, and composed with the deformation up to it
        // (flow2d_compose_nodes_2d), so that what is delivered stays "frame 0 -> frame k at the nodes of frame 0".
        int reference_every = 0;
    };
    struct SequenceStepReport {
        flow2d_subset_record subset;
        flow2d_predict_record prediction[kSequenceMaxFill];  // of the passes that ran; zero in step 1 and beyond `fill`
    };
    // prints what is wrong; needs no device
    static bool SequenceOptionsOk(const SequenceOptions& sequence);
    // dev_frames[0 .. frame_count - 1], frame_count >= 2; dev_frames[0] is the reference.  Step 1 (frames 0, 1) is
    // CorrelateSubsetDevice's chain.  Step k >= 2 (frames 0, k): sequence.fill passes of flow2d_predict_nodes_2d on step k - 1's
    // planes, ping-pong between two sets of planes of the object's own, then flow2d_subset_refine_from_2d with
    // sequence.max_shift.  out[k - 1] gets step k's planes: u, v, the gradients and the state are needed (they are the next step's
    // input), the score is optional; no plane may serve two steps.  dev_flows (optional): 2 * (frame_count - 1) planes, u and v
    // per step, each pair optional: the step's (u, v) on the frame's grid (flow2d_expand_nodes_2d).  first_reports (optional, one
    // per pass) as for CorrelateSubsetDevice; steps_out (optional, frame_count - 1).  There is no new search when many nodes are
    // lost: the records say so, and the caller decides.  Everything is queued on the stream, the records are read back after
    // one synchronisation at the end.  Not for lock-step groups.
    //
    // With sequence.reference_every = N >= 1 the reference moves: step k is measured against frame ref(k) = N * floor((k - 1) / N).
    // The steps with ref = 0 are the ones above, bit for bit.  At a step with ref(k) = k - 1 > 0, the first after a change, the
    // *base* of the new reference is built once -- sequence.fill passes of flow2d_predict_nodes_2d over the delivered planes of
    // step ref, so that its holes are refilled -- and the *increment* is CorrelateSubsetDevice's chain on (frame ref, frame k), the
    // way step 1 runs, with the caller's passes, lo and scale; the later steps of the same reference are the prediction passes and
    // the refinement from the previous increment, with sequence.max_shift.  The increments stay in planes of the object's own
    // (each is the next step's start); out[k - 1] gets flow2d_compose_nodes_2d of base and increment with sequence.min_state: the
    // six planes and the state, state FLOW2D_SUBSET_STATE_COMPOSED or -1, and the increment's score blended where a score plane is
    // given; dev_flows the composed (u, v).  steps_out[k - 1].subset is the increment's refinement; its prediction records are those
    // of the increment's start, or at a reference change those of the base.  compose_out (optional, frame_count - 1): the
    // composition's record per step, zero for the steps with ref = 0.  A moving reference is refused with a mask (it lies in frame
    // 0's coordinates, and the later references' subsets do not) and with curvature planes in `out` (order 2 itself runs: the
    // composition knows gradients only).  Still everything is queued and the call synchronises once.
    bool CorrelateSubsetSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, float lo, float scale, const CorrelationPass* passes,
                                       size_t count, float min_score, const ValidationOptions& validation, const SubsetOptions& subset,
                                       const SequenceOptions& sequence, const SubsetPlanes* out, CorrelationPassReport* first_reports,
                                       SequenceStepReport* steps_out, const DevicePtr* dev_flows = nullptr,
                                       flow2d_compose_record* compose_out = nullptr);
    // The host-image form: lo and scale from CorrelationRange of frames 0 and 1; nodes[8 * (k - 1) + 0 .. 7] -- u, v, ux, uy, vx,
    // vy, score, state of step k, images of the last pass's grid, all but the score needed; flows (optional): 2 per step.
    void CorrelateSubsetSequence(Data2D* const* frames, size_t frame_count, const CorrelationPass* passes, size_t count, float min_score,
                                 const ValidationOptions& validation, const SubsetOptions& subset, const SequenceOptions& sequence,
                                 Data2D* const* nodes, CorrelationPassReport* first_reports, SequenceStepReport* steps_out,
                                 Data2D* const* flows = nullptr, Data2D* mask = nullptr, flow2d_compose_record* compose_out = nullptr);

    // The composition of two node fields across a moved reference (flow2d_compose_nodes_2d): `base` -- frame 0 -> frame r at the
    // nodes of frame 0 -- and `increment` -- frame r -> frame k on the same grid (grid_radius, spacing) laid in frame r -- give u, v,
    // the four gradients and the state each; `out` gets frame 0 -> frame k: u, v and the gradients are needed, the state is
    // optional, the score goes with increment.score (without out.score the increment's is not looked at).  min_state as in
    // SequenceOptions.  record_out (host, optional): the counts, read back -- the call then synchronises, otherwise it only
    // queues.  Not for lock-step groups.
    bool ComposeNodesDevice(const SubsetPlanes& base, const SubsetPlanes& increment, int grid_radius, int spacing, int min_state,
                            const SubsetPlanes& out, flow2d_compose_record* record_out = nullptr);
    // The host-image form: base[7] -- u, v, ux, uy, vx, vy, state --, increment[8] and nodes[8] -- u, v, ux, uy, vx, vy, score, state,
    // of which the increment's score and the nodes' score and state are optional --, images of the grid.
    void ComposeNodes(Data2D* const* base, Data2D* const* increment, int grid_radius, int spacing, int min_state, Data2D* const* nodes,
                      flow2d_compose_record* record_out = nullptr);

    // The uncertainty of a first-order refinement's nodes (flow2d_subset_uncertainty_2d): per node the covariance s2 * H^-1 of
    // p -- the standard deviations of u, v and the four gradients, the correlation of u and v, and sqrt(s2) in grey values.  They
    // estimate the random error the frames' noise puts into p and say nothing about the sample's interpolation bias.
    struct UncertaintyPlanes {
        DevicePtr sigma_u = 0, sigma_v = 0;                                // needed
        DevicePtr rho = 0;                                                 // optional
        DevicePtr sigma_ux = 0, sigma_uy = 0, sigma_vx = 0, sigma_vy = 0;  // all or none
        DevicePtr noise = 0;                                               // optional
    };
    // `nodes` holds u, v, the four gradients and the state of a first-order refinement of (dev_frame_0, dev_frame_1) on the grid
    // (grid_radius, spacing); a node below min_state (0 or 1) is skipped.  Of `subset` the radius, the mask with min_pixels (0: the
    // default) and the interpolation are used: with BSpline frame 1 is prefiltered into the object's coefficient plane first.
    // Refused, with a printed reason, for subset.order == 2 and for curvature planes: twelve parameters need a 12 x 12
    // covariance, which is not built here.  record_out (host, optional): the counts, read back -- the call then synchronises,
    // otherwise it only queues.  Not for lock-step groups.
    // prints what is wrong (order 2 among it); needs no device
    static bool UncertaintyOptionsOk(const SubsetOptions& subset, int min_state);
    bool NodeUncertaintyDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, const SubsetPlanes& nodes, int grid_radius, int spacing,
                               const SubsetOptions& subset, int min_state, const UncertaintyPlanes& out,
                               flow2d_uncertainty_record* record_out = nullptr);
    // The host-image form: nodes[8] -- u, v, ux, uy, vx, vy, score, state as CorrelateSubset delivers them, the score not looked at
    // and optional -- and out[8] -- sigma_u, sigma_v, rho, sigma_ux, sigma_uy, sigma_vx, sigma_vy, noise --, images of the grid;
    // mask (optional): an image of the frames' size in place of subset.mask, which this form does not look at.
    void NodeUncertainty(Data2D& frame_0, Data2D& frame_1, Data2D* const* nodes, int grid_radius, int spacing, const SubsetOptions& subset,
                         int min_state, Data2D* const* out, flow2d_uncertainty_record* record_out = nullptr, Data2D* mask = nullptr);

    // One later step on its own, for a sequence that arrives frame by frame (the CLI's --subset-previous): `previous` holds the
    // last step's u, v, gradients and state (its score is not looked at); the prediction's passes and the refinement of
    // (dev_frame_0, dev_frame_k) with sequence.max_shift into `out`, as CorrelateSubsetSequenceDevice runs them per step.
    // report_out (optional).  Synchronises.  dev_frame_0 may be any frame: with a moved reference the caller passes the reference
    // frame and the previous INCREMENT (not the composed field) as `previous`, and composes `out` with the base of that reference
    // by ComposeNodesDevice; sequence.reference_every is not looked at here.  The composition's record tells when the reference
    // should move again (many nodes outside or without an increment); there is no automatic policy, which would need the
    // device's counts on the host at every step.
    bool ContinueSubsetSequenceDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_k, const SubsetPlanes& previous, int grid_radius,
                                      int spacing, const SubsetOptions& subset, const SequenceOptions& sequence, const SubsetPlanes& out,
                                      SequenceStepReport* report_out, DevicePtr dev_flow_u = 0, DevicePtr dev_flow_v = 0);
    // Its host-image form: previous[7] -- u, v, ux, uy, vx, vy, state -- and nodes[8] as for CorrelateSubset, images of the grid.
    void ContinueSubsetSequence(Data2D& frame_0, Data2D& frame_k, Data2D* const* previous, int grid_radius, int spacing,
                                const SubsetOptions& subset, const SequenceOptions& sequence, Data2D* const* nodes,
                                SequenceStepReport* report_out, Data2D* flow_u = nullptr, Data2D* flow_v = nullptr, Data2D* mask = nullptr);

    // Strain on the node grid (flow2d_node_strain_2d): the nine quantities of flow2d_deformation_2d at every node, from the
    // gradients a refinement delivered (window 0) or from a polynomial of `order` fitted by least squares to the usable nodes
    // within `window` nodes around each node (Pan et al. 2009); nodes below min_state, and nodes that are not finite, are left
    // out of every fit.  min_nodes: the fewest usable nodes a window may hold, 0 = one more than the fit has coefficients.
    // robust_sigma > 0 (pixels; with a window of 1 or more) makes the fit the reweighted one of flow2d_node_strain_robust_2d:
    // robust_iterations passes with a Cauchy weight of that scale, taps further than it from the last fit not kept, a window
    // that keeps fewer than min_nodes sparse.  8 passes are what an order-2 fit at m = 2 needs; order 1 settles within 4
    // (profiles/robust_strain/README.md).  0 = off: the plain entry, the iterations are not looked at.
    // weighted (with a window of 1 or more, and the forms below that take the nodes' sigma planes) makes the fit the Gauss-Markov
    // one of flow2d_node_strain_weighted_2d: every tap weighted by 1 / (sigma^2 + sigma_floor^2) of its node, sigma_floor in
    // pixels (finite, >= 0: what the uncertainty does not see, the sampler's bias above all).  weight_threshold T > 0 adds that
    // entry's reweighted passes with the scale in sigmas, robust_iterations of them; T = 0: none, the iterations are not looked
    // at.  robust_sigma and weighted exclude each other: one scale is in pixels and the other in sigmas.
    struct StrainOptions {
        int window = 2, order = 1, min_nodes = 0 /* 0: k + 1 */, min_state = 1, measure = FLOW2D_STRAIN_SMALL;
        float robust_sigma = 0.f;
        int robust_iterations = 8;
        bool weighted = false;
        float sigma_floor = 0.f, weight_threshold = 0.f;
    };
    // The nine planes of flow2d_strain_sigma_planes as device planes of the container's size, 0 = not wanted.
    struct StrainSigmaPlanes {
        DevicePtr sigma_ux = 0, sigma_uy = 0, sigma_vx = 0, sigma_vy = 0, sigma_divergence = 0, sigma_vorticity = 0, sigma_exx = 0,
                  sigma_eyy = 0, sigma_exy = 0;
    };
    // prints what is wrong; needs no device
    static bool StrainOptionsOk(const StrainOptions& strain);
    // One node field, or every step of a sequence: steps[k] holds step k's planes as RefineNodesDevice / CorrelateSubset*Device
    // wrote them -- u and v are needed, the gradients (all or none) only with window 0, the state is optional (without it every
    // finite node is usable: a field that comes from the search alone), the score is not looked at.  nw x nh: the grid, in planes
    // of the container's size and pitch.  out_planes: nine device planes per step in the order of flow2d_deformation_planes,
    // 0 = not wanted (the array may be null when stats_out is given); stats_out (host, optional): step_count records.  One launch
    // pair per step; the records and the workspace are allocated at the first use and kept; the call synchronises once, at the
    // end, and only when stats_out is given.  Not for lock-step groups.
    // diagnostics (optional, with robust_sigma > 0 only): three device planes per step -- residual, rejected, centre of
    // flow2d_node_strain_diagnostics --, 0 = not wanted; they count as wanted planes.  The records then carry reserved[3 .. 5].
    bool NodeStrainDevice(const SubsetPlanes* steps, size_t step_count, size_t nw, size_t nh, int spacing, const StrainOptions& strain,
                          const DevicePtr* out_planes, flow2d_deformation_stats* stats_out, const DevicePtr* diagnostics = nullptr);
    // The host-image form: nodes[7 * k + 0 .. 6] -- u, v, ux, uy, vx, vy, state of step k, images of the nw x nh grid, of which u and
    // v are needed -- and planes[9 * k + 0 .. 8], images of the grid, null = not wanted.
    // diagnostics[3 * k + 0 .. 2] (optional, with robust_sigma > 0 only): images of the grid, null = not wanted.
    void NodeStrain(Data2D* const* nodes, size_t step_count, int spacing, const StrainOptions& strain, Data2D* const* planes,
                    flow2d_deformation_stats* stats_out, Data2D* const* diagnostics = nullptr);
    // The weighted forms (strain.weighted; flow2d_node_strain_weighted_2d): as above, with uncertainty[2 * k + 0 .. 1] -- sigma_u and
    // sigma_v of step k as NodeUncertainty[Device] wrote them, both needed -- and strain_sigmas (optional): one StrainSigmaPlanes
    // per step, or images strain_sigmas[9 * k + 0 .. 8] in that struct's order, null = not wanted; they count as wanted planes,
    // and so do the diagnostic planes, whose residual and centre are in sigmas here.  The records carry reserved[3 .. 6].
    bool NodeStrainDevice(const SubsetPlanes* steps, size_t step_count, size_t nw, size_t nh, int spacing, const StrainOptions& strain,
                          const DevicePtr* uncertainty, const DevicePtr* out_planes, flow2d_deformation_stats* stats_out,
                          const DevicePtr* diagnostics, const StrainSigmaPlanes* strain_sigmas);
    void NodeStrain(Data2D* const* nodes, size_t step_count, int spacing, const StrainOptions& strain, Data2D* const* uncertainty,
                    Data2D* const* planes, flow2d_deformation_stats* stats_out, Data2D* const* diagnostics, Data2D* const* strain_sigmas);

    // The pyramid started from a prior flow instead of from zero at the coarsest level (no reference counterpart; Brox & Malik's
    // large-displacement flow and the predictor-corrector passes of PIV start the variational solver from matches in the same
    // way).  dev_prior_u / dev_prior_v: a flow in full-resolution pixels in planes of the container's size, only read; a pixel
    // where either component is not finite enters as (0, 0) and is counted.  The level loop starts at the level
    // PriorStartLevel gives instead of at the top one, and that level's warp is flow2d_prior_registration_2d -- the prior brought
    // to the level's size, stored as its base flow and frame 1 warped by it -- instead of the zero-fill form; the frame pyramid,
    // the later levels and the delivery are those of ComputeFlowDevice (an all-zero prior started at the top level gives its
    // bytes).  Optional bag keys: prior_reach (float, pixels, default 2: how far the solver is trusted to correct the prior) and
    // prior_level (int: the start level itself, overriding the rule).  With use_graph the recorded pyramid is keyed by the prior's
    // planes and the start level as well.  report_out (optional) gets the start level, the number of levels run and the count of
    // prior pixels that were not finite; the call then synchronises, otherwise it only queues.  The prior planes must not meet
    // the flow planes or any plane of the object's own.  Not for lock-step groups; there is no prior for a backward flow, so
    // ComputeFlowBidirectional* refuse a bag that carries prior_reach or prior_level.
    struct PriorReport {
        size_t start_level = 0, levels_run = 0;
        unsigned long long not_finite = 0;
    };
    // The start level: the smallest l >= 0 with reach * std::pow(warp_scale_factor, (float)l) <= 1 -- the float pow of the level
    // geometry --, at most the top level min(warp_levels_count, GetMaxWarpLevel(...)) - 1 of the unseeded run; prior_level >= 0
    // replaces the rule (clamped alike), -1 = not given.  False (and a message) for a reach that is not finite and > 0, a
    // prior_level below -1, or parameters with which no level runs.  Needs no device.
    static bool PriorStartLevel(size_t width, size_t height, size_t warp_levels_count, float warp_scale_factor, float reach,
                                int prior_level, size_t* start_level);
    bool ComputeFlowFromPriorDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_prior_u, DevicePtr dev_prior_v,
                                    DevicePtr dev_flow_u, DevicePtr dev_flow_v, OperationParameters& params,
                                    PriorReport* report_out = nullptr);
    // The host-image form (the CLI's --initial-flow).  LastRunSucceeded and LastTotalMs as for ComputeFlow.
    void ComputeFlowFromPrior(Data2D& frame_0, Data2D& frame_1, Data2D& prior_u, Data2D& prior_v, Data2D& flow_u, Data2D& flow_v,
                              OperationParameters& params, PriorReport* report_out = nullptr);
    // Window correlation as the prior: CorrelateDevice (arguments as there) with its field expanded to the frame's grid
    // (flow2d_expand_nodes_2d) into planes of the object's own, then ComputeFlowFromPriorDevice from that field.  No refinement
    // pass in between: pixels whose four nodes are all invalid are NaN in the expansion, enter as 0 and are counted.  The node
    // planes (optional, as for CorrelateDevice) and correlation_out keep the correlation's own result; dev_prior_u / dev_prior_v
    // (optional, both or neither) get a copy of the expanded field.  The call synchronises.
    bool ComputeFlowCorrelationSeededDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, int radius, int range,
                                            int spacing, float min_score, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                                            OperationParameters& params, DevicePtr dev_node_u = 0, DevicePtr dev_node_v = 0,
                                            DevicePtr dev_node_score = 0, flow2d_correlation_record* correlation_out = nullptr,
                                            PriorReport* report_out = nullptr, DevicePtr dev_prior_u = 0, DevicePtr dev_prior_v = 0);
    // The host-image form (the CLI's --correlation-prior): lo and scale from CorrelationRange; node_u / node_v / node_score and
    // prior_u / prior_v are optional images (nw x nh and the frame's size).
    void ComputeFlowCorrelationSeeded(Data2D& frame_0, Data2D& frame_1, int radius, int range, int spacing, float min_score,
                                      Data2D& flow_u, Data2D& flow_v, OperationParameters& params, Data2D* node_u = nullptr,
                                      Data2D* node_v = nullptr, Data2D* node_score = nullptr,
                                      flow2d_correlation_record* correlation_out = nullptr, PriorReport* report_out = nullptr,
                                      Data2D* prior_u = nullptr, Data2D* prior_v = nullptr);

    // Warm starts: the previous pair's flow, carried along itself onto this pair's grid (flow2d_propagate_flow_2d), as the prior of
    // ComputeFlowFromPriorDevice (no reference counterpart).  In a sequence the prior costs a splat and no correlation, and the
    // pyramid runs from PriorStartLevel down instead of from the top.
    //   fill_passes, photo_scale: those of flow2d_propagate_flow_2d (photo_scale acts only where both frames are there).
    //   tail: < 0 -- no adaptation: every seeded pair uses the bag's prior_reach / prior_level.  In [0, 1) -- the adaptive mode of
    //   ComputeFlowSequenceWarmDevice: the share of pixels a prediction may miss by more than the reach (WarmNextReach).
    struct WarmOptions {
        int fill_passes = 4;
        float photo_scale = 1.f;
        float tail = -1.f;
    };
    enum WarmMode { kWarmUnseeded = 0, kWarmSeeded = 1, kWarmRedone = 2 };
    struct WarmReport {
        int mode = kWarmUnseeded;
        int reach = 0;  // adaptive mode: the reach the pair was seeded with (1 .. 3), 0 when it ran unseeded
        PriorReport prior;  // of the seeded run (zeros for an unseeded pair)
        flow2d_propagate_record propagation = {};  // of the prediction (zeros where none was made: pair 0)
        double share[3] = {-1.0, -1.0, -1.0};  // adaptive mode: the shares of pixels where the final flow and the prediction differ by
                                               // more than 1, 2, 3 px; -1 where nothing was measured
    };
    // fill_passes in [0, FLOW2D_PROPAGATE_MAX_FILL], photo_scale finite and >= 0, tail < 0 or in [0, 1) (prints what is wrong);
    // needs no device
    static bool WarmOptionsOk(const WarmOptions& options);
    // The adaptive rule, from the record of flow2d_flow_error_2d with the prediction as the ground truth (its non-finite pixels are
    // invalid there): count = the pixels compared, above[t - 1] = those further than t px from the prediction, t = 1, 2, 3;
    // share(t) = above[t - 1] / count in double.  reach_used: the reach the pair was seeded with, 0 for an unseeded pair.
    //   *redo        reach_used > 0 and (count == 0 or share(reach_used) > tail): the prior did not hold, the pair is to be computed
    //                again unseeded.
    //   *next_reach  the smallest t in {1, 2, 3} with share(t) <= tail; 0 -- the next pair runs unseeded -- when there is none or
    //                count == 0 (a scene cut).
    // False for a tail outside [0, 1), a reach_used outside 0 .. 3, an above[] that is not descending from count, or a null pointer.
    // Needs no device.
    static bool WarmNextReach(unsigned long long count, const unsigned long long* above, float tail, int reach_used, bool* redo,
                              int* next_reach);
    // flow2d_propagate_flow_2d on planes of the container's size with workspace and record of the object's own (allocated at the
    // first call, regrown when needed): (dev_flow_u, dev_flow_v) carried `step` times along itself into dev_out_u / dev_out_v.
    // dev_mask (optional): 1 where a vector is not to be carried; dev_frame_from / dev_frame_to (optional, both or neither) switch
    // the photometric term on.  record_out (optional): the counts, read back -- the call then synchronises, otherwise it only
    // queues.  Not for lock-step groups.
    bool PropagateFlowDevice(DevicePtr dev_flow_u, DevicePtr dev_flow_v, DevicePtr dev_mask, DevicePtr dev_frame_from,
                             DevicePtr dev_frame_to, float step, const WarmOptions& options, DevicePtr dev_out_u, DevicePtr dev_out_v,
                             flow2d_propagate_record* record_out = nullptr);
    // One pair from the previous pair's flow: (dev_prev_u, dev_prev_v), the flow INTO dev_frame_0 from the frame before it, is
    // propagated into two planes of the object's own and ComputeFlowFromPriorDevice runs from them (bag keys prior_reach /
    // prior_level as there).  dev_prev_mask (optional) as for PropagateFlowDevice; dev_prev_frame (optional): the previous pair's
    // frame 0, which switches the photometric term against dev_frame_0 on.  report_out (optional): mode (seeded), the prior's
    // report and the propagation's record; the call then synchronises, otherwise it only queues.  options.tail is not used.
    bool ComputeFlowFromPreviousDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_prev_u, DevicePtr dev_prev_v,
                                       DevicePtr dev_prev_mask, DevicePtr dev_prev_frame, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                                       OperationParameters& params, const WarmOptions& options, WarmReport* report_out = nullptr);
    // The host-image form (the CLI's --previous-flow): prev_mask and prev_frame may be null.
    void ComputeFlowFromPrevious(Data2D& frame_0, Data2D& frame_1, Data2D& prev_u, Data2D& prev_v, Data2D* prev_mask, Data2D* prev_frame,
                                 Data2D& flow_u, Data2D& flow_v, OperationParameters& params, const WarmOptions& options,
                                 WarmReport* report_out = nullptr);
    // The flows of a sequence, every pair after the first started from its predecessor's flow.  Pair 0 is ComputeFlowSequenceDevice's
    // pair 0; pair k >= 1 runs from PropagateFlowDevice(flow k - 1, frames k - 1 and k) through the sequence cache -- every frame's
    // pyramid levels are built once, those above a pair's start level only when a later pair needs them.  Its bytes are those of
    // ComputeFlowFromPriorDevice on the pair from that prior.
    // Without adaptation (options.tail < 0) every pair k >= 1 is seeded with the bag's prior_reach / prior_level and the call only
    // queues unless reports are asked for.  With options.tail in [0, 1) (one host wait per pair): after pair k its flow is scored
    // against its prediction (flow2d_flow_error_2d) and WarmNextReach decides whether the pair is computed again unseeded into the
    // same planes (mode redone) and with which reach pair k + 1 is seeded, if at all; the first seeded pair uses prior_reach
    // rounded up to 1, 2 or 3 (a larger one, and a prior_level, are refused in this mode).  A prediction is made and scored for an
    // unseeded pair k >= 1 too: that is how a sequence finds back to warm starts after a scene cut.
    // reports (optional): frame_count - 1 entries.  Frames are only read; the flow planes must be distinct from each other and
    // from the frames.  Eager; not for lock-step groups.
    bool ComputeFlowSequenceWarmDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                       const DevicePtr* dev_flows_v, OperationParameters& params, const WarmOptions& options,
                                       WarmReport* reports = nullptr);
    // The host-image form: frames[k] -> frame k, flows_u / flows_v: frame_count - 1 images each.
    void ComputeFlowSequenceWarm(Data2D* const* frames, size_t frame_count, Data2D* flows_u, Data2D* flows_v, OperationParameters& params,
                                 const WarmOptions& options, WarmReport* reports = nullptr);

    // When set, ComputeFlowDevice records the whole pyramid of a pair into a HIP graph the first time it
    // sees a (buffers, parameters) combination and replays it afterwards: one host call instead of
    // several hundred launches.  Ignored while timing_mode != 0 (events are not captured).
    bool use_graph = false;

    // Lock-step groups of independent pairs (set BEFORE Initialize; 1 = off).  Every plane of the pool becomes
    // `group_size` containers tall and ComputeFlowDevice computes group_size pairs at once: pair g of each of the four
    // caller planes lives GroupStrideBytes() * g behind the pointer passed (tall containers, pairs one below the other).
    // Every launch then holds the work of the whole group (flow2d_context_set_batch), so a level of a mid-size frame
    // fills the chip and the launch-bound coarse levels cost one launch per group instead of one per pair; each pair's
    // flow is bit-identical to its own ComputeFlowDevice.  Not available for ComputeFlow (host images) and sequences.
    size_t group_size = 1;
    size_t GroupStrideBytes() const { return dev_container_size_.pitch * dev_container_size_.height; }

    // A lock-step group formed from `count` (1 .. group_size) independent pairs, every plane a container of its own
    // anywhere on the device: the frames are gathered into the object's tall staging containers (one launch,
    // flow2d_copy_planes), the group is computed like a tall-container group of `count` pairs, and the flows are handed
    // back to the callers' planes (one launch).  Queued, not synchronised; with use_graph the whole sequence is recorded
    // per (planes, parameters) combination and replayed.  Each pair's flow is bit-identical to its own ComputeFlowDevice.
    bool ComputeFlowGroupDevice(size_t count, const DevicePtr* dev_frames_0, const DevicePtr* dev_frames_1,
                                const DevicePtr* dev_flows_u, const DevicePtr* dev_flows_v, OperationParameters& params);

    const DataSize3& ContainerSize() const { return dev_container_size_; }
    // Device time of the last ComputeFlow (events around upload..download), milliseconds.
    float LastTotalMs() const { return last_total_ms_; }
    // ComputeFlow is void, like the reference's: whether the last call delivered a flow (false after a missing key,
    // a parameter no level can run with, or a failed operator -- the caller's flow images are then left untouched)
    bool LastRunSucceeded() const { return last_run_ok_; }
    int timing_mode = 0;  // flow2d_timing_enable mode used during a run (0 off, 1 per level, 2 + per kernel launch)
    // One record per level solved since the last ResetLevelTimings() (oldest first); call after the
    // context has been synchronised.  Records accumulate across runs while timing_mode is non-zero.
    std::vector<FlowLevelTiming> LastLevelTimings();
    void ResetLevelTimings();

    bool silent = false;

    // Set BEFORE Initialize.  lone: this object runs its pairs one after the other with nothing else of the same job beside them on
    // the device (the CLI, a lone ComputeFlowDevice user, a batch of one lane) -- latency is what counts, and strip launches that leave
    // half the wave slots empty use the build of the strip kernel with packed arithmetic (flow2d_context_set_lone).
    // OpticalFlowBatch2D clears it for its lanes when there are several: in a pipeline the other lanes' work fills the device.
    bool lone = true;

private:
    // Device planes beside the pool that the object keeps until Destroy(); an entry of 0 is a plane not allocated yet.
    // Constructing one registers it with the object (`owned_`), and Destroy() frees every registered plane in one loop: a new
    // member cannot be forgotten there.
    class OwnedPlanes {
    public:
        explicit OwnedPlanes(std::vector<OwnedPlanes*>& registry, size_t count = 0) : planes_(count, 0) { registry.push_back(this); }
        OwnedPlanes(const OwnedPlanes&) = delete;
        OwnedPlanes& operator=(const OwnedPlanes&) = delete;
        // the array, grown to `count` entries when it has fewer
        DevicePtr* AtLeast(size_t count)
        {
            if (planes_.size() < count) planes_.resize(count, 0);
            return planes_.data();
        }
        DevicePtr& operator[](size_t i) { return planes_[i]; }
        DevicePtr operator[](size_t i) const { return planes_[i]; }
        const DevicePtr* data() const { return planes_.data(); }
        DevicePtr* begin() { return planes_.data(); }
        DevicePtr* end() { return planes_.data() + planes_.size(); }

    private:
        std::vector<DevicePtr> planes_;
    };
    // One device allocation addressed by byte offsets: an entry's record first, its workspace behind it.
    struct DeviceScratch {
        explicit DeviceScratch(std::vector<OwnedPlanes*>& registry) : block(registry, 1) {}
        // At least `bytes`.  Grows only when a call asks for more than there is: the stream is drained (queued work may still use
        // the old block), the old block freed and a new one allocated.
        bool Ensure(flow2d_context* context, size_t bytes);
        template <class T = char>
        T* At(size_t offset = 0) const
        {
            return reinterpret_cast<T*>(static_cast<size_t>(block[0]) + offset);
        }
        OwnedPlanes block;
        size_t bytes = 0;
    };
    std::vector<OwnedPlanes*> owned_;  // (declared before the planes that register with it)

    bool InitMemory();
    bool InitOperations();
    bool RunPyramid(OperationParameters& params);
    bool QueuePair(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                   OperationParameters& params);
    bool QueueScatteredGroup(size_t count, const DevicePtr* dev_frames_0, const DevicePtr* dev_frames_1,
                             const DevicePtr* dev_flows_u, const DevicePtr* dev_flows_v, OperationParameters& params);
    bool ReplayOrRecord(std::vector<unsigned char> key, const std::function<bool()>& queue);
    void DropGraphs();
    DevicePtr Acquire();
    void Release(DevicePtr p);

    static constexpr size_t kContainersCount = 12;  // optical_flow_2d.h:45 of the reference
    DataSize3 dev_container_size_{0, 0, 0};
    size_t group_ = 1;  // group_size as it was at Initialize
    size_t active_group_ = 1;  // pairs of the group being queued (a scattered group may be smaller than group_)
    OwnedPlanes group_staging_{owned_, 4};  // ComputeFlowGroupDevice: tall frame 0, frame 1, flow u, flow v (first use)
    std::vector<DevicePtr> all_planes_;
    std::vector<DevicePtr> free_planes_;
    DevicePtr dev_frame_0_ = 0, dev_frame_1_ = 0, dev_flow_u_ = 0, dev_flow_v_ = 0;  // valid inside a run
    // Two planes beside the pool: the x-resampled rows of all pyramid levels of frame 0 / frame 1, side by side
    // (flow2d_resample_x_levels: one read of each frame for the x passes of the whole pyramid)
    OwnedPlanes packed_frames_{owned_, 2};
    // ComputeFlowDevice only: the caller's planes.  With a pre-blur the frames are read once (by the blur), so
    // they are read in place instead of copied; the last level's median writes the caller's flow planes.
    DevicePtr caller_frame_0_ = 0, caller_frame_1_ = 0, caller_flow_u_ = 0, caller_flow_v_ = 0;
    // ComputeFlowSequenceDevice only: a frame's blurred full-resolution plane (level 0; the caller's own plane when
    // there is no pre-blur) and its resampled levels, kept from one pair to the next.
    struct FramePyramid {
        DevicePtr blurred = 0;             // owned: the pre-blurred frame (allocated on first use)
        DevicePtr level0 = 0;              // what level 0 reads: `blurred`, or the caller's plane without a pre-blur
        std::vector<DevicePtr> levels;     // [l] for l >= 1, container width x level height
        std::vector<size_t> level_rows;
        // Levels 0 .. built - 1 hold the frame (0: nothing does).  A pair builds, from its first level down, what is missing: a pair
        // started from a prior at level s leaves s + 1 levels, and a later pair that starts higher adds the rest.
        size_t built = 0;
    };
    FramePyramid sequence_cache_[2];
    FramePyramid* sequence_frames_[2] = {nullptr, nullptr};  // non-null inside a sequence pair: frame 0 / frame 1
    size_t sequence_levels_run_ = 0;  // RunPyramid's sequence branch: the levels of the pair it ran last (first level + 1)
    DevicePtr SequenceLevelPlane(FramePyramid& pyramid, size_t level, size_t rows);
    void FreeSequenceCache();
    bool PrepareSequenceCache(OperationParameters& params);
    // One pair of a sequence: `first` / `second` are the pyramids of frame_0 / frame_1 (the levels they lack are built here).
    // With prior planes the pair starts from them at start_level (ComputeFlowFromPriorDevice's run, through the cache).
    bool RunSequencePair(FramePyramid& first, FramePyramid& second, DevicePtr frame_0, DevicePtr frame_1, DevicePtr flow_u,
                         DevicePtr flow_v, OperationParameters& params, DevicePtr prior_u = 0, DevicePtr prior_v = 0,
                         size_t start_level = 0);
    // ComputeFlowBidirectional: both frames and the six outputs, outside the pool (allocated on first use)
    OwnedPlanes bidirectional_planes_{owned_, 8};
    // InterpolateFrames*: the flows and masks of a pair (u, v, back u, back v, occlusion 0, occlusion 1) and the host form's
    // output frames, outside the pool (allocated on first use)
    OwnedPlanes interpolation_planes_{owned_, 6};
    OwnedPlanes interpolation_outputs_{owned_};
    // full-size planes where `planes` has none yet (0); the second form grows the array to `count` entries first
    bool EnsurePlanes(DevicePtr* planes, size_t count);
    bool EnsurePlanes(OwnedPlanes& planes, size_t count) { return EnsurePlanes(planes.AtLeast(count), count); }
    // "... and lock-step groups do not combine": prints that and returns true for an object initialised with a group size > 1
    bool RefuseGroup(const char* what) const;
    // `bytes` from device memory into host memory, queued on the stream
    bool ReadRecord(void* host, const void* device, size_t bytes);
    // `count` (1 or 2) planes src[i] -> dst[i] with one launch; nothing when the caller gave no planes to fill (dst[0] == 0)
    bool HandBack(size_t count, const DevicePtr* src, const DevicePtr* dst);
    bool InterpolationArgsOk(const float* times, size_t time_count, int iterations, float max_residual);
    // the flow2d_interpolate_2d launches of one pair: flows = u, v, back u, back v, occlusion 0, occlusion 1 (masks unused when
    // !use_masks)
    bool QueueInterpolation(DevicePtr frame_0, DevicePtr frame_1, const DevicePtr* flows, bool use_masks, const float* times,
                            size_t time_count, const DevicePtr* outputs, int iterations, float max_residual);
    // TrackPointsDevice: the flows of a window (u, v, back u, back v per pair) and, in one allocation, the device count and the
    // seeding workspace (allocated on first use, the scratch regrown when a call needs more)
    OwnedPlanes tracking_flows_{owned_};
    DeviceScratch tracking_scratch_{owned_};
    // DenoiseSequenceDevice: the ring of pairs (u, v, back u, back v, occlusion forward, occlusion backward per slot; the masks
    // allocated on the first call with use_masks) and the composed flows of a centre (u, v, mask per direction and distance >= 2)
    OwnedPlanes denoise_pairs_{owned_, 6 * (2 * kDenoiseMaxRadius + kDenoiseWindow)};
    OwnedPlanes denoise_chains_{owned_, 2 * (kDenoiseMaxRadius - 1) * 3};
    // EstimateGlobalMotion* / StabiliseSequence*: the flows of a window (u, v, back u, back v, occlusion forward, occlusion
    // backward per pair; allocated as needed) and, in one allocation, kStabiliseWindow + 1 records and the fit's workspace
    OwnedPlanes stabilise_planes_{owned_, 6 * kStabiliseWindow};
    DeviceScratch stabilise_scratch_{owned_};
    bool EnsureStabiliseScratch();
    flow2d_global_motion* StabiliseRecord(size_t slot) const { return stabilise_scratch_.At<flow2d_global_motion>() + slot; }
    // the records of the flows frames[i] -> frames[i + 1], i < count - 1, of an ordered list of frames into records[i]
    bool FitConsecutivePairs(const DevicePtr* frames, size_t count, int model, double sigma, int iterations, bool use_masks,
                             flow2d_global_motion* records, OperationParameters& params);
    // SegmentMotion*: residual u, residual v and labels, and in one allocation the summary, kSegmentMaxRegions records and the
    // workspace (allocated on first use)
    OwnedPlanes segment_planes_{owned_, 3};
    DeviceScratch segment_scratch_{owned_};
    // AnalyseDeformation*: the pair's flow (u, v, back u, back v, occlusion forward, occlusion backward; the last four with
    // use_masks only), the smoothed flow (u, v; with a sigma only) and, in one allocation, the record and the workspace
    OwnedPlanes deformation_planes_{owned_, 8};
    DeviceScratch deformation_scratch_{owned_};
    // RefineFlow*: the pair's flow (u, v, back u, back v, occlusion forward, occlusion backward; the last four with use_masks
    // only), the two ping-pong pairs of the passes before the last (from the second and the third iteration on) and the record
    OwnedPlanes refine_planes_{owned_, 10};
    DeviceScratch refine_scratch_{owned_};
    // Correlate*: the node planes the caller did not give (u, v) and the record
    OwnedPlanes correlation_planes_{owned_, 2};
    DeviceScratch correlation_scratch_{owned_};
    // CorrelateMultiPass*: a pass's raw nodes (u, v), its validated nodes (u, v), the predictor (u, v); the passes' records
    OwnedPlanes multipass_planes_{owned_, 6};
    DeviceScratch multipass_scratch_{owned_};
    // CorrelateMultiPassDevice, whose synchronisation CorrelateSubsetDevice leaves out (it goes on on the same stream)
    bool QueueCorrelationPasses(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, const CorrelationPass* passes,
                                size_t count, float min_score, const ValidationOptions& validation, DevicePtr dev_predictor_u,
                                DevicePtr dev_predictor_v, DevicePtr dev_node_u, DevicePtr dev_node_v, DevicePtr dev_node_score,
                                CorrelationPassReport* reports_out, DevicePtr dev_flow_u, DevicePtr dev_flow_v, bool synchronise);
    // RefineNodes* / CorrelateSubset*: the chain's nodes (u, v), the refined ones where the caller gave none (u, v); the record
    OwnedPlanes subset_planes_{owned_, 4};
    // SubsetOptions::BSpline: the coefficients of the frame 1 of the call under way (first use)
    OwnedPlanes spline_plane_{owned_, 1};
    DeviceScratch subset_scratch_{owned_};
    // RefineNodesDevice without its synchronisation; *refined gets the planes (u, v) that were written
    // start_gradients (optional): ux0, uy0, vx0, vy0 of flow2d_subset_refine_from_2d
    bool QueueRefineNodes(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_node_u0, DevicePtr dev_node_v0, int grid_radius,
                          int spacing, const SubsetOptions& subset, const SubsetPlanes& out, flow2d_subset_record* record_out,
                          DevicePtr* refined, const DevicePtr* start_gradients = nullptr);
    // CorrelateSubsetDevice, whose synchronisation CorrelateSubsetSequenceDevice leaves out
    bool QueueCorrelateSubset(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, const CorrelationPass* passes,
                              size_t count, float min_score, const ValidationOptions& validation, const SubsetOptions& subset,
                              DevicePtr dev_predictor_u, DevicePtr dev_predictor_v, const SubsetPlanes& out,
                              CorrelationPassReport* reports_out, flow2d_subset_record* record_out, DevicePtr dev_flow_u,
                              DevicePtr dev_flow_v, bool synchronise);
    // one step after the first, queued: the prediction's passes, the refinement from them, the expansion; the step's device
    // records lie at scratch_offset of sequence_scratch_
    bool QueueSequenceStep(DevicePtr dev_frame_0, DevicePtr dev_frame_k, const SubsetPlanes& last, int grid_radius, int spacing,
                           const SubsetOptions& subset, const SequenceOptions& sequence, const SubsetPlanes& out,
                           SequenceStepReport* report_out, size_t scratch_offset, DevicePtr dev_flow_u, DevicePtr dev_flow_v);
    // CorrelateSubsetSequence*: the prediction's two sets of seven planes (u, v, ux, uy, vx, vy, state); the passes' records
    OwnedPlanes sequence_planes_{owned_, 14};
    DeviceScratch sequence_scratch_{owned_};
    // ... with a moving reference (first use): two sets of eight planes for the increments (u, v, ux, uy, vx, vy, score, state),
    // written in turn, and the base's seven (u, v, ux, uy, vx, vy, state)
    OwnedPlanes reference_planes_{owned_, 23};
    // the composition alone, without the checks of the plane sets and without a synchronisation; `record`: device, optional
    bool QueueComposeNodes(const SubsetPlanes& base, const SubsetPlanes& increment, int grid_radius, int spacing, int min_state,
                           const SubsetPlanes& out, flow2d_compose_record* record);
    // ComposeNodesDevice: its record
    DeviceScratch compose_scratch_{owned_};
    // NodeUncertaintyDevice: its record
    DeviceScratch uncertainty_scratch_{owned_};
    // NodeStrain*: per step the record and, behind it, the workspace
    DeviceScratch strain_scratch_{owned_};
    // ComputeFlowFromPrior*: inside such a run the prior's planes and the start level (RunPyramid starts there, from them); the
    // device count of the prior's non-finite pixels; the expanded field of ComputeFlowCorrelationSeeded* (u, v; first use)
    DevicePtr prior_u_ = 0, prior_v_ = 0;
    size_t prior_start_level_ = 0;
    DeviceScratch prior_scratch_{owned_};
    OwnedPlanes prior_planes_{owned_, 2};
    // Warm starts: the propagated flow (u, v) and, in one allocation, the propagation's record, the record of the score, and the
    // workspaces of both (WarmScratch)
    OwnedPlanes warm_planes_{owned_, 2};
    DeviceScratch warm_scratch_{owned_};
    struct WarmScratch {
        flow2d_propagate_record* record;
        flow2d_flow_error_stats* stats;
        void* propagate_workspace;
        void* error_workspace;
        size_t error_workspace_bytes;
    };
    bool EnsureWarmScratch(WarmScratch& scratch);
    bool QueuePropagation(DevicePtr flow_u, DevicePtr flow_v, DevicePtr mask, DevicePtr frame_from, DevicePtr frame_to, float step,
                          const WarmOptions& options, DevicePtr out_u, DevicePtr out_v, const WarmScratch& scratch);
    // whether [plane, plane + one container of the group) meets a plane of the object's own
    bool MeetsOwnPlane(DevicePtr plane) const;
    flow2d_context* context_ = nullptr;
    // One plane beside the pool: the warped frame of a level, when the levels of both frames are computed up front into plane
    // regions of their own (RunPyramid: "stacked" levels) and therefore cannot be overwritten by the warp
    OwnedPlanes level_warp_plane_{owned_, 1};
    float last_total_ms_ = 0.f;
    bool last_run_ok_ = false;
    // recorded pyramids, keyed by the caller buffers and parameters they were recorded for
    struct RecordedGraph {
        void* exec = nullptr;
        unsigned long long last_use = 0;
    };
    std::map<std::vector<unsigned char>, RecordedGraph> graphs_;
    unsigned long long graph_clock_ = 0;
    static constexpr size_t kMaxGraphs = 32;

    CudaOperationAdd2D cuop_add_;
    CudaOperationConvolution2D cuop_convolution_;
    CudaOperationMedian2D cuop_median_;
    CudaOperationRegistration2D cuop_register_;
    CudaOperationResample2D cuop_resample_;
    CudaOperationSolve2D cuop_solve_;
};
